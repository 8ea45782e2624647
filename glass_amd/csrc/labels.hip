// K4b: the labels of one subgraph batch for a replayed training step.
// reference: utils.MaxZOZ (impl/utils.py:32-45: z = 0; z[pos[pos >= 0]] = 1) and the batch hand-over of
// ZGDataloader (impl/SubGDataset.py:75-96).
//
// One launch per step, ONE workgroup (the work is a few thousand entries; what it costs is its chain of dependent
// round trips, not bandwidth):
//   * the batch (pos, target) is copied into the step's fixed buffers (what glass_copy_pair did);
//   * the label bytes are maintained INCREMENTALLY: the nodes the previous batch named are cleared, the new ones set
//     — no pass over the N bytes (incremental == 0: the N bytes are zero-filled here first);
//   * the UNIQUE labeled rows are listed in first-occurrence order (lab_rows, lab_count): the entry with the lowest
//     index naming a node owns it (integer atomicMin on a scratch word per named node: the result does not depend on
//     the order of the atomics), owners are compacted in entry order by ballots — deterministic.  The scratch words hold
//     INT32_MAX between calls (the caller fills them once, every call restores the words it touched), so setting the
//     label bytes and the atomicMin share a phase: three dependent round trips instead of four (6.7 -> 5.4 us).
// The list is what lets the comb pair of GLASSConv run ONE product per row (effective per-label weights, dense.hip):
// every row tile multiplies the unlabeled-row weight, the listed rows are recomputed with the labeled-row weight by a
// few extra workgroups of the same launch.
#include "common.h"
#include "labels_body.h"



using namespace glass;

extern "C" int64_t glass_batch_labels_ws_bytes(int64_t n_nodes) {
    return n_nodes > 0 ? n_nodes * (int64_t)sizeof(int32_t) : GLASS_E_ARG;
}

extern "C" int glass_batch_labels(const int64_t* pos_src, int64_t n_pos, int64_t* pos_dst, const void* y_src, void* y_dst,
                                  int64_t y_bytes, uint8_t* mask, int32_t* lab_rows, int32_t* lab_count, void* ws,
                                  int64_t n_nodes, int incremental, void* stream) {
    GLASS_REQUIRE(pos_src && mask && lab_rows && lab_count && ws, "batch_labels: null pointer");
    GLASS_REQUIRE(n_pos > 0 && n_pos < (1ll << 30) && n_nodes > 0 && n_nodes < (1ll << 31), "batch_labels: bad sizes");
    GLASS_REQUIRE(y_bytes == 0 || (y_src && y_dst && y_bytes > 0 && y_bytes % 4 == 0 &&
                                   ((reinterpret_cast<uintptr_t>(y_src) | reinterpret_cast<uintptr_t>(y_dst)) & 3u) == 0),
                  "batch_labels: the target copy has 4-byte granularity");
    const BatchSrc src{pos_src, (const uint32_t*)y_src, nullptr, 1, 1, 0};
    hipLaunchKernelGGL(batch_labels_kernel<false>, dim3(1), dim3(kLabThreads), 0, (hipStream_t)stream, src, (int)n_pos, pos_dst,
                       (uint32_t*)y_dst, y_bytes / 4, mask, lab_rows, lab_count, (int32_t*)ws, n_nodes, incremental);
    return launch_status("glass_batch_labels");
}

extern "C" int glass_batch_labels_gather(const int64_t* pos_all, int64_t n_all, int64_t smax, const void* y_all,
                                         int64_t y_row_bytes, const int64_t* idx, int64_t n_idx, int64_t* pos_dst, void* y_dst,
                                         uint8_t* mask, int32_t* lab_rows, int32_t* lab_count, void* ws, int64_t n_nodes,
                                         int incremental, void* stream) {
    GLASS_REQUIRE(pos_all && idx && mask && lab_rows && lab_count && ws, "batch_labels_gather: null pointer");
    GLASS_REQUIRE(n_all > 0 && smax > 0 && n_idx > 0 && n_idx * smax < (1ll << 30) && smax < (1ll << 30) && n_nodes > 0 &&
                      n_nodes < (1ll << 31),
                  "batch_labels_gather: bad sizes");
    GLASS_REQUIRE(y_row_bytes == 0 || (y_all && y_dst && y_row_bytes > 0 && y_row_bytes % 4 == 0 && y_row_bytes < (1ll << 30) &&
                                       ((reinterpret_cast<uintptr_t>(y_all) | reinterpret_cast<uintptr_t>(y_dst)) & 3u) == 0),
                  "batch_labels_gather: the target rows have 4-byte granularity");
    const BatchSrc src{pos_all, (const uint32_t*)y_all, idx, (int)smax, y_row_bytes ? (int)(y_row_bytes / 4) : 1, n_all};
    hipLaunchKernelGGL(batch_labels_kernel<true>, dim3(1), dim3(kLabThreads), 0, (hipStream_t)stream, src, (int)(n_idx * smax),
                       pos_dst, (uint32_t*)y_dst, n_idx * (y_row_bytes / 4), mask, lab_rows, lab_count, (int32_t*)ws, n_nodes,
                       incremental);
    return launch_status("glass_batch_labels_gather");
}

// ---- the epoch plan: the unique labeled rows of EVERY batch of an epoch, once (labels_body.h) --------------------------
// One workgroup per lane of owner words; lane g takes batches g, g + lanes, ... of the epoch, one after the other.
namespace glass {
__global__ __launch_bounds__(kLabThreads) void epoch_plan_kernel(const int64_t* __restrict__ pos_all, int64_t n_all, int smax,
                                                                 const int64_t* __restrict__ idx, int n_batches, int n_idx,
                                                                 int32_t* __restrict__ plan, int32_t* __restrict__ owner,
                                                                 int64_t N) {
    const int n_pos = n_idx * smax;
    const int64_t stride = epoch_plan_stride(n_pos);
    for (int b = blockIdx.x; b < n_batches; b += gridDim.x) {
        const BatchSrc src{pos_all, nullptr, idx + (int64_t)b * n_idx, smax, 1, n_all};
        int32_t* rec = plan + b * stride;
        unique_rows_body<true>(src, n_pos, rec + kPlanHead, rec, owner + (int64_t)blockIdx.x * N, N);
    }
}
}  // namespace glass

extern "C" int64_t glass_epoch_plan_bytes(int64_t n_batches, int64_t n_idx, int64_t smax) {
    if (n_batches <= 0 || n_idx <= 0 || smax <= 0 || n_idx * smax >= (1ll << 30) || n_batches >= (1ll << 31)) return GLASS_E_ARG;
    return n_batches * epoch_plan_stride(n_idx * smax) * (int64_t)sizeof(int32_t);
}

extern "C" int glass_epoch_plan_build(const int64_t* pos_all, int64_t n_all, int64_t smax, const int64_t* idx,
                                      int64_t n_batches, int64_t n_idx, int64_t n_nodes, int32_t* plan, int64_t plan_bytes,
                                      void* ws, int64_t ws_lanes, void* stream) {
    GLASS_REQUIRE(pos_all && idx && plan && ws, "epoch_plan_build: null pointer");
    GLASS_REQUIRE(n_all > 0 && smax > 0 && n_idx > 0 && n_idx * smax < (1ll << 30) && smax < (1ll << 30) && n_batches > 0 &&
                      n_batches < (1ll << 31) && n_nodes > 0 && n_nodes < (1ll << 31) && ws_lanes > 0 && ws_lanes <= 1024,
                  "epoch_plan_build: bad sizes");
    GLASS_REQUIRE(plan_bytes >= glass_epoch_plan_bytes(n_batches, n_idx, smax) && (reinterpret_cast<uintptr_t>(plan) & 15u) == 0,
                  "epoch_plan_build: the plan needs %lld bytes (glass_epoch_plan_bytes), 16-B aligned",
                  (long long)glass_epoch_plan_bytes(n_batches, n_idx, smax));
    const unsigned lanes = (unsigned)(ws_lanes < n_batches ? ws_lanes : n_batches);
    hipLaunchKernelGGL(epoch_plan_kernel, dim3(lanes), dim3(kLabThreads), 0, (hipStream_t)stream, pos_all, n_all, (int)smax, idx,
                       (int)n_batches, (int)n_idx, plan, (int32_t*)ws, n_nodes);
    return launch_status("glass_epoch_plan_build");
}
