// K1: CSR aggregation Y = A @ X for gfx950.   Replaces `self.adj @ x` (reference
// impl/models.py:164) and, on the CSR of A^T, its autograd backward.
//
// Shape of the work: per edge one gather of a 4H-byte feature row (256 B at H=64) — HBM/L2
// bound, no matrix-core work.  Layout per wave64: a feature row is covered by LPR lanes x 16 B
// (LPR=16 at H=64), so one wave-instruction gathers G = 64/LPR neighbour rows = 1 KiB, fully
// coalesced per row.  A wave first reads up to 64 (col,val) pairs of its row coalesced, then
// hands them to the lane groups with ds_bpermute (__shfl) — one dependent latency per 64 edges —
// and keeps U gathers in flight.  Partial sums of the G groups are combined with __shfl_xor;
// rows long enough to need a whole workgroup are combined through LDS; rows longer than one
// chunk go through per-chunk partial rows summed in fixed order (no float atomics).
#include "common.h"
#include "spmm_common.h"

#include <stdint.h>
#include <stdlib.h>
#include <vector>

namespace glass {

// stand-alone form: matrices that are ALL long rows (the selection matrix of the embedding backward)
template <int VW, int LPR, int U, bool NT>
__global__ __launch_bounds__(kBlock) void spmm_long_kernel(const int32_t* __restrict__ col,
                                                           const float* __restrict__ val,
                                                           const float* __restrict__ X, int64_t ldx,
                                                           float* __restrict__ Y, int64_t ldy,
                                                           float* __restrict__ partials, int H,
                                                           const int32_t* __restrict__ items) {
    __shared__ float lds[(kBlock / kWave) * LPR * VW];
    long_item_body<VW, LPR, U, NT>(col, val, X, ldx, Y, ldy, partials, H, items + 4 * (int64_t)blockIdx.x, lds);
}

#ifdef GLASS_K1_TRACE  // laboratory build only (tools/Makefile `lab`): per-wave wall-clock stamps of the sweep kernel
__device__ unsigned long long* g_k1_trace;
#define K1_STAMP(slot) do { if (g_k1_trace && lane == 0 && blockIdx.y == 0) g_k1_trace[(size_t)wave * 4 + (slot)] = wall_clock64(); } while (0)
#else
#define K1_STAMP(slot) do { } while (0)
#endif

}  // namespace glass

#include "spmm_sweep.h"  // the sweep kernel's body and constants (after K1_STAMP)

namespace glass {

template <int VW, int LPR, int U, bool NT, bool FLAT>
__global__ GLASS_K1_SWEEP_BOUNDS void spmm_sweep_kernel(const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ col,
                                                            const float* __restrict__ val,
                                                            const float* __restrict__ X, int64_t ldx,
                                                            float* __restrict__ Y, int64_t ldy, int H,
                                                            const int32_t* __restrict__ items, int n_waves,
                                                            int rp_factor, const int32_t* __restrict__ long_items,
                                                            int n_sweep_blocks, float* __restrict__ partials) {
    spmm_sweep_body<VW, LPR, U, NT, FLAT>(rowptr, col, val, X, ldx, Y, ldy, H, items, n_waves, rp_factor, long_items,
                                          n_sweep_blocks, partials);
}

// ---- reduce kernel: rows cut into several chunks: sum their partial rows in slot order --------
__global__ __launch_bounds__(kBlock) void spmm_reduce_kernel(const float* __restrict__ partials, float* __restrict__ Y,
                                                             int64_t ldy, int H, const int32_t* __restrict__ rrows) {
    spmm_reduce_body(partials, Y, ldy, H, rrows);
}

template <int VW, int LPR, int U, bool NT>
static int launch_spmm_u(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                       float* Y, int64_t ldy, int64_t H, const int32_t* hdr, const int32_t* plan, float* ws,
                       hipStream_t st) {
    const int n_ctiles = (int)ceil_div(H, (int64_t)LPR * VW);
    const int n_waves = hdr[H_NSWEEP];
    if (n_waves > 0) {
        const int n_sweep_blocks = (int)ceil_div(n_waves, kBlock / kWave);
        dim3 grid((unsigned)(n_sweep_blocks + hdr[H_NLONG]), n_ctiles);  // sweep workgroups, then one per long-row item
        if (spmm_sweep_flat(hdr, kWave / LPR))
            hipLaunchKernelGGL((spmm_sweep_kernel<VW, LPR, U, NT, true>), grid, dim3(kBlock), 0, st, rowptr, col, val, X, ldx,
                               Y, ldy, (int)H, plan + hdr[H_OFF_SWEEP], n_waves, hdr[H_RP_FACTOR], plan + hdr[H_OFF_LONG],
                               n_sweep_blocks, ws);
        else
            hipLaunchKernelGGL((spmm_sweep_kernel<VW, LPR, U, NT, false>), grid, dim3(kBlock), 0, st, rowptr, col, val, X, ldx,
                               Y, ldy, (int)H, plan + hdr[H_OFF_SWEEP], n_waves, 0, plan + hdr[H_OFF_LONG], n_sweep_blocks, ws);
    } else if (hdr[H_NLONG] > 0) {
        dim3 grid((unsigned)hdr[H_NLONG], n_ctiles);
        hipLaunchKernelGGL((spmm_long_kernel<VW, LPR, U, NT>), grid, dim3(kBlock), 0, st, col, val, X, ldx, Y, ldy, ws,
                           (int)H, plan + hdr[H_OFF_LONG]);
    }
    if (hdr[H_NREDUCE] > 0) {
        hipLaunchKernelGGL(spmm_reduce_kernel, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, ws, Y, ldy, (int)H,
                           plan + hdr[H_OFF_REDUCE]);
    }
    return launch_status("glass_spmm_csr_f32");
}

template <int VW, int LPR>
static int launch_spmm(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                       float* Y, int64_t ldy, int64_t H, const int32_t* hdr, const int32_t* plan, float* ws,
                       hipStream_t st) {
    // gathers in flight per lane group: measured us/launch for U = 2 / 4 / 8 on MI355X — ppi_bp-shape
    // 14.9 / 13.2 / 12.7, hpo_neuro-shape 87.8 / 83.4 / 81.0, power-law H=256 2638 / 2600 / 2597.
    // streamed bytes of this launch (indices in, Y out) beyond what the Infinity Cache holds -> non-temporal streams
    const int64_t streamed = (int64_t)hdr[H_NNZ] * 8 + (int64_t)hdr[H_NROWS] * (4 * H + 4);
    if (streamed > kStreamNtBytes) return launch_spmm_u<VW, LPR, kGathers, true>(rowptr, col, val, X, ldx, Y, ldy, H, hdr, plan, ws, st);
    return launch_spmm_u<VW, LPR, kGathers, false>(rowptr, col, val, X, ldx, Y, ldy, H, hdr, plan, ws, st);
}

}  // namespace glass

using namespace glass;

#ifdef GLASS_K1_TRACE
extern "C" int glass_k1_trace_set(unsigned long long* p) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_k1_trace), &p, sizeof(p));
}
#endif

// Plan policy (host).  Rows with >= kLongThr edges are given to whole workgroups in chunks of
// kLongChunk edges; the rest are swept by waves holding ~edges_per_wave edges each.
// Matrices with few, long rows (the transposed one-hot selection matrix of the embedding backward:
// V ~ 50 rows holding N entries) would keep most of the chip idle under that policy (47 workgroups,
// 26 us at ppi_bp-shape), so when the whole matrix yields fewer than ~1024 chunks the threshold and
// the chunk shrink until it does (never below one 64-edge batch per wave).  Such matrices (<= 1024 rows averaging
// >= 64 entries) also skip the sweep kernel altogether: EVERY row becomes workgroup items (an empty row one empty
// item that stores zeros), so the product is two launches (items + reduce) instead of three.
#ifndef GLASS_K1_SMALL_COST
#define GLASS_K1_SMALL_COST (2ll << 20)   // edges + 4 per row: below this a product is latency-bound (plan policy)
#endif
#ifndef GLASS_K1_LONG_THR
#define GLASS_K1_LONG_THR 256
#endif
static constexpr int kLongThrMax = GLASS_K1_LONG_THR;
static constexpr int kLongChunkMax = 2048;
static constexpr int kRowCost = 4;        // per-row overhead in edge units (rowptr read, reduce, store)
#ifndef GLASS_K1_TARGET_WAVES
#define GLASS_K1_TARGET_WAVES 32768
#endif
static constexpr int kTargetWaves = GLASS_K1_TARGET_WAVES;  // ~4 rounds of 256 CUs x 32 waves
static constexpr int kMinBudget = 16;        // smallest item budget: on small graphs one degree-12 row per wave (density-shape: 5.0 -> 4.0 us; 32 packed two)
static constexpr int kFlatFactor = 4;       // flat mode up to a mean degree of 4 G (uniform degree 12 at H = 64: 988 -> 931 us; degree 37: row mode)

extern "C" int glass_spmm_plan_build(const int32_t* rowptr, int64_t n_rows, int32_t* plan, int64_t* plan_words) {
    GLASS_REQUIRE(rowptr && plan_words && n_rows >= 0 && n_rows < (1ll << 31), "plan_build: bad arguments");
    const int64_t nnz = rowptr[n_rows];
    GLASS_REQUIRE(rowptr[0] == 0 && nnz >= 0, "plan_build: rowptr[0] must be 0 and nnz < 2^31");
    std::vector<int32_t> sweep, longs, reduces;
    int kLongThr = kLongThrMax, kLongChunk = kLongChunkMax;
    while (kLongChunk > 256) {
        int64_t items = 0;
        for (int64_t r = 0; r < n_rows; ++r) {
            const int64_t d = (int64_t)rowptr[r + 1] - rowptr[r];
            if (d >= kLongThr) items += ceil_div(d, kLongChunk);
        }
        if (items + n_rows >= 1024) break;  // enough independent work items
        kLongChunk /= 2;
        if (kLongThr > 64) kLongThr /= 2;
    }
    // Small products (a few generations of resident waves at most) are latency-bound: the launch lasts as long as its
    // longest wave, and a wave walks d edges in d/32 dependent rounds.  There a row of >= 64 edges is worth a workgroup
    // (4 waves share it; the long-row items ride in the sweep launch, so they cost no launch of their own) and a chunk
    // is 512 edges (2 batches per wave; longer rows pay the reduce launch instead of a 16-round chain).  Measured,
    // us per product at H = 64 (2048-edge chunks / threshold 256 -> this): shipped density graph 12.8 -> 6.1; N = 4 998
    // Zipf 0.8 19.4 -> 8.1; N = 17 080, 634 k edges, Zipf 0.5 31.6 -> 16.3; N = 14 587, 1.2 M edges, Zipf 0.7 35.2 -> 24.7.
    // Throughput-bound products keep the large chunks (hpo_neuro-shape, 6.5 M edges: 75.8 vs 77.8 with 512).
    if (nnz + 4 * n_rows <= GLASS_K1_SMALL_COST) {
        if (kLongThr > 64) kLongThr = 64;
        if (kLongChunk > 512) kLongChunk = 512;
    }
    const bool all_long = n_rows > 0 && n_rows <= 1024 && nnz >= 64 * n_rows;
    if (all_long) kLongThr = 0;
    int64_t cost_total = 0;
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t d = (int64_t)rowptr[r + 1] - rowptr[r];
        GLASS_REQUIRE(d >= 0, "plan_build: rowptr not monotone at row %lld", (long long)r);
        cost_total += kRowCost + (d < kLongThr ? d : 0);
    }
    int64_t budget = cost_total / kTargetWaves;
    if (budget < kMinBudget) budget = kMinBudget;
    if (budget > 1024) budget = 1024;
    // Sweep items (r0, r1, e0, e1): maximal runs of consecutive SHORT rows under three caps — the cost budget (balance),
    // kItemRows rows and kItemEdges edges (what the kernel stages per wave).  Long rows belong to the workgroup kernel
    // and end the current item, so an item never contains one.
    int64_t acc = 0, it_r0 = 0, it_edges = 0;
    int32_t n_slots = 0;
    bool open = false;
    int64_t min_item_deg = INT32_MAX;  // min over sweep items of ceil(edges / rows)
    int64_t flat_cost[7] = {0, 0, 0, 0, 0, 0, 0}, sweep_cost = 0;  // cost in items flat-eligible at G = 1, 2, 4, .. 64 lane groups
    auto close_item = [&](int64_t r_end) {
        if (!open) return;
        const int64_t e = (int64_t)rowptr[r_end] - rowptr[it_r0], nr = r_end - it_r0;
        const int64_t md = ceil_div(e, nr);
        if (md < min_item_deg) min_item_deg = md;
        const int64_t cost = e + kRowCost * nr;
        sweep_cost += cost;
        for (int k = 0; k < 7; ++k)
            if (e <= (int64_t)kFlatFactor * (1 << k) * nr) flat_cost[k] += cost;  // the kernel's flat-mode test
        sweep.push_back((int32_t)it_r0);
        sweep.push_back((int32_t)r_end);
        sweep.push_back(rowptr[it_r0]);
        sweep.push_back(rowptr[r_end]);
        open = false;
    };
    for (int64_t r = 0; r < n_rows; ++r) {
        const int64_t d = (int64_t)rowptr[r + 1] - rowptr[r];
        if (d < kLongThr) {
            const int64_t c = kRowCost + d;
            if (open && (acc + c > budget || r - it_r0 >= kItemRows || it_edges + d > kItemEdges)) close_item(r);
            if (!open) {
                open = true;
                it_r0 = r;
                acc = it_edges = 0;
            }
            acc += c;
            it_edges += d;
        } else {
            close_item(r);
            const int64_t n_chunks = d > 0 ? ceil_div(d, kLongChunk) : 1;
            const int64_t per = ceil_div(ceil_div(d, n_chunks), kWave) * kWave;  // even chunks, whole batches
            if (n_chunks > 1) {
                reduces.push_back((int32_t)r);
                reduces.push_back(n_slots);
                reduces.push_back((int32_t)n_chunks);
            }
            for (int64_t k = 0; k < n_chunks; ++k) {
                const int64_t b = rowptr[r] + k * per;
                const int64_t e = (b + per < rowptr[r + 1]) ? b + per : rowptr[r + 1];
                longs.push_back((int32_t)r);
                longs.push_back((int32_t)b);
                longs.push_back((int32_t)e);
                longs.push_back(n_chunks > 1 ? n_slots++ : -1);
            }
        }
    }
    close_item(n_rows);
    const int64_t n_sweep = (int64_t)sweep.size() / 4;
    const int64_t off_sweep = GLASS_PLAN_HEADER_WORDS;
    const int64_t off_long = off_sweep + (int64_t)sweep.size();
    const int64_t off_reduce = off_long + (int64_t)longs.size();
    const int64_t total = off_reduce + (int64_t)reduces.size();
    *plan_words = total;
    if (!plan) return 0;
    for (int i = 0; i < GLASS_PLAN_HEADER_WORDS; ++i) plan[i] = 0;
    plan[H_MAGIC] = kPlanMagic;
    plan[H_VER] = kPlanVersion;
    plan[H_NROWS] = (int32_t)n_rows;
    plan[H_NNZ] = (int32_t)nnz;
    plan[H_NSWEEP] = (int32_t)n_sweep;
    plan[H_NLONG] = (int32_t)(longs.size() / 4);
    plan[H_NREDUCE] = (int32_t)(reduces.size() / 3);
    plan[H_NSLOTS] = n_slots;
    plan[H_LONG_THR] = kLongThr;
    plan[H_LONG_CHUNK] = kLongChunk;
    // Flat-mode threshold (mean degree of an item's rows <= factor * G, G = lane groups per wave at the launch's H).
    plan[H_RP_FACTOR] = kFlatFactor;
    plan[H_MIN_ITEM_DEG] = (int32_t)min_item_deg;
    int32_t shares = 0;  // 7 nibbles: floor(15 * share) of the sweep cost that is flat-eligible at G = 2^k
    for (int k = 0; k < 7; ++k) shares |= (int32_t)(sweep_cost > 0 ? 15 * flat_cost[k] / sweep_cost : 0) << (4 * k);
    plan[H_FLAT_SHARE] = shares;
    plan[H_OFF_SWEEP] = (int32_t)off_sweep;
    plan[H_OFF_LONG] = (int32_t)off_long;
    plan[H_OFF_REDUCE] = (int32_t)off_reduce;
    for (size_t i = 0; i < sweep.size(); ++i) plan[off_sweep + i] = sweep[i];
    for (size_t i = 0; i < longs.size(); ++i) plan[off_long + i] = longs[i];
    for (size_t i = 0; i < reduces.size(); ++i) plan[off_reduce + i] = reduces[i];
    return 0;
}

// the plan's reduce step on its own (for callers that ran the items in another launch: linear.hip)
extern "C" int glass_spmm_reduce_rows_f32(const float* partials, float* Y, int64_t ldy, int64_t H, const int32_t* reduce_rows_dev,
                                          int64_t n_reduce, void* stream) {
    GLASS_REQUIRE(partials && Y && reduce_rows_dev && n_reduce > 0 && H > 0 && ldy >= H, "spmm_reduce_rows: bad arguments");
    hipLaunchKernelGGL(spmm_reduce_kernel, dim3((unsigned)n_reduce), dim3(kBlock), 0, (hipStream_t)stream, partials, Y, ldy,
                       (int)H, reduce_rows_dev);
    return launch_status("glass_spmm_reduce_rows_f32");
}

extern "C" int64_t glass_spmm_ws_bytes(const int32_t* hdr, int64_t H) {
    if (!hdr || hdr[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    return (int64_t)hdr[H_NSLOTS] * H * (int64_t)sizeof(float);
}

extern "C" int glass_spmm_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X,
                                  int64_t ldx, float* Y, int64_t ldy, int64_t n_rows, int64_t H, const int32_t* hdr,
                                  const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && Y && hdr && plan_dev, "spmm: null pointer");
    GLASS_REQUIRE(H > 0 && ldx >= H && ldy >= H, "spmm: need H>0, ldx>=H, ldy>=H (H=%lld ldx=%lld ldy=%lld)",
                  (long long)H, (long long)ldx, (long long)ldy);
    if (hdr[H_MAGIC] != kPlanMagic || hdr[H_VER] != kPlanVersion || hdr[H_NROWS] != n_rows) {
        set_error("spmm: plan does not match (magic %x, rows %d vs %lld)", hdr[H_MAGIC], hdr[H_NROWS],
                  (long long)n_rows);
        return GLASS_E_PLAN;
    }
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val), "spmm: null col/val");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* wsf = (float*)ws;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && aligned16(X) && aligned16(Y) &&
                     (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_SPMM_CASE(VW, LPR) \
    return launch_spmm<VW, LPR>(rowptr, col, val, X, ldx, Y, ldy, H, hdr, plan_dev, wsf, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_SPMM_CASE);
#undef GLASS_SPMM_CASE
}
