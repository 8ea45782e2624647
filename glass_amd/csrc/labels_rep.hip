// K4r: exact zero-one labels for a batch (utils.ZeroOneZ as label bytes): mask[r * N + n] = 1 iff node n occurs in row
// rep0 + r of the padded node matrix pos [B, Smax], r < R — every subgraph marks only its own nodes on its own replica of
// the graph (the paper's labeling trick; utils.MaxZOZ, reference impl/utils.py:32-45, marks the union on one graph).
// -1 and ids >= N are skipped, as the other label kernels do.
//
// One launch, no ordering between workgroups: a workgroup owns kSlab consecutive bytes of the replica-major mask, zero-fills
// them, and then walks the pos rows of the replicas its slab touches and sets the bytes that fall INSIDE the slab — every
// byte is written by one workgroup only, first the zero and (behind a barrier) the one.  A node named twice in a row
// stores the same 1 twice; nothing depends on the order of the entries.
#include "common.h"

namespace glass {

constexpr int kSlab = 16384;  // mask bytes per workgroup: 4 x 16 B per thread

__global__ __launch_bounds__(kBlock) void zeroone_labels_kernel(const int64_t* __restrict__ pos, int Smax, int64_t rep0,
                                                                int64_t N, int64_t total, uint8_t* __restrict__ mask) {
    const int tid = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * kSlab;
    const int64_t b1 = b0 + kSlab < total ? b0 + kSlab : total;
    // 1. zeros: bytes up to the first 16-byte boundary of the ADDRESS, whole vectors, the remaining bytes
    uint8_t* base = mask + b0;
    const int64_t len = b1 - b0;
    int64_t head = (16 - (int64_t)(reinterpret_cast<uintptr_t>(base) & 15u)) & 15;
    if (head > len) head = len;
    for (int64_t k = tid; k < head; k += kBlock) base[k] = 0;
    const int64_t vecs = (len - head) / 16;
    uint4* mv = reinterpret_cast<uint4*>(base + head);
    for (int64_t k = tid; k < vecs; k += kBlock) mv[k] = make_uint4(0u, 0u, 0u, 0u);
    for (int64_t k = head + vecs * 16 + tid; k < len; k += kBlock) base[k] = 0;
    __syncthreads();
    // 2. ones: the entries of the replicas [r_lo, r_hi] this slab overlaps
    const int64_t r_lo = b0 / N, r_hi = (b1 - 1) / N;
    const int64_t n_ent = (r_hi - r_lo + 1) * Smax;
    for (int64_t e = tid; e < n_ent; e += kBlock) {
        const int64_t r = r_lo + e / Smax;
        const int64_t p = pos[(rep0 + r) * Smax + e % Smax];
        if (p >= 0 && p < N) {
            const int64_t flat = r * N + p;
            if (flat >= b0 && flat < b1) mask[flat] = 1;
        }
    }
}

}  // namespace glass

using namespace glass;

extern "C" int glass_zeroone_labels_u8(const int64_t* pos, int64_t B, int64_t Smax, int64_t rep0, int64_t R, int64_t n_nodes,
                                       uint8_t* mask, void* stream) {
    GLASS_REQUIRE(B >= 0 && Smax >= 0 && Smax < (1ll << 31) && n_nodes >= 0 && n_nodes < (1ll << 31),
                  "zeroone_labels: bad sizes B=%lld Smax=%lld N=%lld", (long long)B, (long long)Smax, (long long)n_nodes);
    GLASS_REQUIRE(rep0 >= 0 && R >= 0 && rep0 <= B && R <= B - rep0,
                  "zeroone_labels: rows rep0 .. rep0 + R - 1 must lie inside pos (rep0=%lld R=%lld B=%lld)", (long long)rep0,
                  (long long)R, (long long)B);
    const int64_t total = R * n_nodes;  // < 2^31 * 2^31
    if (total == 0) return 0;
    GLASS_REQUIRE(mask, "zeroone_labels: null mask");
    GLASS_REQUIRE(pos || Smax == 0, "zeroone_labels: null pos");
    GLASS_REQUIRE((reinterpret_cast<uintptr_t>(pos) & 7u) == 0, "zeroone_labels: misaligned pos (8 bytes)");
    const int64_t blocks = ceil_div(total, kSlab);
    if (blocks > 0x7fffffffll) {
        set_error("zeroone_labels: %lld label bytes in one launch, the grid takes %lld", (long long)total,
                  (long long)(0x7fffffffll * kSlab));
        return GLASS_E_UNSUPPORTED;
    }
    hipLaunchKernelGGL(zeroone_labels_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, pos, (int)Smax, rep0,
                       n_nodes, total, mask);
    return launch_status("glass_zeroone_labels_u8");
}
