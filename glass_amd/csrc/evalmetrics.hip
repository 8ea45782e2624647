// Evaluation metrics from exact integer counts (impl/metrics.py:5-27): what micro-F1 and AUROC need from the predictions is
// a handful of integers, so the GPU counts and the host divides.  Every counter is an integer sum — ballot + popcount per
// wave, one integer atomicAdd per wave and counter — hence independent of the order of arrival: bitwise repeatable, no float
// atomic anywhere.  Each entry zeroes its counters on the caller's stream with a one-workgroup fill launch in front of the
// counting launch (a kernel, not hipMemsetAsync: see elementwise.hip on memset nodes in a replayed graph), allocates nothing
// and never synchronises.
#include "head_loss.h"

namespace glass {

constexpr int kF1LaneK = GLASS_EVAL_F1_LANE_K;   // up to this many columns a lane takes a whole row; beyond, a wave does
constexpr int kF1MaxWaves = 4096;                // wave-per-row form: rows are strided over at most this many waves
constexpr int kAurocTile = 1024;                 // scores of one LDS tile of the pair sweep (4 KiB)

using u64 = unsigned long long;

__device__ __forceinline__ void count_add(int64_t* counts, int slot, u64 v) {
    if (v) atomicAdd(reinterpret_cast<u64*>(counts) + slot, v);
}

__global__ __launch_bounds__(kBlock) void counts_zero_kernel(int64_t* __restrict__ counts, int words) {
    for (int k = threadIdx.x; k < words; k += kBlock) counts[k] = 0;
}

// popcount of a predicate over the wave (the same value on every lane)
__device__ __forceinline__ u64 wave_count(bool p) { return (u64)__popcll(__ballot(p)); }

// ---- numpy's argmax as an order on (value, index): a NaN beats every number, the lowest index wins among equals -----------
__device__ __forceinline__ bool argmax_takes(float v, int i, float bv, int bi) {
    const bool vn = v != v, bn = bv != bv;
    if (vn != bn) return vn;
    if (!vn && v != bv) return v > bv;
    return i < bi;  // both NaN, or equal numbers (-0.0 == +0.0)
}

// mode 0, K <= kF1LaneK: one lane per row, the row read in index order (float4 pieces when VEC: base and row stride 16-byte
// aligned).  counts[0] += rows whose argmax is the target; workgroup 0 adds n to counts[1].
template <bool VEC>
__global__ __launch_bounds__(kBlock) void f1_argmax_rows_kernel(const float* __restrict__ pred, int64_t ldp,
                                                                const int64_t* __restrict__ target, int n, int K,
                                                                int64_t* __restrict__ counts) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool hit = false;
    if (i < n) {
        const float* row = pred + (int64_t)i * ldp;
        float bv = row[0];
        int bi = 0;
        int k = 0;
        if (VEC) {
            for (; k + 4 <= K; k += 4) {
                const float4 v = *reinterpret_cast<const float4*>(row + k);
                const float q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (argmax_takes(q[j], k + j, bv, bi)) bv = q[j], bi = k + j;
            }
        }
        for (; k < K; ++k) {
            const float v = row[k];
            if (argmax_takes(v, k, bv, bi)) bv = v, bi = k;
        }
        hit = target[i] == (int64_t)bi;
    }
    const u64 c = wave_count(hit);
    if ((threadIdx.x & (kWave - 1)) == 0) count_add(counts, 0, c);
    if (blockIdx.x == 0 && threadIdx.x == 0) count_add(counts, 1, (u64)n);
}

// mode 0, K > kF1LaneK: one wave per row (rows strided over the grid's waves), lane l holds columns l, l + 64, ..; the
// (value, index) pairs meet in a butterfly.  A lane without a column holds (-inf, INT_MAX): it loses to every real column.
__global__ __launch_bounds__(kBlock) void f1_argmax_wave_kernel(const float* __restrict__ pred, int64_t ldp,
                                                                const int64_t* __restrict__ target, int n, int K,
                                                                int64_t* __restrict__ counts) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    const int n_waves = gridDim.x * (kBlock / kWave);
    u64 hits = 0;  // (wave-uniform)
    for (int i = wave; i < n; i += n_waves) {
        const float* row = pred + (int64_t)i * ldp;
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int k = lane; k < K; k += kWave) {
            const float v = row[k];
            if (argmax_takes(v, k, bv, bi)) bv = v, bi = k;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oi = __shfl_xor(bi, o);
            if (argmax_takes(ov, oi, bv, bi)) bv = ov, bi = oi;
        }
        hits += target[i] == (int64_t)bi ? 1u : 0u;
    }
    if (lane == 0) count_add(counts, 0, hits);
    if (blockIdx.x == 0 && threadIdx.x == 0) count_add(counts, 1, (u64)n);
}

// mode 1: the five counters of one wave.  take(): every lane of the wave calls it together (ballots), `live` false on a
// lane without an element.  prediction bit = pred > 0 (NaN and -0.0: 0); target 1.0 / 0.0, anything else is invalid and
// enters none of the four cells.
struct BinCounts {
    u64 tp = 0, fp = 0, fn = 0, tn = 0, invalid = 0;
    __device__ __forceinline__ void take(bool live, float p, float t) {
        const bool bit = p > 0.f, pos = live && t == 1.f, neg = live && t == 0.f;
        tp += wave_count(pos && bit);
        fp += wave_count(neg && bit);
        fn += wave_count(pos && !bit);
        tn += wave_count(neg && !bit);
        invalid += wave_count(live && !pos && !neg);
    }
    __device__ __forceinline__ void flush(int64_t* counts) const {
        count_add(counts, 0, tp);
        count_add(counts, 1, fp);
        count_add(counts, 2, fn);
        count_add(counts, 3, tn);
        count_add(counts, 4, invalid);
    }
};

// mode 1, K <= kF1LaneK: one lane per row (float4 pieces of both rows when VEC)
template <bool VEC>
__global__ __launch_bounds__(kBlock) void f1_binary_rows_kernel(const float* __restrict__ pred, int64_t ldp,
                                                                const float* __restrict__ target, int64_t ldt, int n, int K,
                                                                int64_t* __restrict__ counts) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < n;
    const float* p = pred + (int64_t)(live ? i : 0) * ldp;   // (a lane past the end reads row 0 and counts nothing)
    const float* t = target + (int64_t)(live ? i : 0) * ldt;
    BinCounts c;
    int k = 0;
    if (VEC) {
        for (; k + 4 <= K; k += 4) {
            const float4 pv = *reinterpret_cast<const float4*>(p + k);
            const float4 tv = *reinterpret_cast<const float4*>(t + k);
            c.take(live, pv.x, tv.x);
            c.take(live, pv.y, tv.y);
            c.take(live, pv.z, tv.z);
            c.take(live, pv.w, tv.w);
        }
    }
    for (; k < K; ++k) c.take(live, p[k], t[k]);
    if ((threadIdx.x & (kWave - 1)) == 0) c.flush(counts);
}

// mode 1, K > kF1LaneK: one wave per row, lanes over the columns
__global__ __launch_bounds__(kBlock) void f1_binary_wave_kernel(const float* __restrict__ pred, int64_t ldp,
                                                                const float* __restrict__ target, int64_t ldt, int n, int K,
                                                                int64_t* __restrict__ counts) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    const int n_waves = gridDim.x * (kBlock / kWave);
    BinCounts c;
    for (int i = wave; i < n; i += n_waves) {
        const float* p = pred + (int64_t)i * ldp;
        const float* t = target + (int64_t)i * ldt;
        for (int k0 = 0; k0 < K; k0 += kWave) {  // (uniform trip count: every lane reaches every ballot)
            const int k = k0 + lane;
            const bool live = k < K;
            c.take(live, live ? p[k] : 0.f, live ? t[k] : 0.f);
        }
    }
    if (lane == 0) c.flush(counts);
}

// AUROC pair count of column k = blockIdx.y: lane = row i keeps its score when its label is 1 (NaN otherwise: every compare
// with a NaN is false, so the lane adds nothing), the workgroup walks all rows j through LDS tiles holding score_j where
// label_j is 0 (NaN otherwise, and as padding up to a multiple of 4).  Every lane reads the same LDS address: a broadcast.
//   twoU += [s_i > s_j] + [s_i >= s_j]   ( = 2 [s_i > s_j] + [s_i == s_j] )
// per lane at most 2 n <= 2^17: 32-bit within a tile, 64-bit across tiles and lanes.
__global__ __launch_bounds__(kBlock) void auroc_pairs_kernel(const float* __restrict__ score, int64_t lds,
                                                             const float* __restrict__ label, int64_t ldl, int n,
                                                             int64_t* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) float tile[kAurocTile];
    const int k = blockIdx.y, tid = threadIdx.x;
    const int i = blockIdx.x * kBlock + tid;
    const float nan = __builtin_nanf("");
    float si = nan;
    bool pos = false, neg = false, bad = false;
    if (i < n) {
        const float s = score[(int64_t)i * lds + k], y = label[(int64_t)i * ldl + k];
        pos = y == 1.f;
        neg = y == 0.f;
        bad = !(fabsf(s) < INFINITY) || !(pos || neg);  // (scikit-learn refuses NaN and infinite scores alike)
        if (pos) si = s;
    }
    u64 two_u = 0;
    for (int j0 = 0; j0 < n; j0 += kAurocTile) {
        const int cnt = min(kAurocTile, n - j0), cnt4 = (cnt + 3) & ~3;
        __syncthreads();  // the previous tile has been read
        for (int j = tid; j < cnt4; j += kBlock) {
            float v = nan;
            if (j < cnt && label[(int64_t)(j0 + j) * ldl + k] == 0.f) v = score[(int64_t)(j0 + j) * lds + k];
            tile[j] = v;
        }
        __syncthreads();
        unsigned acc = 0;
        for (int j = 0; j < cnt4; j += 4) {
            const float4 v = *reinterpret_cast<const float4*>(tile + j);
            acc += (si > v.x) + (si >= v.x) + (si > v.y) + (si >= v.y) + (si > v.z) + (si >= v.z) + (si > v.w) + (si >= v.w);
        }
        two_u += acc;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) two_u += __shfl_xor(two_u, o);
    const u64 P = wave_count(pos), N = wave_count(neg), inv = wave_count(bad);
    if ((tid & (kWave - 1)) == 0) {
        count_add(counts, 4 * k + 0, two_u);
        count_add(counts, 4 * k + 1, P);
        count_add(counts, 4 * k + 2, N);
        count_add(counts, 4 * k + 3, inv);
    }
}

static bool auroc_sizes_ok(int64_t n, int64_t K) { return n >= 1 && n <= GLASS_EVAL_AUROC_MAX_ROWS && K >= 1 && K <= kMaxK; }

}  // namespace glass

using namespace glass;

extern "C" int glass_eval_f1_counts_f32(const float* pred, int64_t ldp, const void* target, int64_t ldt, int64_t n, int64_t K,
                                        int mode, int64_t* counts, void* stream) {
    GLASS_REQUIRE(pred && target && counts, "eval_f1_counts: null pointer");
    GLASS_REQUIRE(n >= 1 && K >= 1, "eval_f1_counts: bad sizes");
    if (!loss_mode_ok(mode)) {
        set_error("eval_f1_counts: unknown mode %d", mode);
        return GLASS_E_UNSUPPORTED;
    }
    if (K > kMaxK) {
        set_error("eval_f1_counts: at most %d columns", kMaxK);
        return GLASS_E_UNSUPPORTED;
    }
    const bool binary = mode == 1;
    GLASS_REQUIRE(ldp >= K && (!binary || ldt >= K), "eval_f1_counts: row stride < K");
    const int64_t ld = binary && ldt > ldp ? ldt : ldp;
    if (ld >= (1ll << 29) || n > ((1ll << 31) - 1) / (4 * ld)) {  // n * ld * 4 < 2^31
        set_error("eval_f1_counts: n * ld * 4 must stay below 2^31");
        return GLASS_E_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(counts_zero_kernel, dim3(1), dim3(kBlock), 0, st, counts, 8);
    const float* tf = (const float*)target;
    const int64_t* ti = (const int64_t*)target;
    if (K <= kF1LaneK) {
        const dim3 grid((unsigned)ceil_div(n, kBlock)), block(kBlock);
        const bool vec = aligned16(pred) && ldp % 4 == 0 && (!binary || (aligned16(target) && ldt % 4 == 0));
        if (binary) {
            if (vec)
                hipLaunchKernelGGL(f1_binary_rows_kernel<true>, grid, block, 0, st, pred, ldp, tf, ldt, (int)n, (int)K, counts);
            else
                hipLaunchKernelGGL(f1_binary_rows_kernel<false>, grid, block, 0, st, pred, ldp, tf, ldt, (int)n, (int)K, counts);
        } else {
            if (vec)
                hipLaunchKernelGGL(f1_argmax_rows_kernel<true>, grid, block, 0, st, pred, ldp, ti, (int)n, (int)K, counts);
            else
                hipLaunchKernelGGL(f1_argmax_rows_kernel<false>, grid, block, 0, st, pred, ldp, ti, (int)n, (int)K, counts);
        }
    } else {
        const int64_t waves = n < kF1MaxWaves ? n : kF1MaxWaves;
        const dim3 grid((unsigned)ceil_div(waves, kBlock / kWave)), block(kBlock);
        if (binary)
            hipLaunchKernelGGL(f1_binary_wave_kernel, grid, block, 0, st, pred, ldp, tf, ldt, (int)n, (int)K, counts);
        else
            hipLaunchKernelGGL(f1_argmax_wave_kernel, grid, block, 0, st, pred, ldp, ti, (int)n, (int)K, counts);
    }
    return launch_status("glass_eval_f1_counts_f32");
}

extern "C" int glass_eval_auroc_supported(int64_t n, int64_t K) { return auroc_sizes_ok(n, K) ? 1 : 0; }

extern "C" int glass_eval_auroc_counts_f32(const float* score, int64_t lds, const float* label, int64_t ldl, int64_t n,
                                           int64_t K, int64_t* counts, void* stream) {
    GLASS_REQUIRE(score && label && counts, "eval_auroc_counts: null pointer");
    GLASS_REQUIRE(n >= 1 && K >= 1, "eval_auroc_counts: bad sizes");
    if (!auroc_sizes_ok(n, K)) {
        set_error("eval_auroc_counts: at most %d rows and %d columns", GLASS_EVAL_AUROC_MAX_ROWS, kMaxK);
        return GLASS_E_UNSUPPORTED;
    }
    GLASS_REQUIRE(lds >= K && ldl >= K, "eval_auroc_counts: row stride < K");
    const int64_t ld = ldl > lds ? ldl : lds;
    if (ld >= (1ll << 29) || n > ((1ll << 31) - 1) / (4 * ld)) {
        set_error("eval_auroc_counts: n * ld * 4 must stay below 2^31");
        return GLASS_E_UNSUPPORTED;
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(counts_zero_kernel, dim3(1), dim3(kBlock), 0, st, counts, (int)(4 * K));
    hipLaunchKernelGGL(auroc_pairs_kernel, dim3((unsigned)ceil_div(n, kBlock), (unsigned)K), dim3(kBlock), 0, st, score, lds,
                       label, ldl, (int)n, counts);
    return launch_status("glass_eval_auroc_counts_f32");
}
