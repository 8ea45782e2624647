// K7a: attention pooling straight from the padded node matrix (pool `attn`, models.AttnPool) — an extension beside K7's
// pool family (reference impl/models.py:275-319, 346-350: the PoolModule classes and the call that applies them); the
// reference itself has no learned readout.  Gated global attention with a softmax over the nodes of each subgraph:
//     s[b,j]   = dot(emb[pos[b,j], :], w)                      pos[b,j] >= 0 (a -1 may sit anywhere in a row: K7's rule)
//     a[b,j]   = exp(s[b,j] - max_j s[b,.]) / sum_j exp(..)    over the valid j of row b; 0 at padding
//     out[b,:] = sum_j a[b,j] * emb[pos[b,j], :]               a node named twice counts twice; an all-padding row gives 0
// There is NO gate bias: a bias adds the same number to every score of a row, the max subtraction removes it again, so its
// gradient is identically 0.
// Backward (dout [B,C]; t[b,j] = dot(dout[b], emb[pos[b,j]])):
//     ds[b,j]   = a[b,j] * (t[b,j] - dot(dout[b], out[b]))
//     demb[n,:] = sum_{(b,j): pos[b,j] = n} (a[b,j] * dout[b,:] + ds[b,j] * w)
//     dw[:]  (+)= sum_{b,j} ds[b,j] * emb[pos[b,j], :]
// Nothing of the softmax is recomputed in the backward: a (saved by the forward) and out are its only state, so there is
// one exp — expf, in the forward — and no second definition that could disagree with it.
//
// One subgraph per workgroup of 256 lanes, or per ONE-WAVE workgroup (64 lanes) for rows of at most kAttnWaveRows entries.
// A row pass has three parts: (1) one wave per entry forms the score dot (lanes stride the columns in index order, a
// butterfly of lane shuffles folds the 64 partial sums: every lane ends with the same bits) and, while the row's entries fit
// kAttnStageFloats of LDS, leaves the gathered row there — the weighted sum then reads LDS, so emb[pos[b,j]] is fetched
// once; beyond that capacity the weighted sum gathers a second time (two-pass form: the scores wait in `alpha`, which is
// normalised in place); (2) max, exp and the normaliser over the row: lane t takes entries t, t + T, .. in index order,
// then the fixed tree; (3) the weighted sum: lane groups of TC columns, entry slots in ascending j, slots folded in slot
// order through LDS.  Every order is a function of (C, Smax, the form) alone: bitwise repeatable, no float atomic anywhere.
//
// dw: every subgraph's share goes to the workspace ([B][C]) and a second launch adds the shares in b order — the order
// depends on their count alone (the scheme of gradclip.hip).  demb: the entries are bucketed by node (bucket.h: integer
// counts, a scan, integer cursors; the order inside a node's list is arbitrary) and a node's row is the sum of its entries'
// contributions in EXACT fixed point (ExactSum: integer addition commutes), so which workgroup ran first never reaches the
// result; every row of demb is written, a node no entry names gets zeros.
//
// Addressing is plain 64-bit pointer arithmetic (no whole-tensor buffer resource), so n_nodes * lde * 4 has no 32-bit limit.
// The library keeps no mutable state and reads no environment.
#include "bucket.h"
#include "common.h"

#include <math.h>

namespace glass {

constexpr int kAttnMaxC = 4096;          // widest pooled row served (JK: output + (L - 1) * hidden)
constexpr int kAttnWaveRows = 16;        // padded rows up to this many entries: one wave (a 64-lane workgroup) per subgraph
constexpr int kAttnStageFloats = 12288;  // Smax * C up to this: the gathered rows stay in LDS (48 KiB), one gather per entry
constexpr int kAttnScoreRows = 2048;     // Smax up to this: the scores wait in LDS; beyond it in `alpha` itself

// Sum / max over a workgroup of T lanes, the same bits on every lane: xor butterfly inside each wave (both partners add the
// same two numbers, so by induction all lanes agree), then the wave results in wave order.
template <int T, bool MAX>
__device__ __forceinline__ float attn_block_fold(float v, float* lds) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off, kWave);
        v = MAX ? fmaxf(v, o) : v + o;
    }
    if (T == kWave) return v;
    if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = lds[0];
#pragma unroll
    for (int w = 1; w < T / kWave; ++w) s = MAX ? fmaxf(s, lds[w]) : s + lds[w];
    __syncthreads();  // (lds is reused by the next fold)
    return s;
}

__device__ __forceinline__ bool attn_valid(int64_t node, int64_t n_nodes) { return node >= 0 && node < n_nodes; }

// dot(x, vec) over C columns by one wave, the same bits on every lane: lane l takes columns l, l + 64, .. in index order,
// then the xor butterfly.  STAGE: x is also copied to keep[0 .. C).
template <bool STAGE>
__device__ __forceinline__ float attn_wave_dot(const float* __restrict__ x, const float* __restrict__ vec, int C, float* keep) {
    float acc = 0.f;
    for (int c = threadIdx.x & (kWave - 1); c < C; c += kWave) {
        const float xv = x[c];
        if (STAGE) keep[c] = xv;
        acc = fmaf(xv, vec[c], acc);
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off, kWave);
    return acc;
}

// (1)  sc[j] = dot(emb[pos[j]], vec) for the valid entries of the row (0 at padding); STAGE: the row also goes to
// stage[j * C ..].  One wave per entry, entries w, w + T/64, ..
template <int T, bool STAGE>
__device__ __forceinline__ void attn_row_dots(const float* __restrict__ emb, int64_t lde, const int64_t* __restrict__ prow,
                                              int Smax, int64_t n_nodes, int C, const float* __restrict__ vec, float* sc,
                                              float* stage) {
    for (int j = threadIdx.x >> 6; j < Smax; j += T / kWave) {
        const int64_t node = prow[j];
        if (!attn_valid(node, n_nodes)) {  // wave-uniform
            if ((threadIdx.x & (kWave - 1)) == 0) sc[j] = 0.f;
            continue;
        }
        const float acc = attn_wave_dot<STAGE>(emb + node * lde, vec, C, stage + (STAGE ? (size_t)j * C : 0));
        if ((threadIdx.x & (kWave - 1)) == 0) sc[j] = acc;
    }
}

// (3)  dst[c] = sum over the valid j of coef[j] * emb[pos[j]][c].  TC = 1 << tc_log2 lanes cover a chunk of columns, the
// T / TC slots take entries slot, slot + T/TC, .. in ascending order, slot sums are added in slot order.
template <int T, bool STAGE>
__device__ __forceinline__ void attn_row_wsum(const float* __restrict__ emb, int64_t lde, const int64_t* __restrict__ prow,
                                              int Smax, int64_t n_nodes, int C, const float* coef, const float* stage,
                                              float* __restrict__ dst, int tc_log2, float* red) {
    const int TC = 1 << tc_log2, slots = T >> tc_log2;
    const int tc = threadIdx.x & (TC - 1), slot = threadIdx.x >> tc_log2;
    for (int c0 = 0; c0 < C; c0 += TC) {  // uniform trip count: barriers inside
        const int c = c0 + tc;
        float acc = 0.f;
        if (c < C)
            for (int j = slot; j < Smax; j += slots) {
                const int64_t node = prow[j];
                if (!attn_valid(node, n_nodes)) continue;
                const float xv = STAGE ? stage[(size_t)j * C + c] : emb[node * lde + c];
                acc = fmaf(coef[j], xv, acc);
            }
        if (slots > 1) {
            red[threadIdx.x] = acc;
            __syncthreads();
            if (slot == 0)
                for (int r = 1; r < slots; ++r) acc += red[(r << tc_log2) + tc];
        }
        if (slot == 0 && c < C) dst[c] = acc;
        if (slots > 1) __syncthreads();
    }
}

template <int T, bool STAGE>
__global__ __launch_bounds__(T) void attn_pool_fwd_kernel(const float* __restrict__ emb, int64_t lde,
                                                          const int64_t* __restrict__ pos, int Smax,
                                                          const float* __restrict__ w, float* __restrict__ out, int64_t ldo,
                                                          float* alpha, int64_t n_nodes, int C, int tc_log2) {
    extern __shared__ float attn_stage[];  // [Smax * C] (STAGE), 4-byte accesses only
    __shared__ float lds_sc[kAttnScoreRows];
    __shared__ float red[T];
    __shared__ float fold[4];
    const int b = blockIdx.x;
    const int64_t* prow = pos + (int64_t)b * Smax;
    float* arow = alpha + (int64_t)b * Smax;
    float* sc = Smax <= kAttnScoreRows ? lds_sc : arow;  // workgroup-uniform
    attn_row_dots<T, STAGE>(emb, lde, prow, Smax, n_nodes, C, w, sc, attn_stage);
    __syncthreads();
    float m = -INFINITY;
    int any = 0;
    for (int j = threadIdx.x; j < Smax; j += T)
        if (attn_valid(prow[j], n_nodes)) {
            m = fmaxf(m, sc[j]);
            any = 1;
        }
    m = attn_block_fold<T, true>(m, fold);
    any = __syncthreads_or(any);
    if (!any) {  // all padding: zeros (K7's rule)
        for (int j = threadIdx.x; j < Smax; j += T) arow[j] = 0.f;
        for (int c = threadIdx.x; c < C; c += T) out[(int64_t)b * ldo + c] = 0.f;
        return;
    }
    float z = 0.f;
    for (int j = threadIdx.x; j < Smax; j += T) {
        const float e = attn_valid(prow[j], n_nodes) ? expf(sc[j] - m) : 0.f;
        sc[j] = e;
        z += e;
    }
    z = attn_block_fold<T, false>(z, fold);
    for (int j = threadIdx.x; j < Smax; j += T) {
        const float a = sc[j] / z;
        sc[j] = a;
        if (sc != arow) arow[j] = a;
    }
    __syncthreads();
    attn_row_wsum<T, STAGE>(emb, lde, prow, Smax, n_nodes, C, sc, attn_stage, out + (int64_t)b * ldo, tc_log2, red);
}

// Backward, per subgraph: ds[b, :] (workspace, 0 at padding) and the subgraph's share of dw (workspace part[b, :]).
template <int T, bool STAGE>
__global__ __launch_bounds__(T) void attn_pool_bwd_row_kernel(const float* __restrict__ dout, int64_t ldd,
                                                              const float* __restrict__ emb, int64_t lde,
                                                              const int64_t* __restrict__ pos, int Smax,
                                                              const float* __restrict__ alpha, const float* __restrict__ out,
                                                              int64_t ldo, float* ds, float* __restrict__ part,
                                                              int64_t n_nodes, int C, int tc_log2) {
    extern __shared__ float attn_stage[];
    __shared__ float red[T];
    const int b = blockIdx.x;
    const int64_t* prow = pos + (int64_t)b * Smax;
    const float* g = dout + (int64_t)b * ldd;
    float* drow = ds + (int64_t)b * Smax;
    // dot(dout[b], out[b]), by every wave for itself and in the order of the entry dots: a row with ONE valid entry has
    // out == that node's row bit for bit, so t - go cancels exactly and its ds is 0, as in exact arithmetic
    const float go = attn_wave_dot<false>(out + (int64_t)b * ldo, g, C, nullptr);
    attn_row_dots<T, STAGE>(emb, lde, prow, Smax, n_nodes, C, g, drow, attn_stage);  // t[b, j]
    __syncthreads();
    for (int j = threadIdx.x; j < Smax; j += T)
        drow[j] = attn_valid(prow[j], n_nodes) ? alpha[(int64_t)b * Smax + j] * (drow[j] - go) : 0.f;
    __syncthreads();
    attn_row_wsum<T, STAGE>(emb, lde, prow, Smax, n_nodes, C, drow, attn_stage, part + (int64_t)b * C, tc_log2, red);
}

// dw[c] (+)= part[0][c] + part[1][c] + ..  in b order (one lane per column)
__global__ __launch_bounds__(kBlock) void attn_pool_dw_fold_kernel(const float* __restrict__ part, int64_t B, int C,
                                                                   float* __restrict__ dw, int acc_dw) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int64_t b = 0; b < B; ++b) s += part[b * C + c];
    dw[c] = acc_dw ? dw[c] + s : s;
}

// demb[node, :] = exact sum over the node's entries e (b = e / Smax) of alpha[e] * dout[b, :] + ds[e] * w.  G lanes per
// node, 256 / G nodes per workgroup.
__global__ __launch_bounds__(kBlock) void attn_pool_demb_kernel(const float* __restrict__ dout, int64_t ldd,
                                                                const float* __restrict__ w, const float* __restrict__ alpha,
                                                                const float* __restrict__ ds, const int32_t* __restrict__ off,
                                                                const int32_t* __restrict__ list, int Smax,
                                                                float* __restrict__ demb, int64_t ldde, int64_t n_nodes, int C,
                                                                int g_log2) {
    const int G = 1 << g_log2, li = threadIdx.x & (G - 1);
    const int64_t node = (int64_t)blockIdx.x * (kBlock >> g_log2) + (threadIdx.x >> g_log2);
    if (node >= n_nodes) return;
    const int beg = off[node], end = off[node + 1];
    for (int c = li; c < C; c += G) {
        ExactSum s{0, 0};
        const float wc = w[c];
        for (int i = beg; i < end; ++i) {
            const int e = list[i];
            const int64_t b = e / Smax;
            s.add(fmaf(ds[e], wc, alpha[e] * dout[b * ldd + c]));
        }
        demb[node * ldde + c] = s.value();
    }
}

__global__ __launch_bounds__(kBlock) void attn_pool_zero_kernel(float* __restrict__ p, int64_t ld, int64_t rows, int C) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < rows * C; i += (int64_t)gridDim.x * kBlock)
        p[(i / C) * ld + i % C] = 0.f;
}

}  // namespace glass

using namespace glass;

static inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

static int attn_sizes_ok(const char* what, int64_t B, int64_t Smax, int64_t n_nodes, int64_t C) {
    GLASS_REQUIRE(B >= 0 && Smax >= 0 && n_nodes >= 0 && C >= 1, "%s: B = %lld, Smax = %lld, n_nodes = %lld, C = %lld", what,
                  (long long)B, (long long)Smax, (long long)n_nodes, (long long)C);
    if (C > kAttnMaxC) {
        set_error("%s: C = %lld (1 <= C <= %d)", what, (long long)C, kAttnMaxC);
        return GLASS_E_UNSUPPORTED;
    }
    GLASS_REQUIRE(B < (1ll << 31) && Smax < (1ll << 31) && n_nodes < (1ll << 31) &&
                      (B == 0 || Smax == 0 || B <= ((1ll << 30) - 1) / Smax),
                  "%s: fewer than 2^30 entries and 2^31 nodes", what);
    return 0;
}

static int attn_tc_log2(int64_t C, int T) {
    const int tc = pow2_ceil_cap(C, T);
    int l = 0;
    while ((1 << l) < tc) ++l;
    return l;
}

extern "C" int64_t glass_attn_pool_wave_rows(void) { return kAttnWaveRows; }
extern "C" int64_t glass_attn_pool_stage_floats(void) { return kAttnStageFloats; }
extern "C" int64_t glass_attn_pool_score_rows(void) { return kAttnScoreRows; }

extern "C" int glass_attn_pool_f32(const float* emb, int64_t lde, const int64_t* pos, int64_t B, int64_t Smax, const float* w,
                                   float* out, int64_t ldo, float* alpha, int64_t n_nodes, int64_t C, void* stream) {
    int rc = attn_sizes_ok("attn_pool", B, Smax, n_nodes, C);
    if (rc) return rc;
    GLASS_REQUIRE(lde >= C && ldo >= C, "attn_pool: lde = %lld, ldo = %lld, C = %lld", (long long)lde, (long long)ldo, (long long)C);
    if (B == 0 || Smax == 0) return 0;  // a valid no-op: nothing is launched, out is not touched
    GLASS_REQUIRE(emb && pos && w && out && alpha, "attn_pool: null pointer");
    GLASS_REQUIRE(aligned4(emb) && aligned4(w) && aligned4(out) && aligned4(alpha) && (reinterpret_cast<uintptr_t>(pos) & 7u) == 0,
                  "attn_pool: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const bool wave = Smax <= kAttnWaveRows, stage = Smax * C <= kAttnStageFloats;
    const size_t dyn = stage ? sizeof(float) * (size_t)(Smax * C) : 0;
    const int tl = attn_tc_log2(C, wave ? kWave : kBlock);
#define GLASS_ATTN_FWD(T, S)                                                                                                  \
    hipLaunchKernelGGL((attn_pool_fwd_kernel<T, S>), dim3((unsigned)B), dim3(T), dyn, st, emb, lde, pos, (int)Smax, w, out, ldo, \
                       alpha, n_nodes, (int)C, tl)
    if (wave && stage) GLASS_ATTN_FWD(kWave, true);
    else if (wave) GLASS_ATTN_FWD(kWave, false);
    else if (stage) GLASS_ATTN_FWD(kBlock, true);
    else GLASS_ATTN_FWD(kBlock, false);
#undef GLASS_ATTN_FWD
    return launch_status("glass_attn_pool_f32");
}

// int32 words of the node buckets (the entries as a [B * Smax, 1] matrix: the lists then carry the ENTRY index), rounded to 16 B
static int64_t attn_bucket_words(int64_t n_nodes, int64_t E) { return (bucket_ws_words(n_nodes, E, 1, false) + 3) & ~(int64_t)3; }

extern "C" int64_t glass_attn_pool_bwd_ws_bytes(int64_t n_nodes, int64_t B, int64_t Smax, int64_t C) {
    if (n_nodes <= 0 || B <= 0 || Smax <= 0 || C <= 0) return 0;
    // node buckets | ds [B * Smax] | per-subgraph dw shares [B * C]   (each part whole 16-byte units)
    return (int64_t)sizeof(int32_t) *
           (attn_bucket_words(n_nodes, B * Smax) + ((B * Smax + 3) & ~(int64_t)3) + ((B * C + 3) & ~(int64_t)3));
}

extern "C" int glass_attn_pool_bwd_f32(const float* dout, int64_t ldd, const float* emb, int64_t lde, const int64_t* pos,
                                       int64_t B, int64_t Smax, const float* w, const float* alpha, const float* out,
                                       int64_t ldo, float* demb, int64_t ldde, float* dw, int acc_dw, int64_t n_nodes, int64_t C,
                                       void* ws, void* stream) {
    int rc = attn_sizes_ok("attn_pool_bwd", B, Smax, n_nodes, C);
    if (rc) return rc;
    GLASS_REQUIRE(ldd >= C && lde >= C && ldo >= C && ldde >= C, "attn_pool_bwd: a leading dimension is smaller than C = %lld",
                  (long long)C);
    GLASS_REQUIRE(dw && (demb || n_nodes == 0), "attn_pool_bwd: null pointer");
    GLASS_REQUIRE(aligned4(dout) && aligned4(emb) && aligned4(w) && aligned4(alpha) && aligned4(out) && aligned4(demb) &&
                      aligned4(dw) && (reinterpret_cast<uintptr_t>(pos) & 7u) == 0 && aligned16(ws),
                  "attn_pool_bwd: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    if (B == 0 || Smax == 0 || n_nodes == 0) {  // no entry: zero gradients
        if (n_nodes > 0) {
            const int64_t blocks = ceil_div(n_nodes * C, (int64_t)kBlock);
            hipLaunchKernelGGL(attn_pool_zero_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(kBlock), 0, st, demb, ldde,
                               n_nodes, (int)C);
        }
        if (!acc_dw)
            hipLaunchKernelGGL(attn_pool_zero_kernel, dim3((unsigned)ceil_div(C, (int64_t)kBlock)), dim3(kBlock), 0, st, dw, C,
                               (int64_t)1, (int)C);
        return launch_status("glass_attn_pool_bwd_f32");
    }
    GLASS_REQUIRE(dout && emb && pos && w && alpha && out && ws, "attn_pool_bwd: null pointer");
    const int64_t E = B * Smax;
    float* ds = reinterpret_cast<float*>(ws) + attn_bucket_words(n_nodes, E);
    float* part = ds + ((E + 3) & ~(int64_t)3);
    const bool wave = Smax <= kAttnWaveRows, stage = Smax * C <= kAttnStageFloats;
    const size_t dyn = stage ? sizeof(float) * (size_t)(Smax * C) : 0;
    const int tl = attn_tc_log2(C, wave ? kWave : kBlock);
#define GLASS_ATTN_BWD(T, S)                                                                                                      \
    hipLaunchKernelGGL((attn_pool_bwd_row_kernel<T, S>), dim3((unsigned)B), dim3(T), dyn, st, dout, ldd, emb, lde, pos, (int)Smax, \
                       alpha, out, ldo, ds, part, n_nodes, (int)C, tl)
    if (wave && stage) GLASS_ATTN_BWD(kWave, true);
    else if (wave) GLASS_ATTN_BWD(kWave, false);
    else if (stage) GLASS_ATTN_BWD(kBlock, true);
    else GLASS_ATTN_BWD(kBlock, false);
#undef GLASS_ATTN_BWD
    rc = launch_status("glass_attn_pool_bwd_f32 (rows)");
    if (rc) return rc;
    hipLaunchKernelGGL(attn_pool_dw_fold_kernel, dim3((unsigned)ceil_div(C, (int64_t)kBlock)), dim3(kBlock), 0, st, part, B, (int)C,
                       dw, acc_dw);
    BucketLists bl;
    rc = bucket_build(pos, E, 1, -1, false, n_nodes, ws, st, &bl);
    if (rc) return rc;
    const int gl = attn_tc_log2(C, kWave);
    hipLaunchKernelGGL(attn_pool_demb_kernel, dim3((unsigned)ceil_div(n_nodes, (int64_t)(kBlock >> gl))), dim3(kBlock), 0, st, dout,
                       ldd, w, alpha, ds, bl.off, bl.list, (int)Smax, demb, ldde, n_nodes, (int)C, gl);
    return launch_status("glass_attn_pool_bwd_f32");
}
