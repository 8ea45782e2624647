// The row-blocked GraphNorm passes as device bodies: shared by the whole-graph kernels (graphnorm.hip) and the replicated
// form (graphnorm_rep.hip: R segments of N rows each, one grid plane per replica), so that a replica's bits are the
// whole-graph entry's bits on its slice by construction.  Every body reads blockIdx.x / gridDim.x as ITS row blocking and
// blockIdx.y as its column tile; the caller hands it the operands of one graph.
#pragma once
#include "common.h"
#include "gn_math.h"
#include "gn_acc.h"

namespace glass {

constexpr int kUnroll = 4;
constexpr int kMaxStatBlocks = 1024;

struct Tiling {
    int vw;       // floats per access (4 if everything is 16-B aligned, else 1)
    int cw;       // column words = ceil(C / vw)
    int tc;       // lanes across columns (power of two <= 256)
    int tc_log2;
    int rpb;      // rows per workgroup step = 256 / tc
    int ctiles;   // grid.y
};

static Tiling make_tiling(int64_t C, bool vec_ok) {
    Tiling t;
    t.vw = vec_ok ? 4 : 1;
    t.cw = (int)ceil_div(C, t.vw);
    t.tc = pow2_ceil_cap(t.cw, kBlock);
    t.tc_log2 = 0;
    while ((1 << t.tc_log2) < t.tc) ++t.tc_log2;
    t.rpb = kBlock / t.tc;
    t.ctiles = (int)ceil_div(t.cw, t.tc);
    return t;
}

static int stat_blocks(int64_t n_rows, const Tiling& t) {
    int64_t b = ceil_div(n_rows, (int64_t)t.rpb * kUnroll * 2);
    if (b < 1) b = 1;
    if (b > kMaxStatBlocks) b = kMaxStatBlocks;
    return (int)b;
}

// scratch: [kMaxStatBlocks][2][C] doubles (column partials) + [4][C] floats (backward coefficients)
static int64_t ws_partials_bytes(int64_t C) { return (int64_t)kMaxStatBlocks * 2 * C * (int64_t)sizeof(double); }

template <int VW> struct F;
template <> struct F<4> {
    float a[4];
    __device__ __forceinline__ void load(const float* p) {
        float4 v = *reinterpret_cast<const float4*>(p);
        a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w;
    }
    __device__ __forceinline__ void store(float* p) const {
        *reinterpret_cast<float4*>(p) = make_float4(a[0], a[1], a[2], a[3]);
    }
};
template <> struct F<1> {
    float a[1];
    __device__ __forceinline__ void load(const float* p) { a[0] = *p; }
    __device__ __forceinline__ void store(float* p) const { *p = a[0]; }
};

// Load per-column parameters for this thread's column word (zeros past C).
template <int VW>
__device__ __forceinline__ void load_cols(float (&dst)[VW], const float* src, int c0, int C) {
#pragma unroll
    for (int k = 0; k < VW; ++k) dst[k] = (c0 + k < C) ? src[c0 + k] : 0.f;
}

// Reduce this thread's 2*VW fp64 accumulators over the row slots of the workgroup (fixed order)
// and let row slot 0 write them to partial[blk][which][c].
template <int VW>
__device__ __forceinline__ void block_reduce_store(double (&s0)[VW], double (&s1)[VW], double* lds, int tc, int tr,
                                                   int TC, int rpb, double* partial, int c0, int C, int exact = 0) {
    double* mine = lds + (size_t)threadIdx.x * 2 * VW;
#pragma unroll
    for (int k = 0; k < VW; ++k) {
        mine[k] = s0[k];
        mine[VW + k] = s1[k];
    }
    __syncthreads();
    if (tr == 0) {
        for (int r = 1; r < rpb; ++r) {
            const double* o = lds + (size_t)(r * TC + tc) * 2 * VW;
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                s0[k] += o[k];
                s1[k] += o[VW + k];
            }
        }
        if (exact) {  // `partial` = exact accumulators (gn_acc.h), forward scale
            long long* a = reinterpret_cast<long long*>(partial);
#pragma unroll
            for (int k = 0; k < VW; ++k)
                if (c0 + k < C) {
                    gn_acc_add(a, blockIdx.x % exact, 0, c0 + k, C, s0[k], kAccScaleFwd);
                    gn_acc_add(a, blockIdx.x % exact, 1, c0 + k, C, s1[k], kAccScaleFwd);
                }
            return;
        }
        double* p = partial + (size_t)blockIdx.x * 2 * C;
#pragma unroll
        for (int k = 0; k < VW; ++k)
            if (c0 + k < C) {
                p[c0 + k] = s0[k];
                p[C + c0 + k] = s1[k];
            }
    }
}

// ---- forward statistics: per-column sum(x), sum(x^2) ------------------------------------------
template <int VW>
__device__ __forceinline__ void gn_stats_body(const float* __restrict__ x, int64_t ldx, int64_t N, int C,
                                                          int tc_log2, double* __restrict__ partial, int exact) {
    __shared__ double lds[kBlock * 2 * VW];
    const int TC = 1 << tc_log2, rpb = kBlock >> tc_log2;
    const int tc = threadIdx.x & (TC - 1), tr = threadIdx.x >> tc_log2;
    const int c0 = (blockIdx.y * TC + tc) * VW;
    const bool ok = c0 < C;
    double s[VW], q[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) s[k] = q[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * rpb;
    for (int64_t r = (int64_t)blockIdx.x * rpb + tr; r < N; r += stride * kUnroll) {
        F<VW> v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t rr = r + u * stride;
#pragma unroll
            for (int k = 0; k < VW; ++k) v[u].a[k] = 0.f;
            if (ok && rr < N) v[u].load(x + rr * ldx + c0);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                const double d = (double)v[u].a[k];
                s[k] += d;
                q[k] += d * d;
            }
    }
    block_reduce_store<VW>(s, q, lds, tc, tr, TC, rpb, partial, c0, C, exact);
}

// ---- forward apply: y = dropout(act(x*scale + shift)) ------------------------------------------
template <int VW>
__device__ __forceinline__ void gn_apply_body(const float* __restrict__ x, int64_t ldx,
                                                          float* __restrict__ y, int64_t ldy, int64_t N, int C,
                                                          int tc_log2, const float* __restrict__ saved, int act,
                                                          Drop drop, const uint64_t* __restrict__ rng_state) {
    const int TC = 1 << tc_log2, rpb = kBlock >> tc_log2;
    const int tc = threadIdx.x & (TC - 1), tr = threadIdx.x >> tc_log2;
    const int c0 = (blockIdx.y * TC + tc) * VW;
    if (c0 >= C) return;
    float scale[VW], shift[VW];
    load_cols<VW>(scale, saved + 2 * C, c0, C);
    load_cols<VW>(shift, saved + 3 * C, c0, C);
    if (drop.p > 0.f) {
        drop.seed = rng_state[0];
        drop.step = rng_state[1];
    }
    const int64_t stride = (int64_t)gridDim.x * rpb;
    for (int64_t r = (int64_t)blockIdx.x * rpb + tr; r < N; r += stride * kUnroll) {
        F<VW> v[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t rr = r + u * stride;
            if (rr < N) v[u].load(x + rr * ldx + c0);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t rr = r + u * stride;
            if (rr >= N) continue;
            float ds[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) ds[k] = 1.f;
            if (drop.p > 0.f) drop_scales<VW>(drop, rr, c0, ds);
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                float h = fmaf(v[u].a[k], scale[k], shift[k]);
                h = act_exact(act, h);
                v[u].a[k] = h * ds[k];
            }
            v[u].store(y + rr * ldy + c0);
        }
    }
}

// ---- backward statistics: S1 = sum(g), S2 = sum(g * xhat), g = dy * dropmask * act'(h) ---------
template <int VW>
__device__ __forceinline__ void bwd_g(float (&g)[VW], const float (&xv)[VW], const float (&scale)[VW],
                                      const float (&shift)[VW], int act, const Drop& drop, int64_t row, int c0) {
    if (drop.p > 0.f) {
        float ds[VW];
        drop_scales<VW>(drop, row, c0, ds);
#pragma unroll
        for (int k = 0; k < VW; ++k) g[k] *= ds[k];
    }
    if (act != GLASS_ACT_NONE) {
#pragma unroll
        for (int k = 0; k < VW; ++k) g[k] *= act_grad(act, fmaf(xv[k], scale[k], shift[k]));
    }
}

template <int VW>
__device__ __forceinline__ void gn_bwd_stats_body(const float* __restrict__ dy, int64_t lddy,
                                                              const float* __restrict__ x, int64_t ldx, int64_t N,
                                                              int C, int tc_log2, const float* __restrict__ saved,
                                                              const float* __restrict__ alpha, int act, Drop drop,
                                                              const uint64_t* __restrict__ rng_state,
                                                              double* __restrict__ partial) {
    __shared__ double lds[kBlock * 2 * VW];
    const int TC = 1 << tc_log2, rpb = kBlock >> tc_log2;
    const int tc = threadIdx.x & (TC - 1), tr = threadIdx.x >> tc_log2;
    const int c0 = (blockIdx.y * TC + tc) * VW;
    const bool ok = c0 < C;
    float mu[VW], rstd[VW], scale[VW], shift[VW], al[VW];
    load_cols<VW>(mu, saved, c0, C);
    load_cols<VW>(rstd, saved + C, c0, C);
    load_cols<VW>(scale, saved + 2 * C, c0, C);
    load_cols<VW>(shift, saved + 3 * C, c0, C);
    load_cols<VW>(al, alpha, c0, C);
    if (drop.p > 0.f) {
        drop.seed = rng_state[0];
        drop.step = rng_state[1];
    }
    double s1[VW], s2[VW];
#pragma unroll
    for (int k = 0; k < VW; ++k) s1[k] = s2[k] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * rpb;
    for (int64_t r = (int64_t)blockIdx.x * rpb + tr; r < N; r += stride * kUnroll) {
        F<VW> g[kUnroll], xv[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t rr = r + u * stride;
#pragma unroll
            for (int k = 0; k < VW; ++k) g[u].a[k] = xv[u].a[k] = 0.f;
            if (ok && rr < N) {
                g[u].load(dy + rr * lddy + c0);
                xv[u].load(x + rr * ldx + c0);
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t rr = r + u * stride;
            if (!ok || rr >= N) continue;
            bwd_g<VW>(g[u].a, xv[u].a, scale, shift, act, drop, rr, c0);
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                const float xhat = (xv[u].a[k] - al[k] * mu[k]) * rstd[k];
                s1[k] += (double)g[u].a[k];
                s2[k] += (double)g[u].a[k] * (double)xhat;
            }
        }
    }
    block_reduce_store<VW>(s1, s2, lds, tc, tr, TC, rpb, partial, c0, C);
}

template <int VW>
__device__ __forceinline__ void gn_bwd_apply_body(const float* __restrict__ dy, int64_t lddy,
                                                              const float* __restrict__ x, int64_t ldx,
                                                              float* __restrict__ dx, int64_t lddx,
                                                              const float* __restrict__ addend, int64_t ldadd,
                                                              int64_t N, int C, int tc_log2,
                                                              const float* __restrict__ saved,
                                                              const float* __restrict__ coef, int act, Drop drop,
                                                              const uint64_t* __restrict__ rng_state) {
    const int TC = 1 << tc_log2, rpb = kBlock >> tc_log2;
    const int tc = threadIdx.x & (TC - 1), tr = threadIdx.x >> tc_log2;
    const int c0 = (blockIdx.y * TC + tc) * VW;
    if (c0 >= C) return;
    float scale[VW], shift[VW], A[VW], Bx[VW], K[VW];
    load_cols<VW>(scale, saved + 2 * C, c0, C);
    load_cols<VW>(shift, saved + 3 * C, c0, C);
    load_cols<VW>(A, coef, c0, C);
    load_cols<VW>(Bx, coef + C, c0, C);
    load_cols<VW>(K, coef + 2 * C, c0, C);
    if (drop.p > 0.f) {
        drop.seed = rng_state[0];
        drop.step = rng_state[1];
    }
    const int64_t stride = (int64_t)gridDim.x * rpb;
    for (int64_t r = (int64_t)blockIdx.x * rpb + tr; r < N; r += stride * kUnroll) {
        F<VW> g[kUnroll], xv[kUnroll], ad[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t rr = r + u * stride;
            if (rr < N) {
                g[u].load(dy + rr * lddy + c0);
                xv[u].load(x + rr * ldx + c0);
                if (addend) ad[u].load(addend + rr * ldadd + c0);
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const int64_t rr = r + u * stride;
            if (rr >= N) continue;
            bwd_g<VW>(g[u].a, xv[u].a, scale, shift, act, drop, rr, c0);
#pragma unroll
            for (int k = 0; k < VW; ++k) {
                g[u].a[k] = fmaf(A[k], g[u].a[k], fmaf(Bx[k], xv[u].a[k], K[k]));
                if (addend) g[u].a[k] += ad[u].a[k];
            }
            g[u].store(dx + rr * lddx + c0);
        }
    }
}

static unsigned apply_blocks(int64_t n_rows, const Tiling& t) {
    int64_t b = ceil_div(n_rows, (int64_t)t.rpb * kUnroll);
    if (b < 1) b = 1;
    if (b > 4096) b = 4096;
    return (unsigned)b;
}

}  // namespace glass
