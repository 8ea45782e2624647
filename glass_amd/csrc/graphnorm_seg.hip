// K6s: per-graph GraphNorm over a batch of graphs (+ optional ELU / ReLU), forward and backward.
// PyG 1.7.2 GraphNorm.forward(x, batch) — the per-graph form of the call at reference GNNSeg.py:103-104,118 and
// impl/models.py:51,60.  For segment s (rows seg_ptr[s] .. seg_ptr[s + 1] - 1) and column c:
//   mu = mean_rows(x);  out = x - alpha[c] * mu;  var = mean_rows(out^2);  y = act(gamma[c] * out * rsqrt(var + eps) + beta[c])
//
// One 256-lane workgroup per segment.  Lanes run over column QUADS (TC = the power of two >= ceil(C / 4) lanes across, 256 / TC
// row slots down); lane (tr, tc) owns rows tr, tr + 256 / TC, .. of its quad in EVERY pass, adds them in row order in fp64, and
// the row slots are folded by a fixed halving tree through LDS.  Everything about a segment's arithmetic is a function of its
// row count and C alone — not of its index, its row offset or the grid — so the same rows give the same bits in any batch.
// The element-load form (C % 4, ld % 4 or a base that is not 16-byte aligned) keeps the layout and only loads differently.
// A segment of at most glass_graphnorm_seg_lds_rows(C) rows is staged in LDS by the lanes that own it (no barrier: a lane
// reads back only what it wrote), so x (backward: dy and x) is read once; a larger one re-reads global memory.
// The statistics are two-pass (mean, then squares of the shifted values).
// Parameter gradients: every segment writes its three fp64 column sums to the caller's workspace, and a second launch folds
// them over the segments in an order that depends on B alone — no float atomic, bitwise repeatable.
#include "common.h"

namespace glass {

constexpr int kSegStageFloats = 5120;  // 20 KB per staged array: forward 1 array + 8 KB tree, backward 2 arrays + 24 KB tree = 64 KB
constexpr int kSegMaxC = 512;
constexpr int kSegUnroll = 4;          // rows a lane has in flight per round of loads
constexpr int kSegFoldCols = 16, kSegFoldSlots = kBlock / kSegFoldCols, kSegFoldFly = 8;

static int seg_lds_rows(int64_t C) { return kSegStageFloats / (int)((C + 3) & ~(int64_t)3); }

static int seg_tc_log2(int64_t C) {
    int l = 0;
    while ((4ll << l) < C) ++l;
    return l;
}

template <bool VEC>
__device__ __forceinline__ void seg_load(float (&a)[4], const float* p, int c0, int C) {
    if (VEC) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        a[0] = v.x, a[1] = v.y, a[2] = v.z, a[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = c0 + k < C ? p[k] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void seg_store(float* p, const float (&a)[4], int c0, int C) {
    if (VEC) {
        *reinterpret_cast<float4*>(p) = make_float4(a[0], a[1], a[2], a[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k < C) p[k] = a[k];
    }
}

__device__ __forceinline__ void seg_cols(float (&dst)[4], const float* src, int c0, int C) {
#pragma unroll
    for (int k = 0; k < 4; ++k) dst[k] = (src && c0 + k < C) ? src[c0 + k] : 0.f;
}

__device__ __forceinline__ void seg_lds_get(float (&a)[4], const float* p) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    a[0] = v.x, a[1] = v.y, a[2] = v.z, a[3] = v.w;
}
__device__ __forceinline__ void seg_lds_put(float* p, const float (&a)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(a[0], a[1], a[2], a[3]);
}

// Fold the NS x 4 fp64 sums of every lane over the row slots: slot tr takes slot tr + h for h = rpb / 2, rpb / 4, .. 1.
// Every lane leaves with the totals of its columns.  red: kBlock * 4 * NS doubles.
template <int NS>
__device__ __forceinline__ void seg_tree(double (&s)[NS][4], double* red, int tr, int tc, int TC, int rpb) {
    double* mine = red + (size_t)threadIdx.x * (4 * NS);
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) mine[4 * j + k] = s[j][k];
    __syncthreads();
    for (int h = rpb >> 1; h > 0; h >>= 1) {
        if (tr < h) {
            const double* o = mine + (size_t)h * TC * (4 * NS);
#pragma unroll
            for (int j = 0; j < 4 * NS; ++j) mine[j] += o[j];
        }
        __syncthreads();
    }
    const double* top = red + (size_t)tc * (4 * NS);
#pragma unroll
    for (int j = 0; j < NS; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) s[j][k] = top[4 * j + k];
    __syncthreads();  // (red is written again by the next fold)
}

// the normalised value and the pre-activation value of one element: ONE formula for the forward and the backward's recomputation
// (x - alpha * mu as ONE rounding: a one-row graph has mu = x, and what is left, x * (1 - alpha), must not inherit the rounding
// of the product alpha * mu — at alpha near 1 it is that rounding)
__device__ __forceinline__ float seg_yhat(float x, float al, float mu, float rstd) { return fmaf(-al, mu, x) * rstd; }
__device__ __forceinline__ float seg_pre(float yhat, float gamma, float beta) { return fmaf(gamma, yhat, beta); }

template <bool VEC>
__global__ __launch_bounds__(kBlock) void gn_seg_fwd_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ y,
                                                            int64_t ldy, const int* __restrict__ seg_ptr, int C, int tc_log2,
                                                            int lds_rows, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ alpha,
                                                            float eps, float* __restrict__ mu_out, float* __restrict__ rstd_out,
                                                            int act) {
    __shared__ __attribute__((aligned(16))) float stage[kSegStageFloats];
    __shared__ double red[kBlock * 4];
    const int TC = 1 << tc_log2, rpb = kBlock >> tc_log2;
    const int tc = threadIdx.x & (TC - 1), tr = threadIdx.x >> tc_log2;
    const int c0 = 4 * tc, Cs = (C + 3) & ~3;
    const bool ok = c0 < C;
    const int r0 = seg_ptr[blockIdx.x], n = seg_ptr[blockIdx.x + 1] - r0;
    float* mu_s = mu_out + (size_t)blockIdx.x * C;
    float* rstd_s = rstd_out + (size_t)blockIdx.x * C;
    if (n <= 0) {  // an empty graph: no rows to write; its statistics are those of scatter_mean over nothing
        if (tr == 0 && ok)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c0 + k < C) mu_s[c0 + k] = 0.f, rstd_s[c0 + k] = (float)(1.0 / sqrt((double)eps));
        return;
    }
    const bool staged = n <= lds_rows;
    const float* xs = x + (int64_t)r0 * ldx + c0;
    float* ys = y + (int64_t)r0 * ldy + c0;
    float ga[4], be[4], al[4];
    seg_cols(ga, gamma, c0, C);
    seg_cols(be, beta, c0, C);
    seg_cols(al, alpha, c0, C);

    // pass 1: column sums (the one read of x when the segment is staged)
    double s[1][4] = {{0.0, 0.0, 0.0, 0.0}};
    if (ok)
        for (int64_t r = tr; r < n; r += kSegUnroll * rpb) {
            float v[kSegUnroll][4];
#pragma unroll
            for (int u = 0; u < kSegUnroll; ++u) {
                const int64_t rr = r + u * rpb;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[u][k] = 0.f;
                if (rr < n) seg_load<VEC>(v[u], xs + rr * ldx, c0, C);
            }
#pragma unroll
            for (int u = 0; u < kSegUnroll; ++u) {
                const int64_t rr = r + u * rpb;
                if (staged && rr < n) seg_lds_put(stage + rr * Cs + c0, v[u]);
#pragma unroll
                for (int k = 0; k < 4; ++k) s[0][k] += (double)v[u][k];
            }
        }
    seg_tree<1>(s, red, tr, tc, TC, rpb);
    float mu[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        mu[k] = (float)(s[0][k] / (double)n);
        s[0][k] = 0.0;
    }

    // pass 2: mean of the squares of the shifted values
    if (ok)
        for (int64_t r = tr; r < n; r += rpb) {
            float v[4];
            if (staged) seg_lds_get(v, stage + r * Cs + c0);
            else seg_load<VEC>(v, xs + r * ldx, c0, C);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double o = (double)v[k] - (double)al[k] * (double)mu[k];
                s[0][k] += o * o;
            }
        }
    seg_tree<1>(s, red, tr, tc, TC, rpb);
    float rstd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) rstd[k] = (float)(1.0 / sqrt(s[0][k] / (double)n + (double)eps));
    if (!ok) return;
    if (tr == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k < C) mu_s[c0 + k] = mu[k], rstd_s[c0 + k] = rstd[k];

    // pass 3: normalise, scale, shift, activate
    for (int64_t r = tr; r < n; r += rpb) {
        float v[4];
        if (staged) seg_lds_get(v, stage + r * Cs + c0);
        else seg_load<VEC>(v, xs + r * ldx, c0, C);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = act_exact(act, seg_pre(seg_yhat(v[k], al[k], mu[k], rstd[k]), ga[k], be[k]));
        seg_store<VEC>(ys + r * ldy, v, c0, C);
    }
}

// dy' (dy through the activation) and yhat of one row quad
__device__ __forceinline__ void seg_bwd_row(float (&g)[4], float (&xv)[4], const float (&al)[4], const float (&mu)[4], const float (&rstd)[4],
                                            const float (&ga)[4], const float (&be)[4], int act) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        xv[k] = seg_yhat(xv[k], al[k], mu[k], rstd[k]);
        if (act != GLASS_ACT_NONE) g[k] *= act_grad(act, seg_pre(xv[k], ga[k], be[k]));
    }
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void gn_seg_bwd_kernel(const float* __restrict__ dy, int64_t lddy, const float* __restrict__ x,
                                                            int64_t ldx, float* __restrict__ dx, int64_t lddx,
                                                            const int* __restrict__ seg_ptr, int C, int tc_log2, int lds_rows,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ alpha, const float* __restrict__ mu_in,
                                                            const float* __restrict__ rstd_in, int act,
                                                            double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float stage_g[kSegStageFloats];
    __shared__ __attribute__((aligned(16))) float stage_y[kSegStageFloats];
    __shared__ double red[kBlock * 12];
    const int TC = 1 << tc_log2, rpb = kBlock >> tc_log2;
    const int tc = threadIdx.x & (TC - 1), tr = threadIdx.x >> tc_log2;
    const int c0 = 4 * tc, Cs = (C + 3) & ~3;
    const bool ok = c0 < C;
    const int r0 = seg_ptr[blockIdx.x], n = seg_ptr[blockIdx.x + 1] - r0;
    double* part = partial + (size_t)blockIdx.x * 3 * C;  // [3][C]: dgamma, dbeta, dalpha of this segment
    if (n <= 0) {
        if (tr == 0 && ok)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c0 + k < C) part[c0 + k] = part[C + c0 + k] = part[2 * C + c0 + k] = 0.0;
        return;
    }
    const bool staged = n <= lds_rows;
    const float* gs = dy + (int64_t)r0 * lddy + c0;
    const float* xs = x + (int64_t)r0 * ldx + c0;
    float* ds = dx + (int64_t)r0 * lddx + c0;
    float ga[4], be[4], al[4], mu[4], rstd[4];
    seg_cols(ga, gamma, c0, C);
    seg_cols(be, beta, c0, C);
    seg_cols(al, alpha, c0, C);
    seg_cols(mu, mu_in + (size_t)blockIdx.x * C, c0, C);
    seg_cols(rstd, rstd_in + (size_t)blockIdx.x * C, c0, C);

    // pass 1: s[0] = sum dy', s[1] = sum dy' * yhat, s[2] = sum yhat  (sum yhat != 0 when alpha != 1)
    double s[3][4];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) s[j][k] = 0.0;
    if (ok)
        for (int64_t r = tr; r < n; r += kSegUnroll * rpb) {
            float g[kSegUnroll][4], v[kSegUnroll][4];
#pragma unroll
            for (int u = 0; u < kSegUnroll; ++u) {
                const int64_t rr = r + u * rpb;
                if (rr < n) {
                    seg_load<VEC>(g[u], gs + rr * lddy, c0, C);
                    seg_load<VEC>(v[u], xs + rr * ldx, c0, C);
                }
            }
#pragma unroll
            for (int u = 0; u < kSegUnroll; ++u) {
                const int64_t rr = r + u * rpb;
                if (rr >= n) continue;
                seg_bwd_row(g[u], v[u], al, mu, rstd, ga, be, act);
                if (staged) {
                    seg_lds_put(stage_g + rr * Cs + c0, g[u]);
                    seg_lds_put(stage_y + rr * Cs + c0, v[u]);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (c0 + k >= C) continue;  // (columns past C carry nothing)
                    s[0][k] += (double)g[u][k];
                    s[1][k] += (double)g[u][k] * (double)v[u][k];
                    s[2][k] += (double)v[u][k];
                }
            }
        }
    seg_tree<3>(s, red, tr, tc, TC, rpb);
    if (!ok) return;
    // dout = (gamma dy' - yhat * mean(gamma dy' yhat)) * rstd;  dx = dout - alpha * mean(dout) = A dy' + Bc yhat + K
    float A[4], Bc[4], K[4];
    const double inv_n = 1.0 / (double)n;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double g = (double)ga[k], r = (double)rstd[k];
        const double m2 = g * s[1][k] * inv_n;
        const double sum_dout = r * (g * s[0][k] - s[2][k] * m2);
        A[k] = (float)(g * r);
        Bc[k] = (float)(-m2 * r);
        K[k] = (float)(-(double)al[k] * sum_dout * inv_n);
        if (tr == 0 && c0 + k < C) {
            part[c0 + k] = s[1][k];
            part[C + c0 + k] = s[0][k];
            part[2 * C + c0 + k] = -(double)mu[k] * sum_dout;
        }
    }

    // pass 2: dx
    for (int64_t r = tr; r < n; r += rpb) {
        float g[4], v[4];
        if (staged) {
            seg_lds_get(g, stage_g + r * Cs + c0);
            seg_lds_get(v, stage_y + r * Cs + c0);
        } else {
            seg_load<VEC>(g, gs + r * lddy, c0, C);
            seg_load<VEC>(v, xs + r * ldx, c0, C);
            seg_bwd_row(g, v, al, mu, rstd, ga, be, act);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = fmaf(A[k], g[k], fmaf(Bc[k], v[k], K[k]));
        seg_store<VEC>(ds + r * lddx, g, c0, C);
    }
}

// Second launch: out[q][c] (+)= sum over the segments of partial[s][q][c].  Workgroup (x, q) takes 16 columns of quantity q;
// segment slot ts adds segments ts, ts + 16, .. in index order (8 in flight), the 16 slots fold by a halving tree.
__global__ __launch_bounds__(kBlock) void gn_seg_fold_kernel(const double* __restrict__ partial, int64_t B, int C,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                             float* __restrict__ dalpha, int accumulate) {
    __shared__ double lds[kBlock];
    const int tc = threadIdx.x & (kSegFoldCols - 1), ts = threadIdx.x / kSegFoldCols;
    const int c = blockIdx.x * kSegFoldCols + tc, q = blockIdx.y;
    const bool ok = c < C;
    double acc = 0.0;
    if (ok)
        for (int64_t b = ts; b < B; b += kSegFoldSlots * kSegFoldFly) {
            double v[kSegFoldFly];
#pragma unroll
            for (int u = 0; u < kSegFoldFly; ++u) {
                const int64_t bb = b + (int64_t)kSegFoldSlots * u;
                v[u] = bb < B ? partial[((size_t)bb * 3 + q) * C + c] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kSegFoldFly; ++u) acc += v[u];
        }
    lds[threadIdx.x] = acc;
    __syncthreads();
    for (int h = kSegFoldSlots >> 1; h > 0; h >>= 1) {
        if (ts < h) lds[threadIdx.x] += lds[threadIdx.x + h * kSegFoldCols];
        __syncthreads();
    }
    float* out = q == 0 ? dgamma : q == 1 ? dbeta : dalpha;
    if (ts == 0 && ok && out) out[c] = (accumulate ? out[c] : 0.f) + (float)lds[tc];
}

static bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

}  // namespace glass

using namespace glass;

extern "C" int64_t glass_graphnorm_seg_lds_rows(int64_t C) {
    if (C <= 0 || C > kSegMaxC) return GLASS_E_ARG;
    return seg_lds_rows(C);
}

extern "C" int64_t glass_graphnorm_seg_ws_bytes(int64_t B, int64_t C) {
    if (B < 0 || B >= (1ll << 31) || C <= 0 || C > kSegMaxC) return GLASS_E_ARG;
    return B * 3 * C * (int64_t)sizeof(double);
}

extern "C" int glass_graphnorm_seg_fwd_f32(const float* x, int64_t ldx, float* y, int64_t ldy, const int32_t* seg_ptr, int64_t B,
                                           int64_t C, const float* gamma, const float* beta, const float* alpha, float eps,
                                           float* mu, float* rstd, int act, void* stream) {
    GLASS_REQUIRE(x && y && seg_ptr && gamma && beta && alpha && mu && rstd, "graphnorm_seg_fwd: null pointer");
    GLASS_REQUIRE(C > 0 && C <= kSegMaxC && B >= 0 && B < (1ll << 31) && ldx >= C && ldy >= C,
                  "graphnorm_seg_fwd: bad sizes B=%lld C=%lld (C <= %d)", (long long)B, (long long)C, kSegMaxC);
    GLASS_REQUIRE(aligned4(x) && aligned4(y) && aligned4(seg_ptr) && aligned4(gamma) && aligned4(beta) && aligned4(alpha) &&
                      aligned4(mu) && aligned4(rstd),
                  "graphnorm_seg_fwd: misaligned pointer");
    GLASS_REQUIRE(act_code_ok(act), "graphnorm_seg_fwd: bad act %d", act);
    if (B == 0) return 0;
    const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && aligned16(x) && aligned16(y);
    if (vec)
        hipLaunchKernelGGL(gn_seg_fwd_kernel<true>, dim3((unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, x, ldx, y, ldy, seg_ptr,
                           (int)C, seg_tc_log2(C), seg_lds_rows(C), gamma, beta, alpha, eps, mu, rstd, act);
    else
        hipLaunchKernelGGL(gn_seg_fwd_kernel<false>, dim3((unsigned)B), dim3(kBlock), 0, (hipStream_t)stream, x, ldx, y, ldy, seg_ptr,
                           (int)C, seg_tc_log2(C), seg_lds_rows(C), gamma, beta, alpha, eps, mu, rstd, act);
    return launch_status("glass_graphnorm_seg_fwd_f32");
}

extern "C" int glass_graphnorm_seg_bwd_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dx, int64_t lddx,
                                           const int32_t* seg_ptr, int64_t B, int64_t C, const float* gamma, const float* beta,
                                           const float* alpha, const float* mu, const float* rstd, float* dgamma, float* dbeta,
                                           float* dalpha, int accumulate, int act, void* ws, void* stream) {
    GLASS_REQUIRE(dy && x && dx && seg_ptr && gamma && alpha && mu && rstd && (ws || B == 0), "graphnorm_seg_bwd: null pointer");
    GLASS_REQUIRE(act_code_ok(act), "graphnorm_seg_bwd: bad act %d", act);
    GLASS_REQUIRE(beta || act == GLASS_ACT_NONE, "graphnorm_seg_bwd: beta is needed to recompute the pre-activation values");
    GLASS_REQUIRE(C > 0 && C <= kSegMaxC && B >= 0 && B < (1ll << 31) && lddy >= C && ldx >= C && lddx >= C,
                  "graphnorm_seg_bwd: bad sizes B=%lld C=%lld (C <= %d)", (long long)B, (long long)C, kSegMaxC);
    GLASS_REQUIRE(aligned4(dy) && aligned4(x) && aligned4(dx) && aligned4(seg_ptr) && aligned4(gamma) && aligned4(beta) &&
                      aligned4(alpha) && aligned4(mu) && aligned4(rstd) && aligned4(dgamma) && aligned4(dbeta) &&
                      aligned4(dalpha) && (reinterpret_cast<uintptr_t>(ws) & 7u) == 0,
                  "graphnorm_seg_bwd: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    double* partial = (double*)ws;
    if (B > 0) {
        const bool vec = C % 4 == 0 && lddy % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0 && aligned16(dy) && aligned16(x) && aligned16(dx);
        if (vec)
            hipLaunchKernelGGL(gn_seg_bwd_kernel<true>, dim3((unsigned)B), dim3(kBlock), 0, st, dy, lddy, x, ldx, dx, lddx, seg_ptr, (int)C,
                               seg_tc_log2(C), seg_lds_rows(C), gamma, beta, alpha, mu, rstd, act, partial);
        else
            hipLaunchKernelGGL(gn_seg_bwd_kernel<false>, dim3((unsigned)B), dim3(kBlock), 0, st, dy, lddy, x, ldx, dx, lddx, seg_ptr, (int)C,
                               seg_tc_log2(C), seg_lds_rows(C), gamma, beta, alpha, mu, rstd, act, partial);
        const int rc = launch_status("glass_graphnorm_seg_bwd_f32 (segments)");
        if (rc) return rc;
    }
    if (!dgamma && !dbeta && !dalpha) return 0;
    hipLaunchKernelGGL(gn_seg_fold_kernel, dim3((unsigned)ceil_div(C, kSegFoldCols), 3), dim3(kBlock), 0, st, partial, B, (int)C, dgamma,
                       dbeta, dalpha, accumulate);
    return launch_status("glass_graphnorm_seg_bwd_f32");
}
