// K1s: softmax neighbour aggregation with a temperature (aggr "softmax", an extension: the reference has none; DeeperGCN,
// PyG's SoftmaxAggregation) on K1's CSR, plans and lane layout.  Per destination i and channel c, over the entries e of row i
// (weight v_e > 0, message x_e = X[col[e], c], temperature t = *t_dev, one fp32 scalar in device memory):
//
//   s_e = t * x_e  (one rounded fp32 multiply)      M = max_e s_e      Z = sum_e v_e exp(s_e - M)
//   Y = (sum_e v_e exp(s_e - M) x_e) / Z            L = M + log Z      (a row without entries: Y = 0, L = 0)
//
//   backward, p_e = v_e exp(t x_e - L_i)  (0 < p <= 1, sum_e p_e = 1; the exponent is formed as s - L, one exponential):
//   dX[j,c] = sum over the entries of row j of the TRANSPOSED CSR (destination i) of p dY[i,c] (1 + t (X[j,c] - Y[i,c]))
//   dt      = sum over i, c, e of dY[i,c] p_e x_e (x_e - Y[i,c])
//
// The max is always subtracted: nothing overflows while t * x is finite (the precondition; weights > 0 is the host's check).
// Forward state per lane element: the online-softmax triple (M, Z, S); a new entry costs ONE exponential, exp(-|s - M|), which
// rescales either the running sums or the entry.  Lane groups (__shfl_xor), the four waves of a long-row item (LDS) and the
// chunks of a cut row (workspace triples, a second small launch, slot order) merge their triples in a fixed order: bitwise
// repeatable for a given plan, not identical across plans (it is a sum).  The backward sums as K1m's does (lane-group
// partial sums, __shfl_xor, LDS, partial rows in slot order); dt leaves one fp64 partial per (plan item, column tile) and a
// one-workgroup launch sums them in a fixed order.  No float atomics anywhere.  Exponential and logarithm are expf / logf.
//
// The items launch is K1m's (spmm_max.hip) with the row handed to the operation: the backward reads its own row of X.
#include "common.h"
#include "spmm_common.h"
#include "spmm_sweep.h"

#include <stdint.h>

namespace glass {

constexpr int kSmFwdGathers = kGathers;  // U of the forward: one row per entry in flight, as K1
constexpr int kSmBwdGathers = 2;         // U of the backward: three rows per entry (dY, Y, L), a quarter of K1's
constexpr int kSmDtGathers = 4;          // U of the dt pass: one row per entry, the row's dY / Y / L live beside it

constexpr int64_t kSmMaxH = 65535ll * kWave;  // the grid's y extent times the columns of one scalar column tile
constexpr int kSmWaves = kBlock / kWave;

template <int VW>
__device__ __forceinline__ void sm_vec_to(const Vec<VW>& t, float (&x)[VW]) {
    if constexpr (VW == 4) { x[0] = t.v.x; x[1] = t.v.y; x[2] = t.v.z; x[3] = t.v.w; }
    else x[0] = t.v;
}
template <int VW>
__device__ __forceinline__ Vec<VW> sm_vec_from(const float (&x)[VW]) {
    Vec<VW> t;
    if constexpr (VW == 4) t.v = make_float4(x[0], x[1], x[2], x[3]);
    else t.v = x[0];
    return t;
}
template <int VW>
__device__ __forceinline__ void sm_load(float (&x)[VW], const float* p) {
    Vec<VW> t;
    t.load(p);
    sm_vec_to<VW>(t, x);
}

// ---- one (M, Z, S) triple: the softmax state of one output element ---------------------------------------------------------
struct SmTriple {
    float m, z, s;
    __device__ __forceinline__ void init() { m = -INFINITY; z = 0.f; s = 0.f; }  // no entry yet
    // one entry with weight v > 0, message x, scaled message sc = t * x (finite)
    __device__ __forceinline__ void take(bool ok, float v, float x, float sc) {
        const float d = sc - m;                  // +inf on the first entry: e = 0, the empty sums are dropped
        const float e = expf(-fabsf(d));
        const bool up = d > 0.f;                 // a new maximum: rescale the running sums, else scale the entry
        const float f = up ? e : 1.f;
        const float w = up ? v : v * e;
        const float zn = fmaf(z, f, w), sn = fmaf(s, f, w * x);
        m = (ok && up) ? sc : m;
        z = ok ? zn : z;
        s = ok ? sn : s;
    }
    // another partial of the same element (either may be empty: m = -inf, z = s = 0)
    __device__ __forceinline__ void merge(float om, float oz, float os) {
        const float nm = fmaxf(m, om);
        const float a = (m == nm) ? 1.f : expf(m - nm);
        const float b = (om == nm) ? 1.f : expf(om - nm);
        z = fmaf(z, a, oz * b);
        s = fmaf(s, a, os * b);
        m = nm;
    }
    __device__ __forceinline__ void finish(float& y, float& l) const {
        const bool any = z > 0.f;
        y = any ? s / z : 0.f;
        l = any ? m + logf(z) : 0.f;
    }
};

template <int VW>
struct SmTriples {
    SmTriple t[VW];
    static constexpr int kLdsWords = 3 * VW;
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int k = 0; k < VW; ++k) t[k].init();
    }
    __device__ __forceinline__ void xor_merge(int sh) {
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            const float om = __shfl_xor(t[k].m, sh), oz = __shfl_xor(t[k].z, sh), os = __shfl_xor(t[k].s, sh);
            t[k].merge(om, oz, os);
        }
    }
    __device__ __forceinline__ void to_lds(float* p) const {
#pragma unroll
        for (int k = 0; k < VW; ++k) { p[k] = t[k].m; p[VW + k] = t[k].z; p[2 * VW + k] = t[k].s; }
    }
    __device__ __forceinline__ void from_lds(const float* p) {
#pragma unroll
        for (int k = 0; k < VW; ++k) { t[k].m = p[k]; t[k].z = p[VW + k]; t[k].s = p[2 * VW + k]; }
    }
    __device__ __forceinline__ void merge_lds(const float* p) {
#pragma unroll
        for (int k = 0; k < VW; ++k) t[k].merge(p[k], p[VW + k], p[2 * VW + k]);
    }
};

template <int VW>
struct SmSum {
    float s[VW];
    static constexpr int kLdsWords = VW;
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int k = 0; k < VW; ++k) s[k] = 0.f;
    }
    __device__ __forceinline__ void xor_merge(int sh) {
#pragma unroll
        for (int k = 0; k < VW; ++k) s[k] += __shfl_xor(s[k], sh);
    }
    __device__ __forceinline__ void to_lds(float* p) const {
#pragma unroll
        for (int k = 0; k < VW; ++k) p[k] = s[k];
    }
    __device__ __forceinline__ void from_lds(const float* p) {
#pragma unroll
        for (int k = 0; k < VW; ++k) s[k] = p[k];
    }
    __device__ __forceinline__ void merge_lds(const float* p) {
#pragma unroll
        for (int k = 0; k < VW; ++k) s[k] += p[k];
    }
};

// ---- forward: what a wave does with entries [e0, e1) of one row, and where a finished row goes ------------------------------
template <int VW_, int LPR_>
struct SmFwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kSmFwdGathers;
    using Acc = SmTriples<VW>;
    const int32_t* col;
    const float* val;
    const float* X;
    int64_t ldx;
    const float* t_dev;
    float* Y;
    int64_t ldy;
    float* L;
    int64_t ldl;
    float* pm;   // partial triples of the chunks of cut rows: [n_slots, H] M, then Z, then S
    float* pz;
    float* ps;
    int H;

    __device__ __forceinline__ void gather(Acc& acc, int row, int e0, int e1, int lane, int grp, int coff, bool col_ok) const {
        constexpr int G = kWave / LPR;
        const float* Xc = X + coff;
        const float t = *t_dev;
        for (int eb = e0; eb < e1; eb += kWave) {
            const int cnt = min(kWave, e1 - eb);
            int my_c = 0;
            float my_v = 0.f;
            if (lane < cnt) {
                my_c = col[eb + lane];
                my_v = val[eb + lane];
            }
            for (int j = 0; j < cnt; j += U * G) {
                float x[U][VW], v[U];
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int idx = j + u * G + grp;  // < 64 + U*G: shfl wraps mod 64, masked by `ok`
                    const int c = __shfl(my_c, idx);
                    v[u] = __shfl(my_v, idx);
                    ok[u] = col_ok && idx < cnt;
                    Vec<VW> r;
                    r.zero();
                    if (ok[u]) r.load(Xc + (int64_t)c * ldx);
                    sm_vec_to<VW>(r, x[u]);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int k = 0; k < VW; ++k) acc.t[k].take(ok[u], v[u], x[u][k], __fmul_rn(t, x[u][k]));
            }
        }
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        if (slot < 0) {
            float y[VW], l[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) acc.t[k].finish(y[k], l[k]);
            sm_vec_from<VW>(y).store(Y + (int64_t)row * ldy + coff);
            sm_vec_from<VW>(l).store(L + (int64_t)row * ldl + coff);
        } else {
            float m[VW], z[VW], s[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) { m[k] = acc.t[k].m; z[k] = acc.t[k].z; s[k] = acc.t[k].s; }
            const int64_t o = (int64_t)slot * H + coff;
            sm_vec_from<VW>(m).store(pm + o);
            sm_vec_from<VW>(z).store(pz + o);
            sm_vec_from<VW>(s).store(ps + o);
        }
    }
};

// ---- backward: row j of the transposed CSR; its own X row once, three destination rows per entry ----------------------------
template <int VW_, int LPR_>
struct SmBwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kSmBwdGathers;
    using Acc = SmSum<VW>;
    const int32_t* col;   // the transposed CSR: destinations
    const float* val;
    const float* X;
    int64_t ldx;
    const float* t_dev;
    const float* dY;
    int64_t lddy;
    const float* Y;
    int64_t ldy;
    const float* L;
    int64_t ldl;
    float* dX;
    int64_t lddx;
    float* partials;      // [n_slots, H] partial rows of the chunks of cut rows
    int H;

    __device__ __forceinline__ void gather(Acc& acc, int row, int e0, int e1, int lane, int grp, int coff, bool col_ok) const {
        constexpr int G = kWave / LPR;
        if (e0 >= e1) return;  // (wave-uniform)
        const float t = *t_dev;
        float xj[VW], sj[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) xj[k] = 0.f;
        if (col_ok) sm_load<VW>(xj, X + (int64_t)row * ldx + coff);
#pragma unroll
        for (int k = 0; k < VW; ++k) sj[k] = __fmul_rn(t, xj[k]);
        const float* dYc = dY + coff;
        const float* Yc = Y + coff;
        const float* Lc = L + coff;
        for (int eb = e0; eb < e1; eb += kWave) {
            const int cnt = min(kWave, e1 - eb);
            int my_c = 0;
            float my_v = 0.f;
            if (lane < cnt) {
                my_c = col[eb + lane];
                my_v = val[eb + lane];
            }
            for (int j = 0; j < cnt; j += U * G) {
                float g[U][VW], y[U][VW], l[U][VW], v[U];
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int idx = j + u * G + grp;  // < 64 + U*G: shfl wraps mod 64, masked by `ok`
                    const int c = __shfl(my_c, idx);
                    v[u] = __shfl(my_v, idx);
                    ok[u] = col_ok && idx < cnt;
                    Vec<VW> rg, ry, rl;
                    rg.zero();
                    ry.zero();
                    rl.zero();
                    if (ok[u]) {
                        rg.load(dYc + (int64_t)c * lddy);
                        ry.load(Yc + (int64_t)c * ldy);
                        rl.load(Lc + (int64_t)c * ldl);
                    }
                    sm_vec_to<VW>(rg, g[u]);
                    sm_vec_to<VW>(ry, y[u]);
                    sm_vec_to<VW>(rl, l[u]);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int k = 0; k < VW; ++k) {
                        const float p = v[u] * expf(sj[k] - l[u][k]);
                        const float term = p * g[u][k] * fmaf(t, xj[k] - y[u][k], 1.f);
                        acc.s[k] += ok[u] ? term : 0.f;
                    }
            }
        }
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        const Vec<VW> r = sm_vec_from<VW>(acc.s);
        r.store((slot < 0 ? dX + (int64_t)row * lddx : partials + (int64_t)slot * H) + coff);
    }
};

// ---- one launch for the whole plan: sweep items (one wave each, row by row), then one workgroup per long-row item ---------
template <class Op>
__global__ __launch_bounds__(kBlock) void spmm_softmax_items_kernel(const Op op, const int32_t* __restrict__ rowptr,
                                                                    const int32_t* __restrict__ items, int n_waves,
                                                                    const int32_t* __restrict__ long_items, int n_sweep_blocks) {
    constexpr int LPR = Op::LPR, VW = Op::VW, kW = Op::Acc::kLdsWords;
    __shared__ float lds[kSmWaves * LPR * kW];
    const int lane = threadIdx.x & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = lane / LPR, sub = lane % LPR;
    const int coff = (blockIdx.y * LPR + sub) * VW;
    const bool col_ok = coff < op.H;
    typename Op::Acc acc;
    if ((int)blockIdx.x >= n_sweep_blocks) {
        const int32_t* it = long_items + 4 * (int64_t)((int)blockIdx.x - n_sweep_blocks);
        const int row = it[0], eb = it[1], ee = it[2], slot = it[3];
        // wave w takes the w-th quarter of the chunk, rounded to whole 64-entry batches
        const int per = ((ee - eb + kSmWaves * kWave - 1) / (kSmWaves * kWave)) * kWave;
        const int e0 = min(eb + w * per, ee), e1 = min(e0 + per, ee);
        acc.init();
        op.gather(acc, row, e0, e1, lane, grp, coff, col_ok);
#pragma unroll
        for (int s = LPR; s < kWave; s <<= 1) acc.xor_merge(s);
        if (grp == 0) acc.to_lds(&lds[(w * LPR + sub) * kW]);
        __syncthreads();
        if (w == 0 && grp == 0 && col_ok) {
            acc.from_lds(&lds[sub * kW]);
#pragma unroll
            for (int k = 1; k < kSmWaves; ++k) acc.merge_lds(&lds[(k * LPR + sub) * kW]);
            op.store(acc, row, slot, coff);
        }
        return;
    }
    const int wave = blockIdx.x * kSmWaves + w;
    if (wave >= n_waves) return;
    const int4 it = reinterpret_cast<const int4*>(items)[wave];
    const int r0 = __builtin_amdgcn_readfirstlane(it.x), r1 = __builtin_amdgcn_readfirstlane(it.y);
    const int e0 = __builtin_amdgcn_readfirstlane(it.z), e1 = __builtin_amdgcn_readfirstlane(it.w);
    const int nrows = r1 - r0;
    // start entry of row r0 + lane (lanes past the item hold e1)
    const int rp_reg = (lane < nrows) ? rowptr[r0 + lane] : e1;
    int es = e0;
    for (int i = 0; i < nrows; ++i) {
        const int ee = (i + 1 < nrows) ? __builtin_amdgcn_readlane(rp_reg, i + 1) : e1;
        acc.init();
        op.gather(acc, r0 + i, es, ee, lane, grp, coff, col_ok);
#pragma unroll
        for (int s = LPR; s < kWave; s <<= 1) acc.xor_merge(s);
        if (grp == 0 && col_ok) op.store(acc, r0 + i, -1, coff);
        es = ee;
    }
}

// ---- rows cut into several chunks: their partial triples merged slot by slot -------------------------------------------------
__global__ __launch_bounds__(kBlock) void spmm_softmax_reduce_kernel(const float* __restrict__ pm, const float* __restrict__ pz,
                                                                     const float* __restrict__ ps, float* __restrict__ Y,
                                                                     int64_t ldy, float* __restrict__ L, int64_t ldl, int H,
                                                                     const int32_t* __restrict__ rrows) {
    const int32_t* rr = rrows + 3 * (int64_t)blockIdx.x;
    const int row = rr[0], first = rr[1], n = rr[2];
    for (int c = threadIdx.x; c < H; c += kBlock) {
        SmTriple p;
        p.init();
        for (int k = 0; k < n; ++k) {
            const int64_t o = (int64_t)(first + k) * H + c;
            p.merge(pm[o], pz[o], ps[o]);
        }
        float y, l;
        p.finish(y, l);
        Y[(int64_t)row * ldy + c] = y;
        L[(int64_t)row * ldl + c] = l;
    }
}

__global__ __launch_bounds__(kBlock) void spmm_softmax_bwd_reduce_kernel(const float* __restrict__ partials, float* __restrict__ dX,
                                                                         int64_t ldx, int H, const int32_t* __restrict__ rrows) {
    spmm_reduce_body(partials, dX, ldx, H, rrows);
}

// ---- dt: the forward CSR once more; one fp64 partial per (plan item, column tile) ------------------------------------------
template <int VW_, int LPR_>
struct SmDtOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kSmDtGathers;
    const int32_t* col;
    const float* val;
    const float* X;
    int64_t ldx;
    const float* t_dev;
    const float* dY;
    int64_t lddy;
    const float* Y;
    int64_t ldy;
    const float* L;
    int64_t ldl;
    double* partials;   // [n_ctiles, n_items]
    int H;

    // entries [e0, e1) of row `row`: this lane's share of sum dY p x (x - Y), added to acc
    __device__ __forceinline__ void gather(float& acc, int row, int e0, int e1, int lane, int grp, int coff, bool col_ok) const {
        constexpr int G = kWave / LPR;
        if (e0 >= e1) return;  // (wave-uniform)
        const float t = *t_dev;
        float gi[VW], yi[VW], li[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) gi[k] = yi[k] = li[k] = 0.f;
        if (col_ok) {
            sm_load<VW>(gi, dY + (int64_t)row * lddy + coff);
            sm_load<VW>(yi, Y + (int64_t)row * ldy + coff);
            sm_load<VW>(li, L + (int64_t)row * ldl + coff);
        }
        const float* Xc = X + coff;
        for (int eb = e0; eb < e1; eb += kWave) {
            const int cnt = min(kWave, e1 - eb);
            int my_c = 0;
            float my_v = 0.f;
            if (lane < cnt) {
                my_c = col[eb + lane];
                my_v = val[eb + lane];
            }
            for (int j = 0; j < cnt; j += U * G) {
                float x[U][VW], v[U];
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int idx = j + u * G + grp;  // < 64 + U*G: shfl wraps mod 64, masked by `ok`
                    const int c = __shfl(my_c, idx);
                    v[u] = __shfl(my_v, idx);
                    ok[u] = col_ok && idx < cnt;
                    Vec<VW> r;
                    r.zero();
                    if (ok[u]) r.load(Xc + (int64_t)c * ldx);
                    sm_vec_to<VW>(r, x[u]);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int k = 0; k < VW; ++k) {
                        const float p = v[u] * expf(__fmul_rn(t, x[u][k]) - li[k]);
                        const float term = gi[k] * p * x[u][k] * (x[u][k] - yi[k]);
                        acc += ok[u] ? term : 0.f;
                    }
            }
        }
    }
};

__device__ __forceinline__ double sm_wave_sum(double a) {
#pragma unroll
    for (int s = 1; s < kWave; s <<= 1) a += __shfl_xor(a, s);
    return a;
}

template <class Op>
__global__ __launch_bounds__(kBlock) void spmm_softmax_dt_items_kernel(const Op op, const int32_t* __restrict__ rowptr,
                                                                       const int32_t* __restrict__ items, int n_waves,
                                                                       const int32_t* __restrict__ long_items, int n_sweep_blocks,
                                                                       int n_items) {
    constexpr int LPR = Op::LPR, VW = Op::VW;
    __shared__ double lds[kSmWaves];
    const int lane = threadIdx.x & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = lane / LPR, sub = lane % LPR;
    const int coff = (blockIdx.y * LPR + sub) * VW;
    const bool col_ok = coff < op.H;
    double* out = op.partials + (int64_t)blockIdx.y * n_items;
    float acc = 0.f;
    if ((int)blockIdx.x >= n_sweep_blocks) {
        const int li = (int)blockIdx.x - n_sweep_blocks;
        const int32_t* it = long_items + 4 * (int64_t)li;
        const int row = it[0], eb = it[1], ee = it[2];
        const int per = ((ee - eb + kSmWaves * kWave - 1) / (kSmWaves * kWave)) * kWave;
        const int e0 = min(eb + w * per, ee), e1 = min(e0 + per, ee);
        op.gather(acc, row, e0, e1, lane, grp, coff, col_ok);
        const double s = sm_wave_sum((double)acc);
        if (lane == 0) lds[w] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot = lds[0];
#pragma unroll
            for (int k = 1; k < kSmWaves; ++k) tot += lds[k];
            out[n_waves + li] = tot;
        }
        return;
    }
    const int wave = blockIdx.x * kSmWaves + w;
    if (wave >= n_waves) return;
    const int4 it = reinterpret_cast<const int4*>(items)[wave];
    const int r0 = __builtin_amdgcn_readfirstlane(it.x), r1 = __builtin_amdgcn_readfirstlane(it.y);
    const int e0 = __builtin_amdgcn_readfirstlane(it.z), e1 = __builtin_amdgcn_readfirstlane(it.w);
    const int nrows = r1 - r0;
    const int rp_reg = (lane < nrows) ? rowptr[r0 + lane] : e1;
    int es = e0;
    double tot = 0.0;
    for (int i = 0; i < nrows; ++i) {
        const int ee = (i + 1 < nrows) ? __builtin_amdgcn_readlane(rp_reg, i + 1) : e1;
        acc = 0.f;
        op.gather(acc, r0 + i, es, ee, lane, grp, coff, col_ok);
        tot += (double)acc;   // one row's fp32 share of this lane, rows added in fp64
        es = ee;
    }
    tot = sm_wave_sum(tot);
    if (lane == 0) out[wave] = tot;
}

// the partials in a fixed order: thread k takes k, k + 256, ...; then a tree over the workgroup
__global__ __launch_bounds__(kBlock) void spmm_softmax_dt_final_kernel(const double* __restrict__ partials, int64_t n,
                                                                       float* __restrict__ dt) {
    __shared__ double lds[kBlock];
    double s = 0.0;
    for (int64_t k = threadIdx.x; k < n; k += kBlock) s += partials[k];
    lds[threadIdx.x] = s;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) lds[threadIdx.x] += lds[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) *dt = (float)lds[0];
}

template <class Op>
static void sm_launch_items(const Op& op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    const int n_ctiles = (int)ceil_div(op.H, (int64_t)Op::LPR * Op::VW);
    const int n_waves = hdr[H_NSWEEP];
    const int n_sweep_blocks = (int)ceil_div(n_waves, kSmWaves);
    const unsigned blocks = (unsigned)(n_sweep_blocks + hdr[H_NLONG]);  // sweep workgroups, then one per long-row item
    if (blocks == 0) return;
    hipLaunchKernelGGL((spmm_softmax_items_kernel<Op>), dim3(blocks, n_ctiles), dim3(kBlock), 0, st, op, rowptr,
                       plan + hdr[H_OFF_SWEEP], n_waves, plan + hdr[H_OFF_LONG], n_sweep_blocks);
}

template <int VW, int LPR>
static int launch_sm_fwd(SmFwdOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    sm_launch_items(op, rowptr, hdr, plan, st);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_softmax_reduce_kernel, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, op.pm, op.pz, op.ps,
                           op.Y, op.ldy, op.L, op.ldl, op.H, plan + hdr[H_OFF_REDUCE]);
    return launch_status("glass_spmm_softmax_csr_f32");
}

template <int VW, int LPR>
static int launch_sm_bwd(SmBwdOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    sm_launch_items(op, rowptr, hdr, plan, st);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_softmax_bwd_reduce_kernel, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, op.partials,
                           op.dX, op.lddx, op.H, plan + hdr[H_OFF_REDUCE]);
    return launch_status("glass_spmm_softmax_bwd_f32");
}

template <int VW, int LPR>
static int launch_sm_dt(SmDtOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st,
                        float* dt) {
    const int n_ctiles = (int)ceil_div(op.H, (int64_t)LPR * VW);
    const int n_waves = hdr[H_NSWEEP];
    const int n_sweep_blocks = (int)ceil_div(n_waves, kSmWaves);
    const int n_items = n_waves + hdr[H_NLONG];
    const unsigned blocks = (unsigned)(n_sweep_blocks + hdr[H_NLONG]);
    if (blocks > 0)
        hipLaunchKernelGGL((spmm_softmax_dt_items_kernel<SmDtOp<VW, LPR>>), dim3(blocks, n_ctiles), dim3(kBlock), 0, st, op, rowptr,
                           plan + hdr[H_OFF_SWEEP], n_waves, plan + hdr[H_OFF_LONG], n_sweep_blocks, n_items);
    hipLaunchKernelGGL(spmm_softmax_dt_final_kernel, dim3(1), dim3(kBlock), 0, st, op.partials, (int64_t)n_items * n_ctiles, dt);
    return launch_status("glass_spmm_softmax_dt_f32");
}

inline bool sm_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool sm_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// what the three entries ask of the plan header and the width; 0, or the code to return
static int sm_check_plan(const char* what, const int32_t* hdr, int64_t n_rows, int64_t H) {
    if (hdr[H_MAGIC] != kPlanMagic || hdr[H_VER] != kPlanVersion || hdr[H_NROWS] != n_rows) {
        set_error("%s: plan does not match (magic %x, rows %d vs %lld)", what, hdr[H_MAGIC], hdr[H_NROWS], (long long)n_rows);
        return GLASS_E_PLAN;
    }
    if (H > kSmMaxH) {
        set_error("%s: H = %lld is beyond the %lld columns one launch covers", what, (long long)H, (long long)kSmMaxH);
        return GLASS_E_UNSUPPORTED;
    }
    return 0;
}

}  // namespace glass

using namespace glass;

extern "C" int64_t glass_spmm_softmax_ws_bytes(const int32_t* hdr, int64_t H) {
    if (!hdr || hdr[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr[H_NSLOTS] * H * 3 * (int64_t)sizeof(float);
}

extern "C" int64_t glass_spmm_softmax_bwd_ws_bytes(const int32_t* hdr_t, int64_t H) {
    if (!hdr_t || hdr_t[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr_t[H_NSLOTS] * H * (int64_t)sizeof(float);
}

// one fp64 partial per plan item and column tile, sized for the scalar form's 64-column tiles (the vector form has fewer)
extern "C" int64_t glass_spmm_softmax_dt_ws_bytes(const int32_t* hdr, int64_t H) {
    if (!hdr || hdr[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return ((int64_t)hdr[H_NSWEEP] + hdr[H_NLONG]) * ceil_div(H, kWave) * (int64_t)sizeof(double);
}

#define GLASS_K1S_DISPATCH(OP, LAUNCH, TAIL, ...)                                              \
    if (vec) {                                                                                 \
        switch (pow2_ceil_cap(H / 4, 64)) {                                                    \
            case 1: return LAUNCH(OP<4, 1>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);      \
            case 2: return LAUNCH(OP<4, 2>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);      \
            case 4: return LAUNCH(OP<4, 4>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);      \
            case 8: return LAUNCH(OP<4, 8>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);      \
            case 16: return LAUNCH(OP<4, 16>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);    \
            case 32: return LAUNCH(OP<4, 32>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);    \
            default: return LAUNCH(OP<4, 64>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);    \
        }                                                                                      \
    }                                                                                          \
    switch (pow2_ceil_cap(H, 64)) {                                                            \
        case 1: return LAUNCH(OP<1, 1>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);          \
        case 2: return LAUNCH(OP<1, 2>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);          \
        case 4: return LAUNCH(OP<1, 4>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);          \
        case 8: return LAUNCH(OP<1, 8>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);          \
        case 16: return LAUNCH(OP<1, 16>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);        \
        case 32: return LAUNCH(OP<1, 32>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);        \
        default: return LAUNCH(OP<1, 64>{__VA_ARGS__}, rowptr, hdr, plan_dev, st TAIL);        \
    }

#define GLASS_K1S_NO_TAIL
#define GLASS_K1S_DT_TAIL , dt

extern "C" int glass_spmm_softmax_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                          const float* t_dev, float* Y, int64_t ldy, float* L, int64_t ldl, int64_t n_rows,
                                          int64_t H, const int32_t* hdr, const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && t_dev && Y && L && hdr && plan_dev, "spmm_softmax: null pointer");
    GLASS_REQUIRE(sm_aligned4(rowptr) && sm_aligned4(col) && sm_aligned4(val) && sm_aligned4(X) && sm_aligned4(t_dev) &&
                  sm_aligned4(Y) && sm_aligned4(L) && sm_aligned4(plan_dev) && sm_aligned4(ws),
                  "spmm_softmax: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && ldy >= H && ldl >= H,
                  "spmm_softmax: need H>0, ldx>=H, ldy>=H, ldl>=H (H=%lld ldx=%lld ldy=%lld ldl=%lld)", (long long)H,
                  (long long)ldx, (long long)ldy, (long long)ldl);
    if (const int rc = sm_check_plan("spmm_softmax", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val), "spmm_softmax: null col/val");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_softmax: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* pm = (float*)ws;
    float* pz = pm + (int64_t)hdr[H_NSLOTS] * H;
    float* ps = pz + (int64_t)hdr[H_NSLOTS] * H;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && (ldl % 4 == 0) && aligned16(X) && aligned16(Y) &&
                     aligned16(L) && (hdr[H_NSLOTS] == 0 || aligned16(ws));
    GLASS_K1S_DISPATCH(SmFwdOp, launch_sm_fwd, GLASS_K1S_NO_TAIL, col, val, X, ldx, t_dev, Y, ldy, L, ldl, pm, pz, ps, (int)H)
}

extern "C" int glass_spmm_softmax_bwd_f32(const int32_t* rowptr, const int32_t* col_t, const float* val_t, const float* X,
                                          int64_t ldx, const float* t_dev, const float* dY, int64_t lddy, const float* Y,
                                          int64_t ldy, const float* L, int64_t ldl, float* dX, int64_t lddx, int64_t n_rows,
                                          int64_t H, const int32_t* hdr, const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && t_dev && dY && Y && L && dX && hdr && plan_dev, "spmm_softmax_bwd: null pointer");
    GLASS_REQUIRE(sm_aligned4(rowptr) && sm_aligned4(col_t) && sm_aligned4(val_t) && sm_aligned4(X) && sm_aligned4(t_dev) &&
                  sm_aligned4(dY) && sm_aligned4(Y) && sm_aligned4(L) && sm_aligned4(dX) && sm_aligned4(plan_dev) &&
                  sm_aligned4(ws), "spmm_softmax_bwd: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && lddy >= H && ldy >= H && ldl >= H && lddx >= H,
                  "spmm_softmax_bwd: need H>0 and every ld >= H (H=%lld ldx=%lld lddy=%lld ldy=%lld ldl=%lld lddx=%lld)",
                  (long long)H, (long long)ldx, (long long)lddy, (long long)ldy, (long long)ldl, (long long)lddx);
    if (const int rc = sm_check_plan("spmm_softmax_bwd", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col_t && val_t), "spmm_softmax_bwd: null col_t/val_t");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_softmax_bwd: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (lddy % 4 == 0) && (ldy % 4 == 0) && (ldl % 4 == 0) && (lddx % 4 == 0) &&
                     aligned16(X) && aligned16(dY) && aligned16(Y) && aligned16(L) && aligned16(dX) &&
                     (hdr[H_NSLOTS] == 0 || aligned16(ws));
    GLASS_K1S_DISPATCH(SmBwdOp, launch_sm_bwd, GLASS_K1S_NO_TAIL, col_t, val_t, X, ldx, t_dev, dY, lddy, Y, ldy, L, ldl, dX, lddx,
                       (float*)ws, (int)H)
}

extern "C" int glass_spmm_softmax_dt_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                         const float* t_dev, const float* dY, int64_t lddy, const float* Y, int64_t ldy,
                                         const float* L, int64_t ldl, float* dt, int64_t n_rows, int64_t H, const int32_t* hdr,
                                         const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && t_dev && dY && Y && L && dt && hdr && plan_dev, "spmm_softmax_dt: null pointer");
    GLASS_REQUIRE(sm_aligned4(rowptr) && sm_aligned4(col) && sm_aligned4(val) && sm_aligned4(X) && sm_aligned4(t_dev) &&
                  sm_aligned4(dY) && sm_aligned4(Y) && sm_aligned4(L) && sm_aligned4(dt) && sm_aligned4(plan_dev),
                  "spmm_softmax_dt: pointer not 4-byte aligned");
    GLASS_REQUIRE(sm_aligned8(ws), "spmm_softmax_dt: ws not 8-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && lddy >= H && ldy >= H && ldl >= H,
                  "spmm_softmax_dt: need H>0 and every ld >= H (H=%lld ldx=%lld lddy=%lld ldy=%lld ldl=%lld)", (long long)H,
                  (long long)ldx, (long long)lddy, (long long)ldy, (long long)ldl);
    if (const int rc = sm_check_plan("spmm_softmax_dt", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val), "spmm_softmax_dt: null col/val");
    GLASS_REQUIRE(hdr[H_NSWEEP] + hdr[H_NLONG] == 0 || ws, "spmm_softmax_dt: plan has %d items but ws is null",
                  hdr[H_NSWEEP] + hdr[H_NLONG]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (lddy % 4 == 0) && (ldy % 4 == 0) && (ldl % 4 == 0) && aligned16(X) &&
                     aligned16(dY) && aligned16(Y) && aligned16(L);
    GLASS_K1S_DISPATCH(SmDtOp, launch_sm_dt, GLASS_K1S_DT_TAIL, col, val, X, ldx, t_dev, dY, lddy, Y, ldy, L, ldl, (double*)ws,
                       (int)H)
}
