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
// This file holds what is K1s: the triple, the three operations' per-row and per-slot steps and their stores, the triple
// reduce, dt's final stage and the entry points.  The item walk (with the row handed to the operation: the backward reads its
// own row of X), its scalar form for dt, the entry-batch loop, the combines and the launches are spmm_items.h's, shared with K1m.
#include "spmm_items.h"

namespace glass {

constexpr int kSmFwdGathers = kGathers;  // U of the forward: one row per entry in flight, as K1
constexpr int kSmBwdGathers = 2;         // U of the backward: three rows per entry (dY, Y, L), a quarter of K1's
constexpr int kSmDtGathers = 4;          // U of the dt pass: one row per entry, the row's dY / Y / L live beside it

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
    __device__ __forceinline__ void to_lds(int32_t* p) const {
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            p[k] = __float_as_int(t[k].m);
            p[VW + k] = __float_as_int(t[k].z);
            p[2 * VW + k] = __float_as_int(t[k].s);
        }
    }
    __device__ __forceinline__ void from_lds(const int32_t* p) {
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            t[k].m = __int_as_float(p[k]);
            t[k].z = __int_as_float(p[VW + k]);
            t[k].s = __int_as_float(p[2 * VW + k]);
        }
    }
    __device__ __forceinline__ void merge_lds(const int32_t* p) {
#pragma unroll
        for (int k = 0; k < VW; ++k) t[k].merge(__int_as_float(p[k]), __int_as_float(p[VW + k]), __int_as_float(p[2 * VW + k]));
    }
};

// ---- forward: what a wave does with entries [e0, e1) of one row, and where a finished row goes ------------------------------
template <int VW_, int LPR_>
struct SmFwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kSmFwdGathers;
    using Acc = SmTriples<VW>;
    using Slot = RowSlot<VW>;
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

    __device__ __forceinline__ void gather(Acc& acc, int /*row*/, int e0, int e1, const ItemLanes& ln) const {
        const float* Xc = X + ln.coff;
        const float t = *t_dev;
        entry_batches<LPR, U, Slot>(
            col, val, nullptr, e0, e1, ln,
            [&](Slot& s, int c, bool ok) { load_row_if<VW>(ok, s.x, Xc + (int64_t)c * ldx); },
            [&](const Slot& s, float v, bool ok, int) {
#pragma unroll
                for (int k = 0; k < VW; ++k) acc.t[k].take(ok, v, s.x[k], __fmul_rn(t, s.x[k]));
            });
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        if (slot < 0) {
            float y[VW], l[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) acc.t[k].finish(y[k], l[k]);
            vec_from<VW>(y).store(Y + (int64_t)row * ldy + coff);
            vec_from<VW>(l).store(L + (int64_t)row * ldl + coff);
        } else {
            float m[VW], z[VW], s[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) { m[k] = acc.t[k].m; z[k] = acc.t[k].z; s[k] = acc.t[k].s; }
            const int64_t o = (int64_t)slot * H + coff;
            vec_from<VW>(m).store(pm + o);
            vec_from<VW>(z).store(pz + o);
            vec_from<VW>(s).store(ps + o);
        }
    }
};

// ---- backward: row j of the transposed CSR; its own X row once, three destination rows per entry ----------------------------
template <int VW_, int LPR_>
struct SmBwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kSmBwdGathers;
    using Acc = SumAcc<VW>;
    struct Slot {
        float g[VW], y[VW], l[VW];  // the destination's dY, Y and L rows
    };
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

    __device__ __forceinline__ void gather(Acc& acc, int row, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        const float t = *t_dev;
        float xj[VW], sj[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) xj[k] = 0.f;
        if (ln.col_ok) load_row<VW>(xj, X + (int64_t)row * ldx + ln.coff);
#pragma unroll
        for (int k = 0; k < VW; ++k) sj[k] = __fmul_rn(t, xj[k]);
        const float* dYc = dY + ln.coff;
        const float* Yc = Y + ln.coff;
        const float* Lc = L + ln.coff;
        entry_batches<LPR, U, Slot>(
            col, val, nullptr, e0, e1, ln,
            [&](Slot& s, int c, bool ok) {
                load_row_if<VW>(ok, s.g, dYc + (int64_t)c * lddy);
                load_row_if<VW>(ok, s.y, Yc + (int64_t)c * ldy);
                load_row_if<VW>(ok, s.l, Lc + (int64_t)c * ldl);
            },
            [&](const Slot& s, float v, bool ok, int) {
#pragma unroll
                for (int k = 0; k < VW; ++k) {
                    const float p = v * expf(sj[k] - s.l[k]);
                    const float term = p * s.g[k] * fmaf(t, xj[k] - s.y[k], 1.f);
                    acc.s[k] += ok ? term : 0.f;
                }
            });
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        const Vec<VW> r = vec_from<VW>(acc.s);
        r.store((slot < 0 ? dX + (int64_t)row * lddx : partials + (int64_t)slot * H) + coff);
    }
};

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

// ---- dt: the forward CSR once more; one fp64 partial per (plan item, column tile) (k1_items_sum_kernel) ---------------------
template <int VW_, int LPR_>
struct SmDtOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kSmDtGathers;
    using Slot = RowSlot<VW>;
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
    int H;

    // entries [e0, e1) of row `row`: this lane's share of sum dY p x (x - Y), added to acc
    __device__ __forceinline__ void gather(float& acc, int row, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        const float t = *t_dev;
        float gi[VW], yi[VW], li[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) gi[k] = yi[k] = li[k] = 0.f;
        if (ln.col_ok) {
            load_row<VW>(gi, dY + (int64_t)row * lddy + ln.coff);
            load_row<VW>(yi, Y + (int64_t)row * ldy + ln.coff);
            load_row<VW>(li, L + (int64_t)row * ldl + ln.coff);
        }
        const float* Xc = X + ln.coff;
        // (the row's values captured by value: by reference the compiler packs the subtractions in pairs, 2 % slower)
        entry_batches<LPR, U, Slot>(
            col, val, nullptr, e0, e1, ln,
            [=](Slot& s, int c, bool ok) { load_row_if<VW>(ok, s.x, Xc + (int64_t)c * ldx); },
            [=, &acc](const Slot& s, float v, bool ok, int) {
#pragma unroll
                for (int k = 0; k < VW; ++k) {
                    const float p = v * expf(__fmul_rn(t, s.x[k]) - li[k]);
                    const float term = gi[k] * p * s.x[k] * (s.x[k] - yi[k]);
                    acc += ok ? term : 0.f;
                }
            });
    }
};

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

template <int VW, int LPR>
static int launch_sm_fwd(SmFwdOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    launch_items(op, rowptr, hdr, plan, st);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_softmax_reduce_kernel, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, op.pm, op.pz, op.ps,
                           op.Y, op.ldy, op.L, op.ldl, op.H, plan + hdr[H_OFF_REDUCE]);
    return launch_status("glass_spmm_softmax_csr_f32");
}

template <int VW, int LPR>
static int launch_sm_bwd(SmBwdOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    launch_items(op, rowptr, hdr, plan, st);
    launch_items_reduce(op.partials, op.dX, op.lddx, op.H, hdr, plan, st);
    return launch_status("glass_spmm_softmax_bwd_f32");
}

template <int VW, int LPR>
static int launch_sm_dt(SmDtOp<VW, LPR> op, double* partials, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan,
                        hipStream_t st, float* dt) {
    const int64_t n = launch_items_sum(op, partials, rowptr, hdr, plan, st);
    hipLaunchKernelGGL(spmm_softmax_dt_final_kernel, dim3(1), dim3(kBlock), 0, st, partials, n, dt);
    return launch_status("glass_spmm_softmax_dt_f32");
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

extern "C" int glass_spmm_softmax_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                          const float* t_dev, float* Y, int64_t ldy, float* L, int64_t ldl, int64_t n_rows,
                                          int64_t H, const int32_t* hdr, const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && t_dev && Y && L && hdr && plan_dev, "spmm_softmax: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col) && aligned4(val) && aligned4(X) && aligned4(t_dev) && aligned4(Y) &&
                  aligned4(L) && aligned4(plan_dev) && aligned4(ws), "spmm_softmax: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && ldy >= H && ldl >= H,
                  "spmm_softmax: need H>0, ldx>=H, ldy>=H, ldl>=H (H=%lld ldx=%lld ldy=%lld ldl=%lld)", (long long)H,
                  (long long)ldx, (long long)ldy, (long long)ldl);
    if (const int rc = check_plan("spmm_softmax", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val), "spmm_softmax: null col/val");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_softmax: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* pm = (float*)ws;
    float* pz = pm + (int64_t)hdr[H_NSLOTS] * H;
    float* ps = pz + (int64_t)hdr[H_NSLOTS] * H;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && (ldl % 4 == 0) && aligned16(X) && aligned16(Y) &&
                     aligned16(L) && (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1S_FWD_CASE(VW, LPR)                                                                                           \
    return launch_sm_fwd(SmFwdOp<VW, LPR>{col, val, X, ldx, t_dev, Y, ldy, L, ldl, pm, pz, ps, (int)H}, rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1S_FWD_CASE);
#undef GLASS_K1S_FWD_CASE
}

extern "C" int glass_spmm_softmax_bwd_f32(const int32_t* rowptr, const int32_t* col_t, const float* val_t, const float* X,
                                          int64_t ldx, const float* t_dev, const float* dY, int64_t lddy, const float* Y,
                                          int64_t ldy, const float* L, int64_t ldl, float* dX, int64_t lddx, int64_t n_rows,
                                          int64_t H, const int32_t* hdr, const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && t_dev && dY && Y && L && dX && hdr && plan_dev, "spmm_softmax_bwd: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col_t) && aligned4(val_t) && aligned4(X) && aligned4(t_dev) && aligned4(dY) &&
                  aligned4(Y) && aligned4(L) && aligned4(dX) && aligned4(plan_dev) && aligned4(ws),
                  "spmm_softmax_bwd: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && lddy >= H && ldy >= H && ldl >= H && lddx >= H,
                  "spmm_softmax_bwd: need H>0 and every ld >= H (H=%lld ldx=%lld lddy=%lld ldy=%lld ldl=%lld lddx=%lld)",
                  (long long)H, (long long)ldx, (long long)lddy, (long long)ldy, (long long)ldl, (long long)lddx);
    if (const int rc = check_plan("spmm_softmax_bwd", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col_t && val_t), "spmm_softmax_bwd: null col_t/val_t");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_softmax_bwd: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (lddy % 4 == 0) && (ldy % 4 == 0) && (ldl % 4 == 0) && (lddx % 4 == 0) &&
                     aligned16(X) && aligned16(dY) && aligned16(Y) && aligned16(L) && aligned16(dX) &&
                     (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1S_BWD_CASE(VW, LPR)                                                                                             \
    return launch_sm_bwd(SmBwdOp<VW, LPR>{col_t, val_t, X, ldx, t_dev, dY, lddy, Y, ldy, L, ldl, dX, lddx, (float*)ws, (int)H}, \
                         rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1S_BWD_CASE);
#undef GLASS_K1S_BWD_CASE
}

extern "C" int glass_spmm_softmax_dt_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                         const float* t_dev, const float* dY, int64_t lddy, const float* Y, int64_t ldy,
                                         const float* L, int64_t ldl, float* dt, int64_t n_rows, int64_t H, const int32_t* hdr,
                                         const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && t_dev && dY && Y && L && dt && hdr && plan_dev, "spmm_softmax_dt: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col) && aligned4(val) && aligned4(X) && aligned4(t_dev) && aligned4(dY) &&
                  aligned4(Y) && aligned4(L) && aligned4(dt) && aligned4(plan_dev), "spmm_softmax_dt: pointer not 4-byte aligned");
    GLASS_REQUIRE(aligned8(ws), "spmm_softmax_dt: ws not 8-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && lddy >= H && ldy >= H && ldl >= H,
                  "spmm_softmax_dt: need H>0 and every ld >= H (H=%lld ldx=%lld lddy=%lld ldy=%lld ldl=%lld)", (long long)H,
                  (long long)ldx, (long long)lddy, (long long)ldy, (long long)ldl);
    if (const int rc = check_plan("spmm_softmax_dt", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val), "spmm_softmax_dt: null col/val");
    GLASS_REQUIRE(hdr[H_NSWEEP] + hdr[H_NLONG] == 0 || ws, "spmm_softmax_dt: plan has %d items but ws is null",
                  hdr[H_NSWEEP] + hdr[H_NLONG]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (lddy % 4 == 0) && (ldy % 4 == 0) && (ldl % 4 == 0) && aligned16(X) &&
                     aligned16(dY) && aligned16(Y) && aligned16(L);
#define GLASS_K1S_DT_CASE(VW, LPR)                                                                                             \
    return launch_sm_dt(SmDtOp<VW, LPR>{col, val, X, ldx, t_dev, dY, lddy, Y, ldy, L, ldl, (int)H}, (double*)ws, rowptr, hdr, \
                        plan_dev, st, dt)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1S_DT_CASE);
#undef GLASS_K1S_DT_CASE
}
