// K1v: standard-deviation and variance neighbour aggregation (aggr "std" / "var", an extension: the reference has none; PNA,
// PyG's StdAggregation / VarAggregation) on K1's CSR, plans and lane layout.  Per destination i and channel c, over the entries
// e of row i (weight w_e > 0, a multiplicity; message x_e = X[col[e], c]):
//
//   W = sum_e w_e      Mu = sum_e w_e x_e / W      Var = sum_e w_e (x_e - Mu)^2 / W      Std = sqrt(Var + eps)
//   (a row without entries: W = Mu = Var = Std = 0)
//
//   backward, on the TRANSPOSED CSR (row j = source, entries = destinations i, val_t), with A and C [n, H] from the caller
//   (std: A = dS / (W S); var: A = 2 dS / W; C = dMu / W; 0 where W = 0):
//   dX[j,c] = sum_e val_t[e] (C[i,c] + A[i,c] (X[j,c] - Mu[i,c]))
//
// One pass, every source row gathered once.  Forward state per lane: the triple (W, mean, M2), W shared by the lane's VW
// channels.  An entry is the triple (w, x, 0); entries, lane groups (__shfl_xor), the four waves of a long-row item (LDS) and
// the chunks of a cut row (workspace triples, a second small launch, slot order) all merge with Chan's update
//
//   d = m_b - m_a    W = W_a + W_b    f = W_b / W    m = m_a + d f    M2 = M2_a + M2_b + d^2 (W_a f)      (empty side: identity)
//
// in a fixed order: bitwise repeatable for a given plan, not identical across plans.  No x^2 is ever formed: a row whose
// messages are all equal has d = 0 at every merge and Var == 0 exactly.  The backward forms X - Mu per entry (never the
// factored X * sum(wA) - sum(wA Mu), which cancels) and sums as K1s's does.  No float atomics anywhere.
//
// The item walk, the entry-batch loop, the combines and the launches are spmm_items.h's, shared with K1m and K1s.
#include "spmm_items.h"

namespace glass {

constexpr int kMomFwdGathers = kGathers;  // U of the forward: one row per entry in flight, as K1
constexpr int kMomBwdGathers = 2;         // U of the backward: two or three rows per entry (A, Mu, C)

// ---- Chan's update of one (W, mean, M2) by another; W and f are shared by the channels of a lane ---------------------------
struct MomStep {
    float W, f, g;  // the merged weight, W_b / W and W_a * f
    __device__ __forceinline__ MomStep(float wa, float wb) {
        W = wa + wb;
        f = W > 0.f ? wb / W : 0.f;  // both sides empty: nothing moves
        g = wa * f;
    }
    __device__ __forceinline__ void apply(float& m, float& q, float mb, float qb) const {
        const float d = mb - m;
        m = fmaf(d, f, m);
        q = (q + qb) + (d * d) * g;
    }
};

template <int VW>
struct MomAcc {
    float W;
    float m[VW], q[VW];
    static constexpr int kLdsWords = 2 * VW + 1;
    __device__ __forceinline__ void init() {
        W = 0.f;
#pragma unroll
        for (int k = 0; k < VW; ++k) m[k] = q[k] = 0.f;
    }
    // one entry: the triple (v, x, 0)
    __device__ __forceinline__ void take(bool ok, float v, const float (&x)[VW]) {
        const MomStep s(W, v);
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            float mn = m[k], qn = q[k];
            s.apply(mn, qn, x[k], 0.f);
            m[k] = ok ? mn : m[k];
            q[k] = ok ? qn : q[k];
        }
        W = ok ? s.W : W;
    }
    __device__ __forceinline__ void xor_merge(int sh) {
        const MomStep s(W, __shfl_xor(W, sh));
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            const float om = __shfl_xor(m[k], sh), oq = __shfl_xor(q[k], sh);
            s.apply(m[k], q[k], om, oq);
        }
        W = s.W;
    }
    __device__ __forceinline__ void to_lds(int32_t* p) const {
        p[0] = __float_as_int(W);
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            p[1 + k] = __float_as_int(m[k]);
            p[1 + VW + k] = __float_as_int(q[k]);
        }
    }
    __device__ __forceinline__ void from_lds(const int32_t* p) {
        W = __int_as_float(p[0]);
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            m[k] = __int_as_float(p[1 + k]);
            q[k] = __int_as_float(p[1 + VW + k]);
        }
    }
    __device__ __forceinline__ void merge_lds(const int32_t* p) {
        const MomStep s(W, __int_as_float(p[0]));
#pragma unroll
        for (int k = 0; k < VW; ++k) s.apply(m[k], q[k], __int_as_float(p[1 + k]), __int_as_float(p[1 + VW + k]));
        W = s.W;
    }
};

// (S, Mu) of a finished triple; kind 0 = std, 1 = var
__device__ __forceinline__ void mom_finish(float W, float m, float q, float eps, int kind, float& s, float& mu) {
    const bool any = W > 0.f;
    const float var = any ? q / W : 0.f;
    mu = any ? m : 0.f;
    s = !any ? 0.f : (kind == 0 ? sqrtf(var + eps) : var);
}

// ---- forward: what a wave does with entries [e0, e1) of one row, and where a finished row goes ------------------------------
template <int VW_, int LPR_>
struct MomFwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kMomFwdGathers;
    using Acc = MomAcc<VW>;
    using Slot = RowSlot<VW>;
    const int32_t* col;
    const float* val;
    const float* X;
    int64_t ldx;
    float eps;
    int kind;
    float* S;
    int64_t lds_;
    float* Mu;
    int64_t ldmu;
    float* Wsum;
    float* pm;   // partial triples of the chunks of cut rows: [n_slots, H] mean, then M2, then [n_slots] W
    float* pq;
    float* pw;
    int H;

    __device__ __forceinline__ void gather(Acc& acc, int /*row*/, int e0, int e1, const ItemLanes& ln) const {
        const float* Xc = X + ln.coff;
        entry_batches<LPR, U, Slot>(
            col, val, nullptr, e0, e1, ln,
            [&](Slot& s, int c, bool ok) { load_row_if<VW>(ok, s.x, Xc + (int64_t)c * ldx); },
            [&](const Slot& s, float v, bool ok, int) { acc.take(ok, v, s.x); });
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        if (slot < 0) {
            float s[VW], mu[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) mom_finish(acc.W, acc.m[k], acc.q[k], eps, kind, s[k], mu[k]);
            vec_from<VW>(s).store(S + (int64_t)row * lds_ + coff);
            vec_from<VW>(mu).store(Mu + (int64_t)row * ldmu + coff);
            if (coff == 0) Wsum[row] = acc.W;
        } else {
            const int64_t o = (int64_t)slot * H + coff;
            vec_from<VW>(acc.m).store(pm + o);
            vec_from<VW>(acc.q).store(pq + o);
            if (coff == 0) pw[slot] = acc.W;
        }
    }
};

// ---- backward: row j of the transposed CSR; its own X row once, two or three destination rows per entry ---------------------
template <int VW_, int LPR_, bool HASC>
struct MomBwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kMomBwdGathers;
    using Acc = SumAcc<VW>;
    struct Slot {
        float a[VW], mu[VW], c[HASC ? VW : 1];  // the destination's A, Mu and C rows
    };
    const int32_t* col;   // the transposed CSR: destinations
    const float* val;
    const float* X;
    int64_t ldx;
    const float* Mu;
    int64_t ldmu;
    const float* A;
    int64_t lda;
    const float* C;
    int64_t ldc;
    float* dX;
    int64_t lddx;
    float* partials;      // [n_slots, H] partial rows of the chunks of cut rows
    int H;

    __device__ __forceinline__ void gather(Acc& acc, int row, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        float xj[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) xj[k] = 0.f;
        if (ln.col_ok) load_row<VW>(xj, X + (int64_t)row * ldx + ln.coff);
        const float* Ac = A + ln.coff;
        const float* Mc = Mu + ln.coff;
        const float* Cc = HASC ? C + ln.coff : nullptr;
        entry_batches<LPR, U, Slot>(
            col, val, nullptr, e0, e1, ln,
            [&](Slot& s, int c, bool ok) {
                load_row_if<VW>(ok, s.a, Ac + (int64_t)c * lda);
                load_row_if<VW>(ok, s.mu, Mc + (int64_t)c * ldmu);
                if constexpr (HASC) load_row_if<VW>(ok, s.c, Cc + (int64_t)c * ldc);
            },
            [&](const Slot& s, float v, bool ok, int) {
#pragma unroll
                for (int k = 0; k < VW; ++k) {
                    const float d = xj[k] - s.mu[k];  // per entry: never factored out of the sum
                    float term;
                    if constexpr (HASC) term = v * fmaf(s.a[k], d, s.c[k]);
                    else term = v * (s.a[k] * d);
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
__global__ __launch_bounds__(kBlock) void spmm_moment_reduce_kernel(const float* __restrict__ pm, const float* __restrict__ pq,
                                                                    const float* __restrict__ pw, float eps, int kind,
                                                                    float* __restrict__ S, int64_t lds_, float* __restrict__ Mu,
                                                                    int64_t ldmu, float* __restrict__ Wsum, int H,
                                                                    const int32_t* __restrict__ rrows) {
    const int32_t* rr = rrows + 3 * (int64_t)blockIdx.x;
    const int row = rr[0], first = rr[1], n = rr[2];
    for (int c = threadIdx.x; c < H; c += kBlock) {
        float W = 0.f, m = 0.f, q = 0.f;
        for (int k = 0; k < n; ++k) {
            const int64_t o = (int64_t)(first + k) * H + c;
            const MomStep s(W, pw[first + k]);
            s.apply(m, q, pm[o], pq[o]);
            W = s.W;
        }
        float sv, mu;
        mom_finish(W, m, q, eps, kind, sv, mu);
        S[(int64_t)row * lds_ + c] = sv;
        Mu[(int64_t)row * ldmu + c] = mu;
        if (c == 0) Wsum[row] = W;
    }
}

template <int VW, int LPR>
static int launch_mom_fwd(MomFwdOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    launch_items(op, rowptr, hdr, plan, st);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_moment_reduce_kernel, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, op.pm, op.pq, op.pw,
                           op.eps, op.kind, op.S, op.lds_, op.Mu, op.ldmu, op.Wsum, op.H, plan + hdr[H_OFF_REDUCE]);
    return launch_status("glass_spmm_moment_csr_f32");
}

template <int VW, int LPR, bool HASC>
static int launch_mom_bwd(MomBwdOp<VW, LPR, HASC> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan,
                          hipStream_t st) {
    launch_items(op, rowptr, hdr, plan, st);
    launch_items_reduce(op.partials, op.dX, op.lddx, op.H, hdr, plan, st);
    return launch_status("glass_spmm_moment_bwd_f32");
}

}  // namespace glass

using namespace glass;

// per partial slot: H means, H M2 and one W
extern "C" int64_t glass_spmm_moment_ws_bytes(const int32_t* hdr, int64_t H) {
    if (!hdr || hdr[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr[H_NSLOTS] * (2 * H + 1) * (int64_t)sizeof(float);
}

extern "C" int64_t glass_spmm_moment_bwd_ws_bytes(const int32_t* hdr_t, int64_t H) {
    if (!hdr_t || hdr_t[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr_t[H_NSLOTS] * H * (int64_t)sizeof(float);
}

extern "C" int glass_spmm_moment_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                         float eps, int kind, float* S, int64_t lds, float* Mu, int64_t ldmu, float* Wsum,
                                         int64_t n_rows, int64_t H, const int32_t* hdr, const int32_t* plan_dev, void* ws,
                                         void* stream) {
    GLASS_REQUIRE(rowptr && X && S && Mu && Wsum && hdr && plan_dev, "spmm_moment: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col) && aligned4(val) && aligned4(X) && aligned4(S) && aligned4(Mu) &&
                  aligned4(Wsum) && aligned4(plan_dev) && aligned4(ws), "spmm_moment: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && lds >= H && ldmu >= H,
                  "spmm_moment: need H>0, ldx>=H, lds>=H, ldmu>=H (H=%lld ldx=%lld lds=%lld ldmu=%lld)", (long long)H,
                  (long long)ldx, (long long)lds, (long long)ldmu);
    GLASS_REQUIRE(kind == 0 || kind == 1, "spmm_moment: kind %d is neither 0 (std) nor 1 (var)", kind);
    GLASS_REQUIRE(eps >= 0.f, "spmm_moment: eps must be >= 0");
    if (const int rc = check_plan("spmm_moment", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val), "spmm_moment: null col/val");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_moment: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* pm = (float*)ws;
    float* pq = pm + (int64_t)hdr[H_NSLOTS] * H;
    float* pw = pq + (int64_t)hdr[H_NSLOTS] * H;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (lds % 4 == 0) && (ldmu % 4 == 0) && aligned16(X) && aligned16(S) &&
                     aligned16(Mu) && (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1V_FWD_CASE(VW, LPR)                                                                                         \
    return launch_mom_fwd(MomFwdOp<VW, LPR>{col, val, X, ldx, eps, kind, S, lds, Mu, ldmu, Wsum, pm, pq, pw, (int)H}, rowptr, \
                          hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1V_FWD_CASE);
#undef GLASS_K1V_FWD_CASE
}

extern "C" int glass_spmm_moment_bwd_f32(const int32_t* rowptr, const int32_t* col_t, const float* val_t, const float* X,
                                         int64_t ldx, const float* Mu, int64_t ldmu, const float* A, int64_t lda, const float* C,
                                         int64_t ldc, float* dX, int64_t lddx, int64_t n_rows, int64_t H, const int32_t* hdr,
                                         const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && Mu && A && dX && hdr && plan_dev, "spmm_moment_bwd: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col_t) && aligned4(val_t) && aligned4(X) && aligned4(Mu) && aligned4(A) &&
                  aligned4(C) && aligned4(dX) && aligned4(plan_dev) && aligned4(ws), "spmm_moment_bwd: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && ldmu >= H && lda >= H && (!C || ldc >= H) && lddx >= H,
                  "spmm_moment_bwd: need H>0 and every ld >= H (H=%lld ldx=%lld ldmu=%lld lda=%lld ldc=%lld lddx=%lld)",
                  (long long)H, (long long)ldx, (long long)ldmu, (long long)lda, (long long)ldc, (long long)lddx);
    if (const int rc = check_plan("spmm_moment_bwd", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col_t && val_t), "spmm_moment_bwd: null col_t/val_t");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_moment_bwd: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (ldmu % 4 == 0) && (lda % 4 == 0) && (!C || ldc % 4 == 0) &&
                     (lddx % 4 == 0) && aligned16(X) && aligned16(Mu) && aligned16(A) && aligned16(C) && aligned16(dX) &&
                     (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1V_BWD_CASE(VW, LPR)                                                                                              \
    do {                                                                                                                         \
        if (C)                                                                                                                   \
            return launch_mom_bwd(MomBwdOp<VW, LPR, true>{col_t, val_t, X, ldx, Mu, ldmu, A, lda, C, ldc, dX, lddx, (float*)ws,  \
                                                          (int)H}, rowptr, hdr, plan_dev, st);                                   \
        return launch_mom_bwd(MomBwdOp<VW, LPR, false>{col_t, val_t, X, ldx, Mu, ldmu, A, lda, nullptr, 0, dX, lddx, (float*)ws, \
                                                       (int)H}, rowptr, hdr, plan_dev, st);                                      \
    } while (0)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1V_BWD_CASE);
#undef GLASS_K1V_BWD_CASE
}
