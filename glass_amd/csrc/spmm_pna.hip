// K1p: PNA neighbour aggregation (aggr "pna", an extension: the reference has none; Principal Neighbourhood Aggregation) on
// K1's CSR, plans and lane layout — mean, max, min and standard deviation of the neighbour messages from ONE gather of every
// source row.  Per destination i and channel c, over the entries e of row i (weight w_e > 0, a multiplicity; message
// x_e = X[col[e], c]):
//
//   W = sum_e w_e      Mu = sum_e w_e x_e / W      Var = sum_e w_e (x_e - Mu)^2 / W      S = sqrt(Var + eps)
//   Mx = max_e x_e     amx = the winning e         Mn = min_e x_e                        amn = the winning e
//   (a row without entries: W = Mu = S = Mx = Mn = 0, amx = amn = -1)
//
//   backward, on the TRANSPOSED CSR (row j = source, entries t = destinations i, val_t, eid_t[t] = the forward entry), with
//   the per-destination rows A = dS / (W S), C = dMu / W, Gmx = dMx, Gmn = dMn from the caller (0 where W = 0):
//   dX[j,c] = sum_t [ val_t (C[i,c] + A[i,c] (X[j,c] - Mu[i,c])) + (amx[i,c] == eid_t ? Gmx[i,c] : 0)
//                                                                  + (amn[i,c] == eid_t ? Gmn[i,c] : 0) ]
//
// The extremes are over the raw message: a multiplicity does not move them, there is no product and no rounding, so Mx, Mn,
// amx and amn are bit-for-bit functions of the inputs.  Ties go to the smaller e under K1m's total order (-0.0 == +0.0, the
// stored value is the winner's own bits).  The triple (W, mean, M2) merges with K1v's form of Chan's update
//
//   d = m_b - m_a    W = W_a + W_b    f = W_b / W    m = m_a + d f    M2 = M2_a + M2_b + d^2 (W_a f)      (empty side: identity)
//
// and no x^2 is ever formed.  Forward state per lane: W once for the lane's VW channels, then mean, M2, the max pair and the
// min pair per channel — 6 VW + 1 words.  Entries, lane groups (__shfl_xor), the four waves of a long-row item (LDS, wave
// order) and the chunks of a cut row (workspace, a second small launch, slot order) all merge in a fixed order: bitwise
// repeatable for a given plan.  The backward forms X - Mu per entry (never factored out: K1v says why) and sums as K1s's
// does.  No float atomics anywhere.
//
// The item walk, the entry-batch loop, the combines and the launches are spmm_items.h's (its fourth consumer); the triple's
// and the pairs' steps are restated here so that no other kernel's code changes.
#include "spmm_items.h"

namespace glass {

constexpr int kPnaFwdGathers = 4;  // U of the forward: 6 VW + 1 words of state beside the slots, so half of K1's
constexpr int kPnaBwdGathers = 2;  // U of the backward: seven rows per entry

// ---- Chan's update of one (W, mean, M2) by another; W and f are shared by the channels of a lane (K1v's arithmetic) --------
struct PnaStep {
    float W, f, g;  // the merged weight, W_b / W and W_a * f
    __device__ __forceinline__ PnaStep(float wa, float wb) {
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

// the total order of the extremes (K1m's): the better value first, on equal values the smaller entry; a < 0 is no entry
__device__ __forceinline__ void pna_merge_max(float& b, int32_t& a, float ob, int32_t oa) {
    const bool t = oa >= 0 && (a < 0 || ob > b || (ob == b && oa < a));
    b = t ? ob : b;
    a = t ? oa : a;
}
__device__ __forceinline__ void pna_merge_min(float& b, int32_t& a, float ob, int32_t oa) {
    const bool t = oa >= 0 && (a < 0 || ob < b || (ob == b && oa < a));
    b = t ? ob : b;
    a = t ? oa : a;
}

template <int VW>
struct PnaAcc {
    float W;
    float m[VW], q[VW];
    float xb[VW], nb[VW];    // the largest and the smallest message
    int32_t xa[VW], na[VW];  // their entries
    static constexpr int kLdsWords = 6 * VW + 1;
    __device__ __forceinline__ void init() {
        W = 0.f;
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            m[k] = q[k] = xb[k] = nb[k] = 0.f;  // an empty row: zeros, arg = -1
            xa[k] = na[k] = -1;
        }
    }
    // entry e, scanned upward by this lane: the triple (v, x, 0); `>` and `<` keep the smaller e on equal values
    __device__ __forceinline__ void take(bool ok, float v, const float (&x)[VW], int e) {
        const PnaStep s(W, v);
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            float mn = m[k], qn = q[k];
            s.apply(mn, qn, x[k], 0.f);
            m[k] = ok ? mn : m[k];
            q[k] = ok ? qn : q[k];
            const bool first = xa[k] < 0;  // (both pairs are empty together)
            const bool tx = ok && (first || x[k] > xb[k]);
            const bool tn = ok && (first || x[k] < nb[k]);
            xb[k] = tx ? x[k] : xb[k];
            xa[k] = tx ? e : xa[k];
            nb[k] = tn ? x[k] : nb[k];
            na[k] = tn ? e : na[k];
        }
        W = ok ? s.W : W;
    }
    __device__ __forceinline__ void xor_merge(int sh) {
        const PnaStep s(W, __shfl_xor(W, sh));
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            const float om = __shfl_xor(m[k], sh), oq = __shfl_xor(q[k], sh);
            s.apply(m[k], q[k], om, oq);
            const float oxb = __shfl_xor(xb[k], sh), onb = __shfl_xor(nb[k], sh);
            const int32_t oxa = __shfl_xor(xa[k], sh), ona = __shfl_xor(na[k], sh);
            pna_merge_max(xb[k], xa[k], oxb, oxa);
            pna_merge_min(nb[k], na[k], onb, ona);
        }
        W = s.W;
    }
    // LDS layout of one lane: W, then VW words each of mean, M2, max, min, arg max, arg min
    __device__ __forceinline__ void to_lds(int32_t* p) const {
        p[0] = __float_as_int(W);
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            p[1 + k] = __float_as_int(m[k]);
            p[1 + VW + k] = __float_as_int(q[k]);
            p[1 + 2 * VW + k] = __float_as_int(xb[k]);
            p[1 + 3 * VW + k] = __float_as_int(nb[k]);
            p[1 + 4 * VW + k] = xa[k];
            p[1 + 5 * VW + k] = na[k];
        }
    }
    __device__ __forceinline__ void from_lds(const int32_t* p) {
        W = __int_as_float(p[0]);
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            m[k] = __int_as_float(p[1 + k]);
            q[k] = __int_as_float(p[1 + VW + k]);
            xb[k] = __int_as_float(p[1 + 2 * VW + k]);
            nb[k] = __int_as_float(p[1 + 3 * VW + k]);
            xa[k] = p[1 + 4 * VW + k];
            na[k] = p[1 + 5 * VW + k];
        }
    }
    __device__ __forceinline__ void merge_lds(const int32_t* p) {
        const PnaStep s(W, __int_as_float(p[0]));
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            s.apply(m[k], q[k], __int_as_float(p[1 + k]), __int_as_float(p[1 + VW + k]));
            pna_merge_max(xb[k], xa[k], __int_as_float(p[1 + 2 * VW + k]), p[1 + 4 * VW + k]);
            pna_merge_min(nb[k], na[k], __int_as_float(p[1 + 3 * VW + k]), p[1 + 5 * VW + k]);
        }
        W = s.W;
    }
};

// (Mu, S) of a finished triple
__device__ __forceinline__ void pna_finish(float W, float m, float q, float eps, float& mu, float& s) {
    const bool any = W > 0.f;
    mu = any ? m : 0.f;
    s = any ? sqrtf(q / W + eps) : 0.f;
}

// where the results go, and the partial states of the chunks of cut rows: six [n_slots, H] arrays, then [n_slots] W
struct PnaOut {
    float* Mu;
    int64_t ldmu;
    float* S;
    int64_t lds_;
    float* Mx;
    int64_t ldmx;
    float* Mn;
    int64_t ldmn;
    int32_t* amx;
    int64_t ldamx;
    int32_t* amn;
    int64_t ldamn;
    float* Wsum;
    float* pm;
    float* pq;
    float* pxb;
    float* pnb;
    int32_t* pxa;
    int32_t* pna;
    float* pw;
};

// ---- forward: what a wave does with entries [e0, e1) of one row, and where a finished row goes ------------------------------
template <int VW_, int LPR_>
struct PnaFwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kPnaFwdGathers;
    using Acc = PnaAcc<VW>;
    using Slot = RowSlot<VW>;
    const int32_t* col;
    const float* val;
    const float* X;
    int64_t ldx;
    float eps;
    PnaOut o;
    int H;

    __device__ __forceinline__ void gather(Acc& acc, int /*row*/, int e0, int e1, const ItemLanes& ln) const {
        const float* Xc = X + ln.coff;
        entry_batches<LPR, U, Slot>(
            col, val, nullptr, e0, e1, ln,
            [&](Slot& s, int c, bool ok) { load_row_if<VW>(ok, s.x, Xc + (int64_t)c * ldx); },
            [&](const Slot& s, float v, bool ok, int e) { acc.take(ok, v, s.x, e); });
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        if (slot < 0) {
            float mu[VW], s[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) pna_finish(acc.W, acc.m[k], acc.q[k], eps, mu[k], s[k]);
            vec_from<VW>(mu).store(o.Mu + (int64_t)row * o.ldmu + coff);
            vec_from<VW>(s).store(o.S + (int64_t)row * o.lds_ + coff);
            vec_from<VW>(acc.xb).store(o.Mx + (int64_t)row * o.ldmx + coff);
            vec_from<VW>(acc.nb).store(o.Mn + (int64_t)row * o.ldmn + coff);
            store_words<VW>(acc.xa, o.amx + (int64_t)row * o.ldamx + coff);
            store_words<VW>(acc.na, o.amn + (int64_t)row * o.ldamn + coff);
            if (coff == 0) o.Wsum[row] = acc.W;
        } else {
            const int64_t p = (int64_t)slot * H + coff;
            vec_from<VW>(acc.m).store(o.pm + p);
            vec_from<VW>(acc.q).store(o.pq + p);
            vec_from<VW>(acc.xb).store(o.pxb + p);
            vec_from<VW>(acc.nb).store(o.pnb + p);
            store_words<VW>(acc.xa, o.pxa + p);
            store_words<VW>(acc.na, o.pna + p);
            if (coff == 0) o.pw[slot] = acc.W;
        }
    }
};

// ---- backward: row j of the transposed CSR; its own X row once, seven destination rows per entry ---------------------------
template <int VW_, int LPR_>
struct PnaBwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kPnaBwdGathers;
    using Acc = SumAcc<VW>;
    struct Slot {
        float a[VW], mu[VW], c[VW];  // the destination's A, Mu and C rows
        float gx[VW], gn[VW];        // the gradients of its max and min
        int32_t ax[VW], an[VW];      // their winning entries
        int32_t e;                   // this entry's index in the forward CSR
    };
    const int32_t* col;   // the transposed CSR: destinations
    const float* val;
    const int32_t* eid;   // index of each transposed entry in the forward CSR
    const float* X;
    int64_t ldx;
    const float* Mu;
    int64_t ldmu;
    const float* A;
    int64_t lda;
    const float* C;
    int64_t ldc;
    const int32_t* amx;
    int64_t ldamx;
    const float* Gmx;
    int64_t ldgmx;
    const int32_t* amn;
    int64_t ldamn;
    const float* Gmn;
    int64_t ldgmn;
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
        const float* Cc = C + ln.coff;
        const float* Gxc = Gmx + ln.coff;
        const float* Gnc = Gmn + ln.coff;
        const int32_t* axc = amx + ln.coff;
        const int32_t* anc = amn + ln.coff;
        entry_batches<LPR, U, Slot>(
            col, val, eid, e0, e1, ln,
            [&](Slot& s, int c, bool ok, int32_t e) {
                load_row_if<VW>(ok, s.a, Ac + (int64_t)c * lda);
                load_row_if<VW>(ok, s.mu, Mc + (int64_t)c * ldmu);
                load_row_if<VW>(ok, s.c, Cc + (int64_t)c * ldc);
                load_row_if<VW>(ok, s.gx, Gxc + (int64_t)c * ldgmx);
                load_row_if<VW>(ok, s.gn, Gnc + (int64_t)c * ldgmn);
#pragma unroll
                for (int k = 0; k < VW; ++k) s.ax[k] = s.an[k] = -1;
                if (ok) {
                    load_words<VW>(s.ax, axc + (int64_t)c * ldamx);
                    load_words<VW>(s.an, anc + (int64_t)c * ldamn);
                }
                s.e = ok ? e : -2;  // matches no arg
            },
            [&](const Slot& s, float v, bool ok, int) {
#pragma unroll
                for (int k = 0; k < VW; ++k) {
                    const float d = xj[k] - s.mu[k];  // per entry: never factored out of the sum
                    float term = v * fmaf(s.a[k], d, s.c[k]);
                    term += s.ax[k] == s.e ? s.gx[k] : 0.f;
                    term += s.an[k] == s.e ? s.gn[k] : 0.f;
                    acc.s[k] += ok ? term : 0.f;
                }
            });
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        const Vec<VW> r = vec_from<VW>(acc.s);
        r.store((slot < 0 ? dX + (int64_t)row * lddx : partials + (int64_t)slot * H) + coff);
    }
};

// ---- rows cut into several chunks: their partial states merged slot by slot ------------------------------------------------
__global__ __launch_bounds__(kBlock) void spmm_pna_reduce_kernel(const PnaOut o, float eps, int H,
                                                                 const int32_t* __restrict__ rrows) {
    const int32_t* rr = rrows + 3 * (int64_t)blockIdx.x;
    const int row = rr[0], first = rr[1], n = rr[2];
    for (int c = threadIdx.x; c < H; c += kBlock) {
        float W = 0.f, m = 0.f, q = 0.f, xb = 0.f, nb = 0.f;
        int32_t xa = -1, na = -1;
        for (int k = 0; k < n; ++k) {
            const int64_t p = (int64_t)(first + k) * H + c;
            const PnaStep s(W, o.pw[first + k]);
            s.apply(m, q, o.pm[p], o.pq[p]);
            W = s.W;
            pna_merge_max(xb, xa, o.pxb[p], o.pxa[p]);
            pna_merge_min(nb, na, o.pnb[p], o.pna[p]);
        }
        float mu, sv;
        pna_finish(W, m, q, eps, mu, sv);
        o.Mu[(int64_t)row * o.ldmu + c] = mu;
        o.S[(int64_t)row * o.lds_ + c] = sv;
        o.Mx[(int64_t)row * o.ldmx + c] = xb;
        o.Mn[(int64_t)row * o.ldmn + c] = nb;
        o.amx[(int64_t)row * o.ldamx + c] = xa;
        o.amn[(int64_t)row * o.ldamn + c] = na;
        if (c == 0) o.Wsum[row] = W;
    }
}

template <int VW, int LPR>
static int launch_pna_fwd(PnaFwdOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    static_assert(kItemWaves * LPR * PnaAcc<VW>::kLdsWords * 4 <= 32 * 1024, "the wave combine's LDS");
    launch_items(op, rowptr, hdr, plan, st);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_pna_reduce_kernel, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, op.o, op.eps, op.H,
                           plan + hdr[H_OFF_REDUCE]);
    return launch_status("glass_spmm_pna_csr_f32");
}

template <int VW, int LPR>
static int launch_pna_bwd(PnaBwdOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    launch_items(op, rowptr, hdr, plan, st);
    launch_items_reduce(op.partials, op.dX, op.lddx, op.H, hdr, plan, st);
    return launch_status("glass_spmm_pna_bwd_f32");
}

}  // namespace glass

using namespace glass;

// per partial slot: H each of mean, M2, max, min, arg max, arg min, and one W
extern "C" int64_t glass_spmm_pna_ws_bytes(const int32_t* hdr, int64_t H) {
    if (!hdr || hdr[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr[H_NSLOTS] * (6 * H + 1) * (int64_t)sizeof(float);
}

extern "C" int64_t glass_spmm_pna_bwd_ws_bytes(const int32_t* hdr_t, int64_t H) {
    if (!hdr_t || hdr_t[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr_t[H_NSLOTS] * H * (int64_t)sizeof(float);
}

extern "C" int glass_spmm_pna_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                      float eps, float* Mu, int64_t ldmu, float* S, int64_t lds, float* Mx, int64_t ldmx,
                                      float* Mn, int64_t ldmn, int32_t* amx, int64_t ldamx, int32_t* amn, int64_t ldamn,
                                      float* Wsum, int64_t n_rows, int64_t H, const int32_t* hdr, const int32_t* plan_dev,
                                      void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && Mu && S && Mx && Mn && amx && amn && Wsum && hdr && plan_dev, "spmm_pna: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col) && aligned4(val) && aligned4(X) && aligned4(Mu) && aligned4(S) &&
                  aligned4(Mx) && aligned4(Mn) && aligned4(amx) && aligned4(amn) && aligned4(Wsum) && aligned4(plan_dev) &&
                  aligned4(ws), "spmm_pna: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && ldmu >= H && lds >= H && ldmx >= H && ldmn >= H && ldamx >= H && ldamn >= H,
                  "spmm_pna: need H>0 and every ld >= H (H=%lld ldx=%lld ldmu=%lld lds=%lld ldmx=%lld ldmn=%lld ldamx=%lld "
                  "ldamn=%lld)", (long long)H, (long long)ldx, (long long)ldmu, (long long)lds, (long long)ldmx,
                  (long long)ldmn, (long long)ldamx, (long long)ldamn);
    GLASS_REQUIRE(eps >= 0.f, "spmm_pna: eps must be >= 0");
    if (const int rc = check_plan("spmm_pna", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val), "spmm_pna: null col/val");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_pna: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t sec = (int64_t)hdr[H_NSLOTS] * H;
    float* pf = (float*)ws;
    int32_t* pi = (int32_t*)ws;
    const PnaOut o{Mu, ldmu, S, lds, Mx, ldmx, Mn, ldmn, amx, ldamx, amn, ldamn, Wsum,
                   pf, pf + sec, pf + 2 * sec, pf + 3 * sec, pi + 4 * sec, pi + 5 * sec, pf + 6 * sec};
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (ldmu % 4 == 0) && (lds % 4 == 0) && (ldmx % 4 == 0) && (ldmn % 4 == 0) &&
                     (ldamx % 4 == 0) && (ldamn % 4 == 0) && aligned16(X) && aligned16(Mu) && aligned16(S) && aligned16(Mx) &&
                     aligned16(Mn) && aligned16(amx) && aligned16(amn) && (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1P_FWD_CASE(VW, LPR) \
    return launch_pna_fwd(PnaFwdOp<VW, LPR>{col, val, X, ldx, eps, o, (int)H}, rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1P_FWD_CASE);
#undef GLASS_K1P_FWD_CASE
}

extern "C" int glass_spmm_pna_bwd_f32(const int32_t* rowptr, const int32_t* col_t, const float* val_t, const int32_t* eid_t,
                                      const float* X, int64_t ldx, const float* Mu, int64_t ldmu, const float* A, int64_t lda,
                                      const float* C, int64_t ldc, const int32_t* amx, int64_t ldamx, const float* Gmx,
                                      int64_t ldgmx, const int32_t* amn, int64_t ldamn, const float* Gmn, int64_t ldgmn,
                                      float* dX, int64_t lddx, int64_t n_rows, int64_t H, const int32_t* hdr,
                                      const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && Mu && A && C && amx && Gmx && amn && Gmn && dX && hdr && plan_dev, "spmm_pna_bwd: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col_t) && aligned4(val_t) && aligned4(eid_t) && aligned4(X) && aligned4(Mu) &&
                  aligned4(A) && aligned4(C) && aligned4(amx) && aligned4(Gmx) && aligned4(amn) && aligned4(Gmn) && aligned4(dX) &&
                  aligned4(plan_dev) && aligned4(ws), "spmm_pna_bwd: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && ldmu >= H && lda >= H && ldc >= H && ldamx >= H && ldgmx >= H && ldamn >= H &&
                  ldgmn >= H && lddx >= H,
                  "spmm_pna_bwd: need H>0 and every ld >= H (H=%lld ldx=%lld ldmu=%lld lda=%lld ldc=%lld ldamx=%lld ldgmx=%lld "
                  "ldamn=%lld ldgmn=%lld lddx=%lld)", (long long)H, (long long)ldx, (long long)ldmu, (long long)lda,
                  (long long)ldc, (long long)ldamx, (long long)ldgmx, (long long)ldamn, (long long)ldgmn, (long long)lddx);
    if (const int rc = check_plan("spmm_pna_bwd", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col_t && val_t && eid_t), "spmm_pna_bwd: null col_t/val_t/eid_t");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_pna_bwd: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (ldmu % 4 == 0) && (lda % 4 == 0) && (ldc % 4 == 0) && (ldamx % 4 == 0) &&
                     (ldgmx % 4 == 0) && (ldamn % 4 == 0) && (ldgmn % 4 == 0) && (lddx % 4 == 0) && aligned16(X) &&
                     aligned16(Mu) && aligned16(A) && aligned16(C) && aligned16(amx) && aligned16(Gmx) && aligned16(amn) &&
                     aligned16(Gmn) && aligned16(dX) && (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1P_BWD_CASE(VW, LPR)                                                                                            \
    return launch_pna_bwd(PnaBwdOp<VW, LPR>{col_t, val_t, eid_t, X, ldx, Mu, ldmu, A, lda, C, ldc, amx, ldamx, Gmx, ldgmx, amn, \
                                            ldamn, Gmn, ldgmn, dX, lddx, (float*)ws, (int)H}, rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1P_BWD_CASE);
#undef GLASS_K1P_BWD_CASE
}
