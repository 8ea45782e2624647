// K1m: max neighbour aggregation (aggr "max", an extension: the reference has none) on K1's CSR, plans and lane layout.
//
//   forward   Y[i,c] = max over entries e of row i of val[e] * X[col[e],c]     arg[i,c] = the winning e (int32), -1: empty row
//   backward  dX[j,c] = sum over entries t of row j of the TRANSPOSED CSR of (arg[i_t,c] == eid_t[t]) ? val_t[t] * dY[i_t,c] : 0
//
// Not a matrix product, so not expressible through K1 — but the same shape of work: per entry one gather of a 4H-byte row
// (forward) or of two (backward: the destination's arg row and its dY row), HBM / L2 bound.  Layout per wave64 as in K1
// (spmm_common.h): a feature row is LPR lanes x VW floats, G = 64 / LPR lane groups take G neighbour rows per wave
// instruction, U gathers in flight per group.  Each lane element carries a running (best, arg) pair; lane groups, the four
// waves of a long-row item and the chunks of a cut row are combined by the same total order — larger value first, on equal
// values (-0.0 == +0.0) the smaller e — which is what a scan over e upward with `>` gives, whatever the order of combination.
// The product is one fp32 multiply (__fmul_rn: never contracted), so Y is bit-for-bit a function of the inputs alone.
// The backward sums in a fixed order (lane-group partial sums, __shfl_xor, LDS, chunk partial rows in slot order): no float
// atomics, bitwise repeatable.  Rows are cut by K1's plan (glass_spmm_plan_build reads the row pointer only).  The plan holds
// no grid-wide ordering, so the chunks of a cut row are always combined by a second, small launch.
//
// This file holds what is K1m: the pair, the two operations' per-slot steps and their stores, the pair reduce and the entry
// points.  The item walk, the entry-batch loop, the combines and the launch are spmm_items.h's, shared with K1s — except
// that the forward keeps a copy of the entry-batch loop of its own (MaxFwdOp::gather says why: speed).
#include "spmm_items.h"

namespace glass {

constexpr int kMaxFwdGathers = kGathers;  // U of the forward: as K1
constexpr int kMaxBwdGathers = 4;         // U of the backward: two rows per entry in flight, so half of K1's

// ---- running (best, arg) pairs of one lane: VW elements ------------------------------------------------------------------
template <int VW>
struct MaxPair {
    float b[VW];
    int32_t a[VW];
    static constexpr int kLdsWords = 2 * VW;
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int k = 0; k < VW; ++k) { b[k] = 0.f; a[k] = -1; }  // an empty row: Y = 0, arg = -1
    }
    // entry e, scanned upward by this lane: `>` keeps the smaller e on equal values
    __device__ __forceinline__ void take(bool ok, float v, const float (&x)[VW], int e) {
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            const float p = __fmul_rn(v, x[k]);
            const bool t = ok && (a[k] < 0 || p > b[k]);
            b[k] = t ? p : b[k];
            a[k] = t ? e : a[k];
        }
    }
    __device__ __forceinline__ void merge1(int k, float ob, int32_t oa) {
        const bool t = oa >= 0 && (a[k] < 0 || ob > b[k] || (ob == b[k] && oa < a[k]));
        b[k] = t ? ob : b[k];
        a[k] = t ? oa : a[k];
    }
    __device__ __forceinline__ void xor_merge(int s) {
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            const float ob = __shfl_xor(b[k], s);
            const int32_t oa = __shfl_xor(a[k], s);
            merge1(k, ob, oa);
        }
    }
    __device__ __forceinline__ void to_lds(int32_t* p) const {
#pragma unroll
        for (int k = 0; k < VW; ++k) { p[k] = __float_as_int(b[k]); p[VW + k] = a[k]; }
    }
    __device__ __forceinline__ void from_lds(const int32_t* p) {
#pragma unroll
        for (int k = 0; k < VW; ++k) { b[k] = __int_as_float(p[k]); a[k] = p[VW + k]; }
    }
    __device__ __forceinline__ void merge_lds(const int32_t* p) {
#pragma unroll
        for (int k = 0; k < VW; ++k) merge1(k, __int_as_float(p[k]), p[VW + k]);
    }
};

// ---- the two operations: what a wave does with entries [e0, e1) of one row, and where a finished row goes ------------------
template <int VW_, int LPR_>
struct MaxFwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kMaxFwdGathers;
    using Acc = MaxPair<VW>;
    const int32_t* col;
    const float* val;
    const float* X;
    int64_t ldx;
    float* Y;
    int64_t ldy;
    int32_t* arg;
    int64_t ldarg;
    float* pbest;    // partial pairs of the chunks of cut rows: [n_slots, H] values, then [n_slots, H] entry indices
    int32_t* parg;
    int H;

    // entry_batches (spmm_items.h) written out, the one copy of that loop outside it: handed to the shared loop as two
    // callbacks, the pair's update compiles to another mix of selects and skip-branches (same 65 VGPRs at hidden 64) that
    // measured 0.7 us per launch slower (19.8 against 19.1 us at hidden 64, ppi_bp shape) — this form is the one that keeps
    // the speed.  A fix to the masked-shuffle loop there belongs here too.
    __device__ __forceinline__ void gather(Acc& acc, int /*row*/, int e0, int e1, const ItemLanes& ln) const {
        constexpr int G = kWave / LPR;
        const int lane = ln.lane, grp = ln.grp;
        const bool col_ok = ln.col_ok;
        const float* Xc = X + ln.coff;
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
                    load_row_if<VW>(ok[u], x[u], Xc + (int64_t)c * ldx);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) acc.take(ok[u], v[u], x[u], eb + j + u * G + grp);
            }
        }
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        const Vec<VW> t = vec_from<VW>(acc.b);
        if (slot < 0) {
            t.store(Y + (int64_t)row * ldy + coff);
            store_words<VW>(acc.a, arg + (int64_t)row * ldarg + coff);
        } else {
            t.store(pbest + (int64_t)slot * H + coff);
            store_words<VW>(acc.a, parg + (int64_t)slot * H + coff);
        }
    }
};

template <int VW_, int LPR_>
struct MaxBwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kMaxBwdGathers;
    using Acc = SumAcc<VW>;
    struct Slot {
        float g[VW];    // the destination's dY row
        int32_t a[VW];  // its arg row
        int32_t e;      // this entry's index in the forward CSR
    };
    const int32_t* col;   // the transposed CSR: destinations
    const float* val;
    const int32_t* eid;   // index of each transposed entry in the forward CSR
    const float* dY;
    int64_t ldy;
    const int32_t* arg;
    int64_t ldarg;
    float* dX;
    int64_t ldx;
    float* partials;      // [n_slots, H] partial rows of the chunks of cut rows
    int H;

    __device__ __forceinline__ void gather(Acc& acc, int /*row*/, int e0, int e1, const ItemLanes& ln) const {
        const float* dYc = dY + ln.coff;
        const int32_t* argc = arg + ln.coff;
        entry_batches<LPR, U, Slot>(
            col, val, eid, e0, e1, ln,
            [&](Slot& s, int c, bool ok, int32_t e) {
                load_row_if<VW>(ok, s.g, dYc + (int64_t)c * ldy);
#pragma unroll
                for (int k = 0; k < VW; ++k) s.a[k] = -1;
                if (ok) load_words<VW>(s.a, argc + (int64_t)c * ldarg);
                s.e = ok ? e : -2;  // matches no arg
            },
            [&](const Slot& s, float v, bool, int) {
#pragma unroll
                for (int k = 0; k < VW; ++k) acc.s[k] = fmaf(s.a[k] == s.e ? v : 0.f, s.g[k], acc.s[k]);
            });
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        const Vec<VW> t = vec_from<VW>(acc.s);
        t.store((slot < 0 ? dX + (int64_t)row * ldx : partials + (int64_t)slot * H) + coff);
    }
};

// ---- rows cut into several chunks: the max of their partial pairs, slot by slot ---------------------------------------------
__global__ __launch_bounds__(kBlock) void spmm_max_reduce_kernel(const float* __restrict__ pbest, const int32_t* __restrict__ parg,
                                                                 float* __restrict__ Y, int64_t ldy, int32_t* __restrict__ arg,
                                                                 int64_t ldarg, int H, const int32_t* __restrict__ rrows) {
    const int32_t* rr = rrows + 3 * (int64_t)blockIdx.x;
    const int row = rr[0], first = rr[1], n = rr[2];
    for (int c = threadIdx.x; c < H; c += kBlock) {
        MaxPair<1> p;
        p.init();
        for (int k = 0; k < n; ++k) p.merge1(0, pbest[(int64_t)(first + k) * H + c], parg[(int64_t)(first + k) * H + c]);
        Y[(int64_t)row * ldy + c] = p.b[0];
        arg[(int64_t)row * ldarg + c] = p.a[0];
    }
}

template <int VW, int LPR>
static int launch_max_fwd(MaxFwdOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    launch_items(op, rowptr, hdr, plan, st);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_max_reduce_kernel, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, op.pbest, op.parg, op.Y,
                           op.ldy, op.arg, op.ldarg, op.H, plan + hdr[H_OFF_REDUCE]);
    return launch_status("glass_spmm_max_csr_f32");
}

template <int VW, int LPR>
static int launch_max_bwd(MaxBwdOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    launch_items(op, rowptr, hdr, plan, st);
    launch_items_reduce(op.partials, op.dX, op.ldx, op.H, hdr, plan, st);
    return launch_status("glass_spmm_max_bwd_f32");
}

}  // namespace glass

using namespace glass;

extern "C" int64_t glass_spmm_max_ws_bytes(const int32_t* hdr, int64_t H) {
    if (!hdr || hdr[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr[H_NSLOTS] * H * (int64_t)(sizeof(float) + sizeof(int32_t));
}

extern "C" int64_t glass_spmm_max_bwd_ws_bytes(const int32_t* hdr_t, int64_t H) {
    if (!hdr_t || hdr_t[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr_t[H_NSLOTS] * H * (int64_t)sizeof(float);
}

extern "C" int glass_spmm_max_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                      float* Y, int64_t ldy, int32_t* arg, int64_t ldarg, int64_t n_rows, int64_t H,
                                      const int32_t* hdr, const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && Y && arg && hdr && plan_dev, "spmm_max: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col) && aligned4(val) && aligned4(X) && aligned4(Y) && aligned4(arg) &&
                  aligned4(plan_dev) && aligned4(ws), "spmm_max: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && ldy >= H && ldarg >= H,
                  "spmm_max: need H>0, ldx>=H, ldy>=H, ldarg>=H (H=%lld ldx=%lld ldy=%lld ldarg=%lld)", (long long)H,
                  (long long)ldx, (long long)ldy, (long long)ldarg);
    if (const int rc = check_plan("spmm_max", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val), "spmm_max: null col/val");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_max: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* pbest = (float*)ws;
    int32_t* parg = (int32_t*)ws + (int64_t)hdr[H_NSLOTS] * H;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && (ldarg % 4 == 0) && aligned16(X) && aligned16(Y) &&
                     aligned16(arg) && (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1M_FWD_CASE(VW, LPR)                                                                                      \
    return launch_max_fwd(MaxFwdOp<VW, LPR>{col, val, X, ldx, Y, ldy, arg, ldarg, pbest, parg, (int)H}, rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1M_FWD_CASE);
#undef GLASS_K1M_FWD_CASE
}

extern "C" int glass_spmm_max_bwd_f32(const int32_t* rowptr, const int32_t* col_t, const float* val_t, const int32_t* eid_t,
                                      const float* dY, int64_t ldy, const int32_t* arg, int64_t ldarg, float* dX, int64_t ldx,
                                      int64_t n_rows, int64_t H, const int32_t* hdr, const int32_t* plan_dev, void* ws,
                                      void* stream) {
    GLASS_REQUIRE(rowptr && dY && arg && dX && hdr && plan_dev, "spmm_max_bwd: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col_t) && aligned4(val_t) && aligned4(eid_t) && aligned4(dY) && aligned4(arg) &&
                  aligned4(dX) && aligned4(plan_dev) && aligned4(ws), "spmm_max_bwd: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && ldy >= H && ldarg >= H,
                  "spmm_max_bwd: need H>0, ldx>=H, ldy>=H, ldarg>=H (H=%lld ldx=%lld ldy=%lld ldarg=%lld)", (long long)H,
                  (long long)ldx, (long long)ldy, (long long)ldarg);
    if (const int rc = check_plan("spmm_max_bwd", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col_t && val_t && eid_t), "spmm_max_bwd: null col_t/val_t/eid_t");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_max_bwd: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && (ldarg % 4 == 0) && aligned16(dY) && aligned16(arg) &&
                     aligned16(dX) && (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1M_BWD_CASE(VW, LPR)                                                                                         \
    return launch_max_bwd(MaxBwdOp<VW, LPR>{col_t, val_t, eid_t, dY, ldy, arg, ldarg, dX, ldx, (float*)ws, (int)H}, rowptr, hdr, \
                          plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1M_BWD_CASE);
#undef GLASS_K1M_BWD_CASE
}
