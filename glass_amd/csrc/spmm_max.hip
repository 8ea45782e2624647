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
// Every item runs in K1's row mode (correct for any item); the flat mode and the non-temporal streams of K1 are not carried.
#include "common.h"
#include "spmm_common.h"
#include "spmm_sweep.h"

#include <stdint.h>

namespace glass {

constexpr int kMaxFwdGathers = kGathers;  // U of the forward: as K1
constexpr int kMaxBwdGathers = 4;         // U of the backward: two rows per entry in flight, so half of K1's

constexpr int64_t kMaxH = 65535ll * kWave;  // the grid's y extent times the columns of one scalar column tile

template <int VW>
__device__ __forceinline__ void vec_to(const Vec<VW>& t, float (&x)[VW]) {
    if constexpr (VW == 4) { x[0] = t.v.x; x[1] = t.v.y; x[2] = t.v.z; x[3] = t.v.w; }
    else x[0] = t.v;
}
template <int VW>
__device__ __forceinline__ Vec<VW> vec_from(const float (&x)[VW]) {
    Vec<VW> t;
    if constexpr (VW == 4) t.v = make_float4(x[0], x[1], x[2], x[3]);
    else t.v = x[0];
    return t;
}
template <int VW>
__device__ __forceinline__ void load_words(int32_t (&w)[VW], const int32_t* p) {
    if constexpr (VW == 4) {
        const int4 t = *reinterpret_cast<const int4*>(p);
        w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
    } else {
        w[0] = *p;
    }
}
template <int VW>
__device__ __forceinline__ void store_words(const int32_t (&w)[VW], int32_t* p) {
    if constexpr (VW == 4) *reinterpret_cast<int4*>(p) = make_int4(w[0], w[1], w[2], w[3]);
    else *p = w[0];
}

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

// ---- backward accumulator: VW partial sums -------------------------------------------------------------------------------
template <int VW>
struct SumAcc {
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
    __device__ __forceinline__ void to_lds(int32_t* p) const {
#pragma unroll
        for (int k = 0; k < VW; ++k) p[k] = __float_as_int(s[k]);
    }
    __device__ __forceinline__ void from_lds(const int32_t* p) {
#pragma unroll
        for (int k = 0; k < VW; ++k) s[k] = __int_as_float(p[k]);
    }
    __device__ __forceinline__ void merge_lds(const int32_t* p) {
#pragma unroll
        for (int k = 0; k < VW; ++k) s[k] += __int_as_float(p[k]);
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

    __device__ __forceinline__ void gather(Acc& acc, int e0, int e1, int lane, int grp, int coff, bool col_ok) const {
        constexpr int G = kWave / LPR;
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
                    Vec<VW> t;
                    t.zero();
                    if (ok[u]) t.load(Xc + (int64_t)c * ldx);
                    vec_to<VW>(t, x[u]);
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

    __device__ __forceinline__ void gather(Acc& acc, int e0, int e1, int lane, int grp, int coff, bool col_ok) const {
        constexpr int G = kWave / LPR;
        const float* dYc = dY + coff;
        const int32_t* argc = arg + coff;
        for (int eb = e0; eb < e1; eb += kWave) {
            const int cnt = min(kWave, e1 - eb);
            int my_c = 0, my_e = -2;
            float my_v = 0.f;
            if (lane < cnt) {
                my_c = col[eb + lane];
                my_v = val[eb + lane];
                my_e = eid[eb + lane];
            }
            for (int j = 0; j < cnt; j += U * G) {
                float g[U][VW], v[U];
                int32_t a[U][VW], e[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int idx = j + u * G + grp;  // < 64 + U*G: shfl wraps mod 64, masked by `ok`
                    const int c = __shfl(my_c, idx);
                    v[u] = __shfl(my_v, idx);
                    e[u] = __shfl(my_e, idx);
                    const bool ok = col_ok && idx < cnt;
                    Vec<VW> t;
                    t.zero();
#pragma unroll
                    for (int k = 0; k < VW; ++k) a[u][k] = -1;
                    if (ok) {
                        t.load(dYc + (int64_t)c * ldy);
                        load_words<VW>(a[u], argc + (int64_t)c * ldarg);
                    } else {
                        e[u] = -2;  // matches no arg
                    }
                    vec_to<VW>(t, g[u]);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int k = 0; k < VW; ++k) acc.s[k] = fmaf(a[u][k] == e[u] ? v[u] : 0.f, g[u][k], acc.s[k]);
            }
        }
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        const Vec<VW> t = vec_from<VW>(acc.s);
        t.store((slot < 0 ? dX + (int64_t)row * ldx : partials + (int64_t)slot * H) + coff);
    }
};

// ---- one launch for the whole plan: sweep items (one wave each, row by row), then one workgroup per long-row item ---------
template <class Op>
__global__ __launch_bounds__(kBlock) void spmm_max_items_kernel(const Op op, const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ items, int n_waves,
                                                                const int32_t* __restrict__ long_items, int n_sweep_blocks) {
    constexpr int LPR = Op::LPR, VW = Op::VW, kWaves = kBlock / kWave, kW = Op::Acc::kLdsWords;
    __shared__ int32_t lds[kWaves * LPR * kW];
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
        const int per = ((ee - eb + kWaves * kWave - 1) / (kWaves * kWave)) * kWave;
        const int e0 = min(eb + w * per, ee), e1 = min(e0 + per, ee);
        acc.init();
        op.gather(acc, e0, e1, lane, grp, coff, col_ok);
#pragma unroll
        for (int s = LPR; s < kWave; s <<= 1) acc.xor_merge(s);
        if (grp == 0) acc.to_lds(&lds[(w * LPR + sub) * kW]);
        __syncthreads();
        if (w == 0 && grp == 0 && col_ok) {
            acc.from_lds(&lds[sub * kW]);
#pragma unroll
            for (int k = 1; k < kWaves; ++k) acc.merge_lds(&lds[(k * LPR + sub) * kW]);
            op.store(acc, row, slot, coff);
        }
        return;
    }
    const int wave = blockIdx.x * kWaves + w;
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
        op.gather(acc, es, ee, lane, grp, coff, col_ok);
#pragma unroll
        for (int s = LPR; s < kWave; s <<= 1) acc.xor_merge(s);
        if (grp == 0 && col_ok) op.store(acc, r0 + i, -1, coff);
        es = ee;
    }
}

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

__global__ __launch_bounds__(kBlock) void spmm_max_bwd_reduce_kernel(const float* __restrict__ partials, float* __restrict__ dX,
                                                                     int64_t ldx, int H, const int32_t* __restrict__ rrows) {
    spmm_reduce_body(partials, dX, ldx, H, rrows);
}

template <class Op>
static void launch_items(const Op& op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    const int n_ctiles = (int)ceil_div(op.H, (int64_t)Op::LPR * Op::VW);
    const int n_waves = hdr[H_NSWEEP];
    const int n_sweep_blocks = (int)ceil_div(n_waves, kBlock / kWave);
    const unsigned blocks = (unsigned)(n_sweep_blocks + hdr[H_NLONG]);  // sweep workgroups, then one per long-row item
    if (blocks == 0) return;
    hipLaunchKernelGGL((spmm_max_items_kernel<Op>), dim3(blocks, n_ctiles), dim3(kBlock), 0, st, op, rowptr,
                       plan + hdr[H_OFF_SWEEP], n_waves, plan + hdr[H_OFF_LONG], n_sweep_blocks);
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
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_max_bwd_reduce_kernel, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, op.partials, op.dX,
                           op.ldx, op.H, plan + hdr[H_OFF_REDUCE]);
    return launch_status("glass_spmm_max_bwd_f32");
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

// what both entries ask of the plan header and the width; 0, or the code to return
static int check_plan(const char* what, const int32_t* hdr, int64_t n_rows, int64_t H) {
    if (hdr[H_MAGIC] != kPlanMagic || hdr[H_VER] != kPlanVersion || hdr[H_NROWS] != n_rows) {
        set_error("%s: plan does not match (magic %x, rows %d vs %lld)", what, hdr[H_MAGIC], hdr[H_NROWS], (long long)n_rows);
        return GLASS_E_PLAN;
    }
    if (H > kMaxH) {
        set_error("%s: H = %lld is beyond the %lld columns one launch covers", what, (long long)H, (long long)kMaxH);
        return GLASS_E_UNSUPPORTED;
    }
    return 0;
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

#define GLASS_K1M_DISPATCH(OP, LAUNCH, ...)                                       \
    if (vec) {                                                                    \
        switch (pow2_ceil_cap(H / 4, 64)) {                                       \
            case 1: return LAUNCH(OP<4, 1>{__VA_ARGS__}, rowptr, hdr, plan_dev, st);   \
            case 2: return LAUNCH(OP<4, 2>{__VA_ARGS__}, rowptr, hdr, plan_dev, st);   \
            case 4: return LAUNCH(OP<4, 4>{__VA_ARGS__}, rowptr, hdr, plan_dev, st);   \
            case 8: return LAUNCH(OP<4, 8>{__VA_ARGS__}, rowptr, hdr, plan_dev, st);   \
            case 16: return LAUNCH(OP<4, 16>{__VA_ARGS__}, rowptr, hdr, plan_dev, st); \
            case 32: return LAUNCH(OP<4, 32>{__VA_ARGS__}, rowptr, hdr, plan_dev, st); \
            default: return LAUNCH(OP<4, 64>{__VA_ARGS__}, rowptr, hdr, plan_dev, st); \
        }                                                                         \
    }                                                                             \
    switch (pow2_ceil_cap(H, 64)) {                                               \
        case 1: return LAUNCH(OP<1, 1>{__VA_ARGS__}, rowptr, hdr, plan_dev, st);       \
        case 2: return LAUNCH(OP<1, 2>{__VA_ARGS__}, rowptr, hdr, plan_dev, st);       \
        case 4: return LAUNCH(OP<1, 4>{__VA_ARGS__}, rowptr, hdr, plan_dev, st);       \
        case 8: return LAUNCH(OP<1, 8>{__VA_ARGS__}, rowptr, hdr, plan_dev, st);       \
        case 16: return LAUNCH(OP<1, 16>{__VA_ARGS__}, rowptr, hdr, plan_dev, st);     \
        case 32: return LAUNCH(OP<1, 32>{__VA_ARGS__}, rowptr, hdr, plan_dev, st);     \
        default: return LAUNCH(OP<1, 64>{__VA_ARGS__}, rowptr, hdr, plan_dev, st);     \
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
    GLASS_K1M_DISPATCH(MaxFwdOp, launch_max_fwd, col, val, X, ldx, Y, ldy, arg, ldarg, pbest, parg, (int)H)
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
    GLASS_K1M_DISPATCH(MaxBwdOp, launch_max_bwd, col_t, val_t, eid_t, dY, ldy, arg, ldarg, dX, ldx, (float*)ws, (int)H)
}
