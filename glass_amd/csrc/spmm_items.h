// The skeleton of the neighbour aggregations that are not a product (K1m: spmm_max.hip, K1s: spmm_softmax.hip), written once:
// the walk over K1's plan items, the entry-batch loop, the lane-group and four-wave combines, the launches and the plan check.
// An aggregation supplies an operation `Op` — what a wave does with entries [e0, e1) of one row (`gather`, built on
// entry_batches), how two partial results combine (`Acc`) and where a finished row goes (`store`).  Every item runs in K1's row
// mode (correct for any item); K1's flat mode and non-temporal streams are not carried, and K1's own device code
// (spmm_common.h, spmm_sweep.h) is separate.
#pragma once
#include "common.h"
#include "spmm_common.h"
#include "spmm_sweep.h"

#include <stdint.h>
#include <type_traits>

namespace glass {

constexpr int64_t kMaxH = 65535ll * kWave;  // the grid's y extent times the columns of one scalar column tile
constexpr int kItemWaves = kBlock / kWave;

// ---- float[VW] / int32[VW] <-> one (vector) access ---------------------------------------------------------------------------
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
__device__ __forceinline__ void load_row(float (&x)[VW], const float* p) {
    Vec<VW> t;
    t.load(p);
    vec_to<VW>(t, x);
}
// a gathered row: zeros where the slot is masked
template <int VW>
__device__ __forceinline__ void load_row_if(bool ok, float (&x)[VW], const float* p) {
    Vec<VW> t;
    t.zero();
    if (ok) t.load(p);
    vec_to<VW>(t, x);
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

// ---- the accumulator of the backward passes: VW partial sums ---------------------------------------------------------------
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

template <int VW>
struct RowSlot {  // the slot (entry_batches) of an operation that gathers one row per entry
    float x[VW];
};

// ---- lane geometry of a wave, as K1's: a feature row is LPR lanes x VW floats, G = 64 / LPR lane groups -----------------------
struct ItemLanes {
    int lane, w;     // lane of the wave; wave of the workgroup (uniform)
    int grp, sub;    // lane group; lane within the group
    int coff;        // first column of this lane
    bool col_ok;     // coff < H
};
template <int VW, int LPR>
__device__ __forceinline__ ItemLanes item_lanes(int H) {
    ItemLanes ln;
    ln.lane = threadIdx.x & (kWave - 1);
    ln.w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    ln.grp = ln.lane / LPR;
    ln.sub = ln.lane % LPR;
    ln.coff = (blockIdx.y * LPR + ln.sub) * VW;
    ln.col_ok = ln.coff < H;
    return ln;
}

// ---- the entry-batch loop -------------------------------------------------------------------------------------------------
// Entries [e0, e1) of one row (wave-uniform), all 64 lanes together: one coalesced read of up to 64 (col, val) pairs, handed to
// the G lane groups with __shfl, U slots in flight per group.  Per slot u the operation is called twice:
//   load(slot, c, ok)        issue the gathers of column c into `slot` (zeros / neutral values where !ok)
//   take(slot, v, ok, e)     consume the slot: weight v, entry index e
// `ext` is an optional third per-entry stream (const int32_t*), read and shuffled beside col / val and handed on as
// load(slot, c, ok, x); an operation without one passes `nullptr`, and nothing of the stream is compiled.
template <int LPR, int U, class Slot, class Ext, class Load, class Take>
__device__ __forceinline__ void entry_batches(const int32_t* col, const float* val, Ext ext, int e0, int e1,
                                              const ItemLanes& ln, Load&& load, Take&& take) {
    constexpr bool EXT = !std::is_same<Ext, decltype(nullptr)>::value;
    constexpr int G = kWave / LPR;
    // (copies: read through `ln` inside the loops, the K1m forward's vector builds took 82 - 86 VGPRs instead of 61 - 76)
    const int lane = ln.lane, grp = ln.grp;
    const bool col_ok = ln.col_ok;
    for (int eb = e0; eb < e1; eb += kWave) {
        const int cnt = min(kWave, e1 - eb);
        int my_c = 0;
        [[maybe_unused]] int my_x = 0;
        float my_v = 0.f;
        if (lane < cnt) {
            my_c = col[eb + lane];
            my_v = val[eb + lane];
            if constexpr (EXT) my_x = ext[eb + lane];
        }
        for (int j = 0; j < cnt; j += U * G) {
            Slot s[U];
            float v[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = j + u * G + grp;  // < 64 + U*G: shfl wraps mod 64, masked by `ok`
                const int c = __shfl(my_c, idx);
                v[u] = __shfl(my_v, idx);
                ok[u] = col_ok && idx < cnt;
                if constexpr (EXT) load(s[u], c, ok[u], __shfl(my_x, idx));
                else load(s[u], c, ok[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) take(s[u], v[u], ok[u], eb + j + u * G + grp);
        }
    }
}

// ---- the item walk ----------------------------------------------------------------------------------------------------------
// Sweep item `wave` = (r0, r1, e0, e1): one wave, row by row — row(r, es, ee) for every row r with its entries [es, ee).
template <class Row>
__device__ __forceinline__ void sweep_item_rows(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ items, int wave,
                                                const ItemLanes& ln, Row&& row) {
    const int4 it = reinterpret_cast<const int4*>(items)[wave];
    const int r0 = __builtin_amdgcn_readfirstlane(it.x), r1 = __builtin_amdgcn_readfirstlane(it.y);
    const int e0 = __builtin_amdgcn_readfirstlane(it.z), e1 = __builtin_amdgcn_readfirstlane(it.w);
    const int nrows = r1 - r0;
    // start entry of row r0 + lane (lanes past the item hold e1)
    const int rp_reg = (ln.lane < nrows) ? rowptr[r0 + ln.lane] : e1;
    int es = e0;
    for (int i = 0; i < nrows; ++i) {
        const int ee = (i + 1 < nrows) ? __builtin_amdgcn_readlane(rp_reg, i + 1) : e1;
        row(r0 + i, es, ee);
        es = ee;
    }
}

// Long-row item (row, eb, ee, slot): one workgroup; wave w takes the w-th quarter [e0, e1) of the chunk, rounded to whole
// 64-entry batches.
struct LongItem {
    int row, slot, e0, e1;
};
__device__ __forceinline__ LongItem long_item_quarter(const int32_t* __restrict__ long_items, int index, int w) {
    const int32_t* it = long_items + 4 * (int64_t)index;
    const int eb = it[1], ee = it[2];
    const int per = ((ee - eb + kItemWaves * kWave - 1) / (kItemWaves * kWave)) * kWave;
    LongItem q;
    q.row = it[0];
    q.slot = it[3];
    q.e0 = min(eb + w * per, ee);
    q.e1 = min(q.e0 + per, ee);
    return q;
}

template <int LPR, class Acc>
__device__ __forceinline__ void fold_groups(Acc& acc) {
#pragma unroll
    for (int s = LPR; s < kWave; s <<= 1) acc.xor_merge(s);
}

// the four waves of a long-row item through LDS, in wave order; true on the lanes that then hold the item's result
template <int LPR, class Acc>
__device__ __forceinline__ bool combine_waves(Acc& acc, int32_t* lds, const ItemLanes& ln) {
    constexpr int kW = Acc::kLdsWords;
    if (ln.grp == 0) acc.to_lds(&lds[(ln.w * LPR + ln.sub) * kW]);
    __syncthreads();
    if (!(ln.w == 0 && ln.grp == 0 && ln.col_ok)) return false;
    acc.from_lds(&lds[ln.sub * kW]);
#pragma unroll
    for (int k = 1; k < kItemWaves; ++k) acc.merge_lds(&lds[(k * LPR + ln.sub) * kW]);
    return true;
}

// ---- one launch for the whole plan: sweep items (one wave each, row by row), then one workgroup per long-row item ---------
template <class Op>
__global__ __launch_bounds__(kBlock) void k1_items_kernel(const Op op, const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ items, int n_waves,
                                                          const int32_t* __restrict__ long_items, int n_sweep_blocks) {
    constexpr int LPR = Op::LPR, VW = Op::VW;
    __shared__ int32_t lds[kItemWaves * LPR * Op::Acc::kLdsWords];
    const ItemLanes ln = item_lanes<VW, LPR>(op.H);
    typename Op::Acc acc;
    if ((int)blockIdx.x >= n_sweep_blocks) {
        const LongItem q = long_item_quarter(long_items, (int)blockIdx.x - n_sweep_blocks, ln.w);
        acc.init();
        op.gather(acc, q.row, q.e0, q.e1, ln);
        fold_groups<LPR>(acc);
        if (combine_waves<LPR>(acc, lds, ln)) op.store(acc, q.row, q.slot, ln.coff);
        return;
    }
    const int wave = blockIdx.x * kItemWaves + ln.w;
    if (wave >= n_waves) return;
    sweep_item_rows(rowptr, items, wave, ln, [&](int row, int es, int ee) {
        acc.init();
        op.gather(acc, row, es, ee, ln);
        fold_groups<LPR>(acc);
        if (ln.grp == 0 && ln.col_ok) op.store(acc, row, -1, ln.coff);
    });
}

// ---- the same walk for a scalar: out[blockIdx.y][item] = the fp64 sum over the item's rows, lanes and columns of this tile -----
// op.gather(acc, row, e0, e1, ln) adds this lane's fp32 share of one row to acc; rows are added in fp64, then the lanes of the
// wave, then (long-row item) the four waves in wave order.  Sweep items come first in `out`, then the long-row items.
__device__ __forceinline__ double wave_sum(double a) {
#pragma unroll
    for (int s = 1; s < kWave; s <<= 1) a += __shfl_xor(a, s);
    return a;
}

template <class Op>
__global__ __launch_bounds__(kBlock) void k1_items_sum_kernel(const Op op, double* __restrict__ out,
                                                              const int32_t* __restrict__ rowptr,
                                                              const int32_t* __restrict__ items, int n_waves,
                                                              const int32_t* __restrict__ long_items, int n_sweep_blocks,
                                                              int n_items) {
    __shared__ double lds[kItemWaves];
    const ItemLanes ln = item_lanes<Op::VW, Op::LPR>(op.H);
    out += (int64_t)blockIdx.y * n_items;
    float acc = 0.f;
    if ((int)blockIdx.x >= n_sweep_blocks) {
        const int li = (int)blockIdx.x - n_sweep_blocks;
        const LongItem q = long_item_quarter(long_items, li, ln.w);
        op.gather(acc, q.row, q.e0, q.e1, ln);
        const double s = wave_sum((double)acc);
        if (ln.lane == 0) lds[ln.w] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot = lds[0];
#pragma unroll
            for (int k = 1; k < kItemWaves; ++k) tot += lds[k];
            out[n_waves + li] = tot;
        }
        return;
    }
    const int wave = blockIdx.x * kItemWaves + ln.w;
    if (wave >= n_waves) return;
    double tot = 0.0;
    sweep_item_rows(rowptr, items, wave, ln, [&](int row, int es, int ee) {
        acc = 0.f;
        op.gather(acc, row, es, ee, ln);
        tot += (double)acc;  // one row's fp32 share of this lane, rows added in fp64
    });
    tot = wave_sum(tot);
    if (ln.lane == 0) out[wave] = tot;
}

// ---- rows cut into several chunks, backward passes: their partial rows summed in slot order (K1's reduce step) ---------------
// (a template only for its linkage: this header is included by two translation units, and a plain __global__ here would be
// defined twice)
template <int = 0>
__global__ __launch_bounds__(kBlock) void k1_items_reduce_kernel(const float* __restrict__ partials, float* __restrict__ dX,
                                                                 int64_t ldx, int H, const int32_t* __restrict__ rrows) {
    spmm_reduce_body(partials, dX, ldx, H, rrows);
}

// ---- host ----------------------------------------------------------------------------------------------------------------
struct ItemsGrid {
    int n_ctiles, n_waves, n_sweep_blocks, n_items;
    unsigned blocks;  // sweep workgroups, then one per long-row item
};
template <class Op>
static ItemsGrid items_grid(const Op& op, const int32_t* hdr) {
    ItemsGrid g;
    g.n_ctiles = (int)ceil_div(op.H, (int64_t)Op::LPR * Op::VW);
    g.n_waves = hdr[H_NSWEEP];
    g.n_sweep_blocks = (int)ceil_div(g.n_waves, kItemWaves);
    g.n_items = g.n_waves + hdr[H_NLONG];
    g.blocks = (unsigned)(g.n_sweep_blocks + hdr[H_NLONG]);
    return g;
}

template <class Op>
static void launch_items(const Op& op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    const ItemsGrid g = items_grid(op, hdr);
    if (g.blocks == 0) return;
    hipLaunchKernelGGL((k1_items_kernel<Op>), dim3(g.blocks, g.n_ctiles), dim3(kBlock), 0, st, op, rowptr,
                       plan + hdr[H_OFF_SWEEP], g.n_waves, plan + hdr[H_OFF_LONG], g.n_sweep_blocks);
}

// the scalar form; returns the number of partials it leaves in `out` (n_items per column tile)
template <class Op>
static int64_t launch_items_sum(const Op& op, double* out, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan,
                                hipStream_t st) {
    const ItemsGrid g = items_grid(op, hdr);
    if (g.blocks > 0)
        hipLaunchKernelGGL((k1_items_sum_kernel<Op>), dim3(g.blocks, g.n_ctiles), dim3(kBlock), 0, st, op, out, rowptr,
                           plan + hdr[H_OFF_SWEEP], g.n_waves, plan + hdr[H_OFF_LONG], g.n_sweep_blocks, g.n_items);
    return (int64_t)g.n_items * g.n_ctiles;
}

static void launch_items_reduce(const float* partials, float* dX, int64_t ldx, int H, const int32_t* hdr, const int32_t* plan,
                                hipStream_t st) {
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(k1_items_reduce_kernel<>, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, partials, dX, ldx, H,
                           plan + hdr[H_OFF_REDUCE]);
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// what every entry asks of the plan header and the width; 0, or the code to return
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
