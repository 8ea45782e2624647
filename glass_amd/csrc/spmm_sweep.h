// K1's sweep kernel (one wave per plan item) and reduce step as device bodies, with the host's choice between the two
// sweep builds: shared by spmm.hip and the replicated form (spmm_rep.hip: Y[r] = A @ X[r], one grid plane per replica),
// so that a replica's bits are glass_spmm_csr_f32's bits on its slice by construction.  The bodies read blockIdx.x as the
// item block and blockIdx.y as the column block; the caller hands them the operands of one product.
#pragma once
#include "spmm_common.h"

#ifndef K1_STAMP  // (the laboratory build of spmm.hip defines it: per-wave wall-clock stamps)
#define K1_STAMP(slot) do { } while (0)
#endif

namespace glass {

// ---- sweep kernel: one wave per plan item (r0, r1, e0, e1): <= 64 consecutive short rows holding <= 256 edges ----
// The item carries its edge range, so the index loads (row pointers, col, val) depend on ONE scalar load of the plan
// and not on a chain plan -> rowptr -> col: plan -> {rowptr chunk, col/val} -> X rows -> store.
//
// Two modes, chosen per wave from the item alone (wave-uniform, a pure function of the plan and H, so results are
// bitwise repeatable):
//  * row mode (mean degree > rp_factor * G): one row at a time, its edges split over the G lane groups, partial sums
//    combined with __shfl_xor;
//  * flat mode (short rows): the item's col/val/rowptr are staged once in LDS with coalesced loads; each lane group
//    owns an edge-balanced run of whole rows and walks ITS edges as one flat stream, U gathers in flight whatever
//    the row lengths (a row boundary only flushes the accumulator), rows summed in plain edge order, no cross-group
//    reduction.  On a degree-1 pattern that is U*G independent 4H-byte gathers in flight per wave behind a single
//    index round trip (the previous form had 2 per group behind three dependent round trips: 0.55 of the HBM roofline).
constexpr int64_t kStreamNtBytes = 256ll << 20;  // Infinity Cache size
constexpr int kFlatMinItems = 8192;   // the flat-capable sweep kernel only on throughput-bound sweeps ...
constexpr int kFlatMinShare15 = 4;    // ... with >= 4/15 of the sweep cost in flat-eligible items
// Tunables (overridable only by the laboratory build, tools/Makefile `lab`): gathers in flight per lane group and the
// sweep item caps
#ifndef GLASS_K1_U
#define GLASS_K1_U 8
#endif
#ifndef GLASS_K1_ITEM_EDGES
#define GLASS_K1_ITEM_EDGES 256
#endif
constexpr int kGathers = GLASS_K1_U;
constexpr int kItemRows = 64;                    // rows per sweep item (one coalesced rowptr load per wave)
constexpr int kItemEdges = GLASS_K1_ITEM_EDGES;  // edges per sweep item (LDS staging: 2 KiB of (col,val) per wave at 256)

// FLAT = false: a specialisation without the flat branch, its LDS staging and its registers (64 instead of 76 VGPRs: 8
// instead of 6 waves per SIMD); every item then runs in row mode, which is correct for any item.  Chosen on the host
// (launch_spmm_u) unless flat mode pays: the sweep must be throughput-bound (>= 8 192 items; on small graphs the
// serial per-group walk of flat mode lengthens the critical path: density-shape 5.9 vs 4.8 us) AND a real share of the
// work must sit in flat-eligible items (header word H_FLAT_SHARE; ppi_bp-shape: a few low-degree rows out of 17 080
// qualify, and carrying the flat branch for them cost 13.4 vs 12.2 us per launch).
template <int VW, int LPR, int U, bool NT, bool FLAT>
__device__ __forceinline__ void spmm_sweep_body(const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ col,
                                                            const float* __restrict__ val,
                                                            const float* __restrict__ X, int64_t ldx,
                                                            float* __restrict__ Y, int64_t ldy, int H,
                                                            const int32_t* __restrict__ items, int n_waves,
                                                            int rp_factor, const int32_t* __restrict__ long_items,
                                                            int n_sweep_blocks, float* __restrict__ partials) {
    constexpr int G = kWave / LPR;
    constexpr int kWaves = kBlock / kWave;
    constexpr bool kFlat = FLAT && G > 1;
    __shared__ int32_t s_rp[kFlat ? kWaves : 1][kFlat ? kItemRows + 1 : 1];
    __shared__ int32_t s_col[kFlat ? kWaves : 1][kFlat ? kItemEdges : 1];
    __shared__ float s_val[kFlat ? kWaves : 1][kFlat ? kItemEdges : 1];
    __shared__ float s_long[kWaves * LPR * VW];
    if ((int)blockIdx.x >= n_sweep_blocks) {
        // The workgroups past the sweep's own run the plan's long-row items in the same launch: on graphs that have both
        // kinds of rows a second dependent launch for a handful of long rows cost more than the rows themselves (the
        // shipped density graph: 4 955 sweep waves + 4 long rows, 12.8 us as two launches).
        long_item_body<VW, LPR, U, NT>(col, val, X, ldx, Y, ldy, partials, H,
                                       long_items + 4 * (int64_t)((int)blockIdx.x - n_sweep_blocks), s_long);
        return;
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wave = blockIdx.x * kWaves + w;
    if (wave >= n_waves) return;
    const int grp = lane / LPR, sub = lane % LPR;
    const int coff = (blockIdx.y * LPR + sub) * VW;
    const bool col_ok = coff < H;
    const float* Xc = X + coff;
    K1_STAMP(0);  // wave start | item known | row pointers known | done
    const int4 it = reinterpret_cast<const int4*>(items)[wave];
    const int r0 = __builtin_amdgcn_readfirstlane(it.x), r1 = __builtin_amdgcn_readfirstlane(it.y);
    const int e0 = __builtin_amdgcn_readfirstlane(it.z), e1 = __builtin_amdgcn_readfirstlane(it.w);
    const int nrows = r1 - r0, ne = e1 - e0;
    K1_STAMP(1);
    // start edge of row r0 + lane (lanes past the item hold e1, so "end of row i" is always lane i + 1's value or e1)
    const int rp_reg = (lane < nrows) ? ld_stream<NT>(rowptr + r0 + lane) : e1;
    if (kFlat && ne <= rp_factor * G * nrows) {
        // ---- flat mode ----
        int32_t* rp_s = s_rp[kFlat ? w : 0];
        int32_t* col_s = s_col[kFlat ? w : 0];
        float* val_s = s_val[kFlat ? w : 0];
        int cr[kItemEdges / kWave];
        float vr[kItemEdges / kWave];
#pragma unroll
        for (int k = 0; k < kItemEdges / kWave; ++k) {
            const int idx = k * kWave + lane;
            cr[k] = 0;
            vr[k] = 0.f;
            if (idx < ne) {
                cr[k] = ld_stream<NT>(col + e0 + idx);
                vr[k] = ld_stream<NT>(val + e0 + idx);
            }
        }
        rp_s[lane] = rp_reg - e0;
        if (lane == 0) rp_s[kItemRows] = ne;
#pragma unroll
        for (int k = 0; k < kItemEdges / kWave; ++k) {
            col_s[k * kWave + lane] = cr[k];
            val_s[k * kWave + lane] = vr[k];
        }
        // this lane group's rows [rbeg, rend): edge-balanced cut points (row granularity) when G is small, equal row
        // counts otherwise
        int rbeg, rend;
        if (G <= 8) {
            rbeg = 0;
            rend = nrows;
#pragma unroll
            for (int g = 1; g < G; ++g) {
                const int tgt = e0 + (int)(((int64_t)ne * g) / G);
                const int cnt = __popcll(__ballot(lane < nrows && rp_reg < tgt));
                if (grp == g) rbeg = cnt;
                if (grp == g - 1) rend = cnt;
            }
        } else {
            const int per = (nrows + G - 1) / G;
            rbeg = min(grp * per, nrows);
            rend = min(rbeg + per, nrows);
        }
        // (the LDS image was written by this wave only; ds operations of one wave complete in order)
        int r = rbeg;
        int e = rbeg < nrows ? rp_s[rbeg] : ne;
        const int ge = rend < nrows ? rp_s[rend] : ne;
        int row_end = rp_s[r + 1];  // entries past the item's rows hold ne
        Vec<VW> acc;
        acc.zero();
        while (e < ge) {
            Vec<VW> x[U];
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool ok = e + u < ge;
                const int c = ok ? col_s[e + u] : 0;
                v[u] = ok ? val_s[e + u] : 0.f;
                x[u].zero();
                if (ok && col_ok) x[u].load(Xc + (int64_t)c * ldx);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (e + u < ge) {
                    while (e + u >= row_end) {  // row r is complete (possibly empty): flush
                        if (col_ok) acc.template store_out<NT>(Y + (int64_t)(r0 + r) * ldy + coff);
                        acc.zero();
                        ++r;
                        row_end = rp_s[r + 1];
                    }
                    acc.fma(v[u], x[u]);
                }
            }
            e += U;
        }
        for (; r < rend; ++r) {  // the row in progress, then trailing empty rows
            if (col_ok) acc.template store_out<NT>(Y + (int64_t)(r0 + r) * ldy + coff);
            acc.zero();
        }
        return;
    }
    // ---- row mode ----
#ifdef GLASS_K1_TRACE
    if (__builtin_amdgcn_readfirstlane(rp_reg) >= 0) K1_STAMP(2);
#endif
    int es = e0;
    for (int i = 0; i < nrows; ++i) {
        const int ee = (i + 1 < nrows) ? __builtin_amdgcn_readlane(rp_reg, i + 1) : e1;
        Vec<VW> acc;
        acc.zero();
        gather_edges<VW, LPR, U, NT>(acc, col, val, Xc, ldx, es, ee, lane, grp, col_ok);
        reduce_groups<VW, LPR>(acc);
        if (grp == 0 && col_ok) acc.template store_out<NT>(Y + (int64_t)(r0 + i) * ldy + coff);
        es = ee;
    }
    K1_STAMP(3);
}

// (row-only build at H >= 64: held to 64 VGPRs = 8 waves per SIMD; the long-row branch would otherwise cost a 65th)
#define GLASS_K1_SWEEP_BOUNDS __launch_bounds__(kBlock, (!FLAT && LPR >= 16) ? 8 : 1)

// ---- reduce step: rows cut into several chunks: sum their partial rows in slot order --------
__device__ __forceinline__ void spmm_reduce_body(const float* __restrict__ partials, float* __restrict__ Y, int64_t ldy, int H,
                                                 const int32_t* __restrict__ rrows) {
    const int32_t* rr = rrows + 3 * (int64_t)blockIdx.x;
    const int row = rr[0], first = rr[1], n = rr[2];
    for (int c = threadIdx.x; c < H; c += kBlock) {
        float s = 0.f;
        for (int k = 0; k < n; ++k) s += partials[(int64_t)(first + k) * H + c];
        Y[(int64_t)row * ldy + c] = s;
    }
}

// The host's choice of the sweep build for a plan at G lane groups per wave (see FLAT above): a pure function of the plan.
inline bool spmm_sweep_flat(const int32_t* hdr, int G) {
    int g_log2 = 0;
    while ((1 << g_log2) < G) ++g_log2;
    const int share15 = (hdr[H_FLAT_SHARE] >> (4 * g_log2)) & 15;  // fifteenths of the sweep cost in flat-eligible items
    return G > 1 && hdr[H_NSWEEP] >= kFlatMinItems && share15 >= kFlatMinShare15;
}

}  // namespace glass
