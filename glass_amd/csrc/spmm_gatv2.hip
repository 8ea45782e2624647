// K1a2: dynamic attention neighbour aggregation (aggr "gatv2", an extension: the reference has none; single-head GATv2, Brody
// et al. 2022) on K1's CSR, plans and lane layout.  X [N, H] the messages, att one [H] vector, slope LeakyReLU's negative
// slope.  Per destination i, over the entries e of row i (source j = col[e], weight v_e > 0, a multiplicity):
//
//   u_ec = X[i,c] + X[j,c]              r_ec = u_ec > 0 ? u_ec : slope * u_ec   (one rounded add, one rounded multiply: fp32)
//   s_e = sum_c att[c] r_ec             (the products and the sum in fp64, rounded once to fp32; stored per entry: s [nnz])
//   M = max_e s_e     Z = sum_e v_e exp(s_e - M)     Y[i,:] = sum_e v_e exp(s_e - M) X[j,:] / Z     L_i = M + log Z
//   a row without entries: Y = 0, L = 0
//
//   backward, p_e = v_e exp(s_e - L_i), f_ec = u_ec > 0 ? 1 : slope (torch's leaky_relu rule: u == 0 takes slope):
//   D_i = sum_c dY[i,c] Y[i,c]          q_e = sum_c dY[i,c] X[j,c]          g_e = p_e (q_e - D_i)
//   Gd[i,c] = sum over the entries of row i of g_e att[c] f_ec              R[i,c] = sum over the entries of row i of g_e r_ec
//   dX[j,c] = sum over the entries with col = j of ( p_e dY[i,c] + g_e att[c] f_ec )  +  Gd[j,c]
//   d att[c] = sum_i R[i,c]
//
// The score is an H-wide reduction over the source row and the destination row, so it is formed where the rows are gathered:
// the score pass (GatV2ScoreOp) is a sampled dense-dense product with the non-linearity inside and leaves s [nnz] in forward
// entry order; every later pass READS s (or p and g, [nnz] too), so an entry's score has the same bits wherever it is used.
// The forward (GatV2FwdOp) is K1a's item walk and (M, Z) accumulator with s[e] streamed beside col / val.  The edge pass
// (GatV2EdgeOp) gathers X[j,:] once per entry, forms q_e over all H columns (a column tile beyond the first re-reads the other
// tiles' columns, in tile order: q_e, and so g_e, has the same bits in every tile), writes g and p and sums Gd and R for its
// own columns.  The transposed pass (GatV2BwdOp) gathers the destination's dY and X rows per entry of A^T and reads p and g by
// eid_t.  d att is a column reduction of R with fp64 partials per workgroup.  Lane groups (__shfl_xor), the four waves of a
// long-row item (LDS) and the chunks of a cut row (workspace partials, a second launch, slot order) combine in a fixed order:
// no float atomics, every entry bitwise repeatable for a given plan.  att, s, p, g, Gd and R are read from device memory when
// the kernels run.  No temporary is [nnz, H].
#include "spmm_gat_common.h"

namespace glass {

constexpr int kGatV2Gathers = 4;  // U of every pass here: one or two rows per entry in flight

// r_ec of one channel from the two rows' values: the same bits in the score, edge and transposed passes (the add commutes)
__device__ __forceinline__ float gatv2_u(float xi, float xj) { return __fadd_rn(xi, xj); }
__device__ __forceinline__ float gatv2_r(float u, float slope) { return u > 0.f ? u : __fmul_rn(slope, u); }

template <int LPR, class T>
__device__ __forceinline__ T gatv2_group_sum(T q) {
#pragma unroll
    for (int s = 1; s < LPR; s <<= 1) q += __shfl_xor(q, s);
    return q;
}

// ---- score pass: s_e for every entry of the forward CSR -------------------------------------------------------------------------
// One column tile (gridDim.y = 1): lane `sub` of a group owns columns (p * LPR + sub) * VW ... of every column pass p.  The
// row's own X and att of pass 0 stay in registers; further passes (H beyond LPR * VW columns: LPR = 64 then) re-read them.
template <int VW_, int LPR_>
struct GatV2ScoreOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kGatV2Gathers;
    using Acc = SumAcc<1>;  // (nothing per row)
    struct Slot {
        float x[VW];  // the source's message row, pass 0
        int c;        // the source, for the further passes
    };
    const int32_t* col;
    const float* val;
    const float* X;
    int64_t ldx;
    const float* att;
    float slope;
    float* s;  // [nnz]
    int H;

    __device__ __forceinline__ double dot(const float (&xi)[VW], const float (&xj)[VW], const float (&at)[VW], double q) const {
#pragma unroll
        for (int k = 0; k < VW; ++k) q = fma((double)at[k], (double)gatv2_r(gatv2_u(xi[k], xj[k]), slope), q);
        return q;
    }

    __device__ __forceinline__ void gather(Acc&, int row, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        constexpr int kPass = LPR * VW;
        const int coff = ln.coff;
        const float* Xi = X + (int64_t)row * ldx + coff;
        const float* Xc = X + coff;
        float xi[VW], at[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) xi[k] = at[k] = 0.f;
        if (ln.col_ok) {
            load_row<VW>(xi, Xi);
#pragma unroll
            for (int k = 0; k < VW; ++k) at[k] = att[coff + k];
        }
        const bool lead = ln.sub == 0;  // column 0: always a live column, so `ok` is "the entry exists" there
        entry_batches<LPR, U, Slot>(
            col, val, nullptr, e0, e1, ln,
            [&](Slot& sl, int c, bool ok) {
                load_row_if<VW>(ok, sl.x, Xc + (int64_t)c * ldx);
                sl.c = c;
            },
            [&](const Slot& sl, float, bool ok, int e) {
                double q = dot(xi, sl.x, at, 0.0);
                // (only at LPR = 64, one group per wave: the slot index stays below 64, so e < e1 says the entry exists)
                for (int c0 = kPass; c0 < H; c0 += kPass) {
                    float xa[VW], xb[VW], aa[VW];
#pragma unroll
                    for (int k = 0; k < VW; ++k) xa[k] = xb[k] = aa[k] = 0.f;
                    if (e < e1 && c0 + coff < H) {
                        load_row<VW>(xa, Xi + c0);
                        load_row<VW>(xb, Xc + (int64_t)sl.c * ldx + c0);
#pragma unroll
                        for (int k = 0; k < VW; ++k) aa[k] = att[c0 + coff + k];
                    }
                    q = dot(xa, xb, aa, q);
                }
                q = gatv2_group_sum<LPR>(q);
                if (ok && lead) s[e] = (float)q;
            });
    }
    __device__ __forceinline__ void store(const Acc&, int, int, int) const {}
};

// ---- forward: K1a's walk and accumulator, the score read per entry beside col / val ------------------------------------------------
template <int VW_, int LPR_>
struct GatV2FwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kGatFwdGathers;
    using Acc = GatAcc<VW>;
    struct Slot {
        float x[VW];  // the source's message row
        float sc;     // the entry's score
    };
    const int32_t* col;
    const float* val;
    const float* X;
    int64_t ldx;
    const float* s;  // [nnz]
    float* Y;
    int64_t ldy;
    float* L;    // [N]
    float* ps;   // partials of the chunks of cut rows: [n_slots, H] sums, then [n_slots] M, then [n_slots] Z
    float* pm;
    float* pz;
    int H;

    __device__ __forceinline__ void gather(Acc& acc, int, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        const float* Xc = X + ln.coff;
        entry_batches<LPR, U, Slot>(
            col, val, reinterpret_cast<const int32_t*>(s), e0, e1, ln,
            [&](Slot& sl, int c, bool ok, int32_t sb) {
                load_row_if<VW>(ok, sl.x, Xc + (int64_t)c * ldx);
                sl.sc = ok ? __int_as_float(sb) : 0.f;
            },
            [&](const Slot& sl, float v, bool ok, int) { acc.take(ok, v, sl.sc, sl.x); });
    }
    // (the lane of column 0 — column tile 0, lane 0 of the row — also writes the row's scalar)
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        if (slot < 0) {
            const bool any = acc.z > 0.f;
            float y[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) y[k] = any ? acc.s[k] / acc.z : 0.f;
            vec_from<VW>(y).store(Y + (int64_t)row * ldy + coff);
            if (coff == 0) L[row] = any ? acc.m + logf(acc.z) : 0.f;
        } else {
            vec_from<VW>(acc.s).store(ps + (int64_t)slot * H + coff);
            if (coff == 0) {
                pm[slot] = acc.m;
                pz[slot] = acc.z;
            }
        }
    }
};

// ---- edge pass: g_e and p_e for every entry of the forward CSR, Gd and R for every row ---------------------------------------------
// Column tile t (blockIdx.y) sums Gd and R for its own columns and gathers them once per entry; q_e and D_i run over the column
// passes p = 0, 1, ... in that order in EVERY tile — pass t from the registers, the others re-read (H beyond LPR * VW columns
// only: LPR = 64 then) — so g_e has the same bits in every tile.  Tile 0's first lane writes g[e] and p[e].
template <int VW_, int LPR_>
struct GatV2EdgeOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kGatV2Gathers;
    using Acc = SumAcc<2 * VW>;  // Gd's partial sums, then R's
    struct Slot {
        float x[VW];  // the source's message row, this tile's columns
        float sc;     // the entry's score
        int c;        // the source, for the other passes
    };
    const int32_t* col;
    const float* val;
    const float* X;
    int64_t ldx;
    const float* att;
    float slope;
    const float* s;  // [nnz]
    const float* dY;
    int64_t lddy;
    const float* Y;
    int64_t ldy;
    const float* L;
    float* g;    // [nnz]
    float* p;    // [nnz]
    float* Gd;   // [N, H]
    float* R;    // [N, H]
    float* psg;  // partials of the chunks of cut rows: [n_slots, H] of Gd, then [n_slots, H] of R
    float* psr;
    int H;

    static __device__ __forceinline__ float dot(const float (&a)[VW], const float (&b)[VW], float q) {
#pragma unroll
        for (int k = 0; k < VW; ++k) q = fmaf(a[k], b[k], q);
        return q;
    }

    __device__ __forceinline__ void gather(Acc& acc, int row, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        constexpr int kPass = LPR * VW;
        const int tile = blockIdx.y, coff = ln.coff, c_sub = ln.sub * VW;
        const bool multi = H > kPass;  // (uniform) several column tiles: LPR = 64, the slot index stays below 64
        const float* dYr = dY + (int64_t)row * lddy;
        const float* Yr = Y + (int64_t)row * ldy;
        float gi[VW], xi[VW], at[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) gi[k] = xi[k] = at[k] = 0.f;
        if (ln.col_ok) {
            load_row<VW>(gi, dYr + coff);
            load_row<VW>(xi, X + (int64_t)row * ldx + coff);
#pragma unroll
            for (int k = 0; k < VW; ++k) at[k] = att[coff + k];
        }
        float d = 0.f;
        for (int c0 = c_sub; c0 - c_sub < H; c0 += kPass) {  // (wave-uniform trip count)
            float gy[VW], yy[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) gy[k] = yy[k] = 0.f;
            if (c0 < H) {
                load_row<VW>(gy, dYr + c0);
                load_row<VW>(yy, Yr + c0);
            }
            d = dot(gy, yy, d);
        }
        const float Di = gatv2_group_sum<LPR>(d);
        const float Li = L[row];
        const float* Xc = X + coff;
        const bool lead = tile == 0 && ln.sub == 0;  // column 0: always live, so `ok` is "the entry exists" there
        entry_batches<LPR, U, Slot>(
            col, val, reinterpret_cast<const int32_t*>(s), e0, e1, ln,
            [&](Slot& sl, int c, bool ok, int32_t sb) {
                load_row_if<VW>(ok, sl.x, Xc + (int64_t)c * ldx);
                sl.sc = __int_as_float(sb);
                sl.c = c;
            },
            [&](const Slot& sl, float v, bool ok, int e) {
                const bool ent = multi ? e < e1 : ok;  // the entry exists (a lane without a live column here still has some in other passes)
                float q = 0.f;
                int pass = 0;
                for (int c0 = c_sub; c0 - c_sub < H; c0 += kPass, ++pass) {
                    if (pass == tile) {
                        q = dot(gi, sl.x, q);
                        continue;
                    }
                    float gy[VW], xx[VW];
#pragma unroll
                    for (int k = 0; k < VW; ++k) gy[k] = xx[k] = 0.f;
                    if (ent && c0 < H) {
                        load_row<VW>(gy, dYr + c0);
                        load_row<VW>(xx, X + (int64_t)sl.c * ldx + c0);
                    }
                    q = dot(gy, xx, q);
                }
                q = gatv2_group_sum<LPR>(q);
                const float pe = v * expf(sl.sc - Li);
                const float ge = ent ? pe * (q - Di) : 0.f;
                const float gs = ge * slope;
#pragma unroll
                for (int k = 0; k < VW; ++k) {
                    const float u = gatv2_u(xi[k], sl.x[k]);
                    const float sg = fmaf(u > 0.f ? ge : gs, at[k], acc.s[k]);
                    const float sr = fmaf(ge, gatv2_r(u, slope), acc.s[VW + k]);
                    acc.s[k] = ok ? sg : acc.s[k];
                    acc.s[VW + k] = ok ? sr : acc.s[VW + k];
                }
                if (ok && lead) {
                    g[e] = ge;
                    p[e] = pe;
                }
            });
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        float a[VW], r[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            a[k] = acc.s[k];
            r[k] = acc.s[VW + k];
        }
        const int64_t at = (int64_t)(slot < 0 ? row : slot) * H + coff;
        vec_from<VW>(a).store((slot < 0 ? Gd : psg) + at);
        vec_from<VW>(r).store((slot < 0 ? R : psr) + at);
    }
};

// ---- transposed pass: row j of A^T; per entry the destination's dY row and X row, the entry's p and g (through eid_t) ----------------
template <int VW_, int LPR_>
struct GatV2BwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kGatV2Gathers;
    using Acc = SumAcc<VW>;
    struct Slot {
        float dy[VW];  // the destination's dY row
        float x[VW];   // and its message row
        float p, g;    // this entry's p and g
    };
    const int32_t* col;  // the transposed CSR: destinations
    const float* val;
    const int32_t* eid;  // index of each transposed entry in the forward CSR
    const float* X;
    int64_t ldx;
    const float* att;
    float slope;
    const float* dY;
    int64_t lddy;
    const float* p;   // [nnz], forward entry order
    const float* g;
    const float* Gd;  // [N, H]
    float* dX;
    int64_t lddx;
    float* ps;        // partials of the chunks of cut rows: [n_slots, H]
    int H;

    __device__ __forceinline__ void gather(Acc& acc, int row, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        const int coff = ln.coff;
        float xj[VW], at[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) xj[k] = at[k] = 0.f;
        if (ln.col_ok) {
            load_row<VW>(xj, X + (int64_t)row * ldx + coff);
#pragma unroll
            for (int k = 0; k < VW; ++k) at[k] = att[coff + k];
        }
        const float* dYc = dY + coff;
        const float* Xc = X + coff;
        entry_batches<LPR, U, Slot>(
            col, val, eid, e0, e1, ln,
            [&](Slot& sl, int c, bool ok, int32_t e) {
                load_row_if<VW>(ok, sl.dy, dYc + (int64_t)c * lddy);
                load_row_if<VW>(ok, sl.x, Xc + (int64_t)c * ldx);
                sl.p = ok ? p[e] : 0.f;
                sl.g = ok ? g[e] : 0.f;
            },
            [&](const Slot& sl, float, bool, int) {  // (a masked slot holds zeros: it adds nothing)
                const float gs = sl.g * slope;
#pragma unroll
                for (int k = 0; k < VW; ++k) {
                    const float u = gatv2_u(sl.x[k], xj[k]);
                    acc.s[k] = fmaf(u > 0.f ? sl.g : gs, at[k], fmaf(sl.p, sl.dy[k], acc.s[k]));
                }
            });
    }
    // a whole row: Gd[j,:] is added here; a chunk of a cut row: left to the reduce launch, which adds it once
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        if (slot < 0) {
            float r[VW];
            load_row<VW>(r, Gd + (int64_t)row * H + coff);
#pragma unroll
            for (int k = 0; k < VW; ++k) r[k] += acc.s[k];
            vec_from<VW>(r).store(dX + (int64_t)row * lddx + coff);
        } else {
            vec_from<VW>(acc.s).store(ps + (int64_t)slot * H + coff);
        }
    }
};

__global__ __launch_bounds__(kBlock) void spmm_gatv2_bwd_reduce_kernel(const float* __restrict__ ps, const float* __restrict__ Gd,
                                                                       float* __restrict__ dX, int64_t lddx, int H,
                                                                       const int32_t* __restrict__ rrows) {
    const int32_t* rr = rrows + 3 * (int64_t)blockIdx.x;
    const int row = rr[0], first = rr[1], n = rr[2];
    for (int c = threadIdx.x; c < H; c += kBlock) {
        float s = 0.f;
        for (int k = 0; k < n; ++k) s += ps[(int64_t)(first + k) * H + c];
        dX[(int64_t)row * lddx + c] = Gd[(int64_t)row * H + c] + s;
    }
}

// ---- d att: the column sums of R over the N rows (the layout of K1a's gat_datt kernels, one sum) -----------------------------------
// Workgroup w takes rows [w * rpw, (w + 1) * rpw); a thread owns column (t % hc) of a column block and every nrs-th row
// (nrs = 256 / hc row phases, hc = the power of two covering H, at most 256); the phases are added through LDS in phase
// order.  part [n_wg][H] fp64.
__global__ __launch_bounds__(kBlock) void gatv2_datt_partial_kernel(const float* __restrict__ R, int64_t n_rows, int H, int hc,
                                                                    int64_t rpw, double* __restrict__ part) {
    __shared__ double lds[kBlock];
    const int t = threadIdx.x;
    const int nrs = kBlock / hc, c0 = t % hc, rs = t / hc;
    const int64_t r0 = (int64_t)blockIdx.x * rpw, r1 = r0 + rpw < n_rows ? r0 + rpw : n_rows;
    for (int cb = 0; cb < H; cb += hc) {  // (one round unless H > 256, where nrs = 1)
        const int c = cb + c0;
        double sa = 0.0;
        if (c < H)
            for (int64_t r = r0 + rs; r < r1; r += nrs) sa += (double)R[r * H + c];
        if (nrs > 1) {
            lds[t] = sa;
            __syncthreads();
            if (rs == 0)
                for (int k = 1; k < nrs; ++k) sa += lds[k * hc + c0];
        }
        if (rs == 0 && c < H) part[(int64_t)blockIdx.x * H + c] = sa;
    }
}

// the workgroups' partials in workgroup order, one thread per column
__global__ __launch_bounds__(kBlock) void gatv2_datt_final_kernel(const double* __restrict__ part, int64_t n_wg, int H,
                                                                  float* __restrict__ datt) {
    for (int c = threadIdx.x; c < H; c += kBlock) {
        double sa = 0.0;
        for (int64_t w = 0; w < n_wg; ++w) sa += part[w * H + c];
        datt[c] = (float)sa;
    }
}

inline int64_t gatv2_datt_rows_per_wg(int64_t H) { return H > 128 ? 2 * H : 256; }  // partials stay within [N] + H doubles

// ---- launches -----------------------------------------------------------------------------------------------------------------
// the item walk with ONE column tile: the operation loops over the column passes itself
template <int VW, int LPR>
static int launch_gatv2_score(GatV2ScoreOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan,
                              hipStream_t st) {
    const ItemsGrid gr = items_grid(op, hdr);
    if (gr.blocks > 0)
        hipLaunchKernelGGL((k1_items_kernel<GatV2ScoreOp<VW, LPR>>), dim3(gr.blocks, 1), dim3(kBlock), 0, st, op, rowptr,
                           plan + hdr[H_OFF_SWEEP], gr.n_waves, plan + hdr[H_OFF_LONG], gr.n_sweep_blocks);
    return launch_status("glass_spmm_gatv2_score_f32");
}

template <int VW, int LPR>
static int launch_gatv2_fwd(GatV2FwdOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    launch_items(op, rowptr, hdr, plan, st);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_gat_reduce_kernel<>, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, op.ps, op.pm, op.pz, op.Y,
                           op.ldy, op.L, op.H, plan + hdr[H_OFF_REDUCE]);
    return launch_status("glass_spmm_gatv2_csr_f32");
}

template <int VW, int LPR>
static int launch_gatv2_edge(GatV2EdgeOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan,
                             hipStream_t st) {
    launch_items(op, rowptr, hdr, plan, st);
    launch_items_reduce(op.psg, op.Gd, op.H, op.H, hdr, plan, st);
    launch_items_reduce(op.psr, op.R, op.H, op.H, hdr, plan, st);
    return launch_status("glass_spmm_gatv2_edge_f32");
}

template <int VW, int LPR>
static int launch_gatv2_bwd(GatV2BwdOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    launch_items(op, rowptr, hdr, plan, st);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_gatv2_bwd_reduce_kernel, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, op.ps, op.Gd, op.dX,
                           op.lddx, op.H, plan + hdr[H_OFF_REDUCE]);
    return launch_status("glass_spmm_gatv2_bwd_f32");
}

// slots * per_slot floats, or the code of a header that is no plan / a width that is none
static int64_t gatv2_ws_bytes(const int32_t* hdr, int64_t H, int64_t per_slot) {
    if (!hdr || hdr[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr[H_NSLOTS] * per_slot * (int64_t)sizeof(float);
}

}  // namespace glass

using namespace glass;

extern "C" int64_t glass_spmm_gatv2_score_ws_bytes(const int32_t* hdr, int64_t H) { return gatv2_ws_bytes(hdr, H, 0); }
extern "C" int64_t glass_spmm_gatv2_ws_bytes(const int32_t* hdr, int64_t H) { return gatv2_ws_bytes(hdr, H, H + 2); }
extern "C" int64_t glass_spmm_gatv2_edge_ws_bytes(const int32_t* hdr, int64_t H) { return gatv2_ws_bytes(hdr, H, 2 * H); }
extern "C" int64_t glass_spmm_gatv2_bwd_ws_bytes(const int32_t* hdr_t, int64_t H) { return gatv2_ws_bytes(hdr_t, H, H); }

extern "C" int64_t glass_spmm_gatv2_datt_ws_bytes(int64_t n_rows, int64_t H) {
    if (H <= 0 || n_rows < 0) return GLASS_E_ARG;
    return ceil_div(n_rows, gatv2_datt_rows_per_wg(H)) * H * (int64_t)sizeof(double);
}

extern "C" int glass_spmm_gatv2_score_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                          const float* att, float slope, float* s, int64_t n_rows, int64_t H, const int32_t* hdr,
                                          const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && att && hdr && plan_dev, "spmm_gatv2_score: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col) && aligned4(val) && aligned4(X) && aligned4(att) && aligned4(s) &&
                  aligned4(plan_dev) && aligned4(ws), "spmm_gatv2_score: pointer not 4-byte aligned");
    GLASS_REQUIRE(n_rows >= 0 && H > 0 && ldx >= H, "spmm_gatv2_score: need n_rows>=0, H>0, ldx>=H (H=%lld ldx=%lld)", (long long)H,
                  (long long)ldx);
    GLASS_REQUIRE(slope == slope, "spmm_gatv2_score: slope is NaN");
    if (const int rc = check_plan("spmm_gatv2_score", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val && s), "spmm_gatv2_score: null col/val/s");
    if (n_rows == 0 || hdr[H_NNZ] == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && aligned16(X);
#define GLASS_K1A2_SCORE_CASE(VW, LPR) \
    return launch_gatv2_score(GatV2ScoreOp<VW, LPR>{col, val, X, ldx, att, slope, s, (int)H}, rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1A2_SCORE_CASE);
#undef GLASS_K1A2_SCORE_CASE
}

extern "C" int glass_spmm_gatv2_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                        const float* s, float* Y, int64_t ldy, float* L, int64_t n_rows, int64_t H,
                                        const int32_t* hdr, const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && Y && L && hdr && plan_dev, "spmm_gatv2: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col) && aligned4(val) && aligned4(X) && aligned4(s) && aligned4(Y) && aligned4(L) &&
                  aligned4(plan_dev) && aligned4(ws), "spmm_gatv2: pointer not 4-byte aligned");
    GLASS_REQUIRE(n_rows >= 0 && H > 0 && ldx >= H && ldy >= H, "spmm_gatv2: need n_rows>=0, H>0, ldx>=H, ldy>=H (H=%lld ldx=%lld ldy=%lld)", (long long)H,
                  (long long)ldx, (long long)ldy);
    if (const int rc = check_plan("spmm_gatv2", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val && s), "spmm_gatv2: null col/val/s");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_gatv2: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0 || hdr[H_NNZ] == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* ps = (float*)ws;
    float* pm = ps + (int64_t)hdr[H_NSLOTS] * H;
    float* pz = pm + hdr[H_NSLOTS];
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && aligned16(X) && aligned16(Y) &&
                     (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1A2_FWD_CASE(VW, LPR) \
    return launch_gatv2_fwd(GatV2FwdOp<VW, LPR>{col, val, X, ldx, s, Y, ldy, L, ps, pm, pz, (int)H}, rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1A2_FWD_CASE);
#undef GLASS_K1A2_FWD_CASE
}

extern "C" int glass_spmm_gatv2_edge_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                         const float* att, float slope, const float* s, const float* dY, int64_t lddy,
                                         const float* Y, int64_t ldy, const float* L, float* g, float* p, float* Gd, float* R,
                                         int64_t n_rows, int64_t H, const int32_t* hdr, const int32_t* plan_dev, void* ws,
                                         void* stream) {
    GLASS_REQUIRE(rowptr && X && att && dY && Y && L && Gd && R && hdr && plan_dev, "spmm_gatv2_edge: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col) && aligned4(val) && aligned4(X) && aligned4(att) && aligned4(s) && aligned4(dY) &&
                  aligned4(Y) && aligned4(L) && aligned4(g) && aligned4(p) && aligned4(Gd) && aligned4(R) && aligned4(plan_dev) &&
                  aligned4(ws), "spmm_gatv2_edge: pointer not 4-byte aligned");
    GLASS_REQUIRE(n_rows >= 0 && H > 0 && ldx >= H && lddy >= H && ldy >= H,
                  "spmm_gatv2_edge: need n_rows>=0, H>0 and every ld >= H (H=%lld ldx=%lld lddy=%lld ldy=%lld)", (long long)H, (long long)ldx,
                  (long long)lddy, (long long)ldy);
    GLASS_REQUIRE(slope == slope, "spmm_gatv2_edge: slope is NaN");
    if (const int rc = check_plan("spmm_gatv2_edge", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val && s && g && p), "spmm_gatv2_edge: null col/val/s/g/p");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_gatv2_edge: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0 || hdr[H_NNZ] == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* psg = (float*)ws;
    float* psr = psg + (int64_t)hdr[H_NSLOTS] * H;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (lddy % 4 == 0) && (ldy % 4 == 0) && aligned16(X) && aligned16(dY) &&
                     aligned16(Y) && aligned16(Gd) && aligned16(R) && (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1A2_EDGE_CASE(VW, LPR)                                                                                              \
    return launch_gatv2_edge(GatV2EdgeOp<VW, LPR>{col, val, X, ldx, att, slope, s, dY, lddy, Y, ldy, L, g, p, Gd, R, psg, psr, (int)H}, \
                             rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1A2_EDGE_CASE);
#undef GLASS_K1A2_EDGE_CASE
}

extern "C" int glass_spmm_gatv2_bwd_f32(const int32_t* rowptr, const int32_t* col_t, const float* val_t, const int32_t* eid_t,
                                        const float* X, int64_t ldx, const float* att, float slope, const float* dY, int64_t lddy,
                                        const float* p, const float* g, const float* Gd, float* dX, int64_t lddx, int64_t n_rows,
                                        int64_t H, const int32_t* hdr, const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && att && dY && Gd && dX && hdr && plan_dev, "spmm_gatv2_bwd: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col_t) && aligned4(val_t) && aligned4(eid_t) && aligned4(X) && aligned4(att) &&
                  aligned4(dY) && aligned4(p) && aligned4(g) && aligned4(Gd) && aligned4(dX) && aligned4(plan_dev) && aligned4(ws),
                  "spmm_gatv2_bwd: pointer not 4-byte aligned");
    GLASS_REQUIRE(n_rows >= 0 && H > 0 && ldx >= H && lddy >= H && lddx >= H,
                  "spmm_gatv2_bwd: need n_rows>=0, H>0 and every ld >= H (H=%lld ldx=%lld lddy=%lld lddx=%lld)", (long long)H, (long long)ldx,
                  (long long)lddy, (long long)lddx);
    GLASS_REQUIRE(slope == slope, "spmm_gatv2_bwd: slope is NaN");
    if (const int rc = check_plan("spmm_gatv2_bwd", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col_t && val_t && eid_t && p && g), "spmm_gatv2_bwd: null col_t/val_t/eid_t/p/g");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_gatv2_bwd: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0 || hdr[H_NNZ] == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (lddy % 4 == 0) && (lddx % 4 == 0) && aligned16(X) && aligned16(dY) &&
                     aligned16(Gd) && aligned16(dX) && (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1A2_BWD_CASE(VW, LPR)                                                                                              \
    return launch_gatv2_bwd(GatV2BwdOp<VW, LPR>{col_t, val_t, eid_t, X, ldx, att, slope, dY, lddy, p, g, Gd, dX, lddx, (float*)ws, \
                                                (int)H},                                                                           \
                            rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1A2_BWD_CASE);
#undef GLASS_K1A2_BWD_CASE
}

extern "C" int glass_spmm_gatv2_datt_f32(const float* R, float* datt, int64_t n_rows, int64_t H, void* ws, void* stream) {
    GLASS_REQUIRE(R && datt, "spmm_gatv2_datt: null pointer");
    GLASS_REQUIRE(aligned4(R) && aligned4(datt), "spmm_gatv2_datt: pointer not 4-byte aligned");
    GLASS_REQUIRE(aligned8(ws), "spmm_gatv2_datt: ws not 8-byte aligned");
    GLASS_REQUIRE(H > 0 && n_rows >= 0 && n_rows < (1ll << 31), "spmm_gatv2_datt: need H>0, 0 <= n_rows < 2^31 (H=%lld n=%lld)",
                  (long long)H, (long long)n_rows);
    if (H > kMaxH) {
        set_error("spmm_gatv2_datt: H = %lld is beyond the %lld columns the aggregation covers", (long long)H, (long long)kMaxH);
        return GLASS_E_UNSUPPORTED;
    }
    GLASS_REQUIRE(n_rows == 0 || ws, "spmm_gatv2_datt: ws is null");
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t rpw = gatv2_datt_rows_per_wg(H), n_wg = ceil_div(n_rows, rpw);
    const int hc = pow2_ceil_cap(H, kBlock);
    hipLaunchKernelGGL(gatv2_datt_partial_kernel, dim3((unsigned)n_wg), dim3(kBlock), 0, st, R, n_rows, (int)H, hc, rpw, (double*)ws);
    hipLaunchKernelGGL(gatv2_datt_final_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)ws, n_wg, (int)H, datt);
    return launch_status("glass_spmm_gatv2_datt_f32");
}
