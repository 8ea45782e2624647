// K1a: attention neighbour aggregation (aggr "gat", an extension: the reference has none; single-head GAT, Velickovic et al.
// 2018) on K1's CSR, plans and lane layout.  X [N, H] the messages, att_src / att_dst two [H] vectors, slope LeakyReLU's
// negative slope.  Per destination i, over the entries e of row i (source j = col[e], weight v_e > 0, a multiplicity):
//
//   a_j = sum_c X[j,c] att_src[c]       b_i = sum_c X[i,c] att_dst[c]       (glass_gat_scores_f32: fp64 sums, fixed order)
//   u_e = a_j + b_i                     s_e = u_e > 0 ? u_e : slope * u_e   (one rounded add, one rounded multiply: gat_score)
//   M = max_e s_e     Z = sum_e v_e exp(s_e - M)     Y[i,:] = sum_e v_e exp(s_e - M) X[j,:] / Z     L_i = M + log Z
//   a row without entries: Y = 0, L = 0
//
//   backward, p_e = v_e exp(s_e - L_i), f_e = u_e > 0 ? 1 : slope (torch's leaky_relu rule: u == 0 takes slope):
//   D_i = sum_c dY[i,c] Y[i,c]          q_e = sum_c dY[i,c] X[j,c]          g_e = p_e (q_e - D_i) f_e
//   da_j = sum over the entries with col = j of g_e                        db_i = sum over the entries of row i of g_e
//   dX[j,:] = sum over the entries with col = j of p_e dY[i,:]  +  da_j att_src  +  db_j att_dst
//   d att_src[c] = sum_j da_j X[j,c]    d att_dst[c] = sum_i db_i X[i,c]
//
// Four passes.  The forward (GatFwdOp) and the transposed pass (GatBwdOp) are operations of the item walk of spmm_items.h, as
// K1m's and K1s's; their state is one scalar pair or sum per lane — the same on every lane of a row — beside VW running sums.
// The edge pass (GatEdgeOp) is the library's sampled dense-dense product: per entry the lane group forms the whole dot q_e,
// looping over the column passes inside the kernel (its grid has one column tile), and leaves g [nnz] in forward entry order
// and db [N].  The attention vectors' gradients are two column reductions with fp64 partials per workgroup and a
// one-workgroup final stage.  Lane groups (__shfl_xor), the four waves of a long-row item (LDS) and the chunks of a cut row
// (workspace partials, a small second launch, slot order) combine in a fixed order: no float atomics, every entry bitwise
// repeatable for a given plan.  a, b, L, g, db, att_src and att_dst are read from device memory when the kernels run.
#include "spmm_gat_common.h"

namespace glass {

// ---- node scores: a = X att_src, b = X att_dst ------------------------------------------------------------------------------
// one wave per row; lane l sums columns l, l + 64, ... in fp64, then the lanes in a butterfly: a fixed order
__global__ __launch_bounds__(kBlock) void gat_scores_kernel(const float* __restrict__ X, int64_t ldx,
                                                            const float* __restrict__ att_src,
                                                            const float* __restrict__ att_dst, float* __restrict__ a,
                                                            float* __restrict__ b, int64_t n_rows, int H) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t row = (int64_t)blockIdx.x * kScoreRows + (threadIdx.x >> 6);
    if (row >= n_rows) return;  // (whole waves)
    const float* x = X + row * ldx;
    double sa = 0.0, sb = 0.0;
    for (int c = lane; c < H; c += kWave) {
        const double xv = (double)x[c];
        sa = fma(xv, (double)att_src[c], sa);
        sb = fma(xv, (double)att_dst[c], sb);
    }
    sa = wave_sum(sa);
    sb = wave_sum(sb);
    if (lane == 0) {
        a[row] = (float)sa;
        b[row] = (float)sb;
    }
}


// ---- forward ------------------------------------------------------------------------------------------------------------------
template <int VW_, int LPR_>
struct GatFwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kGatFwdGathers;
    using Acc = GatAcc<VW>;
    struct Slot {
        float x[VW];  // the source's message row
        float a;      // and its score
    };
    const int32_t* col;
    const float* val;
    const float* X;
    int64_t ldx;
    const float* a;
    const float* b;
    float slope;
    float* Y;
    int64_t ldy;
    float* L;    // [N]
    float* ps;   // partials of the chunks of cut rows: [n_slots, H] sums, then [n_slots] M, then [n_slots] Z
    float* pm;
    float* pz;
    int H;

    __device__ __forceinline__ void gather(Acc& acc, int row, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        const float* Xc = X + ln.coff;
        const float bi = b[row];
        entry_batches<LPR, U, Slot>(
            col, val, nullptr, e0, e1, ln,
            [&](Slot& s, int c, bool ok) {
                load_row_if<VW>(ok, s.x, Xc + (int64_t)c * ldx);
                s.a = ok ? a[c] : 0.f;
            },
            [&](const Slot& s, float v, bool ok, int) { acc.take(ok, v, gat_score(s.a, bi, slope), s.x); });
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

// ---- edge pass: g_e for every entry of the forward CSR, db_i for every row ---------------------------------------------------
// One column tile (gridDim.y = 1): lane `sub` of a group owns columns (p * LPR + sub) * VW ... of every column pass p.  The row's
// dY of pass 0 stays in registers; further passes (H beyond LPR * VW columns: LPR = 64 then, one group per wave) re-read it.
template <int VW_, int LPR_>
struct GatEdgeOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kGatEdgeGathers;
    using Acc = SumAcc<1>;  // db's partial sum, on the lanes with sub == 0
    struct Slot {
        float x[VW];  // the source's message row, pass 0
        float a;      // its score
        int c;        // the source, for the further passes
    };
    const int32_t* col;
    const float* val;
    const float* X;
    int64_t ldx;
    const float* a;
    const float* b;
    float slope;
    const float* dY;
    int64_t lddy;
    const float* Y;
    int64_t ldy;
    const float* L;
    float* g;         // [nnz]
    float* db;        // [N]
    float* partials;  // [n_slots] db of the chunks of cut rows
    int H;

    static __device__ __forceinline__ float group_sum(float q) {
#pragma unroll
        for (int s = 1; s < LPR; s <<= 1) q += __shfl_xor(q, s);
        return q;
    }
    static __device__ __forceinline__ float dot(const float (&p)[VW], const float (&r)[VW], float q) {
#pragma unroll
        for (int k = 0; k < VW; ++k) q = fmaf(p[k], r[k], q);
        return q;
    }

    __device__ __forceinline__ void gather(Acc& acc, int row, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        constexpr int kPass = LPR * VW;
        const float* dYr = dY + (int64_t)row * lddy;
        const float* Yr = Y + (int64_t)row * ldy;
        const int coff = ln.coff;
        float gi[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) gi[k] = 0.f;
        if (ln.col_ok) load_row<VW>(gi, dYr + coff);
        float d = 0.f;
        for (int c0 = 0; c0 < H; c0 += kPass) {  // (wave-uniform)
            float gy[VW], yy[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) gy[k] = yy[k] = 0.f;
            if (c0 + coff < H) {
                load_row<VW>(gy, dYr + c0 + coff);
                load_row<VW>(yy, Yr + c0 + coff);
            }
            d = dot(gy, yy, d);
        }
        const float Di = group_sum(d);
        const float Li = L[row], bi = b[row];
        const float* Xc = X + coff;
        const bool lead = ln.sub == 0;  // column 0: always a live column, so `ok` is "the entry exists" there
        entry_batches<LPR, U, Slot>(
            col, val, nullptr, e0, e1, ln,
            [&](Slot& s, int c, bool ok) {
                load_row_if<VW>(ok, s.x, Xc + (int64_t)c * ldx);
                s.a = ok ? a[c] : 0.f;
                s.c = c;
            },
            [&](const Slot& s, float v, bool ok, int e) {
                float q = dot(gi, s.x, 0.f);
                for (int c0 = kPass; c0 < H; c0 += kPass) {  // (only at LPR = 64, where every lane has a live column in pass 0)
                    float gy[VW], xx[VW];
#pragma unroll
                    for (int k = 0; k < VW; ++k) gy[k] = xx[k] = 0.f;
                    if (ok && c0 + coff < H) {
                        load_row<VW>(gy, dYr + c0 + coff);
                        load_row<VW>(xx, Xc + (int64_t)s.c * ldx + c0);
                    }
                    q = dot(gy, xx, q);
                }
                q = group_sum(q);
                const float p = v * expf(gat_score(s.a, bi, slope) - Li);
                const float ge = p * (q - Di) * gat_slope_of(s.a, bi, slope);
                if (ok && lead) {
                    g[e] = ge;
                    acc.s[0] += ge;
                }
            });
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        if (coff != 0) return;
        if (slot < 0) db[row] = acc.s[0];
        else partials[slot] = acc.s[0];
    }
};

// db of the rows cut into several chunks, in slot order: one thread per row
__global__ __launch_bounds__(kBlock) void spmm_gat_edge_reduce_kernel(const float* __restrict__ partials, float* __restrict__ db,
                                                                      const int32_t* __restrict__ rrows, int n_reduce) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_reduce) return;
    const int32_t* rr = rrows + 3 * (int64_t)i;
    const int row = rr[0], first = rr[1], n = rr[2];
    float s = 0.f;
    for (int k = 0; k < n; ++k) s += partials[first + k];
    db[row] = s;
}

// ---- transposed pass: row j of A^T; per entry the destination's dY row, b, L and the entry's g (through eid_t) -----------------
// DX = false is the same walk for da alone (glass_spmm_gat_da_f32: the attention vectors are trained, X needs no gradient):
// one column tile, no dY row, no exponential — and, entry for entry, the additions of the full pass at this lane layout, so
// da has the same bits either way.
template <int VW_, int LPR_, bool DX>
struct GatBwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kGatBwdGathers;
    using Acc = GatBwdAcc<VW>;
    struct Slot {
        float dy[VW];    // the destination's dY row
        float b, l, g;   // its b and L, this entry's g
    };
    const int32_t* col;   // the transposed CSR: destinations
    const float* val;
    const int32_t* eid;   // index of each transposed entry in the forward CSR
    const float* a;
    const float* b;
    float slope;
    const float* dY;
    int64_t lddy;
    const float* L;
    const float* g;
    const float* db;
    const float* att_src;
    const float* att_dst;
    float* dX;
    int64_t lddx;
    float* da;            // [N]
    float* ps;            // partials of the chunks of cut rows: [n_slots, H] sums, then [n_slots] da
    float* pda;
    int H;

    __device__ __forceinline__ void gather(Acc& acc, int row, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        if constexpr (!DX) {
            entry_batches<LPR, U, Slot>(
                col, val, eid, e0, e1, ln, [&](Slot& s, int, bool ok, int32_t e) { s.g = ok ? g[e] : 0.f; },
                [&](const Slot& s, float, bool, int) { acc.da += s.g; });
            return;
        }
        const float aj = a[row];
        const float* dYc = dY + ln.coff;
        entry_batches<LPR, U, Slot>(
            col, val, eid, e0, e1, ln,
            [&](Slot& s, int c, bool ok, int32_t e) {
                load_row_if<VW>(ok, s.dy, dYc + (int64_t)c * lddy);
                s.b = ok ? b[c] : 0.f;
                s.l = ok ? L[c] : 0.f;
                s.g = ok ? g[e] : 0.f;
            },
            [&](const Slot& s, float v, bool ok, int) {
                const float pe = v * expf(gat_score(aj, s.b, slope) - s.l);
                const float p = ok ? pe : 0.f;
#pragma unroll
                for (int k = 0; k < VW; ++k) acc.s[k] = fmaf(p, s.dy[k], acc.s[k]);
                acc.da += s.g;
            });
    }
    // a whole row: the two rank-one terms are added here; a chunk of a cut row: left to the reduce launch, which adds them once
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        if constexpr (!DX) {
            if (coff == 0) (slot < 0 ? da[row] : pda[slot]) = acc.da;
            return;
        }
        if (slot < 0) {
            const float dbj = db[row];
            float r[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) r[k] = fmaf(dbj, att_dst[coff + k], fmaf(acc.da, att_src[coff + k], acc.s[k]));
            vec_from<VW>(r).store(dX + (int64_t)row * lddx + coff);
            if (coff == 0) da[row] = acc.da;
        } else {
            vec_from<VW>(acc.s).store(ps + (int64_t)slot * H + coff);
            if (coff == 0) pda[slot] = acc.da;
        }
    }
};

__global__ __launch_bounds__(kBlock) void spmm_gat_bwd_reduce_kernel(const float* __restrict__ ps, const float* __restrict__ pda,
                                                                     const float* __restrict__ db,
                                                                     const float* __restrict__ att_src,
                                                                     const float* __restrict__ att_dst, float* __restrict__ dX,
                                                                     int64_t lddx, float* __restrict__ da, int H,
                                                                     const int32_t* __restrict__ rrows) {
    const int32_t* rr = rrows + 3 * (int64_t)blockIdx.x;
    const int row = rr[0], first = rr[1], n = rr[2];
    float daj = 0.f;
    for (int k = 0; k < n; ++k) daj += pda[first + k];
    if (threadIdx.x == 0) da[row] = daj;
    if (!dX) return;  // (the da-only form; uniform)
    const float dbj = db[row];
    for (int c = threadIdx.x; c < H; c += kBlock) {
        float s = 0.f;
        for (int k = 0; k < n; ++k) s += ps[(int64_t)(first + k) * H + c];
        dX[(int64_t)row * lddx + c] = fmaf(dbj, att_dst[c], fmaf(daj, att_src[c], s));
    }
}

// ---- the attention vectors' gradients: two column reductions over the N rows --------------------------------------------------
// Workgroup w takes rows [w * rpw, (w + 1) * rpw); a thread owns column (t % hc) of a column block and every nrs-th row
// (nrs = 256 / hc row phases, hc = the power of two covering H, at most 256); the phases are added through LDS in phase
// order.  part [n_wg][2][H] fp64.
__global__ __launch_bounds__(kBlock) void gat_datt_partial_kernel(const float* __restrict__ X, int64_t ldx,
                                                                  const float* __restrict__ da, const float* __restrict__ db,
                                                                  int64_t n_rows, int H, int hc, int64_t rpw,
                                                                  double* __restrict__ part) {
    __shared__ double lds[2][kBlock];
    const int t = threadIdx.x;
    const int nrs = kBlock / hc, c0 = t % hc, rs = t / hc;
    const int64_t r0 = (int64_t)blockIdx.x * rpw, r1 = r0 + rpw < n_rows ? r0 + rpw : n_rows;
    for (int cb = 0; cb < H; cb += hc) {  // (one round unless H > 256, where nrs = 1)
        const int c = cb + c0;
        double sa = 0.0, sb = 0.0;
        if (c < H)
            for (int64_t r = r0 + rs; r < r1; r += nrs) {
                const double x = (double)X[r * ldx + c];
                sa = fma((double)da[r], x, sa);
                sb = fma((double)db[r], x, sb);
            }
        if (nrs > 1) {
            lds[0][t] = sa;
            lds[1][t] = sb;
            __syncthreads();
            if (rs == 0)
                for (int k = 1; k < nrs; ++k) {
                    sa += lds[0][k * hc + c0];
                    sb += lds[1][k * hc + c0];
                }
        }
        if (rs == 0 && c < H) {
            part[((int64_t)blockIdx.x * 2 + 0) * H + c] = sa;
            part[((int64_t)blockIdx.x * 2 + 1) * H + c] = sb;
        }
    }
}

// the workgroups' partials in workgroup order, one thread per column
__global__ __launch_bounds__(kBlock) void gat_datt_final_kernel(const double* __restrict__ part, int64_t n_wg, int H,
                                                                float* __restrict__ datt_src, float* __restrict__ datt_dst) {
    for (int c = threadIdx.x; c < H; c += kBlock) {
        double sa = 0.0, sb = 0.0;
        for (int64_t w = 0; w < n_wg; ++w) {
            sa += part[(w * 2 + 0) * H + c];
            sb += part[(w * 2 + 1) * H + c];
        }
        datt_src[c] = (float)sa;
        datt_dst[c] = (float)sb;
    }
}

inline int64_t datt_rows_per_wg(int64_t H) { return H > 128 ? 2 * H : 256; }  // partials stay within [N] + 2 H doubles

// ---- launches -----------------------------------------------------------------------------------------------------------------
template <int VW, int LPR>
static int launch_gat_fwd(GatFwdOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    launch_items(op, rowptr, hdr, plan, st);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_gat_reduce_kernel<>, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, op.ps, op.pm, op.pz, op.Y,
                           op.ldy, op.L, op.H, plan + hdr[H_OFF_REDUCE]);
    return launch_status("glass_spmm_gat_csr_f32");
}

// the item walk with ONE column tile: the operation loops over the column passes itself
template <int VW, int LPR>
static int launch_gat_edge(GatEdgeOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan, hipStream_t st) {
    const ItemsGrid gr = items_grid(op, hdr);
    if (gr.blocks > 0)
        hipLaunchKernelGGL((k1_items_kernel<GatEdgeOp<VW, LPR>>), dim3(gr.blocks, 1), dim3(kBlock), 0, st, op, rowptr,
                           plan + hdr[H_OFF_SWEEP], gr.n_waves, plan + hdr[H_OFF_LONG], gr.n_sweep_blocks);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_gat_edge_reduce_kernel, dim3((unsigned)ceil_div(hdr[H_NREDUCE], kBlock)), dim3(kBlock), 0, st,
                           op.partials, op.db, plan + hdr[H_OFF_REDUCE], hdr[H_NREDUCE]);
    return launch_status("glass_spmm_gat_edge_f32");
}

template <int VW, int LPR, bool DX>
static int launch_gat_bwd(GatBwdOp<VW, LPR, DX> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan,
                          hipStream_t st) {
    const ItemsGrid gr = items_grid(op, hdr);
    if (gr.blocks > 0)  // (da alone: one column tile)
        hipLaunchKernelGGL((k1_items_kernel<GatBwdOp<VW, LPR, DX>>), dim3(gr.blocks, DX ? gr.n_ctiles : 1), dim3(kBlock), 0, st, op,
                           rowptr, plan + hdr[H_OFF_SWEEP], gr.n_waves, plan + hdr[H_OFF_LONG], gr.n_sweep_blocks);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_gat_bwd_reduce_kernel, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, op.ps, op.pda, op.db,
                           op.att_src, op.att_dst, op.dX, op.lddx, op.da, op.H, plan + hdr[H_OFF_REDUCE]);
    return launch_status(DX ? "glass_spmm_gat_bwd_f32" : "glass_spmm_gat_da_f32");
}

}  // namespace glass

using namespace glass;

extern "C" int glass_gat_scores_f32(const float* X, int64_t ldx, const float* att_src, const float* att_dst, float* a, float* b,
                                    int64_t n_rows, int64_t H, void* stream) {
    GLASS_REQUIRE(X && att_src && att_dst && a && b, "gat_scores: null pointer");
    GLASS_REQUIRE(aligned4(X) && aligned4(att_src) && aligned4(att_dst) && aligned4(a) && aligned4(b),
                  "gat_scores: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && n_rows >= 0 && n_rows < (1ll << 31), "gat_scores: need H>0, ldx>=H (H=%lld ldx=%lld n=%lld)",
                  (long long)H, (long long)ldx, (long long)n_rows);
    if (H > kMaxH) {
        set_error("gat_scores: H = %lld is beyond the %lld columns the aggregation covers", (long long)H, (long long)kMaxH);
        return GLASS_E_UNSUPPORTED;
    }
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(gat_scores_kernel, dim3((unsigned)ceil_div(n_rows, kScoreRows)), dim3(kBlock), 0, (hipStream_t)stream, X,
                       ldx, att_src, att_dst, a, b, n_rows, (int)H);
    return launch_status("glass_gat_scores_f32");
}

extern "C" int64_t glass_spmm_gat_ws_bytes(const int32_t* hdr, int64_t H) {
    if (!hdr || hdr[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr[H_NSLOTS] * (H + 2) * (int64_t)sizeof(float);
}

extern "C" int64_t glass_spmm_gat_edge_ws_bytes(const int32_t* hdr, int64_t H) {
    if (!hdr || hdr[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr[H_NSLOTS] * (int64_t)sizeof(float);
}

extern "C" int64_t glass_spmm_gat_bwd_ws_bytes(const int32_t* hdr_t, int64_t H) {
    if (!hdr_t || hdr_t[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr_t[H_NSLOTS] * (H + 1) * (int64_t)sizeof(float);
}

extern "C" int64_t glass_gat_datt_ws_bytes(int64_t n_rows, int64_t H) {
    if (H <= 0 || n_rows < 0) return GLASS_E_ARG;
    return ceil_div(n_rows, datt_rows_per_wg(H)) * 2 * H * (int64_t)sizeof(double);
}

extern "C" int glass_spmm_gat_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                      const float* a, const float* b, float slope, float* Y, int64_t ldy, float* L,
                                      int64_t n_rows, int64_t H, const int32_t* hdr, const int32_t* plan_dev, void* ws,
                                      void* stream) {
    GLASS_REQUIRE(rowptr && X && a && b && Y && L && hdr && plan_dev, "spmm_gat: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col) && aligned4(val) && aligned4(X) && aligned4(a) && aligned4(b) && aligned4(Y) &&
                  aligned4(L) && aligned4(plan_dev) && aligned4(ws), "spmm_gat: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && ldy >= H, "spmm_gat: need H>0, ldx>=H, ldy>=H (H=%lld ldx=%lld ldy=%lld)", (long long)H,
                  (long long)ldx, (long long)ldy);
    GLASS_REQUIRE(slope == slope, "spmm_gat: slope is NaN");
    if (const int rc = check_plan("spmm_gat", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val), "spmm_gat: null col/val");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_gat: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* ps = (float*)ws;
    float* pm = ps + (int64_t)hdr[H_NSLOTS] * H;
    float* pz = pm + hdr[H_NSLOTS];
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && aligned16(X) && aligned16(Y) &&
                     (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1A_FWD_CASE(VW, LPR)                                                                                          \
    return launch_gat_fwd(GatFwdOp<VW, LPR>{col, val, X, ldx, a, b, slope, Y, ldy, L, ps, pm, pz, (int)H}, rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1A_FWD_CASE);
#undef GLASS_K1A_FWD_CASE
}

extern "C" int glass_spmm_gat_edge_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                       const float* a, const float* b, float slope, const float* dY, int64_t lddy, const float* Y,
                                       int64_t ldy, const float* L, float* g, float* db, int64_t n_rows, int64_t H,
                                       const int32_t* hdr, const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && a && b && dY && Y && L && db && hdr && plan_dev, "spmm_gat_edge: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col) && aligned4(val) && aligned4(X) && aligned4(a) && aligned4(b) && aligned4(dY) &&
                  aligned4(Y) && aligned4(L) && aligned4(g) && aligned4(db) && aligned4(plan_dev) && aligned4(ws),
                  "spmm_gat_edge: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && lddy >= H && ldy >= H,
                  "spmm_gat_edge: need H>0 and every ld >= H (H=%lld ldx=%lld lddy=%lld ldy=%lld)", (long long)H, (long long)ldx,
                  (long long)lddy, (long long)ldy);
    GLASS_REQUIRE(slope == slope, "spmm_gat_edge: slope is NaN");
    if (const int rc = check_plan("spmm_gat_edge", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val && g), "spmm_gat_edge: null col/val/g");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_gat_edge: plan needs %d partial sums but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (lddy % 4 == 0) && (ldy % 4 == 0) && aligned16(X) && aligned16(dY) &&
                     aligned16(Y);
#define GLASS_K1A_EDGE_CASE(VW, LPR)                                                                                           \
    return launch_gat_edge(GatEdgeOp<VW, LPR>{col, val, X, ldx, a, b, slope, dY, lddy, Y, ldy, L, g, db, (float*)ws, (int)H}, \
                           rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1A_EDGE_CASE);
#undef GLASS_K1A_EDGE_CASE
}

extern "C" int glass_spmm_gat_bwd_f32(const int32_t* rowptr, const int32_t* col_t, const float* val_t, const int32_t* eid_t,
                                      const float* a, const float* b, float slope, const float* dY, int64_t lddy, const float* L,
                                      const float* g, const float* db, const float* att_src, const float* att_dst, float* dX,
                                      int64_t lddx, float* da, int64_t n_rows, int64_t H, const int32_t* hdr,
                                      const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && a && b && dY && L && db && att_src && att_dst && dX && da && hdr && plan_dev,
                  "spmm_gat_bwd: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col_t) && aligned4(val_t) && aligned4(eid_t) && aligned4(a) && aligned4(b) &&
                  aligned4(dY) && aligned4(L) && aligned4(g) && aligned4(db) && aligned4(att_src) && aligned4(att_dst) &&
                  aligned4(dX) && aligned4(da) && aligned4(plan_dev) && aligned4(ws), "spmm_gat_bwd: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && lddy >= H && lddx >= H, "spmm_gat_bwd: need H>0, lddy>=H, lddx>=H (H=%lld lddy=%lld lddx=%lld)",
                  (long long)H, (long long)lddy, (long long)lddx);
    GLASS_REQUIRE(slope == slope, "spmm_gat_bwd: slope is NaN");
    if (const int rc = check_plan("spmm_gat_bwd", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col_t && val_t && eid_t && g), "spmm_gat_bwd: null col_t/val_t/eid_t/g");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_gat_bwd: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* ps = (float*)ws;
    float* pda = ps + (int64_t)hdr[H_NSLOTS] * H;
    const bool vec = (H % 4 == 0) && (lddy % 4 == 0) && (lddx % 4 == 0) && aligned16(dY) && aligned16(dX) &&
                     (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1A_BWD_CASE(VW, LPR)                                                                                            \
    return launch_gat_bwd(GatBwdOp<VW, LPR, true>{col_t, val_t, eid_t, a, b, slope, dY, lddy, L, g, db, att_src, att_dst, dX, lddx, \
                                                  da, ps, pda, (int)H},                                                         \
                          rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1A_BWD_CASE);
#undef GLASS_K1A_BWD_CASE
}

extern "C" int64_t glass_spmm_gat_da_ws_bytes(const int32_t* hdr_t, int64_t H) {
    if (!hdr_t || hdr_t[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr_t[H_NSLOTS] * (int64_t)sizeof(float);
}

extern "C" int glass_spmm_gat_da_f32(const int32_t* rowptr, const int32_t* col_t, const float* val_t, const int32_t* eid_t,
                                     const float* g, float* da, int64_t n_rows, int64_t H, int vec_form, const int32_t* hdr,
                                     const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && da && hdr && plan_dev, "spmm_gat_da: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col_t) && aligned4(val_t) && aligned4(eid_t) && aligned4(g) && aligned4(da) &&
                  aligned4(plan_dev) && aligned4(ws), "spmm_gat_da: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && (!vec_form || H % 4 == 0), "spmm_gat_da: need H>0, and H a multiple of 4 in the 16-byte form (H=%lld)",
                  (long long)H);
    if (const int rc = check_plan("spmm_gat_da", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col_t && val_t && eid_t && g), "spmm_gat_da: null col_t/val_t/eid_t/g");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_gat_da: plan needs %d partial sums but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = vec_form != 0;
#define GLASS_K1A_DA_CASE(VW, LPR)                                                                                             \
    return launch_gat_bwd(GatBwdOp<VW, LPR, false>{col_t, val_t, eid_t, nullptr, nullptr, 0.f, nullptr, 0, nullptr, g, nullptr, \
                                                   nullptr, nullptr, nullptr, 0, da, nullptr, (float*)ws, (int)H},             \
                          rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1A_DA_CASE);
#undef GLASS_K1A_DA_CASE
}

extern "C" int glass_gat_datt_f32(const float* X, int64_t ldx, const float* da, const float* db, float* datt_src, float* datt_dst,
                                  int64_t n_rows, int64_t H, void* ws, void* stream) {
    GLASS_REQUIRE(X && da && db && datt_src && datt_dst, "gat_datt: null pointer");
    GLASS_REQUIRE(aligned4(X) && aligned4(da) && aligned4(db) && aligned4(datt_src) && aligned4(datt_dst),
                  "gat_datt: pointer not 4-byte aligned");
    GLASS_REQUIRE(aligned8(ws), "gat_datt: ws not 8-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && n_rows >= 0 && n_rows < (1ll << 31), "gat_datt: need H>0, ldx>=H (H=%lld ldx=%lld n=%lld)",
                  (long long)H, (long long)ldx, (long long)n_rows);
    if (H > kMaxH) {
        set_error("gat_datt: H = %lld is beyond the %lld columns the aggregation covers", (long long)H, (long long)kMaxH);
        return GLASS_E_UNSUPPORTED;
    }
    GLASS_REQUIRE(n_rows == 0 || ws, "gat_datt: ws is null");
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t rpw = datt_rows_per_wg(H), n_wg = ceil_div(n_rows, rpw);
    const int hc = pow2_ceil_cap(H, kBlock);
    hipLaunchKernelGGL(gat_datt_partial_kernel, dim3((unsigned)n_wg), dim3(kBlock), 0, st, X, ldx, da, db, n_rows, (int)H, hc, rpw,
                       (double*)ws);
    hipLaunchKernelGGL(gat_datt_final_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)ws, n_wg, (int)H, datt_src, datt_dst);
    return launch_status("glass_gat_datt_f32");
}
