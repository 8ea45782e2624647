// K1w: the gradient of a product Y = A(w) X with respect to the edge weights w, for the aggregations whose adjacency values are
// a function of w alone ("sum", "mean", "gcn": K2, elementwise.hip), on K1's CSR, plans and lane layout.  With d~_i the
// row sum of w (+ 1 where it is below 0.5: K2's rule, derivative 1) and r = d~^(-1/2), for entry e of row i with column j:
//
//   dval[e] = sum_c dY[i,c] X[j,c]                  R[i] = sum over the entries of row i of dval[e] val[e]
//   C[k]    = sum over the entries with column k of dval[e] val[e]                                  ("gcn" only)
//   sum:  dw = dval[e]        mean:  dw = (dval[e] - R[i]) / d~_i        gcn:  dw = r_i r_j dval[e] - (R[i] + C[i]) / (2 d~_i)
//
// Three passes.  The first (DvalOp) is the plain form of K1a's edge pass (spmm_gat.hip): an operation of the item walk of
// spmm_items.h with one column tile, the lane group of an entry forming the whole dot over the column passes — at H = 64 in
// the 16-byte form 16 lanes x one float4 per entry, four entries per wave step.  It moves 12 + 4 H bytes per entry (col, val,
// dval, one row of X).  The second (ColsumOp) walks the transposed plan without reading a row, one entry per lane, dval through
// eid_t.  The third is K2's own walk (one wave per row) and writes dw in the CALLER's edge order through the build
// permutation.  Lane groups (__shfl_xor), the four waves of a long-row item (LDS) and the chunks of a cut row (workspace
// partials, a small second launch, slot order) combine in a fixed order: no float atomics, every entry bitwise repeatable
// for a given plan.
#include "spmm_gat_common.h"

namespace glass {

constexpr int kDvalGathers = kGatEdgeGathers;  // U of the first pass: one row per entry, the row's dY beside it

// ---- first pass: dval[e] for every entry of the forward CSR, R[i] for every row ------------------------------------------------
// One column tile (gridDim.y = 1): lane `sub` of a group owns columns (p * LPR + sub) * VW ... of every column pass p.  The row's
// dY of pass 0 stays in registers; further passes (H beyond LPR * VW columns: LPR = 64 then, one group per wave) re-read it.
template <int VW_, int LPR_>
struct DvalOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kDvalGathers;
    using Acc = SumAcc<1>;  // R's partial sum, on the lanes with sub == 0
    struct Slot {
        float x[VW];  // the source's row, pass 0
        int c;        // the source, for the further passes
    };
    const int32_t* col;
    const float* val;
    const float* X;
    int64_t ldx;
    const float* dY;
    int64_t lddy;
    float* dval;      // [nnz]
    float* R;         // [N]
    float* partials;  // [n_slots] R of the chunks of cut rows
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
        const int coff = ln.coff;
        float gi[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) gi[k] = 0.f;
        if (ln.col_ok) load_row<VW>(gi, dYr + coff);
        const float* Xc = X + coff;
        const bool lead = ln.sub == 0;  // column 0: always a live column, so `ok` is "the entry exists" there
        entry_batches<LPR, U, Slot>(
            col, val, nullptr, e0, e1, ln,
            [&](Slot& s, int c, bool ok) {
                load_row_if<VW>(ok, s.x, Xc + (int64_t)c * ldx);
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
                if (ok && lead) {
                    dval[e] = q;
                    acc.s[0] = fmaf(q, v, acc.s[0]);
                }
            });
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        if (coff != 0) return;
        if (slot < 0) R[row] = acc.s[0];
        else partials[slot] = acc.s[0];
    }
};

// ---- second pass: row k of A^T, one entry per lane, no row read ------------------------------------------------------------------
struct ColsumOp {
    static constexpr int VW = 1, LPR = 1, U = 1;  // 64 lane groups of one lane: a batch of 64 entries is one step
    using Acc = SumAcc<1>;
    struct Slot {
        float g;  // this entry's dval
    };
    const int32_t* col;   // the transposed CSR (the columns themselves are not used)
    const float* val;
    const int32_t* eid;   // index of each transposed entry in the forward CSR
    const float* dval;
    float* C;             // [N]
    float* partials;      // [n_slots]
    int H;                // 1: the walk's only column

    __device__ __forceinline__ void gather(Acc& acc, int, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        entry_batches<LPR, U, Slot>(
            col, val, eid, e0, e1, ln, [&](Slot& s, int, bool ok, int32_t e) { s.g = ok ? dval[e] : 0.f; },
            [&](const Slot& s, float v, bool ok, int) { acc.s[0] = ok ? fmaf(s.g, v, acc.s[0]) : acc.s[0]; });
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int) const {
        if (slot < 0) C[row] = acc.s[0];
        else partials[slot] = acc.s[0];
    }
};

// R or C of the rows cut into several chunks, in slot order: one thread per row
__global__ __launch_bounds__(kBlock) void edge_slots_reduce_kernel(const float* __restrict__ partials, float* __restrict__ out,
                                                                   const int32_t* __restrict__ rrows, int n_reduce) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_reduce) return;
    const int32_t* rr = rrows + 3 * (int64_t)i;
    const int row = rr[0], first = rr[1], n = rr[2];
    float s = 0.f;
    for (int k = 0; k < n; ++k) s += partials[first + k];
    out[row] = s;
}

// the item walk with ONE column tile, then the cut rows
template <class Op>
static int launch_edge_items(const Op& op, float* out, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan,
                             hipStream_t st, const char* what) {
    const ItemsGrid gr = items_grid(op, hdr);
    if (gr.blocks > 0)
        hipLaunchKernelGGL((k1_items_kernel<Op>), dim3(gr.blocks, 1), dim3(kBlock), 0, st, op, rowptr, plan + hdr[H_OFF_SWEEP],
                           gr.n_waves, plan + hdr[H_OFF_LONG], gr.n_sweep_blocks);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(edge_slots_reduce_kernel, dim3((unsigned)ceil_div(hdr[H_NREDUCE], kBlock)), dim3(kBlock), 0, st,
                           op.partials, out, plan + hdr[H_OFF_REDUCE], hdr[H_NREDUCE]);
    return launch_status(what);
}

// ---- third pass: K2's walk (one wave per row, lanes stride the row's entries), dw scattered to the caller's edge order ---------
__global__ __launch_bounds__(kBlock) void adj_values_bwd_kernel(const int32_t* __restrict__ rowptr,
                                                                const int32_t* __restrict__ col,
                                                                const int32_t* __restrict__ perm,
                                                                const float* __restrict__ deg, const float* __restrict__ dval,
                                                                const float* __restrict__ R, const float* __restrict__ C,
                                                                int n_rows, int64_t nnz, int aggr, float* __restrict__ dw) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const int e0 = rowptr[row], e1 = rowptr[row + 1];
    if (e0 >= e1) return;
    float d = 1.f, ri = 1.f, shift = 0.f;
    if (aggr != 1) d = deg[row];
    if (aggr == 0) shift = R[row];
    if (aggr == 2) {
        ri = 1.0f / sqrtf(d);  // K2's own r_i
        shift = (R[row] + C[row]) / (2.0f * d);
    }
    for (int e = e0 + lane; e < e1; e += kWave) {
        float g = dval[e];
        if (aggr == 0) g = (g - shift) / d;
        else if (aggr == 2) g = ri * (1.0f / sqrtf(deg[col[e]])) * g - shift;
        const int64_t p = perm[e];
        if (p >= 0 && p < nnz) dw[p] = g;  // (a permutation of [0, nnz) by contract; anything else is dropped, not written)
    }
}

int adj_values_bwd_launch(const int32_t* rowptr, const int32_t* col, const int32_t* perm, const float* deg, const float* dval,
                          const float* R, const float* C, int64_t n_rows, int64_t nnz, int aggr, float* dw, void* stream) {
    const unsigned grid = (unsigned)ceil_div(n_rows, kBlock / kWave);
    hipLaunchKernelGGL(adj_values_bwd_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream, rowptr, col, perm, deg, dval, R, C,
                       (int)n_rows, nnz, aggr, dw);
    return launch_status("glass_adj_values_bwd_f32");
}

}  // namespace glass

using namespace glass;

extern "C" int64_t glass_spmm_dval_ws_bytes(const int32_t* hdr, int64_t H) {
    if (!hdr || hdr[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0) return GLASS_E_ARG;
    return (int64_t)hdr[H_NSLOTS] * (int64_t)sizeof(float);
}

extern "C" int64_t glass_adj_colsum_ws_bytes(const int32_t* hdr_t) {
    if (!hdr_t || hdr_t[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    return (int64_t)hdr_t[H_NSLOTS] * (int64_t)sizeof(float);
}

extern "C" int glass_spmm_dval_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                   const float* dY, int64_t lddy, float* dval, float* R, int64_t n_rows, int64_t H,
                                   const int32_t* hdr, const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && dY && R && hdr && plan_dev, "spmm_dval: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col) && aligned4(val) && aligned4(X) && aligned4(dY) && aligned4(dval) &&
                  aligned4(R) && aligned4(plan_dev) && aligned4(ws), "spmm_dval: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && ldx >= H && lddy >= H, "spmm_dval: need H>0, ldx>=H, lddy>=H (H=%lld ldx=%lld lddy=%lld)", (long long)H,
                  (long long)ldx, (long long)lddy);
    if (const int rc = check_plan("spmm_dval", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val && dval), "spmm_dval: null col/val/dval");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_dval: plan needs %d partial sums but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (lddy % 4 == 0) && aligned16(X) && aligned16(dY);
#define GLASS_K1W_DVAL_CASE(VW, LPR)                                                                                          \
    return launch_edge_items(DvalOp<VW, LPR>{col, val, X, ldx, dY, lddy, dval, R, (float*)ws, (int)H}, R, rowptr, hdr, plan_dev, \
                             st, "glass_spmm_dval_f32")
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1W_DVAL_CASE);
#undef GLASS_K1W_DVAL_CASE
}

extern "C" int glass_adj_colsum_f32(const int32_t* rowptr_t, const int32_t* col_t, const float* val_t, const int32_t* eid_t,
                                    const float* dval, float* C, int64_t n_rows, const int32_t* hdr_t, const int32_t* plan_dev,
                                    void* ws, void* stream) {
    GLASS_REQUIRE(rowptr_t && C && hdr_t && plan_dev, "adj_colsum: null pointer");
    GLASS_REQUIRE(aligned4(rowptr_t) && aligned4(col_t) && aligned4(val_t) && aligned4(eid_t) && aligned4(dval) && aligned4(C) &&
                  aligned4(plan_dev) && aligned4(ws), "adj_colsum: pointer not 4-byte aligned");
    if (const int rc = check_plan("adj_colsum", hdr_t, n_rows, 1)) return rc;
    GLASS_REQUIRE(hdr_t[H_NNZ] == 0 || (col_t && val_t && eid_t && dval), "adj_colsum: null col_t/val_t/eid_t/dval");
    GLASS_REQUIRE(hdr_t[H_NSLOTS] == 0 || ws, "adj_colsum: plan needs %d partial sums but ws is null", hdr_t[H_NSLOTS]);
    if (n_rows == 0) return 0;
    return launch_edge_items(ColsumOp{col_t, val_t, eid_t, dval, C, (float*)ws, 1}, C, rowptr_t, hdr_t, plan_dev,
                             (hipStream_t)stream, "glass_adj_colsum_f32");
}
