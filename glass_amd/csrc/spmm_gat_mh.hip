// K1a, multi-head: attention neighbour aggregation with K heads that partition the H channels (head h owns columns
// [h D, (h + 1) D), D = H / K: the transformer convention).  The operator is block-diagonal: head h's columns of every result
// are what the single-head operator (spmm_gat.hip) gives on X[:, h D : (h + 1) D] with the matching slices of att_src / att_dst.
// Per destination i, entry e of row i (source j = col[e], weight v_e > 0), head h and c a column of head h:
//
//   a[j,h] = sum_{c in h} X[j,c] att_src[c]     b[i,h] = sum_{c in h} X[i,c] att_dst[c]     (fp64 sums, fixed order, rounded once)
//   u = a[j,h] + b[i,h]                         s_eh = u > 0 ? u : slope * u                (gat_score: the same bits in every pass)
//   M_ih = max_e s_eh     Z_ih = sum_e v_e exp(s_eh - M_ih)     Y[i,c] = sum_e v_e exp(s_eh - M_ih) X[j,c] / Z_ih
//   L[i,h] = M_ih + log Z_ih;   a row without entries: Y = 0, L = 0
//
//   backward, p_eh = v_e exp(s_eh - L[i,h]), f_eh = u > 0 ? 1 : slope (u == 0 takes slope):
//   D_ih = sum_{c in h} dY[i,c] Y[i,c]          q_eh = sum_{c in h} dY[i,c] X[j,c]          g[e,h] = p_eh (q_eh - D_ih) f_eh
//   da[j,h] = sum over the entries with col = j of g[e,h]                  db[i,h] = sum over the entries of row i of g[e,h]
//   dX[j,c] = sum over the entries with col = j of p_eh dY[i,c]  +  da[j,h] att_src[c]  +  db[j,h] att_dst[c]
//   d att_src[c] = sum_j da[j,h(c)] X[j,c]      d att_dst[c] = sum_i db[i,h(c)] X[i,c]
//
// a, b, L, da, db are [N, K] row-major, g is [nnz, K] in forward entry order; nothing of size [nnz, H] exists.
//
// The lane layout is the single-head kernels': the item walk of spmm_items.h gives a lane VW contiguous columns of a row, and
// D is a power of two that VW divides, so a head is a contiguous, aligned run of D / VW lanes.  The per-lane state of the
// forward, (M, Z), and of the transposed pass, da, is that of the lane's head; the lane groups of a wave, its four waves and
// the chunks of a cut row combine lane for lane, hence head for head, in the single-head kernels' fixed order.  The edge pass
// forms one dot per head with a butterfly that stays inside the head's lanes (the xor steps below D / VW); where a head is
// wider than the wave's columns (D = 128, 256 in the scalar form) a workgroup's column tile is the head, and the lane adds its
// D / 64 column passes before the wave sum.  No float atomics; every entry is bitwise repeatable for a given plan; the vectors
// and every temporary are read from device memory when the kernels run; slope and K are passed by value.
#include "spmm_gat_common.h"

namespace glass {

constexpr int kMhMinD = 4, kMhMaxD = 256;

// how the heads lie in the columns: D = 1 << dshift columns per head
struct HeadMap {
    int K, dshift;
    __host__ __device__ __forceinline__ int D() const { return 1 << dshift; }
    __device__ __forceinline__ int head(int c) const { return c >> dshift; }
    __device__ __forceinline__ bool first(int c) const { return (c & ((1 << dshift) - 1)) == 0; }  // the head's first column
    __device__ __forceinline__ int64_t at(int64_t r, int h) const { return r * K + h; }            // of an [., K] array
};

// ---- node scores: a, b [N, K] ---------------------------------------------------------------------------------------------
// one wave per row, in rounds of max(D, 64) columns: lane l sums columns l, l + 64, ... of the round in fp64, then the lanes of a
// head in a butterfly (the xor steps below min(D, 64)): a fixed order
__global__ __launch_bounds__(kBlock) void gat_scores_mh_kernel(const float* __restrict__ X, int64_t ldx,
                                                               const float* __restrict__ att_src,
                                                               const float* __restrict__ att_dst, float* __restrict__ a,
                                                               float* __restrict__ b, int64_t n_rows, int H, HeadMap hm) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t row = (int64_t)blockIdx.x * kScoreRows + (threadIdx.x >> 6);
    if (row >= n_rows) return;  // (whole waves)
    const float* x = X + row * ldx;
    const int D = hm.D(), seg = D < kWave ? D : kWave, round = D > kWave ? D : kWave;
    for (int c0 = 0; c0 < H; c0 += round) {  // (wave-uniform)
        const int c1 = c0 + round < H ? c0 + round : H;
        double sa = 0.0, sb = 0.0;
        for (int c = c0 + lane; c < c1; c += kWave) {
            const double xv = (double)x[c];
            sa = fma(xv, (double)att_src[c], sa);
            sb = fma(xv, (double)att_dst[c], sb);
        }
#pragma unroll
        for (int s = 1; s < kWave; s <<= 1)
            if (s < seg) {  // (uniform)
                sa += __shfl_xor(sa, s);
                sb += __shfl_xor(sb, s);
            }
        const int c = c0 + lane;
        if ((lane & (seg - 1)) == 0 && c < H) {
            a[hm.at(row, hm.head(c))] = (float)sa;
            b[hm.at(row, hm.head(c))] = (float)sb;
        }
    }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// GatFwdOp with the score, the pair (M, Z) and L of the lane's head
template <int VW_, int LPR_>
struct GatMhFwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kGatFwdGathers;
    using Acc = GatAcc<VW>;
    struct Slot {
        float x[VW];  // the source's message row
        float a;      // and its score for this lane's head
    };
    const int32_t* col;
    const float* val;
    const float* X;
    int64_t ldx;
    const float* a;  // [N, K]
    const float* b;
    float slope;
    float* Y;
    int64_t ldy;
    float* L;    // [N, K]
    float* ps;   // partials of the chunks of cut rows: [n_slots, H] sums, then [n_slots, K] M, then [n_slots, K] Z
    float* pm;
    float* pz;
    int H;
    HeadMap hm;

    __device__ __forceinline__ void gather(Acc& acc, int row, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        const float* Xc = X + ln.coff;
        const int h = hm.head(ln.coff);  // (a lane past the last column names no head: it reads nothing)
        const float bi = ln.col_ok ? b[hm.at(row, h)] : 0.f;
        entry_batches<LPR, U, Slot>(
            col, val, nullptr, e0, e1, ln,
            [&](Slot& s, int c, bool ok) {
                load_row_if<VW>(ok, s.x, Xc + (int64_t)c * ldx);
                s.a = ok ? a[hm.at(c, h)] : 0.f;
            },
            [&](const Slot& s, float v, bool ok, int) { acc.take(ok, v, gat_score(s.a, bi, slope), s.x); });
    }
    // (the first lane of a head also writes the head's scalar)
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        const int h = hm.head(coff);
        if (slot < 0) {
            const bool any = acc.z > 0.f;
            float y[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) y[k] = any ? acc.s[k] / acc.z : 0.f;
            vec_from<VW>(y).store(Y + (int64_t)row * ldy + coff);
            if (hm.first(coff)) L[hm.at(row, h)] = any ? acc.m + logf(acc.z) : 0.f;
        } else {
            vec_from<VW>(acc.s).store(ps + (int64_t)slot * H + coff);
            if (hm.first(coff)) {
                pm[hm.at(slot, h)] = acc.m;
                pz[hm.at(slot, h)] = acc.z;
            }
        }
    }
};

// rows cut into several chunks: their partials merged slot by slot, each column with the pairs of its head
__global__ __launch_bounds__(kBlock) void spmm_gat_mh_reduce_kernel(const float* __restrict__ ps, const float* __restrict__ pm,
                                                                    const float* __restrict__ pz, float* __restrict__ Y,
                                                                    int64_t ldy, float* __restrict__ L, int H, HeadMap hm,
                                                                    const int32_t* __restrict__ rrows) {
    const int32_t* rr = rrows + 3 * (int64_t)blockIdx.x;
    const int row = rr[0], first = rr[1], n = rr[2];
    for (int c = threadIdx.x; c < H; c += kBlock) {
        const int h = hm.head(c);
        GatAcc<1> p;
        p.init();
        for (int k = 0; k < n; ++k) {
            const float os[1] = {ps[(int64_t)(first + k) * H + c]};
            p.merge(pm[hm.at(first + k, h)], pz[hm.at(first + k, h)], os);
        }
        const bool any = p.z > 0.f;
        Y[(int64_t)row * ldy + c] = any ? p.s[0] / p.z : 0.f;
        if (hm.first(c)) L[hm.at(row, h)] = any ? p.m + logf(p.z) : 0.f;
    }
}

// ---- edge pass: g[e, h] for every entry of the forward CSR and head, db[i, h] for every row and head ---------------------------
// The grid's column tiles are whole heads: a tile is the LPR * VW columns of the lane layout, or one head where a head is wider
// (pp = D / (LPR * VW) column passes: D = 128, 256 at VW = 1, LPR = 64).  A lane's columns lie in one head; its first pass of dY
// stays in registers, further passes are re-read.
template <int VW_, int LPR_>
struct GatMhEdgeOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kGatEdgeGathers;
    static constexpr int kPass = LPR * VW;
    using Acc = SumAcc<1>;  // db's partial sum, on the first lane of each head
    struct Slot {
        float x[VW];  // the source's message row, pass 0
        float a;      // its score for this lane's head
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
    float* g;         // [nnz, K]
    float* db;        // [N, K]
    float* partials;  // [n_slots, K] db of the chunks of cut rows
    int H;
    HeadMap hm;
    int pp;           // column passes per tile

    // first column of the lane whose item_lanes column is coff (the same where pp == 1)
    __device__ __forceinline__ int base_of(int coff) const { return coff + (int)blockIdx.y * (pp - 1) * kPass; }
    // the sum over the lanes of a head within the group
    __device__ __forceinline__ float head_sum(float q) const {
        const int seg = min(hm.D() / VW, LPR);
#pragma unroll
        for (int s = 1; s < LPR; s <<= 1)
            if (s < seg) q += __shfl_xor(q, s);  // (uniform)
        return q;
    }
    static __device__ __forceinline__ float dot(const float (&p)[VW], const float (&r)[VW], float q) {
#pragma unroll
        for (int k = 0; k < VW; ++k) q = fmaf(p[k], r[k], q);
        return q;
    }

    __device__ __forceinline__ void gather(Acc& acc, int row, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        const float* dYr = dY + (int64_t)row * lddy;
        const float* Yr = Y + (int64_t)row * ldy;
        const int base = base_of(ln.coff);
        const bool live = base < H;  // then every pass of the lane is: H is whole heads
        const int h = hm.head(base);
        float gi[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) gi[k] = 0.f;
        if (live) load_row<VW>(gi, dYr + base);
        float d = 0.f;
        for (int p = 0; p < pp; ++p) {  // (wave-uniform)
            float gy[VW], yy[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) gy[k] = yy[k] = 0.f;
            if (live) {
                load_row<VW>(gy, dYr + base + p * kPass);
                load_row<VW>(yy, Yr + base + p * kPass);
            }
            d = dot(gy, yy, d);
        }
        const float Di = head_sum(d);
        const float Li = live ? L[hm.at(row, h)] : 0.f, bi = live ? b[hm.at(row, h)] : 0.f;
        const float* Xc = X + base;
        const bool lead = live && hm.first(base);
        entry_batches<LPR, U, Slot>(
            col, val, nullptr, e0, e1, ln,
            [&](Slot& s, int c, bool ok) {
                load_row_if<VW>(ok && live, s.x, Xc + (int64_t)c * ldx);
                s.a = (ok && live) ? a[hm.at(c, h)] : 0.f;
                s.c = c;
            },
            [&](const Slot& s, float v, bool ok, int e) {
                float q = dot(gi, s.x, 0.f);
                for (int p = 1; p < pp; ++p) {  // (a head wider than the wave's columns: its passes before the group sum)
                    float gy[VW], xx[VW];
#pragma unroll
                    for (int k = 0; k < VW; ++k) gy[k] = xx[k] = 0.f;
                    if (ok && live) {
                        load_row<VW>(gy, dYr + base + p * kPass);
                        load_row<VW>(xx, Xc + (int64_t)s.c * ldx + p * kPass);
                    }
                    q = dot(gy, xx, q);
                }
                q = head_sum(q);
                const float pe = v * expf(gat_score(s.a, bi, slope) - Li);
                const float ge = pe * (q - Di) * gat_slope_of(s.a, bi, slope);
                if (ok && lead) {
                    g[hm.at(e, h)] = ge;
                    acc.s[0] += ge;
                }
            });
    }
    __device__ __forceinline__ void store(const Acc& acc, int row, int slot, int coff) const {
        const int base = base_of(coff);
        if (base >= H || !hm.first(base)) return;
        const int h = hm.head(base);
        if (slot < 0) db[hm.at(row, h)] = acc.s[0];
        else partials[hm.at(slot, h)] = acc.s[0];
    }
};

// db of the rows cut into several chunks, in slot order: one thread per row and head
__global__ __launch_bounds__(kBlock) void spmm_gat_mh_edge_reduce_kernel(const float* __restrict__ partials,
                                                                         float* __restrict__ db,
                                                                         const int32_t* __restrict__ rrows, int n_reduce, int K) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)n_reduce * K) return;
    const int32_t* rr = rrows + 3 * (i / K);
    const int h = (int)(i % K);
    const int row = rr[0], first = rr[1], n = rr[2];
    float s = 0.f;
    for (int k = 0; k < n; ++k) s += partials[(int64_t)(first + k) * K + h];
    db[(int64_t)row * K + h] = s;
}

// ---- transposed pass: GatBwdOp with a, b, L, g, db and da of the lane's head -------------------------------------------------
// DX = false is the same walk for da alone (glass_spmm_gat_mh_da_f32) over the same column tiles: no dY row, no exponential, and
// entry for entry the additions of the full pass at this lane layout, so da has the same bits either way.
template <int VW_, int LPR_, bool DX>
struct GatMhBwdOp {
    static constexpr int VW = VW_, LPR = LPR_, U = kGatBwdGathers;
    using Acc = GatBwdAcc<VW>;
    struct Slot {
        float dy[VW];    // the destination's dY row
        float b, l, g;   // its b and L, this entry's g, of this lane's head
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
    float* da;            // [N, K]
    float* ps;            // partials of the chunks of cut rows: [n_slots, H] sums, then [n_slots, K] da
    float* pda;
    int H;
    HeadMap hm;

    __device__ __forceinline__ void gather(Acc& acc, int row, int e0, int e1, const ItemLanes& ln) const {
        if (e0 >= e1) return;  // (wave-uniform)
        const int h = hm.head(ln.coff);
        if constexpr (!DX) {
            entry_batches<LPR, U, Slot>(
                col, val, eid, e0, e1, ln, [&](Slot& s, int, bool ok, int32_t e) { s.g = ok ? g[hm.at(e, h)] : 0.f; },
                [&](const Slot& s, float, bool, int) { acc.da += s.g; });
            return;
        }
        const float aj = ln.col_ok ? a[hm.at(row, h)] : 0.f;
        const float* dYc = dY + ln.coff;
        entry_batches<LPR, U, Slot>(
            col, val, eid, e0, e1, ln,
            [&](Slot& s, int c, bool ok, int32_t e) {
                load_row_if<VW>(ok, s.dy, dYc + (int64_t)c * lddy);
                s.b = ok ? b[hm.at(c, h)] : 0.f;
                s.l = ok ? L[hm.at(c, h)] : 0.f;
                s.g = ok ? g[hm.at(e, h)] : 0.f;
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
        const int h = hm.head(coff);
        if constexpr (!DX) {
            if (hm.first(coff)) (slot < 0 ? da[hm.at(row, h)] : pda[hm.at(slot, h)]) = acc.da;
            return;
        }
        if (slot < 0) {
            const float dbj = db[hm.at(row, h)];
            float r[VW];
#pragma unroll
            for (int k = 0; k < VW; ++k) r[k] = fmaf(dbj, att_dst[coff + k], fmaf(acc.da, att_src[coff + k], acc.s[k]));
            vec_from<VW>(r).store(dX + (int64_t)row * lddx + coff);
            if (hm.first(coff)) da[hm.at(row, h)] = acc.da;
        } else {
            vec_from<VW>(acc.s).store(ps + (int64_t)slot * H + coff);
            if (hm.first(coff)) pda[hm.at(slot, h)] = acc.da;
        }
    }
};

// every column sums the chunks of its head's da in slot order (the same bits on every column of a head)
__global__ __launch_bounds__(kBlock) void spmm_gat_mh_bwd_reduce_kernel(const float* __restrict__ ps, const float* __restrict__ pda,
                                                                        const float* __restrict__ db,
                                                                        const float* __restrict__ att_src,
                                                                        const float* __restrict__ att_dst, float* __restrict__ dX,
                                                                        int64_t lddx, float* __restrict__ da, int H, HeadMap hm,
                                                                        const int32_t* __restrict__ rrows) {
    const int32_t* rr = rrows + 3 * (int64_t)blockIdx.x;
    const int row = rr[0], first = rr[1], n = rr[2];
    for (int c = threadIdx.x; c < H; c += kBlock) {
        const int h = hm.head(c);
        float daj = 0.f;
        for (int k = 0; k < n; ++k) daj += pda[hm.at(first + k, h)];
        if (hm.first(c)) da[hm.at(row, h)] = daj;
        if (!dX) continue;  // (the da-only form; uniform)
        const float dbj = db[hm.at(row, h)];
        float s = 0.f;
        for (int k = 0; k < n; ++k) s += ps[(int64_t)(first + k) * H + c];
        dX[(int64_t)row * lddx + c] = fmaf(dbj, att_dst[c], fmaf(daj, att_src[c], s));
    }
}

// ---- the attention vectors' gradients: gat_datt_partial_kernel with da, db of the column's head -------------------------------
__global__ __launch_bounds__(kBlock) void gat_datt_mh_partial_kernel(const float* __restrict__ X, int64_t ldx,
                                                                     const float* __restrict__ da, const float* __restrict__ db,
                                                                     int64_t n_rows, int H, HeadMap hm, int hc, int64_t rpw,
                                                                     double* __restrict__ part) {
    __shared__ double lds[2][kBlock];
    const int t = threadIdx.x;
    const int nrs = kBlock / hc, c0 = t % hc, rs = t / hc;
    const int64_t r0 = (int64_t)blockIdx.x * rpw, r1 = r0 + rpw < n_rows ? r0 + rpw : n_rows;
    for (int cb = 0; cb < H; cb += hc) {  // (one round unless H > 256, where nrs = 1)
        const int c = cb + c0;
        double sa = 0.0, sb = 0.0;
        if (c < H) {
            const int h = hm.head(c);
            for (int64_t r = r0 + rs; r < r1; r += nrs) {
                const double x = (double)X[r * ldx + c];
                sa = fma((double)da[hm.at(r, h)], x, sa);
                sb = fma((double)db[hm.at(r, h)], x, sb);
            }
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
__global__ __launch_bounds__(kBlock) void gat_datt_mh_final_kernel(const double* __restrict__ part, int64_t n_wg, int H,
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

inline int64_t datt_mh_rows_per_wg(int64_t H) { return H > 128 ? 2 * H : 256; }  // as the single-head reductions

// ---- launches -----------------------------------------------------------------------------------------------------------------
template <int VW, int LPR>
static int launch_gat_mh_fwd(GatMhFwdOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan,
                             hipStream_t st) {
    launch_items(op, rowptr, hdr, plan, st);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_gat_mh_reduce_kernel, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, op.ps, op.pm, op.pz,
                           op.Y, op.ldy, op.L, op.H, op.hm, plan + hdr[H_OFF_REDUCE]);
    return launch_status("glass_spmm_gat_mh_csr_f32");
}

// the item walk over column tiles of whole heads
template <int VW, int LPR>
static int launch_gat_mh_edge(GatMhEdgeOp<VW, LPR> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan,
                              hipStream_t st) {
    const int D = op.hm.D();
    op.pp = D > LPR * VW ? D / (LPR * VW) : 1;
    const ItemsGrid gr = items_grid(op, hdr);
    const unsigned tiles = (unsigned)ceil_div(op.H, (int64_t)op.pp * LPR * VW);
    if (gr.blocks > 0)
        hipLaunchKernelGGL((k1_items_kernel<GatMhEdgeOp<VW, LPR>>), dim3(gr.blocks, tiles), dim3(kBlock), 0, st, op, rowptr,
                           plan + hdr[H_OFF_SWEEP], gr.n_waves, plan + hdr[H_OFF_LONG], gr.n_sweep_blocks);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_gat_mh_edge_reduce_kernel,
                           dim3((unsigned)ceil_div((int64_t)hdr[H_NREDUCE] * op.hm.K, kBlock)), dim3(kBlock), 0, st, op.partials,
                           op.db, plan + hdr[H_OFF_REDUCE], hdr[H_NREDUCE], op.hm.K);
    return launch_status("glass_spmm_gat_mh_edge_f32");
}

template <int VW, int LPR, bool DX>
static int launch_gat_mh_bwd(GatMhBwdOp<VW, LPR, DX> op, const int32_t* rowptr, const int32_t* hdr, const int32_t* plan,
                             hipStream_t st) {
    launch_items(op, rowptr, hdr, plan, st);
    if (hdr[H_NREDUCE] > 0)
        hipLaunchKernelGGL(spmm_gat_mh_bwd_reduce_kernel, dim3((unsigned)hdr[H_NREDUCE]), dim3(kBlock), 0, st, op.ps, op.pda,
                           op.db, op.att_src, op.att_dst, op.dX, op.lddx, op.da, op.H, op.hm, plan + hdr[H_OFF_REDUCE]);
    return launch_status(DX ? "glass_spmm_gat_mh_bwd_f32" : "glass_spmm_gat_mh_da_f32");
}

// K heads over H columns: 0 and the head map, or the code to return
static int head_map(const char* what, int64_t H, int64_t K, HeadMap* hm) {
    const int64_t D = H / K;
    if (H % K != 0 || D < kMhMinD || D > kMhMaxD || (D & (D - 1)) != 0) {
        set_error("%s: H = %lld, K = %lld, D = H / K = %lld%s: K must divide H and D be a power of two in [%d, %d]", what,
                  (long long)H, (long long)K, (long long)D, H % K != 0 ? " (not whole)" : "", kMhMinD, kMhMaxD);
        return GLASS_E_UNSUPPORTED;
    }
    hm->K = (int)K;
    hm->dshift = 0;
    while ((1ll << hm->dshift) < D) ++hm->dshift;
    return 0;
}

}  // namespace glass

using namespace glass;

// (K == 1 is the single-head operator with [N, 1] temporaries: its entries serve it, at any H they take)

extern "C" int glass_gat_scores_mh_f32(const float* X, int64_t ldx, const float* att_src, const float* att_dst, float* a, float* b,
                                       int64_t n_rows, int64_t H, int64_t K, void* stream) {
    GLASS_REQUIRE(X && att_src && att_dst && a && b, "gat_scores_mh: null pointer");
    GLASS_REQUIRE(aligned4(X) && aligned4(att_src) && aligned4(att_dst) && aligned4(a) && aligned4(b),
                  "gat_scores_mh: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && K > 0 && ldx >= H && n_rows >= 0 && n_rows < (1ll << 31),
                  "gat_scores_mh: need H>0, K>0, ldx>=H (H=%lld K=%lld ldx=%lld n=%lld)", (long long)H, (long long)K, (long long)ldx,
                  (long long)n_rows);
    if (K == 1) return glass_gat_scores_f32(X, ldx, att_src, att_dst, a, b, n_rows, H, stream);
    HeadMap hm;
    if (const int rc = head_map("gat_scores_mh", H, K, &hm)) return rc;
    if (n_rows == 0) return 0;
    hipLaunchKernelGGL(gat_scores_mh_kernel, dim3((unsigned)ceil_div(n_rows, kScoreRows)), dim3(kBlock), 0, (hipStream_t)stream, X,
                       ldx, att_src, att_dst, a, b, n_rows, (int)H, hm);
    return launch_status("glass_gat_scores_mh_f32");
}

extern "C" int64_t glass_spmm_gat_mh_ws_bytes(const int32_t* hdr, int64_t H, int64_t K) {
    if (!hdr || hdr[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0 || K <= 0) return GLASS_E_ARG;
    return (int64_t)hdr[H_NSLOTS] * (H + 2 * K) * (int64_t)sizeof(float);
}

extern "C" int64_t glass_spmm_gat_mh_edge_ws_bytes(const int32_t* hdr, int64_t H, int64_t K) {
    if (!hdr || hdr[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0 || K <= 0) return GLASS_E_ARG;
    return (int64_t)hdr[H_NSLOTS] * K * (int64_t)sizeof(float);
}

extern "C" int64_t glass_spmm_gat_mh_bwd_ws_bytes(const int32_t* hdr_t, int64_t H, int64_t K) {
    if (!hdr_t || hdr_t[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0 || K <= 0) return GLASS_E_ARG;
    return (int64_t)hdr_t[H_NSLOTS] * (H + K) * (int64_t)sizeof(float);
}

extern "C" int64_t glass_spmm_gat_mh_da_ws_bytes(const int32_t* hdr_t, int64_t H, int64_t K) {
    if (!hdr_t || hdr_t[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0 || K <= 0) return GLASS_E_ARG;
    return (int64_t)hdr_t[H_NSLOTS] * K * (int64_t)sizeof(float);
}

extern "C" int64_t glass_gat_datt_mh_ws_bytes(int64_t n_rows, int64_t H) {
    if (H <= 0 || n_rows < 0) return GLASS_E_ARG;
    return ceil_div(n_rows, datt_mh_rows_per_wg(H)) * 2 * H * (int64_t)sizeof(double);
}

extern "C" int glass_spmm_gat_mh_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                         const float* a, const float* b, float slope, float* Y, int64_t ldy, float* L,
                                         int64_t n_rows, int64_t H, int64_t K, const int32_t* hdr, const int32_t* plan_dev,
                                         void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && a && b && Y && L && hdr && plan_dev, "spmm_gat_mh: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col) && aligned4(val) && aligned4(X) && aligned4(a) && aligned4(b) && aligned4(Y) &&
                  aligned4(L) && aligned4(plan_dev) && aligned4(ws), "spmm_gat_mh: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && K > 0 && ldx >= H && ldy >= H, "spmm_gat_mh: need H>0, K>0, ldx>=H, ldy>=H (H=%lld K=%lld ldx=%lld ldy=%lld)",
                  (long long)H, (long long)K, (long long)ldx, (long long)ldy);
    GLASS_REQUIRE(slope == slope, "spmm_gat_mh: slope is NaN");
    if (K == 1) return glass_spmm_gat_csr_f32(rowptr, col, val, X, ldx, a, b, slope, Y, ldy, L, n_rows, H, hdr, plan_dev, ws, stream);
    HeadMap hm;
    if (const int rc = head_map("spmm_gat_mh", H, K, &hm)) return rc;
    if (const int rc = check_plan("spmm_gat_mh", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val), "spmm_gat_mh: null col/val");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_gat_mh: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* ps = (float*)ws;
    float* pm = ps + (int64_t)hdr[H_NSLOTS] * H;
    float* pz = pm + (int64_t)hdr[H_NSLOTS] * K;
    const bool vec = (ldx % 4 == 0) && (ldy % 4 == 0) && aligned16(X) && aligned16(Y) && (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1A_MH_FWD_CASE(VW, LPR)                                                                                           \
    return launch_gat_mh_fwd(GatMhFwdOp<VW, LPR>{col, val, X, ldx, a, b, slope, Y, ldy, L, ps, pm, pz, (int)H, hm}, rowptr, hdr, \
                             plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1A_MH_FWD_CASE);
#undef GLASS_K1A_MH_FWD_CASE
}

extern "C" int glass_spmm_gat_mh_edge_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx,
                                          const float* a, const float* b, float slope, const float* dY, int64_t lddy,
                                          const float* Y, int64_t ldy, const float* L, float* g, float* db, int64_t n_rows,
                                          int64_t H, int64_t K, const int32_t* hdr, const int32_t* plan_dev, void* ws,
                                          void* stream) {
    GLASS_REQUIRE(rowptr && X && a && b && dY && Y && L && db && hdr && plan_dev, "spmm_gat_mh_edge: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col) && aligned4(val) && aligned4(X) && aligned4(a) && aligned4(b) && aligned4(dY) &&
                  aligned4(Y) && aligned4(L) && aligned4(g) && aligned4(db) && aligned4(plan_dev) && aligned4(ws),
                  "spmm_gat_mh_edge: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && K > 0 && ldx >= H && lddy >= H && ldy >= H,
                  "spmm_gat_mh_edge: need H>0, K>0 and every ld >= H (H=%lld K=%lld ldx=%lld lddy=%lld ldy=%lld)", (long long)H,
                  (long long)K, (long long)ldx, (long long)lddy, (long long)ldy);
    GLASS_REQUIRE(slope == slope, "spmm_gat_mh_edge: slope is NaN");
    if (K == 1)
        return glass_spmm_gat_edge_f32(rowptr, col, val, X, ldx, a, b, slope, dY, lddy, Y, ldy, L, g, db, n_rows, H, hdr, plan_dev, ws,
                                       stream);
    HeadMap hm;
    if (const int rc = head_map("spmm_gat_mh_edge", H, K, &hm)) return rc;
    if (const int rc = check_plan("spmm_gat_mh_edge", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val && g), "spmm_gat_mh_edge: null col/val/g");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_gat_mh_edge: plan needs %d partial sums but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (ldx % 4 == 0) && (lddy % 4 == 0) && (ldy % 4 == 0) && aligned16(X) && aligned16(dY) && aligned16(Y);
#define GLASS_K1A_MH_EDGE_CASE(VW, LPR)                                                                                          \
    return launch_gat_mh_edge(GatMhEdgeOp<VW, LPR>{col, val, X, ldx, a, b, slope, dY, lddy, Y, ldy, L, g, db, (float*)ws, (int)H, \
                                                   hm, 1},                                                                       \
                              rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1A_MH_EDGE_CASE);
#undef GLASS_K1A_MH_EDGE_CASE
}

extern "C" int glass_spmm_gat_mh_bwd_f32(const int32_t* rowptr, const int32_t* col_t, const float* val_t, const int32_t* eid_t,
                                         const float* a, const float* b, float slope, const float* dY, int64_t lddy,
                                         const float* L, const float* g, const float* db, const float* att_src,
                                         const float* att_dst, float* dX, int64_t lddx, float* da, int64_t n_rows, int64_t H,
                                         int64_t K, const int32_t* hdr, const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && a && b && dY && L && db && att_src && att_dst && dX && da && hdr && plan_dev,
                  "spmm_gat_mh_bwd: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col_t) && aligned4(val_t) && aligned4(eid_t) && aligned4(a) && aligned4(b) &&
                  aligned4(dY) && aligned4(L) && aligned4(g) && aligned4(db) && aligned4(att_src) && aligned4(att_dst) &&
                  aligned4(dX) && aligned4(da) && aligned4(plan_dev) && aligned4(ws), "spmm_gat_mh_bwd: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && K > 0 && lddy >= H && lddx >= H,
                  "spmm_gat_mh_bwd: need H>0, K>0, lddy>=H, lddx>=H (H=%lld K=%lld lddy=%lld lddx=%lld)", (long long)H, (long long)K,
                  (long long)lddy, (long long)lddx);
    GLASS_REQUIRE(slope == slope, "spmm_gat_mh_bwd: slope is NaN");
    if (K == 1)
        return glass_spmm_gat_bwd_f32(rowptr, col_t, val_t, eid_t, a, b, slope, dY, lddy, L, g, db, att_src, att_dst, dX, lddx, da,
                                      n_rows, H, hdr, plan_dev, ws, stream);
    HeadMap hm;
    if (const int rc = head_map("spmm_gat_mh_bwd", H, K, &hm)) return rc;
    if (const int rc = check_plan("spmm_gat_mh_bwd", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col_t && val_t && eid_t && g), "spmm_gat_mh_bwd: null col_t/val_t/eid_t/g");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_gat_mh_bwd: plan needs %d partial rows but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* ps = (float*)ws;
    float* pda = ps + (int64_t)hdr[H_NSLOTS] * H;
    const bool vec = (lddy % 4 == 0) && (lddx % 4 == 0) && aligned16(dY) && aligned16(dX) && (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_K1A_MH_BWD_CASE(VW, LPR)                                                                                           \
    return launch_gat_mh_bwd(GatMhBwdOp<VW, LPR, true>{col_t, val_t, eid_t, a, b, slope, dY, lddy, L, g, db, att_src, att_dst, dX, \
                                                       lddx, da, ps, pda, (int)H, hm},                                           \
                             rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1A_MH_BWD_CASE);
#undef GLASS_K1A_MH_BWD_CASE
}

extern "C" int glass_spmm_gat_mh_da_f32(const int32_t* rowptr, const int32_t* col_t, const float* val_t, const int32_t* eid_t,
                                        const float* g, float* da, int64_t n_rows, int64_t H, int64_t K, int vec_form,
                                        const int32_t* hdr, const int32_t* plan_dev, void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && da && hdr && plan_dev, "spmm_gat_mh_da: null pointer");
    GLASS_REQUIRE(aligned4(rowptr) && aligned4(col_t) && aligned4(val_t) && aligned4(eid_t) && aligned4(g) && aligned4(da) &&
                  aligned4(plan_dev) && aligned4(ws), "spmm_gat_mh_da: pointer not 4-byte aligned");
    GLASS_REQUIRE(H > 0 && K > 0 && (!vec_form || H % 4 == 0),
                  "spmm_gat_mh_da: need H>0, K>0, and H a multiple of 4 in the 16-byte form (H=%lld K=%lld)", (long long)H, (long long)K);
    if (K == 1) return glass_spmm_gat_da_f32(rowptr, col_t, val_t, eid_t, g, da, n_rows, H, vec_form, hdr, plan_dev, ws, stream);
    HeadMap hm;
    if (const int rc = head_map("spmm_gat_mh_da", H, K, &hm)) return rc;
    if (const int rc = check_plan("spmm_gat_mh_da", hdr, n_rows, H)) return rc;
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col_t && val_t && eid_t && g), "spmm_gat_mh_da: null col_t/val_t/eid_t/g");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_gat_mh_da: plan needs %d partial sums but ws is null", hdr[H_NSLOTS]);
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = vec_form != 0;
#define GLASS_K1A_MH_DA_CASE(VW, LPR)                                                                                            \
    return launch_gat_mh_bwd(GatMhBwdOp<VW, LPR, false>{col_t, val_t, eid_t, nullptr, nullptr, 0.f, nullptr, 0, nullptr, g, nullptr, \
                                                        nullptr, nullptr, nullptr, 0, da, nullptr, (float*)ws, (int)H, hm},      \
                             rowptr, hdr, plan_dev, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_K1A_MH_DA_CASE);
#undef GLASS_K1A_MH_DA_CASE
}

extern "C" int glass_gat_datt_mh_f32(const float* X, int64_t ldx, const float* da, const float* db, float* datt_src,
                                     float* datt_dst, int64_t n_rows, int64_t H, int64_t K, void* ws, void* stream) {
    GLASS_REQUIRE(X && da && db && datt_src && datt_dst, "gat_datt_mh: null pointer");
    GLASS_REQUIRE(aligned4(X) && aligned4(da) && aligned4(db) && aligned4(datt_src) && aligned4(datt_dst),
                  "gat_datt_mh: pointer not 4-byte aligned");
    GLASS_REQUIRE(aligned8(ws), "gat_datt_mh: ws not 8-byte aligned");
    GLASS_REQUIRE(H > 0 && K > 0 && ldx >= H && n_rows >= 0 && n_rows < (1ll << 31),
                  "gat_datt_mh: need H>0, K>0, ldx>=H (H=%lld K=%lld ldx=%lld n=%lld)", (long long)H, (long long)K, (long long)ldx,
                  (long long)n_rows);
    if (K == 1) return glass_gat_datt_f32(X, ldx, da, db, datt_src, datt_dst, n_rows, H, ws, stream);
    HeadMap hm;
    if (const int rc = head_map("gat_datt_mh", H, K, &hm)) return rc;
    GLASS_REQUIRE(n_rows == 0 || ws, "gat_datt_mh: ws is null");
    if (n_rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int64_t rpw = datt_mh_rows_per_wg(H), n_wg = ceil_div(n_rows, rpw);
    const int hc = pow2_ceil_cap(H, kBlock);
    hipLaunchKernelGGL(gat_datt_mh_partial_kernel, dim3((unsigned)n_wg), dim3(kBlock), 0, st, X, ldx, da, db, n_rows, (int)H, hm, hc,
                       rpw, (double*)ws);
    hipLaunchKernelGGL(gat_datt_mh_final_kernel, dim3(1), dim3(kBlock), 0, st, (const double*)ws, n_wg, (int)H, datt_src, datt_dst);
    return launch_status("glass_gat_datt_mh_f32");
}
