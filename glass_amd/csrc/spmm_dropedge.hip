// K2d: edge dropout (DropEdge) for the aggregations whose adjacency values are K2's ("sum", "mean", "gcn").  One keep bit per
// adjacency entry is drawn from the counter-based generator of common.h, the dropped entries' weights become +0.0f, and the
// values K2 (elementwise.hip: adj_degree_kernel / adj_values_kernel) gives for those weights are written for the forward CSR
// AND for the transposed one — the structure is unchanged, K1 runs on (rowptr, col, val') as it does on the stored values.
//
// The keep bit of entry (i = destination row, j = source column) is a function of (seed, step, call_id, i, j, n) alone:
//   key = symmetric ? min(i,j) * n + max(i,j) : i * n + j        (uint64)
//   u   = float(rand4(seed, step, call_id, key)[0] >> 8) * 2^-24, kept iff u >= p    (keep_scale's rule)
// so the transposed operand draws the identical bit from its own (row, col) — no permutation is read — and so do both
// directions of an undirected edge and its parallel duplicates under the symmetric key.
//
// Bit contract: deg', val', val_t' are the bits K2 leaves for the masked weights.  The degree pass therefore adds a row's
// entries in K2's order (one wave per row, lanes stride the entries by 64, the fixed xor-shuffle fold), a dropped entry
// contributing +0.0f in its own lane slot (s + +0.0f == s), and the value pass evaluates K2's expressions literally.
//
// Launches: "mean" / "gcn": the masked-degree launch, then one value launch over 2 n rows (forward rows, then transposed rows).
// "sum": the value launch alone; its forward rows leave the degree as they pass (nothing reads it in that launch).
// No atomics, no float reduction across waves, no plan: rows longer than 64 entries are walked by the lane-stride loop.
// Algorithmic bytes per entry and draw (from the code): degree pass 8 (w + col), value pass 12 forward (w + col + val', +1
// with the keep bytes) and 12 transposed, plus the deg' gathers of "gcn": about 32, against K1's 8 + 4 H.
#include "common.h"

namespace glass {

struct EdgeDrop {
    uint64_t seed, step, call_id;
    uint32_t n;
    float p;
    bool symmetric;
};

// (offsets within a row stay 32-bit; only the key is formed in 64 bits)
__device__ __forceinline__ bool edge_keep(const EdgeDrop& d, uint32_t i, uint32_t j) {
    const uint32_t a = (d.symmetric && j < i) ? j : i, b = (d.symmetric && j < i) ? i : j;
    uint32_t w[4];
    rand4(d.seed, d.step, d.call_id, (uint64_t)a * d.n + b, w);
    return (float)(w[0] >> 8) * (1.0f / 16777216.0f) >= d.p;
}

__device__ __forceinline__ EdgeDrop edge_drop(const int64_t* __restrict__ rng, uint64_t call_id, int n, float p, int symmetric) {
    EdgeDrop d;
    d.seed = (uint64_t)rng[0];
    d.step = (uint64_t)rng[1];
    d.call_id = call_id;
    d.n = (uint32_t)n;
    d.p = p;
    d.symmetric = symmetric != 0;
    return d;
}

// the row sum of the masked weights in K2's order, K2's +1 rule applied by the caller
__device__ __forceinline__ float masked_row_sum(const EdgeDrop& d, const int32_t* __restrict__ col, const float* __restrict__ w,
                                                int row, int e0, int e1, int lane) {
    float s = 0.f;
    for (int e = e0 + lane; e < e1; e += kWave) s += edge_keep(d, (uint32_t)row, (uint32_t)col[e]) ? w[e] : 0.f;
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) s += __shfl_xor(s, k);
    return s;
}

__global__ __launch_bounds__(kBlock) void dropedge_degree_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                 const float* __restrict__ w, int n, float p, int symmetric,
                                                                 const int64_t* __restrict__ rng, uint64_t call_id,
                                                                 float* __restrict__ deg) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (row >= n) return;
    const EdgeDrop d = edge_drop(rng, call_id, n, p, symmetric);
    const float s = masked_row_sum(d, col, w, (int)row, rowptr[row], rowptr[row + 1], lane);
    if (lane == 0) deg[row] = s < 0.5f ? s + 1.0f : s;
}

// Rows [0, n): forward row i, entries (i, col[e]).  Rows [n, 2 n): transposed row j = row - n, entries (col_t[e], j).
// SUM (aggr 1): deg is an OUTPUT of the forward rows; otherwise an input (the degree launch ran before).
template <bool SUM>
__global__ __launch_bounds__(kBlock) void dropedge_values_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                 const float* __restrict__ w, const int32_t* __restrict__ rowptr_t,
                                                                 const int32_t* __restrict__ col_t, const float* __restrict__ w_t,
                                                                 int n, int aggr, float p, int symmetric,
                                                                 const int64_t* __restrict__ rng, uint64_t call_id,
                                                                 float* deg, float* __restrict__ val, float* __restrict__ val_t,
                                                                 uint8_t* __restrict__ keep) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kBlock / kWave) + (threadIdx.x >> 6);
    if (r >= 2 * (int64_t)n) return;
    const EdgeDrop d = edge_drop(rng, call_id, n, p, symmetric);
    if (r < n) {
        const int row = (int)r;
        const int e0 = rowptr[row], e1 = rowptr[row + 1];
        if constexpr (SUM) {
            const float s = masked_row_sum(d, col, w, row, e0, e1, lane);
            if (lane == 0) deg[row] = s < 0.5f ? s + 1.0f : s;
            for (int e = e0 + lane; e < e1; e += kWave) {
                const bool k = edge_keep(d, (uint32_t)row, (uint32_t)col[e]);
                val[e] = k ? w[e] : 0.f;
                if (keep) keep[e] = k ? 1 : 0;
            }
        } else {
            const float dr = deg[row];
            const float inv = 1.0f / dr, rs = 1.0f / sqrtf(dr);  // K2's row factors
            for (int e = e0 + lane; e < e1; e += kWave) {
                const int j = col[e];
                const bool k = edge_keep(d, (uint32_t)row, (uint32_t)j);
                float v = k ? w[e] : 0.f;
                if (aggr == 0) v = inv * v;
                else v = rs * v * (1.0f / sqrtf(deg[j]));
                val[e] = v;
                if (keep) keep[e] = k ? 1 : 0;
            }
        }
    } else {
        const int row = (int)(r - n);  // the SOURCE column j of A; col_t[e] is the destination row i
        const int e0 = rowptr_t[row], e1 = rowptr_t[row + 1];
        if constexpr (SUM) {
            for (int e = e0 + lane; e < e1; e += kWave) val_t[e] = edge_keep(d, (uint32_t)col_t[e], (uint32_t)row) ? w_t[e] : 0.f;
        } else {
            const float rj = 1.0f / sqrtf(deg[row]);
            for (int e = e0 + lane; e < e1; e += kWave) {
                const int i = col_t[e];
                float v = edge_keep(d, (uint32_t)i, (uint32_t)row) ? w_t[e] : 0.f;
                const float di = deg[i];
                if (aggr == 0) v = (1.0f / di) * v;
                else v = (1.0f / sqrtf(di)) * v * rj;  // K2's order: row factor of i, the weight, column factor of j
                val_t[e] = v;
            }
        }
    }
}

int adj_dropedge_launch(const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* rowptr_t, const int32_t* col_t,
                        const float* w_t, int64_t n, int aggr, float p, int symmetric, const int64_t* rng, uint64_t call_id,
                        float* deg, float* val, float* val_t, uint8_t* keep, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int wpb = kBlock / kWave;
    const unsigned grid2 = (unsigned)ceil_div(2 * n, wpb);
    if (aggr == 1) {
        hipLaunchKernelGGL(dropedge_values_kernel<true>, dim3(grid2), dim3(kBlock), 0, st, rowptr, col, w, rowptr_t, col_t, w_t,
                           (int)n, aggr, p, symmetric, rng, call_id, deg, val, val_t, keep);
    } else {
        hipLaunchKernelGGL(dropedge_degree_kernel, dim3((unsigned)ceil_div(n, wpb)), dim3(kBlock), 0, st, rowptr, col, w, (int)n, p,
                           symmetric, rng, call_id, deg);
        hipLaunchKernelGGL(dropedge_values_kernel<false>, dim3(grid2), dim3(kBlock), 0, st, rowptr, col, w, rowptr_t, col_t, w_t,
                           (int)n, aggr, p, symmetric, rng, call_id, deg, val, val_t, keep);
    }
    return launch_status("glass_adj_dropedge_f32");
}

}  // namespace glass
