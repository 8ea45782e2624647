// K10  GNN-seg: induced subgraphs of a split (hop 0) and block-diagonal batches of them.
//
// Extraction (GNNSeg.py:213-226): one workgroup per subgraph.  Its sorted unique node list is staged in LDS when it fits
// (global memory otherwise); each wave takes member nodes in turn and walks the node's base row in both orientations,
// 64 edges at a time, one edge per lane: the far end is looked up by binary search in the list, a hit is an entry of
// the subgraph's local CSR.  Count pass: entries per row (+ the GCN in-degree, a fixed-order wave reduction); the caller
// scans the counts; fill pass: the same walk, each hit placed by a ballot prefix, so entries keep the base row's
// (ascending) column order.  No float atomics anywhere: the output is bitwise repeatable.
//
// Collate (GNNSeg.py:41-62): one workgroup per subgraph of the batch copies its block (columns shifted by the block's
// node offset), its node map and its row of the padded pool matrix.  The batch row pointers come from the host.
#include "common.h"

namespace glass {

constexpr int kSegLds = GLASS_SEG_LDS_NODES;

// index of v in the sorted list[0, m), or -1
__device__ __forceinline__ int seg_find(const int* list, int m, int v) {
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return (lo < m && list[lo] == v) ? lo : -1;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

__device__ __forceinline__ float seg_dinv(float d) { return d > 0.f ? 1.f / sqrtf(d) : (d == 0.f ? 0.f : __builtin_nanf("")); }

// Stage the subgraph's node list; returns the pointer the searches read (LDS or global).
__device__ __forceinline__ const int* seg_stage(int* lds, const int32_t* sub_nodes, int base, int m) {
    if (m <= kSegLds) {
        for (int j = threadIdx.x; j < m; j += kBlock) lds[j] = sub_nodes[base + j];
        __syncthreads();
        return lds;
    }
    return sub_nodes + base;
}

// Entries of one base row inside the subgraph: count, and (GCN) the weight sum, per wave.
__device__ __forceinline__ void seg_row_count(const int32_t* rowptr, const int32_t* col, const float* w, int g,
                                              const int* list, int m, bool want_w, int& cnt, float& wsum) {
    const int lane = threadIdx.x & (kWave - 1);
    const int e1 = rowptr[g + 1];
    int c = 0;
    float s = 0.f;
    for (int e = rowptr[g] + lane; e - lane < e1; e += kWave) {
        if (e < e1 && seg_find(list, m, col[e]) >= 0) {
            ++c;
            if (want_w) s += w[e];
        }
    }
    cnt = wave_sum_i(c);
    wsum = want_w ? wave_sum_f(s) : 0.f;
}

__global__ __launch_bounds__(kBlock) void seg_count_kernel(const int32_t* __restrict__ in_rowptr,
                                                           const int32_t* __restrict__ in_col,
                                                           const float* __restrict__ in_w,
                                                           const int32_t* __restrict__ out_rowptr,
                                                           const int32_t* __restrict__ out_col,
                                                           const int32_t* __restrict__ sub_ptr,
                                                           const int32_t* __restrict__ sub_nodes, int mode,
                                                           int32_t* __restrict__ cnt_in, int32_t* __restrict__ cnt_out,
                                                           float* __restrict__ deg) {
    __shared__ int lds[kSegLds];
    const int base = sub_ptr[blockIdx.x], m = sub_ptr[blockIdx.x + 1] - base;
    const int* list = seg_stage(lds, sub_nodes, base, m);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int diag = mode == GLASS_SEG_GIN ? 1 : 0;
    for (int i = wave; i < m; i += kBlock / kWave) {
        const int g = list[i];
        int c_in, c_out;
        float d, unused;
        seg_row_count(in_rowptr, in_col, in_w, g, list, m, mode == GLASS_SEG_GCN, c_in, d);
        seg_row_count(out_rowptr, out_col, nullptr, g, list, m, false, c_out, unused);
        if (lane == 0) {
            cnt_in[base + i] = c_in + diag;
            cnt_out[base + i] = c_out + diag;
            if (mode == GLASS_SEG_GCN) deg[base + i] = d;
        }
    }
}

// Fill one local row.  Value of a hit: GIN 1; GCN (dinv[src] * w) * dinv[dst] with src / dst the row or the column
// depending on the orientation (row_is_dst: target-major) — the same expression in both orientations, so that the two
// hold bitwise the same values.
__device__ __forceinline__ void seg_row_fill(const int32_t* rowptr, const int32_t* col, const float* w, int g, int i,
                                             const int* list, int m, int mode, bool row_is_dst, const float* deg_blk,
                                             int dst0, int32_t* out_col, float* out_val) {
    const int lane = threadIdx.x & (kWave - 1);
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (kWave - lane));
    const bool gin = mode == GLASS_SEG_GIN;
    const float dinv_row = gin ? 0.f : seg_dinv(deg_blk[i]);
    const int e1 = rowptr[g + 1];
    int run = 0, n_lt = 0;
    for (int e0 = rowptr[g]; e0 < e1; e0 += kWave) {
        const int e = e0 + lane;
        const int j = e < e1 ? seg_find(list, m, col[e]) : -1;
        const uint64_t hits = __ballot(j >= 0);
        const uint64_t lt = __ballot(j >= 0 && j < i);
        if (j >= 0) {
            const int at = dst0 + run + __popcll(hits & below) + ((gin && j >= i) ? 1 : 0);
            out_col[at] = j;
            float v = 1.f;
            if (!gin) {
                const float dinv_col = seg_dinv(deg_blk[j]);
                v = row_is_dst ? (dinv_col * w[e]) * dinv_row : (dinv_row * w[e]) * dinv_col;
            }
            out_val[at] = v;
        }
        run += __popcll(hits);
        n_lt += __popcll(lt);
    }
    if (gin && lane == 0) {
        out_col[dst0 + n_lt] = i;
        out_val[dst0 + n_lt] = 1.f;
    }
}

__global__ __launch_bounds__(kBlock) void seg_fill_kernel(const int32_t* __restrict__ in_rowptr,
                                                          const int32_t* __restrict__ in_col,
                                                          const float* __restrict__ in_w,
                                                          const int32_t* __restrict__ out_rowptr,
                                                          const int32_t* __restrict__ out_col,
                                                          const float* __restrict__ out_w,
                                                          const int32_t* __restrict__ sub_ptr,
                                                          const int32_t* __restrict__ sub_nodes, int mode,
                                                          const float* __restrict__ deg,
                                                          const int32_t* __restrict__ rowptr_in,
                                                          const int32_t* __restrict__ rowptr_out,
                                                          int32_t* __restrict__ col_in, float* __restrict__ val_in,
                                                          int32_t* __restrict__ col_o, float* __restrict__ val_o) {
    __shared__ int lds[kSegLds];
    const int base = sub_ptr[blockIdx.x], m = sub_ptr[blockIdx.x + 1] - base;
    const int* list = seg_stage(lds, sub_nodes, base, m);
    const int wave = threadIdx.x / kWave;
    const float* deg_blk = deg ? deg + base : nullptr;
    for (int i = wave; i < m; i += kBlock / kWave) {
        const int g = list[i];
        seg_row_fill(in_rowptr, in_col, in_w, g, i, list, m, mode, true, deg_blk, rowptr_in[base + i], col_in, val_in);
        seg_row_fill(out_rowptr, out_col, out_w, g, i, list, m, mode, false, deg_blk, rowptr_out[base + i], col_o, val_o);
    }
}

__device__ __forceinline__ void seg_copy_block(const int32_t* rowptr, const int32_t* col, const float* val, int r0,
                                               int r1, const int32_t* brow, int b0, int b1, int shift, int32_t* bcol,
                                               float* bval) {
    const int e0 = rowptr[r0];
    int n = rowptr[r1] - e0;
    const int be0 = brow[b0];
    const int room = brow[b1] - be0;
    if (n > room) n = room;  // (inconsistent row pointers: never write past the block's batch range)
    for (int t = threadIdx.x; t < n; t += kBlock) {
        bcol[be0 + t] = col[e0 + t] + shift;
        bval[be0 + t] = val[e0 + t];
    }
}

__global__ __launch_bounds__(kBlock) void seg_collate_kernel(const int32_t* __restrict__ sub_ptr,
                                                             const int32_t* __restrict__ sub_nodes, int n_sub,
                                                             const int32_t* __restrict__ rowptr_in,
                                                             const int32_t* __restrict__ col_in,
                                                             const float* __restrict__ val_in,
                                                             const int32_t* __restrict__ rowptr_out,
                                                             const int32_t* __restrict__ col_out,
                                                             const float* __restrict__ val_out,
                                                             const int32_t* __restrict__ ids,
                                                             const int32_t* __restrict__ node_off,
                                                             const int32_t* __restrict__ brow_in,
                                                             const int32_t* __restrict__ brow_out,
                                                             int32_t* __restrict__ bcol_in, float* __restrict__ bval_in,
                                                             int32_t* __restrict__ bcol_out, float* __restrict__ bval_out,
                                                             int32_t* __restrict__ node_map, int64_t* __restrict__ pos,
                                                             int pos_width) {
    const int b = blockIdx.x;
    const int s = ids[b];
    const int off = node_off[b];
    int m = node_off[b + 1] - off;
    int r0 = 0;
    if (s >= 0 && s < n_sub) {
        r0 = sub_ptr[s];
        const int ms = sub_ptr[s + 1] - r0;
        if (ms < m) m = ms;
    } else {
        m = 0;
    }
    int64_t* prow = pos + (int64_t)b * pos_width;
    for (int j = threadIdx.x; j < pos_width; j += kBlock) prow[j] = j < m ? (int64_t)(off + j) : (int64_t)-1;
    for (int j = threadIdx.x; j < m; j += kBlock) node_map[off + j] = sub_nodes[r0 + j];
    if (m == 0) return;
    seg_copy_block(rowptr_in, col_in, val_in, r0, r0 + m, brow_in, off, off + m, off, bcol_in, bval_in);
    seg_copy_block(rowptr_out, col_out, val_out, r0, r0 + m, brow_out, off, off + m, off, bcol_out, bval_out);
}

int seg_extract_count_launch(const int32_t* in_rowptr, const int32_t* in_col, const float* in_w,
                             const int32_t* out_rowptr, const int32_t* out_col, const int32_t* sub_ptr,
                             const int32_t* sub_nodes, int64_t n_sub, int mode, int32_t* cnt_in, int32_t* cnt_out,
                             float* deg, void* stream) {
    if (n_sub == 0) return 0;
    hipLaunchKernelGGL(seg_count_kernel, dim3((unsigned)n_sub), dim3(kBlock), 0, (hipStream_t)stream, in_rowptr, in_col,
                       in_w, out_rowptr, out_col, sub_ptr, sub_nodes, mode, cnt_in, cnt_out, deg);
    return launch_status("glass_seg_extract_count");
}

int seg_extract_fill_launch(const int32_t* in_rowptr, const int32_t* in_col, const float* in_w,
                            const int32_t* out_rowptr, const int32_t* out_col, const float* out_w,
                            const int32_t* sub_ptr, const int32_t* sub_nodes, int64_t n_sub, int mode, const float* deg,
                            const int32_t* rowptr_in, const int32_t* rowptr_out, int32_t* col_in, float* val_in,
                            int32_t* col_out, float* val_out, void* stream) {
    if (n_sub == 0) return 0;
    hipLaunchKernelGGL(seg_fill_kernel, dim3((unsigned)n_sub), dim3(kBlock), 0, (hipStream_t)stream, in_rowptr, in_col,
                       in_w, out_rowptr, out_col, out_w, sub_ptr, sub_nodes, mode, deg, rowptr_in, rowptr_out, col_in,
                       val_in, col_out, val_out);
    return launch_status("glass_seg_extract_fill");
}

int seg_collate_launch(const int32_t* sub_ptr, const int32_t* sub_nodes, int64_t n_sub, const int32_t* rowptr_in,
                       const int32_t* col_in, const float* val_in, const int32_t* rowptr_out, const int32_t* col_out,
                       const float* val_out, const int32_t* ids, int64_t n_batch, const int32_t* node_off,
                       const int32_t* brow_in, const int32_t* brow_out, int32_t* bcol_in, float* bval_in,
                       int32_t* bcol_out, float* bval_out, int32_t* node_map, int64_t* pos, int64_t pos_width,
                       void* stream) {
    if (n_batch == 0) return 0;
    hipLaunchKernelGGL(seg_collate_kernel, dim3((unsigned)n_batch), dim3(kBlock), 0, (hipStream_t)stream, sub_ptr,
                       sub_nodes, (int)n_sub, rowptr_in, col_in, val_in, rowptr_out, col_out, val_out, ids, node_off,
                       brow_in, brow_out, bcol_in, bval_in, bcol_out, bval_out, node_map, pos, (int)pos_width);
    return launch_status("glass_seg_collate");
}

}  // namespace glass
