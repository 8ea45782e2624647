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
//
// k-hop balls (GNNSeg.py:213-232, hop > 0): the node lists the extraction above takes, computed from the centre lists
// by a breadth-first walk over bitmaps (below, at seg_khop_kernel).
//
// Centre marks (GNNSeg.py:214-225) and the collate that pools over the centres only: seg_centre_index_kernel and
// seg_collate_centre_kernel, after the collate whose block body they share.
#include <algorithm>

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

// The part of a batch block every collate writes: its node map and its CSR pair.  Returns the block's node count (0 for
// an id outside the split), clamped to the room the caller's node offsets leave; off = the block's first batch node.
__device__ __forceinline__ int seg_collate_block(const int32_t* sub_ptr, const int32_t* sub_nodes, int n_sub,
                                                 const int32_t* rowptr_in, const int32_t* col_in, const float* val_in,
                                                 const int32_t* rowptr_out, const int32_t* col_out, const float* val_out,
                                                 int s, const int32_t* node_off, const int32_t* brow_in,
                                                 const int32_t* brow_out, int32_t* bcol_in, float* bval_in,
                                                 int32_t* bcol_out, float* bval_out, int32_t* node_map, int& off) {
    const int b = blockIdx.x;
    off = node_off[b];
    int m = node_off[b + 1] - off;
    int r0 = 0;
    if (s >= 0 && s < n_sub) {
        r0 = sub_ptr[s];
        const int ms = sub_ptr[s + 1] - r0;
        if (ms < m) m = ms;
    } else {
        m = 0;
    }
    for (int j = threadIdx.x; j < m; j += kBlock) node_map[off + j] = sub_nodes[r0 + j];
    if (m <= 0) return 0;
    seg_copy_block(rowptr_in, col_in, val_in, r0, r0 + m, brow_in, off, off + m, off, bcol_in, bval_in);
    seg_copy_block(rowptr_out, col_out, val_out, r0, r0 + m, brow_out, off, off + m, off, bcol_out, bval_out);
    return m;
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
    int off;
    const int m = seg_collate_block(sub_ptr, sub_nodes, n_sub, rowptr_in, col_in, val_in, rowptr_out, col_out, val_out,
                                    ids[blockIdx.x], node_off, brow_in, brow_out, bcol_in, bval_in, bcol_out, bval_out,
                                    node_map, off);
    int64_t* prow = pos + (int64_t)blockIdx.x * pos_width;
    for (int j = threadIdx.x; j < pos_width; j += kBlock) prow[j] = j < m ? (int64_t)(off + j) : (int64_t)-1;
}

// ---- centre marks of the balls (GNNSeg.py:214-225) and the collate that pools over them (GNNSeg.py:41-62) ----------
// Position of every centre in its own ball's sorted list: one workgroup per subgraph stages the ball (LDS or global, as
// the extraction does), one centre per lane, binary search.  -1 for a centre its ball does not hold.
__global__ __launch_bounds__(kBlock) void seg_centre_index_kernel(const int32_t* __restrict__ centre_ptr,
                                                                  const int32_t* __restrict__ centre_nodes,
                                                                  const int32_t* __restrict__ ball_ptr,
                                                                  const int32_t* __restrict__ ball_nodes,
                                                                  int32_t* __restrict__ centre_local) {
    __shared__ int lds[kSegLds];
    const int base = ball_ptr[blockIdx.x], m = ball_ptr[blockIdx.x + 1] - base;
    const int* list = seg_stage(lds, ball_nodes, base, m);
    const int c1 = centre_ptr[blockIdx.x + 1];
    for (int j = centre_ptr[blockIdx.x] + threadIdx.x; j < c1; j += kBlock)
        centre_local[j] = seg_find(list, m, centre_nodes[j]);
}

// The collate of a batch that pools over the centres: the block as above; the pos row lists the batch rows of the
// block's centres (their local indices ascend with the sorted centre ids); mark is 1 on those rows and 0 on the other
// rows of the ball.  Each mark byte has one writer: the row looks itself up in the block's centre_local list.
__global__ __launch_bounds__(kBlock) void seg_collate_centre_kernel(
    const int32_t* __restrict__ sub_ptr, const int32_t* __restrict__ sub_nodes, int n_sub,
    const int32_t* __restrict__ rowptr_in, const int32_t* __restrict__ col_in, const float* __restrict__ val_in,
    const int32_t* __restrict__ rowptr_out, const int32_t* __restrict__ col_out, const float* __restrict__ val_out,
    const int32_t* __restrict__ centre_ptr, const int32_t* __restrict__ centre_local, const int32_t* __restrict__ ids,
    const int32_t* __restrict__ node_off, const int32_t* __restrict__ brow_in, const int32_t* __restrict__ brow_out,
    int32_t* __restrict__ bcol_in, float* __restrict__ bval_in, int32_t* __restrict__ bcol_out,
    float* __restrict__ bval_out, int32_t* __restrict__ node_map, int64_t* __restrict__ pos, int pos_width,
    uint8_t* __restrict__ mark) {
    const int s = ids[blockIdx.x];
    int off;
    const int m = seg_collate_block(sub_ptr, sub_nodes, n_sub, rowptr_in, col_in, val_in, rowptr_out, col_out, val_out,
                                    s, node_off, brow_in, brow_out, bcol_in, bval_in, bcol_out, bval_out, node_map, off);
    int c0 = 0, k = 0;
    if (m > 0) {
        c0 = centre_ptr[s];
        k = centre_ptr[s + 1] - c0;
    }
    const int32_t* loc = centre_local + c0;
    int64_t* prow = pos + (int64_t)blockIdx.x * pos_width;
    for (int j = threadIdx.x; j < pos_width; j += kBlock) {
        const int l = j < k ? loc[j] : -1;
        prow[j] = (unsigned)l < (unsigned)m ? (int64_t)(off + l) : (int64_t)-1;
    }
    // (every row of the block's node range, also rows past a clamped m: the launch leaves no byte of mark unwritten)
    const int room = node_off[blockIdx.x + 1] - off;
    for (int j = threadIdx.x; j < room; j += kBlock) mark[off + j] = (j < m && seg_find(loc, k, j) >= 0) ? 1 : 0;
}

// ---- k-hop balls (GNNSeg.py:213-232, hop > 0) ----------------------------------------------------------------------
// One workgroup per subgraph walks in-edges breadth first over three bitmaps of the N base nodes: visited, frontier and
// next.  They live in LDS (dynamic, 3 * ceil(N / 32) words) when N <= GLASS_SEG_KHOP_LDS_NODES, otherwise in the
// workgroup's slice of the caller's workspace, and then the grid is capped at GLASS_SEG_KHOP_WS_SLOTS workgroups that
// take the subgraphs in turn.  Bits are only ever set (integer atomicOr), so the ball does not depend on the order the
// lanes run in; reading the visited words in order yields the ids ascending.
template <bool kLds>
struct KhopBits {
    uint32_t* p;
    __device__ __forceinline__ uint32_t ld(int w) const {
        if constexpr (kLds) return p[w];
        else return __hip_atomic_load(p + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void st(int w, uint32_t v) const {
        if constexpr (kLds) p[w] = v;
        else __hip_atomic_store(p + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ bool test(int v) const { return (ld(v >> 5) >> (v & 31)) & 1u; }
    __device__ __forceinline__ void set(int v) const {
        if constexpr (kLds) atomicOr(p + (v >> 5), 1u << (v & 31));
        else __hip_atomic_fetch_or(p + (v >> 5), 1u << (v & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// Barrier between the phases of a walk; the global-memory bitmaps also get an agent-scope release / acquire around it.
template <bool kLds>
__device__ __forceinline__ int khop_sync_or(int pred) {
    if constexpr (!kLds) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const int any = __syncthreads_or(pred);
    if constexpr (!kLds) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return any;
}

// Leaves vis = the radius-`hops` in-ball of the subgraph's centres: each hop adds the sources of the in-edges of the
// frontier's nodes; the walk stops early once a hop adds nothing.
template <bool kLds>
__device__ void khop_walk(const int32_t* in_rowptr, const int32_t* in_col, int n, int W, const int32_t* centres, int m,
                          int hops, KhopBits<kLds> vis, KhopBits<kLds> fr, KhopBits<kLds> nx) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    for (int w = threadIdx.x; w < W; w += kBlock) {
        vis.st(w, 0u);
        fr.st(w, 0u);
        nx.st(w, 0u);
    }
    khop_sync_or<kLds>(0);
    for (int j = threadIdx.x; j < m; j += kBlock) {
        const int v = centres[j];
        if ((unsigned)v < (unsigned)n) {
            vis.set(v);
            fr.set(v);
        }
    }
    khop_sync_or<kLds>(0);
    for (int h = 0; h < hops; ++h) {
        // expand: each wave reads 64 frontier words, then walks the set bits' rows together, one edge per lane
        for (int w0 = wave * kWave; w0 < W; w0 += kBlock) {
            const int w = w0 + lane;
            const uint32_t f = w < W ? fr.ld(w) : 0u;
            uint64_t nz = __ballot(f != 0u);
            while (nz) {
                const int l = __builtin_ctzll(nz);
                nz &= nz - 1;
                uint32_t fw = (uint32_t)__shfl((int)f, l, kWave);
                while (fw) {
                    const int u = ((w0 + l) << 5) + __builtin_ctz(fw);
                    fw &= fw - 1;
                    const int e1 = in_rowptr[u + 1];
                    for (int e = in_rowptr[u] + lane; e < e1; e += kWave) {
                        const int v = in_col[e];
                        if ((unsigned)v < (unsigned)n && !vis.test(v)) nx.set(v);
                    }
                }
            }
        }
        khop_sync_or<kLds>(0);
        // update: next = next & ~visited becomes the frontier, visited |= it
        int grew = 0;
        for (int w = threadIdx.x; w < W; w += kBlock) {
            const uint32_t old = vis.ld(w), x = nx.ld(w) & ~old;
            if (x) {
                vis.st(w, old | x);
                grew = 1;
            }
            fr.st(w, x);
            nx.st(w, 0u);
        }
        if (!khop_sync_or<kLds>(grew)) break;
    }
}

// Reads vis in order: returns the ball size (the same in every thread); kFill also writes the ids ascending to out[0,
// room).  A block-wide exclusive scan of the words' bit counts per 256-word tile (integer: bitwise repeatable).
template <bool kLds, bool kFill>
__device__ int khop_emit(KhopBits<kLds> vis, int W, int32_t* out, int room, int* wave_tot) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int run = 0;
    for (int w0 = 0; w0 < W; w0 += kBlock) {
        const int w = w0 + threadIdx.x;
        uint32_t bits = w < W ? vis.ld(w) : 0u;
        const int c = __popc(bits);
        int incl = c;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int t = __shfl_up(incl, o, kWave);
            if (lane >= o) incl += t;
        }
        if (lane == kWave - 1) wave_tot[wave] = incl;
        __syncthreads();
        int at = run + incl - c, tile = 0;
        for (int k = 0; k < kBlock / kWave; ++k) {
            if (k < wave) at += wave_tot[k];
            tile += wave_tot[k];
        }
        if constexpr (kFill) {
            for (; bits; bits &= bits - 1, ++at)
                if (at < room) out[at] = (w << 5) + __builtin_ctz(bits);
        }
        run += tile;
        __syncthreads();
    }
    return run;
}

template <bool kLds, bool kFill>
__global__ __launch_bounds__(kBlock) void seg_khop_kernel(const int32_t* __restrict__ in_rowptr,
                                                          const int32_t* __restrict__ in_col, int n,
                                                          const int32_t* __restrict__ sub_ptr,
                                                          const int32_t* __restrict__ sub_nodes, int n_sub, int hops,
                                                          uint32_t* __restrict__ ws, int32_t* __restrict__ ball_cnt,
                                                          const int32_t* __restrict__ ball_ptr,
                                                          int32_t* __restrict__ ball_nodes) {
    extern __shared__ uint32_t khop_lds[];
    __shared__ int wave_tot[kBlock / kWave];
    const int W = (n + 31) >> 5;
    uint32_t* bits = kLds ? khop_lds : ws + (size_t)blockIdx.x * 3 * W;
    const KhopBits<kLds> vis{bits}, fr{bits + W}, nx{bits + 2 * (size_t)W};
    for (int s = blockIdx.x; s < n_sub; s += gridDim.x) {
        const int base = sub_ptr[s];
        khop_walk<kLds>(in_rowptr, in_col, n, W, sub_nodes + base, sub_ptr[s + 1] - base, hops, vis, fr, nx);
        if constexpr (kFill) {
            const int out0 = ball_ptr[s];
            khop_emit<kLds, true>(vis, W, ball_nodes + out0, ball_ptr[s + 1] - out0, wave_tot);
        } else {
            const int size = khop_emit<kLds, false>(vis, W, nullptr, 0, wave_tot);
            if (threadIdx.x == 0) ball_cnt[s] = size;
        }
        khop_sync_or<kLds>(0);  // (the next subgraph clears the bitmaps)
    }
}

int seg_khop_launch(const int32_t* in_rowptr, const int32_t* in_col, int64_t n_base, const int32_t* sub_ptr,
                    const int32_t* sub_nodes, int64_t n_sub, int hops, void* ws, bool fill, int32_t* ball_cnt,
                    const int32_t* ball_ptr, int32_t* ball_nodes, void* stream) {
    if (n_sub == 0) return 0;
    const bool lds = n_base <= GLASS_SEG_KHOP_LDS_NODES;
    const unsigned grid = (unsigned)(lds ? n_sub : std::min<int64_t>(n_sub, GLASS_SEG_KHOP_WS_SLOTS));
    const size_t lds_bytes = lds ? (size_t)3 * ((n_base + 31) >> 5) * sizeof(uint32_t) : 0;
    auto kernel = lds ? (fill ? seg_khop_kernel<true, true> : seg_khop_kernel<true, false>)
                      : (fill ? seg_khop_kernel<false, true> : seg_khop_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlock), lds_bytes, (hipStream_t)stream, in_rowptr, in_col, (int)n_base,
                       sub_ptr, sub_nodes, (int)n_sub, hops, (uint32_t*)ws, ball_cnt, ball_ptr, ball_nodes);
    return launch_status(fill ? "glass_seg_khop_fill" : "glass_seg_khop_count");
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

int seg_centre_index_launch(const int32_t* centre_ptr, const int32_t* centre_nodes, int64_t n_sub,
                            const int32_t* ball_ptr, const int32_t* ball_nodes, int32_t* centre_local, void* stream) {
    if (n_sub == 0) return 0;
    hipLaunchKernelGGL(seg_centre_index_kernel, dim3((unsigned)n_sub), dim3(kBlock), 0, (hipStream_t)stream, centre_ptr,
                       centre_nodes, ball_ptr, ball_nodes, centre_local);
    return launch_status("glass_seg_centre_index");
}

int seg_collate_centre_launch(const int32_t* sub_ptr, const int32_t* sub_nodes, int64_t n_sub, const int32_t* rowptr_in,
                              const int32_t* col_in, const float* val_in, const int32_t* rowptr_out,
                              const int32_t* col_out, const float* val_out, const int32_t* centre_ptr,
                              const int32_t* centre_local, const int32_t* ids, int64_t n_batch, const int32_t* node_off,
                              const int32_t* brow_in, const int32_t* brow_out, int32_t* bcol_in, float* bval_in,
                              int32_t* bcol_out, float* bval_out, int32_t* node_map, int64_t* pos, int64_t pos_width,
                              uint8_t* mark, void* stream) {
    if (n_batch == 0) return 0;
    hipLaunchKernelGGL(seg_collate_centre_kernel, dim3((unsigned)n_batch), dim3(kBlock), 0, (hipStream_t)stream, sub_ptr,
                       sub_nodes, (int)n_sub, rowptr_in, col_in, val_in, rowptr_out, col_out, val_out, centre_ptr,
                       centre_local, ids, node_off, brow_in, brow_out, bcol_in, bval_in, bcol_out, bval_out, node_map, pos,
                       (int)pos_width, mark);
    return launch_status("glass_seg_collate_centre");
}

}  // namespace glass
