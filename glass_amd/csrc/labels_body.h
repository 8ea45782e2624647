// K4b, the body of the label launch as a device function (see labels.hip for the algorithm) — shared by the stand-alone
// kernels there and by the label workgroup of the step's head launch (dense.hip: glass_step_head_f32).
#pragma once
#include "common.h"

namespace glass {

constexpr int kLabThreads = 1024;

// Laboratory build only (tools/head_trace.py; D_STAMP: dense_common.h, empty in the product): the label workgroup's phases
// inside the step's head launch, stamped behind the barriers — 2 old labels off / new entries known, 3 owners elected,
// 6 list written.
#ifdef D_STAMP
#define LAB_STAMP(slot) D_STAMP(5, slot)
#else
#define LAB_STAMP(slot) do { } while (0)
#endif

// Where the batch comes from.  Plain: pos_src / y_src ARE the batch.  Gather (kGather): they are the data set's whole
// padded node matrix [n_all, smax] and target matrix [n_all, y_row_words]; the batch is the rows idx[0 .. n_pos / smax) —
// what ZGDataloader's `pos[perm], y[perm]` (impl/SubGDataset.py:69-72, 92-96) materialised with two index kernels and a
// copy is read in place (one more dependent load per entry; a row index outside [0, n_all) reads as padding).
struct BatchSrc {
    const int64_t* pos;
    const uint32_t* y;
    const int64_t* idx;
    int smax, y_row_words;
    int64_t n_all;
};

template <bool kGather>
__device__ __forceinline__ int64_t batch_entry(const BatchSrc& s, int e) {
    if (!kGather) return s.pos[e];
    const int r = e / s.smax;
    const int64_t row = s.idx[r];
    return (row >= 0 && row < s.n_all) ? s.pos[row * s.smax + (e - r * s.smax)] : -1;
}

// The body of the label launch: every thread of a kLabThreads-wide workgroup calls it (the stand-alone kernels of labels.hip; the
// label workgroup of the step's head launch, dense.hip step_head_kernel).
template <bool kGather>
__device__ __forceinline__ void batch_labels_body(const BatchSrc& src, int n_pos, int64_t* __restrict__ pos_dst,
                                                  uint32_t* __restrict__ y_dst, int64_t y_words, uint8_t* __restrict__ mask,
                                                  int32_t* __restrict__ lab_rows, int32_t* __restrict__ lab_count,
                                                  int32_t* __restrict__ owner, int64_t N, int incremental) {
    __shared__ int wave_cnt[kLabThreads / kWave];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    // this thread's first entry of the NEW batch is requested before anything else: its round trip runs beside phase 1's
    // (the barrier between the phases would otherwise put the two loads in a row)
    const int64_t p_first = tid < n_pos ? batch_entry<kGather>(src, tid) : -1;
    // 1. labels of the previous batch off (or all N bytes)
    if (incremental) {
        if (pos_dst)
            for (int e = tid; e < n_pos; e += kLabThreads) {
                const int64_t p = pos_dst[e];
                if (p >= 0 && p < N) mask[p] = 0;
            }
    } else {
        const int64_t head = (16 - (reinterpret_cast<uintptr_t>(mask) & 15u)) & 15u;  // bytes up to 16-B alignment
        for (int64_t k = tid; k < head && k < N; k += kLabThreads) mask[k] = 0;
        const int64_t vecs = N > head ? (N - head) / 16 : 0;
        uint4* mv = reinterpret_cast<uint4*>(mask + head);
        for (int64_t k = tid; k < vecs; k += kLabThreads) mv[k] = make_uint4(0u, 0u, 0u, 0u);
        for (int64_t k = head + vecs * 16 + tid; k < N; k += kLabThreads) mask[k] = 0;
    }
    __syncthreads();
    LAB_STAMP(2);
    // 2. the new batch: fixed buffers, label bytes; the lowest entry index naming a node owns it (owner words are
    //    INT32_MAX on entry)
    for (int e = tid; e < n_pos; e += kLabThreads) {
        const int64_t p = e == tid ? p_first : batch_entry<kGather>(src, e);
        if (pos_dst) pos_dst[e] = p;
        if (p >= 0 && p < N) {
            mask[p] = 1;
            atomicMin(owner + p, e);
        }
    }
    for (int64_t k = tid; k < y_words; k += kLabThreads) {
        if (!kGather) {
            y_dst[k] = src.y[k];
        } else {
            const int64_t r = k / src.y_row_words;
            const int64_t row = src.idx[r];
            y_dst[k] = (row >= 0 && row < src.n_all) ? src.y[row * src.y_row_words + (k - r * src.y_row_words)] : 0u;
        }
    }
    __syncthreads();
    LAB_STAMP(3);
    // 3. owners, compacted in entry order
    int base = 0;
    for (int e0 = 0; e0 < n_pos; e0 += kLabThreads) {
        const int e = e0 + tid;
        const int64_t p = e0 == 0 ? p_first : (e < n_pos ? batch_entry<kGather>(src, e) : -1);
        const bool own = p >= 0 && p < N && __hip_atomic_load(owner + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == e;
        const unsigned long long bal = __ballot(own);
        if (lane == 0) wave_cnt[w] = __popcll(bal);
        __syncthreads();
        int off = base, total = 0;
        for (int ww = 0; ww < kLabThreads / kWave; ++ww) {
            if (ww < w) off += wave_cnt[ww];
            total += wave_cnt[ww];
        }
        if (own) lab_rows[off + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)p;
        base += total;
        __syncthreads();
    }
    LAB_STAMP(6);
    if (tid == 0) lab_count[0] = base;
    // 4. the owner words of the named nodes back to INT32_MAX (every read of them lies before the loop's last barrier)
    for (int e = tid; e < n_pos; e += kLabThreads) {
        const int64_t p = e == tid ? p_first : batch_entry<kGather>(src, e);
        if (p >= 0 && p < N) owner[p] = INT32_MAX;
    }
}

// ---- the epoch plan (glass_epoch_plan_build): what the body above derives from the batch's entries alone — the unique
// labeled rows in first-occurrence order and their number — for EVERY batch of an epoch, built by one launch when the epoch's
// index batches are installed.  One record of epoch_plan_stride(cap) int32 words per batch (cap = n_idx * smax entries):
// word 0 the count, words kPlanHead .. the rows.  The label workgroup of a replayed step then copies its batch's record
// (batch_labels_plan_body) instead of electing owners: no atomicMin round, no owner read-back, no compaction, no owner restore.
constexpr int kPlanHead = 4;  // int32 words in front of a record's rows (the rows stay 16-B aligned)
__host__ __device__ inline int64_t epoch_plan_stride(int64_t cap) { return kPlanHead + ((cap + 3) & ~(int64_t)3); }

// Phases 2 - 4 of batch_labels_body without the label bytes and the hand-over: the same owner election (lowest entry
// index, integer atomicMin) and the same ballot compaction, so rows / count are exactly lab_rows / lab_count of that body.
// owner: N words, INT32_MAX on entry and on exit, private to the calling workgroup.
template <bool kGather>
__device__ __forceinline__ void unique_rows_body(const BatchSrc& src, int n_pos, int32_t* __restrict__ rows,
                                                 int32_t* __restrict__ count, int32_t* __restrict__ owner, int64_t N) {
    __shared__ int plan_wave_cnt[kLabThreads / kWave];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int e = tid; e < n_pos; e += kLabThreads) {
        const int64_t p = batch_entry<kGather>(src, e);
        if (p >= 0 && p < N) atomicMin(owner + p, e);
    }
    __syncthreads();
    int base = 0;
    for (int e0 = 0; e0 < n_pos; e0 += kLabThreads) {
        const int e = e0 + tid;
        const int64_t p = e < n_pos ? batch_entry<kGather>(src, e) : -1;
        const bool own = p >= 0 && p < N && __hip_atomic_load(owner + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == e;
        const unsigned long long bal = __ballot(own);
        if (lane == 0) plan_wave_cnt[w] = __popcll(bal);
        __syncthreads();
        int off = base, total = 0;
        for (int ww = 0; ww < kLabThreads / kWave; ++ww) {
            if (ww < w) off += plan_wave_cnt[ww];
            total += plan_wave_cnt[ww];
        }
        if (own) rows[off + __popcll(bal & ((1ull << lane) - 1ull))] = (int32_t)p;
        base += total;
        __syncthreads();
    }
    if (tid == 0) count[0] = base;
    for (int e = tid; e < n_pos; e += kLabThreads) {
        const int64_t p = batch_entry<kGather>(src, e);
        if (p >= 0 && p < N) owner[p] = INT32_MAX;
    }
    __syncthreads();  // (the caller's next batch elects on the same words)
}

// The label launch of a step whose batch has a plan record `rec`: the hand-over and the incremental label bytes as in
// batch_labels_body, rows / count copied from the record.  Every load that depends on nothing in here (the thread's new
// entry, its old entry, its plan row) is requested before the one barrier.  The owner words are not touched.
template <bool kGather>
__device__ __forceinline__ void batch_labels_plan_body(const BatchSrc& src, int n_pos, int64_t* __restrict__ pos_dst,
                                                       uint32_t* __restrict__ y_dst, int64_t y_words, uint8_t* __restrict__ mask,
                                                       int32_t* __restrict__ lab_rows, int32_t* __restrict__ lab_count,
                                                       const int32_t* __restrict__ rec, int64_t N) {
    const int tid = threadIdx.x;
    const int64_t p_first = tid < n_pos ? batch_entry<kGather>(src, tid) : -1;
    const int32_t r_first = tid < n_pos ? rec[kPlanHead + tid] : -1;  // (inside the record whatever the count says)
    int cnt = rec[0];
    cnt = cnt < 0 ? 0 : (cnt > n_pos ? n_pos : cnt);
    // 1. labels of the previous batch off
    for (int e = tid; e < n_pos; e += kLabThreads) {
        const int64_t p = pos_dst[e];
        if (p >= 0 && p < N) mask[p] = 0;
    }
    __syncthreads();
    LAB_STAMP(2);
    // 2. the new batch: fixed buffers; label bytes and the list from the record
    for (int e = tid; e < n_pos; e += kLabThreads) pos_dst[e] = e == tid ? p_first : batch_entry<kGather>(src, e);
    for (int k = tid; k < cnt; k += kLabThreads) {
        const int32_t r = k == tid ? r_first : rec[kPlanHead + k];
        lab_rows[k] = r;
        if (r >= 0 && r < N) mask[r] = 1;
    }
    for (int64_t k = tid; k < y_words; k += kLabThreads) {
        if (!kGather) {
            y_dst[k] = src.y[k];
        } else {
            const int64_t r = k / src.y_row_words;
            const int64_t row = src.idx[r];
            y_dst[k] = (row >= 0 && row < src.n_all) ? src.y[row * src.y_row_words + (k - r * src.y_row_words)] : 0u;
        }
    }
    if (tid == 0) lab_count[0] = cnt;
}

template <bool kGather>
__global__ __launch_bounds__(kLabThreads) void batch_labels_kernel(const BatchSrc src, int n_pos,
                                                                   int64_t* __restrict__ pos_dst,
                                                                   uint32_t* __restrict__ y_dst, int64_t y_words,
                                                                   uint8_t* __restrict__ mask,
                                                                   int32_t* __restrict__ lab_rows,
                                                                   int32_t* __restrict__ lab_count,
                                                                   int32_t* __restrict__ owner, int64_t N,
                                                                   int incremental) {
    batch_labels_body<kGather>(src, n_pos, pos_dst, y_dst, y_words, mask, lab_rows, lab_count, owner, N, incremental);
}

}  // namespace glass
