// Two-layer MLP prediction head + loss of a training step: the head the reference builds for GNN-seg and GNNEmb,
// MLP(in, hidden, out, 2, dropout, activation) = Linear -> Dropout -> activation -> Linear (impl/models.py:56-80, built at
// GNNSeg.py:272-277), then CrossEntropyLoss or BCEWithLogitsLoss on the flattened tensors with mean reduction, as head.hip
// does for the bare nn.Linear head.  Forward + loss in two launches, the whole backward in two, evaluation in one — as
// separate framework calls the same work is two dozen or so launches (an estimate from the module list, not a count) on
// operands of [B <= a few hundred, <= 512]: launch latency.
// fp32, no float atomics, every sum in a fixed order: bitwise repeatable.  The dropout mask is never stored: forward and
// backward regenerate it from the counter-based stream (common.h: Drop / drop_scales) by element (row, hidden unit).
#include "head_loss.h"

namespace glass {

constexpr int kMlpMaxHd = 1024;   // hidden units: the hidden row of a subgraph stays in LDS
constexpr int kMlpStageC = 4096;  // input features up to which the pooled row is staged in LDS (wider rows are read in place)
constexpr int kMlpTile = 1024;    // subgraphs per LDS tile of the weight-gradient sums

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// 64-lane dot product of two rows (the same sum on every lane)
__device__ __forceinline__ float wave_dot(const float* x, const float* __restrict__ w, int n, int lane) {
    float s = 0.f;
    for (int c = lane; c < n; c += kWave) s = fmaf(x[c], w[c], s);
    return wave_sum(s);
}

__device__ __forceinline__ float mlp_keep(const Drop& drop, int64_t row, int col) {
    if (drop.p <= 0.f) return 1.f;
    float ds[1];
    drop_scales<1>(drop, row, col, ds);
    return ds[0];
}

// derivative of the activation from its argument, with the library exponential (this path is latency-bound, not
// throughput-bound; relu'(0) = 0 as torch's)
__device__ __forceinline__ float mlp_act_grad(int act, float h) {
    if (act == GLASS_ACT_NONE) return 1.f;
    return h > 0.f ? 1.f : (act == GLASS_ACT_ELU ? expf(h) : 0.f);
}

// One workgroup per subgraph b.  The pooled row is staged in LDS (up to kMlpStageC features), waves take hidden units
// j = wave, wave + 4, ... as 64-lane dot products: h = pooled . W1[j] + b1[j], a = act(h * keep) goes to the hidden row
// in LDS (h itself to hidden_pre for the backward); then the waves take the classes the same way over the hidden row.
// TRAIN: lane 0 of wave 0 finishes the K-term softmax / sigmoid and the row's loss term exactly as head_logits_kernel
// does; (head_loss.h: head_loss_row); the mean is head_mlp_loss_mean_kernel's.  Evaluation (TRAIN = false): the logits are all that is written — same
// sums in the same order, so they are bitwise the training entry's at p = 0.
// WT: the weighted losses (head_loss.h; cw / pw nullable) — launched only when one of them is set.
template <bool TRAIN, bool WT>
__global__ __launch_bounds__(kBlock) void head_mlp_fwd_kernel(const float* __restrict__ pooled, int64_t ldp,
                                                              const float* __restrict__ W1, const float* __restrict__ b1,
                                                              const float* __restrict__ W2, const float* __restrict__ b2,
                                                              const void* __restrict__ target, int mode, int act, Drop drop,
                                                              const uint64_t* __restrict__ rng, int C, int Hd, int K,
                                                              int stage, float* __restrict__ hidden_pre,
                                                              float* __restrict__ logits, int64_t ldl,
                                                              float* __restrict__ prob, float* __restrict__ loss_rows,
                                                              const float* __restrict__ cw, const float* __restrict__ pw) {
    extern __shared__ float lds[];  // hidden row [Hd], then the pooled row [C] when staged
    __shared__ float zs[kMaxK];
    float* hs = lds;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* p = pooled + (int64_t)b * ldp;
    if (drop.p > 0.f) {
        drop.seed = rng[0];
        drop.step = rng[1];
    }
    if (stage) {
        float* ps = lds + Hd;
        for (int c = tid; c < C; c += kBlock) ps[c] = p[c];
        __syncthreads();
        p = ps;
    }
    for (int j = w; j < Hd; j += kBlock / kWave) {
        const float s = wave_dot(p, W1 + (int64_t)j * C, C, lane);
        if (lane == 0) {
            const float h = s + b1[j];
            if (TRAIN) hidden_pre[(int64_t)b * Hd + j] = h;
            hs[j] = act_exact(act, h * mlp_keep(drop, b, j));
        }
    }
    __syncthreads();
    for (int k = w; k < K; k += kBlock / kWave) {
        const float s = wave_dot(hs, W2 + (int64_t)k * Hd, Hd, lane);
        if (lane == 0) zs[k] = s + b2[k];
    }
    __syncthreads();
    if (!TRAIN) {
        for (int k = tid; k < K; k += kBlock) logits[(int64_t)b * ldl + k] = zs[k];
        return;
    }
    if (tid != 0) return;
    if constexpr (WT)
        loss_rows[b] = head_loss_row(zs, target, mode, b, K, logits, ldl, prob, cw, pw);
    else
        loss_rows[b] = head_loss_row(zs, target, mode, b, K, logits, ldl, prob);
}

// mean of the B row terms, summed in index order (as head.hip's)
__global__ __launch_bounds__(kBlock) void head_mlp_loss_mean_kernel(const float* __restrict__ loss_rows, int B, float denom,
                                                                    float* __restrict__ loss) {
    head_loss_mean(loss_rows, B, denom, loss);
}

// weighted cross-entropy: divided by the batch's weight sum, recomputed from target and cw
__global__ __launch_bounds__(kBlock) void head_mlp_loss_mean_w_kernel(const float* __restrict__ loss_rows, int B, float denom,
                                                                      float* __restrict__ loss, const float* __restrict__ cw,
                                                                      const void* __restrict__ target, int K) {
    head_loss_mean(loss_rows, B, denom, loss, cw, target, K);
}

// Backward, launch 1 — one workgroup per subgraph b: dlogits[b, :] staged in LDS, then per hidden unit j (thread-strided)
// da = sum_k dlogits[k] W2[k, j], dh = da * act'(h * keep) * keep with the regenerated mask; dh[b, :] and a[b, :] =
// act(h * keep) go to the workspace (launch 2 sums them over b) and dh stays in LDS for dpooled[b, :] = dh @ W1.
// WT (both backward kernels): dlogits of the weighted losses; with class weights each workgroup recomputes the weight sum.
template <bool WT>
__global__ __launch_bounds__(kBlock) void head_mlp_bwd_rows_kernel(const float* __restrict__ W1, const float* __restrict__ W2,
                                                                   const float* __restrict__ hidden_pre,
                                                                   const float* __restrict__ prob,
                                                                   const void* __restrict__ target, int mode, int act,
                                                                   Drop drop, const uint64_t* __restrict__ rng,
                                                                   const float* __restrict__ gl, int B, int C, int Hd, int K,
                                                                   float* __restrict__ dh_ws, float* __restrict__ a_ws,
                                                                   float* __restrict__ dpooled, int64_t lddp,
                                                                   const float* __restrict__ cw, const float* __restrict__ pw) {
    __shared__ float dl[kMaxK];
    __shared__ float dhs[kMlpMaxHd];
    const int b = blockIdx.x, tid = threadIdx.x;
    float scale;
    if constexpr (WT) {
        __shared__ double wred[kBlock];
        scale = head_loss_scale(gl, mode, B, K, cw, target, wred);
    } else {
        scale = gl[0] / head_loss_denom(mode, B, K);
    }
    if (drop.p > 0.f) {
        drop.seed = rng[0];
        drop.step = rng[1];
    }
    for (int k = tid; k < K; k += kBlock) dl[k] = WT ? dlogit(prob, target, mode, b, k, K, scale, cw, pw) : dlogit(prob, target, mode, b, k, K, scale);
    __syncthreads();
    for (int j = tid; j < Hd; j += kBlock) {
        float da = 0.f;
#pragma unroll 8
        for (int k = 0; k < K; ++k) da = fmaf(dl[k], W2[(int64_t)k * Hd + j], da);
        const float keep = mlp_keep(drop, b, j);
        const float hk = hidden_pre[(int64_t)b * Hd + j] * keep;
        const float dh = da * mlp_act_grad(act, hk) * keep;
        dhs[j] = dh;
        dh_ws[(int64_t)b * Hd + j] = dh;
        a_ws[(int64_t)b * Hd + j] = act_exact(act, hk);
    }
    __syncthreads();
    for (int c = tid; c < C; c += kBlock) {
        float s = 0.f;
#pragma unroll 8
        for (int j = 0; j < Hd; ++j) s = fmaf(dhs[j], W1[(int64_t)j * C + c], s);
        dpooled[(int64_t)b * lddp + c] = s;
    }
}

// Backward, launch 2 — one workgroup per weight row.  Workgroups 0..K-1: dW2[k, :] (+)= sum_b dlogits[b, k] a[b, :],
// db2[k] (+)= sum_b dlogits[b, k].  Workgroups K..K+Hd-1: dW1[j, :] (+)= sum_b dh[b, j] pooled[b, :], db1[j] (+)= sum_b
// dh[b, j].  The row's B coefficients are staged in LDS a tile of kMlpTile at a time; every sum runs over b in index order.
template <bool WT>
__global__ __launch_bounds__(kBlock) void head_mlp_bwd_weights_kernel(const float* __restrict__ pooled, int64_t ldp,
                                                                      const float* __restrict__ prob,
                                                                      const void* __restrict__ target, int mode,
                                                                      const float* __restrict__ gl, int B, int C, int Hd, int K,
                                                                      const float* __restrict__ dh_ws,
                                                                      const float* __restrict__ a_ws, float* __restrict__ dW1,
                                                                      float* __restrict__ db1, float* __restrict__ dW2,
                                                                      float* __restrict__ db2, int accumulate,
                                                                      const float* __restrict__ cw, const float* __restrict__ pw) {
    __shared__ float g[kMlpTile];
    const int blk = blockIdx.x, tid = threadIdx.x;
    const bool second = blk < K;            // a row of the second Linear (else of the first)
    const int r = second ? blk : blk - K;   // k or j
    float scale;
    if constexpr (WT) {
        __shared__ double wred[kBlock];
        scale = head_loss_scale(gl, mode, B, K, cw, target, wred);
    } else {
        scale = gl[0] / head_loss_denom(mode, B, K);
    }
    const float* X = second ? a_ws : pooled;
    const int64_t ldx = second ? (int64_t)Hd : ldp;
    const int n = second ? Hd : C;
    float* dW = second ? dW2 + (int64_t)r * Hd : dW1 + (int64_t)r * C;
    float* db = second ? db2 + r : db1 + r;
    float bias = 0.f;  // (thread 0, first column chunk)
    for (int c0 = 0; c0 < n; c0 += kBlock) {
        const int c = c0 + tid;
        float s = 0.f;
        for (int b0 = 0; b0 < B; b0 += kMlpTile) {
            const int nb = min(kMlpTile, B - b0);
            if (c0 == 0 || B > kMlpTile) {  // (one tile: staged once for every column chunk)
                __syncthreads();
                for (int i = tid; i < nb; i += kBlock)
                    g[i] = !second ? dh_ws[(int64_t)(b0 + i) * Hd + r]
                           : WT    ? dlogit(prob, target, mode, b0 + i, r, K, scale, cw, pw)
                                   : dlogit(prob, target, mode, b0 + i, r, K, scale);
                __syncthreads();
            }
            if (c < n) {
#pragma unroll 8
                for (int i = 0; i < nb; ++i) s = fmaf(g[i], X[(int64_t)(b0 + i) * ldx + c], s);
            }
            if (c0 == 0 && tid == 0)
                for (int i = 0; i < nb; ++i) bias += g[i];
        }
        if (c < n) dW[c] = accumulate ? dW[c] + s : s;
    }
    if (tid == 0) *db = accumulate ? *db + bias : bias;
}

// host-side checks shared by the three entries: 0, or the error code after set_error
static int mlp_check(const char* who, int mode, int act, int64_t B, int64_t C, int64_t Hd, int64_t K, int64_t ldp) {
    if (!(B > 0 && C > 0 && Hd > 0 && K > 0 && ldp >= C && B < (1ll << 31) && C < (1ll << 31) && B * K < (1ll << 30) &&
          B * Hd < (1ll << 30))) {
        set_error("%s: bad sizes", who);
        return GLASS_E_ARG;
    }
    if (!loss_mode_ok(mode)) {
        set_error("%s: unknown loss mode %d", who, mode);
        return GLASS_E_UNSUPPORTED;
    }
    if (!act_code_ok(act)) {
        set_error("%s: unknown activation code %d", who, act);
        return GLASS_E_UNSUPPORTED;
    }
    if (K > kMaxK) {
        set_error("%s: at most %d classes", who, kMaxK);
        return GLASS_E_UNSUPPORTED;
    }
    if (Hd > kMlpMaxHd) {
        set_error("%s: at most %d hidden units", who, kMlpMaxHd);
        return GLASS_E_UNSUPPORTED;
    }
    return 0;
}

static bool mlp_drop_ok(float p_drop, const uint64_t* rng) { return p_drop == 0.f || (p_drop > 0.f && p_drop < 1.f && rng); }

// dynamic LDS of the forward kernel: the hidden row, and the pooled row when it is staged (<= 4 KiB + 16 KiB)
static size_t mlp_fwd_lds(int64_t C, int64_t Hd, int* stage) {
    *stage = C <= kMlpStageC;
    return sizeof(float) * (size_t)(Hd + (*stage ? C : 0));
}

}  // namespace glass

using namespace glass;

static int mlp_weights_check(const char* who, int mode, const float* cw, const float* pw) {
    if (loss_weights_ok(mode, cw, pw)) return 0;
    set_error("%s: class_weight goes with cross-entropy, pos_weight with BCE, at most one of them", who);
    return GLASS_E_UNSUPPORTED;
}

extern "C" int glass_head_mlp_loss_fwd_w_f32(const float* pooled, int64_t ldp, const float* W1, const float* b1, const float* W2,
                                             const float* b2, const void* target, int mode, int act, float p_drop,
                                             const uint64_t* rng_state, uint64_t call_id, int64_t B, int64_t C, int64_t Hd,
                                             int64_t K, float* hidden_pre, float* logits, float* prob, float* loss,
                                             const float* class_weight, const float* pos_weight, void* stream) {
    GLASS_REQUIRE(pooled && W1 && b1 && W2 && b2 && target && hidden_pre && logits && prob && loss,
                  "head_mlp_loss_fwd: null pointer");
    GLASS_REQUIRE(mlp_drop_ok(p_drop, rng_state), "head_mlp_loss_fwd: dropout needs 0 <= p < 1 and the rng words");
    if (int rc = mlp_check("head_mlp_loss_fwd", mode, act, B, C, Hd, K, ldp)) return rc;
    if (int rc = mlp_weights_check("head_mlp_loss_fwd", mode, class_weight, pos_weight)) return rc;
    float* loss_rows = prob + B * K;  // prob holds B*K + B floats (as glass_head_loss_fwd_f32's)
    int stage;
    const size_t lds = mlp_fwd_lds(C, Hd, &stage);
    hipStream_t st = (hipStream_t)stream;
    if (class_weight || pos_weight) {
        hipLaunchKernelGGL((head_mlp_fwd_kernel<true, true>), dim3((unsigned)B), dim3(kBlock), lds, st, pooled, ldp, W1, b1, W2, b2,
                           target, mode, act, make_drop(p_drop, call_id, Hd), rng_state, (int)C, (int)Hd, (int)K, stage, hidden_pre,
                           logits, K, prob, loss_rows, class_weight, pos_weight);
        hipLaunchKernelGGL(head_mlp_loss_mean_w_kernel, dim3(1), dim3(kBlock), 0, st, loss_rows, (int)B,
                           head_loss_denom(mode, B, K), loss, class_weight, target, (int)K);
        return launch_status("glass_head_mlp_loss_fwd_w_f32");
    }
    hipLaunchKernelGGL((head_mlp_fwd_kernel<true, false>), dim3((unsigned)B), dim3(kBlock), lds, st, pooled, ldp, W1, b1, W2, b2, target,
                       mode, act, make_drop(p_drop, call_id, Hd), rng_state, (int)C, (int)Hd, (int)K, stage, hidden_pre, logits, K,
                       prob, loss_rows, (const float*)nullptr, (const float*)nullptr);
    hipLaunchKernelGGL(head_mlp_loss_mean_kernel, dim3(1), dim3(kBlock), 0, st, loss_rows, (int)B,
                       head_loss_denom(mode, B, K), loss);
    return launch_status("glass_head_mlp_loss_fwd_f32");
}

extern "C" int glass_head_mlp_loss_fwd_f32(const float* pooled, int64_t ldp, const float* W1, const float* b1, const float* W2,
                                           const float* b2, const void* target, int mode, int act, float p_drop,
                                           const uint64_t* rng_state, uint64_t call_id, int64_t B, int64_t C, int64_t Hd,
                                           int64_t K, float* hidden_pre, float* logits, float* prob, float* loss,
                                           void* stream) {
    return glass_head_mlp_loss_fwd_w_f32(pooled, ldp, W1, b1, W2, b2, target, mode, act, p_drop, rng_state, call_id, B, C, Hd, K,
                                         hidden_pre, logits, prob, loss, nullptr, nullptr, stream);
}

extern "C" int glass_head_mlp_loss_bwd_w_f32(const float* pooled, int64_t ldp, const float* W1, const float* W2,
                                             const float* hidden_pre, const float* prob, const void* target, int mode, int act,
                                             float p_drop, const uint64_t* rng_state, uint64_t call_id, const float* grad_loss,
                                             int64_t B, int64_t C, int64_t Hd, int64_t K, float* ws, float* dpooled, int64_t lddp,
                                             float* dW1, float* db1, float* dW2, float* db2, int accumulate,
                                             const float* class_weight, const float* pos_weight, void* stream) {
    GLASS_REQUIRE(pooled && W1 && W2 && hidden_pre && prob && target && grad_loss && ws && dpooled && dW1 && db1 && dW2 && db2,
                  "head_mlp_loss_bwd: null pointer");
    GLASS_REQUIRE(mlp_drop_ok(p_drop, rng_state), "head_mlp_loss_bwd: dropout needs 0 <= p < 1 and the rng words");
    if (int rc = mlp_check("head_mlp_loss_bwd", mode, act, B, C, Hd, K, ldp)) return rc;
    if (int rc = mlp_weights_check("head_mlp_loss_bwd", mode, class_weight, pos_weight)) return rc;
    GLASS_REQUIRE(lddp >= C, "head_mlp_loss_bwd: lddp < C");
    float* dh_ws = ws;            // [B, Hd]
    float* a_ws = ws + B * Hd;    // [B, Hd]
    hipStream_t st = (hipStream_t)stream;
    if (class_weight || pos_weight) {
        hipLaunchKernelGGL(head_mlp_bwd_rows_kernel<true>, dim3((unsigned)B), dim3(kBlock), 0, st, W1, W2, hidden_pre, prob, target,
                           mode, act, make_drop(p_drop, call_id, Hd), rng_state, grad_loss, (int)B, (int)C, (int)Hd, (int)K, dh_ws,
                           a_ws, dpooled, lddp, class_weight, pos_weight);
        hipLaunchKernelGGL(head_mlp_bwd_weights_kernel<true>, dim3((unsigned)(K + Hd)), dim3(kBlock), 0, st, pooled, ldp, prob,
                           target, mode, grad_loss, (int)B, (int)C, (int)Hd, (int)K, dh_ws, a_ws, dW1, db1, dW2, db2, accumulate,
                           class_weight, pos_weight);
        return launch_status("glass_head_mlp_loss_bwd_w_f32");
    }
    hipLaunchKernelGGL(head_mlp_bwd_rows_kernel<false>, dim3((unsigned)B), dim3(kBlock), 0, st, W1, W2, hidden_pre, prob, target, mode,
                       act, make_drop(p_drop, call_id, Hd), rng_state, grad_loss, (int)B, (int)C, (int)Hd, (int)K, dh_ws, a_ws,
                       dpooled, lddp, (const float*)nullptr, (const float*)nullptr);
    hipLaunchKernelGGL(head_mlp_bwd_weights_kernel<false>, dim3((unsigned)(K + Hd)), dim3(kBlock), 0, st, pooled, ldp, prob, target,
                       mode, grad_loss, (int)B, (int)C, (int)Hd, (int)K, dh_ws, a_ws, dW1, db1, dW2, db2, accumulate,
                       (const float*)nullptr, (const float*)nullptr);
    return launch_status("glass_head_mlp_loss_bwd_f32");
}

extern "C" int glass_head_mlp_loss_bwd_f32(const float* pooled, int64_t ldp, const float* W1, const float* W2,
                                           const float* hidden_pre, const float* prob, const void* target, int mode, int act,
                                           float p_drop, const uint64_t* rng_state, uint64_t call_id, const float* grad_loss,
                                           int64_t B, int64_t C, int64_t Hd, int64_t K, float* ws, float* dpooled, int64_t lddp,
                                           float* dW1, float* db1, float* dW2, float* db2, int accumulate, void* stream) {
    return glass_head_mlp_loss_bwd_w_f32(pooled, ldp, W1, W2, hidden_pre, prob, target, mode, act, p_drop, rng_state, call_id,
                                         grad_loss, B, C, Hd, K, ws, dpooled, lddp, dW1, db1, dW2, db2, accumulate, nullptr,
                                         nullptr, stream);
}

extern "C" int glass_head_mlp_f32(const float* pooled, int64_t ldp, const float* W1, const float* b1, const float* W2,
                                  const float* b2, int act, int64_t B, int64_t C, int64_t Hd, int64_t K, float* logits,
                                  int64_t ldl, void* stream) {
    GLASS_REQUIRE(pooled && W1 && b1 && W2 && b2 && logits, "head_mlp: null pointer");
    if (int rc = mlp_check("head_mlp", GLASS_LOSS_CE, act, B, C, Hd, K, ldp)) return rc;
    GLASS_REQUIRE(ldl >= K, "head_mlp: ldl < K");
    int stage;
    const size_t lds = mlp_fwd_lds(C, Hd, &stage);
    hipLaunchKernelGGL((head_mlp_fwd_kernel<false, false>), dim3((unsigned)B), dim3(kBlock), lds, (hipStream_t)stream, pooled, ldp, W1,
                       b1, W2, b2, (const void*)nullptr, GLASS_LOSS_CE, act, make_drop(0.f, 0, Hd), (const uint64_t*)nullptr, (int)C,
                       (int)Hd, (int)K, stage, (float*)nullptr, logits, ldl, (float*)nullptr, (float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr);
    return launch_status("glass_head_mlp_f32");
}
