// The loss half shared by the two prediction heads (head.hip: bare nn.Linear; head_mlp.hip: two-layer MLP): the per-subgraph
// softmax / sigmoid and loss term, the ordered mean, and dlogits of the backward — ONE definition, so the heads cannot drift.
#pragma once
#include "common.h"

namespace glass {

constexpr int GLASS_LOSS_CE = 0;
constexpr int GLASS_LOSS_BCE = 1;

constexpr int kMaxK = 256;  // classes handled by the per-subgraph workgroup

inline bool loss_mode_ok(int mode) { return mode == GLASS_LOSS_CE || mode == GLASS_LOSS_BCE; }

// One lane finishes subgraph b from its K logits zs (LDS): writes logits[b, :] (row stride ldl) and prob[b, :] (softmax /
// sigmoid, kept for the backward) and returns the row's loss term — CrossEntropyLoss (GLASSTest.py:69) or BCEWithLogitsLoss
// on the flattened tensors (GLASSTest.py:57-58), before the mean.
__device__ __forceinline__ float head_loss_row(const float* zs, const void* __restrict__ target, int mode, int b, int K,
                                               float* __restrict__ logits, int64_t ldl, float* __restrict__ prob) {
    float term = 0.f;
    if (mode == GLASS_LOSS_CE) {
        float m = zs[0];
        for (int k = 1; k < K; ++k) m = fmaxf(m, zs[k]);
        float se = 0.f;
        for (int k = 0; k < K; ++k) se += expf(zs[k] - m);
        const float lse = m + logf(se);
        for (int k = 0; k < K; ++k) {
            logits[(int64_t)b * ldl + k] = zs[k];
            prob[(int64_t)b * K + k] = expf(zs[k] - lse);
        }
        const int64_t t = ((const int64_t*)target)[b];
        term = (t >= 0 && t < K) ? lse - zs[t] : 0.f;
    } else {
        const float* y = (const float*)target + (int64_t)b * K;
        for (int k = 0; k < K; ++k) {
            const float z = zs[k];
            logits[(int64_t)b * ldl + k] = z;
            prob[(int64_t)b * K + k] = 1.f / (1.f + expf(-z));
            // max(z,0) - z*y + log(1 + exp(-|z|))   (torch's stable BCE-with-logits)
            term += fmaxf(z, 0.f) - z * y[k] + log1pf(expf(-fabsf(z)));
        }
    }
    return term;
}

// loss[0] = (sum of the B row terms, in index order per thread, then a fixed tree) / denom — one workgroup of kBlock threads
// (deterministic; a float atomic would not be)
__device__ __forceinline__ void head_loss_mean(const float* __restrict__ loss_rows, int B, float denom, float* __restrict__ loss) {
    __shared__ double red[kBlock];
    double part = 0.0;
    for (int b = threadIdx.x; b < B; b += kBlock) part += (double)loss_rows[b];
    red[threadIdx.x] = part;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] / (double)denom);
}

__host__ __device__ inline float head_loss_denom(int mode, int64_t B, int64_t K) {
    return mode == GLASS_LOSS_CE ? (float)B : (float)B * (float)K;
}

// dlogits[b, k] = scale * (prob - target), scale = grad_loss / (B or B*K)
__device__ __forceinline__ float dlogit(const float* prob, const void* target, int mode, int64_t b, int k, int K, float scale) {
    const float p = prob[b * K + k];
    if (mode == GLASS_LOSS_CE) return scale * (p - (((const int64_t*)target)[b] == k ? 1.f : 0.f));
    return scale * (p - ((const float*)target)[b * K + k]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Weighted forms (torch's CrossEntropyLoss(weight=) / BCEWithLogitsLoss(pos_weight=), mean reduction).  cw: class weights
// [K] of cross-entropy, pw: pos_weight [K] of BCE-with-logits, one per output column; both nullable, at most one set.  The
// kernels are instantiated twice (WT): the instantiation the entries launch with two null pointers never sees these
// functions, so the unweighted launches keep their instruction stream.
//   CE   loss = sum_b w[t_b] (lse_b - z_b[t_b]) / sum_b w[t_b],   dlogits[b,k] = gl w[t_b] / sum_w (softmax_bk - [k = t_b]);
//        a target outside [0, K) adds nothing to either sum and has no gradient
//   BCE  c = 1 + (p_k - 1) y,  term = (1 - y) z + c (log1p(exp(-|z|)) + max(-z, 0)),  d/dz = c sigmoid(z) - p_k y,  mean over B*K
// ---------------------------------------------------------------------------------------------------------------------
inline bool loss_weights_ok(int mode, const float* cw, const float* pw) {
    return !(cw && pw) && !(cw && mode != GLASS_LOSS_CE) && !(pw && mode != GLASS_LOSS_BCE);
}

__device__ __forceinline__ float ce_class_weight(const float* __restrict__ cw, int64_t t, int K) {
    return (t >= 0 && t < K) ? cw[t] : 0.f;
}

__device__ __forceinline__ float bce_pw_term(float z, float y, float p) {
    const float c = 1.f + (p - 1.f) * y;
    return (1.f - y) * z + c * (log1pf(expf(-fabsf(z))) + fmaxf(-z, 0.f));
}

__device__ __forceinline__ float bce_pw_grad(float sig, float y, float p) { return (1.f + (p - 1.f) * y) * sig - p * y; }

// The cross-entropy denominator sum_b cw[target[b]] in fp64, by the whole workgroup of kBlock threads: thread t adds rows
// t, t + kBlock, ... in index order, then the fixed tree of head_loss_mean.  Every workgroup that needs it recomputes it
// (B loads; no launch, no float atomic, the same bits everywhere); returned on every thread.  red: kBlock doubles of LDS,
// free again on return.
__device__ __forceinline__ double ce_weight_sum(const float* __restrict__ cw, const int64_t* __restrict__ target, int B, int K,
                                                double* red) {
    double part = 0.0;
    for (int b = threadIdx.x; b < B; b += kBlock) part += (double)ce_class_weight(cw, target[b], K);
    red[threadIdx.x] = part;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double sum = red[0];
    __syncthreads();
    return sum;
}

// The same sum by ONE wave: lane l stands for threads l, l + 64, l + 128, l + 192 of the workgroup form and the adds follow
// its tree (steps 128 and 64 within the lane, 32 .. 1 across lanes), so the bits are the workgroup form's.
__device__ __forceinline__ double ce_weight_sum_wave(const float* __restrict__ cw, const int64_t* __restrict__ target, int B,
                                                     int K, int lane) {
    static_assert(kBlock == 4 * kWave, "four workgroup threads per lane");
    double p[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 4; ++u)
        for (int b = lane + kWave * u; b < B; b += kBlock) p[u] += (double)ce_class_weight(cw, target[b], K);
    double s = (p[0] + p[2]) + (p[1] + p[3]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

__device__ __forceinline__ float head_loss_row(const float* zs, const void* __restrict__ target, int mode, int b, int K,
                                               float* __restrict__ logits, int64_t ldl, float* __restrict__ prob,
                                               const float* __restrict__ cw, const float* __restrict__ pw) {
    if (mode == GLASS_LOSS_CE) {
        const float term = head_loss_row(zs, target, mode, b, K, logits, ldl, prob);
        return cw ? ce_class_weight(cw, ((const int64_t*)target)[b], K) * term : term;
    }
    if (!pw) return head_loss_row(zs, target, mode, b, K, logits, ldl, prob);
    const float* y = (const float*)target + (int64_t)b * K;
    float term = 0.f;
    for (int k = 0; k < K; ++k) {
        const float z = zs[k];
        logits[(int64_t)b * ldl + k] = z;
        prob[(int64_t)b * K + k] = 1.f / (1.f + expf(-z));
        term += bce_pw_term(z, y[k], pw[k]);
    }
    return term;
}

// the mean with the weighted cross-entropy's denominator (cw set: loss = sum of the weighted row terms / sum_b cw[t_b]);
// cw null: head_loss_mean's division by denom (BCE with pos_weight still averages over B*K)
__device__ __forceinline__ void head_loss_mean(const float* __restrict__ loss_rows, int B, float denom, float* __restrict__ loss,
                                               const float* __restrict__ cw, const void* __restrict__ target, int K) {
    __shared__ double red[kBlock];
    const double den = cw ? ce_weight_sum(cw, (const int64_t*)target, B, K, red) : (double)denom;
    double part = 0.0;
    for (int b = threadIdx.x; b < B; b += kBlock) part += (double)loss_rows[b];
    red[threadIdx.x] = part;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] / den);
}

// grad_loss / denominator of the backward kernels: the weighted cross-entropy's is the recomputed weight sum (all kBlock
// threads call this; red as ce_weight_sum's)
__device__ __forceinline__ float head_loss_scale(const float* __restrict__ gl, int mode, int B, int K, const float* __restrict__ cw,
                                                 const void* __restrict__ target, double* red) {
    if (!cw) return gl[0] / head_loss_denom(mode, B, K);
    return (float)((double)gl[0] / ce_weight_sum(cw, (const int64_t*)target, B, K, red));
}

// dlogits[b, k] of the weighted losses; scale = head_loss_scale's
__device__ __forceinline__ float dlogit(const float* prob, const void* target, int mode, int64_t b, int k, int K, float scale,
                                        const float* __restrict__ cw, const float* __restrict__ pw) {
    if (mode == GLASS_LOSS_CE) {
        if (!cw) return dlogit(prob, target, mode, b, k, K, scale);
        const int64_t t = ((const int64_t*)target)[b];
        return scale * ce_class_weight(cw, t, K) * (prob[b * K + k] - (t == k ? 1.f : 0.f));
    }
    if (!pw) return dlogit(prob, target, mode, b, k, K, scale);
    return scale * bce_pw_grad(prob[b * K + k], ((const float*)target)[b * K + k], pw[k]);
}

}  // namespace glass
