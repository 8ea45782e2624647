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

}  // namespace glass
