// K9c  Gradient clipping by global L2 norm in front of the flat Adam launch (the optimizer of GLASSTest.py:213 with
// torch.nn.utils.clip_grad_norm_ between backward and step).  Two entries:
//   glass_grad_norm_f32       norm of the whole gradient arena + the clip coefficient, in device memory
//   glass_adam_step_clip_f32  glass_adam_step_f32 whose gradient is scaled by that coefficient on load (and stored back)
// The norm is bitwise repeatable and independent of the grid: the arena is cut into chunks of kNormChunk ELEMENTS — a fixed
// function of n — every chunk is summed by one workgroup in a fixed order (per-lane in index order, wave shuffles, LDS) in
// fp64, and a second one-workgroup launch folds the chunk partials in an order that depends on their count alone.  No float
// atomic, no ticket, no device-scope barrier: the hand-over between the two stages is the launch boundary.
#include "common.h"

namespace glass {

constexpr int kNormChunk = 8192;                       // elements per partial sum: 8 float4 per lane of a 256-lane workgroup
constexpr int kNormVecPerLane = kNormChunk / (4 * kBlock);
constexpr int kNormMaxBlocks = 1024;                   // 4 workgroups per CU; more chunks are strided over the grid
static_assert(kNormVecPerLane * 4 * kBlock == kNormChunk, "a chunk is whole float4 rounds of the workgroup");

// Sum of v over the workgroup in a fixed order: shuffle tree inside each wave, then the 4 wave sums in wave order.
// The result is valid on thread 0.
__device__ __forceinline__ double block_sum_f64(double v, double* lds) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < kBlock / kWave; ++w) s += lds[w];
    }
    __syncthreads();  // (lds is reused by the next chunk)
    return s;
}

// partials[c] = sum of squares of grad[c * kNormChunk .. min(n, (c + 1) * kNormChunk)).  Lane t takes the float4 pieces
// t, t + 256, .. of the chunk, elements in index order; VEC = false reads the same elements in the same order one by one
// (a base that is not 16-byte aligned), so both forms give the same bits.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void grad_sumsq_kernel(const float* __restrict__ grad, int64_t n, int64_t n_chunks,
                                                            double* __restrict__ partials) {
    __shared__ double lds[kBlock / kWave];
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int64_t base = c * kNormChunk;
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < kNormVecPerLane; ++j) {
            const int64_t k = base + 4 * ((int64_t)j * kBlock + threadIdx.x);
            float q[4] = {0.f, 0.f, 0.f, 0.f};
            if (VEC && k + 4 <= n) {
                const float4 v = *reinterpret_cast<const float4*>(grad + k);
                q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < n) q[e] = grad[k + e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc += (double)q[e] * (double)q[e];
        }
        const double s = block_sum_f64(acc, lds);
        if (threadIdx.x == 0) partials[c] = s;
    }
}

// One workgroup: lane t adds partials t, t + 256, .. in index order, then the workgroup's fixed tree.  out[0] = the norm
// rounded to fp32; out[1] = torch.nn.utils.clip_grad_norm_'s coefficient from that fp32 value, in fp32:
// clamp(max_norm / (norm + 1e-6), max = 1) — a NaN stays a NaN, as torch.clamp leaves it.
__global__ __launch_bounds__(kBlock) void grad_norm_finish_kernel(const double* __restrict__ partials, int64_t n_chunks,
                                                                  float max_norm, float* __restrict__ out) {
    __shared__ double lds[kBlock / kWave];
    double acc = 0.0;
    for (int64_t c = threadIdx.x; c < n_chunks; c += kBlock) acc += partials[c];
    const double total = block_sum_f64(acc, lds);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(total);
        const float coef = max_norm / (norm + 1e-6f);
        out[0] = norm;
        out[1] = coef > 1.f ? 1.f : coef;
    }
}

__global__ __launch_bounds__(kBlock) void adam_clip_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, int64_t n, const float* __restrict__ lr_dev,
                                                           float beta1, float beta2, float eps, float weight_decay,
                                                           int64_t* __restrict__ step_dev, const float* __restrict__ coef) {
    adam_arena_body<true>(p, g, m, v, n, lr_dev, beta1, beta2, eps, weight_decay, step_dev, coef);
}

}  // namespace glass

using namespace glass;

extern "C" int64_t glass_grad_norm_chunk(void) { return kNormChunk; }

extern "C" int glass_grad_norm_f32(const float* grad, int64_t n, double* partials, int64_t n_partials, float max_norm,
                                   float* out, void* stream) {
    GLASS_REQUIRE(grad && partials && out, "grad_norm: null pointer");
    GLASS_REQUIRE(n > 0, "grad_norm: n = %lld", (long long)n);
    const int64_t n_chunks = ceil_div(n, kNormChunk);
    GLASS_REQUIRE(n_partials >= n_chunks, "grad_norm: n_partials = %lld, %lld chunks of %d elements", (long long)n_partials,
                  (long long)n_chunks, kNormChunk);
    GLASS_REQUIRE(max_norm >= 0.f, "grad_norm: max_norm = %g (must be >= 0)", (double)max_norm);  // (false for a NaN too)
    GLASS_REQUIRE((reinterpret_cast<uintptr_t>(grad) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0 &&
                      (reinterpret_cast<uintptr_t>(partials) & 7u) == 0,
                  "grad_norm: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)(n_chunks < kNormMaxBlocks ? n_chunks : kNormMaxBlocks);
    if (aligned16(grad))
        hipLaunchKernelGGL(grad_sumsq_kernel<true>, dim3(blocks), dim3(kBlock), 0, st, grad, n, n_chunks, partials);
    else
        hipLaunchKernelGGL(grad_sumsq_kernel<false>, dim3(blocks), dim3(kBlock), 0, st, grad, n, n_chunks, partials);
    const int rc = launch_status("glass_grad_norm_f32 (chunk sums)");
    if (rc) return rc;
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(kBlock), 0, st, partials, n_chunks, max_norm, out);
    return launch_status("glass_grad_norm_f32");
}

extern "C" int glass_adam_step_clip_f32(float* param, float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                        const float* lr_dev, double beta1, double beta2, double eps, double weight_decay,
                                        int64_t* step_dev, const float* coef, void* stream) {
    GLASS_REQUIRE(param && grad && exp_avg && exp_avg_sq && lr_dev && step_dev && coef && n > 0, "adam_step_clip: bad arguments");
    hipLaunchKernelGGL(adam_clip_kernel, dim3(adam_arena_blocks(n)), dim3(kBlock), 0, (hipStream_t)stream, param, grad, exp_avg,
                       exp_avg_sq, n, lr_dev, (float)beta1, (float)beta2, (float)eps, (float)weight_decay, step_dev, coef);
    return launch_status("glass_adam_step_clip_f32");
}
