// What the single-head attention kernels (spmm_gat.hip) and the multi-head ones (spmm_gat_mh.hip) share: the gathers in
// flight per pass, the score of one entry and the two per-lane accumulators of the item walk.
#pragma once
#include "spmm_items.h"

namespace glass {

constexpr int kGatFwdGathers = kGathers;  // U of the forward: one row and one score per entry in flight, as K1
constexpr int kGatEdgeGathers = 4;        // U of the edge pass: one row per entry, the row's dY beside it
constexpr int kGatBwdGathers = 4;         // U of the transposed pass: one row and three scalars per entry
constexpr int kScoreRows = kBlock / kWave;  // node scores: one wave per row

// the score of one entry from its source's a and its destination's b, the same bits in all three passes
__device__ __forceinline__ float gat_score(float a, float b, float slope) {
    const float u = __fadd_rn(a, b);
    return u > 0.f ? u : __fmul_rn(slope, u);
}
__device__ __forceinline__ float gat_slope_of(float a, float b, float slope) { return __fadd_rn(a, b) > 0.f ? 1.f : slope; }

// ---- the forward's state: one online-softmax pair (M, Z), the same on every lane of a row, and VW running sums ---------------
template <int VW>
struct GatAcc {
    float m, z, s[VW];
    static constexpr int kLdsWords = VW + 2;
    __device__ __forceinline__ void init() {
        m = -INFINITY;
        z = 0.f;
#pragma unroll
        for (int k = 0; k < VW; ++k) s[k] = 0.f;
    }
    // one entry with weight v > 0, score sc (finite), message row x: ONE exponential, exp(-|sc - M|), which rescales either
    // the running sums or the entry (SmTriple's rule)
    __device__ __forceinline__ void take(bool ok, float v, float sc, const float (&x)[VW]) {
        const float d = sc - m;  // +inf on the first entry: e = 0, the empty sums are dropped
        const float e = expf(-fabsf(d));
        const bool up = d > 0.f;
        const float f = up ? e : 1.f;
        const float w = up ? v : v * e;
        const float zn = fmaf(z, f, w);
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            const float sn = fmaf(s[k], f, w * x[k]);
            s[k] = ok ? sn : s[k];
        }
        m = (ok && up) ? sc : m;
        z = ok ? zn : z;
    }
    // another partial of the same row (either may be empty: m = -inf, z = s = 0)
    __device__ __forceinline__ void merge(float om, float oz, const float (&os)[VW]) {
        const float nm = fmaxf(m, om);
        const float a = (m == nm) ? 1.f : expf(m - nm);
        const float b = (om == nm) ? 1.f : expf(om - nm);
        z = fmaf(z, a, oz * b);
#pragma unroll
        for (int k = 0; k < VW; ++k) s[k] = fmaf(s[k], a, os[k] * b);
        m = nm;
    }
    __device__ __forceinline__ void xor_merge(int sh) {
        const float om = __shfl_xor(m, sh), oz = __shfl_xor(z, sh);
        float os[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) os[k] = __shfl_xor(s[k], sh);
        merge(om, oz, os);
    }
    __device__ __forceinline__ void to_lds(int32_t* p) const {
        p[0] = __float_as_int(m);
        p[1] = __float_as_int(z);
#pragma unroll
        for (int k = 0; k < VW; ++k) p[2 + k] = __float_as_int(s[k]);
    }
    __device__ __forceinline__ void from_lds(const int32_t* p) {
        m = __int_as_float(p[0]);
        z = __int_as_float(p[1]);
#pragma unroll
        for (int k = 0; k < VW; ++k) s[k] = __int_as_float(p[2 + k]);
    }
    __device__ __forceinline__ void merge_lds(const int32_t* p) {
        float os[VW];
#pragma unroll
        for (int k = 0; k < VW; ++k) os[k] = __int_as_float(p[2 + k]);
        merge(__int_as_float(p[0]), __int_as_float(p[1]), os);
    }
};

// rows cut into several chunks, forward: their partials merged slot by slot (a template only for its linkage: this header is
// included by several translation units)
template <int = 0>
__global__ __launch_bounds__(kBlock) void spmm_gat_reduce_kernel(const float* __restrict__ ps, const float* __restrict__ pm,
                                                                 const float* __restrict__ pz, float* __restrict__ Y,
                                                                 int64_t ldy, float* __restrict__ L, int H,
                                                                 const int32_t* __restrict__ rrows) {
    const int32_t* rr = rrows + 3 * (int64_t)blockIdx.x;
    const int row = rr[0], first = rr[1], n = rr[2];
    for (int c = threadIdx.x; c < H; c += kBlock) {
        GatAcc<1> p;
        p.init();
        for (int k = 0; k < n; ++k) {
            const float os[1] = {ps[(int64_t)(first + k) * H + c]};
            p.merge(pm[first + k], pz[first + k], os);
        }
        const bool any = p.z > 0.f;
        Y[(int64_t)row * ldy + c] = any ? p.s[0] / p.z : 0.f;
        if (c == 0) L[row] = any ? p.m + logf(p.z) : 0.f;
    }
}

// ---- the transposed pass's state: da's partial sum beside VW running sums ---------------------------------------------------
template <int VW>
struct GatBwdAcc {
    float da, s[VW];
    static constexpr int kLdsWords = VW + 1;
    __device__ __forceinline__ void init() {
        da = 0.f;
#pragma unroll
        for (int k = 0; k < VW; ++k) s[k] = 0.f;
    }
    __device__ __forceinline__ void xor_merge(int sh) {
        da += __shfl_xor(da, sh);
#pragma unroll
        for (int k = 0; k < VW; ++k) s[k] += __shfl_xor(s[k], sh);
    }
    __device__ __forceinline__ void to_lds(int32_t* p) const {
        p[0] = __float_as_int(da);
#pragma unroll
        for (int k = 0; k < VW; ++k) p[1 + k] = __float_as_int(s[k]);
    }
    __device__ __forceinline__ void from_lds(const int32_t* p) {
        da = __int_as_float(p[0]);
#pragma unroll
        for (int k = 0; k < VW; ++k) s[k] = __int_as_float(p[1 + k]);
    }
    __device__ __forceinline__ void merge_lds(const int32_t* p) {
        da += __int_as_float(p[0]);
#pragma unroll
        for (int k = 0; k < VW; ++k) s[k] += __int_as_float(p[1 + k]);
    }
};

}  // namespace glass
