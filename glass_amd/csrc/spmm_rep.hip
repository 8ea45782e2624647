// K1r: the aggregation over R replicas of one graph in one launch, Y[r] = A @ X[r] (exact zero-one labels: every subgraph
// of a batch runs on its own copy of the activations, models.EmbZGConv with z of shape [B, N]).  The CSR, the plan blob and
// the plan's item lists exist ONCE; the replica is the grid's z plane, which only moves the X / Y / partial-row base
// pointers (in rows: x_rep_stride, y_rep_stride; partial rows: the plan's slot count per replica).  Everything a workgroup
// computes comes from the bodies glass_spmm_csr_f32 runs (spmm_sweep.h, spmm_common.h), and the host picks the same
// build (vector width, lanes per row, flat / row-only sweep) from the same header words, so replica r holds the bits
// glass_spmm_csr_f32 gives on that replica's slice.
#include "common.h"
#include "spmm_sweep.h"

namespace glass {

constexpr int64_t kRepMaxGridZ = 65535;         // replicas per launch: the grid's z extent
constexpr int64_t kRepMaxExtent = 1ll << 47;    // bytes a replicated operand may span (the device's virtual address range)

struct RepStride {
    int64_t x, y, ws;  // floats from one replica's X / Y / partial rows to the next
};

template <int VW, int LPR, int U, bool NT>
__global__ __launch_bounds__(kBlock) void spmm_rep_long_kernel(const int32_t* __restrict__ col, const float* __restrict__ val,
                                                               const float* __restrict__ X, int64_t ldx,
                                                               float* __restrict__ Y, int64_t ldy,
                                                               float* __restrict__ partials, int H,
                                                               const int32_t* __restrict__ items, RepStride rs) {
    __shared__ float lds[(kBlock / kWave) * LPR * VW];
    const int64_t r = blockIdx.z;
    long_item_body<VW, LPR, U, NT>(col, val, X + r * rs.x, ldx, Y + r * rs.y, ldy, partials + r * rs.ws, H,
                                   items + 4 * (int64_t)blockIdx.x, lds);
}

template <int VW, int LPR, int U, bool NT, bool FLAT>
__global__ GLASS_K1_SWEEP_BOUNDS void spmm_rep_sweep_kernel(const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ col,
                                                            const float* __restrict__ val,
                                                            const float* __restrict__ X, int64_t ldx,
                                                            float* __restrict__ Y, int64_t ldy, int H,
                                                            const int32_t* __restrict__ items, int n_waves,
                                                            int rp_factor, const int32_t* __restrict__ long_items,
                                                            int n_sweep_blocks, float* __restrict__ partials, RepStride rs) {
    const int64_t r = blockIdx.z;
    spmm_sweep_body<VW, LPR, U, NT, FLAT>(rowptr, col, val, X + r * rs.x, ldx, Y + r * rs.y, ldy, H, items, n_waves,
                                          rp_factor, long_items, n_sweep_blocks, partials + r * rs.ws);
}

__global__ __launch_bounds__(kBlock) void spmm_rep_reduce_kernel(const float* __restrict__ partials, float* __restrict__ Y,
                                                                 int64_t ldy, int H, const int32_t* __restrict__ rrows,
                                                                 RepStride rs) {
    const int64_t r = blockIdx.z;
    spmm_reduce_body(partials + r * rs.ws, Y + r * rs.y, ldy, H, rrows);
}

// (the launch sequence of spmm.hip's launch_spmm_u, every grid with R planes)
template <int VW, int LPR, int U, bool NT>
static int launch_rep_u(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx, float* Y,
                        int64_t ldy, int64_t H, const int32_t* hdr, const int32_t* plan, float* ws, RepStride rs, int R,
                        hipStream_t st) {
    const int n_ctiles = (int)ceil_div(H, (int64_t)LPR * VW);
    const int n_waves = hdr[H_NSWEEP];
    if (n_waves > 0) {
        const int n_sweep_blocks = (int)ceil_div(n_waves, kBlock / kWave);
        dim3 grid((unsigned)(n_sweep_blocks + hdr[H_NLONG]), n_ctiles, R);
        if (spmm_sweep_flat(hdr, kWave / LPR))
            hipLaunchKernelGGL((spmm_rep_sweep_kernel<VW, LPR, U, NT, true>), grid, dim3(kBlock), 0, st, rowptr, col, val, X,
                               ldx, Y, ldy, (int)H, plan + hdr[H_OFF_SWEEP], n_waves, hdr[H_RP_FACTOR],
                               plan + hdr[H_OFF_LONG], n_sweep_blocks, ws, rs);
        else
            hipLaunchKernelGGL((spmm_rep_sweep_kernel<VW, LPR, U, NT, false>), grid, dim3(kBlock), 0, st, rowptr, col, val, X,
                               ldx, Y, ldy, (int)H, plan + hdr[H_OFF_SWEEP], n_waves, 0, plan + hdr[H_OFF_LONG],
                               n_sweep_blocks, ws, rs);
    } else if (hdr[H_NLONG] > 0) {
        dim3 grid((unsigned)hdr[H_NLONG], n_ctiles, R);
        hipLaunchKernelGGL((spmm_rep_long_kernel<VW, LPR, U, NT>), grid, dim3(kBlock), 0, st, col, val, X, ldx, Y, ldy, ws,
                           (int)H, plan + hdr[H_OFF_LONG], rs);
    }
    if (hdr[H_NREDUCE] > 0) {
        hipLaunchKernelGGL(spmm_rep_reduce_kernel, dim3((unsigned)hdr[H_NREDUCE], 1, R), dim3(kBlock), 0, st, ws, Y, ldy,
                           (int)H, plan + hdr[H_OFF_REDUCE], rs);
    }
    return launch_status("glass_spmm_csr_rep_f32");
}

template <int VW, int LPR>
static int launch_rep(const int32_t* rowptr, const int32_t* col, const float* val, const float* X, int64_t ldx, float* Y,
                      int64_t ldy, int64_t H, const int32_t* hdr, const int32_t* plan, float* ws, RepStride rs, int R,
                      hipStream_t st) {
    // the once-read streams of ALL replicas against the Infinity Cache (a cache policy only: the bits do not depend on it)
    const int64_t streamed = (int64_t)hdr[H_NNZ] * 8 + (int64_t)R * hdr[H_NROWS] * (4 * H + 4);
    if (streamed > kStreamNtBytes)
        return launch_rep_u<VW, LPR, kGathers, true>(rowptr, col, val, X, ldx, Y, ldy, H, hdr, plan, ws, rs, R, st);
    return launch_rep_u<VW, LPR, kGathers, false>(rowptr, col, val, X, ldx, Y, ldy, H, hdr, plan, ws, rs, R, st);
}

}  // namespace glass

using namespace glass;

extern "C" int64_t glass_spmm_rep_max_replicas(void) { return kRepMaxGridZ; }

extern "C" int64_t glass_spmm_rep_ws_bytes(const int32_t* hdr, int64_t H, int64_t R) {
    if (!hdr || hdr[H_MAGIC] != kPlanMagic) return GLASS_E_PLAN;
    if (H <= 0 || R < 0) return GLASS_E_ARG;
    return R * (int64_t)hdr[H_NSLOTS] * H * (int64_t)sizeof(float);
}

extern "C" int glass_spmm_csr_rep_f32(const int32_t* rowptr, const int32_t* col, const float* val, const float* X,
                                      int64_t ldx, int64_t x_rep_stride, float* Y, int64_t ldy, int64_t y_rep_stride,
                                      int64_t n_rows, int64_t H, int64_t R, const int32_t* hdr, const int32_t* plan_dev,
                                      void* ws, void* stream) {
    GLASS_REQUIRE(rowptr && X && Y && hdr && plan_dev, "spmm_rep: null pointer");
    GLASS_REQUIRE(H > 0 && ldx >= H && ldy >= H, "spmm_rep: need H>0, ldx>=H, ldy>=H (H=%lld ldx=%lld ldy=%lld)",
                  (long long)H, (long long)ldx, (long long)ldy);
    GLASS_REQUIRE(R >= 0 && n_rows >= 0 && x_rep_stride >= 0 && y_rep_stride >= n_rows,
                  "spmm_rep: need R >= 0, x_rep_stride >= 0, y_rep_stride >= n_rows (R=%lld strides %lld, %lld rows)",
                  (long long)R, (long long)x_rep_stride, (long long)y_rep_stride);
    if (hdr[H_MAGIC] != kPlanMagic || hdr[H_VER] != kPlanVersion || hdr[H_NROWS] != n_rows) {
        set_error("spmm_rep: plan does not match (magic %x, rows %d vs %lld)", hdr[H_MAGIC], hdr[H_NROWS], (long long)n_rows);
        return GLASS_E_PLAN;
    }
    GLASS_REQUIRE(hdr[H_NNZ] == 0 || (col && val), "spmm_rep: null col/val");
    GLASS_REQUIRE(hdr[H_NSLOTS] == 0 || ws, "spmm_rep: plan needs %d partial rows per replica but ws is null", hdr[H_NSLOTS]);
    if (R > kRepMaxGridZ) {
        set_error("spmm_rep: %lld replicas in one launch, the grid takes %lld", (long long)R, (long long)kRepMaxGridZ);
        return GLASS_E_UNSUPPORTED;
    }
    const int64_t row_bytes = 4 * (ldx > ldy ? ldx : ldy);
    const int64_t stride = x_rep_stride > y_rep_stride ? x_rep_stride : y_rep_stride;
    if (R > 0 && stride > 0 && (stride > kRepMaxExtent / row_bytes || R > kRepMaxExtent / (stride * row_bytes))) {
        set_error("spmm_rep: %lld replicas of %lld rows of %lld bytes span more than the %lld bytes an operand may",
                  (long long)R, (long long)stride, (long long)row_bytes, (long long)kRepMaxExtent);
        return GLASS_E_UNSUPPORTED;
    }
    if (n_rows == 0 || R == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    float* wsf = (float*)ws;
    const RepStride rs = {x_rep_stride * ldx, y_rep_stride * ldy, (int64_t)hdr[H_NSLOTS] * H};
    // 16-byte accesses need every replica's base aligned: the strides in floats must be multiples of 4 (they are whenever
    // ldx / ldy are, which the vector form already asks for); the slice call decides from the same words
    const bool vec = (H % 4 == 0) && (ldx % 4 == 0) && (ldy % 4 == 0) && aligned16(X) && aligned16(Y) &&
                     (hdr[H_NSLOTS] == 0 || aligned16(ws));
#define GLASS_SPMM_REP_CASE(VW, LPR) \
    return launch_rep<VW, LPR>(rowptr, col, val, X, ldx, Y, ldy, H, hdr, plan_dev, wsf, rs, (int)R, st)
    GLASS_K1_WIDTH_DISPATCH(vec, H, GLASS_SPMM_REP_CASE);
#undef GLASS_SPMM_REP_CASE
}
