// K6r: GraphNorm (+ activation + inverted dropout) over R replicas of one graph: R segments of exactly N rows each, rows
// r*N .. r*N + N - 1 of a replica-major [R*N, ld] matrix, every segment normalised over its own rows (exact zero-one labels:
// models.EmbZGConv with z of shape [B, N]).  The per-graph kernels of graphnorm_seg.hip give a segment ONE workgroup, right
// for GNN-seg's tiny graphs; here a segment is a whole graph, so every replica gets the row blocking the whole-graph entry
// gives N rows, as one z plane of the grid.  The passes are the bodies glass_graphnorm_fwd_f32 / _bwd_f32 run (gn_kernels.h)
// and the coefficient math of gn_math.h on the same fixed-order fp64 partials, so replica r holds the bits of the
// whole-graph entry on its slice with call_id + ((uint64)(rep0 + r) << 32) as the dropout stream — a key made of the GLOBAL
// replica index, so that it does not matter how a caller cuts B replicas into launches.  The parameter gradients are sums
// over the replicas: each replica's finalize writes its three fp64 column sums, and a second, small launch folds them in
// ascending r (no float atomics; the scheme of gradclip.hip and graphnorm_seg.hip's fold).
#include "common.h"
#include "gn_kernels.h"

namespace glass {

constexpr int64_t kGnRepMaxGridZ = 65535;  // replicas per launch: the grid's z extent

// one replica's share of the workspace: the whole-graph entry's layout (partials, then 4*C floats of coefficients)
static int64_t rep_chunk_bytes(int64_t C) { return ws_partials_bytes(C) + 4 * C * (int64_t)sizeof(float); }

__device__ __forceinline__ Drop rep_drop(Drop d, int rep0) {
    d.call_id += (uint64_t)(rep0 + (int)blockIdx.z) << 32;
    return d;
}

template <int VW>
__global__ __launch_bounds__(kBlock) void gnr_stats_kernel(const float* __restrict__ x, int64_t ldx, int64_t N, int C,
                                                           int tc_log2, char* __restrict__ ws, int64_t chunk) {
    const int64_t r = blockIdx.z;
    gn_stats_body<VW>(x + r * N * ldx, ldx, N, C, tc_log2, reinterpret_cast<double*>(ws + r * chunk), 0);
}

// (gn_finalize_src_kernel of graphnorm.hip with one source, per replica)
__global__ __launch_bounds__(kBlock) void gnr_finalize_kernel(const char* __restrict__ ws, int64_t chunk, int nblk, int C,
                                                              int64_t N, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float* __restrict__ alpha,
                                                              float eps, float* __restrict__ saved_all) {
    __shared__ double lds[kBlock * 2];
    const int64_t r = blockIdx.z;
    const double* partial = reinterpret_cast<const double*>(ws + r * chunk);
    float* saved = saved_all + r * 4 * C;
    const int tc = threadIdx.x & (kFinCols - 1), tr = threadIdx.x / kFinCols;
    const int c = blockIdx.x * kFinCols + tc;
    const bool ok = c < C;
    double ss, qq;
    gn_sum_partials(ok ? partial : nullptr, nblk, C, ok ? c : 0, ok, tc, tr, lds, ss, qq);
    if (tr == 0 && ok)
        gn_fwd_coeffs(ss, qq, (double)N, gamma[c], beta[c], alpha[c], eps, saved[c], saved[C + c], saved[2 * C + c],
                      saved[3 * C + c]);
}

template <int VW>
__global__ __launch_bounds__(kBlock) void gnr_apply_kernel(const float* __restrict__ x, int64_t ldx, float* __restrict__ y,
                                                           int64_t ldy, int64_t N, int C, int tc_log2,
                                                           const float* __restrict__ saved, int act, Drop drop, int rep0,
                                                           const uint64_t* __restrict__ rng_state) {
    const int64_t r = blockIdx.z;
    gn_apply_body<VW>(x + r * N * ldx, ldx, y + r * N * ldy, ldy, N, C, tc_log2, saved + r * 4 * C, act, rep_drop(drop, rep0),
                      rng_state);
}

template <int VW>
__global__ __launch_bounds__(kBlock) void gnr_bwd_stats_kernel(const float* __restrict__ dy, int64_t lddy,
                                                               const float* __restrict__ x, int64_t ldx, int64_t N, int C,
                                                               int tc_log2, const float* __restrict__ saved,
                                                               const float* __restrict__ alpha, int act, Drop drop, int rep0,
                                                               const uint64_t* __restrict__ rng_state, char* __restrict__ ws,
                                                               int64_t chunk) {
    const int64_t r = blockIdx.z;
    gn_bwd_stats_body<VW>(dy + r * N * lddy, lddy, x + r * N * ldx, ldx, N, C, tc_log2, saved + r * 4 * C, alpha, act,
                          rep_drop(drop, rep0), rng_state, reinterpret_cast<double*>(ws + r * chunk));
}

// per replica: the coefficients of dx = A*g + Bx*x + K (what gn_finalize_bwd_block derives) and the replica's three fp64
// parameter-gradient terms psum[r][0..2][C] = (sum g*xhat, sum g, dalpha)
__global__ __launch_bounds__(kBlock) void gnr_finalize_bwd_kernel(char* __restrict__ ws, int64_t chunk, int64_t coef_off, int nblk, int C,
                                                                  int64_t N, const float* __restrict__ gamma,
                                                                  const float* __restrict__ alpha,
                                                                  const float* __restrict__ saved_all,
                                                                  double* __restrict__ psum) {
    __shared__ double lds[kBlock * 2];
    const int64_t r = blockIdx.z;
    const double* partial = reinterpret_cast<const double*>(ws + r * chunk);
    float* coef = reinterpret_cast<float*>(ws + r * chunk + coef_off);
    const float* saved = saved_all + r * 4 * C;
    const int tc = threadIdx.x & (kFinCols - 1), tr = threadIdx.x / kFinCols;
    const int c = blockIdx.x * kFinCols + tc;
    double s1, s2;
    gn_sum_partials(partial, nblk, C, c, c < C, tc, tr, lds, s1, s2);
    if (tr == 0 && c < C) {
        float da;
        gn_bwd_coeffs(s1, s2, (double)N, gamma[c], alpha[c], saved[c], saved[C + c], coef[c], coef[C + c], coef[2 * C + c], da);
        double* p = psum + r * 3 * C;
        p[c] = s2;
        p[C + c] = s1;
        p[2 * C + c] = (double)da;
    }
}

template <int VW>
__global__ __launch_bounds__(kBlock) void gnr_bwd_apply_kernel(const float* __restrict__ dy, int64_t lddy,
                                                               const float* __restrict__ x, int64_t ldx,
                                                               float* __restrict__ dx, int64_t lddx,
                                                               const float* __restrict__ addend, int64_t ldadd, int64_t N,
                                                               int C, int tc_log2, const float* __restrict__ saved,
                                                               const char* __restrict__ ws, int64_t chunk, int64_t coef_off, int act,
                                                               Drop drop, int rep0, const uint64_t* __restrict__ rng_state) {
    const int64_t r = blockIdx.z;
    const float* coef = reinterpret_cast<const float*>(ws + r * chunk + coef_off);
    gn_bwd_apply_body<VW>(dy + r * N * lddy, lddy, x + r * N * ldx, ldx, dx + r * N * lddx, lddx,
                          addend ? addend + r * N * ldadd : nullptr, ldadd, N, C, tc_log2, saved + r * 4 * C, coef, act,
                          rep_drop(drop, rep0), rng_state);
}

// parameter gradients: the replicas' terms summed in ascending r, one thread per (term, column)
__global__ __launch_bounds__(kBlock) void gnr_fold_kernel(const double* __restrict__ psum, int R, int C,
                                                          float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                          float* __restrict__ dalpha, int accumulate) {
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= 3 * C) return;
    double s = 0.0;
    for (int r = 0; r < R; ++r) s += psum[(int64_t)r * 3 * C + k];
    const int which = k / C, c = k - which * C;
    float* out = which == 0 ? dgamma : (which == 1 ? dbeta : dalpha);
    if (out) out[c] = (accumulate ? out[c] : 0.f) + (float)s;
}

static int rep_check(const char* what, int64_t n_rows, int64_t C, int64_t R, int64_t rep0) {
    GLASS_REQUIRE(n_rows > 0 && C > 0 && R >= 0 && rep0 >= 0 && rep0 + R <= (1ll << 31),
                  "%s: bad sizes N=%lld C=%lld R=%lld rep0=%lld", what, (long long)n_rows, (long long)C, (long long)R,
                  (long long)rep0);
    if (R > kGnRepMaxGridZ) {
        set_error("%s: %lld replicas in one launch, the grid takes %lld", what, (long long)R, (long long)kGnRepMaxGridZ);
        return GLASS_E_UNSUPPORTED;
    }
    return 0;
}

}  // namespace glass

using namespace glass;

extern "C" int64_t glass_graphnorm_rep_max_replicas(void) { return kGnRepMaxGridZ; }

extern "C" int64_t glass_graphnorm_rep_row_block(int64_t C, int vec) {
    if (C <= 0) return GLASS_E_ARG;
    const Tiling t = make_tiling(C, vec != 0 && C % 4 == 0);
    return (int64_t)t.rpb * kUnroll * 2;  // rows one statistics workgroup covers before a second one is started
}

extern "C" int64_t glass_graphnorm_rep_ws_bytes(int64_t n_rows, int64_t C, int64_t R) {
    (void)n_rows;
    if (C <= 0 || R < 0) return GLASS_E_ARG;
    return R * (rep_chunk_bytes(C) + 3 * C * (int64_t)sizeof(double));
}

extern "C" int glass_graphnorm_rep_fwd_f32(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t n_rows, int64_t C,
                                           int64_t R, int64_t rep0, const float* gamma, const float* beta,
                                           const float* alpha, float eps, float* saved, int act, float p_drop,
                                           const uint64_t* rng_state, uint64_t call_id, void* ws, void* stream) {
    GLASS_REQUIRE(x && y && gamma && beta && alpha && saved && ws, "graphnorm_rep_fwd: null pointer");
    GLASS_REQUIRE(ldx >= C && ldy >= C, "graphnorm_rep_fwd: bad leading dimension (C=%lld ldx=%lld ldy=%lld)", (long long)C,
                  (long long)ldx, (long long)ldy);
    if (int rc = rep_check("graphnorm_rep_fwd", n_rows, C, R, rep0)) return rc;
    GLASS_REQUIRE(p_drop >= 0.f && p_drop < 1.f && (p_drop == 0.f || rng_state), "graphnorm_rep_fwd: bad dropout args");
    GLASS_REQUIRE(act_code_ok(act), "graphnorm_rep_fwd: bad act %d", act);
    GLASS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "graphnorm_rep_fwd: misaligned ws (8 bytes)");
    if (R == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && aligned16(x) && aligned16(y);
    const Tiling t = make_tiling(C, vec);
    const int nblk = stat_blocks(n_rows, t);
    const int64_t chunk = rep_chunk_bytes(C);
    const Drop drop = make_drop(p_drop, call_id, C);
    const unsigned Rz = (unsigned)R;
    dim3 gs(nblk, t.ctiles, Rz), ga(apply_blocks(n_rows, t), t.ctiles, Rz);
    if (vec) {
        hipLaunchKernelGGL(gnr_stats_kernel<4>, gs, dim3(kBlock), 0, st, x, ldx, n_rows, (int)C, t.tc_log2, (char*)ws, chunk);
    } else {
        hipLaunchKernelGGL(gnr_stats_kernel<1>, gs, dim3(kBlock), 0, st, x, ldx, n_rows, (int)C, t.tc_log2, (char*)ws, chunk);
    }
    hipLaunchKernelGGL(gnr_finalize_kernel, dim3((unsigned)ceil_div(C, kFinCols), 1, Rz), dim3(kBlock), 0, st, (const char*)ws,
                       chunk, nblk, (int)C, n_rows, gamma, beta, alpha, eps, saved);
    if (vec) {
        hipLaunchKernelGGL(gnr_apply_kernel<4>, ga, dim3(kBlock), 0, st, x, ldx, y, ldy, n_rows, (int)C, t.tc_log2, saved, act,
                           drop, (int)rep0, rng_state);
    } else {
        hipLaunchKernelGGL(gnr_apply_kernel<1>, ga, dim3(kBlock), 0, st, x, ldx, y, ldy, n_rows, (int)C, t.tc_log2, saved, act,
                           drop, (int)rep0, rng_state);
    }
    return launch_status("glass_graphnorm_rep_fwd_f32");
}

extern "C" int glass_graphnorm_rep_bwd_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, float* dx,
                                           int64_t lddx, const float* addend, int64_t ldadd, int64_t n_rows, int64_t C,
                                           int64_t R, int64_t rep0, const float* gamma, const float* alpha,
                                           const float* saved, float* dgamma, float* dbeta, float* dalpha, int accumulate,
                                           int act, float p_drop, const uint64_t* rng_state, uint64_t call_id, void* ws,
                                           void* stream) {
    GLASS_REQUIRE(dy && x && dx && gamma && alpha && saved && ws, "graphnorm_rep_bwd: null pointer");
    GLASS_REQUIRE(lddy >= C && ldx >= C && lddx >= C && (!addend || ldadd >= C), "graphnorm_rep_bwd: bad leading dimension");
    if (int rc = rep_check("graphnorm_rep_bwd", n_rows, C, R, rep0)) return rc;
    GLASS_REQUIRE(p_drop >= 0.f && p_drop < 1.f && (p_drop == 0.f || rng_state), "graphnorm_rep_bwd: bad dropout args");
    GLASS_REQUIRE(act_code_ok(act), "graphnorm_rep_bwd: bad act %d", act);
    GLASS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 7u) == 0, "graphnorm_rep_bwd: misaligned ws (8 bytes)");
    hipStream_t st = (hipStream_t)stream;
    const int64_t chunk = rep_chunk_bytes(C);
    double* psum = reinterpret_cast<double*>((char*)ws + R * chunk);
    const unsigned fold_blocks = (unsigned)ceil_div(3 * C, kBlock);
    if (R == 0) {  // no replica: the sums are zero (the buffers keep their value with `accumulate`)
        if (!accumulate && (dgamma || dbeta || dalpha))
            hipLaunchKernelGGL(gnr_fold_kernel, dim3(fold_blocks), dim3(kBlock), 0, st, psum, 0, (int)C, dgamma, dbeta, dalpha, 0);
        return launch_status("glass_graphnorm_rep_bwd_f32");
    }
    const bool vec = C % 4 == 0 && lddy % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0 && aligned16(dy) && aligned16(x) &&
                     aligned16(dx) && (!addend || (ldadd % 4 == 0 && aligned16(addend)));
    const Tiling t = make_tiling(C, vec);
    const int nblk = stat_blocks(n_rows, t);
    const Drop drop = make_drop(p_drop, call_id, C);
    const unsigned Rz = (unsigned)R;
    dim3 gs(nblk, t.ctiles, Rz), ga(apply_blocks(n_rows, t), t.ctiles, Rz);
    if (vec) {
        hipLaunchKernelGGL(gnr_bwd_stats_kernel<4>, gs, dim3(kBlock), 0, st, dy, lddy, x, ldx, n_rows, (int)C, t.tc_log2, saved,
                           alpha, act, drop, (int)rep0, rng_state, (char*)ws, chunk);
    } else {
        hipLaunchKernelGGL(gnr_bwd_stats_kernel<1>, gs, dim3(kBlock), 0, st, dy, lddy, x, ldx, n_rows, (int)C, t.tc_log2, saved,
                           alpha, act, drop, (int)rep0, rng_state, (char*)ws, chunk);
    }
    hipLaunchKernelGGL(gnr_finalize_bwd_kernel, dim3((unsigned)ceil_div(C, kFinCols), 1, Rz), dim3(kBlock), 0, st, (char*)ws,
                       chunk, ws_partials_bytes(C), nblk, (int)C, n_rows, gamma, alpha, saved, psum);
    if (dgamma || dbeta || dalpha)
        hipLaunchKernelGGL(gnr_fold_kernel, dim3(fold_blocks), dim3(kBlock), 0, st, psum, (int)R, (int)C, dgamma, dbeta, dalpha,
                           accumulate);
    if (vec) {
        hipLaunchKernelGGL(gnr_bwd_apply_kernel<4>, ga, dim3(kBlock), 0, st, dy, lddy, x, ldx, dx, lddx, addend, ldadd, n_rows,
                           (int)C, t.tc_log2, saved, (const char*)ws, chunk, ws_partials_bytes(C), act, drop, (int)rep0, rng_state);
    } else {
        hipLaunchKernelGGL(gnr_bwd_apply_kernel<1>, ga, dim3(kBlock), 0, st, dy, lddy, x, ldx, dx, lddx, addend, ldadd, n_rows,
                           (int)C, t.tc_log2, saved, (const char*)ws, chunk, ws_partials_bytes(C), act, drop, (int)rep0, rng_state);
    }
    return launch_status("glass_graphnorm_rep_bwd_f32");
}
