// Library-wide pieces of the C ABI: version + per-thread error string; host-side validation of the K10 entries.
#include <stdarg.h>
#include <stdio.h>

#include "../../include/glass_hip.h"

namespace glass {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

}  // namespace glass

extern "C" int glass_version(void) { return GLASS_ABI_VERSION; }

extern "C" const char* glass_last_error_string(void) { return glass::g_err; }

// ---- K10  GNN-seg extraction and collate: host-side validation, then the launches in seg.hip ----------------------
namespace glass {
int seg_extract_count_launch(const int32_t*, const int32_t*, const float*, const int32_t*, const int32_t*, const int32_t*,
                             const int32_t*, int64_t, int, int32_t*, int32_t*, float*, void*);
int seg_extract_fill_launch(const int32_t*, const int32_t*, const float*, const int32_t*, const int32_t*, const float*,
                            const int32_t*, const int32_t*, int64_t, int, const float*, const int32_t*, const int32_t*,
                            int32_t*, float*, int32_t*, float*, void*);
int seg_collate_launch(const int32_t*, const int32_t*, int64_t, const int32_t*, const int32_t*, const float*,
                       const int32_t*, const int32_t*, const float*, const int32_t*, int64_t, const int32_t*,
                       const int32_t*, const int32_t*, int32_t*, float*, int32_t*, float*, int32_t*, int64_t*, int64_t,
                       void*);
int seg_khop_launch(const int32_t*, const int32_t*, int64_t, const int32_t*, const int32_t*, int64_t, int, void*, bool,
                    int32_t*, const int32_t*, int32_t*, void*);
int seg_centre_index_launch(const int32_t*, const int32_t*, int64_t, const int32_t*, const int32_t*, int32_t*, void*);
int seg_collate_centre_launch(const int32_t*, const int32_t*, int64_t, const int32_t*, const int32_t*, const float*,
                              const int32_t*, const int32_t*, const float*, const int32_t*, const int32_t*,
                              const int32_t*, int64_t, const int32_t*, const int32_t*, const int32_t*, int32_t*, float*,
                              int32_t*, float*, int32_t*, int64_t*, int64_t, uint8_t*, void*);
}  // namespace glass

#define SEG_REQUIRE(cond, ...)             \
    do {                                   \
        if (!(cond)) {                     \
            glass::set_error(__VA_ARGS__); \
            return GLASS_E_ARG;            \
        }                                  \
    } while (0)

static int seg_check_inputs(const char* what, const int32_t* in_rowptr, const int32_t* in_col, const float* in_w,
                            const int32_t* out_rowptr, const int32_t* out_col, int64_t n_base, const int32_t* sub_ptr,
                            const int32_t* sub_nodes, int64_t n_sub, int64_t n_member, int mode) {
    if (mode != GLASS_SEG_GCN && mode != GLASS_SEG_GIN) {
        glass::set_error("%s: unknown mode %d (0=gcn, 1=gin)", what, mode);
        return GLASS_E_UNSUPPORTED;
    }
    SEG_REQUIRE(n_base >= 0 && n_base < INT32_MAX && n_sub >= 0 && n_sub < INT32_MAX && n_member >= 0 &&
                    n_member < INT32_MAX, "%s: negative or too large size", what);
    SEG_REQUIRE(in_rowptr && out_rowptr && sub_ptr, "%s: null pointer", what);
    SEG_REQUIRE(n_member == 0 || (sub_nodes && in_col && out_col), "%s: null pointer", what);
    SEG_REQUIRE(mode != GLASS_SEG_GCN || n_member == 0 || in_w, "%s: mode gcn needs the edge weights", what);
    return 0;
}

extern "C" int glass_seg_extract_count(const int32_t* in_rowptr, const int32_t* in_col, const float* in_w,
                                       const int32_t* out_rowptr, const int32_t* out_col, int64_t n_base,
                                       const int32_t* sub_ptr, const int32_t* sub_nodes, int64_t n_sub,
                                       int64_t n_member, int mode, int32_t* cnt_in, int32_t* cnt_out, float* deg,
                                       void* stream) {
    int rc = seg_check_inputs("seg_extract_count", in_rowptr, in_col, in_w, out_rowptr, out_col, n_base, sub_ptr,
                              sub_nodes, n_sub, n_member, mode);
    if (rc) return rc;
    SEG_REQUIRE(n_member == 0 || (cnt_in && cnt_out), "seg_extract_count: null count array");
    SEG_REQUIRE(mode != GLASS_SEG_GCN || n_member == 0 || deg, "seg_extract_count: mode gcn needs deg");
    return glass::seg_extract_count_launch(in_rowptr, in_col, in_w, out_rowptr, out_col, sub_ptr, sub_nodes, n_sub, mode,
                                           cnt_in, cnt_out, deg, stream);
}

extern "C" int glass_seg_extract_fill(const int32_t* in_rowptr, const int32_t* in_col, const float* in_w,
                                      const int32_t* out_rowptr, const int32_t* out_col, const float* out_w,
                                      int64_t n_base, const int32_t* sub_ptr, const int32_t* sub_nodes, int64_t n_sub,
                                      int64_t n_member, int mode, const float* deg, const int32_t* rowptr_in,
                                      const int32_t* rowptr_out, int32_t* col_in, float* val_in, int32_t* col_out,
                                      float* val_out, void* stream) {
    int rc = seg_check_inputs("seg_extract_fill", in_rowptr, in_col, in_w, out_rowptr, out_col, n_base, sub_ptr,
                              sub_nodes, n_sub, n_member, mode);
    if (rc) return rc;
    SEG_REQUIRE(mode != GLASS_SEG_GCN || n_member == 0 || (out_w && deg), "seg_extract_fill: mode gcn needs out_w and deg");
    SEG_REQUIRE(n_member == 0 || (rowptr_in && rowptr_out && col_in && val_in && col_out && val_out),
                "seg_extract_fill: null output pointer");
    return glass::seg_extract_fill_launch(in_rowptr, in_col, in_w, out_rowptr, out_col, out_w, sub_ptr, sub_nodes, n_sub,
                                          mode, deg, rowptr_in, rowptr_out, col_in, val_in, col_out, val_out, stream);
}

extern "C" int glass_seg_collate(const int32_t* sub_ptr, const int32_t* sub_nodes, int64_t n_sub,
                                 const int32_t* rowptr_in, const int32_t* col_in, const float* val_in,
                                 const int32_t* rowptr_out, const int32_t* col_out, const float* val_out,
                                 const int32_t* ids, int64_t n_batch, const int32_t* node_off, int64_t n_nodes,
                                 const int32_t* brow_in, const int32_t* brow_out, int32_t* bcol_in, float* bval_in,
                                 int32_t* bcol_out, float* bval_out, int32_t* node_map, int64_t* pos, int64_t pos_width,
                                 void* stream) {
    SEG_REQUIRE(n_sub >= 0 && n_sub < INT32_MAX && n_batch >= 0 && n_batch < INT32_MAX && n_nodes >= 0 &&
                    n_nodes < INT32_MAX && pos_width >= 0 && pos_width < INT32_MAX,
                "seg_collate: negative or too large size");
    if (n_batch == 0) return 0;
    SEG_REQUIRE(sub_ptr && rowptr_in && rowptr_out && ids && node_off && brow_in && brow_out && pos,
                "seg_collate: null pointer");
    SEG_REQUIRE(n_nodes == 0 || (sub_nodes && node_map && col_in && val_in && col_out && val_out && bcol_in &&
                                 bval_in && bcol_out && bval_out),
                "seg_collate: null pointer");
    SEG_REQUIRE(pos_width > 0 || n_nodes == 0, "seg_collate: pos_width 0 with %lld batch nodes", (long long)n_nodes);
    return glass::seg_collate_launch(sub_ptr, sub_nodes, n_sub, rowptr_in, col_in, val_in, rowptr_out, col_out, val_out,
                                     ids, n_batch, node_off, brow_in, brow_out, bcol_in, bval_in, bcol_out, bval_out,
                                     node_map, pos, pos_width, stream);
}

extern "C" int64_t glass_seg_khop_ws_bytes(int64_t n_base, int64_t n_sub) {
    if (n_base < 0 || n_base >= INT32_MAX || n_sub < 0 || n_sub >= INT32_MAX) return GLASS_E_ARG;
    if (n_base <= GLASS_SEG_KHOP_LDS_NODES || n_sub == 0) return 0;
    const int64_t slots = n_sub < GLASS_SEG_KHOP_WS_SLOTS ? n_sub : GLASS_SEG_KHOP_WS_SLOTS;
    return slots * 3 * ((n_base + 31) / 32) * (int64_t)sizeof(uint32_t);
}

static int seg_khop_check(const char* what, const int32_t* in_rowptr, const int32_t* in_col, int64_t n_base,
                          const int32_t* sub_ptr, const int32_t* sub_nodes, int64_t n_sub, int64_t n_member, int hops,
                          const void* ws, int64_t ws_bytes) {
    SEG_REQUIRE(n_base >= 0 && n_base < INT32_MAX && n_sub >= 0 && n_sub < INT32_MAX && n_member >= 0 &&
                    n_member < INT32_MAX, "%s: negative or too large size (n_base, n_sub, n_member < 2^31 - 1)", what);
    SEG_REQUIRE(hops >= 0, "%s: hops %d < 0", what, hops);
    SEG_REQUIRE(in_rowptr && sub_ptr, "%s: null pointer", what);
    SEG_REQUIRE(n_member == 0 || (sub_nodes && in_col), "%s: null pointer", what);
    const int64_t need = glass_seg_khop_ws_bytes(n_base, n_sub);
    if (need > 0 && (!ws || ws_bytes < need)) {
        glass::set_error("%s: n_base %lld needs a workspace of %lld bytes (glass_seg_khop_ws_bytes), got %lld", what,
                         (long long)n_base, (long long)need, ws ? (long long)ws_bytes : 0ll);
        return GLASS_E_WS;
    }
    return 0;
}

extern "C" int glass_seg_khop_count(const int32_t* in_rowptr, const int32_t* in_col, int64_t n_base,
                                    const int32_t* sub_ptr, const int32_t* sub_nodes, int64_t n_sub, int64_t n_member,
                                    int hops, void* ws, int64_t ws_bytes, int32_t* ball_cnt, void* stream) {
    int rc = seg_khop_check("seg_khop_count", in_rowptr, in_col, n_base, sub_ptr, sub_nodes, n_sub, n_member, hops, ws,
                            ws_bytes);
    if (rc) return rc;
    if (n_sub == 0) return 0;
    SEG_REQUIRE(ball_cnt, "seg_khop_count: null ball_cnt");
    return glass::seg_khop_launch(in_rowptr, in_col, n_base, sub_ptr, sub_nodes, n_sub, hops, ws, false, ball_cnt,
                                  nullptr, nullptr, stream);
}

extern "C" int glass_seg_khop_fill(const int32_t* in_rowptr, const int32_t* in_col, int64_t n_base,
                                   const int32_t* sub_ptr, const int32_t* sub_nodes, int64_t n_sub, int64_t n_member,
                                   int hops, void* ws, int64_t ws_bytes, const int32_t* ball_ptr, int32_t* ball_nodes,
                                   void* stream) {
    int rc = seg_khop_check("seg_khop_fill", in_rowptr, in_col, n_base, sub_ptr, sub_nodes, n_sub, n_member, hops, ws,
                            ws_bytes);
    if (rc) return rc;
    if (n_sub == 0) return 0;
    SEG_REQUIRE(ball_ptr && (n_member == 0 || ball_nodes), "seg_khop_fill: null output pointer");
    return glass::seg_khop_launch(in_rowptr, in_col, n_base, sub_ptr, sub_nodes, n_sub, hops, ws, true, nullptr,
                                  ball_ptr, ball_nodes, stream);
}

extern "C" int glass_seg_centre_index(const int32_t* centre_ptr, const int32_t* centre_nodes, int64_t n_sub,
                                      int64_t n_centre, const int32_t* ball_ptr, const int32_t* ball_nodes,
                                      int64_t n_ball, int32_t* centre_local, void* stream) {
    SEG_REQUIRE(n_sub >= 0 && n_sub < INT32_MAX, "seg_centre_index: n_sub %lld outside [0, 2^31 - 1)", (long long)n_sub);
    SEG_REQUIRE(n_centre >= 0 && n_centre < INT32_MAX, "seg_centre_index: n_centre %lld outside [0, 2^31 - 1)",
                (long long)n_centre);
    SEG_REQUIRE(n_ball >= 0 && n_ball < INT32_MAX, "seg_centre_index: n_ball %lld outside [0, 2^31 - 1)",
                (long long)n_ball);
    if (n_sub == 0) return 0;
    SEG_REQUIRE(centre_ptr, "seg_centre_index: null centre_ptr");
    SEG_REQUIRE(ball_ptr, "seg_centre_index: null ball_ptr");
    SEG_REQUIRE(n_centre == 0 || centre_nodes, "seg_centre_index: null centre_nodes");
    SEG_REQUIRE(n_centre == 0 || centre_local, "seg_centre_index: null centre_local");
    SEG_REQUIRE(n_ball == 0 || ball_nodes, "seg_centre_index: null ball_nodes");
    return glass::seg_centre_index_launch(centre_ptr, centre_nodes, n_sub, ball_ptr, ball_nodes, centre_local, stream);
}

extern "C" int glass_seg_collate_centre(const int32_t* sub_ptr, const int32_t* sub_nodes, int64_t n_sub,
                                        const int32_t* rowptr_in, const int32_t* col_in, const float* val_in,
                                        const int32_t* rowptr_out, const int32_t* col_out, const float* val_out,
                                        const int32_t* centre_ptr, const int32_t* centre_local, int64_t n_centre,
                                        const int32_t* ids, int64_t n_batch, const int32_t* node_off, int64_t n_nodes,
                                        const int32_t* brow_in, const int32_t* brow_out, int32_t* bcol_in,
                                        float* bval_in, int32_t* bcol_out, float* bval_out, int32_t* node_map,
                                        int64_t* pos, int64_t pos_width, uint8_t* mark, void* stream) {
    SEG_REQUIRE(n_sub >= 0 && n_sub < INT32_MAX, "seg_collate_centre: n_sub %lld outside [0, 2^31 - 1)", (long long)n_sub);
    SEG_REQUIRE(n_centre >= 0 && n_centre < INT32_MAX, "seg_collate_centre: n_centre %lld outside [0, 2^31 - 1)",
                (long long)n_centre);
    SEG_REQUIRE(n_batch >= 0 && n_batch < INT32_MAX, "seg_collate_centre: n_batch %lld outside [0, 2^31 - 1)",
                (long long)n_batch);
    SEG_REQUIRE(n_nodes >= 0 && n_nodes < INT32_MAX, "seg_collate_centre: n_nodes %lld outside [0, 2^31 - 1)",
                (long long)n_nodes);
    SEG_REQUIRE(pos_width >= 0 && pos_width < INT32_MAX, "seg_collate_centre: pos_width %lld outside [0, 2^31 - 1)",
                (long long)pos_width);
    if (n_batch == 0) return 0;
    SEG_REQUIRE(sub_ptr && rowptr_in && rowptr_out, "seg_collate_centre: null split row pointer (sub_ptr, rowptr_in, rowptr_out)");
    SEG_REQUIRE(ids && node_off && brow_in && brow_out, "seg_collate_centre: null batch index (ids, node_off, brow_in, brow_out)");
    SEG_REQUIRE(centre_ptr, "seg_collate_centre: null centre_ptr");
    SEG_REQUIRE(n_centre == 0 || centre_local, "seg_collate_centre: null centre_local");
    SEG_REQUIRE(pos, "seg_collate_centre: null pos");
    SEG_REQUIRE(n_nodes == 0 || (sub_nodes && col_in && val_in && col_out && val_out),
                "seg_collate_centre: null split array (sub_nodes, col_*, val_*)");
    SEG_REQUIRE(n_nodes == 0 || (node_map && bcol_in && bval_in && bcol_out && bval_out),
                "seg_collate_centre: null batch output (node_map, bcol_*, bval_*)");
    SEG_REQUIRE(n_nodes == 0 || mark, "seg_collate_centre: null mark");
    SEG_REQUIRE(pos_width > 0 || n_nodes == 0, "seg_collate_centre: pos_width 0 with %lld batch nodes",
                (long long)n_nodes);
    return glass::seg_collate_centre_launch(sub_ptr, sub_nodes, n_sub, rowptr_in, col_in, val_in, rowptr_out, col_out,
                                            val_out, centre_ptr, centre_local, ids, n_batch, node_off, brow_in, brow_out,
                                            bcol_in, bval_in, bcol_out, bval_out, node_map, pos, pos_width, mark, stream);
}

// ---- K1w  backward of K2 (glass_adj_values_f32): host-side validation, then the launch in spmm_edge.hip ----------------------
namespace glass {
int adj_values_bwd_launch(const int32_t*, const int32_t*, const int32_t*, const float*, const float*, const float*, const float*,
                          int64_t, int64_t, int, float*, void*);
}  // namespace glass

extern "C" int glass_adj_values_bwd_f32(const int32_t* rowptr, const int32_t* col, const int32_t* perm, const float* deg,
                                        const float* dval, const float* R, const float* C, int64_t n_rows, int64_t nnz,
                                        int aggr, float* dw, void* stream) {
    if (aggr < 0 || aggr > 2) {
        glass::set_error("adj_values_bwd: unknown aggr %d (0=mean,1=sum,2=gcn)", aggr);
        return GLASS_E_UNSUPPORTED;
    }
    SEG_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX && nnz >= 0 && nnz < INT32_MAX, "adj_values_bwd: negative or too large size");
    if (n_rows == 0) return 0;
    SEG_REQUIRE(rowptr, "adj_values_bwd: null rowptr");
    SEG_REQUIRE(nnz == 0 || (perm && dval && dw), "adj_values_bwd: null perm/dval/dw");
    SEG_REQUIRE(aggr == 1 || nnz == 0 || (deg && R), "adj_values_bwd: aggr mean and gcn need deg and R");
    SEG_REQUIRE(aggr != 2 || nnz == 0 || (col && C), "adj_values_bwd: aggr gcn needs col and C");
    if (nnz == 0) return 0;
    return glass::adj_values_bwd_launch(rowptr, col, perm, deg, dval, R, C, n_rows, nnz, aggr, dw, stream);
}

// ---- K2d  edge dropout (glass_adj_dropedge_f32): host-side validation, then the launches in spmm_dropedge.hip ---------------------
namespace glass {
int adj_dropedge_launch(const int32_t*, const int32_t*, const float*, const int32_t*, const int32_t*, const float*, int64_t, int,
                        float, int, const int64_t*, uint64_t, float*, float*, float*, uint8_t*, void*);
}  // namespace glass

extern "C" int glass_adj_dropedge_f32(const int32_t* rowptr, const int32_t* col, const float* w, const int32_t* rowptr_t,
                                      const int32_t* col_t, const float* w_t, int64_t n_rows, int aggr, float p, int symmetric,
                                      const int64_t* rng, uint64_t call_id, float* deg, float* val, float* val_t, uint8_t* keep,
                                      void* stream) {
    if (aggr < 0 || aggr > 2) {
        glass::set_error("adj_dropedge: unknown aggr %d (0=mean,1=sum,2=gcn)", aggr);
        return GLASS_E_UNSUPPORTED;
    }
    SEG_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX, "adj_dropedge: n_rows %lld outside [0, 2^31 - 1)", (long long)n_rows);
    SEG_REQUIRE(p >= 0.f && p < 1.f, "adj_dropedge: p %g outside [0, 1)", (double)p);  // (a NaN fails both comparisons)
    SEG_REQUIRE(rowptr && col && w, "adj_dropedge: null forward CSR (rowptr, col, w)");
    SEG_REQUIRE(rowptr_t && col_t && w_t, "adj_dropedge: null transposed CSR (rowptr_t, col_t, w_t)");
    SEG_REQUIRE(rng, "adj_dropedge: null rng (the device (seed, step) words)");
    SEG_REQUIRE(deg && val && val_t, "adj_dropedge: null output (deg, val, val_t)");
    if (n_rows == 0) return 0;
    return glass::adj_dropedge_launch(rowptr, col, w, rowptr_t, col_t, w_t, n_rows, aggr, p, symmetric, rng, call_id, deg, val,
                                      val_t, keep, stream);
}
