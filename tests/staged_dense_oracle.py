"""Host side of the tests of the staged dense kernels of glass_amd/csrc/dense.hip — the hidden-64 family (trans_fwd2_kernel,
dual_fwd_kernel<64, true, 1, 4>, trans_dgrad2_body, dual_dgrad_kernel<64, 128, 1, 4>, dual_bwd_kernel, comb_fwd_eff2_kernel,
comb_fwd_eff3_kernel, comb_dgrad_eff_kernel, comb_bwd_eff_kernel) and its eight-wave hidden-128 siblings (trans_fwd3_kernel,
trans_dgrad2_kernel<128>, trans_dgrad3_kernel, comb_dgrad3_kernel, comb_fwd_eff2/3_kernel<128>), behind the five C entries
glass_dual_linear_fwd_f32 / _dgrad_f32 / _bwd_f32 and glass_comb_eff_fwd_f32 / _bwd_f32.  Torch fp64 and numpy on the CPU, no GPU.

Truth and mass: the stage functions of tests/tiled_dense_oracle.py (width-generic) as they are, the gate of tests/readout_oracle.py
(|got - want| <= 1e-5 * mass per element), the exact-accumulator helpers of tests/graphnorm_oracle.py, the dW / db truth of
tests/wgrad_oracle.py (plain form for dual_bwd, S / L form with its (c_S, c_L) coefficients for comb_bwd_eff).  Every stage is a
function of what the kernel really read: downstream stages take the kernel's own upstream outputs as read back.

What is new here: the statistics / GraphNorm partials ENTRY BY ENTRY for launches whose entries are no plain 64-row tiles
(`entry_rows`: a main workgroup of the effective-weight launches counts its unlabeled rows, an extra workgroup its 64 (80) listed rows,
an extra workgroup beyond the list writes zeros; the stage-run kernels write one entry per workgroup of rows_main rows and zero the
entries up to ceil(N / 64)); the label lists; the dispatch of the default build restated (`fwd_form`, `dgrad_form`,
`comb_eff_fwd_form`, `comb_eff_bwd_form`), tied to the source text by `source_constants` / tests/test_staged_dense_host.py; the
parameter lists of tests/test_gpu_staged_dense.py (both files share them).

Three things the restated dispatch says openly:
  * at hidden 64 comb_fwd_eff3_kernel has no split instantiation: a tall comb forward (rows_main > 80) forms f32 products whatever the
    call's option; at hidden 128 it is the other way round (comb_fwd_eff2_kernel<128> has no split form);
  * the stand-alone data gradient of the trans pair at hidden 64 (glass_dual_linear_dgrad_f32, and the first of the two launches
    beyond kFusedBwdMaxRows) runs trans_dgrad2_body<64, false> whatever the option; dual_fwd_kernel and dual_dgrad_kernel<64, 128>
    have no split form either;
  * the `g.ny == 1 && g.rows_per_slab % 32 == 0` condition of the fused trans launch holds for EVERY N <= kFusedBwdMaxRows (wgrad_geom
    rounds the slabs of a one-tile shape to 32 rows there): no row count lies on its far side, so the non-split fused trans launch is
    reached through the call's option alone.  The same goes for `rows_per_slab % 32` of the fused comb launch (wgrad_sl_geom).
    `fused_condition_sweep` checks every N of the range (the comb launch at lab_cap 0, 64, 4096 and 100 000).

The exact accumulators (stats_exact / gn_exact in {2, 4, 8, 16}): every workgroup adds ONE value per column.  The forward kernels form it
from fp64 lane sums of the written fp32 values (squares exact), so the decoded sums meet graphnorm_oracle.exact_sum_bound against the exact
column sums of the read-back `out`; the backward ones sum fp32 products g * xhat and are gated at 1e-5 * mass like every other output."""
import functools
import os
import re

import numpy as np
import torch

import graphnorm_oracle as G
import tiled_dense_oracle as TD
import wgrad_oracle as WO
from graphnorm_oracle import acc_decode, bwd_exact_form, column_sums_exact, exact_sum_bound  # noqa: F401  (re-exported)
from readout_oracle import TOL, gate  # noqa: F401  (re-exported)
from tiled_dense_oracle import (ACT_ELU, ACT_NONE, ACT_RELU, _cdiv, restate_product, split3, stage_dgrad, stage_fwd,  # noqa: F401
                                stage_gn_partials, stage_prologue, stage_stats, zw)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
f32 = np.float32
FUSED_MAX_ROWS = 100000      # kFusedBwdMaxRows
COMB_DGRAD3_LIST = 4096      # kCombDgrad3List
CHIP = 256                   # workgroups of one round (the literal 256 of every tall / rows_main condition)
LAYOUT = dict(wave16=0, wave16_eff_fwd=6, wave16_eff_dgrad=7, wave16_eff_fwd_cols=8, wave16_cols=9, wave16_eff_dgrad_cols=10)
V2 = ("GLASS_COMB_DGRAD_V2", "GLASS_TRANS_DGRAD_V2", "GLASS_TRANS_WGRAD_STAGED2", "GLASS_TRANS_FWD_V2", "GLASS_COMB_FWD_V2", "GLASS_SL_STAGED2")


def source_constants(csrc=None):
    """every constant and condition the restated dispatch relies on, read from the text of dense.hip, dense_common.h, wgrad_common.h
    (and wgrad_sl_geom in linear.hip); csrc: another directory holding the files (a scratch copy)"""
    csrc = csrc or os.path.join(ROOT, "glass_amd", "csrc")
    rd = lambda n: open(os.path.join(csrc, n)).read()
    d, c, w, lin = rd("dense.hip"), rd("dense_common.h"), rd("wgrad_common.h"), rd("linear.hip")
    num = lambda pat, text: int(re.search(pat, text, re.S).group(1))
    fwd = re.search(r'extern "C" int glass_dual_linear_fwd_f32\(.*?\n}\n', d, re.S).group(0)
    dg = re.search(r"static int dgrad_launch\(.*?\n}\n", d, re.S).group(0)
    cf = re.search(r'extern "C" int glass_comb_eff_fwd_f32\(.*?\n}\n', d, re.S).group(0)
    cb = re.search(r'extern "C" int glass_comb_eff_bwd_f32\(.*?\n}\n', d, re.S).group(0)
    geom = re.search(r"static CombFwdGeom comb_fwd_geom\(int64_t n_nodes, int64_t lab_cap, int64_t H\) \{.*?\n}\n", d, re.S).group(0)
    slg = re.search(r"WgradSLGeom wgrad_sl_geom\(.*?\n}\n", lin, re.S).group(0)
    return {
        "trans_tall_text": "const int64_t wg80 = ceil_div(n_nodes, 80);" in fwd and
                           "const bool tall = (stats == nullptr || stats_exact) && grid.x > 256 && wg80 <= 256;" in fwd,
        "trans_fwd2_forms_text": "if (tall) GLASS_TF2S(5); else GLASS_TF2S(4);" in fwd and "if (tall) GLASS_TF2(5, 2); else GLASS_TF2(4, 2);" in fwd and
                                 "if (h64_split_products()) {" in fwd and "trans_fwd2_kernel<64, NS, 2, true>" in fwd,
        "trans_fwd_h64_text": "if (GLASS_TRANS_FWD_V2 && !comb && H == 64) {" in fwd and "GLASS_FWD(64, 1, 4)" in fwd,
        "trans_fwd3_text": "if (GLASS_TRANS_FWD_V2 && !comb && H == 128) {" in fwd and
                           "int64_t rows_main = ceil_div(ceil_div(n_nodes, (int64_t)256), (int64_t)16) * 16;" in fwd and
                           "if (rows_main < 64) rows_main = 64;" in fwd and "trans_fwd3_kernel<128, true>" in fwd and "trans_fwd3_kernel<128, false>" in fwd,
        "comb_tall_text": "const int64_t wg80 = ceil_div(n_nodes, 80) + ceil_div(lab_cap, 80);" in cf and
                          "const bool tall = GLASS_COMB_FWD_V2 && (stats == nullptr || stats_exact) && grid.x > 256 && wg80 <= 256;" in cf,
        "comb_fwd3_tall_text": "return comb_fwd3_on() && comb_fwd_geom(n_nodes, lab_cap, H).rows_main > 80;" in d and
                               'static bool comb_fwd3_on() { return lab_knob("GLASS_COMB_FWD3", 1) != 0 && GLASS_COMB_FWD_V2; }' in d,
        "comb_fwd_geom_text": all(s in geom for s in ("const int64_t sr = (H == 64 && fwd_wave_groups(true) == 2) ? 32 : 16;",
                                                      "int64_t rows = ceil_div(ceil_div(n_nodes, (int64_t)256), sr) * sr;", "if (rows < 64) rows = 64;",
                                                      "g.rows_extra = 64;", "g.n_extra = (int)ceil_div(lab_cap, (int64_t)64);")) and
                              "return comb ? 1 : 2;" in d,
        "comb_fwd_forms_text": all(s in cf for s in ("if (H == 128 && tiled_split_products()) {", "if (dr) GLASS_CF3(64, true, 1); else GLASS_CF3(64, false, 1);",
                                                     "} else if (GLASS_COMB_FWD_V2 && h64_split_products()) {", "comb_fwd_eff2_kernel<64, DR, NS, 1, true>",
                                                     "comb_fwd_eff3_kernel<128, DR, 1, true>", "const bool dr = gn_saved && p_drop > 0.f;")) and
                               "comb_fwd_eff3_kernel<64, DR, 1, true>" not in cf and "comb_fwd_eff2_kernel<128, DR, NS, 1, true>" not in cf,
        "comb_fwd_blocks_text": "if (comb_fwd3_tall(n_nodes, lab_cap, H)) {" in d and "return g.n_main + g.n_extra;" in d and
                                d.count("return ceil_div(n_nodes, 64) + ceil_div(lab_cap, 64);") == 2,
        "kFusedBwdMaxRows": num(r"constexpr int64_t kFusedBwdMaxRows = (\d+);", w),
        "fused_cond_text": "if (wg && H == 64 && n_nodes <= kFusedBwdMaxRows && !wgrad_tiled_shape(n_nodes, O, I)) {" in dg,
        "fused_sp_text": "const bool sp = n_out == H && h64_split_products() && GLASS_TRANS_DGRAD_V2 && GLASS_TRANS_WGRAD_STAGED2 && O == 128 && I == 64 &&" in dg and
                         "g.ny == 1 && g.rows_per_slab % 32 == 0;" in dg,
        "fused_kernels_text": all(s in dg for s in ("dual_bwd_kernel<64, 64, true>", "dual_bwd_kernel<64, 64>)", "dual_bwd_kernel<64, 128>)")) and
                              "const unsigned blocks = grid.x + (unsigned)(g.n_slabs * g.ny * g.nz);" in dg,
        "dg2_text": "const bool dg2 = GLASS_TRANS_DGRAD_V2 && H == 64 && n_out == H;" in dg and "GLASS_DG(64, 1, 4)" in dg and
                    "if (GLASS_TRANS_DGRAD_V2 && H == 64 && NT == 64) {" in d,
        "dgrad128_text": all(s in dg for s in ("if (GLASS_TRANS_DGRAD_V2 && H == 128 && n_out == H) {", "const int64_t n_tiles = ceil_div(n_nodes, 64);",
                                               'if (lab_knob("GLASS_TRANS_DGRAD3", 1) && (n_tiles > 256 || split3)) {',
                                               "int stages_per_wg = (int)ceil_div(n_stages, 256);", "if (stages_per_wg < 4) stages_per_wg = 4;",
                                               "trans_dgrad2_kernel<128>), dim3((unsigned)ceil_div(n_nodes, 64))")),
        "comb_dgrad3_text": all(s in dg for s in ("if (GLASS_COMB_DGRAD_V2 && H == 128 && n_out == 2 * H) {", "if (act != GLASS_ACT_NONE || addend || p_drop > 0.f) {",
                                                  "if (rows_main > kCombDgrad3List) rows_main = kCombDgrad3List;")),
        "kCombDgrad3List": num(r"constexpr int kCombDgrad3List = (\d+);", d),
        "comb_bwd_text": all(s in cb for s in ("const unsigned n_dg = (unsigned)(n_main + ceil_div(lab_cap, 64));", "if (!X) {  // data gradient only",
                                               "if (n_nodes > kFusedBwdMaxRows) {", "launch_wgrad_sl(sl, n_nodes, zr, part_w, part_b, st);",
                                               "if (h64_split_products() && GLASS_COMB_DGRAD_V2 && GLASS_SL_STAGED2 && g.rows_per_slab % 32 == 0) {",
                                               "comb_bwd_eff_kernel<64, true>), dim3(n_dg + (unsigned)(g.n_s + g.n_l))", "comb_bwd_eff_kernel<64>), dim3(n_dg + (unsigned)(g.n_s + g.n_l))")),
        "sl_geom_text": all(s in slg for s in ("g.n_l = (int)ceil_div(lab_cap > 0 ? lab_cap : 1, 64);", "int64_t room = N <= 100000 ? 2 * 256 - 4 - ceil_div(N, 64) - 2 * g.n_l : 256;",
                                               "if (room > 256) room = 256;", "if (room < 32) room = 32;", "if (rows < 64) rows = 64;", "rows = ceil_div(rows, 8) * 8;",
                                               "if (N <= kFusedBwdMaxRows) rows = ceil_div(rows, 32) * 32;",
                                               "g.part_b_floats = (int64_t)(g.n_s + g.n_l) * kSLOut + kWgradHeaderFloats;")),
        "gn_src_supported_text": "return (GLASS_COMB_DGRAD_V2 && GLASS_SL_STAGED2 && !GLASS_COMB_BWD_V2 && H == 64 && n_nodes > 0 && n_nodes <= kFusedBwdMaxRows) ? 1 : 0;" in d,
        "image2_text": "A2.WT = A.WT + 2 * (2 * H * H);" in d,
        "v2_defaults": {k: num(r"#\s*define " + k + r" (\d)", d) for k in V2},
        "comb_bwd_v2_default": num(r"#define GLASS_COMB_BWD_V2 (\d)", d),
        "layouts": dict(wave16=num(r"kLayoutWave16 = (\d+),", c), wave16_eff_fwd=num(r"kLayoutWave16EffFwd = (\d+),", c),
                        wave16_eff_dgrad=num(r"kLayoutWave16EffDgrad = (\d+) ", c), wave16_eff_fwd_cols=num(r"constexpr int kLayoutWave16EffFwdCols = (\d+);", c),
                        wave16_cols=num(r"constexpr int kLayoutWave16Cols = (\d+);", c), wave16_eff_dgrad_cols=num(r"constexpr int kLayoutWave16EffDgradCols = (\d+);", c)),
        "layout_queries_text": "if (GLASS_TRANS_FWD_V2 && (wave16_shape_ok(H) || H == 128) && K == H) return kLayoutWave16Cols;" in d and
                               "if (GLASS_TRANS_DGRAD_V2 && (wave16_shape_ok(H) || H == 128) && n_out == H) return kLayoutWave16Cols;" in d and
                               "if (GLASS_COMB_DGRAD_V2 && H == 128 && n_out == 2 * H) return kLayoutWave16EffDgradCols;" in d and
                               "return GLASS_COMB_FWD_V2 ? kLayoutWave16EffFwdCols : kLayoutWave16EffFwd;" in d,
        "stat_rows_text": "return narrow_shape_ok(H) ? narrow_rows() : tiled_here(H) ? tiled_rows(H) : 64; }" in d,
    }


def check_source(k):
    """-> the names of the text conditions that moved (empty: the restatement stands)"""
    moved = [n for n, v in k.items() if n.endswith("_text") and not v]
    if k["kFusedBwdMaxRows"] != FUSED_MAX_ROWS or WO.FUSED_MAX_ROWS != FUSED_MAX_ROWS:
        moved.append("kFusedBwdMaxRows")
    if k["kCombDgrad3List"] != COMB_DGRAD3_LIST:
        moved.append("kCombDgrad3List")
    if set(k["v2_defaults"].values()) != {1} or k["comb_bwd_v2_default"] != 0:
        moved.append("v2_defaults")
    if k["layouts"] != LAYOUT:
        moved.append("layouts")
    return moved


# ---- dispatch restated (default build) ------------------------------------------------------------------------------------------------
def fwd_layout(H, comb):
    return LAYOUT["wave16_cols"] if not comb and H in (64, 128) else LAYOUT["wave16"]


def dgrad_layout(H, n_out):
    if n_out == H and H in (64, 128):
        return LAYOUT["wave16_cols"]
    return LAYOUT["wave16_eff_dgrad_cols"] if H == 128 else LAYOUT["wave16"]


def rows_main_of(N):
    return max(_cdiv(_cdiv(N, CHIP), 16) * 16, 64)


def fwd_form(H, comb, N, has_stats=False, stats_exact=0, f32_products=False):
    """glass_dual_linear_fwd_f32 -> dict kernel, rows (per workgroup), n_wg, split, entries (statistics entries of the partials form),
    entry_rows (rows one entry covers)"""
    if H == 64 and not comb:
        grid, wg80 = _cdiv(N, 64), _cdiv(N, 80)
        tall = (not has_stats or bool(stats_exact)) and grid > CHIP and wg80 <= CHIP
        sp = not f32_products
        return dict(kernel=f"trans_fwd2_kernel<64, {5 if tall else 4}, 2{', true' if sp else ''}>", rows=80 if tall else 64, n_wg=wg80 if tall else grid,
                    split=sp, tall=tall, entries=grid, entry_rows=64)
    if H == 64:
        return dict(kernel="dual_fwd_kernel<64, true, 1, 4>", rows=64, n_wg=_cdiv(N, 64), split=False, tall=False, entries=_cdiv(N, 64), entry_rows=64)
    assert H == 128 and not comb, "the hidden-128 comb forward is the tiled family's (tests/tiled_dense_oracle.py)"
    rm = rows_main_of(N)
    return dict(kernel=f"trans_fwd3_kernel<128, {'false' if f32_products else 'true'}>", rows=rm, n_wg=_cdiv(N, rm), split=not f32_products, tall=False,
                entries=_cdiv(N, 64), entry_rows=rm)


def dgrad_form(H, n_out, N, with_wgrad=False, f32_products=False):
    """glass_dual_linear_dgrad_f32 (with_wgrad False) / glass_dual_linear_bwd_f32 -> dict kernels (launch order), rows, n_wg (data-gradient
    workgroups), split (the data gradient's product form), fused, wgrad (the slab geometry or the second launch's route), entries, entry_rows"""
    assert n_out in (H, 2 * H)
    comb = n_out == 2 * H
    if H == 64:
        grid = _cdiv(N, 64)
        base = dict(rows=64, n_wg=grid, entries=grid, entry_rows=64)
        alone = "dual_dgrad_kernel<64, 128, 1, 4>" if comb else "dual_dgrad_kernel<64, 64, 1, 4> (trans_dgrad2_body<64>)"
        if not with_wgrad:
            return dict(base, kernels=[alone], split=False, fused=False, wgrad=None)
        if N <= FUSED_MAX_ROWS:
            g = WO.wgrad_geom(N, 128, n_out)
            sp = (not comb) and (not f32_products) and g["ny"] == 1 and g["rows"] % 32 == 0
            k = "dual_bwd_kernel<64, 128>" if comb else ("dual_bwd_kernel<64, 64, true>" if sp else "dual_bwd_kernel<64, 64>")
            return dict(base, kernels=[k], split=sp, fused=True, wgrad=dict(g, split=sp, eff=False, family="generic", n_lists=0,
                                                                             staged=not comb, blocks=grid + g["n_slabs"] * g["ny"] * g["nz"]))
        return dict(base, kernels=[alone] + WO.route("dual", N, 64, comb, ACT_NONE, f32_products)["kernels"], split=False, fused=False,
                    wgrad=WO.route("dual", N, 64, comb, ACT_NONE, f32_products))
    assert H == 128
    if not comb:
        n_tiles, sp = _cdiv(N, 64), not f32_products
        if n_tiles > CHIP or sp:
            n_stages = _cdiv(N, 16)
            spw = max(_cdiv(n_stages, CHIP), 4)
            return dict(kernels=[f"trans_dgrad3_kernel<128{', true' if sp else ''}>"], rows=16 * spw, stages_per_wg=spw, n_wg=_cdiv(n_stages, spw), split=sp,
                        fused=False, wgrad=None, entries=n_tiles, entry_rows=16 * spw)
        return dict(kernels=["trans_dgrad2_kernel<128>"], rows=64, n_wg=n_tiles, split=False, fused=False, wgrad=None, entries=n_tiles, entry_rows=64)
    rm = min(rows_main_of(N), COMB_DGRAD3_LIST)
    return dict(kernels=[f"comb_dgrad3_kernel<128, {'false' if f32_products else 'true'}>"], rows=rm, n_wg=_cdiv(N, rm), split=not f32_products, fused=False,
                wgrad=None, entries=_cdiv(N, 64), entry_rows=rm)


def comb_eff_fwd_blocks(N, lab_cap):
    """glass_comb_eff_fwd_blocks"""
    rm = rows_main_of(N)
    return _cdiv(N, rm) + _cdiv(lab_cap, 64) if rm > 80 else _cdiv(N, 64) + _cdiv(lab_cap, 64)


def comb_eff_fwd_form(H, N, lab_cap, has_stats=False, stats_exact=0, p_drop=0.0, f32_products=False, has_prologue=True):
    """glass_comb_eff_fwd_f32 -> dict kernel, rows_main, rows_extra, n_main, n_extra, n_wg, split, forced (the product form is not the call's
    option), entries (= glass_comb_eff_fwd_blocks)"""
    assert H in (64, 128)
    dr = "true" if (has_prologue and p_drop > 0) else "false"
    rm = rows_main_of(N)     # comb_fwd_geom: one wave group (fwd_wave_groups(true) == 1), 16-row stages
    if rm > 80:              # comb_fwd3_tall
        sp = H == 128 and not f32_products
        g = dict(kernel=f"comb_fwd_eff3_kernel<{H}, {dr}, 1{', true' if sp else ''}>", rows_main=rm, rows_extra=64, n_main=_cdiv(N, rm), n_extra=_cdiv(lab_cap, 64),
                 split=sp, forced=(H == 64 and not f32_products), tall=False)
    else:
        grid, wg80 = _cdiv(N, 64) + _cdiv(lab_cap, 64), _cdiv(N, 80) + _cdiv(lab_cap, 80)
        tall = (not has_stats or bool(stats_exact)) and grid > CHIP and wg80 <= CHIP
        r = 80 if tall else 64
        sp = H == 64 and not f32_products
        g = dict(kernel=f"comb_fwd_eff2_kernel<{H}, {dr}, {5 if tall else 4}{', 1, true' if sp else ''}>", rows_main=r, rows_extra=r, n_main=_cdiv(N, r),
                 n_extra=_cdiv(lab_cap, r), split=sp, forced=(H == 128 and not f32_products), tall=tall)
    g["n_wg"] = g["n_main"] + g["n_extra"]
    g["entries"] = comb_eff_fwd_blocks(N, lab_cap)
    assert g["tall"] or g["entries"] == g["n_wg"], "the workgroups of a launch that writes partials are glass_comb_eff_fwd_blocks"
    return g


def wgrad_sl_geom(N, lab_cap):
    n_l = _cdiv(max(lab_cap, 1), 64)
    room = 2 * CHIP - 4 - _cdiv(N, 64) - 2 * n_l if N <= 100000 else CHIP
    room = max(min(room, CHIP), 32)
    rows = _cdiv(max(_cdiv(N, room), 64), 8) * 8
    if N <= FUSED_MAX_ROWS:
        rows = _cdiv(rows, 32) * 32
    n_s = _cdiv(N, rows)
    return dict(n_s=n_s, n_l=n_l, rows=rows, ws_bytes=4 * ((n_s + n_l) * WO.K_TILE + (n_s + n_l) * 64 + WO.HEADER))


def comb_eff_bwd_form(N, lab_cap, with_wgrad=True, f32_products=False, dsrc_gn=False):
    """glass_comb_eff_bwd_f32 (hidden 64) -> dict kernels, n_dg, n_main, n_s, n_l, rows_per_slab, split, ws_bytes"""
    n_main = _cdiv(N, 64)
    n_dg = n_main + _cdiv(lab_cap, 64)
    g = wgrad_sl_geom(N, lab_cap)
    out = dict(n_dg=n_dg, n_main=n_main, n_s=g["n_s"], n_l=g["n_l"], rows_per_slab=g["rows"], ws_bytes=g["ws_bytes"], entries=n_dg, split=False)
    if dsrc_gn:
        assert with_wgrad and N <= FUSED_MAX_ROWS, "GLASS_E_UNSUPPORTED (glass_comb_eff_bwd_gn_src_supported)"
    if not with_wgrad:
        return dict(out, kernels=["comb_dgrad_eff_kernel<64>"])
    if N > FUSED_MAX_ROWS:
        return dict(out, kernels=["comb_dgrad_eff_kernel<64>", "wgrad_sl_kernel"])
    sp = (not f32_products) and g["rows"] % 32 == 0
    return dict(out, kernels=["comb_bwd_eff_kernel<64, true>" if sp else "comb_bwd_eff_kernel<64>"], split=sp)


def fused_condition_sweep(step=1):
    """(rows of the fused trans launch's slabs that are no multiple of 32, of the fused comb launch's) over 1 .. kFusedBwdMaxRows: both empty"""
    bad_t = [N for N in range(1, FUSED_MAX_ROWS + 1, step) if WO.wgrad_geom(N, 128, 64)["rows"] % 32 or WO.wgrad_geom(N, 128, 64)["ny"] != 1]
    bad_c = [N for N in range(1, FUSED_MAX_ROWS + 1, step) for cap in (0, 64, 4096, 100000) if wgrad_sl_geom(N, cap)["rows"] % 32]
    return bad_t, bad_c


# every kernel instantiation the five entries launch at hidden 64, and the hidden-128 stage-run kernels (default build)
INSTANTIATIONS_64 = (
    ["trans_fwd2_kernel<64, 4, 2>", "trans_fwd2_kernel<64, 5, 2>", "trans_fwd2_kernel<64, 4, 2, true>", "trans_fwd2_kernel<64, 5, 2, true>",
     "dual_fwd_kernel<64, true, 1, 4>", "dual_dgrad_kernel<64, 64, 1, 4> (trans_dgrad2_body<64>)", "dual_dgrad_kernel<64, 128, 1, 4>",
     "dual_bwd_kernel<64, 64, true>", "dual_bwd_kernel<64, 64>", "dual_bwd_kernel<64, 128>", "wgrad_partial_kernel<true, false>",
     "comb_dgrad_eff_kernel<64>", "wgrad_sl_kernel", "comb_bwd_eff_kernel<64, true>", "comb_bwd_eff_kernel<64>"] +
    [f"comb_fwd_eff2_kernel<64, {dr}, {ns}{sp}>" for dr in ("false", "true") for ns in (4, 5) for sp in ("", ", 1, true")] +
    [f"comb_fwd_eff3_kernel<64, {dr}, 1>" for dr in ("false", "true")])
INSTANTIATIONS_128 = (
    ["trans_fwd3_kernel<128, true>", "trans_fwd3_kernel<128, false>", "trans_dgrad2_kernel<128>", "trans_dgrad3_kernel<128>", "trans_dgrad3_kernel<128, true>",
     "comb_dgrad3_kernel<128, true>", "comb_dgrad3_kernel<128, false>"] +
    [f"comb_fwd_eff2_kernel<128, {dr}, {ns}>" for dr in ("false", "true") for ns in (4, 5)] +
    [f"comb_fwd_eff3_kernel<128, {dr}, 1{sp}>" for dr in ("false", "true") for sp in ("", ", true")])


# ---- label lists ----------------------------------------------------------------------------------------------------------------------
LISTS = ("empty0", "empty", "row0", "last", "middle", "n63", "n64", "n65", "tail_oob", "all", "wave16", "tile64", "batch")
OOB = 0x7FFFFFF0


def label_list(name, N, cap=None):
    """-> (mask uint8 [N], lab_rows int32 [max(cap, 1)], lab_count, cap): the unique labeled rows in first-occurrence order (the order a
    batch names them in: not sorted), the contract of LabRows in dense_common.h.  The tail behind `count` holds row 0 — a valid row the
    kernel must not store —, in `tail_oob` indices far out of range, which must never be dereferenced."""
    rng = np.random.RandomState(N + 17 * len(name))
    if name == "empty0":
        rows, cap = [], 0
    elif name == "empty":
        rows, cap = [], cap or 64
    elif name == "row0":
        rows = [0]
    elif name == "last":
        rows = [N - 1]
    elif name == "middle":
        rows = [N // 2]
    elif name in ("n63", "n64", "n65"):
        k = min(int(name[1:]), N)
        rows, cap = list(rng.permutation(N)[:k]), cap or 128
    elif name == "tail_oob":
        rows, cap = list(rng.permutation(N)[:min(5, N)]), cap or 128
    elif name == "all":
        rows = list(rng.permutation(N))
    elif name == "wave16":
        rows = list(rng.permutation(np.arange(16, min(32, N))))
    elif name == "tile64":
        t0 = 64 if N >= 128 else 0
        rows = list(rng.permutation(np.arange(t0, min(t0 + 64, N))))
    else:
        assert name == "batch"
        rows = list(rng.permutation(N)[:max(N // 20, 1)])
    cap = _cdiv(max(len(rows), 1), 64) * 64 if cap is None else cap
    assert len(rows) <= cap and len(set(rows)) == len(rows)
    lab = np.full(max(cap, 1), OOB if name == "tail_oob" else 0, dtype=np.int32)
    lab[:len(rows)] = rows
    mask = np.zeros(N, dtype=np.uint8)
    mask[rows] = 1
    return mask, lab, len(rows), cap


def entry_rows(N, form, mask=None, lab=None, count=0):
    """the rows whose values one statistics / GraphNorm-partials entry sums, entry by entry.  Plain launches: entry e < n_wg covers rows
    e * entry_rows ..; effective-weight launches (mask given): a main entry its unlabeled rows, an extra entry its listed rows.  Entries
    beyond the workgroups (and extra workgroups beyond the list) are empty: the kernel writes zeros there."""
    out = []
    if mask is None:
        r = form["entry_rows"]
        for e in range(form["entries"]):
            out.append(np.arange(min(e * r, N), min((e + 1) * r, N)) if e < form["n_wg"] else np.arange(0))
        return out
    m = np.asarray(mask).astype(bool)
    rm, re_, n_main = form.get("rows_main", 64), form.get("rows_extra", 64), form["n_main"]
    for e in range(n_main):
        idx = np.arange(e * rm, min((e + 1) * rm, N))
        out.append(idx[~m[idx]])
    for e in range(form["entries"] - n_main):
        out.append(np.asarray(lab[e * re_:min((e + 1) * re_, count)], dtype=np.int64))
    return out


def stage_entry_stats(out, entries):
    """[n_entries, 2, H] sum / sum of squares of the rows of each entry, from the `out` the kernel wrote (read back)"""
    o = out.to(F64)
    want = torch.stack([torch.stack([o[torch.as_tensor(e, dtype=torch.long)].sum(0), (o[torch.as_tensor(e, dtype=torch.long)]**2).sum(0)]) for e in entries])
    mass = torch.stack([torch.stack([o[torch.as_tensor(e, dtype=torch.long)].abs().sum(0), (o[torch.as_tensor(e, dtype=torch.long)]**2).sum(0)]) for e in entries])
    return want, mass


def stage_entry_gn(g, x, saved, alpha, gn_act, keep, entries):
    """[n_entries, 2, H] GraphNorm backward sums per entry (graphnorm_oracle.stage_bwd_sums on the entry's rows), zeros for an empty one"""
    ws, ms = [], []
    H = g.shape[1]
    for e in entries:
        i = torch.as_tensor(e, dtype=torch.long)
        if len(e) == 0:
            ws.append(torch.zeros(2, H, dtype=F64)), ms.append(torch.zeros(2, H, dtype=F64))
            continue
        w, m = G.stage_bwd_sums(g[i], x[i], saved.float(), alpha, gn_act, None if keep is None else keep[i])
        ws.append(w), ms.append(m)
    return torch.stack(ws), torch.stack(ms)


def gn_terms(g, x, saved, alpha, gn_act, keep):
    """the two per-row terms whose column sums the backward accumulators hold: g' = g keep act'(h), g' xhat (fp64) and their masses"""
    gp = G._g(g, x, saved.float(), gn_act, keep)
    x, mu, rstd, a = x.to(F64), saved[0].to(F64), saved[1].to(F64), alpha.to(F64)
    return gp, gp * (x - a * mu) * rstd


def exact_bound_terms(terms, k, adds, scale):
    """exact_sum_bound's formula on given per-row terms [(N, C)] -> (want [n, C], bound [n, C])"""
    want, bound = [], []
    for t in terms:
        s, e = column_sums_exact(t)
        want.append(s), bound.append((k + 2) * 2.0**-53 * t.to(F64).abs().sum(0) + adds * 2.0**-G.LO_BITS / scale + e)
    return torch.stack(want), torch.stack(bound)


# ---- recipes ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recipe(H, N, comb, seed=0):
    """tiled_dense_oracle.recipe at this width, with the weights of (H, comb, seed) alone (the images depend on nothing else)"""
    p = TD.recipe(H, N, comb, seed)
    w = TD.recipe(H, 8, comb, seed)
    p["W"], p["b"] = w["W"], w["b"]
    return p


# ---- fp32 restatements ------------------------------------------------------------------------------------------------------------------
def _two(N, rows=64):
    return ["two"] * _cdiv(N, rows)


def restate_fwd(A, xb, W, b, mask, z, act, split, N=None, mutant=None):
    """the two-product forward (trans_fwd2 / trans_fwd3 / dual_fwd_kernel) in fp32: tiled_dense_oracle.restate_fwd on 64-row tiles (the
    row tiling does not enter a row's sum).  Mutants: drop_kstep, swap_w (W1 / W0 exchanged: the label mix the other way round)"""
    n = A.shape[0] if N is None else N
    form = dict(BM=64, split=split, eff_live=False, paths=_two(n), partial_rows=64)
    return TD.restate_fwd(A, xb, W, b, mask, z, act, form, N=N, mutant=mutant)


def eff_weights(W, b, z):
    """(W_unl, b_unl, W_lab, b_lab) as the pack kernel and the forward epilogue round them (fp32)"""
    W, b = np.asarray(W, f32), np.asarray(b, f32)
    H = W.shape[0] // 2
    zr, omz = f32(z), f32(1.0 - z)
    return ((omz * W[:H] + zr * W[H:]).astype(f32), (omz * b[:H] + zr * b[H:]).astype(f32),
            (zr * W[:H] + omz * W[H:]).astype(f32), (zr * b[:H] + omz * b[H:]).astype(f32))


def _eff_skip(N, rows, mutant):
    """drop_kstep on a row whose value survives: the first row the list does not redo (main product), else the first listed one"""
    if mutant != "drop_kstep":
        return None, None
    free = sorted(set(range(N)) - set(int(r) for r in rows))
    return ((slice(free[0], free[0] + 1), 1), None) if free else (None, (slice(0, 1), 1))


def restate_eff_fwd(A, xb, W, b, z, split, lab, count, mutant=None):
    """the effective-weight forward: every row with the unlabeled weight (the row tiles), the listed rows redone with the labeled weight
    (the extra workgroups).  Mutants: drop_kstep; listed_unlabeled (a listed row redone with the unlabeled weight); list_entry_count
    (entry `lab_count` of the list consumed too)"""
    X = np.concatenate([np.asarray(A, f32), np.asarray(xb, f32)], 1)
    Wu, bu, Wl, bl = eff_weights(W, b, z)
    n = count + 1 if mutant == "list_entry_count" else count
    rows = np.asarray(lab[:n], dtype=np.int64)
    rows = rows[(rows >= 0) & (rows < X.shape[0])]
    skip, skip_l = _eff_skip(X.shape[0], rows, mutant)
    out = (restate_product(X, Wu, split, skip) + bu).astype(f32)
    if len(rows) and mutant != "listed_unlabeled":
        out[rows] = (restate_product(X[rows], Wl, split, skip_l) + bl).astype(f32)
    return out


def restate_dgrad(dsrc, T, W, mask, z, act, n_out, split, addend=None, keep=None, mutant=None):
    """the two-term data gradient (trans_dgrad2 / trans_dgrad3 / dual_dgrad_kernel): tiled_dense_oracle.restate_dgrad on 64-row tiles.
    Mutants: drop_kstep, swap_w, dropout_twice, addend_dropped"""
    form = dict(BM=64, split=split, paths=_two(np.asarray(dsrc).shape[0]))
    return TD.restate_dgrad(dsrc, T, W, mask, z, act, n_out, form, addend=addend, keep=keep, mutant=mutant)


def restate_eff_dgrad(dsrc, W, z, split, lab, count, mutant=None):
    """the effective-weight data gradient (comb_dgrad_eff / comb_dgrad2_body / comb_dgrad3): dc . W_unl for every row, listed rows redone
    with W_lab.  Mutants as restate_eff_fwd"""
    d = np.asarray(dsrc, f32)
    Wu, _, Wl, _ = eff_weights(W, np.zeros(np.asarray(W).shape[0], f32), z)
    n = count + 1 if mutant == "list_entry_count" else count
    rows = np.asarray(lab[:n], dtype=np.int64)
    rows = rows[(rows >= 0) & (rows < d.shape[0])]
    skip, skip_l = _eff_skip(d.shape[0], rows, mutant)
    out = restate_product(d, np.ascontiguousarray(Wu.T), split, skip)
    if len(rows) and mutant != "listed_unlabeled":
        out[rows] = restate_product(d[rows], np.ascontiguousarray(Wl.T), split, skip_l)
    return out


def restate_entry_stats(out, entries, extra_row=None):
    """the epilogue's sums per entry: fp32 lane sums of up to 20 values (here: the entry's rows in fp32 order), folded in fp64.
    extra_row: a row past N summed into the last non-empty entry (a mutant)"""
    o = np.asarray(out, f32)
    H = o.shape[1]
    st = np.zeros((len(entries), 2, H))
    for e, idx in enumerate(entries):
        s, q = np.zeros(H, f32), np.zeros(H, f32)
        for r in idx:
            s, q = (s + o[r]).astype(f32), (q + (o[r] * o[r]).astype(f32)).astype(f32)
        st[e, 0], st[e, 1] = s, q
    if extra_row is not None:
        last = max(e for e, idx in enumerate(entries) if len(idx))
        x = np.asarray(extra_row, np.float64)
        st[last, 0] += x
        st[last, 1] += x * x
    return st


def wgrad_form_of(form):
    """the weight-gradient half of a fused launch as the form dict wgrad_oracle.restate_dual walks"""
    g = form["wgrad"]
    return dict(family="generic", split=g["split"], eff=False, rows=g["rows"], n_slabs=g["n_slabs"], n_lists=0)


def sl_form_of(form):
    """the S / L partials of comb_bwd_eff as wgrad_oracle.restate_dual's effective-weight form: S per slab, L over the listed rows"""
    return dict(family="generic", split=form["split"], eff=True, rows=form["rows_per_slab"], n_slabs=form["n_s"], n_lists=0)


def restate_wgrad(wform, dsrc, T, mask, z, act, X, X2, N, mutant=None):
    """-> (dW, db) fp32.  Mutants: stage16_skipped (one 16-row stage of the middle slab left out), swap_cs_cl (S / L form), and
    wgrad_oracle's own (row_past_N, label_as_unlabeled, ...)"""
    d = np.asarray(dsrc, f32).copy()
    if mutant == "stage16_skipped":
        b = WO.slab_bounds(wform, N)
        r0, r1 = b[len(b) // 2]
        d[min(r0 + 16, r1 - 1):min(r0 + 32, r1)] = 0
        mutant = None
    return WO.restate_dual(wform, d, None if T is None else np.asarray(T, f32), mask, z, act, np.asarray(X, f32), None if X2 is None else np.asarray(X2, f32),
                           N, mut=mutant)


MUTANTS = ("drop_kstep", "swap_w", "listed_unlabeled", "list_entry_count", "row_N_in_partial", "dropout_twice", "addend_dropped", "stage16_skipped", "swap_cs_cl")


# ---- the cases of tests/test_gpu_staged_dense.py ---------------------------------------------------------------------------------------
ROWS_64 = (1, 15, 16, 17, 63, 64, 65, 77, 1000)
# trans forward, hidden 64: (N, f32_products, gather, (gn_act, p_drop) or None, act, want_T, stats in none | part | exact n_rep, gn_src) — a pairwise
# cover: every value of every axis appears in both product forms
TRANS_FWD_SMALL = [
    (1, False, False, None, 1, True, ("part", 0), False), (15, True, True, (0, 0.0), 2, False, ("none", 0), False),
    (16, False, True, (1, 0.5), 0, True, ("exact", 2), False), (17, True, False, (2, 0.5), 1, True, ("part", 0), False),
    (63, False, False, (2, 0.0), 2, False, ("exact", 4), True), (64, True, False, (1, 0.0), 0, False, ("exact", 8), True),
    (65, False, True, (0, 0.5), 1, False, ("none", 0), False), (77, True, True, (1, 0.5), 2, True, ("exact", 16), False),
    (1000, False, False, (1, 0.0), 1, True, ("part", 0), False), (1000, True, True, (2, 0.0), 0, True, ("exact", 2), False),
    (77, False, False, (0, 0.0), 2, True, ("none", 0), False), (77, True, False, None, 1, False, ("part", 0), False),
    (65, True, False, (0, 0.5), 0, True, ("exact", 4), False), (64, False, True, (2, 0.5), 0, False, ("part", 0), False),
    (17, False, False, None, 0, False, ("exact", 16), False), (1, True, False, None, 2, True, ("none", 0), False)]
# ... on both sides of the tall switch: (N, stats, rows expected)
TRANS_FWD_TALL = [(16384, ("none", 0), 64), (20481, ("none", 0), 64), (16385, ("none", 0), 80), (20480, ("exact", 4), 80), (16385, ("exact", 2), 80),
                  (20480, ("none", 0), 80), (16385, ("part", 0), 64)]
# data gradient, hidden 64: (N, n_out, act, addend, p_drop, gn = (gn_act, gn_p_drop, exact n_rep) or None)
DGRAD_64 = [(1, 64, 0, False, 0.0, None), (1, 128, 1, True, 0.0, (0, 0.0, 4)), (15, 128, 0, True, 0.0, (0, 0.0, 0)), (15, 64, 0, True, 0.5, (2, 0.0, 8)),
            (16, 64, 1, True, 0.5, (1, 0.0, 0)), (16, 128, 2, True, 0.0, None), (17, 128, 2, False, 0.0, (0, 0.5, 2)), (17, 64, 2, True, 0.0, (1, 0.5, 0)),
            (63, 64, 2, False, 0.0, (2, 0.5, 4)), (63, 128, 0, False, 0.0, (1, 0.0, 0)), (64, 128, 1, True, 0.0, None), (64, 64, 0, True, 0.5, (0, 0.0, 0)),
            (65, 64, 1, True, 0.5, (0, 0.0, 16)), (65, 128, 0, True, 0.0, (2, 0.5, 16)), (77, 128, 1, False, 0.0, (1, 0.0, 8)), (77, 64, 0, False, 0.5, (0, 0.0, 2)),
            (1000, 64, 2, True, 0.0, (1, 0.5, 0)), (1000, 128, 0, True, 0.0, (2, 0.0, 0))]
# fused glass_dual_linear_bwd_f32: (N, comb, kernels expected with split products / with f32 products)
BWD_64 = [(77, False), (1000, False), (100000, False), (100001, False), (77, True), (1000, True), (100000, True), (100001, True)]
# glass_comb_eff_fwd_f32, hidden 64: (N, list name, cap, stats, p_drop)
EFF_FWD_64 = ([(N, "batch", None, ("part", 0), 0.0) for N in ROWS_64] +
              [(77, "empty0", 0, ("part", 0), 0.0), (77, "empty", 64, ("part", 0), 0.5), (77, "row0", None, ("exact", 2), 0.0), (77, "last", None, ("part", 0), 0.0),
               (77, "middle", None, ("none", 0), 0.5), (1000, "n63", 128, ("part", 0), 0.0), (1000, "n64", 128, ("part", 0), 0.5), (1000, "n65", 128, ("exact", 4), 0.0),
               (1000, "tail_oob", 128, ("part", 0), 0.0), (77, "all", None, ("part", 0), 0.0), (1000, "wave16", None, ("part", 0), 0.5), (1000, "tile64", None, ("exact", 16), 0.0)])
# ... the launch forms: (N, list, cap, stats, p_drop, kernel family expected, rows_main)
EFF_FWD_FORMS = [(16385, "batch", 832, ("exact", 4), 0.0, "eff2", 80), (16385, "batch", 832, ("part", 0), 0.5, "eff2", 64), (20480, "empty0", 0, ("none", 0), 0.5, "eff2", 80),
                 (20480, "batch", 1024, ("part", 0), 0.0, "eff2", 64), (20481, "batch", 1088, ("part", 0), 0.0, "eff3", 96), (20481, "n65", 128, ("exact", 8), 0.5, "eff3", 96)]
# glass_comb_eff_bwd_f32: (N, list, cap, with_wgrad, gn = (gn_p_drop, exact n_rep) or None)
EFF_BWD_64 = [(77, "batch", None, False, None), (1000, "n65", 128, False, (0.0, 0)), (77, "all", None, True, (0.0, 0)), (1000, "batch", None, True, (0.5, 0)),
              (1000, "tail_oob", 128, True, (0.0, 4)), (1000, "empty", 64, True, None), (1000, "n64", 128, True, (0.5, 16)), (100001, "batch", 5056, True, (0.0, 0))]
# ... its dsrc_gn form (the fused launch only): (N, list, cap, (act, p_drop) of the GraphNorm behind the layer, addend, accumulate, n_rep)
EFF_BWD_GN = [(77, "batch", None, (0, 0.0), False, 0, 2), (1000, "n65", 128, (0, 0.5), True, 1, 4), (1000, "batch", None, (0, 0.5), True, 0, 16),
              (100000, "batch", None, (0, 0.0), False, 1, 8)]
# hidden 128: trans_fwd3 (N; rows_main leaves 64 at N = 16385), the trans data gradient (N, kernel with f32 products; 16441: the last
# workgroup gets a shorter, odd run of stages), comb_dgrad3 (N, density)
TRANS_FWD3 = (1, 63, 64, 65, 1000, 16384, 16385)
TRANS_DGRAD_128 = [(63, "trans_dgrad2_kernel<128>"), (1000, "trans_dgrad2_kernel<128>"), (16384, "trans_dgrad2_kernel<128>"), (16385, "trans_dgrad3_kernel<128>"),
                   (16441, "trans_dgrad3_kernel<128>")]
COMB_DGRAD3 = [(63, "none"), (63, "all"), (1000, "batch"), (1000, "all"), (16385, "batch"), (16385, "none")]
EFF_FWD_128 = [(16385, "batch", 832, ("exact", 8), 0.0), (16385, "batch", 832, ("none", 0), 0.5), (77, "batch", None, ("part", 0), 0.0), (1000, "n65", 128, ("exact", 4), 0.5), (20481, "batch", 1088, ("part", 0), 0.0), (20481, "n64", 128, ("exact", 2), 0.5)]


def named_kernels():
    """every kernel instantiation the case lists reach, from the restated dispatch alone -> set of names"""
    seen = set()
    for f32p in (False, True):
        for (N, f, *_r, stats, _g) in TRANS_FWD_SMALL:
            seen.add(fwd_form(64, False, N, stats[0] != "none", stats[1], f)["kernel"])
        for N, stats, _rows in TRANS_FWD_TALL:
            seen.add(fwd_form(64, False, N, stats[0] != "none", stats[1], f32p)["kernel"])
        for N in ROWS_64:
            seen.add(fwd_form(64, True, N, True, 0, f32p)["kernel"])
        for N, n_out, *_ in DGRAD_64:
            seen.update(dgrad_form(64, n_out, N, False, f32p)["kernels"])
        for N, comb in BWD_64:
            seen.update(dgrad_form(64, 128 if comb else 64, N, True, f32p)["kernels"])
        for N, _l, cap, stats, p in EFF_FWD_64 + [c[:5] for c in EFF_FWD_FORMS]:
            cap = label_list(_l, N, cap)[3]
            seen.add(comb_eff_fwd_form(64, N, cap, stats[0] != "none", stats[1], p, f32p)["kernel"])
        for N, _l, cap, wg, _gn in EFF_BWD_64:
            cap = label_list(_l, N, cap)[3]
            seen.update(comb_eff_bwd_form(N, cap, wg, f32p)["kernels"])
        for N, _l, cap, *_ in EFF_BWD_GN:
            seen.update(comb_eff_bwd_form(N, label_list(_l, N, cap)[3], True, f32p, dsrc_gn=True)["kernels"])
        for N in TRANS_FWD3:
            seen.add(fwd_form(128, False, N, True, 0, f32p)["kernel"])
        for N, _k in TRANS_DGRAD_128:
            seen.update(dgrad_form(128, 128, N, False, f32p)["kernels"])
        for N, _d in COMB_DGRAD3:
            seen.update(dgrad_form(128, 256, N, False, f32p)["kernels"])
        for N, _l, cap, stats, p in EFF_FWD_128:
            cap = label_list(_l, N, cap)[3]
            seen.add(comb_eff_fwd_form(128, N, cap, stats[0] != "none", stats[1], p, f32p)["kernel"])
    return {k for k in seen if k != "wgrad_reduce_kernel"}
