"""Host side of the tests of the weight-gradient family (K5w: glass_amd/csrc/linear.hip, wgrad_common.h, wgrad128.hip, wgrad_tiled.hip)
— torch fp64 and numpy on the CPU, no GPU: input recipes, the fp64 truth with the mass of EVERY element, the dispatch and the slab
geometry restated (tied to the source text by tests/test_wgrad_host.py), an fp32 restatement of the summation in both product forms
and the exact probes.

Scope.  glass_linear_wgrad_f32: the thin kernels wgrad_thin_partial_kernel<1|2|3> and the plain wgrad_partial_kernel<false,false>.
glass_dual_linear_wgrad_f32 for H % 64 == 0: wgrad_partial_kernel<true,false> / <true,true>, wgrad_partial_split_kernel<ACT,EFF> in its
three instantiations, wgrad128_trans_kernel, wgrad128_comb_kernel with its list tiles, tiled_wgrad_kernel<true,EFF,false>,
tiled_wgrad8_kernel<EFF> plus the four-wave labeled-rows launch, and the reduce launch behind each of them.

OUT OF SCOPE, not tested by these files: hidden <= 32 (dense_narrow.hip: tests of its own); the hidden-64 fused backward launches of
dense.hip and their S / L partials (glass_dual_linear_bwd_f32, glass_comb_eff_bwd_f32: tests/staged_dense_oracle.py, tests/test_gpu_staged_dense.py); glass_linear_wgrad_reduce_batch_f32 and
glass_wgrad_reduce_spmm_f32 beyond the deferred-reduce cases of tests/test_gpu_wgrad.py (tests/test_gpu_step_tail.py has them); the
non-eff fallback at rows_per_slab > 2 * kTile - 64, which needs more than 2 M rows.

Truth (fp64):  G[n,o] = coef(mask[n], o < H) * dsrc[n, o mod H] * act'(T[n,o]),  dW = G^T [X | X2],  db = sum_n G, with coef = z on
(labeled, first half) and (unlabeled, second half), else 1 - z, both as the entry rounds them to fp32; act' from the fp32 T the kernel
reads (T > 0 falls the same way: no kinks).  Mass of an element, by the form the restated dispatch names: plain form sum_n |G[n,o]|
|x[n,i]| (db: sum_n |G[n,o]|); effective-weight form |c_S| mass(S) + |c_L| mass(L) with S = dsrc^T [X | X2] over all rows, L over the
labeled rows, (c_S, c_L) = (1-z, 2z-1) for the first output half and (z, 1-2z) for the second; with accumulate |old| is added.  The
gate is |got - want| <= TOL * mass for every element (readout_oracle.gate, TOL = 1e-5), never per tensor.

fp32 restatement (restate_dual / restate_linear): the rows of a slab in the kernel's walking order — the four waves of the
register-pipelined kernels take interleaved row pairs (f32 products) or 16-row groups (split products) and are combined as (w0 + w2)
+ (w1 + w3); the LDS-staged kernels (wgrad128, tiled) own an output per wave and walk the slab in order —, the f32 form one fused
multiply-add per row, the split form six bf16 partial products per 16 (32: wgrad128) rows in the order of split_mma.h, each summed
exactly before the accumulator rounds; slabs summed in slab order; the effective-weight combine in fp32 with the header's z; thin
kernels: block partials (row slots, then slot order), then block order in fp64.  Not bit-exact with the GPU (the reduce kernels'
slot interleaving is not restated): it shows that the gate is satisfiable and that named mistakes are refused.

Exact probes (probe_recipe / probe_expect): all rows zero except <= 16 live rows; live row number k of the list has nonzero dsrc only
in outputs o = k (mod 16), so a dW row names the input row that fed it; dsrc = +-2^e, X = +-2^e (1 + 2^-10 + 2^-18) (one bit in each
bf16 piece, a span that survives a factor 0.25, 0.5, 0.75), z in {0.5, 0.75}, no activation or ReLU with T != 0: every element is ONE
product that fp32 holds exactly, in both product forms, so the expected value is bit for bit.  (Linear entry, O < 16: the live rows
are also told apart by input classes, in groups — probe_recipe_linear.)  probe_rows names the live rows a
geometry needs; probe_is_exact proves exactness for a form by running the restatement (where it is not, the case falls back to the
mass gate)."""
import os
import re

import numpy as np
import torch

from readout_oracle import TOL, gate  # noqa: F401  (re-exported)
from tiled_dense_oracle import SPLIT_ORDER, split3, _cdiv, ACT_NONE, ACT_ELU, ACT_RELU  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
f32 = np.float32
K_OT, K_IT, K_TILE, MAX_SLABS = 128, 64, 128 * 64, 256          # kOT, kIT, kTile, kMaxSlabs
THIN_MAX_O, THIN_MAX_BLOCKS = 3, 1024                           # kThinMaxO, kThinMaxBlocks
KWO, KWI, KWK = 128, 256, 16                                    # wgrad_tiled.hip
FUSED_MAX_ROWS = 100000                                         # kFusedBwdMaxRows
LIST_CAP = 3968                                                 # kW128ListCap
HEADER = 4                                                      # kWgradHeaderFloats = kWHeaderFloats
NARROW_MAX_H, NARROW_SLAB = 32, 64                              # dense_narrow.hip
SPLIT_WIDTHS = (128, 256, 512)                                  # tiled_shape_ok
# the shapes and row counts of tests/test_gpu_wgrad.py (tests/test_wgrad_host.py sweeps the workspace bytes over them: GPU_ROW_COUNTS below)
THIN_O, THIN_I, THIN_N = (1, 2, 3), (4, 20, 64, 256, 260), (1, 63, 64, 65, 65537)
PLAIN_SHAPES, PLAIN_N = ((4, 2), (40, 20), (128, 64), (132, 66), (256, 128)), (1, 5, 63, 64, 65)


def source_constants():
    """what the restatement depends on, read from the text of linear.hip, wgrad_common.h, wgrad128.hip, wgrad_tiled.hip"""
    rd = lambda n: open(os.path.join(ROOT, "glass_amd", "csrc", n)).read()
    lin, com, w128, til, nar, dt = rd("linear.hip"), rd("wgrad_common.h"), rd("wgrad128.hip"), rd("wgrad_tiled.hip"), rd("dense_narrow.hip"), rd("dense_tiled.hip")
    num = lambda pat, text: int(re.search(pat, text, re.S).group(1).replace(" ", ""))
    geom = re.search(r"WgradGeom wgrad_geom\(.*?\n}\n", lin, re.S).group(0)
    tgeom = re.search(r"TiledWgradGeom wgrad_tiled_geom\(.*?\n}\n", til, re.S).group(0)
    dual = re.search(r'extern "C" int glass_dual_linear_wgrad_f32\(.*?\n}\n', lin, re.S).group(0)
    plain = re.search(r'extern "C" int glass_linear_wgrad_f32\(.*?\n}\n', lin, re.S).group(0)
    wsb = re.search(r'extern "C" int64_t glass_linear_wgrad_ws_bytes\(.*?\n}\n', lin, re.S).group(0)
    k8 = re.search(r"void tiled_wgrad8_kernel\(.*?\n}\n", til, re.S).group(0)
    tl = re.search(r"void launch_tiled_wgrad_partial\(.*?\n}\n", til, re.S).group(0)
    return {
        "kOT": num(r"constexpr int kOT = (\d+);", com), "kIT": num(r"constexpr int kIT = (\d+);", com),
        "kTile_text": "constexpr int kTile = kOT * kIT;" in com, "kMaxSlabs": num(r"constexpr int kMaxSlabs = (\d+);", com),
        "kThinMaxO": num(r"constexpr int kThinMaxO = (\d+);", lin), "kThinMaxBlocks": num(r"constexpr int kThinMaxBlocks = (\d+);", lin),
        "kWO": num(r"constexpr int kWO = (\d+),", til), "kWI": num(r"kWI = (\d+),", til), "kWK": num(r"kWK = (\d+),", til),
        "kFusedBwdMaxRows": num(r"constexpr int64_t kFusedBwdMaxRows = (\d+);", com),
        "kW128ListCap": num(r"constexpr int kW128ListCap = (\d+);", w128),
        "header_floats": (num(r"constexpr int kWgradHeaderFloats = (\d+);", com), num(r"constexpr int kWHeaderFloats = (\d+);", til)),
        "narrow": (num(r"constexpr int kNarrowMaxH = (\d+);", nar), num(r"constexpr int kNarrowSlab = (\d+);", nar),
                   "*stride = (int)(ceil_div(O * I + O, 4) * 4);" in nar and "*n_slabs = (int)ceil_div(N, kNarrowSlab);" in nar),
        # the three *_shape predicates
        "wgrad128_shape_text": "bool wgrad128_shape(int64_t N, int64_t O, int64_t I) { return O == 256 && I == 128 && N >= 8192 && N <= kFusedBwdMaxRows * 4; }" in w128,
        "wgrad128_comb_shape_text": "bool wgrad128_comb_shape(int64_t N, int64_t O, int64_t I) { return O == 256 && I == 256 && N >= 8192 && N <= kFusedBwdMaxRows * 4; }" in w128,
        "tiled_shape_text": "bool wgrad_tiled_shape(int64_t N, int64_t O, int64_t I) { return O >= 512 && O % kWO == 0 && I % kWI == 0 && N >= 65536; }" in til,
        "split_widths_text": "bool tiled_shape_ok(int64_t H) { return H == 128 || H == 256 || H == 512; }" in dt,
        "comb_lists_text": all(s in w128 for s in ("int64_t n_l = ceil_div(N, (int64_t)kW128ListCap);", "if (n_l < 16) n_l = 16;")),
        "list_chunk_text": "const int64_t chunk = (N + n_l - 1) / n_l;" in w128,
        "thin_blocks_text": all(s in lin for s in ("const int64_t b = ceil_div(N, 64);", "return (int)(b < kThinMaxBlocks ? b : kThinMaxBlocks);")),
        "thin_entry_text": "if (O <= kThinMaxO && I % 4 == 0 && ldx % 4 == 0 && aligned16(X) && aligned16(ws)) {" in plain and
                           "const int rows = (int)ceil_div(N, nb);" in plain,
        "plain_refusal_text": "if (O % 4 || I % 2 || ldg % 4 || ldx % 2 || !aligned16(G) || (reinterpret_cast<uintptr_t>(X) & 7u)) {" in plain,
        # wgrad_geom
        "geom_comb128_text": all(s in geom for s in ("int64_t room = 256 - wgrad128_comb_lists(N);", "if (room < 64) room = 64;",
                                                     "int64_t rows = ceil_div(ceil_div(N, room), (int64_t)32) * 32;",
                                                     "if (g.n_slabs < wgrad128_comb_lists(N)) g.n_slabs = wgrad128_comb_lists(N);")),
        "geom_trans128_text": "int64_t rows = ceil_div(ceil_div(N, (int64_t)256), (int64_t)32) * 32;" in geom,
        "geom_generic_text": all(s in geom for s in (
            "const int64_t tiles = ceil_div(I, kIT) * ceil_div(O, kOT);", "int64_t max_slabs = kMaxSlabs / tiles;",
            "if (I == O && ceil_div(O, kOT) % 2 == 0) max_slabs *= 2;", "if (max_slabs > 128) max_slabs = 128;", "if (N <= 100000) {",
            "const int64_t room = (2 * 256 - 4 - ceil_div(N, 64)) / tiles;", "if (room >= 32) max_slabs = room < lim ? room : lim;",
            "if (max_slabs < 32) max_slabs = 32;", "int64_t rows = ceil_div(N, max_slabs);", "rows = ceil_div(rows, 8) * 8;",
            "if (N <= kFusedBwdMaxRows) rows = ceil_div(rows, tiles == 1 ? 32 : 16) * (tiles == 1 ? 32 : 16);",
            "g.part_b_floats = (int64_t)g.n_slabs * g.nz * kOT + kWgradHeaderFloats;")) and geom.count("if (rows < 64) rows = 64;") == 3,
        "tiled_geom_text": all(s in tgeom for s in (
            "int64_t slabs = ceil_div(512, (int64_t)g.ny * g.nz);", "if (I == O) slabs *= 2;", "if (slabs > 256) slabs = 256;",
            "int64_t rows = ceil_div(ceil_div(N, slabs), kWK) * kWK;", "g.part_b_floats = (int64_t)g.n_slabs * g.nz * kWO + kWHeaderFloats;")),
        "ws_bytes_text": all(s in wsb for s in ("if (O <= kThinMaxO && (int64_t)thin_blocks(N) * (O * I + O) > floats)",
                                                "if (O <= 2 * 32 && I <= 2 * 32) {", "if (wgrad_tiled_shape(N, O, I)) {")),
        # the entry's conditions
        "eff_cond_text": "const bool eff = X2 != nullptr && act == GLASS_ACT_NONE && I == O && O == 2 * H && g.nz % 2 == 0 &&" in dual and
                         "g.rows_per_slab <= 2 * kTile - 64;" in dual,
        "split_cond_text": "const bool split = tiled_shape_ok(H) && tiled_split_products() && ldx % 2 == 0;" in dual,
        "dual_refusal_text": "if (H % 64 || ldd % 4 || ldx % 2 || (X2 && ldx2 % 2) || !aligned16(dsrc) ||" in dual,
        "route_chain_text": [m for m in re.findall(r"(launch_wgrad128_trans|launch_wgrad128_comb|wgrad_partial_split_kernel<\w+, \w+>|wgrad_partial_kernel<\w+, \w+>)\)?[,(]", dual)],
        "tiled_eff_cond_text": "const bool eff = sy.X2 != nullptr && sy.act == GLASS_ACT_NONE && I == O && g.nz % 2 == 0 && O == 2 * (int64_t)sy.H;" in tl,
        "tiled_refusals_text": all(s in dual for s in ("if (ldx % 4 || !aligned16(X) || (X2 && (ldx2 % 4 || !aligned16(X2)))) {",
                                                       "if (reinterpret_cast<uintptr_t>(mask) & 1u) {",
                                                       "if (((int64_t)t.rows_per_slab + 6 * 16) * ldmax * 4 >= (int64_t)1 << 31) {")),
        "placement_text": all(s in k8 for s in ("if (n_slabs % 8 == 0) {", "const int c = lin & 7, m = lin >> 3;", "bx = c + 8 * (m / T);")),
        "split_order": re.findall(r"GLASS_SMMA\((\d), (\d)\);", rd("split_mma.h")),
    }


ROUTE_CHAIN = ["launch_wgrad128_trans", "launch_wgrad128_comb", "wgrad_partial_split_kernel<false, true>", "wgrad_partial_split_kernel<true, false>",
               "wgrad_partial_split_kernel<false, false>", "wgrad_partial_kernel<true, true>", "wgrad_partial_kernel<true, false>"]


# ---- geometry restated ----------------------------------------------------------------------------------------------------------------
def wgrad128_shape(N, O, I):
    return O == 256 and I == 128 and 8192 <= N <= FUSED_MAX_ROWS * 4


def wgrad128_comb_shape(N, O, I):
    return O == 256 and I == 256 and 8192 <= N <= FUSED_MAX_ROWS * 4


def wgrad128_comb_lists(N):
    return max(_cdiv(N, LIST_CAP), 16)


def wgrad_tiled_shape(N, O, I):
    return O >= 512 and O % KWO == 0 and I % KWI == 0 and N >= 65536


def thin_blocks(N):
    return min(_cdiv(N, 64), THIN_MAX_BLOCKS)


def wgrad_geom(N, O, I):
    ny, nz = _cdiv(I, K_IT), _cdiv(O, K_OT)
    if wgrad128_comb_shape(N, O, I):
        room = max(256 - wgrad128_comb_lists(N), 64)
        rows = max(_cdiv(_cdiv(N, room), 32) * 32, 64)
        n_slabs = max(_cdiv(N, rows), wgrad128_comb_lists(N))
    elif wgrad128_shape(N, O, I):
        rows = max(_cdiv(_cdiv(N, 256), 32) * 32, 64)
        n_slabs = _cdiv(N, rows)
    else:
        tiles = ny * nz
        max_slabs = MAX_SLABS // tiles
        if I == O and nz % 2 == 0:
            max_slabs *= 2
        lim = max_slabs
        max_slabs = min(max_slabs, 128)
        if N <= 100000:
            room = int((2 * 256 - 4 - _cdiv(N, 64)) / tiles)       # C division truncates toward zero
            if room >= 32:
                max_slabs = min(room, lim)
        max_slabs = max(max_slabs, 32)
        rows = max(_cdiv(N, max_slabs), 64)
        rows = _cdiv(rows, 8) * 8
        if N <= FUSED_MAX_ROWS:
            q = 32 if tiles == 1 else 16
            rows = _cdiv(rows, q) * q
        n_slabs = _cdiv(N, rows)
    return dict(rows=rows, n_slabs=n_slabs, ny=ny, nz=nz, part_w=n_slabs * ny * nz * K_TILE, part_b=n_slabs * nz * K_OT + HEADER)


def wgrad_tiled_geom(N, O, I):
    ny, nz = I // KWI, O // KWO
    slabs = _cdiv(512, ny * nz)
    if I == O:
        slabs *= 2
    slabs = min(slabs, 256)
    rows = _cdiv(_cdiv(N, slabs), KWK) * KWK
    n_slabs = _cdiv(N, rows)
    return dict(rows=rows, n_slabs=n_slabs, ny=ny, nz=nz, part_w=n_slabs * ny * nz * KWO * KWI, part_b=n_slabs * nz * KWO + HEADER)


def ws_bytes(N, O, I):
    g = wgrad_geom(N, O, I)
    floats = g["part_w"] + g["part_b"]
    if O <= THIN_MAX_O:
        floats = max(floats, thin_blocks(N) * (O * I + O))
    if O <= 2 * NARROW_MAX_H and I <= 2 * NARROW_MAX_H:
        floats = max(floats, _cdiv(N, NARROW_SLAB) * _cdiv(O * I + O, 4) * 4)
    if wgrad_tiled_shape(N, O, I):
        t = wgrad_tiled_geom(N, O, I)
        floats = max(floats, t["part_w"] + t["part_b"])
    return 4 * floats


def route(entry, N, shape, comb=False, act=ACT_NONE, f32_products=False, aligned4=True, fits32=True):
    """the launches one call takes and their geometry.  entry "linear": shape = (O, I); entry "dual": shape = H.  aligned4: X (and X2)
    16-byte aligned with ld % 4 == 0; fits32: N * max(ld) * 4 < 2^31.  -> dict kernels (in launch order, the reduce last), family,
    rows (per slab / per thin block), n_slabs, ny, nz, n_lists, thin_blocks, eff, split, placement, ws_bytes"""
    if entry == "linear":
        O, I = shape
        out = dict(eff=False, split=False, n_lists=0, thin_blocks=0, placement=None, ws_bytes=ws_bytes(N, O, I), O=O, I=I)
        if O <= THIN_MAX_O and I % 4 == 0 and aligned4:
            nb = thin_blocks(N)
            return dict(out, family="thin", kernels=[f"wgrad_thin_partial_kernel<{O}>", "wgrad_thin_reduce_kernel"], thin_blocks=nb,
                        rows=_cdiv(N, nb), n_slabs=nb, ny=1, nz=1)
        assert O % 4 == 0 and I % 2 == 0, "GLASS_E_UNSUPPORTED"
        g = wgrad_geom(N, O, I)
        return dict(out, family="generic", kernels=["wgrad_partial_kernel<false, false>", "wgrad_reduce_kernel"], **{k: g[k] for k in ("rows", "n_slabs", "ny", "nz")})
    H = shape
    assert entry == "dual" and H % 64 == 0, "hidden <= 32 (dense_narrow.hip) and H % 64 != 0 are out of scope / unsupported"
    O, I = 2 * H, (2 * H if comb else H)
    out = dict(n_lists=0, thin_blocks=0, placement=None, ws_bytes=ws_bytes(N, O, I), O=O, I=I)
    split = H in SPLIT_WIDTHS and not f32_products
    if wgrad_tiled_shape(N, O, I):
        assert aligned4, "GLASS_E_UNSUPPORTED"
        g = wgrad_tiled_geom(N, O, I)
        eff = comb and act == ACT_NONE and I == O and g["nz"] % 2 == 0
        e = "true" if eff else "false"
        if split:
            ks = [f"tiled_wgrad8_kernel<{e}>"] + (["tiled_wgrad_kernel<true, true, true>"] if eff else [])
            placement = "xcd" if g["n_slabs"] % 8 == 0 else "plain"
        else:
            ks, placement = [f"tiled_wgrad_kernel<true, {e}, false>"], None
        return dict(out, family="tiled", kernels=ks + ["tiled_wgrad_reduce_kernel"], eff=eff, split=split, placement=placement,
                    **{k: g[k] for k in ("rows", "n_slabs", "ny", "nz")})
    g = wgrad_geom(N, O, I)
    eff = comb and act == ACT_NONE and I == O and g["nz"] % 2 == 0 and g["rows"] <= 2 * K_TILE - 64
    e, a = ("true" if eff else "false"), ("true" if act != ACT_NONE else "false")
    family, n_lists = "generic", 0
    if split and not eff and not comb and wgrad128_shape(N, O, I) and aligned4 and fits32:
        k, family = "wgrad128_trans_kernel", "wgrad128"
    elif split and eff and wgrad128_comb_shape(N, O, I) and aligned4 and fits32:
        k, family, n_lists = "wgrad128_comb_kernel", "wgrad128", wgrad128_comb_lists(N)
    elif split:
        k = f"wgrad_partial_split_kernel<{'false' if eff else a}, {e}>"
    else:
        k = f"wgrad_partial_kernel<true, {e}>"
    return dict(out, family=family, kernels=[k, "wgrad_reduce_kernel"], eff=eff, split=split, n_lists=n_lists,
                **{kk: g[kk] for kk in ("rows", "n_slabs", "ny", "nz")})


def slab_bounds(form, N):
    """[(r0, r1)] of the slabs that hold rows"""
    return [(s * form["rows"], min(N, (s + 1) * form["rows"])) for s in range(form["n_slabs"]) if s * form["rows"] < N]


def list_chunks(form, N):
    """[(c0, c1)] of the list workgroups of wgrad128_comb_kernel"""
    n_l = form["n_lists"]
    ch = _cdiv(N, n_l)
    return [(k * ch, min(N, (k + 1) * ch)) for k in range(n_l)]


# ---- the cases of tests/test_gpu_wgrad.py (tests/test_wgrad_host.py restates those the CPU can hold) ----------------------------------
ROUTES = {   # name: (H, comb, act, N, first kernel with split products, with f32 products)
    "g64 trans": (64, False, 1, 333, None, "wgrad_partial_kernel<true, false>"),
    "g64 trans none": (64, False, 0, 333, None, "wgrad_partial_kernel<true, false>"),
    "g64 trans relu": (64, False, 2, 333, None, "wgrad_partial_kernel<true, false>"),
    "g64 comb": (64, True, 0, 333, None, "wgrad_partial_kernel<true, false>"),
    "g64 comb elu": (64, True, 1, 333, None, "wgrad_partial_kernel<true, false>"),
    "g192 comb": (192, True, 0, 333, None, "wgrad_partial_kernel<true, false>"),
    "g320 comb": (320, True, 0, 200, None, "wgrad_partial_kernel<true, false>"),
    "g128 trans": (128, False, 1, 3001, "wgrad_partial_split_kernel<true, false>", "wgrad_partial_kernel<true, false>"),
    "g128 trans none": (128, False, 0, 3001, "wgrad_partial_split_kernel<false, false>", "wgrad_partial_kernel<true, false>"),
    "g128 comb": (128, True, 0, 3001, "wgrad_partial_split_kernel<false, true>", "wgrad_partial_kernel<true, true>"),
    "g128 trans 400k": (128, False, 0, 400001, "wgrad_partial_split_kernel<false, false>", "wgrad_partial_kernel<true, false>"),
    "g128 comb 400k": (128, True, 0, 400001, "wgrad_partial_split_kernel<false, true>", "wgrad_partial_kernel<true, true>"),
    "g256 trans": (256, False, 2, 4099, "wgrad_partial_split_kernel<true, false>", "wgrad_partial_kernel<true, false>"),
    "g256 comb": (256, True, 0, 4099, "wgrad_partial_split_kernel<false, true>", "wgrad_partial_kernel<true, true>"),
    "w128 trans": (128, False, 1, 8193, "wgrad128_trans_kernel", "wgrad_partial_kernel<true, false>"),
    "w128 comb": (128, True, 0, 8193, "wgrad128_comb_kernel", "wgrad_partial_kernel<true, true>"),
    "t256 trans": (256, False, 1, 65553, "tiled_wgrad8_kernel<false>", "tiled_wgrad_kernel<true, false, false>"),
    "t256 comb": (256, True, 0, 65553, "tiled_wgrad8_kernel<true>", "tiled_wgrad_kernel<true, true, false>"),
    "t512 trans": (512, False, 0, 65576, "tiled_wgrad8_kernel<false>", "tiled_wgrad_kernel<true, false, false>"),
    "t512 comb": (512, True, 0, 65576, "tiled_wgrad8_kernel<true>", "tiled_wgrad_kernel<true, true, false>"),
}
# further row counts per route: a whole last slab and one row into the next slab (hidden 128 at 64-row slabs, hidden 256 at 144-row
# slabs); hidden 128 beyond the wgrad128 kernels' 400 000 rows: 64 slabs of 6 256 rows with the last one row short (400 383) and whole
# (400 384) — one row more and wgrad_geom takes 6 264-row slabs (400 385) —; both ends of the wgrad128 range; 128 slabs at hidden 256
EXTRA_ROWS = ([(n, N) for n in ("g128 trans", "g128 comb") for N in (3008, 3009)] + [(n, N) for n in ("g256 trans", "g256 comb") for N in (4176, 4177)] +
              [(n, N) for n in ("g128 trans 400k", "g128 comb 400k") for N in (400383, 400384, 400385)] +
              [(n, N) for n in ("w128 trans", "w128 comb") for N in (8192, 50003)] + [("t256 trans", 71680), ("t256 comb", 71680)])
LIST_ROWS = (50003, 63488, 63489, 8193)      # test_wgrad128_comb_list_tiles_at_the_chunk_boundaries


def plain_rows(O, I):
    """the row counts of the plain kernel's cases: (128, 64) adds one slab edge - 1 / 0 / + 1 and both sides of kFusedBwdMaxRows"""
    if (O, I) != (128, 64):
        return list(PLAIN_N)
    rows = wgrad_geom(333, O, I)["rows"]
    return list(PLAIN_N) + [3 * rows - 1, 3 * rows, 3 * rows + 1, 100000, 100001]


GPU_ROW_COUNTS = tuple(sorted(set(THIN_N) | {n for s in PLAIN_SHAPES for n in plain_rows(*s)} | {r[3] for r in ROUTES.values()} |
                              {n for _, n in EXTRA_ROWS} | set(LIST_ROWS)))


# ---- recipes --------------------------------------------------------------------------------------------------------------------------
PATTERNS = ("none", "all", "last", "slab_first", "slab_whole", "per_slab", "stage16")


def label_pattern(name, N, form):
    """label bytes [N]: none; all; only row N - 1; only the first row of a slab (the middle one); one whole slab; one row per slab
    (moving through the slab); every row of one 16-row stage (the second of the middle slab, clipped at N)"""
    m = np.zeros(N, dtype=np.uint8)
    b = slab_bounds(form, N) if form["family"] != "thin" else [(0, N)]
    r0, r1 = b[len(b) // 2]
    if name == "all":
        m[:] = 1
    elif name == "last":
        m[N - 1] = 1
    elif name == "slab_first":
        m[r0] = 1
    elif name == "slab_whole":
        m[r0:r1] = 1
    elif name == "per_slab":
        for s, (a, e) in enumerate(b):
            m[a + (5 * s + 3) % (e - a)] = 1
    elif name == "stage16":
        m[min(r0 + 16, r1 - 1):min(r0 + 32, r1)] = 1
    else:
        assert name == "none"
    return m


def random_mask(N, seed, density=0.3):
    return (torch.rand(N, generator=torch.Generator().manual_seed(seed)) < density).numpy().astype(np.uint8)


def recipe(N, H, comb, seed=0):
    """fp32 inputs of one dual call: dsrc [N, H], T [N, 2H] (both signs), X (+ 0.25: column sums do not cancel to nothing), X2"""
    g = torch.Generator().manual_seed(7919 * H + 31 * N + 7 * seed + int(comb))
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(N=N, H=H, comb=comb, dsrc=r(N, H), T=r(N, 2 * H) * 1.5, X=r(N, H) + 0.25, X2=(r(N, H) - 0.25) if comb else None)


def recipe_linear(N, O, I, seed=0):
    g = torch.Generator().manual_seed(104729 * O + 613 * I + N + seed)
    return dict(N=N, O=O, I=I, G=torch.randn(N, O, generator=g), X=torch.randn(N, I, generator=g) + 0.25)


# ---- the fp64 truth -------------------------------------------------------------------------------------------------------------------
def zw(z):
    return float(f32(z)), float(f32(1.0 - z))


def synth_G(dsrc, T, mask, z, act, device="cpu"):
    """G [N, 2H] fp64"""
    zr, omz = zw(z)
    d = dsrc.to(device).to(F64)
    lab = torch.as_tensor(np.asarray(mask)).to(device).bool().reshape(-1, 1)
    c1 = torch.where(lab, torch.tensor(zr, dtype=F64, device=device), torch.tensor(omz, dtype=F64, device=device))
    c0 = torch.where(lab, torch.tensor(omz, dtype=F64, device=device), torch.tensor(zr, dtype=F64, device=device))
    G = torch.cat([c1 * d, c0 * d], 1)
    if act != ACT_NONE:
        t = T.to(device).to(F64)
        G = G * torch.where(t > 0, torch.ones_like(t), torch.exp(t) if act == ACT_ELU else torch.zeros_like(t))
    return G


def truth_linear(G, X, old_W=None, old_b=None, device="cpu"):
    """-> dW, dW mass, db, db mass (fp64, on the CPU)"""
    G, X = G.to(device).to(F64), X.to(device).to(F64)
    dW, mW, db, mb = G.t() @ X, G.abs().t() @ X.abs(), G.sum(0), G.abs().sum(0)
    if old_W is not None:
        dW, mW = dW + old_W.to(device).to(F64), mW + old_W.to(device).to(F64).abs()
    if old_b is not None:
        db, mb = db + old_b.to(device).to(F64), mb + old_b.to(device).to(F64).abs()
    return dW.cpu(), mW.cpu(), db.cpu(), mb.cpu()


def truth_dual(dsrc, T, mask, z, act, X, X2, eff, old_W=None, old_b=None, device="cpu"):
    """-> dW [2H, I], its mass, db [2H], its mass; the mass of the form (`eff`) the restated dispatch names"""
    G = synth_G(dsrc, T, mask, z, act, device)
    Xin = X.to(device).to(F64) if X2 is None else torch.cat([X.to(device).to(F64), X2.to(device).to(F64)], 1)
    dW, db = G.t() @ Xin, G.sum(0)
    if not eff:
        mW, mb = G.abs().t() @ Xin.abs(), G.abs().sum(0)
    else:
        zr, _ = zw(z)
        d = dsrc.to(device).to(F64).abs()
        lab = torch.as_tensor(np.asarray(mask)).to(device).bool()
        mS, mL = d.t() @ Xin.abs(), d[lab].t() @ Xin[lab].abs()
        bS, bL = d.sum(0), d[lab].sum(0)
        c = ((abs(1 - zr), abs(2 * zr - 1)), (abs(zr), abs(1 - 2 * zr)))
        mW = torch.cat([c[0][0] * mS + c[0][1] * mL, c[1][0] * mS + c[1][1] * mL], 0)
        mb = torch.cat([c[0][0] * bS + c[0][1] * bL, c[1][0] * bS + c[1][1] * bL], 0)
    if old_W is not None:
        dW, mW = dW + old_W.to(device).to(F64), mW + old_W.to(device).to(F64).abs()
    if old_b is not None:
        db, mb = db + old_b.to(device).to(F64), mb + old_b.to(device).to(F64).abs()
    return dW.cpu(), mW.cpu(), db.cpu(), mb.cpu()


# ---- the fp32 restatement -------------------------------------------------------------------------------------------------------------
def _fl(x):
    return np.asarray(x, dtype=np.float64).astype(f32)


def _sum_rows(Gr, Xr, split, waves, unit, mut=None):
    """rows of one slab in walking order, Gr [n, O], Xr [n, I] fp32 -> (fp32 [O, I], fp32 [O]).  `waves` accumulators take interleaved
    units of `unit` rows (f32 form: one fused multiply-add per row; split form: the unit's six partial products, each summed exactly)
    and are combined (w0 + w2) + (w1 + w3)."""
    n, O, I = Gr.shape[0], Gr.shape[1], Xr.shape[1]
    steps = max(_cdiv(n, waves * unit), 1)
    pad = steps * waves * unit - n
    Gp = np.concatenate([Gr, np.zeros((pad, O), f32)]).reshape(steps, waves, unit, O)
    Xp = np.concatenate([Xr, np.zeros((pad, I), f32)]).reshape(steps, waves, unit, I)
    acc = np.zeros((waves, O, I), f32)
    bs = np.zeros((waves, O), f32)
    if split:
        ga, xb = [p.reshape(Gp.shape).astype(np.float64) for p in split3(Gp)], [p.reshape(Xp.shape).astype(np.float64) for p in split3(Xp)]
        if mut == "drop_lo_x":
            xb[2] = np.zeros_like(xb[2])
    for s in range(steps):
        if split:
            for pa, pb in SPLIT_ORDER:
                if mut == "drop_mid_hi" and (pa, pb) == (0, 1):
                    continue
                acc = _fl(acc + np.einsum("wko,wki->woi", ga[pa][s], xb[pb][s]))
        else:
            g64, x64 = Gp[s].astype(np.float64), Xp[s].astype(np.float64)
            for u in range(unit):
                acc = _fl(acc + g64[:, u, :, None] * x64[:, u, None, :])
        for u in range(unit):
            bs = (bs + Gp[s][:, u]).astype(f32)
    if waves == 4:
        return ((acc[0] + acc[2]).astype(f32) + (acc[1] + acc[3]).astype(f32)).astype(f32), ((bs[0] + bs[1]).astype(f32) + (bs[2] + bs[3]).astype(f32)).astype(f32)
    return acc[0], bs[0]


def _walk(form):
    """(waves, unit) of the partial kernel of a form"""
    if form["family"] == "generic":
        return (4, 16) if form["split"] else (4, 2)
    if form["family"] == "wgrad128":
        return (1, 32)
    return (1, 16)


MUTANTS = ("drop_slab_last_row", "row_past_N", "slab_first_row_twice", "label_as_unlabeled", "swap_cs_cl", "L_all_rows", "bias_tile1_to_tile0",
           "accumulate_overwrites", "swap_input_halves", "drop_lo_x", "drop_mid_hi", "swap_pair_in_tile")
PROBE_MUTANTS = ("drop_lo_x", "drop_mid_hi", "swap_pair_in_tile")


def _finish(dW, db, old_W, old_b, mut):
    """the reduce's tail: mistakes of placement, then accumulate"""
    if mut == "bias_tile1_to_tile0" and db.shape[0] >= 2 * K_OT:
        db = db.copy()
        db[:K_OT], db[K_OT:2 * K_OT] = db[K_OT:2 * K_OT].copy(), 0
    if mut == "swap_input_halves" and dW.shape[1] >= 2 * K_IT:
        dW = dW.copy()
        dW[:, :K_IT], dW[:, K_IT:2 * K_IT] = dW[:, K_IT:2 * K_IT].copy(), dW[:, :K_IT].copy()
    if mut == "swap_pair_in_tile":   # two elements of one 128 x 64 tile that no row / column sum tells apart from afar: neighbours
        dW = dW.copy()
        o, i = [int(v[0]) for v in np.nonzero(dW[:, :-1] != dW[:, 1:])]   # (the first neighbours that hold two different values)
        dW[o, i], dW[o, i + 1] = dW[o, i + 1], dW[o, i]
    if old_W is not None and mut != "accumulate_overwrites":
        dW = (dW + np.asarray(old_W, f32)).astype(f32)
    if old_b is not None and mut != "accumulate_overwrites":
        db = (db + np.asarray(old_b, f32)).astype(f32)
    return dW, db


def _slab_rows(form, N, mut):
    """row index lists per slab, with the row-range mistakes applied to the middle slab"""
    b = slab_bounds(form, N)
    out = [list(range(a, e)) for a, e in b]
    mid = len(b) // 2
    if mut == "drop_slab_last_row":
        out[mid] = out[mid][:-1]
    elif mut == "row_past_N":
        out[-1] = out[-1] + [N]
    elif mut == "slab_first_row_twice" and len(b) > 1:
        s = max(mid, 1)
        out[s - 1] = out[s - 1] + [b[s][0]]
    return out


def restate_linear(form, G, X, N, old_W=None, old_b=None, mut=None):
    """glass_linear_wgrad_f32 in fp32 -> dW [O, I], db [O].  G, X may hold one row more than N (what a row past N would add)."""
    G, X = np.asarray(G, f32), np.asarray(X, f32)
    O, I = G.shape[1], X.shape[1]
    if form["family"] == "thin":
        tc = 1
        while tc < min(I // 4, 64):   # pow2_ceil_cap(I / 4, 64) lanes over the input columns, the rest of the 256 threads are row slots
            tc *= 2
        n_slot = 256 // tc
        W64, b64 = np.zeros((O, I)), np.zeros(O)
        for idx in _slab_rows(form, N, mut):   # (a thin block is a slab of form["rows"] rows)
            w, bsum = _thin_block(G[idx], X[idx], n_slot)
            W64, b64 = W64 + w, b64 + bsum
        return _finish(W64.astype(f32), b64.astype(f32), old_W, old_b, mut)
    dW, db = np.zeros((O, I), f32), np.zeros(O, f32)
    for idx in _slab_rows(form, N, mut):
        w, bsum = _sum_rows(G[idx], X[idx], False, 4, 2)
        dW, db = (dW + w).astype(f32), (db + bsum).astype(f32)
    return _finish(dW, db, old_W, old_b, mut)


def _thin_block(Gr, Xr, n_slot):
    """one block of the thin kernel: row slot s takes rows s, s + n_slot, ... (fused multiply-add chain), slots summed in order"""
    n, O, I = Gr.shape[0], Gr.shape[1], Xr.shape[1]
    steps = _cdiv(n, n_slot)
    pad = steps * n_slot - n
    Gp = np.concatenate([Gr, np.zeros((pad, O), f32)]).reshape(steps, n_slot, O).astype(np.float64)
    Xp = np.concatenate([Xr, np.zeros((pad, I), f32)]).reshape(steps, n_slot, I).astype(np.float64)
    acc, bs = np.zeros((n_slot, O, I), f32), np.zeros((n_slot, O), f32)
    for s in range(steps):
        acc = _fl(acc + Gp[s][:, :, None] * Xp[s][:, None, :])
        bs = _fl(bs + Gp[s])
    w, b = np.zeros((O, I), f32), np.zeros(O, f32)
    for t in range(n_slot):
        w, b = (w + acc[t]).astype(f32), (b + bs[t]).astype(f32)
    return w.astype(np.float64), b.astype(np.float64)


def restate_dual(form, dsrc, T, mask, z, act, X, X2, N, old_W=None, old_b=None, mut=None):
    """glass_dual_linear_wgrad_f32 in fp32 -> dW [2H, I], db [2H].  The operands may hold one row more than N."""
    d, X = np.asarray(dsrc, f32), np.asarray(X, f32)
    Xin = X if X2 is None else np.concatenate([X, np.asarray(X2, f32)], 1)
    H = d.shape[1]
    zr, omz = f32(z), f32(1.0 - z)
    lab = np.zeros(d.shape[0], bool)
    lab[:N] = np.asarray(mask)[:N].astype(bool)
    waves, unit = _walk(form)
    slabs = _slab_rows(form, N, mut)
    if not form["eff"]:
        lab_c = lab.copy()
        if mut == "label_as_unlabeled" and lab_c.any():
            lab_c[np.nonzero(lab_c)[0][0]] = False
        c1, c0 = np.where(lab_c, zr, omz).astype(f32)[:, None], np.where(lab_c, omz, zr).astype(f32)[:, None]
        G = np.concatenate([(d * c1).astype(f32), (d * c0).astype(f32)], 1)
        if act != ACT_NONE:
            t = np.asarray(T, f32)
            with np.errstate(all="ignore"):
                G = (G * np.where(t > 0, f32(1), np.exp(t.astype(np.float64)).astype(f32) if act == ACT_ELU else f32(0)).astype(f32)).astype(f32)
        dW, db = np.zeros((2 * H, Xin.shape[1]), f32), np.zeros(2 * H, f32)
        for idx in slabs:
            w, bsum = _sum_rows(G[idx], Xin[idx], form["split"], waves, unit, mut)
            dW, db = (dW + w).astype(f32), (db + bsum).astype(f32)
        return _finish(dW, db, old_W, old_b, mut)
    # effective-weight form: S over all rows, L over the labeled rows (per slab, or per list chunk), the combine from the header's z
    S, Sb = np.zeros((H, Xin.shape[1]), f32), np.zeros(H, f32)
    L, Lb = S.copy(), Sb.copy()
    for idx in slabs:
        w, bsum = _sum_rows(d[idx], Xin[idx], form["split"], waves, unit, mut)
        S, Sb = (S + w).astype(f32), (Sb + bsum).astype(f32)
    lab_l = lab.copy()
    if mut == "label_as_unlabeled" and lab_l.any():
        lab_l[np.nonzero(lab_l)[0][0]] = False
    if mut == "L_all_rows":
        lab_l[:N] = True
    groups = [list(range(a, e)) for a, e in list_chunks(form, N)] if form["n_lists"] else slabs
    for idx in groups:
        idx = [r for r in idx if lab_l[r]]
        if idx:
            w, bsum = _sum_rows(d[idx], Xin[idx], form["split"], waves, unit, mut)
            L, Lb = (L + w).astype(f32), (Lb + bsum).astype(f32)
    one, two = f32(1), f32(2)
    cs1, cl1, cs0, cl0 = f32(one - zr), f32(two * zr - one), zr, f32(one - two * zr)
    if mut == "swap_cs_cl":
        cs1, cl1, cs0, cl0 = cs0, cl0, cs1, cl1
    mix = lambda cs, cl, s, l: _fl(_fl(cs * s.astype(np.float64)).astype(np.float64) + _fl(cl * l.astype(np.float64)))
    dW = np.concatenate([mix(cs1, cl1, S, L), mix(cs0, cl0, S, L)], 0)
    db = np.concatenate([mix(cs1, cl1, Sb, Lb), mix(cs0, cl0, Sb, Lb)], 0)
    return _finish(dW, db, old_W, old_b, mut)


# ---- exact probes -----------------------------------------------------------------------------------------------------------------------
PROBE_Z = (0.5, 0.75)


def probe_rows(form, N):
    """the live rows a geometry needs (<= 16, ascending): first and last row of the first, a middle and the last slab, the first row
    behind the middle slab (with its last row: the pair that straddles the slab end), row N - 1 (the last row of a ragged 16- or
    32-row stage whenever N is no multiple of it), the last row of the first 16-row stage"""
    b = slab_bounds(form, N) if form["family"] != "thin" else [(s * form["rows"], min(N, (s + 1) * form["rows"])) for s in range(form["thin_blocks"]) if s * form["rows"] < N]
    rows = {N - 1, min(15, N - 1)}
    for a, e in (b[0], b[len(b) // 2], b[-1]):
        rows |= {a, e - 1, min(e, N - 1)}
    rows = sorted(rows)
    assert len(rows) <= 16
    return rows


def probe_masks(live, N):
    """two label vectors: the live rows labeled alternately, and the other way round (every live row is seen labeled and unlabeled)"""
    a, b = np.zeros(N, np.uint8), np.zeros(N, np.uint8)
    for k, r in enumerate(live):
        (a if k % 2 == 0 else b)[r] = 1
    return a, b


def _h(*v):
    x = 0x9E3779B1
    for t in v:
        x = ((x ^ (int(t) + 0x7F4A7C15)) * 0x85EBCA6B) & 0xFFFFFFFF
        x ^= x >> 13
    return x


def probe_recipe(N, H, comb, live, relu=False, seed=0):
    """-> dict dsrc, T, X, X2 (torch fp32).  Zero everywhere except the live rows."""
    live = list(live)
    assert len(live) <= 16 and len(set(live)) == len(live)
    d, X = np.zeros((N, H), f32), np.zeros((N, H), f32)
    X2 = np.zeros((N, H), f32) if comb else None
    T = np.zeros((N, 2 * H), f32)
    m = f32(1 + 2.0**-10 + 2.0**-18)
    for k, r in enumerate(live):
        for o in range(k, H, 16):
            d[r, o] = (-1.0 if _h(seed, r, o) & 1 else 1.0) * 2.0**((_h(seed, r, o, 1) % 3) - 1)
        for i in range(H):
            X[r, i] = (-1.0 if _h(seed, r, i, 2) & 1 else 1.0) * 2.0**((_h(seed, r, i, 3) % 5) - 2) * m
            if comb:
                X2[r, i] = (-1.0 if _h(seed, r, i, 4) & 1 else 1.0) * 2.0**((_h(seed, r, i, 5) % 5) - 2) * m
        for o in range(2 * H):
            T[r, o] = -1.0 if _h(seed, r, o, 6) % 3 == 0 else 1.0
    t = lambda a: None if a is None else torch.from_numpy(a)
    return dict(N=N, H=H, comb=comb, dsrc=t(d), T=t(T) if relu else None, X=t(X), X2=t(X2), act=ACT_RELU if relu else ACT_NONE)


def probe_groups_linear(live, O, I):
    """the live rows in groups one linear probe can hold: min(O, 16) output classes x min(I, 16) input classes"""
    cap = min(O, 16) * min(I, 16)
    live = list(live)
    return [live[k:k + cap] for k in range(0, len(live), cap)]


def probe_recipe_linear(N, O, I, live, seed=0):
    """live row number k owns the cells (o, i) with o = k mod Oc (mod Oc) and i = k div Oc (mod Ic), Oc = min(O, 16), Ic = the number
    of input classes the group needs: with O >= 16 a dW row names its input row, with the thin kernels' O <= 3 the input columns tell
    the live rows apart, so that every live row feeds elements of dW.  (db[o] sums the rows of class o: +-2^e, exact in any order.)"""
    live = list(live)
    Oc = min(O, 16)
    Ic = max(_cdiv(len(live), Oc), 1)
    assert Ic <= min(I, 16), "too many live rows for one probe: probe_groups_linear"
    G, X = np.zeros((N, O), f32), np.zeros((N, I), f32)
    m = f32(1 + 2.0**-10 + 2.0**-18)
    for k, r in enumerate(live):
        for o in range(k % Oc, O, Oc):
            G[r, o] = (-1.0 if _h(seed, r, o) & 1 else 1.0) * 2.0**((_h(seed, r, o, 1) % 3) - 1)
        for i in range(k // Oc, I, Ic):
            X[r, i] = (-1.0 if _h(seed, r, i, 2) & 1 else 1.0) * 2.0**((_h(seed, r, i, 3) % 5) - 2) * m
    return dict(N=N, O=O, I=I, G=torch.from_numpy(G), X=torch.from_numpy(X))


def probe_expect(dW64, db64):
    """the fp64 truth of a probe as fp32, after the proof that fp32 holds it exactly"""
    w, b = dW64.numpy().astype(f32), db64.numpy().astype(f32)
    assert np.array_equal(w.astype(np.float64), dW64.numpy()) and np.array_equal(b.astype(np.float64), db64.numpy()), "a probe value is no fp32 number"
    return w, b


def probe_is_exact(form, p, mask, z):
    """does the fp32 restatement of this form give the probe's truth bit for bit (both outputs)"""
    dW64, _, db64, _ = truth_dual(p["dsrc"], p["T"], mask, z, p["act"], p["X"], p["X2"], False)
    w, b = probe_expect(dW64, db64)
    gw, gb = restate_dual(form, p["dsrc"].numpy(), None if p["T"] is None else p["T"].numpy(), mask, z, p["act"], p["X"].numpy(),
                          None if p["X2"] is None else p["X2"].numpy(), p["N"])
    return np.array_equal(gw.view(np.uint32), w.view(np.uint32)) and np.array_equal(gb.view(np.uint32), b.view(np.uint32))


def bits_equal(got, want):
    """bit equality of two fp32 arrays, +0 and -0 told apart only where the value is not zero (a sum of zeros has no sign to keep)"""
    got, want = np.ascontiguousarray(np.asarray(got, f32)), np.ascontiguousarray(np.asarray(want, f32))
    return got.shape == want.shape and bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0))))
