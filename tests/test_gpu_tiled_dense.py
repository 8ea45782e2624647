"""The LDS-tiled dense kernels (K5t: tiled_fwd_kernel / tiled_dgrad_kernel, glass_amd/csrc/dense_tiled.hip) on the GPU, called through
the C entries glass_dual_linear_fwd_f32 / glass_dual_linear_dgrad_f32 with operand images from glass_dense_pack_batch_f32, in every
instantiation and launch form the default build reaches, graded stage by stage and element by element against
tests/tiled_dense_oracle.py at |got - want| <= 1e-5 * mass; the statistics and GraphNorm partials tile by tile.  Every output lives
in a NaN-filled buffer with guard columns (ld > width) and guard rows that must come back untouched; the guard rows of every input
hold Inf / NaN (what lies behind row N - 1 reaches nothing); every case runs twice and must repeat bit for bit, and asserts the form
it was written for through the restated dispatch.  The product form is the call's option in the act word.

Out of scope (tiled_dense_oracle.reaches_tiled): the hidden-128 trans forward and both hidden-128 data gradients (stage-run kernels
of dense.hip: tests/test_gpu_staged_dense.py), the K5t weight gradients.

One case fails on the parent commit's library: tests/test_tiled_dense_host.py::test_k5t_entry_codes_on_the_host_before_any_launch
(the data gradient took any act code).

Worst share of the bar per stage and product form as measured on MI355X: see MEASURED below."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import graphnorm_oracle as G  # noqa: E402
import tiled_dense_oracle as TD  # noqa: E402
from helpers import Buf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
Z = 0.85
CALL, GN_CALL = 7, 11
FORMS = [False, True]   # f32_products

MEASURED = """
  211 cases, 7.9 s.  Worst share of the 1e-5 * mass bar, split / f32 products:
  forward out 0.041 / 0.041   T 0.047 / 0.038   xa_out 0.010 / 0.010   stats partials 0.000 / 0.000 (fp64 sums of the written out)
  data gradient out 0.050 / 0.059   GraphNorm partials 0.027 / 0.028
(the CPU restatement's worst: out 0.027, T 0.030, xa_out 0.011, stats 0.000, data gradient 0.027, GraphNorm partials 0.036.)
"""

_WORST = {}


def _lib():
    from glass_amd import _lib
    return _lib.load()


def _f32_bit():
    from glass_amd import _lib
    return _lib.DENSE_F32_PRODUCTS


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc):
    assert rc == 0, _lib().glass_last_error_string()


def _act_word(act, f32p):
    return int(act) | (_f32_bit() if f32p else 0)


def _vec(src, dtype=torch.float32):
    t = torch.as_tensor(src).to(dtype).to(DEV).contiguous()
    assert t.data_ptr() % 16 == 0
    return t


def _words(seed=1234, step=3):
    return torch.tensor([seed, step], dtype=torch.int64, device=DEV)


def _keep(words, call, p, N, C):
    """the very keep-scales a kernel draws for (p, call id) at width C"""
    out = torch.full((N, C), NAN, dtype=torch.float32, device=DEV)
    _ok(_lib().glass_dropout_scales_f32(words.data_ptr(), call, p, N, C, out.data_ptr(), _stream()))
    k = out.cpu()
    inv = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))
    assert bool(((k == 0) | (k == inv)).all())
    return k


@functools.lru_cache(maxsize=None)
def _images(H, comb, seed, z):
    """(W, b on the device, forward image, data-gradient image) of recipe (H, *, comb, seed): the images depend on the weights alone"""
    lib = _lib()
    p = TD.recipe(H, 8, comb, seed)
    W, b = _vec(p["W"]), _vec(p["b"])
    K = W.shape[1]
    imgs = []
    for transposed, layout in ((0, lib.glass_dual_linear_fwd_layout(H, K)), (1, lib.glass_dual_linear_dgrad_layout(H, K))):
        nt, kt = (K, 2 * H) if transposed else (2 * H, K)
        flags = transposed | (layout << 1)
        img = torch.full((int(lib.glass_dense_image_floats(nt, kt, flags)), ), NAN, device=DEV)
        a = lambda v, dt: np.array([v], dtype=dt)
        args = (a(W.data_ptr(), np.uint64), a(img.data_ptr(), np.uint64), a(img.numel(), np.int64), a(nt, np.int64), a(kt, np.int64),
                a(flags, np.int32), a(z, np.float32))
        _ok(lib.glass_dense_pack_batch_f32(*[x.ctypes.data for x in args], 1, None, _stream()))
        torch.cuda.synchronize()
        imgs.append((img, layout))
    want_f = (5 if TD.eff_fwd_shape(H, K) else 1)
    want_d = (4 if TD.eff_dgrad_shape(H, K) else 2)
    assert imgs[0][1] == want_f and (H == 128 or imgs[1][1] == want_d), "the layouts the restated dispatch expects"
    return p["W"], p["b"], W, b, imgs[0][0], imgs[1][0]


@functools.lru_cache(maxsize=None)
def _recipe(H, N, comb, seed=0):
    p = TD.recipe(H, N, comb, seed)
    W, b = TD.recipe(H, 8, comb, seed)["W"], TD.recipe(H, 8, comb, seed)["b"]   # the weights of _images (independent of N)
    p["W"], p["b"] = W, b
    return p


def _note(stage, f32p, share, tag):
    key = (stage, "f32" if f32p else "split")
    _WORST[key] = max(_WORST.get(key, 0.0), share)
    print(f"tiled {tag}: {stage} {share:.3f}")


def _gate(stage, f32p, got, want, mass, tag):
    ok, share, at = TD.gate(got, want, mass)
    _note(stage, f32p, share, tag)
    assert ok, f"{tag}: {stage} misses the bar: share {share:.3g} at flat index {at}"


# ---- the two entries ----------------------------------------------------------------------------------------------------------------
def run_fwd(p, mask, z, act, f32p, want_T, want_stats, pro=None, gather=False, xa=None, allow_nan=False):
    """one forward, twice -> dict of CPU tensors out, T, stats, xa_out (each None when not requested).  pro = (gn_act, p_drop)"""
    lib = _lib()
    H, N, comb = p["H"], p["N"], p["comb"]
    _, _, W, b, Wimg, _ = _images(H, comb, 0, z)
    xa_h = p["xa"] if xa is None else xa
    src = Buf(p["V"], H, p["table"], tail=INF) if gather else Buf(N, H, xa_h, tail=INF)
    xb = Buf(N, H, p["xb"], tail=NAN) if comb else None
    m = torch.ones(N + 8, dtype=torch.uint8, device=DEV)
    m[:N] = torch.as_tensor(mask)
    idx = p["index"].to(DEV) if gather else None
    saved = _vec(p["saved"].reshape(-1)) if pro else None
    words = _words()
    n_part = TD._cdiv(N, TD.tiled_rows(H))
    res = []
    for _ in range(2):
        out = Buf(N, H)
        T = Buf(N, 2 * H) if want_T else None
        st = Buf(n_part, 2 * H, dtype=torch.float64, pad=0) if want_stats else None
        side = Buf(N, H) if pro else None
        _ok(lib.glass_dual_linear_fwd_f32(src.ptr, src.ld, xb.ptr if comb else None, xb.ld if comb else 0, Wimg.data_ptr(), b.data_ptr(), m.data_ptr(),
                                          z, _act_word(act, f32p), T.ptr if T else None, T.ld if T else 0, out.ptr, out.ld, N, H,
                                          st.ptr if st else None, 0, saved.data_ptr() if pro else None, None, pro[0] if pro else 0,
                                          pro[1] if pro else 0.0, words.data_ptr() if pro and pro[1] > 0 else None, CALL,
                                          side.ptr if pro else None, side.ld if pro else 0, idx.data_ptr() if gather else None, p["V"] if gather else 0,
                                          _stream()))
        torch.cuda.synchronize()
        for name, bf in (("out", out), ("T", T), ("stats", st), ("xa_out", side)):
            if bf is not None:
                bf.check(name, allow_nan)
        res.append((out, T, st, side))
    for a, c in zip(*res):
        if a is not None:
            assert torch.equal(a.flat.view(torch.int32 if a.flat.dtype == torch.float32 else torch.int64),
                               c.flat.view(torch.int32 if c.flat.dtype == torch.float32 else torch.int64)), "the second run differs"
    out, T, st, side = res[0]
    keep = _keep(words, CALL, pro[1], N, H) if pro and pro[1] > 0 else None
    return dict(out=out.cpu(), T=T.cpu() if T else None, stats=st.cpu().view(n_part, 2, H) if st else None,
                xa_out=side.cpu() if side else None, keep=keep)


def grade_fwd(p, mask, z, act, f32p, got, tag, pro=None, gather=False):
    H, N = p["H"], p["N"]
    x = p["table"][p["index"]] if gather else p["xa"]
    A = x
    if pro:
        want, mass = TD.stage_prologue(x, p["saved"], pro[0], got["keep"])
        _gate("xa_out", f32p, got["xa_out"], want, mass, tag)
        A = got["xa_out"]
    tr = TD.stage_fwd(A, p["xb"], p["W"], p["b"], mask, z, act)
    if got["T"] is not None:
        _gate("T", f32p, got["T"], tr["T"], tr["T_m"], tag)
    _gate("out", f32p, got["out"], tr["out"], tr["out_m"], tag)
    if got["stats"] is not None:
        sw, sm = TD.stage_stats(got["out"], N, TD.tiled_rows(H))
        _gate("stats", f32p, got["stats"], sw, sm, tag)
    return tr


def run_dgrad(p, mask, z, act, f32p, n_out, addend=False, p_drop=0.0, gn=None, dsrc=None, allow_nan=False):
    """one data gradient, twice -> dict out, part, keep, gn_keep.  gn = (gn_act, gn_p_drop)"""
    lib = _lib()
    H, N = p["H"], p["N"]
    _, _, W, b, _, WTimg = _images(H, n_out == 2 * H, 0, z)
    d = Buf(N, H, p["dsrc"] if dsrc is None else dsrc, tail=INF)
    T = Buf(N, 2 * H, p["T"], tail=NAN) if act else None
    ad = Buf(N, n_out, p["addend"], tail=NAN) if addend else None
    m = torch.ones(N + 8, dtype=torch.uint8, device=DEV)
    m[:N] = torch.as_tensor(mask)
    words = _words()
    n_part = TD._cdiv(N, 128)
    gx = Buf(N, H, p["gn_x"], tail=NAN) if gn else None
    saved, alpha = (_vec(p["saved"].reshape(-1)), _vec(p["alpha"])) if gn else (None, None)
    need_rng = p_drop > 0 or (gn and gn[1] > 0)
    res = []
    for _ in range(2):
        out = Buf(N, n_out)
        part = Buf(n_part, 2 * H, dtype=torch.float64, pad=0) if gn else None
        _ok(lib.glass_dual_linear_dgrad_f32(d.ptr, d.ld, T.ptr if T else None, T.ld if T else 0, m.data_ptr(), z, _act_word(act, f32p), WTimg.data_ptr(),
                                            n_out, ad.ptr if ad else None, ad.ld if ad else 0, p_drop, words.data_ptr() if need_rng else None, CALL,
                                            out.ptr, out.ld, N, H, part.ptr if gn else None, gx.ptr if gn else None, gx.ld if gn else 0,
                                            saved.data_ptr() if gn else None, alpha.data_ptr() if gn else None, gn[0] if gn else 0,
                                            gn[1] if gn else 0.0, GN_CALL, 0, _stream()))
        torch.cuda.synchronize()
        out.check("dgrad out", allow_nan)
        if part:
            part.check("gn partials", allow_nan)
        res.append((out, part))
    for a, c in zip(*res):
        if a is not None:
            it = torch.int32 if a.flat.dtype == torch.float32 else torch.int64
            assert torch.equal(a.flat.view(it), c.flat.view(it)), "the second run differs"
    out, part = res[0]
    return dict(out=out.cpu(), part=part.cpu().view(n_part, 2, H) if part else None,
                keep=_keep(words, CALL, p_drop, N, n_out) if p_drop > 0 else None,
                gn_keep=_keep(words, GN_CALL, gn[1], N, H) if gn and gn[1] > 0 else None)


def grade_dgrad(p, mask, z, act, f32p, n_out, got, tag, addend=False, gn=None):
    H, N = p["H"], p["N"]
    want, mass = TD.stage_dgrad(p["dsrc"], p["T"], p["W"], mask, z, act, n_out, p["addend"] if addend else None, got["keep"])
    _gate("dgrad", f32p, got["out"], want, mass, tag)
    if gn:
        pw, pm = TD.stage_gn_partials(got["out"][:, :H], p["gn_x"], p["saved"], p["alpha"], gn[0], got["gn_keep"], N)
        _gate("gn_partials", f32p, got["part"], pw, pm, tag)
    return want, mass


# ---- 1. row counts -----------------------------------------------------------------------------------------------------------------
def _random_mask(N, seed):
    return (torch.rand(N, generator=torch.Generator().manual_seed(seed)) < 0.3).numpy().astype(np.uint8)


@pytest.mark.parametrize("f32p", FORMS)
@pytest.mark.parametrize("comb", [False, True])
@pytest.mark.parametrize("N", [1, 127, 128, 129, 1023, 1025, 1153])
@pytest.mark.parametrize("H", [256, 512])
def test_row_counts_of_128_row_tiles(H, N, comb, f32p):
    """one tile, a ragged tile, exactly 8 tiles, 9 tiles (a grid rounded to 16 with 7 empty row tiles), 10 tiles; a third of the rows
    labeled, so every tile takes the two-weight path; forward with T (trans) and statistics, data gradient with the GraphNorm partials"""
    p = _recipe(H, N, comb)
    mask = _random_mask(N, N)
    act = 0 if comb else 1
    form = TD.fwd_form(H, comb, N, f32p, act=act, has_T=not comb, mask=mask)
    assert form["BM"] == 128 and form["split"] == (not f32p) and form["eff"] == comb and form["n_rt"] == TD._cdiv(N, 128)
    assert form["grid"] == TD._cdiv(form["n_rt"], 8) * 8 * (H // 128)
    if N >= 127:
        assert "two" in form["paths"]
    tag = f"rows H={H} N={N} comb={int(comb)} f32={int(f32p)}"
    got = run_fwd(p, mask, Z, act, f32p, want_T=not comb, want_stats=True)
    grade_fwd(p, mask, Z, act, f32p, got, tag)
    n_out = 2 * H if comb else H
    dform = TD.dgrad_form(H, n_out, N, f32p, act=act, mask=mask)
    assert dform["n_partials"] == TD._cdiv(N, 128) and dform["eff"] == comb
    dgot = run_dgrad(p, mask, Z, act, f32p, n_out, gn=(0, 0.0))
    grade_dgrad(p, mask, Z, act, f32p, n_out, dgot, tag, gn=(0, 0.0))


@pytest.mark.parametrize("f32p", FORMS)
@pytest.mark.parametrize("N", [1, 63, 64, 65, 513, 577])
def test_row_counts_of_64_row_tiles_at_hidden_128(N, f32p):
    p = _recipe(128, N, True)
    mask = _random_mask(N, N)
    form = TD.fwd_form(128, True, N, f32p, mask=mask)
    assert form["BM"] == 64 and not form["eff"] and form["n_partials"] == TD._cdiv(N, 64) and form["nct"] == 1
    for want_T, want_stats in ((False, True), (True, False)):
        got = run_fwd(p, mask, Z, 0, f32p, want_T=want_T, want_stats=want_stats)
        grade_fwd(p, mask, Z, 0, f32p, got, f"rows H=128 N={N} f32={int(f32p)}")


@pytest.mark.parametrize("f32p", FORMS)
@pytest.mark.parametrize("N", [32768, 32769, 32833])
def test_both_sides_of_the_128_row_threshold_at_hidden_128(N, f32p):
    """512 tiles of 64 rows keep them; one row more takes 128-row tiles in the split form (ragged in the lower / in the upper row wave)
    and stays on 64-row tiles with f32 products.  The partials are graded per 64 rows: the two row waves of a 128-row tile write their
    own slots in order, and no slot at or past ceil(N / 64) is written."""
    p = _recipe(128, N, True)
    mask = _random_mask(N, 5)
    form = TD.fwd_form(128, True, N, f32p, mask=mask)
    assert form["BM"] == (128 if (N > 32768 and not f32p) else 64) and form["n_partials"] == TD._cdiv(N, 64)
    got = run_fwd(p, mask, Z, 0, f32p, want_T=False, want_stats=True)
    grade_fwd(p, mask, Z, 0, f32p, got, f"tall H=128 N={N} f32={int(f32p)}")
    # the swap of two neighbouring 64-row slots is refused by this gate on these very outputs
    sw, sm = TD.stage_stats(got["out"], N, 64)
    swapped = got["stats"].clone()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert not TD.gate(swapped, sw, sm)[0]


# ---- 2. forward: every instantiation and argument ---------------------------------------------------------------------------------
@pytest.mark.parametrize("f32p", FORMS)
@pytest.mark.parametrize("H", [256, 512])
def test_forward_trans_pair_acts_T_and_stats(H, f32p):
    """act 0 / 1 / 2, T requested and NULL, stats requested and NULL: `out` is bit-equal across the requests"""
    N = 129
    p = _recipe(H, N, False)
    mask = _random_mask(N, 3)
    for act in (0, 1, 2):
        outs = []
        for want_T, want_stats in ((True, True), (False, True), (True, False), (False, False)):
            form = TD.fwd_form(H, False, N, f32p, act=act, has_T=want_T, mask=mask)
            assert not form["eff"] and form["paths"] == ["two", "two"]
            got = run_fwd(p, mask, Z, act, f32p, want_T, want_stats)
            grade_fwd(p, mask, Z, act, f32p, got, f"trans H={H} act={act} T={int(want_T)} stats={int(want_stats)} f32={int(f32p)}")
            outs.append(got["out"])
        assert all(torch.equal(o, outs[0]) for o in outs[1:])


@pytest.mark.parametrize("f32p", FORMS)
@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("gn_act", [0, 1, 2])
@pytest.mark.parametrize("H,comb", [(128, True), (256, False), (256, True), (512, False), (512, True)])
def test_forward_graphnorm_prologue(H, comb, gn_act, p_drop, f32p):
    """the GraphNorm + dropout prologue with the very masks, the side output with ldxo > H; trans pair: also gathered from a 37-row table"""
    N = 300
    p = _recipe(H, N, comb)
    bm = 64 if H == 128 else 128
    mask = TD.label_pattern("cap_next_over", N, bm, TD.MAXFIX_FWD)   # comb at 256 / 512: a repaired tile next to a two-weight tile
    act = 0 if comb else 1
    for gather in ((False, True) if not comb else (False, )):
        form = TD.fwd_form(H, comb, N, f32p, act=act, has_T=not comb, mask=mask)
        if comb and H != 128:
            assert form["paths"] == ["pure", "two", "pure"]
        got = run_fwd(p, mask, Z, act, f32p, want_T=not comb, want_stats=True, pro=(gn_act, p_drop), gather=gather)
        if p_drop > 0:
            assert 0.4 < float((got["keep"] == 0).float().mean()) < 0.6
        grade_fwd(p, mask, Z, act, f32p, got, f"prologue H={H} comb={int(comb)} gn_act={gn_act} p={p_drop} gather={int(gather)} f32={int(f32p)}",
                  pro=(gn_act, p_drop), gather=gather)


# ---- 3. data gradient: every instantiation and argument ------------------------------------------------------------------------------
@pytest.mark.parametrize("f32p", FORMS)
@pytest.mark.parametrize("H", [256, 512])
def test_dgrad_trans_pair_arguments(H, f32p):
    """n_out = H: act 0 / 1 / 2 with T, addend present and absent, the dropout epilogue 0 and 0.5, the GraphNorm partials requested
    and not with gn_act and gn_p_drop 0 and 0.5; the output is bit-equal with and without the partials"""
    N = 129
    p = _recipe(H, N, False)
    mask = _random_mask(N, 4)
    for act, addend, p_drop, gn in ((0, False, 0.0, None), (1, True, 0.0, (0, 0.0)), (2, False, 0.5, (1, 0.0)), (1, True, 0.5, (2, 0.5)), (0, True, 0.0, (1, 0.5))):
        form = TD.dgrad_form(H, H, N, f32p, act=act, mask=mask)
        assert not form["eff"] and form["nct"] == H // 256
        tag = f"dgrad H={H} n_out=H act={act} addend={int(addend)} p={p_drop} gn={gn} f32={int(f32p)}"
        got = run_dgrad(p, mask, Z, act, f32p, H, addend, p_drop, gn)
        grade_dgrad(p, mask, Z, act, f32p, H, got, tag, addend, gn)
        if gn:
            plain = run_dgrad(p, mask, Z, act, f32p, H, addend, p_drop, None)
            assert torch.equal(plain["out"], got["out"]), tag + ": the partials changed the output"


@pytest.mark.parametrize("f32p", FORMS)
@pytest.mark.parametrize("H", [256, 512])
def test_dgrad_comb_pair_arguments(H, f32p):
    """n_out = 2H (effective-weight image): addend present and absent, GraphNorm partials with gn_act / gn_p_drop, on a launch that
    holds a repaired tile and a two-term tile; the output is bit-equal with and without the partials"""
    N = 300
    p = _recipe(H, N, True)
    mask = TD.label_pattern("cap_next_over", N, 128, TD.MAXFIX_DGRAD)
    for addend, gn in ((False, None), (True, (0, 0.0)), (False, (1, 0.5)), (True, (2, 0.0))):
        form = TD.dgrad_form(H, 2 * H, N, f32p, mask=mask)
        assert form["eff_live"] and form["paths"] == ["pure", "two", "pure"]
        tag = f"dgrad H={H} n_out=2H addend={int(addend)} gn={gn} f32={int(f32p)}"
        got = run_dgrad(p, mask, Z, 0, f32p, 2 * H, addend, 0.0, gn)
        grade_dgrad(p, mask, Z, 0, f32p, 2 * H, got, tag, addend, gn)
        if gn:
            plain = run_dgrad(p, mask, Z, 0, f32p, 2 * H, addend, 0.0, None)
            assert torch.equal(plain["out"], got["out"]), tag + ": the partials changed the output"


# ---- 4. the effective-weight path under every label pattern ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pattern_truth(H, N, pattern, kmax, z, direction):
    p = _recipe(H, N, True)
    mask = TD.label_pattern(pattern, N, 128, kmax)
    if direction == "fwd":
        return mask, TD.stage_fwd(p["xa"], p["xb"], p["W"], p["b"], mask, z, 0)
    return mask, TD.stage_dgrad(p["dsrc"], None, p["W"], mask, z, 0, 2 * H)


@pytest.mark.parametrize("f32p", FORMS)
@pytest.mark.parametrize("pattern", TD.PATTERNS)
@pytest.mark.parametrize("H", [256, 512])
def test_effective_weight_label_patterns(H, pattern, f32p):
    """N = 300: two whole tiles and a ragged one of 44 rows.  Forward (kMaxFix 3) and data gradient (kMaxFix 7); `last` labels row
    N - 1 in the ragged tile; the cap / over patterns sit in tile 1, inside one wave's rows or across the two row waves."""
    N = 300
    p = _recipe(H, N, True)
    tag = f"labels H={H} {pattern} f32={int(f32p)}"
    expect = {"none": ["pure"] * 3, "all": ["two"] * 3, "over": ["pure", "two", "pure"], "over_wave": ["pure", "two", "pure"],
              "over_split": ["pure", "two", "pure"], "cap_next_over": ["pure", "two", "pure"]}.get(pattern, ["pure"] * 3)
    mask, tr = _pattern_truth(H, N, pattern, TD.MAXFIX_FWD, Z, "fwd")
    assert TD.fwd_form(H, True, N, f32p, mask=mask)["paths"] == expect
    got = run_fwd(p, mask, Z, 0, f32p, want_T=False, want_stats=True)
    _gate("out", f32p, got["out"], tr["out"], tr["out_m"], tag)
    sw, sm = TD.stage_stats(got["out"], N, 128)
    _gate("stats", f32p, got["stats"], sw, sm, tag)
    mask, (want, mass) = _pattern_truth(H, N, pattern, TD.MAXFIX_DGRAD, Z, "dgrad")
    assert TD.dgrad_form(H, 2 * H, N, f32p, mask=mask)["paths"] == expect
    dgot = run_dgrad(p, mask, Z, 0, f32p, 2 * H)
    _gate("dgrad", f32p, dgot["out"], want, mass, tag)


@pytest.mark.parametrize("f32p", FORMS)
@pytest.mark.parametrize("z", [0.5, 0.3])
@pytest.mark.parametrize("H", [256, 512])
def test_effective_weight_z_half_and_below(H, z, f32p):
    """z = 0.5: the correction is exactly zero, the output bit-equal to the no-label run of the same rows; z = 0.3: the sign of
    z - (1 - z) flips"""
    N = 200
    p = _recipe(H, N, True)
    for kmax, direction in ((TD.MAXFIX_FWD, "fwd"), (TD.MAXFIX_DGRAD, "dgrad")):
        mask = TD.label_pattern("cap", N, 128, kmax)
        none = np.zeros(N, dtype=np.uint8)
        tag = f"z={z} H={H} {direction} f32={int(f32p)}"
        if direction == "fwd":
            assert TD.fwd_form(H, True, N, f32p, mask=mask)["paths"] == ["pure", "pure"]
            got = run_fwd(p, mask, z, 0, f32p, False, True)
            grade_fwd(p, mask, z, 0, f32p, got, tag)
            if z == 0.5:
                ref = run_fwd(p, none, z, 0, f32p, False, True)
                assert torch.equal(got["out"], ref["out"]) and torch.equal(got["stats"], ref["stats"]), tag
        else:
            assert TD.dgrad_form(H, 2 * H, N, f32p, mask=mask)["paths"] == ["pure", "pure"]
            got = run_dgrad(p, mask, z, 0, f32p, 2 * H)
            grade_dgrad(p, mask, z, 0, f32p, 2 * H, got, tag)
            if z == 0.5:
                assert torch.equal(got["out"], run_dgrad(p, none, z, 0, f32p, 2 * H)["out"]), tag


# ---- 5. non-finite inputs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32p", FORMS)
@pytest.mark.parametrize("H,comb", [(128, True), (256, False), (256, True), (512, True)])
def test_a_nan_row_stays_in_its_row_and_its_tile(H, comb, f32p):
    """NaN in one element of an unlabeled row of tile 0 and of a labeled, afterwards repaired row of tile 1 (comb at 256 / 512): those
    rows of the output, and those tiles' partials, hold NaN and nothing else does.  (What lies behind row N - 1 — Inf / NaN in the
    guard rows of xa, xb, dsrc, T, addend — reaches nothing in ANY case of this file.)"""
    bm = 64 if H == 128 else 128
    N = 2 * bm + 40
    p = _recipe(H, N, comb)
    rows = [5, bm + 77 % bm]
    mask = np.zeros(N, dtype=np.uint8)
    mask[rows[1]] = 1
    act = 0 if comb else 1
    xa = p["xa"].clone()
    xa[rows[0], 3], xa[rows[1], H - 1] = NAN, NAN
    form = TD.fwd_form(H, comb, N, f32p, act=act, has_T=not comb, mask=mask)
    if comb and H != 128:
        assert form["paths"] == ["pure"] * 3
    got = run_fwd(p, mask, Z, act, f32p, want_T=not comb, want_stats=True, xa=xa, allow_nan=True)
    tr = TD.stage_fwd(p["xa"], p["xb"], p["W"], p["b"], mask, Z, act)
    tag = f"nan H={H} comb={int(comb)} f32={int(f32p)}"
    ok, share, _ = TD.gate_nan_rows(got["out"], tr["out"], tr["out_m"], rows)
    assert ok, (tag, share)
    if got["T"] is not None:
        assert TD.gate_nan_rows(got["T"], tr["T"], tr["T_m"], rows)[0], tag
    nan_part = torch.isnan(got["stats"]).all(dim=2).all(dim=1)
    assert nan_part.tolist() == [t in (rows[0] // bm, rows[1] // bm) for t in range(TD._cdiv(N, bm))], tag
    if H != 128:
        n_out = 2 * H if comb else H
        dsrc = p["dsrc"].clone()
        dsrc[rows[0], 3], dsrc[rows[1], H - 1] = NAN, NAN
        dgot = run_dgrad(p, mask, Z, act, f32p, n_out, gn=(0, 0.0), dsrc=dsrc, allow_nan=True)
        want, mass = TD.stage_dgrad(p["dsrc"], p["T"], p["W"], mask, Z, act, n_out)
        assert TD.gate_nan_rows(dgot["out"], want, mass, rows)[0], tag
        assert torch.isnan(dgot["part"]).all(dim=2).all(dim=1).tolist() == [True, True, False], tag


# ---- the figures ---------------------------------------------------------------------------------------------------------------------------
def test_zz_report_worst_shares():
    """prints the worst share of the bar per stage and product form over the cases that ran in this process (file order: last)"""
    for (stage, form), v in sorted(_WORST.items()):
        print(f"tiled worst share: {stage:12s} {form:5s} {v:.3f}")
    assert all(v <= 1.0 for v in _WORST.values())
