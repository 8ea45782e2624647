"""tests/tiled_dense_oracle.py checked on the CPU: the restated dispatch against the source text of dense_tiled.hip / dense.hip, every
gate of tests/test_gpu_tiled_dense.py against the honest fp32 restatement of the kernels (it must pass with room) and against one
mistake at a time (each must be refused), and the entries' argument checks that answer before any launch."""
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

E_ARG, E_UNSUPPORTED = -1, -3
Z = 0.85
F64 = torch.float64
_WORST = {}


# ---- the dispatch and the source text -------------------------------------------------------------------------------------------------
def test_restated_dispatch_is_tied_to_the_source_text():
    k = TD.source_constants()
    assert k["kTK"] == TD.KSTEP and k["kTThreads"] == 256
    assert k["tiled_rows_text"] and k["shape_text"], "tiled_rows / tiled_shape_ok moved"
    assert k["tall_limit"] == TD.TALL_TILES and k["tall_launch_text"] and k["bm_text"], "tall128's limit or the BM table moved"
    assert k["grid_round"] == TD.GRID_ROUND and k["tile_of_block_text"] and k["eff_block_text"], "tiled_grid's rounding / the block maps moved"
    assert k["kMaxFix_fwd"] == TD.MAXFIX_FWD and k["kMaxFix_dgrad"] == TD.MAXFIX_DGRAD, "kMaxFix moved"
    assert k["fwd_eff_cond_text"] and k["dgrad_eff_cond_text"] and k["pure_text"]
    assert k["eff_fwd_shape_text"] and k["eff_dgrad_shape_text"] and k["half_partials_text"] and k["dgrad_widths_text"]
    assert k["fwd_leave_text"] and k["dgrad_leave_text"] and set(k["v2_defaults"].values()) == {1}, "which (H, pair) reach the tiled family moved"
    assert tuple((int(a), int(b)) for a, b in k["split_order"]) == TD.SPLIT_ORDER


def test_restated_dispatch_values():
    assert [TD.tiled_rows(H) for H in TD.WIDTHS] == [64, 128, 128]
    assert not TD.tall128(32768, False) and TD.tall128(32769, False) and not TD.tall128(32769, True)
    assert [TD.tiled_grid(n, 2) for n in (1, 8, 9, 10)] == [16, 16, 32, 32]
    # every (row tile, column tile) is owned by exactly one block of the rounded grid, the rest are empty
    for n_rt, nct in ((1, 1), (9, 2), (10, 4), (8, 2), (17, 1)):
        got = [TD.tile_of_block(b, nct, n_rt) for b in range(TD.tiled_grid(n_rt, nct))]
        assert sorted(t for t in got if t) == [(r, c) for r in range(n_rt) for c in range(nct)] and got.count(None) == len(got) - n_rt * nct
    assert TD.tile_of_block(9, 2, 10) == (1, 1) and TD.tile_of_block(16, 2, 10) == (8, 0)
    reach = {(H, c, d): TD.reaches_tiled(H, c, d) for H in (64, 128, 256, 512) for c in (False, True) for d in ("fwd", "dgrad")}
    assert [k for k, v in reach.items() if v] == [(128, True, "fwd")] + [(H, c, d) for H in (256, 512) for c in (False, True) for d in ("fwd", "dgrad")]
    f = TD.fwd_form(128, True, 32768, False)
    assert (f["BM"], f["n_rt"], f["n_partials"], f["eff"]) == (64, 512, 512, False)
    f = TD.fwd_form(128, True, 32833, False)
    assert (f["BM"], f["n_rt"], f["n_partials"], f["grid"]) == (128, 257, 514, 264)
    assert TD.fwd_form(128, True, 32833, True)["BM"] == 64
    for kmax, form in ((TD.MAXFIX_FWD, lambda m: TD.fwd_form(256, True, 300, False, mask=m)), (TD.MAXFIX_DGRAD, lambda m: TD.dgrad_form(256, 512, 300, False, mask=m))):
        assert form(TD.label_pattern("cap", 300, 128, kmax))["paths"] == ["pure"] * 3
        assert form(TD.label_pattern("over", 300, 128, kmax))["paths"] == ["pure", "two", "pure"]
        assert form(TD.label_pattern("cap_next_over", 300, 128, kmax))["paths"] == ["pure", "two", "pure"]
        assert form(TD.label_pattern("all", 300, 128, kmax))["paths"] == ["two"] * 3
        for name in ("cap_wave", "over_wave", "cap_split", "over_split"):
            m = TD.label_pattern(name, 300, 128, kmax)
            assert int(m.sum()) == kmax + name.startswith("over") and int(m[:128].sum()) == 0 and int(m[256:].sum()) == 0
            assert (int(m[128:192].sum()) == 0) == name.endswith("wave")
    assert TD.fwd_form(256, True, 300, False, act=0, has_T=True, mask=np.zeros(300))["paths"] == ["two"] * 3
    assert TD.fwd_form(256, False, 300, False, mask=np.zeros(300))["paths"] == ["two"] * 3
    assert TD.dgrad_form(512, 512, 300, False, mask=np.zeros(300))["paths"] == ["two"] * 3
    m = TD.label_pattern("last", 1153, 128, 3)
    assert int(m.sum()) == 1 and m[1152] == 1


def test_split_pieces_are_exact_and_bf16():
    x = (torch.randn(4096, generator=torch.Generator().manual_seed(1)) * 3).numpy()
    hi, mid, lo = TD.split3(x)
    assert np.array_equal((hi.astype(np.float64) + mid + lo).astype(np.float32), x)
    for p in (hi, mid, lo):
        assert not (p.view(np.uint32) & 0xFFFF).any()


# ---- the gates on the fp32 restatement ---------------------------------------------------------------------------------------------------
FWD_RECIPES = [   # (H, comb, N, act, pattern, BM forced)
    (128, True, 65, 0, "last", None), (128, True, 130, 0, "row0", 128),
    (256, False, 129, 1, "over", None), (256, False, 40, 2, "all", None), (256, True, 200, 0, "cap_next_over", None),
    (512, True, 130, 0, "row0", None), (512, False, 33, 1, "last", None)]
DGRAD_RECIPES = [  # (H, n_out, N, act, pattern)
    (256, 256, 129, 1, "over"), (256, 256, 40, 2, "all"), (256, 512, 200, 0, "cap_next_over"), (512, 1024, 130, 0, "row127"), (512, 512, 33, 1, "last")]


@functools.lru_cache(maxsize=None)
def _fwd_case(H, comb, N, act, pattern, bm):
    p = TD.recipe(H, N, comb)
    BM = bm or (64 if H == 128 else 128)
    mask = TD.label_pattern(pattern, N, BM, TD.MAXFIX_FWD)
    keep = G.keep_mask(N, H, 0.5, 5)
    A, _ = TD.stage_prologue(p["xa"], p["saved"], TD.ACT_ELU, keep)
    A32 = TD.restate_prologue(p["xa"].numpy(), p["saved"].numpy(), TD.ACT_ELU, keep.numpy())
    truth = TD.stage_fwd(torch.from_numpy(A32), p["xb"], p["W"], p["b"], mask, Z, act)
    return p, mask, keep, A32, truth


def _fwd_form(H, comb, N, act, mask, f32p, bm):
    form = TD.fwd_form(H, comb, N, f32p, act=act, has_T=not comb, mask=mask)
    if bm:   # the 128-row split tiles of hidden 128 at a size the host can restate (the GPU reaches them beyond 32 768 rows)
        form = dict(form, BM=bm, paths=["two"] * TD._cdiv(N, bm))
    return form


def _note(stage, share):
    _WORST[stage] = max(_WORST.get(stage, 0.0), share)


FWD_PARAMS = [r + (f, ) for r in FWD_RECIPES for f in (False, True) if not (f and r[5])]   # (128-row tiles at hidden 128: split form only)


@pytest.mark.parametrize("H,comb,N,act,pattern,bm,f32p", FWD_PARAMS)
def test_forward_gates_pass_the_restatement_and_refuse_each_mistake(H, comb, N, act, pattern, bm, f32p):
    """Worst share of the 1e-5 * mass bar of the honest restatement (both product forms, all recipes): xa_out 0.011, T 0.030,
    out 0.027, stats 0.000 (fp64 sums of the written fp32 values) — the condition is < 0.5.  Mutants refused: drop_kstep, swap_w,
    fix_no_bias, fix_unlabeled, fix_row_plus1, upper_ct_unwritten (hidden 512), row_past_N, halves_swapped (128-row tiles of hidden 128)."""
    p, mask, keep, A32, truth = _fwd_case(H, comb, N, act, pattern, bm)
    form = _fwd_form(H, comb, N, act, mask, f32p, bm)
    want_A, mass_A = TD.stage_prologue(p["xa"], p["saved"], TD.ACT_ELU, keep)
    ok, share, _ = TD.gate(torch.from_numpy(A32), want_A, mass_A)
    assert ok and share < 0.5
    _note("xa_out", share)
    xb = None if p["xb"] is None else p["xb"].numpy()
    got = TD.restate_fwd(A32, xb, p["W"].numpy(), p["b"].numpy(), mask, Z, act, form)
    assert (got["T"] is None) == form["eff_live"]
    if got["T"] is not None:
        ok, share, _ = TD.gate(torch.from_numpy(got["T"]), truth["T"], truth["T_m"])
        assert ok and share < 0.5, share
        _note("T", share)
    ok, share, _ = TD.gate(torch.from_numpy(got["out"]), truth["out"], truth["out_m"])
    assert ok and share < 0.5, share
    _note("out", share)
    sw, sm = TD.stage_stats(torch.from_numpy(got["out"]), N, form["partial_rows"])
    ok, share, _ = TD.gate(torch.from_numpy(got["stats"]), sw, sm)
    assert ok and share < 0.5
    _note("stats", share)
    print(f"tiled fwd host H={H} comb={comb} N={N} f32={f32p}: " + " ".join(f"{k} {v:.3f}" for k, v in _WORST.items()))
    # one mistake at a time
    labeled_pure = any(pa == "pure" and mask[t * form["BM"]:(t + 1) * form["BM"]].any() for t, pa in enumerate(form["paths"]))
    labeled_two = any(pa == "two" and mask[t * form["BM"]:(t + 1) * form["BM"]].any() for t, pa in enumerate(form["paths"]))
    for mutant in TD.MUTANTS_FWD:
        applies = {"drop_kstep": True, "swap_w": labeled_two, "fix_no_bias": labeled_pure, "fix_unlabeled": labeled_pure,
                   "fix_row_plus1": labeled_pure and pattern != "last", "upper_ct_unwritten": H == 512 and "pure" in form["paths"]}[mutant]
        if not applies:
            continue
        bad = TD.restate_fwd(A32, xb, p["W"].numpy(), p["b"].numpy(), mask, Z, act, form, mutant=mutant)
        assert not TD.gate(torch.from_numpy(bad["out"]), truth["out"], truth["out_m"])[0], f"the out gate took mutant {mutant}"
        _seen.add(("fwd", mutant))
    extra = got["out"][0] * 0 + 1e-3   # a row past N as small as 1e-3 per column
    bad = TD.restate_partials(got["out"], N, form["partial_rows"], extra_row=extra)
    assert not TD.gate(torch.from_numpy(bad), sw, sm)[0], "the stats gate took a row past N"
    _seen.add(("partials", "row_past_N"))
    if bm:
        bad = TD.restate_partials(got["out"], N, form["partial_rows"], swap_halves=True)
        assert not TD.gate(torch.from_numpy(bad), sw, sm)[0], "the stats gate took swapped 64-row halves"
        assert TD.gate(torch.from_numpy(bad.sum(0)), sw.sum(0), sm.sum(0))[0], "(summed over the tiles first, the swap is invisible)"
        _seen.add(("partials", "halves_swapped"))


_seen = set()


@pytest.mark.parametrize("f32p", [False, True])
@pytest.mark.parametrize("H,n_out,N,act,pattern", DGRAD_RECIPES)
def test_dgrad_gates_pass_the_restatement_and_refuse_each_mistake(H, n_out, N, act, pattern, f32p):
    """Worst share of the bar of the honest restatement: data gradient out 0.027, GraphNorm partials 0.036 — the condition is < 0.5.
    Mutants refused: drop_kstep, swap_w, fix_unlabeled, fix_row_plus1, dropout_twice, addend_dropped, row_past_N."""
    comb = n_out == 2 * H
    p = TD.recipe(H, N, comb)
    mask = TD.label_pattern(pattern, N, 128, TD.MAXFIX_DGRAD)
    form = TD.dgrad_form(H, n_out, N, f32p, act=act, mask=mask)
    keep = G.keep_mask(N, n_out, 0.5, 9) if not comb else None
    want, mass = TD.stage_dgrad(p["dsrc"], p["T"], p["W"], mask, Z, act, n_out, p["addend"], keep)
    args = (p["dsrc"].numpy(), p["T"].numpy(), p["W"].numpy(), mask, Z, act, n_out, form)
    kw = dict(addend=p["addend"].numpy(), keep=None if keep is None else keep.numpy())
    got = TD.restate_dgrad(*args, **kw)
    ok, share, _ = TD.gate(torch.from_numpy(got), want, mass)
    assert ok and share < 0.5, share
    _note("dgrad", share)
    gkeep = G.keep_mask(N, H, 0.5, 11)
    g = torch.from_numpy(got[:, :H])
    for gn_act in (0, 1, 2):
        pw, pm = TD.stage_gn_partials(g, p["gn_x"], p["saved"], p["alpha"], gn_act, gkeep, N)
        part = TD.restate_gn_partials(got[:, :H], p["gn_x"].numpy(), p["saved"].numpy(), p["alpha"].numpy(), gn_act, gkeep.numpy(), N)
        ok, share, _ = TD.gate(torch.from_numpy(part), pw, pm)
        assert ok and share < 0.5, share
        _note("gn_partials", share)
    print(f"tiled dgrad host H={H} n_out={n_out} N={N} f32={f32p}: " + " ".join(f"{k} {v:.3f}" for k, v in _WORST.items()))
    bm = form["BM"]
    labeled_pure = any(pa == "pure" and mask[t * bm:(t + 1) * bm].any() for t, pa in enumerate(form["paths"]))
    labeled_two = any(pa == "two" and mask[t * bm:(t + 1) * bm].any() for t, pa in enumerate(form["paths"]))
    for mutant in TD.MUTANTS_DGRAD:
        applies = {"drop_kstep": True, "swap_w": labeled_two, "fix_unlabeled": labeled_pure, "fix_row_plus1": labeled_pure and pattern != "last",
                   "dropout_twice": keep is not None, "addend_dropped": True}[mutant]
        if not applies:
            continue
        bad = TD.restate_dgrad(*args, mutant=mutant, **kw)
        assert not TD.gate(torch.from_numpy(bad), want, mass)[0], f"the data-gradient gate took mutant {mutant}"
        _seen.add(("dgrad", mutant))
    pw, pm = TD.stage_gn_partials(g, p["gn_x"], p["saved"], p["alpha"], 0, None, N)
    part = TD.restate_gn_partials(got[:, :H], p["gn_x"].numpy(), p["saved"].numpy(), p["alpha"].numpy(), 0, None, N)
    part[-1, 0] += 1e-3
    assert not TD.gate(torch.from_numpy(part), pw, pm)[0], "the GraphNorm-partials gate took a row past N"


def test_every_named_mutant_was_refused_somewhere():
    """runs after the two parametrised tests above (file order): each mistake of the list met a recipe it applies to"""
    want = {("fwd", m) for m in TD.MUTANTS_FWD} | {("dgrad", m) for m in TD.MUTANTS_DGRAD} | {("partials", m) for m in TD.MUTANTS_PARTIALS}
    if not _seen:   # run on its own: the recipes that cover the list
        for r in FWD_PARAMS:
            if not r[6]:
                test_forward_gates_pass_the_restatement_and_refuse_each_mistake(*r)
        for r in DGRAD_RECIPES:
            test_dgrad_gates_pass_the_restatement_and_refuse_each_mistake(*r, False)
    assert _seen == want, sorted(want - _seen)
    assert max(_WORST.values()) < 0.5, _WORST


# ---- the entries on the host ------------------------------------------------------------------------------------------------------------
def test_k5t_entry_codes_on_the_host_before_any_launch():
    """null stream, no launch: every refusal below answers from the entry's own checks.  The `bad act` lines of the data gradient fail
    on the parent commit's library: dgrad_launch had no act check (an unknown code went on to launch and ran act_grad's ReLU formula)."""
    from glass_amd import _lib
    lib = _lib.load()
    raw = np.zeros(8200, dtype=np.float32)
    buf = raw[(-raw.ctypes.data % 16) // 4:][:8192]
    p = buf.ctypes.data
    assert p % 16 == 0
    H = 256
    forder = ["xa", "lda", "xb", "ldb", "W", "bias", "mask", "z", "act", "T", "ldt", "out", "ldo", "n", "H", "stats", "stats_exact", "gn_saved", "gn_src",
              "gn_act", "p_drop", "rng", "call", "xa_out", "ldxo", "xa_index", "xa_rows", "stream"]
    fd = dict(xa=p, lda=H, xb=None, ldb=0, W=p, bias=p, mask=p, z=Z, act=1, T=p, ldt=2 * H, out=p, ldo=H, n=8, H=H, stats=None, stats_exact=0,
              gn_saved=None, gn_src=None, gn_act=0, p_drop=0.0, rng=None, call=0, xa_out=None, ldxo=0, xa_index=None, xa_rows=0, stream=None)
    fwd = lambda **o: lib.glass_dual_linear_fwd_f32(*[dict(fd, **o)[k] for k in forder])
    pro = dict(gn_saved=p, xa_out=p, ldxo=H)
    for o in (dict(xa=None), dict(W=None), dict(bias=None), dict(mask=None), dict(out=None), dict(n=0),
              dict(lda=H + 2), dict(ldo=H + 1), dict(ldt=2 * H + 2), dict(xb=p, ldb=H + 3), dict(lda=H - 4), dict(ldt=2 * H - 4),
              dict(xa=p + 4), dict(out=p + 8), dict(T=p + 4), dict(W=p + 4), dict(bias=p + 4), dict(xb=p + 4, ldb=H),
              dict(act=3), dict(act=0xff), dict(act=3 | _lib.DENSE_F32_PRODUCTS),
              dict(xa_index=p, xa_rows=37), dict(pro, xa_index=p, xa_rows=0), dict(pro, xa_index=p, xa_rows=37, xb=p, ldb=H),
              dict(pro, p_drop=0.5), dict(pro, p_drop=1.0, rng=p), dict(pro, gn_act=3), dict(pro, xa_out=None), dict(pro, ldxo=H + 2),
              dict(pro, xa_out=p + 4), dict(pro, gn_saved=p + 4), dict(stats=p, stats_exact=4)):
        assert fwd(**o) == E_ARG, o
    assert fwd(H=192, lda=192, ldo=192, ldt=384) == E_UNSUPPORTED
    dorder = ["dsrc", "ldd", "T", "ldt", "mask", "z", "act", "WT", "n_out", "addend", "ldadd", "p_drop", "rng", "call", "out", "ldo", "n", "H",
              "gn_partial", "gn_x", "gn_ldx", "gn_saved", "gn_alpha", "gn_act", "gn_p_drop", "gn_call", "gn_exact", "stream"]
    dd = dict(dsrc=p, ldd=H, T=p, ldt=2 * H, mask=p, z=Z, act=1, WT=p, n_out=H, addend=None, ldadd=0, p_drop=0.0, rng=None, call=0, out=p, ldo=H, n=8,
              H=H, gn_partial=None, gn_x=None, gn_ldx=0, gn_saved=None, gn_alpha=None, gn_act=0, gn_p_drop=0.0, gn_call=0, gn_exact=0, stream=None)
    dg = lambda **o: lib.glass_dual_linear_dgrad_f32(*[dict(dd, **o)[k] for k in dorder])
    gn = dict(gn_partial=p, gn_x=p, gn_ldx=H, gn_saved=p, gn_alpha=p)
    for o in (dict(dsrc=None), dict(mask=None), dict(WT=None), dict(out=None), dict(n=0), dict(T=None),
              dict(ldd=H + 2), dict(ldo=H + 1), dict(ldt=2 * H + 2), dict(addend=p, ldadd=H + 2), dict(addend=p, ldadd=H - 4), dict(ldo=H - 4),
              dict(dsrc=p + 4), dict(out=p + 8), dict(T=p + 4), dict(WT=p + 4), dict(addend=p + 4, ldadd=H),
              dict(p_drop=0.5), dict(p_drop=1.0, rng=p), dict(p_drop=0.5, rng=p, n_out=2 * H, ldo=2 * H, act=0),
              dict(gn, gn_x=None), dict(gn, gn_saved=None), dict(gn, gn_alpha=None), dict(gn, gn_ldx=H + 2), dict(gn, gn_x=p + 4), dict(gn, gn_act=3),
              dict(gn, gn_p_drop=0.5), dict(gn, gn_exact=4)):
        assert dg(**o) == E_ARG, o
    for a in (3, -1 & 0xff, 3 | _lib.DENSE_F32_PRODUCTS):
        assert dg(act=a) == E_ARG, f"glass_dual_linear_dgrad_f32 took act {a}"
        assert b"dual_linear_dgrad: bad act" in lib.glass_last_error_string()
    for n_out in (H // 2, 3 * H, H + 4, 0):
        assert dg(n_out=n_out, ldo=4 * H) == E_UNSUPPORTED, n_out
