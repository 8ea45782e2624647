"""tests/staged_dense_oracle.py checked on the CPU: the restated dispatch against the source text of dense.hip / dense_common.h /
wgrad_common.h (every text condition by name), every case of tests/test_gpu_staged_dense.py against the form it is named for, the
coverage of the kernel instantiations by the case lists, every gate against the honest fp32 restatement (it must pass with room; the
worst share is printed) and against one mistake at a time (each must be refused), and the entries' argument checks that answer before
any launch."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import graphnorm_oracle as G  # noqa: E402
import staged_dense_oracle as SD  # noqa: E402
import wgrad_oracle as WO  # noqa: E402

E_ARG, E_UNSUPPORTED = -1, -3
Z = 0.85
_WORST, _SEEN = {}, set()


def _note(stage, share):
    _WORST[stage] = max(_WORST.get(stage, 0.0), share)


def _passes(stage, got, want, mass):
    ok, share, at = SD.gate(torch.as_tensor(got), want, mass)
    assert ok and share < 0.5, f"{stage}: the honest restatement takes {share:.3g} of the bar (index {at}): the mass is wrong"
    _note(stage, share)


def _refuses(name, got, want, mass):
    assert not SD.gate(torch.as_tensor(got), want, mass)[0], f"the gate took mutant {name}"
    _SEEN.add(name)


# ---- the dispatch and the source text -------------------------------------------------------------------------------------------------
def test_restated_dispatch_is_tied_to_the_source_text():
    moved = SD.check_source(SD.source_constants())
    assert not moved, f"moved in the source text: {moved}"


def test_an_edited_condition_is_named(tmp_path):
    """two conditions edited in a scratch copy of dense.hip: the tall switch of the trans forward and kFusedBwdMaxRows' use in the
    fused launch's condition"""
    src = os.path.join(SD.ROOT, "glass_amd", "csrc")
    for n in ("dense.hip", "dense_common.h", "wgrad_common.h", "linear.hip"):
        shutil.copy(os.path.join(src, n), tmp_path / n)
    text = (tmp_path / "dense.hip").read_text()
    edits = {"trans_tall_text": ("(stats == nullptr || stats_exact) && grid.x > 256 && wg80 <= 256;\n#define GLASS_TF2", "(stats == nullptr || stats_exact) && grid.x > 255 && wg80 <= 256;\n#define GLASS_TF2"),
             "fused_cond_text": ("if (wg && H == 64 && n_nodes <= kFusedBwdMaxRows &&", "if (wg && H == 64 && n_nodes < kFusedBwdMaxRows &&")}
    for name, (old, new) in edits.items():
        assert text.count(old) == 1
        (tmp_path / "dense.hip").write_text(text.replace(old, new))
        assert SD.check_source(SD.source_constants(str(tmp_path))) == [name]
    (tmp_path / "dense.hip").write_text(text)
    assert SD.check_source(SD.source_constants(str(tmp_path))) == []


def test_every_case_takes_the_form_it_is_named_for():
    for N, stats, rows in SD.TRANS_FWD_TALL:
        for f32p in (False, True):
            f = SD.fwd_form(64, False, N, stats[0] != "none", stats[1], f32p)
            assert f["rows"] == rows and f["kernel"] == f"trans_fwd2_kernel<64, {5 if rows == 80 else 4}, 2{'' if f32p else ', true'}>"
    assert all(SD.fwd_form(64, False, c[0], c[6][0] != "none", c[6][1], c[1])["rows"] == 64 for c in SD.TRANS_FWD_SMALL)
    # the pairwise cover: every value of every axis of the trans forward in both product forms
    for f32p in (False, True):
        cs = [c for c in SD.TRANS_FWD_SMALL if c[1] == f32p]
        assert {c[2] for c in cs} == {False, True} and {c[4] for c in cs} == {0, 1, 2} and {c[5] for c in cs} == {False, True}
        assert {c[6][0] for c in cs} == {"none", "part", "exact"} and {None if c[3] is None else c[3][0] for c in cs} >= {None, 0, 1, 2}
        assert {c[3][1] for c in cs if c[3]} == {0.0, 0.5}
    assert {c[6][1] for c in SD.TRANS_FWD_SMALL if c[6][0] == "exact"} == {2, 4, 8, 16} and any(c[7] for c in SD.TRANS_FWD_SMALL)
    assert set(SD.ROWS_64) <= {c[0] for c in SD.TRANS_FWD_SMALL}
    for N, comb in SD.BWD_64:
        for f32p in (False, True):
            f = SD.dgrad_form(64, 128 if comb else 64, N, True, f32p)
            assert f["fused"] == (N <= 100000)
            want = "dual_bwd_kernel<64, 128>" if comb else ("dual_bwd_kernel<64, 64>" if f32p else "dual_bwd_kernel<64, 64, true>")
            assert f["kernels"][0] == (want if f["fused"] else ("dual_dgrad_kernel<64, 128, 1, 4>" if comb else "dual_dgrad_kernel<64, 64, 1, 4> (trans_dgrad2_body<64>)"))
    for N, name, cap, stats, p, family, rows_main in SD.EFF_FWD_FORMS:
        cap = SD.label_list(name, N, cap)[3]
        for f32p in (False, True):
            f = SD.comb_eff_fwd_form(64, N, cap, stats[0] != "none", stats[1], p, f32p)
            assert family in f["kernel"].replace("_kernel", "").replace("comb_fwd_", "") and f["rows_main"] == rows_main
            assert f["forced"] == (family == "eff3" and not f32p), "a tall comb forward at hidden 64 forms f32 products whatever the option"
            assert f["tall"] or f["n_wg"] == SD.comb_eff_fwd_blocks(N, cap)
    f = SD.comb_eff_fwd_form(64, 20481, 1088, True, 0, 0.0, False)
    assert (f["rows_main"], f["n_main"], f["n_extra"]) == (96, 214, 17)
    for N, k in SD.TRANS_DGRAD_128:
        assert SD.dgrad_form(128, 128, N, False, True)["kernels"] == [k] and SD.dgrad_form(128, 128, N, False, False)["kernels"] == ["trans_dgrad3_kernel<128, true>"]
    assert SD.fwd_form(128, False, 16384, True, 0)["rows"] == 64 and SD.fwd_form(128, False, 16385, True, 0)["rows"] == 80
    g = SD.comb_eff_bwd_form(1000, 128)
    assert (g["n_dg"], g["n_s"], g["n_l"], g["rows_per_slab"]) == (18, 16, 2, 64)
    assert SD.comb_eff_bwd_form(100001, 5056)["kernels"] == ["comb_dgrad_eff_kernel<64>", "wgrad_sl_kernel"]
    assert SD.comb_eff_bwd_form(1000, 128, False)["kernels"] == ["comb_dgrad_eff_kernel<64>"]


def test_the_fused_launch_conditions_have_no_far_side():
    """rows_per_slab % 32 / ny == 1 of the fused trans launch and rows_per_slab % 32 of the fused comb launch hold for every row count the
    fused launches serve: both product forms are reached through the call's option alone"""
    assert SD.fused_condition_sweep(1) == ([], []), "every N of 1 .. kFusedBwdMaxRows"
    for N in (1, 63, 64, 65, 2047, 2048, 2049, 31999, 99999, 100000):
        assert WO.wgrad_geom(N, 128, 64)["rows"] % 32 == 0 and SD.wgrad_sl_geom(N, 64)["rows"] % 32 == 0


def test_the_case_lists_name_every_instantiation():
    named = SD.named_kernels()
    want = set(SD.INSTANTIATIONS_64) | set(SD.INSTANTIATIONS_128)
    assert not (want - named), f"no case names {sorted(want - named)}"
    assert not (named - want), f"the case lists reach kernels the lists of instantiations do not hold: {sorted(named - want)}"


def test_label_lists():
    for name in SD.LISTS:
        for N in (77, 1000):
            mask, lab, count, cap = SD.label_list(name, N, None if name != "empty0" else 0)
            rows = lab[:count].tolist()
            assert len(set(rows)) == count and sorted(rows) == np.nonzero(mask)[0].tolist() and count <= cap and len(lab) == max(cap, 1)
    assert SD.label_list("tail_oob", 1000, 128)[1][5:].min() >= 1000 and SD.label_list("n65", 1000, 128)[2:] == (65, 128)
    assert SD.label_list("all", 77)[2] == 77 and SD.label_list("last", 77)[1][0] == 76
    mask, lab, count, cap = SD.label_list("n65", 1000, 128)
    e = SD.entry_rows(1000, SD.comb_eff_fwd_form(64, 1000, cap, True, 0), mask, lab, count)
    assert len(e) == 18 and len(e[16]) == 64 and len(e[17]) == 1 and sum(len(x) for x in e) == 1000
    e = SD.entry_rows(16385, SD.fwd_form(128, False, 16385, True, 0))
    assert len(e) == 257 and [len(x) for x in e[:205]] == [80] * 204 + [65] and all(len(x) == 0 for x in e[205:])


# ---- the gates on the fp32 restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("H,comb,N,act", [(64, False, 77, 1), (64, True, 65, 0), (64, False, 1000, 2), (128, False, 65, 1)])
def test_two_product_forward_and_data_gradient(H, comb, N, act, split):
    p = SD.recipe(H, N, comb)
    mask = WO.random_mask(N, 3)
    keep = G.keep_mask(N, H, 0.5, 5)
    A32 = SD.TD.restate_prologue(p["xa"].numpy(), p["saved"].numpy(), 1, keep.numpy())
    _passes("xa_out", A32, *SD.stage_prologue(p["xa"], p["saved"], 1, keep))
    tr = SD.stage_fwd(torch.from_numpy(A32), p["xb"], p["W"], p["b"], mask, Z, act)
    xb = None if p["xb"] is None else p["xb"].numpy()
    got = SD.restate_fwd(A32, xb, p["W"].numpy(), p["b"].numpy(), mask, Z, act, split)
    _passes("T", got["T"], tr["T"], tr["T_m"])
    _passes("out", got["out"], tr["out"], tr["out_m"])
    entries = SD.entry_rows(N, SD.fwd_form(H, comb, N, True, 0, not split) if not (H == 128 and comb) else None)
    sw, sm = SD.stage_entry_stats(torch.from_numpy(got["out"]), entries)
    _passes("stats", SD.restate_entry_stats(got["out"], entries), sw, sm)
    _refuses("row_N_in_partial", SD.restate_entry_stats(got["out"], entries, extra_row=np.full(H, 1e-2)), sw, sm)
    for mut in ("drop_kstep", "swap_w"):
        _refuses(mut, SD.restate_fwd(A32, xb, p["W"].numpy(), p["b"].numpy(), mask, Z, act, split, mutant=mut)["out"], tr["out"], tr["out_m"])
    n_out = 2 * H if comb else H
    dk = G.keep_mask(N, n_out, 0.5, 9) if not comb else None
    want, mass = SD.stage_dgrad(p["dsrc"], p["T"], p["W"], mask, Z, act, n_out, p["addend"], dk)
    args = (p["dsrc"].numpy(), p["T"].numpy(), p["W"].numpy(), mask, Z, act, n_out, split)
    kw = dict(addend=p["addend"].numpy(), keep=None if dk is None else dk.numpy())
    dg = SD.restate_dgrad(*args, **kw)
    _passes("dgrad", dg, want, mass)
    for mut in ("drop_kstep", "swap_w", "addend_dropped") + (("dropout_twice", ) if dk is not None else ()):
        _refuses(mut, SD.restate_dgrad(*args, mutant=mut, **kw), want, mass)
    gk = G.keep_mask(N, H, 0.5, 11)
    ent = SD.entry_rows(N, SD.dgrad_form(H, n_out, N, False, not split)) if H == 64 else [np.arange(N)]
    pw, pm = SD.stage_entry_gn(torch.from_numpy(dg[:, :H]), p["gn_x"], p["saved"], p["alpha"], 0, gk, ent)
    part = np.stack([SD.TD.restate_gn_partials(dg[e, :H], p["gn_x"].numpy()[e], p["saved"].numpy(), p["alpha"].numpy(), 0, gk.numpy()[e], len(e), rows=len(e))[0] for e in ent])
    _passes("gn_partials", part, pw, pm)
    print("staged host worst shares: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(_WORST.items())))


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("N,name,cap", [(77, "last", None), (1000, "n65", 128), (200, "tail_oob", 128), (77, "all", None)])
def test_effective_weight_forward_and_backward(N, name, cap, split):
    H = 64
    p = SD.recipe(H, N, True)
    mask, lab, count, cap = SD.label_list(name, N, cap)
    keep = G.keep_mask(N, H, 0.5, 5)
    A32 = SD.TD.restate_prologue(p["xa"].numpy(), p["saved"].numpy(), 0, keep.numpy())
    want_A, mass_A = SD.stage_prologue(p["xa"], p["saved"], 0, keep)
    _passes("xa_out", A32, want_A, mass_A)
    _refuses("dropout_twice", (A32 * keep.numpy()).astype(np.float32), want_A, mass_A)
    tr = SD.stage_fwd(torch.from_numpy(A32), p["xb"], p["W"], p["b"], mask, Z, 0)
    args = (A32, p["xb"].numpy(), p["W"].numpy(), p["b"].numpy(), Z, split, lab, count)
    out = SD.restate_eff_fwd(*args)
    _passes("eff_out", out, tr["out"], tr["out_m"])
    form = SD.comb_eff_fwd_form(H, N, cap, True, 0, 0.5, not split)
    entries = SD.entry_rows(N, form, mask, lab, count)
    sw, sm = SD.stage_entry_stats(torch.from_numpy(out), entries)
    _passes("stats", SD.restate_entry_stats(out, entries), sw, sm)
    muts = ["drop_kstep", "listed_unlabeled"] + (["list_entry_count"] if name in ("n65", "last") else [])
    for mut in muts:
        _refuses(mut, SD.restate_eff_fwd(*args, mutant=mut), tr["out"], tr["out_m"])
    want, mass = SD.stage_dgrad(p["dsrc"], None, p["W"], mask, Z, 0, 2 * H)
    dargs = (p["dsrc"].numpy(), p["W"].numpy(), Z, split, lab, count)
    _passes("eff_dgrad", SD.restate_eff_dgrad(*dargs), want, mass)
    for mut in muts:
        _refuses(mut, SD.restate_eff_dgrad(*dargs, mutant=mut), want, mass)
    # the S / L weight gradient of the fused launch
    bf = SD.comb_eff_bwd_form(N, cap, True, not split)
    wf = SD.sl_form_of(bf)
    tW, mW, tb, mb = WO.truth_dual(p["dsrc"], None, mask, Z, 0, p["xa"], p["xb"], True)
    wargs = (wf, p["dsrc"].numpy(), None, mask, Z, 0, p["xa"].numpy(), p["xb"].numpy(), N)
    dW, db = SD.restate_wgrad(*wargs)
    _passes("dW_sl", dW, tW, mW)
    _passes("db_sl", db, tb, mb)
    for mut in ("stage16_skipped", "swap_cs_cl"):
        _refuses(mut, SD.restate_wgrad(*wargs, mutant=mut)[0], tW, mW)


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("N,comb", [(77, False), (1000, False), (333, True)])
def test_fused_weight_gradient_plain_form(N, comb, split):
    p = SD.recipe(64, N, comb)
    mask = WO.random_mask(N, 4)
    act = 0 if comb else 1
    form = SD.dgrad_form(64, 128 if comb else 64, N, True, not split)
    wf = SD.wgrad_form_of(form)
    tW, mW, tb, mb = WO.truth_dual(p["dsrc"], p["T"], mask, Z, act, p["xa"], p["xb"] if comb else None, False)
    wargs = (wf, p["dsrc"].numpy(), p["T"].numpy(), mask, Z, act, p["xa"].numpy(), p["xb"].numpy() if comb else None, N)
    dW, db = SD.restate_wgrad(*wargs)
    _passes("dW", dW, tW, mW)
    _passes("db", db, tb, mb)
    _refuses("stage16_skipped", SD.restate_wgrad(*wargs, mutant="stage16_skipped")[0], tW, mW)


def test_every_named_mutant_was_refused_somewhere():
    """runs the recipes that cover the list itself (whatever ran before): each mistake of MUTANTS meets a recipe it applies to"""
    _SEEN.clear()
    test_two_product_forward_and_data_gradient(64, False, 77, 1, True)
    test_effective_weight_forward_and_backward(1000, "n65", 128, True)
    test_fused_weight_gradient_plain_form(77, False, True)
    assert _SEEN == set(SD.MUTANTS), sorted(set(SD.MUTANTS) ^ _SEEN)
    print("staged host worst shares: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(_WORST.items())))
    assert max(_WORST.values()) < 0.5


def test_backward_accumulators_cannot_be_held_to_the_exact_bound():
    """Why gn_exact stays with the 1e-5 * mass gate.  The backward accumulators sum g' and g' * xhat, where g' = g * keep * act'(h) and
    xhat = (x - alpha mu) rstd are formed in fp32 by the kernel and never written: the only tensor read back is g.  Summed EXACTLY (fp64,
    column_sums_exact), the fp32 terms of the restatement still lie orders of magnitude outside exact_bound_terms of the fp64 terms of the
    read-back g — the distance is the rounding of the terms (2^-24 each), which no summation order removes —, while they pass the mass
    gate with room.  S1 without activation and dropout is the one sum whose terms ARE the read-back values: it meets the bound."""
    N, H = 1000, 64
    p = SD.recipe(H, N, False)
    g = p["dsrc"]
    keep = G.keep_mask(N, H, 0.5, 11)
    for act, kp in ((1, keep), (0, None)):
        t64 = SD.gn_terms(g, p["gn_x"], p["saved"], p["alpha"], act, kp)
        want, bound = SD.exact_bound_terms(t64, 20, 16, G.SCALE_BWD)
        x32, sv, al = p["gn_x"].numpy(), p["saved"].numpy(), p["alpha"].numpy()
        g32 = G._g32(g.numpy(), x32, sv, act, None if kp is None else kp.numpy())
        xhat32 = ((x32 - (al * sv[0]).astype(np.float32)).astype(np.float32) * sv[1]).astype(np.float32)
        got = torch.stack([SD.column_sums_exact(torch.from_numpy(g32).double())[0],
                           SD.column_sums_exact(torch.from_numpy(g32).double() * torch.from_numpy(xhat32).double())[0]])
        ratio = (got - want).abs() / bound
        pw, pm = G.stage_bwd_sums(g, p["gn_x"], p["saved"].float(), p["alpha"], act, kp)
        ok, share, _ = SD.gate(got, pw, pm)
        print(f"backward sums of exactly added fp32 terms, act={act}: |err| / exact bound S1 {float(ratio[0].max()):.3g} S2 {float(ratio[1].max()):.3g}; share of the mass bar {share:.3g}")
        assert ok and share < 0.5 and float(ratio[1].max()) > 1e3
        assert (float(ratio[0].max()) <= 1.0) == (act == 0), "S1 of a plain gradient is a sum of read-back values; with act' or dropout it is not"


# ---- the entries on the host ------------------------------------------------------------------------------------------------------------
def test_staged_entry_codes_on_the_host_before_any_launch():
    """null stream, no launch: every refusal below answers from the entry's own checks (hidden 64 and the hidden-128 stage-run forms)"""
    from glass_amd import _lib
    lib = _lib.load()
    raw = np.zeros(8200, dtype=np.float32)
    buf = raw[(-raw.ctypes.data % 16) // 4:][:8192]
    p = buf.ctypes.data
    H = 64
    corder = ["xa", "lda", "xb", "ldb", "W", "bias", "mask", "z", "out", "ldo", "n", "H", "stats", "stats_exact", "gn_saved", "gn_src", "gn_act", "p_drop", "rng",
              "call", "xa_out", "ldxo", "lab_rows", "lab_count", "lab_cap", "stream"]
    cd = dict(xa=p, lda=H, xb=p, ldb=H, W=p, bias=p, mask=p, z=Z, out=p, ldo=H, n=8, H=H, stats=None, stats_exact=0, gn_saved=None, gn_src=None, gn_act=0,
              p_drop=0.0, rng=None, call=0, xa_out=None, ldxo=0, lab_rows=p, lab_count=p, lab_cap=64, stream=None)
    cf = lambda **o: lib.glass_comb_eff_fwd_f32(*[dict(cd, **o)[k] for k in corder])
    pro = dict(gn_saved=p, xa_out=p, ldxo=H)
    for o in (dict(xa=None), dict(xb=None), dict(W=None), dict(bias=None), dict(mask=None), dict(out=None), dict(lab_rows=None), dict(lab_count=None), dict(n=0),
              dict(lab_cap=-1), dict(lda=H + 2), dict(ldb=H - 4), dict(ldo=H + 1), dict(xa=p + 4), dict(out=p + 8), dict(stats=None, stats_exact=4),
              dict(stats=p, stats_exact=3), dict(pro, p_drop=0.5), dict(pro, p_drop=1.0, rng=p), dict(pro, xa_out=None), dict(pro, ldxo=H + 2),
              dict(pro, gn_act=1), dict(pro, gn_act=3)):
        assert cf(**o) == E_ARG, o
    assert cf(H=256, lda=256, ldb=256, ldo=256) == E_UNSUPPORTED and cf(H=32, lda=32, ldb=32, ldo=32) == E_UNSUPPORTED
    border = ["dsrc", "ldd", "mask", "z", "WT", "out", "ldo", "n", "H", "gn_partial", "gn_x", "gn_ldx", "gn_saved", "gn_alpha", "gn_act", "gn_p_drop", "rng", "gn_call",
              "gn_exact", "X", "ldx", "X2", "ldx2", "ws", "lab_rows", "lab_count", "lab_cap", "dsrc_gn", "stream"]
    bd = dict(dsrc=p, ldd=H, mask=p, z=Z, WT=p, out=p, ldo=2 * H, n=8, H=H, gn_partial=None, gn_x=None, gn_ldx=0, gn_saved=None, gn_alpha=None, gn_act=0,
              gn_p_drop=0.0, rng=None, gn_call=0, gn_exact=0, X=p, ldx=H, X2=p, ldx2=H, ws=p, lab_rows=p, lab_count=p, lab_cap=64, dsrc_gn=None, stream=None)
    cb = lambda **o: lib.glass_comb_eff_bwd_f32(*[dict(bd, **o)[k] for k in border])
    gn = dict(gn_partial=p, gn_x=p, gn_ldx=H, gn_saved=p, gn_alpha=p)
    for o in (dict(dsrc=None), dict(mask=None), dict(WT=None), dict(out=None), dict(lab_rows=None), dict(lab_count=None), dict(n=0), dict(lab_cap=-1),
              dict(ldd=H + 2), dict(ldo=2 * H - 4), dict(ldo=2 * H + 2), dict(dsrc=p + 4), dict(out=p + 4), dict(WT=p + 4), dict(X2=None), dict(ws=None),
              dict(ldx=H + 2), dict(ldx2=H - 4), dict(X=p + 4), dict(ws=p + 4), dict(gn, gn_x=None), dict(gn, gn_saved=None), dict(gn, gn_ldx=H + 2),
              dict(gn, gn_p_drop=0.5), dict(gn, gn_act=3), dict(gn, gn_act=1), dict(gn_exact=4), dict(gn, gn_exact=3)):
        assert cb(**o) == E_ARG, o
    assert cb(H=128, ldd=128, ldo=256, ldx=128, ldx2=128) == E_UNSUPPORTED
    # the dsrc_gn form is the fused launch's: no data-gradient-only call, nothing beyond kFusedBwdMaxRows, hidden 64 only
    src = _lib.GnBwdSrc(p, 4, p, H, p, H, None, 0, p, p, p, p, p, p, 0, 0, 0.0, 0)
    assert lib.glass_comb_eff_bwd_gn_src_supported(100000, 64) == 1 and lib.glass_comb_eff_bwd_gn_src_supported(100001, 64) == 0
    assert lib.glass_comb_eff_bwd_gn_src_supported(1000, 128) == 0
    assert cb(dsrc=None, dsrc_gn=src.ptr, X=None) == E_UNSUPPORTED and cb(dsrc=None, dsrc_gn=src.ptr, n=100001) == E_UNSUPPORTED
    assert cb(dsrc=None, dsrc_gn=None) == E_ARG
    for bad in (dict(n_rep=3), dict(acc=None), dict(lddy=H + 2), dict(p_drop=0.5), dict(act=3), dict(gamma=None)):
        f = dict(acc=p, n_rep=4, dy=p, lddy=H, x=p, ldx=H, addend=None, ldadd=0, saved=p, gamma=p, alpha=p, dgamma=p, dbeta=p, dalpha=p, accumulate=0, act=0, p_drop=0.0, call_id=0)
        f.update(bad)
        assert cb(dsrc=None, dsrc_gn=_lib.GnBwdSrc(*f.values()).ptr) == E_ARG, bad
    # the fused entry of the Linear pair: its own checks, and those of the data gradient it shares
    worder = ["dsrc", "ldd", "T", "ldt", "mask", "z", "act", "WT", "n_out", "addend", "ldadd", "p_drop", "rng", "call", "out", "ldo", "n", "H", "gn_partial", "gn_x",
              "gn_ldx", "gn_saved", "gn_alpha", "gn_act", "gn_p_drop", "gn_call", "gn_exact", "X", "ldx", "X2", "ldx2", "ws", "stream"]
    wd = dict(dsrc=p, ldd=H, T=p, ldt=2 * H, mask=p, z=Z, act=1, WT=p, n_out=H, addend=None, ldadd=0, p_drop=0.0, rng=None, call=0, out=p, ldo=H, n=8, H=H,
              gn_partial=None, gn_x=None, gn_ldx=0, gn_saved=None, gn_alpha=None, gn_act=0, gn_p_drop=0.0, gn_call=0, gn_exact=0, X=p, ldx=H, X2=None, ldx2=0, ws=p,
              stream=None)
    wb = lambda **o: lib.glass_dual_linear_bwd_f32(*[dict(wd, **o)[k] for k in worder])
    for o in (dict(X=None), dict(ws=None), dict(dsrc=None), dict(act=3), dict(T=None), dict(ldd=H + 2), dict(ldo=H - 4), dict(p_drop=0.5), dict(ldx=H + 1),
              dict(X=p + 4), dict(X2=p, ldx2=H + 1), dict(gn_exact=4), dict(gn_partial=p, gn_x=p, gn_ldx=H, gn_saved=p, gn_alpha=p, gn_exact=3)):
        assert wb(**o) == E_ARG, o
    assert wb(n_out=3 * H, ldo=4 * H) == E_UNSUPPORTED
    # hidden 128: the comb pair's stage-run data gradient takes no activation, addend or dropout; no exact accumulators at this width
    dorder = worder[:27] + ["stream"]
    dg = lambda **o: lib.glass_dual_linear_dgrad_f32(*[dict(wd, H=128, ldd=128, ldt=256, **o)[k] for k in dorder])
    assert dg(n_out=256, ldo=256, act=1) == E_UNSUPPORTED and dg(n_out=256, ldo=256, act=0, addend=p, ldadd=256) == E_UNSUPPORTED
    # dropout with n_out = 2H never reaches that refusal: the entry's own dropout check (the masked output must be the [N, H] layer input) answers GLASS_E_ARG first
    assert dg(n_out=256, ldo=256, act=0, p_drop=0.5, rng=p) == E_ARG
    assert dg(n_out=128, ldo=128, gn_partial=p, gn_x=p, gn_ldx=128, gn_saved=p, gn_alpha=p, gn_exact=4) == E_ARG
