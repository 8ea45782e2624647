"""The whole-graph GraphNorm (K6) without a GPU: the stage chain of tests/graphnorm_oracle.py equals oracle.glass_oracle.GraphNorm
under autograd (all three activations, the addend, accumulate and dropout by given masks), an fp32 restatement of every stage IN
THE KERNELS' SUMMATION ORDER passes every gate below half its bar on every recipe (worst share printed per stage; the share of
excluded activation kinks printed per recipe, <= 0.1 %), the gate refuses each single mistake a kernel could make, the restated
dispatch has the constants of the source text and the expected form on both sides of every threshold, the accumulator limbs
round-trip in exact integers, and the argument codes of every K6 entry through the real library before any launch."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import graphnorm_oracle as G  # noqa: E402

ACTS = (G.ACT_NONE, G.ACT_ELU, G.ACT_RELU)
E_ARG = -1


# ---- the chain is the autograd statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "mixed", "flat"])
@pytest.mark.parametrize("act", ACTS)
def test_chain_equals_autograd(act, kind):
    ins = G.recipe(97, 12, 11, kind)
    keep = G.keep_mask(97, 12, 0.5, 12)
    g = torch.Generator().manual_seed(13)
    prev = tuple(torch.randn(12, generator=g) for _ in range(3))
    for kp in (None, keep):
        want = G.autograd_graphnorm(ins, act, kp)
        got = G.chain(ins, act, kp)
        assert not bool(got["kinks"].any())
        for k in ("y", "dx", "dgamma", "dbeta", "dalpha"):
            assert G.rel_inf(got[k], want[k]) < 1e-12, (k, kp is not None)
        # by linearity: the addend is added to dx, the previous contents to the parameter gradients
        more = G.chain(ins, act, kp, addend=ins["addend"], prev=prev)
        assert G.rel_inf(more["dx"], want["dx"] + ins["addend"].double()) < 1e-12
        for k, p in zip(("dgamma", "dbeta", "dalpha"), prev):
            assert G.rel_inf(more[k], want[k] + p.double()) < 1e-12, k


# ---- fp32 restatement in the kernels' order ----------------------------------------------------------------------------------------
def _fwd_coeffs(S, Q, N, gamma, beta, alpha, eps):
    """gn_math.h gn_fwd_coeffs in numpy fp64 -> saved [4, C] fp32"""
    a = alpha.astype(np.float64)
    mu = S / N
    var = np.maximum(Q / N - mu * mu * (2.0 * a - a * a), 0.0)
    rstd = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
    scale = gamma.astype(np.float64) * rstd
    return np.stack([mu, rstd, scale, beta.astype(np.float64) - scale * a * mu]).astype(np.float32)


def _restate(ins, act, keep, vec, addend=True):
    """every stage in the kernels' order -> dict of tensors (partials in fp64, the rest fp32)"""
    x, dy = ins["x"].numpy(), ins["dy"].numpy()
    N = x.shape[0]
    kp = None if keep is None else keep.numpy()
    part = G.restate_stats(x, vec)
    SQ = G.fin_order_sum(part)
    saved = _fwd_coeffs(SQ[0], SQ[1], float(N), ins["gamma"].numpy(), ins["beta"].numpy(), ins["alpha"].numpy(), ins["eps"])
    y = G.restate_apply(x, saved, act, kp)
    bpart = G.restate_bwd_stats(dy, x, saved, ins["alpha"].numpy(), act, kp, vec)
    S12 = torch.from_numpy(G.fin_order_sum(bpart))
    Gn = G.stage_gn_bwd(*G.sums_as_partial(S12), N, ins["gamma"], ins["alpha"], torch.from_numpy(saved))
    coef = Gn["coef"][0].float()
    dx = G.restate_dx(dy, x, saved, coef.numpy(), ins["addend"].numpy() if addend else None, act, kp)
    out = dict(part=torch.from_numpy(part), saved=torch.from_numpy(saved), y=torch.from_numpy(y), bpart=torch.from_numpy(bpart), coef=coef,
               dx=torch.from_numpy(dx))
    out.update({k: Gn[k][0].float() for k in ("dgamma", "dbeta", "dalpha")})
    return out


def grade(got, ins, act, keep, addend=True, prev=None):
    """every stage of `got` through its gate, each from the upstream outputs in `got` -> dict stage -> (ok, share, index)"""
    x, N = ins["x"], ins["x"].shape[0]
    out = {}
    out["sums"] = G.gate(got["part"].sum(0), *G.stage_sums(x))
    out["saved"] = G.gate(got["saved"], *G.stage_saved(x, ins["gamma"], ins["beta"], ins["alpha"], ins["eps"]))
    sv = got["saved"]
    out["y"] = G.gate(got["y"], *G.stage_apply(x, sv, act, keep))
    out["bsums"] = G.gate(got["bpart"].sum(0), *G.stage_bwd_sums(ins["dy"], x, sv, ins["alpha"], act, keep))
    Gn = G.stage_gn_bwd(got["bpart"], got["bpart"].abs(), N, ins["gamma"], ins["alpha"], sv, prev)
    for k in ("coef", "dgamma", "dbeta", "dalpha"):
        out[k] = G.gate(got[k], *Gn[k])
    out["dx"] = G.gate(got["dx"], *G.stage_dx(ins["dy"], x, sv, got["coef"], ins["addend"] if addend else None, act, keep))
    return out


_WORST = {}


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("N,C,vec", [(300, 20, True), (97, 17, False)])
def test_fp32_restatement_in_kernel_order_passes_every_gate_below_half_the_bar(N, C, vec, act, kind):
    """(no mass term had to change for any recipe: every stage stays below half the bar with the masses of the module docstring)"""
    ins = G.recipe(N, C, 21 + C, kind)
    keep = G.keep_mask(N, C, 0.5, 22) if act != G.ACT_NONE else None
    got = _restate(ins, act, keep, vec)
    res = grade(got, ins, act, keep)
    kink = float(G.kinks(ins["x"], got["saved"], act).double().mean())
    print(f"fp32 restatement {kind} act {act} N {N} C {C}: " + " ".join(f"{k} {v[1]:.3f}" for k, v in res.items()) + f" | kinks {100 * kink:.4f} %")
    assert kink <= G.KINK_CAP
    assert all(v[0] and v[1] <= 0.5 for v in res.values()), res
    for k, v in res.items():
        _WORST[k] = max(_WORST.get(k, 0.0), v[1])
    want = G.chain(ins, act, keep, addend=ins["addend"])
    ok_cols = ~want["kinks"].any(0)
    for k in ("y", "dx", "dgamma", "dbeta", "dalpha"):
        sel = (lambda t: t[..., ok_cols])
        assert G.rel_inf(sel(got[k]), sel(want[k])) <= G.TOL, k


def test_zz_print_worst_restatement_shares():
    print("WORST fp32 restatement: " + " ".join(f"{k} {v:.3f}" for k, v in _WORST.items()))
    assert all(v <= 0.5 for v in _WORST.values())


def test_restated_exact_statistics_stay_inside_the_derived_bound():
    """gn_stats64_exact_kernel's order through integer limbs, decoded: inside exact_sum_bound; one replica left out of the fold,
    or the lo limbs ignored, is not"""
    for N, n_rep in ((17, 1), (200, 4), (200, 16)):
        x = G.recipe(N, 64, 5, "plain")["x"]
        words = G.restate_stats64(x.numpy(), n_rep)
        form = G.exact_stats_form(N, 64, True)
        want, bound = G.exact_sum_bound(x, 64, form, adds=form[2])
        dec = G.acc_decode(words, 64, n_rep, G.SCALE_FWD)
        err = (dec["value"] - want).abs()
        print(f"restated stats64 N {N} n_rep {n_rep}: worst share of the bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all())
        if n_rep > 1 and form[2] >= n_rep:
            assert not bool(((G.acc_decode(words, 64, n_rep - 1, G.SCALE_FWD)["value"] - want).abs() <= bound).all()), "a replica left out"
        hi_only = torch.tensor([[float(t >> G.LO_BITS) / G.SCALE_FWD for t in row] for row in dec["total"]], dtype=torch.float64)
        assert not bool(((hi_only - want).abs() <= bound).all()), "the lo limbs ignored"


# ---- the gate refuses single mistakes ----------------------------------------------------------------------------------------------
def _exact_got(ins, act, keep, prev=None):
    """the chain's outputs rounded to fp32 (what a correct kernel returns, up to one rounding), each stage recomputed from the
    ROUNDED upstream outputs"""
    x, N = ins["x"], ins["x"].shape[0]
    got = dict(part=G.stage_sums(x)[0].unsqueeze(0))
    got["saved"] = G.stage_saved(x, ins["gamma"], ins["beta"], ins["alpha"], ins["eps"])[0].float()
    sv = got["saved"]
    got["y"] = G.stage_apply(x, sv, act, keep)[0].float()
    got["bpart"] = G.stage_bwd_sums(ins["dy"], x, sv, ins["alpha"], act, keep)[0].unsqueeze(0)
    Gn = G.stage_gn_bwd(got["bpart"], got["bpart"].abs(), N, ins["gamma"], ins["alpha"], sv, prev)
    got.update({k: Gn[k][0].float() for k in ("coef", "dgamma", "dbeta", "dalpha")})
    got["dx"] = G.stage_dx(ins["dy"], x, sv, got["coef"], ins["addend"], act, keep)[0].float()
    return got


def test_gate_accepts_the_rounded_truth_and_refuses_each_single_mistake():
    N, C = 97, 12
    ins = G.recipe(N, C, 31, "mixed")
    keep = G.keep_mask(N, C, 0.5, 32)
    x, dy, sv_args = ins["x"], ins["dy"], None
    for act in ACTS:
        for kp in (None, keep):
            assert all(v[0] for v in grade(_exact_got(ins, act, kp), ins, act, kp).values()), (act, kp is not None)
    act = G.ACT_ELU
    base = _exact_got(ins, act, keep)
    sv = base["saved"]
    verdict = lambda got, **kw: {k: v[0] for k, v in grade(got, ins, act, keep, **kw).items()}

    def but(**kw):
        got = dict(base)
        got.update(kw)
        return got

    # a dropped tail row: in the statistics, and a row of y / dx never written (still NaN, or the previous contents)
    assert not verdict(but(part=G.stage_sums(x[:-1])[0].unsqueeze(0)))["sums"]
    short = dict(ins, x=x[:-1])
    assert not verdict(but(saved=G.stage_saved(short["x"], ins["gamma"], ins["beta"], ins["alpha"], ins["eps"])[0].float()))["saved"]
    for fill in (float("nan"), 0.0):
        y, dx = base["y"].clone(), base["dx"].clone()
        y[-1], dx[-1] = fill, fill
        v = verdict(but(y=y, dx=dx))
        assert not v["y"] and not v["dx"], fill
    assert not verdict(but(bpart=G.stage_bwd_sums(dy[:-1], x[:-1], sv, ins["alpha"], act, keep[:-1])[0].unsqueeze(0)))["bsums"]
    # a column shifted by one: the output, the coefficients used
    v = verdict(but(y=base["y"].roll(1, 1), dx=base["dx"].roll(1, 1)))
    assert not v["y"] and not v["dx"]
    assert not verdict(but(y=G.stage_apply(x, sv.roll(1, 1), act, keep)[0].float()))["y"]
    for which in range(3):
        coef = base["coef"].clone()
        coef[which] = coef[which].roll(1)
        assert not verdict(but(dx=G.stage_dx(dy, x, sv, coef, ins["addend"], act, keep)[0].float()))["dx"], which
    # alpha left out of xhat
    no_alpha = G.stage_bwd_sums(dy, x, sv, torch.ones(C), act, keep)[0].unsqueeze(0)
    assert not verdict(but(bpart=no_alpha))["bsums"]
    # the mask not applied in the backward
    assert not verdict(but(bpart=G.stage_bwd_sums(dy, x, sv, ins["alpha"], act, None)[0].unsqueeze(0)))["bsums"]
    assert not verdict(but(dx=G.stage_dx(dy, x, sv, base["coef"], ins["addend"], act, None)[0].float()))["dx"]
    # the derivative of the activation left out
    assert not verdict(but(dx=G.stage_dx(dy, x, sv, base["coef"], ins["addend"], G.ACT_NONE, keep)[0].float()))["dx"]
    # K without the a * mean(do) term
    Sb, g, a, mu, r = base["bpart"][0], ins["gamma"].double(), ins["alpha"].double(), sv[0].double(), sv[1].double()
    coef = base["coef"].clone()
    coef[2] = (g * r * r * (Sb[1] / N) * a * mu).float()
    v = verdict(but(coef=coef, dx=G.stage_dx(dy, x, sv, coef, ins["addend"], act, keep)[0].float()))
    assert not v["coef"]
    assert not verdict(but(dx=G.stage_dx(dy, x, sv, coef, ins["addend"], act, keep)[0].float()))["dx"]
    # the addend left out; accumulate overwriting
    assert not verdict(but(dx=G.stage_dx(dy, x, sv, base["coef"], None, act, keep)[0].float()))["dx"]
    prev = tuple(torch.full((C, ), v) for v in (0.25, -0.5, 2.0))
    assert all(grade(_exact_got(ins, act, keep, prev), ins, act, keep, prev=prev)[k][0] for k in ("dgamma", "dbeta", "dalpha"))
    v = verdict(base, prev=prev)
    assert not v["dgamma"] and not v["dbeta"] and not v["dalpha"]
    # ReLU returning 0 for NaN: one NaN makes its column's statistics, h and y NaN; a column of clean zeros is refused
    bad = x.clone()
    bad[5, 3], bad[9, 3] = float("nan"), float("inf")
    svn = G.stage_saved(bad, ins["gamma"], ins["beta"], ins["alpha"], ins["eps"])[0].float()
    assert bool(torch.isnan(svn[:, 3]).all()) and int(torch.isnan(svn).sum()) == 4
    for a_ in ACTS:
        want, mass = G.stage_apply(bad, svn, a_)
        assert bool(torch.isnan(want[:, 3]).all()) and int(torch.isnan(want).sum()) == N
        assert G.gate_with_nan(want.float(), want, mass)[0]
        assert G.gate_with_nan(torch.from_numpy(G.restate_apply(bad.numpy(), svn.numpy(), a_)), want, mass)[0]
        zeros = want.float().clone()
        zeros[:, 3] = 0.0
        assert not G.gate_with_nan(zeros, want, mass)[0], "a NaN column written as zeros"


# ---- dispatch -----------------------------------------------------------------------------------------------------------------
def test_restated_constants_are_the_ones_in_the_source_text():
    k = G.gn_source_constants()
    assert k["kBlock"] == G.BLOCK == 256 and k["kUnroll"] == G.UNROLL == 4 and k["kMaxStatBlocks"] == G.MAX_STAT_BLOCKS == 1024
    assert k["apply_cap"] == G.APPLY_CAP == 4096
    assert k["kFinCols"] == G.FIN_COLS == 4 and k["kFinFly"] == G.FIN_FLY == 8 and G.FIN_SLOTS == k["kBlock"] // k["kFinCols"] == 64
    assert k["kAccRep"] == G.ACC_REP == 16 and k["kAccScaleFwd"] == G.SCALE_FWD == 2.0**12 and k["kAccScaleBwd"] == G.SCALE_BWD == 2.0**24
    assert k["acc_bound"] == G.ACC_BOUND == 4.0e18 and 1 << k["poison_bit"] == G.POISON and k["lo_scale"] == float(1 << G.LO_BITS)
    assert k["kMaxStatSrc"] == G.MAX_SRC == 8
    assert G.STATS64_ROWS * G.STATS64_ROUND == 80 and G.STATS64_WGS == 256 and G.ACC64_UN == 5
    for text in ("stat_div_text", "apply_div_text", "tiling_text", "fin_slots_text", "fin_walk_text", "fin_fold_text", "lo_inv_text",
                 "index_text", "vec_fwd_text", "vec_in_text", "vec_bwd_text", "stats64_text", "bwd_exact_text"):
        assert k[text], text


def test_restated_forms_on_both_sides_of_every_threshold():
    t = G.tiling
    # tilings (vw, cw, tc, rpb, ctiles)
    assert t(4, True) == (4, 1, 1, 256, 1) and t(20, True) == (4, 5, 8, 32, 1) and t(64, True) == (4, 16, 16, 16, 1)
    assert t(1024, True) == (4, 256, 256, 1, 1) and t(1028, True) == (4, 257, 256, 1, 2)
    assert t(256, False) == (1, 256, 256, 1, 1) and t(257, False) == (1, 257, 256, 1, 2) and t(300, False) == (1, 300, 256, 1, 2)
    assert t(17, False) == (1, 17, 32, 8, 1) and t(1, False) == (1, 1, 1, 256, 1) and t(3, False) == (1, 3, 4, 64, 1)
    assert t(16, True)[3] == 64 and t(32, True)[3] == 32 and t(128, True)[3] == 8
    # the vector predicates: every operand's stride and pointer; the input-only entries do not look at y
    assert G.vec_fwd(64, 64, 64) and not G.vec_fwd(17, 20, 20) and not G.vec_fwd(64, 65, 64) and not G.vec_fwd(64, 64, 65)
    assert not G.vec_fwd(64, 64, 64, x_ptr=4) and not G.vec_fwd(64, 64, 64, y_ptr=4)
    assert G.vec_in(64, 64) and not G.vec_in(64, 65) and not G.vec_in(64, 64, 4) and not G.vec_in(3, 4)
    assert G.vec_bwd(64, 64, 64, 64) and G.vec_bwd(64, 64, 64, 64, 64) and not G.vec_bwd(64, 64, 64, 64, 65)
    assert not G.vec_bwd(64, 64, 64, 64, 64, add_ptr=4) and not G.vec_bwd(64, 68, 64, 65)
    for kw in (dict(dy_ptr=4), dict(x_ptr=4), dict(dx_ptr=4)):
        assert not G.vec_bwd(64, 64, 64, 64, **kw)
    # rows: one trip against two of the unrolled loop does not change the grid; the caps do
    assert G.stat_blocks(1, 64, True) == 1 and G.stat_blocks(128, 64, True) == 1 and G.stat_blocks(129, 64, True) == 2
    assert G.apply_blocks(63, 64, True) == G.apply_blocks(64, 64, True) == 1 and G.apply_blocks(65, 64, True) == 2
    assert G.stat_blocks(8192, 1024, True) == 1024 == G.stat_blocks(8200, 1024, True) and G.stat_blocks(8184, 1024, True) == 1023
    assert G.apply_blocks(16384, 1024, True) == 4096 == G.apply_blocks(16392, 1024, True) and G.apply_blocks(16380, 1024, True) == 4095
    # exact statistics: nst 1 -> 2, -> 5, a second and a third round of five; the generic kernel for every other width / stride
    f = G.exact_stats_form
    assert [f(n, 64, True) for n in (1, 15, 16, 17)] == [("stats64", 1, 1), ("stats64", 1, 1), ("stats64", 1, 1), ("stats64", 1, 2)]
    assert f(4096, 64, True) == ("stats64", 1, 256) and f(4097, 64, True) == ("stats64", 2, 129)
    assert f(5119, 64, True) == ("stats64", 2, 160) and f(5120, 64, True) == ("stats64", 5, 64)
    assert f(20480, 64, True) == ("stats64", 5, 256) and f(20481, 64, True) == ("stats64", 6, 214) and f(40961, 64, True) == ("stats64", 11, 233)
    assert f(300, 64, False) == ("generic", 1, (10, 1)) and f(300, 128, True) == ("generic", 4, (5, 1)) and f(300, 20, True)[0] == "generic"
    assert all(f(300, C, True)[0] == "generic" for C in (16, 32, 128, 20))
    # the exact backward: the 80-row kernel at C = 64 with two or more replicas, the LDS fold otherwise, the refusals
    b = G.bwd_exact_form
    assert b(64, 2, 80) == ("acc64x5", 1) and b(64, 2, 81) == ("acc64x5", 2) and b(64, 16, 161) == ("acc64x5", 3) and b(64, 4, 79) == ("acc64x5", 1)
    assert b(64, 1, 161) == ("acc_lds", 3) and b(16, 2, 257) == ("acc_lds", 2) and b(32, 4, 128) == ("acc_lds", 1) and b(128, 16, 33) == ("acc_lds", 2)
    for C, n_rep, kw in ((48, 2, {}), (64, 3, {}), (64, 18, {}), (64, 0, {}), (64, 2, dict(vec4=False)), (64, 2, dict(acc_aligned=False)), (256, 2, {})):
        assert b(C, n_rep, 100, **kw)[0] == "refused", (C, n_rep, kw)
    # the finalize reads every partial row below nblk once and none at or above it
    for nblk in (1, 63, 64, 65, 512, 513, 1024):
        assert G.fin_slots_read(nblk) == list(range(nblk)), nblk
    part = np.random.default_rng(0).standard_normal((513, 3))
    assert np.allclose(G.fin_order_sum(part), part.sum(0), rtol=0, atol=1e-12)


# ---- the accumulators ---------------------------------------------------------------------------------------------------------
def test_accumulator_limbs_round_trip_in_exact_integers():
    unit = lambda scale: 1.0 / (scale * float(1 << G.LO_BITS))   # the resolution
    for scale in (G.SCALE_FWD, G.SCALE_BWD):
        vals = [0.0, 1.0, -1.0, 0.75, -0.75, 123456.789, -123456.789, unit(scale), -unit(scale), unit(scale) / 4, -unit(scale) / 4,
                G.ACC_BOUND / scale, -G.ACC_BOUND / scale, 3.0 * unit(scale) - 5.0]
        for v in vals:
            hi, lo = G.acc_encode(v, scale)
            assert 0 <= lo < (1 << G.LO_BITS) and -(1 << 63) <= hi < (1 << 63)
            exact = int(np.floor(np.float64(v) * scale * float(1 << G.LO_BITS))) if abs(v) < 2.0**20 else None
            if exact is not None:  # the limbs hold floor(v * scale * 2^40) exactly (v * scale * 2^40 is an integer or is truncated)
                assert (hi << G.LO_BITS) + lo == exact, v
            words = [0] * G.acc_words(4)
            G.acc_add(words, 2, 1, 3, 4, v, scale)
            dec = G.acc_decode(words, 4, 3, scale)
            assert dec["total"][1][3] == (hi << G.LO_BITS) + lo and not dec["bad"][1][3]
            assert abs(float(dec["value"][1, 3]) - v) <= unit(scale) + abs(v) * 2.0**-52
            assert G.acc_decode(words, 4, 2, scale)["total"][1][3] == 0            # replica 2 is not among the first two
        # below the resolution: a positive value truncates to 0, a negative one to -1 unit
        assert G.acc_encode(unit(scale) / 4, scale) == (0, 0) and G.acc_encode(-unit(scale) / 4, scale) == (-1, (1 << G.LO_BITS) - 1)
        # poison: NaN, +-Inf, beyond the range; sticky under later adds, confined to its column's quantity
        for v in (float("nan"), float("inf"), float("-inf"), 4.0001e18 / scale, -4.0001e18 / scale):
            assert G.acc_encode(v, scale) is None, v
        words = [0] * G.acc_words(4)
        G.acc_add(words, 0, 0, 1, 4, float("nan"), scale)
        for _ in range(3):
            for c in range(4):
                G.acc_add(words, 0, 0, c, 4, 0.6, scale)
                G.acc_add(words, 1, 1, c, 4, -0.6, scale)
        dec = G.acc_decode(words, 4, 2, scale)
        assert dec["bad"] == [[False, True, False, False], [False] * 4] and int(torch.isnan(dec["value"]).sum()) == 1
        assert dec["total"][0][0] == 3 * ((lambda e: (e[0] << G.LO_BITS) + e[1])(G.acc_encode(0.6, scale)))
        # sums: many adds of either sign spread over replicas decode to the exact integer sum; negative hi with positive lo
        rng = np.random.default_rng(1)
        vs = rng.standard_normal(200) * 1e3
        words, total = [0] * G.acc_words(1), 0
        for i, v in enumerate(vs):
            G.acc_add(words, i % 5, 0, 0, 1, v, scale)
            e = G.acc_encode(v, scale)
            total += (e[0] << G.LO_BITS) + e[1]
        assert G.acc_decode(words, 1, 5, scale)["total"][0][0] == total
        # the tensor form is the scalar form
        t = torch.tensor(vals + [float("nan"), float("inf"), 4.0001e18 / scale], dtype=torch.float64)
        hi, lo, bad = G.acc_encode_tensor(t, scale)
        for i, v in enumerate(t.tolist()):
            e = G.acc_encode(v, scale)
            assert (e is None) == bool(bad[i]) and (e is None or (int(hi[i]), int(lo[i])) == e), v
    # the guarantee ends where the module docstring says: 2^63 / scale wraps into a finite value, unpoisoned
    words = [0] * G.acc_words(1)
    for _ in range(3):
        G.acc_add(words, 0, 0, 0, 1, 3.9e18 / G.SCALE_FWD, G.SCALE_FWD)
    dec = G.acc_decode(words, 1, 1, G.SCALE_FWD)
    assert not dec["bad"][0][0] and float(dec["value"][0, 0]) < 0
    assert G.acc_layout(0, 0, 0, 64) == 0 and G.acc_layout(0, 1, 0, 64) == 128 and G.acc_layout(1, 0, 0, 64) == 256 and G.acc_layout(2, 1, 5, 64) == 650


# ---- the entries on the host ----------------------------------------------------------------------------------------------------
def test_k6_entry_codes_on_the_host_before_any_launch():
    """null stream, no launch: every refusal below answers GLASS_E_ARG from the entry's own checks.  The two `bad act` lines of
    the backward entries fail on the parent commit's library (no act check there: the call went on to launch — without a GPU
    it answered the launch error 100 (hipErrorNoDevice) instead of -1; with one, an unknown code ran as ReLU)."""
    from glass_amd import _lib
    lib = _lib.load()
    raw = np.zeros(4100, dtype=np.float32)
    buf = raw[(-raw.ctypes.data % 16) // 4:][:4096]
    p = buf.ctypes.data
    assert p % 16 == 0
    fwd = lambda **o: lib.glass_graphnorm_fwd_f32(*_a(dict(x=p, ldx=64, y=p, ldy=64, n=8, C=64, gamma=p, beta=p, alpha=p, eps=1e-5, saved=p, act=1,
                                                          p_drop=0.0, rng=None, call=0, ws=p, stream=None), o))
    for o in (dict(x=None), dict(y=None), dict(gamma=None), dict(beta=None), dict(alpha=None), dict(saved=None), dict(ws=None), dict(n=0), dict(C=0),
              dict(ldx=63), dict(ldy=63), dict(p_drop=0.5), dict(p_drop=1.0, rng=p), dict(p_drop=-0.1), dict(act=3), dict(act=-1)):
        assert fwd(**o) == E_ARG, o
    assert b"bad act" in lib.glass_last_error_string()
    stats = lambda **o: lib.glass_graphnorm_stats_f32(*_a(dict(x=p, ldx=64, n=8, C=64, gamma=p, beta=p, alpha=p, eps=1e-5, saved=p, ws=p, stream=None), o))
    for o in (dict(x=None), dict(gamma=None), dict(saved=None), dict(ws=None), dict(n=0), dict(C=0), dict(ldx=63)):
        assert stats(**o) == E_ARG, o
    apply_ = lambda **o: lib.glass_graphnorm_apply_f32(*_a(dict(x=p, ldx=64, y=p, ldy=64, n=8, C=64, saved=p, act=1, p_drop=0.0, rng=None, call=0,
                                                              stream=None), o))
    for o in (dict(x=None), dict(y=None), dict(saved=None), dict(n=0), dict(ldx=63), dict(ldy=63), dict(p_drop=0.5), dict(act=3)):
        assert apply_(**o) == E_ARG, o
    exact = lambda **o: lib.glass_graphnorm_stats_exact_f32(*_a(dict(x=p, ldx=64, n=8, C=64, acc=p, n_rep=4, stream=None), o))
    for o in (dict(x=None), dict(acc=None), dict(n=0), dict(C=0), dict(ldx=63), dict(n_rep=0), dict(n_rep=17)):
        assert exact(**o) == E_ARG, o
    ptrs = np.array([p] * 9, dtype=np.uint64)
    fin = lambda **o: lib.glass_graphnorm_finalize_f32(*_a(dict(parts=ptrs.ctypes.data, n_src=2, nblk=4, C_each=6, n=8, gamma=p, beta=p, alpha=p, eps=1e-5,
                                                                saved=p, stream=None), o))
    for o in (dict(parts=None), dict(gamma=None), dict(saved=None), dict(n_src=0), dict(n_src=9), dict(nblk=0), dict(nblk=1 << 31), dict(C_each=0), dict(n=0)):
        assert fin(**o) == E_ARG, o
    hole = np.array([p, 0, p], dtype=np.uint64)
    assert fin(parts=hole.ctypes.data, n_src=3) == E_ARG and b"null source 1" in lib.glass_last_error_string()
    bwd_d = dict(dy=p, lddy=64, x=p, ldx=64, dx=p, lddx=64, addend=None, ldadd=0, n=8, C=64, gamma=p, alpha=p, saved=p, dgamma=p, dbeta=p, dalpha=p,
                 accumulate=0, act=1, p_drop=0.0, rng=None, call=0, ws=p, stream=None)
    bwd = lambda **o: lib.glass_graphnorm_bwd_f32(*_a(bwd_d, o))
    for o in (dict(dy=None), dict(x=None), dict(dx=None), dict(gamma=None), dict(alpha=None), dict(saved=None), dict(ws=None), dict(n=0), dict(C=0),
              dict(lddy=63), dict(ldx=63), dict(lddx=63), dict(addend=p, ldadd=63), dict(p_drop=0.5), dict(p_drop=1.0, rng=p)):
        assert bwd(**o) == E_ARG, o
    for a in (3, -1, 0x101):
        assert bwd(act=a) == E_ARG, f"glass_graphnorm_bwd_f32 took act {a}"
        assert b"graphnorm_bwd: bad act" in lib.glass_last_error_string()
    fs_d = dict(bwd_d)
    fs_d.pop("ws"), fs_d.pop("stream")
    order = ["dy", "lddy", "x", "ldx", "dx", "lddx", "addend", "ldadd", "n", "C", "gamma", "alpha", "saved", "partial", "nblk", "dgamma", "dbeta",
             "dalpha", "accumulate", "act", "p_drop", "rng", "call", "ws", "stream"]
    fs_d.update(partial=p, nblk=-4, ws=p, stream=None)
    fs = lambda **o: lib.glass_graphnorm_bwd_from_stats_f32(*[dict(fs_d, **o)[k] for k in order])
    for o in (dict(dy=None), dict(partial=None), dict(ws=None), dict(nblk=0), dict(nblk=1 << 31), dict(lddx=63), dict(addend=p, ldadd=63),
              dict(p_drop=0.5), dict(nblk=3, p_drop=0.5)):
        assert fs(**o) == E_ARG, o
    for o in (dict(act=3), dict(act=-1), dict(act=3, nblk=3)):
        assert fs(**o) == E_ARG, f"glass_graphnorm_bwd_from_stats_f32 took {o}"
        assert b"graphnorm_bwd_from_stats: bad act" in lib.glass_last_error_string()
    # the exact form's refusals: C = 48, 3 and 18 replicas, any misaligned operand or stride
    for o in (dict(C=48, lddy=48, ldx=48, lddx=48), dict(nblk=-3), dict(nblk=-18), dict(nblk=-17), dict(dy=p + 4), dict(x=p + 4), dict(dx=p + 4),
              dict(partial=p + 8), dict(addend=p + 4, ldadd=64), dict(addend=p, ldadd=65), dict(lddy=65), dict(ldx=66), dict(lddx=67),
              dict(C=256, lddy=256, ldx=256, lddx=256)):
        assert fs(**o) == E_ARG, o
    assert lib.glass_dropout_scales_f32(None, 0, 0.5, 4, 4, p, None) == E_ARG and lib.glass_dropout_scales_f32(p, 0, 0.0, 4, 4, p, None) == E_ARG
    assert lib.glass_graphnorm_ws_bytes(100, 64) == G.MAX_STAT_BLOCKS * 2 * 64 * 8 + 4 * 64 * 4
    assert lib.glass_gn_exact_words(64) == G.acc_words(64)


def _a(defaults, over):
    assert set(over) <= set(defaults), over
    return list(dict(defaults, **over).values())
