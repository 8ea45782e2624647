"""Host side of the step-tail tests (no GPU): tests/step_tail_oracle.py against torch fp64 autograd, its index vectors against
the library's host-side K1 plan builder, its arena layouts, and the conditioning of the Adam states that
tests/test_gpu_step_tail.py compares within 2 ulp."""
import numpy as np
import pytest
import torch

import gradclip_oracle as GO
import step_tail_oracle as TO
from helpers import rel_inf

VECTORS = sorted(TO.PLAN_KIND)


def _lib():
    from glass_amd import _lib
    return _lib.load()


_model = TO.model_inputs


@pytest.mark.parametrize("name", VECTORS)
def test_index_vectors_give_the_plans_they_are_named_for(name):
    x, V = TO.index_vector(name)
    assert int(x.min()) >= 0 and int(x.max()) < V
    plan = TO.host_plan(_lib(), x, V)
    sweep, cut = TO.PLAN_KIND[name]
    assert (plan[TO.HDR_SWEEP] > 0) == sweep, plan[:16]
    assert (plan[TO.HDR_REDUCE] > 0) == cut and (plan[TO.HDR_SLOTS] > 0) == cut, plan[:16]
    assert plan[TO.HDR_ITEMS] > 0 or (sweep and not cut)  # (v200: short rows only, everything swept)
    rows = TO.reduce_list(plan)
    assert sum(n for _r, _f, n in rows) == plan[TO.HDR_SLOTS] and all(n > 1 for _r, _f, n in rows)
    counts = np.bincount(x.numpy(), minlength=V)
    if name == "long_cut":
        assert list(counts[:5]) == [0, 1, 256, 257, 700] and counts[39] == 0 and len(x) == 3000 and V == 40
        assert [(r, n) for r, _f, n in rows if r < 5] == [(3, 2), (4, 3)]  # 256 entries: one chunk; 257: two; 700: three
        assert plan[TO.HDR_ITEMS] >= V  # an empty row is an (empty) item too
    if name == "long_nocut":
        assert counts.max() == 256 and counts.min() == 0 and len(x) == 1024 and V == 8
    if name == "sweep":
        assert len(x) == 5000 and V == 1024 and [r for r, _f, _n in rows] == [0]
    if name in ("v64c", "v65c"):
        assert V == int(name[1:3]) and [r for r, _f, _n in rows] == [0]


@pytest.mark.parametrize("name,H", [("long_cut", 64), ("long_nocut", 4), ("sweep", 20), ("v1", 16), ("v3", 128), ("v65c", 20)])
def test_table_form_is_the_autograd_gradient(name, H):
    x, V, W, gamma, beta, alpha, gout = _model(name, H)
    ref = TO.autograd_grads(x, W, gamma, beta, alpha, gout)
    got = TO.table_form_grads(x, W, gamma, beta, alpha, gout)
    for k, r, g in zip(("dW", "dgamma", "dbeta", "dalpha"), ref, got):
        assert rel_inf(g, r) < 1e-12, (k, rel_inf(g, r))
    unused = torch.bincount(x, minlength=V) == 0
    assert float(ref[0][unused].abs().max() if unused.any() else 0.0) == 0.0  # an unused row has an exactly zero gradient


def test_autograd_reference_is_the_oracle_module():
    """the reference restated here == oracle.glass_oracle.GraphNorm on an Embedding lookup (what the model runs)"""
    from oracle import glass_oracle as O
    x, V, W, gamma, beta, alpha, gout = _model("long_cut", 16)
    Wd = W.double().requires_grad_(True)
    gn = O.GraphNorm(16).double()
    with torch.no_grad():
        gn.weight.copy_(gamma), gn.bias.copy_(beta), gn.mean_scale.copy_(alpha)
    gn(Wd[x]).backward(gout.double())
    ref = TO.autograd_grads(x, W, gamma, beta, alpha, gout)
    for a, b in zip(ref, (Wd.grad, gn.weight.grad, gn.bias.grad, gn.mean_scale.grad)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["first", "middle", "last", "tight", "stride"])
def test_arena_layouts(name):
    V, H = 40, 64
    lay = TO.arena_layout(name, V, H)
    n = lay[0]
    r = sorted(TO.tail_ranges(lay, V, H).values())
    assert r[0][0] >= 0 and r[-1][1] <= n
    assert all(a[1] <= b[0] for a, b in zip(r, r[1:])), "ranges overlap"
    rng = TO.tail_ranges(lay, V, H)
    if name in ("first", "tight"):
        assert rng["W"][0] == 0 and rng["W"][1] == rng["alpha"][0] and rng["alpha"][1] == rng["gamma"][0] and rng["gamma"][1] == rng["beta"][0]
    if name == "middle":
        assert rng["beta"][1] == rng["alpha"][0] and rng["alpha"][1] == rng["gamma"][0] and rng["gamma"][1] == rng["W"][0] and rng["W"][0] % 2 == 1
    if name == "last":
        assert rng["W"][1] == n and rng["gamma"][0] == 0 and rng["beta"][1] == rng["W"][0]
    if name == "tight":
        assert -(-TO.arena_layout(name, 3, 4)[0] // 256) == 1
    if name == "stride":
        assert n == 2048 * 256 + 4099 and rng["W"][0] < 2048 * 256 < rng["W"][1] and rng["gamma"][1] == n


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("steps_done", [0, 5])
@pytest.mark.parametrize("layout,name,H", [("first", "long_cut", 64), ("middle", "v65c", 20), ("last", "long_nocut", 16),
                                           ("tight", "v3", 4), ("stride", "v200", 16)])
def test_tail_adam_states_are_well_conditioned(layout, name, H, steps_done, wd):
    """On the states the GPU test starts from, the separately rounded update (gradclip_oracle) and the fully contracted one
    stay within the GPU test's 2 ulp per element of each other (1 ulp of a value just below a power of two counts as 2 of the
    value just above it; over the 528 k elements of the `stride` layout that happens) — the bound separates rounding from
    errors: an element updated twice or not at all is hundreds of ulp away."""
    x, V, W, gamma, beta, alpha, gout = _model(name, H)
    grads = dict(zip(("W", "gamma", "beta", "alpha"), TO.autograd_grads(x, W, gamma, beta, alpha, gout)))
    lay = TO.arena_layout(layout, V, H)
    params = {"W": W, "gamma": gamma, "beta": beta, "alpha": alpha}
    st = TO.tail_adam_state(lay, V, H, params, grads, seed=7)
    for k, (lo, hi) in TO.tail_ranges(lay, V, H).items():
        assert torch.equal(st["p"][lo:hi], params[k].reshape(-1)) and bool(st["g"][lo:hi].isnan().all())
        st["g"][lo:hi] = grads[k].reshape(-1).float()
    lr = float(np.float32(1e-2))
    a = GO.clipped_adam_step(st["p"], st["g"], st["m"], st["v"], steps_done + 1, lr, 0.9, 0.999, 1e-8, wd, 1.0)
    b = TO.adam_step_contracted(st["p"], st["g"], st["m"], st["v"], steps_done + 1, lr, 0.9, 0.999, 1e-8, wd)
    worst = {k: TO.ulps(bb, aa) for k, aa, bb in (("p", a[0], b[0]), ("m", a[2], b[1]), ("v", a[3], b[2]))}
    assert max(worst.values()) <= 2.0, worst
    # teeth: the update applied twice, or skipped, is far outside
    twice = GO.clipped_adam_step(a[0], st["g"], a[2], a[3], steps_done + 1, lr, 0.9, 0.999, 1e-8, wd, 1.0)
    assert TO.ulps(twice[0], a[0]) > 100 and TO.ulps(st["p"], a[0]) > 100
