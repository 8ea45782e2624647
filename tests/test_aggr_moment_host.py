"""Standard-deviation / variance neighbour aggregation without a GPU: the restatement tests/aggr_moment_oracle.py against fp64
autograd through a dense formulation; the merge the kernel uses (Chan's update, in fp32, in two orders) inside the variance
bound the GPU tests grade with, and the plain E[x^2] - Mu^2 form outside it as soon as the messages have an offset; the argument
codes of the new exports (validation runs before any HIP call); the names where the aggregation is chosen."""
import numpy as np
import pytest
import torch

import aggr_moment_oracle as MO
from aggr_max_oracle import MaxAdj

OFFSETS = (0, 1, 30, 1000, 30000)


def _graph(seed, n, nnz):
    g = torch.Generator().manual_seed(seed)
    ei = torch.stack((torch.randint(0, n - 2, (nnz, ), generator=g), torch.randint(0, n, (nnz, ), generator=g)))  # rows n-2, n-1: empty
    ei = torch.cat((ei, torch.tensor([[3, 3, 5], [7, 7, 5]])), dim=1)   # a duplicate pair, a self-loop
    ew = torch.rand(nnz + 3, generator=g, dtype=torch.float64) * 1.75 + 0.25
    return ei, ew


@pytest.mark.parametrize("with_mu", (False, True))
@pytest.mark.parametrize("kind", ("std", "var"))
def test_restatement_equals_fp64_autograd_on_the_dense_formulation(kind, with_mu):
    n, nnz, H, eps = 40, 300, 7, 1e-5
    ei, ew = _graph(0, n, nnz)
    g = torch.Generator().manual_seed(1)
    X = torch.randn(n, H, generator=g, dtype=torch.float64, requires_grad=True)
    dS = torch.randn(n, H, generator=g, dtype=torch.float64)
    dMu = torch.randn(n, H, generator=g, dtype=torch.float64)
    S_want, Mu_want = MO.dense_moments(ei, ew, n, X, kind, eps)
    outs, grads = ((S_want, Mu_want), (dS, dMu)) if with_mu else ((S_want, ), (dS, ))
    (dX_want, ) = torch.autograd.grad(outs, (X, ), grads)
    adj = MaxAdj(ei, ew, n)
    Xn = X.detach().numpy()
    m = MO.moments(adj.rowptr.numpy(), adj.col.numpy(), adj.val.numpy(), Xn, eps)
    S = m["Std"] if kind == "std" else m["Var"]
    A, C = MO.factors(kind, S, m["W"], dS.numpy(), dMu.numpy() if with_mu else None)
    assert (C is None) != with_mu
    dX, mass = MO.moments_bwd(adj.rowptr_t.numpy(), adj.col_t.numpy(), adj.val_t.numpy(), Xn, m["Mu"], A, C)
    for got, want in ((S, S_want), (m["Mu"], Mu_want), (dX, dX_want)):
        want = want.detach().numpy()
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all()   # per element
    assert (np.abs(dX) <= mass * (1 + 1e-12)).all() and mass.min() >= 0
    # a row without entries: zeros, and no gradient through it; the scatter form (the model oracle's) is the same operator
    assert not S[-2:].any() and not m["Mu"][-2:].any() and not m["W"][-2:].any() and not A[-2:].any()
    S2, Mu2 = MO.scatter_moments(ei, ew, n, X, kind, eps)
    assert float((S2 - S_want).detach().abs().max()) <= 1e-13 and float((Mu2 - Mu_want).detach().abs().max()) <= 1e-13
    assert torch.equal((MO.MomentAdj(ei, ew, n, kind, eps) @ X).detach(), S2.detach())


def test_single_entry_and_equal_messages():
    # row 0: two equal messages (sources 1 and 2, channel 1); row 1: none; row 2: one entry
    ei = torch.tensor([[0, 0, 2], [1, 2, 0]])
    ew = torch.tensor([1.0, 3.0, 0.5], dtype=torch.float64)
    X = np.array([[1.0, -2.0], [0.0, 4.0], [2.0, 4.0]])
    adj = MaxAdj(ei, ew, 3)
    m = MO.moments(adj.rowptr.numpy(), adj.col.numpy(), adj.val.numpy(), X, 1e-5)
    assert m["Var"][0, 1] == 0 and m["Std"][0, 1] == np.sqrt(1e-5) and m["Mu"][0, 1] == 4.0
    assert abs(m["Var"][0, 0] - 0.75) <= 1e-15 and abs(m["Mu"][0, 0] - 1.5) <= 1e-15     # weights 1 and 3 on 0 and 2
    assert not m["Var"][1].any() and not m["Std"][1].any() and m["W"][1] == 0
    assert not m["Var"][2].any() and (m["Std"][2] == np.sqrt(1e-5)).all() and (m["Mu"][2] == X[0]).all()
    A, C = MO.factors("std", m["Std"], m["W"], np.ones((3, 2)))
    dX, _ = MO.moments_bwd(adj.rowptr_t.numpy(), adj.col_t.numpy(), adj.val_t.numpy(), X, m["Mu"], A, C)
    assert np.abs(dX.sum(0)).max() <= 1e-12 and not dX[0].any()   # a shift of X moves no spread; one entry: zero gradient


def _rows_of_messages(rng, n, T, offset):
    """T rows of n entries: mixed magnitudes, positive weights; every fifth row holds equal messages"""
    x = (rng.standard_normal((n, T)) * rng.choice([1e-3, 1.0, 50.0], (1, T)) + offset).astype(np.float32)
    x[:, ::5] = x[0, ::5]
    w = (rng.random((n, T)) * 2 + 0.01).astype(np.float32)
    return w, x


@pytest.mark.parametrize("offset", OFFSETS)
def test_chan_merge_keeps_the_variance_bound_and_the_plain_form_does_not(offset):
    """Both merge orders of the kernel's update, in fp32, against fp64 on the same fp32 data: inside the bound at every offset
    (and exactly 0 on equal messages).  The plain form keeps it only without an offset: the bound tells the two apart."""
    rng = np.random.default_rng(offset)
    worst = {"sequential": 0.0, "pairwise": 0.0, "plain": 0.0, "mu": 0.0}
    for n in (1, 2, 3, 5, 64, 65, 300, 2000):
        T = 20
        w, x = _rows_of_messages(rng, n, T, offset)
        w64, x64 = w.astype(np.float64), x.astype(np.float64)
        W = w64.sum(0)
        mu = (w64 * x64).sum(0) / W
        var = (w64 * (x64 - mu) ** 2).sum(0) / W
        sq, ab = (w64 * x64 * x64).sum(0) / W, (w64 * np.abs(x64)).sum(0) / W
        bound = MO.gamma(8 * n + 8) * (var + np.sqrt(var * sq))
        bmu = MO.gamma(3 * n + 4) * ab
        equal = np.arange(T) % 5 == 0
        for name, fn in (("sequential", MO.chan_sequential), ("pairwise", MO.chan_pairwise)):
            Wt, m, Q = fn(w, x)
            v = (Q / Wt).astype(np.float32).astype(np.float64)
            assert (v[equal] == 0).all() and (m[equal] == x[0, equal]).all(), (name, n, "equal messages")
            err = np.abs(v - var)
            assert (err <= bound).all(), (name, offset, n, float((err / np.maximum(bound, 1e-300)).max()))
            assert (np.abs(m.astype(np.float64) - mu) <= bmu).all(), (name, offset, n, "Mu")
            live = bound > 0
            if live.any():
                worst[name] = max(worst[name], float((err[live] / bound[live]).max()))
            worst["mu"] = max(worst["mu"], float((np.abs(m.astype(np.float64) - mu) / bmu).max()))
        if n > 1:
            live = ~equal & (bound > 0)   # (at a large offset a row of small messages can be equal once rounded to fp32)
            err = np.abs(MO.plain_variance(w, x).astype(np.float64) - var)
            worst["plain"] = max(worst["plain"], float((err[live] / bound[live]).max()))
    print(f"offset {offset}: largest share of the Var bound — sequential {worst['sequential']:.3g}, pairwise {worst['pairwise']:.3g}, "
          f"plain E[x^2] - Mu^2 {worst['plain']:.3g}; of the Mu bound {worst['mu']:.3g}")
    assert worst["sequential"] <= 1 and worst["pairwise"] <= 1
    if offset >= 1:
        assert worst["plain"] > 1, "the plain form must break the bound on data with an offset"


def _plan(rowptr):
    import ctypes
    from glass_amd import _lib
    lib = _lib.load()
    rp = np.asarray(rowptr, dtype=np.int32)
    words = ctypes.c_int64(0)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, rp.shape[0] - 1, None, ctypes.byref(words)) == 0
    plan = np.zeros(words.value, dtype=np.int32)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, rp.shape[0] - 1, plan.ctypes.data, ctypes.byref(words)) == 0
    return plan


def test_new_exports_answer_with_argument_codes_before_any_launch():
    import ctypes as c
    from glass_amd import _lib
    lib = _lib.load()
    P, I = c.c_void_p, c.c_int64
    assert _lib.SIGNATURES["glass_spmm_moment_ws_bytes"] == (c.c_int64, [P, I])
    assert _lib.SIGNATURES["glass_spmm_moment_bwd_ws_bytes"] == (c.c_int64, [P, I])
    assert _lib.SIGNATURES["glass_spmm_moment_csr_f32"] == (c.c_int, [P, P, P, P, I, c.c_float, c.c_int, P, I, P, I, P, I, I, P, P, P, P])
    assert _lib.SIGNATURES["glass_spmm_moment_bwd_f32"] == (c.c_int, [P, P, P, P, I, P, I, P, I, P, I, P, I, I, I, P, P, P, P])
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glass_hip.h")).read()
    for name in ("glass_spmm_moment_ws_bytes", "glass_spmm_moment_csr_f32", "glass_spmm_moment_bwd_ws_bytes",
                 "glass_spmm_moment_bwd_f32"):
        assert hasattr(lib, name) and (name + "(") in header, name
    E_ARG, E_PLAN, E_UNSUPPORTED = -1, -2, -3
    plan = _plan([0, 1, 2])
    cut = _plan([0, 700, 700, 701])   # a row cut into chunks: partial slots
    x = np.zeros(64, dtype=np.float64)   # (stands in for every pointer)
    p, h = x.ctypes.data, plan.ctypes.data
    assert int(cut[7]) >= 2
    assert lib.glass_spmm_moment_ws_bytes(cut.ctypes.data, 12) == int(cut[7]) * (2 * 12 + 1) * 4
    assert lib.glass_spmm_moment_bwd_ws_bytes(cut.ctypes.data, 12) == int(cut[7]) * 12 * 4
    assert lib.glass_spmm_moment_ws_bytes(h, 64) == 0 and lib.glass_spmm_moment_bwd_ws_bytes(h, 64) == 0
    for q in (lib.glass_spmm_moment_ws_bytes, lib.glass_spmm_moment_bwd_ws_bytes):
        assert q(p, 64) == E_PLAN and q(None, 64) == E_PLAN and q(h, 0) == E_ARG and q(h, -4) == E_ARG
    fwd = lambda **k: lib.glass_spmm_moment_csr_f32(*[k.get(n, d) for n, d in (
        ("rowptr", h), ("col", h), ("val", p), ("X", p), ("ldx", 8), ("eps", 1e-5), ("kind", 0), ("S", p), ("lds", 8), ("Mu", p),
        ("ldmu", 8), ("Wsum", p), ("n_rows", 2), ("H", 8), ("hdr", h), ("plan", h), ("ws", None), ("stream", None))])
    bwd = lambda **k: lib.glass_spmm_moment_bwd_f32(*[k.get(n, d) for n, d in (
        ("rowptr", h), ("col", h), ("val", p), ("X", p), ("ldx", 8), ("Mu", p), ("ldmu", 8), ("A", p), ("lda", 8), ("C", p),
        ("ldc", 8), ("dX", p), ("lddx", 8), ("n_rows", 2), ("H", 8), ("hdr", h), ("plan", h), ("ws", None), ("stream", None))])
    for call, ptrs, lds in ((fwd, ("rowptr", "X", "S", "Mu", "Wsum", "hdr", "plan", "col", "val"), ("ldx", "lds", "ldmu")),
                            (bwd, ("rowptr", "X", "Mu", "A", "dX", "hdr", "plan", "col", "val"), ("ldx", "ldmu", "lda", "ldc", "lddx"))):
        for name in ptrs:
            assert call(**{name: None}) == E_ARG, name
        for name in lds:
            assert call(**{name: 7}) == E_ARG, name
        assert call(H=0) == E_ARG
        assert call(n_rows=3) == E_PLAN and b"plan does not match" in lib.glass_last_error_string()
        assert call(hdr=p) == E_PLAN
        assert call(X=p + 2) == E_ARG and b"aligned" in lib.glass_last_error_string()
        big = 65535 * 64 + 1
        assert call(H=big, **{name: big for name in lds}) == E_UNSUPPORTED
        # a plan with partial slots and no workspace
        assert call(hdr=cut.ctypes.data, plan=cut.ctypes.data, n_rows=3) == E_ARG and b"ws is null" in lib.glass_last_error_string()
    assert fwd(kind=2) == E_ARG and fwd(kind=-1) == E_ARG and fwd(eps=-1.0) == E_ARG
    assert bwd(C=p + 2) == E_ARG     # (a null C is a call without the mean's gradient, not an error: it reaches the plan check)
    assert bwd(C=None, ldc=0, n_rows=3) == E_PLAN


def test_names_are_accepted_where_the_aggregation_is_chosen():
    import GLASSTest
    for name in ("std", "var"):
        assert GLASSTest.parse_args(["--use_one", "--aggr", name]).aggr == name
    with pytest.raises(SystemExit):
        GLASSTest.parse_args(["--use_one", "--aggr", "min"])
    from glass_amd import graph, models, ops, _lib
    ei, ew = torch.tensor([[0, 1], [1, 0]]), torch.ones(2)
    for name in ("min", "softmin", "median"):   # still refused, as the reference refuses them
        with pytest.raises(NotImplementedError):
            graph.CSRAdj(ei, ew, 2, name)
        with pytest.raises(NotImplementedError):
            models.buildAdj(ei, ew, 2, name)
    for name in ("std", "var"):                 # known names: the host side refuses a CPU graph loudly
        with pytest.raises(_lib.GlassHipError, match="GPU only"):
            graph.CSRAdj(ei, ew, 2, name)
        with pytest.raises(_lib.GlassHipError, match="GPU only"):
            models.buildAdj(ei, ew, 2, name)

    class _Adj:   # the dispatch reads the name only
        aggr = "std"
    with pytest.raises(_lib.GlassHipError, match="spmm_moments"):
        ops.spmm(_Adj(), torch.zeros(2, 4))
    with pytest.raises(_lib.GlassHipError, match="replicated std aggregation is not built"):
        ops.spmm_rep(_Adj(), torch.zeros(4, 4), 2)
    with pytest.raises(_lib.GlassHipError, match="no edge-weight gradient"):
        ops.spmm_w(_Adj(), torch.zeros(2, 4), torch.ones(2))
    with pytest.raises(ValueError, match="kind"):
        ops.spmm_moments(_Adj(), torch.zeros(2, 4), kind="range")
    for other in ("mean", "softmax", "gat", "max"):
        _Adj.aggr = other
        with pytest.raises(_lib.GlassHipError, match="not 'std' or 'var'"):
            ops.spmm_moments(_Adj(), torch.zeros(2, 4))


def test_the_layer_owns_no_parameter_and_refuses_what_max_refuses():
    from glass_amd import models, stack
    from helpers import build_glass
    mean_keys = list(models.GLASSConv(8, 8, aggr="mean").state_dict())
    for aggr in ("std", "var"):
        conv = models.GLASSConv(8, 8, aggr=aggr)
        assert list(conv.state_dict()) == mean_keys and conv.moment_eps == 1e-5 and conv.aggr == aggr
        assert models.GLASSConv(8, 8, aggr=aggr, moment_eps=1e-3).moment_eps == 1e-3
        with pytest.raises(ValueError, match="live_edge_weight"):
            models.GLASSConv(8, 8, aggr=aggr, live_edge_weight=True)
        with pytest.raises(ValueError, match="no replicated form"):
            conv(torch.zeros(4, 8), torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0), torch.zeros(4, dtype=torch.uint8),
                 batch=object())
        model = build_glass(64, 2, 5, 3, aggr, "mean", 0.8)
        assert list(model.state_dict()) == list(build_glass(64, 2, 5, 3, "mean", "mean", 0.8).state_dict())
        assert all(c.aggr == aggr for c in model.conv.convs) and not stack.StackProgram.supported(model.conv)
        with pytest.raises(ValueError, match="live_edge_weight"):
            build_glass(64, 2, 5, 3, aggr, "mean", 0.8, live_edge_weight=True)


def test_weights_are_multiplicities():
    """zero, negative and NaN weights are refused when the adjacency is built, before the device is looked at"""
    from glass_amd import graph, models
    ei = torch.tensor([[0, 1, 1], [1, 0, 1]])
    for aggr in ("std", "var"):
        for bad in (0.0, -1.0, float("nan")):
            ew = torch.tensor([1.0, bad, 2.0])
            with pytest.raises(ValueError, match="strictly positive"):
                graph.CSRAdj(ei, ew, 2, aggr)
            with pytest.raises(ValueError, match="strictly positive"):
                models.buildAdj(ei, ew, 2, aggr)
