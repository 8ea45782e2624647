"""Attention neighbour aggregation without a GPU: the restatement tests/aggr_gat_oracle.py against fp64 autograd through a plain
scatter formulation, its limits (zero vectors: the weighted mean; slope 1: no dependence on att_dst) and its rule at u = 0, the
argument codes of the new exports (validation runs before any HIP call), the driver flags and the layer's two parameters."""
import ctypes

import numpy as np
import pytest
import torch

import aggr_gat_oracle as GO
from aggr_max_oracle import MaxAdj, rows_of


def _graph(seed, n, nnz):
    """the generator of tests/test_aggr_softmax_host.py: rows n-2 and n-1 stay empty, weights in [0.25, 2)"""
    g = torch.Generator().manual_seed(seed)
    ei = torch.stack((torch.randint(0, n - 2, (nnz, ), generator=g), torch.randint(0, n, (nnz, ), generator=g)))
    ew = torch.rand(nnz, generator=g, dtype=torch.float64) * 1.75 + 0.25
    return ei, ew


def _closed_forms(adj, X, dY, att_src, att_dst, slope):
    Y, L, a, b = GO.gat_aggregate(adj.rowptr, adj.col, adj.val, X, att_src, att_dst, slope)
    return Y, L, GO.gat_aggregate_bwd(adj.rowptr, adj.col, adj.val, dY, X, Y, L, a, b, att_src, att_dst, slope)


def _within(got, want, mass, tol=1e-12):
    return bool(((got - want).abs() <= tol * mass).all())


@pytest.mark.parametrize("zero_vectors", (False, True))
@pytest.mark.parametrize("slope", (0.2, 0.0, 1.0))
def test_restatement_equals_fp64_autograd_through_the_scatter_formulation(slope, zero_vectors):
    """zero_vectors: every u_e is exactly 0 there, so f_e = slope for every entry — the closed forms agree with autograd only
    under torch's rule that u == 0 takes the negative side."""
    n, nnz, H = 40, 300, 7
    ei, ew = _graph(0, n, nnz)
    g = torch.Generator().manual_seed(1)
    X = torch.randn(n, H, generator=g, dtype=torch.float64, requires_grad=True)
    dY = torch.randn(n, H, generator=g, dtype=torch.float64)
    scale = 0.0 if zero_vectors else 1.0
    att_src = ((torch.rand(H, generator=g, dtype=torch.float64) - 0.5) * scale).requires_grad_(True)
    att_dst = ((torch.rand(H, generator=g, dtype=torch.float64) - 0.5) * scale).requires_grad_(True)
    want = GO.scatter_gat_aggregate(ei, ew, n, X, att_src, att_dst, slope)
    dX_want, ds_want, dd_want = torch.autograd.grad(want, (X, att_src, att_dst), dY)
    adj = MaxAdj(ei, ew, n)
    Xd, As, Ad = X.detach(), att_src.detach(), att_dst.detach()
    Y, L, r = _closed_forms(adj, Xd, dY, As, Ad, slope)
    assert float((Y - want.detach()).abs().max()) <= 1e-12 * float(want.detach().abs().max())
    assert float((r.dX - dX_want).abs().max()) <= 1e-12 * float(dX_want.abs().max())
    assert _within(r.datt_src, ds_want, r.mass_datt_src) and _within(r.datt_dst, dd_want, r.mass_datt_dst)
    if not zero_vectors:
        assert float(ds_want.abs().max()) > 1e-3 and (slope == 1.0 or float(dd_want.abs().max()) > 1e-3)
    # da and db against autograd through the scores as free inputs
    a0 = (Xd @ As).requires_grad_(True)
    b0 = (Xd @ Ad).requires_grad_(True)
    rows = ei[0]
    import torch.nn.functional as F
    s = F.leaky_relu(a0[ei[1]] + b0[rows], slope)
    w = ew * torch.exp(s - L[rows])   # (L is the log-sum-exp: these are the normalised weights at the forward's point)
    Z = torch.zeros(n, dtype=torch.float64).index_add(0, rows, w)
    live = torch.bincount(rows, minlength=n) > 0
    Yab = torch.zeros(n, H, dtype=torch.float64).index_add(0, rows, w[:, None] * Xd[ei[1]]) / torch.where(live, Z, torch.ones(()))[:, None]
    da_want, db_want = torch.autograd.grad(Yab, (a0, b0), dY)
    assert _within(r.da, da_want, r.mass_da) and _within(r.db, db_want, r.mass_db)
    if zero_vectors:
        u = (Xd @ As)[adj.col] + (Xd @ Ad)[rows_of(adj.rowptr)]
        assert bool((u == 0).all())
        if slope == 0.0:
            assert bool((r.g == 0).all()) and bool((ds_want == 0).all()), "u == 0 takes the slope: no gradient at slope 0"
        else:
            assert float(r.g.abs().max()) > 0
    # p sums to one over every row with entries
    psum = torch.zeros(n, dtype=torch.float64).index_add_(0, rows_of(adj.rowptr), r.p)
    alive = adj.rowptr[1:] > adj.rowptr[:-1]
    assert int((~alive).sum()) >= 2 and float((psum[alive] - 1).abs().max()) <= 1e-12 and bool((r.p > 0).all())
    assert bool((Y[~alive] == 0).all()) and bool((L[~alive] == 0).all())
    # the GatAdj wrapper (what the model oracle uses) is the same operator
    assert torch.equal((GO.GatAdj(ei, ew, n, att_src, att_dst, slope) @ X).detach(), want.detach())


def test_zero_vectors_give_the_weighted_mean():
    n, nnz, H = 30, 200, 5
    ei, ew = _graph(3, n, nnz)
    X = torch.randn(n, H, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    adj = MaxAdj(ei, ew, n)
    rows = rows_of(adj.rowptr)
    z = torch.zeros(H, dtype=torch.float64)
    Y0, L0, a, b = GO.gat_aggregate(adj.rowptr, adj.col, adj.val, X, z, z, 0.2)
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, rows, adj.val)
    mean = torch.zeros(n, H, dtype=torch.float64).index_add_(0, rows, adj.val[:, None] * X[adj.col])
    live = deg > 0
    assert bool((a == 0).all()) and bool((b == 0).all())
    assert float((Y0[live] - mean[live] / deg[live, None]).abs().max()) <= 1e-13
    assert float((L0[live] - torch.log(deg[live])).abs().max()) <= 1e-13   # M = 0, Z = the weighted degree


def test_slope_one_makes_the_destination_term_cancel():
    """At slope 1 the score is a_j + b_i: b_i is common to a row's entries and cancels in its softmax, so Y does not depend on
    att_dst and db is zero up to rounding (1e-12 of its mass)."""
    n, nnz, H = 40, 300, 7
    ei, ew = _graph(0, n, nnz)
    g = torch.Generator().manual_seed(2)
    X = torch.randn(n, H, generator=g, dtype=torch.float64)
    dY = torch.randn(n, H, generator=g, dtype=torch.float64)
    As, Ad, Ad2 = (torch.rand(H, generator=g, dtype=torch.float64) - 0.5 for _ in range(3))
    adj = MaxAdj(ei, ew, n)
    Y, L, r = _closed_forms(adj, X, dY, As, Ad, 1.0)
    Y2, _L2, _r2 = _closed_forms(adj, X, dY, As, Ad2, 1.0)
    assert float((Y - Y2).abs().max()) <= 1e-13 * float(Y.abs().max())
    assert _within(r.db, torch.zeros(n, dtype=torch.float64), r.mass_db) and float(r.mass_db.max()) > 0
    Y3, _L3, r3 = _closed_forms(adj, X, dY, As, Ad, 0.2)
    assert float((Y - Y3).abs().max()) > 1e-3 and float(r3.db.abs().max()) > 1e-3   # (another slope: it does depend on it)


def _plan(rowptr):
    from glass_amd import _lib
    lib = _lib.load()
    rp = np.asarray(rowptr, dtype=np.int32)
    words = ctypes.c_int64(0)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, rp.shape[0] - 1, None, ctypes.byref(words)) == 0
    plan = np.zeros(words.value, dtype=np.int32)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, rp.shape[0] - 1, plan.ctypes.data, ctypes.byref(words)) == 0
    return plan


def test_new_exports_answer_with_argument_codes_before_any_launch():
    from glass_amd import _lib
    lib = _lib.load()
    E_ARG, E_PLAN, E_UNSUPPORTED = -1, -2, -3
    plan = _plan([0, 1, 2])
    cut = _plan([0, 700, 700, 701])   # a row cut into chunks: partial slots
    x = np.zeros(64, dtype=np.float64)   # (8-byte aligned: it stands in for every pointer, the datt workspace included)
    p, h = x.ctypes.data, plan.ctypes.data
    slots = int(cut[7])
    assert slots >= 2
    assert lib.glass_spmm_gat_ws_bytes(cut.ctypes.data, 12) == slots * (12 + 2) * 4
    assert lib.glass_spmm_gat_edge_ws_bytes(cut.ctypes.data, 12) == slots * 4
    assert lib.glass_spmm_gat_bwd_ws_bytes(cut.ctypes.data, 12) == slots * (12 + 1) * 4
    assert lib.glass_spmm_gat_da_ws_bytes(cut.ctypes.data, 12) == slots * 4
    assert lib.glass_gat_datt_ws_bytes(1000, 64) == 4 * 2 * 64 * 8 and lib.glass_gat_datt_ws_bytes(1000, 260) == 2 * 2 * 260 * 8
    assert lib.glass_gat_datt_ws_bytes(0, 64) == 0 and lib.glass_gat_datt_ws_bytes(5, 0) == E_ARG
    assert lib.glass_gat_datt_ws_bytes(-1, 8) == E_ARG
    for q in (lib.glass_spmm_gat_ws_bytes, lib.glass_spmm_gat_edge_ws_bytes, lib.glass_spmm_gat_bwd_ws_bytes,
              lib.glass_spmm_gat_da_ws_bytes):
        assert q(h, 64) == 0 and q(p, 64) == E_PLAN and q(None, 64) == E_PLAN and q(h, 0) == E_ARG and q(h, -4) == E_ARG
    call = lambda fn, spec: (lambda **k: fn(*[k.get(n, d) for n, d in spec]))
    fwd = call(lib.glass_spmm_gat_csr_f32, (
        ("rowptr", h), ("col", h), ("val", p), ("X", p), ("ldx", 8), ("a", p), ("b", p), ("slope", 0.2), ("Y", p), ("ldy", 8),
        ("L", p), ("n_rows", 2), ("H", 8), ("hdr", h), ("plan", h), ("ws", None), ("stream", None)))
    edge = call(lib.glass_spmm_gat_edge_f32, (
        ("rowptr", h), ("col", h), ("val", p), ("X", p), ("ldx", 8), ("a", p), ("b", p), ("slope", 0.2), ("dY", p), ("lddy", 8),
        ("Y", p), ("ldy", 8), ("L", p), ("g", p), ("db", p), ("n_rows", 2), ("H", 8), ("hdr", h), ("plan", h), ("ws", None),
        ("stream", None)))
    bwd = call(lib.glass_spmm_gat_bwd_f32, (
        ("rowptr", h), ("col", h), ("val", p), ("eid", h), ("a", p), ("b", p), ("slope", 0.2), ("dY", p), ("lddy", 8), ("L", p),
        ("g", p), ("db", p), ("att_src", p), ("att_dst", p), ("dX", p), ("lddx", 8), ("da", p), ("n_rows", 2), ("H", 8),
        ("hdr", h), ("plan", h), ("ws", None), ("stream", None)))
    da = call(lib.glass_spmm_gat_da_f32, (
        ("rowptr", h), ("col", h), ("val", p), ("eid", h), ("g", p), ("da", p), ("n_rows", 2), ("H", 8), ("vec", 1), ("hdr", h),
        ("plan", h), ("ws", None), ("stream", None)))
    big = 65535 * 64 + 1
    for fn, ptrs, lds, odd in (
            (fwd, ("rowptr", "X", "a", "b", "Y", "L", "hdr", "plan", "col", "val"), ("ldx", "ldy"), "X"),
            (edge, ("rowptr", "X", "a", "b", "dY", "Y", "L", "g", "db", "hdr", "plan", "col", "val"), ("ldx", "lddy", "ldy"), "X"),
            (bwd, ("rowptr", "a", "b", "dY", "L", "g", "db", "att_src", "att_dst", "dX", "da", "hdr", "plan", "col", "val", "eid"),
             ("lddy", "lddx"), "dY"),
            (da, ("rowptr", "g", "da", "hdr", "plan", "col", "val", "eid"), (), "g")):
        for name in ptrs:
            assert fn(**{name: None}) == E_ARG, name
        for name in lds:
            assert fn(**{name: 7}) == E_ARG, name
        assert fn(H=0) == E_ARG
        assert fn(n_rows=3) == E_PLAN and b"plan does not match" in lib.glass_last_error_string()
        assert fn(hdr=p) == E_PLAN
        assert fn(**{odd: p + 2}) == E_ARG and b"aligned" in lib.glass_last_error_string()
        assert fn(H=big, **{name: big for name in lds}, **({"vec": 0} if fn is da else {})) == E_UNSUPPORTED
        # a plan with partial slots and no workspace
        assert fn(hdr=cut.ctypes.data, plan=cut.ctypes.data, n_rows=3) == E_ARG and b"ws is null" in lib.glass_last_error_string()
        if fn is not da:
            assert fn(slope=float("nan")) == E_ARG and b"slope" in lib.glass_last_error_string()
    assert da(H=6, vec=1) == E_ARG   # the 16-byte form needs H % 4 == 0
    scores = call(lib.glass_gat_scores_f32, (("X", p), ("ldx", 8), ("att_src", p), ("att_dst", p), ("a", p), ("b", p), ("n_rows", 2),
                                             ("H", 8), ("stream", None)))
    datt = call(lib.glass_gat_datt_f32, (("X", p), ("ldx", 8), ("da", p), ("db", p), ("datt_src", p), ("datt_dst", p), ("n_rows", 2),
                                         ("H", 8), ("ws", p), ("stream", None)))
    for fn, ptrs in ((scores, ("X", "att_src", "att_dst", "a", "b")), (datt, ("X", "da", "db", "datt_src", "datt_dst", "ws"))):
        for name in ptrs:
            assert fn(**{name: None}) == E_ARG, name
        assert fn(ldx=7) == E_ARG and fn(H=0) == E_ARG and fn(n_rows=-1) == E_ARG
        assert fn(X=p + 2) == E_ARG and b"aligned" in lib.glass_last_error_string()
        assert fn(H=big, ldx=big) == E_UNSUPPORTED
        assert fn(n_rows=0) == 0   # nothing to launch
    assert datt(ws=p + 4) == E_ARG and b"8-byte" in lib.glass_last_error_string()


def test_names_are_accepted_where_the_aggregation_is_chosen():
    import GLASSTest
    args = GLASSTest.parse_args(["--use_one", "--aggr", "gat", "--gat_slope", "0.1"])
    assert args.aggr == "gat" and args.gat_slope == 0.1
    assert GLASSTest.parse_args(["--use_one"]).gat_slope == 0.2
    with pytest.raises(SystemExit):
        GLASSTest.parse_args(["--use_one", "--aggr", "gat", "--gat_slope", "steep"])
    from glass_amd import graph, models, ops, _lib
    ei, ew = torch.tensor([[0, 1], [1, 0]]), torch.ones(2)
    with pytest.raises(_lib.GlassHipError, match="GPU only"):
        graph.CSRAdj(ei, ew, 2, "gat")
    with pytest.raises(_lib.GlassHipError, match="GPU only"):
        models.buildAdj(ei, ew, 2, "gat")

    class _Adj:   # the dispatch reads the name only
        aggr = "gat"
    with pytest.raises(_lib.GlassHipError, match="spmm_gat"):
        ops.spmm(_Adj(), torch.zeros(2, 4))
    with pytest.raises(_lib.GlassHipError, match="replicated gat aggregation is not built"):
        ops.spmm_rep(_Adj(), torch.zeros(4, 4), 2)
    _Adj.aggr = "softmax"
    with pytest.raises(_lib.GlassHipError, match="not 'gat'"):
        ops.spmm_gat(_Adj(), torch.zeros(2, 4), torch.zeros(4), torch.zeros(4), 0.2)
    for what in ("gat_scores", "gat_fwd", "gat_edge", "gat_bwd", "gat_da", "gat_datt"):
        with pytest.raises(_lib.GlassHipError, match="not 'gat'"):
            graph.CSRAdj._need(_Adj(), what, "gat")


def test_the_attention_vectors_are_parameters_of_gat_layers_only():
    from glass_amd import models
    for aggr in ("mean", "sum", "gcn", "max", "softmax"):
        conv = models.GLASSConv(8, 8, aggr=aggr)
        assert not any(k.startswith("att_") for k in conv.state_dict()) and not hasattr(conv, "att_src"), aggr
    base = set(models.GLASSConv(8, 12, aggr="sum").state_dict())
    conv = models.GLASSConv(8, 12, aggr="gat")
    assert set(conv.state_dict()) - base == {"att_src", "att_dst"} and base <= set(conv.state_dict())
    assert conv.gat_slope == 0.2 and models.GLASSConv(8, 12, aggr="gat", gat_slope=0.05).gat_slope == 0.05
    bound = (6.0 / (1 + 12)) ** 0.5   # xavier_uniform_ on the [1, H] view
    for v in (conv.att_src, conv.att_dst):
        assert v.shape == (12, ) and v.dtype == torch.float32 and v.requires_grad
        assert 0 < float(v.detach().abs().max()) <= bound
    before = conv.att_src.detach().clone()
    ptr = conv.att_src.data_ptr()
    conv.reset_parameters()
    assert conv.att_src.data_ptr() == ptr and not torch.equal(conv.att_src.detach(), before)
    assert float(conv.att_src.detach().abs().max()) <= bound
    from helpers import build_glass
    keys = set(build_glass(64, 2, 5, 3, "gat", "mean", 0.8).state_dict()) - set(build_glass(64, 2, 5, 3, "mean", "mean", 0.8).state_dict())
    assert keys == {f"conv.convs.{l}.att_{s}" for l in range(2) for s in ("src", "dst")}
