"""Softmax neighbour aggregation without a GPU: the restatement tests/aggr_softmax_oracle.py against fp64 autograd through a
plain scatter formulation, its limits (t = 0: the weighted mean; large t: the row max) and its empty-row rule, the argument
codes of the new exports (validation runs before any HIP call), the driver flag and the layers' temperature parameter."""
import numpy as np
import pytest
import torch

import aggr_softmax_oracle as SO
from aggr_max_oracle import MaxAdj, rows_of


def _graph(seed, n, nnz, unit=False):
    g = torch.Generator().manual_seed(seed)
    ei = torch.stack((torch.randint(0, n - 2, (nnz, ), generator=g), torch.randint(0, n, (nnz, ), generator=g)))  # rows n-2, n-1: empty
    ew = torch.ones(nnz, dtype=torch.float64) if unit else torch.rand(nnz, generator=g, dtype=torch.float64) * 1.75 + 0.25
    return ei, ew


@pytest.mark.parametrize("t", (0.0, 1.0, -0.5, 4.0))
def test_restatement_equals_fp64_autograd_through_the_scatter_formulation(t):
    n, nnz, H = 40, 300, 7
    ei, ew = _graph(0, n, nnz)
    g = torch.Generator().manual_seed(1)
    X = torch.randn(n, H, generator=g, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor([t], dtype=torch.float64, requires_grad=True)
    dY = torch.randn(n, H, generator=g, dtype=torch.float64)
    want = SO.scatter_softmax_aggregate(ei, ew, n, X, tt)
    dX_want, dt_want = torch.autograd.grad(want, (X, tt), dY)
    adj = MaxAdj(ei, ew, n)
    Xd = X.detach()
    Y, L = SO.softmax_aggregate(adj.rowptr, adj.col, adj.val, Xd, t)
    dX = SO.softmax_aggregate_bwd(adj.rowptr_t, adj.col_t, adj.val_t, dY, Xd, Y, L, t)
    dt, mass = SO.softmax_aggregate_dt(adj.rowptr, adj.col, adj.val, dY, Xd, Y, L, t)
    assert float((Y - want.detach()).abs().max()) <= 1e-12 * float(want.detach().abs().max())
    assert float((dX - dX_want).abs().max()) <= 1e-12 * float(dX_want.abs().max())
    assert abs(float(dt) - float(dt_want)) <= 1e-12 * float(mass)
    # p sums to one over every row with entries, and L is the weighted log-sum-exp
    rows = rows_of(adj.rowptr)
    p = adj.val[:, None] * torch.exp(t * Xd[adj.col] - L[rows])
    psum = torch.zeros(n, H, dtype=torch.float64).index_add_(0, rows, p)
    live = adj.rowptr[1:] > adj.rowptr[:-1]
    assert float((psum[live] - 1).abs().max()) <= 1e-12 and bool((p > 0).all()) and bool((p <= 1 + 1e-12).all())
    # the SoftmaxAdj wrapper (what the model oracle uses) is the same operator
    assert torch.equal((SO.SoftmaxAdj(ei, ew, n, tt) @ X).detach(), want.detach())


def test_t_zero_is_the_weighted_mean_and_large_t_approaches_the_max():
    n, nnz, H = 30, 200, 5
    ei, ew = _graph(3, n, nnz)
    X = torch.randn(n, H, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    adj = MaxAdj(ei, ew, n)
    rows = rows_of(adj.rowptr)
    Y0, L0 = SO.softmax_aggregate(adj.rowptr, adj.col, adj.val, X, 0.0)
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, rows, adj.val)
    mean = torch.zeros(n, H, dtype=torch.float64).index_add_(0, rows, adj.val[:, None] * X[adj.col])
    live = deg > 0
    assert float((Y0[live] - mean[live] / deg[live, None]).abs().max()) <= 1e-13
    assert float((L0[live] - torch.log(deg[live])[:, None]).abs().max()) <= 1e-13   # M = 0, Z = the weighted degree
    # unit weights, every entry its own source (entry e reads X2[e]), the winner of every row and channel lifted by 0.5: a gap
    # of at least 0.5 to the runner-up, so t = 200 is the max up to e^-100
    m = 200
    g = torch.Generator().manual_seed(5)
    rows2 = torch.sort(torch.randint(0, 28, (m, ), generator=g)).values
    adj2 = MaxAdj(torch.stack((rows2, torch.arange(m))), torch.ones(m, dtype=torch.float64), m)
    assert torch.equal(adj2.col, torch.arange(m)) and torch.equal(rows_of(adj2.rowptr), rows2)
    X2 = torch.randn(m, H, generator=g, dtype=torch.float64)
    idx2 = rows2[:, None].expand(-1, H)
    top = torch.zeros(m, H, dtype=torch.float64).scatter_reduce(0, idx2, X2, "amax", include_self=False)
    X2 = X2 + 0.5 * (X2 == top[rows2]).to(torch.float64)
    top = torch.zeros(m, H, dtype=torch.float64).scatter_reduce(0, idx2, X2, "amax", include_self=False)
    Yt, _ = SO.softmax_aggregate(adj2.rowptr, adj2.col, adj2.val, X2, 200.0)
    live2 = adj2.rowptr[1:] > adj2.rowptr[:-1]
    assert int(live2.sum()) >= 20 and int((adj2.rowptr[1:] - adj2.rowptr[:-1]).max()) >= 5
    assert float((Yt[live2] - top[live2]).abs().max()) <= 1e-30
    Ys, _ = SO.softmax_aggregate(adj2.rowptr, adj2.col, adj2.val, X2, 2.0)
    assert float((Ys[live2] - top[live2]).abs().max()) > 1e-3    # (a small t is not the max: the limit is a limit)


def test_empty_row_rule():
    # row 0: two entries; row 1: none; row 2: one entry (its own softmax: Y = x, L = t x + log v)
    ei = torch.tensor([[0, 0, 2], [1, 2, 0]])
    ew = torch.tensor([1.0, 3.0, 0.5], dtype=torch.float64)
    X = torch.tensor([[1.0, -2.0], [0.0, 4.0], [2.0, 4.0]], dtype=torch.float64)
    adj = MaxAdj(ei, ew, 3)
    Y, L = SO.softmax_aggregate(adj.rowptr, adj.col, adj.val, X, 1.5)
    assert Y[1].tolist() == [0.0, 0.0] and L[1].tolist() == [0.0, 0.0]
    assert torch.allclose(Y[2], X[0], rtol=0, atol=1e-15) and torch.allclose(L[2], 1.5 * X[0] + np.log(0.5), rtol=0, atol=1e-15)
    e = np.exp(1.5 * 2.0)
    assert abs(float(Y[0, 0]) - 3 * e * 2.0 / (1 + 3 * e)) <= 1e-15 and float(Y[0, 1]) == 4.0   # equal messages: their value
    dX = SO.softmax_aggregate_bwd(adj.rowptr_t, adj.col_t, adj.val_t, torch.ones(3, 2, dtype=torch.float64), X, Y, L, 1.5)
    assert torch.allclose(dX.sum(0), torch.tensor([2.0, 2.0], dtype=torch.float64), rtol=0, atol=1e-14)  # a shift of X shifts Y


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
    from glass_amd import _lib
    lib = _lib.load()
    E_ARG, E_PLAN, E_UNSUPPORTED = -1, -2, -3
    plan = _plan([0, 1, 2])
    cut = _plan([0, 700, 700, 701])   # a row cut into chunks: partial slots
    x = np.zeros(64, dtype=np.float64)   # (8-byte aligned: it stands in for every pointer, the dt workspace included)
    p, h = x.ctypes.data, plan.ctypes.data
    assert int(cut[7]) >= 2 and int(cut[4]) + int(cut[5]) >= 3
    assert lib.glass_spmm_softmax_ws_bytes(cut.ctypes.data, 12) == int(cut[7]) * 12 * 12
    assert lib.glass_spmm_softmax_bwd_ws_bytes(cut.ctypes.data, 12) == int(cut[7]) * 12 * 4
    assert lib.glass_spmm_softmax_dt_ws_bytes(cut.ctypes.data, 12) == (int(cut[4]) + int(cut[5])) * 1 * 8
    assert lib.glass_spmm_softmax_dt_ws_bytes(cut.ctypes.data, 130) == (int(cut[4]) + int(cut[5])) * 3 * 8
    assert lib.glass_spmm_softmax_ws_bytes(h, 64) == 0 and lib.glass_spmm_softmax_bwd_ws_bytes(h, 64) == 0
    for q in (lib.glass_spmm_softmax_ws_bytes, lib.glass_spmm_softmax_bwd_ws_bytes, lib.glass_spmm_softmax_dt_ws_bytes):
        assert q(p, 64) == E_PLAN and q(None, 64) == E_PLAN and q(h, 0) == E_ARG and q(h, -4) == E_ARG
    fwd = lambda **k: lib.glass_spmm_softmax_csr_f32(*[k.get(n, d) for n, d in (
        ("rowptr", h), ("col", h), ("val", p), ("X", p), ("ldx", 8), ("t", p), ("Y", p), ("ldy", 8), ("L", p), ("ldl", 8),
        ("n_rows", 2), ("H", 8), ("hdr", h), ("plan", h), ("ws", None), ("stream", None))])
    bwd = lambda **k: lib.glass_spmm_softmax_bwd_f32(*[k.get(n, d) for n, d in (
        ("rowptr", h), ("col", h), ("val", p), ("X", p), ("ldx", 8), ("t", p), ("dY", p), ("lddy", 8), ("Y", p), ("ldy", 8),
        ("L", p), ("ldl", 8), ("dX", p), ("lddx", 8), ("n_rows", 2), ("H", 8), ("hdr", h), ("plan", h), ("ws", None),
        ("stream", None))])
    dt = lambda **k: lib.glass_spmm_softmax_dt_f32(*[k.get(n, d) for n, d in (
        ("rowptr", h), ("col", h), ("val", p), ("X", p), ("ldx", 8), ("t", p), ("dY", p), ("lddy", 8), ("Y", p), ("ldy", 8),
        ("L", p), ("ldl", 8), ("dt", p), ("n_rows", 2), ("H", 8), ("hdr", h), ("plan", h), ("ws", p), ("stream", None))])
    for call, ptrs, lds in ((fwd, ("rowptr", "X", "t", "Y", "L", "hdr", "plan", "col", "val"), ("ldx", "ldy", "ldl")),
                            (bwd, ("rowptr", "X", "t", "dY", "Y", "L", "dX", "hdr", "plan", "col", "val"),
                             ("ldx", "lddy", "ldy", "ldl", "lddx")),
                            (dt, ("rowptr", "X", "t", "dY", "Y", "L", "dt", "hdr", "plan", "col", "val", "ws"),
                             ("ldx", "lddy", "ldy", "ldl"))):
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
    for call in (fwd, bwd):
        assert call(hdr=cut.ctypes.data, plan=cut.ctypes.data, n_rows=3) == E_ARG and b"ws is null" in lib.glass_last_error_string()
    assert dt(ws=p + 4) == E_ARG and b"8-byte" in lib.glass_last_error_string()


def test_names_are_accepted_where_the_aggregation_is_chosen():
    import GLASSTest
    assert GLASSTest.parse_args(["--use_one", "--aggr", "softmax"]).aggr == "softmax"
    with pytest.raises(SystemExit):
        GLASSTest.parse_args(["--use_one", "--aggr", "softmin"])
    # the host side refuses before it touches a device: an unknown name as the reference does, a CPU graph loudly
    from glass_amd import graph, models, ops, _lib
    ei, ew = torch.tensor([[0, 1], [1, 0]]), torch.ones(2)
    with pytest.raises(NotImplementedError):
        graph.CSRAdj(ei, ew, 2, "softmin")
    with pytest.raises(NotImplementedError):
        models.buildAdj(ei, ew, 2, "softmin")
    with pytest.raises(_lib.GlassHipError, match="GPU only"):
        graph.CSRAdj(ei, ew, 2, "softmax")
    with pytest.raises(_lib.GlassHipError, match="GPU only"):
        models.buildAdj(ei, ew, 2, "softmax")

    class _Adj:   # the dispatch reads the name only
        aggr = "softmax"
    with pytest.raises(_lib.GlassHipError, match="spmm_softmax"):
        ops.spmm(_Adj(), torch.zeros(2, 4))
    with pytest.raises(_lib.GlassHipError, match="replicated softmax aggregation is not built"):
        ops.spmm_rep(_Adj(), torch.zeros(4, 4), 2)
    _Adj.aggr = "mean"
    with pytest.raises(_lib.GlassHipError, match="not 'softmax'"):
        ops.spmm_softmax(_Adj(), torch.zeros(2, 4), torch.ones(1))


def test_the_temperature_is_a_parameter_of_softmax_layers_only():
    from glass_amd import models
    for cls in (models.GLASSConv, models.MyGCNConv):
        for aggr in ("mean", "sum", "gcn", "max"):
            conv = cls(8, 8, aggr=aggr)
            assert "t" not in conv.state_dict() and not hasattr(conv, "t"), (cls.__name__, aggr)
        conv = cls(8, 8, aggr="softmax")
        assert conv.state_dict()["t"].tolist() == [1.0] and conv.t.requires_grad and conv.t.dtype == torch.float32
        conv = cls(8, 8, aggr="softmax", softmax_t=2.0)
        assert conv.t.tolist() == [2.0]
        with torch.no_grad():
            conv.t.fill_(-3.0)
        ptr = conv.t.data_ptr()
        conv.reset_parameters()
        assert conv.t.tolist() == [2.0] and conv.t.data_ptr() == ptr and "t" in dict(conv.named_parameters())
    from helpers import build_glass
    keys = set(build_glass(64, 2, 5, 3, "softmax", "mean", 0.8).state_dict()) - set(build_glass(64, 2, 5, 3, "mean", "mean", 0.8).state_dict())
    assert keys == {"conv.convs.0.t", "conv.convs.1.t"}
