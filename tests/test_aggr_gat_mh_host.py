"""Multi-head attention aggregation without a GPU: the sliced restatement tests/aggr_gat_mh_oracle.py against fp64 autograd
through its direct scatter statement, the argument codes and workspace formulas of the glass_*_mh_* exports (validation runs
before any HIP call), the driver flag and the layer's gat_heads argument."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aggr_gat_mh_oracle as MO
from aggr_max_oracle import MaxAdj, rows_of

E_ARG, E_PLAN, E_UNSUPPORTED = -1, -2, -3
MH_NAMES = ("glass_gat_scores_mh_f32", "glass_spmm_gat_mh_ws_bytes", "glass_spmm_gat_mh_csr_f32", "glass_spmm_gat_mh_edge_ws_bytes",
            "glass_spmm_gat_mh_edge_f32", "glass_spmm_gat_mh_bwd_ws_bytes", "glass_spmm_gat_mh_bwd_f32",
            "glass_spmm_gat_mh_da_ws_bytes", "glass_spmm_gat_mh_da_f32", "glass_gat_datt_mh_ws_bytes", "glass_gat_datt_mh_f32")


def _small_graph():
    """n = 12: row 11 (and column 11) empty, the pair (2, 3) twice with different weights, a self-loop (4, 4); weights in
    [0.25, 2), edge order shuffled"""
    g = torch.Generator().manual_seed(7)
    n, nnz = 12, 60
    ei = torch.stack((torch.randint(0, n - 1, (nnz, ), generator=g), torch.randint(0, n - 1, (nnz, ), generator=g)))
    ei = torch.cat((ei, torch.tensor([[2, 2, 4], [3, 3, 4]])), 1)
    ew = torch.rand(ei.shape[1], generator=g, dtype=torch.float64) * 1.75 + 0.25
    perm = torch.randperm(ei.shape[1], generator=g)
    return n, ei[:, perm], ew[perm]


def _within(got, want, mass, tol=1e-12):
    return bool(((got - want).abs() <= tol * mass).all())


@pytest.mark.parametrize("H,K", [(8, 2), (16, 4), (12, 3)])
@pytest.mark.parametrize("slope", (0.2, 0.0))
def test_sliced_restatement_equals_fp64_autograd_through_the_direct_statement(H, K, slope):
    n, ei, ew = _small_graph()
    assert int(((ei[0] == 2) & (ei[1] == 3)).sum()) >= 2 and bool(((ei[0] == 4) & (ei[1] == 4)).any())
    assert not bool((ei[0] == n - 1).any())
    g = torch.Generator().manual_seed(100 * H + K)
    X = torch.randn(n, H, generator=g, dtype=torch.float64, requires_grad=True)
    dY = torch.randn(n, H, generator=g, dtype=torch.float64)
    att_src = (torch.rand(H, generator=g, dtype=torch.float64) - 0.5).requires_grad_(True)
    att_dst = (torch.rand(H, generator=g, dtype=torch.float64) - 0.5).requires_grad_(True)
    want = MO.scatter_gat_mh_aggregate(ei, ew, n, X, att_src, att_dst, slope, K)
    dX_want, ds_want, dd_want = torch.autograd.grad(want, (X, att_src, att_dst), dY)
    adj = MaxAdj(ei, ew, n)
    Xd, As, Ad = X.detach(), att_src.detach(), att_dst.detach()
    Y, L, a, b = MO.gat_mh_aggregate(adj.rowptr, adj.col, adj.val, Xd, As, Ad, slope, K)
    r = MO.gat_mh_aggregate_bwd(adj.rowptr, adj.col, adj.val, dY, Xd, Y, L, a, b, As, Ad, slope, K)
    nnz = adj.col.shape[0]
    assert Y.shape == (n, H) and L.shape == a.shape == b.shape == r.da.shape == r.db.shape == (n, K) and r.g.shape == (nnz, K)
    assert float((Y - want.detach()).abs().max()) <= 1e-12 * float(want.detach().abs().max())
    assert float((r.dX - dX_want).abs().max()) <= 1e-12 * float(dX_want.abs().max())
    assert float((r.datt_src - ds_want).abs().max()) <= 1e-12 * float(ds_want.abs().max())
    assert float((r.datt_dst - dd_want).abs().max()) <= 1e-12 * float(dd_want.abs().max())
    assert float(ds_want.abs().max()) > 1e-3 and float(dd_want.abs().max()) > 1e-3
    # g, da, db through their definitions: autograd with the per-edge scores / the node scores as free inputs, every head at once
    D = H // K
    rows, col = rows_of(adj.rowptr), adj.col
    a0, b0 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    u = (a0[col] + b0[rows]).detach().requires_grad_(True)   # [nnz, K], sorted entry order
    s = F.leaky_relu(u, slope)
    w = adj.val[:, None] * torch.exp(s - L[rows])            # (L is the log-sum-exp: the normalised weights at the forward's point)
    Z = torch.zeros(n, K, dtype=torch.float64).index_add(0, rows, w)
    live = (adj.rowptr[1:] > adj.rowptr[:-1])[:, None]
    Yu = torch.zeros(n, K, D, dtype=torch.float64).index_add(0, rows, w[:, :, None] * Xd.reshape(n, K, D)[col])
    Yu = (Yu / torch.where(live, Z, torch.ones(()))[:, :, None]).reshape(n, H)
    g_want, = torch.autograd.grad(Yu, u, dY)
    assert _within(r.g, g_want, r.mass_g)
    da_want = torch.zeros(n, K, dtype=torch.float64).index_add_(0, col, g_want)
    db_want = torch.zeros(n, K, dtype=torch.float64).index_add_(0, rows, g_want)
    assert _within(r.da, da_want, r.mass_da) and _within(r.db, db_want, r.mass_db)
    assert float(r.g.abs().max()) > 1e-3
    # the empty row, and p sums to one per row and head
    assert bool((Y[n - 1] == 0).all()) and bool((L[n - 1] == 0).all()) and bool((r.db[n - 1] == 0).all()) and bool((r.da[n - 1] == 0).all())
    psum = torch.zeros(n, K, dtype=torch.float64).index_add_(0, rows, r.p)
    assert float((psum[live[:, 0]] - 1).abs().max()) <= 1e-12
    # heads differ: no head's softmax is another's
    assert float((r.p[:, 0] - r.p[:, 1]).abs().max()) > 1e-3
    # the wrapper the model oracle uses is the direct statement
    assert torch.equal((MO.GatMHAdj(ei, ew, n, att_src, att_dst, slope, K) @ X).detach(), want.detach())


def test_one_head_is_the_single_head_restatement():
    import aggr_gat_oracle as GO
    n, ei, ew = _small_graph()
    g = torch.Generator().manual_seed(3)
    X = torch.randn(n, 6, generator=g, dtype=torch.float64)
    As, Ad = (torch.rand(6, generator=g, dtype=torch.float64) - 0.5 for _ in range(2))
    got, want = MO.scatter_gat_mh_aggregate(ei, ew, n, X, As, Ad, 0.2, 1), GO.scatter_gat_aggregate(ei, ew, n, X, As, Ad, 0.2)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def _plan(rowptr):
    from glass_amd import _lib
    lib = _lib.load()
    rp = np.asarray(rowptr, dtype=np.int32)
    words = ctypes.c_int64(0)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, rp.shape[0] - 1, None, ctypes.byref(words)) == 0
    plan = np.zeros(words.value, dtype=np.int32)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, rp.shape[0] - 1, plan.ctypes.data, ctypes.byref(words)) == 0
    return plan


def test_symbols_exist_and_are_declared():
    import os
    from glass_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glass_hip.h")).read()
    for name in MH_NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert f" {name}(" in header, name
        if name != "glass_gat_datt_mh_ws_bytes":   # K after H
            assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[name.replace("_mh", "")][1]) + 1, name
    assert lib.glass_version() == _lib.ABI_VERSION == 6   # purely additive


def test_mh_exports_answer_with_argument_codes_before_any_launch():
    from glass_amd import _lib
    lib = _lib.load()
    plan = _plan([0, 1, 2])
    cut = _plan([0, 700, 700, 701])   # a row cut into chunks: partial slots
    x = np.zeros(64, dtype=np.float64)   # (8-byte aligned: it stands in for every pointer, the datt workspace included)
    p, h = x.ctypes.data, plan.ctypes.data
    slots = int(cut[7])
    assert slots >= 2
    H, K = 24, 3
    assert lib.glass_spmm_gat_mh_ws_bytes(cut.ctypes.data, H, K) == slots * (H + 2 * K) * 4
    assert lib.glass_spmm_gat_mh_edge_ws_bytes(cut.ctypes.data, H, K) == slots * K * 4
    assert lib.glass_spmm_gat_mh_bwd_ws_bytes(cut.ctypes.data, H, K) == slots * (H + K) * 4
    assert lib.glass_spmm_gat_mh_da_ws_bytes(cut.ctypes.data, H, K) == slots * K * 4
    for n, W in ((1000, 64), (1000, 260), (0, 64)):
        assert lib.glass_gat_datt_mh_ws_bytes(n, W) == lib.glass_gat_datt_ws_bytes(n, W)
    assert lib.glass_gat_datt_mh_ws_bytes(1000, 64) == 4 * 2 * 64 * 8
    assert lib.glass_gat_datt_mh_ws_bytes(5, 0) == E_ARG and lib.glass_gat_datt_mh_ws_bytes(-1, 8) == E_ARG
    for q in (lib.glass_spmm_gat_mh_ws_bytes, lib.glass_spmm_gat_mh_edge_ws_bytes, lib.glass_spmm_gat_mh_bwd_ws_bytes,
              lib.glass_spmm_gat_mh_da_ws_bytes):
        assert q(h, 64, 4) == 0 and q(p, 64, 4) == E_PLAN and q(None, 64, 4) == E_PLAN
        assert q(h, 0, 4) == E_ARG and q(h, -4, 4) == E_ARG and q(h, 64, 0) == E_ARG and q(h, 64, -2) == E_ARG
    call = lambda fn, spec: (lambda **k: fn(*[k.get(n, d) for n, d in spec]))
    fwd = call(lib.glass_spmm_gat_mh_csr_f32, (
        ("rowptr", h), ("col", h), ("val", p), ("X", p), ("ldx", 8), ("a", p), ("b", p), ("slope", 0.2), ("Y", p), ("ldy", 8),
        ("L", p), ("n_rows", 2), ("H", 8), ("K", 2), ("hdr", h), ("plan", h), ("ws", None), ("stream", None)))
    edge = call(lib.glass_spmm_gat_mh_edge_f32, (
        ("rowptr", h), ("col", h), ("val", p), ("X", p), ("ldx", 8), ("a", p), ("b", p), ("slope", 0.2), ("dY", p), ("lddy", 8),
        ("Y", p), ("ldy", 8), ("L", p), ("g", p), ("db", p), ("n_rows", 2), ("H", 8), ("K", 2), ("hdr", h), ("plan", h),
        ("ws", None), ("stream", None)))
    bwd = call(lib.glass_spmm_gat_mh_bwd_f32, (
        ("rowptr", h), ("col", h), ("val", p), ("eid", h), ("a", p), ("b", p), ("slope", 0.2), ("dY", p), ("lddy", 8), ("L", p),
        ("g", p), ("db", p), ("att_src", p), ("att_dst", p), ("dX", p), ("lddx", 8), ("da", p), ("n_rows", 2), ("H", 8), ("K", 2),
        ("hdr", h), ("plan", h), ("ws", None), ("stream", None)))
    da = call(lib.glass_spmm_gat_mh_da_f32, (
        ("rowptr", h), ("col", h), ("val", p), ("eid", h), ("g", p), ("da", p), ("n_rows", 2), ("H", 8), ("K", 2), ("vec", 1),
        ("hdr", h), ("plan", h), ("ws", None), ("stream", None)))
    scores = call(lib.glass_gat_scores_mh_f32, (("X", p), ("ldx", 8), ("att_src", p), ("att_dst", p), ("a", p), ("b", p),
                                                ("n_rows", 2), ("H", 8), ("K", 2), ("stream", None)))
    datt = call(lib.glass_gat_datt_mh_f32, (("X", p), ("ldx", 8), ("da", p), ("db", p), ("datt_src", p), ("datt_dst", p),
                                            ("n_rows", 2), ("H", 8), ("K", 2), ("ws", p), ("stream", None)))
    table = (
        (fwd, ("rowptr", "X", "a", "b", "Y", "L", "hdr", "plan", "col", "val"), ("ldx", "ldy"), "X", True),
        (edge, ("rowptr", "X", "a", "b", "dY", "Y", "L", "g", "db", "hdr", "plan", "col", "val"), ("ldx", "lddy", "ldy"), "X", True),
        (bwd, ("rowptr", "a", "b", "dY", "L", "g", "db", "att_src", "att_dst", "dX", "da", "hdr", "plan", "col", "val", "eid"),
         ("lddy", "lddx"), "dY", True),
        (da, ("rowptr", "g", "da", "hdr", "plan", "col", "val", "eid"), (), "g", False),
        (scores, ("X", "att_src", "att_dst", "a", "b"), ("ldx", ), "X", False),
        (datt, ("X", "da", "db", "datt_src", "datt_dst", "ws"), ("ldx", ), "X", False))
    for fn, ptrs, lds, odd, has_slope in table:
        for name in ptrs:
            assert fn(**{name: None}) == E_ARG, name
        for name in lds:
            assert fn(**{name: 7}) == E_ARG, name
        assert fn(H=0) == E_ARG
        assert fn(K=0) == E_ARG and fn(K=-1) == E_ARG
        assert fn(**{odd: p + 2}) == E_ARG and b"aligned" in lib.glass_last_error_string()
        if has_slope:
            assert fn(slope=float("nan")) == E_ARG and b"slope" in lib.glass_last_error_string()
        # D = 9 and D = 512: refused, never computed, the message names the three numbers
        for Hb, Kb, Db in ((18, 2, 9), (1024, 2, 512)):
            wide = {name: Hb for name in lds}
            assert fn(H=Hb, K=Kb, **wide, **({"vec": 0} if fn is da else {})) == E_UNSUPPORTED, (Hb, Kb)
            msg = lib.glass_last_error_string()
            assert f"H = {Hb}".encode() in msg and f"K = {Kb}".encode() in msg and f"D = H / K = {Db}".encode() in msg, msg
        assert fn(H=12, K=5, **{name: 12 for name in lds}, **({"vec": 0} if fn is da else {})) == E_UNSUPPORTED   # K does not divide H
        assert fn(H=4, K=2, **({"vec": 0} if fn is da else {})) == E_UNSUPPORTED    # D = 2
        if fn not in (scores, datt):
            assert fn(n_rows=3) == E_PLAN and b"plan does not match" in lib.glass_last_error_string()
            assert fn(hdr=p) == E_PLAN
            # a plan with partial slots and no workspace
            assert fn(hdr=cut.ctypes.data, plan=cut.ctypes.data, n_rows=3) == E_ARG and b"ws is null" in lib.glass_last_error_string()
        else:
            assert fn(n_rows=-1) == E_ARG
            assert fn(n_rows=0) == 0   # nothing to launch
    assert datt(ws=p + 4) == E_ARG and b"8-byte" in lib.glass_last_error_string()


def test_gat_heads_flag_parses():
    import GLASSTest
    assert GLASSTest.parse_args(["--use_one"]).gat_heads == 1
    args = GLASSTest.parse_args(["--use_one", "--aggr", "gat", "--gat_heads", "4"])
    assert args.aggr == "gat" and args.gat_heads == 4
    for bad in ("0", "x", "-2", "1.5"):
        with pytest.raises(SystemExit):
            GLASSTest.parse_args(["--use_one", "--aggr", "gat", "--gat_heads", bad])


def test_the_layer_takes_gat_heads():
    from glass_amd import graph, models, ops
    with pytest.raises(ValueError, match="heads"):
        models.GLASSConv(8, 12, aggr="gat", gat_heads=5)
    for out, heads in ((12, 2), (12, 6), (1024, 2), (16, 0), (16, -1), (16, 1.5)):   # D = 6, 2, 512; no head; not an integer
        with pytest.raises(ValueError):
            models.GLASSConv(8, out, aggr="gat", gat_heads=heads)
    for aggr in ("mean", "sum", "gcn", "max", "softmax"):   # ignored, as gat_slope is
        conv = models.GLASSConv(8, 12, aggr=aggr, gat_heads=5)
        assert not any(k.startswith("att_") for k in conv.state_dict())
    one, four = models.GLASSConv(8, 16, aggr="gat", gat_heads=1), models.GLASSConv(8, 16, aggr="gat", gat_heads=4)
    assert one.gat_heads == 1 and four.gat_heads == 4 and models.GLASSConv(8, 16, aggr="gat").gat_heads == 1
    sd1, sd4 = one.state_dict(), four.state_dict()
    assert list(sd1) == list(sd4) and all(sd1[k].shape == sd4[k].shape and sd1[k].dtype == sd4[k].dtype for k in sd1)
    assert sd4["att_src"].shape == sd4["att_dst"].shape == (16, )
    # one head: the constructor without the argument, bit for bit
    torch.manual_seed(11)
    a = models.GLASSConv(8, 16, aggr="gat")
    torch.manual_seed(11)
    b = models.GLASSConv(8, 16, aggr="gat", gat_heads=1)
    assert all(torch.equal(a.state_dict()[k], b.state_dict()[k]) for k in a.state_dict())
    b.att_src.data.zero_()
    torch.manual_seed(5)
    b.reset_parameters()
    torch.manual_seed(5)
    a.reset_parameters()
    assert torch.equal(a.att_src, b.att_src) and torch.equal(a.att_dst, b.att_dst)
    # ... and what xavier_uniform_ on the [1, H] view draws
    v = torch.empty(16)
    torch.manual_seed(9)
    torch.nn.init.xavier_uniform_(v.view(1, -1))
    torch.manual_seed(9)
    models._reset_gat_att(one)
    assert torch.equal(one.att_src.detach(), v)
    # four heads: xavier on a [1, D] view per head
    bound = (6.0 / (1 + 4)) ** 0.5
    for seed in range(5):
        torch.manual_seed(seed)
        conv = models.GLASSConv(8, 16, aggr="gat", gat_heads=4)
        for vec in (conv.att_src, conv.att_dst):
            assert float(vec.detach().abs().max()) <= bound
    torch.manual_seed(21)
    many = torch.cat([models.GLASSConv(8, 256, aggr="gat", gat_heads=64).att_src.detach() for _ in range(4)])
    assert float(many.abs().max()) > 0.9 * bound > (6.0 / (1 + 256)) ** 0.5, "the bound is the head's, not the row's"
    # the width rule, where the operator is called
    assert graph.CSRAdj.gat_head_width(64, 4) == 16 and graph.CSRAdj.gat_head_width(18, 1) == 18

    class _Adj:
        aggr = "gat"
    for H, K in ((12, 5), (18, 2), (1024, 2), (16, 0)):
        with pytest.raises(ValueError):
            ops.spmm_gat(_Adj(), torch.zeros(2, H), torch.zeros(H), torch.zeros(H), 0.2, heads=K)
