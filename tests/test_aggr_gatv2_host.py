"""Dynamic attention neighbour aggregation (aggr "gatv2") without a GPU: the restatement tests/aggr_gatv2_oracle.py against fp64
autograd through a dense-mask statement, the fp32 restatement in the kernels' summation order against the fp64 one on the GPU
test's own inputs and bounds, the argument codes of the new exports (validation runs before any HIP call), the driver flag and
the layer's parameter."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import aggr_gatv2_oracle as VO
from aggr_max_oracle import MaxAdj


def _small_graph():
    """12 nodes: a self-loop (3, 3), a parallel duplicate (1 <- 2 twice, other weights), a one-directional edge (4 <- 5 only),
    node 11 isolated (no entry in, none out); the rest undirected pairs.  (row = destination, col = source)"""
    und = [(0, 1), (0, 2), (2, 6), (6, 7), (7, 8), (8, 9), (9, 10), (10, 0), (5, 6), (1, 7)]
    row = [a for a, b in und] + [b for a, b in und] + [3, 1, 1, 4]
    col = [b for a, b in und] + [a for a, b in und] + [3, 2, 2, 5]
    g = torch.Generator().manual_seed(5)
    ew = torch.rand(len(row), generator=g, dtype=torch.float64) * 1.75 + 0.25
    return torch.tensor([row, col]), ew, 12


@pytest.mark.parametrize("slope", (0.2, 0.0, 1.0))
def test_restatement_equals_fp64_autograd_through_a_dense_mask(slope):
    """The dense statement: W[i, j] the summed weight of the entries (i <- j) — duplicates have one score, so their weights
    add — and a softmax over j of s[i, j] + log W[i, j], -inf where there is no entry."""
    ei, ew, n = _small_graph()
    H = 7
    g = torch.Generator().manual_seed(1)
    X = torch.randn(n, H, generator=g, dtype=torch.float64, requires_grad=True)
    dY = torch.randn(n, H, generator=g, dtype=torch.float64)
    att = (torch.rand(H, generator=g, dtype=torch.float64) - 0.5).requires_grad_(True)
    W = torch.zeros(n, n, dtype=torch.float64).index_put_((ei[0], ei[1]), ew, accumulate=True)
    S = (F.leaky_relu(X[:, None, :] + X[None, :, :], slope) * att).sum(-1)
    logits = torch.where(W > 0, S + torch.log(torch.where(W > 0, W, torch.ones(()).double())), torch.full((), -float("inf")).double())
    live = (W > 0).any(1)
    P = torch.zeros(n, n, dtype=torch.float64)
    P[live] = torch.softmax(logits[live], dim=1)
    want = P @ X
    dX_want, datt_want = torch.autograd.grad(want, (X, att), dY)
    adj = MaxAdj(ei, ew, n)
    r = VO.reference(adj, X.detach(), dY, att.detach(), slope)
    assert float(np.abs(r.Y - want.detach().numpy()).max()) <= 1e-12 * float(want.detach().abs().max())
    assert float(np.abs(r.dX - dX_want.numpy()).max()) <= 1e-12 * float(dX_want.abs().max())
    assert bool((np.abs(r.datt - datt_want.numpy()) <= 1e-12 * r.mass_datt).all()) and float(datt_want.abs().max()) > 1e-3
    assert not live[11] and bool((r.Y[11] == 0).all()) and r.L[11] == 0 and bool((r.dX[11] == 0).all())
    assert float(np.abs(r.L[live.numpy()] - torch.logsumexp(logits[live], 1).detach().numpy()).max()) <= 1e-12
    # p sums to one over every row with entries; the scatter form (what the model oracle uses) is the same operator
    psum = np.zeros(n)
    np.add.at(psum, VO.rows_of(adj.rowptr), r.p)
    assert float(np.abs(psum[live.numpy()] - 1).max()) <= 1e-12
    sc = VO.GatV2Adj(ei, ew, n, att, slope) @ X
    assert float((sc - want).detach().abs().max()) <= 1e-12 * float(want.detach().abs().max())
    # dynamic attention: two destinations rank the same two sources in different orders (static attention cannot)
    if slope == 0.2:
        Xr = torch.tensor([[1.0, -1.0], [-1.0, 1.0], [2.0, 0.0], [0.0, 2.0]], dtype=torch.float64)
        a2 = torch.tensor([1.0, 1.0], dtype=torch.float64)
        s = (F.leaky_relu(Xr[:2, None, :] + Xr[None, 2:, :], slope) * a2).sum(-1)   # destinations 0, 1 x sources 2, 3
        assert s[0, 0] > s[0, 1] and s[1, 0] < s[1, 1]


def test_the_rule_at_u_zero_is_torchs():
    """Rows where X[i] = -X[j] exactly: u = 0 in every channel, f = slope there, as torch's leaky_relu backward has it."""
    ei = torch.tensor([[0, 0, 1], [1, 2, 0]])
    ew = torch.tensor([1.0, 0.5, 2.0], dtype=torch.float64)
    x1 = torch.tensor([0.5, -1.25, 2.0], dtype=torch.float64)
    X = torch.stack((-x1, x1, torch.tensor([0.25, 1.0, -0.5], dtype=torch.float64))).requires_grad_(True)
    att = torch.tensor([0.3, -0.2, 0.4], dtype=torch.float64, requires_grad=True)
    dY = torch.tensor([[1.0, -2.0, 0.5], [0.25, 1.0, -1.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    want = VO.scatter_gatv2_aggregate(ei, ew, 3, X, att, 0.2)
    dX_want, datt_want = torch.autograd.grad(want, (X, att), dY)
    r = VO.reference(MaxAdj(ei, ew, 3), X.detach(), dY, att.detach(), 0.2)
    assert float(np.abs(r.dX - dX_want.numpy()).max()) <= 1e-12 and float(np.abs(r.datt - datt_want.numpy()).max()) <= 1e-12
    assert float(np.abs(r.dX).max()) > 1e-2


@pytest.mark.parametrize("kind", ("mixed", "all_long"))
def test_fp32_in_the_kernels_order_stays_within_the_gpu_tests_bounds(kind):
    """The GPU test's own graphs, seeds, widths and slopes: att and X are drawn so that |s_e| <= 8 (asserted), and the fp32
    restatement — rounded u and r, s from fp64 sums rounded once, the accumulators' rules along the lane groups' sequences —
    must meet the bounds the GPU test applies, so the reference alone is known to stay within them."""
    import test_gpu_aggr_gatv2 as T
    adj = T.ref_adj(kind)
    worst = {}
    for H in VO.WIDTHS:
        X, dY, att = T.operands(kind, H)
        for slope in VO.SLOPES:
            r = VO.reference(adj, X, dY, att, slope)
            assert float(np.abs(r.s).max()) <= VO.S_MAX
            for vec in ((True, False) if H % 4 == 0 else (False, )):
                e = VO.errors(VO.gatv2_fp32(adj, X, dY, att, slope, vec=vec), r)
                assert all(v <= VO.TOL for v in e.values()), (kind, H, slope, vec, e)
                worst = {k: max(v, worst.get(k, 0.0)) for k, v in e.items()}
    print(f"{kind}: worst fp32-restatement error per quantity: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_the_attention_vector_is_a_parameter_of_gatv2_layers_only():
    from glass_amd import models
    for aggr in ("mean", "sum", "gcn", "max", "softmax", "gat"):
        conv = models.GLASSConv(8, 8, aggr=aggr)
        assert "att" not in conv.state_dict() and not hasattr(conv, "att"), aggr
    mean_keys = list(models.GLASSConv(8, 12, aggr="mean").state_dict())
    assert mean_keys == ["trans_fns.0.weight", "trans_fns.0.bias", "trans_fns.1.weight", "trans_fns.1.bias", "comb_fns.0.weight",
                         "comb_fns.0.bias", "comb_fns.1.weight", "comb_fns.1.bias"] + [k for k in mean_keys if k.startswith("gn.")]
    conv = models.GLASSConv(8, 12, aggr="gatv2")
    assert set(conv.state_dict()) - set(mean_keys) == {"att"} and set(mean_keys) <= set(conv.state_dict())
    assert conv.gat_slope == 0.2 and models.GLASSConv(8, 12, aggr="gatv2", gat_slope=0.05).gat_slope == 0.05
    bound = (6.0 / (1 + 12)) ** 0.5   # xavier_uniform_ on the [1, H] view
    assert conv.att.shape == (12, ) and conv.att.dtype == torch.float32 and conv.att.requires_grad
    assert 0 < float(conv.att.detach().abs().max()) <= bound
    before, ptr = conv.att.detach().clone(), conv.att.data_ptr()
    conv.reset_parameters()
    assert conv.att.data_ptr() == ptr and not torch.equal(conv.att.detach(), before) and float(conv.att.detach().abs().max()) <= bound
    from helpers import build_glass
    keys = set(build_glass(64, 2, 5, 3, "gatv2", "mean", 0.8).state_dict()) - set(build_glass(64, 2, 5, 3, "mean", "mean", 0.8).state_dict())
    assert keys == {"conv.convs.0.att", "conv.convs.1.att"}
    from glass_amd import stack
    assert not stack.StackProgram.supported(build_glass(64, 2, 5, 3, "gatv2", "mean", 0.8).conv)


def test_what_gatv2_refuses():
    from glass_amd import graph, models, ops, _lib
    for heads in (2, 0, True):
        with pytest.raises(ValueError, match="one attention head"):
            models.GLASSConv(8, 8, aggr="gatv2", gat_heads=heads)
    with pytest.raises(ValueError, match="live_edge_weight"):
        models.GLASSConv(8, 8, aggr="gatv2", live_edge_weight=True)
    with pytest.raises(ValueError, match="edge_dropout"):
        models.GLASSConv(8, 8, aggr="gatv2", edge_dropout=0.1)
    conv = models.GLASSConv(8, 8, aggr="gatv2")
    ei, ew = torch.tensor([[0, 1], [1, 0]]), torch.ones(2)
    with pytest.raises(ValueError, match="no replicated form"):
        conv(torch.zeros(4, 8), ei, ew, torch.zeros(4, dtype=torch.uint8), batch=ops.Replicas(2, 2))
    with pytest.raises(_lib.GlassHipError, match="GPU only"):
        graph.CSRAdj(ei, ew, 2, "gatv2")
    with pytest.raises(_lib.GlassHipError, match="GPU only"):
        models.buildAdj(ei, ew, 2, "gatv2")
    with pytest.raises(NotImplementedError):
        models.buildAdj(ei, ew, 2, "gatv3")

    class _Adj:   # the dispatch reads the name only
        aggr = "gatv2"
    with pytest.raises(_lib.GlassHipError, match="spmm_gatv2"):
        ops.spmm(_Adj(), torch.zeros(2, 4))
    with pytest.raises(_lib.GlassHipError, match="replicated gatv2 aggregation is not built"):
        ops.spmm_rep(_Adj(), torch.zeros(4, 4), 2)
    _Adj.aggr = "gat"
    with pytest.raises(_lib.GlassHipError, match="not 'gatv2'"):
        ops.spmm_gatv2(_Adj(), torch.zeros(2, 4), torch.zeros(4), 0.2)
    for what in ("gatv2_score", "gatv2_fwd", "gatv2_edge", "gatv2_bwd", "gatv2_datt"):
        with pytest.raises(_lib.GlassHipError, match="not 'gatv2'"):
            graph.CSRAdj._need(_Adj(), what, "gatv2")


def test_the_driver_takes_the_name():
    import GLASSTest
    args = GLASSTest.parse_args(["--use_one", "--aggr", "gatv2", "--gat_slope", "0.1"])
    assert args.aggr == "gatv2" and args.gat_slope == 0.1
    with pytest.raises(SystemExit):
        GLASSTest.parse_args(["--use_one", "--aggr", "gatv3"])


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
    none = _plan([0, 0, 0])           # a plan without entries
    x = np.zeros(64, dtype=np.float64)   # (8-byte aligned: it stands in for every pointer, the datt workspace included)
    p, h = x.ctypes.data, plan.ctypes.data
    slots = int(cut[7])
    assert slots >= 2
    assert lib.glass_spmm_gatv2_score_ws_bytes(cut.ctypes.data, 12) == 0
    assert lib.glass_spmm_gatv2_ws_bytes(cut.ctypes.data, 12) == slots * (12 + 2) * 4
    assert lib.glass_spmm_gatv2_edge_ws_bytes(cut.ctypes.data, 12) == slots * 2 * 12 * 4
    assert lib.glass_spmm_gatv2_bwd_ws_bytes(cut.ctypes.data, 12) == slots * 12 * 4
    assert lib.glass_spmm_gatv2_datt_ws_bytes(1000, 64) == 4 * 64 * 8 and lib.glass_spmm_gatv2_datt_ws_bytes(1000, 260) == 2 * 260 * 8
    assert lib.glass_spmm_gatv2_datt_ws_bytes(0, 64) == 0 and lib.glass_spmm_gatv2_datt_ws_bytes(5, 0) == E_ARG
    assert lib.glass_spmm_gatv2_datt_ws_bytes(-1, 8) == E_ARG
    for q in (lib.glass_spmm_gatv2_score_ws_bytes, lib.glass_spmm_gatv2_ws_bytes, lib.glass_spmm_gatv2_edge_ws_bytes,
              lib.glass_spmm_gatv2_bwd_ws_bytes):
        assert q(h, 64) == 0 and q(p, 64) == E_PLAN and q(None, 64) == E_PLAN and q(h, 0) == E_ARG and q(h, -4) == E_ARG
    call = lambda fn, spec: (lambda **k: fn(*[k.get(n, d) for n, d in spec]))
    tail = (("n_rows", 2), ("H", 8), ("hdr", h), ("plan", h), ("ws", None), ("stream", None))
    score = call(lib.glass_spmm_gatv2_score_f32, (
        ("rowptr", h), ("col", h), ("val", p), ("X", p), ("ldx", 8), ("att", p), ("slope", 0.2), ("s", p)) + tail)
    fwd = call(lib.glass_spmm_gatv2_csr_f32, (
        ("rowptr", h), ("col", h), ("val", p), ("X", p), ("ldx", 8), ("s", p), ("Y", p), ("ldy", 8), ("L", p)) + tail)
    edge = call(lib.glass_spmm_gatv2_edge_f32, (
        ("rowptr", h), ("col", h), ("val", p), ("X", p), ("ldx", 8), ("att", p), ("slope", 0.2), ("s", p), ("dY", p), ("lddy", 8),
        ("Y", p), ("ldy", 8), ("L", p), ("g", p), ("p", p), ("Gd", p), ("R", p)) + tail)
    bwd = call(lib.glass_spmm_gatv2_bwd_f32, (
        ("rowptr", h), ("col", h), ("val", p), ("eid", h), ("X", p), ("ldx", 8), ("att", p), ("slope", 0.2), ("dY", p), ("lddy", 8),
        ("p", p), ("g", p), ("Gd", p), ("dX", p), ("lddx", 8)) + tail)
    big = 65535 * 64 + 1
    for fn, ptrs, lds, odd, has_slope, has_ws in (
            (score, ("rowptr", "X", "att", "hdr", "plan", "col", "val", "s"), ("ldx", ), "X", True, False),
            (fwd, ("rowptr", "X", "Y", "L", "hdr", "plan", "col", "val", "s"), ("ldx", "ldy"), "X", False, True),
            (edge, ("rowptr", "X", "att", "dY", "Y", "L", "Gd", "R", "hdr", "plan", "col", "val", "s", "g", "p"),
             ("ldx", "lddy", "ldy"), "X", True, True),
            (bwd, ("rowptr", "X", "att", "dY", "Gd", "dX", "hdr", "plan", "col", "val", "eid", "p", "g"), ("ldx", "lddy", "lddx"),
             "dY", True, True)):
        for name in ptrs:
            assert fn(**{name: None}) == E_ARG, name
        for name in lds:
            assert fn(**{name: 7}) == E_ARG, name
        assert fn(H=0) == E_ARG and fn(H=-8) == E_ARG
        assert fn(n_rows=3) == E_PLAN and b"plan does not match" in lib.glass_last_error_string()
        assert fn(n_rows=-1) == E_ARG
        assert fn(hdr=p) == E_PLAN
        assert fn(**{odd: p + 2}) == E_ARG and b"aligned" in lib.glass_last_error_string()
        assert fn(H=big, **{name: big for name in lds}) == E_UNSUPPORTED
        if has_ws:   # a plan with partial slots and no workspace
            assert fn(hdr=cut.ctypes.data, plan=cut.ctypes.data, n_rows=3) == E_ARG and b"ws is null" in lib.glass_last_error_string()
        if has_slope:
            assert fn(slope=float("nan")) == E_ARG and b"slope" in lib.glass_last_error_string()
        # no rows, or no entries: nothing is launched (the pointers here are host memory), and the call succeeds
        assert fn(hdr=none.ctypes.data, plan=none.ctypes.data) == 0
        assert fn(hdr=none.ctypes.data, plan=none.ctypes.data, col=None, val=None, s=None, g=None, p=None, eid=None) == 0
    datt = call(lib.glass_spmm_gatv2_datt_f32, (("R", p), ("datt", p), ("n_rows", 2), ("H", 8), ("ws", p), ("stream", None)))
    for name in ("R", "datt", "ws"):
        assert datt(**{name: None}) == E_ARG, name
    assert datt(H=0) == E_ARG and datt(n_rows=-1) == E_ARG and datt(H=big) == E_UNSUPPORTED
    assert datt(R=p + 2) == E_ARG and b"aligned" in lib.glass_last_error_string()
    assert datt(ws=p + 4) == E_ARG and b"8-byte" in lib.glass_last_error_string()
    assert datt(n_rows=0) == 0 and datt(n_rows=0, ws=None) == 0   # nothing to launch
