"""Max neighbour aggregation without a GPU: the restatement tests/aggr_max_oracle.py against torch's own scatter-max and
fp64 autograd, its tie and empty-row rules against hand-written expectations, the argument codes of the new exports (validation
runs before any HIP call), and the driver flag."""
import numpy as np
import pytest
import torch

import aggr_max_oracle as MO


def _graph(seed, n, nnz):
    g = torch.Generator().manual_seed(seed)
    ei = torch.stack((torch.randint(0, n - 2, (nnz, ), generator=g), torch.randint(0, n, (nnz, ), generator=g)))  # rows n-2, n-1: empty
    ew = torch.rand(nnz, generator=g, dtype=torch.float64) * 3 - 1.5   # negative and non-unit weights
    return ei, ew


def test_restatement_equals_scatter_amax_and_fp64_autograd_on_tie_free_inputs():
    n, nnz, H = 40, 300, 7
    ei, ew = _graph(0, n, nnz)
    g = torch.Generator().manual_seed(1)
    X = torch.randn(n, H, generator=g, dtype=torch.float64, requires_grad=True)
    adj = MO.MaxAdj(ei, ew, n)
    Y = adj @ X
    # torch: the products of the edge list (any order), scatter amax without the initial value, empty rows stay 0
    P = ew[:, None] * X[ei[1]]
    want = torch.zeros(n, H, dtype=torch.float64).scatter_reduce(0, ei[0][:, None].expand(nnz, H), P, "amax", include_self=False)
    assert MO.smallest_gap(adj, X.detach()) > 0, "the inputs hold a tie"
    assert torch.equal(Y.detach(), want.detach())
    dY = torch.randn(n, H, generator=g, dtype=torch.float64)
    (dX, ) = torch.autograd.grad(Y, X, dY)
    (dX_want, ) = torch.autograd.grad(want, X, dY)
    assert float((dX - dX_want).abs().max()) <= 1e-12 * float(dX_want.abs().max())
    assert bool((Y.detach()[n - 2:] == 0).all()) and bool((adj.last_arg[n - 2:] == -1).all())
    # arg names an entry of the right row whose product is the output
    rowptr, col, val = adj.rowptr, adj.col, adj.val
    rows = MO.rows_of(rowptr)
    a = adj.last_arg[:n - 2].to(torch.int64)
    live = (rowptr[1:] - rowptr[:-1])[:n - 2] > 0
    assert bool((rows[a[live]] == torch.arange(n - 2)[live][:, None]).all())
    assert torch.equal((val[a[live]] * X.detach()[col[a[live]], torch.arange(H)]), Y.detach()[:n - 2][live])


def test_tie_and_empty_row_rules():
    # row 0: entries 0, 1, 2 from sources 1, 2, 2 (a duplicate pair); row 1: empty; row 2: entries 3, 4 from sources 0, 1
    ei = torch.tensor([[0, 0, 0, 2, 2], [2, 1, 2, 1, 0]])
    ew = torch.tensor([1.0, 1.0, 2.0, -1.0, 1.0])
    #                      c0    c1     c2    c3
    X = torch.tensor([[0.0, -3.0, 5.0, -0.0],    # source 0
                      [2.0, -1.0, 1.0, 0.0],     # source 1
                      [2.0, -1.0, 0.5, 7.0]])    # source 2
    adj = MO.MaxAdj(ei, ew, 3)
    assert adj.col.tolist() == [1, 2, 2, 0, 1] and adj.val.tolist() == [1.0, 1.0, 2.0, 1.0, -1.0]  # sorted by (row, col), stable
    Y, arg = MO.max_aggregate(adj.rowptr, adj.col, adj.val, X)
    # row 0: products e0 = (2, -1, 1, 0), e1 = (2, -1, .5, 7), e2 = (4, -2, 1, 14): c1 ties e0 / e1 -> e0, c2 ties e0 / e2 -> e0
    # row 2: products e3 = (0, -3, 5, -0), e4 = (-2, 1, -1, -0): c3 ties -0.0 / -0.0 -> e3
    assert Y.tolist() == [[4.0, -1.0, 1.0, 14.0], [0.0, 0.0, 0.0, 0.0], [0.0, 1.0, 5.0, -0.0]]
    assert arg.tolist() == [[2, 0, 0, 2], [-1, -1, -1, -1], [3, 4, 3, 3]] and arg.dtype == torch.int32
    # +0.0 against -0.0: equal, the smaller e wins and its sign is kept
    X2 = torch.tensor([[0.0], [-0.0], [1.0]])
    ei2, ew2 = torch.tensor([[0, 0, 1, 1], [0, 1, 1, 0]]), torch.ones(4)
    adj2 = MO.MaxAdj(ei2, ew2, 3)
    Y2, arg2 = MO.max_aggregate(adj2.rowptr, adj2.col, adj2.val, X2)
    assert arg2.reshape(-1).tolist() == [0, 2, -1] and Y2.reshape(-1).tolist() == [0.0, 0.0, 0.0]
    assert not bool(torch.signbit(Y2[0, 0])) and not bool(torch.signbit(Y2[1, 0]))
    adj3 = MO.MaxAdj(ei2, torch.tensor([-1.0, -1.0, 1.0, 1.0]), 3)   # row 0: -0.0 (e0) against +0.0 (e1) -> e0, Y = -0.0
    Y3, arg3 = MO.max_aggregate(adj3.rowptr, adj3.col, adj3.val, X2)
    assert arg3[0, 0] == 0 and bool(torch.signbit(Y3[0, 0]))
    # backward: the winner alone receives val * dY; a source that never wins receives exactly 0
    dY = torch.tensor([[1.0, 10.0, 100.0, 1000.0], [5.0, 5.0, 5.0, 5.0], [2.0, 20.0, 200.0, 2000.0]])
    dX = MO.max_aggregate_bwd(adj.rowptr_t, adj.col_t, adj.val_t, adj.eid_t, dY, arg)
    assert adj.eid_t.tolist() == [3, 0, 4, 1, 2] and adj.col_t.tolist() == [2, 0, 2, 0, 0]
    assert dX.tolist() == [[2.0, 0.0, 200.0, 2000.0], [0.0, 10.0 - 20.0, 100.0, 0.0], [2.0, 0.0, 0.0, 2000.0]]


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
    x = np.zeros(64, dtype=np.float32)
    p, h = x.ctypes.data, plan.ctypes.data
    assert int(cut[7]) >= 2
    assert lib.glass_spmm_max_ws_bytes(cut.ctypes.data, 12) == int(cut[7]) * 12 * 8
    assert lib.glass_spmm_max_bwd_ws_bytes(cut.ctypes.data, 12) == int(cut[7]) * 12 * 4
    assert lib.glass_spmm_max_ws_bytes(h, 64) == 0 and lib.glass_spmm_max_bwd_ws_bytes(h, 64) == 0
    assert lib.glass_spmm_max_ws_bytes(p, 64) == E_PLAN and lib.glass_spmm_max_bwd_ws_bytes(None, 64) == E_PLAN
    assert lib.glass_spmm_max_ws_bytes(h, 0) == E_ARG and lib.glass_spmm_max_bwd_ws_bytes(h, -4) == E_ARG
    fwd = lambda **k: lib.glass_spmm_max_csr_f32(*[k.get(n, d) for n, d in (
        ("rowptr", h), ("col", h), ("val", p), ("X", p), ("ldx", 8), ("Y", p), ("ldy", 8), ("arg", h), ("ldarg", 8), ("n_rows", 2),
        ("H", 8), ("hdr", h), ("plan", h), ("ws", None), ("stream", None))])
    bwd = lambda **k: lib.glass_spmm_max_bwd_f32(*[k.get(n, d) for n, d in (
        ("rowptr", h), ("col", h), ("val", p), ("eid", h), ("dY", p), ("ldy", 8), ("arg", h), ("ldarg", 8), ("dX", p), ("ldx", 8),
        ("n_rows", 2), ("H", 8), ("hdr", h), ("plan", h), ("ws", None), ("stream", None))])
    for call, ptrs in ((fwd, ("rowptr", "X", "Y", "arg", "hdr", "plan", "col", "val")),
                       (bwd, ("rowptr", "dY", "arg", "dX", "hdr", "plan", "col", "val", "eid"))):
        for name in ptrs:
            assert call(**{name: None}) == E_ARG, name
        for name in ("ldx", "ldy", "ldarg"):
            assert call(**{name: 7}) == E_ARG, name
        assert call(H=0) == E_ARG
        assert call(n_rows=3) == E_PLAN and b"plan does not match" in lib.glass_last_error_string()
        assert call(hdr=p) == E_PLAN
        assert call(**{ptrs[1]: p + 2}) == E_ARG and b"aligned" in lib.glass_last_error_string()
        big = 65535 * 64 + 1
        assert call(H=big, ldx=big, ldy=big, ldarg=big) == E_UNSUPPORTED
        # a plan with partial slots and no workspace
        assert call(hdr=cut.ctypes.data, plan=cut.ctypes.data, n_rows=3) == E_ARG and b"ws is null" in lib.glass_last_error_string()


def test_names_are_accepted_where_the_aggregation_is_chosen():
    import GLASSTest
    assert GLASSTest.parse_args(["--use_one"]).aggr is None
    for a in ("mean", "sum", "gcn", "max"):
        assert GLASSTest.parse_args(["--use_one", "--aggr", a]).aggr == a
    with pytest.raises(SystemExit):
        GLASSTest.parse_args(["--use_one", "--aggr", "min"])
    # the host side refuses before it touches a device: an unknown name as the reference does, a CPU graph loudly
    from glass_amd import graph, _lib
    ei, ew = torch.tensor([[0, 1], [1, 0]]), torch.ones(2)
    with pytest.raises(NotImplementedError):
        graph.CSRAdj(ei, ew, 2, "min")
    with pytest.raises(_lib.GlassHipError, match="GPU only"):
        graph.CSRAdj(ei, ew, 2, "max")
