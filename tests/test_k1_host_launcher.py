"""The host side of K1 (glass_amd/graph.py): the one workspace cache and the one launcher of the CSR entries.  The cache and the
launcher's argument count are checked on CPU tensors; that a repeated call through the public path launches on the SAME
workspaces — what a captured graph relies on, and what no value test looks at — is checked on the GPU."""
import ctypes
import types

import numpy as np
import pytest
import torch

DEV = "cuda:0"


@pytest.fixture
def branch0():
    from glass_amd import graph
    yield graph
    graph.set_workspace_branch(0)


def test_workspace_cache_grows_retires_and_keeps_pointers(branch0):
    graph = branch0
    from glass_amd import _lib
    ws = graph._Workspaces("cpu")
    a = ws.fetch("e", (64, ), 1000)
    assert a.numel() * a.element_size() >= 1000 and a.data_ptr() % 8 == 0
    assert ws.fetch("e", (64, ), 1000) is a and ws.fetch("e", (64, ), 8).data_ptr() == a.data_ptr(), "a request that fits: the same tensor"
    assert ws.retired == [] and len(ws) == 1
    # a larger request: a new tensor; the old one is kept, alive, in the retired list
    a.fill_(7.0)
    b = ws.fetch("e", (64, ), 1001)
    assert b is not a and b.data_ptr() != a.data_ptr() and b.numel() * b.element_size() >= 1001
    assert len(ws.retired) == 1 and ws.retired[0] is a and bool((a == 7.0).all()) and len(ws) == 1
    assert ws.fetch("e", (64, ), 1000) is b, "the grown buffer serves the smaller request from now on"
    # another branch: another tensor; back on branch 0 the first one again
    graph.set_workspace_branch(3)
    c = ws.fetch("e", (64, ), 1001)
    assert c.data_ptr() != b.data_ptr()
    graph.set_workspace_branch(0)
    assert ws.fetch("e", (64, ), 1001) is b
    # (H, K) and H do not alias, nor do two entries at one width
    d, e = ws.fetch("e", (64, 4), 1001), ws.fetch("f", (64, ), 1001)
    assert len({t.data_ptr() for t in (b, c, d, e)}) == 4 and len(ws.retired) == 1
    # a query that refused the header; a plan without cut rows
    with pytest.raises(_lib.GlassHipError, match="bad plan header"):
        ws.fetch("e", (64, ), -2)
    z = ws.fetch("g", (64, ), 0)
    assert z.numel() * z.element_size() >= 16 and z.data_ptr() % 8 == 0


def _cpu_operand(rowptr):
    """what _launch reads of a CSROperand, on CPU tensors, with the library's own plan for `rowptr`"""
    from glass_amd import graph, _lib
    lib = _lib.load()
    rp = np.asarray(rowptr, dtype=np.int32)
    n = rp.shape[0] - 1
    words = ctypes.c_int64(0)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, n, None, ctypes.byref(words)) == 0
    plan = np.zeros(words.value, dtype=np.int32)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, n, plan.ctypes.data, ctypes.byref(words)) == 0
    nnz = int(rp[-1])
    header = plan[:_lib.PLAN_HEADER_WORDS].copy()
    return types.SimpleNamespace(rowptr=torch.from_numpy(rp), col=torch.zeros(nnz, dtype=torch.int32), val=torch.ones(nnz),
                                 n_rows=n, header=header, plan=torch.from_numpy(plan),
                                 _ws=graph._Workspaces("cpu"))


@pytest.mark.parametrize("off", [+1, -1])
def test_launcher_refuses_a_call_whose_argument_count_is_not_the_entrys(off, monkeypatch):
    from glass_amd import graph, _lib
    lib = _lib.load()
    op = _cpu_operand([0, 3, 3, 5000])   # (one row is cut: the workspace query answers > 0)
    assert op.header[7] > 0
    calls = []

    class Stub:   # an entry that takes one argument more (fewer) than the launcher passes
        argtypes = [ctypes.c_void_p] * (len(_lib.SIGNATURES["glass_spmm_csr_f32"][1]) + off)

        def __call__(self, *args):
            calls.append(args)
            return 0
    monkeypatch.setattr(lib, "glass_spmm_csr_f32", Stub())
    monkeypatch.setitem(_lib.SIGNATURES, "glass_spmm_csr_f32", (ctypes.c_int, Stub.argtypes))   # (as load() would have read it)
    with pytest.raises(_lib.GlassHipError, match=rf"glass_spmm_csr_f32.* 13 .* {13 + off}\b"):
        graph._launch(op, op._ws, "spmm", "glass_spmm_csr_f32", "glass_spmm_ws_bytes", (0, 8, 0, 8), 8)
    assert calls == []
    ((key, ws), ) = op._ws.items()
    assert key == ("spmm", (8, ), 0) and ws.numel() * 8 >= int(op.header[7]) * 8 * 4


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
def test_a_copied_operand_passes_its_own_headers_address(how, monkeypatch):
    """copy.deepcopy(model) copies the adjacencies, and an operand may be pickled: every launch and size query of the copy reads
    the COPY's header array, wherever the original's went."""
    import copy
    import gc
    import pickle
    from glass_amd import graph, _lib
    lib = _lib.load()
    rp = torch.tensor([0, 3, 3, 5000], dtype=torch.int32)
    op0 = graph.CSROperand(rp, torch.zeros(5000, dtype=torch.int32), torch.ones(5000), 3, 3)
    addr0, words = op0.header.ctypes.data, op0.header.copy()
    op = copy.deepcopy(op0) if how == "deepcopy" else pickle.loads(pickle.dumps(op0))
    assert op.header is not op0.header and op.header.ctypes.data != addr0 and np.array_equal(op.header, words)
    op0.header[:] = -1   # what freed memory may hold
    del op0
    gc.collect()
    seen = []

    class Entry:
        def __call__(self, *args):
            seen.append(args)
            return 0

    class Query:
        def __call__(self, hdr, H):
            seen.append((hdr, H))
            return real_query(hdr, H)
    real_query = lib.glass_spmm_ws_bytes
    monkeypatch.setattr(lib, "glass_spmm_csr_f32", Entry())
    monkeypatch.setattr(lib, "glass_spmm_ws_bytes", Query())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: types.SimpleNamespace(cuda_stream=0))
    ws = graph._launch(op, op._ws, "spmm", "glass_spmm_csr_f32", "glass_spmm_ws_bytes", (0, 8, 0, 8), 8)
    (q_hdr, _H), args = seen
    assert q_hdr == args[-4] == op.header.ctypes.data and args[-2] == ws.data_ptr() and args[-3] == op.plan.data_ptr()
    assert ws.numel() * 8 >= int(words[7]) * 8 * 4 > 0 and op.workspace(8) is ws


# ---- GPU: a second call launches on the first call's workspaces ----------------------------------------------------------------
def _hub_graph(n=700, spokes=640):
    """node 0 joined to 1 .. spokes in both directions, a ring through 1 .. n - 2, node n - 1 isolated"""
    ring = torch.arange(1, n - 1)
    nxt = torch.roll(ring, -1)
    hub = torch.arange(1, spokes + 1)
    zero = torch.zeros_like(hub)
    src = torch.cat([zero, hub, ring, nxt])
    dst = torch.cat([hub, zero, nxt, ring])
    ew = 0.5 + torch.rand(src.shape[0], generator=torch.Generator().manual_seed(0))
    return n, torch.stack([src, dst]), ew


def _cache_state(adj):
    caches = {"fwd": adj.fwd._ws, "bwd": adj.bwd._ws, "aggr": getattr(adj, "_aggr_ws", {})}
    live = {(owner, ) + k: t.data_ptr() for owner, c in caches.items() for k, t in c.items()}
    return live, sum(len(getattr(c, "retired", ())) for c in caches.values())


@pytest.mark.gpu
def test_a_repeated_call_launches_on_the_same_workspaces():
    from glass_amd import graph, ops
    n, ei, ew = _hub_graph()
    H = 64
    g = torch.Generator().manual_seed(1)
    X, dY = torch.randn(n, H, generator=g).to(DEV), torch.randn(n, H, generator=g).to(DEV)
    t = torch.tensor([0.7], device=DEV, requires_grad=True)
    att = [(0.3 * torch.randn(H, generator=g)).to(DEV).requires_grad_(True) for _ in range(2)]
    calls = {"sum": lambda adj, x: (ops.spmm(adj, x), ()),
             "max": lambda adj, x: (ops.spmm(adj, x), ()),
             "softmax": lambda adj, x: (ops.spmm_softmax(adj, x, t), (t, )),
             "gat": lambda adj, x: (ops.spmm_gat(adj, x, att[0], att[1], 0.2), tuple(att)),
             "gat4": lambda adj, x: (ops.spmm_gat(adj, x, att[0], att[1], 0.2, heads=4), tuple(att)),
             "std": lambda adj, x: (sum(ops.spmm_moments(adj, x, "std")), ()),
             "pna": lambda adj, x: (sum(ops.spmm_pna(adj, x)), ())}

    def once(adj, name):
        x = X.clone().requires_grad_(True)
        y, params = calls[name](adj, x)
        return (y.detach(), ) + torch.autograd.grad(y, (x, ) + params, dY)
    adjs = {}
    for name in ("sum", "max", "softmax", "gat", "std", "pna"):
        adj = adjs[name] = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, name)
        assert int(adj.fwd.header[7]) > 0 and int(adj.bwd.header[7]) > 0, "H_NSLOTS: both plans write their workspace"
        first = once(adj, name)
        state = _cache_state(adj)
        assert state[0] and state[1] == 0
        again = once(adj, name)
        assert _cache_state(adj) == state, f"{name}: the second call made or replaced a workspace"
        for a, b in zip(first, again):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    # several heads: buffers of their own, next to the single head's, which stay where they are
    adj = adjs["gat"]
    one_head = _cache_state(adj)
    first = once(adj, "gat4")
    state = _cache_state(adj)
    again = once(adj, "gat4")
    assert _cache_state(adj) == state and state[1] == 0
    for a, b in zip(first, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    mh = {k: p for k, p in state[0].items() if k[2] == (H, 4)}
    assert mh and all(state[0][k] == p for k, p in one_head[0].items()) and set(mh) | set(one_head[0]) == set(state[0])
    assert not set(mh.values()) & set(one_head[0].values()) and {k[1] for k in mh} >= {"gat_fwd", "gat_edge", "gat_bwd", "gat_datt"}
