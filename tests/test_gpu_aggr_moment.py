"""K1v on the GPU: glass_spmm_moment_csr_f32 / _bwd_f32 (csrc/spmm_moment.hip) graded per element against the fp64 restatement
tests/aggr_moment_oracle.py of the same fp32 inputs, on every plan form and lane layout; the host objects
(graph.CSRAdj.moment_fwd / moment_bwd, ops.spmm_moments); a GLASS model with aggr "std" / "var" against an fp64 restatement of
the model; impl.train.train on the captured per-op step.

Bounds (aggr_moment_oracle.bounds / bound_dx), gamma(n) = n 2^-24 / (1 - n 2^-24), n_i the row's entry count:
  Wsum  gamma(n_i) W                     Mu   gamma(3 n_i + 4) sum w |x| / W
  Var   gamma(8 n_i + 8) (Var + sqrt(Var sum w x^2 / W))      Std  the Var bound / (2 Std64) + one ulp of Std64
  dX[j] gamma(n_j + 6) sum_e w (|C| + |A| |X - Mu|), on the kernel's own fp32 A / C / Mu / X
Each test prints the largest share of every bound it saw (holds the table)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import aggr_moment_oracle as MO
from aggr_max_oracle import MaxAdj
from helpers import rel_inf, flat_grads
from test_gpu_aggr_softmax import Guarded, _graph   # the graphs `mixed` and `all_long`, the guarded buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
EPS = 1e-5
WIDTHS = (4, 18, 64, 68, 128, 132, 256, 260)   # every VW / LPR case, two column tiles
DATA = ("normal", "offset", "equal", "mixed")
KINDS = ("std", "var")


def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _adj(kind):
    """(graph.CSRAdj on the device built for "std", the sorted CSR of the restatement as numpy arrays)"""
    from glass_amd import graph
    n, ei, ew = _graph(kind)
    adj = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "std")
    ref = MaxAdj(ei, ew.double(), n)
    return adj, {k: getattr(ref, k).numpy() for k in ("rowptr", "col", "val", "rowptr_t", "col_t", "val_t")}


def _data(name, n, H, seed):
    """(a) standard normal, (b) normal + 1000, (c) every source row equal, (d) magnitudes mixed over 1e-3 .. 50"""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, H, generator=g)
    if name == "offset":
        X = X + 1000.0
    elif name == "equal":
        X = X[:1].expand(n, H).contiguous() * 7.0 + 3.0
    elif name == "mixed":
        X = X * torch.pow(10.0, torch.rand(n, H, generator=g) * (np.log10(50.0) + 3.0) - 3.0)
    return X


# ---- raw entries on guarded buffers ----------------------------------------------------------------------------------------
def _raw_fwd(adj, Xv, kind, pad_s=0, pad_mu=0, off=0, ws=True):
    """glass_spmm_moment_csr_f32 -> (rc, S [n, ld] view, Mu view, Wsum, the Guarded buffers)"""
    L_, lib = _lib()
    op, (n, H) = adj.fwd, (adj.fwd.n_rows, Xv.shape[1])
    lds, ldmu = H + pad_s, H + pad_mu
    S, Mu = Guarded(n * lds, float("nan"), off=off), Guarded(n * ldmu, float("nan"), off=off)
    Ws = Guarded(n, float("nan"))
    nbytes = lib.glass_spmm_moment_ws_bytes(op.header.ctypes.data, H)
    assert nbytes == int(op.header[7]) * (2 * H + 1) * 4
    W = Guarded(max(nbytes // 4, 4), float("nan"))   # (need not be initialised: junk on purpose)
    rc = lib.glass_spmm_moment_csr_f32(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), Xv.data_ptr(), Xv.stride(0),
                                       EPS, MO_KIND[kind], S.t.data_ptr(), lds, Mu.t.data_ptr(), ldmu, Ws.t.data_ptr(), n, H,
                                       op.header.ctypes.data, op.plan.data_ptr(), W.t.data_ptr() if ws else None, _stream())
    torch.cuda.synchronize()
    return rc, S.t.view(n, lds), Mu.t.view(n, ldmu), Ws.t, (S, Mu, Ws, W)


def _raw_bwd(adj, Xv, Muv, Av, Cv, pad=0, off=0, ws=True):
    L_, lib = _lib()
    op, (n, H) = adj.bwd, (adj.bwd.n_rows, Xv.shape[1])
    lddx = H + pad
    D = Guarded(n * lddx, float("nan"), off=off)
    nbytes = lib.glass_spmm_moment_bwd_ws_bytes(op.header.ctypes.data, H)
    assert nbytes == int(op.header[7]) * H * 4
    W = Guarded(max(nbytes // 4, 4), float("nan"))
    rc = lib.glass_spmm_moment_bwd_f32(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), Xv.data_ptr(), Xv.stride(0),
                                       Muv.data_ptr(), Muv.stride(0), Av.data_ptr(), Av.stride(0),
                                       None if Cv is None else Cv.data_ptr(), 0 if Cv is None else Cv.stride(0), D.t.data_ptr(),
                                       lddx, n, H, op.header.ctypes.data, op.plan.data_ptr(), W.t.data_ptr() if ws else None,
                                       _stream())
    torch.cuda.synchronize()
    return rc, D.t.view(n, lddx), (D, W)


MO_KIND = {"std": 0, "var": 1}


def _share(err, bound):
    """the largest err / bound; where the bound is 0 the error must be 0 too"""
    assert (err[bound == 0] == 0).all(), "an error where the bound allows none"
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def _grade_fwd(ref, X, Sv, Muv, Wv, kind, m=None):
    """shares of the bounds of (Wsum, Mu, S) against fp64 on the same fp32 X; every element must keep its bound"""
    m = MO.moments(ref["rowptr"], ref["col"], ref["val"], X.double().numpy(), EPS) if m is None else m
    b = MO.bounds(m)
    S64, bS = (m["Std"], b["Std"]) if kind == "std" else (m["Var"], b["Var"])
    shares = {"Wsum": _share(np.abs(Wv.cpu().double().numpy() - m["W"]), b["W"]),
              "Mu": _share(np.abs(Muv.cpu().double().numpy() - m["Mu"]), b["Mu"]),
              "Std" if kind == "std" else "Var": _share(np.abs(Sv.cpu().double().numpy() - S64), bS)}
    return shares, m


def _grade_bwd(ref, X, Muv, Av, Cv, dXv):
    dX64, mass = MO.moments_bwd(ref["rowptr_t"], ref["col_t"], ref["val_t"], X.double().numpy(), Muv.cpu().double().numpy(),
                                Av.cpu().double().numpy(), None if Cv is None else Cv.cpu().double().numpy())
    return _share(np.abs(dXv.cpu().double().numpy() - dX64), MO.bound_dx(ref["rowptr_t"], mass))


def _merge(worst, shares):
    for k, v in shares.items():
        worst[k] = max(worst.get(k, 0.0), v)


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("graph_kind", ("mixed", "all_long"))
def test_values_per_element_and_repeatability(graph_kind, H):
    from glass_amd import ops
    L_, _ = _lib()
    adj, ref = _adj(graph_kind)
    n = adj.n_node
    empty = torch.from_numpy(np.nonzero(np.diff(ref["rowptr"]) == 0)[0]).to(DEV)
    assert len(empty) >= 1
    worst = {}
    for di, name in enumerate(DATA):
        X = _data(name, n, H, 1000 * H + 10 * di + (graph_kind == "mixed"))
        Xd = X.to(DEV)
        g = torch.Generator().manual_seed(77 + di)
        dS, dMu = torch.randn(n, H, generator=g).to(DEV), torch.randn(n, H, generator=g).to(DEV)
        m = None
        keep = {}
        for kind in KINDS:
            rc, Sv, Muv, Wv, guards = _raw_fwd(adj, Xd, kind)
            L_.check(rc, "glass_spmm_moment_csr_f32")
            assert all(g_.intact() for g_ in guards), (graph_kind, H, name, kind, "guards of S / Mu / Wsum / workspace")
            assert not bool(torch.isnan(Sv).any() | torch.isnan(Muv).any() | torch.isnan(Wv).any()), "every element is written"
            assert bool((Sv[empty] == 0).all()) and bool((Muv[empty] == 0).all()) and bool((Wv[empty] == 0).all()), "a row without entries"
            rc, S2, Mu2, W2, _g = _raw_fwd(adj, Xd, kind)
            assert torch.equal(_bits(Sv), _bits(S2)) and torch.equal(_bits(Muv), _bits(Mu2)) and torch.equal(_bits(Wv), _bits(W2)), \
                (graph_kind, H, name, kind, "two forward runs differ")
            shares, m = _grade_fwd(ref, X, Sv, Muv, Wv, kind, m)
            _merge(worst, shares)
            keep[kind] = (Muv, Wv)
            if name == "equal":   # no x^2, d = 0 at every merge: exactly no spread, bit for bit
                live = Wv > 0
                want = 0.0 if kind == "var" else float(np.sqrt(np.float32(np.float32(0.0) + np.float32(EPS))))
                assert bool((Sv[live] == want).all()) and bool((Muv[live] == Xd[0].expand(n, H)[live]).all()), (graph_kind, H, kind)
            # backward on the kernel's own results: with the mean's gradient and without
            for with_mu in (True, False):
                A, C = ops.moment_factors(kind, Sv, Wv, dS, dMu if with_mu else None)
                assert (C is None) != with_mu and not bool(A[empty].any())
                rc, dXv, guards = _raw_bwd(adj, Xd, Muv, A, C)
                L_.check(rc, "glass_spmm_moment_bwd_f32")
                assert all(g_.intact() for g_ in guards) and not bool(torch.isnan(dXv).any()), (graph_kind, H, name, kind, with_mu)
                rc, dX2, _g = _raw_bwd(adj, Xd, Muv, A, C)
                assert torch.equal(_bits(dXv), _bits(dX2)), (graph_kind, H, name, kind, "two backward runs differ")
                _merge(worst, {"dX": _grade_bwd(ref, X, Muv, A, C, dXv)})
        # the mean and the weight sums do not depend on the kind
        assert torch.equal(_bits(keep["std"][0]), _bits(keep["var"][0])) and torch.equal(_bits(keep["std"][1]), _bits(keep["var"][1]))
    print(f"K1v shares {graph_kind} H={H}: " + " ".join(f"{k} {worst[k]:.3f}" for k in ("Wsum", "Mu", "Var", "Std", "dX")))
    assert all(v <= 1.0 for v in worst.values()), (graph_kind, H, worst)


@pytest.mark.parametrize("H,pads,off", [(64, (8, 4, 12, 4), 0), (64, (3, 1, 2, 5), 0), (18, (2, 6, 1, 3), 0), (64, (0, 0, 0, 0), 1),
                                        (64, (4, 4, 4, 4), 3)])
def test_strided_and_unaligned_operands(H, pads, off):
    """X, S, Mu, A, C and dX as column slices of wider buffers (multiples of 4 keep the 16-byte form, anything else takes the
    scalar one), and every operand `off` floats past a 16-byte boundary (the scalar form at a width that has a vector one);
    the columns beyond H are neither read (NaN) nor written."""
    from glass_amd import ops
    L_, _ = _lib()
    adj, ref = _adj("mixed")
    n = adj.n_node
    px, ps, pm, pd = pads
    X = _data("normal", n, H, 5)
    g = torch.Generator().manual_seed(6)
    dS, dMu = torch.randn(n, H, generator=g).to(DEV), torch.randn(n, H, generator=g).to(DEV)

    def wide(src, pad):
        buf = torch.full((n * (H + pad) + off + 4, ), float("nan"), device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + n * (H + pad)].view(n, H + pad)
        v[:, :H] = src.to(DEV)
        return v[:, :H]
    Xv = wide(X, px)
    assert Xv.data_ptr() % 16 == 4 * off
    worst = {}
    for kind in KINDS:
        rc, Sv, Muv, Wv, guards = _raw_fwd(adj, Xv, kind, ps, pm, off)
        L_.check(rc, "glass_spmm_moment_csr_f32")
        assert bool(torch.isnan(Sv[:, H:]).all()) and bool(torch.isnan(Muv[:, H:]).all()) and all(g_.intact() for g_ in guards)
        shares, _m = _grade_fwd(ref, X, Sv[:, :H], Muv[:, :H], Wv, kind)
        _merge(worst, shares)
        A, C = ops.moment_factors(kind, Sv[:, :H], Wv, dS, dMu)
        Av, Cv = wide(A, ps), wide(C, pm)
        for Cuse in (Cv, None):
            rc, dXv, guards = _raw_bwd(adj, Xv, Muv[:, :H], Av, Cuse, pd, off)
            L_.check(rc, "glass_spmm_moment_bwd_f32")
            assert bool(torch.isnan(dXv[:, H:]).all()) and all(g_.intact() for g_ in guards)
            _merge(worst, {"dX": _grade_bwd(ref, X, Muv[:, :H], Av, Cuse, dXv[:, :H])})
    print(f"K1v shares strided H={H} pads {pads} off {off}: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_refusals_on_the_device_and_a_call_without_rows():
    import ctypes
    from glass_amd import graph
    L_, lib = _lib()
    adj, ref = _adj("mixed")
    n, H = adj.n_node, 8
    Xd = _data("normal", n, H, 1).to(DEV)
    # partial slots and no workspace: refused before any launch, nothing written
    assert int(adj.fwd.header[7]) > 0 and int(adj.bwd.header[7]) > 0
    rc, Sv, Muv, Wv, guards = _raw_fwd(adj, Xd, "std", ws=False)
    assert rc == -1 and b"ws is null" in lib.glass_last_error_string()
    assert all(g_.intact() for g_ in guards) and bool(torch.isnan(Sv).all()) and bool(torch.isnan(Muv).all()) and bool(torch.isnan(Wv).all())
    rc, dXv, guards = _raw_bwd(adj, Xd, Xd, Xd, None, ws=False)
    assert rc == -1 and b"ws is null" in lib.glass_last_error_string() and bool(torch.isnan(dXv).all())
    # n_rows == 0: 0 without a launch
    rp = np.zeros(1, dtype=np.int32)
    words = ctypes.c_int64(0)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, 0, None, ctypes.byref(words)) == 0
    plan = np.zeros(words.value, dtype=np.int32)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, 0, plan.ctypes.data, ctypes.byref(words)) == 0
    pd = torch.from_numpy(plan).to(DEV)
    rpd = torch.zeros(1, dtype=torch.int32, device=DEV)
    bufs = [Guarded(4 * H, float("nan")) for _ in range(6)]
    x, s, mu, w, a, dx = (b.t.data_ptr() for b in bufs)
    h, st = plan.ctypes.data, _stream()
    assert lib.glass_spmm_moment_csr_f32(rpd.data_ptr(), None, None, x, H, EPS, 0, s, H, mu, H, w, 0, H, h, pd.data_ptr(), None, st) == 0
    assert lib.glass_spmm_moment_bwd_f32(rpd.data_ptr(), None, None, x, H, mu, H, a, H, None, 0, dx, H, 0, H, h, pd.data_ptr(),
                                         None, st) == 0
    torch.cuda.synchronize()
    assert all(b.intact() and bool(torch.isnan(b.t).all()) for b in bufs)
    # weights are multiplicities
    n2, ei, ew = _graph("all_long")
    for bad in (0.0, -1.0, float("nan")):
        wbad = ew.clone()
        wbad[3] = bad
        with pytest.raises(ValueError, match="strictly positive"):
            graph.CSRAdj(ei.to(DEV), wbad.to(DEV), n2, "var")
    with pytest.raises(NotImplementedError):
        graph.CSRAdj(ei.to(DEV), ew.to(DEV), n2, "min")


@pytest.mark.parametrize("kind", KINDS)
def test_autograd_binding(kind, monkeypatch):
    from glass_amd import graph, ops
    L_, _ = _lib()
    n, ei, ew = _graph("mixed")
    adj = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, kind)   # (its own: the workspace cache is looked at below)
    H = 20
    X = _data("normal", n, H, 3)
    g = torch.Generator().manual_seed(4)
    dS, dMu = torch.randn(n, H, generator=g), torch.randn(n, H, generator=g)
    calls = []
    real = graph.CSRAdj.moment_bwd
    monkeypatch.setattr(graph.CSRAdj, "moment_bwd", lambda self, x, mu, A, C=None: (calls.append(C is not None), real(self, x, mu, A, C))[1])
    # under no_grad, and with an operand that needs no gradient: no backward, its workspace is never made
    with torch.no_grad():
        S0, Mu0 = ops.spmm_moments(adj, X.to(DEV), kind, EPS)
    S1, Mu1 = ops.spmm_moments(adj, X.to(DEV), kind, EPS)
    assert S0.grad_fn is None and S1.grad_fn is None and calls == []
    assert not any(k[0] == "moment_bwd" for k in adj._aggr_ws) and any(k[0] == "moment_fwd" for k in adj._aggr_ws)
    # the raw entry's bits
    rc, Sv, Muv, Wv, _g = _raw_fwd(adj, X.to(DEV), kind)
    L_.check(rc, "glass_spmm_moment_csr_f32")
    for a in (S0, S1):
        assert torch.equal(_bits(a), _bits(Sv))
    for a in (Mu0, Mu1):
        assert torch.equal(_bits(a), _bits(Muv))
    # fp64 autograd on the same data
    X64 = X.double().requires_grad_(True)
    S64, Mu64 = MO.scatter_moments(ei, ew.double(), n, X64, kind, EPS)
    (dX_s, ) = torch.autograd.grad(S64, X64, dS.double(), retain_graph=True)
    (dX_sm, ) = torch.autograd.grad((S64, Mu64), X64, (dS.double(), dMu.double()))
    Xd = X.to(DEV).requires_grad_(True)
    S, Mu = ops.spmm_moments(adj, Xd, kind, EPS)
    assert torch.equal(_bits(S.detach()), _bits(Sv)) and torch.equal(_bits(Mu.detach()), _bits(Muv))
    (got_s, ) = torch.autograd.grad(S, Xd, dS.to(DEV), retain_graph=True)
    assert calls == [False], "C is passed only when Mu's gradient is asked for"
    (got_sm, ) = torch.autograd.grad((S, Mu), Xd, (dS.to(DEV), dMu.to(DEV)))
    assert calls == [False, True] and any(k[0] == "moment_bwd" for k in adj._aggr_ws)
    e_s, e_sm = rel_inf(got_s.cpu(), dX_s), rel_inf(got_sm.cpu(), dX_sm)
    print(f"{kind}: autograd dX through S {e_s:.2e}, through S and Mu {e_sm:.2e}; S {rel_inf(S.detach().cpu(), S64.detach()):.2e}")
    assert e_s <= TOL and e_sm <= TOL
    with pytest.raises(L_.GlassHipError, match="spmm_moments"):
        ops.spmm(adj, X.to(DEV))
    with pytest.raises(L_.GlassHipError, match=f"replicated {kind} aggregation is not built"):
        ops.spmm_rep(adj, torch.zeros(2 * n, H, device=DEV), 2)
    mean = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "mean")
    with pytest.raises(L_.GlassHipError, match="not 'std' or 'var'"):
        ops.spmm_moments(mean, X.to(DEV))
    with pytest.raises(L_.GlassHipError, match="not 'std' or 'var'"):
        mean.moment_fwd(X.to(DEV), "std")


# ---- through the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", ("sum", "mean"))
@pytest.mark.parametrize("aggr", KINDS)
@pytest.mark.parametrize("hidden", (64, 8))
def test_model_against_the_fp64_restatement(hidden, aggr, pool):
    """Two GLASSConv layers on the 200-node graph with six subgraphs of tests/test_gpu_edge_saliency.py: the fp64 side is
    OracleGLASS(aggr "sum") whose conv.adj are MomentAdj — the aggregation from plain torch ops, differentiated by autograd."""
    from helpers import build_glass
    from impl import utils
    from oracle import glass_oracle as O
    from test_gpu_edge_saliency import _graph as small_graph, N, K
    x, ei, ew, pos, y = small_graph()
    torch.manual_seed(5)
    model = build_glass(hidden, 2, int(x.max()), K, aggr, pool, 0.8, dropout=0.0, jk=True)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    orc = O.OracleGLASS(hidden, 2, int(x.max()), K, aggr="sum", pool=pool, z_ratio=0.8).double()
    orc.load_state_dict(sd)
    orc.train()
    for conv in orc.conv.convs:
        conv.adj = MO.MomentAdj(ei, ew.double(), N, aggr, EPS)
    logits_ref = orc(x, ei, ew.double(), pos, O.max_zero_one(x, pos))
    loss_ref = nn.CrossEntropyLoss()(logits_ref, y)
    loss_ref.backward()
    grads_ref = {k: p.grad.clone() for k, p in orc.named_parameters()}

    model.to(DEV).train()
    xg, eig, ewg, posg, yg = (a.to(DEV) for a in (x, ei, ew, pos, y))
    logits = model(xg, eig, ewg, posg, utils.MaxZOZ(xg, posg), id=0)
    loss = nn.CrossEntropyLoss()(logits, yg)
    loss.backward()
    torch.cuda.synchronize()
    assert all(c.adj.aggr == aggr for c in model.conv.convs)
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    keys = sorted(grads_ref)
    assert set(keys) == set(mine)
    e_logits = rel_inf(logits.detach().cpu(), logits_ref.detach())
    e_loss = abs(loss.item() - loss_ref.item()) / abs(loss_ref.item())
    e_grad = rel_inf(flat_grads(mine, keys), flat_grads(grads_ref, keys))
    print(f"hidden {hidden} {aggr} pool {pool}: loss {e_loss:.2e} logits {e_logits:.2e} flat gradient {e_grad:.2e}")
    assert e_loss <= TOL and e_logits <= TOL and e_grad <= TOL


@pytest.mark.parametrize("aggr", KINDS)
def test_training_on_the_captured_per_op_step(aggr):
    """Three steps of impl.train.train (one batch an epoch): the TrainStep is captured and reports the per-op form (the stack
    program does not serve std / var); the losses are finite, fall, and are the same bits on a second run from the same
    start."""
    from helpers import build_glass
    from impl import SubGDataset, config, train, utils
    from glass_amd import stack, synth
    config.set_device(0)
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=2, n_batches=1)
    x, ei, ew, pos, y = (torch.from_numpy(a).to(DEV) for a in (x, ei, ew, pos, y))
    torch.manual_seed(3)
    gnn = build_glass(64, 2, int(x.max()), w.n_class, aggr, w.pool, w.z_ratio).to(DEV)
    twin = copy.deepcopy(gnn)
    loss_fn = nn.CrossEntropyLoss()
    ds = SubGDataset.GDataset(x, ei, ew, pos, y)
    loader = lambda: SubGDataset.ZGDataloader(ds, w.batch, z_fn=utils.MaxZOZ, shuffle=False, drop_last=True)
    out = []
    for net in (gnn, twin):
        opt = torch.optim.Adam(net.parameters(), lr=5e-3)
        out.append([train.train(opt, net, loader(), loss_fn) for _ in range(3)])
        steps = net.__dict__.get("_glass_train_steps") or {}
        assert len(steps) == 1
        step = next(iter(steps.values()))
        net.train()
        assert step.graphed and not step._program_step() and not stack.step_supported(net, loss_fn)
        assert not stack.StackProgram.supported(net.conv) and all(c.adj.aggr == aggr for c in net.conv.convs)
    print(f"{aggr}: losses {out[0]}")
    assert np.isfinite(out[0]).all() and out[0][0] > out[0][1] > out[0][2]
    assert np.array_equal(np.float32(out[0]).view(np.int32), np.float32(out[1]).view(np.int32)), out
