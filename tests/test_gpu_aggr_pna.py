"""K1p on the GPU: glass_spmm_pna_csr_f32 / _bwd_f32 (csrc/spmm_pna.hip) graded per element against the fp64 restatement
tests/aggr_pna_oracle.py of the same fp32 inputs, on every plan form and lane layout; the host objects (graph.CSRAdj.pna_fwd /
pna_bwd, ops.spmm_pna, ops.pna_mix); a GLASS model with aggr "pna" against an fp64 restatement of the model; impl.train.train on
the captured per-op step.

Mx, Mn, amx and amn are compared BIT FOR BIT: no product, no rounding, the winner of equal values fixed by rule.  Bounds of the
rest (aggr_moment_oracle.bounds, K1v's: the merge arithmetic is the same; aggr_pna_oracle.bound_dx), gamma(n) = n 2^-24 /
(1 - n 2^-24), n_i the row's entry count:
  Wsum  gamma(n_i) W                     Mu   gamma(3 n_i + 4) sum w |x| / W
  S     gamma(8 n_i + 8) (Var + sqrt(Var sum w x^2 / W)) / (2 S64) + one ulp of S64
  dX[j] gamma(n_j + 8) sum_t [w (|C| + |A| |X - Mu|) + hit_mx |Gmx| + hit_mn |Gmn|], on the kernel's own fp32 A / C / Mu / X / G
Each test prints the largest share of every bound it saw (holds the table)."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import aggr_moment_oracle as MO
import aggr_pna_oracle as PO
from aggr_max_oracle import MaxAdj
from helpers import rel_inf, flat_grads
from test_gpu_aggr_softmax import Guarded, _graph   # the graphs `mixed` and `all_long`, the guarded buffers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
EPS = 1e-5
WIDTHS = (4, 18, 64, 68, 128, 132, 256, 260)   # every VW / LPR case, two column tiles
DATA = ("normal", "offset", "equal", "ties")


def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _adj(kind):
    """(graph.CSRAdj on the device built for "pna", the sorted CSR of the restatement as numpy arrays)"""
    from glass_amd import graph
    n, ei, ew = _graph(kind)
    adj = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "pna")
    ref = MaxAdj(ei, ew.double(), n)
    return adj, {k: getattr(ref, k).numpy() for k in ("rowptr", "col", "val", "rowptr_t", "col_t", "val_t", "eid_t")}


def _data(name, n, H, seed):
    """(a) standard normal, (b) normal + 1000, (c) every source row equal, (d) values drawn from {-1, -0.0, +0.0, 1}: almost
    every extreme is contested"""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, H, generator=g)
    if name == "offset":
        X = X + 1000.0
    elif name == "equal":
        X = X[:1].expand(n, H).contiguous() * 7.0 + 3.0
    elif name == "ties":
        X = torch.tensor([-1.0, -0.0, 0.0, 1.0])[torch.randint(0, 4, (n, H), generator=g)]
    return X


# ---- raw entries on guarded buffers ----------------------------------------------------------------------------------------
FWD_OUT = ("Mu", "S", "Mx", "Mn", "amx", "amn")


def _raw_fwd(adj, Xv, pads=(0, ) * 6, off=0, ws=True):
    """glass_spmm_pna_csr_f32 -> (rc, {name: [n, ld] view} with Wsum, the Guarded buffers); the workspace holds NaNs"""
    L_, lib = _lib()
    op, (n, H) = adj.fwd, (adj.fwd.n_rows, Xv.shape[1])
    bufs, args = {}, []
    for name, pad in zip(FWD_OUT, pads):
        isint = name.startswith("a")
        bufs[name] = Guarded(n * (H + pad), -7 if isint else float("nan"), dtype=torch.int32 if isint else torch.float32, off=off)
        args += [bufs[name].t.data_ptr(), H + pad]
    bufs["Wsum"] = Guarded(n, float("nan"))
    nbytes = lib.glass_spmm_pna_ws_bytes(op.header.ctypes.data, H)
    assert nbytes == int(op.header[7]) * (6 * H + 1) * 4
    bufs["ws"] = Guarded(max(nbytes // 4, 4), float("nan"))   # (need not be initialised: junk on purpose)
    rc = lib.glass_spmm_pna_csr_f32(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), Xv.data_ptr(), Xv.stride(0), EPS,
                                    *args, bufs["Wsum"].t.data_ptr(), n, H, op.header.ctypes.data, op.plan.data_ptr(),
                                    bufs["ws"].t.data_ptr() if ws else None, _stream())
    torch.cuda.synchronize()
    out = {name: bufs[name].t.view(n, H + pad) for name, pad in zip(FWD_OUT, pads)}
    out["Wsum"] = bufs["Wsum"].t
    return rc, out, list(bufs.values())


def _raw_bwd(adj, Xv, Muv, Av, Cv, amxv, Gxv, amnv, Gnv, pad=0, off=0, ws=True):
    L_, lib = _lib()
    op, (n, H) = adj.bwd, (adj.bwd.n_rows, Xv.shape[1])
    lddx = H + pad
    D = Guarded(n * lddx, float("nan"), off=off)
    nbytes = lib.glass_spmm_pna_bwd_ws_bytes(op.header.ctypes.data, H)
    assert nbytes == int(op.header[7]) * H * 4
    W = Guarded(max(nbytes // 4, 4), float("nan"))
    rows = []
    for a in (Xv, Muv, Av, Cv, amxv, Gxv, amnv, Gnv):
        rows += [a.data_ptr(), a.stride(0)]
    rc = lib.glass_spmm_pna_bwd_f32(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), adj.eid_t.data_ptr(), *rows,
                                    D.t.data_ptr(), lddx, n, H, op.header.ctypes.data, op.plan.data_ptr(),
                                    W.t.data_ptr() if ws else None, _stream())
    torch.cuda.synchronize()
    return rc, D.t.view(n, lddx), (D, W)


def _share(err, bound):
    """the largest err / bound; where the bound is 0 the error must be 0 too"""
    assert (err[bound == 0] == 0).all(), "an error where the bound allows none"
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


def _np64(t):
    return t.detach().cpu().double().numpy()


def _grade_fwd(ref, X, out, H, m=None):
    """the extremes and their entries bit for bit; shares of the bounds of (Wsum, Mu, S) against fp64 on the same fp32 X"""
    m = PO.forward(ref["rowptr"], ref["col"], ref["val"], X.double().numpy(), EPS) if m is None else m
    for name in ("Mx", "Mn"):
        want = torch.from_numpy(m[name].astype(np.float32))   # (exact: the winner's own fp32 bits, its sign included)
        assert torch.equal(_bits(out[name][:, :H].cpu()), _bits(want)), name
    for name in ("amx", "amn"):
        assert torch.equal(out[name][:, :H].cpu(), torch.from_numpy(m[name])), name
    b = MO.bounds(m)
    shares = {"Wsum": _share(np.abs(_np64(out["Wsum"]) - m["W"]), b["W"]),
              "Mu": _share(np.abs(_np64(out["Mu"][:, :H]) - m["Mu"]), b["Mu"]),
              "S": _share(np.abs(_np64(out["S"][:, :H]) - m["Std"]), b["Std"])}
    return shares, m


def _grade_bwd(ref, X, Muv, Av, Cv, amxv, Gxv, amnv, Gnv, dXv):
    dX64, mass = PO.backward(ref["rowptr_t"], ref["col_t"], ref["val_t"], ref["eid_t"], X.double().numpy(), _np64(Muv), _np64(Av),
                             _np64(Cv), amxv.cpu().numpy(), _np64(Gxv), amnv.cpu().numpy(), _np64(Gnv))
    return _share(np.abs(_np64(dXv) - dX64), PO.bound_dx(ref["rowptr_t"], mass))


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
        dMu, dS, Gx, Gn = (torch.randn(n, H, generator=g).to(DEV) for _ in range(4))
        rc, out, guards = _raw_fwd(adj, Xd)
        L_.check(rc, "glass_spmm_pna_csr_f32")
        assert all(g_.intact() for g_ in guards), (graph_kind, H, name, "guards of the results / workspace")
        assert not any(bool(torch.isnan(out[k]).any()) for k in ("Mu", "S", "Mx", "Mn", "Wsum")), "every element is written"
        assert bool((out["amx"] >= -1).all()) and bool((out["amn"] >= -1).all())
        for k in ("Mu", "S", "Mx", "Mn", "Wsum"):
            assert bool((out[k][empty] == 0).all()), (k, "a row without entries")
        assert bool((out["amx"][empty] == -1).all()) and bool((out["amn"][empty] == -1).all())
        rc, out2, _g = _raw_fwd(adj, Xd)
        for k in out:
            assert torch.equal(_bits(out[k]), _bits(out2[k])), (graph_kind, H, name, k, "two forward runs differ")
        shares, m = _grade_fwd(ref, X, out, H)
        _merge(worst, shares)
        if name == "equal":   # no x^2, d = 0 at every merge: exactly no spread, bit for bit
            live = out["Wsum"] > 0
            want = float(np.sqrt(np.float32(np.float32(0.0) + np.float32(EPS))))
            assert bool((out["S"][live] == want).all()) and bool((out["Mu"][live] == Xd[0].expand(n, H)[live]).all()), (graph_kind, H)
        # backward on the kernel's own results
        A, C = ops.pna_factors(out["S"], out["Wsum"], dS, dMu)
        assert not bool(A[empty].any()) and not bool(C[empty].any())
        operands = (Xd, out["Mu"], A, C, out["amx"], Gx, out["amn"], Gn)
        rc, dXv, guards = _raw_bwd(adj, *operands)
        L_.check(rc, "glass_spmm_pna_bwd_f32")
        assert all(g_.intact() for g_ in guards) and not bool(torch.isnan(dXv).any()), (graph_kind, H, name)
        rc, dX2, _g = _raw_bwd(adj, *operands)
        assert torch.equal(_bits(dXv), _bits(dX2)), (graph_kind, H, name, "two backward runs differ")
        _merge(worst, {"dX": _grade_bwd(ref, X, *operands[1:], dXv)})
    print(f"K1p shares {graph_kind} H={H}: " + " ".join(f"{k} {worst[k]:.3f}" for k in ("Wsum", "Mu", "S", "dX")))
    assert all(v <= 1.0 for v in worst.values()), (graph_kind, H, worst)


@pytest.mark.parametrize("H,pads,off", [(64, (8, 4, 12, 4, 8, 16, 4), 0), (64, (3, 1, 2, 5, 7, 3, 1), 0), (18, (2, 6, 1, 3, 5, 2, 4), 0),
                                        (64, (0, ) * 7, 1), (64, (4, ) * 7, 3)])
def test_strided_and_unaligned_operands(H, pads, off):
    """Every operand as a column slice of a wider buffer (multiples of 4 keep the 16-byte form, anything else takes the scalar
    one), and every operand `off` floats past a 16-byte boundary (the scalar form at a width that has a vector one); the columns
    beyond H are neither read (NaN) nor written."""
    from glass_amd import ops
    L_, _ = _lib()
    adj, ref = _adj("mixed")
    n = adj.n_node
    X = _data("normal", n, H, 5)
    g = torch.Generator().manual_seed(6)
    dMu, dS, Gx, Gn = (torch.randn(n, H, generator=g).to(DEV) for _ in range(4))

    def wide(src, pad):
        src = src.to(DEV)
        buf = torch.full((n * (H + pad) + off + 4, ), float("nan") if src.is_floating_point() else -9, dtype=src.dtype, device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + n * (H + pad)].view(n, H + pad)
        v[:, :H] = src
        return v[:, :H]
    Xv = wide(X, pads[0])
    assert Xv.data_ptr() % 16 == 4 * off
    rc, out, guards = _raw_fwd(adj, Xv, pads[1:], off)
    L_.check(rc, "glass_spmm_pna_csr_f32")
    for name in ("Mu", "S", "Mx", "Mn"):
        assert bool(torch.isnan(out[name][:, H:]).all()), name
    assert bool((out["amx"][:, H:] == -7).all()) and bool((out["amn"][:, H:] == -7).all()) and all(g_.intact() for g_ in guards)
    worst, _m = _grade_fwd(ref, X, out, H)
    A, C = ops.pna_factors(out["S"][:, :H], out["Wsum"], dS, dMu)
    operands = (Xv, out["Mu"][:, :H], wide(A, pads[1]), wide(C, pads[2]), out["amx"][:, :H], wide(Gx, pads[3]), out["amn"][:, :H],
                wide(Gn, pads[4]))
    rc, dXv, guards = _raw_bwd(adj, *operands, pad=pads[6], off=off)
    L_.check(rc, "glass_spmm_pna_bwd_f32")
    assert bool(torch.isnan(dXv[:, H:]).all()) and all(g_.intact() for g_ in guards)
    _merge(worst, {"dX": _grade_bwd(ref, X, *operands[1:], dXv[:, :H])})
    print(f"K1p shares strided H={H} pads {pads} off {off}: " + " ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_refusals_on_the_device_and_a_call_without_rows():
    from glass_amd import graph
    L_, lib = _lib()
    adj, ref = _adj("mixed")
    n, H = adj.n_node, 8
    Xd = _data("normal", n, H, 1).to(DEV)
    arg = torch.zeros(n, H, dtype=torch.int32, device=DEV)
    # partial slots and no workspace: refused before any launch, nothing written
    assert int(adj.fwd.header[7]) > 0 and int(adj.bwd.header[7]) > 0
    rc, out, guards = _raw_fwd(adj, Xd, ws=False)
    assert rc == -1 and b"ws is null" in lib.glass_last_error_string()
    assert all(g_.intact() for g_ in guards) and all(bool(torch.isnan(out[k]).all()) for k in ("Mu", "S", "Mx", "Mn", "Wsum"))
    assert bool((out["amx"] == -7).all()) and bool((out["amn"] == -7).all())
    rc, dXv, guards = _raw_bwd(adj, Xd, Xd, Xd, Xd, arg, Xd, arg, Xd, ws=False)
    assert rc == -1 and b"ws is null" in lib.glass_last_error_string() and bool(torch.isnan(dXv).all())
    # n_rows == 0: 0 without a launch
    rp = np.zeros(1, dtype=np.int32)
    words = ctypes.c_int64(0)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, 0, None, ctypes.byref(words)) == 0
    plan = np.zeros(words.value, dtype=np.int32)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, 0, plan.ctypes.data, ctypes.byref(words)) == 0
    pd = torch.from_numpy(plan).to(DEV)
    rpd = torch.zeros(1, dtype=torch.int32, device=DEV)
    bufs = [Guarded(4 * H, float("nan")) for _ in range(8)]
    p = [b.t.data_ptr() for b in bufs]
    h, st = plan.ctypes.data, _stream()
    assert lib.glass_spmm_pna_csr_f32(rpd.data_ptr(), None, None, p[0], H, EPS, p[1], H, p[2], H, p[3], H, p[4], H, p[5], H, p[6], H,
                                      p[7], 0, H, h, pd.data_ptr(), None, st) == 0
    assert lib.glass_spmm_pna_bwd_f32(rpd.data_ptr(), None, None, None, p[0], H, p[1], H, p[2], H, p[3], H, p[4], H, p[5], H, p[6], H,
                                      p[6], H, p[7], H, 0, H, h, pd.data_ptr(), None, st) == 0
    torch.cuda.synchronize()
    assert all(b.intact() and bool(torch.isnan(b.t).all()) for b in bufs)
    # weights are multiplicities
    n2, ei, ew = _graph("all_long")
    for bad in (0.0, -1.0, float("nan")):
        wbad = ew.clone()
        wbad[3] = bad
        with pytest.raises(ValueError, match="strictly positive"):
            graph.CSRAdj(ei.to(DEV), wbad.to(DEV), n2, "pna")


def test_host_objects_delta_and_the_mix():
    from glass_amd import ops
    adj, ref = _adj("mixed")
    n, H = adj.n_node, 20
    W64 = MO.segsum(ref["val"], ref["rowptr"])
    assert isinstance(adj.pna_delta, float) and abs(adj.pna_delta - PO.delta(W64)) <= 1e-14
    assert torch.equal(adj.pna_wsum.cpu(), torch.from_numpy(W64.astype(np.float32))) and adj.eid_t.dtype == torch.int32
    X = _data("normal", n, H, 9)
    theta = torch.randn(12, H, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        mu, mx, mn, s = ops.spmm_pna(adj, X.to(DEV), EPS)
        Y = ops.pna_mix(mu, mx, mn, s, adj.pna_wsum, adj.pna_delta, theta.to(DEV))
    want = PO.pna_mix(_np64(mu), _np64(mx), _np64(mn), _np64(s), W64, adj.pna_delta, theta.double().numpy())
    e = rel_inf(Y.cpu(), torch.from_numpy(want))
    print(f"pna_mix on the device against fp64 on the same aggregates: {e:.2e}")
    assert e <= TOL and not bool(Y[torch.from_numpy(W64 == 0).to(DEV)].any())


@pytest.mark.parametrize("which", ("mu", "mx", "mn", "s", "all"))
def test_autograd_binding(which, monkeypatch):
    from glass_amd import graph, ops
    L_, _ = _lib()
    n, ei, ew = _graph("mixed")
    adj = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "pna")   # (its own: the workspace cache is looked at below)
    H = 20
    X = _data("normal", n, H, 3)
    g = torch.Generator().manual_seed(4)
    names = ("mu", "mx", "mn", "s")
    G = {k: torch.randn(n, H, generator=g) for k in names}
    calls = []
    real = graph.CSRAdj.pna_bwd
    monkeypatch.setattr(graph.CSRAdj, "pna_bwd", lambda self, *a: (calls.append(1), real(self, *a))[1])
    # under no_grad, and with an operand that needs no gradient: no backward, its workspace is never made
    with torch.no_grad():
        r0 = ops.spmm_pna(adj, X.to(DEV), EPS)
    r1 = ops.spmm_pna(adj, X.to(DEV), EPS)
    assert all(a.grad_fn is None for a in r0 + r1) and calls == []
    assert not any(k[0] == "pna_bwd" for k in adj._aggr_ws) and any(k[0] == "pna_fwd" for k in adj._aggr_ws)
    rc, out, _g = _raw_fwd(adj, X.to(DEV))
    L_.check(rc, "glass_spmm_pna_csr_f32")
    for got in (r0, r1):
        for a, k in zip(got, ("Mu", "Mx", "Mn", "S")):
            assert torch.equal(_bits(a), _bits(out[k])), k
    # fp64 autograd of the restatement on the same data
    keys = names if which == "all" else (which, )
    X64 = X.double().requires_grad_(True)
    ref = dict(zip(names, PO.torch_pna(ei, ew.double(), n, X64, EPS)))
    (dX_want, ) = torch.autograd.grad([ref[k] for k in keys], X64, [G[k].double() for k in keys])
    Xd = X.to(DEV).requires_grad_(True)
    mine = dict(zip(names, ops.spmm_pna(adj, Xd, EPS)))
    (got, ) = torch.autograd.grad([mine[k] for k in keys], Xd, [G[k].to(DEV) for k in keys])   # the other results: None
    assert calls == [1] and any(k[0] == "pna_bwd" for k in adj._aggr_ws)
    e = rel_inf(got.cpu(), dX_want)
    print(f"autograd dX through {which}: {e:.2e}")
    assert e <= TOL
    if which == "all":
        with pytest.raises(L_.GlassHipError, match="spmm_pna"):
            ops.spmm(adj, X.to(DEV))
        with pytest.raises(L_.GlassHipError, match="replicated pna aggregation is not built"):
            ops.spmm_rep(adj, torch.zeros(2 * n, H, device=DEV), 2)
        mean = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "mean")
        with pytest.raises(L_.GlassHipError, match="not 'pna'"):
            ops.spmm_pna(mean, X.to(DEV))
        with pytest.raises(L_.GlassHipError, match="not 'pna'"):
            mean.pna_fwd(X.to(DEV))


# ---- through the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", ("sum", "mean"))
@pytest.mark.parametrize("hidden", (64, 8))
def test_model_against_the_fp64_restatement(hidden, pool):
    """Two GLASSConv layers with aggr "pna" on tests/test_gpu_aggr_max.py's model_graph (one hub destination) at the seeds of
    aggr_pna_oracle.MODEL_SEEDS, whose winner / runner-up gaps tests/test_aggr_pna_host.py asserts; every element is compared,
    pna_weight's gradient included."""
    from impl import utils
    model, loss_ref, logits_ref, grads_ref, gap, (N, ei, ew, x, pos, y) = PO.model_oracle(hidden, pool)
    print(f"hidden {hidden} pool {pool}: smallest winner / runner-up gap in the oracle {gap:.3e} of the layer's largest message")
    model.to(DEV).train()
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in (x, ei, ew, pos, y))
    logits = model(xg, eig, ewg, posg, utils.MaxZOZ(xg, posg), id=0)
    loss = nn.CrossEntropyLoss()(logits, yg)
    loss.backward()
    torch.cuda.synchronize()
    assert all(c.adj.aggr == "pna" for c in model.conv.convs)
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    keys = sorted(grads_ref)
    assert set(keys) == set(mine) and sum(k.endswith("pna_weight") for k in keys) == 2
    gmax = max(float(grads_ref[k].abs().max()) for k in keys)
    assert all(float(grads_ref[k].abs().max()) > 1e-3 * gmax for k in keys if k.endswith("pna_weight")), \
        "pna_weight's gradients must count in the flat metric"
    e_logits = rel_inf(logits.detach().cpu(), logits_ref)
    e_loss = abs(loss.item() - loss_ref.item()) / abs(loss_ref.item())
    e_grad = rel_inf(flat_grads(mine, keys), flat_grads(grads_ref, keys))
    print(f"hidden {hidden} pna pool {pool}: loss {e_loss:.2e} logits {e_logits:.2e} flat gradient {e_grad:.2e}")
    assert e_loss <= TOL and e_logits <= TOL and e_grad <= TOL


def test_training_on_the_captured_per_op_step_equals_its_eager_run(monkeypatch):
    """Three epochs of impl.train.train (one batch each) at aggr "pna": the TrainStep is captured and reports the per-op form (the
    stack program does not serve pna); losses and parameters equal, bit for bit, those of a deep copy trained with eager
    launches; pna_weight lives in the parameter arena and has moved from 1 / 12."""
    from helpers import build_glass
    from impl import SubGDataset, config, train, utils
    from glass_amd import stack, synth, train as gtrain
    config.set_device(0)
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=2, n_batches=1)
    x, ei, ew, pos, y = (torch.from_numpy(a).to(DEV) for a in (x, ei, ew, pos, y))
    torch.manual_seed(3)
    gnn = build_glass(64, 2, int(x.max()), w.n_class, "pna", w.pool, w.z_ratio).to(DEV)
    twin = copy.deepcopy(gnn)
    loss_fn = nn.CrossEntropyLoss()
    ds = SubGDataset.GDataset(x, ei, ew, pos, y)
    loader = lambda: SubGDataset.ZGDataloader(ds, w.batch, z_fn=utils.MaxZOZ, shuffle=False, drop_last=True)
    out = {}
    for name, net, use_graph in (("graph", gnn, True), ("eager", twin, False)):
        monkeypatch.setattr(gtrain, "USE_GRAPH", use_graph)
        opt = torch.optim.Adam(net.parameters(), lr=5e-3)
        out[name] = [train.train(opt, net, loader(), loss_fn) for _ in range(3)]
        steps = net.__dict__.get("_glass_train_steps") or {}
        assert len(steps) == 1
        step = next(iter(steps.values()))
        net.train()
        assert step.graphed == use_graph and not step._program_step() and not stack.step_supported(net, loss_fn)
        assert not stack.StackProgram.supported(net.conv) and all(c.adj.aggr == "pna" for c in net.conv.convs)
        arena = net.__dict__["_glass_grad_bucket"]
        lo, hi = arena.flat_param.data_ptr(), arena.flat_param.data_ptr() + 4 * arena.flat_param.numel()
        for c in net.conv.convs:
            assert any(c.pna_weight is p for p in arena.params) and lo <= c.pna_weight.data_ptr() < hi
    print(f"pna: losses {out['graph']}")
    assert np.isfinite(out["graph"]).all() and out["graph"][1] != out["graph"][0]
    assert np.array_equal(np.float32(out["graph"]).view(np.int32), np.float32(out["eager"]).view(np.int32)), out
    sd, sd2 = gnn.state_dict(), twin.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    for l in range(2):
        assert not bool((sd[f"conv.convs.{l}.pna_weight"] == torch.tensor(1.0 / 12.0, device=DEV)).all())
