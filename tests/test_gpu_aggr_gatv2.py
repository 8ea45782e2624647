"""K1a2 on the GPU: glass_spmm_gatv2_score_f32 / _csr_f32 / _edge_f32 / _bwd_f32 / _datt_f32 (csrc/spmm_gatv2.hip) against the fp64
restatement tests/aggr_gatv2_oracle.py on every plan form and lane layout (the two graphs of tests/test_gpu_aggr_gat.py), the host
objects (graph.CSRAdj.gatv2_*, ops.spmm_gatv2), a GLASS model with aggr "gatv2" against an fp64 restatement of the model, and
impl.train.train on the captured per-op step, whose replays must read the live attention vector.

Y, L and dX are compared at rel-inf <= 1e-5 against fp64; s, g, Gd, R and d att, cancelling sums, by the same rule
applied to a sum, element by element: |got - ref| <= 1e-5 * (the sum of the absolute values of the terms).  Run to run every
entry gives the same bits.  att and X are drawn so that |s_e| <= 8 (aggr_gatv2_oracle.case_operands); tests/
test_aggr_gatv2_host.py shows on the CPU that an fp32 restatement of these very cases stays within the same bounds."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import aggr_gatv2_oracle as VO
from aggr_max_oracle import MaxAdj
from helpers import flat_grads, rel_inf
from test_gpu_aggr_gat import Guarded, _graph, model_graph

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = VO.TOL


def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def ref_adj(kind):
    """the sorted CSR of the restatement (fp64 weights), from the shuffled edge list of the gat tests' graph `kind`"""
    n, ei, ew = _graph(kind)
    return MaxAdj(ei, ew.double(), n)


@functools.lru_cache(maxsize=None)
def operands(kind, H):
    """(X, dY, att) on the host: |s_e| <= 8 over the graph at every slope of the tests (VO.case_operands)"""
    return VO.case_operands(ref_adj(kind), 1000 * H + (kind == "mixed"), H)


@functools.lru_cache(maxsize=None)
def _adj(kind):
    from glass_amd import graph
    n, ei, ew = _graph(kind)
    return graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "gatv2")


@functools.lru_cache(maxsize=None)
def _reference(kind, H, slope):
    X, dY, att = operands(kind, H)
    return VO.reference(ref_adj(kind), X, dY, att, slope)


def test_the_adjacency_is_the_gat_one_and_weights_must_be_positive():
    from glass_amd import graph
    for kind in ("mixed", "all_long"):
        adj, ref = _adj(kind), ref_adj(kind)
        assert adj.aggr == "gatv2"
        for got, want in ((adj.fwd.rowptr, ref.rowptr), (adj.fwd.col, ref.col), (adj.bwd.rowptr, ref.rowptr_t),
                          (adj.bwd.col, ref.col_t), (adj.eid_t, ref.eid_t)):
            assert got.dtype == torch.int32 and torch.equal(got.cpu().to(torch.int64), want)
        assert torch.equal(adj.fwd.val.cpu().double(), ref.val) and torch.equal(adj.bwd.val.cpu().double(), ref.val_t)  # raw weights
    f, b = _adj("mixed").fwd.header, _adj("mixed").bwd.header
    assert f[4] > 100 and f[5] >= 9 and f[6] == 2 and f[7] == 2 + 3, "sweep items, long items, two cut rows"
    assert b[4] > 100 and b[5] >= 3 and b[6] >= 1 and b[7] >= 3, "the hub's transposed row is cut"
    n, ei, ew = _graph("all_long")
    for bad in (0.0, -1.0, float("nan")):
        w = ew.clone()
        w[3] = bad
        with pytest.raises(ValueError, match="strictly positive"):
            graph.CSRAdj(ei.to(DEV), w.to(DEV), n, "gatv2")


# ---- raw entries on guarded buffers --------------------------------------------------------------------------------------
def _dev_vec(v, off=0):
    """a vector on the device, `off` floats past a 16-byte boundary"""
    buf = torch.empty(v.numel() + off + 4, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[off:off + v.numel()]
    out.copy_(v)
    return out


class Run:
    """Every entry of K1a2 once, in the order of a forward and a backward, each result in a Guarded buffer (NaN-filled), every
    workspace in a Guarded buffer of NaN (it need not be initialised).  X, dY are [n, H] views with any row stride; Y and dX get
    ldy_extra / lddx_extra columns of padding; `off` floats of offset from a 16-byte boundary on every result."""
    def __init__(self, adj, Xv, dYv, att, slope, ldy_extra=0, lddx_extra=0, off=0):
        L_, lib = _lib()
        f, b = adj.fwd, adj.bwd
        n, H, nnz = f.n_rows, Xv.shape[1], f.nnz
        st = _stream()
        self.guards = []

        def out(numel, dtype=torch.float32, o=off):
            g = Guarded(numel, float("nan"), dtype, off=o)
            self.guards.append(g)
            return g

        def ws(nbytes, want, dtype=torch.float32):
            assert nbytes == want, (nbytes, want)
            return out(max(nbytes // (4 if dtype == torch.float32 else 8), 4), dtype, 0)
        fh, bh = f.header.ctypes.data, b.header.ctypes.data
        fs, bs = int(f.header[7]), int(b.header[7])
        ldy, lddx = H + ldy_extra, H + lddx_extra
        csr = (f.rowptr.data_ptr(), f.col.data_ptr(), f.val.data_ptr())
        x, ldx, dy, lddy = Xv.data_ptr(), Xv.stride(0), dYv.data_ptr(), dYv.stride(0)
        S = out(nnz)
        assert lib.glass_spmm_gatv2_score_ws_bytes(fh, H) == 0
        L_.check(lib.glass_spmm_gatv2_score_f32(*csr, x, ldx, att.data_ptr(), slope, S.t.data_ptr(), n, H, fh, f.plan.data_ptr(),
                                                None, st), "glass_spmm_gatv2_score_f32")
        Y, L = out(n * ldy), out(n)
        W = ws(lib.glass_spmm_gatv2_ws_bytes(fh, H), fs * (H + 2) * 4)
        L_.check(lib.glass_spmm_gatv2_csr_f32(*csr, x, ldx, S.t.data_ptr(), Y.t.data_ptr(), ldy, L.t.data_ptr(), n, H, fh,
                                              f.plan.data_ptr(), W.t.data_ptr(), st), "glass_spmm_gatv2_csr_f32")
        Yv = Y.t.view(n, ldy)[:, :H]
        G, P, GD, R = out(nnz), out(nnz), out(n * H), out(n * H)
        W = ws(lib.glass_spmm_gatv2_edge_ws_bytes(fh, H), fs * 2 * H * 4)
        L_.check(lib.glass_spmm_gatv2_edge_f32(*csr, x, ldx, att.data_ptr(), slope, S.t.data_ptr(), dy, lddy, Yv.data_ptr(), ldy,
                                               L.t.data_ptr(), G.t.data_ptr(), P.t.data_ptr(), GD.t.data_ptr(), R.t.data_ptr(), n, H,
                                               fh, f.plan.data_ptr(), W.t.data_ptr(), st), "glass_spmm_gatv2_edge_f32")
        DX = out(n * lddx)
        W = ws(lib.glass_spmm_gatv2_bwd_ws_bytes(bh, H), bs * H * 4)
        L_.check(lib.glass_spmm_gatv2_bwd_f32(b.rowptr.data_ptr(), b.col.data_ptr(), b.val.data_ptr(), adj.eid_t.data_ptr(), x, ldx,
                                              att.data_ptr(), slope, dy, lddy, P.t.data_ptr(), G.t.data_ptr(), GD.t.data_ptr(),
                                              DX.t.data_ptr(), lddx, n, H, bh, b.plan.data_ptr(), W.t.data_ptr(), st),
                 "glass_spmm_gatv2_bwd_f32")
        DA = out(H)
        rpw = 2 * H if H > 128 else 256
        W = ws(lib.glass_spmm_gatv2_datt_ws_bytes(n, H), -(-n // rpw) * H * 8, torch.float64)
        L_.check(lib.glass_spmm_gatv2_datt_f32(R.t.data_ptr(), DA.t.data_ptr(), n, H, W.t.data_ptr(), st), "glass_spmm_gatv2_datt_f32")
        torch.cuda.synchronize()
        self.H = H
        self.Y, self.dX = Y.t.view(n, ldy), DX.t.view(n, lddx)
        self.res = dict(s=S.t, Y=self.Y[:, :H], L=L.t, g=G.t, p=P.t, Gd=GD.t.view(n, H), R=R.t.view(n, H), dX=self.dX[:, :H],
                        datt=DA.t)

    def intact(self):
        return all(g.intact() for g in self.guards)


WORST = {}   # the largest error per quantity over the value tests of this session (printed by each; DESIGN.md quotes them)


@pytest.mark.parametrize("H", VO.WIDTHS)
@pytest.mark.parametrize("kind", ("mixed", "all_long"))
def test_values_against_the_restatement_and_repeatability(kind, H):
    adj, ref = _adj(kind), ref_adj(kind)
    X, dY, att = operands(kind, H)
    Xd, dYd, attd = X.to(DEV), dY.to(DEV), att.to(DEV)
    empty = (ref.rowptr[1:] == ref.rowptr[:-1]).nonzero().reshape(-1).to(DEV)
    assert len(empty) >= 1
    for slope in VO.SLOPES:
        r = _reference(kind, H, slope)
        assert float(np.abs(r.s).max()) <= VO.S_MAX
        run = Run(adj, Xd, dYd, attd, slope)
        res = run.res
        assert run.intact(), (kind, H, slope, "guards of the results / workspaces")
        assert all(bool(torch.isfinite(v).all()) for v in res.values())
        for k in ("Y", "L", "Gd", "R"):
            assert bool((res[k][empty] == 0).all()), (k, "a row without entries")
        res2 = Run(adj, Xd, dYd, attd, slope).res
        for k in res:
            assert torch.equal(_bits(res[k]), _bits(res2[k])), (kind, H, slope, k, "two runs differ")
        e = VO.errors(res, r)
        e["p"] = VO.rel_inf(res["p"], r.p)
        for k, v in e.items():
            WORST[k] = max(WORST.get(k, 0.0), v)
        print(f"{kind} H={H} slope={slope}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + " (s, g .. datt: of their mass)")
        assert all(v <= TOL for v in e.values()), (kind, H, slope, e)
    print("worst so far: " + " ".join(f"{k} {v:.2e}" for k, v in WORST.items()))


@pytest.mark.parametrize("H", (64, 18, 260))
def test_cross_checks_against_the_static_attention_and_softmax_kernels(H):
    """slope 1: the score is att . X[i] + att . X[j], what K1a computes from att_src = att_dst = att; att = 0: the weighted
    mean of the messages, what K1s computes at t = 0.  Other kernels on the same CSR."""
    from glass_amd import graph, ops
    for kind in ("mixed", "all_long"):
        n, ei, ew = _graph(kind)
        adj = _adj(kind)
        X, dY, att = operands(kind, H)
        attd, dYd = att.to(DEV), dY.to(DEV)
        gat = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "gat")
        x1, x2 = X.to(DEV).requires_grad_(True), X.to(DEV).requires_grad_(True)
        y1 = ops.spmm_gatv2(adj, x1, attd, 1.0)
        y2 = ops.spmm_gat(gat, x2, attd, attd, slope=1.0)
        y1.backward(dYd)
        y2.backward(dYd)
        e_y, e_dx = rel_inf(y1.detach().cpu(), y2.detach().cpu()), rel_inf(x1.grad.cpu(), x2.grad.cpu())
        sm = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "softmax")
        y0 = ops.spmm_gatv2(adj, X.to(DEV), torch.zeros(H, device=DEV), 0.2)
        e_0 = rel_inf(y0.cpu(), ops.spmm_softmax(sm, X.to(DEV), torch.zeros(1, device=DEV)).cpu())
        print(f"{kind} H={H}: against K1a at slope 1: Y {e_y:.2e} dX {e_dx:.2e}; against K1s at att = 0, t = 0: Y {e_0:.2e}")
        assert e_y <= TOL and e_dx <= TOL and e_0 <= TOL


@pytest.mark.parametrize("H", (64, 18))
def test_the_rule_at_u_zero(H):
    """Rows with X[i] = -X[j] exactly for an entry (i <- j): u = 0 in every channel of that entry, where f = slope (torch's
    rule, the restatement's) — at slope 0.2 a kernel that took f = 1 there would miss dX and d att by far more than the bound."""
    adj, ref = _adj("mixed"), ref_adj("mixed")
    X, dY, att = (t.clone() for t in operands("mixed", H))
    rows = torch.from_numpy(VO.rows_of(ref.rowptr))
    pick = torch.arange(0, ref.col.shape[0], 7)
    pick = pick[rows[pick] != ref.col[pick]]
    done = set()
    for i, j in zip(rows[pick].tolist(), ref.col[pick].tolist()):   # (each node is set or read once: the pairs stay exact)
        if i not in done and j not in done:
            X[i] = -X[j]
            done.update((i, j))
    u0 = (X[rows] + X[ref.col] == 0).all(1)
    assert int(u0.sum()) >= 50
    r = VO.reference(ref, X, dY, att, 0.2)
    res = Run(adj, X.to(DEV), dY.to(DEV), att.to(DEV), 0.2).res
    e = VO.errors(res, r)
    print(f"H={H}: {int(u0.sum())} entries at u = 0: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(v <= TOL for v in e.values()), e
    # the rule matters at these inputs: with f = 1 at u = 0 the destination-side sums move by far more than the bound
    af1 = np.where((X[rows] + X[ref.col]).numpy() >= 0, 1.0, 0.2) * att.double().numpy()
    gd1 = np.zeros_like(r.Gd)
    np.add.at(gd1, rows.numpy(), r.g[:, None] * af1)
    assert float(np.abs(gd1 - r.Gd).max()) > 100 * TOL * float(np.abs(r.Gd).max())


@pytest.mark.parametrize("H", (64, 18, 260))
def test_large_scores_stay_finite(H):
    """att scaled so that |s| reaches about 80: the max is always subtracted, so everything stays finite, and Y, a convex
    combination, lies within its row's [min x, max x] up to rounding (1e-5 of the row's largest |x|: the rule)."""
    for kind in ("mixed", "all_long"):
        adj, ref = _adj(kind), ref_adj(kind)
        X, dY, att = operands(kind, H)
        att = att * (80.0 / float(np.abs(_reference(kind, H, 0.2).s).max()))   # (s is linear in att)
        res = Run(adj, X.to(DEV), dY.to(DEV), att.to(DEV), 0.2).res
        top = float(res["s"].abs().max())
        assert 79 <= top <= 81, top
        assert all(bool(torch.isfinite(v).all()) for v in res.values()), [k for k, v in res.items() if not bool(torch.isfinite(v).all())]
        idx = torch.from_numpy(VO.rows_of(ref.rowptr))[:, None].expand(-1, H)
        lo = torch.zeros(ref.n, H).scatter_reduce(0, idx, X[ref.col], "amin", include_self=False)
        hi = torch.zeros(ref.n, H).scatter_reduce(0, idx, X[ref.col], "amax", include_self=False)
        slack = TOL * torch.maximum(lo.abs(), hi.abs())
        Yc = res["Y"].cpu()
        assert bool((Yc >= lo - slack).all()) and bool((Yc <= hi + slack).all()), (kind, H)


@pytest.mark.parametrize("H,pads,off", [(64, (8, 4, 12, 4), 0), (64, (3, 1, 2, 5), 0), (18, (2, 6, 1, 3), 0), (64, (0, 0, 0, 0), 1),
                                        (260, (4, 4, 4, 4), 3), (260, (1, 0, 0, 0), 0)])
def test_strided_and_unaligned_operands(H, pads, off):
    """X, dY, Y and dX as column slices of wider buffers (multiples of 4 keep the 16-byte form, anything else takes the scalar
    one), and every operand `off` floats past a 16-byte boundary (the scalar form at a width that has a vector one); the
    columns beyond H are neither read (NaN) nor written.  The same bounds."""
    adj, ref = _adj("mixed"), ref_adj("mixed")
    px, pdy, py, pdx = pads
    X, dY, att = operands("mixed", H)
    r = _reference("mixed", H, 0.2)

    def wide(src, pad):
        buf = torch.full((ref.n * (H + pad) + off + 4, ), float("nan"), device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + ref.n * (H + pad)].view(ref.n, H + pad)
        v[:, :H] = src.to(DEV)
        return v[:, :H]
    Xv, dYv = wide(X, px), wide(dY, pdy)
    assert Xv.data_ptr() % 16 == 4 * off
    run = Run(adj, Xv, dYv, _dev_vec(att, off), 0.2, py, pdx, off)
    e = VO.errors(run.res, r)
    print(f"H={H} pads={pads} off={off}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(v <= TOL for v in e.values()), e
    assert run.intact() and bool(torch.isnan(run.Y[:, H:]).all()) and bool(torch.isnan(run.dX[:, H:]).all())


def test_a_call_without_rows_or_entries_launches_nothing():
    L_, lib = _lib()
    H = 8
    for n in (0, 2):   # no rows; two rows without entries
        rp = np.zeros(n + 1, dtype=np.int32)
        words = ctypes.c_int64(0)
        assert lib.glass_spmm_plan_build(rp.ctypes.data, n, None, ctypes.byref(words)) == 0
        plan = np.zeros(words.value, dtype=np.int32)
        assert lib.glass_spmm_plan_build(rp.ctypes.data, n, plan.ctypes.data, ctypes.byref(words)) == 0
        pd = torch.from_numpy(plan).to(DEV)
        rpd = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
        bufs = [Guarded(4 * H, float("nan")) for _ in range(9)]
        x, att, y, l, dy, gd, rr, dx, da = (q.t.data_ptr() for q in bufs)
        h, st, r, p = plan.ctypes.data, _stream(), rpd.data_ptr(), pd.data_ptr()
        assert lib.glass_spmm_gatv2_score_f32(r, None, None, x, H, att, 0.2, None, n, H, h, p, None, st) == 0
        assert lib.glass_spmm_gatv2_csr_f32(r, None, None, x, H, None, y, H, l, n, H, h, p, None, st) == 0
        assert lib.glass_spmm_gatv2_edge_f32(r, None, None, x, H, att, 0.2, None, dy, H, y, H, l, None, None, gd, rr, n, H, h, p, None,
                                             st) == 0
        assert lib.glass_spmm_gatv2_bwd_f32(r, None, None, None, x, H, att, 0.2, dy, H, None, None, gd, dx, H, n, H, h, p, None, st) == 0
        assert lib.glass_spmm_gatv2_datt_f32(rr, da, 0, H, None, st) == 0
        torch.cuda.synchronize()
        assert all(q.intact() and bool(torch.isnan(q.t).all()) for q in bufs)


def test_isolated_nodes_and_a_graph_without_edges():
    """Node 0 and node 4 have no entry in either direction: Y = 0, L = 0, dX = 0 there.  A graph without any edge: the entries
    launch nothing and the host objects hand out the zeros."""
    from glass_amd import graph, ops
    H = 12
    ei = torch.tensor([[1, 2, 3, 1, 2], [2, 3, 1, 1, 1]])
    ew = torch.tensor([0.5, 1.0, 2.0, 1.5, 0.25])
    g = torch.Generator().manual_seed(9)
    X, dY, att = torch.randn(5, H, generator=g), torch.randn(5, H, generator=g), torch.rand(H, generator=g) - 0.5
    adj = graph.CSRAdj(ei.to(DEV), ew.to(DEV), 5, "gatv2")
    x = X.to(DEV).requires_grad_(True)
    a = att.to(DEV).requires_grad_(True)
    y = ops.spmm_gatv2(adj, x, a, 0.2)
    y.backward(dY.to(DEV))
    r = VO.reference(MaxAdj(ei, ew.double(), 5), X, dY, att, 0.2)
    assert rel_inf(y.detach().cpu(), r.Y) <= TOL and rel_inf(x.grad.cpu(), r.dX) <= TOL and VO.of_mass(a.grad, r.datt, r.mass_datt) <= TOL
    lse = adj.gatv2_fwd(x.detach(), adj.gatv2_score(x.detach(), a.detach(), 0.2))[1]
    for node in (0, 4):
        assert bool((y[node] == 0).all()) and float(lse[node]) == 0.0 and bool((x.grad[node] == 0).all())
    none = graph.CSRAdj(torch.zeros((2, 0), dtype=torch.int64, device=DEV), torch.zeros(0, device=DEV), 5, "gatv2")
    x0 = X.to(DEV).requires_grad_(True)
    a0 = att.to(DEV).requires_grad_(True)
    y0 = ops.spmm_gatv2(none, x0, a0, 0.2)
    y0.backward(dY.to(DEV))
    assert y0.shape == (5, H) and bool((y0 == 0).all()) and bool((x0.grad == 0).all()) and bool((a0.grad == 0).all())


def test_autograd_binding_and_frozen_inputs(monkeypatch):
    from glass_amd import graph, ops
    L_, _ = _lib()
    adj, ref = _adj("mixed"), ref_adj("mixed")
    H, slope = 20, 0.2
    X, dY, att = operands("mixed", H)
    r = _reference("mixed", H, slope)
    calls = {"edge": 0, "bwd": 0, "datt": 0}
    for key in calls:
        real = getattr(graph.CSRAdj, "gatv2_" + key)
        monkeypatch.setattr(graph.CSRAdj, "gatv2_" + key,
                            lambda self, *a_, _real=real, _key=key: (calls.__setitem__(_key, calls[_key] + 1), _real(self, *a_))[1])
    Xd = X.to(DEV).requires_grad_(True)
    a1 = nn.Parameter(att.to(DEV))
    out = ops.spmm_gatv2(adj, Xd, a1, slope)
    out.backward(dY.to(DEV))
    assert rel_inf(out.detach().cpu(), r.Y) <= TOL and rel_inf(Xd.grad.cpu(), r.dX) <= TOL
    assert a1.grad.shape == (H, ) and VO.of_mass(a1.grad, r.datt, r.mass_datt) <= TOL
    assert calls == {"edge": 1, "bwd": 1, "datt": 1}
    # att frozen: no column reduction, no .grad, the same dX bits
    X2 = X.to(DEV).requires_grad_(True)
    a2 = nn.Parameter(att.to(DEV)).requires_grad_(False)
    ops.spmm_gatv2(adj, X2, a2, slope).backward(dY.to(DEV))
    assert a2.grad is None and calls == {"edge": 2, "bwd": 2, "datt": 1}
    assert torch.equal(_bits(X2.grad), _bits(Xd.grad))
    # only att: no transposed pass, the same gradient bits
    a3 = nn.Parameter(att.to(DEV))
    ops.spmm_gatv2(adj, X.to(DEV), a3, slope).backward(dY.to(DEV))
    assert calls == {"edge": 3, "bwd": 2, "datt": 2}
    assert torch.equal(_bits(a3.grad), _bits(a1.grad))
    with pytest.raises(L_.GlassHipError, match="spmm_gatv2"):
        ops.spmm(adj, X.to(DEV))
    with pytest.raises(L_.GlassHipError, match="replicated gatv2 aggregation is not built"):
        ops.spmm_rep(adj, torch.zeros(2 * ref.n, H, device=DEV), 2)
    other = graph.CSRAdj(*(t.to(DEV) for t in _graph("all_long")[1:]), _graph("all_long")[0], "gat")
    with pytest.raises(L_.GlassHipError, match="not 'gatv2'"):
        other.gatv2_score(torch.zeros(other.n_node, 4, device=DEV), torch.zeros(4, device=DEV), 0.2)


# ---- through the model ----------------------------------------------------------------------------------------------------
MODEL_SEEDS = (11, 5)   # (graph, weights): those of the gat model test


def model_and_oracle(graph_seed, weight_seed, hidden=64):
    """(model on the CPU, its fp64 oracle after backward, the attention keys, data): the oracle is OracleGLASS(aggr "sum") whose
    conv.adj are GatV2Adj — the aggregation from plain torch ops, differentiated by autograd, both att included."""
    from helpers import build_glass
    from oracle import glass_oracle as O
    N, ei, ew, x, pos, y = model_graph(graph_seed)
    torch.manual_seed(weight_seed)
    model = build_glass(hidden, 2, int(x.max()), 3, "gatv2", "mean", 0.8, dropout=0.0, jk=True)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    att_keys = sorted(k for k in sd if k.endswith(".att"))
    assert att_keys == ["conv.convs.0.att", "conv.convs.1.att"]
    orc = O.OracleGLASS(hidden, 2, int(x.max()), 3, aggr="sum", pool="mean", z_ratio=0.8).double()
    orc.load_state_dict({k: v for k, v in sd.items() if k not in att_keys})
    orc.train()
    att = {k: sd[k].double().requires_grad_(True) for k in att_keys}
    for l, conv in enumerate(orc.conv.convs):
        conv.adj = VO.GatV2Adj(ei, ew.double(), N, att[f"conv.convs.{l}.att"], 0.2)
    logits_ref = orc(x, ei, ew.double(), pos, O.max_zero_one(x, pos))
    loss_ref = nn.CrossEntropyLoss()(logits_ref, y)
    loss_ref.backward()
    grads_ref = {k: p.grad.clone() for k, p in orc.named_parameters()}
    grads_ref.update({k: v.grad.clone() for k, v in att.items()})
    return model, logits_ref.detach(), loss_ref.item(), grads_ref, att_keys, (N, ei, ew, x, pos, y)


def test_model_with_dynamic_attention_against_the_fp64_restatement():
    """Two GLASSConv layers at hidden 64, jk, no dropout: loss, logits and the flat gradient over all parameters, both attention
    vectors included."""
    from impl import utils
    model, logits_ref, loss_ref, grads_ref, att_keys, (N, ei, ew, x, pos, y) = model_and_oracle(*MODEL_SEEDS)
    keys = sorted(grads_ref)
    gmax = float(flat_grads(grads_ref, keys).abs().max())
    shares = {k: float(grads_ref[k].abs().max()) / gmax for k in att_keys}
    print("largest gradient of each attention vector, of the largest gradient overall (fp64 oracle):", shares)
    assert all(v > 1e-3 for v in shares.values()), "the attention vectors' gradients must count in the flat metric"

    model.to(DEV).train()
    xg, eig, ewg, posg, yg = (a.to(DEV) for a in (x, ei, ew, pos, y))
    logits = model(xg, eig, ewg, posg, utils.MaxZOZ(xg, posg), id=0)
    loss = nn.CrossEntropyLoss()(logits, yg)
    loss.backward()
    torch.cuda.synchronize()
    assert all(c.adj.aggr == "gatv2" for c in model.conv.convs)
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    assert set(keys) == set(mine)
    e_logits = rel_inf(logits.detach().cpu(), logits_ref)
    e_loss = abs(loss.item() - loss_ref) / abs(loss_ref)
    e_grad = rel_inf(flat_grads(mine, keys), flat_grads(grads_ref, keys))
    for k in att_keys:
        print(f"{k}: error {float((mine[k].double() - grads_ref[k]).abs().max()) / gmax:.2e} of the largest gradient {gmax:.3e}")
    print(f"loss {e_loss:.2e} logits {e_logits:.2e} flat gradient {e_grad:.2e}")
    assert e_loss <= TOL and e_logits <= TOL and e_grad <= TOL


def test_training_on_the_captured_per_op_step_equals_its_eager_run(monkeypatch):
    """Two epochs of impl.train.train at aggr "gatv2": the TrainStep is captured and reports the per-op form (the stack program
    does not serve gatv2); losses and parameters equal, bit for bit, those of a deep copy trained with eager launches.  The
    attention vectors live in the parameter arena, have moved from their initial bits and hold the same bits on both routes —
    a replay that read a stale copy (its values or its pre-arena address) would differ."""
    from helpers import build_glass
    from impl import SubGDataset, config, train, utils
    from glass_amd import stack, synth, train as gtrain
    config.set_device(0)
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=2, n_batches=2)
    x, ei, ew, pos, y = (torch.from_numpy(a).to(DEV) for a in (x, ei, ew, pos, y))
    torch.manual_seed(3)
    gnn = build_glass(64, 2, int(x.max()), w.n_class, "gatv2", w.pool, w.z_ratio).to(DEV)
    vectors = lambda net: [c.att for c in net.conv.convs]
    initial = [v.detach().clone() for v in vectors(gnn)]
    twin = copy.deepcopy(gnn)
    loss_fn = nn.CrossEntropyLoss()
    ds = SubGDataset.GDataset(x, ei, ew, pos, y)
    loader = lambda: SubGDataset.ZGDataloader(ds, w.batch, z_fn=utils.MaxZOZ, shuffle=False, drop_last=True)
    out = {}
    for name, net, use_graph in (("graph", gnn, True), ("eager", twin, False)):
        monkeypatch.setattr(gtrain, "USE_GRAPH", use_graph)
        opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=5e-3)
        out[name] = [train.train(opt, net, loader(), loss_fn) for _ in range(2)]
        steps = net.__dict__.get("_glass_train_steps") or {}
        assert len(steps) == 1
        step = next(iter(steps.values()))
        net.train()
        assert step.graphed == use_graph and not step._program_step() and not stack.step_supported(net, loss_fn)
        assert not stack.StackProgram.supported(net.conv) and all(c.adj.aggr == "gatv2" for c in net.conv.convs)
        arena = net.__dict__["_glass_grad_bucket"]
        lo, hi = arena.flat_param.data_ptr(), arena.flat_param.data_ptr() + 4 * arena.flat_param.numel()
        for v in vectors(net):
            assert any(v is p for p in arena.params) and lo <= v.data_ptr() < hi, (name, "attention vector outside the arena")
    assert np.isfinite(out["graph"]).all() and out["graph"][1] != out["graph"][0]
    assert np.array_equal(np.float32(out["graph"]).view(np.int32), np.float32(out["eager"]).view(np.int32)), out
    sd, sd2 = gnn.state_dict(), twin.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    for v, v0 in zip(vectors(gnn), initial):
        print(f"attention vector moved by {float((v.detach() - v0).abs().max()):.3e} after two epochs")
        assert not torch.equal(_bits(v.detach()), _bits(v0))
