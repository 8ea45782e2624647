"""K1w on the GPU: glass_spmm_dval_f32, glass_adj_colsum_f32 and glass_adj_values_bwd_f32 (csrc/spmm_edge.hip) graded element by
element against the fp64 restatement tests/edge_grad_oracle.py on every plan form and lane layout, then the host objects
(graph.CSRAdj.values_of / dval / colsum / values_bwd, ops.spmm_w).

Bounds (derived, not measured; u = 2^-24, gamma(n) = n u / (1 - n u), the textbook bound of n rounded operations in any order,
times the MASS of the element: the sum of the absolute values of its terms):
  dval[e]  H products, H - 1 additions                                          n = H + 1
  R[i]     n_i entries of row i, each a computed dval times an exact val       n = H + 1 + n_i
  C[k]     c_k entries of column k, likewise                                    n = H + 1 + c_k
  dw sum   dval itself                                                          n = H + 1
  dw mean  (dval - R[i]) / d~_i: R, the fp32 weight sum d~_i (n_i), - and /    n = H + 1 + 2 n_i + 2
  dw gcn   r_i r_j dval - (R[i] + C[i]) / (2 d~_i): R and C, the weight sums of i (twice) and j, two square roots and
           reciprocals, the products, the sum, the quotient, the difference    n = H + 1 + 3 n_i + n_j + c_i + 12
The largest observed share of each bound is printed per case (DESIGN.md K1w keeps the table)."""
import functools

import numpy as np
import pytest
import torch

import edge_grad_oracle as EO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
U = 2.0 ** -24
# (H, columns of padding behind every row of X and dY): scalar, narrow, no multiple of 4, one wave's row, just past it, the
# two tiled families' widths; a padding that is a multiple of 4 keeps the 16-byte form, any other takes the scalar one
CASES = [(1, 3), (8, 4), (8, 3), (17, 2), (64, 4), (64, 1), (65, 3), (128, 4), (256, 4)]
AGGR_CODE = {"mean": 0, "sum": 1, "gcn": 2}


def gamma(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U / (1.0 - n * U)


def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """`n` elements filled with `fill`, GUARD sentinel elements in front and behind (tests/test_gpu_aggr_gat.py's)"""
    def __init__(self, n, fill=float("nan"), dtype=torch.float32):
        self.buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=DEV)
        self.sentinel = (torch.arange(2 * GUARD, device=DEV) * 3 - 11).to(dtype)
        self.buf[:GUARD] = self.sentinel[:GUARD]
        self.buf[GUARD + n:] = self.sentinel[GUARD:]
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        n = self.t.numel()
        return torch.equal(self.buf[:GUARD], self.sentinel[:GUARD]) and torch.equal(self.buf[GUARD + n:], self.sentinel[GUARD:])


@functools.lru_cache(maxsize=None)
def _csr(kind):
    n, ei, w = EO.graph(kind)
    return EO.SortedCSR(ei, n)


@functools.lru_cache(maxsize=None)
def _adj(kind, aggr):
    from glass_amd import graph
    n, ei, w = EO.graph(kind)
    return graph.CSRAdj(torch.from_numpy(ei).to(DEV), torch.from_numpy(w).to(DEV), n, aggr)


@functools.lru_cache(maxsize=None)
def _operands(kind, H):
    n = EO.graph(kind)[0]
    g = torch.Generator().manual_seed(1000 * H + (kind == "mixed"))
    return torch.randn(n, H, generator=g), torch.randn(n, H, generator=g)


def _padded(M, pad):
    """M on the device as the first columns of a buffer with `pad` more columns of NaN (never read)"""
    buf = torch.full((M.shape[0], M.shape[1] + pad), float("nan"), device=DEV)
    buf[:, :M.shape[1]] = M.to(DEV)
    return buf[:, :M.shape[1]]


def test_plans_take_every_form():
    for kind in ("mixed", "all_long"):
        csr = _csr(kind)
        for aggr in EO.AGGRS:
            adj = _adj(kind, aggr)
            for got, want in ((adj.fwd.rowptr, csr.rowptr), (adj.fwd.col, csr.col), (adj.bwd.rowptr, csr.rowptr_t),
                              (adj.bwd.col, csr.col_t), (adj.perm, csr.perm), (adj._edge_grad_state("test")[0], csr.eid_t)):
                assert torch.equal(got.cpu().to(torch.int64), torch.from_numpy(want)), (kind, aggr)
            assert not hasattr(adj, "eid_t"), "the stored fields of a sum / mean / gcn adjacency are as before"
    f, b = _adj("mixed", "sum").fwd.header, _adj("mixed", "sum").bwd.header
    # header words (tests/test_cabi.py): 4 sweep items, 5 long items, 6 reduce rows, 7 partial slots, 8 threshold, 9 chunk
    assert f[4] > 100 and f[5] >= 9 and f[6] == 2 and f[7] == 2 + 3 and f[8] == 64 and f[9] == 256
    assert b[4] > 100 and b[5] >= 3 and b[6] >= 1 and b[7] >= 3, "the hub's transposed row is cut"
    for h in (_adj("all_long", "sum").fwd.header, _adj("all_long", "sum").bwd.header):
        assert h[4] == 0 and h[8] == 0 and h[5] >= 42 and h[6] >= 1 and h[7] >= 2, "no sweep, every row workgroup items, cut rows"


class Run:
    """The three entries once on guarded, NaN-filled results and workspaces"""
    def __init__(self, adj, Xv, dYv):
        L_, lib = _lib()
        f, b = adj.fwd, adj.bwd
        n, H, nnz = f.n_rows, Xv.shape[1], f.nnz
        s = _stream()
        self.guards = []

        def out(numel):
            g = Guarded(numel)
            self.guards.append(g)
            return g
        eid_t, perm32, _ws = adj._edge_grad_state("test")
        fh, bh = f.header.ctypes.data, b.header.ctypes.data
        DV, R = out(nnz), out(n)
        nb = lib.glass_spmm_dval_ws_bytes(fh, H)
        assert nb == 4 * int(f.header[7])
        W = out(max(nb // 4, 4))
        L_.check(lib.glass_spmm_dval_f32(f.rowptr.data_ptr(), f.col.data_ptr(), f.val.data_ptr(), Xv.data_ptr(), Xv.stride(0),
                                         dYv.data_ptr(), dYv.stride(0), DV.t.data_ptr(), R.t.data_ptr(), n, H, fh,
                                         f.plan.data_ptr(), W.t.data_ptr(), s), "glass_spmm_dval_f32")
        self.dval, self.R, self.C = DV.t, R.t, None
        if adj.aggr == "gcn":
            C = out(n)
            nb = lib.glass_adj_colsum_ws_bytes(bh)
            assert nb == 4 * int(b.header[7])
            W = out(max(nb // 4, 4))
            L_.check(lib.glass_adj_colsum_f32(b.rowptr.data_ptr(), b.col.data_ptr(), b.val.data_ptr(), eid_t.data_ptr(),
                                              DV.t.data_ptr(), C.t.data_ptr(), n, bh, b.plan.data_ptr(), W.t.data_ptr(), s),
                     "glass_adj_colsum_f32")
            self.C = C.t
        DW = out(nnz)
        L_.check(lib.glass_adj_values_bwd_f32(f.rowptr.data_ptr(), f.col.data_ptr(), perm32.data_ptr(), adj.deg.data_ptr(),
                                              DV.t.data_ptr(), R.t.data_ptr(), None if self.C is None else self.C.data_ptr(), n,
                                              nnz, AGGR_CODE[adj.aggr], DW.t.data_ptr(), s), "glass_adj_values_bwd_f32")
        torch.cuda.synchronize()
        self.dw = DW.t

    def intact(self):
        return all(g.intact() for g in self.guards)

    def results(self):
        r = dict(dval=self.dval, R=self.R, dw=self.dw)
        if self.C is not None:
            r["C"] = self.C
        return r


def _share(got, want, mass, n):
    """the largest |got - want| / (gamma(n) mass); an element without mass must be exact (inf otherwise)"""
    d = np.abs(got.detach().cpu().double().numpy() - want)
    bound = gamma(n) * mass
    if not bool((d[mass == 0] == 0).all()):
        return float("inf")
    live = mass > 0
    return float((d[live] / bound[live]).max()) if bool(live.any()) else 0.0


def _grade(csr, w, aggr, val32, X, dY, res, H):
    """{name: share of its bound} for the results in `res`; val32 the fp32 values the kernels read (exact inputs)"""
    val = val32.cpu().double().numpy()
    dval, m_dval, R, m_R = EO.dval_R(csr, X.numpy(), dY.numpy(), val)
    n_i = np.diff(csr.rowptr)           # entries per row
    c_k = np.diff(csr.rowptr_t)         # entries per column
    e = {}
    if "dval" in res:
        e["dval"] = _share(res["dval"], dval, m_dval, H + 1)                                       # n = H + 1
    if "R" in res:
        e["R"] = _share(res["R"], R, m_R, H + 1 + n_i)                                             # n = H + 1 + n_i
    C = m_C = None
    if aggr == "gcn":
        C, m_C = EO.colsum(csr, dval, val, m_dval)
        if "C" in res:
            e["C"] = _share(res["C"], C, m_C, H + 1 + c_k)                                         # n = H + 1 + c_k
    dw, m_dw = EO.values_bwd(csr, w, aggr, dval, R, C, m_dval, m_R, m_C)
    ni, nj, ci = (np.empty(csr.nnz) for _ in range(3))
    ni[csr.perm], nj[csr.perm], ci[csr.perm] = n_i[csr.row], n_i[csr.col], c_k[csr.row]
    count = {"sum": H + 1 + 0 * ni,                                                                # n = H + 1
             "mean": H + 1 + 2 * ni + 2,                                                           # n = H + 1 + 2 n_i + 2
             "gcn": H + 1 + 3 * ni + nj + ci + 12}[aggr]                                           # n = H + 1 + 3 n_i + n_j + c_i + 12
    e["dw"] = _share(res["dw"], dw, m_dw, count)
    return e


@pytest.mark.parametrize("H,pad", CASES)
@pytest.mark.parametrize("kind", ("mixed", "all_long"))
def test_kernels_against_the_restatement_and_repeatability(kind, H, pad):
    csr = _csr(kind)
    n, ei, w = EO.graph(kind)
    X, dY = _operands(kind, H)
    Xd, dYd = _padded(X, pad), _padded(dY, pad)
    assert Xd.stride(0) == H + pad > H
    empty = torch.from_numpy(np.nonzero(np.diff(csr.rowptr) == 0)[0]).to(DEV)
    empty_t = torch.from_numpy(np.nonzero(np.diff(csr.rowptr_t) == 0)[0]).to(DEV)
    assert len(empty) >= 2 and len(empty_t) >= 1
    dval_bits = None
    for aggr in EO.AGGRS:
        adj = _adj(kind, aggr)
        run = Run(adj, Xd, dYd)
        res = run.results()
        assert run.intact(), (kind, H, pad, aggr, "guards of the results / workspaces")
        assert all(bool(torch.isfinite(v).all()) for v in res.values()), "every element written, no padding column read"
        assert bool((res["R"][empty] == 0).all()) and (aggr != "gcn" or bool((res["C"][empty_t] == 0).all()))
        res2 = Run(adj, Xd, dYd).results()
        for k in res:
            assert torch.equal(_bits(res[k]), _bits(res2[k])), (kind, H, pad, aggr, k, "two runs differ")
        if dval_bits is None:
            dval_bits = _bits(res["dval"]).clone()
        assert torch.equal(_bits(res["dval"]), dval_bits), "dval does not depend on the values"
        e = _grade(csr, w, aggr, adj.fwd.val, X, dY, res, H)
        print(f"{kind} H={H} ld={H + pad} {aggr}: share of the bound " + " ".join(f"{k} {v:.3f}" for k, v in e.items()))
        assert all(v <= 1.0 for v in e.values()), (kind, H, pad, aggr, e)
        if kind == "mixed":   # dw is in the caller's order: the duplicate pair's two slots hold the per-entry value, each
            pair = EO.pair_positions(ei)
            want = EO.edge_grad(csr, w, aggr, X.numpy(), dY.numpy())
            got = res["dw"].cpu().double().numpy()
            assert pair.shape == (2, ) and got[pair[0]] == got[pair[1]] != 0
            assert abs(got[pair[0]] - want[pair[0]]) < abs(got[pair[0]] - 2 * want[pair[0]]), "not a coalesced entry's sum"


class Counting:
    """the library handle, counting the calls of each entry"""
    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn):
            return fn

        def call(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)
        return call


EDGE_ENTRIES = ("glass_spmm_dval_f32", "glass_adj_colsum_f32", "glass_adj_values_bwd_f32")


@pytest.mark.parametrize("aggr", EO.AGGRS)
@pytest.mark.parametrize("H", (64, 17))
def test_spmm_w_against_spmm_and_the_restatement(aggr, H, monkeypatch):
    """A(w1) on the structure of an adjacency built from w0: forward and dX have the bits of an adjacency built from w1; dw
    is the restatement's, in the caller's order; without a gradient for w no edge kernel runs."""
    from glass_amd import graph, ops
    L_, lib = _lib()
    kind = "mixed"
    csr = _csr(kind)
    n, ei, w0 = EO.graph(kind)
    rng = np.random.Generator(np.random.PCG64(3))
    w1 = (w0 * rng.uniform(0.9, 1.1, w0.shape[0])).astype(np.float32)
    assert float(np.abs(EO.degrees(csr, w1)[0] - 0.5).min()) >= 1e-3
    adj0 = _adj(kind, aggr)
    adj1 = graph.CSRAdj(torch.from_numpy(ei).to(DEV), torch.from_numpy(w1).to(DEV), n, aggr)
    val0 = adj0.fwd.val.clone()
    X, G = _operands(kind, H)
    counting = Counting(lib)
    monkeypatch.setattr(L_, "load", lambda: counting)

    x = X.to(DEV).requires_grad_()
    wd = torch.from_numpy(w1).to(DEV).requires_grad_()
    y = ops.spmm_w(adj0, x, wd)
    y.backward(G.to(DEV))
    x1 = X.to(DEV).requires_grad_()
    y1 = ops.spmm(adj1, x1)
    y1.backward(G.to(DEV))
    assert torch.equal(_bits(y.detach()), _bits(y1.detach())), "forward bits"
    assert torch.equal(_bits(x.grad), _bits(x1.grad)), "dX bits"
    assert torch.equal(_bits(adj0.fwd.val), _bits(val0)), "the stored values are not touched"
    assert all(counting.calls.get(k, 0) == (1 if k != "glass_adj_colsum_f32" or aggr == "gcn" else 0) for k in EDGE_ENTRIES)
    e = _grade(csr, w1, aggr, adj1.fwd.val, X, G, {"dw": wd.grad}, H)
    print(f"spmm_w {aggr} H={H}: dw share of its bound {e['dw']:.3f}")
    assert e["dw"] <= 1.0
    # w without a gradient: dw is None, dX the same bits, and no edge kernel is launched; x without: no transposed product
    counting.calls.clear()
    x2 = X.to(DEV).requires_grad_()
    w2 = torch.from_numpy(w1).to(DEV)
    ops.spmm_w(adj0, x2, w2).backward(G.to(DEV))
    assert w2.grad is None and torch.equal(_bits(x2.grad), _bits(x1.grad))
    assert not any(k in counting.calls for k in EDGE_ENTRIES) and counting.calls["glass_spmm_csr_f32"] == 2
    counting.calls.clear()
    w3 = torch.from_numpy(w1).to(DEV).requires_grad_()
    ops.spmm_w(adj0, X.to(DEV), w3).backward(G.to(DEV))
    assert torch.equal(_bits(w3.grad), _bits(wd.grad)) and counting.calls["glass_spmm_csr_f32"] == 1


def test_refusals_come_before_any_launch(monkeypatch):
    from glass_amd import graph, ops
    L_, lib = _lib()
    n, ei, w = EO.graph("all_long")
    eid, wd = torch.from_numpy(ei).to(DEV), torch.from_numpy(w).to(DEV)
    others = {a: graph.CSRAdj(eid, wd, n, a) for a in ("max", "softmax", "gat")}
    adj = _adj("all_long", "mean")
    adj._edge_grad_state("test")
    x = torch.zeros(n, 8, device=DEV)
    counting = Counting(lib)
    monkeypatch.setattr(L_, "load", lambda: counting)
    for a, other in others.items():
        with pytest.raises(L_.GlassHipError, match=a):
            ops.spmm_w(other, x, wd)
    for bad in (wd[:-1], torch.from_numpy(w), wd.double(), wd.reshape(1, -1)):
        with pytest.raises(ValueError, match="spmm_w"):
            ops.spmm_w(adj, x, bad)
    assert counting.calls == {}
