"""K1a multi-head on the GPU: the glass_*_mh_* entries (csrc/spmm_gat_mh.hip) against the fp64 restatement
tests/aggr_gat_mh_oracle.py on every plan form and on the lane geometries a head can take, the host objects
(graph.CSRAdj.gat_*(heads=K), ops.spmm_gat(heads=K)), a GLASS model with gat_heads = 4 against an fp64 restatement of the model,
impl.train.train on the captured per-op step, and the driver.

The rule is tests/test_gpu_aggr_gat.py's: a, b, Y, L and dX at rel-inf <= 1e-5 against fp64; g, da, db and the vectors' gradients,
cancelling sums, element by element within 1e-5 of their mass (per head).  Run to run every entry gives the same bits.

Worst errors measured on an MI355X over the twenty cases of test_values_against_the_restatement_and_repeatability (both slopes):
a 4.7e-8, b 5.0e-8, Y 5.3e-7, L 1.3e-7, dX 9.3e-7; g 1.2e-6, da 1.1e-6, db 6.8e-7, datt_src 6.6e-8, datt_dst 5.4e-8 of their mass;
the model: loss 9.6e-8, logits 4.4e-7, flat gradient 4.2e-7 ("multi-head")."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import aggr_gat_mh_oracle as MO
import test_gpu_aggr_gat as T1
from aggr_max_oracle import rows_of
from helpers import rel_inf, flat_grads
from test_gpu_aggr_gat import Guarded, _adj, _graph, _of_mass, TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (H, K): heads of one lane (D = 4), of 2, 1, 2 and 8 lanes, 17 live lanes of 32, D = 128, two column tiles / passes with a nearly
# empty last one, and a head that is exactly one column pass (D = 256)
CASES = ((8, 2), (16, 2), (64, 16), (64, 8), (64, 2), (68, 17), (128, 8), (256, 2), (260, 65), (512, 2))
SLOPES = (0.2, 0.0)
NAMES = ("a", "b", "Y", "L", "g", "db", "dX", "da", "da_alone", "datt_src", "datt_dst")


_lib, _stream, _bits = T1._lib, T1._stream, T1._bits


class RunMH:
    """Every multi-head entry once, in the order of a forward and a backward, each result in a Guarded buffer (NaN-filled),
    every workspace in a Guarded buffer of NaN of exactly the queried size.  Operands are [n, H] views with any row stride.
    forward_only: the scores and the forward alone."""
    def __init__(self, adj, Xv, dYv, As, Ad, slope, K, ldy_extra=0, lddx_extra=0, off=0, forward_only=False):
        L_, lib = _lib()
        f, b = adj.fwd, adj.bwd
        n, H, nnz = f.n_rows, Xv.shape[1], f.nnz
        s = _stream()
        self.guards = []

        def out(numel, dtype=torch.float32, o=off):
            g = Guarded(numel, float("nan"), dtype, off=o)
            self.guards.append(g)
            return g

        def ws(nbytes, want, dtype=torch.float32):
            assert nbytes == want, (nbytes, want)
            size = 4 if dtype == torch.float32 else 8
            return out(max(nbytes // size, 4), dtype, 0)
        fh, bh = f.header.ctypes.data, b.header.ctypes.data
        fs, bs = int(f.header[7]), int(b.header[7])
        ldy, lddx = H + ldy_extra, H + lddx_extra
        A, B = out(n * K), out(n * K)
        L_.check(lib.glass_gat_scores_mh_f32(Xv.data_ptr(), Xv.stride(0), As.data_ptr(), Ad.data_ptr(), A.t.data_ptr(),
                                             B.t.data_ptr(), n, H, K, s), "glass_gat_scores_mh_f32")
        Y, L = out(n * ldy), out(n * K)
        W = ws(lib.glass_spmm_gat_mh_ws_bytes(fh, H, K), fs * (H + 2 * K) * 4)
        L_.check(lib.glass_spmm_gat_mh_csr_f32(f.rowptr.data_ptr(), f.col.data_ptr(), f.val.data_ptr(), Xv.data_ptr(), Xv.stride(0),
                                               A.t.data_ptr(), B.t.data_ptr(), slope, Y.t.data_ptr(), ldy, L.t.data_ptr(), n, H, K,
                                               fh, f.plan.data_ptr(), W.t.data_ptr(), s), "glass_spmm_gat_mh_csr_f32")
        self.a, self.b, self.L = A.t.view(n, K), B.t.view(n, K), L.t.view(n, K)
        self.Y, self.H, self.K = Y.t.view(n, ldy), H, K
        if forward_only:
            torch.cuda.synchronize()
            return
        Yv = self.Y[:, :H]
        G, DB = out(max(nnz * K, 1)), out(n * K)
        W = ws(lib.glass_spmm_gat_mh_edge_ws_bytes(fh, H, K), fs * K * 4)
        L_.check(lib.glass_spmm_gat_mh_edge_f32(f.rowptr.data_ptr(), f.col.data_ptr(), f.val.data_ptr(), Xv.data_ptr(),
                                                Xv.stride(0), A.t.data_ptr(), B.t.data_ptr(), slope, dYv.data_ptr(), dYv.stride(0),
                                                Yv.data_ptr(), ldy, L.t.data_ptr(), G.t.data_ptr(), DB.t.data_ptr(), n, H, K, fh,
                                                f.plan.data_ptr(), W.t.data_ptr(), s), "glass_spmm_gat_mh_edge_f32")
        DX, DA = out(n * lddx), out(n * K)
        W = ws(lib.glass_spmm_gat_mh_bwd_ws_bytes(bh, H, K), bs * (H + K) * 4)
        L_.check(lib.glass_spmm_gat_mh_bwd_f32(b.rowptr.data_ptr(), b.col.data_ptr(), b.val.data_ptr(), adj.eid_t.data_ptr(),
                                               A.t.data_ptr(), B.t.data_ptr(), slope, dYv.data_ptr(), dYv.stride(0), L.t.data_ptr(),
                                               G.t.data_ptr(), DB.t.data_ptr(), As.data_ptr(), Ad.data_ptr(), DX.t.data_ptr(), lddx,
                                               DA.t.data_ptr(), n, H, K, bh, b.plan.data_ptr(), W.t.data_ptr(), s),
                 "glass_spmm_gat_mh_bwd_f32")
        # da alone, in the lane layout the transposed pass took
        vec = dYv.stride(0) % 4 == 0 and lddx % 4 == 0 and dYv.data_ptr() % 16 == 0 and DX.t.data_ptr() % 16 == 0
        DA2 = out(n * K)
        W = ws(lib.glass_spmm_gat_mh_da_ws_bytes(bh, H, K), bs * K * 4)
        L_.check(lib.glass_spmm_gat_mh_da_f32(b.rowptr.data_ptr(), b.col.data_ptr(), b.val.data_ptr(), adj.eid_t.data_ptr(),
                                              G.t.data_ptr(), DA2.t.data_ptr(), n, H, K, int(vec), bh, b.plan.data_ptr(),
                                              W.t.data_ptr(), s), "glass_spmm_gat_mh_da_f32")
        DS, DD = out(H), out(H)
        rpw = 2 * H if H > 128 else 256
        W = ws(lib.glass_gat_datt_mh_ws_bytes(n, H), -(-n // rpw) * 2 * H * 8, torch.float64)
        L_.check(lib.glass_gat_datt_mh_f32(Xv.data_ptr(), Xv.stride(0), DA.t.data_ptr(), DB.t.data_ptr(), DS.t.data_ptr(),
                                           DD.t.data_ptr(), n, H, K, W.t.data_ptr(), s), "glass_gat_datt_mh_f32")
        torch.cuda.synchronize()
        self.g, self.db, self.da, self.da_alone = G.t[:nnz * K].view(nnz, K), DB.t.view(n, K), DA.t.view(n, K), DA2.t.view(n, K)
        self.datt_src, self.datt_dst = DS.t, DD.t
        self.dX = DX.t.view(n, lddx)

    def intact(self):
        return all(g.intact() for g in self.guards)

    def results(self):
        H = self.H
        return dict(a=self.a, b=self.b, Y=self.Y[:, :H], L=self.L, g=self.g, db=self.db, dX=self.dX[:, :H], da=self.da,
                    da_alone=self.da_alone, datt_src=self.datt_src, datt_dst=self.datt_dst)


@functools.lru_cache(maxsize=None)
def _operands(kind, H):
    """X, dY randn; the attention vectors uniform in +-0.5 (never changed afterwards: the tests share them)"""
    n = _graph(kind)[0]
    g = torch.Generator().manual_seed(7000 * H + (kind == "mixed"))
    return (torch.randn(n, H, generator=g), torch.randn(n, H, generator=g), torch.rand(H, generator=g) - 0.5,
            torch.rand(H, generator=g) - 0.5)


@functools.lru_cache(maxsize=None)
def _reference(kind, H, K, slope):
    """fp64 from the fp32 operands, computed once per case: (Y, L, a, b, the backward's namespace)"""
    ref = _adj(kind)[1]
    X, dY, As, Ad = (t.double() for t in _operands(kind, H))
    Y, L, a, b = MO.gat_mh_aggregate(ref.rowptr, ref.col, ref.val, X, As, Ad, slope, K)
    return Y, L, a, b, MO.gat_mh_aggregate_bwd(ref.rowptr, ref.col, ref.val, dY, X, Y, L, a, b, As, Ad, slope, K)


def _errors(res, Y, L, a, b, r):
    return dict(a=rel_inf(res["a"].cpu(), a), b=rel_inf(res["b"].cpu(), b), Y=rel_inf(res["Y"].cpu(), Y), L=rel_inf(res["L"].cpu(), L),
                dX=rel_inf(res["dX"].cpu(), r.dX), g=_of_mass(res["g"], r.g, r.mass_g), da=_of_mass(res["da"], r.da, r.mass_da),
                db=_of_mass(res["db"], r.db, r.mass_db), datt_src=_of_mass(res["datt_src"], r.datt_src, r.mass_datt_src),
                datt_dst=_of_mass(res["datt_dst"], r.datt_dst, r.mass_datt_dst))


@pytest.mark.parametrize("H,K", CASES)
@pytest.mark.parametrize("kind", ("mixed", "all_long"))
def test_values_against_the_restatement_and_repeatability(kind, H, K):
    adj, ref = _adj(kind)
    X, dY, As, Ad = _operands(kind, H)
    Xd, dYd, Asd, Add = X.to(DEV), dY.to(DEV), As.to(DEV), Ad.to(DEV)
    empty = (ref.rowptr[1:] == ref.rowptr[:-1]).nonzero().reshape(-1).to(DEV)
    empty_t = (ref.rowptr_t[1:] == ref.rowptr_t[:-1]).nonzero().reshape(-1).to(DEV)
    assert len(empty) >= 1
    for slope in SLOPES:
        Y, L, a, b, r = _reference(kind, H, K, slope)
        run = RunMH(adj, Xd, dYd, Asd, Add, slope, K)
        res = run.results()
        assert run.intact(), (kind, H, K, slope, "guards of the results / workspaces")
        assert bool((res["Y"][empty] == 0).all()) and bool((res["L"][empty] == 0).all()), "a row without entries"
        assert bool((res["db"][empty] == 0).all()) and bool((res["da"][empty_t] == 0).all())
        assert torch.equal(_bits(res["da"]), _bits(res["da_alone"])), (kind, H, K, slope, "da alone has other bits")
        res2 = RunMH(adj, Xd, dYd, Asd, Add, slope, K).results()
        for k in res:
            assert torch.equal(_bits(res[k]), _bits(res2[k])), (kind, H, K, slope, k, "two runs differ")
        e = _errors(res, Y, L, a, b, r)
        print(f"{kind} H={H} K={K} slope={slope}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + " (g .. datt: of their mass)")
        assert all(v <= TOL for v in e.values()), (kind, H, K, slope, e)


@pytest.mark.parametrize("H,K", ((64, 8), (260, 65)))
def test_heads_do_not_leak(H, K):
    """Head 1's columns of X, dY and both vectors replaced by other values: every element of every other head keeps its bits."""
    D = H // K
    mine = slice(D, 2 * D)
    for kind in ("mixed", "all_long"):
        adj, ref = _adj(kind)
        ops_ = [t.clone() for t in _operands(kind, H)]
        base = RunMH(adj, *(t.to(DEV) for t in ops_), 0.2, K).results()
        g = torch.Generator().manual_seed(99)
        for t in ops_:
            t[..., mine] = torch.randn(t[..., mine].shape, generator=g) * 0.7
        other = RunMH(adj, *(t.to(DEV) for t in ops_), 0.2, K).results()
        cols = torch.ones(H, dtype=torch.bool, device=DEV)
        cols[mine] = False
        heads = torch.ones(K, dtype=torch.bool, device=DEV)
        heads[1] = False
        for k in NAMES:
            keep = cols if k in ("Y", "dX", "datt_src", "datt_dst") else heads
            x, y = base[k][..., keep], other[k][..., keep]
            assert torch.equal(_bits(x), _bits(y)), (kind, H, K, k, "another head's element moved")
            x, y = base[k][..., ~keep], other[k][..., ~keep]
            assert not torch.equal(_bits(x), _bits(y)), (kind, H, K, k, "head 1 did not move")


@pytest.mark.parametrize("H,K", ((64, 8), (16, 2)))
def test_zero_vectors_have_the_bits_of_the_single_head_forward(H, K):
    """Every score is exactly 0 then, in every head and in the single-head kernel: the same sums in the same order."""
    L_, lib = _lib()
    for kind in ("mixed", "all_long"):
        adj, ref = _adj(kind)
        f = adj.fwd
        n = f.n_rows
        X = _operands(kind, H)[0].to(DEV)
        z = torch.zeros(H, device=DEV)
        run = RunMH(adj, X, X, z, z, 0.2, K, forward_only=True)
        assert bool((run.a == 0).all()) and bool((run.b == 0).all())
        y1, l1 = Guarded(n * H, float("nan")), Guarded(n, float("nan"))
        zero = torch.zeros(n, device=DEV)
        slots = int(f.header[7])
        ws = Guarded(max(slots * (H + 2), 4), float("nan"))
        assert lib.glass_spmm_gat_ws_bytes(f.header.ctypes.data, H) == slots * (H + 2) * 4
        L_.check(lib.glass_spmm_gat_csr_f32(f.rowptr.data_ptr(), f.col.data_ptr(), f.val.data_ptr(), X.data_ptr(), H, zero.data_ptr(),
                                            zero.data_ptr(), 0.2, y1.t.data_ptr(), H, l1.t.data_ptr(), n, H, f.header.ctypes.data,
                                            f.plan.data_ptr(), ws.t.data_ptr(), _stream()), "glass_spmm_gat_csr_f32")
        torch.cuda.synchronize()
        assert run.intact() and y1.intact() and l1.intact() and ws.intact()
        assert torch.equal(_bits(run.Y), _bits(y1.t.view(n, H))), (kind, H, K, "Y")
        for h in range(K):
            assert torch.equal(_bits(run.L[:, h]), _bits(l1.t)), (kind, H, K, h, "L")


def test_large_exponents_stay_finite():
    """X scaled by 1e4: scores of thousands.  Every head's max is subtracted, so everything stays finite, and Y, a convex
    combination per head, lies within its row's [min x, max x] up to rounding (1e-5 of the row's largest |x|: the rule)."""
    H, K = 64, 8
    for kind in ("mixed", "all_long"):
        adj, ref = _adj(kind)
        X, dY, As, Ad = _operands(kind, H)
        X = X * 1e4
        res = RunMH(adj, X.to(DEV), dY.to(DEV), As.to(DEV), Ad.to(DEV), 0.2, K).results()
        assert all(bool(torch.isfinite(v).all()) for v in res.values()), (kind, [k for k, v in res.items() if not bool(torch.isfinite(v).all())])
        rows = rows_of(ref.rowptr)
        idx = rows[:, None].expand(-1, H)
        lo = torch.zeros(ref.n, H).scatter_reduce(0, idx, X[ref.col], "amin", include_self=False)
        hi = torch.zeros(ref.n, H).scatter_reduce(0, idx, X[ref.col], "amax", include_self=False)
        slack = TOL * torch.maximum(lo.abs(), hi.abs())
        Yc = res["Y"].cpu()
        assert bool((Yc >= lo - slack).all()) and bool((Yc <= hi + slack).all()), kind


STRIDED = [(H, K, pads, off) for H, K in ((64, 8), (16, 4)) for pads, off in (((3, 1, 2, 5), 0), ((0, 0, 0, 0), 1), ((8, 4, 12, 4), 0))]
STRIDED += [(256, 2, (0, 0, 0, 0), 1), (512, 2, (3, 1, 2, 5), 0)]   # the scalar form's heads of two and four column passes


@pytest.mark.parametrize("H,K,pads,off", STRIDED)
def test_strided_and_unaligned_operands(H, K, pads, off):
    """X, dY, Y and dX as column slices of wider buffers (odd paddings take the scalar form, multiples of 4 keep the 16-byte
    one), and every operand one float past a 16-byte boundary (the scalar form at a width that has a vector one); the columns
    beyond H are neither read (NaN) nor written.  At D = 128 and 256 the scalar form's head spans two and four column passes."""
    adj, ref = _adj("mixed")
    px, pdy, py, pdx = pads
    X, dY, As, Ad = _operands("mixed", H)
    slope = 0.2
    Y, L, a, b, r = _reference("mixed", H, K, slope)

    def wide(src, pad):
        buf = torch.full((ref.n * (H + pad) + off + 4, ), float("nan"), device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + ref.n * (H + pad)].view(ref.n, H + pad)
        v[:, :H] = src.to(DEV)
        return v[:, :H]
    Xv, dYv = wide(X, px), wide(dY, pdy)
    assert Xv.data_ptr() % 16 == 4 * off
    run = RunMH(adj, Xv, dYv, T1._dev_vec(As, off), T1._dev_vec(Ad, off), slope, K, py, pdx, off)
    res = run.results()
    e = _errors(res, Y, L, a, b, r)
    print(f"H={H} K={K} pads={pads} off={off}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(v <= TOL for v in e.values()), e
    assert run.intact() and bool(torch.isnan(run.Y[:, H:]).all()) and bool(torch.isnan(run.dX[:, H:]).all())
    assert torch.equal(_bits(res["da"]), _bits(res["da_alone"]))


def test_a_call_without_rows_launches_nothing():
    L_, lib = _lib()
    rp = np.zeros(1, dtype=np.int32)
    words = ctypes.c_int64(0)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, 0, None, ctypes.byref(words)) == 0
    plan = np.zeros(words.value, dtype=np.int32)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, 0, plan.ctypes.data, ctypes.byref(words)) == 0
    pd = torch.from_numpy(plan).to(DEV)
    rpd = torch.zeros(1, dtype=torch.int32, device=DEV)
    H, K = 8, 2
    bufs = [Guarded(4 * H, float("nan")) for _ in range(14)]
    x, a, b, y, l, dy, g, db, dx, da, asrc, adst, ds, dd = (q.t.data_ptr() for q in bufs)
    h, s, r, p = plan.ctypes.data, _stream(), rpd.data_ptr(), pd.data_ptr()
    assert lib.glass_gat_scores_mh_f32(x, H, asrc, adst, a, b, 0, H, K, s) == 0
    assert lib.glass_spmm_gat_mh_csr_f32(r, None, None, x, H, a, b, 0.2, y, H, l, 0, H, K, h, p, None, s) == 0
    assert lib.glass_spmm_gat_mh_edge_f32(r, None, None, x, H, a, b, 0.2, dy, H, y, H, l, None, db, 0, H, K, h, p, None, s) == 0
    assert lib.glass_spmm_gat_mh_bwd_f32(r, None, None, None, a, b, 0.2, dy, H, l, None, db, asrc, adst, dx, H, da, 0, H, K, h, p,
                                         None, s) == 0
    assert lib.glass_spmm_gat_mh_da_f32(r, None, None, None, None, da, 0, H, K, 1, h, p, None, s) == 0
    assert lib.glass_gat_datt_mh_f32(x, H, da, db, ds, dd, 0, H, K, None, s) == 0
    torch.cuda.synchronize()
    assert all(q.intact() and bool(torch.isnan(q.t).all()) for q in bufs)


def test_autograd_binding_and_frozen_vectors(monkeypatch):
    from glass_amd import graph, ops
    adj, ref = _adj("mixed")
    n, ei, ew = _graph("mixed")
    H, K, slope = 32, 4, 0.2
    X, dY, As, Ad = _operands("mixed", H)
    # fp64 autograd through the direct statement on the raw edge list
    Xr, Asr, Adr = (t.double().requires_grad_(True) for t in (X, As, Ad))
    Yr = MO.scatter_gat_mh_aggregate(ei, ew.double(), n, Xr, Asr, Adr, slope, K)
    dXr, dsr, ddr = torch.autograd.grad(Yr, (Xr, Asr, Adr), dY.double())
    mass = _reference("mixed", H, K, slope)[4]
    calls = {"datt": 0, "bwd": 0, "da": 0}
    for name, key in (("gat_datt", "datt"), ("gat_bwd", "bwd"), ("gat_da", "da")):
        real = getattr(graph.CSRAdj, name)

        def counted(self, *a_, _real=real, _key=key, **kw):
            assert kw == {"heads": K}
            calls[_key] += 1
            return _real(self, *a_, **kw)
        monkeypatch.setattr(graph.CSRAdj, name, counted)
    Xd = X.to(DEV).requires_grad_(True)
    s1, d1 = nn.Parameter(As.to(DEV)), nn.Parameter(Ad.to(DEV))
    out = ops.spmm_gat(adj, Xd, s1, d1, slope, heads=K)
    out.backward(dY.to(DEV))
    assert out.shape == (n, H)
    assert rel_inf(out.detach().cpu(), Yr.detach()) <= TOL and rel_inf(Xd.grad.cpu(), dXr) <= TOL
    assert s1.grad.shape == (H, ) and _of_mass(s1.grad, dsr, mass.mass_datt_src) <= TOL
    assert d1.grad.shape == (H, ) and _of_mass(d1.grad, ddr, mass.mass_datt_dst) <= TOL
    assert calls == {"datt": 1, "bwd": 1, "da": 0}
    # frozen: no column-reduction launch, no .grad, the same dX bits
    X2 = X.to(DEV).requires_grad_(True)
    s2, d2 = nn.Parameter(As.to(DEV)).requires_grad_(False), nn.Parameter(Ad.to(DEV)).requires_grad_(False)
    ops.spmm_gat(adj, X2, s2, d2, slope, heads=K).backward(dY.to(DEV))
    assert s2.grad is None and d2.grad is None and calls == {"datt": 1, "bwd": 2, "da": 0}
    assert torch.equal(_bits(X2.grad), _bits(Xd.grad))
    # only the vectors: no transposed pass, the same gradient bits
    s3, d3 = nn.Parameter(As.to(DEV)), nn.Parameter(Ad.to(DEV))
    ops.spmm_gat(adj, X.to(DEV), s3, d3, slope, heads=K).backward(dY.to(DEV))
    assert calls == {"datt": 2, "bwd": 2, "da": 1}
    assert torch.equal(_bits(s3.grad), _bits(s1.grad)) and torch.equal(_bits(d3.grad), _bits(d1.grad))
    # a head count the kernels do not serve is refused before any launch
    for bad in (3, 16):   # 32 / 3 is not whole; D = 2
        with pytest.raises(ValueError, match="heads"):
            ops.spmm_gat(adj, X.to(DEV), s3, d3, slope, heads=bad)


# ---- through the model ----------------------------------------------------------------------------------------------------
MODEL_SEEDS = (11, 5)   # (graph, weights): chosen on the fp64 oracle alone, see the assertion on the heads' gradients
HEADS = 4


def model_and_oracle(graph_seed, weight_seed, hidden=64):
    """tests/test_gpu_aggr_gat.py's, with gat_heads = 4 and GatMHAdj in the oracle's layers"""
    from helpers import build_glass
    from oracle import glass_oracle as O
    N, ei, ew, x, pos, y = T1.model_graph(graph_seed)
    torch.manual_seed(weight_seed)
    model = build_glass(hidden, 2, int(x.max()), 3, "gat", "mean", 0.8, dropout=0.0, jk=True, gat_heads=HEADS)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    att_keys = sorted(k for k in sd if ".att_" in k)
    assert att_keys == ["conv.convs.0.att_dst", "conv.convs.0.att_src", "conv.convs.1.att_dst", "conv.convs.1.att_src"]
    orc = O.OracleGLASS(hidden, 2, int(x.max()), 3, aggr="sum", pool="mean", z_ratio=0.8).double()
    orc.load_state_dict({k: v for k, v in sd.items() if k not in att_keys})
    orc.train()
    att = {k: sd[k].double().requires_grad_(True) for k in att_keys}
    for l, conv in enumerate(orc.conv.convs):
        conv.adj = MO.GatMHAdj(ei, ew.double(), N, att[f"conv.convs.{l}.att_src"], att[f"conv.convs.{l}.att_dst"], 0.2, HEADS)
    logits_ref = orc(x, ei, ew.double(), pos, O.max_zero_one(x, pos))
    loss_ref = nn.CrossEntropyLoss()(logits_ref, y)
    loss_ref.backward()
    grads_ref = {k: p.grad.clone() for k, p in orc.named_parameters()}
    grads_ref.update({k: v.grad.clone() for k, v in att.items()})
    return model, logits_ref.detach(), loss_ref.item(), grads_ref, att_keys, (N, ei, ew, x, pos, y)


def test_model_with_four_heads_against_the_fp64_restatement():
    """Two GLASSConv layers at hidden 64 with four heads of 16 channels, jk, no dropout: loss, logits and the flat gradient over
    all parameters, the four attention vectors included."""
    from impl import utils
    model, logits_ref, loss_ref, grads_ref, att_keys, (N, ei, ew, x, pos, y) = model_and_oracle(*MODEL_SEEDS)
    keys = sorted(grads_ref)
    gmax = float(flat_grads(grads_ref, keys).abs().max())
    shares = {(k, h): float(grads_ref[k].view(HEADS, -1)[h].abs().max()) / gmax for k in att_keys for h in range(HEADS)}
    print("largest gradient of each head of each attention vector, of the largest gradient overall (fp64 oracle):",
          {f"{k}[{h}]": f"{v:.2e}" for (k, h), v in shares.items()})
    assert all(v > 1e-3 for v in shares.values()), "every head's gradient must count in the flat metric"

    model.to(DEV).train()
    xg, eig, ewg, posg, yg = (a.to(DEV) for a in (x, ei, ew, pos, y))
    logits = model(xg, eig, ewg, posg, utils.MaxZOZ(xg, posg), id=0)
    loss = nn.CrossEntropyLoss()(logits, yg)
    loss.backward()
    torch.cuda.synchronize()
    assert all(c.adj.aggr == "gat" and c.gat_heads == HEADS for c in model.conv.convs)
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    assert set(keys) == set(mine)
    e_logits = rel_inf(logits.detach().cpu(), logits_ref)
    e_loss = abs(loss.item() - loss_ref) / abs(loss_ref)
    e_grad = rel_inf(flat_grads(mine, keys), flat_grads(grads_ref, keys))
    for k in att_keys:
        print(f"{k}: error {float((mine[k].double() - grads_ref[k]).abs().max()) / gmax:.2e} of the largest gradient {gmax:.3e}")
    print(f"loss {e_loss:.2e} logits {e_logits:.2e} flat gradient {e_grad:.2e}")
    assert e_loss <= TOL and e_logits <= TOL and e_grad <= TOL


@pytest.mark.parametrize("frozen", (False, True))
def test_training_on_the_captured_per_op_step_equals_its_eager_run(monkeypatch, frozen):
    """Two epochs of impl.train.train at aggr "gat" with four heads (tests/test_gpu_aggr_gat.py's test, its tiny dataset): the
    captured per-op step and a deep copy trained with eager launches end with the same losses and parameters, bit for bit; the
    attention vectors have moved (frozen: they have not, and the column reductions never ran)."""
    from helpers import build_glass
    from impl import SubGDataset, train, utils
    from glass_amd import graph, stack, train as gtrain
    w, x, ei, ew, pos, y = T1._tiny(2, 2)
    torch.manual_seed(3)
    gnn = build_glass(64, 2, int(x.max()), w.n_class, "gat", w.pool, w.z_ratio, gat_heads=HEADS).to(DEV)
    vectors = lambda net: [v for c in net.conv.convs for v in (c.att_src, c.att_dst)]
    if frozen:
        for v in vectors(gnn):
            v.requires_grad_(False)
    initial = [v.detach().clone() for v in vectors(gnn)]
    twin = copy.deepcopy(gnn)
    calls = []
    real = graph.CSRAdj.gat_datt

    def counted(self, *a, **kw):
        assert kw == {"heads": HEADS}
        calls.append(1)
        return real(self, *a, **kw)
    monkeypatch.setattr(graph.CSRAdj, "gat_datt", counted)
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
        assert not stack.StackProgram.supported(net.conv) and all(c.adj.aggr == "gat" and c.gat_heads == HEADS for c in net.conv.convs)
    assert bool(calls) != frozen
    assert np.isfinite(out["graph"]).all() and out["graph"][1] != out["graph"][0]
    assert np.array_equal(np.float32(out["graph"]).view(np.int32), np.float32(out["eager"]).view(np.int32)), out
    sd, sd2 = gnn.state_dict(), twin.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    for v, v0 in zip(vectors(gnn), initial):
        moved = not torch.equal(_bits(v.detach()), _bits(v0))
        assert moved != frozen


def test_driver_runs_with_four_heads(capsys, monkeypatch):
    """GLASSTest.main with --aggr gat --gat_heads 4 on density, two epochs.  The shipped config has hidden_dim 8, where four heads
    would be two channels wide — refused at construction, which is checked first; the run itself takes the config at hidden_dim
    16 (heads of four channels), handed in where the driver reads its YAML."""
    import GLASSTest
    argv = ["--use_one", "--use_seed", "--use_maxzeroone", "--repeat", "1", "--device", "0", "--dataset", "density",
            "--max_epoch", "2", "--aggr", "gat", "--gat_heads", "4"]
    with pytest.raises(ValueError, match="heads"):
        GLASSTest.main(argv)
    capsys.readouterr()
    real = GLASSTest.yaml.safe_load
    monkeypatch.setattr(GLASSTest.yaml, "safe_load", lambda f: dict(real(f), hidden_dim=16))
    GLASSTest.main(argv)
    text = capsys.readouterr().out
    assert "gat_heads=4" in text and "'hidden_dim': 16" in text and "end: epoch" in text and "average " in text
