"""K1a on the GPU: glass_gat_scores_f32, glass_spmm_gat_csr_f32 / _edge_f32 / _bwd_f32 / _da_f32 and glass_gat_datt_f32
(csrc/spmm_gat.hip) against the fp64 restatement tests/aggr_gat_oracle.py on every plan form and lane layout, the host objects
(graph.CSRAdj.gat_*, ops.spmm_gat), a GLASS model with aggr "gat" against an fp64 restatement of the model, and
impl.train.train on the captured per-op step, whose replays must read the live attention vectors.

Y, L and dX are compared at rel-inf <= 1e-5 against fp64; g, da, db and the vectors' gradients, cancelling sums,
by the same rule applied to a sum, element by element: |got - ref| <= 1e-5 * (the sum of the absolute values of the terms).  Run
to run every entry gives the same bits."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import aggr_gat_oracle as GO
from aggr_max_oracle import MaxAdj, rows_of
from helpers import rel_inf, flat_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
GUARD = 64
WIDTHS = (4, 18, 64, 68, 128, 132, 256, 260)   # every VW / LPR case, two column tiles / column passes
SLOPES = (0.2, 0.0, 1.0)


def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """`n` elements filled with `fill`, GUARD sentinel elements in front and behind (tests/test_gpu_aggr_softmax.py's); `off`
    more filled elements in front of the view `t`, which then starts `off` elements past a 16-byte boundary"""
    def __init__(self, n, fill, dtype=torch.float32, off=0):
        self.buf = torch.empty(n + off + 2 * GUARD, dtype=dtype, device=DEV)
        self.sentinel = (torch.arange(2 * GUARD, device=DEV) * 3 - 11).to(dtype)
        self.buf[:GUARD] = self.sentinel[:GUARD]
        self.buf[GUARD + off + n:] = self.sentinel[GUARD:]
        self.pad = self.buf[GUARD:GUARD + off]
        self.t = self.buf[GUARD + off:GUARD + off + n]
        self.pad.fill_(fill)
        self.t.fill_(fill)
        self.fill = fill
        assert self.buf[GUARD:].data_ptr() % 16 == 0

    def intact(self):
        n = self.t.numel() + self.pad.numel()
        same = torch.isnan(self.pad).all() if self.fill != self.fill else (self.pad == self.fill).all()
        return (torch.equal(self.buf[:GUARD], self.sentinel[:GUARD]) and torch.equal(self.buf[GUARD + n:], self.sentinel[GUARD:])
                and bool(same))


# ---- the two adjacencies (the generator of tests/test_gpu_aggr_softmax.py) ---------------------------------------------------
def _edges(degrees, n, rng, hub_share, hub_frac=0.0):
    """One destination row per entry of `degrees`; sources uniform, except that a share of the rows also names source 5, and a
    fraction of all entries (a hub: its row of the TRANSPOSED matrix is long and cut).  Not symmetric.  Weights in [0.25, 2)."""
    rows, cols = [], []
    for r, d in enumerate(degrees):
        c = rng.integers(0, n, d)
        if d and rng.random() < hub_share:
            c[rng.integers(0, d)] = 5
        rows.append(np.full(d, r))
        cols.append(c)
    row, col = np.concatenate(rows), np.concatenate(cols)
    col[rng.random(col.shape[0]) < hub_frac] = 5
    w = rng.uniform(0.25, 2.0, row.shape[0]).astype(np.float32)
    return row, col, w


@functools.lru_cache(maxsize=None)
def _graph(kind):
    """-> (n, edge_index, edge_weight) on the host, in SHUFFLED edge order (CSRAdj sorts).
    mixed: rows of 0, 1, 2, 63, 64, 65, 255, 256, 257 and 700 in-entries (both sides of the long-row threshold, 257 and 700 are
      cut, 700 into three chunks), then 997 short rows of 1..12 (sweep items), a duplicate (row, col) pair with different
      weights, a self-loop; source 5 is a hub, so its row of the transposed matrix is cut.
    all_long: 40 rows of 64..300 entries, one of 700, one empty — fewer than 1 024 rows, nnz >= 64 n: no sweep at all."""
    rng = np.random.Generator(np.random.PCG64(17 if kind == "mixed" else 18))
    if kind == "mixed":
        degrees = [0, 1, 2, 63, 64, 65, 255, 256, 257, 700] + list(rng.integers(1, 13, 997))
        n = len(degrees)
        row, col, w = _edges(degrees, n, rng, 0.7)
        extra_r, extra_c = np.array([20, 20, 30]), np.array([40, 40, 30])      # (20, 40) twice; self-loop (30, 30)
        extra_w = np.array([0.5, 1.25, 0.75], dtype=np.float32)
        row, col, w = np.concatenate((row, extra_r)), np.concatenate((col, extra_c)), np.concatenate((w, extra_w))
    else:
        degrees = list(rng.integers(64, 301, 38)) + [700, 0] + [200, 200]
        n = len(degrees)
        row, col, w = _edges(degrees, n, rng, 0.0, 0.2)
    perm = rng.permutation(row.shape[0])
    ei = torch.from_numpy(np.stack((row[perm], col[perm])).astype(np.int64))
    return n, ei, torch.from_numpy(w[perm].copy())


@functools.lru_cache(maxsize=None)
def _adj(kind):
    """(graph.CSRAdj on the device, the sorted CSR of the restatement in fp64, both from the same shuffled edge list)"""
    from glass_amd import graph
    n, ei, ew = _graph(kind)
    adj = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "gat")
    return adj, MaxAdj(ei, ew.double(), n)


def test_plans_take_every_form_and_the_weight_rule():
    from glass_amd import graph
    for kind in ("mixed", "all_long"):
        adj, ref = _adj(kind)
        assert adj.aggr == "gat"
        for got, want in ((adj.fwd.rowptr, ref.rowptr), (adj.fwd.col, ref.col), (adj.bwd.rowptr, ref.rowptr_t),
                          (adj.bwd.col, ref.col_t), (adj.eid_t, ref.eid_t)):
            assert got.dtype == torch.int32 and torch.equal(got.cpu().to(torch.int64), want)
        assert torch.equal(adj.fwd.val.cpu().double(), ref.val) and torch.equal(adj.bwd.val.cpu().double(), ref.val_t)  # raw weights
        assert float(ref.val.min()) >= 0.25 and not torch.equal(ref.rowptr, ref.rowptr_t)
    n, ei, ew = _graph("mixed")
    assert n == 1007 and bool(((ei[0] == 30) & (ei[1] == 30)).any())
    dup = (ei[0] == 20) & (ei[1] == 40)
    assert int(dup.sum()) >= 2 and len(set(ew[dup].tolist())) >= 2
    f, b = _adj("mixed")[0].fwd.header, _adj("mixed")[0].bwd.header
    # header words (tests/test_cabi.py): 4 sweep items, 5 long items, 6 reduce rows, 7 partial slots, 8 threshold, 9 chunk
    assert f[4] > 100 and f[5] >= 9 and f[6] == 2 and f[7] == 2 + 3 and f[8] == 64 and f[9] == 256
    assert b[4] > 100 and b[5] >= 3 and b[6] >= 1 and b[7] >= 3, "the hub's transposed row is cut"
    for h in (_adj("all_long")[0].fwd.header, _adj("all_long")[0].bwd.header):
        assert h[4] == 0 and h[8] == 0 and h[5] >= 42 and h[6] >= 1 and h[7] >= 2, "no sweep, every row workgroup items, cut rows"
    # weights are multiplicities: zero, negative and NaN are refused at build, with one device read
    n, ei, ew = _graph("all_long")
    for bad in (0.0, -1.0, float("nan")):
        w = ew.clone()
        w[3] = bad
        with pytest.raises(ValueError, match="strictly positive"):
            graph.CSRAdj(ei.to(DEV), w.to(DEV), n, "gat")
    _L, _ = _lib()
    other = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "softmax")
    with pytest.raises(_L.GlassHipError, match="not 'gat'"):
        other.gat_scores(torch.zeros(n, 4, device=DEV), torch.zeros(4, device=DEV), torch.zeros(4, device=DEV))


# ---- raw entries on guarded buffers --------------------------------------------------------------------------------------
def _dev_vec(v, off=0):
    """a vector on the device, `off` floats past a 16-byte boundary"""
    buf = torch.empty(v.numel() + off + 4, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = buf[off:off + v.numel()]
    out.copy_(v)
    return out


class Run:
    """Every entry of K1a once, in the order of a forward and a backward, each result in a Guarded buffer (NaN-filled), every
    workspace in a Guarded buffer of NaN (it need not be initialised).  Operands are [n, H] views with any row stride."""
    def __init__(self, adj, Xv, dYv, As, Ad, slope, ldy_extra=0, lddx_extra=0, off=0):
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
        A, B = out(n), out(n)
        L_.check(lib.glass_gat_scores_f32(Xv.data_ptr(), Xv.stride(0), As.data_ptr(), Ad.data_ptr(), A.t.data_ptr(), B.t.data_ptr(),
                                          n, H, s), "glass_gat_scores_f32")
        Y, L = out(n * ldy), out(n)
        W = ws(lib.glass_spmm_gat_ws_bytes(fh, H), fs * (H + 2) * 4)
        L_.check(lib.glass_spmm_gat_csr_f32(f.rowptr.data_ptr(), f.col.data_ptr(), f.val.data_ptr(), Xv.data_ptr(), Xv.stride(0),
                                            A.t.data_ptr(), B.t.data_ptr(), slope, Y.t.data_ptr(), ldy, L.t.data_ptr(), n, H, fh,
                                            f.plan.data_ptr(), W.t.data_ptr(), s), "glass_spmm_gat_csr_f32")
        Yv = Y.t.view(n, ldy)[:, :H]
        G, DB = out(nnz), out(n)
        W = ws(lib.glass_spmm_gat_edge_ws_bytes(fh, H), fs * 4)
        L_.check(lib.glass_spmm_gat_edge_f32(f.rowptr.data_ptr(), f.col.data_ptr(), f.val.data_ptr(), Xv.data_ptr(), Xv.stride(0),
                                             A.t.data_ptr(), B.t.data_ptr(), slope, dYv.data_ptr(), dYv.stride(0), Yv.data_ptr(),
                                             ldy, L.t.data_ptr(), G.t.data_ptr(), DB.t.data_ptr(), n, H, fh, f.plan.data_ptr(),
                                             W.t.data_ptr(), s), "glass_spmm_gat_edge_f32")
        DX, DA = out(n * lddx), out(n)
        W = ws(lib.glass_spmm_gat_bwd_ws_bytes(bh, H), bs * (H + 1) * 4)
        L_.check(lib.glass_spmm_gat_bwd_f32(b.rowptr.data_ptr(), b.col.data_ptr(), b.val.data_ptr(), adj.eid_t.data_ptr(),
                                            A.t.data_ptr(), B.t.data_ptr(), slope, dYv.data_ptr(), dYv.stride(0), L.t.data_ptr(),
                                            G.t.data_ptr(), DB.t.data_ptr(), As.data_ptr(), Ad.data_ptr(), DX.t.data_ptr(), lddx,
                                            DA.t.data_ptr(), n, H, bh, b.plan.data_ptr(), W.t.data_ptr(), s),
                 "glass_spmm_gat_bwd_f32")
        # da alone, in the lane layout the transposed pass took
        vec = H % 4 == 0 and dYv.stride(0) % 4 == 0 and lddx % 4 == 0 and dYv.data_ptr() % 16 == 0 and DX.t.data_ptr() % 16 == 0
        DA2 = out(n)
        W = ws(lib.glass_spmm_gat_da_ws_bytes(bh, H), bs * 4)
        L_.check(lib.glass_spmm_gat_da_f32(b.rowptr.data_ptr(), b.col.data_ptr(), b.val.data_ptr(), adj.eid_t.data_ptr(),
                                           G.t.data_ptr(), DA2.t.data_ptr(), n, H, int(vec), bh, b.plan.data_ptr(),
                                           W.t.data_ptr(), s), "glass_spmm_gat_da_f32")
        DS, DD = out(H), out(H)
        rpw = 2 * H if H > 128 else 256
        W = ws(lib.glass_gat_datt_ws_bytes(n, H), -(-n // rpw) * 2 * H * 8, torch.float64)
        L_.check(lib.glass_gat_datt_f32(Xv.data_ptr(), Xv.stride(0), DA.t.data_ptr(), DB.t.data_ptr(), DS.t.data_ptr(),
                                        DD.t.data_ptr(), n, H, W.t.data_ptr(), s), "glass_gat_datt_f32")
        torch.cuda.synchronize()
        self.a, self.b, self.L, self.g, self.db, self.da, self.da_alone = A.t, B.t, L.t, G.t, DB.t, DA.t, DA2.t
        self.datt_src, self.datt_dst = DS.t, DD.t
        self.Y, self.dX = Y.t.view(n, ldy), DX.t.view(n, lddx)
        self.H = H

    def intact(self):
        return all(g.intact() for g in self.guards)

    def results(self):
        H = self.H
        return dict(a=self.a, b=self.b, Y=self.Y[:, :H], L=self.L, g=self.g, db=self.db, dX=self.dX[:, :H], da=self.da,
                    da_alone=self.da_alone, datt_src=self.datt_src, datt_dst=self.datt_dst)


@functools.lru_cache(maxsize=None)
def _operands(kind, H):
    """X, dY randn; the attention vectors uniform in +-0.5"""
    n = _graph(kind)[0]
    g = torch.Generator().manual_seed(1000 * H + (kind == "mixed"))
    return (torch.randn(n, H, generator=g), torch.randn(n, H, generator=g), torch.rand(H, generator=g) - 0.5,
            torch.rand(H, generator=g) - 0.5)


def _reference(ref, X, dY, As, Ad, slope):
    """fp64 from the fp32 operands: (Y, L, a, b, the backward's namespace)"""
    X, dY, As, Ad = X.double(), dY.double(), As.double(), Ad.double()
    Y, L, a, b = GO.gat_aggregate(ref.rowptr, ref.col, ref.val, X, As, Ad, slope)
    return Y, L, a, b, GO.gat_aggregate_bwd(ref.rowptr, ref.col, ref.val, dY, X, Y, L, a, b, As, Ad, slope)


def _of_mass(got, want, mass):
    """the largest |got - want| / mass; an element without mass must be exact (inf otherwise)"""
    d = (got.detach().cpu().double() - want).abs()
    ok0 = bool((d[mass == 0] == 0).all())
    live = mass > 0
    worst = float((d[live] / mass[live]).max()) if bool(live.any()) else 0.0
    return worst if ok0 else float("inf")


def _errors(res, Y, L, a, b, r):
    return dict(a=rel_inf(res["a"].cpu(), a), b=rel_inf(res["b"].cpu(), b), Y=rel_inf(res["Y"].cpu(), Y), L=rel_inf(res["L"].cpu(), L),
                dX=rel_inf(res["dX"].cpu(), r.dX), g=_of_mass(res["g"], r.g, r.mass_g), da=_of_mass(res["da"], r.da, r.mass_da),
                db=_of_mass(res["db"], r.db, r.mass_db), datt_src=_of_mass(res["datt_src"], r.datt_src, r.mass_datt_src),
                datt_dst=_of_mass(res["datt_dst"], r.datt_dst, r.mass_datt_dst))


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("kind", ("mixed", "all_long"))
def test_values_against_the_restatement_and_repeatability(kind, H):
    adj, ref = _adj(kind)
    X, dY, As, Ad = _operands(kind, H)
    Xd, dYd, Asd, Add = X.to(DEV), dY.to(DEV), As.to(DEV), Ad.to(DEV)
    empty = (ref.rowptr[1:] == ref.rowptr[:-1]).nonzero().reshape(-1).to(DEV)
    empty_t = (ref.rowptr_t[1:] == ref.rowptr_t[:-1]).nonzero().reshape(-1).to(DEV)
    assert len(empty) >= 1
    for slope in SLOPES:
        Y, L, a, b, r = _reference(ref, X, dY, As, Ad, slope)
        run = Run(adj, Xd, dYd, Asd, Add, slope)
        res = run.results()
        assert run.intact(), (kind, H, slope, "guards of the results / workspaces")
        assert bool((res["Y"][empty] == 0).all()) and bool((res["L"][empty] == 0).all()), "a row without entries"
        assert bool((res["db"][empty] == 0).all()) and bool((res["da"][empty_t] == 0).all())
        assert torch.equal(_bits(res["da"]), _bits(res["da_alone"])), (kind, H, slope, "da alone has other bits")
        res2 = Run(adj, Xd, dYd, Asd, Add, slope).results()
        for k in res:
            assert torch.equal(_bits(res[k]), _bits(res2[k])), (kind, H, slope, k, "two runs differ")
        e = _errors(res, Y, L, a, b, r)
        print(f"{kind} H={H} slope={slope}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()) + " (g .. datt: of their mass)")
        assert all(v <= TOL for v in e.values()), (kind, H, slope, e)
        if slope == 1.0:   # b cancels in a row's softmax: db is rounding only, and its mass says how much that may be
            assert float(r.db.abs().max()) <= 1e-12 * float(r.mass_db.max())


@pytest.mark.parametrize("H", (64, 18))
def test_large_exponents_stay_finite(H):
    """X scaled by 1e4: scores of tens of thousands.  The max is always subtracted, so everything stays finite, and Y, a convex
    combination, lies within its row's [min x, max x] up to rounding (1e-5 of the row's largest |x|: the rule)."""
    for kind in ("mixed", "all_long"):
        adj, ref = _adj(kind)
        X, dY, As, Ad = _operands(kind, H)
        X = X * 1e4
        res = Run(adj, X.to(DEV), dY.to(DEV), As.to(DEV), Ad.to(DEV), 0.2).results()
        assert all(bool(torch.isfinite(v).all()) for v in res.values()), (kind, H, [k for k, v in res.items() if not bool(torch.isfinite(v).all())])
        rows = rows_of(ref.rowptr)
        idx = rows[:, None].expand(-1, H)
        lo = torch.zeros(ref.n, H).scatter_reduce(0, idx, X[ref.col], "amin", include_self=False)
        hi = torch.zeros(ref.n, H).scatter_reduce(0, idx, X[ref.col], "amax", include_self=False)
        slack = TOL * torch.maximum(lo.abs(), hi.abs())
        Yc = res["Y"].cpu()
        assert bool((Yc >= lo - slack).all()) and bool((Yc <= hi + slack).all()), (kind, H)


@pytest.mark.parametrize("H", (64, 18))
def test_zero_vectors_agree_with_softmax_aggregation_at_t_zero(H):
    """Both are then the weighted mean of the neighbour messages, from different kernels on the same CSR."""
    from glass_amd import graph, ops
    for kind in ("mixed", "all_long"):
        adj, ref = _adj(kind)
        n, ei, ew = _graph(kind)
        sm = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "softmax")
        X = _operands(kind, H)[0].to(DEV)
        z = torch.zeros(H, device=DEV)
        y = ops.spmm_gat(adj, X, z, z, 0.2)
        want = ops.spmm_softmax(sm, X, torch.zeros(1, device=DEV))
        err = rel_inf(y.cpu(), want.cpu())
        print(f"{kind} H={H}: zero attention vectors against softmax aggregation at t = 0: {err:.2e}")
        assert err <= TOL


@pytest.mark.parametrize("H,pads,off", [(64, (8, 4, 12, 4), 0), (64, (3, 1, 2, 5), 0), (18, (2, 6, 1, 3), 0), (64, (0, 0, 0, 0), 1),
                                        (64, (4, 4, 4, 4), 3)])
def test_strided_and_unaligned_operands(H, pads, off):
    """X, dY, Y and dX as column slices of wider buffers (multiples of 4 keep the 16-byte form, anything else takes the scalar
    one), and every operand `off` floats past a 16-byte boundary (the scalar form at a width that has a vector one); the
    columns beyond H are neither read (NaN) nor written."""
    adj, ref = _adj("mixed")
    px, pdy, py, pdx = pads
    X, dY, As, Ad = _operands("mixed", H)
    slope = 0.2
    Y, L, a, b, r = _reference(ref, X, dY, As, Ad, slope)

    def wide(src, pad):
        buf = torch.full((ref.n * (H + pad) + off + 4, ), float("nan"), device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + ref.n * (H + pad)].view(ref.n, H + pad)
        v[:, :H] = src.to(DEV)
        return v[:, :H]
    Xv, dYv = wide(X, px), wide(dY, pdy)
    assert Xv.data_ptr() % 16 == 4 * off
    run = Run(adj, Xv, dYv, _dev_vec(As, off), _dev_vec(Ad, off), slope, py, pdx, off)
    res = run.results()
    e = _errors(res, Y, L, a, b, r)
    print(f"H={H} pads={pads} off={off}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
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
    H = 8
    bufs = [Guarded(4 * H, float("nan")) for _ in range(14)]
    x, a, b, y, l, dy, g, db, dx, da, asrc, adst, ds, dd = (q.t.data_ptr() for q in bufs)
    h, s, r, p = plan.ctypes.data, _stream(), rpd.data_ptr(), pd.data_ptr()
    assert lib.glass_gat_scores_f32(x, H, asrc, adst, a, b, 0, H, s) == 0
    assert lib.glass_spmm_gat_csr_f32(r, None, None, x, H, a, b, 0.2, y, H, l, 0, H, h, p, None, s) == 0
    assert lib.glass_spmm_gat_edge_f32(r, None, None, x, H, a, b, 0.2, dy, H, y, H, l, None, db, 0, H, h, p, None, s) == 0
    assert lib.glass_spmm_gat_bwd_f32(r, None, None, None, a, b, 0.2, dy, H, l, None, db, asrc, adst, dx, H, da, 0, H, h, p, None, s) == 0
    assert lib.glass_spmm_gat_da_f32(r, None, None, None, None, da, 0, H, 1, h, p, None, s) == 0
    assert lib.glass_gat_datt_f32(x, H, da, db, ds, dd, 0, H, None, s) == 0
    torch.cuda.synchronize()
    assert all(q.intact() and bool(torch.isnan(q.t).all()) for q in bufs)


def test_autograd_binding_and_frozen_vectors(monkeypatch):
    from glass_amd import graph, ops
    L_, _ = _lib()
    adj, ref = _adj("mixed")
    H, slope = 20, 0.2
    X, dY, As, Ad = _operands("mixed", H)
    Y, L, a, b, r = _reference(ref, X, dY, As, Ad, slope)
    calls = {"datt": 0, "bwd": 0, "da": 0}
    for name, key in (("gat_datt", "datt"), ("gat_bwd", "bwd"), ("gat_da", "da")):
        real = getattr(graph.CSRAdj, name)
        monkeypatch.setattr(graph.CSRAdj, name,
                            lambda self, *a_, _real=real, _key=key: (calls.__setitem__(_key, calls[_key] + 1), _real(self, *a_))[1])
    Xd = X.to(DEV).requires_grad_(True)
    s1, d1 = nn.Parameter(As.to(DEV)), nn.Parameter(Ad.to(DEV))
    out = ops.spmm_gat(adj, Xd, s1, d1, slope)
    out.backward(dY.to(DEV))
    assert rel_inf(out.detach().cpu(), Y) <= TOL and rel_inf(Xd.grad.cpu(), r.dX) <= TOL
    assert s1.grad.shape == (H, ) and _of_mass(s1.grad, r.datt_src, r.mass_datt_src) <= TOL
    assert d1.grad.shape == (H, ) and _of_mass(d1.grad, r.datt_dst, r.mass_datt_dst) <= TOL
    assert calls == {"datt": 1, "bwd": 1, "da": 0}
    # frozen: no column-reduction launch, no .grad, the same dX bits
    X2 = X.to(DEV).requires_grad_(True)
    s2, d2 = nn.Parameter(As.to(DEV)).requires_grad_(False), nn.Parameter(Ad.to(DEV)).requires_grad_(False)
    ops.spmm_gat(adj, X2, s2, d2, slope).backward(dY.to(DEV))
    assert s2.grad is None and d2.grad is None and calls == {"datt": 1, "bwd": 2, "da": 0}
    assert torch.equal(_bits(X2.grad), _bits(Xd.grad))
    # only the vectors: no transposed pass, the same gradient bits
    s3, d3 = nn.Parameter(As.to(DEV)), nn.Parameter(Ad.to(DEV))
    ops.spmm_gat(adj, X.to(DEV), s3, d3, slope).backward(dY.to(DEV))
    assert calls == {"datt": 2, "bwd": 2, "da": 1}
    assert torch.equal(_bits(s3.grad), _bits(s1.grad)) and torch.equal(_bits(d3.grad), _bits(d1.grad))
    with pytest.raises(L_.GlassHipError, match="spmm_gat"):
        ops.spmm(adj, X.to(DEV))
    with pytest.raises(L_.GlassHipError, match="replicated gat aggregation is not built"):
        ops.spmm_rep(adj, torch.zeros(2 * ref.n, H, device=DEV), 2)


# ---- through the model ----------------------------------------------------------------------------------------------------
MODEL_SEEDS = (11, 5)   # (graph, weights): chosen on the fp64 oracle alone, see the assertion on the vectors' gradients


def model_graph(seed):
    """N = 1 000, 6 000 entries (mean degree 6), node 0 isolated, not symmetric, weights in [0.25, 2); use_deg-style features
    (the rank of a node's degree, entries in plus entries out, among the distinct degrees).  (tests/test_gpu_aggr_softmax.py's)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    N, nnz = 1000, 6000
    row, col = rng.integers(1, N, nnz), rng.integers(1, N, nnz)
    w = rng.uniform(0.25, 2.0, nnz).astype(np.float32)
    ei = torch.from_numpy(np.stack((row, col)).astype(np.int64))
    total = np.bincount(row, minlength=N) + np.bincount(col, minlength=N)
    ranks = np.unique(total, return_inverse=True)[1]
    x = torch.from_numpy(ranks.astype(np.int64)).reshape(N, 1, 1)
    pos = torch.from_numpy(np.stack([rng.choice(N, 8, replace=False) for _ in range(10)]).astype(np.int64))
    pos[::3, -2:] = -1
    y = torch.from_numpy(rng.integers(0, 3, 10))
    return N, ei, torch.from_numpy(w), x, pos, y


def model_and_oracle(graph_seed, weight_seed, hidden=64):
    """(model on the CPU, its fp64 oracle after backward, the attention keys, data): the oracle is OracleGLASS(aggr "sum") whose
    conv.adj are GatAdj — the aggregation from plain torch ops, differentiated by autograd, the four vectors included."""
    from helpers import build_glass
    from oracle import glass_oracle as O
    N, ei, ew, x, pos, y = model_graph(graph_seed)
    torch.manual_seed(weight_seed)
    model = build_glass(hidden, 2, int(x.max()), 3, "gat", "mean", 0.8, dropout=0.0, jk=True)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    att_keys = sorted(k for k in sd if ".att_" in k)
    assert att_keys == ["conv.convs.0.att_dst", "conv.convs.0.att_src", "conv.convs.1.att_dst", "conv.convs.1.att_src"]
    orc = O.OracleGLASS(hidden, 2, int(x.max()), 3, aggr="sum", pool="mean", z_ratio=0.8).double()
    orc.load_state_dict({k: v for k, v in sd.items() if k not in att_keys})
    orc.train()
    att = {k: sd[k].double().requires_grad_(True) for k in att_keys}
    for l, conv in enumerate(orc.conv.convs):
        conv.adj = GO.GatAdj(ei, ew.double(), N, att[f"conv.convs.{l}.att_src"], att[f"conv.convs.{l}.att_dst"], 0.2)
    logits_ref = orc(x, ei, ew.double(), pos, O.max_zero_one(x, pos))
    loss_ref = nn.CrossEntropyLoss()(logits_ref, y)
    loss_ref.backward()
    grads_ref = {k: p.grad.clone() for k, p in orc.named_parameters()}
    grads_ref.update({k: v.grad.clone() for k, v in att.items()})
    return model, logits_ref.detach(), loss_ref.item(), grads_ref, att_keys, (N, ei, ew, x, pos, y)


def test_model_with_attention_aggregation_against_the_fp64_restatement():
    """Two GLASSConv layers at hidden 64, jk, no dropout: loss, logits and the flat gradient over all parameters, the four
    attention vectors included."""
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
    assert all(c.adj.aggr == "gat" for c in model.conv.convs)
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    assert set(keys) == set(mine)
    e_logits = rel_inf(logits.detach().cpu(), logits_ref)
    e_loss = abs(loss.item() - loss_ref) / abs(loss_ref)
    e_grad = rel_inf(flat_grads(mine, keys), flat_grads(grads_ref, keys))
    for k in att_keys:
        print(f"{k}: error {float((mine[k].double() - grads_ref[k]).abs().max()) / gmax:.2e} of the largest gradient {gmax:.3e}")
    print(f"loss {e_loss:.2e} logits {e_logits:.2e} flat gradient {e_grad:.2e}")
    assert e_loss <= TOL and e_logits <= TOL and e_grad <= TOL


def _tiny(seed, n_batches):
    from glass_amd import synth
    from impl import config
    config.set_device(0)
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=seed, n_batches=n_batches)
    return (w, ) + tuple(torch.from_numpy(a).to(DEV) for a in (x, ei, ew, pos, y))


@pytest.mark.parametrize("frozen", (False, True))
def test_training_on_the_captured_per_op_step_equals_its_eager_run(monkeypatch, frozen):
    """Two epochs of impl.train.train at aggr "gat": the TrainStep is captured and reports the per-op form (the stack program
    does not serve gat); losses and parameters equal, bit for bit, those of a deep copy trained with eager launches.  The
    attention vectors live in the parameter arena, have moved from their initial bits and hold the same bits on both routes —
    a replay that read a stale copy (its values or its pre-arena address) would differ.  frozen: requires_grad_(False) on the
    vectors trains the rest, leaves them outside the arena at their initial bits and never launches the column reductions."""
    from helpers import build_glass
    from impl import SubGDataset, train, utils
    from glass_amd import graph, stack, train as gtrain
    w, x, ei, ew, pos, y = _tiny(2, 2)
    torch.manual_seed(3)
    gnn = build_glass(64, 2, int(x.max()), w.n_class, "gat", w.pool, w.z_ratio).to(DEV)
    vectors = lambda net: [v for c in net.conv.convs for v in (c.att_src, c.att_dst)]
    if frozen:
        for v in vectors(gnn):
            v.requires_grad_(False)
    initial = [v.detach().clone() for v in vectors(gnn)]
    twin = copy.deepcopy(gnn)
    calls = []
    real = graph.CSRAdj.gat_datt
    monkeypatch.setattr(graph.CSRAdj, "gat_datt", lambda self, *a: (calls.append(1), real(self, *a))[1])
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
        assert not stack.StackProgram.supported(net.conv) and all(c.adj.aggr == "gat" for c in net.conv.convs)
        arena = net.__dict__["_glass_grad_bucket"]
        lo, hi = arena.flat_param.data_ptr(), arena.flat_param.data_ptr() + 4 * arena.flat_param.numel()
        for v in vectors(net):
            in_arena = any(v is p for p in arena.params) and lo <= v.data_ptr() < hi
            assert in_arena != frozen, (name, "attention vector in the arena", in_arena)
    assert bool(calls) != frozen
    assert np.isfinite(out["graph"]).all() and out["graph"][1] != out["graph"][0]
    assert np.array_equal(np.float32(out["graph"]).view(np.int32), np.float32(out["eager"]).view(np.int32)), out
    sd, sd2 = gnn.state_dict(), twin.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    for v, v0 in zip(vectors(gnn), initial):
        moved = not torch.equal(_bits(v.detach()), _bits(v0))
        print(f"attention vector moved by {float((v.detach() - v0).abs().max()):.3e} after two epochs (frozen: {frozen})")
        assert moved != frozen
