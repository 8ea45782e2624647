"""K1s on the GPU: glass_spmm_softmax_csr_f32 / _bwd_f32 / _dt_f32 (csrc/spmm_softmax.hip) against the fp64 restatement
tests/aggr_softmax_oracle.py on every plan form and lane layout, the host objects (graph.CSRAdj.softmax_fwd / softmax_bwd /
softmax_dt, ops.spmm_softmax), a GLASS model with aggr "softmax" against an fp64 restatement of the model, and impl.train.train
on the captured per-op step, whose replays must read the live temperature.

Everything here is a sum: Y, L and dX are compared at rel-inf <= 1e-5 against fp64; dt, a cancelling sum, by the
same rule applied to a sum, |dt - dt64| <= 1e-5 * sum |terms|.  Run to run every entry gives the same bits."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import aggr_softmax_oracle as SO
from aggr_max_oracle import MaxAdj, rows_of
from helpers import rel_inf, flat_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
GUARD = 64
WIDTHS = (4, 18, 64, 68, 128, 132, 256, 260)   # every VW / LPR case, two column tiles
TEMPS = (0.0, 1.0, -0.5, 4.0)


def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


def _t(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


class Guarded:
    """`n` elements filled with `fill`, GUARD sentinel elements in front and behind (tests/test_gpu_aggr_max.py's); `off` more
    filled elements in front of the view `t`, which then starts `off` elements past a 16-byte boundary"""
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


# ---- the two adjacencies (the generator of tests/test_gpu_aggr_max.py, with positive weights) ------------------------------
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
      weights, a self-loop.
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
    adj = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "softmax")
    return adj, MaxAdj(ei, ew.double(), n)


def test_plans_take_every_form_and_the_weight_rule():
    from glass_amd import graph
    for kind in ("mixed", "all_long"):
        adj, ref = _adj(kind)
        assert adj.aggr == "softmax" and not hasattr(adj, "eid_t")
        for got, want in ((adj.fwd.rowptr, ref.rowptr), (adj.fwd.col, ref.col), (adj.bwd.rowptr, ref.rowptr_t),
                          (adj.bwd.col, ref.col_t)):
            assert got.dtype == torch.int32 and torch.equal(got.cpu().to(torch.int64), want)
        assert torch.equal(adj.fwd.val.cpu().double(), ref.val) and torch.equal(adj.bwd.val.cpu().double(), ref.val_t)  # raw weights
        assert float(ref.val.min()) >= 0.25 and not torch.equal(ref.rowptr, ref.rowptr_t)
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
            graph.CSRAdj(ei.to(DEV), w.to(DEV), n, "softmax")


# ---- raw entries on guarded buffers --------------------------------------------------------------------------------------
def _raw_fwd(adj, Xv, t, ldy_extra=0, ldl_extra=0, off=0):
    """glass_spmm_softmax_csr_f32 -> (Y [n, H] view, L view, their Guarded buffers + the workspace's)"""
    L_, lib = _lib()
    op, (n, H) = adj.fwd, (adj.fwd.n_rows, Xv.shape[1])
    ldy, ldl = H + ldy_extra, H + ldl_extra
    Y, L = Guarded(n * ldy, float("nan"), off=off), Guarded(n * ldl, float("nan"), off=off)
    nbytes = lib.glass_spmm_softmax_ws_bytes(op.header.ctypes.data, H)
    assert nbytes == int(op.header[7]) * H * 12
    W = Guarded(max(nbytes // 4, 4), float("nan"))   # (need not be initialised: junk on purpose)
    rc = lib.glass_spmm_softmax_csr_f32(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), Xv.data_ptr(), Xv.stride(0),
                                        t.data_ptr(), Y.t.data_ptr(), ldy, L.t.data_ptr(), ldl, n, H, op.header.ctypes.data,
                                        op.plan.data_ptr(), W.t.data_ptr(), _stream())
    L_.check(rc, "glass_spmm_softmax_csr_f32")
    torch.cuda.synchronize()
    return Y.t.view(n, ldy), L.t.view(n, ldl), (Y, L, W)


def _raw_bwd(adj, dYv, Xv, Yv, Lv, t, ldx_extra=0, off=0):
    L_, lib = _lib()
    op, (n, H) = adj.bwd, (adj.bwd.n_rows, dYv.shape[1])
    lddx = H + ldx_extra
    D = Guarded(n * lddx, float("nan"), off=off)
    nbytes = lib.glass_spmm_softmax_bwd_ws_bytes(op.header.ctypes.data, H)
    assert nbytes == int(op.header[7]) * H * 4
    W = Guarded(max(nbytes // 4, 4), float("nan"))
    rc = lib.glass_spmm_softmax_bwd_f32(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), Xv.data_ptr(), Xv.stride(0),
                                        t.data_ptr(), dYv.data_ptr(), dYv.stride(0), Yv.data_ptr(), Yv.stride(0), Lv.data_ptr(),
                                        Lv.stride(0), D.t.data_ptr(), lddx, n, H, op.header.ctypes.data, op.plan.data_ptr(),
                                        W.t.data_ptr(), _stream())
    L_.check(rc, "glass_spmm_softmax_bwd_f32")
    torch.cuda.synchronize()
    return D.t.view(n, lddx), (D, W)


def _raw_dt(adj, dYv, Xv, Yv, Lv, t):
    L_, lib = _lib()
    op, (n, H) = adj.fwd, (adj.fwd.n_rows, dYv.shape[1])
    D = Guarded(1, float("nan"))
    nbytes = lib.glass_spmm_softmax_dt_ws_bytes(op.header.ctypes.data, H)
    assert nbytes == (int(op.header[4]) + int(op.header[5])) * ((H + 63) // 64) * 8
    W = Guarded(max(nbytes // 8, 2), float("nan"), torch.float64)
    rc = lib.glass_spmm_softmax_dt_f32(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), Xv.data_ptr(), Xv.stride(0),
                                       t.data_ptr(), dYv.data_ptr(), dYv.stride(0), Yv.data_ptr(), Yv.stride(0), Lv.data_ptr(),
                                       Lv.stride(0), D.t.data_ptr(), n, H, op.header.ctypes.data, op.plan.data_ptr(),
                                       W.t.data_ptr(), _stream())
    L_.check(rc, "glass_spmm_softmax_dt_f32")
    torch.cuda.synchronize()
    return D.t, (D, W)


@functools.lru_cache(maxsize=None)
def _operands(kind, H):
    n = _graph(kind)[0]
    g = torch.Generator().manual_seed(1000 * H + (kind == "mixed"))
    return torch.randn(n, H, generator=g), torch.randn(n, H, generator=g)


def _reference(ref, X, dY, t):
    """fp64: (Y, L, dX, dt, sum |dt terms|) from the fp32 operands"""
    X, dY = X.double(), dY.double()
    Y, L = SO.softmax_aggregate(ref.rowptr, ref.col, ref.val, X, t)
    dX = SO.softmax_aggregate_bwd(ref.rowptr_t, ref.col_t, ref.val_t, dY, X, Y, L, t)
    dt, mass = SO.softmax_aggregate_dt(ref.rowptr, ref.col, ref.val, dY, X, Y, L, t)
    return Y, L, dX, float(dt), float(mass)


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("kind", ("mixed", "all_long"))
def test_values_against_the_restatement_and_repeatability(kind, H):
    adj, ref = _adj(kind)
    X, dY = _operands(kind, H)
    Xd, dYd = X.to(DEV), dY.to(DEV)
    empty = (ref.rowptr[1:] == ref.rowptr[:-1]).nonzero().reshape(-1)
    assert len(empty) >= 1
    for tv in TEMPS:
        Y_ref, L_ref, dX_ref, dt_ref, mass = _reference(ref, X, dY, tv)
        t = _t(tv)
        Yv, Lv, guards = _raw_fwd(adj, Xd, t)
        e_y, e_l = rel_inf(Yv.cpu(), Y_ref), rel_inf(Lv.cpu(), L_ref)
        assert all(g.intact() for g in guards), (kind, H, tv, "guards of Y / L / workspace")
        assert bool((Yv[empty.to(DEV)] == 0).all()) and bool((Lv[empty.to(DEV)] == 0).all()), "a row without entries"
        Y2, L2, _g = _raw_fwd(adj, Xd, t)
        assert torch.equal(_bits(Yv), _bits(Y2)) and torch.equal(_bits(Lv), _bits(L2)), (kind, H, tv, "two forward runs differ")
        dXv, guards = _raw_bwd(adj, dYd, Xd, Yv, Lv, t)
        e_dx = rel_inf(dXv.cpu(), dX_ref)
        assert all(g.intact() for g in guards), (kind, H, tv, "guards of dX / workspace")
        dX2, _g = _raw_bwd(adj, dYd, Xd, Yv, Lv, t)
        assert torch.equal(_bits(dXv), _bits(dX2)), (kind, H, tv, "two backward runs differ")
        dtv, guards = _raw_dt(adj, dYd, Xd, Yv, Lv, t)
        e_dt = abs(float(dtv[0]) - dt_ref) / mass
        assert all(g.intact() for g in guards), (kind, H, tv, "guards of dt / workspace")
        dt2, _g = _raw_dt(adj, dYd, Xd, Yv, Lv, t)
        assert torch.equal(_bits(dtv), _bits(dt2)), (kind, H, tv, "two dt runs differ")
        print(f"{kind} H={H} t={tv}: Y {e_y:.2e} L {e_l:.2e} dX {e_dx:.2e} dt {e_dt:.2e} of sum|terms| (dt64 {dt_ref:.4e}, "
              f"sum|terms| {mass:.4e})")
        assert e_y <= TOL and e_l <= TOL and e_dx <= TOL and e_dt <= TOL, (kind, H, tv, e_y, e_l, e_dx, e_dt)
        if tv == 0.0:
            assert abs(dt_ref) > 0   # (t = 0 is no stationary point: the dt pass is exercised there too)


@pytest.mark.parametrize("H", (64, 18))
def test_large_exponents_stay_finite(H):
    """X scaled by 1e4 at t = 1: exponents of tens of thousands.  The max is always subtracted, so everything stays finite, and
    Y, a convex combination, lies within its row's [min x, max x] up to rounding (1e-5 of the row's largest |x|: the rule)."""
    for kind in ("mixed", "all_long"):
        adj, ref = _adj(kind)
        X, dY = _operands(kind, H)
        X = X * 1e4
        t = _t(1.0)
        Xd, dYd = X.to(DEV), dY.to(DEV)
        Yv, Lv, _g = _raw_fwd(adj, Xd, t)
        dXv, _g = _raw_bwd(adj, dYd, Xd, Yv, Lv, t)
        dtv, _g = _raw_dt(adj, dYd, Xd, Yv, Lv, t)
        assert all(bool(torch.isfinite(a).all()) for a in (Yv, Lv, dXv, dtv)), (kind, H)
        rows = rows_of(ref.rowptr)
        idx = rows[:, None].expand(-1, H)
        lo = torch.zeros(ref.n, H).scatter_reduce(0, idx, X[ref.col], "amin", include_self=False)
        hi = torch.zeros(ref.n, H).scatter_reduce(0, idx, X[ref.col], "amax", include_self=False)
        slack = TOL * torch.maximum(lo.abs(), hi.abs())
        Yc = Yv.cpu()
        assert bool((Yc >= lo - slack).all()) and bool((Yc <= hi + slack).all()), (kind, H)
        Y_ref, L_ref = SO.softmax_aggregate(ref.rowptr, ref.col, ref.val, X.double(), 1.0)
        print(f"{kind} H={H} X * 1e4: Y {rel_inf(Yc, Y_ref):.2e} L {rel_inf(Lv.cpu(), L_ref):.2e}")


@pytest.mark.parametrize("H", (64, 18))
def test_t_zero_is_the_mean_aggregation(H):
    """Against ops.spmm on a "mean" adjacency of the same graph and weights.  One documented difference is undone first: aggr
    "mean" divides by deg + 1 where a row's weighted degree is below 0.5 (the reference's rule for isolated nodes, buildAdj:
    `deg[deg < 0.5] += 1`), which weights from [0.25, 2) reach on rows with a single light entry — there "mean" is not the
    weighted mean, so its rows are scaled back by (deg + 1) / deg, exactly, in fp64.  Every row is compared."""
    from glass_amd import graph, ops
    light = 0
    for kind in ("mixed", "all_long"):
        adj, ref = _adj(kind)
        n, ei, ew = _graph(kind)
        mean = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "mean")
        X, _dY = _operands(kind, H)
        Xd = X.to(DEV)
        y = ops.spmm_softmax(adj, Xd, _t(0.0))
        deg = torch.zeros(n, dtype=torch.float64).index_add_(0, rows_of(ref.rowptr), ref.val)
        rule = (deg > 0) & (deg < 0.5)
        light += int(rule.sum())
        undo = torch.where(rule, (deg + 1) / torch.where(rule, deg, torch.ones(())), torch.ones((), dtype=torch.float64))
        want = ops.spmm(mean, Xd).cpu().double() * undo[:, None]
        err = rel_inf(y.cpu(), want)
        print(f"{kind} H={H}: t = 0 against aggr mean {err:.2e} ({int(rule.sum())} rows under the deg < 0.5 rule)")
        assert err <= TOL
    assert light >= 1


@pytest.mark.parametrize("H,pads,off", [(64, (8, 4, 12, 4), 0), (64, (3, 1, 2, 5), 0), (18, (2, 6, 1, 3), 0), (64, (0, 0, 0, 0), 1),
                                        (64, (4, 4, 4, 4), 3)])
def test_strided_and_unaligned_operands(H, pads, off):
    """X, Y, L, dY and dX as column slices of wider buffers (multiples of 4 keep the 16-byte form, anything else takes the
    scalar one), and every operand `off` floats past a 16-byte boundary (the scalar form at a width that has a vector one);
    the columns beyond H are neither read (NaN) nor written."""
    adj, ref = _adj("mixed")
    px, py, pl, pd = pads
    X, dY = _operands("mixed", H)
    tv = 1.0
    t = _t(tv)
    Y_ref, L_ref, dX_ref, dt_ref, mass = _reference(ref, X, dY, tv)

    def wide(src, pad):
        buf = torch.full((ref.n * (H + pad) + off + 4, ), float("nan"), device=DEV)
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + ref.n * (H + pad)].view(ref.n, H + pad)
        v[:, :H] = src.to(DEV)
        return v[:, :H]
    Xv, dYv = wide(X, px), wide(dY, py)
    assert Xv.data_ptr() % 16 == 4 * off
    Yv, Lv, guards = _raw_fwd(adj, Xv, t, py, pl, off)
    assert rel_inf(Yv[:, :H].cpu(), Y_ref) <= TOL and rel_inf(Lv[:, :H].cpu(), L_ref) <= TOL
    assert bool(torch.isnan(Yv[:, H:]).all()) and bool(torch.isnan(Lv[:, H:]).all()) and all(g.intact() for g in guards)
    dXv, guards = _raw_bwd(adj, dYv, Xv, Yv[:, :H], Lv[:, :H], t, pd, off)
    assert rel_inf(dXv[:, :H].cpu(), dX_ref) <= TOL
    assert bool(torch.isnan(dXv[:, H:]).all()) and all(g.intact() for g in guards)
    dtv, guards = _raw_dt(adj, dYv, Xv, Yv[:, :H], Lv[:, :H], t)
    assert abs(float(dtv[0]) - dt_ref) <= TOL * mass and all(g.intact() for g in guards)


def test_a_call_without_rows_launches_nothing():
    import ctypes
    L_, lib = _lib()
    rp = np.zeros(1, dtype=np.int32)
    words = ctypes.c_int64(0)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, 0, None, ctypes.byref(words)) == 0
    plan = np.zeros(words.value, dtype=np.int32)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, 0, plan.ctypes.data, ctypes.byref(words)) == 0
    pd = torch.from_numpy(plan).to(DEV)
    rpd = torch.zeros(1, dtype=torch.int32, device=DEV)
    H = 8
    bufs = [Guarded(4 * H, float("nan")) for _ in range(6)]
    x, y, l, dy, dx, dt = (b.t.data_ptr() for b in bufs)
    t, h, s = _t(1.0), plan.ctypes.data, _stream()
    assert lib.glass_spmm_softmax_csr_f32(rpd.data_ptr(), None, None, x, H, t.data_ptr(), y, H, l, H, 0, H, h, pd.data_ptr(), None, s) == 0
    assert lib.glass_spmm_softmax_bwd_f32(rpd.data_ptr(), None, None, x, H, t.data_ptr(), dy, H, y, H, l, H, dx, H, 0, H, h,
                                          pd.data_ptr(), None, s) == 0
    assert lib.glass_spmm_softmax_dt_f32(rpd.data_ptr(), None, None, x, H, t.data_ptr(), dy, H, y, H, l, H, dt, 0, H, h,
                                         pd.data_ptr(), None, s) == 0
    torch.cuda.synchronize()
    assert all(b.intact() and bool(torch.isnan(b.t).all()) for b in bufs)


def test_autograd_binding_and_a_frozen_temperature(monkeypatch):
    from glass_amd import graph, ops
    L_, _ = _lib()
    adj, ref = _adj("mixed")
    H, tv = 20, 1.0
    X, dY = _operands("mixed", H)
    Y_ref, L_ref, dX_ref, dt_ref, mass = _reference(ref, X, dY, tv)
    calls = []
    real_dt = graph.CSRAdj.softmax_dt
    monkeypatch.setattr(graph.CSRAdj, "softmax_dt", lambda self, *a: (calls.append(1), real_dt(self, *a))[1])
    Xd = X.to(DEV).requires_grad_(True)
    t = nn.Parameter(_t(tv))
    Y = ops.spmm_softmax(adj, Xd, t)
    Y.backward(dY.to(DEV))
    assert rel_inf(Y.detach().cpu(), Y_ref) <= TOL and rel_inf(Xd.grad.cpu(), dX_ref) <= TOL
    assert t.grad.shape == (1, ) and abs(float(t.grad[0]) - dt_ref) <= TOL * mass and calls == [1]
    # frozen: no dt launch, no t.grad, the same dX bits
    X2 = X.to(DEV).requires_grad_(True)
    t2 = nn.Parameter(_t(tv)).requires_grad_(False)
    ops.spmm_softmax(adj, X2, t2).backward(dY.to(DEV))
    assert t2.grad is None and calls == [1] and torch.equal(_bits(X2.grad), _bits(Xd.grad))
    # only t: no dX launch is needed, the same dt bits
    t3 = nn.Parameter(_t(tv))
    ops.spmm_softmax(adj, X.to(DEV), t3).backward(dY.to(DEV))
    assert calls == [1, 1] and torch.equal(_bits(t3.grad), _bits(t.grad))
    with pytest.raises(L_.GlassHipError, match="spmm_softmax"):
        ops.spmm(adj, X.to(DEV))
    with pytest.raises(L_.GlassHipError, match="replicated softmax aggregation is not built"):
        ops.spmm_rep(adj, torch.zeros(2 * ref.n, H, device=DEV), 2)


# ---- through the model ----------------------------------------------------------------------------------------------------
def model_graph(seed):
    """N = 1 000, 6 000 entries (mean degree 6), node 0 isolated, not symmetric, weights in [0.25, 2); use_deg-style features
    (the rank of a node's degree, entries in plus entries out, among the distinct degrees)."""
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


def test_model_with_softmax_aggregation_against_the_fp64_restatement():
    """Two GLASSConv layers at hidden 64 with temperatures 1.0 and -0.75: the fp64 side is OracleGLASS(aggr "sum") whose
    conv.adj are SoftmaxAdj — the aggregation from plain torch ops, differentiated by autograd, t included."""
    from helpers import build_glass
    from impl import utils
    from oracle import glass_oracle as O
    hidden = 64
    N, ei, ew, x, pos, y = model_graph(11)
    torch.manual_seed(5)
    model = build_glass(hidden, 2, int(x.max()), 3, "softmax", "mean", 0.8, dropout=0.0, jk=True)
    with torch.no_grad():
        model.conv.convs[1].t.fill_(-0.75)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    t_keys = sorted(k for k in sd if k.endswith(".t"))
    assert t_keys == ["conv.convs.0.t", "conv.convs.1.t"]
    orc = O.OracleGLASS(hidden, 2, int(x.max()), 3, aggr="sum", pool="mean", z_ratio=0.8).double()
    orc.load_state_dict({k: v for k, v in sd.items() if k not in t_keys})
    orc.train()
    ts = {k: sd[k].double().requires_grad_(True) for k in t_keys}
    for l, conv in enumerate(orc.conv.convs):
        conv.adj = SO.SoftmaxAdj(ei, ew.double(), N, ts[f"conv.convs.{l}.t"])
    logits_ref = orc(x, ei, ew.double(), pos, O.max_zero_one(x, pos))
    loss_ref = nn.CrossEntropyLoss()(logits_ref, y)
    loss_ref.backward()
    grads_ref = {k: p.grad.clone() for k, p in orc.named_parameters()}
    grads_ref.update({k: v.grad.clone() for k, v in ts.items()})

    model.to(DEV).train()
    xg, eig, ewg, posg, yg = (a.to(DEV) for a in (x, ei, ew, pos, y))
    logits = model(xg, eig, ewg, posg, utils.MaxZOZ(xg, posg), id=0)
    loss = nn.CrossEntropyLoss()(logits, yg)
    loss.backward()
    torch.cuda.synchronize()
    assert all(c.adj.aggr == "softmax" for c in model.conv.convs)
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    keys = sorted(grads_ref)
    assert set(keys) == set(mine) and all(k in keys for k in t_keys)
    e_logits = rel_inf(logits.detach().cpu(), logits_ref.detach())
    e_loss = abs(loss.item() - loss_ref.item()) / abs(loss_ref.item())
    e_grad = rel_inf(flat_grads(mine, keys), flat_grads(grads_ref, keys))
    gmax = float(flat_grads(grads_ref, keys).abs().max())
    for k in t_keys:
        print(f"{k}: gradient {float(mine[k][0]):.6e}, fp64 {float(grads_ref[k][0]):.6e}, error {abs(float(mine[k][0]) - float(grads_ref[k][0])) / gmax:.2e} "
              f"of the largest gradient {gmax:.3e}")
    print(f"loss {e_loss:.2e} logits {e_logits:.2e} flat gradient {e_grad:.2e}")
    assert all(float(grads_ref[k].abs()) > 1e-3 * gmax for k in t_keys), "the temperatures' gradients must count in the flat metric"
    assert e_loss <= TOL and e_logits <= TOL and e_grad <= TOL


def _tiny(seed, n_batches):
    from glass_amd import synth
    from impl import config
    config.set_device(0)
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=seed, n_batches=n_batches)
    return (w, ) + tuple(torch.from_numpy(a).to(DEV) for a in (x, ei, ew, pos, y))


@pytest.mark.parametrize("frozen", (False, True))
def test_training_on_the_captured_per_op_step_equals_its_eager_run(monkeypatch, frozen):
    """Two epochs of impl.train.train at aggr "softmax": the TrainStep is captured and reports the per-op form (the stack program
    does not serve softmax); losses and parameters equal, bit for bit, those of a deep copy trained with eager launches.  The
    temperatures live in the parameter arena, have moved from 1.0 and hold the same bits on both routes — a replay that read a
    stale copy of t (its value or its pre-arena address) would differ.  frozen: t.requires_grad_(False) trains the rest, leaves t
    at 1.0 outside the arena and never launches the dt pass."""
    from helpers import build_glass
    from impl import SubGDataset, train, utils
    from glass_amd import graph, stack, train as gtrain
    w, x, ei, ew, pos, y = _tiny(2, 2)
    torch.manual_seed(3)
    gnn = build_glass(64, 2, int(x.max()), w.n_class, "softmax", w.pool, w.z_ratio).to(DEV)
    if frozen:
        for c in gnn.conv.convs:
            c.t.requires_grad_(False)
    twin = copy.deepcopy(gnn)
    calls = []
    real_dt = graph.CSRAdj.softmax_dt
    monkeypatch.setattr(graph.CSRAdj, "softmax_dt", lambda self, *a: (calls.append(1), real_dt(self, *a))[1])
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
        assert not stack.StackProgram.supported(net.conv) and all(c.adj.aggr == "softmax" for c in net.conv.convs)
        arena = net.__dict__["_glass_grad_bucket"]
        lo, hi = arena.flat_param.data_ptr(), arena.flat_param.data_ptr() + 4 * arena.flat_param.numel()
        for c in net.conv.convs:
            in_arena = any(c.t is p for p in arena.params) and lo <= c.t.data_ptr() < hi
            assert in_arena != frozen, (name, "t in the arena", in_arena)
    assert bool(calls) != frozen
    assert np.isfinite(out["graph"]).all() and out["graph"][1] != out["graph"][0]
    assert np.array_equal(np.float32(out["graph"]).view(np.int32), np.float32(out["eager"]).view(np.int32)), out
    sd, sd2 = gnn.state_dict(), twin.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    for l in range(2):
        tv = float(sd[f"conv.convs.{l}.t"][0])
        print(f"layer {l}: t = {tv!r} after two epochs (frozen: {frozen})")
        assert (tv == 1.0) == frozen
