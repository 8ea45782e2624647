"""The three replica entries on the GPU (csrc/labels_rep.hip, spmm_rep.hip, graphnorm_rep.hip): the labels against numpy,
the replicated aggregation and GraphNorm BITWISE against the single-graph entries on each replica's slice (the contract of
include/glass_hip.h), parameter gradients against an fp64 sum at the project's rel-inf bar."""
import numpy as np
import pytest
import torch

from helpers import rel_inf
import zeroone_oracle as ZO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
H_NSWEEP, H_NLONG, H_NREDUCE, H_NSLOTS, H_LONG_THR, H_LONG_CHUNK, H_FLAT_SHARE = 4, 5, 6, 7, 8, 9, 15


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- labels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B,Smax,rep0,R", [(7001, 5, 40, 2, 3), (13, 6, 5, 0, 6), (1, 4, 3, 1, 2), (40000, 2, 9, 1, 1)])
def test_zeroone_labels_equal_numpy(n, B, Smax, rep0, R):
    from glass_amd import ops
    rng = np.random.Generator(np.random.PCG64(n))
    pos = rng.integers(-1, n + 3, (B, Smax)).astype(np.int64)   # -1 padding and ids >= n among them
    pos[rep0, :2] = [n - 1, n - 1]                               # the last node, twice
    if B > rep0 + 1:
        pos[rep0 + 1] = -1                                       # an all-padding row
    want = ZO.zeroone_z(n, pos)[rep0:rep0 + R].astype(np.uint8).reshape(-1)
    got = ops.zeroone_labels(torch.from_numpy(pos).to(DEV), n, rep0, R)
    assert got.dtype == torch.uint8 and got.numel() == R * n
    assert np.array_equal(got.cpu().numpy(), want)
    # an unaligned destination inside a poisoned buffer: exactly the R * n bytes are written
    from glass_amd import _lib
    buf = torch.full((R * n + 40, ), 9, dtype=torch.uint8, device=DEV)
    pg = torch.from_numpy(pos).to(DEV)
    _lib.check(_lib.load().glass_zeroone_labels_u8(pg.data_ptr(), B, Smax, rep0, R, n, buf.data_ptr() + 3, _stream()), "labels")
    out = buf.cpu().numpy()
    assert np.all(out[:3] == 9) and np.all(out[3 + R * n:] == 9) and np.array_equal(out[3:3 + R * n], want)
    from impl import utils
    z = utils.ZeroOneZ(torch.zeros(n, 1, device=DEV), pg)
    assert z.dtype == torch.int64 and np.array_equal(z.cpu().numpy(), ZO.zeroone_z(n, pos))


# ---- replicated K1 --------------------------------------------------------------------------------------------------------
def _csr(deg, n_cols, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = rng.integers(0, n_cols, int(rowptr[-1])).astype(np.int32)
    val = rng.standard_normal(int(rowptr[-1])).astype(np.float32)
    return rowptr, col, val


def _operand(rowptr, col, val, n_cols):
    from glass_amd.graph import CSROperand
    return CSROperand(torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV), torch.from_numpy(val).to(DEV),
                      len(rowptr) - 1, n_cols, rowptr_host=rowptr)


def _transpose(rowptr, col, val, n_cols):
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    order = np.argsort(col.astype(np.int64) * len(rowptr) + rows, kind="stable")
    rp_t = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n_cols))]).astype(np.int32)
    return rp_t, rows[order].astype(np.int32), val[order]


def _mixed_graph():
    """A few hundred rows: isolated rows, short rows, one row just over the plan's long-row threshold and one longer than a
    chunk (several chunks: the reduce step).  The thresholds are read from the plan header of the graph itself."""
    n = 300
    rng = np.random.Generator(np.random.PCG64(5))
    deg = rng.integers(0, 6, n)
    deg[[0, 7, 8, 150, 299]] = 0
    probe = _operand(*_csr(deg, n, 1), n)
    thr, chunk = int(probe.header[H_LONG_THR]), int(probe.header[H_LONG_CHUNK])
    deg[40] = thr + 1
    deg[200] = 2 * chunk + 70
    rowptr, col, val = _csr(deg, n, 2)
    # ... and two popular columns, so that the transpose holds a long row and a several-chunk row of its own
    col[rowptr[40]:rowptr[41]] = 17
    col[rowptr[200]:rowptr[200] + 2 * chunk + 10] = 23
    op = _operand(rowptr, col, val, n)
    hdr = op.header
    assert (int(hdr[H_LONG_THR]), int(hdr[H_LONG_CHUNK])) == (thr, chunk), "the long rows moved the plan's thresholds"
    assert hdr[H_NSWEEP] > 0 and hdr[H_NLONG] >= 4 and hdr[H_NREDUCE] == 1 and hdr[H_NSLOTS] == 3
    return n, (rowptr, col, val), op


def _check_rep(op, n_cols, H, R, seed):
    """Replica r of one replicated launch == the single-graph entry on that replica's slice, bit for bit; rows and columns
    between the replicas (non-trivial strides, ld > H) are left alone."""
    ldx, ldy = H + 4, H + 8
    xs, ys = n_cols + 3, op.n_rows + 2
    g = torch.Generator(device="cpu").manual_seed(seed)
    X = torch.randn((R * xs, ldx), generator=g).to(DEV)
    Y = torch.full((R * ys, ldy), 7.0, device=DEV)
    op.spmm_rep(X[:, :H], R, x_rep_stride=xs, out=Y[:, :H], y_rep_stride=ys)
    for r in range(R):
        want = op.spmm(X[r * xs:r * xs + n_cols, :H])
        assert torch.equal(Y[r * ys:r * ys + op.n_rows, :H], want), (H, R, r)
        assert torch.all(Y[r * ys + op.n_rows:(r + 1) * ys] == 7.0)
    assert torch.all(Y[:, H:] == 7.0)
    return Y


@pytest.mark.parametrize("H", [8, 17, 64, 260])
def test_spmm_rep_bitwise_equals_slices(H):
    n, (rowptr, col, val), op = _mixed_graph()
    op_t = _operand(*_transpose(rowptr, col, val, n), n)
    assert op_t.header[H_NSWEEP] > 0 and op_t.header[H_NLONG] >= 4 and op_t.header[H_NREDUCE] >= 1, op_t.header
    for R in (1, 2, 5):
        for which, o in (("A", op), ("At", op_t)):
            Y1 = _check_rep(o, n, H, R, 10 * R + len(which))
            Y2 = _check_rep(o, n, H, R, 10 * R + len(which))
            assert torch.equal(Y1, Y2)


@pytest.mark.parametrize("H", [8, 64])
def test_spmm_rep_flat_mode(H):
    """The flat-capable sweep build is chosen only for throughput-bound sweeps (thousands of items of short rows): a long
    run of degree-1 / degree-2 rows, asserted from the plan header (item count and flat-eligible share at this width)."""
    n = 40000
    deg = np.ones(n, dtype=np.int64)
    deg[::7] = 2
    deg[::1001] = 0
    rowptr, col, val = _csr(deg, n, 3)
    col[:] = np.random.Generator(np.random.PCG64(9)).permutation(n)[np.arange(len(col)) % n]  # short columns too
    op = _operand(rowptr, col, val, n)
    op_t = _operand(*_transpose(rowptr, col, val, n), n)
    G = 64 // min(64, max(1, 1 << int(np.ceil(np.log2(H / 4)))))
    share = (int(op.header[H_FLAT_SHARE]) >> (4 * int(np.log2(G)))) & 15
    share_t = (int(op_t.header[H_FLAT_SHARE]) >> (4 * int(np.log2(G)))) & 15
    assert op.header[H_NSWEEP] >= 8192 and G > 1 and share >= 8, (op.header[H_NSWEEP], G, share)
    assert op_t.header[H_NSWEEP] >= 8192 and share_t >= 8, (op_t.header[H_NSWEEP], share_t)
    for R in (1, 2, 5):
        _check_rep(op, n, H, R, 4 + R)
        _check_rep(op_t, n, H, R, 40 + R)


def test_spmm_rep_autograd_and_chunk_error():
    from glass_amd import ops
    from glass_amd._lib import GlassHipError
    from impl import models
    n, ei, ew, _x, _pos = ZO.graph(120, 1)
    adj = models.buildAdj(ei.to(DEV), ew.to(DEV), n, "mean")
    x = torch.randn(3 * n, 16, device=DEV, requires_grad=True)
    gout = torch.randn(3 * n, 16, device=DEV)
    y = ops.spmm_rep(adj, x, 3)
    y.backward(gout)
    x1 = x.detach().clone().requires_grad_(True)
    for r in range(3):
        yr = ops.spmm(adj, x1[r * n:(r + 1) * n])
        yr.backward(gout[r * n:(r + 1) * n])
        assert torch.equal(yr, y[r * n:(r + 1) * n])
    assert torch.equal(x.grad, x1.grad)
    from glass_amd import _lib
    R = _lib.load().glass_spmm_rep_max_replicas() + 1   # one more than a launch takes (every replica reads the same X)
    with pytest.raises(GlassHipError, match="replica_chunk"):
        adj.fwd.spmm_rep(x.detach()[:n], R, x_rep_stride=0, out=torch.empty((R * n, 16), device=DEV))


# ---- replicated GraphNorm -------------------------------------------------------------------------------------------------
def _gn_single(lib, x, dy, N, C, params, act, p, rng, call_id, acc=None):
    """The whole-graph entries on one slice: (y, saved, dx, dparams[3, C])."""
    g, b, a = params
    y, dx = torch.empty_like(x), torch.empty_like(x)
    saved = torch.empty(4 * C, device=DEV)
    dpar = torch.zeros((3, C), device=DEV)
    ws = torch.empty(lib.glass_graphnorm_ws_bytes(N, C) // 8 + 1, dtype=torch.float64, device=DEV)
    rp = rng.data_ptr() if p > 0 else 0
    assert lib.glass_graphnorm_fwd_f32(x.data_ptr(), C, y.data_ptr(), C, N, C, g.data_ptr(), b.data_ptr(), a.data_ptr(), 1e-5,
                                       saved.data_ptr(), act, p, rp, call_id, ws.data_ptr(), _stream()) == 0
    assert lib.glass_graphnorm_bwd_f32(dy.data_ptr(), C, x.data_ptr(), C, dx.data_ptr(), C, 0, 0, N, C, g.data_ptr(), a.data_ptr(),
                                       saved.data_ptr(), dpar[0].data_ptr(), dpar[1].data_ptr(), dpar[2].data_ptr(), 0, act, p, rp,
                                       call_id, ws.data_ptr(), _stream()) == 0
    return y, saved, dx, dpar


def _gn_rep(lib, x, dy, N, C, R, rep0, params, act, p, rng, call_id, dpar, accumulate):
    g, b, a = params
    y, dx = torch.empty_like(x), torch.empty_like(x)
    saved = torch.empty(R * 4 * C, device=DEV)
    ws = torch.empty(lib.glass_graphnorm_rep_ws_bytes(N, C, R) // 8 + 1, dtype=torch.float64, device=DEV)
    rp = rng.data_ptr() if p > 0 else 0
    assert lib.glass_graphnorm_rep_fwd_f32(x.data_ptr(), C, y.data_ptr(), C, N, C, R, rep0, g.data_ptr(), b.data_ptr(),
                                           a.data_ptr(), 1e-5, saved.data_ptr(), act, p, rp, call_id, ws.data_ptr(), _stream()) == 0
    assert lib.glass_graphnorm_rep_bwd_f32(dy.data_ptr(), C, x.data_ptr(), C, dx.data_ptr(), C, 0, 0, N, C, R, rep0, g.data_ptr(),
                                           a.data_ptr(), saved.data_ptr(), dpar[0].data_ptr(), dpar[1].data_ptr(),
                                           dpar[2].data_ptr(), accumulate, act, p, rp, call_id, ws.data_ptr(), _stream()) == 0
    return y, saved, dx


@pytest.mark.parametrize("C", [8, 17, 64, 192])
def test_graphnorm_rep_bitwise_equals_slices(C):
    from glass_amd import _lib
    lib = _lib.load()
    block = lib.glass_graphnorm_rep_row_block(C, 1 if C % 4 == 0 else 0)
    assert block >= 8
    rng_words = torch.tensor([12345, 7], dtype=torch.int64, device=DEV)
    gen = torch.Generator(device="cpu").manual_seed(C)
    params = tuple((torch.randn(C, generator=gen) * 0.5 + s).to(DEV) for s in (1.0, 0.0, 0.8))
    call_id, rep0, worst = 33, 2, 0.0
    for N in (1, 63, block + 1):
        for R in (1, 3):
            x = (torch.randn((R * N, C), generator=gen) * 2 + 0.5).to(DEV)
            dy = torch.randn((R * N, C), generator=gen).to(DEV)
            for act in (0, 1, 2):
                for p in (0.0, 0.5):
                    dpar = torch.zeros((3, C), device=DEV)
                    y, saved, dx = _gn_rep(lib, x, dy, N, C, R, rep0, params, act, p, rng_words, call_id, dpar, 0)
                    want_par = torch.zeros((3, C), dtype=torch.float64, device=DEV)
                    for r in range(R):
                        sl = slice(r * N, (r + 1) * N)
                        cid = call_id + ((rep0 + r) << 32)
                        y1, s1, dx1, dp1 = _gn_single(lib, x[sl].contiguous(), dy[sl].contiguous(), N, C, params, act, p,
                                                      rng_words, cid)
                        tag = (C, N, R, r, act, p)
                        assert torch.equal(y[sl], y1), tag
                        assert torch.equal(saved[r * 4 * C:(r + 1) * 4 * C], s1), tag
                        assert torch.equal(dx[sl], dx1), tag
                        want_par += dp1.double()
                    err = rel_inf(dpar.cpu(), want_par.cpu())
                    worst = max(worst, err)
                    assert err <= TOL, (C, N, R, act, p, err)
                    # accumulate: what the buffers hold is kept
                    acc = torch.full((3, C), 0.25, device=DEV)
                    _gn_rep(lib, x, dy, N, C, R, rep0, params, act, p, rng_words, call_id, acc, 1)
                    assert rel_inf(acc.cpu(), (want_par + 0.25).cpu()) <= TOL
                    if R == 1:
                        assert torch.equal(acc, 0.25 + dpar)
    # repeatability: the same bits on a second stream
    N, R = block + 1, 3
    x = torch.randn((R * N, C), generator=gen).to(DEV)
    dy = torch.randn((R * N, C), generator=gen).to(DEV)
    d1, d2 = torch.zeros((3, C), device=DEV), torch.zeros((3, C), device=DEV)
    first = _gn_rep(lib, x, dy, N, C, R, rep0, params, 1, 0.5, rng_words, call_id, d1, 0)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        second = _gn_rep(lib, x, dy, N, C, R, rep0, params, 1, 0.5, rng_words, call_id, d2, 0)
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and torch.equal(d1, d2)
    print(f"graphnorm_rep C={C}: parameter gradients vs fp64 sum of the slices, worst rel-inf {worst:.2e}")


def test_graphnorm_rep_autograd_sums_replicas():
    from glass_amd import ops
    from impl import models
    C, N, R = 24, 50, 3
    gn = models.GraphNorm(C).to(DEV)
    with torch.no_grad():
        gn.weight.uniform_(0.5, 1.5), gn.bias.uniform_(-0.5, 0.5), gn.mean_scale.uniform_(0.5, 1.0)
    x = torch.randn(R * N, C, device=DEV, requires_grad=True)
    gout = torch.randn(R * N, C, device=DEV)
    y = gn(x, batch=ops.Replicas(R, N, 0), act=ops.ACT_ELU)
    y.backward(gout)
    mine = [p.grad.clone() for p in gn.parameters()]
    for p in gn.parameters():
        p.grad = None
    x1 = x.detach().clone().requires_grad_(True)
    for r in range(R):
        yr = gn(x1[r * N:(r + 1) * N], act=ops.ACT_ELU)
        yr.backward(gout[r * N:(r + 1) * N])
        assert torch.equal(yr, y[r * N:(r + 1) * N])
    assert torch.equal(x.grad, x1.grad)
    for a, p in zip(mine, gn.parameters()):
        assert rel_inf(a.cpu(), p.grad.cpu()) <= TOL
