"""Kernel-level parity: every HIP kernel (through the C ABI, via glass_amd.ops) against the CPU
oracle on the same seeded inputs.  Tolerance: rel-inf <= 1e-5 (north_star), written per test;
integer / index outputs must be exact."""
import numpy as np
import pytest
import torch

from helpers import load, rel_inf, record_parity
from oracle import glass_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda:0"


def _graph(n, n_pairs, seed, weighted=False, powerlaw=0.0):
    from glass_amd import synth
    ei, ew = synth.make_graph(n, n_pairs, seed, powerlaw)
    if weighted:
        rng = np.random.default_rng(seed + 100)
        ew = rng.uniform(0.25, 2.0, ew.shape[0]).astype(np.float32)
    return torch.from_numpy(ei), torch.from_numpy(ew)


# ---------------------------------------------------------------------------------- K2 + K1
@pytest.mark.parametrize("aggr", ["mean", "sum", "gcn"])
def test_adj_values_g1(aggr):
    """buildAdj on the golden 12-node graph: isolated node, duplicate edge, self-loop, weights."""
    from glass_amd.graph import CSRAdj
    g = load("g1_buildadj.npz")
    ei, ew = torch.from_numpy(g["edge_index"]).to(DEV), torch.from_numpy(g["edge_weight"]).to(DEV)
    adj = CSRAdj(ei, ew, int(g["n_node"]), aggr)
    assert rel_inf(adj.to_dense().cpu(), g["A_" + aggr]) < 1e-6
    # transpose operand really is A^T
    n = adj.n_node
    x = torch.eye(n, device=DEV)
    assert rel_inf(adj.bwd.spmm(x).cpu(), g["A_" + aggr].T) < 1e-6
    assert rel_inf(adj.fwd.spmm(x).cpu(), g["A_" + aggr]) < 1e-6


def test_adj_unknown_aggr_raises():
    from glass_amd.models import buildAdj
    ei, ew = _graph(20, 30, 0)
    with pytest.raises(NotImplementedError):
        buildAdj(ei.to(DEV), ew.to(DEV), 20, "median")


@pytest.mark.parametrize("H", [1, 4, 8, 17, 20, 64, 100, 128, 256, 260, 512])
@pytest.mark.parametrize("aggr", ["mean", "gcn"])
def test_spmm_widths(H, aggr):
    """All feature widths: float4 path (H%4==0), scalar path (17), column tiling (>256)."""
    from glass_amd.graph import CSRAdj
    from glass_amd import ops
    n = 700
    ei, ew = _graph(n, 6000, 3, weighted=True)
    x = torch.randn(n, H, generator=torch.Generator().manual_seed(H))
    ref = O.build_adj(ei, ew, n, aggr).to(torch.float64) @ x.double()
    adj = CSRAdj(ei.to(DEV), ew.to(DEV), n, aggr)
    xg = x.to(DEV).requires_grad_(True)
    y = ops.spmm(adj, xg)
    assert rel_inf(y.detach().cpu(), ref) < TOL
    gout = torch.randn(n, H, generator=torch.Generator().manual_seed(H + 1))
    y.backward(gout.to(DEV))
    ref_g = O.build_adj(ei, ew, n, aggr).to(torch.float64).t() @ gout.double()
    assert rel_inf(xg.grad.cpu(), ref_g) < TOL


def test_spmm_long_rows_and_repeatable():
    """Power-law graph: rows >= 256 edges (workgroup path) and > 2048 (chunked partials)."""
    from glass_amd.graph import CSRAdj
    n = 20000
    ei, ew = _graph(n, 400000, 5, weighted=True, powerlaw=0.9)
    deg = torch.bincount(ei[0], minlength=n)
    assert int((deg >= 256).sum()) > 0 and int(deg.max()) > 2048
    x = torch.randn(n, 64, generator=torch.Generator().manual_seed(1))
    ref = O.build_adj(ei, ew, n, "mean").to(torch.float64) @ x.double()
    adj = CSRAdj(ei.to(DEV), ew.to(DEV), n, "mean")
    assert adj.fwd.header[5] > 0 and adj.fwd.header[6] > 0  # long items and multi-chunk rows exist
    xg = x.to(DEV)
    y1 = adj.fwd.spmm(xg)
    y2 = adj.fwd.spmm(xg)
    assert rel_inf(y1.cpu(), ref) < TOL
    assert torch.equal(y1, y2)  # bitwise repeatable: no float atomics
    yt = adj.bwd.spmm(xg)
    ref_t = O.build_adj(ei, ew, n, "mean").to(torch.float64).t() @ x.double()
    assert rel_inf(yt.cpu(), ref_t) < TOL


def test_spmm_empty_rows_and_strided():
    from glass_amd.graph import CSRAdj
    n = 50
    ei = torch.tensor([[0, 1, 1, 49], [1, 0, 49, 1]])
    ew = torch.ones(4)
    adj = CSRAdj(ei.to(DEV), ew.to(DEV), n, "sum")
    wide = torch.randn(n, 96, device=DEV)
    x = wide[:, 32:64]  # ld = 96
    out = torch.full((n, 80), 7.0, device=DEV)
    adj.fwd.spmm(x, out=out[:, 16:48])
    ref = O.build_adj(ei, ew, n, "sum") @ x.cpu()
    assert rel_inf(out[:, 16:48].cpu(), ref) < 1e-6
    assert float(out[:, :16].min()) == 7.0 and float(out[:, 48:].min()) == 7.0  # neighbours untouched
    assert float(out[5, 16:48].abs().max()) == 0.0  # isolated row written as zeros


# ---------------------------------------------------------------------------------- K4, K3
def test_maxzoz_g6_and_random():
    from glass_amd import utils
    g = load("g6_utils.npz")
    x = torch.zeros(int(g["mz_n"]), 1, 1, dtype=torch.int64, device=DEV)
    z = utils.MaxZOZ(x, torch.from_numpy(g["mz_pos"]).to(DEV))
    assert z.dtype == torch.int64 and np.array_equal(z.cpu().numpy(), g["mz_z"])
    rng = np.random.default_rng(0)
    pos = rng.integers(-1, 5000, (80, 37))
    zr = O.max_zero_one(torch.zeros(5000, 1), torch.from_numpy(pos))
    zg = utils.MaxZOZ(torch.zeros(5000, 1, device=DEV), torch.from_numpy(pos).to(DEV))
    assert torch.equal(zg.cpu(), zr)


def test_pad2batch_batch2pad_docstrings():
    from glass_amd import utils
    pad = utils.batch2pad(torch.tensor([0, 1, 0, 0, 1, 1, 2, 2], device=DEV))
    assert pad.cpu().tolist() == [[0, 2, 3], [1, 4, 5], [6, 7, -1]]
    b, p = utils.pad2batch(pad)
    assert b.cpu().tolist() == [0, 0, 0, 1, 1, 1, 2, 2] and p.cpu().tolist() == [0, 2, 3, 1, 4, 5, 6, 7]


@pytest.mark.parametrize("H,V", [(64, 40), (17, 3), (8, 2)])
def test_embed_label(H, V):
    from glass_amd import ops
    from glass_amd.graph import Selection
    n = 3000
    gen = torch.Generator().manual_seed(7)
    x = torch.randint(0, V, (n, ), generator=gen)
    if V == 2:
        x[:] = 1  # use_one: every node -> row 1 (a single hot table row)
    w = torch.randn(V, H, generator=gen)
    z = (torch.rand(n, generator=gen) < 0.1).to(torch.int64)
    wg = w.to(DEV).requires_grad_(True)
    xg = x.to(DEV)
    h, mask = ops.embed_label(wg, xg, z.to(DEV), Selection(xg, V))
    assert torch.equal(h.detach().cpu(), w[x])  # gather is exact
    assert torch.equal(mask.cpu().bool(), z > 0)
    gout = torch.randn(n, H, generator=gen)
    h.backward(gout.to(DEV))
    ref = torch.zeros(V, H, dtype=torch.float64).index_add_(0, x, gout.double())
    assert rel_inf(wg.grad.cpu(), ref) < TOL
    _, mask_all = ops.embed_label(wg, xg, None, Selection(xg, V))
    assert bool(mask_all.bool().all())  # z=None -> every node labeled (models.py:243-244)


def test_embed_index_out_of_range_raises():
    from glass_amd.graph import Selection
    with pytest.raises(IndexError):
        Selection(torch.tensor([0, 5, 2], device=DEV), 5)


# ---------------------------------------------------------------------------------- mix
@pytest.mark.parametrize("H", [8, 17, 64])
@pytest.mark.parametrize("act", [0, 1])
def test_mix(H, act):
    from glass_amd import ops
    n = 1234
    gen = torch.Generator().manual_seed(11)
    T = torch.randn(n, 2 * H, generator=gen)
    mask = torch.rand(n, generator=gen) < 0.3
    gout = torch.randn(n, H, generator=gen)
    zr = 0.85
    Tc = T.double().requires_grad_(True)
    a = torch.nn.functional.elu(Tc) if act else Tc
    ref = O._mix(mask.reshape(-1, 1), zr, a[:, :H], a[:, H:])
    ref.backward(gout.double())
    Tg = T.to(DEV).requires_grad_(True)
    out = ops.mix(Tg, mask.to(DEV).to(torch.uint8), zr, act)
    out.backward(gout.to(DEV))
    assert rel_inf(out.detach().cpu(), ref.detach()) < 1e-6
    assert rel_inf(Tg.grad.cpu(), Tc.grad) < 1e-6


# ---------------------------------------------------------------------------------- K6
@pytest.mark.parametrize("n,C", [(4998, 64), (1000, 17), (333, 8), (20000, 128), (513, 300), (70000, 64), (3, 4)])
@pytest.mark.parametrize("act", [0, 1])
def test_graphnorm(n, C, act):
    """(70000, 64): every statistics workgroup loops more than once; (3, 4): fewer rows than row slots."""
    from glass_amd import ops
    gen = torch.Generator().manual_seed(n + C)
    x = torch.randn(n, C, generator=gen) * 2.0 + 5.0  # mean 5 / std 2: the hard case for one-pass variance
    gamma = 1 + 0.3 * torch.randn(C, generator=gen)
    beta = 0.2 * torch.randn(C, generator=gen)
    alpha = 1 + 0.3 * torch.randn(C, generator=gen)
    gout = torch.randn(n, C, generator=gen)
    gn = O.GraphNorm(C).double()
    with torch.no_grad():
        gn.weight.copy_(gamma), gn.bias.copy_(beta), gn.mean_scale.copy_(alpha)
    xc = x.double().requires_grad_(True)
    ref = gn(xc)
    if act:
        ref = torch.nn.functional.elu(ref)
    ref.backward(gout.double())
    xg = x.to(DEV).requires_grad_(True)
    params = [t.to(DEV).requires_grad_(True) for t in (gamma, beta, alpha)]
    y = ops.graphnorm(xg, *params, 1e-5, act)
    y.backward(gout.to(DEV))
    assert rel_inf(y.detach().cpu(), ref.detach()) < TOL
    assert rel_inf(xg.grad.cpu(), xc.grad) < TOL
    for mine, theirs in zip(params, (gn.weight, gn.bias, gn.mean_scale)):
        assert rel_inf(mine.grad.cpu(), theirs.grad) < TOL


def test_graphnorm_strided_input_and_repeatable():
    from glass_amd import ops
    n, C = 5000, 64
    wide = torch.randn(n, 3 * C, device=DEV)
    x = wide[:, C:2 * C]
    ones, zeros = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    y1 = ops.graphnorm(x, ones, zeros, ones)
    y2 = ops.graphnorm(x.contiguous(), ones, zeros, ones)
    assert torch.equal(y1, y2)
    ref = O.GraphNorm(C)(x.cpu())
    assert rel_inf(y1.cpu(), ref.detach()) < TOL


def test_graphnorm_dropout_statistics():
    """Inverted dropout fused after GraphNorm: keep-rate, scaling, and the backward reuses the
    forward's mask (regenerated from the counter, not stored)."""
    from glass_amd import ops
    n, C, p = 20000, 64, 0.5
    x = torch.randn(n, C, device=DEV).requires_grad_(True)
    ones, zeros = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    ops.rng_seed(123, x.device)
    ops.rng_advance(x.device)
    y0 = ops.graphnorm(x, ones, zeros, ones)
    y = ops.graphnorm(x, ones, zeros, ones, p_drop=p, call_id=5)
    kept = y != 0
    rate = kept.float().mean().item()
    assert abs(rate - (1 - p)) < 0.01
    assert rel_inf(y[kept].cpu(), (y0[kept] / (1 - p)).cpu()) < 1e-6
    # same (seed, step, call_id) -> same mask; other call_id or next step -> different mask
    y_same = ops.graphnorm(x, ones, zeros, ones, p_drop=p, call_id=5)
    assert torch.equal(y_same, y)
    assert not torch.equal(ops.graphnorm(x, ones, zeros, ones, p_drop=p, call_id=6) != 0, kept)
    # backward: gradient flows only through kept elements.  d/dx of sum(y*w) through GraphNorm is
    # dense, so check the mask by linearity: grad(p) computed with upstream w must equal
    # grad(no-dropout) computed with upstream w * keepmask / (1-p).
    w = torch.randn(n, C, device=DEV)
    (g_drop, ) = torch.autograd.grad(y, x, w)
    (g_ref, ) = torch.autograd.grad(y0, x, w * kept / (1 - p))
    assert rel_inf(g_drop.cpu(), g_ref.cpu()) < 1e-5
    ops.rng_advance(x.device)
    assert not torch.equal(ops.graphnorm(x, ones, zeros, ones, p_drop=p, call_id=5) != 0, kept)


# ---------------------------------------------------------------------------------- K7
@pytest.mark.parametrize("mode", ["sum", "mean", "max", "size"])
def test_pool_g4(mode):
    from glass_amd import ops
    g = load("g4_pool.npz")
    e = torch.from_numpy(g["emb"]).to(DEV).requires_grad_(True)
    y = ops.segment_pool(e, torch.from_numpy(g["pos"]).to(DEV), mode)
    y.backward(torch.from_numpy(g["gout"]).to(DEV))
    assert rel_inf(y.detach().cpu(), g["y_" + mode]) < 1e-6
    assert rel_inf(e.grad.cpu(), g["grad_" + mode]) < 1e-6


@pytest.mark.parametrize("mode", ["sum", "mean", "max", "size"])
@pytest.mark.parametrize("C", [128, 17, 512])
def test_pool_ragged(mode, C):
    from glass_amd import ops
    n, B, S = 5000, 99, 40
    rng = np.random.default_rng(C)
    pos = np.full((B, S), -1, dtype=np.int64)
    for b in range(B):
        k = rng.integers(1, S + 1)
        pos[b, :k] = rng.choice(n, k, replace=False)
    pos[3, :] = -1  # an all-padding row pools to 0 (torch_scatter semantics for an empty segment)
    pos[4, :5] = pos[5, :5]  # nodes shared between subgraphs
    emb = torch.randn(n, C, generator=torch.Generator().manual_seed(C))
    gout = torch.randn(B, C, generator=torch.Generator().manual_seed(C + 1))
    post = torch.from_numpy(pos)
    ec = emb.double().requires_grad_(True)
    batch, p = O.pad_to_batch(post)
    ref = O.segment_pool(ec[p], batch, B, mode)
    ref.backward(gout.double())
    eg = emb.to(DEV).requires_grad_(True)
    y = ops.segment_pool(eg, post.to(DEV), mode)
    y.backward(gout.to(DEV))
    assert rel_inf(y.detach().cpu(), ref.detach()) < 1e-6
    assert float(y[3].abs().max()) == 0.0
    assert rel_inf(eg.grad.cpu(), ec.grad) < 1e-6
    g1 = eg.grad.clone()   # no float atomic in any mode (max: exact sums over the node's subgraph list): bitwise repeatable
    eg.grad = None
    ops.segment_pool(eg, post.to(DEV), mode).backward(gout.to(DEV))
    assert torch.equal(g1, eg.grad)


def test_pool_max_backward_with_repeated_nodes():
    """Max pooling's backward through the node-bucketed lists: a node named twice by one row (a tie between its own two
    entries) counts once for it, a node that wins most columns in every subgraph collects all their gradients."""
    from glass_amd import ops
    n, B, S, C = 50, 300, 9, 20
    rng = np.random.default_rng(3)
    pos = rng.integers(0, n, (B, S))
    pos[:, 3] = pos[:, 1]                   # a repeated node in every row
    pos[rng.random((B, S)) < 0.2] = -1
    pos[:, 0] = 5                           # node 5 in every subgraph
    emb = torch.randn(n, C, generator=torch.Generator().manual_seed(1))
    emb[5] += 3.0                           # node 5 wins most columns everywhere
    gout = torch.randn(B, C, generator=torch.Generator().manual_seed(2))
    post = torch.from_numpy(pos)
    ec = emb.double().requires_grad_(True)
    batch, p = O.pad_to_batch(post)
    O.segment_pool(ec[p], batch, B, "max").backward(gout.double())
    eg = emb.to(DEV).requires_grad_(True)
    y = ops.segment_pool(eg, post.to(DEV), "max")
    y.backward(gout.to(DEV))
    assert rel_inf(eg.grad.cpu(), ec.grad) < 1e-6
    g1 = eg.grad.clone()
    eg.grad = None
    ops.segment_pool(eg, post.to(DEV), "max").backward(gout.to(DEV))
    assert torch.equal(g1, eg.grad)


@pytest.mark.parametrize("mode", ["sum", "mean", "size"])
@pytest.mark.parametrize("C", [64, 17])
def test_pool_backward_beyond_lds_staging_is_exact_and_repeatable(mode, C):
    """Padded node matrices beyond the ordered scatter's LDS staging (12 288 entries): the backward buckets the entries by
    node and sums in exact fixed point instead of falling back to float atomics — vs fp64, bitwise repeatable, a node
    shared by every subgraph (its list is summed by the whole workgroup), an all-padding row, no warning."""
    import warnings
    from glass_amd import ops
    n, B, S = 4000, 500, 37
    rng = np.random.default_rng(C + 7)
    pos = np.full((B, S), -1, dtype=np.int64)
    for b in range(B):
        k = rng.integers(1, S)
        pos[b, :k] = rng.choice(n - 100, k, replace=False) + 1
        pos[b, k] = 0      # node 0 sits in every subgraph
    pos[3, :] = -1
    emb = torch.randn(n, C, generator=torch.Generator().manual_seed(C))
    gout = torch.randn(B, C, generator=torch.Generator().manual_seed(C + 1))
    post = torch.from_numpy(pos)
    ec = emb.double().requires_grad_(True)
    batch, p = O.pad_to_batch(post)
    O.segment_pool(ec[p], batch, B, mode).backward(gout.double())
    eg = emb.to(DEV).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ops.segment_pool(eg, post.to(DEV), mode).backward(gout.to(DEV))
    assert rel_inf(eg.grad.cpu(), ec.grad) < 1e-6
    assert float(eg.grad[n - 99:].abs().max()) == 0.0
    g1 = eg.grad.clone()
    eg.grad = None
    ops.segment_pool(eg, post.to(DEV), mode).backward(gout.to(DEV))
    assert torch.equal(g1, eg.grad)


@pytest.mark.parametrize("mode", ["sum", "mean", "size"])
@pytest.mark.parametrize("C", [64, 20, 17, 320])
def test_pair_pool(mode, C):
    """Node pairs (the pre-training path's link batches): lane-group kernels; the backward is bucketed by node and summed in
    exact fixed point — no float atomic, bitwise repeatable; padding entries, a hub node whose list the whole workgroup sums,
    nodes no pair names (zero rows), a wider (strided) embedding buffer."""
    from glass_amd import ops
    n, B = 3000, 20000
    rng = np.random.default_rng(C)
    pairs = rng.integers(0, n - 50, size=(B, 2))   # the last 50 nodes are named by no pair
    pairs[::7, 0] = 11                              # hub: ~2900 entries
    pairs[5, 1] = -1                                # one-sided pair
    pairs[6, :] = -1                                # empty pair -> 0
    wide = torch.randn(n, C + 4, generator=torch.Generator().manual_seed(C))
    gout = torch.randn(B, C, generator=torch.Generator().manual_seed(C + 1))
    post = torch.from_numpy(pairs)
    ec = wide[:, :C].double().requires_grad_(True)
    batch, p = O.pad_to_batch(post)
    ref = O.segment_pool(ec[p], batch, B, mode)
    ref.backward(gout.double())
    wg = wide.to(DEV)
    eg = wg[:, :C].requires_grad_(True)
    y = ops.segment_pool(eg, post.to(DEV), mode)
    y.backward(gout.to(DEV))
    assert rel_inf(y.detach().cpu(), ref.detach()) < 1e-6
    assert float(y[6].abs().max()) == 0.0
    assert rel_inf(eg.grad.cpu(), ec.grad) < 1e-6
    assert float(eg.grad[n - 50:].abs().max()) == 0.0
    g1 = eg.grad.clone()
    eg.grad = None
    ops.segment_pool(eg, post.to(DEV), mode).backward(gout.to(DEV))
    assert torch.equal(g1, eg.grad)


@pytest.mark.parametrize("N,O,I", [(131072, 1, 64), (5000, 2, 20), (77, 3, 256), (100000, 1, 320)])
def test_linear_wgrad_thin_outputs(N, O, I):
    """Weight / bias gradient of a Linear with 1-3 outputs (the pre-training head's hidden -> 1 layer) on the thin kernels
    instead of a library GEMM: vs fp64, accumulate mode, repeatable."""
    from glass_amd import ops
    gen = torch.Generator().manual_seed(N + O)
    G = torch.randn(N, O, generator=gen)
    X = torch.randn(N, I, generator=gen)
    Gg, Xg = G.to(DEV), X.to(DEV)
    ref_w, ref_b = G.double().t() @ X.double(), G.double().sum(0)
    dW, db = torch.full((O, I), 3.0, device=DEV), torch.full((O, ), -2.0, device=DEV)
    assert ops.linear_wgrad(Gg, Xg, dW, db, False)
    assert rel_inf(dW.cpu(), ref_w) < TOL and rel_inf(db.cpu(), ref_b) < TOL
    dW2, db2 = torch.empty_like(dW), torch.empty_like(db)
    ops.linear_wgrad(Gg, Xg, dW2, db2, False)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    ops.linear_wgrad(Gg, Xg, dW2, db2, True)
    assert rel_inf(dW2.cpu(), 2 * ref_w) < TOL and rel_inf(db2.cpu(), 2 * ref_b) < TOL
    lin = torch.nn.Linear(I, O).to(DEV)
    xg = Xg.clone().requires_grad_(True)
    ops.linear(xg, lin).backward(Gg)
    assert rel_inf(lin.weight.grad.cpu(), ref_w) < TOL and rel_inf(xg.grad.cpu(), G.double() @ lin.weight.detach().cpu().double()) < TOL


def test_pool_unknown_mode_raises():
    from glass_amd import ops
    with pytest.raises(NotImplementedError):
        ops.segment_pool(torch.randn(4, 4, device=DEV), torch.zeros(1, 2, dtype=torch.int64, device=DEV), "median")


def test_cpu_tensor_fails_loudly():
    """No CPU fallback: the product path refuses CPU tensors instead of computing on the host."""
    from glass_amd import ops
    from glass_amd._lib import GlassHipError
    with pytest.raises(GlassHipError):
        ops.graphnorm(torch.randn(8, 4), torch.ones(4), torch.zeros(4), torch.ones(4))
    with pytest.raises(GlassHipError):
        ops.maxzoz(10, torch.zeros(2, 2, dtype=torch.int64))


# ---------------------------------------------------------------------------------- K5w, K9
@pytest.mark.parametrize("N,O,I", [(17080, 128, 64), (17080, 128, 128), (1000, 16, 8), (333, 40, 20), (70000, 256, 128),
                                   (5, 128, 64)])
def test_linear_wgrad(N, O, I):
    """Split-K fp32-MFMA weight/bias gradient vs an fp64 GEMM; overwrite and accumulate modes;
    strided operands (X as the right half of a wider buffer); bitwise repeatable."""
    from glass_amd import ops
    gen = torch.Generator().manual_seed(N + O)
    G = torch.randn(N, O, generator=gen)
    wide = torch.randn(N, 2 * I, generator=gen)
    Gg, wg = G.to(DEV), wide.to(DEV)
    X = wg[:, I:]
    ref_w = G.double().t() @ wide[:, I:].double()
    ref_b = G.double().sum(0)
    dW = torch.full((O, I), 3.0, device=DEV)
    db = torch.full((O, ), -2.0, device=DEV)
    assert ops.linear_wgrad(Gg, X, dW, db, False)
    assert rel_inf(dW.cpu(), ref_w) < TOL and rel_inf(db.cpu(), ref_b) < TOL
    dW2, db2 = torch.empty_like(dW), torch.empty_like(db)
    ops.linear_wgrad(Gg, X, dW2, db2, False)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    ops.linear_wgrad(Gg, X, dW2, db2, True)  # accumulate on top
    assert rel_inf(dW2.cpu(), 2 * ref_w) < TOL and rel_inf(db2.cpu(), 2 * ref_b) < TOL


def test_linear_wgrad_unsupported_shape_falls_back_to_library_gemm():
    from glass_amd import ops
    G, X = torch.randn(50, 17, device=DEV), torch.randn(50, 17, device=DEV)
    assert ops.linear_wgrad(G, X, torch.empty(17, 17, device=DEV), None, False) is False


def test_stacked_linear_matches_two_linears():
    from glass_amd import ops
    import torch.nn as nn
    torch.manual_seed(0)
    l1, l0 = nn.Linear(64, 64).to(DEV), nn.Linear(64, 64).to(DEV)
    x = torch.randn(3000, 64, device=DEV, requires_grad=True)
    gout = torch.randn(3000, 128, device=DEV)
    T = ops.stacked_linear(x, l1, l0)
    T.backward(gout)
    got = [x.grad.clone(), l1.weight.grad.clone(), l0.weight.grad.clone(), l1.bias.grad.clone(), l0.bias.grad.clone()]
    x.grad = None
    for p in list(l1.parameters()) + list(l0.parameters()):
        p.grad = None
    xd = x.detach().double().requires_grad_(True)
    l1d, l0d = nn.Linear(64, 64).double().to(DEV), nn.Linear(64, 64).double().to(DEV)
    l1d.load_state_dict({k: v.double() for k, v in l1.state_dict().items()})
    l0d.load_state_dict({k: v.double() for k, v in l0.state_dict().items()})
    Td = torch.cat((l1d(xd), l0d(xd)), -1)
    Td.backward(gout.double())
    want = [xd.grad, l1d.weight.grad, l0d.weight.grad, l1d.bias.grad, l0d.bias.grad]
    assert rel_inf(T.detach().cpu(), Td.detach().cpu()) < TOL
    for a, b in zip(got, want):
        assert rel_inf(a.cpu(), b.cpu()) < TOL


def test_flat_adam_matches_torch_adam():
    """glass_adam_step_f32 over a ParamArena == torch.optim.Adam, 5 steps, incl. a learning-rate change
    made the way ReduceLROnPlateau makes it (param_groups[0]['lr'])."""
    import copy
    import torch.nn as nn
    from glass_amd.arena import ParamArena
    from glass_amd.optim import FlatAdam
    torch.manual_seed(0)
    a = nn.Sequential(nn.Linear(20, 33), nn.ELU(), nn.Linear(33, 7)).to(DEV)
    b = copy.deepcopy(a)
    arena = ParamArena(a)
    oa, ob = FlatAdam(arena, lr=1e-2), torch.optim.Adam(b.parameters(), lr=1e-2)
    for step in range(5):
        x = torch.randn(64, 20, device=DEV)
        if step == 3:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 2e-3
        for m, o in ((a, oa), (b, ob)):
            o.zero_grad()
            m(x).pow(2).mean().backward()
            o.step()
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert rel_inf(pa.detach().cpu(), pb.detach().cpu()) < 1e-6
    assert arena.attached()
    assert oa.step_dev.tolist() == [5, 0]  # (steps completed, ticket back at zero): counted inside the Adam launch


def test_pack_launch_advances_dropout_stream():
    """glass_dense_pack_batch_f32(rng_state) == pack + glass_rng_advance in one launch."""
    from glass_amd import _lib, ops
    dev = torch.device(DEV)
    ops.rng_seed(77, dev)
    st = ops.rng_state(dev)
    W = torch.randn(128, 64, device=DEV)
    img = torch.empty(W.numel(), device=DEV)
    src, dst = np.array([W.data_ptr()], dtype=np.uint64), np.array([img.data_ptr()], dtype=np.uint64)
    nts, kts, trs = np.array([128], dtype=np.int64), np.array([64], dtype=np.int64), np.array([0], dtype=np.int32)
    caps = np.array([img.numel()], dtype=np.int64)
    for expect in (1, 2):
        rc = _lib.load().glass_dense_pack_batch_f32(src.ctypes.data, dst.ctypes.data, caps.ctypes.data, nts.ctypes.data, kts.ctypes.data,
                                                    trs.ctypes.data, 0, 1, st.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0 and st.tolist() == [77, expect]
    assert torch.equal(img, _pack(W, False))
    rc = _lib.load().glass_dense_pack_batch_f32(0, 0, 0, 0, 0, 0, 0, 0, st.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc != 0  # null arrays are rejected even for zero jobs
    # a destination smaller than the layout's image is refused before any launch (the image sizes differ by layout)
    small = np.array([img.numel() - 1], dtype=np.int64)
    rc = _lib.load().glass_dense_pack_batch_f32(src.ctypes.data, dst.ctypes.data, small.ctypes.data, nts.ctypes.data, kts.ctypes.data,
                                                trs.ctypes.data, 0, 1, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == -1 and b"glass_dense_image_floats" in _lib.load().glass_last_error_string()
    # a tiled layout carries the cut image behind the fp32 image: NT*KT floats are NOT enough there
    W2, img2 = torch.randn(256, 128, device=DEV), torch.empty(256 * 128, device=DEV)
    a = [np.array([v], dtype=t) for v, t in ((W2.data_ptr(), np.uint64), (img2.data_ptr(), np.uint64), (img2.numel(), np.int64),
                                             (256, np.int64), (128, np.int64), (0 | (1 << 1), np.int32))]
    rc = _lib.load().glass_dense_pack_batch_f32(*(v.ctypes.data for v in a), 0, 1, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == -1


def test_graphnorm_scratch_reuse_stress():
    """Column partials pass from the statistics kernel to the finalize kernel through one scratch buffer
    that every GraphNorm call on the device reuses.  400 back-to-back launches over changing inputs, with
    a second stream keeping the chip unevenly busy; every launch must reproduce its statistics bitwise
    (a stale partial would be an O(1) error).  (A single-launch variant in which the last workgroup to
    arrive finalizes was built and measured: no faster than the kernel boundary — DESIGN.md.)"""
    from glass_amd import ops
    n, C = 17080, 64
    xs = [torch.randn(n, C, device=DEV) * (1 + k) + k for k in range(8)]
    refs = []
    for x in xs:
        xd = x.double()
        refs.append(((xd - xd.mean(0)) / (xd.var(0, unbiased=False) + 1e-5).sqrt()).float())
    ones, zeros = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    first = [ops.graphnorm(x, ones, zeros, ones) for x in xs]
    for y, r in zip(first, refs):
        assert rel_inf(y.cpu(), r.cpu()) < 1e-6
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=DEV)
    bad = 0
    for it in range(400):
        if it % 7 == 0:
            with torch.cuda.stream(side):
                for _ in range(3):
                    a = (a @ a).clamp_(-1, 1)
        k = (it * 5) % 8
        y = ops.graphnorm(xs[k], ones, zeros, ones)
        bad += int(not torch.equal(y, first[k]))  # bitwise equal to the first evaluation
    torch.cuda.synchronize()
    assert bad == 0
    # backward hand-off too
    x = xs[3].clone().requires_grad_(True)
    g = torch.randn(n, C, device=DEV)
    (d0, ) = torch.autograd.grad(ops.graphnorm(x, ones, zeros, ones, 1e-5, 1), x, g)
    for _ in range(100):
        (d, ) = torch.autograd.grad(ops.graphnorm(x, ones, zeros, ones, 1e-5, 1), x, g)
        bad += int(not torch.equal(d, d0))
    assert bad == 0


# ---------------------------------------------------------------------------------- K5 fused dense
@pytest.mark.parametrize("H,N", [(64, 17080), (64, 77), (128, 5000), (128, 1030), (128, 50003), (128, 63), (128, 1), (128, 17),
                                 (256, 2100), (256, 33), (256, 70001), (512, 300)])
@pytest.mark.parametrize("comb", [False, True])
def test_dual_linear_mix_fused(H, N, comb):
    """Fused (Linear pair + ELU + mix) MFMA kernels vs an fp64 composition of nn.Linear, ELU and the mix:
    forward, data gradient (both inputs for the comb pair) and weight / bias gradients accumulated into the
    arena.  Inputs are strided views (the comb pair reads [g || x_] in place).  Hidden 256: the LDS-tiled kernels
    (row counts off their 128-row tile); N = 70 001 also takes the tiled weight-gradient kernel (N >= 65 536)."""
    import torch.nn as nn
    from glass_amd import ops
    gen = torch.Generator().manual_seed(H + N)
    K = 2 * H if comb else H
    act = 0 if comb else 1
    zr = 0.85
    W = torch.randn(2 * H, K, generator=gen) / K**0.5
    b = torch.randn(2 * H, generator=gen) * 0.1
    wide_a, wide_b = torch.randn(N, H + 4, generator=gen), torch.randn(N, 2 * H, generator=gen)
    mask = torch.rand(N, generator=gen) < 0.3
    gout = torch.randn(N, H, generator=gen)
    # fp64 reference
    xa64 = wide_a[:, :H].double().requires_grad_(True)
    xb64 = wide_b[:, H:].double().requires_grad_(True)
    W64, b64 = W.double().requires_grad_(True), b.double().requires_grad_(True)
    xin = torch.cat((xa64, xb64), -1) if comb else xa64
    Z = xin @ W64.t() + b64
    A = torch.nn.functional.elu(Z) if act else Z
    ref = O._mix(mask.reshape(-1, 1), zr, A[:, :H], A[:, H:])
    ref.backward(gout.double())
    # HIP
    Wg, bg = W.to(DEV), b.to(DEV)
    dW, db = torch.zeros_like(Wg), torch.zeros_like(bg)
    Wimg, WTimg = _pack(Wg, False, H, zr), _pack(Wg, True, H, zr)
    lin1, lin0 = nn.Linear(K, H).to(DEV), nn.Linear(K, H).to(DEV)  # carriers for the autograd edges only
    # as under a ParamArena: the parameters' .grad ARE views of the stacked gradient buffers (the in-place path is only
    # taken while that holds: ops._arena_grads_live)
    lin1.weight.grad, lin0.weight.grad, lin1.bias.grad, lin0.bias.grad = dW[:H], dW[H:], db[:H], db[H:]
    xa = wide_a.to(DEV)[:, :H].requires_grad_(True)
    xb = wide_b.to(DEV)[:, H:].requires_grad_(True) if comb else None
    out = ops.dual_linear_mix(xa, xb, lin1, lin0, mask.to(DEV).to(torch.uint8), zr, act, (Wg, bg, dW, db, Wimg, WTimg))
    out.backward(gout.to(DEV))
    assert rel_inf(out.detach().cpu(), ref.detach()) < TOL
    assert rel_inf(xa.grad.cpu(), xa64.grad) < TOL
    if comb:
        assert rel_inf(xb.grad.cpu(), xb64.grad) < TOL
    assert rel_inf(dW.cpu(), W64.grad) < TOL
    assert rel_inf(db.cpu(), b64.grad) < TOL
    out2 = ops.dual_linear_mix(xa.detach(), None if xb is None else xb.detach(), lin1, lin0,
                               mask.to(DEV).to(torch.uint8), zr, act, (Wg, bg, dW, db, Wimg, WTimg))
    assert torch.equal(out2, out.detach())


@pytest.mark.parametrize("N,H", [(71680, 256), (70001, 256), (65536 + 17, 256), (65536 + 40, 512)])
@pytest.mark.parametrize("comb,act", [(False, 1), (False, 2), (False, 0), (True, 0)])
def test_tiled_wgrad_eight_wave_kernel(N, H, comb, act):
    """glass_dual_linear_wgrad_f32 at hidden 256 / 512 on a graph of >= 65 536 rows: the all-rows tiles run on the eight-wave kernel
    (wgrad_tiled.hip: three stages of raw rows in flight, rows past a slab read as zero through the buffer resource, one
    16-bit load for a thread's two label bytes).  N = 71 680 gives 128 slabs — the XCD-aware placement; the other sizes a slab
    count that is not a multiple of 8 (plain placement) and a ragged last slab.  ELU / ReLU / no activation for the trans
    pair (pre-activations NULL without one), the comb pair in effective-weight form (labeled-rows tiles on the four-wave
    kernel); vs the fp64 sums, twice (bitwise repeat: no atomics, fixed slab order)."""
    from glass_amd import ops, _lib
    lib = _lib.load()
    gen = torch.Generator().manual_seed(N + 7 * act + comb)
    zr = 0.8
    dsrc = torch.randn(N, H + 8, generator=gen)[:, 4:4 + H]  # strided views: ld = H + 8, 16-B aligned columns
    T = torch.randn(N, 2 * H, generator=gen)
    X = torch.randn(N, H, generator=gen)
    X2 = torch.randn(N, H, generator=gen) if comb else None
    mask = torch.rand(N, generator=gen) < 0.01
    mask[-1] = True   # odd N: the last slab's final row pair (N - 1, N) straddles the label resource's end — the last real
    mask[-4] = True   # row's byte must not read as 0 (a partly out-of-range 16-bit buffer load returns 0 for both bytes)
    # fp64: G[n, o] = coef(mask[n], o < H) * dsrc[n, o mod H] * act'(T[n, o]);  dW = G^T [X | X2],  db = column sums of G
    c1 = torch.where(mask, zr, 1 - zr).double().reshape(-1, 1)
    G = torch.cat((c1 * dsrc.double(), (1 - c1) * dsrc.double()), 1)
    if act == 1:
        G = G * torch.where(T > 0, torch.ones(()), torch.exp(T)).double()
    elif act == 2:
        G = G * (T > 0).double()
    Xin = torch.cat((X, X2), 1).double() if comb else X.double()
    dW_ref, db_ref = G.t() @ Xin, G.sum(0)
    dg, Tg, Xg, mg = dsrc.to(DEV), T.to(DEV), X.to(DEV), mask.to(DEV).to(torch.uint8)
    dg = torch.randn(N, H + 8, device=DEV)
    dg[:, 4:4 + H] = dsrc.to(DEV)
    dgv = dg[:, 4:4 + H]
    X2g = X2.to(DEV) if comb else None
    I = 2 * H if comb else H
    ws = ops._wgrad_workspace(torch.device(DEV), N, 2 * H, I, slot=("t8", N, H, comb, act))
    got = []
    for _ in range(2):
        dW = torch.full((2 * H, I), float("nan"), device=DEV)
        db = torch.full((2 * H,), float("nan"), device=DEV)
        rc = lib.glass_dual_linear_wgrad_f32(dgv.data_ptr(), dgv.stride(0), Tg.data_ptr() if act else 0, Tg.stride(0) if act else 0,
                                             mg.data_ptr(), zr, ops.act_word(act), Xg.data_ptr(), Xg.stride(0),
                                             0 if X2g is None else X2g.data_ptr(), 0 if X2g is None else X2g.stride(0), N, H,
                                             dW.data_ptr(), dW.stride(0), db.data_ptr(), 0, ws.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.glass_last_error_string()
        got.append((dW.cpu(), db.cpu()))
    assert rel_inf(got[0][0], dW_ref) < TOL and rel_inf(got[0][1], db_ref) < TOL
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    record_parity(f"kernel/tiled_wgrad8_H{H}_N{N}_{'comb' if comb else 'trans'}_act{act}", dW_rel_inf=rel_inf(got[0][0], dW_ref),
                  db_rel_inf=rel_inf(got[0][1], db_ref))
    if N == 70001 and not comb and act == 1:  # a label mask at an odd address is refused, not misread (one 16-bit load per row pair)
        odd = torch.zeros(N + 1, dtype=torch.uint8, device=DEV)[1:]
        rc = lib.glass_dual_linear_wgrad_f32(dgv.data_ptr(), dgv.stride(0), Tg.data_ptr(), Tg.stride(0), odd.data_ptr(), zr,
                                             ops.act_word(act), Xg.data_ptr(), Xg.stride(0), 0, 0, N, H, dW.data_ptr(), dW.stride(0),
                                             db.data_ptr(), 0, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc != 0 and b"2-byte" in lib.glass_last_error_string()


@pytest.mark.parametrize("N", [8192, 50003, 70001, 100000 + 31])
@pytest.mark.parametrize("act", [1, 2, 0])
def test_wgrad128_rows_shared_through_lds(N, act):
    """glass_dual_linear_wgrad_f32 for the trans pair of hidden 128 on a mid-size graph (round 6, wgrad128.hip: one workgroup per
    slab, the slab's rows requested once and shared through LDS as swizzled bf16 images, all four 128 x 64 tiles from 16
    accumulator tiles per wave): dW, db against the fp64 sums for ELU / ReLU / no activation, odd N (a slab that ends inside a
    row pair, the last row labeled), strided operands; twice -> identical bits (no atomics, fixed slab order); the f32-input
    product form of the same call (the register-pipelined kernel on the same slab geometry) against the same sums."""
    from glass_amd import ops, _lib
    lib = _lib.load()
    H = 128
    gen = torch.Generator().manual_seed(N + act)
    zr = 0.8
    dsrc = torch.randn(N, H, generator=gen)
    T = torch.randn(N, 2 * H, generator=gen)
    X = torch.randn(N, H, generator=gen)
    mask = torch.rand(N, generator=gen) < 0.02
    mask[-1] = True
    c1 = torch.where(mask, zr, 1 - zr).double().reshape(-1, 1)
    G = torch.cat((c1 * dsrc.double(), (1 - c1) * dsrc.double()), 1)
    if act == 1:
        G = G * torch.where(T > 0, torch.ones(()), torch.exp(T)).double()
    elif act == 2:
        G = G * (T > 0).double()
    dW_ref, db_ref = G.t() @ X.double(), G.sum(0)
    dg = torch.randn(N, H + 8, device=DEV)
    dg[:, 4:4 + H] = dsrc.to(DEV)
    dgv = dg[:, 4:4 + H]   # strided: ld = H + 8, 16-B aligned columns
    Tg, Xg, mg = T.to(DEV), X.to(DEV), mask.to(DEV).to(torch.uint8)
    ws = ops._wgrad_workspace(torch.device(DEV), N, 2 * H, H, slot=("w128", N, act))
    prev = ops.DENSE_F32_PRODUCTS
    try:
        for form in (False, True):
            ops.DENSE_F32_PRODUCTS = form
            got = []
            for _ in range(2):
                dW = torch.full((2 * H, H), float("nan"), device=DEV)
                db = torch.full((2 * H,), float("nan"), device=DEV)
                rc = lib.glass_dual_linear_wgrad_f32(dgv.data_ptr(), dgv.stride(0), Tg.data_ptr() if act else 0, Tg.stride(0) if act else 0,
                                                     mg.data_ptr(), zr, ops.act_word(act), Xg.data_ptr(), Xg.stride(0), 0, 0, N, H,
                                                     dW.data_ptr(), dW.stride(0), db.data_ptr(), 0, ws.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream)
                assert rc == 0, lib.glass_last_error_string()
                got.append((dW.cpu(), db.cpu()))
            e_w, e_b = rel_inf(got[0][0], dW_ref), rel_inf(got[0][1], db_ref)
            assert e_w < TOL and e_b < TOL, (form, e_w, e_b)
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
            if not form:
                record_parity(f"kernel/wgrad128_lds_N{N}_act{act}", dW_rel_inf=e_w, db_rel_inf=e_b)
    finally:
        ops.DENSE_F32_PRODUCTS = prev


@pytest.mark.parametrize("N,labeled", [(8192, "few"), (50003, "few"), (50003, "none"), (9001, "all"), (100000 + 31, "dense")])
def test_wgrad128_comb_pair_list_tiles(N, labeled):
    """glass_dual_linear_wgrad_f32 for the COMB pair of hidden 128 on a mid-size graph (round 6, wgrad128_comb_kernel: S tile per
    slab with the rows shared through LDS, the labeled rows as LIST tiles — n_l trailing workgroups each scan one chunk of the
    label bytes — and the batched reduce's form 3): dW [256 x 256], db against the fp64 sums with a batch-like label density,
    no labeled row at all, EVERY row labeled (L = S: the list workgroups walk whole chunks) and a third of the rows; odd N, the
    last row labeled; twice -> identical bits; the f32-input product form of the same call on the same geometry."""
    from glass_amd import ops, _lib
    lib = _lib.load()
    H = 128
    gen = torch.Generator().manual_seed(N + len(labeled))
    zr = 0.8
    dsrc = torch.randn(N, H, generator=gen)
    X = torch.randn(N, H, generator=gen)
    X2 = torch.randn(N, H, generator=gen)
    mask = {"few": torch.rand(N, generator=gen) < 0.02, "none": torch.zeros(N, dtype=torch.bool),
            "all": torch.ones(N, dtype=torch.bool), "dense": torch.rand(N, generator=gen) < 0.33}[labeled]
    if labeled == "few":
        mask[-1] = True
    c1 = torch.where(mask, zr, 1 - zr).double().reshape(-1, 1)
    G = torch.cat((c1 * dsrc.double(), (1 - c1) * dsrc.double()), 1)
    dW_ref, db_ref = G.t() @ torch.cat((X, X2), 1).double(), G.sum(0)
    dg, Xg, X2g, mg = dsrc.to(DEV), X.to(DEV), X2.to(DEV), mask.to(DEV).to(torch.uint8)
    ws = ops._wgrad_workspace(torch.device(DEV), N, 2 * H, 2 * H, slot=("w128c", N, labeled))
    prev = ops.DENSE_F32_PRODUCTS
    try:
        for form in (False, True):
            ops.DENSE_F32_PRODUCTS = form
            got = []
            for _ in range(2):
                dW = torch.full((2 * H, 2 * H), float("nan"), device=DEV)
                db = torch.full((2 * H,), float("nan"), device=DEV)
                rc = lib.glass_dual_linear_wgrad_f32(dg.data_ptr(), dg.stride(0), 0, 0, mg.data_ptr(), zr, ops.act_word(0), Xg.data_ptr(),
                                                     Xg.stride(0), X2g.data_ptr(), X2g.stride(0), N, H, dW.data_ptr(), dW.stride(0),
                                                     db.data_ptr(), 0, ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
                assert rc == 0, lib.glass_last_error_string()
                got.append((dW.cpu(), db.cpu()))
            e_w, e_b = rel_inf(got[0][0], dW_ref), rel_inf(got[0][1], db_ref)
            assert e_w < TOL and e_b < TOL, (form, e_w, e_b)
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
            if not form:
                record_parity(f"kernel/wgrad128_comb_N{N}_{labeled}", dW_rel_inf=e_w, db_rel_inf=e_b)
    finally:
        ops.DENSE_F32_PRODUCTS = prev


def _canaried_ws(N, O, I):
    """Workspace of exactly glass_linear_wgrad_ws_bytes(N, O, I) with a NaN-filled canary region right behind it."""
    from glass_amd import _lib
    nbytes = int(_lib.load().glass_linear_wgrad_ws_bytes(N, O, I))
    assert nbytes > 0 and nbytes % 4 == 0
    buf = torch.full((nbytes // 4 + 16384, ), float("nan"), device=DEV)
    return buf, nbytes // 4, buf[nbytes // 4:].clone().view(torch.int32)


def _wgrad_off_dispatch_check(tag, call, buf, n_ws, canary, dW_ref, db_ref):
    """Both product forms: dW, db against the fp64 sums, two calls bit-identical, the canary behind the workspace untouched."""
    from glass_amd import ops
    prev = ops.DENSE_F32_PRODUCTS
    try:
        for form in (False, True):
            ops.DENSE_F32_PRODUCTS = form
            got = [call() for _ in range(2)]
            e_w, e_b = rel_inf(got[0][0], dW_ref), rel_inf(got[0][1], db_ref)
            assert torch.equal(buf[n_ws:].view(torch.int32).cpu(), canary.cpu()), f"{tag}: written past the workspace (f32 form {form})"
            assert e_w < TOL and e_b < TOL, (tag, form, e_w, e_b)
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), (tag, form)
            if not form:
                record_parity(f"kernel/{tag}", dW_rel_inf=e_w, db_rel_inf=e_b)
    finally:
        ops.DENSE_F32_PRODUCTS = prev


@pytest.mark.parametrize("N", [8192, 50003, 400001])
@pytest.mark.parametrize("pair,labeled", [("trans", "few"), ("comb", "few"), ("comb", "none"), ("comb", "all")])
def test_wgrad128_shapes_off_the_wgrad128_dispatch(N, pair, labeled):
    """glass_dual_linear_wgrad_f32 at hidden 128 on the wgrad128 row range with the wgrad128 kernels refused by their
    alignment predicate (trans pair: ld of X = H + 2; comb pair: ld of X2 = H + 2): wgrad_geom still sizes the slabs, the
    generic or split kernel runs on them.  dW, db against the fp64 sums in both product forms, bitwise repeat, and nothing
    written past glass_linear_wgrad_ws_bytes."""
    from glass_amd import ops, _lib
    lib = _lib.load()
    H = 128
    gen = torch.Generator().manual_seed(N + 3 * len(labeled) + len(pair))
    zr = 0.8
    dsrc = torch.randn(N, H, generator=gen)
    X = torch.randn(N, H + 2, generator=gen) if pair == "trans" else torch.randn(N, H, generator=gen)
    X2 = torch.randn(N, H + 2, generator=gen) if pair == "comb" else None
    T = torch.randn(N, 2 * H, generator=gen) if pair == "trans" else None
    mask = {"few": torch.rand(N, generator=gen) < 0.02, "none": torch.zeros(N, dtype=torch.bool),
            "all": torch.ones(N, dtype=torch.bool)}[labeled]
    if labeled == "few":
        mask[-1] = True
    act = 1 if pair == "trans" else 0
    c1 = torch.where(mask, zr, 1 - zr).double().reshape(-1, 1)
    G = torch.cat((c1 * dsrc.double(), (1 - c1) * dsrc.double()), 1)
    if act:
        G = G * torch.where(T > 0, torch.ones(()), torch.exp(T)).double()
    Xin = X[:, :H].double() if X2 is None else torch.cat((X, X2[:, :H]), 1).double()
    dW_ref, db_ref = G.t() @ Xin, G.sum(0)
    I = Xin.shape[1]
    dg, Xg, mg = dsrc.to(DEV), X.to(DEV), mask.to(DEV).to(torch.uint8)
    Tg = T.to(DEV) if act else None
    X2g = X2.to(DEV) if X2 is not None else None
    assert (Xg.stride(0) if X2g is None else X2g.stride(0)) % 4 == 2
    buf, n_ws, canary = _canaried_ws(N, 2 * H, I)

    def call():
        dW = torch.full((2 * H, I), float("nan"), device=DEV)
        db = torch.full((2 * H, ), float("nan"), device=DEV)
        rc = lib.glass_dual_linear_wgrad_f32(dg.data_ptr(), dg.stride(0), Tg.data_ptr() if act else 0, Tg.stride(0) if act else 0,
                                             mg.data_ptr(), zr, ops.act_word(act), Xg.data_ptr(), Xg.stride(0),
                                             0 if X2g is None else X2g.data_ptr(), 0 if X2g is None else X2g.stride(0), N, H,
                                             dW.data_ptr(), dW.stride(0), db.data_ptr(), 0, buf.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.glass_last_error_string()
        return dW.cpu(), db.cpu()
    _wgrad_off_dispatch_check(f"wgrad128_off_dispatch_{pair}_{labeled}_N{N}", call, buf, n_ws, canary, dW_ref, db_ref)


@pytest.mark.parametrize("N", [8192, 100031])
def test_linear_wgrad_on_wgrad128_geometry(N):
    """glass_linear_wgrad_f32 with O = 256, I = 128 (the trans pair's shape, which wgrad_geom gives the wgrad128 slab geometry)
    runs the generic kernel on that geometry: dW, db against the fp64 sums, bitwise repeat, nothing written past
    glass_linear_wgrad_ws_bytes."""
    from glass_amd import _lib
    lib = _lib.load()
    O_, I = 256, 128
    gen = torch.Generator().manual_seed(N + 11)
    G = torch.randn(N, O_, generator=gen)
    X = torch.randn(N, I, generator=gen)
    dW_ref, db_ref = G.double().t() @ X.double(), G.double().sum(0)
    Gg, Xg = G.to(DEV), X.to(DEV)
    buf, n_ws, canary = _canaried_ws(N, O_, I)

    def call():
        dW = torch.full((O_, I), float("nan"), device=DEV)
        db = torch.full((O_, ), float("nan"), device=DEV)
        rc = lib.glass_linear_wgrad_f32(Gg.data_ptr(), Gg.stride(0), Xg.data_ptr(), Xg.stride(0), N, O_, I, dW.data_ptr(),
                                        dW.stride(0), db.data_ptr(), 0, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.glass_last_error_string()
        return dW.cpu(), db.cpu()
    _wgrad_off_dispatch_check(f"linear_wgrad_O256_I128_N{N}", call, buf, n_ws, canary, dW_ref, db_ref)


@pytest.mark.parametrize("H,N,comb", [(128, 3001, False), (256, 4099, False), (256, 4099, True), (256, 70001, True),
                                      # hidden 64 (round 6: the staged forward kernels take the split form too)
                                      (64, 3001, False), (64, 17080, False), (64, 3001, True)])
def test_both_product_forms_against_fp64(H, N, comb):
    """The LDS-tiled kernels (forward, data gradient, weight gradient) once per product form — the f32-input MFMA and the six
    bf16 partial products of 3-way split operands (split_mma.h) — against the same fp64 composition: the split form is as
    close as the f32-input instruction (within a factor of two, plus a floor) and both are inside the 1e-5 bar."""
    import torch.nn as nn
    from glass_amd import _lib, ops
    lib = _lib.load()
    gen = torch.Generator().manual_seed(3 * H + N)
    K = 2 * H if comb else H
    act = 0 if comb else 1
    zr = 0.8
    W = torch.randn(2 * H, K, generator=gen) / K**0.5
    b = torch.randn(2 * H, generator=gen) * 0.1
    xa_h, xb_h = torch.randn(N, H, generator=gen), torch.randn(N, H, generator=gen)
    mask = torch.rand(N, generator=gen) < 0.02
    gout = torch.randn(N, H, generator=gen)
    xa64, xb64 = xa_h.double().requires_grad_(True), xb_h.double().requires_grad_(True)
    W64, b64 = W.double().requires_grad_(True), b.double().requires_grad_(True)
    Z = (torch.cat((xa64, xb64), -1) if comb else xa64) @ W64.t() + b64
    A = torch.nn.functional.elu(Z) if act else Z
    ref = O._mix(mask.reshape(-1, 1), zr, A[:, :H], A[:, H:])
    ref.backward(gout.double())
    want = [ref.detach(), xa64.grad] + ([xb64.grad] if comb else []) + [W64.grad, b64.grad]
    prev = ops.DENSE_F32_PRODUCTS
    errs = {}
    try:
        for form in (0, 1):
            ops.DENSE_F32_PRODUCTS = form == 0  # an option of every dense CALL (act word), not library state
            Wg, bg = W.to(DEV), b.to(DEV)
            dW, db = torch.zeros_like(Wg), torch.zeros_like(bg)
            Wimg, WTimg = _pack(Wg, False, H, zr), _pack(Wg, True, H, zr)
            lin1, lin0 = nn.Linear(K, H).to(DEV), nn.Linear(K, H).to(DEV)
            lin1.weight.grad, lin0.weight.grad, lin1.bias.grad, lin0.bias.grad = dW[:H], dW[H:], db[:H], db[H:]
            xa = xa_h.to(DEV).requires_grad_(True)
            xb = xb_h.to(DEV).requires_grad_(True) if comb else None
            out = ops.dual_linear_mix(xa, xb, lin1, lin0, mask.to(DEV).to(torch.uint8), zr, act, (Wg, bg, dW, db, Wimg, WTimg))
            out.backward(gout.to(DEV))
            got = [out.detach().cpu(), xa.grad.cpu()] + ([xb.grad.cpu()] if comb else []) + [dW.cpu(), db.cpu()]
            errs[form] = [rel_inf(g_, w_) for g_, w_ in zip(got, want)]
    finally:
        ops.DENSE_F32_PRODUCTS = prev
    for e0, e1 in zip(errs[0], errs[1]):
        assert e0 < TOL and e1 < TOL, errs
        assert e1 <= 2.0 * e0 + 2e-7, errs


@pytest.mark.parametrize("H,N,comb", [(256, 70001, False), (256, 70001, True), (128, 50003, False)])
def test_tiled_split_kernels_repeat_bitwise(H, N, comb):
    """Race screen of the LDS-DMA weight operand (dense_tiled.hip: global_load_lds copies retired by vmcnt(0) + a barrier before
    the stage is read, re-staged one barrier after its last read): forward + backward of a tiled pair 60 times on the same
    inputs, every output bit-identical to the first run."""
    import torch.nn as nn
    from glass_amd import _lib, ops
    if ops.DENSE_F32_PRODUCTS:
        pytest.skip("split product form switched off")
    gen = torch.Generator().manual_seed(11 + H + N)
    K = 2 * H if comb else H
    act = 0 if comb else 1
    zr = 0.8
    Wg = (torch.randn(2 * H, K, generator=gen) / K**0.5).to(DEV)
    bg = (torch.randn(2 * H, generator=gen) * 0.1).to(DEV)
    xa_h, xb_h = torch.randn(N, H, generator=gen).to(DEV), torch.randn(N, H, generator=gen).to(DEV)
    mask = (torch.rand(N, generator=gen) < 0.02).to(DEV).to(torch.uint8)
    gout = torch.randn(N, H, generator=gen).to(DEV)
    Wimg, WTimg = _pack(Wg, False, H, zr), _pack(Wg, True, H, zr)
    first = None
    for it in range(60):
        dW, db = torch.zeros_like(Wg), torch.zeros_like(bg)
        lin1, lin0 = nn.Linear(K, H).to(DEV), nn.Linear(K, H).to(DEV)
        lin1.weight.grad, lin0.weight.grad, lin1.bias.grad, lin0.bias.grad = dW[:H], dW[H:], db[:H], db[H:]
        xa = xa_h.clone().requires_grad_(True)
        xb = xb_h.clone().requires_grad_(True) if comb else None
        out = ops.dual_linear_mix(xa, xb, lin1, lin0, mask, zr, act, (Wg, bg, dW, db, Wimg, WTimg))
        out.backward(gout)
        got = [out.detach(), xa.grad] + ([xb.grad] if comb else []) + [dW, db]
        if first is None:
            first = [g.clone() for g in got]
        else:
            for a, b in zip(got, first):
                assert torch.equal(a, b), f"run {it} differs from run 0"


def _pack(W, transposed, H=64, z=None):
    """glass_dense_pack_batch_f32 on one matrix: operand image of W ([NT][KT]) or of W^T, in the layout the fused dense
    kernels of hidden size H read.  z = the pair's z_ratio: the layout the KERNELS read for this operand (the library's
    glass_dual_linear_{fwd,dgrad}_layout, incl. the effective-weight appendix of the comb pair); z = None: the base
    layout without an appendix (forward paired, data-gradient plain / split), as the layout tests address it."""
    from glass_amd import _lib
    lib = _lib.load()
    nt, kt = (W.shape[1], W.shape[0]) if transposed else W.shape
    if lib.glass_dual_linear_layout(H) != 1:
        # wave16 family: the forward operand of the trans pair has its own column order (layout 9) — ask the library
        layout = 0 if z is None else (lib.glass_dual_linear_dgrad_layout(H, nt) if transposed else
                                      lib.glass_dual_linear_fwd_layout(H, kt))
    elif z is not None:
        layout = lib.glass_dual_linear_dgrad_layout(H, nt) if transposed else lib.glass_dual_linear_fwd_layout(H, kt)
    else:
        layout = (2 if nt % 256 == 0 else 3) if transposed else 1
    img = torch.empty(int(lib.glass_dense_image_floats(nt, kt, int(transposed) | (layout << 1))), device=DEV)
    src, dst = np.array([W.data_ptr()], dtype=np.uint64), np.array([img.data_ptr()], dtype=np.uint64)
    nts, kts = np.array([nt], dtype=np.int64), np.array([kt], dtype=np.int64)  # keep the host arrays alive
    trs = np.array([int(transposed) | (layout << 1)], dtype=np.int32)
    zs = np.array([0.0 if z is None else z], dtype=np.float32)
    caps = np.array([img.numel()], dtype=np.int64)
    rc = lib.glass_dense_pack_batch_f32(src.ctypes.data, dst.ctypes.data, caps.ctypes.data, nts.ctypes.data, kts.ctypes.data,
                                        trs.ctypes.data, zs.ctypes.data, 1, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return img


def test_dense_pack_is_a_permutation():
    """The packed image holds exactly the elements of the operand, in the documented fragment order (wave16 layout: hidden 64)."""
    W = torch.arange(128 * 64, dtype=torch.float32, device=DEV).reshape(128, 64)
    for transposed in (False, True):
        img = _pack(W, transposed, 64).cpu()
        assert sorted(img.tolist()) == W.reshape(-1).cpu().tolist()
        B = (W.t() if transposed else W).cpu()  # logical operand [NT][KT]
        NT, KT = B.shape
        KQ = KT // 4
        for (kc, t, v, lane) in ((0, 0, 0, 0), (0, min(5, NT // 16 - 1), 3, 37), (KQ // 16 - 1, NT // 16 - 1, 2, 63)):
            j, q = lane & 15, lane >> 4
            n, k = 64 * (t >> 2) + 4 * j + (t & 3), q * KQ + kc * 16 + 4 * v
            off = (((kc * (NT // 16) + t) * 4 + v) * 64 + lane) * 4
            assert img[off:off + 4].tolist() == B[n, k:k + 4].tolist()


def test_dense_pack_tiled_layouts():
    """Operand images of the LDS-tiled kernels (hidden 256): a permutation of the operand, element order as documented
    in dense_common.h::tiled_col — image[((ct*NKS + ks)*4 + q)*256 + nl] = B[col(ct, nl)][16 ks + 4 q .. +3]."""
    for H in (256, 128):
        W = torch.arange(2 * H * H, dtype=torch.float32, device=DEV).reshape(2 * H, H)  # trans pair weight [2H][H]
        for transposed in (False, True):
            full = _pack(W, transposed, H).cpu()
            img = full[:W.numel()]  # the fp32 image; behind it the same image cut into bf16 pieces (checked below)
            assert sorted(img.tolist()) == W.reshape(-1).cpu().tolist()
            B = (W.t() if transposed else W).cpu()
            NT, KT = B.shape
            _check_cut_image(full, W.numel())
            if transposed and H == 128:
                # split layout: ONE 256-slot tile over K = KT / 2 holds both stacked halves side by side —
                # slot v = wn*128 + 4j + cb: v < 128 -> B[v][k], else B[v - 128][KT/2 + k]
                for (ks, q, nl) in ((0, 0, 0), (KT // 32 - 1, 3, 255), (3, 2, 97), (5, 1, 200)):
                    wn, cb, j = nl >> 7, (nl >> 5) & 3, nl & 31
                    v = wn * 128 + 4 * j + cb
                    k = (v // NT) * (KT // 2) + 16 * ks + 4 * q
                    off = (((ks * 4 + q) * 256) + nl) * 4
                    assert img[off:off + 4].tolist() == B[v % NT, k:k + 4].tolist()
                continue
            NKS = KT // 16
            for (ct, ks, q, nl) in ((0, 0, 0, 0), (NT // 256 - 1, NKS - 1, 3, 255), (0, 3, 2, 97), (NT // 256 - 1, 5, 1, 200)):
                wn, cb, j = nl >> 7, (nl >> 5) & 3, nl & 31
                if not transposed:  # paired: cb 0,1 -> f1 columns 2j + cb ; cb 2,3 -> the same columns of the f0 half
                    c = ct * 128 + wn * 64 + 2 * j + (cb & 1)
                    n = H + c if cb >= 2 else c
                else:               # plain: four consecutive columns per lane
                    n = ct * 256 + wn * 128 + 4 * j + cb
                off = ((((ct * NKS + ks) * 4 + q) * 256) + nl) * 4
                assert img[off:off + 4].tolist() == B[n, 16 * ks + 4 * q:16 * ks + 4 * q + 4].tolist()


def _check_cut_image(full, n_fp32):
    """The cut image behind a tiled fp32 image (glass_dense_image_floats; written in either product form): per tile of 16 k x 256
    slots [piece 3][h 2][slot 256] x 8 bf16 — the three pieces of element (slot, k = 8h + t) sum to the fp32 element exactly."""
    assert full.numel() == n_fp32 * 5 // 2
    fp = full[:n_fp32].reshape(-1, 4, 256, 4)                     # [tile][k-quad][slot][4 k]
    cut = full[n_fp32:].contiguous().view(torch.int16).reshape(-1, 3, 2, 256, 8)  # [tile][piece][h][slot][8 k]
    pieces = (cut.to(torch.int32) << 16).view(torch.float32)     # bf16 -> fp32
    total = pieces[:, 0].double() + pieces[:, 1].double() + pieces[:, 2].double()   # [tile][h][slot][8]
    want = fp.reshape(-1, 2, 2, 256, 4).permute(0, 1, 3, 2, 4).reshape(-1, 2, 256, 8).double()  # k-quads 2h, 2h+1 side by side
    assert torch.equal(total, want)


def test_dense_pack_effective_weight_appendix():
    """Layout 4 (comb pair's data-gradient operand at hidden 256 / 512): the plain image, then the effective weight of
    unlabeled rows (1 - z) * B[:, :KT/2] + z * B[:, KT/2:] in the same tiling over K = KT / 2."""
    from glass_amd import _lib
    H, z = 256, 0.9
    assert _lib.load().glass_dual_linear_dgrad_layout(H, 2 * H) == 4 and _lib.load().glass_dual_linear_dgrad_layout(H, H) == 2
    assert _lib.load().glass_dual_linear_dgrad_layout(128, 128) in (3, 9) and _lib.load().glass_dual_linear_dgrad_layout(64, 64) in (0, 9)
    assert _lib.load().glass_dual_linear_dgrad_layout(128, 256) in (4, 10)  # (10: the stage-run comb data gradient of hidden 128, two effective-weight images)
    gen = torch.Generator().manual_seed(3)
    W = torch.randn(2 * H, 2 * H, generator=gen).to(DEV)  # comb weight [2H out][2H in]; operand B = W^T: [NT = 2H in][KT = 2H out]
    img = torch.empty(int(_lib.load().glass_dense_image_floats(2 * H, 2 * H, 1 | (4 << 1))), device=DEV)
    src, dst = np.array([W.data_ptr()], dtype=np.uint64), np.array([img.data_ptr()], dtype=np.uint64)
    nts, kts = np.array([2 * H], dtype=np.int64), np.array([2 * H], dtype=np.int64)
    trs, zs = np.array([1 | (4 << 1)], dtype=np.int32), np.array([z], dtype=np.float32)
    caps = np.array([img.numel()], dtype=np.int64)
    rc = _lib.load().glass_dense_pack_batch_f32(src.ctypes.data, dst.ctypes.data, caps.ctypes.data, nts.ctypes.data, kts.ctypes.data,
                                                trs.ctypes.data, zs.ctypes.data, 1, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(img[:W.numel()], _pack(W, True, H)[:W.numel()])  # the plain part is layout 2
    _check_cut_image(img.cpu(), W.numel() * 3 // 2)  # (the cut image covers the appendix too)
    B = W.t().cpu()
    Beff = ((1 - np.float32(z)) * B[:, :H] + np.float32(z) * B[:, H:])
    app = img[W.numel():W.numel() * 3 // 2].cpu()
    NT, K2 = 2 * H, H
    NKS = K2 // 16
    for (ct, ks, q, nl) in ((0, 0, 0, 0), (NT // 256 - 1, NKS - 1, 3, 255), (0, 3, 2, 97), (1, 5, 1, 200)):
        wn, cb, j = nl >> 7, (nl >> 5) & 3, nl & 31
        n = ct * 256 + wn * 128 + 4 * j + cb
        off = ((((ct * NKS + ks) * 4 + q) * 256) + nl) * 4
        assert torch.allclose(app[off:off + 4], Beff[n, 16 * ks + 4 * q:16 * ks + 4 * q + 4], rtol=0, atol=1e-6)


def test_dense_pack_forward_effective_weight_appendix():
    """Layout 5 (comb pair's forward operand at hidden 256 / 512): the paired image, then W_unl = (1 - z) * W[:H] + z * W[H:]
    ([H][2H]) in the plain tiling (256 output columns per column tile)."""
    from glass_amd import _lib
    H, z = 256, 0.85
    assert _lib.load().glass_dual_linear_fwd_layout(H, 2 * H) == 5 and _lib.load().glass_dual_linear_fwd_layout(H, H) == 1
    assert _lib.load().glass_dual_linear_fwd_layout(128, 256) == 1 and _lib.load().glass_dual_linear_fwd_layout(64, 128) == 0
    gen = torch.Generator().manual_seed(4)
    W = torch.randn(2 * H, 2 * H, generator=gen).to(DEV)  # comb weight [2H out][2H in] = the operand B itself
    img = torch.empty(int(_lib.load().glass_dense_image_floats(2 * H, 2 * H, 0 | (5 << 1))), device=DEV)
    src, dst = np.array([W.data_ptr()], dtype=np.uint64), np.array([img.data_ptr()], dtype=np.uint64)
    nts, kts = np.array([2 * H], dtype=np.int64), np.array([2 * H], dtype=np.int64)
    trs, zs = np.array([0 | (5 << 1)], dtype=np.int32), np.array([z], dtype=np.float32)
    caps = np.array([img.numel()], dtype=np.int64)
    rc = _lib.load().glass_dense_pack_batch_f32(src.ctypes.data, dst.ctypes.data, caps.ctypes.data, nts.ctypes.data, kts.ctypes.data,
                                                trs.ctypes.data, zs.ctypes.data, 1, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert torch.equal(img[:W.numel()], _pack(W, False, H)[:W.numel()])  # the first part is the paired layout
    _check_cut_image(img.cpu(), W.numel() * 3 // 2)
    Wc = W.cpu()
    Weff = (1 - np.float32(z)) * Wc[:H] + np.float32(z) * Wc[H:]
    app = img[W.numel():W.numel() * 3 // 2].cpu()
    NKS = 2 * H // 16
    for (ct, ks, q, nl) in ((0, 0, 0, 0), (H // 256 - 1, NKS - 1, 3, 255), (0, 3, 2, 97), (0, 17, 1, 200)):
        wn, cb, j = nl >> 7, (nl >> 5) & 3, nl & 31
        n = ct * 256 + wn * 128 + 4 * j + cb
        off = ((((ct * NKS + ks) * 4 + q) * 256) + nl) * 4
        assert torch.allclose(app[off:off + 4], Weff[n, 16 * ks + 4 * q:16 * ks + 4 * q + 4], rtol=0, atol=1e-6)


@pytest.mark.parametrize("N", [16400, 50003, 70001])
def test_trans_dgrad_hidden128_stage_split(N):
    """Trans pair's data gradient at hidden 128 on a graph of more than 256 row tiles (trans_dgrad3_kernel: workgroups take
    runs of 16-row STAGES — 13 of them at N = 50 003, the last workgroup a shorter run, an odd count —): out = (mix'(dout) .
    ELU'(T)) @ Wstack + addend against fp64, and the backward-GraphNorm column sums of its epilogue — one partials entry per
    WORKGROUP, the remaining per-tile entries zeroed by the kernel (the buffer is handed over full of NaNs) — against fp64
    sums; twice -> identical bits."""
    from glass_amd import stack
    from glass_amd.arena import ParamArena
    from glass_amd.factory import build_glass
    torch.manual_seed(N)
    H, z = 128, 0.8
    model = build_glass(H, 1, 5, 3, "mean", "sum", z).to(DEV).train()
    ParamArena(model)
    st = model.conv.convs[0]._stack["trans"]
    gmod = model.conv.convs[0].gn
    mask = (torch.rand(N, device=DEV) < 0.1).to(torch.uint8)
    mask[-1] = 1
    dsrc, T = torch.randn(N, H, device=DEV), torch.randn(N, 2 * H, device=DEV)
    addend, gx = torch.randn(N, H, device=DEV), torch.randn(N, H, device=DEV)
    saved = torch.cat([gx.mean(0), 1.0 / (gx.var(0, unbiased=False) + 1e-5).sqrt(), torch.ones(H, device=DEV),
                       torch.zeros(H, device=DEV)]).contiguous()
    nblk = -(-N // int(stack._lib.load().glass_dual_linear_stat_rows(H)))
    W = st[0].double()
    lab = mask.bool().unsqueeze(1)
    w1 = torch.where(lab, torch.tensor(z, device=DEV, dtype=torch.float64), torch.tensor(1 - z, device=DEV, dtype=torch.float64))
    elu_g = lambda t: torch.where(t > 0, torch.ones_like(t), torch.exp(t))
    d = dsrc.double()
    ref = (w1 * d * elu_g(T[:, :H].double())) @ W[:H] + ((1 - w1) * d * elu_g(T[:, H:].double())) @ W[H:] + addend.double()
    xhat = (gx.double() - gmod.mean_scale.double() * saved[:H].double()) * saved[H:2 * H].double()
    from glass_amd import ops
    prev = ops.DENSE_F32_PRODUCTS
    try:
        for form in (False, True):   # six bf16 partial products (default) / the f32-input MFMA
            ops.DENSE_F32_PRODUCTS = form
            got = []
            for _ in range(2):
                out = torch.full((N, H), float("nan"), device=DEV)
                gpart = torch.full((nblk, 2, H), float("nan"), dtype=torch.float64, device=DEV)
                stack._dual_dgrad(dsrc, T, st, mask, z, 1, H, addend, out, gn=(gpart, gx, saved, gmod.mean_scale, 0, 0.0, 0))
                got.append((out, gpart))
            out, gpart = got[0]
            e_out = rel_inf(out.double(), ref)
            e_s1, e_s2 = rel_inf(gpart[:, 0].sum(0), ref.sum(0)), rel_inf(gpart[:, 1].sum(0), (ref * xhat).sum(0))
            assert e_out < TOL and e_s1 < TOL and e_s2 < TOL, (form, e_out, e_s1, e_s2)
            assert torch.equal(got[1][0], out) and torch.equal(got[1][1], gpart)
            if not form:
                record_parity(f"kernel/trans_dgrad128_stage_split_N{N}", out_rel_inf=e_out, gn_sum_rel_inf=max(e_s1, e_s2))
    finally:
        ops.DENSE_F32_PRODUCTS = prev


@pytest.mark.parametrize("N,gather,p_drop", [(50003, False, 0.0), (50003, True, 0.5), (1000, True, 0.0), (63, False, 0.5), (17080, False, 0.0)])
def test_trans_fwd_hidden128_stage_run(N, gather, p_drop):
    """Trans pair's forward at hidden 128 (trans_fwd3_kernel): GraphNorm prologue (scale / shift from `saved`, ELU, dropout) in the
    loader with the normalised operand as side output, the operand rows optionally gathered from a 37-row table (layer 0),
    T = h W^T + b, out = label mix of ELU(T), and the column sums of `out` — one entry per WORKGROUP, the rest of the 64-row
    entries zeroed by the kernel (NaN prefill).  fp64 reference built on the kernel's own side output (so the dropout mask is
    the kernel's), the side output itself against the formula where nothing is dropped; both product forms; twice -> bits."""
    from glass_amd import ops, stack
    from glass_amd.arena import ParamArena
    from glass_amd.factory import build_glass
    torch.manual_seed(N + int(gather))
    H, z = 128, 0.8
    model = build_glass(H, 1, 5, 3, "mean", "sum", z).to(DEV).train()
    ParamArena(model)
    st = model.conv.convs[0]._stack["trans"]
    W, b = st[0].double(), st[1].double()
    mask = (torch.rand(N, device=DEV) < 0.1).to(torch.uint8)
    mask[-1] = 1
    V = 37
    src = torch.randn(V if gather else N, H, device=DEV)
    idx = torch.randint(0, V, (N,), device=DEV, dtype=torch.int64) if gather else None
    scale, shift = torch.rand(H, device=DEV) + 0.5, torch.randn(H, device=DEV) * 0.1
    saved = torch.cat([torch.zeros(H, device=DEV), torch.ones(H, device=DEV), scale, shift]).contiguous()
    nblk = -(-N // int(stack._lib.load().glass_dual_linear_stat_rows(H)))
    rows = src[idx] if gather else src
    h_formula = torch.nn.functional.elu(rows.double() * scale.double() + shift.double())
    lab = mask.bool().unsqueeze(1)
    prev = ops.DENSE_F32_PRODUCTS
    try:
        for form in (False, True):
            ops.DENSE_F32_PRODUCTS = form
            got = []
            for _ in range(2):
                T = torch.full((N, 2 * H), float("nan"), device=DEV)
                out = torch.full((N, H), float("nan"), device=DEV)
                side = torch.full((N, H), float("nan"), device=DEV)
                cstat = torch.full((nblk, 2, H), float("nan"), dtype=torch.float64, device=DEV)
                stack._dual_fwd(src, None, st, mask, z, 1, T, out, cstat, gn=(saved, 1, p_drop, 3, side), xa_index=idx)
                got.append((T, out, side, cstat))
            T, out, side, cstat = got[0]
            if p_drop == 0.0:
                assert rel_inf(side.double(), h_formula) < TOL
            else:   # kept elements scaled by 1 / (1 - p), about half of them dropped
                kept = side != 0
                assert 0.4 < float(kept.float().mean()) < 0.6
                assert rel_inf(side.double()[kept], (h_formula / (1 - p_drop))[kept]) < TOL
            Tref = side.double() @ W.t() + b
            A = torch.nn.functional.elu(Tref)
            oref = torch.where(lab, z * A[:, :H] + (1 - z) * A[:, H:], (1 - z) * A[:, :H] + z * A[:, H:])
            e_T, e_o = rel_inf(T.double(), Tref), rel_inf(out.double(), oref)
            e_s, e_q = rel_inf(cstat[:, 0].sum(0), oref.sum(0)), rel_inf(cstat[:, 1].sum(0), (oref * oref).sum(0))
            assert max(e_T, e_o, e_s, e_q) < TOL, (form, e_T, e_o, e_s, e_q)
            for a, b2 in zip(got[0], got[1]):
                assert torch.equal(a, b2)
            if not form:
                record_parity(f"kernel/trans_fwd128_stage_run_N{N}_gather{int(gather)}_p{p_drop}", T_rel_inf=e_T, out_rel_inf=e_o,
                              stats_rel_inf=max(e_s, e_q))
    finally:
        ops.DENSE_F32_PRODUCTS = prev


@pytest.mark.parametrize("N,labeled", [(50003, "few"), (50003, "none"), (5000, "all"), (63, "few"), (17080, "dense"), (1100000, "few")])
def test_comb_dgrad_hidden128_stage_run(N, labeled):
    """Comb pair's data gradient at hidden 128 (comb_dgrad3_kernel: a workgroup walks its rows with the UNLABELED effective
    weight, lists its labeled rows and redoes those with the LABELED one): d[g || x_] = [w1 dc | w0 dc] @ Wstack against fp64
    for a batch-like label density, no labeled row, every row labeled (the second pass as long as the first), a graph
    smaller than one workgroup, a third of the rows, and more than 256 x 4096 rows (the list cap bounds the rows per
    workgroup); the backward-GraphNorm column sums of the first 128 columns — one entry per workgroup, the rest zeroed (NaN
    prefill) — against fp64; both product forms; twice -> identical bits."""
    from glass_amd import ops, stack
    from glass_amd.arena import ParamArena
    from glass_amd.factory import build_glass
    torch.manual_seed(N + len(labeled))
    H, z = 128, 0.8
    model = build_glass(H, 1, 5, 3, "mean", "sum", z).to(DEV).train()
    ParamArena(model)
    st = model.conv.convs[0]._stack["comb"]
    gmod = model.conv.convs[0].gn
    mask = {"few": torch.rand(N, device=DEV) < 0.02, "none": torch.zeros(N, dtype=torch.bool, device=DEV),
            "all": torch.ones(N, dtype=torch.bool, device=DEV), "dense": torch.rand(N, device=DEV) < 0.33}[labeled].to(torch.uint8)
    if labeled == "few":
        mask[-1] = 1
        mask[0] = 1
    dc, gx = torch.randn(N, H, device=DEV), torch.randn(N, H, device=DEV)
    saved = torch.cat([gx.mean(0), 1.0 / (gx.var(0, unbiased=False) + 1e-5).sqrt(), torch.ones(H, device=DEV),
                       torch.zeros(H, device=DEV)]).contiguous()
    nblk = -(-N // int(stack._lib.load().glass_dual_linear_stat_rows(H)))
    W = st[0].double()
    lab = mask.bool().unsqueeze(1)
    w1 = torch.where(lab, torch.tensor(z, device=DEV, dtype=torch.float64), torch.tensor(1 - z, device=DEV, dtype=torch.float64))
    ref = (w1 * dc.double()) @ W[:H] + ((1 - w1) * dc.double()) @ W[H:]
    g = ref[:, :H]
    xhat = (gx.double() - gmod.mean_scale.double() * saved[:H].double()) * saved[H:2 * H].double()
    prev = ops.DENSE_F32_PRODUCTS
    try:
        for form in (False, True):
            ops.DENSE_F32_PRODUCTS = form
            got = []
            for _ in range(2):
                din = torch.full((N, 2 * H), float("nan"), device=DEV)
                gpart = torch.full((nblk, 2, H), float("nan"), dtype=torch.float64, device=DEV)
                stack._dual_dgrad(dc, None, st, mask, z, 0, 2 * H, None, din, gn=(gpart, gx, saved, gmod.mean_scale, 0, 0.0, 0))
                got.append((din, gpart))
            din, gpart = got[0]
            e_out = rel_inf(din.double(), ref)
            e_s1, e_s2 = rel_inf(gpart[:, 0].sum(0), g.sum(0)), rel_inf(gpart[:, 1].sum(0), (g * xhat).sum(0))
            assert e_out < TOL and e_s1 < TOL and e_s2 < TOL, (form, e_out, e_s1, e_s2)
            assert torch.equal(got[1][0], din) and torch.equal(got[1][1], gpart)
            # without the statistics epilogue: the same gradient
            din2 = torch.full((N, 2 * H), float("nan"), device=DEV)
            stack._dual_dgrad(dc, None, st, mask, z, 0, 2 * H, None, din2)
            assert torch.equal(din2, din)
            if not form:
                record_parity(f"kernel/comb_dgrad128_stage_run_N{N}_{labeled}", out_rel_inf=e_out, gn_sum_rel_inf=max(e_s1, e_s2))
    finally:
        ops.DENSE_F32_PRODUCTS = prev


@pytest.mark.parametrize("pattern", ["none", "one_per_tile_3", "sparse", "cap3", "cap4", "cap7", "cap8", "all"])
def test_comb_pair_effective_weight_paths(pattern):
    """Comb pair at hidden 256 on the tiled kernels: the effective-weight (one product) and two-product paths — forward
    (+ statistics) and data gradient (one product for every tile with few labeled rows, those rows corrected
    afterwards) against fp64, for label patterns that exercise the paths side by side inside one launch."""
    from glass_amd import stack
    from glass_amd.arena import ParamArena
    from glass_amd.factory import build_glass
    torch.manual_seed(7)
    N, H, z = 1000, 256, 0.9   # 8 row tiles of 128 (the last one ragged)
    model = build_glass(H, 1, 5, 3, "mean", "sum", z).to(DEV).train()
    ParamArena(model)
    st = model.conv.convs[0]._stack["comb"]
    mask = torch.zeros(N, dtype=torch.uint8, device=DEV)
    if pattern == "one_per_tile_3":
        mask[3 * 128 + 17] = 1
    elif pattern == "sparse":
        mask[torch.tensor([5, 300, 301, 999], device=DEV)] = 1
    elif pattern.startswith("cap"):   # at / just past the most labeled rows a single-product tile corrects afterwards
        k = int(pattern[3:])          # (3 in the forward, 7 in the data gradient; one more falls back to two products)
        mask[2 * 128 + torch.arange(k, device=DEV) * 17 + 5] = 1
    elif pattern == "all":
        mask[:] = 1
    a, h = torch.randn(N, H, device=DEV), torch.randn(N, H, device=DEV)
    c = torch.empty(N, H, device=DEV)
    nblk = -(-N // int(stack._lib.load().glass_dual_linear_stat_rows(H)))
    cstat = torch.empty(nblk, 2, H, dtype=torch.float64, device=DEV)
    stack._dual_fwd(a, h, st, mask, z, 0, None, c, cstat)
    W, b = st[0].double(), st[1].double()
    x = torch.cat([a, h], 1).double()
    C1, C0 = x @ W[:H].t() + b[:H], x @ W[H:].t() + b[H:]
    lab = mask.bool().unsqueeze(1)
    ref = torch.where(lab, z * C1 + (1 - z) * C0, (1 - z) * C1 + z * C0)
    assert rel_inf(c.double(), ref) < 1e-5
    assert rel_inf(cstat[:, 0].sum(0), ref.sum(0)) < 1e-5 and rel_inf(cstat[:, 1].sum(0), (ref * ref).sum(0)) < 1e-5
    # data gradient: dIN = [w1 dc | w0 dc] @ Wstack
    dc = torch.randn(N, H, device=DEV)
    din = torch.empty(N, 2 * H, device=DEV)
    stack._dual_dgrad(dc, None, st, mask, z, 0, 2 * H, None, din)
    w1 = torch.where(lab, torch.tensor(z, device=DEV, dtype=torch.float64), torch.tensor(1 - z, device=DEV, dtype=torch.float64))
    dref = (w1 * dc.double()) @ W[:H] + ((1 - w1) * dc.double()) @ W[H:]
    assert rel_inf(din.double(), dref) < 1e-5
    # the same launch with the backward-GraphNorm column sums in its epilogue (the LDS reduction of those sums reuses the
    # memory the labeled-row corrections are read from)
    gmod = model.conv.convs[0].gn
    gx = torch.randn(N, H, device=DEV)
    saved = torch.cat([gx.mean(0), 1.0 / (gx.var(0, unbiased=False) + 1e-5).sqrt(), torch.ones(H, device=DEV),
                       torch.zeros(H, device=DEV)]).contiguous()
    gpart = torch.empty(nblk, 2, H, dtype=torch.float64, device=DEV)
    din2 = torch.empty_like(din)
    stack._dual_dgrad(dc, None, st, mask, z, 0, 2 * H, None, din2, gn=(gpart, gx, saved, gmod.mean_scale, 0, 0.0, 0))
    assert torch.equal(din2, din)
    g = dref[:, :H]
    xhat = (gx.double() - gmod.mean_scale.double() * saved[:H].double()) * saved[H:2 * H].double()
    assert rel_inf(gpart[:, 0].sum(0), g.sum(0)) < 1e-5 and rel_inf(gpart[:, 1].sum(0), (g * xhat).sum(0)) < 1e-5


# ---------------------------------------------------------------------------------- K8 head + loss
@pytest.mark.parametrize("mode,B,C,K", [(0, 80, 128, 6), (0, 7, 17, 3), (1, 99, 128, 10), (1, 5, 64, 1)])
def test_head_loss_fused(mode, B, C, K):
    """Linear head + CrossEntropy / BCE-with-logits fused (2 launches) vs torch in fp64."""
    import torch.nn as nn
    from glass_amd import losses
    gen = torch.Generator().manual_seed(B + K)
    pooled = torch.randn(B, C, generator=gen)
    lin = nn.Linear(C, K)
    y = torch.randint(0, K, (B, ), generator=gen) if mode == 0 else (torch.rand(B, K, generator=gen) < 0.4).float()
    p64 = pooled.double().requires_grad_(True)
    l64 = nn.Linear(C, K).double()
    l64.load_state_dict({k: v.double() for k, v in lin.state_dict().items()})
    z = l64(p64)
    ref = nn.functional.cross_entropy(z, y) if mode == 0 else nn.functional.binary_cross_entropy_with_logits(
        z.flatten(), y.double().flatten())
    (ref * 1.7).backward()
    ling = nn.Linear(C, K).to(DEV)
    ling.load_state_dict(lin.state_dict())
    pg = pooled.to(DEV).requires_grad_(True)
    loss, logits = losses.head_loss(pg, ling, y.to(DEV), mode)
    (loss * 1.7).backward()
    assert abs(loss.item() - ref.item()) < TOL * abs(ref.item())
    assert rel_inf(logits.cpu(), z.detach()) < TOL
    assert rel_inf(pg.grad.cpu(), p64.grad) < TOL
    assert rel_inf(ling.weight.grad.cpu(), l64.weight.grad) < TOL
    assert rel_inf(ling.bias.grad.cpu(), l64.bias.grad) < TOL
    # the marker modules are ordinary losses too
    m = losses.CrossEntropy() if mode == 0 else losses.BCEWithLogits()
    assert abs(m(logits, y.to(DEV)).item() - ref.item()) < TOL * abs(ref.item())


# ---------------------------------------------------------------------------------- degenerate inputs
def test_spmm_graph_without_edges_and_single_node():
    from glass_amd.graph import CSRAdj
    ei = torch.zeros((2, 0), dtype=torch.int64, device=DEV)
    adj = CSRAdj(ei, torch.zeros(0, device=DEV), 7, "mean")
    y = adj.fwd.spmm(torch.randn(7, 64, device=DEV))
    assert y.shape == (7, 64) and float(y.abs().max()) == 0.0
    assert float(adj.deg.min()) == 1.0  # isolated rows get degree 1 (models.py:93-94)
    one = CSRAdj(torch.tensor([[0], [0]], device=DEV), torch.tensor([2.0], device=DEV), 1, "gcn")  # one self-loop
    x = torch.randn(1, 8, device=DEV)
    assert rel_inf(one.fwd.spmm(x).cpu(), x.cpu()) < 1e-6  # 2 / sqrt(2) / sqrt(2) = 1


def test_model_on_degenerate_batches():
    """B = 1, Smax = 1, an all-padding subgraph row, a graph with isolated nodes only around the batch."""
    from helpers import build_glass
    from impl import utils
    from glass_amd import synth
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=5, n_batches=1)
    ei, ew, x = (torch.from_numpy(a).to(DEV) for a in (ei, ew, x))
    torch.manual_seed(0)
    model = build_glass(16, 2, int(x.max()), 3, "gcn", "mean", 0.75).to(DEV).train()
    for p in (torch.tensor([[5]]), torch.tensor([[5, -1, -1], [-1, -1, -1]]), torch.tensor([[0, 1, 2, 3]])):
        p = p.to(DEV)
        out = model(x, ei, ew, p, utils.MaxZOZ(x, p))
        assert out.shape == (p.shape[0], 3) and bool(torch.isfinite(out).all())
        out.sum().backward()
    assert all(bool(torch.isfinite(q.grad).all()) for q in model.parameters())


@pytest.mark.parametrize("shape", ["em_user", "powerlaw"])
def test_spmm_full_size_properties(shape):
    """BASELINE-size graphs (C4: N=50 000 / nnz=1 M; C5: N=1 M / nnz=20 M power-law with 50 000-edge hubs), too big
    for the CPU oracle in a test: size-independent properties instead.
      linearity        A(ax + by) = a Ax + b Ay
      row sums         A 1 = 1 on non-isolated rows for aggr=mean (every row of A sums to 1)
      adjointness      <A x, y> = <x, A^T y>: the backward operand really is the transpose of the forward one
      repeatability    bitwise equal across launches (no float atomics, also through the chunked-row path)"""
    from glass_amd import synth
    from glass_amd.graph import CSRAdj
    w = synth.WORKLOADS[shape]
    ei, ew = synth.make_graph(w.n_node, w.n_pairs, 0, w.powerlaw)
    n, H = w.n_node, 32
    adj = CSRAdj(torch.from_numpy(ei).to(DEV), torch.from_numpy(ew).to(DEV), n, "mean")
    assert adj.nnz == 2 * w.n_pairs
    gen = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(n, H, device=DEV, generator=gen)
    y = torch.randn(n, H, device=DEV, generator=gen)
    ax, ay = adj.fwd.spmm(x), adj.fwd.spmm(y)
    lin = adj.fwd.spmm(0.3 * x - 1.7 * y)
    assert rel_inf(lin.cpu(), (0.3 * ax - 1.7 * ay).cpu()) < TOL
    ones = adj.fwd.spmm(torch.ones(n, 4, device=DEV))
    deg = torch.bincount(torch.from_numpy(ei[0]), minlength=n).to(DEV)
    assert rel_inf(ones[deg > 0].cpu(), torch.ones_like(ones[deg > 0]).cpu()) < 1e-5
    assert float(ones[deg == 0].abs().max() if bool((deg == 0).any()) else 0.0) == 0.0
    lhs = (ax.double() * y.double()).sum().item()
    rhs = (x.double() * adj.bwd.spmm(y).double()).sum().item()
    assert abs(lhs - rhs) < 1e-6 * max(abs(lhs), (ax.double().norm() * y.double().norm()).item())
    assert torch.equal(adj.fwd.spmm(x), ax)
    if shape == "powerlaw":
        assert adj.fwd.header[6] > 0 and int(deg.max()) == 50000  # chunked rows present


@pytest.mark.parametrize("H", [8, 64, 128, 17])
def test_spmm_row_parallel_mode_for_short_rows(H):
    """Short rows in the sweep kernel's ROW mode: degrees 0-3 with two long rows (300 edges, which belong to the workgroup
    items and cut the sweep items) mixed in.  The plan holds about 2 500 sweep items, fewer than the 8 192 at which a launch
    takes the flat-capable build (asserted from the header; tests/test_k1_sum_host.py rebuilds this plan on the host), so
    every item runs one row at a time.  Flat mode at a small shape is tests/test_gpu_k1_sum.py::test_flat_build's."""
    from glass_amd.graph import CSRAdj
    rng = np.random.default_rng(H)
    n = 6000
    rows = np.repeat(np.arange(n), rng.integers(0, 4, n))
    cols = rng.integers(0, n, rows.shape[0])
    hub = np.array([17, 3000])
    rows = np.concatenate([rows, np.repeat(hub, 300)])
    cols = np.concatenate([cols, rng.integers(0, n, 600)])
    ei = torch.from_numpy(np.stack([rows, cols]))
    ew = torch.from_numpy(rng.uniform(0.5, 2.0, rows.shape[0]).astype(np.float32))
    x = torch.randn(n, H, generator=torch.Generator().manual_seed(H))
    ref = O.build_adj(ei, ew, n, "sum").to(torch.float64) @ x.double()
    adj = CSRAdj(ei.to(DEV), ew.to(DEV), n, "sum")
    for h in (adj.fwd.header, adj.bwd.header):  # header word 4: sweep items -> the row-only sweep build at every width
        assert 0 < int(h[4]) < 8192
    assert int(adj.fwd.header[5]) == 2 and int(adj.fwd.header[8]) == 64  # the two long rows are workgroup items
    y = adj.fwd.spmm(x.to(DEV))
    assert rel_inf(y.cpu(), ref) < TOL
    assert torch.equal(adj.fwd.spmm(x.to(DEV)), y)
    yt = adj.bwd.spmm(x.to(DEV))
    assert rel_inf(yt.cpu(), O.build_adj(ei, ew, n, "sum").to(torch.float64).t() @ x.double()) < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("H,n", [(64, 1_100_000), (16, 300_000), (128, 300_000), (17, 200_000)])
def test_spmm_row_parallel_wide_threshold_on_large_graphs(H, n):
    """Flat mode (factor 4, header word 13): degrees 0-8 (mean 4 <= 4 * G) on sweeps of >= 8 192 items, where the launch
    takes the flat-capable kernel (header word 15: share of the sweep cost in flat-eligible items); H = 64 at a size
    that also takes the non-temporal index / output streams (n_rows * 260 B + nnz * 8 B > 256 MiB); other widths: G = 16,
    2 and the scalar path.  Checked against a float64 CSR product built with scipy."""
    import scipy.sparse as sp
    from glass_amd.graph import CSRAdj
    rng = np.random.default_rng(5)
    rows = np.repeat(np.arange(n), rng.integers(0, 9, n))
    cols = rng.integers(0, n, rows.shape[0])
    w = rng.uniform(0.5, 2.0, rows.shape[0]).astype(np.float32)
    x = torch.randn(n, H, generator=torch.Generator().manual_seed(5))
    adj = CSRAdj(torch.from_numpy(np.stack([rows, cols])).to(DEV), torch.from_numpy(w).to(DEV), n, "sum")
    assert int(adj.fwd.header[13]) == 4 and int(adj.fwd.header[4]) >= 8192
    g_log2 = {64: 2, 16: 4, 128: 1, 17: 1}[H]  # lane groups per wave: 64 / lanes-per-row
    assert (int(adj.fwd.header[15]) >> (4 * g_log2)) & 15 >= 4  # -> the flat-capable kernel is the one launched
    if H == 64:
        assert n * (4 * H + 4) + rows.shape[0] * 8 > (256 << 20)
    y = adj.fwd.spmm(x.to(DEV))
    ref = sp.csr_matrix((w.astype(np.float64), (rows, cols)), shape=(n, n)) @ x.double().numpy()
    assert rel_inf(y.cpu(), torch.from_numpy(ref)) < TOL
    assert torch.equal(adj.fwd.spmm(x.to(DEV)), y)


# ---------------------------------------------------------------------------------- K3n embedding table path
@pytest.mark.parametrize("H,V,n", [(64, 40, 3000), (17, 3, 500), (128, 1024, 5000), (8, 3, 100)])
def test_embed_norm_table_path(H, V, n):
    """glass_embed_norm_fwd/bwd (lookup + emb_gn through the V-row table) against torch fp64 autograd of
    GraphNorm(Embedding(x)) on the node matrix; some table rows unused (count 0)."""
    from glass_amd import _lib
    from glass_amd.graph import Selection
    lib = _lib.load()
    gen = torch.Generator().manual_seed(H + V)
    x = torch.randint(0, max(V - 1, 1), (n, ), generator=gen)  # last row never used when V > 1
    W = torch.randn(V, H, generator=gen) * 1.5 + 0.7
    gamma, beta, alpha = (1 + 0.3 * torch.randn(H, generator=gen), 0.2 * torch.randn(H, generator=gen),
                          1 + 0.3 * torch.randn(H, generator=gen))
    z = (torch.rand(n, generator=gen) < 0.2).to(torch.int64)
    gout = torch.randn(n, H, generator=gen)
    # reference
    Wd = W.double().requires_grad_(True)
    gn = O.GraphNorm(H).double()
    with torch.no_grad():
        gn.weight.copy_(gamma), gn.bias.copy_(beta), gn.mean_scale.copy_(alpha)
    ref = gn(Wd[x])
    ref.backward(gout.double())
    # HIP
    xg, Wg, zg = x.to(DEV), W.to(DEV), z.to(DEV)
    g, b, a = gamma.to(DEV), beta.to(DEV), alpha.to(DEV)
    sel = Selection(xg, V)
    saved, table = torch.empty(4 * H, device=DEV), torch.empty(V, H, device=DEV)
    out, mask = torch.empty(n, H, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.glass_embed_norm_fwd_f32(xg.data_ptr(), Wg.data_ptr(), V, sel.op.rowptr.data_ptr(), g.data_ptr(), b.data_ptr(),
                                      a.data_ptr(), 1e-5, saved.data_ptr(), table.data_ptr(), zg.data_ptr(), 0, 0, 0.0, 0, 1,
                                      out.data_ptr(), H, mask.data_ptr(), n, H, st)
    assert rc == 0
    assert rel_inf(out.cpu(), ref.detach()) < TOL
    assert torch.equal(mask.cpu().bool(), z > 0)
    G = sel.op.spmm(gout.to(DEV))
    dW = torch.full((V, H), 0.5, device=DEV)       # accumulate_w = 1: adds to what is there
    dg, db, da = (torch.zeros(H, device=DEV) for _ in range(3))
    rc = lib.glass_embed_norm_bwd_f32(G.data_ptr(), Wg.data_ptr(), V, sel.op.rowptr.data_ptr(), g.data_ptr(), a.data_ptr(),
                                      saved.data_ptr(), dW.data_ptr(), 1, dg.data_ptr(), db.data_ptr(), da.data_ptr(), 0, H, st)
    assert rc == 0
    assert rel_inf((dW - 0.5).cpu(), Wd.grad) < TOL
    assert rel_inf(dg.cpu(), gn.weight.grad) < TOL and rel_inf(db.cpu(), gn.bias.grad) < TOL
    assert rel_inf(da.cpu(), gn.mean_scale.grad) < TOL
    if V > 1:
        assert float((dW[V - 1] - 0.5).abs().max()) == 0.0  # unused row: no gradient
    # more rows than the table path takes -> rejected (callers keep the whole-graph kernels)
    assert lib.glass_embed_norm_fwd_f32(xg.data_ptr(), Wg.data_ptr(), _lib.EMBED_NORM_MAX_ROWS + 1, sel.op.rowptr.data_ptr(), g.data_ptr(),
                                        b.data_ptr(), a.data_ptr(), 1e-5, saved.data_ptr(), table.data_ptr(), 0, 0, 0, 0.0,
                                        0, 1, out.data_ptr(), H, mask.data_ptr(), n, H, st) != 0


def test_dgrad_dropout_epilogue_matches_graphnorm_mask():
    """The data-gradient kernel's dropout epilogue draws the same mask as glass_graphnorm_fwd_f32 with the same
    (p, call id): masking there == masking in the GraphNorm backward."""
    from glass_amd import _lib, ops
    from glass_amd.arena import ParamArena
    import torch.nn as nn
    from impl import models
    dev = torch.device(DEV)
    n, H, p, call = 1000, 64, 0.5, 1
    ops.rng_seed(99, dev)
    ones, zeros = torch.ones(H, device=DEV), torch.zeros(H, device=DEV)
    x = torch.randn(n, H, device=DEV)
    kept = ops.graphnorm(x, ones, zeros, ones, p_drop=p, call_id=call) != 0
    conv = models.GLASSConv(H, H, activation=nn.ELU(), aggr="mean", z_ratio=0.9, dropout=0.0).to(DEV)
    ParamArena(conv)
    st = conv._stack["trans"]
    from glass_amd.stack import _dual_dgrad
    mask = (torch.rand(n, device=DEV) < 0.3).to(torch.uint8)
    dsrc, T = torch.randn(n, H, device=DEV), torch.randn(n, 2 * H, device=DEV)
    plain, dropped = torch.empty(n, H, device=DEV), torch.empty(n, H, device=DEV)
    _dual_dgrad(dsrc, T, st, mask, 0.9, 1, H, None, plain)
    _dual_dgrad(dsrc, T, st, mask, 0.9, 1, H, None, dropped, drop=(p, call))
    assert torch.equal(dropped, torch.where(kept, plain / (1 - p), torch.zeros_like(plain)))


def test_copy_pair():
    from glass_amd import _lib
    a = torch.randint(-5, 1000, (80, 11), device=DEV)
    b = torch.rand(80, 6, device=DEV)
    da, db = torch.empty_like(a), torch.full_like(b, -1.0)
    rc = _lib.load().glass_copy_pair(da.data_ptr(), a.data_ptr(), a.numel() * 8, db.data_ptr(), b.data_ptr(), b.numel() * 4,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(da, a) and torch.equal(db, b)
    assert _lib.load().glass_copy_pair(da.data_ptr(), a.data_ptr(), 6, db.data_ptr(), b.data_ptr(), 4,
                                       torch.cuda.current_stream().cuda_stream) != 0  # 4-byte granularity


# ---------------------------------------------------------------------------------- K4b batch labels + comb pair, hidden 64
def _first_occurrence_unique(pos_flat, n):
    seen, rows = set(), []
    for p in pos_flat.tolist():
        if 0 <= p < n and p not in seen:
            seen.add(p)
            rows.append(p)
    return rows


@pytest.mark.parametrize("B,S,n", [(80, 10, 17080), (3, 7, 50), (99, 155, 5000), (1, 1, 9)])
def test_batch_labels(B, S, n):
    """glass_batch_labels: label bytes == utils.MaxZOZ's z (impl/utils.py:32-45), unique labeled rows in first-occurrence
    order, the batch copied into the fixed buffers; three batches through the incremental form (labels of the previous
    batch cleared without a pass over the N bytes) and one through the stand-alone form.  Integer outputs: exact."""
    from glass_amd import stack
    rng = np.random.default_rng(B * 1000 + S)
    labels = stack.BatchLabels(n, B * S, DEV)
    pos_fix = torch.full((B, S), -1, dtype=torch.int64, device=DEV)
    y_fix = torch.zeros(B, dtype=torch.int64, device=DEV)
    for it in range(3):
        pos = rng.integers(0, min(n, max(4, B * S // 2)), (B, S))   # small id range -> many nodes shared by subgraphs
        pos[rng.random((B, S)) < 0.3] = -1                           # padding
        if B * S > 1:
            pos.flat[0] = pos.flat[-1] if pos.flat[-1] >= 0 else 0   # a duplicate at the extreme entries
        y = rng.integers(0, 5, B)
        pos_t, y_t = torch.from_numpy(pos).to(DEV), torch.from_numpy(y).to(DEV)
        labels.load(pos_t, pos_fix, y_t, y_fix)
        z = O.max_zero_one(torch.zeros(n, 1, 1, dtype=torch.int64), torch.from_numpy(pos))
        assert torch.equal(labels.mask.cpu().to(torch.int64), z), it
        rows = _first_occurrence_unique(pos.reshape(-1), n)
        assert int(labels.count[0]) == len(rows)
        assert labels.rows[:len(rows)].cpu().tolist() == rows
        assert torch.equal(pos_fix.cpu(), torch.from_numpy(pos)) and torch.equal(y_fix.cpu(), torch.from_numpy(y))
    solo = stack.BatchLabels(n, B * S, DEV)
    solo.mask.fill_(1)   # the stand-alone form zero-fills the N bytes itself
    solo.load(pos_t)
    assert torch.equal(solo.mask, labels.mask) and int(solo.count[0]) == int(labels.count[0])
    assert torch.equal(solo.rows[:len(rows)], labels.rows[:len(rows)])


@pytest.mark.parametrize("N,pattern", [(17080, "batch"), (1000, "none"), (1000, "one"), (1000, "tile_full"), (77, "all"),
                                       (5000, "dense")])
@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("f32_products", [False, True])
def test_comb_pair_effective_weight_hidden64(N, pattern, p_drop, f32_products, monkeypatch):
    """Comb pair at hidden 64 in effective-weight form (glass_comb_eff_fwd/bwd_f32: every row tile multiplies the
    unlabeled-row weight, the listed labeled rows are recomputed by extra workgroups) against fp64 — forward with the
    GraphNorm prologue (+ dropout, side output) and the output statistics, data gradient with the backward-GraphNorm column
    sums, weight / bias gradient — and against the two-product kernels on the same inputs.  reference impl/models.py:165-173."""
    from glass_amd import stack, ops
    from glass_amd.arena import ParamArena
    from glass_amd.factory import build_glass
    # the forward's product form (split bf16 pieces by default, the f32-input MFMA as the per-call option): both against fp64
    monkeypatch.setattr(ops, "DENSE_F32_PRODUCTS", f32_products)
    torch.manual_seed(11)
    H, z = 64, 0.95
    model = build_glass(H, 1, 5, 3, "mean", "sum", z).to(DEV).train()
    arena = ParamArena(model)
    conv = model.conv.convs[0]
    st = conv._stack["comb"]
    rng = np.random.default_rng(N)
    if pattern == "batch":      # ppi_bp-shape: 80 subgraphs x 10 nodes, nodes shared between subgraphs, some padding
        pos = rng.integers(0, N, (80, 10))
        pos[:, 8:][rng.random((80, 2)) < 0.5] = -1
        pos[5] = pos[4]
    elif pattern == "none":
        pos = np.full((4, 5), -1)
    elif pattern == "one":
        pos = np.full((4, 5), -1)
        pos[2, 3] = 517
    elif pattern == "tile_full":  # every row of one 16-row wave tile and of one 64-row workgroup tile
        pos = np.concatenate([np.arange(32, 48), np.arange(640, 704)]).reshape(8, 10)
    elif pattern == "all":
        pos = np.arange(N + 3).reshape(-1, 10) % N   # every node, three of them twice
    else:                        # a third of the rows labeled: more extra workgroups than a batch ever has
        pos = rng.permutation(N)[:1660].reshape(-1, 10)
    pos_t = torch.from_numpy(pos.astype(np.int64)).to(DEV)
    labels = stack.BatchLabels(N, pos_t.numel(), DEV)
    labels.load(pos_t)
    mask = labels.mask
    lab = mask.bool().unsqueeze(1)
    ops.rng_seed(99, DEV)
    arena.refresh_transposes(ops.rng_state(DEV))
    a, h = torch.randn(N, H, device=DEV) * 2 + 0.5, torch.randn(N, H, device=DEV)
    gmod = conv.gn
    with torch.no_grad():
        gmod.weight.uniform_(0.5, 1.5)
        gmod.bias.uniform_(-0.3, 0.3)
        gmod.mean_scale.uniform_(0.7, 1.1)
    gsaved = stack._GN(gmod).stats(a)
    call = 16
    # ---- forward: eff form vs two-product kernel vs fp64
    nblk_eff = int(stack._lib.load().glass_comb_eff_blocks(N, H, labels.cap))           # backward partials
    nblk_fwd = int(stack._lib.load().glass_comb_eff_fwd_blocks(N, H, labels.cap))       # forward partials (its own geometry)
    c, g = torch.empty(N, H, device=DEV), torch.empty(N, H, device=DEV)
    cstat = torch.empty(nblk_fwd, 2, H, dtype=torch.float64, device=DEV)
    stack._comb_eff_fwd(a, h, conv, mask, c, cstat, (gsaved, 0, p_drop, call, g), labels)
    c2, g2 = torch.empty(N, H, device=DEV), torch.empty(N, H, device=DEV)
    cstat2 = torch.empty(-(-N // 64), 2, H, dtype=torch.float64, device=DEV)
    stack._dual_fwd(a, h, st, mask, z, 0, None, c2, cstat2, gn=(gsaved, 0, p_drop, call, g2))
    assert torch.equal(g, g2)   # the normalised (+ dropped) operand: same arithmetic, same mask
    W, b = st[0].double(), st[1].double()
    x = torch.cat([g, h], 1).double()
    C1, C0 = x @ W[:H].t() + b[:H], x @ W[H:].t() + b[H:]
    ref = torch.where(lab, z * C1 + (1 - z) * C0, (1 - z) * C1 + z * C0)
    assert rel_inf(c.double(), ref) < TOL and rel_inf(c2.double(), ref) < TOL
    assert rel_inf(cstat[:, 0].sum(0), ref.sum(0)) < TOL and rel_inf(cstat[:, 1].sum(0), (ref * ref).sum(0)) < TOL
    if p_drop == 0:   # g = GraphNorm(a) checked against fp64 as well
        mu = a.double().mean(0)
        o = a.double() - gmod.mean_scale.double() * mu
        gref = gmod.weight.double() * o / (o.pow(2).mean(0) + gmod.eps).sqrt() + gmod.bias.double()
        assert rel_inf(g.double(), gref) < TOL
    # ---- backward: data gradient (+ conv.gn's backward column sums) and weight-gradient partials, one launch
    for p in (st[2], st[3]):
        p.zero_()
    dc = torch.randn(N, H, device=DEV)
    din = torch.empty(N, 2 * H, device=DEV)
    gpart = torch.empty(nblk_eff, 2, H, dtype=torch.float64, device=DEV)
    pending = []
    stack._comb_eff_bwd(dc, conv, mask, din, g, h, pending, 0, (gpart, a, gsaved, gmod.mean_scale, 0, p_drop, call), labels)
    stack._reduce_pending(pending)
    w1 = torch.where(lab, torch.tensor(z, device=DEV, dtype=torch.float64), torch.tensor(1 - z, device=DEV, dtype=torch.float64))
    dZ = torch.cat([w1 * dc.double(), (1 - w1) * dc.double()], 1)
    dref = dZ @ W
    assert rel_inf(din.double(), dref) < TOL
    assert rel_inf(st[2].double(), dZ.t() @ x) < TOL and rel_inf(st[3].double(), dZ.sum(0)) < TOL
    keep = (g != 0).double() / (1 - p_drop) if p_drop > 0 else torch.ones_like(dref[:, :H])
    if p_drop > 0:   # where the normalised value itself is 0 the mask cannot be read back from g: use the two-product kernel's sums
        gpart2 = torch.empty(-(-N // 64), 2, H, dtype=torch.float64, device=DEV)
        din2 = torch.empty_like(din)
        stack._dual_dgrad(dc, None, st, mask, z, 0, 2 * H, None, din2, gn=(gpart2, a, gsaved, gmod.mean_scale, 0, p_drop, call))
        assert rel_inf(din.double(), din2.double()) < TOL
        assert rel_inf(gpart.sum(0), gpart2.sum(0)) < TOL
    else:
        gg = dref[:, :H] * keep
        xhat = (a.double() - gmod.mean_scale.double() * gsaved[:H].double()) * gsaved[H:2 * H].double()
        assert rel_inf(gpart[:, 0].sum(0), gg.sum(0)) < TOL and rel_inf(gpart[:, 1].sum(0), (gg * xhat).sum(0)) < TOL
    # repeatable bit for bit
    c3 = torch.empty_like(c)
    stack._comb_eff_fwd(a, h, conv, mask, c3, cstat, (gsaved, 0, p_drop, call, g), labels)
    assert torch.equal(c3, c)
