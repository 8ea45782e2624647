"""K1m on the GPU: glass_spmm_max_csr_f32 / glass_spmm_max_bwd_f32 (csrc/spmm_max.hip) against the restatement
tests/aggr_max_oracle.py on every plan form and lane layout, the host objects (graph.CSRAdj.max_fwd / max_bwd, ops.spmm), a
GLASS model with aggr "max" against the fp64 oracle, and impl.train.train on the captured per-op step.

The forward is compared BIT FOR BIT: every output is one rounded fp32 product, no sum exists to reorder, and the winner of
equal values is fixed by rule.  The backward is a sum: rel-inf <= 1e-5 against fp64, and bitwise run to run."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import aggr_max_oracle as MO
from helpers import rel_inf, flat_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
GUARD = 64
WIDTHS = (4, 18, 64, 68, 128, 132, 256, 260)   # the widths of tests/test_gpu_step_tail.py: every VW / LPR case, two column tiles
NEVER = 9                                        # a source of the mixed graph that never wins (below)


def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """`n` elements filled with `fill`, GUARD sentinel elements in front and behind (tests/test_gpu_step_tail.py's)"""
    def __init__(self, n, fill, dtype=torch.float32):
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


# ---- the two adjacencies -------------------------------------------------------------------------------------------------
def _edges(degrees, n, rng, hub_share, hub_frac=0.0):
    """One destination row per entry of `degrees`; sources uniform, except that a share of the rows also names source 5, and a
    fraction of all entries (a hub: its row of the TRANSPOSED matrix is long and cut).  Not symmetric.  Weights in +-[0.25, 2)."""
    rows, cols = [], []
    for r, d in enumerate(degrees):
        c = rng.integers(0, n, d)
        if d and rng.random() < hub_share:
            c[rng.integers(0, d)] = 5
        rows.append(np.full(d, r))
        cols.append(c)
    row, col = np.concatenate(rows), np.concatenate(cols)
    col[rng.random(col.shape[0]) < hub_frac] = 5
    w = (rng.uniform(0.25, 2.0, row.shape[0]) * rng.choice([-1.0, 1.0], row.shape[0])).astype(np.float32)
    return row, col, w


@functools.lru_cache(maxsize=None)
def _graph(kind):
    """-> (n, edge_index, edge_weight) on the host, in SHUFFLED edge order (CSRAdj sorts).
    mixed: rows of 0, 1, 2, 63, 64, 65, 255, 256, 257 and 700 in-entries (both sides of GLASS_K1_LONG_THR = 256 and of the 64
      the plan lowers it to on a product this small; 257 and 700 are cut, 700 into three chunks), then 997 short rows of 1..12
      (sweep items), a duplicate (row, col) pair with different weights, a self-loop; source NEVER feeds the long rows only,
      with positive weights.
    all_long: 40 rows of 64..300 entries, one of 700, one empty — fewer than 1 024 rows, nnz >= 64 n: no sweep at all."""
    rng = np.random.Generator(np.random.PCG64(7 if kind == "mixed" else 8))
    if kind == "mixed":
        head = [0, 1, 2, 63, 64, 65, 255, 256, 257, 700]
        degrees = [d - (d >= 255) for d in head] + list(rng.integers(1, 13, 997))   # (the long rows' last entry: below)
        n = len(degrees)
        row, col, w = _edges(degrees, n, rng, 0.7)
        col[col == NEVER] = NEVER + 1
        long_rows = [r for r, d in enumerate(head) if d >= 255]
        extra_r = np.array(long_rows + [20, 20, 30])           # NEVER -> every long row; (20, 40) twice; self-loop (30, 30)
        extra_c = np.array([NEVER] * len(long_rows) + [40, 40, 30])
        extra_w = np.array([1.5] * len(long_rows) + [0.5, -1.25, 0.75], dtype=np.float32)
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
    """(graph.CSRAdj on the device, MaxAdj restatement on the host, both built from the same shuffled edge list)"""
    from glass_amd import graph
    n, ei, ew = _graph(kind)
    adj = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "max")
    return adj, MO.MaxAdj(ei, ew, n)


def test_plans_take_every_form_and_the_device_csr_is_the_restatements():
    from glass_amd import graph
    for kind in ("mixed", "all_long"):
        adj, ref = _adj(kind)
        assert adj.aggr == "max"
        # the CSR, the transposed CSR and the entry map: integer for integer
        for got, want in ((adj.fwd.rowptr, ref.rowptr), (adj.fwd.col, ref.col), (adj.bwd.rowptr, ref.rowptr_t),
                          (adj.bwd.col, ref.col_t), (adj.eid_t, ref.eid_t)):
            assert got.dtype == torch.int32 and torch.equal(got.cpu().to(torch.int64), want)
        assert torch.equal(adj.fwd.val.cpu(), ref.val) and torch.equal(adj.bwd.val.cpu(), ref.val_t)   # raw weights: "sum" values
        n, ei, ew = _graph(kind)
        as_sum = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "sum")   # values and deg are the ones "sum" computes, bit for bit
        assert torch.equal(_bits(adj.deg), _bits(as_sum.deg)) and torch.equal(_bits(adj.fwd.val), _bits(as_sum.fwd.val))
        assert not torch.equal(ref.rowptr, ref.rowptr_t), "the pattern must not be symmetric"
    f, b = _adj("mixed")[0].fwd.header, _adj("mixed")[0].bwd.header
    # header words (tests/test_cabi.py): 4 sweep items, 5 long items, 6 reduce rows, 7 partial slots, 8 threshold, 9 chunk
    assert f[4] > 100 and f[5] >= 9 and f[6] == 2 and f[7] == 2 + 3 and f[8] == 64 and f[9] == 256
    assert b[4] > 100 and b[5] >= 3 and b[6] >= 1 and b[7] >= 3, "the hub's transposed row is cut"
    for h in (_adj("all_long")[0].fwd.header, _adj("all_long")[0].bwd.header):
        assert h[4] == 0 and h[8] == 0 and h[5] >= 42 and h[6] >= 1 and h[7] >= 2, "no sweep, every row workgroup items, cut rows"


# ---- raw entries on guarded buffers --------------------------------------------------------------------------------------
def _raw_fwd(adj, Xv, ldy_extra=0, lda_extra=0):
    """glass_spmm_max_csr_f32 -> (Y [n, H] view, arg view, their Guarded buffers + the workspace's)"""
    L, lib = _lib()
    op, (n, H) = adj.fwd, (adj.fwd.n_rows, Xv.shape[1])
    ldy, lda = H + ldy_extra, H + lda_extra
    Y, A = Guarded(n * ldy, float("nan")), Guarded(n * lda, -7, torch.int32)
    nbytes = lib.glass_spmm_max_ws_bytes(op.header.ctypes.data, H)
    assert nbytes == int(op.header[7]) * H * 8
    W = Guarded(max(nbytes // 4, 4), -1, torch.int32)   # (need not be initialised: junk on purpose)
    rc = lib.glass_spmm_max_csr_f32(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), Xv.data_ptr(), Xv.stride(0),
                                    Y.t.data_ptr(), ldy, A.t.data_ptr(), lda, n, H, op.header.ctypes.data, op.plan.data_ptr(),
                                    W.t.data_ptr(), _stream())
    L.check(rc, "glass_spmm_max_csr_f32")
    torch.cuda.synchronize()
    return Y.t.view(n, ldy), A.t.view(n, lda), (Y, A, W)


def _raw_bwd(adj, dYv, argv, ldx_extra=0):
    L, lib = _lib()
    op, (n, H) = adj.bwd, (adj.bwd.n_rows, dYv.shape[1])
    ldx = H + ldx_extra
    D = Guarded(n * ldx, float("nan"))
    nbytes = lib.glass_spmm_max_bwd_ws_bytes(op.header.ctypes.data, H)
    assert nbytes == int(op.header[7]) * H * 4
    W = Guarded(max(nbytes // 4, 4), float("nan"))
    rc = lib.glass_spmm_max_bwd_f32(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), adj.eid_t.data_ptr(),
                                    dYv.data_ptr(), dYv.stride(0), argv.data_ptr(), argv.stride(0), D.t.data_ptr(), ldx, n, H,
                                    op.header.ctypes.data, op.plan.data_ptr(), W.t.data_ptr(), _stream())
    L.check(rc, "glass_spmm_max_bwd_f32")
    torch.cuda.synchronize()
    return D.t.view(n, ldx), (D, W)


def _operands(kind, H):
    n = _graph(kind)[0]
    g = torch.Generator().manual_seed(1000 * H + (kind == "mixed"))
    X = torch.randn(n, H, generator=g)
    if kind == "mixed":
        X[NEVER] = -100.0   # positive weights into rows that hold hundreds of other entries: never the largest product
    return X, torch.randn(n, H, generator=g)


@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("kind", ("mixed", "all_long"))
def test_forward_bits_and_backward_against_the_restatement(kind, H):
    adj, ref = _adj(kind)
    X, dY = _operands(kind, H)
    Y_ref, arg_ref = MO.max_aggregate(ref.rowptr, ref.col, ref.val, X)           # fp32: the same single product
    Yv, Av, guards = _raw_fwd(adj, X.to(DEV))
    assert torch.equal(Av.cpu(), arg_ref), (kind, H, "arg")
    assert torch.equal(_bits(Yv.cpu()), _bits(Y_ref)), (kind, H, "Y bits")
    assert all(g.intact() for g in guards), (kind, H, "guards of Y / arg / workspace")
    empty = (ref.rowptr[1:] == ref.rowptr[:-1]).nonzero().reshape(-1)
    assert len(empty) >= 1 and bool((Yv.cpu()[empty] == 0).all()) and bool((Av.cpu()[empty] == -1).all())
    # backward, from the device's own arg
    dX_ref = MO.max_aggregate_bwd(ref.rowptr_t, ref.col_t, ref.val_t, ref.eid_t, dY.double(), arg_ref)
    dYd = dY.to(DEV)
    dXv, guards = _raw_bwd(adj, dYd, Av)
    first = dXv.clone()
    err = rel_inf(dXv.cpu(), dX_ref)
    print(f"{kind} H={H}: dX rel-inf {err:.2e}")
    assert err <= TOL, (kind, H, err)
    assert all(g.intact() for g in guards), (kind, H, "guards of dX / workspace")
    dXv2, _g = _raw_bwd(adj, dYd, Av)
    assert torch.equal(_bits(first), _bits(dXv2)), (kind, H, "two runs differ")
    winners = set(ref.col[arg_ref[arg_ref >= 0].to(torch.int64)].tolist())
    losers = [s for s in range(ref.n) if s not in winners and ref.rowptr_t[s + 1] > ref.rowptr_t[s]]
    if kind == "mixed":
        assert NEVER in losers
    for s in losers:
        assert bool((dXv[s] == 0).all()), (kind, H, s, "a source that never wins")


def test_constructed_ties_go_to_the_smaller_entry():
    """Row 0: 700 entries (cut into chunks, four waves each, every lane group) from sources 1 and 2, whose rows and weights are
    identical — every product of a channel is the same number, so arg is the row's first entry, in every channel.  Row 3:
    +0.0 (source 4) against -0.0 (source 5), both orders.  Row 6: the same two sources again behind a larger-weight duplicate."""
    from glass_amd import graph
    n = 1030   # (>= 1 024 rows: the plan keeps its sweep for the short rows)
    r = [0] * 700 + [3, 3, 6, 6, 6, 7]
    c = [1, 2] * 350 + [4, 5, 5, 4, 4, 5]
    w = [0.75] * 700 + [1.0, 1.0, 1.0, 1.0, 2.0, 1.0]
    ei, ew = torch.tensor([r, c]), torch.tensor(w)
    ref = MO.MaxAdj(ei, ew, n)
    adj = graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, "max")
    assert adj.fwd.header[7] >= 2
    for H in (64, 18):
        X = torch.randn(n, H, generator=torch.Generator().manual_seed(H))
        X[2] = X[1]
        X[4], X[5] = 0.0, -0.0
        Y_ref, arg_ref = MO.max_aggregate(ref.rowptr, ref.col, ref.val, X)
        assert bool((arg_ref[0] == 0).all()) and arg_ref[3, 0] == 700 and bool(torch.signbit(Y_ref[7]).all())
        Yv, Av, guards = _raw_fwd(adj, X.to(DEV))
        assert torch.equal(Av.cpu(), arg_ref) and torch.equal(_bits(Yv.cpu()), _bits(Y_ref))
        assert bool((Av[0] == 0).all()) and all(g.intact() for g in guards)
        # the whole gradient of row 0 goes to source 1 (entry 0), none to source 2
        dY = torch.randn(n, H, generator=torch.Generator().manual_seed(H + 1))
        dXv, _g = _raw_bwd(adj, dY.to(DEV), Av)
        assert torch.equal(_bits(dXv[1].cpu()), _bits(0.75 * dY[0])) and bool((dXv[2] == 0).all())


@pytest.mark.parametrize("H,pads", [(64, (8, 4, 12, 4)), (64, (3, 1, 2, 5)), (18, (2, 6, 1, 3))])
def test_strided_operands(H, pads):
    """X, Y, arg and dX / dY as column slices of wider buffers: multiples of 4 keep the 16-byte form, anything else takes the
    scalar one; the columns beyond H are neither read (NaN) nor written."""
    adj, ref = _adj("mixed")
    px, py, pa, pd = pads
    X, dY = _operands("mixed", H)
    Y_ref, arg_ref = MO.max_aggregate(ref.rowptr, ref.col, ref.val, X)
    Xb = torch.full((ref.n, H + px), float("nan"), device=DEV)
    Xb[:, :H] = X.to(DEV)
    Yv, Av, guards = _raw_fwd(adj, Xb[:, :H], py, pa)
    assert torch.equal(Av[:, :H].cpu(), arg_ref) and torch.equal(_bits(Yv[:, :H].cpu()), _bits(Y_ref))
    assert bool(torch.isnan(Yv[:, H:]).all()) and bool((Av[:, H:] == -7).all()) and all(g.intact() for g in guards)
    dYb = torch.full((ref.n, H + py), float("nan"), device=DEV)
    dYb[:, :H] = dY.to(DEV)
    dXv, guards = _raw_bwd(adj, dYb[:, :H], Av[:, :H], pd)
    dX_ref = MO.max_aggregate_bwd(ref.rowptr_t, ref.col_t, ref.val_t, ref.eid_t, dY.double(), arg_ref)
    assert rel_inf(dXv[:, :H].cpu(), dX_ref) <= TOL
    assert bool(torch.isnan(dXv[:, H:]).all()) and all(g.intact() for g in guards)
    # the contiguous call gives the same bits where it takes the same form (the order of the sum follows the lane layout:
    # strides that are no multiple of 4 floats move a width that has a 16-byte form to the scalar one)
    if H % 4 or all(p % 4 == 0 for p in pads):
        dXc, _g = _raw_bwd(adj, dY.to(DEV), Av[:, :H].contiguous())
        assert torch.equal(_bits(dXc), _bits(dXv[:, :H].contiguous()))


def test_autograd_binding_and_the_replicated_refusal():
    from glass_amd import ops
    L, _ = _lib()
    adj, ref = _adj("mixed")
    H = 20
    X, dY = _operands("mixed", H)
    Xd = X.to(DEV).requires_grad_(True)
    Y = ops.spmm(adj, Xd)
    Y.backward(dY.to(DEV))
    Y_ref, arg_ref = MO.max_aggregate(ref.rowptr, ref.col, ref.val, X)
    assert torch.equal(_bits(Y.detach().cpu()), _bits(Y_ref))
    assert rel_inf(Xd.grad.cpu(), MO.max_aggregate_bwd(ref.rowptr_t, ref.col_t, ref.val_t, ref.eid_t, dY.double(), arg_ref)) <= TOL
    with pytest.raises(L.GlassHipError, match="replicated max aggregation is not built"):
        ops.spmm_rep(adj, torch.zeros(2 * ref.n, H, device=DEV), 2)


# ---- through the model ----------------------------------------------------------------------------------------------------
def model_graph(seed):
    """N = 120, 720 entries (mean degree 6), node 0 isolated, not symmetric; use_deg-style features (the rank of a node's
    degree, entries in plus entries out, among the distinct degrees).

    Max is not smooth: where winner and runner-up are closer than the fp32 error of the operand, the gradient takes another
    route, so the test asserts — in the fp64 oracle alone — that the closest pair of every layer, row and channel is at least
    1e-3 of the layer's largest product apart.  On a graph whose 720 entries are spread evenly that cannot be had by choosing
    a seed: the activations are heavy-tailed (largest product ~15 standard deviations), and measured on such graphs 2 - 3 %
    of the contested elements lie below 1e-3 — hundreds of the 119 x 64 x 2 at hidden 64.  So the entries are spread
    UNEVENLY: one destination (node 1) takes 602 in-entries from all over the graph, duplicates with different weights among
    them, the other 118 exactly one (no runner-up, no tie to flip).  That leaves hidden x 2 contested elements, each a max
    over 602 entries, and a seed search on the CPU finds parameters where none of them is close.  Every element is compared."""
    rng = np.random.Generator(np.random.PCG64(seed))
    N = 120
    deg = np.ones(N, dtype=np.int64)
    deg[0] = 0
    deg[1] = 720 - (N - 2)
    row = np.repeat(np.arange(N), deg)
    col = rng.integers(1, N, row.shape[0])            # node 0 is no source either
    w = rng.uniform(0.5, 1.5, row.shape[0]).astype(np.float32)
    perm = rng.permutation(row.shape[0])
    ei = torch.from_numpy(np.stack((row[perm], col[perm])))
    total = deg + np.bincount(col, minlength=N)
    ranks = np.unique(total, return_inverse=True)[1]
    x = torch.from_numpy(ranks.astype(np.int64)).reshape(N, 1, 1)
    pos = torch.from_numpy(np.stack([rng.choice(N, 8, replace=False) for _ in range(10)]).astype(np.int64))
    pos[::3, -2:] = -1
    y = torch.from_numpy(rng.integers(0, 3, 10))
    return N, ei, torch.from_numpy(w[perm].copy()), x, pos, y


MODEL_SEEDS = {8: (0, 2), 64: (3, 4)}   # hidden -> (graph seed, parameter seed), found on the CPU (see model_oracle)


def model_oracle(hidden, seeds):
    """The fp64 oracle of the model case: OracleGLASS(aggr "sum") with every conv.adj = MaxAdj.  Returns (state dict in fp32,
    loss, logits, gradients, smallest relative winner / runner-up gap over the layers, inputs)."""
    from helpers import build_glass
    from oracle import glass_oracle as O
    gseed, pseed = seeds
    N, ei, ew, x, pos, y = model_graph(gseed)
    torch.manual_seed(pseed)
    model = build_glass(hidden, 2, int(x.max()), 3, "max", "mean", 0.8, dropout=0.0, jk=True)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    orc = O.OracleGLASS(hidden, 2, int(x.max()), 3, aggr="sum", pool="mean", z_ratio=0.8).double()
    orc.load_state_dict(sd)
    orc.train()
    madj = MO.MaxAdj(ei, ew.double(), N)
    for conv in orc.conv.convs:
        conv.adj = madj
    logits = orc(x, ei, ew.double(), pos, O.max_zero_one(x, pos))
    loss = nn.CrossEntropyLoss()(logits, y)
    loss.backward()
    assert len(madj.seen) == 2
    gap = min(MO.smallest_gap(madj, X) for X in madj.seen)
    grads = {k: p.grad.clone() for k, p in orc.named_parameters()}
    return model, sd, loss.detach(), logits.detach(), grads, gap, (N, ei, ew, x, pos, y)


@pytest.mark.parametrize("hidden", (8, 64))
def test_model_with_max_aggregation_against_the_fp64_oracle(hidden):
    from impl import utils
    model, sd, loss_ref, logits_ref, grads_ref, gap, (N, ei, ew, x, pos, y) = model_oracle(hidden, MODEL_SEEDS[hidden])
    print(f"hidden {hidden}: smallest winner / runner-up gap in the oracle {gap:.3e} of the layer's largest product")
    assert gap >= 1e-3, gap
    model.to(DEV).train()
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in (x, ei, ew, pos, y))
    logits = model(xg, eig, ewg, posg, utils.MaxZOZ(xg, posg), id=0)
    loss = nn.CrossEntropyLoss()(logits, yg)
    loss.backward()
    torch.cuda.synchronize()
    assert all(c.adj.aggr == "max" for c in model.conv.convs)
    keys = sorted(grads_ref)
    e_logits = rel_inf(logits.detach().cpu(), logits_ref)
    e_loss = abs(loss.item() - loss_ref.item()) / abs(loss_ref.item())
    e_grad = rel_inf(flat_grads({k: p.grad.cpu() for k, p in model.named_parameters()}, keys), flat_grads(grads_ref, keys))
    print(f"hidden {hidden}: loss {e_loss:.2e} logits {e_logits:.2e} flat gradient {e_grad:.2e}")
    assert e_loss <= TOL and e_logits <= TOL and e_grad <= TOL


def _tiny(seed, n_batches):
    from glass_amd import synth
    from impl import config
    config.set_device(0)
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=seed, n_batches=n_batches)
    return (w, ) + tuple(torch.from_numpy(a).to(DEV) for a in (x, ei, ew, pos, y))


def test_training_on_the_captured_per_op_step_equals_its_eager_run(monkeypatch):
    """Two epochs of impl.train.train at aggr "max": a TrainStep is cached on the model, it is captured and reports the per-op
    form (the stack program does not serve max), and loss and parameters equal, bit for bit, those of a deep copy trained by the
    same TrainStep with eager launches."""
    from helpers import build_glass
    from impl import SubGDataset, train, utils
    from glass_amd import stack, train as gtrain
    w, x, ei, ew, pos, y = _tiny(2, 2)
    torch.manual_seed(3)
    gnn = build_glass(64, 2, int(x.max()), w.n_class, "max", w.pool, w.z_ratio).to(DEV)
    twin = copy.deepcopy(gnn)
    loss_fn = nn.CrossEntropyLoss()
    ds = SubGDataset.GDataset(x, ei, ew, pos, y)
    loader = lambda: SubGDataset.ZGDataloader(ds, w.batch, z_fn=utils.MaxZOZ, shuffle=False, drop_last=True)
    out = {}
    for name, net, use_graph in (("graph", gnn, True), ("eager", twin, False)):
        monkeypatch.setattr(gtrain, "USE_GRAPH", use_graph)
        opt = torch.optim.Adam(net.parameters(), lr=5e-3)
        out[name] = [train.train(opt, net, loader(), loss_fn) for _ in range(2)]
        steps = net.__dict__.get("_glass_train_steps") or {}
        assert len(steps) == 1
        step = next(iter(steps.values()))
        net.train()
        assert step.graphed == use_graph and not step._program_step() and not stack.step_supported(net, loss_fn)
        assert not stack.StackProgram.supported(net.conv) and all(c.adj.aggr == "max" for c in net.conv.convs)
    assert np.isfinite(out["graph"]).all() and out["graph"][1] != out["graph"][0]
    assert np.array_equal(np.float32(out["graph"]).view(np.int32), np.float32(out["eager"]).view(np.int32)), out
    sd, sd2 = gnn.state_dict(), twin.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
