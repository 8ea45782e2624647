"""Edge dropout on the GPU (K2d, csrc/spmm_dropedge.hip): the drawn mask against the exact integer restatement, the values against
the existing K2 on the masked weights (ops.spmm_w / CSRAdj.values_of, bit for bit) and the fp64 restatement, the pairing of a
backward with its forward's mask, the model against a live-edge-weight twin, and the captured per-op training step."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import dropedge_oracle as DO
from helpers import build_glass, flat_grads, rel_inf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5          # the project's standing bound: rel-inf on the vector against the fp64 restatement


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _adj(aggr, family):
    from glass_amd import graph
    n, ei, w, _ = DO.mixed(family)
    eid, wd = torch.tensor(ei, device=DEV), torch.tensor(w, device=DEV)   # (copies: the oracle's arrays are read-only)
    return graph.CSRAdj(eid, wd, n, aggr), wd


def _state(step):
    """The dropout stream at (SEED, step), reached through rng_advance; returns the words as the device holds them."""
    from glass_amd import ops
    ops.rng_seed(DO.SEED, DEV)
    for _ in range(step):
        ops.rng_advance(DEV)
    assert _words() == (DO.SEED, step)
    return DO.SEED, step


def _words():
    """The live (seed, step) words, read back from the device."""
    from glass_amd import ops
    return tuple(int(v) for v in ops.rng_state(DEV).cpu())


# ---- 1. the mask, exactly ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symmetric", (True, False))
@pytest.mark.parametrize("p", DO.PS)
def test_mask_equals_the_integer_restatement(p, symmetric):
    from glass_amd import ops
    n, ei, _w, _ = DO.mixed("rand")
    adj = _adj("sum", "rand")[0]
    seen = []
    for step in (0, 1):
        seed, st = _state(step)
        for call_id in DO.CALL_IDS:
            got = ops.edge_keep_mask(adj, p, call_id, symmetric)
            assert got.dtype == torch.uint8 and got.shape == (ei.shape[1], ) and got.device.type == "cuda"
            want = DO.keep_mask(ei, n, p, seed, st, call_id, symmetric)
            assert np.array_equal(got.cpu().numpy(), want), (p, symmetric, step, call_id)
            seen.append(want)
    if p == 0.0:
        assert all(bool(k.all()) for k in seen)
    else:
        assert all(not np.array_equal(seen[0], k) for k in seen[1:]) and 0 < seen[0].mean() < 1
        # the same bits from an adjacency of another aggregation (two launches instead of one)
        assert torch.equal(ops.edge_keep_mask(_adj("gcn", "rand")[0], p, DO.CALL_IDS[1], symmetric).cpu(), torch.from_numpy(seen[-1]))


# ---- 2. the values, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", DO.FAMILIES)
@pytest.mark.parametrize("aggr", DO.AGGRS)
def test_values_equal_k2_on_the_masked_weights(aggr, family):
    from glass_amd import ops
    n, ei, w, _ = DO.mixed(family)
    adj, wd = _adj(aggr, family)
    seed, st = _state(1)
    gen = torch.Generator().manual_seed(5)
    for p, symmetric, call_id in ((0.3, True, DO.CALL_IDS[0]), (0.9, True, DO.CALL_IDS[1]), (0.3, False, DO.CALL_IDS[1])):
        keep = ops.edge_keep_mask(adj, p, call_id, symmetric)
        keep_np = DO.keep_mask(ei, n, p, seed, st, call_id, symmetric)
        assert np.array_equal(keep.cpu().numpy(), keep_np)
        wk = wd * keep.to(torch.float32)
        val, val_t, deg = adj.values_of(wk)                                   # the existing K2: the yardstick
        got = [t.clone() for t in adj.dropedge_values(p, call_id, symmetric)]
        again = adj.dropedge_values(p, call_id, symmetric)
        for name, a, b, c in zip(("val", "val_t", "deg"), got, (val, val_t, deg), again):
            assert a.dtype == torch.float32 and a.shape == b.shape
            assert torch.equal(_bits(a), _bits(b)), (aggr, family, p, symmetric, name)
            assert torch.equal(_bits(a), _bits(c)), "two draws at one state"
        assert bool((got[0][keep[adj.perm] == 0] == 0).all())
        if p == 0.9:
            size = np.bincount(ei[0], minlength=n)
            dead = (np.bincount(ei[0], weights=keep_np, minlength=n) == 0) & (size > 0)
            assert dead.any() and bool((got[2].cpu().numpy()[dead] == 1.0).all())
        val64, deg64 = DO.masked_values(ei, w, keep_np, n, aggr)
        A64 = DO.dense(ei, val64, n)
        for H in (64, 8):
            x = torch.randn(n, H, generator=gen)
            dy = torch.randn(n, H, generator=gen)
            xa, xb = (x.to(DEV).requires_grad_(True) for _ in range(2))
            ya = ops.spmm_dropedge(adj, xa, p, call_id, symmetric)
            yb = ops.spmm_w(adj, xb, wk)
            (dxa, ) = torch.autograd.grad(ya, xa, dy.to(DEV))
            (dxb, ) = torch.autograd.grad(yb, xb, dy.to(DEV))
            assert torch.equal(_bits(ya), _bits(yb)) and torch.equal(_bits(dxa), _bits(dxb)), (aggr, family, p, symmetric, H)
            y2 = ops.spmm_dropedge(adj, xa, p, call_id, symmetric)
            assert torch.equal(_bits(ya), _bits(y2))
            if p == 0.9:
                assert bool((ya[torch.from_numpy(dead).to(DEV)] == 0).all()), "a fully dropped row aggregates to zero"
            if family == "rand":
                caller = torch.empty_like(got[0])
                caller[adj.perm] = got[0]
                e = (rel_inf(caller.cpu(), val64), rel_inf(got[2].cpu(), deg64),
                     rel_inf(ya.detach().cpu(), A64 @ x.double().numpy()), rel_inf(dxa.cpu(), A64.T @ dy.double().numpy()))
                print(f"{aggr} p {p} symmetric {symmetric} H {H}: val {e[0]:.2e} deg {e[1]:.2e} y {e[2]:.2e} dx {e[3]:.2e}")
                assert max(e) <= TOL, (aggr, p, symmetric, H, e)


def test_op_refusals():
    from glass_amd import graph, ops, _lib
    n, ei, w, _ = DO.mixed("int")
    mx = graph.CSRAdj(torch.tensor(ei, device=DEV), torch.tensor(w, device=DEV), n, "max")
    x = torch.zeros(n, 8, device=DEV)
    with pytest.raises(_lib.GlassHipError, match="edge dropout"):
        mx.dropedge_values(0.3, 18)
    with pytest.raises(_lib.GlassHipError, match="edge dropout"):
        ops.spmm_dropedge(mx, x, 0.3, 18)
    with pytest.raises(_lib.GlassHipError, match="edge dropout"):
        ops.edge_keep_mask(mx, 0.3, 18)
    adj = _adj("mean", "int")[0]
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            ops.spmm_dropedge(adj, x, bad, 18)
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            adj.dropedge_values(bad, 18)


# ---- 3. a backward runs with its forward's mask -----------------------------------------------------------------------------
@pytest.mark.parametrize("aggr", ("mean", "gcn"))
def test_backward_uses_the_forwards_mask_after_another_training_forward(aggr):
    """SpMMDropFn keeps the transposed values in the adjacency's per-call_id buffers and draws them again, from the words its
    forward read, when another draw has overwritten them."""
    from glass_amd import ops
    n = DO.mixed("rand")[0]
    adj, wd = _adj(aggr, "rand")
    p, call_id = 0.3, DO.CALL_IDS[0]
    gen = torch.Generator().manual_seed(9)
    x1, x2, dy = (torch.randn(n, 8, generator=gen).to(DEV) for _ in range(3))
    x1.requires_grad_(True)
    ops.rng_seed(DO.SEED, DEV)
    keeps, ys = [], []
    for x in (x1, x2):                                   # two training forwards as EmbZGConv.forward frames them
        ops.rng_advance(DEV)
        with ops.rng_scope(DEV, ops.rng_snapshot(DEV)):
            keeps.append(ops.edge_keep_mask(adj, p, call_id))
            ys.append(ops.spmm_dropedge(adj, x, p, call_id))
    assert not torch.equal(keeps[0], keeps[1])
    (dx, ) = torch.autograd.grad(ys[0], x1, dy)          # ... then the backward of the first
    refs = []
    for k in keeps:
        xr = x1.detach().clone().requires_grad_(True)
        yr = ops.spmm_w(adj, xr, wd * k.to(torch.float32))
        refs.append((yr, torch.autograd.grad(yr, xr, dy)[0]))
    assert torch.equal(_bits(ys[0]), _bits(refs[0][0])) and torch.equal(_bits(dx), _bits(refs[0][1]))
    assert not torch.equal(_bits(dx), _bits(refs[1][1]))
    # without a snapshot (the live words) the mask cannot be drawn again once the stream has moved on: refused, not mispaired
    y_live = ops.spmm_dropedge(adj, x1, p, call_id)
    ops.rng_advance(DEV)
    ops.spmm_dropedge(adj, x2, p, call_id)
    with pytest.raises(RuntimeError, match="dropout stream was advanced"):
        torch.autograd.grad(y_live, x1, dy)


# ---- 4. the model -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch():
    n, ei, w, _ = DO.mixed("rand")
    rng = np.random.Generator(np.random.PCG64(3))
    x = rng.integers(0, 5, (n, 1, 1)).astype(np.int64)
    B, S = 6, 9
    pos = np.full((B, S), -1, dtype=np.int64)
    for b in range(B):
        k = int(rng.integers(4, S + 1))
        pos[b, :k] = rng.choice(np.arange(n), k, replace=False)
    y = rng.integers(0, 3, B).astype(np.int64)
    return tuple(torch.tensor(a, device=DEV) for a in (x, ei, w, pos, y))


@pytest.mark.parametrize("aggr", ("mean", "gcn", "sum"))
@pytest.mark.parametrize("hidden", (64, 8))
def test_model_against_a_live_edge_weight_twin(hidden, aggr):
    from impl import utils
    from glass_amd import ops
    x, ei, w, pos, y = _batch()
    z = utils.MaxZOZ(x, pos)
    p = 0.3
    torch.manual_seed(1)
    model = build_glass(hidden, 2, 4, 3, aggr, "sum", 0.8, dropout=0.0, edge_dropout=p).to(DEV).train()
    twin = build_glass(hidden, 2, 4, 3, aggr, "sum", 0.8, dropout=0.0, live_edge_weight=True).to(DEV).train()
    plain = build_glass(hidden, 2, 4, 3, aggr, "sum", 0.8, dropout=0.0).to(DEV).eval()
    twin.load_state_dict(model.state_dict())
    plain.load_state_dict(model.state_dict())
    loss_fn = nn.CrossEntropyLoss()
    ops.rng_seed(DO.SEED, DEV)
    logits = model(x, ei, w, pos, z, id=0)                       # advances the stream once: the masks of (SEED, 1)
    loss = loss_fn(logits, y)
    loss.backward()
    assert _words() == (DO.SEED, 1)
    keeps = [ops.edge_keep_mask(c.adj, p, c.call_base + 2, c.edge_dropout_symmetric) for c in model.conv.convs]
    assert not torch.equal(keeps[0], keeps[1]) and all(0.2 <= 1 - float(k.float().mean()) <= 0.4 for k in keeps)
    for c, k in zip(twin.conv.convs, keeps):
        c.register_forward_pre_hook(lambda mod, args, k=k: (args[0], args[1], args[2] * k.to(torch.float32)) + tuple(args[3:]))
    logits_t = twin(x, ei, w, pos, z, id=0)
    loss_t = loss_fn(logits_t, y)
    loss_t.backward()
    mine = {k: v.grad.cpu() for k, v in model.named_parameters()}
    ref = {k: v.grad.cpu() for k, v in twin.named_parameters()}
    keys = sorted(ref)
    assert sorted(mine) == keys
    e = (rel_inf(logits.detach().cpu(), logits_t.detach().cpu()), abs(loss.item() - loss_t.item()) / abs(loss_t.item()),
         rel_inf(flat_grads(mine, keys), flat_grads(ref, keys)))
    print(f"hidden {hidden} {aggr}: logits {e[0]:.2e} loss {e[1]:.2e} flat gradient {e[2]:.2e}")
    assert max(e) <= TOL, e
    # ... and the masks matter: the model without edge dropout gives other logits in training mode
    with torch.no_grad():
        model.eval()
        ev, ev_plain = model(x, ei, w, pos, z, id=0), plain(x, ei, w, pos, z, id=0)
        assert torch.equal(_bits(ev), _bits(ev_plain)), "eval mode: bit for bit the model without the argument"
        assert rel_inf(logits.detach().cpu(), plain.train()(x, ei, w, pos, z, id=0).cpu()) > 1e-3
    assert _words() == (DO.SEED, 1), "neither the eval pass nor a model without dropout advanced the stream"


# ---- 5. the captured per-op step --------------------------------------------------------------------------------------------
def test_training_on_the_captured_per_op_step_equals_its_eager_run(monkeypatch):
    """Three epochs of impl.train.train (one batch each) with edge_dropout 0.3 from one seed: the TrainStep is captured and
    reports the per-op form; losses and parameters equal, bit for bit, those of a deep copy trained with eager launches; the
    mask of layer 0 at the stream's words is another one after every step."""
    from impl import SubGDataset, config, train, utils
    from glass_amd import losses, models, ops, stack, synth, train as gtrain
    config.set_device(0)
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=2, n_batches=1)
    x, ei, ew, pos, y = (torch.from_numpy(a).to(DEV) for a in (x, ei, ew, pos, y))
    torch.manual_seed(3)
    gnn = build_glass(64, 2, int(x.max()), w.n_class, "mean", w.pool, w.z_ratio, edge_dropout=0.3).to(DEV)
    twin = copy.deepcopy(gnn)
    loss_fn = nn.CrossEntropyLoss()
    ds = SubGDataset.GDataset(x, ei, ew, pos, y)
    loader = lambda: SubGDataset.ZGDataloader(ds, w.batch, z_fn=utils.MaxZOZ, shuffle=False, drop_last=True)
    out, masks = {}, {}
    for name, net, use_graph in (("graph", gnn, True), ("eager", twin, False)):
        monkeypatch.setattr(gtrain, "USE_GRAPH", use_graph)
        opt = torch.optim.Adam(net.parameters(), lr=5e-3)
        ops.rng_seed(DO.SEED, DEV)
        out[name], masks[name] = [], []
        for _ in range(3):
            out[name].append(train.train(opt, net, loader(), loss_fn))
            c = net.conv.convs[0]
            masks[name].append(ops.edge_keep_mask(c.adj, c.edge_dropout, c.call_base + 2).cpu())
        steps = net.__dict__.get("_glass_train_steps") or {}
        assert len(steps) == 1
        step = next(iter(steps.values()))
        net.train()
        assert step.graphed == use_graph and not step._program_step() and not stack.step_supported(net, loss_fn)
        assert not stack.StackProgram.supported(net.conv)
    print(f"edge dropout: losses {out['graph']}")
    assert np.isfinite(out["graph"]).all() and out["graph"][1] != out["graph"][0]
    assert np.array_equal(np.float32(out["graph"]).view(np.int32), np.float32(out["eager"]).view(np.int32)), out
    sd, sd2 = gnn.state_dict(), twin.state_dict()
    assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    for a, b in zip(masks["graph"], masks["eager"]):
        assert torch.equal(a, b)
    assert not torch.equal(masks["graph"][0], masks["graph"][1]) and not torch.equal(masks["graph"][1], masks["graph"][2])
    # the stack program declines the model only while a layer drops edges
    models.set_edge_dropout(gnn.conv, 0.0)
    assert stack.StackProgram.supported(gnn.conv) and stack.step_supported(gnn, losses.CrossEntropy())
