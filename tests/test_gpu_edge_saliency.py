"""Edge-weight gradients at model level: explain.edge_saliency of a 2-layer GLASS against the oracle model differentiated in fp64
by torch autograd on the CPU, explain.live_copy, explain.learn_edge_mask and GLASSTest.py --edge_saliency."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from helpers import build_glass, rel_inf
from oracle import glass_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5          # the project's model-level bound (README: rel-inf on the vector against the fp64 oracle)
N, B, S, K = 200, 6, 9, 3


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _graph():
    """A 200-node random directed graph (1 400 edges, weights in [0.5, 1.5), a few nodes without in-edges), a 6-clique planted
    on nodes 0..5, node features in 0..4, and a batch of 6 subgraphs of 5..9 nodes (padded with -1): the first three hold the
    clique (label 1), the others do not (label 0)."""
    rng = np.random.Generator(np.random.PCG64(7))
    src, dst = rng.integers(0, N, 1400), rng.integers(6, N - 4, 1400)        # (rows N-4.. have no in-edges: d~ = 1)
    cl = np.array([(a, b) for a in range(6) for b in range(6) if a != b]).T
    ei = np.concatenate((np.stack((dst, src)), cl), axis=1).astype(np.int64)
    ei = ei[:, rng.permutation(ei.shape[1])]
    w = rng.uniform(0.5, 1.5, ei.shape[1]).astype(np.float32)
    x = rng.integers(0, 5, (N, 1, 1)).astype(np.int64)
    pos = np.full((B, S), -1, dtype=np.int64)
    for b in range(B):
        if b < 3:
            k = int(rng.integers(0, S - 6 + 1))
            pos[b, :6] = np.arange(6)
            pos[b, 6:6 + k] = rng.choice(np.arange(6, N), k, replace=False)
        else:
            k = int(rng.integers(5, S + 1))
            pos[b, :k] = rng.choice(np.arange(6, N), k, replace=False)
    y = np.array([1, 1, 1, 0, 0, 0], dtype=np.int64)
    return tuple(torch.from_numpy(a) for a in (x, ei, w, pos, y))


def _models(hidden, aggr, pool, live=True, seed=0):
    """(the product model on the device in eval mode, its state_dict on the host)"""
    x = _graph()[0]
    torch.manual_seed(seed)
    model = build_glass(hidden, 2, int(x.max()), K, aggr, pool, 0.8, live_edge_weight=live)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    return model.to(DEV).eval(), sd


def _oracle_saliency(sd, hidden, aggr, pool, dtype, target=None, loss=False, detach_layer=None):
    """d (summed target logit, or the loss) / d edge_weight by torch autograd on the oracle model in `dtype`"""
    x, ei, w, pos, y = _graph()
    orc = O.OracleGLASS(hidden, 2, int(x.max()), K, aggr=aggr, pool=pool, z_ratio=0.8)
    orc.load_state_dict(sd)
    orc = orc.to(dtype).eval()
    wt = w.to(dtype).clone().requires_grad_()
    if detach_layer is not None:   # that layer's adjacency from constant weights
        orc.conv.convs[detach_layer].adj = O.build_adj(ei, w.to(dtype), N, aggr)
    logits = orc(x, ei, wt, pos, O.max_zero_one(x, pos))
    if loss:
        out = nn.CrossEntropyLoss()(logits, y)
    elif target is None:
        out = logits.gather(1, logits.detach().argmax(dim=1, keepdim=True)).sum()
    else:
        out = logits[:, target].sum()
    out.backward()
    return wt.grad.detach(), logits.detach()


def _dev_batch():
    from impl import utils
    x, ei, w, pos, y = (t.to(DEV) for t in _graph())
    return x, ei, w, pos, utils.MaxZOZ(x, pos), y


@pytest.mark.parametrize("pool", ("sum", "mean"))
@pytest.mark.parametrize("aggr", ("sum", "mean", "gcn"))
@pytest.mark.parametrize("hidden", (64, 8))
def test_saliency_against_the_oracle_model(hidden, aggr, pool):
    from glass_amd import explain
    model, sd = _models(hidden, aggr, pool)
    x, ei, w, pos, z, y = _dev_batch()
    for kw, okw in (({"target": 1}, {"target": 1}), ({}, {}), ({"loss_fn": nn.CrossEntropyLoss(), "y": y}, {"loss": True})):
        got = explain.edge_saliency(model, x, ei, w, pos, z, **kw)
        assert got.shape == w.shape and got.dtype == torch.float32 and got.device == w.device
        want, logits64 = _oracle_saliency(sd, hidden, aggr, pool, torch.float64, **okw)
        o32, logits32 = _oracle_saliency(sd, hidden, aggr, pool, torch.float32, **okw)
        if not kw:   # the argmax column must be the same column on both sides for the comparison to mean anything
            top = logits64.topk(2, dim=1).values
            assert float((top[:, 0] - top[:, 1]).min()) > 1e-3 * float(logits64.abs().max())
            assert torch.equal(logits32.argmax(1), logits64.argmax(1))
        err, err32 = rel_inf(got.cpu(), want), rel_inf(o32, want)
        print(f"hidden {hidden} {aggr} pool {pool} {sorted(kw) or ['argmax']}: saliency rel-inf {err:.2e} against the fp64 oracle "
              f"(the fp32 oracle on the CPU: {err32:.2e})")
        assert float(want.abs().max()) > 0 and err <= TOL, (hidden, aggr, pool, kw, err, err32)


@pytest.mark.parametrize("aggr", ("mean", "gcn"))
def test_the_gradient_accumulates_over_both_layers(aggr):
    from glass_amd import explain
    model, sd = _models(64, aggr, "sum")
    x, ei, w, pos, z, y = _dev_batch()
    full = explain.edge_saliency(model, x, ei, w, pos, z, target=1)
    layer2 = model.conv.convs[1]
    forward = layer2.forward                          # layer 2 sees the weights as constants from here on
    layer2.forward = lambda x_, ei_, ew_, mask, **kw: forward(x_, ei_, ew_.detach(), mask, **kw)
    part = explain.edge_saliency(model, x, ei, w, pos, z, target=1)
    want_full = _oracle_saliency(sd, 64, aggr, "sum", torch.float64, target=1)[0]
    want_part = _oracle_saliency(sd, 64, aggr, "sum", torch.float64, target=1, detach_layer=1)[0]
    assert rel_inf(want_part, want_full) > 1e-2, "the two layers' shares are both there"
    assert rel_inf(full.cpu(), want_full) <= TOL and rel_inf(part.cpu(), want_part) <= TOL
    assert rel_inf(part.cpu(), want_full) > 1e-2


@pytest.mark.parametrize("aggr", ("sum", "mean", "gcn"))
def test_live_copy_shares_parameters_and_leaves_the_model_alone(aggr):
    from glass_amd import explain, models
    model, _sd = _models(64, aggr, "mean", live=False)
    x, ei, w, pos, z, y = _dev_batch()
    with torch.no_grad():
        before = model(x, ei, w, pos, z)
    val = model.conv.convs[0].adj.fwd.val
    val_bits = _bits(val).clone()
    copy = explain.live_copy(model)
    assert copy is not model and isinstance(copy, models.GLASS) and not copy.training
    assert all(c.live_edge_weight for c in copy.conv.convs) and not any(c.live_edge_weight for c in model.conv.convs)
    mine, theirs = dict(model.named_parameters()), dict(copy.named_parameters())
    assert sorted(mine) == sorted(theirs) and all(mine[k].data_ptr() == theirs[k].data_ptr() for k in mine)
    assert sorted(model.state_dict()) == sorted(copy.state_dict())
    with torch.no_grad():
        assert torch.equal(_bits(copy(x, ei, w, pos, z)), _bits(before)), "live weights equal to the build-time ones: the same bits"
        other = copy(x, ei, w * 1.5 if aggr == "sum" else w * torch.linspace(0.5, 1.5, w.shape[0], device=DEV), pos, z)
        assert not torch.equal(_bits(other), _bits(before)), "the copy reads the weights of each call"
    g = explain.edge_saliency(model, x, ei, w, pos, z, target=0)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    with torch.no_grad():
        assert torch.equal(_bits(model(x, ei, w, pos, z)), _bits(before))
    assert model.conv.convs[0].adj.fwd.val is val and torch.equal(_bits(val), val_bits)
    assert all(p.grad is None for p in model.parameters()), "a saliency call leaves no parameter gradient behind"


def test_refusals():
    from glass_amd import explain, models, stack, losses
    for aggr in ("max", "softmax", "gat"):
        with pytest.raises(ValueError, match=aggr):
            build_glass(8, 2, 4, K, aggr, "sum", 0.8, live_edge_weight=True)
        with pytest.raises(ValueError, match=aggr):
            models.GLASSConv(8, 8, aggr=aggr, live_edge_weight=True)
    model, _sd = _models(64, "mean", "sum")
    x, ei, w, pos, z, y = _dev_batch()
    from impl import utils
    with pytest.raises(ValueError, match="replicated"):
        model(x, ei, w, pos, utils.ZeroOneZ(x, pos))
    with pytest.raises(ValueError, match="edge_weight"):
        explain.edge_saliency(model, x, ei, w[:-1], pos, z)
    # the stack program and the step program decline a live model, with an arena and in training mode as well
    from glass_amd.arena import ParamArena
    model.train()
    ParamArena(model)
    assert not stack.StackProgram.supported(model.conv) and not stack.step_supported(model, losses.CrossEntropy())
    plain, _sd = _models(64, "mean", "sum", live=False)
    plain.train()
    ParamArena(plain)
    assert stack.StackProgram.supported(plain.conv) and stack.step_supported(plain, losses.CrossEntropy())


def test_learn_edge_mask():
    from glass_amd import explain
    model, _sd = _models(64, "mean", "sum", live=False)
    batch = _dev_batch()
    mask, losses = explain.learn_edge_mask(model, batch, steps=5, lr=0.05, l1=0.01, seed=3, return_losses=True)
    assert mask.shape == batch[2].shape and bool((mask > 0).all()) and bool((mask < 1).all())
    assert len(losses) == 5 and losses[-1] < losses[0], losses
    again = explain.learn_edge_mask(model, batch, steps=5, lr=0.05, l1=0.01, seed=3)
    assert torch.equal(_bits(mask), _bits(again)), "two runs with one seed"
    other = explain.learn_edge_mask(model, batch, steps=5, lr=0.05, l1=0.01, seed=4)
    assert not torch.equal(_bits(mask), _bits(other))
    assert all(p.requires_grad for p in model.parameters()) and all(p.grad is None for p in model.parameters())


def test_driver_writes_the_saliency_file(tmp_path):
    path = tmp_path / "saliency.npy"
    cmd = [sys.executable, os.path.join(ROOT, "GLASSTest.py"), "--use_one", "--use_seed", "--use_maxzeroone", "--repeat", "1",
           "--device", "0", "--dataset", "synthetic:tiny", "--max_epoch", "3", "--edge_saliency", str(path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    import datasets
    E = datasets.load_dataset("synthetic:tiny").edge_index.shape[1]
    s = np.load(path)
    assert s.shape == (E, ) and s.dtype == np.float32 and bool(np.isfinite(s).all()) and bool((s >= 0).all()) and float(s.max()) > 0
    for bad in (["--aggr", "max"], ["--aggr", "gat"], ["--use_zeroone"]):
        args = [a for a in cmd if a != "--use_maxzeroone"] if bad == ["--use_zeroone"] else cmd
        import GLASSTest
        with pytest.raises(SystemExit):
            GLASSTest.parse_args(args[2:] + bad)
