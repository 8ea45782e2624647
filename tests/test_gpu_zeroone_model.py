"""Exact zero-one labels through the model on the GPU (EmbZGConv with z [B, N], GLASS.Pool on [B, N, C]): logits against
the per-subgraph CPU oracle and against this model's own MaxZOZ path at batch size 1, batch independence bit for bit,
training gradients against CPU autograd through the oracle, the captured training step and the driver."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from helpers import rel_inf, build_glass, assert_grad_parity
from oracle import glass_oracle as O
import zeroone_oracle as ZO

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda:0"
_graph = {}


def _inputs():
    """(n, ei, ew, x, pos) on the host and on the GPU, made once."""
    if not _graph:
        host = ZO.graph(300, 0)
        _graph["host"] = host
        _graph["dev"] = (host[0], ) + tuple(t.to(DEV) for t in host[1:])
    return _graph["host"], _graph["dev"]


def _models(hidden, jk, pool, dropout=0.0, seed=0):
    """(oracle in fp64 or None for the attention pool, product model on the GPU) with the same parameters."""
    from impl import models
    torch.manual_seed(seed)
    base = "mean" if pool == "attn" else pool
    oracle = O.OracleGLASS(hidden, 2, 3, 3, aggr="mean", pool=base, z_ratio=0.8, dropout=0.0, jk=bool(jk))
    with torch.no_grad():  # (GraphNorm parameters away from their 1 / 0 / 1 start)
        for name, p in oracle.named_parameters():
            if "gn" in name:
                p.add_(torch.randn_like(p) * 0.2)
    model = build_glass(hidden, 2, 3, 3, "mean", base, 0.8, dropout=dropout, jk=bool(jk), pad_width=False)
    model.load_state_dict(oracle.state_dict())
    if pool == "attn":
        width = hidden * 2 if jk else hidden
        model.pools[0] = models.AttnPool(width)
        with torch.no_grad():
            model.pools[0].gate.weight.normal_(0, 0.3)
        oracle = None
    return (None if oracle is None else oracle.double()), model.to(DEV)


@pytest.mark.parametrize("pool", ["sum", "max", "attn"])
@pytest.mark.parametrize("jk", [0, 1])
@pytest.mark.parametrize("hidden", [64, 17])
def test_eval_logits_exact_and_batch_independent(hidden, jk, pool):
    from impl import utils
    (n, ei, ew, x, pos), (_n, eig, ewg, xg, posg) = _inputs()
    oracle, model = _models(hidden, jk, pool)
    model.eval()
    with torch.no_grad():
        z = utils.ZeroOneZ(xg, posg)
        got = model(xg, eig, ewg, posg, z)
        assert tuple(model.NodeEmb(xg, eig, ewg, z).shape)[:2] == (5, n)
        alone = torch.cat([model(xg, eig, ewg, posg[b:b + 1], utils.MaxZOZ(xg, posg[b:b + 1])) for b in range(5)])
        union = model(xg, eig, ewg, posg, utils.MaxZOZ(xg, posg))
        e_own = rel_inf(got.cpu(), alone.cpu())
        assert e_own <= TOL, e_own
        e_or = float("nan")
        if oracle is not None:
            want = ZO.logits(oracle, x, ei, ew.double(), pos)
            e_or = rel_inf(got.cpu(), want)
            assert e_or <= TOL, e_or
        print(f"zeroone eval hidden={hidden} jk={jk} pool={pool}: rel-inf vs oracle {e_or:.2e}, vs own batch-1 path {e_own:.2e}")
        # the labeled path of the union differs (adjacent / overlapping subgraphs see each other's marks)
        assert rel_inf(union.cpu(), got.cpu()) > 1e-4
        # batch independence, bit for bit: another composition and position ...
        perm = torch.tensor([3, 1, 4], device=DEV)
        other = model(xg, eig, ewg, posg[perm], utils.ZeroOneZ(xg, posg[perm]))
        assert torch.equal(other, got[perm])
        # ... and any grouping of the replicas
        for chunk in (1, 2):
            model.conv.replica_chunk = chunk
            assert torch.equal(model(xg, eig, ewg, posg, z), got), chunk
        model.conv.replica_chunk = None
        # a [1, N] z keeps today's path
        assert torch.equal(model(xg, eig, ewg, posg[:1], utils.ZeroOneZ(xg, posg[:1])), alone[:1])


@pytest.mark.parametrize("hidden", [64, 17])
def test_training_gradients_against_oracle_autograd(hidden):
    from impl import utils
    (n, ei, ew, x, pos), (_n, eig, ewg, xg, posg) = _inputs()
    oracle, model = _models(hidden, 1, "sum")
    y = torch.tensor([0, 2, 1, 1, 0])
    oracle.train()
    loss64 = nn.CrossEntropyLoss()(ZO.logits(oracle, x, ei, ew.double(), pos), y)
    loss64.backward()
    ref64 = {k: p.grad for k, p in oracle.named_parameters()}
    model.train()
    grads = {}
    for chunk in (None, 2):
        model.conv.replica_chunk = chunk
        model.zero_grad(set_to_none=True)
        loss = nn.CrossEntropyLoss()(model(xg, eig, ewg, posg, utils.ZeroOneZ(xg, posg)), y.to(DEV))
        loss.backward()
        assert abs(loss.item() - loss64.item()) <= TOL * abs(loss64.item())
        grads[chunk] = {k: p.grad.cpu() for k, p in model.named_parameters()}
    keys = sorted(ref64)
    assert sorted(grads[None]) == keys
    for k in keys:  # the grouping does not enter: every parameter gradient, bit for bit
        assert torch.equal(grads[None][k], grads[2][k]), k
    # biases right in front of a GraphNorm with mean_scale != 1 are NOT cancellation-defined here: every parameter is graded
    assert_grad_parity(grads[None], ref64, keys, TOL, label=f"zeroone hidden={hidden}")
    assert_grad_parity(grads[2], ref64, keys, TOL, label=f"zeroone hidden={hidden} replica_chunk=2")


@pytest.mark.parametrize("arena", [False, True])
def test_dropout_is_seeded_and_independent_of_the_grouping(arena):
    from impl import utils
    from glass_amd import ops
    _host, (_n, eig, ewg, xg, posg) = _inputs()
    _o, model = _models(64, 1, "sum", dropout=0.5)
    model.train()
    if arena:  # the fused dense path (stacked weight views, gradients into the arena)
        from glass_amd.arena import ParamArena
        bank = ParamArena(model)
        assert "comb" in model.conv.convs[0]._stack
    y = torch.tensor([0, 2, 1, 1, 0], device=DEV)
    runs = []
    for chunk in (None, None, 1, 2):
        model.conv.replica_chunk = chunk
        ops.rng_seed(1234, DEV)
        if arena:
            bank.zero()
        else:
            model.zero_grad(set_to_none=True)
        logits = model(xg, eig, ewg, posg, utils.ZeroOneZ(xg, posg))
        nn.CrossEntropyLoss()(logits, y).backward()
        runs.append((logits.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}))
    assert len(runs[0][1]) == 34 and all(g.abs().max() > 0 for g in runs[0][1].values())
    for other in runs[1:]:   # seeded: the same bits; and under any grouping: logits and EVERY parameter gradient, bit for bit
        assert torch.equal(other[0], runs[0][0])
        for k, g in runs[0][1].items():
            assert torch.equal(other[1][k], g), k
    model.eval()
    with torch.no_grad():
        assert not torch.equal(model(xg, eig, ewg, posg, utils.ZeroOneZ(xg, posg)), runs[0][0])  # dropout was on


def test_captured_train_step_over_zeroone_loader():
    """impl.train.train over ZGDataloader(z_fn=ZeroOneZ): the per-op step, captured; three steps, finite and repeatable."""
    from impl import SubGDataset, train, utils
    from glass_amd import ops, stack
    from glass_amd.step import TrainStep
    _host, (_n, eig, ewg, xg, posg) = _inputs()
    pos6 = torch.cat([posg, posg[:1]])
    y6 = torch.tensor([0, 2, 1, 1, 0, 2], device=DEV)
    losses = []
    for _ in range(2):
        _o, model = _models(64, 1, "sum", dropout=0.5, seed=3)
        ops.rng_seed(77, DEV)
        torch.manual_seed(5)
        ds = SubGDataset.GDataset(xg, eig, ewg, pos6, y6)
        loader = SubGDataset.ZGDataloader(ds, 2, z_fn=utils.ZeroOneZ, shuffle=False, drop_last=True)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        loss_fn = nn.CrossEntropyLoss()
        losses.append(train.train(opt, model, loader, loss_fn))
        step = next(iter(model.__dict__["_glass_train_steps"].values()))
        assert isinstance(step, TrainStep) and step.z_fn is utils.ZeroOneZ and step.graphed and not step._program_step()
    assert np.isfinite(losses[0]) and losses[0] == losses[1]


def test_driver_runs_with_use_zeroone(capsys):
    import GLASSTest
    GLASSTest.main(["--use_one", "--use_seed", "--use_zeroone", "--repeat", "1", "--device", "0", "--dataset", "density",
                    "--max_epoch", "2"])
    text = capsys.readouterr().out
    assert "use_zeroone=True" in text and "end: epoch" in text and "average " in text
