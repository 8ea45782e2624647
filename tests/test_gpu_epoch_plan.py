"""The epoch plan of the step's head launch (glass_epoch_plan_build, glass_batch_cursor.plan): every batch's unique labeled
rows listed once per epoch, the head launch of a replayed step copies its batch's record instead of electing the rows.
Everything here is exact: the plan's lists against the per-step label launch, the label state the head launch leaves with
and without the plan, and the captured training step with the plan against the same step with the plan forced off.
(The plan holds the labeled-row lists only; the readout's per-subgraph ids and its backfill lists are derived per step, with
or without it, so there is nothing of theirs to compare.)"""
import functools

import numpy as np
import pytest
import torch

from helpers import build_glass

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, N_B, B, SMAX = 300, 5, 4, 6


def _epoch(seed):
    """5 batches of 4 subgraphs x 6 slots over 300 nodes, as data set rows + a permutation cut into batches.  Rows (in data set
    order; the permutation scatters them): padding, an id >= N, a node twice in one subgraph, a node in two subgraphs of a
    batch, a node in consecutive batches, an empty subgraph."""
    rng = np.random.default_rng(seed)
    pos = np.stack([rng.choice(N, SMAX, replace=False) for _ in range(N_B * B)]).astype(np.int64)
    perm = rng.permutation(N_B * B).astype(np.int64).reshape(N_B, B)
    row = lambda b, s: int(perm[b, s])  # noqa: E731
    pos[row(0, 0), 4:] = -1                            # padding
    pos[row(0, 1), 2] = N + 7                          # out of range
    pos[row(1, 0), 5] = pos[row(1, 0), 1]              # twice in one subgraph
    pos[row(1, 2), 0] = pos[row(1, 1), 3]              # shared by two subgraphs of a batch
    pos[row(2, 1), 2] = pos[row(1, 3), 4]              # shared by consecutive batches
    pos[row(0, 2), 1] = pos[row(N_B - 1, 0), 0]        # ... and by the last batch and batch 0 (the wrap)
    pos[row(3, 3), :] = -1                             # an empty subgraph
    y = rng.integers(0, 3, (N_B * B, )).astype(np.int64)
    dev = torch.device(DEV)
    return torch.from_numpy(pos).to(dev), torch.from_numpy(y).to(dev), torch.from_numpy(perm).to(dev)


def _head(lib, labels):
    st = torch.cuda.current_stream().cuda_stream
    rc = lib.glass_step_head_f32(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0, 0, 0, *labels.head_args(), st)
    assert rc == 0, lib.glass_last_error_string()
    torch.cuda.synchronize()


def _plan_records(labels):
    stride = 4 + (B * SMAX + 3) // 4 * 4
    rec = labels._plan[:N_B * stride].reshape(N_B, stride).cpu()
    return [(int(r[0]), r[4:4 + int(r[0])].clone()) for r in rec]


def test_plan_lists_and_label_state_equal_the_per_step_launch():
    """For every batch of the epoch: the plan's record == rows / count of glass_batch_labels_gather on the same batch; the head
    launch with the plan leaves label bytes, list, count, batch and targets identical to the head launch without it (and to
    the eager launch), over 1.4 epochs so that the wrap from the last batch to batch 0 is walked; the owner words stay
    untouched; a second epoch with another permutation is planned into the same buffer."""
    from glass_amd import stack, _lib
    lib = _lib.load()
    dev = torch.device(DEV)
    a, b, c = (stack.BatchLabels(N, B * SMAX, dev) for _ in range(3))   # eager launch | head without plan | head with plan
    pa, pb, pc = (torch.full((B, SMAX), -1, dtype=torch.int64, device=dev) for _ in range(3))
    ya, yb, yc = (torch.zeros((B, ), dtype=torch.int64, device=dev) for _ in range(3))
    plan_ptr = None
    for seed in (11, 12):
        pos_all, y_all, idx = _epoch(seed)
        b.set_epoch(pos_all, y_all, idx, pb, yb, wrap=True)
        c.set_epoch(pos_all, y_all, idx, pc, yc, wrap=True, plan=True)
        torch.cuda.synchronize()
        assert b.plan_bytes == 0 and int(b.cursor[7]) == 0
        assert c.plan_bytes == lib.glass_epoch_plan_bytes(N_B, B, SMAX) > 0 and int(c.cursor[7]) == c._plan.data_ptr()
        assert plan_ptr in (None, c._plan.data_ptr()), "the second epoch's plan went to another buffer"
        plan_ptr = c._plan.data_ptr()
        assert torch.equal(c._plan_ws, torch.full_like(c._plan_ws, 2**31 - 1))
        records = _plan_records(c)
        for k in range(N_B + 2):  # 0 .. 4, then the wrap: 0, 1
            a.load_gather(pos_all, y_all, idx[k % N_B], pa, ya)
            _head(lib, b)
            _head(lib, c)
            na = int(a.count[0])
            assert records[k % N_B][0] == na and torch.equal(records[k % N_B][1], a.rows[:na].cpu())
            assert int(b.count[0]) == na and int(c.count[0]) == na
            assert torch.equal(a.rows[:na], c.rows[:na]) and torch.equal(b.rows[:na], c.rows[:na])
            assert torch.equal(a.mask, c.mask) and torch.equal(b.mask, c.mask)
            z = torch.zeros(N, dtype=torch.uint8, device=dev)
            cur = pos_all[idx[k % N_B]].flatten()
            z[cur[(cur >= 0) & (cur < N)]] = 1
            assert torch.equal(c.mask, z)
            assert torch.equal(pa, pc) and torch.equal(ya, yc) and torch.equal(pb, pc) and torch.equal(yb, yc)
            assert int(c.cursor[5]) == k + 1
            assert torch.equal(c.ws, torch.full_like(c.ws, 2**31 - 1))
    # first-occurrence order, checked once against the definition (not only against the other kernel)
    cur = pos_all[idx[1]].flatten().cpu().tolist()
    seen = []
    for p in cur:
        if 0 <= p < N and p not in seen:
            seen.append(p)
    assert records[1][1].tolist() == seen


def test_plan_build_refuses_bad_arguments():
    from glass_amd import _lib
    lib = _lib.load()
    p = torch.zeros(64, dtype=torch.int64, device=DEV).data_ptr()
    assert lib.glass_epoch_plan_bytes(0, 4, 6) < 0 and lib.glass_epoch_plan_bytes(5, 4, 6) == 5 * 28 * 4
    assert lib.glass_epoch_plan_build(p, 20, 6, p, 5, 4, N, None, 560, p, 1, None) == -1
    assert lib.glass_epoch_plan_build(p, 20, 6, p, 5, 4, N, p, 556, p, 1, None) == -1      # plan too small
    assert lib.glass_epoch_plan_build(p, 20, 6, p, 5, 4, N, p, 560, p, 0, None) == -1      # no lane of owner words


@functools.lru_cache(maxsize=None)
def _run(pool, clip, plan, cap=None):
    """12 captured steps (hidden 64, 2 layers, N = 300, dropout 0.5, seeded) over 4 cycling batches with a node shared by every
    subgraph -> (losses, gradient arena, parameters, bytes of the installed plan)."""
    from glass_amd import synth, losses, ops, stack
    from glass_amd.arena import ParamArena
    from glass_amd.optim import FlatAdam
    from glass_amd.step import TrainStep
    dev = torch.device(DEV)
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=0, n_batches=4)
    ei, ew, x, pos, y = (torch.from_numpy(v).to(dev) for v in (ei, ew, x, pos, y))
    pos[:, 0] = pos[0, 0]
    pos[5, 3:] = -1
    torch.manual_seed(0)
    ops.rng_seed(321, dev)
    model = build_glass(64, 2, int(x.max()), w.n_class, w.aggr, pool, w.z_ratio, dropout=0.5).to(dev).train()
    arena = ParamArena(model)
    opt = FlatAdam(arena, lr=1e-2, max_grad_norm=0.05 if clip else None)
    step = TrainStep(model, opt, losses.CrossEntropy(), x, ei, ew, arena, use_graph=True, warmup_iters=2, preserve_state=True)
    step.epoch_plan = plan
    old_cap = stack.EPOCH_PLAN_MAX_BYTES
    if cap is not None:
        stack.EPOCH_PLAN_MAX_BYTES = cap
    try:
        idx = torch.arange(4 * w.batch, device=dev).reshape(4, w.batch)
        assert step.begin_epoch(pos, y, idx, wrap=True), "the step program did not take the head-label form"
        seen = [step.next_step().clone() for _ in range(12)]
    finally:
        stack.EPOCH_PLAN_MAX_BYTES = old_cap
    torch.cuda.synchronize()
    assert step.graphed and step._labels.in_head and int(step._labels.cursor[5]) == 12
    return torch.stack(seen), arena.flat.clone(), arena.flat_param.clone(), step._labels.plan_bytes


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("pool", ["sum", "max"])
def test_captured_steps_with_the_plan_equal_the_steps_without(pool, clip):
    off, on = _run(pool, clip, False), _run(pool, clip, True)
    assert off[3] == 0 and on[3] > 0
    for name, u, v in zip(("loss", "gradients", "parameters"), off, on):
        assert torch.equal(u, v), name
    assert float(off[0].std()) > 0  # (the twelve losses differ: the steps did train)


def test_a_plan_above_the_cap_leaves_the_per_step_path():
    off, capped = _run("sum", False, False), _run("sum", False, True, 0)
    assert capped[3] == 0, "a plan was installed although the cap is 0 bytes"
    for name, u, v in zip(("loss", "gradients", "parameters"), off, capped):
        assert torch.equal(u, v), name
