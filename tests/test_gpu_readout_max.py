"""Max pooling in the fused training readout on the GPU (glass_readout_max_train_f32; reference MaxPool,
impl/models.py:300-303, chosen by GLASSTest.py:162-167): the entry itself against the fp64 restatement
(tests/readout_max_oracle.py) through every launch form, whole models on the step program against the fp64 oracle and
against the product's own per-op path, and the reference's caller with MaxPool on the captured step."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.nn import CrossEntropyLoss
from torch.optim import Adam

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import readout_max_oracle as R  # noqa: E402
from helpers import build_glass, flat_grads, load, rel_inf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
EPS = 1e-5


def _align16(v):
    return (v + 15) & ~15


# (C, K, B, Smax, N, form): form = "" | "lab" (listed pooled rows: one-launch backfill) | "two" (+ gn_bwd_acc: two launches)
# C = 64: four columns per lane, 16 lanes per row slot, 16 slots -> Smax = 3 short loop, Smax = 40 > 2 * 16 unrolled loop + id
# stash; C = 17: scalar form (32 lanes per slot, 8 slots: Smax = 20 > 16); C = 1024 with Smax = 1700: the stash no longer fits
# 64 KiB (59 392 B + 4 * Smax), the unrolled loop reads pos from memory; 128 x 128 = 16 384 entries: the ordered scatter's
# limit, 130 x 128 beyond it (bucketed gather-add with scatter_ws)
CASES = [
    (64, 3, 40, 3, 300, ""), (64, 2, 40, 3, 300, "lab"), (64, 3, 40, 3, 300, "two"),
    (64, 2, 24, 40, 300, ""), (64, 3, 24, 40, 300, "two"),
    (17, 3, 40, 3, 300, ""), (17, 2, 24, 20, 300, ""),
    (1024, 3, 9, 1700, 400, "lab"),
    (64, 3, 128, 128, 300, ""), (64, 2, 128, 128, 300, "lab"), (64, 3, 128, 128, 300, "two"),
    (64, 3, 130, 128, 300, ""), (64, 2, 130, 128, 300, "lab"),
    # the scalar form beyond 256 columns: a thread's four slots take the columns c0 + 256 k.  (The parent commit pooled only
    # the first 256 columns there and computed everything else from uninitialised LDS: both cases fail on its library.)  C = 260 is
    # vector-capable and forced scalar by ldj = 261
    (258, 3, 40, 3, 300, ""), (260, 3, 40, 3, 300, ""),
]
LDJ = {260: 261}  # row stride of jk where it is not C


def _case_inputs(C, K, B, Smax, N, seed):
    g = torch.Generator().manual_seed(seed)
    jk = R.separated_columns(N, C, g).float()
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    gamma[0], gamma[1] = 0.7, -0.9                      # both signs for sure: the max is over y, not over the raw row
    beta, alpha = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    if Smax <= 8:
        pos = torch.stack([torch.randperm(N, generator=g)[:Smax] for _ in range(B)])
    else:
        pos = torch.randint(0, N, (B, Smax), generator=g)  # long rows: nodes repeat within a row and across rows
        pos[torch.rand(B, Smax, generator=g) < 0.2] = -1
    pos[1, :] = -1                                       # a row of all padding: pooled 0, no gradient
    pos[2, 0] = N + 5                                    # out-of-range ids
    pos[2, 1] = 1 << 40
    pos[3, 1] = pos[3, 0] = 7                            # a node listed twice in one row
    pos[4, 0] = pos[5, 0] = pos[6, 0] = 11               # a node shared by three subgraphs
    # an exact tie between two distinct nodes in column 0 (gamma[0] > 0): nodes 20 and 21 carry the column's largest raw
    # value, row 8 lists 20 at position 0 and 21 at position 2; node 21 is in no other row; node 22 (in no row at all) has
    # node 21's raw value in that column, so its d jk there is the dense part of node 21's
    big = jk[:, 0].max().item() + 1.0
    jk[20, 0] = jk[21, 0] = jk[22, 0] = big
    pos[pos == 21] = 23
    pos[pos == 22] = 23
    pos[8, 0], pos[8, 2] = 20, 21
    Wh, bh = torch.randn(K, C, generator=g) / C ** 0.5, torch.randn(K, generator=g)
    target = torch.randint(0, K, (B, ), generator=g) if K == 3 else (torch.rand(B, K, generator=g) > 0.5).float()
    return jk, gamma, beta, alpha, pos, Wh, bh, target, (0 if K == 3 else 1)


def _call(C, K, B, Smax, N, form, ins, stats_jk=None):
    """One call of glass_readout_max_train_f32 on fresh buffers; returns its outputs on the CPU.  stats_jk: the matrix the
    caller's GraphNorm statistics are taken from (default: jk itself)."""
    from glass_amd import _lib, stack
    from glass_amd.ops import _stream
    lib = _lib.load()
    jk, gamma, beta, alpha, pos, Wh, bh, target, loss_mode = ins
    mu, rstd = R.graphnorm_stats((jk if stats_jk is None else stats_jk).double(), alpha.double(), EPS)
    scale = (gamma.double() * rstd).float()
    shift = (beta.double() - scale.double() * alpha.double() * mu).float()
    saved = torch.cat([mu.float(), rstd.float(), scale, shift]).to(DEV)
    ldj = LDJ.get(C, C)
    jk_pad = torch.full((N, ldj), float("nan"))
    jk_pad[:, :C] = jk
    d = {k: v.to(DEV).contiguous() for k, v in dict(jk=jk_pad, gamma=gamma, alpha=alpha, pos=pos, Wh=Wh, bh=bh).items()}
    tgt = target.to(DEV).contiguous()
    f32 = dict(dtype=torch.float32, device=DEV)
    out = dict(pooled=torch.full((B, C), 7.0, **f32), logits=torch.full((B, K), 7.0, **f32), loss=torch.full((), 7.0, **f32),
               djk=torch.full((N, C), 7.0, **f32), dWh=torch.full((K, C), 7.0, **f32), dbh=torch.full((K, ), 7.0, **f32),
               dgamma=torch.full((C, ), 7.0, **f32), dbeta=torch.full((C, ), 7.0, **f32), dalpha=torch.full((C, ), 7.0, **f32))
    ws_bytes = lib.glass_readout_max_ws_bytes(B, C, K)
    ws = torch.zeros(ws_bytes // 8 + 1, dtype=torch.float64, device=DEV)
    one = torch.ones((), **f32)
    largs, labels = (0, 0, 0), None
    if form in ("lab", "two") or C % 4 or ldj % 4:
        labels = stack.BatchLabels(N, pos.numel(), DEV)
        labels.load(d["pos"])
        largs = (labels.mask.data_ptr(), labels.rows.data_ptr(), labels.count.data_ptr())
    acc = None
    if form == "two":
        acc = torch.zeros(int(lib.glass_gn_exact_words(C)), dtype=torch.int64, device=DEV)
    sws_bytes = int(lib.glass_readout_scatter_ws_bytes(N, B, Smax))
    assert (sws_bytes > 0) == (B * Smax > 16384)
    sws = torch.empty(sws_bytes + 16, dtype=torch.uint8, device=DEV) if sws_bytes else None
    rc = lib.glass_readout_max_train_f32(
        d["jk"].data_ptr(), ldj, saved.data_ptr(), d["gamma"].data_ptr(), d["alpha"].data_ptr(), d["pos"].data_ptr(), B, Smax,
        d["Wh"].data_ptr(), d["bh"].data_ptr(), tgt.data_ptr(), loss_mode, K, one.data_ptr(), out["pooled"].data_ptr(),
        out["logits"].data_ptr(), out["loss"].data_ptr(), out["djk"].data_ptr(), C, out["dWh"].data_ptr(), out["dbh"].data_ptr(), 0,
        out["dgamma"].data_ptr(), out["dbeta"].data_ptr(), out["dalpha"].data_ptr(), 0, ws.data_ptr(), N, C, *largs, 0,
        0 if acc is None else acc.data_ptr(), stack.REP_DENSE, 0 if sws is None else sws.data_ptr(), 0, _stream())
    assert rc == 0, lib.glass_last_error_string()
    torch.cuda.synchronize()
    off = _align16(8 * 2 * B * C + 4 * (4 * C + B * C + B * K + B))
    arg = ws.view(torch.uint8)[off:off + 4 * B * C].view(torch.int32).reshape(B, C)
    res = {k: v.cpu() for k, v in out.items()}
    res["arg"] = arg.cpu().to(torch.int64)
    res["saved"] = saved.cpu()
    return res


@pytest.mark.parametrize("C,K,B,Smax,N,form", CASES, ids=[f"C{c}_K{k}_B{b}_S{s}_{f or 'plain'}" for c, k, b, s, _n, f in CASES])
def test_max_readout_entry_vs_fp64_restatement(C, K, B, Smax, N, form):
    """The entry on its own: pooled / argmax positions / logits / loss / d jk / head and GraphNorm parameter gradients against
    the fp64 restatement at rel-inf <= 1e-5, through the launch form the case selects; an all-padding row, out-of-range ids,
    a node listed twice, a node shared by three subgraphs, negative gamma, and an exact tie between two distinct nodes whose
    gradient must land on the lower position alone; two calls give the same bits."""
    ins = _case_inputs(C, K, B, Smax, N, seed=1000 + C + Smax)
    jk, gamma, beta, alpha, pos, Wh, bh, target, loss_mode = ins
    want = R.readout_max(jk, gamma, beta, alpha, EPS, pos, Wh, bh, target, loss_mode)
    ok, gap = R.top_gap_ok(want["y"], torch.where(pos == 21, torch.full_like(pos, -1), pos), rel=1e-4)
    assert ok, gap  # (apart from the crafted exact tie no two distinct nodes are close: separated_columns, |gamma| >= 0.5)
    got = _call(C, K, B, Smax, N, form, ins)
    again = _call(C, K, B, Smax, N, form, ins)
    for k in got:
        assert torch.equal(got[k], again[k]), f"{k}: two calls on the same inputs differ"
    got.pop("saved")
    assert torch.equal(got["arg"], want["arg"])
    errs = {k: rel_inf(got[k], want[k]) for k in ("pooled", "logits", "loss", "djk")}
    keys = ("dWh", "dbh", "dgamma", "dbeta", "dalpha")
    errs["param_grads"] = rel_inf(flat_grads(got, keys), flat_grads(want, keys))
    print(f"max readout C={C} K={K} B={B} Smax={Smax} {form or 'plain'}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) +
          " | per tensor " + " ".join(f"{k} {rel_inf(got[k], want[k]):.2e}" for k in keys))
    assert all(v <= TOL for v in errs.values()), errs
    # the empty row
    assert bool((got["arg"][1] == -1).all()) and float(got["pooled"][1].abs().sum()) == 0.0
    # the crafted tie: position 0 (node 20) wins column 0 of row 8; node 21 gets the dense part alone there — bitwise what
    # node 22, in no row and with the same raw value, gets
    assert int(got["arg"][8, 0]) == 0
    assert got["djk"][21, 0].item() == got["djk"][22, 0].item()
    assert got["djk"][20, 0].item() != got["djk"][22, 0].item()


def test_max_readout_nan_takes_the_column_like_the_pooling_kernel():
    """NaNs in one column of jk at the nodes of two positions of one row that fall into different row slots (C = 64: 16
    slots; positions 5 and 18 are slots 5 and 2, so the slot fold meets the LATER NaN first), and at a third position in the
    first one's slot; statistics from the clean matrix.  pool.hip's rule: a NaN takes the column, the first NaN by position is
    the argmax and carries the gradient.  The argmax positions equal what glass_segment_pool_f32's max mode returns for the
    same y, in every row and column.  (The parent commit's compare `y > acc` dropped every NaN: the column pooled to its
    largest number; this test fails on its library.)"""
    from glass_amd import _lib
    from glass_amd.ops import _stream
    lib = _lib.load()
    C, K, B, Smax, N = 64, 3, 24, 40, 300
    ins = _case_inputs(C, K, B, Smax, N, seed=77)
    jk, gamma, beta, alpha, pos, Wh, bh, target, loss_mode = ins
    row, col = 10, 3
    pos[row, 5], pos[row, 18], pos[row, 21] = 250, 251, 252
    dirty = jk.clone()
    dirty[250, col] = dirty[251, col] = dirty[252, col] = float("nan")
    clean = _call(C, K, B, Smax, N, "", ins)
    got = _call(C, K, B, Smax, N, "", (dirty, ) + ins[1:], stats_jk=jk)
    assert int(got["arg"][row, col]) == 5 and bool(torch.isnan(got["pooled"][row, col]))
    # the pooling kernel on the same y (fp32 affine of the same saved scale | shift; the columns are separated, so one rounding
    # of y moves no argmax between numbers)
    scale, shift = got["saved"][2 * C:3 * C], got["saved"][3 * C:]
    y = (dirty * scale + shift).to(DEV).contiguous()
    posd = pos.to(DEV).contiguous()
    out = torch.empty(B, C, dtype=torch.float32, device=DEV)
    node = torch.full((B, C), -7, dtype=torch.int32, device=DEV)
    rc = lib.glass_segment_pool_f32(y.data_ptr(), C, posd.data_ptr(), B, Smax, _lib.POOL_MODES["max"], out.data_ptr(), C, node.data_ptr(),
                                    N, C, _stream())
    assert rc == 0, lib.glass_last_error_string()
    torch.cuda.synchronize()
    node = node.cpu().to(torch.int64)
    mine = torch.where(got["arg"] >= 0, pos.gather(1, got["arg"].clamp(min=0)), torch.full_like(got["arg"], -1))
    assert torch.equal(mine, node)
    # rows that name none of the three nodes keep their argmax; the NaN reaches d jk of node 250 in that column (the gradient's row)
    touched = ((pos == 250) | (pos == 251) | (pos == 252)).any(1)
    assert torch.equal(got["arg"][~touched], clean["arg"][~touched])
    hit = got["arg"][:, col] != clean["arg"][:, col]
    assert bool(hit[row]) and bool((got["arg"][:, :col] == clean["arg"][:, :col]).all()) and bool((got["arg"][:, col + 1:] == clean["arg"][:, col + 1:]).all())


# ---- model level -------------------------------------------------------------------------------------------------------
# seed of the model's weights per hidden width.  torch.manual_seed(hidden), the seed of test_model_outside_the_fused_family_vs_oracle,
# does not meet the gap condition below at any of these widths (smallest top-two gaps 1.7e-5 / 4.8e-6 / 1.1e-5 / 8.0e-5 of the
# column's max-abs at hidden 64 / 128 / 17 / 96); these are the first seeds counting up from `hidden` that do, found with
# the fp64 oracle on the CPU (gaps 1.7e-4 / 1.3e-4 / 2.4e-4 / 1.1e-4)
MODEL_SEEDS = {64: 72, 128: 266, 17: 18, 96: 202}


def _model_inputs():
    from glass_amd import synth
    n, K = 3000, 4
    ei, ew = synth.make_graph(n, 20000, 21, 0.4)
    x = synth.degree_feature(ei, n)
    pos, y = synth.make_subgraphs(n, 30, 12, K, 1, False)
    pos[2, 5:] = -1
    pos[4, :3] = pos[5, :3]
    return tuple(torch.from_numpy(a) for a in (ei, ew, x, pos, y)) + (K, )


@pytest.mark.parametrize("hidden", [64, 128, 17, 96])
def test_max_pool_model_runs_the_step_program_vs_oracle(hidden, monkeypatch):
    """A MaxPool model built by the factory on a parameter arena (N = 3 000, 30 ragged subgraphs, one emptied tail, shared
    nodes; hidden 64 staged family, 128 tiled, 17 narrow with the scalar readout, 96 zero-padded to 128): step_supported and
    covers_arena hold, stack.loss_and_grads equals the fp64 OracleGLASS(pool="max") on loss, logits and the flat gradient at
    1e-5, and equals the product's own per-op path on the same weights at the same tolerance.  Precondition, checked here from
    the oracle: in every (subgraph, column) the two largest GraphNorm outputs over distinct nodes differ by >= 1e-4 of the
    column's max-abs (a closer pair may legitimately change places between an fp32 and an fp64 evaluation)."""
    from glass_amd import stack, losses, widths
    from glass_amd.arena import ParamArena
    from impl import utils
    from oracle import glass_oracle as O
    ei, ew, x, pos, y, K = _model_inputs()
    torch.manual_seed(MODEL_SEEDS[hidden])
    model = build_glass(hidden, 2, int(x.max()), K, "mean", "max", 0.85)
    sd = {k: v.clone() for k, v in model.state_dict().items()}  # (logical shapes)
    orc = O.OracleGLASS(hidden, 2, int(x.max()), K, aggr="mean", pool="max", z_ratio=0.85)
    orc.load_state_dict(sd)
    orc = orc.double().train()
    z = O.max_zero_one(x, pos)
    with torch.no_grad():
        ok, gap = R.top_gap_ok(orc.node_emb(x, ei, ew.double(), z), pos, rel=1e-4)
    assert ok, f"hidden {hidden} seed {MODEL_SEEDS[hidden]}: top-two gap {gap:.2e} of the column's max-abs"
    po = orc(x, ei, ew.double(), pos, z)
    lo = nn.CrossEntropyLoss()(po, y)
    lo.backward()
    theirs = {k: p.grad for k, p in orc.named_parameters()}
    keys = sorted(theirs)

    def logical_grads():
        if hasattr(model, "_glass_logical_width"):
            g, pad_max = widths.logical_named_grads(model)
            assert pad_max == 0.0
        else:
            g = {k: p.grad for k, p in model.named_parameters()}
        return {k: v.detach().cpu().clone() for k, v in g.items()}

    model.to(DEV).train()
    arena = ParamArena(model)
    loss_fn = losses.CrossEntropy()
    assert stack.step_supported(model, loss_fn) and stack.covers_arena(model, arena)
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in (x, ei, ew, pos, y))
    loss, logits = stack.loss_and_grads(model, loss_fn, xg, eig, ewg, posg, "pos", yg, overwrite=True)
    torch.cuda.synchronize()
    mine = logical_grads()
    assert sorted(mine) == keys
    e = dict(logits=rel_inf(logits.cpu(), po.detach()), loss=abs(loss.item() - lo.item()) / abs(lo.item()),
             grad=rel_inf(flat_grads(mine, keys), flat_grads(theirs, keys)))
    # the product's per-op path (autograd tape over per-op kernels) on the same weights
    monkeypatch.setattr(stack, "USE_READOUT", False)
    assert not stack.step_supported(model, loss_fn)
    arena.zero()
    pred = model(xg, eig, ewg, posg, utils.MaxZOZ(xg, posg))
    loss_b = nn.CrossEntropyLoss()(pred, yg)
    loss_b.backward()
    torch.cuda.synchronize()
    perop = logical_grads()
    e2 = dict(logits=rel_inf(logits.cpu(), pred.detach().cpu()), loss=abs(loss.item() - loss_b.item()) / abs(loss_b.item()),
              grad=rel_inf(flat_grads(mine, keys), flat_grads(perop, keys)))
    print(f"max pool hidden {hidden}: gap {gap:.2e}; vs fp64 oracle {e}; vs per-op path {e2}")
    assert all(v < TOL for v in e.values()), e
    assert all(v < TOL for v in e2.values()), e2


# ---- caller level ------------------------------------------------------------------------------------------------------
def test_reference_caller_with_maxpool_lands_on_the_captured_step():
    """The g8-style tiny setup of tests/test_gpu_reference_caller.py with MaxPool: impl.train.train puts GLASSTest.py's own
    objects on the captured step program; three one-batch epochs equal an eager loop of the per-op path from the same state."""
    from test_gpu_reference_caller import reference_build_model, reference_loader, _eager_epoch, _taken_step
    from impl import SubGDataset, train, config
    config.set_device(0)
    g = load("g8_adam.npz")
    x = torch.from_numpy(g["x"]).to(DEV)
    ei, ew = torch.from_numpy(g["edge_index"]).to(DEV), torch.from_numpy(g["edge_weight"]).to(DEV)
    pos, y = torch.from_numpy(g["pos"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    torch.manual_seed(8)
    gnn = reference_build_model(int(g["hidden"]), int(g["layers"]), 0.0, True, "max", float(g["z_ratio"]), str(g["aggr"]),
                                torch.max(x), 3)
    twin = copy.deepcopy(gnn)
    optimizer, opt_twin = Adam(gnn.parameters(), lr=float(g["lr"])), Adam(twin.parameters(), lr=float(g["lr"]))
    loss_fn = CrossEntropyLoss()
    got, want = [], []
    for k in range(3):
        ds = SubGDataset.GDataset(x, ei, ew, pos[4 * k:4 * k + 4], y[4 * k:4 * k + 4])
        got.append(train.train(optimizer, gnn, reference_loader(ds, 4, shuffle=False), loss_fn))
        want.append(_eager_epoch(twin, opt_twin, reference_loader(ds, 4, shuffle=False), loss_fn))
    step = _taken_step(gnn)
    assert step.graphed and step._program_step(), "MaxPool caller not on the captured step program"
    print(f"MaxPool reference caller: losses {got} eager per-op {want}")
    assert np.allclose(got, want, rtol=1e-5, atol=0), (got, want)


def _probe(use_graph, steps=3):
    from glass_amd import synth, losses
    from glass_amd.arena import ParamArena
    from glass_amd.optim import FlatAdam
    from glass_amd.step import TrainStep
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=0, n_batches=3)
    ei, ew, x, pos, y = (torch.from_numpy(a).to(DEV) for a in (ei, ew, x, pos, y))
    pos[:, 0] = pos[0, 0]  # one node shared by every subgraph of a batch
    torch.manual_seed(0)
    model = build_glass(64, w.layers, int(x.max()), w.n_class, w.aggr, "max", w.z_ratio).to(DEV).train()
    arena = ParamArena(model)
    step = TrainStep(model, FlatAdam(arena, lr=1e-2), losses.CrossEntropy(), x, ei, ew, arena, use_graph=use_graph, warmup_iters=2,
                     preserve_state=True)
    B = w.batch
    seen = [step(pos[k * B:(k + 1) * B], y[k * B:(k + 1) * B]).clone() for k in range(steps)]
    torch.cuda.synchronize()
    assert step._program_step() and step.graphed == use_graph
    return torch.stack(seen), arena.flat_param.clone()


def test_max_pool_step_replay_equals_eager_bitwise():
    """Three training steps (fused Adam in the last launch) of a MaxPool model: the captured step replayed equals the same
    step program run eagerly, bit for bit, on losses and parameters."""
    l_graph, p_graph = _probe(True)
    l_eager, p_eager = _probe(False)
    assert torch.equal(l_graph, l_eager) and torch.equal(p_graph, p_eager)
    assert bool(torch.isfinite(l_graph).all()) and float(l_graph[0]) != float(l_graph[2])
