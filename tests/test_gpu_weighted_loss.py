"""Class-weighted losses on the GPU: the `_w` entries of the two fused heads and of the training readout against the fp64
restatement (tests/weighted_loss_oracle.py; rel-inf <= 1e-5 on loss, logits and every gradient), their bitwise identity with
the unweighted entries under two null pointers, and the model paths: the captured TrainStep, stack.loss_and_grads, the per-op
autograd path with the fused head, the eager per-batch loop, and GNN-seg's loss_and_logits."""
import pytest
import torch
import torch.nn as nn

import readout_max_oracle as R
import weighted_loss_oracle as WO
from helpers import build_glass, flat_grads, rel_inf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
EPS = 1e-5
KBLOCK = 256  # workgroup size of the loss kernels (common.h): B = KBLOCK + 1 reaches the ordered sums' second round and tree
ACT_ELU = 1


def _weights(kind, K, g):
    if kind == "wide":
        return torch.logspace(-3, 3, K)[torch.randperm(K, generator=g)] if K > 1 else torch.tensor([1e3])
    return 0.25 + 3.0 * torch.rand(K, generator=g)


def _head_inputs(mode, K, B, kind, seed, absent=False):
    g = torch.Generator().manual_seed(seed)
    C, Hd = 40, 24
    d = dict(pooled=torch.randn(B, C, generator=g), W=torch.randn(K, C, generator=g) / C ** 0.5, b=0.3 * torch.randn(K, generator=g),
             W1=torch.randn(Hd, C, generator=g) / C ** 0.5, b1=0.3 * torch.randn(Hd, generator=g),
             W2=torch.randn(K, Hd, generator=g) / Hd ** 0.5, b2=0.3 * torch.randn(K, generator=g))
    if mode == 0:
        t = torch.randint(0, K, (B, ), generator=g)
        if absent:
            t[t == 1] = 0          # class 1 occurs nowhere in the batch: its weight must not reach the denominator
    else:
        t = (torch.rand(B, K, generator=g) > 0.5).float()
    return d, t, _weights(kind, K, g)


def _oracle_head(d, t, mode, w, mlp, gl):
    p = {k: v.double().clone().requires_grad_(True) for k, v in d.items()}
    if mlp:
        logits = nn.functional.elu(p["pooled"] @ p["W1"].t() + p["b1"]) @ p["W2"].t() + p["b2"]
        keys = ("pooled", "W1", "b1", "W2", "b2")
    else:
        logits = p["pooled"] @ p["W"].t() + p["b"]
        keys = ("pooled", "W", "b")
    loss = WO.loss(logits, t, mode, w if mode == 0 else None, w if mode == 1 else None)
    grads = torch.autograd.grad(loss * gl, [p[k] for k in keys])
    return dict(loss=loss.detach(), logits=logits.detach(), **{"d" + k: g for k, g in zip(keys, grads)})


def _run_head(d, t, mode, w, mlp, gl, old=False):
    """One forward + backward through the head entries on fresh buffers (old: the unweighted entries; w None with the `_w`
    entries: two null pointers)."""
    from glass_amd import _lib
    from glass_amd.ops import _stream
    lib = _lib.load()
    dv = {k: v.to(DEV).contiguous() for k, v in d.items()}
    B, C = d["pooled"].shape
    K, Hd = d["W"].shape[0], d["W1"].shape[0]
    tgt = t.to(DEV).contiguous()
    f32 = dict(dtype=torch.float32, device=DEV)
    wd = None if w is None else w.to(DEV).contiguous()
    wargs = () if old else ((wd.data_ptr() if (wd is not None and mode == 0) else 0), (wd.data_ptr() if (wd is not None and mode == 1) else 0))
    logits, prob, loss = torch.full((B, K), 7.0, **f32), torch.full((B * K + B, ), 7.0, **f32), torch.full((), 7.0, **f32)
    glt, dpooled = torch.tensor(gl, **f32), torch.full((B, C), 7.0, **f32)
    sfx = "_f32" if old else "_w_f32"
    if not mlp:
        dW, db = torch.full((K, C), 7.0, **f32), torch.full((K, ), 7.0, **f32)
        rc = getattr(lib, "glass_head_loss_fwd" + sfx)(dv["pooled"].data_ptr(), C, dv["W"].data_ptr(), dv["b"].data_ptr(),
                                                       tgt.data_ptr(), mode, B, C, K, logits.data_ptr(), prob.data_ptr(),
                                                       loss.data_ptr(), *wargs, _stream())
        assert rc == 0, lib.glass_last_error_string()
        rc = getattr(lib, "glass_head_loss_bwd" + sfx)(dv["pooled"].data_ptr(), C, dv["W"].data_ptr(), prob.data_ptr(),
                                                       tgt.data_ptr(), mode, glt.data_ptr(), B, C, K, dpooled.data_ptr(), C,
                                                       dW.data_ptr(), db.data_ptr(), 0, *wargs, _stream())
        assert rc == 0, lib.glass_last_error_string()
        out = dict(loss=loss, logits=logits, dpooled=dpooled, dW=dW, db=db)
    else:
        hidden, ws = torch.full((B, Hd), 7.0, **f32), torch.full((2 * B * Hd, ), 7.0, **f32)
        g = [torch.full((Hd, C), 7.0, **f32), torch.full((Hd, ), 7.0, **f32), torch.full((K, Hd), 7.0, **f32), torch.full((K, ), 7.0, **f32)]
        rc = getattr(lib, "glass_head_mlp_loss_fwd" + sfx)(dv["pooled"].data_ptr(), C, dv["W1"].data_ptr(), dv["b1"].data_ptr(),
                                                           dv["W2"].data_ptr(), dv["b2"].data_ptr(), tgt.data_ptr(), mode, ACT_ELU,
                                                           0.0, 0, 3, B, C, Hd, K, hidden.data_ptr(), logits.data_ptr(),
                                                           prob.data_ptr(), loss.data_ptr(), *wargs, _stream())
        assert rc == 0, lib.glass_last_error_string()
        rc = getattr(lib, "glass_head_mlp_loss_bwd" + sfx)(dv["pooled"].data_ptr(), C, dv["W1"].data_ptr(), dv["W2"].data_ptr(),
                                                           hidden.data_ptr(), prob.data_ptr(), tgt.data_ptr(), mode, ACT_ELU, 0.0, 0,
                                                           3, glt.data_ptr(), B, C, Hd, K, ws.data_ptr(), dpooled.data_ptr(), C,
                                                           *(x.data_ptr() for x in g), 0, *wargs, _stream())
        assert rc == 0, lib.glass_last_error_string()
        out = dict(loss=loss, logits=logits, dpooled=dpooled, dW1=g[0], db1=g[1], dW2=g[2], db2=g[3])
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _check(got, want, label):
    errs = {k: rel_inf(got[k], want[k]) for k in want}
    print(label + ": " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), (label, errs)


HEAD_CASES = ([(0, K, B, "plain", False) for K in (2, 3, 256) for B in (1, 5, KBLOCK + 1)] +
              [(1, K, B, "plain", False) for K in (1, 4, 256) for B in (1, 5, KBLOCK + 1)] +
              [(0, 3, 5, "plain", True), (0, 3, KBLOCK + 1, "wide", False), (0, 256, 5, "wide", False), (1, 4, 5, "wide", False)])


@pytest.mark.parametrize("mlp", [False, True], ids=["linear", "mlp"])
@pytest.mark.parametrize("mode,K,B,kind,absent", HEAD_CASES,
                         ids=[f"{'ce' if m == 0 else 'bce'}_K{k}_B{b}_{kind}{'_absent' if a else ''}" for m, k, b, kind, a in HEAD_CASES])
def test_head_entries_vs_fp64_restatement(mode, K, B, kind, absent, mlp):
    """glass_head_loss_*_w_f32 / glass_head_mlp_loss_*_w_f32: loss, logits, dpooled and every parameter gradient; grad_loss
    0.37 (not 1) so that the scale reaches the check; two calls give the same bits."""
    d, t, w = _head_inputs(mode, K, B, kind, seed=100 * K + B + mode)
    if absent:
        d, t, w = _head_inputs(mode, K, B, kind, seed=7, absent=True)
        assert not bool((t == 1).any())
    want = _oracle_head(d, t, mode, w, mlp, 0.37)
    got = _run_head(d, t, mode, w, mlp, 0.37)
    again = _run_head(d, t, mode, w, mlp, 0.37)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    _check(got, want, f"{'mlp' if mlp else 'linear'} head mode {mode} K={K} B={B} {kind}")
    if B > 1:
        plain = _oracle_head(d, t, mode, None, mlp, 0.37)
        assert abs(float(plain["loss"]) - float(want["loss"])) > 1e-3 * abs(float(want["loss"]))  # (the weights matter here)


@pytest.mark.parametrize("mlp", [False, True], ids=["linear", "mlp"])
@pytest.mark.parametrize("mode,K,B", [(0, 3, 5), (1, 4, KBLOCK + 1)])
def test_head_entries_with_null_weights_equal_the_old_entries_bitwise(mode, K, B, mlp):
    d, t, _w = _head_inputs(mode, K, B, "plain", seed=5)
    new, old = _run_head(d, t, mode, None, mlp, 0.37), _run_head(d, t, mode, None, mlp, 0.37, old=True)
    for k in old:
        assert torch.equal(new[k], old[k]), k


# ---- fused readout ---------------------------------------------------------------------------------------------------------
def _readout_inputs(K, seed):
    g = torch.Generator().manual_seed(seed)
    N, C, B, Smax = 300, 64, 5, 9
    jk = R.separated_columns(N, C, g).float()
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    beta, alpha = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    pos = torch.stack([torch.randperm(N, generator=g)[:Smax] for _ in range(B)])
    for b, n in enumerate((9, 4, 7, 1, 6)):          # ragged rows, padding -1
        pos[b, n:] = -1
    pos[2, 0] = pos[4, 0] = 11                        # a node shared by two subgraphs
    Wh, bh = torch.randn(K, C, generator=g) / C ** 0.5, torch.randn(K, generator=g)
    mode = 0 if K == 3 else 1
    target = torch.randint(0, K, (B, ), generator=g) if mode == 0 else (torch.rand(B, K, generator=g) > 0.5).float()
    return dict(jk=jk, gamma=gamma, beta=beta, alpha=alpha, pos=pos, Wh=Wh, bh=bh, target=target, mode=mode,
                w=_weights("plain", K, g))


def _oracle_readout(ins, pool, w):
    jk, gamma, beta, alpha, Wh, bh = (ins[k].double().clone().requires_grad_(True) for k in ("jk", "gamma", "beta", "alpha", "Wh", "bh"))
    pos, mode = ins["pos"], ins["mode"]
    N, C = jk.shape
    mu, rstd = R.graphnorm_stats(jk, alpha, EPS)
    y = gamma * ((jk - alpha * mu) * rstd) + beta
    valid = ((pos >= 0) & (pos < N)).double().unsqueeze(-1)
    rows = y[pos.clamp(0, N - 1)]                      # [B, S, C]
    cnt = valid.sum(dim=1)
    if pool == "max":
        arg = R.readout_max(ins["jk"], ins["gamma"], ins["beta"], ins["alpha"], EPS, pos, ins["Wh"], ins["bh"], ins["target"], mode)["arg"]
        pooled = rows.gather(1, arg.clamp(min=0).unsqueeze(1)).squeeze(1) * (arg >= 0)
    else:
        s = (rows * valid).sum(dim=1)
        pooled = s if pool == "sum" else s / cnt.clamp(min=1) if pool == "mean" else s / cnt.clamp(min=1).sqrt()
    logits = pooled @ Wh.t() + bh
    loss = WO.loss(logits, ins["target"], mode, w if mode == 0 else None, w if mode == 1 else None)
    djk, dWh, dbh = torch.autograd.grad(loss, [jk, Wh, bh])
    return dict(loss=loss.detach(), logits=logits.detach(), djk=djk, dWh=dWh, dbh=dbh)


def _run_readout(ins, pool, w, form, old=False):
    from glass_amd import _lib, stack
    from glass_amd.ops import _stream
    lib = _lib.load()
    mx, mode = pool == "max", ins["mode"]
    N, C = ins["jk"].shape
    B, Smax = ins["pos"].shape
    K = ins["Wh"].shape[0]
    mu, rstd = R.graphnorm_stats(ins["jk"].double(), ins["alpha"].double(), EPS)
    scale = (ins["gamma"].double() * rstd).float()
    shift = (ins["beta"].double() - scale.double() * ins["alpha"].double() * mu).float()
    saved = torch.cat([mu.float(), rstd.float(), scale, shift]).to(DEV)
    d = {k: ins[k].to(DEV).contiguous() for k in ("jk", "gamma", "alpha", "pos", "Wh", "bh", "target")}
    f32 = dict(dtype=torch.float32, device=DEV)
    out = dict(pooled=torch.full((B, C), 7.0, **f32), logits=torch.full((B, K), 7.0, **f32), loss=torch.full((), 7.0, **f32),
               djk=torch.full((N, C), 7.0, **f32), dWh=torch.full((K, C), 7.0, **f32), dbh=torch.full((K, ), 7.0, **f32),
               dgamma=torch.full((C, ), 7.0, **f32), dbeta=torch.full((C, ), 7.0, **f32), dalpha=torch.full((C, ), 7.0, **f32))
    ws_bytes = lib.glass_readout_max_ws_bytes(B, C, K) if mx else lib.glass_readout_ws_bytes(B, C, K)
    ws = torch.zeros(ws_bytes // 8 + 1, dtype=torch.float64, device=DEV)
    one = torch.ones((), **f32)
    labels = stack.BatchLabels(N, d["pos"].numel(), DEV)   # the listed pooled rows: the one-launch backfill behind the reduce launch
    labels.load(d["pos"])
    acc = torch.zeros(int(lib.glass_gn_exact_words(C)), dtype=torch.int64, device=DEV) if form == "two" else None
    wd = None if w is None else w.to(DEV).contiguous()
    wargs = () if old else ((wd.data_ptr() if (wd is not None and mode == 0) else 0), (wd.data_ptr() if (wd is not None and mode == 1) else 0))
    name = "glass_readout_" + ("max_" if mx else "") + "train" + ("_f32" if old else "_w_f32")
    mode_arg = () if mx else (_lib.POOL_MODES[pool], )
    rc = getattr(lib, name)(
        d["jk"].data_ptr(), C, saved.data_ptr(), d["gamma"].data_ptr(), d["alpha"].data_ptr(), d["pos"].data_ptr(), B, Smax, *mode_arg,
        d["Wh"].data_ptr(), d["bh"].data_ptr(), d["target"].data_ptr(), mode, K, one.data_ptr(), out["pooled"].data_ptr(),
        out["logits"].data_ptr(), out["loss"].data_ptr(), out["djk"].data_ptr(), C, out["dWh"].data_ptr(), out["dbh"].data_ptr(), 0,
        out["dgamma"].data_ptr(), out["dbeta"].data_ptr(), out["dalpha"].data_ptr(), 0, ws.data_ptr(), N, C, labels.mask.data_ptr(),
        labels.rows.data_ptr(), labels.count.data_ptr(), 0, 0 if acc is None else acc.data_ptr(), stack.REP_DENSE, 0, 0, *wargs,
        _stream())
    assert rc == 0, lib.glass_last_error_string()
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("form", ["one", "two"])
@pytest.mark.parametrize("K", [3, 4], ids=["ce_K3", "bce_K4"])
@pytest.mark.parametrize("pool", ["sum", "mean", "size", "max"])
def test_readout_entries_vs_fp64_restatement(pool, K, form):
    """glass_readout_train_w_f32 / glass_readout_max_train_w_f32 (B = 5 ragged rows, N = 300, C = 64): loss, logits, d jk, dWh,
    dbh — the mean through the reduce launch ("one": its mean role, then the one-launch backfill) and through the two-launch
    finish ("two": the backfill's mean role); two calls give the same bits."""
    ins = _readout_inputs(K, seed=40 + K)
    want = _oracle_readout(ins, pool, ins["w"])
    got = _run_readout(ins, pool, ins["w"], form)
    again = _run_readout(ins, pool, ins["w"], form)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    _check({k: got[k] for k in want}, want, f"readout {pool} K={K} {form}")
    plain = _oracle_readout(ins, pool, None)
    assert abs(float(plain["loss"]) - float(want["loss"])) > 1e-3 * abs(float(want["loss"]))


@pytest.mark.parametrize("form", ["one", "two"])
@pytest.mark.parametrize("pool,K", [("size", 3), ("max", 4)])
def test_readout_entries_with_null_weights_equal_the_old_entries_bitwise(pool, K, form):
    ins = _readout_inputs(K, seed=40 + K)
    new, old = _run_readout(ins, pool, None, form), _run_readout(ins, pool, None, form, old=True)
    for k in old:
        assert torch.equal(new[k], old[k]), k


# ---- whole model -----------------------------------------------------------------------------------------------------------
_MODEL = {}


def _model_case(hidden):
    """A ~300-node graph, 6 subgraphs, 3 classes, 2 layers; the fp64 oracle's weighted loss and gradients (computed once)."""
    if hidden not in _MODEL:
        from glass_amd import synth
        from oracle import glass_oracle as O
        n, K = 300, 3
        ei, ew = synth.make_graph(n, 2000, 21, 0.4)
        x = synth.degree_feature(ei, n)
        pos, y = synth.make_subgraphs(n, 6, 8, K, 1, False)
        ei, ew, x, pos, y = (torch.from_numpy(a) for a in (ei, ew, x, pos, y))
        pos[2, 5:] = -1
        y[:] = torch.tensor([0, 1, 2, 0, 0, 1])
        w = torch.tensor([0.5, 2.0, 3.5])
        torch.manual_seed(hidden)
        sd = {k: v.clone() for k, v in build_glass(hidden, 2, int(x.max()), K, "mean", "size", 0.85).state_dict().items()}

        def oracle(weight):
            orc = O.OracleGLASS(hidden, 2, int(x.max()), K, aggr="mean", pool="size", z_ratio=0.85)
            orc.load_state_dict(sd)
            orc = orc.double().train()
            po = orc(x, ei, ew.double(), pos, O.max_zero_one(x, pos))
            lo = WO.ce_weighted(po, y, weight)
            lo.backward()
            return dict(loss=lo.detach(), logits=po.detach(), grads={k: p.grad for k, p in orc.named_parameters()})
        _MODEL[hidden] = dict(ei=ei, ew=ew, x=x, pos=pos, y=y, K=K, w=w, sd=sd, want=oracle(w), w2=torch.tensor([3.0, 0.25, 1.0]))
        _MODEL[hidden]["want2"] = oracle(_MODEL[hidden]["w2"])
    return _MODEL[hidden]


def _fresh_model(c, hidden):
    from glass_amd.arena import ParamArena
    model = build_glass(hidden, 2, int(c["x"].max()), c["K"], "mean", "size", 0.85)
    model.load_state_dict(c["sd"])
    model.to(DEV).train()
    return model, ParamArena(model)


def _logical_grads(model):
    from glass_amd import widths
    if hasattr(model, "_glass_logical_width"):
        g, pad_max = widths.logical_named_grads(model)
        assert pad_max == 0.0
    else:
        g = {k: p.grad for k, p in model.named_parameters()}
    return {k: v.detach().cpu().clone() for k, v in g.items()}


def _model_check(label, loss, logits, model, want):
    keys = sorted(want["grads"])
    e = dict(loss=abs(float(loss.detach() if torch.is_tensor(loss) else loss) - float(want["loss"])) / abs(float(want["loss"])),
             grad=rel_inf(flat_grads(_logical_grads(model), keys), flat_grads(want["grads"], keys)))
    if logits is not None:
        e["logits"] = rel_inf(logits.detach().cpu(), want["logits"])
    print(f"{label}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert all(v <= TOL for v in e.values()), (label, e)


@pytest.mark.parametrize("hidden", [64, 8])
def test_model_paths_vs_oracle(hidden, monkeypatch):
    """One training step with CrossEntropy(weight=) through stack.loss_and_grads, the per-op autograd path with the fused
    Linear head (what TrainStep runs without the step program) and the eager per-batch loop of train.train: loss, logits and
    the flat gradient against the fp64 OracleGLASS + the weighted restatement."""
    from glass_amd import stack, losses
    from impl import SubGDataset, train, utils, config
    c = _model_case(hidden)
    xg, eig, ewg, posg, yg = (c[k].to(DEV) for k in ("x", "ei", "ew", "pos", "y"))
    loss_fn = losses.CrossEntropy(weight=c["w"]).to(DEV)
    # the step program
    model, arena = _fresh_model(c, hidden)
    assert stack.step_supported(model, loss_fn) and stack.covers_arena(model, arena)
    loss, logits = stack.loss_and_grads(model, loss_fn, xg, eig, ewg, posg, "pos", yg, overwrite=True)
    torch.cuda.synchronize()
    _model_check(f"hidden {hidden} loss_and_grads", loss, logits, model, c["want"])
    with pytest.raises(ValueError):   # K must equal the weight's length, before any launch
        stack.loss_and_grads(model, losses.CrossEntropy(weight=torch.ones(4)).to(DEV), xg, eig, ewg, posg, "pos", yg, overwrite=True)
    # the per-op autograd path with the fused head
    monkeypatch.setattr(stack, "USE_READOUT", False)
    assert not stack.step_supported(model, loss_fn)
    arena.zero()
    emb = model.NodeEmb(xg, eig, ewg, utils.MaxZOZ(xg, posg))
    pooled = model.Pool(emb, posg, model.pools[0])
    loss, logits = losses.head_loss(pooled, model.preds[0], yg, losses.fusable_spec(loss_fn), direct=True)
    loss.backward()
    torch.cuda.synchronize()
    _model_check(f"hidden {hidden} per-op path + fused head", loss, logits, model, c["want"])
    # the eager per-batch loop (GLASS_TRAIN_STEP=0); lr 0 keeps the weights, the gradients stay in .grad
    monkeypatch.setattr(train, "USE_STEP", False)
    config.set_device(0)
    model, arena = _fresh_model(c, hidden)
    ds = SubGDataset.GDataset(xg, eig, ewg, posg, yg)
    loader = SubGDataset.ZGDataloader(ds, posg.shape[0], z_fn=utils.MaxZOZ, shuffle=False, drop_last=True)
    cpu_loss = losses.CrossEntropy(weight=c["w"])    # (train.train moves a marker's weights beside the model)
    mean = train.train(torch.optim.SGD(model.parameters(), lr=0.0), model, loader, cpu_loss)
    assert cpu_loss.weight.is_cuda
    _model_check(f"hidden {hidden} eager loop", mean, None, model, c["want"])


@pytest.mark.parametrize("hidden", [64, 8])
def test_captured_step_vs_oracle_and_weight_updates(hidden):
    """TrainStep (captured): the first step's loss and gradients equal the oracle's; replayed twice from the same state it is
    bitwise repeatable; an in-place change of the weight values is followed by the next replay without a new capture;
    another tensor means exactly one new capture."""
    from glass_amd import losses
    from glass_amd.optim import FlatAdam
    from glass_amd.step import TrainStep
    c = _model_case(hidden)
    xg, eig, ewg, posg, yg = (c[k].to(DEV) for k in ("x", "ei", "ew", "pos", "y"))
    loss_fn = losses.CrossEntropy(weight=c["w"])
    model, arena = _fresh_model(c, hidden)
    step = TrainStep(model, FlatAdam(arena, lr=1e-3), loss_fn, xg, eig, ewg, arena, use_graph=True, warmup_iters=1, preserve_state=True)
    assert loss_fn.weight.is_cuda           # (the step moved the marker's buffer to the GPU)
    snap = step._snapshot()
    l1 = step(posg, yg).clone()
    torch.cuda.synchronize()
    assert step.graphed and step._program_step() and step.n_captures == 1
    _model_check(f"hidden {hidden} captured step", l1, None, model, c["want"])
    g1, p1 = arena.flat.clone(), arena.flat_param.clone()
    step._restore(snap)
    l2 = step(posg, yg).clone()
    torch.cuda.synchronize()
    assert torch.equal(l1, l2) and torch.equal(g1, arena.flat) and torch.equal(p1, arena.flat_param)
    # new values in the same tensor: no capture, the replay reads them
    step._restore(snap)
    loss_fn.weight.copy_(c["w2"])
    l3 = step(posg, yg).clone()
    torch.cuda.synchronize()
    assert step.n_captures == 1
    _model_check(f"hidden {hidden} captured step, weights edited in place", l3, None, model, c["want2"])
    assert abs(float(l3) - float(l1)) > 1e-3 * abs(float(l1))
    # another tensor: one new capture, then none
    step._restore(snap)
    loss_fn.weight = c["w"].to(DEV)
    l4 = step(posg, yg).clone()
    torch.cuda.synchronize()
    assert step.n_captures == 2
    _model_check(f"hidden {hidden} captured step, weight tensor replaced", l4, None, model, c["want"])
    step(posg, yg)
    assert step.n_captures == 2


def test_gnn_seg_loss_and_logits_with_a_weighted_marker():
    """seg.GNN.loss_and_logits with CrossEntropy(weight=): the fused MLP head + weighted loss against the restatement of the
    same step — the model's own pooled embedding (fp32, from the GPU) through the MLP head and the weighted loss in fp64:
    loss, logits, the head's parameter gradients and d pooled."""
    from test_gpu_head_mlp import _density, _gnn
    from glass_amd import losses
    _ds, (bx, adj, ew, bpos, by) = _density("gin")
    K = int(by.max()) + 1
    w = torch.linspace(0.5, 3.0, K)
    m = _gnn("gin", K).train()
    loss_fn = losses.CrossEntropy(weight=w).to(DEV)
    kept = {}
    pooled_fn = m._pooled
    m._pooled = lambda *a: kept.setdefault("pooled", pooled_fn(*a).requires_grad_(True))  # (a leaf copy would cut the graph: keep the node)
    loss, logits = m.loss_and_logits(bx, adj, ew, bpos, by, loss_fn)
    kept["pooled"].retain_grad()
    loss.backward()
    torch.cuda.synchronize()
    mods = list(m.mods[1].seq.modlist)
    lin1, lin2 = mods[0], mods[-1]
    d = dict(pooled=kept["pooled"].detach().cpu(), W1=lin1.weight.detach().cpu(), b1=lin1.bias.detach().cpu(),
             W2=lin2.weight.detach().cpu(), b2=lin2.bias.detach().cpu())
    want = _oracle_head(d, by.cpu(), 0, w, True, 1.0)
    got = dict(loss=loss.detach().cpu(), logits=logits.detach().cpu(), dpooled=kept["pooled"].grad.cpu(), dW1=lin1.weight.grad.cpu(),
               db1=lin1.bias.grad.cpu(), dW2=lin2.weight.grad.cpu(), db2=lin2.bias.grad.cpu())
    _check(got, want, "GNN-seg weighted step")
    plain = _oracle_head(d, by.cpu(), 0, None, True, 1.0)
    assert abs(float(plain["loss"]) - float(want["loss"])) > 1e-3 * abs(float(want["loss"]))
