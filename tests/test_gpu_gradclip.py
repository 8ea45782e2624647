"""K9c on the GPU: glass_grad_norm_f32 / glass_adam_step_clip_f32 against the host and tests/gradclip_oracle.py, and clipping
through the model — TrainStep with FlatAdam(max_grad_norm=m), replayed and eager, against a CPU twin stepped with
torch.optim.Adam + clip_grad_norm_, and the reference-style caller (plain torch.optim.Adam whose group carries the key)."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

import gradclip_oracle as GO
from helpers import build_glass, rel_inf, flat_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _norm(g, max_norm, partials=None):
    L, lib = _lib()
    chunk = lib.glass_grad_norm_chunk()
    if partials is None:
        partials = torch.full((-(-g.numel() // chunk), ), float("nan"), dtype=torch.float64, device=DEV)  # (every slot is written)
    out = torch.full((2, ), -7.0, dtype=torch.float32, device=DEV)
    L.check(lib.glass_grad_norm_f32(g.data_ptr(), g.numel(), partials.data_ptr(), partials.numel(), max_norm, out.data_ptr(),
                                    _stream()), "glass_grad_norm_f32")
    return out


def _mixed(n, seed, offset):
    """n values with magnitudes from 1e-20 to 1e+18 and both signs; offset 1: the data starts one element behind a 16-byte
    boundary (the element-load form of the kernel)."""
    gen = torch.Generator().manual_seed(seed)
    v = (torch.rand(n, generator=gen, dtype=torch.float64) + 0.5) * 10.0 ** torch.randint(-20, 19, (n, ), generator=gen).double()
    v = (v * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)).float()
    buf = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    g = buf[offset:offset + n]
    g.copy_(v)
    return g, v


def _sizes():
    chunk = _lib()[1].glass_grad_norm_chunk()
    return [1, 3, 63, 64, 65, chunk - 1, chunk, chunk + 1, 3 * chunk + 17]


def _coef32(norm32, max_norm):
    """The fp32 formula on the host, from the fp32 norm."""
    return GO.clip_coef(torch.tensor(norm32, dtype=torch.float32), float(np.float32(max_norm)))


@pytest.mark.parametrize("offset", [0, 1])
def test_norm_and_coefficient_against_the_host(offset):
    """out[0] == float32(sqrt(sum g^2 in fp64)) within 1 ulp (an fp64 sum of n non-negative terms is off by < n 2^-53
    relative, far below half an fp32 ulp: only the final rounding can differ); out[1] == the fp32 formula on out[0], bitwise;
    a second run gives the same bits."""
    for i, n in enumerate(_sizes()):
        g, v = _mixed(n, 100 + i, offset)
        assert g.data_ptr() % 16 == 4 * offset
        want = np.float32(np.sqrt(np.sum(v.double().numpy() ** 2)))
        for max_norm in (1.0, float(want) * 0.37):
            out = _norm(g, max_norm)
            again = _norm(g, max_norm)
            got = out.cpu()
            assert abs(float(got[0]) - float(want)) <= float(np.spacing(want)), (n, offset, float(got[0]), float(want))
            assert got[1].view(torch.int32) == _coef32(float(got[0]), max_norm).view(torch.int32), (n, offset, got)
            assert torch.equal(out.view(torch.int32), again.view(torch.int32))
        assert float(got[1]) < 1.0


def test_norm_aligned_and_element_forms_give_the_same_bits():
    for i, n in enumerate(_sizes()):
        g0, v = _mixed(n, 300 + i, 0)
        g1, _ = _mixed(n, 300 + i, 1)
        assert torch.equal(_norm(g0, 1.0).view(torch.int32), _norm(g1, 1.0).view(torch.int32)), n


def test_norm_is_independent_of_what_else_runs():
    """The same input on a second stream while another stream keeps the device busy with large products: the partition is a
    function of n alone, so the bits are those of the quiet run."""
    chunk = _lib()[1].glass_grad_norm_chunk()
    g, _ = _mixed(37 * chunk + 5, 9, 0)
    quiet = _norm(g, 1.0).clone()
    a = torch.randn(4096, 4096, device=DEV)
    torch.cuda.synchronize()
    busy, side = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(busy):
        for _ in range(8):
            a = (a @ a).clamp_(-1.0, 1.0)
    with torch.cuda.stream(side):
        loud = _norm(g, 1.0)
    torch.cuda.synchronize()
    assert torch.equal(quiet.view(torch.int32), loud.view(torch.int32))


def test_norm_special_values():
    chunk = _lib()[1].glass_grad_norm_chunk()
    n = chunk + 77
    z = torch.zeros(n, device=DEV)
    assert _norm(z, 1.0).tolist() == [0.0, 1.0]
    g, _ = _mixed(n, 1, 0)
    g = (g.clamp(-1e3, 1e3)).contiguous()
    gi = g.clone()
    gi[chunk + 3] = float("inf")
    assert _norm(gi, 1.0).tolist() == [math.inf, 0.0]
    gn = g.clone()
    gn[5] = float("nan")
    out = _norm(gn, 1.0).tolist()
    assert math.isnan(out[0]) and math.isnan(out[1])  # (torch.clamp keeps a NaN)


# ---- the clipped Adam launch ------------------------------------------------------------------------------------------
def _adam_state(n, seed):
    """A state in which no sum of the update cancels: moments of an earlier run on gradients of the same sign and size (m ~ g,
    v ~ g^2), parameters of the gradient's sign (the decay term adds), magnitudes 0.5 .. 2."""
    gen = torch.Generator().manual_seed(seed)
    u = lambda: 0.5 + 1.5 * torch.rand(n, generator=gen)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    g = u() * sign
    return {"p": u() * sign, "g": g, "m": 0.25 * g * (0.5 + torch.rand(n, generator=gen)),
            "v": (0.25 * g) ** 2 * (0.5 + torch.rand(n, generator=gen))}


def _launch_adam(st, wd, coef=None, steps_done=5, lr=1e-2):
    L, lib = _lib()
    t = {k: v.clone().to(DEV) for k, v in st.items()}
    step_dev = torch.tensor([steps_done, 0], dtype=torch.int64, device=DEV)
    lr_dev = torch.tensor([lr], dtype=torch.float32, device=DEV)
    args = (t["p"].data_ptr(), t["g"].data_ptr(), t["m"].data_ptr(), t["v"].data_ptr(), t["p"].numel(), lr_dev.data_ptr(), 0.9, 0.999,
            1e-8, wd, step_dev.data_ptr())
    if coef is None:
        L.check(lib.glass_adam_step_f32(*args, _stream()), "glass_adam_step_f32")
    else:
        c = torch.tensor([coef], dtype=torch.float32, device=DEV)
        L.check(lib.glass_adam_step_clip_f32(*args, c.data_ptr(), _stream()), "glass_adam_step_clip_f32")
    torch.cuda.synchronize()
    t["step"] = step_dev
    return {k: v.cpu() for k, v in t.items()}


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("n", [1, 65, 4099])
def test_clipped_adam_with_coefficient_one_is_the_plain_launch(n, wd):
    st = _adam_state(n, n)
    plain, clip = _launch_adam(st, wd), _launch_adam(st, wd, coef=1.0)
    for k in ("p", "m", "v", "g"):
        assert torch.equal(plain[k].view(torch.int32), clip[k].view(torch.int32)), k
    assert plain["step"].tolist() == clip["step"].tolist() == [6, 0]
    assert torch.equal(clip["g"], st["g"]) and not torch.equal(clip["p"], st["p"])


def _ulps(a, b):
    a, b = a.numpy(), b.numpy()
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b))))


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("n", [1, 65, 4099])
def test_clipped_adam_against_the_restatement(n, wd):
    """coef = 0.25: parameters and moments within 2 ulp per element of tests/gradclip_oracle.py (fp32 torch ops on the host:
    each rounds on its own where the kernel may contract a multiply-add), the gradient left behind == g * 0.25 bitwise."""
    st = _adam_state(n, 50 + n)
    got = _launch_adam(st, wd, coef=0.25)
    p, gs, m, v = GO.clipped_adam_step(st["p"], st["g"], st["m"], st["v"], 6, 1e-2, 0.9, 0.999, 1e-8, wd, 0.25)
    assert torch.equal(got["g"].view(torch.int32), (st["g"] * 0.25).view(torch.int32)) and torch.equal(gs, st["g"] * 0.25)
    worst = {k: _ulps(got[k], w) for k, w in (("p", p), ("m", m), ("v", v))}
    assert max(worst.values()) <= 2.0, worst
    assert got["step"].tolist() == [6, 0]
    # the decay is added AFTER the scaling: scaling (g + wd p) instead moves the first moment by 0.75 wd p (1 - beta1)
    if wd:
        wrong = st["m"] + 0.1 * ((st["g"] + wd * st["p"]) * 0.25 - st["m"])
        assert _ulps(got["m"], wrong) > 100


# ---- through the model ------------------------------------------------------------------------------------------------
H, LAYERS, K_OUT, LR = 64, 2, 3, 1e-3


@pytest.fixture(scope="module")
def task():
    """The tiny synthetic graph with all-one features (`--use_one`), 3 batches of 8 subgraphs, one set of initial weights.

    The GraphNorm parameters are moved off their defaults (as tests/test_gpu_model.py's `_emb_pair` does).  With all-one
    features every embedding row is the same; at the default mean_scale = 1 emb_gn subtracts the mean of equal rows — rounding
    noise — and divides it by sqrt(eps), and Adam turns the sign of that noise into full steps: the model is then DEFINED by
    rounding (the fp32 oracle is 6e-5 .. 8e-4 from its own fp64 run on the first loss, percents two steps later), and no twin
    comparison says anything.  With mean_scale != 1 the rows keep a value of their own.  Weights (seed 11) and learning rate
    (1e-3) are ones at which the fp32 oracle, stepped with clip_grad_norm_ + Adam, stays within 2.7e-6 (losses) and 6.4e-6
    (parameters, rel-inf) of its own fp64 run over the three steps — a quarter of the bounds of the twin test below, so the
    twin is a reference at those bounds; at other seeds it is not (1.7e-5 .. 1.8e-4 on a loss at seeds 13, 14)."""
    from glass_amd import synth
    from impl import config
    config.set_device(0)
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=3, n_batches=3)
    ei, ew, pos, y = (torch.from_numpy(a) for a in (ei, ew, pos, y))
    x = torch.ones((x.shape[0], 1, 1), dtype=torch.int64)
    torch.manual_seed(11)
    sd = {k: v.clone() for k, v in build_glass(H, LAYERS, 1, K_OUT, "mean", "sum", 0.9).state_dict().items()}
    gen = torch.Generator().manual_seed(12)
    for k in sd:
        if k.endswith(("gn.weight", "gn.bias", "gn.mean_scale")) or ".gns." in k:
            sd[k] = sd[k] + 0.2 * torch.randn(sd[k].shape, generator=gen)
    return {"w": w, "cpu": (x, ei, ew, pos, y), "gpu": tuple(t.to(DEV) for t in (x, ei, ew, pos, y)), "sd": sd}


def _model(task):
    model = build_glass(H, LAYERS, 1, K_OUT, "mean", "sum", 0.9)
    model.load_state_dict(task["sd"])
    return model.to(DEV).train()


_ABSENT = object()


def _run(task, max_grad_norm, use_graph, steps=3):
    """`steps` steps of TrainStep on the FIRST batch (the same batch every step).  Returns per-step losses and grad_norm_dev pairs, the
    final flat parameters, and the live objects."""
    from glass_amd import losses
    from glass_amd.arena import ParamArena
    from glass_amd.optim import FlatAdam
    from glass_amd.step import TrainStep
    x, ei, ew, pos, y = task["gpu"]
    B = task["w"].batch
    model = _model(task)
    arena = ParamArena(model)
    opt = FlatAdam(arena, lr=LR) if max_grad_norm is _ABSENT else FlatAdam(arena, lr=LR, max_grad_norm=max_grad_norm)
    step = TrainStep(model, opt, losses.CrossEntropy(), x, ei, ew, arena, use_graph=use_graph, warmup_iters=1, preserve_state=True)
    out = {"loss": [], "norm": [], "params": [], "model": model, "opt": opt, "step": step, "arena": arena}
    for _ in range(steps):
        loss = step(pos[:B], y[:B])
        torch.cuda.synchronize()
        out["loss"].append(float(loss))
        out["norm"].append(opt.grad_norm_dev.cpu().clone())
        out["params"].append(arena.flat_param.cpu().clone())
    assert step.graphed == use_graph
    return out


@pytest.fixture(scope="module")
def runs(task):
    """A dry run whose threshold never clips gives the three norms; m lies between the first and the smallest later one."""
    dry = _run(task, 1e30, use_graph=False)
    norms = [float(n[0]) for n in dry["norm"]]
    assert all(float(n[1]) == 1.0 for n in dry["norm"])
    later = min(norms[1:])
    assert later < 0.9 * norms[0], f"the gradient norm does not shrink on the repeated batch: {norms}"
    m = math.sqrt(norms[0] * later)
    return {"m": m, "dry_norms": norms, "graph": _run(task, m, use_graph=True), "eager": _run(task, m, use_graph=False)}


def test_first_step_clips_and_a_later_one_does_not(runs):
    coefs = [float(n[1]) for n in runs["graph"]["norm"]]
    seen = [float(n[0]) for n in runs["graph"]["norm"]]
    msg = f"m = {runs['m']}, unclipped norms {runs['dry_norms']}, clipped run's norms {seen}, coefficients {coefs}"
    assert coefs[0] < 1.0 and max(coefs[1:]) == 1.0, msg
    assert seen[0] == runs["dry_norms"][0], msg  # (the first gradient does not depend on the threshold)
    step = runs["graph"]["step"]
    assert step._clip == runs["m"] and len(step._hyper) == 4
    assert not runs["graph"]["opt"].fusable()


def test_replay_and_eager_agree_bitwise(runs):
    g, e = runs["graph"], runs["eager"]
    for i in range(3):
        assert torch.equal(g["params"][i].view(torch.int32), e["params"][i].view(torch.int32)), i
        assert torch.equal(g["norm"][i].view(torch.int32), e["norm"][i].view(torch.int32)), (i, g["norm"][i], e["norm"][i])
    assert g["loss"] == e["loss"]


def test_against_the_cpu_twin(task, runs):
    """The oracle model on the same weights, torch.optim.Adam + clip_grad_norm_(max_norm = m) in fp32 on the CPU.  Bounds: those
    of tests/test_gpu_reference_caller.py's three-step comparison with the reference's own run (g8) — losses rtol 1e-5,
    parameters rel-inf < 1e-4; clipping adds one scalar multiply per gradient element to that comparison.
    The twin's own fp32 error on these weights is a quarter of those bounds (see `task`)."""
    from oracle import glass_oracle as O
    x, ei, ew, pos, y = task["cpu"]
    B = task["w"].batch
    orc = O.OracleGLASS(H, LAYERS, 1, K_OUT, aggr="mean", pool="sum", z_ratio=0.9)
    orc.load_state_dict(task["sd"])
    orc.train()
    opt = torch.optim.Adam(orc.parameters(), lr=LR)
    want, norms = [], []
    for _ in range(3):
        opt.zero_grad()
        loss = nn.CrossEntropyLoss()(orc(x, ei, ew, pos[:B], O.max_zero_one(x, pos[:B])), y[:B])
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(orc.parameters(), max_norm=runs["m"])))
        opt.step()
        want.append(loss.item())
    got = runs["graph"]
    keys = sorted(k for k, _ in orc.named_parameters())
    mine = {k: v.detach().cpu() for k, v in got["model"].named_parameters()}
    theirs = {k: v.detach() for k, v in orc.named_parameters()}
    e_par = rel_inf(flat_grads(mine, keys), flat_grads(theirs, keys))
    print(f"clipped twin: loss rel {[abs(a - b) / abs(b) for a, b in zip(got['loss'], want)]}, parameters rel-inf {e_par:.2e}, "
          f"norms {norms} vs {[float(n[0]) for n in got['norm']]}, m {runs['m']}")
    assert np.allclose(got["loss"], want, rtol=1e-5, atol=0), (got["loss"], want)
    assert e_par < 1e-4
    assert norms[0] > runs["m"] > min(norms[1:]), (norms, runs["m"])
    # and clipping acted: the unclipped trajectory (the first Adam step is scale-free, the later ones are not) is outside the
    # bound the clipped one meets
    free = _run(task, _ABSENT, use_graph=False)
    assert rel_inf(free["params"][-1], got["params"][-1]) > 1e-4


def test_switch_off_is_the_code_of_before(task):
    """max_grad_norm=None == a run that never mentions the keyword, bitwise, on the fused tail (fusable() is True)."""
    off, absent = _run(task, None, use_graph=True), _run(task, _ABSENT, use_graph=True)
    assert off["opt"].fusable() and absent["opt"].fusable()
    assert off["step"]._clip is None and off["step"]._hyper == (0.9, 0.999, 1e-8, 0.0)
    for i in range(3):
        assert torch.equal(off["params"][i].view(torch.int32), absent["params"][i].view(torch.int32))
    assert float(off["opt"].grad_norm_dev.abs().sum()) == 0.0  # no norm launch ran
    from glass_amd import stack
    assert stack.applied_optimizer(off["model"]), "with clipping off Adam still rides in the step's last launch"


def test_changed_threshold_recaptures_and_takes_effect(task, runs):
    from glass_amd import optim
    r = _run(task, runs["m"], use_graph=True, steps=1)
    step, opt = r["step"], r["opt"]
    x, ei, ew, pos, y = task["gpu"]
    B = task["w"].batch
    g0 = step._g_fb
    step(pos[:B], y[:B])
    assert step._g_fb is g0, "an unchanged threshold must not need a new capture"
    small = runs["m"] * 1e-3
    optim.set_max_grad_norm(opt, small)
    step(pos[:B], y[:B])
    torch.cuda.synchronize()
    assert step._g_fb is not g0 and step._clip == small
    norm, coef = opt.grad_norm_dev.cpu()
    assert coef.view(torch.int32) == _coef32(float(norm), small).view(torch.int32) and float(coef) < 1e-2
    # p.grad holds the scaled gradient: its norm is coef * norm (each element rounded once: far inside 1e-6 relative)
    assert float(torch.linalg.vector_norm(r["arena"].flat.double())) == pytest.approx(float(coef) * float(norm), rel=1e-6)
    g1 = step._g_fb
    optim.set_max_grad_norm(opt, None)
    before = opt.grad_norm_dev.clone()
    step(pos[:B], y[:B])
    torch.cuda.synchronize()
    assert step._g_fb is not g1 and step._clip is None and opt.fusable()
    assert torch.equal(opt.grad_norm_dev, before)  # no clipping launch in the new capture


def test_reference_style_caller_with_the_group_key(task, runs):
    """A plain torch.optim.Adam whose group carries max_grad_norm, driven by impl.train.train over ZGDataloader(MaxZOZ,
    drop_last): it takes the step program, and ends bitwise where FlatAdam(max_grad_norm=m) ends from the same seed."""
    from glass_amd import optim, losses
    from glass_amd.arena import ParamArena
    from impl import SubGDataset, train, utils
    x, ei, ew, pos, y = task["gpu"]
    ds = SubGDataset.GDataset(x, ei, ew, pos, y)
    ends = []
    for kind in ("torch", "flat"):
        model = _model(task)
        if kind == "torch":
            opt = torch.optim.Adam(model.parameters(), lr=LR)
            optim.set_max_grad_norm(opt, runs["m"])
        else:
            opt = optim.FlatAdam(ParamArena(model), lr=LR, max_grad_norm=runs["m"])
        loss_fn = nn.CrossEntropyLoss()
        for epoch in range(2):
            loader = SubGDataset.ZGDataloader(ds, task["w"].batch, z_fn=utils.MaxZOZ, shuffle=True, drop_last=True)
            loader.generator = torch.Generator().manual_seed(40 + epoch)
            if epoch == 0:
                assert train._graph_step(opt, model, loader, loss_fn) is not None
            train.train(opt, model, loader, loss_fn)
        step = next(iter(model.__dict__["_glass_train_steps"].values()))
        assert step.graphed and step._program_step() and step._clip == runs["m"]
        assert float(step.opt.grad_norm_dev[0]) > 0
        ends.append(torch.cat([p.detach().reshape(-1) for _k, p in sorted(model.named_parameters())]).cpu())
    assert torch.equal(ends[0].view(torch.int32), ends[1].view(torch.int32))


def test_unsupported_combinations_raise(task):
    """An attached one-shot peer exchange / a sharded arena: step() refuses, nothing is clipped wrongly."""
    from glass_amd._lib import GlassHipError
    from glass_amd.arena import ParamArena
    from glass_amd.optim import FlatAdam
    model = _model(task)
    arena = ParamArena(model)
    opt = FlatAdam(arena, lr=LR, max_grad_norm=1.0)
    before = arena.flat_param.clone()
    arena._peer = object()  # (never reached: the refusal comes first)
    with pytest.raises(GlassHipError, match="peer"):
        opt.step()
    arena._peer = None
    arena.sharded = lambda: True
    with pytest.raises(GlassHipError, match="sharded"):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(arena.flat_param, before)
