"""The fused two-layer MLP head on the MI355X (glass_amd/csrc/head_mlp.hip): the three entry points against the fp64 oracle
of tests/head_mlp_oracle.py, and the model paths that use them (seg.GNN.loss_and_logits, train.train / train.test on a
GsDataloader, step.TrainStep with an MLP head, the over-the-limit fallback).

Bounds: rel-inf <= 1e-5 against fp64 is the project's parity bound (README); an fp32 sum of <= 1024 terms in a fixed order
is a few 1e-7 of the largest term away from it.  accumulate = 1 adds one fp32 rounding (2^-24) to the accumulate = 0 value:
rel-inf <= 1e-6.  The evaluation entry runs the training entry's kernel template without the loss: the same sums in the same
order, so its logits are BITWISE the training entry's at p = 0 (asserted as such, not to a tolerance)."""
import copy
import ctypes
import functools
import os
import sys

import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import head_mlp_oracle as O  # noqa: E402
from helpers import flat_grads, rel_inf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5
CALL_ID = 3
GL = 0.75  # the incoming gradient of the loss (exact in fp32)


# ---------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def _inputs(B, C, Hd, K, mode, multilabel, pad, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + B + 7 * C + 13 * Hd + 31 * K)
    full = torch.randn(B, C + pad, generator=g)
    W1 = torch.randn(Hd, C, generator=g) / C ** 0.5
    b1 = 0.5 * torch.randn(Hd, generator=g)
    W2 = torch.randn(K, Hd, generator=g) / Hd ** 0.5
    b2 = 0.5 * torch.randn(K, generator=g)
    if mode == 0:
        tgt = torch.randint(0, K, (B, ), generator=g)
    else:
        tgt = (torch.rand((B, K) if multilabel else (B * K, ), generator=g) > 0.5).float()
    return full, W1, b1, W2, b2, tgt


def _mask(lib, B, Hd, p):
    """(rng words, keep-scales [B, Hd]) of a (seed, step) pair whose mask drops something: the scales are fetched with
    glass_dropout_scales_f32 from the very words and stream the head is then handed."""
    stream = torch.cuda.current_stream().cuda_stream
    for seed in range(64):
        words = torch.tensor([1234 + seed, 5], dtype=torch.int64, device=DEV)
        keep = torch.empty(B, Hd, device=DEV)
        assert lib.glass_dropout_scales_f32(words.data_ptr(), CALL_ID, p, B, Hd, keep.data_ptr(), stream) == 0
        if bool((keep == 0).any()):
            return words, keep
    raise AssertionError("no mask with a dropped element in 64 seeds")


def _run(lib, data, B, C, Hd, K, mode, act, p, words, accumulate=0, prefill=None):
    full, W1, b1, W2, b2, tgt = (t.to(DEV) for t in data)
    pooled = full[:, :C]  # a slice when the buffer is wider: ldp = C + pad
    ldp = full.stride(0)
    stream = torch.cuda.current_stream().cuda_stream
    hidden, logits = torch.empty(B, Hd, device=DEV), torch.empty(B, K, device=DEV)
    prob, loss = torch.empty(B * K + B, device=DEV), torch.empty((), device=DEV)
    rng = words.data_ptr() if p > 0 else None
    rc = lib.glass_head_mlp_loss_fwd_f32(pooled.data_ptr(), ldp, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr(),
                                         tgt.data_ptr(), mode, act, p, rng, CALL_ID, B, C, Hd, K, hidden.data_ptr(),
                                         logits.data_ptr(), prob.data_ptr(), loss.data_ptr(), stream)
    assert rc == 0, lib.glass_last_error_string()
    gl = torch.tensor([GL], device=DEV)
    ws = torch.empty(2 * B * Hd, device=DEV)
    dpooled = torch.full((B, C), float("nan"), device=DEV)
    sizes = (Hd * C, Hd, K * Hd, K)
    grads = [torch.full((n, ), float("nan"), device=DEV) for n in sizes] if prefill is None else [t.clone() for t in prefill]
    rc = lib.glass_head_mlp_loss_bwd_f32(pooled.data_ptr(), ldp, W1.data_ptr(), W2.data_ptr(), hidden.data_ptr(),
                                         prob.data_ptr(), tgt.data_ptr(), mode, act, p, rng, CALL_ID, gl.data_ptr(), B, C, Hd, K,
                                         ws.data_ptr(), dpooled.data_ptr(), C, *(t.data_ptr() for t in grads), accumulate,
                                         stream)
    assert rc == 0, lib.glass_last_error_string()
    ev = torch.empty(B, K, device=DEV)
    rc = lib.glass_head_mlp_f32(pooled.data_ptr(), ldp, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(), b2.data_ptr(), act, B, C,
                                Hd, K, ev.data_ptr(), K, stream)
    assert rc == 0, lib.glass_last_error_string()
    torch.cuda.synchronize()
    return {"logits": logits, "loss": loss, "hidden": hidden, "dpooled": dpooled, "grads": torch.cat(grads), "eval": ev}


# (B, C, Hd, K, mode, multi-label targets, extra columns of the pooled buffer)
SHAPES = [
    (1, 1, 1, 1, 1, False, 0),
    (3, 5, 4, 1, 1, False, 0),
    (7, 64, 16, 3, 0, False, 0),
    (5, 130, 17, 6, 0, False, 0),      # widths off every 4- and 64-lane boundary
    (6, 32, 8, 5, 1, True, 0),         # multi-label y[B, K]
    (9, 128, 64, 256, 0, False, 0),    # K at the limit
    (4, 16, 1024, 2, 0, False, 0),     # Hd at the limit
    (160, 512, 64, 1, 1, False, 0),    # GNN-seg ppi_bp's own head
    (7, 64, 16, 3, 0, False, 3),       # ldp = C + 3 from a sliced tensor
    (2, 4100, 3, 2, 0, False, 0),      # a pooled row wider than the LDS stage (4096): read in place
    (1030, 3, 2, 2, 1, False, 0),      # more subgraphs than one tile (1024) of the weight-gradient sums
]
ACT_CASES = [(s, O.ACT_ELU, p) for s in SHAPES for p in (0.0, 0.4)] + [(SHAPES[3], a, p) for a in (O.ACT_RELU, O.ACT_NONE)
                                                                       for p in (0.0, 0.4)]


def _id(case):
    (B, C, Hd, K, mode, ml, pad), act, p = case
    return f"B{B}-C{C}-Hd{Hd}-K{K}-{'bce' if mode else 'ce'}{'-ml' if ml else ''}{'-ld' if pad else ''}-act{act}-p{p}"


@pytest.mark.parametrize("case", ACT_CASES, ids=[_id(c) for c in ACT_CASES])
def test_entries_match_the_fp64_oracle(case):
    from glass_amd import _lib
    lib = _lib.load()
    (B, C, Hd, K, mode, ml, pad), act, p = case
    data = _inputs(B, C, Hd, K, mode, ml, pad)
    words = keep = None
    if p > 0:
        words, keep = _mask(lib, B, Hd, p)
        vals = set(torch.unique(keep).tolist())
        assert vals <= {0.0, float(torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p)))} and 0.0 in vals
    got = _run(lib, data, B, C, Hd, K, mode, act, p, words)
    full, W1, b1, W2, b2, tgt = data
    ref = O.run(full[:, :C], W1, b1, W2, b2, tgt, mode, act, keep)
    errs = {"logits": rel_inf(got["logits"].cpu(), ref["logits"]),
            "loss": abs(got["loss"].item() - ref["loss"].item()) / abs(ref["loss"].item()),
            "dpooled": rel_inf(got["dpooled"].cpu(), GL * ref["dpooled"]),
            "grads": rel_inf(got["grads"].cpu(), GL * ref["grads"])}
    print(_id(case), " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert all(v <= TOL for v in errs.values()), errs
    # the evaluation entry: the training entry's logits, bitwise, when nothing is dropped
    if p == 0:
        assert torch.equal(_bits(got["eval"]), _bits(got["logits"]))
    else:
        assert rel_inf(got["eval"].cpu(), O.run(full[:, :C], W1, b1, W2, b2, tgt, mode, act, None)["logits"]) <= TOL
    # two runs are bitwise equal
    again = _run(lib, data, B, C, Hd, K, mode, act, p, words)
    for k in got:
        assert torch.equal(_bits(got[k]), _bits(again[k])), k
    # accumulate = 1 into pre-filled gradients = the pre-fill + the accumulate = 0 result
    g = torch.Generator().manual_seed(5)
    prefill = [torch.randn(n, generator=g).to(DEV) for n in (Hd * C, Hd, K * Hd, K)]
    acc = _run(lib, data, B, C, Hd, K, mode, act, p, words, accumulate=1, prefill=prefill)
    assert rel_inf(acc["grads"].cpu(), torch.cat(prefill).cpu().double() + got["grads"].cpu().double()) <= 1e-6
    assert torch.equal(_bits(acc["dpooled"]), _bits(got["dpooled"]))


def test_mask_is_the_stream_of_the_words_it_is_given():
    """Other (seed, step) words, another mask and other logits; p = 0 ignores the words altogether."""
    from glass_amd import _lib
    lib = _lib.load()
    B, C, Hd, K = 7, 64, 16, 3
    data = _inputs(B, C, Hd, K, 0, False, 0)
    w0, k0 = _mask(lib, B, Hd, 0.4)
    w1 = w0 + torch.tensor([0, 1], device=DEV)
    a = _run(lib, data, B, C, Hd, K, 0, O.ACT_ELU, 0.4, w0)
    b = _run(lib, data, B, C, Hd, K, 0, O.ACT_ELU, 0.4, w1)
    assert not torch.equal(a["logits"], b["logits"]) and torch.equal(_bits(a["hidden"]), _bits(b["hidden"]))
    c = _run(lib, data, B, C, Hd, K, 0, O.ACT_ELU, 0.0, w0)
    d = _run(lib, data, B, C, Hd, K, 0, O.ACT_ELU, 0.0, None)
    assert torch.equal(_bits(c["logits"]), _bits(d["logits"])) and torch.equal(_bits(c["grads"]), _bits(d["grads"]))


# ---------------------------------------------------------------------------------------------------------------------
# model level: GNN-seg on the shipped density graph
# ---------------------------------------------------------------------------------------------------------------------
_DENSITY = {}


def _density(mode):
    """One full batch of the density test split in the convolution's value mode (built once per mode)."""
    if mode not in _DENSITY:
        import datasets
        from glass_amd import seg
        torch.manual_seed(0)
        g = datasets.load_dataset("density")
        g.addOneFeature()
        _, ei, w, pos, y = g.get_split("test")
        ds = seg.GsDataset(g.x.to(DEV), ei.to(DEV), w.to(DEV), pos.to(DEV), y.long().to(DEV), mode=mode)
        _DENSITY[mode] = (ds, next(iter(seg.GsDataloader(ds, len(ds), shuffle=False, drop_last=False))))
    return _DENSITY[mode]


def _gnn(mode, n_out, dropout=0.0, H=16, L=1, seed=3):
    from glass_amd import models, seg
    torch.manual_seed(seed)
    conv = seg.GConv(1, H, H, L, conv=seg.MyGINConv if mode == "gin" else seg.GCNConv, activation=nn.ELU(inplace=True),
                     dropout=dropout)
    mlp = models.MLP(H * L, H, n_out, 2, dropout=dropout, activation=nn.ELU(inplace=True))
    return seg.GNN(conv, mlp).to(DEV)


def _flat(model):
    return torch.cat([p.grad.reshape(-1) for p in model.parameters()]).double().cpu()


@pytest.mark.parametrize("mode,L", [("gin", 1), ("gcn", 2)])
def test_loss_and_logits_matches_the_module_path(mode, L):
    _ds, (bx, adj, ew, bpos, by) = _density(mode)
    n_out = int(by.max()) + 1
    a, b = _gnn(mode, n_out, L=L), _gnn(mode, n_out, L=L)
    a.train(), b.train()
    loss_fn = nn.CrossEntropyLoss()
    loss, logits = a.loss_and_logits(bx, adj, ew, bpos, by, loss_fn)
    loss.backward()
    pred = b(bx, adj, ew, bpos)
    ref = loss_fn(pred, by)
    ref.backward()
    e_loss = abs(loss.item() - ref.item()) / abs(ref.item())
    e_log, e_grad = rel_inf(logits.cpu(), pred.detach().cpu()), rel_inf(_flat(a), _flat(b))
    print(f"{mode}: loss {e_loss:.2e} logits {e_log:.2e} flat gradient {e_grad:.2e}")
    assert e_loss <= TOL and e_log <= TOL and e_grad <= TOL


def test_dropout_steps_repeat_with_the_seed_and_differ_from_no_dropout():
    import GNNSeg
    _ds, (bx, adj, ew, bpos, by) = _density("gin")
    n_out = int(by.max()) + 1
    loss_fn = nn.CrossEntropyLoss()
    outs = []
    for _ in range(2):
        GNNSeg.set_seed(7)
        m = _gnn("gin", n_out, dropout=0.4, seed=7)
        m.train()
        loss, logits = m.loss_and_logits(bx, adj, ew, bpos, by, loss_fn)
        loss.backward()
        outs.append(torch.cat([loss.detach().reshape(1), logits.reshape(-1)] + [q.grad.reshape(-1) for q in m.parameters()]))
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    # a second step draws another mask (the stream advanced); the same weights without dropout give another loss
    loss2, _ = m.loss_and_logits(bx, adj, ew, bpos, by, loss_fn)
    zero = _gnn("gin", n_out, dropout=0.0, seed=7)
    with torch.no_grad():
        for q, r in zip(zero.parameters(), m.parameters()):
            q.copy_(r)
    zero.train()
    loss0, _ = zero.loss_and_logits(bx, adj, ew, bpos, by, loss_fn)
    assert loss2.item() != outs[0][0].item() and loss0.item() != outs[0][0].item()
    # in eval mode the dropout is off: the two models agree bitwise
    m.eval(), zero.eval()
    le, _ = m.loss_and_logits(bx, adj, ew, bpos, by, loss_fn)
    lz, _ = zero.loss_and_logits(bx, adj, ew, bpos, by, loss_fn)
    assert torch.equal(_bits(le.detach()), _bits(lz.detach()))


def _spy(monkeypatch):
    from glass_amd import losses
    calls = []
    real = losses.MLPHeadLossFn.apply

    def apply(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(losses.MLPHeadLossFn, "apply", staticmethod(apply))
    return calls


def _spy_eval(monkeypatch):
    """Return codes of every glass_head_mlp_f32 call (the one-launch evaluation entry), in order."""
    from glass_amd import _lib
    lib = _lib.load()
    real, codes = lib.glass_head_mlp_f32, []

    def entry(*args):
        codes.append(real(*args))
        return codes[-1]

    monkeypatch.setattr(lib, "glass_head_mlp_f32", entry)
    return codes


def test_train_loop_fuses_once_per_batch_and_honours_the_opt_out(monkeypatch):
    from glass_amd import seg, train
    ds, (_bx, _adj, _ew, _bpos, by) = _density("gin")
    model = _gnn("gin", int(by.max()) + 1, dropout=0.4)
    loader = seg.GsDataloader(ds, max(len(ds) // 3, 1), shuffle=True, drop_last=True)
    assert len(loader) >= 2
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    calls = _spy(monkeypatch)
    loss = train.train(opt, model, loader, nn.CrossEntropyLoss())
    assert len(calls) == len(loader) and loss == loss
    del calls[:]

    def opted_out(pred, y):
        return nn.functional.cross_entropy(pred, y)

    opted_out._glass_no_fuse = True
    loss = train.train(opt, model, loader, opted_out)
    assert len(calls) == 0 and loss == loss


def test_evaluation_predictions_match_the_module_path(monkeypatch):
    from glass_amd import seg, train
    ds, (bx, adj, ew, bpos, by) = _density("gin")
    model = _gnn("gin", int(by.max()) + 1, dropout=0.4)
    loader = seg.GsDataloader(ds, len(ds), shuffle=False, drop_last=False)
    codes = _spy_eval(monkeypatch)
    pred, _loss = train.test(model, loader, lambda p, y: p, nn.CrossEntropyLoss())
    assert not model.training and codes == [0] * len(loader)  # one accepted call of the evaluation entry per batch
    ref = model(bx, adj, ew, bpos)  # grad enabled: the modules themselves
    assert codes == [0] * len(loader) and ref.requires_grad and rel_inf(pred, ref.detach().cpu()) <= TOL
    model.train()
    with torch.no_grad():  # training mode keeps the modules (the dropout is on), whatever the grad mode
        model(bx, adj, ew, bpos)
    assert codes == [0] * len(loader)


def test_head_over_the_limits_falls_back_to_the_modules(monkeypatch):
    _ds, (bx, adj, ew, bpos, by) = _density("gin")
    K = 300
    y = (torch.arange(by.shape[0], device=DEV) * 37) % K
    a, b = _gnn("gin", K), _gnn("gin", K)
    a.train(), b.train()
    loss_fn = nn.CrossEntropyLoss()
    calls = _spy(monkeypatch)
    loss, logits = a.loss_and_logits(bx, adj, ew, bpos, y, loss_fn)
    loss.backward()
    assert len(calls) == 1 and logits.requires_grad  # the fused entry was asked, refused, and the modules ran
    ref = loss_fn(b(bx, adj, ew, bpos), y)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= TOL * abs(ref.item()) and rel_inf(_flat(a), _flat(b)) <= TOL
    a.eval()
    codes = _spy_eval(monkeypatch)
    with torch.no_grad():
        out = a(bx, adj, ew, bpos)
        assert codes == [-3]  # the evaluation entry was asked once and refused (GLASS_E_UNSUPPORTED): the modules ran
        assert rel_inf(out.cpu(), a.mods[1](a._pooled(bx, adj, ew, bpos)).cpu()) <= TOL


# ---------------------------------------------------------------------------------------------------------------------
# model level: GLASS with an MLP head on the training step
# ---------------------------------------------------------------------------------------------------------------------
def test_train_step_takes_an_mlp_head():
    from glass_amd import losses, synth
    from glass_amd.arena import ParamArena
    from glass_amd.optim import FlatAdam
    from glass_amd.step import TrainStep
    from impl import models, utils
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=0, n_batches=1)
    ei, ew, x, pos, y = (torch.from_numpy(t).to(DEV) for t in (ei, ew, x, pos, y))
    h, L = w.hidden, w.layers
    torch.manual_seed(0)
    conv = models.EmbZGConv(h, h, L, max_deg=int(x.max()), activation=nn.ELU(inplace=True), jk=True, dropout=0.0,
                            conv=functools.partial(models.GLASSConv, aggr=w.aggr, z_ratio=w.z_ratio, dropout=0.0), gn=True)
    head = models.MLP(h * L, h, w.n_class, 2, dropout=0.0, activation=nn.ELU(inplace=True))
    model = models.GLASS(conv, nn.ModuleList([head]), nn.ModuleList([models.AddPool()])).to(DEV).train()
    plain = copy.deepcopy(model).train()
    pred = plain(x, ei, ew, pos, utils.MaxZOZ(x, pos), id=0)
    ref = nn.CrossEntropyLoss()(pred, y)
    ref.backward()
    arena = ParamArena(model)
    step = TrainStep(model, FlatAdam(arena, lr=1e-3), losses.CrossEntropy(), x, ei, ew, arena, use_graph=False,
                     warmup_iters=0)
    assert step._fused_head() == "mlp2" and not step._program_step()
    step._pos, step._y = pos.clone(), y.clone()
    step._fwd_bwd()
    torch.cuda.synchronize()
    assert abs(step._loss.item() - ref.item()) <= TOL * abs(ref.item())
    keys = [k for k, _ in plain.named_parameters()]
    mine = dict(model.named_parameters())
    assert rel_inf(flat_grads({k: mine[k].grad.cpu() for k in keys}, keys),
                   flat_grads({k: v.grad.cpu() for k, v in plain.named_parameters()}, keys)) <= TOL
