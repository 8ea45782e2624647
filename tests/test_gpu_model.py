"""Model-level parity on the GPU: the drop-in `impl.models` stack (HIP kernels through the C ABI)
against (a) the golden fixtures produced by the reference itself and (b) the CPU oracle on
larger seeded synthetic graphs.  Bar: rel-inf <= 1e-5 per output tensor and on the flat gradient
vector; the reference's own fp32-vs-fp64 noise is allowed where measured."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from helpers import load, sd_from, grads_from, rel_inf, flat_grads, density_inputs, build_glass, record_parity
from oracle import glass_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda:0"


@pytest.mark.parametrize("aggr", ["mean", "sum", "gcn"])
def test_g2_glassconv(aggr):
    from impl import models
    g = load(f"g2_conv_{aggr}.npz")
    conv = models.GLASSConv(8, 8, activation=nn.ELU(inplace=True), aggr=aggr, z_ratio=float(g["z_ratio"]), dropout=0.0)
    conv.load_state_dict(sd_from(g))
    conv.to(DEV)
    x = torch.from_numpy(g["x"]).to(DEV).requires_grad_(True)
    y = conv(x, torch.from_numpy(g["edge_index"]).to(DEV), torch.from_numpy(g["edge_weight"]).to(DEV),
             torch.from_numpy(g["mask"]).to(DEV).reshape(-1, 1))
    (y * torch.from_numpy(g["gout"]).to(DEV)).sum().backward()
    assert rel_inf(y.detach().cpu(), g["y64"]) < TOL
    assert rel_inf(x.grad.cpu(), g["grad_x64"]) < TOL
    ref = grads_from(g, "grad64/")
    keys = sorted(ref)
    mine = {k: p.grad.cpu() for k, p in conv.named_parameters()}
    assert sorted(mine) == keys
    assert rel_inf(flat_grads(mine, keys), flat_grads(ref, keys)) < TOL
    # and against the reference's fp32 run
    assert rel_inf(y.detach().cpu(), g["y"]) < TOL
    assert rel_inf(flat_grads(mine, keys), flat_grads(grads_from(g), keys)) < TOL


@pytest.mark.parametrize("layers", [1, 2, 3])
@pytest.mark.parametrize("jk", [0, 1])
def test_g3_embzgconv(layers, jk):
    import functools
    from impl import models
    g = load(f"g3_emb_L{layers}_jk{jk}.npz")
    h = int(g["hidden"])
    emb = models.EmbZGConv(h, h, layers, max_deg=5, activation=nn.ELU(inplace=True), jk=bool(jk), dropout=0.0,
                           conv=functools.partial(models.GLASSConv, aggr=str(g["aggr"]), z_ratio=float(g["z_ratio"]),
                                                  dropout=0.0), gn=True)
    emb.load_state_dict(sd_from(g))
    emb.to(DEV).eval()
    args = [torch.from_numpy(g[k]).to(DEV) for k in ("x", "edge_index", "edge_weight")]
    with torch.no_grad():
        y = emb(*args, torch.from_numpy(g["z"]).to(DEV))
        y_noz = emb(*args, None)
    assert rel_inf(y.cpu(), g["y64"]) < TOL
    assert rel_inf(y.cpu(), g["y"]) < TOL
    assert rel_inf(y_noz.cpu(), g["y_noz"]) < TOL


@pytest.mark.parametrize("aggr", ["sum", "mean", "gcn"])
def test_g5_density_full_model(aggr):
    """GLASS fwd + CE loss + every parameter gradient on the shipped density graph (H=64, L=2)."""
    from impl import utils
    g = load(f"g5_density_{aggr}.npz")
    n, ei, ew, x, pos, y, z = density_inputs(g)
    model = build_glass(int(g["hidden"]), int(g["layers"]), int(g["max_deg"]), 3, aggr, str(g["pool"]),
                        float(g["z_ratio"]))
    model.load_state_dict(sd_from(g))
    model.to(DEV).train()  # dropout = 0
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in (x, ei, ew, pos, y))
    zg = utils.MaxZOZ(xg, posg)
    assert np.array_equal(zg.cpu().numpy(), g["z"].astype(np.int64))
    emb = model.NodeEmb(xg, eig, ewg, zg)
    pred = model.preds[0](model.Pool(emb, posg, model.pools[0]))
    loss = nn.CrossEntropyLoss()(pred, yg)
    loss.backward()
    keys = [str(k) for k in g["gnorm64_keys"]]
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    assert sorted(mine) == keys
    ref64, ref32 = grads_from(g, "grad64/"), grads_from(g)
    # vs the reference evaluated in float64
    assert rel_inf(emb[:16].detach().cpu(), g["emb_rows64"]) < TOL
    assert rel_inf(emb.detach().double().sum(0).cpu(), g["emb_colsum64"]) < 1e-4  # cancelling column sums
    assert rel_inf(pred.detach().cpu(), g["pred64"]) < TOL
    assert abs(loss.item() - float(g["loss64"])) < TOL * abs(float(g["loss64"]))
    assert rel_inf(flat_grads(mine, keys), flat_grads(ref64, keys)) < TOL
    # vs the reference's fp32 run, allowing its own measured fp32 noise
    assert rel_inf(pred.detach().cpu(), g["pred"]) < TOL + rel_inf(g["pred"], g["pred64"])
    assert rel_inf(flat_grads(mine, keys), flat_grads(ref32, keys)) < TOL + rel_inf(flat_grads(ref32, keys),
                                                                                 flat_grads(ref64, keys))


def test_g8_adam_three_steps():
    from impl import utils
    g = load("g8_adam.npz")
    x = torch.from_numpy(g["x"]).to(DEV)
    ei, ew = torch.from_numpy(g["edge_index"]).to(DEV), torch.from_numpy(g["edge_weight"]).to(DEV)
    pos_all, y_all = torch.from_numpy(g["pos"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    model = build_glass(int(g["hidden"]), int(g["layers"]), int(x.max()), 3, str(g["aggr"]), str(g["pool"]),
                        float(g["z_ratio"]))
    model.load_state_dict(sd_from(g))
    model.to(DEV).train()
    opt = torch.optim.Adam(model.parameters(), lr=float(g["lr"]))
    losses = []
    for step in range(3):
        sel = torch.arange(step * 4, step * 4 + 4, device=DEV)
        p = pos_all[sel]
        z = utils.MaxZOZ(x, p)
        opt.zero_grad()
        loss = nn.CrossEntropyLoss()(model(x, ei, ew, p, z, id=0), y_all[sel])
        loss.backward()
        losses.append(loss.item())
        opt.step()
    assert np.allclose(losses, g["losses"], rtol=1e-5, atol=0)


@pytest.mark.parametrize("aggr", ["mean"])
def test_g5_density_with_param_arena(aggr):
    """Same fixture through the flat parameter/gradient arena: stacked weight VIEWS (no cat), weight and
    GraphNorm gradients accumulated straight into the arena by the kernels."""
    from impl import utils
    from glass_amd.arena import ParamArena
    g = load(f"g5_density_{aggr}.npz")
    n, ei, ew, x, pos, y, z = density_inputs(g)
    model = build_glass(int(g["hidden"]), int(g["layers"]), int(g["max_deg"]), 3, aggr, str(g["pool"]),
                        float(g["z_ratio"]))
    model.to(DEV).train()
    arena = ParamArena(model)
    model.load_state_dict(sd_from(g))  # in-place copy: keeps the aliasing
    assert arena.attached() and "trans" in model.conv.convs[0]._stack and "comb" in model.conv.convs[1]._stack
    W = model.conv.convs[0]._stack["trans"][0]
    assert torch.equal(W[:64], model.conv.convs[0].trans_fns[1].weight) and torch.equal(
        W[64:], model.conv.convs[0].trans_fns[0].weight)
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in (x, ei, ew, pos, y))
    for _ in range(2):  # twice: gradients must not leak across arena.zero()
        arena.zero()
        pred = model(xg, eig, ewg, posg, utils.MaxZOZ(xg, posg))
        loss = nn.CrossEntropyLoss()(pred, yg)
        loss.backward()
    keys = [str(k) for k in g["gnorm64_keys"]]
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    assert rel_inf(pred.detach().cpu(), g["pred64"]) < TOL
    assert rel_inf(flat_grads(mine, keys), flat_grads(grads_from(g, "grad64/"), keys)) < TOL
    assert list(model.state_dict().keys()) == [k[3:] for k in g.files if k.startswith("sd/")]


def test_g8_adam_three_steps_arena_flat_adam():
    from impl import utils
    from glass_amd.arena import ParamArena
    from glass_amd.optim import FlatAdam
    g = load("g8_adam.npz")
    x = torch.from_numpy(g["x"]).to(DEV)
    ei, ew = torch.from_numpy(g["edge_index"]).to(DEV), torch.from_numpy(g["edge_weight"]).to(DEV)
    pos_all, y_all = torch.from_numpy(g["pos"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    model = build_glass(int(g["hidden"]), int(g["layers"]), int(x.max()), 3, str(g["aggr"]), str(g["pool"]),
                        float(g["z_ratio"])).to(DEV).train()
    arena = ParamArena(model)
    model.load_state_dict(sd_from(g))
    opt = FlatAdam(arena, lr=float(g["lr"]))
    losses = []
    for step in range(3):
        sel = torch.arange(step * 4, step * 4 + 4, device=DEV)
        p = pos_all[sel]
        opt.zero_grad()
        loss = nn.CrossEntropyLoss()(model(x, ei, ew, p, utils.MaxZOZ(x, p), id=0), y_all[sel])
        loss.backward()
        losses.append(loss.item())
        opt.step()
    assert np.allclose(losses, g["losses"], rtol=1e-5, atol=0)
    end = sd_from(g, "sd_end/")
    keys = sorted(end)
    mine = {k: v.cpu() for k, v in model.state_dict().items()}
    assert rel_inf(flat_grads(mine, keys), flat_grads(end, keys)) < 1e-4


def test_train_step_graph_replay_matches_eager():
    """The hipGraph-replayed step (TrainStep) follows the eager step: same losses over 6 steps (dropout 0)."""
    from glass_amd import synth
    from glass_amd.arena import ParamArena
    from glass_amd.optim import FlatAdam
    from glass_amd.step import TrainStep
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=2, n_batches=6)
    ei, ew, x, pos, y = (torch.from_numpy(a).to(DEV) for a in (ei, ew, x, pos, y))
    pos, y = pos.reshape(6, w.batch, -1), y.reshape(6, w.batch)
    from glass_amd import losses
    curves = []
    for use_graph, loss_fn in ((False, nn.CrossEntropyLoss()), (True, nn.CrossEntropyLoss()),
                               (False, losses.CrossEntropy()), (True, losses.CrossEntropy())):
        torch.manual_seed(0)
        model = build_glass(w.hidden, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio).to(DEV).train()
        arena = ParamArena(model)
        opt = FlatAdam(arena, lr=5e-3)
        step = TrainStep(model, opt, loss_fn, x, ei, ew, arena, use_graph=use_graph, warmup_iters=2)
        curves.append([float(step(pos[i], y[i]).item()) for i in range(6)])
        assert step.graphed == use_graph
    for c in curves[1:]:  # graph replay == eager; fused head+loss == torch's Linear + CrossEntropyLoss
        assert np.allclose(curves[0], c, rtol=2e-5, atol=0)
    assert curves[0][-1] != curves[0][0]


def test_g9_state_dict_keys():
    g = load("g9_keys.npz")
    model = build_glass(64, 2, 1, 3, "mean", "sum", 0.8)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [str(list(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]]


def _oracle_vs_hip(name, seed, dtype64=True):
    from glass_amd import synth
    from impl import utils
    w, ei, ew, x, pos, y = synth.make_workload(name, seed=seed, n_batches=1)
    ei, ew, x, pos = (torch.from_numpy(a) for a in (ei, ew, x, pos))
    y = torch.from_numpy(y)
    max_deg = int(x.max())
    out_ch = w.n_class
    loss_fn = (lambda p, t: nn.BCEWithLogitsLoss()(p.flatten(), t.flatten())) if w.multilabel else nn.CrossEntropyLoss()
    torch.manual_seed(seed)
    model = build_glass(w.hidden, w.layers, max_deg, out_ch, w.aggr, w.pool, w.z_ratio)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(DEV).train()
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in (x, ei, ew, pos, y))
    pred = model(xg, eig, ewg, posg, utils.MaxZOZ(xg, posg))
    loss = loss_fn(pred, yg)
    loss.backward()
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    res = {}
    for dt in ((torch.float64, torch.float32) if dtype64 else (torch.float32, )):
        orc = O.OracleGLASS(w.hidden, w.layers, max_deg, out_ch, aggr=w.aggr, pool=w.pool, z_ratio=w.z_ratio)
        orc.load_state_dict(sd)
        orc = orc.to(dt).train()
        z = O.max_zero_one(x, pos)
        po = orc(x, ei, ew.to(dt), pos, z)
        lo = loss_fn(po, y if not w.multilabel else y.to(dt))
        lo.backward()
        res[dt] = (po.detach(), lo.item(), {k: p.grad for k, p in orc.named_parameters()})
    return pred.detach().cpu(), loss.item(), mine, res


@pytest.mark.parametrize("name", ["tiny", "ppi_bp", "em_user"])
def test_synthetic_workload_vs_oracle(name):
    """BASELINE configs' shapes (C2 ppi_bp-shaped H=64 L=2 mean/sum; C4 em_user-scale H=128 gcn/size):
    full step forward + loss + gradients vs the CPU oracle in fp64 and fp32."""
    pred, loss, mine, res = _oracle_vs_hip(name, seed=0)
    keys = sorted(mine)
    p64, l64, g64 = res[torch.float64]
    p32, l32, g32 = res[torch.float32]
    record_parity(f"per_op_path/{name}", logits_rel_inf=rel_inf(pred, p64), loss_rel=abs(loss - l64) / abs(l64),
                  grad_rel_inf=rel_inf(flat_grads(mine, keys), flat_grads(g64, keys)),
                  oracle_fp32_vs_fp64_logits=rel_inf(p32, p64),
                  oracle_fp32_vs_fp64_grad=rel_inf(flat_grads(g32, keys), flat_grads(g64, keys)))
    assert rel_inf(pred, p64) < TOL
    assert abs(loss - l64) < TOL * abs(l64)
    assert rel_inf(flat_grads(mine, keys), flat_grads(g64, keys)) < TOL
    # the HIP path should sit as close to fp64 truth as the CPU fp32 oracle does (within 1e-5)
    assert rel_inf(pred, p32) < TOL
    assert rel_inf(flat_grads(mine, keys), flat_grads(g32, keys)) < TOL


def test_hpo_neuro_shape_vs_oracle():
    """C3 (hpo_neuro-shaped, mean degree 444, gcn, multilabel BCE): report build-vs-fp64 next to
    oracle-fp32-vs-fp64 (SpMM re-ordering alone costs ~1e-5 here)."""
    pred, loss, mine, res = _oracle_vs_hip("hpo_neuro", seed=0)
    keys = sorted(mine)
    p64, l64, g64 = res[torch.float64]
    p32, l32, g32 = res[torch.float32]
    e_pred, e_grad = rel_inf(pred, p64), rel_inf(flat_grads(mine, keys), flat_grads(g64, keys))
    o_pred, o_grad = rel_inf(p32, p64), rel_inf(flat_grads(g32, keys), flat_grads(g64, keys))
    print(f"hpo_neuro-shape: hip-vs-fp64 pred {e_pred:.2e} grad {e_grad:.2e} | cpu-fp32-vs-fp64 pred {o_pred:.2e} "
          f"grad {o_grad:.2e}")
    record_parity("per_op_path/hpo_neuro", logits_rel_inf=e_pred, loss_rel=abs(loss - l64) / abs(l64), grad_rel_inf=e_grad,
                  oracle_fp32_vs_fp64_logits=o_pred, oracle_fp32_vs_fp64_grad=o_grad)
    assert e_pred < TOL and e_grad < TOL  # (measured 4e-7: the noise form max(TOL, 2 * o_grad) was 25x looser than the code)


def test_eval_forward_bitwise_repeatable():
    """Reference eval-mode forward is bitwise repeatable on CPU; so is ours."""
    from glass_amd import synth
    from impl import utils
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=3, n_batches=1)
    ei, ew, x, pos = (torch.from_numpy(a).to(DEV) for a in (ei, ew, x, pos))
    torch.manual_seed(0)
    model = build_glass(w.hidden, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio).to(DEV).eval()
    z = utils.MaxZOZ(x, pos)
    with torch.no_grad():
        a = model(x, ei, ew, pos, z)
        b = model(x, ei, ew, pos, z)
    assert torch.equal(a, b)


def test_train_and_test_loops():
    """impl.train.train / impl.train.test with ZGDataloader(z_fn=MaxZOZ): tuple layout
    (x, ei, ea, pos, z, y), mean loss returned, loss decreases over a few epochs."""
    from glass_amd import synth
    from impl import SubGDataset, train, utils, metrics
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=1, n_batches=6)
    ds = SubGDataset.GDataset(*(torch.from_numpy(a) for a in (x, ei, ew, pos, y))).to(DEV)
    loader = SubGDataset.ZGDataloader(ds, w.batch, z_fn=utils.MaxZOZ, shuffle=True, drop_last=True)
    batch = next(iter(loader))
    assert len(batch) == 6 and batch[3].shape == (w.batch, w.sub_size) and batch[4].shape == (w.n_node, )
    torch.manual_seed(0)
    model = build_glass(w.hidden, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=5e-3)
    losses = [train.train(opt, model, loader, nn.CrossEntropyLoss()) for _ in range(8)]
    assert losses[-1] < losses[0]
    score, loss = train.test(model, SubGDataset.ZGDataloader(ds, w.batch, z_fn=utils.MaxZOZ, shuffle=True,
                                                             drop_last=False), metrics.microf1, nn.CrossEntropyLoss())
    assert 0.0 <= score <= 1.0 and torch.isfinite(loss)


def test_driver_density_learns(capsys):
    """GLASSTest.py-compatible driver end to end on the shipped density set with the README recipe
    (--use_one --use_seed --use_maxzeroone; config/density.yml: H=8, L=1, batch 2): log format and the test
    micro-F1 after 40 epochs.  The reference's CPU run reaches 0.968; with `--use_one` features the
    trajectory is rounding-defined (any change of a summation order moves the outputs at O(0.1)),
    so builds of this library have landed between 0.90 and 0.97 — each of them reproducibly, run to run."""
    import GLASSTest
    outs = GLASSTest.main(["--use_one", "--use_seed", "--use_maxzeroone", "--repeat", "1", "--device", "0",
                           "--dataset", "density", "--max_epoch", "40"])
    text = capsys.readouterr().out
    assert "params {" in text and "repeat 0" in text and "end: epoch" in text and "average " in text
    assert any(line.startswith("iter ") and " val " in line and " tst " in line for line in text.splitlines())
    assert outs[0] > 0.85


@pytest.mark.parametrize("name", ["L2_jk0_mean", "L3_jk1_gcn", "L1_jk0_sum"])
def test_g10_edgegnn_ssl_path(name):
    """SSL pre-training path: EdgeGNN / EmbGConv / MyGCNConv on the HIP kernels vs the reference
    (fp64 and fp32 runs), incl. the in-place-ReLU JK quirk."""
    import functools
    from impl import models
    g = load(f"g10_edgegnn_{name}.npz")
    h, layers, jk = int(g["hidden"]), int(g["layers"]), bool(g["jk"])
    x = torch.from_numpy(g["x"])
    conv = models.EmbGConv(h, h, h, layers, max_deg=int(x.max()), activation=nn.ReLU(inplace=True), jk=jk, dropout=0.0,
                           conv=functools.partial(models.MyGCNConv, aggr=str(g["aggr"])), gn=True)
    head = models.MLP(h * layers if jk else h, h, 1, 2, dropout=0.0, activation=nn.ReLU(inplace=True))
    model = models.EdgeGNN(conv, nn.ModuleList([head]), nn.ModuleList([models.MeanPool()]))
    model.load_state_dict(sd_from(g))
    model.to(DEV).train()
    pred = model(x.to(DEV), torch.from_numpy(g["edge_index"]).to(DEV), torch.from_numpy(g["edge_weight"]).to(DEV),
                 torch.from_numpy(g["pairs"]).to(DEV))
    loss = nn.BCEWithLogitsLoss()(pred.flatten(), torch.from_numpy(g["y"]).to(DEV))
    loss.backward()
    ref64, ref32 = grads_from(g, "grad64/"), grads_from(g, "grad/")
    keys = sorted(ref64)
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    assert sorted(mine) == keys
    assert rel_inf(pred.detach().cpu(), g["pred64"]) < TOL and rel_inf(pred.detach().cpu(), g["pred"]) < TOL
    assert abs(loss.item() - float(g["loss64"])) < TOL * abs(float(g["loss64"]))
    assert rel_inf(flat_grads(mine, keys), flat_grads(ref64, keys)) < TOL
    assert rel_inf(flat_grads(mine, keys), flat_grads(ref32, keys)) < TOL


def test_pretraining_driver_learns_links(tmp_path, capsys):
    """GNNEmb.py-compatible driver: one trial of link-prediction pre-training on the shipped density graph
    learns to separate edges from sampled non-edges and writes the [N,64] embedding file GLASSTest.py
    --use_nodeid consumes."""
    import GNNEmb
    score, params = GNNEmb.main(["--use_nodeid", "--use_seed", "--device", "0", "--dataset", "density", "--name",
                                 "density", "--path", str(tmp_path) + "/", "--optruns", "1", "--max_epoch", "16"])
    text = capsys.readouterr().out
    assert "iter 0 loss" in text and "best valf1" in text
    emb = torch.load(str(tmp_path / "density_64.pt"))
    assert emb.shape == (4998, 64) and bool(torch.isfinite(emb).all())
    assert score > 0.6  # binary F1 on a balanced edge / non-edge set: well above the 0.5 of an untrained model


def test_pretraining_graphed_step_matches_eager_step():
    """GNNEmb.GraphedPairStep: the link-prediction forward + backward replayed from a hipGraph (third batch of a shape
    onwards) leaves the gradients and loss of the eager step — dropout 0, same batches; a batch of another shape in between
    runs eagerly and does not disturb the captured one."""
    import functools
    import GNNEmb
    from impl import models
    from glass_amd import synth
    w, ei, ew, x, _pos, _y = synth.make_workload("tiny", seed=2, n_batches=1)
    ei, ew, x = (torch.from_numpy(a).to(DEV) for a in (ei, ew, x))
    rng = np.random.default_rng(5)
    h = 64

    def build():
        torch.manual_seed(3)
        conv = models.EmbGConv(h, h, h, 2, max_deg=int(x.max()), activation=nn.ReLU(inplace=True), jk=False, dropout=0.0,
                               conv=functools.partial(models.MyGCNConv, aggr="mean"), gn=True)
        head = models.MLP(h, h, 1, 2, dropout=0.0, activation=nn.ReLU(inplace=True))
        return models.EdgeGNN(conv, nn.ModuleList([head]), nn.ModuleList([models.MeanPool()])).to(DEV).train()

    def loss_fn(pred, t):
        return nn.BCEWithLogitsLoss()(pred.flatten(), t.flatten())

    batches = []
    for k in range(6):
        nb = 333 if k == 3 else 2048
        batches.append((torch.from_numpy(rng.integers(0, w.n_node, size=(nb, 2))).to(DEV),
                        torch.from_numpy(rng.integers(0, 2, size=nb).astype(np.float32)).to(DEV)))
    runs = []
    for graph in (False, True):
        model = build()
        step = GNNEmb.GraphedPairStep(model, loss_fn, x, ei, ew)
        step.enabled = graph
        opt = torch.optim.SGD(model.parameters(), lr=0.05)
        losses = []
        for pairs, target in batches:
            losses.append(float(step(pairs, target)))
            opt.step()
        assert bool(step.graphs) == graph
        runs.append((losses, torch.cat([p.detach().flatten() for p in model.parameters()]).cpu()))
    assert runs[0][0] == pytest.approx(runs[1][0], rel=1e-6)
    assert rel_inf(runs[1][1], runs[0][1]) < 1e-6


def test_train_epoch_graph_path_matches_eager_path():
    """impl.train.train replays the step from a hipGraph when the epoch is graph-safe (FlatAdam, ZGDataloader with
    MaxZOZ, drop_last).  The state-preserving warm-up must leave the trajectory untouched: epoch losses and final
    weights equal the eager loop's (dropout 0, same shuffles)."""
    from glass_amd import synth
    from glass_amd.arena import ParamArena
    from glass_amd.optim import FlatAdam
    from impl import SubGDataset, train, utils
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=4, n_batches=6)
    ds = SubGDataset.GDataset(*(torch.from_numpy(a) for a in (x, ei, ew, pos, y))).to(DEV)
    results = []
    for use_graph in (False, True):
        train.USE_STEP = use_graph   # False: the plain per-batch autograd loop; True: TrainStep, replayed from a hipGraph
        torch.manual_seed(0)
        model = build_glass(w.hidden, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio).to(DEV)
        opt = FlatAdam(ParamArena(model), lr=5e-3)
        loader = SubGDataset.ZGDataloader(ds, w.batch, z_fn=utils.MaxZOZ, shuffle=True, drop_last=True)
        loader.generator = torch.Generator().manual_seed(7)
        losses = [train.train(opt, model, loader, nn.CrossEntropyLoss()) for _ in range(4)]
        results.append((losses, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()))
        assert ("_glass_train_steps" in model.__dict__) == use_graph
    train.USE_STEP = True
    assert np.allclose(results[0][0], results[1][0], rtol=2e-5, atol=0)
    assert rel_inf(results[1][1], results[0][1]) < 1e-4
    assert results[0][0][-1] < results[0][0][0]


# ---------------------------------------------------------------------------------- whole-stack program
def _emb_pair(layers, jk, aggr, z_ratio, dropout, seed, n=700, n_pairs=4000, V=9, H=64):
    """(product EmbZGConv with arena on the GPU, oracle twin with the same weights, inputs)."""
    import functools
    from glass_amd import synth
    from glass_amd.arena import ParamArena
    from impl import models
    torch.manual_seed(seed)
    emb = models.EmbZGConv(H, H, layers, max_deg=V - 1, activation=nn.ELU(inplace=True), jk=bool(jk), dropout=dropout,
                           conv=functools.partial(models.GLASSConv, aggr=aggr, z_ratio=z_ratio, dropout=dropout),
                           gn=True)
    with torch.no_grad():  # non-trivial GraphNorm parameters
        for m in emb.modules():
            if isinstance(m, models.GraphNorm):
                m.weight.add_(0.2 * torch.randn_like(m.weight))
                m.bias.add_(0.2 * torch.randn_like(m.bias))
                m.mean_scale.add_(0.2 * torch.randn_like(m.mean_scale))
    sd = {k: v.clone() for k, v in emb.state_dict().items()}
    ei, ew = synth.make_graph(n, n_pairs, seed, 0.0)
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.integers(0, V, n)).reshape(n, 1)
    z = torch.from_numpy((rng.random(n) < 0.1).astype(np.int64))
    gout = torch.randn(n, H * layers if jk else H, generator=torch.Generator().manual_seed(seed))
    orc = O.OracleEmbZGConv(H, H, layers, V - 1, dropout, aggr, z_ratio, jk=bool(jk))
    orc.load_state_dict(sd)
    emb.to(DEV)
    arena = ParamArena(emb)
    return emb, arena, orc, (x, torch.from_numpy(ei), torch.from_numpy(ew), z), gout


@pytest.mark.parametrize("layers,jk,aggr,hidden", [(1, 1, "mean", 64), (2, 1, "gcn", 64), (3, 1, "sum", 64), (2, 0, "mean", 64),
                                                   (3, 0, "gcn", 64), (2, 1, "mean", 128), (3, 0, "sum", 128),
                                                   (2, 1, "mean", 256), (1, 0, "gcn", 256), (1, 1, "sum", 512),
                                                   # the widths of the reference's own YAMLs for the shipped sets (thread-per-row
                                                   # kernels, dense_narrow.hip): density / cut_ratio 8, component 17, coreness 20
                                                   (1, 1, "sum", 8), (2, 0, "mean", 8), (1, 1, "sum", 17), (3, 1, "gcn", 17),
                                                   (2, 1, "sum", 20), (2, 1, "mean", 32), (1, 0, "gcn", 4)])
def test_stack_program_vs_oracle(layers, jk, aggr, hidden):
    """EmbZGConv as one forward/backward program (glass_amd/stack.py), hidden 64, 128 (column-split dense kernels) and
    256 (LDS-tiled dense kernels; n = 700 is not a multiple of their 128-row tile), against the fp64 oracle: output, every parameter gradient (accumulated in place in the arena), and eval mode."""
    from glass_amd import stack
    emb, arena, orc, (x, ei, ew, z), gout = _emb_pair(layers, jk, aggr, 0.85, 0.0, seed=layers * 2 + jk, H=hidden)
    assert stack.StackProgram.supported(emb)
    emb.train()
    args = [t.to(DEV) for t in (x, ei, ew, z)]
    for _ in range(2):  # twice: activations of the first pass must not leak into the second
        arena.zero()
        y = emb(*args)
        assert isinstance(y.grad_fn, stack.StackFn._backward_cls)
        y.backward(gout.to(DEV))
    orc = orc.double().train()
    yo = orc(x.reshape(-1), ei, ew.double(), z)
    yo.backward(gout.double())
    assert rel_inf(y.detach().cpu(), yo.detach()) < TOL
    mine = {k: p.grad.cpu() for k, p in emb.named_parameters()}
    theirs = {k: p.grad for k, p in orc.named_parameters()}
    keys = sorted(mine)
    assert rel_inf(flat_grads(mine, keys), flat_grads(theirs, keys)) < TOL
    for k in keys:  # no tensor may hide behind a larger one in the flat norm
        assert rel_inf(mine[k], theirs[k]) < 5 * TOL, k
    emb.eval()
    with torch.no_grad():
        ye = emb(*args[:3], None)
    assert rel_inf(ye.cpu(), orc.eval()(x.reshape(-1), ei, ew.double(), None).detach()) < TOL


@pytest.mark.parametrize("hidden", [64, 256, 17, 20])
def test_stack_program_matches_per_op_path_with_dropout(monkeypatch, hidden):
    """Same kernels, same dropout call ids: with dropout 0.5 the program and the per-op autograd path must draw the
    same masks, so outputs and gradients agree to rounding (the gradient sums are merely associated differently).
    hidden 256: the masks drawn in the tiled kernels' operand staging / epilogues against the stand-alone GraphNorm's."""
    from glass_amd import models as gm, ops
    emb, arena, _orc, (x, ei, ew, z), gout = _emb_pair(2, 1, "mean", 0.95, 0.5, seed=11, H=hidden)
    emb.train()
    args = [t.to(DEV) for t in (x, ei, ew, z)]
    res = []
    for use in (True, False):
        monkeypatch.setattr(gm, "USE_STACK", use)
        ops.rng_seed(1234, torch.device(DEV))
        arena.zero()
        y = emb(*args)
        y.backward(gout.to(DEV))
        res.append((y.detach().clone(), arena.flat.clone()))
    assert float((res[0][0] == 0).float().mean()) < 0.01  # final GraphNorm output: dropout acts upstream only
    assert rel_inf(res[0][0].cpu(), res[1][0].cpu()) < 1e-6
    assert rel_inf(res[0][1].cpu(), res[1][1].cpu()) < 1e-6


@pytest.mark.parametrize("layers", [1, 3])
def test_exact_graphnorm_accumulators_match_partial_sums(monkeypatch, layers):
    """Hidden 64: the backward column sums of the GraphNorms accumulated with 64-bit fixed-point atomics (gn_acc.h, no
    finalize launch) against the per-workgroup partials + finalize form: same masks, gradients equal to fp32 rounding;
    and the exact form twice -> bit-identical gradients (integer atomics commute, float atomics would not)."""
    from glass_amd import ops, stack, _lib
    emb, arena, _orc, (x, ei, ew, z), gout = _emb_pair(layers, 1, "mean", 0.95, 0.5, seed=5, H=64)
    assert _lib.load().glass_gn_exact_supported(64) == 1 and _lib.load().glass_gn_exact_supported(128) == 0
    emb.train()
    args = [t.to(DEV) for t in (x, ei, ew, z)]
    res = []
    for exact in (True, False, True):
        monkeypatch.setattr(stack, "USE_GN_EXACT", exact)
        ops.rng_seed(99, torch.device(DEV))
        arena.zero()
        y = emb(*args)
        y.backward(gout.to(DEV))
        res.append((y.detach().clone(), arena.flat.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert rel_inf(res[0][1].cpu(), res[1][1].cpu()) < 1e-6
    assert torch.equal(res[0][1], res[2][1])


def test_eval_after_optimizer_step_uses_current_weights():
    """The fused dense kernels read packed operand images of the weights; they must be re-packed whenever the
    weights may have changed, also for a no-grad evaluation right after an optimizer step."""
    from glass_amd.optim import FlatAdam
    emb, arena, _orc, (x, ei, ew, z), gout = _emb_pair(2, 1, "mean", 0.9, 0.0, seed=3)
    args = [t.to(DEV) for t in (x, ei, ew, z)]
    opt = FlatAdam(arena, lr=0.05)
    emb.train()
    arena.zero()
    emb(*args).backward(gout.to(DEV))
    opt.step()
    emb.eval()
    with torch.no_grad():
        y1 = emb(*args)
    arena.refresh_transposes()
    with torch.no_grad():
        y2 = emb(*args)
    assert torch.equal(y1, y2)
    sd = {k: v.detach().cpu().clone() for k, v in emb.state_dict().items()}
    _orc.load_state_dict(sd)
    assert rel_inf(y1.cpu(), _orc.double().eval()(x.reshape(-1), ei, ew.double(), z).detach()) < TOL


@pytest.mark.parametrize("V,n", [(1500, 700), (9000, 9500)])
def test_stack_program_large_tables(V, n):
    """Large embedding tables: up to GLASS_EMBED_NORM_MAX_ROWS = 8 192 rows (the degree feature of the 1 M-node power-law
    graph has 1 814) the lookup + emb_gn still run through the table; beyond (node-id style features) they stay on
    the [N,H] kernels.  Both against the fp64 oracle."""
    emb, arena, orc, (x, ei, ew, z), gout = _emb_pair(2, 1, "mean", 0.8, 0.0, seed=5, V=V, n=n, n_pairs=6 * n)
    emb.train()
    args = [t.to(DEV) for t in (x, ei, ew, z)]
    arena.zero()
    y = emb(*args)
    y.backward(gout.to(DEV))
    orc = orc.double().train()
    yo = orc(x.reshape(-1), ei, ew.double(), z)
    yo.backward(gout.double())
    assert rel_inf(y.detach().cpu(), yo.detach()) < TOL
    mine = {k: p.grad.cpu() for k, p in emb.named_parameters()}
    theirs = {k: p.grad for k, p in orc.named_parameters()}
    keys = sorted(mine)
    assert rel_inf(flat_grads(mine, keys), flat_grads(theirs, keys)) < TOL


@pytest.mark.parametrize("pool,multilabel,H,L", [("sum", False, 64, 2), ("mean", False, 64, 2), ("size", True, 64, 2),
                                                 # long padded rows (em_user's subgraphs): the readout stages the node ids in
                                                 # LDS and walks four entries per round (H < 0 marks the case: |H|, S = 75)
                                                 ("mean", False, -64, 2), ("size", True, -128, 1),
                                                 # the shipped sets' own widths: component (17, one layer: a 17-column readout),
                                                 # coreness (20, two layers), density / cut_ratio (8)
                                                 ("sum", False, 17, 1), ("mean", False, 20, 2), ("size", True, 8, 1),
                                                 # hidden 128: one layer takes the forward GraphNorm sums through exact accumulators
                                                 # (statistics kernel -> staged comb forward -> readout), two layers do not
                                                 ("size", False, 128, 1), ("sum", True, 128, 2)])
def test_fused_readout_step_matches_autograd_path_and_oracle(pool, multilabel, H, L):
    """stack.loss_and_grads (no tape; final GraphNorm apply + pool + head + loss and their backward as K8r) against
    (a) the autograd path of the same model and (b) the fp64 oracle: loss, logits, every gradient.  The subgraphs
    share nodes and are ragged (padding -1)."""
    from glass_amd import stack, losses
    from glass_amd.arena import ParamArena
    from impl import utils
    from glass_amd import synth
    n, K, B, S = 900, 5, 12, (75 if H < 0 else 9)
    H = abs(H)
    torch.manual_seed(21)
    model = build_glass(H, L, 7, K, "mean", pool, 0.9)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    ei, ew = synth.make_graph(n, 5000, 4, 0.0)
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.integers(0, 8, n)).reshape(n, 1, 1)
    pos = rng.integers(0, 40, (B, S))          # drawn from 40 nodes: heavy sharing between subgraphs
    pos[:, -3:][rng.random((B, 3)) < 0.5] = -1
    if S > 9:
        pos[rng.random((B, S)) < 0.2] = -1      # padding anywhere in a long row
        pos[:, 0] = rng.integers(0, 40, B)
    pos[0, 1:] = -1                            # a single-node subgraph
    pos = torch.from_numpy(pos)
    y = torch.from_numpy((rng.random((B, K)) < 0.4).astype(np.float32)) if multilabel else torch.from_numpy(rng.integers(0, K, B))
    loss_fn = losses.BCEWithLogits() if multilabel else losses.CrossEntropy()
    model.to(DEV).train()
    arena = ParamArena(model)
    xg, eig, ewg, posg, yg = x.to(DEV), torch.from_numpy(ei).to(DEV), torch.from_numpy(ew).to(DEV), pos.to(DEV), y.to(DEV)
    z = utils.MaxZOZ(xg, posg)
    assert stack.step_supported(model, loss_fn)
    arena.zero()
    loss_a, logits_a = stack.loss_and_grads(model, loss_fn, xg, eig, ewg, posg, z, yg)
    grads_a = arena.flat.clone()
    # overwrite mode + labels straight from pos: no zero-fill needed, garbage in the arena must not survive
    assert stack.covers_arena(model, arena)
    arena.flat.fill_(7.0)
    loss_o, _ = stack.loss_and_grads(model, loss_fn, xg, eig, ewg, posg, "pos", yg, overwrite=True)
    assert abs(loss_o.item() - loss_a.item()) < 1e-6 * abs(loss_a.item())
    used = torch.zeros_like(arena.flat, dtype=torch.bool)
    for p_ in arena.params:
        o = arena._offsets[id(p_)]
        used[o:o + p_.numel()] = True
    assert rel_inf(arena.flat[used].cpu(), grads_a[used].cpu()) < 1e-6
    arena.zero()
    pred = model(xg, eig, ewg, posg, z)
    loss_b = loss_fn(pred, yg)
    loss_b.backward()
    assert rel_inf(logits_a.cpu(), pred.detach().cpu()) < 1e-6
    assert abs(loss_a.item() - loss_b.item()) < 1e-6 * abs(loss_b.item())
    assert rel_inf(grads_a.cpu(), arena.flat.cpu()) < 2e-6
    orc = O.OracleGLASS(H, L, 7, K, aggr="mean", pool=pool, z_ratio=0.9)
    orc.load_state_dict(sd)
    orc = orc.double().train()
    po = orc(x, torch.from_numpy(ei), torch.from_numpy(ew).double(), pos, O.max_zero_one(x, pos))
    lo = loss_fn(po, y.double() if multilabel else y)
    lo.backward()
    assert rel_inf(logits_a.cpu(), po.detach()) < TOL and abs(loss_a.item() - lo.item()) < TOL * abs(lo.item())
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    theirs = {k: p.grad for k, p in orc.named_parameters()}
    keys = sorted(mine)
    arena.flat.copy_(grads_a)
    assert rel_inf(flat_grads({k: p.grad.cpu() for k, p in model.named_parameters()}, keys), flat_grads(theirs, keys)) < TOL


# ---------------------------------------------------------------------------------- repeatability / graph safety
def _train_probe(name, hidden, dropout, steps, use_graph=True):
    from glass_amd import synth, losses, ops
    from glass_amd.arena import ParamArena
    from glass_amd.optim import FlatAdam
    from glass_amd.step import TrainStep
    dev = torch.device(DEV)
    w, ei, ew, x, pos, y = synth.make_workload(name, seed=0, n_batches=4)
    ei, ew, x, pos, y = (torch.from_numpy(a).to(dev) for a in (ei, ew, x, pos, y))
    pos[:, 0] = pos[0, 0]  # one node shared by EVERY subgraph of a batch: order-dependent if summed with atomics
    torch.manual_seed(0)
    ops.rng_seed(321, dev)
    model = build_glass(hidden, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio, dropout=dropout).to(dev).train()
    arena = ParamArena(model)
    opt = FlatAdam(arena, lr=1e-2)
    step = TrainStep(model, opt, losses.CrossEntropy(), x, ei, ew, arena, use_graph=use_graph, warmup_iters=2,
                     preserve_state=True)
    B = w.batch
    for k in range(steps):
        b = k % 4
        step(pos[b * B:(b + 1) * B], y[b * B:(b + 1) * B])
    torch.cuda.synchronize()
    return arena.flat_param.clone()


def _train_probe_head(name, hidden, dropout, steps, switch_at=None):
    """_train_probe's run with the labels in the step's HEAD launch (TrainStep.begin_epoch / next_step: prologue || labels,
    the batch named by the device cursor); switch_at: from that step on the eager-label form step(pos, y) again."""
    from glass_amd import synth, losses, ops
    from glass_amd.arena import ParamArena
    from glass_amd.optim import FlatAdam
    from glass_amd.step import TrainStep
    dev = torch.device(DEV)
    w, ei, ew, x, pos, y = synth.make_workload(name, seed=0, n_batches=4)
    ei, ew, x, pos, y = (torch.from_numpy(a).to(dev) for a in (ei, ew, x, pos, y))
    pos[:, 0] = pos[0, 0]
    torch.manual_seed(0)
    ops.rng_seed(321, dev)
    model = build_glass(hidden, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio, dropout=dropout).to(dev).train()
    arena = ParamArena(model)
    opt = FlatAdam(arena, lr=1e-2)
    step = TrainStep(model, opt, losses.CrossEntropy(), x, ei, ew, arena, use_graph=True, warmup_iters=2, preserve_state=True)
    B = w.batch
    idx = torch.arange(4 * B, device=dev).reshape(4, B)
    assert step.begin_epoch(pos, y, idx, wrap=True), "the step program did not take the head-label form"
    losses_seen = []
    for k in range(steps):
        if switch_at is not None and k >= switch_at:
            b = k % 4
            losses_seen.append(step(pos[b * B:(b + 1) * B], y[b * B:(b + 1) * B]).clone())
        else:
            losses_seen.append(step.next_step().clone())
    torch.cuda.synchronize()
    cur = int(step._labels.cursor[5])
    return arena.flat_param.clone(), torch.stack(losses_seen), cur, step


def test_labels_in_the_head_launch_equal_the_eager_label_launch():
    """Round 6: prologue || labels as ONE in-graph launch over a device cursor (glass_step_head_f32).  Same kernels' bodies,
    same order of everything else: 40 steps over 4 cycling batches give BIT-identical parameters to the form with an eager
    label launch in front of every replay; the cursor advanced once per replay; switching back to step(pos, y) mid-run
    (a new capture without the labels in the head) stays on the same trajectory; an exhausted cursor without wrap stays on
    the last batch."""
    ref = _train_probe("tiny", 64, 0.5, 40)
    got, _l, cur, step = _train_probe_head("tiny", 64, 0.5, 40)
    assert step.graphed and step._program_step() and step._labels.in_head
    assert cur == 40, f"cursor at {cur} after 40 replays"
    assert torch.equal(ref, got)
    mixed, _l2, _c, step2 = _train_probe_head("tiny", 64, 0.5, 40, switch_at=20)
    assert not step2._labels.in_head
    assert torch.equal(ref, mixed)


@pytest.mark.parametrize("hidden,switches", [(16, ()), (16, ("USE_GATHER_IN_TRANS", "USE_READOUT_TWO")), (128, ())],
                         ids=["h16", "h16_no_table_no_acc", "h128"])
def test_head_labels_equal_eager_labels_at_other_widths(hidden, switches, monkeypatch):
    """The head-label form against the eager-label form (40 steps, dropout 0.5, bitwise) where the model has no packed weight
    images (hidden 16, the narrow family) and at hidden 128.  With neither the embedding table in layer 0's launch nor
    exact accumulators to zero-fill, hidden 16's prologue carries nothing but the dropout advance: the head launch has to
    do that advance alone, not on top of the one the arena makes for a pack-less model."""
    from glass_amd import stack
    for name in switches:
        monkeypatch.setattr(stack, name, False)
    ref = _train_probe("tiny", hidden, 0.5, 40)
    got, _l, cur, step = _train_probe_head("tiny", hidden, 0.5, 40)
    assert step.graphed and step._program_step() and step._labels.in_head
    assert cur == 40, f"cursor at {cur} after 40 replays"
    assert torch.equal(ref, got)


def test_step_head_labels_match_the_label_launch():
    """glass_step_head_f32 against glass_batch_labels_gather through the C ABI: two batches in a row (incremental label
    bytes), the second one with a duplicate node and a padded tail — label bytes, unique-row list and count, the copied batch
    and targets are identical; the cursor advances, clamps at the last batch without wrap and cycles with it."""
    import numpy as np
    from glass_amd import stack, _lib
    lib = _lib.load()
    dev = torch.device(DEV)
    n, n_all, smax, B = 3000, 40, 7, 8
    rng = np.random.default_rng(5)
    pos_all = torch.from_numpy(rng.integers(0, n, (n_all, smax))).to(dev)
    pos_all[3, 2] = pos_all[5, 1]
    pos_all[::3, -2:] = -1
    y_all = torch.from_numpy(rng.integers(0, 5, (n_all, 1))).to(dev)
    idx = torch.from_numpy(rng.permutation(n_all)[:3 * B].reshape(3, B).astype(np.int64)).to(dev)
    a, b = stack.BatchLabels(n, B * smax, dev), stack.BatchLabels(n, B * smax, dev)
    pa, pb = (torch.full((B, smax), -1, dtype=torch.int64, device=dev) for _ in range(2))
    ya, yb = (torch.zeros((B, 1), dtype=torch.int64, device=dev) for _ in range(2))
    b.set_epoch(pos_all, y_all, idx, pb, yb)
    st = torch.cuda.current_stream().cuda_stream
    for k in range(5):  # batches 0, 1, 2, then the clamp: 2, 2
        a.load_gather(pos_all, y_all, idx[min(k, 2)], pa, ya)
        rc = lib.glass_step_head_f32(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0, 0, 0, *b.head_args(), st)
        assert rc == 0, lib.glass_last_error_string()
        torch.cuda.synchronize()
        assert int(b.cursor[5]) == k + 1
        na = int(a.count[0])
        assert na == int(b.count[0]) and na > 0
        assert torch.equal(a.mask, b.mask) and torch.equal(a.rows[:na], b.rows[:na])
        assert torch.equal(pa, pb) and torch.equal(ya, yb)
        assert torch.equal(b.ws, torch.full_like(b.ws, 2**31 - 1))
    b.set_epoch(pos_all, y_all, idx, pb, yb, wrap=True)
    for k in range(4):  # 0, 1, 2, 0
        rc = lib.glass_step_head_f32(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0, 0, 0, 0, 0, 0, *b.head_args(), st)
        assert rc == 0, lib.glass_last_error_string()
    torch.cuda.synchronize()
    assert torch.equal(pb, pos_all[idx[0]]) and torch.equal(yb, y_all[idx[0]])


@pytest.mark.parametrize("hidden", [16, 64])
def test_training_is_bitwise_repeatable(hidden):
    """The same seeded training twice -> bit-identical parameters, on the per-op path (hidden 16) and on the step
    program (hidden 64: fused readout with its ordered, atomic-free scatter), with dropout and with a node shared by
    all subgraphs of every batch; and the hipGraph replay equals the eager execution of the same step bit for bit."""
    a = _train_probe("tiny", hidden, 0.5, 40)
    b = _train_probe("tiny", hidden, 0.5, 40)
    c = _train_probe("tiny", hidden, 0.5, 40, use_graph=False)
    assert torch.equal(a, b)
    assert torch.equal(a, c)


def test_graph_epochs_with_evaluation_between_match_eager_loop(monkeypatch):
    """impl.train.train replays a captured step; evaluations (eager kernels on other tensors: the validation set's own
    copies of x / edge_index, its own label vectors) run between the epochs.  The captured graph must not depend on
    anything those touch: parameters after 3 epochs equal the plain eager loop's.  (Regression: a hipMemsetAsync NODE
    in the captured MaxZOZ left stale labels behind after such interleaving; an evicted selection CSR would dangle.)"""
    import GLASSTest
    from impl import config, train
    from glass_amd import train as gtrain
    from glass_amd.arena import ParamArena
    from glass_amd.optim import FlatAdam
    config.set_device(0)
    args = GLASSTest.parse_args(["--use_one", "--use_seed", "--use_maxzeroone", "--device", "0", "--dataset", "density"])
    outs = []
    for use_graph in (True, False):
        monkeypatch.setattr(gtrain, "USE_GRAPH", use_graph)
        GLASSTest.set_seed(0)
        run = GLASSTest.Run(args)
        run.split()
        GLASSTest.set_seed(0)
        gnn = run.build_model(8, 1, 0.0, 1, "size", 1.0, "sum")
        arena = ParamArena(gnn)
        opt = FlatAdam(arena, lr=1e-3)
        trn, val, _tst = run.loaders(2)
        scores = []
        for _ in range(3):
            train.train(opt, gnn, trn, run.loss_fn)
            scores.append(train.test(gnn, val, run.score_fn, loss_fn=run.loss_fn)[0])
        torch.cuda.synchronize()
        outs.append((arena.flat_param.clone(), scores))
    assert outs[0][1] == outs[1][1]
    assert rel_inf(outs[0][0].cpu(), outs[1][0].cpu()) < 1e-6


@pytest.mark.parametrize("name", ["ppi_bp", "hpo_neuro", "em_user"])
def test_step_program_full_size_vs_oracle(name):
    """The benchmarked path itself — ParamArena + stack.loss_and_grads (table embedding, fused dense + GraphNorm
    fusion, fused readout, labels from pos, gradients overwritten) — at the full BASELINE shapes (C2 ppi_bp-shaped
    N=17 080 nnz=633 902 mean/sum CE; C3 hpo_neuro-shaped gcn multilabel BCE; C4 em_user-shaped N=50 000 hidden 128
    gcn/size: the column-split dense kernels), dropout 0, against the fp64 oracle: logits, loss, every gradient."""
    from glass_amd import synth, stack, losses
    from glass_amd.arena import ParamArena
    w, ei, ew, x, pos, y = synth.make_workload(name, seed=0, n_batches=1)
    ei, ew, x, pos, y = (torch.from_numpy(a) for a in (ei, ew, x, pos, y))
    torch.manual_seed(0)
    model = build_glass(w.hidden, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    loss_fn = losses.BCEWithLogits() if w.multilabel else losses.CrossEntropy()
    model.to(DEV).train()
    arena = ParamArena(model)
    assert stack.step_supported(model, loss_fn) and stack.covers_arena(model, arena)
    arena.flat.fill_(3.0)  # overwrite mode: stale contents must not survive
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in (x, ei, ew, pos, y))
    loss, logits = stack.loss_and_grads(model, loss_fn, xg, eig, ewg, posg, "pos", yg, overwrite=True)
    res = {}
    for dt in (torch.float64, torch.float32):
        orc = O.OracleGLASS(w.hidden, w.layers, int(x.max()), w.n_class, aggr=w.aggr, pool=w.pool, z_ratio=w.z_ratio)
        orc.load_state_dict(sd)
        orc = orc.to(dt).train()
        po = orc(x, ei, ew.to(dt), pos, O.max_zero_one(x, pos))
        lo = loss_fn(po, y.to(dt) if w.multilabel else y)
        lo.backward()
        res[dt] = (po.detach(), lo.item(), {k: p.grad for k, p in orc.named_parameters()})
    po, lo, theirs = res[torch.float64]
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    keys = sorted(mine)
    e_pred, e_loss = rel_inf(logits.cpu(), po), abs(loss.item() - lo) / abs(lo)
    err = rel_inf(flat_grads(mine, keys), flat_grads(theirs, keys))
    # the fp32 CPU oracle against its own fp64 evaluation: the noise floor of THIS input (the SpMM
    # summation order alone costs ~1e-5 on the gradient at hpo_neuro-shape)
    o_pred, o_grad = rel_inf(res[torch.float32][0], po), rel_inf(flat_grads(res[torch.float32][2], keys), flat_grads(theirs, keys))
    print(f"{name}: step program vs fp64 oracle: logits {e_pred:.2e} grad {err:.2e} | cpu-fp32-vs-fp64 {o_pred:.2e} {o_grad:.2e}")
    record_parity(f"step_program/{name}", logits_rel_inf=e_pred, loss_rel=e_loss, grad_rel_inf=err,
                  oracle_fp32_vs_fp64_logits=o_pred, oracle_fp32_vs_fp64_grad=o_grad)
    assert e_pred < TOL and e_loss < TOL
    assert err < TOL  # plain bar (measured 3e-7 .. 5e-7 at all three shapes)


def test_pretraining_step_full_size_vs_oracle():
    """The link-prediction pre-training step at the size GNNEmb.py runs it — ppi_bp-shaped graph (N = 17 080, nnz = 633 902),
    131 072 node pairs, hidden 64, two MyGCNConv layers, MLP head, BCE — through the per-op path the driver uses (pair-pool
    kernels with the exact backward, thin-output weight gradient, K1, GraphNorm) against the fp64 oracle, dropout 0:
    predictions, loss, every gradient; and the fp32 CPU oracle against fp64 as this input's noise floor."""
    import functools
    from impl import models
    from glass_amd import synth
    w, ei, ew, x, _pos, _y = synth.make_workload("ppi_bp", seed=0, n_batches=1)
    rng = np.random.default_rng(11)
    n_pairs, h, layers = 131072, 64, 2
    pairs = torch.from_numpy(rng.integers(0, w.n_node, size=(n_pairs, 2)))
    y = torch.from_numpy(rng.integers(0, 2, size=n_pairs).astype(np.float32))
    ei, ew, x = (torch.from_numpy(a) for a in (ei, ew, x))
    torch.manual_seed(0)
    conv = models.EmbGConv(h, h, h, layers, max_deg=int(x.max()), activation=nn.ReLU(inplace=True), jk=False, dropout=0.0,
                           conv=functools.partial(models.MyGCNConv, aggr=w.aggr), gn=True)
    head = models.MLP(h, h, 1, 2, dropout=0.0, activation=nn.ReLU(inplace=True))
    model = models.EdgeGNN(conv, nn.ModuleList([head]), nn.ModuleList([models.MeanPool()]))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(DEV).train()
    # the ReLU branches the evaluated path took, in call order (conv 0's trans ReLU, the one behind gns[0], conv 1's, the head's)
    relu_masks, hooks, seen = [], [], set()
    for m in model.modules():
        if isinstance(m, nn.ReLU) and id(m) not in seen:
            seen.add(id(m))
            hooks.append(m.register_forward_hook(lambda _m, _i, out: relu_masks.append((out > 0).cpu())))
    pred = model(x.to(DEV), ei.to(DEV), ew.to(DEV), pairs.to(DEV))
    for hk in hooks:
        hk.remove()
    assert len(relu_masks) == 2 * layers
    loss = nn.BCEWithLogitsLoss()(pred.flatten(), y.to(DEV))
    loss.backward()
    res = {}
    for tag, dt, feed in (("fp64", torch.float64, None), ("fp32", torch.float32, None), ("fp64_same_branches", torch.float64, relu_masks)):
        orc = O.OracleEdgeGNN(h, layers, int(x.max()), aggr=w.aggr, jk=False)
        orc.load_state_dict(sd)
        orc = orc.to(dt).train()
        O.relu_mask_feed(feed or [])
        po = orc(x, ei, ew.to(dt), pairs)
        O.relu_mask_feed([])
        lo = nn.BCEWithLogitsLoss()(po.flatten(), y.to(dt))
        lo.backward()
        res[tag] = (po.detach(), lo.item(), {k: p.grad for k, p in orc.named_parameters()})
    po, lo, theirs = res["fp64_same_branches"]
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    keys = sorted(mine)
    assert keys == sorted(theirs)
    e_pred, e_loss = rel_inf(pred.detach().cpu(), po), abs(loss.item() - lo) / abs(lo)
    err = rel_inf(flat_grads(mine, keys), flat_grads(theirs, keys))
    # What round 3's 4.18e-5 was: ReLU is not differentiable at 0, and among the 8.4 M pre-activations
    # of the MLP head a few lie within fp32 rounding of 0 — there relu' is decided by the sign of the evaluation's own
    # rounding error.  Each flip moves preds.0.seq.modlist.0.{bias,weight} (and, through the pooled rows, the conv weights)
    # by ~1.4e-5 of the largest gradient; the CPU fp32 oracle flips too (its 4.18e-5 was the same elements).  Measured here:
    # against the fp64 evaluation on ITS OWN branches the error is the flips; on the branches the GPU took it is rounding.
    own = res["fp64"]
    err_own = rel_inf(flat_grads(mine, keys), flat_grads(own[2], keys))
    o_pred = rel_inf(res["fp32"][0], own[0])
    o_grad = rel_inf(flat_grads(res["fp32"][2], keys), flat_grads(own[2], keys))
    from helpers import grad_table
    worst = grad_table(mine, own[2], keys, res["fp32"][2])[0]
    print(f"pre-training step vs fp64 oracle on the same ReLU branches: pred {e_pred:.2e} loss {e_loss:.2e} grad {err:.2e} | vs fp64 on "
          f"its own branches: grad {err_own:.2e} (worst {worst[0]} {worst[2]:.2e}; cpu-fp32 there {worst[3]:.2e}) | cpu-fp32-vs-fp64 "
          f"{o_pred:.2e} {o_grad:.2e}")
    record_parity("pretraining_step/ppi_bp_131072_pairs", pred_rel_inf=e_pred, loss_rel=e_loss, grad_rel_inf=err,
                  grad_rel_inf_vs_fp64_on_its_own_relu_branches=err_own, worst_parameter_on_own_branches=worst[0],
                  oracle_fp32_vs_fp64_pred=o_pred, oracle_fp32_vs_fp64_grad=o_grad)
    assert e_pred < TOL and e_loss < TOL
    assert err < TOL


@pytest.mark.parametrize("name", ["ppi_bp", "em_user"])
def test_benchmarked_dropout_step_vs_oracle_on_the_same_masks(name):
    """The benchmarked step WITH its YAML dropout (0.5) at the full BASELINE shapes against the fp64 oracle given the very
    masks the kernels drew: the library writes out the keep-scales of every dropout of the pass (glass_dropout_scales_f32:
    same counter-based hash, same (seed, step) words) and the oracle multiplies by them instead of drawing its own
    (reference impl/models.py:166, 251, 259).  Round 2 could only check dropout-on runs statistically."""
    from glass_amd import synth, stack, losses, ops, _lib
    from glass_amd.arena import ParamArena
    w, ei, ew, x, pos, y = synth.make_workload(name, seed=0, n_batches=1)
    assert w.dropout == 0.5
    ei, ew, x, pos, y = (torch.from_numpy(a) for a in (ei, ew, x, pos, y))
    torch.manual_seed(0)
    model = build_glass(w.hidden, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio, dropout=w.dropout)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    loss_fn = losses.BCEWithLogits() if w.multilabel else losses.CrossEntropy()
    model.to(DEV).train()
    arena = ParamArena(model)
    assert stack.step_supported(model, loss_fn) and stack.covers_arena(model, arena)
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in (x, ei, ew, pos, y))
    ops.rng_seed(2024, DEV)
    loss, logits = stack.loss_and_grads(model, loss_fn, xg, eig, ewg, posg, "pos", yg, overwrite=True)
    # the masks of that pass, in the oracle's call order: emb_gn's dropout (call id 1), then per layer conv.gn's (16 (l+1))
    # and, between layers, the one behind gns[l] (16 (l+1) + 1)
    N, H, L = x.shape[0], w.hidden, w.layers
    ids = [1]
    for l in range(L):
        ids.append(16 * (l + 1))
        if l + 1 < L:
            ids.append(16 * (l + 1) + 1)
    feed = []
    for cid in ids:
        m = torch.empty(N, H, device=DEV)
        _lib.check(_lib.load().glass_dropout_scales_f32(ops.rng_state(DEV).data_ptr(), cid, w.dropout, N, H, m.data_ptr(),
                                                        torch.cuda.current_stream().cuda_stream), "glass_dropout_scales_f32")
        feed.append(m.cpu())
        kept = float((feed[-1] > 0).double().mean())
        assert abs(kept - 0.5) < 0.01 and set(feed[-1].unique().tolist()) == {0.0, 2.0}
    orc = O.OracleGLASS(w.hidden, w.layers, int(x.max()), w.n_class, aggr=w.aggr, pool=w.pool, z_ratio=w.z_ratio,
                        dropout=w.dropout)
    orc.load_state_dict(sd)
    orc = orc.double().train()
    O.mask_feed(feed)
    po = orc(x, ei, ew.double(), pos, O.max_zero_one(x, pos))
    assert not O._MASK_FEED  # every fed mask was consumed, in order
    lo = loss_fn(po, y.double() if w.multilabel else y)
    lo.backward()
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    theirs = {k: p.grad for k, p in orc.named_parameters()}
    keys = sorted(mine)
    e_pred, e_loss = rel_inf(logits.cpu(), po.detach()), abs(loss.item() - lo.item()) / abs(lo.item())
    err = rel_inf(flat_grads(mine, keys), flat_grads(theirs, keys))
    print(f"{name} (dropout 0.5, same masks): logits {e_pred:.2e} loss {e_loss:.2e} grad {err:.2e}")
    record_parity(f"step_program_dropout_same_masks/{name}", logits_rel_inf=e_pred, loss_rel=e_loss, grad_rel_inf=err)
    assert e_pred < TOL and e_loss < TOL and err < TOL


def test_large_batches_stay_exact_and_repeatable():
    """pos matrices beyond the LDS staging of the ordered scatters (readout: B*Smax > 16 384, pool backward:
    > 12 288) take the node-bucketed exact sums (bucket.h) instead of float atomics: no warning, results within tolerance
    of the fp64 oracle AND bitwise equal between two runs (every subgraph shares node 7)."""
    from glass_amd import stack, losses, ops, synth
    from glass_amd.arena import ParamArena
    n, H, L, K, B, S = 3000, 64, 1, 4, 132, 128          # B*S = 16 896
    torch.manual_seed(3)
    model = build_glass(H, L, 5, K, "mean", "sum", 0.8)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    ei, ew = synth.make_graph(n, 9000, 2, 0.0)
    rng = np.random.default_rng(2)
    x = torch.from_numpy(rng.integers(0, 6, n)).reshape(n, 1, 1)
    pos = np.stack([rng.choice(n, S, replace=False) for _ in range(B)])
    pos[:, -40:][rng.random((B, 40)) < 0.5] = -1
    pos[:, 0] = 7                                        # a node shared by every subgraph: its list is summed by a whole workgroup
    pos = torch.from_numpy(pos)
    y = torch.from_numpy(rng.integers(0, K, B))
    loss_fn = losses.CrossEntropy()
    model.to(DEV).train()
    arena = ParamArena(model)
    xg, eig, ewg, posg, yg = x.to(DEV), torch.from_numpy(ei).to(DEV), torch.from_numpy(ew).to(DEV), pos.to(DEV), y.to(DEV)
    import warnings
    arena.zero()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loss, logits = stack.loss_and_grads(model, loss_fn, xg, eig, ewg, posg, "pos", yg)
        first = arena.flat.clone()
        arena.zero()
        loss2, _ = stack.loss_and_grads(model, loss_fn, xg, eig, ewg, posg, "pos", yg)
    assert torch.equal(first, arena.flat) and loss.item() == loss2.item()
    orc = O.OracleGLASS(H, L, 5, K, aggr="mean", pool="sum", z_ratio=0.8)
    orc.load_state_dict(sd)
    orc = orc.double().train()
    po = orc(x, torch.from_numpy(ei), torch.from_numpy(ew).double(), pos, O.max_zero_one(x, pos))
    lo = loss_fn(po, y)
    lo.backward()
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    theirs = {k: p.grad for k, p in orc.named_parameters()}
    keys = sorted(mine)
    assert rel_inf(logits.cpu(), po.detach()) < TOL
    assert rel_inf(flat_grads(mine, keys), flat_grads(theirs, keys)) < TOL
    # pool backward beyond its staging limit, through the per-op op
    emb = torch.randn(n, 32, device=DEV, requires_grad=True)
    out = ops.segment_pool(emb, posg, "mean")
    gout = torch.randn_like(out)
    out.backward(gout)
    e64 = emb.detach().cpu().double().requires_grad_(True)
    valid = (pos >= 0)
    rows = e64[pos.clamp(min=0)] * valid.unsqueeze(-1)                       # [B, S, C]
    r = rows.sum(1) / valid.sum(1).clamp(min=1).unsqueeze(-1)
    r.backward(gout.cpu().double())
    assert rel_inf(out.detach().cpu(), r.detach()) < TOL and rel_inf(emb.grad.cpu(), e64.grad) < TOL


@pytest.mark.parametrize("aggr", ["sum", "mean", "gcn"])
def test_g5_density_step_program_vs_reference_fixture(aggr):
    """Golden fixture g5 (the REFERENCE itself run on the real density graph, fp64: loss, logits, every gradient)
    against the benchmarked form of the step — stack.loss_and_grads with the fused readout, labels from pos,
    gradients overwritten."""
    from glass_amd import stack, losses
    from glass_amd.arena import ParamArena
    g = load(f"g5_density_{aggr}.npz")
    n, ei, ew, x, pos, y, z = density_inputs(g)
    model = build_glass(int(g["hidden"]), int(g["layers"]), int(g["max_deg"]), 3, aggr, str(g["pool"]), float(g["z_ratio"]))
    model.to(DEV).train()
    arena = ParamArena(model)
    model.load_state_dict(sd_from(g))
    loss_fn = losses.CrossEntropy()
    assert stack.step_supported(model, loss_fn) and stack.covers_arena(model, arena)
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in (x, ei, ew, pos, y))
    assert torch.equal(O.max_zero_one(x, pos), z)  # the fixture's labels are the max-zero-one labels of pos
    arena.flat.fill_(-2.0)
    loss, logits = stack.loss_and_grads(model, loss_fn, xg, eig, ewg, posg, "pos", yg, overwrite=True)
    keys = [str(k) for k in g["gnorm64_keys"]]
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    assert rel_inf(logits.cpu(), g["pred64"]) < TOL
    assert abs(loss.item() - float(g["loss64"])) < TOL * abs(float(g["loss64"]))
    assert rel_inf(flat_grads(mine, keys), flat_grads(grads_from(g, "grad64/"), keys)) < TOL


def test_g8_adam_three_steps_through_captured_step_program():
    """Fixture g8 (the reference's losses over three Adam steps and its final weights) against the captured
    training step: TrainStep -> hipGraph replay of stack.loss_and_grads + FlatAdam, warm-up with state restore."""
    from glass_amd import losses as gl
    from glass_amd.arena import ParamArena
    from glass_amd.optim import FlatAdam
    from glass_amd.step import TrainStep
    g = load("g8_adam.npz")
    x = torch.from_numpy(g["x"]).to(DEV)
    ei, ew = torch.from_numpy(g["edge_index"]).to(DEV), torch.from_numpy(g["edge_weight"]).to(DEV)
    pos_all, y_all = torch.from_numpy(g["pos"]).to(DEV), torch.from_numpy(g["y"]).to(DEV)
    model = build_glass(int(g["hidden"]), int(g["layers"]), int(x.max()), 3, str(g["aggr"]), str(g["pool"]),
                        float(g["z_ratio"])).to(DEV).train()
    arena = ParamArena(model)
    model.load_state_dict(sd_from(g))
    opt = FlatAdam(arena, lr=float(g["lr"]))
    step = TrainStep(model, opt, gl.CrossEntropy(), x, ei, ew, arena, use_graph=True, warmup_iters=2, preserve_state=True)
    got = []
    for k in range(3):
        sel = torch.arange(k * 4, k * 4 + 4, device=DEV)
        got.append(float(step(pos_all[sel].contiguous(), y_all[sel].contiguous()).item()))
    assert step.graphed
    assert np.allclose(got, g["losses"], rtol=1e-5, atol=0)
    end = sd_from(g, "sd_end/")
    keys = sorted(end)
    mine = {k: v.cpu() for k, v in model.state_dict().items()}
    assert rel_inf(flat_grads(mine, keys), flat_grads(end, keys)) < 1e-4


def test_step_program_at_c5_scale_matches_per_op_path(monkeypatch):
    """N = 1 M nodes, nnz = 20 M (power-law, long rows -> all three K1 kernels), hidden 64: the step program (stats from
    15 625 producer workgroups, fused readout) against the per-op autograd path of the same model on the GPU — loss,
    logits and the flat gradient; and bitwise repeatable.  (Size-independent property check; the CPU oracle is not
    run at this size.)"""
    from glass_amd import synth, stack, losses, models as gm
    from glass_amd.arena import ParamArena
    from impl import utils
    ei, ew, x, pos, y = _c5_graph()
    torch.manual_seed(0)
    V = int(x.max()) + 1
    model = build_glass(64, 2, V - 1, 6, "mean", "sum", 0.9).to(DEV).train()
    arena = ParamArena(model)
    loss_fn = losses.CrossEntropy()
    assert stack.step_supported(model, loss_fn)
    arena.zero()
    loss_a, logits_a = stack.loss_and_grads(model, loss_fn, x, ei, ew, pos, "pos", y)
    ga = arena.flat.clone()
    arena.zero()
    loss_a2, _ = stack.loss_and_grads(model, loss_fn, x, ei, ew, pos, "pos", y)
    assert torch.equal(arena.flat, ga) and torch.equal(loss_a, loss_a2)
    monkeypatch.setattr(gm, "USE_STACK", False)
    arena.zero()
    pred = model(x, ei, ew, pos, utils.MaxZOZ(x, pos))
    loss_b = loss_fn(pred, y)
    loss_b.backward()
    assert torch.isfinite(loss_a) and rel_inf(logits_a.cpu(), pred.detach().cpu()) < TOL
    assert abs(loss_a.item() - loss_b.item()) < TOL * abs(loss_b.item())
    assert rel_inf(ga.cpu(), arena.flat.cpu()) < 2 * TOL



_C5 = {}


def _c5_graph():
    """BASELINE config 5's graph (power-law, N = 1 M, nnz = 20 M), generated once per test session."""
    from glass_amd import synth
    if not _C5:
        w = synth.WORKLOADS["powerlaw"]
        ei, ew = synth.make_graph(w.n_node, w.n_pairs, 0, w.powerlaw)
        x = synth.degree_feature(ei, w.n_node)
        pos, y = synth.make_subgraphs(w.n_node, w.batch, w.sub_size, w.n_class, 1, False)
        _C5["data"] = tuple(torch.from_numpy(a).to(DEV) for a in (ei, ew, x, pos, y))
    return _C5["data"]


def _product_step(model, arena, loss_fn, x, ei, ew, pos, y):
    """loss and flat gradient of one step through the PRODUCT'S OWN dispatch (step.TrainStep._fwd_bwd picks the step
    program or the per-op path exactly as a training run would), eager, no optimizer step."""
    from glass_amd.step import TrainStep
    from glass_amd.optim import FlatAdam
    ts = TrainStep(model, FlatAdam(arena, lr=1e-3), loss_fn, x, ei, ew, arena, use_graph=False, warmup_iters=0)
    ts._pos, ts._y = pos.clone(), y.clone()
    ts._fwd_bwd()
    torch.cuda.synchronize()
    return ts._loss.detach().clone(), arena.flat.clone()


def test_c5_family_hidden256_vs_oracle():
    """BASELINE config 5's family at a size the fp64 oracle finishes in seconds: power-law graph (N = 20 000,
    nnz = 400 000, Zipf 0.8: hub rows far beyond one 2 048-edge chunk -> sweep + workgroup + reduce kernels of K1),
    hidden = 256, 2 layers, mean / sum, through whatever path the product selects for hidden 256 — against the fp64
    oracle on logits, loss and the flat gradient."""
    from glass_amd import synth, losses
    from glass_amd.arena import ParamArena
    from impl import utils
    n, pairs, H, L, K = 20000, 200000, 256, 2, 6
    ei, ew = synth.make_graph(n, pairs, 5, 0.8)
    x = synth.degree_feature(ei, n)
    pos, y = synth.make_subgraphs(n, 48, 24, K, 3, False)
    deg = np.bincount(ei[0], minlength=n)
    assert deg.max() > 2048
    ei, ew, x, pos, y = (torch.from_numpy(a) for a in (ei, ew, x, pos, y))
    torch.manual_seed(0)
    model = build_glass(H, L, int(x.max()), K, "mean", "sum", 0.9)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    loss_fn = losses.CrossEntropy()
    model.to(DEV).train()
    arena = ParamArena(model)
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in (x, ei, ew, pos, y))
    loss, grad = _product_step(model, arena, loss_fn, xg, eig, ewg, posg, yg)
    mine = {k: p.grad.detach().cpu().clone() for k, p in model.named_parameters()}
    with torch.no_grad():
        logits = model(xg, eig, ewg, posg, utils.MaxZOZ(xg, posg))
    res = {}
    for dt in (torch.float64, torch.float32):
        orc = O.OracleGLASS(H, L, int(x.max()), K, aggr="mean", pool="sum", z_ratio=0.9)
        orc.load_state_dict(sd)
        orc = orc.to(dt).train()
        po = orc(x, ei, ew.to(dt), pos, O.max_zero_one(x, pos))
        lo = loss_fn(po, y)
        lo.backward()
        res[dt] = (po.detach(), lo.item(), {k: p.grad for k, p in orc.named_parameters()})
    po, lo, theirs = res[torch.float64]
    keys = sorted(mine)
    e_pred, e_loss = rel_inf(logits.cpu(), po), abs(loss.item() - lo) / abs(lo)
    e_grad = rel_inf(flat_grads(mine, keys), flat_grads(theirs, keys))
    o_pred = rel_inf(res[torch.float32][0], po)
    o_grad = rel_inf(flat_grads(res[torch.float32][2], keys), flat_grads(theirs, keys))
    print(f"C5 family H=256: logits {e_pred:.2e} loss {e_loss:.2e} grad {e_grad:.2e} | cpu-fp32-vs-fp64 {o_pred:.2e} {o_grad:.2e}")
    record_parity("product_dispatch/powerlaw_family_N20000_hidden256", logits_rel_inf=e_pred, loss_rel=e_loss,
                  grad_rel_inf=e_grad, oracle_fp32_vs_fp64_logits=o_pred, oracle_fp32_vs_fp64_grad=o_grad)
    assert e_pred < TOL and e_loss < TOL and e_grad < TOL  # plain bar (measured 3.4e-7)


def test_c5_family_quarter_size_vs_fp64_oracle():
    """BASELINE config 5's family at the largest size whose fp64 CPU evaluation finishes inside a test:
    the power-law generator of config 5 at N = 250 000 / nnz = 5 M, hidden 256, BOTH layers, through the step program,
    against the fp64 oracle on logits, loss and the flat gradient (round 3 had this only as an off-suite tool record:
    logits 5.6e-7, gradient 4.7e-7).  Needs ~56 GiB of host memory for the fp64 tape (the GPU box has 3 TB)."""
    import time
    import psutil
    from glass_amd import synth, stack, losses
    from glass_amd.arena import ParamArena
    if psutil.virtual_memory().available < 56 * 2**30:
        pytest.skip("fp64 tape of the N = 250 000 evaluation needs ~56 GiB of host memory")
    w = synth.WORKLOADS["powerlaw"]
    n_node, n_pairs = 250_000, 2_500_000
    ei, ew = synth.make_graph(n_node, n_pairs, 0, w.powerlaw)
    x = synth.degree_feature(ei, n_node)
    pos, y = synth.make_subgraphs(n_node, w.batch, w.sub_size, w.n_class, 1, w.multilabel)
    ei, ew, x, pos, y = (torch.from_numpy(a) for a in (ei, ew, x, pos, y))
    torch.manual_seed(0)
    model = build_glass(w.hidden, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio)
    assert w.hidden == 256 and w.layers == 2
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    loss_fn = losses.CrossEntropy()
    model.to(DEV).train()
    arena = ParamArena(model)
    assert stack.step_supported(model, loss_fn) and stack.covers_arena(model, arena)
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in (x, ei, ew, pos, y))
    loss, logits = stack.loss_and_grads(model, loss_fn, xg, eig, ewg, posg, "pos", yg, overwrite=True)
    torch.cuda.synchronize()
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    keys = sorted(mine)
    t0 = time.time()
    threads = torch.get_num_threads()
    torch.set_num_threads(__import__("os").cpu_count())
    try:
        orc = O.OracleGLASS(w.hidden, w.layers, int(x.max()), w.n_class, aggr=w.aggr, pool=w.pool, z_ratio=w.z_ratio)
        orc.load_state_dict(sd)
        orc = orc.double().train()
        po = orc(x, ei, ew.double(), pos, O.max_zero_one(x, pos))
        lo = loss_fn(po, y)
        lo.backward()
    finally:
        torch.set_num_threads(threads)
    theirs = {k: p.grad for k, p in orc.named_parameters()}
    e_pred, e_loss = rel_inf(logits.cpu(), po.detach()), abs(loss.item() - lo.item()) / abs(lo.item())
    e_grad = rel_inf(flat_grads(mine, keys), flat_grads(theirs, keys))
    print(f"C5 family N=250k H=256 L=2 vs fp64 oracle ({time.time() - t0:.0f} s of CPU): logits {e_pred:.2e} loss {e_loss:.2e} grad {e_grad:.2e}")
    record_parity("config5_family/powerlaw_N250k_hidden256_L2_vs_fp64_in_suite", n_node=n_node, nnz=ei.shape[1], logits_rel_inf=e_pred,
                  loss_rel=e_loss, grad_rel_inf=e_grad, oracle_seconds=time.time() - t0)
    assert e_pred < TOL and e_loss < TOL and e_grad < TOL


def test_c5_full_size_hidden256_step(monkeypatch):
    """BASELINE config 5 at its own size and width (N = 1 M, nnz = 20 M, hidden = 256, 2 layers, mean / sum, batch
    64 x 32): the step through the product's dispatch is finite, bitwise repeatable, and equals (<= 2e-5 rel-inf on
    loss, logits and the flat gradient) the same step with every fusion switched off (per-op autograd path, library
    GEMMs + stand-alone mix / GraphNorm kernels).  The CPU oracle is not run at this size: size-independent property."""
    from glass_amd import synth, stack, losses, ops, models as gm
    from glass_amd.arena import ParamArena
    from impl import utils
    w = synth.WORKLOADS["powerlaw"]
    ei, ew, x, pos, y = _c5_graph()
    torch.manual_seed(0)
    model = build_glass(w.hidden, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio).to(DEV).train()
    assert w.hidden == 256
    arena = ParamArena(model)
    loss_fn = losses.CrossEntropy()
    loss_a, ga = _product_step(model, arena, loss_fn, x, ei, ew, pos, y)
    loss_a2, ga2 = _product_step(model, arena, loss_fn, x, ei, ew, pos, y)
    assert torch.isfinite(loss_a) and bool(torch.isfinite(ga).all())
    assert torch.equal(ga, ga2) and torch.equal(loss_a, loss_a2)
    with torch.no_grad():
        logits_a = model(x, ei, ew, pos, utils.MaxZOZ(x, pos))
    used_program = stack.step_supported(model, loss_fn)
    # every fusion off: no step program, no fused dense kernels, no table embedding, no fused readout
    monkeypatch.setattr(gm, "USE_STACK", False)
    monkeypatch.setattr(ops, "USE_FUSED_DENSE", False)
    monkeypatch.setattr(stack, "USE_EMBED_TABLE", False)
    monkeypatch.setattr(stack, "USE_READOUT", False)
    assert not stack.step_supported(model, loss_fn)
    arena.zero()
    pred = model(x, ei, ew, pos, utils.MaxZOZ(x, pos))
    loss_b = loss_fn(pred, y)
    loss_b.backward()
    torch.cuda.synchronize()
    e_pred = rel_inf(logits_a.cpu(), pred.detach().cpu())
    e_loss = abs(loss_a.item() - loss_b.item()) / abs(loss_b.item())
    e_grad = rel_inf(ga.cpu(), arena.flat.cpu())
    print(f"C5 full size H=256 (step program: {used_program}): fused vs unfused logits {e_pred:.2e} loss {e_loss:.2e} grad {e_grad:.2e}")
    record_parity("product_dispatch/powerlaw_N1M_hidden256_fused_vs_unfused", logits_rel_inf=e_pred, loss_rel=e_loss,
                  grad_rel_inf=e_grad, step_program=bool(used_program), bitwise_repeatable=True)
    assert e_pred < 2 * TOL and e_loss < 2 * TOL and e_grad < 2 * TOL


def test_detached_grads_fall_back_to_autograd():
    """with a ParamArena attached, optimizer.zero_grad() (set_to_none=True, torch's default) detaches
    .grad from the arena.  The per-op path must then hand every Linear-pair gradient back through autograd instead of
    writing it to the (now unread) arena: all parameters get a gradient equal to the oracle's."""
    from glass_amd import synth, losses, stack
    from glass_amd.arena import ParamArena
    from impl import utils
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=4, n_batches=1)
    ei, ew, x, pos, y = (torch.from_numpy(a) for a in (ei, ew, x, pos, y))
    torch.manual_seed(0)
    model = build_glass(64, 2, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    model.to(DEV).train()
    ParamArena(model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt.zero_grad()  # set_to_none=True: every .grad is now None
    assert all(p.grad is None for p in model.parameters())
    assert not stack.StackProgram.supported(model.conv)
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in (x, ei, ew, pos, y))
    loss = nn.CrossEntropyLoss()(model(xg, eig, ewg, posg, utils.MaxZOZ(xg, posg)), yg)
    loss.backward()
    assert all(p.grad is not None for p in model.parameters())
    orc = O.OracleGLASS(64, 2, int(x.max()), w.n_class, aggr=w.aggr, pool=w.pool, z_ratio=w.z_ratio)
    orc.load_state_dict(sd)
    orc = orc.double().train()
    lo = nn.CrossEntropyLoss()(orc(x, ei, ew.double(), pos, O.max_zero_one(x, pos)), y)
    lo.backward()
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    theirs = {k: p.grad for k, p in orc.named_parameters()}
    keys = sorted(mine)
    assert rel_inf(flat_grads(mine, keys), flat_grads(theirs, keys)) < TOL


@pytest.mark.parametrize("arena", [False, True])
def test_several_training_forwards_before_backward_with_dropout(arena):
    """Dropout masks are regenerated in the backward pass from the (seed, step) words of THEIR forward: every training
    forward on the autograd paths keeps a private snapshot, so two forwards may precede the backwards (gradient
    accumulation; round 2 refused this).  The accumulated gradient must equal the sum of the two passes run one at a
    time from the same dropout words.  arena=False: per-op path; True: the stack program as one autograd node."""
    from glass_amd import synth, ops
    from glass_amd.arena import ParamArena
    from impl import utils
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=5, n_batches=2)
    ei, ew, x, pos, y = (torch.from_numpy(a).to(DEV) for a in (ei, ew, x, pos, y))
    B = w.batch
    torch.manual_seed(0)
    model = build_glass(64 if arena else w.hidden, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio,
                        dropout=0.3).to(DEV).train()
    if arena:
        ParamArena(model)
    params = [p for p in model.parameters()]
    loss = nn.CrossEntropyLoss()
    batches = [(pos[:B], y[:B]), (pos[B:2 * B], y[B:2 * B])]

    def grads_of(fn):
        for p in params:
            if p.grad is not None:
                p.grad.zero_()
        fn()
        return torch.cat([p.grad.reshape(-1).clone() for p in params])

    def both_then_backward():
        ops.rng_seed(77, DEV)
        ls = [loss(model(x, ei, ew, ps, utils.MaxZOZ(x, ps)), ys) for ps, ys in batches]  # two forwards ...
        ls[0].backward()                                                                   # ... then the backwards,
        ls[1].backward()                                                                   # oldest first

    def one_at_a_time():
        ops.rng_seed(77, DEV)
        for ps, ys in batches:   # the stream advances once per training forward either way: same (seed, step) per pass
            loss(model(x, ei, ew, ps, utils.MaxZOZ(x, ps)), ys).backward()

    g_acc, g_seq = grads_of(both_then_backward), grads_of(one_at_a_time)
    assert float(g_seq.abs().max()) > 0
    assert torch.equal(g_acc, g_seq)   # same kernels, same masks, same accumulation order


def test_node_emb_over_two_feature_channels_trains_with_dropout():
    """GLASS.NodeEmb loops self.conv over the feature channels and averages (reference impl/models.py:336-344): with
    dropout on, every channel's pass draws its own masks and its backward regenerates exactly those.  For a loss that is
    linear in the node embedding, the gradient of the 2-channel model is the mean of the two single-channel gradients
    taken from the same dropout words."""
    from glass_amd import synth, ops
    from glass_amd.arena import ParamArena
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=6, n_batches=1)
    ei, ew, x = (torch.from_numpy(a).to(DEV) for a in (ei, ew, x))
    torch.manual_seed(1)
    model = build_glass(64, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio, dropout=0.3).to(DEV).train()
    ParamArena(model)
    params = list(model.conv.parameters())
    xb = x.flip(0)                                   # a second feature channel: the same table rows, other nodes
    x2 = torch.cat([x, xb], dim=1)                   # [N, 2, 1]
    z = (torch.arange(x.shape[0], device=DEV) % 7 == 0).to(torch.int64)
    R = torch.randn(x.shape[0], model.conv.gns[-1].weight.shape[0], device=DEV)

    def grads(fn):
        for p in params:
            p.grad.zero_()
        fn()
        return torch.cat([p.grad.reshape(-1).clone() for p in params])

    def two_channels():
        ops.rng_seed(5, DEV)
        (model.NodeEmb(x2, ei, ew, z) * R).sum().backward()

    def channel(k, xc):
        def run():
            ops.rng_seed(5, DEV)
            ops.rng_state(DEV)[1] = k                # the k-th training forward since the seed
            (model.NodeEmb(xc, ei, ew, z) * R).sum().backward()
        return run

    g2, ga, gb = grads(two_channels), grads(channel(0, x)), grads(channel(1, xb))
    ref = 0.5 * (ga.double() + gb.double())
    assert float(ref.abs().max()) > 0
    assert rel_inf(g2.double(), ref) < 1e-5


def test_label_vector_dtypes_and_shapes():
    """z may arrive as int64 [N] (MaxZOZ), but also as a float / bool / [N,1] tensor: the reference thresholds it at
    0.5 whatever it is (impl/models.py:243-248)."""
    emb, arena, _orc, (x, ei, ew, z), _g = _emb_pair(1, 1, "mean", 0.8, 0.0, seed=2)
    emb.eval()
    args = [t.to(DEV) for t in (x, ei, ew)]
    zg = z.to(DEV)
    with torch.no_grad():
        ref = emb(*args, zg)
        for variant in (zg.to(torch.float32) * 0.9, zg.bool(), zg.reshape(-1, 1), zg.to(torch.int32), zg.double() + 0.3 * (1 - zg.double())):
            assert torch.equal(emb(*args, variant), ref)
        with pytest.raises(ValueError):
            emb(*args, zg[:-1])


def test_split_step_with_rccl_allreduce_on_one_rank():
    """The N>1 forms of the step on a 1-rank RCCL group, in a subprocess: (a) captured forward/backward + eager RCCL
    all-reduce(AVG) of the gradient arena + eager fused Adam; (b) with an embedding-sized bucket: two graphs cut where
    the small bucket is final, its all-reduce on a second stream beside the tail of the backward, reduce-scatter +
    sharded Adam + all-gather for the table.  Both bit-identical in parameters to the single-process form."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import socket
    with socket.socket() as sk:   # a free port, not a fixed one: two test runs on one box must not collide
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "dist_step_probe.py")], capture_output=True, text=True,
                         timeout=600, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "ALL EQUAL" in out.stdout and "DIFFERENT" not in out.stdout, out.stdout[-500:]


def test_step_program_randomised_configurations():
    """tools/fuzz_step_program.py: 12 random configurations (hidden 64 / 128, 1-3 layers, all aggregations and fusable
    pools, CE / BCE, uniform and power-law graphs with random edge weights, ragged subgraphs with repeated nodes) of the
    step program against the fp64 oracle, rel-inf <= 1e-5 on logits, loss and the flat gradient."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_step_program.py"), "12", "2024"],
                         capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]


@pytest.mark.parametrize("flags,overlapped", [(["--workload", "ppi_bp"], False),
                                              (["--workload", "em_user", "--features", "nodeid"], True)])
def test_bench_two_ranks_share_the_gpu_over_gloo(flags, overlapped):
    """`bench.py --gpus 2` end to end on the 1-GPU box: the launcher starts two ranks that share cuda:0 and exchange over
    gloo (GLASS_BENCH_BACKEND=gloo; RCCL refuses two ranks on one device).  use_deg features: one small bucket,
    all-reduced.  use_nodeid features at em_user-shape: the 25.6 MB embedding gradient forms the big bucket — two graphs
    cut at the tail hook, small all-reduce on the communication stream, reduce-scatter + sharded Adam + all-gather.
    Timings over gloo mean nothing; the line must be complete, n_gpus 2, the loss finite."""
    import json
    import math
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(GLASS_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "10", "--warmup", "3", "--full",
                          "--no-cpu-baseline", "--no-roofline-hbm", *flags], capture_output=True, text=True, timeout=900,
                         env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 10 and d["scaling"] == "weak" and d["value"] > 0
    assert math.isfinite(d["config"]["final_loss"])
    c = d["collective"]
    assert c["world"] == 2 and c["small_bucket_overlaps_backward_tail"] is overlapped
    assert (c["payload_bytes"]["big_reduce_scatter"] > 0) is overlapped and c["payload_bytes"]["small_allreduce"] > 0


def test_bench_plain_run_times_exactly_steps_and_dumps_the_last_step(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` run: one timed block of exactly K steps and the headline line only
    (none of the --full parts); --dump-outputs writes the last step's loss, parameters and gradients (float32, <= 64 MiB),
    and a second run with the same arguments writes the same arrays."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    lines = []
    for run in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3",
                              "--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=600, env=env, cwd=root)
        assert out.returncode == 0, out.stderr[-3000:]
        js = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(js) == 1, out.stdout[-2000:]
        lines.append(json.loads(js[0]))
    d = lines[0]
    assert d["steps"] == 7 and d["warmup"] == 3 and d["n_gpus"] == 1 and d["value"] > 0 and d["config"]["hip_graph"]
    assert d["unit"] == "edges/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert abs(d["ms_per_step"] - d["timed_region_s"] * 1e3 / 7) <= 1e-9 * d["ms_per_step"]
    assert not {"roofline", "roofline_hbm", "step_breakdown", "step_floor", "cpu_baseline", "blocks"} & set(d)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b")) and "loss.npy" in files
    assert any(f.startswith("param.") for f in files) and any(f.startswith("grad.") for f in files)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [np.float32(d["config"]["final_loss"])]
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and a.shape == b.shape and np.isfinite(a).all(), f
        assert np.abs(a - b).max() <= 1e-4 * max(np.abs(b).max(), 1e-30), f


def test_eval_graph_parallel_branches_match_eager_forward():
    """evalstep.EvalGraph (train.test's forward passes as K parallel branches of one hipGraph behind a shared prologue):
    every branch returns bit for bit what the eager forward returns for its batch, for K = 1 .. 4, on a graph whose K1 plan
    has long rows (per-branch partial-row workspaces) — and train.test gives the same score and loss with and without it."""
    from glass_amd import synth, train as gtrain
    from glass_amd.evalstep import EvalGraph
    from glass_amd.arena import ParamArena
    from impl import SubGDataset, utils, metrics
    n = 20000
    ei, ew = synth.make_graph(n, 150000, 3, 0.9)   # Zipf 0.9: hub rows beyond one chunk
    x = synth.degree_feature(ei, n)
    pos, y = synth.make_subgraphs(n, 16 * 9 + 5, 10, 4, 1, False)
    ei, ew, x, pos, y = (torch.from_numpy(a).to(DEV) for a in (ei, ew, x, pos, y))
    torch.manual_seed(0)
    model = build_glass(64, 2, int(x.max()), 4, "mean", "sum", 0.9).to(DEV)
    ParamArena(model)
    model.eval()
    B = 16
    with torch.no_grad():
        eager = [model(x, ei, ew, pos[b * B:(b + 1) * B], utils.MaxZOZ(x, pos[b * B:(b + 1) * B])).clone() for b in range(8)]
        for k in (1, 2, 3, 4):
            g = EvalGraph(model, x, ei, ew, (B, pos.shape[1]), k).capture()
            for start in range(0, 8, k):
                grp = list(range(start, min(start + k, 8)))
                outs = g([pos[b * B:(b + 1) * B] for b in grp])
                for b, o in zip(grp, outs):
                    assert torch.equal(o, eager[b]), (k, b)
    ds = SubGDataset.GDataset(x, ei, ew, pos, y)
    loader = SubGDataset.ZGDataloader(ds, B, z_fn=utils.MaxZOZ, shuffle=False, drop_last=False)  # 9 full batches + a tail of 5
    loss_fn = nn.CrossEntropyLoss()
    a = gtrain.test(model, loader, metrics.microf1, loss_fn)
    assert model.__dict__.get("_glass_eval_graphs")
    old = gtrain.USE_EVAL_GRAPH
    gtrain.USE_EVAL_GRAPH = False
    try:
        b = gtrain.test(model, loader, metrics.microf1, loss_fn)
    finally:
        gtrain.USE_EVAL_GRAPH = old
    assert a[0] == b[0] and torch.equal(a[1], b[1])


def test_dropped_multi_branch_eval_graphs_do_not_crash_later_replays():
    """Regression for a host crash inside hipGraphLaunch (hip::Graph::UpdateStreams) after a hipGraphExec with parallel
    branches had been destroyed: evalstep parks such execs instead of destroying them (evalstep._RETIRED).  Create / replay /
    drop / collect six times, replaying a freshly captured multi-branch graph each round."""
    import gc
    from glass_amd import synth, evalstep
    from glass_amd.evalstep import EvalGraph
    from glass_amd.arena import ParamArena
    from impl import utils
    n = 3000
    ei, ew = synth.make_graph(n, 20000, 5, 0.5)
    x = synth.degree_feature(ei, n)
    pos, _y = synth.make_subgraphs(n, 64, 8, 3, 1, False)
    ei, ew, x, pos = (torch.from_numpy(a).to(DEV) for a in (ei, ew, x, pos))
    parked = len(evalstep._RETIRED)
    reserved = []
    for it in range(6):
        torch.manual_seed(it)
        model = build_glass(64, 1, int(x.max()), 3, "sum", "mean", 0.8).to(DEV)
        ParamArena(model)
        model.eval()
        with torch.no_grad():
            want = [model(x, ei, ew, pos[8 * b:8 * b + 8], utils.MaxZOZ(x, pos[8 * b:8 * b + 8])).clone() for b in range(4)]
            g = EvalGraph(model, x, ei, ew, (8, pos.shape[1]), 4).capture()
            outs = g([pos[8 * b:8 * b + 8] for b in range(4)])
            torch.cuda.synchronize()
            assert all(torch.equal(o, w) for o, w in zip(outs, want))
        del g, outs, model
        gc.collect()
        reserved.append(torch.cuda.memory_reserved())
    assert len(evalstep._RETIRED) >= parked + 6  # (earlier tests' graphs may be collected here as well)
    # parked execs pin no memory of their own: every evaluation graph captures into one shared pool, so after the first
    # rounds the reserved memory stops growing
    assert reserved[-1] <= reserved[2] + (8 << 20), reserved
