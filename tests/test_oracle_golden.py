"""Pin the CPU oracle (oracle/glass_oracle.py) to vectors produced by the reference itself
(tests/golden/make_golden.py) and to the reference's docstring examples."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from helpers import load, sd_from, grads_from, rel_inf, flat_grads, density_inputs
from oracle import glass_oracle as O

TOL = 1e-5  # north_star: 1e-5 relative fp32 (rel-inf)


def test_docstring_examples():
    # impl/utils.py:9  batch [0,1,0,0,1,1,2,2] -> pad [[0,2,3],[1,4,5],[6,7,-1]]
    pad = O.batch_to_pad(torch.tensor([0, 1, 0, 0, 1, 1, 2, 2]))
    assert pad.tolist() == [[0, 2, 3], [1, 4, 5], [6, 7, -1]]
    # impl/utils.py:21 (inverse; row-major order)
    b, p = O.pad_to_batch(pad)
    assert b.tolist() == [0, 0, 0, 1, 1, 1, 2, 2]
    assert p.tolist() == [0, 2, 3, 1, 4, 5, 6, 7]
    # impl/models.py:288-289 batch-vector comment: nodes 0,2,3 -> subgraph 0, ...
    emb = torch.arange(8, dtype=torch.float32).reshape(8, 1)
    out = O.segment_pool(emb, torch.tensor([0, 1, 0, 0, 1, 1, 2, 2]), 3, "sum")
    assert out.reshape(-1).tolist() == [0 + 2 + 3, 1 + 4 + 5, 6 + 7]


def test_g6_utils():
    g = load("g6_utils.npz")
    assert np.array_equal(O.batch_to_pad(torch.from_numpy(g["batch"])).numpy(), g["pad"])
    b, p = O.pad_to_batch(torch.from_numpy(g["pad"]))
    assert np.array_equal(b.numpy(), g["p2b_batch"]) and np.array_equal(p.numpy(), g["p2b_pos"])
    z = O.max_zero_one(torch.zeros(int(g["mz_n"]), 1, 1), torch.from_numpy(g["mz_pos"]))
    assert np.array_equal(z.numpy(), g["mz_z"])


@pytest.mark.parametrize("aggr", ["mean", "sum", "gcn"])
def test_g1_buildadj(aggr):
    g = load("g1_buildadj.npz")
    ei, ew = torch.from_numpy(g["edge_index"]), torch.from_numpy(g["edge_weight"])
    a = O.dense_adj(ei, ew, int(g["n_node"]), aggr)
    assert rel_inf(a, g["A_" + aggr]) < 1e-6
    assert rel_inf(O.build_adj(ei, ew, int(g["n_node"]), aggr).to_dense(), g["A_" + aggr]) < 1e-6


@pytest.mark.parametrize("aggr", ["mean", "sum", "gcn"])
def test_g2_conv(aggr):
    g = load(f"g2_conv_{aggr}.npz")
    conv = O.OracleConv(8, 8, aggr, float(g["z_ratio"]), 0.0)
    conv.load_state_dict(sd_from(g))
    x = torch.from_numpy(g["x"]).requires_grad_(True)
    y = conv(x, torch.from_numpy(g["edge_index"]), torch.from_numpy(g["edge_weight"]),
             torch.from_numpy(g["mask"]).reshape(-1, 1), torch.nn.functional.elu)
    (y * torch.from_numpy(g["gout"])).sum().backward()
    assert rel_inf(y.detach(), g["y"]) < TOL
    assert rel_inf(x.grad, g["grad_x"]) < TOL
    ref = grads_from(g)
    mine = {k: p.grad for k, p in conv.named_parameters()}
    keys = sorted(ref)
    assert sorted(mine) == keys
    assert rel_inf(flat_grads(mine, keys), flat_grads(ref, keys)) < TOL
    # math pin: oracle.double() vs the reference module evaluated in float64
    conv64 = O.OracleConv(8, 8, aggr, float(g["z_ratio"]), 0.0).double()
    conv64.load_state_dict({k: v.double() for k, v in sd_from(g).items()})
    x64 = torch.from_numpy(g["x"]).double().requires_grad_(True)
    y64 = conv64(x64, torch.from_numpy(g["edge_index"]), torch.from_numpy(g["edge_weight"]),
                 torch.from_numpy(g["mask"]).reshape(-1, 1), torch.nn.functional.elu)
    (y64 * torch.from_numpy(g["gout"]).double()).sum().backward()
    assert rel_inf(y64.detach(), g["y64"]) < 1e-12
    assert rel_inf(x64.grad, g["grad_x64"]) < 1e-12
    ref64 = grads_from(g, "grad64/")
    assert rel_inf(flat_grads({k: p.grad for k, p in conv64.named_parameters()}, keys), flat_grads(ref64, keys)) < 1e-12


@pytest.mark.parametrize("layers", [1, 2, 3])
@pytest.mark.parametrize("jk", [0, 1])
def test_g3_emb(layers, jk):
    g = load(f"g3_emb_L{layers}_jk{jk}.npz")
    h = int(g["hidden"])
    emb = O.OracleEmbZGConv(h, h, layers, 5, 0.0, str(g["aggr"]), float(g["z_ratio"]), jk=bool(jk))
    emb.load_state_dict(sd_from(g))
    emb.eval()
    args = (torch.from_numpy(g["x"]), torch.from_numpy(g["edge_index"]), torch.from_numpy(g["edge_weight"]))
    assert rel_inf(emb(*args, torch.from_numpy(g["z"])).detach(), g["y"]) < TOL
    for c in emb.convs:
        c.adj = None
    assert rel_inf(emb(*args, None).detach(), g["y_noz"]) < TOL
    emb64 = O.OracleEmbZGConv(h, h, layers, 5, 0.0, str(g["aggr"]), float(g["z_ratio"]), jk=bool(jk)).double()
    emb64.load_state_dict({k: v.double() for k, v in sd_from(g).items()})
    emb64.eval()
    assert rel_inf(emb64(*args, torch.from_numpy(g["z"])).detach(), g["y64"]) < 1e-12


@pytest.mark.parametrize("mode", ["sum", "mean", "max", "size"])
def test_g4_pool(mode):
    g = load("g4_pool.npz")
    e = torch.from_numpy(g["emb"]).requires_grad_(True)
    batch, pos = O.pad_to_batch(torch.from_numpy(g["pos"]))
    y = O.segment_pool(e[pos], batch, int(batch.max()) + 1, mode)
    (y * torch.from_numpy(g["gout"])).sum().backward()
    assert rel_inf(y.detach(), g["y_" + mode]) < 1e-6
    assert rel_inf(e.grad, g["grad_" + mode]) < 1e-6


def _run_density(g, aggr, dtype):
    n, ei, ew, x, pos, y, z = density_inputs(g)
    model = O.OracleGLASS(int(g["hidden"]), int(g["layers"]), int(g["max_deg"]), 3, aggr=aggr, pool=str(g["pool"]),
                          z_ratio=float(g["z_ratio"]))
    model.load_state_dict(sd_from(g))
    model = model.to(dtype)
    emb = model.node_emb(x, ei, ew.to(dtype), z)
    pred = model.preds[0](model.pool_emb(emb, pos))
    loss = nn.CrossEntropyLoss()(pred, y)
    loss.backward()
    return emb.detach(), pred.detach(), loss.item(), {k: p.grad for k, p in model.named_parameters()}


@pytest.mark.parametrize("aggr", ["sum", "mean", "gcn"])
def test_g5_density_full_model(aggr):
    """Full GLASS fwd + loss + every parameter gradient on the shipped density graph.

    The reference evaluated in fp32 deviates from ITSELF evaluated in fp64 by 1e-5..3e-5 rel-inf on this
    input (PyG's scatter_mean sums the 4998 rows sequentially in fp32), so three statements are checked:
      (1) oracle.double() == reference.double() to 1e-10   -> the restated MATH is the reference's;
      (2) oracle fp32 is within 1e-5 of the reference's fp64 result;
      (3) oracle fp32 vs reference fp32 differ by no more than 1e-5 + the reference's own fp32 noise.
    """
    g = load(f"g5_density_{aggr}.npz")
    n, ei, ew, x, pos, y, z = density_inputs(g)
    assert np.array_equal(O.max_zero_one(x, pos).numpy(), g["z"].astype(np.int64))
    keys = [str(k) for k in g["gnorm64_keys"]]
    ref32, ref64 = grads_from(g), grads_from(g, "grad64/")
    assert sorted(ref32) == keys

    # (1) math pin in float64
    emb64, pred64, loss64, grads64 = _run_density(g, aggr, torch.float64)
    assert sorted(grads64) == keys
    assert rel_inf(pred64, g["pred64"]) < 1e-10
    assert abs(loss64 - float(g["loss64"])) < 1e-10 * abs(float(g["loss64"]))
    assert rel_inf(emb64[:16], g["emb_rows64"]) < 1e-10
    assert rel_inf(emb64.sum(0), g["emb_colsum64"]) < 1e-9
    gn = np.array([grads64[k].norm().item() for k in keys])
    assert np.allclose(gn, g["gnorm64"], rtol=1e-9, atol=1e-12 * g["gnorm64"].max())
    assert rel_inf(flat_grads(grads64, keys), flat_grads(ref64, keys)) < 2e-7  # stored rounded to f32

    # (2) fp32 oracle vs reference-fp64
    emb, pred, loss, grads = _run_density(g, aggr, torch.float32)
    assert rel_inf(pred, g["pred64"]) < TOL
    assert abs(loss - float(g["loss64"])) < TOL * abs(float(g["loss64"]))
    assert rel_inf(emb[:16], g["emb_rows64"]) < TOL
    assert rel_inf(flat_grads(grads, keys), flat_grads(ref64, keys)) < TOL

    # (3) fp32 oracle vs reference-fp32, allowing the reference's own measured fp32 noise
    noise_pred = rel_inf(g["pred"], g["pred64"])
    noise_grad = rel_inf(flat_grads(ref32, keys), flat_grads(ref64, keys))
    assert rel_inf(pred, g["pred"]) < TOL + noise_pred
    assert rel_inf(flat_grads(grads, keys), flat_grads(ref32, keys)) < TOL + noise_grad


def test_g8_adam_three_steps():
    g = load("g8_adam.npz")
    x = torch.from_numpy(g["x"])
    ei, ew = torch.from_numpy(g["edge_index"]), torch.from_numpy(g["edge_weight"])
    pos_all, y_all = torch.from_numpy(g["pos"]), torch.from_numpy(g["y"])
    model = O.OracleGLASS(int(g["hidden"]), int(g["layers"]), int(x.max()), 3, aggr=str(g["aggr"]),
                          pool=str(g["pool"]), z_ratio=float(g["z_ratio"]))
    model.load_state_dict(sd_from(g))
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=float(g["lr"]))
    losses = []
    for step in range(3):
        sel = torch.arange(step * 4, step * 4 + 4)
        losses.append(O.train_step(model, opt, nn.CrossEntropyLoss(), x, ei, ew, pos_all[sel], y_all[sel]))
    assert np.allclose(losses, g["losses"], rtol=1e-5, atol=0)
    end = sd_from(g, "sd_end/")
    mine = model.state_dict()
    keys = sorted(end)
    assert rel_inf(flat_grads(mine, keys), flat_grads(end, keys)) < 1e-4  # 3 Adam steps amplify sign(g) noise


def test_g9_state_dict_keys():
    g = load("g9_keys.npz")
    model = O.OracleGLASS(64, 2, 1, 3)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [str(list(v.shape)) for v in sd.values()] == [str(s) for s in g["shapes"]]
    assert sum(p.numel() for p in model.parameters()) == int(g["n_params"]) == 51331


def test_oracle_fp64_mode():
    """The oracle runs in float64 (ground truth for noise-floor comparisons)."""
    g = load("g2_conv_mean.npz")
    conv = O.OracleConv(8, 8, "mean", 0.8, 0.0).double()
    conv.load_state_dict({k: v.double() for k, v in sd_from(g).items()})
    y = conv(torch.from_numpy(g["x"]).double(), torch.from_numpy(g["edge_index"]),
             torch.from_numpy(g["edge_weight"]), torch.from_numpy(g["mask"]).reshape(-1, 1), torch.nn.functional.elu)
    assert y.dtype == torch.float64 and rel_inf(y.detach(), g["y"]) < TOL


@pytest.mark.parametrize("name", ["L2_jk0_mean", "L3_jk1_gcn", "L1_jk0_sum"])
def test_g10_edgegnn_ssl_path(name):
    """SSL pre-training path (EdgeGNN / EmbGConv / MyGCNConv): oracle vs the reference in fp64 (math pin) and fp32."""
    g = load(f"g10_edgegnn_{name}.npz")
    x, ei, ew = torch.from_numpy(g["x"]), torch.from_numpy(g["edge_index"]), torch.from_numpy(g["edge_weight"])
    pairs, y = torch.from_numpy(g["pairs"]), torch.from_numpy(g["y"])
    for dt, tag, tol in ((torch.float64, "64", 1e-11), (torch.float32, "", TOL)):
        m = O.OracleEdgeGNN(int(g["hidden"]), int(g["layers"]), int(x.max()), aggr=str(g["aggr"]), jk=bool(g["jk"]))
        m.load_state_dict(sd_from(g))
        m = m.to(dt).train()
        pred = m(x, ei, ew.to(dt), pairs)
        loss = nn.BCEWithLogitsLoss()(pred.flatten(), y.to(dt))
        loss.backward()
        ref = grads_from(g, "grad" + tag + "/")
        keys = sorted(ref)
        mine = {k: p.grad for k, p in m.named_parameters()}
        assert sorted(mine) == keys
        assert rel_inf(pred.detach(), g["pred" + tag]) < tol
        assert abs(loss.item() - float(g["loss" + tag])) < tol * abs(float(g["loss" + tag]))
        assert rel_inf(flat_grads(mine, keys), flat_grads(ref, keys)) < tol


@pytest.mark.parametrize("name,p", [("L2_jk0_mean", 0.5), ("L3_jk1_gcn", 0.3), ("L1_jk0_sum", 0.5)])
def test_edgegnn_fed_dropout_masks_reproduce_the_unfed_run(name, p, monkeypatch):
    """The pre-training oracle takes fed keep-scales (O.mask_feed) at all of its dropouts — the embedding, behind each
    non-last layer's ReLU, the head, in that order: feeding the scales F.dropout itself draws under a seed reproduces the
    unfed fp64 forward and gradients bit for bit, and the feed is used up.  The scales are recorded by a hook around
    O._dropout that replays the draw of each call on a tensor of ones."""
    g = load(f"g10_edgegnn_{name}.npz")
    x, ei, ew = torch.from_numpy(g["x"]), torch.from_numpy(g["edge_index"]), torch.from_numpy(g["edge_weight"])
    pairs, y = torch.from_numpy(g["pairs"]), torch.from_numpy(g["y"])
    layers = int(g["layers"])
    torch.manual_seed(11)
    m = O.OracleEdgeGNN(int(g["hidden"]), layers, int(x.max()), aggr=str(g["aggr"]), dropout=p, jk=bool(g["jk"])).double().train()
    keys = sorted(k for k, _ in m.named_parameters())
    assert "preds.0.seq.modlist.0.weight" in keys and "preds.0.seq.modlist.3.weight" in keys  # the reference's keys at p > 0

    def run():
        m.zero_grad()
        pred = m(x, ei, ew.double(), pairs)
        loss = nn.BCEWithLogitsLoss()(pred.flatten(), y.double())
        loss.backward()
        return pred.detach().clone(), loss.item(), flat_grads({k: q.grad for k, q in m.named_parameters()}, keys).clone()

    recorded, plain = [], O._dropout

    def recording(h, pp, training):
        state = torch.get_rng_state()
        out = plain(h, pp, training)
        after = torch.get_rng_state()
        torch.set_rng_state(state)
        recorded.append(torch.nn.functional.dropout(torch.ones_like(h), p=pp, training=training))
        assert torch.equal(torch.get_rng_state(), after)  # the replay consumed what the call consumed
        return out

    O.mask_feed([])
    monkeypatch.setattr(O, "_dropout", recording)
    torch.manual_seed(5)
    pred0, loss0, grad0 = run()
    monkeypatch.setattr(O, "_dropout", plain)
    torch.manual_seed(5)
    pred1, loss1, grad1 = run()  # unfed, unhooked: the hook changed nothing
    assert torch.equal(pred0, pred1) and loss0 == loss1 and torch.equal(grad0, grad1)
    assert len(recorded) == 1 + (layers - 1) + 1
    assert [tuple(r.shape) for r in recorded] == [(x.shape[0], int(g["hidden"]))] * layers + [(pairs.shape[0], int(g["hidden"]))]
    for r in recorded:
        assert set(r.unique().tolist()) == {0.0, 1.0 / (1.0 - p)}
    torch.manual_seed(77)  # another seed: a fed run draws nothing
    O.mask_feed(recorded)
    try:
        pred2, loss2, grad2 = run()
        assert not O._MASK_FEED  # fully consumed, in call order
    finally:
        O.mask_feed([])
    assert torch.equal(pred2, pred0) and loss2 == loss0 and torch.equal(grad2, grad0)
    assert float(grad0.abs().max()) > 0 and not torch.equal(run()[0], pred0)  # (unfed again under seed 77's stream: other masks)


G11 = ["relu_gn_max_mean", "relu_nogn_sum_gcn", "relu_gn_size_sum"]


@pytest.mark.parametrize("name", G11)
def test_g11_reference_constructor_defaults(name):
    """The reference's constructor defaults outside the fused kernels' coverage — nn.ReLU() (impl/models.py:125,192),
    gn=False (:194), MaxPool (:300-303), hidden 48 — oracle vs the reference run in fp64 (math pin) and fp32."""
    g = load(f"g11_defaults_{name}.npz")
    x, ei, ew = torch.from_numpy(g["x"]), torch.from_numpy(g["edge_index"]), torch.from_numpy(g["edge_weight"])
    pos, y = torch.from_numpy(g["pos"]), torch.from_numpy(g["y"])
    assert np.array_equal(O.max_zero_one(x, pos).numpy(), g["z"])
    ref = grads_from(g, "grad64/")
    keys = sorted(ref)
    assert ("conv.gns.0.weight" in keys) == bool(g["gn"])
    for dt, tol in ((torch.float64, 1e-11), (torch.float32, TOL)):
        m = O.OracleGLASS(int(g["hidden"]), int(g["layers"]), int(x.max()), 3, aggr=str(g["aggr"]), pool=str(g["pool"]),
                          z_ratio=float(g["z_ratio"]), gn=bool(g["gn"]), act="relu")
        m.load_state_dict(sd_from(g))
        m = m.to(dt).train()
        pred = m(x, ei, ew.to(dt), pos, O.max_zero_one(x, pos))
        loss = nn.CrossEntropyLoss()(pred, y)
        loss.backward()
        mine = {k: p.grad for k, p in m.named_parameters()}
        assert sorted(mine) == keys
        assert rel_inf(pred.detach(), g["pred64"]) < tol
        assert abs(loss.item() - float(g["loss64"])) < tol * abs(float(g["loss64"]))
        assert rel_inf(flat_grads(mine, keys), flat_grads(ref, keys)) < tol
        if dt == torch.float32:
            assert rel_inf(pred.detach(), g["pred"]) < TOL + rel_inf(g["pred"], g["pred64"])
