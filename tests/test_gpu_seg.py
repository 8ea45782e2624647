"""GNN-seg on the MI355X: the K10 extraction and collate kernels and the GNN-seg models (glass_amd/seg.py) against the
fp64 oracle of tests/seg_oracle.py, and one short run of the GNNSeg.py driver."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import seg_oracle as O  # noqa: E402
from helpers import flat_grads, rel_inf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _graph(name, seed=0):
    """(x [N,1,F] float, edge_index, edge_weight, pos, y) on the CPU: a dataset split, or a random DIRECTED graph with
    duplicate edges and weight-2 edges."""
    if name.startswith("random"):
        g = torch.Generator().manual_seed(seed)
        n, e = 5000, 40000
        ei = torch.randint(0, n, (2, e), generator=g)
        ei = torch.cat((ei, ei[:, :200]), 1)  # duplicates
        w = torch.ones(ei.shape[1])
        w[torch.randint(0, ei.shape[1], (300, ), generator=g)] = 2.0
        w[:5] = 0.25
        pos = torch.randint(0, n, (40, 24), generator=g)
        pos[torch.rand(pos.shape, generator=g) < 0.3] = -1
        pos[0, :] = -1
        pos[0, :3] = torch.tensor([7, 7, 3])  # duplicate id
        pos[1, :] = -1
        pos[1, 0] = 11
        big = torch.randperm(n, generator=g)[:4500]
        pos = torch.nn.functional.pad(pos, (0, n - pos.shape[1]), value=-1)
        pos[2] = -1
        pos[2, :big.shape[0]] = big  # a list longer than the LDS stage: the searches read global memory
        return torch.ones(n, 1, 1), ei, w, pos, torch.zeros(pos.shape[0], dtype=torch.int64)
    import datasets
    torch.manual_seed(seed)
    g = datasets.load_dataset(name)
    if name in ("synthetic:ppi_bp", "synthetic:em_user", "synthetic:hpo_neuro"):
        g.addDegreeFeature()  # the driver's feature rule
    else:
        g.addOneFeature()
    _, ei, w, pos, y = g.get_split("test")
    return g.x, ei, w, pos, y if y.dtype.is_floating_point else y.long()


def _oracle_blocks(ei, w, pos, mode):
    members = torch.unique(pos[pos >= 0])
    inside = torch.zeros(int(max(ei.max(), members.max())) + 1, dtype=torch.bool)
    inside[members] = True
    keep = inside[ei[0]] & inside[ei[1]]  # (only edges inside the union matter: same order, fewer to scan)
    return O.split_blocks(ei[:, keep], w[keep], pos, mode)


def _split_csr(blocks, o):
    lens = torch.cat([b[1 + o][0][1:] - b[1 + o][0][:-1] for b in blocks])
    rp = torch.zeros(lens.shape[0] + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(lens, 0)
    return rp, torch.cat([b[1 + o][1] for b in blocks]), torch.cat([b[1 + o][2] for b in blocks])


def _vals_close(a, b):
    a, b = a.double().cpu(), b.double()
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    return bool(((a - b).abs() <= 1e-6 * b.abs() + 1e-30).all())


CASES = [("density", "gin"), ("density", "gcn"), ("synthetic:ppi_bp", "gcn"), ("synthetic:em_user", "gcn"),
         ("synthetic:hpo_neuro", "gcn"), ("random0", "gcn"), ("random1", "gin")]


@pytest.mark.parametrize("name,mode", CASES)
def test_extraction_and_collate_match_the_oracle(name, mode):
    from glass_amd import seg
    x, ei, w, pos, y = _graph(name, seed=int(name[-1]) if name.startswith("random") else 0)
    blocks = _oracle_blocks(ei, w.double(), pos, mode)
    ds = seg.GsDataset(x.to(DEV), ei.to(DEV), w.to(DEV), pos.to(DEV), y.to(DEV), mode=mode)
    ds2 = seg.GsDataset(x.to(DEV), ei.to(DEV), w.to(DEV), pos.to(DEV), y.to(DEV), mode=mode)
    assert torch.equal(ds.sub_nodes.cpu().long(), torch.cat([b[0] for b in blocks]))
    for o, (rp, col, val) in enumerate(((ds.rowptr_in, ds.col_in, ds.val_in), (ds.rowptr_out, ds.col_out, ds.val_out))):
        orp, ocol, oval = _split_csr(blocks, o)
        assert torch.equal(rp.cpu().long(), orp) and torch.equal(col.cpu().long(), ocol)
        assert _vals_close(val, oval)
    for a, b in ((ds.col_in, ds2.col_in), (ds.val_in, ds2.val_in), (ds.col_out, ds2.col_out), (ds.val_out, ds2.val_out)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))  # bitwise repeatable
    # a batch of permuted subgraphs = the concatenation of their blocks
    ids = np.random.default_rng(1).permutation(len(ds))[:max(2, len(ds) - 3)]
    bt, bt2 = ds.collate(ids), ds2.collate(ids)
    node_map, (rp, col, val), (rpt, colt, valt), opos = O.collate(blocks, list(ids))
    assert torch.equal(bt.node_map.cpu().long(), node_map) and torch.equal(bt.pos.cpu(), opos)
    assert torch.equal(bt.adj.fwd.rowptr.cpu().long(), rp) and torch.equal(bt.adj.fwd.col.cpu().long(), col)
    assert torch.equal(bt.adj.bwd.rowptr.cpu().long(), rpt) and torch.equal(bt.adj.bwd.col.cpu().long(), colt)
    assert _vals_close(bt.adj.fwd.val, val) and _vals_close(bt.adj.bwd.val, valt)
    assert torch.equal(bt.adj.fwd.val.view(torch.int32), bt2.adj.fwd.val.view(torch.int32))
    assert torch.equal(bt.x.cpu(), x[node_map]) and torch.equal(bt.y.cpu(), y[torch.as_tensor(ids)])


def _sparse(csr, n):
    rp, col, val = csr
    rows = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    return torch.sparse_coo_tensor(torch.stack((rows, col)), val.double(), (n, n)).coalesce()


def _build(mode, F_in, H, L, n_out, dropout=0.0):
    import torch.nn as nn
    from glass_amd import models, seg
    torch.manual_seed(3)
    conv = seg.GConv(F_in, H, H, L, conv=seg.MyGINConv if mode == "gin" else seg.GCNConv,
                     activation=nn.ELU(inplace=True), dropout=dropout)
    mlp = models.MLP(H * L, H, n_out, 2, dropout=dropout, activation=nn.ELU(inplace=True))
    return seg.GNN(conv, mlp).to(DEV)


MODEL_CASES = [("density", "gin", 1, 16, 1), ("density", "gcn", 8, 4, 2), ("density", "gcn", 1, 64, 1),
               ("synthetic:ppi_bp", "gcn", 8, 64, 1), ("synthetic:ppi_bp", "gcn", 1, 16, 2),
               ("synthetic:ppi_bp", "gin", 8, 16, 1)]


@pytest.mark.parametrize("name,mode,L,H,C", MODEL_CASES)
def test_gnn_forward_loss_and_gradients_match_fp64(name, mode, L, H, C):
    from glass_amd import seg
    x, ei, w, pos, y = _graph(name)
    if C == 2:  # two feature channels: ones and the degree one-hot (mean over channels)
        deg = O.degree_feature(ei, w, x.shape[0])
        x = torch.cat((torch.nn.functional.pad(torch.ones(x.shape[0], 1, 1), (0, deg.shape[-1] - 1)), deg), 1)
    n_out = int(y.max()) + 1
    ds = seg.GsDataset(x.to(DEV), ei.to(DEV), w.to(DEV), pos.to(DEV), y.to(DEV), mode=mode)
    bx, adj, ew, bpos, by = next(iter(seg.GsDataloader(ds, len(ds), shuffle=False, drop_last=False)))
    model = _build(mode, x.shape[-1], H, L, n_out)
    model.train()
    pred = model(bx, adj, ew, bpos)
    loss = torch.nn.CrossEntropyLoss()(pred, by)
    loss.backward()
    p = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    n = bx.shape[0]
    blocks = _oracle_blocks(ei, w.double(), pos, mode)
    _, (rp, col, val), _, _ = O.collate(blocks, list(range(len(ds))))
    A = _sparse((rp, col, val), n)  # the fp64 operator, not the kernel's fp32 values
    mlp_keys = sorted({k.rsplit(".", 1)[0] + "." for k in p if k.startswith("mods.1.")})
    po = O.gnn(p, bx.cpu(), A, bpos.cpu(), mode, L, mlp_keys)
    lo = torch.nn.CrossEntropyLoss()(po, by.cpu())
    lo.backward()
    assert rel_inf(pred.detach().cpu(), po.detach()) < 1e-5
    assert abs(loss.item() - lo.item()) <= 1e-5 * abs(lo.item())
    # (the project's parity metric: rel-inf over ALL parameter gradients at once — per parameter, a first-layer weight
    # behind GraphNorm's scale invariance has a true gradient near zero and no relative accuracy to speak of)
    keys = sorted(p)
    assert rel_inf(flat_grads({k: v.grad.cpu() for k, v in model.named_parameters()}, keys),
                   flat_grads({k: v.grad for k, v in p.items()}, keys)) < 1e-5


def test_dropout_eval_masks_and_seeded_repeatability():
    import torch.nn as nn
    from glass_amd import seg
    x, ei, w, pos, y = _graph("density")
    ds = seg.GsDataset(x.to(DEV), ei.to(DEV), w.to(DEV), pos.to(DEV), y.to(DEV), mode="gcn")
    bx, adj, ew, bpos, by = next(iter(seg.GsDataloader(ds, len(ds), shuffle=False, drop_last=False)))
    p_drop, H, L = 0.4, 16, 3
    m_drop = _build("gcn", 1, H, L, 3, dropout=p_drop)
    m_zero = _build("gcn", 1, H, L, 3, dropout=0.0)
    with torch.no_grad():
        for a, b in zip(m_zero.parameters(), m_drop.parameters()):  # (the MLP's module indices differ: no Dropout)
            a.copy_(b)
    m_drop.eval()
    m_zero.eval()
    with torch.no_grad():
        assert torch.equal(m_drop(bx, adj, ew, bpos), m_zero(bx, adj, ew, bpos))
    # training: GConv's dropout masks are {0, 1/(1-p)} drawn from torch's generator (nothing else in GConv draws)
    conv = m_drop.mods[0].train()
    torch.manual_seed(5)
    out = conv(bx[:, 0, :], adj, ew)
    torch.manual_seed(5)
    masks = [torch.nn.functional.dropout(torch.ones(bx.shape[0], H, device=DEV), p=p_drop).cpu().double()
             for _ in range(L - 1)]
    for m in masks:
        assert set(torch.unique(m).tolist()) <= {0.0, float(torch.tensor(1.0 / (1 - p_drop)))} and (m == 0).any()
    prm = {"mods.0." + k: v.detach().cpu().double() for k, v in conv.state_dict().items()}
    blocks = _oracle_blocks(ei, w.double(), pos, "gcn")
    _, csr, _, _ = O.collate(blocks, list(range(len(ds))))
    ref = O.gconv(prm, "mods.0.", bx[:, 0, :].cpu().double(), _sparse(csr, bx.shape[0]), "gcn", L, masks=masks)
    assert rel_inf(out.detach().cpu(), ref) < 1e-5
    # two seeded training steps are identical
    outs = []
    for _ in range(2):
        torch.manual_seed(7)
        m = _build("gcn", 1, H, L, 3, dropout=p_drop)
        m.train()
        loss = torch.nn.CrossEntropyLoss()(m(bx, adj, ew, bpos), by)
        loss.backward()
        outs.append(torch.cat([loss.detach().reshape(1)] + [q.grad.reshape(-1) for q in m.parameters()]).cpu())
    assert torch.equal(outs[0], outs[1])


def test_driver_runs_density_briefly():
    env = dict(os.environ)
    r = subprocess.run([sys.executable, "GNNSeg.py", "--dataset", "density", "--repeat", "1", "--epochs", "10"],
                       cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout
    assert "repeat 0" in out and "seed  0" in out and "iter 0 loss " in out and " val " in out and " tst " in out
    end = [ln for ln in out.splitlines() if ln.startswith("end: val ")]
    assert len(end) == 1
    tst = float(end[0].split()[-1])
    assert np.isfinite(tst) and 0.0 <= tst <= 1.0
    assert "tst scores [" in out and "best params {'conv_layer': 1, 'dropout': 0.4, 'hidden_dim': 16}" in out
