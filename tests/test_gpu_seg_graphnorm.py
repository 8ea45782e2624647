"""GNN-seg with the per-graph GraphNorm (seg.GConv(graph_norm="graph")) on the MI355X: values against an fp64 restatement,
independence of a subgraph's logits from the batch around it, and the untouched default."""
import functools
import os
import sys

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import graphnorm_seg_oracle as GO  # noqa: E402
import seg_oracle as O  # noqa: E402
from helpers import flat_grads, grad_table, rel_inf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, L, N_OUT = 16, 3, 3


@functools.lru_cache(maxsize=None)
def _graph():
    """A random DIRECTED 60-node graph with duplicate and weight-2 edges and 12 subgraphs of 1 .. 9 distinct nodes."""
    g = torch.Generator().manual_seed(21)
    n, e = 60, 400
    ei = torch.randint(0, n, (2, e), generator=g)
    ei = torch.cat((ei, ei[:, :20]), 1)
    w = torch.ones(ei.shape[1])
    w[torch.randint(0, ei.shape[1], (30, ), generator=g)] = 2.0
    sizes = [1, 9, 2, 5, 7, 3, 1, 8, 4, 6, 2, 9]
    pos = torch.full((len(sizes), 9), -1, dtype=torch.int64)
    for b, s in enumerate(sizes):
        pos[b, :s] = torch.randperm(n, generator=g)[:s]
    x = torch.randn(n, 1, 4, generator=g)
    y = torch.randint(0, N_OUT, (len(sizes), ), generator=g)
    return x, ei, w, pos, y


def _model(mode, graph_norm=None, seed=3):
    from glass_amd import models, seg
    torch.manual_seed(seed)
    kw = {} if graph_norm is None else {"graph_norm": graph_norm}
    conv = seg.GConv(4, H, H, L, conv=seg.MyGINConv if mode == "gin" else seg.GCNConv, activation=nn.ELU(inplace=True),
                     dropout=0.0, **kw)
    mlp = models.MLP(H * L, H, N_OUT, 2, dropout=0.0, activation=nn.ELU(inplace=True))
    model = seg.GNN(conv, mlp)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():  # non-trivial GraphNorm parameters (the initial 1, 0, 1 hide mean_scale)
        for gn in conv.gns:
            gn.weight.copy_(1 + 0.3 * torch.randn(H, generator=gen))
            gn.bias.copy_(0.2 * torch.randn(H, generator=gen))
            a = 1 + 0.3 * torch.randn(H, generator=gen)
            a[(a - 1).abs() < 0.05] = 1.25
            gn.mean_scale.copy_(a)
    return model.to(DEV)


def _dataset(mode):
    from glass_amd import seg
    x, ei, w, pos, y = _graph()
    return seg.GsDataset(x.to(DEV), ei.to(DEV), w.to(DEV), pos.to(DEV), y.to(DEV), mode=mode)


def _oracle_logits(p, x, A, seg_ptr, pos, mode):
    """seg_oracle.gnn with the per-graph norm in place of the whole-batch one (one feature channel)."""
    h, xs = x[:, 0, :].double(), []
    for l in range(L):
        c = f"mods.0.convs.{l}."
        if mode == "gcn":
            h = A @ (h @ p[c + "weight"]) + p[c + "bias"]
        else:
            h = (A @ h) @ p[c + "conv.nn.weight"].t() + p[c + "conv.nn.bias"]
        if l < L - 1:
            g = f"mods.0.gns.{l}."
            h = GO.graphnorm_seg(h, seg_ptr, p[g + "weight"], p[g + "bias"], p[g + "mean_scale"], act=1)
        xs.append(h)
    emb = torch.cat(xs, -1)
    sel = torch.zeros(pos.shape[0], emb.shape[0], dtype=torch.float64)
    for b in range(pos.shape[0]):
        sel[b, pos[b][pos[b] >= 0]] = 1
    keys = sorted({k.rsplit(".", 1)[0] + "." for k in p if k.startswith("mods.1.")})
    (w0, b0), (w1, b1) = [(p[k + "weight"], p[k + "bias"]) for k in keys]
    return F.elu((sel @ emb) @ w0.t() + b0) @ w1.t() + b1


@pytest.mark.parametrize("mode", ["gin", "gcn"])
def test_loss_and_gradients_match_fp64(mode):
    x, ei, w, pos, y = _graph()
    ds = _dataset(mode)
    bt = ds.collate(list(range(len(ds))))
    bx, adj, ew, bpos, by = bt.as_tuple()
    assert adj.seg_ptr is not None and adj.seg_ptr.dtype == torch.int32 and adj.seg_ptr.shape[0] == len(ds) + 1
    model = _model(mode, "graph")
    model.train()
    pred = model(bx, adj, ew, bpos)
    loss = nn.CrossEntropyLoss()(pred, by)
    loss.backward()
    p = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    blocks = O.split_blocks(ei, w.double(), pos, mode)
    _, csr, _, opos = O.collate(blocks, list(range(len(ds))))
    assert torch.equal(opos, bpos.cpu())
    n = bx.shape[0]
    seg_ptr = adj.seg_ptr.cpu().long()
    assert seg_ptr.tolist() == GO.seg_ptr_of([b[0].shape[0] for b in blocks]).tolist()
    po = _oracle_logits(p, bx.cpu(), O.dense(csr, n), seg_ptr, opos, mode)
    lo = nn.CrossEntropyLoss()(po, by.cpu())
    lo.backward()
    keys = sorted(p)
    mine = {k: v.grad.cpu() for k, v in model.named_parameters()}
    ref = {k: v.grad for k, v in p.items()}
    err_p, err_g = rel_inf(pred.detach().cpu(), po.detach()), rel_inf(flat_grads(mine, keys), flat_grads(ref, keys))
    print(mode, f"logits {err_p:.2e} loss {abs(loss.item() - lo.item()) / abs(lo.item()):.2e} gradients {err_g:.2e}",
          grad_table(mine, ref, keys)[:3])
    assert err_p <= 1e-5
    assert abs(loss.item() - lo.item()) <= 1e-5 * abs(lo.item())
    # the project's gradient metric: rel-inf over all parameter gradients at once (tests/test_gpu_seg.py)
    assert err_g <= 1e-5


@pytest.mark.parametrize("mode", ["gin", "gcn"])
def test_logits_do_not_depend_on_the_batch(mode):
    """Evaluation logits of subgraph k in a batch of 12, in a batch of 3 and alone agree to rel-inf 1e-5 (not bitwise: the
    K1 plans of the batches differ).  k is a subgraph of at least 2 nodes: a 1-node graph normalises to bias exactly.
    The whole-batch mode (graph_norm="batch", the reference's) does not have this property: there the statistics, and with
    them every logit, change with the subgraphs that share the batch."""
    ds = _dataset(mode)
    model = _model(mode, "graph").eval()
    k = 4  # 7 nodes
    assert ds.sizes_h[k] >= 2

    def logits(ids):
        bx, adj, ew, bpos, _ = ds.collate(ids).as_tuple()
        with torch.no_grad():
            return model(bx, adj, ew, bpos)[ids.index(k)].cpu()

    full, three, alone = logits(list(range(12))), logits([7, k, 0]), logits([k])
    print(mode, rel_inf(three, full.double()), rel_inf(alone, full.double()))
    assert rel_inf(three, full.double()) <= 1e-5 and rel_inf(alone, full.double()) <= 1e-5


@pytest.mark.parametrize("mode", ["gin", "gcn"])
def test_default_is_the_whole_batch_norm_untouched(mode):
    ds = _dataset(mode)
    bx, adj, ew, bpos, by = ds.collate(list(range(len(ds)))).as_tuple()
    outs = []
    for graph_norm in (None, "batch"):
        model = _model(mode, graph_norm)
        model.train()
        pred = model(bx, adj, ew, bpos)
        nn.CrossEntropyLoss()(pred, by).backward()
        outs.append(torch.cat([pred.detach().reshape(-1)] + [q.grad.reshape(-1) for q in model.parameters()]).cpu())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    # and it is the whole-batch statistics: the fp64 oracle of the reference's form
    x, ei, w, pos, y = _graph()
    model = _model(mode, "batch").eval()
    p = {k: v.detach().cpu().double() for k, v in model.named_parameters()}
    _, csr, _, opos = O.collate(O.split_blocks(ei, w.double(), pos, mode), list(range(len(ds))))
    keys = sorted({k.rsplit(".", 1)[0] + "." for k in p if k.startswith("mods.1.")})
    with torch.no_grad():
        ref = O.gnn(p, bx.cpu(), O.dense(csr, bx.shape[0]), opos, mode, L, keys)
        assert rel_inf(model(bx, adj, ew, bpos).cpu(), ref) <= 1e-5
