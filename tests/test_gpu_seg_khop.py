"""GNN-seg at hop > 0 on the MI355X: the k-hop ball kernels (glass_seg_khop_count / _fill) and everything downstream of
them — extraction, collate, the models, the driver — against the CPU restatement of k_hop_subgraph in
tests/seg_khop_oracle.py and the fp64 oracle of tests/seg_oracle.py."""
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
import seg_khop_oracle as K  # noqa: E402
import seg_oracle as O  # noqa: E402
from helpers import flat_grads, rel_inf  # noqa: E402
from test_gpu_seg import _build, _graph, _sparse, _split_csr, _vals_close  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the largest base graph whose bitmaps take the LDS form, and one node more (tests/test_seg_khop_host.py checks them
# against GLASS_SEG_KHOP_LDS_NODES)
LDS_EDGE_N = (131072, 131073)


def _dataset(x, ei, w, pos, y, mode, hop, base=None):
    from glass_amd import seg
    return seg.GsDataset(x.to(DEV), ei.to(DEV), w.to(DEV), pos.to(DEV), y.to(DEV), mode=mode, base=base, hop=hop)


def _isolated(seed=0):
    """A random directed graph (duplicates, weight-2 edges) plus node n with no edge at all, as a centre alone and beside
    another centre."""
    x, ei, w, pos, y = _graph("random0", seed)
    n = x.shape[0]
    pos = pos[:12].clone()
    pos[3] = -1
    pos[3, 0] = n
    pos[4, :2] = torch.tensor([n, 5])
    return torch.ones(n + 1, 1, 1), ei, w, pos, y[:12]


def _sparse_random(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, 3 * n), generator=g)
    ei[:, :4] = torch.tensor([[n - 1, n - 2, 0, n - 1], [3, n - 1, n - 1, 0]])  # the last node, last word's high bits
    w = torch.ones(ei.shape[1])
    w[torch.randint(0, ei.shape[1], (100, ), generator=g)] = 2.0
    pos = torch.randint(0, n, (48, 4), generator=g)
    pos[0] = torch.tensor([n - 1, -1, -1, -1])
    pos[1] = torch.tensor([0, 31, 32, n - 1])
    return torch.ones(n, 1, 1), ei, w, pos, torch.zeros(48, dtype=torch.int64)


def _check_split(x, ei, w, pos, y, mode, hop):
    n = x.shape[0]
    blocks = K.split_blocks(ei, w.double(), pos, mode, hop, n)
    ds = _dataset(x, ei, w, pos, y, mode, hop)
    ds2 = _dataset(x, ei, w, pos, y, mode, hop)
    sizes = torch.tensor([b[0].shape[0] for b in blocks])
    assert torch.equal(ds.sub_nodes.cpu().long(), torch.cat([b[0] for b in blocks]))
    assert torch.equal(ds.sub_ptr.cpu().long(), torch.cat((torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0))))
    assert ds.sizes_h.tolist() == sizes.tolist() and ds.n_member == int(sizes.sum())
    for o, (rp, col, val) in enumerate(((ds.rowptr_in, ds.col_in, ds.val_in), (ds.rowptr_out, ds.col_out, ds.val_out))):
        orp, ocol, oval = _split_csr(blocks, o)
        assert torch.equal(rp.cpu().long(), orp) and torch.equal(col.cpu().long(), ocol)
        assert _vals_close(val, oval)
    for a, b in ((ds.sub_nodes, ds2.sub_nodes), (ds.sub_ptr, ds2.sub_ptr), (ds.col_in, ds2.col_in),
                 (ds.val_in, ds2.val_in), (ds.col_out, ds2.col_out), (ds.val_out, ds2.val_out)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))  # bitwise repeatable
    ids = np.random.default_rng(1).permutation(len(ds))[:max(2, len(ds) - 3)]
    bt, bt2 = ds.collate(ids), ds2.collate(ids)
    node_map, (rp, col, val), (rpt, colt, valt), opos = O.collate(blocks, list(ids))
    assert torch.equal(bt.node_map.cpu().long(), node_map) and torch.equal(bt.pos.cpu(), opos)
    assert torch.equal(bt.adj.fwd.rowptr.cpu().long(), rp) and torch.equal(bt.adj.fwd.col.cpu().long(), col)
    assert torch.equal(bt.adj.bwd.rowptr.cpu().long(), rpt) and torch.equal(bt.adj.bwd.col.cpu().long(), colt)
    assert _vals_close(bt.adj.fwd.val, val) and _vals_close(bt.adj.bwd.val, valt)
    assert torch.equal(bt.adj.fwd.val.view(torch.int32), bt2.adj.fwd.val.view(torch.int32))
    assert torch.equal(bt.x.cpu(), x[node_map]) and torch.equal(bt.y.cpu(), y[torch.as_tensor(ids)])
    return ds


CASES = [("density", "gin", 1), ("density", "gcn", 1), ("density", "gin", 2), ("density", "gcn", 2),
         ("cut_ratio", "gcn", 2), ("component", "gcn", 2), ("synthetic:ppi_bp", "gcn", 1),
         ("random0", "gcn", 1), ("random1", "gin", 2), ("random2", "gcn", 3)]


@pytest.mark.parametrize("name,mode,hop", CASES)
def test_balls_extraction_and_collate_match_the_oracle(name, mode, hop):
    x, ei, w, pos, y = _graph(name, seed=int(name[-1]) if name.startswith("random") else 0)
    ds = _check_split(x, ei, w, pos, y, mode, hop)
    assert ds.n_member > int((pos >= 0).sum()) // 2  # (the balls did grow)
    if name.startswith("random"):  # a directed graph: the in-ball the kernels follow is not the out-ball
        rev = ei.flip(0)
        assert any(not torch.equal(K.k_hop_nodes(r[r >= 0], hop, ei, x.shape[0]),
                                   K.k_hop_nodes(r[r >= 0], hop, rev, x.shape[0])) for r in pos[3:13])


@pytest.mark.parametrize("mode,hop", [("gcn", 1), ("gin", 3)])
def test_isolated_centre(mode, hop):
    x, ei, w, pos, y = _isolated()
    ds = _check_split(x, ei, w, pos, y, mode, hop)
    n = x.shape[0] - 1
    lo, hi = int(ds.sub_ptr_h[3]), int(ds.sub_ptr_h[4])
    assert ds.sub_nodes[lo:hi].tolist() == [n]


@pytest.mark.parametrize("n", LDS_EDGE_N)
def test_both_sides_of_the_lds_threshold(n):
    from glass_amd import _lib
    ws = _lib.load().glass_seg_khop_ws_bytes(n, 48)
    assert (ws == 0) == (n == LDS_EDGE_N[0]) and ws >= 0
    x, ei, w, pos, y = _sparse_random(n)
    _check_split(x, ei, w, pos, y, "gcn", 2)
    _check_split(x, ei, w, pos, y, "gin", 3)


def test_refusal_past_the_int32_limit():
    """Star graph: hub 0 and 2^20 leaves, both directions.  2 049 leaf-centred subgraphs at hop 2 are each the whole
    graph: 2 049 * (2^20 + 1) > 2^31 ball nodes.  The split is refused after the count pass, before the fill's output is
    allocated: the peak memory of the call stays within the count's workspace."""
    from glass_amd import _lib, seg
    leaves = 2**20
    n = leaves + 1
    leaf = torch.arange(1, n, device=DEV)
    ei = torch.cat((torch.stack((torch.zeros_like(leaf), leaf)), torch.stack((leaf, torch.zeros_like(leaf)))), 1)
    w = torch.ones(ei.shape[1], device=DEV)
    base = seg.SegBase(ei, w, n)
    n_sub = 2049
    pos = torch.arange(1, n_sub + 1, device=DEV).reshape(-1, 1)
    x = torch.ones(n, 1, 1, device=DEV)
    y = torch.zeros(n_sub, dtype=torch.int64, device=DEV)
    ws = _lib.load().glass_seg_khop_ws_bytes(n, n_sub)
    assert ws > 0
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with pytest.raises(_lib.GlassHipError, match=r"2\^31"):
        seg.GsDataset(x, ei, w, pos, y, mode="gcn", base=base, hop=2)
    peak = torch.cuda.max_memory_allocated() - before
    print(f"star: workspace {ws} B, peak during the refused split {peak} B")
    assert peak <= ws + (4 << 20)
    # hop 1 (leaf + hub) is taken, and its balls are right
    ds = seg.GsDataset(x, ei, w, pos, y, mode="gcn", base=base, hop=1)
    assert ds.sizes_h.tolist() == [2] * n_sub
    assert torch.equal(ds.sub_nodes.cpu().long().reshape(-1, 2)[:, 1], torch.arange(1, n_sub + 1))


@pytest.mark.parametrize("name,mode", [("density", "gcn"), ("random0", "gin"), ("synthetic:ppi_bp", "gcn")])
def test_hop_zero_is_unchanged(name, mode, monkeypatch):
    from glass_amd import _lib, seg
    x, ei, w, pos, y = _graph(name)
    ref = _dataset(x, ei, w, pos, y, mode, 0)
    a = seg.GsDataset(x.to(DEV), ei.to(DEV), w.to(DEV), pos.to(DEV), y.to(DEV), mode=mode)
    lib = _lib.load()

    class NoKhop:  # hop 0 launches none of the k-hop entries
        def __getattr__(self, name):
            assert "khop" not in name, name
            return getattr(lib, name)

    monkeypatch.setattr(_lib, "load", lambda: NoKhop())
    b = _dataset(x, ei, w, pos, y, mode, 0)
    for ds in (ref, b):
        for k in ("sub_nodes", "sub_ptr", "rowptr_in", "rowptr_out", "col_in", "val_in", "col_out", "val_out", "deg"):
            u, v = getattr(a, k), getattr(ds, k)
            assert (u is None and v is None) or (u.dtype == v.dtype and torch.equal(u.view(torch.int32),
                                                                                     v.view(torch.int32))), k
        for k in ("sizes_h", "sub_ptr_h", "cnt_in_h", "cnt_out_h"):
            assert np.array_equal(getattr(a, k), getattr(ds, k)), k
        assert ds.n_member == a.n_member and ds.n_sub == a.n_sub


MODEL_CASES = [("density", "gin", 1, 16, 1), ("density", "gcn", 2, 16, 2), ("component", "gcn", 2, 64, 2)]


@pytest.mark.parametrize("name,mode,L,H,hop", MODEL_CASES)
def test_gnn_forward_loss_and_gradients_match_fp64(name, mode, L, H, hop):
    from glass_amd import seg
    x, ei, w, pos, y = _graph(name)
    n_out = int(y.max()) + 1
    ds = _dataset(x, ei, w, pos, y, mode, hop)
    bx, adj, ew, bpos, by = next(iter(seg.GsDataloader(ds, len(ds), shuffle=False, drop_last=False)))
    model = _build(mode, x.shape[-1], H, L, n_out)
    model.train()
    pred = model(bx, adj, ew, bpos)
    loss = torch.nn.CrossEntropyLoss()(pred, by)
    loss.backward()
    p = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    n = bx.shape[0]
    blocks = K.split_blocks(ei, w.double(), pos, mode, hop, x.shape[0])
    _, (rp, col, val), _, opos = O.collate(blocks, list(range(len(ds))))
    assert torch.equal(bpos.cpu(), opos)  # the pool covers every node of each ball
    A = _sparse((rp, col, val), n)
    mlp_keys = sorted({k.rsplit(".", 1)[0] + "." for k in p if k.startswith("mods.1.")})
    po = O.gnn(p, bx.cpu(), A, bpos.cpu(), mode, L, mlp_keys)
    lo = torch.nn.CrossEntropyLoss()(po, by.cpu())
    lo.backward()
    e_pred = rel_inf(pred.detach().cpu(), po.detach())
    keys = sorted(p)
    e_grad = rel_inf(flat_grads({k: v.grad.cpu() for k, v in model.named_parameters()}, keys),
                     flat_grads({k: v.grad for k, v in p.items()}, keys))
    print(f"{name} {mode} hop {hop} L {L} H {H}: {n} nodes, pred rel-inf {e_pred:.2e}, grad rel-inf {e_grad:.2e}")
    assert e_pred < 1e-5
    assert abs(loss.item() - lo.item()) <= 1e-5 * abs(lo.item())
    assert e_grad < 1e-5


def test_driver_runs_density_at_hop_one():
    r = subprocess.run([sys.executable, "GNNSeg.py", "--dataset", "density", "--hop", "1", "--repeat", "1", "--epochs",
                        "10"], cwd=ROOT, capture_output=True, text=True, timeout=900, env=dict(os.environ))
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout
    assert "hop=1" in out and "repeat 0" in out and "seed  0" in out and "iter 0 loss " in out and " val " in out
    end = [ln for ln in out.splitlines() if ln.startswith("end: val ")]
    assert len(end) == 1
    tst = float(end[0].split()[-1])
    assert np.isfinite(tst) and 0.0 <= tst <= 1.0
    assert "tst scores [" in out and "best params {'conv_layer': 1, 'dropout': 0.4, 'hidden_dim': 16}" in out
