"""GNN-seg centre pooling on the MI355X: glass_seg_centre_index and glass_seg_collate_centre, GsDataset(pool="centre"),
the model on centre-pooled batches and the driver's --pool flag, against the CPU restatement of the reference's centre
mark in tests/seg_centre_oracle.py and the fp64 oracle of tests/seg_oracle.py."""
import functools
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
import seg_centre_oracle as C  # noqa: E402
import seg_khop_oracle as K  # noqa: E402
import seg_oracle as O  # noqa: E402
from helpers import flat_grads, rel_inf  # noqa: E402
from test_gpu_seg import _build, _graph, _sparse  # noqa: E402
from test_gpu_seg_khop import _isolated  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the largest ball the kernels stage in LDS, and one id more (tests/test_seg_centre_host.py checks them against
# GLASS_SEG_LDS_NODES and against the balls of _hub)
LDS_EDGE_BALL = (4096, 4097)


def _dataset(x, ei, w, pos, y, mode, hop, pool, base=None):
    from glass_amd import seg
    return seg.GsDataset(x.to(DEV), ei.to(DEV), w.to(DEV), pos.to(DEV), y.to(DEV), mode=mode, base=base, hop=hop,
                         pool=pool)


def _hub(size):
    """Node 0 with size - 1 in-neighbours (1 .. size-1), a few edges among other nodes.  Row 0 (the hub, two of its
    in-neighbours, the hub listed twice) has a hop-1 ball of exactly `size` ids; every other row's ball is tiny."""
    leaves = torch.arange(1, size)
    n = size + 40
    far = torch.arange(size, n - 1)
    ei = torch.cat((torch.stack((leaves, torch.zeros_like(leaves))), torch.stack((far, far + 1)),
                    torch.tensor([[3, size + 2, 1, size], [size + 1, 5, size - 1, 2]])), 1)  # (an edge inside every ball)
    w = torch.ones(ei.shape[1])
    w[::7] = 2.0
    pos = torch.full((6, 5), -1, dtype=torch.int64)
    pos[0] = torch.tensor([size - 1, 0, 7, size - 2, 0])
    pos[1, :2] = torch.tensor([n - 1, 4])  # two chain ends: hop-1 balls of a few nodes
    pos[2, :1] = torch.tensor([5])
    pos[3, :3] = torch.tensor([size + 1, size + 3, 9])
    pos[4, :1] = torch.tensor([size - 1])
    pos[5, :2] = torch.tensor([size, 2])
    return torch.ones(n, 1, 1), ei, w, pos, torch.zeros(6, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def _case(name, hop):
    x, ei, w, pos, y = _hub(int(name[3:])) if name.startswith("hub") else _isolated() if name == "isolated" else _graph(name)
    return (x, ei, w, pos, y), C.centre_marks(ei, pos, hop, x.shape[0])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8),
                                                                     b.contiguous().view(torch.uint8))


def _batch_orders(n_sub):
    """Natural order in batches with a last partial one, and a shuffled order cut the same way."""
    bs = max(2, (n_sub * 2) // 5)
    while n_sub % bs == 0 and bs < n_sub - 1:
        bs += 1
    assert n_sub % bs != 0
    out = []
    for order in (np.arange(n_sub), np.random.default_rng(3).permutation(n_sub)):
        out += [order[i:i + bs] for i in range(0, n_sub, bs)]
    return out


def _check_centre_split(name, mode, hop):
    """centre_local, pos and mark equal the oracle exactly, in natural and in shuffled id order with a last partial
    batch; the CSR pair and the node map of a centre batch are bitwise those of the ball batch of the same ids; a second
    construction and a second collation give the same bytes."""
    (x, ei, w, pos, y), parts = _case(name, hop)
    ball = _dataset(x, ei, w, pos, y, mode, hop, "ball")
    ds = _dataset(x, ei, w, pos, y, mode, hop, "centre", base=ball.base)
    ds2 = _dataset(x, ei, w, pos, y, mode, hop, "centre")
    assert ball.centre_local is None and ds.pool == "centre" and ball.pool == "ball"
    assert torch.equal(ds.sub_nodes.cpu().long(), torch.cat([p[0] for p in parts]))
    assert torch.equal(ds.centre_local.cpu().long(), torch.cat([p[1] for p in parts]))
    assert ds.centre_local.dtype == torch.int32
    csz = [int(p[1].shape[0]) for p in parts]
    for d in (ds, ball):  # the centre lists are kept whatever pool is
        assert d.centre_sizes_h.tolist() == csz and d.n_centre == sum(csz)
        assert torch.equal(d.centre_ptr.cpu().long(), torch.tensor([0] + list(np.cumsum(csz))))
        assert torch.equal(d.centre_nodes.cpu().long(), torch.cat([p[0][p[1]] for p in parts]))
    for k in ("sub_nodes", "sub_ptr", "centre_nodes", "centre_ptr", "centre_local", "rowptr_in", "col_in", "val_in",
              "rowptr_out", "col_out", "val_out"):
        assert _same_bits(getattr(ds, k), getattr(ds2, k)), k
        if k != "centre_local":
            assert _same_bits(getattr(ds, k), getattr(ball, k)), k
    for ids in _batch_orders(len(ds)):
        bt, bt2, bb = ds.collate(ids), ds2.collate(ids), ball.collate(ids)
        opos, omark = C.batch(parts, list(ids))
        assert bt.pos.dtype == torch.int64 and torch.equal(bt.pos.cpu(), opos)
        assert bt.mark.dtype == torch.uint8 and torch.equal(bt.mark.cpu(), omark)
        assert bb.mark is None  # ball mode at hop > 0 does not locate the centres
        for get in (lambda b: b.node_map, lambda b: b.adj.fwd.rowptr, lambda b: b.adj.fwd.col, lambda b: b.adj.fwd.val,
                    lambda b: b.adj.bwd.rowptr, lambda b: b.adj.bwd.col, lambda b: b.adj.bwd.val, lambda b: b.x,
                    lambda b: b.y, lambda b: b.ids):
            assert _same_bits(get(bt), get(bb)) and _same_bits(get(bt), get(bt2))
        assert _same_bits(bt.pos, bt2.pos) and _same_bits(bt.mark, bt2.mark)
        assert bt.as_tuple()[3] is bt.pos and len(bt.as_tuple()) == 5
    return ds, parts


CASES = [(name, mode, hop) for name in ("density", "component", "synthetic:ppi_bp") for hop in (1, 2)
         for mode in ("gcn", "gin")]


@pytest.mark.parametrize("name,mode,hop", CASES)
def test_centre_index_pos_and_mark_match_the_oracle(name, mode, hop):
    ds, parts = _check_centre_split(name, mode, hop)
    assert ds.n_member > ds.n_centre  # (the balls did grow: some rows are context only)


@pytest.mark.parametrize("size", LDS_EDGE_BALL)
def test_both_sides_of_the_lds_threshold(size):
    for mode in ("gcn", "gin"):
        ds, parts = _check_centre_split(f"hub{size}", mode, 1)
        assert int(ds.sizes_h.max()) == size and ds.sizes_h[0] == size
        lo = int(ds.centre_ptr[0])
        assert ds.centre_local[lo:lo + 4].tolist() == [0, 7, size - 2, size - 1]


@pytest.mark.parametrize("mode,hop", [("gcn", 1), ("gin", 3)])
def test_isolated_centre_and_duplicated_id_are_marked_and_pooled_once(mode, hop):
    from glass_amd import ops
    ds, parts = _check_centre_split("isolated", mode, hop)
    (x, ei, w, pos, y), _ = _case("isolated", hop)
    n = x.shape[0] - 1
    assert pos[0, :3].tolist() == [7, 7, 3] and pos[3, 0] == n and pos[4, :2].tolist() == [n, 5]
    bt = ds.collate(np.arange(len(ds)))
    one = torch.ones(bt.node_map.shape[0], 1, device=DEV)
    pooled = ops.segment_pool(one, bt.pos, "sum").cpu().flatten()
    assert pooled.tolist() == [float(len(set(r[r >= 0].tolist()))) for r in pos]
    assert pooled[0] == 2 and pooled[3] == 1
    off = np.concatenate(([0], np.cumsum(ds.sizes_h)))
    mark, node_map = bt.mark.cpu(), bt.node_map.cpu()
    assert int(ds.sizes_h[3]) == 1 and mark[off[3]] == 1 and node_map[off[3]] == n  # alone in its ball, marked
    blk = slice(off[0], off[1])
    assert sorted(node_map[blk][mark[blk] == 1].tolist()) == [3, 7] and int(mark[blk].sum()) == 2
    assert int(mark.sum()) == int(pooled.sum())


# ---- hop 0: pool="centre" is pool="ball" ---------------------------------------------------------------------------
def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, sorted({e.name for e in prof.events() if "_kernel" in e.name})


@pytest.mark.parametrize("name,mode", [("density", "gin"), ("component", "gcn"), ("synthetic:ppi_bp", "gcn")])
def test_hop_zero_centre_is_ball_and_launches_nothing_new(name, mode):
    x, ei, w, pos, y = _graph(name)
    ids = np.random.default_rng(5).permutation(pos.shape[0])[:max(2, pos.shape[0] - 3)]

    def make(pool, hop=0):
        ds = _dataset(x, ei, w, pos, y, mode, hop, pool)
        return ds, ds.collate(ids)

    (a, ba), names_ball = _kernel_names(lambda: make("ball"))
    (b, bb), names = _kernel_names(lambda: make("centre"))
    assert any("seg_collate_kernel" in k for k in names) and any("seg_fill_kernel" in k for k in names)
    assert not any("centre" in k or "khop" in k for k in names), names
    assert [k for k in names if "seg_" in k] == [k for k in names_ball if "seg_" in k]
    # (the same profile does see the new kernels where they run)
    _, names_hop1 = _kernel_names(lambda: make("centre", 1))
    assert any("seg_centre_index_kernel" in k for k in names_hop1)
    assert any("seg_collate_centre_kernel" in k for k in names_hop1)
    assert not any("seg_collate_kernel" in k for k in names_hop1)  # one collate launch per batch, not two
    assert b.centre_local is None and b.centre_ptr is b.sub_ptr and b.centre_nodes is b.sub_nodes
    for k in ("sub_nodes", "sub_ptr", "rowptr_in", "rowptr_out", "col_in", "val_in", "col_out", "val_out", "deg"):
        u, v = getattr(a, k), getattr(b, k)
        assert (u is None and v is None) or _same_bits(u, v), k
    for k in ("sizes_h", "sub_ptr_h", "cnt_in_h", "cnt_out_h", "centre_sizes_h"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert np.array_equal(b.centre_sizes_h, b.sizes_h)
    for u, v in zip(ba.as_tuple(), bb.as_tuple()):
        if isinstance(u, torch.Tensor):
            assert _same_bits(u, v)
    for get in (lambda t: t.node_map, lambda t: t.adj.fwd.rowptr, lambda t: t.adj.fwd.col, lambda t: t.adj.fwd.val,
                lambda t: t.adj.bwd.rowptr, lambda t: t.adj.bwd.col, lambda t: t.adj.bwd.val):
        assert _same_bits(get(ba), get(bb))
    for t in (ba, bb):
        assert t.mark.dtype == torch.uint8 and t.mark.shape == t.node_map.shape and bool((t.mark == 1).all())


def _driver(*flags, epochs="3", seed=None):
    """The driver in a fresh process.  seed: torch's global generator is seeded before the driver's main() — the
    train/valid/test split is drawn from it when the dataset loads (as in the reference), before any set_seed."""
    argv = ["--dataset", "density", "--repeat", "1", "--epochs", epochs, *flags]
    cmd = [sys.executable, "GNNSeg.py", *argv] if seed is None else \
        [sys.executable, "-c", f"import torch; torch.manual_seed({seed}); import GNNSeg; GNNSeg.main({argv!r})"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=dict(os.environ))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


def test_hop_zero_driver_prints_the_same_lines_in_both_modes():
    outs = [_driver("--pool", pool, epochs="6", seed=11) for pool in ("ball", "centre")]
    assert "pool='ball'" in outs[0] and "pool='centre'" in outs[1] and "hop=0" in outs[1]
    lines = [[ln for ln in out.splitlines() if not ln.startswith("Namespace(")] for out in outs]
    assert lines[0] == lines[1]
    assert sum(ln.startswith("iter ") for ln in lines[0]) >= 2 and any(ln.startswith("end: val ") for ln in lines[0])


def test_driver_runs_density_at_hop_one_with_centre_pooling():
    out = _driver("--hop", "1", "--pool", "centre")
    assert "hop=1" in out and "pool='centre'" in out and "repeat 0" in out and "iter 0 loss " in out and " val " in out
    end = [ln for ln in out.splitlines() if ln.startswith("end: val ")]
    assert len(end) == 1
    tst = float(end[0].split()[-1])
    assert np.isfinite(tst) and 0.0 <= tst <= 1.0
    assert "tst scores [" in out and "best params {'conv_layer': 1, 'dropout': 0.4, 'hidden_dim': 16}" in out


# ---- the model on centre-pooled batches ----------------------------------------------------------------------------
MODEL_CASES = [("density", "gin", 1, 16, 1), ("density", "gin", 1, 16, 2), ("component", "gcn", 3, 64, 1),
               ("component", "gcn", 3, 64, 2)]


@pytest.mark.parametrize("name,mode,L,H,hop", MODEL_CASES)
def test_gnn_forward_loss_and_gradients_match_fp64(name, mode, L, H, hop):
    """Logits, loss and the flat parameter gradient against the fp64 restatement on the same batch, rel-inf <= 1e-5 (the
    bar of every GPU parity test here).  The pool backward leaves the rows absent from pos at exactly 0: the gradient
    of the layer stack's output is 0 on every row whose mark is 0, while one layer earlier (L >= 2) such rows do
    receive gradient through the aggregation, so the context takes part in the training."""
    from glass_amd import seg
    (x, ei, w, pos, y), parts = _case(name, hop)
    n_out = int(y.max()) + 1
    ds = _dataset(x, ei, w, pos, y, mode, hop, "centre")
    loader = seg.GsDataloader(ds, len(ds), shuffle=False, drop_last=False)
    (bx, adj, ew, bpos, by), = list(loader)
    mark = ds.collate(np.arange(len(ds))).mark.cpu()
    opos, omark = C.batch(parts, list(range(len(ds))))
    assert torch.equal(bpos.cpu(), opos) and torch.equal(mark, omark)
    assert int((mark == 0).sum()) > 0 and bpos.shape[1] < int(ds.sizes_h.max())
    model = _build(mode, x.shape[-1], H, L, n_out)
    model.train()
    grads = {}

    def keep(key):
        def hook(g):
            grads[key] = g.detach().clone()
        return hook

    def on_stack_output(module, inputs, out):  # (returns None: the output itself goes on)
        out.register_hook(keep("out"))

    def on_last_conv_input(module, inputs):
        inputs[0].register_hook(keep("inner"))

    model.mods[0].register_forward_hook(on_stack_output)
    if L >= 2:
        model.mods[0].convs[-1].register_forward_pre_hook(on_last_conv_input)
    pred = model(bx, adj, ew, bpos)
    loss = torch.nn.CrossEntropyLoss()(pred, by)
    loss.backward()
    g_out = grads["out"].cpu()
    assert g_out.shape == (bx.shape[0], H * L)
    assert bool((g_out[mark == 0] == 0).all()) and bool((g_out[mark == 1] != 0).any())
    if L >= 2:
        assert bool((grads["inner"].cpu()[mark == 0] != 0).any())

    p = {k: v.detach().cpu().double().requires_grad_() for k, v in model.named_parameters()}
    n = bx.shape[0]
    blocks = K.split_blocks(ei, w.double(), pos, mode, hop, x.shape[0])
    _, (rp, col, val), _, ball_pos = O.collate(blocks, list(range(len(ds))))
    assert ball_pos.shape[0] == opos.shape[0] and int((ball_pos >= 0).sum()) == n
    A = _sparse((rp, col, val), n)
    mlp_keys = sorted({k.rsplit(".", 1)[0] + "." for k in p if k.startswith("mods.1.")})
    po = O.gnn(p, bx.cpu(), A, opos, mode, L, mlp_keys)  # the readout over the oracle's centre rows
    lo = torch.nn.CrossEntropyLoss()(po, by.cpu())
    lo.backward()
    e_pred = rel_inf(pred.detach().cpu(), po.detach())
    keys = sorted(p)
    e_grad = rel_inf(flat_grads({k: v.grad.cpu() for k, v in model.named_parameters()}, keys),
                     flat_grads({k: v.grad for k, v in p.items()}, keys))
    e_loss = abs(loss.item() - lo.item()) / abs(lo.item())
    print(f"{name} {mode} hop {hop} L {L} H {H}: {n} nodes, {int(mark.sum())} centres, pred rel-inf {e_pred:.2e}, "
          f"loss rel {e_loss:.2e}, grad rel-inf {e_grad:.2e}")
    assert e_pred <= 1e-5
    assert e_loss <= 1e-5
    assert e_grad <= 1e-5
