"""GNN-seg, the baseline the GLASS paper compares against (reference GNNSeg.py), on the HIP path.

Every subgraph of a split becomes its own graph — the induced subgraph of its sorted unique node ids at hop 0
(GNNSeg.py:213-226), or of their radius-k in-ball at hop k > 0 (GNNSeg.py:213-232) — and batches are disjoint unions of
those graphs (GNNSeg.py:41-62).  Here:

  * `SegBase`: the base graph as CSR in both orientations (torch index plumbing, once per graph);
  * `GsDataset`: one split, extracted by the K10 kernels (glass_seg_extract_count -> torch scan -> glass_seg_extract_fill)
    into per-subgraph local CSR blocks, in the value mode of the model's convolution (GCN norm or GIN's A + I); at
    hop > 0 the node lists are first grown into k-hop in-balls (glass_seg_khop_count -> host sum -> glass_seg_khop_fill);
  * `GsDataloader`: one glass_seg_collate launch per batch writes the batch's block-diagonal CSR pair, its node map and
    its pool matrix; the row pointers and K1 plans are host arithmetic on the row lengths kept at split time (no
    device->host sync); batches of a loader without shuffle are built once and reused;
  * `GsDataset(pool="centre")` at hop > 0: message passing runs over the ball, the readout over the subgraph's own nodes.
    glass_seg_centre_index finds every centre in its ball once per split (the reference's `inv`, GNNSeg.py:214-225), and
    glass_seg_collate_centre is then the batch's one launch: the same CSR pair and node map, a pool matrix that lists
    only the centres' rows, and the 0/1 centre mark of every batch row (the reference's Data.pos);
  * `GCNConv`, `MyGINConv`, `GConv`, `GNN`: the reference's models (PyG 1.7.2 parameter names and shapes), aggregating on
    K1 (graph.CSROperand: target-major forward, source-major backward), GraphNorm + ELU on the GraphNorm kernels, the sum
    pool on the segment-pool kernels.

Orientation follows PyG: messages flow from edge_index[0] (source) to edge_index[1] (target), where they are summed.
"""
import math

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, ops
from .graph import CSROperand, _csr_from_sorted
from .models import GraphNorm, _act_code, _head


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _scan(counts):
    rp = torch.zeros(counts.shape[0] + 1, dtype=torch.int64, device=counts.device)
    rp[1:] = torch.cumsum(counts, 0)
    return rp.to(torch.int32)


class SegBase:
    """The base graph by target (in_*: rows edge_index[1], columns sources) and by source (out_*: rows edge_index[0],
    columns targets), (row, column)-sorted, duplicate edges kept in base order."""
    def __init__(self, edge_index, edge_weight, n_node):
        if not edge_index.is_cuda:
            raise _lib.GlassHipError("GNN-seg runs on the GPU only (edge_index is on %s)" % edge_index.device)
        n = int(n_node)
        if n >= 2**31 - 1 or edge_index.shape[1] >= 2**31 - 1:
            raise _lib.GlassHipError("int32 CSR: need n_node, nnz < 2^31")
        self.n_node = n
        src, dst = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
        w = edge_weight.to(device=edge_index.device, dtype=torch.float32)
        perm = torch.argsort(dst * n + src, stable=True)
        self.in_rowptr = _csr_from_sorted(dst[perm], n)
        self.in_col = src[perm].to(torch.int32).contiguous()
        self.in_w = w[perm].contiguous()
        perm = torch.argsort(src * n + dst, stable=True)
        self.out_rowptr = _csr_from_sorted(src[perm], n)
        self.out_col = dst[perm].to(torch.int32).contiguous()
        self.out_w = w[perm].contiguous()


def _ptr(t):
    return t.data_ptr() if t is not None and t.numel() else None


class SegAdj:
    """The normalised adjacency of one batch: fwd = target-major CSR (y[dst] = sum val * x[src]), bwd = its transpose.
    Takes the place of edge_index in the model calls (ops.spmm reads .fwd / .bwd).  seg_ptr: the int32 device vector
    [B + 1] of the row offsets of the batch's graphs (what the per-graph GraphNorm of GConv(graph_norm="graph") reads)."""
    def __init__(self, fwd, bwd, mode, seg_ptr=None):
        self.fwd, self.bwd, self.mode, self.seg_ptr = fwd, bwd, mode, seg_ptr
        self.n_node = fwd.n_rows

    def edge_index(self):
        """[2, nnz] (source, target) of the target-major entries (for checks; not on the hot path)."""
        rp = self.fwd.rowptr.to(torch.int64)
        dst = torch.repeat_interleave(torch.arange(self.n_node, device=rp.device), rp[1:] - rp[:-1])
        return torch.stack((self.fwd.col.to(torch.int64), dst))


class SegBatch:
    """Device operands of one collated batch (the tensors the CSR operands point into are held here).  pos lists the rows
    the readout pools: every row of a block, or, for a GsDataset(pool="centre") at hop > 0, the rows of its centres.
    mark (uint8 per batch row, 1 on a centre: the reference's Data.pos over the batch) is written by the centre collate;
    at hop 0 every row is a centre and the all-ones mark is made when first read (no launch on the collate path); in
    ball mode at hop > 0 the split never located its centres and mark is None."""
    def __init__(self, ds, ids):
        ids = np.asarray(ids, dtype=np.int64)
        dev = ds.pos.device
        sizes = ds.sizes_h[ids]
        node_off = np.zeros(ids.shape[0] + 1, dtype=np.int64)
        np.cumsum(sizes, out=node_off[1:])
        n = int(node_off[-1])
        rows = np.repeat(ds.sub_ptr_h[ids] - node_off[:-1], sizes) + np.arange(n, dtype=np.int64)
        brow_in = np.zeros(n + 1, dtype=np.int64)
        brow_out = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(ds.cnt_in_h[rows], out=brow_in[1:])
        np.cumsum(ds.cnt_out_h[rows], out=brow_out[1:])
        nnz_in, nnz_out = int(brow_in[-1]), int(brow_out[-1])
        if n >= 2**31 - 1 or nnz_in >= 2**31 - 1:
            raise _lib.GlassHipError("int32 CSR: batch too large")
        centre = ds.centre_local is not None
        pooled = ds.centre_sizes_h[ids] if centre else sizes
        width = max(int(pooled.max()) if pooled.size else 0, 1)
        host = np.concatenate((ids, node_off, brow_in, brow_out)).astype(np.int32)
        up = torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)
        B = ids.shape[0]
        self.ids = up[:B].to(torch.int64)
        node_off_d = up[B:2 * B + 1]
        brow_in_d = up[2 * B + 1:2 * B + n + 2]
        brow_out_d = up[2 * B + n + 2:]
        col_in = torch.empty(nnz_in, dtype=torch.int32, device=dev)
        val_in = torch.empty(nnz_in, dtype=torch.float32, device=dev)
        col_out = torch.empty(nnz_out, dtype=torch.int32, device=dev)
        val_out = torch.empty(nnz_out, dtype=torch.float32, device=dev)
        self.node_map = torch.empty(n, dtype=torch.int32, device=dev)
        self.pos = torch.empty((B, width), dtype=torch.int64, device=dev)
        split = (ds.sub_ptr.data_ptr(), _ptr(ds.sub_nodes), ds.n_sub, ds.rowptr_in.data_ptr(), _ptr(ds.col_in),
                 _ptr(ds.val_in), ds.rowptr_out.data_ptr(), _ptr(ds.col_out), _ptr(ds.val_out))
        batch = (up.data_ptr(), B, node_off_d.data_ptr(), n, brow_in_d.data_ptr(), brow_out_d.data_ptr(), _ptr(col_in),
                 _ptr(val_in), _ptr(col_out), _ptr(val_out), _ptr(self.node_map), self.pos.data_ptr(), width)
        self._all_centres = ds.hop == 0
        if centre:
            self._mark = torch.empty(n, dtype=torch.uint8, device=dev)
            rc = _lib.load().glass_seg_collate_centre(*split, ds.centre_ptr.data_ptr(), _ptr(ds.centre_local),
                                                      ds.n_centre, *batch, _ptr(self._mark), _stream())
            _lib.check(rc, "glass_seg_collate_centre")
        else:
            self._mark = None
            _lib.check(_lib.load().glass_seg_collate(*split, *batch, _stream()), "glass_seg_collate")
        self.adj = SegAdj(CSROperand(brow_in_d, col_in, val_in, n, n, rowptr_host=brow_in.astype(np.int32)),
                          CSROperand(brow_out_d, col_out, val_out, n, n, rowptr_host=brow_out.astype(np.int32)), ds.mode,
                          seg_ptr=node_off_d)
        self.x = ds.x[self.node_map.to(torch.int64)]
        self.y = ds.y[self.ids]

    @property
    def mark(self):
        if self._mark is None and self._all_centres:
            self._mark = torch.ones(self.node_map.shape[0], dtype=torch.uint8, device=self.node_map.device)
        return self._mark

    def as_tuple(self):
        """(x [n,C,F], edge_index slot, edge_weight slot, pos, y): the reference loader's 5-tuple; the edge_index slot
        holds the batch's SegAdj, the edge_weight slot its target-major values."""
        return self.x, self.adj, self.adj.fwd.val, self.pos, self.y


class GsDataset:
    """One split of GNN-seg: every subgraph (a row of pos, -1 padding) cut out of the base graph as its induced subgraph.
    mode: "gcn" (values of PyG's gcn_norm without self-loops) or "gin" (A + I, unit weights) — the convolution the model
    uses.  base: a SegBase of (edge_index, edge_attr) shared by the splits of one graph (built here when None).
    hop: k_hop_subgraph's num_hops (GNNSeg.py:213-232) — hop > 0 replaces each row's nodes by their radius-hop in-ball
    (glass_seg_khop_count / _fill) before the extraction.
    pool: "ball" (the reference: the batch pools over every node of the ball) or "centre" (it pools over the subgraph's
    own nodes only, the ones the reference marks in Data.pos, GNNSeg.py:214-225; the ball is context for the message
    passing).  At hop 0 the two are the same batches.  The centre lists stay in centre_ptr / centre_nodes /
    centre_sizes_h either way; centre_local (each centre's row within its ball's block) exists for "centre" at hop > 0."""
    def __init__(self, x, edge_index, edge_attr, pos, y, mode="gcn", base=None, hop=0, pool="ball"):
        if mode not in _lib.SEG_MODES:
            raise NotImplementedError(f"GsDataset mode {mode!r}: gcn or gin")
        if pool not in ("ball", "centre"):
            raise ValueError(f"GsDataset pool {pool!r}: \"ball\" or \"centre\"")
        if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or hop < 0:
            raise ValueError(f"GsDataset hop {hop!r}: a non-negative integer")
        if hop >= 2**31:
            raise ValueError(f"GsDataset hop {hop}: below 2^31")
        if not pos.is_cuda:
            raise _lib.GlassHipError("GNN-seg runs on the GPU only (pos is on %s)" % pos.device)
        self.mode = mode
        self.x = x if x.dtype == torch.float32 else x.to(torch.float32)
        self.y = y
        self.pos = pos
        n = x.shape[0]
        self.base = base if base is not None else SegBase(edge_index, edge_attr, n)
        if self.base.n_node != n:
            raise _lib.GlassHipError(f"base graph has {self.base.n_node} nodes, x has {n}")
        # sorted unique node list of every subgraph (duplicates in a pos row merge into one node)
        p = torch.where(pos >= 0, pos, torch.full_like(pos, n)).to(torch.int64)
        p = torch.sort(p, dim=1).values
        keep = p < n
        keep[:, 1:] &= p[:, 1:] != p[:, :-1]
        sizes = keep.sum(1)
        self.n_sub = pos.shape[0]
        self.sub_nodes = p[keep].to(torch.int32).contiguous()
        self.sub_ptr = _scan(sizes)
        self.n_member = int(self.sub_nodes.shape[0])
        self.hop = int(hop)
        self.pool = pool
        dev = pos.device
        self.centre_ptr, self.centre_nodes, self.n_centre = self.sub_ptr, self.sub_nodes, self.n_member
        self.centre_sizes_h = self.centre_local = None
        cl_min = None
        if self.hop > 0:
            self.centre_sizes_h = sizes.cpu().numpy().astype(np.int64)  # (_balls' own read would wait for the same work)
            sizes = self._balls(n)
            if pool == "centre":
                self.centre_local = torch.empty(self.n_centre, dtype=torch.int32, device=dev)
                rc = _lib.load().glass_seg_centre_index(self.centre_ptr.data_ptr(), _ptr(self.centre_nodes), self.n_sub,
                                                        self.n_centre, self.sub_ptr.data_ptr(), _ptr(self.sub_nodes),
                                                        self.n_member, _ptr(self.centre_local), _stream())
                _lib.check(rc, "glass_seg_centre_index")
                if self.n_centre:
                    cl_min = self.centre_local.min().reshape(1)
        cnt_in = torch.empty(self.n_member, dtype=torch.int32, device=dev)
        cnt_out = torch.empty(self.n_member, dtype=torch.int32, device=dev)
        self.deg = torch.empty(self.n_member, dtype=torch.float32, device=dev) if mode == "gcn" else None
        b = self.base
        lib, m = _lib.load(), _lib.SEG_MODES[mode]
        rc = lib.glass_seg_extract_count(b.in_rowptr.data_ptr(), _ptr(b.in_col), _ptr(b.in_w), b.out_rowptr.data_ptr(),
                                         _ptr(b.out_col), n, self.sub_ptr.data_ptr(), _ptr(self.sub_nodes), self.n_sub,
                                         self.n_member, m, _ptr(cnt_in), _ptr(cnt_out), _ptr(self.deg), _stream())
        _lib.check(rc, "glass_seg_extract_count")
        self.rowptr_in, self.rowptr_out = _scan(cnt_in), _scan(cnt_out)
        # the split's one host sync: the row lengths every batch's row pointer and plan are built from
        self.sizes_h = sizes.cpu().numpy().astype(np.int64)
        if cl_min is None:
            self.sub_ptr_h = self.sub_ptr.cpu().numpy().astype(np.int64)
        else:  # the smallest centre_local rides in the same read-back
            self.sub_ptr_h = torch.cat((self.sub_ptr, cl_min)).cpu().numpy().astype(np.int64)
            lowest, self.sub_ptr_h = int(self.sub_ptr_h[-1]), self.sub_ptr_h[:-1]
            if lowest < 0:
                raise _lib.GlassHipError("glass_seg_centre_index: a centre is missing from its own ball (centre_local "
                                         f"min {lowest})")
        if self.centre_sizes_h is None:
            self.centre_sizes_h = self.sizes_h
        self.cnt_in_h = cnt_in.cpu().numpy().astype(np.int64)
        self.cnt_out_h = cnt_out.cpu().numpy().astype(np.int64)
        nnz_in, nnz_out = int(self.cnt_in_h.sum()), int(self.cnt_out_h.sum())
        if nnz_in >= 2**31 - 1:
            raise _lib.GlassHipError("int32 CSR: split too large")
        self.col_in = torch.empty(nnz_in, dtype=torch.int32, device=dev)
        self.val_in = torch.empty(nnz_in, dtype=torch.float32, device=dev)
        self.col_out = torch.empty(nnz_out, dtype=torch.int32, device=dev)
        self.val_out = torch.empty(nnz_out, dtype=torch.float32, device=dev)
        rc = lib.glass_seg_extract_fill(b.in_rowptr.data_ptr(), _ptr(b.in_col), _ptr(b.in_w), b.out_rowptr.data_ptr(),
                                        _ptr(b.out_col), _ptr(b.out_w), n, self.sub_ptr.data_ptr(), _ptr(self.sub_nodes),
                                        self.n_sub, self.n_member, m, _ptr(self.deg), self.rowptr_in.data_ptr(),
                                        self.rowptr_out.data_ptr(), _ptr(self.col_in), _ptr(self.val_in),
                                        _ptr(self.col_out), _ptr(self.val_out), _stream())
        _lib.check(rc, "glass_seg_extract_fill")

    def _balls(self, n):
        """Replaces sub_nodes / sub_ptr (the centres, kept as centre_nodes / centre_ptr) by the sorted unique in-balls of
        radius self.hop; returns the ball sizes.  One host read of the sizes, whose int64 sum is checked before anything
        is allocated for the fill."""
        b, lib, dev = self.base, _lib.load(), self.pos.device
        ws_bytes = lib.glass_seg_khop_ws_bytes(n, self.n_sub)
        if ws_bytes < 0:
            _lib.check(ws_bytes, "glass_seg_khop_ws_bytes")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
        args = (b.in_rowptr.data_ptr(), _ptr(b.in_col), n, self.sub_ptr.data_ptr(), _ptr(self.sub_nodes), self.n_sub,
                self.n_member, self.hop, _ptr(ws), ws_bytes)
        ball = torch.empty(self.n_sub, dtype=torch.int32, device=dev)
        _lib.check(lib.glass_seg_khop_count(*args, _ptr(ball), _stream()), "glass_seg_khop_count")
        total = int(ball.cpu().numpy().astype(np.int64).sum())
        if total >= 2**31 - 1:
            raise _lib.GlassHipError(f"GsDataset hop {self.hop}: the balls hold {total} nodes in all; int32 node lists "
                                     "need fewer than 2^31 - 1")
        ball_ptr = _scan(ball)
        nodes = torch.empty(total, dtype=torch.int32, device=dev)
        _lib.check(lib.glass_seg_khop_fill(*args, ball_ptr.data_ptr(), _ptr(nodes), _stream()), "glass_seg_khop_fill")
        self.sub_ptr, self.sub_nodes, self.n_member = ball_ptr, nodes, total
        return ball

    def __len__(self):
        return self.n_sub

    def collate(self, ids):
        """SegBatch of the subgraphs `ids` (host integers) in that order."""
        return SegBatch(self, ids)


class GsDataloader:
    """Batches of a GsDataset as (x, edge_index slot, edge_weight slot, pos, y) (GNNSeg.py:41-62).  shuffle draws a
    permutation from torch's global generator per epoch; drop_last drops the last partial batch.  Without shuffle the
    batches never change: they are collated once and reused."""
    def __init__(self, Gsdataset, batch_size=64, shuffle=True, drop_last=True):
        self.Gsdataset = Gsdataset
        self.batch_size = int(batch_size)
        self.shuffle, self.drop_last = shuffle, drop_last
        self._fixed = None

    def _index_batches(self):
        n = len(self.Gsdataset)
        order = torch.randperm(n).numpy() if self.shuffle else np.arange(n)
        bs = self.batch_size
        stop = (n // bs) * bs if self.drop_last else n
        return [order[i:min(i + bs, n)] for i in range(0, stop, bs)]

    def __len__(self):
        n = len(self.Gsdataset)
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def __iter__(self):
        if self.shuffle:
            return (self.Gsdataset.collate(ids).as_tuple() for ids in self._index_batches())
        if self._fixed is None:
            self._fixed = [self.Gsdataset.collate(ids).as_tuple() for ids in self._index_batches()]
        return iter(self._fixed)


# ---------------------------------------------------------------------------------------------------------------------
def _seg_adj(edge_index, mode, who):
    if not isinstance(edge_index, SegAdj):
        raise TypeError(f"{who} takes the SegAdj a GsDataloader yields in the edge_index slot, got {type(edge_index)}")
    if edge_index.mode != mode:
        raise ValueError(f"{who} needs a batch extracted in mode {mode!r} (GsDataset(mode=...)), got {edge_index.mode!r}")
    return edge_index


class _XW(torch.autograd.Function):
    """x @ W with W [in, out] (PyG's layout); the weight gradient x^T @ dy on the split-K kernel where it applies."""
    @staticmethod
    def forward(ctx, x, W):
        ctx.save_for_backward(x, W)
        return x @ W

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        dx = dy @ W.t() if ctx.needs_input_grad[0] else None
        dW = None
        if ctx.needs_input_grad[1]:
            dyc, xc = dy.contiguous(), x.contiguous()
            dW = torch.empty_like(W, memory_format=torch.contiguous_format)
            if not ops.linear_wgrad(xc, dyc, dW, None, accumulate=False, slot=("seg_xw", tuple(W.shape))):
                dW = xc.t() @ dyc
        return dx, dW


class GCNConv(nn.Module):
    """PyG 1.7.2 GCNConv(in, out, add_self_loops=False): out = Â (x @ weight) + bias, Â[dst, src] = dinv[src] w dinv[dst]
    with dinv = (weighted in-degree)^-1/2 (0 where the degree is 0).  Parameters weight [in, out] (glorot), bias [out]."""
    def __init__(self, in_channels, out_channels, add_self_loops=False, bias=True, **kwargs):
        super().__init__()
        if add_self_loops:
            raise NotImplementedError("GCNConv: add_self_loops=True is not supported (GNN-seg uses False)")
        if kwargs:
            raise NotImplementedError(f"GCNConv: unsupported options {sorted(kwargs)}")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels))
        self.bias = nn.Parameter(torch.empty(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.weight.size(-2) + self.weight.size(-1)))
        with torch.no_grad():
            self.weight.uniform_(-a, a)
            if self.bias is not None:
                self.bias.zero_()

    def forward(self, x, edge_index, edge_weight=None):
        adj = _seg_adj(edge_index, "gcn", "GCNConv")
        out = ops.spmm(adj, _XW.apply(x, self.weight))
        return out + self.bias if self.bias is not None else out


class _GINConv(nn.Module):
    """PyG GINConv(nn, eps=0, train_eps=False): nn(x + sum over in-edges of x[src]); edge weights ignored."""
    def __init__(self, mlp):
        super().__init__()
        self.nn = mlp
        self.register_buffer("eps", torch.tensor([0.0]))

    def forward(self, x, edge_index):
        agg = ops.spmm(_seg_adj(edge_index, "gin", "MyGINConv"), x)  # (A + I) x: the diagonal is in the operand
        if isinstance(self.nn, nn.Linear):
            return ops.linear(agg, self.nn)
        return self.nn(agg)


class MyGINConv(nn.Module):
    """GNNSeg.py:161-171: GINConv(nn.Linear(in, out), 0, False); reset_parameters is a no-op (torch's default init)."""
    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = _GINConv(nn.Linear(in_channels, out_channels))

    def reset_parameters(self):
        pass

    def forward(self, x, edge_index, edge_weight=None):
        return self.conv(x, edge_index)


class GConv(nn.Module):
    """num_layers convolutions in -> hidden -> ... -> out with a GraphNorm, the activation and dropout between them; returns
    the concatenation of every layer's output (GNNSeg.py:70-124).  With an in-place activation (the driver's
    ELU(inplace=True)) the stored inner outputs are the ACTIVATED tensors, as in the reference.
    graph_norm: "batch" (the reference: statistics over all rows of the batch, so a subgraph's output depends on the
    subgraphs batched with it) or "graph" (statistics over each subgraph's own rows, the batch's SegAdj.seg_ptr: a
    subgraph's output no longer depends on its batch)."""
    def __init__(self, input_channels, hidden_channels, output_channels, num_layers, dropout=0,
                 activation=nn.ReLU(inplace=True), conv=GCNConv, graph_norm="batch", **kwargs):
        super().__init__()
        if graph_norm not in ("batch", "graph"):
            raise ValueError(f"GConv graph_norm {graph_norm!r}: \"batch\" or \"graph\"")
        self.graph_norm = graph_norm
        dims = [input_channels] + [hidden_channels] * (num_layers - 1) + [output_channels]
        self.convs = nn.ModuleList([conv(in_channels=dims[i], out_channels=dims[i + 1], **kwargs)
                                    for i in range(num_layers)])
        self.activation = activation
        self.dropout = dropout
        self.gns = nn.ModuleList([GraphNorm(hidden_channels) for _ in range(num_layers - 1)])
        self.reset_parameters()

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()
        for gn in self.gns:
            gn.reset_parameters()

    def forward(self, x, edge_index, edge_weight, z=None):
        code = _act_code(self.activation)
        inplace = bool(getattr(self.activation, "inplace", False))
        batch = None
        if self.graph_norm == "graph":
            if getattr(edge_index, "seg_ptr", None) is None:
                raise TypeError("GConv(graph_norm=\"graph\") needs the SegAdj of a collated batch (its seg_ptr)")
            batch = ops.SegPtr(edge_index.seg_ptr)
        xs = []
        for layer, conv in enumerate(self.convs[:-1]):
            h = conv(x, edge_index, edge_weight)
            if inplace and code is not None:
                h = self.gns[layer](h, batch, act=code)  # GraphNorm + activation in one kernel: the tensor the reference stores
                xs.append(h)
            else:
                pre = self.gns[layer](h, batch)
                h = self.activation(pre.clone() if inplace else pre)
                xs.append(h if inplace else pre)
            x = F.dropout(h, p=self.dropout, training=self.training)
        xs.append(self.convs[-1](x, edge_index, edge_weight))
        return torch.cat(xs, dim=-1) if len(xs) > 1 else xs[0]


class GNN(nn.Module):
    """GNNSeg.py:126-158: GConv on every feature channel x[:, c, :], mean over channels, SUM pool over each subgraph's
    nodes (pos), then the prediction MLP.  Parameters mods.0 (GConv), mods.1 (MLP)."""
    def __init__(self, conv, pred, aggr="sum"):
        super().__init__()
        self.mods = nn.ModuleList([conv, pred])

    def _pooled(self, x, edge_index, edge_weight, subG_node):
        C = x.shape[1]
        embs = [self.mods[0](x[:, c, :].contiguous(), edge_index, edge_weight) for c in range(C)]
        emb = embs[0] if C == 1 else torch.stack(embs, dim=1).mean(dim=1)
        return ops.segment_pool(emb, subG_node, "sum")

    def forward(self, x, edge_index, edge_weight, subG_node, id=0):
        emb = self._pooled(x, edge_index, edge_weight, subG_node)
        if not torch.is_grad_enabled() and not self.training:
            return _head(self.mods[1], emb)  # evaluation: a two-layer MLP head in one launch
        return self.mods[1](emb)

    def loss_and_logits(self, x, edge_index, edge_weight, subG_node, y, loss_fn):
        """-> (loss, logits) of one batch: forward up to the pool, then head + loss as four launches forward and
        backward (losses.mlp_head_loss) when the loss is cross-entropy / BCE-with-logits (losses.fusable_spec) and the
        head a two-layer MLP (losses.fusable_head); otherwise the head module and loss_fn(logits, y)."""
        from . import losses
        emb = self._pooled(x, edge_index, edge_weight, subG_node)
        spec = losses.fusable_spec(loss_fn)  # (mode, class weights, pos_weight): a weighted marker keeps its weights
        if spec is not None and losses.fusable_head(self.mods[1]) == "mlp2":
            return losses.mlp_head_loss(emb, self.mods[1], y, spec)
        logits = self.mods[1](emb)
        return loss_fn(logits, y), logits
