"""GLASS model stack on the MI355X HIP kernels — the host-side mirror of the reference's
`impl/models.py` surface (same class names, constructor arguments, forward signatures,
state_dict keys and error types), so `GLASSTest.py`-style drivers are drop-in
callers.  The arithmetic runs in libglass_hip (ops.py); dense Linears stay on rocBLAS through
torch; there is no CPU path.

Reference map (file:line under /root/reference):
  Seq 10-24 · MLP 27-80 · buildAdj 83-111 · GLASSConv 114-174 · EmbZGConv 177-272 ·
  PoolModule/AddPool/MaxPool/MeanPool/SizePool 275-319 · GLASS 322-355   (impl/models.py)
Not in the reference: AttnPool (attention readout, pool "attn"); aggr "max" (max neighbour aggregation, buildAdj); aggr
"softmax" (softmax neighbour aggregation with a learned temperature: the conv layers' parameter `t`); aggr "gat" (attention
aggregation with `gat_heads` heads: GLASSConv's parameters `att_src` and `att_dst`); aggr "gatv2" (dynamic attention, one head:
GLASSConv's parameter `att`); aggr "std" / "var" (the weighted standard deviation / variance of the neighbour messages, GLASSConv only: no parameter, the constant `moment_eps`); aggr "pna" (PNA:
mean, max, min and standard deviation of the neighbour messages under three degree scalers, GLASSConv only: its parameter
`pna_weight` [12, out_channels], the constant `moment_eps`).
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

import os

from . import ops, stack
from .graph import CSRAdj, Selection
from .ops import ACT_ELU, ACT_NONE, ACT_RELU
from .utils import batch2pad


USE_STACK = os.environ.get("GLASS_STACK", "1") != "0"  # A/B switch: whole-stack program vs per-op autograd nodes


# ---------------------------------------------------------------------------------------------
class GraphNorm(nn.Module):
    """GraphNorm (PyG 1.7.2 semantics): parameters `weight`, `bias`, `mean_scale` initialised to 1, 0, 1.
    batch=None normalises over all rows as one graph, and `forward` then optionally fuses the ELU and the inverted dropout
    that follow every GraphNorm in the reference (models.py:166,251,258-259).  With `batch` every graph of a batch is
    normalised over its own rows (ops.graphnorm_seg); the activation is still fused, dropout is not.  With an ops.Replicas as
    `batch` the rows are R replicas of ONE graph (exact zero-one labels): each is normalised over its own N rows by the
    whole-graph kernels' replicated form (ops.graphnorm_rep), activation and dropout fused as for batch=None."""
    def __init__(self, in_channels, eps=1e-5):
        super().__init__()
        self.in_channels, self.eps = in_channels, eps
        self.weight = nn.Parameter(torch.ones(in_channels))
        self.bias = nn.Parameter(torch.zeros(in_channels))
        self.mean_scale = nn.Parameter(torch.ones(in_channels))

    def reset_parameters(self):
        nn.init.ones_(self.weight)
        nn.init.zeros_(self.bias)
        nn.init.ones_(self.mean_scale)

    def forward(self, x, batch=None, act=ACT_NONE, p_drop=0.0, call_id=0, batch_size=None):
        """batch: None; or PyG's sorted int64 vector [n] of graph indices — the number of graphs is `batch_size` when given
        (no device read), else batch[-1] + 1, fetched with the sortedness flag in one read-back; or an ops.SegPtr around the
        int32 row offsets [B + 1] of the graphs (what seg.SegAdj carries), which costs nothing.  An unsorted batch raises
        ValueError where it is looked at (without batch_size)."""
        direct = getattr(self, "_direct_grad", False)
        if isinstance(batch, ops.Replicas):  # R replicas of one graph, N rows each, every replica over its own rows
            return ops.graphnorm_rep(x, batch, self.weight, self.bias, self.mean_scale, self.eps, act, p_drop, call_id, direct)
        if batch is None:
            return ops.graphnorm(x, self.weight, self.bias, self.mean_scale, self.eps, act, p_drop, call_id, direct)
        if p_drop > 0:
            raise ValueError("GraphNorm: dropout is not fused into the per-graph form (batch given); apply it separately")
        if not isinstance(batch, ops.SegPtr):
            batch = ops.SegPtr(_seg_ptr_of(batch, x.shape[0], batch_size))
        return ops.graphnorm_seg(x, batch, self.weight, self.bias, self.mean_scale, self.eps, act, direct)


def _seg_ptr_of(batch, n_rows, batch_size=None):
    """int32 row offsets [B + 1] of a sorted PyG batch vector (int64 [n], graph index per row)."""
    if not isinstance(batch, torch.Tensor) or batch.dtype != torch.int64 or batch.dim() != 1 or batch.shape[0] != n_rows:
        raise ValueError(f"GraphNorm: batch must be an int64 vector with one graph index per row of x ({n_rows})")
    if batch_size is None:
        if n_rows == 0:
            batch_size = 0
        else:
            last, unsorted, first = torch.stack((batch[-1], (batch[1:] < batch[:-1]).any().to(torch.int64), batch[0])).tolist()
            if unsorted or first < 0:
                raise ValueError("GraphNorm: batch must be sorted (non-decreasing graph indices starting at >= 0)")
            batch_size = last + 1
    bounds = torch.arange(int(batch_size) + 1, dtype=torch.int64, device=batch.device)
    return torch.searchsorted(batch, bounds).to(torch.int32)


def _act_code(activation):
    """ELU(alpha=1) (the driver's choice, GLASSTest.py:143) and ReLU (the reference's constructor default,
    impl/models.py:125,192; the pre-training path, GNNEmb.py:90) are fused into the kernels; any other module runs as a
    torch GPU op."""
    if isinstance(activation, nn.ELU) and activation.alpha == 1.0:
        return ACT_ELU
    if type(activation) is nn.ReLU:
        return ACT_RELU
    return None


class Seq(nn.Module):
    """nn.Sequential whose first module also receives the extra positional / keyword arguments."""
    def __init__(self, modlist):
        super().__init__()
        self.modlist = nn.ModuleList(modlist)

    def forward(self, *args, **kwargs):
        it = iter(self.modlist)
        out = next(it)(*args, **kwargs)
        for m in it:
            out = m(out)
        return out


class Linear(nn.Linear):
    """nn.Linear (same parameters, same state_dict keys) whose weight gradient runs on the split-K MFMA kernel
    (ops.LinearFn) — for layers applied to every node or to a large edge batch."""
    def forward(self, x):
        return ops.linear(x, self)


class MLP(nn.Module):
    """Linear / GraphNorm / Dropout / activation stack with the reference's layer ordering
    (GNNEmb / GNNSeg use it; GLASSTest's head is a bare nn.Linear).  The two-layer form without GraphNorm is the one
    losses.fusable_head recognises ("mlp2"): losses.mlp_head_loss in training, _head below in evaluation."""
    def __init__(self, input_channels, hidden_channels, output_channels, num_layers, dropout=0, tail_activation=False,
                 activation=nn.ReLU(inplace=True), gn=False):
        super().__init__()

        def tail(width):
            mods = [GraphNorm(width)] if gn else []
            if dropout > 0:
                mods.append(nn.Dropout(p=dropout, inplace=True))
            return mods + [activation]

        dims = [input_channels] + [hidden_channels] * (num_layers - 1) + [output_channels]
        mods = []
        for i in range(num_layers):
            mods.append(Linear(dims[i], dims[i + 1]))
            if i + 1 < num_layers or tail_activation:
                mods += tail(dims[i + 1])
        self.seq = Seq(mods)

    def forward(self, x):
        return self.seq(x)


# ---------------------------------------------------------------------------------------------
_adj_cache = []  # [(edge_index, edge_weight, n, aggr, CSRAdj)] — tensors are held so pointers stay valid


def buildAdj(edge_index, edge_weight, n_node: int, aggr: str):
    """Normalised adjacency for aggr in {mean,sum,gcn} as a device CSR (graph.CSRAdj) instead of the
    reference's COO.  One instance is shared by every layer asking for the same (graph, aggr) —
    the reference builds an identical copy per layer (models.py:154-156).  aggr "max" (an extension): the raw weights,
    aggregated by ops.spmm with a max instead of a sum.  aggr "softmax" (an extension): the raw weights, strictly positive
    (ValueError otherwise), aggregated by ops.spmm_softmax with the layer's temperature.  aggr "std" / "var" (extensions): built
    like "softmax", aggregated by ops.spmm_moments.  aggr "pna" (an extension): built like "softmax", aggregated by
    ops.spmm_pna / ops.pna_mix."""
    # ("gat" / "gatv2", extensions: built like "softmax", ops.spmm_gat / ops.spmm_gatv2)
    if aggr not in ("mean", "sum", "gcn", "max", "softmax", "gat", "gatv2", "std", "var", "pna"):
        raise NotImplementedError
    for ei, ew, n, a, adj in _adj_cache:
        if ei is edge_index and ew is edge_weight and n == int(n_node) and a == aggr:
            return adj
    adj = CSRAdj(edge_index, edge_weight, n_node, aggr)
    _adj_cache.append((edge_index, edge_weight, int(n_node), aggr, adj))
    del _adj_cache[:-8]
    return adj


def _reset_softmax_t(conv):
    """The temperature of a conv layer with aggr "softmax" back to its constructor value (in place: it may live in an arena)."""
    if conv.aggr == "softmax":
        with torch.no_grad():
            conv.t.fill_(conv.softmax_t)


def _reset_gat_att(conv):
    """The attention vectors of a conv layer with aggr "gat": xavier_uniform_ on the [1, D] view of every head, D = H /
    gat_heads (in place): one uniform_ call per vector with the bound sqrt(6 / (1 + D)) — at one head, xavier_uniform_ on the
    [1, H] view, draw for draw."""
    if conv.aggr == "gat":
        bound = math.sqrt(3.0) * math.sqrt(2.0 / float(1 + conv.att_src.numel() // conv.gat_heads))  # (xavier_uniform_'s own arithmetic)
        with torch.no_grad():
            conv.att_src.uniform_(-bound, bound)
            conv.att_dst.uniform_(-bound, bound)


def _reset_gatv2_att(conv):
    """The attention vector of a conv layer with aggr "gatv2": xavier_uniform_ on its [1, H] view (in place)."""
    if conv.aggr == "gatv2":
        with torch.no_grad():
            nn.init.xavier_uniform_(conv.att.view(1, -1))


def _reset_pna_weight(conv):
    """The twelve views of a conv layer with aggr "pna" back to equal shares (in place: the parameter may live in an arena)."""
    if conv.aggr == "pna":
        with torch.no_grad():
            conv.pna_weight.fill_(1.0 / 12.0)


def set_live_edge_weight(emb):
    """Every GLASSConv layer of `emb` to live edge weights (what their constructor argument sets)."""
    for c in emb.convs:
        if getattr(c, "aggr", None) not in ("sum", "mean", "gcn") or not isinstance(c, GLASSConv):
            raise ValueError(f"live_edge_weight needs GLASSConv layers with aggr 'sum', 'mean' or 'gcn', not "
                             f"{type(c).__name__} with aggr {getattr(c, 'aggr', None)!r}")
        if getattr(c, "edge_dropout", 0.0) > 0:
            raise ValueError("live_edge_weight is not available together with edge_dropout")
    for c in emb.convs:
        c.live_edge_weight = True


def _check_edge_dropout(p, aggr, live_edge_weight):
    """The edge dropout rate as a float, or ValueError: outside [0, 1); > 0 with an aggregation other than "sum" / "mean" / "gcn"
    (those need the entry excluded, not weighted zero) or together with live_edge_weight."""
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not (0.0 <= float(p) < 1.0):
        raise ValueError(f"GLASSConv: edge_dropout must be a number in [0, 1), not {p!r}")
    p = float(p)
    if p > 0 and aggr not in ("sum", "mean", "gcn"):
        raise ValueError(f"GLASSConv: edge_dropout needs aggr 'sum', 'mean' or 'gcn', not {aggr!r} (the other aggregations "
                         "need a dropped entry excluded, not weighted zero)")
    if p > 0 and live_edge_weight:
        raise ValueError("GLASSConv: edge_dropout is not available together with live_edge_weight")
    return p


def set_edge_dropout(emb, p, symmetric=None):
    """Every GLASSConv layer of `emb` to edge dropout rate p (what their constructor argument sets; ValueError, before any layer
    is changed, where a layer's constructor would refuse it).  symmetric: None keeps each layer's key mode."""
    for c in emb.convs:
        if not isinstance(c, GLASSConv):
            raise ValueError(f"edge_dropout needs GLASSConv layers, not {type(c).__name__}")
        _check_edge_dropout(p, c.aggr, c.live_edge_weight)
    for c in emb.convs:
        c.edge_dropout = float(p)
        if symmetric is not None:
            c.edge_dropout_symmetric = bool(symmetric)


class GLASSConv(nn.Module):
    """Labeled message-passing layer: two weight sets (index 1 = labeled, 0 = unlabeled) mixed by
    z_ratio before and after the neighbour aggregation.  aggr "gat" (an extension): attention over the mixed messages, the
    layer owns att_src and att_dst ([out_channels] each) and the constants gat_slope (LeakyReLU's negative slope) and
    gat_heads: K heads partition the channels (head h: channels [h D, (h + 1) D), D = out_channels / K, of the messages, the
    result and both vectors), each with its own softmax; the output width and the state_dict do not depend on K.  K must
    divide out_channels and D be a power of two in [4, 256] (ValueError at construction; other aggregations ignore it).
    aggr "gatv2" (an extension, GATv2): dynamic attention over the mixed messages, one head — the score of an entry is att .
    LeakyReLU(m[destination] + m[source]), the non-linearity before the dot, so a destination ranks its neighbours in an order
    of its own.  The layer owns att ([out_channels]) and the constant gat_slope; the state_dict is that of aggr "mean" plus
    `att`; gat_heads other than 1 is a ValueError at construction; one graph at a time (ValueError with `batch`,
    live_edge_weight or edge_dropout).
    live_edge_weight (an extension, aggr "sum" / "mean" / "gcn" only: ValueError otherwise): the layer aggregates with the
    `edge_weight` of EACH call (ops.spmm_w: the normalisation is evaluated again, and the result is differentiable in the
    weights) on the structure cached from the first call; no parameter, the same state_dict.  Such a layer runs as per-op
    autograd nodes: the stack program (stack.StackProgram, the captured step program of step.TrainStep) declines its model.
    aggr "std" / "var" (extensions): the layer aggregates with the weighted standard deviation sqrt(Var + moment_eps) or the
    weighted variance of the mixed messages (ops.spmm_moments' first result: the widths do not change); no parameter, the
    state_dict of aggr "mean"; one graph at a time (ValueError with `batch` or live_edge_weight).
    aggr "pna" (an extension, PNA): the layer aggregates with ops.pna_mix of ops.spmm_pna's four results — mean, max, min and
    standard deviation sqrt(Var + moment_eps) of the mixed messages, each under the scalers 1, log(W + 1) / delta and
    delta / log(W + 1) (W the node's weight sum, delta the graph's mean of log(W + 1)), the twelve views weighted per channel
    by the layer's parameter pna_weight [12, out_channels] (1 / 12 each at the start: the widths do not change, and PNA's
    dense post-tower is the comb pair this layer already has).  The state_dict is that of aggr "mean" plus `pna_weight`; one
    graph at a time (ValueError with `batch` or live_edge_weight).
    edge_dropout=p (an extension, DropEdge; 0 <= p < 1, aggr "sum" / "mean" / "gcn" only, not with live_edge_weight or `batch`:
    ValueError otherwise): every TRAINING forward draws one keep bit per adjacency entry on the GPU (ops.spmm_dropedge, stream
    call_base + 2: each layer its own mask, a new one every step) and aggregates with the normalisation of the surviving
    weights; edge_dropout_symmetric (default True) gives both directions of an undirected edge, and parallel duplicates, one
    fate.  There is NO 1 / (1 - p) rescale (PyG's dropout_edge has none): "mean" and "gcn" renormalise by construction, "sum"
    does not — its aggregate shrinks by 1 - p in expectation.  A dropped entry stays in the structure at weight +0.0, so a
    non-finite source row still propagates, as at a stored weight of 0.  In eval mode or at p == 0 nothing is drawn or launched
    and the results are bit for bit those of a layer without the argument; no parameter, the same state_dict.  Such a layer
    runs as per-op autograd nodes (the stack program declines its model)."""
    def __init__(self, in_channels: int, out_channels: int, activation=nn.ReLU(inplace=True), aggr="mean",
                 z_ratio=0.8, dropout=0.2, softmax_t=1.0, gat_slope=0.2, gat_heads=1, live_edge_weight=False, moment_eps=1e-5,
                 edge_dropout=0.0, edge_dropout_symmetric=True):
        super().__init__()
        if live_edge_weight and aggr not in ("sum", "mean", "gcn"):
            raise ValueError(f"GLASSConv: live_edge_weight needs aggr 'sum', 'mean' or 'gcn', not {aggr!r} (no edge-weight "
                             "gradient for the other aggregations)")
        self.live_edge_weight = bool(live_edge_weight)
        self.edge_dropout = _check_edge_dropout(edge_dropout, aggr, self.live_edge_weight)
        self.edge_dropout_symmetric = bool(edge_dropout_symmetric)
        self.trans_fns = nn.ModuleList([nn.Linear(in_channels, out_channels), nn.Linear(in_channels, out_channels)])
        self.comb_fns = nn.ModuleList([nn.Linear(in_channels + out_channels, out_channels),
                                       nn.Linear(in_channels + out_channels, out_channels)])
        self.adj = None
        self.activation = activation
        self.aggr = aggr
        self.gn = GraphNorm(out_channels)
        self.z_ratio = z_ratio
        self.dropout = dropout
        self.call_base = 0  # set by EmbZGConv: distinguishes dropout streams of different layers
        self.softmax_t = float(softmax_t)
        if aggr == "softmax":  # (no other configuration owns the key: their state_dict is unchanged)
            self.t = nn.Parameter(torch.full((1, ), self.softmax_t))
        self.moment_eps = float(moment_eps)
        if aggr == "pna":  # (likewise: only this configuration owns the key)
            self.pna_weight = nn.Parameter(torch.full((12, out_channels), 1.0 / 12.0))
        self.gat_slope = float(gat_slope)
        self.gat_heads = gat_heads
        if aggr == "gat":  # (likewise: only this configuration owns the two keys)
            if isinstance(gat_heads, bool) or int(gat_heads) != gat_heads:
                raise ValueError(f"GLASSConv: gat_heads must be an integer >= 1, not {gat_heads!r}")
            self.gat_heads = int(gat_heads)
            from .graph import CSRAdj
            CSRAdj.gat_head_width(out_channels, self.gat_heads)
            self.att_src = nn.Parameter(torch.empty(out_channels))
            self.att_dst = nn.Parameter(torch.empty(out_channels))
            _reset_gat_att(self)
        if aggr == "gatv2":  # (likewise: only this configuration owns the key)
            if isinstance(gat_heads, bool) or gat_heads != 1:
                raise ValueError(f"GLASSConv: aggr 'gatv2' has one attention head, not gat_heads={gat_heads!r}")
            self.att = nn.Parameter(torch.empty(out_channels))
            _reset_gatv2_att(self)

    def reset_parameters(self):
        for lin in list(self.trans_fns) + list(self.comb_fns):
            lin.reset_parameters()
        self.gn.reset_parameters()
        _reset_softmax_t(self)
        _reset_gat_att(self)
        _reset_gatv2_att(self)
        _reset_pna_weight(self)

    def forward(self, x_, edge_index, edge_weight, mask, out=None, batch=None):
        """`out` (optional, fused path only): a preallocated [N,H] view (a slice of the JK buffer) to write into.
        `batch`: an ops.Replicas when x_ holds R replicas of the graph's rows (replica-major, [R * N, H]) with one label byte
        per replica row: the aggregation and the GraphNorm then run per replica (ops.spmm_rep, ops.graphnorm_rep); the dense
        calls key only on the row's label byte and take the R * N rows as they are."""
        if self.live_edge_weight and batch is not None:
            raise ValueError("GLASSConv: live_edge_weight has no replicated form (exact zero-one labels: `batch` given)")
        if self.aggr in ("std", "var", "pna", "gatv2") and batch is not None:
            raise ValueError(f"GLASSConv: aggr {self.aggr!r} has no replicated form (exact zero-one labels: `batch` given)")
        p_edge = _check_edge_dropout(self.edge_dropout, self.aggr, self.live_edge_weight)  # (the attributes may have been set since)
        if p_edge > 0 and batch is not None:
            raise ValueError("GLASSConv: edge_dropout has no replicated form (exact zero-one labels: `batch` given)")
        if self.adj is None:
            self.adj = buildAdj(edge_index, edge_weight.detach() if self.live_edge_weight else edge_weight,
                                x_.shape[0] if batch is None else batch.N, self.aggr)
        if batch is not None and x_.shape[0] != batch.R * batch.N:
            raise ValueError(f"GLASSConv: {x_.shape[0]} rows for {batch!r}")
        if self.live_edge_weight:
            agg = lambda m: ops.spmm_w(self.adj, m, edge_weight)
        elif self.training and p_edge > 0:
            # (call_base + 0 and + 1 are the two GraphNorm streams of this layer)
            agg = lambda m: ops.spmm_dropedge(self.adj, m, p_edge, self.call_base + 2, self.edge_dropout_symmetric)
        elif batch is not None:
            agg = lambda m: ops.spmm_rep(self.adj, m, batch.R)
        elif self.aggr == "softmax":
            agg = lambda m: ops.spmm_softmax(self.adj, m, self.t)
        elif self.aggr == "gat":
            agg = lambda m: ops.spmm_gat(self.adj, m, self.att_src, self.att_dst, self.gat_slope, self.gat_heads)
        elif self.aggr == "gatv2":
            agg = lambda m: ops.spmm_gatv2(self.adj, m, self.att, self.gat_slope)
        elif self.aggr in ("std", "var"):
            agg = lambda m: ops.spmm_moments(self.adj, m, self.aggr, self.moment_eps)[0]
        elif self.aggr == "pna":
            agg = lambda m: ops.pna_mix(*ops.spmm_pna(self.adj, m, self.moment_eps), self.adj.pna_wsum, self.adj.pna_delta,
                                        self.pna_weight)
        else:
            agg = lambda m: ops.spmm(self.adj, m)
        rep = {} if batch is None else {"rep": batch}  # (a training pass collects the weight gradients replica by replica)
        if mask.dtype != torch.uint8:
            mask = mask.reshape(-1).to(torch.uint8)
        p = self.dropout if self.training else 0.0
        code = _act_code(self.activation)
        stack = getattr(self, "_stack", {})  # set by arena.ParamArena: stacked weight views
        H = x_.shape[1]
        if (code is not None and "trans" in stack and "comb" in stack and len(stack["trans"]) == 6 and
                self.trans_fns[0].weight.shape == (H, H) and ops.dual_linear_supported(H) and ops.USE_FUSED_DENSE):
            # fused dense path: Linear pair + ELU + mix in one MFMA kernel each; no cat, no [N,2H] round trips
            m = ops.dual_linear_mix(x_, None, self.trans_fns[1], self.trans_fns[0], mask, self.z_ratio, code,
                                    stack["trans"], **rep)
            a = agg(m)
            g = self.gn(a, batch=batch, p_drop=p, call_id=self.call_base)
            return ops.dual_linear_mix(g, x_, self.comb_fns[1], self.comb_fns[0], mask, self.z_ratio, ACT_NONE,
                                       stack["comb"], out, **rep)
        # both weight sets in one GEMM: T = [f1 | f0]
        T = ops.stacked_linear(x_, self.trans_fns[1], self.trans_fns[0], stack.get("trans"), **rep)
        if code is None:
            T = self.activation(T)
        m = ops.mix(T, mask, self.z_ratio, ACT_NONE if code is None else code)
        a = agg(m)
        g = self.gn(a, batch=batch, p_drop=p, call_id=self.call_base)
        c = torch.cat((g, x_), dim=-1)
        C = ops.stacked_linear(c, self.comb_fns[1], self.comb_fns[0], stack.get("comb"), **rep)
        return ops.mix(C, mask, self.z_ratio, ACT_NONE)


class EmbZGConv(nn.Module):
    """Embedding of the integer node feature + label mask, then `num_layers` GLASSConv layers
    with GraphNorm / activation / dropout between them and optional JK concatenation.  live_edge_weight: handed to every
    layer (GLASSConv: the aggregation reads the edge weights of each call and is differentiable in them)."""
    def __init__(self, hidden_channels, output_channels, num_layers, max_deg, dropout=0, activation=nn.ReLU(),
                 conv=GLASSConv, gn=True, jk=False, live_edge_weight=False, **kwargs):
        super().__init__()
        if live_edge_weight:
            kwargs["live_edge_weight"] = True
        self.input_emb = nn.Embedding(int(max_deg) + 1, hidden_channels, scale_grad_by_freq=False)
        self.emb_gn = GraphNorm(hidden_channels)
        self.convs = nn.ModuleList()
        self.jk = jk
        widths = [hidden_channels] * (num_layers - 1) + [output_channels]
        for l, w in enumerate(widths):
            layer = conv(in_channels=hidden_channels, out_channels=w, activation=activation, **kwargs)
            layer.call_base = 16 * (l + 1)
            self.convs.append(layer)
        self.activation = activation
        self.dropout = dropout
        self.replica_chunk = None  # exact zero-one labels (z [B, N]): replicas per group of launches; None = all B at once
        if gn:
            self.gns = nn.ModuleList([GraphNorm(hidden_channels) for _ in range(num_layers - 1)])
            self.gns.append(GraphNorm(output_channels + (num_layers - 1) * hidden_channels if jk else output_channels))
        else:
            self.gns = None
        self.reset_parameters()

    def reset_parameters(self):
        self.input_emb.reset_parameters()
        self.emb_gn.reset_parameters()
        for conv in self.convs:
            conv.reset_parameters()
        if self.gns is not None:
            for gn in self.gns:
                gn.reset_parameters()

    def _selection(self, x_flat):
        # x is static per dataset: the selection CSR is cached per feature tensor, keyed on the storage it views (the
        # tensor is kept alive in the entry so the pointer cannot be recycled underneath us).  SEVERAL entries are kept:
        # train / validation / test sets hold their own copies of x, and a captured training step (hipGraph) keeps
        # launching K1 with the raw pointers of ITS entry — evicting that entry when an evaluation comes by with another
        # x would leave the graph reading freed memory.
        key = (x_flat.data_ptr(), x_flat.shape[0], self.input_emb.weight.shape[0])
        cache = self.__dict__.setdefault("_sel_cache", {})
        hit = cache.get(key)
        if hit is None:
            if len(cache) >= 16:
                raise RuntimeError("EmbZGConv: more than 16 distinct node-feature tensors seen by one model; the selection "
                                   "cache keeps them alive for captured graphs — reuse the dataset tensors")
            hit = cache[key] = (x_flat, Selection(x_flat, key[2]))
        return hit[1]

    def forward(self, x, edge_index, edge_weight, z=None):
        n = x.shape[0]
        if x.numel() != n:
            raise NotImplementedError("one integer feature per node (x of shape [N,1])")
        x_flat = x.reshape(n)
        if x_flat.dtype != torch.int64:
            x_flat = x_flat.to(torch.int64)
        if not x_flat.is_contiguous():  # a channel slice of a [N, C, 1] feature tensor: the kernels read a dense int64[N]
            x_flat = x_flat.contiguous()
        if z is not None and z.dim() == 2 and z.shape[0] > 1 and z.shape[1] == n:
            # exact zero-one labels (utils.ZeroOneZ): row b of z marks subgraph b alone -> [B, N, C], one replica of the graph
            # per subgraph.  Always the per-op form (the stack program is one graph with one label vector).
            return self._forward_replicas(x_flat, z, edge_index, edge_weight)
        if z is not None:
            # reference: mask = (z > 0.5) for whatever z holds (impl/models.py:243-248); the kernels read int64
            if z.numel() != n:
                raise ValueError(f"z must hold one label per node ({n}), got {tuple(z.shape)}")
            z = z.reshape(n)
            if z.dtype != torch.int64:
                z = (z > 0.5).to(torch.int64)
            elif not z.is_contiguous():
                z = z.contiguous()
        if USE_STACK and stack.StackProgram.supported(self):
            # the whole stack as one autograd node (explicit forward / backward program, glass_amd/stack.py)
            return stack.run(self, x_flat, z, edge_index, edge_weight)
        p = self.dropout if self.training else 0.0
        if self.training and (p > 0 or any(c.dropout > 0 or getattr(c, "edge_dropout", 0.0) > 0 for c in self.convs)):
            ops.rng_advance(x.device)  # new dropout masks for this forward/backward pair
            # ... read from a private snapshot of the (seed, step) words by this forward's ops and by their backward, so
            # further training forwards may come before it (NodeEmb over several channels, gradient accumulation)
            with ops.rng_scope(x.device, ops.rng_snapshot(x.device) if torch.is_grad_enabled() else None):
                return self._forward_per_op(x_flat, z, edge_index, edge_weight, p)
        return self._forward_per_op(x_flat, z, edge_index, edge_weight, p)

    def _forward_replicas(self, x_flat, z, edge_index, edge_weight):
        """z [B, N] -> [B, N, C]: output row b is what z[b] alone gives on the whole graph (message passing, every GraphNorm
        statistic).  The replicas run in groups of at most `replica_chunk`.  They are independent, their dropout key carries
        the replica's index in the batch, and a training pass collects every parameter gradient replica by replica in an
        ops.RepSink that is summed once, in an order that depends on B alone — so neither logits nor gradients depend on the
        grouping, bit for bit.  (The dropout generator hashes the low 32 bits of the key: all replicas draw the same mask.)"""
        B, n = z.shape
        ops._need_gpu(x_flat, z, self.input_emb.weight)
        if z.dtype == torch.uint8:  # label bytes as ops.zeroone_labels makes them: taken as they are
            mask = z.contiguous()
        else:
            mask = (z > 0.5 if z.dtype != torch.int64 else z != 0).to(torch.uint8).contiguous()  # (impl/models.py:243-248: z > 0.5)
        chunk = B if self.replica_chunk is None else int(self.replica_chunk)
        if chunk < 1:
            raise ValueError(f"EmbZGConv.replica_chunk must be None or >= 1, got {self.replica_chunk!r}")
        p = self.dropout if self.training else 0.0
        draws = self.training and (p > 0 or any(c.dropout > 0 for c in self.convs))
        if draws:
            ops.rng_advance(x_flat.device)  # new dropout masks for this forward/backward pair (one advance for all groups)
        words = ops.rng_snapshot(x_flat.device) if (draws and torch.is_grad_enabled()) else None
        outs = []
        with ops.rng_scope(x_flat.device, words):
            # the embedding and its GraphNorm do not see the labels: once on N rows, then replicated.  (Every replica's
            # dropout mask of emb_gn is the one the plain call draws: the generator hashes the low 32 bits of the key.)
            h0, _m = ops.embed_label(self.input_emb.weight, x_flat, None, self._selection(x_flat))
            h0 = self.emb_gn(h0, p_drop=p, call_id=1)
            sink = None
            if torch.is_grad_enabled() and any(t.requires_grad for t in self.parameters()):
                sink = ops.RepSink(B, h0.device)
                h0 = ops.replica_root(h0, sink)
            for rep0 in range(0, B, chunk):
                rep = ops.Replicas(min(chunk, B - rep0), n, rep0, sink)
                m = mask[rep0:rep0 + rep.R].reshape(-1)
                if m.data_ptr() % 16:  # (a group that starts inside the batch: the dense kernels read the bytes in pairs)
                    m = m.clone()
                out = self._forward_per_op(x_flat, None, edge_index, edge_weight, p, rep=rep, h0=h0, mask=m)
                outs.append(out.view(rep.R, n, out.shape[1]))
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def _forward_per_op(self, x_flat, z, edge_index, edge_weight, p, rep=None, h0=None, mask=None):
        """rep (an ops.Replicas) with h0 (the embedded, normalised rows [N, H]) and mask (uint8 [R * N]): the replicated form."""
        n = x_flat.shape[0]
        arena = getattr(self, "_glass_arena", None)
        if arena is not None:
            arena.refresh_transposes()  # operand images (W, W^T) of the fused dense kernels follow the weights
        code = _act_code(self.activation)
        if rep is None:
            h, mask = ops.embed_label(self.input_emb.weight, x_flat, z, self._selection(x_flat))
            h = self.emb_gn(h, p_drop=p, call_id=1)
        else:
            n = rep.R * rep.N
            h = ops.replicate_rows(h0, rep)
        extra = {} if rep is None else {"batch": rep}
        xs = []
        # JK buffer written in place by the fused layers (no torch.cat) when every layer takes that path
        widths = [c.trans_fns[0].weight.shape[0] for c in self.convs if isinstance(c, GLASSConv)]
        jk_buf = None
        if (self.jk and len(widths) == len(self.convs) and len(set(widths)) == 1 and widths[0] == h.shape[1] and
                code is not None and all("comb" in getattr(c, "_stack", {}) and len(c._stack["comb"]) == 6
                                         for c in self.convs) and ops.dual_linear_supported(h.shape[1]) and
                ops.USE_FUSED_DENSE):
            jk_buf = torch.empty((n, sum(widths)), dtype=torch.float32, device=h.device)
        for layer, conv in enumerate(self.convs):
            if jk_buf is not None:
                h = conv(h, edge_index, edge_weight, mask, out=jk_buf[:, layer * widths[0]:(layer + 1) * widths[0]], **extra)
            else:
                h = conv(h, edge_index, edge_weight, mask, **extra)
            xs.append(h)
            if layer + 1 == len(self.convs):
                break
            if self.gns is not None:
                if code is not None:
                    h = self.gns[layer](h, act=code, p_drop=p, call_id=conv.call_base + 1, **extra)
                    continue
                h = self.gns[layer](h, **extra)
            h = self.activation(h)
            h = F.dropout(h, p=self.dropout, training=self.training)
        if jk_buf is not None:
            h = ops.join_cols(jk_buf, xs)
        else:
            h = torch.cat(xs, dim=-1) if self.jk else xs[-1]
        if self.gns is not None:
            h = self.gns[-1](h, **extra)
        return h


# ---------------------------------------------------------------------------------------------
class PoolModule(nn.Module):
    """Subgraph readout.  `forward(x, batch)` keeps the reference's gathered-rows + batch-vector
    calling convention; GLASS.Pool uses the fused padded-matrix kernel directly."""
    mode = None

    def __init__(self, pool_fn=None, trans_fn=None):
        super().__init__()
        self.pool_fn = pool_fn
        self.trans_fn = trans_fn

    def forward(self, x, batch):
        if self.trans_fn is not None:
            x = self.trans_fn(x)
        return ops.segment_pool(x, batch2pad(batch), self.mode)


class AddPool(PoolModule):
    mode = "sum"

    def __init__(self, trans_fn=None):
        super().__init__(None, trans_fn)


class MaxPool(PoolModule):
    mode = "max"

    def __init__(self, trans_fn=None):
        super().__init__(None, trans_fn)


class MeanPool(PoolModule):
    mode = "mean"

    def __init__(self, trans_fn=None):
        super().__init__(None, trans_fn)


class SizePool(AddPool):
    mode = "size"


class AttnPool(PoolModule):
    """Attention readout (an extension: the reference has no learned pool): out[b] = sum_j alpha[b, j] * x_j with alpha the
    softmax over the subgraph's nodes of gate(x_j) (ops.attn_pool, csrc/pool_attn.hip).  The gate has no bias — it would
    cancel in the softmax — and starts at ZERO: the pool is then exactly mean pooling."""
    mode = "attn"

    def __init__(self, in_channels, trans_fn=None):
        super().__init__(None, trans_fn)
        self.gate = nn.Linear(in_channels, 1, bias=False)
        nn.init.zeros_(self.gate.weight)

    def forward(self, x, batch):
        if self.trans_fn is not None:
            x = self.trans_fn(x)
        return ops.attn_pool(x, batch2pad(batch), self.gate.weight)


class GLASS(nn.Module):
    """EmbZGConv + per-target pooling and prediction heads (`preds[id]`, `pools[id]`).  live_edge_weight=True switches every
    layer of `conv` to live edge weights (GLASSConv; ValueError for an aggregation that has none)."""
    def __init__(self, conv: EmbZGConv, preds: nn.ModuleList, pools: nn.ModuleList, live_edge_weight=False):
        super().__init__()
        if live_edge_weight:
            set_live_edge_weight(conv)
        self.conv = conv
        self.preds = preds
        self.pools = pools

    def __deepcopy__(self, memo):
        """copy.deepcopy(model) (an early-stopping snapshot, a twin): a PLAIN copy — own parameter storage, no arena, no captured
        graphs, no adopted optimizer (arena.strip_runtime); it gets its own runtime objects the first time it trains."""
        from .arena import deepcopy_plain
        return deepcopy_plain(self, memo)

    def _channels(self, x):
        """The feature channels of x [N, C, F] as dense tensors, made once per feature tensor: x is static per dataset, and
        the conv caches its selection CSR (and captured graphs hold its pointers) by the tensor it is handed."""
        if x.shape[1] == 1:
            return [x.reshape(x.shape[0], x.shape[-1])]
        cache = self.__dict__.setdefault("_chan_cache", {})
        key = (x.data_ptr(), tuple(x.shape), x._version)
        hit = cache.get(key)
        if hit is None:
            if len(cache) >= 8:
                cache.clear()
            hit = cache[key] = (x, [x[:, c, :].contiguous() for c in range(x.shape[1])])
        return hit[1]

    def NodeEmb(self, x, edge_index, edge_weight, z=None):
        embs = [self.conv(xc, edge_index, edge_weight, z) for xc in self._channels(x)]
        if len(embs) == 1:
            return embs[0]  # mean over a single feature channel is the identity
        return torch.stack(embs, dim=1).mean(dim=1)

    def Pool(self, emb, subG_node, pool):
        if emb.dim() == 3:
            # exact zero-one labels: emb [B, N, C] holds one replica of the graph per subgraph; row b of subG_node pools from
            # replica b only — the existing pools on the flattened matrix, the valid entries moved to their replica's rows
            B, N, C = emb.shape
            if subG_node.shape[0] != B:
                raise ValueError(f"Pool: {subG_node.shape[0]} subgraphs for {B} replicas")
            shift = torch.arange(B, dtype=subG_node.dtype, device=subG_node.device).unsqueeze(1) * N
            valid = (subG_node >= 0) & (subG_node < N)
            return self.Pool(emb.reshape(B * N, C), torch.where(valid, subG_node + shift, torch.full_like(subG_node, -1)), pool)
        if isinstance(pool, AttnPool) and pool.trans_fn is None:
            return ops.attn_pool(emb, subG_node, pool.gate.weight)
        if isinstance(pool, PoolModule) and pool.trans_fn is None and pool.mode is not None:
            return ops.segment_pool(emb, subG_node, pool.mode)
        from .utils import pad2batch
        batch, pos = pad2batch(subG_node)
        return pool(emb[pos], batch)

    def forward(self, x, edge_index, edge_weight, subG_node, z=None, id=0):
        emb = self.NodeEmb(x, edge_index, edge_weight, z)
        emb = self.Pool(emb, subG_node, self.pools[id])
        return _head(self.preds[id], emb)


def _head(pred, emb):
    """The prediction head.  Under no_grad (evaluation: train.test) a bare nn.Linear runs as one small kernel of this
    library (glass_head_linear_f32) instead of a library GEMM, and a two-layer MLP in eval mode (losses.fusable_head:
    "mlp2", the GNN-seg / GNNEmb head) as one launch of glass_head_mlp_f32 instead of module by module; anything else is
    the module itself."""
    if (torch.is_grad_enabled() or not emb.is_cuda or emb.dim() != 2 or emb.dtype != torch.float32):
        return pred(emb)
    from . import _lib
    stream = torch.cuda.current_stream().cuda_stream
    if type(pred) is nn.Linear and pred.weight.dtype == torch.float32:
        emb = emb if emb.stride(1) == 1 else emb.contiguous()
        w = pred.weight if pred.weight.is_contiguous() else pred.weight.contiguous()
        out = torch.empty((emb.shape[0], w.shape[0]), dtype=torch.float32, device=emb.device)
        rc = _lib.load().glass_head_linear_f32(emb.data_ptr(), emb.stride(0), w.data_ptr(),
                                               0 if pred.bias is None else pred.bias.data_ptr(), emb.shape[0], emb.shape[1],
                                               w.shape[0], out.data_ptr(), out.stride(0), stream)
        _lib.check(rc, "glass_head_linear_f32")
        return out
    if type(pred) is MLP and not pred.training and emb.shape[0] > 0:
        from . import losses
        parts = losses._mlp2_parts(pred)
        if parts is not None and parts[0].weight.dtype == torch.float32 and parts[0].weight.shape[1] == emb.shape[1]:
            lin1, _p, act, lin2 = parts
            emb, ldp = ops._rows(emb)
            w1, b1, w2, b2 = (t.contiguous() for t in (lin1.weight, lin1.bias, lin2.weight, lin2.bias))
            out = torch.empty((emb.shape[0], w2.shape[0]), dtype=torch.float32, device=emb.device)
            rc = _lib.load().glass_head_mlp_f32(emb.data_ptr(), ldp, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                                act, emb.shape[0], emb.shape[1], w1.shape[0], w2.shape[0], out.data_ptr(),
                                                out.stride(0), stream)
            if rc != -3:  # (GLASS_E_UNSUPPORTED — sizes over the kernel's limits — runs the modules)
                _lib.check(rc, "glass_head_mlp_f32")
                return out
    return pred(emb)


# ---------------------------------------------------------------------------------------------
# SSL pre-training models (link prediction) — reference impl/models.py:361-509.  Same kernels:
# K1 for the aggregation, K6 GraphNorm, K3 embedding gather (+ K1 backward), K7 for the pair readout.
# ---------------------------------------------------------------------------------------------
class MyGCNConv(nn.Module):
    """Unlabeled message-passing layer: comb_fn([GraphNorm(adj @ act(trans_fn(x_))) || x_])."""
    def __init__(self, in_channels: int, out_channels: int, activation=nn.ReLU(inplace=True), aggr="mean", softmax_t=1.0):
        super().__init__()
        self.trans_fn = Linear(in_channels, out_channels)
        self.comb_fn = Linear(in_channels + out_channels, out_channels)
        self.adj = None
        self.activation = activation
        self.aggr = aggr
        self.gn = GraphNorm(out_channels)
        self.softmax_t = float(softmax_t)
        if aggr == "softmax":
            self.t = nn.Parameter(torch.full((1, ), self.softmax_t))

    def reset_parameters(self):
        self.trans_fn.reset_parameters()
        self.comb_fn.reset_parameters()
        self.gn.reset_parameters()
        _reset_softmax_t(self)

    def forward(self, x_, edge_index, edge_weight):
        if self.adj is None:
            self.adj = buildAdj(edge_index, edge_weight, x_.shape[0], self.aggr)
        x = self.activation(self.trans_fn(x_))
        x = self.gn(ops.spmm_softmax(self.adj, x, self.t) if self.aggr == "softmax" else ops.spmm(self.adj, x))
        return self.comb_fn(torch.cat((x, x_), dim=-1))


class EmbGConv(nn.Module):
    """Embedding + `num_layers` unlabeled conv layers (GraphNorm / activation / dropout between them)."""
    def __init__(self, input_channels: int, hidden_channels: int, output_channels: int, num_layers: int, max_deg: int,
                 dropout=0, activation=nn.ReLU(inplace=True), conv=MyGCNConv, gn=True, jk=False, **kwargs):
        super().__init__()
        self.input_emb = nn.Embedding(int(max_deg) + 1, hidden_channels)
        self.jk = jk
        dims = [input_channels] + [hidden_channels] * (num_layers - 1) + [output_channels]
        self.convs = nn.ModuleList([conv(in_channels=dims[i], out_channels=dims[i + 1], **kwargs)
                                    for i in range(num_layers)])
        for l, layer in enumerate(self.convs):
            layer.call_base = 16 * (l + 1)  # dropout streams of the step program (stack.StackProgram, unlabeled mode)
        self.activation = activation
        self.dropout = dropout
        self.gns = nn.ModuleList([GraphNorm(hidden_channels) for _ in range(num_layers - 1)]) if gn else None
        self.reset_parameters()

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()
        if self.gns is not None:
            for gn in self.gns:
                gn.reset_parameters()

    _selection = EmbZGConv._selection

    def forward(self, x, edge_index, edge_weight, z=None):
        x_flat = x.reshape(-1)
        if x_flat.dtype != torch.int64:
            x_flat = x_flat.to(torch.int64)
        if USE_STACK and z is None and stack.StackProgram.supported(self):
            # the whole stack as one autograd node on the fused kernels (glass_amd/stack.py, unlabeled mode)
            if not x_flat.is_contiguous():
                x_flat = x_flat.contiguous()
            return stack.run(self, x_flat, None, edge_index, edge_weight)
        h, _mask = ops.embed_label(self.input_emb.weight, x_flat, None, self._selection(x_flat))
        h = F.dropout(h, p=self.dropout, training=self.training)
        # The reference appends the GraphNorm output and then applies the activation to that very tensor; with
        # the driver's nn.ReLU(inplace=True) (GNNEmb.py:90) the appended tensor is therefore the ACTIVATED one.
        inplace = bool(getattr(self.activation, "inplace", False))
        xs = []
        for layer, conv in enumerate(self.convs[:-1]):
            h = conv(h, edge_index, edge_weight)
            if self.gns is not None:
                h = self.gns[layer](h)
            pre = h
            h = self.activation(h)
            xs.append(h if inplace else pre)
            h = F.dropout(h, p=self.dropout, training=self.training)
        xs.append(self.convs[-1](h, edge_index, edge_weight))
        return torch.cat(xs, dim=-1) if self.jk else xs[-1]


class EdgeGNN(nn.Module):
    """Link-prediction wrapper: node embeddings -> mean over each node pair -> preds[id]."""
    def __init__(self, conv, preds: nn.ModuleList, pools: nn.ModuleList):
        super().__init__()
        self.conv = conv
        self.preds = preds
        self.pools = pools

    NodeEmb, _channels, __deepcopy__ = GLASS.NodeEmb, GLASS._channels, GLASS.__deepcopy__

    def Pool(self, emb, subG_node, pool):
        return ops.segment_pool(emb, subG_node, "mean")  # emb[subG_node].mean(dim=1); pairs carry no padding

    def forward(self, x, edge_index, edge_weight, subG_node, z=None, id=0):
        emb = self.NodeEmb(x, edge_index, edge_weight, z)
        emb = self.Pool(emb, subG_node, self.pools[id])
        return self.preds[id](emb)
