"""torch.autograd bindings of the HIP kernels (host side of the C ABI in include/glass_hip.h).

Every op here enqueues hand-written gfx950 kernels on torch's current HIP stream through ctypes;
torch only supplies device memory, streams and the autograd tape.  There is no CPU path: a CPU
tensor raises GlassHipError (the CPU restatement lives in oracle/ and is a checker only).
"""
import os

import torch

from . import _lib
from ._lib import ACT_NONE, ACT_ELU, ACT_RELU, POOL_MODES, GlassHipError


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise GlassHipError(f"glass_amd op got a {t.device} tensor: the HIP path is the only path (no CPU fallback)")


def _rows(t):
    """Row-major 2-D fp32 view -> (tensor, leading dimension)."""
    if t.dim() != 2 or t.dtype != torch.float32:
        raise GlassHipError(f"expected a 2-D float32 tensor, got {tuple(t.shape)} {t.dtype}")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0)))


# ---------------------------------------------------------------------------------------------
# dropout RNG state: uint64[2] = (seed, step) in DEVICE memory, so captured graphs get fresh masks
# ---------------------------------------------------------------------------------------------
_rng = {}


def _dev(device):
    """One key per device however it is spelled ("cuda:0", torch.device("cuda", 0), torch.device("cuda"))."""
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def rng_state(device):
    device = _dev(device)
    st = _rng.get(device)
    if st is None:
        st = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=device)
        _rng[device] = st
    return st


def rng_seed(seed, device):
    """(Re)seed the dropout stream IN PLACE: captured graphs keep reading the same device words."""
    device = _dev(device)
    st = _rng.get(device)
    new = torch.tensor([int(seed) & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64)
    if st is None:
        _rng[device] = new.to(device)
    else:
        st.copy_(new)


# Host-side count of advances of the device-resident stream.  The backward of a dropout regenerates the forward's
# mask from the LIVE (seed, step) words, so a second training forward (which advances them) between a forward and its
# backward would silently pair the gradient with the wrong mask (gradient accumulation, GLASS.NodeEmb over several
# feature channels, two model calls before loss.backward()).  Every autograd node that drew a mask remembers the
# epoch of its forward and refuses to run its backward under another one.  (Replays of a captured step do not touch
# the host counter; there forward and backward sit in the same graph.)
_rng_epoch = {}


def note_rng_advance(device):
    device = _dev(device)
    _rng_epoch[device] = _rng_epoch.get(device, 0) + 1


def rng_epoch(device):
    return _rng_epoch.get(_dev(device), 0)


def check_rng_epoch(device, epoch, what):
    if epoch != rng_epoch(device):
        raise RuntimeError(f"{what}: the dropout stream was advanced by another training forward between this "
                           "forward and its backward; its mask can no longer be regenerated (run backward() before "
                           "the next training forward, or use dropout 0)")


# ---- the dropout words of the CURRENT pass -------------------------------------------------------------------------
# A training forward on the autograd paths takes a private 16-byte snapshot of (seed, step) right after advancing the
# stream; every kernel of that forward AND of its backward reads the snapshot, so any number of training forwards may lie
# between a forward and its backward (GLASS.NodeEmb over several feature channels, reference impl/models.py:336-344;
# gradient accumulation; two model calls before loss.backward()).  The tape-free step program (stack.loss_and_grads)
# runs forward and backward back to back and reads the live words — no copy launch in the replayed step.
_rng_cur = {}


def rng_tensor(device):
    """The (seed, step) words the kernels launched NOW read: the current pass's snapshot, else the live stream."""
    t = _rng_cur.get(_dev(device))
    return t if t is not None else rng_state(device)


def rng_snapshot(device):
    """A private copy of the live words (one small device copy; a captured graph replays it with the step)."""
    return rng_state(device).clone()


class rng_scope:
    """`with rng_scope(device, words):` — the kernels launched inside read `words` (None: the live stream)."""
    def __init__(self, device, words):
        self.device, self.words = _dev(device), words

    def __enter__(self):
        self.prev = _rng_cur.get(self.device)
        _rng_cur[self.device] = self.words
        return self.words

    def __exit__(self, *exc):
        _rng_cur[self.device] = self.prev
        return False


def rng_advance(device):
    _lib.check(_lib.load().glass_rng_advance(rng_state(device).data_ptr(), _stream()), "glass_rng_advance")
    note_rng_advance(device)


# ---------------------------------------------------------------------------------------------
# K4  MaxZOZ
# ---------------------------------------------------------------------------------------------
def maxzoz(n_nodes, pos):
    """z[n] = 1 iff n occurs in pos (int64, -1 = padding).  reference impl/utils.py:32-45"""
    _need_gpu(pos)
    pos = pos.contiguous()
    if pos.dtype != torch.int64:
        pos = pos.to(torch.int64)
    z = torch.empty(n_nodes, dtype=torch.int64, device=pos.device)
    _lib.check(_lib.load().glass_maxzoz_i64(pos.data_ptr(), pos.numel(), z.data_ptr(), n_nodes, _stream()),
               "glass_maxzoz_i64")
    return z


# ---------------------------------------------------------------------------------------------
# K1  aggregation
# ---------------------------------------------------------------------------------------------
# aggr -> (why ops.spmm and ops.spmm_rep do not serve it, the call that does).  "max" is not here: ops.spmm serves it.
_OWN_CALL = {
    "softmax": ("has no temperature of its own", "ops.spmm_softmax(adj, x, t)"),
    "gat": ("has no attention vectors of its own", "ops.spmm_gat(adj, x, att_src, att_dst, slope)"),
    "gatv2": ("has no attention vector of its own", "ops.spmm_gatv2(adj, x, att, slope)"),
    "std": ("is no product", "ops.spmm_moments(adj, x, kind, eps)"),
    "var": ("is no product", "ops.spmm_moments(adj, x, kind, eps)"),
    "pna": ("is no product", "ops.spmm_pna(adj, x, eps)"),
}


def _need_aggr(adj, what, *aggrs):
    """ops.`what` serves the adjacencies built for `aggrs`, and no other"""
    aggr = getattr(adj, "aggr", None)
    if aggr not in aggrs:
        raise GlassHipError(f"{what}: the adjacency was built for aggr {aggr!r}, not " + " or ".join(repr(a) for a in aggrs))


def _need_weighted(adj, what, thing):
    """`thing` exists for the aggregations that are products with K2's values only"""
    aggr = getattr(adj, "aggr", None)
    if aggr not in _lib.AGGR_MODES:
        raise GlassHipError(f"{what}: no {thing} for aggr {aggr!r} (only 'sum', 'mean', 'gcn')")


class SpMMFn(torch.autograd.Function):
    """y = A @ x with A a graph.CSRAdj; backward dx = A^T @ dy (A carries no gradient:
    edge weights never require grad in the reference, datasets.py:126,226)."""
    @staticmethod
    def forward(ctx, adj, x):
        _need_gpu(x)
        x, _ = _rows(x)
        ctx.adj = adj
        return adj.fwd.spmm(x)

    @staticmethod
    def backward(ctx, dy):
        dy, _ = _rows(dy)
        return None, ctx.adj.bwd.spmm(dy)


class SpMMMaxFn(torch.autograd.Function):
    """y[i] = max over the entries of row i of A of val * x[col] (aggr "max", K1m: csrc/spmm_max.hip); the forward keeps
    the winning entry of every output element, the backward routes dy through it (A carries no gradient)."""
    @staticmethod
    def forward(ctx, adj, x):
        _need_gpu(x)
        x, _ = _rows(x)
        y, arg = adj.max_fwd(x)
        ctx.adj = adj
        ctx.save_for_backward(arg)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy, _ = _rows(dy)
        (arg, ) = ctx.saved_tensors
        return None, ctx.adj.max_bwd(dy, arg)


class SpMMSoftmaxFn(torch.autograd.Function):
    """y[i] = softmax-weighted mean of the messages val, x[col] over the entries of row i of A at temperature t (aggr "softmax",
    K1s: csrc/spmm_softmax.hip).  The node keeps x, y and the log-sum-exp; the backward launches the dX pass and the dt pass
    only for the input that needs a gradient (A carries none)."""
    @staticmethod
    def forward(ctx, adj, x, t):
        _need_gpu(x)
        x, _ = _rows(x)
        y, lse = adj.softmax_fwd(x, t)
        ctx.adj = adj
        ctx.save_for_backward(x, y, lse, t)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy, _ = _rows(dy)
        x, y, lse, t = ctx.saved_tensors
        dx = ctx.adj.softmax_bwd(dy, x, y, lse, t) if ctx.needs_input_grad[1] else None
        dt = ctx.adj.softmax_dt(dy, x, y, lse, t).view_as(t) if ctx.needs_input_grad[2] else None
        return None, dx, dt


def spmm_softmax(adj, x, t):
    """Softmax neighbour aggregation: `adj` a graph.CSRAdj built for aggr "softmax", t one fp32 on the device (a parameter, or
    any tensor of one element)."""
    _need_aggr(adj, "spmm_softmax", "softmax")
    return SpMMSoftmaxFn.apply(adj, x, t)


class SpMMMomentFn(torch.autograd.Function):
    """(s, mu) = the weighted standard deviation (or variance) and mean of the messages x[col] over the entries of row i of A
    (aggr "std" / "var", K1v: csrc/spmm_moment.hip).  The node keeps x, s, mu and the rows' weight sums; the backward is one
    transposed pass, which reads the mean's factor only when mu's gradient was asked for (A carries no gradient)."""
    @staticmethod
    def forward(ctx, adj, x, kind, eps):
        _need_gpu(x)
        x, _ = _rows(x)
        s, mu, wsum = adj.moment_fwd(x, kind, eps)
        ctx.adj, ctx.kind = adj, kind
        ctx.save_for_backward(x, s, mu, wsum)
        ctx.set_materialize_grads(False)  # a result nobody used arrives as None, not as zeros: C is then not formed
        return s, mu

    @staticmethod
    def backward(ctx, ds, dmu):
        if not ctx.needs_input_grad[1] or (ds is None and dmu is None):
            return None, None, None, None
        x, s, mu, wsum = ctx.saved_tensors
        A, C = moment_factors(ctx.kind, s, wsum, ds, dmu)
        return None, ctx.adj.moment_bwd(x, mu, A, C), None, None


def _live_quotients(s, wsum):
    """(w, q) for K1v's and K1p's factors: w = W as a column, q(g, den) = where(W > 0, g / den, 0) — a row without entries
    (W = 0, and den with it) gives 0, not 0 / 0"""
    w = wsum[:, None]
    live = w > 0
    one = torch.ones((), dtype=s.dtype, device=s.device)

    def q(g, den):
        g, _ = _rows(g)
        return torch.where(live, g / torch.where(live, den, one), torch.zeros_like(g)).contiguous()
    return w, q


def moment_factors(kind, s, wsum, ds, dmu=None):
    """(A, C) of K1v's backward from the forward's results and the gradients of S and Mu (either may be None) — per destination,
    N * H work: std: A = dS / (W S); var: A = 2 dS / W; C = dMu / W (None without dMu); a row without entries gives 0."""
    w, q = _live_quotients(s, wsum)
    A = torch.zeros_like(s) if ds is None else q(ds, w * s if kind == "std" else (0.5 * w).expand_as(s))
    return A, (None if dmu is None else q(dmu, w))


def spmm_moments(adj, x, kind="std", eps=1e-5):
    """Spread of the neighbour messages: `adj` a graph.CSRAdj built for aggr "std" or "var".  Returns (S, Mu): per destination
    and channel the weighted standard deviation sqrt(Var + eps) (kind "std") or the weighted variance (kind "var"), and the
    weighted mean; zeros for a node without in-edges.  Differentiable in x through both results; under no_grad, or when x needs
    no gradient, nothing of the backward is launched."""
    _need_aggr(adj, "spmm_moments", "std", "var")
    if kind not in ("std", "var"):
        raise ValueError(f"spmm_moments: kind must be 'std' or 'var', not {kind!r}")
    return SpMMMomentFn.apply(adj, x, kind, float(eps))


class SpMMPnaFn(torch.autograd.Function):
    """(mu, mx, mn, s) = the weighted mean, the largest and the smallest, and the weighted standard deviation of the messages
    x[col] over the entries of row i of A (aggr "pna", K1p: csrc/spmm_pna.hip), from one gather of every source row.  The node
    keeps x, mu, s, the winning entries of both extremes and the rows' weight sums; the backward is one transposed pass for all
    four results (A carries no gradient)."""
    @staticmethod
    def forward(ctx, adj, x, eps):
        _need_gpu(x)
        x, _ = _rows(x)
        mu, s, mx, mn, amx, amn, wsum = adj.pna_fwd(x, eps)
        ctx.adj = adj
        ctx.save_for_backward(x, mu, s, amx, amn, wsum)
        ctx.set_materialize_grads(False)  # a result nobody used arrives as None, not as zeros
        return mu, mx, mn, s

    @staticmethod
    def backward(ctx, dmu, dmx, dmn, ds):
        if not ctx.needs_input_grad[1] or (dmu is None and dmx is None and dmn is None and ds is None):
            return None, None, None
        x, mu, s, amx, amn, wsum = ctx.saved_tensors
        A, C = pna_factors(s, wsum, ds, dmu)
        zero = None
        rows = []
        for g in (dmx, dmn):  # the kernel has one form: a result without a gradient hands it zeros
            if g is None:
                g = zero = torch.zeros_like(s) if zero is None else zero
            else:
                g, _ = _rows(g)
            rows.append(g)
        return None, ctx.adj.pna_bwd(x, mu, A, C, amx, rows[0], amn, rows[1]), None


def pna_factors(s, wsum, ds, dmu):
    """(A, C) of K1p's backward from the forward's results and the gradients of S and Mu (either may be None: zeros) — per
    destination, N * H work: A = dS / (W S), C = dMu / W; a row without entries gives 0."""
    w, q = _live_quotients(s, wsum)
    A, C = (torch.zeros_like(s) if g is None else q(g, den) for g, den in ((ds, w * s), (dmu, w.expand_as(s))))
    return A, C


def spmm_pna(adj, x, eps=1e-5):
    """PNA's four aggregators from one pass: `adj` a graph.CSRAdj built for aggr "pna".  Returns (Mu, Mx, Mn, S): per destination
    and channel the weighted mean, the largest and the smallest neighbour message, and the weighted standard deviation
    sqrt(Var + eps); zeros for a node without in-edges.  Differentiable in x through all four; under no_grad, when x needs no
    gradient, or when no result received one, nothing of the backward is launched."""
    _need_aggr(adj, "spmm_pna", "pna")
    return SpMMPnaFn.apply(adj, x, float(eps))


def pna_mix(mu, mx, mn, s, wsum, delta, theta):
    """PNA's degree scalers and a per-channel choice among the twelve views, plain differentiable torch:
    Y[i, c] = sum over aggregators a (mean, max, min, std) and scalers k of s_k(i) * theta[3 a + k, c] * Agg_a[i, c] with
    s_0 = 1, s_1 = log(W_i + 1) / delta (amplification), s_2 = delta / log(W_i + 1) (attenuation); wsum [N] the rows' weight
    sums, delta a float (graph.CSRAdj.pna_delta), theta [12, H].  A row with W = 0 gives 0."""
    live = wsum > 0
    lw = torch.log1p(torch.where(live, wsum, torch.ones_like(wsum)))
    zero = torch.zeros_like(wsum)
    scal = (live.to(mu.dtype)[:, None], torch.where(live, lw / delta, zero)[:, None], torch.where(live, delta / lw, zero)[:, None])
    y = None
    for a, agg in enumerate((mu, mx, mn, s)):
        coef = scal[0] * theta[3 * a] + scal[1] * theta[3 * a + 1] + scal[2] * theta[3 * a + 2]
        y = agg * coef if y is None else y + agg * coef
    return y


def _heads_kw(heads):
    """heads == 1 calls the CSRAdj methods exactly as before the argument existed"""
    return {} if heads == 1 else {"heads": heads}


class SpMMGatFn(torch.autograd.Function):
    """y[i] = attention-weighted mean of the messages x[col] over the entries of row i of A (aggr "gat", K1a:
    csrc/spmm_gat.hip): the weights are the softmax, times the edge weights, of LeakyReLU(x[col] . att_src + x[i] . att_dst).
    heads = K > 1 (csrc/spmm_gat_mh.hip): K heads partition the channels, head h owns columns [h D, (h + 1) D) of x, y and the
    two vectors, D = H / K, and has its own softmax; the scores and the log-sum-exp are then [N, K].  The node keeps x, y, the
    log-sum-exp and the two node scores; the backward runs the edge pass, then the transposed pass only when x needs a
    gradient and the two column reductions only when an attention vector does (A carries none)."""
    @staticmethod
    def forward(ctx, adj, x, att_src, att_dst, slope, heads):
        _need_gpu(x)
        x, _ = _rows(x)
        heads = int(heads)
        a, b = adj.gat_scores(x, att_src, att_dst, **_heads_kw(heads))
        y, lse = adj.gat_fwd(x, a, b, slope, **_heads_kw(heads))
        ctx.adj, ctx.slope, ctx.heads = adj, float(slope), heads
        ctx.save_for_backward(x, y, lse, a, b, att_src, att_dst)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy, _ = _rows(dy)
        x, y, lse, a, b, att_src, att_dst = ctx.saved_tensors
        adj = ctx.adj
        need_x, need_att = ctx.needs_input_grad[1], ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        if not (need_x or need_att):
            return None, None, None, None, None, None
        kw = _heads_kw(ctx.heads)
        g, db = adj.gat_edge(dy, x, y, lse, a, b, ctx.slope, **kw)
        dx = da = ds = dd = None
        if need_x:
            dx, da = adj.gat_bwd(dy, lse, a, b, g, db, att_src, att_dst, ctx.slope, **kw)
        if need_att:
            if da is None:  # the transposed pass's walk for da alone: the same bits, no rows read
                da = adj.gat_da(g, dy, **kw)
            ds, dd = adj.gat_datt(x, da, db, **kw)
            ds = ds if ctx.needs_input_grad[2] else None
            dd = dd if ctx.needs_input_grad[3] else None
        return None, dx, ds, dd, None, None


def spmm_gat(adj, x, att_src, att_dst, slope=0.2, heads=1):
    """Attention neighbour aggregation (GAT): `adj` a graph.CSRAdj built for aggr "gat", att_src / att_dst two fp32 vectors of
    x's width on the device (parameters, or any tensors), slope LeakyReLU's negative slope.  heads = K: K heads partition the
    channels (head h: columns [h D, (h + 1) D), D = width / K, of x, the result and both vectors), each with its own softmax;
    K must divide the width and D be a power of two in [4, 256] (ValueError otherwise, before any launch).  heads = 1 is
    single-head attention at any width."""
    _need_aggr(adj, "spmm_gat", "gat")
    if heads != 1:
        from .graph import CSRAdj
        if int(heads) != heads:
            raise ValueError(f"spmm_gat: heads must be an integer >= 1, not {heads!r}")
        CSRAdj.gat_head_width(x.shape[-1], int(heads))
    return SpMMGatFn.apply(adj, x, att_src, att_dst, slope, int(heads))


class SpMMGatV2Fn(torch.autograd.Function):
    """y[i] = attention-weighted mean of the messages x[col] over the entries of row i of A (aggr "gatv2", K1a2:
    csrc/spmm_gatv2.hip): the weights are the softmax, times the edge weights, of att . LeakyReLU(x[i] + x[col]) — dynamic
    attention, the non-linearity before the dot.  The node keeps x, y, the log-sum-exp and the entries' scores; the backward
    always runs the edge pass, then the transposed pass only when x needs a gradient and the column reduction only when att
    does (A carries none)."""
    @staticmethod
    def forward(ctx, adj, x, att, slope):
        _need_gpu(x)
        x, _ = _rows(x)
        s = adj.gatv2_score(x, att, slope)
        y, lse = adj.gatv2_fwd(x, s)
        ctx.adj, ctx.slope = adj, float(slope)
        ctx.save_for_backward(x, y, lse, s, att)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy, _ = _rows(dy)
        x, y, lse, s, att = ctx.saved_tensors
        adj = ctx.adj
        need_x, need_att = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if not (need_x or need_att):
            return None, None, None, None
        g, p, gd, r = adj.gatv2_edge(dy, x, y, lse, s, att, ctx.slope)
        dx = adj.gatv2_bwd(dy, x, p, g, gd, att, ctx.slope) if need_x else None
        datt = adj.gatv2_datt(r) if need_att else None
        return None, dx, datt, None


def spmm_gatv2(adj, x, att, slope=0.2):
    """Dynamic attention neighbour aggregation (GATv2, one head): `adj` a graph.CSRAdj built for aggr "gatv2", att one fp32
    vector of x's width on the device (a parameter, or any tensor), slope LeakyReLU's negative slope."""
    _need_aggr(adj, "spmm_gatv2", "gatv2")
    return SpMMGatV2Fn.apply(adj, x, att, slope)


class SpMMWFn(torch.autograd.Function):
    """y = A(w) @ x with the values of A a function of the edge weights w (K2's normalisation of aggr "sum" / "mean" / "gcn",
    CSRAdj.values_of) on the structure of a graph.CSRAdj; backward dx = A(w)^T @ dy on K1 and dw by K1w (csrc/spmm_edge.hip:
    the sampled dense-dense product, for "gcn" the column sums, then K2's backward, in the caller's edge order).  Each side
    runs only when its input needs a gradient."""
    @staticmethod
    def forward(ctx, adj, x, w):
        _need_gpu(x)
        x, _ = _rows(x)
        val, val_t, deg = adj.values_of(w)
        ctx.adj = adj
        ctx.save_for_backward(x, val, val_t, deg)
        return adj.fwd.spmm(x, val=val)

    @staticmethod
    def backward(ctx, dy):
        dy, _ = _rows(dy)
        x, val, val_t, deg = ctx.saved_tensors
        adj = ctx.adj
        dx = adj.bwd.spmm(dy, val=val_t) if ctx.needs_input_grad[1] else None
        dw = None
        if ctx.needs_input_grad[2]:
            dval, R = adj.dval(dy, x, val)
            C = adj.colsum(dval, val_t) if adj.aggr == "gcn" else None
            dw = adj.values_bwd(dval, R if adj.aggr != "sum" else None, C, None, deg=deg)
        return None, dx, dw


def spmm_w(adj, x, w):
    """Aggregation at live edge weights: `adj` a graph.CSRAdj built for aggr "sum", "mean" or "gcn" (its structure is used, its
    stored values are not), w fp32 [E] on the device in the order of the edge_index the adjacency was built from.  The result
    has the bits ops.spmm gives on an adjacency built from w, and is differentiable in x and in w."""
    _need_weighted(adj, "spmm_w", "edge-weight gradient")
    if (not isinstance(w, torch.Tensor) or w.dim() != 1 or w.shape[0] != adj.nnz or w.dtype != torch.float32 or
            w.device != adj.fwd.rowptr.device):
        got = f"{tuple(w.shape)} {w.dtype} on {w.device}" if isinstance(w, torch.Tensor) else type(w).__name__
        raise ValueError(f"spmm_w: w must be {adj.nnz} fp32 on {adj.fwd.rowptr.device} (one per edge, the order of edge_index), "
                         f"got {got}")
    return SpMMWFn.apply(adj, x, w)


class SpMMDropFn(torch.autograd.Function):
    """y = A' @ x with A' the adjacency under edge dropout (DropEdge; K2d, CSRAdj.dropedge_values: one keep bit per entry from the
    dropout words of this pass, the dropped entries at weight +0.0, K2's normalisation of the masked weights); backward
    dx = A'^T @ dy on K1 with the transposed values of the SAME draw.  The mask is a constant: no gradient to the weights.
    The draw's values live in the adjacency's per-call_id buffers, which the next draw of that call_id overwrites; the backward
    uses them as they are when no draw has come in between (always so inside a captured step) and otherwise draws again from
    the words its forward read."""
    @staticmethod
    def forward(ctx, adj, x, p, call_id, symmetric):
        _need_gpu(x)
        x, _ = _rows(x)
        words = rng_tensor(x.device)  # this pass's (seed, step): a redraw in the backward re-reads THESE
        val, val_t, _deg = adj.dropedge_values(p, call_id, symmetric, rng=words)
        ctx.adj, ctx.cfg, ctx.rng_words = adj, (p, call_id, symmetric), words
        ctx.rec = adj.dropedge_record(call_id)  # the buffers' record: its "gen" counts the draws that went into them
        ctx.val_t, ctx.gen = val_t, ctx.rec["gen"]
        ctx.rng_epoch = rng_epoch(x.device)
        return adj.fwd.spmm(x, val=val)

    @staticmethod
    def backward(ctx, dy):
        dy, _ = _rows(dy)
        adj = ctx.adj
        p, call_id, symmetric = ctx.cfg
        val_t = ctx.val_t
        if ctx.rec["gen"] != ctx.gen:  # another draw has overwritten the buffers since the forward
            if ctx.rng_words is rng_state(dy.device):  # no snapshot was taken: the live words must be unchanged
                check_rng_epoch(dy.device, ctx.rng_epoch, "SpMMDropFn.backward")
            val_t = adj.dropedge_values(p, call_id, symmetric, rng=ctx.rng_words)[1]
        return None, adj.bwd.spmm(dy, val=val_t), None, None, None


def _dropedge_args(adj, p, what):
    _need_weighted(adj, what, "edge dropout")
    p = float(p)
    if not (0.0 <= p < 1.0):
        raise ValueError(f"{what}: the edge dropout rate must lie in [0, 1), got {p!r}")
    return p


def spmm_dropedge(adj, x, p, call_id, symmetric=True):
    """Aggregation under edge dropout: `adj` a graph.CSRAdj built for aggr "sum", "mean" or "gcn".  Every call draws one keep
    bit per adjacency entry from (rng_tensor's (seed, step), call_id, destination, source, N) — with symmetric=True the two
    directions of an undirected edge, and parallel duplicates, share one bit — and aggregates with K2's values of the masked
    weights: the bits of ops.spmm_w(adj, x, w * keep), differentiable in x only.  No 1 / (1 - p) rescale (as PyG's
    dropout_edge): "mean" and "gcn" renormalise by construction, "sum" does NOT — its expected output shrinks by 1 - p.  A dropped
    entry stays in the structure at value +0.0: K1 still gathers its source row, so a non-finite source row propagates as it
    does at a stored weight of 0."""
    p = _dropedge_args(adj, p, "spmm_dropedge")
    return SpMMDropFn.apply(adj, x, p, int(call_id), bool(symmetric))


def edge_keep_mask(adj, p, call_id, symmetric=True):
    """uint8 [E] in the order of the edge_index `adj` was built from: the keep bits ops.spmm_dropedge(adj, x, p, call_id,
    symmetric) draws at the CURRENT dropout words (rng_tensor).  A copy of its own: later draws do not change it."""
    p = _dropedge_args(adj, p, "edge_keep_mask")
    keep = adj.dropedge_values(p, int(call_id), bool(symmetric), want_keep=True)[3]
    out = torch.empty_like(keep)
    out[adj.perm] = keep
    return out


def spmm(adj, x):
    aggr = getattr(adj, "aggr", None)
    if aggr == "max":
        return SpMMMaxFn.apply(adj, x)
    if aggr in _OWN_CALL:
        why, call = _OWN_CALL[aggr]
        raise GlassHipError(f"spmm: a {aggr} adjacency {why}; call {call}")
    return SpMMFn.apply(adj, x)


# ---------------------------------------------------------------------------------------------
# K3+K4  label + embedding
# ---------------------------------------------------------------------------------------------
class EmbedLabelFn(torch.autograd.Function):
    """(h, mask) = (W[x], label byte).  Backward dW = S^T @ dh on K1 via graph.Selection."""
    @staticmethod
    def forward(ctx, weight, x_flat, z, selection):
        _need_gpu(weight, x_flat, z)
        n, (V, H) = x_flat.shape[0], weight.shape
        w = weight.contiguous()
        out = torch.empty((n, H), dtype=torch.float32, device=w.device)
        mask = torch.empty(n, dtype=torch.uint8, device=w.device)
        zp = 0 if z is None else z.data_ptr()
        rc = _lib.load().glass_embed_label_f32(x_flat.data_ptr(), w.data_ptr(), V, zp, 0, 0, out.data_ptr(), H,
                                               mask.data_ptr(), n, H, _stream())
        _lib.check(rc, "glass_embed_label_f32")
        ctx.selection = selection
        ctx.mark_non_differentiable(mask)
        ctx.set_materialize_grads(False)  # no zero-filled gradient tensor for the mask output
        return out, mask

    @staticmethod
    def backward(ctx, dout, _dmask):
        dout, _ = _rows(dout)
        return ctx.selection.op.spmm(dout), None, None, None


def embed_label(weight, x_flat, z, selection):
    return EmbedLabelFn.apply(weight, x_flat, z, selection)


# ---------------------------------------------------------------------------------------------
# mix
# ---------------------------------------------------------------------------------------------
class MixFn(torch.autograd.Function):
    """out = mask ? zr*a1+(1-zr)*a0 : zr*a0+(1-zr)*a1 with a = act(T), T = [T1 | T0]  [N,2H]."""
    @staticmethod
    def forward(ctx, T, mask, z_ratio, act):
        _need_gpu(T, mask)
        T, ldt = _rows(T)
        n, H = T.shape[0], T.shape[1] // 2
        out = torch.empty((n, H), dtype=torch.float32, device=T.device)
        rc = _lib.load().glass_mix_fwd_f32(T.data_ptr(), ldt, mask.data_ptr(), float(z_ratio), act, out.data_ptr(), H,
                                           n, H, _stream())
        _lib.check(rc, "glass_mix_fwd_f32")
        ctx.save_for_backward(T if act != ACT_NONE else None, mask)
        ctx.z_ratio, ctx.act, ctx.shape = float(z_ratio), act, (n, H)
        return out

    @staticmethod
    def backward(ctx, dout):
        T, mask = ctx.saved_tensors
        n, H = ctx.shape
        dout, ldd = _rows(dout)
        dT = torch.empty((n, 2 * H), dtype=torch.float32, device=dout.device)
        tp, ldt = (0, 0) if T is None else (T.data_ptr(), T.stride(0))
        rc = _lib.load().glass_mix_bwd_f32(dout.data_ptr(), ldd, tp, ldt, mask.data_ptr(), ctx.z_ratio, ctx.act,
                                           dT.data_ptr(), 2 * H, n, H, _stream())
        _lib.check(rc, "glass_mix_bwd_f32")
        return dT, None, None, None


def mix(T, mask, z_ratio, act):
    return MixFn.apply(T, mask, z_ratio, act)


# ---------------------------------------------------------------------------------------------
# K5  the two Linears of a weight-set pair as one GEMM; weight gradient on the fp32 matrix cores
# ---------------------------------------------------------------------------------------------
import os as _os

# (Weight gradients on a side stream beside the backward chain were measured on MI355X at ppi_bp-shape, hipGraph replay,
# 3 interleaved A/B rounds: 0.765 ms/step forked vs 0.678 on one stream — the fork/join dependencies cost more than the
# overlap of these 10-20 us kernels buys.  The variant is not part of the product; DESIGN.md §7 keeps the record.)
USE_FUSED_DENSE = _os.environ.get("GLASS_FUSED_DENSE", "1") != "0"  # A/B switch: fused MFMA dense path
# Product form of the LDS-tiled dense kernels (hidden 128 / 256 / 512): the default is the split-bf16 form; GLASS_DENSE_SPLIT=0
# (or setting this flag) asks every dense call for the f32-input MFMA instead — an option of each CALL (the library itself
# keeps no such state: include/glass_hip.h GLASS_DENSE_F32_PRODUCTS)
DENSE_F32_PRODUCTS = _os.environ.get("GLASS_DENSE_SPLIT", "1") == "0"


def act_word(act):
    """The `act` argument of the dense entries: activation code + this call's options."""
    return int(act) | (_lib.DENSE_F32_PRODUCTS if DENSE_F32_PRODUCTS else 0)
_wgrad_ws = {}
_retired_ws = []


def _wgrad_workspace(device, N, O, I, slot=0, min_bytes=0):
    nbytes = max(_lib.load().glass_linear_wgrad_ws_bytes(N, O, I), min_bytes)
    ws = _wgrad_ws.get((device, slot))
    if ws is None or ws.numel() * 4 < nbytes:
        if ws is not None:
            _retired_ws.append(ws)  # a captured graph may still launch with this pointer: never hand it back
        ws = torch.empty(nbytes // 4 + 16, dtype=torch.float32, device=device)
        _wgrad_ws[(device, slot)] = ws
    return ws


def linear_wgrad(G, X, dW, db, accumulate, slot=0):
    """dW (+)= G^T @ X, db (+)= colsum(G) with glass_linear_wgrad_f32; False if the shape is unsupported.
    `slot` selects a scratch buffer (calls that may overlap on different streams need different ones)."""
    G, ldg = _rows(G)
    X, ldx = _rows(X)
    N, O = G.shape
    I = X.shape[1]
    thin = O <= 3 and I % 4 == 0 and ldx % 4 == 0 and X.data_ptr() % 16 == 0  # hidden -> 1 heads: the library's thin kernels
    if dW.stride(1) != 1 or not (thin or not (O % 4 or I % 2 or ldg % 4 or ldx % 2 or G.data_ptr() % 16 or X.data_ptr() % 8)):
        return False
    ws = _wgrad_workspace(G.device, N, O, I, slot)
    rc = _lib.load().glass_linear_wgrad_f32(G.data_ptr(), ldg, X.data_ptr(), ldx, N, O, I, dW.data_ptr(), dW.stride(0),
                                            0 if db is None else db.data_ptr(), int(accumulate), ws.data_ptr(),
                                            _stream())
    _lib.check(rc, "glass_linear_wgrad_f32")
    return True


class LinearFn(torch.autograd.Function):
    """y = x @ W^T + b for a plain nn.Linear whose weight gradient reduces over MANY rows into a tiny [O, I] output (the
    SSL pre-training path's MyGCNConv / MLP layers over all nodes or a 131 072-edge batch): forward and dx are library
    GEMMs through torch, dW / db the split-K MFMA kernel (glass_linear_wgrad_f32) — the library takes 160-290 us per
    such weight gradient at ppi_bp-shape (rocprofv3: 44 % of a pre-training step), the kernel 20-40."""
    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        ctx.has_bias = b is not None
        return torch.addmm(b, x, W.t()) if b is not None else x @ W.t()

    @staticmethod
    def backward(ctx, dy):
        x, W = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            dx = None
        elif W.shape[0] == 1:
            dx = dy * W  # one output: an outer product (bitwise what the K = 1 GEMM gives), no library call
        else:
            dx = dy @ W
        dW = db = None
        if ctx.needs_input_grad[1]:
            dyc, xc = dy.contiguous(), x.contiguous()
            dW = torch.empty_like(W)
            db = torch.empty(W.shape[0], dtype=W.dtype, device=W.device) if ctx.has_bias else None
            if not (dyc.is_cuda and linear_wgrad(dyc, xc, dW, db, accumulate=False, slot=("linear", W.shape))):
                dW = dyc.t() @ xc
                db = dyc.sum(0) if ctx.has_bias else None
        elif ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum(0)
        return dx, dW, db


def linear(x, lin):
    """nn.Linear forward through LinearFn (2-D CUDA fp32 inputs; anything else: torch's own)."""
    if x.dim() == 2 and x.is_cuda and x.dtype == torch.float32 and lin.weight.dtype == torch.float32:
        return LinearFn.apply(x, lin.weight, lin.bias)
    return torch.nn.functional.linear(x, lin.weight, lin.bias)


def _wgrad_supported(G, X, dW):
    O, I = G.shape[1], X.shape[1]
    return not (O % 4 or I % 2 or G.stride(0) % 4 or X.stride(0) % 2 or G.data_ptr() % 16 or X.data_ptr() % 8 or
                G.stride(1) != 1 or X.stride(1) != 1 or dW.stride(1) != 1)


def _arena_grads_live(stack, params):
    """The in-place gradient path writes into the arena views stack[2] / stack[3] and hands autograd None.  That is only
    correct while every parameter's .grad still IS its arena view: optimizer.zero_grad(set_to_none=True) (torch's
    default) detaches them, after which gradients written to the arena would never reach the optimizer."""
    base = stack[2].untyped_storage().data_ptr()
    return all(p.grad is not None and p.grad.untyped_storage().data_ptr() == base for p in params)


class StackedLinearFn(torch.autograd.Function):
    """T = x @ [W1; W0]^T + [b1 | b0]  — both weight sets of a GLASSConv Linear pair in one GEMM
    (rocBLAS/hipBLASLt through torch).  With a ParamArena the stacked weight is a view (no cat) and
    the backward accumulates dW / db straight into the gradient arena with the split-K MFMA kernel."""
    @staticmethod
    def forward(ctx, x, w1, w0, b1, b0, stack, rep=None):
        _need_gpu(x, w1)
        if stack is not None:
            W, b = stack[0], stack[1]
        else:
            W, b = torch.cat((w1, w0)), torch.cat((b1, b0))
        ctx.save_for_backward(x, W)
        ctx.stack = stack
        ctx.rep = rep if (rep is not None and rep.sink is not None) else None
        ctx.params = (w1, w0, b1, b0)
        ctx.split = w1.shape[0]
        return torch.addmm(b, x, W.t())

    @staticmethod
    def backward(ctx, dT):
        x, W = ctx.saved_tensors
        dT, _ = _rows(dT)
        if ctx.stack is not None and not _arena_grads_live(ctx.stack, ctx.params):
            ctx.stack = None  # .grad no longer aliases the arena: gradients go back through autograd
        dx = torch.mm(dT, W) if (ctx.needs_input_grad[0] and ctx.rep is None) else (None if not ctx.needs_input_grad[0] else dT)
        if ctx.rep is not None:
            # replicas: every replica's weight gradient on its own, into its slot of the sink (summed over the replicas in a
            # fixed order when the whole batch is through: RepSink.fold) — the bits do not depend on the grouping
            rep, N = ctx.rep, ctx.rep.N
            Ws, bs = rep.sink.linear(ctx.params, W.shape)
            if dx is not None:
                # (the library GEMM picks its kernel by the row count: one product per replica, N rows whatever the group)
                dx = torch.empty((dT.shape[0], W.shape[1]), dtype=dT.dtype, device=dT.device)
            for r in range(rep.R):
                g, xr = dT[r * N:(r + 1) * N], x[r * N:(r + 1) * N]
                if dx is not None:
                    torch.mm(g, W, out=dx[r * N:(r + 1) * N])
                dWr, dbr = Ws[rep.rep0 + r], bs[rep.rep0 + r]
                if not linear_wgrad(g, xr, dWr, dbr, False):
                    g, xr = g.clone(), xr.clone()  # (fresh, equally aligned operands whatever the group's base address)
                    torch.mm(g.t(), xr, out=dWr)
                    torch.sum(g, 0, out=dbr)
            return dx, None, None, None, None, None, None
        if ctx.stack is not None and _wgrad_supported(dT, x, ctx.stack[2]) and ctx.stack[2].is_contiguous():
            # arena views: dW / db accumulate straight into the gradient arena (no temporaries, no autograd add kernels)
            if linear_wgrad(dT, x, ctx.stack[2], ctx.stack[3], True):
                return dx, None, None, None, None, None, None
        dW = torch.empty_like(W)
        db = torch.empty(W.shape[0], dtype=W.dtype, device=W.device)
        if not linear_wgrad(dT, x, dW, db, False):
            dW = torch.mm(dT.t(), x)
            db = dT.sum(0)
        k = ctx.split
        return dx, dW[:k], dW[k:], db[:k], db[k:], None, None


def stacked_linear(x, lin1, lin0, stack=None, rep=None):
    return StackedLinearFn.apply(x, lin1.weight, lin0.weight, lin1.bias, lin0.bias, stack, rep)


class JoinColsFn(torch.autograd.Function):
    """`buf` already holds the column blocks `parts` (each op wrote its output straight into its slice of
    the JK buffer); this only tells autograd that buf depends on them — no copy in either direction
    (replaces torch.cat((xs...), -1) of reference impl/models.py:263)."""
    @staticmethod
    def forward(ctx, buf, *parts):
        off = 0
        for p in parts:
            if p.data_ptr() != buf.data_ptr() + 4 * off or p.stride(0) != buf.stride(0) or p.shape[0] != buf.shape[0]:
                raise GlassHipError("JoinColsFn: parts must be consecutive column slices of buf")
            off += p.shape[1]
        ctx.widths = [p.shape[1] for p in parts]
        return buf.view_as(buf)

    @staticmethod
    def backward(ctx, g):
        outs, off = [], 0
        for w in ctx.widths:
            outs.append(g[:, off:off + w])
            off += w
        return (None, *outs)


def join_cols(buf, parts):
    return JoinColsFn.apply(buf, *parts)


# A/B switches of the fused dense path per hidden size (the library itself keeps no state): GLASS_DENSE_H128=0 /
# GLASS_DENSE_H256=0 send that width back to library GEMMs + stand-alone mix kernels.
_DENSE_OFF = {h for h in (128, 256, 512) if os.environ.get(f"GLASS_DENSE_H{h}", "1") == "0"}


def dual_linear_supported(H):
    return int(H) not in _DENSE_OFF and bool(_lib.load().glass_dual_linear_supported(int(H)))


class DualLinearMixFn(torch.autograd.Function):
    """out = mix(act(Z1), act(Z0)) with Z = [xa || xb] @ [W1;W0]^T + [b1|b0] in ONE kernel on the fp32 matrix
    cores (glass_dual_linear_fwd_f32); xb=None for the trans pair (ELU, Z kept for the backward), xb=x_ for
    the comb pair (no activation, no cat, Z never materialised).  Backward: one fused data-gradient kernel
    and the split-K weight-gradient kernel, both synthesising dZ from `dout` on the fly; weight / bias
    gradients are accumulated straight into the gradient arena (stack = arena views W, b, dW, db + the packed
    operand images of W and W^T)."""
    @staticmethod
    def forward(ctx, xa, xb, w1, w0, b1, b0, mask, z_ratio, act, stack, out, rep=None):
        ctx.rep = rep if (rep is not None and rep.sink is not None) else None
        _need_gpu(xa, mask)
        xa, lda = _rows(xa)
        n, H = xa.shape
        if xb is not None:
            xb, ldb = _rows(xb)
        Wimg, b = stack[4], stack[1]
        T = torch.empty((n, 2 * H), dtype=torch.float32, device=xa.device) if act != ACT_NONE else None
        if out is None:
            out = torch.empty((n, H), dtype=torch.float32, device=xa.device)
        rc = _lib.load().glass_dual_linear_fwd_f32(xa.data_ptr(), lda, 0 if xb is None else xb.data_ptr(),
                                                   0 if xb is None else ldb, Wimg.data_ptr(), b.data_ptr(),
                                                   mask.data_ptr(), float(z_ratio), act_word(act), 0 if T is None else T.data_ptr(),
                                                   2 * H, out.data_ptr(), out.stride(0), n, H, 0, 0, 0, 0, 0, 0.0, 0, 0, 0, 0,
                                                   0, 0, _stream())
        _lib.check(rc, "glass_dual_linear_fwd_f32")
        ctx.save_for_backward(xa, xb, T, mask)
        ctx.cfg = (float(z_ratio), act, stack, n, H)
        ctx.params = (w1, w0, b1, b0)
        return out

    @staticmethod
    def backward(ctx, dout):
        xa, xb, T, mask = ctx.saved_tensors
        z_ratio, act, stack, n, H = ctx.cfg
        dout, ldd = _rows(dout)
        n_out = H if xb is None else 2 * H
        lib = _lib.load()
        tp, ldt = (0, 0) if T is None else (T.data_ptr(), T.stride(0))
        din = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            din = torch.empty((n, n_out), dtype=torch.float32, device=dout.device)
            rc = lib.glass_dual_linear_dgrad_f32(dout.data_ptr(), ldd, tp, ldt, mask.data_ptr(), z_ratio, act_word(act),
                                                 stack[5].data_ptr(), n_out, 0, 0, 0.0, 0, 0, din.data_ptr(), n_out, n, H,
                                                 0, 0, 0, 0, 0, 0, 0.0, 0, 0, _stream())
            _lib.check(rc, "glass_dual_linear_dgrad_f32")
        I = n_out
        ws = _wgrad_workspace(dout.device, n, 2 * H, I)
        da = din if xb is None else (None if din is None else din[:, :H])
        db_ = None if (xb is None or din is None) else din[:, H:]
        if ctx.rep is not None:
            # replicas: one weight-gradient launch per replica into its slot of the sink (see StackedLinearFn.backward)
            rep, N = ctx.rep, ctx.rep.N
            Ws, bs = rep.sink.linear(ctx.params, (2 * H, I))
            for r in range(rep.R):
                mk = mask[r * N:(r + 1) * N]
                if mk.data_ptr() % 16:
                    mk = mk.clone()
                dWr, dbr = Ws[rep.rep0 + r], bs[rep.rep0 + r]
                rc = lib.glass_dual_linear_wgrad_f32(dout[r * N:].data_ptr(), ldd, 0 if T is None else T[r * N:].data_ptr(), ldt,
                                                     mk.data_ptr(), z_ratio, act_word(act), xa[r * N:].data_ptr(), xa.stride(0),
                                                     0 if xb is None else xb[r * N:].data_ptr(),
                                                     0 if xb is None else xb.stride(0), N, H, dWr.data_ptr(), dWr.stride(0),
                                                     dbr.data_ptr(), 0, ws.data_ptr(), _stream())
                _lib.check(rc, "glass_dual_linear_wgrad_f32")
            return da, db_, None, None, None, None, None, None, None, None, None, None
        live = _arena_grads_live(stack, ctx.params)
        if live:   # accumulate straight into the gradient arena
            dW, dbias, accumulate = stack[2], stack[3], 1
        else:      # .grad was detached from the arena (zero_grad(set_to_none=True)): hand the gradients to autograd
            dW = torch.empty((2 * H, I), dtype=torch.float32, device=dout.device)
            dbias = torch.empty(2 * H, dtype=torch.float32, device=dout.device)
            accumulate = 0
        rc = lib.glass_dual_linear_wgrad_f32(dout.data_ptr(), ldd, tp, ldt, mask.data_ptr(), z_ratio, act_word(act), xa.data_ptr(),
                                             xa.stride(0), 0 if xb is None else xb.data_ptr(),
                                             0 if xb is None else xb.stride(0), n, H, dW.data_ptr(),
                                             dW.stride(0), dbias.data_ptr(), accumulate, ws.data_ptr(), _stream())
        _lib.check(rc, "glass_dual_linear_wgrad_f32")
        if live:
            return da, db_, None, None, None, None, None, None, None, None, None, None
        return da, db_, dW[:H], dW[H:], dbias[:H], dbias[H:], None, None, None, None, None, None


def dual_linear_mix(xa, xb, lin1, lin0, mask, z_ratio, act, stack, out=None, rep=None):
    return DualLinearMixFn.apply(xa, xb, lin1.weight, lin0.weight, lin1.bias, lin0.bias, mask, z_ratio, act, stack, out, rep)


# ---------------------------------------------------------------------------------------------
# K6  GraphNorm (+ELU +dropout)
# ---------------------------------------------------------------------------------------------
_gn_ws = {}


def _graphnorm_ws(device, n_rows, C):
    """Per-workgroup partial sums of the stand-alone GraphNorm kernels: one buffer per width and per BRANCH
    (graph.set_workspace_branch: the parallel evaluation branches of evalstep.EvalGraph run the same kernels concurrently
    and must not share it).  A buffer that has to grow is retired, not freed (a captured graph may hold its pointer)."""
    from . import graph as ggraph
    key = (device, C, ggraph._ws_branch)
    nbytes = _lib.load().glass_graphnorm_ws_bytes(n_rows, C)
    ws = _gn_ws.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        if ws is not None:
            _retired_ws.append(ws)
        ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=device)
        _gn_ws[key] = ws
    return ws


class GraphNormFn(torch.autograd.Function):
    """y = dropout(act(GraphNorm(x))) over the whole graph (PyG GraphNorm with batch=None)."""
    @staticmethod
    def forward(ctx, x, gamma, beta, alpha, eps, act, p_drop, call_id, direct=False):
        _need_gpu(x, gamma)
        x, ldx = _rows(x)
        n, C = x.shape
        y = torch.empty((n, C), dtype=torch.float32, device=x.device)
        saved = torch.empty(4 * C, dtype=torch.float32, device=x.device)
        ws = _graphnorm_ws(x.device, n, C)
        words = rng_tensor(x.device) if p_drop > 0 else None  # this pass's (seed, step): the backward re-reads THESE
        rng = words.data_ptr() if words is not None else 0
        g, b, a = gamma.contiguous(), beta.contiguous(), alpha.contiguous()
        rc = _lib.load().glass_graphnorm_fwd_f32(x.data_ptr(), ldx, y.data_ptr(), C, n, C, g.data_ptr(), b.data_ptr(),
                                                 a.data_ptr(), eps, saved.data_ptr(), act, p_drop, rng, call_id,
                                                 ws.data_ptr(), _stream())
        _lib.check(rc, "glass_graphnorm_fwd_f32")
        ctx.save_for_backward(x, g, a, saved)
        ctx.cfg = (act, p_drop, call_id)
        ctx.rng_words = words
        ctx.rng_epoch = rng_epoch(x.device)
        # direct: parameter gradients are accumulated straight into the flat gradient arena
        ctx.direct = (gamma, beta, alpha) if (direct and all(t.grad is not None for t in (gamma, beta, alpha))) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, a, saved = ctx.saved_tensors
        act, p_drop, call_id = ctx.cfg
        n, C = x.shape
        dy, lddy = _rows(dy)
        dx = torch.empty((n, C), dtype=torch.float32, device=x.device)
        if ctx.direct is not None:
            dg, db, da = (t.grad for t in ctx.direct)
            accumulate = 1
        else:
            dparams = torch.empty((3, C), dtype=torch.float32, device=x.device)
            dg, db, da = dparams[0], dparams[1], dparams[2]
            accumulate = 0
        ws = _graphnorm_ws(x.device, n, C)
        if p_drop > 0 and ctx.rng_words is rng_state(x.device):  # no snapshot was taken: the live words must be unchanged
            check_rng_epoch(x.device, ctx.rng_epoch, "GraphNormFn.backward")
        rng = ctx.rng_words.data_ptr() if p_drop > 0 else 0
        rc = _lib.load().glass_graphnorm_bwd_f32(dy.data_ptr(), lddy, x.data_ptr(), x.stride(0), dx.data_ptr(), C, 0, 0,
                                                 n, C, g.data_ptr(), a.data_ptr(), saved.data_ptr(), dg.data_ptr(),
                                                 db.data_ptr(), da.data_ptr(), accumulate, act, p_drop, rng, call_id,
                                                 ws.data_ptr(), _stream())
        _lib.check(rc, "glass_graphnorm_bwd_f32")
        if ctx.direct is not None:
            return dx, None, None, None, None, None, None, None, None
        return dx, dg, db, da, None, None, None, None, None


def graphnorm(x, gamma, beta, alpha, eps=1e-5, act=ACT_NONE, p_drop=0.0, call_id=0, direct=False):
    return GraphNormFn.apply(x, gamma, beta, alpha, float(eps), int(act), float(p_drop), int(call_id), bool(direct))


# ---------------------------------------------------------------------------------------------
# K6s  per-graph GraphNorm over a batch of graphs
# ---------------------------------------------------------------------------------------------
class SegPtr:
    """Marks an int32 device vector [B + 1] as segment POINTERS (row s of the batch's graphs: seg_ptr[s] .. seg_ptr[s + 1] - 1,
    seg_ptr[0] = 0, seg_ptr[B] = n) — so that it cannot be taken for a PyG batch vector (one graph index per row)."""
    def __init__(self, seg_ptr):
        if not isinstance(seg_ptr, torch.Tensor) or seg_ptr.dtype != torch.int32 or seg_ptr.dim() != 1 or seg_ptr.numel() < 1:
            raise ValueError("SegPtr takes an int32 vector [B + 1]")
        self.ptr = seg_ptr.contiguous()

    def __len__(self):
        return self.ptr.numel() - 1


class GraphNormSegFn(torch.autograd.Function):
    """y = act(GraphNorm(x, batch)): mean and variance over each graph's own rows (PyG GraphNorm with a batch vector)."""
    @staticmethod
    def forward(ctx, x, seg_ptr, gamma, beta, alpha, eps, act, direct=False):
        _need_gpu(x, seg_ptr, gamma)
        x, ldx = _rows(x)
        n, C = x.shape
        B = seg_ptr.numel() - 1
        y = torch.empty((n, C), dtype=torch.float32, device=x.device)
        stats = torch.empty((2, max(B, 1), C), dtype=torch.float32, device=x.device)
        g, b, a = gamma.contiguous(), beta.contiguous(), alpha.contiguous()
        rc = _lib.load().glass_graphnorm_seg_fwd_f32(x.data_ptr(), ldx, y.data_ptr(), C, seg_ptr.data_ptr(), B, C, g.data_ptr(),
                                                     b.data_ptr(), a.data_ptr(), eps, stats[0].data_ptr(), stats[1].data_ptr(),
                                                     act, _stream())
        _lib.check(rc, "glass_graphnorm_seg_fwd_f32")
        ctx.save_for_backward(x, seg_ptr, g, b, a, stats)
        ctx.act = act
        # direct: parameter gradients are accumulated straight into the flat gradient arena
        ctx.direct = (gamma, beta, alpha) if (direct and all(t.grad is not None for t in (gamma, beta, alpha))) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, seg_ptr, g, b, a, stats = ctx.saved_tensors
        n, C = x.shape
        B = seg_ptr.numel() - 1
        dy, lddy = _rows(dy)
        dx = torch.empty((n, C), dtype=torch.float32, device=x.device)
        if ctx.direct is not None:
            dg, db, da = (t.grad for t in ctx.direct)
            accumulate = 1
        else:
            dparams = torch.empty((3, C), dtype=torch.float32, device=x.device)
            dg, db, da = dparams[0], dparams[1], dparams[2]
            accumulate = 0
        lib = _lib.load()
        from . import graph as ggraph
        ws = _scratch(("graphnorm_seg", C, ggraph._ws_branch), x.device, lib.glass_graphnorm_seg_ws_bytes(B, C))
        rc = lib.glass_graphnorm_seg_bwd_f32(dy.data_ptr(), lddy, x.data_ptr(), x.stride(0) if n > 1 else max(C, x.stride(0)),
                                             dx.data_ptr(), C, seg_ptr.data_ptr(), B, C, g.data_ptr(), b.data_ptr(), a.data_ptr(),
                                             stats[0].data_ptr(), stats[1].data_ptr(), dg.data_ptr(), db.data_ptr(), da.data_ptr(),
                                             accumulate, ctx.act, ws.data_ptr(), _stream())
        _lib.check(rc, "glass_graphnorm_seg_bwd_f32")
        if ctx.direct is not None:
            return dx, None, None, None, None, None, None, None
        return dx, None, dg, db, da, None, None, None


def graphnorm_seg(x, seg_ptr, gamma, beta, alpha, eps=1e-5, act=ACT_NONE, direct=False):
    """Per-graph GraphNorm; seg_ptr: int32 [B + 1] device vector of row offsets (a SegPtr or the bare tensor)."""
    if isinstance(seg_ptr, SegPtr):
        seg_ptr = seg_ptr.ptr
    if seg_ptr.dtype != torch.int32 or seg_ptr.dim() != 1 or seg_ptr.numel() < 1:
        raise GlassHipError(f"graphnorm_seg: seg_ptr must be an int32 vector [B + 1], got {tuple(seg_ptr.shape)} {seg_ptr.dtype}")
    return GraphNormSegFn.apply(x, seg_ptr.contiguous(), gamma, beta, alpha, float(eps), int(act), bool(direct))


# ---------------------------------------------------------------------------------------------
# K7  subgraph pooling
# ---------------------------------------------------------------------------------------------
# Largest padded node matrices (B * Smax entries) the ORDERED, atomic-free scatters stage in LDS (pool.hip kPoolOrderedMax,
# readout.hip kReadoutOrderedMax).  Beyond them the pool backward and the fused readout bucket the entries by node and sum
# in exact fixed point (bucket.h: still no float atomic), and so does max pooling's backward.  The C ABI's one float-atomic
# scatter (glass_segment_pool_bwd_atomic_f32) is not used by this module.
POOL_ORDERED_MAX, READOUT_ORDERED_MAX = 12288, 16384


_scratch_bufs = {}


_retired_scratch = []


def _scratch(key, device, nbytes):
    """Uninitialised device scratch of at least `nbytes`, one buffer per key (kept for the process's life).  A buffer that
    has to grow is RETIRED, not freed: a captured hipGraph may still launch with its pointer (as _wgrad_workspace does)."""
    buf = _scratch_bufs.get((device, key))
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _retired_scratch.append(buf)
        buf = _scratch_bufs[(device, key)] = torch.empty(int(nbytes) + 16, dtype=torch.uint8, device=device)
    return buf


class SegmentPoolFn(torch.autograd.Function):
    """out[b] = reduce over the non-padding nodes of pos[b] of emb[node]  (sum|mean|max|size)."""
    @staticmethod
    def forward(ctx, emb, pos, mode):
        _need_gpu(emb, pos)
        if mode not in POOL_MODES:
            raise NotImplementedError  # reference: GLASSTest.py:168-171
        emb, lde = _rows(emb)
        pos = pos.contiguous()
        if pos.dtype != torch.int64:
            pos = pos.to(torch.int64)
        n, C = emb.shape
        B, Smax = pos.shape
        out = torch.empty((B, C), dtype=torch.float32, device=emb.device)
        if Smax == 2 and mode != "max":  # node pairs (link-prediction batches): lane groups per pair, not a workgroup
            rc = _lib.load().glass_pair_pool_f32(emb.data_ptr(), lde, pos.data_ptr(), B, POOL_MODES[mode], out.data_ptr(), C,
                                                 n, C, _stream())
            _lib.check(rc, "glass_pair_pool_f32")
            ctx.save_for_backward(pos, None)
            ctx.cfg = (mode, n, C)
            return out
        argmax = torch.empty((B, C), dtype=torch.int32, device=emb.device) if mode == "max" else None
        rc = _lib.load().glass_segment_pool_f32(emb.data_ptr(), lde, pos.data_ptr(), B, Smax, POOL_MODES[mode],
                                                out.data_ptr(), C, 0 if argmax is None else argmax.data_ptr(), n, C,
                                                _stream())
        _lib.check(rc, "glass_segment_pool_f32")
        ctx.save_for_backward(pos, argmax)
        ctx.cfg = (mode, n, C)
        return out

    @staticmethod
    def backward(ctx, dout):
        pos, argmax = ctx.saved_tensors
        mode, n, C = ctx.cfg
        dout, ldd = _rows(dout)
        B, Smax = pos.shape
        if Smax == 2 and mode != "max":  # exact, atomic-free backward; writes every row
            lib = _lib.load()
            demb = torch.empty((n, C), dtype=torch.float32, device=dout.device)
            ws = _scratch(("pair_pool", n, B), dout.device, lib.glass_pair_pool_ws_bytes(n, B))
            rc = lib.glass_pair_pool_bwd_f32(dout.data_ptr(), ldd, pos.data_ptr(), B, POOL_MODES[mode], demb.data_ptr(), C, n,
                                             C, ws.data_ptr(), _stream())
            _lib.check(rc, "glass_pair_pool_bwd_f32")
            return demb, None, None
        if mode != "max" and B * Smax + B > POOL_ORDERED_MAX:  # beyond the LDS staging: bucketed by node, exact sums (no float atomics)
            lib = _lib.load()
            demb = torch.empty((n, C), dtype=torch.float32, device=dout.device)
            ws = _scratch(("pool_exact", n, B, Smax), dout.device, lib.glass_segment_pool_bwd_exact_ws_bytes(n, B, Smax))
            rc = lib.glass_segment_pool_bwd_exact_f32(dout.data_ptr(), ldd, pos.data_ptr(), B, Smax, POOL_MODES[mode],
                                                      demb.data_ptr(), C, n, C, ws.data_ptr(), _stream())
            _lib.check(rc, "glass_segment_pool_bwd_exact_f32")
            return demb, None, None
        if mode == "max":  # exact too: the node's subgraph list (deduplicated per row), gradients of the columns it won
            lib = _lib.load()
            demb = torch.empty((n, C), dtype=torch.float32, device=dout.device)
            ws = _scratch(("pool_exact_max", n, B, Smax), dout.device, lib.glass_segment_pool_bwd_exact_ws_bytes(n, B, Smax))
            rc = lib.glass_segment_pool_max_bwd_exact_f32(dout.data_ptr(), ldd, pos.data_ptr(), B, Smax, argmax.data_ptr(),
                                                          demb.data_ptr(), C, n, C, ws.data_ptr(), _stream())
            _lib.check(rc, "glass_segment_pool_max_bwd_exact_f32")
            return demb, None, None
        demb = torch.zeros((n, C), dtype=torch.float32, device=dout.device)
        rc = _lib.load().glass_segment_pool_bwd_f32(dout.data_ptr(), ldd, pos.data_ptr(), B, Smax, POOL_MODES[mode],
                                                    0 if argmax is None else argmax.data_ptr(), demb.data_ptr(), C, n,
                                                    C, _stream())
        _lib.check(rc, "glass_segment_pool_bwd_f32")
        return demb, None, None


def segment_pool(emb, pos, mode):
    return SegmentPoolFn.apply(emb, pos, mode)


# ---------------------------------------------------------------------------------------------
# K7a  attention pooling (pool "attn": an extension, csrc/pool_attn.hip)
# ---------------------------------------------------------------------------------------------
class AttnPoolFn(torch.autograd.Function):
    """out[b] = sum_j alpha[b, j] * emb[pos[b, j]], alpha = softmax over the non-padding nodes of pos[b] of emb[node] . w
    (one launch; alpha and out are what the backward keeps — it recomputes nothing of the softmax)."""
    @staticmethod
    def forward(ctx, emb, pos, weight):
        _need_gpu(emb, pos, weight)
        emb, lde = _rows(emb)
        pos = pos.contiguous()
        if pos.dtype != torch.int64:
            pos = pos.to(torch.int64)
        n, C = emb.shape
        if weight.numel() != C or weight.dtype != torch.float32:
            raise GlassHipError(f"attn_pool: gate weight {tuple(weight.shape)} {weight.dtype} for embeddings of width {C}")
        w = weight.reshape(-1).contiguous()
        B, Smax = pos.shape
        if B == 0 or Smax == 0:  # (the entry launches nothing: rows without entries pool to 0)
            out = torch.zeros((B, C), dtype=torch.float32, device=emb.device)
        else:
            out = torch.empty((B, C), dtype=torch.float32, device=emb.device)
        alpha = torch.empty((B, Smax), dtype=torch.float32, device=emb.device)
        rc = _lib.load().glass_attn_pool_f32(emb.data_ptr(), lde, pos.data_ptr(), B, Smax, w.data_ptr(), out.data_ptr(), C,
                                             alpha.data_ptr(), n, C, _stream())
        _lib.check(rc, "glass_attn_pool_f32")
        ctx.save_for_backward(emb, pos, w, alpha, out)
        ctx.cfg = (lde, tuple(weight.shape))
        ctx.mark_non_differentiable(alpha)
        return out, alpha

    @staticmethod
    def backward(ctx, dout, _dalpha):
        emb, pos, w, alpha, out = ctx.saved_tensors
        lde, wshape = ctx.cfg
        dout, ldd = _rows(dout)
        n, C = emb.shape
        B, Smax = pos.shape
        lib = _lib.load()
        demb = torch.empty((n, C), dtype=torch.float32, device=dout.device)
        dw = torch.empty(C, dtype=torch.float32, device=dout.device)
        ws = _scratch(("attn_pool", n, B, Smax, C), dout.device, lib.glass_attn_pool_bwd_ws_bytes(n, B, Smax, C))
        rc = lib.glass_attn_pool_bwd_f32(dout.data_ptr(), ldd, emb.data_ptr(), lde, pos.data_ptr(), B, Smax, w.data_ptr(),
                                         alpha.data_ptr(), out.data_ptr(), C, demb.data_ptr(), C, dw.data_ptr(), 0, n, C,
                                         ws.data_ptr(), _stream())
        _lib.check(rc, "glass_attn_pool_bwd_f32")
        return demb, None, dw.view(wshape)


def attn_pool(emb, pos, weight, return_alpha=False):
    """Attention readout of the padded node matrix `pos` ([B, Smax] int64, -1 = padding) with the gate weight `weight`
    ([C] or [1, C], no bias): [B, C] — and the attention weights [B, Smax] (no gradient) with return_alpha."""
    out, alpha = AttnPoolFn.apply(emb, pos, weight)
    return (out, alpha) if return_alpha else out


# ---------------------------------------------------------------------------------------------
# K4r / K1r / K6r  exact zero-one labels: R replicas of one graph, replica-major rows (row r * N + n)
# ---------------------------------------------------------------------------------------------
class Replicas:
    """Marks an activation matrix [R * N, C] as R replicas of one N-node graph, the replicas rep0 .. rep0 + R - 1 of a batch.
    rep0 enters the dropout key (call_id + ((rep0 + r) << 32): the replica's index in the WHOLE batch, so the key does not
    depend on how the batch is cut into groups; the generator hashes the low 32 bits of call_id only, so today all replicas
    of a call draw the SAME mask) and names the replica's slot in `sink`.  Passed as `batch` to models.GraphNorm and
    models.GLASSConv."""
    def __init__(self, R, N, rep0=0, sink=None):
        self.R, self.N, self.rep0 = int(R), int(N), int(rep0)
        self.sink = sink  # a RepSink: where the backward of a training pass over a whole batch collects parameter gradients
        if self.R < 1 or self.N < 1 or self.rep0 < 0:
            raise ValueError(f"Replicas: need R >= 1, N >= 1, rep0 >= 0 (got {R}, {N}, {rep0})")

    def __repr__(self):
        return f"Replicas(R={self.R}, N={self.N}, rep0={self.rep0})"


class RepSink:
    """Parameter gradients of ONE training pass over B replicas (EmbZGConv with z [B, N]).  The backward of every replica-form
    op writes each replica's own contribution into slot rep0 + r of a [B, ...] buffer — one weight-gradient launch per
    replica, GraphNorm's per-replica fp64 terms, the gradient of the replicated input rows — and `fold`, run by
    ReplicaRootFn's backward once every group is through, sums the slots over the replicas and adds the sums to the
    parameters' .grad.  Slot shapes and the sum's order depend on B only: the gradient bits do not depend on how the batch was
    cut into groups (EmbZGConv.replica_chunk), nor on the order in which autograd ran the groups."""
    def __init__(self, B, device):
        self.B, self.device = int(B), device
        self._lin, self._gn, self.rows = {}, {}, None

    def linear(self, params, wshape):
        """([B, 2O, I], [B, 2O]) slots of a Linear pair (params = w1, w0, b1, b0; stacked [W1; W0])."""
        hit = self._lin.get(id(params[0]))
        if hit is None:
            hit = self._lin[id(params[0])] = (params, torch.zeros((self.B, ) + tuple(wshape), dtype=torch.float32, device=self.device),
                                              torch.zeros((self.B, wshape[0]), dtype=torch.float32, device=self.device))
        return hit[1], hit[2]

    def graphnorm(self, params, C):
        """[B, 3, C] fp64 slots (sum g * xhat, sum g, dalpha) of a GraphNorm (params = gamma, beta, alpha)."""
        hit = self._gn.get(id(params[0]))
        if hit is None:
            hit = self._gn[id(params[0])] = (params, torch.zeros((self.B, 3, C), dtype=torch.float64, device=self.device))
        return hit[1]

    def input_rows(self, N, H):
        if self.rows is None:
            self.rows = torch.zeros((self.B, N, H), dtype=torch.float32, device=self.device)
        return self.rows

    @staticmethod
    def _add(p, g):
        if p.requires_grad:
            if p.grad is None:
                p.grad = g.reshape(p.shape).clone()
            else:
                p.grad.add_(g.reshape(p.shape))

    def fold(self):
        """Sum every slot buffer over the replicas into the parameters' .grad; returns the input rows' gradient [N, H]."""
        for (w1, w0, b1, b0), Ws, bs in self._lin.values():
            dW, db = Ws.sum(0), bs.sum(0)
            k = w1.shape[0]
            self._add(w1, dW[:k]), self._add(w0, dW[k:]), self._add(b1, db[:k]), self._add(b0, db[k:])
        for (gamma, beta, alpha), S in self._gn.values():
            s = S.sum(0).to(torch.float32)
            self._add(gamma, s[0]), self._add(beta, s[1]), self._add(alpha, s[2])
        return None if self.rows is None else self.rows.sum(0)


class ReplicaRootFn(torch.autograd.Function):
    """Identity on the rows every group of replicas starts from; its backward runs when all groups are through (each depends
    on it) and folds the sink: parameter gradients into .grad, the rows' gradient to autograd."""
    @staticmethod
    def forward(ctx, h, anchor, sink):
        ctx.sink = sink
        return h.view_as(h)

    @staticmethod
    def backward(ctx, _g):
        return ctx.sink.fold(), None, None


class ReplicateRowsFn(torch.autograd.Function):
    """[N, H] -> [R * N, H], the rows repeated for each replica; the backward puts each replica's gradient into its slot of the
    sink (summed by RepSink.fold) and hands autograd zeros."""
    @staticmethod
    def forward(ctx, h, rep):
        ctx.rep = rep
        return h.unsqueeze(0).expand(rep.R, *h.shape).reshape(rep.R * h.shape[0], h.shape[1])

    @staticmethod
    def backward(ctx, g):
        rep = ctx.rep
        N, H = g.shape[0] // rep.R, g.shape[1]
        rep.sink.input_rows(N, H)[rep.rep0:rep.rep0 + rep.R].copy_(g.reshape(rep.R, N, H))
        return torch.zeros((N, H), dtype=g.dtype, device=g.device), None


def replica_root(h, sink):
    """(the anchor makes the node part of the graph even when nothing upstream of h requires a gradient)"""
    return ReplicaRootFn.apply(h, torch.zeros((), device=h.device, requires_grad=True), sink)


def replicate_rows(h, rep):
    if rep.sink is None:
        return h.unsqueeze(0).expand(rep.R, *h.shape).reshape(rep.R * h.shape[0], h.shape[1])
    return ReplicateRowsFn.apply(h, rep)


def _chunk_error(lib, what):
    msg = lib.glass_last_error_string().decode(errors="replace")
    return GlassHipError(f"{what}: {msg}; run the replicas in smaller groups (EmbZGConv.replica_chunk)")


def zeroone_labels(pos, n_nodes, rep0=0, R=None):
    """Label bytes uint8 [R * n_nodes] of the rows rep0 .. rep0 + R - 1 of the padded node matrix pos [B, Smax]: byte
    r * n_nodes + n is 1 iff node n occurs in row rep0 + r (-1 and ids >= n_nodes are skipped).  One launch."""
    _need_gpu(pos)
    if pos.dim() != 2:
        raise GlassHipError(f"zeroone_labels: pos must be [B, Smax], got {tuple(pos.shape)}")
    pos = pos.contiguous()
    if pos.dtype != torch.int64:
        pos = pos.to(torch.int64)
    B, Smax = pos.shape
    R = B - int(rep0) if R is None else int(R)
    mask = torch.empty(max(R, 0) * int(n_nodes), dtype=torch.uint8, device=pos.device)
    _lib.check(_lib.load().glass_zeroone_labels_u8(pos.data_ptr(), B, Smax, int(rep0), R, int(n_nodes), mask.data_ptr(), _stream()),
               "glass_zeroone_labels_u8")
    return mask


class SpMMRepFn(torch.autograd.Function):
    """y[r] = A @ x[r] for R replicas in one launch (replica-major rows); backward dx[r] = A^T @ dy[r], the same entry on
    the CSR of A^T.  Replica r has the bits SpMMFn gives on its slice."""
    @staticmethod
    def forward(ctx, adj, x, R):
        _need_gpu(x)
        x, _ = _rows(x)
        ctx.adj, ctx.R = adj, R
        return adj.fwd.spmm_rep(x, R)

    @staticmethod
    def backward(ctx, dy):
        dy, _ = _rows(dy)
        return None, ctx.adj.bwd.spmm_rep(dy, ctx.R), None


def spmm_rep(adj, x, R):
    aggr = getattr(adj, "aggr", None)
    if aggr == "max" or aggr in _OWN_CALL:
        raise GlassHipError(f"replicated {aggr} aggregation is not built: aggr '{aggr}' runs one graph at a time (no exact "
                            "zero-one labels / --use_zeroone with it)")
    return SpMMRepFn.apply(adj, x, int(R))


class GraphNormRepFn(torch.autograd.Function):
    """y = dropout(act(GraphNorm(x))) with x [R * N, C] as R graphs of N rows, each normalised over its own rows; the shared
    parameters receive the sum of the replicas' gradients.  Replica r has the bits GraphNormFn gives on its slice with the
    dropout stream call_id + ((rep0 + r) << 32)."""
    @staticmethod
    def forward(ctx, x, gamma, beta, alpha, eps, act, p_drop, call_id, rep, direct=False):
        _need_gpu(x, gamma)
        x, ldx = _rows(x)
        n, C = x.shape
        R, N = rep.R, rep.N
        if n != R * N:
            raise GlassHipError(f"graphnorm_rep: {n} rows for {rep!r}")
        lib = _lib.load()
        y = torch.empty((n, C), dtype=torch.float32, device=x.device)
        saved = torch.empty(R * 4 * C, dtype=torch.float32, device=x.device)
        from . import graph as ggraph
        ws = _scratch(("graphnorm_rep", C, ggraph._ws_branch), x.device, lib.glass_graphnorm_rep_ws_bytes(N, C, R))
        words = rng_tensor(x.device) if p_drop > 0 else None  # this pass's (seed, step): the backward re-reads THESE
        rng = words.data_ptr() if words is not None else 0
        g, b, a = gamma.contiguous(), beta.contiguous(), alpha.contiguous()
        rc = lib.glass_graphnorm_rep_fwd_f32(x.data_ptr(), ldx, y.data_ptr(), C, N, C, R, rep.rep0, g.data_ptr(), b.data_ptr(),
                                             a.data_ptr(), eps, saved.data_ptr(), act, p_drop, rng, call_id, ws.data_ptr(),
                                             _stream())
        if rc == -3:
            raise _chunk_error(lib, "glass_graphnorm_rep_fwd_f32")
        _lib.check(rc, "glass_graphnorm_rep_fwd_f32")
        ctx.save_for_backward(x, g, a, saved)
        ctx.cfg = (act, p_drop, call_id, rep)
        ctx.sink_params = (gamma, beta, alpha) if rep.sink is not None else None
        ctx.rng_words = words
        ctx.rng_epoch = rng_epoch(x.device)
        # direct: parameter gradients are accumulated straight into the flat gradient arena
        ctx.direct = (gamma, beta, alpha) if (direct and all(t.grad is not None for t in (gamma, beta, alpha))) else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, a, saved = ctx.saved_tensors
        act, p_drop, call_id, rep = ctx.cfg
        n, C = x.shape
        dy, lddy = _rows(dy)
        dx = torch.empty((n, C), dtype=torch.float32, device=x.device)
        sink = rep.sink if ctx.sink_params is not None else None
        if sink is not None:
            dg = db = da = None  # the per-replica terms go to the sink (below); no fold in this launch
            accumulate = 0
        elif ctx.direct is not None:
            dg, db, da = (t.grad for t in ctx.direct)
            accumulate = 1
        else:
            dparams = torch.empty((3, C), dtype=torch.float32, device=x.device)
            dg, db, da = dparams[0], dparams[1], dparams[2]
            accumulate = 0
        lib = _lib.load()
        from . import graph as ggraph
        ws = _scratch(("graphnorm_rep", C, ggraph._ws_branch), x.device, lib.glass_graphnorm_rep_ws_bytes(rep.N, C, rep.R))
        if p_drop > 0 and ctx.rng_words is rng_state(x.device):  # no snapshot was taken: the live words must be unchanged
            check_rng_epoch(x.device, ctx.rng_epoch, "GraphNormRepFn.backward")
        rng = ctx.rng_words.data_ptr() if p_drop > 0 else 0
        ldx = x.stride(0) if n > 1 else max(C, x.stride(0))
        rc = lib.glass_graphnorm_rep_bwd_f32(dy.data_ptr(), lddy, x.data_ptr(), ldx, dx.data_ptr(), C, 0, 0, rep.N, C, rep.R,
                                             rep.rep0, g.data_ptr(), a.data_ptr(), saved.data_ptr(),
                                             0 if dg is None else dg.data_ptr(), 0 if db is None else db.data_ptr(),
                                             0 if da is None else da.data_ptr(), accumulate, act, p_drop, rng, call_id,
                                             ws.data_ptr(), _stream())
        _lib.check(rc, "glass_graphnorm_rep_bwd_f32")
        if sink is not None:
            # the replicas' fp64 terms [R, 3, C] lie behind the R per-replica chunks of ws (include/glass_hip.h)
            off = rep.R * lib.glass_graphnorm_ws_bytes(rep.N, C)
            terms = ws[off:off + rep.R * 3 * C * 8].view(torch.float64).view(rep.R, 3, C)
            sink.graphnorm(ctx.sink_params, C)[rep.rep0:rep.rep0 + rep.R].copy_(terms)
            return dx, None, None, None, None, None, None, None, None, None
        if ctx.direct is not None:
            return dx, None, None, None, None, None, None, None, None, None
        return dx, dg, db, da, None, None, None, None, None, None


def graphnorm_rep(x, rep, gamma, beta, alpha, eps=1e-5, act=ACT_NONE, p_drop=0.0, call_id=0, direct=False):
    """GraphNorm over the R replicas `rep` (an ops.Replicas) of one graph, each over its own N rows."""
    if not isinstance(rep, Replicas):
        raise GlassHipError(f"graphnorm_rep: rep must be an ops.Replicas, got {type(rep).__name__}")
    return GraphNormRepFn.apply(x, gamma, beta, alpha, float(eps), int(act), float(p_drop), int(call_id), rep, bool(direct))
