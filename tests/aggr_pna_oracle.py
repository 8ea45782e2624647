"""Numpy restatement of PNA neighbour aggregation (aggr "pna", K1p: glass_amd/csrc/spmm_pna.hip) — a checker, CPU only, meant
for fp64 — with the mass its backward's error bound is stated in, the degree scalers and the per-channel mix, the
winner / runner-up gap of both extremes, and a differentiable torch formulation for autograd to differentiate.

Forward CSR as graph.CSRAdj builds it (tests/aggr_max_oracle.py: entries sorted by (row, col), stable, duplicates kept, row =
destination, values = the raw edge weights, here > 0).  For row i, channel c, entries e (source j_e, weight w_e, x_e = X[j_e, c]):

    W = sum_e w_e     Mu = sum_e w_e x_e / W     Var = sum_e w_e (x_e - Mu)^2 / W     S = sqrt(Var + eps)
    Mx = max_e x_e    amx = the smallest e with x_e == Mx      Mn = min_e x_e     amn = the smallest e with x_e == Mn
    (-0.0 == +0.0; the stored extreme is the winner's own value; a row without entries: zeros, amx = amn = -1)

    backward, on the TRANSPOSED CSR (row j = source, entries t = destinations i, val_t, eid_t), with per-destination rows
    A = dS / (W S)     C = dMu / W     Gmx = dMx     Gmn = dMn     (0 where W = 0)
    dX[j, c] = sum_t [ val_t (C[i, c] + A[i, c] (X[j, c] - Mu[i, c])) + (amx[i, c] == eid_t) Gmx[i, c] + (amn[i, c] == eid_t) Gmn[i, c] ]

Moments, their bounds, gamma and the segment sums are tests/aggr_moment_oracle.py's."""
import numpy as np
import torch

import aggr_moment_oracle as MO
from aggr_max_oracle import MaxAdj
from aggr_moment_oracle import gamma, rows_of, segsum

AGGREGATORS = ("mean", "max", "min", "std")   # the order of theta's rows: theta[3 a + k], k the scaler


def extremes(rowptr, col, X):
    """(Mx, amx, Mn, amn): Mx / Mn in X's dtype holding the winner's own bits, amx / amn int32 entry indices under the tie rule."""
    rowptr, col, X = np.asarray(rowptr), np.asarray(col), np.asarray(X)
    n, H = rowptr.shape[0] - 1, X.shape[1]
    xe = X[col]
    rows = rows_of(rowptr)
    live = rowptr[1:] > rowptr[:-1]
    e_idx = np.arange(col.shape[0], dtype=np.int64)[:, None]
    out = []
    for red in (np.maximum, np.minimum):
        best = np.zeros((n, H), dtype=X.dtype)
        arg = np.full((n, H), -1, dtype=np.int64)
        if live.any():
            best[live] = red.reduceat(xe, rowptr[:-1][live], axis=0)
            hit = xe == best[rows]                                    # (== : -0.0 ties +0.0)
            arg[live] = np.minimum.reduceat(np.where(hit, e_idx, col.shape[0]), rowptr[:-1][live], axis=0)
            win = np.where(arg >= 0, arg, 0)
            best = np.where(arg >= 0, X[col[win], np.arange(H)[None, :]], 0).astype(X.dtype)   # the winner's own bits
        out += [best, arg.astype(np.int32)]
    return tuple(out)


def forward(rowptr, col, val, X, eps=1e-5):
    """aggr_moment_oracle.moments' dict (W, cnt, Mu, Var, Std, abs_x, sq_x) with Mx, amx, Mn, amn added"""
    m = MO.moments(rowptr, col, val, X, eps)
    m["Mx"], m["amx"], m["Mn"], m["amn"] = extremes(rowptr, col, np.asarray(X, dtype=np.float64))
    return m


def factors(S, W, dS, dMu):
    """(A, C) in fp64; a missing gradient (None) gives zeros"""
    S, W = np.asarray(S, dtype=np.float64), np.asarray(W, dtype=np.float64)
    live = (W > 0)[:, None]
    Wd = np.where(W > 0, W, 1.0)[:, None]
    A = np.zeros_like(S) if dS is None else np.where(live, np.asarray(dS, dtype=np.float64) / np.where(live, Wd * S, 1.0), 0.0)
    C = np.zeros_like(S) if dMu is None else np.where(live, np.asarray(dMu, dtype=np.float64) / Wd, 0.0)
    return A, C


def backward(rowptr_t, col_t, val_t, eid_t, X, Mu, A, C, amx, Gmx, amn, Gmn):
    """(dX, mass) in fp64 on the transposed CSR:
    mass[j, c] = sum_t [ val_t (|C| + |A| |X - Mu|) + hit_mx |Gmx| + hit_mn |Gmn| ]"""
    rowptr_t, col_t, eid_t = np.asarray(rowptr_t), np.asarray(col_t), np.asarray(eid_t)
    val_t, X, Mu, A, C, Gmx, Gmn = (np.asarray(a, dtype=np.float64) for a in (val_t, X, Mu, A, C, Gmx, Gmn))
    j = rows_of(rowptr_t)
    d = X[j] - Mu[col_t]
    w = val_t[:, None]
    hx = np.asarray(amx)[col_t] == eid_t[:, None]
    hn = np.asarray(amn)[col_t] == eid_t[:, None]
    term = w * (C[col_t] + A[col_t] * d) + np.where(hx, Gmx[col_t], 0.0) + np.where(hn, Gmn[col_t], 0.0)
    mass = w * (np.abs(C[col_t]) + np.abs(A[col_t]) * np.abs(d)) + np.where(hx, np.abs(Gmx[col_t]), 0.0) + \
        np.where(hn, np.abs(Gmn[col_t]), 0.0)
    return segsum(term, rowptr_t), segsum(mass, rowptr_t)


def bound_dx(rowptr_t, mass):
    """gamma(n_j + 8) mass, n_j the transposed row's entry count: each entry's term is at most five rounded operations (d, the
    fma, the product, two adds), and the n_j terms are summed in some order"""
    return gamma(np.diff(np.asarray(rowptr_t)).astype(np.float64) + 8)[:, None] * mass


# ---- the degree scalers and the mix ---------------------------------------------------------------------------------------
def delta(W):
    """the mean over the rows with W > 0 of log(W + 1); 1.0 if no row has entries"""
    W = np.asarray(W, dtype=np.float64)
    live = W > 0
    return float(np.log1p(W[live]).mean()) if live.any() else 1.0


def scalers(W, dl):
    """[n, 3]: 1, log(W + 1) / delta (amplification), delta / log(W + 1) (attenuation); zeros for a row with W = 0"""
    W = np.asarray(W, dtype=np.float64)
    live = W > 0
    lw = np.log1p(np.where(live, W, 1.0))
    return np.stack((live.astype(np.float64), np.where(live, lw / dl, 0.0), np.where(live, dl / lw, 0.0)), axis=1)


def pna_mix(Mu, Mx, Mn, S, W, dl, theta):
    """Y[i, c] = sum_{a, k} s_k(i) theta[3 a + k, c] Agg_a[i, c], aggregators in the order mean, max, min, std"""
    sc = scalers(W, dl)
    theta = np.asarray(theta, dtype=np.float64)
    return sum(np.asarray(agg, dtype=np.float64) * (sc @ theta[3 * a:3 * a + 3]) for a, agg in enumerate((Mu, Mx, Mn, S)))


# ---- how far the winner is from the runner-up ------------------------------------------------------------------------------
def smallest_gap(adj, X):
    """Smallest distance, over both extremes, every row and every channel, between the winning message and the best DIFFERENT
    message row, relative to the largest |message| of the graph (inf where no row has two).  The extremes are over the raw
    message, so entries whose whole message ROW is equal are no runner-up but a tie, and the rule decides it the same way in
    every precision: a duplicate edge names one source twice, and at the first layer two nodes with the same feature and
    label hold rows computed by the same arithmetic from the same inputs — equal in fp64 and equal in fp32.  What the
    comparison cannot bear is two DIFFERENT rows closer than fp32 resolves; that is what is measured.
    `adj` a MaxAdj, X a torch tensor [n, H]."""
    best = float("inf")
    col = adj.col
    for i in range(adj.n):
        s, e = int(adj.rowptr[i]), int(adj.rowptr[i + 1])
        P = torch.unique(X[col[s:e]], dim=0)
        if P.shape[0] >= 2:
            top = torch.topk(P, 2, dim=0).values
            low = torch.topk(-P, 2, dim=0).values
            best = min(best, float((top[0] - top[1]).min()), float((low[0] - low[1]).min()))
    scale = float(X[col].abs().max()) if col.numel() else 1.0
    return best / scale


# ---- the same operator from differentiable torch ops ----------------------------------------------------------------------
class _ExtremeFn(torch.autograd.Function):
    """(Mx, Mn) of X under the tie rule; the gradient of each goes to the winning entry's source alone"""
    @staticmethod
    def forward(ctx, X, adj):
        Mx, amx, Mn, amn = extremes(adj.rowptr.numpy(), adj.col.numpy(), X.detach().numpy())
        ctx.adj, ctx.args = adj, (torch.from_numpy(amx), torch.from_numpy(amn))
        adj.last_args = ctx.args
        return torch.from_numpy(Mx), torch.from_numpy(Mn)

    @staticmethod
    def backward(ctx, dMx, dMn):
        a = ctx.adj
        H = dMx.shape[1]
        dX = torch.zeros((a.n, H), dtype=dMx.dtype)
        cols = torch.arange(H)[None, :].expand(a.n, H)
        for g, arg in zip((dMx, dMn), ctx.args):
            live = arg >= 0
            src = a.col[arg.to(torch.int64).clamp(min=0)]           # the winning entry's source, per (i, c)
            dX.index_put_((src[live], cols[live]), g[live], accumulate=True)
        return dX, None


def torch_pna(edge_index, edge_weight, n, X, eps=1e-5, adj=None):
    """(Mu, Mx, Mn, S) differentiable in X: the moments by aggr_moment_oracle.scatter_moments, the extremes under the tie rule"""
    adj = MaxAdj(edge_index, edge_weight, n) if adj is None else adj
    S, Mu = MO.scatter_moments(edge_index, edge_weight, n, X, "std", eps)
    Mx, Mn = _ExtremeFn.apply(X, adj)
    return Mu, Mx, Mn, S


def scatter_pna(edge_index, edge_weight, n, X, eps=1e-5):
    """(Mu, Mx, Mn, S) on the raw edge list from torch's own ops alone (scatter_reduce amax / amin): autograd splits the
    gradient of an extreme evenly over equal values, so this is the operator above only where equal messages of a row come
    from one source (duplicate edges) — there the shares land on the same row of X and add up to the whole."""
    S, Mu = MO.scatter_moments(edge_index, edge_weight, n, X, "std", eps)
    idx = edge_index[0][:, None].expand(edge_index.shape[1], X.shape[1])
    zeros = torch.zeros((n, X.shape[1]), dtype=X.dtype)
    Mx = zeros.scatter_reduce(0, idx, X[edge_index[1]], "amax", include_self=False)
    Mn = zeros.scatter_reduce(0, idx, X[edge_index[1]], "amin", include_self=False)
    return Mu, Mx, Mn, S


def torch_mix(Mu, Mx, Mn, S, W, dl, theta):
    """pna_mix from differentiable torch ops (W a tensor [n], dl a float, theta [12, H])"""
    sc = torch.from_numpy(scalers(W.detach().numpy(), dl)).to(Mu.dtype)
    return sum(agg * (sc @ theta[3 * a:3 * a + 3]) for a, agg in enumerate((Mu, Mx, Mn, S)))


class PnaAdj(MaxAdj):
    """`PnaAdj(edge_index, edge_weight, n, theta, eps) @ X`: the differentiable PNA aggregation of a GLASSConv layer in the dtype
    of X, theta [12, H] the layer's pna_weight; takes the place of OracleConv.adj.  `seen` collects the operands."""
    def __init__(self, edge_index, edge_weight, n, theta, eps=1e-5):
        super().__init__(edge_index, edge_weight, n)
        self.edge_index, self.edge_weight, self.theta, self.eps = edge_index, edge_weight, theta, eps
        self.W = torch.zeros(n, dtype=torch.float64).index_add(0, edge_index[0], edge_weight.double())
        self.delta = delta(self.W.numpy())

    def __matmul__(self, X):
        self.seen.append(X.detach().clone())
        return torch_mix(*torch_pna(self.edge_index, self.edge_weight, self.n, X, self.eps, adj=self), self.W, self.delta,
                         self.theta)


# ---- the model case ---------------------------------------------------------------------------------------------------------
# hidden -> (graph seed, parameter seed, seed of the pna_weight perturbation), found by a CPU search over seeds (model_oracle's
# gap, below): max and min are not smooth, so the comparison needs every winner at least 1e-3 of the layer's largest message
# away from the best different message — in the fp64 oracle alone.  The graph is tests/test_gpu_aggr_max.py's model_graph:
# one hub destination (602 entries from 118 sources), every other row one entry (no runner-up).  That leaves hidden x 2
# extremes x 2 layers contested elements; measured, 3 - 4 % of them lie below 1e-3 at a random seed (the minimum crowds where
# ELU saturates), so at hidden 64 the search is staged: graph and parameter seeds until the first layer is clear, then the
# third seed — it moves the second layer's messages alone — until the second is.
MODEL_SEEDS = {8: (0, 4, 0), 64: (0, 11, 18)}   # smallest gaps 4.6e-3 and 1.006e-3


def model_oracle(hidden, pool, seeds=None, backward=True):
    """The fp64 oracle of the model case: OracleGLASS(aggr "sum") with conv.adj = PnaAdj whose theta is the layer's pna_weight
    (a leaf of its own: its gradient is compared too).  Returns (the product model on the CPU, loss, logits, gradients by
    the product model's parameter names, smallest relative winner / runner-up gap over both extremes and both layers, inputs)."""
    import torch.nn as nn
    from helpers import build_glass
    from oracle import glass_oracle as O
    from test_gpu_aggr_max import model_graph
    gseed, pseed, tseed = MODEL_SEEDS[hidden] if seeds is None else seeds
    N, ei, ew, x, pos, y = model_graph(gseed)
    torch.manual_seed(pseed)
    model = build_glass(hidden, 2, int(x.max()), 3, "pna", pool, 0.8, dropout=0.0, jk=True)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    theta_keys = [k for k in sd if k.endswith("pna_weight")]
    assert len(theta_keys) == 2
    # (the layers start at equal shares; the case perturbs them so that the twelve views do not enter symmetrically)
    g = torch.Generator().manual_seed(tseed)
    for k in theta_keys:
        sd[k] = sd[k] + 0.05 * torch.randn(sd[k].shape, generator=g)
    model.load_state_dict(sd)
    thetas = {k: sd[k].double().requires_grad_(True) for k in theta_keys}
    orc = O.OracleGLASS(hidden, 2, int(x.max()), 3, aggr="sum", pool=pool, z_ratio=0.8).double()
    orc.load_state_dict({k: v for k, v in sd.items() if k not in thetas})
    orc.train()
    adjs = []
    for l, conv in enumerate(orc.conv.convs):
        conv.adj = PnaAdj(ei, ew.double(), N, thetas[f"conv.convs.{l}.pna_weight"], 1e-5)
        adjs.append(conv.adj)
    logits = orc(x, ei, ew.double(), pos, O.max_zero_one(x, pos))
    loss = nn.CrossEntropyLoss()(logits, y)
    assert all(len(a.seen) == 1 for a in adjs)
    gap = min(smallest_gap(a, a.seen[0]) for a in adjs)
    if not backward:
        return model, loss.detach(), logits.detach(), None, gap, (N, ei, ew, x, pos, y)
    loss.backward()
    grads = {k: p.grad.clone() for k, p in orc.named_parameters()}
    grads.update({k: t.grad.clone() for k, t in thetas.items()})
    return model, loss.detach(), logits.detach(), grads, gap, (N, ei, ew, x, pos, y)
