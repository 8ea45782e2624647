"""Torch restatement of multi-head attention neighbour aggregation (aggr "gat" with gat_heads = K, K1a multi-head:
glass_amd/csrc/spmm_gat_mh.hip) — a checker, CPU only, meant for fp64.

K heads partition the H channels: head h owns columns [h D, (h + 1) D), D = H / K.  The operator is block-diagonal, so
`gat_mh_aggregate*` ARE the single-head restatement (tests/aggr_gat_oracle.py) on the column slices, concatenated: a, b, L, da,
db come out [n, K], g [nnz, K] (forward entry order), every mass per head.  `scatter_gat_mh_aggregate` states the formulas
directly — [n, K] scores from a reshape, one softmax per destination and head on the raw edge list — in differentiable torch,
without slicing: the independent statement the sliced one is checked against (tests/test_aggr_gat_mh_host.py)."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import aggr_gat_oracle as GO
from aggr_max_oracle import MaxAdj


def _slices(H, K):
    assert H % K == 0, (H, K)
    D = H // K
    return [slice(h * D, (h + 1) * D) for h in range(K)]


def gat_mh_aggregate(rowptr, col, val, X, att_src, att_dst, slope, K):
    """(Y, L, a, b) in X's dtype: Y [n, H]; L, a, b [n, K]."""
    parts = [GO.gat_aggregate(rowptr, col, val, X[:, s], att_src[s], att_dst[s], slope) for s in _slices(X.shape[1], K)]
    return (torch.cat([p[0] for p in parts], 1), ) + tuple(torch.stack([p[i] for p in parts], 1) for i in (1, 2, 3))


def gat_mh_aggregate_bwd(rowptr, col, val, dY, X, Y, L, a, b, att_src, att_dst, slope, K):
    """The backward from the forward's operands and results.  Returns a namespace: dX [n, H]; g, p [nnz, K]; da, db [n, K];
    datt_src, datt_dst [H]; mass_g, mass_da, mass_db, mass_datt_src, mass_datt_dst of the same shapes (per head)."""
    parts = [GO.gat_aggregate_bwd(rowptr, col, val, dY[:, s], X[:, s], Y[:, s], L[:, h], a[:, h], b[:, h], att_src[s], att_dst[s],
                                  slope) for h, s in enumerate(_slices(X.shape[1], K))]
    cat = lambda name: torch.cat([getattr(p, name) for p in parts], -1)
    stack = lambda name: torch.stack([getattr(p, name) for p in parts], 1)
    return SimpleNamespace(dX=cat("dX"), datt_src=cat("datt_src"), datt_dst=cat("datt_dst"), mass_datt_src=cat("mass_datt_src"),
                           mass_datt_dst=cat("mass_datt_dst"),
                           **{name: stack(name) for name in ("g", "da", "db", "p", "mass_g", "mass_da", "mass_db")})


def scatter_gat_mh_aggregate(edge_index, edge_weight, n, X, att_src, att_dst, slope, K):
    """The operator on the raw edge list (any order) from differentiable torch ops, every head at once: X and the vectors may
    require grad."""
    row, col = edge_index[0], edge_index[1]
    H = X.shape[1]
    D = H // K
    assert K * D == H
    Xh = X.reshape(n, K, D)
    a = (Xh * att_src.reshape(1, K, D)).sum(2)   # [n, K]
    b = (Xh * att_dst.reshape(1, K, D)).sum(2)
    s = F.leaky_relu(a[col] + b[row], float(slope))   # [E, K]
    idx = row[:, None].expand(-1, K)
    M = torch.zeros((n, K), dtype=X.dtype).scatter_reduce(0, idx, s.detach(), "amax", include_self=False)
    w = edge_weight.to(X.dtype)[:, None] * torch.exp(s - M[row])   # [E, K]
    Z = torch.zeros((n, K), dtype=X.dtype).index_add(0, row, w)
    S = torch.zeros((n, K, D), dtype=X.dtype).index_add(0, row, w[:, :, None] * Xh[col])
    live = (torch.bincount(row, minlength=n) > 0)[:, None, None]
    Zs = torch.where(live, Z[:, :, None], torch.ones((), dtype=X.dtype))
    return torch.where(live, S / Zs, torch.zeros((), dtype=X.dtype)).reshape(n, H)


class GatMHAdj(MaxAdj):
    """`GatMHAdj(edge_index, edge_weight, n, att_src, att_dst, slope, K) @ X`: differentiable K-head attention aggregation in
    the dtype of X; takes the place of OracleConv.adj, as aggr_gat_oracle.GatAdj does for one head."""
    def __init__(self, edge_index, edge_weight, n, att_src, att_dst, slope=0.2, heads=1):
        super().__init__(edge_index, edge_weight, n)
        self.edge_index, self.edge_weight = edge_index, edge_weight
        self.att_src, self.att_dst, self.slope, self.heads = att_src, att_dst, float(slope), int(heads)

    def __matmul__(self, X):
        return scatter_gat_mh_aggregate(self.edge_index, self.edge_weight, self.n, X, self.att_src.to(X.dtype),
                                        self.att_dst.to(X.dtype), self.slope, self.heads)
