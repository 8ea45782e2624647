"""Torch restatement of attention neighbour aggregation (aggr "gat", K1a: glass_amd/csrc/spmm_gat.hip; single-head GAT) — a
checker, CPU only, meant for fp64.

Forward CSR as graph.CSRAdj builds it (tests/aggr_max_oracle.py: entries sorted by (row, col), stable, duplicates kept, row =
destination, values = the raw edge weights, here > 0).  For destination i and entry e of row i, source j = col[e], weight v_e:

    a_j = sum_c X[j,c] att_src[c]        b_i = sum_c X[i,c] att_dst[c]
    u_e = a_j + b_i                      s_e = u_e > 0 ? u_e : slope * u_e
    M_i = max_e s_e     Z_i = sum_e v_e exp(s_e - M_i)
    Y[i,:] = sum_e v_e exp(s_e - M_i) X[j,:] / Z_i          L_i = M_i + log Z_i
    a row without entries: Y[i,:] = 0, L_i = 0

    p_e = v_e exp(s_e - L_i)             f_e = u_e > 0 ? 1 : slope   (torch's leaky_relu rule: u_e == 0 takes slope)
    D_i = sum_c dY[i,c] Y[i,c]           q_e = sum_c dY[i,c] X[j,c]          g_e = p_e (q_e - D_i) f_e
    da_j = sum over entries with col = j of g_e        db_i = sum over entries of row i of g_e
    dX[j,:] = sum over entries with col = j of p_e dY[i,:]  +  da_j att_src  +  db_j att_dst
    d att_src[c] = sum_j da_j X[j,c]                   d att_dst[c] = sum_i db_i X[i,c]

g, da, db and the two vector gradients cancel; each comes with its MASS, the sum of the absolute values of its terms:
p_e (sum_c |dY X| + sum_c |dY Y|) |f_e| per entry, summed the same way as the quantity (the vector gradients: times |X|).

`gat_aggregate*` state these formulas; `scatter_gat_aggregate` is the same operator written as plain differentiable torch ops
on the raw edge list, for autograd to differentiate."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from aggr_max_oracle import MaxAdj, rows_of


def gat_aggregate(rowptr, col, val, X, att_src, att_dst, slope):
    """(Y, L, a, b) in X's dtype: Y [n, H], L, a, b [n]."""
    n, H = rowptr.shape[0] - 1, X.shape[1]
    rows = rows_of(rowptr)
    a, b = X @ att_src.to(X.dtype), X @ att_dst.to(X.dtype)
    u = a[col] + b[rows]
    s = torch.where(u > 0, u, slope * u)
    M = torch.zeros(n, dtype=X.dtype).scatter_reduce(0, rows, s, "amax", include_self=False)
    w = val.to(X.dtype) * torch.exp(s - M[rows])
    Z = torch.zeros(n, dtype=X.dtype).index_add_(0, rows, w)
    S = torch.zeros((n, H), dtype=X.dtype).index_add_(0, rows, w[:, None] * X[col])
    live = rowptr[1:] > rowptr[:-1]
    one = torch.ones((), dtype=X.dtype)
    Zs = torch.where(live, Z, one)
    Y = torch.where(live[:, None], S / Zs[:, None], torch.zeros((), dtype=X.dtype))
    L = torch.where(live, M + torch.log(Zs), torch.zeros((), dtype=X.dtype))
    return Y, L, a, b


def gat_aggregate_bwd(rowptr, col, val, dY, X, Y, L, a, b, att_src, att_dst, slope):
    """The backward from the forward's operands and results.  Returns a namespace: dX [n, H], g [nnz] (forward entry order),
    da, db [n], datt_src, datt_dst [H], and mass_g, mass_da, mass_db, mass_datt_src, mass_datt_dst of the same shapes."""
    n = rowptr.shape[0] - 1
    rows = rows_of(rowptr)
    dt = X.dtype
    att_src, att_dst = att_src.to(dt), att_dst.to(dt)
    u = a[col] + b[rows]
    s = torch.where(u > 0, u, slope * u)
    f = torch.where(u > 0, torch.ones((), dtype=dt), torch.full((), float(slope), dtype=dt))
    p = val.to(dt) * torch.exp(s - L[rows])
    D = (dY * Y).sum(1)
    q = (dY[rows] * X[col]).sum(1)
    g = p * (q - D[rows]) * f
    mass_g = p * ((dY[rows] * X[col]).abs().sum(1) + (dY * Y).abs().sum(1)[rows]) * f.abs()
    zero = lambda: torch.zeros(n, dtype=dt)
    da, db = zero().index_add_(0, col, g), zero().index_add_(0, rows, g)
    mass_da, mass_db = zero().index_add_(0, col, mass_g), zero().index_add_(0, rows, mass_g)
    dX = torch.zeros_like(X).index_add_(0, col, p[:, None] * dY[rows]) + da[:, None] * att_src + db[:, None] * att_dst
    return SimpleNamespace(dX=dX, g=g, da=da, db=db, datt_src=da @ X, datt_dst=db @ X, p=p, mass_g=mass_g, mass_da=mass_da,
                           mass_db=mass_db, mass_datt_src=mass_da @ X.abs(), mass_datt_dst=mass_db @ X.abs())


def scatter_gat_aggregate(edge_index, edge_weight, n, X, att_src, att_dst, slope):
    """The same operator on the raw edge list (any order) from differentiable torch ops: X and the vectors may require grad."""
    row, col = edge_index[0], edge_index[1]
    H = X.shape[1]
    a, b = X @ att_src, X @ att_dst
    s = F.leaky_relu(a[col] + b[row], float(slope))
    M = torch.zeros(n, dtype=X.dtype).scatter_reduce(0, row, s.detach(), "amax", include_self=False)
    w = edge_weight.to(X.dtype) * torch.exp(s - M[row])
    Z = torch.zeros(n, dtype=X.dtype).index_add(0, row, w)
    S = torch.zeros((n, H), dtype=X.dtype).index_add(0, row, w[:, None] * X[col])
    live = (torch.bincount(row, minlength=n) > 0)[:, None]
    return torch.where(live, S / torch.where(live, Z[:, None], torch.ones((), dtype=X.dtype)), torch.zeros((), dtype=X.dtype))


class GatAdj(MaxAdj):
    """`GatAdj(edge_index, edge_weight, n, att_src, att_dst, slope) @ X`: differentiable attention aggregation in the dtype of X;
    takes the place of OracleConv.adj.  The vectors are tensors that may require grad (the layer's parameters)."""
    def __init__(self, edge_index, edge_weight, n, att_src, att_dst, slope=0.2):
        super().__init__(edge_index, edge_weight, n)
        self.edge_index, self.edge_weight = edge_index, edge_weight
        self.att_src, self.att_dst, self.slope = att_src, att_dst, float(slope)

    def __matmul__(self, X):
        return scatter_gat_aggregate(self.edge_index, self.edge_weight, self.n, X, self.att_src.to(X.dtype),
                                     self.att_dst.to(X.dtype), self.slope)
