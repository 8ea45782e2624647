"""Torch restatement of softmax neighbour aggregation (aggr "softmax", K1s: glass_amd/csrc/spmm_softmax.hip) — a checker,
CPU only, meant for fp64.

Forward CSR as graph.CSRAdj builds it (tests/aggr_max_oracle.py: entries sorted by (row, col), stable, duplicates kept, row =
destination, values = the raw edge weights, here > 0).  For row i, channel c, entries e, temperature t:

    s_e = t x_e     M = max_e s_e     Z = sum_e v_e exp(s_e - M)     Y = sum_e v_e exp(s_e - M) x_e / Z     L = M + log Z
    a row without entries: Y = 0, L = 0

    p_e = v_e exp(t x_e - L)
    dX[j, c] = sum over the entries of row j of the TRANSPOSED CSR (destination i) of p dY[i, c] (1 + t (X[j, c] - Y[i, c]))
    dt       = sum over i, c, e of dY[i, c] p_e x_e (x_e - Y[i, c])

`softmax_aggregate*` state these formulas; `scatter_softmax_aggregate` is the same operator written as plain differentiable
torch ops on the edge list, for autograd to differentiate."""
import torch

from aggr_max_oracle import MaxAdj, rows_of


def softmax_aggregate(rowptr, col, val, X, t):
    """(Y, L) in X's dtype; t a python float or a one-element tensor."""
    n, H = rowptr.shape[0] - 1, X.shape[1]
    t = float(t)
    rows = rows_of(rowptr)
    v = val.to(X.dtype)[:, None]
    xe = X[col]
    s = t * xe
    idx = rows[:, None].expand(-1, H)
    M = torch.zeros((n, H), dtype=X.dtype).scatter_reduce(0, idx, s, "amax", include_self=False)
    w = v * torch.exp(s - M[rows])
    Z = torch.zeros((n, H), dtype=X.dtype).index_add_(0, rows, w)
    S = torch.zeros((n, H), dtype=X.dtype).index_add_(0, rows, w * xe)
    live = (rowptr[1:] > rowptr[:-1])[:, None]
    one = torch.ones((), dtype=X.dtype)
    Y = torch.where(live, S / torch.where(live, Z, one), torch.zeros((), dtype=X.dtype))
    L = torch.where(live, M + torch.log(torch.where(live, Z, one)), torch.zeros((), dtype=X.dtype))
    return Y, L


def softmax_aggregate_bwd(rowptr_t, col_t, val_t, dY, X, Y, L, t):
    """dX, on the transposed CSR (row j = source, col_t = destination)."""
    t = float(t)
    j = rows_of(rowptr_t)
    p = val_t.to(X.dtype)[:, None] * torch.exp(t * X[j] - L[col_t])
    contrib = p * dY[col_t] * (1 + t * (X[j] - Y[col_t]))
    return torch.zeros_like(X).index_add_(0, j, contrib)


def softmax_aggregate_dt(rowptr, col, val, dY, X, Y, L, t):
    """(dt, sum of |terms|): the temperature's gradient and the size of what it cancels from."""
    t = float(t)
    i = rows_of(rowptr)
    xe = X[col]
    p = val.to(X.dtype)[:, None] * torch.exp(t * xe - L[i])
    terms = dY[i] * p * xe * (xe - Y[i])
    return terms.sum(), terms.abs().sum()


def scatter_softmax_aggregate(edge_index, edge_weight, n, X, t):
    """The same operator on the raw edge list (any order) from differentiable torch ops: X and t may require grad."""
    row, col = edge_index[0], edge_index[1]
    H = X.shape[1]
    xe = X[col]
    s = t * xe
    idx = row[:, None].expand(-1, H)
    M = torch.zeros((n, H), dtype=X.dtype).scatter_reduce(0, idx, s.detach(), "amax", include_self=False)
    w = edge_weight.to(X.dtype)[:, None] * torch.exp(s - M[row])
    Z = torch.zeros((n, H), dtype=X.dtype).index_add(0, row, w)
    S = torch.zeros((n, H), dtype=X.dtype).index_add(0, row, w * xe)
    live = (torch.bincount(row, minlength=n) > 0)[:, None]
    return torch.where(live, S / torch.where(live, Z, torch.ones((), dtype=X.dtype)), torch.zeros((), dtype=X.dtype))


class SoftmaxAdj(MaxAdj):
    """`SoftmaxAdj(edge_index, edge_weight, n, t) @ X`: differentiable softmax aggregation in the dtype of X; takes the place of
    OracleConv.adj.  `t` is a one-element tensor that may require grad (the layer's temperature)."""
    def __init__(self, edge_index, edge_weight, n, t):
        super().__init__(edge_index, edge_weight, n)
        self.edge_index, self.edge_weight, self.t = edge_index, edge_weight, t

    def __matmul__(self, X):
        return scatter_softmax_aggregate(self.edge_index, self.edge_weight, self.n, X, self.t.to(X.dtype))
