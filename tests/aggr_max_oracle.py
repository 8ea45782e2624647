"""Torch restatement of max neighbour aggregation (aggr "max", K1m: glass_amd/csrc/spmm_max.hip) — a checker, CPU only.

Forward CSR as graph.CSRAdj builds it: entries sorted by (row, col), stable, duplicates kept, row = destination, values =
the raw edge weights.  Y[i, c] = max over the entries e of row i of val[e] * X[col[e], c] (one multiply in X's dtype),
arg[i, c] = the smallest such e on equal values (-0.0 == +0.0), Y = 0 / arg = -1 for a row without entries.  The backward
walks the TRANSPOSED CSR in stored order."""
import torch


def csr_from_edges(edge_index, edge_weight, n):
    """(rowptr, col, val) int64 / int64 / weight dtype: the forward CSR of an edge list (row = edge_index[0])."""
    row, col = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    perm = torch.argsort(row * n + col, stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
    return rowptr, col[perm].contiguous(), edge_weight[perm].contiguous()


def rows_of(rowptr):
    n = rowptr.shape[0] - 1
    return torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])


def transpose_csr(rowptr, col, val):
    """(rowptr_t, col_t, val_t, eid_t): the same entries keyed by (col, row), stable; col_t = destinations, eid_t[t] = the
    index of transposed entry t in the forward CSR."""
    n = rowptr.shape[0] - 1
    row = rows_of(rowptr)
    perm_t = torch.argsort(col * n + row, stable=True)
    rowptr_t = torch.zeros(n + 1, dtype=torch.int64)
    rowptr_t[1:] = torch.cumsum(torch.bincount(col, minlength=n), 0)
    return rowptr_t, row[perm_t].contiguous(), val[perm_t].contiguous(), perm_t.contiguous()


def max_aggregate(rowptr, col, val, X):
    """(Y, arg): Y in X's dtype, arg int32."""
    n, H = rowptr.shape[0] - 1, X.shape[1]
    Y = torch.zeros((n, H), dtype=X.dtype)
    arg = torch.full((n, H), -1, dtype=torch.int32)
    v = val.to(X.dtype)
    cols = torch.arange(H)
    for i in range(n):
        s, e = int(rowptr[i]), int(rowptr[i + 1])
        if e == s:
            continue
        P = v[s:e, None] * X[col[s:e]]
        k = torch.arange(e - s)[:, None].expand(e - s, H)
        first = torch.where(P == P.max(0).values, k, e - s).min(0).values  # the first maximal value (== : -0.0 ties +0.0)
        Y[i] = P[first, cols]
        arg[i] = (s + first).to(torch.int32)
    return Y, arg


def max_aggregate_bwd(rowptr_t, col_t, val_t, eid_t, dY, arg):
    """dX[j, c] = sum over the entries t of row j of the transposed CSR, in stored order, of
    (arg[col_t[t], c] == eid_t[t]) ? val_t[t] * dY[col_t[t], c] : 0, in dY's dtype."""
    n = rowptr_t.shape[0] - 1
    hit = arg[col_t].to(torch.int64) == eid_t[:, None]
    contrib = torch.where(hit, val_t.to(dY.dtype)[:, None] * dY[col_t], torch.zeros((), dtype=dY.dtype))
    return torch.zeros((n, dY.shape[1]), dtype=dY.dtype).index_add_(0, rows_of(rowptr_t), contrib)  # (in index order)


class _MaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, adj):
        Y, arg = max_aggregate(adj.rowptr, adj.col, adj.val, X)
        ctx.adj, ctx.arg = adj, arg
        adj.last_arg = arg
        return Y

    @staticmethod
    def backward(ctx, dY):
        a = ctx.adj
        return max_aggregate_bwd(a.rowptr_t, a.col_t, a.val_t, a.eid_t, dY, ctx.arg), None


class MaxAdj:
    """`MaxAdj(edge_index, edge_weight, n) @ X`: differentiable max aggregation; takes the place of OracleConv.adj (a cached
    attribute).  `seen` collects the operand of every product, for gap_report."""
    def __init__(self, edge_index, edge_weight, n):
        self.n = int(n)
        self.rowptr, self.col, self.val = csr_from_edges(edge_index, edge_weight, self.n)
        self.rowptr_t, self.col_t, self.val_t, self.eid_t = transpose_csr(self.rowptr, self.col, self.val)
        self.last_arg = None
        self.seen = []

    def __matmul__(self, X):
        self.seen.append(X.detach().clone())
        return _MaxFn.apply(X, self)


def smallest_gap(adj, X):
    """Smallest distance between the winner and the runner-up over every row with two or more entries and every channel,
    relative to the largest |val * X[col]| of the product (inf for a graph without such rows)."""
    P = adj.val.to(X.dtype)[:, None] * X[adj.col]
    best = float("inf")
    for i in range(adj.n):
        s, e = int(adj.rowptr[i]), int(adj.rowptr[i + 1])
        if e - s >= 2:
            top = torch.topk(P[s:e], 2, dim=0).values
            best = min(best, float((top[0] - top[1]).min()))
    return best / float(P.abs().max())
