"""Numpy restatement of standard-deviation / variance neighbour aggregation (aggr "std" / "var", K1v:
glass_amd/csrc/spmm_moment.hip) — a checker, CPU only, meant for fp64 — with the per-element masses its error bounds are
stated in, fp32 restatements of the kernel's merge (Chan's update) in two orders, the plain E[x^2] - Mu^2 form in fp32, and a
differentiable torch formulation for autograd to differentiate.

Forward CSR as graph.CSRAdj builds it (tests/aggr_max_oracle.py: entries sorted by (row, col), stable, duplicates kept, row =
destination, values = the raw edge weights, here > 0).  For row i, channel c, entries e (source j_e, weight w_e):

    W = sum_e w_e     Mu = sum_e w_e x_e / W     Var = sum_e w_e (x_e - Mu)^2 / W     Std = sqrt(Var + eps)
    a row without entries: W = Mu = Var = Std = 0

    backward, on the TRANSPOSED CSR (row j = source, entries = destinations i, val_t), with per-destination factors
    std: A = dS / (W S)     var: A = 2 dS / W     C = dMu / W     (0 where W = 0)
    dX[j, c] = sum_e val_t[e] (C[i, c] + A[i, c] (X[j, c] - Mu[i, c]))"""
import numpy as np
import torch

from aggr_max_oracle import MaxAdj

U32 = 2.0 ** -24


def gamma(n):
    """n rounded fp32 operations in a row: n u / (1 - n u)"""
    n = np.asarray(n, dtype=np.float64)
    return n * U32 / (1 - n * U32)


def rows_of(rowptr):
    rowptr = np.asarray(rowptr)
    return np.repeat(np.arange(rowptr.shape[0] - 1), np.diff(rowptr))


def segsum(a, rowptr):
    """sums of a's rows over the segments of rowptr -> [n, ...]; zeros for an empty segment"""
    rowptr = np.asarray(rowptr)
    out = np.zeros((rowptr.shape[0] - 1, ) + a.shape[1:], dtype=a.dtype)
    live = rowptr[1:] > rowptr[:-1]
    if live.any():
        out[live] = np.add.reduceat(a, rowptr[:-1][live], axis=0)
    return out


def moments(rowptr, col, val, X, eps=1e-5):
    """fp64, two passes -> dict with W [n], cnt [n], Mu, Var, Std [n, H] and the masses abs_x = sum w |x| / W and
    sq_x = sum w x^2 / W ([n, H], zeros for a row without entries)."""
    rowptr, col = np.asarray(rowptr), np.asarray(col)
    val, X = np.asarray(val, dtype=np.float64), np.asarray(X, dtype=np.float64)
    rows = rows_of(rowptr)
    w, xe = val[:, None], X[col]
    W = segsum(val, rowptr)
    live = W > 0
    Wd = np.where(live, W, 1.0)[:, None]
    Mu = segsum(w * xe, rowptr) / Wd
    dev = xe - Mu[rows]
    Var = segsum(w * dev * dev, rowptr) / Wd
    Std = np.where(live[:, None], np.sqrt(Var + eps), 0.0)
    return {"W": W, "cnt": np.diff(rowptr), "Mu": Mu, "Var": Var, "Std": Std,
            "abs_x": segsum(w * np.abs(xe), rowptr) / Wd, "sq_x": segsum(w * xe * xe, rowptr) / Wd}


def bounds(m):
    """The per-element error bounds of the fp32 forward against `moments`' fp64 result m, n the row's entry count:
    W: gamma(n) W;  Mu: gamma(3 n + 4) sum w |x| / W;  Var: gamma(8 n + 8) (Var + sqrt(Var sum w x^2 / W)) — eight rounded
    operations per merge, the second mass the first-order condition term of Welford's update;  Std: the Var bound divided by
    2 Std, plus one fp32 ulp of Std."""
    n = m["cnt"].astype(np.float64)
    bvar = gamma(8 * n + 8)[:, None] * (m["Var"] + np.sqrt(m["Var"] * m["sq_x"]))
    std = m["Std"]
    ulp = np.spacing(std.astype(np.float32)).astype(np.float64)
    bstd = np.where(std > 0, bvar / (2 * np.where(std > 0, std, 1.0)) + ulp, 0.0)
    return {"W": gamma(n) * m["W"], "Mu": gamma(3 * n + 4)[:, None] * m["abs_x"], "Var": bvar, "Std": bstd}


def factors(kind, S, W, dS, dMu=None):
    """(A, C) in fp64; C is None without dMu"""
    S, W, dS = (np.asarray(a, dtype=np.float64) for a in (S, W, dS))
    live = (W > 0)[:, None]
    Wd = np.where(W > 0, W, 1.0)[:, None]
    if kind == "std":
        A = np.where(live, dS / np.where(live, Wd * S, 1.0), 0.0)
    else:
        A = np.where(live, 2 * dS / Wd, 0.0)
    C = None if dMu is None else np.where(live, np.asarray(dMu, dtype=np.float64) / Wd, 0.0)
    return A, C


def moments_bwd(rowptr_t, col_t, val_t, X, Mu, A, C=None):
    """(dX, mass) in fp64 on the transposed CSR: mass[j, c] = sum_e val_t (|C| + |A| |X - Mu|)"""
    rowptr_t, col_t = np.asarray(rowptr_t), np.asarray(col_t)
    val_t, X, Mu, A = (np.asarray(a, dtype=np.float64) for a in (val_t, X, Mu, A))
    j = rows_of(rowptr_t)
    d = X[j] - Mu[col_t]
    w = val_t[:, None]
    term, mass = A[col_t] * d, np.abs(A[col_t]) * np.abs(d)
    if C is not None:
        C = np.asarray(C, dtype=np.float64)
        term, mass = term + C[col_t], mass + np.abs(C[col_t])
    return segsum(w * term, rowptr_t), segsum(w * mass, rowptr_t)


def bound_dx(rowptr_t, mass):
    """gamma(n_j + 6) mass, n_j the transposed row's entry count"""
    return gamma(np.diff(np.asarray(rowptr_t)).astype(np.float64) + 6)[:, None] * mass


# ---- the kernel's arithmetic in fp32, element-wise over arrays: Chan's update in two merge orders, and the plain form --------
_f = np.float32


def chan_merge(a, b):
    """(W, m, M2) of two partials, fp32 arrays of one shape, every operation rounded once; an empty side is the identity"""
    Wa, ma, Qa = a
    Wb, mb, Qb = b
    W = (Wa + Wb).astype(_f)
    f = np.where(W > 0, Wb / np.where(W > 0, W, _f(1)), _f(0)).astype(_f)
    d = (mb - ma).astype(_f)
    m = (ma + (d * f).astype(_f)).astype(_f)
    Q = ((Qa + Qb).astype(_f) + ((d * d).astype(_f) * (Wa * f).astype(_f)).astype(_f)).astype(_f)
    return W, m, Q


def _items(w, x):
    w, x = np.asarray(w, dtype=_f), np.asarray(x, dtype=_f)
    return [(w[k], x[k], np.zeros_like(x[k])) for k in range(x.shape[0])]


def chan_sequential(w, x):
    """w, x fp32 [n, ...]: entry after entry -> (W, m, M2)"""
    items = _items(w, x)
    acc = items[0]
    for it in items[1:]:
        acc = chan_merge(acc, it)
    return acc


def chan_pairwise(w, x):
    """the same entries merged as a binary tree"""
    items = _items(w, x)
    while len(items) > 1:
        items = [chan_merge(items[k], items[k + 1]) if k + 1 < len(items) else items[k] for k in range(0, len(items), 2)]
    return items[0]


def plain_variance(w, x):
    """E[x^2] - Mu^2 with fp32 running sums: what two products give"""
    w, x = np.asarray(w, dtype=_f), np.asarray(x, dtype=_f)
    s0, s1, s2 = (np.zeros_like(x[0]) for _ in range(3))
    for k in range(x.shape[0]):
        wx = (w[k] * x[k]).astype(_f)
        s0, s1, s2 = (s0 + w[k]).astype(_f), (s1 + wx).astype(_f), (s2 + (wx * x[k]).astype(_f)).astype(_f)
    mu = (s1 / s0).astype(_f)
    return ((s2 / s0).astype(_f) - (mu * mu).astype(_f)).astype(_f)


# ---- the same operator from differentiable torch ops ----------------------------------------------------------------------
def dense_moments(edge_index, edge_weight, n, X, kind, eps=1e-5):
    """(S, Mu) through the dense [n, n] multiplicity matrix (duplicates add up) and an [n, n, H] broadcast: for small n"""
    Wd = torch.zeros((n, n), dtype=X.dtype).index_put((edge_index[0], edge_index[1]), edge_weight.to(X.dtype), accumulate=True)
    W = Wd.sum(1)
    live = (W > 0)[:, None]
    Ws = torch.where(W > 0, W, torch.ones((), dtype=X.dtype))[:, None]
    Mu = (Wd @ X) / Ws
    dev = X[None, :, :] - Mu[:, None, :]
    Var = (Wd[:, :, None] * dev * dev).sum(1) / Ws
    zero = torch.zeros((), dtype=X.dtype)
    S = torch.sqrt(Var + eps) if kind == "std" else Var
    return torch.where(live, S, zero), torch.where(live, Mu, zero)


def scatter_moments(edge_index, edge_weight, n, X, kind, eps=1e-5):
    """(S, Mu) on the raw edge list (any order) from differentiable torch ops, two passes"""
    row, col = edge_index[0], edge_index[1]
    w = edge_weight.to(X.dtype)
    W = torch.zeros(n, dtype=X.dtype).index_add(0, row, w)
    live = (W > 0)[:, None]
    Ws = torch.where(W > 0, W, torch.ones((), dtype=X.dtype))[:, None]
    xe = X[col]
    Mu = torch.zeros((n, X.shape[1]), dtype=X.dtype).index_add(0, row, w[:, None] * xe) / Ws
    dev = xe - Mu[row]
    Var = torch.zeros((n, X.shape[1]), dtype=X.dtype).index_add(0, row, w[:, None] * dev * dev) / Ws
    zero = torch.zeros((), dtype=X.dtype)
    S = torch.sqrt(Var + eps) if kind == "std" else Var
    return torch.where(live, S, zero), torch.where(live, Mu, zero)


class MomentAdj(MaxAdj):
    """`MomentAdj(edge_index, edge_weight, n, kind, eps) @ X`: the differentiable std / var aggregation in the dtype of X;
    takes the place of OracleConv.adj."""
    def __init__(self, edge_index, edge_weight, n, kind, eps=1e-5):
        super().__init__(edge_index, edge_weight, n)
        self.edge_index, self.edge_weight, self.kind, self.eps = edge_index, edge_weight, kind, eps

    def __matmul__(self, X):
        return scatter_moments(self.edge_index, self.edge_weight, self.n, X, self.kind, self.eps)[0]
