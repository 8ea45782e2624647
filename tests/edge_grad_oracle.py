"""fp64 restatement of K1w (csrc/spmm_edge.hip): the gradient of Y = A(w) X with respect to the edge weights w for the
aggregations "sum", "mean" and "gcn", on a sorted CSR — a checker, CPU only, numpy.

Entry e of row i (the destination) has column j = col[e] (the source).  d_i = the row sum of w, d~_i = d_i + 1 where d_i < 0.5
(K2's rule, derivative 1), r = d~^(-1/2), val = w (sum), w / d~_i (mean), r_i w r_j (gcn).  With G = dL/dY:

  dval[e] = sum_c G[i,c] X[j,c]        R[i] = sum over row i of dval val        C[k] = sum over the entries with column k of dval val
  sum: dw = dval      mean: dw = (dval - R[i]) / d~_i      gcn: dw = r_i r_j dval - (R[i] + C[i]) / (2 d~_i)

tests/test_edge_grad_host.py checks these against torch autograd in fp64.  Beside every value the functions return its MASS, the
sum of the absolute values of the terms it adds up: the rounding bounds of the GPU test are multiples of it."""
import functools

import numpy as np

AGGRS = ("sum", "mean", "gcn")


# ---- the graphs (the generator of tests/test_gpu_aggr_gat.py, with low-degree rows and a pure source added) -------------------
def _edges(degrees, n, rng, hub_share, hub_frac=0.0):
    """One destination row per entry of `degrees`; sources uniform, except that a share of the rows also names source 5, and a
    fraction of all entries (a hub: its row of the TRANSPOSED matrix is long and cut).  Not symmetric.  Weights in [0.25, 2)."""
    rows, cols = [], []
    for r, d in enumerate(degrees):
        c = rng.integers(0, n, d)
        if d and rng.random() < hub_share:
            c[rng.integers(0, d)] = 5
        rows.append(np.full(d, r))
        cols.append(c)
    row, col = np.concatenate(rows), np.concatenate(cols)
    col[rng.random(col.shape[0]) < hub_frac] = 5
    w = rng.uniform(0.25, 2.0, row.shape[0]).astype(np.float32)
    return row, col, w


N_LOW = 5  # rows with one entry of weight in [0.25, 0.45]: their weight sum is below 0.5 and takes the + 1


@functools.lru_cache(maxsize=None)
def graph(kind):
    """-> (n, edge_index int64 [2, E], edge_weight fp32 [E]) as numpy, in SHUFFLED edge order.
    mixed: rows of 0, 1, 2, 63, 64, 65, 255, 256, 257 and 700 in-entries (both sides of the long-row threshold, 257 and 700 are
      cut, 700 into three chunks), then 997 short rows of 1..12 (sweep items), a duplicate (row, col) pair with different
      weights, a self-loop; source 5 is a hub, so its row of the transposed matrix is cut.
    all_long: 40 rows of 64..300 entries, one of 700, one empty — fewer than 1 024 rows, nnz >= 64 n: no sweep at all.
    Both then get N_LOW more rows of one light entry each, and a last node that is a source (of two entries) and never a
    destination."""
    rng = np.random.Generator(np.random.PCG64(17 if kind == "mixed" else 18))
    if kind == "mixed":
        degrees = [0, 1, 2, 63, 64, 65, 255, 256, 257, 700] + list(rng.integers(1, 13, 997))
        n = len(degrees)
        row, col, w = _edges(degrees, n, rng, 0.7)
        extra_r, extra_c = np.array([20, 20, 30]), np.array([40, 40, 30])      # (20, 40) twice; self-loop (30, 30)
        extra_w = np.array([0.5, 1.25, 0.75], dtype=np.float32)
        row, col, w = np.concatenate((row, extra_r)), np.concatenate((col, extra_c)), np.concatenate((w, extra_w))
    else:
        degrees = list(rng.integers(64, 301, 38)) + [700, 0] + [200, 200]
        n = len(degrees)
        row, col, w = _edges(degrees, n, rng, 0.0, 0.2)
    low_r = np.arange(n, n + N_LOW)
    low_c = rng.integers(0, n, N_LOW)
    low_w = rng.uniform(0.25, 0.45, N_LOW).astype(np.float32)
    src = n + N_LOW                                                            # the pure source: column of two more entries of row 12
    row = np.concatenate((row, low_r, [12, 12]))
    col = np.concatenate((col, low_c, [src, src]))
    w = np.concatenate((w, low_w, np.array([0.6, 1.5], dtype=np.float32)))
    n = src + 1
    # the + 1 rule is discontinuous at a weight sum of 0.5: a row that lands within 0.01 of it gets 0.05 more on its first entry
    d = np.bincount(row, weights=w.astype(np.float64), minlength=n)
    for r in np.nonzero(np.abs(d - 0.5) < 1e-2)[0]:
        w[np.nonzero(row == r)[0][0]] += np.float32(0.05)
    perm = rng.permutation(row.shape[0])
    return n, np.stack((row[perm], col[perm])).astype(np.int64), w[perm].copy()


def pair_positions(ei):
    """caller positions of the two (20, 40) entries of `mixed`"""
    return np.nonzero((ei[0] == 20) & (ei[1] == 40))[0]


# ---- sorted CSR ------------------------------------------------------------------------------------------------------------
class SortedCSR:
    """graph.CSRAdj's index arrays from a caller-order edge list: perm (entry e is the caller's edge perm[e]), rowptr, row, col,
    and the transpose's rowptr_t, col_t, eid_t (transposed entry t is forward entry eid_t[t])."""
    def __init__(self, ei, n):
        ei = np.asarray(ei, dtype=np.int64)
        self.n = int(n)
        self.perm = np.argsort(ei[0] * self.n + ei[1], kind="stable")
        self.row, self.col = ei[0][self.perm], ei[1][self.perm]
        self.rowptr = np.concatenate(([0], np.cumsum(np.bincount(self.row, minlength=self.n)))).astype(np.int64)
        self.eid_t = np.argsort(self.col * self.n + self.row, kind="stable")
        self.col_t = self.row[self.eid_t]
        self.rowptr_t = np.concatenate(([0], np.cumsum(np.bincount(self.col, minlength=self.n)))).astype(np.int64)
        self.nnz = int(self.row.shape[0])


def degrees(csr, w):
    """(d, d~) of the caller-order weights w, fp64"""
    ws = np.asarray(w, dtype=np.float64)[csr.perm]
    d = np.bincount(csr.row, weights=ws, minlength=csr.n)
    return d, np.where(d < 0.5, d + 1.0, d)


def values(csr, w, aggr):
    """val [nnz] in forward entry order (fp64) of the caller-order weights w"""
    ws = np.asarray(w, dtype=np.float64)[csr.perm]
    _d, dt = degrees(csr, w)
    if aggr == "sum":
        return ws
    if aggr == "mean":
        return ws / dt[csr.row]
    if aggr == "gcn":
        r = dt ** -0.5
        return r[csr.row] * ws * r[csr.col]
    raise NotImplementedError(aggr)


def dval_R(csr, X, G, val):
    """(dval, mass of dval, R, mass of R): dval[e] = G[row] . X[col]; its mass sum_c |G X|; R[i] = sum dval val over row i; its
    mass sum |val| (mass of dval)."""
    X, G, val = (np.asarray(a, dtype=np.float64) for a in (X, G, val))
    prod = G[csr.row] * X[csr.col]
    dval, m_dval = prod.sum(1), np.abs(prod).sum(1)
    R = np.bincount(csr.row, weights=dval * val, minlength=csr.n)
    m_R = np.bincount(csr.row, weights=m_dval * np.abs(val), minlength=csr.n)
    return dval, m_dval, R, m_R


def colsum(csr, dval, val, m_dval=None):
    """(C, mass of C): C[k] = sum over the entries with column k of dval val; mass from |dval| (or the given masses of dval)"""
    dval, val = np.asarray(dval, dtype=np.float64), np.asarray(val, dtype=np.float64)
    m = np.abs(dval) if m_dval is None else m_dval
    return (np.bincount(csr.col, weights=dval * val, minlength=csr.n),
            np.bincount(csr.col, weights=m * np.abs(val), minlength=csr.n))


def values_bwd(csr, w, aggr, dval, R=None, C=None, m_dval=None, m_R=None, m_C=None):
    """(dw, mass) in the CALLER's edge order from the entry gradients dval (forward entry order) and their sums R, C.  mass: the
    sum of the absolute values of the terms of the formula, scaled as the formula scales them — from the masses of dval, R and
    C where they are given (what the rounding of a computed dval, R, C is proportional to), else from their absolute values."""
    dval = np.asarray(dval, dtype=np.float64)
    _d, dt = degrees(csr, w)
    i, j = csr.row, csr.col
    md = np.abs(dval) if m_dval is None else m_dval
    if aggr == "sum":
        g, m = dval, md
    elif aggr == "mean":
        R = np.asarray(R, dtype=np.float64)
        mr = np.abs(R) if m_R is None else m_R
        g, m = (dval - R[i]) / dt[i], (md + mr[i]) / dt[i]
    elif aggr == "gcn":
        R, C = np.asarray(R, dtype=np.float64), np.asarray(C, dtype=np.float64)
        mr, mc = np.abs(R) if m_R is None else m_R, np.abs(C) if m_C is None else m_C
        r = dt ** -0.5
        g = r[i] * r[j] * dval - (R[i] + C[i]) / (2.0 * dt[i])
        m = r[i] * r[j] * md + (mr[i] + mc[i]) / (2.0 * dt[i])
    else:
        raise NotImplementedError(aggr)
    dw, mass = np.empty(csr.nnz), np.empty(csr.nnz)
    dw[csr.perm], mass[csr.perm] = g, m
    return dw, mass


def edge_grad(csr, w, aggr, X, G):
    """dw [E] (caller order, fp64) of sum(A(w) X * G): the three passes one after the other"""
    val = values(csr, w, aggr)
    dval, _m, R, _mr = dval_R(csr, X, G, val)
    C = colsum(csr, dval, val)[0] if aggr == "gcn" else None
    return values_bwd(csr, w, aggr, dval, R, C)[0]
