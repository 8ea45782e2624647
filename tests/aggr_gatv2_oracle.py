"""Restatement of dynamic attention neighbour aggregation (aggr "gatv2", K1a2: glass_amd/csrc/spmm_gatv2.hip; single-head GATv2)
— a checker, CPU only.

Forward CSR as graph.CSRAdj builds it (tests/aggr_max_oracle.py: entries sorted by (row, col), stable, duplicates kept, row =
destination, values = the raw edge weights, here > 0).  For destination i and entry e of row i, source j = col[e], weight v_e:

    u_ec = X[i,c] + X[j,c]               r_ec = u_ec > 0 ? u_ec : slope * u_ec          s_e = sum_c att[c] r_ec
    M_i = max_e s_e     Z_i = sum_e v_e exp(s_e - M_i)
    Y[i,:] = sum_e v_e exp(s_e - M_i) X[j,:] / Z_i          L_i = M_i + log Z_i
    a row without entries: Y[i,:] = 0, L_i = 0

    p_e = v_e exp(s_e - L_i)             f_ec = u_ec > 0 ? 1 : slope   (torch's leaky_relu rule: u == 0 takes slope)
    D_i = sum_c dY[i,c] Y[i,c]           q_e = sum_c dY[i,c] X[j,c]          g_e = p_e (q_e - D_i)
    Gd[i,c] = sum over entries of row i of g_e att[c] f_ec          R[i,c] = sum over entries of row i of g_e r_ec
    dX[j,c] = sum over entries with col = j of ( p_e dY[i,c] + g_e att[c] f_ec )  +  Gd[j,c]
    d att[c] = sum_i R[i,c]

`gatv2_aggregate*` state these formulas in numpy fp64.  s, g, Gd, R and d att cancel; each comes with its MASS, the sum of the
absolute values of its terms: sum_c |att[c] r_ec| for s; p_e (sum_c |dY X| + sum_c |dY Y|) for g, and that mass summed the same
way as the quantity, times |att[c] f_ec| or |r_ec|, for Gd, R and d att.

`gatv2_fp32` is the same operator in fp32 in the kernels' summation order, for a bound on what fp32 alone costs.
`scatter_gatv2_aggregate` / `GatV2Adj` write it as plain differentiable torch ops on the raw edge list, for autograd."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from aggr_max_oracle import MaxAdj


def _np(a, dtype=np.float64):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).astype(dtype)


def rows_of(rowptr):
    rp = _np(rowptr, np.int64)
    return np.repeat(np.arange(rp.shape[0] - 1), rp[1:] - rp[:-1])


def _row_sum(rows, terms, n):
    out = np.zeros((n, ) + terms.shape[1:], dtype=terms.dtype)
    np.add.at(out, rows, terms)
    return out


def gatv2_aggregate(rowptr, col, val, X, att, slope):
    """(Y [n, H], L [n], s [nnz], mass_s [nnz]) in fp64."""
    rp, col, val, X, att = _np(rowptr, np.int64), _np(col, np.int64), _np(val), _np(X), _np(att)
    n, rows = rp.shape[0] - 1, rows_of(rp)
    u = X[rows] + X[col]
    r = np.where(u > 0, u, slope * u)
    s, mass_s = r @ att, np.abs(r) @ np.abs(att)
    M = np.full(n, -np.inf)
    np.maximum.at(M, rows, s)
    live = rp[1:] > rp[:-1]
    M = np.where(live, M, 0.0)
    w = val * np.exp(s - M[rows])
    Z = _row_sum(rows, w, n)
    S = _row_sum(rows, w[:, None] * X[col], n)
    Zs = np.where(live, Z, 1.0)
    return np.where(live[:, None], S / Zs[:, None], 0.0), np.where(live, M + np.log(Zs), 0.0), s, mass_s


def gatv2_aggregate_bwd(rowptr, col, val, dY, X, Y, L, s, att, slope):
    """The backward from the forward's operands and results (fp64).  Returns a namespace: dX [n, H], p, g [nnz] (forward entry
    order), Gd, R [n, H], datt [H], and mass_g, mass_Gd, mass_R, mass_datt of the same shapes."""
    rp, col, val, att = _np(rowptr, np.int64), _np(col, np.int64), _np(val), _np(att)
    dY, X, Y, L, s = _np(dY), _np(X), _np(Y), _np(L), _np(s)
    n, rows = rp.shape[0] - 1, rows_of(rp)
    u = X[rows] + X[col]
    r = np.where(u > 0, u, slope * u)
    f = np.where(u > 0, 1.0, float(slope))
    p = val * np.exp(s - L[rows])
    D = (dY * Y).sum(1)
    g = p * ((dY[rows] * X[col]).sum(1) - D[rows])
    mass_g = p * (np.abs(dY[rows] * X[col]).sum(1) + np.abs(dY * Y).sum(1)[rows])
    af = att[None, :] * f
    Gd, mass_Gd = _row_sum(rows, g[:, None] * af, n), _row_sum(rows, mass_g[:, None] * np.abs(af), n)
    R, mass_R = _row_sum(rows, g[:, None] * r, n), _row_sum(rows, mass_g[:, None] * np.abs(r), n)
    dX = _row_sum(col, p[:, None] * dY[rows] + g[:, None] * af, n) + Gd
    return SimpleNamespace(dX=dX, p=p, g=g, Gd=Gd, R=R, datt=R.sum(0), mass_g=mass_g, mass_Gd=mass_Gd, mass_R=mass_R,
                           mass_datt=mass_R.sum(0))


# ---- the same operator in fp32, in the kernels' summation order ----------------------------------------------------------------
def lane_layout(H, vec):
    """(VW, LPR) of the build the host dispatch picks (GLASS_K1_WIDTH_DISPATCH)"""
    VW = 4 if vec else 1
    LPR = 1
    while LPR < -(-H // VW) and LPR < 64:
        LPR *= 2
    return VW, LPR


def _fma(a, b, c):
    """fmaf: the product of two fp32 is exact in fp64; the sum is rounded to fp64, then to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _streams(rowptr, G):
    """Which lane group's sequence an entry belongs to, as the item walk deals a row's entries: a row of fewer than 64 entries
    is one wave's — entry o goes to group o % G at position o // G; a longer row goes in chunks of 256 entries (the plan's cut;
    it may place the cuts elsewhere), each chunk in four quarters of 64 for the four waves, each dealt to the groups likewise.
    Returns (sid [nnz] the stream of each entry, pos [nnz] its position in the stream, srow [n_streams] the row of each stream,
    sk [n_streams] the stream's order within its row: chunk, then wave, then group)."""
    rp = _np(rowptr, np.int64)
    rows = rows_of(rp)
    o = np.arange(rp[-1]) - rp[rows]
    long_ = (rp[1:] - rp[:-1])[rows] >= 64
    cw = np.where(long_, o // 64, 0)        # (chunk, wave) as one number
    ow = np.where(long_, o % 64, o)
    key = (rows * (1 << 20) + cw) * 64 + ow % G
    uniq, sid = np.unique(key, return_inverse=True)
    srow = uniq // 64 // (1 << 20)
    first = np.searchsorted(srow, srow)      # the first stream of each stream's row
    return sid, ow // G, srow, np.arange(uniq.shape[0]) - first


def _by_position(pos):
    order = np.argsort(pos, kind="stable")
    cuts = np.searchsorted(pos[order], np.arange(pos.max() + 2)) if pos.size else np.zeros(1, dtype=np.int64)
    return [order[cuts[t]:cuts[t + 1]] for t in range(len(cuts) - 1)]


def _softmax_streams(rowptr, G, v, sc, Xg):
    """GatAcc in fp32: `take` along every stream, then `merge` of a row's streams in their order.  (The kernels merge lane
    groups in a butterfly, waves and chunks in sequence: the same rule, the pairings differ.)  -> (m, z, S) per row."""
    sid, pos, srow, sk = _streams(rowptr, G)
    ns, H = srow.shape[0], Xg.shape[1]
    f32 = np.float32
    m, z, S = np.full(ns, -np.inf, f32), np.zeros(ns, f32), np.zeros((ns, H), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for idx in _by_position(pos):
            k = sid[idx]
            d = sc[idx] - m[k]
            e = np.exp(-np.abs(d)).astype(f32)
            up = d > 0
            f = np.where(up, f32(1) * e, f32(1)).astype(f32)
            w = np.where(up, v[idx], v[idx] * e).astype(f32)
            z[k] = _fma(z[k], f, w)
            S[k] = _fma(S[k], f[:, None], w[:, None] * Xg[idx])
            m[k] = np.where(up, sc[idx], m[k])
        n = _np(rowptr, np.int64).shape[0] - 1
        rm, rz, rS = np.full(n, -np.inf, f32), np.zeros(n, f32), np.zeros((n, H), f32)
        for idx in _by_position(sk):
            r = srow[idx]
            nm = np.maximum(rm[r], m[idx])
            a = np.where(rm[r] == nm, f32(1), np.exp(rm[r] - nm)).astype(f32)
            b = np.where(m[idx] == nm, f32(1), np.exp(m[idx] - nm)).astype(f32)
            rz[r] = _fma(rz[r], a, z[idx] * b)
            rS[r] = _fma(rS[r], a[:, None], S[idx] * b[:, None])
            rm[r] = nm
    return rm, rz, rS


def _sum_streams(rowptr, G, step, H):
    """SumAcc in fp32: acc = step(acc, entries) along every stream, then the streams of a row added in their order."""
    sid, pos, srow, sk = _streams(rowptr, G)
    acc = np.zeros((srow.shape[0], H), np.float32)
    for idx in _by_position(pos):
        acc[sid[idx]] = step(acc[sid[idx]], idx)
    out = np.zeros((_np(rowptr, np.int64).shape[0] - 1, H), np.float32)
    for idx in _by_position(sk):
        out[srow[idx]] = out[srow[idx]] + acc[idx]
    return out


def _group_dot(A, B, VW, LPR):
    """sum_c A[:,c] B[:,c] as a lane group forms it: lane `sub` runs fmaf over its columns (p * LPR + sub) * VW + k in order,
    then the lanes add in a butterfly"""
    n, H = A.shape
    lane = np.zeros((n, LPR), np.float32)
    for c0 in range(0, H, LPR * VW):
        for k in range(VW):
            cols = c0 + np.arange(LPR) * VW + k
            ok = cols < H
            lane[:, ok] = _fma(A[:, cols[ok]], B[:, cols[ok]], lane[:, ok])
    sh = 1
    while sh < LPR:
        lane = lane + lane[:, np.arange(LPR) ^ sh]
        sh *= 2
    return lane[:, 0]


def gatv2_fp32(adj, X, dY, att, slope, vec=None):
    """Every result of the five entries in fp32, in the kernels' order of operations (see _streams, _softmax_streams,
    _group_dot), from fp32 operands; `adj` a MaxAdj.  -> namespace s, Y, L, p, g, Gd, R, dX, datt (numpy fp32)."""
    f32 = np.float32
    X, dY, att, slope = _np(X, f32), _np(dY, f32), _np(att, f32), f32(slope)
    H = X.shape[1]
    VW, LPR = lane_layout(H, H % 4 == 0 if vec is None else vec)
    G = 64 // LPR
    rp, col, val = _np(adj.rowptr, np.int64), _np(adj.col, np.int64), _np(adj.val, f32)
    rows = rows_of(rp)
    u = X[rows] + X[col]                                       # one rounded add
    pos_ = u > 0
    r = np.where(pos_, u, slope * u).astype(f32)               # one rounded multiply
    s = (r.astype(np.float64) @ att.astype(np.float64)).astype(f32)   # products and sum in fp64, rounded once
    m, z, S = _softmax_streams(rp, G, val, s, X[col])
    live = z > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        Y = np.where(live[:, None], S / np.where(live, z, f32(1))[:, None], f32(0)).astype(f32)
        L = np.where(live, m + np.log(np.where(live, z, f32(1))), f32(0)).astype(f32)
    D = _group_dot(dY, Y, VW, LPR)
    q = _group_dot(dY[rows], X[col], VW, LPR)
    p = (val * np.exp(s - L[rows]).astype(f32)).astype(f32)
    g = (p * (q - D[rows])).astype(f32)
    gf = np.where(pos_, g[:, None], (g * slope)[:, None]).astype(f32)
    Gd = _sum_streams(rp, G, lambda acc, idx: _fma(gf[idx], np.broadcast_to(att, gf[idx].shape), acc), H)
    R = _sum_streams(rp, G, lambda acc, idx: _fma(np.broadcast_to(g[idx, None], r[idx].shape), r[idx], acc), H)
    # the transposed pass: the entries in A^T's order, p and g through eid_t
    rpt, eid = _np(adj.rowptr_t, np.int64), _np(adj.eid_t, np.int64)
    dest = rows[eid]
    pt, gft, dYt = p[eid], gf[eid], dY[dest]
    T = _sum_streams(rpt, G, lambda acc, idx: _fma(gft[idx], np.broadcast_to(att, gft[idx].shape),
                                                   _fma(np.broadcast_to(pt[idx, None], dYt[idx].shape), dYt[idx], acc)), H)
    datt = R.astype(np.float64).sum(0).astype(f32)
    return SimpleNamespace(s=s, Y=Y, L=L, p=p, g=g, Gd=Gd, R=R, dX=(Gd + T).astype(f32), datt=datt)


# ---- for autograd ------------------------------------------------------------------------------------------------------------------
def scatter_gatv2_aggregate(edge_index, edge_weight, n, X, att, slope):
    """The same operator on the raw edge list (any order) from differentiable torch ops: X and att may require grad."""
    row, col = edge_index[0], edge_index[1]
    H = X.shape[1]
    s = F.leaky_relu(X[row] + X[col], float(slope)) @ att
    M = torch.zeros(n, dtype=X.dtype).scatter_reduce(0, row, s.detach(), "amax", include_self=False)
    w = edge_weight.to(X.dtype) * torch.exp(s - M[row])
    Z = torch.zeros(n, dtype=X.dtype).index_add(0, row, w)
    S = torch.zeros((n, H), dtype=X.dtype).index_add(0, row, w[:, None] * X[col])
    live = (torch.bincount(row, minlength=n) > 0)[:, None]
    return torch.where(live, S / torch.where(live, Z[:, None], torch.ones((), dtype=X.dtype)), torch.zeros((), dtype=X.dtype))


class GatV2Adj(MaxAdj):
    """`GatV2Adj(edge_index, edge_weight, n, att, slope) @ X`: differentiable dynamic attention aggregation in the dtype of X;
    takes the place of OracleConv.adj.  att is a tensor that may require grad (the layer's parameter)."""
    def __init__(self, edge_index, edge_weight, n, att, slope=0.2):
        super().__init__(edge_index, edge_weight, n)
        self.edge_index, self.edge_weight, self.att, self.slope = edge_index, edge_weight, att, float(slope)

    def __matmul__(self, X):
        return scatter_gatv2_aggregate(self.edge_index, self.edge_weight, self.n, X, self.att.to(X.dtype), self.slope)


# ---- the cases and the grading the GPU test and its CPU twin share ------------------------------------------------------------------
TOL = 1e-5
WIDTHS = (4, 18, 64, 68, 128, 132, 256, 260)   # every VW / LPR case, two column tiles / column passes
SLOPES = (0.2, 0.0, 1.0)
S_MAX = 8.0


def case_operands(adj, seed, H):
    """(X, dY, att) fp32 torch tensors for a MaxAdj: X, dY randn; att uniform in +-0.5, then scaled so that the largest |s_e|
    over the graph and the three slopes is 7.5 — |s_e| <= 8 for every entry, with scores large enough to rank neighbours."""
    g = torch.Generator().manual_seed(seed)
    X, dY = torch.randn(adj.n, H, generator=g), torch.randn(adj.n, H, generator=g)
    att = torch.rand(H, generator=g) - 0.5
    top = max(float(np.abs(gatv2_aggregate(adj.rowptr, adj.col, adj.val, X, att, sl)[2]).max()) for sl in SLOPES)
    return X, dY, (att * (7.5 / top)).float()


def reference(adj, X, dY, att, slope):
    """fp64 from the fp32 operands: a namespace with Y, L, s, mass_s and the backward's fields"""
    Y, L, s, mass_s = gatv2_aggregate(adj.rowptr, adj.col, adj.val, X, att, slope)
    r = gatv2_aggregate_bwd(adj.rowptr, adj.col, adj.val, dY, X, Y, L, s, att, slope)
    r.Y, r.L, r.s, r.mass_s = Y, L, s, mass_s
    return r


def of_mass(got, want, mass):
    """the largest |got - want| / mass; an element without mass must be exact (inf otherwise)"""
    d = np.abs(_np(got) - want)
    live = mass > 0
    if not bool((d[~live] == 0).all()):
        return float("inf")
    return float((d[live] / mass[live]).max()) if bool(live.any()) else 0.0


def rel_inf(got, want):
    """||got - want||_inf / ||want||_inf"""
    den = float(np.abs(want).max()) if want.size else 0.0
    return (float(np.abs(_np(got) - want).max()) if want.size else 0.0) / (den if den > 0 else 1.0)


def errors(res, r):
    """res: anything with Y, L, dX, s, g, Gd, R, datt (torch or numpy); r: reference().  Y, L, dX at rel-inf, the cancelling sums
    element by element of their mass: every figure must be <= TOL."""
    get = (lambda k: res[k]) if isinstance(res, dict) else (lambda k: getattr(res, k))
    return dict(Y=rel_inf(get("Y"), r.Y), L=rel_inf(get("L"), r.L), dX=rel_inf(get("dX"), r.dX),
                s=of_mass(get("s"), r.s, r.mass_s), g=of_mass(get("g"), r.g, r.mass_g), Gd=of_mass(get("Gd"), r.Gd, r.mass_Gd),
                R=of_mass(get("R"), r.R, r.mass_R), datt=of_mass(get("datt"), r.datt, r.mass_datt))
