"""Host side of the K1 sum-kernel tests (glass_amd/csrc/spmm.hip, spmm_sweep.h, spmm_common.h, spmm_rep.hip) — numpy and
torch fp64, CPU only: the graphs, the plan read back as item lists, the fp64 CSR product with the mass of every
element, and the gate.

Graphs (deterministic, edges in SHUFFLED order, not symmetric, weights uniform in [0.25, 2)):
  mixed, all_long   the recipes of tests/test_gpu_aggr_gat.py (same seeds, so the same plans).
  flat              28 000 rows.  85 % hold 0..3 entries (sweep items of two to four rows, flat-eligible at every G), 15 % hold
                    20..40 (each an item of its own: not eligible at G = 2 and 4, partly at G = 8, eligible from G = 16), rows
                    of 63 (the longest short row), 64, 65, 100 and 300 entries and one of 600 (cut into two chunks).  The
                    sources are drawn so that the TRANSPOSED matrix has the same make-up: 85 % / 15 % of the sources, and
                    sources 5 .. 10 are hubs of 600 (cut), 300, 100, 65, 64 and 63 entries.
  flat_runs         640 000 rows of 0, 1 or 2 entries (one half empty).  At the smallest item budget a flat item holds at most four
                    rows, so with 16 or more lane groups per wave no group ever owns two; only a sweep large enough for a budget
                    of about 90 cost units packs some twenty rows into an item, and at G = 16 a group then walks a run of two
                    rows, empty ones in front, between and behind.  Forward only, one width.

Gate: element by element |got - want| <= 1e-5 * mass, mass[r, c] = sum_e |val_e * x[col_e, c]|; an element without mass
(an empty row) must be exactly 0.  The plain fp32 product in CSR order (product_f32: every product and every sum rounded)
stays below 4e-7 of its mass on the three graphs (tests/test_k1_sum_host.py prints it), so the bar has 25x headroom over
honest fp32 in the worst order a kernel could take."""
import ctypes
import functools

import numpy as np
import torch

TOL = 1e-5
KINDS = ("mixed", "all_long", "flat")
ALL_KINDS = KINDS + ("flat_runs", )
# header word indices (glass_amd/csrc/spmm_common.h)
(H_MAGIC, H_VER, H_NROWS, H_NNZ, H_NSWEEP, H_NLONG, H_NREDUCE, H_NSLOTS, H_LONG_THR, H_LONG_CHUNK, H_OFF_SWEEP, H_OFF_LONG,
 H_OFF_REDUCE, H_RP_FACTOR, H_MIN_ITEM_DEG, H_FLAT_SHARE) = range(16)
FLAT_MIN_ITEMS = 8192   # kFlatMinItems (spmm_sweep.h)
FLAT_MIN_SHARE15 = 4    # kFlatMinShare15

# the widths of tests/test_gpu_k1_sum.py: (H, vector layout)
VEC_WIDTHS = (4, 8, 16, 32, 64, 128, 256, 260, 520)        # LPR 1 .. 64, then 2 and 3 column tiles
SCALAR_WIDTHS = (1, 2, 3, 7, 13, 17, 33, 100, 130)         # LPR 1 .. 64, then 2 and 3 column tiles
FLAT_VEC_WIDTHS = (4, 16, 32, 64, 128)                     # G = 64, 16, 8, 4, 2
FLAT_SCALAR_WIDTHS = (17, )                                # LPR 32, G = 2


def build_of(H, vec):
    """(VW, LPR, column tiles): GLASS_K1_WIDTH_DISPATCH restated"""
    vw = 4 if vec else 1
    assert not vec or H % 4 == 0
    lanes, lpr = H // vw, 1
    while lpr < lanes and lpr < 64:
        lpr *= 2
    return vw, lpr, -(-H // (lpr * vw))


def _edges(degrees, n, rng, hub_share, hub_frac=0.0):
    """One destination row per entry of `degrees`; sources uniform, except that a share of the rows also names source 5, and a
    fraction of all entries (a hub: its row of the TRANSPOSED matrix is long and cut).  (tests/test_gpu_aggr_gat.py's)"""
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


FLAT_ROWS = 28000
FLAT_SPECIAL = ((101, 63), (3001, 64), (3002, 65), (9000, 100), (15000, 300), (27990, 600))   # (row, entries)
FLAT_HUBS = ((5, 600), (6, 300), (7, 100), (8, 65), (9, 64), (10, 63))                        # (source, entries)


def _flat_degrees(rng, n):
    d = rng.integers(0, 4, n)
    heavy = rng.random(n) < 0.15
    d[heavy] = rng.integers(20, 41, int(heavy.sum()))
    return d


def _flat_edges(rng):
    n = FLAT_ROWS
    deg = _flat_degrees(rng, n)
    for r, d in FLAT_SPECIAL:
        deg[r] = d
    row = np.repeat(np.arange(n), deg)
    nnz = row.shape[0]
    # the sources: a pool with the same two kinds of out-degree, thinned or padded to nnz entries, then the hubs
    pool = np.repeat(np.arange(n), _flat_degrees(rng, n))
    pool = pool[rng.permutation(pool.shape[0])]
    col = pool[:nnz] if pool.shape[0] >= nnz else np.concatenate((pool, rng.integers(0, n, nnz - pool.shape[0])))
    col = col.copy()
    short = np.flatnonzero(deg[row] < 20)   # hub entries go into short rows, which stay short: one entry is renamed, none added
    take = rng.permutation(short)
    at = 0
    for src, d in FLAT_HUBS:
        col[col == src] = (src + 100) % n
        col[take[at:at + d]] = src
        at += d
    w = rng.uniform(0.25, 2.0, nnz).astype(np.float32)
    return n, row, col, w


FLAT_RUNS_ROWS = 640000


def _flat_runs_edges(rng):
    n = FLAT_RUNS_ROWS
    row = np.repeat(np.arange(n), rng.choice(3, n, p=(0.5, 0.4, 0.1)))
    col = rng.integers(0, n, row.shape[0])
    return n, row, col, rng.uniform(0.25, 2.0, row.shape[0]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def graph(kind):
    """-> (n, edge_index int64 [2, nnz], edge_weight fp32) on the host, in shuffled edge order"""
    rng = np.random.Generator(np.random.PCG64({"mixed": 17, "all_long": 18, "flat": 19, "flat_runs": 20}[kind]))
    if kind == "mixed":
        degrees = [0, 1, 2, 63, 64, 65, 255, 256, 257, 700] + list(rng.integers(1, 13, 997))
        n = len(degrees)
        row, col, w = _edges(degrees, n, rng, 0.7)
        extra_r, extra_c = np.array([20, 20, 30]), np.array([40, 40, 30])      # (20, 40) twice; self-loop (30, 30)
        extra_w = np.array([0.5, 1.25, 0.75], dtype=np.float32)
        row, col, w = np.concatenate((row, extra_r)), np.concatenate((col, extra_c)), np.concatenate((w, extra_w))
    elif kind == "all_long":
        degrees = list(rng.integers(64, 301, 38)) + [700, 0] + [200, 200]
        n = len(degrees)
        row, col, w = _edges(degrees, n, rng, 0.0, 0.2)
    elif kind == "flat":
        n, row, col, w = _flat_edges(rng)
    else:
        n, row, col, w = _flat_runs_edges(rng)
    perm = rng.permutation(row.shape[0])
    ei = torch.from_numpy(np.stack((row[perm], col[perm])).astype(np.int64))
    return n, ei, torch.from_numpy(w[perm].copy())


def csr(kind, transposed=False):
    """(rowptr int32 [n + 1], col int64, val fp32) as graph.CSRAdj sorts them: by (row, col), stable, duplicates kept; the
    transposed matrix by (col, row) of that order."""
    n, ei, ew = graph(kind)
    row, col = ei[0].numpy(), ei[1].numpy()
    perm = np.argsort(row * n + col, kind="stable")
    row, col, w = row[perm], col[perm], ew.numpy()[perm]
    if transposed:
        perm_t = np.argsort(col * n + row, kind="stable")
        row, col, w = col[perm_t], row[perm_t], w[perm_t]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=n))
    return rowptr.astype(np.int32), col.copy(), w.copy()


class Plan:
    """glass_spmm_plan_build's blob as lists: header, sweep items (r0, r1, e0, e1), long items (row, e0, e1, slot), reduce rows
    (row, first slot, slots)"""
    def __init__(self, rowptr):
        from glass_amd import _lib
        lib = _lib.load()
        rp = np.ascontiguousarray(rowptr, dtype=np.int32)
        words = ctypes.c_int64(0)
        assert lib.glass_spmm_plan_build(rp.ctypes.data, rp.shape[0] - 1, None, ctypes.byref(words)) == 0
        blob = np.zeros(words.value, dtype=np.int32)
        assert lib.glass_spmm_plan_build(rp.ctypes.data, rp.shape[0] - 1, blob.ctypes.data, ctypes.byref(words)) == 0
        self.blob = blob
        self.header = h = blob[:16].copy()
        self.sweep = blob[h[H_OFF_SWEEP]:h[H_OFF_SWEEP] + 4 * h[H_NSWEEP]].reshape(-1, 4)
        self.long = blob[h[H_OFF_LONG]:h[H_OFF_LONG] + 4 * h[H_NLONG]].reshape(-1, 4)
        self.reduce = blob[h[H_OFF_REDUCE]:h[H_OFF_REDUCE] + 3 * h[H_NREDUCE]].reshape(-1, 3)


def flat_share15(header, G):
    """fifteenths of the sweep cost in items that are flat-eligible at G lane groups per wave (a power of two)"""
    return (int(header[H_FLAT_SHARE]) >> (4 * (int(G).bit_length() - 1))) & 15


def takes_flat_build(header, G):
    """spmm_sweep_flat (spmm_sweep.h) restated: does a launch at G lane groups take the flat-capable sweep build"""
    return G > 1 and int(header[H_NSWEEP]) >= FLAT_MIN_ITEMS and flat_share15(header, G) >= FLAT_MIN_SHARE15


def flat_eligible(sweep, factor, G):
    """per sweep item, the kernel's test: edges <= factor * G * rows"""
    return (sweep[:, 3] - sweep[:, 2]) <= factor * G * (sweep[:, 1] - sweep[:, 0])


def product(rowptr, col, val, X):
    """fp64 from the fp32 values: (Y, mass) with Y = A @ X and mass[r, c] = sum_e |val_e * X[col_e, c]|; torch fp64"""
    rowptr, col = torch.as_tensor(np.asarray(rowptr)).to(torch.int64), torch.as_tensor(np.asarray(col)).to(torch.int64)
    val, X = torch.as_tensor(np.asarray(val)).double(), torch.as_tensor(np.asarray(X)).double()
    n, H = rowptr.shape[0] - 1, X.shape[1]
    rows = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1])
    Y, mass = torch.zeros((n, H), dtype=torch.float64), torch.zeros((n, H), dtype=torch.float64)
    for c0 in range(0, H, 32):   # (column blocks bound the [nnz, block] temporary)
        P = val[:, None] * X[col, c0:c0 + 32]
        Y[:, c0:c0 + 32].index_add_(0, rows, P)
        mass[:, c0:c0 + 32].index_add_(0, rows, P.abs())
    return Y, mass


def product_f32(rowptr, col, val, X, skip=()):
    """The plain fp32 product, every row summed in CSR order, one rounded multiply and one rounded add per entry (numpy fp32);
    `skip`: entry indices left out."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    val, X = np.asarray(val, dtype=np.float32), np.asarray(X, dtype=np.float32)
    keep = np.ones(val.shape[0], dtype=bool)
    keep[list(skip)] = False
    n, deg = rowptr.shape[0] - 1, rowptr[1:] - rowptr[:-1]
    Y = np.zeros((n, X.shape[1]), dtype=np.float32)
    for k in range(int(deg.max()) if n else 0):
        live = np.flatnonzero(deg > k)
        e = rowptr[live] + k
        live, e = live[keep[e]], e[keep[e]]
        Y[live] = Y[live] + val[e, None] * X[col[e]]
    return Y


def of_mass(got, want, mass):
    """the largest |got - want| / mass; an element without mass must be exact (inf otherwise)"""
    got = torch.as_tensor(np.asarray(got.detach().cpu() if isinstance(got, torch.Tensor) else got)).double()
    d = (got - want).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    ok0 = bool((d[mass == 0] == 0).all())
    live = mass > 0
    worst = float((d[live] / mass[live]).max()) if bool(live.any()) else 0.0
    return worst if ok0 else float("inf")


@functools.lru_cache(maxsize=None)
def operand(kind, H, seed=0):
    """X: randn, fp32, one per (graph, width, seed)"""
    n = graph(kind)[0]
    g = torch.Generator().manual_seed(1000 * H + 10 * ALL_KINDS.index(kind) + seed)
    return torch.randn(n, H, generator=g)
