"""Restatements for the edge dropout tests (K2d, csrc/spmm_dropedge.hip), numpy only.

* mix32 / rand4_word0 / edge_key / keep_mask: the generator of csrc/common.h, the key and the keep rule in exact integer
  arithmetic (uint32 wrap-around carried in uint64 and masked) — bit-exact, no tolerance applies.
* masked_values: deg', val' of the masked weights in fp64 (K2's rules: row sums, + 1 below 0.5, the three normalisations).
* mixed(): the test graph.
"""
import functools

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
SEED, CALL_IDS, PS = 1234, (18, 34), (0.0, 0.3, 0.9)   # call ids: 16 * (layer + 1) + 2, what a 2-layer model's layers draw from
AGGRS = ("sum", "mean", "gcn")
FAMILIES = ("int", "rand")


def _u64(x):
    return np.asarray(x, dtype=np.uint64)


def mix32(x):
    x = _u64(x) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & M32
    x ^= x >> np.uint64(16)
    return x


def rand4_word0(seed, step, call_id, idx):
    """out[0] of rand4(seed, step, call_id, idx) for an array of uint64 counters."""
    seed, step, call_id, idx = int(seed), int(step), int(call_id), _u64(idx)
    lo = lambda v: np.uint64(v & 0xFFFFFFFF)
    key = mix32(lo(seed) ^ mix32(lo(seed >> 32) ^ mix32(lo(step) ^ mix32((lo(call_id) + np.uint64(0x9E3779B9)) & M32))))
    x = (mix32((idx & M32) ^ key) + (((idx >> np.uint64(32)) * np.uint64(0x85EBCA6B)) & M32)) & M32
    return mix32((x + np.uint64(0x632BE5AB)) & M32)


def edge_key(ei, n, symmetric):
    """uint64 key of every edge (ei[0] = destination row i, ei[1] = source column j)."""
    i, j = _u64(ei[0]), _u64(ei[1])
    if symmetric:
        i, j = np.minimum(i, j), np.maximum(i, j)
    return i * np.uint64(n) + j


def keep_mask(ei, n, p, seed, step, call_id, symmetric=True):
    """uint8 [E], the caller's edge order: u = (word >> 8) * 2^-24 (exact in fp32 and fp64), kept iff u >= float32(p)."""
    word = rand4_word0(seed, step, call_id, edge_key(ei, n, symmetric))
    u = (word >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return (u >= float(np.float32(p))).astype(np.uint8)


def masked_values(ei, w, keep, n, aggr):
    """(val' [E] in the caller's order, deg' [n]) in fp64."""
    wm = np.where(keep != 0, w.astype(np.float64), 0.0)
    deg = np.bincount(ei[0], weights=wm, minlength=n)
    deg = np.where(deg < 0.5, deg + 1.0, deg)
    if aggr == "sum":
        return wm, deg
    if aggr == "mean":
        return wm / deg[ei[0]], deg
    assert aggr == "gcn"
    return wm / np.sqrt(deg[ei[0]]) / np.sqrt(deg[ei[1]]), deg


def dense(ei, val, n):
    A = np.zeros((n, n), dtype=np.float64)
    np.add.at(A, (ei[0], ei[1]), val)
    return A


N = 300
HUBS = {0: 200, 1: 63, 2: 64, 3: 65, 4: 1, 5: 2}   # node -> undirected neighbours (rows AND columns of that length); node 6: none
IN_ONLY, OUT_ONLY = 7, 8                           # three one-directional edges each: a forward row / a transposed row of 0
LOOPS = (120, 121)
DUP = (130, 131)                                   # an undirected pair listed twice (four entries)


@functools.lru_cache(maxsize=None)
def mixed(family="rand"):
    """(n, ei int64 [2, E], w fp32 [E], und): 300 nodes.  Nodes 0..5 have exactly 200 / 63 / 64 / 65 / 1 / 2 undirected neighbours among
    the fillers 100..299 (both directions listed: the forward rows and the transposed rows of those lengths), node 6 none, node 7
    three in-edges only, node 8 three out-edges only, five more one-directional edges among the fillers, two self-loops, one
    undirected pair listed twice, 150 random undirected filler pairs; the edge list is shuffled.  und: bool [E], the entries
    whose reverse is listed too (self-loops excluded).  Weights: "int" in {1, 2, 3}, "rand" uniform in [0.2, 2)."""
    rng = np.random.Generator(np.random.PCG64(11))
    pairs = []
    for hub, k in HUBS.items():
        pairs += [(hub, 100 + t) for t in range(k)]
    seen = set()
    while len(seen) < 150:
        a, b = (int(v) for v in rng.integers(100, N, 2))
        if a != b and not {a, b} & set(LOOPS + DUP) and (min(a, b), max(a, b)) not in seen:
            seen.add((min(a, b), max(a, b)))
    pairs += sorted(seen) + [DUP, DUP]
    und_edges = [(a, b) for a, b in pairs] + [(b, a) for a, b in pairs]
    one_way = [(IN_ONLY, 140 + t) for t in range(3)] + [(150 + t, OUT_ONLY) for t in range(3)]
    one_way += [(20 + t, 40 + t) for t in range(5)]                      # (dst, src) among nodes with no other edges
    loops = [(v, v) for v in LOOPS]
    ei = np.array(und_edges + one_way + loops, dtype=np.int64).T
    und = np.zeros(ei.shape[1], dtype=bool)
    und[:len(und_edges)] = True
    order = rng.permutation(ei.shape[1])
    ei, und = np.ascontiguousarray(ei[:, order]), und[order]
    if family == "int":
        w = rng.integers(1, 4, ei.shape[1]).astype(np.float32)
    else:
        assert family == "rand"
        w = rng.uniform(0.2, 2.0, ei.shape[1]).astype(np.float32)
    for a in (ei, w, und):
        a.setflags(write=False)
    return N, ei, w, und


def row_lengths(ei, n):
    """(forward row lengths, transposed row lengths)"""
    return np.bincount(ei[0], minlength=n), np.bincount(ei[1], minlength=n)
