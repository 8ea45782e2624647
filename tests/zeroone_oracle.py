"""Exact zero-one labels restated with the CPU oracle (oracle/glass_oracle.py, pinned to the reference by the golden
fixtures): row b of the result is what the reference computes for pos[b:b+1] ALONE with MaxZOZ — its own label vector on the
whole graph, its own message passing, GraphNorm statistics and pooling.  One oracle call per subgraph."""
import numpy as np
import torch

from oracle import glass_oracle as O


def zeroone_z(n_nodes, pos):
    """numpy restatement of utils.ZeroOneZ: z[b, n] = 1 iff n occurs in pos[b] (-1 and ids >= n_nodes skipped)."""
    pos = np.asarray(pos)
    z = np.zeros((pos.shape[0], n_nodes), dtype=np.int64)
    for b in range(pos.shape[0]):
        ids = pos[b][(pos[b] >= 0) & (pos[b] < n_nodes)]
        z[b, ids] = 1
    return z


def logits(model, x, ei, ew, pos):
    """[B, out] logits of the oracle model, subgraph by subgraph."""
    rows = []
    for b in range(pos.shape[0]):
        p = pos[b:b + 1]
        rows.append(model(x, ei, ew, p, O.max_zero_one(x, p)))
    return torch.cat(rows, dim=0)


def graph(n=300, seed=0):
    """A connected random graph (ring + chords), symmetrised and (row, col)-sorted, with five subgraphs: two that overlap,
    one adjacent to them along the ring, one padded row, one row that names a node twice."""
    rng = np.random.Generator(np.random.PCG64(seed))
    u = np.concatenate([np.arange(n), rng.integers(0, n, 2 * n)])
    v = np.concatenate([(np.arange(n) + 1) % n, rng.integers(0, n, 2 * n)])
    keep = u != v
    pairs = np.unique(np.stack([np.minimum(u[keep], v[keep]), np.maximum(u[keep], v[keep])]), axis=1)
    ei = np.concatenate([pairs, pairs[::-1]], axis=1)
    ei = ei[:, np.argsort(ei[0] * n + ei[1], kind="stable")]
    pos = np.full((5, 10), -1, dtype=np.int64)
    pos[0] = np.arange(0, 10)
    pos[1] = np.arange(5, 15)          # overlaps row 0
    pos[2, :8] = np.arange(15, 23)     # adjacent to row 1 (ring edge 14-15); padded
    pos[3, :3] = [40, 41, 42]          # mostly padding
    pos[4] = [100, 101, 101, 102, 103, 104, 105, 106, 107, 108]  # node 101 twice
    x = torch.from_numpy(rng.integers(0, 4, n)).reshape(n, 1, 1)
    return n, torch.from_numpy(ei.copy()), torch.ones(ei.shape[1]), x, torch.from_numpy(pos)
