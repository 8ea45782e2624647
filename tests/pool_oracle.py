"""Host side of the K7 pooling tests (glass_amd/csrc/pool.hip, bucket.h) — numpy fp64, numpy fp32 and Python integers, CPU only:
the input recipes, the fp64 truth of every form with the mass of every element, max pooling in closed form, the dispatch
restated (and checked against the constants in the source text by tests/test_pool_host.py), the kernels' own summation orders
in fp32, ExactSum in Python integers, and the gates.

Recipes (deterministic; `valid` means 0 <= id < n, everything else is padding):
  ragged(B, Smax, n)   subgraphs of 1 .. Smax distinct nodes; row 2 full, row 3 all padding, row 5 a single node, rows 6 and 7 share a
                       node, row 8 names a node twice (Smax >= 2), node 1 is named by no row, node n - 1 is in row 0, row 9
                       has a padding entry in front of valid ones and row 10 an id beyond n (Smax >= 3).
  ties(B, Smax, n, C)  ragged's pos with embeddings from {-1, -0.5, 0, 0, 0, 0.5, 1}, every third zero a -0; columns c % 5 == 1
                       hold no positive value (zeros win there, as after dropout); the full row's column-0 maximum sits at
                       the last j only.
  lists()              B = 400, Smax = 31, n = 262: node lists of exactly 64, 1, 63, 65 (nodes 0 .. 3: two long nodes with two
                       short ones between them in the first gather workgroup at G = 64, four nodes, and at G = 1, 256 nodes),
                       0, 62, 200 and 400 = every row (nodes 4 .. 7), 64 and 1 (nodes 260, 261: the last, partly filled
                       workgroup at both G, a long node in it); every other node 0 .. 5.  A node's entries are in distinct rows.
  pairs(B, n)          (a, b), (a, a), (-1, b), (a, -1), (-1, -1) in rows 1 .. 5, node 11 named by every seventh pair, the last
                       ten nodes but n - 1 named by none.
  operand(rows, C)     randn; column C - 1 times 1e4 (C >= 2) and column C - 2 times 1e-6 (C >= 3): a small and a large element
                       side by side, the large one in the last lane of the tail tile.

Gates, element by element (a NaN is an infinite error, an element whose bound is 0 must be exactly 0):
  float forms (forward sum / mean / size, pair forward, ordered scatter, atomic scatter):  |got - want| <= 1e-5 * mass
  exact forms (pair, bucketed, max gathers):  |got - want| <= rel * mass + entries * 2^-60, rel = 2^-21 (max: 2^-23).  An addend
      carries at most three fp32 roundings (1 / sqrt(cnt) or 1 / cnt two, the product one; max pooling: none), the integer sum
      none, value() one more: 4 * 2^-24 = 2^-22 of the mass (max: 2^-24), and one binade of slack for the second-order terms; the
      truncation to the 2^-60 quantum costs at most 2^-60 per addend.

Measured by tests/test_pool_host.py (the fp32 restatement of each order, worst share of its bound):
  forward, slot-then-LDS order    sum 0.008, mean 0.010, size 0.011   (`ragged`, Smax 40)
  pair forward                    sum 0.006, mean 0.006, size 0.012
  ordered scatter (fma chain)     sum 0.009, mean 0.010, size 0.011
  atomic scatter in (b, s) order  sum 0.009, mean 0.013, size 0.013
  exact gather, ExactSum          sum 0.117, mean 0.220, size 0.238   (rel 2^-21; `ragged` and `lists`)
  max gather, ExactSum            0.408                               (rel 2^-23)
(The max gather's bound is value()'s one rounding with one binade of slack, so its share approaches 0.5 from below on wide
inputs: tests/test_gpu_pool.py prints up to 0.499 on `lists`.)"""
import functools
import os
import re

import numpy as np

TOL = 1e-5
REL_EXACT, REL_MAX, QUANTUM = 2.0**-21, 2.0**-23, 2.0**-60
MODES = {"sum": 0, "mean": 1, "max": 2, "size": 3}
BLOCK, WAVE = 256, 64              # common.h kBlock, kWave
POOL_ORDERED_MAX = 12288           # pool.hip kPoolOrderedMax
PAIR_LONG_LIST = 64                # pool.hip kPairLongList
PAIR_GROUP_CAP = 64                # pair_group_log2's cap

# the widths of tests/test_gpu_pool.py
FWD_VEC, FWD_SCALAR = (4, 8, 64, 512, 1024, 1028), (1, 3, 17, 255, 257)
FWD_SMAX = (1, 3, 40, 257)
PAIR_VEC, PAIR_SCALAR = (4, 8, 64, 256, 320), (1, 3, 17, 65, 100)
LIST_WIDTHS = ((4, True), (17, False), (64, True), (320, True))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source_constants():
    """the constants the restatements depend on, read from the source text"""
    pool = open(os.path.join(ROOT, "glass_amd", "csrc", "pool.hip")).read()
    common = open(os.path.join(ROOT, "glass_amd", "csrc", "common.h")).read()
    num = lambda pat, text: int(re.search(pat, text).group(1))
    group = re.search(r"static int pair_group_log2\(.*?\n}", pool, re.S).group(0)
    fwd = re.search(r'extern "C" int glass_segment_pool_f32\(.*?\n}', pool, re.S).group(0)
    return {"kBlock": num(r"constexpr int kBlock = (\d+);", common), "kWave": num(r"constexpr int kWave = (\d+);", common),
            "kPoolOrderedMax": num(r"constexpr int64_t kPoolOrderedMax = (\d+);", pool),
            "kPairLongList": num(r"constexpr int kPairLongList = (\d+);", pool),
            "pair_group_cap": num(r"pow2_ceil_cap\(cw, (\d+)\)", group), "fwd_cap_is_kBlock": "pow2_ceil_cap(cw, kBlock)" in fwd}


def _pow2_ceil_cap(v, cap):
    p = 1
    while p < v and p < cap:
        p *= 2
    return p


def fwd_build(C, aligned=True):
    """glass_segment_pool_f32's choice -> (VW, TC lanes per row, row slots, column tiles); aligned: lde, ldo multiples of 4 and
    both pointers on 16 bytes"""
    vw = 4 if aligned and C % 4 == 0 else 1
    cw = -(-C // vw)
    tc = _pow2_ceil_cap(cw, BLOCK)
    return vw, tc, BLOCK // tc, -(-cw // tc)


def pair_group(C, vec):
    """lanes per pair (forward) or per node (the gathers): pair_group_log2 restated"""
    assert not vec or C % 4 == 0
    return _pow2_ceil_cap(-(-C // (4 if vec else 1)), PAIR_GROUP_CAP)


def bwd_form(B, Smax, mode):
    """which backward ops.segment_pool takes"""
    if Smax == 2 and mode != "max":
        return "pair"
    if mode == "max":
        return "max_exact"
    return "exact" if B * Smax + B > POOL_ORDERED_MAX else "ordered"


# ---- recipes -------------------------------------------------------------------------------------------------------------------
def valid_of(pos, n):
    return (pos >= 0) & (pos < n)


@functools.lru_cache(maxsize=None)
def ragged(B, Smax, n):
    """-> (pos int64 [B, Smax], facts)"""
    assert B >= 11 and n >= Smax + 8
    rng = np.random.Generator(np.random.PCG64(1000 * Smax + B))
    pool = np.arange(2, n - 1)                       # node 0: shared, node 1: unused, node n - 1: row 0's
    pos = np.full((B, Smax), -1, dtype=np.int64)
    for b in range(B):
        k = int(rng.integers(1, Smax + 1))
        pos[b, :k] = rng.choice(pool, k, replace=False)
    pos[0, 0] = n - 1
    pos[2, :] = rng.choice(pool, Smax, replace=False)        # a full row
    pos[3, :] = -1
    pos[5, :] = -1
    pos[5, 0] = pool[7]
    pos[6, 0] = pos[7, 0] = 0
    facts = {"full": 2, "empty": 3, "single": 5, "shared": (6, 7, 0), "unused": 1, "dup": None, "lead_pad": None, "beyond": None}
    if Smax >= 2:
        pos[8:11, :] = -1
        pos[8, :2] = pool[9]
        facts["dup"] = (8, int(pool[9]))
    if Smax >= 3:
        pos[8, 2] = pool[10]
        pos[9, :3] = (-1, pool[11], pool[12])
        pos[10, :3] = (pool[13], n + 3, pool[14])
        facts["lead_pad"], facts["beyond"] = 9, 10
    pos.setflags(write=False)
    return pos, facts


TIE_VALUES = np.array([-1.0, -0.5, 0.0, 0.0, 0.0, 0.5, 1.0], dtype=np.float32)


def tie_emb(n, C, seed=0):
    """embeddings from TIE_VALUES, every third zero a -0, no positive value in the columns c % 5 == 1"""
    rng = np.random.Generator(np.random.PCG64(77 + 13 * C + seed))
    emb = TIE_VALUES[rng.integers(0, 7, (n, C))]
    neg = emb[:, 1::5]
    neg[neg > 0] *= -1
    flat = emb.reshape(-1)
    zeros = np.flatnonzero(flat == 0)
    flat[zeros[::3]] = -0.0
    return emb


@functools.lru_cache(maxsize=None)
def ties(B, Smax, n, C):
    """-> (pos, emb fp32 [n, C], row whose column-0 maximum is at the last j only)"""
    pos, facts = ragged(B, Smax, n)
    emb = tie_emb(n, C)
    row = facts["full"]
    emb[pos[row, -1], 0] = 2.0
    emb.setflags(write=False)
    return pos, emb, row


LISTS_B, LISTS_SMAX, LISTS_N = 400, 31, 262
LISTS_SPECIAL = {0: 64, 1: 1, 2: 63, 3: 65, 4: 0, 5: 62, 6: 200, 7: 400, 260: 64, 261: 1}


@functools.lru_cache(maxsize=None)
def lists():
    """-> pos int64 [400, 31] over 262 nodes (module docstring); a node's entries sit in distinct rows, padding interleaved"""
    B, S, n = LISTS_B, LISTS_SMAX, LISTS_N
    rng = np.random.Generator(np.random.PCG64(5))
    length = rng.integers(0, 6, n)
    for node, L in LISTS_SPECIAL.items():
        length[node] = L
    fill = np.zeros(B, dtype=np.int64)
    pos = np.full((B, S), -1, dtype=np.int64)
    for node in np.argsort(-length, kind="stable"):
        order = rng.permutation(B)
        rows = order[np.argsort(fill[order], kind="stable")[:length[node]]]     # the emptiest rows, ties at random
        pos[rows, fill[rows]] = node
        fill[rows] += 1
    assert int(fill.max()) <= S
    for b in range(B):
        pos[b] = pos[b, rng.permutation(S)]
    pos.setflags(write=False)
    return pos


def list_lengths(pos, n, dedup=False):
    """entries per node; dedup: rows per node (max pooling's lists)"""
    out = np.zeros(n, dtype=np.int64)
    for row in pos:
        ids = row[valid_of(row, n)]
        np.add.at(out, np.unique(ids) if dedup else ids, 1)
    return out


@functools.lru_cache(maxsize=None)
def pairs(B, n):
    rng = np.random.Generator(np.random.PCG64(B + n))
    p = rng.integers(0, n - 10, (B, 2))
    p[::7, 0] = 11
    p[1], p[2], p[3], p[4], p[5] = (20, 21), (22, 22), (-1, 23), (24, -1), (-1, -1)
    p[8, 1] = n - 1
    p = p.astype(np.int64)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def operand(rows, C, seed=0):
    rng = np.random.Generator(np.random.PCG64(100000 * seed + 1000 * C + rows))
    x = rng.standard_normal((rows, C)).astype(np.float32)
    if C >= 2:
        x[:, C - 1] *= np.float32(1e4)
    if C >= 3:
        x[:, C - 2] *= np.float32(1e-6)
    x.setflags(write=False)
    return x


# ---- fp64 truth -----------------------------------------------------------------------------------------------------------------
def scales64(pos, n, mode):
    cnt = valid_of(pos, n).sum(1).astype(np.float64)
    if mode == "mean":
        return 1.0 / np.maximum(cnt, 1.0)
    if mode == "size":
        return np.where(cnt > 0, 1.0 / np.sqrt(np.maximum(cnt, 1.0)), 0.0)
    return np.ones_like(cnt)


def scales32(pos, n, mode, count_off=0):
    """pool_scale in fp32: 1.0f / (float)cnt, 1.0f / sqrtf((float)cnt); count_off: a mistake, added to every count"""
    cnt = (valid_of(pos, n).sum(1) + count_off).astype(np.float32)
    one = np.float32(1)
    if mode == "mean":
        return one / np.maximum(cnt, one)
    if mode == "size":
        return np.where(cnt > 0, one / np.sqrt(np.maximum(cnt, one)), np.float32(0)).astype(np.float32)
    return np.ones_like(cnt)


def forward_truth(emb, pos, mode):
    """sum | mean | size -> (want, mass) fp64 [B, C]: padding dropped, duplicates count"""
    n = emb.shape[0]
    e = np.asarray(emb, dtype=np.float64)
    sc = scales64(pos, n, mode)
    want, mass = np.zeros((pos.shape[0], e.shape[1])), np.zeros((pos.shape[0], e.shape[1]))
    for b, row in enumerate(pos):
        v = e[row[valid_of(row, n)]]
        want[b], mass[b] = sc[b] * v.sum(0), sc[b] * np.abs(v).sum(0)
    return want, mass


def backward_truth(dout, pos, n, mode):
    """sum | mean | size -> (want, mass fp64 [n, C], entries [n])"""
    ok = valid_of(pos, n)
    rows = np.nonzero(ok)[0]
    g = scales64(pos, n, mode)[:, None] * np.asarray(dout, dtype=np.float64)
    want, mass = np.zeros((n, g.shape[1])), np.zeros((n, g.shape[1]))
    np.add.at(want, pos[ok], g[rows])
    np.add.at(mass, pos[ok], np.abs(g[rows]))
    return want, mass, list_lengths(pos, n)


def max_truth(emb, pos):
    """Closed form -> (out fp32 [B, C], argmax int32 [B, C]): the valid entry with the largest value, the lowest j among equals
    (-0 == +0); a NaN takes its column, the first one; an empty row, or a column whose valid entries are all -inf: 0 and -1."""
    n, C = emb.shape
    out, arg = np.zeros((pos.shape[0], C), dtype=np.float32), np.full((pos.shape[0], C), -1, dtype=np.int32)
    cols = np.arange(C)
    for b, row in enumerate(pos):
        ids = row[valid_of(row, n)]
        if not ids.size:
            continue
        v = emb[ids]
        nan = np.isnan(v)
        j = np.where(nan.any(0), nan.argmax(0), np.where(nan, -np.inf, v).argmax(0))    # argmax: the first of equals
        win = v[j, cols]
        live = ~(win == -np.inf)
        out[b], arg[b] = np.where(live, win, np.float32(0)), np.where(live, ids[j], -1)
    return out, arg


def max_backward_truth(dout, pos, n, arg):
    """-> (want, mass fp64 [n, C], rows holding each node [n])"""
    d = np.asarray(dout, dtype=np.float64)
    want, mass = np.zeros((n, d.shape[1])), np.zeros((n, d.shape[1]))
    b, c = np.nonzero(arg >= 0)
    np.add.at(want, (arg[b, c], c), d[b, c])
    np.add.at(mass, (arg[b, c], c), np.abs(d[b, c]))
    return want, mass, list_lengths(pos, n, dedup=True)


# ---- the kernels' orders in fp32 ----------------------------------------------------------------------------------------------
def forward_f32(emb, pos, mode, aligned=True, skip=(), twice=(), count_off=0):
    """pool_fwd_kernel's order: row slot r adds the entries j = r, r + slots, ... in turn, slot 0 then adds slots 1, 2, ... and
    scales.  skip / twice: (b, j) entries left out / added twice; count_off: added to every count before the scale."""
    n, C = emb.shape
    slots = fwd_build(C, aligned)[2]
    sc = scales32(pos, n, mode, count_off)
    out = np.zeros((pos.shape[0], C), dtype=np.float32)
    for b, row in enumerate(np.where(valid_of(pos, n), pos, -1)):
        part = np.zeros((slots, C), dtype=np.float32)
        for j, node in enumerate(row):
            if node < 0 or (b, j) in skip:
                continue
            for _ in range(2 if (b, j) in twice else 1):
                part[j % slots] = part[j % slots] + emb[node]
        acc = part[0]
        for r in range(1, slots):
            acc = acc + part[r]
        out[b] = acc * sc[b]
    return out


def pair_forward_f32(emb, prs, mode):
    """pair_fwd_kernel: (x + y) * scale, a padding side is 0"""
    n = emb.shape[0]
    ok = valid_of(prs, n)
    x = np.where(ok[:, 0, None], emb[np.where(ok[:, 0], prs[:, 0], 0)], np.float32(0))
    y = np.where(ok[:, 1, None], emb[np.where(ok[:, 1], prs[:, 1], 0)], np.float32(0))
    return ((x + y) * scales32(prs, n, mode)[:, None]).astype(np.float32)


def _entries(pos, n):
    """(b, j) of the valid entries in (b, s) order"""
    return [(int(b), int(j)) for b, j in zip(*np.nonzero(valid_of(pos, n)))]


def scatter_f32(dout, pos, n, mode, fused, skip=(), twice=(), count_off=0):
    """The scatters in fp32, every node's entries taken in (b, s) order.  fused: the ordered kernel's chain acc = fma(dout, scale,
    acc) (the product exact in fp64, one rounding to fp64 and one to fp32: double rounding, which the gate's 25x headroom covers);
    otherwise the atomic kernel's rounded product added with a rounded add."""
    d = np.asarray(dout, dtype=np.float32)
    sc = scales32(pos, n, mode, count_off)
    out = np.zeros((n, d.shape[1]), dtype=np.float32)
    for b, j in _entries(pos, n):
        if (b, j) in skip:
            continue
        node = pos[b, j]
        for _ in range(2 if (b, j) in twice else 1):
            if fused:
                out[node] = (d[b].astype(np.float64) * np.float64(sc[b]) + out[node].astype(np.float64)).astype(np.float32)
            else:
                out[node] = out[node] + d[b] * sc[b]
    return out


MASK64 = (1 << 64) - 1


def _wrap64(v):
    v &= MASK64
    return v - (1 << 64) if v >> 63 else v


class ExactSum:
    """bucket.h's ExactSum in Python integers.  checked = False: the sum wraps at 64 bits (the struct before the range check);
    checked = True: a sum that leaves the 64-bit range sets the sticky mark."""
    MARK = 1 << 50

    def __init__(self, checked=True):
        self.hi, self.lo, self.checked = 0, 0, checked

    def _add_hi(self, v):
        s = self.hi + v
        if self.checked and not -(1 << 63) <= s < (1 << 63):
            self.lo |= self.MARK
        self.hi = _wrap64(s)

    def add(self, v):
        sv = float(np.float32(v)) * 1048576.0
        if not abs(sv) <= 4.0e18:
            self.lo |= self.MARK
            return
        fl = np.floor(sv)
        self.lo += int((sv - fl) * 1099511627776.0)
        self._add_hi(int(fl) + ((self.lo >> 40) & 1))
        self.lo &= ~(1 << 40)

    def merge(self, other):
        """the cross-lane reduction: limbs added, no carry"""
        self._add_hi(other.hi)
        self.lo += other.lo

    def value(self):
        if self.lo >= self.MARK:
            return np.float32("nan")
        return np.float32((float(self.hi) + float(self.lo) * (1.0 / 1099511627776.0)) * (1.0 / 1048576.0))


def exact_gather_f32(dout, pos, n, mode, arg=None, checked=True, skip=(), twice=(), count_off=0, lanes=1):
    """pair_gather_kernel / pool_max_gather_kernel: every node's addends fl32(dout * scale) (max pooling, `arg` given: dout
    where the node is the row's argmax, a node counted once per row) summed in ExactSum.  lanes > 1: the entries dealt to that
    many partial sums which are then merged (the long-list path)."""
    d = np.asarray(dout, dtype=np.float32)
    C = d.shape[1]
    sc = scales32(pos, n, mode, count_off) if arg is None else None
    sums = [[[ExactSum(checked) for _ in range(lanes)] for _ in range(C)] for _ in range(n)]
    turn = np.zeros(n, dtype=np.int64)
    seen = set()
    for b, j in _entries(pos, n):
        node = int(pos[b, j])
        if (b, j) in skip or (arg is not None and (b, node) in seen and (b, j) not in twice):
            continue
        seen.add((b, node))
        for _ in range(2 if (b, j) in twice and arg is None else 1):
            lane = int(turn[node]) % lanes
            turn[node] += 1
            for c in range(C):
                if arg is None:
                    sums[node][c][lane].add(d[b, c] * sc[b])
                elif arg[b, c] == node:
                    sums[node][c][lane].add(d[b, c])
    out = np.zeros((n, C), dtype=np.float32)
    for node in range(n):
        for c in range(C):
            tot = ExactSum(checked)
            for s in sums[node][c]:
                tot.merge(s)
            out[node, c] = tot.value()
    return out


# ---- gates ----------------------------------------------------------------------------------------------------------------------
def share_of_bound(got, want, bound):
    """the largest |got - want| / bound; where the bound is 0 the element must be exact; NaN is an infinite error"""
    got = np.asarray(got.detach().cpu().numpy() if hasattr(got, "detach") else got, dtype=np.float64)
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    d = np.abs(got - want)
    d[np.isnan(d)] = np.inf
    if bool((d[bound == 0] != 0).any()):
        return float("inf")
    live = bound > 0
    return float((d[live] / bound[live]).max()) if bool(live.any()) else 0.0


def float_share(got, want, mass):
    return share_of_bound(got, want, TOL * mass)


def exact_share(got, want, mass, entries, rel=REL_EXACT):
    return share_of_bound(got, want, rel * mass + (np.asarray(entries, dtype=np.float64) * QUANTUM)[:, None] * (mass > 0))


SENTINEL = -777.25   # what the columns beyond C of a wider output row hold before a call


def beyond_columns_intact(full, C):
    """nothing was stored past column C of any row of the [rows, ld] buffer"""
    full = np.asarray(full.detach().cpu().numpy() if hasattr(full, "detach") else full)
    return bool((full[:, C:] == np.float32(SENTINEL)).all())


def max_forward_ok(out, arg, want_out, want_arg):
    """`out` equals the winner's fp32 value under == (a NaN winner: NaN), `arg` its node id"""
    out, arg = np.asarray(out), np.asarray(arg)
    return bool((((out == want_out) | (np.isnan(out) & np.isnan(want_out))).all()) and np.array_equal(arg, want_arg))
