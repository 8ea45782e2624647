"""K7's pooling kernels without a GPU: the recipes of tests/pool_oracle.py hold what they claim, its restatements of the
dispatch agree with the constants in glass_amd/csrc/pool.hip, the widths of tests/test_gpu_pool.py name every build, every gate
passes the fp32 restatement of the kernel it grades (and prints the worst share of the bound) and refuses each single mistake,
and ExactSum in Python integers shows the 64-bit wrap and the range check that ends it."""
import numpy as np
import pytest

import pool_oracle as P

B, SMAX, N, C = 37, 40, 300, 5


# ---- recipes and dispatch -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Smax", P.FWD_SMAX)
def test_recipe_ragged(Smax):
    n = max(N, Smax + 8)
    pos, f = P.ragged(B, Smax, n)
    ok = P.valid_of(pos, n)
    cnt = ok.sum(1)
    assert pos.shape == (B, Smax) and cnt[f["empty"]] == 0 and cnt[f["single"]] == 1 and int(cnt.max()) <= Smax
    assert int(cnt.min()) == 0 and (Smax == 1 or int(cnt.max()) > 1)
    b0, b1, node = f["shared"]
    assert node in pos[b0] and node in pos[b1]
    lengths = P.list_lengths(pos, n)
    assert lengths[f["unused"]] == 0 and lengths[n - 1] >= 1 and lengths[node] >= 2
    if Smax >= 2:
        b, node = f["dup"]
        assert int((pos[b] == node).sum()) == 2 and P.list_lengths(pos, n, dedup=True)[node] == lengths[node] - 1
    if Smax >= 3:
        assert pos[f["lead_pad"], 0] == -1 and cnt[f["lead_pad"]] == 2
        assert int((pos[f["beyond"]] >= n).sum()) == 1 and cnt[f["beyond"]] == 2
    if Smax > P.BLOCK:
        assert int(cnt.max()) > P.BLOCK, "count_valid's second round holds valid entries"


@pytest.mark.parametrize("Smax", P.FWD_SMAX)
def test_recipe_ties(Smax):
    n = max(N, Smax + 8)
    pos, emb, last_row = P.ties(B, Smax, n, 16)
    assert set(np.unique(emb).tolist()) <= {-1.0, -0.5, 0.0, 0.5, 1.0, 2.0}
    assert bool((np.signbit(emb) & (emb == 0)).any()) and bool((~np.signbit(emb) & (emb == 0)).any()), "+0 and -0"
    assert float(emb[:, 1::5].max()) == 0.0, "columns without a positive value"
    out, arg = P.max_truth(emb, pos)
    # (b, c) whose maximum is held by two or more different nodes
    tied = total = 0
    for b, row in enumerate(pos):
        ids = np.unique(row[P.valid_of(row, n)])
        if ids.size < 2:
            continue
        tied += int(((emb[ids] == out[b]).sum(0) >= 2).sum())
        total += emb.shape[1]
    print(f"ties Smax={Smax}: {tied} of {total} (row, column) maxima are shared by different nodes")
    assert Smax < 3 or tied >= total // 5
    assert Smax < 40 or tied >= total // 2
    if Smax >= 40:
        assert bool((out[:, 1::5][P.valid_of(pos, n).sum(1) > 8] == 0).all()), "zero is the maximum of the negative columns"
    ids = pos[last_row]
    assert bool(P.valid_of(ids, n).all()) and emb[ids[-1], 0] == 2.0 and (Smax == 1 or float(emb[ids[:-1], 0].max()) < 2.0)
    assert arg[last_row, 0] == ids[-1] and out[last_row, 0] == 2.0


def test_recipe_lists():
    pos, n = P.lists(), P.LISTS_N
    assert pos.shape == (P.LISTS_B, P.LISTS_SMAX) and P.bwd_form(P.LISTS_B, P.LISTS_SMAX, "sum") == "exact"
    lengths = P.list_lengths(pos, n)
    assert np.array_equal(lengths, P.list_lengths(pos, n, dedup=True)), "a node's entries are in distinct rows"
    for node, L in P.LISTS_SPECIAL.items():
        assert lengths[node] == L, (node, L)
    assert set(P.LISTS_SPECIAL.values()) >= {0, 1, 62, 63, 64, 65, 200, P.LISTS_B}
    assert bool((pos == 7).any(1).all()), "node 7 is in every row"
    others = np.delete(lengths, list(P.LISTS_SPECIAL))
    assert int(others.max()) <= 5
    long = lengths >= P.PAIR_LONG_LIST
    for C_, vec in P.LIST_WIDTHS:
        per = P.BLOCK // P.pair_group(C_, vec)
        assert long[0] and not long[1] and not long[2] and long[3] and per >= 4, "two long nodes, short ones between, one workgroup"
        assert n % per != 0 and bool(long[n - n % per:].any()), "the last workgroup is partly filled and holds a long node"
    assert {P.pair_group(C_, vec) for C_, vec in P.LIST_WIDTHS} == {1, 32, 16, 64}
    assert [P.BLOCK // P.pair_group(C_, vec) for C_, vec in P.LIST_WIDTHS if C_ in (4, 320)] == [256, 4]


def test_recipe_pairs():
    Bp, n = 1003, 600
    p = P.pairs(Bp, n)
    assert p[1, 0] != p[1, 1] and p[2, 0] == p[2, 1] and tuple(p[3]) == (-1, 23) and tuple(p[4]) == (24, -1) and tuple(p[5]) == (-1, -1)
    assert bool((p[::7, 0] == 11).all()) and P.list_lengths(p, n)[11] >= Bp // 7 >= 2 * P.PAIR_LONG_LIST
    lengths = P.list_lengths(p, n)
    assert lengths[n - 1] >= 1 and bool((lengths[n - 10:n - 1] == 0).all()) and lengths[22] >= 2
    for G in (1, 2, 4, 8, 16, 32, 64):
        assert Bp % (P.BLOCK // G) != 0


def test_the_restatements_agree_with_the_source_text():
    k = P.source_constants()
    assert (k["kBlock"], k["kWave"]) == (P.BLOCK, P.WAVE)
    assert k["kPoolOrderedMax"] == P.POOL_ORDERED_MAX and k["kPairLongList"] == P.PAIR_LONG_LIST
    assert k["pair_group_cap"] == P.PAIR_GROUP_CAP and k["fwd_cap_is_kBlock"]
    from glass_amd import ops
    assert ops.POOL_ORDERED_MAX == P.POOL_ORDERED_MAX and ops.POOL_MODES == P.MODES


def test_the_widths_name_every_build():
    vec = {C_: P.fwd_build(C_) for C_ in P.FWD_VEC}
    sca = {C_: P.fwd_build(C_) for C_ in P.FWD_SCALAR}
    assert vec == {4: (4, 1, 256, 1), 8: (4, 2, 128, 1), 64: (4, 16, 16, 1), 512: (4, 128, 2, 1), 1024: (4, 256, 1, 1),
                   1028: (4, 256, 1, 2)}
    assert sca == {1: (1, 1, 256, 1), 3: (1, 4, 64, 1), 17: (1, 32, 8, 1), 255: (1, 256, 1, 1), 257: (1, 256, 1, 2)}
    assert P.fwd_build(64, aligned=False) == (1, 64, 4, 1), "a misaligned view at a vector width"
    # both sides of the column-tile limits: 4 * 256 and 256 columns
    assert P.fwd_build(1024)[3] == 1 and P.fwd_build(1028)[3] == 2 and P.fwd_build(256, False)[3] == 1 and P.fwd_build(257, False)[3] == 2
    assert [P.pair_group(C_, True) for C_ in P.PAIR_VEC] == [1, 2, 16, 64, 64] and 320 // 4 > 64, "G = 1 .. 64, then the column loop"
    assert [P.pair_group(C_, False) for C_ in P.PAIR_SCALAR] == [1, 4, 32, 64, 64] and 65 > 64
    # count_valid's second round, and the backward forms on both sides of kPoolOrderedMax
    assert max(P.FWD_SMAX) > P.BLOCK > sorted(P.FWD_SMAX)[-2]
    assert 384 * 31 + 384 == P.POOL_ORDERED_MAX and P.bwd_form(384, 31, "sum") == "ordered" and P.bwd_form(385, 31, "sum") == "exact"
    assert P.bwd_form(37, 2, "max") == "max_exact" and P.bwd_form(1003, 2, "mean") == "pair" and P.bwd_form(385, 31, "max") == "max_exact"


# ---- the gates --------------------------------------------------------------------------------------------------------------------
def _first_entry(pos, n, b):
    return b, int(np.flatnonzero(P.valid_of(pos[b], n))[0])


def _long_row(pos, n):
    return int(P.valid_of(pos, n).sum(1).argmax())


def _shift(honest, c=1):
    bad = honest.copy()
    bad[:, c] = honest[:, c + 1]
    return bad


@pytest.mark.parametrize("mode", ("sum", "mean", "size"))
def test_forward_gate(mode):
    pos, f = P.ragged(B, SMAX, N)
    emb = P.operand(N, C)
    want, mass = P.forward_truth(emb, pos, mode)
    assert bool((mass[f["empty"]] == 0).all()) and bool((np.delete(mass, f["empty"], 0) > 0).all())
    honest = P.forward_f32(emb, pos, mode, aligned=False)
    share = P.float_share(honest, want, mass)
    print(f"forward {mode}: the slot-then-LDS order in fp32 is at {share:.3f} of its bound")
    assert share <= 0.5
    e = _first_entry(pos, N, _long_row(pos, N))
    bad = {"an entry dropped": P.forward_f32(emb, pos, mode, False, skip={e}),
           "an entry twice": P.forward_f32(emb, pos, mode, False, twice={e}),
           "the duplicate counted once": P.forward_f32(emb, pos, mode, False, skip={(f["dup"][0], 1)}),
           "a column shifted": _shift(honest)}
    if mode != "sum":
        bad["a count off by one"] = P.forward_f32(emb, pos, mode, False, count_off=1)
    one = honest.copy()
    one[f["empty"], 2] = 1e-30
    bad["an empty row not zero"] = one
    one = honest.copy()
    one[f["single"], 0] = np.nan
    bad["a NaN"] = one
    for what, got in bad.items():
        s = P.float_share(got, want, mass)
        print(f"forward {mode}: {what}: {s:.3g} of the bound")
        assert s > 10, what


@pytest.mark.parametrize("mode", ("sum", "mean", "size"))
def test_pair_forward_gate(mode):
    prs, n = P.pairs(1003, 600), 600
    emb = P.operand(n, C)
    want, mass = P.forward_truth(emb, prs, mode)
    honest = P.pair_forward_f32(emb, prs, mode)
    share = P.float_share(honest, want, mass)
    print(f"pair forward {mode}: fp32 is at {share:.3f} of its bound")
    assert share <= 0.5 and bool((honest[5] == 0).all())
    half = honest.copy()
    half[2] = (emb[prs[2, 0]] * P.scales32(prs, n, mode)[2]).astype(np.float32)     # (a, a) counted once
    assert P.float_share(half, want, mass) > 10
    one_sided = honest.copy()
    one_sided[3] = honest[3] * np.float32(0.5 if mode == "sum" else 2.0 ** -0.5)      # (-1, b) scaled as if it had two entries
    assert P.float_share(one_sided, want, mass) > 10
    assert P.float_share(_shift(honest), want, mass) > 10


@pytest.mark.parametrize("fused", (True, False), ids=("ordered", "atomic"))
@pytest.mark.parametrize("mode", ("sum", "mean", "size"))
def test_scatter_gate(mode, fused):
    pos, f = P.ragged(B, SMAX, N)
    dout = P.operand(B, C, seed=1)
    want, mass, entries = P.backward_truth(dout, pos, N, mode)
    assert bool((mass[entries == 0] == 0).all()) and bool((mass[entries > 0] > 0).all())
    honest = P.scatter_f32(dout, pos, N, mode, fused)
    share = P.float_share(honest, want, mass)
    print(f"{'ordered' if fused else 'atomic'} scatter {mode}: fp32 in (b, s) order is at {share:.3f} of its bound")
    assert share <= 0.5
    e = _first_entry(pos, N, _long_row(pos, N))
    bad = {"an entry dropped": P.scatter_f32(dout, pos, N, mode, fused, skip={e}),
           "an entry twice": P.scatter_f32(dout, pos, N, mode, fused, twice={e}),
           "the duplicate counted once": P.scatter_f32(dout, pos, N, mode, fused, skip={(f["dup"][0], 1)}),
           "a column shifted": _shift(honest)}
    if mode != "sum":
        bad["a count off by one"] = P.scatter_f32(dout, pos, N, mode, fused, count_off=1)
    one = honest.copy()
    one[f["unused"], 3] = -1e-30
    bad["an unnamed node not zero"] = one
    for what, got in bad.items():
        assert P.float_share(got, want, mass) > 10, what


@pytest.mark.parametrize("mode", ("sum", "mean", "size"))
def test_exact_gate(mode):
    """The bucketed gather on `ragged` (short lists) and on three columns of `lists` (lists of 64 .. 400 entries through 256
    merged partial sums, as the long-list path forms them)."""
    worst = 0.0
    for pos, n, lanes, Bq in ((P.ragged(B, SMAX, N)[0], N, 1, B), (P.lists(), P.LISTS_N, 256, P.LISTS_B)):
        dout = P.operand(Bq, 3, seed=2)
        want, mass, entries = P.backward_truth(dout, pos, n, mode)
        honest = P.exact_gather_f32(dout, pos, n, mode, lanes=lanes)
        assert np.array_equal(honest, P.exact_gather_f32(dout, pos, n, mode, lanes=1, checked=False)), "order and lanes do not matter"
        share = P.exact_share(honest, want, mass, entries)
        worst = max(worst, share)
        assert share <= 0.5, (mode, share)
        long_node = int(entries.argmax())
        b = int(np.flatnonzero((pos == long_node).any(1))[0])
        e = (b, int(np.flatnonzero(pos[b] == long_node)[0]))
        bad = {"an entry dropped": P.exact_gather_f32(dout, pos, n, mode, skip={e}),
               "an entry twice": P.exact_gather_f32(dout, pos, n, mode, twice={e}), "a column shifted": _shift(honest)}
        if mode != "sum":
            bad["a count off by one"] = P.exact_gather_f32(dout, pos, n, mode, count_off=1)
        one = honest.copy()
        one[int(np.flatnonzero(entries == 0)[0]), 0] = 1e-30
        bad["a node without entries not zero"] = one
        for what, got in bad.items():
            assert P.exact_share(got, want, mass, entries) > 10, (mode, what)
    print(f"exact gather {mode}: ExactSum of the fp32 addends is at {worst:.3f} of its bound (rel 2^-21)")


def test_max_gates():
    pos, emb, last_row = P.ties(B, SMAX, N, 16)
    out, arg = P.max_truth(emb, pos)
    assert P.max_forward_ok(out, arg, out, arg)
    # a tie given to the second entry: same value, another node
    b = c = None
    for b in range(B):
        ids = pos[b][P.valid_of(pos[b], N)]
        hit = [(c, ids[np.flatnonzero(emb[ids, c] == out[b, c])]) for c in range(16)]
        hit = [(c, h) for c, h in hit if np.unique(h).size >= 2]
        if hit:
            c, h = hit[0]
            second = int(h[h != arg[b, c]][0])
            break
    bad_arg = arg.copy()
    bad_arg[b, c] = second
    assert emb[second, c] == out[b, c] and not P.max_forward_ok(out, bad_arg, out, arg), "a tie given to the second entry"
    bad_out = out.copy()
    bad_out[last_row, 0] = 1.0
    assert not P.max_forward_ok(bad_out, arg, out, arg), "the maximum at the last j missed"
    neg0 = out.copy()
    neg0[out == 0] = -0.0
    assert P.max_forward_ok(neg0, arg, out, arg), "-0 and +0 tie: values compare under =="
    assert not P.max_forward_ok(_shift(out), arg, out, arg) or np.array_equal(out[:, 1], out[:, 2])
    # NaN takes its column (the first one), a column of -inf only reports 0 and -1
    e2 = emb.copy()
    ids = pos[last_row]
    e2[ids[3], 4] = e2[ids[7], 4] = np.nan
    e2[ids, 5] = -np.inf
    o2, a2 = P.max_truth(e2, pos)
    assert np.isnan(o2[last_row, 4]) and a2[last_row, 4] == ids[3] and o2[last_row, 5] == 0 and a2[last_row, 5] == -1
    # backward: exact sums of dout over the rows a node won
    dout = P.operand(B, 16, seed=3)
    want, mass, rows = P.max_backward_truth(dout, pos, N, arg)
    honest = P.exact_gather_f32(dout, pos, N, "max", arg=arg)
    share = P.exact_share(honest, want, mass, rows, P.REL_MAX)
    print(f"max gather: ExactSum of dout is at {share:.3f} of its bound (rel 2^-23)")
    assert share <= 0.5
    assert P.exact_share(P.exact_gather_f32(dout, pos, N, "max", arg=bad_arg), want, mass, rows, P.REL_MAX) > 10, "the tie's gradient"
    dup_b, dup_node = P.ragged(B, SMAX, N)[1]["dup"]
    assert bool((arg[dup_b] == dup_node).any())
    twice = P.exact_gather_f32(dout, pos, N, "max", arg=arg, twice={(dup_b, 1)})
    assert P.exact_share(twice, want, mass, rows, P.REL_MAX) > 10, "a node named twice by a row counted twice"
    assert P.exact_share(_shift(honest), want, mass, rows, P.REL_MAX) > 10


def test_a_row_written_beyond_c_is_refused():
    full = np.full((B, C + 4), P.SENTINEL, dtype=np.float32)
    full[:, :C] = 1.0
    assert P.beyond_columns_intact(full, C)
    full[B - 1, C] = 0.0
    assert not P.beyond_columns_intact(full, C)


# ---- ExactSum ---------------------------------------------------------------------------------------------------------------------
def _sum_of(values, checked, lanes=1):
    parts = [P.ExactSum(checked) for _ in range(lanes)]
    for i, v in enumerate(values):
        parts[i % lanes].add(v)
    tot = P.ExactSum(checked)
    for p in parts:
        tot.merge(p)
    return tot.value()


@pytest.mark.parametrize("values,lanes", [([3e12] * 4, 1), ([2e11] * 80, 1), ([2e11] * 80, 256), ([-3e12] * 4, 1)],
                         ids=("4x3e12", "80x2e11", "80x2e11-merged", "4x-3e12"))
def test_exact_sum_wraps_without_the_range_check_and_not_with_it(values, lanes):
    true = float(np.sum(np.asarray(values, dtype=np.float32).astype(np.float64)))
    assert abs(true) * 2.0**20 > 2.0**63 and all(abs(v) * 2.0**20 <= 4.0e18 for v in values), "every addend is accepted"
    wrapped = float(_sum_of(values, checked=False, lanes=lanes))
    print(f"sum {true:.4g}: 64-bit wrap gives {wrapped:.4g}")
    assert np.isfinite(wrapped) and abs(wrapped - true) > 0.5 * abs(true), "finite, wrong"
    assert np.isnan(_sum_of(values, checked=True, lanes=lanes)), "the range check marks it"


def test_exact_sum_in_range_is_unchanged_by_the_check():
    rng = np.random.Generator(np.random.PCG64(9))
    v = (rng.standard_normal(500) * 10.0 ** rng.integers(-8, 9, 500)).astype(np.float32)
    for lanes in (1, 64):
        a, b = _sum_of(v, False, lanes), _sum_of(v, True, lanes)
        assert a == b == _sum_of(v[::-1], True, 7), "order and lanes do not reach the result"
        assert abs(float(a) - float(v.astype(np.float64).sum())) <= 2.0**-24 * float(np.abs(v).sum()) + 500 * P.QUANTUM
    big = [2.0**41] * 4                   # 2^43 * 2^20 = 2^63: one past the largest sum
    assert np.isnan(_sum_of(big, True)) and float(_sum_of(big[:3], True)) == 3 * 2.0**41 and float(_sum_of([-2.0**41] * 4, True)) == -2.0**43
    assert np.isnan(_sum_of([1.0, np.inf], True)) and np.isnan(_sum_of([np.nan], True)) and np.isnan(_sum_of([1e13], True))
