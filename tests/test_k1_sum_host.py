"""K1's sum kernels without a GPU: the plans that tests/test_gpu_k1_sum.py launches (glass_spmm_plan_build is host code) take
the forms that module claims, its widths name every build of GLASS_K1_WIDTH_DISPATCH, and the gate of tests/k1_sum_oracle.py
passes honest fp32 arithmetic and refuses single dropped entries."""
import numpy as np
import pytest
import torch

import k1_sum_oracle as K


@pytest.mark.parametrize("transposed", (False, True))
def test_plan_of_the_mixed_graph(transposed):
    rp, _col, _val = K.csr("mixed", transposed)
    p = K.Plan(rp)
    h, deg = p.header, np.diff(rp)
    assert h[K.H_NROWS] == 1007 and h[K.H_LONG_THR] == 64 and h[K.H_LONG_CHUNK] == 256 and h[K.H_NSWEEP] > 100
    assert h[K.H_NSWEEP] < K.FLAT_MIN_ITEMS, "every width takes the row-only sweep build"
    if not transposed:
        assert list(deg[:10]) == [0, 1, 2, 63, 64, 65, 255, 256, 257, 700]
        assert h[K.H_NLONG] >= 9 and p.reduce.tolist() == [[8, 0, 2], [9, 2, 3]], "two cut rows, 2 + 3 partial slots"
        assert h[K.H_NSLOTS] == 5
    else:
        assert int(deg[5]) > 512 and p.reduce.tolist() == [[5, 0, 3]] and h[K.H_NLONG] >= 3, "the hub's transposed row is cut"
        assert h[K.H_NSLOTS] == 3
    assert int((deg == 0).sum()) >= 1
    # the sweep items and the long items tile the short and the long rows
    assert all(int(deg[r]) >= 64 for r in p.long[:, 0]) and int((deg >= 64).sum()) == len(set(p.long[:, 0].tolist()))
    assert int((p.sweep[:, 1] - p.sweep[:, 0]).sum()) == int((deg < 64).sum())


@pytest.mark.parametrize("transposed", (False, True))
def test_plan_of_the_all_long_graph(transposed):
    rp, _col, _val = K.csr("all_long", transposed)
    p = K.Plan(rp)
    h, deg = p.header, np.diff(rp)
    assert h[K.H_NROWS] == 42 and h[K.H_NSWEEP] == 0 and h[K.H_LONG_THR] == 0, "no sweep item: the stand-alone long kernel"
    assert h[K.H_NLONG] >= 42 and h[K.H_NREDUCE] >= 1 and h[K.H_NSLOTS] >= 2
    assert sorted(set(p.long[:, 0].tolist())) == list(range(42)), "every row is workgroup items, the empty ones included"
    assert int(deg.max()) >= 700 and (transposed or int((deg == 0).sum()) >= 1)


@pytest.mark.parametrize("transposed", (False, True))
def test_plan_of_the_flat_graph(transposed):
    """The smallest shape at which a launch takes the flat-capable sweep build, with both kinds of item in it, long items in
    the same launch and a cut row.  The transposed matrix meets the same conditions (the sources are drawn for it)."""
    rp, _col, _val = K.csr("flat", transposed)
    p = K.Plan(rp)
    h, deg = p.header, np.diff(rp)
    assert 24000 <= h[K.H_NROWS] <= 32000 and h[K.H_NNZ] + 4 * h[K.H_NROWS] < (2 << 20)
    assert h[K.H_NSWEEP] >= K.FLAT_MIN_ITEMS and h[K.H_RP_FACTOR] == 4 and h[K.H_LONG_THR] == 64
    assert h[K.H_NLONG] >= 1 and h[K.H_NREDUCE] >= 1 and h[K.H_NSLOTS] >= 2
    assert sorted(deg[deg >= 64].tolist()) == [64, 65, 100, 300, 600] and int((deg == 63).sum()) >= 1
    for G in (2, 4, 8, 16, 64):
        assert K.flat_share15(h, G) >= K.FLAT_MIN_SHARE15 and K.takes_flat_build(h, G), G
    assert not K.takes_flat_build(h, 1), "one lane group per wave (H >= 256): the row-only build"
    n_items = p.sweep.shape[0]
    for G in (2, 4):
        ok = K.flat_eligible(p.sweep, int(h[K.H_RP_FACTOR]), G)
        assert int(ok.sum()) >= n_items / 10 and int((~ok).sum()) >= n_items / 10, (G, int(ok.sum()), n_items)
    # flat items of several rows, empty rows among them (a row boundary flushes the accumulator)
    rows_per = p.sweep[:, 1] - p.sweep[:, 0]
    assert int((rows_per >= 3).sum()) >= 1000 and int((deg == 0).sum()) >= 1000
    print(f"flat{' transposed' if transposed else ''}: {n_items} sweep items, {h[K.H_NLONG]} long items, shares (G = 1 .. 64) "
          f"{[K.flat_share15(h, 1 << k) for k in range(7)]}")


def test_plan_of_the_flat_runs_graph():
    """Runs of rows per lane group in flat mode's equal-row-count split (G > 8): per = ceil(rows / G) exceeds one only in items of
    more than G rows.  At the smallest budget (16 cost units, 4 per row) an item holds at most four rows, which is every plan of
    fewer than about 500 000 cost units, `flat` included; this plan's budget packs more than 16 rows into most items."""
    rp, _col, _val = K.csr("flat_runs")
    p = K.Plan(rp)
    h, deg = p.header, np.diff(rp)
    rows_per = p.sweep[:, 1] - p.sweep[:, 0]
    assert h[K.H_NSWEEP] >= K.FLAT_MIN_ITEMS and K.takes_flat_build(h, 16) and h[K.H_NLONG] == 0 and int(deg.max()) <= 2
    assert bool(K.flat_eligible(p.sweep, int(h[K.H_RP_FACTOR]), 16).all())
    assert int((rows_per > 16).sum()) >= p.sweep.shape[0] // 2 and int(rows_per.max()) <= 64
    assert int((deg == 0).sum()) >= 300000
    rp_flat = K.csr("flat")[0]
    assert int((K.Plan(rp_flat).sweep[:, 1] - K.Plan(rp_flat).sweep[:, 0]).max()) <= 4, "`flat` never gives a group of 16 two rows"
    print(f"flat_runs: {p.sweep.shape[0]} sweep items, rows per item median {int(np.median(rows_per))}, largest {int(rows_per.max())}")


@pytest.mark.parametrize("H", (8, 64, 128, 17))
def test_plan_of_the_short_row_test_in_test_gpu_kernels(H):
    """test_spmm_row_parallel_mode_for_short_rows (tests/test_gpu_kernels.py) rebuilt on the host: 6 000 rows of 0 .. 3 entries
    and two of 300 give about 2 500 sweep items, fewer than the 8 192 the flat-capable build asks for — that test runs short
    rows in ROW mode (and asserts so from the header); flat mode is tests/test_gpu_k1_sum.py's."""
    rng = np.random.default_rng(H)
    n = 6000
    rows = np.repeat(np.arange(n), rng.integers(0, 4, n))
    cols = rng.integers(0, n, rows.shape[0])
    rows = np.concatenate([rows, np.repeat(np.array([17, 3000]), 300)])
    cols = np.concatenate([cols, rng.integers(0, n, 600)])
    for keys, n_long in ((rows, 2), (cols, 0)):
        rp = np.zeros(n + 1, dtype=np.int64)
        rp[1:] = np.cumsum(np.bincount(keys, minlength=n))
        h = K.Plan(rp.astype(np.int32)).header
        assert 2000 < h[K.H_NSWEEP] < 3000 and h[K.H_NLONG] == n_long and h[K.H_NREDUCE] == 0
        assert not any(K.takes_flat_build(h, G) for G in (1, 2, 4, 8, 16, 32, 64))


def test_the_widths_name_every_build():
    builds = {K.build_of(H, True)[:2] for H in K.VEC_WIDTHS} | {K.build_of(H, False)[:2] for H in K.SCALAR_WIDTHS}
    assert builds == {(vw, lpr) for vw in (4, 1) for lpr in (1, 2, 4, 8, 16, 32, 64)}
    assert [K.build_of(H, True) for H in (256, 260, 520)] == [(4, 64, 1), (4, 64, 2), (4, 64, 3)]
    assert [K.build_of(H, False) for H in (33, 100, 130)] == [(1, 64, 1), (1, 64, 2), (1, 64, 3)]
    assert [64 // K.build_of(H, True)[1] for H in K.FLAT_VEC_WIDTHS] == [64, 16, 8, 4, 2]
    assert K.build_of(17, False)[:2] == (1, 32) and K.build_of(256, True)[:2] == (4, 64)


def _row_with(deg, d):
    return int(np.flatnonzero(deg == d)[0])


@pytest.mark.parametrize("kind", K.KINDS)
def test_the_gate_passes_plain_fp32_and_refuses_one_dropped_entry(kind):
    """H = 17.  The fp32 product in CSR order passes at far below the bar; each of the four mistakes alone fails it."""
    H = 17
    rp, col, val = K.csr(kind)
    X = K.operand(kind, H).numpy()
    want, mass = K.product(rp, col, val, X)
    deg = np.diff(rp)
    assert bool((mass[torch.from_numpy(deg == 0)] == 0).all()) and bool((mass[torch.from_numpy(deg > 0)] > 0).all())
    honest = K.product_f32(rp, col, val, X)
    worst = K.of_mass(honest, want, mass)
    print(f"{kind}: the fp32 product in CSR order is within {worst:.2e} of its mass (bar {K.TOL:g})")
    assert worst <= K.TOL / 10
    # an element without mass must be exact
    bad = honest.copy()
    bad[_row_with(deg, 0), 3] = 1e-30
    assert K.of_mass(bad, want, mass) == float("inf")
    bad[_row_with(deg, 0), 3] = float("nan")
    assert K.of_mass(bad, want, mass) == float("inf")
    mistakes = {}
    long_row = _row_with(deg, 700 if kind != "flat" else 600)
    mistakes["an entry of the longest row"] = K.product_f32(rp, col, val, X, skip=[int(rp[long_row]) + 300])
    if kind == "mixed":
        mistakes["an entry of the 2-entry row"] = K.product_f32(rp, col, val, X, skip=[int(rp[2]) + 1])
        one = honest.copy()
        one[1, 4] = one[1, 5]
        mistakes["a column of the 1-entry row"] = one
    p = K.Plan(rp)
    row, first, slots = p.reduce[-1].tolist()
    assert row == long_row and slots >= 2
    _r, e0, e1, slot = [it for it in p.long.tolist() if it[3] == first + slots - 1][0]   # the row's LAST chunk: its shortest
    assert _r == row and e1 == rp[row + 1]
    mistakes["the partial of one chunk"] = K.product_f32(rp, col, val, X, skip=range(e0, e1))
    for what, got in mistakes.items():
        e = K.of_mass(got, want, mass)
        print(f"{kind}: without {what}: {e:.2e}")
        assert e > 10 * K.TOL, what
