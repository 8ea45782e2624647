"""Host side of the narrow dense tests (no GPU): tests/narrow_dense_oracle.py against torch fp64 autograd, and the shape list of
tests/test_gpu_narrow_dense.py against the geometry each entry is named for (the library's host functions)."""
import pytest
import torch

import narrow_dense_oracle as NO
from helpers import rel_inf
from oracle import glass_oracle as O


def _lib():
    from glass_amd import _lib
    return _lib.load()


@pytest.mark.parametrize("comb", [False, True])
@pytest.mark.parametrize("H", [1, 9, 17, 32])
@pytest.mark.parametrize("pattern", ["random", "last"])
def test_pair_is_the_autograd_composition(H, comb, pattern):
    """fwd -> dgrad / wgrad == fp64 autograd through nn.functional.linear, ELU and the oracle's mix"""
    N, z = 77, 0.85
    p = NO.make_pair(H, N, comb, pattern=pattern)
    act = p["act"]
    xa = p["xa"].double().requires_grad_(True)
    xb = p["xb"].double().requires_grad_(True) if comb else None
    W, b = p["W"].double().requires_grad_(True), p["b"].double().requires_grad_(True)
    Z = torch.nn.functional.linear(torch.cat((xa, xb), 1) if comb else xa, W, b)
    A = torch.nn.functional.elu(Z) if act == NO.ACT_ELU else Z
    ref = O._mix(p["mask"].bool().reshape(-1, 1), z, A[:, :H], A[:, H:])
    ref.backward(p["dsrc"].double())
    T, out = NO.fwd(p["xa"], p["xb"], p["W"], p["b"], p["mask"], z, act)
    assert rel_inf(T, Z.detach()) < 1e-12 and rel_inf(out, ref.detach()) < 1e-12
    din = NO.dgrad(p["dsrc"], T, p["W"], p["mask"], z, act, p["n_out"])
    assert rel_inf(din[:, :H], xa.grad) < 1e-12
    if comb:
        assert rel_inf(din[:, H:], xb.grad) < 1e-12
    with_add = NO.dgrad(p["dsrc"], T, p["W"], p["mask"], z, act, p["n_out"], p["addend"])
    assert rel_inf(with_add - p["addend"].double(), din) < 1e-12
    dW, db = NO.wgrad(p["dsrc"], T, p["mask"], z, act, p["xa"], p["xb"])
    assert rel_inf(dW, W.grad) < 1e-12 and rel_inf(db, b.grad) < 1e-12
    aW, ab = NO.wgrad_abs(p["dsrc"], T, p["mask"], z, act, p["xa"], p["xb"])
    assert bool((aW >= dW.abs() * (1 - 1e-12)).all()) and bool((ab >= db.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("H,N", [(1, 257), (9, 300), (17, 1025), (32, 256)])
@pytest.mark.parametrize("act", [NO.ACT_NONE, NO.ACT_ELU])
def test_block_sums_are_the_graphnorm_column_sums(H, N, act):
    """`stats` summed over blocks gives the mean and variance a GraphNorm forward needs; `gn_partials` summed over blocks gives
    d beta and d gamma of y = act((x - alpha mean) rstd gamma + beta) under fp64 autograd (the two sums its backward needs)."""
    gen = torch.Generator().manual_seed(H * 7 + N)
    eps = 1e-5
    x = (torch.randn(N, H, generator=gen) * 2 + 0.5)
    gamma = (torch.rand(H, generator=gen) + 0.5).double().requires_grad_(True)
    beta = (torch.randn(H, generator=gen) * 0.3).double().requires_grad_(True)
    alpha = (torch.rand(H, generator=gen) * 0.4 + 0.7).double().requires_grad_(True)
    g = torch.randn(N, H, generator=gen)
    x64 = x.double().requires_grad_(True)
    mean = x64.mean(0)
    cen = x64 - alpha * mean
    var = (cen * cen).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    pre = cen * rstd * gamma + beta
    y = torch.nn.functional.elu(pre) if act == NO.ACT_ELU else pre
    y.backward(g.double())
    # forward sums -> the statistics
    st = NO.stats(x)
    assert st.shape == (NO.blocks(N, NO.ROWS), 2, H)
    S1, S2 = st[:, 0].sum(0), st[:, 1].sum(0)
    m = S1 / N
    a = alpha.detach()
    v = S2 / N - (2 * a - a * a) * m * m
    assert rel_inf(m, mean.detach()) < 1e-12 and rel_inf(v, var.detach()) < 1e-11
    assert bool((NO.stats_abs(x)[:, 0].sum(0) >= S1.abs()).all())
    # saved = [mean, rstd, scale, shift]: x * scale + shift is the pre-activation
    scale = (gamma * rstd).detach()
    saved = torch.cat((mean.detach(), rstd.detach(), scale, (beta - a * mean * gamma * rstd).detach()))
    assert rel_inf(NO.prologue(x, saved, act), y.detach()) < 1e-12
    part = NO.gn_partials(g, x, saved, a, act)
    assert part.shape == (NO.blocks(N, NO.ROWS), 2, H)
    assert rel_inf(part[:, 0].sum(0), beta.grad) < 1e-12 and rel_inf(part[:, 1].sum(0), gamma.grad) < 1e-12
    # a keep-scale multiplies the gradient element by element
    ks = (torch.rand(N, H, generator=gen) < 0.5).double() * 2
    assert torch.equal(NO.gn_partials(g, x, saved, a, act, ks), NO.gn_partials(g.double() * ks, x, saved, a, act))
    # blocks partition the rows
    assert rel_inf(NO.gn_partials(g, x, saved, a, act, rows=64).sum(0), part.sum(0)) < 1e-12


def test_shape_list_maps_to_the_geometry_it_is_named_for():
    """Workgroup counts from glass_dual_linear_stat_rows (kNarrowRows), slab counts of 64 rows (kNarrowSlab) that fit the
    workspace glass_linear_wgrad_ws_bytes sizes.  (That size is the largest of several weight-gradient geometries; below 64 rows
    per slab the narrow one is what would outgrow it.  The GPU test pins the slab count exactly: every float below
    n_slabs * stride written, none beyond.)"""
    lib = _lib()
    assert list(NO.ROW_SWEEP) == [1, 63, 64, 65, 255, 256, 257, 1024, 1025, 4096, 4097]
    assert [v[0] for v in NO.ROW_SWEEP.values()] == [1, 1, 1, 2, 4, 4, 5, 16, 17, 64, 65]
    assert [v[1] for v in NO.ROW_SWEEP.values()] == [1, 1, 1, 1, 1, 1, 2, 4, 5, 16, 17]
    widths = sorted(set(NO.SWEEP_WIDTHS) | set(NO.ROW_WIDTHS))
    assert widths == list(range(1, 33))
    for H in widths:
        assert lib.glass_dual_linear_supported(H) == 1 and lib.glass_dual_linear_layout(H) == 2
        assert lib.glass_dual_linear_stat_rows(H) == NO.ROWS
    assert lib.glass_dual_linear_layout(33) != 2 and lib.glass_dual_linear_layout(64) != 2
    shapes = [(NO.SWEEP_N, H, (6, 2)) for H in NO.SWEEP_WIDTHS] + [(N, H, g) for N, g in NO.ROW_SWEEP.items() for H in NO.ROW_WIDTHS]
    for N, H, (slabs, wgs) in shapes:
        assert -(-N // int(lib.glass_dual_linear_stat_rows(H))) == wgs, (N, H)
        assert NO.blocks(N, NO.SLAB) == slabs, (N, H)
        for I in (H, 2 * H):
            need = slabs * NO.wgrad_stride(2 * H, I) * 4
            assert lib.glass_linear_wgrad_ws_bytes(N, 2 * H, I) >= need, (N, H, I)
    # the sweep's second workgroup has 65 rows, its last slab one row
    assert NO.SWEEP_N - NO.ROWS == 65 and NO.SWEEP_N - 5 * NO.SLAB == 1
    # every instantiation at H = HP and at every H below it
    for hp_lo, hp in zip((0, ) + NO.HP_STEPS, NO.HP_STEPS):
        assert [H for H in NO.SWEEP_WIDTHS if NO.hp_of(H) == hp] == list(range(hp_lo + 1, hp + 1))
    # the slab counts straddle the reduce's walk: 16 slabs per pass of a thread row, 64 per round
    assert {15 < s for s, _ in NO.ROW_SWEEP.values()} == {True, False} and {64 < s for s, _ in NO.ROW_SWEEP.values()} == {True, False}
    assert NO.wgrad_stride(64, 64) == 4160 and NO.wgrad_stride(2, 1) == 4 and NO.wgrad_stride(34, 17) == 612
