"""K7's pooling kernels on the GPU (glass_amd/csrc/pool.hip, bucket.h's ExactSum): every build and dispatch form against the
fp64 truth and the closed-form max of tests/pool_oracle.py, graded element by element against each element's own mass
(float forms: 1e-5 of it; exact forms: the derived bound 2^-21 * mass + entries * 2^-60, max pooling 2^-23).  Each case asserts
from the host restatement which build or form it runs; tests/test_pool_host.py holds the facts about the recipes.

  pool_fwd_kernel<4>: TC 1 / 2 / 16 / 128 / 256, two column tiles     test_forward_builds[4 / 8 / 64 / 512 / 1024 / 1028-vec-*]
  pool_fwd_kernel<1>: TC 1 / 4 / 32 / 256, two column tiles           test_forward_builds[1 / 3 / 17 / 255 / 257-scalar-*]
  the scalar build at a vector width (misaligned view)               test_forward_builds[64-view-*]
  count_valid's second round                                         test_forward_builds[*-257]
  pair_fwd_kernel / pair form of the gather, G = 1 .. 64, column loop test_pair_forward_and_backward (C ABI; [100-scalar]: a
                                                                     misaligned view), test_pair_autograd_binding
  ordered scatter at kPoolOrderedMax, exact gather just beyond it    test_backward_at_the_ordered_limit
  short / long list paths of the gather at G = 1 .. 64                test_gathers_on_lists
  max gather; Smax = 2 in max mode                                   test_gathers_on_lists[max-*], test_max_backward_on_ties
  float-atomic scatter                                               test_atomic_entry_point
  writes beyond C                                                    test_guard_columns_*
  row order does not reach the exact forms                           test_exact_forms_do_not_depend_on_the_row_order
  non-finite embeddings, ExactSum's range                            test_nonfinite_forward, test_exact_sum_range"""
import functools

import numpy as np
import pytest
import torch

import pool_oracle as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N = 37, 300
SUMS = ("sum", "mean", "size")


def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _aligned(*tensors):
    return all(t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0 for t in tensors)


def forward(emb_v, pos, mode, pad=0):
    """glass_segment_pool_f32 over the C ABI into a [B, C + pad] sentinel buffer -> (full buffer, argmax or None)"""
    L_, lib = _lib()
    n, C = emb_v.shape
    Bq, Smax = pos.shape
    full = torch.full((Bq + 1, C + pad), P.SENTINEL, device=DEV)
    arg = torch.full((Bq + 1, C), -7, dtype=torch.int32, device=DEV) if mode == "max" else None
    L_.check(lib.glass_segment_pool_f32(emb_v.data_ptr(), emb_v.stride(0), pos.data_ptr(), Bq, Smax, P.MODES[mode], full.data_ptr(),
                                        C + pad, None if arg is None else arg.data_ptr(), n, C, _stream()), "glass_segment_pool_f32")
    torch.cuda.synchronize()
    assert bool((full[Bq] == P.SENTINEL).all()) and (arg is None or bool((arg[Bq] == -7).all())), "the row behind the last"
    return full[:Bq], (None if arg is None else arg[:Bq])


@functools.lru_cache(maxsize=8)
def _fwd_truth(kind, Smax, C, mode):
    n = max(N, Smax + 8)
    if kind == "ties":
        pos, emb, _row = P.ties(B, Smax, n, C)
    else:
        pos, emb = P.ragged(B, Smax, n)[0], P.operand(n, C)
    if mode == "max":
        return pos, emb, P.max_truth(emb, pos)
    return pos, emb, P.forward_truth(emb, pos, mode)


FWD_CASES = [(C, "vec") for C in P.FWD_VEC] + [(C, "scalar") for C in P.FWD_SCALAR] + [(64, "view")]


@pytest.mark.parametrize("Smax", P.FWD_SMAX)
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_forward_builds(case, Smax):
    C, layout = case
    n = max(N, Smax + 8)
    worst = {}
    for kind in ("ragged", "ties"):
        for mode in ("sum", "mean", "size", "max"):
            pos, emb, truth = _fwd_truth(kind, Smax, C, mode)
            if layout == "view":
                wide = torch.zeros((n, 68), device=DEV)
                emb_v = wide[:, 1:65]
                emb_v.copy_(_dev(emb))
            else:
                emb_v = _dev(emb)
            full, arg = forward(emb_v, _dev(pos), mode)
            build = P.fwd_build(C, _aligned(emb_v, full))
            assert (build[0] == 4) == (layout == "vec"), (case, build)
            if mode == "max":
                assert P.max_forward_ok(full.cpu().numpy(), arg.cpu().numpy(), *truth), (case, Smax, kind, "max")
            else:
                s = P.float_share(full, *truth)
                worst[kind, mode] = s
                assert s <= 1.0, (case, Smax, kind, mode, s)
    vw, tc, slots, tiles = build
    print(f"C={C} {layout} Smax={Smax}: VW={vw} TC={tc} slots={slots} tiles={tiles}; worst share of the bound {max(worst.values()):.3f}")


# ---- pairs ----------------------------------------------------------------------------------------------------------------------
PAIR_CASES = [(C, "vec") for C in P.PAIR_VEC] + [(C, "scalar") for C in P.PAIR_SCALAR] + [(64, "strided")]


def _view(a, layout):
    """a on the device: contiguous; "strided": the first columns of a buffer 4 wider; "scalar" at a width that has a vector form:
    columns 1 .. C of a wider buffer, 4 bytes past a 16-byte boundary"""
    rows, C = a.shape
    if layout == "strided" or (layout == "scalar" and C % 4 == 0):
        wide = torch.full((rows, C + 4), float("nan"), device=DEV)
        v = wide[:, :C] if layout == "strided" else wide[:, 1:C + 1]
        v.copy_(_dev(a))
        return v
    return _dev(a)


def pair_calls(ev, pg, dv, mode, n):
    """glass_pair_pool_f32 and glass_pair_pool_bwd_f32 over the C ABI -> (out [B, C], demb [n, C]) in NaN-filled buffers"""
    L_, lib = _lib()
    Bp, C = dv.shape
    out, demb = torch.full((Bp, C), float("nan"), device=DEV), torch.full((n, C), float("nan"), device=DEV)
    ws = torch.empty(int(lib.glass_pair_pool_ws_bytes(n, Bp)) + 16, dtype=torch.uint8, device=DEV)
    L_.check(lib.glass_pair_pool_f32(ev.data_ptr(), ev.stride(0), pg.data_ptr(), Bp, P.MODES[mode], out.data_ptr(), C, n, C, _stream()),
             "glass_pair_pool_f32")
    L_.check(lib.glass_pair_pool_bwd_f32(dv.data_ptr(), dv.stride(0), pg.data_ptr(), Bp, P.MODES[mode], demb.data_ptr(), C, n, C,
                                         ws.data_ptr(), _stream()), "glass_pair_pool_bwd_f32")
    torch.cuda.synchronize()
    return out, demb


@pytest.mark.parametrize("case", PAIR_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_pair_forward_and_backward(case):
    C, layout = case
    Bp, n = 1003, 600
    prs, emb, dout = P.pairs(Bp, n), P.operand(n, C), P.operand(Bp, C, seed=1)
    ev, dv, pg = _view(emb, layout), _view(dout, layout), _dev(prs)
    vec = C % 4 == 0 and _aligned(ev) and _aligned(dv)
    assert vec == (layout != "scalar") and (vec or not (C % 4 == 0 and (_aligned(ev) or _aligned(dv)))), "layout of the case"
    G = P.pair_group(C, vec)
    lengths = P.list_lengths(prs, n)
    assert int(lengths.max()) >= 2 * P.PAIR_LONG_LIST and int((lengths == 0).sum()) >= 9
    for mode in SUMS:
        assert P.bwd_form(Bp, 2, mode) == "pair"
        y, g = pair_calls(ev, pg, dv, mode, n)
        s_f = P.float_share(y, *P.forward_truth(emb, prs, mode))
        s_b = P.exact_share(g, *P.backward_truth(dout, prs, n, mode))
        print(f"pairs C={C} {layout} G={G} {mode}: forward {s_f:.3f}, backward {s_b:.3f} of the bound")
        assert s_f <= 1.0 and s_b <= 1.0, (case, mode, s_f, s_b)
        assert torch.equal(_bits(g), _bits(pair_calls(ev, pg, dv, mode, n)[1])), "two runs differ"


def test_pair_autograd_binding():
    """ops.segment_pool on pairs (a strided emb view, C = 20): the same kernels behind autograd"""
    from glass_amd import ops
    Bp, n, C = 1003, 600, 20
    prs, emb, dout = P.pairs(Bp, n), P.operand(n, C), P.operand(Bp, C, seed=1)
    eg = _view(emb, "strided").requires_grad_(True)
    y = ops.segment_pool(eg, _dev(prs), "mean")
    (g, ) = torch.autograd.grad(y, eg, _dev(dout))
    assert P.float_share(y.detach(), *P.forward_truth(emb, prs, "mean")) <= 1.0
    assert P.exact_share(g, *P.backward_truth(dout, prs, n, "mean")) <= 1.0


# ---- backward forms through ops.segment_pool ------------------------------------------------------------------------------------
def _backward(emb, pos, dout, mode):
    from glass_amd import ops
    eg = _dev(emb).requires_grad_(True)
    pg, dg = _dev(pos), _dev(dout)
    (g, ) = torch.autograd.grad(ops.segment_pool(eg, pg, mode), eg, dg)
    (g2, ) = torch.autograd.grad(ops.segment_pool(eg, pg, mode), eg, dg)
    assert torch.equal(_bits(g), _bits(g2)), (mode, "two runs differ")
    return g


@pytest.mark.parametrize("Bq,form", [(384, "ordered"), (385, "exact")])
@pytest.mark.parametrize("C", (64, 17))
def test_backward_at_the_ordered_limit(C, Bq, form):
    Smax, n = 31, 600
    assert (Bq * Smax + Bq <= P.POOL_ORDERED_MAX) == (form == "ordered") and 384 * Smax + 384 == P.POOL_ORDERED_MAX
    pos, emb, dout = P.ragged(Bq, Smax, n)[0], P.operand(n, C), P.operand(Bq, C, seed=1)
    for mode in SUMS:
        assert P.bwd_form(Bq, Smax, mode) == form
        g = _backward(emb, pos, dout, mode)
        want, mass, entries = P.backward_truth(dout, pos, n, mode)
        s = P.float_share(g, want, mass) if form == "ordered" else P.exact_share(g, want, mass, entries)
        print(f"{form} B={Bq} C={C} {mode}: {s:.3f} of the bound")
        assert s <= 1.0, (form, C, mode, s)


@pytest.mark.parametrize("case", P.LIST_WIDTHS, ids=lambda c: f"{c[0]}-{'vec' if c[1] else 'scalar'}")
@pytest.mark.parametrize("mode", ("sum", "mean", "size", "max"))
def test_gathers_on_lists(mode, case):
    C, vec = case
    pos, n, Bq = P.lists(), P.LISTS_N, P.LISTS_B
    assert P.bwd_form(Bq, P.LISTS_SMAX, mode) == ("max_exact" if mode == "max" else "exact") and (C % 4 == 0) == vec
    dout = P.operand(Bq, C, seed=2)
    if mode == "max":
        emb = P.tie_emb(n, C, seed=1)
        out, arg = P.max_truth(emb, pos)
        full, got_arg = forward(_dev(emb), _dev(pos), "max")
        assert P.max_forward_ok(full.cpu().numpy(), got_arg.cpu().numpy(), out, arg)
        want, mass, entries = P.max_backward_truth(dout, pos, n, arg)
        s = P.exact_share(_backward(emb, pos, dout, "max"), want, mass, entries, P.REL_MAX)
    else:
        emb = P.operand(n, C)
        want, mass, entries = P.backward_truth(dout, pos, n, mode)
        s = P.exact_share(_backward(emb, pos, dout, mode), want, mass, entries)
    print(f"lists C={C} G={P.pair_group(C, vec)} {mode}: {s:.3f} of the bound")
    assert s <= 1.0, (mode, case, s)


@pytest.mark.parametrize("Smax", (2, 3, 40))
@pytest.mark.parametrize("C", (16, 17))
def test_max_backward_on_ties(C, Smax):
    """Ties between different nodes: the gradient goes to the lowest j.  Smax = 2 in max mode takes the segment kernels."""
    assert P.bwd_form(B, Smax, "max") == "max_exact"
    pos, emb, _row = P.ties(B, Smax, N, C)
    dout = P.operand(B, C, seed=3)
    out, arg = P.max_truth(emb, pos)
    full, got_arg = forward(_dev(emb), _dev(pos), "max")
    assert P.max_forward_ok(full.cpu().numpy(), got_arg.cpu().numpy(), out, arg)
    want, mass, entries = P.max_backward_truth(dout, pos, N, arg)
    s = P.exact_share(_backward(emb, pos, dout, "max"), want, mass, entries, P.REL_MAX)
    print(f"max backward on ties C={C} Smax={Smax}: {s:.3f} of the bound")
    assert s <= 1.0


# ---- the C ABI: atomic entry point, guard columns ---------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (64, 17))
@pytest.mark.parametrize("mode", ("sum", "mean", "size", "max"))
def test_atomic_entry_point(mode, C):
    L_, lib = _lib()
    Smax = 40
    if mode == "max":
        pos, emb, _row = P.ties(B, Smax, N, C)
        arg = P.max_truth(emb, pos)[1]
    else:
        pos, arg = P.ragged(B, Smax, N)[0], None
    dout = P.operand(B, C, seed=4)
    want, mass, _e = P.max_backward_truth(dout, pos, N, arg) if mode == "max" else P.backward_truth(dout, pos, N, mode)
    dg, pg, ag = _dev(dout), _dev(pos), (None if arg is None else _dev(arg))
    demb = torch.zeros((N, C), device=DEV)
    L_.check(lib.glass_segment_pool_bwd_atomic_f32(dg.data_ptr(), C, pg.data_ptr(), B, Smax, P.MODES[mode],
                                                   None if ag is None else ag.data_ptr(), demb.data_ptr(), C, N, C, _stream()),
             "glass_segment_pool_bwd_atomic_f32")
    torch.cuda.synchronize()
    s = P.float_share(demb, want, mass)
    print(f"atomic scatter C={C} {mode}: {s:.3f} of the bound")
    assert s <= 1.0


@pytest.mark.parametrize("pad", (4, 1))
@pytest.mark.parametrize("C", (64, 1028, 257))
def test_guard_columns_forward(C, pad):
    Smax = 40
    for mode in ("sum", "max"):
        pos, emb, truth = _fwd_truth("ragged", Smax, C, mode)
        emb_v = _dev(emb)
        full, arg = forward(emb_v, _dev(pos), mode, pad)
        assert P.fwd_build(C, _aligned(emb_v, full))[0] == (4 if C % 4 == 0 and pad == 4 else 1)
        assert P.beyond_columns_intact(full, C), (C, pad, mode)
        if mode == "max":
            assert P.max_forward_ok(full[:, :C].cpu().numpy(), arg.cpu().numpy(), *truth)
        else:
            assert P.float_share(full[:, :C], *truth) <= 1.0


@pytest.mark.parametrize("C", (64, 320, 17))
@pytest.mark.parametrize("mode", ("size", "max"))
def test_guard_columns_exact_backward(mode, C):
    """lde = C + 4 on `lists`: nothing is stored beyond C, every row of demb is written, rows without entries are zeros."""
    L_, lib = _lib()
    pos, n, Bq, Smax = P.lists(), P.LISTS_N, P.LISTS_B, P.LISTS_SMAX
    dout = P.operand(Bq, C, seed=2)
    dg, pg = _dev(dout), _dev(pos)
    full = torch.full((n + 1, C + 4), P.SENTINEL, device=DEV)
    ws = torch.empty(int(lib.glass_segment_pool_bwd_exact_ws_bytes(n, Bq, Smax)) + 16, dtype=torch.uint8, device=DEV)
    if mode == "max":
        arg = P.max_truth(P.tie_emb(n, C, seed=1), pos)[1]
        want, mass, entries = P.max_backward_truth(dout, pos, n, arg)
        ag = _dev(arg)
        L_.check(lib.glass_segment_pool_max_bwd_exact_f32(dg.data_ptr(), C, pg.data_ptr(), Bq, Smax, ag.data_ptr(), full.data_ptr(), C + 4,
                                                          n, C, ws.data_ptr(), _stream()), "glass_segment_pool_max_bwd_exact_f32")
    else:
        want, mass, entries = P.backward_truth(dout, pos, n, mode)
        L_.check(lib.glass_segment_pool_bwd_exact_f32(dg.data_ptr(), C, pg.data_ptr(), Bq, Smax, P.MODES[mode], full.data_ptr(), C + 4, n, C,
                                                      ws.data_ptr(), _stream()), "glass_segment_pool_bwd_exact_f32")
    torch.cuda.synchronize()
    assert P.beyond_columns_intact(full[:n], C) and bool((full[n] == P.SENTINEL).all())
    got = full[:n, :C]
    assert bool((got[_dev(entries == 0)] == 0).all()) and int((entries == 0).sum()) >= 1, "rows without entries are written: zeros"
    assert P.exact_share(got, want, mass, entries, P.REL_MAX if mode == "max" else P.REL_EXACT) <= 1.0


def test_exact_forms_do_not_depend_on_the_row_order():
    """Integer sums commute: the rows of (pos, dout) permuted give the same bits in the pair, bucketed and max gathers."""
    perm = np.random.Generator(np.random.PCG64(3)).permutation
    for form, mode, pos, n, C in (("pair", "size", P.pairs(1003, 600), 600, 20), ("exact", "mean", P.lists(), P.LISTS_N, 17),
                                  ("exact", "size", P.lists(), P.LISTS_N, 64), ("max_exact", "max", P.lists(), P.LISTS_N, 64)):
        Bq = pos.shape[0]
        assert P.bwd_form(Bq, pos.shape[1], mode) == form
        emb = P.tie_emb(n, C, seed=1) if mode == "max" else P.operand(n, C)
        dout = P.operand(Bq, C, seed=5)
        p = perm(Bq)
        assert torch.equal(_bits(_backward(emb, pos, dout, mode)), _bits(_backward(emb, pos[p], dout[p], mode))), (form, mode)


# ---- non-finite values --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (64, 17))
@pytest.mark.parametrize("bad", (float("nan"), float("inf")), ids=("nan", "inf"))
def test_nonfinite_forward(bad, C):
    """A NaN / +Inf embedding element reaches exactly the subgraphs that name its node, in every mode; in max mode it takes the
    column and its node is the argmax (the first NaN's).  A column whose valid entries are all -Inf: 0 and argmax -1."""
    Smax = 40
    pos, f = P.ragged(B, Smax, N)
    emb = P.operand(N, C).copy()
    b0, b1, shared = f["shared"]
    dup_b, dup_node = f["dup"]
    full_row = pos[f["full"]]
    emb[shared, 3] = emb[dup_node, 5] = emb[full_row[7], 6] = emb[full_row[20], 6] = bad
    emb[pos[f["single"], 0], 8] = -np.inf
    for mode in ("sum", "mean", "size", "max"):
        full, arg = forward(_dev(emb), _dev(pos), mode)
        got = full.cpu().numpy()
        want_bad = np.zeros((B, C), dtype=bool)
        for node, c in ((shared, 3), (dup_node, 5), (full_row[7], 6), (full_row[20], 6)):
            want_bad[(pos == node).any(1), c] = True
        assert want_bad[b0, 3] and want_bad[b1, 3] and want_bad[dup_b, 5]
        hit = np.isnan(got) if bad != bad else (got == np.inf)
        assert np.array_equal(hit, want_bad), (mode, "the non-finite value reaches the rows naming the node, nothing else")
        assert bool(np.isfinite(got[~want_bad]).all()) or mode != "max"
        if mode == "max":
            out, want_arg = P.max_truth(emb, pos)
            assert P.max_forward_ok(got, arg.cpu().numpy(), out, want_arg)
            assert arg[f["full"], 6] == full_row[7] and got[f["single"], 8] == 0 and arg[f["single"], 8] == -1
        else:
            assert got[f["single"], 8] == -np.inf


@pytest.mark.parametrize("C", (4, 17))
@pytest.mark.parametrize("count,value", [(4, 3e12), (80, 2e11)], ids=("short-list", "long-list"))
def test_exact_sum_range(count, value, C):
    """Every addend is inside ExactSum's addend range, their sum is beyond 2^63 quanta: NaN or the sum, never another number."""
    from glass_amd import ops
    n = count + 1
    prs = np.stack((np.zeros(count, dtype=np.int64), np.arange(1, count + 1))).T.copy()
    assert (count >= P.PAIR_LONG_LIST) == (count == 80) and count * value * 2.0**20 > 2.0**63 > value * 2.0**20
    dout = np.full((count, C), value, dtype=np.float32)
    eg = torch.zeros((n, C), device=DEV, requires_grad=True)
    (g, ) = torch.autograd.grad(ops.segment_pool(eg, _dev(prs), "sum"), eg, _dev(dout))
    got = g.cpu().numpy().astype(np.float64)
    want, mass, entries = P.backward_truth(dout, prs, n, "sum")
    print(f"{count} x {value:g}: node 0 reads {got[0, 0]:g}, the sum is {want[0, 0]:g}")
    bound = P.REL_EXACT * mass + entries[:, None] * P.QUANTUM
    assert bool((np.isnan(got[0]) | (np.abs(got[0] - want[0]) <= bound[0])).all()), "finite and wrong"
    assert bool((np.abs(got[1:] - want[1:]) <= bound[1:]).all())
