"""K1w without a GPU: the fp64 restatement tests/edge_grad_oracle.py against torch autograd through the oracle package's
buildAdj, and the host-side answers of the three new C entries (csrc/spmm_edge.hip, api.cpp)."""
import ctypes

import numpy as np
import pytest
import torch

import edge_grad_oracle as EO
from oracle import glass_oracle as O


@pytest.mark.parametrize("kind", ("mixed", "all_long"))
def test_restatement_agrees_with_autograd_through_build_adj(kind):
    """d/dw of sum(A(w) X * G), both sides fp64: 1e-12 relative, per element.  (Per element relative to the element's own
    terms: a gradient that is a difference of much larger terms has no digits of its own to compare.)"""
    n, ei, w = EO.graph(kind)
    csr = EO.SortedCSR(ei, n)
    d, _dt = EO.degrees(csr, w)
    assert float(np.abs(d - 0.5).min()) >= 1e-3, "the + 1 rule is discontinuous at a weight sum of 0.5"
    low = d[n - 1 - EO.N_LOW:n - 1]
    assert low.shape == (EO.N_LOW, ) and bool(((low >= 0.25) & (low < 0.5)).all()), "the rows that take the + 1"
    src = n - 1
    assert not bool((ei[0] == src).any()) and int((ei[1] == src).sum()) == 2 and d[src] == 0, "a source that is no destination"
    if kind == "mixed":
        pair = EO.pair_positions(ei)
        assert pair.shape == (2, ) and w[pair[0]] != w[pair[1]] and bool(((ei[0] == 30) & (ei[1] == 30)).any())
    rng = np.random.Generator(np.random.PCG64(5))
    H = 7
    X, G = rng.standard_normal((n, H)), rng.standard_normal((n, H))
    eit, Xt, Gt = torch.from_numpy(ei), torch.from_numpy(X), torch.from_numpy(G)
    for aggr in EO.AGGRS:
        wt = torch.from_numpy(w).double().requires_grad_()
        A = O.build_adj(eit, wt, n, aggr)
        ((A @ Xt) * Gt).sum().backward()
        want = wt.grad.numpy()
        val = EO.values(csr, w, aggr)
        assert np.allclose(val, O.adjacency_values(eit, wt.detach(), n, aggr).numpy()[csr.perm], rtol=1e-14, atol=0)
        dval, _m, R, _mr = EO.dval_R(csr, X, G, val)
        C = EO.colsum(csr, dval, val)[0] if aggr == "gcn" else None
        got, mass = EO.values_bwd(csr, w, aggr, dval, R, C)
        assert np.array_equal(got, EO.edge_grad(csr, w, aggr, X, G))
        # "mean" on a row of ONE entry with d >= 0.5: val = w / w, the gradient is zero in exact arithmetic and what either
        # side returns is the rounding of its two cancelling terms — those elements are held to 1e-12 of the terms instead
        deg1 = np.empty(csr.nnz, dtype=bool)
        deg1[csr.perm] = (np.diff(csr.rowptr) == 1)[csr.row] & (d >= 0.5)[csr.row]
        dead = deg1 if aggr == "mean" else np.zeros(csr.nnz, dtype=bool)
        assert bool((want[~dead] != 0).all()) and bool((np.abs(want[dead]) <= 1e-12 * mass[dead]).all())
        worst = float((np.abs(got - want)[~dead] / np.abs(want[~dead])).max())
        print(f"{kind} {aggr}: restatement against autograd, worst relative difference {worst:.2e} over {int((~dead).sum())} edges")
        assert worst <= 1e-12, (kind, aggr, worst)
        assert bool((np.abs(got - want)[dead] <= 1e-12 * mass[dead]).all())
        if kind == "mixed":
            # the duplicate pair: two entries, two gradients — each the per-entry value (which depends on the entry's row and
            # column alone, so the two are equal), not a coalesced entry's sum
            assert want[pair[0]] == want[pair[1]] and abs(got[pair[0]] - got[pair[1]]) <= 1e-12 * abs(want[pair[0]])
        if aggr != "sum":
            assert not np.allclose(got, dval[np.argsort(csr.perm)]), "the normalisation's own terms are there"


def _plan(rowptr):
    from glass_amd import _lib
    lib = _lib.load()
    rp = np.asarray(rowptr, dtype=np.int32)
    n = rp.shape[0] - 1
    words = ctypes.c_int64(0)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, n, None, ctypes.byref(words)) == 0
    plan = np.zeros(words.value, dtype=np.int32)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, n, plan.ctypes.data, ctypes.byref(words)) == 0
    return plan


def test_entries_validate_on_the_host():
    """Refusals come before any HIP call (the host buffers never reach a kernel): no GPU needed."""
    from glass_amd import _lib
    lib = _lib.load()
    E_ARG, E_PLAN, E_UNSUPPORTED = -1, -2, -3
    plan = _plan([0, 1, 2])
    cut = _plan([0, 700, 1400] + [1400] * 30)           # two rows of 700 entries: cut rows, partial slots
    assert cut[7] > 0
    empty = _plan([0])
    x = np.zeros(64, dtype=np.float32)
    p, hp = x.ctypes.data, plan.ctypes.data
    # the workspace queries
    assert lib.glass_spmm_dval_ws_bytes(hp, 64) == 0 and lib.glass_spmm_dval_ws_bytes(cut.ctypes.data, 64) == 4 * int(cut[7])
    assert lib.glass_spmm_dval_ws_bytes(p, 64) == E_PLAN and lib.glass_spmm_dval_ws_bytes(None, 64) == E_PLAN
    assert lib.glass_spmm_dval_ws_bytes(hp, 0) == E_ARG and lib.glass_spmm_dval_ws_bytes(hp, -4) == E_ARG
    assert lib.glass_adj_colsum_ws_bytes(hp) == 0 and lib.glass_adj_colsum_ws_bytes(cut.ctypes.data) == 4 * int(cut[7])
    assert lib.glass_adj_colsum_ws_bytes(p) == E_PLAN and lib.glass_adj_colsum_ws_bytes(None) == E_PLAN

    def dval(rowptr=hp, col=p, val=p, X=p, ldx=8, dY=p, lddy=8, dv=p, R=p, n=2, H=8, hdr=hp, pl=hp, ws=None):
        return lib.glass_spmm_dval_f32(rowptr, col, val, X, ldx, dY, lddy, dv, R, n, H, hdr, pl, ws, None)
    for null in ("rowptr", "X", "dY", "R", "hdr", "pl", "col", "val", "dv"):
        assert dval(**{null: None}) == E_ARG, null
    assert b"spmm_dval" in lib.glass_last_error_string()
    assert dval(H=0) == E_ARG and dval(H=-1) == E_ARG and dval(ldx=7) == E_ARG and dval(lddy=7) == E_ARG
    assert dval(X=p + 2) == E_ARG                                         # misaligned
    assert dval(n=3) == E_PLAN and dval(hdr=p) == E_PLAN
    assert b"plan does not match" in lib.glass_last_error_string()
    assert dval(H=65535 * 64 + 1, ldx=1 << 23, lddy=1 << 23) == E_UNSUPPORTED
    assert dval(hdr=cut.ctypes.data, n=32) == E_ARG and b"partial sums" in lib.glass_last_error_string()   # slots, no ws
    assert dval(hdr=empty.ctypes.data, n=0) == 0                           # nothing to do: no launch

    def colsum(rowptr=hp, col=p, val=p, eid=hp, dv=p, C=p, n=2, hdr=hp, pl=hp, ws=None):
        return lib.glass_adj_colsum_f32(rowptr, col, val, eid, dv, C, n, hdr, pl, ws, None)
    for null in ("rowptr", "C", "hdr", "pl", "col", "val", "eid", "dv"):
        assert colsum(**{null: None}) == E_ARG, null
    assert b"adj_colsum" in lib.glass_last_error_string()
    assert colsum(n=3) == E_PLAN and colsum(hdr=p) == E_PLAN and colsum(C=p + 1) == E_ARG
    assert colsum(hdr=cut.ctypes.data, n=32) == E_ARG and colsum(hdr=empty.ctypes.data, n=0) == 0

    def bwd(rowptr=hp, col=hp, perm=hp, deg=p, dv=p, R=p, C=p, n=2, nnz=2, aggr=2, dw=p):
        return lib.glass_adj_values_bwd_f32(rowptr, col, perm, deg, dv, R, C, n, nnz, aggr, dw, None)
    assert bwd(aggr=7) == E_UNSUPPORTED and bwd(aggr=-1) == E_UNSUPPORTED and b"adj_values_bwd" in lib.glass_last_error_string()
    for null in ("rowptr", "perm", "dv", "dw", "deg", "R", "col", "C"):
        assert bwd(**{null: None}) == E_ARG, null
    assert bwd(aggr=1, deg=None, R=None, C=None, col=None, n=0) == 0 and bwd(n=0) == 0 and bwd(nnz=0) == 0
    assert bwd(aggr=0, deg=None) == E_ARG and bwd(aggr=0, R=None) == E_ARG and bwd(n=-1) == E_ARG and bwd(nnz=-1) == E_ARG
    assert lib.glass_version() == _lib.ABI_VERSION == 6  # purely additive
