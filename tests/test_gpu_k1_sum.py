"""K1's sum kernels on the GPU: glass_spmm_csr_f32 (csrc/spmm.hip, spmm_sweep.h, spmm_common.h) and glass_spmm_csr_rep_f32
(csrc/spmm_rep.hip) called directly, on every plan form and in every build, against the fp64 CSR product of
tests/k1_sum_oracle.py formed from the fp32 values the kernels read (adj.fwd.val / adj.bwd.val read back).

Every result is graded element by element against its own mass, |got - want| <= 1e-5 * sum_e |val_e * x[col_e, c]|, an
element without mass (an empty row) exactly 0; Y and the partial-row workspace sit in NaN-filled buffers between sentinels
(the workspace need not be initialised: graph.py hands out torch.empty), the workspace is exactly H_NSLOTS * H * 4 bytes
(times R for the replicated entry), and two runs give the same bits.  Each test prints the worst value of its cases.
tests/test_k1_sum_host.py holds the facts about the three plans that this module relies on.

Build -> case (VW x LPR of GLASS_K1_WIDTH_DISPATCH; every one on the graphs `mixed`: row-mode sweep items + long items in the
sweep launch + reduce, and `all_long`: spmm_long_kernel + reduce, forward and transposed):
  VW 4, LPR 1 / 2 / 4 / 8 / 16 / 32 / 64     test_every_build_on_every_plan_form[*-4 / 8 / 16 / 32 / 64 / 128 / 256-vec]
  VW 4, LPR 64, 2 and 3 column tiles         test_every_build_on_every_plan_form[*-260-vec], [*-520-vec]
  VW 1, LPR 1 / 2 / 4 / 8 / 16 / 32 / 64     test_every_build_on_every_plan_form[*-1 / 2 / 3 / 7 / 13 / 17 / 33-scalar]
  VW 1, LPR 64, 2 and 3 column tiles         test_every_build_on_every_plan_form[*-100-scalar], [*-130-scalar]
  scalar build at a vector width             test_strided_and_unaligned_operands (ld % 4 != 0; X, Y or the workspace off 16 B)
  flat-capable sweep build (FLAT = true), flat and row items, long items and a cut row in the same launch, graph `flat`:
    VW 4, G = 64 / 16 / 8 / 4 / 2            test_flat_build[4 / 16 / 32 / 64 / 128-vec]
    VW 1, G = 2                              test_flat_build[17-scalar]
    G = 1: the row-only build on that plan   test_flat_build[256-vec]
    VW 4, G = 16, two rows per lane group    test_flat_build_with_runs_of_rows_per_lane_group (graph `flat_runs`)
  stand-alone long kernel                    every `all_long` case above
  replicated launches (launch_rep_u)         test_replicated_product[mixed / flat - 64 / 17 - own / shared]; the long kernel's
                                             replicated form: test_replicated_product_on_the_all_long_plan
  aggr "mean" and "gcn" values               test_mean_and_gcn_through_csradj
  autograd binding                           test_autograd_binding
The non-temporal builds (NT = true) need more than 256 MiB streamed by one launch; they stay with
test_spmm_row_parallel_wide_threshold_on_large_graphs (tests/test_gpu_kernels.py)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import k1_sum_oracle as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = K.TOL
GUARD = 64
NAN = float("nan")


def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """`n` elements filled with `fill`, GUARD sentinel elements in front and behind (tests/test_gpu_aggr_gat.py's); `off` more
    filled elements in front of the view `t`, which then starts `off` elements past a 16-byte boundary"""
    def __init__(self, n, fill, dtype=torch.float32, off=0):
        self.buf = torch.empty(n + off + 2 * GUARD, dtype=dtype, device=DEV)
        self.sentinel = (torch.arange(2 * GUARD, device=DEV) * 3 - 11).to(dtype)
        self.buf[:GUARD] = self.sentinel[:GUARD]
        self.buf[GUARD + off + n:] = self.sentinel[GUARD:]
        self.pad = self.buf[GUARD:GUARD + off]
        self.t = self.buf[GUARD + off:GUARD + off + n]
        self.pad.fill_(fill)
        self.t.fill_(fill)
        self.fill = fill
        assert self.buf[GUARD:].data_ptr() % 16 == 0

    def intact(self):
        n = self.t.numel() + self.pad.numel()
        same = torch.isnan(self.pad).all() if self.fill != self.fill else (self.pad == self.fill).all()
        return (torch.equal(self.buf[:GUARD], self.sentinel[:GUARD]) and torch.equal(self.buf[GUARD + n:], self.sentinel[GUARD:])
                and bool(same))


@functools.lru_cache(maxsize=None)
def _adj(kind, aggr="sum"):
    from glass_amd import graph
    n, ei, ew = K.graph(kind)
    return graph.CSRAdj(ei.to(DEV), ew.to(DEV), n, aggr)


def _op(kind, transposed, aggr="sum"):
    adj = _adj(kind, aggr)
    return adj.bwd if transposed else adj.fwd


@functools.lru_cache(maxsize=12)
def _reference(kind, transposed, H, seed=0, aggr="sum"):
    """(Y, mass, empty rows) in fp64 from the operand's own fp32 values, read back"""
    op = _op(kind, transposed, aggr)
    rp = op.rowptr.cpu().numpy()
    Y, mass = K.product(rp, op.col.cpu().numpy(), op.val.cpu().numpy(), K.operand(kind, H, seed).numpy())
    return Y, mass, torch.from_numpy(np.flatnonzero(np.diff(rp) == 0))


def _wide(src, pad, off=0):
    """src as the first columns of a NaN-filled [n, H + pad] buffer that starts `off` floats past a 16-byte boundary"""
    n, H = src.shape
    buf = torch.full((n * (H + pad) + off + 4, ), NAN, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + n * (H + pad)].view(n, H + pad)
    v[:, :H] = src.to(DEV)
    return v[:, :H]


def _is_vec(H, ldx, ldy, x_ptr, y_ptr, ws_ptr, slots):
    """the layout glass_spmm_csr_f32 / _rep_f32 choose (spmm.hip)"""
    return (H % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and x_ptr % 16 == 0 and y_ptr % 16 == 0
            and (slots == 0 or ws_ptr % 16 == 0))


class Product:
    """One call of glass_spmm_csr_f32 on guarded NaN buffers: Y [n, ldy] with ldy = H + pad_y, `y_off` / `ws_off` floats past a
    16-byte boundary.  `vec` is the layout the case means to take: asserted from the pointers."""
    def __init__(self, op, Xv, vec, pad_y=0, y_off=0, ws_off=0):
        L_, lib = _lib()
        n, H = op.n_rows, Xv.shape[1]
        hdr = op.header
        slots = int(hdr[K.H_NSLOTS])
        nbytes = lib.glass_spmm_ws_bytes(hdr.ctypes.data, H)
        assert nbytes == slots * H * 4, (nbytes, slots, H)
        self.ldy = H + pad_y
        self.W = Guarded(max(nbytes // 4, 4), NAN, off=ws_off)
        self.Yg = Guarded(n * self.ldy, NAN, off=y_off)
        ldx = Xv.stride(0)
        assert _is_vec(H, ldx, self.ldy, Xv.data_ptr(), self.Yg.t.data_ptr(), self.W.t.data_ptr(), slots) == vec, "layout of the case"
        L_.check(lib.glass_spmm_csr_f32(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), Xv.data_ptr(), ldx,
                                        self.Yg.t.data_ptr(), self.ldy, n, H, hdr.ctypes.data, op.plan.data_ptr(),
                                        self.W.t.data_ptr(), _stream()), "glass_spmm_csr_f32")
        torch.cuda.synchronize()
        self.H = H
        self.full = self.Yg.t.view(n, self.ldy)
        self.Y = self.full[:, :H]

    def intact(self):
        return self.Yg.intact() and self.W.intact() and bool(torch.isnan(self.full[:, self.H:]).all())


def _grade(tag, make, want, mass, empty):
    """the gates of one case: guards, empty rows, of_mass, two runs; -> the worst of-mass value"""
    run = make()
    assert run.intact(), (tag, "guards of Y / the workspace, columns beyond H")
    Y = run.Y.cpu()
    assert bool((Y[empty] == 0).all()), (tag, "a row without entries")
    e = K.of_mass(Y, want, mass)
    assert e <= TOL, (tag, e)
    assert torch.equal(_bits(make().Y), _bits(run.Y)), (tag, "two runs differ")
    return e


def test_the_device_plans_are_the_host_tests_plans():
    """graph.CSRAdj's CSR and plan on the device are what tests/test_k1_sum_host.py states its facts about"""
    for kind in K.KINDS:
        for transposed in (False, True):
            op = _op(kind, transposed)
            rp, col, val = K.csr(kind, transposed)
            assert torch.equal(op.rowptr.cpu(), torch.from_numpy(rp)) and torch.equal(op.col.cpu().to(torch.int64), torch.from_numpy(col))
            assert torch.equal(op.val.cpu(), torch.from_numpy(val)), "aggr sum: the raw weights"
            assert np.array_equal(op.header, K.Plan(rp).header) and np.array_equal(op.plan.cpu().numpy(), K.Plan(rp).blob)


CASES = [(H, True) for H in K.VEC_WIDTHS] + [(H, False) for H in K.SCALAR_WIDTHS]
_id = lambda c: f"{c[0]}-{'vec' if c[1] else 'scalar'}"


def _operands_for(kind, H, vec, seed=0):
    """(X view on the device, pad of Y's rows): contiguous, unless a scalar case has a width that would take the vector form"""
    X = K.operand(kind, H, seed)
    if not vec and H % 4 == 0:
        return _wide(X, 1), 3
    return X.to(DEV), 0


@pytest.mark.parametrize("case", CASES, ids=_id)
@pytest.mark.parametrize("kind", ("mixed", "all_long"))
def test_every_build_on_every_plan_form(kind, case):
    H, vec = case
    worst = {}
    for transposed in (False, True):
        op = _op(kind, transposed)
        hdr = op.header
        if kind == "mixed":
            assert 0 < hdr[K.H_NSWEEP] < K.FLAT_MIN_ITEMS and hdr[K.H_NLONG] >= 3 and hdr[K.H_NREDUCE] >= 1
        else:
            assert hdr[K.H_NSWEEP] == 0 and hdr[K.H_NLONG] >= 42 and hdr[K.H_NREDUCE] >= 1
        want, mass, empty = _reference(kind, transposed, H)
        Xv, pad_y = _operands_for(kind, H, vec)
        worst["transposed" if transposed else "forward"] = _grade((kind, H, vec, transposed), lambda: Product(op, Xv, vec, pad_y),
                                                                  want, mass, empty)
    vw, lpr, tiles = K.build_of(H, vec)
    print(f"{kind} H={H} VW={vw} LPR={lpr} column tiles={tiles}: worst of mass " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("H", (64, 17))
@pytest.mark.parametrize("aggr", ("mean", "gcn"))
def test_mean_and_gcn_through_csradj(aggr, H):
    """The normalised values (glass_adj_values_f32, graded by test_adj_values_g1) read back: the same kernels on other values."""
    for kind in ("mixed", "all_long"):
        assert not torch.equal(_adj(kind, aggr).fwd.val, _adj(kind).fwd.val)
        for transposed in (False, True):
            op = _op(kind, transposed, aggr)
            want, mass, empty = _reference(kind, transposed, H, 0, aggr)
            Xv = K.operand(kind, H).to(DEV)
            e = _grade((aggr, kind, H, transposed), lambda: Product(op, Xv, H % 4 == 0), want, mass, empty)
            print(f"{aggr} {kind} H={H}{' transposed' if transposed else ''}: worst of mass {e:.2e}")


FLAT_CASES = [(H, True) for H in K.FLAT_VEC_WIDTHS] + [(H, False) for H in K.FLAT_SCALAR_WIDTHS] + [(256, True)]


@pytest.mark.parametrize("case", FLAT_CASES, ids=_id)
def test_flat_build(case):
    """The flat-capable sweep build at its smallest plan (>= 8 192 sweep items): at G = 2 and 4 lane groups per wave more than a
    tenth of the items walk flat and more than a tenth take the row path inside that build, at G = 8 some, from G = 16 all walk
    flat; six long-row items ride in the same launch and one row is cut (reduce launch).  H = 256 (G = 1) takes the row-only
    build on the same plan.  (The non-temporal builds need > 256 MiB streamed: tests/test_gpu_kernels.py's large test.)"""
    H, vec = case
    vw, lpr, _tiles = K.build_of(H, vec)
    G = 64 // lpr
    for transposed in (False, True):
        op = _op("flat", transposed)
        hdr = op.header
        assert hdr[K.H_NSWEEP] >= K.FLAT_MIN_ITEMS and hdr[K.H_RP_FACTOR] == 4 and hdr[K.H_NLONG] >= 1 and hdr[K.H_NREDUCE] >= 1
        assert K.takes_flat_build(hdr, G) == (H != 256), "the launch is the flat-capable one (header words 4 and 15)"
        want, mass, empty = _reference("flat", transposed, H)
        assert len(empty) >= 1000
        Xv = K.operand("flat", H).to(DEV)
        e = _grade(("flat", H, vec, transposed), lambda: Product(op, Xv, vec), want, mass, empty)
        print(f"flat H={H} VW={vw} G={G}{' transposed' if transposed else ''}: worst of mass {e:.2e}")


def test_flat_build_with_runs_of_rows_per_lane_group():
    """H = 16 (G = 16) on `flat_runs`: items of about twenty rows, so a lane group of the equal-row-count split (G > 8) owns two
    rows and has to flush at a row boundary and to write its run's empty rows — on `flat` (at most four rows per item) it never
    owns more than one.  640 000 rows because only a sweep of that cost gets a budget that packs so many rows into an item."""
    H = 16
    op = _op("flat_runs", False)
    hdr = op.header
    assert np.array_equal(hdr, K.Plan(K.csr("flat_runs")[0]).header), "the plan tests/test_k1_sum_host.py describes"
    assert K.takes_flat_build(hdr, 16) and hdr[K.H_NLONG] == 0 and hdr[K.H_NSLOTS] == 0
    want, mass, empty = _reference("flat_runs", False, H)
    Xv = K.operand("flat_runs", H).to(DEV)
    e = _grade(("flat_runs", H), lambda: Product(op, Xv, True), want, mass, empty)
    print(f"flat_runs H={H} VW=4 G=16: worst of mass {e:.2e}")


@pytest.mark.parametrize("H,pads,offs,vec", [
    (64, (8, 4), (0, 0, 0), True), (64, (3, 1), (0, 0, 0), False), (18, (2, 6), (0, 0, 0), False), (18, (3, 1), (0, 0, 0), False),
    (64, (0, 0), (1, 1, 1), False), (64, (4, 4), (3, 3, 3), False), (64, (0, 0), (1, 0, 0), False), (64, (0, 0), (0, 3, 0), False),
    (64, (0, 0), (0, 0, 1), False), (64, (4, 8), (0, 0, 3), False), (18, (2, 6), (3, 1, 3), False)])
def test_strided_and_unaligned_operands(H, pads, offs, vec):
    """X and Y as column slices of wider NaN-filled buffers (pads that are multiples of 4 keep the 16-byte form, anything else
    takes the scalar one), and X, Y, the workspace — together and one at a time — 1 or 3 floats past a 16-byte boundary (the
    scalar form at a width that has a vector one).  The columns beyond H are neither read (NaN) nor written."""
    (pad_x, pad_y), (off_x, off_y, off_w) = pads, offs
    for transposed in (False, True):
        op = _op("mixed", transposed)
        assert op.header[K.H_NSLOTS] >= 3, "both directions have a workspace"
        want, mass, empty = _reference("mixed", transposed, H)
        Xv = _wide(K.operand("mixed", H), pad_x, off_x)
        assert Xv.data_ptr() % 16 == 4 * off_x and Xv.stride(0) == H + pad_x
        e = _grade((H, pads, offs, transposed), lambda: Product(op, Xv, vec, pad_y, off_y, off_w), want, mass, empty)
        print(f"H={H} pads={pads} offsets={offs}{' transposed' if transposed else ''}: worst of mass {e:.2e}")


# ---- the replicated product --------------------------------------------------------------------------------------------------
class RepProduct:
    """One call of glass_spmm_csr_rep_f32: replica r reads X rows from r * xs (xs = 0: one X for all) and writes Y rows from
    r * ys; X's and Y's gap rows are NaN."""
    def __init__(self, op, kind, H, R, xs, ys):
        L_, lib = _lib()
        n = op.n_rows
        hdr = op.header
        slots = int(hdr[K.H_NSLOTS])
        nbytes = lib.glass_spmm_rep_ws_bytes(hdr.ctypes.data, H, R)
        assert nbytes == R * slots * H * 4
        self.W = Guarded(max(nbytes // 4, 4), NAN)
        x_rows = (R - 1) * xs + n
        self.X = torch.full((x_rows, H), NAN, device=DEV)
        for r in range(R if xs else 1):
            self.X[r * xs:r * xs + n] = K.operand(kind, H, r).to(DEV)
        self.Yg = Guarded(((R - 1) * ys + n) * H, NAN)
        L_.check(lib.glass_spmm_csr_rep_f32(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), self.X.data_ptr(), H, xs,
                                            self.Yg.t.data_ptr(), H, ys, n, H, R, hdr.ctypes.data, op.plan.data_ptr(),
                                            self.W.t.data_ptr(), _stream()), "glass_spmm_csr_rep_f32")
        torch.cuda.synchronize()
        self.full = self.Yg.t.view(-1, H)
        self.reps = [self.full[r * ys:r * ys + n] for r in range(R)]
        self.gaps = [self.full[r * ys + n:(r + 1) * ys] for r in range(R - 1)]

    def intact(self):
        return self.Yg.intact() and self.W.intact() and all(bool(torch.isnan(g).all()) for g in self.gaps)


@pytest.mark.parametrize("x_mode", ("own", "shared"))
@pytest.mark.parametrize("H", (64, 17))
@pytest.mark.parametrize("kind", ("mixed", "flat"))
def test_replicated_product(kind, H, x_mode):
    """R = 3, y_rep_stride = n + 5 (the gap rows stay NaN), x_rep_stride = n + 3 (every replica its own X; the gap rows of X
    are NaN and must not be read) or 0 (one X for all).  R = 1 gives the bits of glass_spmm_csr_f32."""
    R = 3
    for transposed in (False, True):
        op = _op(kind, transposed)
        n = op.n_rows
        xs, ys = (n + 3 if x_mode == "own" else 0), n + 5
        if kind == "flat":
            assert K.takes_flat_build(op.header, 64 // K.build_of(H, H % 4 == 0)[1])
        run = RepProduct(op, kind, H, R, xs, ys)
        assert len(run.gaps) == 2 and run.gaps[0].shape == (5, H) and run.intact(), (kind, H, x_mode, transposed)
        again = RepProduct(op, kind, H, R, xs, ys)
        worst = 0.0
        for r in range(R):
            want, mass, empty = _reference(kind, transposed, H, r if xs else 0)
            Y = run.reps[r].cpu()
            assert bool((Y[empty] == 0).all())
            e = K.of_mass(Y, want, mass)
            assert e <= TOL, (kind, H, x_mode, transposed, r, e)
            worst = max(worst, e)
            assert torch.equal(_bits(again.reps[r]), _bits(run.reps[r])), "two runs differ"
        if not xs:
            assert torch.equal(_bits(run.reps[1]), _bits(run.reps[0])) and torch.equal(_bits(run.reps[2]), _bits(run.reps[0]))
        one = RepProduct(op, kind, H, 1, xs, ys)
        single = Product(op, K.operand(kind, H).to(DEV), H % 4 == 0)
        assert one.intact() and torch.equal(_bits(one.reps[0]), _bits(single.Y)), "R = 1 is glass_spmm_csr_f32"
        assert torch.equal(_bits(run.reps[0]), _bits(single.Y)), "replica 0 of three has the same bits too"
        print(f"replicated {kind} H={H} X {x_mode}{' transposed' if transposed else ''}: worst of mass over 3 replicas {worst:.2e}")


@pytest.mark.parametrize("H", (64, 17))
def test_replicated_product_on_the_all_long_plan(H):
    """spmm_rep_long_kernel: no sweep item, every replica its own partial rows"""
    for transposed in (False, True):
        op = _op("all_long", transposed)
        n = op.n_rows
        run = RepProduct(op, "all_long", H, 3, n + 3, n + 5)
        assert run.intact()
        for r in range(3):
            want, mass, empty = _reference("all_long", transposed, H, r)
            e = K.of_mass(run.reps[r].cpu(), want, mass)
            print(f"replicated all_long H={H}{' transposed' if transposed else ''} replica {r}: of mass {e:.2e}")
            assert e <= TOL and bool((run.reps[r].cpu()[empty] == 0).all())


def test_calls_without_replicas_or_rows_launch_nothing():
    L_, lib = _lib()
    H = 8
    op = _op("mixed", False)
    n = op.n_rows
    x, y, w = Guarded(n * H, NAN), Guarded(n * H, NAN), Guarded(int(op.header[K.H_NSLOTS]) * H, NAN)
    assert lib.glass_spmm_rep_ws_bytes(op.header.ctypes.data, H, 0) == 0
    assert lib.glass_spmm_csr_rep_f32(op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(), x.t.data_ptr(), H, n, y.t.data_ptr(),
                                      H, n, n, H, 0, op.header.ctypes.data, op.plan.data_ptr(), w.t.data_ptr(), _stream()) == 0
    # a matrix without rows
    rp = np.zeros(1, dtype=np.int32)
    words = ctypes.c_int64(0)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, 0, None, ctypes.byref(words)) == 0
    plan = np.zeros(words.value, dtype=np.int32)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, 0, plan.ctypes.data, ctypes.byref(words)) == 0
    pd, rpd = torch.from_numpy(plan).to(DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.glass_spmm_ws_bytes(plan.ctypes.data, H) == 0 and lib.glass_spmm_rep_ws_bytes(plan.ctypes.data, H, 3) == 0
    assert lib.glass_spmm_csr_f32(rpd.data_ptr(), None, None, x.t.data_ptr(), H, y.t.data_ptr(), H, 0, H, plan.ctypes.data,
                                  pd.data_ptr(), None, _stream()) == 0
    assert lib.glass_spmm_csr_rep_f32(rpd.data_ptr(), None, None, x.t.data_ptr(), H, 0, y.t.data_ptr(), H, 0, 0, H, 3,
                                      plan.ctypes.data, pd.data_ptr(), None, _stream()) == 0
    torch.cuda.synchronize()
    assert all(q.intact() and bool(torch.isnan(q.t).all()) for q in (x, y, w))


def test_autograd_binding():
    """ops.spmm and ops.spmm_rep on `mixed` at H = 20 (VW 4, LPR 8): the backward is the product with the transposed operand."""
    from glass_amd import ops
    adj = _adj("mixed")
    n, H, R = adj.n_node, 20, 2
    X, dY = K.operand("mixed", H, 0), K.operand("mixed", H, 1)
    want, mass, _e = _reference("mixed", False, H, 0)
    want_t, mass_t, _e = _reference("mixed", True, H, 1)
    Xd = X.to(DEV).requires_grad_(True)
    out = ops.spmm(adj, Xd)
    out.backward(dY.to(DEV))
    e, e_t = K.of_mass(out, want, mass), K.of_mass(Xd.grad, want_t, mass_t)
    print(f"ops.spmm H={H}: forward {e:.2e} backward {e_t:.2e} of mass")
    assert e <= TOL and e_t <= TOL
    # two replicas: (X, dY) and (dY, X)
    want1, mass1, _e = _reference("mixed", False, H, 1)
    want1_t, mass1_t, _e = _reference("mixed", True, H, 0)
    Xr = torch.cat((X, dY)).to(DEV).requires_grad_(True)
    out = ops.spmm_rep(adj, Xr, R)
    assert out.shape == (R * n, H)
    out.backward(torch.cat((dY, X)).to(DEV))
    errs = (K.of_mass(out[:n], want, mass), K.of_mass(out[n:], want1, mass1), K.of_mass(Xr.grad[:n], want_t, mass_t),
            K.of_mass(Xr.grad[n:], want1_t, mass1_t))
    print(f"ops.spmm_rep H={H} R={R}: forward {errs[0]:.2e} {errs[1]:.2e} backward {errs[2]:.2e} {errs[3]:.2e} of mass")
    assert all(v <= TOL for v in errs)
    assert torch.equal(_bits(out[:n].detach()), _bits(ops.spmm(adj, X.to(DEV)))), "a replica has the bits of the single product"
