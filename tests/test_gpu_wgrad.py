"""The weight-gradient kernels (K5w: linear.hip, wgrad_common.h, wgrad128.hip, wgrad_tiled.hip) on the GPU, called through the C entries
glass_linear_wgrad_f32 / glass_dual_linear_wgrad_f32 in every kernel and launch form tests/wgrad_oracle.py names, graded element by
element against its fp64 truth at |got - want| <= 1e-5 * mass, and bit for bit on the exact probes.  dW and db live in NaN-filled
buffers with guard rows and columns (lddw = I + 4) that must come back untouched (with accumulate: pre-filled with finite values); the
workspace is exactly glass_linear_wgrad_ws_bytes long with a canary behind it; every input is a strided view (ld = width + 4) whose
guard columns and the two rows behind row N - 1 hold Inf / NaN; every case asserts the route and geometry it was written for through
wgrad_oracle.route — the dispatch restated, tied to the source text by tests/test_wgrad_host.py; which kernel ran is not observed —,
runs twice and must repeat bit for bit, in both product forms (the act word's DENSE_F32_PRODUCTS) where the route has two.  For
N >= 65 536 the fp64 truth and mass are formed with torch fp64 on the device (held to the CPU truth at 1e-12 once); the recipes of
N >= 8 192 are drawn on the device.

Hidden 64 through this entry has ONE output tile (nz = 1): its comb pair takes the plain form, as the restated dispatch says.

Worst share of the bar per route and product form as measured on MI355X: see MEASURED below."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import wgrad_oracle as WO  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
Z = 0.8
BIG = 8192          # from here on the recipes are drawn on the device
TRUTH_DEV = 65536   # ... and the fp64 truth and mass formed there

MEASURED = """
  317 cases, 14.3 s.  Worst share of the 1e-5 * mass bar, dW / db, split | f32 products (- : the route has one form):
  thin              -             | 0.009 / 0.009      plain             -             | 0.014 / 0.010
  g64 trans (elu)   -             | 0.007 / 0.003      g64 trans none    -             | 0.006 / 0.003
  g64 trans relu    -             | 0.009 / 0.003      g64 comb          -             | 0.009 / 0.003
  g64 comb elu      -             | 0.008 / 0.007      g192 comb         -             | 0.008 / 0.003
  g320 comb         -             | 0.011 / 0.004      g128 trans        0.005 / 0.002 | 0.003 / 0.002
  g128 trans none   0.003 / 0.001 | 0.003 / 0.001      g128 comb (eff)   0.004 / 0.002 | 0.004 / 0.002
  g128 trans 400k   0.002 / 0.000 | 0.001 / 0.000      g128 comb 400k    0.001 / 0.000 | 0.001 / 0.000
  g256 trans        0.006 / 0.002 | 0.005 / 0.002      g256 comb (eff)   0.004 / 0.002 | 0.004 / 0.001
  w128 trans        0.002 / 0.001 | 0.002 / 0.001      w128 comb (lists) 0.003 / 0.001 | 0.002 / 0.001
  t256 trans        0.003 / 0.001 | 0.003 / 0.001      t256 comb (eff)   0.003 / 0.001 | 0.002 / 0.001
  t512 trans        0.004 / 0.001 | 0.004 / 0.001      t512 comb (eff)   0.004 / 0.001 | 0.004 / 0.001
(the f32 column of the w128 routes is the register-pipelined kernel on the same slab geometry.  The CPU restatement on the same recipes,
tests/test_wgrad_host.py: thin 0.009, plain 0.014, g320 comb 0.009, g256 trans 0.006; on its reduced clones of the routes from 8 192 rows
on: 0.015 at most.)
Every exact probe is bit-equal on every route in both forms; no case fails on the parent commit: no defect was found.
"""

_WORST = {}


def _lib():
    from glass_amd import _lib
    return _lib.load()


def _act_word(act, f32p):
    from glass_amd import _lib
    return int(act) | (_lib.DENSE_F32_PRODUCTS if f32p else 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc):
    assert rc == 0, _lib().glass_last_error_string()


class Buf:
    """a [rows, cols] fp32 view with ld = cols + 4, two guard rows in front and behind, in a NaN-filled flat buffer.  tail: what the
    two guard rows behind hold (inputs: Inf / NaN); fill: what the view holds before the call (accumulate: finite values)."""
    def __init__(self, rows, cols, src=None, tail=None, align=16, fill=None):
        ld = cols + 4
        self.ld, self.rows, self.cols = ld, rows, cols
        self.flat = torch.full(((rows + 4) * ld + 8, ), NAN, device=DEV)
        off = 2 * ld + 4
        self.v = torch.as_strided(self.flat, (rows, cols), (ld, 1), off)
        assert self.v.data_ptr() % align == 0
        if src is not None:
            self.v.copy_(torch.as_tensor(src))
        if fill is not None:
            self.v.copy_(fill)
        if tail is not None:
            torch.as_strided(self.flat, (2, cols), (ld, 1), off + rows * ld).fill_(tail)
        self.inside = torch.zeros(self.flat.numel(), dtype=torch.bool, device=DEV)
        torch.as_strided(self.inside, (rows, cols), (ld, 1), off).fill_(True)
        self.before = self.flat.clone()

    @property
    def ptr(self):
        return self.v.data_ptr()

    def check(self, tag, allow_nan=False, untouched=False):
        assert bool(torch.isnan(self.flat[~self.inside]).all()), f"{tag}: written outside its view (guard rows / columns)"
        if untouched:
            assert torch.equal(self.flat.view(torch.int32), self.before.view(torch.int32)), f"{tag}: written although not asked for"
        elif not allow_nan:
            assert not bool(torch.isnan(self.flat[self.inside]).any()), f"{tag}: NaN or unwritten element inside its view"
        return self

    def cpu(self):
        return self.v.detach().cpu()


class Workspace:
    """exactly glass_linear_wgrad_ws_bytes(N, O, I) bytes of 0xFF (NaN words) with a 256-byte canary behind them"""
    def __init__(self, N, O, I):
        self.n = int(_lib().glass_linear_wgrad_ws_bytes(N, O, I))
        assert self.n == WO.ws_bytes(N, O, I)
        self.raw = torch.full((self.n + 256, ), 0xFF, dtype=torch.uint8, device=DEV)
        self.raw[self.n:] = 0xA5
        assert self.raw.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.raw.data_ptr()

    def check(self, tag):
        assert bool((self.raw[self.n:] == 0xA5).all()), f"{tag}: written behind the workspace"


def _bits(t):
    return t.view(torch.int32)


def _note(route, f32p, sw, sb, tag):
    key = (route, "f32" if f32p else "split")
    w = _WORST.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], sw), max(w[1], sb)
    print(f"wgrad {tag}: dW {sw:.3f} db {sb:.3f}")


def _grade(route, f32p, got, truth, tag, db=True):
    a = WO.gate(got[0], truth[0], truth[1])
    b = WO.gate(got[1], truth[2], truth[3]) if db else (True, 0.0, -1)
    _note(route, f32p, a[1], b[1], tag)
    assert a[0], f"{tag}: dW misses the bar: share {a[1]:.3g} at flat index {a[2]}"
    assert b[0], f"{tag}: db misses the bar: share {b[1]:.3g} at index {b[2]}"


# ---- the two entries ------------------------------------------------------------------------------------------------------------------
def _reduce_batch(ws, N, O, I, dW, db, accumulate):
    a = lambda v, dt: np.array([v], dtype=dt)
    args = (a(ws.ptr, np.uint64), a(N, np.int64), a(O, np.int64), a(I, np.int64), a(dW.ptr, np.uint64), a(dW.ld, np.int64),
            a(db.ptr if db is not None else 0, np.uint64), a(accumulate, np.int32))
    _ok(_lib().glass_linear_wgrad_reduce_batch_f32(1, *[x.ctypes.data for x in args], None, _stream()))


def run_dual(p, mask, z, act, f32p, want_db=True, old=None, deferred=False, allow_nan=False, over=None):
    """one dual call, twice -> (dW, db) on the CPU (db: the buffer's content, untouched when want_db is False).  old = (W, b): accumulate
    onto them.  deferred: dW == NULL, then glass_linear_wgrad_reduce_batch_f32.  over: operands replaced by name."""
    lib = _lib()
    N, H, comb = p["N"], p["H"], p["comb"]
    O, I = 2 * H, (2 * H if comb else H)
    q = dict(p, **(over or {}))
    d = Buf(N, H, q["dsrc"], tail=INF)
    T = Buf(N, 2 * H, q["T"], tail=NAN) if act else None
    X = Buf(N, H, q["X"], tail=NAN)
    X2 = Buf(N, H, q["X2"], tail=INF) if comb else None
    m = torch.ones(N + 8, dtype=torch.uint8, device=DEV)
    m[:N] = torch.as_tensor(np.asarray(mask))
    res = []
    for _ in range(2):
        dW = Buf(O, I, fill=None if old is None else old[0].to(DEV))
        db = Buf(1, O, fill=None if old is None else old[1].to(DEV).reshape(1, -1))
        ws = Workspace(N, O, I)
        give_db = want_db or deferred
        _ok(lib.glass_dual_linear_wgrad_f32(d.ptr, d.ld, T.ptr if T else None, T.ld if T else 0, m.data_ptr(), z, _act_word(act, f32p), X.ptr, X.ld,
                                            X2.ptr if comb else None, X2.ld if comb else 0, N, H, None if deferred else dW.ptr, dW.ld,
                                            db.ptr if (give_db and not deferred) else None, 0 if old is None else 1, ws.ptr, _stream()))
        if deferred:
            torch.cuda.synchronize()
            dW.check("dW before the deferred reduce", untouched=True)
            _reduce_batch(ws, N, O, I, dW, db if want_db else None, 0 if old is None else 1)
        torch.cuda.synchronize()
        ws.check("workspace")
        dW.check("dW", allow_nan)
        db.check("db", allow_nan, untouched=not want_db)
        res.append((dW, db))
    assert torch.equal(_bits(res[0][0].flat), _bits(res[1][0].flat)) and torch.equal(_bits(res[0][1].flat), _bits(res[1][1].flat)), "the second run differs"
    return res[0][0].cpu(), res[0][1].cpu().reshape(-1)


def run_linear(p, N, want_db=True, old=None):
    lib = _lib()
    O, I = p["O"], p["I"]
    G = Buf(N, O, p["G"][:N], tail=INF, align=4)
    X = Buf(N, I, p["X"][:N], tail=NAN, align=8)
    res = []
    for _ in range(2):
        dW = Buf(O, I, fill=None if old is None else old[0].to(DEV), align=4)
        db = Buf(1, O, fill=None if old is None else old[1].to(DEV).reshape(1, -1), align=4)
        ws = Workspace(N, O, I)
        _ok(lib.glass_linear_wgrad_f32(G.ptr, G.ld, X.ptr, X.ld, N, O, I, dW.ptr, dW.ld, db.ptr if want_db else None, 0 if old is None else 1, ws.ptr, _stream()))
        torch.cuda.synchronize()
        ws.check("workspace")
        dW.check("dW")
        db.check("db", untouched=not want_db)
        res.append((dW, db))
    assert torch.equal(_bits(res[0][0].flat), _bits(res[1][0].flat)) and torch.equal(_bits(res[0][1].flat), _bits(res[1][1].flat)), "the second run differs"
    return res[0][0].cpu(), res[0][1].cpu().reshape(-1)


def _old(O, I, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(O, I, generator=g), torch.randn(O, generator=g)


# ---- glass_linear_wgrad_f32 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", WO.THIN_I)
@pytest.mark.parametrize("O", WO.THIN_O)
def test_thin_kernels(O, I):
    """N = 1, 63, 64, 65 (one block, a ragged block, two blocks) and 65 537 (past the 1 024-block cap: 65 rows per block); I = 260 walks
    two column chunks; db == NULL and accumulate at N = 65; the exact probe at N = 65 and 65 537"""
    for N in WO.THIN_N:
        form = WO.route("linear", N, (O, I))
        assert form["kernels"] == [f"wgrad_thin_partial_kernel<{O}>", "wgrad_thin_reduce_kernel"]
        assert form["thin_blocks"] == min(-(-N // 64), 1024) and form["rows"] == -(-N // form["thin_blocks"])
        p = _linear_recipe(N, O, I)
        tag = f"thin O={O} I={I} N={N}"
        _grade("thin", True, run_linear(p, N), _linear_truth(N, O, I), tag)
        if N in (65, 65537):
            _linear_probe(form, N, O, I, tag)
        if N == 65:
            old = _old(O, I)
            _grade("thin", True, run_linear(p, N, old=old), WO.truth_linear(p["G"], p["X"], *old), tag + " accumulate")
            gw, _ = run_linear(p, N, want_db=False)
            _grade("thin", True, (gw, None), _linear_truth(N, O, I), tag + " db NULL", db=False)


def _linear_probe(form, N, O, I, tag):
    """every live row feeds elements of dW (small O: the live rows in groups, told apart by input columns)"""
    for live in WO.probe_groups_linear(WO.probe_rows(form, N), O, I):
        pp = WO.probe_recipe_linear(N, O, I, live)
        assert all(bool(pp["G"][r].any()) and bool(pp["X"][r].any()) for r in live)
        tw = WO.truth_linear(pp["G"], pp["X"])
        w, b = WO.probe_expect(tw[0], tw[2])
        gw, gb = run_linear(pp, N)
        assert WO.bits_equal(gw.numpy(), w) and WO.bits_equal(gb.numpy(), b), tag + f": the probe is not bit-exact (live rows {live})"


@functools.lru_cache(maxsize=None)
def _linear_recipe(N, O, I):
    return WO.recipe_linear(N, O, I)


@functools.lru_cache(maxsize=None)
def _linear_truth(N, O, I):
    p = _linear_recipe(N, O, I)
    return WO.truth_linear(p["G"], p["X"], device=DEV if N >= TRUTH_DEV else "cpu")


@pytest.mark.parametrize("O,I", WO.PLAIN_SHAPES)
def test_plain_kernel(O, I):
    """wgrad_partial_kernel<false, false>: partial tiles in O and I ((4, 2), (40, 20), (132, 66): a second, nearly empty tile), N = 1 ..
    65; (128, 64): one slab edge - 1 / 0 / + 1 of the restated geometry and N = 100 000 / 100 001 (kFusedBwdMaxRows: the slab rounding
    changes); db == NULL, accumulate and the exact probe at N = 65"""
    ns = WO.plain_rows(O, I)
    if (O, I) == (128, 64):
        rows = WO.route("linear", 333, (O, I))["rows"]
        assert ns[5:8] == [3 * rows - 1, 3 * rows, 3 * rows + 1] and WO.route("linear", ns[6], (O, I))["n_slabs"] == 3 and WO.route("linear", ns[7], (O, I))["n_slabs"] == 4
        assert WO.wgrad_geom(100000, O, I)["rows"] % 32 == 0 and WO.wgrad_geom(100001, O, I)["rows"] % 32 != 0
    for N in ns:
        form = WO.route("linear", N, (O, I))
        assert form["kernels"][0] == "wgrad_partial_kernel<false, false>" and (form["ny"], form["nz"]) == (-(-I // 64), -(-O // 128))
        p = _linear_recipe(N, O, I)
        tag = f"plain O={O} I={I} N={N}"
        _grade("plain", True, run_linear(p, N), _linear_truth(N, O, I), tag)
        if N == 65 or N == 100001:
            _linear_probe(form, N, O, I, tag)
        if N == 65:
            old = _old(O, I)
            _grade("plain", True, run_linear(p, N, old=old), WO.truth_linear(p["G"], p["X"], *old), tag + " accumulate")
            gw, _ = run_linear(p, N, want_db=False)
            _grade("plain", True, (gw, None), _linear_truth(N, O, I), tag + " db NULL", db=False)


# ---- glass_dual_linear_wgrad_f32 ------------------------------------------------------------------------------------------------------
ROUTES = WO.ROUTES   # name: (H, comb, act, N, first kernel with split products, with f32 products)


def _forms(name):
    return [f for f in (False, True) if ROUTES[name][5 if f else 4] is not None]


@functools.lru_cache(maxsize=None)
def _recipe(N, H, comb):
    if N < BIG:
        return WO.recipe(N, H, comb)
    g = torch.Generator(DEV).manual_seed(7919 * H + 31 * N + int(comb))
    r = lambda *s: torch.randn(*s, generator=g, device=DEV)
    return dict(N=N, H=H, comb=comb, dsrc=r(N, H), T=r(N, 2 * H) * 1.5, X=r(N, H) + 0.25, X2=(r(N, H) - 0.25) if comb else None)


def _form(name, f32p, N=None, act=None):
    H, comb, a, n = ROUTES[name][:4]
    form = WO.route("dual", N or n, H, comb, a if act is None else act, f32p)
    if N is None and act is None:
        assert form["kernels"][0] == ROUTES[name][5 if f32p else 4], (name, form["kernels"])
    return form


@functools.lru_cache(maxsize=None)
def _truth(N, H, comb, act, mask_key, z, eff):
    p = _recipe(N, H, comb)
    return WO.truth_dual(p["dsrc"], p["T"], _MASKS[mask_key], z, act, p["X"], p["X2"], eff, device=DEV if N >= TRUTH_DEV else "cpu")


_MASKS = {}


def _mask(key, make):
    if key not in _MASKS:
        _MASKS[key] = make()
    return key


def _case(name, f32p, mask_key, z, tag, N=None, **kw):
    H, comb, act, n = ROUTES[name][:4]
    N = N or n
    form = _form(name, f32p, N)
    p = _recipe(N, H, comb)
    got = run_dual(p, _MASKS[mask_key], z, act, f32p, **kw)
    _grade(name, f32p, got, _truth(N, H, comb, act, mask_key, z, form["eff"]), tag)
    return got


@pytest.mark.parametrize("pattern", WO.PATTERNS)
@pytest.mark.parametrize("name", list(ROUTES))
def test_label_patterns_on_every_route(name, pattern):
    """none; all; only row N - 1; only the first row of a slab; one whole slab; one per slab; every row of one 16-row stage"""
    H, comb, act, N = ROUTES[name][:4]
    for f32p in _forms(name):
        form = _form(name, f32p)
        assert form["eff"] == (comb and act == 0 and H in (128, 256, 512)) and form["split"] == ((not f32p) and H in (128, 256, 512))
        key = _mask((name, pattern), lambda: WO.label_pattern(pattern, N, form))
        _case(name, f32p, key, Z, f"{name} {pattern} f32={int(f32p)}")


@pytest.mark.parametrize("z", [0.5, 1.0, 0.3])
@pytest.mark.parametrize("name", list(ROUTES))
def test_z_values_on_every_route(name, z):
    """z = 0.5: the labeled-rows coefficient of the effective-weight combine is zero; z = 1: the all-rows coefficient of the first half
    and the unlabeled coefficient of the plain form are zero; z = 0.3: the signs flip.  A third of the rows labeled, row N - 1 too."""
    N = ROUTES[name][3]
    for f32p in _forms(name):
        key = _mask((name, "random"), lambda: _random_mask(N))
        _case(name, f32p, key, z, f"{name} z={z} f32={int(f32p)}")


def _random_mask(N):
    m = WO.random_mask(N, N)
    m[N - 1] = 1
    return m


@pytest.mark.parametrize("name", list(ROUTES))
def test_launch_forms_on_every_route(name):
    """db == NULL with dW given (db untouched, dW right and bit-equal to the call with db); accumulate = 1 with lddw > I on the
    partial-producing call itself; dW == NULL followed by glass_linear_wgrad_reduce_batch_f32, bit-equal to the direct call"""
    H, comb, act, N = ROUTES[name][:4]
    O, I = 2 * H, (2 * H if comb else H)
    for f32p in _forms(name):
        form = _form(name, f32p)
        key = _mask((name, "random"), lambda: _random_mask(N))
        p = _recipe(N, H, comb)
        tag = f"{name} f32={int(f32p)}"
        direct = _case(name, f32p, key, Z, tag + " direct")
        gw, gb = run_dual(p, _MASKS[key], Z, act, f32p, want_db=False)
        assert torch.equal(_bits(gw), _bits(direct[0])), tag + ": dW differs without db"
        dw, dbv = run_dual(p, _MASKS[key], Z, act, f32p, deferred=True)
        assert torch.equal(_bits(dw), _bits(direct[0])) and torch.equal(_bits(dbv), _bits(direct[1])), tag + ": the deferred reduce differs from the direct call"
        old = _old(O, I)
        got = run_dual(p, _MASKS[key], Z, act, f32p, old=old)
        tw = _truth(N, H, comb, act, key, Z, form["eff"])
        o64 = (old[0].double(), old[1].double())
        _grade(name, f32p, got, (tw[0] + o64[0], tw[1] + o64[0].abs(), tw[2] + o64[1], tw[3] + o64[1].abs()), tag + " accumulate")


EXTRA_ROWS = WO.EXTRA_ROWS


@pytest.mark.parametrize("name,N", EXTRA_ROWS)
def test_row_counts_and_slab_edges(name, N):
    """the neighbours of each route's row count where the last slab's raggedness changes (a whole last slab, one row into the next);
    hidden 128 beyond the wgrad128 kernels' 400 000 rows: the last of the 64 slabs of 6 256 rows one row short and whole, and one row
    more, where the geometry takes 6 264-row slabs; both ends of the wgrad128 range; 71 680 rows at hidden 256: 128 slabs, the XCD
    placement of the eight-wave kernel"""
    H, comb, act, n = ROUTES[name][:4]
    for f32p in _forms(name):
        form = _form(name, f32p, N)
        base = _form(name, f32p)
        if N in (3008, 4176, 400384):
            assert N % form["rows"] == 0 and form["rows"] == base["rows"] and form["n_slabs"] == base["n_slabs"]
        if N in (3009, 4177):
            assert N % form["rows"] == 1 and form["rows"] == base["rows"] and form["n_slabs"] == base["n_slabs"] + 1
        if N == 400383:
            assert (form["rows"], form["n_slabs"]) == (6256, 64) == (base["rows"], base["n_slabs"]) and (N + 1) % form["rows"] == 0
        if N == 400385:
            assert form["family"] == "generic" and (form["rows"], form["n_slabs"]) == (6264, 64)
        if N == 71680:
            assert form["n_slabs"] == 128 and form["placement"] == (None if f32p else "xcd")
        if name.startswith("w128"):
            assert form["family"] == ("generic" if f32p else "wgrad128")
        key = _mask((name, N, "random"), lambda: _random_mask(N))
        _case(name, f32p, key, Z, f"{name} N={N} f32={int(f32p)}", N=N)


@pytest.mark.parametrize("N,kind", [(50003, "chunk_edges"), (50003, "one_chunk"), (63488, "all"), (63489, "all"), (8193, "all")])
def test_wgrad128_comb_list_tiles_at_the_chunk_boundaries(N, kind):
    """the list workgroups of wgrad128_comb_kernel: labeled rows exactly at the first and last row of every chunk; one whole chunk
    labeled; every row labeled at N = 16 * kW128ListCap (every list full to the cap) and one row more (17 lists)"""
    form = WO.route("dual", N, 128, True)
    assert form["kernels"][0] == "wgrad128_comb_kernel" and form["n_lists"] == (17 if N == 63489 else 16)
    ch = WO.list_chunks(form, N)
    assert max(e - a for a, e in ch) <= WO.LIST_CAP and (N != 63488 or ch[0][1] - ch[0][0] == WO.LIST_CAP)

    def make():
        m = np.zeros(N, np.uint8)
        if kind == "all":
            m[:] = 1
        elif kind == "one_chunk":
            m[ch[7][0]:ch[7][1]] = 1
        else:
            for a, e in ch:
                m[a], m[e - 1] = 1, 1
        return m
    key = _mask(("w128 comb", N, kind), make)
    _case("w128 comb", False, key, Z, f"w128 comb lists N={N} {kind}", N=N)


# ---- exact probes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z", WO.PROBE_Z)
@pytest.mark.parametrize("name", list(ROUTES))
def test_exact_probes_on_every_route(name, z):
    """every element of dW and db is one product that fp32 holds exactly: bit equality, in both product forms, with every live row seen
    labeled and unlabeled; trans pairs also under ReLU"""
    H, comb, act, N = ROUTES[name][:4]
    for f32p in _forms(name):
        form = _form(name, f32p)
        live = WO.probe_rows(form, N)
        for relu in ((False, True) if (act and not comb) else (False, )):
            assert WO.route("dual", N, H, comb, 2 if relu else 0, f32p)["family"] == form["family"]
            p = WO.probe_recipe(N, H, comb, live, relu=relu)
            for mask in WO.probe_masks(live, N):
                dW64, _, db64, _ = WO.truth_dual(p["dsrc"], p["T"], mask, z, p["act"], p["X"], p["X2"], False, device=DEV if N >= TRUTH_DEV else "cpu")
                w, b = WO.probe_expect(dW64, db64)
                gw, gb = run_dual(p, mask, z, p["act"], f32p)
                bad = np.nonzero(~((gw.numpy().view(np.uint32) == w.view(np.uint32)) | ((gw.numpy() == 0) & (w == 0))))
                assert WO.bits_equal(gw.numpy(), w), f"{name} f32={int(f32p)} z={z} relu={int(relu)}: dW differs from the exact value at {bad[0][:4]}, {bad[1][:4]}"
                assert WO.bits_equal(gb.numpy(), b), f"{name} f32={int(f32p)} z={z} relu={int(relu)}: db differs from the exact value"


# ---- non-finite inputs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g64 trans none", "g64 trans relu", "g64 comb", "g128 trans", "g128 comb", "g256 comb", "w128 trans", "w128 comb", "t256 trans", "t256 comb"])
def test_one_nan_stays_in_its_column_or_its_rows(name):
    """one NaN in X[n, i]: column i of dW is NaN and nothing else, db is clean.  One NaN in dsrc[n, o]: rows o and o + H of dW and of db
    are NaN and nothing else — in the effective-weight form too: S (all rows) holds the NaN in row o whether row n is labeled or not,
    and both output halves take S with a coefficient (0 * NaN = NaN at z = 1)."""
    H, comb, act, N = ROUTES[name][:4]
    I = 2 * H if comb else H
    p = _recipe(N, H, comb)
    key = _mask((name, "random"), lambda: _random_mask(N))
    n, i, o = N // 2 + 1, 7, H - 3
    for f32p in _forms(name):
        form = _form(name, f32p)
        tw = _truth(N, H, comb, act, key, Z, form["eff"])
        X = p["X"].clone()
        X[n, i] = NAN
        gw, gb = run_dual(p, _MASKS[key], Z, act, f32p, allow_nan=True, over=dict(X=X))
        nanw = torch.isnan(gw)
        assert bool(nanw[:, i].all()) and int(nanw.sum()) == 2 * H and not bool(torch.isnan(gb).any()), f"{name} f32={int(f32p)}: NaN in X"
        keep = torch.ones(I, dtype=torch.bool)
        keep[i] = False
        assert WO.gate(gw[:, keep], tw[0][:, keep], tw[1][:, keep])[0]
        d = p["dsrc"].clone()
        d[n, o] = NAN
        gw, gb = run_dual(p, _MASKS[key], Z, act, f32p, allow_nan=True, over=dict(dsrc=d))
        rows = torch.zeros(2 * H, dtype=torch.bool)
        rows[o], rows[o + H] = True, True
        assert torch.equal(torch.isnan(gw), rows[:, None].expand(-1, I)) and torch.equal(torch.isnan(gb), rows), f"{name} f32={int(f32p)}: NaN in dsrc"
        assert WO.gate(gw[~rows], tw[0][~rows], tw[1][~rows])[0] and WO.gate(gb[~rows], tw[2][~rows], tw[3][~rows])[0]


# ---- the device truth -------------------------------------------------------------------------------------------------------------------
def test_device_truth_equals_the_cpu_truth():
    p = WO.recipe(700, 128, True)
    mask = _random_mask(700)
    for eff, act in ((True, 0), (False, 1)):
        a = WO.truth_dual(p["dsrc"], p["T"], mask, Z, act, p["X"], p["X2"], eff)
        b = WO.truth_dual(p["dsrc"], p["T"], mask, Z, act, p["X"], p["X2"], eff, device=DEV)
        for x, y, m in ((a[0], b[0], a[1]), (a[1], b[1], a[1]), (a[2], b[2], a[3]), (a[3], b[3], a[3])):
            assert bool(((x - y).abs() <= 1e-12 * m).all())


# ---- the figures ------------------------------------------------------------------------------------------------------------------------
def test_zz_report_worst_shares():
    """prints the worst share of the bar per route and product form over the cases that ran in this process (file order: last)"""
    for (route, form), (w, b) in sorted(_WORST.items()):
        print(f"wgrad worst share: {route:16s} {form:5s} dW {w:.3f} db {b:.3f}")
    assert all(max(v) <= 1.0 for v in _WORST.values())
