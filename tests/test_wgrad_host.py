"""tests/wgrad_oracle.py checked on the CPU: the restated dispatch and slab geometry against the source text of linear.hip /
wgrad_common.h / wgrad128.hip / wgrad_tiled.hip and against glass_linear_wgrad_ws_bytes (host code), the gate of
tests/test_gpu_wgrad.py against the honest fp32 restatement (it must pass with room) and against one named mistake at a time (each
must be refused), the exact probes, and the two entries' argument checks that answer before any launch.

The restatement runs on the GPU file's own recipes wherever the CPU can hold them: every route of wgrad_oracle.ROUTES below 8 192
rows in each of its product forms (the same recipe, random mask and z), every plain case (100 000 / 100 001 rows included) and every
thin case (65 537 rows for the smallest and the widest shape).  Routes from 8 192 rows on (wgrad128, tiled, hidden 128 at 400 001)
use a reduced clone instead — the same kernels and walking order on slabs of 48 / 64 rows, recipes of their own (HOST_DUAL) —, and
the named mistakes are applied to HOST_DUAL recipes drawn with one row more than N (what a row past N would add).

Worst share of the 1e-5 * mass bar of the honest restatement (dW / db).  On the GPU file's recipes:
  thin 0.009 / 0.009   plain 0.014 / 0.012   hidden 64 (five routes) 0.007 / 0.004   g192 comb 0.006 / 0.003   g320 comb 0.009 / 0.004
  g128 trans 0.004 / 0.002 in both forms   g128 comb (eff) 0.003 / 0.001 in both   g256 trans split 0.006 / 0.002, f32 0.005 / 0.002
  g256 comb (eff) 0.003 / 0.001 in both
On the clones and HOST_DUAL recipes:
  generic f32 0.009 / 0.003   generic eff f32 0.005 / 0.002   generic split 0.004 / 0.002   generic eff split 0.005 / 0.003
  wgrad128 trans 0.004 / 0.003   wgrad128 comb (lists) 0.004 / 0.002   tiled f32 0.015 / 0.006   tiled split 0.009 / 0.007
  tiled eff f32 0.009 / 0.003   tiled eff split 0.007 / 0.003
The condition is < 0.5.

Mass gate against the three mistakes the probes exist for (random recipes, split products): the low bf16 piece of X dropped PASSES
it (|lo| <= 2^-18 |x|, 0.4 of the bar at most; measured share 0.08 - 0.15 — only the probes see it); the dropped hi x mid product
(the gradient's high piece times the input's middle piece, ~2^-9 of a product) and the exchanged element pair are refused by it too."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import wgrad_oracle as WO  # noqa: E402

E_ARG, E_UNSUPPORTED = -1, -3
Z = 0.8
_WORST = {}


# ---- source ties ------------------------------------------------------------------------------------------------------------------------
def test_restated_dispatch_is_tied_to_the_source_text():
    k = WO.source_constants()
    assert (k["kOT"], k["kIT"], k["kMaxSlabs"]) == (WO.K_OT, WO.K_IT, WO.MAX_SLABS) and k["kTile_text"]
    assert (k["kThinMaxO"], k["kThinMaxBlocks"]) == (WO.THIN_MAX_O, WO.THIN_MAX_BLOCKS)
    assert (k["kWO"], k["kWI"], k["kWK"]) == (WO.KWO, WO.KWI, WO.KWK)
    assert k["kFusedBwdMaxRows"] == WO.FUSED_MAX_ROWS and k["kW128ListCap"] == WO.LIST_CAP and k["header_floats"] == (WO.HEADER, WO.HEADER)
    assert k["narrow"] == (WO.NARROW_MAX_H, WO.NARROW_SLAB, True)
    for name in ("wgrad128_shape_text", "wgrad128_comb_shape_text", "tiled_shape_text", "split_widths_text", "comb_lists_text", "list_chunk_text",
                 "thin_blocks_text", "thin_entry_text", "plain_refusal_text", "geom_comb128_text", "geom_trans128_text", "geom_generic_text",
                 "tiled_geom_text", "ws_bytes_text", "eff_cond_text", "split_cond_text", "dual_refusal_text", "tiled_eff_cond_text",
                 "tiled_refusals_text", "placement_text"):
        assert k[name], f"{name}: the source text the restatement was written against moved"
    assert k["route_chain_text"] == WO.ROUTE_CHAIN, k["route_chain_text"]
    assert tuple((int(a), int(b)) for a, b in k["split_order"]) == WO.SPLIT_ORDER


def test_restated_geometry_values():
    g = WO.wgrad_geom(3001, 256, 128)
    assert (g["rows"], g["n_slabs"], g["ny"], g["nz"]) == (64, 47, 2, 2)
    g = WO.wgrad_geom(400001, 256, 256)
    assert (g["rows"], g["n_slabs"]) == (6256, 64)
    g = WO.wgrad_geom(4099, 512, 512)
    assert (g["rows"], g["n_slabs"], g["nz"]) == (144, 29, 4)
    g = WO.wgrad_geom(50003, 256, 256)
    assert (g["rows"], g["n_slabs"]) == (224, 224) and WO.wgrad128_comb_lists(50003) == 16 and WO.wgrad128_comb_lists(63489) == 17
    g = WO.wgrad_geom(8192, 256, 128)
    assert (g["rows"], g["n_slabs"]) == (64, 128)
    t = WO.wgrad_tiled_geom(65553, 512, 512)
    assert (t["rows"], t["n_slabs"], t["ny"], t["nz"]) == (528, 125, 2, 4)
    assert WO.wgrad_tiled_geom(71680, 512, 256)["n_slabs"] == 128 and WO.wgrad_tiled_geom(65576, 1024, 512)["n_slabs"] == 32
    assert [WO.thin_blocks(n) for n in (1, 64, 65, 65536, 65537)] == [1, 1, 2, 1024, 1024]
    r = WO.route("dual", 400000, 128, False, 1)
    assert r["kernels"][0] == "wgrad128_trans_kernel" and WO.route("dual", 400001, 128, False, 1)["kernels"][0] == "wgrad_partial_split_kernel<true, false>"
    assert WO.route("dual", 8191, 128, True)["kernels"][0] == "wgrad_partial_split_kernel<false, true>"
    assert WO.route("dual", 8192, 128, True)["kernels"][0] == "wgrad128_comb_kernel"
    assert WO.route("dual", 8192, 128, True, f32_products=True)["kernels"][0] == "wgrad_partial_kernel<true, true>"
    assert WO.route("dual", 8192, 128, True, aligned4=False)["kernels"][0] == "wgrad_partial_split_kernel<false, true>"
    assert WO.route("dual", 333, 192, True)["kernels"][0] == "wgrad_partial_kernel<true, false>" and WO.route("dual", 333, 192, True)["nz"] == 3
    # hidden 64: ONE output tile (nz = 1), so the comb pair takes the plain form here (its S / L form lives in dense.hip's fused launch)
    assert not WO.route("dual", 333, 64, True)["eff"] and WO.route("dual", 333, 64, True)["kernels"][0] == "wgrad_partial_kernel<true, false>"
    assert WO.route("dual", 333, 128, True, f32_products=True)["eff"] and not WO.route("dual", 333, 128, True, act=1)["eff"] and not WO.route("dual", 333, 64, True)["split"]
    assert WO.route("dual", 65535, 256, True)["family"] == "generic" and WO.route("dual", 65536, 256, True)["family"] == "tiled"
    r = WO.route("dual", 71680, 256, True)
    assert r["kernels"] == ["tiled_wgrad8_kernel<true>", "tiled_wgrad_kernel<true, true, true>", "tiled_wgrad_reduce_kernel"] and r["placement"] == "xcd"
    assert WO.route("dual", 65553, 256, False, 1)["placement"] == "plain"
    assert WO.route("dual", 65553, 256, True, f32_products=True)["kernels"][0] == "tiled_wgrad_kernel<true, true, false>"
    assert WO.route("linear", 65537, (3, 260))["kernels"][0] == "wgrad_thin_partial_kernel<3>" and WO.route("linear", 65537, (3, 260))["rows"] == 65
    assert WO.route("linear", 5, (4, 2))["family"] == "generic"


# ---- workspace bytes -------------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_equal_the_host_code():
    from glass_amd import _lib
    lib = _lib.load()
    shapes = [(o, i) for o in WO.THIN_O for i in WO.THIN_I] + list(WO.PLAIN_SHAPES) + [(2 * h, k * h) for h in (64, 128, 192, 256, 320, 512) for k in (1, 2)]
    ns = sorted(set(WO.GPU_ROW_COUNTS) | {b + d for b in (8192, 65536, 100000, 400000) for d in (-1, 0, 1)})
    for O, I in shapes:
        for N in ns:
            assert WO.ws_bytes(N, O, I) == lib.glass_linear_wgrad_ws_bytes(N, O, I), (N, O, I)
    assert lib.glass_linear_wgrad_ws_bytes(0, 4, 4) == E_ARG


# ---- the gate on the fp32 restatement ---------------------------------------------------------------------------------------------------
def _clone(form, rows, N, n_lists=0):
    """a form with the same kernels and walking order at a slab size the CPU can restate"""
    return dict(form, rows=rows, n_slabs=WO._cdiv(N, rows), n_lists=n_lists)


def _np(t):
    return None if t is None else t.numpy()


@functools.lru_cache(maxsize=None)
def _dual_case(name):
    H, comb, act, N, f32p, clone = HOST_DUAL[name]
    form = WO.route("dual", clone[0] if clone else N, H, comb, act, f32p)
    if clone:
        form = _clone(form, clone[1], N, 16 if form["n_lists"] else 0)
    p = WO.recipe(N + 1, H, comb)     # one row more: what a row past N would add
    mask = WO.random_mask(N, N)
    mask[N - 1] = 1
    return form, p, mask


HOST_DUAL = {   # name: (H, comb, act, N, f32 products, (route's N, clone rows) or None)
    "generic f32 trans64 elu": (64, False, 1, 333, True, None), "generic f32 trans64 relu": (64, False, 2, 333, True, None),
    "generic f32 comb64 elu": (64, True, 1, 333, True, None), "generic f32 comb64": (64, True, 0, 333, True, None),
    "generic f32 comb192": (192, True, 0, 150, True, None),
    "generic f32 trans128": (128, False, 1, 700, True, None), "generic eff f32 comb128": (128, True, 0, 700, True, None),
    "generic split trans128": (128, False, 1, 700, False, None), "generic split trans128 none": (128, False, 0, 700, False, None),
    "generic eff split comb128": (128, True, 0, 700, False, None), "generic eff split comb256": (256, True, 0, 300, False, None),
    "wgrad128 trans": (128, False, 1, 700, False, (8193, 64)), "wgrad128 comb (lists)": (128, True, 0, 700, False, (8193, 64)),
    "tiled f32 trans256": (256, False, 2, 200, True, (65553, 48)), "tiled split trans256": (256, False, 1, 200, False, (65553, 48)),
    "tiled eff f32 comb256": (256, True, 0, 200, True, (65553, 48)), "tiled eff split comb256": (256, True, 0, 200, False, (65553, 48)),
}


def _note(key, sw, sb):
    w = _WORST.setdefault(key, [0.0, 0.0])
    w[0], w[1] = max(w[0], sw), max(w[1], sb)


def _gate_dual(form, p, mask, N, got, z=Z, act=0, old=None):
    cut = lambda t: None if t is None else t[:N]
    tw = WO.truth_dual(cut(p["dsrc"]), cut(p["T"]), mask, z, act, cut(p["X"]), cut(p["X2"]), form["eff"], *(old or (None, None)))
    a = WO.gate(torch.from_numpy(got[0]), tw[0], tw[1])
    b = WO.gate(torch.from_numpy(got[1]), tw[2], tw[3])
    return a, b


@pytest.mark.parametrize("name", list(HOST_DUAL))
def test_dual_gate_passes_the_restatement(name):
    H, comb, act, N, f32p, _ = HOST_DUAL[name]
    form, p, mask = _dual_case(name)
    assert form["split"] == ((not f32p) and H in WO.SPLIT_WIDTHS)
    got = WO.restate_dual(form, _np(p["dsrc"]), _np(p["T"]), mask, Z, act, _np(p["X"]), _np(p["X2"]), N)
    a, b = _gate_dual(form, p, mask, N, got, act=act)
    print(f"wgrad host {name}: dW {a[1]:.3f} db {b[1]:.3f}")
    assert a[0] and b[0] and a[1] < 0.5 and b[1] < 0.5, (a, b)
    _note(name, a[1], b[1])


GPU_DUAL = [(n, f) for n, r in WO.ROUTES.items() if r[3] < 8192 for f in (False, True) if r[5 if f else 4] is not None]


@pytest.mark.parametrize("name,f32p", GPU_DUAL)
def test_dual_gate_passes_the_restatement_on_the_gpu_files_own_recipes(name, f32p):
    """every route of tests/test_gpu_wgrad.py below 8 192 rows, on the very recipe, random mask and z it uses there"""
    H, comb, act, N = WO.ROUTES[name][:4]
    form = WO.route("dual", N, H, comb, act, f32p)
    assert form["kernels"][0] == WO.ROUTES[name][5 if f32p else 4]
    p = WO.recipe(N, H, comb)
    mask = WO.random_mask(N, N)
    mask[N - 1] = 1
    got = WO.restate_dual(form, _np(p["dsrc"]), _np(p["T"]), mask, Z, act, _np(p["X"]), _np(p["X2"]), N)
    a, b = _gate_dual(form, p, mask, N, got, act=act)
    print(f"wgrad host gpu recipe {name} f32={int(f32p)}: dW {a[1]:.3f} db {b[1]:.3f}")
    assert a[0] and b[0] and a[1] < 0.5 and b[1] < 0.5, (a, b)
    _note(f"gpu recipe {name} {'f32' if f32p else 'split'}", a[1], b[1])


GPU_LINEAR = ([(o, i, n) for o in WO.THIN_O for i in WO.THIN_I for n in WO.THIN_N if n < 8192 or (o, i) in ((1, 4), (3, 260))] +
              [(o, i, n) for o, i in WO.PLAIN_SHAPES for n in WO.plain_rows(o, i)])


@pytest.mark.parametrize("O,I,N", GPU_LINEAR)
def test_linear_gate_passes_the_restatement_on_the_gpu_files_own_recipes(O, I, N):
    """every thin and plain case of the GPU file (the thin kernels at 65 537 rows for the smallest and the widest shape)"""
    form = WO.route("linear", N, (O, I))
    p = WO.recipe_linear(N, O, I)
    tw = WO.truth_linear(p["G"], p["X"])
    got = WO.restate_linear(form, p["G"].numpy(), p["X"].numpy(), N)
    a, b = WO.gate(torch.from_numpy(got[0]), tw[0], tw[1]), WO.gate(torch.from_numpy(got[1]), tw[2], tw[3])
    assert a[0] and b[0] and a[1] < 0.5 and b[1] < 0.5, (a, b)
    _note("gpu recipe thin" if form["family"] == "thin" else "gpu recipe plain", a[1], b[1])


LINEAR_HOST = [(1, 4, 65), (2, 20, 130), (3, 260, 200), (3, 64, 1), (4, 2, 5), (40, 20, 65), (132, 66, 200), (128, 64, 333)]


@pytest.mark.parametrize("O,I,N", LINEAR_HOST)
def test_linear_gate_passes_the_restatement_and_refuses_row_mistakes(O, I, N):
    form = WO.route("linear", N, (O, I))
    if form["family"] == "thin":
        form = dict(form, rows=max(form["rows"] // 2, 1), thin_blocks=WO._cdiv(N, max(form["rows"] // 2, 1)), n_slabs=WO._cdiv(N, max(form["rows"] // 2, 1)))
    p = WO.recipe_linear(N + 1, O, I)
    old_W, old_b = torch.randn(O, I, generator=torch.Generator().manual_seed(3)), torch.randn(O, generator=torch.Generator().manual_seed(4))
    tw = WO.truth_linear(p["G"][:N], p["X"][:N], old_W, old_b)
    run = lambda mut=None: WO.restate_linear(form, p["G"].numpy(), p["X"].numpy(), N, old_W.numpy(), old_b.numpy(), mut)
    got = run()
    a, b = WO.gate(torch.from_numpy(got[0]), tw[0], tw[1]), WO.gate(torch.from_numpy(got[1]), tw[2], tw[3])
    print(f"wgrad host linear {form['family']} O={O} I={I} N={N}: dW {a[1]:.3f} db {b[1]:.3f}")
    assert a[0] and b[0] and a[1] < 0.5 and b[1] < 0.5
    _note("thin" if form["family"] == "thin" else "plain f32", a[1], b[1])
    for mut in ("drop_slab_last_row", "row_past_N", "accumulate_overwrites") + (("slab_first_row_twice", ) if N > form["rows"] else ()):
        bad = run(mut)
        assert not (WO.gate(torch.from_numpy(bad[0]), tw[0], tw[1])[0] and WO.gate(torch.from_numpy(bad[1]), tw[2], tw[3])[0]), f"the gate took {mut}"


# ---- named mistakes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["generic eff split comb128", "generic eff f32 comb128", "generic split trans128", "wgrad128 comb (lists)", "tiled eff split comb256",
                                  "generic f32 comb64 elu"])
def test_each_named_mistake_is_refused_by_the_gate(name):
    assert _gate_refusals(name)


@functools.lru_cache(maxsize=None)
def _gate_refusals(name):
    """-> the mistakes that applied to this recipe (each asserted refused)"""
    refused = set()
    H, comb, act, N, f32p, _ = HOST_DUAL[name]
    form, p, mask = _dual_case(name)
    g = torch.Generator().manual_seed(11)
    old = (torch.randn(2 * H, form["I"], generator=g), torch.randn(2 * H, generator=g))
    run = lambda mut=None: WO.restate_dual(form, _np(p["dsrc"]), _np(p["T"]), mask, Z, act, _np(p["X"]), _np(p["X2"]), N, old[0].numpy(), old[1].numpy(), mut)
    a, b = _gate_dual(form, p, mask, N, run(), act=act, old=old)
    assert a[0] and b[0] and a[1] < 0.5 and b[1] < 0.5, "the honest restatement with accumulate"
    applies = {"drop_slab_last_row": True, "row_past_N": True, "slab_first_row_twice": True, "label_as_unlabeled": True, "swap_cs_cl": form["eff"],
               "L_all_rows": form["eff"], "bias_tile1_to_tile0": 2 * H >= 256, "accumulate_overwrites": True, "swap_input_halves": comb,
               "drop_mid_hi": form["split"], "swap_pair_in_tile": True}
    for mut, on in applies.items():
        if not on:
            continue
        a, b = _gate_dual(form, p, mask, N, run(mut), act=act, old=old)
        assert not (a[0] and b[0]), f"{name}: the gate took {mut}"
        refused.add(mut)
    if form["split"]:
        a, b = _gate_dual(form, p, mask, N, run("drop_lo_x"), act=act, old=old)
        assert a[0] and b[0], "the mass gate alone does NOT see a dropped low bf16 piece (|lo| <= 2^-18 |x|): the probes exist for it"
        print(f"wgrad host {name}: drop_lo_x under the mass gate at share {a[1]:.3f}")
    return frozenset(refused)


@pytest.mark.parametrize("z", WO.PROBE_Z)
@pytest.mark.parametrize("name", ["generic eff split comb128", "generic split trans128", "wgrad128 comb (lists)", "tiled eff split comb256", "generic eff f32 comb128"])
def test_exact_probes_hold_bit_for_bit_and_refuse_the_three_fine_mistakes(name, z):
    assert _probe_refusals(name, z)


@functools.lru_cache(maxsize=None)
def _probe_refusals(name, z):
    refused = set()
    H, comb, act, N, f32p, _ = HOST_DUAL[name]
    form, _, _ = _dual_case(name)
    live = WO.probe_rows(form, N)
    assert N - 1 in live and 0 in live and len(live) <= 16
    for relu in (False, True):
        f = form if not relu else dict(form, eff=False)   # (an activation takes the plain form)
        p = WO.probe_recipe(N, H, comb, live, relu=relu)
        for mask in WO.probe_masks(live, N):
            assert WO.probe_is_exact(f, p, mask, z), (name, z, relu)
            dW64, _, db64, _ = WO.truth_dual(p["dsrc"], p["T"], mask, z, p["act"], p["X"], p["X2"], False)
            w, b = WO.probe_expect(dW64, db64)
            assert np.count_nonzero(w) >= (w.size // 16) * len(live) // (2 if relu else 1) // 2
            for mut in WO.PROBE_MUTANTS:
                if mut != "swap_pair_in_tile" and not f["split"]:
                    continue
                gw, gb = WO.restate_dual(f, _np(p["dsrc"]), _np(p["T"]), mask, z, p["act"], _np(p["X"]), _np(p["X2"]), N, mut=mut)
                assert not (WO.bits_equal(gw, w) and WO.bits_equal(gb, b)), f"{name}: the probe took {mut}"
                refused.add(mut)
    return frozenset(refused)


def test_linear_probe_is_exact_and_every_live_row_feeds_dw():
    for O, I, N in ((1, 4, 200), (3, 260, 200), (4, 2, 200), (132, 66, 200)):
        form = WO.route("linear", N, (O, I))
        rows = WO.probe_rows(form, N)
        groups = WO.probe_groups_linear(rows, O, I)
        assert sorted(r for g in groups for r in g) == rows
        for live in groups:
            p = WO.probe_recipe_linear(N, O, I, live)
            tw = WO.truth_linear(p["G"], p["X"])
            w, b = WO.probe_expect(tw[0], tw[2])
            for r in live:   # the row alone gives elements of dW that the whole probe holds unchanged: single products
                one = p["G"][r].double()[:, None] * p["X"][r].double()[None, :]
                assert bool(one.any()) and bool((tw[0][one != 0] == one[one != 0]).all()), (O, I, r)
            gw, gb = WO.restate_linear(form, p["G"].numpy(), p["X"].numpy(), N)
            assert WO.bits_equal(gw, w) and WO.bits_equal(gb, b)


def test_zz_every_named_mistake_was_refused_somewhere():
    """one recipe covers the list (the results are shared with the tests above when they ran, and formed here when not)"""
    seen = _gate_refusals("generic eff split comb128") | _probe_refusals("generic eff split comb128", 0.75)
    assert seen == set(WO.MUTANTS), sorted(set(WO.MUTANTS) - seen)
    for k, (w, b) in sorted(_WORST.items()):
        print(f"wgrad host worst share: {k:36s} dW {w:.3f} db {b:.3f}")


# ---- the entries on the host ------------------------------------------------------------------------------------------------------------
def test_k5w_entry_codes_on_the_host_before_any_launch():
    """null stream, dummy non-null pointers, no launch: every refusal below answers from the entries' own checks"""
    from glass_amd import _lib
    lib = _lib.load()
    raw = np.zeros(8200, dtype=np.float32)
    buf = raw[(-raw.ctypes.data % 16) // 4:][:8192]
    p = buf.ctypes.data
    assert p % 16 == 0
    lorder = ["G", "ldg", "X", "ldx", "N", "O", "I", "dW", "lddw", "db", "acc", "ws", "stream"]
    ld = dict(G=p, ldg=8, X=p, ldx=8, N=5, O=8, I=6, dW=p, lddw=8, db=p, acc=0, ws=p, stream=None)
    lin = lambda **o: lib.glass_linear_wgrad_f32(*[dict(ld, **o)[k] for k in lorder])
    for o in (dict(G=None), dict(X=None), dict(dW=None), dict(ws=None), dict(N=0), dict(O=0), dict(I=0), dict(ldg=7), dict(ldx=5), dict(lddw=5)):
        assert lin(**o) == E_ARG, o
    for o in (dict(O=6), dict(I=5), dict(ldg=10), dict(ldx=9), dict(G=p + 4), dict(X=p + 4), dict(O=3, I=6, ldg=4), dict(O=2, I=8, ldx=10, ldg=4)):
        assert lin(**o) == E_UNSUPPORTED, o    # (O <= 3 off the thin kernel's conditions falls to the O % 4 refusal)
        assert b"linear_wgrad: needs" in lib.glass_last_error_string()
    H = 256
    dorder = ["dsrc", "ldd", "T", "ldt", "mask", "z", "act", "X", "ldx", "X2", "ldx2", "N", "H", "dW", "lddw", "db", "acc", "ws", "stream"]
    dd = dict(dsrc=p, ldd=H, T=p, ldt=2 * H, mask=p, z=Z, act=1, X=p, ldx=H, X2=None, ldx2=0, N=8, H=H, dW=p, lddw=H, db=p, acc=0, ws=p, stream=None)
    dual = lambda **o: lib.glass_dual_linear_wgrad_f32(*[dict(dd, **o)[k] for k in dorder])
    for o in (dict(dsrc=None), dict(mask=None), dict(X=None), dict(ws=None), dict(N=0), dict(H=0), dict(ldd=H - 4), dict(ldx=H - 2), dict(lddw=H - 4),
              dict(X2=p, ldx2=H - 2, lddw=2 * H), dict(X2=p, ldx2=H, lddw=2 * H - 4), dict(T=None), dict(ldt=2 * H - 4)):
        assert dual(**o) == E_ARG, o
    for o in (dict(H=96, ldt=192), dict(H=40, ldt=80), dict(ldd=H + 2), dict(ldx=H + 1), dict(X2=p, ldx2=H + 1, lddw=2 * H), dict(dsrc=p + 4), dict(X=p + 4),
              dict(X2=p + 4, ldx2=H, lddw=2 * H), dict(ldt=2 * H + 2), dict(T=p + 4)):
        assert dual(**o) == E_UNSUPPORTED, o
        assert b"dual_linear_wgrad: needs H%64==0" in lib.glass_last_error_string()
    # the tiled route (N >= 65 536 at hidden 256): its own refusals, before the launch
    big = dict(N=65553)
    assert WO.route("dual", 65553, H, False, 1)["family"] == "tiled"
    for o, msg in ((dict(ldx=H + 2), b"ld % 4 == 0"), (dict(X=p + 8), b"ld % 4 == 0"), (dict(X2=p, ldx2=H + 2, lddw=2 * H), b"ld % 4 == 0"),
                   (dict(X2=p + 8, ldx2=H, lddw=2 * H), b"ld % 4 == 0"), (dict(mask=p + 1), b"2-byte aligned label mask")):
        assert dual(**dict(big, **o)) == E_UNSUPPORTED, o
        assert msg in lib.glass_last_error_string(), o
    rows = WO.wgrad_tiled_geom(65553, 2 * H, H)["rows"]
    wide = -(-(1 << 31) // ((rows + 96) * 4))
    wide += -wide % 4
    for o in (dict(ldd=wide), dict(ldx=wide), dict(ldt=wide), dict(X2=p, ldx2=wide, lddw=2 * H, act=0)):
        assert dual(**dict(big, **o)) == E_UNSUPPORTED, o
        assert b"32-bit slab offsets" in lib.glass_last_error_string(), o
