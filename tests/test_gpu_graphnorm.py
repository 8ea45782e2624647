"""The whole-graph GraphNorm's C entries (K6: glass_graphnorm_fwd / _stats / _apply / _finalize / _stats_exact / _bwd /
_bwd_from_stats, glass_amd/csrc/graphnorm.hip) on the GPU through every launch form, graded stage by stage and element by element
against tests/graphnorm_oracle.py: every output and every workspace intermediate (saved, the partial rows or accumulator words,
coef, y, dx, the parameter gradients) against the fp64 function of the kernel's own upstream outputs at |got - want| <= 1e-5 *
mass, and every case end to end against the fp64 chain (pinned to autograd on the CPU) at rel-inf <= 1e-5.  Every workspace
starts filled with NaN, every operand has guard columns (ld > C) that must come back untouched, and every case asserts the form
the restated dispatch predicts — with the direct observation where one exists: partial rows at index nblk or above are still
NaN (the statistics grid), accumulator replicas at index n_rep or above are still zero / are never read.

Two cases fail on the parent commit's library:
  test_nonfinite_column_stays_visible[2]: ReLU through gn_apply_kernel wrote 0.0 in all N rows of the column holding a NaN
    (act_exact: `h > 0 ? h : 0`), where torch.relu and the other two activations give NaN;
  tests/test_graphnorm_host.py::test_k6_entry_codes_on_the_host_before_any_launch: the backward entries took any act code.

Worst share of the bar per stage as measured on MI355X: see MEASURED below."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import graphnorm_oracle as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
CALL_ID = 7
ACTS = (G.ACT_NONE, G.ACT_ELU, G.ACT_RELU)

MEASURED = """
  forward        sums 0.000 saved 0.005 y 0.006
  finalize       saved 0.005
  exact_stats    decoded sums 0.821 of the DERIVED bound (C = 128, `mixed`: the truncation term of five adds rules); saved 0.006
  backward       bsums 0.011 coef 0.006 dgamma 0.006 dbeta 0.008 dalpha 0.007 dx 0.030
  from_partials  coef 0.006 dgamma 0.006 dbeta 0.006 dalpha 0.006 dx 0.022
  exact_backward dgamma 0.002 dbeta 0.002 dalpha 0.001 dx 0.007
(the CPU restatement's worst: saved 0.005, y 0.007, bsums 0.007, coef 0.005, dx 0.022.)  The exact form and the partials form
gave bit-equal parameter gradients and dx in every column of every agreement case.
"""

_WORST = {}
_CACHE = {}


def _lib():
    from glass_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc):
    assert rc == 0, _lib().glass_last_error_string()


def _mat(host, ld, off=False):
    """host [N, C] on the device with row stride ld, guard columns NaN; off: the base pointer one float past 16 bytes"""
    N, C = host.shape
    buf = torch.full((N * ld + 8, ), NAN, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    m = buf[1 if off else 0:][:N * ld].view(N, ld)
    m[:, :C] = host.to(DEV)
    assert m.data_ptr() % 16 == (4 if off else 0)
    return m


def _guards_untouched(m, C, what):
    if m.shape[1] > C:
        assert bool(torch.isnan(m[:, C:]).all()), f"{what}: guard columns were written"


def _vecs(ins):
    return {k: ins[k].to(DEV).contiguous() for k in ("gamma", "beta", "alpha")}


def _words(seed=1234, step=3):
    return torch.tensor([seed, step], dtype=torch.int64, device=DEV)


def _keep(words, p, N, C):
    out = torch.full((N, C), NAN, dtype=torch.float32, device=DEV)
    _ok(_lib().glass_dropout_scales_f32(words.data_ptr(), CALL_ID, p, N, C, out.data_ptr(), _stream()))
    k = out.cpu()
    inv = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))
    assert bool(((k == 0) | (k == inv)).all()) and abs(float((k == 0).float().mean()) - p) < 0.05
    return k


def _ws(C):
    nbytes = int(_lib().glass_graphnorm_ws_bytes(1, C))
    assert nbytes == G.MAX_STAT_BLOCKS * 2 * C * 8 + 16 * C
    return torch.full((nbytes // 8 + 1, ), NAN, dtype=torch.float64, device=DEV)


def _carve(ws, C):
    part = ws[:G.MAX_STAT_BLOCKS * 2 * C].cpu().view(G.MAX_STAT_BLOCKS, 2, C)
    coef = ws[G.MAX_STAT_BLOCKS * 2 * C:].view(torch.float32)[:3 * C].cpu().view(3, C)
    return part, coef


def _rows_written(part, nblk, what):
    """the direct observation of the statistics grid: rows below nblk written, rows at or above it still NaN"""
    assert not bool(torch.isnan(part[:nblk]).any()), f"{what}: a partial row below nblk = {nblk} was not written"
    assert bool(torch.isnan(part[nblk:]).all()), f"{what}: a partial row at or above nblk = {nblk} was written"


def _note(stage, res, what):
    print(f"graphnorm {what}: " + " ".join(f"{k} {v[1]:.3f}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not v[0]}
    assert not bad, f"{what}: {bad}"
    w = _WORST.setdefault(stage, {})
    for k, v in res.items():
        w[k] = max(w.get(k, 0.0), v[1])


def _recipe(N, C, seed, kind):
    key = (N, C, seed, kind)
    if key not in _CACHE:
        _CACHE[key] = G.recipe(N, C, seed, kind)
    return _CACHE[key]


def _saved32(ins):
    return G.stage_saved(ins["x"], ins["gamma"], ins["beta"], ins["alpha"], ins["eps"])[0].float()


def _e2e(got, want, keys, what):
    ok_cols = ~want["kinks"].any(0)
    assert float(want["kinks"].double().mean()) <= G.KINK_CAP
    for k in keys:
        e = G.rel_inf(got[k][..., ok_cols], want[k][..., ok_cols])
        assert e <= G.TOL, f"{what}: end to end {k} {e:.2e}"


# ---- forward -------------------------------------------------------------------------------------------------------------------------
def _forward(ins, act, ldx, ldy, offx=False, offy=False, p=0.0, split=False, words=None):
    """glass_graphnorm_fwd_f32, or (split) glass_graphnorm_stats_f32 + glass_graphnorm_apply_f32 -> dict on the CPU"""
    lib, (N, C) = _lib(), ins["x"].shape
    x, y, v = _mat(ins["x"], ldx, offx), _mat(torch.full((N, C), NAN), ldy, offy), _vecs(ins)
    saved, ws = torch.full((4 * C, ), NAN, dtype=torch.float32, device=DEV), _ws(C)
    words = _words() if words is None else words
    keep = _keep(words, p, N, C) if p > 0 else None
    rng = words.data_ptr() if p > 0 else None
    if split:
        _ok(lib.glass_graphnorm_stats_f32(x.data_ptr(), ldx, N, C, v["gamma"].data_ptr(), v["beta"].data_ptr(), v["alpha"].data_ptr(), ins["eps"],
                                          saved.data_ptr(), ws.data_ptr(), _stream()))
        _ok(lib.glass_graphnorm_apply_f32(x.data_ptr(), ldx, y.data_ptr(), ldy, N, C, saved.data_ptr(), act, p, rng, CALL_ID, _stream()))
    else:
        _ok(lib.glass_graphnorm_fwd_f32(x.data_ptr(), ldx, y.data_ptr(), ldy, N, C, v["gamma"].data_ptr(), v["beta"].data_ptr(), v["alpha"].data_ptr(),
                                        ins["eps"], saved.data_ptr(), act, p, rng, CALL_ID, ws.data_ptr(), _stream()))
    torch.cuda.synchronize()
    _guards_untouched(y, C, "y")
    _guards_untouched(x, C, "x")
    assert torch.equal(x[:, :C].cpu().view(torch.int32), ins["x"].view(torch.int32))
    part, _ = _carve(ws, C)
    vec_stats = G.vec_in(C, ldx, x.data_ptr()) if split else G.vec_fwd(C, ldx, ldy, x.data_ptr(), y.data_ptr())
    return dict(part=part, saved=saved.cpu().view(4, C), y=y[:, :C].cpu(), keep=keep, vec_stats=vec_stats,
                vec_apply=G.vec_fwd(C, ldx, ldy, x.data_ptr(), y.data_ptr()), nblk=G.stat_blocks(N, C, vec_stats))


def _grade_forward(got, ins, act, what, e2e=True):
    x = ins["x"]
    _rows_written(got["part"], got["nblk"], what)
    res = dict(sums=G.gate(got["part"][:got["nblk"]].sum(0), *G.stage_sums(x)),
               saved=G.gate(got["saved"], *G.stage_saved(x, ins["gamma"], ins["beta"], ins["alpha"], ins["eps"])),
               y=G.gate(got["y"], *G.stage_apply(x, got["saved"], act, got["keep"])))
    _note("forward", res, what)
    if e2e:
        _e2e(got, G.chain(ins, act, got["keep"]), ("y", ), what)


# (C, ldx, ldy, x off, y off, vector form expected)
FWD_FORMS = [(17, 20, 20, False, False, False), (1, 4, 4, False, False, False), (3, 4, 8, False, False, False),
             (64, 65, 68, False, False, False), (64, 68, 65, False, False, False), (64, 68, 68, True, False, False), (64, 68, 68, False, True, False),
             (4, 8, 8, False, False, True), (20, 24, 24, False, False, True), (64, 68, 72, False, False, True), (1024, 1028, 1028, False, False, True),
             (1028, 1032, 1032, False, False, True), (256, 257, 257, False, False, False), (257, 260, 260, False, False, False),
             (300, 301, 304, False, False, False)]


@pytest.mark.parametrize("C,ldx,ldy,offx,offy,vec", FWD_FORMS, ids=[f"C{c}_ldx{a}_ldy{b}" + ("_xoff" if o else "") + ("_yoff" if q else "")
                                                                     for c, a, b, o, q, _ in FWD_FORMS])
def test_forward_vector_and_scalar_forms_and_tilings(C, ldx, ldy, offx, offy, vec):
    ins = _recipe(300, C, 100 + C, "plain")
    got = _forward(ins, G.ACT_ELU, ldx, ldy, offx, offy)
    assert got["vec_stats"] == vec == got["vec_apply"] and got["nblk"] == G.stat_blocks(300, C, vec)
    _grade_forward(got, ins, G.ACT_ELU, f"fwd C{C} ldx{ldx} ldy{ldy} off{int(offx)}{int(offy)}")
    if offy or ldy % 4:  # the input-only entry ignores y: vector statistics (fewer partial rows), scalar apply
        sp = _forward(ins, G.ACT_ELU, ldx, ldy, offx, offy, split=True)
        assert sp["vec_stats"] == G.vec_in(C, ldx, 4 if offx else 0) and not sp["vec_apply"]
        if sp["vec_stats"]:
            assert sp["nblk"] < got["nblk"]
        _grade_forward(sp, ins, G.ACT_ELU, f"stats+apply C{C} ldx{ldx} ldy{ldy}")


ROWS = [(64, 1), (64, 3), (64, 63), (64, 64), (64, 65), (20, 127), (20, 128), (20, 129), (64, 129), (17, 33)]
CAPS = [(1024, 8192), (1024, 8200), (1024, 16384), (1024, 16392)]


@pytest.mark.parametrize("C,N", ROWS + CAPS, ids=[f"C{c}_N{n}" for c, n in ROWS + CAPS])
def test_forward_row_edges_and_grid_caps(C, N):
    """rpb * 4 - 1, rpb * 4, rpb * 4 + 1 (one trip against two of the unrolled loop); at C = 1024 (rpb 1) the statistics grid at
    its cap of 1024 (N = 8192) and beyond (8200: a second trip), the apply grid at its cap of 4096 (16384) and beyond (16392)"""
    vec = C % 4 == 0
    ins = _recipe(N, C, 200 + N % 97, "plain")
    if (C, N) in CAPS:
        assert G.stat_blocks(N, C, True) == 1024 and (G.apply_blocks(N, C, True) == 4096) == (N >= 16384)
        assert G.stat_blocks(8184, C, True) == 1023 and G.apply_blocks(16380, C, True) == 4095
    got = _forward(ins, G.ACT_NONE if N > 1000 else G.ACT_ELU, C + (4 if vec else 3), C + (4 if vec else 3), split=N == 16392)
    assert got["vec_stats"] == vec
    _grade_forward(got, ins, G.ACT_NONE if N > 1000 else G.ACT_ELU, f"fwd rows C{C} N{N}", e2e=N > 1)


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("act", ACTS)
def test_forward_activations_and_recipes(act, kind):
    ins = _recipe(300, 64, 300, kind)
    _grade_forward(_forward(ins, act, 68, 68), ins, act, f"fwd act{act} {kind}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("p", [0.5, 0.9])
def test_forward_dropout_with_the_very_masks(p, act):
    """keep-scales from glass_dropout_scales_f32 under the same (seed, step, call_id): y is the oracle's y with those masks per
    element; the vector and the scalar form of one tensor draw the same mask and give the same bits"""
    ins = _recipe(300, 64, 301, "plain")
    vecf, scal = _forward(ins, act, 68, 68, p=p), _forward(ins, act, 65, 68, p=p)
    assert vecf["vec_apply"] and not scal["vec_apply"] and torch.equal(vecf["keep"], scal["keep"])
    for got, name in ((vecf, "vector"), (scal, "scalar")):
        _grade_forward(got, ins, act, f"fwd dropout p{p} act{act} {name}")
        assert bool((got["y"][got["keep"] == 0] == 0).all())
    assert torch.equal(vecf["y"].view(torch.int32), scal["y"].view(torch.int32))
    other = _forward(ins, act, 68, 68, p=p, words=_words(step=4))
    assert not torch.equal(other["keep"], vecf["keep"])


@pytest.mark.parametrize("act", ACTS)
def test_nonfinite_column_stays_visible(act):
    """one NaN and one +Inf in one column: saved and y of that column are NaN wherever torch's are (everywhere), under every
    activation — ReLU included, whose `h > 0 ? h : 0` wrote a column of clean zeros on the parent commit — and every other
    column keeps the bits of the clean run"""
    ins = dict(_recipe(300, 64, 302, "plain"))
    clean = _forward(ins, act, 68, 68)
    x = ins["x"].clone()
    x[5, 3], x[9, 3] = NAN, float("inf")
    ins["x"] = x
    ref = torch.nn.functional.elu if act == G.ACT_ELU else torch.relu if act == G.ACT_RELU else (lambda t: t)
    mu = x.mean(0)
    cen = x - ins["alpha"] * mu
    want_nan = torch.isnan(ref(ins["gamma"] * cen / (cen.pow(2).mean(0) + ins["eps"]).sqrt() + ins["beta"]))
    assert bool(want_nan[:, 3].all()) and int(want_nan.sum()) == 300
    for split in (False, True):
        got = _forward(ins, act, 68, 68, split=split)
        assert bool(torch.isnan(got["saved"][:, 3]).all()) and int(torch.isnan(got["saved"]).sum()) == 4
        n_nan = int(torch.isnan(got["y"][:, 3]).sum())
        assert torch.equal(torch.isnan(got["y"]), want_nan), f"act {act}: {n_nan} of 300 rows of the NaN column are NaN, {int((got['y'][:, 3] == 0).sum())} are 0"
        keep = torch.ones(64, dtype=torch.bool)
        keep[3] = False
        assert torch.equal(got["y"][:, keep].view(torch.int32), clean["y"][:, keep].view(torch.int32))
        assert torch.equal(got["saved"][:, keep].view(torch.int32), clean["saved"][:, keep].view(torch.int32))
        ok, share, at = G.gate_with_nan(got["y"], *G.stage_apply(x, got["saved"], act))
        assert ok, (share, at)


# ---- finalize ------------------------------------------------------------------------------------------------------------------------
FIN = [(1, 1, 20), (63, 1, 20), (64, 1, 20), (65, 1, 20), (512, 1, 20), (513, 1, 20), (1024, 1, 20), (65, 2, 8), (65, 8, 4), (65, 3, 6), (513, 3, 6),
       (5, 1, 17)]


@pytest.mark.parametrize("nblk,n_src,C_each", FIN, ids=[f"nblk{b}_src{s}_C{c}" for b, s, c in FIN])
def test_finalize_from_hand_written_partials(nblk, n_src, C_each):
    """glass_graphnorm_finalize_f32 over partial buffers written by the test (8 rows of x per partial row): every slot-walk
    length, several sources, a four-column workgroup straddling two sources (C_each = 6), C off 4; partial rows at nblk and
    beyond hold NaN and must not be read"""
    import numpy as np
    lib, C, N = _lib(), n_src * C_each, nblk * 8
    ins = _recipe(N, C, 400 + nblk, "plain")
    x = ins["x"].double()
    rows = torch.stack([x.reshape(nblk, 8, C).sum(1), (x * x).reshape(nblk, 8, C).sum(1)], 1)   # [nblk, 2, C]
    bufs = []
    for k in range(n_src):
        b = torch.full((nblk + 4, 2, C_each), NAN, dtype=torch.float64)
        b[:nblk] = rows[:, :, k * C_each:(k + 1) * C_each]
        bufs.append(b.to(DEV).contiguous())
    ptrs = np.array([b.data_ptr() for b in bufs], dtype=np.uint64)
    v, saved = _vecs(ins), torch.full((4 * C, ), NAN, dtype=torch.float32, device=DEV)
    _ok(lib.glass_graphnorm_finalize_f32(ptrs.ctypes.data, n_src, nblk, C_each, N, v["gamma"].data_ptr(), v["beta"].data_ptr(), v["alpha"].data_ptr(),
                                         ins["eps"], saved.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert G.fin_slots_read(nblk) == list(range(nblk))
    res = dict(saved=G.gate(saved.cpu().view(4, C), *G.stage_saved(ins["x"], ins["gamma"], ins["beta"], ins["alpha"], ins["eps"])))
    _note("finalize", res, f"finalize nblk{nblk} src{n_src} C_each{C_each}")


# ---- exact statistics ----------------------------------------------------------------------------------------------------------------
def _stats_exact(x_host, ldx, n_rep, off=False):
    lib, (N, C) = _lib(), x_host.shape
    x = _mat(x_host, ldx, off)
    acc = torch.zeros(int(lib.glass_gn_exact_words(C)), dtype=torch.int64, device=DEV)
    assert acc.numel() == G.acc_words(C)
    _ok(lib.glass_graphnorm_stats_exact_f32(x.data_ptr(), ldx, N, C, acc.data_ptr(), n_rep, _stream()))
    torch.cuda.synchronize()
    return acc.cpu(), G.exact_stats_form(N, C, G.vec_in(C, ldx, x.data_ptr()))


def _grade_exact(words, x, C, n_rep, form, what, ins=None):
    N = x.shape[0]
    grid = form[2] if form[0] == "stats64" else form[2][0]
    w = words.view(G.ACC_REP, 2, C, 2)
    assert not bool(w[n_rep:].any()), f"{what}: a replica at or above n_rep = {n_rep} was written"
    used = [bool(w[r, 1, :, :].any()) for r in range(n_rep)]     # sum x^2 > 0 in every column: a replica that received an add shows it
    assert used == [r < grid for r in range(n_rep)], f"{what}: workgroup b must add to replica b % n_rep ({used}, grid {grid})"
    dec = G.acc_decode(words, C, n_rep, G.SCALE_FWD)
    want, bound = G.exact_sum_bound(x, C, form, adds=grid)
    err = (dec["value"] - want).abs()
    share = float((err / bound).max())
    print(f"graphnorm {what}: form {form} decoded sums {share:.3f} of the derived bound")
    assert bool((err <= bound).all()), (what, share)
    _WORST.setdefault("exact_stats", {})["bound"] = max(_WORST.get("exact_stats", {}).get("bound", 0.0), share)
    if ins is not None:
        sv = G.saved_from_sums(dec["value"][0], dec["value"][1], N, ins["gamma"], ins["beta"], ins["alpha"], ins["eps"])
        _note("exact_stats", dict(saved=G.gate(sv.float(), *G.stage_saved(x, ins["gamma"], ins["beta"], ins["alpha"], ins["eps"]))), what)


EXACT64 = [(1, 16), (15, 16), (16, 2), (17, 1), (17, 2), (17, 3), (300, 3), (4096, 16), (4097, 16), (5119, 16), (5120, 2), (20480, 16), (20481, 16), (40961, 3)]


@pytest.mark.parametrize("N,n_rep", EXACT64, ids=[f"N{n}_rep{r}" for n, r in EXACT64])
def test_exact_statistics_c64_every_row_tile(N, n_rep):
    """gn_stats64_exact_kernel: nst 1 -> 2 (4096 / 4097), -> 5 (5119 / 5120), a second round of five (20480 / 20481), a third
    (40961); the limbs read back and decoded in integers; twice -> the same words"""
    ins = _recipe(N, 64, 500, "plain")
    words, form = _stats_exact(ins["x"], 68, n_rep)
    assert form[0] == "stats64"
    _grade_exact(words, ins["x"], 64, n_rep, form, f"stats64 N{N} rep{n_rep}", ins)
    again, _ = _stats_exact(ins["x"], 68, n_rep)
    assert torch.equal(words, again)


GENERIC = [(64, 65, False, 4), (64, 68, True, 4), (16, 16, False, 2), (32, 36, False, 16), (128, 128, False, 1), (128, 132, False, 16), (20, 24, False, 3),
           (17, 20, False, 2)]


@pytest.mark.parametrize("C,ldx,off,n_rep", GENERIC, ids=[f"C{c}_ldx{l}" + ("_off" if o else "") + f"_rep{r}" for c, l, o, r in GENERIC])
def test_exact_statistics_generic_kernel(C, ldx, off, n_rep):
    """every other width, and C = 64 with an odd stride or an offset pointer: gn_stats_kernel with exact = n_rep"""
    ins = _recipe(300, C, 501, "mixed")
    words, form = _stats_exact(ins["x"], ldx, n_rep, off)
    assert form[0] == "generic" and form[1] == (4 if C % 4 == 0 and ldx % 4 == 0 and not off else 1)
    _grade_exact(words, ins["x"], C, n_rep, form, f"exact generic C{C} ldx{ldx} off{int(off)} rep{n_rep}", ins)
    again, _ = _stats_exact(ins["x"], ldx, n_rep, off)
    assert torch.equal(words, again)


@pytest.mark.parametrize("C,ldx", [(64, 64), (64, 65), (128, 128)])
def test_exact_statistics_poison_exactly_its_quantity(C, ldx):
    """a NaN (column 3), an Inf (column 7) and a partial beyond 4.0e18 / scale (column 11: x = 4e7, x^2 = 1.6e15 > 9.8e14 while
    the sum of x stays in range) poison exactly (sum, sum of squares) of 3 and 7 and the sum of squares of 11"""
    ins = _recipe(40, C, 502, "plain")
    x = ins["x"].clone()
    x[5, 3], x[9, 7], x[20, 11] = NAN, float("inf"), 4.0e7
    assert 1.6e15 * G.SCALE_FWD > G.ACC_BOUND > 4.0e7 * 40 * G.SCALE_FWD
    words, form = _stats_exact(x, ldx, 4)
    dec = G.acc_decode(words, C, 4, G.SCALE_FWD)
    want_bad = [[c in (3, 7) for c in range(C)], [c in (3, 7, 11) for c in range(C)]]
    assert dec["bad"] == want_bad and torch.equal(torch.isnan(dec["value"]), torch.tensor(want_bad))
    fine = torch.tensor([c not in (3, 7, 11) for c in range(C)])
    want, bound = G.exact_sum_bound(ins["x"][:, fine], C, form, adds=4)
    assert bool(((dec["value"][:, fine] - want).abs() <= bound).all())


# ---- backward ------------------------------------------------------------------------------------------------------------------------
def _backward(ins, act, lds=None, off=(), add="none", accumulate=0, prev=None, null=(), p=0.0, partial=None, nblk=None, acc=None, n_rep=0):
    """glass_graphnorm_bwd_f32 (partial None), or glass_graphnorm_bwd_from_stats_f32 with hand-written partial rows (nblk > 0)
    or accumulator words (acc, n_rep).  lds = (lddy, ldx, lddx, ldadd); off: names of operands one float past 16 bytes;
    add: none | aligned | odd (ldadd odd).  -> dict on the CPU"""
    lib, (N, C) = _lib(), ins["x"].shape
    lddy, ldx, lddx, ldadd = lds or (C + 4, C + 8, C + 4, C + 4)
    if add == "odd":
        ldadd = C + 1
    dy, x = _mat(ins["dy"], lddy, "dy" in off), _mat(ins["x"], ldx, "x" in off)
    dx = _mat(torch.full((N, C), NAN), lddx, "dx" in off)
    ad = _mat(ins["addend"], ldadd, "addend" in off) if add != "none" else None
    v, saved = _vecs(ins), _saved32(ins)
    saved_d = saved.reshape(-1).to(DEV).contiguous()
    words = _words()
    keep = _keep(words, p, N, C) if p > 0 else None
    grads = {}
    for i, k in enumerate(("dgamma", "dbeta", "dalpha")):
        if k not in null:
            grads[k] = prev[i].to(DEV).contiguous().clone() if prev is not None else torch.full((C, ), NAN, dtype=torch.float32, device=DEV)
    gp = [grads[k].data_ptr() if k in grads else None for k in ("dgamma", "dbeta", "dalpha")]
    ws = _ws(C)
    tail = (accumulate, act, p, words.data_ptr() if p > 0 else None, CALL_ID, ws.data_ptr(), _stream())
    head = (dy.data_ptr(), lddy, x.data_ptr(), ldx, dx.data_ptr(), lddx, ad.data_ptr() if ad is not None else None, ldadd if ad is not None else 0, N, C,
            v["gamma"].data_ptr(), v["alpha"].data_ptr(), saved_d.data_ptr())
    if acc is not None:
        acc_d = acc.to(DEV).contiguous()
        before = acc_d.clone()
        _ok(lib.glass_graphnorm_bwd_from_stats_f32(*head, acc_d.data_ptr(), -n_rep, *gp, *tail))
    elif partial is not None:
        part_d = partial.to(DEV).contiguous()
        _ok(lib.glass_graphnorm_bwd_from_stats_f32(*head, part_d.data_ptr(), nblk, *gp, *tail))
    else:
        _ok(lib.glass_graphnorm_bwd_f32(*head, *gp, *tail))
    torch.cuda.synchronize()
    if acc is not None:
        assert torch.equal(acc_d, before), "the consumer wrote to the accumulators"
    for m, name in ((dx, "dx"), (dy, "dy"), (x, "x")) + (((ad, "addend"), ) if ad is not None else ()):
        _guards_untouched(m, C, name)
    part, coef = _carve(ws, C)
    vec = G.vec_bwd(C, lddy, ldx, lddx, ldadd if ad is not None else None, dy.data_ptr(), x.data_ptr(), dx.data_ptr(), ad.data_ptr() if ad is not None else 0)
    out = dict(part=part, coef=coef, dx=dx[:, :C].cpu(), keep=keep, saved=saved, vec=vec, nblk=G.stat_blocks(N, C, vec),
               addend=ins["addend"] if ad is not None else None, coef_untouched=bool(torch.isnan(ws[G.MAX_STAT_BLOCKS * 2 * C:]).all()))
    out.update({k: t.cpu() for k, t in grads.items()})
    return out


def _grade_backward(got, ins, act, what, prev=None, part=None, stage="backward", e2e=True):
    """part: the partial rows the call was GIVEN (from_stats), else the rows it wrote (bwd_f32: gated, and rows >= nblk NaN)"""
    x, dy, sv, N = ins["x"], ins["dy"], got["saved"], ins["x"].shape[0]
    res = {}
    if part is None:
        _rows_written(got["part"], got["nblk"], what)
        part = got["part"][:got["nblk"]]
        res["bsums"] = G.gate(part.sum(0), *G.stage_bwd_sums(dy, x, sv, ins["alpha"], act, got["keep"]))
    else:
        assert bool(torch.isnan(got["part"]).all()), f"{what}: the statistics rows of the workspace were written"
    Gn = G.stage_gn_bwd(part, part.abs(), N, ins["gamma"], ins["alpha"], sv, prev)
    res["coef"] = G.gate(got["coef"], *Gn["coef"])
    for k in ("dgamma", "dbeta", "dalpha"):
        if k in got:
            res[k] = G.gate(got[k], *Gn[k])
    res["dx"] = G.gate(got["dx"], *G.stage_dx(dy, x, sv, got["coef"], got["addend"], act, got["keep"]))
    _note(stage, res, what)
    if e2e:
        want = G.chain(ins, act, got["keep"], addend=got["addend"], prev=prev)
        _e2e(got, want, [k for k in ("dx", "dgamma", "dbeta", "dalpha") if k in got], what)


BWD_FORMS = [(17, (20, 20, 20, 20), (), False), (1, (4, 4, 4, 4), (), False), (3, (4, 8, 4, 4), (), False), (64, (65, 68, 68, 68), (), False),
             (64, (68, 65, 68, 68), (), False), (64, (68, 68, 65, 68), (), False), (64, (68, 68, 68, 68), ("dy", ), False),
             (64, (68, 68, 68, 68), ("x", ), False), (64, (68, 68, 68, 68), ("dx", ), False), (4, (8, 8, 8, 8), (), True), (20, (24, 24, 24, 24), (), True),
             (64, (68, 72, 68, 68), (), True), (1024, (1028, 1028, 1028, 1028), (), True), (1028, (1032, 1032, 1032, 1032), (), True),
             (256, (257, 257, 257, 257), (), False), (257, (260, 260, 260, 260), (), False), (300, (301, 304, 301, 304), (), False)]


@pytest.mark.parametrize("C,lds,off,vec", BWD_FORMS, ids=[f"C{c}_" + "_".join(map(str, l)) + "".join("_" + o for o in f) for c, l, f, _ in BWD_FORMS])
def test_backward_vector_and_scalar_forms_and_tilings(C, lds, off, vec):
    ins = _recipe(300, C, 100 + C, "plain")
    got = _backward(ins, G.ACT_ELU, lds, off)
    assert got["vec"] == vec
    _grade_backward(got, ins, G.ACT_ELU, f"bwd C{C} lds{lds} off{off}")


@pytest.mark.parametrize("C,N", ROWS + [(1024, 8200), (1024, 16392)], ids=[f"C{c}_N{n}" for c, n in ROWS + [(1024, 8200), (1024, 16392)]])
def test_backward_row_edges_and_grid_caps(C, N):
    ins = _recipe(N, C, 200 + N % 97, "plain")
    act = G.ACT_NONE if N > 1000 else G.ACT_ELU
    got = _backward(ins, act)
    assert got["vec"] == (C % 4 == 0)
    _grade_backward(got, ins, act, f"bwd rows C{C} N{N}", e2e=N > 1)


@pytest.mark.parametrize("add,vec", [("none", True), ("aligned", True), ("odd", False), ("offset", False)])
def test_backward_addend(add, vec):
    """absent; present and aligned; present with ldadd odd or its pointer off 16 bytes, either of which forces the scalar form
    (seen in the statistics grid: 10 partial rows instead of 3 at N = 300, C = 64)"""
    ins = _recipe(300, 64, 303, "mixed")
    got = _backward(ins, G.ACT_ELU, add="aligned" if add == "offset" else add, off=("addend", ) if add == "offset" else ())
    assert got["vec"] == vec and got["nblk"] == (3 if vec else 10)
    _grade_backward(got, ins, G.ACT_ELU, f"bwd addend {add}")


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("act", ACTS)
def test_backward_activations_and_recipes(act, kind):
    ins = _recipe(300, 64, 300, kind)
    _grade_backward(_backward(ins, act, add="aligned"), ins, act, f"bwd act{act} {kind}")


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("p", [0.5, 0.9])
def test_backward_dropout_with_the_forward_masks(p, act):
    ins = _recipe(300, 64, 301, "plain")
    fwd = _forward(ins, act, 68, 68, p=p)
    for lds in (None, (65, 68, 68, 68)):
        got = _backward(ins, act, lds, p=p)
        assert torch.equal(got["keep"], fwd["keep"]) and got["vec"] == (lds is None)
        _grade_backward(got, ins, act, f"bwd dropout p{p} act{act} vec{int(got['vec'])}")


@pytest.mark.parametrize("null", [(), ("dgamma", ), ("dbeta", ), ("dalpha", ), ("dgamma", "dbeta", "dalpha")], ids=lambda n: "null_" + "_".join(n) if n else "all")
@pytest.mark.parametrize("accumulate", [0, 1])
def test_backward_accumulate_and_null_parameter_gradients(accumulate, null):
    """accumulate = 1 adds to the previous contents, 0 overwrites them; each of the three gradients may be null"""
    ins = _recipe(300, 64, 304, "plain")
    g = torch.Generator().manual_seed(305)
    prev = tuple(torch.randn(64, generator=g) for _ in range(3))
    got = _backward(ins, G.ACT_RELU, accumulate=accumulate, prev=prev, null=null)
    assert all(k not in got for k in null)
    _grade_backward(got, ins, G.ACT_RELU, f"bwd accumulate{accumulate} null{null}", prev=prev if accumulate else None)


def _hand_partials(S, nblk, seed, pad=4):
    """nblk fp64 rows that add up to S [2, C] (noise rows of zero sum on top of S / nblk), then `pad` rows of NaN"""
    g = torch.Generator().manual_seed(seed)
    noise = torch.randn(nblk, *S.shape, generator=g, dtype=torch.float64) * (S.abs() + S.abs().mean())
    rows = S / nblk + noise - noise.mean(0)
    return torch.cat([rows, torch.full((pad, ) + S.shape, NAN, dtype=torch.float64)])


@pytest.mark.parametrize("C,lds", [(64, None), (20, None), (17, (20, 20, 20, 20))])
@pytest.mark.parametrize("nblk", [1, 65, 513])
def test_backward_from_hand_written_partials(nblk, C, lds):
    """glass_graphnorm_bwd_from_stats_f32, nblk > 0: the finalize over rows the test wrote (NaN rows behind them), then the apply"""
    ins = _recipe(300, C, 306, "mixed")
    S, _ = G.stage_bwd_sums(ins["dy"], ins["x"], _saved32(ins), ins["alpha"], G.ACT_ELU)
    rows = _hand_partials(S, nblk, 307)
    got = _backward(ins, G.ACT_ELU, lds, add="aligned", partial=rows, nblk=nblk)
    _grade_backward(got, ins, G.ACT_ELU, f"bwd from partials nblk{nblk} C{C}", part=rows[:nblk], stage="from_partials")


# ---- the exact backward: accumulators written by the test --------------------------------------------------------------------------------
PATTERNS = ("replica0", "round_robin", "negative_hi", "lo_past_2_40")


def _hand_acc(S, C, n_rep, pattern, seed, poison=()):
    """accumulator words [kAccRep, 2, C, 2] holding adds that sum to S (up to the encoding's truncation), spread by `pattern`;
    replicas at n_rep and beyond hold garbage WITH the poison bit; poison: (rep, which, c) inside the first n_rep.
    -> (words, decoded value [2, C] by the integer restatement, mass = sum |add|)"""
    g = torch.Generator().manual_seed(seed)
    K = {"replica0": 7, "round_robin": 37, "negative_hi": 8, "lo_past_2_40": 64}[pattern]
    noise = torch.randn(K, 2, C, generator=g, dtype=torch.float64) * (S.abs() + S.abs().mean())
    adds = S / K + noise - noise.mean(0)
    if pattern == "negative_hi":      # large adds of either sign that cancel: negative hi limbs next to lo limbs in [0, 2^40)
        adds[0] -= 1000.3
        adds[1] += 1000.3
    if pattern == "lo_past_2_40":     # every add just below a multiple of the hi unit: lo near 2^40 each, 64 of them in one replica
        unit = 1.0 / G.SCALE_BWD
        adds = torch.floor(adds / unit) * unit + unit * (1 - 2.0**-20)
    hi, lo, bad = G.acc_encode_tensor(adds, G.SCALE_BWD)
    assert not bool(bad.any())
    rep = [0 if pattern in ("replica0", "lo_past_2_40") else k % n_rep for k in range(K)]
    w = torch.zeros(G.ACC_REP, 2, C, 2, dtype=torch.int64)
    for k in range(K):
        w[rep[k], :, :, 0] += hi[k]
        w[rep[k], :, :, 1] += lo[k]
    if pattern == "negative_hi":
        assert bool((w[:n_rep, :, :, 0] < 0).any()) and bool((w[:n_rep, :, :, 1] >= 0).all())
    if pattern == "lo_past_2_40":
        assert bool((w[0, :, :, 1] > (1 << 40)).all())
    if n_rep < G.ACC_REP:
        w[n_rep:] = torch.randint(-(1 << 62), 1 << 62, w[n_rep:].shape, generator=g, dtype=torch.int64)
        w[n_rep:, :, ::2, 1] |= -(1 << 63)
    for r, which, c in poison:
        w[r, which, c, 1] |= -(1 << 63)
    dec = G.acc_decode(w.reshape(-1), C, n_rep, G.SCALE_BWD)
    return w.reshape(-1), dec["value"], adds.abs().sum(0)


def _grade_exact_backward(got, ins, act, S, M, what, prev=None, nan_ok=False):
    """coef is not written by the one-launch form: dx is gated with the fp64 coefficients of the decoded sums and their mass"""
    x, dy, sv, N = ins["x"], ins["dy"], got["saved"], ins["x"].shape[0]
    assert bool(torch.isnan(got["part"]).all()) and got["coef_untouched"], f"{what}: the one-launch form wrote to the workspace"
    Gn = G.stage_gn_bwd(*G.sums_as_partial(S, M), N, ins["gamma"], ins["alpha"], sv, prev)
    gate = G.gate_with_nan if nan_ok else G.gate
    res = {k: gate(got[k], *Gn[k]) for k in ("dgamma", "dbeta", "dalpha") if k in got}
    res["dx"] = gate(got["dx"], *G.stage_dx(dy, x, sv, Gn["coef"][0], got["addend"], act, got["keep"], coef_m=Gn["coef"][1]))
    _note("exact_backward", res, what)


EXACT_BWD = [(64, 2, 80), (64, 2, 81), (64, 4, 79), (64, 16, 161), (64, 4, 1), (64, 1, 161), (64, 1, 64), (16, 2, 255), (16, 1, 257), (32, 4, 128),
             (32, 16, 129), (128, 16, 33), (128, 2, 31), (128, 1, 32)]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("C,n_rep,N", EXACT_BWD, ids=[f"C{c}_rep{r}_N{n}" for c, r, n in EXACT_BWD])
def test_exact_backward_from_hand_written_accumulators(C, n_rep, N, pattern):
    """glass_graphnorm_bwd_from_stats_f32, nblk = -n_rep: C = 64 with two or more replicas takes the 80-row kernel (N = 79, 80,
    81, 161: one, one, two, three workgroups), C = 64 with one replica and every other width the LDS fold (its own rpb * 4
    edges); garbage with the poison bit in the replicas at n_rep and beyond must not be read; accumulate = 1 over previous
    contents: the parameter gradients are written once, by workgroup 0, whatever the grid"""
    form = G.bwd_exact_form(C, n_rep, N)
    assert form[0] == ("acc64x5" if C == 64 and n_rep >= 2 else "acc_lds")
    ins = _recipe(N, C, 600 + C, "tiny_grad" if pattern == "round_robin" else "plain")
    act = G.ACT_ELU
    want_S, _ = G.stage_bwd_sums(ins["dy"], ins["x"], _saved32(ins), ins["alpha"], act)
    words, S, M = _hand_acc(want_S, C, n_rep, pattern, 601)
    g = torch.Generator().manual_seed(602)
    prev = tuple(torch.randn(C, generator=g) * (1e-12 if ins["kind"] == "tiny_grad" else 1.0) for _ in range(3))
    got = _backward(ins, act, (C, C + 4, C + 8, C), add="aligned", accumulate=1, prev=prev, acc=words, n_rep=n_rep)
    assert got["vec"]
    _grade_exact_backward(got, ins, act, S, M, f"exact bwd C{C} rep{n_rep} N{N} {pattern} {form}", prev=prev)
    if pattern != "lo_past_2_40" and N > 1:   # (that pattern moves every add by up to 2^-24: its sums are not the true sums)
        _e2e(got, G.chain(ins, act, None, addend=ins["addend"], prev=prev), ("dx", "dgamma", "dbeta", "dalpha"), "exact bwd")


@pytest.mark.parametrize("C,n_rep,N", [(64, 4, 161), (64, 1, 161), (128, 2, 33)])
def test_exact_backward_poison_inside_the_folded_replicas(C, n_rep, N):
    """the poison bit on the S2 limb of column 5 (last folded replica) and the S1 limb of column 9 (replica 0): exactly what
    depends on them is NaN — columns 5 and 9 of dx, dgamma / dalpha of 5, dbeta / dalpha of 9 — and nothing else"""
    ins = _recipe(N, C, 610, "plain")
    want_S, _ = G.stage_bwd_sums(ins["dy"], ins["x"], _saved32(ins), ins["alpha"], G.ACT_RELU)
    words, S, M = _hand_acc(want_S, C, n_rep, "round_robin", 611, poison=((n_rep - 1, 1, 5), (0, 0, 9)))
    assert bool(torch.isnan(S[1, 5])) and bool(torch.isnan(S[0, 9])) and int(torch.isnan(S).sum()) == 2
    got = _backward(ins, G.ACT_RELU, (C, C, C, C), acc=words, n_rep=n_rep)
    _grade_exact_backward(got, ins, G.ACT_RELU, S, M, f"exact bwd poison C{C} rep{n_rep}", nan_ok=True)
    cols = torch.isnan(got["dx"]).any(0).nonzero().flatten().tolist()
    assert cols == [5, 9] and bool(torch.isnan(got["dx"][:, [5, 9]]).all())
    assert [torch.isnan(got[k]).nonzero().flatten().tolist() for k in ("dgamma", "dbeta", "dalpha")] == [[5], [9], [5, 9]]


@pytest.mark.parametrize("C,n_rep", [(64, 4), (64, 1), (32, 2), (128, 16)])
def test_exact_form_agrees_with_the_partials_form(C, n_rep):
    """the same sums through the one-launch exact form and (as one partial row holding the decoded doubles) through finalize +
    apply: the parameter gradients within the two forms' bars; where they — and with them the coefficients — are bit-equal,
    dx is bit-equal too"""
    N, act = 300, G.ACT_ELU
    ins = _recipe(N, C, 620, "plain")
    want_S, _ = G.stage_bwd_sums(ins["dy"], ins["x"], _saved32(ins), ins["alpha"], act)
    words, S, M = _hand_acc(want_S, C, n_rep, "round_robin", 621)
    lds = (C, C, C, C)
    a = _backward(ins, act, lds, add="aligned", acc=words, n_rep=n_rep)
    b = _backward(ins, act, lds, add="aligned", partial=S.unsqueeze(0).contiguous(), nblk=1)
    _grade_exact_backward(a, ins, act, S, M, f"agreement exact C{C} rep{n_rep}")
    _grade_backward(b, ins, act, f"agreement partials C{C}", part=S.unsqueeze(0), stage="from_partials")
    same = all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in ("dgamma", "dbeta", "dalpha"))
    cols = torch.stack([a[k].view(torch.int32) == b[k].view(torch.int32) for k in ("dgamma", "dbeta", "dalpha")]).all(0)
    dx_same = (a["dx"].view(torch.int32) == b["dx"].view(torch.int32)).all(0)
    print(f"graphnorm agreement C{C} rep{n_rep}: parameter gradients bit-equal in {int(cols.sum())} of {C} columns, dx in {int(dx_same.sum())}")
    if same:
        assert bool(dx_same.all()), "equal sums and coefficients, different dx"


def test_zz_print_worst_shares():
    """(last in the module) the table for the docstring and the commit message"""
    for fam, w in sorted(_WORST.items()):
        print(f"WORST {fam:14s} " + " ".join(f"{k} {v:.3f}" for k, v in w.items()))
