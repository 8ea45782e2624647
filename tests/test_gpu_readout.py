"""The fused training readout's sum / mean / size entry (glass_readout_train_f32) on the GPU through every launch form, graded
stage by stage and element by element against tests/readout_oracle.py: every output and every workspace intermediate against
the fp64 function of the kernel's own upstream outputs at |got - want| <= 1e-5 * mass, and every case also end to end against
the fp64 chain (pinned to autograd on the CPU) at rel-inf <= 1e-5.  Every case asserts the dispatch record it was written for
(the test cannot observe the launches, so it asserts the restatement the host test ties to the source text), runs twice and
must give identical bits in every output, starts from outputs filled with NaN (every element must be written; guard columns
must still hold NaN afterwards).

Forms: plain = no label list (reduce launch, dense kernel, ordered scatter / gather-add); lab = the listed pooled rows (reduce
launch, one-launch backfill); two = lab + gn_bwd_acc (two launches: `partial` and `coef` are not written to memory then).  The
scalar form (C % 4 != 0, a row stride off 4, a base pointer off 16 bytes) always needs the label bytes.

Widths beyond 256 columns in the scalar form (C = 258; C = 260 with ldj = 261): the parent commit's VW = 1 subgraph kernel
gave a thread the single column tid & 255, so columns 256 .. C - 1 were never pooled — pooled[b, c] kept its previous
contents (here NaN), logits, loss and every gradient were computed from uninitialised LDS: run against the parent's library
these cases fail, at once with "logits differs between two calls".  Now a scalar thread's four accumulator slots take the
columns c0 + 256 k, and these widths are served.

Bitwise equality between forms: plain, lab and two agree in every bit of pooled, logits, loss, dys, dlogits, djk, dWh, dbh;
dgamma / dbeta / dalpha of `two` come from fixed-point accumulators instead of fp64 partials and are only gated.

Worst share of the 1e-5 * mass bar per stage and form family as measured on MI355X: see MEASURED below."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import readout_oracle as Q  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POOLS = ("sum", "mean", "size")
FORMS = ("plain", "lab", "two")
OUT = ("pooled", "logits", "loss", "djk", "dWh", "dbh", "dgamma", "dbeta", "dalpha")
E2E = ("pooled", "logits", "loss", "djk", "dWh", "dbh")

# worst share of the bar on MI355X over all cases below, per form family (printed again by the last test of the module)
MEASURED = """
  family         pooled logits loss_rows dlogits loss  dys   dWh   dbh   partial coef  dgamma dbeta dalpha djk
  dense+ordered  0.395  0.007  0.016     0.011   0.004 0.018 0.047 0.019 0.131   0.078 0.078  0.006 0.040  0.061
  backfill       0.395  0.007  0.029     0.016   0.004 0.091 0.060 0.066 0.131   0.078 0.078  0.006 0.040  0.061
  two            0.395  0.007  0.029     0.016   0.004 0.091 0.060 0.066 -       -     0.078  0.006 0.040  0.061
  dense+gather   0.023  0.007  0.010     0.010   0.004 0.020 0.032 0.012 0.012   0.006 0.004  0.005 0.005  0.008
  scalar         0.022  0.009  0.015     0.010   0.006 0.016 0.030 0.012 0.012   0.006 0.004  0.005 0.005  0.018
  gn_src: saved 0.005
(pooled 0.395 and partial 0.131 are the 3584-entry rows at C = 1024: one row slot adds them all in turn)
"""

_WORST = {}


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _call(ins, mode, form, grad_loss=1.0, acc_head=0, acc_gn=0, prev=None, loss_sum=None, gn_src=None, saved=None, offset4=False,
          weighted_entry=False, calls=1, jk=None):
    """`calls` calls of glass_readout_train_f32 on one set of buffers (outputs filled with NaN, or `prev` where it
    accumulates); returns the outputs, the carved workspace and gn_saved on the CPU.  gn_src = (n_src, n_rep): the forward sums
    come in exact accumulators filled by glass_graphnorm_stats_exact_f32 and gn_saved (NaN-filled) is written by the call."""
    from glass_amd import _lib, stack
    from glass_amd.ops import _stream
    lib = _lib.load()
    C, K, B, Smax, N, ldj, lddj = (ins[k] for k in ("C", "K", "B", "Smax", "N", "ldj", "lddj"))
    f32 = dict(dtype=torch.float32, device=DEV)
    jk_host = ins["jk"] if jk is None else jk
    if offset4:  # the base pointer one float past a 16-byte boundary
        buf = torch.empty(N * ldj + 4, **f32)
        jk_d = buf[1:1 + N * ldj].view(N, ldj)
        jk_d.copy_(jk_host)
        assert jk_d.data_ptr() % 16 == 4
    else:
        jk_d = jk_host.to(DEV).contiguous()
    d = {k: ins[k].to(DEV).contiguous() for k in ("gamma", "beta", "alpha", "pos", "Wh", "bh", "target")}
    acc_f = None
    if gn_src is not None:
        n_src, n_rep = gn_src
        each = C // n_src
        words = int(lib.glass_gn_exact_words(each))
        acc_f = torch.zeros(n_src * words, dtype=torch.int64, device=DEV)
        for k in range(n_src):
            rc = lib.glass_graphnorm_stats_exact_f32(jk_d.data_ptr() + 4 * k * each, ldj, N, each, acc_f.data_ptr() + 8 * k * words, n_rep, _stream())
            assert rc == 0, lib.glass_last_error_string()
        saved_d = torch.full((4 * C, ), float("nan"), **f32)
        src = _lib.GnSrc(acc_f.data_ptr(), n_src, n_rep, d["gamma"].data_ptr(), d["beta"].data_ptr(), d["alpha"].data_ptr(), float(ins["eps"]))
        src_ptr = src.ptr
    else:
        if saved is None:
            saved = Q.stage_saved(ins["jk"][:, :C], ins["gamma"], ins["beta"], ins["alpha"], ins["eps"])[0].float()
        saved_d, src_ptr = saved.reshape(-1).to(DEV).contiguous(), 0
    nan = float("nan")
    out = dict(pooled=torch.full((B, C), nan, **f32), logits=torch.full((B, K), nan, **f32), loss=torch.full((), nan, **f32),
               djk=torch.full((N, lddj), nan, **f32), dWh=torch.full((K, C), nan, **f32), dbh=torch.full((K, ), nan, **f32),
               dgamma=torch.full((C, ), nan, **f32), dbeta=torch.full((C, ), nan, **f32), dalpha=torch.full((C, ), nan, **f32))
    for k, v in (prev or {}).items():
        out[k] = v.to(DEV).contiguous().clone()
    nbytes = int(lib.glass_readout_ws_bytes(B, C, K))
    assert nbytes == Q.ws_bytes(B, C, K)
    ws = torch.zeros(nbytes // 8 + 1, dtype=torch.float64, device=DEV)
    gl = torch.full((), grad_loss, **f32)
    ls = None if loss_sum is None else torch.full((), loss_sum, **f32)
    aligned = ldj % 4 == 0 and lddj % 4 == 0 and not offset4
    largs, labels = (0, 0, 0), None
    if form in ("lab", "two") or C % 4 or not aligned:
        labels = stack.BatchLabels(N, d["pos"].numel(), DEV)
        labels.load(d["pos"])
        largs = (labels.mask.data_ptr(), labels.rows.data_ptr(), labels.count.data_ptr())
    acc_b = torch.zeros(int(lib.glass_gn_exact_words(C)), dtype=torch.int64, device=DEV) if form == "two" else None
    sws_bytes = int(lib.glass_readout_scatter_ws_bytes(N, B, Smax))
    assert (sws_bytes > 0) == (B * Smax > Q.ORDERED_MAX)
    sws = torch.empty(sws_bytes + 16, dtype=torch.uint8, device=DEV) if sws_bytes else None
    fn = lib.glass_readout_train_w_f32 if weighted_entry else lib.glass_readout_train_f32
    wargs = (0, 0) if weighted_entry else ()
    for _ in range(calls):
        if acc_b is not None:
            acc_b.zero_()
        rc = fn(jk_d.data_ptr(), ldj, saved_d.data_ptr(), d["gamma"].data_ptr(), d["alpha"].data_ptr(), d["pos"].data_ptr(), B, Smax,
                Q.MODES[mode], d["Wh"].data_ptr(), d["bh"].data_ptr(), d["target"].data_ptr(), ins["loss_mode"], K, gl.data_ptr(),
                out["pooled"].data_ptr(), out["logits"].data_ptr(), out["loss"].data_ptr(), out["djk"].data_ptr(), lddj,
                out["dWh"].data_ptr(), out["dbh"].data_ptr(), acc_head, out["dgamma"].data_ptr(), out["dbeta"].data_ptr(),
                out["dalpha"].data_ptr(), acc_gn, ws.data_ptr(), N, C, *largs, src_ptr, 0 if acc_b is None else acc_b.data_ptr(),
                stack.REP_DENSE, 0 if sws is None else sws.data_ptr(), 0 if ls is None else ls.data_ptr(), *wargs, _stream())
        assert rc == 0, lib.glass_last_error_string()
    torch.cuda.synchronize()
    res = {k: v.cpu() for k, v in out.items()}
    res.update(Q.carve_ws(ws.view(torch.uint8)[:nbytes].cpu(), B, C, K))
    res["saved"] = saved_d.cpu().reshape(4, C)
    if ls is not None:
        res["loss_sum"] = ls.cpu()
    return res


def _record(ins, form, offset4=False):
    C, B, Smax, N = ins["C"], ins["B"], ins["Smax"], ins["N"]
    aligned = ins["ldj"] % 4 == 0 and ins["lddj"] % 4 == 0 and not offset4
    scalar = C % 4 != 0 or not aligned
    return Q.dispatch(C, B, Smax, N, aligned=aligned, labels=form in ("lab", "two") or scalar, bwd_acc=form == "two",
                      longest_list=int(Q.multiplicity(ins["pos"], N).max()))


def _check(got, ins, mode, rec, label, family, grad_loss=1.0, prev=None, e2e=True):
    """guard columns, the stage gates, the end-to-end rel-inf; records the worst shares per family"""
    C = ins["C"]
    if ins["lddj"] > C:
        assert bool(torch.isnan(got["djk"][:, C:]).all()), f"{label}: guard columns of d jk were written"
    res = Q.grade(got, ins, mode, rec, grad_loss=grad_loss, prev=prev)
    print(f"readout {label} [{family}]: " + " ".join(f"{k} {v[1]:.3f}" for k, v in res.items()))
    bad = {k: v for k, v in res.items() if not v[0]}
    assert not bad, f"{label}: {bad}"
    w = _WORST.setdefault(family, {})
    for k, v in res.items():
        w[k] = max(w.get(k, 0.0), v[1])
    if e2e:
        want = Q.chain(ins, mode, grad_loss, prev)
        errs = {k: Q.rel_inf(got[k][:, :C] if k == "djk" else got[k], want[k]) for k in E2E}
        assert all(v <= Q.TOL for v in errs.values()), f"{label}: end to end {errs}"


def _run(ins, mode, form, expect, label, family, **kw):
    """one case: the record, two calls with the same bits, all gates"""
    ins = Q.for_mode(ins, mode)
    rec = _record(ins, form, kw.get("offset4", False))
    for k, v in expect.items():
        assert rec[k] == v, f"{label}: dispatch {k} = {rec[k]}, the case was written for {v}"
    got, again = _call(ins, mode, form, **kw), _call(ins, mode, form, **kw)
    for k in got:
        assert _same_bits(got[k], again[k]), f"{label}: {k} differs between two calls"
    chk = {k: kw[k] for k in ("grad_loss", "prev") if k in kw}
    _check(got, ins, mode, rec, label, family, **chk)
    if ins["facts"]["all_padding"] is not None:
        assert float(got["pooled"][1].abs().sum()) == 0.0
    return got, rec


# ---- lane geometry, loops, stash, ordered limit --------------------------------------------------------------------------------------
# (C, K, B, Smax, N, expected record)
GEOMETRY = [(4, 3, 40, 3, 300, dict(tc=1, vec=True)), (64, 3, 40, 3, 300, dict(tc=16, early=True)), (96, 3, 40, 3, 300, dict(tc=32)),
            (128, 3, 40, 3, 300, dict(tc=32, early=True)), (132, 3, 40, 3, 300, dict(tc=64, early=False)),
            (1024, 3, 40, 3, 300, dict(tc=256, rpb=1, loop="unrolled"))]
LOOPS = [(64, 3, 40, 32, 300, dict(loop="short", stash=False)), (64, 3, 40, 33, 300, dict(loop="unrolled", stash=True)),
         (1024, 3, 40, 2, 300, dict(loop="short", rpb=1)),
         (17, 3, 40, 16, 300, dict(loop="short", vec=False, tc=32)), (17, 3, 40, 17, 300, dict(loop="unrolled", vec=False, stash=True)),
         (64, 3, 12, 256, 300, dict(loop="unrolled", stash=True)), (64, 3, 12, 257, 300, dict(loop="unrolled", stash=True)),
         (1024, 3, 4, 3584, 300, dict(stash=True, lds1=65536)), (1024, 3, 4, 3585, 300, dict(stash=False, lds1=51200, loop="unrolled"))]
TAILS = {"plain": "dense+ordered", "lab": "backfill", "two": "backfill"}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", POOLS)
@pytest.mark.parametrize("C,K,B,Smax,N,expect", GEOMETRY + LOOPS, ids=[f"C{c}_S{s}_B{b}" for c, _k, b, s, _n, _e in GEOMETRY + LOOPS])
def test_lane_geometry_loops_and_stash(C, K, B, Smax, N, expect, mode, form):
    ins = Q.recipe(C, K, B, Smax, N, seed=100 + C + Smax)
    exp = dict(expect)
    if C % 4 == 0:
        exp.update(tail=TAILS[form], two=form == "two")
    else:
        exp.update(tail="scalar", two=False)
    got, rec = _run(ins, mode, form, exp, f"C{C} S{Smax} {mode} {form}", ("two" if form == "two" and C % 4 == 0 else exp["tail"]))
    if ins["facts"]["twice"]:  # the node listed twice counts twice: its row of d jk carries 2 A dy on top of the dense part
        b, n = ins["facts"]["twice"]
        assert int(Q.multiplicity(ins["pos"], N)[n]) == 2


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", POOLS)
def test_ordered_limit_exactly(mode, form):
    """128 x 128 = 16 384 entries: the last size of the LDS-staged forms; `two` needs 65 536 + 28 C bytes of dynamic LDS in
    readout_backfill_kernel<false> (its own hipFuncSetAttribute)."""
    ins = Q.recipe(64, 3, 128, 128, 300, seed=7)
    exp = dict(tail=TAILS[form], two=form == "two")
    if form == "two":
        exp["lds3"] = 65536 + 28 * 64
    _run(ins, mode, form, exp, f"128x128 {mode} {form}", "two" if form == "two" else exp["tail"])


@pytest.mark.parametrize("form", ["plain", "two"])
@pytest.mark.parametrize("mode", POOLS)
def test_beyond_the_ordered_limit_gather_add(mode, form):
    """5 x 3277 = 16 385 entries: dense kernel + bucketed gather-add with scatter_ws — also with the label list and gn_bwd_acc
    given, which must select neither the backfill nor the two-launch form."""
    ins = Q.recipe(64, 3, 5, 3277, 300, seed=8)
    _run(ins, mode, form, dict(tail="dense+gather", two=False), f"5x3277 {mode} {form}", "dense+gather")


@pytest.mark.parametrize("mode", POOLS)
def test_gather_add_short_and_workgroup_wide_lists(mode):
    """130 x 128 with nodes of exactly 63, 64 and 65 entries: the lane-group path (< 64) and the workgroup-wide path of
    readout_gather_add_kernel"""
    ins = Q.recipe(64, 3, 130, 128, 300, seed=9, shared=((11, 63), (12, 64), (13, 65)))
    mult = Q.multiplicity(ins["pos"], 300)
    assert [int(mult[n]) for n in (11, 12, 13)] == [63, 64, 65]
    _run(ins, mode, "plain", dict(tail="dense+gather", long_lists=True), f"130x128 {mode}", "dense+gather")


def test_gather_add_sum_beyond_the_fixed_point_range_is_exact_or_nan():
    """130 x 128, grad_loss scaled (from the fp64 chain on the CPU, not from the kernel) so that node 13's 65 addends A * g sum
    to 1.5 * 2^43 in one column: beyond ExactSum's range.  The parent commit merged the lanes' limbs with plain integer adds,
    so the sum wrapped into a finite number of the wrong sign (run against the parent's library this test fails with "a finite
    element is not the sum").  Now the merge
    sets the sticky mark: that element is NaN — or, were it in range, the exact sum.  An element whose addends' absolute
    values sum to less than 2^41 (inside both the addend and the sum range, bucket.h) is gated as always."""
    ins = Q.for_mode(Q.recipe(64, 3, 130, 128, 300, seed=9, shared=((11, 63), (12, 64), (13, 65))), "sum")
    C, N, pos = 64, 300, ins["pos"]
    unit = Q.chain(ins, "sum", 1.0)
    rows13 = (pos == 13).any(1)
    signed = (unit["coef"][0] * unit["dys"][rows13]).sum(0)
    col = int(signed.abs().argmax())
    gl = float(1.5 * 2.0**43 / signed[col].abs())
    want = Q.chain(ins, "sum", gl)
    v = Q.valid_of(pos, N)
    bidx = torch.arange(130).reshape(-1, 1).expand(130, 128)[v]
    mass_g = torch.zeros(N, C, dtype=torch.float64).index_add_(0, pos[v], (want["coef"][0] * want["dys"][bidx]).abs())
    assert float(mass_g[13, col]) > 2.0**43 and abs(float((want["coef"][0] * want["dys"][rows13]).sum(0)[col])) > 2.0**43
    in_range = mass_g < 2.0**41
    assert bool(in_range[N - 1].all()) and int(in_range.sum()) > 0
    rec = _record(ins, "plain")
    assert rec["tail"] == "dense+gather" and rec["long_lists"]
    got = _call(ins, "sum", "plain", grad_loss=gl)
    djk = got["djk"].double()
    coefw, coefm = (Q.stage_gn_bwd(*Q.stage_partial(got["dys"], ins["jk"], got["saved"], ins["alpha"], pos), N, ins["gamma"], ins["alpha"],
                                   got["saved"])["coef"])
    w, m = Q.stage_djk(ins["jk"], coefw, coefm, got["dys"], pos)
    isnan = torch.isnan(djk)
    assert not bool((isnan & in_range).any()), "an in-range element is NaN"
    share = ((djk - w).abs() / (Q.TOL * m))
    assert bool((share[~isnan] <= 1.0).all()), "a finite element is not the sum"   # never a finite value of the wrong sign
    assert bool(isnan[13, col]), "node 13's sum left the range: the sticky mark makes it NaN"
    print(f"overflow case: grad_loss {gl:.3e}, column {col}, NaN elements {int(isnan.sum())}, out-of-range elements {int((~in_range).sum())}")
    for k in ("pooled", "logits", "loss"):
        assert Q.rel_inf(got[k], want[k]) <= Q.TOL, k


# ---- grid caps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,form,cap", [(16384, "plain", False), (16500, "plain", True), (32768, "lab", False), (33000, "lab", True)])
def test_grid_caps_second_round_of_rows(N, form, cap):
    """C = 1024 (one row per 256 threads): 4096 dense workgroups x 4 rows = 16 384 rows, 2048 backfill workgroups x 4 rows x 4 =
    32 768; beyond them a thread takes a second round of rows.  Sum mode; graded on 600 rows that hold every pooled row, the
    first and last rows of each round."""
    ins = Q.for_mode(Q.recipe(1024, 3, 6, 5, N, seed=10), "sum")
    C, pos = 1024, ins["pos"]
    tail = TAILS[form]
    rec = _record(ins, form)
    assert rec["tail"] == tail and rec["cap"] == cap and rec["rpb"] == 1
    got, again = _call(ins, "sum", form), _call(ins, "sum", form)
    for k in got:
        assert _same_bits(got[k], again[k]), k
    per = 4 * (Q.DENSE_CAP if form == "plain" else Q.BACKFILL_CAP * 4)
    pooled_rows = torch.unique(pos[Q.valid_of(pos, N)])
    rows = torch.unique(torch.cat([pooled_rows, torch.arange(0, 200), torch.arange(per - 200, min(per + 200, N)), torch.arange(N - 200, N)]))
    assert not bool(torch.isnan(got["djk"]).any()), "a row of d jk was not written"
    res = Q.grade(got, ins, "sum", rec, rows=rows)
    print(f"grid cap N={N} {form}: " + " ".join(f"{k} {v[1]:.3f}" for k, v in res.items()))
    assert all(v[0] for v in res.values()), res
    # every unpooled row, all N of them, is the dense part alone: Bx * x + K from the coefficients as the kernel wrote them,
    # one fp32 rounding (2^-24 of |Bx x| + |K| would do; held to 1e-5 of it)
    Bx, Kc = got["coef"][1].double(), got["coef"][2].double()
    unp = torch.ones(N, dtype=torch.bool)
    unp[pooled_rows] = False
    for r0 in range(0, N, 4096):
        x = ins["jk"][r0:r0 + 4096].double()
        err = (got["djk"][r0:r0 + 4096].double() - (Bx * x + Kc)).abs()
        assert bool((err <= Q.TOL * ((Bx * x).abs() + Kc.abs()))[unp[r0:r0 + 4096]].all()), f"rows {r0} .."
    if cap:  # the second round explicitly: row 4 * grid * rows-per-workgroup is taken by the thread that took row 0
        first, second = Q.second_round_rows(C, N, tail)
        assert second == per and second < N and bool(unp[first]) and bool(unp[second]) and bool(keep_rows(rows, first, second))
        assert not _same_bits(got["djk"][second], got["djk"][first])
        pair = torch.tensor([first, second])
        ok, share, _ = Q.gate(got["djk"][pair], *Q.stage_djk(ins["jk"], got["coef"].double(), got["coef"].double().abs(), got["dys"], pos, pair))
        assert ok, share
    want = Q.chain(ins, "sum", rows=rows)
    assert Q.rel_inf(got["djk"][rows], want["djk"]) <= Q.TOL
    for k in ("pooled", "logits", "loss", "dWh", "dbh"):
        assert Q.rel_inf(got[k], want[k]) <= Q.TOL, k


def keep_rows(rows, *which):
    return all(int(w) in set(rows.tolist()) for w in which)


# ---- scalar form ---------------------------------------------------------------------------------------------------------------------
SCALAR = [(17, None, False), (1, None, False), (255, None, False), (64, 65, False), (64, None, True), (258, None, False), (260, 261, False)]


@pytest.mark.parametrize("mode", POOLS)
@pytest.mark.parametrize("C,ldj,offset4", SCALAR, ids=[f"C{c}" + (f"_ldj{l}" if l else "") + ("_off4" if o else "") for c, l, o in SCALAR])
def test_scalar_form(C, ldj, offset4, mode):
    """one column per lane: odd widths, a vector-capable width forced scalar by its row stride or its base pointer, and the
    widths beyond 256 columns (see the module docstring for what the parent commit did with them)"""
    ins = Q.recipe(C, 3, 40, 3, 300, seed=200 + C, ldj=ldj)
    exp = dict(vec=False, tail="scalar", two=False, slots_used=-(-C // 256))
    _run(ins, mode, "two", exp, f"scalar C{C} ldj{ldj} off{offset4} {mode}", "scalar", offset4=offset4)


def test_scalar_form_long_rows_beyond_256_columns():
    """C = 258, Smax = 9 > 2 row slots' worth: the unrolled loop with the four column slots live"""
    ins = Q.recipe(258, 3, 12, 9, 300, seed=33)
    _run(ins, "mean", "lab", dict(vec=False, loop="unrolled", tc=256, slots_used=2), "scalar C258 S9", "scalar")


# ---- head sizes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["lab", "two"])
@pytest.mark.parametrize("K,loss_mode", [(1, 1), (4, 0), (4, 1), (5, 0), (5, 1), (256, 0), (256, 1)])
def test_head_sizes(K, loss_mode, form):
    """K = 1 .. 256 at C = 64: the head-weight prefetch serves a wave's first class only (K > 4: a second round per wave)"""
    ins = Q.recipe(64, K, 40, 3, 300, seed=300 + K, loss_mode=loss_mode)
    _run(ins, "mean", form, dict(tail="backfill", two=form == "two"), f"K{K} loss{loss_mode} {form}", "two" if form == "two" else "backfill")


@pytest.mark.parametrize("form", ["lab", "two"])
@pytest.mark.parametrize("B", [1, 257, 300])
def test_batch_sizes(B, form):
    """B = 1; B > 256: a second round of the loss reduction loops"""
    ins = Q.recipe(64, 3, B, 3, 300, seed=400 + B)
    _run(ins, "size", form, dict(tail="backfill", two=form == "two"), f"B{B} {form}", "two" if form == "two" else "backfill")


# ---- gn_src ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("C,n_src,n_rep,early", [(64, 1, 2, True), (64, 1, 16, True), (128, 2, 16, True), (128, 2, 2, True), (256, 2, 16, False),
                                                 (256, 2, 2, False)])
def test_statistics_from_exact_accumulators(C, n_src, n_rep, early, form):
    """The forward sums arrive in exact accumulators (n_src column blocks, n_rep replicas, filled by the statistics entry);
    workgroup 0 writes gn_saved: graded against fp64 column sums, and every output equals, bit for bit, the same call given
    final statistics equal to that gn_saved."""
    ins = Q.for_mode(Q.recipe(C, 3, 40, 3, 300, seed=500 + C), "mean")
    rec = _record(ins, form)
    assert rec["early"] == early and rec["two"] == (form == "two")
    got = _call(ins, "mean", form, gn_src=(n_src, n_rep))
    ok, share, at = Q.gate(got["saved"], *Q.stage_saved(ins["jk"], ins["gamma"], ins["beta"], ins["alpha"], ins["eps"]))
    print(f"gn_src C={C} n_src={n_src} n_rep={n_rep} {form}: saved {share:.3f}")
    assert ok, (share, at)
    _WORST.setdefault("gn_src", {})["saved"] = max(_WORST.get("gn_src", {}).get("saved", 0.0), share)
    _check(got, ins, "mean", rec, f"gn_src C{C} {form}", "two" if form == "two" else rec["tail"])
    final = _call(ins, "mean", form, saved=got["saved"])
    for k in got:
        assert _same_bits(got[k], final[k]), f"{k}: differs from the call given final statistics"


# ---- accumulate, seeds, strides --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_accumulate_seed_loss_sum_and_guard_columns(form):
    """acc_head = acc_gn = 1 over nonzero previous contents, grad_loss = -2.5, loss_sum from 3.0 over two calls, ldj = C + 8,
    lddj = C + 4 with guard columns"""
    C, K = 64, 3
    ins = Q.for_mode(Q.recipe(C, K, 40, 3, 300, seed=600, ldj=C + 8, lddj=C + 4), "size")
    g = torch.Generator().manual_seed(601)
    prev = dict(dWh=torch.randn(K, C, generator=g), dbh=torch.randn(K, generator=g), dgamma=torch.randn(C, generator=g),
                dbeta=torch.randn(C, generator=g), dalpha=torch.randn(C, generator=g))
    rec = _record(ins, form)
    assert rec["vec"] and rec["two"] == (form == "two")
    kw = dict(grad_loss=-2.5, acc_head=1, acc_gn=1, prev=prev, loss_sum=3.0)
    got, again = _call(ins, "size", form, **kw), _call(ins, "size", form, **kw)
    for k in got:
        assert _same_bits(got[k], again[k]), k
    _check(got, ins, "size", rec, f"accumulate {form}", "two" if form == "two" else rec["tail"], grad_loss=-2.5, prev=prev)
    assert float(got["loss_sum"]) == float(torch.tensor(3.0) + got["loss"])
    twice = _call(ins, "size", form, calls=2, **kw)
    assert float(twice["loss_sum"]) == float((torch.tensor(3.0) + got["loss"]) + got["loss"])
    # without the flags the previous contents are overwritten
    plain = _call(ins, "size", form, grad_loss=-2.5, prev=prev)
    _check(plain, ins, "size", rec, f"overwrite {form}", "two" if form == "two" else rec["tail"], grad_loss=-2.5)


# ---- forms against each other ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", POOLS)
def test_forms_give_the_same_bits_and_the_weighted_entry_too(mode):
    ins = Q.for_mode(Q.recipe(64, 3, 40, 9, 300, seed=700), mode)
    got = {f: _call(ins, mode, f) for f in FORMS}
    for k in ("pooled", "logits", "loss", "dys", "dlogits", "loss_rows", "djk", "dWh", "dbh"):
        assert _same_bits(got["plain"][k], got["lab"][k]) and _same_bits(got["lab"][k], got["two"][k]), k
    for k in ("partial", "coef", "dgamma", "dbeta", "dalpha"):
        assert _same_bits(got["plain"][k], got["lab"][k]), k
    for f in ("lab", "two"):  # null weights through glass_readout_train_w_f32
        w = _call(ins, mode, f, weighted_entry=True)
        for k in got[f]:
            assert _same_bits(w[k], got[f][k]), (f, k)


# ---- non-finite ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_nan_in_an_unpooled_row_stays_in_its_element(form):
    """A NaN in jk at a node no row names (statistics supplied by the caller, from the clean matrix): NaN in exactly that element
    of d jk, every other output bit-equal to the clean run."""
    ins = Q.for_mode(Q.recipe(64, 3, 40, 3, 300, seed=800), "sum")
    n, c = 299, 5
    assert int(Q.multiplicity(ins["pos"], 300)[n]) == 0
    clean = _call(ins, "sum", form)
    jk = ins["jk"].clone()
    jk[n, c] = float("nan")
    got = _call(ins, "sum", form, jk=jk)
    assert bool(torch.isnan(got["djk"][n, c])) and int(torch.isnan(got["djk"]).sum()) == 1
    for k in got:
        a, b = got[k].clone(), clean[k].clone()
        if k == "djk":
            a[n, c] = b[n, c] = 0.0
        assert _same_bits(a, b), k


def test_zz_print_worst_shares():
    """(last in the module) the table for the docstring and the commit message"""
    for fam, w in sorted(_WORST.items()):
        print(f"WORST {fam:14s} " + " ".join(f"{k} {v:.3f}" for k, v in w.items()))
