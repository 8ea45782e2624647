"""K9 alone through the C ABI (glass_pair_head_{fwd,bwd}_f32, pairhead.hip) against its fp64 statement
(tests/pair_head_oracle.py) at the edges of its tiles, lists and arguments: the last 64-pair forward tile and 256-row
weight-gradient slab, a slab of one 16-row stage, the reduce kernel's second round, the 64-entry switch of the embedding
gradient's list walk, ids outside [0, N), leading dimensions, dropout on the very scales the kernel drew, accumulate /
grad_scale, the evaluation form, saturated logits, addends near the fixed-point quantum, and the reported workspace size.

Every run keeps its buffers between canaries (NaN rows around emb; marked rows / bytes around hid, logits, dlogit, demb
and a workspace of exactly glass_pair_head_ws_bytes) and checks them.  Every comparison is made on the ReLU branches the
kernel took (hid > 0), bars as in test_gpu_ssl_program.py::test_pair_head_kernels_vs_fp64: rel-inf 1e-6 for logits / loss,
2e-6 for gradients."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_head_oracle as PH  # noqa: E402
from helpers import rel_inf, record_parity  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = 64
FWD_BAR, GRAD_BAR = 1e-6, 2e-6
MARK = -7.25            # canary value of the float buffers
WS_GUARD = 4096         # canary bytes on either side of the workspace
GRADS = ("dW0", "db0", "dw1", "db1")


@pytest.fixture(scope="module", autouse=True)
def _module_cost():
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    wall, peak = time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 2**20
    print(f"test_gpu_pair_head: {wall:.1f} s, peak device memory {peak:.0f} MiB")


def _inputs(n, P, seed, pairs=None):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(n, H, generator=g)
    rnd = torch.randint(0, n, (P, 2), generator=g)
    y = torch.randint(0, 2, (P, ), generator=g).float()
    W0, b0 = torch.randn(H, H, generator=g) * 0.2, torch.randn(H, generator=g) * 0.1
    w1, b1 = torch.randn(H, generator=g) * 0.3, torch.randn(1, generator=g)
    return dict(emb=emb, pairs=rnd if pairs is None else pairs, y=y, W0=W0, b0=b0, w1=w1, b1=b1)


def _run(c, p=0.0, call_id=2, gscale=None, accumulate=0, prefill=None, lde=H, col0=0, ldde=H, dcol0=0, want_loss=True):
    """One training forward + backward.  Returns CPU tensors (hid, logits, dlogit, loss, dW0, db0, dw1, db1, demb, and the
    whole demb buffer with its canary rows / columns as `dbuf`) after checking every canary."""
    from glass_amd import _lib, ops
    lib = _lib.load()
    n, P = c["emb"].shape[0], c["pairs"].shape[0]
    f32 = dict(dtype=torch.float32, device=DEV)
    ebuf = torch.full((n + 2, lde), float("nan"), **f32)       # NaN rows before and after, NaN columns beside
    ebuf[1:n + 1, col0:col0 + H] = c["emb"].to(DEV)
    dbuf = torch.full((n + 2, ldde), MARK, **f32)
    hbuf, lbuf, gbuf = torch.full((P + 2, H), MARK, **f32), torch.full((P + 8, ), MARK, **f32), torch.full((P + 8, ), MARK, **f32)
    pairs, y = c["pairs"].to(DEV).contiguous(), c["y"].to(DEV).contiguous()
    W0, b0, w1, b1 = (c[k].to(DEV).contiguous() for k in ("W0", "b0", "w1", "b1"))
    need = int(lib.glass_pair_head_ws_bytes(n, P))
    assert need > 0
    wbuf = torch.full((WS_GUARD + need + WS_GUARD, ), 0xA5, dtype=torch.uint8, device=DEV)
    ws_ptr = wbuf.data_ptr() + WS_GUARD
    assert ws_ptr % 16 == 0
    if prefill is None:
        prefill = {k: torch.full(s, float("nan")) for k, s in zip(GRADS, ((H, H), (H, ), (H, ), (1, )))}
    gr = {k: prefill[k].to(DEV).clone() for k in GRADS}
    loss = torch.full((), MARK, **f32)
    gs = torch.tensor([gscale], **f32) if gscale is not None else None
    rng = ops.rng_state(DEV).data_ptr() if p > 0 else None
    emb_ptr, demb_ptr = ebuf.data_ptr() + (lde + col0) * 4, dbuf.data_ptr() + (ldde + dcol0) * 4
    hid_ptr, logit_ptr, dlogit_ptr = hbuf.data_ptr() + H * 4, lbuf.data_ptr() + 16, gbuf.data_ptr() + 16
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.glass_pair_head_fwd_f32(emb_ptr, lde, n, pairs.data_ptr(), P, W0.data_ptr(), b0.data_ptr(), w1.data_ptr(),
                                           b1.data_ptr(), y.data_ptr(), float(p), rng, call_id, gs.data_ptr() if gs is not None else None,
                                           hid_ptr, logit_ptr, dlogit_ptr, ws_ptr, st), "glass_pair_head_fwd_f32")
    _lib.check(lib.glass_pair_head_bwd_f32(emb_ptr, lde, n, pairs.data_ptr(), P, W0.data_ptr(), w1.data_ptr(), hid_ptr, dlogit_ptr,
                                           float(p), gr["dW0"].data_ptr(), gr["db0"].data_ptr(), gr["dw1"].data_ptr(),
                                           gr["db1"].data_ptr(), accumulate, loss.data_ptr() if want_loss else None, demb_ptr, ldde,
                                           ws_ptr, st), "glass_pair_head_bwd_f32")
    torch.cuda.synchronize()
    wb = wbuf.cpu()
    assert bool((wb[:WS_GUARD] == 0xA5).all()) and bool((wb[WS_GUARD + need:] == 0xA5).all()), \
        f"the workspace of glass_pair_head_ws_bytes({n}, {P}) = {need} bytes was overrun"
    hb, lb, gb, db = hbuf.cpu(), lbuf.cpu(), gbuf.cpu(), dbuf.cpu()
    for name, guard in (("hid", torch.cat([hb[0], hb[P + 1]])), ("logits", torch.cat([lb[:4], lb[P + 4:]])),
                        ("dlogit", torch.cat([gb[:4], gb[P + 4:]])), ("demb rows", torch.cat([db[0], db[n + 1]])),
                        ("demb columns", torch.cat([db[:, :dcol0].reshape(-1), db[:, dcol0 + H:].reshape(-1)]))):
        assert bool((guard == MARK).all()), f"{name}: written outside the tensor"
    out = dict(hid=hb[1:P + 1], logits=lb[4:P + 4], dlogit=gb[4:P + 4], loss=loss.cpu(), demb=db[1:n + 1, dcol0:dcol0 + H], dbuf=db)
    out.update({k: v.cpu() for k, v in gr.items()})
    return out


def _eval_logits(c):
    """The evaluation form: target = hid = dlogit = ws = NULL."""
    from glass_amd import _lib
    lib = _lib.load()
    n, P = c["emb"].shape[0], c["pairs"].shape[0]
    d = {k: c[k].to(DEV).contiguous() for k in ("emb", "pairs", "W0", "b0", "w1", "b1")}
    lbuf = torch.full((P + 8, ), MARK, dtype=torch.float32, device=DEV)
    _lib.check(lib.glass_pair_head_fwd_f32(d["emb"].data_ptr(), H, n, d["pairs"].data_ptr(), P, d["W0"].data_ptr(), d["b0"].data_ptr(),
                                           d["w1"].data_ptr(), d["b1"].data_ptr(), None, 0.0, None, 0, None, None, lbuf.data_ptr() + 16,
                                           None, None, torch.cuda.current_stream().cuda_stream), "glass_pair_head_fwd_f32 (evaluation)")
    torch.cuda.synchronize()
    lb = lbuf.cpu()
    assert bool((torch.cat([lb[:4], lb[P + 4:]]) == MARK).all())
    return lb[4:P + 4]


def _ref(c, out, scales=None, gscale=1.0, dtype=torch.float64):
    return PH.pair_head(c["emb"], c["pairs"], c["W0"], c["b0"], c["w1"], c["b1"], c["y"], scales=scales,
                        relu_mask=out["hid"] > 0, grad_scale=gscale, dtype=dtype)


def _errors(out, ref):
    e = {k: rel_inf(out[k], ref[k]) for k in ("hid", "logits", "dlogit", "demb") + GRADS}
    e["loss"] = abs(float(out["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    return e


def _fp32_floor(c, out, ref, **kw):
    """The error of the SAME statement evaluated in fp32 on the CPU (same ReLU branches, same scales) against fp64: what
    the number format itself costs at this input."""
    return _errors(_ref(c, out, dtype=torch.float32, **kw), ref)


def _compare(tag, c, out, ref, floor=None, floor_keys=()):
    """Print and record every error, then assert: 1e-6 for hid / logits / loss, 2e-6 for dlogit and the gradients.  A
    quantity named in `floor_keys` (one measured above its bar, with the figures in the test's docstring) may also be within
    4 x the fp32 statement's own error (`floor` = _fp32_floor; summation order differs).  A node no valid entry names gets an
    exactly zero row."""
    e = _errors(out, ref)
    print(f"pair head {tag}: " + " ".join(f"{k} {v:.2e}" for k, v in e.items()))
    record_parity(f"pair_head/{tag}", **e)
    if floor is not None:
        print(f"pair head {tag} fp32 floor: " + " ".join(f"{k} {v:.2e}" for k, v in floor.items()))
        record_parity(f"pair_head/{tag}_fp32_floor", **floor)
    for k in ("hid", "logits", "dlogit", "loss", "demb") + GRADS:
        assert bool(torch.isfinite(out[k]).all()), f"{tag}: {k} not finite"
    n = c["emb"].shape[0]
    flat = c["pairs"].reshape(-1)
    named = torch.zeros(n, dtype=torch.bool)
    named[flat[(flat >= 0) & (flat < n)]] = True
    assert float(out["demb"][~named].abs().max() if bool((~named).any()) else 0.0) == 0.0, f"{tag}: a node no pair names has a gradient"
    for k, v in e.items():
        bar = FWD_BAR if k in ("hid", "logits", "loss") else GRAD_BAR
        if k in floor_keys:
            bar = max(bar, 4.0 * floor[k])
        assert v < bar, f"{tag}: {k} rel-inf {v:.3e} >= {bar:.3e}"
    return e


# ---- P edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 32768, 32769])
def test_pair_count_edges(P):
    """n = 1001 nodes (not a multiple of the 16-node groups of the embedding gradient), P on either side of the 16-row stage,
    the 64-pair forward tile and the 256-row slab; 32 768 / 32 769 = 128 slabs / 128 slabs + 1 row: the reduce kernel's
    second round, whose last slab holds one stage of one row.  Also the evaluation form (target = hid = dlogit = ws = NULL):
    its logits are the training forward's, bitwise.
    Seed 100 + P, but 216 at P = 16: at seed 116 the sixteen signed dlogit cancel 82-fold in db1 (sum |dlogit| / |sum dlogit|
    of the fp64 statement; 1.15 at seed 216), and rel-inf of that one number would measure the input."""
    c = _inputs(1001, P, 216 if P == 16 else 100 + P)
    out = _run(c)
    _compare(f"P{P}", c, out, _ref(c, out))
    assert torch.equal(_eval_logits(c), out["logits"])


# ---- list lengths -------------------------------------------------------------------------------------------------------
LIST_COUNTS = {16: 64, 17: 0, 18: 1, 19: 2, 20: 3, 21: 63, 22: 65, 23: 200, 40: 70, 39: 0}


def _list_case():
    """41 nodes = two groups of 16 and a partial one.  Group 16..31 holds three lists of >= 64 entries (16: exactly 64, 22: 65,
    23: 200) next to lists of 0, 1, 2, 3 and 63; node 40 in the partial group has 70; 39 has none.  Self pairs on 16, 19, 23."""
    g = torch.Generator().manual_seed(7)
    n = 41
    left = dict(LIST_COUNTS)
    fill = [v for v in range(n) if v not in left]
    pairs = [(19, 19), (23, 23), (23, 23), (23, 23), (16, 16)] + [(16, 23)] * 10 + [(22, 40)] * 5 + [(40, 21)] * 4
    for a, b in pairs:
        left[a] -= 1
        left[b] -= 1
    for node, k in left.items():
        assert k >= 0
        for i in range(k):
            other = fill[int(torch.randint(0, len(fill), (1, ), generator=g))]
            pairs.append((node, other) if i % 2 == 0 else (other, node))
    pairs = torch.tensor(pairs)[torch.randperm(len(pairs), generator=g)]
    cnt = torch.bincount(pairs.reshape(-1), minlength=n)
    assert all(int(cnt[v]) == k for v, k in LIST_COUNTS.items()) and int(cnt[fill].max()) < 64
    return _inputs(n, pairs.shape[0], 8, pairs=pairs)


def test_list_length_edges_and_repeatability():
    """Entry lists of exactly 0, 1, 2, 3, 63, 64, 65 and 200 entries: the per-lane-group walk (pairs of entries + a tail) and,
    from 64 entries, the whole-workgroup walk — several long lists in one group of 16 nodes, one in the last, partial
    group, self pairs (a, a) counting twice.  Two runs give the same bits in demb and the weight gradients."""
    c = _list_case()
    out = _run(c)
    _compare("list_lengths", c, out, _ref(c, out))
    assert float(out["demb"][[17, 39]].abs().max()) == 0.0 and float(out["demb"][18].abs().max()) > 0
    again = _run(c)
    for k in ("demb", "hid", "logits", "dlogit", "loss") + GRADS:
        assert torch.equal(out[k], again[k]), k


def _single_node_inputs(P, seed):
    """n = 1: every pair is (0, 0), every row of the head is the same row, and rel-inf over a quantity is the relative error
    of ONE number: the logit (a 64-term dot) and, in every gradient, the factor sum_p dlogit[p] = n0 a - n1 b.  With signed
    w1 / b1 that dot may cancel, and an absolute error of a rounding or two of its terms then reads as a large relative error
    of the logit, which measures the input, not the kernel.  So here w1, b1 >= 0: no term of the logit's dot cancels
    (hid >= 0), scaled so that the logit stays between 0.5 and 3 (sigmoid unsaturated), and the conditioning of both numbers
    is asserted on the fp64 statement: 1 for the logit, at most 3 for the sum over dlogit."""
    c = _inputs(1, P, seed, pairs=torch.zeros(P, 2, dtype=torch.int64))
    c["w1"], c["b1"] = c["w1"].abs() * 0.15, c["b1"].abs() * 0.25
    r = PH.pair_head(c["emb"], c["pairs"], c["W0"], c["b0"], c["w1"], c["b1"], c["y"])
    x, dl = r["logits"][0], r["dlogit"]
    assert float(((r["hid"][0] * c["w1"].double()).abs().sum() + c["b1"].double().abs().sum()) / x.abs()) < 1 + 1e-12
    assert 0.5 < float(x) < 3.0
    assert float(dl.abs().sum() / dl.sum().abs()) <= 3.0
    return c


@pytest.mark.parametrize("P", [3, 70])
def test_single_node(P):
    """n = 1: every pair is (0, 0); 6 entries for the short walk, 140 for the long one, on the inputs of
    _single_node_inputs, at the plain bars.  Measured on an MI355X: P = 3 logits 3.5e-8, worst gradient dw1 2.9e-7;
    P = 70 logits 6.0e-8, worst gradient dW0 5.5e-7."""
    c = _single_node_inputs(P, 20 + P)
    out = _run(c)
    _compare(f"single_node_P{P}", c, out, _ref(c, out))


# ---- ids outside [0, N) ---------------------------------------------------------------------------------------------------
def test_invalid_ids_count_as_zero_rows():
    """include/glass_hip.h, K9: an id outside [0, N) counts as a zero row (the mean still divides by 2) and gets no gradient.
    -1, n, n + 7 and 2^40 on one side, on both sides, in the first and the last pair of a forward tile and in the last pair;
    emb lies between NaN rows, so a read of row -1 or row n would show in the logits."""
    n, P = 1001, 197
    c = _inputs(n, P, 31)
    big = 1 << 40
    for row, (a, b) in {0: (-1, None), 63: (None, n), 64: (n + 7, big), 127: (big, -1), 100: (None, -1), 128: (n, None),
                        191: (n + 7, n + 7), 192: (None, big), 196: (n, None)}.items():
        if a is not None:
            c["pairs"][row, 0] = a
        if b is not None:
            c["pairs"][row, 1] = b
    out = _run(c)
    ref = _ref(c, out)
    _compare("invalid_ids", c, out, ref)
    both = PH.pair_head(c["emb"], c["pairs"][[64]], c["W0"], c["b0"], c["w1"], c["b1"], c["y"][[64]])["logits"]
    assert rel_inf(out["logits"][[64, 127, 191]], both.expand(3)) < FWD_BAR  # no valid endpoint: relu(b0) . w1 + b1
    assert torch.equal(_eval_logits(c), out["logits"])


# ---- leading dimensions -----------------------------------------------------------------------------------------------------
def test_leading_dimensions():
    """emb = columns 4..67 of a [n, 132] buffer whose other columns are NaN, demb = columns 4..67 of a [n, 72] buffer: the
    other columns of demb keep their bytes (checked in _run) and the values do not depend on the strides."""
    c = _inputs(1001, 257, 41)
    out = _run(c, lde=132, col0=4, ldde=72, dcol0=4)
    _compare("leading_dims", c, out, _ref(c, out))
    plain = _run(c)
    for k in ("demb", "hid", "logits", "dlogit", "loss") + GRADS:
        assert torch.equal(out[k], plain[k]), k
    mark = torch.full((1, ), MARK).view(torch.int32)
    side = torch.cat([out["dbuf"][:, :4], out["dbuf"][:, 68:]], dim=1).contiguous().view(torch.int32)
    assert bool((side == mark).all())  # bytes, not values


# ---- dropout on the scales the kernel drew ---------------------------------------------------------------------------------
def _scales(call_id, p, P):
    from glass_amd import _lib, ops
    m = torch.empty(P, H, device=DEV)
    _lib.check(_lib.load().glass_dropout_scales_f32(ops.rng_state(DEV).data_ptr(), call_id, p, P, H, m.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream), "glass_dropout_scales_f32")
    return m.cpu()


@pytest.mark.parametrize("p,call_id", [(0.2, 2), (0.5, 2), (0.5, 37)])
def test_dropout_on_the_same_scales(p, call_id):
    """Dropout between the head's Linear and its ReLU: the keep-scales of (seed, step, call id) are read back from the library
    (glass_dropout_scales_f32), are 0 or 1 / (1 - p), hid is exactly 0 where they are 0, and the whole forward and backward
    match fp64 on those scales — a wrong 1 / (1 - p) in either backward kernel, a mask of another stream, or dropped elements
    that get a gradient all show here.  P = 4097: 262 208 draws, kept share within 0.02 of 1 - p (binomial sd 0.001)."""
    from glass_amd import ops
    P = 4097
    c = _inputs(1001, P, 50 + call_id)
    c["pairs"][:100, 1] = 7   # a long list
    ops.rng_seed(1234, DEV)
    out = _run(c, p=p, call_id=call_id)
    sc = _scales(call_id, p, P)
    vals = sorted(sc.unique().tolist())
    assert len(vals) == 2 and vals[0] == 0.0 and abs(vals[1] * (1.0 - p) - 1.0) < 2.0 ** -22   # fp32 1 / (1 - p)
    kept = float((sc > 0).double().mean())
    assert abs(kept - (1.0 - p)) < 0.02
    assert bool((out["hid"][sc == 0] == 0).all())
    assert float((out["hid"][sc > 0] > 0).double().mean()) > 0.3   # ... and only there
    other = _scales(call_id + 1, p, P)
    assert not torch.equal(other, sc)                              # another stream, other masks
    ops.rng_seed(1235, DEV)
    assert not torch.equal(_scales(call_id, p, P), sc)             # another seed, other masks
    e = _compare(f"dropout_p{p}_id{call_id}", c, out, _ref(c, out, scales=sc))
    record_parity(f"pair_head/dropout_p{p}_id{call_id}_kept", kept_share=kept, **e)


# ---- accumulate, grad_scale, loss = NULL ------------------------------------------------------------------------------------
def test_accumulate_grad_scale_and_null_loss():
    """accumulate = 0 over NaN gradient buffers: the gradient alone; accumulate = 1 over random ones: prefill + gradient (the
    same fp32 addition: bitwise); demb is overwritten in both modes (_run starts it from canaries).  grad_scale = 0.37 as a
    device scalar scales dlogit and every gradient, not the loss.  loss = NULL changes nothing else."""
    c = _inputs(1001, 257, 61)
    base = _run(c)
    _compare("accumulate0", c, base, _ref(c, base))
    g = torch.Generator().manual_seed(62)
    pre = {k: torch.randn(base[k].shape, generator=g) for k in GRADS}
    acc = _run(c, accumulate=1, prefill=pre)
    for k in GRADS:
        assert torch.equal(acc[k], pre[k] + base[k]), k
    for k in ("demb", "hid", "logits", "dlogit", "loss"):
        assert torch.equal(acc[k], base[k]), k
    gs = float(torch.tensor(0.37, dtype=torch.float32))
    scaled = _run(c, gscale=0.37)
    assert torch.equal(scaled["logits"], base["logits"]) and torch.equal(scaled["loss"], base["loss"])
    assert torch.equal(scaled["hid"], base["hid"])
    _compare("grad_scale_0.37", c, scaled, _ref(c, scaled, gscale=gs))
    assert rel_inf(scaled["demb"], base["demb"].double() * gs) < GRAD_BAR
    noloss = _run(c, want_loss=False)
    assert float(noloss["loss"]) == MARK   # not written
    for k in ("demb", "hid", "logits", "dlogit") + GRADS:
        assert torch.equal(noloss[k], base[k]), k


# ---- saturated logits -------------------------------------------------------------------------------------------------------
def test_stable_bce_at_large_logits():
    """w1 / b1 scaled so that the logits span about +-200 with targets on both sides: exp(200) overflows fp32, so loss and
    dlogit are finite only in the stable form max(x, 0) - x y + log1p(exp(-|x|)); they match torch's fp64
    binary_cross_entropy_with_logits at the plain bars.  Measured on an MI355X: dlogit 1.74e-6 (a logit of magnitude 200
    carries 200 * 2^-24 = 1.2e-5 of rounding into a sigmoid whose slope is 1 / 4 near 0; the fp32 statement on the CPU has
    4.4e-6), demb 6.7e-7, logits 2.6e-7, loss 3.5e-8, weight gradients under 2.3e-7."""
    c = _inputs(1001, 257, 71)
    x = PH.pair_head(c["emb"], c["pairs"], c["W0"], c["b0"], c["w1"], c["b1"], c["y"])["logits"]
    mid, half = float(x.max() + x.min()) / 2, float(x.max() - x.min()) / 2
    c["w1"], c["b1"] = c["w1"] * (200.0 / half), (c["b1"] - mid) * (200.0 / half)   # logit -> (logit - mid) * 200 / half
    out = _run(c)
    ref = _ref(c, out)
    assert float(ref["logits"].max()) > 190 and float(ref["logits"].min()) < -190
    wrong = (ref["logits"] > 0) != (c["y"] > 0.5)
    assert int((wrong & (ref["logits"].abs() > 100)).sum()) > 3          # terms of ~|x| in the loss, from both sides
    assert int((wrong & (ref["logits"] > 100)).sum()) > 0 and int((wrong & (ref["logits"] < -100)).sum()) > 0
    _compare("stable_bce", c, out, ref)


# ---- addends near the fixed-point quantum -----------------------------------------------------------------------------------
def test_small_gradients_against_the_fixed_point_quantum():
    """grad_scale = 2^-20 at P = 32 769: an addend of the embedding gradient's exact sums is dlogit ~ 2^-20 * 0.5 / P ~ 1e-11,
    2^24 quanta of the 2^-60 that bucket.h states (each addend is truncated to it).  The bound is derived, not fitted: with
    the kernel's own dlogit and ReLU branches, demb[n, i] = sum_c S[n, c] W0[c, i], S[n, c] = 0.5 w1[c] sum_e dlogit[e] (p = 0);
    truncation moves a list's sum by less than (entries) * 2^-60, so |error| <= (longest list) * 2^-60 * 0.5 / (1 - p) *
    sum_c |w1[c] W0[c, i]|, plus fp32 rounding: the sum's conversion and the two factors of S (3 roundings) and the 64-term
    fma chain, <= 67 * 2^-24 * sum_c |S[n, c] W0[c, i]|."""
    P, n = 32769, 1001
    c = _inputs(n, P, 81)
    c["pairs"][:2000, 0] = 7
    gs = 2.0 ** -20
    out = _run(c, gscale=gs)
    ref = _ref(c, out, gscale=gs)
    e = _errors(out, ref)
    for k in ("logits", "loss"):
        assert e[k] < FWD_BAR
    assert e["hid"] < FWD_BAR
    for k in ("dlogit", ) + GRADS:     # fp32 products scale with grad_scale: the plain bar holds
        assert e[k] < GRAD_BAR, f"small gradients: {k} rel-inf {e[k]:.3e}"
    assert float(out["dlogit"].abs().max()) < 2.0 ** -34
    mask, dl = (out["hid"] > 0).double(), out["dlogit"].double()
    T = torch.zeros(n, H, dtype=torch.float64)
    for side in (0, 1):
        T.index_add_(0, c["pairs"][:, side], mask * dl.reshape(-1, 1))
    W0, w1 = c["W0"].double(), c["w1"].double()
    S = 0.5 * T * w1
    exact = S @ W0
    longest = int(torch.bincount(c["pairs"].reshape(-1), minlength=n).max())
    assert longest >= 2000
    bound = longest * 2.0 ** -60 * 0.5 * (w1.abs() @ W0.abs()) + 67 * 2.0 ** -24 * (S.abs() @ W0.abs())
    err = (out["demb"].double() - exact).abs()
    worst = float((err / bound).max())
    print(f"pair head small gradients: demb |err| max {float(err.max()):.3e} (largest entry {float(exact.abs().max()):.3e}), "
          f"worst err / bound {worst:.3f}, longest list {longest}, vs fp64 end to end: {e}")
    record_parity("pair_head/small_gradients", demb_abs_err=float(err.max()), demb_max=float(exact.abs().max()),
                  worst_err_over_bound=worst, **e)
    assert bool((err <= bound).all())
    assert float(exact.abs().max()) > 0 and rel_inf(exact, ref["demb"]) < GRAD_BAR  # the closed form is the fp64 statement's


# ---- the reported workspace size --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1001])
@pytest.mark.parametrize("P", [1, 257, 32769])
def test_workspace_of_exactly_the_reported_size(n, P):
    """ws = exactly glass_pair_head_ws_bytes(n, P) bytes, 16-B aligned, between 4 KiB of canary bytes (every caller in the
    project allocates 16 more): forward then backward leave the canaries alone (_run) and the results match fp64 at the plain
    bars, with one exception.  n = 1 runs on _single_node_inputs; there a slab's weight gradient is a chain of 256 fp32 fmas
    over addends that take two values (dlogit is a or b, the pooled row is one row), so the roundings along the chain are
    correlated and add up instead of averaging out.  Measured on an MI355X: the canaries are intact in all six cases; n = 1,
    P = 257: dW0 2.38e-6 against the bar of 2e-6, fp32 statement on the CPU 7.3e-7 (it loses 2.4e-6 in demb and 3.2e-6 in dw1
    of the same case, where the kernel has 2.0e-7 and 2.3e-7), so dW0 of that case alone may be within 4 x the fp32
    statement's error, 2.9e-6.  Every other quantity of every case is under its plain bar: n = 1, P = 32 769 dW0 1.52e-6,
    all else under 4.2e-7."""
    c = _single_node_inputs(P, 91 + P) if n == 1 else _inputs(n, P, 91 + P)
    out = _run(c)
    ref = _ref(c, out)
    if (n, P) == (1, 257):
        _compare(f"ws_exact_n{n}_P{P}", c, out, ref, floor=_fp32_floor(c, out, ref), floor_keys=("dW0", ))
    else:
        _compare(f"ws_exact_n{n}_P{P}", c, out, ref)
