"""K7a on the GPU: glass_attn_pool_f32 / glass_attn_pool_bwd_f32 (csrc/pool_attn.hip) against the fp64 restatement
tests/attn_pool_oracle.py on both sides of every dispatch threshold, the fixed points, bitwise repeatability, the autograd
binding ops.attn_pool, and models.AttnPool through impl.train.train / impl.train.test.

Ids >= n_nodes get NO error code, although a refusal was asked for: `pos` is device memory, and an entry point cannot read
it without a host synchronisation, which the C ABI rules out (enqueue only, capturable).  They are checked where the other
pool entries check them — INSIDE the kernels, where such an entry is skipped like padding (pool.hip).
test_out_of_range_ids_are_skipped_like_padding pins that behaviour: no access outside emb / demb, bitwise the result of the
same matrix with -1 in place of the id."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import attn_pool_oracle as AO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5  # the suite's rel-inf bar
E_UNSUPPORTED = -3


def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _limits():
    lib = _lib()[1]
    return int(lib.glass_attn_pool_wave_rows()), int(lib.glass_attn_pool_stage_floats()), int(lib.glass_attn_pool_score_rows())


# ---- raw entries ---------------------------------------------------------------------------------------------------------
def _strided(a, extra):
    """`a` [R, C] on the device inside a buffer of row stride C + extra (the rest NaN: never read, never written)."""
    a = torch.as_tensor(a, dtype=torch.float32)
    buf = torch.full((a.shape[0], a.shape[1] + extra), float("nan"), dtype=torch.float32, device=DEV)
    view = buf[:, :a.shape[1]]
    view.copy_(a)
    return buf, view


def _raw_forward(emb_v, pos_d, w_d, ldo_extra=0):
    L, lib = _lib()
    n, C = emb_v.shape
    B, Smax = pos_d.shape
    out_buf = torch.full((B, C + ldo_extra), float("nan"), dtype=torch.float32, device=DEV)
    alpha = torch.full((B, Smax), float("nan"), dtype=torch.float32, device=DEV)
    rc = lib.glass_attn_pool_f32(emb_v.data_ptr(), emb_v.stride(0), pos_d.data_ptr(), B, Smax, w_d.data_ptr(), out_buf.data_ptr(),
                                 out_buf.stride(0), alpha.data_ptr(), n, C, _stream())
    L.check(rc, "glass_attn_pool_f32")
    return out_buf, out_buf[:, :C], alpha


def _raw_backward(dout_v, emb_v, pos_d, w_d, alpha, out_v, dw, acc_dw, ldde_extra=0):
    L, lib = _lib()
    n, C = emb_v.shape
    B, Smax = pos_d.shape
    demb_buf = torch.full((n, C + ldde_extra), float("nan"), dtype=torch.float32, device=DEV)  # every row must be written
    nbytes = lib.glass_attn_pool_bwd_ws_bytes(n, B, Smax, C)
    ws = torch.full((nbytes // 4 + 4, ), -1, dtype=torch.int32, device=DEV)  # (need not be initialised: junk on purpose)
    rc = lib.glass_attn_pool_bwd_f32(dout_v.data_ptr(), dout_v.stride(0), emb_v.data_ptr(), emb_v.stride(0), pos_d.data_ptr(), B, Smax,
                                     w_d.data_ptr(), alpha.data_ptr(), out_v.data_ptr(), out_v.stride(0), demb_buf.data_ptr(),
                                     demb_buf.stride(0), dw.data_ptr(), int(acc_dw), n, C, ws.data_ptr(), _stream())
    L.check(rc, "glass_attn_pool_bwd_f32")
    return demb_buf, demb_buf[:, :C]


def _inputs(seed, n, B, Smax, C, hub=False, scale=None):
    """The project's usual scale: rows of mean 0 / std 1, w with |s| <~ 3 (std 1).  Only EVEN nodes are named (half the
    nodes appear in no row); ragged rows with interior -1, row 1 all padding, row 2 names one node three times; hub: node 0
    sits in every row."""
    rng = np.random.Generator(np.random.PCG64(seed))
    emb = rng.standard_normal((n, C)).astype(np.float32)
    w = (rng.standard_normal(C) / np.sqrt(C)).astype(np.float32)
    pos = (2 * rng.integers(0, n // 2, (B, Smax))).astype(np.int64)
    if Smax > 1:
        pos[rng.random((B, Smax)) < 0.25] = -1      # padding anywhere
        pos[:, 0] = np.where(pos[:, 0] < 0, 2, pos[:, 0]) if B > 1 else pos[:, 0]
    if B >= 3:
        pos[1, :] = -1
        if Smax >= 3:
            pos[2, [0, Smax // 2, Smax - 1]] = 6
    if hub:
        pos[:, Smax // 3] = 0
        pos[1, :] = -1
    if scale is not None:  # max |s| ~ scale
        s = np.abs(emb.astype(np.float64) @ w.astype(np.float64)).max()
        w = (w * (scale / s)).astype(np.float32)
    dout = rng.standard_normal((B, C)).astype(np.float32)
    return emb, pos, w, dout


def _run_case(emb, pos, w, dout, strided):
    """Forward + backward through the raw entries -> host arrays (out, alpha, demb, dw) and the dw the call started from."""
    n, C = emb.shape
    pos_d = torch.from_numpy(pos).to(DEV)
    w_d = torch.from_numpy(w).to(DEV)
    if strided:   # lde = C + 3, strided dout / out / demb, dw accumulated over a pre-filled vector
        _eb, emb_v = _strided(emb, 3)
        _db, dout_v = _strided(dout, 5)
        dw0 = np.linspace(-2.0, 3.0, C).astype(np.float32)
        dw = torch.from_numpy(dw0.copy()).to(DEV)
        extra = (1, 2)
    else:
        emb_v, dout_v = torch.from_numpy(emb).to(DEV), torch.from_numpy(dout).to(DEV)
        dw0 = np.zeros(C, dtype=np.float32)
        dw = torch.full((C, ), float("nan"), dtype=torch.float32, device=DEV)  # overwritten
        extra = (0, 0)
    out_buf, out_v, alpha = _raw_forward(emb_v, pos_d, w_d, extra[0])
    demb_buf, demb_v = _raw_backward(dout_v, emb_v, pos_d, w_d, alpha, out_v, dw, strided, extra[1])
    torch.cuda.synchronize()
    if strided:  # the padding columns of the strided outputs were not touched
        assert bool(torch.isnan(out_buf[:, C:]).all()) and bool(torch.isnan(demb_buf[:, C:]).all())
    return out_v.cpu().numpy(), alpha.cpu().numpy(), demb_v.cpu().numpy(), dw.cpu().numpy(), dw0


def _shapes(C):
    wave, stage, score = _limits()
    rows = max(stage // C, 1)
    shapes = [(1, 1), (3, 2), (5, 63), (5, 64), (5, 65), (80, 40), (2, 300),
              (4, wave), (4, wave + 1),        # one wave per subgraph | a 256-lane workgroup
              (3, rows), (3, rows + 1),        # gathered rows resident in LDS | two-pass
              (2, score), (2, score + 1)]      # scores in LDS | in alpha
    return list(dict.fromkeys(shapes))


def test_thresholds_are_what_the_cases_assume():
    wave, stage, score = _limits()
    assert 2 <= wave < 63 and score > 300, "the fixed shapes no longer sit on both sides of the wave / score splits"
    for C in (1, 8, 17, 64, 65, 192, 512):
        sm = [s for _b, s in _shapes(C)]
        assert any(s * C <= stage for s in sm) and any(s * C > stage for s in sm)
        assert any(s <= wave for s in sm) and any(s > wave for s in sm)
        assert any(s <= score for s in sm) and any(s > score for s in sm)


@pytest.mark.parametrize("C", [1, 8, 17, 64, 65, 192, 512])
def test_forward_backward_against_the_fp64_oracle(C):
    """out, alpha, demb, dw: rel-inf <= 1e-5 against the fp64 restatement, contiguous (dw overwritten) and strided (lde = C + 3,
    strided dout / out / demb, dw accumulated over a pre-filled vector); the (80, 40) shape is the hub shape (node 0 in every
    row); odd nodes are named by no row: their demb rows are exactly 0."""
    worst = {}
    for i, (B, Smax) in enumerate(_shapes(C)):
        n = 2000 if B * Smax > 2000 else 2 * max(8, min(1000, B * Smax))
        emb, pos, w, dout = _inputs(1000 * C + i, n, B, Smax, C, hub=(B, Smax) == (80, 40))
        o64, a64, _s = AO.forward(emb, pos, w)
        d64, w64 = AO.backward(emb, pos, w, dout)
        for strided in (False, True):
            out, alpha, demb, dw, dw0 = _run_case(emb, pos, w, dout, strided)
            errs = {"out": AO.rel_inf(out, o64), "alpha": AO.rel_inf(alpha, a64), "demb": AO.rel_inf(demb, d64),
                    "dw": AO.rel_inf(dw, w64 + dw0)}
            for k, v in errs.items():
                worst[k] = max(worst.get(k, 0.0), v)
                assert v <= TOL, (C, B, Smax, strided, k, v)
            assert np.all(alpha[pos < 0] == 0) and np.all(demb[1::2] == 0), (C, B, Smax, strided)
            if B >= 3:
                assert np.all(out[1] == 0) and np.all(alpha[1] == 0)  # all padding
    print(f"attn pool C={C}: worst rel-inf {worst}")


@pytest.mark.parametrize("B,Smax,C", [(5, 65, 64), (80, 40, 17)])
def test_large_scores(B, Smax, C):
    """max |s| ~ 200: an unsubtracted softmax overflows (exp(200) > fp32's range), rows are near one-hot.  Everything stays
    finite; the fp32 score itself is only good to ~|s| 2^-24 sqrt(C), so the bound is 4 x the error of the restatement
    evaluated in fp32 against fp64 on the same inputs (floor 1e-5), computed here from the restatement alone."""
    emb, pos, w, dout = _inputs(77 + C, 400, B, Smax, C, hub=B == 80, scale=200.0)
    o64, a64, s64 = AO.forward(emb, pos, w)
    assert 150 < np.abs(s64).max() <= 201
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.exp(np.float32(np.abs(s64).max())))
    d64, w64 = AO.backward(emb, pos, w, dout)
    o32, a32, _ = AO.forward(emb, pos, w, np.float32)
    d32, w32 = AO.backward(emb, pos, w, dout, np.float32)
    out, alpha, demb, dw, _ = _run_case(emb, pos, w, dout, False)
    assert all(np.isfinite(t).all() for t in (out, alpha, demb, dw))
    for name, got, f32, f64 in (("out", out, o32, o64), ("alpha", alpha, a32, a64), ("demb", demb, d32, d64), ("dw", dw, w32, w64)):
        ref_err, err = AO.rel_inf(f32, f64), AO.rel_inf(got, f64)
        bound = max(TOL, 4 * ref_err)
        print(f"large scores B={B} Smax={Smax} C={C} {name}: kernel {err:.3e}, fp32 restatement {ref_err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, err, ref_err)
    assert float(alpha.max()) > 0.9  # near one-hot rows exist


def test_fixed_point_zero_gate_is_mean_pooling():
    from glass_amd import ops
    for (B, Smax, C) in ((5, 65, 64), (4, 7, 17), (2, 300, 8)):
        emb, pos, _w, _d = _inputs(5 + C, 600, B, Smax, C)
        e_d, p_d = torch.from_numpy(emb).to(DEV), torch.from_numpy(pos).to(DEV)
        _b, out, alpha = _raw_forward(e_d, p_d, torch.zeros(C, device=DEV))
        mean = ops.segment_pool(e_d, p_d, "mean")
        assert float((out - mean).abs().max()) <= 1e-6 * max(1.0, float(mean.abs().max()))
        cnt = (pos >= 0).sum(axis=1)
        want = np.where(pos >= 0, (np.float32(1) / np.maximum(cnt, 1).astype(np.float32))[:, None], np.float32(0)).astype(np.float32)
        assert np.array_equal(alpha.cpu().numpy().view(np.int32), want.view(np.int32)), "alpha is exactly 1 / n_b"


def test_fixed_point_single_entry_row():
    wave, _stage, _score = _limits()
    for Smax in (1, 5, wave + 9):
        for C in (17, 64, 192):
            emb, _p, w, _d = _inputs(9, 50, 4, Smax, C)
            pos = np.full((4, Smax), -1, dtype=np.int64)
            for b in range(4):
                pos[b, (3 * b) % Smax] = 7 * b + 1
            _b, out, alpha = _raw_forward(torch.from_numpy(emb).to(DEV), torch.from_numpy(pos).to(DEV), torch.from_numpy(40 * w).to(DEV))
            want = emb[pos.max(axis=1)]
            assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32)), (Smax, C)
            assert np.array_equal(alpha.cpu().numpy(), (pos >= 0).astype(np.float32))


def _bits(*tensors):
    return [t.clone().view(torch.int32) for t in tensors]


def test_repeatable_bits_on_the_hub_shape():
    """Forward + backward three times, and once more on a second stream: identical bits in out, alpha, demb, dw."""
    B, Smax, C = 80, 40, 64
    emb, pos, w, dout = _inputs(31, 400, B, Smax, C, hub=True)
    assert np.all((pos == 0).sum(axis=1)[np.arange(B) != 1] >= 1)
    e_d, p_d, w_d, g_d = (torch.from_numpy(a).to(DEV) for a in (emb, pos, w, dout))

    def once():
        _b, out, alpha = _raw_forward(e_d, p_d, w_d)
        dw = torch.empty(C, device=DEV)
        _db, demb = _raw_backward(g_d, e_d, p_d, w_d, alpha, out, dw, False)
        return _bits(out, alpha, demb, dw)

    first = once()
    for _ in range(2):
        assert all(torch.equal(a, b) for a, b in zip(first, once()))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = once()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, other))


def test_autograd_binding_equals_the_raw_entries_and_a_finite_difference():
    from glass_amd import ops
    B, Smax, C, n = 4, 5, 6, 20
    emb, pos, w, dout = _inputs(3, n, B, Smax, C)
    p_d, g_d = torch.from_numpy(pos).to(DEV), torch.from_numpy(dout).to(DEV)
    e_t = torch.from_numpy(emb).to(DEV).requires_grad_(True)
    w_t = torch.from_numpy(w.reshape(1, C)).to(DEV).requires_grad_(True)   # the module's [1, C] weight
    out, alpha = ops.attn_pool(e_t, p_d, w_t, return_alpha=True)
    assert not alpha.requires_grad
    out.backward(g_d)
    _b, r_out, r_alpha = _raw_forward(e_t.detach(), p_d, w_t.detach().reshape(-1))
    r_dw = torch.empty(C, device=DEV)
    _db, r_demb = _raw_backward(g_d, e_t.detach(), p_d, w_t.detach().reshape(-1), r_alpha, r_out, r_dw, False)
    assert tuple(w_t.grad.shape) == (1, C)
    for a, b in ((out.detach(), r_out), (alpha, r_alpha), (e_t.grad, r_demb), (w_t.grad.reshape(-1), r_dw)):
        assert torch.equal(a.view(torch.int32), b.contiguous().view(torch.int32))
    # a strided embedding view (the JK buffer's column block) takes the same route
    wide = torch.zeros((n, C + 3), device=DEV)
    wide[:, :C] = e_t.detach()
    assert torch.equal(ops.attn_pool(wide[:, :C], p_d, w_t.detach()), out.detach())
    # directional finite difference of f = <out, dout> in fp64 (the restatement) against the analytic gradients: the
    # gradients are within 1e-5 rel-inf of fp64 (the test above), so |<g32 - g64, u>| <= 1e-5 (max|g_e| sum|u_e| + max|g_w| sum|u_w|)
    rng = np.random.Generator(np.random.PCG64(8))
    u_e, u_w = rng.standard_normal((n, C)), rng.standard_normal(C)
    h = 1e-6
    f = lambda s: float((AO.forward(emb.astype(np.float64) + s * h * u_e, pos, w.astype(np.float64) + s * h * u_w)[0] * dout).sum())  # noqa: E731
    fd = (f(1.0) - f(-1.0)) / (2 * h)
    ge, gw = e_t.grad.cpu().numpy().astype(np.float64), w_t.grad.cpu().numpy().astype(np.float64).reshape(-1)
    an = float((ge * u_e).sum() + (gw * u_w).sum())
    bound = TOL * (np.abs(ge).max() * np.abs(u_e).sum() + np.abs(gw).max() * np.abs(u_w).sum()) + 1e-8
    assert abs(fd - an) <= bound, (fd, an, bound)
    assert abs(fd) > 1e-3


def test_out_of_range_ids_are_skipped_like_padding():
    """(module docstring)  An id >= n_nodes is skipped inside the kernels, exactly like -1."""
    B, Smax, C, n = 6, 9, 17, 40
    emb, pos, w, dout = _inputs(12, n, B, Smax, C)
    bad = pos.copy()
    holes = np.argwhere(pos < 0)
    assert len(holes) >= 3
    for (b, j), v in zip(holes[:3], (n, n + 5, 2 ** 40)):
        bad[b, j] = v
    got = _run_case(emb, bad, w, dout, False)
    want = _run_case(emb, pos, w, dout, False)
    for a, b in zip(got[:4], want[:4]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_device_entries_refuse_unsupported_widths_without_touching_out():
    _L, lib = _lib()
    C, B, Smax, n = 4097, 2, 3, 10
    emb = torch.zeros((n, C), device=DEV)
    pos = torch.zeros((B, Smax), dtype=torch.int64, device=DEV)
    w = torch.zeros(C, device=DEV)
    out = torch.full((B, C), 7.0, device=DEV)
    alpha = torch.full((B, Smax), 7.0, device=DEV)
    rc = lib.glass_attn_pool_f32(emb.data_ptr(), C, pos.data_ptr(), B, Smax, w.data_ptr(), out.data_ptr(), C, alpha.data_ptr(), n, C,
                                 _stream())
    assert rc == E_UNSUPPORTED and b"4097" in lib.glass_last_error_string()
    demb, dw = torch.full((n, C), 7.0, device=DEV), torch.full((C, ), 7.0, device=DEV)
    ws = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    rc = lib.glass_attn_pool_bwd_f32(out.data_ptr(), C, emb.data_ptr(), C, pos.data_ptr(), B, Smax, w.data_ptr(), alpha.data_ptr(),
                                     out.data_ptr(), C, demb.data_ptr(), C, dw.data_ptr(), 0, n, C, ws.data_ptr(), _stream())
    assert rc == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((alpha == 7.0).all()) and bool((demb == 7.0).all()) and bool((dw == 7.0).all())
    # the widest width served
    C = 4096
    e2, p2, w2, d2 = _inputs(4, 16, 2, 3, C)
    o, a, de, dwv, _ = _run_case(e2, p2, w2, d2, False)
    assert AO.rel_inf(o, AO.forward(e2, p2, w2)[0]) <= TOL
    d64, w64 = AO.backward(e2, p2, w2, d2)
    assert AO.rel_inf(de, d64) <= TOL and AO.rel_inf(dwv, w64) <= TOL


def test_empty_problems_are_no_ops_and_the_backward_zero_fills():
    from glass_amd import ops
    L, lib = _lib()
    n, C = 12, 8
    emb = torch.randn((n, C), device=DEV)
    w = torch.randn(C, device=DEV)
    for B, Smax in ((0, 4), (3, 0)):
        pos = torch.zeros((B, Smax), dtype=torch.int64, device=DEV)
        out = torch.full((max(B, 1), C), 7.0, device=DEV)
        alpha = torch.full((max(B * Smax, 1), ), 7.0, device=DEV)
        assert lib.glass_attn_pool_f32(emb.data_ptr(), C, pos.data_ptr(), B, Smax, w.data_ptr(), out.data_ptr(), C, alpha.data_ptr(), n,
                                       C, _stream()) == 0
        demb = torch.full((n, C), float("nan"), device=DEV)
        dw = torch.full((C, ), 5.0, device=DEV)
        ws = torch.zeros(64, dtype=torch.int32, device=DEV)
        for acc, want in ((1, 5.0), (0, 0.0)):
            L.check(lib.glass_attn_pool_bwd_f32(out.data_ptr(), C, emb.data_ptr(), C, pos.data_ptr(), B, Smax, w.data_ptr(),
                                                alpha.data_ptr(), out.data_ptr(), C, demb.data_ptr(), C, dw.data_ptr(), acc, n, C,
                                                ws.data_ptr(), _stream()), "glass_attn_pool_bwd_f32")
            torch.cuda.synchronize()
            assert bool((demb == 0).all()) and bool((dw == want).all())
        assert bool((out == 7.0).all())
        pooled = ops.attn_pool(emb, pos, w)   # the binding hands back zeros of the right shape
        assert tuple(pooled.shape) == (B, C) and bool((pooled == 0).all())


# ---- through the model ----------------------------------------------------------------------------------------------------
def _build(hidden, layers, max_deg, n_class, pool):
    """GLASSTest.build_model's construction (jk = 1) with the readout `pool` ("attn": gate perturbed off its zero start)."""
    from impl import models
    conv = models.EmbZGConv(hidden, hidden, layers, max_deg=max_deg, activation=nn.ELU(inplace=True), jk=True, dropout=0.0,
                            conv=functools.partial(models.GLASSConv, aggr="mean", z_ratio=0.9, dropout=0.0), gn=True)
    width = hidden * layers
    head = nn.Linear(width, n_class)
    pool_fn = models.AttnPool(width) if pool == "attn" else models.MeanPool()
    if pool == "attn":
        with torch.no_grad():
            pool_fn.gate.weight.normal_(0.0, 0.05)
    return models.GLASS(conv, nn.ModuleList([head]), nn.ModuleList([pool_fn])).to(DEV)


def _tiny(seed, n_batches):
    from glass_amd import synth
    from impl import config
    config.set_device(0)
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=seed, n_batches=n_batches)
    pos = pos.copy()
    pos[::3, -2:] = -1
    return (w, ) + tuple(torch.from_numpy(a).to(DEV) for a in (x, ei, ew, pos, y))


def _loader(ds, bs, drop_last=True):
    from impl import SubGDataset, utils
    return SubGDataset.ZGDataloader(ds, bs, z_fn=utils.MaxZOZ, shuffle=False, drop_last=drop_last)


def test_model_with_attn_pool_trains_on_the_captured_step_like_an_eager_twin():
    """Three Adam steps through impl.train.train (the TrainStep's per-op form: stack node, attn pool, fused head + loss,
    captured) against a deep copy stepped eagerly with the reference's loop; losses at the tolerance the twin comparisons of
    tests/test_gpu_reference_caller.py:153 use (2e-4 relative).  The gate weight moves and lives in the arena."""
    from impl import SubGDataset, train
    from glass_amd import stack
    w, x, ei, ew, pos, y = _tiny(2, 3)
    torch.manual_seed(4)
    gnn = _build(64, 2, int(x.max()), w.n_class, "attn")
    twin = copy.deepcopy(gnn)
    loss_fn = nn.CrossEntropyLoss()
    opt, opt_twin = torch.optim.Adam(gnn.parameters(), lr=5e-3), torch.optim.Adam(twin.parameters(), lr=5e-3)
    gate0 = gnn.pools[0].gate.weight.detach().clone()
    bs = w.batch
    for k in range(3):
        ds = SubGDataset.GDataset(x, ei, ew, pos[bs * k:bs * k + bs], y[bs * k:bs * k + bs])
        got = train.train(opt, gnn, _loader(ds, bs), loss_fn)
        twin.train()
        for batch in _loader(ds, bs):
            opt_twin.zero_grad()
            loss = loss_fn(twin(*batch[:-1], id=0), batch[-1])
            loss.backward()
            opt_twin.step()
        want = loss.item()
        assert abs(got - want) <= 2e-4 * abs(want), (k, got, want)
    steps = gnn.__dict__.get("_glass_train_steps") or {}
    assert len(steps) == 1
    step = next(iter(steps.values()))
    gnn.train()
    assert step.graphed and not step._program_step() and not stack.step_supported(gnn, loss_fn)
    gate = gnn.pools[0].gate.weight
    assert float((gate.detach() - gate0).abs().max()) > 1e-4, "the gate weight did not move"
    arena = gnn._glass_grad_bucket
    lo = arena.flat_param.data_ptr()
    assert lo <= gate.data_ptr() and gate.data_ptr() + 4 * gate.numel() <= lo + 4 * arena.flat_param.numel()
    glo = arena.flat.data_ptr()
    assert gate.grad is not None and glo <= gate.grad.data_ptr() < glo + 4 * arena.flat.numel()
    assert any(p is gate for p in arena.params)
    # deep copy: a plain model with the same state
    clone = copy.deepcopy(gnn)
    sd, sd2 = gnn.state_dict(), clone.state_dict()
    assert list(sd) == list(sd2) and "pools.0.gate.weight" in sd and all(torch.equal(sd[k], sd2[k]) for k in sd)
    cg = clone.pools[0].gate.weight
    assert not (lo <= cg.data_ptr() < lo + 4 * arena.flat_param.numel())


def test_evaluation_graph_replays_the_attn_pool(monkeypatch):
    """impl.train.test through evalstep.EvalGraph (parallel branches, one replay) == module-by-module evaluation, bit for bit."""
    from impl import SubGDataset, train, metrics
    from glass_amd import train as gtrain
    w, x, ei, ew, pos, y = _tiny(3, 4)
    torch.manual_seed(5)
    gnn = _build(64, 2, int(x.max()), w.n_class, "attn")
    ds = SubGDataset.GDataset(x, ei, ew, pos, y)
    loss_fn = nn.CrossEntropyLoss()
    seen = {}
    real = metrics.microf1

    def spy(pred, yy):
        seen["pred"] = np.array(pred, copy=True)
        return real(pred, yy)

    monkeypatch.setattr(gtrain, "USE_EVAL_METRICS", False)  # the metric sees the predictions on the host
    outs = []
    for use_graph in (True, False):
        monkeypatch.setattr(gtrain, "USE_EVAL_GRAPH", use_graph)
        score, loss = train.test(gnn, _loader(ds, w.batch, drop_last=False), spy, loss_fn)
        outs.append((seen["pred"], score, float(loss)))
    graphs = gnn.__dict__.get("_glass_eval_graphs") or {}
    assert len(graphs) >= 1 and all(g is not None for g in graphs.values()), "the evaluation graph was not captured"
    assert np.array_equal(outs[0][0].view(np.int32), outs[1][0].view(np.int32))
    assert outs[0][1:] == outs[1][1:]
