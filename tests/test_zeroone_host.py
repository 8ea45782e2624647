"""Host side of the exact zero-one labels (utils.ZeroOneZ, csrc/labels_rep.hip, spmm_rep.hip, graphnorm_rep.hip) — no GPU:
ZeroOneZ against a numpy restatement, the driver's flags, the new symbols of the C ABI and the argument checks of the three
entries, which answer with codes before anything is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch

import zeroone_oracle as ZO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_PLAN, E_UNSUPPORTED = -1, -2, -3


# ---- 1. ZeroOneZ -----------------------------------------------------------------------------------------------------------
def test_zeroonez_equals_numpy_restatement():
    from impl import utils
    assert utils.ZeroOneZ is __import__("glass_amd.utils", fromlist=["ZeroOneZ"]).ZeroOneZ
    n = 9
    pos = np.array([[0, 2, 3, -1], [1, 4, 4, 4], [-1, -1, -1, -1], [8, -1, 9, 12], [7, 7, -1, 0]], dtype=np.int64)
    x = torch.zeros(n, 1, 1)
    z = utils.ZeroOneZ(x, torch.from_numpy(pos))
    assert z.dtype == torch.int64 and tuple(z.shape) == (5, n)
    assert np.array_equal(z.numpy(), ZO.zeroone_z(n, pos))
    assert z[2].sum() == 0                                   # an all-padding row
    assert z[1].sum() == 2 and z[3].tolist() == [0] * 8 + [1]  # duplicates once; ids >= N skipped
    one = utils.ZeroOneZ(x, torch.from_numpy(pos[:1]))       # B = 1: MaxZOZ's labels as a [1, N] row
    assert tuple(one.shape) == (1, n) and one[0].tolist() == [1, 0, 1, 1, 0, 0, 0, 0, 0]
    with pytest.raises(ValueError):
        utils.ZeroOneZ(x, torch.from_numpy(pos[0]))


def test_driver_flags_are_mutually_exclusive():
    import GLASSTest
    a = GLASSTest.parse_args(["--use_one", "--use_zeroone"])
    assert a.use_zeroone and not a.use_maxzeroone
    assert not GLASSTest.parse_args(["--use_one", "--use_maxzeroone"]).use_zeroone
    with pytest.raises(SystemExit):
        GLASSTest.parse_args(["--use_one", "--use_zeroone", "--use_maxzeroone"])


def test_batched_z_no_longer_refused_on_shape():
    """z [B, N] with B > 1 used to raise ValueError("z must hold one label per node"); now it reaches the kernels (which, on a
    machine without a GPU, refuse the CPU tensor)."""
    import torch.nn as nn
    from glass_amd import models
    from glass_amd._lib import GlassHipError
    emb = models.EmbZGConv(8, 8, 1, max_deg=3, activation=nn.ELU(inplace=True))
    assert emb.replica_chunk is None
    x = torch.zeros(6, 1, dtype=torch.int64)
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(GlassHipError):
        emb(x, ei, torch.ones(2), torch.zeros(3, 6, dtype=torch.int64))
    with pytest.raises(ValueError):  # a z that is neither [N] nor [B, N] is still refused
        emb(x, ei, torch.ones(2), torch.zeros(3, 5, dtype=torch.int64))


def test_replicas_marker():
    from glass_amd import ops
    r = ops.Replicas(3, 7, 2)
    assert (r.R, r.N, r.rep0) == (3, 7, 2)
    for bad in ((0, 7, 0), (3, 0, 0), (3, 7, -1)):
        with pytest.raises(ValueError):
            ops.Replicas(*bad)


# ---- 2. the C ABI ----------------------------------------------------------------------------------------------------------
def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


NEW = ("glass_zeroone_labels_u8", "glass_spmm_rep_max_replicas", "glass_spmm_rep_ws_bytes", "glass_spmm_csr_rep_f32",
       "glass_graphnorm_rep_max_replicas", "glass_graphnorm_rep_row_block", "glass_graphnorm_rep_ws_bytes",
       "glass_graphnorm_rep_fwd_f32", "glass_graphnorm_rep_bwd_f32")


def test_symbols_and_header():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES and (name + "(") in header, name
    assert lib.glass_version() == L.ABI_VERSION == 6  # purely additive
    assert lib.glass_spmm_rep_max_replicas() == lib.glass_graphnorm_rep_max_replicas() == 65535
    assert lib.glass_graphnorm_rep_row_block(64, 1) == 128 and lib.glass_graphnorm_rep_row_block(17, 0) == 64
    assert lib.glass_graphnorm_rep_row_block(0, 1) == E_ARG


def test_labels_argument_checks():
    _L, lib = _lib()
    pos = np.full((4, 3), -1, dtype=np.int64)
    mask = np.full(4 * 10, 7, dtype=np.uint8)
    names = ["pos", "B", "Smax", "rep0", "R", "n_nodes", "mask"]
    good = [pos.ctypes.data, 4, 3, 1, 2, 10, mask.ctypes.data]

    def call(**edit):
        args = list(good)
        for k, v in edit.items():
            args[names.index(k)] = v
        return lib.glass_zeroone_labels_u8(*args, None)

    assert call(pos=None) == E_ARG and call(mask=None) == E_ARG
    assert b"null" in lib.glass_last_error_string()
    assert call(B=-1) == E_ARG and call(Smax=-1) == E_ARG and call(n_nodes=-1) == E_ARG and call(n_nodes=1 << 31) == E_ARG
    assert call(rep0=-1) == E_ARG and call(R=-1) == E_ARG
    assert call(rep0=3, R=2) == E_ARG and call(rep0=5, R=0) == E_ARG   # rows outside pos
    assert b"inside pos" in lib.glass_last_error_string()
    assert call(pos=pos.ctypes.data + 4) == E_ARG and b"misaligned" in lib.glass_last_error_string()
    assert call(R=0, mask=None) == 0 and call(n_nodes=0, mask=None) == 0   # nothing to label: no launch
    assert np.all(mask == 7)


def _plan(rowptr):
    _L, lib = _lib()
    rp = np.ascontiguousarray(rowptr, dtype=np.int32)
    words = ctypes.c_int64(0)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, len(rp) - 1, None, ctypes.byref(words)) == 0
    plan = np.zeros(words.value, dtype=np.int32)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, len(rp) - 1, plan.ctypes.data, ctypes.byref(words)) == 0
    return rp, plan


def test_spmm_rep_argument_checks_and_workspace():
    L, lib = _lib()
    n, H = 6, 8
    rp, plan = _plan([0, 1, 2, 3, 4, 5, 6])
    col = np.zeros(6, dtype=np.int32)
    val = np.zeros(6, dtype=np.float32)
    X = np.zeros((3 * n, H), dtype=np.float32)
    Y = np.full((3 * n, H), 5, dtype=np.float32)
    names = ["rowptr", "col", "val", "X", "ldx", "xs", "Y", "ldy", "ys", "n_rows", "H", "R", "hdr", "plan", "ws"]
    good = [rp.ctypes.data, col.ctypes.data, val.ctypes.data, X.ctypes.data, H, n, Y.ctypes.data, H, n, n, H, 3,
            plan.ctypes.data, plan.ctypes.data, None]

    def call(**edit):
        args = list(good)
        for k, v in edit.items():
            args[names.index(k)] = v
        return lib.glass_spmm_csr_rep_f32(*args, None)

    for ptr in ("rowptr", "X", "Y", "hdr", "plan", "col", "val"):
        assert call(**{ptr: None}) == E_ARG, ptr
        assert b"null" in lib.glass_last_error_string()
    assert call(H=0) == E_ARG and call(ldx=H - 1) == E_ARG and call(ldy=H - 1) == E_ARG
    assert call(R=-1) == E_ARG and call(xs=-1) == E_ARG and call(ys=n - 1) == E_ARG
    assert call(n_rows=n - 1) == E_PLAN
    bad = plan.copy()
    bad[0] = 0
    assert call(hdr=bad.ctypes.data) == E_PLAN
    limit = lib.glass_spmm_rep_max_replicas()
    assert call(R=limit + 1) == E_UNSUPPORTED and str(limit).encode() in lib.glass_last_error_string()
    assert call(R=2, xs=1 << 45, ys=1 << 45) == E_UNSUPPORTED and str(1 << 47).encode() in lib.glass_last_error_string()
    assert call(R=0) == 0   # no replica: no launch
    assert np.all(Y == 5)
    # a plan with partial rows needs ws, R times the single product's
    deg = [600] + [1] * 5
    rp2, plan2 = _plan(np.concatenate([[0], np.cumsum(deg)]))
    assert plan2[7] > 0  # H_NSLOTS
    single = lib.glass_spmm_ws_bytes(plan2.ctypes.data, H)
    assert single > 0 and lib.glass_spmm_rep_ws_bytes(plan2.ctypes.data, H, 5) == 5 * single
    assert lib.glass_spmm_rep_ws_bytes(plan2.ctypes.data, H, 0) == 0
    assert lib.glass_spmm_rep_ws_bytes(None, H, 1) == E_PLAN and lib.glass_spmm_rep_ws_bytes(plan2.ctypes.data, 0, 1) == E_ARG
    assert call(rowptr=rp2.ctypes.data, hdr=plan2.ctypes.data, plan=plan2.ctypes.data) == E_ARG
    assert b"ws is null" in lib.glass_last_error_string()


def test_graphnorm_rep_argument_checks_and_workspace():
    _L, lib = _lib()
    N, C, R = 5, 8, 2
    f = lambda *s: np.zeros(s, dtype=np.float32)  # noqa: E731
    x, y, g, b, a, saved = f(R * N, C), f(R * N, C), f(C), f(C), f(C), f(R * 4 * C)
    ws = np.zeros(lib.glass_graphnorm_rep_ws_bytes(N, C, R) // 8 + 1, dtype=np.float64)
    rng = np.zeros(2, dtype=np.uint64)
    names = ["x", "ldx", "y", "ldy", "n_rows", "C", "R", "rep0", "gamma", "beta", "alpha", "eps", "saved", "act", "p_drop",
             "rng", "call_id", "ws"]
    good = [x.ctypes.data, C, y.ctypes.data, C, N, C, R, 0, g.ctypes.data, b.ctypes.data, a.ctypes.data, 1e-5,
            saved.ctypes.data, 0, 0.0, None, 1, ws.ctypes.data]

    def fwd(**edit):
        args = list(good)
        for k, v in edit.items():
            args[names.index(k)] = v
        return lib.glass_graphnorm_rep_fwd_f32(*args, None)

    for ptr in ("x", "y", "gamma", "beta", "alpha", "saved", "ws"):
        assert fwd(**{ptr: None}) == E_ARG, ptr
        assert b"null" in lib.glass_last_error_string()
    assert fwd(ldx=C - 1) == E_ARG and fwd(ldy=C - 1) == E_ARG
    assert fwd(n_rows=0) == E_ARG and fwd(C=0, ldx=0, ldy=0) == E_ARG and fwd(R=-1) == E_ARG and fwd(rep0=-1) == E_ARG
    assert fwd(p_drop=0.5) == E_ARG and fwd(p_drop=1.0, rng=rng.ctypes.data) == E_ARG and fwd(act=9) == E_ARG
    assert fwd(ws=ws.ctypes.data + 4) == E_ARG and b"misaligned" in lib.glass_last_error_string()
    limit = lib.glass_graphnorm_rep_max_replicas()
    assert fwd(R=limit + 1) == E_UNSUPPORTED and str(limit).encode() in lib.glass_last_error_string()
    assert fwd(R=0) == 0   # no replica: no launch

    dy, dx, dparams = f(R * N, C), f(R * N, C), f(3, C)
    bnames = ["dy", "lddy", "x", "ldx", "dx", "lddx", "addend", "ldadd", "n_rows", "C", "R", "rep0", "gamma", "alpha", "saved",
              "dgamma", "dbeta", "dalpha", "accumulate", "act", "p_drop", "rng", "call_id", "ws"]
    bgood = [dy.ctypes.data, C, x.ctypes.data, C, dx.ctypes.data, C, None, 0, N, C, R, 0, g.ctypes.data, a.ctypes.data,
             saved.ctypes.data, dparams[0].ctypes.data, dparams[1].ctypes.data, dparams[2].ctypes.data, 0, 0, 0.0, None, 1,
             ws.ctypes.data]

    def bwd(**edit):
        args = list(bgood)
        for k, v in edit.items():
            args[bnames.index(k)] = v
        return lib.glass_graphnorm_rep_bwd_f32(*args, None)

    for ptr in ("dy", "x", "dx", "gamma", "alpha", "saved", "ws"):
        assert bwd(**{ptr: None}) == E_ARG, ptr
    for ld in ("lddy", "ldx", "lddx"):
        assert bwd(**{ld: C - 1}) == E_ARG, ld
    assert bwd(addend=x.ctypes.data, ldadd=C - 1) == E_ARG
    assert bwd(n_rows=0) == E_ARG and bwd(R=-1) == E_ARG and bwd(rep0=-1) == E_ARG and bwd(act=9) == E_ARG
    assert bwd(p_drop=0.5) == E_ARG and bwd(ws=ws.ctypes.data + 4) == E_ARG
    assert bwd(R=limit + 1) == E_UNSUPPORTED
    # the workspace query: host arithmetic; R chunks of the whole-graph entry's scratch plus the per-replica gradient terms
    size, single = lib.glass_graphnorm_rep_ws_bytes, lib.glass_graphnorm_ws_bytes
    assert size(N, C, 0) == 0 and size(N, 0, 1) == E_ARG and size(N, C, -1) == E_ARG
    for c in (8, 17, 192):
        for r in (1, 3):
            assert size(N, c, r) == r * (single(N, c) + 3 * c * 8) and size(N, c, r) % 8 == 0
