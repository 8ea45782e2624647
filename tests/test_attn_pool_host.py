"""Host side of K7a, attention pooling (glass_amd/csrc/pool_attn.hip, ops.attn_pool, models.AttnPool) — no GPU:
the restatement tests/attn_pool_oracle.py against a torch autograd composition on the CPU, the module / driver surface,
and the argument checks of the three entry points, which answer with codes before anything is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import attn_pool_oracle as AO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_UNSUPPORTED = -1, -3


# ---- 1. the oracle against torch autograd --------------------------------------------------------------------------------
def _case(seed, n=23, B=6, Smax=7, C=5):
    rng = np.random.Generator(np.random.PCG64(seed))
    emb = rng.standard_normal((n, C))
    w = rng.standard_normal(C) * 0.8
    pos = rng.integers(0, n, (B, Smax)).astype(np.int64)
    pos[0, [1, 4]] = -1            # interior padding
    pos[1, :] = -1                 # an all-padding row
    pos[2, [0, 3, 5]] = 11         # one node three times in a row
    pos[3, 2:] = -1                # padding at the end
    pos[4, 1:] = -1                # a single valid entry
    pos[4, 0] = 11                 # ... naming the repeated node (several rows share it)
    dout = rng.standard_normal((B, C))
    return emb, pos, w, dout


def _torch_composition(emb, pos, w, dout):
    """softmax(emb[valid] @ w) @ emb[valid] per row with torch's own ops, gradients by autograd (fp64)."""
    e = torch.tensor(emb, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    rows, alphas = [], []
    for b in range(pos.shape[0]):
        js = np.nonzero(pos[b] >= 0)[0]
        a_row = torch.zeros(pos.shape[1], dtype=torch.float64)
        if js.size == 0:
            rows.append(torch.zeros(emb.shape[1], dtype=torch.float64))
        else:
            x = e[torch.from_numpy(pos[b, js])]
            a = torch.softmax(x @ wt, dim=0)
            rows.append(a @ x)
            a_row[torch.from_numpy(js)] = a.detach()
        alphas.append(a_row)
    out = torch.stack(rows)
    out.backward(torch.tensor(dout, dtype=torch.float64))
    return out.detach().numpy(), torch.stack(alphas).numpy(), e.grad.numpy(), wt.grad.numpy()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_oracle_equals_torch_autograd(seed):
    emb, pos, w, dout = _case(seed)
    out, alpha, _s = AO.forward(emb, pos, w)
    demb, dw = AO.backward(emb, pos, w, dout)
    t_out, t_alpha, t_demb, t_dw = _torch_composition(emb, pos, w, dout)
    for name, got, want in (("out", out, t_out), ("alpha", alpha, t_alpha), ("demb", demb, t_demb), ("dw", dw, t_dw)):
        err = AO.rel_inf(got, want)
        assert err <= 1e-12, (name, err)
    assert np.all(out[1] == 0) and np.all(alpha[1] == 0)            # all padding
    assert np.all(alpha[pos < 0] == 0)
    assert np.array_equal(out[4], emb[11]) and alpha[4, 0] == 1.0   # one valid entry: the node's row itself
    assert np.allclose(alpha.sum(axis=1)[[0, 2, 3, 4, 5]], 1.0, rtol=0, atol=1e-15)
    named = np.unique(pos[pos >= 0])
    assert np.all(demb[np.setdiff1d(np.arange(emb.shape[0]), named)] == 0)


def test_oracle_zero_gate_is_mean_pooling_and_bias_cancels():
    emb, pos, w, dout = _case(3)
    out, alpha, _s = AO.forward(emb, pos, np.zeros_like(w))
    for b in range(pos.shape[0]):
        js = np.nonzero(pos[b] >= 0)[0]
        if js.size:
            assert np.all(alpha[b, js] == 1.0 / js.size)
            assert np.allclose(out[b], emb[pos[b, js]].mean(axis=0), rtol=0, atol=1e-15)
    # a gate bias adds one number to every score of a row: the same weights, so no gradient — why the module has none
    emb1 = np.concatenate([emb, np.ones((emb.shape[0], 1))], axis=1)
    _o, a_bias, _ = AO.forward(emb1, pos, np.concatenate([w, [3.7]]))
    assert AO.rel_inf(a_bias, AO.forward(emb, pos, w)[1]) <= 1e-14


def test_oracle_fp32_mode_is_fp32():
    emb, pos, w, dout = _case(4)
    out32, a32, _ = AO.forward(emb, pos, w, np.float32)
    d32, w32 = AO.backward(emb, pos, w, dout, np.float32)
    assert all(t.dtype == np.float32 for t in (out32, a32, d32, w32))
    out64 = AO.forward(emb, pos, w)[0]
    assert 0 < AO.rel_inf(out32, out64) < 1e-5


# ---- 2. module and driver surface ---------------------------------------------------------------------------------------
def test_attn_pool_module_surface():
    from glass_amd import models
    pool = models.AttnPool(24)
    assert isinstance(pool, models.PoolModule) and pool.mode == "attn" and models.AttnPool.mode == "attn"
    assert pool.trans_fn is None
    sd = pool.state_dict()
    assert list(sd) == ["gate.weight"] and tuple(sd["gate.weight"].shape) == (1, 24)
    assert isinstance(pool.gate, nn.Linear) and pool.gate.bias is None
    assert torch.count_nonzero(sd["gate.weight"]) == 0, "the gate starts at zero: mean pooling"
    assert pool.gate.weight.requires_grad
    fn = nn.Identity()
    assert models.AttnPool(8, trans_fn=fn).trans_fn is fn


def _driver_run(monkeypatch, n_out=3):
    """GLASSTest.Run without loading a dataset: what build_model reads of it."""
    import GLASSTest
    from impl import config
    monkeypatch.setattr(config, "device", torch.device("cpu"))  # (undone after the test: the selector is process-wide)
    run = GLASSTest.Run.__new__(GLASSTest.Run)
    run.args = GLASSTest.parse_args(["--use_one", "--pool", "attn"])
    run.max_deg, run.output_channels = torch.tensor(1), n_out
    return run


@pytest.mark.parametrize("jk", [0, 1])
def test_driver_builds_attn_pool_at_the_pooled_width(monkeypatch, jk):
    import GLASSTest
    from glass_amd import models, stack
    run = _driver_run(monkeypatch)
    assert "attn" in GLASSTest.POOLS and GLASSTest.POOLS["attn"] is models.AttnPool
    assert run.args.pool == "attn" and GLASSTest.parse_args(["--use_one"]).pool is None
    with pytest.raises(SystemExit):
        GLASSTest.parse_args(["--pool", "median"])
    hidden, layers = 64, 3
    gnn = run.build_model(hidden, layers, 0.0, jk, run.args.pool, 0.9, "mean")
    pool, head = gnn.pools[0], gnn.preds[0]
    width = hidden * layers if jk else hidden
    assert type(pool) is models.AttnPool
    assert tuple(pool.gate.weight.shape) == (1, width) and head.weight.shape[1] == width
    assert "pools.0.gate.weight" in gnn.state_dict()
    assert any(p is pool.gate.weight for p in gnn.parameters())   # what ParamArena / Adam collect
    gnn.train()
    assert stack.step_supported(gnn, nn.CrossEntropyLoss()) is False
    # the other pools are built as before (no argument)
    assert type(run.build_model(hidden, layers, 0.0, jk, "mean", 0.9, "mean").pools[0]) is models.MeanPool
    with pytest.raises(NotImplementedError):
        run.build_model(hidden, layers, 0.0, jk, "median", 0.9, "mean")


# ---- 3. the C ABI's argument checks --------------------------------------------------------------------------------------
def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def test_symbols_prototypes_and_header():
    L, lib = _lib()
    c, P, I = ctypes, ctypes.c_void_p, ctypes.c_int64
    assert L.SIGNATURES["glass_attn_pool_f32"] == (c.c_int, [P, I, P, I, I, P, P, I, P, I, I, P])
    assert L.SIGNATURES["glass_attn_pool_bwd_ws_bytes"] == (c.c_int64, [I, I, I, I])
    assert L.SIGNATURES["glass_attn_pool_bwd_f32"] == (c.c_int, [P, I, P, I, P, I, I, P, P, P, I, P, I, P, c.c_int, I, I, P, P])
    header = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    for name in ("glass_attn_pool_f32", "glass_attn_pool_bwd_ws_bytes", "glass_attn_pool_bwd_f32", "glass_attn_pool_wave_rows",
                 "glass_attn_pool_stage_floats", "glass_attn_pool_score_rows"):
        assert hasattr(lib, name) and name in L.SIGNATURES and (name + "(") in header
    block = header[header.index("K7a attention pooling"):header.index("glass_attn_pool_wave_rows(void)")]
    assert "impl/models.py:275-319" in block and "impl/models.py:346-350" in block
    assert lib.glass_version() == L.ABI_VERSION == 6  # purely additive
    wave, stage, score = lib.glass_attn_pool_wave_rows(), lib.glass_attn_pool_stage_floats(), lib.glass_attn_pool_score_rows()
    assert 1 <= wave < score and stage >= 4096 and stage * 4 + score * 4 <= 60 * 1024  # (LDS of one workgroup: under 64 KiB)


def _host_buffers(n=8, C=4, B=2, Smax=3):
    """Host memory that never reaches a kernel: every call below is refused before its launch."""
    f = lambda *s: np.zeros(s, dtype=np.float32)  # noqa: E731
    return dict(emb=f(n, C + 4), pos=np.zeros((B, Smax), dtype=np.int64), w=f(C + 4), out=f(B, C + 4), alpha=f(B, Smax),
                dout=f(B, C + 4), demb=f(n, C + 4), dw=f(C + 4), ws=np.zeros(4096, dtype=np.int32))


def test_forward_argument_checks():
    _L, lib = _lib()
    h = _host_buffers()
    p = {k: v.ctypes.data for k, v in h.items()}
    n, C, B, Smax = 8, 4, 2, 3
    good = [p["emb"], C, p["pos"], B, Smax, p["w"], p["out"], C, p["alpha"], n, C]

    def call(**edit):
        names = ["emb", "lde", "pos", "B", "Smax", "w", "out", "ldo", "alpha", "n_nodes", "C"]
        args = list(good)
        for k, v in edit.items():
            args[names.index(k)] = v
        return lib.glass_attn_pool_f32(*args, None)

    for ptr in ("emb", "pos", "w", "out", "alpha"):
        assert call(**{ptr: None}) == E_ARG, ptr
        assert b"null" in lib.glass_last_error_string()
    assert call(C=4097, lde=4097, ldo=4097) == E_UNSUPPORTED
    assert b"4097" in lib.glass_last_error_string()
    assert call(C=0) == E_ARG
    assert call(lde=C - 1) == E_ARG and call(ldo=C - 1) == E_ARG
    assert call(B=-1) == E_ARG and call(Smax=-1) == E_ARG and call(n_nodes=-1) == E_ARG
    assert call(emb=p["emb"] + 2) == E_ARG and b"misaligned" in lib.glass_last_error_string()
    assert call(pos=p["pos"] + 4) == E_ARG and b"misaligned" in lib.glass_last_error_string()
    assert call(B=1 << 20, Smax=1 << 10) == E_ARG   # 2^30 entries
    # nothing to do is not an error, and nothing is launched (the output pointers may then be anything)
    assert call(B=0, out=None, alpha=None) == 0
    assert call(Smax=0, alpha=None) == 0
    assert not h["out"].any()


def test_backward_argument_checks_and_workspace_size():
    _L, lib = _lib()
    h = _host_buffers()
    p = {k: v.ctypes.data for k, v in h.items()}
    n, C, B, Smax = 8, 4, 2, 3
    names = ["dout", "ldd", "emb", "lde", "pos", "B", "Smax", "w", "alpha", "out", "ldo", "demb", "ldde", "dw", "acc_dw",
             "n_nodes", "C", "ws"]
    good = [p["dout"], C, p["emb"], C, p["pos"], B, Smax, p["w"], p["alpha"], p["out"], C, p["demb"], C, p["dw"], 0, n, C, p["ws"]]

    def call(**edit):
        args = list(good)
        for k, v in edit.items():
            args[names.index(k)] = v
        return lib.glass_attn_pool_bwd_f32(*args, None)

    for ptr in ("dout", "emb", "pos", "w", "alpha", "out", "demb", "dw", "ws"):
        assert call(**{ptr: None}) == E_ARG, ptr
        assert b"null" in lib.glass_last_error_string()
    assert call(C=4097, ldd=4097, lde=4097, ldo=4097, ldde=4097) == E_UNSUPPORTED
    for ld in ("ldd", "lde", "ldo", "ldde"):
        assert call(**{ld: C - 1}) == E_ARG, ld
    assert call(B=-1) == E_ARG and call(Smax=-2) == E_ARG and call(n_nodes=-1) == E_ARG and call(C=0) == E_ARG
    assert call(ws=p["ws"] + 4) == E_ARG and b"misaligned" in lib.glass_last_error_string()
    assert call(dw=p["dw"] + 1) == E_ARG and b"misaligned" in lib.glass_last_error_string()
    # the workspace query: pure host arithmetic, 0 for an empty problem, monotone in every argument, 16-byte granular
    size = lib.glass_attn_pool_bwd_ws_bytes
    for args in ((0, 2, 3, 4), (8, 0, 3, 4), (8, 2, 0, 4), (8, 2, 3, 0)):
        assert size(*args) == 0
    base = (100, 7, 9, 17)
    s0 = size(*base)
    assert s0 >= 4 * (7 * 9 + 7 * 17) and s0 % 16 == 0
    for k in range(4):
        prev = s0
        for step in (1, 5, 64, 1000):
            args = list(base)
            args[k] += step
            cur = size(*args)
            assert cur >= prev and cur % 16 == 0, (k, step, cur, prev)
            prev = cur
        assert prev > s0, k
