"""Host side of K9c, gradient clipping by global norm (no GPU): the two exports and their argument checks, the optimizer
switch (`param_groups[0]["max_grad_norm"]`) with its validation, what hyper() / fusable() / adoptable() answer, and the
restatement tests/gradclip_oracle.py against torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the CPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import gradclip_oracle as GO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1


def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def test_symbols_prototypes_and_header():
    L, lib = _lib()
    c, P, I = ctypes, ctypes.c_void_p, ctypes.c_int64
    assert L.SIGNATURES["glass_grad_norm_chunk"] == (c.c_int64, [])
    assert L.SIGNATURES["glass_grad_norm_f32"] == (c.c_int, [P, I, P, I, c.c_float, P, P])
    assert L.SIGNATURES["glass_adam_step_clip_f32"] == (c.c_int, [P, P, P, P, I, P, c.c_double, c.c_double, c.c_double, c.c_double,
                                                                   P, P, P])
    # glass_adam_step_f32's arguments plus `coef` in front of the stream
    base = L.SIGNATURES["glass_adam_step_f32"][1]
    assert L.SIGNATURES["glass_adam_step_clip_f32"][1] == base[:-1] + [P] + base[-1:]
    for name in ("glass_grad_norm_chunk", "glass_grad_norm_f32", "glass_adam_step_clip_f32"):
        assert hasattr(lib, name)
    chunk = lib.glass_grad_norm_chunk()
    assert chunk > 0 and chunk % 4 == 0
    header = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    for name in ("glass_grad_norm_chunk", "glass_grad_norm_f32", "glass_adam_step_clip_f32"):
        m = re.search(r"^(?:int|int64_t) %s\(.*?;(.*)$" % name, header, re.M | re.S)
        assert m and "GLASSTest.py:213" in m.group(1).split("\n")[0], f"{name}: no reference call site behind the declaration"
    assert lib.glass_version() == L.ABI_VERSION == 6  # purely additive


def test_grad_norm_argument_checks():
    """Every refusal happens on the host before any launch (the buffers below are host memory and never reach a kernel)."""
    _L, lib = _lib()
    chunk = lib.glass_grad_norm_chunk()
    g = np.zeros(4 * chunk + 8, dtype=np.float32)
    part = np.zeros(8, dtype=np.float64)
    out = np.zeros(2, dtype=np.float32)
    gp, pp, op = g.ctypes.data, part.ctypes.data, out.ctypes.data
    n = 3 * chunk + 17  # 4 chunks

    def refused(*args, text):
        assert lib.glass_grad_norm_f32(*args, None) == E_ARG
        msg = lib.glass_last_error_string().decode()
        assert text in msg, msg

    refused(None, n, pp, 8, 1.0, op, text="null")
    refused(gp, n, None, 8, 1.0, op, text="null")
    refused(gp, n, pp, 8, 1.0, None, text="null")
    refused(gp, 0, pp, 8, 1.0, op, text="n = 0")
    refused(gp, -5, pp, 8, 1.0, op, text="n = -5")
    refused(gp, n, pp, 3, 1.0, op, text="n_partials = 3")          # 4 chunks need 4
    refused(gp, chunk + 1, pp, 1, 1.0, op, text="n_partials = 1")  # one element past a chunk: 2
    refused(gp, n, pp, 8, -1.0, op, text="max_norm")
    refused(gp, n, pp, 8, float("nan"), op, text="max_norm")
    refused(gp + 2, n, pp, 8, 1.0, op, text="misaligned")          # not even a float boundary
    refused(gp, n, pp + 4, 8, 1.0, op, text="misaligned")


def test_adam_step_clip_argument_checks():
    _L, lib = _lib()
    a = np.zeros(8, dtype=np.float32)
    s = np.zeros(2, dtype=np.int64)
    p, sp = a.ctypes.data, s.ctypes.data
    good = [p, p, p, p, 8, p, 0.9, 0.999, 1e-8, 0.0, sp, p]
    for k in (0, 1, 2, 3, 5, 10, 11):  # each pointer in turn
        args = list(good)
        args[k] = None
        assert lib.glass_adam_step_clip_f32(*args, None) == E_ARG
        assert b"adam_step_clip" in lib.glass_last_error_string()
    for n in (0, -1):
        args = list(good)
        args[4] = n
        assert lib.glass_adam_step_clip_f32(*args, None) == E_ARG
        assert b"adam_step_clip" in lib.glass_last_error_string()


class _Arena:
    """What _FlatAdamCore reads of an arena, on the CPU; the state switches are plain attributes."""
    def __init__(self, n=40):
        self.params = [torch.nn.Parameter(torch.zeros(n))]
        self.flat_param = self.params[0].data
        self.flat = torch.zeros(n)
        self.is_sharded, self.is_attached = False, True

    def sharded(self):
        return self.is_sharded

    def attached(self):
        return self.is_attached


def test_flat_adam_switch_validation_hyper_and_fusable():
    from glass_amd import optim
    from glass_amd._lib import GlassHipError
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            optim.FlatAdam(_Arena(), max_grad_norm=bad)
    off = optim.FlatAdam(_Arena())
    assert off.param_groups[0]["max_grad_norm"] is None
    assert off.hyper() == (0.9, 0.999, 1e-8, 0.0, None) and len(off.hyper()) == 5
    assert len(off.fused_args()) == 11  # (the fused tail's tuple is unchanged: clipping never rides in it)
    on = optim.FlatAdam(_Arena(), lr=1e-2, weight_decay=1e-2, max_grad_norm=0.5)
    assert on.hyper() == (0.9, 0.999, 1e-8, 1e-2, 0.5)
    assert tuple(on.grad_norm_dev.shape) == (2, ) and on.grad_norm_dev.dtype == torch.float32
    # fusable(): off -> the arena's state decides, exactly as before; on -> never
    for opt, clipped in ((off, False), (on, True)):
        a = opt.arena
        for sharded, attached, peer in ((False, True, None), (True, True, None), (False, False, None), (False, True, object())):
            a.is_sharded, a.is_attached, a._peer = sharded, attached, peer
            want = (not sharded) and attached and peer is None and not clipped
            assert opt.fusable() is want, (clipped, sharded, attached, peer)
        a.is_sharded, a.is_attached, a._peer = False, True, None
    # the switch on a live optimizer
    for bad in (0, -2.0, float("nan")):
        with pytest.raises(ValueError):
            optim.set_max_grad_norm(off, bad)
    optim.set_max_grad_norm(off, 2.0)
    assert off.hyper()[4] == 2.0 and not off.fusable()
    optim.set_max_grad_norm(off, None)
    assert off.hyper()[4] is None and off.fusable()
    # a value written into the group behind the helper's back is validated where it is read
    off.param_groups[0]["max_grad_norm"] = -1.0
    with pytest.raises(ValueError):
        off.hyper()
    # not served: a sharded arena, an attached peer exchange — refused before any launch
    for attr, value, word in (("is_sharded", True, "sharded"), ("_peer", object(), "peer")):
        opt = optim.FlatAdam(_Arena(), max_grad_norm=1.0)
        setattr(opt.arena, attr, value)
        with pytest.raises(GlassHipError, match=word):
            opt.step()


def test_switch_on_a_plain_torch_adam_and_adoptable_is_unchanged():
    from glass_amd import optim
    model = torch.nn.Linear(3, 2)
    adam = torch.optim.Adam(model.parameters(), lr=1e-3)
    optim.set_max_grad_norm(adam, 1.5)
    assert adam.param_groups[0]["max_grad_norm"] == 1.5
    assert adam.state_dict()["param_groups"][0]["max_grad_norm"] == 1.5  # torch keeps the unknown key
    with pytest.raises(ValueError):
        optim.set_max_grad_norm(adam, 0.0)
    # adoptable(): the answers of before, with and without the key (CPU parameters: the last check speaks)
    for clip in (None, 1.0):
        a = torch.optim.Adam(model.parameters(), lr=1e-3)
        optim.set_max_grad_norm(a, clip)
        assert optim.adoptable(a, model) == "parameters must be fp32 on the GPU"
        w = torch.optim.AdamW(model.parameters(), lr=1e-3)
        optim.set_max_grad_norm(w, clip)
        assert optim.adoptable(w, model) == "optimizer is AdamW, not torch.optim.Adam"
        s = torch.optim.Adam(model.parameters(), lr=1e-3, amsgrad=True)
        optim.set_max_grad_norm(s, clip)
        assert optim.adoptable(s, model) == "amsgrad=True"


def test_driver_flag():
    import GLASSTest
    assert GLASSTest.parse_args([]).clip is None
    assert GLASSTest.parse_args(["--clip", "0.5"]).clip == 0.5
    for bad in ("0", "-1", "nan"):
        with pytest.raises(SystemExit):
            GLASSTest.parse_args(["--clip", bad])


# ---- the restatement against torch on the CPU ---------------------------------------------------------------------------
SHAPES = [(7, 5), (5, ), (33, ), (4, 3, 2)]


def _case(seed, dtype):
    """Parameters of magnitude 0.5..2 (so 2 ulp OF A PARAMETER is a bound on the update's error, not on a cancelled
    difference), three gradients per parameter with magnitudes over four decades and both signs."""
    gen = torch.Generator().manual_seed(seed)
    ps = [((0.5 + 1.5 * torch.rand(s, generator=gen)) * torch.where(torch.rand(s, generator=gen) < 0.5, -1.0, 1.0)).to(dtype)
          for s in SHAPES]
    gs = [[(torch.randn(s, generator=gen) * 10.0 ** torch.randint(-3, 1, s, generator=gen).double()).to(dtype) for s in SHAPES]
          for _ in range(3)]
    return ps, gs


def _torch_run(ps, gs, max_norm, lr, wd):
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.Adam(params, lr=lr, weight_decay=wd)
    norms = []
    for step in gs:
        for p, g in zip(params, step):
            p.grad = g.clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, max_norm)))
        opt.step()
    return torch.cat([p.detach().reshape(-1) for p in params]), norms


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("where", ["below", "above"])
def test_oracle_equals_torch_clip_and_adam(wd, where):
    """Three steps of clip_grad_norm_ + torch.optim.Adam over four tensors == the restatement on the flat vector.  fp32:
    within 2 ulp of each parameter (torch's norm is an fp32 reduction, the restatement's an fp64 one rounded once: the
    coefficients may differ in the last bit).  fp64: 1e-12 relative."""
    ps32, gs32 = _case(5, torch.float32)
    flat_g = [torch.cat([g.reshape(-1) for g in step]) for step in gs32]
    norms = [float(GO.global_norm(g)) for g in flat_g]
    # "below": no step clips; "above": every step clips (coefficient ~ 0.1 .. 0.5)
    max_norm = 2.0 * max(norms) if where == "below" else 0.1 * min(norms)
    lr = 1e-3
    want, t_norms = _torch_run(ps32, gs32, max_norm, lr, wd)
    got, seen = GO.clipped_run(torch.cat([p.reshape(-1) for p in ps32]), flat_g, max_norm, lr, weight_decay=wd)
    assert all((c == 1.0) == (where == "below") for _n, c in seen), seen
    assert np.allclose([n for n, _c in seen], t_norms, rtol=4e-7, atol=0)
    ulp = np.spacing(np.abs(want.numpy()))
    worst = float(np.max(np.abs(got.numpy().astype(np.float64) - want.numpy().astype(np.float64)) / ulp))
    assert worst <= 2.0, f"restatement vs torch fp32: {worst} ulp"
    assert not torch.equal(got, torch.cat([p.reshape(-1) for p in ps32]))
    # the same in double
    ps64, gs64 = [p.double() for p in ps32], [[g.double() for g in step] for step in gs32]
    want64, _ = _torch_run(ps64, gs64, max_norm, lr, wd)
    got64, _ = GO.clipped_run(torch.cat([p.reshape(-1) for p in ps64]), [g.double() for g in flat_g], max_norm, lr, weight_decay=wd)
    rel = float(((got64 - want64).abs() / want64.abs()).max())
    assert rel <= 1e-12, rel
    # clipping acted: the clipped run is not the unclipped one
    if where == "above":
        free, _ = GO.clipped_run(torch.cat([p.reshape(-1) for p in ps64]), [g.double() for g in flat_g], math.inf, lr, weight_decay=wd)
        assert float((free - got64).abs().max()) > 1e-6


def test_oracle_coefficient_edge_values():
    f = lambda x: torch.tensor(x, dtype=torch.float32)
    assert float(GO.clip_coef(f(0.0), 1.0)) == 1.0
    assert float(GO.clip_coef(f(math.inf), 1.0)) == 0.0
    assert math.isnan(float(GO.clip_coef(f(math.nan), 1.0)))
    assert float(GO.global_norm(torch.tensor([3e18, -4e18, 1e-20]))) == float(f(5e18))
