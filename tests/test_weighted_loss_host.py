"""Class-weighted losses, everything that needs no GPU: the marker classes and their validation, losses.fusable_spec, the fp64
restatement (tests/weighted_loss_oracle.py) against torch's functional losses, the six `_w` entries of the C ABI (exported,
declared, refusing bad weight / mode pairs before any HIP call) and the drivers' `balanced` weights."""
import ctypes
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import weighted_loss_oracle as WO
from glass_amd import _lib, losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("glass_head_loss_fwd_w_f32", "glass_head_loss_bwd_w_f32", "glass_head_mlp_loss_fwd_w_f32",
         "glass_head_mlp_loss_bwd_w_f32", "glass_readout_train_w_f32", "glass_readout_max_train_w_f32")
E_UNSUPPORTED = -3


def _data(B, K, seed):
    g = torch.Generator().manual_seed(seed)
    z = 3.0 * torch.randn(B, K, generator=g, dtype=torch.float64)
    return z, torch.randint(0, K, (B, ), generator=g), (torch.rand(B, K, generator=g) > 0.5).double(), g


def test_markers_without_arguments_are_unchanged():
    z, t, y, _ = _data(7, 4, 0)
    z = z.float()
    ce, bce = losses.CrossEntropy(), losses.BCEWithLogits()
    assert ce.weight is None and bce.pos_weight is None and ce.mode == 0 and bce.mode == 1
    assert torch.equal(ce(z, t), F.cross_entropy(z, t))
    assert torch.equal(bce(z, y.float()), F.binary_cross_entropy_with_logits(z.flatten(), y.float().flatten()))
    assert losses.fusable_mode(ce) == 0 and losses.fusable_mode(bce) == 1
    assert losses.fusable_spec(ce) == (0, None, None) and losses.fusable_spec(bce) == (1, None, None)
    assert not list(ce.state_dict()) and not list(bce.state_dict())


def test_weighted_markers_equal_torch_and_keep_a_buffer():
    z, t, y, g = _data(9, 4, 1)
    z = z.float()
    w = 0.25 + 2.0 * torch.rand(4, generator=g)
    ce, bce = losses.CrossEntropy(weight=w), losses.BCEWithLogits(pos_weight=w)
    assert torch.equal(ce(z, t), F.cross_entropy(z, t, weight=w))
    assert torch.equal(bce(z, y.float()), F.binary_cross_entropy_with_logits(z, y.float(), pos_weight=w))
    assert "weight" in dict(ce.named_buffers()) and "pos_weight" in dict(bce.named_buffers())
    assert ce.weight is not w and torch.equal(ce.weight, w)  # (its own copy: a later edit of the argument does not reach it)
    assert ce.to(torch.device("cpu")).weight.device.type == "cpu"
    # K = 1 (binary, 1-D targets as the drivers have them)
    b1 = losses.BCEWithLogits(pos_weight=torch.tensor([3.0]))
    z1, y1 = z[:, :1].contiguous(), y[:, 0].float()
    assert torch.equal(b1(z1, y1), F.binary_cross_entropy_with_logits(z1.flatten(), y1, pos_weight=torch.tensor(3.0)))


@pytest.mark.parametrize("bad", [torch.tensor([1.0, 0.0]), torch.tensor([1.0, -2.0]), torch.tensor([1.0, float("nan")]),
                                 torch.tensor([1.0, float("inf")]), torch.ones(2, 2), torch.ones(2, dtype=torch.float64),
                                 torch.ones(0), [1.0, 2.0]], ids=["zero", "negative", "nan", "inf", "2d", "fp64", "empty", "list"])
def test_weight_validation(bad):
    with pytest.raises(ValueError):
        losses.CrossEntropy(weight=bad)
    with pytest.raises(ValueError):
        losses.BCEWithLogits(pos_weight=bad)


def test_fusable_spec():
    w = torch.tensor([1.0, 2.0, 0.5])
    ce, bce = losses.CrossEntropy(weight=w), losses.BCEWithLogits(pos_weight=w)
    mode, cw, pw = losses.fusable_spec(ce)
    assert mode == 0 and cw is ce.weight and pw is None
    mode, cw, pw = losses.fusable_spec(bce)
    assert mode == 1 and cw is None and pw is bce.pos_weight
    assert losses.fusable_spec(nn.CrossEntropyLoss()) == (0, None, None)
    assert losses.fusable_spec(lambda a, b: nn.BCEWithLogitsLoss()(a.flatten(), b.flatten())) == (1, None, None)
    # torch's own weighted losses, bare or inside a callable: not fusable (a probe cannot recover the weight tensor)
    for other in (nn.CrossEntropyLoss(weight=torch.ones(3)), nn.CrossEntropyLoss(weight=torch.tensor([1.0, 2.0, 3.0])),
                  nn.BCEWithLogitsLoss(pos_weight=torch.tensor([2.0])),
                  lambda a, b: F.cross_entropy(a, b, weight=torch.linspace(0.5, 2.0, a.shape[1])),
                  lambda a, b: F.binary_cross_entropy_with_logits(a.flatten(), b.flatten(), pos_weight=torch.tensor(3.0)),
                  nn.MSELoss(), None):
        assert losses.fusable_spec(other) is None, other
    # the length is checked against the head's K before any launch
    with pytest.raises(ValueError):
        losses.weight_ptrs(losses.fusable_spec(ce), 4, "cpu")
    assert losses.weight_ptrs(losses.fusable_spec(ce), 3, "cpu") == (ce.weight.data_ptr(), 0)
    assert losses.weight_ptrs((1, None, None), 3, "cpu") == (0, 0)


@pytest.mark.parametrize("B,K", [(1, 2), (5, 3), (257, 6)])
def test_restatement_equals_torch_fp64(B, K):
    z, t, y, g = _data(B, K, 10 + B)
    for w in (None, 0.2 + 3.0 * torch.rand(K, generator=g, dtype=torch.float64),
              torch.logspace(-3, 3, K, dtype=torch.float64)):
        for gl in (1.0, 0.37):
            zr = z.clone().requires_grad_(True)
            want = F.cross_entropy(zr, t, weight=w)
            gw, = torch.autograd.grad(want * gl, zr)
            zo = z.clone().requires_grad_(True)
            got = WO.ce_weighted(zo, t, w)
            go, = torch.autograd.grad(got * gl, zo)
            assert abs(float(got.detach()) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
            assert float((go - gw).abs().max()) <= 1e-12 * max(float(gw.abs().max()), 1e-300)
            assert float((WO.ce_weighted_dlogits(z, t, w, gl) - gw).abs().max()) <= 1e-12 * max(float(gw.abs().max()), 1e-300)
            zr = z.clone().requires_grad_(True)
            want = F.binary_cross_entropy_with_logits(zr, y, pos_weight=w)
            gw, = torch.autograd.grad(want * gl, zr)
            zo = z.clone().requires_grad_(True)
            got = WO.bce_pos_weighted(zo, y, w)
            go, = torch.autograd.grad(got * gl, zo)
            assert abs(float(got.detach()) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
            assert float((go - gw).abs().max()) <= 1e-12 * float(gw.abs().max())
            assert float((WO.bce_pos_weighted_dlogits(z, y, w, gl) - gw).abs().max()) <= 1e-12 * float(gw.abs().max())


def test_restatement_drops_targets_outside_the_classes():
    z, t, _y, g = _data(6, 3, 3)
    w = torch.tensor([0.5, 2.0, 4.0], dtype=torch.float64)
    t2 = t.clone()
    t2[1], t2[4] = -100, 7
    keep = torch.tensor([0, 2, 3, 5])
    assert abs(float(WO.ce_weighted(z, t2, w)) - float(F.cross_entropy(z[keep], t[keep], weight=w))) < 1e-12
    d = WO.ce_weighted_dlogits(z, t2, w)
    assert float(d[1].abs().max()) == 0.0 and float(d[4].abs().max()) == 0.0


def test_symbols_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert f"int {name}(" in header
        old = name.replace("_w_f32", "_f32")
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[old][1]) + 2   # class_weight, pos_weight before stream
        assert _lib.SIGNATURES[name][1][:-3] == _lib.SIGNATURES[old][1][:-1]


def test_abi_refusals_come_before_any_hip_call():
    """Both weights set, class_weight with BCE (mode 1), pos_weight with cross-entropy (mode 0): GLASS_E_UNSUPPORTED from
    every `_w` entry on this machine without a GPU — the pointers are never followed; two nulls pass the check (the head
    entries then fail later, at the launch)."""
    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    B, C, K, Hd = 4, 8, 3, 8

    def calls(mode, cw, pw):
        yield "head_fwd", lib.glass_head_loss_fwd_w_f32(p, C, p, p, p, mode, B, C, K, p, p, p, cw, pw, None)
        yield "head_bwd", lib.glass_head_loss_bwd_w_f32(p, C, p, p, p, mode, p, B, C, K, p, C, p, p, 0, cw, pw, None)
        yield "mlp_fwd", lib.glass_head_mlp_loss_fwd_w_f32(p, C, p, p, p, p, p, mode, 1, 0.0, None, 3, B, C, Hd, K, p, p, p, p,
                                                           cw, pw, None)
        yield "mlp_bwd", lib.glass_head_mlp_loss_bwd_w_f32(p, C, p, p, p, p, p, mode, 1, 0.0, None, 3, p, B, C, Hd, K, p, p, C,
                                                           p, p, p, p, 0, cw, pw, None)
        ro = (p, C, p, p, p, p, B, 5)
        rest = (p, p, p, mode, K, p, p, p, p, p, C, p, p, 0, p, p, p, 0, p, 100, C, None, None, None, None, None, 1, None, None,
                cw, pw, None)
        yield "readout", lib.glass_readout_train_w_f32(*ro, 0, *rest)
        yield "readout_max", lib.glass_readout_max_train_w_f32(*ro, *rest)

    for mode, cw, pw in ((0, p, p), (1, p, p), (1, p, None), (0, None, p)):
        for who, rc in calls(mode, cw, pw):
            assert rc == E_UNSUPPORTED, (who, mode, cw is not None, pw is not None, rc)
            assert b"class_weight" in lib.glass_last_error_string()


def test_balanced_weights():
    # multi-class: w_k = n / (K * count_k); class 2 is absent -> 1
    y = torch.tensor([0, 0, 0, 1, 3, 3, 0, 1])
    w = losses.balanced_weights(y, 4)
    assert w.dtype == torch.float32 and torch.allclose(w, torch.tensor([8 / (4 * 4), 8 / (4 * 2), 1.0, 8 / (4 * 2)]))
    assert torch.equal(losses.balanced_weights(y), w)                     # K defaults to max + 1
    assert losses.balanced_weights(y, 5)[4].item() == 1.0
    # multi-label: p_k = neg_k / pos_k; an all-zero column (and an all-one column) -> 1
    Y = torch.tensor([[1, 0, 0, 1], [0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1]], dtype=torch.float32)
    p = losses.balanced_weights(Y)
    assert torch.allclose(p, torch.tensor([3.0, 1.0, 1 / 3, 1.0]))
    # binary with 1-D float targets: one column
    assert torch.allclose(losses.balanced_weights(torch.tensor([1.0, 0.0, 0.0, 0.0, 0.0])), torch.tensor([4.0]))
    ce, bce = losses.balanced_loss(y, 4), losses.balanced_loss(Y, 4)
    assert isinstance(ce, losses.CrossEntropy) and torch.equal(ce.weight, w)
    assert isinstance(bce, losses.BCEWithLogits) and torch.equal(bce.pos_weight, p)


def test_drivers_take_the_flag():
    import GLASSTest
    import GNNSeg
    for mod in (GLASSTest, GNNSeg):
        assert mod.parse_args(["--dataset", "density"]).class_weight == "none"
        assert mod.parse_args(["--dataset", "density", "--class_weight", "balanced"]).class_weight == "balanced"
        with pytest.raises(SystemExit):
            mod.parse_args(["--class_weight", "sqrt"])
