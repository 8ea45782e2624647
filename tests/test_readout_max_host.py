"""Max pooling in the fused training readout without a GPU: the fp64 restatement (tests/readout_max_oracle.py) pinned to
oracle.glass_oracle's GraphNorm + segment_pool(..., "max") plus autograd on inputs without ties, its tie / duplicate / empty
row rules on hand-made rows, and the host-side answers and refusals of the glass_readout_max_* C entries."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import readout_max_oracle as R  # noqa: E402
from helpers import rel_inf  # noqa: E402

E_ARG, E_UNSUPPORTED, E_WS = -1, -3, -4


def _inputs(seed, N=120, C=9, B=7, S=6, K=3):
    g = torch.Generator().manual_seed(seed)
    jk = R.separated_columns(N, C, g)
    gamma = torch.randn(C, generator=g, dtype=torch.float64)  # (negative entries: the max is over y, not over the raw row)
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    alpha = 0.5 + torch.rand(C, generator=g, dtype=torch.float64)
    pos = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(B)])  # no node twice in a row: no ties
    pos[1, 3:] = -1
    pos[2, :] = -1                      # an empty row: pooled 0, no gradient
    pos[4, 0] = pos[3, 0]               # a node shared by three subgraphs
    pos[5, 0] = pos[3, 0]
    Wh = torch.randn(K, C, generator=g, dtype=torch.float64)
    bh = torch.randn(K, generator=g, dtype=torch.float64)
    return g, jk, gamma, beta, alpha, pos, Wh, bh


@pytest.mark.parametrize("loss_mode", [0, 1])
def test_restatement_equals_the_oracle_with_autograd(loss_mode):
    """GraphNorm module + segment_pool(..., "max") + nn.Linear + the torch loss, differentiated by autograd, against the closed
    forms of the helper: every output and gradient within 1e-12 (fp64)."""
    from oracle import glass_oracle as O
    g, jk, gamma, beta, alpha, pos, Wh, bh = _inputs(3)
    assert bool((gamma < 0).any()) and bool((gamma > 0).any())
    B, K, C = pos.shape[0], Wh.shape[0], jk.shape[1]
    target = torch.randint(0, K, (B, ), generator=g) if loss_mode == 0 else (torch.rand(B, K, generator=g) > 0.5).double()
    gn = O.GraphNorm(C).double()
    head = nn.Linear(C, K).double()
    with torch.no_grad():
        gn.weight.copy_(gamma), gn.bias.copy_(beta), gn.mean_scale.copy_(alpha)
        head.weight.copy_(Wh), head.bias.copy_(bh)
    x = jk.clone().requires_grad_(True)
    y = gn(x)
    valid = pos >= 0
    batch = torch.arange(B).reshape(-1, 1).expand_as(pos)[valid]
    pooled = O.segment_pool(y[pos[valid]], batch, B, "max")
    logits = head(pooled)
    loss = nn.CrossEntropyLoss()(logits, target) if loss_mode == 0 else nn.BCEWithLogitsLoss()(logits.flatten(), target.flatten())
    loss.backward()
    got = R.readout_max(jk, gamma, beta, alpha, gn.eps, pos, Wh, bh, target, loss_mode)
    want = dict(pooled=pooled, logits=logits, loss=loss, djk=x.grad, dWh=head.weight.grad, dbh=head.bias.grad,
                dgamma=gn.weight.grad, dbeta=gn.bias.grad, dalpha=gn.mean_scale.grad)
    for k, v in want.items():
        assert rel_inf(got[k], v.detach()) < 1e-12, k
    assert bool((got["arg"][2] == -1).all()) and bool((got["pooled"][2] == 0).all())
    ok, gap = R.top_gap_ok(got["y"], pos)
    assert ok, gap  # "without ties" is a property of these inputs (separated_columns), not luck


def test_restatement_tie_duplicate_and_range_rules():
    """Hand-made rows: an exact tie between two distinct nodes goes to the lower position; a node listed twice counts at its
    first position; padding and out-of-range ids are skipped; the winner is decided on y (negative gamma picks the smallest
    raw value)."""
    jk = torch.tensor([[1.0, 5.0], [3.0, 2.0], [3.0, -4.0], [0.0, 0.5], [-2.0, 1.0], [2.5, 9.0]], dtype=torch.float64)
    gamma, beta, alpha = torch.tensor([1.0, -1.0]).double(), torch.zeros(2).double(), torch.ones(2).double()
    pos = torch.tensor([[0, 2, 1, -1],      # column 0: nodes 2 and 1 tie at 3.0 -> position 1; column 1 (gamma < 0): node 2
                        [4, 4, 3, 99],      # node 4 twice, 99 out of range
                        [-1, -1, -1, -1],
                        [7, -5, -1, 6]])    # nothing valid
    Wh, bh = torch.tensor([[1.0, 2.0], [-1.0, 0.5]]).double(), torch.zeros(2).double()
    out = R.readout_max(jk, gamma, beta, alpha, 1e-5, pos, Wh, bh, torch.tensor([0, 1, 1, 0]), 0)
    assert out["arg"].tolist() == [[1, 1], [2, 2], [-1, -1], [-1, -1]]
    assert out["pooled"][2:].abs().sum() == 0
    # node 1 (the tie's loser) and node 5 (in no row) get the dense part only: rows of d jk that are affine in the raw row
    dense = out["djk"]
    slope = (dense[5] - dense[0]) / (jk[5] - jk[0])  # nodes 0 and 5 carry no pooled gradient
    assert torch.allclose(dense[1], dense[0] + slope * (jk[1] - jk[0]), rtol=0, atol=1e-12)
    assert not torch.allclose(dense[2], dense[0] + slope * (jk[2] - jk[0]), rtol=0, atol=1e-6)


def test_max_entries_exist_and_answer_on_the_host():
    from glass_amd import _lib
    lib = _lib.load()
    assert lib.glass_version() == _lib.ABI_VERSION == 6
    for name in ("glass_readout_max_supported", "glass_readout_max_ws_bytes", "glass_readout_max_train_f32"):
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    for name in ("int glass_readout_max_supported(", "int64_t glass_readout_max_ws_bytes(", "int glass_readout_max_train_f32("):
        assert name in header
    # the C and K limits of glass_readout_supported
    for C, K in ((128, 6), (130, 6), (17, 2), (1024, 256), (1025, 6), (2048, 6), (128, 257), (128, 300), (0, 6), (128, 0)):
        assert lib.glass_readout_max_supported(C, K) == lib.glass_readout_supported(C, K, 0), (C, K)
    assert lib.glass_readout_max_supported(1024, 256) == 1 and lib.glass_readout_max_supported(1025, 6) == 0
    # the existing layout plus the [B][C] int32 argmax block (16-B aligned)
    for B, C, K in ((80, 128, 6), (7, 17, 3), (1, 1, 1), (513, 96, 2)):
        extra = lib.glass_readout_max_ws_bytes(B, C, K) - lib.glass_readout_ws_bytes(B, C, K) - 4 * B * C
        assert 0 <= extra < 16, (B, C, K, extra)
    for bad in ((0, 128, 6), (80, 0, 6), (80, 128, 0), (-1, 128, 6)):
        assert lib.glass_readout_max_ws_bytes(*bad) == -1
    # the old entries answer for mode 2 (max) what they answered before
    assert lib.glass_readout_supported(128, 6, 2) == 0 and lib.glass_readout_supported(17, 2, 2) == 0
    assert lib.glass_readout_ws_bytes(80, 128, 6) == 8 * 2 * 80 * 128 + 4 * (4 * 128 + 80 * 128 + 80 * 6 + 80) + 64
    p = np.zeros(64, dtype=np.float32).ctypes.data
    old = [p, 128, p, p, p, p, 80, 10, 2, p, p, p, 0, 6, p, p, p, p, p, 128, p, p, 1, p, p, p, 1, p, 1000, 128, None, None, None,
           None, None, 0, None, None, None]
    assert lib.glass_readout_train_f32(*old) == E_UNSUPPORTED


def _max_args(p, B=80, Smax=10, n=1000, C=128, K=6, loss_mode=0, **over):
    a = dict(jk=p, ldj=C, saved=p, gamma=p, alpha=p, pos=p, B=B, Smax=Smax, Wh=p, bh=p, target=p, loss_mode=loss_mode, K=K,
             grad_loss=p, pooled=p, logits=p, loss=p, djk=p, lddj=C, dWh=p, dbh=p, acc_head=0, dgamma=p, dbeta=p, dalpha=p,
             acc_gn=0, ws=p, n=n, C=C, mask=None, rows=None, count=None, gn_src=None, bwd_acc=None, bwd_rep=0, sws=None,
             loss_sum=None, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def test_max_train_entry_refuses_on_the_host_before_any_launch():
    """Null pointers / bad sizes -> GLASS_E_ARG, limits -> GLASS_E_UNSUPPORTED, more than 16 384 padded entries without
    scatter_ws -> GLASS_E_WS (this entry never falls back to float atomics); codes, never exceptions, no HIP call."""
    from glass_amd import _lib
    lib = _lib.load()
    x = np.zeros(64, dtype=np.float32)
    p = x.ctypes.data
    for name in ("jk", "saved", "gamma", "alpha", "pos", "Wh", "bh", "target", "grad_loss", "pooled", "logits", "loss", "djk", "dWh",
                 "dbh", "ws"):
        assert lib.glass_readout_max_train_f32(*_max_args(p, **{name: None})) == E_ARG, name
    assert b"null pointer" in lib.glass_last_error_string()
    for over in (dict(B=0), dict(Smax=0), dict(n=0), dict(ldj=64), dict(lddj=64), dict(Smax=1 << 31)):
        assert lib.glass_readout_max_train_f32(*_max_args(p, **over)) == E_ARG, over
    assert lib.glass_readout_max_train_f32(*_max_args(p, C=2048, ldj=2048, lddj=2048)) == E_UNSUPPORTED
    assert lib.glass_readout_max_train_f32(*_max_args(p, K=300)) == E_UNSUPPORTED
    assert lib.glass_readout_max_train_f32(*_max_args(p, loss_mode=2)) == E_UNSUPPORTED
    # scalar form (C % 4 != 0) needs the label bytes
    assert lib.glass_readout_max_train_f32(*_max_args(p, C=17, ldj=17, lddj=17)) == E_ARG
    assert b"label bytes" in lib.glass_last_error_string()
    # 200 x 155 padded entries > 16 384 without scatter_ws
    assert lib.glass_readout_max_train_f32(*_max_args(p, B=200, Smax=155, n=50000)) == E_WS
    assert b"scatter_ws" in lib.glass_last_error_string()
    # gn_bwd_rep outside 1 .. 16 with accumulators given
    assert lib.glass_readout_max_train_f32(*_max_args(p, mask=p, rows=p, count=p, bwd_acc=p, bwd_rep=0)) == E_ARG


def test_step_supported_keys_on_the_max_query(monkeypatch):
    """stack.step_supported asks glass_readout_max_supported for a MaxPool model (and the old query for the others)."""
    from glass_amd import stack, losses, models
    from glass_amd.factory import build_glass

    class Lib:
        def __init__(self):
            self.asked = []

        def glass_readout_max_supported(self, C, K):
            self.asked.append(("max", C, K))
            return 1

        def glass_readout_supported(self, C, K, mode):
            self.asked.append(("old", C, K, mode))
            return 0 if mode == 2 else 1

    torch.manual_seed(0)
    built = {}
    for pool in ("max", "sum"):
        model = build_glass(64, 2, 10, 3, "mean", pool, 0.8).train()
        for p in model.parameters():
            p.grad = torch.zeros_like(p)
        assert isinstance(model.pools[0], models.PoolModule) and model.pools[0].mode == pool
        built[pool] = model
    fake = Lib()
    monkeypatch.setattr(stack._lib, "load", lambda: fake)
    monkeypatch.setattr(stack.StackProgram, "supported", staticmethod(lambda emb: True))
    for pool, model in built.items():
        assert stack.step_supported(model, losses.CrossEntropy()), pool
    assert fake.asked == [("max", 128, 3), ("old", 128, 3, 0)]
