"""K9 (the pair head of the pre-training path, pairhead.hip) without a GPU: the fp64 statement of the head
(tests/pair_head_oracle.py) pinned against the oracle's head + nn.BCEWithLogitsLoss, the argument checks of
glass_pair_head_{fwd,bwd}_f32 (each refusal returns GLASS_E_ARG with a message, before any launch), and the size the
workspace entry reports."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pair_head_oracle as PH  # noqa: E402
from helpers import rel_inf  # noqa: E402
from oracle import glass_oracle as O  # noqa: E402

H = 64
E_ARG = -1


# ---- the fp64 statement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_pair_head_statement_vs_oracle_head(p):
    """pair_head() = OracleEdgeGNN's head (Linear, [Dropout], ReLU, Linear on the mean over the pair) + BCEWithLogitsLoss in
    fp64 at a small valid input (a hub, a self pair, a node no pair names), to fp64 rounding: 1e-12 relative.  With dropout,
    both sides multiply by the same fed keep-scales."""
    g = torch.Generator().manual_seed(3)
    n, P = 37, 150
    emb = torch.randn(n, H, generator=g, dtype=torch.float64)
    pairs = torch.randint(0, n - 1, (P, 2), generator=g)   # node n - 1: never named
    pairs[:20, 0] = 5
    pairs[7] = torch.tensor([9, 9])
    y = torch.randint(0, 2, (P, ), generator=g).double()
    torch.manual_seed(1)
    orc = O.OracleEdgeGNN(H, 1, 3, dropout=p).double().train()
    head = orc.preds[0]
    lin0, lin1 = head.seq.modlist[0], head.seq.modlist[-1]
    scales = None
    if p > 0:
        scales = (torch.rand(P, H, generator=g) >= p).double() / (1.0 - p)
        O.mask_feed([scales])
    e = emb.clone().requires_grad_(True)
    try:
        logits = head(e[pairs].mean(dim=1)).flatten()
        assert not O._MASK_FEED
    finally:
        O.mask_feed([])
    loss = nn.BCEWithLogitsLoss()(logits, y)
    logits.retain_grad()
    loss.backward()
    r = PH.pair_head(emb, pairs, lin0.weight, lin0.bias, lin1.weight.reshape(-1), lin1.bias, y, scales=scales)
    for mine, ref in ((r["logits"], logits.detach()), (r["loss"], loss.detach()), (r["dlogit"], logits.grad),
                      (r["dW0"], lin0.weight.grad), (r["db0"], lin0.bias.grad), (r["dw1"], lin1.weight.grad.reshape(-1)),
                      (r["db1"], lin1.bias.grad), (r["demb"], e.grad)):
        assert rel_inf(mine, ref) < 1e-12
    assert float(r["demb"][n - 1].abs().max()) == 0.0 and float(r["demb"].abs().max()) > 0
    if p > 0:
        assert bool((r["hid"][scales == 0] == 0).all())
    # the ReLU as a fed mask of the same branches changes nothing; grad_scale scales every gradient and not the loss
    r2 = PH.pair_head(emb, pairs, lin0.weight, lin0.bias, lin1.weight.reshape(-1), lin1.bias, y, scales=scales,
                      relu_mask=r["hid"] > 0, grad_scale=0.25)
    assert torch.equal(r2["logits"], r["logits"]) and torch.equal(r2["loss"], r["loss"])
    for k in ("dlogit", "dW0", "db0", "dw1", "db1", "demb"):
        assert torch.equal(r2[k], r[k] * 0.25)


def test_pair_head_statement_counts_an_invalid_id_as_a_zero_row():
    """include/glass_hip.h, K9: an id outside [0, N) counts as a zero row — the mean still divides by 2."""
    g = torch.Generator().manual_seed(4)
    n = 6
    emb = torch.randn(n, H, generator=g, dtype=torch.float64)
    W0, b0 = torch.randn(H, H, generator=g, dtype=torch.float64), torch.randn(H, generator=g, dtype=torch.float64)
    w1, b1 = torch.randn(H, generator=g, dtype=torch.float64), torch.randn(1, generator=g, dtype=torch.float64)
    y = torch.tensor([1., 0., 1., 0.])
    bad = torch.tensor([[2, -1], [n, 3], [n + 7, 1 << 40], [4, 4]])
    pad = torch.cat([emb, torch.zeros(1, H, dtype=torch.float64)])       # row n: the zero row
    good = torch.tensor([[2, n], [n, 3], [n, n], [4, 4]])
    r, ref = PH.pair_head(emb, bad, W0, b0, w1, b1, y), PH.pair_head(pad, good, W0, b0, w1, b1, y)
    for k in ("logits", "loss", "dlogit", "dW0", "db0", "dw1", "db1"):
        assert torch.equal(r[k], ref[k])
    assert torch.equal(r["demb"], ref["demb"][:n])
    assert abs(float(r["logits"][2]) - float(torch.relu(b0) @ w1 + b1)) < 1e-13  # both ids invalid: pooled = 0
    assert float(r["demb"][[0, 5]].abs().max()) == 0.0


# ---- C ABI: refused with a code and a message before any launch --------------------------------------------------------
def _buf():
    raw = np.zeros(4096 + 16, dtype=np.uint8)
    base = raw.ctypes.data
    return raw, base + (-base) % 16


def _last(lib):
    return lib.glass_last_error_string()


def test_pair_head_fwd_refusals():
    from glass_amd import _lib
    lib = _lib.load()
    keep, p = _buf()
    m = p + 4  # 4-B aligned, not 16

    def fwd(emb=p, lde=H, n=8, pairs=p, P=8, W0=p, b0=p, w1=p, b1=p, target=p, p_drop=0.0, rng=None, hid=p, logits=p,
            dlogit=p, ws=p):
        return lib.glass_pair_head_fwd_f32(emb, lde, n, pairs, P, W0, b0, w1, b1, target, p_drop, rng, 2, None, hid, logits,
                                           dlogit, ws, None)
    for kw in (dict(emb=None), dict(pairs=None), dict(W0=None), dict(b0=None), dict(w1=None), dict(b1=None), dict(logits=None),
               dict(lde=63), dict(lde=0), dict(P=0), dict(P=-5), dict(n=0), dict(n=-1)):
        assert fwd(**kw) == E_ARG, kw
        assert b"pair_head_fwd: null pointer / bad sizes" in _last(lib), kw
    for kw in (dict(lde=66), dict(lde=65), dict(emb=m), dict(W0=m), dict(w1=m), dict(hid=m)):
        assert fwd(**kw) == E_ARG, kw
        assert b"pair_head_fwd: operands must be 16-B aligned" in _last(lib), kw
    for kw in (dict(hid=None), dict(dlogit=None), dict(ws=None), dict(ws=m)):  # a target makes it a training pass
        assert fwd(**kw) == E_ARG, kw
        assert b"a training pass needs hid, dlogit and the workspace" in _last(lib), kw
    for kw in (dict(p_drop=-0.1), dict(p_drop=1.0), dict(p_drop=1.5), dict(p_drop=0.5, rng=None), dict(p_drop=float("nan"))):
        assert fwd(**kw) == E_ARG, kw
        assert b"pair_head_fwd: bad dropout arguments" in _last(lib), kw
    assert fwd(n=1 << 23, lde=H) == E_ARG and b"below 2^31" in _last(lib)   # 2^23 rows * 64 * 4 B = 2^31
    assert fwd(P=1 << 23) == E_ARG and b"below 2^31" in _last(lib)
    del keep


def test_pair_head_bwd_refusals():
    from glass_amd import _lib
    lib = _lib.load()
    keep, p = _buf()
    m = p + 4

    def bwd(emb=p, lde=H, n=8, pairs=p, P=8, W0=p, w1=p, hid=p, dlogit=p, p_drop=0.0, dW0=p, db0=p, dw1=p, db1=p, loss=p,
            demb=p, ldde=H, ws=p):
        return lib.glass_pair_head_bwd_f32(emb, lde, n, pairs, P, W0, w1, hid, dlogit, p_drop, dW0, db0, dw1, db1, 0, loss, demb,
                                           ldde, ws, None)
    for kw in (dict(emb=None), dict(pairs=None), dict(W0=None), dict(w1=None), dict(hid=None), dict(dlogit=None), dict(dW0=None),
               dict(db0=None), dict(dw1=None), dict(db1=None), dict(demb=None), dict(ws=None), dict(P=0), dict(P=-1), dict(n=0),
               dict(n=-3)):
        assert bwd(**kw) == E_ARG, kw
        assert b"pair_head_bwd: null pointer" in _last(lib), kw
    for kw in (dict(lde=63), dict(lde=66), dict(ldde=63), dict(ldde=0), dict(ldde=70), dict(emb=m), dict(hid=m), dict(demb=m),
               dict(W0=m), dict(w1=m), dict(ws=m), dict(p_drop=-0.5), dict(p_drop=1.0), dict(p_drop=float("nan"))):
        assert bwd(**kw) == E_ARG, kw
        assert b"pair_head_bwd: operands must be 16-B aligned" in _last(lib), kw
    assert bwd(n=1 << 23) == E_ARG and b"below 2^31" in _last(lib)
    assert bwd(P=1 << 23) == E_ARG and b"below 2^31" in _last(lib)
    del keep


def test_pair_head_ws_bytes_and_supported():
    from glass_amd import _lib
    lib = _lib.load()
    assert lib.glass_pair_head_supported(64) == 1
    assert lib.glass_pair_head_supported(32) == 0 and lib.glass_pair_head_supported(128) == 0
    for n, P in ((0, 5), (5, 0), (-1, 5), (5, -1), (0, 0)):
        assert lib.glass_pair_head_ws_bytes(n, P) < 0
    for n, P in ((1, 1), (1001, 1), (1, 257), (1001, 257), (1001, 32769), (17080, 131072), (3, 4096)):
        slabs, tiles = -(-P // 256), -(-P // 64)
        partials = slabs * (H * H + 2 * H + 4) * 4       # per slab: dW0 tile + db0 + dw1 + db1 (padded to 4 floats)
        loss_parts = tiles * 8                           # one double per forward workgroup
        bucket = 4 * (((n + 1 + 3) // 4) * 4 + 2 * 2 * P)  # off [n + 1, padded to 4] | rank [2P] | list [2P]
        assert bucket == lib.glass_pair_pool_ws_bytes(n, P)
        assert lib.glass_pair_head_ws_bytes(n, P) >= partials + loss_parts + bucket
