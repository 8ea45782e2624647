"""Host-side checks of the per-graph GraphNorm (no GPU): the fp64 restatement against the whole-graph oracle, the errors of
the Python surface, and the argument validation of the C entries (refusals come before any launch)."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import graphnorm_seg_oracle as GO  # noqa: E402
from oracle import glass_oracle as O  # noqa: E402

E_ARG = -1
ENTRIES = ("glass_graphnorm_seg_fwd_f32", "glass_graphnorm_seg_bwd_f32")
QUERIES = ("glass_graphnorm_seg_lds_rows", "glass_graphnorm_seg_ws_bytes")


def _data(n, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, C, generator=g) * 2 + 5).double()
    gamma = (1 + 0.3 * torch.randn(C, generator=g)).double()
    beta = (0.2 * torch.randn(C, generator=g)).double()
    alpha = (1 + 0.3 * torch.randn(C, generator=g)).double()
    return x, gamma, beta, alpha, torch.randn(n, C, generator=g).double()


def test_one_segment_is_the_whole_graph_formula():
    x, gamma, beta, alpha, gout = _data(37, 5)
    gn = O.GraphNorm(5).double()
    with torch.no_grad():
        gn.weight.copy_(gamma), gn.bias.copy_(beta), gn.mean_scale.copy_(alpha)
    xc = x.clone().requires_grad_(True)
    ref = gn(xc)
    ref.backward(gout)
    mine = GO.reference(x, GO.seg_ptr_of([37]), gamma, beta, alpha, gout)
    assert (mine["y"] - ref.detach()).abs().max() < 1e-12
    assert (mine["dx"] - xc.grad).abs().max() < 1e-12
    for k, p in (("dgamma", gn.weight), ("dbeta", gn.bias), ("dalpha", gn.mean_scale)):
        assert (mine[k] - p.grad).abs().max() < 1e-12 * max(1.0, p.grad.abs().max().item())


def test_segments_are_independent_and_empty_ones_take_no_part():
    x, gamma, beta, alpha, _ = _data(10, 3, seed=1)
    y = GO.graphnorm_seg(x, GO.seg_ptr_of([0, 4, 0, 6, 0]), gamma, beta, alpha)
    gn = O.GraphNorm(3).double()
    with torch.no_grad():
        gn.weight.copy_(gamma), gn.bias.copy_(beta), gn.mean_scale.copy_(alpha)
    assert (y - torch.cat((gn(x[:4]), gn(x[4:]))).detach()).abs().max() < 1e-12
    mu, rstd = GO.stats(x, GO.seg_ptr_of([0, 4, 6]), alpha)
    assert mu.shape == (3, 3) and bool((mu[0] == 0).all()) and torch.allclose(mu[1], x[:4].mean(0))


def test_unsorted_batch_raises():
    from glass_amd import models
    gn = models.GraphNorm(4)
    x = torch.randn(5, 4)
    with pytest.raises(ValueError, match="sorted"):
        gn(x, torch.tensor([0, 1, 0, 2, 2]))
    with pytest.raises(ValueError, match="sorted"):
        gn(x, torch.tensor([-1, 0, 0, 2, 2]))
    with pytest.raises(ValueError):
        gn(x, torch.tensor([0, 0, 1]))  # not one index per row
    with pytest.raises(ValueError):
        gn(x, torch.tensor([0, 0, 1, 1, 2], dtype=torch.int32))  # an int32 vector is a seg_ptr only inside the marker


def test_batch_vector_to_segment_pointers():
    from glass_amd import models, ops
    b = torch.tensor([0, 0, 1, 1, 3])
    assert models._seg_ptr_of(b, 5).tolist() == [0, 2, 4, 4, 5] and models._seg_ptr_of(b, 5).dtype == torch.int32
    assert models._seg_ptr_of(b, 5, batch_size=6).tolist() == [0, 2, 4, 4, 5, 5, 5]
    assert models._seg_ptr_of(torch.zeros(0, dtype=torch.int64), 0).tolist() == [0]
    assert len(ops.SegPtr(torch.tensor([0, 2, 5], dtype=torch.int32))) == 2
    with pytest.raises(ValueError):
        ops.SegPtr(torch.tensor([0, 2, 5]))  # int64: that is a batch vector's type


def test_dropout_with_batch_raises():
    from glass_amd import models
    gn = models.GraphNorm(4)
    with pytest.raises(ValueError, match="dropout"):
        gn(torch.randn(5, 4), torch.tensor([0, 0, 1, 1, 2]), p_drop=0.3)


def test_bad_graph_norm_value_raises():
    from glass_amd import seg
    with pytest.raises(ValueError, match="graph_norm"):
        seg.GConv(1, 4, 4, 2, graph_norm="layer")
    assert seg.GConv(1, 4, 4, 2).graph_norm == "batch" and seg.GConv(1, 4, 4, 2, graph_norm="graph").graph_norm == "graph"
    # the keyword is GConv's own: it does not reach the convolution's constructor
    seg.GConv(1, 4, 4, 2, conv=seg.MyGINConv, graph_norm="graph")


def test_driver_flag():
    import GNNSeg
    assert GNNSeg.parse_args([]).graph_norm == "batch"
    assert GNNSeg.parse_args(["--graph_norm", "graph"]).graph_norm == "graph"
    with pytest.raises(SystemExit):
        GNNSeg.parse_args(["--graph_norm", "layer"])


def test_queries():
    from glass_amd import _lib
    lib = _lib.load()
    for C in (1, 8, 17, 20, 64, 128, 256, 512):
        L = lib.glass_graphnorm_seg_lds_rows(C)
        assert L >= 2 and L == lib.glass_graphnorm_seg_lds_rows(C)
        if C > 1:
            assert L <= lib.glass_graphnorm_seg_lds_rows(C - 1)  # wider rows: no more of them fit
    assert lib.glass_graphnorm_seg_lds_rows(0) == E_ARG and lib.glass_graphnorm_seg_lds_rows(513) == E_ARG
    assert lib.glass_graphnorm_seg_ws_bytes(0, 64) == 0
    assert lib.glass_graphnorm_seg_ws_bytes(700, 64) >= 700 * 3 * 64 * 4
    assert lib.glass_graphnorm_seg_ws_bytes(1401, 64) > lib.glass_graphnorm_seg_ws_bytes(700, 64)
    assert lib.glass_graphnorm_seg_ws_bytes(-1, 64) == E_ARG and lib.glass_graphnorm_seg_ws_bytes(4, 0) == E_ARG
    assert lib.glass_graphnorm_seg_ws_bytes(4, 513) == E_ARG


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every call below is refused on the host: the numpy buffers never reach a kernel."""
    from glass_amd import _lib
    lib = _lib.load()
    f = np.zeros(256, dtype=np.float32)
    d = np.zeros(256, dtype=np.float64)
    sp = np.array([0, 2, 4], dtype=np.int32)
    p, q, w = f.ctypes.data, sp.ctypes.data, d.ctypes.data

    def fwd(x=p, ldx=8, y=p, ldy=8, ptr=q, B=2, C=8, gamma=p, beta=p, alpha=p, mu=p, rstd=p, act=0):
        return lib.glass_graphnorm_seg_fwd_f32(x, ldx, y, ldy, ptr, B, C, gamma, beta, alpha, 1e-5, mu, rstd, act, None)

    def bwd(dy=p, lddy=8, x=p, ldx=8, dx=p, lddx=8, ptr=q, B=2, C=8, gamma=p, beta=p, alpha=p, mu=p, rstd=p, dg=p, db=p, da=p,
            act=0, ws=w):
        return lib.glass_graphnorm_seg_bwd_f32(dy, lddy, x, ldx, dx, lddx, ptr, B, C, gamma, beta, alpha, mu, rstd, dg, db, da, 0,
                                               act, ws, None)

    for bad in (dict(x=None), dict(y=None), dict(ptr=None), dict(gamma=None), dict(beta=None), dict(alpha=None), dict(mu=None),
                dict(rstd=None), dict(C=0), dict(C=-4), dict(C=513, ldx=520, ldy=520), dict(B=-1), dict(ldx=7), dict(ldy=7),
                dict(x=p + 2), dict(y=p + 1), dict(ptr=q + 2), dict(mu=p + 2), dict(act=7)):
        assert fwd(**bad) == E_ARG, bad
        assert b"graphnorm_seg_fwd" in lib.glass_last_error_string()
    for bad in (dict(dy=None), dict(x=None), dict(dx=None), dict(ptr=None), dict(gamma=None), dict(alpha=None), dict(mu=None),
                dict(rstd=None), dict(ws=None), dict(C=0), dict(C=513, lddy=520, ldx=520, lddx=520), dict(B=-1), dict(lddy=7),
                dict(ldx=7), dict(lddx=7), dict(dy=p + 2), dict(dx=p + 1), dict(dg=p + 2), dict(ws=w + 4), dict(act=7),
                dict(beta=None, act=1)):
        assert bwd(**bad) == E_ARG, bad
        assert b"graphnorm_seg_bwd" in lib.glass_last_error_string()


def test_symbols_and_header_lines():
    from glass_amd import _lib
    lib = _lib.load()
    for name in ENTRIES + QUERIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    text = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    for name in ENTRIES + QUERIES:
        m = re.search(r"\b" + name + r"\s*\([^;]*;[ \t]*/\*([^\n]*)\*/", text)
        assert m, f"{name}: no trailing comment on its declaration"
        assert "GNNSeg.py:103-104,118" in m.group(1) and "impl/models.py:51,60" in m.group(1)
    assert lib.glass_version() == 6
