"""Per-graph GraphNorm on the MI355X (glass_amd/csrc/graphnorm_seg.hip, ops.graphnorm_seg, models.GraphNorm(x, batch))
against the fp64 restatement of tests/graphnorm_seg_oracle.py.  Data are 5 + 2 randn (the hard case for a one-pass
variance), gamma / beta / alpha random with alpha != 1; the tolerance is the project's rel-inf 1e-5 on y, dx and the three
parameter gradients."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import graphnorm_seg_oracle as GO  # noqa: E402
from helpers import rel_inf  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-5  # TOL of tests/test_gpu_kernels.py
KEYS = ("y", "dx", "dgamma", "dbeta", "dalpha")


def _lds_rows(C):
    from glass_amd import _lib
    L = _lib.load().glass_graphnorm_seg_lds_rows(C)
    assert L >= 2
    return L


def _mixed_sizes(C):
    """Sizes where the kernel can go wrong: fewer rows than row slots, around one wave of rows, both sides of the LDS staging
    limit; an empty segment first, in the middle and last."""
    L = _lds_rows(C)
    return [0, 1, 2, 3, 0, 63, 64, 65, 0, L - 1, L, L + 1, 1, 0]


def _inputs(sizes, C, seed):
    gen = torch.Generator().manual_seed(seed)
    n = int(sum(sizes))
    x = torch.randn(n, C, generator=gen) * 2.0 + 5.0
    gamma = 1 + 0.3 * torch.randn(C, generator=gen)
    beta = 0.2 * torch.randn(C, generator=gen)
    alpha = 1 + 0.3 * torch.randn(C, generator=gen)
    alpha[(alpha - 1).abs() < 0.05] = 1.25  # alpha != 1, and not by a rounding error
    gout = torch.randn(n, C, generator=gen)
    return x, gamma, beta, alpha, gout


@functools.lru_cache(maxsize=None)
def _case(sizes, C, seed=0, act=0):
    """(inputs, fp64 reference): computed once per (sizes, C, seed, act) and shared by the tests; never modified."""
    inp = _inputs(sizes, C, seed)
    return inp, GO.reference(inp[0], GO.seg_ptr_of(sizes), *inp[1:4], inp[4], act=act)


def _run(inp, sizes, act=0, pad=0, prefill=None):
    """One forward + backward on the GPU -> dict of KEYS (+ mu, rstd).  pad: extra columns of the row pitch of x.
    prefill: the parameter gradients start at these values and are accumulated into (direct)."""
    from glass_amd import ops
    x, gamma, beta, alpha, gout = inp
    n, C = x.shape
    ptr = GO.seg_ptr_of(sizes).to(torch.int32).to(DEV)
    wide = torch.zeros(n, C + pad)
    wide[:, :C] = x
    xw = wide.to(DEV).requires_grad_(True)
    params = [t.to(DEV).requires_grad_(True) for t in (gamma, beta, alpha)]
    if prefill is not None:
        for p, g in zip(params, prefill):
            p.grad = g.to(DEV).clone()
    y = ops.graphnorm_seg(xw[:, :C] if pad else xw, ops.SegPtr(ptr), *params, 1e-5, act, direct=prefill is not None)
    stats = y.grad_fn.saved_tensors[-1]
    y.backward(gout.to(DEV))
    torch.cuda.synchronize()
    out = {"y": y.detach(), "dx": xw.grad[:, :C], "dgamma": params[0].grad, "dbeta": params[1].grad, "dalpha": params[2].grad,
           "mu": stats[0], "rstd": stats[1]}
    return {k: v.cpu() for k, v in out.items()}


def _check(got, ref, label):
    errs = {k: rel_inf(got[k], ref[k]) for k in KEYS}
    print(label, {k: f"{v:.2e}" for k, v in errs.items()})
    for k in KEYS:
        assert errs[k] <= TOL, (label, k, errs[k])


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("C", [64, 8, 17, 20, 128, 256])
def test_segment_sizes_and_widths(C):
    sizes = tuple(_mixed_sizes(C))
    inp, ref = _case(sizes, C)
    got = _run(inp, sizes)
    _check(got, ref, f"C={C}")
    mu, rstd = GO.stats(inp[0], GO.seg_ptr_of(sizes), inp[3])
    assert rel_inf(got["mu"], mu) <= TOL and rel_inf(got["rstd"], rstd) <= TOL


@pytest.mark.parametrize("pad", [4, 1])
def test_row_pitch_wider_than_the_rows(pad):
    """ldx = C + 4 keeps the 16-byte accesses; ldx = C + 1 forces element loads at C = 64 — same layout, same sums: the two
    give the bits of the contiguous call."""
    sizes = tuple(_mixed_sizes(64))
    inp, ref = _case(sizes, 64)
    got = _run(inp, sizes, pad=pad)
    _check(got, ref, f"ldx=C+{pad}")
    plain = _run(inp, sizes)
    for k in KEYS + ("mu", "rstd"):
        assert _bits(got[k], plain[k]), k


@pytest.mark.parametrize("rows", [300, None])
def test_single_segment_matches_the_whole_graph_path(rows):
    from glass_amd import ops
    C = 64
    sizes = (rows if rows is not None else _lds_rows(C) + 1, )
    inp, ref = _case(sizes, C, seed=3)
    got = _run(inp, sizes)
    _check(got, ref, f"B=1 rows={sizes[0]}")
    x, gamma, beta, alpha, gout = inp
    xg = x.to(DEV).requires_grad_(True)
    params = [t.to(DEV).requires_grad_(True) for t in (gamma, beta, alpha)]
    y = ops.graphnorm(xg, *params, 1e-5, 0)
    y.backward(gout.to(DEV))
    whole = {"y": y.detach().cpu(), "dx": xg.grad.cpu(), "dgamma": params[0].grad.cpu(), "dbeta": params[1].grad.cpu(),
             "dalpha": params[2].grad.cpu()}
    for k in KEYS:  # two orders of summation: to tolerance, not bitwise
        assert rel_inf(got[k], whole[k].double()) <= TOL, k


def test_many_segments_fold_in_several_rounds():
    """700 segments: more than the 16 segment slots x 8 partials in flight one round of the second launch takes."""
    gen = torch.Generator().manual_seed(9)
    sizes = tuple(torch.randint(1, 41, (700, ), generator=gen).tolist())
    inp, ref = _case(sizes, 64, seed=4)
    _check(_run(inp, sizes), ref, "B=700")


@pytest.mark.parametrize("act", [0, 1, 2])
def test_activations(act):
    sizes = (0, 1, 7, 70, _lds_rows(20) + 3, 0, 2)
    inp, ref = _case(sizes, 20, seed=5, act=act)
    _check(_run(inp, sizes, act=act), ref, f"act={act}")


def test_bitwise_repeatable():
    sizes = tuple(_mixed_sizes(64))
    inp, _ = _case(sizes, 64)
    a, b = _run(inp, sizes, act=1), _run(inp, sizes, act=1)
    for k in KEYS + ("mu", "rstd"):
        assert _bits(a[k], b[k]), k


def test_position_invariance_bitwise():
    """Three segments (5, 64 and L + 1 rows) as a batch of their own, and embedded in another order between the segments of
    the mixed batch: y, mu, rstd and dx of their rows are the same bits."""
    C = 64
    L = _lds_rows(C)
    own = (5, 64, L + 1)
    x, gamma, beta, alpha, gout = _inputs(own, C, seed=6)
    cut = [0, 5, 69, 69 + L + 1]
    a = _run((x, gamma, beta, alpha, gout), own, act=1)
    others = _mixed_sizes(C)
    ox, _, _, _, og = _inputs(tuple(others), C, seed=7)
    # (b): others[0:4], own[2], others[4:7], own[0], others[7:11], own[1], others[11:]
    order = [("o", 0, 4), ("w", 2), ("o", 4, 7), ("w", 0), ("o", 7, 11), ("w", 1), ("o", 11, len(others))]
    optr = GO.seg_ptr_of(others).tolist()
    sizes_b, xs, gs, where, row = [], [], [], {}, 0
    for item in order:
        if item[0] == "o":
            lo, hi = optr[item[1]], optr[item[2]]
            sizes_b += others[item[1]:item[2]]
            xs.append(ox[lo:hi]), gs.append(og[lo:hi])
            row += hi - lo
        else:
            k = item[1]
            where[k] = (len(sizes_b), row)
            sizes_b.append(own[k])
            xs.append(x[cut[k]:cut[k + 1]]), gs.append(gout[cut[k]:cut[k + 1]])
            row += own[k]
    b = _run((torch.cat(xs), gamma, beta, alpha, torch.cat(gs)), tuple(sizes_b), act=1)
    for k in range(3):
        seg, r0 = where[k]
        for key in ("y", "dx"):
            assert _bits(a[key][cut[k]:cut[k + 1]], b[key][r0:r0 + own[k]]), (k, key)
        for key in ("mu", "rstd"):
            assert _bits(a[key][k], b[key][seg]), (k, key)


def test_accumulate_adds_to_prefilled_gradients():
    sizes = tuple(_mixed_sizes(64))
    inp, ref = _case(sizes, 64)
    gen = torch.Generator().manual_seed(8)
    pre = [torch.randn(64, generator=gen) * 10 for _ in range(3)]
    got = _run(inp, sizes, prefill=pre)
    for k, p in zip(("dgamma", "dbeta", "dalpha"), pre):
        assert rel_inf(got[k], ref[k] + p.double()) <= TOL, k
    assert rel_inf(got["dx"], ref["dx"]) <= TOL


def _sync_checks_work():
    torch.cuda.set_sync_debug_mode("error")
    try:
        torch.ones(1, device=DEV).item()
    except RuntimeError:
        return True
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return False


def test_module_batch_vector_and_segment_pointers(monkeypatch):
    """GraphNorm(C)(x, batch) and GraphNorm(C)(x, SegPtr) are the same bits, and right.  With batch_size= nothing is read
    back: the call runs under torch.cuda.set_sync_debug_mode("error") where this torch flags a synchronising read (checked
    first on a .item()), and in any case with Tensor.tolist / .item / .cpu replaced by functions that raise — the only
    ways models._seg_ptr_of could look at device data."""
    from glass_amd import models, ops
    C = 20
    sizes = (3, 0, 41, 1, 0, 0, 9)
    inp, ref = _case(sizes, C, seed=10)
    x, gamma, beta, alpha, gout = inp
    gn = models.GraphNorm(C).to(DEV)
    with torch.no_grad():
        gn.weight.copy_(gamma), gn.bias.copy_(beta), gn.mean_scale.copy_(alpha)
    ptr = GO.seg_ptr_of(sizes)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), ptr[1:] - ptr[:-1]).to(DEV)
    xg = x.to(DEV)
    outs = {}
    # trailing empty graphs are invisible in a batch vector: the count of graphs needs batch_size= (or ends at batch[-1] + 1)
    for name, arg, kw in (("ptr", ops.SegPtr(ptr.to(torch.int32).to(DEV)), {}), ("vec", batch, {}),
                          ("vec_bs", batch, {"batch_size": len(sizes)})):
        xi = xg.clone().requires_grad_(True)
        gn.zero_grad()
        y = gn(xi, arg, **kw)
        y.backward(gout.to(DEV))
        outs[name] = {"y": y.detach().cpu(), "dx": xi.grad.cpu(), "dgamma": gn.weight.grad.cpu().clone(),
                      "dbeta": gn.bias.grad.cpu().clone(), "dalpha": gn.mean_scale.grad.cpu().clone()}
    _check(outs["ptr"], ref, "module")
    for name in ("vec", "vec_bs"):
        for k in KEYS:
            assert _bits(outs[name][k], outs["ptr"][k]), (name, k)
    with pytest.raises(ValueError, match="sorted"):
        gn(xg, batch.flip(0))

    def boom(*a, **k):
        raise AssertionError("device data was read back")

    strict = _sync_checks_work()
    with monkeypatch.context() as m:
        for name in ("tolist", "item", "cpu"):
            m.setattr(torch.Tensor, name, boom)
        if strict:
            torch.cuda.set_sync_debug_mode("error")
        try:
            with torch.no_grad():
                y = gn(xg, batch, batch_size=len(sizes))
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert _bits(y.cpu(), outs["ptr"]["y"])
