"""fp64 CPU restatement of the per-graph GraphNorm (PyG 1.7.2 GraphNorm.forward(x, batch)) for the tests of
glass_amd/csrc/graphnorm_seg.hip and its Python surface.  For every graph s with rows seg_ptr[s] .. seg_ptr[s + 1] - 1:

    mu  = sum_rows(x) / max(rows, 1)          (scatter_mean clamps the count)
    out = x - mean_scale * mu
    var = sum_rows(out^2) / max(rows, 1)
    y   = act(weight * out / sqrt(var + eps) + bias)

A plain loop over the graphs in torch double; gradients come from autograd on this very loop.  An empty graph has no rows
and takes no part.  Not placed under oracle/: it is the checker of this path only.
"""
import torch
import torch.nn.functional as F

ACTS = {0: lambda h: h, 1: F.elu, 2: F.relu}  # GLASS_ACT_NONE / _ELU / _RELU


def seg_ptr_of(sizes):
    ptr = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.as_tensor(sizes, dtype=torch.int64), 0)
    return ptr


def stats(x, seg_ptr, mean_scale, eps=1e-5):
    """(mu [B, C], rstd [B, C]) in fp64; an empty graph: mu = 0, rstd = 1 / sqrt(eps)."""
    x, a = x.double(), mean_scale.double()
    mus, rstds = [], []
    for s in range(len(seg_ptr) - 1):
        xs = x[int(seg_ptr[s]):int(seg_ptr[s + 1])]
        cnt = max(xs.shape[0], 1)
        mu = xs.sum(0) / cnt
        var = (xs - a * mu).pow(2).sum(0) / cnt
        mus.append(mu)
        rstds.append((var + eps).rsqrt())
    return torch.stack(mus), torch.stack(rstds)


def graphnorm_seg(x, seg_ptr, weight, bias, mean_scale, eps=1e-5, act=0):
    """y [n, C] in the dtype of x (hand it doubles); differentiable in x, weight, bias, mean_scale."""
    parts = []
    for s in range(len(seg_ptr) - 1):
        xs = x[int(seg_ptr[s]):int(seg_ptr[s + 1])]
        if xs.shape[0] == 0:
            continue
        cnt = max(xs.shape[0], 1)
        mu = xs.sum(0, keepdim=True) / cnt
        out = xs - mean_scale * mu
        var = out.pow(2).sum(0, keepdim=True) / cnt
        parts.append(weight * out / (var + eps).sqrt() + bias)
    y = torch.cat(parts) if parts else x[:0] * weight
    return ACTS[int(act)](y)


def reference(x, seg_ptr, gamma, beta, alpha, gout, eps=1e-5, act=0):
    """-> dict(y, dx, dgamma, dbeta, dalpha) in fp64 for fp32 (or fp64) inputs and the upstream gradient gout."""
    xd = x.double().requires_grad_(True)
    p = [t.double().clone().requires_grad_(True) for t in (gamma, beta, alpha)]
    y = graphnorm_seg(xd, seg_ptr, *p, eps=eps, act=act)
    y.backward(gout.double())
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return {"y": y.detach(), "dx": zero(xd), "dgamma": zero(p[0]), "dbeta": zero(p[1]), "dalpha": zero(p[2])}
