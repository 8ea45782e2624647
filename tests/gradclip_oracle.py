"""torch restatement of K9c (glass_amd/csrc/gradclip.hip, include/glass_hip.h): the global gradient norm, the clip coefficient
and the clipped single-tensor Adam update, shared by tests/test_gradclip_host.py (checked there against
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the CPU) and tests/test_gpu_gradclip.py (the kernels against it).

Everything works on ONE flat tensor — the update is elementwise, so a model's parameters enter concatenated.  `dtype` is the
working precision: torch.float32 restates the kernels (fp64 sum of squares, the norm rounded to fp32, everything after it in
fp32); torch.float64 is the same formulas in double, for the comparison with a torch run in double."""
import math

import torch


def global_norm(grad, dtype=torch.float32):
    """sqrt(sum g^2) with squares and sum in fp64, rounded to `dtype`."""
    return torch.sqrt((grad.double() ** 2).sum()).to(dtype)


def clip_coef(norm, max_norm):
    """clip_grad_norm_'s coefficient in norm's dtype: clamp(max_norm / (norm + 1e-6), max = 1); NaN stays NaN.  The quotient is
    ONE correctly rounded division, as the kernel's (tensor / tensor; torch's `float / tensor`, which clip_grad_norm_ itself
    writes, evaluates reciprocal * float — two roundings, up to an ulp away)."""
    return torch.clamp(torch.as_tensor(max_norm, dtype=norm.dtype) / (norm + 1e-6), max=1.0)


def clipped_adam_step(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay, coef):
    """One update, `step` = the 1-based number of this update.  Returns (p, g_scaled, m, v) as new tensors of p's dtype.
    Order: scale the raw gradient by coef, THEN add weight_decay * p (clip first, the optimizer adds the decay); moments and
    parameter as torch.optim.Adam's single-tensor form (common.h: adam_element) — bias corrections evaluated in double,
    step size and sqrt(bias_correction2) rounded to the working dtype."""
    dt = p.dtype
    coef = torch.as_tensor(coef, dtype=dt)
    gs = g * coef
    gk = gs + weight_decay * p if weight_decay != 0 else gs
    m = m + (1.0 - torch.tensor(beta1, dtype=dt)) * (gk - m)
    v = v * torch.tensor(beta2, dtype=dt) + (1.0 - torch.tensor(beta2, dtype=dt)) * gk * gk
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    step_size = torch.tensor(lr / bc1, dtype=dt)
    bc2_sqrt = torch.tensor(math.sqrt(bc2), dtype=dt)
    denom = torch.sqrt(v) / bc2_sqrt + torch.tensor(eps, dtype=dt)
    p = p - step_size * (m / denom)
    return p, gs, m, v


def clipped_run(p0, grads, max_norm, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    """len(grads) clipped Adam steps from zero moments on flat tensors; returns (p, [(norm, coef) per step])."""
    dt = p0.dtype
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    seen = []
    for t, g in enumerate(grads, 1):
        norm = global_norm(g, dt)
        coef = clip_coef(norm, max_norm)
        p, _gs, m, v = clipped_adam_step(p, g.to(dt), m, v, t, lr, beta1, beta2, eps, weight_decay, coef)
        seen.append((float(norm), float(coef)))
    return p, seen
