"""fp64 restatement of the training step's tail launches, shared by tests/test_step_tail_host.py (checked there against torch
fp64 autograd and the library's host-side plan builder) and tests/test_gpu_step_tail.py (the kernels against it):

  * the index vectors of the selection product, chosen by the K1 plan they give (spmm.hip: glass_spmm_plan_build);
  * GraphNorm(Embedding(x)) backward: fp64 autograd, and the table form the kernels use (embnorm.hip) restated in fp64;
  * the hand-built parameter arena of the fused tail (glass_embed_norm_bwd_adam_f32) and a well-conditioned Adam state for it.
"""
import ctypes

import numpy as np
import torch

EPS = 1e-5
HDR_SWEEP, HDR_ITEMS, HDR_REDUCE, HDR_SLOTS, HDR_OFF_REDUCE = 4, 5, 6, 7, 12


# ---- index vectors ----------------------------------------------------------------------------------------------------------
def _from_counts(counts, seed):
    x = np.repeat(np.arange(len(counts)), counts)
    return torch.from_numpy(np.random.default_rng(seed).permutation(x).astype(np.int64))


def _spread(total, rows, seed):
    """`rows` counts that add up to `total`, each within a few of total / rows"""
    rng = np.random.default_rng(seed)
    c = np.full(rows, total // rows)
    c[:total - c.sum()] += 1
    for _ in range(rows):
        a, b = rng.integers(0, rows, 2)
        d = min(int(rng.integers(0, 9)), c[a] - 1)
        c[a] -= d
        c[b] += d
    return c


def index_vector(name):
    """(x int64 [n], V).  By plan:
    long_cut    V = 40, n = 3000: every row a workgroup item; row counts 0, 1, exactly 256 (one chunk), 257 (two), 700 (three);
                rows 0 and 39 unused.
    long_nocut  V = 8, n = 1024: every row a workgroup item of at most 256 entries: nothing to reduce.
    sweep       V = 1024, n = 5000: short rows swept by waves; one row of 700 entries is cut in two; rows 1000.. unused.
    v1 v3 v200  plain tables of 1 / 3 / 200 rows without a cut row;  v64c v65c  64 / 65 rows with one row of 600 entries (cut):
                the two sides of the tail's register path (V <= 64)."""
    if name == "long_cut":
        counts = np.concatenate([[0, 1, 256, 257, 700], _spread(3000 - 1214, 34, 1), [0]])
    elif name == "long_nocut":
        counts = np.array([256, 256, 200, 100, 0, 56, 128, 28])
    elif name == "sweep":
        counts = np.concatenate([[700], _spread(5000 - 700, 999, 2), np.zeros(24, dtype=np.int64)])
    elif name == "v1":
        counts = np.array([100])
    elif name == "v3":
        counts = np.array([90, 0, 110])
    elif name == "v200":
        counts = np.concatenate([_spread(3000, 199, 3), [0]])
    elif name in ("v64c", "v65c"):
        V = int(name[1:3])
        counts = np.concatenate([[600], _spread(1400, V - 2, V), [0]])
    else:
        raise KeyError(name)
    counts = np.asarray(counts, dtype=np.int64)
    return _from_counts(counts, len(counts)), len(counts)


# what the plan header must say for each vector: (sweep items > 0, reduce rows > 0)
PLAN_KIND = {"long_cut": (False, True), "long_nocut": (False, False), "sweep": (True, True), "v1": (False, False),
             "v3": (False, False), "v200": (True, False), "v64c": (True, True), "v65c": (True, True)}


def rowptr_of(x, V):
    rp = np.zeros(V + 1, dtype=np.int32)
    rp[1:] = np.cumsum(np.bincount(x.numpy(), minlength=V))
    return rp


def host_plan(lib, x, V):
    """The K1 plan of the selection matrix of x, from the library's host-side builder (no GPU involved)."""
    rp = rowptr_of(x, V)
    words = ctypes.c_int64(0)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, V, None, ctypes.byref(words)) == 0
    plan = np.zeros(words.value, dtype=np.int32)
    assert lib.glass_spmm_plan_build(rp.ctypes.data, V, plan.ctypes.data, ctypes.byref(words)) == 0
    return plan


def reduce_list(plan):
    """[(row, first slot, number of slots)] of the rows the plan cuts into several chunks"""
    off, n = int(plan[HDR_OFF_REDUCE]), int(plan[HDR_REDUCE])
    return [tuple(int(v) for v in plan[off + 3 * i:off + 3 * i + 3]) for i in range(n)]


def model_inputs(name, H, scale=8.0):
    """(x, V, W, gamma, beta, alpha, gout) on the host for index vector `name` at width H: table entries of 0.5 .. 2 in
    magnitude with both signs, emb_gn's weight and bias in 0.5 .. 1.5 (no parameter near 0, where an Adam step would cancel
    it), mean_scale in 0.5 .. 0.9 (a one-row table is W (1 - alpha) after centring: alpha near 1 would leave fp32 rounding), output gradients of scale 8 (table gradients well above weight_decay * W).
    V = 1: every node holds the same row, the centred value c = W (1 - alpha) is the whole variance, and the table's gradient is
    gamma rstd G eps / (c^2 + eps) — what is left when two terms of size gamma rstd G cancel.  With |c| ~ 0.5 that is 4e-5 of
    the terms, and ANY fp32 evaluation (torch's fp32 autograd included: 2e-3 from its own fp64 run) returns its rounding; the
    table is scaled to |W| ~ 0.01 there, so that c^2 is of eps's size and the gradient a fifth of the terms or more."""
    x, V = index_vector(name)
    gen = torch.Generator().manual_seed(H + V)
    sign = torch.where(torch.rand(V, H, generator=gen) < 0.5, -1.0, 1.0)
    W = sign * (0.5 + 1.5 * torch.rand(V, H, generator=gen))
    if V == 1:
        W = W * 0.01
    gamma, beta = (0.5 + torch.rand(H, generator=gen) for _ in range(2))
    alpha = 0.5 + 0.4 * torch.rand(H, generator=gen)
    gout = scale * torch.randn(x.shape[0], H, generator=gen)
    return x, V, W, gamma, beta, alpha, gout


# ---- GraphNorm(Embedding(x)) backward -----------------------------------------------------------------------------------------
def selection_product(x, gout, V):
    """G[v] = sum of gout over the nodes that use table row v (fp64)"""
    return torch.zeros(V, gout.shape[1], dtype=torch.float64).index_add_(0, x, gout.double())


def autograd_grads(x, W, gamma, beta, alpha, gout):
    """(dW, dgamma, dbeta, dalpha) of sum(gout * GraphNorm(W[x])) by torch autograd in fp64 — the reference."""
    Wd, g, b, a = (t.double().clone().requires_grad_(True) for t in (W, gamma, beta, alpha))
    h = Wd[x]
    centred = h - h.mean(0, keepdim=True) * a
    y = g * centred / (centred.pow(2).mean(0, keepdim=True) + EPS).sqrt() + b
    y.backward(gout.double())
    return Wd.grad, g.grad, b.grad, a.grad


def table_form_grads(x, W, gamma, beta, alpha, gout):
    """The same four gradients the way the kernels compute them (embnorm.hip): from the [V, H] selection product G, the row
    counts and the table alone, never from the [n, H] node matrix.  In fp64."""
    V = W.shape[0]
    Wd, g, a = W.double(), gamma.double(), alpha.double()
    cnt = torch.bincount(x, minlength=V).double().reshape(-1, 1)
    n = float(x.shape[0])
    G = selection_product(x, gout, V)
    mu = (cnt * Wd).sum(0) / n
    centred = Wd - a * mu
    rstd = ((cnt * centred * centred).sum(0) / n + EPS).rsqrt()
    xhat = centred * rstd
    s1, s2 = G.sum(0), (G * xhat).sum(0)
    # dL/d centred[node] = g rstd (gout - xhat s2 / n); every node of row v shares xhat[v]
    dcent = g * rstd * (G - cnt * xhat * s2 / n)            # summed over the nodes of each row
    dmu = -(a * dcent.sum(0))                               # centred = h - a mu
    dW = dcent + cnt * dmu / n
    dalpha = -(mu * dcent.sum(0))
    return dW, s2, s1, dalpha


# ---- the arena of the fused tail ------------------------------------------------------------------------------------------------
def arena_layout(name, V, H):
    """(n_param, off_W, off_gamma, off_beta, off_alpha) — the table [V * H] and emb_gn's three vectors [H] inside a flat arena.
    first   table at offset 0, then (alpha, gamma, beta) back to back behind it
    middle  (beta, alpha, gamma) back to back, the table right behind them at an odd offset, other parameters on both sides
    last    gamma at offset 0, alpha alone in the middle, beta right in front of the table, the table ends at n_param
    tight   as `first`, 5 other elements in all: one workgroup for the rest of the arena
    stride  n_param = 2048 * 256 + 4099: the rest workgroups walk the arena in strides; the table lies across the first
            stride's end and the vectors at the arena's end"""
    T = V * H
    if name == "first":
        return T + 3 * H + 1237, 0, T + H, T + 2 * H, T
    if name == "middle":
        o = 301
        return o + 3 * H + T + 555, o + 3 * H, o + 2 * H, o, o + H
    if name == "last":
        n = 777 + 3 * H + T
        return n, n - T, 0, n - T - H, 400
    if name == "tight":
        return T + 3 * H + 5, 0, T + H, T + 2 * H, T
    if name == "stride":
        n = 2048 * 256 + 4099
        return n, 2048 * 256 - T // 2 - 3, n - H, n - 3 * H, n - 2 * H
    raise KeyError(name)


def tail_ranges(layout, V, H):
    n, oW, og, ob, oa = layout
    return {"W": (oW, oW + V * H), "gamma": (og, og + H), "beta": (ob, ob + H), "alpha": (oa, oa + H)}


def tail_adam_state(layout, V, H, params, grads, seed):
    """Four flat fp32 buffers {"p", "g", "m", "v"} of n_param elements in which no sum of the Adam update cancels (the 2 ulp
    comparison with tests/gradclip_oracle.py is only meaningful there; tests/test_gpu_gradclip.py: _adam_state): moments of an
    earlier run on gradients of the same sign and size (m ~ g / 4, v ~ (g / 4)^2), parameters of 0.5 .. 2 in magnitude.
    Outside the tail's ranges g is given (0.5 .. 2) and p takes its sign.  Inside them p is `params` (the model's table and
    emb_gn vectors {"W", "gamma", "beta", "alpha"}), the gradient is what the launch will produce — "g" holds NaN there — and
    the moments follow `grads` (its fp64 value): its sign (the parameter's where it is exactly 0: an unused table row, so the
    decay term adds) and max(|g|, 1) as the size, so that an element whose gradient happens to be small — where g + wd p
    may cancel — still ends with a first moment much larger than the rounding of that sum."""
    n = layout[0]
    gen = torch.Generator().manual_seed(seed)
    u = lambda: 0.5 + 1.5 * torch.rand(n, generator=gen)
    sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    g = u() * sign
    st = {"p": u() * sign, "g": g, "m": 0.25 * g * (0.5 + torch.rand(n, generator=gen)),
          "v": (0.25 * g) ** 2 * (0.5 + torch.rand(n, generator=gen))}
    for k, (lo, hi) in tail_ranges(layout, V, H).items():
        gr, p = grads[k].reshape(-1).float(), params[k].reshape(-1).float()
        size = 0.25 * torch.where(gr != 0, torch.sign(gr), torch.sign(p)) * gr.abs().clamp(min=1.0)
        st["p"][lo:hi] = p
        st["g"][lo:hi] = float("nan")
        st["m"][lo:hi] = size * (0.5 + torch.rand(hi - lo, generator=gen))
        st["v"][lo:hi] = size ** 2 * (0.5 + torch.rand(hi - lo, generator=gen))
    return st


def adam_step_contracted(p, g, m, v, step, lr, beta1, beta2, eps, weight_decay):
    """gradclip_oracle.clipped_adam_step(coef = 1) with every multiply-add the compiler may contract evaluated as ONE rounding
    (fp64 product and sum of fp32 operands, rounded to fp32 once): the other end of what a correct kernel may return.  A state
    on which this and the separately rounded form differ by more than the comparison's bound is badly conditioned."""
    import math
    f = lambda t: t.double()
    r = lambda t: t.float()
    b1, b2 = np.float32(beta1), np.float32(beta2)
    w1, w2 = float(np.float32(1) - b1), float(np.float32(1) - b2)
    gk = r(f(g) + float(np.float32(weight_decay)) * f(p)) if weight_decay != 0 else g
    m2 = r(f(m) + w1 * f(gk - m))
    v2 = r(float(b2) * f(v) + f(r(w2 * f(gk))) * f(gk))
    step_size = float(np.float32(lr / (1.0 - beta1 ** step)))
    bc2_sqrt = torch.tensor(math.sqrt(1.0 - beta2 ** step), dtype=torch.float32)
    denom = torch.sqrt(v2) / bc2_sqrt + torch.tensor(eps, dtype=torch.float32)
    p2 = r(f(p) - step_size * f(m2 / denom))
    return p2, m2, v2


def ulps(a, b):
    """largest |a - b| in units of b's spacing"""
    a, b = a.numpy(), b.numpy()
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b))))
