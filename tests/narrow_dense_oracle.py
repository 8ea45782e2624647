"""fp64 restatement of the narrow dense family (glass_amd/csrc/dense_narrow.hip, hidden <= 32), shared by
tests/test_narrow_dense_host.py (checked there against torch fp64 autograd and the library's host-side geometry) and
tests/test_gpu_narrow_dense.py (the kernels against it).  Plain torch fp64 written out from the formulas in the kernels'
comments; nothing here calls the library.

  pair      T = [xa || xb] W^T + b  (W [2H, K], K = H for the trans pair, 2H for the comb pair), A = act(T),
            out = z A1 + (1 - z) A0 on labelled rows, (1 - z) A1 + z A0 on the others  (A1 = A[:, :H], A0 = A[:, H:])
  backward  dZ[n, o] = coef(n, o < H) * dsrc[n, o mod H] * act'(T[n, o]);  din = dZ W[:, :n_out] (+ addend);
            dW = dZ^T [xa || xb], db = sum_n dZ
  fusions   per-workgroup column sums of `out` (sum v, sum v^2); GraphNorm apply while loading (saved = [mean, rstd, scale,
            shift]); the backward column sums of a GraphNorm whose output gradient the data gradient is (sum gp, sum gp xhat)

Every sum also comes with the sum of the absolute values of its terms: the kernels add exact doubles of fp32 terms (or fp32
fma chains), so a sum is graded against what its terms can be wrong by, per column, never against another column's size.
"""
import torch

ACT_NONE, ACT_ELU = 0, 1
ROWS = 256   # rows per forward / data-gradient workgroup = rows per statistics partial (kNarrowRows)
SLAB = 64    # rows per weight-gradient slab (kNarrowSlab)

# ---- the shapes of the GPU tests, by the geometry each is named for ------------------------------------------------------------
HP_STEPS = (8, 12, 16, 20, 24, 28, 32)        # register widths of GLASS_NARROW_DISPATCH
SWEEP_WIDTHS = tuple(range(1, 33))            # every H: each instantiation at H = HP and at every H below it
SWEEP_N = 321                                 # two workgroups (the second with 65 rows), six slabs (the last with one row)
ROW_WIDTHS = (1, 8, 17, 20, 32)
ROW_SWEEP = {                                 # N: (weight-gradient slabs, forward / data-gradient workgroups)
    1: (1, 1), 63: (1, 1), 64: (1, 1), 65: (2, 1), 255: (4, 1), 256: (4, 1), 257: (5, 2), 1024: (16, 4), 1025: (17, 5),
    4096: (64, 16), 4097: (65, 17)}


def hp_of(H):
    """the instantiation GLASS_NARROW_DISPATCH picks for hidden size H"""
    return next(hp for hp in HP_STEPS if H <= hp)


def wgrad_stride(O, I):
    """floats of one slab's partial: dW[O][I] then db[O], rounded up to 4"""
    return -(-(O * I + O) // 4) * 4


def blocks(n, rows):
    return -(-n // rows)


# ---- activation ------------------------------------------------------------------------------------------------------------
def act_fn(act, t):
    if act == ACT_NONE:
        return t
    return torch.where(t > 0, t, torch.expm1(t))


def act_grad(act, t):
    """derivative from the PRE-activation value"""
    if act == ACT_NONE:
        return torch.ones_like(t)
    return torch.where(t > 0, torch.ones_like(t), torch.exp(t))


def _lab(mask):
    return mask.reshape(-1, 1) != 0


# ---- forward ---------------------------------------------------------------------------------------------------------------
def fwd(xa, xb, W, b, mask, z, act):
    """T [N, 2H], out [N, H]"""
    x = xa.double() if xb is None else torch.cat((xa.double(), xb.double()), 1)
    W, b = W.double(), b.double()
    H = W.shape[0] // 2
    T = x @ W.t() + b
    A = act_fn(act, T)
    A1, A0 = A[:, :H], A[:, H:]
    out = torch.where(_lab(mask), z * A1 + (1 - z) * A0, (1 - z) * A1 + z * A0)
    return T, out


def block_sums(term, rows=ROWS):
    """[ceil(N / rows), C]: the column sums of each block of `rows` rows"""
    n, C = term.shape
    nb = blocks(n, rows)
    pad = torch.zeros(nb * rows, C, dtype=torch.float64)
    pad[:n] = term.double()
    return pad.reshape(nb, rows, C).sum(1)


def stats(out, rows=ROWS):
    """[ceil(N / rows), 2, H]: per-block sum v and sum v^2"""
    v = out.double()
    return torch.stack((block_sums(v, rows), block_sums(v * v, rows)), 1)


def stats_abs(out, rows=ROWS):
    """the same sums over the absolute values of the terms"""
    v = out.double()
    return torch.stack((block_sums(v.abs(), rows), block_sums(v * v, rows)), 1)


def prologue(x, saved, act):
    """act(x * scale + shift), saved = [mean, rstd, scale, shift] ([4H]); dropout is not restated: the tests take the mask from
    the kernel's own side output"""
    H = x.shape[1]
    s = saved.double()
    return act_fn(act, x.double() * s[2 * H:3 * H] + s[3 * H:4 * H])


# ---- backward --------------------------------------------------------------------------------------------------------------
def dz(dsrc, T, mask, z, act):
    """dZ [N, 2H]"""
    d = dsrc.double()
    c1 = torch.where(_lab(mask), torch.tensor(float(z), dtype=torch.float64), torch.tensor(1.0 - float(z), dtype=torch.float64))
    g = torch.cat((c1 * d, (1 - c1) * d), 1)
    if act != ACT_NONE:
        g = g * act_grad(act, T.double())
    return g


def dgrad(dsrc, T, W, mask, z, act, n_out, addend=None):
    """dZ W[:, :n_out] (+ addend): [N, n_out]"""
    out = dz(dsrc, T, mask, z, act) @ W.double()[:, :n_out]
    return out if addend is None else out + addend.double()


def gn_terms(g, x, saved, alpha, act, keep_scale=None):
    """(gp, gp * xhat) [N, H] each: gp = g * keep_scale * act'(x * scale + shift), xhat = (x - alpha * mean) * rstd"""
    H = x.shape[1]
    s, x = saved.double(), x.double()
    gp = g.double()
    if keep_scale is not None:
        gp = gp * keep_scale.double()
    gp = gp * act_grad(act, x * s[2 * H:3 * H] + s[3 * H:4 * H])
    xhat = (x - alpha.double() * s[:H]) * s[H:2 * H]
    return gp, gp * xhat


def gn_partials(g, x, saved, alpha, act, keep_scale=None, rows=ROWS):
    """[ceil(N / rows), 2, H]: per-block sum gp and sum gp * xhat"""
    a, b = gn_terms(g, x, saved, alpha, act, keep_scale)
    return torch.stack((block_sums(a, rows), block_sums(b, rows)), 1)


def gn_partials_abs(g, x, saved, alpha, act, keep_scale=None, rows=ROWS):
    a, b = gn_terms(g, x, saved, alpha, act, keep_scale)
    return torch.stack((block_sums(a.abs(), rows), block_sums(b.abs(), rows)), 1)


def wgrad(dsrc, T, mask, z, act, xa, xb):
    """dW = dZ^T [xa || xb]  [2H, I],  db = sum_n dZ  [2H]"""
    g = dz(dsrc, T, mask, z, act)
    x = xa.double() if xb is None else torch.cat((xa.double(), xb.double()), 1)
    return g.t() @ x, g.sum(0)


def wgrad_abs(dsrc, T, mask, z, act, xa, xb):
    """sum_n |dZ x| per element of dW, sum_n |dZ| per element of db"""
    g = dz(dsrc, T, mask, z, act).abs()
    x = (xa.double() if xb is None else torch.cat((xa.double(), xb.double()), 1)).abs()
    return g.t() @ x, g.sum(0)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def make_mask(pattern, n, gen):
    if pattern == "none":
        m = torch.zeros(n, dtype=torch.bool)
    elif pattern == "all":
        m = torch.ones(n, dtype=torch.bool)
    elif pattern == "last":
        m = torch.zeros(n, dtype=torch.bool)
        m[-1] = True
    else:
        m = torch.rand(n, generator=gen) < 0.3
    return m.to(torch.uint8)


def make_pair(H, N, comb, seed=0, pattern="random"):
    """fp32 CPU inputs of one pair: dict with xa, xb (None for the trans pair), W, b, mask, dsrc, addend, act, n_out"""
    gen = torch.Generator().manual_seed(1000 * H + N + (500000 if comb else 0) + seed)
    K = 2 * H if comb else H
    d = {"H": H, "N": N, "comb": comb, "act": ACT_NONE if comb else ACT_ELU, "n_out": K, "K": K}
    d["W"] = torch.randn(2 * H, K, generator=gen) / K**0.5
    d["b"] = torch.randn(2 * H, generator=gen) * 0.1
    d["xa"] = torch.randn(N, H, generator=gen)
    d["xb"] = torch.randn(N, H, generator=gen) if comb else None
    d["mask"] = make_mask(pattern, N, gen)
    d["dsrc"] = torch.randn(N, H, generator=gen)
    d["addend"] = torch.randn(N, K, generator=gen)
    if N == 1:
        # A column sum of one row is that row's value: graded against TOL * |value| it must not be the small difference of
        # large products (fp32 rounds each product to 2^-24 of ITS size).  Non-negative operands keep every such value as
        # large as the products it is made of; the signs are exercised at every other row count.
        for k in ("W", "b", "xa", "xb"):
            d[k] = None if d[k] is None else d[k].abs()
    return d
