"""Host side of the tests of the LDS-tiled dense family (K5t: tiled_fwd_kernel / tiled_dgrad_kernel, glass_amd/csrc/dense_tiled.hip,
behind glass_dual_linear_fwd_f32 / glass_dual_linear_dgrad_f32) — torch fp64 and numpy on the CPU, no GPU: the input recipes, the
fp64 truth STAGE BY STAGE with the mass of every element, the dispatch restated (checked against the source text by
tests/test_tiled_dense_host.py) and fp32 restatements of the kernels' summation order in both product forms.

Scope.  The family serves, in the default build: the forward of the comb pair at hidden 128 and of both pairs at hidden 256 / 512,
and the data gradient of both pairs at hidden 256 / 512.  The hidden-128 trans forward and both hidden-128 data gradients left it
for the stage-run kernels of dense.hip (trans_fwd3 / trans_dgrad2 / trans_dgrad3 / comb_dgrad3): OUT OF SCOPE here — they are tested by
tests/staged_dense_oracle.py and tests/test_gpu_staged_dense.py — (`reaches_tiled` says so and the host test ties it to the entry's text).  The K5t weight gradients are not part of it.

Stages (every function -> (want, mass), fp64; each a function of what the kernel really read — its own upstream outputs as read
back where a stage consumes them —, so that one stage's rounding is left to bound; the pattern of tests/graphnorm_oracle.py, whose
stage_apply / stage_bwd_sums / gate are reused as they are):

  xa_out   from xa (gathered), saved, keep      keep * act(x * scale + shift)                    (|x scale| + |shift|) * keep
  T        from A (= xa_out read back), xb      Z = [A || xb] W^T + b                            sum_k |a_k| |w_k| + |b|
  out      from the same                        mix of act(Z1), act(Z0) by w1, w0 = z | 1 - z    |w1| mass(Z1) + |w0| mass(Z0)
  stats    from out (read back), per tile       sum o, sum o^2 over the tile's rows < N          sum |o|, sum o^2
  dgrad    from dsrc, T, W, addend, keep        (dZ @ Wstack + addend) * keep                    (sum_o |dZ_o| |W_o| + |addend|) * keep
  gn part  from dgrad out[:, :H] (read back)    sum g, sum g xhat per tile (graphnorm_oracle)    sum |g|, sum |g| (|x| + |a mu|) rstd

ELU and ReLU are Lipschitz 1: a mass passes through them unchanged.  act' in the data gradient is formed from the fp32 T the kernel
reads, so `T > 0` falls the same way in the truth: no kinks there; the GraphNorm partials inherit graphnorm_oracle's kink slack.
The gate is |got - want| <= 1e-5 * mass per element (readout_oracle.gate), the partials tile by tile, never summed first.

Product forms restated (restate_product): K steps of 16; f32 form — one fused multiply-add per k into the fp32 accumulator; split
form — each operand cut into three bf16 pieces (split_mma.h), six products per K step in its order (mid*mid, lo*hi, hi*lo, mid*hi,
hi*mid, hi*hi), the 16 k of one instruction summed exactly before the accumulator rounds.  The effective-weight form is one product
over W_unl = fl32((1-z) W1 + z W0) for the whole tile and, per labeled row, the correction (z - (1-z)) * (sum_k a_k (w1_k - w0_k)
(+ b1 - b0)) as a sequential fp32 sum."""
import os
import re

import numpy as np
import torch

import graphnorm_oracle as G
from readout_oracle import TOL, gate  # noqa: F401  (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
f32 = np.float32
ACT_NONE, ACT_ELU, ACT_RELU = 0, 1, 2
KSTEP = 16                          # kTK
TALL_TILES = 512                    # tall128: more than this many 64-row tiles
GRID_ROUND = 8                      # tiled_grid / tile_of_block: row tiles in groups of 8
MAXFIX_FWD, MAXFIX_DGRAD = 3, 7     # kMaxFix of the two kernels
WIDTHS = (128, 256, 512)            # tiled_shape_ok


def source_constants():
    """what the restatement depends on, read from the text of dense_tiled.hip and dense.hip"""
    rd = lambda n: open(os.path.join(ROOT, "glass_amd", "csrc", n)).read()
    t, d = rd("dense_tiled.hip"), rd("dense.hip")
    num = lambda pat, text: int(re.search(pat, text, re.S).group(1))
    fwd = re.search(r"void tiled_fwd_kernel\(.*?\n}\n", t, re.S).group(0)
    dg = re.search(r"void tiled_dgrad_kernel\(.*?\n}\n", t, re.S).group(0)
    fwd_entry = re.search(r'extern "C" int glass_dual_linear_fwd_f32\(.*?\n}\n', d, re.S).group(0)
    dg_entry = re.search(r"static int dgrad_launch\(.*?\n}\n", d, re.S).group(0)
    return {"kTK": num(r"constexpr int kTK = (\d+),", t), "kTThreads": num(r"kTThreads = (\d+);", t),
            "tiled_rows_text": "int tiled_rows(int64_t H) { return H == 128 ? 64 : 128; }" in t,
            "shape_text": "bool tiled_shape_ok(int64_t H) { return H == 128 || H == 256 || H == 512; }" in t,
            "tall_limit": num(r"static bool tall128\(int64_t N\) \{.*?tiled_split_products\(\) && ceil_div\(N, 64\) > (\d+);", t),
            "tall_launch_text": "if (H == 128 && tall128(N)) {" in t and "tiled_fwd_launch<128, 128, true>(" in t,
            "bm_text": "GLASS_TFWD(128, 64) GLASS_TFWD(256, 128) GLASS_TFWD(512, 128)" in t,
            "grid_round": num(r"static inline unsigned tiled_grid\(int64_t n_rowtiles, int nct\) \{ return \(unsigned\)\(ceil_div\(n_rowtiles, (\d+)\) \* \1 \* nct\); \}", t),
            "tile_of_block_text": all(s in t for s in ("const int b = blockIdx.x, grp = 8 * nct, r = b % grp;", "ct = r / 8;",
                                                       "rt = (b / grp) * 8 + (r % 8);", "return rt < n_rowtiles;")),
            "eff_block_text": all(s in fwd for s in ("const int per = (int)(gridDim.x / NCT);", "ct = (int)blockIdx.x / per;",
                                                     "rt = (int)blockIdx.x % per;", "if (pure && ct >= NCT / 2) return;")),
            "kMaxFix_fwd": num(r"constexpr int kMaxFix = (\d+);", fwd), "kMaxFix_dgrad": num(r"constexpr int kMaxFix = (\d+);", dg),
            "fwd_eff_cond_text": "if (EFF && act == GLASS_ACT_NONE && T == nullptr) {" in fwd,
            "dgrad_eff_cond_text": "if (EFF && act == GLASS_ACT_NONE) {" in dg,
            "pure_text": fwd.count("pure = n_fix <= kMaxFix;") == 1 and dg.count("pure = n_fix <= kMaxFix;") == 1,
            "eff_fwd_shape_text": "bool tiled_eff_fwd_shape(int64_t H, int64_t K) { return (H == 256 || H == 512) && K == 2 * H; }" in t,
            "eff_dgrad_shape_text": "bool tiled_eff_dgrad_shape(int64_t H, int64_t n_out) { return tiled_shape_ok(H) && n_out == 2 * H; }" in t,
            "half_partials_text": fwd.count("if (H == 128 && BM == 128) {") == 1 and "const int64_t part = 2 * (int64_t)rt + hw;" in fwd,
            "dgrad_widths_text": "if (H == 256) {" in t and "} else if (H == 512) {" in t and "GLASS_TDG1(128" not in t,
            # which (H, pair) leave the family in dense.hip's entries, and that the stage-run forms are compiled in
            "fwd_leave_text": "if (GLASS_TRANS_FWD_V2 && !comb && H == 128) {" in fwd_entry and "if (tiled_here(H)) {" in fwd_entry,
            "dgrad_leave_text": "if (GLASS_TRANS_DGRAD_V2 && H == 128 && n_out == H) {" in dg_entry and
                                "if (GLASS_COMB_DGRAD_V2 && H == 128 && n_out == 2 * H) {" in dg_entry,
            "v2_defaults": {k: num(r"#\s*define " + k + r" (\d)", d) for k in ("GLASS_TRANS_FWD_V2", "GLASS_TRANS_DGRAD_V2", "GLASS_COMB_DGRAD_V2")},
            "split_order": re.findall(r"GLASS_SMMA\((\d), (\d)\);", rd("split_mma.h"))}


# ---- dispatch restated ------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def reaches_tiled(H, comb, direction):
    """does (H, pair) run tiled_fwd_kernel ("fwd") / tiled_dgrad_kernel ("dgrad") in the default build"""
    if H not in WIDTHS:
        return False
    if direction == "fwd":
        return H != 128 or comb
    return H != 128


def tiled_rows(H):
    """rows per statistics partial"""
    return 64 if H == 128 else 128


def tall128(N, f32_products):
    return (not f32_products) and _cdiv(N, 64) > TALL_TILES


def tiled_grid(n_rt, nct):
    return _cdiv(n_rt, GRID_ROUND) * GRID_ROUND * nct


def tile_of_block(b, nct, n_rt):
    """-> (rt, ct) or None (an empty block of the rounded grid)"""
    grp = GRID_ROUND * nct
    r = b % grp
    ct, rt = r // GRID_ROUND, (b // grp) * GRID_ROUND + r % GRID_ROUND
    return (rt, ct) if rt < n_rt else None


def eff_fwd_shape(H, K):
    return H in (256, 512) and K == 2 * H


def eff_dgrad_shape(H, n_out):
    return H in WIDTHS and n_out == 2 * H


def labeled_per_tile(mask, N, BM):
    m = np.asarray(mask[:N]).astype(bool)
    return [int(m[t * BM:(t + 1) * BM].sum()) for t in range(_cdiv(N, BM))]


def fwd_form(H, comb, N, f32_products, act=ACT_NONE, has_T=False, mask=None):
    """the launch tiled_fwd takes: BM, product form, effective-weight image, grid, and per row tile "pure" (one product + repairs) or
    "two" (the two-weight product)"""
    assert reaches_tiled(H, comb, "fwd")
    BM = 128 if H != 128 or tall128(N, f32_products) else 64
    n_rt, nct = _cdiv(N, BM), H // 128
    eff = comb and eff_fwd_shape(H, 2 * H)
    eff_live = eff and act == ACT_NONE and not has_T
    paths = None
    if mask is not None:
        paths = ["pure" if eff_live and n <= MAXFIX_FWD else "two" for n in labeled_per_tile(mask, N, BM)]
    return dict(BM=BM, split=not f32_products, eff=eff, eff_live=eff_live, n_rt=n_rt, nct=nct, grid=tiled_grid(n_rt, nct),
                partial_rows=tiled_rows(H), n_partials=_cdiv(N, tiled_rows(H)), paths=paths)


def dgrad_form(H, n_out, N, f32_products, act=ACT_NONE, mask=None):
    assert reaches_tiled(H, n_out == 2 * H, "dgrad") and n_out in (H, 2 * H)
    BM, n_rt, nct = 128, _cdiv(N, 128), n_out // 256
    eff = eff_dgrad_shape(H, n_out)
    eff_live = eff and act == ACT_NONE
    paths = None
    if mask is not None:
        paths = ["pure" if eff_live and n <= MAXFIX_DGRAD else "two" for n in labeled_per_tile(mask, N, BM)]
    return dict(BM=BM, split=not f32_products, eff=eff, eff_live=eff_live, n_rt=n_rt, nct=nct, grid=tiled_grid(n_rt, nct),
                partial_rows=128, n_partials=n_rt, paths=paths)


# ---- recipes ----------------------------------------------------------------------------------------------------------------------
PATTERNS = ("none", "all", "row0", "row127", "last", "cap", "over", "cap_wave", "over_wave", "cap_split", "over_split", "cap_next_over")


def label_pattern(name, N, BM, kmax):
    """label bytes [N] for the effective-weight cases.  Patterns that need a whole tile use tile 1 when N has one, else tile 0; rows
    at or past N are dropped (the ragged tile keeps fewer)."""
    m = np.zeros(N, dtype=np.uint8)
    t0 = BM if N > BM else 0
    put = lambda rows: [m.__setitem__(r, 1) for r in rows if 0 <= r < N]
    if name == "all":
        m[:] = 1
    elif name == "row0":
        put([t0])
    elif name == "row127":
        put([t0 + BM - 1])
    elif name == "last":
        put([N - 1])
    elif name in ("cap", "over"):          # spread over the tile, both row waves
        k = kmax + (name == "over")
        put([t0 + (5 + 17 * i) % BM for i in range(k)])
    elif name in ("cap_wave", "over_wave"):    # inside one wave's 64 rows (the upper one)
        k = kmax + (name == "over_wave")
        put([t0 + 64 + 7 * i + 1 for i in range(k)])
    elif name in ("cap_split", "over_split"):  # across the two row waves, around the seam
        k = kmax + (name == "over_split")
        put([t0 + 64 - (k // 2) + i for i in range(k)])
    elif name == "cap_next_over":         # a tile at the cap next to a tile over it
        put([(5 + 17 * i) % BM for i in range(kmax)])
        put([BM + (3 + 11 * i) % BM for i in range(kmax + 1)])
    else:
        assert name == "none"
    return m


def recipe(H, N, comb, seed=0, n_out=None, V=37):
    """Deterministic fp32 inputs of one pair: xa, xb [N, H] (+ 2 guard rows of Inf / NaN kept apart in `guard`), W [2H, K], b [2H],
    dsrc [N, H], T [N, 2H] (a plausible pre-activation with both signs), addend [N, n_out], GraphNorm operands of width H, a 37-row
    table with indices.  Scale: weights 1 / sqrt(K), activations N(0, 1) + 0.25 (a mean, so column sums do not cancel to nothing)."""
    g = torch.Generator().manual_seed(1000 * H + N + 7 * seed + int(comb))
    K = 2 * H if comb else H
    n_out = K if n_out is None else n_out
    r = lambda *s: torch.randn(*s, generator=g)
    p = dict(H=H, N=N, comb=comb, K=K, n_out=n_out, V=V)
    p["xa"], p["xb"] = r(N, H) + 0.25, (r(N, H) - 0.25 if comb else None)
    p["W"], p["b"] = r(2 * H, K) / K**0.5, r(2 * H) * 0.3
    p["dsrc"], p["T"], p["addend"] = r(N, H), r(N, 2 * H) * 1.5, r(N, n_out)
    p["table"], p["index"] = r(V, H) + 0.25, torch.randint(0, V, (N, ), generator=g, dtype=torch.int64)
    p["index"][0], p["index"][-1] = V - 1, 0
    scale = (0.5 + torch.rand(H, generator=g)) * torch.where(torch.rand(H, generator=g) < 0.5, -1.0, 1.0)
    # shift of either sign with |shift| >= 0.5: the prologue's ELU is the hardware exponential minus one (act_fast), whose absolute
    # error near h -> 0- is that of exp(h) ~ 1 (2^-24) whatever |h|; an element whose whole mass |x scale| + |shift| lies below ~1e-2
    # cannot meet 1e-5 * mass through it (restate_prologue shows the same on the CPU), so the recipe keeps every mass above 0.5
    shift = (0.5 + 0.5 * torch.rand(H, generator=g)) * torch.where(torch.rand(H, generator=g) < 0.5, -1.0, 1.0)
    p["saved"] = torch.stack([r(H) * 0.2, 0.5 + torch.rand(H, generator=g), scale, shift]).float()   # mean, rstd, scale, shift
    p["alpha"], p["gn_x"] = 0.5 + torch.rand(H, generator=g), r(N, H) * 2.0 + 0.5
    return p


# ---- the fp64 truth ---------------------------------------------------------------------------------------------------------------
def zw(z):
    """(zr, omz) as the entries round them"""
    return float(f32(z)), float(f32(1.0 - z))


def stage_prologue(x, saved, gn_act, keep=None):
    """xa_out: graphnorm_oracle.stage_apply (h rounded once to fp32, as the kernel's fmaf)"""
    return G.stage_apply(x, saved.float(), gn_act, keep)


def stage_fwd(A, xb, W, b, mask, z, act):
    """-> dict T, T_m [N, 2H], out, out_m [N, H]"""
    X = A.to(F64) if xb is None else torch.cat([A.to(F64), xb.to(F64)], 1)
    W, b = W.to(F64), b.to(F64)
    H = W.shape[0] // 2
    T = X @ W.t() + b
    T_m = X.abs() @ W.abs().t() + b.abs()
    zr, omz = zw(z)
    lab = torch.as_tensor(np.asarray(mask)).bool().reshape(-1, 1)
    w1 = torch.where(lab, torch.tensor(zr, dtype=F64), torch.tensor(omz, dtype=F64))
    w0 = torch.where(lab, torch.tensor(omz, dtype=F64), torch.tensor(zr, dtype=F64))
    a = G.act_f(T, act)
    out = w1 * a[:, :H] + w0 * a[:, H:]
    out_m = w1.abs() * T_m[:, :H] + w0.abs() * T_m[:, H:]
    return dict(T=T, T_m=T_m, out=out, out_m=out_m)


def stage_stats(out, N, rows):
    """[n_partials, 2, H] from the out the kernel wrote (read back): sum, sum of squares of the partial's own rows"""
    o = out.to(F64)[:N]
    n = _cdiv(N, rows)
    want = torch.stack([torch.stack([o[t * rows:(t + 1) * rows].sum(0), (o[t * rows:(t + 1) * rows]**2).sum(0)]) for t in range(n)])
    mass = torch.stack([torch.stack([o[t * rows:(t + 1) * rows].abs().sum(0), (o[t * rows:(t + 1) * rows]**2).sum(0)]) for t in range(n)])
    return want, mass


def stage_dgrad(dsrc, T, W, mask, z, act, n_out, addend=None, keep=None):
    W, d = W.to(F64), dsrc.to(F64)
    H = W.shape[0] // 2
    zr, omz = zw(z)
    lab = torch.as_tensor(np.asarray(mask)).bool().reshape(-1, 1)
    w1 = torch.where(lab, torch.tensor(zr, dtype=F64), torch.tensor(omz, dtype=F64))
    w0 = torch.where(lab, torch.tensor(omz, dtype=F64), torch.tensor(zr, dtype=F64))
    dZ = torch.cat([w1 * d, w0 * d], 1)
    if act != ACT_NONE:
        dZ = dZ * G.act_d(T.to(F64), act)
    assert W.shape[1] == n_out
    want, mass = dZ @ W, dZ.abs() @ W.abs()
    if addend is not None:
        want, mass = want + addend.to(F64), mass + addend.to(F64).abs()
    if keep is not None:
        want, mass = want * keep.to(F64), mass * keep.to(F64)
    return want, mass


def stage_gn_partials(g, x, saved, alpha, gn_act, keep, N, rows=128):
    """[n_tiles, 2, H] from the data gradient the kernel wrote (read back): graphnorm_oracle.stage_bwd_sums per tile"""
    ws, ms = [], []
    for t in range(_cdiv(N, rows)):
        s = slice(t * rows, min((t + 1) * rows, N))
        w, m = G.stage_bwd_sums(g[s], x[s], saved.float(), alpha, gn_act, None if keep is None else keep[s])
        ws.append(w), ms.append(m)
    return torch.stack(ws), torch.stack(ms)


# ---- fp32 restatements ------------------------------------------------------------------------------------------------------------
def _bf16_rne(x):
    u = np.asarray(x, dtype=f32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(f32)


def split3(x):
    """x = hi + mid + lo, each the RNE bf16 rounding of what the pieces before left (split2 of split_mma.h)"""
    x = np.asarray(x, dtype=f32)
    hi = _bf16_rne(x)
    r = (x - hi).astype(f32)
    mid = _bf16_rne(r)
    lo = _bf16_rne((r - mid).astype(f32))
    return hi, mid, lo


SPLIT_ORDER = ((1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0))


def restate_product(A, B, split, skip_step=None):
    """A [N, K] . B [C, K]^T in the kernel's order -> fp32 [N, C]; skip_step = (rows slice, ks): that K step left out for those rows
    (a mutant)"""
    A, B = np.asarray(A, dtype=f32), np.asarray(B, dtype=f32)
    N, K = A.shape
    acc = np.zeros((N, B.shape[0]), dtype=f32)
    pa = split3(A) if split else None
    pb = split3(B) if split else None
    for ks in range(K // KSTEP):
        s = slice(ks * KSTEP, (ks + 1) * KSTEP)
        new = acc.copy()
        if split:
            for ia, ib in SPLIT_ORDER:
                new = (new.astype(np.float64) + pa[ia][:, s].astype(np.float64) @ pb[ib][:, s].astype(np.float64).T).astype(f32)
        else:
            for k in range(s.start, s.stop):
                new = (new.astype(np.float64) + np.outer(A[:, k].astype(np.float64), B[:, k].astype(np.float64))).astype(f32)
        if skip_step is not None and skip_step[1] == ks:
            new[skip_step[0]] = acc[skip_step[0]]
        acc = new
    return acc


def _act32(h, act):
    h = np.asarray(h, dtype=f32)
    if act == ACT_NONE:
        return h
    with np.errstate(all="ignore"):
        e = G._expf_fast(h) if act == ACT_ELU else np.zeros_like(h)
        return np.where(h > 0, h, (e - f32(1) if act == ACT_ELU else np.where(np.isnan(h), h, f32(0)))).astype(f32)


def _actd32(h, act):
    h = np.asarray(h, dtype=f32)
    if act == ACT_NONE:
        return np.ones_like(h)
    with np.errstate(all="ignore"):
        return np.where(h > 0, f32(1), G._expf_fast(h) if act == ACT_ELU else f32(0)).astype(f32)


def restate_prologue(x, saved, gn_act, keep=None):
    """the operand staging's GraphNorm apply in fp32: fmaf, act_fast (ELU = hardware exponential - 1), the keep-scale"""
    x, saved = np.asarray(x, f32), np.asarray(saved, f32)
    o = _act32(G._fma32(x, saved[2], saved[3]), gn_act)
    return o if keep is None else (o * np.asarray(keep, f32)).astype(f32)


def restate_fwd(A, xb, W, b, mask, z, act, form, N=None, mutant=None):
    """tiled_fwd_kernel in fp32 -> dict T (or None on the effective-weight path), out [N, H], stats [n_partials, 2, H] (fp64 sums of
    the fp32 outputs).  A: the operand after the prologue (xa_out).  form: fwd_form(..., mask=mask).  mutant: a name of MUTANTS_FWD."""
    A, W, b = np.asarray(A, dtype=f32), np.asarray(W, dtype=f32), np.asarray(b, dtype=f32)
    X = A if xb is None else np.concatenate([A, np.asarray(xb, dtype=f32)], 1)
    N = X.shape[0] if N is None else N
    H, BM, split = W.shape[0] // 2, form["BM"], form["split"]
    zr, omz = f32(z), f32(1.0 - z)
    lab = np.asarray(mask).astype(bool)
    out = np.full((N, H), np.nan, dtype=f32)
    T = None if form["eff_live"] else np.full((N, 2 * H), np.nan, dtype=f32)
    W_unl = (omz * W[:H] + zr * W[H:]).astype(f32)
    b_unl = (omz * b[:H] + zr * b[H:]).astype(f32)
    for t, path in enumerate(form["paths"]):
        rows = slice(t * BM, min((t + 1) * BM, N))
        skip = (slice(0, 1), 1) if (mutant == "drop_kstep" and t == len(form["paths"]) - 1) else None
        if path == "pure":
            o = (restate_product(X[rows], W_unl, split, skip) + b_unl).astype(f32)
            for r in np.nonzero(lab[rows])[0]:
                if mutant == "fix_unlabeled":
                    continue
                s = f32(0)
                d = (W[:H] - W[H:]).astype(f32)
                prod = (X[rows][r][None, :] * d).astype(f32)
                s = np.zeros(H, dtype=f32)
                for k in range(prod.shape[1]):
                    s = (s + prod[:, k]).astype(f32)
                db = (b[:H] - b[H:]).astype(f32) if mutant != "fix_no_bias" else np.zeros(H, dtype=f32)
                c = ((zr - omz) * (s + db).astype(f32)).astype(f32)
                rr = r + 1 if (mutant == "fix_row_plus1" and r + 1 < o.shape[0]) else r
                o[rr] = (o[rr] + c).astype(f32)
            if mutant == "upper_ct_unwritten" and H > 256:
                o[:, 256:] = np.nan
            out[rows] = o
        else:
            Zt = (restate_product(X[rows], W, split, skip) + b).astype(f32)
            if T is not None:
                T[rows] = Zt
            a = _act32(Zt, act)
            l = lab[rows][:, None]
            if mutant == "swap_w":
                l = ~l
            w1, w0 = np.where(l, zr, omz).astype(f32), np.where(l, omz, zr).astype(f32)
            out[rows] = ((w1 * a[:, :H]).astype(f32).astype(np.float64) + (w0 * a[:, H:]).astype(f32).astype(np.float64)).astype(f32)
    return dict(T=T, out=out, stats=restate_partials(out, N, form["partial_rows"]))


def restate_partials(out, N, rows, extra_row=None, swap_halves=False):
    """the epilogue's fp64 sums of fp32 values per partial; extra_row: a row past N counted in the last partial, swap_halves: the two
    64-row partials of each 128-row tile exchanged (mutants)"""
    o = np.asarray(out, dtype=np.float64)[:N]
    n = _cdiv(N, rows)
    st = np.stack([np.stack([o[t * rows:(t + 1) * rows].sum(0), (o[t * rows:(t + 1) * rows]**2).sum(0)]) for t in range(n)])
    if extra_row is not None:
        e = np.asarray(extra_row, dtype=np.float64)
        st[-1, 0] += e
        st[-1, 1] += e * e
    if swap_halves:
        for t in range(0, n - 1, 2):
            st[[t, t + 1]] = st[[t + 1, t]]
    return st


def restate_dgrad(dsrc, T, W, mask, z, act, n_out, form, addend=None, keep=None, mutant=None):
    """tiled_dgrad_kernel in fp32 -> out [N, n_out]"""
    d, W = np.asarray(dsrc, dtype=f32), np.asarray(W, dtype=f32)
    N, H = d.shape
    split, BM = form["split"], form["BM"]
    zr, omz = f32(z), f32(1.0 - z)
    lab = np.asarray(mask).astype(bool)
    out = np.full((N, n_out), np.nan, dtype=f32)
    Wt = np.ascontiguousarray(W.T)                       # [n_out, 2H]: the operand image's logical form
    W_unl = (omz * Wt[:, :H] + zr * Wt[:, H:]).astype(f32)
    for t, path in enumerate(form["paths"]):
        rows = slice(t * BM, min((t + 1) * BM, N))
        skip = (slice(0, 1), 1) if (mutant == "drop_kstep" and t == len(form["paths"]) - 1) else None
        if path == "pure":
            o = restate_product(d[rows], W_unl, split, skip)
            for r in np.nonzero(lab[rows])[0]:
                if mutant == "fix_unlabeled":
                    continue
                prod = (d[rows][r][None, :] * (Wt[:, :H] - Wt[:, H:]).astype(f32)).astype(f32)
                s = np.zeros(n_out, dtype=f32)
                for k in range(H):
                    s = (s + prod[:, k]).astype(f32)
                rr = r + 1 if (mutant == "fix_row_plus1" and r + 1 < o.shape[0]) else r
                o[rr] = (o[rr] + ((zr - omz) * s).astype(f32)).astype(f32)
        else:
            l = lab[rows][:, None]
            if mutant == "swap_w":
                l = ~l
            w1, w0 = np.where(l, zr, omz).astype(f32), np.where(l, omz, zr).astype(f32)
            dZ = np.concatenate([(d[rows] * w1).astype(f32), (d[rows] * w0).astype(f32)], 1)
            if act != ACT_NONE:
                dZ = (dZ * _actd32(np.asarray(T, dtype=f32)[rows], act)).astype(f32)
            o = restate_product(dZ, Wt, split, skip)
        if addend is not None and mutant != "addend_dropped":
            o = (o + np.asarray(addend, dtype=f32)[rows]).astype(f32)
        if keep is not None:
            k = np.asarray(keep, dtype=f32)[rows]
            o = (o * k).astype(f32)
            if mutant == "dropout_twice":
                o = (o * k).astype(f32)
        out[rows] = o
    return out


def restate_gn_partials(g, x, saved, alpha, gn_act, keep, N, rows=128):
    """the data gradient's GraphNorm epilogue: gp and xhat in fp32, products and sums in fp64, per tile"""
    g, x, saved, alpha = np.asarray(g, f32)[:N], np.asarray(x, f32)[:N], np.asarray(saved, f32), np.asarray(alpha, f32)
    gp = g if keep is None else (g * np.asarray(keep, f32)[:N]).astype(f32)
    if gn_act != ACT_NONE:
        gp = (gp * _actd32(G._fma32(x, saved[2], saved[3]), gn_act)).astype(f32)
    xhat = ((x - (alpha * saved[0]).astype(f32)).astype(f32) * saved[1]).astype(f32)
    gp, xhat = gp.astype(np.float64), xhat.astype(np.float64)
    n = _cdiv(N, rows)
    return np.stack([np.stack([gp[t * rows:(t + 1) * rows].sum(0), (gp * xhat)[t * rows:(t + 1) * rows].sum(0)]) for t in range(n)])


MUTANTS_FWD = ("drop_kstep", "swap_w", "fix_no_bias", "fix_unlabeled", "fix_row_plus1", "upper_ct_unwritten")
MUTANTS_DGRAD = ("drop_kstep", "swap_w", "fix_unlabeled", "fix_row_plus1", "dropout_twice", "addend_dropped")
MUTANTS_PARTIALS = ("row_past_N", "halves_swapped")


def gate_nan_rows(got, want, mass, nan_rows):
    """the gate where whole rows of the truth are NaN (a non-finite input row): `got` is NaN in every element of exactly those rows
    — the split form turns Inf into NaN too —, the other rows are gated"""
    got, nan_rows = torch.as_tensor(got).to(F64), sorted(set(nan_rows))
    keep = torch.ones(got.shape[0], dtype=torch.bool)
    keep[nan_rows] = False
    if not bool(torch.isnan(got[~keep]).all()) or bool(torch.isnan(got[keep]).any()):
        return False, float("inf"), -1
    return gate(got[keep], torch.as_tensor(want).to(F64)[keep], torch.as_tensor(mass).to(F64)[keep])
