"""Host side of the whole-graph GraphNorm's tests (K6: glass_amd/csrc/graphnorm.hip, gn_kernels.h, gn_math.h, gn_acc.h) — torch
fp64 and Python integers on the CPU: the input recipes, the fp64 truth STAGE BY STAGE with the mass of every element, the exact
accumulators restated in integers, the launch dispatch restated (checked against the source text by
tests/test_graphnorm_host.py) and fp32 restatements of the kernels' summation orders.

Stages (every function -> (want, mass), fp64; each is a function of the kernel's OWN upstream outputs as read back, so that
only one stage's rounding is left to bound — the pattern of tests/readout_oracle.py, whose stage_saved / stage_gn_bwd / gate
are reused as they are):

  sums     from x                         S = sum x, Q = sum x^2 per column                         mass sum |x|, sum x^2
  saved    from x (readout_oracle.stage_saved)   mean, rstd, scale, shift
  y        from x, saved (read back), keep       keep * act(x * scale + shift)                      (|x scale| + |shift|) * keep
  S1, S2   from dy, x, saved, keep               sum g, sum g xhat; g = dy keep act'(h)             sum |g|, sum |g| (|x| + |a mu|) rstd
  coef, dgamma, dbeta, dalpha  from S1, S2 (read back: partial rows or decoded limbs)   readout_oracle.stage_gn_bwd
  dx       from dy, x, saved, coef (read back)   A g + Bx x + K (+ addend)                          sum of the absolute terms

(The Lipschitz bound of all three activations is 1 — ELU' = exp(h) <= 1 on h <= 0 — so the derivative bound the apply mass
is multiplied by is 1 and is left out.)  The pre-activation h: with `saved` in fp32 (the kernel's) h is restated as the
kernel forms it, ONE rounding of x * scale + shift to fp32 (fmaf); with `saved` in fp64 (the chain) it stays fp64.

Activation kinks.  ReLU' jumps at h = 0, and ELU' is formed from another branch there: an element whose fp64 h lies within
4 ulp(fp32) of 0 — measured at the magnitude of its addends, |h| <= 4 * 2^-23 * (|x scale| + |shift|), the only place where
the kernel's h and this file's can differ in sign — may fall either way.  `kinks` marks them; stage_dx gives them an infinite
mass (excluded), stage_bwd_sums adds their |dy keep| in full to the column's bar, the callers count them (cap: 0.1 % of a
case's elements; the host test checks that the recipes stay under it on the reference alone).

THE EXACT ACCUMULATORS (gn_acc.h), restated in Python integers.  A partial v is added as two 64-bit limbs, v * scale * 2^40 =
hi * 2^40 + lo with hi = floor(v * scale), lo in [0, 2^40) (truncated: up to 2^-40 / scale is lost per add: 2^-52 forward,
2^-64 backward); NaN, +-Inf or |v * scale| > 4.0e18 sets bit 63 of the lo limb instead (sticky: poison).
What the limbs guarantee, read from the code: the folded sum is the exact integer sum of the encoded partials WHILE the sum
over a replica's adds of |hi| — and the sum of these over the folded replicas — stays below 2^63, and fewer than 2^22 adds
went into a lo limb (their sum stays below 2^62 and never reaches the poison bit).  What they do NOT guarantee: a total beyond
that wraps modulo 2^64 into a finite value; it is NOT poisoned (only a single partial beyond 4.0e18 / scale is).  The documented
range |sum| < 2^50 (forward) / 2^38 (backward) lies inside the guarantee for that reason only: 2^50 * 2^12 = 2^38 * 2^24 =
2^62 < 2^63.  Beyond 2^53 / scale the conversion of hi to a double rounds (one more fp64 rounding, not a wrap).

Bound of the decoded forward sums (exact_sum_bound; derived, not chosen): a thread's fp64 walk, the row-slot fold and the
wave fold make a chain of k additions, each rounding by at most 2^-53 of the running sum of |addend| (<= sum |v|); every
add into the limbs truncates by less than 2^-52 (forward); the decode rounds twice more.  |got - exact| <= (k + 2) * 2^-53 *
sum |v| + adds * 2^-52, the exact sum taken on a per-column grid (column_sums_exact: its own error is returned and added).

Measured by tests/test_graphnorm_host.py (fp32 restatement, worst share of the 1e-5 * mass bar over all recipes): see its
printout; on MI355X: the table in tests/test_gpu_graphnorm.py."""
import math
import os
import re

import numpy as np
import torch

from readout_oracle import TOL, gate, rel_inf, source_constants, stage_gn_bwd, stage_saved  # noqa: F401  (re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
ACT_NONE, ACT_ELU, ACT_RELU = 0, 1, 2
BLOCK, UNROLL, MAX_STAT_BLOCKS, APPLY_CAP = 256, 4, 1024, 4096   # common.h kBlock; gn_kernels.h kUnroll, kMaxStatBlocks, apply_blocks
FIN_COLS, FIN_SLOTS, FIN_FLY, MAX_SRC = 4, 64, 8, 8               # gn_math.h kFinCols, kFinSlots, kFinFly; graphnorm.hip kMaxStatSrc
ACC_REP, SCALE_FWD, SCALE_BWD = 16, 4096.0, 16777216.0            # gn_acc.h kAccRep, kAccScaleFwd, kAccScaleBwd
ACC_BOUND, POISON, LO_BITS = 4.0e18, 1 << 63, 40                  # gn_acc_add's range test, kAccPoison, the lo limb's width
STATS64_ROWS, STATS64_ROUND, STATS64_WGS = 16, 5, 256             # gn_stats64_exact_kernel: rows per step, kRound; the host's 256 workgroups
ACC64_UN = 5                                                      # gn_bwd_apply_acc_kernel<4, 64, 5>
KINK_ULPS, KINK_CAP = 4, 1e-3


def gn_source_constants():
    """the constants the restatement depends on, read from the source text of the four K6 files"""
    rd = lambda n: open(os.path.join(ROOT, "glass_amd", "csrc", n)).read()
    kern, mth, acc, hip = rd("gn_kernels.h"), rd("gn_math.h"), rd("gn_acc.h"), rd("graphnorm.hip")
    num = lambda pat, text: int(re.search(pat, text).group(1))
    flt = lambda pat, text: float(re.search(pat, text).group(1))
    flat = hip.replace("\n", " ")
    k = source_constants()
    return {"kBlock": k["kBlock"], "kUnroll": num(r"constexpr int kUnroll = (\d+);", kern),
            "kMaxStatBlocks": num(r"constexpr int kMaxStatBlocks = (\d+);", kern),
            "apply_cap": num(r"static unsigned apply_blocks\(.*?if \(b > (\d+)\) b = \1;", kern.replace("\n", " ")),
            "stat_div_text": "ceil_div(n_rows, (int64_t)t.rpb * kUnroll * 2)" in kern,
            "apply_div_text": "ceil_div(n_rows, (int64_t)t.rpb * kUnroll)" in kern,
            "tiling_text": all(s in kern for s in ("t.vw = vec_ok ? 4 : 1;", "t.cw = (int)ceil_div(C, t.vw);", "t.tc = pow2_ceil_cap(t.cw, kBlock);",
                                                   "t.rpb = kBlock / t.tc;", "t.ctiles = (int)ceil_div(t.cw, t.tc);")),
            "kFinCols": num(r"constexpr int kFinCols = (\d+),", mth), "kFinFly": num(r"kFinFly = (\d+);", mth),
            "fin_slots_text": "kFinSlots = kBlock / kFinCols" in mth, "fin_walk_text": "b += kFinSlots * kFinFly" in mth,
            "fin_fold_text": "for (int r = tr; r < kFinSlots; r += 8)" in mth,
            "kAccRep": num(r"#define GLASS_ACC_REP (\d+)", acc), "kAccScaleFwd": flt(r"constexpr double kAccScaleFwd = ([\d.]+);", acc),
            "kAccScaleBwd": flt(r"constexpr double kAccScaleBwd = ([\d.]+);", acc),
            "acc_bound": flt(r"if \(!\(fabs\(sv\) <= ([\d.e]+)\)\)", acc), "poison_bit": num(r"constexpr unsigned long long kAccPoison = 1ull << (\d+);", acc),
            "lo_scale": flt(r"\(sv - fl\) \* ([\d.]+)\);", acc), "lo_inv_text": "(double)lo * (1.0 / 1099511627776.0)" in acc,
            "index_text": "return (((size_t)rep * 2 + which) * C + c) * 2;" in acc,
            "kMaxStatSrc": num(r"constexpr int kMaxStatSrc = (\d+);", hip),
            "vec_fwd_text": flat.count("const bool vec = C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && aligned16(x) && aligned16(y);") == 2,
            "vec_in_text": flat.count("const bool vec = C % 4 == 0 && ldx % 4 == 0 && aligned16(x);") == 2,
            "vec_bwd_text": len(re.findall(r"const bool vec4? = C % 4 == 0 && lddy % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0 && aligned16\(dy\) && aligned16\(x\) &&\s+"
                                           r"aligned16\(dx\) && \(!addend \|\| \(ldadd % 4 == 0 && aligned16\(addend\)\)\);", hip)) == 3,
            "stats64_text": "if (vec && C == 64) {" in hip and "int nst = (int)ceil_div(ceil_div(n_rows, (int64_t)256), (int64_t)16);" in hip
                            and "if (nst < 5) nst = n_rows >= 80 * 64 ? 5 : (nst < 1 ? 1 : nst);" in hip
                            and "ceil_div(n_rows, (int64_t)16 * nst)" in hip and "constexpr int C = 64, kRound = 5;" in hip,
            "bwd_exact_text": "(C == 16 || C == 32 || C == 64 || C == 128) && aligned16(partial)" in hip
                              and "n_rep <= kAccRep && (n_rep == 1 || n_rep % 2 == 0)" in hip and "if (C == 64 && n_rep >= 2)" in hip
                              and "gn_bwd_apply_acc_kernel<4, 64, 5>), dim3((unsigned)ceil_div(n_rows, (int64_t)t4.rpb * 5))" in hip
                              and "gn_bwd_apply_acc_kernel<4, 0>), dim3(apply_blocks(n_rows, t4))" in hip}


# ---- dispatch restated --------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _pow2_ceil_cap(v, cap):
    p = 1
    while p < v and p < cap:
        p *= 2
    return p


def tiling(C, vec):
    """make_tiling -> (vw, cw, tc, rpb, ctiles)"""
    vw = 4 if vec else 1
    cw = _cdiv(C, vw)
    tc = _pow2_ceil_cap(cw, BLOCK)
    return vw, cw, tc, BLOCK // tc, _cdiv(cw, tc)


def stat_blocks(N, C, vec):
    return min(max(_cdiv(N, tiling(C, vec)[3] * UNROLL * 2), 1), MAX_STAT_BLOCKS)


def apply_blocks(N, C, vec):
    return min(max(_cdiv(N, tiling(C, vec)[3] * UNROLL), 1), APPLY_CAP)


def _al(*ptrs):
    return all(p % 16 == 0 for p in ptrs)


def vec_fwd(C, ldx, ldy, x_ptr=0, y_ptr=0):
    """glass_graphnorm_fwd_f32, glass_graphnorm_apply_f32"""
    return C % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and _al(x_ptr, y_ptr)


def vec_in(C, ldx, x_ptr=0):
    """glass_graphnorm_stats_f32, glass_graphnorm_stats_exact_f32: input-only entries"""
    return C % 4 == 0 and ldx % 4 == 0 and _al(x_ptr)


def vec_bwd(C, lddy, ldx, lddx, ldadd=None, dy_ptr=0, x_ptr=0, dx_ptr=0, add_ptr=0):
    """glass_graphnorm_bwd_f32, glass_graphnorm_bwd_from_stats_f32 (ldadd None: no addend)"""
    return C % 4 == 0 and lddy % 4 == 0 and ldx % 4 == 0 and lddx % 4 == 0 and _al(dy_ptr, x_ptr, dx_ptr) and \
        (ldadd is None or (ldadd % 4 == 0 and _al(add_ptr)))


def exact_stats_form(N, C, vec):
    """glass_graphnorm_stats_exact_f32 -> ("stats64", nst, grid) | ("generic", vw, (grid.x, grid.y))"""
    if vec and C == 64:
        nst = _cdiv(_cdiv(N, STATS64_WGS), STATS64_ROWS)
        if nst < STATS64_ROUND:
            nst = STATS64_ROUND if N >= 80 * 64 else max(nst, 1)
        return "stats64", nst, _cdiv(N, STATS64_ROWS * nst)
    return "generic", tiling(C, vec)[0], (stat_blocks(N, C, vec), tiling(C, vec)[4])


def bwd_exact_form(C, n_rep, N, vec4=True, acc_aligned=True):
    """glass_graphnorm_bwd_from_stats_f32 with nblk = -n_rep -> ("acc64x5", grid) | ("acc_lds", grid) | ("refused", why)"""
    if not (vec4 and C in (16, 32, 64, 128) and acc_aligned):
        return "refused", "width or alignment"
    if not (1 <= n_rep <= ACC_REP and (n_rep == 1 or n_rep % 2 == 0)):
        return "refused", "replicas"
    if C == 64 and n_rep >= 2:
        return "acc64x5", _cdiv(N, tiling(C, True)[3] * ACC64_UN)
    return "acc_lds", apply_blocks(N, C, True)


def fin_order_sum(part):
    """gn_sum_partials' order in fp64: part [nblk, ...] numpy float64 -> the sum over axis 0 as slot tr adds b = tr + 64 u + 512 j
    in turn, lane tr < 8 adds the slots tr, tr + 8, .., and slot 0 the eight results"""
    part = np.asarray(part, dtype=np.float64)
    nblk = part.shape[0]
    slot = np.zeros((FIN_SLOTS, ) + part.shape[1:])
    for tr in range(min(FIN_SLOTS, nblk)):
        for b in range(tr, nblk, FIN_SLOTS * FIN_FLY):
            for u in range(FIN_FLY):
                if b + FIN_SLOTS * u < nblk:
                    slot[tr] = slot[tr] + part[b + FIN_SLOTS * u]
    eight = np.zeros((8, ) + part.shape[1:])
    for tr in range(8):
        for r in range(tr, FIN_SLOTS, 8):
            eight[tr] = eight[tr] + slot[r]
    out = np.zeros(part.shape[1:])
    for r in range(8):
        out = out + eight[r]
    return out


def fin_slots_read(nblk):
    """partial rows gn_sum_partials reads: exactly 0 .. nblk - 1 (each once)"""
    seen = []
    for tr in range(FIN_SLOTS):
        for b in range(tr, nblk, FIN_SLOTS * FIN_FLY):
            seen += [b + FIN_SLOTS * u for u in range(FIN_FLY) if b + FIN_SLOTS * u < nblk]
    return sorted(seen)


# ---- the accumulators in integers ------------------------------------------------------------------------------------------------------
def _wrap(v):
    """a Python integer as the int64 two's-complement word holding it"""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def acc_layout(rep, which, c, C):
    """gn_acc_index: the word index of the hi limb (lo follows)"""
    return ((rep * 2 + which) * C + c) * 2


def acc_words(C):
    return ACC_REP * 2 * C * 2


def acc_encode(v, scale):
    """gn_acc_add on one partial -> (hi, lo) integers, or None: poison"""
    sv = float(v) * scale
    if not (abs(sv) <= ACC_BOUND):
        return None
    fl = math.floor(sv)
    return int(fl), int((sv - fl) * float(1 << LO_BITS))


def acc_add(words, rep, which, c, C, v, scale):
    """one gn_acc_add into `words` (a list of Python integers holding int64 words, wrapping like the atomics do)"""
    i = acc_layout(rep, which, c, C)
    e = acc_encode(v, scale)
    if e is None:
        words[i + 1] = _wrap(words[i + 1] | POISON)
    else:
        words[i], words[i + 1] = _wrap(words[i] + e[0]), _wrap(words[i + 1] + e[1])


def acc_encode_tensor(v, scale):
    """acc_encode on a fp64 tensor -> (hi, lo) int64 tensors and the poison mask (hi = lo = 0 there)"""
    sv = v.to(F64) * scale
    bad = ~(sv.abs() <= ACC_BOUND)
    sv = torch.where(bad, torch.zeros_like(sv), sv)
    fl = sv.floor()
    return fl.to(torch.int64), ((sv - fl) * float(1 << LO_BITS)).to(torch.int64), bad


def acc_decode(words, C, n_rep, scale):
    """gn_acc_fold over the first n_rep replicas -> dict: total [2][C] Python integers hi * 2^40 + lo of the WRAPPED limb sums
    (units of 2^-40 / scale), bad [2][C], value [2, C] fp64 as gn_acc_value forms it (NaN where poisoned)"""
    w = [int(t) for t in (words.tolist() if hasattr(words, "tolist") else words)]
    total, bad, value = [[0] * C for _ in range(2)], [[False] * C for _ in range(2)], torch.zeros(2, C, dtype=F64)
    for which in range(2):
        for c in range(C):
            hi = lo = 0
            for r in range(n_rep):
                i = acc_layout(r, which, c, C)
                hi, lo = _wrap(hi + w[i]), _wrap(lo + w[i + 1])
                bad[which][c] |= w[i + 1] < 0
            total[which][c] = (hi << LO_BITS) + lo
            value[which, c] = float("nan") if bad[which][c] else (float(hi) + float(lo) * (1.0 / float(1 << LO_BITS))) * (1.0 / scale)
    return dict(total=total, bad=bad, value=value)


def column_sums_exact(v):
    """sum over axis 0 of a fp64 [N, C] tensor -> (sum, bound of its own error): every value is cut on a per-column grid so
    coarse that the grid parts add exactly in fp64 (N * max / grid < 2^52); the remainders (|.| <= grid / 2, themselves exact)
    add with the usual N * 2^-53 * sum |remainder|."""
    v = v.to(F64)
    N = v.shape[0]
    mx = v.abs().max(0).values.clamp(min=2.0**-900)
    grid = torch.exp2(torch.ceil(torch.log2(mx * N)) - 51)
    vh = torch.round(v / grid) * grid
    vl = v - vh
    assert bool(((vh.abs().sum(0) / grid) < 2.0**53).all())
    return vh.sum(0) + vl.sum(0), N * 2.0**-53 * vl.abs().sum(0) + 2.0**-53 * v.abs().sum(0)


def exact_sum_bound(x, C, form, adds, scale=SCALE_FWD):
    """the bound of the module docstring on the decoded (sum x, sum x^2) -> (want [2, C], bound [2, C]); adds = workgroups that
    added into a column's limbs.  k = additions between an element and its workgroup's partial: the thread's walk + the row-slot
    fold (generic) / the walk, two lane shuffles and the wave fold (stats64)"""
    x = x.to(F64)
    N = x.shape[0]
    if form[0] == "stats64":
        k = form[1] + 4
    else:
        rpb = tiling(C, form[1] == 4)[3]
        k = _cdiv(N, form[2][0] * rpb) + rpb
    S, eS = column_sums_exact(x)
    Q, eQ = column_sums_exact(x * x)
    m = torch.stack([x.abs().sum(0), (x * x).sum(0)])
    return torch.stack([S, Q]), (k + 2) * 2.0**-53 * m + adds * 2.0**-LO_BITS / scale + torch.stack([eS, eQ])


def saved_from_sums(S, Q, N, gamma, beta, alpha, eps):
    """gn_math.h gn_fwd_coeffs in fp64 from given column sums -> saved [4, C] (what a consumer of decoded accumulators forms)"""
    a, N = alpha.to(F64), float(N)
    mu = S.to(F64) / N
    var = (Q.to(F64) / N - mu * mu * (2.0 * a - a * a)).clamp(min=0)
    rstd = 1.0 / torch.sqrt(var + float(np.float32(eps)))
    scale = gamma.to(F64) * rstd
    return torch.stack([mu, rstd, scale, beta.to(F64) - scale * a * mu])


# ---- stages --------------------------------------------------------------------------------------------------------------------------
def act_f(h, act):
    if act == ACT_ELU:
        return torch.where(h > 0, h, torch.expm1(h))
    return torch.relu(h) if act == ACT_RELU else h     # torch.relu keeps NaN


def act_d(h, act):
    if act == ACT_ELU:
        return torch.where(h > 0, torch.ones_like(h), torch.exp(h))
    return (h > 0).to(h.dtype) if act == ACT_RELU else torch.ones_like(h)


def pre_act(x, saved):
    """h and the magnitude of its addends; saved fp32: rounded once to fp32 like the kernel's fmaf, saved fp64: left in fp64"""
    h = x.to(F64) * saved[2].to(F64) + saved[3].to(F64)
    mag = (x.to(F64) * saved[2].to(F64)).abs() + saved[3].to(F64).abs()
    return (h.float().to(F64) if saved.dtype == torch.float32 else h), mag


def kinks(x, saved, act):
    """elements whose derivative may fall either way (module docstring)"""
    if act == ACT_NONE:
        return torch.zeros(x.shape, dtype=torch.bool)
    h, mag = pre_act(x, saved)
    return h.abs() <= KINK_ULPS * 2.0**-23 * mag


def _keep(keep, like):
    return torch.ones_like(like, dtype=F64) if keep is None else keep.to(F64)


def stage_sums(x):
    x = x.to(F64)
    return torch.stack([x.sum(0), (x * x).sum(0)]), torch.stack([x.abs().sum(0), (x * x).sum(0)])


def stage_apply(x, saved, act, keep=None):
    h, mag = pre_act(x, saved)
    k = _keep(keep, h)
    return k * act_f(h, act), mag * k


def _g(dy, x, saved, act, keep):
    h, _ = pre_act(x, saved)
    return dy.to(F64) * _keep(keep, h) * act_d(h, act)


def stage_bwd_sums(dy, x, saved, alpha, act, keep=None):
    """[2, C]: S1 = sum g, S2 = sum g xhat; a kink element's |dy keep| is allowed in full (as |.| / TOL of mass)"""
    g = _g(dy, x, saved, act, keep)
    x, mu, rstd, a = x.to(F64), saved[0].to(F64), saved[1].to(F64), alpha.to(F64)
    xh, xh_m = (x - a * mu) * rstd, (x.abs() + (a * mu).abs()) * rstd.abs()
    slack = torch.where(kinks(x, saved, act), (dy.to(F64) * _keep(keep, g)).abs() / TOL, torch.zeros_like(g))
    return torch.stack([g.sum(0), (g * xh).sum(0)]), torch.stack([(g.abs() + slack).sum(0), ((g.abs() + slack) * xh_m).sum(0)])


def stage_dx(dy, x, saved, coef, addend, act, keep=None, coef_m=None):
    """A g + Bx x + K (+ addend); coef [3, C] as read back (or fp64 with its mass coef_m); kink elements get an infinite mass"""
    g = _g(dy, x, saved, act, keep)
    x, coef = x.to(F64), coef.to(F64)
    coef_m = coef.abs() if coef_m is None else coef_m.to(F64)
    want, mass = coef[0] * g + coef[1] * x + coef[2], coef_m[0] * g.abs() + coef_m[1] * x.abs() + coef_m[2]
    if addend is not None:
        want, mass = want + addend.to(F64), mass + addend.to(F64).abs()
    return want, torch.where(kinks(x, saved, act), torch.full_like(mass, float("inf")), mass)


def gate_with_nan(got, want, mass, tol=TOL):
    """the gate where the truth itself holds NaN (non-finite input): NaN exactly where the truth's is, the rest gated"""
    got, want, mass = got.to(F64).reshape(-1), want.to(F64).reshape(-1), mass.to(F64).reshape(-1)
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(got), nan):
        return False, float("inf"), int((torch.isnan(got) != nan).nonzero()[0])
    return gate(got[~nan], want[~nan], mass[~nan], tol)


def sums_as_partial(S, M=None):
    """[2, C] column sums as the one-row partial buffer stage_gn_bwd takes"""
    return S.to(F64).unsqueeze(0), (S.to(F64).abs() if M is None else M.to(F64)).unsqueeze(0)


# ---- the chain and its autograd statement ----------------------------------------------------------------------------------------------
def chain(ins, act, keep=None, addend=None, prev=None):
    """the stages on their own fp64 outputs: saved, y, sums [2, C], coef, dgamma, dbeta, dalpha, dx (prev: previous contents of
    the three parameter gradients under accumulate = 1)"""
    x, N = ins["x"], ins["x"].shape[0]
    saved, _ = stage_saved(x, ins["gamma"], ins["beta"], ins["alpha"], ins["eps"])
    y, _ = stage_apply(x, saved, act, keep)
    S, M = stage_bwd_sums(ins["dy"], x, saved, ins["alpha"], act, keep)
    Gn = stage_gn_bwd(*sums_as_partial(S, M), N, ins["gamma"], ins["alpha"], saved, prev)
    dx, _ = stage_dx(ins["dy"], x, saved, Gn["coef"][0], addend, act, keep)
    return dict(saved=saved, y=y, sums=S, coef=Gn["coef"][0], dgamma=Gn["dgamma"][0], dbeta=Gn["dbeta"][0], dalpha=Gn["dalpha"][0], dx=dx,
                kinks=kinks(x, saved, act))


def autograd_graphnorm(ins, act, keep=None):
    """oracle.glass_oracle.GraphNorm in fp64 under autograd, then the activation and the given keep-scales; the loss is
    sum(y * dy) -> y, dx, dgamma, dbeta, dalpha"""
    import sys
    sys.path.insert(0, ROOT)
    from oracle.glass_oracle import GraphNorm
    C = ins["x"].shape[1]
    gn = GraphNorm(C, eps=ins["eps"]).double()
    with torch.no_grad():
        gn.weight.copy_(ins["gamma"].double())
        gn.bias.copy_(ins["beta"].double())
        gn.mean_scale.copy_(ins["alpha"].double())
    x = ins["x"].double().clone().requires_grad_(True)
    h = gn(x)
    y = {ACT_NONE: lambda t: t, ACT_ELU: torch.nn.functional.elu, ACT_RELU: torch.relu}[act](h)
    if keep is not None:
        y = y * keep.double()
    (y * ins["dy"].double()).sum().backward()
    return dict(y=y.detach(), dx=x.grad, dgamma=gn.weight.grad, dbeta=gn.bias.grad, dalpha=gn.mean_scale.grad)


# ---- recipes -----------------------------------------------------------------------------------------------------------------------------
KINDS = ("plain", "mixed", "flat", "tiny_grad")
ALPHAS = (0.0, 0.5, 1.0, 1.5, 2.0, 2.5, -0.5)   # 2a - a^2 = 0, .75, 1, .75, 0, -1.25, -1.25


def recipe(N, C, seed, kind="plain"):
    """Deterministic inputs x, dy, addend [N, C] and gamma, beta, alpha [C] (fp32), eps.
    plain: x of mean 5, std 2 (the cancelling variance), gamma of both signs, alpha in [0.5, 1.5);
    mixed: column scales 1e-3 .. 1e3, column means of either sign, alpha cycling through ALPHAS, gamma of both signs;
    flat: plain with every third column constant (var = 0 where alpha = 1: eps rules), alpha = 1 on every sixth;
    tiny_grad: plain with dy around 1e-12 (the reason kAccScaleBwd exists)."""
    assert kind in KINDS
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, generator=g) * 2.0 + 5.0
    dy = torch.randn(N, C, generator=g)
    addend = torch.randn(N, C, generator=g)
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    gamma[0] = 0.7
    if C > 1:
        gamma[1] = -0.9
    beta, alpha = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    if kind == "mixed":
        sc = torch.logspace(-3, 3, C)[torch.randperm(C, generator=g)] if C > 1 else torch.ones(1)
        x = (torch.randn(N, C, generator=g) + 2.0 * torch.randn(C, generator=g)) * sc
        alpha = torch.tensor([ALPHAS[c % len(ALPHAS)] for c in range(C)])
    if kind == "flat":
        cols = torch.arange(0, C, 3)
        # (constants of small magnitude: y = x * scale + shift cancels at |x gamma| / sqrt(eps) there, 316 |x gamma|, and fp32
        # leaves 2^-24 of THAT in y — the stage gate's mass says so, the end-to-end rel-inf of 1e-5 holds only below |x| ~ 1)
        x[:, cols] = (0.03125 * (1 + cols % 7).float()).reshape(1, -1)
        alpha[torch.arange(0, C, 6)] = 1.0
    if kind == "tiny_grad":
        dy, addend = dy * 1e-12, addend * 1e-12
    return dict(x=x, dy=dy, addend=addend, gamma=gamma, beta=beta, alpha=alpha, eps=1e-5, N=N, C=C, kind=kind)


def keep_mask(N, C, p, seed):
    """a stand-in for the kernel's keep-scales on the host: 0 or fl32(1 / (1 - p))"""
    g = torch.Generator().manual_seed(seed)
    return torch.where(torch.rand(N, C, generator=g) >= p, torch.tensor(np.float32(1) / (np.float32(1) - np.float32(p))), torch.tensor(0.0))


# ---- fp32 restatements in the kernels' order (numpy) ---------------------------------------------------------------------------------------
f32 = np.float32


def _fma32(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def _expf_fast(h):
    """__expf: the hardware exp2 of fl32(h * log2 e)"""
    return np.exp2((h.astype(f32) * f32(1.4426950408889634)).astype(f32)).astype(f32)


def _rows_of(N, grid, rpb):
    """rows[blk][tr]: the rows thread slot tr of workgroup blk adds, in its order (trip by trip, u = 0 .. 3)"""
    stride = grid * rpb
    return [[np.arange(b * rpb + tr, N, stride) for tr in range(rpb)] for b in range(grid)]


def _walk_fold(terms, N, grid, rpb):
    """terms [N, K] fp64 -> partial [grid, K]: each slot adds its rows in turn from 0.0, slot 0 then adds the slots 1 .. rpb - 1"""
    out = np.zeros((grid, terms.shape[1]))
    for b, slots in enumerate(_rows_of(N, grid, rpb)):
        tot = None
        for rows in slots:
            s = np.zeros(terms.shape[1])
            for r in rows:
                s = s + terms[r]
            tot = s if tot is None else tot + s
        out[b] = tot
    return out


def restate_stats(x, vec=True):
    """gn_stats_kernel -> partial [nblk, 2, C] fp64"""
    x = np.asarray(x, dtype=np.float64)
    N, C = x.shape
    grid, rpb = stat_blocks(N, C, vec), tiling(C, vec)[3]
    p = _walk_fold(np.concatenate([x, x * x], 1), N, grid, rpb)
    return p.reshape(grid, 2, C)


def restate_stats64(x, n_rep):
    """gn_stats64_exact_kernel -> the accumulator words (a list of Python integers)"""
    x = np.asarray(x, dtype=np.float64)
    N, C = x.shape
    assert C == 64
    _, nst, grid = exact_stats_form(N, C, True)
    words = [0] * acc_words(C)
    t = np.concatenate([x, x * x], 1)
    for b in range(grid):
        s = np.zeros((16, 2 * C))
        for rs in range(16):
            for st in range(nst):
                r = b * 16 * nst + 16 * st + rs
                if r < N:
                    s[rs] = s[rs] + t[r]
        w = [(s[4 * k] + s[4 * k + 1]) + (s[4 * k + 2] + s[4 * k + 3]) for k in range(4)]
        tot = (w[0] + w[1]) + (w[2] + w[3])
        for i in range(2 * C):
            acc_add(words, b % n_rep, i // C, i % C, C, tot[i], SCALE_FWD)
    return words


def restate_apply(x, saved, act, keep=None):
    x, saved = np.asarray(x, f32), np.asarray(saved, f32)
    h = _fma32(x, saved[2], saved[3])
    with np.errstate(all="ignore"):
        if act == ACT_ELU:
            h = np.where(h > 0, h, np.expm1(h).astype(f32))
        elif act == ACT_RELU:
            h = np.where(h > 0, h, np.where(np.isnan(h), h, f32(0)))
    return h if keep is None else (h * np.asarray(keep, f32)).astype(f32)


def _g32(dy, x, saved, act, keep):
    g = np.asarray(dy, f32)
    if keep is not None:
        g = (g * np.asarray(keep, f32)).astype(f32)
    if act != ACT_NONE:
        h = _fma32(x, saved[2], saved[3])
        d = np.where(h > 0, f32(1), _expf_fast(h) if act == ACT_ELU else f32(0)).astype(f32)
        g = (g * d).astype(f32)
    return g


def restate_bwd_stats(dy, x, saved, alpha, act, keep=None, vec=True):
    """gn_bwd_stats_kernel -> partial [nblk, 2, C] fp64 (xhat in fp32 with the contracted a * mu, the products in fp64)"""
    x, saved, alpha = np.asarray(x, f32), np.asarray(saved, f32), np.asarray(alpha, f32)
    N, C = x.shape
    g = _g32(dy, x, saved, act, keep).astype(np.float64)
    xhat = (_fma32(-alpha, saved[0], x) * saved[1]).astype(f32).astype(np.float64)
    grid, rpb = stat_blocks(N, C, vec), tiling(C, vec)[3]
    return _walk_fold(np.concatenate([g, g * xhat], 1), N, grid, rpb).reshape(grid, 2, C)


def restate_dx(dy, x, saved, coef, addend, act, keep=None):
    x, saved, coef = np.asarray(x, f32), np.asarray(saved, f32), np.asarray(coef, f32)
    out = _fma32(coef[0], _g32(dy, x, saved, act, keep), _fma32(coef[1], x, coef[2]))
    return out if addend is None else (out + np.asarray(addend, f32)).astype(f32)
