"""Host side of the fused training readout's tests (glass_amd/csrc/readout.hip, glass_readout_train_f32: sum / mean / size
pooling) — torch fp64 on the CPU: the input recipes, the launch dispatch restated (checked against the source text by
tests/test_readout_host.py), the workspace layout restated, and the fp64 truth STAGE BY STAGE with the mass of every element.

Why stage by stage: the readout is a chain (GraphNorm apply -> pool -> head -> loss -> head backward -> GraphNorm backward
sums -> coefficients -> d jk).  A whole-tensor rel-inf against an end-to-end oracle lets the error of one stage hide under the
scale of another.  Here every output is graded against an fp64 function of the kernel's OWN upstream outputs as read back
(the intermediates are in the workspace), so only one stage's rounding is left to bound:

  saved      (gn_src only) mean, rstd, scale, shift from fp64 column sums of jk
  pooled     from jk, saved, pos          sum over the row's valid entries of scale * x + shift, times the pool scale
  logits     from pooled (read back)      sum_c pooled * Wh + bh
  loss_rows, dlogits, loss                from logits (read back); CE denominators B, BCE B * K; the grad_loss seed
  dys        from dlogits (read back)     pool scale * sum_k dl * Wh
  dWh, dbh   from dlogits, pooled (read back), plus the previous contents under acc_head
  partial    (forms with a reduce launch) from dys (read back): cnt * dy and dy * sum xhat
  coef, dgamma, dbeta, dalpha             from the column sums S1, S2 of dys (read back): gn_math.h gn_bwd_coeffs restated
  djk        Bx * x + K + A * sum of dys over the entries naming the row; the coefficients in fp64 from dys as read back
             (the two-launch form keeps them in LDS), the mass expanding Bx and K down to the addends of S1 and S2

The gate, element by element: |got - want| <= 1e-5 * mass, mass = sum of |addend| of the fp64 expression of that element; an
element of mass 0 must be exactly 0 (the pooled row of an all-padding subgraph); a NaN is an infinite error.  `chain` runs the
same stages on their own fp64 outputs: the end-to-end statement, pinned to torch autograd by the host test, against which every
case is also held at rel-inf <= 1e-5 — stage-wise grading alone could not see a stage that is wrong consistently.

Measured by tests/test_readout_host.py (fp32 restatement of the kernels' summation orders, worst share of the bar, N 97,
C 64, B 9, Smax 40, K 3, grad_loss -2.5): every stage <= 0.02; on MI355X: the table in
tests/test_gpu_readout.py."""
import os
import re

import torch

TOL = 1e-5
MODES = {"sum": 0, "mean": 1, "size": 3}
BLOCK, WAVE, ORD_BLOCK = 256, 64, 1024     # common.h kBlock, kWave; readout.hip kOrdBlock
ORDERED_MAX = 16384                         # kReadoutOrderedMax
MAX_K = 256                                 # kReadoutMaxK
MAX_C = 4 * BLOCK                           # glass_readout_supported
DENSE_CAP, BACKFILL_CAP = 4096, 2048        # grid caps of readout_dense_kernel / readout_backfill_kernel's dense role
LONG_LIST = 64                              # readout_gather_add_kernel kLong
LDS_HEAD, RED_STRIDE = 10, 8                # readout_lds_head(false), readout_red_stride(false)
LDS_LIMIT = 64 * 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def source_constants():
    """the constants the restatement depends on, read from the source text"""
    src = open(os.path.join(ROOT, "glass_amd", "csrc", "readout.hip")).read()
    common = open(os.path.join(ROOT, "glass_amd", "csrc", "common.h")).read()
    num = lambda pat, text: int(re.search(pat, text).group(1))
    host = re.search(r"static int readout_train\(.*?\n}", src, re.S).group(0)
    return {"kBlock": num(r"constexpr int kBlock = (\d+);", common), "kWave": num(r"constexpr int kWave = (\d+);", common),
            "kOrdBlock": num(r"constexpr int kOrdBlock = (\d+);", src),
            "kReadoutOrderedMax": num(r"constexpr int64_t kReadoutOrderedMax = (\d+);", src),
            "kReadoutMaxK": num(r"constexpr int kReadoutMaxK = (\d+);", src),
            "kLong": num(r"constexpr int kLong = (\d+);", src),
            "max_c_in_blocks": num(r"glass_readout_supported\(.*?C <= (\d+) \* kBlock", src.replace("\n", " ")),
            "backfill_cap": num(r"if \(n_dense > (\d+)\) n_dense = \1;", host),
            "dense_cap": num(r"if \(blocks > (\d+)\) blocks = \1;", host),
            "lds_head": num(r"readout_lds_head\(bool mx\) \{ return mx \? \d+ : (\d+); \}", src),
            "red_stride": num(r"readout_red_stride\(bool mx\) \{ return mx \? \d+ : (\d+); \}", src),
            "lds1_text": "sizeof(float) * (size_t)(readout_lds_head(MAX) * C + kBlock * readout_red_stride(MAX) + 2 * kReadoutMaxK)" in host,
            "stash_text": "Smax > 2 * (kBlock >> tc_log2) && n_nodes < (1ll << 31) && lds1_base + sizeof(float) * (size_t)Smax <= 64 * 1024" in host,
            "lds3_attr_text": "if (lds3 > 64 * 1024)" in host,
            "tc_text": "pow2_ceil_cap(vec ? C / 4 : C, kBlock)" in host,
            "early_text": "const bool early = 2 * C <= kBlock;" in src,
            "short_text": "if (a.Smax <= 2 * rpb)" in src}


def _pow2_ceil_cap(v, cap):
    p = 1
    while p < v and p < cap:
        p *= 2
    return p


def _cdiv(a, b):
    return -(-a // b)


def dispatch(C, B, Smax, N, aligned=True, labels=False, bwd_acc=False, longest_list=0):
    """readout_train<false>'s choices restated.  aligned: ldj, lddj multiples of 4 and jk, djk, pooled on 16 bytes; labels:
    the label bytes, rows and count are given; bwd_acc: gn_bwd_acc given; longest_list: entries of the most-named node (only
    read for the gather-add tail)."""
    vec = C % 4 == 0 and aligned
    tc = _pow2_ceil_cap(C // 4 if vec else C, BLOCK)
    rpb = BLOCK // tc
    lds1_base = 4 * (LDS_HEAD * C + BLOCK * RED_STRIDE + 2 * MAX_K)
    short = Smax <= 2 * rpb
    stash = (not short) and N < (1 << 31) and lds1_base + 4 * Smax <= LDS_LIMIT
    ordered = B * Smax <= ORDERED_MAX
    two = bool(bwd_acc and vec and labels and ordered)
    rec = dict(vec=vec, tc=tc, rpb=rpb, loop="short" if short else "unrolled", stash=stash,
               lds1=lds1_base + (4 * Smax if stash else 0), two=two, early=2 * C <= BLOCK, lds3=0, cap=False, long_lists=False,
               slots_used=_cdiv(C, BLOCK) if not vec else 4)
    if not vec:
        rec["tail"] = "scalar"
    elif labels and ordered:
        rec["tail"] = "backfill"
        rec["lds3"] = 4 * B * Smax
        if two:
            rec["lds3"] = max(4 * ((B * Smax + 1) & ~1) + 8 * 2 * C + 4 * 3 * C, 4 * B)
        rec["cap"] = _cdiv(N, (ORD_BLOCK // tc) * 4) > BACKFILL_CAP
    elif ordered:
        rec["tail"] = "dense+ordered"
        rec["lds3"] = 4 * B * Smax
        rec["cap"] = _cdiv(N, rpb * 4) > DENSE_CAP
    else:
        rec["tail"] = "dense+gather"
        rec["cap"] = _cdiv(N, rpb * 4) > DENSE_CAP
        rec["long_lists"] = longest_list >= LONG_LIST
    return rec


def second_round_rows(C, N, tail):
    """(first, second): a row of the first and the matching row of the second round of a thread's rows under a binding grid cap
    (the row loops advance by 4 * grid * rows-per-workgroup)"""
    tc = _pow2_ceil_cap(C // 4, BLOCK)
    per = (ORD_BLOCK // tc if tail == "backfill" else BLOCK // tc) * (BACKFILL_CAP if tail == "backfill" else DENSE_CAP)
    assert N > 4 * per
    return 0, 4 * per


def carve_ws(ws_bytes, B, C, K):
    """carve_ws restated: ws_bytes a uint8 CPU tensor -> dict of views"""
    o = 0
    out = {}
    for name, dt, n in (("partial", torch.float64, 2 * B * C), ("coef", torch.float32, 4 * C), ("dys", torch.float32, B * C),
                        ("dlogits", torch.float32, B * K), ("loss_rows", torch.float32, B)):
        size = n * (8 if dt == torch.float64 else 4)
        out[name] = ws_bytes[o:o + size].view(dt).clone()
        o += size
    out["partial"] = out["partial"].reshape(B, 2, C)
    out["coef"] = out["coef"][:3 * C].reshape(3, C)
    out["dys"] = out["dys"].reshape(B, C)
    out["dlogits"] = out["dlogits"].reshape(B, K)
    return out


def ws_bytes(B, C, K):
    return 8 * 2 * B * C + 4 * (4 * C + B * C + B * K + B) + 64


# ---- recipes -------------------------------------------------------------------------------------------------------------------
TWICE, THRICE = 7, 9   # the node listed twice in row 3; the node shared by rows 4, 5, 6


def recipe(C, K, B, Smax, N, seed, loss_mode=None, ldj=None, lddj=None, shared=()):
    """Deterministic inputs.  pos: ragged rows with -1 padding (a row keeps 1 .. Smax leading entries, 20 % of a long row's
    entries are padding too); row 1 all padding (B >= 2); row 2 starts with the out-of-range ids N + 5 and 1 << 40 (B >= 3,
    Smax >= 2); row 3 lists node 7 twice (B >= 4, Smax >= 2); rows 4, 5, 6 share node 9 (B >= 7); shared = ((n, m), ...): node
    n in exactly m rows (rows 7 .. 7 + m - 1, slot n % Smax); nodes N - 2 and N - 1 are named by no row.  gamma of both signs.
    jk [N, ldj]: guard columns (ldj > C) hold NaN.  -> dict, with facts = what the recipe placed."""
    g = torch.Generator().manual_seed(seed)
    ldj, lddj = ldj or C, lddj or C
    jk = torch.full((N, ldj), float("nan"), dtype=torch.float32)
    jk[:, :C] = torch.randn(N, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    gamma[0] = 0.7
    if C > 1:
        gamma[1] = -0.9
    beta, alpha = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    reserved = {TWICE, THRICE, N - 2, N - 1} | {n for n, _ in shared}
    free = torch.tensor([n for n in range(N) if n not in reserved], dtype=torch.int64)
    if Smax <= free.numel() // 2:
        pos = torch.stack([free[torch.randperm(free.numel(), generator=g)[:Smax]] for _ in range(B)])
    else:
        pos = free[torch.randint(0, free.numel(), (B, Smax), generator=g)]
    if Smax > 8:
        pos[torch.rand(B, Smax, generator=g) < 0.2] = -1
    lens = torch.randint(1, Smax + 1, (B, ), generator=g)
    lens[0] = Smax
    pos[torch.arange(Smax).reshape(1, -1) >= lens.reshape(-1, 1)] = -1
    facts = dict(all_padding=None, out_of_range=None, twice=None, thrice=None, shared={})
    if B >= 2:
        pos[1, :] = -1
        facts["all_padding"] = 1
    if B >= 3 and Smax >= 2:
        pos[2, 0], pos[2, 1] = N + 5, 1 << 40
        facts["out_of_range"] = 2
    if B >= 4 and Smax >= 2:
        pos[3, 0] = pos[3, 1] = TWICE
        facts["twice"] = (3, TWICE)
    if B >= 7:
        pos[4, 0] = pos[5, 0] = pos[6, 0] = THRICE
        facts["thrice"] = THRICE
    for n, m in shared:
        assert 7 + m <= B and all(n % Smax != n2 % Smax for n2, _ in shared if n2 != n)
        pos[7:7 + m, n % Smax] = n
        facts["shared"][n] = m
    Wh, bh = torch.randn(K, C, generator=g) / C ** 0.5, torch.randn(K, generator=g)
    loss_mode = (1 if K == 1 else 0) if loss_mode is None else loss_mode
    target = torch.randint(0, K, (B, ), generator=g) if loss_mode == 0 else (torch.rand(B, K, generator=g) > 0.5).float()
    return dict(jk=jk, gamma=gamma, beta=beta, alpha=alpha, pos=pos, Wh=Wh, bh=bh, target=target, loss_mode=loss_mode, C=C, K=K,
                B=B, Smax=Smax, N=N, ldj=ldj, lddj=lddj, facts=facts, eps=1e-5)


def for_mode(ins, mode):
    """the recipe with the head weights scaled for the pool mode (sum: / Smax, size: / sqrt(Smax)), so that the logits stay
    O(1) whatever the row length: with saturated logits the cross-entropy gradient is the rounding of 1 - softmax, which no
    end-to-end comparison at 1e-5 can hold (the stage gates can, and do not need this)"""
    out = dict(ins)
    out["Wh"] = ins["Wh"] / {"sum": float(ins["Smax"]), "size": float(ins["Smax"]) ** 0.5, "mean": 1.0}[mode]
    return out


def valid_of(pos, N):
    return (pos >= 0) & (pos < N)


def multiplicity(pos, N):
    """entries naming each node (a node listed twice in a row counts twice), int64 [N]"""
    v = pos[valid_of(pos, N)]
    return torch.bincount(v, minlength=N)


def pool_scale(mode, cnt):
    cnt = cnt.to(F64)
    if mode == "mean":
        return 1.0 / cnt.clamp(min=1)
    if mode == "size":
        return torch.where(cnt > 0, cnt.clamp(min=1).rsqrt(), torch.zeros_like(cnt))
    return torch.ones_like(cnt)


# ---- stages: every function -> (want, mass) or a dict of such pairs, all fp64 ------------------------------------------------------
def stage_saved(jk, gamma, beta, alpha, eps):
    """gn_math.h gn_fwd_coeffs from exact column sums -> saved [4, C] = mean, rstd, scale, shift"""
    x, ga, be, a = jk.to(F64), gamma.to(F64), beta.to(F64), alpha.to(F64)
    N = x.shape[0]
    mu, mu_m = x.sum(0) / N, x.abs().sum(0) / N
    k = 2 * a - a * a
    var = ((x * x).sum(0) / N - mu * mu * k).clamp(min=0)
    var_m = (x * x).sum(0) / N + mu * mu * k.abs()          # the cancelling variance sum
    rstd = (var + eps).rsqrt()
    rstd_m = rstd * (1 + 0.5 * var_m / (var + eps))
    scale, scale_m = ga * rstd, ga.abs() * rstd_m
    shift = be - scale * a * mu
    shift_m = be.abs() + a.abs() * (scale_m * mu.abs() + scale.abs() * mu_m)
    return torch.stack([mu, rstd, scale, shift]), torch.stack([mu_m, rstd_m, scale_m, shift_m])


def _rows(jk, pos):
    N = jk.shape[0]
    v = valid_of(pos, N)
    return jk[pos.clamp(0, N - 1)], v.to(F64).unsqueeze(-1), v.sum(1)   # [B, S, C], [B, S, 1], [B]


def stage_pooled(jk, saved, pos, mode):
    x, v, cnt = _rows(jk.to(F64), pos)
    scale, shift = saved[2].to(F64), saved[3].to(F64)
    sc = pool_scale(mode, cnt).unsqueeze(-1)
    return sc * ((x * scale + shift) * v).sum(1), sc * (((x * scale).abs() + shift.abs()) * v).sum(1)


def stage_logits(pooled, Wh, bh):
    p, W, b = pooled.to(F64), Wh.to(F64), bh.to(F64)
    return p @ W.t() + b, p.abs() @ W.abs().t() + b.abs()


F32_TINY = 2.0**-126  # the smallest normal fp32: below it a softmax / sigmoid value may underflow to 0


def stage_loss(logits, target, loss_mode, grad_loss=1.0):
    """-> dict: loss_rows, dlogits (grade the device loss with `stage_mean`).
    Mass of d logits (changed after the first GPU run, not the bar): softmax_k = exp(z_k - m - log se) is an exponential of a
    fp32 DIFFERENCE, so the roundings of its addends z_k, m, log se reach it multiplied by softmax_k itself — the mass is
    softmax_k * (1 + |z_k| + |m| + |log se|) + onehot, not softmax_k + onehot (at |z| ~ 50 the plain form asked for less than
    one ulp of the exponent) — and a softmax / sigmoid value below the fp32 normal range may be flushed to 0: the bar gets the
    absolute floor 2^-126 * |grad_loss| / denominator (as 2^-126 / 1e-5 of mass)."""
    z = logits.to(F64)
    B, K = z.shape
    floor = F32_TINY / TOL
    if loss_mode == 0:
        t = target.to(torch.int64).reshape(-1, 1)
        m = z.max(1).values
        lse = torch.logsumexp(z, 1)
        zt = z.gather(1, t).reshape(-1)
        rows, rows_m = lse - zt, m.abs() + (lse - m).abs() + zt.abs()
        oh = torch.nn.functional.one_hot(t.reshape(-1), K).to(F64)
        sm = torch.softmax(z, 1)
        cond = 1 + z.abs() + (m.abs() + (lse - m).abs()).reshape(-1, 1)
        dl, dl_m = grad_loss / B * (sm - oh), abs(grad_loss) / B * (sm * cond + oh + floor)
    else:
        y = target.to(F64).reshape(B, K)
        t1, t2, t3 = z.clamp(min=0), z * y, torch.log1p(torch.exp(-z.abs()))
        rows, rows_m = (t1 - t2 + t3).sum(1), (t1 + t2.abs() + t3).sum(1)
        sg = torch.sigmoid(z)
        dl, dl_m = grad_loss / (B * K) * (sg - y), abs(grad_loss) / (B * K) * (sg + y.abs() + floor)
    return dict(loss_rows=(rows, rows_m), dlogits=(dl, dl_m))


def stage_mean(loss_rows, loss_mode, K):
    r = loss_rows.to(F64)
    den = r.numel() * (1 if loss_mode == 0 else K)
    return r.sum() / den, r.abs().sum() / den


def stage_dys(dlogits, Wh, pos, N, mode):
    sc = pool_scale(mode, valid_of(pos, N).sum(1)).unsqueeze(-1)
    dl, W = dlogits.to(F64), Wh.to(F64)
    return sc * (dl @ W), sc * (dl.abs() @ W.abs())


def stage_head_grads(dlogits, pooled, prev_dWh=None, prev_dbh=None):
    dl, p = dlogits.to(F64), pooled.to(F64)
    dWh, dWh_m, dbh, dbh_m = dl.t() @ p, dl.abs().t() @ p.abs(), dl.sum(0), dl.abs().sum(0)
    if prev_dWh is not None:
        dWh, dWh_m, dbh, dbh_m = dWh + prev_dWh.to(F64), dWh_m + prev_dWh.to(F64).abs(), dbh + prev_dbh.to(F64), dbh_m + prev_dbh.to(F64).abs()
    return dict(dWh=(dWh, dWh_m), dbh=(dbh, dbh_m))


def stage_partial(dys, jk, saved, alpha, pos):
    """[B, 2, C]: cnt * dy and dy * (sum of xhat over the row's valid entries)"""
    x, v, cnt = _rows(jk.to(F64), pos)
    mu, rstd, a, dy = saved[0].to(F64), saved[1].to(F64), alpha.to(F64), dys.to(F64)
    xh = (((x - a * mu) * rstd) * v).sum(1)
    xh_m = (((x.abs() + (a * mu).abs()) * rstd) * v).sum(1)
    c = cnt.to(F64).unsqueeze(-1)
    return torch.stack([c * dy, dy * xh], 1), torch.stack([c * dy.abs(), dy.abs() * xh_m], 1)


def stage_gn_bwd(partial, partial_m, N, gamma, alpha, saved, prev=None):
    """gn_bwd_coeffs restated from S1 = sum_b partial[b, 0], S2 = sum_b partial[b, 1] -> dict: coef [3, C] = A, Bx, K; dgamma,
    dbeta, dalpha (prev = (dgamma, dbeta, dalpha) previous contents under acc_gn)"""
    S1, S2, M1, M2 = partial[:, 0].sum(0), partial[:, 1].sum(0), partial_m[:, 0].sum(0), partial_m[:, 1].sum(0)
    g, a, mu, r = gamma.to(F64), alpha.to(F64), saved[0].to(F64), saved[1].to(F64)
    m2, m2_m = S2 / N, M2 / N
    sum_xhat = r * N * mu * (1 - a)
    sum_do, sum_do_m = g * r * (S1 - sum_xhat * m2), (g * r).abs() * (M1 + sum_xhat.abs() * m2_m)
    A = g * r
    Bx, Bx_m = -g * r * r * m2, (g * r * r).abs() * m2_m
    Kc = g * r * r * m2 * a * mu - a * (sum_do / N)
    Kc_m = (g * r * r * a * mu).abs() * m2_m + a.abs() * sum_do_m / N
    da, da_m = -mu * sum_do, mu.abs() * sum_do_m
    out = dict(coef=(torch.stack([A, Bx, Kc]), torch.stack([A.abs(), Bx_m, Kc_m])), dgamma=(S2, M2), dbeta=(S1, M1), dalpha=(da, da_m))
    if prev is not None:
        for k, p in zip(("dgamma", "dbeta", "dalpha"), prev):
            out[k] = (out[k][0] + p.to(F64), out[k][1] + p.to(F64).abs())
    return out


def stage_djk(jk, coef, coef_m, dys, pos, rows=None):
    """Bx * x + K + A * sum of dys over the entries naming the row, for all rows or the given ones (int64, ascending)"""
    N = jk.shape[0]
    dy = dys.to(F64)
    B, S = pos.shape
    v = valid_of(pos, N)
    node = pos[v]
    bidx = torch.arange(B).reshape(-1, 1).expand(B, S)[v]
    if rows is not None:
        where = torch.full((N, ), -1, dtype=torch.int64)
        where[rows] = torch.arange(rows.numel())
        sel = where[node] >= 0
        node, bidx, jk = where[node][sel], bidx[sel], jk[rows]
    G = torch.zeros(jk.shape[0], dy.shape[1], dtype=F64).index_add_(0, node, dy[bidx])
    Gm = torch.zeros(jk.shape[0], dy.shape[1], dtype=F64).index_add_(0, node, dy[bidx].abs())
    x = jk.to(F64)
    return coef[1] * x + coef[2] + coef[0] * G, coef_m[1] * x.abs() + coef_m[2] + coef_m[0] * Gm


# ---- the gate ---------------------------------------------------------------------------------------------------------------------
def gate(got, want, mass, tol=TOL):
    """-> (ok, worst share of the bar, index of the worst element).  mass 0: the element must be exactly 0."""
    got, want, mass = got.to(F64).reshape(-1), want.to(F64).reshape(-1), mass.to(F64).reshape(-1)
    assert got.shape == want.shape == mass.shape
    err = (got - want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    bar = tol * mass
    share = torch.where(bar > 0, err / bar.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    if share.numel() == 0:
        return True, 0.0, -1
    w = int(share.argmax())
    return bool(share[w] <= 1.0), float(share[w]), w


def rel_inf(a, b):
    a, b = a.to(F64), b.to(F64)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


# ---- the chain: the stages on their own outputs (the end-to-end fp64 statement) ---------------------------------------------------------
def chain(ins, mode, grad_loss=1.0, prev=None, rows=None):
    """prev: dict of previous contents (dWh, dbh under acc_head; dgamma, dbeta, dalpha under acc_gn); rows: the rows of d jk to
    return (all by default)."""
    C, N = ins["C"], ins["N"]
    prev = prev or {}
    jk = ins["jk"][:, :C]
    saved, _ = stage_saved(jk, ins["gamma"], ins["beta"], ins["alpha"], ins["eps"])
    pooled, _ = stage_pooled(jk, saved, ins["pos"], mode)
    logits, _ = stage_logits(pooled, ins["Wh"], ins["bh"])
    L = stage_loss(logits, ins["target"], ins["loss_mode"], grad_loss)
    loss, _ = stage_mean(L["loss_rows"][0], ins["loss_mode"], ins["K"])
    dl = L["dlogits"][0]
    dys, _ = stage_dys(dl, ins["Wh"], ins["pos"], N, mode)
    H = stage_head_grads(dl, pooled, prev.get("dWh"), prev.get("dbh"))
    part, part_m = stage_partial(dys, jk, saved, ins["alpha"], ins["pos"])
    gn_prev = (prev["dgamma"], prev["dbeta"], prev["dalpha"]) if "dgamma" in prev else None
    Gn = stage_gn_bwd(part, part_m, N, ins["gamma"], ins["alpha"], saved, gn_prev)
    djk, _ = stage_djk(jk, Gn["coef"][0], Gn["coef"][1], dys, ins["pos"], rows)
    return dict(saved=saved, pooled=pooled, logits=logits, loss=loss, dlogits=dl, dys=dys, dWh=H["dWh"][0], dbh=H["dbh"][0],
                dgamma=Gn["dgamma"][0], dbeta=Gn["dbeta"][0], dalpha=Gn["dalpha"][0], coef=Gn["coef"][0], djk=djk)


def autograd_readout(ins, mode, grad_loss=1.0):
    """torch autograd in fp64 over GraphNorm (PyG, batch=None) -> pool -> Linear -> the torch loss; what `chain` is pinned to"""
    C, N = ins["C"], ins["N"]
    jk, gamma, beta, alpha, Wh, bh = (ins[k].double().clone().requires_grad_(True) for k in ("jk", "gamma", "beta", "alpha", "Wh", "bh"))
    x = jk[:, :C]
    mu = x.mean(0)
    cen = x - alpha * mu
    y = gamma * cen * (cen.pow(2).mean(0) + ins["eps"]).rsqrt() + beta
    pos = ins["pos"]
    v = valid_of(pos, N).double().unsqueeze(-1)
    s = (y[pos.clamp(0, N - 1)] * v).sum(1)
    cnt = v.sum(1)
    pooled = s if mode == "sum" else s / cnt.clamp(min=1) if mode == "mean" else s * torch.where(cnt > 0, cnt.clamp(min=1).rsqrt(), 0 * cnt)
    logits = pooled @ Wh.t() + bh
    if ins["loss_mode"] == 0:
        loss = torch.nn.functional.cross_entropy(logits, ins["target"])
    else:
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits.flatten(), ins["target"].double().flatten())
    grads = torch.autograd.grad(loss * grad_loss, [jk, gamma, beta, alpha, Wh, bh])
    out = dict(zip(("djk", "dgamma", "dbeta", "dalpha", "dWh", "dbh"), grads))
    out["djk"] = out["djk"][:, :C]
    out.update(pooled=pooled.detach(), logits=logits.detach(), loss=loss.detach())
    return out


def grade(got, ins, mode, rec, grad_loss=1.0, prev=None, saved=None, rows=None):
    """Every stage of one call's outputs (`got`: the entry's outputs plus the carved workspace and `saved` as the call used or
    wrote it) through the gate -> dict stage -> (ok, worst share of the bar, index); asserts nothing.  rows: the rows of d jk
    to grade (all by default)."""
    C, N, K = ins["C"], ins["N"], ins["K"]
    prev = prev or {}
    jk = ins["jk"][:, :C]
    sv = got["saved"].reshape(4, C) if saved is None else saved
    out = {}

    def put(name, g, wm):
        out[name] = gate(g, wm[0], wm[1])

    put("pooled", got["pooled"], stage_pooled(jk, sv, ins["pos"], mode))
    put("logits", got["logits"], stage_logits(got["pooled"], ins["Wh"], ins["bh"]))
    L = stage_loss(got["logits"], ins["target"], ins["loss_mode"], grad_loss)
    put("loss_rows", got["loss_rows"], L["loss_rows"])
    put("dlogits", got["dlogits"], L["dlogits"])
    put("loss", got["loss"], stage_mean(got["loss_rows"], ins["loss_mode"], K))
    put("dys", got["dys"], stage_dys(got["dlogits"], ins["Wh"], ins["pos"], N, mode))
    H = stage_head_grads(got["dlogits"], got["pooled"], prev.get("dWh"), prev.get("dbh"))
    put("dWh", got["dWh"], H["dWh"])
    put("dbh", got["dbh"], H["dbh"])
    part, part_m = stage_partial(got["dys"], jk, sv, ins["alpha"], ins["pos"])
    if not rec["two"]:
        put("partial", got["partial"], (part, part_m))
    gn_prev = (prev["dgamma"], prev["dbeta"], prev["dalpha"]) if "dgamma" in prev else None
    Gn = stage_gn_bwd(part, part_m, N, ins["gamma"], ins["alpha"], sv, gn_prev)
    if not rec["two"]:
        put("coef", got["coef"], Gn["coef"])
    for k in ("dgamma", "dbeta", "dalpha"):
        put(k, got[k], Gn[k])
    g = got["djk"][:, :C] if rows is None else got["djk"][rows][:, :C]
    put("djk", g, stage_djk(jk, Gn["coef"][0], Gn["coef"][1], got["dys"], ins["pos"], rows))
    return out
