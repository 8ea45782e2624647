"""Kernel value tests of the narrow dense family (glass_amd/csrc/dense_narrow.hip and the narrow branches of linear.hip / dense.hip,
hidden <= 32) against the fp64 oracle of tests/narrow_dense_oracle.py: every register-width instantiation at H = HP and below it,
the edges of the 256-row workgroups, of the 64-row weight-gradient slabs and of the reduce's 16 / 64-slab walk, each fusion on its
own, and operands of any alignment.  The kernels are driven through the launch helpers of glass_amd/stack.py and through
ops.dual_linear_mix; for this family the stack tuple is (W, b, dW, db, W, W), so no model is needed.

Every output lives in a wider NaN-filled buffer: what a kernel writes outside its view, or leaves unwritten inside, shows.
Tolerance: TOL on rel_inf per tensor; sums (statistics, GraphNorm partials, dW, db) per column / per element against
TOL * sum |term| — a column whose sum cancels is graded against its own terms, not against another column.  The statistics
are, in addition, the exact double sums of the kernel's own fp32 outputs per 256-row block (1e-12 of sum |term|: doubles add
fp32 values and their squares without rounding beyond the order of the additions)."""
import functools

import pytest
import torch

import narrow_dense_oracle as NO
from helpers import rel_inf, record_parity
from oracle import glass_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5
EXACT = 1e-12
DEV = "cuda:0"
Z = 0.85
NAN = float("nan")
PATTERNS = ("none", "all", "random", "last")
SHAPES = [(H, NO.SWEEP_N) for H in NO.SWEEP_WIDTHS] + [(H, N) for N in NO.ROW_SWEEP for H in NO.ROW_WIDTHS]
PAIRS = [False, True]   # comb


def _stack():
    from glass_amd import stack
    return stack


def _ops():
    from glass_amd import ops
    return ops


def _pair(comb):
    return "comb" if comb else "trans"


# ---- buffers ---------------------------------------------------------------------------------------------------------------
class Buf:
    """A [rows, cols] view `v` with leading dimension ld, `off` elements into a NaN-filled flat buffer."""
    def __init__(self, rows, cols, ld, off, src=None, dtype=torch.float32):
        self.flat = torch.full((off + rows * ld + 2 * ld + 8, ), NAN, dtype=dtype, device=DEV)
        self.v = torch.as_strided(self.flat, (rows, cols), (ld, 1), off)
        self.inside = torch.zeros(self.flat.numel(), dtype=torch.bool, device=DEV)
        torch.as_strided(self.inside, (rows, cols), (ld, 1), off).fill_(True)
        if src is not None:
            self.v.copy_(src)

    def check(self, tag):
        assert bool(torch.isnan(self.flat[~self.inside]).all()), f"{tag}: written outside its view"
        assert not bool(torch.isnan(self.flat[self.inside]).any()), f"{tag}: NaN or unwritten element inside its view"
        return self.v

    def cpu(self):
        return self.v.detach().cpu().double()


def _mat(rows, cols, H, una=False, src=None):
    """aligned form: two guard rows and two guard columns in front, ld = cols + 4.  Unaligned form (una): ld = H + 3 for an
    H-wide operand, cols + 1 otherwise (2H + 1), the view starting one float into the buffer."""
    if una:
        ld = cols + 3 if cols == H else cols + 1
        b = Buf(rows, cols, ld, 1, src)
        assert b.v.data_ptr() % 16 == 4
        return b
    ld = cols + 4
    return Buf(rows, cols, ld, 2 * ld + 2, src)


def _vec(src, una=False):
    """a contiguous operand (weight, bias): 16-byte aligned, or one float into its buffer"""
    flat = torch.full((src.numel() + 5, ), NAN, device=DEV)
    off = 1 if una else 4
    v = flat[off:off + src.numel()].view(src.shape)
    v.copy_(src)
    assert v.data_ptr() % 16 == (4 if una else 0)
    return v


def _mask(m, una=False):
    buf = torch.ones(m.numel() + 3, dtype=torch.uint8, device=DEV)
    v = buf[1:1 + m.numel()] if una else buf[:m.numel()]
    v.copy_(m)
    assert v.data_ptr() % 2 == (1 if una else 0)
    return v


def _blocks_buf(nblk, H):
    """[nblk, 2, H] float64 inside a NaN buffer with one guard block on either side"""
    return Buf(nblk, 2 * H, 2 * H, 2 * H, dtype=torch.float64)


def _as_blocks(buf, nblk, H):
    return buf.v.view(nblk, 2, H)


# ---- references ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=512)
def _case(H, N, comb, pattern="random"):
    """inputs of one pair (fp32, CPU) with the forward's fp64 reference; computed once, shared by the tests, never changed"""
    p = NO.make_pair(H, N, comb, pattern=pattern)
    p["T_ref"], p["out_ref"] = NO.fwd(p["xa"], p["xb"], p["W"], p["b"], p["mask"], Z, p["act"])
    p["T32"] = p["T_ref"].float()   # the backward kernels' input
    return p


def _sums_check(got, ref, ref_abs, tag, tol=TOL):
    """|got - ref| <= tol * sum |term|, element by element; returns the largest achieved ratio"""
    err = (got - ref).abs()
    bad = err > tol * ref_abs
    assert not bool(bad.any()), f"{tag}: {int(bad.sum())} sums off by more than {tol:g} of their terms; worst {float((err / ref_abs.clamp_min(1e-300)).max()):.3e}"
    return float((err / ref_abs.clamp_min(1e-300)).max())


def _stats_check(got, out_k, out_ref, tag):
    """got [nblk, 2, H] (CPU fp64): per block the exact sums of the kernel's own outputs; per column within TOL of the oracle"""
    _sums_check(got, NO.stats(out_k), NO.stats_abs(out_k), tag + " (own outputs, per block)", EXACT)
    return _sums_check(got.sum(0), NO.stats(out_ref).sum(0), NO.stats_abs(out_ref).sum(0), tag + " (oracle, per column)")


class Dev:
    """device operands of one case"""
    def __init__(self, p, una=False):
        H, N = p["H"], p["N"]
        self.p, self.H, self.N, self.una = p, H, N, una
        self.xa = _mat(N, H, H, una, p["xa"])
        self.xb = _mat(N, H, H, una, p["xb"]) if p["comb"] else None
        self.W, self.b = _vec(p["W"], una), _vec(p["b"], una)
        self.mask = _mask(p["mask"], una)
        self.dsrc = _mat(N, H, H, una, p["dsrc"])
        self.T32 = _mat(N, 2 * H, H, una, p["T32"])
        self.addend = _mat(N, p["n_out"], H, una, p["addend"])
        self.nblk = NO.blocks(N, NO.ROWS)

    def xbv(self):
        return None if self.xb is None else self.xb.v

    def stack(self, dW=None, db=None):
        return (self.W, self.b, dW, db, self.W, self.W)

    def forward(self, stats=True):
        H, N = self.H, self.N
        T, out = _mat(N, 2 * H, H, self.una), _mat(N, H, H, self.una)
        cst = _blocks_buf(self.nblk, H) if stats else None
        _stack()._dual_fwd(self.xa.v, self.xbv(), self.stack(), self.mask, Z, self.p["act"], T.v, out.v,
                           None if cst is None else _as_blocks(cst, self.nblk, H))
        return T, out, cst

    def dgrad(self, T, addend=None, drop=None, gn=None):
        din = _mat(self.N, self.p["n_out"], self.H, self.una)
        _stack()._dual_dgrad(self.dsrc.v, T, self.stack(), self.mask, Z, self.p["act"], self.p["n_out"], addend, din.v, drop, gn)
        return din


# ---- 1. forward + statistics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("comb", PAIRS)
@pytest.mark.parametrize("H,N", SHAPES)
def test_forward_and_stats(H, N, comb):
    """T, out and the per-workgroup column sums against the oracle under four label patterns; guards and padding untouched, one
    statistics block per workgroup and nothing beyond; a second run gives the same bits."""
    worst = {"T": 0.0, "out": 0.0, "stats": 0.0}
    for pattern in PATTERNS:
        p = _case(H, N, comb, pattern)
        d = Dev(p)
        T, out, cst = d.forward()
        tag = f"fwd {_pair(comb)} H={H} N={N} mask={pattern}"
        T.check(tag + " T"), out.check(tag + " out"), cst.check(tag + " stats")
        e_T, e_o = rel_inf(T.cpu(), p["T_ref"]), rel_inf(out.cpu(), p["out_ref"])
        print(f"{tag}: T {e_T:.2e} out {e_o:.2e}")
        assert e_T < TOL and e_o < TOL, (tag, e_T, e_o)
        e_s = _stats_check(_as_blocks(cst, d.nblk, H).cpu(), out.cpu(), p["out_ref"], tag + " stats")
        T2, out2, cst2 = d.forward()
        assert torch.equal(T2.v, T.v) and torch.equal(out2.v, out.v) and torch.equal(cst2.v, cst.v), tag + ": second run differs"
        # without the statistics and without T the same `out`
        outn = _mat(N, H, H)
        _stack()._dual_fwd(d.xa.v, d.xbv(), d.stack(), d.mask, Z, p["act"], None, outn.v)
        assert torch.equal(outn.check(tag + " out alone"), out.v)
        worst = {"T": max(worst["T"], e_T), "out": max(worst["out"], e_o), "stats": max(worst["stats"], e_s)}
    record_parity(f"kernel/narrow_fwd_{_pair(comb)}_H{H}_N{N}", T_rel_inf=worst["T"], out_rel_inf=worst["out"],
                  stats_col_ratio=worst["stats"])


# ---- 2. unaligned operands ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("comb", PAIRS)
@pytest.mark.parametrize("H", [5, 17, 32])
def test_unaligned_operands(H, comb):
    """Every matrix operand a view with leading dimension H + 3 / 2H + 1 that starts one float into its buffer, weight and bias
    4-byte aligned, the label bytes at an odd address, dW strided (lddw = I + 1): forward, data gradient and weight gradient
    give the bits of the aligned run."""
    N = 257
    p = _case(H, N, comb)
    I, n_out, act = p["K"], p["n_out"], p["act"]
    res = {}
    for una in (False, True):
        d = Dev(p, una)
        tag = f"{'unaligned' if una else 'aligned'} {_pair(comb)} H={H}"
        if una:
            for b in (d.xa, d.dsrc, d.T32, d.addend) + ((d.xb, ) if comb else ()):
                assert b.v.data_ptr() % 16 == 4 and b.v.stride(0) in (H + 3, 2 * H + 1)
        T, out, cst = d.forward()
        T.check(tag + " T"), out.check(tag + " out"), cst.check(tag + " stats")
        din = d.dgrad(d.T32.v, d.addend.v)
        din.check(tag + " din")
        dW = Buf(2 * H, I, I + 1, 1) if una else _mat(2 * H, I, H)
        db = Buf(1, 2 * H, 2 * H, 1 if una else 4)
        pending = []
        _stack()._dual_wgrad(d.dsrc.v, d.T32.v, d.stack(dW.v, db.v[0]), d.mask, Z, act, d.xa.v, d.xbv(), pending, acc=0)
        _stack()._reduce_pending(pending)
        dW.check(tag + " dW"), db.check(tag + " db")
        res[una] = (T, out, cst, din, dW, db)
    for name, a, b in zip(("T", "out", "stats", "din", "dW", "db"), res[False], res[True]):
        assert torch.equal(a.v, b.v), f"{_pair(comb)} H={H}: {name} differs between the aligned and the unaligned run"
    T, out, cst, din, dW, db = res[True]
    assert rel_inf(T.cpu(), p["T_ref"]) < TOL and rel_inf(out.cpu(), p["out_ref"]) < TOL
    assert rel_inf(din.cpu(), NO.dgrad(p["dsrc"], p["T32"], p["W"], p["mask"], Z, act, n_out, p["addend"])) < TOL
    rW, rb = NO.wgrad(p["dsrc"], p["T32"], p["mask"], Z, act, p["xa"], p["xb"])
    aW, ab = NO.wgrad_abs(p["dsrc"], p["T32"], p["mask"], Z, act, p["xa"], p["xb"])
    _sums_check(dW.cpu(), rW, aW, "unaligned dW"), _sums_check(db.cpu()[0], rb, ab, "unaligned db")


# ---- 3. GraphNorm prologue ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("N", [257, 1025])
@pytest.mark.parametrize("H", [8, 12, 17, 24, 28])
def test_graphnorm_prologue(H, N, p_drop, gather):
    """Trans pair with gn = (saved, ELU, p, call, side): the operand is ELU(x * scale + shift) (+ dropout) formed while loading
    and written to `side`; optionally its rows are gathered from a 37-row table.  `side` against the formula (p = 0) and, bit
    for bit, against the stand-alone GraphNorm apply with the same (p, call id) — the mask is that kernel's; T, out and the
    statistics referenced on the kernel's own `side`."""
    stack, ops = _stack(), _ops()
    p = _case(H, N, False)
    gen = torch.Generator().manual_seed(31 * H + N + int(gather))
    V, call = 37, 5
    scale, shift = torch.rand(H, generator=gen) + 0.5, torch.randn(H, generator=gen) * 0.1
    saved = _vec(torch.cat([torch.zeros(H), torch.ones(H), scale, shift]), una=True)
    d = Dev(p)
    if gather:
        table = torch.randn(V, H, generator=gen)
        idx = torch.randint(0, V, (N, ), generator=gen, dtype=torch.int64)
        idx[0], idx[-1], idx[N // 2] = V - 1, 0, V - 1
        assert int(idx.min()) == 0 and int(idx.max()) == V - 1
        tbuf = _mat(V + 3, H, H)          # rows beyond the table stay NaN
        tbuf.v[:V].copy_(table)
        src, rows, idx_d = tbuf.v[:V], table[idx], idx.to(DEV)
    else:
        src, rows, idx_d = d.xa.v, p["xa"], None
    formula = NO.prologue(rows, saved.cpu(), NO.ACT_ELU)
    tag = f"gn prologue H={H} N={N} p={p_drop} gather={int(gather)}"
    got = []
    for _ in range(2):
        ops.rng_seed(4242, torch.device(DEV))
        T, out, side, cst = _mat(N, 2 * H, H), _mat(N, H, H), _mat(N, H, H), _blocks_buf(d.nblk, H)
        stack._dual_fwd(src, None, d.stack(), d.mask, Z, NO.ACT_ELU, T.v, out.v, _as_blocks(cst, d.nblk, H),
                        gn=(saved, NO.ACT_ELU, p_drop, call, side.v), xa_index=idx_d)
        T.check(tag + " T"), out.check(tag + " out"), side.check(tag + " side"), cst.check(tag + " stats")
        got.append((T, out, side, cst))
    for a, b in zip(*got):
        assert torch.equal(a.v, b.v), tag + ": second run differs"
    T, out, side, cst = got[0]
    # the stand-alone GraphNorm apply on the same rows, same (p, call id), same dropout words
    ops.rng_seed(4242, torch.device(DEV))
    alone = torch.full((N, H), NAN, device=DEV)
    stack._GN(None).apply(rows.to(DEV).contiguous(), alone, saved, NO.ACT_ELU, p_drop, call)
    assert torch.equal(side.v, alone), tag + ": side output is not the stand-alone GraphNorm's"
    s64 = side.cpu()
    if p_drop == 0.0:
        e_side = rel_inf(s64, formula)
    else:
        kept = s64 != 0
        assert 0.4 < float(kept.double().mean()) < 0.6, tag
        e_side = rel_inf(s64[kept], (formula / (1 - p_drop))[kept])
    assert e_side < TOL, (tag, e_side)
    T_ref, out_ref = NO.fwd(side.v.cpu(), None, p["W"], p["b"], p["mask"], Z, NO.ACT_ELU)
    e_T, e_o = rel_inf(T.cpu(), T_ref), rel_inf(out.cpu(), out_ref)
    print(f"{tag}: side {e_side:.2e} T {e_T:.2e} out {e_o:.2e}")
    assert e_T < TOL and e_o < TOL, (tag, e_T, e_o)
    e_s = _stats_check(_as_blocks(cst, d.nblk, H).cpu(), out.cpu(), out_ref, tag + " stats")
    record_parity(f"kernel/narrow_gn_prologue_H{H}_N{N}_p{p_drop}_gather{int(gather)}", side_rel_inf=e_side, T_rel_inf=e_T,
                  out_rel_inf=e_o, stats_col_ratio=e_s)


# ---- 4. data gradient ------------------------------------------------------------------------------------------------------
def _keep_scales(N, H, p_drop, call, seed):
    """the keep-scales (0 or 1 / (1 - p)) the stand-alone GraphNorm of width H draws for (p, call id): gamma = 0, beta = 1
    make its output the scale itself"""
    ops = _ops()
    ops.rng_seed(seed, torch.device(DEV))
    ones, zeros = torch.ones(H, device=DEV), torch.zeros(H, device=DEV)
    return ops.graphnorm(torch.randn(N, H, device=DEV), zeros, ones, ones, p_drop=p_drop, call_id=call)


@pytest.mark.parametrize("comb", PAIRS)
@pytest.mark.parametrize("H,N", SHAPES)
def test_data_gradient(H, N, comb):
    """din = dZ W (+ addend) against the oracle, plain and with a strided addend; for the trans pair the dropout epilogue is, bit
    for bit, the plain result under the mask the stand-alone GraphNorm of width H draws for the same (p, call id)."""
    p = _case(H, N, comb)
    d = Dev(p)
    act, n_out = p["act"], p["n_out"]
    tag = f"dgrad {_pair(comb)} H={H} N={N}"
    plain = d.dgrad(d.T32.v)
    added = d.dgrad(d.T32.v, d.addend.v)
    plain.check(tag + " plain"), added.check(tag + " addend")
    ref = NO.dgrad(p["dsrc"], p["T32"], p["W"], p["mask"], Z, act, n_out)
    e_p, e_a = rel_inf(plain.cpu(), ref), rel_inf(added.cpu(), ref + p["addend"].double())
    print(f"{tag}: plain {e_p:.2e} with addend {e_a:.2e}")
    assert e_p < TOL and e_a < TOL, (tag, e_p, e_a)
    again = d.dgrad(d.T32.v, d.addend.v)
    assert torch.equal(again.v, added.v), tag + ": second run differs"
    if not comb:
        pd, call = 0.5, 3
        scales = _keep_scales(N, H, pd, call, 99)
        kept = scales != 0
        if N * H >= 256:
            assert 0.4 < float(kept.float().mean()) < 0.6
        assert bool(((scales == 0) | (scales == 1 / (1 - pd))).all())
        dropped = d.dgrad(d.T32.v, drop=(pd, call))
        dropped.check(tag + " dropout")
        assert torch.equal(dropped.v, torch.where(kept, plain.v / (1 - pd), torch.zeros_like(plain.v))), tag + ": dropout epilogue"
    record_parity(f"kernel/narrow_dgrad_{_pair(comb)}_H{H}_N{N}", plain_rel_inf=e_p, addend_rel_inf=e_a)


# ---- 5. backward GraphNorm column sums in the data-gradient epilogue -------------------------------------------------------------
@pytest.mark.parametrize("comb", PAIRS)
@pytest.mark.parametrize("p_drop", [0.0, 0.5])
@pytest.mark.parametrize("gact", [NO.ACT_NONE, NO.ACT_ELU])
@pytest.mark.parametrize("N", [257, 1025])
@pytest.mark.parametrize("H", [8, 12, 17, 24, 28, 32])
def test_gn_backward_epilogue(H, N, gact, p_drop, comb):
    """gn = (partial, x, saved, alpha, act, p, call): the first H output columns are the gradient of a GraphNorm output; the
    epilogue leaves that GraphNorm's backward column sums (sum gp, sum gp xhat) per workgroup.  Per column against the oracle on
    the kernel's own `out`; `out` itself unchanged by the epilogue; and the GraphNorm backward fed with the partials agrees
    with the one that computes them itself."""
    from glass_amd import models
    stack = _stack()
    p = _case(H, N, comb)
    d = Dev(p)
    call, seed = 7, 123
    tag = f"gn bwd epilogue {_pair(comb)} H={H} N={N} act={gact} p={p_drop}"
    torch.manual_seed(17 * H + N)
    mod = models.GraphNorm(H).to(DEV)
    with torch.no_grad():
        mod.weight.uniform_(0.5, 1.5)
        mod.bias.uniform_(-0.3, 0.3)
        mod.mean_scale.uniform_(0.7, 1.1)
    gen = torch.Generator().manual_seed(H + N)
    x = _mat(N, H, H, src=torch.randn(N, H, generator=gen) * 2 + 0.5)
    xc = x.v.contiguous()
    gn = stack._GN(mod)
    saved = gn.stats(xc)
    plain = d.dgrad(d.T32.v)
    keep = None
    if p_drop > 0:
        keep = _keep_scales(N, H, p_drop, call, seed).cpu()
    _ops().rng_seed(seed, torch.device(DEV))
    part = _blocks_buf(d.nblk, H)
    part_v = _as_blocks(part, d.nblk, H)
    with_gn = d.dgrad(d.T32.v, gn=(part_v, x.v, saved, mod.mean_scale.detach(), gact, p_drop, call))
    with_gn.check(tag + " out"), part.check(tag + " partials")
    assert torch.equal(with_gn.v, plain.v), tag + ": the epilogue changed the data gradient"
    g = with_gn.cpu()[:, :H]
    args = (g, x.v.cpu(), saved.cpu(), mod.mean_scale.detach().cpu(), gact, keep)
    e = _sums_check(part_v.cpu(), NO.gn_partials(*args), NO.gn_partials_abs(*args), tag)
    print(f"{tag}: partials within {e:.2e} of their terms")
    # the GraphNorm backward from these sums == the one that forms them itself
    dy = with_gn.v[:, :H]
    outs = []
    for partial in (None, part_v):
        for t in (mod.weight, mod.bias, mod.mean_scale):
            t.grad = torch.zeros_like(t)
        dx = _mat(N, H, H)
        gn.bwd(dy, xc, saved, dx.v, gact, p_drop, call, acc=0, partial=partial)
        dx.check(tag + " dx")
        outs.append((dx.cpu(), mod.weight.grad.cpu().double(), mod.bias.grad.cpu().double(), mod.mean_scale.grad.cpu().double()))
    errs = [rel_inf(a, b) for a, b in zip(outs[1], outs[0])]
    assert max(errs) < TOL, (tag, errs)
    record_parity(f"kernel/narrow_gn_bwd_{_pair(comb)}_H{H}_N{N}_act{gact}_p{p_drop}", partial_col_ratio=e, dx_rel_inf=errs[0],
                  dgamma_rel_inf=errs[1], dbeta_rel_inf=errs[2], dalpha_rel_inf=errs[3])


# ---- 6. weight gradient ------------------------------------------------------------------------------------------------------
def _arena(H, I, fill):
    """(flat, dW [2H, I], db [2H]): one storage, as the gradient arena holds a pair"""
    flat = torch.empty(2 * H * I + 2 * H, device=DEV)
    if isinstance(fill, torch.Tensor):
        flat.copy_(fill)
    else:
        flat.fill_(fill)
    return flat, flat[:2 * H * I].view(2 * H, I), flat[2 * H * I:]


@pytest.mark.parametrize("comb", PAIRS)
@pytest.mark.parametrize("H,N", SHAPES)
def test_weight_gradient(H, N, comb):
    """dW, db from the slab partials + the deferred reduce (overwriting and accumulating), from the direct form behind
    ops.dual_linear_mix (gradient arena live and detached) and from the fused backward entry: each element within TOL of its
    terms, all forms bit-identical when they overwrite; the workspace holds n_slabs * stride partial floats and nothing else."""
    import torch.nn as nn
    stack, ops = _stack(), _ops()
    p = _case(H, N, comb)
    d = Dev(p)
    act, I, n_out = p["act"], p["K"], p["n_out"]
    tag = f"wgrad {_pair(comb)} H={H} N={N}"
    # T of the kernel's own forward: what ops.dual_linear_mix keeps for its backward
    Tk, _out, _ = d.forward(stats=False)
    T_in = Tk.v if act != NO.ACT_NONE else None
    T_cpu = Tk.v.cpu() if act != NO.ACT_NONE else None
    rW, rb = NO.wgrad(p["dsrc"], T_cpu, p["mask"], Z, act, p["xa"], p["xb"])
    aW, ab = NO.wgrad_abs(p["dsrc"], T_cpu, p["mask"], Z, act, p["xa"], p["xb"])
    n_slabs, stride = NO.blocks(N, NO.SLAB), NO.wgrad_stride(2 * H, I)
    assert n_slabs == dict(NO.ROW_SWEEP).get(N, (6, 2))[0]
    # (a) partials + deferred reduce, overwriting a NaN arena
    ws = ops._wgrad_workspace(torch.device(DEV), N, 2 * H, I, slot=("stack", 0))
    ws.fill_(NAN)
    _, dW0, db0 = _arena(H, I, NAN)
    pending = []
    stack._dual_wgrad(d.dsrc.v, T_in, d.stack(dW0, db0), d.mask, Z, act, d.xa.v, d.xbv(), pending, acc=0)
    assert pending[0][0] == ws.data_ptr()
    stack._reduce_pending(pending)
    part = ws[:n_slabs * stride].view(n_slabs, stride)
    assert not bool(torch.isnan(part[:, :2 * H * I + 2 * H]).any()), tag + ": a slab partial was left unwritten"
    assert bool(torch.isnan(part[:, 2 * H * I + 2 * H:]).all()) and bool(torch.isnan(ws[n_slabs * stride:]).all()), \
        tag + ": workspace written beyond the slab partials"
    e_W = _sums_check(dW0.cpu().double(), rW, aW, tag + " dW")
    e_b = _sums_check(db0.cpu().double(), rb, ab, tag + " db")
    print(f"{tag}: dW within {e_W:.2e}, db within {e_b:.2e} of their terms")
    # (b) accumulating onto a non-zero arena: the arena's value is one more term
    gen = torch.Generator().manual_seed(H + N)
    base = torch.randn(2 * H * I + 2 * H, generator=gen)
    _, dW1, db1 = _arena(H, I, base)
    pending = []
    stack._dual_wgrad(d.dsrc.v, T_in, d.stack(dW1, db1), d.mask, Z, act, d.xa.v, d.xbv(), pending, acc=1)
    stack._reduce_pending(pending)
    bW, bb = base[:2 * H * I].view(2 * H, I).double(), base[2 * H * I:].double()
    _sums_check(dW1.cpu().double(), rW + bW, aW + bW.abs(), tag + " dW accumulated")
    _sums_check(db1.cpu().double(), rb + bb, ab + bb.abs(), tag + " db accumulated")
    # (c) the fused backward entry
    _, dW2, db2 = _arena(H, I, NAN)
    din = _mat(N, n_out, H)
    pending = []
    stack._dual_bwd(True, d.dsrc.v, T_in, d.stack(dW2, db2), d.mask, Z, act, n_out, None, din.v, d.xa.v, d.xbv(), pending, 0)
    stack._reduce_pending(pending)
    assert torch.equal(dW2, dW0) and torch.equal(db2, db0), tag + ": fused backward entry differs from the two launches"
    assert torch.equal(din.check(tag + " din of the fused entry"), d.dgrad(T_in).v)
    # (d) the direct form behind ops.dual_linear_mix: arena live (accumulates onto zeros), then detached (autograd gets dW, db)
    for live in (True, False):
        _, dW3, db3 = _arena(H, I, 0.0)
        lin1, lin0 = nn.Linear(I, H).to(DEV), nn.Linear(I, H).to(DEV)  # carriers for the autograd edges only
        if live:
            lin1.weight.grad, lin0.weight.grad, lin1.bias.grad, lin0.bias.grad = dW3[:H], dW3[H:], db3[:H], db3[H:]
        st = d.stack(dW3, db3)
        assert ops._arena_grads_live(st, (lin1.weight, lin0.weight, lin1.bias, lin0.bias)) == live
        xa = d.xa.v.detach().requires_grad_(True)
        xb = d.xbv().detach().requires_grad_(True) if comb else None
        out = ops.dual_linear_mix(xa, xb, lin1, lin0, d.mask, Z, act, st)
        assert torch.equal(out.detach(), _out.v)
        out.backward(d.dsrc.v.contiguous())
        if live:
            gW, gb = dW3, db3
        else:
            assert float(dW3.abs().max()) == 0.0 and float(db3.abs().max()) == 0.0
            gW, gb = torch.cat((lin1.weight.grad, lin0.weight.grad)), torch.cat((lin1.bias.grad, lin0.bias.grad))
        assert torch.equal(gW, dW0) and torch.equal(gb, db0), f"{tag}: direct form (arena live={live}) differs from the deferred reduce"
        assert torch.equal(xa.grad, din.v[:, :H])
        if comb:
            assert torch.equal(xb.grad, din.v[:, H:])
    record_parity(f"kernel/narrow_wgrad_{_pair(comb)}_H{H}_N{N}", dW_elem_ratio=e_W, db_elem_ratio=e_b)


# ---- 7. ops.dual_linear_mix end to end ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,N", [(H, N) for H in (1, 8, 17, 20, 32) for N in (1, 77, 1030)])
@pytest.mark.parametrize("comb", PAIRS)
def test_dual_linear_mix_narrow(H, N, comb):
    """test_gpu_kernels.py::test_dual_linear_mix_fused at the narrow widths, with this family's stack tuple (the weight itself
    in place of the packed images): forward, data gradient (both inputs for the comb pair) and weight / bias gradients
    accumulated into the arena against an fp64 composition of nn.Linear, ELU and the mix; inputs are strided views."""
    import torch.nn as nn
    ops = _ops()
    gen = torch.Generator().manual_seed(H + N)
    K = 2 * H if comb else H
    act = 0 if comb else 1
    zr = 0.85
    W = torch.randn(2 * H, K, generator=gen) / K**0.5
    b = torch.randn(2 * H, generator=gen) * 0.1
    wide_a, wide_b = torch.randn(N, H + 4, generator=gen), torch.randn(N, 2 * H, generator=gen)
    mask = torch.rand(N, generator=gen) < 0.3
    gout = torch.randn(N, H, generator=gen)
    # fp64 reference
    xa64 = wide_a[:, :H].double().requires_grad_(True)
    xb64 = wide_b[:, H:].double().requires_grad_(True)
    W64, b64 = W.double().requires_grad_(True), b.double().requires_grad_(True)
    xin = torch.cat((xa64, xb64), -1) if comb else xa64
    Zt = xin @ W64.t() + b64
    A = torch.nn.functional.elu(Zt) if act else Zt
    ref = O._mix(mask.reshape(-1, 1), zr, A[:, :H], A[:, H:])
    ref.backward(gout.double())
    # HIP
    Wg, bg = W.to(DEV), b.to(DEV)
    dW, db = torch.zeros_like(Wg), torch.zeros_like(bg)
    lin1, lin0 = nn.Linear(K, H).to(DEV), nn.Linear(K, H).to(DEV)  # carriers for the autograd edges only
    lin1.weight.grad, lin0.weight.grad, lin1.bias.grad, lin0.bias.grad = dW[:H], dW[H:], db[:H], db[H:]
    xa = wide_a.to(DEV)[:, :H].requires_grad_(True)
    xb = wide_b.to(DEV)[:, H:].requires_grad_(True) if comb else None
    out = ops.dual_linear_mix(xa, xb, lin1, lin0, mask.to(DEV).to(torch.uint8), zr, act, (Wg, bg, dW, db, Wg, Wg))
    out.backward(gout.to(DEV))
    assert rel_inf(out.detach().cpu(), ref.detach()) < TOL
    assert rel_inf(xa.grad.cpu(), xa64.grad) < TOL
    if comb:
        assert rel_inf(xb.grad.cpu(), xb64.grad) < TOL
    assert rel_inf(dW.cpu(), W64.grad) < TOL
    assert rel_inf(db.cpu(), b64.grad) < TOL
    out2 = ops.dual_linear_mix(xa.detach(), None if xb is None else xb.detach(), lin1, lin0,
                               mask.to(DEV).to(torch.uint8), zr, act, (Wg, bg, dW, db, Wg, Wg))
    assert torch.equal(out2, out.detach())
    record_parity(f"kernel/narrow_dual_linear_mix_{_pair(comb)}_H{H}_N{N}", out_rel_inf=rel_inf(out.detach().cpu(), ref.detach()),
                  dW_rel_inf=rel_inf(dW.cpu(), W64.grad), db_rel_inf=rel_inf(db.cpu(), b64.grad))
