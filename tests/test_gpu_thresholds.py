"""The step program on both sides of every row-count dispatch threshold, against the fp64 oracle.

The step program picks its kernels by row count N and hidden width H; several choices flip at a fixed N (_limits reads
them from the code).  CASES holds, for each threshold, the last row count on one side and the first on the other.  Every case runs
ParamArena + stack.loss_and_grads once under the profiler and checks, from the launched kernel names and the program's own
state, that it took the branch the code says; then logits, loss and the flat gradient against the fp64 oracle at the plain
bar.  test_threshold_table_straddles_the_code (no GPU) re-reads the limits from the sources, so a moved threshold fails
until the cases move with it.  test_step_switch_vs_oracle runs every Python A/B switch that acts inside a training pass
in its non-default position at the shapes where the size-selected kernels run."""
import importlib
import os
import re

import pytest
import torch

from helpers import rel_inf, flat_grads, build_glass, record_parity, STEP_SWITCHES
from oracle import glass_oracle as O

TOL = 1e-5
DEV = "cuda:0"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "glass_amd", "csrc")

# (H, L, N): the last row count of one branch and the first of the other, for each threshold (comparisons as in the code)
CASES = [
    (64, 2, 100_000), (64, 2, 100_001),        # kFusedBwdMaxRows: N <= 100 000 -> data + weight gradient of a pair in one launch
    (64, 2, 262_144), (64, 2, 262_145),        # stack.GN_EXACT_MAX_ROWS: N <= 2^18 -> exact GraphNorm accumulators
    (128, 1, 8_191), (128, 1, 8_192),          # wgrad128_shape: N >= 8 192
    (128, 1, 16_384), (128, 1, 16_385),        # stack.GN_EXACT_FWD_ONLY_MAX_ROWS: N <= 2^14 -> exact forward sums alone
    (128, 1, 65_536), (128, 1, 65_537),        # stack.GN_EXACT_READOUT_MAX_ROWS: N <= 2^16 -> readout sums exact (H * L <= 128)
    (128, 1, 400_000), (128, 1, 400_001),      # wgrad128_shape: N <= 4 * kFusedBwdMaxRows
    (128, 2, 100_000), (128, 2, 100_001),      # kFusedBwdMaxRows at hidden 128: slab geometry of the weight gradients
    (256, 1, 65_535), (256, 1, 65_536),        # wgrad_tiled_shape: N >= 65 536 -> LDS-tiled weight gradient
]
# per hidden width: the case above its highest threshold (dropout case; repeatability)
LARGEST = {H: max(N for h, _l, N in CASES if h == H) for H in (64, 128, 256)}
# model per width: C2's (mean / sum), C4's (gcn / size), C5's (mean / sum)
MODEL = {64: ("mean", "sum", 0.95), 128: ("gcn", "size", 0.75), 256: ("mean", "sum", 0.9)}
K, B, S = 6, 16, 20   # classes, subgraphs, nodes per subgraph


def _csrc(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _limits():
    """Every row-count threshold the cases must straddle, read from the code: {name: (H, layers or None, last N of the
    lower branch)} — the lower branch runs up to and including that N, the other from N + 1."""
    from glass_amd import stack
    common = _csrc("wgrad_common.h")
    fused = int(re.search(r"constexpr\s+int64_t\s+kFusedBwdMaxRows\s*=\s*(\d+)\s*;", common).group(1))
    w128 = _csrc("wgrad128.hip")
    m = re.search(r"bool wgrad128_shape\(int64_t N, int64_t O, int64_t I\)\s*\{\s*return O == 256 && I == 128 && "
                  r"N >= (\d+) && N <= kFusedBwdMaxRows \* (\d+);", w128)
    assert m, "wgrad128_shape changed form: update the threshold table"
    m2 = re.search(r"bool wgrad128_comb_shape\(int64_t N, int64_t O, int64_t I\)\s*\{\s*return O == 256 && I == 256 && "
                   r"N >= (\d+) && N <= kFusedBwdMaxRows \* (\d+);", w128)
    assert m2 and m2.groups() == m.groups(), "wgrad128_comb_shape no longer has wgrad128_shape's rows: update the table"
    mt = re.search(r"bool wgrad_tiled_shape\(int64_t N, int64_t O, int64_t I\)\s*\{\s*return O >= 512 && [^;]*N >= (\d+);",
                   _csrc("wgrad_tiled.hip"))
    assert mt, "wgrad_tiled_shape changed form: update the threshold table"
    return {"kFusedBwdMaxRows (hidden 64)": (64, None, fused),
            "kFusedBwdMaxRows (hidden 128)": (128, 2, fused),
            "GN_EXACT_MAX_ROWS": (64, None, stack.GN_EXACT_MAX_ROWS),
            "wgrad128_shape lower": (128, None, int(m.group(1)) - 1),
            "wgrad128_shape upper": (128, None, fused * int(m.group(2))),
            "GN_EXACT_FWD_ONLY_MAX_ROWS": (128, 1, stack.GN_EXACT_FWD_ONLY_MAX_ROWS),
            "GN_EXACT_READOUT_MAX_ROWS": (128, 1, stack.GN_EXACT_READOUT_MAX_ROWS),
            "wgrad_tiled_shape": (256, None, int(mt.group(1)) - 1)}


def test_threshold_table_straddles_the_code():
    """CPU: each threshold read from the sources (stack.py constants; kFusedBwdMaxRows, wgrad128_shape, wgrad_tiled_shape
    by regex) has a case at its last row count and one at the next."""
    for name, (H, L, last) in _limits().items():
        Ns = {N for h, l, N in CASES if h == H and (L is None or l == L)}
        assert last in Ns and last + 1 in Ns, f"{name}: no cases at N = {last} / {last + 1} (hidden {H}, layers {L})"


def _expected(H, L, N, jk=True):
    """What the code selects at (H, L, N): kernel-name substrings that must appear / must not, and the program's state."""
    from glass_amd import stack
    lim = _limits()
    fused = lim["kFusedBwdMaxRows (hidden 64)"][2]
    present, absent = [], []
    if H == 64:
        (present if N <= fused else absent).extend(["dual_bwd_kernel", "comb_bwd_eff_kernel"])
        if N > fused:
            present.append("comb_dgrad_eff_kernel")
    if H == 128:
        lo, hi = lim["wgrad128_shape lower"][2] + 1, lim["wgrad128_shape upper"][2]
        (present if lo <= N <= hi else absent).extend(["wgrad128_trans_kernel", "wgrad128_comb_kernel"])
    if H == 256:
        (present if N > lim["wgrad_tiled_shape"][2] else absent).append("tiled_wgrad")
    exact_all = H == 64 and N <= stack.GN_EXACT_MAX_ROWS
    fwd_only = H == 128 and L == 1 and N <= stack.GN_EXACT_FWD_ONLY_MAX_ROWS
    state = {"gn_exact": exact_all, "fwd_exact": exact_all or fwd_only,
             "gn_exact_readout": exact_all or fwd_only or ((H * L if jk else H) <= 128 and N <= stack.GN_EXACT_READOUT_MAX_ROWS)}
    return present, absent, state


def _data(N, seed):
    """Power-law graph with mean degree 8 (hub rows take K1's long-row kernels), use_deg features, B subgraphs of S nodes."""
    from glass_amd import synth
    ei, ew = synth.make_graph(N, 4 * N, seed, 0.7)
    x = synth.degree_feature(ei, N)
    pos, y = synth.make_subgraphs(N, B, S, K, seed + 1)
    return tuple(torch.from_numpy(a) for a in (ei, ew, x, pos, y))


def _model(H, L, x, dropout=0.0):
    aggr, pool, zr = MODEL[H]
    torch.manual_seed(0)
    model = build_glass(H, L, int(x.max()), K, aggr, pool, zr, dropout=dropout)
    return model, {k: v.clone() for k, v in model.state_dict().items()}


def _oracle(H, L, sd, data, dropout=0.0, masks=None):
    """fp64 oracle: (logits, loss, {name: grad}); masks: the kernels' own dropout keep-scales, in the oracle's call order."""
    from glass_amd import losses
    ei, ew, x, pos, y = data
    aggr, pool, zr = MODEL[H]
    orc = O.OracleGLASS(H, L, int(x.max()), K, aggr=aggr, pool=pool, z_ratio=zr, dropout=dropout)
    orc.load_state_dict(sd)
    orc = orc.double().train()
    O.mask_feed(masks or [])
    try:
        po = orc(x, ei, ew.double(), pos, O.max_zero_one(x, pos))
        assert not O._MASK_FEED  # every fed mask was consumed, in order
    finally:
        O.mask_feed([])
    lo = losses.CrossEntropy()(po, y)
    lo.backward()
    return po.detach(), lo.item(), {k: p.grad for k, p in orc.named_parameters()}


def _spy_state(monkeypatch):
    """Record, for each StackProgram.forward, which exact-accumulator forms the program chose (Python-side predicates)."""
    from glass_amd import stack
    seen = {"fwd_exact": False}
    orig, orig_exact = stack.StackProgram.forward, stack._GN.stats_exact

    def forward(self, *a, **kw):
        out, st = orig(self, *a, **kw)
        if st is not None:
            seen.update(gn_exact=st.get("gn_exact") is not None, gn_exact_readout=st.get("gn_exact_readout") is not None)
        return out, st

    def stats_exact(self, *a, **kw):  # conv.gn's forward sums go to the exact accumulators
        seen["fwd_exact"] = True
        return orig_exact(self, *a, **kw)
    monkeypatch.setattr(stack.StackProgram, "forward", forward)
    monkeypatch.setattr(stack._GN, "stats_exact", stats_exact)
    return seen


def _compare(tag, model, logits, loss, ref, **extra):
    po, lo, theirs = ref
    mine = {k: p.grad.cpu() for k, p in model.named_parameters()}
    keys = sorted(mine)
    assert keys == sorted(theirs)
    e_pred, e_loss = rel_inf(logits.cpu(), po), abs(loss.item() - lo) / abs(lo)
    e_grad = rel_inf(flat_grads(mine, keys), flat_grads(theirs, keys))
    print(f"{tag}: logits {e_pred:.2e} loss {e_loss:.2e} grad {e_grad:.2e}")
    record_parity(tag, logits_rel_inf=e_pred, loss_rel=e_loss, grad_rel_inf=e_grad, **extra)
    assert e_pred < TOL and e_loss < TOL and e_grad < TOL, (tag, e_pred, e_loss, e_grad)


@pytest.mark.gpu
@pytest.mark.parametrize("H,L,N", CASES, ids=[f"H{h}_L{l}_N{n}" for h, l, n in CASES])
def test_step_program_at_threshold_vs_oracle(H, L, N, monkeypatch):
    """One case of the table: the step (overwrite mode over a garbage-filled arena, dropout 0) under the profiler — the kernel
    names and the program's exact-accumulator choices are those of this side of the threshold — against the fp64 oracle; at
    the largest N of each width, a second step gives the same gradient bits."""
    from torch.profiler import profile, ProfilerActivity
    from glass_amd import stack, losses
    from glass_amd.arena import ParamArena
    data = _data(N, N % 97)
    ei, ew, x, pos, y = data
    model, sd = _model(H, L, x)
    loss_fn = losses.CrossEntropy()
    model.to(DEV).train()
    arena = ParamArena(model)
    assert stack.step_supported(model, loss_fn) and stack.covers_arena(model, arena)
    seen = _spy_state(monkeypatch)
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in data[2:3] + data[:2] + data[3:])
    arena.flat.fill_(3.0)  # overwrite mode: stale contents must not survive
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        loss, logits = stack.loss_and_grads(model, loss_fn, xg, eig, ewg, posg, "pos", yg, overwrite=True)
        torch.cuda.synchronize()
    names = {e.name for e in prof.events()}
    kernels = sorted(n for n in names if "_kernel" in n)
    assert kernels, f"the profiler reported no HIP kernel of the step (events: {sorted(names)[:20]})"
    present, absent, state = _expected(H, L, N, model.conv.jk)
    for k in present:
        assert any(k in n for n in kernels), f"H{H} L{L} N{N}: no '{k}' launch; kernels: {kernels}"
    for k in absent:
        assert not any(k in n for n in kernels), f"H{H} L{L} N{N}: '{k}' launched; kernels: {kernels}"
    assert seen == state, f"H{H} L{L} N{N}: program state {seen}, the code says {state}"
    first = arena.flat.clone()
    if N == LARGEST[H]:
        arena.flat.fill_(3.0)  # (slots between parameters are never written)
        loss2, _ = stack.loss_and_grads(model, loss_fn, xg, eig, ewg, posg, "pos", yg, overwrite=True)
        assert torch.equal(first, arena.flat) and torch.equal(loss, loss2), "two steps on the same input differ"
    _compare(f"threshold/H{H}_L{L}_N{N}", model, logits, loss, _oracle(H, L, sd, data), n_node=N, nnz=ei.shape[1])


@pytest.mark.gpu
@pytest.mark.parametrize("H", sorted(LARGEST))
def test_step_program_dropout_above_thresholds_vs_oracle(H):
    """Dropout 0.5 at each width's largest case against the fp64 oracle given the kernels' own keep-scales
    (glass_dropout_scales_f32 + O.mask_feed, as in the benchmarked dropout test)."""
    from glass_amd import stack, losses, ops, _lib
    from glass_amd.arena import ParamArena
    N, L = LARGEST[H], max(l for h, l, n in CASES if h == H and n == LARGEST[H])
    data = _data(N, N % 97)
    ei, ew, x, pos, y = data
    model, sd = _model(H, L, x, dropout=0.5)
    loss_fn = losses.CrossEntropy()
    model.to(DEV).train()
    arena = ParamArena(model)
    assert stack.step_supported(model, loss_fn) and stack.covers_arena(model, arena)
    xg, eig, ewg, posg, yg = (t.to(DEV) for t in data[2:3] + data[:2] + data[3:])
    ops.rng_seed(2024, DEV)
    loss, logits = stack.loss_and_grads(model, loss_fn, xg, eig, ewg, posg, "pos", yg, overwrite=True)
    # the pass's masks in the oracle's call order: emb_gn's (call id 1), per layer conv.gn's (16 (l+1)) and between layers gns[l]'s
    ids = [1]
    for l in range(L):
        ids.append(16 * (l + 1))
        if l + 1 < L:
            ids.append(16 * (l + 1) + 1)
    feed = []
    for cid in ids:
        m = torch.empty(N, H, device=DEV)
        _lib.check(_lib.load().glass_dropout_scales_f32(ops.rng_state(DEV).data_ptr(), cid, 0.5, N, H, m.data_ptr(),
                                                        torch.cuda.current_stream().cuda_stream), "glass_dropout_scales_f32")
        feed.append(m.cpu())
        assert abs(float((feed[-1] > 0).double().mean()) - 0.5) < 0.01
    _compare(f"threshold_dropout/H{H}_L{L}_N{N}", model, logits, loss, _oracle(H, L, sd, data, 0.5, feed))


# ------------------------------------------------------------------ the A/B switches at the sizes where they choose kernels
_SHAPES = {"c2": (64, 2, 17_080), "c4": (128, 1, 50_000), "h256": (256, 1, 70_001)}
_TILED_SWITCHES = {("glass_amd.models", "USE_STACK"), ("glass_amd.ops", "USE_FUSED_DENSE"), ("glass_amd.ops", "DENSE_F32_PRODUCTS"),
                   ("glass_amd.ops", "_DENSE_OFF"), ("glass_amd.stack", "USE_FUSED_BWD")}
_SW_CASES = [(shape, m, n, v) for shape in _SHAPES for m, n, v in STEP_SWITCHES
             if shape != "h256" or ((m, n) in _TILED_SWITCHES and v != {128})]
_REF = {}


def _shape_ref(shape):
    """(data, state dict, fp64 oracle) of one shape: C2's and C4's workloads themselves, and a hidden-256 power-law graph just
    above the tiled weight gradient's threshold — computed once per module."""
    if shape not in _REF:
        from glass_amd import synth
        H, L, N = _SHAPES[shape]
        if shape == "h256":
            data = _data(N, 3)
            (aggr, pool, zr), n_class = MODEL[256], K
        else:
            w, ei, ew, x, pos, y = synth.make_workload({"c2": "ppi_bp", "c4": "em_user"}[shape], seed=0, n_batches=1)
            assert (w.hidden, w.layers, w.n_node) == (H, L, N)
            data = tuple(torch.from_numpy(a) for a in (ei, ew, x, pos, y))
            aggr, pool, zr, n_class = w.aggr, w.pool, w.z_ratio, w.n_class
        torch.manual_seed(0)
        model = build_glass(H, L, int(data[2].max()), n_class, aggr, pool, zr)
        sd = {k: v.clone() for k, v in model.state_dict().items()}
        orc = O.OracleGLASS(H, L, int(data[2].max()), n_class, aggr=aggr, pool=pool, z_ratio=zr)
        orc.load_state_dict(sd)
        orc = orc.double().train()
        ei, ew, x, pos, y = data
        po = orc(x, ei, ew.double(), pos, O.max_zero_one(x, pos))
        from glass_amd import losses
        lo = losses.CrossEntropy()(po, y)
        lo.backward()
        _REF[shape] = (data, sd, (aggr, pool, zr, n_class), (po.detach(), lo.item(), {k: p.grad for k, p in orc.named_parameters()}))
    return _REF[shape]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,module,name,value", _SW_CASES,
                         ids=[f"{s}-{m.split('.')[-1]}.{n}" + (f"{sorted(v)[0]}" if isinstance(v, set) else "") for s, m, n, v in _SW_CASES])
def test_step_switch_vs_oracle(shape, module, name, value, monkeypatch):
    """One Python A/B switch in its non-default position (set before the model and its arena exist: the arena's packs depend
    on some), one training pass through whatever the product then selects — the step program when it still applies, else the
    per-op forward and autograd backward — against the shape's fp64 oracle at the plain bar."""
    from glass_amd import stack, losses
    from glass_amd.arena import ParamArena
    from impl import utils
    monkeypatch.setattr(importlib.import_module(module), name, value)
    data, sd, (aggr, pool, zr, n_class), ref = _shape_ref(shape)
    H, L, N = _SHAPES[shape]
    model = build_glass(H, L, int(data[2].max()), n_class, aggr, pool, zr)
    model.load_state_dict(sd)
    model.to(DEV).train()
    arena = ParamArena(model)
    loss_fn = losses.CrossEntropy()
    ei, ew, x, pos, y = (t.to(DEV) for t in data)
    program = stack.step_supported(model, loss_fn)
    if program:
        if not stack.covers_arena(model, arena):
            arena.zero()
        loss, logits = stack.loss_and_grads(model, loss_fn, x, ei, ew, pos, "pos", y, overwrite=stack.covers_arena(model, arena))
    else:
        arena.zero()
        logits = model(x, ei, ew, pos, utils.MaxZOZ(x, pos))
        loss = loss_fn(logits, y)
        loss.backward()
        logits = logits.detach()
    torch.cuda.synchronize()
    tag = f"switch/{shape}/{module.split('.')[-1]}.{name}" + (f"{sorted(value)[0]}" if isinstance(value, set) else "")
    _compare(tag, model, logits, loss, ref, step_program=bool(program))
