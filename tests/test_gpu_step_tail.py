"""Kernel-level value tests of the last three launches of a captured training step, through the C ABI:

  1. glass_linear_wgrad_reduce_batch_f32 — the deferred, batched reduction of the weight-gradient partials (linear.hip:
     reduce_batch_impl), every job kind, batches of 1 / 8 / 9 / 17 jobs, mixed kinds, mixed accumulate, strided destinations;
  2. glass_wgrad_reduce_spmm_f32 (+ glass_spmm_reduce_rows_f32) — the same reduction carrying the selection product
     G = S^T dh (wgrad_reduce_sel_kernel<16|32|64>), and its two-call fallback;
  3. glass_embed_norm_bwd_adam_f32 (embnorm.hip: emb_tail_kernel) — partial-row sums, table-form GraphNorm backward and Adam
     over a hand-built arena.

References are fp64 on the CPU (tests/step_tail_oracle.py); gradients are graded PER TENSOR (rel-inf < 1e-5, the TOL of
tests/test_gpu_kernels.py); every output buffer sits between guard floats that must come back bit-identical."""
import itertools

import numpy as np
import pytest
import torch

import gradclip_oracle as GO
import step_tail_oracle as TO
from helpers import rel_inf

pytestmark = pytest.mark.gpu
TOL = 1e-5
DEV = "cuda:0"
GUARD = 64  # floats: 256 bytes, so the guarded view keeps the buffer's alignment
NAN = float("nan")


def _lib():
    from glass_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int32)


class Guarded:
    """`n` floats filled with `fill`, GUARD sentinel floats in front and behind"""
    def __init__(self, n, fill, dtype=torch.float32):
        self.buf = torch.empty(n + 2 * GUARD, dtype=dtype, device=DEV)
        self.sentinel = (torch.arange(2 * GUARD, device=DEV) * 0.375 - 11.0).to(dtype)
        self.buf[:GUARD] = self.sentinel[:GUARD]
        self.buf[GUARD + n:] = self.sentinel[GUARD:]
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        n = self.t.numel()
        return torch.equal(self.buf[:GUARD], self.sentinel[:GUARD]) and torch.equal(self.buf[GUARD + n:], self.sentinel[GUARD:])


# =============================================================================================== 1. batched deferred reduce
def _synth_ref(dsrc, T, mask, zr, act, X, X2):
    """fp64: G[n, o] = coef(mask[n], o < H) * dsrc[n, o mod H] * act'(T[n, o]);  dW = G^T [X | X2],  db = column sums of G
    (the reference of the weight-gradient tests of tests/test_gpu_kernels.py)"""
    c1 = torch.where(mask, zr, 1 - zr).double().reshape(-1, 1)
    G = torch.cat((c1 * dsrc.double(), (1 - c1) * dsrc.double()), 1)
    if act == 1:
        G = G * torch.where(T > 0, torch.ones(()), torch.exp(T)).double()
    elif act == 2:
        G = G * (T > 0).double()
    Xin = torch.cat((X, X2), 1).double() if X2 is not None else X.double()
    return G.t() @ Xin, G.sum(0)


def _plain_job(name, N, H, comb, act, seed):
    """Partials of glass_dual_linear_wgrad_f32 with dW = 0 (as stack._dual_wgrad calls it), and the result of the same call
    with dW given (its own reduce launch) for the bitwise comparison."""
    from glass_amd import ops
    L, lib = _lib()
    gen = torch.Generator().manual_seed(seed)
    zr = 0.8
    dsrc = torch.randn(N, H, generator=gen)
    T = torch.randn(N, 2 * H, generator=gen) if act else None
    X = torch.randn(N, H, generator=gen)
    X2 = torch.randn(N, H, generator=gen) if comb else None
    mask = torch.rand(N, generator=gen) < 0.05
    mask[-1] = True
    dW_ref, db_ref = _synth_ref(dsrc, T, mask, zr, act, X, X2)
    dg, Xg, mg = dsrc.to(DEV), X.to(DEV), mask.to(DEV).to(torch.uint8)
    Tg = T.to(DEV) if act else None
    X2g = X2.to(DEV) if comb else None
    O, I = 2 * H, (2 * H if comb else H)
    n_ws = lib.glass_linear_wgrad_ws_bytes(N, O, I) // 4 + 16
    ws, ws2 = torch.zeros(n_ws, device=DEV), torch.zeros(n_ws, device=DEV)
    dW, db = torch.full((O, I), NAN, device=DEV), torch.full((O, ), NAN, device=DEV)

    def call(dWp, ld, dbp, wsp):
        L.check(lib.glass_dual_linear_wgrad_f32(dg.data_ptr(), dg.stride(0), Tg.data_ptr() if act else 0, Tg.stride(0) if act else 0,
                                                mg.data_ptr(), zr, ops.act_word(act), Xg.data_ptr(), Xg.stride(0),
                                                X2g.data_ptr() if comb else 0, X2g.stride(0) if comb else 0, N, H, dWp, ld, dbp,
                                                0 if dWp else 1, wsp, _stream()), "glass_dual_linear_wgrad_f32")
    call(0, 0, 0, ws.data_ptr())
    call(dW.data_ptr(), dW.stride(0), db.data_ptr(), ws2.data_ptr())
    torch.cuda.synchronize()
    return {"name": name, "ws": ws, "N": N, "O": O, "I": I, "cap": 0, "dW_ref": dW_ref, "db_ref": db_ref,
            "dW_direct": dW.cpu(), "db_direct": db.cpu()}


def _sl_job():
    """S / L partials of glass_comb_eff_bwd_f32 (comb pair at hidden 64, lab_cap > 0), driven as
    test_comb_pair_effective_weight_hidden64 of tests/test_gpu_kernels.py drives it."""
    from glass_amd import stack, ops
    from glass_amd.arena import ParamArena
    from glass_amd.factory import build_glass
    torch.manual_seed(11)
    H, z, N = 64, 0.95, 1000
    model = build_glass(H, 1, 5, 3, "mean", "sum", z).to(DEV).train()
    arena = ParamArena(model)
    conv = model.conv.convs[0]
    # every row of one 16-row wave tile and of one 64-row workgroup tile, and a few single rows
    pos = np.concatenate([np.arange(32, 48), np.arange(640, 704), [3, 517, 999, 998, 3, -1, -1, -1, -1, -1]]).reshape(9, 10)
    pos_t = torch.from_numpy(pos.astype(np.int64)).to(DEV)
    labels = stack.BatchLabels(N, pos_t.numel(), DEV)
    labels.load(pos_t)
    mask = labels.mask
    ops.rng_seed(99, DEV)
    arena.refresh_transposes(ops.rng_state(DEV))
    a, h = torch.randn(N, H, device=DEV) * 2 + 0.5, torch.randn(N, H, device=DEV)
    gmod = conv.gn
    with torch.no_grad():
        gmod.weight.uniform_(0.5, 1.5)
        gmod.bias.uniform_(-0.3, 0.3)
        gmod.mean_scale.uniform_(0.7, 1.1)
    gsaved = stack._GN(gmod).stats(a)
    lib = stack._lib.load()
    c, g = torch.empty(N, H, device=DEV), torch.empty(N, H, device=DEV)
    cstat = torch.empty(int(lib.glass_comb_eff_fwd_blocks(N, H, labels.cap)), 2, H, dtype=torch.float64, device=DEV)
    stack._comb_eff_fwd(a, h, conv, mask, c, cstat, (gsaved, 0, 0.0, 16, g), labels)  # g = the normalised operand
    dc = torch.randn(N, H, device=DEV)
    din = torch.empty(N, 2 * H, device=DEV)
    gpart = torch.empty(int(lib.glass_comb_eff_blocks(N, H, labels.cap)), 2, H, dtype=torch.float64, device=DEV)
    pending = []
    stack._comb_eff_bwd(dc, conv, mask, din, g, h, pending, 0, (gpart, a, gsaved, gmod.mean_scale, 0, 0.0, 16), labels)
    torch.cuda.synchronize()
    ws_ptr, n, O, I, _dW, _ld, _db, _acc, cap = pending[0]
    assert (n, O, I, cap) == (N, 128, 128, 90)
    live = [w for w in ops._wgrad_ws.values() if w.data_ptr() == ws_ptr]
    assert len(live) == 1
    ws = live[0].clone()  # (the cached scratch buffer belongs to the step program)
    lab = mask.bool().cpu().unsqueeze(1)
    w1 = torch.where(lab, torch.tensor(z, dtype=torch.float64), torch.tensor(1 - z, dtype=torch.float64))
    dZ = torch.cat([w1 * dc.cpu().double(), (1 - w1) * dc.cpu().double()], 1)
    x = torch.cat([g, h], 1).cpu().double()
    return {"name": "sl64", "ws": ws, "N": N, "O": O, "I": I, "cap": cap, "dW_ref": dZ.t() @ x, "db_ref": dZ.sum(0)}


KINDS = ["trans64", "comb128", "sl64", "w128", "narrow", "tiled"]


@pytest.fixture(scope="module")
def jobs():
    """The partials of every job kind, produced once by the product's own kernels and left unchanged.
    trans64  plain, trans pair, H = 64, N = 3001 (ELU)        comb128  plain, comb pair, H = 128, N = 3001: 8 chunks
    w128     plain, H = 128, N = 8192: the wgrad128 route      sl64     S / L form of glass_comb_eff_bwd_f32, lab_cap = 90
    narrow   hidden 20 (dense_narrow.hip), N = 3001             tiled    N = 65536 + 17, H = 256: its own reduce launch"""
    from glass_amd import ops
    out = {"trans64": _plain_job("trans64", 3001, 64, False, 1, 1), "comb128": _plain_job("comb128", 3001, 128, True, 0, 2),
           "w128": _plain_job("w128", 8192, 128, False, 1, 3), "narrow": _plain_job("narrow", 3001, 20, False, 1, 4),
           "tiled": _plain_job("tiled", 65536 + 17, 256, False, 0, 5)}
    # the S / L producer seeds torch and the process-wide dropout stream (and its pack launch advances that stream): both are
    # put back, so that whatever runs after this module in the same process starts from the state it would have found
    words = ops.rng_state(DEV).clone()
    with torch.random.fork_rng(devices=[0]):
        out["sl64"] = _sl_job()
    ops.rng_state(DEV).copy_(words)
    torch.cuda.synchronize()
    return out


class Dest:
    """Guarded dW [O, ld] (ld > I: a strided view inside a wider buffer) and db [O]; accumulate: both pre-filled with 0.5 (as
    the table-path test does), else with NaN."""
    def __init__(self, job, accumulate, pad):
        self.job, self.acc, self.ld = job, int(accumulate), job["I"] + pad
        self.fill = 0.5 if accumulate else NAN
        self.dW, self.db = Guarded(job["O"] * self.ld, self.fill), Guarded(job["O"], self.fill)

    def check(self, tag, bitwise=True):
        j = self.job
        dW = self.dW.t.view(j["O"], self.ld).cpu()
        db = self.db.t.cpu()
        got_w, got_b = dW[:, :j["I"]], db
        off = 0.5 if self.acc else 0.0
        e_w, e_b = rel_inf(got_w - off, j["dW_ref"]), rel_inf(got_b - off, j["db_ref"])
        assert e_w < TOL and e_b < TOL, (tag, j["name"], self.acc, self.ld, e_w, e_b)
        assert self.dW.intact() and self.db.intact(), (tag, j["name"], "guard floats")
        pad = dW[:, j["I"]:]
        assert torch.equal(_bits(pad), _bits(torch.full_like(pad, self.fill))), (tag, j["name"], "columns beyond I")
        if bitwise and "dW_direct" in j:
            # wgrad_reduce_kernel (the call with dW given) and wgrad_reduce_batch_kernel run the same wgrad_reduce_body on the same
            # partials with the same geometry, the tiled and narrow forms the same reduce launch either way: identical bits,
            # and accumulate adds the same fp32 sum to 0.5.  (The S / L form has no call with dW given.)
            want_w = j["dW_direct"] + 0.5 if self.acc else j["dW_direct"]
            want_b = j["db_direct"] + 0.5 if self.acc else j["db_direct"]
            assert torch.equal(_bits(got_w), _bits(want_w)) and torch.equal(_bits(got_b), _bits(want_b)), (tag, j["name"], "bits")
        return e_w, e_b


def _job_arrays(dests):
    u64 = lambda v: np.array(v, dtype=np.uint64)
    i64 = lambda v: np.array(v, dtype=np.int64)
    arrs = (u64([d.job["ws"].data_ptr() for d in dests]), i64([d.job["N"] for d in dests]), i64([d.job["O"] for d in dests]),
            i64([d.job["I"] for d in dests]), u64([d.dW.t.data_ptr() for d in dests]), i64([d.ld for d in dests]),
            u64([d.db.t.data_ptr() for d in dests]), np.array([d.acc for d in dests], dtype=np.int32), i64([d.job["cap"] for d in dests]))
    return arrs


def _make_dests(jobs, names):
    """accumulate alternates along the batch, every third destination is strided (lddw = I + 4)"""
    return [Dest(jobs[n], k % 2, 4 if k % 3 == 2 else 0) for k, n in enumerate(names)]


def _reduce_batch(dests):
    L, lib = _lib()
    arrs = _job_arrays(dests)
    L.check(lib.glass_linear_wgrad_reduce_batch_f32(len(dests), *(a.ctypes.data for a in arrs), _stream()),
            "glass_linear_wgrad_reduce_batch_f32")
    torch.cuda.synchronize()


def _cycle(n, start):
    return list(itertools.islice(itertools.cycle(KINDS[start:] + KINDS[:start]), n))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("accumulate,pad", [(0, 0), (1, 4)])
def test_reduce_single_job(jobs, kind, accumulate, pad):
    d = Dest(jobs[kind], accumulate, pad)
    _reduce_batch([d])
    d.check("n_jobs=1")


@pytest.mark.parametrize("n_jobs,start", [(6, 0), (8, 1), (9, 0), (9, 3), (17, 2)])
def test_reduce_batches_of_mixed_kinds(jobs, n_jobs, start):
    """6: every kind once in one launch — max_chunks comes from comb128 (8 chunks) while the blocks of the other jobs return early,
    the tiled job leaves an empty slot; 8 = kMaxReduceJobs: exactly one launch; 9: a second launch of one job (a tiled job as
    the ninth: no second launch at all); 17: three launches.  accumulate 0 / 1 and strided destinations mixed in every batch."""
    names = _cycle(n_jobs, start)
    dests = _make_dests(jobs, names)
    _reduce_batch(dests)
    for k, d in enumerate(dests):
        d.check(f"n_jobs={n_jobs} job {k}")


# =============================================================================================== 2. reduce + selection product
_SEL = {}


def _selection(name):
    from glass_amd.graph import Selection
    if name not in _SEL:
        x, V = TO.index_vector(name)
        sel = Selection(x.to(DEV), V)
        hdr = sel.op.header
        sweep, cut = TO.PLAN_KIND[name]
        # the case is what it claims to be: header words 4 = sweep items, 5 = workgroup items, 6 = reduce rows, 7 = slots
        assert (hdr[4] > 0) == sweep and (hdr[6] > 0) == cut and (hdr[7] > 0) == cut and (hdr[5] > 0 or not cut), (name, hdr)
        if not sweep:
            assert hdr[5] >= V
        assert sel._hdr_noreduce[6] == 0 and sel._n_reduce == hdr[6]
        _SEL[name] = (x, V, sel, sel.op.plan.cpu().numpy())
    return _SEL[name]


def _strided(X, wide):
    """X on the device; wide: as a column slice of a wider matrix (ldx = H + 8, 16-byte aligned columns)"""
    if not wide:
        return X.to(DEV)
    big = torch.full((X.shape[0], X.shape[1] + 8), 3.0, device=DEV)
    big[:, 4:4 + X.shape[1]] = X.to(DEV)
    return big[:, 4:4 + X.shape[1]]


def _product(name, Xg, full, dests=()):
    """glass_wgrad_reduce_spmm_f32 on guarded G / partial-row buffers (NaN-filled); returns (G, P) as Guarded"""
    L, lib = _lib()
    x, V, sel, plan = _selection(name)
    op, H = sel.op, Xg.shape[1]
    G, P = Guarded(V * H, NAN), Guarded(max(int(op.header[7]) * H, 4), NAN)
    hdr = op.header if full else sel._hdr_noreduce
    arrs = _job_arrays(dests) if dests else ()  # (kept alive across the call)
    ptrs = [a.ctypes.data for a in arrs] if dests else [0] * 9
    L.check(lib.glass_wgrad_reduce_spmm_f32(len(dests), *ptrs, op.rowptr.data_ptr(), op.col.data_ptr(), op.val.data_ptr(),
                                            Xg.data_ptr(), Xg.stride(0), G.t.data_ptr(), H, V, H, hdr.ctypes.data,
                                            op.plan.data_ptr(), P.t.data_ptr(), _stream()), "glass_wgrad_reduce_spmm_f32")
    torch.cuda.synchronize()
    return G, P


def _check_product(name, G, P, X, full):
    x, V, sel, plan = _selection(name)
    H = X.shape[1]
    ref = TO.selection_product(x, X, V)
    got = G.t.view(V, H).cpu().clone()
    parts = P.t.cpu()
    if not full:
        # the cut rows of G are left to the consumer: untouched here, their value is the sum of the partial rows in slot order
        for row, first, n in TO.reduce_list(plan):
            assert bool(got[row].isnan().all()), (name, H, row)
            got[row] = parts[first * H:(first + n) * H].view(n, H).double().sum(0).float()
    e = rel_inf(got, ref)
    assert e < TOL, (name, H, full, e)
    unused = torch.bincount(x, minlength=V) == 0
    assert unused.any() and float(got[unused].abs().max()) == 0.0 and not bool(got.isnan().any())
    assert G.intact() and P.intact(), (name, H, "guard floats")
    return e


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("H", [4, 64, 68, 128, 132, 256, 260, 18])
@pytest.mark.parametrize("name", ["long_cut", "long_nocut", "sweep"])
def test_selection_product(name, H, full):
    """G against fp64 index_add.  long_cut / long_nocut are fusable (no sweep items): H = 4 .. 256 covers the three templates of
    wgrad_reduce_sel_kernel on both sides of 64 and 128; H = 260 (> 256) and H = 18 (not a multiple of 4) take the two-call
    fallback, as does every H of `sweep`.  full: the whole header, glass_spmm_reduce_rows_f32 completes G; else
    Selection._hdr_noreduce.  n_jobs = 0: the launch carries the product alone."""
    x, V, sel, plan = _selection(name)
    X = 8.0 * torch.randn(x.shape[0], H, generator=torch.Generator().manual_seed(H))
    G, P = _product(name, _strided(X, False), full)
    _check_product(name, G, P, X, full)


@pytest.mark.parametrize("name,H", [("long_cut", 64), ("long_cut", 132), ("long_nocut", 256), ("sweep", 64), ("long_cut", 18)])
def test_selection_product_strided_input(name, H):
    """ldx > H: X is a column slice of a wider matrix — the same bits as from the packed copy"""
    x, V, sel, plan = _selection(name)
    X = 8.0 * torch.randn(x.shape[0], H, generator=torch.Generator().manual_seed(H))
    Xw = _strided(X, True)
    assert Xw.stride(0) == H + 8
    for full in (True, False):
        G, P = _product(name, Xw, full)
        _check_product(name, G, P, X, full)
        G2, _P2 = _product(name, _strided(X, False), full)
        assert torch.equal(_bits(G.t), _bits(G2.t))


@pytest.mark.parametrize("name,H,full", [("long_cut", 64, False), ("long_cut", 128, True), ("sweep", 64, True), ("long_cut", 260, False)])
@pytest.mark.parametrize("n_jobs,start", [(1, 0), (1, 2), (9, 0), (9, 4)])
def test_reduce_carrying_the_product(jobs, name, H, full, n_jobs, start):
    """The jobs of part 1 in the launch that carries the product (9 jobs: the product rides with the first eight, the ninth gets
    a batch launch of its own): G as without jobs, every dW / db right — and bitwise what glass_linear_wgrad_reduce_batch_f32
    alone gives for the same partials and destinations.  (sweep, 64) and (long_cut, 260): the two-call fallback."""
    x, V, sel, plan = _selection(name)
    X = 8.0 * torch.randn(x.shape[0], H, generator=torch.Generator().manual_seed(H))
    names = _cycle(n_jobs, start)
    dests, alone = _make_dests(jobs, names), _make_dests(jobs, names)
    G, P = _product(name, _strided(X, False), full, dests)
    _check_product(name, G, P, X, full)
    _reduce_batch(alone)
    for k, (d, a) in enumerate(zip(dests, alone)):
        d.check(f"with product, job {k}")
        assert torch.equal(_bits(d.dW.t), _bits(a.dW.t)) and torch.equal(_bits(d.db.t), _bits(a.db.t)), (k, d.job["name"])


# =============================================================================================== 3. the tail launch
NO_OPT = (0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0)


def _saved(xg, V, sel, W, gamma, beta, alpha, H):
    """emb_gn's saved statistics [4H] from the forward launch (glass_embed_norm_fwd_f32) on aligned copies of the parameters"""
    L, lib = _lib()
    n = xg.shape[0]
    saved, table = torch.empty(4 * H, device=DEV), torch.empty(V, H, device=DEV)
    out, mask = torch.empty(n, H, device=DEV), torch.empty(n, dtype=torch.uint8, device=DEV)
    Wg, g, b, a = (t.to(DEV).contiguous() for t in (W, gamma, beta, alpha))
    zg = torch.zeros(n, dtype=torch.int64, device=DEV)
    L.check(lib.glass_embed_norm_fwd_f32(xg.data_ptr(), Wg.data_ptr(), V, sel.op.rowptr.data_ptr(), g.data_ptr(), b.data_ptr(),
                                         a.data_ptr(), TO.EPS, saved.data_ptr(), table.data_ptr(), zg.data_ptr(), 0, 0, 0.0, 0, 1,
                                         out.data_ptr(), H, mask.data_ptr(), n, H, _stream()), "glass_embed_norm_fwd_f32")
    return saved


def _tail(sel, G, P, V, H, W, gamma, alpha, saved, dW, acc_w, dg, db, da, acc, opt=NO_OPT):
    """glass_embed_norm_bwd_adam_f32 on the output of the no-reduce product (tensors or views; opt: the 15 optimizer arguments)"""
    L, lib = _lib()
    L.check(lib.glass_embed_norm_bwd_adam_f32(G.t.data_ptr(), W.data_ptr(), V, sel.op.rowptr.data_ptr(), gamma.data_ptr(),
                                              alpha.data_ptr(), saved.data_ptr(), dW.data_ptr(), acc_w, dg.data_ptr(),
                                              db.data_ptr(), da.data_ptr(), acc, H, P.t.data_ptr(),
                                              sel.op.plan.data_ptr() + 4 * sel._off_reduce, sel._n_reduce, *opt, _stream()),
            "glass_embed_norm_bwd_adam_f32")
    torch.cuda.synchronize()


TAIL_VECTORS = ["v1", "v3", "long_nocut", "long_cut", "v64c", "v65c", "v200", "sweep"]
TAIL_WIDTHS = [4, 16, 20, 64, 128]


@pytest.mark.parametrize("H", TAIL_WIDTHS)
@pytest.mark.parametrize("name", TAIL_VECTORS)
def test_tail_gradients_without_optimizer(name, H):
    """param = 0.  V = 1, 3, 8, 40, 64 take the register path (V <= 4 * 16 rows), V = 65, 200, 1024 the general one; cut rows
    (n_reduce > 0) at V = 40, 64 and at V = 65, 1024, none at the others; H = 4 / 20 leave 12 idle lanes in the last table
    workgroup; accumulate and accumulate_w take all four combinations along the cases.  dW, dgamma, dbeta, dalpha each against
    fp64 autograd of GraphNorm(Embedding(x)); unused rows exactly zero; the cut rows of G hold their sum afterwards."""
    x, V, W, gamma, beta, alpha, gout = TO.model_inputs(name, H)
    _x, _V, sel, plan = _selection(name)
    case = TAIL_VECTORS.index(name) * len(TAIL_WIDTHS) + TAIL_WIDTHS.index(H)
    acc_w, acc = case % 2, (case // 2 + case // 5) % 2
    assert (V <= 64) == (name in ("v1", "v3", "long_nocut", "long_cut", "v64c")) and (sel._n_reduce > 0) == TO.PLAN_KIND[name][1]
    ref = TO.autograd_grads(x, W, gamma, beta, alpha, gout)
    G, P = _product(name, gout.to(DEV), False)
    Wg, gg, ag = W.to(DEV), gamma.to(DEV), alpha.to(DEV)
    saved = _saved(x.to(DEV), V, sel, W, gamma, beta, alpha, H)
    dW = Guarded(V * H, 0.5 if acc_w else NAN)
    vecs = [Guarded(H, 0.25 if acc else NAN) for _ in range(3)]
    _tail(sel, G, P, V, H, Wg, gg, ag, saved, dW.t, acc_w, vecs[0].t, vecs[1].t, vecs[2].t, acc)
    got = [dW.t.view(V, H).cpu() - (0.5 if acc_w else 0.0)] + [v.t.cpu() - (0.25 if acc else 0.0) for v in vecs]
    errs = {k: rel_inf(g, r) for k, g, r in zip(("dW", "dgamma", "dbeta", "dalpha"), got, ref)}
    print(f"tail {name} H={H} acc_w={acc_w} acc={acc}: {errs}")
    assert all(e < TOL for e in errs.values()), errs
    unused = torch.bincount(x, minlength=V) == 0
    if unused.any():
        assert float(got[0][unused].abs().max()) == 0.0
    assert rel_inf(G.t.view(V, H).cpu(), TO.selection_product(x, gout, V)) < TOL  # cut rows included: the launch summed them
    assert all(b.intact() for b in [dW, G, P] + vecs)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("steps_done", [0, 5])
@pytest.mark.parametrize("layout,name,H", [("first", "long_cut", 64), ("middle", "v65c", 20), ("last", "long_nocut", 16),
                                           ("tight", "v3", 4), ("stride", "v200", 16)])
def test_tail_with_adam_over_the_arena(layout, name, H, steps_done, wd):
    """The arena built by hand: four guarded buffers (p, g, m, v), the table and emb_gn's vectors views at the offsets of
    step_tail_oracle.arena_layout (table at 0 / in the middle at an odd offset / ending at n_param; the vectors adjacent to the
    table and to each other, never in the order gamma, beta, alpha; `tight`: 29 elements, one rest workgroup; `stride`:
    2048 * 256 + 4099 elements, the table across the first stride's end).  Nonzero moments (tail_adam_state), lr through the
    device scalar.  The gradients left in the table / vector ranges per tensor against fp64 autograd; p, m, v of EVERY element
    within 2 ulp of gradclip_oracle.clipped_adam_step(coef = 1) applied to the gradient found in the arena (the bound and the
    oracle of test_clipped_adam_against_the_restatement) — an element updated twice, never, or from a stale weight is
    hundreds of ulp away; step_dev counts each launch once.
    Worst ulp per layout measured on MI355X (p / m / v; every run prints its own): first 2 / 1 / 1, middle 1 / 1 / 1,
    last 1 / 1 / 1, tight 1 / 1 / 1, stride 2 / 2 / 1 — the figures tests/test_step_tail_host.py finds between the separately
    rounded and the contracted form of the same update on the host."""
    x, V, W, gamma, beta, alpha, gout = TO.model_inputs(name, H)
    _x, _V, sel, plan = _selection(name)
    ref = dict(zip(("W", "gamma", "beta", "alpha"), TO.autograd_grads(x, W, gamma, beta, alpha, gout)))
    lay = TO.arena_layout(layout, V, H)
    n_param = lay[0]
    rng = TO.tail_ranges(lay, V, H)
    st = TO.tail_adam_state(lay, V, H, {"W": W, "gamma": gamma, "beta": beta, "alpha": alpha}, ref, seed=7)
    buf = {k: Guarded(n_param, 0.0) for k in "pgmv"}
    for k in "pgmv":
        buf[k].t.copy_(st[k])
    view = lambda k, r: buf[k].t[rng[r][0]:rng[r][1]]
    G, P = _product(name, gout.to(DEV), False)
    saved = _saved(x.to(DEV), V, sel, W, gamma, beta, alpha, H)
    lr = float(np.float32(1e-2))
    lr_dev = torch.tensor([lr], dtype=torch.float32, device=DEV)
    step_dev = torch.tensor([steps_done, 0], dtype=torch.int64, device=DEV)
    opt = (buf["p"].t.data_ptr(), buf["g"].t.data_ptr(), buf["m"].t.data_ptr(), buf["v"].t.data_ptr(), n_param, lr_dev.data_ptr(),
           0.9, 0.999, 1e-8, wd, step_dev.data_ptr(), lay[1], lay[2], lay[3], lay[4])
    args = (sel, G, P, V, H, view("p", "W"), view("p", "gamma"), view("p", "alpha"), saved, view("g", "W"), 0, view("g", "gamma"),
            view("g", "beta"), view("g", "alpha"), 0, opt)
    _tail(*args)
    after = {k: buf[k].t.cpu() for k in "pgmv"}
    # gradients: the launch's own ranges per tensor, everything else untouched
    errs = {k: rel_inf(after["g"][lo:hi], ref[k]) for k, (lo, hi) in rng.items()}
    assert all(e < TOL for e in errs.values()), errs
    outside = torch.ones(n_param, dtype=torch.bool)
    for lo, hi in rng.values():
        outside[lo:hi] = False
    assert torch.equal(_bits(after["g"][outside]), _bits(st["g"][outside])) and not bool(after["g"].isnan().any())
    unused = (torch.bincount(x, minlength=V) == 0).reshape(-1, 1).expand(V, H).reshape(-1)
    assert float(after["g"][rng["W"][0]:rng["W"][1]][unused].abs().max() if unused.any() else 0.0) == 0.0
    # every element of the arena against the restatement
    p, _gs, m, v = GO.clipped_adam_step(st["p"], after["g"], st["m"], st["v"], steps_done + 1, lr, 0.9, 0.999, 1e-8, wd, 1.0)
    worst = {k: TO.ulps(after[k], w) for k, w in (("p", p), ("m", m), ("v", v))}
    print(f"tail adam layout={layout} {name} H={H} t={steps_done} wd={wd}: worst ulp {worst}, gradients {errs}")
    assert max(worst.values()) <= 2.0, worst
    assert TO.ulps(st["p"], p) > 100  # (the comparison would see an element that was never updated)
    assert step_dev.tolist() == [steps_done + 1, 0]
    assert all(b.intact() for b in list(buf.values()) + [G, P])
    _tail(*args)
    assert step_dev.tolist() == [steps_done + 2, 0]
    assert all(b.intact() for b in list(buf.values()) + [G, P])
