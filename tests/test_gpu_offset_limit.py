"""The staged dense kernels on both sides of the 32-bit buffer-offset limit, against fp64.

Those kernels read and write their operands through buffer resources built on the whole tensor (make_rsrc in common.h:
a 32-bit record count and 32-bit byte offsets).  An access past the record count does not fault — a load returns 0, a
store is dropped — so a wrapped offset gives a silently wrong answer, never a crash.  Every such resource is therefore
behind a host-side guard `rows * ld * 4 < (1ll << 31)` in the C entry that launches it.

SITES lists every kernel or device body that builds a whole-tensor resource and the guards that protect it;
test_whole_tensor_resources_are_in_the_table (no GPU) re-reads the sources, so an unlisted site or a guard that no longer
reads `< (1ll << 31)` fails.  CASES calls the C entries directly with one operand padded to a wide leading dimension
(NaN in the padding columns and in guard rows behind row N), at the largest row count the guard admits, one row more,
and a row count whose padded operand exceeds 2^32 bytes (where a wrapped offset would really land elsewhere): the first
matches fp64, the others are refused with the message naming the limit and touch nothing.  The large-graph branch of
glass_comb_eff_bwd_f32 addresses its rows through 64-bit pointers (comb_dgrad_eff_kernel, wgrad_sl_kernel) and has no
limit: it matches fp64 at all three row counts."""
import os
import re

import pytest
import torch

from helpers import rel_inf, build_glass

TOL = 1e-5
DEV = "cuda:0"
Z = 0.85
LIMIT = 1 << 31
E_ARG, E_UNSUPPORTED = -1, -3
GUARD_ROWS = 64
NAN_BITS = 0x7FC00000  # torch.full(.., nan)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "glass_amd", "csrc")

# ---------------------------------------------------------------------------------------------------- the audit table
# ld_max of the trans pair's data-gradient guards (hidden 64 and 128)
_DGRAD_LD = (r"ld_max = std::max\(std::max\(ldd, ldo\), std::max\(std::max\(act != GLASS_ACT_NONE \? ldt : \(int64_t\)0, "
             r"addend \? ldadd : \(int64_t\)0\),\s*gn_partial \? gn_ldx : \(int64_t\)0\)\);")
# Guards: id -> (file, regex of the guard as written, operands and all; it must end in `< (1ll << 31)`) and the leading
# dimensions its ld_max covers.
GUARDS = {
    "fwd_h64": ("dense.hip", r"GLASS_TRANS_FWD_V2 && !comb && H == 64\)[\s\S]{0,400}?ld_max = std::max\(std::max\(ldo, T \? ldt : "
                r"\(int64_t\)0\), gn_saved \? ldxo : \(int64_t\)0\);\s*GLASS_REQUIRE\(n_nodes \* ld_max \* 4 < \(1ll << 31\) && "
                r"src_rows \* lda \* 4 < \(1ll << 31\)", "ldo, ldt, ldxo; lda over the source rows"),
    "fwd_h128": ("dense.hip", r"GLASS_TRANS_FWD_V2 && !comb && H == 128\)[\s\S]{0,400}?ld_max = std::max\(std::max\(ldo, T \? ldt : "
                 r"\(int64_t\)0\), gn_saved \? ldxo : \(int64_t\)0\);\s*GLASS_REQUIRE\(n_nodes \* ld_max \* 4 < \(1ll << 31\) && "
                 r"src_rows \* lda \* 4 < \(1ll << 31\)", "ldo, ldt, ldxo; lda over the source rows"),
    "dgrad_h64": ("dense.hip", r"if \(dg2\) \{[\s\S]{0,100}?" + _DGRAD_LD + r"\s*GLASS_REQUIRE\(n_nodes \* ld_max \* 4 < \(1ll << 31\)",
                  "ldd, ldo, ldt, ldadd, gn_ldx"),
    "dgrad_h128": ("dense.hip", r"GLASS_TRANS_DGRAD_V2 && H == 128 && n_out == H\)[\s\S]{0,100}?" + _DGRAD_LD +
                   r"\s*GLASS_REQUIRE\(n_nodes \* ld_max \* 4 < \(1ll << 31\)", "ldd, ldo, ldt, ldadd, gn_ldx"),
    "dgrad_comb128": ("dense.hip", r"GLASS_COMB_DGRAD_V2 && H == 128 && n_out == 2 \* H\)[\s\S]{0,600}?ld_max = std::max\(std::max\(ldd, ldo\), "
                      r"gn_partial \? gn_ldx : \(int64_t\)0\);\s*GLASS_REQUIRE\(n_nodes \* ld_max \* 4 < \(1ll << 31\)", "ldd, ldo, gn_ldx"),
    "dual_bwd_fused": ("dense.hip", r"GLASS_REQUIRE\(wg->X2 \|\| n_nodes \* wg->ldx \* 4 < \(1ll << 31\)",
                       "ldx of the trans pair (the dgrad_h64 guard covers the rest; with X2 the 64-bit wgrad_partial_body runs)"),
    "comb_eff_fwd": ("dense.hip", r"ld_max = std::max\(std::max\(lda, ldb\), std::max\(ldo, gn_saved \? ldxo : \(int64_t\)0\)\);\s*"
                     r"GLASS_REQUIRE\(!GLASS_COMB_FWD_V2 \|\| n_nodes \* ld_max \* 4 < \(1ll << 31\)", "lda, ldb, ldo, ldxo"),
    "comb_eff_bwd_fused": ("dense.hip", r"ld_max = std::max\(std::max\(std::max\(ldd, ldo\), gn_partial \? gn_ldx : \(int64_t\)0\), "
                           r"std::max\(ldx, ldx2\)\);\s*GLASS_REQUIRE\(n_nodes \* ld_max \* 4 < \(1ll << 31\)",
                           "ldd, ldo, gn_ldx, ldx, ldx2"),
    "comb_eff_bwd_gn_src": ("dense.hip", r"n_nodes \* std::max\(std::max\(g\.lddy, g\.ldx\), g\.addend \? g\.ldadd : \(int64_t\)0\) "
                            r"\* 4 < \(1ll << 31\)", "lddy, ldx, ldadd of dsrc_gn"),
    "wgrad128_trans": ("linear.hip", r"N \* std::max\(std::max\(ldd, ldx\), act != GLASS_ACT_NONE \? ldt : \(int64_t\)0\) \* 4 < "
                       r"\(1ll << 31\)", "ldd, ldx, ldt (else the slab kernel)"),
    "wgrad128_comb": ("linear.hip", r"N \* std::max\(std::max\(ldd, ldx\), ldx2\) \* 4 < \(1ll << 31\)", "ldd, ldx, ldx2 (else the slab kernel)"),
    "pair_head_fwd": ("pairhead.hip", r"n_nodes \* lde \* 4 < \(1ll << 31\) && P \* kPH \* 4 < \(1ll << 31\), \"pair_head_fwd", "lde; P rows of kPH"),
    "pair_head_bwd": ("pairhead.hip", r"n_nodes \* lde \* 4 < \(1ll << 31\) && P \* kPH \* 4 < \(1ll << 31\) && P < \(1ll << 29\)",
                      "lde; P rows of kPH"),
}

# Kernel or device body with a whole-tensor make_rsrc -> (file, the C entries and branches that launch it, guard ids)
SITES = {
    "trans_fwd2_kernel": ("dense.hip", "glass_dual_linear_fwd_f32: trans pair, hidden 64", ("fwd_h64",)),
    "trans_fwd3_kernel": ("dense.hip", "glass_dual_linear_fwd_f32: trans pair, hidden 128", ("fwd_h128",)),
    "trans_dgrad2_body": ("dense.hip", "glass_dual_linear_{dgrad,bwd}_f32: trans pair, hidden 64 (dual_dgrad_kernel, dual_bwd_kernel); "
                          "hidden 128 up to 256 row tiles, f32 products (trans_dgrad2_kernel)", ("dgrad_h64", "dgrad_h128")),
    "trans_dgrad3_kernel": ("dense.hip", "glass_dual_linear_{dgrad,bwd}_f32: trans pair, hidden 128, > 256 row tiles or split products",
                            ("dgrad_h128",)),
    "comb_dgrad3_kernel": ("dense.hip", "glass_dual_linear_{dgrad,bwd}_f32: comb pair, hidden 128", ("dgrad_comb128",)),
    "comb_fwd_eff2_kernel": ("dense.hip", "glass_comb_eff_fwd_f32: hidden 64 / 128, up to 80-row tiles", ("comb_eff_fwd",)),
    "comb_fwd_eff3_kernel": ("dense.hip", "glass_comb_eff_fwd_f32: hidden 64 / 128, taller tiles", ("comb_eff_fwd",)),
    "comb_dgrad2_body": ("dense.hip", "glass_comb_eff_bwd_f32: hidden 64, N <= kFusedBwdMaxRows (comb_bwd_eff_kernel)",
                         ("comb_eff_bwd_fused", "comb_eff_bwd_gn_src")),
    "wgrad_trans_staged2_body": ("wgrad_common.h", "glass_dual_linear_bwd_f32: trans pair, hidden 64, N <= kFusedBwdMaxRows, f32 "
                                 "products (dual_bwd_kernel)", ("dgrad_h64", "dual_bwd_fused")),
    "wgrad_trans_staged2s_body": ("wgrad_common.h", "the same, split products", ("dgrad_h64", "dual_bwd_fused")),
    "wgrad_sl_staged2_body": ("wgrad_common.h", "glass_comb_eff_bwd_f32: hidden 64, N <= kFusedBwdMaxRows, f32 products",
                              ("comb_eff_bwd_fused", "comb_eff_bwd_gn_src")),
    "wgrad_sl_staged2s_body": ("wgrad_common.h", "the same, split products", ("comb_eff_bwd_fused", "comb_eff_bwd_gn_src")),
    "wgrad128_trans_kernel": ("wgrad128.hip", "glass_dual_linear_wgrad_f32 (+ _bwd at hidden 128): trans pair, split products, "
                              "wgrad128_shape", ("wgrad128_trans",)),
    "wgrad128_comb_kernel": ("wgrad128.hip", "glass_dual_linear_wgrad_f32 (+ _bwd at hidden 128): comb pair, split products, "
                             "wgrad128_comb_shape", ("wgrad128_comb",)),
    "pair_head_fwd_kernel": ("pairhead.hip", "glass_pair_head_fwd_f32", ("pair_head_fwd",)),
    "pair_head_wgrad_kernel": ("pairhead.hip", "glass_pair_head_bwd_f32", ("pair_head_bwd",)),
}
# (tiled_wgrad8_kernel, wgrad_tiled.hip, rebases its resources on each slab: `rows * ld * 4` from `p + r0 * ld`; its own
# slab-size check in glass_dual_linear_wgrad_f32 is of another form and not a whole-tensor site)

# a make_rsrc whose size is rows-of-the-whole-tensor * leading dimension * 4
_WHOLE = re.compile(r"make_rsrc\((?:[^;]*?),\s*(?:[^;,]*?\?\s*)?\(?(?:N|n_nodes|a\.n_nodes|a\.P|xa_rows)\s*\*\s*[\w.>-]+\s*\*\s*4")


def _csrc(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _whole_tensor_sites():
    """{function name: file} of every whole-tensor make_rsrc in the sources (the nearest column-0 `void name(` above it)."""
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h", ".cpp")):
            continue
        lines = _csrc(name).split("\n")
        for i, line in enumerate(lines):
            if "make_rsrc(" not in line or "buf_rsrc make_rsrc(const void" in line:
                continue
            if not any(_WHOLE.search(part) for part in ("make_rsrc(" + p for p in line.split("make_rsrc(")[1:])):
                continue
            for j in range(i, -1, -1):
                m = re.match(r"^[^\s#/].*?\bvoid\s+(\w+)\s*\(", lines[j])
                if m:
                    found.setdefault(m.group(1), name)
                    break
            else:
                raise AssertionError(f"{name}:{i + 1}: make_rsrc outside any function")
    return found


def test_whole_tensor_resources_are_in_the_table():
    """CPU: every kernel or body that builds a whole-tensor buffer resource is a row of SITES (and every row still does),
    and every guard the table names still reads `< (1ll << 31)` where the table says it is."""
    found = _whole_tensor_sites()
    unlisted = sorted(set(found) - set(SITES))
    assert not unlisted, f"whole-tensor make_rsrc in kernels the offset-limit table does not list: {unlisted}"
    stale = sorted(set(SITES) - set(found))
    assert not stale, f"table rows without a whole-tensor make_rsrc in the sources: {stale}"
    for fn, (f, _entry, guards) in SITES.items():
        assert found[fn] == f, (fn, found[fn], f)
        assert guards and set(guards) <= set(GUARDS), (fn, guards)
    for gid, (f, rx, _covers) in GUARDS.items():
        assert re.search(rx, _csrc(f)), f"guard {gid} ({f}) no longer reads `< (1ll << 31)` over {_covers}"
    m = re.search(r"glass_comb_eff_max_rows\(int64_t ld\)[\s\S]{0,200}?\(\(1ll << 31\) - 1\) / \(4 \* ld\)", _csrc("dense.hip"))
    assert m, "glass_comb_eff_max_rows no longer caps rows at (2^31 - 1) / (4 ld)"


def test_comb_eff_gate_takes_the_widest_operand():
    """CPU: the step program's gate for the comb pair in effective-weight form asks glass_comb_eff_max_rows at the widest
    row stride of the pair's operands — the [n, 2H] data gradient, the H * L wide JK output the forward writes into — and
    never above the 4H the gate has always used (up to four JK layers it admits exactly the row counts it did)."""
    from types import SimpleNamespace
    from glass_amd import stack
    emb = lambda L, jk: SimpleNamespace(convs=[None] * L, jk=jk)
    assert stack._comb_eff_ld(emb(1, True), 64) == 256
    assert stack._comb_eff_ld(emb(2, False), 64) == 256
    assert stack._comb_eff_ld(emb(5, True), 128) == 640
    assert stack._comb_eff_ld(emb(4, True), 64) == 256
    assert stack._comb_eff_ld(emb(6, True), 64) == 384


# ---------------------------------------------------------------------------------------------------------- GPU cases
def _nmax(ld):
    """largest row count a guard `N * ld * 4 < 2^31` admits"""
    return (LIMIT - 1) // (4 * ld)


# id -> (entry, H, padded operand, ld at the limit, expect at N_max + 1 and above 2^32 bytes, ld and N above 2^32 bytes)
CASES = {
    "fwd_trans64": ("fwd", 64, "out", 2048, "refuse", 2048, 524_352),
    "fwd_trans128": ("fwd", 128, "out", 2048, "refuse", 2048, 524_352),
    "dgrad_trans64": ("dgrad", 64, "dsrc", 2048, "refuse", 2048, 524_352),
    "dgrad_trans128": ("dgrad", 128, "out", 2048, "refuse", 2048, 524_352),
    "dgrad_comb128": ("dgrad_comb", 128, "dsrc", 2048, "refuse", 2048, 524_352),
    "dual_bwd_trans64_fused": ("bwd", 64, "X", 5376, "refuse", 10_752, 100_000),
    "comb_eff_fwd64": ("comb_eff_fwd", 64, "out", 2048, "refuse", 2048, 524_352),
    "comb_eff_bwd64_fused": ("comb_eff_bwd", 64, "X", 5376, "refuse", 10_752, 100_000),
    "comb_eff_bwd64_two_launch": ("comb_eff_bwd", 64, "out", 2048, "match", 2048, 524_352),
    # the wgrad128 guards choose a kernel: past them the slab kernel (64-bit pointers) serves the call
    "wgrad128_trans": ("dual_wgrad", 128, "X", 2048, "match", 2752, 400_000),
    "wgrad128_comb": ("dual_wgrad", 128, "X", 2048, "match", 2752, 400_000),
    "linear_wgrad": ("linear_wgrad", 64, "X", 2048, "match", 2048, 524_352),   # generic geometry: 64-bit pointers, no limit
    "pair_head": ("pair_head", 64, "emb", 2048, "refuse", 2048, 524_352),     # forward and backward
}
# kernel-name substrings of the launches each case must make where it runs
KERNELS = {"fwd_trans64": ["trans_fwd2_kernel"], "fwd_trans128": ["trans_fwd3_kernel"], "dgrad_trans64": ["dual_dgrad_kernel"],
           "dgrad_trans128": ["trans_dgrad3_kernel"], "dgrad_comb128": ["comb_dgrad3_kernel"],
           "dual_bwd_trans64_fused": ["dual_bwd_kernel"], "comb_eff_fwd64": ["comb_fwd_eff3_kernel"],
           "comb_eff_bwd64_fused": ["comb_bwd_eff_kernel"], "comb_eff_bwd64_two_launch": ["comb_dgrad_eff_kernel", "wgrad_sl_kernel"],
           "wgrad128_trans": ["wgrad128_trans_kernel"], "wgrad128_comb": ["wgrad128_comb_kernel"], "linear_wgrad": ["wgrad_partial_kernel"],
           "pair_head": ["pair_head_fwd_kernel", "pair_head_wgrad_kernel"]}
# ... above the limit, where the case runs: (present, absent)
KERNELS_ABOVE = {"comb_eff_bwd64_two_launch": (KERNELS["comb_eff_bwd64_two_launch"], []),
                 "wgrad128_trans": (["wgrad_partial_split_kernel"], ["wgrad128_"]),
                 "wgrad128_comb": (["wgrad_partial_split_kernel"], ["wgrad128_"]),
                 "linear_wgrad": (["wgrad_partial_kernel"], [])}
# guard ids each case stands in front of (every guard of a launched row of SITES but the pair head's and wgrad128's)
CASE_GUARDS = {"fwd_trans64": "fwd_h64", "fwd_trans128": "fwd_h128", "dgrad_trans64": "dgrad_h64", "dgrad_trans128": "dgrad_h128",
               "dgrad_comb128": "dgrad_comb128", "dual_bwd_trans64_fused": "dual_bwd_fused", "comb_eff_fwd64": "comb_eff_fwd",
               "comb_eff_bwd64_fused": "comb_eff_bwd_fused", "wgrad128_trans": "wgrad128_trans", "wgrad128_comb": "wgrad128_comb",
               "pair_head": ("pair_head_fwd", "pair_head_bwd")}


def test_case_table_straddles_the_guards():
    """CPU: each case's N_max is the largest N its guard admits, the fused branches stay at or below kFusedBwdMaxRows and
    the other large-graph cases above it, and the third row count puts the padded operand past 2^32 bytes."""
    fused = int(re.search(r"constexpr\s+int64_t\s+kFusedBwdMaxRows\s*=\s*(\d+)\s*;", _csrc("wgrad_common.h")).group(1))
    for cid, (entry, H, _op, ld, _exp, ld4, n4) in CASES.items():
        n = _nmax(ld)
        assert n * ld * 4 < LIMIT <= (n + 1) * ld * 4
        assert n4 * ld4 * 4 > 2 * LIMIT, cid
        if "fused" in cid:
            assert n + 1 <= fused and n4 <= fused, cid
        else:
            assert n > fused, cid
    assert set(CASE_GUARDS) | {"comb_eff_bwd64_two_launch", "linear_wgrad"} == set(CASES)
    assert all(8192 <= n <= fused * 4 for c in ("wgrad128_trans", "wgrad128_comb") for n in (_nmax(CASES[c][3]), CASES[c][6]))
    # every row of the audit table stands behind at least one guard a case straddles
    covered = {g for v in CASE_GUARDS.values() for g in ((v, ) if isinstance(v, str) else v)}
    for fn, (_f, _entry, guards) in SITES.items():
        assert covered & set(guards), f"{fn}: no case at its guards {guards}"


def _padded(N, width, ld, fill):
    """[N + GUARD_ROWS, ld] float32 of NaN; the [N, width] view filled with `fill` (a callable of the shape) or left NaN"""
    buf = torch.full((N + GUARD_ROWS, ld), float("nan"), device=DEV)
    v = buf[:N, :width]
    if fill is not None:
        for r0 in range(0, N, 1 << 18):
            v[r0:r0 + (1 << 18)].copy_(fill((min(N, r0 + (1 << 18)) - r0, width)))
    return buf, v


def _canary_intact(buf, N, width, whole=False):
    """padding columns of rows < N and every column of the guard rows (or the whole buffer) still hold the NaN bits"""
    bits = buf.view(torch.int32)
    ok = True
    for r0 in range(0, buf.shape[0], 1 << 17):
        blk = bits[r0:r0 + (1 << 17)]
        if whole:
            ok &= bool((blk == NAN_BITS).all())
            continue
        nrow = max(0, min(N - r0, blk.shape[0]))
        if width < buf.shape[1] and nrow:
            ok &= bool((blk[:nrow, width:] == NAN_BITS).all())
        if nrow < blk.shape[0]:
            ok &= bool((blk[nrow:] == NAN_BITS).all())
    return ok


def _rows(N, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.cat([torch.arange(min(N, 4096)), torch.arange(max(0, N - 4096), N), torch.randperm(N, generator=g)[:65536]])
    return torch.unique(idx).to(DEV)


def _conv(H):
    from glass_amd.arena import ParamArena
    torch.manual_seed(0)
    model = build_glass(H, 1, 5, 3, "mean", "sum", Z).to(DEV).train()
    ParamArena(model)
    return model.conv.convs[0]


def _mix_w(mask_rows):
    """w1 of the label mix out = w1 A1 + (1 - w1) A0 (fp64 column)"""
    lab = mask_rows.bool().unsqueeze(1)
    return torch.where(lab, torch.tensor(Z, dtype=torch.float64, device=DEV), torch.tensor(1 - Z, dtype=torch.float64, device=DEV))


def _labels(N, seed):
    """label bytes (~1 %, first and last row labeled) and the labeled-row list of the comb-eff entries"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    mask = (torch.rand(N, device=DEV, generator=g) < 0.01).to(torch.uint8)
    mask[0] = mask[-1] = 1
    rows = mask.nonzero().flatten().to(torch.int32)
    cap = -(-rows.numel() // 64) * 64
    lab_rows = torch.zeros(cap, dtype=torch.int32, device=DEV)
    lab_rows[:rows.numel()] = rows
    return mask, lab_rows, torch.tensor([rows.numel()], dtype=torch.int32, device=DEV), cap


def _run(cid, N, ld):
    """One call of case `cid` at N rows with its padded operand at leading dimension ld (the pair head: its forward, then
    its backward).  Returns (return codes, message, kernel names, check_result(above), check_untouched): check_result
    asserts the result against fp64 and the launched kernels (called only when the entry ran), check_untouched the
    canaries and inputs."""
    from glass_amd import _lib, ops, stack
    lib = _lib.load()
    entry, H, padop, _ld, _exp, _ld4, _n4 = CASES[cid]
    conv = _conv(H)
    seed = N % 997
    gen = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda shape: torch.randn(shape, device=DEV, generator=gen)
    stream = torch.cuda.current_stream().cuda_stream
    if entry in ("comb_eff_fwd", "comb_eff_bwd") or cid == "wgrad128_comb":
        mask, lab_rows, lab_count, cap = _labels(N, seed)
    else:
        mask = (torch.rand(N, device=DEV, generator=gen) < 0.3).to(torch.uint8)
    pair = "comb" if entry in ("dgrad_comb", "comb_eff_fwd", "comb_eff_bwd") or cid == "wgrad128_comb" else "trans"
    st = conv._stack[pair]
    W, b = st[0].double(), st[1].double()
    # operands: name -> (buffer, view); the padded one at ld, the others contiguous
    bufs = {}
    small_outs = []  # outputs not shaped by N (the pair head's per-pair rows): all NaN after a refusal
    wgrad = None

    def operand(name, width, fill):
        buf, v = _padded(N, width, ld if name == padop else width, fill)
        bufs[name] = (buf, v, fill is None)
        return v
    if entry == "fwd":
        xa, out = operand("xa", H, rnd), operand("out", H, None)
        call = lambda: lib.glass_dual_linear_fwd_f32(xa.data_ptr(), xa.stride(0), 0, 0, st[4].data_ptr(), st[1].data_ptr(),
                                                     mask.data_ptr(), Z, ops.act_word(1), 0, 0, out.data_ptr(), out.stride(0), N, H,
                                                     0, 0, 0, 0, 0, 0.0, 0, 0, 0, 0, 0, 0, stream)
    elif entry in ("dgrad", "dgrad_comb", "bwd"):
        n_out = 2 * H if entry == "dgrad_comb" else H
        dsrc, out = operand("dsrc", H, rnd), operand("out", n_out, None)
        if entry == "bwd":
            X = operand("X", H, rnd)
            ws = torch.empty(int(lib.glass_linear_wgrad_ws_bytes(N, 2 * H, H)) // 4 + 16, device=DEV)
            call = lambda: lib.glass_dual_linear_bwd_f32(dsrc.data_ptr(), dsrc.stride(0), 0, 0, mask.data_ptr(), Z, ops.act_word(0),
                                                         st[5].data_ptr(), n_out, 0, 0, 0.0, 0, 0, out.data_ptr(), out.stride(0), N, H,
                                                         0, 0, 0, 0, 0, 0, 0.0, 0, 0, X.data_ptr(), X.stride(0), 0, 0, ws.data_ptr(),
                                                         stream)
        else:
            call = lambda: lib.glass_dual_linear_dgrad_f32(dsrc.data_ptr(), dsrc.stride(0), 0, 0, mask.data_ptr(), Z, ops.act_word(0),
                                                           st[5].data_ptr(), n_out, 0, 0, 0.0, 0, 0, out.data_ptr(), out.stride(0), N, H,
                                                           0, 0, 0, 0, 0, 0, 0.0, 0, 0, stream)
    elif entry == "comb_eff_fwd":
        xa, xb, out = operand("xa", H, rnd), operand("xb", H, rnd), operand("out", H, None)
        call = lambda: lib.glass_comb_eff_fwd_f32(xa.data_ptr(), xa.stride(0), xb.data_ptr(), xb.stride(0),
                                                  conv._stack_eff["comb"][0].data_ptr(), st[1].data_ptr(), mask.data_ptr(), Z,
                                                  out.data_ptr(), out.stride(0), N, H, 0, 0, 0, 0, ops.act_word(0), 0.0, 0, 0, 0, 0,
                                                  lab_rows.data_ptr(), lab_count.data_ptr(), cap, stream)
    elif entry == "dual_wgrad":
        dsrc, X = operand("dsrc", H, rnd), operand("X", H, rnd)
        X2 = operand("X2", H, rnd) if pair == "comb" else None
        I = 2 * H if pair == "comb" else H
        ws = torch.empty(int(lib.glass_linear_wgrad_ws_bytes(N, 2 * H, I)) // 4 + 16, device=DEV)
        wgrad = (torch.full((2 * H, I), float("nan"), device=DEV), torch.full((2 * H, ), float("nan"), device=DEV))
        call = lambda: lib.glass_dual_linear_wgrad_f32(dsrc.data_ptr(), dsrc.stride(0), 0, 0, mask.data_ptr(), Z, ops.act_word(0),
                                                       X.data_ptr(), X.stride(0), 0 if X2 is None else X2.data_ptr(),
                                                       0 if X2 is None else X2.stride(0), N, H, wgrad[0].data_ptr(), I,
                                                       wgrad[1].data_ptr(), 0, ws.data_ptr(), stream)
    elif entry == "linear_wgrad":  # G [N, 2H] against X [N, H]
        dsrc, X = operand("dsrc", 2 * H, rnd), operand("X", H, rnd)
        ws = torch.empty(int(lib.glass_linear_wgrad_ws_bytes(N, 2 * H, H)) // 4 + 16, device=DEV)
        wgrad = (torch.full((2 * H, H), float("nan"), device=DEV), torch.full((2 * H, ), float("nan"), device=DEV))
        call = lambda: lib.glass_linear_wgrad_f32(dsrc.data_ptr(), dsrc.stride(0), X.data_ptr(), X.stride(0), N, 2 * H, H,
                                                  wgrad[0].data_ptr(), H, wgrad[1].data_ptr(), 0, ws.data_ptr(), stream)
    elif entry == "pair_head":
        P = 20_011
        emb = operand("emb", H, rnd)
        demb = operand("demb", H, None)
        pairs = torch.randint(0, N, (P, 2), device=DEV, generator=gen)
        pairs[:300, 1] = N - 1  # a hub at the last row, and the first row
        pairs[300:400, 0] = 0
        y = (torch.rand(P, device=DEV, generator=gen) < 0.5).float()
        W0, b0 = 0.2 * rnd((H, H)), 0.1 * rnd((H, ))
        w1, b1 = 0.3 * rnd((H, )), rnd((1, ))
        hid, logits, dlogit = (torch.full(sh, float("nan"), device=DEV) for sh in ((P, H), (P, ), (P, )))
        dW0, db0, dw1, db1, loss = (torch.full(sh, float("nan"), device=DEV) for sh in ((H, H), (H, ), (H, ), (1, ), ()))
        small_outs += [hid, logits, dlogit, dW0, db0, dw1, db1, loss]
        pws = torch.empty(int(lib.glass_pair_head_ws_bytes(N, P)) + 16, dtype=torch.uint8, device=DEV)
        rcs = []

        def call():
            rcs.append(lib.glass_pair_head_fwd_f32(emb.data_ptr(), emb.stride(0), N, pairs.data_ptr(), P, W0.data_ptr(), b0.data_ptr(),
                                                   w1.data_ptr(), b1.data_ptr(), y.data_ptr(), 0.0, 0, 2, 0, hid.data_ptr(),
                                                   logits.data_ptr(), dlogit.data_ptr(), pws.data_ptr(), stream))
            # (the backward also after a refused forward: it must refuse on its own)
            rcs.append(lib.glass_pair_head_bwd_f32(emb.data_ptr(), emb.stride(0), N, pairs.data_ptr(), P, W0.data_ptr(), w1.data_ptr(),
                                                   hid.data_ptr(), dlogit.data_ptr(), 0.0, dW0.data_ptr(), db0.data_ptr(), dw1.data_ptr(),
                                                   db1.data_ptr(), 0, loss.data_ptr(), demb.data_ptr(), demb.stride(0), pws.data_ptr(),
                                                   stream))
            return rcs
    else:  # comb_eff_bwd
        dsrc, out = operand("dsrc", H, rnd), operand("out", 2 * H, None)
        X, X2 = operand("X", H, rnd), operand("X2", H, rnd)
        ws = torch.empty(int(lib.glass_comb_eff_ws_bytes(N, H, cap)) // 4 + 16, device=DEV)
        call = lambda: lib.glass_comb_eff_bwd_f32(dsrc.data_ptr(), dsrc.stride(0), mask.data_ptr(), Z,
                                                  conv._stack_eff["comb"][1].data_ptr(), out.data_ptr(), out.stride(0), N, H,
                                                  0, 0, 0, 0, 0, ops.act_word(0), 0.0, 0, 0, 0, X.data_ptr(), X.stride(0),
                                                  X2.data_ptr(), X2.stride(0), ws.data_ptr(), lab_rows.data_ptr(),
                                                  lab_count.data_ptr(), cap, 0, stream)
    inputs = {k: v.clone() for k, (_b, v, is_out) in bufs.items() if not is_out}
    torch.cuda.synchronize()
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        rc = call()
        torch.cuda.synchronize()
    rc = list(rc) if isinstance(rc, list) else [rc]
    kernels = sorted({e.name for e in prof.events() if "_kernel" in e.name})
    msg = lib.glass_last_error_string().decode(errors="replace") if any(rc) else ""
    if not any(rc) and entry in ("bwd", "comb_eff_bwd"):  # the deferred reduction of the weight-gradient partials
        dW = torch.full((2 * H, 2 * H if entry == "comb_eff_bwd" else H), float("nan"), device=DEV)
        db = torch.full((2 * H, ), float("nan"), device=DEV)
        job = (ws.data_ptr(), N, 2 * H, dW.shape[1], dW.data_ptr(), dW.stride(0), db.data_ptr(), 0)
        stack._reduce_pending([job + ((cap, ) if entry == "comb_eff_bwd" else ())])
        torch.cuda.synchronize()
        wgrad = (dW, db)

    def check_untouched():
        for k, (buf, v, is_out) in bufs.items():
            assert _canary_intact(buf, N, v.shape[1], whole=is_out and any(rc)), f"{cid} N={N}: canary of '{k}' overwritten"
            if not is_out:
                assert torch.equal(v, inputs[k]), f"{cid} N={N}: input '{k}' changed"
        if any(rc):
            for t in small_outs + ([] if wgrad is None else list(wgrad)):
                assert bool(torch.isnan(t).all()), f"{cid} N={N}: refused, but an output was written"

    def check_result(above):
        rows = _rows(N, seed)
        wm = _mix_w(mask[rows])
        worst = {}
        if entry == "pair_head":  # fp64 autograd of the head (the ReLU branches the kernel took, as in the SSL test)
            e64 = emb.double().requires_grad_(True)
            Wt, bt, wt, bbt = (t.double().requires_grad_(True) for t in (W0, b0, w1, b1))
            pre = e64[pairs].mean(dim=1) @ Wt.T + bt
            x64 = (pre * (hid > 0).double()) @ wt + bbt
            l64 = torch.nn.BCEWithLogitsLoss()(x64, y.double())
            l64.backward()
            worst["logits"] = rel_inf(logits.double(), x64.detach())
            worst["loss"] = abs(loss.item() - l64.item()) / abs(l64.item())
            for k, mine, ref in (("dW0", dW0, Wt.grad), ("db0", db0, bt.grad), ("dw1", dw1, wt.grad), ("db1", db1, bbt.grad)):
                worst[k] = rel_inf(mine.double(), ref)
            worst["demb"] = rel_inf(demb.double()[rows], e64.grad[rows])
            worst["demb_hub"] = rel_inf(demb.double()[N - 1], e64.grad[N - 1])
        elif entry in ("fwd", "comb_eff_fwd"):
            x = xa[rows].double() if entry == "fwd" else torch.cat([xa[rows], xb[rows]], 1).double()
            A = x @ W.t() + b
            if entry == "fwd":
                A = torch.nn.functional.elu(A)
            ref = wm * A[:, :H] + (1 - wm) * A[:, H:]
        elif entry not in ("dual_wgrad", "linear_wgrad"):
            dc = dsrc[rows].double()
            ref = (wm * dc) @ W[:H] + ((1 - wm) * dc) @ W[H:]
        if entry not in ("dual_wgrad", "linear_wgrad", "pair_head"):
            worst["out"] = rel_inf(out[rows].double(), ref)
        if wgrad is not None:  # the full reduction over all N rows, in fp64 on the device
            dW_ref = torch.zeros(wgrad[0].shape, dtype=torch.float64, device=DEV)
            db_ref = torch.zeros(2 * H, dtype=torch.float64, device=DEV)
            for r0 in range(0, N, 1 << 17):
                sl = slice(r0, min(N, r0 + (1 << 17)))
                dc = dsrc[sl].double()
                if entry == "linear_wgrad":
                    dZ = dc
                else:
                    ww = _mix_w(mask[sl])
                    dZ = torch.cat([ww * dc, (1 - ww) * dc], 1)
                x = torch.cat([X[sl], X2[sl]], 1).double() if pair == "comb" and entry != "dgrad_comb" else X[sl].double()
                dW_ref += dZ.t() @ x
                db_ref += dZ.sum(0)
            worst["dW"] = rel_inf(wgrad[0].double(), dW_ref)
            worst["db"] = rel_inf(wgrad[1].double(), db_ref)
        print(f"{cid} N={N} ld={ld}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()) + f"  kernels {kernels}")
        assert max(worst.values()) <= TOL, (cid, N, worst)
        present, absent = KERNELS_ABOVE[cid] if above else (KERNELS[cid], [])
        for k in present:
            assert any(k in n for n in kernels), f"{cid} N={N}: no '{k}' launch; kernels: {kernels}"
        for k in absent:
            assert not any(k in n for n in kernels), f"{cid} N={N}: '{k}' launched past its guard; kernels: {kernels}"

    return rc, msg, kernels, check_result, check_untouched


def _case(cid, which):
    entry, H, padop, ld, expect, ld4, n4 = CASES[cid]
    if which == "nmax":
        return ld, _nmax(ld), "match"
    if which == "nmax+1":
        return ld, _nmax(ld) + 1, expect
    return ld4, n4, expect


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["nmax", "nmax+1", "over4g"])
@pytest.mark.parametrize("cid", sorted(CASES))
def test_entry_at_the_offset_limit(cid, which):
    """One entry / branch at one row count: the largest N its guard admits -> fp64 (first / last 4 096 rows + a 64 K sample;
    weight gradients over every row); one row more and a padded operand past 2^32 bytes -> GLASS_E_ARG naming the 2^31
    limit, output, padding and guard rows untouched (the large-graph comb-eff backward: fp64 at every N).  Inputs never
    change."""
    ld, N, expect = _case(cid, which)
    run = None
    try:
        run = _run(cid, N, ld)
        rc, msg, kernels, check_result, check_untouched = run
        if expect == "match":
            assert not any(rc), f"{cid} N={N} ld={ld}: refused ({rc}): {msg}"
            check_result(which != "nmax")
        else:
            assert all(r in (E_ARG, E_UNSUPPORTED) for r in rc), f"{cid} N={N} ld={ld}: returned {rc} past the 32-bit offset limit"
            assert "2^31" in msg, msg
            assert not kernels, f"{cid} N={N}: refused, but launched {kernels}"
        check_untouched()
    finally:
        print(f"{cid} N={N}: peak device memory {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB")
        del run  # (the closures hold the multi-GiB operands) before the cache is handed back
        rc = msg = kernels = check_result = check_untouched = None
        torch.cuda.empty_cache()
