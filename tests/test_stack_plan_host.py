"""CPU: glass_amd.stack.plan_stack — which kernel form each step of the stack program takes, on both sides of every limit
and with every switch flipped alone.  Only the host-side query exports of libglass_hip.so are needed (no GPU).  The expected
values are written out from the rules (the comments of plan_stack), never computed with plan_stack itself."""
import pytest

from glass_amd import _lib, stack

CAP = 80  # capacity of the labeled-row list (B * Smax)


def _lib_q():
    return _lib.load()


def P(**kw):
    """plan_stack over a default training pass with a fused readout at hidden 64, two layers, jk; checks on EVERY plan that the
    accumulator blocks handed to producers are distinct and inside the allocation, and that the allocation adds up."""
    H, L = kw.get("H", 64), kw.get("L", 2)
    a = dict(H=H, L=L, V=100, n=300, jk=True, unlabeled=False, train=True, keep=True, has_labels=True, labels_cap=CAP,
             in_head=False, readout=("sum", False), prologue_done=False, advance=False,
             eff=((True, H == 64), ) * L)  # arena: both images at hidden 64, the forward image alone at hidden 128
    a.update(kw)
    plan = stack.plan_stack(**a)
    assert len(plan.layers) == a["L"]
    written = [b for lp in plan.layers for b in (lp.gn_fwd_acc, lp.c_acc, lp.gn_bwd_acc, lp.gns_bwd_acc) if b >= 0]
    assert len(set(written)) == len(written) and all(b < plan.n_bwd + plan.n_fwd for b in written), plan
    assert plan.acc_words == (plan.n_bwd + plan.n_fwd) * plan.w_h + plan.w_ro, plan
    assert (plan.exact == "none") == (plan.acc_words == 0)
    if plan.final_src is not None:  # the final GraphNorm reads the blocks the comb epilogues wrote
        first, count = plan.final_src
        assert list(range(first, first + count)) == [lp.c_acc for lp in plan.layers][-count:]
    for lp in plan.layers:  # a sum lives in an accumulator block or in partials, never both
        assert not (lp.c_acc >= 0 and lp.c_blocks) and (lp.gn_bwd_acc >= 0) != (lp.gn_bwd_blocks > 0)
    return plan


def forms(plan):
    return [(lp.comb_fwd, lp.comb_bwd) for lp in plan.layers]


def words(C):
    return int(_lib_q().glass_gn_exact_words(C))


def dense_blocks(n, H):
    return -(-n // int(_lib_q().glass_dual_linear_stat_rows(H)))


def test_library_facts_the_cases_rest_on():
    lib = _lib_q()
    assert lib.glass_gn_exact_supported(64) == 1 and lib.glass_gn_exact_supported(128) == 0
    assert lib.glass_gn_exact_fwd_supported(128) == 1
    assert lib.glass_comb_eff_supported(64) == 1 and lib.glass_comb_eff_supported(128) == 0
    assert lib.glass_comb_eff_fwd_supported(64) == 1 and lib.glass_comb_eff_fwd_supported(128) == 1
    assert lib.glass_dual_linear_fwd_gather_supported(64) == 1
    # above every exact-sum limit: the effective-form limit is tested with the partials forms around it
    assert lib.glass_comb_eff_max_rows(256) > stack.GN_EXACT_MAX_ROWS and lib.glass_comb_eff_max_rows(512) > stack.GN_EXACT_MAX_ROWS
    assert (stack.GN_EXACT_MAX_ROWS, stack.GN_EXACT_FWD_ONLY_MAX_ROWS, stack.GN_EXACT_READOUT_MAX_ROWS) == (1 << 18, 1 << 14, 1 << 16)
    assert _lib.EMBED_NORM_MAX_ROWS == 8192


def test_hidden64_default_plan_in_full():
    """N = 300: every sum in exact accumulators — blocks [gn0 bwd | gns0 bwd | gn1 bwd | gn0 fwd, gn1 fwd | c0, c1 | readout]."""
    lib = _lib_q()
    plan = P()
    assert plan.embed == "gather" and not plan.skip_prologue and not plan.head and plan.tail == "fused" and plan.fused_bwd
    assert (plan.exact, plan.n_bwd, plan.n_fwd, plan.w_h, plan.w_ro) == ("all", 3, 4, words(64), words(128))
    assert plan.acc_words == 7 * words(64) + words(128) and plan.final_src == (5, 2)
    assert plan.n_rep == stack.REP_DENSE and plan.dense_blocks == dense_blocks(300, 64)
    in_comb = bool(lib.glass_comb_eff_bwd_gn_src_supported(300, 64))
    assert plan.layers == (stack.LayerPlan("eff", 3, 5, 0, "eff", 0, 0, -1, in_comb), stack.LayerPlan("eff", 4, 6, 0, "eff", 2, 0, 1, False))


@pytest.mark.parametrize("H,L", [(64, 2), (128, 1)])
def test_gn_exact_max_rows(H, L):
    """2^18: hidden 64 leaves the `all` mode (two layers, 128 output columns: no smaller mode takes over); hidden 128 is far
    above its own limits on both sides."""
    lib = _lib_q()
    lo, hi = P(H=H, L=L, n=1 << 18), P(H=H, L=L, n=(1 << 18) + 1)
    if H == 64:
        assert (lo.exact, lo.n_bwd, lo.n_fwd, lo.w_ro) == ("all", 3, 4, words(128))
        assert lo.layers[0].gn_in_comb == bool(lib.glass_comb_eff_bwd_gn_src_supported(1 << 18, 64))
    else:
        assert lo.exact == "none"
    n = (1 << 18) + 1
    assert (hi.exact, hi.acc_words, hi.final_src) == ("none", 0, None)
    for lp in hi.layers:  # float64 partials everywhere; the effective kernels' own block counts where they run
        assert (lp.gn_fwd_acc, lp.c_acc, lp.gn_bwd_acc, lp.gns_bwd_acc, lp.gn_in_comb) == (-1, -1, -1, -1, False)
        assert lp.c_blocks == lib.glass_comb_eff_fwd_blocks(n, H, CAP)
        assert lp.gn_bwd_blocks == (lib.glass_comb_eff_blocks(n, H, CAP) if H == 64 else dense_blocks(n, 128))
    assert forms(hi) == [("eff", "eff")] * 2 if H == 64 else [("eff", "dual")]


def test_hidden128_fwd_only_and_readout_only_limits():
    """One layer at hidden 128 (H * L = 128): forward sums + readout block up to 2^14 rows, the readout's block alone up to
    2^16, nothing above."""
    lib = _lib_q()
    a, b = P(H=128, L=1, n=1 << 14), P(H=128, L=1, n=(1 << 14) + 1)
    assert (a.exact, a.n_bwd, a.n_fwd, a.w_h, a.w_ro, a.acc_words) == ("fwd_only", 0, 2, words(128), words(128), 3 * words(128))
    assert a.final_src == (1, 1)
    assert a.layers == (stack.LayerPlan("eff", 0, 1, 0, "dual", -1, dense_blocks(1 << 14, 128), -1, False), )
    assert (b.exact, b.n_bwd, b.n_fwd, b.w_ro, b.acc_words, b.final_src) == ("readout_only", 0, 0, words(128), words(128), None)
    assert b.layers == (stack.LayerPlan("eff", -1, -1, int(lib.glass_comb_eff_fwd_blocks((1 << 14) + 1, 128, CAP)), "dual", -1,
                                        dense_blocks((1 << 14) + 1, 128), -1, False), )
    c, d = P(H=128, L=1, n=1 << 16), P(H=128, L=1, n=(1 << 16) + 1)
    assert (c.exact, c.w_ro, c.acc_words) == ("readout_only", words(128), words(128))
    assert (d.exact, d.w_ro, d.acc_words) == ("none", 0, 0)
    # two layers with jk: 256 output columns — no readout block at any size, and no forward-only mode (gns[0] between layers)
    assert P(H=128, L=2, n=300).exact == "none"
    assert P(H=128, L=2, n=300, jk=False).exact == "readout_only"


@pytest.mark.parametrize("H,L,ld", [(64, 2, 256), (128, 1, 512)])
def test_comb_eff_max_rows(H, L, ld):
    lib = _lib_q()
    n = int(lib.glass_comb_eff_max_rows(ld))
    lo, hi = P(H=H, L=L, n=n), P(H=H, L=L, n=n + 1)
    assert forms(lo) == [("eff", "eff" if H == 64 else "dual")] * L and forms(hi) == [("dual", "dual")] * L
    assert [lp.c_blocks for lp in lo.layers] == [lib.glass_comb_eff_fwd_blocks(n, H, CAP)] * L
    assert [lp.c_blocks for lp in hi.layers] == [dense_blocks(n + 1, H)] * L
    assert [lp.gn_bwd_blocks for lp in lo.layers] == [lib.glass_comb_eff_blocks(n, H, CAP) if H == 64 else dense_blocks(n, H)] * L
    assert [lp.gn_bwd_blocks for lp in hi.layers] == [dense_blocks(n + 1, H)] * L
    # six layers with jk at hidden 64: the row stride of the cap is the JK buffer's (384 floats)
    n6 = int(lib.glass_comb_eff_max_rows(384))
    assert n6 < n or H == 128
    if H == 64:
        assert forms(P(L=6, n=n6))[0] == ("eff", "eff") and forms(P(L=6, n=n6 + 1))[0] == ("dual", "dual")


@pytest.mark.parametrize("H,L", [(64, 2), (128, 1)])
def test_table_rows_labels_readout_keep(H, L):
    gather = "gather" if _lib_q().glass_dual_linear_fwd_gather_supported(H) else "table"
    # V: the table kernels up to 8192 rows
    assert (P(H=H, L=L, V=8192).embed, P(H=H, L=L, V=8192).tail) == (gather, "fused")
    assert (P(H=H, L=L, V=8193).embed, P(H=H, L=L, V=8193).tail) == ("plain", "plain")
    # no labels handed in (z tensor): no effective form, no gather in trans, no readout-only block; `all` needs no labels
    nl = P(H=H, L=L, has_labels=False)
    assert nl.embed == "table" and nl.tail == "fused" and forms(nl) == [("dual", "dual")] * L
    assert not any(lp.gn_in_comb for lp in nl.layers)
    assert (nl.exact, nl.n_bwd, nl.n_fwd) == (("all", 3, 4) if H == 64 else ("none", 0, 0))
    # no readout (the autograd node): no forward sums, no readout block
    nr = P(H=H, L=L, readout=None)
    assert (nr.exact, nr.n_bwd, nr.n_fwd, nr.w_ro, nr.final_src) == (("all", 3, 0, 0, None) if H == 64 else ("none", 0, 0, 0, None))
    assert all(lp.gn_fwd_acc == -1 and lp.c_acc == -1 and lp.c_blocks > 0 for lp in nr.layers)
    # keep = False: no backward blocks, no readout block
    nk = P(H=H, L=L, keep=False)
    assert (nk.exact, nk.n_bwd, nk.n_fwd, nk.w_ro) == (("all", 0, 4, 0) if H == 64 else ("fwd_only", 0, 2, 0))
    assert nk.final_src == ((2, 2) if H == 64 else (1, 1))
    ev = P(H=H, L=L, keep=False, readout=None, train=False)
    assert (ev.exact, ev.acc_words) == ("none", 0)


def test_prologue_skip_and_head():
    """The evaluation forward behind a shared prologue skips its own launch unless it needs something from it."""
    ev = dict(keep=False, readout=None, train=False, prologue_done=True, has_labels=False)
    assert P(**ev).skip_prologue and P(**ev, V=8193).skip_prologue
    assert not P(**dict(ev, prologue_done=False)).skip_prologue
    assert not P(**ev, advance=True).skip_prologue
    assert not P(**dict(ev, has_labels=True)).skip_prologue            # gather in trans: emb_gn's table statistics
    assert not P(**dict(ev, readout=("sum", False))).skip_prologue      # accumulators to zero-fill
    assert P(in_head=True).head and not P(in_head=True, train=False).head and not P(in_head=True, has_labels=False).head
    assert not P(**dict(ev, has_labels=True, in_head=True, train=True, V=8193)).skip_prologue   # the head launch labels the batch


def test_unlabeled_stack():
    lib = _lib_q()
    plan = P(jk=False, unlabeled=True, labels_cap=1, readout=None, advance=True)
    assert (plan.embed, plan.tail, plan.skip_prologue) == ("identity", "unlabeled", False)
    assert (plan.exact, plan.n_bwd, plan.n_fwd, plan.w_ro, plan.acc_words, plan.final_src) == ("all", 3, 4, 0, 7 * words(64), None)
    in_comb = bool(lib.glass_comb_eff_bwd_gn_src_supported(300, 64))
    assert plan.layers == (stack.LayerPlan("eff", 3, 5, 0, "eff", 0, 0, -1, in_comb),
                           stack.LayerPlan("eff_nostats", 4, -1, 0, "eff", 2, 0, 1, False))
    assert P(jk=False, unlabeled=True, labels_cap=1, readout=None, V=1 << 20).embed == "identity"  # any table size


def test_each_switch_flipped_alone(monkeypatch):
    base = P()

    def flipped(name, value=False, **kw):
        with monkeypatch.context() as m:
            m.setattr(stack, name, value)
            return P(**kw)
    p = flipped("USE_COMB_EFF")
    assert forms(p) == [("dual", "dual")] * 2 and not p.layers[0].gn_in_comb and p._replace(layers=()) == base._replace(layers=())
    p = flipped("USE_GN_EXACT")
    assert (p.exact, p.acc_words, p.final_src) == ("none", 0, None) and forms(p) == [("eff", "eff")] * 2
    assert all(lp.c_blocks > 0 and lp.gn_bwd_blocks > 0 and not lp.gn_in_comb for lp in p.layers)
    p = flipped("USE_GN_EXACT_FWD")
    assert (p.exact, p.n_bwd, p.n_fwd, p.w_ro, p.acc_words, p.final_src) == ("all", 3, 0, words(128), 3 * words(64) + words(128), None)
    assert [lp.gn_bwd_acc for lp in p.layers] == [0, 2] and all(lp.gn_fwd_acc == -1 and lp.c_blocks > 0 for lp in p.layers)
    p = flipped("USE_READOUT_TWO")
    assert p == base._replace(w_ro=0, acc_words=7 * words(64))
    assert flipped("USE_READOUT_TWO", H=128, L=1, n=20000).exact == "none" and P(H=128, L=1, n=20000).exact == "readout_only"
    p = flipped("USE_GN_BWD_IN_COMB")
    assert p == base._replace(layers=(base.layers[0]._replace(gn_in_comb=False), base.layers[1]))
    assert flipped("USE_EMBED_TABLE") == base._replace(embed="plain", tail="plain")
    assert flipped("USE_GATHER_IN_TRANS") == base._replace(embed="table")
    assert flipped("USE_FUSED_TAIL") == base._replace(tail="table")
    assert flipped("USE_FUSED_BWD") == base._replace(fused_bwd=False)
    assert flipped("REP_DENSE", 8) == base._replace(n_rep=8)
    assert flipped("USE_READOUT") == base  # (a gate of step_supported, not a kernel form)
    # (300 rows above the limit: 128 output columns, so the readout's block alone is kept)
    assert flipped("GN_EXACT_MAX_ROWS", 299).exact == "readout_only" and flipped("GN_EXACT_MAX_ROWS", 300) == base
    # the defaults are back
    assert P() == base


def test_gates_read_the_switches_at_call_time(monkeypatch):
    assert stack._readout_ok("sum", 128, 6) and stack._readout_ok("max", 128, 6) and stack._unlabeled_forms_ok(64)
    assert not stack._unlabeled_forms_ok(128)
    monkeypatch.setattr(stack, "USE_READOUT", False)
    assert not stack._readout_ok("sum", 128, 6)
    monkeypatch.setattr(stack, "USE_COMB_EFF", False)
    assert not stack._unlabeled_forms_ok(64)
