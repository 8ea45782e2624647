"""The fused training readout (sum / mean / size) without a GPU: the recipes of tests/readout_oracle.py produce what they claim,
the stage chain equals torch autograd, an fp32 restatement of every stage IN THE KERNELS' SUMMATION ORDER passes the gate with
room to spare (its worst share of the bar is printed per stage and held to 0.5), the gate refuses each single mistake a kernel
could make, the restated dispatch gives the expected record on both sides of every threshold and its constants are the ones in
the source text, and the entry's argument codes through the real library with dummy pointers."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import readout_oracle as Q  # noqa: E402

E_ARG, E_UNSUPPORTED, E_WS = -1, -3, -4
POOLS = ("sum", "mean", "size")


# ---- recipes -------------------------------------------------------------------------------------------------------------------
def test_recipes_produce_what_they_claim():
    ins = Q.recipe(64, 3, 130, 128, 300, seed=5, shared=((11, 63), (12, 64), (13, 65)))
    pos, N = ins["pos"], 300
    mult = Q.multiplicity(pos, N)
    assert [int(mult[n]) for n in (11, 12, 13)] == [63, 64, 65] and ins["facts"]["shared"] == {11: 63, 12: 64, 13: 65}
    assert Q.LONG_LIST == 64  # 63 below, 64 and 65 on the workgroup-wide path of the gather-add
    for n in (11, 12, 13):  # exactly m ROWS: once per row
        assert int(((pos == n).sum(1) > 0).sum()) == int(mult[n])
    assert int(mult[Q.TWICE]) == 2 and int((pos[3] == Q.TWICE).sum()) == 2
    assert int(mult[Q.THRICE]) == 3 and all(int(pos[b, 0]) == Q.THRICE for b in (4, 5, 6))
    assert int(mult[N - 1]) == 0 and int(mult[N - 2]) == 0
    assert bool((pos[1] == -1).all()) and int(pos[2, 0]) == N + 5 and int(pos[2, 1]) == 1 << 40
    cnt = Q.valid_of(pos, N).sum(1)
    assert int(cnt[1]) == 0 and int(cnt[0]) > 0 and len(set(cnt.tolist())) > 10  # ragged
    assert bool((ins["gamma"] > 0).any()) and bool((ins["gamma"] < 0).any())
    again = Q.recipe(64, 3, 130, 128, 300, seed=5, shared=((11, 63), (12, 64), (13, 65)))
    assert torch.equal(again["pos"], pos) and torch.equal(again["jk"], ins["jk"])
    # guard columns
    g = Q.recipe(64, 3, 40, 3, 300, seed=5, ldj=72, lddj=68)
    assert g["jk"].shape == (300, 72) and bool(torch.isnan(g["jk"][:, 64:]).all()) and bool(torch.isfinite(g["jk"][:, :64]).all())
    # small batches keep what fits
    one = Q.recipe(64, 3, 1, 3, 300, seed=5)
    assert one["facts"]["all_padding"] is None and int(Q.valid_of(one["pos"], 300).sum()) == 3
    assert Q.recipe(64, 1, 40, 3, 300, seed=5)["loss_mode"] == 1


# ---- the chain is the autograd statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_mode", [0, 1])
@pytest.mark.parametrize("mode", POOLS)
def test_chain_equals_autograd(mode, loss_mode):
    ins = Q.recipe(12, 3, 9, 7, 97, seed=11, loss_mode=loss_mode, ldj=14)
    want = Q.autograd_readout(ins, mode, grad_loss=-2.5)
    got = Q.chain(ins, mode, grad_loss=-2.5)
    for k in ("pooled", "logits", "loss", "djk", "dWh", "dbh", "dgamma", "dbeta", "dalpha"):
        assert Q.rel_inf(got[k], want[k]) < 1e-11, k
    assert float(got["pooled"][1].abs().sum()) == 0.0


# ---- fp32 restatement in the kernels' order ----------------------------------------------------------------------------------------
f32 = np.float32


def _fma(a, b, c):
    return (a.astype(np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def _restate_f32(ins, mode, rec, grad_loss):
    """numpy fp32 in the order of readout_subgraph_kernel<4>, readout_reduce_kernel and the ordered scatter: a row slot adds
    its entries j = tr, tr + rpb, ... in turn (fmaf for the affine), the slots are added in order, the logits' lanes run an fma
    chain over c = lane, lane + 64, ... and fold by xor shuffles 32 .. 1, d pooled / dWh are fma chains over k / b, the scatter an
    fma chain over the entries in (b, s) order added to fmaf(Bx, x, K)."""
    C, K, B, S, N = ins["C"], ins["K"], ins["B"], ins["Smax"], ins["N"]
    jk = ins["jk"][:, :C].numpy()
    pos = ins["pos"].numpy()
    saved = Q.stage_saved(ins["jk"][:, :C], ins["gamma"], ins["beta"], ins["alpha"], ins["eps"])[0].numpy().astype(f32)
    mu, rstd, scale, shift = saved
    al, Wh, bh = ins["alpha"].numpy(), ins["Wh"].numpy(), ins["bh"].numpy()
    rpb = rec["rpb"]
    valid = (pos >= 0) & (pos < N)
    cnt = valid.sum(1)
    sc = np.ones(B, dtype=f32)
    if mode == "mean":
        sc = (f32(1) / np.maximum(cnt, 1).astype(f32)).astype(f32)
    if mode == "size":
        sc = np.where(cnt > 0, f32(1) / np.sqrt(np.maximum(cnt, 1).astype(f32)), f32(0)).astype(f32)
    pooled, xh = np.zeros((B, C), f32), np.zeros((B, C), f32)
    for b in range(B):
        ay, ah = np.zeros((rpb, C), f32), np.zeros((rpb, C), f32)
        for tr in range(rpb):
            for j in range(tr, S, rpb):
                if valid[b, j]:
                    x = jk[pos[b, j]]
                    ay[tr] = ay[tr] + _fma(x, scale, shift)
                    ah[tr] = ah[tr] + ((x - al * mu).astype(f32) * rstd).astype(f32)
        for r in range(1, rpb):
            ay[0] = ay[0] + ay[r]
            ah[0] = ah[0] + ah[r]
        pooled[b], xh[b] = ay[0] * sc[b], ah[0]
    logits = np.zeros((B, K), f32)
    for b in range(B):
        for k in range(K):
            s = np.zeros(64, f32)
            for c0 in range(0, C, 64):
                n = min(64, C - c0)
                s[:n] = _fma(pooled[b, c0:c0 + n], Wh[k, c0:c0 + n], s[:n])
            for o in (32, 16, 8, 4, 2, 1):
                s = (s + s[np.arange(64) ^ o]).astype(f32)
            logits[b, k] = s[0] + bh[k]
    dl, rows = np.zeros((B, K), f32), np.zeros(B, f32)
    gscale = f32(grad_loss) / (f32(B) if ins["loss_mode"] == 0 else f32(B) * f32(K))
    for b in range(B):
        z = logits[b]
        if ins["loss_mode"] == 0:
            m = z.max()
            se = f32(0)
            for k in range(K):
                se = f32(se + np.exp(f32(z[k] - m)))
            lse = f32(m + np.log(se))
            t = int(ins["target"][b])
            for k in range(K):
                dl[b, k] = gscale * f32(np.exp(f32(z[k] - lse)) - f32(1 if t == k else 0))
            rows[b] = lse - z[t]
        else:
            y = ins["target"].numpy().reshape(B, K)[b]
            term = f32(0)
            for k in range(K):
                dl[b, k] = gscale * f32(f32(1) / f32(f32(1) + np.exp(-z[k])) - y[k])
                term = f32(term + f32(f32(max(z[k], f32(0)) - f32(z[k] * y[k])) + np.log1p(np.exp(-np.abs(z[k])))))
            rows[b] = term
    loss = f32(rows.astype(np.float64).sum() / (B if ins["loss_mode"] == 0 else B * K))
    dys = np.zeros((B, C), f32)
    for b in range(B):
        s = np.zeros(C, f32)
        for k in range(K):
            s = _fma(np.full(C, dl[b, k], f32), Wh[k], s)
        dys[b] = sc[b] * s
    partial = np.stack([cnt.reshape(-1, 1).astype(np.float64) * dys.astype(np.float64), dys.astype(np.float64) * xh.astype(np.float64)], 1)
    dWh, dbh = np.zeros((K, C), f32), np.zeros(K, f32)
    for k in range(K):
        s = np.zeros(C, f32)
        for b in range(B):
            s = _fma(np.full(C, dl[b, k], f32), pooled[b], s)
            dbh[k] = dbh[k] + dl[b, k]
        dWh[k] = s
    part_t = torch.from_numpy(partial)
    Gn = Q.stage_gn_bwd(part_t, part_t.abs(), N, ins["gamma"], ins["alpha"], torch.from_numpy(saved))
    coef = Gn["coef"][0].numpy().astype(f32)
    djk = _fma(jk, coef[1], coef[2])
    acc = np.zeros((N, C), f32)
    for b in range(B):
        for s_ in range(S):
            if valid[b, s_]:
                acc[pos[b, s_]] = _fma(coef[0], dys[b], acc[pos[b, s_]])
    djk = (djk + acc).astype(f32)
    out = dict(saved=saved, pooled=pooled, logits=logits, loss_rows=rows, dlogits=dl, loss=np.asarray(loss), dys=dys, partial=partial,
               coef=coef, dWh=dWh, dbh=dbh, djk=djk)
    out.update({k: Gn[k][0].numpy().astype(f32) for k in ("dgamma", "dbeta", "dalpha")})
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


@pytest.mark.parametrize("loss_mode", [0, 1])
@pytest.mark.parametrize("mode", POOLS)
def test_fp32_restatement_in_kernel_order_passes_the_gate(mode, loss_mode):
    """C = 64: 16 lanes per row slot, 16 slots, Smax = 40 -> up to three entries per slot, then the slot fold."""
    ins = Q.recipe(64, 3, 9, 40, 97, seed=21, loss_mode=loss_mode)
    rec = Q.dispatch(64, 9, 40, 97)
    got = _restate_f32(ins, mode, rec, grad_loss=-2.5)
    sv = Q.stage_saved(ins["jk"], ins["gamma"], ins["beta"], ins["alpha"], ins["eps"])
    ok, share, _ = Q.gate(got["saved"], *sv)
    shares = {k: v[1] for k, v in Q.grade(got, ins, mode, rec, grad_loss=-2.5).items()}
    shares["saved"] = share
    print(f"fp32 restatement {mode} loss {loss_mode}: " + " ".join(f"{k} {v:.3f}" for k, v in shares.items()))
    assert all(v <= 0.5 for v in shares.values()), shares
    e2e = Q.chain(ins, mode, grad_loss=-2.5)
    for k in ("pooled", "logits", "loss", "djk", "dWh", "dbh"):
        assert Q.rel_inf(got[k], e2e[k]) <= Q.TOL, k


# ---- the gate refuses single mistakes ----------------------------------------------------------------------------------------------
def _exact_got(ins, mode, grad_loss=1.0, prev=None):
    """the chain's outputs rounded to fp32: what a correct kernel returns, up to one rounding"""
    c = Q.chain(ins, mode, grad_loss, prev)
    got = {k: v.float() for k, v in c.items()}
    L = Q.stage_loss(c["logits"], ins["target"], ins["loss_mode"], grad_loss)
    got["loss_rows"] = L["loss_rows"][0].float()
    got["partial"] = Q.stage_partial(c["dys"], ins["jk"][:, :ins["C"]], c["saved"], ins["alpha"], ins["pos"])[0]
    return got


def _verdicts(got, ins, mode, **kw):
    return {k: v[0] for k, v in Q.grade(got, ins, mode, Q.dispatch(ins["C"], ins["B"], ins["Smax"], ins["N"]), **kw).items()}


def test_gate_accepts_the_rounded_truth_and_refuses_each_single_mistake():
    ins = Q.recipe(12, 3, 9, 7, 97, seed=31)
    pos, N, C = ins["pos"], 97, 12
    jk = ins["jk"]
    for mode in POOLS:
        assert all(_verdicts(_exact_got(ins, mode), ins, mode).values()), mode
    base = _exact_got(ins, "sum")
    saved = base["saved"]

    def with_pos(fn, mode="sum", as_mode=None):
        p = pos.clone()
        fn(p)
        got = dict(base if as_mode is None else _exact_got(ins, as_mode))
        got["pooled"] = Q.stage_pooled(jk, saved, p, mode)[0].float()
        return _verdicts(got, ins, as_mode or "sum")

    b0 = 0  # a full row
    assert not with_pos(lambda p: p.__setitem__((b0, 2), -1))["pooled"], "one dropped entry"

    def count_padding(p):
        b, s = [(b, s) for b in range(9) for s in range(7) if p[b, s] < 0 and b != 1][0]
        p[b, s] = 0
    assert not with_pos(count_padding)["pooled"], "a padding entry counted"
    assert not with_pos(lambda p: None, mode="mean", as_mode="size")["pooled"], "mean scale used for size"
    assert not with_pos(lambda p: p.__setitem__((3, 1), -1))["pooled"], "the twice-listed node counted once"
    # d jk: one subgraph's contribution missing from the shared node; the neighbouring column's coefficients
    c = Q.chain(ins, "sum")
    part, part_m = Q.stage_partial(c["dys"], jk, c["saved"], ins["alpha"], pos)
    Gn = Q.stage_gn_bwd(part, part_m, N, ins["gamma"], ins["alpha"], c["saved"])
    p = pos.clone()
    p[5, 0] = -1
    got = dict(base)
    got["djk"] = Q.stage_djk(jk, Gn["coef"][0], Gn["coef"][1], c["dys"], p)[0].float()
    assert int((got["djk"] != base["djk"]).any(1).sum()) == 1 and bool((got["djk"][Q.THRICE] != base["djk"][Q.THRICE]).any())
    assert not _verdicts(got, ins, "sum")["djk"], "a subgraph missing from a shared node's d jk"
    for which in (1, 2):
        coef = Gn["coef"][0].clone()
        coef[which] = coef[which].roll(1)
        got = dict(base)
        got["djk"] = Q.stage_djk(jk, coef, Gn["coef"][1], c["dys"], pos)[0].float()
        assert not _verdicts(got, ins, "sum")["djk"], ("Bx", "K")[which - 1] + " of the neighbouring column"
    # acc_head ignored
    prev = dict(dWh=torch.full((3, C), 0.25), dbh=torch.full((3, ), -0.5))
    assert all(_verdicts(_exact_got(ins, "sum", prev=prev), ins, "sum", prev=prev).values())
    v = _verdicts(base, ins, "sum", prev=prev)
    assert not v["dWh"] and not v["dbh"], "acc_head ignored"
    # BCE: denominator B instead of B * K
    bce = Q.recipe(12, 3, 9, 7, 97, seed=31, loss_mode=1)
    good = _exact_got(bce, "sum")
    assert all(_verdicts(good, bce, "sum").values())
    bad = dict(good)
    bad["dlogits"], bad["loss"] = good["dlogits"] * 3, good["loss"] * 3
    v = _verdicts(bad, bce, "sum")
    assert not v["dlogits"] and not v["loss"], "the BCE denominator B instead of B * K"
    # mass 0 means exactly 0; a NaN is an error
    bad = dict(base)
    bad["pooled"] = base["pooled"].clone()
    bad["pooled"][1, 0] = 1e-30
    assert not _verdicts(bad, ins, "sum")["pooled"]
    bad["pooled"][1, 0] = float("nan")
    assert not _verdicts(bad, ins, "sum")["pooled"]


# ---- dispatch -----------------------------------------------------------------------------------------------------------------
def test_restated_constants_are_the_ones_in_the_source_text():
    k = Q.source_constants()
    assert k["kBlock"] == Q.BLOCK == 256 and k["kWave"] == Q.WAVE == 64 and k["kOrdBlock"] == Q.ORD_BLOCK == 1024
    assert k["kReadoutOrderedMax"] == Q.ORDERED_MAX == 16384 and k["kReadoutMaxK"] == Q.MAX_K == 256
    assert k["max_c_in_blocks"] * k["kBlock"] == Q.MAX_C == 1024
    assert k["backfill_cap"] == Q.BACKFILL_CAP == 2048 and k["dense_cap"] == Q.DENSE_CAP == 4096
    assert k["kLong"] == Q.LONG_LIST == 64
    assert k["lds_head"] == Q.LDS_HEAD == 10 and k["red_stride"] == Q.RED_STRIDE == 8
    for text in ("lds1_text", "stash_text", "lds3_attr_text", "tc_text", "early_text", "short_text"):
        assert k[text], text
    assert Q.LDS_LIMIT == 64 * 1024
    assert Q.dispatch(1024, 4, 2, 300)["lds1"] == 51200  # the 10 * C / 8 * kBlock / 2 * 256 head at C = 1024


def test_dispatch_record_on_both_sides_of_every_threshold():
    d = Q.dispatch
    # lane geometry
    assert [d(C, 40, 3, 300)["tc"] for C in (4, 64, 96, 128, 132, 1024)] == [1, 16, 32, 32, 64, 256]
    assert d(1024, 40, 3, 300)["rpb"] == 1 and d(4, 40, 3, 300)["rpb"] == 256
    assert d(128, 40, 3, 300)["early"] and not d(132, 40, 3, 300)["early"]
    # the short loop: Smax <= 2 * rpb
    for C, s, kw in ((64, 32, {}), (1024, 2, {}), (17, 16, dict(labels=True))):
        lo, hi = d(C, 40, s, 300, **kw), d(C, 40, s + 1, 300, **kw)
        assert lo["loop"] == "short" and not lo["stash"] and hi["loop"] == "unrolled" and hi["stash"], (C, s)
    assert d(17, 40, 3, 300, labels=True)["tc"] == 32 and d(17, 40, 3, 300, labels=True)["tail"] == "scalar"
    # the stash bound at C = 1024
    lo, hi = d(1024, 4, 3584, 300), d(1024, 4, 3585, 300)
    assert lo["stash"] and lo["lds1"] == 65536 and not hi["stash"] and hi["lds1"] == 51200 and hi["loop"] == "unrolled"
    # the ordered limit
    for kw, tail in ((dict(), "dense+ordered"), (dict(labels=True), "backfill"), (dict(labels=True, bwd_acc=True), "backfill")):
        assert d(64, 128, 128, 300, **kw)["tail"] == tail
    two = d(64, 128, 128, 300, labels=True, bwd_acc=True)
    assert two["two"] and two["lds3"] == 65536 + 28 * 64 > Q.LDS_LIMIT
    assert d(64, 128, 128, 300, labels=True)["lds3"] == 65536 and not d(64, 128, 128, 300, labels=True)["two"]
    for kw in (dict(), dict(labels=True), dict(labels=True, bwd_acc=True)):
        r = d(64, 5, 3277, 300, **kw)
        assert r["tail"] == "dense+gather" and not r["two"], kw
    assert d(64, 130, 128, 300, longest_list=65)["long_lists"] and not d(64, 130, 128, 300, longest_list=63)["long_lists"]
    # grid caps
    assert not d(1024, 6, 5, 16384)["cap"] and d(1024, 6, 5, 16500)["cap"]
    assert not d(1024, 6, 5, 32768, labels=True)["cap"] and d(1024, 6, 5, 33000, labels=True)["cap"]
    assert Q.second_round_rows(1024, 16500, "dense+ordered") == (0, 16384) and Q.second_round_rows(1024, 33000, "backfill") == (0, 32768)
    # scalar form
    for C, kw in ((17, {}), (1, {}), (255, {}), (64, dict(aligned=False)), (258, {}), (260, dict(aligned=False))):
        r = d(C, 40, 3, 300, labels=True, bwd_acc=True, **kw)
        assert not r["vec"] and r["tail"] == "scalar" and not r["two"], C
    assert d(255, 40, 3, 300, labels=True)["slots_used"] == 1 and d(258, 40, 3, 300, labels=True)["slots_used"] == 2
    assert d(258, 40, 3, 300, labels=True)["tc"] == 256 and d(258, 40, 3, 300, labels=True)["loop"] == "unrolled"


# ---- the entry on the host -----------------------------------------------------------------------------------------------------
def _args(p, B=80, Smax=10, n=1000, C=128, K=6, loss_mode=0, mode=0, **over):
    a = dict(jk=p, ldj=C, saved=p, gamma=p, alpha=p, pos=p, B=B, Smax=Smax, mode=mode, Wh=p, bh=p, target=p, loss_mode=loss_mode, K=K,
             grad_loss=p, pooled=p, logits=p, loss=p, djk=p, lddj=C, dWh=p, dbh=p, acc_head=0, dgamma=p, dbeta=p, dalpha=p,
             acc_gn=0, ws=p, n=n, C=C, mask=None, rows=None, count=None, gn_src=None, bwd_acc=None, bwd_rep=0, sws=None,
             loss_sum=None, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def test_train_entry_codes_on_the_host_before_any_launch():
    from glass_amd import _lib
    lib = _lib.load()
    x = np.zeros(64, dtype=np.float32)
    p = x.ctypes.data
    f = lib.glass_readout_train_f32
    for name in ("jk", "saved", "gamma", "alpha", "pos", "Wh", "bh", "target", "grad_loss", "pooled", "logits", "loss", "djk", "dWh",
                 "dbh", "ws"):
        assert f(*_args(p, **{name: None})) == E_ARG, name
    for over in (dict(B=0), dict(Smax=0), dict(n=0), dict(ldj=64), dict(lddj=64), dict(Smax=1 << 31)):
        assert f(*_args(p, **over)) == E_ARG, over
    assert f(*_args(p, C=1028, ldj=1028, lddj=1028)) == E_UNSUPPORTED
    assert f(*_args(p, K=257)) == E_UNSUPPORTED and f(*_args(p, loss_mode=2)) == E_UNSUPPORTED and f(*_args(p, mode=2)) == E_UNSUPPORTED
    # the scalar form (C % 4 != 0, a row stride off 4, a base pointer off 16 bytes) needs the label bytes
    for over in (dict(C=17, ldj=17, lddj=17), dict(ldj=129), dict(lddj=130), dict(jk=p + 4), dict(C=258, ldj=258, lddj=258),
                 dict(C=260, ldj=261, lddj=260)):
        assert f(*_args(p, **over)) == E_ARG, over
        assert b"label bytes" in lib.glass_last_error_string()
    # 4(a): widths beyond 256 columns are SERVED by the scalar form (a thread's four slots take the columns c0 + 256 k)
    for C in (258, 260, 1023, 1024):
        assert lib.glass_readout_supported(C, 6, 0) == 1 and lib.glass_readout_max_supported(C, 6) == 1
    assert lib.glass_readout_supported(1025, 6, 0) == 0
    # the ordered limit: 16 384 entries need no scatter workspace, 16 385 do
    assert lib.glass_readout_scatter_ws_bytes(300, 128, 128) == 0 and lib.glass_readout_scatter_ws_bytes(300, 5, 3277) > 0
    assert f(*_args(p, B=5, Smax=3277)) == E_WS and b"scatter_ws" in lib.glass_last_error_string()
    assert f(*_args(p, mask=p, rows=p, count=p, bwd_acc=p, bwd_rep=17)) == E_ARG
    for B, C, K in ((80, 128, 6), (7, 17, 3), (1, 1, 1)):
        assert lib.glass_readout_ws_bytes(B, C, K) == Q.ws_bytes(B, C, K)
