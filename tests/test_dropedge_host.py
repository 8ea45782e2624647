"""Edge dropout without a GPU: self-checks of the restatement tests/dropedge_oracle.py (so that the GPU tests cannot pass
vacuously), the host-side answers of glass_adj_dropedge_f32, and the refusals of the layer, the factory and the driver."""
import numpy as np
import pytest
import torch

import dropedge_oracle as DO


def test_generator_restatement_against_hand_values():
    """mix32 of three words worked by hand from the definition (Python integers), and the avalanche's fixed point 0."""
    def by_hand(x):
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        return x ^ (x >> 16)
    xs = [0, 1, 0x9E3779B9, 0xFFFFFFFF, 123456789]
    assert [int(v) for v in DO.mix32(np.array(xs, dtype=np.uint64))] == [by_hand(x) for x in xs] and by_hand(0) == 0
    # the counter's high word enters rand4 on its own: keys 2^32 apart differ
    a = DO.rand4_word0(DO.SEED, 0, 18, np.array([5, 5 + (1 << 32)], dtype=np.uint64))
    assert int(a[0]) != int(a[1]) and int(a.max()) < 1 << 32


def test_the_graph_has_the_row_lengths_on_both_sides_of_the_lane_stride():
    n, ei, w, und = DO.mixed("rand")
    fwd, tr = DO.row_lengths(ei, n)
    for lens in (fwd, tr):
        assert {0, 1, 2, 63, 64, 65, 200} <= set(int(v) for v in lens)
    assert fwd[DO.IN_ONLY] == 3 and tr[DO.IN_ONLY] == 0 and fwd[DO.OUT_ONLY] == 0 and tr[DO.OUT_ONLY] == 3
    assert int((ei[0] == ei[1]).sum()) == len(DO.LOOPS)
    assert int(((ei[0] == DO.DUP[0]) & (ei[1] == DO.DUP[1])).sum()) == 2       # a parallel duplicate
    assert int((~und).sum()) == 11 + len(DO.LOOPS) and not np.array_equal(ei[0] * n + ei[1], np.sort(ei[0] * n + ei[1]))
    wi = DO.mixed("int")[2]
    assert set(np.unique(wi)) == {1.0, 2.0, 3.0} and float(w.min()) >= 0.2 and len(np.unique(w)) > 100
    assert np.array_equal(DO.mixed("int")[1], ei)


@pytest.mark.parametrize("step", (0, 1))
@pytest.mark.parametrize("call_id", DO.CALL_IDS)
def test_oracle_masks_are_not_vacuous(call_id, step):
    n, ei, w, und = DO.mixed("rand")
    assert bool(DO.keep_mask(ei, n, 0.0, DO.SEED, step, call_id).all())
    k3 = DO.keep_mask(ei, n, 0.3, DO.SEED, step, call_id)
    assert 0.2 <= 1.0 - k3.mean() <= 0.4
    k9 = DO.keep_mask(ei, n, 0.9, DO.SEED, step, call_id)
    kept = np.bincount(ei[0], weights=k9, minlength=n)
    size = np.bincount(ei[0], minlength=n)
    assert bool(((size > 0) & (kept == 0)).any()), "a non-empty row fully dropped"
    assert bool(((kept > 0) & (kept < size)).any()), "a row partly dropped"
    # symmetric: (i, j) and (j, i) agree for every undirected pair (parallel duplicates included); non-symmetric: some differ
    pos = {}
    for e in range(ei.shape[1]):
        pos.setdefault((int(ei[0, e]), int(ei[1, e])), []).append(e)
    for p in (0.3, 0.9):
        ks, kn = DO.keep_mask(ei, n, p, DO.SEED, step, call_id, True), DO.keep_mask(ei, n, p, DO.SEED, step, call_id, False)
        differ = 0
        for (i, j), es in pos.items():
            if und[es[0]]:
                both = es + pos[(j, i)]
                assert len(set(int(ks[e]) for e in both)) == 1
                differ += len(set(int(kn[e]) for e in both)) == 2
        assert differ > 0
    # the mask depends on the step, on the call id and on the key mode
    assert not np.array_equal(k3, DO.keep_mask(ei, n, 0.3, DO.SEED, step + 2, call_id))
    assert not np.array_equal(k3, DO.keep_mask(ei, n, 0.3, DO.SEED, step, call_id + 1))


def test_masked_values_restatement():
    """Row sums below 0.5 take the + 1 (a fully dropped row: degree 1, all-zero values); no row sum near the rule's jump."""
    n, ei, w, _ = DO.mixed("rand")
    keep = DO.keep_mask(ei, n, 0.9, DO.SEED, 0, DO.CALL_IDS[0])
    for aggr in DO.AGGRS:
        val, deg = DO.masked_values(ei, w, keep, n, aggr)
        assert float(np.abs(deg - 0.5).min()) > 1e-3 and bool((val[keep == 0] == 0).all()) and bool((val[keep != 0] > 0).all())
        dead = np.bincount(ei[0], weights=keep, minlength=n) == 0
        assert bool((deg[dead] == 1.0).all()) and bool((DO.dense(ei, val, n)[dead] == 0).all())
        if aggr == "mean":
            live = ~dead & (np.bincount(ei[0], weights=np.where(keep != 0, w, 0), minlength=n) >= 0.5)
            assert np.allclose(DO.dense(ei, val, n)[live].sum(1), 1.0, rtol=1e-12)


def test_entry_validates_on_the_host():
    """Refusals come before any HIP call (the host buffers never reach a kernel): no GPU needed."""
    from glass_amd import _lib
    lib = _lib.load()
    E_ARG, E_UNSUPPORTED = -1, -3
    f = np.zeros(8, dtype=np.float32)
    i32 = np.zeros(8, dtype=np.int32)
    i64 = np.zeros(2, dtype=np.int64)
    u8 = np.zeros(8, dtype=np.uint8)
    P, I = f.ctypes.data, i32.ctypes.data

    def call(rowptr=I, col=I, w=P, rowptr_t=I, col_t=I, w_t=P, n=2, aggr=0, p=0.3, sym=1, rng=i64.ctypes.data, call_id=18, deg=P,
             val=P, val_t=P, keep=u8.ctypes.data):
        return lib.glass_adj_dropedge_f32(rowptr, col, w, rowptr_t, col_t, w_t, n, aggr, p, sym, rng, call_id, deg, val, val_t, keep,
                                          None)
    for null in ("rowptr", "col", "w", "rowptr_t", "col_t", "w_t", "rng", "deg", "val", "val_t"):
        assert call(**{null: None}) == E_ARG, null
        assert b"adj_dropedge" in lib.glass_last_error_string()
    assert call(n=-1) == E_ARG and call(n=2**31 - 1) == E_ARG
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert call(p=bad) == E_ARG, bad
    assert b"outside [0, 1)" in lib.glass_last_error_string()
    assert call(aggr=3) == E_UNSUPPORTED and call(aggr=-1) == E_UNSUPPORTED and b"unknown aggr" in lib.glass_last_error_string()
    assert call(aggr=7, rowptr=None) == E_UNSUPPORTED
    assert call(n=0) == 0 and call(n=0, keep=None) == 0          # nothing to do: no launch
    assert lib.glass_version() == _lib.ABI_VERSION == 6          # purely additive
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "glass_hip.h")) as fh:
        assert "int glass_adj_dropedge_f32(" in fh.read()
    assert "glass_adj_dropedge_f32" in _lib.SIGNATURES


def test_layer_factory_and_helper_refusals():
    from helpers import build_glass
    from impl import models
    for bad in (-0.1, 1.0, 2, float("nan"), "0.3", True):
        with pytest.raises(ValueError, match="edge_dropout"):
            models.GLASSConv(8, 8, aggr="mean", edge_dropout=bad)
    for aggr in ("max", "softmax", "gat", "std", "var", "pna"):
        with pytest.raises(ValueError, match="edge_dropout"):
            models.GLASSConv(8, 8, aggr=aggr, edge_dropout=0.2)
        assert models.GLASSConv(8, 8, aggr=aggr, edge_dropout=0.0).edge_dropout == 0.0       # 0 is always accepted
        with pytest.raises(ValueError, match="edge_dropout"):
            build_glass(8, 2, 4, 3, aggr, "sum", 0.8, edge_dropout=0.2)
    with pytest.raises(ValueError, match="live_edge_weight"):
        models.GLASSConv(8, 8, aggr="mean", edge_dropout=0.2, live_edge_weight=True)
    with pytest.raises(ValueError, match="live_edge_weight"):
        build_glass(8, 2, 4, 3, "mean", "sum", 0.8, edge_dropout=0.2, live_edge_weight=True)
    conv = models.GLASSConv(8, 8, aggr="gcn", edge_dropout=0.25, edge_dropout_symmetric=False)
    assert conv.edge_dropout == 0.25 and conv.edge_dropout_symmetric is False
    assert models.GLASSConv(8, 8).edge_dropout == 0.0 and models.GLASSConv(8, 8).edge_dropout_symmetric is True
    # a replicated batch is refused at the call, before anything is built or launched
    x, mask = torch.zeros(6, 8), torch.zeros(6, dtype=torch.uint8)
    ei, ew = torch.zeros(2, 1, dtype=torch.int64), torch.ones(1)
    from glass_amd import ops
    with pytest.raises(ValueError, match="replicated"):
        conv(x, ei, ew, mask, batch=ops.Replicas(2, 3))
    assert conv.adj is None
    # the helper: all layers or none
    model = build_glass(8, 2, 4, 3, "mean", "sum", 0.8)
    models.set_edge_dropout(model.conv, 0.4, symmetric=False)
    assert all(c.edge_dropout == 0.4 and c.edge_dropout_symmetric is False for c in model.conv.convs)
    with pytest.raises(ValueError, match="edge_dropout"):
        models.set_edge_dropout(model.conv, 1.0)
    assert all(c.edge_dropout == 0.4 for c in model.conv.convs)
    with pytest.raises(ValueError, match="edge_dropout"):
        models.set_live_edge_weight(model.conv)
    pna = build_glass(8, 2, 4, 3, "pna", "sum", 0.8)
    with pytest.raises(ValueError, match="edge_dropout"):
        models.set_edge_dropout(pna.conv, 0.2)
    models.set_edge_dropout(pna.conv, 0.0)
    live = build_glass(8, 2, 4, 3, "mean", "sum", 0.8, live_edge_weight=True)
    with pytest.raises(ValueError, match="live_edge_weight"):
        models.set_edge_dropout(live.conv, 0.2)


def test_state_dict_and_stack_program():
    from helpers import build_glass
    from glass_amd import stack
    for hidden in (64, 8):
        torch.manual_seed(0)
        plain = build_glass(hidden, 2, 4, 3, "mean", "sum", 0.8)
        torch.manual_seed(0)
        drop = build_glass(hidden, 2, 4, 3, "mean", "sum", 0.8, edge_dropout=0.3)
        zero = build_glass(hidden, 2, 4, 3, "mean", "sum", 0.8, edge_dropout=0.0)
        sd, sd2 = plain.state_dict(), drop.state_dict()
        assert list(sd) == list(sd2) == list(zero.state_dict()) and all(torch.equal(sd[k], sd2[k]) for k in sd)
        assert all(c.edge_dropout == 0.3 for c in drop.conv.convs)
        assert stack.StackProgram.supported(drop.conv) is False
        assert stack.StackProgram.supported(zero.conv) == stack.StackProgram.supported(plain.conv)

    # what `supported` answers once everything else holds: a stand-in whose other conditions are cut short
    class Conv:
        aggr, live_edge_weight, edge_dropout = "mean", False, 0.3

    class Emb:
        convs = [Conv()]
    assert stack.StackProgram.supported(Emb()) is False


def test_driver_arguments():
    import GLASSTest
    assert GLASSTest.parse_args(["--use_one"]).edge_dropout is None
    assert GLASSTest.parse_args(["--use_one", "--edge_dropout", "0.2"]).edge_dropout == 0.2
    assert GLASSTest.parse_args(["--use_one", "--edge_dropout", "0.2", "--aggr", "gcn"]).edge_dropout == 0.2
    assert GLASSTest.parse_args(["--use_one", "--edge_dropout", "0", "--use_zeroone"]).edge_dropout == 0.0
    for extra in (["--use_zeroone"], ["--edge_saliency", "s.npy"], ["--aggr", "max"], ["--aggr", "pna"]):
        with pytest.raises(SystemExit):
            GLASSTest.parse_args(["--use_one", "--edge_dropout", "0.2"] + extra)
    for bad in ("1.0", "-0.1", "nan", "half"):
        with pytest.raises(SystemExit):
            GLASSTest.parse_args(["--use_one", "--edge_dropout", bad])
    # the layers the driver builds carry the rate
    from impl import models
    run = GLASSTest.Run.__new__(GLASSTest.Run)
    run.args = GLASSTest.parse_args(["--use_one", "--edge_dropout", "0.2"])
    run.max_deg, run.output_channels = 4, 3
    model = run.build_model(64, 2, 0.0, 1, "sum", 0.8, "mean", edge_dropout=0.2)
    assert isinstance(model, models.GLASS) and all(c.edge_dropout == 0.2 for c in model.conv.convs)
    assert all(c.edge_dropout == 0.0 for c in run.build_model(64, 2, 0.0, 1, "sum", 0.8, "mean").conv.convs)
