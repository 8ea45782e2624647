"""Evaluation metrics on the MI355X (glass_amd/csrc/evalmetrics.hip): the device counters against the numpy restatement of
tests/metrics_counts.py — EXACT integer equality, they are integer sums — then glass_amd.metrics.device_score against the
host functions, and train.test on a tiny GLASS model and a tiny seg.GNN model.

Bounds: counters ==; both F1 forms == (one division of the same integers scikit-learn divides); AUROC |difference| <= 1e-12
(twoU / (2 P N) rounded once against scikit-learn's fp64 trapezoid sum)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from helpers import build_glass  # noqa: E402
from metrics_counts import auroc_counts, f1_counts  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 63, 64, 65, 255, 256, 257, 1000)


def _lib():
    from glass_amd import _lib
    return _lib.load()


def _ks():
    """Columns: both sides of the lane-per-row / wave-per-row threshold, one and 256, and 5 / 13: with rows of K + 3
    elements those take the float4 loads and a scalar tail."""
    from glass_amd import _lib
    t = _lib.EVAL_F1_LANE_K
    return sorted({1, 2, 3, 5, 13, 16, 17, 256, t, t + 1})


def _place(a, layout):
    """numpy [n, K] -> (device view with the same values, row stride): contiguous, rows of K + 3 elements, or contiguous
    from a base pointer 4 bytes past a 16-byte boundary."""
    n, K = a.shape
    t = torch.from_numpy(np.ascontiguousarray(a))
    if layout == "strided":
        buf = torch.full((n, K + 3), 7.0, dtype=t.dtype, device=DEV)  # (the padding would count if it were read)
        buf[:, :K] = t.to(DEV)
        return buf[:, :K], K + 3
    if layout == "misaligned":
        buf = torch.empty(n * K + 1, dtype=t.dtype, device=DEV)
        view = buf[1:].view(n, K)
        view.copy_(t.to(DEV))
        assert view.data_ptr() % 16 == 4
        return view, K
    return t.to(DEV), K


def _f1_dev(pred, ldp, target, ldt, n, K, mode, counts=None):
    counts = torch.full((8, ), -5, dtype=torch.int64, device=DEV) if counts is None else counts  # (stale values: the entry zeroes)
    rc = _lib().glass_eval_f1_counts_f32(pred.data_ptr(), ldp, target.data_ptr(), ldt, n, K, mode, counts.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib().glass_last_error_string()
    return counts


def _auroc_dev(score, lds, label, ldl, n, K, counts=None):
    counts = torch.full((K, 4), -5, dtype=torch.int64, device=DEV) if counts is None else counts
    rc = _lib().glass_eval_auroc_counts_f32(score.data_ptr(), lds, label.data_ptr(), ldl, n, K, counts.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _lib().glass_last_error_string()
    return counts


def _adversarial_pred(rng, n, K, kind):
    """Logits quantised to {-1, 0, 1} (most rows have tied maxima) or Gaussian; then, where the shape has room: one row all
    equal, rows with a NaN at index 0 / in the middle / at K - 1, rows with +inf and -inf, and -0.0 / +0.0 entries."""
    pred = rng.integers(-1, 2, (n, K)).astype(np.float32) if kind == "ties" else rng.standard_normal((n, K)).astype(np.float32)
    if n >= 12:
        pred[1, :] = 0.5
        pred[2, 0] = np.nan
        pred[3, K // 2] = np.nan
        pred[4, K - 1] = np.nan
        pred[5, 0], pred[5, K - 1] = np.nan, np.nan        # the first NaN wins
        pred[6, K - 1] = np.inf
        pred[7, :] = -np.inf                                # all -inf: argmax 0
        pred[8, K // 2] = -np.inf
        pred[9, :] = -0.0
        pred[9, K - 1] = 0.0                                # -0.0 == +0.0: the lowest index; neither is > 0
        pred[10, :] = np.inf                                # tied infinities
        pred[11, 0] = -0.0
    return pred


@pytest.mark.parametrize("layout", ["contiguous", "strided", "misaligned"])
@pytest.mark.parametrize("kind", ["ties", "normal"])
def test_multiclass_counters_equal_numpy(layout, kind):
    rng = np.random.default_rng(1)
    for n in NS:
        for K in _ks():
            pred = _adversarial_pred(rng, n, K, kind)
            y = rng.integers(0, K, n)
            if n >= 12:
                y[2], y[3], y[4], y[5], y[7], y[9], y[10] = 0, K // 2, K - 1, 0, 0, 0, 0   # (hits only with numpy's argmax)
                y[0], y[6], y[8] = K, -1, 1 << 40                                          # outside [0, K): never correct
            p, ldp = _place(pred, layout)
            got = _f1_dev(p, ldp, torch.from_numpy(y).to(DEV), 1, n, K, 0).cpu().numpy()
            want = f1_counts(pred, y, 0)
            assert (got == want).all(), (n, K, got, want)
            assert got[4] == 0


@pytest.mark.parametrize("layout", ["contiguous", "strided", "misaligned"])
@pytest.mark.parametrize("kind", ["ties", "normal"])
def test_binary_counters_equal_numpy(layout, kind):
    rng = np.random.default_rng(2)
    for n in NS:
        for K in _ks():
            pred = _adversarial_pred(rng, n, K, kind)
            y = (rng.random((n, K)) < 0.4).astype(np.float32)
            if n >= 12:
                y[9, :] = 1.0          # against -0.0 / +0.0 predictions: all false negatives
                y[11, 0] = -0.0        # a target of -0.0 is the class 0
            p, ldp = _place(pred, layout)
            t, ldt = _place(y, layout)
            got = _f1_dev(p, ldp, t, ldt, n, K, 1).cpu().numpy()
            want = f1_counts(pred, y, 1)
            assert (got == want).all(), (n, K, got, want)
            assert got[:4].sum() == n * K and got[4] == 0


@pytest.mark.parametrize("K", [1, 3, 16, 17, 256])
def test_invalid_binary_targets_are_counted_and_refused(K):
    from glass_amd import metrics
    rng = np.random.default_rng(3)
    n = 130
    pred = rng.standard_normal((n, K)).astype(np.float32)
    y = (rng.random((n, K)) < 0.5).astype(np.float32)
    y[5, 0], y[77, K - 1], y[129, K // 2] = 0.5, np.nan, 2.0
    want = f1_counts(pred, y, 1)
    assert want[4] == 3
    p, t = torch.from_numpy(pred).to(DEV), torch.from_numpy(y).to(DEV)
    got = _f1_dev(p, K, t, K, n, K, 1).cpu().numpy()
    assert (got == want).all() and got[:5].sum() == n * K
    assert metrics.device_score(metrics.binaryf1, p, t) is None


def test_targets_outside_the_classes_are_wrong_not_invalid():
    from glass_amd import metrics
    pred = torch.tensor([[1., 0., 0.], [0., 1., 0.], [0., 0., 1.], [1., 0., 0.]], device=DEV)
    y = torch.tensor([0, 3, -1, 0], device=DEV)
    got = _f1_dev(pred, 3, y, 1, 4, 3, 0).cpu().numpy()
    assert list(got) == [2, 4, 0, 0, 0, 0, 0, 0]
    assert metrics.device_score(metrics.microf1, pred, y) == 0.5 == metrics.microf1(pred.cpu().numpy(), y.cpu().numpy())


# n on both sides of the row tile (256 lanes) and of the LDS tile of the pair sweep (1024 scores)
AUROC_NS = (2, 64, 65, 256, 257, 1023, 1024, 1025, 3000)


def _auroc_case(rng, n, K, kind):
    s = rng.standard_normal((n, K)).astype(np.float32)
    if kind == "rounded":
        s = np.round(s, 1)                    # heavy ties
    elif kind == "equal":
        s[:] = 0.25
    elif kind == "inf":
        s[rng.random((n, K)) < 0.2] = np.inf
        s[rng.random((n, K)) < 0.2] = -np.inf
    elif kind == "nan":
        s[rng.integers(0, n), :] = np.nan
    elif kind == "zeros":
        s = np.where(rng.random((n, K)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    y = (rng.random((n, K)) < 0.4).astype(np.float32)
    y[0], y[1] = 0.0, 1.0                     # both classes in every column: no case is skipped
    return s, y


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("kind", ["normal", "rounded", "equal", "inf", "nan", "zeros"])
def test_auroc_counters_equal_brute_force(kind, K):
    from glass_amd import metrics
    from sklearn.metrics import roc_auc_score
    rng = np.random.default_rng(4)
    for n in AUROC_NS:
        s, y = _auroc_case(rng, n, K, kind)
        for layout in ("contiguous", "strided") if n in (65, 1025) else ("contiguous", ):
            st, lds = _place(s, layout)
            yt, ldl = _place(y, layout)
            got = _auroc_dev(st, lds, yt, ldl, n, K).cpu().numpy()
            want = auroc_counts(s, y)
            assert (got == want).all(), (n, K, got, want)
            score = metrics.device_score(metrics.auroc, st, yt)
            if kind in ("inf", "nan"):   # scikit-learn refuses scores that are not finite: so does the device path
                assert want[:, 3].any() and score is None
                with pytest.raises(ValueError):
                    metrics.auroc(st, yt)
                continue
            assert not want[:, 3].any()
            ref = roc_auc_score(y[:, 0] if K == 1 else y, s[:, 0] if K == 1 else s)
            assert abs(score - ref) <= 1e-12 and abs(metrics.auroc(st, yt) - ref) <= 1e-12
            if kind in ("equal", "zeros"):
                assert score == 0.5


def _outcome(fn):
    """What a call answers: ("raise", exception type) or ("value", repr, warning categories)."""
    import warnings
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        try:
            value = fn()
        except Exception as e:  # noqa: BLE001
            return ("raise", type(e))
    return ("value", repr(float(value)), sorted({w.category.__name__ for w in caught}))


def test_auroc_one_class_column_goes_to_the_host():
    """A column with one class only: device_score declines, and metrics.auroc answers exactly as scikit-learn does on the
    host arrays — a ValueError in the releases that raise, UndefinedMetricWarning and NaN in those that warn."""
    from glass_amd import metrics
    from sklearn.metrics import roc_auc_score
    rng = np.random.default_rng(5)
    s = torch.from_numpy(rng.standard_normal((40, 3)).astype(np.float32)).to(DEV)
    y = torch.from_numpy((rng.random((40, 3)) < 0.5).astype(np.float32)).to(DEV)
    y[0], y[1] = 0.0, 1.0
    assert metrics.device_score(metrics.auroc, s, y) is not None
    y[:, 1] = 1.0
    c = _auroc_dev(s, 3, y, 3, 40, 3).cpu().numpy()
    assert c[1, 1] == 40 and c[1, 2] == 0 and c[1, 0] == 0
    assert metrics.device_score(metrics.auroc, s, y) is None
    host = _outcome(lambda: roc_auc_score(y.cpu().numpy(), s.cpu().numpy()))
    assert host[0] == "raise" or host[1] == "nan"           # no number either way
    assert _outcome(lambda: metrics.auroc(s, y)) == host
    # one column, 1-D labels and scores, as roc_auc_score takes them
    assert metrics.device_score(metrics.auroc, s[:, 0].contiguous(), y[:, 0].contiguous()) is not None
    s1, y1 = s[:, 1].contiguous(), y[:, 1].contiguous()
    assert metrics.device_score(metrics.auroc, s1, y1) is None
    host = _outcome(lambda: roc_auc_score(y1.cpu().numpy(), s1.cpu().numpy()))
    assert host[0] == "raise" or host[1] == "nan"
    assert _outcome(lambda: metrics.auroc(s1, y1)) == host


def test_device_scores_equal_the_host_functions():
    from glass_amd import metrics
    rng = np.random.default_rng(6)
    for n, K in ((160, 6), (1, 3), (300, 1), (257, 17), (64, 2)):
        pred = rng.integers(-2, 3, (n, K)).astype(np.float32) / 2
        y = rng.integers(0, K, n)
        p, t = torch.from_numpy(pred).to(DEV), torch.from_numpy(y).to(DEV)
        got = metrics.device_score(metrics.microf1, p, t)
        assert isinstance(got, np.float64) and got == metrics.microf1(pred, y) == metrics.microf1(p, t)
        yb = (rng.random((n, K)) < 0.4).astype(np.float32)
        yb[0, 0], pred[0, 0] = 1.0, 1.0
        p, t = torch.from_numpy(pred).to(DEV), torch.from_numpy(yb).to(DEV)
        got = metrics.device_score(metrics.binaryf1, p, t)
        assert isinstance(got, np.float64) and got == metrics.binaryf1(pred, yb) == metrics.binaryf1(p, t)
        if K == 1:   # the drivers' binary sets: labels [n] against logits [n, 1] — the accuracy
            assert metrics.device_score(metrics.binaryf1, p, t[:, 0].contiguous()) == got == ((pred > 0) == (yb == 1)).mean()
    # what the device path does not serve: other dtypes, a label count that does not match, another function
    p, t = torch.zeros(8, 3, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV)
    assert metrics.device_score(metrics.microf1, p.double(), t) is None
    assert metrics.device_score(metrics.microf1, p, t.int()) is None
    assert metrics.device_score(metrics.microf1, p, t[:7]) is None
    assert metrics.device_score(metrics.binaryf1, p, torch.zeros(8, 2, device=DEV)) is None
    assert metrics.device_score(metrics.binaryf1, p, torch.zeros(8, 3, dtype=torch.float64, device=DEV)) is None
    assert metrics.device_score(lambda a, b: 0.0, p, t) is None
    # no true and no predicted bit in two or more columns: scikit-learn's warning and its 0.0
    from sklearn.exceptions import UndefinedMetricWarning
    assert metrics.device_score(metrics.binaryf1, p - 1, torch.zeros(8, 3, device=DEV)) is None
    with pytest.warns(UndefinedMetricWarning):
        assert metrics.binaryf1(p - 1, torch.zeros(8, 3, device=DEV)) == 0.0


def test_counters_repeat_and_replay_from_a_captured_graph():
    rng = np.random.default_rng(7)
    n, K = 1000, 17
    pred = torch.from_numpy(rng.integers(-1, 2, (n, K)).astype(np.float32)).to(DEV)
    y = torch.from_numpy(rng.integers(0, K, n)).to(DEV)
    yb = torch.from_numpy((rng.random((n, K)) < 0.4).astype(np.float32)).to(DEV)
    calls = [lambda c: _f1_dev(pred, K, y, 1, n, K, 0, c), lambda c: _f1_dev(pred, K, yb, K, n, K, 1, c),
             lambda c: _f1_dev(pred[:, :3], K, yb[:, :3], K, n, 3, 1, c), lambda c: _auroc_dev(pred, K, yb, K, n, K, c)]
    for call in calls:
        a, b = call(None).clone(), call(None).clone()
        assert torch.equal(a, b) and int(a.sum()) > 0
        # captured: the zeroing is part of the captured work, so a second replay does not add to the first
        buf = torch.full_like(a, -5)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call(buf)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call(buf)
        for _ in range(2):
            buf.fill_(-5)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(buf, a)


# ---------------------------------------------------------------------------------------------------------------------
# train.test
# ---------------------------------------------------------------------------------------------------------------------
class _HostPathRan(Exception):
    pass


def _raise(*_a, **_k):
    raise _HostPathRan


def _check_train_test(monkeypatch, model, loader, metric, loss_fn):
    from glass_amd import metrics, train
    (pred, y), loss0 = train.test(model, loader, lambda p, t: (p, t), loss_fn)   # the host arrays a metric is handed
    want = metric(pred, y)
    monkeypatch.setattr(metrics, "f1_score", _raise)
    got, loss = train.test(model, loader, metric, loss_fn)    # scikit-learn would raise: the device path ran
    assert isinstance(got, np.float64) and got == want and torch.equal(loss, loss0)
    with pytest.raises(_HostPathRan):                          # a user function sees host arrays, as before
        train.test(model, loader, lambda p, t: metric(p, t), loss_fn)
    monkeypatch.setattr(train, "USE_EVAL_METRICS", False)      # GLASS_EVAL_METRICS=0
    with pytest.raises(_HostPathRan):
        train.test(model, loader, metric, loss_fn)
    return got


def test_train_test_scores_on_the_device_glass(monkeypatch):
    from glass_amd import synth
    from impl import SubGDataset, utils, metrics
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=1, n_batches=3)
    ds = SubGDataset.GDataset(*(torch.from_numpy(a) for a in (x, ei, ew, pos, y))).to(DEV)
    loader = SubGDataset.ZGDataloader(ds, w.batch, z_fn=utils.MaxZOZ, shuffle=False, drop_last=False)
    torch.manual_seed(0)
    model = build_glass(w.hidden, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio).to(DEV)
    score = _check_train_test(monkeypatch, model, loader, metrics.microf1, nn.CrossEntropyLoss())
    assert 0.0 <= score <= 1.0


def test_train_test_scores_on_the_device_glass_binary(monkeypatch):
    """A binary set as the drivers run it: one output column, float labels [n], BCE on the flattened tensors."""
    from glass_amd import synth
    from impl import SubGDataset, utils, metrics
    w, ei, ew, x, pos, y = synth.make_workload("tiny", seed=2, n_batches=3)
    yb = torch.from_numpy(y % 2).float()
    ds = SubGDataset.GDataset(*(torch.from_numpy(a) for a in (x, ei, ew, pos)), yb).to(DEV)
    loader = SubGDataset.ZGDataloader(ds, w.batch, z_fn=utils.MaxZOZ, shuffle=False, drop_last=False)
    torch.manual_seed(0)
    model = build_glass(w.hidden, w.layers, int(x.max()), 1, w.aggr, w.pool, w.z_ratio).to(DEV)

    def loss_fn(p, t):
        return nn.BCEWithLogitsLoss()(p.flatten(), t.flatten())

    score = _check_train_test(monkeypatch, model, loader, metrics.binaryf1, loss_fn)
    assert 0.0 <= score <= 1.0


def test_train_test_scores_on_the_device_gnn_seg(monkeypatch):
    import datasets
    from glass_amd import models, seg
    from impl import metrics
    torch.manual_seed(0)
    g = datasets.load_dataset("density")
    g.addOneFeature()
    _, ei, w, pos, y = g.get_split("test")
    ds = seg.GsDataset(g.x.to(DEV), ei.to(DEV), w.to(DEV), pos.to(DEV), y.long().to(DEV), mode="gin")
    loader = seg.GsDataloader(ds, max(len(ds) // 2, 1), shuffle=False, drop_last=False)
    n_out = int(y.max()) + 1
    torch.manual_seed(3)
    conv = seg.GConv(1, 16, 16, 1, conv=seg.MyGINConv, activation=nn.ELU(inplace=True), dropout=0.0)
    mlp = models.MLP(16, 16, n_out, 2, dropout=0.0, activation=nn.ELU(inplace=True))
    model = seg.GNN(conv, mlp).to(DEV)
    score = _check_train_test(monkeypatch, model, loader, metrics.microf1, nn.CrossEntropyLoss())
    assert 0.0 <= score <= 1.0
