"""Host side of the evaluation metrics on the GPU (glass_amd/csrc/evalmetrics.hip, glass_amd/metrics.py) — no GPU needed:
the three entry points exist and refuse bad arguments with codes before any HIP call, and the count-to-score formulas give
scikit-learn's numbers from counters taken by the numpy restatement of tests/metrics_counts.py.

Bounds.  Both F1 forms are one division of two integers below 2^53, which is what scikit-learn's own arithmetic reduces
to: compared with ==.  AUROC = twoU / (2 P N) is the exact Mann-Whitney ratio rounded once; scikit-learn sums trapezoids
in fp64 (an ulp or so away): |difference| <= 1e-12."""
import os
import sys
import warnings

import numpy as np
import pytest
from sklearn.exceptions import UndefinedMetricWarning
from sklearn.metrics import f1_score, roc_auc_score

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from metrics_counts import auroc_counts, f1_counts  # noqa: E402

E_ARG, E_UNSUPPORTED = -1, -3


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from glass_amd import _lib
    lib = _lib.load()
    x = np.zeros(4096, dtype=np.float32)
    c = np.zeros(4 * 256, dtype=np.int64)
    p, q = x.ctypes.data, c.ctypes.data
    f1, au = lib.glass_eval_f1_counts_f32, lib.glass_eval_auroc_counts_f32
    for mode in (0, 1):
        assert f1(None, 4, p, 4, 8, 4, mode, q, None) == E_ARG
        assert f1(p, 4, None, 4, 8, 4, mode, q, None) == E_ARG
        assert f1(p, 4, p, 4, 8, 4, mode, None, None) == E_ARG
        assert f1(p, 4, p, 4, 0, 4, mode, q, None) == E_ARG            # n = 0
        assert f1(p, 4, p, 4, 8, 0, mode, q, None) == E_ARG            # K = 0
        assert f1(p, 257, p, 257, 8, 257, mode, q, None) == E_UNSUPPORTED  # K = 257
        assert f1(p, 3, p, 4, 8, 4, mode, q, None) == E_ARG            # ldp < K
        assert f1(p, 1 << 20, p, 4, 512, 4, mode, q, None) == E_UNSUPPORTED   # n * ldp * 4 = 2^31
    assert f1(p, 4, p, 3, 8, 4, 1, q, None) == E_ARG                   # ldt < K (mode 1 reads target rows)
    assert b"eval_f1_counts" in lib.glass_last_error_string()
    assert f1(p, 4, p, 4, 8, 4, 2, q, None) == E_UNSUPPORTED and f1(p, 4, p, 4, 8, 4, -1, q, None) == E_UNSUPPORTED
    assert b"unknown mode" in lib.glass_last_error_string()
    assert au(None, 4, p, 4, 8, 4, q, None) == E_ARG and au(p, 4, None, 4, 8, 4, q, None) == E_ARG
    assert au(p, 4, p, 4, 8, 4, None, None) == E_ARG
    assert au(p, 4, p, 4, 0, 4, q, None) == E_ARG and au(p, 4, p, 4, 8, 0, q, None) == E_ARG
    assert au(p, 3, p, 4, 8, 4, q, None) == E_ARG and au(p, 4, p, 3, 8, 4, q, None) == E_ARG
    assert au(p, 257, p, 257, 8, 257, q, None) == E_UNSUPPORTED
    assert au(p, 1, p, 1, 65537, 1, q, None) == E_UNSUPPORTED
    assert b"eval_auroc_counts" in lib.glass_last_error_string()
    sup = lib.glass_eval_auroc_supported
    assert sup(65536, 1) == 1 and sup(65537, 1) == 0 and sup(1, 256) == 1 and sup(8, 257) == 0
    assert sup(0, 1) == 0 and sup(8, 0) == 0
    # the threshold between the lane-per-row and the wave-per-row kernels is a named constant of the header
    header = open(os.path.join(os.path.dirname(HERE), "include", "glass_hip.h")).read()
    assert f"#define GLASS_EVAL_F1_LANE_K {_lib.EVAL_F1_LANE_K}\n" in header
    for cite in ("impl/metrics.py:5-12", "impl/metrics.py:15-20", "impl/metrics.py:23-27"):
        assert cite in header


def test_functions_keep_their_identity_and_numpy_results():
    import impl.metrics
    from glass_amd import metrics
    assert impl.metrics.binaryf1 is metrics.binaryf1 and impl.metrics.microf1 is metrics.microf1
    assert impl.metrics.auroc is metrics.auroc
    g = np.load(os.path.join(HERE, "golden", "g7_metrics.npz"))
    assert metrics.binaryf1(g["pred_b"], g["lab_b"]) == float(g["f1_b"])
    assert metrics.microf1(g["pred_m"], g["lab_m"]) == float(g["f1_m"])
    # the golden vectors through the counters
    c = f1_counts(g["pred_b"], g["lab_b"], 1)
    assert metrics.binaryf1_from_counts(*c[:4], 4) == float(g["f1_b"])
    c = f1_counts(g["pred_m"], g["lab_m"], 0)
    assert metrics.microf1_from_counts(c[0], c[1]) == float(g["f1_m"])


def test_device_score_does_not_apply_to_host_inputs():
    import torch
    from glass_amd import metrics
    pred, y = np.zeros((4, 3), dtype=np.float32), np.arange(4) % 3
    assert metrics.device_score(metrics.microf1, pred, y) is None
    assert metrics.device_score(metrics.microf1, torch.from_numpy(pred), torch.from_numpy(y)) is None   # CPU tensors
    assert metrics.device_score(lambda p, t: 0.0, pred, y) is None
    # CPU tensors still score, on the host
    assert metrics.microf1(torch.from_numpy(pred), torch.from_numpy(y)) == metrics.microf1(pred, y)


def _quantised(rng, shape, levels):
    return rng.integers(-levels, levels + 1, shape).astype(np.float32) / np.float32(levels)


@pytest.mark.parametrize("K", [1, 2, 3, 6, 17])
def test_microf1_formula_equals_sklearn(K):
    from glass_amd import metrics
    rng = np.random.default_rng(100 + K)
    for trial in range(40):
        n = int(rng.integers(1, 200))
        pred = _quantised(rng, (n, K), 1) if trial % 2 else rng.standard_normal((n, K)).astype(np.float32)  # ties
        y = rng.integers(0, K + (trial % 3 == 0), n)   # every third trial: some targets outside [0, K)
        c = f1_counts(pred, y, 0)
        assert c[1] == n and c[4] == 0
        assert metrics.microf1_from_counts(c[0], c[1]) == f1_score(y, np.argmax(pred, axis=1), average="micro")


@pytest.mark.parametrize("K", [1, 2, 3, 6, 17])
def test_binaryf1_formula_equals_sklearn(K):
    """K = 1: scikit-learn reads the [n, 1] indicator as a binary target — micro-F1 is the accuracy."""
    from glass_amd import metrics
    rng = np.random.default_rng(200 + K)
    for trial in range(40):
        n = int(rng.integers(2, 200))
        pred = _quantised(rng, (n, K), 1) if trial % 2 else rng.standard_normal((n, K)).astype(np.float32)
        y = (rng.random((n, K)) < rng.random()).astype(np.float32)
        if K > 1:
            y[0, 0], pred[0, 0] = 1.0, 1.0   # (a true positive: the denominator is not zero; that case has its own test)
        c = f1_counts(pred, y, 1)
        assert c[:4].sum() == n * K and c[4] == 0
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            want = f1_score(y.reshape(n, -1), (pred > 0).astype(np.int64), average="micro")
        assert metrics.binaryf1_from_counts(*c[:4], K) == want


def test_single_column_is_accuracy_not_f1_of_the_positive_class():
    from glass_amd import metrics
    y, pred = np.array([[1.], [0.], [1.]], dtype=np.float32), np.array([[1.], [1.], [-1.]], dtype=np.float32)
    c = f1_counts(pred, y, 1)
    assert list(c[:4]) == [1, 1, 1, 0]
    got = metrics.binaryf1_from_counts(*c[:4], 1)
    assert got == 1 / 3 == metrics.binaryf1(pred, y)   # (the F1 of class 1 alone would be 0.5)


def test_zero_denominator_with_two_or_more_columns_is_zero_as_sklearn_warns():
    from glass_amd import metrics
    pred, y = -np.ones((5, 3), dtype=np.float32), np.zeros((5, 3), dtype=np.float32)
    c = f1_counts(pred, y, 1)
    assert list(c[:5]) == [0, 0, 0, 15, 0]
    with pytest.warns(UndefinedMetricWarning):
        want = metrics.binaryf1(pred, y)
    assert metrics.binaryf1_from_counts(*c[:4], 3) == want == 0.0


@pytest.mark.parametrize("K", [1, 3])
def test_auroc_formula_matches_sklearn(K):
    from glass_amd import metrics
    rng = np.random.default_rng(300 + K)
    for trial in range(30):
        n = int(rng.integers(2, 300))
        s = rng.standard_normal((n, K)).astype(np.float32)
        if trial % 3 == 1:
            s = np.round(s, 1)            # heavy ties
        elif trial % 3 == 2:
            s[:] = 0.25                   # all equal: exactly 0.5
        y = (rng.random((n, K)) < 0.4).astype(np.float32)
        y[0], y[1] = 0.0, 1.0             # both classes in every column: no case is skipped
        c = auroc_counts(s, y)
        assert (c[:, 1] + c[:, 2] == n).all() and not c[:, 3].any()
        got = metrics.auroc_from_counts(c)
        want = roc_auc_score(y[:, 0] if K == 1 else y, s[:, 0] if K == 1 else s)
        assert abs(got - want) <= 1e-12
        if trial % 3 == 2:
            assert got == 0.5
    # -0.0 ties with +0.0
    s = np.array([-0.0, 0.0, 2.0, -3.0, 2.0, 1.0], dtype=np.float32)
    y = np.array([1, 0, 1, 0, 0, 1], dtype=np.float32)
    c = auroc_counts(s, y)
    assert list(c[0]) == [2 * 5 + 2, 3, 3, 0]
    assert abs(metrics.auroc_from_counts(c) - roc_auc_score(y, s)) <= 1e-12
    # infinities order like numbers in the pair count, but scikit-learn refuses them (as it does a NaN): counted invalid
    s[2], s[3], s[4] = np.inf, -np.inf, np.inf
    assert list(auroc_counts(s, y)[0]) == [2 * 5 + 2, 3, 3, 3]
    with pytest.raises(ValueError):
        roc_auc_score(y, s)
