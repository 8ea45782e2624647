"""numpy restatement of the integer counters glass_amd/csrc/evalmetrics.hip takes (include/glass_hip.h, K11), shared by
tests/test_metrics_device_host.py (formulas against scikit-learn) and tests/test_gpu_metrics.py (the device counters)."""
import numpy as np


def f1_counts(pred, target, mode):
    """int64[8] as glass_eval_f1_counts_f32 fills it.  mode 0: pred [n, K], target int64 [n] -> {correct, n};
    mode 1: target float [n, K] -> {tp, fp, fn, tn, invalid}."""
    c = np.zeros(8, dtype=np.int64)
    if mode == 0:
        c[0] = int((np.argmax(pred, axis=1) == target).sum())   # numpy's argmax: lowest index among equals, first NaN wins
        c[1] = pred.shape[0]
        return c
    target = target.reshape(pred.shape)
    bit, pos, neg = pred > 0, target == 1, target == 0
    c[:5] = [(bit & pos).sum(), (bit & neg).sum(), (~bit & pos).sum(), (~bit & neg).sum(), (~pos & ~neg).sum()]
    return c


def auroc_counts(score, label):
    """int64[K, 4] = {twoU, P, N, invalid} per column, by brute force over all (label 1, label 0) pairs; invalid = scores
    that are not finite and labels that are neither 0 nor 1."""
    score, label = score.reshape(score.shape[0], -1), label.reshape(label.shape[0], -1)
    out = np.zeros((score.shape[1], 4), dtype=np.int64)
    for k in range(score.shape[1]):
        s, y = score[:, k], label[:, k]
        pos, neg = y == 1, y == 0
        with np.errstate(invalid="ignore"):
            sp, sn = s[pos][:, None], s[neg][None, :]
            out[k] = [2 * int((sp > sn).sum()) + int((sp == sn).sum()), pos.sum(), neg.sum(),
                      (~np.isfinite(s) | ~(pos | neg)).sum()]
    return out
