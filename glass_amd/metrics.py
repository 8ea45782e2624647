"""Evaluation metrics with the reference's interface (/root/reference/impl/metrics.py:5-27).

numpy arrays take scikit-learn on the host, as the reference does.  fp32 / int64 torch tensors on the GPU take the device
path: glass_amd/csrc/evalmetrics.hip counts (exact integers: the micro-F1 cells, the Mann-Whitney pair count), the host
reads a few counters back and divides (device_score).  Whatever the device path does not serve — and every input that
scikit-learn answers with an exception or a warning — goes to the host functions below, unchanged."""
import numpy as np
from sklearn.metrics import f1_score, roc_auc_score


def _host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else a


def binaryf1(pred, label):
    """micro-F1 of (logit > 0) against binary / multi-label targets."""
    score = device_score(binaryf1, pred, label)
    if score is not None:
        return score
    pred, label = _host(pred), _host(label)
    return f1_score(label.reshape(pred.shape[0], -1), (pred > 0).astype(np.int64), average="micro")


def microf1(pred, label):
    """multi-class micro-F1 of argmax."""
    score = device_score(microf1, pred, label)
    if score is not None:
        return score
    pred, label = _host(pred), _host(label)
    return f1_score(label, np.argmax(pred, axis=1), average="micro")


def auroc(pred, label):
    score = device_score(auroc, pred, label)
    if score is not None:
        return score
    return roc_auc_score(_host(label), _host(pred))


# ---- scores from the integer counters (Python floats: one correctly rounded division each) ---------------------------------
def microf1_from_counts(correct, n):
    """Multi-class micro-F1 is the accuracy of the argmax."""
    return np.float64(int(correct) / int(n))


def binaryf1_from_counts(tp, fp, fn, tn, n_columns):
    """micro-F1 of the bits.  ONE column: scikit-learn reads an [n, 1] indicator as a plain binary target, whose micro
    average runs over both classes: the accuracy (tp + tn) / n.  Two or more columns: 2 tp / (2 tp + fp + fn) over all
    cells, 0.0 when nothing is true or predicted (scikit-learn's zero_division default)."""
    tp, fp, fn, tn = int(tp), int(fp), int(fn), int(tn)
    if n_columns == 1:
        return np.float64((tp + tn) / (tp + fp + fn + tn))
    den = 2 * tp + fp + fn
    return np.float64(2 * tp / den if den else 0.0)


def auroc_from_counts(counts):
    """counts [K, 4] = (twoU, P, N, invalid) per column: the unweighted mean over the columns of twoU / (2 P N) —
    scikit-learn's macro average for 2-D labels.  (Its trapezoid sum agrees to an ulp, not bitwise.)"""
    return np.float64(np.mean([int(u) / (2 * int(p) * int(q)) for u, p, q, _ in counts]))


def _rows(t, n, K):
    """t as [n, K] rows with unit column stride: (tensor, row stride), or None when its strides do not allow it."""
    t = t.detach().reshape(n, K)
    if (K > 1 and t.stride(1) != 1) or (n > 1 and t.stride(0) < K):
        return None
    return t, (t.stride(0) if n > 1 else K)


def device_score(fn, pred, y):
    """fn(pred, y) from counters taken on the GPU, as numpy.float64 — or None when the device path does not apply and the
    caller runs fn on the host: fn is not one of the three functions of this module; pred is not an fp32 tensor on the GPU;
    the target is not int64 [n] (microf1) / float32 with one element per prediction (binaryf1, auroc); sizes the entry
    points refuse; a target that is not 0 / 1, a NaN or infinite score for AUROC (invalid > 0); a column with one class only (auroc);
    no true and no predicted bit at all (binaryf1 with two or more columns).  The last three are the inputs scikit-learn
    answers with an exception or a warning: they come from there.  One host sync: the counter read-back."""
    import torch
    from . import _lib
    if fn not in (binaryf1, microf1, auroc):
        return None
    if not (isinstance(pred, torch.Tensor) and isinstance(y, torch.Tensor) and pred.is_cuda and y.device == pred.device and
            pred.dtype == torch.float32 and pred.dim() in (1, 2) and pred.shape[0] >= 1):
        return None
    n = pred.shape[0]
    K = pred.shape[1] if pred.dim() == 2 else 1
    if K < 1 or K > _lib.EVAL_MAX_K or (pred.dim() == 1 and fn is not auroc):
        return None
    if fn is microf1:
        if y.dtype != torch.int64 or y.dim() != 1 or y.shape[0] != n:
            return None
        t, ldt = (y.detach().contiguous(), 1)
    else:
        # binaryf1 reshapes the labels to [n, -1]; roc_auc_score takes [n] / [n, 1] against [n] / [n, 1], or equal 2-D shapes
        if y.dtype != torch.float32 or y.numel() != n * K or (fn is auroc and K > 1 and y.shape != pred.shape):
            return None
        rows = _rows(y, n, K)
        if rows is None:
            return None
        t, ldt = rows
    rows = _rows(pred, n, K)
    if rows is None:
        return None
    p, ldp = rows
    if n * max(ldp, ldt) * 4 >= 1 << 31:
        return None
    lib = _lib.load()
    stream = torch.cuda.current_stream(pred.device).cuda_stream
    with torch.cuda.device(pred.device):
        if fn is auroc:
            if not lib.glass_eval_auroc_supported(n, K):
                return None
            counts = torch.empty(K, 4, dtype=torch.int64, device=pred.device)
            _lib.check(lib.glass_eval_auroc_counts_f32(p.data_ptr(), ldp, t.data_ptr(), ldt, n, K, counts.data_ptr(), stream),
                       "glass_eval_auroc_counts_f32")
            c = counts.cpu().numpy()
            if c[:, 3].any() or not c[:, 1].all() or not c[:, 2].all():
                return None
            return auroc_from_counts(c)
        mode = 0 if fn is microf1 else 1
        counts = torch.empty(8, dtype=torch.int64, device=pred.device)
        _lib.check(lib.glass_eval_f1_counts_f32(p.data_ptr(), ldp, t.data_ptr(), ldt, n, K, mode, counts.data_ptr(), stream),
                   "glass_eval_f1_counts_f32")
        c = counts.cpu().numpy()
    if c[4]:
        return None
    if mode == 0:
        return microf1_from_counts(c[0], c[1])
    if K > 1 and 2 * c[0] + c[1] + c[2] == 0:
        return None  # scikit-learn warns (UndefinedMetricWarning) and returns 0.0: from there
    return binaryf1_from_counts(c[0], c[1], c[2], c[3], K)
