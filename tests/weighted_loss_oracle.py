"""fp64 restatement of the class-weighted losses the fused heads and the training readout compute (head_loss.h, readout.hip):
value and d loss / d logits, written from the formulas and pinned on the CPU (tests/test_weighted_loss_host.py) against
torch.nn.functional.cross_entropy(weight=) and binary_cross_entropy_with_logits(pos_weight=) in fp64.

  cross-entropy, class weights w[K]:   loss = sum_b w[t_b] (lse_b - z_b[t_b]) / sum_b w[t_b]
                                       dlogits[b, k] = gl w[t_b] / sum_w (softmax_bk - [k = t_b])
                                       a target outside [0, K) adds nothing to either sum and has no gradient
  BCE with logits, pos_weight p[K]:    c = 1 + (p_k - 1) y;  term = (1 - y) z + c (log1p(exp(-|z|)) + max(-z, 0))
                                       d/dz = c sigmoid(z) - p_k y;  mean over B*K
The value functions are plain differentiable torch expressions: a test that needs gradients further up (head weights, the
GraphNorm input) lets autograd carry dlogits there, in fp64."""
import torch


def ce_weighted(logits, target, w=None):
    """-> loss (0-dim, differentiable in logits).  w None: all ones."""
    z = logits.double()
    B, K = z.shape
    t = target.to(torch.int64).reshape(B)
    w = torch.ones(K, dtype=torch.float64) if w is None else w.double()
    valid = (t >= 0) & (t < K)
    tc = t.clamp(0, K - 1)
    wt = torch.where(valid, w[tc], torch.zeros((), dtype=torch.float64))
    lse = torch.logsumexp(z, dim=1)
    return (wt * (lse - z.gather(1, tc.reshape(-1, 1)).reshape(-1))).sum() / wt.sum()


def ce_weighted_dlogits(logits, target, w=None, gl=1.0):
    z = logits.double()
    B, K = z.shape
    t = target.to(torch.int64).reshape(B)
    w = torch.ones(K, dtype=torch.float64) if w is None else w.double()
    valid = (t >= 0) & (t < K)
    tc = t.clamp(0, K - 1)
    wt = torch.where(valid, w[tc], torch.zeros((), dtype=torch.float64))
    onehot = torch.nn.functional.one_hot(tc, K).double() * valid.reshape(-1, 1)
    return gl * (wt / wt.sum()).reshape(-1, 1) * (torch.softmax(z, dim=1) - onehot)


def bce_pos_weighted(logits, y, p=None):
    """-> loss (0-dim, differentiable in logits); logits [B, K], y [B, K] (or [B] for K = 1).  p None: all ones."""
    z = logits.double()
    B, K = z.shape
    y = y.double().reshape(B, K)
    p = torch.ones(K, dtype=torch.float64) if p is None else p.double()
    c = 1.0 + (p - 1.0) * y
    return ((1.0 - y) * z + c * (torch.log1p(torch.exp(-z.abs())) + (-z).clamp(min=0))).mean()


def bce_pos_weighted_dlogits(logits, y, p=None, gl=1.0):
    z = logits.double()
    B, K = z.shape
    y = y.double().reshape(B, K)
    p = torch.ones(K, dtype=torch.float64) if p is None else p.double()
    return gl * ((1.0 + (p - 1.0) * y) * torch.sigmoid(z) - p * y) / (B * K)


def loss(logits, target, mode, cw=None, pw=None):
    """mode 0: ce_weighted(cw); mode 1: bce_pos_weighted(pw)."""
    return ce_weighted(logits, target, cw) if mode == 0 else bce_pos_weighted(logits, target, pw)


def dlogits(logits, target, mode, cw=None, pw=None, gl=1.0):
    return ce_weighted_dlogits(logits, target, cw, gl) if mode == 0 else bce_pos_weighted_dlogits(logits, target, pw, gl)
