"""fp64 restatement of K9, the link-prediction head of the pre-training path (glass_pair_head_{fwd,bwd}_f32; reference
EdgeGNN.Pool + MLP(hidden, hidden, 1, 2) + BCEWithLogitsLoss, impl/models.py:497-509, 33-50, GNNEmb.py:129-130):

    pooled[p] = (emb[pairs[p,0]] + emb[pairs[p,1]]) / 2      an id outside [0, N) gathers a ZERO row, the mean still
                                                             divides by 2 (include/glass_hip.h, K9)
    hid[p]    = relu(dropout(pooled[p] W0^T + b0))           Linear -> Dropout -> ReLU
    logit[p]  = hid[p] . w1 + b1
    loss      = mean_p BCE-with-logits(logit[p], target[p])
    dlogit    = grad_scale * d loss / d logit                the seed of the backward; every gradient carries grad_scale,
                                                             the loss does not

in plain torch ops with autograd, nothing closed-form.  The dropout is given as keep-scales (0 or 1 / (1 - p), [P, hidden]),
the ReLU optionally as the 0 / 1 mask of the branches to take (ReLU is not differentiable at 0: a comparison with an fp32
evaluation is made on the branches that evaluation took).

Pinned on the CPU (tests/test_pair_head_host.py) against oracle.glass_oracle.OracleEdgeGNN's head + nn.BCEWithLogitsLoss."""
import torch


def pair_head(emb, pairs, W0, b0, w1, b1, target, scales=None, relu_mask=None, grad_scale=1.0, dtype=torch.float64):
    """Everything on the CPU in `dtype` (fp64: the reference; fp32: the rounding floor of the same statement).
    Returns a dict: hid, logits, loss, dlogit, dW0, db0, dw1, db1, demb (tensors of `dtype`, loss 0-d)."""
    emb, W0, b0, w1, b1 = (t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in (emb, W0, b0, w1, b1))
    pairs = pairs.detach().cpu().to(torch.int64)
    target = target.detach().cpu().to(dtype).reshape(-1)
    n = emb.shape[0]
    valid = (pairs >= 0) & (pairs < n)
    rows = emb[pairs.clamp(0, n - 1)] * valid.to(dtype).unsqueeze(-1)   # [P, 2, H]; an invalid id: a zero row
    pooled = rows.sum(dim=1) / 2
    pre = pooled @ W0.t() + b0
    if scales is not None:
        pre = pre * scales.detach().cpu().to(dtype)
    hid = pre * relu_mask.detach().cpu().to(dtype) if relu_mask is not None else torch.relu(pre)
    logits = hid @ w1.reshape(-1) + b1.reshape(())
    logits.retain_grad()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, target)
    loss.backward(torch.tensor(float(grad_scale), dtype=dtype))
    return dict(hid=hid.detach(), logits=logits.detach(), loss=loss.detach(), dlogit=logits.grad, dW0=W0.grad, db0=b0.grad,
                dw1=w1.grad, db1=b1.grad, demb=emb.grad)
