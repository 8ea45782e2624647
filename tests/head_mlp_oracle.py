"""fp64 restatement of the two-layer MLP prediction head and its loss (reference impl/models.py:56-80: Linear -> Dropout ->
activation -> Linear; the losses of GLASSTest.py:57-58, 69): plain torch CPU ops, gradients from autograd.  The dropout's
keep-scales (0 or 1 / (1 - p) per hidden element) are an explicit argument, so a test hands over the very mask the device
stream drew."""
import torch
import torch.nn.functional as F

ACT_NONE, ACT_ELU, ACT_RELU = 0, 1, 2


def head(pooled, W1, b1, W2, b2, keep, act):
    """logits [B, K] of the head; keep: [B, Hd] scales, or None for no dropout."""
    h = pooled @ W1.t() + b1
    if keep is not None:
        h = h * keep
    if act == ACT_ELU:
        h = F.elu(h)
    elif act == ACT_RELU:
        h = F.relu(h)
    elif act != ACT_NONE:
        raise ValueError(f"activation code {act}")
    return h @ W2.t() + b2


def loss_of(logits, target, mode):
    """mode 0: cross-entropy over int64 class targets; 1: BCE-with-logits on the flattened tensors; mean reduction."""
    if mode == 0:
        return F.cross_entropy(logits, target)
    return F.binary_cross_entropy_with_logits(logits.flatten(), target.flatten().to(logits.dtype))


def run(pooled, W1, b1, W2, b2, target, mode, act, keep=None):
    """-> dict(logits, loss, dpooled, grads = flat [dW1, db1, dW2, db2]) in fp64."""
    leaves = [t.detach().double().cpu().clone().requires_grad_(True) for t in (pooled, W1, b1, W2, b2)]
    tgt = target.detach().cpu()
    k = None if keep is None else keep.detach().double().cpu()
    logits = head(*leaves, k, act)
    loss = loss_of(logits, tgt if mode == 0 else tgt.double(), mode)
    g = torch.autograd.grad(loss, leaves)
    return {"logits": logits.detach(), "loss": loss.detach(), "dpooled": g[0],
            "grads": torch.cat([t.reshape(-1) for t in g[1:]])}
