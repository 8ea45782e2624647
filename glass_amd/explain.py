"""Which edges made a prediction: gradients of a GLASS model's output with respect to the edge weights (edge saliency) and a
small GNNExplainer-style learned edge mask.  Both rest on ops.spmm_w (K1w, csrc/spmm_edge.hip): aggr "sum", "mean" and "gcn"
only, one label vector per batch (no exact zero-one replicas).  The model runs as per-op autograd nodes here, never as the
stack program.  **Not timed.**"""
import torch
import torch.nn.functional as F

from . import models
from ._lib import GlassHipError


def live_copy(model):
    """A GLASS model with live edge weights (GLASSConv.live_edge_weight) around the SAME parameters as `model`: the copy's
    modules are new objects, its parameters and buffers are the model's own tensors (shared storage, nothing is retrained,
    training either trains both), and the layers' adjacency structure is shared once built.  An arena, captured graphs and
    the other runtime attachments of `model` are not carried over: the copy runs per-op."""
    from .arena import _RUNTIME_ATTRS
    if not isinstance(model, models.GLASS):
        raise GlassHipError(f"live_copy: expected a models.GLASS, got {type(model).__name__}")

    def clone(m):
        """a new module object per module: its own containers, the same tensors and plain attributes (`adj` among them)"""
        new = m.__class__.__new__(m.__class__)
        for k, v in m.__dict__.items():
            if k not in _RUNTIME_ATTRS:   # (runtime attachments hold device pointers of the original's launches: left behind)
                new.__dict__[k] = v.copy() if isinstance(v, dict) else v
        new.__dict__["_modules"] = {k: (None if c is None else clone(c)) for k, c in m._modules.items()}
        return new

    new = clone(model)
    models.set_live_edge_weight(new.conv)
    return new


def _live(model):
    convs = getattr(getattr(model, "conv", None), "convs", ())
    if len(convs) and all(getattr(c, "live_edge_weight", False) for c in convs):
        return model
    return live_copy(model)


def _check_weights(edge_index, edge_weight):
    if (not isinstance(edge_weight, torch.Tensor) or edge_weight.dim() != 1 or edge_weight.shape[0] != edge_index.shape[1] or
            not edge_weight.is_cuda):
        raise ValueError(f"edge_weight: one weight per edge ({edge_index.shape[1]}) on the GPU")


def edge_saliency(model, x, edge_index, edge_weight, pos, z=None, target=None, loss_fn=None, y=None):
    """[E] fp32: the gradient, in eval mode, with respect to edge_weight of the batch's summed target logit — column `target`
    of model(x, edge_index, edge_weight, pos, z) where given, else every subgraph's argmax column (column 0 of a single
    output) — or, with loss_fn and y, of loss_fn(logits, y).  `model`: a GLASS built with live_edge_weight=True, or an
    ordinary one with aggr "sum" / "mean" / "gcn" (a live_copy of it is differentiated; the model itself is not touched)."""
    _check_weights(edge_index, edge_weight)
    if (loss_fn is None) != (y is None):
        raise ValueError("edge_saliency: loss_fn and y go together")
    live = _live(model)
    was_training = live.training
    live.eval()
    try:
        w = edge_weight.detach().to(torch.float32).clone().requires_grad_()
        with torch.enable_grad():
            logits = live(x, edge_index, w, pos, z)
            if loss_fn is not None:
                out = loss_fn(logits, y)
            elif target is not None:
                out = logits[:, int(target)].sum()
            elif logits.shape[1] == 1:
                out = logits[:, 0].sum()
            else:
                out = logits.gather(1, logits.detach().argmax(dim=1, keepdim=True)).sum()
            (g, ) = torch.autograd.grad(out, w)
    finally:
        live.train(was_training)
    return g


def learn_edge_mask(model, batch, steps=100, lr=0.05, l1=0.05, seed=0, return_losses=False):
    """A GNNExplainer-style edge mask for one batch (x, edge_index, edge_weight, pos, z[, y]; y is not used): mask logits
    theta [E] drawn N(0, 0.1) from `seed`, w = edge_weight * sigmoid(theta); `steps` Adam steps on theta alone (the model is
    frozen, eval mode) on the loss against the model's OWN prediction at the unmasked weights — cross-entropy with its argmax
    class, binary cross-entropy with its thresholded logits for a single output — plus l1 * mean(sigmoid(theta)).  Returns
    sigmoid(theta) [E] (with return_losses: also the list of the prediction-loss term, one per step)."""
    x, edge_index, edge_weight, pos, z = batch[:5]
    _check_weights(edge_index, edge_weight)
    live = _live(model)
    was_training = live.training
    live.eval()
    params = list(live.parameters())
    frozen = [p.requires_grad for p in params]
    w0 = edge_weight.detach().to(torch.float32)
    gen = torch.Generator().manual_seed(int(seed))
    theta = (0.1 * torch.randn(w0.shape[0], generator=gen)).to(w0.device).requires_grad_()
    opt = torch.optim.Adam([theta], lr=lr)
    losses = []
    try:
        for p in params:
            p.requires_grad_(False)
        with torch.no_grad():
            ref = live(x, edge_index, w0, pos, z)
            want = (ref > 0).to(torch.float32) if ref.shape[1] == 1 else ref.argmax(dim=1)
        for _ in range(int(steps)):
            opt.zero_grad()
            with torch.enable_grad():
                m = torch.sigmoid(theta)
                logits = live(x, edge_index, w0 * m, pos, z)
                fit = F.binary_cross_entropy_with_logits(logits, want) if ref.shape[1] == 1 else F.cross_entropy(logits, want)
                (fit + l1 * m.mean()).backward()
            losses.append(float(fit.detach()))
            opt.step()
    finally:
        for p, r in zip(params, frozen):
            p.requires_grad_(r)
        live.train(was_training)
    mask = torch.sigmoid(theta.detach())
    return (mask, losses) if return_losses else mask
