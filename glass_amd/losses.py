"""Losses the training step can fuse with the prediction head.

`CrossEntropy()` / `BCEWithLogits()` behave exactly like the losses the reference driver builds
(GLASSTest.py:57-58, 69) when called as `loss_fn(pred, y)`; in addition `glass_amd.step.TrainStep`
recognises them — and any callable that computes one of them, the reference driver's own lambda included (`fusable_mode`) —
and, when the model's head is a bare nn.Linear (GLASSTest.py:159-160), runs head + loss + their backward as two kernels
(`glass_head_loss_fwd/bwd_f32`) instead of ~12 launches.  The reference's other head, the two-layer `models.MLP` of GNN-seg
and GNNEmb (Linear -> Dropout -> activation -> Linear), is recognised by `fusable_head` and runs with its loss and their
backward as four launches (`mlp_head_loss`, `glass_head_mlp_loss_fwd/bwd_f32`); DESIGN.md has the launch counts measured
with and without it.  `CrossEntropy(weight=)` / `BCEWithLogits(pos_weight=)` carry class weights into the same launches
(`fusable_spec`, the `_w` entries of the C ABI; `balanced_weights` is the drivers' `--class_weight balanced`)."""
import torch
import torch.nn as nn

from . import _lib, ops


def _checked_weight(w, what):
    """A weight vector the kernels can take: a 1-D fp32 tensor, every value finite and > 0 (ValueError otherwise)."""
    if not (isinstance(w, torch.Tensor) and w.dim() == 1 and w.numel() > 0 and w.dtype == torch.float32):
        raise ValueError(f"{what}: a non-empty 1-D float32 tensor expected, got "
                         f"{tuple(w.shape)} {w.dtype}" if isinstance(w, torch.Tensor) else f"{what}: a tensor expected, got {type(w).__name__}")
    if not bool((torch.isfinite(w) & (w > 0)).all()):
        raise ValueError(f"{what}: every value must be finite and greater than 0")
    return w.detach().clone().contiguous()


class CrossEntropy(nn.Module):
    """CrossEntropyLoss(weight=weight), mean reduction.  weight (optional): one fp32 value per class, finite and > 0 — kept
    as a buffer (it follows .to(device)); the fused heads and the captured step read it on the device (`fusable_spec`)."""
    mode = 0

    def __init__(self, weight=None):
        super().__init__()
        self.register_buffer("weight", None if weight is None else _checked_weight(weight, "CrossEntropy(weight=)"))

    def forward(self, pred, y):
        return nn.functional.cross_entropy(pred, y, weight=self.weight)


class BCEWithLogits(nn.Module):
    """Binary / multi-label: BCEWithLogitsLoss(pos_weight=pos_weight)(pred.flatten(), y.flatten()) — pos_weight (optional):
    one fp32 value per output column, finite and > 0, kept as a buffer."""
    mode = 1

    def __init__(self, pos_weight=None):
        super().__init__()
        self.register_buffer("pos_weight",
                             None if pos_weight is None else _checked_weight(pos_weight, "BCEWithLogits(pos_weight=)"))

    def forward(self, pred, y):
        if self.pos_weight is None:
            return nn.functional.binary_cross_entropy_with_logits(pred.flatten(), y.flatten())
        # (one weight per output column: applied on [B, K], the mean over B*K elements as on the flattened tensors)
        K = self.pos_weight.numel()
        return nn.functional.binary_cross_entropy_with_logits(pred.reshape(-1, K), y.reshape(-1, K).to(pred.dtype),
                                                              pos_weight=self.pos_weight)


import os as _os
PROBE_OPAQUE_LOSSES = _os.environ.get("GLASS_LOSS_PROBE", "1") != "0"   # 0: never evaluate an opaque loss callable to classify it
_PROBE_TOL = 1e-6
_probed = {}  # id(loss_fn) -> (weakref or None, mode or None)


def _probe(loss_fn):
    """Decide by EVALUATION what an opaque callable computes: it is called on small seeded CPU logit / target pairs — value
    and gradient with respect to the logits must equal the fused head's cross-entropy (int64 class targets, mean reduction)
    or BCE-with-logits on the flattened tensors (float targets, mean reduction) to 1e-6 on every pair.  The reference's
    binary loss is such a callable: `lambda x, y: BCEWithLogitsLoss()(x.flatten(), y.flatten())` (GLASSTest.py:57-58).  The
    pairs have different row counts and class counts, every class occurs, so a sum reduction, class weights, label smoothing
    or a non-default ignore_index all fail the comparison.  Anything that raises is simply not fusable."""
    import torch.nn.functional as F
    gen = torch.Generator().manual_seed(20240613)

    def agree(logits, target, ref):
        try:
            x = logits.clone().requires_grad_(True)
            with torch.enable_grad():
                out = loss_fn(x, target)
            if not (isinstance(out, torch.Tensor) and out.dim() == 0 and out.dtype == torch.float32 and out.requires_grad):
                return False
            g, = torch.autograd.grad(out, x)
            xr = logits.clone().requires_grad_(True)
            with torch.enable_grad():
                want = ref(xr, target)
            gr, = torch.autograd.grad(want, xr)
            got, want = float(out.detach()), float(want.detach())
            return got == got and abs(got - want) <= _PROBE_TOL * max(1.0, abs(want)) and float((g - gr).abs().max()) <= _PROBE_TOL
        except Exception:  # noqa: BLE001 — a loss that cannot take these tensors is not one of the two
            return False

    def ce_pairs():
        for b, k in ((5, 3), (8, 6)):
            yield 3.0 * torch.randn(b, k, generator=gen), torch.arange(b) % k

    def bce_pairs():
        for shape, yshape in (((6, 1), (6, )), ((5, 4), (5, 4))):
            yield 3.0 * torch.randn(*shape, generator=gen), (torch.rand(*yshape, generator=gen) > 0.5).float()

    if all(agree(x, y, F.cross_entropy) for x, y in ce_pairs()):
        return 0
    if all(agree(x, y, lambda a, t: F.binary_cross_entropy_with_logits(a.flatten(), t.flatten())) for x, y in bce_pairs()):
        return 1
    return None


def fusable_mode(loss_fn):
    """0 (cross-entropy) / 1 (BCE with logits on the flattened tensors) when the training step can fuse this loss with the
    head, else None.  Recognised by type: this module's marker classes and torch's own CrossEntropyLoss with default settings
    (what the reference driver builds for multi-class sets, GLASSTest.py:69).  Any other callable — the reference's binary
    case is a lambda around BCEWithLogitsLoss (GLASSTest.py:57-58) — is recognised by what it computes (`_probe`, once per
    callable)."""
    if isinstance(loss_fn, (CrossEntropy, BCEWithLogits)):
        return loss_fn.mode  # (a marker's weights are `fusable_spec`'s business: every consumer asks that)
    if (type(loss_fn) is nn.CrossEntropyLoss and loss_fn.weight is None and loss_fn.reduction == "mean" and
            loss_fn.ignore_index == -100 and getattr(loss_fn, "label_smoothing", 0.0) == 0.0):
        return 0
    if not callable(loss_fn):
        return None
    # Opt-out: the probe CALLS the loss (<= 4 times, on small synthetic CPU tensors) — a stateful callable (running statistics,
    # logging, counters) sees those phantom calls, and one that equals CE / BCE at probe time but depends on state that changes
    # later would be replaced by the fused kernel for good.  `loss_fn._glass_no_fuse = True` (or GLASS_LOSS_PROBE=0 in the
    # environment) keeps such a callable on the plain path: it is then called as it is, once per step, by autograd.
    if getattr(loss_fn, "_glass_no_fuse", False) or not PROBE_OPAQUE_LOSSES:
        return None
    hit = _probed.get(id(loss_fn))
    if hit is not None and (hit[0] is None or hit[0]() is loss_fn):
        return hit[1]
    import weakref
    try:
        ref = weakref.ref(loss_fn)
    except TypeError:
        ref = None
    import warnings
    with warnings.catch_warnings():  # (a loss of another kind may warn about the probe's shapes: not the user's business)
        warnings.simplefilter("ignore")
        mode = _probe(loss_fn)
    if ref is not None:  # (no weak reference possible: the id could be reused by another object — probe again next time)
        if len(_probed) > 256:
            _probed.clear()
        _probed[id(loss_fn)] = (ref, mode)
    return mode


def fusable_spec(loss_fn):
    """(mode, class_weight, pos_weight) when the training step can fuse this loss with the head, else None — what every
    consumer asks (stack, step.TrainStep, head_loss / mlp_head_loss, the GNN-seg model): mode as `fusable_mode`, and the
    weight tensors of this module's marker classes (at most one of them set; None: unweighted).  Weights come from the
    marker classes ONLY: torch's own weighted losses and opaque callables around them stay None — the probe compares a
    callable with the unweighted losses, and no number of evaluations would tell which tensor object holds its weights, so
    the captured step could not follow them."""
    mode = fusable_mode(loss_fn)
    if mode is None:
        return None
    if isinstance(loss_fn, CrossEntropy):
        return mode, loss_fn.weight, None
    if isinstance(loss_fn, BCEWithLogits):
        return mode, None, loss_fn.pos_weight
    return mode, None, None


def on_device(loss_fn, device):
    """A marker loss whose weight buffer lives elsewhere is moved to `device` (in place, as nn.Module.to does): the fused
    kernels and the eager loss both read it there.  Anything else is returned as it is."""
    if isinstance(loss_fn, (CrossEntropy, BCEWithLogits)):
        w = loss_fn.weight if isinstance(loss_fn, CrossEntropy) else loss_fn.pos_weight
        if w is not None and w.device != torch.device(device):
            loss_fn.to(device)
    return loss_fn


def balanced_weights(y, n_class=None):
    """The `--class_weight balanced` vector of the drivers, from the TRAINING split's targets only (fp32, CPU).
    Multi-class (integer y [n]): w_k = n / (K * count_k), K = n_class (default max + 1) -> CrossEntropy(weight=).
    Binary / multi-label (floating y [n] or [n, K]): p_k = neg_k / pos_k per column -> BCEWithLogits(pos_weight=).
    A class or column with a zero count (no sample, or for p_k no positive or no negative) gets 1."""
    y = y.detach().cpu()
    if not y.is_floating_point():
        y = y.reshape(-1).to(torch.int64)
        K = int(n_class) if n_class is not None else int(y.max()) + 1
        count = torch.bincount(y[(y >= 0) & (y < K)], minlength=K).to(torch.float64)
        w = torch.where(count > 0, float(y.numel()) / (K * count.clamp(min=1.0)), torch.ones_like(count))
        return w.to(torch.float32)
    y2 = y.reshape(y.shape[0], -1).to(torch.float64)
    pos = (y2 > 0.5).sum(dim=0).to(torch.float64)
    neg = float(y2.shape[0]) - pos
    p = torch.where((pos > 0) & (neg > 0), neg / pos.clamp(min=1.0), torch.ones_like(pos))
    return p.to(torch.float32)


def balanced_loss(y_train, n_out):
    """The marker loss with `balanced_weights` of the training targets: CrossEntropy(weight=) over n_out classes for integer
    targets, BCEWithLogits(pos_weight=) for floating ones (binary / multi-label, n_out columns)."""
    if not y_train.is_floating_point():
        return CrossEntropy(weight=balanced_weights(y_train, n_out))
    return BCEWithLogits(pos_weight=balanced_weights(y_train))


def _spec(mode):
    """A consumer's `mode` argument: the plain mode number (unweighted) or a fusable_spec tuple."""
    return (mode, None, None) if isinstance(mode, int) else tuple(mode)


def weight_ptrs(spec, K, device):
    """(class_weight pointer, pos_weight pointer) of a spec for a head of K outputs on `device` (0: not set), checked before
    any launch: the length is K and the tensor is fp32, contiguous and on the device (ValueError otherwise)."""
    out = []
    for w, what in ((spec[1], "class weight"), (spec[2], "pos_weight")):
        if w is None:
            out.append(0)
            continue
        if w.dim() != 1 or w.numel() != K:
            raise ValueError(f"{what}: {w.numel()} values for a head of {K} outputs")
        if w.dtype != torch.float32 or not w.is_contiguous() or w.device != torch.device(device):
            raise ValueError(f"{what}: a contiguous float32 tensor on {device} expected (move the loss with .to(device)), "
                             f"got {w.dtype} on {w.device}")
        out.append(w.data_ptr())
    return tuple(out)


def _functional_loss(logits, target, spec):
    """torch's functional form of a spec (the module paths: sizes the kernels refuse, tensors not fp32 on the GPU)."""
    mode, cw, pw = spec
    if mode == 0:
        return nn.functional.cross_entropy(logits, target, weight=cw)
    if pw is None:
        return nn.functional.binary_cross_entropy_with_logits(logits.flatten(), target.flatten().to(logits.dtype))
    K = pw.numel()
    return nn.functional.binary_cross_entropy_with_logits(logits.reshape(-1, K), target.reshape(-1, K).to(logits.dtype),
                                                          pos_weight=pw)


class HeadLossFn(torch.autograd.Function):
    """loss = L(pooled @ W^T + b, target) — forward in one launch, backward in one launch."""
    @staticmethod
    def forward(ctx, pooled, weight, bias, target, mode, direct):
        ops._need_gpu(pooled, weight, target)
        pooled, ldp = ops._rows(pooled)
        B, C = pooled.shape
        K = weight.shape[0]
        spec = _spec(mode)
        mode = spec[0]
        wptrs = weight_ptrs(spec, K, pooled.device)
        w, b = weight.contiguous(), bias.contiguous()
        tgt = target.contiguous().to(torch.int64 if mode == 0 else torch.float32)
        logits = torch.empty((B, K), dtype=torch.float32, device=pooled.device)
        prob = torch.empty(B * K + B, dtype=torch.float32, device=pooled.device)  # probabilities + per-row loss terms
        loss = torch.empty((), dtype=torch.float32, device=pooled.device)
        rc = _lib.load().glass_head_loss_fwd_w_f32(pooled.data_ptr(), ldp, w.data_ptr(), b.data_ptr(), tgt.data_ptr(), mode,
                                                   B, C, K, logits.data_ptr(), prob.data_ptr(), loss.data_ptr(), *wptrs,
                                                   ops._stream())
        _lib.check(rc, "glass_head_loss_fwd_w_f32")
        ctx.save_for_backward(pooled, w, prob, tgt)
        ctx.cfg = (mode, B, C, K)
        ctx.wspec = spec  # (keeps the weight tensors alive until the backward has read them)
        # direct: accumulate dW / db straight into the flat gradient arena (weight.grad / bias.grad views)
        ctx.direct = (weight, bias) if (direct and weight.grad is not None and bias.grad is not None) else None
        ctx.mark_non_differentiable(logits)
        ctx.set_materialize_grads(False)  # no zero-filled gradient tensor for the logits output
        return loss, logits

    @staticmethod
    def backward(ctx, gl, _glogits):
        pooled, w, prob, tgt = ctx.saved_tensors
        mode, B, C, K = ctx.cfg
        gl = gl.contiguous().reshape(1).to(torch.float32)
        dpooled = torch.empty((B, C), dtype=torch.float32, device=pooled.device)
        if ctx.direct is not None:
            dW, db, acc = ctx.direct[0].grad, ctx.direct[1].grad, 1
        else:
            dW, db, acc = torch.empty_like(w), torch.empty(K, dtype=torch.float32, device=w.device), 0
        rc = _lib.load().glass_head_loss_bwd_w_f32(pooled.data_ptr(), pooled.stride(0), w.data_ptr(), prob.data_ptr(),
                                                   tgt.data_ptr(), mode, gl.data_ptr(), B, C, K, dpooled.data_ptr(), C,
                                                   dW.data_ptr(), db.data_ptr(), acc, *weight_ptrs(ctx.wspec, K, pooled.device),
                                                   ops._stream())
        _lib.check(rc, "glass_head_loss_bwd_w_f32")
        if ctx.direct is not None:
            return dpooled, None, None, None, None, None
        return dpooled, dW, db, None, None, None


def head_loss(pooled, linear, target, mode, direct=False):
    """-> (loss, logits) for an nn.Linear head; mode 0 = cross-entropy, 1 = BCE-with-logits — or a `fusable_spec` tuple,
    whose weights the kernels then apply (their length must be the head's K: ValueError before any launch)."""
    return HeadLossFn.apply(pooled, linear.weight, linear.bias, target, mode, direct)


# ---------------------------------------------------------------------------------------------------------------------
# The two-layer MLP head: MLP(in, hidden, out, 2, dropout, activation) = Linear -> Dropout -> activation -> Linear
# (reference impl/models.py:56-80), the head of GNN-seg (GNNSeg.py:272-277) and of GNNEmb.
# ---------------------------------------------------------------------------------------------------------------------
# Dropout streams (`call_id`) of the device-resident generator: 1 the embedding's GraphNorm, 2 the pair head (ssl.py),
# 16 (l + 1) [+ 1] the GraphNorm dropouts of conv layer l (models.EmbZGConv / EmbGConv) — and 3 this head's.
HEAD_MLP_CALL_ID = 3


def _mlp2_parts(pred):
    """(first Linear, dropout p, activation code, second Linear) of a fusable two-layer models.MLP, else None."""
    from .models import MLP, _act_code
    if type(pred) is not MLP:
        return None
    mods = list(pred.seq.modlist)
    p = 0.0
    if len(mods) == 4 and type(mods[1]) is nn.Dropout:  # (dropout == 0 builds no Dropout module: the Linear is modlist.2)
        p = float(mods[1].p)
        del mods[1]
    if len(mods) != 3 or not 0.0 <= p < 1.0:
        return None
    lin1, act, lin2 = mods
    code = _act_code(act)
    if not (isinstance(lin1, nn.Linear) and isinstance(lin2, nn.Linear) and lin1.bias is not None and
            lin2.bias is not None and code is not None and lin2.in_features == lin1.out_features):
        return None
    return lin1, p, code, lin2


def fusable_head(pred):
    """"linear": a bare nn.Linear with bias (GLASSTest.py:159-160) — head_loss; "mlp2": a models.MLP whose sequence is
    exactly [Linear, (Dropout)?, ELU | ReLU, Linear], both Linears with bias (no GraphNorm, no tail activation) —
    mlp_head_loss; None: anything else runs as the module."""
    if type(pred) is nn.Linear and pred.bias is not None:
        return "linear"
    return "mlp2" if _mlp2_parts(pred) is not None else None


class _HeadUnsupported(Exception):
    """The C entry refused the sizes (GLASS_E_UNSUPPORTED) before any launch: the caller runs the modules."""


class MLPHeadLossFn(torch.autograd.Function):
    """loss = L(act(dropout(pooled @ W1^T + b1)) @ W2^T + b2, target) — forward in two launches, backward in two.
    rng: the (seed, step) words this call's dropout reads, in the forward and again in the backward (None: no dropout)."""
    @staticmethod
    def forward(ctx, pooled, w1, b1, w2, b2, target, mode, act, p_drop, rng, direct):
        ops._need_gpu(pooled, w1, w2, target)
        pooled, ldp = ops._rows(pooled)
        B, C = pooled.shape
        Hd, K = w1.shape[0], w2.shape[0]
        spec = _spec(mode)
        mode = spec[0]
        wptrs = weight_ptrs(spec, K, pooled.device)
        if w1.shape[1] != C or w2.shape[1] != Hd or any(t.dtype != torch.float32 for t in (w1, b1, w2, b2)):
            raise _lib.GlassHipError(f"MLP head: fp32 weights [Hd,{C}] and [K,Hd] expected, got {tuple(w1.shape)} {w1.dtype}, "
                                     f"{tuple(w2.shape)} {w2.dtype}")
        params = (w1, b1, w2, b2)
        w1c, b1c, w2c, b2c = (t.contiguous() for t in params)
        tgt = target.contiguous().to(torch.int64 if mode == 0 else torch.float32)
        dev = pooled.device
        hidden = torch.empty((B, Hd), dtype=torch.float32, device=dev)
        logits = torch.empty((B, K), dtype=torch.float32, device=dev)
        prob = torch.empty(B * K + B, dtype=torch.float32, device=dev)  # probabilities + per-row loss terms
        loss = torch.empty((), dtype=torch.float32, device=dev)
        rc = _lib.load().glass_head_mlp_loss_fwd_w_f32(pooled.data_ptr(), ldp, w1c.data_ptr(), b1c.data_ptr(), w2c.data_ptr(),
                                                       b2c.data_ptr(), tgt.data_ptr(), mode, act, p_drop,
                                                       0 if rng is None else rng.data_ptr(), HEAD_MLP_CALL_ID, B, C, Hd, K,
                                                       hidden.data_ptr(), logits.data_ptr(), prob.data_ptr(), loss.data_ptr(),
                                                       *wptrs, ops._stream())
        if rc == -3:  # GLASS_E_UNSUPPORTED
            raise _HeadUnsupported(_lib.load().glass_last_error_string().decode(errors="replace"))
        _lib.check(rc, "glass_head_mlp_loss_fwd_w_f32")
        ctx.wspec = spec  # (keeps the weight tensors alive until the backward has read them)
        ctx.save_for_backward(pooled, w1c, w2c, hidden, prob, tgt)
        ctx.cfg = (mode, act, p_drop, B, C, Hd, K, ldp)
        ctx.rng = rng
        # direct: accumulate the four gradients straight into the flat gradient arena (the parameters' .grad views)
        ctx.direct = params if (direct and all(t.grad is not None for t in params)) else None
        ctx.mark_non_differentiable(logits)
        ctx.set_materialize_grads(False)  # no zero-filled gradient tensor for the logits output
        return loss, logits

    @staticmethod
    def backward(ctx, gl, _glogits):
        pooled, w1, w2, hidden, prob, tgt = ctx.saved_tensors
        mode, act, p_drop, B, C, Hd, K, ldp = ctx.cfg
        gl = gl.contiguous().reshape(1).to(torch.float32)
        dev = pooled.device
        dpooled = torch.empty((B, C), dtype=torch.float32, device=dev)
        ws = torch.empty(2 * B * Hd, dtype=torch.float32, device=dev)
        if ctx.direct is not None:
            grads, acc = [t.grad for t in ctx.direct], 1
        else:
            grads, acc = [torch.empty_like(w1), torch.empty(Hd, dtype=torch.float32, device=dev), torch.empty_like(w2),
                          torch.empty(K, dtype=torch.float32, device=dev)], 0
        rc = _lib.load().glass_head_mlp_loss_bwd_w_f32(pooled.data_ptr(), ldp, w1.data_ptr(), w2.data_ptr(),
                                                       hidden.data_ptr(), prob.data_ptr(), tgt.data_ptr(), mode, act, p_drop,
                                                       0 if ctx.rng is None else ctx.rng.data_ptr(), HEAD_MLP_CALL_ID,
                                                       gl.data_ptr(), B, C, Hd, K, ws.data_ptr(), dpooled.data_ptr(), C,
                                                       *(g.data_ptr() for g in grads), acc,
                                                       *weight_ptrs(ctx.wspec, K, pooled.device), ops._stream())
        _lib.check(rc, "glass_head_mlp_loss_bwd_w_f32")
        if ctx.direct is not None:
            return (dpooled, ) + (None, ) * 10
        return (dpooled, *grads) + (None, ) * 6


def mlp_head_loss(pooled, mlp, target, mode, direct=False):
    """-> (loss, logits) for a two-layer models.MLP head (fusable_head(mlp) == "mlp2"); mode 0 = cross-entropy, 1 =
    BCE-with-logits — or a `fusable_spec` tuple, whose weights every path below applies (length K, else ValueError before
    any launch).  In training with dropout the mask comes from the device-resident counter stream (stream
    HEAD_MLP_CALL_ID): this call reads a private snapshot of the (seed, step) words, in its forward and in its backward, and
    advances the live stream — a later training forward cannot pair this backward with another mask.  Same distribution as
    nn.Dropout's, other bits.  Sizes the kernels refuse (GLASS_E_UNSUPPORTED: more than 256 classes or 1024 hidden units) run
    as the modules, same semantics; so do tensors that are not fp32 on the GPU."""
    lin1, p, act, lin2 = _mlp2_parts(mlp)
    p = p if mlp.training else 0.0
    spec = _spec(mode)
    for w, what in ((spec[1], "class weight"), (spec[2], "pos_weight")):
        if w is not None and w.numel() != lin2.out_features:
            raise ValueError(f"{what}: {w.numel()} values for a head of {lin2.out_features} outputs")

    def modules():
        logits = mlp(pooled)
        return _functional_loss(logits, target, spec), logits

    params = (lin1.weight, lin1.bias, lin2.weight, lin2.bias)
    # the kernels are fp32 on the GPU: anything else (a half / double model, a CPU tensor) is the modules' business, as before
    if not (pooled.is_cuda and pooled.dim() == 2 and all(t.dtype == torch.float32 and t.is_cuda for t in (pooled, ) + params)):
        return modules()
    # the words are copied BEFORE the stream advances, and it advances only after the entry accepted the call: a refused call
    # leaves the stream alone.  (The first mask after ops.rng_seed is therefore drawn at step word 0.)
    rng = ops.rng_snapshot(pooled.device) if p > 0 else None
    try:
        out = MLPHeadLossFn.apply(pooled, *params, target, spec, act, p, rng, direct)
    except _HeadUnsupported:
        return modules()
    if rng is not None:
        ops.rng_advance(pooled.device)  # the next training forward draws another mask
    return out
