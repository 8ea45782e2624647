"""fp64 restatement of the max-pooling training readout (glass_readout_max_train_f32): final GraphNorm (PyG GraphNorm
with batch=None, reference impl/models.py:266/271) -> MaxPool over the rows of the padded node matrix (impl/models.py:300-303,
346-350) -> Linear head (GLASSTest.py:159-160) -> CrossEntropyLoss (:69) / BCEWithLogitsLoss on the flattened logits (:57-58),
and the whole backward to the GraphNorm INPUT in closed form, with the project's max semantics spelled out:

  * the max is over the GraphNorm OUTPUT y = gamma * xhat + beta (gamma may be negative);
  * strict compare walking the row's positions s upwards: on a tie the LOWEST position wins, so a node listed twice counts
    at its first position only;
  * padding (-1) and out-of-range ids are skipped; an empty row pools to 0 and gets no gradient.

Pinned on the CPU (tests/test_readout_max_host.py) against oracle.glass_oracle (GraphNorm + segment_pool(..., "max")) plus
autograd on inputs without ties."""
import torch


def graphnorm_stats(jk, alpha, eps):
    """(mu, rstd) per column of jk [N, C]: out = x - alpha*mu, var = mean(out^2), rstd = (var + eps)^-1/2."""
    mu = jk.mean(dim=0)
    cen = jk - alpha * mu
    rstd = (cen.pow(2).mean(dim=0) + eps).rsqrt()
    return mu, rstd


def readout_max(jk, gamma, beta, alpha, eps, pos, Wh, bh, target, loss_mode, stats=None):
    """Everything in torch fp64 on the CPU.  loss_mode 0: cross-entropy, target int64 [B]; 1: BCE-with-logits, target [B, K]
    (or [B] for K = 1); mean reduction.  stats: (mu, rstd) to apply instead of the ones derived from jk.
    Returns a dict: y, pooled, arg (position s in the row, -1 for an empty row), logits, loss, djk, dWh, dbh, dgamma, dbeta,
    dalpha."""
    jk, gamma, beta, alpha, Wh, bh = (t.detach().double().cpu() for t in (jk, gamma, beta, alpha, Wh, bh))
    pos = pos.detach().cpu().to(torch.int64)
    N, C = jk.shape
    B, S = pos.shape
    K = Wh.shape[0]
    mu, rstd = graphnorm_stats(jk, alpha, eps) if stats is None else (stats[0].double(), stats[1].double())
    xhat = (jk - alpha * mu) * rstd
    y = gamma * xhat + beta
    # ---- max pooling: strict compare, positions ascending ----
    best = torch.full((B, C), float("-inf"), dtype=torch.float64)
    arg = torch.full((B, C), -1, dtype=torch.int64)
    for s in range(S):
        node = pos[:, s]
        valid = (node >= 0) & (node < N)
        v = y[node.clamp(0, N - 1)]
        upd = valid.reshape(-1, 1) & (v > best)
        best = torch.where(upd, v, best)
        arg = torch.where(upd, torch.full_like(arg, s), arg)
    has = arg >= 0
    pooled = torch.where(has, best, torch.zeros_like(best))
    # ---- head + loss ----
    logits = pooled @ Wh.t() + bh
    if loss_mode == 0:
        t = target.detach().cpu().to(torch.int64)
        lse = torch.logsumexp(logits, dim=1)
        loss = (lse - logits.gather(1, t.reshape(-1, 1)).reshape(-1)).mean()
        dlogits = (torch.softmax(logits, dim=1) - torch.nn.functional.one_hot(t, K).double()) / B
    else:
        t = target.detach().double().cpu().reshape(B, K)
        loss = (logits.clamp(min=0) - logits * t + torch.log1p(torch.exp(-logits.abs()))).mean()
        dlogits = (torch.sigmoid(logits) - t) / (B * K)
    dWh = dlogits.t() @ pooled
    dbh = dlogits.sum(dim=0)
    dpooled = dlogits @ Wh
    # ---- the gradient of the GraphNorm output: only the row at each column's argmax carries one ----
    G = torch.zeros(N, C, dtype=torch.float64)
    bb, cc = torch.nonzero(has, as_tuple=True)
    rows = pos[bb, arg[bb, cc]]
    G.index_put_((rows, cc), dpooled[bb, cc], accumulate=True)
    # ---- GraphNorm backward ----
    dbeta = G.sum(dim=0)
    dgamma = (G * xhat).sum(dim=0)
    dxhat = G * gamma
    dcen = rstd * (dxhat - xhat * (dxhat * xhat).mean(dim=0))
    djk = dcen - alpha * dcen.mean(dim=0)
    dalpha = -mu * dcen.sum(dim=0)
    return dict(y=y, pooled=pooled, arg=arg, logits=logits, loss=loss, djk=djk, dWh=dWh, dbh=dbh, dgamma=dgamma, dbeta=dbeta,
                dalpha=dalpha, mu=mu, rstd=rstd)


def separated_columns(N, C, gen):
    """[N, C] fp64 values whose columns are scaled permutations of a grid: two distinct nodes differ by at least 1 / N of the
    column's range in every column, so no fp32 evaluation can move an argmax between distinct nodes."""
    cols = []
    for _ in range(C):
        step = 0.5 + torch.rand((), generator=gen, dtype=torch.float64)
        off = torch.randn((), generator=gen, dtype=torch.float64)
        cols.append((torch.randperm(N, generator=gen).double() - N / 2) * (4.0 * step / N) + off)
    return torch.stack(cols, dim=1)


def top_gap_ok(y, pos, rel=1e-4):
    """The condition under which an fp32 and an fp64 evaluation must agree on every argmax: for every (b, c) with at least two
    DISTINCT valid nodes in row b, the largest and the second-largest y over those nodes differ by at least rel * max|y[:, c]|.
    Returns (ok, smallest gap / column max-abs)."""
    N, C = y.shape
    colmax = y.abs().max(dim=0).values.clamp(min=1e-300)
    worst = float("inf")
    for b in range(pos.shape[0]):
        nodes = torch.unique(pos[b][(pos[b] >= 0) & (pos[b] < N)])
        if nodes.numel() < 2:
            continue
        top = torch.topk(y[nodes], 2, dim=0).values
        worst = min(worst, float(((top[0] - top[1]) / colmax).min()))
    return worst >= rel, worst
