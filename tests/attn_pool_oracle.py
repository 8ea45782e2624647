"""numpy restatement of attention pooling over a padded node matrix (pool `attn`), forward and backward, in the precision
`dtype` (fp64: the checker; fp32: the measure of what fp32 arithmetic can deliver on the same inputs).  The five formulas:

    s[b,j]   = dot(emb[pos[b,j], :], w)                      pos[b,j] >= 0 (-1 = padding, anywhere in a row)
    a[b,j]   = exp(s[b,j] - max_j s[b,.]) / sum_j exp(...)   over the valid j of row b; 0 at padding
    out[b,:] = sum_j a[b,j] * emb[pos[b,j], :]               a node named twice counts twice; an all-padding row gives 0
    ds[b,j]  = a[b,j] * (dot(dout[b], emb[pos[b,j]]) - dot(dout[b], out[b]))
    demb[n,:] = sum_{(b,j): pos[b,j]=n} (a[b,j] * dout[b,:] + ds[b,j] * w);   dw = sum_{b,j} ds[b,j] * emb[pos[b,j], :]

No torch, nothing of the code under test."""
import numpy as np


def forward(emb, pos, w, dtype=np.float64):
    """-> (out [B, C], alpha [B, Smax], scores [B, Smax] (0 at padding))."""
    emb = np.asarray(emb, dtype=dtype)
    w = np.asarray(w, dtype=dtype).reshape(-1)
    pos = np.asarray(pos, dtype=np.int64)
    B, Smax = pos.shape
    C = emb.shape[1]
    out = np.zeros((B, C), dtype=dtype)
    alpha = np.zeros((B, Smax), dtype=dtype)
    scores = np.zeros((B, Smax), dtype=dtype)
    for b in range(B):
        js = np.nonzero(pos[b] >= 0)[0]
        if js.size == 0:
            continue
        x = emb[pos[b, js]]
        s = (x @ w).astype(dtype)
        e = np.exp(s - s.max()).astype(dtype)
        a = (e / e.sum(dtype=dtype)).astype(dtype)
        scores[b, js] = s
        alpha[b, js] = a
        out[b] = (a[:, None] * x).sum(axis=0, dtype=dtype)
    return out, alpha, scores


def backward(emb, pos, w, dout, dtype=np.float64):
    """-> (demb [n_nodes, C], dw [C]) for the upstream gradient dout [B, C]."""
    emb = np.asarray(emb, dtype=dtype)
    w = np.asarray(w, dtype=dtype).reshape(-1)
    dout = np.asarray(dout, dtype=dtype)
    pos = np.asarray(pos, dtype=np.int64)
    out, alpha, _ = forward(emb, pos, w, dtype)
    demb = np.zeros_like(emb)
    dw = np.zeros_like(w)
    for b in range(pos.shape[0]):
        js = np.nonzero(pos[b] >= 0)[0]
        if js.size == 0:
            continue
        nodes = pos[b, js]
        x = emb[nodes]
        t = (x @ dout[b]).astype(dtype)
        ds = (alpha[b, js] * (t - dout[b] @ out[b])).astype(dtype)
        contrib = alpha[b, js][:, None] * dout[b][None, :] + ds[:, None] * w[None, :]
        np.add.at(demb, nodes, contrib.astype(dtype))
        dw += (ds[:, None] * x).sum(axis=0, dtype=dtype)
    return demb, dw


def rel_inf(a, b):
    """max |a - b| / max |b| (1 in place of a zero denominator): the suite's rel-inf."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.size == 0:
        return 0.0
    d = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / (d if d > 0 else 1.0)
