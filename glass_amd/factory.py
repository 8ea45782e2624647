"""Model construction as the reference driver does it (GLASSTest.py:129-175 `buildModel`), through the
drop-in `impl.models` surface: EmbZGConv(GLASSConv layers, ELU, JK, GraphNorm) + nn.Linear head + pool."""
import functools

import torch.nn as nn


def build_glass(hidden, layers, max_deg, out_ch, aggr, pool, z_ratio, dropout=0.0, jk=True, pad_width=True, gat_heads=1,
                live_edge_weight=False, moment_eps=1e-5, edge_dropout=0.0):
    """pad_width: a hidden width no kernel family serves (33..63, 65..127, ...) is built at the next family width with
    zero padding — exact, same logical parameters, logical state_dict (glass_amd/widths.py); False keeps the width as it
    is (the per-op path with library GEMMs serves it).  gat_heads: the attention heads of aggr "gat" (GLASSConv; aggr "gatv2" has one).
    live_edge_weight: the layers aggregate with each call's edge weights, differentiably (GLASSConv).  moment_eps: the
    constant under the root of aggr "std" (GLASSConv).  edge_dropout: the share of adjacency entries every layer drops in each
    training forward (DropEdge; GLASSConv: aggr "sum" / "mean" / "gcn", not with live_edge_weight)."""
    if edge_dropout and live_edge_weight:  # (live_edge_weight reaches the layers after their construction)
        raise ValueError("build_glass: edge_dropout is not available together with live_edge_weight")
    from impl import models
    pools = {"mean": models.MeanPool, "max": models.MaxPool, "sum": models.AddPool, "size": models.SizePool}
    if pool not in pools:
        raise NotImplementedError

    def build(h):
        conv = models.EmbZGConv(h, h, layers, max_deg=max_deg, activation=nn.ELU(inplace=True), jk=jk, dropout=dropout,
                                conv=functools.partial(models.GLASSConv, aggr=aggr, z_ratio=z_ratio, dropout=dropout,
                                                       gat_heads=gat_heads, moment_eps=moment_eps, edge_dropout=edge_dropout),
                                gn=True)
        mlp = nn.Linear(h * layers if jk else h, out_ch)
        return models.GLASS(conv, nn.ModuleList([mlp]), nn.ModuleList([pools[pool]()]), live_edge_weight=live_edge_weight)

    if not pad_width:
        return build(hidden)
    from . import widths
    return widths.build_at_fused_width(hidden, build)
