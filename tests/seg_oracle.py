"""fp64 CPU restatement of GNN-seg (the reference's GNNSeg.py on PyG 1.7.2) for the tests of glass_amd/seg.py.

Contract points restated here:
  features   one_hot(weighted row degree) as float [N,1,maxdeg+1] / ones [N,1,1]
  extract    hop-0 induced subgraph: nodes = sorted unique ids, edges = base edges with both ends inside, in base order,
             base weights, duplicates kept
  collate    disjoint union in batch order; pos = each subgraph's batch nodes, -1 padded
  operators  PyG orientation (messages edge_index[0] -> edge_index[1], summed at the target); GCN without self-loops:
             val = dinv[src] w dinv[dst], dinv = (weighted in-degree)^-1/2, 0 where the degree is 0 (no clamp);
             GIN: (A + I) x with unit weights, then the Linear
  models     GConv (GraphNorm over the whole batch, in-place ELU: the stored inner outputs are the activated tensors,
             dropout after), GNN (per channel, mean over channels, SUM pool, Linear -> Dropout -> ELU -> Linear)
Not placed under oracle/: it is the checker of this path only.
"""
import torch
import torch.nn.functional as F


def degree_feature(edge_index, edge_attr, n):
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, edge_index[0], edge_attr.double()).to(torch.int64)
    return F.one_hot(deg).to(torch.float).reshape(n, 1, -1)


def one_feature(n):
    return torch.ones(n, 1, 1)


def extract(edge_index, edge_weight, nodes):
    """k_hop_subgraph(nodes, 0, edge_index, relabel_nodes=True): (sorted unique nodes, local edge_index, weights)."""
    node = torch.unique(torch.as_tensor(nodes, dtype=torch.int64))
    size = max(int(edge_index.max()) + 1 if edge_index.numel() else 0, int(node.max()) + 1 if node.numel() else 0)
    inside = torch.zeros(size, dtype=torch.bool)
    inside[node] = True
    mask = inside[edge_index[0]] & inside[edge_index[1]]
    relabel = torch.full((inside.shape[0], ), -1, dtype=torch.int64)
    relabel[node] = torch.arange(node.shape[0])
    return node, relabel[edge_index[:, mask]], edge_weight[mask].double()


def gcn_values(ei, w, n):
    """Per-edge values of PyG's gcn_norm (add_self_loops=False) for a local edge list."""
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], w)
    dinv = deg.pow(-0.5)
    dinv[torch.isinf(dinv)] = 0
    return dinv[ei[0]] * w * dinv[ei[1]]


def csr_pair(ei, val, n, mode):
    """((rowptr, col, val) by target, (rowptr, col, val) by source), columns ascending, duplicates in base order; mode
    gin: unit values plus one diagonal entry per row placed before equal columns."""
    src, dst = ei[0], ei[1]
    if mode == "gin":
        diag = torch.arange(n)
        src, dst = torch.cat((diag, src)), torch.cat((diag, dst))
        val = torch.ones(src.shape[0], dtype=torch.float64)
    out = []
    for row, col in ((dst, src), (src, dst)):
        perm = torch.argsort(row * max(n, 1) + col, stable=True)
        rp = torch.zeros(n + 1, dtype=torch.int64)
        rp[1:] = torch.cumsum(torch.bincount(row, minlength=n), 0)
        out.append((rp, col[perm], val[perm]))
    return tuple(out)


def split_blocks(edge_index, edge_weight, pos, mode):
    """Every row of pos (-1 padding) extracted: list of (nodes, (csr by target), (csr by source))."""
    blocks = []
    for row in pos:
        node, ei, w = extract(edge_index, edge_weight, row[row >= 0])
        n = node.shape[0]
        val = gcn_values(ei, w, n) if mode == "gcn" else None
        blocks.append((node, *csr_pair(ei, val, n, mode)))
    return blocks


def collate(blocks, ids):
    """Block-diagonal batch: (node_map, (rowptr, col, val) by target, same by source, pos)."""
    maps, parts, off = [], [[], []], 0
    sizes = [blocks[i][0].shape[0] for i in ids]
    width = max(max(sizes), 1)
    pos = torch.full((len(ids), width), -1, dtype=torch.int64)
    for b, i in enumerate(ids):
        node = blocks[i][0]
        maps.append(node)
        for o in range(2):
            parts[o].append((blocks[i][1 + o], off))
        pos[b, :node.shape[0]] = off + torch.arange(node.shape[0])
        off += node.shape[0]
    csrs = []
    for o in range(2):
        lens = torch.cat([rp[1:] - rp[:-1] for (rp, _, _), _ in parts[o]]) if parts[o] else torch.zeros(0, dtype=torch.int64)
        rp = torch.zeros(off + 1, dtype=torch.int64)
        rp[1:] = torch.cumsum(lens, 0)
        col = torch.cat([c + s for (_, c, _), s in parts[o]])
        val = torch.cat([v for (_, _, v), _ in parts[o]])
        csrs.append((rp, col, val))
    return torch.cat(maps), csrs[0], csrs[1], pos


def dense(csr, n):
    rp, col, val = csr
    rows = torch.repeat_interleave(torch.arange(n), rp[1:] - rp[:-1])
    a = torch.zeros(n * n, dtype=torch.float64)
    a.index_add_(0, rows * n + col, val.double())
    return a.reshape(n, n)


def graphnorm(x, weight, bias, mean_scale, eps=1e-5):
    out = x - x.mean(0, keepdim=True) * mean_scale
    var = out.pow(2).mean(0, keepdim=True)
    return weight * out / (var + eps).sqrt() + bias


def gconv(p, prefix, x, A, mode, n_layers, masks=None):
    """GConv forward; p: fp64 parameters by state_dict key; A: dense target-major operator ((A + I) for gin);
    masks[l]: keep-scales of the dropout after inner layer l (None: no dropout)."""
    xs = []
    for l in range(n_layers):
        c = f"{prefix}convs.{l}."
        if mode == "gcn":
            h = A @ (x @ p[c + "weight"]) + p[c + "bias"]
        else:
            h = (A @ x) @ p[c + "conv.nn.weight"].t() + p[c + "conv.nn.bias"]
        if l == n_layers - 1:
            xs.append(h)
            break
        g = f"{prefix}gns.{l}."
        h = F.elu(graphnorm(h, p[g + "weight"], p[g + "bias"], p[g + "mean_scale"]))
        xs.append(h)  # the in-place ELU: the stored tensor is the activated one
        x = h * masks[l] if masks is not None else h
    return torch.cat(xs, dim=-1)


def gnn(p, x, A, pos, mode, n_layers, mlp_keys):
    """GNN forward (dropout 0): per channel GConv, mean over channels, sum pool, Linear -> ELU -> Linear."""
    embs = [gconv(p, "mods.0.", x[:, c, :].double(), A, mode, n_layers) for c in range(x.shape[1])]
    emb = torch.stack(embs, 1).mean(1)
    sel = torch.zeros(pos.shape[0], emb.shape[0], dtype=torch.float64)
    for b in range(pos.shape[0]):
        for j in pos[b][pos[b] >= 0]:
            sel[b, j] += 1
    h = sel @ emb
    (w0, b0), (w1, b1) = [(p[k + "weight"], p[k + "bias"]) for k in mlp_keys]
    return F.elu(h @ w0.t() + b0) @ w1.t() + b1
