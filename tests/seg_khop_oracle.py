"""CPU restatement of PyG 1.7.2's k_hop_subgraph (flow "source_to_target") for the hop > 0 GNN-seg tests.

    col, row = edge_index
    subsets = [node_idx]
    for _ in range(num_hops):
        node_mask[:] = False; node_mask[subsets[-1]] = True
        subsets.append(col[node_mask[row]])      # the sources of the edges whose target is in the last frontier
    subset = unique(cat(subsets))                # sorted ascending

The subgraph is then the one induced on `subset`, exactly as at hop 0 (seg_oracle.extract).  Not placed under oracle/:
it is the checker of this path only.
"""
import torch

import seg_oracle as O


def k_hop_nodes(nodes, hop, edge_index, n):
    """Sorted unique node ids of k_hop_subgraph(nodes, hop, edge_index) on n base nodes (the walk as PyG writes it)."""
    col, row = edge_index[0], edge_index[1]
    subsets = [torch.as_tensor(nodes, dtype=torch.int64).flatten()]
    mask = torch.zeros(n, dtype=torch.bool)
    for _ in range(hop):
        mask.fill_(False)
        mask[subsets[-1]] = True
        subsets.append(col[mask[row]])
    return torch.unique(torch.cat(subsets))


def extract(edge_index, edge_weight, nodes, hop, n):
    """k_hop_subgraph(nodes, hop, edge_index, relabel_nodes=True): (sorted unique nodes, local edge_index, weights)."""
    return O.extract(edge_index, edge_weight, k_hop_nodes(nodes, hop, edge_index, n))


def balls(edge_index, pos, hop, n):
    """The ball of every row of pos (-1 padding), as a list of sorted id tensors."""
    return [k_hop_nodes(row[row >= 0], hop, edge_index, n) for row in pos]


def split_blocks(edge_index, edge_weight, pos, mode, hop, n):
    """seg_oracle.split_blocks at `hop`: every row of pos grown into its ball, then extracted.  Only the edges inside the
    union of the balls are scanned for the induced subgraphs (same order, fewer to scan)."""
    bs = balls(edge_index, pos, hop, n)
    inside = torch.zeros(n, dtype=torch.bool)
    for b in bs:
        inside[b] = True
    keep = inside[edge_index[0]] & inside[edge_index[1]]
    width = max([b.shape[0] for b in bs] + [1])
    bpos = torch.full((len(bs), width), -1, dtype=torch.int64)
    for i, b in enumerate(bs):
        bpos[i, :b.shape[0]] = b
    blocks = O.split_blocks(edge_index[:, keep], edge_weight[keep], bpos, mode)
    for b, blk in zip(bs, blocks):  # (an empty row stays empty: its ball is empty too)
        assert torch.equal(blk[0], b)
    return blocks
