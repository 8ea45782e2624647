"""CPU restatement of the centre mark of GNN-seg's k-hop balls, for the tests of GsDataset(pool="centre").

Restates reference GNNSeg.py:214-225 (todata): k_hop_subgraph(centre, hop, edge_index, relabel_nodes=True) returns, beside
the ball's sorted node list, the position `inv` of every entry of `centre` in that list; the mark is a zero vector over
the ball with ones at `inv`, so a node listed twice in a pos row still gets one mark.  PyG's collate (GNNSeg.py:41-62)
then concatenates the marks of a batch's graphs in batch order.  The balls themselves come from seg_khop_oracle.
Not placed under oracle/: it is the checker of this path only.
"""
import torch

import seg_khop_oracle as K


def centre_marks(edge_index, pos, hop, n):
    """Per row of pos (-1 padding): (sorted ball, the centres' indices within it ascending, 0/1 mark over the ball)."""
    out = []
    for row in pos:
        centre = row[row >= 0].to(torch.int64)
        ball = K.k_hop_nodes(centre, hop, edge_index, n)
        inv = torch.searchsorted(ball, centre)  # a ball holds its seeds: every centre is found where it sorts
        assert torch.equal(ball[inv], centre)
        mark = torch.zeros_like(ball)
        mark[inv] = 1
        out.append((ball, torch.nonzero(mark).flatten(), mark))
    return out


def batch(parts, ids):
    """For the subgraphs `ids` in batch order: (pos [len(ids), max centre count or 1] = the batch rows of each block's
    centres, ascending, -1 padding; mark uint8 over the batch rows)."""
    width = max([int(parts[i][1].shape[0]) for i in ids] + [1])
    pos = torch.full((len(ids), width), -1, dtype=torch.int64)
    marks, off = [], 0
    for b, i in enumerate(ids):
        ball, local, mark = parts[i]
        pos[b, :local.shape[0]] = off + local
        marks.append(mark.to(torch.uint8))
        off += ball.shape[0]
    return pos, torch.cat(marks) if marks else torch.zeros(0, dtype=torch.uint8)
