"""GNN-seg at hop > 0 without a GPU: the k_hop_subgraph oracle (tests/seg_khop_oracle.py) pinned to the hop-0 oracle and
to hand-computed cases, the host-side refusals of the glass_seg_khop_* C entries, GsDataset's hop argument and the
driver's --hop flag."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import seg_khop_oracle as K  # noqa: E402
import seg_oracle as O  # noqa: E402


def _random_directed(seed, n=300, e=1200):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, e), generator=g)
    ei = torch.cat((ei, ei[:, :50]), 1)  # duplicates
    w = torch.ones(ei.shape[1])
    w[torch.randint(0, ei.shape[1], (60, ), generator=g)] = 2.0
    return ei, w, g


def test_hop_zero_is_the_induced_subgraph_oracle():
    ei, w, g = _random_directed(0)
    for _ in range(20):
        nodes = torch.randint(0, 300, (12, ), generator=g)
        a, b = K.extract(ei, w, nodes, 0, 300), O.extract(ei, w, nodes)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_path_walks_in_edges():
    ei = torch.tensor([[0, 1, 2], [1, 2, 3]])  # 0 -> 1 -> 2 -> 3
    assert [K.k_hop_nodes([3], h, ei, 4).tolist() for h in range(4)] == [[3], [2, 3], [1, 2, 3], [0, 1, 2, 3]]
    assert [K.k_hop_nodes([0], h, ei, 4).tolist() for h in range(4)] == [[0]] * 4
    node, lei, lw = K.extract(ei, torch.tensor([1., 2., 3.]), [3], 2, 4)
    assert node.tolist() == [1, 2, 3] and lei.tolist() == [[0, 1], [1, 2]] and lw.tolist() == [2., 3.]


def test_ball_is_the_union_of_walk_frontiers():
    """The radius-k in-ball by a visited-set BFS equals PyG's walk (which keeps re-visiting nodes), hop 1..3."""
    ei, w, g = _random_directed(1)
    for hop in (1, 2, 3):
        for _ in range(10):
            nodes = torch.randint(0, 300, (3, ), generator=g)
            seen, front = set(nodes.tolist()), set(nodes.tolist())
            for _ in range(hop):
                front = {int(s) for s, t in ei.t().tolist() if t in front} - seen
                seen |= front
            assert K.k_hop_nodes(nodes, hop, ei, 300).tolist() == sorted(seen)


# ---- C ABI: refused with codes before any launch -----------------------------------------------------------------
def test_khop_entry_points_validate_on_the_host():
    from glass_amd import _lib
    lib = _lib.load()
    a = np.zeros(64, dtype=np.int32)
    p = a.ctypes.data
    lds_nodes = _lds_nodes()
    # workspace query: 0 while the bitmaps fit in LDS, then capped slots of 3 bitmaps
    assert lib.glass_seg_khop_ws_bytes(lds_nodes, 5000) == 0
    assert lib.glass_seg_khop_ws_bytes(lds_nodes + 1, 0) == 0
    words = (lds_nodes + 1 + 31) // 32
    assert lib.glass_seg_khop_ws_bytes(lds_nodes + 1, 7) == 7 * 3 * words * 4
    assert lib.glass_seg_khop_ws_bytes(lds_nodes + 1, 10**6) == 1024 * 3 * words * 4
    assert lib.glass_seg_khop_ws_bytes(-1, 4) == -1 and lib.glass_seg_khop_ws_bytes(2**31, 4) == -1
    for name, tail in (("glass_seg_khop_count", (p, None)), ("glass_seg_khop_fill", (p, p, None))):
        f = getattr(lib, name)
        # (every call below is refused before a launch: the host buffers never reach a kernel)
        # hops < 0
        assert f(p, p, 4, p, p, 1, 2, -1, None, 0, *tail) == -1
        assert b"hops -1 < 0" in lib.glass_last_error_string()
        # n_base >= 2^31 - 1, negative sizes
        assert f(p, p, 2**31, p, p, 1, 2, 1, None, 0, *tail) == -1
        assert b"too large size" in lib.glass_last_error_string()
        assert f(p, p, 4, p, p, -1, 2, 1, None, 0, *tail) == -1
        assert f(p, p, 4, p, p, 1, -2, 1, None, 0, *tail) == -1
        # null pointers
        assert f(None, p, 4, p, p, 1, 2, 1, None, 0, *tail) == -1
        assert b"null pointer" in lib.glass_last_error_string()
        assert f(p, p, 4, None, p, 1, 2, 1, None, 0, *tail) == -1
        assert f(p, None, 4, p, p, 1, 2, 1, None, 0, *tail) == -1
        assert f(p, p, 4, p, None, 1, 2, 1, None, 0, *tail) == -1
        # a workspace too small (or none) once the bitmaps leave LDS -> GLASS_E_WS, naming the query
        need = lib.glass_seg_khop_ws_bytes(lds_nodes + 1, 1)
        assert f(p, p, lds_nodes + 1, p, p, 1, 2, 1, None, 0, *tail) == -4
        assert b"glass_seg_khop_ws_bytes" in lib.glass_last_error_string()
        assert f(p, p, lds_nodes + 1, p, p, 1, 2, 1, p, need - 1, *tail) == -4
        assert b"%d bytes" % need in lib.glass_last_error_string()
        # an empty split: 0 without a launch (no pointers needed)
        assert f(p, None, 4, p, None, 0, 0, 2, None, 0, *((None, ) * len(tail))) == 0
    # null outputs
    assert lib.glass_seg_khop_count(p, p, 4, p, p, 1, 2, 1, None, 0, None, None) == -1
    assert b"null ball_cnt" in lib.glass_last_error_string()
    assert lib.glass_seg_khop_fill(p, p, 4, p, p, 1, 2, 1, None, 0, None, p, None) == -1
    assert lib.glass_seg_khop_fill(p, p, 4, p, p, 1, 2, 1, None, 0, p, None, None) == -1
    assert b"null output pointer" in lib.glass_last_error_string()


def _lds_nodes():
    text = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    return int(re.search(r"^#define GLASS_SEG_KHOP_LDS_NODES (\d+)$", text, re.M).group(1))


def test_khop_header_cites_the_reference_and_the_abi_stays():
    from glass_amd import _lib
    text = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    assert "GNNSeg.py:213-232" in text and re.search(r"^#define GLASS_SEG_KHOP_WS_SLOTS 1024$", text, re.M)
    assert _lib.ABI_VERSION == 6 and "#define GLASS_ABI_VERSION 6" in text
    for name in ("glass_seg_khop_count", "glass_seg_khop_fill", "glass_seg_khop_ws_bytes"):
        assert name in _lib.SIGNATURES and name + "(" in text


def test_lds_cases_straddle_the_threshold():
    import test_gpu_seg_khop as G
    assert G.LDS_EDGE_N == (_lds_nodes(), _lds_nodes() + 1)


# ---- Python surface ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hop", [-1, 1.0, 1.5, "1", True, None])
def test_dataset_refuses_a_bad_hop(hop):
    from glass_amd import seg
    x, ei, pos = torch.ones(4, 1, 1), torch.tensor([[0, 1], [1, 2]]), torch.tensor([[0, 1]])
    with pytest.raises(ValueError, match="hop"):
        seg.GsDataset(x, ei, torch.ones(2), pos, torch.zeros(1), hop=hop)


def test_driver_hop_flag():
    sys.path.insert(0, ROOT)
    import GNNSeg
    assert GNNSeg.parse_args(["--hop", "2"]).hop == 2
    assert GNNSeg.parse_args([]).hop == 0
    assert "hop=0" in repr(GNNSeg.parse_args(["--dataset", "density"]))
