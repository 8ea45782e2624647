"""GNN-seg centre pooling without a GPU: the centre-mark oracle (tests/seg_centre_oracle.py) on hand-made graphs, the
host-side refusals of glass_seg_centre_index / glass_seg_collate_centre, GsDataset's pool argument, the driver's --pool
flag, and the new exports in the header, the binding and the built library."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import seg_centre_oracle as C  # noqa: E402
import seg_khop_oracle as K  # noqa: E402


# ---- the oracle on graphs small enough to do by hand ---------------------------------------------------------------
def test_path_with_a_known_in_ball():
    ei = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 4]])  # 0 -> 1 -> 2 -> 3 -> 4
    pos = torch.tensor([[3, -1], [4, 2]])
    (b0, l0, m0), (b1, l1, m1) = C.centre_marks(ei, pos, 2, 5)
    assert b0.tolist() == [1, 2, 3] and l0.tolist() == [2] and m0.tolist() == [0, 0, 1]
    assert b1.tolist() == [0, 1, 2, 3, 4] and l1.tolist() == [2, 4] and m1.tolist() == [0, 0, 1, 0, 1]
    (b0, l0, m0), _ = C.centre_marks(ei, pos, 0, 5)  # hop 0: the ball is the centres, every node marked
    assert b0.tolist() == [3] and l0.tolist() == [0] and m0.tolist() == [1]
    bpos, mark = C.batch(C.centre_marks(ei, pos, 2, 5), [1, 0])
    assert bpos.tolist() == [[2, 4], [7, -1]] and mark.tolist() == [0, 0, 1, 0, 1, 0, 0, 1]
    bpos, mark = C.batch(C.centre_marks(ei, pos, 2, 5), [0])
    assert bpos.tolist() == [[2]] and mark.tolist() == [0, 0, 1]


def test_directed_edge_is_followed_one_way_only():
    ei = torch.tensor([[5], [2]])  # 5 -> 2: 5 is in the in-ball of 2, 2 is not in the in-ball of 5
    (b0, l0, m0), (b1, l1, m1) = C.centre_marks(ei, torch.tensor([[2], [5]]), 1, 6)
    assert b0.tolist() == [2, 5] and l0.tolist() == [0] and m0.tolist() == [1, 0]
    assert b1.tolist() == [5] and l1.tolist() == [0] and m1.tolist() == [1]


def test_duplicated_id_in_a_row_gives_one_mark():
    ei = torch.tensor([[0, 1], [1, 2]])
    (ball, local, mark), = C.centre_marks(ei, torch.tensor([[2, 2, 1, -1]]), 1, 3)
    assert ball.tolist() == [0, 1, 2] and local.tolist() == [1, 2] and mark.tolist() == [0, 1, 1]
    bpos, bmark = C.batch([(ball, local, mark)], [0, 0])
    assert bpos.tolist() == [[1, 2], [4, 5]] and bmark.tolist() == [0, 1, 1, 0, 1, 1]


def test_isolated_centre_and_empty_row():
    ei = torch.tensor([[0], [1]])
    parts = C.centre_marks(ei, torch.tensor([[3, -1], [3, 1], [-1, -1]]), 2, 4)
    assert [p[0].tolist() for p in parts] == [[3], [0, 1, 3], []]
    assert [p[1].tolist() for p in parts] == [[0], [1, 2], []]
    assert [p[2].tolist() for p in parts] == [[1], [0, 1, 1], []]
    bpos, mark = C.batch(parts, [2, 0, 1])
    assert bpos.tolist() == [[-1, -1], [0, -1], [2, 3]] and mark.tolist() == [1, 0, 1, 1]
    bpos, mark = C.batch(parts, [2])
    assert bpos.tolist() == [[-1]] and mark.tolist() == []


def test_marks_agree_with_membership_on_a_random_directed_graph():
    g = torch.Generator().manual_seed(4)
    ei = torch.randint(0, 200, (2, 700), generator=g)
    pos = torch.randint(0, 200, (15, 6), generator=g)
    pos[torch.rand(pos.shape, generator=g) < 0.3] = -1
    for hop in (1, 2):
        for row, (ball, local, mark) in zip(pos, C.centre_marks(ei, pos, hop, 200)):
            want = sorted(set(row[row >= 0].tolist()))
            assert torch.equal(ball, K.k_hop_nodes(row[row >= 0], hop, ei, 200))
            assert ball[local].tolist() == want and int(mark.sum()) == len(want)
            assert [int(v) in want for v in ball.tolist()] == mark.bool().tolist()


# ---- C ABI: refused with codes before any launch -----------------------------------------------------------------
def test_centre_entry_points_validate_on_the_host():
    from glass_amd import _lib
    lib = _lib.load()
    a = np.zeros(64, dtype=np.int32)
    p = a.ctypes.data
    err = lib.glass_last_error_string
    # (every call below is refused before a launch: the host buffers never reach a kernel)
    f = lib.glass_seg_centre_index
    for k, name in ((2, b"n_sub"), (3, b"n_centre"), (6, b"n_ball")):
        for bad in (-1, 2**31 - 1, 2**31):
            args = [p, p, 1, 2, p, p, 3, p, None]
            args[k] = bad
            assert f(*args) == -1
            assert name in err() and b"%d outside [0, 2^31 - 1)" % bad in err()
    for k, name in ((0, b"centre_ptr"), (1, b"centre_nodes"), (4, b"ball_ptr"), (5, b"ball_nodes"), (7, b"centre_local")):
        args = [p, p, 1, 2, p, p, 3, p, None]
        args[k] = None
        assert f(*args) == -1
        assert b"null " + name in err()
    assert f(None, None, 0, 0, None, None, 0, None, None) == 0  # an empty split: 0 without a launch

    g = lib.glass_seg_collate_centre

    def args():
        return [p, p, 1, p, p, p, p, p, p, p, p, 2, p, 1, p, 4, p, p, p, p, p, p, p, p, 2, p, None]

    for k, name in ((2, b"n_sub"), (11, b"n_centre"), (13, b"n_batch"), (15, b"n_nodes"), (24, b"pos_width")):
        for bad in (-2, 2**31 - 1):
            v = args()
            v[k] = bad
            assert g(*v) == -1
            assert name in err() and b"%d outside [0, 2^31 - 1)" % bad in err()
    for k, name in ((0, b"sub_ptr"), (1, b"sub_nodes"), (3, b"rowptr_in"), (4, b"col_"), (5, b"val_"), (6, b"rowptr_out"),
                    (7, b"col_"), (8, b"val_"), (9, b"centre_ptr"), (10, b"centre_local"), (12, b"ids"), (14, b"node_off"),
                    (16, b"brow_in"), (17, b"brow_out"), (18, b"bcol_"), (19, b"bval_"), (20, b"bcol_"), (21, b"bval_"),
                    (22, b"node_map"), (23, b"pos"), (25, b"mark")):
        v = args()
        v[k] = None
        assert g(*v) == -1, k
        assert b"null" in err() and name in err(), (k, err())
    v = args()
    v[24] = 0
    assert g(*v) == -1 and b"pos_width 0 with 4 batch nodes" in err()
    v = [None] * 27
    for k in (2, 11, 13, 15, 24):
        v[k] = 0
    assert g(*v) == 0  # an empty batch: 0 without a launch


def test_new_exports_are_in_the_header_the_binding_and_the_library():
    from glass_amd import _lib
    text = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("glass_seg_centre_index", "glass_seg_collate_centre"):
        assert re.search(r"^int %s\(" % name, text, re.M) and name in _lib.SIGNATURES
        assert getattr(so, name) is not None
    assert len(_lib.SIGNATURES["glass_seg_centre_index"][1]) == 9
    assert len(_lib.SIGNATURES["glass_seg_collate_centre"][1]) == 27
    assert "GNNSeg.py:214-225" in text and "GNNSeg.py:41-62" in text
    assert _lib.ABI_VERSION == 6 and "#define GLASS_ABI_VERSION 6" in text and so.glass_version() == 6


def test_lds_cases_straddle_the_threshold():
    import test_gpu_seg_centre as G
    text = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    lds = int(re.search(r"^#define GLASS_SEG_LDS_NODES (\d+)$", text, re.M).group(1))
    assert G.LDS_EDGE_BALL == (lds, lds + 1)
    for size in G.LDS_EDGE_BALL:
        x, ei, w, pos, y = G._hub(size)
        sizes = [p[0].shape[0] for p in C.centre_marks(ei, pos, 1, x.shape[0])]
        assert max(sizes) == size and min(sizes) < 8


# ---- Python surface ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool", ["center", "", None, 0, "Ball", "max"])
def test_dataset_refuses_a_bad_pool(pool):
    from glass_amd import seg
    x, ei, pos = torch.ones(4, 1, 1), torch.tensor([[0, 1], [1, 2]]), torch.tensor([[0, 1]])
    with pytest.raises(ValueError, match=r'"ball" or "centre"'):
        seg.GsDataset(x, ei, torch.ones(2), pos, torch.zeros(1), hop=1, pool=pool)


def test_driver_pool_flag():
    sys.path.insert(0, ROOT)
    import GNNSeg
    assert GNNSeg.parse_args([]).pool == "ball"
    assert GNNSeg.parse_args(["--hop", "1"]).pool == "ball"
    a = GNNSeg.parse_args(["--hop", "2", "--pool", "centre"])
    assert (a.hop, a.pool) == (2, "centre")
    with pytest.raises(SystemExit):
        GNNSeg.parse_args(["--pool", "max"])
    assert "--pool" in GNNSeg.__doc__
