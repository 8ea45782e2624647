"""GNN-seg without a GPU: the fp64 oracle (tests/seg_oracle.py) on hand-computed cases, the K10 C ABI's argument checks,
the GNN-seg node features of datasets.BaseGraph, and the GNNSeg.py driver's table and flags."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import seg_oracle as O  # noqa: E402


def test_extract_sorts_and_merges_duplicate_ids():
    ei = torch.tensor([[5, 2, 9, 2, 7], [2, 5, 2, 9, 5]])
    w = torch.tensor([1., 2., 1., 1., 1.])
    node, lei, lw = O.extract(ei, w, [9, 2, 5, 2])
    assert node.tolist() == [2, 5, 9]
    assert lei.tolist() == [[1, 0, 2, 0], [0, 1, 0, 2]]  # base order kept; (7,5) left out
    assert lw.tolist() == [1., 2., 1., 1.]


def test_directed_graph_aggregates_at_the_target():
    # 0 -> 1, 0 -> 2, 1 -> 2 (directed): PyG sums at edge_index[1]
    ei = torch.tensor([[0, 0, 1], [1, 2, 2]])
    _, lei, w = O.extract(ei, torch.ones(3), [0, 1, 2])
    val = O.gcn_values(lei, w, 3)
    # in-degrees 0, 1, 2: dinv = 0, 1, 1/sqrt 2
    assert torch.allclose(val, torch.tensor([0., 0., 1 / math.sqrt(2)], dtype=torch.float64))
    (rp, col, v), (rpt, colt, vt) = O.csr_pair(lei, val, 3, "gcn")
    assert rp.tolist() == [0, 0, 1, 3] and col.tolist() == [0, 0, 1]
    assert rpt.tolist() == [0, 2, 3, 3] and colt.tolist() == [1, 2, 2]
    A = O.dense((rp, col, v), 3)
    x = torch.tensor([[1.], [10.], [100.]], dtype=torch.float64)
    assert (A @ x).flatten().tolist() == pytest.approx([0., 0., 10 / math.sqrt(2)])


def test_fractional_weight_has_no_degree_clamp():
    ei = torch.tensor([[0, 1], [1, 0]])
    w = torch.tensor([0.25, 0.25])
    _, lei, lw = O.extract(ei, w, [0, 1])
    val = O.gcn_values(lei, lw, 2)
    # deg 0.25 each: 0.25^-1/2 * 0.25 * 0.25^-1/2 = 1 (the clamp deg < 0.5 -> +1 would give 0.25 / 1.25)
    assert val.tolist() == pytest.approx([1.0, 1.0])


def test_isolated_member_node():
    ei = torch.tensor([[0, 1], [1, 0]])
    node, lei, lw = O.extract(ei, torch.ones(2), [0, 1, 3])
    assert node.tolist() == [0, 1, 3]
    (rp, col, v), _ = O.csr_pair(lei, O.gcn_values(lei, lw, 3), 3, "gcn")
    assert rp.tolist() == [0, 1, 2, 2]
    (rp, col, v), _ = O.csr_pair(lei, None, 3, "gin")
    assert rp.tolist() == [0, 2, 4, 5] and col.tolist() == [0, 1, 0, 1, 2]


def test_gin_ignores_weights():
    ei = torch.tensor([[0, 1], [1, 0]])
    _, lei, lw = O.extract(ei, torch.tensor([2., 2.]), [0, 1])
    (rp, col, v), _ = O.csr_pair(lei, None, 2, "gin")
    assert v.tolist() == [1., 1., 1., 1.]
    x = torch.tensor([[1.], [3.]], dtype=torch.float64)
    assert (O.dense((rp, col, v), 2) @ x).flatten().tolist() == [4., 4.]


def test_gin_diagonal_goes_before_an_equal_column():
    ei = torch.tensor([[1, 0], [1, 1]])  # self-loop 1 -> 1 and 0 -> 1
    _, lei, _ = O.extract(ei, torch.ones(2), [0, 1])
    (rp, col, _), _ = O.csr_pair(lei, None, 2, "gin")
    assert rp.tolist() == [0, 1, 4] and col.tolist() == [0, 0, 1, 1]


def test_gconv_stores_activated_inner_outputs():
    torch.manual_seed(0)
    n, H = 4, 3
    A = torch.eye(n, dtype=torch.float64)
    p = {"mods.0.convs.0.weight": torch.randn(2, H, dtype=torch.float64), "mods.0.convs.0.bias": torch.zeros(H),
         "mods.0.convs.1.weight": torch.randn(H, H, dtype=torch.float64), "mods.0.convs.1.bias": torch.zeros(H),
         "mods.0.gns.0.weight": torch.ones(H), "mods.0.gns.0.bias": torch.zeros(H), "mods.0.gns.0.mean_scale": torch.ones(H)}
    p = {k: v.double() for k, v in p.items()}
    x = torch.randn(n, 2, dtype=torch.float64)
    out = O.gconv(p, "mods.0.", x, A, "gcn", 2)
    inner = out[:, :H]
    assert inner.min() >= -1 and (inner < 0).any()  # ELU-activated, not the GraphNorm output
    gn = O.graphnorm(x @ p["mods.0.convs.0.weight"], torch.ones(H), torch.zeros(H), torch.ones(H))
    assert torch.allclose(inner, torch.nn.functional.elu(gn))


def test_collate_block_diagonal():
    ei = torch.tensor([[0, 1, 2, 3], [1, 0, 3, 2]])
    blocks = O.split_blocks(ei, torch.ones(4), torch.tensor([[0, 1, -1], [2, 3, 3]]), "gcn")
    node_map, (rp, col, val), _, pos = O.collate(blocks, [1, 0])
    assert node_map.tolist() == [2, 3, 0, 1]
    assert rp.tolist() == [0, 1, 2, 3, 4] and col.tolist() == [1, 0, 3, 2]
    assert pos.tolist() == [[0, 1], [2, 3]]


# ---- C ABI: refused with codes before any launch -----------------------------------------------------------------
def test_seg_entry_points_validate_on_the_host():
    from glass_amd import _lib
    lib = _lib.load()
    a = np.zeros(64, dtype=np.int32)
    p = a.ctypes.data
    # unknown mode -> GLASS_E_UNSUPPORTED
    assert lib.glass_seg_extract_count(p, p, p, p, p, 4, p, p, 1, 2, 7, p, p, p, None) == -3
    assert b"unknown mode 7" in lib.glass_last_error_string()
    assert lib.glass_seg_extract_fill(p, p, p, p, p, p, 4, p, p, 1, 2, 9, p, p, p, p, p, p, p, None) == -3
    # negative sizes, null pointers -> GLASS_E_ARG
    assert lib.glass_seg_extract_count(p, p, p, p, p, -1, p, p, 1, 2, 0, p, p, p, None) == -1
    assert lib.glass_seg_extract_count(None, p, p, p, p, 4, p, p, 1, 2, 0, p, p, p, None) == -1
    assert lib.glass_seg_extract_count(p, p, p, p, p, 4, p, p, 1, 2, 0, p, p, None, None) == -1  # gcn without deg
    assert b"needs deg" in lib.glass_last_error_string()
    assert lib.glass_seg_extract_count(p, p, None, p, p, 4, p, p, 1, 2, 0, p, p, p, None) == -1  # gcn without weights
    assert lib.glass_seg_extract_fill(p, p, p, p, p, None, 4, p, p, 1, 2, 0, p, p, p, p, p, p, p, None) == -1
    assert lib.glass_seg_extract_fill(p, p, p, p, p, p, 4, p, p, 1, 2, 1, None, p, p, None, p, p, p, None) == -1
    assert lib.glass_seg_collate(p, p, 1, p, p, p, p, p, p, p, -2, p, 4, p, p, p, p, p, p, p, p, 2, None) == -1
    assert lib.glass_seg_collate(p, p, 1, p, p, p, p, p, p, None, 1, p, 4, p, p, p, p, p, p, p, p, 2, None) == -1
    assert lib.glass_seg_collate(p, p, 1, p, p, p, p, p, p, p, 1, p, 4, p, p, p, p, p, p, p, p, 0, None) == -1
    assert b"pos_width 0" in lib.glass_last_error_string()
    # nothing to do -> 0 without a launch
    assert lib.glass_seg_collate(None, None, 0, None, None, None, None, None, None, None, 0, None, 0, None, None, None,
                                 None, None, None, None, None, 0, None) == 0


def test_seg_modes_match_the_header():
    from glass_amd import _lib
    text = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    assert "#define GLASS_SEG_GCN 0" in text and "#define GLASS_SEG_GIN 1" in text
    assert _lib.SEG_MODES == {"gcn": 0, "gin": 1}
    assert "GNNSeg.py:213-226" in text and "GNNSeg.py:41-62" in text


# ---- node features ----------------------------------------------------------------------------------------------
def test_one_and_degree_features_on_density():
    import datasets
    g = datasets.load_dataset("density")
    n = g.x.shape[0]
    g.addOneFeature()
    assert g.x.shape == (n, 1, 1) and g.x.dtype == torch.float32 and bool((g.x == 1).all())
    g = datasets.load_dataset("density")
    g.addDegreeFeature()
    ref = O.degree_feature(g.edge_index, g.edge_attr, n)
    assert g.x.dtype == torch.float32 and g.x.shape == ref.shape and torch.equal(g.x, ref)
    deg = torch.zeros(n).index_add_(0, g.edge_index[0], g.edge_attr.float()).to(torch.int64)
    assert g.x.shape[-1] == int(deg.max()) + 1
    assert torch.equal(g.x[:, 0, :].argmax(1), deg) and bool((g.x.sum(-1) == 1).all())


# ---- driver -----------------------------------------------------------------------------------------------------
def test_driver_table_and_flags():
    sys.path.insert(0, ROOT)
    import GNNSeg
    assert GNNSeg.best_hyperparams == {
        "density": {"conv_layer": 1, "dropout": 0.4, "hidden_dim": 16},
        "component": {"conv_layer": 1, "dropout": 0.0, "hidden_dim": 16},
        "coreness": {"conv_layer": 1, "dropout": 0.3, "hidden_dim": 16},
        "cut_ratio": {"conv_layer": 1, "dropout": 0.1, "hidden_dim": 4},
        "hpo_neuro": {"conv_layer": 1, "dropout": 0.4, "hidden_dim": 64},
        "ppi_bp": {"conv_layer": 8, "dropout": 0.4, "hidden_dim": 64},
        "hpo_metab": {"conv_layer": 1, "dropout": 0.1, "hidden_dim": 64},
        "em_user": {"conv_layer": 1, "dropout": 0.4, "hidden_dim": 64}}
    a = GNNSeg.parse_args(["--test", "--repeat", "10", "--device", "1", "--dataset", "coreness"])
    assert (a.test, a.repeat, a.device, a.dataset, a.epochs) == (True, 10, 1, "coreness", 500)
    assert GNNSeg.parse_args(["--epochs", "3"]).epochs == 3
    assert GNNSeg.parse_args([]).dataset == "ppi_bp"
    assert GNNSeg.conv_mode("density") == "gin" and GNNSeg.conv_mode("synthetic:density") == "gin"
    assert all(GNNSeg.conv_mode(d) == "gcn" for d in GNNSeg.best_hyperparams if d != "density")
    assert GNNSeg.base_name("synthetic:ppi_bp") == "ppi_bp"
    for bad in ("synthetic:tiny", "cora"):
        with pytest.raises(NotImplementedError):
            GNNSeg.base_name(bad)


def test_models_keep_pyg_parameter_names_and_shapes():
    from glass_amd import seg
    with pytest.raises(NotImplementedError):
        seg.GCNConv(3, 4, add_self_loops=True)
    g = seg.GConv(5, 8, 8, 3, conv=seg.GCNConv)
    shapes = {k: tuple(v.shape) for k, v in g.state_dict().items()}
    assert shapes["convs.0.weight"] == (5, 8) and shapes["convs.0.bias"] == (8, ) and shapes["convs.2.weight"] == (8, 8)
    assert shapes["gns.1.mean_scale"] == (8, ) and "gns.2.weight" not in shapes
    assert float(g.state_dict()["convs.1.bias"].abs().max()) == 0.0
    bound = math.sqrt(6 / 13)
    assert float(g.convs[0].weight.abs().max()) <= bound
    gi = seg.GConv(5, 8, 8, 1, conv=seg.MyGINConv)
    assert {k: tuple(v.shape) for k, v in gi.state_dict().items() if "nn" in k} == {"convs.0.conv.nn.weight": (8, 5),
                                                                                     "convs.0.conv.nn.bias": (8, )}
