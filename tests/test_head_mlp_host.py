"""Host side of the fused two-layer MLP head (glass_amd/csrc/head_mlp.hip, losses.fusable_head / mlp_head_loss): which heads
are recognised, that the three entry points are declared, bound and exported, and that their argument checks answer with
codes before anything is launched.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("glass_head_mlp_loss_fwd_f32", "glass_head_mlp_loss_bwd_f32", "glass_head_mlp_f32")
E_ARG, E_UNSUPPORTED = -1, -3


def _driver_head(monkeypatch, dropout, n_out=3):
    """mods.1 of the model GNNSeg.Run.build_model builds (GNNSeg.py:272-277), without loading a dataset."""
    import GNNSeg
    from impl import config
    monkeypatch.setattr(config, "device", torch.device("cpu"))  # (undone after the test: the selector is process-wide)
    run = GNNSeg.Run.__new__(GNNSeg.Run)
    run.input_channels, run.mode, run.output_channels = 1, "gin", n_out
    return run.build_model(hidden_dim=16, conv_layer=1, dropout=dropout).mods[1]


def test_fusable_head_recognises_the_driver_heads(monkeypatch):
    from glass_amd import losses, models
    h0, h4 = _driver_head(monkeypatch, 0.0), _driver_head(monkeypatch, 0.4)
    # both sequence layouts: no Dropout module at dropout 0 (the second Linear is modlist.2), else modlist.3
    assert [type(m).__name__ for m in h0.seq.modlist] == ["Linear", "ELU", "Linear"]
    assert [type(m).__name__ for m in h4.seq.modlist] == ["Linear", "Dropout", "ELU", "Linear"]
    assert losses.fusable_head(h0) == "mlp2" and losses.fusable_head(h4) == "mlp2"
    lin1, p, act, lin2 = losses._mlp2_parts(h4)
    assert lin1 is h4.seq.modlist[0] and lin2 is h4.seq.modlist[3] and p == 0.4 and act == models.ACT_ELU
    assert losses._mlp2_parts(h0)[1] == 0.0 and losses._mlp2_parts(h0)[3] is h0.seq.modlist[2]
    assert losses.fusable_head(models.MLP(8, 4, 2, 2, activation=nn.ReLU(inplace=True))) == "mlp2"
    assert losses.fusable_head(nn.Linear(8, 3)) == "linear"


def test_fusable_head_rejects_everything_else():
    from glass_amd import losses, models
    elu = lambda: nn.ELU(inplace=True)  # noqa: E731
    for layers in (1, 3):
        assert losses.fusable_head(models.MLP(8, 4, 2, layers, dropout=0.4, activation=elu())) is None
    assert losses.fusable_head(models.MLP(8, 4, 2, 2, activation=elu(), gn=True)) is None
    assert losses.fusable_head(models.MLP(8, 4, 2, 2, dropout=0.4, activation=elu(), tail_activation=True)) is None
    assert losses.fusable_head(models.MLP(8, 4, 2, 2, activation=elu(), tail_activation=True)) is None
    assert losses.fusable_head(models.MLP(8, 4, 2, 2, activation=nn.Tanh())) is None          # a foreign activation
    assert losses.fusable_head(models.MLP(8, 4, 2, 2, activation=nn.ELU(alpha=0.5))) is None
    for which in (0, -1):                                                                    # a bias-less Linear
        m = models.MLP(8, 4, 2, 2, dropout=0.4, activation=elu())
        m.seq.modlist[which].bias = None
        assert losses.fusable_head(m) is None
    assert losses.fusable_head(nn.Linear(8, 3, bias=False)) is None
    assert losses.fusable_head(models.Linear(8, 3)) is None          # (not the bare nn.Linear of the GLASS driver)
    assert losses.fusable_head(nn.Sequential(nn.Linear(8, 4), nn.ELU(), nn.Linear(4, 2))) is None


def test_head_call_id_is_its_own_stream():
    """The head's dropout stream is none of the convolutions' (1, 16 (l + 1), 16 (l + 1) + 1) nor the pair head's (2)."""
    from glass_amd import losses
    taken = {1, 2} | {16 * (l + 1) + d for l in range(64) for d in (0, 1)}
    assert losses.HEAD_MLP_CALL_ID not in taken


def test_header_table_and_library_agree_on_the_three_entries():
    from glass_amd import _lib
    text = open(os.path.join(ROOT, "include", "glass_hip.h")).read()
    assert "impl/models.py:56-80" in text and "GNNSeg.py:272-277" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, code), f"{n} not declared"
        assert n in _lib.SIGNATURES and hasattr(lib, n)
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[n][1]), n
    assert "head_mlp.hip" in open(os.path.join(ROOT, "glass_amd", "csrc", "Makefile")).read()


def _args():
    """Valid argument lists (host buffers: every call below is refused before a launch) as dicts by position name."""
    x = np.zeros(4096, dtype=np.float32)
    p = x.ctypes.data
    fwd = dict(pooled=p, ldp=8, W1=p, b1=p, W2=p, b2=p, target=p, mode=0, act=1, p_drop=0.0, rng=None, call_id=3, B=2, C=8,
               Hd=4, K=3, hidden_pre=p, logits=p, prob=p, loss=p, stream=None)
    bwd = dict(pooled=p, ldp=8, W1=p, W2=p, hidden_pre=p, prob=p, target=p, mode=0, act=1, p_drop=0.0, rng=None, call_id=3,
               grad_loss=p, B=2, C=8, Hd=4, K=3, ws=p, dpooled=p, lddp=8, dW1=p, db1=p, dW2=p, db2=p, accumulate=0, stream=None)
    ev = dict(pooled=p, ldp=8, W1=p, b1=p, W2=p, b2=p, act=1, B=2, C=8, Hd=4, K=3, logits=p, ldl=3, stream=None)
    return x, {NAMES[0]: fwd, NAMES[1]: bwd, NAMES[2]: ev}


CASES = [("null pointer", dict(W1=None), E_ARG), ("K = 0", dict(K=0), E_ARG), ("ldp < C", dict(ldp=7), E_ARG),
         ("B = 0", dict(B=0), E_ARG), ("Hd = 0", dict(Hd=0), E_ARG),
         ("K = 257", dict(K=257), E_UNSUPPORTED), ("Hd = 1025", dict(Hd=1025), E_UNSUPPORTED),
         ("unknown activation", dict(act=7), E_UNSUPPORTED), ("unknown mode", dict(mode=2), E_UNSUPPORTED),
         ("dropout without the rng words", dict(p_drop=0.4), E_ARG), ("p = 1", dict(p_drop=1.0, rng=1), E_ARG)]


@pytest.mark.parametrize("what,change,code", CASES, ids=[c[0] for c in CASES])
def test_validation_returns_codes_not_exceptions(what, change, code):
    from glass_amd import _lib
    lib = _lib.load()
    keep, table = _args()
    for name, args in table.items():
        if not set(change) <= set(args):
            continue  # (the evaluation entry has no mode / dropout)
        if "rng" in change:
            change = dict(change, rng=keep.ctypes.data)
        rc = getattr(lib, name)(*dict(args, **change).values())
        assert rc == code, (name, what, rc, lib.glass_last_error_string())
        assert b"head_mlp" in lib.glass_last_error_string()


def test_limits_themselves_pass_the_size_checks():
    """K = 256 and Hd = 1024 are inside: with them the only complaint left is the null pointer planted here."""
    from glass_amd import _lib
    lib = _lib.load()
    _keep, table = _args()
    for name, args in table.items():
        rc = getattr(lib, name)(*dict(args, K=256, Hd=1024, pooled=None).values())
        assert rc == E_ARG and b"null pointer" in lib.glass_last_error_string()


def test_gnn_offers_loss_and_logits_and_the_loop_uses_it():
    import inspect
    from glass_amd import seg, train, losses
    assert list(inspect.signature(seg.GNN.loss_and_logits).parameters) == ["self", "x", "edge_index", "edge_weight",
                                                                           "subG_node", "y", "loss_fn"]
    assert "loss_and_logits" in inspect.getsource(train.train) and "_glass_no_fuse" in inspect.getsource(train.train)
    assert issubclass(losses.MLPHeadLossFn, torch.autograd.Function) and callable(losses.mlp_head_loss)
