"""GNN-seg baseline driver on the MI355X path — same command line, control flow and log lines as the reference's
GNNSeg.py (flags 186-194, split 213-249, buildModel 252-274, test 277-355, best hyper-parameters 358-394):

    python GNNSeg.py --test --repeat 10 --device 0 --dataset density

Every subgraph is cut out of the base graph as its induced subgraph and batched block-diagonally by the HIP kernels of
glass_amd/seg.py.  Extensions: `--epochs` (default 500) caps the epochs of a repeat; `--dataset synthetic:<w>` selects
a seeded synthetic graph (glass_amd/synth.py) run with the hyper-parameters and convolution of `<w>`; `--hop K` (default
0, the reference's value) grows every subgraph into the radius-K in-ball of its nodes (todatalist(gd, hop)); `--pool
{ball,centre}` (default ball, the reference's readout over every node of the ball) — centre pools over the subgraph's
own nodes only, the ones the reference marks in Data.pos, and leaves the rest of the ball as context for the message
passing; at hop 0 the two are the same run; `--graph_norm {batch,graph}` (default batch, the reference's GraphNorm
over all rows of a batch) — graph normalises every subgraph over its own rows, so its prediction does not depend on the
subgraphs batched with it.  GPU only.
"""
import argparse
import functools

import numpy as np
import torch
import torch.nn as nn
from torch.nn import BCEWithLogitsLoss, CrossEntropyLoss
from torch.optim import Adam, lr_scheduler

import datasets
from glass_amd import ops, seg
from impl import config, metrics, models, train

DEGREE_FEATURE_SETS = ("hpo_metab", "hpo_neuro", "ppi_bp", "em_user")
ONE_FEATURE_SETS = ("component", "coreness", "density", "cut_ratio")

best_hyperparams = {
    "density": {"conv_layer": 1, "dropout": 0.4, "hidden_dim": 16},
    "component": {"conv_layer": 1, "dropout": 0.0, "hidden_dim": 16},
    "coreness": {"conv_layer": 1, "dropout": 0.3, "hidden_dim": 16},
    "cut_ratio": {"conv_layer": 1, "dropout": 0.1, "hidden_dim": 4},
    "hpo_neuro": {"conv_layer": 1, "dropout": 0.4, "hidden_dim": 64},
    "ppi_bp": {"conv_layer": 8, "dropout": 0.4, "hidden_dim": 64},
    "hpo_metab": {"conv_layer": 1, "dropout": 0.1, "hidden_dim": 64},
    "em_user": {"conv_layer": 1, "dropout": 0.4, "hidden_dim": 64},
}


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="")
    p.add_argument("--dataset", type=str, default="ppi_bp")
    p.add_argument("--repeat", type=int, default=1)
    p.add_argument("--test", action="store_true")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--epochs", type=int, default=500, help="(extension) cap on epochs per repeat")
    p.add_argument("--hop", type=int, default=0, help="(extension) k_hop_subgraph hops of every subgraph")
    p.add_argument("--pool", type=str, default="ball", choices=("ball", "centre"),
                   help="(extension) readout over the whole ball, or over the subgraph's own nodes")
    p.add_argument("--graph_norm", type=str, default="batch", choices=("batch", "graph"),
                   help="(extension) GraphNorm statistics over the whole batch, or over each subgraph's own rows")
    p.add_argument("--class_weight", type=str, default="none", choices=("none", "balanced"),
                   help="(extension) balanced: class weights (multi-class) / pos_weight (binary, multi-label) from the training "
                        "split's label counts, applied inside the fused head + loss (default: none)")
    return p.parse_args(argv)


def base_name(dataset):
    """The entry of the hyper-parameter table (and of the feature / convolution rules) a dataset name uses."""
    name = dataset.split(":", 1)[1] if dataset.startswith("synthetic:") else dataset
    if name not in best_hyperparams:
        raise NotImplementedError(f"GNN-seg has no hyper-parameters for {dataset!r}")
    return name


def conv_mode(dataset):
    """GIN for density, GCN (without self-loops) for every other set (GNNSeg.py:256-257)."""
    return "gin" if base_name(dataset) == "density" else "gcn"


def set_seed(seed: int):
    print("seed ", seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    if torch.cuda.is_available():
        # the head's dropout masks come from the device-resident stream (losses.mlp_head_loss): a repeat stays a function of its seed
        on_gpu = config.device is not None and config.device.type == "cuda"
        ops.rng_seed(seed, config.device if on_gpu else "cuda")


class Run:
    """State the reference keeps in module globals (baseG, datasets, task type)."""
    def __init__(self, args):
        self.args = args
        self.name = base_name(args.dataset)
        self.mode = conv_mode(args.dataset)
        g = datasets.load_dataset(args.dataset)
        if g.y.unique().shape[0] == 2:
            def loss_fn(x, y):
                return BCEWithLogitsLoss()(x.flatten(), y.flatten())

            g.y = g.y.to(torch.float)
            self.loss_fn = loss_fn
            self.output_channels = g.y.shape[1] if g.y.ndim > 1 else 1
            self.score_fn = metrics.binaryf1
        else:
            g.y = g.y.to(torch.int64)
            self.loss_fn = CrossEntropyLoss()
            self.output_channels = g.y.unique().shape[0]
            self.score_fn = metrics.microf1
        self.baseG = g
        self.trn = self.val = self.tst = None
        self.input_channels = 1

    def split(self):
        g = self.baseG
        if self.name in DEGREE_FEATURE_SETS:
            g.addDegreeFeature()
        elif self.name in ONE_FEATURE_SETS:
            g.addOneFeature()
        else:
            raise NotImplementedError
        self.input_channels = g.x.shape[-1]
        g.to(config.device)
        base = seg.SegBase(g.edge_index, g.edge_attr, g.x.shape[0])
        self.trn, self.val, self.tst = (seg.GsDataset(*g.get_split(s), mode=self.mode, base=base, hop=self.args.hop,
                                                      pool=self.args.pool)
                                        for s in ("train", "valid", "test"))
        if getattr(self.args, "class_weight", "none") == "balanced":
            # weights from the TRAINING split only; the marker classes carry them into the fused head (losses.fusable_spec)
            from glass_amd import losses
            self.loss_fn = losses.balanced_loss(g.get_split("train")[-1], self.output_channels).to(config.device)

    def loaders(self, batch_size):
        return (seg.GsDataloader(self.trn, batch_size, shuffle=True, drop_last=True),
                seg.GsDataloader(self.val, batch_size, shuffle=False, drop_last=False),
                seg.GsDataloader(self.tst, batch_size, shuffle=False, drop_last=False))

    def build_model(self, hidden_dim, conv_layer, dropout):
        conv = seg.GConv(self.input_channels, hidden_dim, hidden_dim, conv_layer,
                         conv=seg.MyGINConv if self.mode == "gin" else functools.partial(seg.GCNConv, add_self_loops=False),
                         activation=nn.ELU(inplace=True), dropout=dropout,
                         graph_norm=getattr(getattr(self, "args", None), "graph_norm", "batch"))
        mlp = models.MLP(hidden_dim * conv_layer, hidden_dim, self.output_channels, 2, dropout=dropout,
                         activation=nn.ELU(inplace=True))
        return seg.GNN(conv, mlp, aggr="sum").to(config.device)

    def test(self, hidden_dim=64, conv_layer=8, dropout=0.3, lr=1e-3, batch_size=160):
        trn_loader, val_loader, tst_loader = self.loaders(batch_size)
        outs = []

        def evaluate(loader):
            return train.test(gnn, loader, self.score_fn, loss_fn=self.loss_fn)[0]

        for r in range(self.args.repeat):
            print(f"repeat {r}")
            set_seed(r)
            gnn = self.build_model(hidden_dim, conv_layer, dropout)
            optimizer = Adam(gnn.parameters(), lr=lr)
            scd = lr_scheduler.ReduceLROnPlateau(optimizer, factor=0.7, min_lr=5e-5)
            val_score, early_stop, tst_score = 0, 0, 0
            for i in range(self.args.epochs):
                loss = train.train(optimizer, gnn, trn_loader, self.loss_fn)
                scd.step(loss)
                if i % 5 == 0:
                    score = evaluate(val_loader)
                    early_stop += 1
                    if score > val_score:
                        val_score = score
                        tst_score = evaluate(tst_loader)
                        print(f"iter {i} loss {loss:.4f} val {val_score:.4f} tst {tst_score:.4f}", flush=True)
                        early_stop /= 2
                    elif score >= val_score - 1e-5:
                        score = evaluate(tst_loader)
                        tst_score = max(score, tst_score)
                        print(f"iter {i} loss {loss:.4f} val {val_score:.4f} tst {score:.4f}", flush=True)
                        early_stop /= 2
                    else:
                        print(f"iter {i} loss {loss:.4f} val {score:.4f} tst {evaluate(tst_loader):.4f}", flush=True)
                    if early_stop > 10:
                        break
            print(f"end: val {val_score:.4f} tst {tst_score:.4f}", flush=True)
            outs.append(tst_score)
        print("tst scores", outs)
        print(np.average(outs), np.std(outs) / np.sqrt(len(outs)))
        return np.average(outs)


def main(argv=None):
    args = parse_args(argv)
    config.set_device(args.device)
    if config.device.type != "cuda":
        raise SystemExit("this driver runs the MI355X HIP path only; use the reference itself for --device -1")
    bhp = best_hyperparams[base_name(args.dataset)]
    run = Run(args)
    print(args)
    run.split()
    print(run.test(**bhp, batch_size=len(run.tst)))
    print("best params", bhp, flush=True)


if __name__ == "__main__":
    main()
