"""GLASS training driver on the MI355X path — same command line, YAML keys, control flow and log
lines as the reference's GLASSTest.py (flags 14-30, split 77-126, buildModel 129-175, test 178-269):

    python GLASSTest.py --use_one --use_seed --use_maxzeroone --repeat 1 --device 0 --dataset density

It builds what the reference builds — `Adam(gnn.parameters(), lr)`, `ReduceLROnPlateau`, the binary loss as a function
around `BCEWithLogitsLoss`, `CrossEntropyLoss()` — and nothing of glass_amd by name: `impl.train.train` itself moves such a
caller onto the captured step program (flat parameter arena, fused Adam, fused head + loss; glass_amd/optim.py `adopt`,
glass_amd/losses.py `fusable_mode`).  The reference's own GLASSTest.py run against this repo's `impl/` gets the same path.
Extension: `--dataset synthetic:<workload>` selects a seeded synthetic graph (glass_amd/synth.py).  GPU only:
`--device -1` stops with an error.
"""
import argparse
import functools
import random
import time

import numpy as np
import torch
import torch.nn as nn
import yaml
from torch.nn import BCEWithLogitsLoss, CrossEntropyLoss
from torch.optim import Adam, lr_scheduler

import datasets
from impl import SubGDataset, config, metrics, models, train, utils

SYNTHETIC_SETS = ("density", "component", "cut_ratio", "coreness")
POOLS = {"mean": models.MeanPool, "max": models.MaxPool, "sum": models.AddPool, "size": models.SizePool,
         "attn": models.AttnPool}  # attn (extension): a learned readout, constructed with the pooled width


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="")
    p.add_argument("--dataset", type=str, default="ppi_bp")
    # node features: degree rank, all-ones, or pretrained node-id embeddings from ./Emb
    p.add_argument("--use_deg", action="store_true")
    p.add_argument("--use_one", action="store_true")
    p.add_argument("--use_nodeid", action="store_true")
    p.add_argument("--use_maxzeroone", action="store_true")
    p.add_argument("--use_zeroone", action="store_true",
                   help="(extension) exact zero-one labels: every subgraph of a batch labeled on its own replica of the graph "
                        "(utils.ZeroOneZ; about batch-size times the work and memory of --use_maxzeroone)")
    p.add_argument("--repeat", type=int, default=1)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--use_seed", action="store_true")
    p.add_argument("--max_epoch", type=int, default=300, help="(extension) cap on epochs per repeat")
    p.add_argument("--clip", type=float, default=None,
                   help="(extension) clip the gradient's global L2 norm to this value before every Adam update (default: off)")
    p.add_argument("--class_weight", type=str, default="none", choices=("none", "balanced"),
                   help="(extension) balanced: class weights (multi-class) / pos_weight (binary, multi-label) from the training "
                        "split's label counts, applied inside the fused loss (default: none)")
    p.add_argument("--pool", type=str, default=None, choices=tuple(POOLS),
                   help="(extension) readout instead of the config file's `pool` (default: the config's value)")
    p.add_argument("--aggr", type=str, default=None, choices=("mean", "sum", "gcn", "max", "softmax", "gat", "gatv2", "std", "var", "pna"),
                   help="(extension) neighbour aggregation instead of the config file's `aggr` (default: the config's value); "
                        "max: the largest weighted neighbour message per channel; softmax: the softmax-weighted mean of the "
                        "messages with a learned temperature per layer (positive edge weights); gat: attention (--gat_heads heads), "
                        "the weights from two learned vectors per layer (positive edge weights); gatv2: dynamic attention, one head, the "
                        "score of an edge from one learned vector per layer applied after the non-linearity (positive edge weights); std / var: the weighted standard "
                        "deviation / variance of the messages (positive edge weights); pna: mean, max, min and standard deviation of the "
                        "messages under three degree scalers, mixed per channel by a learned [12, hidden] weight per layer "
                        "(positive edge weights); none of the seven is available "
                        "with --use_zeroone")
    p.add_argument("--gat_slope", type=float, default=0.2,
                   help="(extension) LeakyReLU's negative slope in the attention scores of --aggr gat and gatv2 (default: 0.2)")
    p.add_argument("--gat_heads", type=int, default=1,
                   help="(extension) attention heads of --aggr gat: they partition the hidden channels, so the count must divide "
                        "hidden_dim and leave a power of two in [4, 256] channels per head (default: 1)")
    p.add_argument("--edge_saliency", type=str, default=None, metavar="PATH",
                   help="(extension) after the last repeat write PATH (.npy, one fp32 per edge of the graph): the mean over the "
                        "test split's batches of |d loss / d edge_weight| of the trained model; aggregations mean, sum and gcn "
                        "only, not with --use_zeroone")
    p.add_argument("--edge_dropout", type=float, default=None, metavar="P",
                   help="(extension) edge dropout (DropEdge): every training step each layer drops a random share P in [0, 1) of "
                        "the adjacency entries, drawn on the GPU, undirected edges as one (default: the config file's "
                        "`edge_dropout`, else 0); aggregations mean, sum and gcn only, not with --use_zeroone or --edge_saliency")
    args = p.parse_args(argv)
    if args.edge_dropout is not None and not (0.0 <= args.edge_dropout < 1.0):
        p.error("--edge_dropout must lie in [0, 1)")
    if args.edge_dropout and args.use_zeroone:
        p.error("--edge_dropout is not available with --use_zeroone (no edge dropout on the replicated path)")
    if args.edge_dropout and args.edge_saliency is not None:
        p.error("--edge_dropout is not available with --edge_saliency (edge dropout and live edge weights exclude each other)")
    if args.edge_dropout and args.aggr not in (None, "mean", "sum", "gcn"):
        p.error(f"--edge_dropout needs --aggr mean, sum or gcn ({args.aggr} needs a dropped edge excluded, not weighted zero)")
    if args.edge_saliency is not None and args.use_zeroone:
        p.error("--edge_saliency is not available with --use_zeroone (no edge-weight gradient on the replicated path)")
    if args.edge_saliency is not None and args.aggr not in (None, "mean", "sum", "gcn"):
        p.error(f"--edge_saliency needs --aggr mean, sum or gcn (no edge-weight gradient for {args.aggr})")
    if args.gat_heads < 1:
        p.error("--gat_heads must be an integer >= 1")
    if args.use_zeroone and args.use_maxzeroone:
        p.error("--use_zeroone and --use_maxzeroone are mutually exclusive")
    if args.clip is not None and not args.clip > 0:
        p.error("--clip must be positive")
    if args.gat_slope != args.gat_slope:
        p.error("--gat_slope must be a number")
    return args


def set_seed(seed: int):
    print("seed ", seed)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)


class Run:
    """State the reference keeps in module globals (baseG, datasets, loaders, task type)."""
    def __init__(self, args):
        self.args = args
        base = datasets.load_dataset(args.dataset)
        if base.y.unique().shape[0] == 2:  # binary / multi-label: BCE on flattened logits + micro-F1 of (logit > 0)
            def loss_fn(x, y):  # (the reference's function, GLASSTest.py:57-58; the training step recognises what it computes)
                return BCEWithLogitsLoss()(x.flatten(), y.flatten())

            self.loss_fn = loss_fn
            self.output_channels = base.y.shape[1] if base.y.ndim > 1 else 1
            self.score_fn = metrics.binaryf1
        else:  # multi-class
            self.loss_fn = CrossEntropyLoss()
            self.output_channels = base.y.unique().shape[0]
            self.score_fn = metrics.microf1
        self.max_deg = 0
        self.trn = self.val = self.tst = None

    def split(self):
        """Load, pick the node feature, move to the device, split (reference split(), 77-126)."""
        a = self.args
        g = datasets.load_dataset(a.dataset)
        g.y = g.y.to(torch.float) if g.y.unique().shape[0] == 2 else g.y.to(torch.int64)
        if a.use_deg:
            g.setDegreeFeature()
        elif a.use_one:
            g.setOneFeature()
        elif a.use_nodeid:
            g.setNodeIdFeature()
        else:
            raise NotImplementedError
        self.max_deg = torch.max(g.x)
        g.to(config.device)
        self.trn = SubGDataset.GDataset(*g.get_split("train"))
        self.val = SubGDataset.GDataset(*g.get_split("valid"))
        self.tst = SubGDataset.GDataset(*g.get_split("test"))
        if getattr(a, "class_weight", "none") == "balanced":
            # weights from the TRAINING split only; the marker classes carry them into the captured step (losses.fusable_spec)
            from glass_amd import losses
            self.loss_fn = losses.balanced_loss(self.trn.y, self.output_channels).to(config.device)

    def loaders(self, batch_size):
        """(train, valid, test) loaders.  With --use_maxzeroone every batch is labeled by utils.MaxZOZ and the training
        loader drops the last partial batch (--use_zeroone: the same with utils.ZeroOneZ); without it plain loaders are used and nothing is dropped.  All shuffle."""
        if self.args.use_maxzeroone or getattr(self.args, "use_zeroone", False):
            z_fn = utils.ZeroOneZ if getattr(self.args, "use_zeroone", False) else utils.MaxZOZ
            make = functools.partial(SubGDataset.ZGDataloader, z_fn=z_fn, shuffle=True)
            # (under torch.distributed the TRAINING loader hands every rank its slice of each batch — subgraph-batch data
            # parallelism, glass_amd/dist.py; evaluation loaders are never sharded, so scores agree on every rank)
            from glass_amd import dist as gdist
            return (make(self.trn, batch_size, drop_last=True, shard=gdist.is_distributed()),
                    make(self.val, batch_size, drop_last=False), make(self.tst, batch_size, drop_last=False))
        from glass_amd import dist as gdist
        return (SubGDataset.GDataloader(self.trn, batch_size, shuffle=True, drop_last=False, shard=gdist.is_distributed()),
                SubGDataset.GDataloader(self.val, batch_size, shuffle=True, drop_last=False),
                SubGDataset.GDataloader(self.tst, batch_size, shuffle=True, drop_last=False))

    def build_model(self, hidden_dim, conv_layer, dropout, jk, pool, z_ratio, aggr, gat_heads=None, edge_dropout=0.0):
        a = self.args
        if pool not in POOLS:
            raise NotImplementedError

        def build(h):
            conv = models.EmbZGConv(h, h, conv_layer, max_deg=self.max_deg,
                                    activation=nn.ELU(inplace=True), jk=jk, dropout=dropout,
                                    conv=functools.partial(models.GLASSConv, aggr=aggr, z_ratio=z_ratio, dropout=dropout,
                                                           gat_slope=getattr(a, "gat_slope", 0.2),
                                                           gat_heads=getattr(a, "gat_heads", 1) if gat_heads is None else gat_heads,
                                                           edge_dropout=edge_dropout),
                                    gn=True)
            if a.use_nodeid:
                print("load ", f"./Emb/{a.dataset}_{hidden_dim}.pt")
                emb = torch.load(f"./Emb/{a.dataset}_{hidden_dim}.pt", map_location=torch.device("cpu")).detach()
                if h > emb.shape[1]:  # (a width no kernel family serves runs zero-padded: glass_amd/widths.py)
                    emb = torch.nn.functional.pad(emb, (0, h - emb.shape[1]))
                conv.input_emb = nn.Embedding.from_pretrained(emb, freeze=False)
            width = h * conv_layer if jk else h  # what the readout hands the head
            mlp = nn.Linear(width, self.output_channels)
            pool_fn = POOLS[pool](width) if pool == "attn" else POOLS[pool]()
            return models.GLASS(conv, nn.ModuleList([mlp]), nn.ModuleList([pool_fn]))

        # widths outside the kernel families (every shipped config is inside) run at the next family width, zero padded: exact
        from glass_amd import widths
        return widths.build_at_fused_width(hidden_dim, build).to(config.device)

    def evaluate(self, model, loader):
        """Score of the task metric on one split."""
        return train.test(model, loader, self.score_fn, loss_fn=self.loss_fn)[0]

    def fit_once(self, model, optimizer, scheduler, loaders, warmup_epochs, patience):
        """One training run.  Validation starts after `warmup_epochs`; the test score is the one measured at the best
        validation score (ties within 1e-5 keep the larger test score).  Returns (epochs, seconds, val, test)."""
        trn_loader, val_loader, tst_loader = loaders
        policy = Patience(patience)
        seconds = 0.0
        epoch = 0
        for epoch in range(self.args.max_epoch):
            start = time.time()
            loss = train.train(optimizer, model, trn_loader, self.loss_fn)
            seconds += time.time() - start
            scheduler.step(loss)
            if epoch >= warmup_epochs:
                val = self.evaluate(model, val_loader)
                verdict = policy.judge(val)
                if verdict == "better":
                    policy.test_at_best = self.evaluate(model, tst_loader)
                    print(f"iter {epoch} loss {loss:.4f} val {policy.best_val:.4f} tst {policy.test_at_best:.4f}", flush=True)
                elif verdict == "tie":
                    tst = self.evaluate(model, tst_loader)
                    policy.test_at_best = max(tst, policy.test_at_best)
                    print(f"iter {epoch} loss {loss:.4f} val {policy.best_val:.4f} tst {tst:.4f}", flush=True)
                elif epoch % 10 == 0:  # worse: a progress line every tenth epoch only
                    print(f"iter {epoch} loss {loss:.4f} val {val:.4f} tst {self.evaluate(model, tst_loader):.4f}", flush=True)
            if policy.saturated():
                policy.strikes += 1
            if policy.exhausted():
                break
        return epoch + 1, seconds, policy.best_val, policy.test_at_best

    def test(self, pool="size", aggr="mean", hidden_dim=64, conv_layer=8, dropout=0.3, jk=1, lr=1e-3, z_ratio=0.8,
             batch_size=None, resi=0.7, gat_heads=None, edge_dropout=None):
        """Train `repeat` times with one hyper-parameter set (the YAML keys); prints the reference's log lines.  gat_heads (an
        extension key, aggr "gat" only): the attention heads; absent, --gat_heads.  edge_dropout (an extension key, aggr "mean" /
        "sum" / "gcn" only): the share of edges every layer drops per training step; absent, --edge_dropout, else 0."""
        if edge_dropout is None:
            edge_dropout = getattr(self.args, "edge_dropout", None) or 0.0
        # evaluation cadence: both the warm-up and the patience are 100 test-set batches' worth of epochs (synthetic
        # sets: a fifth of that)
        batches_in_test = self.tst.y.shape[0] / batch_size
        if self.args.dataset in SYNTHETIC_SETS:
            batches_in_test /= 5
        horizon = 100 / batches_in_test
        results = []
        for repeat in range(self.args.repeat):
            set_seed((1 << repeat) - 1)
            print(f"repeat {repeat}")
            self.split()
            model = self.build_model(hidden_dim, conv_layer, dropout, jk, pool, z_ratio, aggr, gat_heads, edge_dropout)
            optimizer = Adam(model.parameters(), lr=lr)  # (impl.train.train runs it as one fused launch inside the step's graph)
            if self.args.clip is not None:
                # torch keeps unknown group keys; the step reads this one (norm launch + clipped Adam inside the step's graph)
                optimizer.param_groups[0]["max_grad_norm"] = self.args.clip
            scheduler = lr_scheduler.ReduceLROnPlateau(optimizer, factor=resi, min_lr=5e-5)
            epochs, seconds, val, tst = self.fit_once(model, optimizer, scheduler, self.loaders(batch_size), horizon, horizon)
            print(f"end: epoch {epochs}, train time {seconds:.2f} s, val {val:.3f}, tst {tst:.3f}", flush=True)
            results.append(tst)
        print(f"average {np.average(results):.3f} error {np.std(results) / np.sqrt(len(results)):.3f}")
        if getattr(self.args, "edge_saliency", None) is not None and self.args.repeat > 0:
            self.write_edge_saliency(model, self.loaders(batch_size)[2], self.args.edge_saliency)
        return results

    def write_edge_saliency(self, model, tst_loader, path):
        """--edge_saliency: the mean over the test split's batches of |d loss / d edge_weight| of `model`, [E] fp32 as .npy."""
        from glass_amd import explain
        total, n_batches = None, 0
        for batch in tst_loader:
            x, ei, ea, pos = batch[:4]
            z = batch[4] if len(batch) > 5 else None
            g = explain.edge_saliency(model, x, ei, ea, pos, z, loss_fn=self.loss_fn, y=batch[-1]).abs()
            total = g if total is None else total + g
            n_batches += 1
        with open(path, "wb") as f:
            np.save(f, (total / n_batches).cpu().numpy().astype(np.float32))
        print(f"edge saliency of {n_batches} test batches -> {path}", flush=True)


class Patience:
    """Early-stop bookkeeping of the driver: an epoch is `better` (new best validation score), a `tie` (within 1e-5
    below the best) or `worse` (one strike).  A saturated validation score (>= 1 - 1e-5) also costs a strike per
    epoch.  More strikes than `limit` end the run; a better epoch clears them."""
    def __init__(self, limit):
        self.limit = limit
        self.best_val = 0
        self.test_at_best = 0
        self.strikes = 0

    def judge(self, val):
        if val > self.best_val:
            self.best_val, self.strikes = val, 0
            return "better"
        if val >= self.best_val - 1e-5:
            return "tie"
        self.strikes += 1
        return "worse"

    def saturated(self):
        return self.best_val >= 1 - 1e-5

    def exhausted(self):
        return self.strikes > self.limit


def main(argv=None):
    args = parse_args(argv)
    config.set_device(args.device)
    if config.device.type != "cuda":
        raise SystemExit("this driver runs the MI355X HIP path only; use the reference itself for --device -1")
    if args.use_seed:
        set_seed(0)
    run = Run(args)
    print(args)
    with open(f"config/{args.dataset.replace(':', '_')}.yml") as f:
        params = yaml.safe_load(f)
    print("params", params, flush=True)
    if args.pool is not None:
        params["pool"] = args.pool
    if args.aggr is not None:
        params["aggr"] = args.aggr
    if args.gat_heads != 1:  # (the flag, where given, instead of the config file's `gat_heads`)
        params["gat_heads"] = args.gat_heads
    if args.edge_dropout is not None:  # (the flag, where given, instead of the config file's `edge_dropout`)
        params["edge_dropout"] = args.edge_dropout
    if params.get("edge_dropout"):
        if params.get("aggr", "mean") not in ("mean", "sum", "gcn"):
            raise SystemExit(f"edge_dropout needs aggr mean, sum or gcn; the configuration says {params['aggr']!r} "
                             "(the other aggregations need a dropped edge excluded, not weighted zero)")
        if args.use_zeroone or args.edge_saliency is not None:
            raise SystemExit("edge_dropout is not available with --use_zeroone or --edge_saliency")
    if args.edge_saliency is not None and params.get("aggr", "mean") not in ("mean", "sum", "gcn"):
        raise SystemExit(f"--edge_saliency needs aggr mean, sum or gcn; the configuration says {params['aggr']!r} "
                         "(no edge-weight gradient for the other aggregations)")
    run.split()
    return run.test(**params)


if __name__ == "__main__":
    main()
