"""Time of one captured training step per pooling mode at the C2 shape (ppi_bp-shaped graph, hidden 64, two layers, batch
80 x 10, dropout 0.5, fused Adam): the step as bench.py replays it (TrainStep, hipGraph), for each of sum | mean | size | max.

usage: python tools/pool_step_timing.py [--root DIR] [--pools sum,mean,size,max] [--steps 300] [--repeats 7]

--root DIR imports glass_amd from another checkout (a build of the parent commit), so that two trees can be timed in
alternation from one shell script in one session.  Prints one JSON line per pool: median / min / max ms per step over the
repeats, and whether the step ran as the step program (stack.step_supported) or as the captured per-op step."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--pools", default="sum,mean,size,max")
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from glass_amd import losses, synth  # noqa: E402
from glass_amd.arena import ParamArena  # noqa: E402
from glass_amd.factory import build_glass  # noqa: E402
from glass_amd.optim import FlatAdam  # noqa: E402
from glass_amd.step import TrainStep  # noqa: E402


def main():
    dev = "cuda:0"
    w, ei, ew, x, pos, y = synth.make_workload("ppi_bp", seed=0, n_batches=4)
    ei, ew, x, pos, y = (torch.from_numpy(a).to(dev) for a in (ei, ew, x, pos, y))
    B = w.batch
    loss_fn = losses.BCEWithLogits() if w.multilabel else losses.CrossEntropy()
    for pool in args.pools.split(","):
        torch.manual_seed(0)
        model = build_glass(w.hidden, w.layers, int(x.max()), w.n_class, w.aggr, pool, w.z_ratio, dropout=w.dropout).to(dev).train()
        arena = ParamArena(model)
        step = TrainStep(model, FlatAdam(arena, lr=w.lr), loss_fn, x, ei, ew, arena, use_graph=True)
        for k in range(20):  # capture + warm replays of every batch shape used below
            step(pos[(k % 4) * B:(k % 4 + 1) * B], y[(k % 4) * B:(k % 4 + 1) * B])
        torch.cuda.synchronize()
        per_step = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            for k in range(args.steps):
                b = k % 4
                step(pos[b * B:(b + 1) * B], y[b * B:(b + 1) * B])
            torch.cuda.synchronize()
            per_step.append((time.perf_counter() - t0) / args.steps * 1e3)
        loss = float(step(pos[:B], y[:B]))
        print(json.dumps(dict(tag=args.tag, pool=pool, ms_median=round(statistics.median(per_step), 4), ms_min=round(min(per_step), 4),
                              ms_max=round(max(per_step), 4), graphed=bool(step.graphed), step_program=bool(step._program_step()),
                              steps=args.steps, repeats=args.repeats, loss=loss)), flush=True)


if __name__ == "__main__":
    main()
