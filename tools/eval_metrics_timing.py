"""Time of one evaluation (glass_amd.train.test: forward passes, metric, loss) with the metric counted on the GPU and with
the metric on the host, on the shipped density validation split with the GLASSTest.py model (config/density.yml) and on
synthetic:ppi_bp (config/synthetic_ppi_bp.yml, 6 classes).

usage: [GLASS_EVAL_METRICS=0|1] python tools/eval_metrics_timing.py [--root DIR] [--datasets density,synthetic:ppi_bp]
                                                                     [--calls 30] [--warmup 3] [--tag T]

--root DIR imports the drivers and glass_amd from another checkout (a build of the parent commit), so that two trees can be
timed in alternation in one session.  Per data set one JSON line: the median / min / max of `--calls` synchronised
train.test calls after `--warmup` untimed ones, the host metric's own time on the same predictions (median of `--calls`
calls on the arrays train.test hands a metric) and, where the tree has it, the time of metrics.device_score alone."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--datasets", default="density,synthetic:ppi_bp")
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--tag", default="")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
os.chdir(ROOT)

import torch  # noqa: E402
import yaml  # noqa: E402
import GLASSTest  # noqa: E402
from impl import config, train  # noqa: E402
from glass_amd import metrics as gmetrics, train as gtrain  # noqa: E402


def timed(fn, calls, warmup):
    """(median, min, max) milliseconds of fn(), each call closed by a device synchronise."""
    out = []
    for k in range(warmup + calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return [round(v, 4) for v in (statistics.median(out), min(out), max(out))]


def main():
    config.set_device(0)
    for name in args.datasets.split(","):
        a = GLASSTest.parse_args(["--use_one", "--use_seed", "--use_maxzeroone", "--device", "0", "--dataset", name])
        with open(os.path.join(ROOT, "config", name.replace(":", "_") + ".yml")) as f:
            p = yaml.safe_load(f)
        GLASSTest.set_seed(0)
        run = GLASSTest.Run(a)
        run.split()
        model = run.build_model(p["hidden_dim"], p["conv_layer"], p["dropout"], 1, p["pool"], p["z_ratio"], p["aggr"])
        val = run.loaders(p["batch_size"])[1]
        test_ms = timed(lambda: train.test(model, val, run.score_fn, loss_fn=run.loss_fn), args.calls, args.warmup)
        score = train.test(model, val, run.score_fn, loss_fn=run.loss_fn)[0]
        # the arrays a metric is handed on the host path, and the tensors the device path reads
        (pred, y), _ = train.test(model, val, lambda q, t: (q, t), loss_fn=run.loss_fn)
        host_ms = timed(lambda: run.score_fn(pred, y), args.calls, args.warmup)
        dev_ms = None
        if hasattr(gmetrics, "device_score"):
            pt, yt = torch.from_numpy(pred).cuda(), torch.from_numpy(y).cuda()
            dev_ms = timed(lambda: gmetrics.device_score(run.score_fn, pt, yt), args.calls, args.warmup)
        print(json.dumps(dict(tag=args.tag, dataset=name, device_metrics=bool(getattr(gtrain, "USE_EVAL_METRICS", False)),
                              rows=int(pred.shape[0]), columns=int(pred.shape[1]), batches=len(val), score=float(score),
                              test_ms_median_min_max=test_ms, host_metric_ms_median_min_max=host_ms,
                              device_score_ms_median_min_max=dev_ms, calls=args.calls, warmup=args.warmup)), flush=True)


if __name__ == "__main__":
    main()
