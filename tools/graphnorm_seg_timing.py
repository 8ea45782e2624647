"""Time of the per-graph GraphNorm entries (glass_graphnorm_seg_fwd_f32 / _bwd_f32) and of the whole-batch entries
(glass_graphnorm_fwd_f32 / _bwd_f32) on the same tensor: one GNN-seg training batch of the shipped density set, cut by the
driver's own loader (GNNSeg.py trains with batch_size = size of the test split), at hidden width --hidden (default 64).

usage: python tools/graphnorm_seg_timing.py [--hidden 64] [--calls 200] [--rounds 7] [--warmup 20]

Per entry: `--rounds` windows of `--calls` back-to-back launches between two device events, the four entries alternating
round by round, after `--warmup` untimed calls each; one JSON line with the median / min / max window mean in microseconds
per call, the algorithmic bytes (forward 2 n C 4, backward 3 n C 4) and the rate they amount to.  These are times per CALL
in a stream of calls (2-3 launches each for the whole-batch form, 1 forward / 2 backward for the per-graph form); kernel
times come from running the same script with --calls 20 --rounds 1 under `rocprofv3 --kernel-trace --stats -- python ...`."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--hidden", type=int, default=64)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--warmup", type=int, default=20)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.chdir(ROOT)

import torch  # noqa: E402
import GNNSeg  # noqa: E402
from impl import config  # noqa: E402
from glass_amd import _lib  # noqa: E402


def main():
    config.set_device(0)
    GNNSeg.set_seed(0)
    run = GNNSeg.Run(GNNSeg.parse_args(["--dataset", "density"]))
    run.split()
    bx, adj, _, _, _ = next(iter(run.loaders(len(run.tst))[0]))
    n, C, B = int(bx.shape[0]), args.hidden, int(adj.seg_ptr.shape[0]) - 1
    sizes = (adj.seg_ptr[1:] - adj.seg_ptr[:-1]).cpu()
    dev = bx.device
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    gen = torch.Generator().manual_seed(0)
    x = (torch.randn(n, C, generator=gen) * 2 + 5).to(dev)
    dy = torch.randn(n, C, generator=gen).to(dev)
    gamma, beta, alpha = (torch.ones(C, device=dev), torch.zeros(C, device=dev), torch.full((C, ), 0.9, device=dev))
    y, dx = torch.empty_like(x), torch.empty_like(x)
    dpar = torch.empty(3, C, device=dev)
    stats = torch.empty(2, B, C, device=dev)
    saved = torch.empty(4 * C, device=dev)
    ws_seg = torch.empty(lib.glass_graphnorm_seg_ws_bytes(B, C) + 16, dtype=torch.uint8, device=dev)
    ws_all = torch.empty(lib.glass_graphnorm_ws_bytes(n, C) + 16, dtype=torch.uint8, device=dev)
    P = lambda t: t.data_ptr()
    act = _lib.ACT_ELU
    entries = {
        "seg_fwd": lambda: lib.glass_graphnorm_seg_fwd_f32(P(x), C, P(y), C, P(adj.seg_ptr), B, C, P(gamma), P(beta), P(alpha), 1e-5,
                                                           P(stats[0]), P(stats[1]), act, st),
        "seg_bwd": lambda: lib.glass_graphnorm_seg_bwd_f32(P(dy), C, P(x), C, P(dx), C, P(adj.seg_ptr), B, C, P(gamma), P(beta),
                                                           P(alpha), P(stats[0]), P(stats[1]), P(dpar[0]), P(dpar[1]), P(dpar[2]),
                                                           0, act, P(ws_seg), st),
        "batch_fwd": lambda: lib.glass_graphnorm_fwd_f32(P(x), C, P(y), C, n, C, P(gamma), P(beta), P(alpha), 1e-5, P(saved), act,
                                                         0.0, None, 0, P(ws_all), st),
        "batch_bwd": lambda: lib.glass_graphnorm_bwd_f32(P(dy), C, P(x), C, P(dx), C, None, 0, n, C, P(gamma), P(alpha), P(saved),
                                                         P(dpar[0]), P(dpar[1]), P(dpar[2]), 0, act, 0.0, None, 0, P(ws_all), st),
    }
    for name, fn in entries.items():
        for _ in range(args.warmup):
            _lib.check(fn(), name)
    torch.cuda.synchronize()
    times = {name: [] for name in entries}
    for _ in range(args.rounds):
        for name, fn in entries.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / args.calls)
    print(json.dumps(dict(dataset="density", rows=n, segments=B, hidden=C, rows_per_segment_min_median_max=[
        int(sizes.min()), float(sizes.double().median()), int(sizes.max())], lds_rows=lib.glass_graphnorm_seg_lds_rows(C),
        calls=args.calls, rounds=args.rounds)), flush=True)
    for name, t in times.items():
        nbytes = (2 if name.endswith("fwd") else 3) * n * C * 4
        med = statistics.median(t)
        print(json.dumps(dict(entry=name, us_per_call_median_min_max=[round(v, 3) for v in (med, min(t), max(t))],
                              algorithmic_bytes=nbytes, gb_per_s=round(nbytes / med / 1e3, 2))), flush=True)


if __name__ == "__main__":
    main()
