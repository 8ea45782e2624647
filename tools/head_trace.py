"""Phase timeline of the head launch of a replayed training step (laboratory tool; step_head_kernel: prologue || labels).

Needs a library built with -DGLASS_DENSE_TRACE (tools/build_trace.sh); run with GLASS_HIP_LIB pointing at it:
    GLASS_HIP_LIB=$PWD/tools/bin/libglass_trace.so [GLASS_EPOCH_PLAN=0] python tools/head_trace.py [workload]
The step is captured as bench.py captures it (TrainStep.begin_epoch, cycling batches) and replayed; the stamps (wall_clock64,
100 MHz: 10 ns steps) are those of ONE replay.
  sel 5, the label workgroup (waves 0-3 of its 16): 0 entry, 1 cursor record read, 2 behind the first barrier (old labels off,
  the thread's new entries arrived), 3 owners elected (atomicMin round drained; per-step path only), 6 list written (owner
  read-back + compaction; per-step path only), 4 last store issued.
  sel 6, the prologue workgroups: 0 entry, 4 exit."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glass_amd import _lib, losses, ops, synth  # noqa: E402
from glass_amd.arena import ParamArena  # noqa: E402
from glass_amd.factory import build_glass  # noqa: E402
from glass_amd.optim import FlatAdam  # noqa: E402
from glass_amd.step import TrainStep  # noqa: E402


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "ppi_bp"
    dev = torch.device("cuda:0")
    n_b = 16
    w, ei, ew, x, pos, y = synth.make_workload(name, seed=0, n_batches=n_b)
    ei, ew, x, pos, y = (torch.from_numpy(a).to(dev) for a in (ei, ew, x, pos, y))
    torch.manual_seed(0)
    ops.rng_seed(1234, dev)
    model = build_glass(w.hidden, w.layers, int(x.max()), w.n_class, w.aggr, w.pool, w.z_ratio, dropout=w.dropout).to(dev).train()
    arena = ParamArena(model)
    opt = FlatAdam(arena, lr=w.lr)
    loss_fn = losses.BCEWithLogits() if w.multilabel else losses.CrossEntropy()
    step = TrainStep(model, opt, loss_fn, x, ei, ew, arena, use_graph=True)
    idx = torch.arange(n_b * w.batch, device=dev).reshape(n_b, w.batch)
    assert step.begin_epoch(pos, y, idx, wrap=True), "the step did not take the head-label form"
    lib = _lib.load()
    lib.glass_dense_trace_set.restype = ctypes.c_int
    lib.glass_dense_trace_set.argtypes = [ctypes.c_void_p, ctypes.c_int]
    for _ in range(20):
        step.next_step()
    torch.cuda.synchronize()
    print(f"{name}: epoch plan {'on, %d bytes' % step._labels.plan_bytes if step._labels.plan_bytes else 'off'}")
    buf = torch.zeros((4096, 4, 8), dtype=torch.int64, device=dev)
    rows = []
    for rep in range(5):
        out = {}
        for sel in (5, 6):
            buf.zero_()
            torch.cuda.synchronize()
            assert lib.glass_dense_trace_set(buf.data_ptr(), sel) == 0
            step.next_step()
            torch.cuda.synchronize()
            lib.glass_dense_trace_set(None, 0)
            out[sel] = buf.cpu().numpy().astype(np.float64) * 10.0  # ns
        lab = out[5][0]                       # [wave][slot] of the label workgroup
        t0 = lab[:, 0].min()
        ph = {s: (lab[:, s].max() - t0) if (lab[:, s] > 0).all() else float("nan") for s in (1, 2, 3, 6, 4)}
        pk = out[6]
        live = pk[:, :, 0] > 0
        span = (pk[:, :, 4][live].max() - pk[:, :, 0][live].min()) if live.any() else float("nan")
        life = (pk[:, :, 4] - pk[:, :, 0])[live]
        rows.append((ph, span, float(np.median(life)) if live.any() else float("nan"), int(live.sum())))
    print("label workgroup, ns after its entry (slowest of waves 0-3) | prologue workgroups (their own replay)")
    print("  replay  cursor  barrier1  elected  listed    done | span first entry -> last exit, median wave life, waves")
    for k, (ph, span, life, n) in enumerate(rows):
        print(f"  {k:6d} {ph[1]:7.0f} {ph[2]:9.0f} {ph[3]:8.0f} {ph[6]:7.0f} {ph[4]:7.0f} | {span:7.0f} {life:7.0f} {n:5d}")


if __name__ == "__main__":
    main()
