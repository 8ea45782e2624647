"""Shared test helpers (fixture loading, parity metric)."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return np.load(os.path.join(GOLDEN, name), allow_pickle=False)


def sd_from(npz, prefix="sd/"):
    return {k[len(prefix):]: torch.from_numpy(npz[k].copy()) for k in npz.files if k.startswith(prefix)}


def grads_from(npz, prefix="grad/"):
    return {k[len(prefix):]: torch.from_numpy(npz[k].copy()) for k in npz.files if k.startswith(prefix)}


def rel_inf(a, b):
    """SURVEY.md §8d parity metric: ||a-b||_inf / ||b||_inf (never per-element relative error)."""
    a = torch.as_tensor(a, dtype=torch.float64).reshape(-1)
    b = torch.as_tensor(b, dtype=torch.float64).reshape(-1)
    denom = b.abs().max().item()
    return (a - b).abs().max().item() / (denom if denom > 0 else 1.0)


def flat_grads(named, keys):
    return torch.cat([named[k].reshape(-1).double() for k in keys])


def grad_table(mine, ref64, keys, ref32=None):
    """Per-parameter picture of a gradient comparison: rows (key, |g64|_inf / gmax, |mine - g64|_inf / gmax,
    |ref32 - g64|_inf / gmax) with gmax = ||all fp64 gradients||_inf — i.e. each parameter's share of the FLAT rel-inf metric
     — worst first."""
    gmax = max(float(ref64[k].abs().max()) for k in keys) or 1.0
    rows = []
    for k in keys:
        g = ref64[k].double()
        rows.append((k, float(g.abs().max()) / gmax, float((mine[k].double() - g).abs().max()) / gmax,
                     float((ref32[k].double() - g).abs().max()) / gmax if ref32 is not None else float("nan")))
    return sorted(rows, key=lambda r: -r[2])


def assert_grad_parity(mine, ref64, keys, tol, exact_zero=(), ref32=None, label=""):
    """The gradient gate of the parity contract: rel-inf on the FLAT vector < tol — plain
    tol, no noise multiple — over every parameter except those named in `exact_zero`: parameters whose gradient is ZERO IN
    EXACT ARITHMETIC (a bias added right in front of a GraphNorm whose mean_scale is 1: the norm subtracts the column mean,
    so d loss / d bias = sum of a mean-free column).  What ANY fp32 evaluation returns for such a parameter is its own
    rounding noise (N terms of size |g| cancelling), so it carries no parity information beyond "as small as the
    reference's own noise": the claim is first PROVEN (the fp64 gradient there is < 1e-9 of the largest gradient), then the
    parameter is graded against the fp32 oracle's error on the same parameter, |err| <= 2 * that (or tol, if larger).
    Returns (flat rel-inf without the exact-zero parameters, {key: (err, oracle32 err)} for the exact-zero ones)."""
    table = grad_table(mine, ref64, keys, ref32)
    rows = {r[0]: r for r in table}
    for k in exact_zero:
        assert k in rows, f"{label}: exact-zero parameter {k} not in the model"
        assert rows[k][1] < 1e-9, f"{label}: {k} is claimed cancellation-defined but |g64| = {rows[k][1]:.2e} of the largest gradient"
    graded = [k for k in keys if k not in set(exact_zero)]
    err = max(rows[k][2] for k in graded)
    worst = table[0]
    print(f"{label}: flat gradient rel-inf {err:.2e} over {len(graded)} parameters (worst overall: {worst[0]} {worst[2]:.2e}, "
          f"fp32 oracle there {worst[3]:.2e})")
    assert err < tol, f"{label}: gradient rel-inf {err:.3e} >= {tol:g}; worst rows {table[:3]}"
    zeros = {}
    for k in exact_zero:
        mine_e, o_e = rows[k][2], rows[k][3]
        zeros[k] = (mine_e, o_e)
        print(f"{label}: exact-zero gradient {k}: |err| {mine_e:.2e} of gmax (fp32 oracle: {o_e:.2e})")
        assert mine_e < max(tol, 2 * o_e), f"{label}: {k}: {mine_e:.3e} vs oracle noise {o_e:.3e}"
    return err, zeros


def density_inputs(npz):
    """Rebuild the symmetrised, (row,col)-sorted density graph from the stored u<v pairs."""
    und = npz["und_pairs"].astype(np.int64)
    n = int(npz["n_node"])
    ei = np.concatenate([und, und[::-1]], axis=1)
    order = np.argsort(ei[0] * n + ei[1], kind="stable")
    ei = torch.from_numpy(ei[:, order].copy())
    ew = torch.ones(ei.shape[1])
    x = torch.from_numpy(npz["x"].astype(np.int64)).reshape(n, 1, 1)
    pos = torch.from_numpy(npz["pos"].astype(np.int64))
    y = torch.from_numpy(npz["y"].astype(np.int64))
    z = torch.from_numpy(npz["z"].astype(np.int64))
    return n, ei, ew, x, pos, y, z


def build_glass(*args, **kwargs):
    """The product model, constructed exactly as GLASSTest.py:129-175 (buildModel) constructs the reference one."""
    from glass_amd.factory import build_glass as _build
    return _build(*args, **kwargs)


def record_parity(config, **metrics):
    """Append one parity record (achieved rel-inf numbers, not just pass/fail) to gpurun_out/parity_r06.json under the
    repo root — gpurun merges that directory back, and the file is then committed as profiles/parity_r06.json."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.join(root, "gpurun_out")
    try:
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, "parity_r06.json")
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[config] = {k: (v if isinstance(v, (bool, str)) else float(v)) for k, v in metrics.items()}
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    except OSError:
        pass  # a read-only checkout must not fail a parity test


# The Python A/B switches (module, attribute, non-default value); each environment variable named in the g8 switch test sets one.
PYTHON_SWITCHES = [
    ("glass_amd.train", "USE_STEP", False), ("glass_amd.train", "USE_GRAPH", False), ("glass_amd.train", "USE_HEAD_LABELS", False),
    ("glass_amd.train", "USE_EVAL_GRAPH", False), ("glass_amd.models", "USE_STACK", False), ("glass_amd.ops", "USE_FUSED_DENSE", False),
    ("glass_amd.stack", "USE_COMB_EFF", False), ("glass_amd.stack", "USE_GN_EXACT", False), ("glass_amd.stack", "USE_READOUT", False),
    ("glass_amd.stack", "USE_READOUT_TWO", False), ("glass_amd.stack", "USE_GN_BWD_IN_COMB", False),
    ("glass_amd.stack", "USE_GATHER_IN_TRANS", False), ("glass_amd.stack", "USE_EMBED_TABLE", False),
    ("glass_amd.stack", "USE_FUSED_TAIL", False), ("glass_amd.stack", "USE_FUSED_BWD", False), ("glass_amd.ops", "DENSE_F32_PRODUCTS", True)]

# ... those that act inside one training pass (stack.loss_and_grads or the per-op forward / backward it falls back to): every
# switch of PYTHON_SWITCHES outside glass_amd.train, GLASS_GN_EXACT_FWD, and GLASS_DENSE_H128 / GLASS_DENSE_H256 (ops._DENSE_OFF)
STEP_SWITCHES = [s for s in PYTHON_SWITCHES if s[0] != "glass_amd.train"] + [
    ("glass_amd.stack", "USE_GN_EXACT_FWD", False), ("glass_amd.ops", "_DENSE_OFF", {128}), ("glass_amd.ops", "_DENSE_OFF", {256})]


class Buf:
    """a [rows, cols] fp32 / fp64 view with leading dimension ld = cols + 4, two guard rows in front and behind, in a NaN-filled flat
    buffer; 16-byte aligned.  tail: what the two guard rows behind hold (inputs: Inf, NaN)."""
    def __init__(self, rows, cols, src=None, dtype=torch.float32, tail=None, pad=4):
        ld = cols + pad   # (pad = 0: the contiguous [tile][2][H] partials, guarded by the rows in front and behind)
        self.ld, self.rows, self.cols = ld, rows, cols
        self.flat = torch.full(((rows + 4) * ld + 8, ), float("nan"), dtype=dtype, device="cuda:0")
        off = 2 * ld + 4
        self.v = torch.as_strided(self.flat, (rows, cols), (ld, 1), off)
        assert self.v.data_ptr() % 16 == 0
        if src is not None:
            self.v.copy_(torch.as_tensor(src))
        if tail is not None:
            torch.as_strided(self.flat, (1, cols), (ld, 1), off + rows * ld).fill_(tail)
        self.inside = torch.zeros(self.flat.numel(), dtype=torch.bool, device="cuda:0")
        torch.as_strided(self.inside, (rows, cols), (ld, 1), off).fill_(True)

    @property
    def ptr(self):
        return self.v.data_ptr()

    def check(self, tag, allow_nan=False):
        assert bool(torch.isnan(self.flat[~self.inside]).all()), f"{tag}: written outside its view (guard rows / columns)"
        if not allow_nan:
            assert not bool(torch.isnan(self.flat[self.inside]).any()), f"{tag}: NaN or unwritten element inside its view"
        return self

    def cpu(self):
        return self.v.detach().cpu()
