"""Device-resident CSR form of the normalised adjacency and the K1 launch plans.

Replaces the reference's cached uncoalesced COO (`buildAdj`, /root/reference/impl/models.py:83-111,
cached at 154-156).  Built once per (graph, aggr) — index plumbing (sort, bincount) uses torch ops
on the device; the values come from the HIP kernel `glass_adj_values_f32`; the launch plans are
built by the library's host function `glass_spmm_plan_build` from the row pointer.

HBM layout (all on the device the graph lives on):
  rowptr int32[N+1], col int32[nnz], val fp32[nnz]            CSR of A   (row = destination)
  rowptr_t, col_t, val_t                                      CSR of A^T (for the backward)
  plan / plan_t int32[...]                                    opaque K1 schedules
  eid_t int32[nnz]                                            aggr "max", "gat", "gatv2" and "pna": forward index of each entry of A^T
  perm int64[nnz]                                             the build permutation: entry e is the caller's edge perm[e]
aggr "sum", "mean" and "gcn" can also be evaluated at OTHER edge weights on the same structure, with the gradient with respect
to them (values_of / dval / colsum / values_bwd: K1w, ops.spmm_w); what that needs beyond perm is built on first use.
aggr "max", "softmax", "gat", "gatv2", "std", "var" and "pna" keep the raw edge weights in val (the values of "sum"); all but
"max" require them > 0.
Duplicate (row,col) entries are kept as separate entries: they add up in the product exactly as in
the reference's uncoalesced COO matmul.

Every entry that walks a CSR takes `rowptr, col, val[, eid_t]`, its own operands, then `n_rows[, H[, K]]`, trailing scalars,
and `header, plan, ws, stream`: `_launch` is the one place that puts that list together, sizes and fetches the workspace, and
checks the return code.  `_call` (under it, and under the entries without a CSR) refuses a call whose argument count is not
the entry's — ctypes itself lets extra arguments through.  Workspaces come from one grow-or-retire cache (`_Workspaces`):
every matrix has one for its product, the adjacencies of the extensions one for their kernels, and the edge-weight path one
made with the rest of its state on first use.
"""
import ctypes

import numpy as np
import torch

from . import _lib

_ws_branch = 0


def set_workspace_branch(b):
    """Which workspace set CSROperand.workspace hands out from now on (0: the default one)."""
    global _ws_branch
    _ws_branch = int(b)


class _Workspaces(dict):
    """The kernels' scratch (partial rows, pairs and triples of rows cut into several chunks; fp64 partials): the live buffers,
    one 8-byte aligned buffer of at least 16 bytes per (entry, width, BRANCH) — entry the launch method's name, width (H, ) or
    (H, K); set_workspace_branch: concurrent launches on the same matrix, the parallel evaluation branches of
    evalstep.EvalGraph, must not share one.  A request that fits gets the SAME tensor again; a larger one gets a new tensor and
    the old one goes to `retired`, never freed or handed out again: a captured graph may still launch with its pointer."""
    def __init__(self, device):
        super().__init__()
        self.device, self.retired = device, []

    def fetch(self, entry, width, nbytes):
        """nbytes: the answer of the entry's *_ws_bytes query (negative: it refused the plan header)"""
        if nbytes < 0:
            raise _lib.GlassHipError("bad plan header")
        key = (entry, width, _ws_branch)
        ws = self.get(key)
        if ws is None or ws.numel() * 8 < nbytes:
            if ws is not None:
                self.retired.append(ws)
            ws = self[key] = torch.empty(max((nbytes + 7) // 8, 2), dtype=torch.float64, device=self.device)
        return ws


def _call(fn, entry, args):
    """The return code of the library's `entry` (fn) on `args` and the current stream (looked up now: a launch goes where the
    caller is working).  The count is held to the entry's row of _lib.SIGNATURES — what load() gave fn as argtypes; fn itself
    may be a plain wrapper without them (bench.py's instrumented pass brackets every entry in one)."""
    want = len(_lib.SIGNATURES[entry][1])
    if len(args) + 1 != want:
        raise _lib.GlassHipError(f"{entry}: called with {len(args) + 1} arguments, the entry takes {want}")
    return fn(*args, torch.cuda.current_stream().cuda_stream)


def _run(entry, args):
    _lib.check(_call(getattr(_lib.load(), entry), entry, args), entry)


def _launch(op, cache, key, entry, query, mid, H=None, K=None, eid_t=None, tail=(), val=None, header=None):
    """One CSR entry on the matrix `op` (a CSROperand): entry(rowptr, col, val[, eid_t], *mid, n_rows[, H[, K]], *tail, header,
    plan, ws, stream) with ws from `cache` under `key` (the launch method's name) at the size `query`(header[, H[, K]]) names.
    val / header: others than op's own (same entries, same plan).  Returns the workspace."""
    lib = _lib.load()
    hdr = (op.header if header is None else header).ctypes.data
    width = () if H is None else (H, ) if K is None else (H, K)
    ws = cache.get((key, width, _ws_branch))
    if ws is None:  # (these sizes are functions of the plan and the width alone: asked once per key)
        ws = cache.fetch(key, width, getattr(lib, query)(hdr, *width))
    args = [op.rowptr.data_ptr(), op.col.data_ptr(), (op.val if val is None else val).data_ptr()]
    if eid_t is not None:
        args.append(eid_t.data_ptr())
    args += mid
    args += (op.n_rows, *width, *tail, hdr, op.plan.data_ptr(), ws.data_ptr())
    _lib.check(_call(getattr(lib, entry), entry, args), entry)
    return ws


def _operand(a, n, name, dtype=torch.float32):
    """The leading dimension of a row-major [n, H] operand on the device: its row stride, and for a single row at least H."""
    assert a.dim() == 2 and a.stride(1) == 1 and a.dtype == dtype and a.is_cuda, name
    assert a.shape[0] == n, f"{name} has {a.shape[0]} rows, the adjacency has {n} nodes"
    return a.stride(0) if a.shape[0] > 1 else max(a.shape[1], a.stride(0))


def _empty(like, *shape, dtype=torch.float32):
    return torch.empty(shape, dtype=dtype, device=like.device)


class CSROperand:
    """One CSR matrix + its K1 plan; `spmm` enqueues Y = M @ X on the current stream."""
    def __init__(self, rowptr, col, val, n_rows, n_cols, rowptr_host=None):
        """rowptr_host: the same row pointer already in host memory (int32 numpy) — no device->host sync then, and the plan
        goes up through pinned memory without waiting for the stream."""
        self.rowptr, self.col, self.val = rowptr, col, val
        self.n_rows, self.n_cols = int(n_rows), int(n_cols)
        lib = _lib.load()
        if rowptr_host is None:
            rp_host = rowptr.cpu().numpy()  # one-time sync: the plan is host arithmetic on the row pointer
        else:
            rp_host = np.ascontiguousarray(rowptr_host, dtype=np.int32)
        words = ctypes.c_int64(0)
        _lib.check(lib.glass_spmm_plan_build(rp_host.ctypes.data, self.n_rows, None, ctypes.byref(words)), "plan size")
        plan = np.zeros(words.value, dtype=np.int32)
        _lib.check(lib.glass_spmm_plan_build(rp_host.ctypes.data, self.n_rows, plan.ctypes.data, ctypes.byref(words)),
                   "plan build")
        self.header = plan[:_lib.PLAN_HEADER_WORDS].copy()  # read on the host by every launch
        if rowptr_host is None:
            self.plan = torch.from_numpy(plan).to(rowptr.device)
        else:
            self.plan = torch.from_numpy(plan).pin_memory().to(rowptr.device, non_blocking=True)
        self._ws = _Workspaces(rowptr.device)

    @property
    def nnz(self):
        return int(self.header[3])

    def workspace(self, H):
        """Partial-row scratch of products with rows cut into several chunks (the buffer `spmm` launches with): one per feature
        width and per branch."""
        ws = self._ws.get(("spmm", (H, ), _ws_branch))
        if ws is None:
            ws = self._ws.fetch("spmm", (H, ), _lib.load().glass_spmm_ws_bytes(self.header.ctypes.data, H))
        return ws

    def spmm(self, x, out=None, val=None):
        """val: other values for the same entries (fp32 [nnz] on the device: CSRAdj.values_of) instead of the stored ones."""
        assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32 and x.is_cuda
        assert x.shape[0] == self.n_cols, f"X has {x.shape[0]} rows, matrix has {self.n_cols} columns"
        H = x.shape[1]
        if out is None:
            out = torch.empty((self.n_rows, H), dtype=torch.float32, device=x.device)
        assert out.stride(1) == 1 and out.shape == (self.n_rows, H)
        if val is None:
            val = self.val
        assert val.dtype == torch.float32 and val.shape == self.val.shape and val.is_contiguous() and val.device == self.val.device
        # (the row strides as they are: no single-row rule here)
        _launch(self, self._ws, "spmm", "glass_spmm_csr_f32", "glass_spmm_ws_bytes",
                (x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0)), H, val=val)
        return out

    def spmm_rep(self, x, R, x_rep_stride=None, out=None, y_rep_stride=None):
        """Y[r] = M @ X[r] for R replicas in one launch (glass_spmm_csr_rep_f32): x holds replica r's rows from row
        r * x_rep_stride (default n_cols: replica-major [R * n_cols, H]), out likewise from r * y_rep_stride (default
        n_rows).  Same plan and indices as `spmm`; replica r has the bits `spmm` gives on its slice."""
        assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32 and x.is_cuda
        R = int(R)
        xs = self.n_cols if x_rep_stride is None else int(x_rep_stride)
        ys = self.n_rows if y_rep_stride is None else int(y_rep_stride)
        assert R == 0 or x.shape[0] >= (R - 1) * xs + self.n_cols, f"X has {x.shape[0]} rows for {R} replicas of {self.n_cols}"
        H = x.shape[1]
        if out is None:
            out = torch.empty((R * ys, H), dtype=torch.float32, device=x.device)
        assert out.stride(1) == 1 and out.shape[1] == H and (R == 0 or out.shape[0] >= (R - 1) * ys + self.n_rows)
        lib = _lib.load()
        hdr = self.header.ctypes.data
        # not through _launch: one buffer per width (not per R), grown when a call needs more replicas' partial rows, and a
        # return code with an answer of its own
        ws = self._ws.fetch("rep", (H, ), lib.glass_spmm_rep_ws_bytes(hdr, H, R))
        ldx = x.stride(0) if x.shape[0] > 1 else max(H, x.stride(0))
        ldy = out.stride(0) if out.shape[0] > 1 else max(H, out.stride(0))
        rc = _call(lib.glass_spmm_csr_rep_f32, "glass_spmm_csr_rep_f32",
                   (self.rowptr.data_ptr(), self.col.data_ptr(), self.val.data_ptr(), x.data_ptr(), ldx, xs, out.data_ptr(), ldy, ys,
                    self.n_rows, H, R, hdr, self.plan.data_ptr(), ws.data_ptr()))
        if rc == -3:  # GLASS_E_UNSUPPORTED: too many replicas, or too much memory, for one launch
            msg = lib.glass_last_error_string().decode(errors="replace")
            raise _lib.GlassHipError(f"glass_spmm_csr_rep_f32: {msg}; run the replicas in smaller groups (EmbZGConv.replica_chunk)")
        _lib.check(rc, "glass_spmm_csr_rep_f32")
        return out


def _csr_from_sorted(row, n_rows):
    counts = torch.bincount(row, minlength=n_rows)
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=row.device)
    rowptr[1:] = torch.cumsum(counts, 0)
    return rowptr.to(torch.int32)


def _pna_degrees(rowptr, w):
    """(delta, wsum) of PNA's degree scalers, in fp64 on the host (once, at build): W_i the weight sum of row i (the weights
    are positive, so a row with entries has W > 0); delta the mean over the rows with entries of log(W_i + 1), 1.0 when no
    row has entries; wsum the W_i rounded to fp32, on the graph's device."""
    rp = rowptr.cpu().numpy().astype(np.int64)
    live = rp[1:] > rp[:-1]
    W = np.zeros(rp.shape[0] - 1, dtype=np.float64)
    if live.any():
        W[live] = np.add.reduceat(w.double().cpu().numpy(), rp[:-1][live])
    delta = float(np.log1p(W[live]).mean()) if live.any() else 1.0
    return delta, torch.from_numpy(W.astype(np.float32)).to(rowptr.device)


_RAW_AGGR = ("max", "softmax", "gat", "gatv2", "std", "var", "pna")  # the extensions: raw edge weights in val, kernels of their own
MOMENT_KINDS = {"std": 0, "var": 1}


class CSRAdj:
    """Normalised adjacency A (forward) and A^T (backward) for one aggregation scheme.  Every launch method below is a guard
    on the aggr the adjacency was built for (`_need`), the operands' leading dimensions (`_operand`), the results, and one
    `_launch` on `fwd` or `bwd` with a workspace from `_aggr_ws`.  aggr "max" (an extension): the raw
    edge weights (the values of "sum"), aggregated by K1m (max_fwd / max_bwd) instead of K1's product.  aggr "softmax" (an
    extension): the raw weights too, strictly positive (checked here, once), aggregated by K1s (softmax_fwd / softmax_bwd /
    softmax_dt) with a temperature the caller owns.  aggr "gat" (an extension): built like "softmax", aggregated by K1a
    (gat_scores / gat_fwd / gat_edge / gat_bwd / gat_datt, each with heads=K for multi-head attention) with two attention
    vectors the caller owns.  aggr "gatv2" (an extension): built like "gat", aggregated by K1a2 (gatv2_score / gatv2_fwd /
    gatv2_edge / gatv2_bwd / gatv2_datt) with one attention vector the caller owns.  aggr "std" / "var" (extensions): built like "softmax", aggregated by K1v (moment_fwd /
    moment_bwd: the weighted standard deviation or variance of the neighbour messages, with their weighted mean).  aggr "pna"
    (an extension): built like "softmax", aggregated by K1p (pna_fwd / pna_bwd: mean, standard deviation, max and min of the
    neighbour messages from one gather); `pna_delta` is the mean of log(W_i + 1) over the rows with entries (PNA's degree
    normaliser, a Python float from fp64 arithmetic at build; 1.0 for a graph without entries) and `pna_wsum` [N] the W_i
    it was formed from, rounded to fp32 (what ops.pna_mix scales with)."""
    def __init__(self, edge_index, edge_weight, n_node, aggr):
        if aggr not in _lib.AGGR_MODES and aggr not in _RAW_AGGR:
            raise NotImplementedError  # same error type as the reference (models.py:110-111)
        if (aggr in MOMENT_KINDS or aggr == "pna") and not bool((edge_weight > 0).all()):  # one read; the kernels do not test it
            raise ValueError(f"aggr {aggr!r}: edge weights are multiplicities and must be strictly positive")
        if not edge_index.is_cuda:
            raise _lib.GlassHipError("glass_amd runs on the GPU only (edge_index is on %s); the CPU path lives in "
                                     "oracle/ as a checker, not as a fallback" % edge_index.device)
        n = int(n_node)
        nnz = edge_index.shape[1]
        if n >= 2**31 - 1 or nnz >= 2**31 - 1:
            raise _lib.GlassHipError("int32 CSR: need n_node, nnz < 2^31")
        dev = edge_index.device
        row, col = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
        perm = torch.argsort(row * n + col, stable=True)
        row, col = row[perm], col[perm]
        w = edge_weight.to(torch.float32)[perm].contiguous()
        if aggr in ("softmax", "gat", "gatv2") and not bool((w > 0).all()):  # one device read; the kernels do not test it
            raise ValueError(f"aggr {aggr!r}: edge weights are multiplicities and must be strictly positive")
        rowptr = _csr_from_sorted(row, n)
        col32 = col.to(torch.int32).contiguous()
        self.deg = torch.empty(n, dtype=torch.float32, device=dev)
        val = torch.empty(nnz, dtype=torch.float32, device=dev)
        _run("glass_adj_values_f32", (rowptr.data_ptr(), col32.data_ptr(), w.data_ptr(), n,
                                      _lib.AGGR_MODES["sum" if aggr in _RAW_AGGR else aggr], self.deg.data_ptr(), val.data_ptr()))
        # transpose: same entries keyed by (col,row); values are permuted, never recomputed
        perm_t = torch.argsort(col * n + row, stable=True)
        rowptr_t = _csr_from_sorted(col[perm_t], n)
        col_t = row[perm_t].to(torch.int32).contiguous()
        val_t = val[perm_t].contiguous()
        self.n_node, self.aggr = n, aggr
        self.perm = perm  # entry e of the forward CSR is edge perm[e] of the caller's edge_index (int64, as argsort left it)
        self.fwd = CSROperand(rowptr, col32, val, n, n)
        self.bwd = CSROperand(rowptr_t, col_t, val_t, n, n)
        if aggr in _lib.AGGR_MODES:
            self._raw_w = val if aggr == "sum" else w  # the raw weights, forward entry order (edge dropout redraws from them)
        if aggr in ("max", "gat", "gatv2", "pna"):
            self.eid_t = perm_t.to(torch.int32).contiguous()  # transposed entry t is forward entry eid_t[t]
        if aggr in _RAW_AGGR:
            self._aggr_ws = _Workspaces(dev)
        if aggr == "pna":
            self.pna_delta, self.pna_wsum = _pna_degrees(rowptr, w)

    @property
    def nnz(self):
        return self.fwd.nnz

    def _need(self, what, *aggrs):
        if self.aggr not in aggrs:
            raise _lib.GlassHipError(f"CSRAdj.{what}: this adjacency was built for aggr {self.aggr!r}, not "
                                     + " or ".join(repr(a) for a in aggrs))

    # ---- K1w: the gradient with respect to the edge weights (aggr "sum", "mean", "gcn"; csrc/spmm_edge.hip) -----------------
    def _edge_grad_state(self, what):
        """(eid_t, perm32, workspaces), built the first time the edge-weight path asks: eid_t is the stable sort that built the
        transpose, made again from the stored CSR (the same permutation), perm32 the build permutation as the kernel reads it."""
        if self.aggr not in _lib.AGGR_MODES:
            raise _lib.GlassHipError(f"CSRAdj.{what}: no edge-weight gradient for aggr {self.aggr!r} (only 'sum', 'mean', 'gcn')")
        st = self.__dict__.get("_edge_grad")
        if st is None:
            rp = self.fwd.rowptr.to(torch.int64)
            row = torch.repeat_interleave(torch.arange(self.n_node, device=rp.device), rp[1:] - rp[:-1])
            eid_t = torch.argsort(self.fwd.col.to(torch.int64) * self.n_node + row, stable=True).to(torch.int32).contiguous()
            st = self._edge_grad = (eid_t, self.perm.to(torch.int32).contiguous(), _Workspaces(rp.device))
        return st

    def values_of(self, w):
        """(val, val_t, deg) for the caller-order weight vector w (fp32 [E] on the device, the order of the edge_index this
        adjacency was built from): what the constructor would store for it — K2 on the permuted weights, the transpose a permute
        of the result.  The stored values are not touched."""
        op = self.fwd
        if self.aggr in _lib.AGGR_MODES and (w.dim() != 1 or w.shape[0] != op.nnz or w.dtype != torch.float32 or
                                             w.device != op.rowptr.device):  # (before any launch)
            raise ValueError(f"edge weights: expected {op.nnz} fp32 on {op.rowptr.device}, got {tuple(w.shape)} {w.dtype} on {w.device}")
        eid_t, _p, _ws = self._edge_grad_state("values_of")
        ws = w.detach()[self.perm].contiguous()
        deg = _empty(w, self.n_node)
        val = _empty(w, op.nnz)
        _run("glass_adj_values_f32", (op.rowptr.data_ptr(), op.col.data_ptr(), ws.data_ptr(), self.n_node,
                                      _lib.AGGR_MODES[self.aggr], deg.data_ptr(), val.data_ptr()))
        return val, val[eid_t.to(torch.int64)].contiguous(), deg

    def dval(self, dy, x, val):
        """(dval, R) = the sampled dense-dense product over the forward CSR: dval [nnz] the dot of dy[destination] and
        x[source] of every entry, in forward entry order; R [N] the row sums of dval * val."""
        _e, _p, cache = self._edge_grad_state("dval")
        op = self.fwd
        ldx = _operand(x, op.n_cols, "X")
        lddy = _operand(dy, op.n_rows, "dY")
        assert dy.shape == x.shape
        assert val.dtype == torch.float32 and val.shape == (op.nnz, ) and val.is_contiguous() and val.is_cuda
        H = x.shape[1]
        dv = _empty(x, max(op.nnz, 1))[:op.nnz]
        R = _empty(x, op.n_rows)
        _launch(op, cache, "dval", "glass_spmm_dval_f32", "glass_spmm_dval_ws_bytes",
                (x.data_ptr(), ldx, dy.data_ptr(), lddy, dv.data_ptr(), R.data_ptr()), H, val=val)
        return dv, R

    def colsum(self, dval, val_t):
        """C [N] = the column sums of dval * val, over the transposed CSR (aggr "gcn" needs them)."""
        eid_t, _p, cache = self._edge_grad_state("colsum")
        op = self.bwd
        for a in (dval, val_t):
            assert a.dtype == torch.float32 and a.shape == (op.nnz, ) and a.is_contiguous() and a.is_cuda
        C = _empty(dval, op.n_rows)
        _launch(op, cache, "colsum", "glass_adj_colsum_f32", "glass_adj_colsum_ws_bytes", (dval.data_ptr(), C.data_ptr()),
                eid_t=eid_t, val=val_t)
        return C

    def values_bwd(self, dval, R, C, w, deg=None):
        """dw [E], in the caller's edge order: the backward of values_of at w for the entry gradients dval (with their row sums R
        and, for "gcn", column sums C; None where the aggregation does not read them).  deg: values_of(w)'s third result when
        the caller kept it; made again from w otherwise."""
        _e, perm32, _ws = self._edge_grad_state("values_bwd")
        op = self.fwd
        if deg is None and self.aggr != "sum":
            deg = self.values_of(w)[2]
        assert dval.dtype == torch.float32 and dval.shape == (op.nnz, ) and dval.is_contiguous() and dval.is_cuda
        for a in (R, C, deg):
            assert a is None or (a.dtype == torch.float32 and a.shape == (self.n_node, ) and a.is_contiguous() and a.is_cuda)
        dw = _empty(dval, op.nnz)
        ptr = lambda a: None if a is None else a.data_ptr()
        _run("glass_adj_values_bwd_f32", (op.rowptr.data_ptr(), op.col.data_ptr(), perm32.data_ptr(), ptr(deg), dval.data_ptr(),
                                          ptr(R), ptr(C), self.n_node, op.nnz, _lib.AGGR_MODES[self.aggr], dw.data_ptr()))
        return dw

    # ---- K2d: edge dropout (aggr "sum", "mean", "gcn"; csrc/spmm_dropedge.hip) -------------------------------------------------
    def _dropedge_state(self, what):
        """(raw weights in forward order, raw weights in transposed order, buffers), built the first time edge dropout asks.  The
        transposed-order weights of "sum" are the stored backward values; "mean" and "gcn" permute the raw forward weights once
        with the transpose's stable sort (the same permutation the constructor used)."""
        if self.aggr not in _lib.AGGR_MODES:
            raise _lib.GlassHipError(f"CSRAdj.{what}: no edge dropout for aggr {self.aggr!r} (only 'sum', 'mean', 'gcn': the others "
                                     "need the entry excluded, not weighted zero)")
        st = self.__dict__.get("_dropedge")
        if st is None:
            if self.aggr == "sum":
                w_t = self.bwd.val
            else:
                eid_t = self._edge_grad_state(what)[0]
                w_t = self._raw_w[eid_t.to(torch.int64)].contiguous()
            st = self._dropedge = (self._raw_w, w_t, {})
        return st

    def dropedge_values(self, p, call_id, symmetric=True, want_keep=False, rng=None):
        """(val, val_t, deg[, keep]) under edge dropout at rate p: one keep bit per entry drawn by K2d from (seed, step, call_id,
        destination, source, N) — `rng` the int64[2] (seed, step) words on the device, default ops.rng_tensor — the dropped
        entries' weights set to +0.0, and K2's values for those weights on the unchanged structure: the bits of
        values_of(w * keep).  keep: uint8 [nnz] in FORWARD ENTRY order (entry e is the caller's edge perm[e]).
        The results live in one set of buffers per (call_id, workspace branch), overwritten by the next call with that key: a
        captured graph keeps launching on them (their sizes never change, so none is ever replaced or handed back).
        `dropedge_record(call_id)["gen"]` counts the draws into the current key's buffers."""
        w, w_t, bufs = self._dropedge_state("dropedge_values")
        p = float(p)
        if not (0.0 <= p < 1.0):
            raise ValueError(f"edge dropout rate must lie in [0, 1), got {p!r}")
        op, dev = self.fwd, self.fwd.rowptr.device
        key = (int(call_id), _ws_branch)
        b = bufs.get(key)
        if b is None:
            e = max(op.nnz, 1)
            b = bufs[key] = {"val": torch.empty(e, dtype=torch.float32, device=dev)[:op.nnz],
                             "val_t": torch.empty(e, dtype=torch.float32, device=dev)[:op.nnz],
                             "deg": torch.empty(self.n_node, dtype=torch.float32, device=dev), "keep": None, "gen": 0}
        if want_keep and b["keep"] is None:
            b["keep"] = torch.empty(max(op.nnz, 1), dtype=torch.uint8, device=dev)[:op.nnz]
        b["gen"] += 1
        if op.nnz == 0:
            b["deg"].fill_(1.0)  # K2's rule on an empty row
        else:
            if rng is None:
                from . import ops
                rng = ops.rng_tensor(dev)
            assert rng.dtype == torch.int64 and rng.numel() == 2 and rng.device == dev
            _run("glass_adj_dropedge_f32", (op.rowptr.data_ptr(), op.col.data_ptr(), w.data_ptr(), self.bwd.rowptr.data_ptr(),
                                            self.bwd.col.data_ptr(), w_t.data_ptr(), self.n_node, _lib.AGGR_MODES[self.aggr], p,
                                            1 if symmetric else 0, rng.data_ptr(), int(call_id), b["deg"].data_ptr(),
                                            b["val"].data_ptr(), b["val_t"].data_ptr(),
                                            b["keep"].data_ptr() if want_keep else None))
        out = (b["val"], b["val_t"], b["deg"])
        return out + (b["keep"], ) if want_keep else out

    def dropedge_record(self, call_id):
        """The record of the buffers of (call_id, current workspace branch), after a draw into them: its "gen" counts the draws
        so far — a holder of the tensors knows from it whether they still hold ITS draw."""
        return self._dropedge_state("dropedge_record")[2][(int(call_id), _ws_branch)]

    # ---- K1m: aggr "max" (csrc/spmm_max.hip) -------------------------------------------------------------------------------
    def max_fwd(self, x):
        """(y, arg) = K1m forward: y[i, c] = max over the entries e of row i of val[e] * x[col[e], c], arg the winning e
        (int32; -1 and y = 0 for a row without entries)."""
        self._need("max_fwd", "max")
        op = self.fwd
        ldx = _operand(x, op.n_cols, "X")
        H = x.shape[1]
        y = _empty(x, op.n_rows, H)
        arg = _empty(x, op.n_rows, H, dtype=torch.int32)
        _launch(op, self._aggr_ws, "max_fwd", "glass_spmm_max_csr_f32", "glass_spmm_max_ws_bytes",
                (x.data_ptr(), ldx, y.data_ptr(), H, arg.data_ptr(), H), H)
        return y, arg

    def max_bwd(self, dy, arg):
        """dx of K1m: every dy[i, c] goes, times its entry's weight, to the source of the entry arg[i, c] names."""
        self._need("max_bwd", "max")
        op = self.bwd
        ldy = _operand(dy, op.n_cols, "dY")
        lda = _operand(arg, op.n_cols, "arg", torch.int32)
        assert arg.shape == dy.shape
        H = dy.shape[1]
        dx = _empty(dy, op.n_rows, H)
        _launch(op, self._aggr_ws, "max_bwd", "glass_spmm_max_bwd_f32", "glass_spmm_max_bwd_ws_bytes",
                (dy.data_ptr(), ldy, arg.data_ptr(), lda, dx.data_ptr(), H), H, eid_t=self.eid_t)
        return dx

    # ---- K1s: aggr "softmax" (csrc/spmm_softmax.hip) -------------------------------------------------------------------------
    @staticmethod
    def _softmax_t(t, like):
        assert t.numel() == 1 and t.dtype == torch.float32 and t.device == like.device, "t: one fp32 on the operand's device"
        return t.data_ptr()  # read by the kernels when they run: a captured launch follows the parameter

    def softmax_fwd(self, x, t):
        """(y, lse) = K1s forward: per destination and channel the softmax-weighted mean of the neighbour messages at temperature
        t (one fp32 on the device), lse = max + log of the weighted sum of exponentials, kept for the backward."""
        self._need("softmax_fwd", "softmax")
        op = self.fwd
        ldx = _operand(x, op.n_cols, "X")
        H = x.shape[1]
        y = _empty(x, op.n_rows, H)
        lse = _empty(x, op.n_rows, H)
        _launch(op, self._aggr_ws, "softmax_fwd", "glass_spmm_softmax_csr_f32", "glass_spmm_softmax_ws_bytes",
                (x.data_ptr(), ldx, self._softmax_t(t, x), y.data_ptr(), H, lse.data_ptr(), H), H)
        return y, lse

    def softmax_bwd(self, dy, x, y, lse, t):
        """dx of K1s, from the forward's operand x and its results (y, lse)."""
        self._need("softmax_bwd", "softmax")
        op = self.bwd
        ldx = _operand(x, op.n_rows, "X")
        lddy, ldy, ldl = (_operand(a, op.n_cols, n) for a, n in ((dy, "dY"), (y, "Y"), (lse, "L")))
        assert dy.shape == x.shape == y.shape == lse.shape
        H = x.shape[1]
        dx = _empty(x, op.n_rows, H)
        _launch(op, self._aggr_ws, "softmax_bwd", "glass_spmm_softmax_bwd_f32", "glass_spmm_softmax_bwd_ws_bytes",
                (x.data_ptr(), ldx, self._softmax_t(t, x), dy.data_ptr(), lddy, y.data_ptr(), ldy, lse.data_ptr(), ldl,
                 dx.data_ptr(), H), H)
        return dx

    def softmax_dt(self, dy, x, y, lse, t):
        """The temperature's gradient (shape [1]): a further pass over the forward CSR, run only when t is trained."""
        self._need("softmax_dt", "softmax")
        op = self.fwd
        ldx = _operand(x, op.n_cols, "X")
        lddy, ldy, ldl = (_operand(a, op.n_rows, n) for a, n in ((dy, "dY"), (y, "Y"), (lse, "L")))
        assert dy.shape == x.shape == y.shape == lse.shape
        H = x.shape[1]
        dt = torch.zeros(1, dtype=torch.float32, device=x.device)
        _launch(op, self._aggr_ws, "softmax_dt", "glass_spmm_softmax_dt_f32", "glass_spmm_softmax_dt_ws_bytes",
                (x.data_ptr(), ldx, self._softmax_t(t, x), dy.data_ptr(), lddy, y.data_ptr(), ldy, lse.data_ptr(), ldl,
                 dt.data_ptr()), H)
        return dt

    # ---- K1v: aggr "std" / "var" (csrc/spmm_moment.hip) ----------------------------------------------------------------------
    def moment_fwd(self, x, kind=None, eps=1e-5):
        """(s, mu, wsum) = K1v forward: per destination and channel the weighted standard deviation sqrt(var + eps) (kind "std")
        or variance (kind "var"; None: the adjacency's own aggr) of the neighbour messages, their weighted mean, and per
        destination the sum of its weights; zeros for a row without entries."""
        self._need("moment_fwd", *MOMENT_KINDS)
        kind = self.aggr if kind is None else kind
        if kind not in MOMENT_KINDS:
            raise ValueError(f"moment_fwd: kind must be 'std' or 'var', not {kind!r}")
        op = self.fwd
        ldx = _operand(x, op.n_cols, "X")
        H = x.shape[1]
        s = _empty(x, op.n_rows, H)
        mu = _empty(x, op.n_rows, H)
        wsum = _empty(x, op.n_rows)
        _launch(op, self._aggr_ws, "moment_fwd", "glass_spmm_moment_csr_f32", "glass_spmm_moment_ws_bytes",
                (x.data_ptr(), ldx, float(eps), MOMENT_KINDS[kind], s.data_ptr(), H, mu.data_ptr(), H, wsum.data_ptr()), H)
        return s, mu, wsum

    def moment_bwd(self, x, mu, A, C=None):
        """dx of K1v from the forward's operand x, its mean mu and the caller's per-destination factors A and C (None: the mean
        carries no gradient): dx[j] = sum over the entries (destination i) of val * (C[i] + A[i] * (x[j] - mu[i]))."""
        self._need("moment_bwd", *MOMENT_KINDS)
        op = self.bwd
        ldx = _operand(x, op.n_rows, "X")
        ldmu, lda = (_operand(a, op.n_cols, n) for a, n in ((mu, "Mu"), (A, "A")))
        ldc = 0 if C is None else _operand(C, op.n_cols, "C")
        assert x.shape == mu.shape == A.shape and (C is None or C.shape == x.shape)
        H = x.shape[1]
        dx = _empty(x, op.n_rows, H)
        _launch(op, self._aggr_ws, "moment_bwd", "glass_spmm_moment_bwd_f32", "glass_spmm_moment_bwd_ws_bytes",
                (x.data_ptr(), ldx, mu.data_ptr(), ldmu, A.data_ptr(), lda, None if C is None else C.data_ptr(), ldc,
                 dx.data_ptr(), H), H)
        return dx

    # ---- K1p: aggr "pna" (csrc/spmm_pna.hip) ---------------------------------------------------------------------------------
    def pna_fwd(self, x, eps=1e-5):
        """(mu, s, mx, mn, amx, amn, wsum) = K1p forward, one gather of every source row: per destination and channel the
        weighted mean and standard deviation sqrt(var + eps) of the neighbour messages, their largest and smallest with the
        winning entries (int32, -1 for a row without entries), and per destination the sum of its weights; zeros for a row
        without entries."""
        self._need("pna_fwd", "pna")
        op = self.fwd
        ldx = _operand(x, op.n_cols, "X")
        H = x.shape[1]
        mu, s, mx, mn = (_empty(x, op.n_rows, H) for _ in range(4))
        amx, amn = (_empty(x, op.n_rows, H, dtype=torch.int32) for _ in range(2))
        wsum = _empty(x, op.n_rows)
        _launch(op, self._aggr_ws, "pna_fwd", "glass_spmm_pna_csr_f32", "glass_spmm_pna_ws_bytes",
                (x.data_ptr(), ldx, float(eps), mu.data_ptr(), H, s.data_ptr(), H, mx.data_ptr(), H, mn.data_ptr(), H,
                 amx.data_ptr(), H, amn.data_ptr(), H, wsum.data_ptr()), H)
        return mu, s, mx, mn, amx, amn, wsum

    def pna_bwd(self, x, mu, A, C, amx, gmx, amn, gmn):
        """dx of K1p from the forward's operand x, its mean mu and winners amx / amn, and the caller's per-destination rows A, C
        (ops.pna_factors), gmx and gmn (all required: zeros for a result without a gradient):
        dx[j] = sum over the entries (destination i) of val * (C[i] + A[i] * (x[j] - mu[i])) + gmx[i] where this entry won
        the max + gmn[i] where it won the min."""
        self._need("pna_bwd", "pna")
        op = self.bwd
        ldx = _operand(x, op.n_rows, "X")
        ldmu, lda, ldc, ldgx, ldgn = (_operand(a, op.n_cols, n)
                                      for a, n in ((mu, "Mu"), (A, "A"), (C, "C"), (gmx, "Gmx"), (gmn, "Gmn")))
        ldax, ldan = (_operand(a, op.n_cols, n, torch.int32) for a, n in ((amx, "Amx"), (amn, "Amn")))
        assert x.shape == mu.shape == A.shape == C.shape == gmx.shape == gmn.shape == amx.shape == amn.shape
        H = x.shape[1]
        dx = _empty(x, op.n_rows, H)
        _launch(op, self._aggr_ws, "pna_bwd", "glass_spmm_pna_bwd_f32", "glass_spmm_pna_bwd_ws_bytes",
                (x.data_ptr(), ldx, mu.data_ptr(), ldmu, A.data_ptr(), lda, C.data_ptr(), ldc, amx.data_ptr(), ldax,
                 gmx.data_ptr(), ldgx, amn.data_ptr(), ldan, gmn.data_ptr(), ldgn, dx.data_ptr(), H), H, eid_t=self.eid_t)
        return dx

    # ---- K1a: aggr "gat" (csrc/spmm_gat.hip; heads = K > 1: the glass_*_mh_* entries, csrc/spmm_gat_mh.hip) ------------------
    def _gat_vec(self, v, n, name):
        assert v.dim() == 1 and v.shape[0] == n and v.stride(0) == 1 and v.dtype == torch.float32 and v.is_cuda, \
            f"{name}: {n} contiguous fp32 on the device"
        return v.data_ptr()  # read by the kernels when they run: a captured launch follows the parameter

    @staticmethod
    def gat_head_width(H, heads):
        """D = H / heads where the multi-head kernels serve it (heads divides H, D a power of two in [4, 256]; heads == 1: any
        H); ValueError otherwise."""
        H, K = int(H), int(heads)
        if K < 1:
            raise ValueError(f"gat: heads must be an integer >= 1, not {heads!r}")
        if K == 1:
            return H
        D = H // K
        if H % K != 0 or D < 4 or D > 256 or D & (D - 1):
            raise ValueError(f"gat: {K} heads over {H} channels (D = {H / K:g}) is not supported: heads must divide the width "
                             "and D = width / heads be a power of two in [4, 256]")
        return D

    def _gat_mat(self, v, n, K, name):
        """an [n, K] temporary of the multi-head kernels, row-major"""
        assert v.shape == (n, K) and v.is_contiguous() and v.dtype == torch.float32 and v.is_cuda, \
            f"{name}: [{n}, {K}] contiguous fp32 on the device"
        return v.data_ptr()

    def _gat_form(self, H, heads):
        """(kdim, mh, tmp) of one gat call.  heads == 1 is ALWAYS the single-head entries — other kernels, with other bits, than
        glass_*_mh_* at K = 1, and they take any width: kdim (), mh "", the per-node temporaries [n], checked by
        tmp(v, n, name).  heads = K > 1: (K, ) — what follows H among the arguments and n in the temporaries' shapes [n, K] —
        and "_mh", the infix of the entries' names; a width the heads do not cut into powers of two raises here, before any
        launch."""
        if heads == 1:
            return (), "", self._gat_vec
        K = int(heads)
        self.gat_head_width(H, K)
        return (K, ), "_mh", lambda v, n, name: self._gat_mat(v, n, K, name)

    def gat_scores(self, x, att_src, att_dst, heads=1):
        """(a, b) = K1a node scores: a = x @ att_src, b = x @ att_dst, [N] each (fp64 sums, rounded once).  heads = K > 1: per
        head, over the head's columns, [N, K] each."""
        self._need("gat_scores", "gat")
        ldx = _operand(x, self.n_node, "X")
        H = x.shape[1]
        kdim, mh, _tmp = self._gat_form(H, heads)
        a = _empty(x, self.n_node, *kdim)
        b = _empty(x, self.n_node, *kdim)
        _run(f"glass_gat_scores{mh}_f32", (x.data_ptr(), ldx, self._gat_vec(att_src, H, "att_src"),
                                           self._gat_vec(att_dst, H, "att_dst"), a.data_ptr(), b.data_ptr(), self.n_node, H, *kdim))
        return a, b

    def gat_fwd(self, x, a, b, slope, heads=1):
        """(y, lse) = K1a forward: per destination the attention-weighted mean of the neighbour messages, the weights a softmax
        over the row's entries of LeakyReLU(a[source] + b[destination]); lse [N] ([N, K]) = max + log of the weighted sum of
        exponentials, kept for the backward."""
        self._need("gat_fwd", "gat")
        op = self.fwd
        ldx = _operand(x, op.n_cols, "X")
        H = x.shape[1]
        kdim, mh, tmp = self._gat_form(H, heads)
        y = _empty(x, op.n_rows, H)
        lse = _empty(x, op.n_rows, *kdim)
        _launch(op, self._aggr_ws, "gat_fwd", f"glass_spmm_gat{mh}_csr_f32", f"glass_spmm_gat{mh}_ws_bytes",
                (x.data_ptr(), ldx, tmp(a, op.n_cols, "a"), tmp(b, op.n_rows, "b"), float(slope), y.data_ptr(), H, lse.data_ptr()),
                H, *kdim)
        return y, lse

    def gat_edge(self, dy, x, y, lse, a, b, slope, heads=1):
        """(g, db) = K1a edge pass over the forward CSR: g [nnz] ([nnz, K]) the score gradient of every entry, in forward entry
        order (a sampled dense-dense product: per entry the dot of dy[destination] and x[source]), db [N] ([N, K]) its row sums."""
        self._need("gat_edge", "gat")
        op = self.fwd
        ldx = _operand(x, op.n_cols, "X")
        lddy, ldy = (_operand(t, op.n_rows, n) for t, n in ((dy, "dY"), (y, "Y")))
        assert dy.shape == x.shape == y.shape
        H = x.shape[1]
        kdim, mh, tmp = self._gat_form(H, heads)
        g = _empty(x, max(op.nnz, 1), *kdim)[:op.nnz]
        db = _empty(x, op.n_rows, *kdim)
        _launch(op, self._aggr_ws, "gat_edge", f"glass_spmm_gat{mh}_edge_f32", f"glass_spmm_gat{mh}_edge_ws_bytes",
                (x.data_ptr(), ldx, tmp(a, op.n_cols, "a"), tmp(b, op.n_rows, "b"), float(slope), dy.data_ptr(), lddy, y.data_ptr(),
                 ldy, tmp(lse, op.n_rows, "L"), g.data_ptr(), db.data_ptr()), H, *kdim)
        return g, db

    def gat_bwd(self, dy, lse, a, b, g, db, att_src, att_dst, slope, heads=1):
        """(dx, da) = K1a transposed pass: dx[j] = the attention-weighted sum of dy over the entries that read x[j], plus
        da[j] att_src + db[j] att_dst; da [N] ([N, K]) = the sums of g over those entries."""
        self._need("gat_bwd", "gat")
        op = self.bwd
        lddy = _operand(dy, op.n_cols, "dY")
        H = dy.shape[1]
        kdim, mh, tmp = self._gat_form(H, heads)
        dx = _empty(dy, op.n_rows, H)
        da = _empty(dy, op.n_rows, *kdim)
        _launch(op, self._aggr_ws, "gat_bwd", f"glass_spmm_gat{mh}_bwd_f32", f"glass_spmm_gat{mh}_bwd_ws_bytes",
                (tmp(a, op.n_rows, "a"), tmp(b, op.n_cols, "b"), float(slope), dy.data_ptr(), lddy, tmp(lse, op.n_cols, "L"),
                 tmp(g, op.nnz, "g"), tmp(db, op.n_rows, "db"), self._gat_vec(att_src, H, "att_src"),
                 self._gat_vec(att_dst, H, "att_dst"), dx.data_ptr(), H, da.data_ptr()), H, *kdim, eid_t=self.eid_t)
        return dx, da

    def gat_da(self, g, dy, heads=1):
        """da alone (gat_bwd's second result, the same bits) when no dx is wanted; dy only names the lane layout gat_bwd would
        take (its width, stride and alignment)."""
        self._need("gat_da", "gat")
        op = self.bwd
        lddy = _operand(dy, op.n_cols, "dY")
        H = dy.shape[1]
        kdim, mh, tmp = self._gat_form(H, heads)
        da = _empty(g, op.n_rows, *kdim)
        # gat_bwd's 16-byte form (its own dx and workspace are 16-byte aligned); several heads have H % 4 == 0 by their width
        vec = H % 4 == 0 and lddy % 4 == 0 and dy.data_ptr() % 16 == 0
        _launch(op, self._aggr_ws, "gat_da", f"glass_spmm_gat{mh}_da_f32", f"glass_spmm_gat{mh}_da_ws_bytes",
                (tmp(g, op.nnz, "g"), da.data_ptr()), H, *kdim, eid_t=self.eid_t, tail=(int(vec), ))
        return da

    def gat_datt(self, x, da, db, heads=1):
        """(datt_src, datt_dst) = x^T da, x^T db: the attention vectors' gradients, run only when they are trained."""
        self._need("gat_datt", "gat")
        ldx = _operand(x, self.n_node, "X")
        H = x.shape[1]
        kdim, mh, tmp = self._gat_form(H, heads)
        ds = torch.zeros(H, dtype=torch.float32, device=x.device)
        dd = torch.zeros(H, dtype=torch.float32, device=x.device)
        entry = f"glass_gat_datt{mh}_f32"
        ws = self._aggr_ws.fetch("gat_datt", (H, *kdim), getattr(_lib.load(), f"glass_gat_datt{mh}_ws_bytes")(self.n_node, H))
        _run(entry, (x.data_ptr(), ldx, tmp(da, self.n_node, "da"), tmp(db, self.n_node, "db"), ds.data_ptr(), dd.data_ptr(),
                     self.n_node, H, *kdim, ws.data_ptr()))
        return ds, dd

    # ---- K1a2: aggr "gatv2" (csrc/spmm_gatv2.hip) ---------------------------------------------------------------------------
    # (an adjacency without entries launches nothing: the entries return at once, and the results, all zero, are made here)
    def _gatv2_out(self, like, *shape):
        return (torch.zeros if self.nnz == 0 else torch.empty)(shape, dtype=torch.float32, device=like.device)

    def gatv2_score(self, x, att, slope):
        """s [nnz] = K1a2 score pass: per entry of the forward CSR the dot of att with LeakyReLU(x[destination] + x[source]),
        in forward entry order (products and sum in fp64, rounded once).  Every later pass reads it."""
        self._need("gatv2_score", "gatv2")
        op = self.fwd
        ldx = _operand(x, op.n_cols, "X")
        H = x.shape[1]
        s = _empty(x, max(op.nnz, 1))[:op.nnz]
        _launch(op, self._aggr_ws, "gatv2_score", "glass_spmm_gatv2_score_f32", "glass_spmm_gatv2_score_ws_bytes",
                (x.data_ptr(), ldx, self._gat_vec(att, H, "att"), float(slope), s.data_ptr()), H)
        return s

    def gatv2_fwd(self, x, s):
        """(y, lse) = K1a2 forward: per destination the attention-weighted mean of the neighbour messages, the weights a softmax
        over the row's entries of s; lse [N] = max + log of the weighted sum of exponentials, kept for the backward."""
        self._need("gatv2_fwd", "gatv2")
        op = self.fwd
        ldx = _operand(x, op.n_cols, "X")
        H = x.shape[1]
        y = self._gatv2_out(x, op.n_rows, H)
        lse = self._gatv2_out(x, op.n_rows)
        _launch(op, self._aggr_ws, "gatv2_fwd", "glass_spmm_gatv2_csr_f32", "glass_spmm_gatv2_ws_bytes",
                (x.data_ptr(), ldx, self._gat_vec(s, op.nnz, "s"), y.data_ptr(), H, lse.data_ptr()), H)
        return y, lse

    def gatv2_edge(self, dy, x, y, lse, s, att, slope):
        """(g, p, gd, r) = K1a2 edge pass over the forward CSR, one gather of x[source] per entry: p [nnz] the attention weights,
        g [nnz] the score gradients, gd [N, H] the destination side of dx (the row sums of g att f) and r [N, H] the row sums
        of g LeakyReLU(x[destination] + x[source]), whose column sums are att's gradient."""
        self._need("gatv2_edge", "gatv2")
        op = self.fwd
        ldx = _operand(x, op.n_cols, "X")
        lddy, ldy = (_operand(t, op.n_rows, n) for t, n in ((dy, "dY"), (y, "Y")))
        assert dy.shape == x.shape == y.shape
        H = x.shape[1]
        g = _empty(x, max(op.nnz, 1))[:op.nnz]
        p = _empty(x, max(op.nnz, 1))[:op.nnz]
        gd = self._gatv2_out(x, op.n_rows, H)
        r = self._gatv2_out(x, op.n_rows, H)
        _launch(op, self._aggr_ws, "gatv2_edge", "glass_spmm_gatv2_edge_f32", "glass_spmm_gatv2_edge_ws_bytes",
                (x.data_ptr(), ldx, self._gat_vec(att, H, "att"), float(slope), self._gat_vec(s, op.nnz, "s"), dy.data_ptr(), lddy,
                 y.data_ptr(), ldy, self._gat_vec(lse, op.n_rows, "L"), g.data_ptr(), p.data_ptr(), gd.data_ptr(), r.data_ptr()), H)
        return g, p, gd, r

    def gatv2_bwd(self, dy, x, p, g, gd, att, slope):
        """dx = K1a2 transposed pass: dx[j] = the sum over the entries that read x[j] of p dy[destination] + g att f, plus gd[j]."""
        self._need("gatv2_bwd", "gatv2")
        op = self.bwd
        lddy = _operand(dy, op.n_cols, "dY")
        ldx = _operand(x, op.n_rows, "X")
        H = dy.shape[1]
        assert gd.shape == (op.n_rows, H) and gd.is_contiguous() and gd.dtype == torch.float32 and gd.is_cuda, "gd"
        dx = self._gatv2_out(dy, op.n_rows, H)
        _launch(op, self._aggr_ws, "gatv2_bwd", "glass_spmm_gatv2_bwd_f32", "glass_spmm_gatv2_bwd_ws_bytes",
                (x.data_ptr(), ldx, self._gat_vec(att, H, "att"), float(slope), dy.data_ptr(), lddy, self._gat_vec(p, op.nnz, "p"),
                 self._gat_vec(g, op.nnz, "g"), gd.data_ptr(), dx.data_ptr(), H), H, eid_t=self.eid_t)
        return dx

    def gatv2_datt(self, r):
        """datt [H] = the column sums of r (fp64 partials, a fixed order): att's gradient, run only when it is trained."""
        self._need("gatv2_datt", "gatv2")
        n, H = self.n_node, r.shape[1]
        assert r.shape == (n, H) and r.is_contiguous() and r.dtype == torch.float32 and r.is_cuda, "r"
        datt = torch.zeros(H, dtype=torch.float32, device=r.device)
        ws = self._aggr_ws.fetch("gatv2_datt", (H, ), _lib.load().glass_spmm_gatv2_datt_ws_bytes(n, H))
        _run("glass_spmm_gatv2_datt_f32", (r.data_ptr(), datt.data_ptr(), n, H, ws.data_ptr()))
        return datt

    def to_dense(self):
        """Dense [N,N] (tests on tiny graphs only)."""
        n = self.n_node
        rp = self.fwd.rowptr.to(torch.int64)
        rows = torch.repeat_interleave(torch.arange(n, device=rp.device), rp[1:] - rp[:-1])
        a = torch.zeros(n * n, dtype=torch.float32, device=rp.device)
        a.index_add_(0, rows * n + self.fwd.col.to(torch.int64), self.fwd.val)
        return a.reshape(n, n)


class Selection:
    """Transpose of the [N,V] one-hot selection matrix of an embedding lookup (x is static per
    dataset): CSR with V rows whose columns are the node ids using that table row, values 1.
    `dW = S^T @ dout` is the embedding backward (ATen embedding_dense_backward) run on K1."""
    def __init__(self, x_flat, n_rows_table):
        n = x_flat.shape[0]
        lo, hi = int(x_flat.min()), int(x_flat.max())  # one-time validation (nn.Embedding raises IndexError)
        if lo < 0 or hi >= n_rows_table:
            raise IndexError(f"index out of range in embedding: [{lo},{hi}] vs table of {n_rows_table} rows")
        perm = torch.argsort(x_flat, stable=True)
        rowptr = _csr_from_sorted(x_flat[perm], n_rows_table)
        self.op = CSROperand(rowptr, perm.to(torch.int32).contiguous(),
                             torch.ones(n, dtype=torch.float32, device=x_flat.device), n_rows_table, n)
        # the same plan with its reduce launch switched off (header word 6 = number of reduce rows): the consumer sums the
        # partial rows itself (glass_embed_norm_bwd_adam_f32)
        self._hdr_noreduce = self.op.header.copy()
        self._n_reduce = int(self.op.header[6])
        self._off_reduce = int(self.op.header[12])
        self._hdr_noreduce[6] = 0

    def product_without_reduce(self, x):
        """G = S^T @ x on K1 WITHOUT the final reduce launch: rows cut into several chunks are left as partial rows.
        Returns (G, partials pointer, device pointer of the plan's reduce list, number of reduce rows)."""
        op = self.op
        H = x.shape[1]
        G = _empty(x, op.n_rows, H)
        # (on op.workspace(H): the size does not depend on the reduce rows)
        ws = _launch(op, op._ws, "spmm", "glass_spmm_csr_f32", "glass_spmm_ws_bytes",
                     (x.data_ptr(), x.stride(0), G.data_ptr(), G.stride(0)), H, header=self._hdr_noreduce)
        return G, ws.data_ptr(), op.plan.data_ptr() + 4 * self._off_reduce, self._n_reduce
