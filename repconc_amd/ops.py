"""Tensor-level wrappers over the C ABI (include/repconc_hip.h).

Every function takes CUDA(=HIP) torch tensors, launches on `torch.cuda.current_stream()` of the
tensor's device and returns without synchronising.  torch is used for memory and streams only;
all arithmetic happens in librepconc_hip.so.  CPU tensors are rejected: there is no fallback.
"""
from __future__ import annotations

import collections
import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

K = 256
SUPPORTED_DSUB = (8, 12, 16, 24, 32, 48, 64, 96)


def _need_cuda(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.RepconcHipError(
                "repconc_amd runs on the GPU only (got a CPU tensor); the package has no CPU fallback")


def _ctx(t: torch.Tensor):
    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    return _lib.load(), _lib.handle(dev), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), dev


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _rows_f32(x: torch.Tensor) -> torch.Tensor:
    """fp32 [B, D] with unit inner stride and 16-byte aligned rows (fp16/bf16 inputs are promoted
    exactly like the reference's fp32 centroids promote them)."""
    if x.dim() != 2:
        raise ValueError("expected a [B, D] matrix")
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(1) != 1 or x.stride(0) % 4 != 0 or x.data_ptr() % 16 != 0:
        x = x.contiguous()                                  # no copy of contiguous rows whose width is no multiple of 4
        if x.data_ptr() % 16 != 0:                          # already contiguous, at an odd storage offset: .contiguous() copied nothing
            x = x.clone()
    return x


def _centroids(c: torch.Tensor) -> torch.Tensor:
    if c.dim() != 3 or c.shape[1] != K:
        raise ValueError("centroids must be [M, 256, dsub]")
    c = c.detach()
    if c.dtype != torch.float32 or not c.is_contiguous():
        c = c.float().contiguous()
    if c.data_ptr() % 16 != 0:                              # a contiguous view at an odd storage offset: the kernels load float4
        c = c.clone()
    return c


def _shape(x: torch.Tensor, c: torch.Tensor):
    B, D = x.shape
    M, _, dsub = c.shape
    if D != M * dsub:
        raise ValueError(f"embedding width {D} != M*dsub = {M}*{dsub}")
    # every width is served: SUPPORTED_DSUB are the widths with specialised kernels (the recipes'), any other divisor goes
    # through the run-time-width kernels with the same arithmetic (csrc/pq_distance.hip, "any width")
    return B, D, M, dsub


def _code_dtype(codes: torch.Tensor) -> int:
    if codes.dtype == torch.uint8:
        return _lib.RC_CODE_U8
    if codes.dtype == torch.int64:
        return _lib.RC_CODE_I64
    raise ValueError("codes must be uint8 or int64")


# --------------------------------------------------------------------------- nearest codes
def assign_nearest(x: torch.Tensor, centroids: torch.Tensor, dtype=torch.int64, method: str = "auto",
                   stats: dict | None = None) -> torch.Tensor:
    """argmin_k ||x_m - C[m,k]||^2 -> codes [B, M].  modeling_repconc.py:49-52,66.

    method: "exact" = every distance in the reference's fp32 order (rc_pq_assign_nearest); "mfma" = matrix-core screen
    + exact recomputation of the doubtful pairs (rc_pq_assign_nearest_fast) — the same codes, bit for bit; "auto" =
    mfma when its alignment preconditions hold.  stats (optional dict) receives {"method", "doubtful"}.
    """
    _need_cuda(x, centroids)
    x, c = _rows_f32(x), _centroids(centroids)
    B, D, M, dsub = _shape(x, c)
    lib, h, s, _ = _ctx(x)
    codes = torch.empty((B, M), dtype=dtype, device=x.device)
    u8 = codes if dtype == torch.uint8 else None
    i64 = codes if dtype == torch.int64 else None
    if u8 is None and i64 is None:
        raise ValueError("dtype must be torch.uint8 or torch.int64")
    if method not in ("auto", "exact", "mfma"):
        raise ValueError("method must be auto|exact|mfma")
    if B == 0:
        return codes
    fast_ok = x.data_ptr() % 16 == 0 and x.stride(0) % 4 == 0 and B * M < 2 ** 32
    if method == "mfma" and not fast_ok:
        raise _lib.RepconcHipError("mfma assignment needs 16-byte aligned rows, ldx % 4 == 0 and B*M < 2^32")
    # a width without a matrix-core screen goes straight to the exact entry: the fast one would only fall through to it, and
    # leave its workspace, the doubt count with it, unwritten
    if method != "exact" and fast_ok and dsub in SUPPORTED_DSUB:
        n = lib.rc_pq_assign_nearest_fast_ws_bytes(B, M)
        ws = torch.empty(n, dtype=torch.uint8, device=x.device)
        _lib.check(lib.rc_pq_assign_nearest_fast(h, _p(x), x.stride(0), _p(c), B, D, M, K, _p(u8), _p(i64), _p(ws), n, s),
                   "rc_pq_assign_nearest_fast", h)
        if stats is not None:                               # statistics only: this (and nothing else) synchronises
            doubtful = C.c_int(0)
            over = lib.rc_pq_assign_nearest_fast_overflow(h, _p(ws), B, M, C.byref(doubtful))
            if over < 0:
                _lib.check(over, "rc_pq_assign_nearest_fast_overflow", h)
            stats.update(method="mfma", doubtful=int(doubtful.value), overflow=bool(over))
        return codes
    _lib.check(lib.rc_pq_assign_nearest(h, _p(x), x.stride(0), _p(c), B, D, M, K, _p(u8), _p(i64), s),
               "rc_pq_assign_nearest", h)
    if stats is not None:
        stats.setdefault("doubtful", 0)
        stats["method"] = "exact"
    return codes


def assign_margin(dsub: int) -> float:
    """The compiled margin of the matrix-core screen of assign_nearest: a (row, sub-quantiser) pair is re-judged exactly
    unless its best screened value leads the second best by more than margin * (||x_m||^2 + max_k ||c_mk||^2).  Needs no GPU."""
    v = float(_lib.load().rc_pq_assign_nearest_fast_margin(int(dsub)))
    if v < 0:
        raise ValueError(f"no matrix-core screen for dsub = {dsub}")
    return v


# --------------------------------------------------------------------------- distance table
def dist_table(x: torch.Tensor, centroids: torch.Tensor, with_minmax: bool = True):
    """d [M,B,K] fp32 (+ minmax [2M]: max then min per m).  modeling_repconc.py:50,76-77."""
    _need_cuda(x, centroids)
    x, c = _rows_f32(x), _centroids(centroids)
    B, D, M, _ = _shape(x, c)
    lib, h, s, _ = _ctx(x)
    d = torch.empty((M, B, K), dtype=torch.float32, device=x.device)
    if B == 0:
        # no rows, no launch (an empty tensor has no pointer for the entry to take): the range of an empty table is the
        # neutral pair of the max / min reduction, as the solve fills it in for a rank without rows (solve_fill_range_kernel)
        inf = float("inf")
        return d, (torch.tensor([-inf] * M + [inf] * M, dtype=torch.float32).to(x.device) if with_minmax else None)
    mm = torch.empty((2 * M,), dtype=torch.float32, device=x.device) if with_minmax else None
    wsb = lib.rc_pq_dist_table_ws_bytes(B, M)
    ws = torch.empty((max(wsb, 1),), dtype=torch.uint8, device=x.device)
    _lib.check(lib.rc_pq_dist_table(h, _p(x), x.stride(0), _p(c), B, D, M, K, _p(d), _p(mm), _p(ws), wsb, s),
               "rc_pq_dist_table", h)
    return d, mm


def centre_(d: torch.Tensor, minmax: torch.Tensor) -> torch.Tensor:
    """In-place center_distance_for_constraint, modeling_repconc.py:81-84."""
    _need_cuda(d, minmax)
    M, B, _ = d.shape
    lib, h, s, _ = _ctx(d)
    _lib.check(lib.rc_pq_centre(h, _p(d), _p(minmax), B, M, K, s), "rc_pq_centre", h)
    return d


# --------------------------------------------------------------------------- Sinkhorn stages
def sinkhorn_potentials_f64(out: torch.Tensor, eps: float, iters: int, allgather=None) -> torch.Tensor:
    """Row potentials f [M,K] (fp64) of `iters` Sinkhorn iterations on ANY fp64 cost tensor out [M,K,B] (this rank's columns) —
    rc_sk64_rows / rc_sk64_cols, modeling_repconc.py:137-165.  `allgather(t[M,K]) -> [G,M,K]` moves the row values between
    ranks (None: one rank).  The plan is softmax_k(out / eps + f)."""
    _need_cuda(out)
    if out.dtype != torch.float64 or out.dim() != 3 or out.shape[1] != K:
        raise _lib.RepconcHipError(f"out must be fp64 [M, {K}, B], got {out.dtype} {tuple(out.shape)}")
    out = out.contiguous()
    M, _, B = out.shape
    lib, h, s, _ = _ctx(out)
    dev = out.device
    lse = torch.empty((M, K), dtype=torch.float64, device=dev)
    f = torch.empty((M, K), dtype=torch.float64, device=dev)
    g = torch.empty((M, max(B, 1)), dtype=torch.float64, device=dev)
    gather = allgather if allgather is not None else (lambda t: t.unsqueeze(0))

    def rows(gp):
        _lib.check(lib.rc_sk64_rows(h, _p(out), _p(gp), B, M, K, float(eps), _p(lse), s), "rc_sk64_rows", h)

    def cols(want_g):
        lg = gather(lse).contiguous()
        _lib.check(lib.rc_sk64_cols(h, _p(out), _p(lg), lg.shape[0], B, M, K, float(eps), _p(f), _p(g if want_g else None), s),
                   "rc_sk64_cols", h)
    rows(None)
    for _ in range(1, int(iters)):
        cols(True)
        rows(g)
    cols(False)
    return f


class SinkhornState:
    """Device buffers of one rank's Sinkhorn solve over a centred table d [M,B,K] (staged C ABI).

        rows = st.sweep(eps, 0, None)                    # sweep 0
        for t in 1 .. T-1:  rows = st.sweep(eps, t, gathered(rows))
        codes = st.argmax(eps, T, gathered(rows))

    `gathered(rows)` is the [G,M,K] stack of every rank's row sums (G = 1: rows.unsqueeze(0))."""

    def __init__(self, d: torch.Tensor):
        _need_cuda(d)
        self.d = d
        self.M, self.B, _ = d.shape
        dev = d.device
        self.f2 = torch.empty((2, self.M, K), dtype=torch.float64, device=dev)
        self.g = torch.empty((self.M, self.B), dtype=torch.float64, device=dev)
        self.colsum = torch.empty((self.M, self.B), dtype=torch.float64, device=dev)
        self._rows = torch.empty((2, self.M, K), dtype=torch.float64, device=dev)
        self.flags = torch.zeros((1,), dtype=torch.int32, device=dev)
        lib = _lib.load()
        self._wsb = lib.rc_sk_ws_bytes(self.B, self.M, K)
        self._ws = torch.empty((max(self._wsb, 1),), dtype=torch.uint8, device=dev)

    @staticmethod
    def _gathered(rows_prev):
        if rows_prev is None:
            return None, 0
        if rows_prev.dim() == 2:
            rows_prev = rows_prev.unsqueeze(0)
        return rows_prev.contiguous(), rows_prev.shape[0]

    def sweep(self, eps: float, t: int, rows_prev: Optional[torch.Tensor]) -> torch.Tensor:
        """Sweep t; returns this rank's row sums [M,K] (a buffer that stays valid until sweep t+2)."""
        lib, h, s, _ = _ctx(self.d)
        rp, G = self._gathered(rows_prev)
        out = self._rows[t & 1]
        _lib.check(lib.rc_sk_sweep(h, _p(self.d), _p(rp), G, _p(self.f2), _p(self.g), _p(self.colsum), _p(out),
                                   self.B, self.M, K, float(eps), int(t), _p(self.flags), _p(self._ws), self._wsb, s),
                   "rc_sk_sweep", h)
        return out

    def argmax(self, eps: float, t: int, rows_prev: torch.Tensor, dtype=torch.int64) -> torch.Tensor:
        lib, h, s, _ = _ctx(self.d)
        rp, G = self._gathered(rows_prev)
        codes = torch.empty((self.B, self.M), dtype=dtype, device=self.d.device)
        u8 = codes if dtype == torch.uint8 else None
        i64 = codes if dtype == torch.int64 else None
        _lib.check(lib.rc_sk_argmax(h, _p(self.d), _p(rp), G, _p(self.f2), self.B, self.M, K, float(eps), int(t),
                                    _p(u8), _p(i64), _p(self.flags), s), "rc_sk_argmax", h)
        return codes

    def potentials(self, t: int, rows_prev: torch.Tensor) -> torch.Tensor:
        """f [M,K] after t row normalisations (what rc_sk_argmax(t) uses); bookkeeping on [M,K] only."""
        rp, _ = self._gathered(rows_prev)
        tot = rp[0].clone()
        for r in range(1, rp.shape[0]):
            tot = tot + rp[r]
        prev = torch.zeros_like(tot) if t == 1 else self.f2[(t - 1) & 1]
        return prev - torch.log(tot)


def assign_sinkhorn(x: torch.Tensor, centroids: torch.Tensor, eps: float, iters: int,
                    dtype=torch.int64) -> Tuple[torch.Tensor, torch.Tensor]:
    """Single-rank constrained codes [B,M] + flags (int32[1]).  modeling_repconc.py:47-67 with
    dist.is_initialized()==False.  One C call: distance table, centring, `iters` Sinkhorn
    iterations, argmax."""
    _need_cuda(x, centroids)
    x, c = _rows_f32(x), _centroids(centroids)
    B, D, M, _ = _shape(x, c)
    lib, h, s, _ = _ctx(x)
    codes = torch.empty((B, M), dtype=dtype, device=x.device)
    flags = torch.zeros((1,), dtype=torch.int32, device=x.device)
    if B == 0:
        return codes, flags
    wsb = lib.rc_pq_assign_sinkhorn_ws_bytes(B, M, K)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=x.device)
    u8 = codes if dtype == torch.uint8 else None
    i64 = codes if dtype == torch.int64 else None
    _lib.check(lib.rc_pq_assign_sinkhorn(h, _p(x), x.stride(0), _p(c), B, D, M, K, float(eps), int(iters),
                                         _p(u8), _p(i64), _p(flags), _p(ws), wsb, s), "rc_pq_assign_sinkhorn", h)
    return codes, flags


# --------------------------------------------------------------------------- N ranks, native loop
_comm_ready = {}
_dist_ws = {}          # device index -> persistent workspace of assign_sinkhorn_dist


def comm_transport() -> str:
    """RC_COMM=ipc|rccl|auto (default auto): how the ranks exchange the Sinkhorn row sums and k-means statistics.
    ipc = hand-written peer stores into IPC-mapped receive buffers (csrc/comm.hip; works between processes on ONE GPU
    too; all ranks on one node, at most 16), rccl = two RCCL communicators (one GPU per rank; any number of nodes).
    auto = ipc where it can work (one node, world <= 16), else rccl; a failed IPC connect falls back to rccl on ALL ranks."""
    import os
    v = os.environ.get("RC_COMM", "auto").lower()
    if v not in ("ipc", "rccl", "auto"):
        raise ValueError("RC_COMM must be ipc, rccl or auto")
    return v


RC_IPC_MAX_WORLD = 16
IPC_MAX_M = 128        # csrc/comm.hip: IPC_XMAX_M (sub-quantisers per chain on the IPC transport)


def _all_ranks_ok(ok: bool, group) -> bool:
    """Collective AND over the group (any backend): a set-up step either worked on every rank or is undone on every rank."""
    import torch.distributed as dist
    flags = [None] * dist.get_world_size(group)
    dist.all_gather_object(flags, bool(ok), group=group)
    return all(flags)


def _same_node(group) -> bool:
    import socket
    import torch.distributed as dist
    names = [None] * dist.get_world_size(group)
    dist.all_gather_object(names, socket.gethostname(), group=group)
    return len(set(names)) == 1


def _connect_ipc(lib, h, rank, world, group) -> bool:
    """Export + connect on every rank; False (with the handle released again) on every rank if any rank failed."""
    import torch.distributed as dist
    blob = (C.c_char * _lib.RC_IPC_BLOB_BYTES)()
    ok = lib.rc_comm_ipc_export(h, rank, world, C.cast(blob, C.c_void_p)) == _lib.RC_OK
    blobs = [None] * world
    dist.all_gather_object(blobs, bytes(blob.raw) if ok else None, group=group)
    if all(b is not None for b in blobs):
        raw = (C.c_char * (_lib.RC_IPC_BLOB_BYTES * world)).from_buffer_copy(b"".join(blobs))
        ok = lib.rc_comm_ipc_connect(h, C.cast(raw, C.c_void_p)) == _lib.RC_OK
    else:
        ok = False
    ok = _all_ranks_ok(ok, group)                           # also the barrier: every rank has mapped every buffer
    if not ok:
        lib.rc_comm_destroy(h)                              # releases an exported-but-unconnected buffer too
    return ok


def _connect_rccl(lib, h, dev, rank, world, group) -> bool:
    import torch.distributed as dist
    ids = torch.zeros(256, dtype=torch.uint8)
    if rank == 0:
        buf = (C.c_char * 256)()
        _lib.check(lib.rc_comm_unique_ids(C.cast(buf, C.c_void_p)), "rc_comm_unique_ids")
        ids = torch.frombuffer(bytearray(buf.raw), dtype=torch.uint8).clone()
    if world > 1:
        backend = dist.get_backend(group)
        t = ids.to(torch.device("cuda", dev)) if backend == "nccl" else ids
        dist.broadcast(t, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        ids = t.cpu()
    raw = (C.c_char * 256).from_buffer_copy(bytes(ids.numpy().tobytes()))
    ok = lib.rc_comm_init(h, C.cast(raw, C.c_void_p), rank, world) == _lib.RC_OK
    ok = _all_ranks_ok(ok, group) if world > 1 else ok
    if not ok:
        lib.rc_comm_destroy(h)
    return ok


def comm_init(group=None, transport: Optional[str] = None) -> str:
    """Set up the exchange layer of this process's handle (once per process group); returns the transport that runs.
    Only the set-up handshake goes through torch.distributed (any backend): the IPC descriptors (128 bytes per rank,
    all-gathered) or the RCCL unique ids (256 bytes, broadcast from rank 0); everything after that happens inside
    librepconc_hip.so.  COLLECTIVE: every rank of the group calls it, every step is agreed on by all ranks (a connect that
    fails on one rank is undone on all of them), and all ranks end on the same transport or all raise — no rank is left
    spinning in IPC waits while another has fallen back.  transport = "auto" (default, RC_COMM): ipc when all ranks share
    a host and world <= 16, else rccl; ipc that fails to connect falls back to rccl."""
    import torch.distributed as dist
    dev = torch.cuda.current_device()
    want = (transport or comm_transport()).lower()
    key0 = id(group) if group is not None else 0
    ready = _comm_ready.get(dev)
    if ready is not None and ready[0] == key0 and (want == "auto" or ready[1] == want):
        return ready[1]
    lib, h = _lib.load(), _lib.handle(dev)
    if dev in _comm_ready:                                  # another process group / transport: start over
        comm_destroy(group_barrier=False)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    import logging
    log = logging.getLogger(__name__)
    tried = []
    if want in ("ipc", "auto"):
        ipc_possible = world <= RC_IPC_MAX_WORLD and _same_node(group)
        if ipc_possible and _connect_ipc(lib, h, rank, world, group):
            _comm_ready[dev] = (key0, "ipc")
            log.info("comm_init: rank %d / %d on cuda:%d exchanges over the IPC transport", rank, world, dev)
            return "ipc"
        tried.append("ipc (world > 16 or ranks on several hosts)" if not ipc_possible else "ipc (export / connect failed on a rank)")
        # an EXPLICIT request for ipc (argument or RC_COMM=ipc) is strict: ranks that share one GPU cannot run RCCL at all
        # (its ncclCommInitRank would hang, not fail), so only "auto" falls back.  RC_COMM_STRICT=0 restores the fall-back.
        if want == "ipc" and rc_env_strict(default=True):
            raise _lib.RepconcHipError("comm_init: the IPC transport was requested and is unavailable: " + tried[-1] +
                                       " (RC_COMM=auto or RC_COMM_STRICT=0 fall back to rccl)")
        log.warning("comm_init: %s; falling back to rccl", tried[-1])
    if _connect_rccl(lib, h, dev, rank, world, group):
        _comm_ready[dev] = (key0, "rccl")
        log.info("comm_init: rank %d / %d on cuda:%d exchanges over RCCL", rank, world, dev)
        return "rccl"
    tried.append("rccl (rc_comm_init failed on a rank)")
    raise _lib.RepconcHipError("comm_init: no exchange transport could be set up on all ranks: " + "; ".join(tried))


def rc_env_strict(default: bool = False) -> bool:
    """RC_COMM_STRICT=1 / 0: whether an explicitly requested transport that is unavailable raises instead of falling back."""
    import os
    v = os.environ.get("RC_COMM_STRICT", "")
    return default if v == "" else v == "1"


_comm_flags = {}       # device index -> int32 flags word passed to every rc_comm_allgather of that device


def comm_check(device=None) -> None:
    """Raise if an exchange of this device's handle has timed out since comm_init() (RC_FLAG_COMM: a peer rank is missing or
    more than RC_IPC_TIMEOUT_MS behind; the transport is broken from then on and every later gather is flagged).
    Synchronises — call where the results of the gathers are consumed (the multi-rank paths of the package do)."""
    if not _comm_flags:                                     # no native gather has run (CPU / torch.distributed paths)
        return
    if isinstance(device, torch.device):
        if device.type != "cuda":
            return
        device = device.index
    dev = torch.cuda.current_device() if device is None else int(device)
    fl = _comm_flags.get(dev)
    if fl is not None and int(fl.item()) & _lib.RC_FLAG_COMM:
        raise _lib.RepconcHipError("an inter-rank exchange timed out (RC_FLAG_COMM): a peer rank is missing or more than "
                                   "RC_IPC_TIMEOUT_MS behind; the gathered data of this and every later exchange is invalid")


def comm_destroy(group=None, group_barrier: bool = True):
    """Release the exchange layer of the current device's handle.  With the IPC transport no peer may still be storing
    into this rank's buffer: `group_barrier` synchronises the device and the process group first."""
    dev = torch.cuda.current_device()
    if dev not in _comm_ready:
        return
    if group_barrier:
        import torch.distributed as dist
        torch.cuda.synchronize(dev)
        if dist.is_initialized():
            dist.barrier(group=group)
    lib, h = _lib.load(), _lib.handle(dev)
    _lib.check(lib.rc_comm_destroy(h), "rc_comm_destroy", h)
    del _comm_ready[dev]
    _comm_flags.pop(dev, None)


def comm_allgather(t: torch.Tensor, flags: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[world, *t.shape] stack of every rank's `t` (same shape and dtype on all ranks) through the handle's exchange
    layer (rc_comm_allgather; comm_init() first), on the current stream."""
    _need_cuda(t)
    t = t.contiguous()
    lib, h, s, _ = _ctx(t)
    world = lib.rc_comm_world(h)
    if world < 1:
        raise _lib.RepconcHipError("comm_allgather: call ops.comm_init() first")
    out = torch.empty((world,) + tuple(t.shape), dtype=t.dtype, device=t.device)
    if flags is None:                                       # the device's own flags word: comm_check() reads it
        dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
        flags = _comm_flags.get(dev)
        if flags is None:
            flags = _comm_flags[dev] = torch.zeros((1,), dtype=torch.int32, device=t.device)
    _lib.check(lib.rc_comm_allgather(h, _p(t), _p(out), t.numel() * t.element_size(), _p(flags), s), "rc_comm_allgather", h)
    return out


def all_gather(t: torch.Tensor, group=None) -> torch.Tensor:
    """[world, *t.shape] stack of every rank's `t`: through the handle's own exchange layer when comm_init() has been
    called for this process group on t's device (IPC peer stores or RCCL, from C), otherwise through torch.distributed.
    The ONE all-gather the multi-rank code paths (k-means statistics run_warmup.py:102-113, row-sharded / replicated
    search results evaluate_repconc.py:121-135) are written against."""
    import torch.distributed as dist
    if t.is_cuda:
        dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
        ready = _comm_ready.get(dev)
        if ready is not None and ready[0] == (id(group) if group is not None else 0):
            return comm_allgather(t)
    G = dist.get_world_size(group)
    out = torch.empty((G,) + tuple(t.shape), dtype=t.dtype, device=t.device)
    dist.all_gather_into_tensor(out.view(-1), t.contiguous().view(-1), group=group)
    return out


def assign_sinkhorn_dist(x: torch.Tensor, centroids: torch.Tensor, eps: float, iters: int, dtype=torch.int64):
    """This rank's codes of the batch-sharded constrained assignment, the whole solve in one C call
    (rc_pq_assign_sinkhorn_dist; comm_init() first).  modeling_repconc.py:47-67 with dist.is_initialized()."""
    _need_cuda(x, centroids)
    x, c = _rows_f32(x), _centroids(centroids)
    B, D, M, _ = _shape(x, c)
    lib, h, s, _ = _ctx(x)
    world = lib.rc_comm_world(h)
    if world < 1:
        raise _lib.RepconcHipError("assign_sinkhorn_dist: call ops.comm_init() first")
    if lib.rc_comm_kind(h) == 2 and M > IPC_MAX_M * lib.rc_solve_num_chains_on(h, world, M):
        raise _lib.RepconcHipError(f"assign_sinkhorn_dist: MCQ_M = {M} exceeds what the IPC transport exchanges per chain "
                                   f"({IPC_MAX_M} sub-quantisers: [M, 256] fp64 row sums through a 256 KiB slot); "
                                   "set RC_COMM=rccl for this model")
    codes = torch.empty((B, M), dtype=dtype, device=x.device)
    flags = torch.zeros((1,), dtype=torch.int32, device=x.device)
    # a rank without rows (ragged last batch) still takes part in every collective of the solve
    wsb = lib.rc_pq_assign_sinkhorn_dist_ws_bytes(B, M, K, world)
    # The iteration graph (csrc/comm.hip) is cached per workspace ADDRESS: keep one block per device and reuse it while
    # it is large enough, instead of asking the caching allocator for a (possibly different) block on every call.  The
    # block is only touched by this function, on the caller's stream, so consecutive solves are ordered by the stream.
    dev = x.device.index if x.device.index is not None else torch.cuda.current_device()
    ws = _dist_ws.get(dev)
    if ws is None or ws.numel() < wsb:
        _dist_ws.pop(dev, None)
        ws = _dist_ws[dev] = torch.empty((wsb,), dtype=torch.uint8, device=x.device)
    u8 = codes if dtype == torch.uint8 else None
    i64 = codes if dtype == torch.int64 else None
    _lib.check(lib.rc_pq_assign_sinkhorn_dist(h, _p(x), x.stride(0), _p(c), B, D, M, K, float(eps), int(iters),
                                              _p(u8), _p(i64), _p(flags), _p(ws), wsb, s), "rc_pq_assign_sinkhorn_dist", h)
    return codes, flags


# --------------------------------------------------------------------------- decode
def decode_raw(codes: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
    """out[n, m*dsub:(m+1)*dsub] = centroids[m, codes[n, m]].  Only the low 8 bits of an int64 code are read."""
    if centroids.dim() != 3 or centroids.shape[1] != K:
        raise ValueError("centroids must be [M, 256, dsub]")
    M, _, dsub = centroids.shape
    if codes.dim() != 2 or codes.shape[1] != M:
        raise ValueError("codes must be [n, M]")
    code_dtype = _code_dtype(codes)
    _need_cuda(codes, centroids)
    c = _centroids(centroids)
    codes = codes.contiguous()
    n = codes.shape[0]
    out = torch.empty((n, M * dsub), dtype=torch.float32, device=codes.device)
    if n == 0:
        return out
    lib, h, s, _ = _ctx(codes)
    _lib.check(lib.rc_pq_decode(h, _p(codes), code_dtype, _p(c), n, M, K, dsub, _p(out), s),
               "rc_pq_decode", h)
    return out


def decode_bwd_ws_bytes(n: int, M: int) -> int:
    """Workspace of the deterministic backward of `decode` (the row sort); needs no GPU."""
    return int(_lib.load().rc_pq_decode_bwd_det_ws_bytes(int(n), int(M)))


class _DecodeFn(torch.autograd.Function):
    """decode with the scatter-add gradient into the centroids (autograd of the gather at
    modeling_repconc.py:175): fp32 atomics, or — `deterministic` — the fixed-order fp64 sums of csrc/decode_det.hip."""

    @staticmethod
    def forward(ctx, codes, centroids, deterministic):
        ctx.save_for_backward(codes)
        ctx.cshape = tuple(centroids.shape)
        ctx.cdtype = centroids.dtype
        ctx.deterministic = bool(deterministic)
        return decode_raw(codes, centroids)

    @staticmethod
    def backward(ctx, grad_out):
        (codes,) = ctx.saved_tensors
        M, _, dsub = ctx.cshape
        go = grad_out.float().contiguous()
        codes = codes.contiguous()
        n = codes.shape[0]
        if n == 0:
            return None, torch.zeros(ctx.cshape, dtype=ctx.cdtype, device=go.device), None
        lib, h, s, _ = _ctx(go)
        if ctx.deterministic:
            gC = torch.empty(ctx.cshape, dtype=torch.float32, device=go.device)        # the entry overwrites
            wsb = lib.rc_pq_decode_bwd_det_ws_bytes(n, M)
            ws = torch.empty((wsb,), dtype=torch.uint8, device=go.device) if wsb else None
            _lib.check(lib.rc_pq_decode_bwd_det(h, _p(codes), _code_dtype(codes), _p(go), n, M, K, dsub, _p(gC), _p(ws), wsb, s),
                       "rc_pq_decode_bwd_det", h)
        else:
            gC = torch.zeros(ctx.cshape, dtype=torch.float32, device=go.device)
            _lib.check(lib.rc_pq_decode_bwd(h, _p(codes), _code_dtype(codes), _p(go), n, M, K, dsub, _p(gC), s),
                       "rc_pq_decode_bwd", h)
        return None, gC.to(ctx.cdtype), None


def decode(codes: torch.Tensor, centroids: torch.Tensor, deterministic: Optional[bool] = None) -> torch.Tensor:
    """decode_raw, differentiable w.r.t. the centroids.  deterministic selects the backward: False = fp32 atomics (the last
    bits depend on the arrival order), True = fixed-order fp64 sums (include/repconc_hip.h, rc_pq_decode_bwd_det: bit-identical
    from run to run), None = follow torch.are_deterministic_algorithms_enabled() as it stands at this call."""
    if centroids.requires_grad and torch.is_grad_enabled():
        det = torch.are_deterministic_algorithms_enabled() if deterministic is None else bool(deterministic)
        return _DecodeFn.apply(codes, centroids, det)
    return decode_raw(codes, centroids)


# --------------------------------------------------------------------------- JPQ scoring head
def jpq_head_ws_bytes(nq: int, k: int, M: int) -> int:
    """Workspace of the centroid gradient of `jpq_scores` (the pair sort); needs no GPU."""
    return int(_lib.load().rc_jpq_head_ws_bytes(int(nq), int(k), int(M)))


def _jpq_args(q: torch.Tensor, codes: torch.Tensor, pids: torch.Tensor, centroids: torch.Tensor):
    if centroids.dim() != 3 or centroids.shape[1] != K:
        raise ValueError("centroids must be [M, 256, dsub]")
    M, _, dsub = centroids.shape
    if q.dim() != 2 or q.shape[1] != M * dsub:
        raise ValueError(f"q must be [nq, M*dsub = {M}*{dsub}]: centroids must be [M, 256, D/M]")
    if codes.dim() != 2 or codes.shape[1] != M:
        raise ValueError("codes must be [N, M]")
    if codes.dtype != torch.uint8:
        raise ValueError("codes must be uint8 (the index's resident array)")
    if pids.dim() != 2 or pids.shape[0] != q.shape[0]:
        raise ValueError("pids must be [nq, k]")
    if pids.dtype != torch.int64:
        raise ValueError("pids must be int64")
    _need_cuda(q, codes, pids, centroids)
    if not codes.is_contiguous():
        raise ValueError("codes must be contiguous: the head reads the index's array in place")
    return M, dsub


class _JPQScoresFn(torch.autograd.Function):
    """scores[i, t] = <q[i], decode(codes[pids[i, t]])> without the decoded rows; both gradients in a fixed order
    (csrc/jpq_head.hip), so a step is bit-reproducible."""

    @staticmethod
    def forward(ctx, q, codes, pids, centroids):
        M, _, dsub = centroids.shape
        qc = q.detach().float().contiguous()
        pc = pids.contiguous()
        c = _centroids(centroids)
        nq, k = pc.shape
        ctx.save_for_backward(qc, codes, pc, c)
        ctx.qdtype, ctx.cdtype, ctx.cshape = q.dtype, centroids.dtype, tuple(centroids.shape)
        scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        if nq == 0 or k == 0:
            return scores
        lib, h, s, _ = _ctx(qc)
        _lib.check(lib.rc_jpq_head_fwd(h, _p(qc), _p(codes), codes.shape[0], _p(pc), _p(c), nq, k, M, K, dsub, _p(scores), s),
                   "rc_jpq_head_fwd", h)
        return scores

    @staticmethod
    def backward(ctx, grad_out):
        qc, codes, pc, c = ctx.saved_tensors
        M, _, dsub = ctx.cshape
        nq, k = pc.shape
        want_q, want_c = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
        gq = torch.empty_like(qc) if want_q else None
        gC = torch.empty(ctx.cshape, dtype=torch.float32, device=qc.device) if want_c else None
        if nq == 0 or k == 0:
            gq = None if gq is None else gq.zero_()
            gC = None if gC is None else gC.zero_()
        elif want_q or want_c:
            go = grad_out.float().contiguous()
            lib, h, s, _ = _ctx(qc)
            wsb = lib.rc_jpq_head_ws_bytes(nq, k, M) if want_c else 0
            ws = torch.empty((wsb,), dtype=torch.uint8, device=qc.device) if wsb else None
            _lib.check(lib.rc_jpq_head_bwd(h, _p(qc), _p(codes), codes.shape[0], _p(pc), _p(c), _p(go), nq, k, M, K, dsub,
                                           _p(gq), _p(gC), _p(ws), wsb, s), "rc_jpq_head_bwd", h)
        return (None if gq is None else gq.to(ctx.qdtype), None, None, None if gC is None else gC.to(ctx.cdtype))


def jpq_scores(q: torch.Tensor, codes: torch.Tensor, pids: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
    """[nq, k] fp32 scores of query i against the documents pids[i, :] of a PQ index: sum_m <q_m, centroids[m, codes[pid, m]]>.

    codes is the index's resident [N, M] uint8 array (read in place, never copied or widened); an id outside [0, N) — the
    -1 padding of a short search result — is a hole: score 0.0, no gradient.  Differentiable w.r.t. q and centroids; every
    sum runs in fp64 in a fixed order (include/repconc_hip.h, rc_jpq_head_*), so scores and gradients are bit-reproducible.
    Temperature stays outside: `jpq_scores(...) / temperature`."""
    _jpq_args(q, codes, pids, centroids)
    return _JPQScoresFn.apply(q, codes, pids, centroids)


# --------------------------------------------------------------------------- stage-1 contrastive loss
def contrastive_ws_bytes(nq: int, nd: int) -> int:
    """Workspace of `contrastive_loss` (duplicate flags, keep bits, per-row statistics); needs no GPU."""
    return int(_lib.load().rc_contrastive_ws_bytes(int(nq), int(nd)))


class _ContrastiveLossFn(torch.autograd.Function):
    """The fused in-batch loss on a similarity matrix and its gradient w.r.t. that matrix (csrc/contrastive.hip); the
    backward recomputes the logits from sim, the ids and the keep bits the forward left in the workspace."""

    @staticmethod
    def forward(ctx, sim, docids, rel_off, rel_ids, topk, return_logits):
        nq, nd = sim.shape
        simc = sim.detach().contiguous()
        lib, h, s, _ = _ctx(simc)
        wsb = lib.rc_contrastive_ws_bytes(nq, nd)
        if wsb == 0:
            raise ValueError(f"contrastive_loss needs 1 <= nq <= nd <= 262144 (got nq = {nq}, nd = {nd})")
        ws = torch.empty((wsb,), dtype=torch.uint8, device=simc.device)
        loss = torch.empty((), dtype=torch.float32, device=simc.device)
        z = torch.empty_like(simc) if return_logits else None
        R = rel_ids.numel()
        _lib.check(lib.rc_contrastive_fwd(h, _p(simc), _p(docids), _p(rel_off), _p(rel_ids) if R else _p(None), R, nq, nd, topk,
                                          _p(loss), _p(z), _p(ws), wsb, s), "rc_contrastive_fwd", h)
        ctx.save_for_backward(simc, docids, rel_off, rel_ids, ws)
        ctx.topk = topk
        if return_logits:
            ctx.mark_non_differentiable(z)
            return loss, z
        return loss

    @staticmethod
    def backward(ctx, grad_loss, *_unused):
        simc, docids, rel_off, rel_ids, ws = ctx.saved_tensors
        nq, nd = simc.shape
        go = grad_loss.detach().float().contiguous()
        grad = torch.empty_like(simc)
        lib, h, s, _ = _ctx(simc)
        R = rel_ids.numel()
        _lib.check(lib.rc_contrastive_bwd(h, _p(simc), _p(docids), _p(rel_off), _p(rel_ids) if R else _p(None), R, nq, nd, ctx.topk,
                                          _p(go), _p(grad), _p(ws), ws.numel(), s), "rc_contrastive_bwd", h)
        return grad, None, None, None, None, None


def contrastive_loss(sim: torch.Tensor, docids: torch.Tensor, rel_off: torch.Tensor, rel_ids: torch.Tensor, topk: int = 0,
                     return_logits: bool = False):
    """Stage 1's in-batch softmax loss on sim [nq, nd] fp32 (label of row i = column i), differentiable w.r.t. sim.

    docids [nd] int64; the positives of query i are rel_ids[rel_off[i]:rel_off[i + 1]] (int64 CSR, rows may be empty).  A column
    is masked (-10000) when its docid repeats an earlier column's or is a positive of the row, the diagonal excepted; topk > 0
    keeps the topk largest remaining negatives of a row plus its label and pushes the rest down by another 10000 (the reference's
    dynamic_topk_hard_negative).  Masks, cut, log-softmax and gradient are one pass of HIP kernels after the caller's GEMM, in a
    fixed order (include/repconc_hip.h, rc_contrastive_*): bit-reproducible, no [nd, nd] or [nq, nd] mask is ever allocated.
    return_logits: also return the fp32 logits z [nq, nd] (not differentiable; a test hook)."""
    _need_cuda(sim, docids, rel_off, rel_ids)
    if sim.dim() != 2 or docids.dim() != 1 or rel_off.dim() != 1 or rel_ids.dim() != 1:
        raise ValueError("expected sim [nq, nd], docids [nd], rel_off [nq + 1], rel_ids [R]")
    nq, nd = sim.shape
    if any(t.device != sim.device for t in (docids, rel_off, rel_ids)):
        raise ValueError(f"docids, rel_off and rel_ids must be on sim's device ({sim.device}): the kernels run there")
    if sim.dtype != torch.float32:
        raise ValueError("sim must be float32 (take .float() of an autocast GEMM's output)")
    if docids.dtype != torch.int64 or rel_off.dtype != torch.int64 or rel_ids.dtype != torch.int64:
        raise ValueError("docids, rel_off and rel_ids must be int64")
    if docids.shape[0] != nd or rel_off.shape[0] != nq + 1:
        raise ValueError(f"docids must hold nd = {nd} ids and rel_off nq + 1 = {nq + 1} offsets")
    topk = int(topk)
    if not 0 <= topk <= nd:
        raise ValueError(f"topk must be in [0, nd = {nd}]")
    return _ContrastiveLossFn.apply(sim, docids.contiguous(), rel_off.contiguous(), rel_ids.contiguous(), topk, bool(return_logits))


# --------------------------------------------------------------------------- small ops
def normalize_centroids_(centroids: torch.Tensor) -> torch.Tensor:
    _need_cuda(centroids)
    if centroids.dtype != torch.float32 or not centroids.is_contiguous():
        raise ValueError("centroids must be contiguous fp32")
    M, Kc, dsub = centroids.shape
    lib, h, s, _ = _ctx(centroids)
    _lib.check(lib.rc_normalize_centroids(h, _p(centroids), M, Kc, dsub, s), "rc_normalize_centroids", h)
    return centroids


def code_hist(codes: torch.Tensor) -> torch.Tensor:
    """hist [M, 256] int32.  finetune_repconc.py:588-592 for every sub-quantiser."""
    if codes.dim() != 2 or codes.shape[1] < 1:
        raise ValueError("codes must be [n, M]")
    code_dtype = _code_dtype(codes)
    _need_cuda(codes)
    codes = codes.contiguous()
    n, M = codes.shape
    if n == 0:
        return torch.zeros((M, K), dtype=torch.int32, device=codes.device)
    hist = torch.empty((M, K), dtype=torch.int32, device=codes.device)
    lib, h, s, _ = _ctx(codes)
    _lib.check(lib.rc_code_hist(h, _p(codes), code_dtype, n, M, K, _p(hist), s), "rc_code_hist", h)
    return hist


def _stats_buffers(sums: Optional[torch.Tensor], counts: Optional[torch.Tensor], cshape) -> None:
    """The kernels read sums as fp64 [M, K, dsub] and counts as int64 [M, K] through raw pointers: anything else is an
    out-of-bounds read, not a conversion."""
    M, Kc, dsub = cshape
    if sums is not None and (sums.dtype != torch.float64 or tuple(sums.shape) != (M, Kc, dsub) or not sums.is_contiguous()):
        raise ValueError(f"sums must be contiguous fp64 [{M}, {Kc}, {dsub}]")
    if counts is not None and (counts.dtype != torch.int64 or tuple(counts.shape) != (M, Kc) or not counts.is_contiguous()):
        raise ValueError(f"counts must be contiguous int64 [{M}, {Kc}]")


def kmeans_stats(x: torch.Tensor, codes: torch.Tensor, sums: Optional[torch.Tensor] = None,
                 counts: Optional[torch.Tensor] = None):
    """Accumulate Lloyd sufficient statistics (sums [M,K,dsub] fp64, counts [M,K] int64)."""
    if x.dim() != 2 or codes.dim() != 2 or codes.shape[1] < 1:
        raise ValueError("expected x [n, D] and codes [n, M]")
    n, D = x.shape
    M = codes.shape[1]
    if codes.shape[0] != n:
        raise ValueError(f"codes has {codes.shape[0]} rows, x has {n}")
    if D % M != 0:
        raise ValueError(f"embedding width {D} is not a multiple of M = {M}")
    dsub = D // M
    _stats_buffers(sums, counts, (M, K, dsub))
    _need_cuda(x, codes, sums, counts)
    x = _rows_f32(x)
    if codes.dtype != torch.uint8:
        codes = codes.to(torch.uint8)
    codes = codes.contiguous()
    if sums is None:
        sums = torch.zeros((M, K, dsub), dtype=torch.float64, device=x.device)
    if counts is None:
        counts = torch.zeros((M, K), dtype=torch.int64, device=x.device)
    if n == 0:
        return sums, counts
    lib, h, s, _ = _ctx(x)
    _lib.check(lib.rc_kmeans_stats(h, _p(x), x.stride(0), _p(codes), n, D, M, K, _p(sums), _p(counts), s),
               "rc_kmeans_stats", h)
    return sums, counts


def kmeans_update_(sums: torch.Tensor, counts: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
    """centroids[m, k] <- fp32(sums[m, k] / counts[m, k]) where counts[m, k] > 0, unchanged otherwise; in place."""
    if centroids.dim() != 3 or centroids.shape[1] != K:
        raise ValueError("centroids must be [M, 256, dsub]")
    if centroids.dtype != torch.float32 or not centroids.is_contiguous():
        raise ValueError("centroids must be contiguous fp32")
    if sums is None or counts is None:
        raise ValueError("sums and counts are required")
    _stats_buffers(sums, counts, tuple(centroids.shape))
    _need_cuda(sums, counts, centroids)
    M, Kc, dsub = centroids.shape
    lib, h, s, _ = _ctx(centroids)
    _lib.check(lib.rc_kmeans_update(h, _p(sums), _p(counts), _p(centroids), M, Kc, dsub, s), "rc_kmeans_update", h)
    return centroids


def kmeans_split_empty_(centroids: torch.Tensor, counts: torch.Tensor, nsplit: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Faiss's empty-cluster rule (`split_clusters`) applied in place on the device; see include/repconc_hip.h."""
    _need_cuda(centroids, counts, nsplit)
    if centroids.dtype != torch.float32 or not centroids.is_contiguous() or counts.dtype != torch.int64 or not counts.is_contiguous():
        raise ValueError("centroids must be contiguous fp32 [M,256,dsub], counts contiguous int64 [M,256]")
    M, Kc, dsub = centroids.shape
    lib, h, s, _ = _ctx(centroids)
    _lib.check(lib.rc_kmeans_split_empty(h, _p(centroids), _p(counts), M, Kc, dsub, _p(nsplit), s), "rc_kmeans_split_empty", h)
    return centroids


# --------------------------------------------------------------------------- ADC search
METRIC_INNER_PRODUCT, METRIC_L2 = 0, 1      # faiss.METRIC_INNER_PRODUCT / faiss.METRIC_L2 (re-exported by repconc_amd.index)


def _adc_metric(metric) -> bool:
    """True for the L2 metric; anything but the two Faiss values is an error."""
    if metric not in (METRIC_INNER_PRODUCT, METRIC_L2):
        raise ValueError(f"metric must be METRIC_INNER_PRODUCT (0) or METRIC_L2 (1), not {metric!r}")
    return metric == METRIC_L2


def adc_lut(centroids: torch.Tensor, q: torch.Tensor, metric: int = METRIC_INNER_PRODUCT) -> torch.Tensor:
    """The per-query tables [nq, M, 256] every ADC search scores with.  Inner product: <q_m, C[m][c]>.  METRIC_L2: S = 0.0f - T with
    T[m][c] = the fp32 chain of (q_j - c_j)^2, j ascending — the searches run on s = -d, and no entry is -0.0f (rc_adc_lut_l2)."""
    l2 = _adc_metric(metric)
    _need_cuda(centroids, q)
    c, q = _centroids(centroids), _rows_f32(q).contiguous()
    M, _, dsub = c.shape
    nq, D = q.shape
    lut = torch.empty((nq, M, K), dtype=torch.float32, device=q.device)
    lib, h, s, _ = _ctx(q)
    fn, name = (lib.rc_adc_lut_l2, "rc_adc_lut_l2") if l2 else (lib.rc_adc_lut, "rc_adc_lut")
    _lib.check(fn(h, _p(c), _p(q), nq, D, M, K, _p(lut), s), name, h)
    return lut


def adc_image_row_bytes(M: int) -> int:
    """Bytes per row of the permuted code image the ADC screen of this M streams (rc_adc_scan_image); 0 = none."""
    return int(_lib.load().rc_adc_scan_image_bytes(1 << 20, int(M))) >> 20


def adc_image_bytes(N: int, M: int) -> int:
    """Bytes of the FLAT-SEARCH image of an N-row index (rc_adc_scan_image_bytes): N * row bytes, rounded up to whole
    storage tiles for the M whose image is tile-blocked (M = 96: 32768-row tiles, phase-major inside a tile)."""
    return int(_lib.load().rc_adc_scan_image_bytes(int(N), int(M)))


def adc_image_supported(M: int) -> bool:
    return adc_image_row_bytes(M) > 0


def adc_image_rows_bytes(N: int, M: int) -> int:
    """Bytes of the IVF search's image (layout "rows") of an N-row index: whole chunks of 16 rows."""
    return int(_lib.load().rc_adc_scan_image_rows_bytes(int(N), int(M)))


def adc_image_rows_at(M: int, n: int, m: int) -> int:
    """Byte offset of codes[n][m] in the IVF search's image (host-side description, no GPU involved)."""
    return int(_lib.load().rc_adc_scan_image_rows_at(int(M), int(n), int(m)))


def adc_image_rows16_at(M: int, n: int, m: int) -> int:
    """Byte offset of codes[n][m] in the image of the 16-query IVF screen (layout "rows16"; host-side description)."""
    return int(_lib.load().rc_adc_scan_image_rows16_at(int(M), int(n), int(m)))


def adc_scan_image_(codes: torch.Tensor, image: torch.Tensor, n0: int = 0, n: Optional[int] = None,
                    layout: str = "flat") -> torch.Tensor:
    """(Re)build rows [n0, n0+n) of the permuted code image of an index: codes uint8 [>=n0+n, M] contiguous; image a
    contiguous uint8 buffer of at least adc_image_bytes(n0+n, M) bytes (layout "flat": what `adc_search` takes — row-major
    for M in {16,32,48,64}, tile-blocked for M = 96) or adc_image_rows_bytes(n0+n, M) bytes (layout "rows": what the
    list-centric IVF search takes, blocked by chunks of 16 rows; `adc_image_rows_at(M, n, m)` is the byte offset of
    codes[n][m] in it; layout "rows16": the image of its 16-query screen, same size, `adc_image_rows16_at`).  See include/repconc_hip.h rc_adc_scan_image."""
    _need_cuda(codes, image)
    if codes.dtype != torch.uint8 or image.dtype != torch.uint8 or not codes.is_contiguous() or not image.is_contiguous():
        raise ValueError("codes and image must be contiguous uint8")
    if layout not in ("flat", "rows", "rows16"):
        raise ValueError("layout must be flat|rows|rows16")
    M = codes.shape[1]
    if n is None:
        n = codes.shape[0] - n0
    need = adc_image_bytes(n0 + n, M) if layout == "flat" else adc_image_rows_bytes(n0 + n, M)   # rows16: the same size as rows
    if n0 < 0 or n < 0 or n0 + n > codes.shape[0] or adc_image_row_bytes(M) == 0 or image.numel() < need:
        raise ValueError("row range outside the code / image buffers")
    lib, h, s, _ = _ctx(codes)
    fn = {"flat": lib.rc_adc_scan_image, "rows": lib.rc_adc_scan_image_rows, "rows16": lib.rc_adc_scan_image_rows16}[layout]
    _lib.check(fn(h, _p(codes), int(n0), int(n), M, _p(image), s), "rc_adc_scan_image", h)
    return image


SEARCH_SCREEN_M = frozenset((8, 12, 16, 24, 32, 48, 64, 96))      # widths of the screened flat search: the M of ADC_SEARCH_WIDTHS (csrc/adc_common.h)
# Default head-room of the sampled candidate threshold: the threshold is the r-th best score of the 32 768-row sample,
# r = floor(mu + slack sqrt(mu + 1) + 4) + 1 with mu = k S / N expected top-k rows in the sample (rc_adc_search_q).  A query whose
# sample holds MORE than r - 1 of the true top-k keeps too few candidates and is repeated alone (~1 ms, PendingSearch).  Round 6:
# 6 -> 3.  At k = 1000 over 8.84 M rows (mu = 3.7, r = 22 -> 15) the chance of that is 8e-6 per query instead of 1e-10 — one repeated
# query per ~100 batches of 1200 — and the screen keeps 6.3 k rows per query instead of 8.7 k, the rescoring 4.0 k instead of 5.7 k:
# 147.4 -> 154.2 k queries/s; slack 2 (1e-4 per query: 3 of 28 800 repeated) is not faster (profiles/r06m_adc_slack.txt).
ADC_SEL_SLACK = 3.0
_warned_slow_m = set()


class PendingSearch:
    """A search that has been enqueued but whose status word has not been read yet (`adc_search(..., defer=True)`).
    `result()` synchronises and reads the status.  In the rare case that the sampled threshold admitted too few or too
    many candidates for SOME queries, only those queries are repeated with an adjusted slack (the others' results stand),
    and queries that still fail after `max_retries` repetitions are answered by the exact path (`adc_search_exact`),
    which terminates for any index content — like Faiss's `index.search` (evaluate_repconc.py:180-185) this never raises
    on degenerate data (thousands of identical codes, all rows tied).  Lets a caller enqueue every query batch before the
    first host synchronisation."""

    def __init__(self, rerun, scores, ids, status, qstatus, slack, max_retries, stream=None, metric: int = 0,
                 rows: Optional[torch.Tensor] = None, id_offset: int = 0):
        self._rerun, self._scores, self._ids, self._status, self._qstatus = rerun, scores, ids, status, qstatus
        self._slack, self._left, self._done = slack, max_retries, status is None
        self._stream = stream
        # a subset search (`adc_search(rows=...)`): every entry ran over the selection with id_offset 0, so `ids` are positions in
        # `rows`; `result` turns them into id_offset + rows[.] ONCE, after the repeated and exact-route queries have been merged in
        self._rows, self._id_offset = rows, int(id_offset)
        # the metric of `scores` (ADC searches: METRIC_INNER_PRODUCT / METRIC_L2).  `rerun` repeats and hands over to the exact
        # route under the same one, and each of those entries returns the metric's final values: rows are only ever copied here
        self.metric = metric
        self.stats = {"retried_queries": 0, "exact_queries": 0}

    def result(self):
        if self._done and self._rows is None:
            return self._scores, self._ids
        # retries run on the stream the search was enqueued on, whatever stream is current when result() is called
        with torch.cuda.stream(self._stream) if self._stream is not None else _nullcontext():
            if not self._done and int(self._status.item()) != 0:
                bad = torch.nonzero(self._qstatus).flatten()
                bits = self._qstatus[bad]
                slack_few, slack_many = self._slack, self._slack
                while bad.numel() and self._left > 0:
                    self._left -= 1
                    self.stats["retried_queries"] += int(bad.numel())
                    slack_few = max(slack_few, 0.0) * 3.0 + 2.0          # bit0: too few candidates -> wider
                    slack_many = max(slack_many / 3.0, 0.0)              # bit1 without bit0: a list overflowed -> tighter
                    still, still_bits = [], []
                    # bit2 (dense fp16 search: the threshold is too close to the k-th score to certify) wants a lower threshold
                    # like bit0, unless the list overflowed as well
                    few = ((bits & 1) != 0) | ((bits & 6) == 4)
                    for sel, slack in ((few, slack_few), (~few, slack_many)):
                        idx = bad[sel]
                        if idx.numel() == 0:
                            continue
                        s, i, qs = self._rerun(idx, slack, False)
                        ok = qs == 0
                        self._scores[idx[ok]] = s[ok]
                        self._ids[idx[ok]] = i[ok]
                        still.append(idx[~ok])
                        still_bits.append(qs[~ok])
                    bad, bits = torch.cat(still), torch.cat(still_bits)
                if bad.numel():
                    self.stats["exact_queries"] = int(bad.numel())
                    s, i, _ = self._rerun(bad, 0.0, True)
                    self._scores[bad] = s
                    self._ids[bad] = i
            if self._rows is not None:
                _map_ids_(self._ids, self._rows, self._id_offset)
        self._done = True
        self._rerun = self._rows = None
        return self._scores, self._ids


_retry_ops_warm = set()


def _warm_retry_ops(dev):
    """The torch operators of the retry path (`PendingSearch.result`, `rerun`: nonzero, mask / index selection, index_put,
    cat) once per device, on eight elements.  A framework operator's first use on a device loads its code object — measured: the
    FIRST repeated query of a process cost 300 ms, every later one ~1 ms (profiles/r06m_adc_retry_cost.txt).  With the threshold's
    head-room at 3 standard deviations a 6 980-query evaluation repeats a query with a probability of 5 %: that load belongs to
    the first search of the process, not to a random batch in the middle of an evaluation."""
    key = (dev.type, dev.index)
    if key in _retry_ops_warm:
        return
    _retry_ops_warm.add(key)
    qs = torch.tensor([0, 1, 0, 2, 0, 0, 1, 0], dtype=torch.int32, device=dev)
    sc = torch.zeros((8, 4), dtype=torch.float32, device=dev)
    ii = torch.zeros((8, 4), dtype=torch.int64, device=dev)
    bad = torch.nonzero(qs).flatten()
    bits = qs[bad]
    for sel in ((bits & 1) != 0, (bits & 1) == 0):
        idx = bad[sel]
        part = sc[idx].contiguous()
        ok = qs[idx] == 1
        sc[idx[ok]] = part[ok]
        ii[idx[ok]] = ii[idx][ok]
        torch.cat([idx[~ok], idx[ok]])
    torch.cat([bad, bad])


class _nullcontext:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


ADC_IMAGE_LAYOUTS = {"flat": 0, "rows": 1, "rows16": 2}        # rc_adc_select_rows' `layout`; the three of `adc_scan_image_`


def _map_ids_(ids: torch.Tensor, rows: torch.Tensor, id_offset: int = 0) -> torch.Tensor:
    """ids[i] <- id_offset + rows[ids[i]] where ids[i] >= 0, in place (rc_map_ids): the end of a search over a selection."""
    if ids.numel() == 0 or rows.numel() == 0:
        return ids
    _need_cuda(ids, rows)
    if ids.dtype != torch.int64 or not ids.is_contiguous() or rows.dtype != torch.int64 or not rows.is_contiguous():
        raise ValueError("ids and rows must be contiguous int64")
    lib, h, s, _ = _ctx(ids)
    _lib.check(lib.rc_map_ids(h, _p(ids), ids.numel(), _p(rows), int(id_offset), s), "rc_map_ids", h)
    return ids


def adc_select_rows(codes: torch.Tensor, rows: torch.Tensor, layout: str = "flat", check_rows: bool = True):
    """The SELECTION a subset search scans in place of the index: (sel_codes uint8 [ns, M] = codes[rows], sel_image = their
    permuted image in `layout` — flat | rows | rows16, the buffers `adc_scan_image_` fills — or None for an M without one), from
    one kernel (rc_adc_select_rows).  rows: int64 [ns] on the device of `codes`, contiguous, strictly ascending, in [0, N);
    check_rows (one host read) verifies that, as `dense_search(rows=...)` does: everything refused is a ValueError before any
    library call."""
    if layout not in ADC_IMAGE_LAYOUTS:
        raise ValueError("layout must be flat|rows|rows16")
    if not isinstance(codes, torch.Tensor) or codes.dim() != 2 or codes.dtype != torch.uint8 or not codes.is_contiguous():
        raise ValueError("adc_select_rows: index codes must be contiguous uint8 [N, M]")
    rows = _dense_rows("adc_select_rows", rows, codes, check_rows)
    _need_cuda(codes, rows)
    N, M = codes.shape
    ns = rows.numel()
    imaged = adc_image_supported(M)
    if imaged and codes.data_ptr() % 16 != 0:               # a view at an odd byte offset: the kernel loads 16 bytes at a time
        codes = codes.clone()
    sel_codes = torch.empty((ns, M), dtype=torch.uint8, device=codes.device)
    sel_image = None
    if imaged:
        nbytes = adc_image_bytes(ns, M) if layout == "flat" else adc_image_rows_bytes(ns, M)
        sel_image = torch.empty((nbytes,), dtype=torch.uint8, device=codes.device)
    if ns:
        lib, h, s, _ = _ctx(codes)
        _lib.check(lib.rc_adc_select_rows(h, _p(codes), N, M, _p(rows), ns, ADC_IMAGE_LAYOUTS[layout], _p(sel_codes),
                                          _p(sel_image), s), "rc_adc_select_rows", h)
    return sel_codes, sel_image


def _adc_rows(name: str, rows, codes: torch.Tensor, check_rows: bool) -> torch.Tensor:
    """`rows` of a search over a selection: codes are the SELECTION's [ns, M], so rows is int64 [ns] on their device, contiguous,
    and (check_rows) non-negative and strictly ascending — refused with a ValueError before anything reaches the library."""
    if not isinstance(rows, torch.Tensor) or rows.dim() != 1:
        raise ValueError(f"{name}: rows must be a 1-d tensor of row numbers")
    if rows.dtype != torch.int64:
        raise ValueError(f"{name}: rows must be int64, got {rows.dtype}")
    if rows.device != codes.device:
        raise ValueError(f"{name}: rows must be on the device of the codes ({codes.device}), got {rows.device}")
    if not rows.is_contiguous():
        raise ValueError(f"{name}: rows must be contiguous")
    if codes.dim() != 2 or rows.numel() != codes.shape[0]:
        raise ValueError(f"{name}: {rows.numel()} rows for the {tuple(codes.shape)} codes of a selection (adc_select_rows)")
    if check_rows and rows.numel():
        ok = rows[0] >= 0
        if rows.numel() > 1:
            ok = ok & (rows[1:] > rows[:-1]).all()
        if not bool(ok):
            raise ValueError(f"{name}: rows must be strictly ascending row numbers >= 0")
    return rows


def adc_search_exact(codes: torch.Tensor, centroids: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0,
                     metric: int = METRIC_INNER_PRODUCT, *, rows: Optional[torch.Tensor] = None, check_rows: bool = True):
    """The same answer as `adc_search` by the path that cannot fail (rc_adc_search_exact / rc_adc_search_l2_exact): exact scores
    of every row and a radix select of the min(k, N) best keys.  For the queries the sampled-threshold path gives up on, and a
    slow but independent cross-check in the tests.  rows: as in `adc_search`."""
    l2 = _adc_metric(metric)
    if rows is not None:
        rows = _adc_rows("adc_search_exact", rows, codes, check_rows)
        scores, ids = adc_search_exact(codes, centroids, q, k, 0, metric)
        return scores, _map_ids_(ids, rows, id_offset)
    _need_cuda(codes, centroids, q)
    if codes.dtype != torch.uint8 or not codes.is_contiguous():
        raise ValueError("index codes must be contiguous uint8 [N, M]")
    c, q = _centroids(centroids), _rows_f32(q).contiguous()
    N, M = codes.shape
    nq, D = q.shape
    lib, h, s, _ = _ctx(q)
    scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    if nq == 0 or N == 0:
        scores.fill_(float("inf") if l2 else float("-inf"))
        ids.fill_(-1)
        return scores, ids
    wsb = lib.rc_adc_search_exact_ws_bytes(N, M, K, nq, k)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=q.device)
    fn, name = (lib.rc_adc_search_l2_exact, "rc_adc_search_l2_exact") if l2 else (lib.rc_adc_search_exact, "rc_adc_search_exact")
    _lib.check(fn(h, _p(codes), N, M, K, _p(c), D, _p(q), nq, int(k), int(id_offset), _p(scores), _p(ids), _p(ws), wsb, s), name, h)
    return scores, ids


def adc_search(codes: torch.Tensor, centroids: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0,
               sel_slack: Optional[float] = None, max_retries: int = 2, scan_image: Optional[torch.Tensor] = None,
               defer: bool = False, stats: Optional[dict] = None, metric: int = METRIC_INNER_PRODUCT, *,
               rows: Optional[torch.Tensor] = None, check_rows: bool = True):
    """Top-k ADC search of `q` [nq,D] against uint8 `codes` [N,M].
    Returns (scores [nq,k] fp32, ids [nq,k] int64), sorted (score desc, id asc).
    evaluate_repconc.py:180-185 / finetune_jpq.py:176.
    metric: METRIC_INNER_PRODUCT, or METRIC_L2 — then the first array holds squared distances (the fp32 sum over m ascending of
    the sub-distances, `adc_lut`), sorted (distance asc, id asc), +0.0f for a zero, +inf / -1 past N.  The library entries of the
    metric (rc_adc_search_l2_q / rc_adc_search_l2_exact) return distances themselves, and every path of `PendingSearch` — first
    pass, per-query repeat, exact route — ends in exactly one of them per query: nothing is negated here.
    scan_image: the index's permuted code image (adc_scan_image_), kept by PQIndex; None = rebuilt per call.
    defer: return a `PendingSearch` instead (no host synchronisation here; `.result()` gives the pair).
    stats (measurement): receives "survivors" / "candidates" = int32 [nq] device tensors, the rows of every query that passed
    the 8-bit screen / that the exact rescoring kept in the FIRST pass (rc_adc_search_ws_counts).
    rows (subset search): int64 [N] ascending — `codes` / `scan_image` are then a SELECTION (`adc_select_rows(store, rows)`), the
    search is the one of an index that holds just them, run with id_offset 0, and every id i >= 0 comes back as id_offset + rows[i]
    (`PendingSearch` maps once, at the end); check_rows: one host read, off for a list that is valid by construction.
    Never raises on degenerate index content: see `PendingSearch`."""
    l2 = _adc_metric(metric)
    if rows is not None:
        rows = _adc_rows("adc_search", rows, codes, check_rows)
    _need_cuda(codes, centroids, q, scan_image)
    caller_offset, id_offset = id_offset, (0 if rows is not None else id_offset)       # what the entries see
    sub = dict(rows=rows, id_offset=caller_offset)
    if sel_slack is None:
        sel_slack = ADC_SEL_SLACK
    if codes.dtype != torch.uint8 or not codes.is_contiguous():
        raise ValueError("index codes must be contiguous uint8 [N, M]")
    if scan_image is not None and (scan_image.dtype != torch.uint8 or not scan_image.is_contiguous()
                                   or adc_image_row_bytes(codes.shape[1]) == 0
                                   or scan_image.numel() < adc_image_bytes(codes.shape[0], codes.shape[1])):
        raise ValueError("scan_image must be a contiguous uint8 buffer of >= adc_image_bytes(N, M) bytes (adc_scan_image_)")
    c, q = _centroids(centroids), _rows_f32(q).contiguous()
    N, M = codes.shape
    nq, D = q.shape
    if D != M * c.shape[2]:
        raise ValueError("query width does not match the centroid table")
    lib, h, s, dev = _ctx(q)
    if M not in SEARCH_SCREEN_M and nq and N:
        # a width without a screening kernel (the reference's IndexPQ takes any M, evaluate_repconc.py:81): the exact scan with a
        # run-time width answers — correct and complete, an order of magnitude slower than the screened search
        global _warned_slow_m
        if M not in _warned_slow_m:
            _warned_slow_m.add(M)
            import logging
            logging.getLogger(__name__).warning("adc_search: MCQ_M = %d has no screening kernel (%s have); using the exact scan",
                                                M, sorted(SEARCH_SCREEN_M))
        got = adc_search_exact(codes, c, q, k, id_offset, metric)
        pending = PendingSearch(None, got[0], got[1], None, None, 0.0, 0, metric=metric, **sub)
        return pending if defer else pending.result()
    scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    if nq == 0 or N == 0:
        if nq and N == 0:
            scores.fill_(float("inf") if l2 else float("-inf"))
            ids.fill_(-1)
        pending = PendingSearch(None, scores, ids, None, None, 0.0, 0, metric=metric)     # nothing to map: no id >= 0
        return pending if defer else pending.result()
    ws_fn = lib.rc_adc_search_img_ws_bytes if scan_image is not None else lib.rc_adc_search_ws_bytes
    search_fn, search_name = (lib.rc_adc_search_l2_q, "rc_adc_search_l2_q") if l2 else (lib.rc_adc_search_q, "rc_adc_search_q")

    def launch(qq, slack, out_s, out_i):
        # the workspace is released when this returns: the caching allocator hands it out again in stream order only
        n = qq.shape[0]
        wsb = ws_fn(N, M, K, n, k)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=q.device)
        status = torch.zeros((1,), dtype=torch.int32, device=q.device)
        qstatus = torch.zeros((n,), dtype=torch.int32, device=q.device)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(search_fn(h, _p(codes), _p(scan_image), N, M, K, _p(c), D, _p(qq), n, int(k), int(id_offset),
                             float(slack), _p(out_s), _p(out_i), _p(status), _p(qstatus), _p(ws), wsb, st), search_name, h)
        if stats is not None and "candidates" not in stats:
            so, co = C.c_size_t(0), C.c_size_t(0)
            _lib.check(lib.rc_adc_search_ws_counts(N, M, K, n, C.byref(so), C.byref(co)), "rc_adc_search_ws_counts", h)
            if so.value:
                stats["survivors"] = ws[so.value:so.value + 4 * n].view(torch.int32).clone()
            stats["candidates"] = ws[co.value:co.value + 4 * n].view(torch.int32).clone()
        return status, qstatus

    def rerun(idx, slack, exact):
        qq = q[idx].contiguous()
        if exact:
            s_, i_ = adc_search_exact(codes, c, qq, k, id_offset, metric)
            return s_, i_, None
        s_ = torch.empty((qq.shape[0], k), dtype=torch.float32, device=q.device)
        i_ = torch.empty((qq.shape[0], k), dtype=torch.int64, device=q.device)
        _, qs = launch(qq, slack, s_, i_)
        return s_, i_, qs

    _warm_retry_ops(q.device)
    status, qstatus = launch(q, float(sel_slack), scores, ids)
    pending = PendingSearch(rerun, scores, ids, status, qstatus, float(sel_slack), max_retries,
                            stream=torch.cuda.current_stream(dev), metric=metric, **sub)
    return pending if defer else pending.result()


# ---------------------------------------------------------------------------------------------------------------- dense
DENSE_SEL_SLACK = ADC_SEL_SLACK     # head-room of the dense search's sampled threshold (same rank formula, rc_dense_search_q)
DENSE_MAX_K = 8192                  # the select's cap (ADC_CAND_CAP / 2, csrc/topk.h)
DENSE_EXACT_MAX_N = 131072          # up to here every dense search takes the exact route (csrc/dense_gemm.h)
DENSE_QCHUNK = 2048                 # queries per library call: <= 2048 x 256 KiB of sample scores and candidate keys
DENSE_SQ8_MAX_D = 65536             # widest row of the int8 search (DENSE_I8_MAX_D, csrc/dense_i8_gemm.h)


def _dense_args(x: torch.Tensor, q: torch.Tensor, k: int):
    _need_cuda(x, q)
    if x.dim() != 2 or q.dim() != 2 or x.shape[1] != q.shape[1]:
        raise ValueError("dense search: x [N, D] and q [nq, D] with the same D")
    if not 1 <= int(k) <= DENSE_MAX_K:
        raise ValueError(f"dense search: k must be in [1, {DENSE_MAX_K}]")
    if x.dtype != torch.float32 or x.stride(1) != 1 or x.stride(0) % 4 != 0 or x.data_ptr() % 16 != 0:
        x = x.float().contiguous()
    if x.shape[0] >= 1 << 32:
        raise ValueError("dense search: N must be < 2^32")
    q = q.to(x.device, torch.float32).contiguous()
    return x, q


def _dense_f16_args(x16: torch.Tensor, q: torch.Tensor, k: int):
    _need_cuda(x16, q)
    if x16.dim() != 2 or q.dim() != 2 or x16.shape[1] != q.shape[1]:
        raise ValueError("dense search: x [N, D] and q [nq, D] with the same D")
    if x16.dtype != torch.float16:
        raise ValueError("dense_search_f16: the corpus must be float16 (FlatIPIndex(storage='float16') rounds and checks it)")
    if not 1 <= int(k) <= DENSE_MAX_K:
        raise ValueError(f"dense search: k must be in [1, {DENSE_MAX_K}]")
    if x16.stride(1) != 1 or (x16.shape[1] % 16 == 0 and (x16.stride(0) % 8 != 0 or x16.data_ptr() % 16 != 0)):
        x16 = x16.clone(memory_format=torch.contiguous_format)      # a strided or misaligned view: a fresh allocation is aligned
    if x16.shape[0] >= 1 << 32:
        raise ValueError("dense search: N must be < 2^32")
    q16 = q.to(x16.device).to(torch.float16).contiguous()           # round to nearest even, as the corpus was
    return x16, q16


def _dense_sq8_args(x8: torch.Tensor, q: torch.Tensor, k: int):
    if x8.dim() != 2 or q.dim() != 2 or x8.shape[1] != q.shape[1]:
        raise ValueError("dense search: x [N, D] and q [nq, D] with the same D")
    if x8.dtype != torch.int8:
        raise ValueError("dense_search_sq8: the corpus must be int8 codes, c - 128 (FlatSQ8Index encodes them)")
    if not 1 <= int(k) <= DENSE_MAX_K:
        raise ValueError(f"dense search: k must be in [1, {DENSE_MAX_K}]")
    if x8.shape[1] > DENSE_SQ8_MAX_D:
        raise ValueError(f"dense_search_sq8: D must be <= {DENSE_SQ8_MAX_D} (the screen's int32 accumulators)")
    _need_cuda(x8, q)
    if x8.stride(1) != 1 or (x8.shape[0] > 1 and x8.stride(0) < x8.shape[1]):
        x8 = x8.contiguous()
    if x8.shape[0] >= 1 << 32:
        raise ValueError("dense search: N must be < 2^32")
    return x8, q.to(x8.device, torch.float32).contiguous()


# One dense search in eight variants.  args: (x, q, k) -> the checked corpus and the queries in the storage type; entry: the
# library's rc_<entry>_search_q / rc_<entry>_search_ws_bytes / rc_<entry>_scores; exact: rc_<exact>_search_exact / ..._ws_bytes,
# the route that cannot fail; side / exact_side: the side operands those two entries take after the queries, by name and in the
# header's order (xnorm_max [1]: the screen only approximates the score, the answer carries a certificate; xsq [N]: the squared
# norm of every row; dec [2, D] and cstat [2]: the decoding vectors and the statistics of int8 codes); pad: the value of the
# slots past N; scores_ws: rc_<entry>_scores takes a workspace.
_DenseVariant = collections.namedtuple("_DenseVariant", "args entry exact side exact_side pad scores_ws",
                                       defaults=((), (), float("-inf"), False))
_DENSE_F32 = _DenseVariant(_dense_args, "dense", "dense")
_DENSE_F16 = _DenseVariant(_dense_f16_args, "dense_f16", "dense_f16", ("xnorm_max",))
_DENSE_BF16X3 = _DenseVariant(_dense_args, "dense_bf16x3", "dense", ("xnorm_max",), scores_ws=True)
_DENSE_L2 = _DenseVariant(_dense_args, "dense_l2", "dense_l2", ("xsq", "xnorm_max"), pad=float("inf"))
_DENSE_L2_F16 = _DenseVariant(_dense_f16_args, "dense_l2_f16", "dense_l2_f16", ("xsq", "xnorm_max"), pad=float("inf"))
_DENSE_L2_BF16X3 = _DenseVariant(_dense_args, "dense_l2_bf16x3", "dense_l2", ("xsq", "xnorm_max"), pad=float("inf"),
                                 scores_ws=True)
_DENSE_SQ8 = _DenseVariant(_dense_sq8_args, "dense_sq8", "dense_sq8", ("dec", "cstat"), ("dec",), scores_ws=True)
_DENSE_L2_SQ8 = _DenseVariant(_dense_sq8_args, "dense_l2_sq8", "dense_l2_sq8", ("dec", "xsq", "cstat"), ("dec",),
                              pad=float("inf"), scores_ws=True)


def _dense_call(v: _DenseVariant, kind: str, h, x, q, t: dict, stream, k=0, id_offset=0, sel_slack=0.0):
    """(name, argument tuple) of one library call of variant `v`; kind: "search_q", "search_exact", "scores", or the subset
    searches "search_rows_q" and "search_rows_exact".  The header's order: h, x, ldx, N, D, q, nq, the side operands the variant
    names for that entry, (the subset searches: rows, ns,) the scalars, the outputs, the workspace (where `t` holds one), the
    stream.  `t`: the side operands, "rows", the outputs and "ws" by name.  Touches no device and loads no library: the
    positions come from the variant's names alone (tests/test_search_arg_order.py)."""
    search_q = (v.entry, v.side, (int(k), int(id_offset), float(sel_slack)), ("scores", "ids", "status", "qstatus"))
    search_exact = (v.exact, v.exact_side, (int(k), int(id_offset)), ("scores", "ids"))
    entry, side, scalars, outs = {
        "search_q": search_q,
        "search_exact": search_exact,
        "scores": (v.entry, tuple(n for n in v.side if n in ("dec", "xsq")), (), ("out",)),    # no certificate: no xnorm_max, cstat
        "search_rows_q": search_q,
        "search_rows_exact": search_exact,
    }[kind]
    rows = (_p(t["rows"]), t["rows"].numel()) if kind in ("search_rows_q", "search_rows_exact") else ()
    ws = () if t.get("ws") is None else (_p(t["ws"]), t["ws"].numel())
    return f"rc_{entry}_{kind}", (h, _p(x), x.stride(0), x.shape[0], x.shape[1], _p(q), q.shape[0], *(_p(t[n]) for n in side),
                                  *rows, *scalars, *(_p(t[n]) for n in outs), *ws, stream)


# the variants whose kernels read the store through a row list (rc_<entry>_search_rows_q / _rows_exact)
_DENSE_SUBSET = ("dense", "dense_f16", "dense_l2", "dense_l2_f16")


def _dense_rows(name: str, rows, x: torch.Tensor, check_rows: bool) -> torch.Tensor:
    """The row list of a subset search, refused with a ValueError before anything reaches the library: int64 [ns] on the
    device of `x`, contiguous, and (check_rows: one host read) every row in [0, N), strictly ascending.  The library reads
    x[rows[i]] unchecked: a list that is not valid by construction must not pass with the check off."""
    if not isinstance(rows, torch.Tensor) or rows.dim() != 1:
        raise ValueError(f"{name}: rows must be a 1-d tensor of row numbers")
    if x.dim() != 2:
        raise ValueError(f"{name}: x [N, D]")
    if rows.dtype != torch.int64:
        raise ValueError(f"{name}: rows must be int64, got {rows.dtype}")
    if rows.device != x.device:
        raise ValueError(f"{name}: rows must be on the device of the corpus ({x.device}), got {rows.device}")
    if not rows.is_contiguous():
        raise ValueError(f"{name}: rows must be contiguous")
    if rows.numel() > x.shape[0]:
        raise ValueError(f"{name}: {rows.numel()} rows selected of a corpus of {x.shape[0]}")
    if check_rows and rows.numel():
        ok = (rows[0] >= 0) & (rows[-1] < x.shape[0])
        if rows.numel() > 1:
            ok = ok & (rows[1:] > rows[:-1]).all()
        if not bool(ok):
            raise ValueError(f"{name}: rows must be strictly ascending row numbers in [0, {x.shape[0]})")
    return rows


def _dense_search_exact(v: _DenseVariant, x: torch.Tensor, q: torch.Tensor, k: int, id_offset: int,
                        dec: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None, check_rows: bool = True):
    """rows (checked here unless the caller has: check_rows): the search runs over x[rows] in place, N below is then ns."""
    if rows is not None:
        rows = _dense_rows(f"rc_{v.exact}_search_rows_exact", rows, x, check_rows)
    x, q = v.args(x, q, k)
    N, D = (x.shape[0] if rows is None else rows.numel()), x.shape[1]
    nq = q.shape[0]
    lib, h, s, _ = _ctx(q)
    scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    if nq == 0 or N == 0:
        scores.fill_(v.pad)
        ids.fill_(-1)
        return scores, ids
    wsb = getattr(lib, f"rc_{v.exact}_search_exact_ws_bytes")(N, D, nq, int(k))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=q.device)
    name, args = _dense_call(v, "search_exact" if rows is None else "search_rows_exact", h, x, q,
                             {"dec": dec, "rows": rows, "scores": scores, "ids": ids, "ws": ws}, s, k, id_offset)
    _lib.check(getattr(lib, name)(*args), name, h)
    return scores, ids


def _dense_search(v: _DenseVariant, x: torch.Tensor, q: torch.Tensor, k: int, id_offset: int, sel_slack: Optional[float],
                  defer: bool, method: str, max_retries: int, xnorm_max: Optional[torch.Tensor] = None,
                  xsq: Optional[torch.Tensor] = None, dec: Optional[torch.Tensor] = None,
                  cstat: Optional[torch.Tensor] = None, stats: Optional[dict] = None, rows: Optional[torch.Tensor] = None,
                  check_rows: bool = True):
    """rows: the subset search (`dense_search`): the route runs over x[rows] in place.  NS below is the number of rows it
    searches (ns, or N without rows): the route, the sample and the workspace follow it; xsq and xnorm_max stay the store's."""
    if method not in ("auto", "exact"):
        raise ValueError("method must be 'auto' or 'exact'")
    if rows is not None:
        if v.entry not in _DENSE_SUBSET:
            raise ValueError(f"rc_{v.entry}_search_q: no subset search for this variant")
        rows = _dense_rows(f"rc_{v.entry}_search_rows_q", rows, x, check_rows)
    x, q = v.args(x, q, k)
    if sel_slack is None:
        sel_slack = DENSE_SEL_SLACK
    N, D = x.shape
    NS = N if rows is None else rows.numel()
    nq = q.shape[0]
    if method == "exact" or nq == 0 or NS == 0:
        got = _dense_search_exact(v, x, q, k, id_offset, dec, rows, False)
        return PendingSearch(None, got[0], got[1], None, None, 0.0, 0) if defer else got
    lib, h, _, dev = _ctx(q)
    side = {"dec": dec, "cstat": cstat}          # the tensors behind the entry's side operands (v.side)
    if "xnorm_max" in v.side:
        if xnorm_max is None:
            # up to DENSE_EXACT_MAX_N rows the library takes the exact route and never reads the norm
            xnorm_max = dense_xnorm_max(x) if NS > DENSE_EXACT_MAX_N else torch.zeros((1,), dtype=torch.float32, device=x.device)
        _need_cuda(xnorm_max)
        side["xnorm_max"] = xnorm_max.to(torch.float32).reshape(1)
    if "xsq" in v.side:
        if xsq is None:
            xsq = dense_row_sqnorms(x) if NS > DENSE_EXACT_MAX_N else torch.zeros((N,), dtype=torch.float32, device=x.device)
        _need_cuda(xsq)
        if xsq.shape != (N,):
            raise ValueError("dense search: xsq must hold one squared norm per row, [N]")
        side["xsq"] = xsq.to(torch.float32).contiguous()
    kind = "search_q" if rows is None else "search_rows_q"
    side["rows"] = rows
    name = f"rc_{v.entry}_{kind}"
    search_q, ws_bytes = getattr(lib, name), getattr(lib, f"rc_{v.entry}_search_ws_bytes")

    def launch(qq, slack, out_s, out_i, status, qstatus):
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for c0 in range(0, qq.shape[0], DENSE_QCHUNK):
            n = min(DENSE_QCHUNK, qq.shape[0] - c0)
            wsb = ws_bytes(NS, D, n, int(k))
            ws = torch.empty((wsb,), dtype=torch.uint8, device=q.device)     # released in stream order
            t = dict(side, scores=out_s[c0:c0 + n], ids=out_i[c0:c0 + n], status=status, qstatus=qstatus[c0:c0 + n], ws=ws)
            _lib.check(search_q(*_dense_call(v, kind, h, x, qq[c0:c0 + n], t, st, k, id_offset, slack)[1]), name, h)
            if stats is not None and len(stats.setdefault("survivors", [])) * DENSE_QCHUNK < nq:
                off = C.c_size_t(0)          # measurement: the first pass's candidate counts (rc_<entry>_search_ws_counts)
                _lib.check(getattr(lib, f"rc_{v.entry}_search_ws_counts")(N, D, n, int(k), C.byref(off)), name, h)
                if off.value:
                    stats["survivors"].append(ws[off.value:off.value + 4 * n].view(torch.int32).clone())

    def rerun(idx, slack, exact):
        qq = q[idx].contiguous()
        if exact:
            s_, i_ = _dense_search_exact(v, x, qq, k, id_offset, dec, rows, False)
            return s_, i_, None
        s_ = torch.empty((qq.shape[0], k), dtype=torch.float32, device=q.device)
        i_ = torch.empty((qq.shape[0], k), dtype=torch.int64, device=q.device)
        status = torch.zeros((1,), dtype=torch.int32, device=q.device)
        qs = torch.zeros((qq.shape[0],), dtype=torch.int32, device=q.device)
        launch(qq, slack, s_, i_, status, qs)
        return s_, i_, qs

    _warm_retry_ops(q.device)
    scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    status = torch.zeros((1,), dtype=torch.int32, device=q.device)
    qstatus = torch.zeros((nq,), dtype=torch.int32, device=q.device)
    launch(q, float(sel_slack), scores, ids, status, qstatus)
    pending = PendingSearch(rerun, scores, ids, status, qstatus, float(sel_slack), max_retries,
                            stream=torch.cuda.current_stream(dev))
    return pending if defer else pending.result()


def _dense_scores(v: _DenseVariant, name: str, x, q, dec=None, xsq=None) -> torch.Tensor:
    """The `*_scores` test hooks: the raw screen values [nq, N] of variant `v` (rc_<entry>_scores).  `dec` and `xsq` are looked
    at where the variant's search takes them; a missing xsq is computed from the rows (the decoded rows of int8 codes)."""
    x, q = v.args(x, q, 1)
    t = {"dec": _dense_sq8_dec(x, dec) if "dec" in v.side else None}
    lib, h, s, _ = _ctx(q)
    if "xsq" in v.side:
        if xsq is None:
            xsq = dense_row_sqnorms(x) if t["dec"] is None else dense_sq8_row_sqnorms(x, t["dec"])
        _need_cuda(xsq)
        t["xsq"] = xsq.to(torch.float32).contiguous()
        if xsq.shape != (x.shape[0],):
            raise ValueError(f"{name}: xsq must hold one squared norm per row, [N]")
    t["out"] = torch.empty((q.shape[0], x.shape[0]), dtype=torch.float32, device=q.device)
    if t["out"].numel():
        if v.scores_ws:
            wsb = getattr(lib, f"rc_{v.entry}_scores_ws_bytes")(x.shape[1], q.shape[0])
            t["ws"] = torch.empty((wsb,), dtype=torch.uint8, device=q.device)
        entry, args = _dense_call(v, "scores", h, x, q, t, s)
        _lib.check(getattr(lib, entry)(*args), entry, h)
    return t["out"]


def _error_constants(entry: str, n: int) -> tuple:
    """The `n` doubles of rc_<entry>_error_constants.  No GPU needed."""
    c = (C.c_double * n)()
    getattr(_lib.load(), f"rc_{entry}_error_constants")(c)
    return tuple(float(v) for v in c)


DENSE_RERANK_MAX_KC = 16384         # candidates per query of dense_rerank (ADC_CAND_CAP, csrc/topk.h)


def dense_rerank_ws_bytes(nq: int, kc: int) -> int:
    """Workspace of one rc_dense_rerank / rc_dense_f16_rerank call: a multiple of 256; 0 for a shape outside the limits."""
    return int(_lib.load().rc_dense_rerank_ws_bytes(int(nq), int(kc)))


def dense_rerank(x: torch.Tensor, q: torch.Tensor, cand_ids: torch.Tensor, k: int, metric: int = METRIC_INNER_PRODUCT,
                 id_offset: int = 0):
    """Exact re-ranking of candidate lists (the second stage of faiss.IndexRefineFlat): `cand_ids` [nq, kc] int64 are scored
    against their rows of the dense store `x` [N, D] and the `k` best per query returned as (scores [nq, k] fp32, ids [nq, k]
    int64) — csrc/dense_rerank.hip.  x is fp32, or fp16 (then the queries are rounded to fp16 as `dense_search_f16` rounds
    them).  A candidate c is valid iff 0 <= c - id_offset < N; everything else (the -1 holes of an IVF search, foreign ids) is
    skipped, an id given twice is scored twice.  The score of a valid candidate is bit for bit the one `dense_search_exact` /
    `dense_search_l2_exact` (or their f16 forms) give that (query, row).  METRIC_INNER_PRODUCT: score descending, ties by the
    lower id, (-inf, -1) after the valid ones; METRIC_L2: squared distance ascending, ties by the lower id, (+inf, -1).
    1 <= k <= 8192, 1 <= kc <= 16384, N < 2^32; argument errors are ValueError before any device work."""
    l2 = _adc_metric(metric)
    if x.dim() != 2 or q.dim() != 2 or x.shape[1] != q.shape[1] or x.shape[1] < 1:
        raise ValueError("dense_rerank: x [N, D] and q [nq, D] with the same D >= 1")
    if x.dtype not in (torch.float32, torch.float16):
        raise ValueError("dense_rerank: the store must be float32 or float16")
    if cand_ids.dim() != 2 or cand_ids.dtype != torch.int64:
        raise ValueError("dense_rerank: cand_ids must be an int64 [nq, kc] matrix")
    if cand_ids.shape[0] != q.shape[0]:
        raise ValueError(f"dense_rerank: {cand_ids.shape[0]} candidate lists for {q.shape[0]} queries")
    k, kc = int(k), int(cand_ids.shape[1])
    if not 1 <= k <= DENSE_MAX_K:
        raise ValueError(f"dense_rerank: k must be in [1, {DENSE_MAX_K}]")
    if not 1 <= kc <= DENSE_RERANK_MAX_KC:
        raise ValueError(f"dense_rerank: kc must be in [1, {DENSE_RERANK_MAX_KC}]")
    if x.shape[0] >= 1 << 32:
        raise ValueError("dense_rerank: N must be < 2^32")
    _need_cuda(x, q, cand_ids)
    f16 = x.dtype == torch.float16
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    q = q.to(x.device).to(x.dtype).contiguous()             # fp16: round to nearest even, as the corpus was
    cand_ids = cand_ids.to(x.device)
    if cand_ids.stride(1) != 1 or cand_ids.stride(0) < kc:
        cand_ids = cand_ids.contiguous()
    N, D = x.shape
    nq = q.shape[0]
    scores = torch.empty((nq, k), dtype=torch.float32, device=q.device)
    ids = torch.empty((nq, k), dtype=torch.int64, device=q.device)
    if nq == 0:
        return scores, ids
    lib, h, s, _ = _ctx(q)
    name = "rc_dense_f16_rerank" if f16 else "rc_dense_rerank"
    ldx = x.stride(0) if N > 1 else D
    for c0 in range(0, nq, DENSE_QCHUNK):
        n = min(DENSE_QCHUNK, nq - c0)
        wsb = lib.rc_dense_rerank_ws_bytes(n, kc)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=q.device)         # released in stream order
        _lib.check(getattr(lib, name)(h, _p(x), ldx, N, D, _p(q[c0:c0 + n]), n, _p(cand_ids[c0:c0 + n]), cand_ids.stride(0), kc,
                                      k, int(id_offset), int(l2), _p(scores[c0:c0 + n]), _p(ids[c0:c0 + n]), _p(ws), wsb, s),
                   name, h)
    return scores, ids


IVF_FLAT_MAX_NLIST = 16384          # cells of the dense IVF search (csrc/ivf_flat.hip)


def ivf_flat_query_group() -> int:
    """Queries of one cell that share a task of the dense IVF scan (IVFF_QG of csrc/ivf_flat.hip, read from the library)."""
    return int(_lib.load().rc_ivf_flat_query_group())


def ivf_flat_search_ws_bytes(nq: int, nprobe: int, nlist: int, stride: int) -> int:
    """Workspace of one rc_ivf_flat_search / rc_ivf_flat_f16_search call: a multiple of 256; 0 for nq <= 0, nprobe <= 0,
    nprobe > nlist or stride <= 0.  No GPU involved."""
    return int(_lib.load().rc_ivf_flat_search_ws_bytes(int(nq), int(nprobe), int(nlist), int(stride)))


def ivf_flat_search(xb: torch.Tensor, list_off: torch.Tensor, ids: torch.Tensor, q: torch.Tensor, probes: torch.Tensor,
                    stride: int, k: int, metric: int = METRIC_INNER_PRODUCT, *, rows: Optional[torch.Tensor] = None,
                    sel_off: Optional[torch.Tensor] = None, check_rows: bool = True):
    """One call of the exact IVF search over dense rows (csrc/ivf_flat.hip): `xb` [N, D] fp32 or fp16, list-major; `list_off`
    [nlist + 1] int64; `ids` [N] int64 corpus positions; `q` [nq, D] (rounded to fp16 for an fp16 store, as `dense_search_f16`
    rounds it); `probes` [nq, nprobe] int32, distinct cells per query in ascending order (rc_ivf_select_probes); `stride` >= the
    rows any nprobe cells hold.  Returns (scores or distances [nq, k], ids [nq, k], status [1] int32, qstatus [nq] int32) without
    synchronising: bit 1 of a query's status = more than 16384 of its probed rows tie at its k-th score and its row of the
    output is not valid (`IVFFlatIndex` answers those queries by the exact search over their probed rows); bit 2 of `status` =
    a probe outside [0, nlist) or a `stride` too small.  Argument errors are ValueError before any device work.
    rows, sel_off (both or neither): the search runs over the selected rows of the store in place (rc_ivf_flat_search_rows).
    `rows` int64 [ns]: the list-major positions (rows of `xb`) selected, strictly ascending, in [0, N), on the store's device;
    `sel_off` int64 [nlist + 1]: the offsets of the cells inside `rows`, from 0 to ns, every row of segment c inside
    [list_off[c], list_off[c + 1]).  The result is that of a store holding only those rows under the same cells, with the ids
    of this one; `stride` then bounds the SELECTED rows of any nprobe cells.  An empty `rows` returns padding without a
    launch.  check_rows=True verifies the pair on the device (one synchronisation) and raises ValueError before any library
    call; the library reads x[rows[i]] unchecked, so check_rows=False is for lists valid by construction
    (`IVFFlatIndex._selection`)."""
    return _ivf_flat_search("ivf_flat_search", "xb", xb, None, None, list_off, ids, q, probes, stride, k, metric, rows, sel_off,
                            check_rows)


def ivf_flat_sq8_search(xb8: torch.Tensor, dec: torch.Tensor, list_off: torch.Tensor, ids: torch.Tensor, q: torch.Tensor,
                        probes: torch.Tensor, stride: int, k: int, metric: int = METRIC_INNER_PRODUCT, *,
                        rows: Optional[torch.Tensor] = None, sel_off: Optional[torch.Tensor] = None, check_rows: bool = True):
    """`ivf_flat_search` over a list-major store of 8-bit scalar-quantiser codes (rc_ivf_flat_sq8_search): `xb8` [N, D] int8 =
    c - 128, `dec` [2, D] fp32 = the steps, then the mids (`dense_search_sq8`'s), `q` [nq, D] fp32, not rounded; everything
    else, the returns and the status bits as `ivf_flat_search`.  Scores are bit for bit those of `ivf_flat_search` over
    `dense_sq8_decode(xb8, dec)`, under either metric.  Any row pitch >= D and any alignment (a column slice of a wider
    matrix is read in place).  D <= 65536; argument errors are ValueError before any device work.  rows, sel_off,
    check_rows: as `ivf_flat_search` (rc_ivf_flat_sq8_search_rows)."""
    return _ivf_flat_search("ivf_flat_sq8_search", "xb8", xb8, dec, None, list_off, ids, q, probes, stride, k, metric, rows,
                            sel_off, check_rows)


def ivf_flat_sq8r_search(xb8: torch.Tensor, dec: torch.Tensor, coarse: torch.Tensor, list_off: torch.Tensor, ids: torch.Tensor,
                         q: torch.Tensor, probes: torch.Tensor, stride: int, k: int, metric: int = METRIC_INNER_PRODUCT, *,
                         rows: Optional[torch.Tensor] = None, sel_off: Optional[torch.Tensor] = None, check_rows: bool = True):
    """`ivf_flat_sq8_search` over codes of residuals (rc_ivf_flat_sq8r_search): the rows of cell l hold the codes of x -
    `coarse`[l], `coarse` [nlist, D] fp32 on the device of the store (any row pitch >= D), and a stored value is
    fp32(fmaf(c', step, mid) + coarse[l][d]) — the decode, then one separate fp32 addition.  Scores are bit for bit those of
    `ivf_flat_search` over `dense_sq8_decode(xb8, dec)` + the centroid of every row's cell, under either metric.  The checks
    of `ivf_flat_sq8_search`, and `coarse` must be float32 [nlist, D].  rows, sel_off, check_rows: as `ivf_flat_search`
    (rc_ivf_flat_sq8r_search_rows); a selected row keeps the centroid of its cell."""
    if not isinstance(coarse, torch.Tensor):
        raise ValueError("ivf_flat_sq8r_search: coarse must be a float32 tensor [nlist, D]")
    return _ivf_flat_search("ivf_flat_sq8r_search", "xb8", xb8, dec, coarse, list_off, ids, q, probes, stride, k, metric, rows,
                            sel_off, check_rows)


def _ivf_flat_call(h, xb, list_off, ids, q, dec, coarse, probes, stride, k, l2, scores, out_ids, status, qstatus, ws, stream,
                   rows=None, sel_off=None):
    """(name, argument tuple) of one call of the four rc_ivf_flat*_search entries, chosen by the store's type and by which of
    `dec` / `coarse` are tensors.  The header's order: h, x, ldx, list_off, ids, N, nlist, D, q, nq, [dec, [coarse, ldc]], probes,
    nprobe, stride, k, metric, the outputs, the workspace, the stream.  rows: the entry of the same name with _rows, and `rows,
    ns, sel_off` after the stream.  Touches no device and loads no library."""
    (N, D), nlist = xb.shape, list_off.numel() - 1
    side = () if dec is None else (_p(dec),) if coarse is None else (_p(dec), _p(coarse), coarse.stride(0) if nlist > 1 else D)
    form = "_f16" if xb.dtype == torch.float16 else "" if dec is None else "_sq8" if coarse is None else "_sq8r"
    sub = () if rows is None else (_p(rows), rows.numel(), _p(sel_off))
    return f"rc_ivf_flat{form}_search" + ("_rows" if sub else ""), (
        h, _p(xb), xb.stride(0) if N > 1 else D, _p(list_off), _p(ids), N, nlist, D, _p(q), q.shape[0], *side, _p(probes),
        probes.shape[1], int(stride), int(k), int(l2), _p(scores), _p(out_ids), _p(status), _p(qstatus), _p(ws), ws.numel(), stream,
        *sub)


def _ivf_flat_rows(name: str, rows, sel_off, xb: torch.Tensor, list_off: torch.Tensor, check_rows: bool):
    """The (rows, sel_off) pair of an IVF-flat subset search, refused with a ValueError before anything reaches the library.
    Always: both given, int64, 1-d, rows on the device of the store, sel_off [nlist + 1].  check_rows (one synchronisation):
    rows strictly ascending in [0, N); sel_off non-decreasing from 0 to ns; every row of segment c in [list_off[c],
    list_off[c + 1]).  Returns the pair, contiguous, sel_off on the device of rows."""
    if rows is None or sel_off is None:
        raise ValueError(f"{name}: rows and sel_off come together (both, or neither)")
    if not isinstance(rows, torch.Tensor) or rows.dim() != 1 or rows.dtype != torch.int64:
        raise ValueError(f"{name}: rows must be a 1-d int64 tensor of list-major row positions")
    if rows.device != xb.device:
        raise ValueError(f"{name}: rows must be on the device of the store ({xb.device}), got {rows.device}")
    N, nlist = xb.shape[0], list_off.numel() - 1
    if not isinstance(sel_off, torch.Tensor) or sel_off.dtype != torch.int64 or sel_off.shape != (nlist + 1,):
        raise ValueError(f"{name}: sel_off must be int64 [nlist + 1] = [{nlist + 1}]")
    ns = rows.numel()
    if ns > N:
        raise ValueError(f"{name}: {ns} rows selected of a store of {N}")
    sel_off = sel_off.to(rows.device)
    if check_rows:
        lo = list_off.to(rows.device)
        ok = (sel_off[0] == 0) & (sel_off[-1] == ns) & (sel_off[1:] >= sel_off[:-1]).all()
        if ns:
            ok = ok & (rows[0] >= 0) & (rows[-1] < N)
            if ns > 1:
                ok = ok & (rows[1:] > rows[:-1]).all()
            # the cell a row is LISTED under (its segment of sel_off) must be the cell that holds it (its segment of list_off)
            at = torch.arange(ns, device=rows.device)
            ok = ok & (torch.searchsorted(sel_off, at, right=True) == torch.searchsorted(lo, rows, right=True)).all()
        if not bool(ok):
            raise ValueError(f"{name}: rows must be strictly ascending positions in [0, {N}), sel_off non-decreasing from 0 to "
                             f"{ns}, and every row of segment c inside [list_off[c], list_off[c + 1])")
    return rows.contiguous(), sel_off.contiguous()


def _ivf_flat_search(name, store, xb, dec, coarse, list_off, ids, q, probes, stride, k, metric, rows=None, sel_off=None,
                     check_rows=True):
    """The body of the three IVF-flat searches.  store "xb": the fp32 / fp16 store, queries of any type rounded to the store's;
    "xb8": int8 codes with `dec`, fp32 queries, and `coarse` None = the vectors themselves are encoded, else their residuals."""
    coded = store == "xb8"
    l2 = _adc_metric(metric)
    if xb.dim() != 2 or q.dim() != 2 or xb.shape[1] != q.shape[1] or xb.shape[1] < 1:
        raise ValueError(f"{name}: {store} [N, D] and q [nq, D] with the same D >= 1")
    N, D = xb.shape
    if coded:
        if xb.dtype != torch.int8:
            raise ValueError(f"{name}: the store must be int8 codes, c - 128")
        if q.dtype != torch.float32:
            raise ValueError(f"{name}: the queries must be float32")
        if D > DENSE_SQ8_MAX_D:
            raise ValueError(f"{name}: D must be <= {DENSE_SQ8_MAX_D}")
        if dec.dtype != torch.float32 or dec.shape != (2, D):
            raise ValueError(f"{name}: dec must be float32 [2, D]: the steps, then the mids")
    elif xb.dtype not in (torch.float32, torch.float16):
        raise ValueError(f"{name}: the store must be float32 or float16")
    if not 1 <= int(k) <= DENSE_MAX_K:
        raise ValueError(f"{name}: k must be in [1, {DENSE_MAX_K}]")
    nlist = list_off.numel() - 1
    if list_off.dtype != torch.int64 or list_off.dim() != 1 or not 1 <= nlist <= IVF_FLAT_MAX_NLIST:
        raise ValueError(f"{name}: list_off must be int64 [nlist + 1], 1 <= nlist <= {IVF_FLAT_MAX_NLIST}")
    if coarse is not None and (coarse.dtype != torch.float32 or coarse.shape != (nlist, D)):
        raise ValueError(f"{name}: coarse must be float32 [nlist, D]: the centroids the rows were encoded against")
    if ids.dtype != torch.int64 or ids.shape != (N,):
        raise ValueError(f"{name}: ids must be int64 [N]")
    if probes.dim() != 2 or probes.dtype != torch.int32 or probes.shape[0] != q.shape[0] or not 1 <= probes.shape[1] <= nlist:
        raise ValueError(f"{name}: probes must be int32 [nq, nprobe], 1 <= nprobe <= nlist")
    if not 1 <= N < 1 << 32:
        raise ValueError(f"{name}: 1 <= N < 2^32")
    if int(stride) < 1:
        raise ValueError(f"{name}: stride must be >= 1")
    if rows is not None or sel_off is not None:
        rows, sel_off = _ivf_flat_rows(name, rows, sel_off, xb, list_off, check_rows)
    _need_cuda(xb, dec, coarse, list_off, ids, q, probes)
    if coarse is not None and coarse.device != xb.device:
        raise ValueError(f"{name}: coarse must be on the device of the store")
    if xb.stride(1) != 1 or (N > 1 and xb.stride(0) < D):
        xb = xb.contiguous()
    if coded:
        q, dec = q.to(xb.device).contiguous(), dec.to(xb.device).contiguous()
    else:
        q = q.to(xb.device).to(xb.dtype).contiguous()       # fp16: round to nearest even, as the corpus was
    list_off, ids, probes = list_off.contiguous(), ids.contiguous(), probes.contiguous()
    nq, nprobe = probes.shape
    scores = torch.empty((nq, int(k)), dtype=torch.float32, device=q.device)
    out_ids = torch.empty((nq, int(k)), dtype=torch.int64, device=q.device)
    flags = torch.zeros((1 + nq,), dtype=torch.int32, device=q.device)       # [status | per-query status]: one fill
    status, qstatus = flags[:1], flags[1:]
    if nq == 0:
        return scores, out_ids, status, qstatus
    if rows is not None and rows.numel() == 0:               # an empty selection: all padding, no launch
        scores.fill_(float("inf") if l2 else float("-inf"))
        out_ids.fill_(-1)
        return scores, out_ids, status, qstatus
    if coarse is not None and (coarse.stride(1) != 1 or (nlist > 1 and coarse.stride(0) < D)):
        coarse = coarse.contiguous()
    lib, h, s, _ = _ctx(q)
    ws = torch.empty((lib.rc_ivf_flat_search_ws_bytes(nq, nprobe, nlist, int(stride)),), dtype=torch.uint8,
                     device=q.device)                                        # released in stream order
    entry, args = _ivf_flat_call(h, xb, list_off, ids, q, dec, coarse, probes, stride, k, l2, scores, out_ids, status, qstatus,
                                 ws, s, rows, sel_off)
    _lib.check(getattr(lib, entry)(*args), entry, h)
    return scores, out_ids, status, qstatus


def dense_xnorm_max(x: torch.Tensor, rows_per_step: int = 1 << 16) -> torch.Tensor:
    """Device fp32 scalar [1] >= the largest Euclidean row norm of the floating-point matrix `x` of any dtype (fp64 sums,
    rounded upwards; +inf if the norm exceeds fp32): the `xnorm_max` of `dense_search_bf16x3` and `dense_search_f16`.  No host
    synchronisation."""
    if not x.dtype.is_floating_point:
        raise ValueError("dense_xnorm_max: a floating-point matrix")
    best = torch.zeros((), dtype=torch.float64, device=x.device)
    for r0 in range(0, x.shape[0], rows_per_step):
        best = torch.maximum(best, x[r0:r0 + rows_per_step].double().square_().sum(1).max())
    # the fp64 -> fp32 conversion rounds to nearest, by a factor of at most 1 + 2^-24: the 2^-20 covers it
    return (best.sqrt() * (1.0 + 2.0 ** -20)).float().reshape(1)


def dense_search_exact(x: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0, *, rows: Optional[torch.Tensor] = None,
                       check_rows: bool = True):
    """The same answer as `dense_search` by the route that cannot fail (rc_dense_search_exact): full score rows and a radix
    select of the min(k, N) best keys.  rows, check_rows: as `dense_search` (rc_dense_search_rows_exact)."""
    return _dense_search_exact(_DENSE_F32, x, q, k, id_offset, None, rows, check_rows)


def dense_search(x: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0, sel_slack: Optional[float] = None,
                 defer: bool = False, method: str = "auto", max_retries: int = 2, *, rows: Optional[torch.Tensor] = None,
                 check_rows: bool = True):
    """Exact top-k inner-product search of `q` [nq, D] against the fp32 corpus `x` [N, D] (faiss.IndexFlatIP,
    evaluate_dense.py:84-129).  Returns (scores [nq, k] fp32, ids [nq, k] int64 = row + id_offset), sorted (score desc, id
    asc); -inf / -1 past N.  Scores are the fp32 fmaf chain over d ascending (include/repconc_hip.h), bit for bit.
    method="exact": the exact route only.  defer: a `PendingSearch` (queries the sampled threshold fails are repeated, then
    answered by the exact route; `.stats`).  Query sets larger than DENSE_QCHUNK are split into several library calls.
    rows (keyword only): search only the rows `rows` of `x`, in place — int64 [ns] on x's device, contiguous, strictly ascending,
    in [0, N).  The answer is exactly that of the same search over `x[rows]` with every id i replaced by id_offset +
    rows[i] (ids and score bits, the padding past ns included); the route, the sample and the workspace follow ns, and ns = 0
    returns padding.  check_rows=True verifies the list (one host read) and raises ValueError before any library call; the
    library itself reads x[rows[i]] unchecked, so pass False only for a list that is valid by construction
    (`repconc_amd.selector`)."""
    return _dense_search(_DENSE_F32, x, q, k, id_offset, sel_slack, defer, method, max_retries, rows=rows, check_rows=check_rows)


# --------------------------------------------------------------------------------------------------- dense, fp16 storage
def dense_f16_error_constant() -> float:
    """The factor of E_q as the certificate kernel was compiled with it (DENSE_F16_ERR_C, csrc/dense_search_f16.hip)."""
    return float(_lib.load().rc_dense_f16_error_constant())


def dense_f16_error_bound(D: int, qnorm, xmax):
    """E = 4 D_pad 2^-24 ||q||_2 X, D_pad = D rounded up to 16: the bound on |s~ - s| between ANY fp32 accumulation s~ of the D
    exact products q_d x_d (the f16 matrix cores' screen) and the fmaf chain s that the certificate of `dense_search_f16` uses
    (include/repconc_hip.h, rc_dense_f16_search_q).  Either sum errs by at most D - 1 roundings of at most 2^-23 (truncation)
    of a partial sum <= sum_d |q_d x_d| <= ||q|| ||x||.  Plain float / numpy arithmetic: `qnorm`, `xmax` scalars or arrays."""
    dpad = (int(D) + 15) // 16 * 16
    return dense_f16_error_constant() * dpad * 2.0 ** -24 * qnorm * xmax


dense_f16_xnorm_max = dense_xnorm_max      # the `xnorm_max` of `dense_search_f16`


def dense_search_f16_exact(x16: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0, *,
                           rows: Optional[torch.Tensor] = None, check_rows: bool = True):
    """The same answer as `dense_search_f16` by the route that cannot fail (rc_dense_f16_search_exact).  rows, check_rows: as
    `dense_search` (rc_dense_f16_search_rows_exact)."""
    return _dense_search_exact(_DENSE_F16, x16, q, k, id_offset, None, rows, check_rows)


def dense_f16_scores(x16: torch.Tensor, q16: torch.Tensor) -> torch.Tensor:
    """The raw approximate scores s~ [nq, N] of the f16 matrix-core screen (rc_dense_f16_scores): a test hook, never a result."""
    return _dense_scores(_DENSE_F16, "dense_f16_scores", x16, q16)


def dense_search_f16(x16: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0, sel_slack: Optional[float] = None,
                     defer: bool = False, method: str = "auto", max_retries: int = 2,
                     xnorm_max: Optional[torch.Tensor] = None, *, rows: Optional[torch.Tensor] = None, check_rows: bool = True):
    """Exact top-k inner-product search of `q` [nq, D] against the FINITE fp16 corpus `x16` [N, D] (faiss.IndexFlatIP with
    useFloat16).  The queries are rounded to fp16 (round to nearest even; a component of magnitude >= 65520 becomes inf and is
    not checked for: such a query gets no certificate and the exact route gives it the chain's inf / NaN scores); scores are
    the fp32 fmaf chain over d ascending of
    the widened values: ids and score bits equal `dense_search(x16.float(), q.half().float(), k)`.  The f16 matrix cores only
    screen; candidates are rescored by the chain and every answer of the fast route carries a certificate (qstatus bit2 when
    it cannot be given: such queries are repeated, then answered by the exact route — `.stats` of the `PendingSearch`).
    xnorm_max: device fp32 [1], >= the largest row norm of x16 (`dense_f16_xnorm_max`, computed here when None).
    Everything else as `dense_search`, the subset search (rows, check_rows) included: xnorm_max stays the bound over ALL rows."""
    return _dense_search(_DENSE_F16, x16, q, k, id_offset, sel_slack, defer, method, max_retries, xnorm_max, rows=rows,
                         check_rows=check_rows)


# ------------------------------------------------------------------------------------ dense, fp32 corpus, bf16x3 screen
def dense_bf16x3_error_constants():
    """(c_sum, c_split, c_sub, c_under) of E_q as the certificate kernel was compiled with them (csrc/dense_search_bf16x3.hip)."""
    return _error_constants("dense_bf16x3", 4)


def dense_bf16x3_error_bound(D: int, qnorm, xmax):
    """E = (8 D_pad 2^-24 + 4 * 2^-16) ||q|| X + 2^-133 sqrt(D_pad) (||q|| + X) + 4 D_pad 2^-149, D_pad = D rounded up to 16:
    the bound on |s~ - s| between the bf16x3 screen (any fp32 accumulation of the 3 D products q_h x_h + q_h x_l + q_l x_h of the
    round-to-nearest-even bf16 splits) and the fmaf chain s that the certificate of `dense_search_bf16x3` uses; derivation in
    the header comment of csrc/dense_search_bf16x3.hip.  The constants are the library's.  Plain float / numpy arithmetic."""
    c_sum, c_split, c_sub, c_under = dense_bf16x3_error_constants()
    dpad = (int(D) + 15) // 16 * 16
    return (c_sum * dpad * 2.0 ** -24 + c_split * 2.0 ** -16) * qnorm * xmax + c_sub * dpad ** 0.5 * (qnorm + xmax) + c_under * dpad


def dense_bf16x3_scores(x: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """The raw approximate scores s~ [nq, N] of the bf16x3 matrix-core screen (rc_dense_bf16x3_scores): a test hook, never a
    result."""
    return _dense_scores(_DENSE_BF16X3, "dense_bf16x3_scores", x, q)


def dense_search_bf16x3(x: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0, sel_slack: Optional[float] = None,
                        defer: bool = False, method: str = "auto", max_retries: int = 2,
                        xnorm_max: Optional[torch.Tensor] = None):
    """`dense_search` with the screen on the bf16 matrix cores: the same ids and score bits for a FINITE fp32 corpus `x` whose
    values round to finite bf16 (magnitude < 2^128 - 2^119; `FlatIPIndex(screen="bf16x3")` checks it) and any queries.
    Nothing is rounded in the result: the screen's three-term bf16 split only chooses candidates, which are rescored by the
    fp32 fmaf chain, and every answer of the fast route carries a certificate (qstatus bit2 when it cannot be given — also for
    a query with a non-finite value or one that rounds to a bf16 inf: such queries are repeated, then answered by
    `dense_search_exact`; `.stats` of the `PendingSearch`).  xnorm_max: device fp32 [1], >= the largest row norm of x
    (`dense_xnorm_max`, computed here when None).  Everything else as `dense_search`."""
    return _dense_search(_DENSE_BF16X3, x, q, k, id_offset, sel_slack, defer, method, max_retries, xnorm_max)


# ------------------------------------------------------------------------- dense, 8-bit scalar-quantised storage
def dense_sq8_error_constants():
    """(c_q, c_w, c_ad, c_ac, c_b, c_ch, c_abs) of E_q as the certificate kernel was compiled with them
    (csrc/dense_search_sq8.hip).  No GPU needed."""
    return _error_constants("dense_sq8", 7)


def dense_sq8_qmax() -> int:
    """The largest |256 h + l| of the query pre-pass, 127 * 256 + 127 (DENSE_I8_QMAX, csrc/dense_i8_gemm.h)."""
    return int(_lib.load().rc_dense_sq8_qmax())


def dense_sq8_error_bound(D: int, alpha, w1, b1, qnorm, c1, xmax):
    """E_q of the certificate of `dense_search_sq8` (include/repconc_hip.h, rc_dense_sq8_search_q; derivation in the header
    comment of csrc/dense_search_sq8.hip): the bound on |s~ - s| between the int8 screen and the fmaf chain.  alpha: the
    query's quantisation step, w1 = sum_d |fl(q_d step_d)|, b1 = sum_d |q_d mid_d|, qnorm = ||q||_2, c1 >= the largest
    sum_d |c'_d| of a row, xmax >= the largest norm of a decoded row.  The constants are the library's.  Plain float / numpy
    arithmetic: scalars or arrays."""
    c_q, c_w, c_ad, c_ac, c_b, c_ch, c_abs = dense_sq8_error_constants()
    dpad = float((int(D) + 15) // 16 * 16)
    rel = c_q * alpha * c1 + 2.0 ** -24 * (c_w * w1 + c_ad * alpha * D + c_ac * alpha * c1 + c_b * b1
                                          + c_ch * (dpad + 1.0) * qnorm * xmax)
    return (rel + c_abs * 2.0 ** -149 * (dpad + dpad ** 0.5 * qnorm + c1 + 1.0)) * (1.0 + 2.0 ** -20)


def _dense_sq8_dec(x8: torch.Tensor, dec: torch.Tensor) -> torch.Tensor:
    if dec.shape != (2, x8.shape[1]):
        raise ValueError("dense_search_sq8: dec must be [2, D]: the steps, then the mids")
    _need_cuda(dec)
    return dec.to(x8.device, torch.float32).contiguous()


def _dense_sq8_front(name: str, x8, dec, q, k, cstat):
    """The checked (x8, dec, cstat) of `dense_search_sq8` / `dense_search_l2_sq8`; a missing cstat is computed here."""
    if x8.dim() == 2 and dec.shape != (2, x8.shape[1]):
        raise ValueError(f"{name}: dec must be [2, D]: the steps, then the mids")
    x8, _ = _dense_sq8_args(x8, q, k)
    dec = _dense_sq8_dec(x8, dec)
    if cstat is None:
        # up to DENSE_EXACT_MAX_N rows the library takes the exact route and never reads the statistics
        cstat = dense_sq8_cstat(x8, dec) if x8.shape[0] > DENSE_EXACT_MAX_N else torch.zeros((2,), device=x8.device)
    _need_cuda(cstat)
    if cstat.shape != (2,):
        raise ValueError(f"{name}: cstat must be [2]: C1 and X (dense_sq8_cstat)")
    return x8, dec, cstat.to(x8.device, torch.float32).contiguous()


def dense_sq8_decode(x8: torch.Tensor, dec: torch.Tensor, rows_per_step: int = 1 << 16) -> torch.Tensor:
    """The decoded corpus, fp32 [N, D]: x^ = fmaf(c', step, mid) with one rounding (rc_dense_sq8_decode) — the rows whose
    `dense_search` IS `dense_search_sq8`."""
    x8, _ = _dense_sq8_args(x8, x8.new_zeros((0, x8.shape[1]), dtype=torch.float32), 1)
    dec = _dense_sq8_dec(x8, dec)
    N, D = x8.shape
    out = torch.empty((N, D), dtype=torch.float32, device=x8.device)
    if N:
        lib, h, s, _ = _ctx(x8)
        for r0 in range(0, N, rows_per_step):
            n = min(rows_per_step, N - r0)
            _lib.check(lib.rc_dense_sq8_decode(h, _p(x8[r0:]), x8.stride(0), n, D, _p(dec), _p(out[r0:]), s),
                       "rc_dense_sq8_decode", h)
    return out


def _sq8_decode_cpu(codes: torch.Tensor, dec: torch.Tensor) -> torch.Tensor:
    """fmaf(c', step, mid) with its single rounding, in torch operators (the CPU device): the product is exact in fp64 (8 + 24
    significant bits), the sum is rounded to odd there (TwoSum finds whether it was inexact), and fp64 -> fp32 of a value rounded
    to odd is the correctly rounded fp32 of the exact sum."""
    p, mid = codes.double() * dec[0].double(), dec[1].double().expand(codes.shape)
    s = p + mid
    b = s - p
    err = (p - (s - b)) + (mid - b)                                 # TwoSum: p + mid = s + err exactly
    even = (s.view(torch.int64) & 1) == 0
    odd = torch.nextafter(s, torch.where(err > 0, torch.inf, -torch.inf).to(s.dtype))
    return torch.where((err != 0) & even, odd, s).float()           # inexact and even: the odd neighbour


def dense_sq8_cstat(x8: torch.Tensor, dec: torch.Tensor, rows_per_step: int = 1 << 16) -> torch.Tensor:
    """Device fp32 [2]: C1 = the largest sum_d |c'_d| of a row of `x8` (an integer below 2^24: exact) and X >= the largest
    Euclidean norm of a decoded row (fp64 sums over the fp64 decode, pushed upwards by 2^-20, which covers both the decode's
    fp32 rounding and the conversion): the `cstat` of `dense_search_sq8`.  No host synchronisation."""
    step, mid = dec[0].double(), dec[1].double()
    c1 = torch.zeros((), dtype=torch.float64, device=x8.device)
    xx = torch.zeros((), dtype=torch.float64, device=x8.device)
    for r0 in range(0, x8.shape[0], rows_per_step):
        c = x8[r0:r0 + rows_per_step].double()
        c1 = torch.maximum(c1, c.abs().sum(1).max())
        xx = torch.maximum(xx, (c * step + mid).square_().sum(1).max())
    return torch.stack([c1, xx.sqrt() * (1.0 + 2.0 ** -20)]).float()


def dense_search_sq8_exact(x8: torch.Tensor, dec: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0):
    """The same answer as `dense_search_sq8` by the route that cannot fail (rc_dense_sq8_search_exact)."""
    return _dense_search_exact(_DENSE_SQ8, x8, q, k, id_offset, _dense_sq8_dec(x8, dec))


def dense_sq8_scores(x8: torch.Tensor, dec: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """The raw approximate scores s~ [nq, N] of the int8 matrix-core screen (rc_dense_sq8_scores): a test hook, never a
    result."""
    return _dense_scores(_DENSE_SQ8, "dense_sq8_scores", x8, q, dec)


def dense_search_sq8(x8: torch.Tensor, dec: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0,
                     sel_slack: Optional[float] = None, defer: bool = False, method: str = "auto", max_retries: int = 2,
                     cstat: Optional[torch.Tensor] = None, stats: Optional[dict] = None):
    """Exact top-k inner-product search of `q` [nq, D] against a corpus of 8-bit scalar-quantiser codes (faiss
    IndexScalarQuantizer, QT_8bit): `x8` [N, D] int8 holds c - 128, `dec` [2, D] fp32 the steps and the mids.  A row decodes
    to fmaf(c', step, mid) and the scores are the fp32 fmaf chain over d ascending over the decoded values: ids and score
    bits equal `dense_search(dense_sq8_decode(x8, dec), q, k)`.  The int8 matrix cores only screen (two int8 limbs of
    q * step per query); candidates are rescored by the chain and every answer of the fast route carries a certificate
    (qstatus bit2 when it cannot be given — also for a non-finite or huge query value: such queries are repeated, then
    answered by `dense_search_sq8_exact`; `.stats` of the `PendingSearch`).  cstat: device fp32 [2] (`dense_sq8_cstat`,
    computed here when None).  stats (measurement): receives "survivors", a list of int32 device tensors (one per library
    call of the FIRST pass) with the rows of every query that passed the screen.  1 <= D <= 65536.  Everything else as
    `dense_search`."""
    x8, dec, cstat = _dense_sq8_front("dense_search_sq8", x8, dec, q, k, cstat)
    return _dense_search(_DENSE_SQ8, x8, q, k, id_offset, sel_slack, defer, method, max_retries, dec=dec, cstat=cstat,
                         stats=stats)


# ---------------------------------------------------------------------------------------------------- dense, L2 metric
def dense_row_sqnorms(x: torch.Tensor, rows_per_step: int = 1 << 16) -> torch.Tensor:
    """Device fp32 [N]: the squared Euclidean norm of every row of the floating-point matrix `x`, an fp64 sum rounded to
    nearest (+inf if it exceeds fp32): the `xsq` of `dense_search_l2`.  No host synchronisation."""
    if not x.dtype.is_floating_point or x.dim() != 2:
        raise ValueError("dense_row_sqnorms: a floating-point matrix")
    out = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    for r0 in range(0, x.shape[0], rows_per_step):
        out[r0:r0 + rows_per_step] = x[r0:r0 + rows_per_step].double().square_().sum(1)
    return out


def _dense_l2_xnorm_max(xsq: torch.Tensor) -> torch.Tensor:
    """Device fp32 [1] >= the largest row norm, from the rounded squared norms (the true square is at most xsq (1 + 2^-24); the
    2^-20 covers that, the square root and the conversion).  No host synchronisation."""
    return (xsq.max().double().sqrt() * (1.0 + 2.0 ** -20)).float().reshape(1)


def dense_l2_error_constants():
    """(c_rel, c_flush, c_under) of E_q as the certificate kernel was compiled with them (csrc/dense_search_l2.hip)."""
    return _error_constants("dense_l2", 3)


def dense_l2_error_bound(D: int, qnorm, xmax):
    """E = 2 D_pad 2^-24 (||q|| + X)^2 + 4 * 2^-126 sqrt(D_pad) (||q|| + X) + 4 D_pad 2^-149, D_pad = D rounded up to 16: the
    bound on |sigma - ||q||^2 + d| between the L2 screen sigma = fmaf(2, dot, -xsq) and the chain d that the certificate of
    `dense_search_l2` uses; derivation in the header comment of csrc/dense_search_l2.hip.  The constants are the library's.
    Plain float / numpy arithmetic: `qnorm`, `xmax` scalars or arrays."""
    c_rel, c_flush, c_under = dense_l2_error_constants()
    dpad = (int(D) + 15) // 16 * 16
    r = qnorm + xmax
    return c_rel * dpad * 2.0 ** -24 * r * r + c_flush * dpad ** 0.5 * r + c_under * dpad


def dense_l2_scores(x: torch.Tensor, q: torch.Tensor, xsq: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The raw screen values sigma [nq, N] = fmaf(2, dot(q, x_n), -xsq[n]) of the L2 search (rc_dense_l2_scores): a test hook,
    never a result."""
    return _dense_scores(_DENSE_L2, "dense_l2_scores", x, q, xsq=xsq)


def dense_search_l2_exact(x: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0, *, rows: Optional[torch.Tensor] = None,
                          check_rows: bool = True):
    """The same answer as `dense_search_l2` by the route that cannot fail (rc_dense_l2_search_exact): full rows of distances
    from the vector-ALU kernel and a radix select of the min(k, N) nearest.  rows, check_rows: as `dense_search`
    (rc_dense_l2_search_rows_exact)."""
    return _dense_search_exact(_DENSE_L2, x, q, k, id_offset, None, rows, check_rows)


def dense_search_l2(x: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0, sel_slack: Optional[float] = None,
                    defer: bool = False, method: str = "auto", max_retries: int = 2, xsq: Optional[torch.Tensor] = None,
                    xnorm_max: Optional[torch.Tensor] = None, *, rows: Optional[torch.Tensor] = None, check_rows: bool = True):
    """Exact top-k squared-Euclidean search of `q` [nq, D] against the fp32 corpus `x` [N, D] (faiss.IndexFlatL2,
    evaluate_repconc.py:102, run_warmup.py:102,107).  Returns (distances [nq, k] fp32, ids [nq, k] int64 = row + id_offset),
    sorted (distance asc, id asc); +inf / -1 past N.  A distance is the fp32 chain t = q_j - x_j, acc = fmaf(t, t, acc) over j
    ascending (include/repconc_hip.h), bit for bit, never negative.  The matrix cores only screen with the expanded form;
    candidates are rescored by the chain and every answer of the fast route carries a certificate (qstatus bit2 when it cannot
    be given: such queries are repeated, then answered by `dense_search_l2_exact`; `.stats` of the `PendingSearch`).
    xsq: device fp32 [N], the rows' squared norms (`dense_row_sqnorms`); xnorm_max: device fp32 [1] >= the largest row norm;
    both computed here when None, and neither is read up to DENSE_EXACT_MAX_N rows.  Everything else as `dense_search`, the
    subset search (rows, check_rows) included: xsq stays the [N] norms of ALL rows, read at rows[i], xnorm_max their bound."""
    return _dense_search_l2(_DENSE_L2, x, q, k, id_offset, sel_slack, defer, method, max_retries, xsq, xnorm_max, rows=rows,
                            check_rows=check_rows)


def _dense_search_l2(v: _DenseVariant, x, q, k, id_offset, sel_slack, defer, method, max_retries, xsq, xnorm_max,
                     dec=None, cstat=None, stats=None, rows=None, check_rows=True):
    """The front of the four L2 searches: a missing xnorm_max comes from the squared norms, which are then computed once.
    Over int8 codes (`dec` given) the norms are those of the decoded rows and the certificate reads `cstat`, not xnorm_max."""
    if not 1 <= int(k) <= DENSE_MAX_K:
        raise ValueError(f"dense search: k must be in [1, {DENSE_MAX_K}]")
    missing = xnorm_max is None if dec is None else xsq is None
    searched = rows.numel() if isinstance(rows, torch.Tensor) else x.shape[0] if x.dim() == 2 else 0      # the rows the route sees
    if missing and searched > DENSE_EXACT_MAX_N and method == "auto" and x.is_cuda:
        if xsq is None:
            xsq = dense_row_sqnorms(x) if dec is None else dense_sq8_row_sqnorms(x, dec)
        if dec is None:
            xnorm_max = _dense_l2_xnorm_max(xsq)
    return _dense_search(v, x, q, k, id_offset, sel_slack, defer, method, max_retries, xnorm_max, xsq, dec, cstat, stats, rows,
                         check_rows)


# ---------------------------------------------------------------------------------------- dense, L2 metric, fp16 storage
def dense_l2_f16_error_constants():
    """(c_rel, max_d) of E_q as the certificate kernel was compiled with them (csrc/dense_search_l2_f16.hip)."""
    return _error_constants("dense_l2_f16", 2)


def dense_l2_f16_error_bound(D: int, qnorm, xmax):
    """E = 2.5 D_pad 2^-24 (||q|| + X)^2, D_pad = D rounded up to 16: the bound on |sigma - ||q||^2 + d| between the fp16 L2
    screen sigma = fmaf(2, dot, -xsq), dot ANY fp32 accumulation of the D exact products of finite fp16 values, and the chain d
    that the certificate of `dense_search_l2_f16` uses, for D <= 65536; derivation in the header comment of
    csrc/dense_search_l2_f16.hip.  The constant is the library's.  Plain float / numpy arithmetic: scalars or arrays."""
    c_rel, _ = dense_l2_f16_error_constants()
    dpad = (int(D) + 15) // 16 * 16
    r = qnorm + xmax
    return c_rel * dpad * 2.0 ** -24 * r * r


def dense_l2_f16_scores(x16: torch.Tensor, q16: torch.Tensor, xsq: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The raw screen values sigma [nq, N] = fmaf(2, dot(q, x_n), -xsq[n]) of the fp16 L2 search (rc_dense_l2_f16_scores): a
    test hook, never a result."""
    return _dense_scores(_DENSE_L2_F16, "dense_l2_f16_scores", x16, q16, xsq=xsq)


def dense_search_l2_f16_exact(x16: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0, *,
                              rows: Optional[torch.Tensor] = None, check_rows: bool = True):
    """The same answer as `dense_search_l2_f16` by the route that cannot fail (rc_dense_l2_f16_search_exact).  rows,
    check_rows: as `dense_search` (rc_dense_l2_f16_search_rows_exact)."""
    return _dense_search_exact(_DENSE_L2_F16, x16, q, k, id_offset, None, rows, check_rows)


def dense_search_l2_f16(x16: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0, sel_slack: Optional[float] = None,
                        defer: bool = False, method: str = "auto", max_retries: int = 2, xsq: Optional[torch.Tensor] = None,
                        xnorm_max: Optional[torch.Tensor] = None, *, rows: Optional[torch.Tensor] = None,
                        check_rows: bool = True):
    """Exact top-k squared-Euclidean search of `q` [nq, D] against the FINITE fp16 corpus `x16` [N, D] (faiss.IndexFlatL2 with
    useFloat16).  The queries are rounded to fp16 as `dense_search_f16` rounds them (to nearest even, no range check: a value of
    magnitude >= 65520 becomes inf, such a query gets no certificate and the exact route gives it the chain's inf / NaN
    distances).  A distance is the chain of `dense_search_l2` over the widened values: ids and distance bits equal
    `dense_search_l2(x16.float(), q.half().float(), k)`.  The f16 matrix cores only screen; candidates are rescored by the chain
    and every answer of the fast route carries a certificate (qstatus bit2 when it cannot be given: such queries are repeated,
    then answered by `dense_search_l2_f16_exact`; `.stats` of the `PendingSearch`).  xsq: device fp32 [N], the squared norms of
    the fp16 rows (`dense_row_sqnorms`); xnorm_max: device fp32 [1] >= the largest row norm; both computed here from the fp16
    corpus when None, and neither is read up to DENSE_EXACT_MAX_N rows.  Everything else as `dense_search_l2`, rows and
    check_rows included."""
    if x16.dtype != torch.float16:       # before any norm is computed from it
        raise ValueError("dense_search_l2_f16: the corpus must be float16 (FlatL2F16Index rounds and checks it)")
    return _dense_search_l2(_DENSE_L2_F16, x16, q, k, id_offset, sel_slack, defer, method, max_retries, xsq, xnorm_max,
                            rows=rows, check_rows=check_rows)


# ------------------------------------------------------------------------ dense, L2 metric, fp32 corpus, bf16x3 screen
def dense_l2_bf16x3_error_constants():
    """(c_sum, c_split, c_flush, c_under) of E_q as the certificate kernel was compiled with them
    (csrc/dense_search_l2_bf16x3.hip)."""
    return _error_constants("dense_l2_bf16x3", 4)


def dense_l2_bf16x3_error_bound(D: int, qnorm, xmax):
    """E = (5 D_pad 2^-24 + 2 * 2^-16) (||q|| + X)^2 + 4 * 2^-126 sqrt(D_pad) (||q|| + X) + 8 D_pad 2^-149, D_pad = D rounded
    up to 16: the bound on |sigma~ - ||q||^2 + d| between the bf16x3 L2 screen sigma~ = fmaf(2, s~, -xsq) (s~ any fp32
    accumulation of the 3 D products of the round-to-nearest-even bf16 splits) and the chain d that the certificate of
    `dense_search_l2_bf16x3` uses, for D <= 65536; derivation in the header comment of csrc/dense_search_l2_bf16x3.hip.  The
    constants are the library's.  Plain float / numpy arithmetic: `qnorm`, `xmax` scalars or arrays."""
    c_sum, c_split, c_flush, c_under = dense_l2_bf16x3_error_constants()
    dpad = (int(D) + 15) // 16 * 16
    r = qnorm + xmax
    return (c_sum * dpad * 2.0 ** -24 + c_split * 2.0 ** -16) * r * r + c_flush * dpad ** 0.5 * r + c_under * dpad


def dense_l2_bf16x3_scores(x: torch.Tensor, q: torch.Tensor, xsq: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The raw screen values sigma~ [nq, N] = fmaf(2, s~(q, x_n), -xsq[n]) of the bf16x3 L2 search
    (rc_dense_l2_bf16x3_scores): a test hook, never a result."""
    return _dense_scores(_DENSE_L2_BF16X3, "dense_l2_bf16x3_scores", x, q, xsq=xsq)


def dense_search_l2_bf16x3(x: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0, sel_slack: Optional[float] = None,
                           defer: bool = False, method: str = "auto", max_retries: int = 2,
                           xsq: Optional[torch.Tensor] = None, xnorm_max: Optional[torch.Tensor] = None):
    """`dense_search_l2` with the screen on the bf16 matrix cores: the same ids and distance bits for a FINITE fp32 corpus `x`
    whose values round to finite bf16 (magnitude < 2^128 - 2^119; `FlatL2Bf16x3Index` checks it) and any queries.  Nothing is
    rounded in the result: the screen's three-term bf16 split only chooses candidates, which are rescored by the chain of
    `dense_search_l2`, and every answer of the fast route carries a certificate (qstatus bit2 when it cannot be given, also
    for a query with a non-finite value or one that rounds to a bf16 inf: such queries are repeated, then answered by
    `dense_search_l2_exact`; `.stats` of the `PendingSearch`).  xsq, xnorm_max and everything else as `dense_search_l2`."""
    return _dense_search_l2(_DENSE_L2_BF16X3, x, q, k, id_offset, sel_slack, defer, method, max_retries, xsq, xnorm_max)


# ----------------------------------------------------------------- dense, L2 metric, 8-bit scalar-quantised storage
def dense_l2_sq8_error_constants():
    """(c_q, c_w, c_ad, c_ac, c_b, c_r, c_abs, max_r, max_e) of E_q as the certificate kernel was compiled with them
    (csrc/dense_search_l2_sq8.hip).  No GPU needed."""
    return _error_constants("dense_l2_sq8", 9)


def dense_l2_sq8_error_bound(D: int, alpha, w1, b1, qnorm, c1, xmax):
    """E_q of the certificate of `dense_search_l2_sq8` (include/repconc_hip.h, rc_dense_l2_sq8_search_q; derivation in the
    header comment of csrc/dense_search_l2_sq8.hip): the bound on |sigma - ||q||^2 + d| between the int8 L2 screen sigma =
    fmaf(2, s~, -xsq) and the chain d.  Arguments as `dense_sq8_error_bound`; +inf where (qnorm + xmax)^2 or E_q itself leaves
    the range in which nothing overflows.  The constants are the library's.  numpy arithmetic: scalars or arrays."""
    c_q, c_w, c_ad, c_ac, c_b, c_r, c_abs, max_r, max_e = dense_l2_sq8_error_constants()
    dpad = float((int(D) + 15) // 16 * 16)
    r = np.asarray(qnorm, dtype=np.float64) + xmax
    R = r * r
    rel = c_q * alpha * c1 + 2.0 ** -24 * (c_w * w1 + c_ad * alpha * D + c_ac * alpha * c1 + c_b * b1 + c_r * (dpad + 5.0) * R)
    e = (rel + c_abs * 2.0 ** -149 * (dpad + dpad ** 0.5 * qnorm + c1 + 3.0)) * (1.0 + 2.0 ** -20)
    return np.where((R < max_r) & (e < max_e), e, np.where(np.isnan(e), e, np.inf))


def dense_sq8_row_sqnorms(x8: torch.Tensor, dec: torch.Tensor, rows_per_step: int = 1 << 16) -> torch.Tensor:
    """fp32 [N] on the device of `x8`: the squared Euclidean norm of every DECODED row fmaf(c', step, mid), an fp64 sum rounded
    to nearest (the rule of `dense_row_sqnorms`): the `xsq` of `dense_search_l2_sq8`.  On the GPU a kernel computes it from
    the codes (rc_dense_sq8_row_sqnorms; the decoded corpus is never written); on the CPU, torch operators (the decode's one
    rounding through an fp64 sum rounded to odd).  No host synchronisation."""
    if x8.dim() != 2 or x8.dtype != torch.int8 or dec.shape != (2, x8.shape[1]):
        raise ValueError("dense_sq8_row_sqnorms: int8 codes [N, D] and dec [2, D]")
    N, D = x8.shape
    dec = dec.to(x8.device, torch.float32).contiguous()
    out = torch.empty((N,), dtype=torch.float32, device=x8.device)
    if x8.is_cuda:
        if x8.stride(1) != 1 or (N > 1 and x8.stride(0) < D):
            x8 = x8.contiguous()
        if N:
            lib, h, s, _ = _ctx(x8)
            _lib.check(lib.rc_dense_sq8_row_sqnorms(h, _p(x8), x8.stride(0), N, D, _p(dec), _p(out), s),
                       "rc_dense_sq8_row_sqnorms", h)
        return out
    for r0 in range(0, N, rows_per_step):
        out[r0:r0 + rows_per_step] = _sq8_decode_cpu(x8[r0:r0 + rows_per_step], dec).double().square_().sum(1)
    return out


def dense_search_l2_sq8_exact(x8: torch.Tensor, dec: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0):
    """The same answer as `dense_search_l2_sq8` by the route that cannot fail (rc_dense_l2_sq8_search_exact)."""
    return _dense_search_exact(_DENSE_L2_SQ8, x8, q, k, id_offset, _dense_sq8_dec(x8, dec))


def dense_l2_sq8_scores(x8: torch.Tensor, dec: torch.Tensor, q: torch.Tensor, xsq: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The raw screen values sigma [nq, N] = fmaf(2, s~(q, n), -xsq[n]) of the int8 L2 search (rc_dense_l2_sq8_scores): a test
    hook, never a result."""
    return _dense_scores(_DENSE_L2_SQ8, "dense_l2_sq8_scores", x8, q, dec, xsq)


def dense_search_l2_sq8(x8: torch.Tensor, dec: torch.Tensor, q: torch.Tensor, k: int, id_offset: int = 0,
                        sel_slack: Optional[float] = None, defer: bool = False, method: str = "auto", max_retries: int = 2,
                        xsq: Optional[torch.Tensor] = None, cstat: Optional[torch.Tensor] = None,
                        stats: Optional[dict] = None):
    """Exact top-k squared-Euclidean search of `q` [nq, D] against a corpus of 8-bit scalar-quantiser codes (faiss
    IndexScalarQuantizer, QT_8bit, METRIC_L2): the store of `dense_search_sq8` under the distance of `dense_search_l2`.  A
    distance is the chain t = q_j - x^_j, acc = fmaf(t, t, acc) over the decoded values x^ = fmaf(c', step, mid): ids and
    distance bits equal `dense_search_l2(dense_sq8_decode(x8, dec), q, k)`; sorted (distance asc, id asc), +inf / -1 past N.
    The int8 matrix cores only screen with sigma = fmaf(2, s~, -xsq); candidates are rescored by the chain and every answer of
    the fast route carries a certificate (qstatus bit2 when it cannot be given: such queries are repeated, then answered by
    `dense_search_l2_sq8_exact`; `.stats` of the `PendingSearch`).  xsq: device fp32 [N], the squared norms of the decoded rows
    (`dense_sq8_row_sqnorms`); cstat: device fp32 [2] (`dense_sq8_cstat`); both computed here when None, and neither is read up
    to DENSE_EXACT_MAX_N rows.  stats and everything else as `dense_search_sq8`."""
    x8, dec, cstat = _dense_sq8_front("dense_search_l2_sq8", x8, dec, q, k, cstat)
    return _dense_search_l2(_DENSE_L2_SQ8, x8, q, k, id_offset, sel_slack, defer, method, max_retries, xsq, None, dec, cstat,
                            stats)
