"""Exact inner-product index resident in HBM: the GPU `faiss.IndexFlatIP` of the reference's dense evaluation,
models/dense/evaluate_dense.py:84-129 (useFloat16 = False by default, `storage="float16"` for useFloat16 = True).

`FlatIPIndex` is duck-typed like that object (`d`, `ntotal`, `metric_type`, `is_trained`, `add`, `reset`, `search`) and
searches with `ops.dense_search` (csrc/dense_search.hip): scores are the fp32 fmaf chain over d ascending, bit for bit,
ties broken by the lower id.  The vectors live in ONE fp32 [capacity, d] device tensor appended to in place: the first
`add` allocates exactly, later growth is 1.5x (`reserve` sets the capacity up front).

`storage="float16"`: `add` rounds every value to IEEE fp16 (round to nearest even) and keeps fp16, half the bytes; `search`
rounds the queries the same way and answers with `ops.dense_search_f16` (csrc/dense_search_f16.hip): the scores are the same
fmaf chain over the rounded values, bit for bit what the fp32 index returns for `x.half().float()`, `q.half().float()`.

`screen="bf16x3"` (float32 storage only): the vectors stay fp32 and `search` returns the same ids and score bits as the default
index, but the candidates are chosen on the bf16 matrix cores by `ops.dense_search_bf16x3` (csrc/dense_search_bf16x3.hip).
`add` then refuses values whose bf16 rounding is not finite (magnitude >= 2^128 - 2^119, inf, NaN).

`FlatL2Index` / `FlatL2F16Index` / `FlatL2Bf16x3Index`: the squared-Euclidean indexes (`faiss.IndexFlatL2`: fp32 storage, fp16
storage, fp32 storage with the bf16x3 screen), classes of their own beside `FlatIPIndex`.

`FlatSQ8Index` / `FlatL2SQ8Index`: the inner-product and the squared-Euclidean index over 8-bit scalar-quantiser codes
(`faiss.IndexScalarQuantizer`, QT_8bit), one byte per dimension; they share the store and its training (`_SQ8Store`).

Subset search: `search(x, k, params=SearchParameters(sel=...))` with the selectors of `repconc_amd.selector` answers over the
selected ids only, in place, with the ids and score bits the same index would return had it been given just those vectors
(and their ids).  Served by the fp32- and fp16-storage indexes of both metrics under their own screens; the bf16x3 screens and
the int8 stores refuse a selector.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops
from .index import METRIC_INNER_PRODUCT, METRIC_L2, _as_device, _as_f32_tensor
from .selector import IDSelectorRange, SearchParameters


class _FlatIndex:
    """What the flat indexes share: the device, ONE [capacity, d] tensor of vectors appended to in place (the first `add`
    allocates exactly, later growth is 1.5x), the front end of `add` (`_rows`), `reset`, and `search` / `search_async` around
    the subclass's `_enqueue`."""
    PAD = float("-inf")          # the value of the slots past ntotal
    SUBSET = True                # `search(..., params=)` takes a selector (the kernels of this storage and screen read a row list)

    def _init_store(self, d: int, device, dtype) -> None:
        self._dtype = dtype
        self.device = _as_device(device)
        self.d = int(d)
        self.is_trained = True
        self.ntotal = 0
        self.id_offset = 0       # global id of local row 0
        self.sel_slack = ops.DENSE_SEL_SLACK
        self.last_search = None
        self._x = torch.empty((0, self.d), dtype=self._dtype, device=self.device)
        # screened searches: device fp32 [1] >= the largest row norm held (the search's certificate)
        self._xnorm_max = None

    @property
    def xb(self) -> torch.Tensor:
        """[ntotal, d] view of the stored vectors, in the storage type."""
        return self._x[: self.ntotal]

    def reserve(self, n: int) -> None:
        """Capacity for `n` rows in total (the rows held so far are kept)."""
        if n > self._x.shape[0]:
            grown = torch.empty((int(n), self.d), dtype=self._dtype, device=self.device)
            grown[: self.ntotal] = self._x[: self.ntotal]
            self._x = grown

    def _grow_for(self, need: int) -> None:
        if need > self._x.shape[0]:
            self.reserve(need if self.ntotal == 0 else max(need, int(self._x.shape[0] * 1.5)))

    def _rows(self, x) -> torch.Tensor:
        """The argument of `add` as a tensor (numpy -> fp32), checked to be [n, d]."""
        xt = _as_f32_tensor(x)
        if xt.dim() != 2 or xt.shape[1] != self.d:
            raise ValueError(f"add: expected [n, {self.d}] vectors, got {tuple(xt.shape)}")
        return xt

    def _rounded_f16(self, xt: torch.Tensor) -> torch.Tensor:
        """The rows of an `add` on the device, rounded to fp16 and checked before anything is stored or grown; one host read."""
        xt = xt.to(self.device).to(torch.float16)
        if xt.shape[0] and not bool(torch.isfinite(xt).all()):
            raise ValueError("add: float16 storage needs finite values of magnitude < 65520 (fp16 rounds the rest to inf)")
        return xt

    def _finite_bf16(self, xt: torch.Tensor) -> torch.Tensor:
        """The rows of an `add` on the device in fp32, checked to round to finite bf16 before anything is stored or grown; one
        host read."""
        xt = xt.to(self.device, torch.float32)
        if xt.shape[0] and not bool(torch.isfinite(xt.to(torch.bfloat16)).all()):
            raise ValueError("add: the bf16x3 screen needs finite values of magnitude < 2^128 - 2^119 (bf16 rounds the rest to inf)")
        return xt

    def reset(self) -> None:
        self.ntotal = 0
        self._x = torch.empty((0, self.d), dtype=self._dtype, device=self.device)
        self._xnorm_max = None

    def search(self, x, k: int, params: Optional[SearchParameters] = None):
        """(scores or distances [nq, k], ids [nq, k]); numpy in -> numpy out (evaluate_dense.py:74), CUDA tensors in -> CUDA
        tensors out (faiss.contrib.torch_utils).  float16 storage rounds the queries to fp16 without a range check: a query
        value of magnitude >= 65520 becomes inf (`ops.dense_search_f16`).
        params: None or `SearchParameters()` is the whole store.  `SearchParameters(sel=...)` (faiss's `params=`) searches
        only the ids the selector holds: ids and score bits are those of an index holding just those vectors under those
        ids, padding past their number included.  An `IDSelectorRange` searches the matching slice of the store as a view;
        every other selector becomes a row list (`sel.rows`, cached on the selector; building it reads the device once)
        that the kernels follow in place (`ops.dense_search(rows=...)`)."""
        return self.search_async(x, k, params)()

    def _selector(self, params):
        """The selector of `params`, or None for the whole store; ValueError where this index serves none."""
        if params is None:
            return None
        if not isinstance(params, SearchParameters):
            raise ValueError("search: params must be a SearchParameters or None")
        if params.sel is not None and not self.SUBSET:
            raise ValueError(f"{type(self).__name__}: no subset search (params.sel) under this storage or screen; the fp32- and "
                             "fp16-storage indexes with their own screens serve it")
        return params.sel

    def search_async(self, x, k: int, params: Optional[SearchParameters] = None):
        """Enqueue the search and return a callable that yields what `search` returns; nothing synchronises with the host
        until it is called (`batch_dense_search` enqueues every batch first; a selector other than a range builds its row
        list on first use, which does read the device)."""
        sel = self._selector(params)
        as_numpy = not isinstance(x, torch.Tensor)
        q = _as_f32_tensor(x).to(self.device, torch.float32, non_blocking=True)
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"search: expected [nq, {self.d}] queries, got {tuple(q.shape)}")
        k = int(k)
        lo, hi, rows = 0, self.ntotal, None
        if isinstance(sel, IDSelectorRange):
            lo, hi = sel.span(self.ntotal, self.id_offset)
        elif sel is not None and self.ntotal:
            rows = sel.rows(self.ntotal, self.id_offset, self.device)
            hi = rows.numel()                # (only "is anything selected" is read from it below)
        if hi == lo or q.shape[0] == 0:
            scores = torch.full((q.shape[0], k), self.PAD, dtype=torch.float32, device=self.device)
            ids = torch.full((q.shape[0], k), -1, dtype=torch.int64, device=self.device)
            pending = ops.PendingSearch(None, scores, ids, None, None, 0.0, 0)
        elif sel is None:
            pending = self._enqueue(q, k)
        elif rows is None:
            pending = self._enqueue(q, k, lo=lo, hi=hi)
        else:
            pending = self._enqueue(q, k, rows=rows)
        self.last_search = pending           # .stats: queries repeated / answered by the exact route

        def finish():
            scores, ids = pending.result()
            if as_numpy:
                return scores.cpu().numpy(), ids.cpu().numpy()
            return scores, ids
        return finish

    def rerank(self, x, cand_ids, k: int):
        """Exact re-ranking of candidate lists (`ops.dense_rerank`, the second stage of faiss.IndexRefineFlat): the `k` best of
        the ids `cand_ids` [nq, kc] of every query by this index's own metric and storage, scored against the stored vectors
        with the bits `search` gives them.  Ids outside [id_offset, id_offset + ntotal) — the -1 holes of an IVF search — are
        skipped; what is missing after them is padded like `search` pads.  numpy in -> numpy out, tensors in -> tensors out."""
        as_numpy = not isinstance(x, torch.Tensor)
        q = _as_f32_tensor(x)
        c = cand_ids if isinstance(cand_ids, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(cand_ids))
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"rerank: expected [nq, {self.d}] queries, got {tuple(q.shape)}")
        if c.dim() != 2 or c.shape[0] != q.shape[0] or c.dtype != torch.int64:
            raise ValueError(f"rerank: expected int64 [{q.shape[0]}, kc] candidate ids, got {c.dtype} {tuple(c.shape)}")
        k = int(k)
        q = q.to(self.device, torch.float32, non_blocking=True)
        c = c.to(self.device, non_blocking=True)
        if self.ntotal == 0 or q.shape[0] == 0:
            if not 1 <= k <= ops.DENSE_MAX_K:
                raise ValueError(f"rerank: k must be in [1, {ops.DENSE_MAX_K}]")
            scores = torch.full((q.shape[0], k), self.PAD, dtype=torch.float32, device=self.device)
            ids = torch.full((q.shape[0], k), -1, dtype=torch.int64, device=self.device)
        else:
            scores, ids = ops.dense_rerank(self.xb, q, c, k, metric=self.metric_type, id_offset=self.id_offset)
        if as_numpy:
            return scores.cpu().numpy(), ids.cpu().numpy()
        return scores, ids


class FlatIPIndex(_FlatIndex):
    STORAGE = {"float32": torch.float32, "float16": torch.float16}
    SCREENS = ("fp32", "bf16x3")

    @classmethod
    def check_options(cls, storage: str, screen: str) -> None:
        """ValueError for an unknown storage or screen, or a combination that does not exist; touches no device."""
        if storage not in cls.STORAGE:
            raise ValueError(f"storage must be one of {sorted(cls.STORAGE)}, got {storage!r}")
        if screen not in cls.SCREENS:
            raise ValueError(f"screen must be one of {list(cls.SCREENS)}, got {screen!r}")
        if screen == "bf16x3" and storage != "float32":
            raise ValueError("screen='bf16x3' needs storage='float32'")

    def __init__(self, d: int, device: Optional[torch.device] = None, storage: str = "float32", screen: str = "fp32"):
        self.check_options(storage, screen)
        self.storage = storage
        self.screen = screen
        self._init_store(d, device, self.STORAGE[storage])
        self.metric_type = METRIC_INNER_PRODUCT
        self._search = ops.dense_search_f16 if storage == "float16" else ops.dense_search_bf16x3 if screen == "bf16x3" \
            else ops.dense_search
        self.SUBSET = screen != "bf16x3"

    def add(self, x) -> None:
        xt = self._rows(x)
        n = xt.shape[0]
        need = self.ntotal + n
        xnorm = None
        if self.storage == "float16":
            xt = self._rounded_f16(xt)
            if n:
                xnorm = ops.dense_f16_xnorm_max(xt)
        elif self.screen == "bf16x3":
            xt = self._finite_bf16(xt)
            if n:
                xnorm = ops.dense_xnorm_max(xt)
        self._grow_for(need)
        self._x[self.ntotal:need] = xt.to(self.device, self._dtype)
        self.ntotal = need
        if xnorm is not None:
            self._xnorm_max = xnorm if self._xnorm_max is None else torch.maximum(self._xnorm_max, xnorm)

    def _enqueue(self, q, k: int, lo: int = 0, hi: Optional[int] = None, rows: Optional[torch.Tensor] = None):
        """The whole store; the rows lo .. hi - 1 as a view (the norm bound of the whole store covers them); or the row list
        `rows` of a selector, valid by construction."""
        more = {} if self._search is ops.dense_search else {"xnorm_max": self._xnorm_max}
        if rows is not None:
            more.update(rows=rows, check_rows=False)
        return self._search(self.xb[lo:hi], q, k, id_offset=self.id_offset + lo, sel_slack=self.sel_slack, defer=True, **more)


class _FlatL2(_FlatIndex):
    """What the L2 indexes share: beside the vectors, their fp32 squared norms in a capacity-sized tensor and a bound of the
    largest norm, both updated by `add` without a host read: the screen's second operand and its certificate's X.  A subclass
    says how `add` stores a row (`_stored`) and which search answers (`_search`)."""
    PAD = float("inf")

    def _init_l2(self, d: int, device, dtype) -> None:
        self._init_store(d, device, dtype)
        self.metric_type = METRIC_L2
        self._xsq = torch.empty((0,), dtype=torch.float32, device=self.device)

    def reserve(self, n: int) -> None:
        """Capacity for `n` rows in total (the rows and norms held so far are kept)."""
        if n > self._x.shape[0]:
            super().reserve(n)
            grown = torch.empty((int(n),), dtype=torch.float32, device=self.device)
            grown[: self.ntotal] = self._xsq[: self.ntotal]
            self._xsq = grown

    def add(self, x) -> None:
        xt = self._rows(x)
        n = xt.shape[0]
        if n == 0:
            return
        need = self.ntotal + n
        xt = self._stored(xt)
        self._grow_for(need)
        self._x[self.ntotal:need] = xt
        xsq = ops.dense_row_sqnorms(xt)
        self._xsq[self.ntotal:need] = xsq
        xnorm = ops._dense_l2_xnorm_max(xsq)
        self._xnorm_max = xnorm if self._xnorm_max is None else torch.maximum(self._xnorm_max, xnorm)
        self.ntotal = need

    def reset(self) -> None:
        super().reset()
        self._xsq = torch.empty((0,), dtype=torch.float32, device=self.device)

    def _enqueue(self, q, k: int, lo: int = 0, hi: Optional[int] = None, rows: Optional[torch.Tensor] = None):
        """As `FlatIPIndex._enqueue`; the norms are sliced with the rows."""
        hi = self.ntotal if hi is None else hi
        more = {} if rows is None else {"rows": rows, "check_rows": False}
        return self._search(self.xb[lo:hi], q, k, id_offset=self.id_offset + lo, sel_slack=self.sel_slack, defer=True,
                            xsq=self._xsq[lo:hi], xnorm_max=self._xnorm_max, **more)


class FlatL2Index(_FlatL2):
    """Exact squared-Euclidean index resident in HBM: the GPU `faiss.IndexFlatL2` the reference names at
    models/repconc/evaluate_repconc.py:102 and train/run_warmup.py:102,107.  Duck-typed like `FlatIPIndex`, fp32 storage and
    the fp32 screen only (no `storage` / `screen` options; fp16 storage is `FlatL2F16Index`, the bf16x3 screen
    `FlatL2Bf16x3Index`).  `search` answers with
    `ops.dense_search_l2` (csrc/dense_search_l2.hip): a distance is the fp32 chain t = q_j - x_j, acc = fmaf(t, t, acc) over j
    ascending, bit for bit, never negative; results are sorted (distance asc, id asc), +inf / -1 past ntotal.  Beside the
    vectors the index keeps their fp32 squared norms in a capacity-sized tensor and a bound of the largest norm, both updated
    by `add` without a host read: the screen's second operand and its certificate's X."""
    _search = staticmethod(ops.dense_search_l2)

    def __init__(self, d: int, device: Optional[torch.device] = None):
        self._init_l2(d, device, torch.float32)

    def _stored(self, xt: torch.Tensor) -> torch.Tensor:
        return xt.to(self.device, torch.float32)


class FlatL2F16Index(_FlatL2):
    """`FlatL2Index` with the vectors stored as IEEE fp16 (`faiss.IndexFlatL2` with useFloat16), half the bytes.  `add` rounds
    every value to fp16 (round to nearest even) and refuses a non-finite value or a magnitude >= 65520 before anything is
    stored (the one host read of an `add`, as `FlatIPIndex(storage="float16")`); `search` rounds the queries the same way,
    without a range check, and answers with `ops.dense_search_l2_f16` (csrc/dense_search_l2_f16.hip): ids and distance bits are
    what `FlatL2Index` returns for `x.half().float()`, `q.half().float()`.  The squared norms kept are those of the rounded
    rows."""
    _search = staticmethod(ops.dense_search_l2_f16)

    def __init__(self, d: int, device: Optional[torch.device] = None):
        self._init_l2(d, device, torch.float16)

    def _stored(self, xt: torch.Tensor) -> torch.Tensor:
        return self._rounded_f16(xt)


class FlatL2Bf16x3Index(_FlatL2):
    """`FlatL2Index` with the candidates chosen on the bf16 matrix cores: the vectors stay fp32 and `search` returns the same
    ids and distance bits, answered by `ops.dense_search_l2_bf16x3` (csrc/dense_search_l2_bf16x3.hip).  `add` refuses values
    whose bf16 rounding is not finite (magnitude >= 2^128 - 2^119, inf, NaN) before anything is stored (the one host read of an
    `add`, as `FlatIPIndex(screen="bf16x3")`)."""
    _search = staticmethod(ops.dense_search_l2_bf16x3)
    SUBSET = False

    def __init__(self, d: int, device: Optional[torch.device] = None):
        self._init_l2(d, device, torch.float32)

    def _stored(self, xt: torch.Tensor) -> torch.Tensor:
        return self._finite_bf16(xt)


SQ8_ROWS_PER_STEP = 1 << 18     # rows that the scalar quantiser's training and the indexes' `add` move and encode at a time


def sq8_train_range(xt: torch.Tensor, device, residual=None) -> tuple:
    """The 8-bit scalar quantiser's training, shared by `FlatSQ8Index` and `IVFFlatIndex(storage="int8")`: xt [n >= 1, d] ->
    (vmin [d], dec [2, d] = step, mid) fp32 on `device`.  vmin / vmax per dimension over the rows (Faiss's RS_minmax with
    argument 0), step = fp32((vmax - vmin) / 255), mid = fp32(vmin + 128.5 step), evaluated in fp64 and rounded once.
    `residual` (the residual form of the IVF index): a function of a chunk of fp32 rows on `device` giving the rows the range
    is fitted on in their place."""
    if xt.shape[0] == 0:
        raise ValueError("train: no rows")
    vmin = torch.full((xt.shape[1],), float("inf"), device=device)
    vmax = -vmin
    for r0 in range(0, xt.shape[0], SQ8_ROWS_PER_STEP):
        part = xt[r0:r0 + SQ8_ROWS_PER_STEP].to(device, torch.float32)
        if residual is not None:
            part = residual(part)
        vmin, vmax = torch.minimum(vmin, part.amin(0)), torch.maximum(vmax, part.amax(0))     # a NaN propagates
    if not bool((torch.isfinite(vmin) & torch.isfinite(vmax)).all()):
        raise ValueError("train: finite values only")
    step = ((vmax.double() - vmin.double()) / 255.0).float()
    mid = (vmin.double() + 128.5 * step.double()).float()
    if not bool((torch.isfinite(step) & torch.isfinite(mid)).all()):
        raise ValueError("train: the range of a dimension exceeds fp32")
    return vmin, torch.stack([step, mid]).contiguous()


def sq8_encode(xt: torch.Tensor, vmin: torch.Tensor, step: torch.Tensor) -> torch.Tensor:
    """The int8 codes c - 128 of fp32 rows on the device of vmin and step: c = clamp(floor((x - vmin) / step), 0, 255) in fp32,
    0 where step = 0; values outside the trained range clamp."""
    c = torch.floor((xt - vmin) / step).clamp_(0.0, 255.0)
    c = torch.where(step == 0, torch.zeros_like(c), c)
    return (c - 128.0).to(torch.int8)


def _sq8_encode_chunks(xt: torch.Tensor, vmin: torch.Tensor, step: torch.Tensor, finite: torch.Tensor,
                      rows_per_step: int = SQ8_ROWS_PER_STEP, shift=None):
    """The rows of an `add`, `rows_per_step` at a time: yields (r0, the int8 codes of rows r0 ..) on the device of vmin and
    step, and ANDs into the device flag `finite` whether every value seen was finite, without a host read (the caller refuses
    the rows after one read; a non-finite value is encoded as 0, int8(NaN) being undefined).  shift(r0, n) (the residual form):
    the fp32 rows subtracted from rows r0 .. r0 + n - 1 before they are encoded; the differences are checked too."""
    for r0 in range(0, xt.shape[0], rows_per_step):
        part = xt[r0:r0 + rows_per_step].to(vmin.device, torch.float32)
        finite &= torch.isfinite(part).all()
        if shift is not None:
            part = part - shift(r0, part.shape[0])
            finite &= torch.isfinite(part).all()                            # finite values whose difference overflows
        yield r0, sq8_encode(torch.nan_to_num(part, nan=0.0, posinf=0.0, neginf=0.0), vmin, step)


class _SQ8Store(_FlatIndex):
    """What the indexes over 8-bit scalar-quantiser codes share: the training, `add` (encode in chunks, refuse non-finite rows
    before anything counts, the certificate's statistics `ops.dense_sq8_cstat` without a host read), `reconstruct_n`, and a
    `reset` that keeps the training.  A subclass says which search answers (`_enqueue`) and may keep more per row
    (`_chunk_added`)."""
    ROWS_PER_STEP = SQ8_ROWS_PER_STEP     # rows that `add` moves and encodes at a time
    SUBSET = False

    def _init_sq8(self, d: int, device, init_store) -> None:
        if not 1 <= int(d) <= ops.DENSE_SQ8_MAX_D:
            raise ValueError(f"{type(self).__name__}: d must be in [1, {ops.DENSE_SQ8_MAX_D}]")
        init_store(d, device, torch.int8)
        self.is_trained = False
        self.vmin = self.step = self.mid = None
        self._dec = None            # [2, d] fp32: step, mid
        self._cstat = None          # [2] fp32: the largest row L1 norm of the codes, a bound of the largest decoded row norm

    def train(self, x) -> None:
        self.vmin, self._dec = sq8_train_range(self._rows(x), self.device)
        self.step, self.mid = self._dec[0], self._dec[1]
        self.is_trained = True

    def _need_trained(self, what: str) -> None:
        if not self.is_trained:
            raise ValueError(f"{what}: the index is not trained (train(x) sets the per-dimension ranges)")

    def encode(self, xt: torch.Tensor) -> torch.Tensor:
        """The int8 codes c - 128 of fp32 rows on the index's device."""
        return sq8_encode(xt, self.vmin, self.step)

    def _chunk_added(self, lo: int, codes: torch.Tensor) -> None:
        """The codes of one chunk of an `add` were written at row `lo` (past ntotal: they do not count yet)."""

    def add(self, x) -> None:
        xt = self._rows(x)
        self._need_trained("add")
        n = xt.shape[0]
        if n == 0:
            return
        need = self.ntotal + n
        self._grow_for(need)
        # the codes are written past ntotal and count only once every value has been seen to be finite (one host read)
        finite = torch.ones((), dtype=torch.bool, device=self.device)
        cstat = torch.zeros((2,), dtype=torch.float32, device=self.device)
        for r0, codes in _sq8_encode_chunks(xt, self.vmin, self.step, finite, self.ROWS_PER_STEP):
            self._x[self.ntotal + r0:self.ntotal + r0 + codes.shape[0]] = codes
            cstat = torch.maximum(cstat, ops.dense_sq8_cstat(codes, self._dec))
            self._chunk_added(self.ntotal + r0, codes)
        if not bool(finite):
            raise ValueError("add: int8 storage needs finite values")
        self.ntotal = need
        self._cstat = cstat if self._cstat is None else torch.maximum(self._cstat, cstat)

    def reset(self) -> None:
        super().reset()
        self._cstat = None

    def reconstruct_n(self, i0: int = 0, ni: int = -1) -> torch.Tensor:
        """fp32 [ni, d]: the decoded rows i0 .. i0 + ni - 1 (ni = -1: up to ntotal), as the search scores them."""
        self._need_trained("reconstruct_n")
        ni = self.ntotal - int(i0) if ni < 0 else int(ni)
        if not (0 <= int(i0) and ni >= 0 and int(i0) + ni <= self.ntotal):
            raise ValueError(f"reconstruct_n: rows [{i0}, {int(i0) + ni}) outside [0, {self.ntotal})")
        return ops.dense_sq8_decode(self._x[int(i0):int(i0) + ni], self._dec)

    def search_async(self, x, k: int, params: Optional[SearchParameters] = None):
        self._selector(params)              # a selector is refused whatever else is missing
        self._need_trained("search")
        return super().search_async(x, k, params)

    def rerank(self, x, cand_ids, k: int):
        raise ValueError(f"{type(self).__name__}: rerank over an int8 store is not served")


class FlatSQ8Index(_SQ8Store):
    """Exact inner-product index over 8-bit scalar-quantiser codes resident in HBM: `faiss.IndexScalarQuantizer(d, QT_8bit,
    METRIC_INNER_PRODUCT)`, one byte per dimension.  Duck-typed like `FlatIPIndex`, plus `train`.

    `train(x)`: per dimension vmin and vmax over the training rows (Faiss's RS_minmax with argument 0), step = fp32((vmax -
    vmin) / 255) and mid = fp32(vmin + 128.5 step), evaluated in fp64 and rounded once.  `add` encodes c = clamp(floor((x -
    vmin) / step), 0, 255) in fp32 (0 where step = 0; values outside the trained range clamp) and stores c - 128 as int8; a
    non-finite value is refused before anything is stored (the one host read of an `add`).  A stored row IS its decoded value
    x^ = fmaf(c - 128, step, mid), the centre of its bin (`reconstruct_n`), and `search` answers with `ops.dense_search_sq8`
    (csrc/dense_search_sq8.hip): ids and score bits are what `FlatIPIndex` returns over `reconstruct_n(0, ntotal)`.  `reset`
    drops the rows and keeps the training.  Beside the codes the index keeps the two statistics of the search's certificate
    (`ops.dense_sq8_cstat`), updated by `add` without a host read.  METRIC_L2 is not served here: `FlatL2SQ8Index` is the
    squared-Euclidean index over the same store."""

    def __init__(self, d: int, device: Optional[torch.device] = None, metric: int = METRIC_INNER_PRODUCT):
        if metric != METRIC_INNER_PRODUCT:
            raise ValueError("FlatSQ8Index: METRIC_INNER_PRODUCT only (the L2 index over int8 codes is FlatL2SQ8Index)")
        self._init_sq8(d, device, self._init_store)
        self.metric_type = METRIC_INNER_PRODUCT

    def _enqueue(self, q, k: int):
        return ops.dense_search_sq8(self.xb, self._dec, q, k, id_offset=self.id_offset, sel_slack=self.sel_slack, defer=True,
                                    cstat=self._cstat)


class FlatL2SQ8Index(_SQ8Store, _FlatL2):
    """Exact squared-Euclidean index over 8-bit scalar-quantiser codes resident in HBM: `faiss.IndexScalarQuantizer(d, QT_8bit)`
    with Faiss's default metric, a class of its own beside `FlatSQ8Index` as `FlatL2F16Index` is beside `FlatIPIndex`.  The
    store, `train`, `add`, `reconstruct_n` and `reset` are `FlatSQ8Index`'s; `search` answers with `ops.dense_search_l2_sq8`
    (csrc/dense_search_l2_sq8.hip): ids and distance bits are what `FlatL2Index` returns over `reconstruct_n(0, ntotal)`,
    sorted (distance asc, id asc), +inf / -1 past ntotal.  Beside the codes and the certificate's statistics the index keeps the
    fp32 squared norms of the decoded rows in a capacity-sized tensor, as the other L2 indexes keep theirs
    (`ops.dense_sq8_row_sqnorms`, computed from the codes chunk by chunk in `add`, no extra host read)."""

    def __init__(self, d: int, device: Optional[torch.device] = None):
        self._init_sq8(d, device, self._init_l2)

    def _chunk_added(self, lo: int, codes: torch.Tensor) -> None:
        self._xsq[lo:lo + codes.shape[0]] = ops.dense_sq8_row_sqnorms(codes, self._dec)

    def _enqueue(self, q, k: int):
        return ops.dense_search_l2_sq8(self.xb, self._dec, q, k, id_offset=self.id_offset, sel_slack=self.sel_slack,
                                       defer=True, xsq=self._xsq[: self.ntotal], cstat=self._cstat)
