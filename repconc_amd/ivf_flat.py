"""Exact IVF index over dense vectors: the GPU `faiss.IndexIVFFlat`, between the flat indexes of `dense_index` (every row, exactly)
and `IVFPQIndex` (the probed cells, lossy codes).  A query is scored exactly against the rows of its `nprobe` best cells only.
The semantics are fixed here, as `ivf.py` fixes them for the PQ index:

  * store: the rows are kept list-major — `xb` [N, d] sorted by coarse cell (fp32, or fp16 with `storage="float16"`),
    `list_off` [nlist + 1], `ids` [N] corpus positions, ascending inside a cell (stable sort).  A document goes to its L2-nearest
    coarse centroid (`coarse_assign`, first minimum) under either metric, the rule of `IVFPQIndex`;
  * probing: `IVFPQIndex.probe`'s rule (`ivf.CoarseProbe`): the `nprobe` cells with the largest <q, c> (METRIC_L2: the largest
    2 <q, c> - ||c||^2), ties at the boundary to the lower cell id, `nprobe` clipped to `nlist`;
  * score: the chain of the flat searches, bit for bit — one fp32 accumulator from +0.0f, d ascending, values widened to fp32,
    s = fmaf(q_d, x_d, s), or t = q_d - x_d, s = fmaf(t, t, s) for L2.  float16 storage rounds rows and queries to fp16 first, as
    `FlatIPIndex(storage="float16")` / `FlatL2F16Index` do, and `add` refuses magnitudes >= 65520;
  * result [nq, k]: inner product: score descending; L2: distance ascending; ties go to the lower CORPUS id; -inf / +inf and -1
    when the probed cells hold fewer than k rows.  Probing every cell returns exactly what the flat index over the same vectors
    returns: ids and score bits.

`search` runs `ops.ivf_flat_search` (csrc/ivf_flat.hip: a list-centric scan, then an exact k-th-score selection — no sampling,
no slack) in chunks of queries whose workspace stays under `MAX_WS_BYTES`.  The one query that route cannot answer is one with
more than 16384 probed rows tied at its k-th score (status bit 1): those queries alone are answered by `_search_exact_probed`,
the exact dense search over their probed rows gathered in corpus-id order (the mirror of `IVFPQIndex._search_exact_probed`).

`storage="int8"` (`faiss.IndexIVFScalarQuantizer`, QT_8bit, the vectors encoded themselves, not their residuals): the store holds
8-bit scalar-quantiser codes, one byte per dimension, and the codec is `FlatSQ8Index`'s (`dense_index.sq8_train_range`,
`sq8_encode`): per dimension vmin, step = fp32((vmax - vmin) / 255), mid = fp32(vmin + 128.5 step), c = clamp(floor((x - vmin) /
step), 0, 255) stored as c - 128, a stored row IS its decoded value x^ = fmaf(c - 128, step, mid).  `train(x)` fits the coarse
centroids and the range from the same rows, `train_sq(x)` the range alone (beside `set_coarse`); `is_trained` needs both, and
`add`, `set_lists`, `search` and `reconstruct_n` before the range exists are ValueErrors.  `add` / `set_lists` take fp32 rows,
assign cells from the values given, refuse non-finite values before anything is stored and clamp values outside the trained
range; the list-major store holds codes, a repeated `add` re-sorts codes and never re-encodes them; `reset` keeps the centroids
and the range.  Queries are fp32 and are not rounded.  The contract of this storage:
  * results equal the flat fp32 index of the same metric (`FlatIPIndex` / `FlatL2Index`) over `reconstruct_n(0, ntotal)`,
    restricted to the probed cells: ids and score bits (`ops.ivf_flat_sq8_search` decodes a value once and runs the same chain);
  * ties go to the lower corpus id; padding is -inf / +inf and -1;
  * under the inner product, probing every cell equals `FlatSQ8Index` trained on the same rows; under L2, probing every cell
    IS the exact L2 search over int8 codes (the flat int8 index does not serve L2).

`storage="int8", by_residual=True` (Faiss's default for that index): a row is stored as the code of its RESIDUAL, r = fp32(x -
coarse[cell]), one fp32 subtraction per value, under the same codec and ONE range (vmin, step, mid) shared by all cells.  The
residuals of clustered rows span less than the rows do, so the same byte buys a finer step.  What changes against the above:
  * `train(x)` fits the centroids first, assigns the training rows (`coarse_assign`) and fits the range on their residuals;
    `train_sq(x)` needs the centroids (ValueError otherwise), assigns x and fits the range on the residuals;
  * `add` encodes against the centroid of the L2-nearest cell of the values given, `set_lists` against the centroid of the
    cell GIVEN; both refuse a non-finite row and a non-finite residual before anything is stored; a repeated `add` still
    re-sorts codes and never re-encodes them (a row's cell never changes);
  * `set_coarse` over stored rows is a ValueError naming `reset`: new centroids would change what the stored codes mean;
  * a stored row IS x^ = fp32(fmaf(c - 128, step, mid) + coarse[cell]): the decode above, then one separate fp32 addition (two
    roundings).  `reconstruct_n` returns exactly x^, and results equal the flat fp32 index of the same metric over
    `reconstruct_n(0, ntotal)` restricted to the probed cells, in ids and score bits (`ops.ivf_flat_sq8r_search` adds the
    centroid once per value on its way into the scan's tile); ties, padding, probing and the limits are unchanged.
Index files, `create_index` / `run_dense_eval` and the Faiss shim do not serve this form.

Subset search: `search(x, k, params=SearchParameters(sel=...))` (or `SearchParametersIVF(sel=, nprobe=)`) with the selectors of
`repconc_amd.selector`, for every storage above.  The result is what an `IVFFlatIndex` with the same coarse centroids (and the
same range) would return if it held only the selected vectors, each under the cell it has here: the same probes, ids and score
bits equal, ties to the lower corpus id, padding where the probed cells hold fewer than k selected rows; probing every cell
returns what the flat index returns under the same selector.  Nothing is copied: `_selection` turns the selector into the
list-major positions of the selected rows and their offsets per cell (cached on the selector until the store changes), the
plan reads those offsets in place of `list_off`, and the scan reads the store through the positions
(`ops.ivf_flat_search(rows=, sel_off=)`), so the score rows, the workspace and the rows read follow the selection.  Ids outside
the index are ignored; an empty selection is all padding without a launch; `params=None`, `SearchParameters()` and `sel=None`
are the plain search.

On the CPU device (`device="cpu"`: the build side with torch operators, for inspection and tests; the searches are GPU only)
cells are assigned by the same rule, argmin_l (||c_l||^2 - 2 <x, c_l>), first minimum, and codes decode with the same single
rounding.

`add` may be called repeatedly; ids continue from `ntotal`.  Every `add` rebuilds the list-major store from the rows held and the
new ones: while it runs, a second copy of the whole store exists on the device.
"""
from __future__ import annotations

import functools
import itertools
from typing import Optional

import numpy as np
import torch

from . import ops
from .dense_index import SQ8_ROWS_PER_STEP, sq8_encode  # noqa: F401  (names this module has always had)
from .dense_index import _sq8_encode_chunks, sq8_train_range
from .index import METRIC_INNER_PRODUCT, METRIC_L2, _as_device, _as_f32_tensor
from .ivf import CoarseProbe, coarse_assign, coarse_kmeans
from .selector import IDSelector, SearchParameters

_GENERATION = itertools.count(1)      # one number per store ever built, over all indexes: the key of a selector's cached selection


class IVFFlatIndex(CoarseProbe):
    STORAGE = {"float32": torch.float32, "float16": torch.float16, "int8": torch.int8}
    MAX_NLIST = ops.IVF_FLAT_MAX_NLIST
    MAX_WS_BYTES = 4 << 30            # workspace of one library call: a search is cut into chunks of queries that stay below it

    def __init__(self, d: int, nlist: int, device: Optional[torch.device] = None, metric=METRIC_INNER_PRODUCT,
                 storage: str = "float32", *, by_residual: bool = False):
        if metric not in (METRIC_INNER_PRODUCT, METRIC_L2):
            raise ValueError(f"metric must be METRIC_INNER_PRODUCT (0) or METRIC_L2 (1), not {metric!r}")
        if storage not in self.STORAGE:
            raise ValueError(f"storage must be one of {sorted(self.STORAGE)}, got {storage!r}")
        if int(d) < 1 or not 1 <= int(nlist) <= self.MAX_NLIST:
            raise ValueError(f"d must be >= 1 and nlist in [1, {self.MAX_NLIST}]")
        if storage == "int8" and int(d) > ops.DENSE_SQ8_MAX_D:
            raise ValueError(f"int8 storage: d must be <= {ops.DENSE_SQ8_MAX_D}")
        if by_residual and storage != "int8":
            raise ValueError(f"by_residual=True encodes residuals: it needs storage='int8', not {storage!r}")
        self.metric_type = metric
        self.storage = storage
        self.by_residual = bool(by_residual)
        self._dtype = self.STORAGE[storage]
        self._coarse_sq = (None, None, None)                                # CoarseProbe: (coarse, its version, ||c_l||^2)
        self.device = _as_device(device)
        self.d, self.nlist = int(d), int(nlist)
        self.coarse = None                                                  # [nlist, d] fp32
        self.vmin = self.step = self.mid = self._dec = None                 # int8 storage: the trained range, _dec [2, d] = step, mid
        self.nprobe = 8                                                     # Faiss's attribute: cells probed when search() is not told
        self.last_search_stats = {"queries": 0, "fallback_queries": 0, "chunks": 0}
        self.reset()

    # ---- build
    @property
    def is_trained(self) -> bool:
        return self.coarse is not None and (self.storage != "int8" or self._dec is not None)

    def reset(self) -> None:
        """Empties the index; the coarse centroids (and the range of int8 storage) stay."""
        self.xb = torch.empty((0, self.d), dtype=self._dtype, device=self.device)
        self.ids = torch.empty((0,), dtype=torch.int64, device=self.device)
        self.list_off = torch.zeros((self.nlist + 1,), dtype=torch.int64, device=self.device)
        self.ntotal = 0
        self._sizes_desc = np.zeros(0, np.int64)      # cell sizes, descending (host copy): bounds a query's score row
        self._generation = next(_GENERATION)

    def _rows(self, x, what: str) -> torch.Tensor:
        xt = _as_f32_tensor(x)
        if xt.dim() != 2 or xt.shape[1] != self.d:
            raise ValueError(f"{what}: expected [n, {self.d}] vectors, got {tuple(xt.shape)}")
        return xt

    def train(self, x, iters: int = 10, seed: int = 1234) -> None:
        """Fits the `nlist` coarse centroids by `coarse_kmeans` on x [n >= nlist, d]; int8 storage: also the per-dimension range
        of the same rows (`train_sq`); by_residual: the range of their residuals against the centroids just fitted."""
        xt = self._rows(x, "train")
        if xt.shape[0] < self.nlist:
            raise ValueError(f"train: {xt.shape[0]} vectors for {self.nlist} cells")
        if self.by_residual and self.ntotal:
            raise ValueError("train: the index holds residual codes of the current centroids and range; reset() first")
        if self.storage == "int8" and not self.by_residual:
            self.train_sq(xt)
        self.coarse = coarse_kmeans(xt.to(self.device, torch.float32), self.nlist, iters, seed)
        if self.by_residual:
            self.train_sq(xt)

    def train_sq(self, x) -> None:
        """int8 storage: sets the scalar quantiser's per-dimension range from x [n >= 1, d] alone (beside `set_coarse`);
        by_residual: from the residuals of x against the centroids of their L2-nearest cells, which have to exist."""
        if self.storage != "int8":
            raise ValueError("train_sq: only int8 storage has a range to train")
        if self.ntotal:
            raise ValueError("train_sq: the index holds codes of the current range; reset() first")
        if self.by_residual and self.coarse is None:
            raise ValueError("train_sq: residual encoding needs the coarse centroids first (set_coarse, or train)")
        self.vmin, self._dec = sq8_train_range(self._rows(x, "train_sq"), self.device, self._residual if self.by_residual else None)
        self.step, self.mid = self._dec[0], self._dec[1]

    def _need_range(self, what: str) -> None:
        if self.storage == "int8" and self._dec is None:
            raise ValueError(f"{what}: int8 storage needs its range first (train(x), or train_sq(x) beside set_coarse)")

    def set_coarse(self, centroids) -> None:
        """Installs given coarse centroids [nlist, d]."""
        if self.by_residual and self.ntotal:
            raise ValueError("set_coarse: the index holds codes of residuals against the current centroids; reset() first")
        c = centroids.detach() if isinstance(centroids, torch.Tensor) else torch.from_numpy(np.asarray(centroids, dtype=np.float32))
        if c.dim() != 2 or tuple(c.shape) != (self.nlist, self.d):
            raise ValueError(f"set_coarse: expected [{self.nlist}, {self.d}] centroids, got {tuple(c.shape)}")
        self.coarse = c.to(self.device, torch.float32).contiguous().clone()

    def _assign(self, xt: torch.Tensor) -> torch.Tensor:
        """The L2-nearest cell [n] int64 of fp32 rows on the index's device: `coarse_assign`; the CPU device: its rule in torch
        operators."""
        if self.device.type == "cuda":
            return coarse_assign(xt, self.coarse)
        c2 = (self.coarse * self.coarse).sum(1)
        parts = [torch.argmin(c2[None, :] - 2.0 * (xt[i:i + (1 << 16)] @ self.coarse.T), dim=1) for i in range(0, xt.shape[0], 1 << 16)]
        return torch.cat(parts) if parts else torch.empty((0,), dtype=torch.int64, device=self.device)

    def _residual(self, part: torch.Tensor) -> torch.Tensor:
        """fp32 rows on the device minus the centroids of their L2-nearest cells; a non-finite row (refused by whoever takes the
        residuals) is assigned as zeros and stays non-finite."""
        return part - self.coarse[self._assign(torch.nan_to_num(part, nan=0.0, posinf=0.0, neginf=0.0))]

    def _stored(self, xt: torch.Tensor, cells: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The rows of an `add` in the storage type, checked before anything is stored; one host read.  by_residual: `cells` [n]
        on the device, the codes are those of fp32(x - coarse[cell])."""
        if self.storage == "int8":
            codes = torch.empty((xt.shape[0], self.d), dtype=torch.int8, device=self.device)
            finite = torch.ones((), dtype=torch.bool, device=self.device)
            shift = (lambda r0, n: self.coarse[cells[r0:r0 + n]]) if self.by_residual else None
            for r0, part in _sq8_encode_chunks(xt, self.vmin, self.step, finite, shift=shift):
                codes[r0:r0 + part.shape[0]] = part
            if not bool(finite):
                raise ValueError("add: int8 storage needs finite values" + (" and finite residuals" if self.by_residual else ""))
            return codes
        xs = xt.to(self.device).to(self._dtype)
        if xs.shape[0] and not bool(torch.isfinite(xs).all()):
            raise ValueError("add: finite values only" if self.storage == "float32" else
                             "add: float16 storage needs finite values of magnitude < 65520 (fp16 rounds the rest to inf)")
        return xs

    def _corpus_order(self) -> tuple:
        """(rows [ntotal, d] in corpus order, their cells [ntotal]) from the list-major store."""
        x = torch.empty_like(self.xb)
        x[self.ids] = self.xb
        sizes = self.list_off[1:] - self.list_off[:-1]
        cells = torch.empty((self.ntotal,), dtype=torch.int64, device=self.device)
        cells[self.ids] = torch.repeat_interleave(torch.arange(self.nlist, device=self.device), sizes)
        return x, cells

    def _store(self, xs: torch.Tensor, cells: torch.Tensor) -> None:
        """xs [N, d] in the storage type and corpus order, cells [N] int64 in [0, nlist): the list-major store (stable sort)."""
        if xs.shape[0] >= 1 << 32:
            raise ValueError("the index holds fewer than 2^32 rows")
        order = torch.argsort(cells, stable=True)
        self.xb = xs[order].contiguous()
        self.ids = order.to(torch.int64).contiguous()
        cnt = torch.bincount(cells, minlength=self.nlist)
        self.list_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), torch.cumsum(cnt, 0)]).contiguous()
        self.ntotal = int(xs.shape[0])
        self._sizes_desc = np.sort(cnt.cpu().numpy())[::-1].astype(np.int64)
        self._generation = next(_GENERATION)

    def set_lists(self, x, list_ids) -> None:
        """Replaces the content by the rows x [N, d] (corpus order: row i has id i) stored under the given cells list_ids [N]."""
        xt = self._rows(x, "set_lists")
        self._need_range("set_lists")
        li = list_ids if isinstance(list_ids, torch.Tensor) else torch.from_numpy(np.asarray(list_ids))
        if li.dim() != 1 or li.shape[0] != xt.shape[0] or li.dtype.is_floating_point:
            raise ValueError(f"set_lists: expected {xt.shape[0]} integer cells, got {li.dtype} {tuple(li.shape)}")
        if li.numel() and (int(li.min()) < 0 or int(li.max()) >= self.nlist):
            raise ValueError(f"set_lists: cells must lie in [0, {self.nlist})")
        li = li.to(self.device, torch.int64)
        self._store(self._stored(xt, li), li)

    def add(self, x) -> None:
        """Appends x [n, d]: ids ntotal .. ntotal + n - 1, every row under its L2-nearest coarse centroid (of the values given,
        before any rounding to the storage type).  Rebuilds the list-major store: a transient second copy of it exists meanwhile."""
        if self.coarse is None:
            raise ValueError("add: train() or set_coarse() the coarse quantiser first")
        self._need_range("add")
        xt = self._rows(x, "add")
        if xt.shape[0] == 0:
            return
        if self.by_residual:      # the codes need the cells first; a non-finite row, which `_stored` refuses, is assigned as zeros
            cells = self._assign(torch.nan_to_num(xt.to(self.device, torch.float32), nan=0.0, posinf=0.0, neginf=0.0))
            xs = self._stored(xt, cells)
        else:
            xs = self._stored(xt)
            cells = self._assign(xt.to(self.device, torch.float32))
        if self.ntotal:
            old_x, old_cells = self._corpus_order()
            xs, cells = torch.cat([old_x, xs], 0), torch.cat([old_cells, cells], 0)
        self._store(xs, cells)

    def reconstruct_n(self, i0: int = 0, ni: int = -1) -> torch.Tensor:
        """fp32 [ni, d]: the stored values of corpus rows i0 .. i0 + ni - 1 (ni = -1: up to ntotal), as the search scores them;
        int8 storage: the decoded rows (`ops.dense_sq8_decode`), by_residual: plus the centroid of every row's cell."""
        self._need_range("reconstruct_n")
        ni = self.ntotal - int(i0) if ni < 0 else int(ni)
        if not (0 <= int(i0) and ni >= 0 and int(i0) + ni <= self.ntotal):
            raise ValueError(f"reconstruct_n: rows [{i0}, {int(i0) + ni}) outside [0, {self.ntotal})")
        where = torch.empty_like(self.ids)
        where[self.ids] = torch.arange(self.ntotal, device=self.device)
        pos = where[int(i0):int(i0) + ni]
        return self._decoded(pos) if self.storage == "int8" else self.xb[pos].float()

    def _decoded(self, pos: torch.Tensor) -> torch.Tensor:
        """int8 storage: the stored values fp32 [n, d] of the list-major rows `pos`: the decode with its one rounding, and
        by_residual one separate fp32 addition of the centroid of the row's cell (the scan's two roundings)."""
        codes = self.xb[pos].contiguous()
        rows = ops.dense_sq8_decode(codes, self._dec) if self.device.type == "cuda" else ops._sq8_decode_cpu(codes, self._dec)
        if self.by_residual:
            rows = rows + self.coarse[torch.searchsorted(self.list_off, pos, right=True) - 1]
        return rows

    # ---- search
    def _queries(self, x, k: int):
        as_numpy = not isinstance(x, torch.Tensor)
        q = _as_f32_tensor(x)
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"search: expected [nq, {self.d}] queries, got {tuple(q.shape)}")
        if not 1 <= int(k) <= ops.DENSE_MAX_K:
            raise ValueError(f"search: k must be in [1, {ops.DENSE_MAX_K}]")
        self._need_range("search")
        return q, as_numpy

    def _padding(self, nq: int, k: int):
        pad = float("inf") if self.metric_type == METRIC_L2 else float("-inf")
        return (torch.full((nq, k), pad, dtype=torch.float32, device=self.device),
                torch.full((nq, k), -1, dtype=torch.int64, device=self.device))

    @staticmethod
    def _params(params):
        """(selector or None, nprobe or None) of `params`: None, a SearchParameters or a SearchParametersIVF."""
        if params is None:
            return None, None
        if not isinstance(params, SearchParameters):
            raise ValueError("search: params must be a SearchParameters / SearchParametersIVF or None")
        if params.sel is not None and not isinstance(params.sel, IDSelector):
            raise ValueError("search: params.sel must be an IDSelector or None")
        return params.sel, getattr(params, "nprobe", None)

    def _selection(self, sel: IDSelector):
        """(rows, sel_off, sizes_desc) of a selector over this store: rows int64 [ns], the list-major positions of the rows
        whose corpus id it holds, ascending (so grouped by cell, and ascending by corpus id inside a cell: the store is stably
        sorted); sel_off int64 [nlist + 1], the offsets of the cells inside rows; sizes_desc, the host copy of the selected
        sizes per cell, descending.  A range of corpus ids is no slice of a list-major store: every selector takes this path.
        Valid by construction (`ops.ivf_flat_search(check_rows=False)`); cached on the selector until the store changes."""
        if sel._ivf_key != self._generation:
            member = sel._mask(self.ntotal, 0, self.device)[self.ids]
            rows = torch.nonzero(member).flatten().contiguous()
            sel_off = torch.searchsorted(rows, self.list_off).contiguous()
            sizes = (sel_off[1:] - sel_off[:-1]).cpu().numpy()
            sel._ivf = (rows, sel_off, np.sort(sizes)[::-1].astype(np.int64))
            sel._ivf_key = self._generation
        return sel._ivf

    def search(self, x, k: int, nprobe: Optional[int] = None, params: Optional[SearchParameters] = None):
        """(scores or distances [nq, k], ids [nq, k]) over the `nprobe` best cells of every query (default: `params.nprobe` of a
        `SearchParametersIVF`, then the index's `nprobe` attribute, as with a Faiss IVF index).  numpy in -> numpy out, tensors
        in -> tensors out.  params: None or `SearchParameters()` is the whole store; `SearchParameters(sel=...)` answers over
        the selected ids only, in place (the module's text)."""
        sel, params_nprobe = self._params(params)
        q, as_numpy = self._queries(x, k)
        if self.coarse is None:
            raise ValueError("search: train() or set_coarse() the coarse quantiser first")
        if nprobe is None:
            nprobe = self.nprobe if params_nprobe is None else params_nprobe
        nprobe = min(max(int(nprobe), 1), self.nlist)
        return self._answer(q, lambda qd: self.probe(qd, nprobe, ordered=False), int(k), as_numpy, sel)

    def _answer(self, q: torch.Tensor, probes_of, k: int, as_numpy: bool, sel: Optional[IDSelector] = None):
        """The common end of `search` and `_search_probes`: the queries on the device, all padding without a launch for an empty
        index, no query or an empty selection, `_run` on probes_of(queries on the device) otherwise, numpy out for numpy in."""
        q = q.to(self.device, torch.float32).contiguous()
        selection = None if sel is None or self.ntotal == 0 else self._selection(sel)
        if q.shape[0] == 0 or self.ntotal == 0 or (selection is not None and selection[0].numel() == 0):
            self.last_search_stats = {"queries": int(q.shape[0]), "fallback_queries": 0, "chunks": 0}
            scores, ids = self._padding(q.shape[0], k)
        else:
            scores, ids = self._run(q, probes_of(q), k, selection)
        if sel is not None:
            self.last_search_stats["rows_selected"] = 0 if selection is None else int(selection[0].numel())
        return (scores.cpu().numpy(), ids.cpu().numpy()) if as_numpy else (scores, ids)

    def _search_probes(self, x, probes, k: int, params: Optional[SearchParameters] = None):
        """`search` with explicit probes [nq, nprobe] (distinct cells of [0, nlist) per query, any order)."""
        sel, _ = self._params(params)
        q, as_numpy = self._queries(x, k)
        pr = probes if isinstance(probes, torch.Tensor) else torch.from_numpy(np.asarray(probes))
        if pr.dim() != 2 or pr.shape[0] != q.shape[0] or not 1 <= pr.shape[1] <= self.nlist or pr.dtype.is_floating_point:
            raise ValueError(f"_search_probes: expected integer probes [{q.shape[0]}, 1 .. {self.nlist}], got {tuple(pr.shape)}")
        pr = torch.sort(pr.to(torch.int32), dim=1).values
        if pr.numel() and (int(pr.min()) < 0 or int(pr.max()) >= self.nlist or bool((pr[:, 1:] == pr[:, :-1]).any())):
            raise ValueError(f"_search_probes: a query's probes must be distinct cells of [0, {self.nlist})")
        return self._answer(q, lambda qd: pr.to(self.device).contiguous(), int(k), as_numpy, sel)

    def _chunk_queries(self, nq: int, nprobe: int, stride: int) -> int:
        """The most queries (>= 1) whose workspace stays under MAX_WS_BYTES."""
        if ops.ivf_flat_search_ws_bytes(nq, nprobe, self.nlist, stride) <= self.MAX_WS_BYTES:
            return nq
        lo, hi = 1, nq                                  # ws(lo) fits (or lo == 1), ws(hi) does not
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if ops.ivf_flat_search_ws_bytes(mid, nprobe, self.nlist, stride) <= self.MAX_WS_BYTES:
                lo = mid
            else:
                hi = mid
        return lo

    def _run(self, q: torch.Tensor, probes: torch.Tensor, k: int, selection=None):
        """q [nq, d] fp32 on the device, probes [nq, nprobe] int32 ascending per query; nq > 0, ntotal > 0.  selection: None, or
        the non-empty (rows, sel_off, sizes_desc) of `_selection`: the score rows, the workspace and the chunks follow it."""
        nq, nprobe = probes.shape
        sizes_desc = self._sizes_desc if selection is None else selection[2]
        stride = (max(4, int(sizes_desc[:nprobe].sum())) + 3) // 4 * 4            # the nprobe largest cells bound a score row
        step = self._chunk_queries(nq, nprobe, stride)
        if self.by_residual:                  # the search of this store with the store's own operands, chosen once
            search = functools.partial(ops.ivf_flat_sq8r_search, self.xb, self._dec, self.coarse)
        elif self.storage == "int8":
            search = functools.partial(ops.ivf_flat_sq8_search, self.xb, self._dec)
        else:
            search = functools.partial(ops.ivf_flat_search, self.xb)
        if selection is not None:             # valid by construction: no check, no synchronisation
            search = functools.partial(search, rows=selection[0], sel_off=selection[1], check_rows=False)
        parts, fallback, chunks = [], 0, 0
        for c0 in range(0, nq, step):
            qc, pc = q[c0:c0 + step], probes[c0:c0 + step]
            scores, ids, status, qstatus = search(self.list_off, self.ids, qc, pc, stride, k, metric=self.metric_type)
            chunks += 1
            st = int(status.item())
            if st & 4:
                raise RuntimeError("ivf_flat_search: a probe outside the index or a score row too short (status bit 2)")
            if st & 2:
                # more than 16384 probed rows tie at these queries' k-th score: the exact dense search over their probed rows
                bad = torch.nonzero(qstatus & 2).flatten()
                scores[bad], ids[bad] = self._search_exact_probed(qc[bad], pc[bad], k, selection)
                fallback += int(bad.numel())
            parts.append((scores, ids))
        self.last_search_stats = {"queries": int(nq), "fallback_queries": fallback, "chunks": chunks}
        if len(parts) == 1:
            return parts[0]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])

    def _search_exact_probed(self, q: torch.Tensor, probes: torch.Tensor, k: int, selection=None):
        """The answer for ANY content of the probed cells, query by query: the probed rows gathered in corpus-id order (the
        search's tie rule becomes the exact entry's "lower row"), then the exact route of the flat search of this metric and
        storage (int8: the fp32 exact route over the gathered rows, decoded, by_residual with their centroids added).  Slow —
        one gather of the probed rows per query — and only reached for queries the selection could not decide.  selection
        (`_selection`): only the selected rows of the probed cells are gathered."""
        exact = ((ops.dense_search_exact, ops.dense_search_f16_exact),
                 (ops.dense_search_l2_exact, ops.dense_search_l2_f16_exact))[self.metric_type == METRIC_L2][self.storage == "float16"]
        scores, ids = self._padding(q.shape[0], k)
        off = self.list_off if selection is None else selection[1]
        for j in range(q.shape[0]):
            cells = probes[j].long()
            a, b = off[cells].tolist(), off[cells + 1].tolist()
            rows = torch.cat([torch.arange(lo, hi, device=self.device) for lo, hi in zip(a, b)])
            if selection is not None:
                rows = selection[0][rows]
            if rows.numel() == 0:
                continue
            corpus = self.ids[rows]
            order = torch.argsort(corpus)
            rows, corpus = rows[order], corpus[order]
            gathered = self._decoded(rows) if self.storage == "int8" else self.xb[rows].contiguous()
            s, i = exact(gathered, q[j:j + 1], k)
            valid = i[0] >= 0
            scores[j] = s[0]
            ids[j, valid] = corpus[i[0][valid]]
        return scores, ids
