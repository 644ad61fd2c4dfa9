"""Exact inner-product index resident in HBM: the GPU `faiss.IndexFlatIP` (useFloat16 = False) of the reference's dense
evaluation, models/dense/evaluate_dense.py:84-129.

`FlatIPIndex` is duck-typed like that object (`d`, `ntotal`, `metric_type`, `is_trained`, `add`, `reset`, `search`) and
searches with `ops.dense_search` (csrc/dense_search.hip): scores are the fp32 fmaf chain over d ascending, bit for bit,
ties broken by the lower id.  The vectors live in ONE fp32 [capacity, d] device tensor appended to in place: the first
`add` allocates exactly, later growth is 1.5x (`reserve` sets the capacity up front).
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops
from .index import METRIC_INNER_PRODUCT


class FlatIPIndex:
    def __init__(self, d: int, device: Optional[torch.device] = None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type == "cuda" and self.device.index is None:        # "cuda" -> the current device, by index
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.d = int(d)
        self.metric_type = METRIC_INNER_PRODUCT
        self.is_trained = True
        self.ntotal = 0
        self.id_offset = 0       # global id of local row 0
        self.sel_slack = ops.DENSE_SEL_SLACK
        self.last_search = None
        self._x = torch.empty((0, self.d), dtype=torch.float32, device=self.device)

    @property
    def xb(self) -> torch.Tensor:
        """fp32 [ntotal, d] view of the stored vectors."""
        return self._x[: self.ntotal]

    def reserve(self, n: int) -> None:
        """Capacity for `n` rows in total (the rows held so far are kept)."""
        if n > self._x.shape[0]:
            grown = torch.empty((int(n), self.d), dtype=torch.float32, device=self.device)
            grown[: self.ntotal] = self._x[: self.ntotal]
            self._x = grown

    def add(self, x) -> None:
        xt = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        if xt.dim() != 2 or xt.shape[1] != self.d:
            raise ValueError(f"add: expected [n, {self.d}] vectors, got {tuple(xt.shape)}")
        n = xt.shape[0]
        need = self.ntotal + n
        if need > self._x.shape[0]:
            self.reserve(need if self.ntotal == 0 else max(need, int(self._x.shape[0] * 1.5)))
        self._x[self.ntotal:need] = xt.to(self.device, torch.float32)
        self.ntotal = need

    def reset(self) -> None:
        self.ntotal = 0
        self._x = torch.empty((0, self.d), dtype=torch.float32, device=self.device)

    def search(self, x, k: int):
        """(scores [nq, k], ids [nq, k]); numpy in -> numpy out (evaluate_dense.py:74), CUDA tensors in -> CUDA tensors
        out (faiss.contrib.torch_utils)."""
        return self.search_async(x, k)()

    def search_async(self, x, k: int):
        """Enqueue the search and return a callable that yields what `search` returns; nothing synchronises with the host
        until it is called (`batch_dense_search` enqueues every batch first)."""
        as_numpy = not isinstance(x, torch.Tensor)
        q = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) if as_numpy else x
        q = q.to(self.device, torch.float32, non_blocking=True)
        if q.dim() != 2 or q.shape[1] != self.d:
            raise ValueError(f"search: expected [nq, {self.d}] queries, got {tuple(q.shape)}")
        k = int(k)
        if self.ntotal == 0 or q.shape[0] == 0:
            scores = torch.full((q.shape[0], k), float("-inf"), dtype=torch.float32, device=self.device)
            ids = torch.full((q.shape[0], k), -1, dtype=torch.int64, device=self.device)
            pending = ops.PendingSearch(None, scores, ids, None, None, 0.0, 0)
        else:
            pending = ops.dense_search(self.xb, q, k, id_offset=self.id_offset, sel_slack=self.sel_slack, defer=True)
        self.last_search = pending           # .stats: queries repeated / answered by the exact route

        def finish():
            scores, ids = pending.result()
            if as_numpy:
                return scores.cpu().numpy(), ids.cpu().numpy()
            return scores, ids
        return finish
