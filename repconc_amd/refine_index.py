"""Search a compressed index, re-rank its candidates exactly: the GPU `faiss.IndexRefineFlat`.

`RefineIndex(base, refine, k_factor)` joins the two search families of the package.  `base` is anything with
`search(x, k)` and `ntotal` — `PQIndex`, `IVFPQIndex`, the sharded / replicated wrappers of `multi_index` — and ranks by
ADC scores; `refine` is a flat index of `dense_index` that holds the same rows, uncompressed, under the same ids.  A search
takes `kc = k * k_factor` candidates from `base`, scores only those rows against the stored vectors
(`refine.rerank`, `ops.dense_rerank`, csrc/dense_rerank.hip) and returns the top-k of that: the scores are the flat
index's own, bit for bit, for every id returned.  The exact work per batch is nq * kc row reads instead of nq * ntotal.

There is no `add`: the two indexes are filled by their owners (`encode.encode_corpus_to_index(..., refine=flat)` fills
both from one pass over the corpus, with the re-ranking vectors in the rotated space of the queries).
"""
from __future__ import annotations

import inspect
import math

from . import ops


class RefineIndex:
    MAX_KC = ops.DENSE_MAX_K          # the base searches return at most 8192 results per query

    def __init__(self, base, refine, k_factor: float = 1.0):
        if not callable(getattr(base, "search", None)) or not hasattr(base, "ntotal"):
            raise ValueError("RefineIndex: base needs search(x, k) and ntotal")
        if not callable(getattr(refine, "rerank", None)) or not hasattr(refine, "ntotal"):
            raise ValueError("RefineIndex: refine must be a flat index (rerank(x, cand_ids, k) and ntotal)")
        self.base = base
        try:                          # decided once: does base.search(x, k, ..., params=) exist
            self._base_takes_params = "params" in inspect.signature(base.search).parameters
        except (TypeError, ValueError):           # a callable without an inspectable signature takes none
            self._base_takes_params = False
        self.refine = refine
        self.k_factor = k_factor      # a plain attribute, as in Faiss
        self._check_metric()

    def _check_metric(self) -> None:
        mb, mr = getattr(self.base, "metric_type", None), getattr(self.refine, "metric_type", None)
        if mb is not None and mr is not None and mb != mr:
            raise ValueError(f"RefineIndex: base ranks by metric {mb}, refine by metric {mr}")

    @property
    def ntotal(self) -> int:
        return self.base.ntotal

    @property
    def d(self) -> int:
        return self.refine.d

    @property
    def metric_type(self):
        return getattr(self.refine, "metric_type", getattr(self.base, "metric_type", None))

    def candidates(self, k: int) -> int:
        """kc of a search for `k` results: min(max(k, ceil(k * k_factor)), 8192)."""
        k = int(k)
        if k < 1:
            raise ValueError("RefineIndex: k must be >= 1")
        return min(max(k, int(math.ceil(k * float(self.k_factor)))), self.MAX_KC)

    def search(self, x, k: int, x_refine=None, params=None, **base_kwargs):
        """(scores or distances [nq, k], ids [nq, k]) of the `k` best of `base`'s `candidates(k)` results, re-ranked by
        `refine`.  x_refine: the queries in the space of the refine vectors when it is not the base's (default: x).  Further
        keyword arguments go to `base.search` (`nprobe=` of an IVF base).  Slots `base` left unfilled (-1) are skipped; what is
        missing after them is padded as `refine.search` pads.  params (`SearchParameters(sel=...)`): handed to a base whose
        `search` takes them — `PQIndex`, `IVFPQIndex`, a flat index that serves the subset search, an `IVFFlatIndex`; the
        candidates are then selected ids already and the re-rank needs nothing.  Refused with a ValueError: here, for a base whose
        `search` has no `params` argument (the multi-device wrappers); by the base itself, for a flat index whose storage or
        screen serves no subset search."""
        self._check_metric()
        if self.refine.ntotal != self.base.ntotal:
            raise ValueError(f"RefineIndex: base holds {self.base.ntotal} rows, refine {self.refine.ntotal}")
        if params is not None:
            if not self._base_takes_params:
                raise ValueError(f"RefineIndex: {type(self.base).__name__}.search takes no params (no subset search)")
            base_kwargs["params"] = params
        _, ids = self.base.search(x, self.candidates(k), **base_kwargs)
        return self.refine.rerank(x if x_refine is None else x_refine, ids, int(k))
