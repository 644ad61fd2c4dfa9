"""The handful of `faiss.*` idioms the reference's call sites use on the index object, for `PQIndex`.

A maintainer who swaps `import faiss` for `from repconc_amd import faiss_compat as faiss` in
evaluate/run_repconc_eval.py, models/jpq/finetune_jpq.py and train/run_warmup.py keeps these lines unchanged:

    faiss.copy_array_to_vector(centroids.ravel(), index.pq.centroids)   evaluate_repconc.py:84-85, run_repconc_eval.py:123-127,
                                                                        finetune_jpq.py:211-213
    faiss.vector_to_array(index.pq.centroids) / (index.codes)           run_warmup.py:124-125, finetune_jpq.py:161
    faiss.IndexPQ(D, M, 8, faiss.METRIC_INNER_PRODUCT)                  evaluate_repconc.py:81
    faiss.IndexFlatIP(d)                                                evaluate_dense.py:116 (exact fp32, dense_index.py;
                                                                        useFloat16: FlatIPIndex(d, storage="float16"))
    faiss.IndexFlatL2(d)                                                evaluate_repconc.py:102, run_warmup.py:102,107 (exact
                                                                        fp32 squared distances, dense_index.FlatL2Index)
    faiss.IndexScalarQuantizer(d, faiss.ScalarQuantizer.QT_8bit,        not in the reference; the flat format between fp16 and PQ
                               faiss.METRIC_INNER_PRODUCT)              (one byte per dimension, dense_index.FlatSQ8Index)
    faiss.IndexIVFFlat(quantizer, d, nlist[, metric])                   not in the reference; what a Faiss user expects beside
                                                                        IndexFlat* and IndexIVFPQ (exact scan of the probed cells,
                                                                        ivf_flat.IVFFlatIndex)
    faiss.IndexIVFScalarQuantizer(quantizer, d, nlist,                  not in the reference; the same scan over 8-bit codes
                                  faiss.ScalarQuantizer.QT_8bit,        (IVFFlatIndex(storage="int8")); by_residual=False has to
                                  metric, by_residual=False)            be passed: the vectors themselves are encoded
    index.search(x, k, params=faiss.SearchParameters(sel=               not in the reference; subset search of the flat indexes
        faiss.IDSelectorRange / Batch / Array / Bitmap / Not(...)))     (fp32 and fp16 storage, both metrics; selector.py)
    index.search(x, k, params=faiss.SearchParametersIVF(sel=...,        not in the reference; the same selectors, and nprobe, on
        nprobe=...))                                                    IndexIVFFlat / IndexIVFScalarQuantizer (ivf_flat.py)
    index.search(x, k, params=faiss.SearchParameters(sel=...))          not in the reference; the same selectors on IndexPQ (and the
        on faiss.IndexPQ / faiss.IndexIVFPQ                             shim's IndexIVFPQ, which is the PQ index): the selected codes
                                                                        are compacted once per selector (index.py, ops.adc_select_rows)
    faiss.write_index(index, path) / faiss.read_index(path)             run_warmup.py:187, run_repconc_eval.py:42
    faiss.omp_set_num_threads(n)                                        run_repconc_eval.py:149 (no-op: the scan runs on the GPU)

The "vectors" are torch tensors here: `copy_array_to_vector` writes in place (the index's centroid table is ONE
resident tensor shared by `index.pq.centroids` and the search), `vector_to_array` returns a numpy copy.
"""
from __future__ import annotations

import numpy as np
import torch

from .dense_index import FlatIPIndex, FlatL2Index, FlatSQ8Index
from .faiss_io import read_index, write_index  # noqa: F401  (re-exported)
from .index import METRIC_INNER_PRODUCT, METRIC_L2, PQIndex  # noqa: F401  (METRIC_L2 re-exported)
from .ivf_flat import IVFFlatIndex
from .selector import (IDSelectorArray, IDSelectorBatch, IDSelectorBitmap, IDSelectorNot, IDSelectorRange,  # noqa: F401
                       SearchParameters, SearchParametersIVF)


def IndexPQ(d: int, M: int, nbits: int = 8, metric=METRIC_INNER_PRODUCT) -> PQIndex:
    return PQIndex(d, M, nbits, metric)


IndexFlatIP = FlatIPIndex      # faiss.IndexFlatIP(d): exact inner product over fp32 vectors resident on the device
IndexFlatL2 = FlatL2Index      # faiss.IndexFlatL2(d): exact squared Euclidean distance over the same storage


class ScalarQuantizer:
    """faiss.ScalarQuantizer's quantiser types, Faiss's numbering.  QT_8bit is the one that is served."""
    QT_8bit, QT_4bit, QT_8bit_uniform, QT_4bit_uniform, QT_fp16, QT_8bit_direct, QT_6bit = range(7)


class IndexScalarQuantizer(FlatSQ8Index):
    """faiss.IndexScalarQuantizer(d, qtype, metric): `FlatSQ8Index` with Faiss's argument order.  Faiss's default metric is
    METRIC_L2, which is not served over int8 codes: the metric has to be given as METRIC_INNER_PRODUCT, and any qtype but
    ScalarQuantizer.QT_8bit is refused."""

    def __init__(self, d: int, qtype: int = ScalarQuantizer.QT_8bit, metric=METRIC_L2, device=None):
        if qtype != ScalarQuantizer.QT_8bit:
            raise ValueError("IndexScalarQuantizer: only ScalarQuantizer.QT_8bit is served")
        if metric != METRIC_INNER_PRODUCT:
            raise ValueError("IndexScalarQuantizer: only METRIC_INNER_PRODUCT is served (pass it: Faiss's default is METRIC_L2)")
        super().__init__(d, device=device, metric=metric)
        self.qtype = qtype


class IndexIVFFlat(IVFFlatIndex):
    """faiss.IndexIVFFlat(quantizer, d, nlist, metric=METRIC_L2): `IVFFlatIndex` with Faiss's argument order and default
    metric.  `quantizer` is a flat index (IndexFlatL2 / IndexFlatIP) or None: one that already holds `nlist` vectors provides the
    coarse centroids and the index is trained; otherwise `train` fits them and, as Faiss does, adds them to an empty quantizer.
    The index lives on the quantizer's device."""

    _STORAGE = "float32"

    def __init__(self, quantizer, d: int, nlist: int, metric=METRIC_L2):
        if quantizer is not None and getattr(quantizer, "d", d) != d:
            raise ValueError(f"{type(self).__name__}: the quantizer holds vectors of width {quantizer.d}, the index {d}")
        super().__init__(d, nlist, device=getattr(quantizer, "device", None), metric=metric, storage=self._STORAGE)
        self.quantizer = quantizer
        if quantizer is not None and getattr(quantizer, "ntotal", 0) == self.nlist:
            self.set_coarse(quantizer.xb.float())

    def train(self, x, iters: int = 10, seed: int = 1234) -> None:
        if self.is_trained:                             # Faiss: training a trained index is a no-op
            return
        if self.coarse is not None:                     # int8 storage over a filled quantizer: only the range is missing
            self.train_sq(x)
            return
        super().train(x, iters, seed)
        if self.quantizer is not None and getattr(self.quantizer, "ntotal", None) == 0 and hasattr(self.quantizer, "add"):
            self.quantizer.add(self.coarse)


class IndexIVFScalarQuantizer(IndexIVFFlat):
    """faiss.IndexIVFScalarQuantizer(quantizer, d, nlist, qtype, metric=METRIC_L2, by_residual=True): `IVFFlatIndex(storage=
    "int8")` with Faiss's argument order and default metric; the quantizer is treated as `IndexIVFFlat` treats it.  Any qtype
    but ScalarQuantizer.QT_8bit is refused, and so is Faiss's default by_residual=True: this index encodes the vectors
    themselves, so that its scores are the flat int8 index's — pass by_residual=False.  (Residual codes exist as
    `IVFFlatIndex(storage="int8", by_residual=True)`; this class does not turn into them under Faiss's default.)"""
    _STORAGE = "int8"

    def __init__(self, quantizer, d: int, nlist: int, qtype: int = ScalarQuantizer.QT_8bit, metric=METRIC_L2,
                 by_residual: bool = True):
        if qtype != ScalarQuantizer.QT_8bit:
            raise ValueError("IndexIVFScalarQuantizer: only ScalarQuantizer.QT_8bit is served")
        if by_residual:
            raise ValueError("IndexIVFScalarQuantizer: residual encoding is not served; pass by_residual=False (Faiss's "
                             "default is True): the vectors themselves are encoded")
        super().__init__(quantizer, d, nlist, metric)
        self.qtype, self.by_residual = qtype, False


def copy_array_to_vector(array, vector: torch.Tensor) -> None:
    """`vector` is `index.pq.centroids` (or any tensor of the same size): overwritten in place, [m][k][j] order."""
    src = array.detach() if isinstance(array, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(array))
    if src.numel() != vector.numel():
        raise ValueError(f"size mismatch: {src.numel()} values for a vector of {vector.numel()}")
    vector.copy_(src.reshape(vector.shape).to(vector.device, vector.dtype))


def vector_to_array(vector) -> np.ndarray:
    """Flat numpy copy of `index.pq.centroids` (float32) or `index.codes` (uint8, row-major [ntotal * M])."""
    # tensors, and the fan-out view a multi-device index exposes as pq.centroids (multi_index._FanoutCentroids)
    t = vector.detach() if hasattr(vector, "detach") else torch.as_tensor(vector)
    return t.reshape(-1).cpu().numpy().copy()


def omp_set_num_threads(n: int) -> None:
    """Accepted and ignored: there is no OpenMP pool behind the search."""


def downcast_index(index):
    return index
