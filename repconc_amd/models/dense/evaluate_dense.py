"""Everything evaluate/run_dense_eval.py imports from the reference's models/dense/evaluate_dense.py, under the same names:
`DenseEvaluater`, `encode_dense_corpus`, `encode_dense_query`, `dense_search`, `batch_dense_search`, `create_index`.
No Faiss import: the index is repconc_amd.dense_index.FlatIPIndex, the exact fp32 inner-product search of a GPU
faiss.IndexFlatIP with useFloat16 = False (evaluate_dense.py:84-129) on the matrix cores (csrc/dense_search.hip);
`create_index(metric="l2")` builds the squared-Euclidean indexes of the same module instead (faiss.IndexFlatL2).

`DenseEvaluater` keeps the reference's constructor and `.predict(dataset).predictions` contract (evaluate_dense.py:18-33)
but is a plain batched loop, not an HF-Trainer subclass, like RepCONCEvaluater (evaluate_repconc.py here).  It runs on one
device: the reference's `index_cpu_to_all_gpus` branch (more than one visible GPU, evaluate_dense.py:118-122) builds the
index on one device here.
"""
from __future__ import annotations

import logging
import math
from types import SimpleNamespace
from typing import Dict, Union

import numpy as np
import torch

from ...dense_index import FlatIPIndex, FlatL2Bf16x3Index, FlatL2F16Index, FlatL2Index, FlatSQ8Index
from ...index import METRIC_INNER_PRODUCT, METRIC_L2
from ...ivf_flat import IVFFlatIndex
from ...utils.eval_utils import TextDataset, get_collator_func

logger = logging.getLogger(__name__)


class DenseEvaluater:
    """`DenseEvaluater(model=..., args=..., data_collator=..., tokenizer=...).predict(dataset)` -> object with
    `.predictions` (fp32 numpy [n, hidden]) in dataset order.  args.fp16 / args.bf16 run the encoder under autocast, as the
    Trainer's autocast_smart_context_manager does; the predictions are fp32 either way."""

    def __init__(self, model=None, args=None, data_collator=None, tokenizer=None, **_ignored):
        self.model, self.args, self.data_collator, self.tokenizer = model, args, data_collator, tokenizer

    @torch.no_grad()
    def prediction_step(self, model, inputs, prediction_loss_only=False, ignore_keys=None):
        """One batch -> (None, embeddings fp32 [b, hidden], None).  evaluate_dense.py:19-33."""
        assert not prediction_loss_only and ignore_keys is None
        dev = next(model.parameters()).device
        inputs = {k: v.to(dev, non_blocking=True) for k, v in inputs.items() if k != "text_ids"}
        amp = bool(getattr(self.args, "fp16", False) or getattr(self.args, "bf16", False))
        dtype = torch.bfloat16 if getattr(self.args, "bf16", False) else torch.float16
        with torch.autocast(dev.type, dtype=dtype, enabled=amp):
            logits = model(**inputs).detach().float().contiguous()
        return None, logits, None

    def predict(self, dataset):
        model = self.model
        model.eval()
        bs = int(getattr(self.args, "per_device_eval_batch_size", 64) or 64)
        chunks = []
        for s in range(0, len(dataset), bs):
            batch = self.data_collator([dataset[i] for i in range(s, min(s + bs, len(dataset)))])
            chunks.append(self.prediction_step(model, batch)[1])
        hidden = model.config.hidden_size
        preds = torch.cat(chunks, 0).cpu().numpy() if chunks else np.empty((0, hidden), dtype=np.float32)
        return SimpleNamespace(predictions=preds, label_ids=None, metrics={})


def encode_dense_corpus(corpus: Dict[Union[str, int], str], model, tokenizer, max_seq_length: int, eval_args,
                        split_corpus_num=20):
    """(corpus embeddings fp32 numpy [n, hidden], corpus ids): documents sorted longest first by word count, encoded in
    `split_corpus_num` parts.  evaluate_dense.py:36-65."""
    logger.info("Sorting Corpus by document length (Longest first)...")
    corpus_ids = np.array(sorted(corpus, key=lambda k: len(corpus[k].split()), reverse=True))
    corpus_embeds = np.empty((len(corpus_ids), model.config.hidden_size), dtype=np.float32)
    write_num = 0
    for doc_ids in np.array_split(corpus_ids, max(1, min(split_corpus_num, len(corpus_ids)))):
        doc_text = [corpus[did] for did in doc_ids]
        doc_out = DenseEvaluater(model=model, args=eval_args, tokenizer=tokenizer,
                                 data_collator=get_collator_func(tokenizer, max_seq_length, input_text_type="doc"),
                                 ).predict(TextDataset(doc_text))
        assert len(doc_out.predictions) == len(doc_text)
        corpus_embeds[write_num:write_num + len(doc_text)] = doc_out.predictions
        write_num += len(doc_text)
    return corpus_embeds, corpus_ids


def encode_dense_query(queries: Dict[Union[str, int], str], model, tokenizer, max_seq_length: int, eval_args):
    """(query embeddings fp32 numpy [nq, hidden], query ids sorted ascending).  evaluate_dense.py:68-81."""
    logger.info("Encoding Queries...")
    query_ids = sorted(queries.keys())
    out = DenseEvaluater(model=model, args=eval_args, tokenizer=tokenizer,
                         data_collator=get_collator_func(tokenizer, max_seq_length, input_text_type="query"),
                         ).predict(TextDataset([queries[qid] for qid in query_ids]))
    assert len(out.predictions) == len(query_ids)
    return out.predictions, np.array(query_ids)


def dense_search(query_ids: np.ndarray, query_embeds, corpus_ids: np.ndarray, index: FlatIPIndex, topk: int):
    """evaluate_dense.py:84-90."""
    topk_scores, topk_idx = index.search(query_embeds, topk)
    if isinstance(topk_idx, torch.Tensor):
        topk_idx, topk_scores = topk_idx.cpu().numpy(), topk_scores.cpu().numpy()
    topk_ids = np.asarray(corpus_ids)[topk_idx]
    assert len(query_ids) == len(topk_scores) == len(topk_ids)
    return topk_scores, topk_ids


def batch_dense_search(query_ids: np.ndarray, query_embeds, corpus_ids: np.ndarray, index: FlatIPIndex, topk: int,
                       batch_size: int):
    """evaluate_dense.py:93-112 (np.array_split batching).  Every batch is enqueued through `search_async` before the first
    result is read, so the device runs the batches back to back; an index without `search_async` takes the reference's
    batch-by-batch loop."""
    iterations = max(1, math.ceil(len(query_ids) / batch_size))
    qid_parts, emb_parts = np.array_split(query_ids, iterations), np.array_split(query_embeds, iterations)
    if not hasattr(index, "search_async"):
        got = [dense_search(qid_it, emb_it, corpus_ids, index, topk) for qid_it, emb_it in zip(qid_parts, emb_parts)]
        return np.concatenate([g[0] for g in got], axis=0), np.concatenate([g[1] for g in got], axis=0)
    pending = [index.search_async(emb_it, topk) for emb_it in emb_parts]
    ids_table = np.asarray(corpus_ids)
    all_scores, all_ids = [], []
    for qid_it, fin in zip(qid_parts, pending):
        topk_scores, topk_idx = fin()
        if isinstance(topk_idx, torch.Tensor):
            topk_idx, topk_scores = topk_idx.cpu().numpy(), topk_scores.cpu().numpy()
        assert len(qid_it) == len(topk_scores) == len(topk_idx)
        all_scores.append(topk_scores)
        all_ids.append(ids_table[topk_idx])
    return np.concatenate(all_scores, axis=0), np.concatenate(all_ids, axis=0)


INDEX_METRICS = ("ip", "l2")
INDEX_STORAGES = (None, "int8")


def check_index_options(metric: str, use_float16: bool, screen: str, nlist: int = 0, storage=None) -> None:
    """ValueError for an unknown metric, storage or screen, or a combination that does not exist (fp16 storage with the bf16x3
    screen, under either metric; the bf16x3 screen with an IVF index, nlist > 0; storage="int8" with fp16 storage, the bf16x3
    screen, nlist > 0 or the L2 metric); touches no device.  The one rule of `create_index` and of run_dense_eval's arguments."""
    if metric not in INDEX_METRICS:
        raise ValueError(f"metric must be one of {list(INDEX_METRICS)}, got {metric!r}")
    if storage not in INDEX_STORAGES:
        raise ValueError(f"storage must be one of {list(INDEX_STORAGES)}, got {storage!r}")
    if storage == "int8" and (use_float16 or screen != "fp32" or int(nlist) > 0 or metric != "ip"):
        raise ValueError("storage='int8' is the flat inner-product index over 8-bit codes: it cannot be combined with "
                         "use_float16, screen='bf16x3', nlist > 0 or metric='l2'")
    FlatIPIndex.check_options("float16" if use_float16 else "float32", screen)
    if int(nlist) < 0 or int(nlist) > IVFFlatIndex.MAX_NLIST:
        raise ValueError(f"nlist must be in [0, {IVFFlatIndex.MAX_NLIST}], got {nlist!r}")
    if int(nlist) > 0 and screen == "bf16x3":
        raise ValueError("screen='bf16x3' belongs to the flat indexes: it cannot be combined with nlist > 0")


IVF_TRAIN_ROWS = 1 << 18       # rows of the seeded sample the coarse centroids are fitted on (IVFPQIndex.from_flat's)


def create_index(corpus_embeds, single_gpu_id=None, use_float16=False, screen="fp32", metric="ip", nlist=0, nprobe=8,
                 storage=None):
    """An exact index holding `corpus_embeds`, on device `single_gpu_id` or the current device.
    use_float16: store the vectors as fp16 (GpuClonerOptions.useFloat16, which the reference leaves False).
    screen="bf16x3" (fp32 storage only): the same results, candidates chosen on the bf16 matrix cores.
    metric="ip": `FlatIPIndex` (evaluate_dense.py:115-129); metric="l2": squared Euclidean distance, smallest first,
    `FlatL2Index`, `FlatL2F16Index` (use_float16) or `FlatL2Bf16x3Index` (screen="bf16x3").
    nlist > 0: an `IVFFlatIndex` of that many cells instead (faiss.IndexIVFFlat; not in the reference): the coarse centroids are
    fitted on a seeded sample of at most 2^18 rows, as `IVFPQIndex.from_flat` fits them, and a search scores exactly the rows of
    the `nprobe` best cells of every query — the flat index's scores for the rows it reaches, not every row.
    storage="int8" (metric "ip", flat, alone): a `FlatSQ8Index` (faiss.IndexScalarQuantizer, QT_8bit), one byte per dimension,
    trained on the batch it is given, `corpus_embeds`; its scores are exact for the DECODED rows, the centres of their bins."""
    check_index_options(metric, use_float16, screen, nlist, storage)                           # before a device is looked at
    dev = torch.device("cuda", single_gpu_id if single_gpu_id is not None else torch.cuda.current_device())
    d = corpus_embeds.shape[1]
    if storage == "int8":
        index = FlatSQ8Index(d, device=dev)
        index.train(corpus_embeds)
        index.add(corpus_embeds)
        return index
    if int(nlist) > 0:
        index = IVFFlatIndex(d, int(nlist), device=dev, metric=METRIC_L2 if metric == "l2" else METRIC_INNER_PRODUCT,
                             storage="float16" if use_float16 else "float32")
        index.nprobe = int(nprobe)
        n = corpus_embeds.shape[0]
        sel = np.sort(np.random.default_rng(1234).permutation(n)[:IVF_TRAIN_ROWS])
        index.train(corpus_embeds[torch.from_numpy(sel)] if isinstance(corpus_embeds, torch.Tensor) else corpus_embeds[sel])
        index.add(corpus_embeds)
        return index
    if metric == "l2":
        index = (FlatL2F16Index if use_float16 else FlatL2Bf16x3Index if screen == "bf16x3" else FlatL2Index)(d, device=dev)
    else:
        index = FlatIPIndex(d, device=dev, storage="float16" if use_float16 else "float32", screen=screen)
    index.add(corpus_embeds)
    return index
