"""Stage-2 (JPQ) model: query encoder + PQ centroids trained against a FIXED code index.

Mirror of the `JPQ` module of models/jpq/finetune_jpq.py:139-246 (constructor arguments, `forward(query_input_ids,
query_attention_mask, qids) -> {"loss"}`, `synchronize_model_index`, `normalize_centrodis`, `state_dict` /
`load_state_dict` delegating to the wrapped RepCONC) with the index side replaced:

  * the reference re-copies the centroid table into two Faiss indexes and re-clones the whole IVFPQ index (424 MB at
    M = 48) to the GPU after EVERY optimiser step (:209-214, callback :249-255).  Here `pq_index` is a
    `repconc_amd.index.PQIndex` whose codes never move; `synchronize_model_index` is `pq_index.set_centroids`
    (786 KB device copy), and the hard-negative search (:176) is `rc_adc_search` on CUDA tensors;
  * the int64 copy of all codes the reference registers as a buffer (:161-163, 3.4 GB at M = 48) is not made: rows of the
    resident uint8 codes are gathered and decoded directly (`rc_pq_decode` takes uint8), with the scatter-add backward
    into the centroids (`rc_pq_decode_bwd`).

Around it, with the reference's names (finetune_jpq.py:31-139,246-373): `DataTrainingArguments`, `JPQFinetuneArguments`,
`FinetuneQueryCollator`, `QueryDataset`, `JPQ_SyncIndex_Callback` and the HF-Trainer subclass `JPQFinetuner` on the
transformers 5.x Trainer.  `jpq_step_end` is what the two callbacks do after each optimiser step, for callers that run
their own loop.  Validation (`JPQFinetuner.evaluate`) searches the resident training index: no clone, no second copy of
the codes.
"""
from __future__ import annotations

import inspect
import logging
import os
import random
from collections import defaultdict
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import numpy as np
import torch
from torch import nn
from torch.utils.data import Dataset
from transformers import Trainer, TrainerCallback, TrainingArguments

from ... import ops
from ...index import PQIndex
from ..repconc.finetune_repconc import (RepCONC_Norm_Centroid_Callback, inference_settings, map_evaluation_strategy,
                                        tokenizer_keywords, validation_max_length, validation_metrics)
from ..repconc.modeling_repconc import RepCONC

logger = logging.getLogger(__name__)


@dataclass
class DataTrainingArguments:
    """finetune_jpq.py:31-37."""
    qrel_path: str = field()
    query_path: str = field()
    valid_qrel_path: str = field()
    valid_query_path: str = field()
    max_query_len: int = field()


@dataclass
class JPQFinetuneArguments(TrainingArguments):
    """finetune_jpq.py:40-49, plus this package's two switches and the two command-line compatibility fields of stage 1."""
    dynamic_topk_negative: int = field(default=200)
    centroid_learning_rate: float = field(default=1e-3)
    temperature: float = field(default=1.0)
    seed: int = field(default=2023)
    remove_unused_columns: Optional[bool] = field(default=False)
    head: str = field(default="decode", metadata={"help": "decode: rows decoded then scored; fused: ops.jpq_scores (deterministic)",
                                                  "choices": ["decode", "fused"]})
    deterministic_decode: bool = field(default=False, metadata={"help": "fixed-order (bit-reproducible) centroid gradient of decode"})
    evaluation_strategy: Optional[str] = field(default=None, metadata={"help": "the recipes' name of --eval_strategy"})
    overwrite_output_dir: bool = field(default=False, metadata={"help": "resume from the last checkpoint of a used output_dir"})

    def __post_init__(self):
        map_evaluation_strategy(self)
        super().__post_init__()


class FinetuneQueryCollator:
    """Tokenises the queries of a batch; the query offsets travel along as `qids`.  finetune_jpq.py:53-83."""

    def __init__(self, tokenizer, max_query_len: int):
        self.tokenizer, self.max_query_len = tokenizer, max_query_len
        try:
            typed = "input_text_type" in inspect.signature(tokenizer.__call__).parameters
        except (TypeError, ValueError):
            typed = False
        self.input_query_text_type = {"input_text_type": "query"} if typed else {}

    def __call__(self, features: List[Dict[str, Any]]) -> Dict[str, Any]:
        query_input = self.tokenizer([f["query"] for f in features], padding=True, return_tensors="pt",
                                     add_special_tokens=True, return_attention_mask=True, return_token_type_ids=False,
                                     truncation=True, max_length=self.max_query_len, **self.input_query_text_type)
        return {"query_input_ids": query_input["input_ids"], "query_attention_mask": query_input["attention_mask"],
                "qids": torch.tensor([f["qid"] for f in features], dtype=torch.long)}


class QueryDataset(Dataset):
    """One item per training query that has a positive: {"query", "qid"}.  Queries are addressed by line offset in
    `query_path`, documents by their row in the index (`index_doc_ids`, the corpus_ids.npy next to the index file);
    `get_qrels()` is {query offset: [index rows]} — what `JPQ` takes.  finetune_jpq.py:86-139."""

    def __init__(self, tokenizer, qrel_path: str, query_path: str, max_query_len: int, index_doc_ids, rel_threshold=1,
                 verbose=True):
        super().__init__()
        self.tokenizer = tokenizer
        docid2offset = {str(docid): i for i, docid in enumerate(np.asarray(index_doc_ids).tolist())}
        self.queries, qid2offset = [], {}
        with open(query_path) as f:
            for i, line in enumerate(f):
                qid, query = line.split("\t")
                qid2offset[qid] = i
                self.queries.append(query.strip())
        qrels = defaultdict(list)
        with open(qrel_path) as f:
            for lineno, line in enumerate(f, 1):
                qid, _, docid, rel = line.split()
                if int(rel) < rel_threshold:
                    continue
                if qid not in qid2offset:
                    raise ValueError(f"{qrel_path}:{lineno}: query {qid!r} is not in {query_path}")
                if docid not in docid2offset:
                    raise ValueError(f"{qrel_path}:{lineno}: document {docid!r} is not among the {len(docid2offset)} ids of the index")
                qrels[qid2offset[qid]].append(docid2offset[docid])
        self.qrels = dict(qrels)
        self.qids = sorted(self.qrels)
        self.max_query_len = max_query_len
        if verbose:
            logger.info("%d training queries with a positive, %d queries, %d index rows", len(self.qids), len(self.queries),
                        len(docid2offset))

    def get_qrels(self):
        return self.qrels

    def __len__(self):
        return len(self.qids)

    def __getitem__(self, index):
        qid = self.qids[index]
        return {"query": self.queries[qid], "qid": qid}


class JPQ(nn.Module):
    def __init__(self, repconc: RepCONC, pq_index: PQIndex, qrels: Dict[int, List[int]], neg_top_k: int,
                 temperature: float, gpu_id=None, head: str = "decode"):
        super().__init__()
        if head not in ("decode", "fused"):
            raise ValueError(f'head must be "decode" or "fused", got {head!r}')
        self.head = head
        self.repconc = repconc
        self.qrels = qrels
        self.neg_top_k = neg_top_k
        self.temperature = temperature
        self.pq_index = pq_index
        self.gpu_id = gpu_id            # kept for signature compatibility: the index already lives on its device
        self.synchronize_model_index()

    @property
    def codes(self) -> torch.Tensor:
        """uint8 [N, M], the index's own resident codes (the reference keeps a second, int64 copy)."""
        return self.pq_index.codes

    def _decode_rows(self, pids: torch.Tensor) -> torch.Tensor:
        rows = self.pq_index.codes.index_select(0, pids.reshape(-1))
        # differentiable w.r.t. the centroids; the model's switch picks the backward (fixed-order when set: a reproducible step)
        return ops.decode(rows, self.repconc.centroids, self.repconc.deterministic_decode)

    def forward(self, query_input_ids: torch.Tensor, query_attention_mask: torch.Tensor, qids: torch.Tensor):
        query_embeds = self.repconc(query_input_ids, query_attention_mask, return_code=False,
                                    return_quantized_embedding=False).continuous_embeds          # [nq, D]
        with torch.no_grad():                                                                     # :176
            neg_pids = self.pq_index.search(query_embeds.detach().float().contiguous(), self.neg_top_k)[1]
        if self.head == "fused":
            return {"loss": self._fused_loss(query_embeds, neg_pids, qids)}
        nq, k = neg_pids.shape
        # an index with fewer than neg_top_k rows pads the result with id -1: those slots decode row 0 and are then
        # pushed out of the softmax (the reference would index with -1, i.e. silently use the LAST row)
        empty = neg_pids < 0
        neg_doc_embeds = self._decode_rows(neg_pids.clamp_min(0)).reshape(nq, k, -1)
        neg_masks = self._compute_negative_mask(qids, neg_pids)
        query_negdoc_scores = (query_embeds.unsqueeze(1) * neg_doc_embeds).sum(-1) / self.temperature
        query_negdoc_scores = query_negdoc_scores.masked_fill(empty, -10000.0)
        pos_pids = torch.tensor([random.choice(self.qrels[int(q)]) for q in qids.tolist()], dtype=torch.int64,
                                device=neg_pids.device)
        rel_doc_embeds = self._decode_rows(pos_pids)
        query_reldoc_scores = (query_embeds * rel_doc_embeds).sum(-1, keepdim=True) / self.temperature
        loss = self.compute_loss(query_reldoc_scores, query_negdoc_scores, neg_masks)
        return {"loss": loss}

    def _fused_loss(self, query_embeds: torch.Tensor, neg_pids: torch.Tensor, qids: torch.Tensor) -> torch.Tensor:
        """head="fused": the positive and the retrieved ids scored by ONE ops.jpq_scores call on the resident codes — no
        decoded rows, and both gradients summed in a fixed order, so the step is bit-reproducible.  The -1 padding of a
        short index is a hole of the op (score 0, no gradient) and is pushed out of the softmax as in the decode head."""
        neg_masks = self._compute_negative_mask(qids, neg_pids)
        pos_pids = torch.tensor([random.choice(self.qrels[int(q)]) for q in qids.tolist()], dtype=torch.int64,
                                device=neg_pids.device)
        pids = torch.cat([pos_pids[:, None], neg_pids], 1)
        scores = ops.jpq_scores(query_embeds, self.pq_index.codes, pids, self.repconc.centroids) / self.temperature
        query_reldoc_scores = scores[:, :1]
        query_negdoc_scores = scores[:, 1:].masked_fill(neg_pids < 0, -10000.0)
        return self.compute_loss(query_reldoc_scores, query_negdoc_scores, neg_masks)

    @torch.no_grad()
    def _compute_negative_mask(self, qids: torch.Tensor, docids: torch.Tensor) -> torch.Tensor:
        """1.0 where a retrieved document is a labelled positive of its query (:196-207), [nq, k] fp32."""
        mask = torch.zeros(docids.shape, dtype=torch.bool, device=docids.device)
        for i, q in enumerate(qids.tolist()):
            rel = torch.tensor(self.qrels[int(q)], dtype=docids.dtype, device=docids.device)
            mask[i] = torch.isin(docids[i], rel)
        return mask.float()

    @torch.no_grad()
    def synchronize_model_index(self):
        self.pq_index.set_centroids(self.repconc.centroids.data)

    @torch.no_grad()
    def normalize_centrodis(self):
        self.repconc.normalize_centrodis()

    def state_dict(self, *args, **kwargs):
        return self.repconc.state_dict(*args, **kwargs)

    def load_state_dict(self, state_dict, strict: bool = True):
        missing = self.repconc.load_state_dict(state_dict, strict)
        self.synchronize_model_index()
        return missing

    def compute_loss(self, query_reldoc_scores, query_negdoc_scores, neg_masks):
        """Cross-entropy of the positive against the retrieved documents (:232-246).  As in the reference the mask of
        false negatives is computed but does not enter the loss."""
        scores = torch.hstack((query_reldoc_scores, query_negdoc_scores))
        labels = torch.zeros(scores.size(0), dtype=torch.long, device=scores.device)
        return nn.functional.cross_entropy(scores, labels)


@torch.no_grad()
def jpq_step_end(model: JPQ):
    """What RepCONC_Norm_Centroid_Callback + JPQ_SyncIndex_Callback do after every optimiser step (:249-266)."""
    if getattr(model.repconc.config, "similarity_metric", None) == "METRIC_CENTROID_COS":
        model.normalize_centrodis()
    model.synchronize_model_index()


class JPQ_SyncIndex_Callback(TrainerCallback):
    """After every optimiser step the index scores with the centroids the step produced.  finetune_jpq.py:246-252."""

    def on_step_end(self, args, state, control, model=None, **kwargs):
        model.synchronize_model_index()


class JPQFinetuner(Trainer):
    """`JPQFinetuner(model=JPQ, args=JPQFinetuneArguments, train_dataset=QueryDataset, data_collator=FinetuneQueryCollator,
    tokenizer=..., eval_dataset=(corpus_ids, queries, qrels))`, finetune_jpq.py:255-373.  The training step is the stock
    one (`JPQ.forward` returns {"loss"}).  Centroids are normalised (METRIC_CENTROID_COS) BEFORE they are copied into the
    index: the callbacks run in the order they were added.  Checkpoints hold the wrapped RepCONC in the layout
    `RepCONC.from_pretrained` reads; the stock loading hooks find pytorch_model.bin and hand it to `JPQ.load_state_dict`,
    which re-synchronises the index."""

    def __init__(self, *args, **kwargs):
        tokenizer = tokenizer_keywords(kwargs)
        super().__init__(*args, **kwargs)
        self.tokenizer = tokenizer
        if getattr(self.args, "deterministic_decode", False):
            self.model.repconc.deterministic_decode = True
        if getattr(self.model.repconc.config, "similarity_metric", None) == "METRIC_CENTROID_COS":
            self.add_callback(RepCONC_Norm_Centroid_Callback)
        self.add_callback(JPQ_SyncIndex_Callback)

    def floating_point_ops(self, inputs):
        return 0

    def _save(self, output_dir: Optional[str] = None, state_dict=None):
        """pytorch_model.bin (rotation, centroids, dense_encoder.*) + config + dense_encoder/ (:269-272), the tokenizer and
        the arguments: the directory `RepCONC.from_pretrained` and run_repconc_eval's `replace_pq_centroids` read."""
        output_dir = output_dir or self.args.output_dir
        self.model.repconc.save_pretrained(output_dir)
        if self.tokenizer is not None:
            self.tokenizer.save_pretrained(output_dir)
        torch.save(self.args, os.path.join(output_dir, "training_args.bin"))

    def evaluate(self, eval_dataset=None, ignore_keys=None, metric_key_prefix: str = "eval") -> Dict[str, float]:
        """In-training validation, finetune_jpq.py:274-319: the validation queries encoded in fp32 by the wrapped model and
        searched at depth 10 in the resident index (its centroids are the model's after every step), trec measures at cut
        10 logged as `<prefix>_<measure>`."""
        from ..repconc.evaluate_repconc import batch_search, encode_query
        corpus_ids, queries, qrels = eval_dataset if eval_dataset is not None else self.eval_dataset
        repconc = self.model.repconc
        with inference_settings(self.args):
            query_embeds, query_ids = encode_query(queries, repconc, self.tokenizer, validation_max_length(repconc.config),
                                                   self.args)
        all_topk_scores, all_topk_ids = batch_search(query_ids, query_embeds.astype(np.float32), corpus_ids,
                                                     self.model.pq_index, topk=10, batch_size=512)
        metrics = validation_metrics(qrels, query_ids, all_topk_scores, all_topk_ids, metric_key_prefix)
        self.log(dict(metrics))              # Trainer.log adds its own keys to what it is given
        # as the stock evaluate: clears should_evaluate (else a step that ends an epoch validates twice), feeds early stopping
        self.control = self.callback_handler.on_evaluate(self.args, self.state, self.control, metrics)
        return metrics

    def create_optimizer(self, *args, **kwargs):
        """Three groups as in stage 1: decayed / undecayed encoder parameters, centroids at `centroid_learning_rate` without
        decay; the rotation is a buffer and in none.  finetune_jpq.py:321-373."""
        if self.optimizer is None:
            named = [(n, p) for n, p in self.model.named_parameters() if p.requires_grad]
            no_decay = {n for n, p in named if p.ndim < 2 or "bias" in n or "LayerNorm" in n or "layer_norm" in n}
            groups = [
                {"params": [p for n, p in named if n not in no_decay and "centroids" not in n], "weight_decay": self.args.weight_decay},
                {"params": [p for n, p in named if n in no_decay and "centroids" not in n], "weight_decay": 0.0},
                {"params": [p for n, p in named if "centroids" in n], "weight_decay": 0.0, "lr": self.args.centroid_learning_rate},
            ]
            logger.info("optimizer groups: %s", [len(g["params"]) for g in groups])
            self.optimizer = torch.optim.AdamW(groups, lr=self.args.learning_rate, betas=(self.args.adam_beta1, self.args.adam_beta2),
                                               eps=self.args.adam_epsilon)
        return self.optimizer
