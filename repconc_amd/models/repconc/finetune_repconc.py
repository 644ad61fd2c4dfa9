"""Stage-1 (constrained clustering) fine-tuning with the reference's names — models/repconc/finetune_repconc.py:
`DataTrainingArguments`, `RepCONCFinetuneArguments`, `FinetuneCollator`, `QDRelDataset`, `RepCONC_Norm_Centroid_Callback`,
`RepCONCFinetuner`, `eval_balance`, `test_quantize` — on the transformers 5.x Trainer and this package's `GradCache`.

What is kept of the reference: the two-pass cached-gradient step (encode every tower without graph
in `cache_chunk_size` chunks -> constrained `quantize` of cat(pos, neg) over the GLOBAL batch -> contrastive loss on
(query, decode(codes)) with false-negative / duplicate masks and dynamic hard negatives -> second pass per chunk with
the cached gradient applied to the continuous embedding (straight-through) and to decode(codes) (-> centroids) plus the
weighted MSE), the cross-rank gather of representations and ids, the three optimiser groups, centroid re-normalisation
for METRIC_CENTROID_COS.  What changed: no use of Trainer members that 5.x dropped (`use_amp`, `scaler`, `use_apex`,
`sharded_ddp`, `_prepare_inputs` on nested dicts), fp16 scaling goes through the accelerator's scaler.
`RepCONCFinetuner.evaluate` is the in-training validation (:530-577); `_save` also writes the tokenizer, so that the output
directory and every checkpoint load with `AutoTokenizer.from_pretrained`; the recipes' `--evaluation_strategy` and
`--overwrite_output_dir` are fields of the arguments.
The arithmetic of quantize / decode / decode-backward / the balance statistics is `repconc_amd.ops`.
"""
from __future__ import annotations

import inspect
import json
import logging
import os
import random
from collections import defaultdict
from contextlib import contextmanager, nullcontext
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import numpy as np
import torch
import torch.distributed as dist
import torch.nn.functional as F
from torch import Tensor, nn
from torch.utils.data import Dataset
from transformers import Trainer, TrainerCallback, TrainingArguments

from ...diagnostics import eval_balance, test_quantize  # noqa: F401  (same names as finetune_repconc.py:580-613)
from ...gradcache import GradCache
from .modeling_repconc import RepCONC

logger = logging.getLogger(__name__)


@dataclass
class DataTrainingArguments:
    qrel_path: str = field()
    query_path: str = field()
    corpus_path: str = field()
    valid_qrel_path: str = field()
    valid_query_path: str = field()
    valid_corpus_path: str = field()
    max_query_len: int = field()
    max_doc_len: int = field()


@dataclass
class RepCONCFinetuneArguments(TrainingArguments):
    """finetune_repconc.py:44-58."""
    negative_per_query: int = field(default=1)
    dynamic_topk_hard_negative: int = field(default=None)
    centroid_learning_rate: float = field(default=1e-3)
    temperature: float = field(default=1.0)
    mse_loss_weight: float = field(default=0)
    not_use_constraint: bool = field(default=False)
    negative: str = field(default="random", metadata={"help": "inbatch, random, or the path of a qid -> [docid] json"})
    cache_chunk_size: int = field(default=-1)
    deterministic_decode: bool = field(default=False, metadata={"help": "fixed-order (bit-reproducible) centroid gradient of decode"})
    fused_contrastive_loss: bool = field(default=False, metadata={"help": "masks, top-k cut and softmax loss in fused HIP kernels after the GEMM"})
    seed: int = field(default=2022)
    remove_unused_columns: Optional[bool] = field(default=False)
    evaluation_strategy: Optional[str] = field(default=None, metadata={"help": "the recipes' name of --eval_strategy"})
    overwrite_output_dir: bool = field(default=False, metadata={"help": "resume from the last checkpoint of a used output_dir"})

    def __post_init__(self):
        map_evaluation_strategy(self)
        super().__post_init__()


def map_evaluation_strategy(args):
    """The recipes pass `--evaluation_strategy`, which TrainingArguments renamed to `eval_strategy`: the old name fills the
    new field before TrainingArguments validates it.  Both given and different is an error."""
    old = args.evaluation_strategy
    if old is None:
        return
    new = getattr(args.eval_strategy, "value", args.eval_strategy)
    if new not in (None, "no") and new != old:
        raise ValueError(f"--evaluation_strategy {old} and --eval_strategy {new} disagree: pass one of them")
    args.eval_strategy = old


def _unwrap(model):
    return model.module if hasattr(model, "module") else model


# the keyword the installed Trainer takes the tokenizer under (`tokenizer` until transformers 4.x, `processing_class` since)
_TOKENIZER_KEYWORD = "processing_class" if "processing_class" in inspect.signature(Trainer.__init__).parameters else "tokenizer"


def tokenizer_keywords(kwargs: Dict[str, Any]):
    """Takes `tokenizer=` (the reference's call) and / or `processing_class=` out of a trainer's keyword arguments and puts
    the tokenizer back under the name the installed Trainer takes.  Returns the tokenizer (None when neither was given)."""
    old, new = kwargs.pop("tokenizer", None), kwargs.pop("processing_class", None)
    if old is not None and new is not None and old is not new and old != new:
        raise ValueError("tokenizer= and processing_class= name two different objects: pass one of them")
    tokenizer = old if old is not None else new
    if tokenizer is not None:
        kwargs[_TOKENIZER_KEYWORD] = tokenizer
    return tokenizer


@contextmanager
def inference_settings(args, model=None):
    """What both trainers switch off while `evaluate` encodes (finetune_repconc.py:539-549, finetune_jpq.py:285-291):
    the arguments' fp16 / bf16 / dataloader_drop_last and, for a model given, its `use_constraint` (validation codes are
    the nearest ones).  Everything is put back on the way out, also when an exception passes through."""
    saved = (args.fp16, args.bf16, args.dataloader_drop_last)
    constraint = model.use_constraint if model is not None else None
    args.fp16, args.bf16, args.dataloader_drop_last = False, False, False
    if model is not None:
        model.use_constraint = False
    try:
        yield
    finally:
        args.fp16, args.bf16, args.dataloader_drop_last = saved
        if model is not None:
            model.use_constraint = constraint


def validation_max_length(config) -> int:
    """The reference encodes the validation texts at 512 tokens (finetune_repconc.py:545-546); an encoder with fewer
    positions takes what it has."""
    return min(512, int(getattr(config, "max_position_embeddings", None) or 512))


def validation_metrics(qrels, query_ids, all_topk_scores, all_topk_ids, metric_key_prefix: str) -> Dict[str, float]:
    """Search result -> {"<prefix>_<measure>"} for every summary measure of `pytrec_evaluate` at cut 10
    (finetune_repconc.py:560-573).  The run dictionary is built from the host arrays in one pass (`tolist()`)."""
    from ...utils.eval_utils import pytrec_evaluate
    run = {str(qid): dict(zip(map(str, row_ids), row_scores))
           for qid, row_scores, row_ids in zip(np.asarray(query_ids).tolist(), np.asarray(all_topk_scores).tolist(),
                                               np.asarray(all_topk_ids).tolist())}
    metrics = {}
    for category, cat_metrics in pytrec_evaluate(qrels, run, k_values=(10,), mrr_k_values=(10,)).items():
        if category == "perquery":
            continue
        for metric, score in cat_metrics.items():
            metrics[f"{metric_key_prefix}_{metric}"] = score
    return metrics


class FinetuneCollator:
    """Tokenises queries, positives and (flattened) negatives of a batch; ids travel along so that the trainer can mask
    in-batch false negatives after the cross-rank gather.  finetune_repconc.py:61-126."""

    def __init__(self, tokenizer, max_query_len: int, max_doc_len: int):
        self.tokenizer, self.max_query_len, self.max_doc_len = tokenizer, max_query_len, max_doc_len
        try:
            typed = "input_text_type" in inspect.signature(tokenizer.__call__).parameters
        except (TypeError, ValueError):
            typed = False
        self._q = {"input_text_type": "query"} if typed else {}
        self._d = {"input_text_type": "doc"} if typed else {}

    def _tok(self, texts, max_len, extra):
        return self.tokenizer(texts, padding=True, return_tensors="pt", add_special_tokens=True, return_attention_mask=True,
                              return_token_type_ids=False, truncation=True, max_length=max_len, **extra)

    def __call__(self, features: List[Dict[str, Any]]) -> Dict[str, Any]:
        batch = {"query_input": self._tok([f["query"] for f in features], self.max_query_len, self._q),
                 "pos_doc_input": self._tok([f["pos_doc"] for f in features], self.max_doc_len, self._d),
                 "qids": torch.tensor([f["qid"] for f in features], dtype=torch.long),
                 "pos_docids": torch.tensor([f["pos_docid"] for f in features], dtype=torch.long)}
        if "neg_docs" in features[0]:
            batch["neg_doc_input"] = self._tok([t for f in features for t in f["neg_docs"]], self.max_doc_len, self._d)
            batch["neg_docids"] = torch.tensor([d for f in features for d in f["neg_docids"]], dtype=torch.long)
        return batch


class QDRelDataset(Dataset):
    """(query, one random positive, `negative_per_query` negatives) per item, texts tokenised later by the collator.
    Queries / documents are addressed by line offset; `negative` = "inbatch" | "random" | path of a json with
    qid -> [docid] hard negatives.  finetune_repconc.py:129-218."""

    def __init__(self, tokenizer, qrel_path, query_path, corpus_path, max_query_len, max_doc_len, negative,
                 negative_per_query, rel_threshold=1, verbose=True):
        self.tokenizer = tokenizer
        self.queries, q_off = [], {}
        with open(query_path) as f:
            for i, line in enumerate(f):
                qid, text = line.split("\t")
                q_off[qid] = i
                self.queries.append(text.strip())
        self.corpus, d_off = [], {}
        with open(corpus_path) as f:
            for i, line in enumerate(f):
                parts = line.strip().split("\t")
                d_off[parts[0]] = i
                self.corpus.append(str(tokenizer.sep_token).join(p.strip() for p in parts[1:]).strip()[:10000])
        qrels = defaultdict(list)
        with open(qrel_path) as f:
            for line in f:
                qid, _, docid, rel = line.split()
                if int(rel) >= rel_threshold:
                    qrels[q_off[qid]].append(d_off[docid])
        self.qrels = dict(qrels)
        self.qids = sorted(self.qrels)
        self.negative_per_query = negative_per_query
        if negative in ("inbatch", "random"):
            self.negative = negative
        else:
            with open(negative) as f:
                self.negative = {q_off[q]: [d_off[d] for d in docs] for q, docs in json.load(f).items()}
        self.max_query_len, self.max_doc_len = max_query_len, max_doc_len

    def get_qrels(self):
        return self.qrels

    def __len__(self):
        return len(self.qids)

    def __getitem__(self, index):
        qid = self.qids[index]
        pos = random.choice(self.qrels[qid])
        item = {"query": self.queries[qid], "pos_doc": self.corpus[pos], "pos_docid": pos, "qid": qid}
        if self.negative == "inbatch":
            assert self.negative_per_query == 0
            return item
        pool = range(len(self.corpus)) if self.negative == "random" else self.negative[qid]
        negs = random.sample(pool, self.negative_per_query)
        item.update(neg_docids=negs, neg_docs=[self.corpus[d] for d in negs])
        return item


class RepCONC_Norm_Centroid_Callback(TrainerCallback):
    def on_step_end(self, args, state, control, model=None, **kwargs):
        _unwrap(model).normalize_centrodis()


class RepCONCFinetuner(Trainer):
    """`RepCONCFinetuner(qrels, model=..., args=RepCONCFinetuneArguments, train_dataset=..., data_collator=...,
    tokenizer=..., eval_dataset=(corpus, queries, qrels))`.  The tokenizer may come as `tokenizer=` (the reference's call,
    run_train_conc.py:129-137) or `processing_class=`; `evaluate` and `_save` use it as `self.tokenizer`.  The validation
    triple is only stored by the base class: `evaluate` is this class's own."""

    def __init__(self, qrels, *args, **kwargs):
        tokenizer = tokenizer_keywords(kwargs)
        super().__init__(*args, **kwargs)
        self.tokenizer = tokenizer
        self.qrels = qrels
        if getattr(self.args, "deterministic_decode", False):
            _unwrap(self.model).deterministic_decode = True
        self._gc_scaler = getattr(getattr(self, "accelerator", None), "scaler", None) if self.args.fp16 else None
        if self.args.cache_chunk_size != -1:
            self.gc = GradCache(models=[self.model], chunk_sizes=self.args.cache_chunk_size,
                                loss_fn=self.compute_contrastive_loss, get_rep_fn=lambda out: out.continuous_embeds,
                                fp16=bool(self.args.fp16 and self._gc_scaler is not None), scaler=self._gc_scaler)
        if getattr(self.model.config, "similarity_metric", None) == "METRIC_CENTROID_COS":
            self.add_callback(RepCONC_Norm_Centroid_Callback)

    # ------------------------------------------------------------------ helpers
    def _world(self):
        return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1

    def _rank(self):
        return dist.get_rank() if self._world() > 1 else 0

    def _to_device(self, td):
        dev = self.args.device
        return {k: v.to(dev, non_blocking=True) for k, v in dict(td).items() if isinstance(v, torch.Tensor)}

    def split_tensor_dict(self, td: Dict[str, Tensor]):
        keys = list(td)
        parts = [td[k].split(self.args.cache_chunk_size) for k in keys]
        return [dict(zip(keys, p)) for p in zip(*parts)]

    def gather_tensors(self, *tt: Tensor):
        """Every rank's rows in rank order, the local rows being the live tensors.  finetune_repconc.py:453-462."""
        if self._world() == 1:
            return list(tt)
        out = []
        for t in tt:
            parts = [torch.empty_like(t) for _ in range(self._world())]
            dist.all_gather(parts, t.contiguous())
            parts[self._rank()] = t
            out.append(torch.cat(parts))
        return out

    def _autocast(self):
        if self.args.bf16:
            return torch.autocast("cuda", dtype=torch.bfloat16)
        if self.args.fp16:
            return torch.autocast("cuda", dtype=torch.float16)
        return nullcontext()

    # ------------------------------------------------------------------ one step
    def training_step(self, model, inputs, num_items_in_batch=None) -> torch.Tensor:
        """finetune_repconc.py:245-281: returns the (detached) contrastive loss; the backward passes happen inside."""
        if self.args.cache_chunk_size == -1:
            raise NotImplementedError("RepCONC stage 1 trains with cached gradients: set --cache_chunk_size")
        if self.args.gradient_accumulation_steps > 1:
            raise ValueError("gradient accumulation is what the gradient cache replaces")
        model.train()
        core = _unwrap(model)
        towers = [("query", self.split_tensor_dict(self._to_device(inputs["query_input"])), None),
                  ("pos", self.split_tensor_dict(self._to_device(inputs["pos_doc_input"])), inputs["pos_docids"])]
        if "neg_doc_input" in inputs:
            towers.append(("neg", self.split_tensor_dict(self._to_device(inputs["neg_doc_input"])), inputs["neg_docids"]))
        reps, rnd = {}, {}
        for name, chunks, _ in towers:
            reps[name], rnd[name] = self.gc.forward_no_grad(model, chunks)
        # constrained clustering over the (global) batch of documents — the hot path (:296-318)
        doc_names = [n for n, _, _ in towers if n != "query"]
        docs = torch.vstack([reps[n] for n in doc_names])
        codes_all = core.quantize(docs)
        codes, quant, off = {}, {}, 0
        for n in doc_names:
            codes[n] = codes_all[off:off + len(reps[n])]
            quant[n] = core.decode(codes[n])
            off += len(reps[n])
        if self.state.global_step % max(int(self.args.logging_steps), 1) == 0:
            self.log(test_quantize(docs, core, self._rank() if self._world() > 1 else -1, block_id=0))
        dev = self.args.device
        qids = inputs["qids"].to(dev).contiguous()
        ids = {n: t.to(dev).contiguous() for n, _, t in towers if t is not None}
        g_query, = self.gather_tensors(reps["query"].contiguous())
        g_quant = {n: self.gather_tensors(quant[n].contiguous())[0] for n in doc_names}
        g_qids, = self.gather_tensors(qids)
        g_ids = {n: self.gather_tensors(ids[n])[0] for n in doc_names}
        all_docs = torch.vstack([g_quant[n] for n in doc_names])
        all_ids = torch.hstack([g_ids[n] for n in doc_names])
        (g_q, g_d), loss = self.gc.build_cache(g_query, all_docs, qids=g_qids, docids=all_ids)
        grads, off = {"query": g_q}, 0
        for n in doc_names:
            grads[n] = g_d[off:off + len(g_quant[n])]
            off += len(g_quant[n])
        self._forward_backward(model, [(chunks, grads[name], rnd[name], codes.get(name)) for name, chunks, _ in towers])
        return loss.detach().float()

    def _forward_backward(self, model, plan):
        """Second pass with graph, chunk by chunk (finetune_repconc.py:346-396).  `plan`: [(chunks, cached grads over the
        GLOBAL rows of that tower, RNG snapshots, local codes | None for the query tower)]."""
        W, r, cs = self._world(), self._rank(), self.args.cache_chunk_size
        scaler = self._gc_scaler
        for ti, (chunks, cache, rnd, codes) in enumerate(plan):
            n_local = sum(next(iter(c.values())).shape[0] for c in chunks)
            assert W * n_local == len(cache), f"{W} * {n_local} != {len(cache)}"
            base = r * n_local
            for ci, chunk in enumerate(chunks):
                lo = ci * cs
                with rnd[ci], self._autocast():
                    if codes is None:
                        out = model(**chunk)
                    else:
                        out = model(discrete_codes=codes[lo:lo + cs], return_quantized_embedding=True, **chunk)
                    n = out.continuous_embeds.shape[0]
                    g = cache[base + lo: base + lo + n].flatten()
                    obj = torch.dot(g, out.continuous_embeds.flatten().to(g.dtype))
                    if codes is not None:
                        obj = obj + torch.dot(g, out.quantized_embeds.flatten().to(g.dtype))
                        mse = ((out.quantized_embeds - out.continuous_embeds) ** 2).sum(-1).mean() * self.args.mse_loss_weight
                        obj = obj + (scaler.scale(mse) if scaler is not None else mse)
                last = ci + 1 == len(chunks) and ti + 1 == len(plan)
                sync = nullcontext() if (W == 1 or last or not hasattr(model, "no_sync")) else model.no_sync()
                with sync:
                    obj.backward()

    # ------------------------------------------------------------------ loss
    def compute_contrastive_loss(self, query_embeds, doc_embeds, qids, docids):
        """In-batch softmax over every gathered document, labels on the diagonal.  finetune_repconc.py:398-431."""
        if getattr(self.args, "fused_contrastive_loss", False):
            return self._fused_contrastive_loss(query_embeds, doc_embeds, qids, docids)
        nq = query_embeds.shape[0]
        labels = torch.arange(nq, dtype=torch.long, device=query_embeds.device)
        mask = torch.logical_or(self._compute_mask_for_false_negative(qids, docids),
                                self._compute_mask_for_duplicate_negative(qids, docids)).float()
        sim = query_embeds @ doc_embeds.T
        if getattr(self.model.config, "similarity_metric", None) == "METRIC_CENTROID_COS":
            sim = sim / self.model.config.MCQ_M
        if self.args.temperature != 1:
            sim = sim / self.args.temperature
        sim = sim - 10000.0 * mask
        topk = self.args.dynamic_topk_hard_negative
        if topk is not None and topk > 0:
            drop = torch.ones_like(sim)
            neg = sim.detach().clone()
            neg.scatter_(1, labels[:, None], -10000.0)
            drop.scatter_(1, torch.topk(neg, topk).indices, 0)
            drop.scatter_(1, labels[:, None], 0)
            sim = sim - 10000.0 * drop
        return F.cross_entropy(sim, labels)

    def _fused_contrastive_loss(self, query_embeds, doc_embeds, qids, docids):
        """The same loss with everything after the GEMM in ops.contrastive_loss (csrc/contrastive.hip): the similarity and its
        two divisions are the torch ops of the composition under the ambient autocast, the positives of the batch's queries go
        to the device as a CSR built from one `tolist()`."""
        from ... import ops
        sim = query_embeds @ doc_embeds.T
        if getattr(self.model.config, "similarity_metric", None) == "METRIC_CENTROID_COS":
            sim = sim / self.model.config.MCQ_M
        if self.args.temperature != 1:
            sim = sim / self.args.temperature
        off, rel = [0], []
        for qid in qids.tolist():
            rel.extend(self.qrels.get(qid, ()))
            off.append(len(rel))
        dev = sim.device
        topk = self.args.dynamic_topk_hard_negative
        if topk is not None and topk > sim.shape[1]:
            raise ValueError(f"dynamic_topk_hard_negative = {topk} exceeds the {sim.shape[1]} documents of the gathered batch")
        return ops.contrastive_loss(sim.float(), docids, torch.tensor(off, dtype=torch.long, device=dev),
                                    torch.tensor(rel, dtype=torch.long, device=dev), topk if topk is not None and topk > 0 else 0)

    @torch.no_grad()
    def _compute_mask_for_false_negative(self, qids, docids):
        mask = torch.zeros((len(qids), len(docids)), dtype=torch.bool, device=qids.device)
        for i, qid in enumerate(qids.tolist()):
            for d in self.qrels.get(qid, ()):
                mask[i] |= docids == d
        mask.fill_diagonal_(False)
        return mask

    @torch.no_grad()
    def _compute_mask_for_duplicate_negative(self, qids, docids):
        dup = torch.triu(docids[:, None] == docids[None, :], diagonal=1).any(dim=0, keepdim=True).repeat(len(qids), 1)
        dup.fill_diagonal_(False)
        return dup

    # ------------------------------------------------------------------ Trainer plumbing
    def floating_point_ops(self, inputs):
        return 0

    def _save(self, output_dir: Optional[str] = None, state_dict=None):
        """pytorch_model.bin + config + dense_encoder/ (:471-474), the tokenizer and the arguments: what
        `RepCONC.from_pretrained` / `AutoTokenizer.from_pretrained` read, and — pytorch_model.bin being the name the stock
        `_load_from_checkpoint` / `_load_best_model` look for — what resume and `load_best_model_at_end` load back."""
        output_dir = output_dir or self.args.output_dir
        _unwrap(self.model).save_pretrained(output_dir)
        if self.tokenizer is not None:
            self.tokenizer.save_pretrained(output_dir)
        torch.save(self.args, os.path.join(output_dir, "training_args.bin"))

    def evaluate(self, eval_dataset=None, ignore_keys=None, metric_key_prefix: str = "eval") -> Dict[str, float]:
        """In-training validation, finetune_repconc.py:530-577: the validation corpus coded by nearest centroid and the
        queries encoded in fp32, the codes searched at depth 10, trec measures at cut 10 logged as `<prefix>_<measure>`.
        The model is left in eval mode; `training_step` sets its own."""
        from .evaluate_repconc import batch_search, encode_corpus, encode_query, from_pq_to_ivfpq, load_index_to_gpu
        corpus, queries, qrels = eval_dataset if eval_dataset is not None else self.eval_dataset
        core = _unwrap(self.model)
        max_length = validation_max_length(core.config)
        with inference_settings(self.args, core):
            index, corpus_ids = encode_corpus(corpus, core, self.tokenizer, max_length, self.args)
            query_embeds, query_ids = encode_query(queries, core, self.tokenizer, max_length, self.args)
        index = load_index_to_gpu(from_pq_to_ivfpq(index), index.device.index)      # the model's device, as :553
        all_topk_scores, all_topk_ids = batch_search(query_ids, query_embeds.astype(np.float32), corpus_ids, index,
                                                     topk=10, batch_size=512)
        metrics = validation_metrics(qrels, query_ids, all_topk_scores, all_topk_ids, metric_key_prefix)
        self.log(dict(metrics))              # Trainer.log adds its own keys to what it is given
        # as the stock evaluate: clears should_evaluate (else a step that ends an epoch validates twice), feeds early stopping
        self.control = self.callback_handler.on_evaluate(self.args, self.state, self.control, metrics)
        return metrics

    def create_optimizer(self, *args, **kwargs):
        """Three groups: decayed / undecayed encoder parameters, centroids at `centroid_learning_rate` without decay.
        finetune_repconc.py:476-528."""
        if self.optimizer is None:
            core = _unwrap(self.model)
            no_decay = {n for n, p in core.named_parameters() if p.ndim < 2 or "bias" in n or "LayerNorm" in n or "layer_norm" in n}
            named = [(n, p) for n, p in core.named_parameters() if p.requires_grad]
            groups = [
                {"params": [p for n, p in named if n not in no_decay and "centroids" not in n], "weight_decay": self.args.weight_decay},
                {"params": [p for n, p in named if n in no_decay and "centroids" not in n], "weight_decay": 0.0},
                {"params": [p for n, p in named if "centroids" in n], "weight_decay": 0.0, "lr": self.args.centroid_learning_rate},
            ]
            logger.info("optimizer groups: %s", [len(g["params"]) for g in groups])
            self.optimizer = torch.optim.AdamW(groups, lr=self.args.learning_rate, betas=(self.args.adam_beta1, self.args.adam_beta2),
                                               eps=self.args.adam_epsilon)
        return self.optimizer
