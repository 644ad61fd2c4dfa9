"""`python -m repconc.evaluate.run_dense_eval`: evaluate a dense retriever (the reference's evaluate/run_dense_eval.py,
recipe step 3) — same arguments, same module-level names and positional signatures (the TCT-ColBERT / ANCE examples import
`DataArguments, ModelArguments, EvalArguments, load_or_encode_query, load_or_encode_corpus, search_and_compute_metrics`).

Pipeline: corpus and queries encoded by the dense model (or read from corpus_embeds.npy / corpus_ids.npy and
query_embeds.npy / qids.npy, written only with --save_corpus_embed / --save_query_embed); `create_index` +
`batch_dense_search` (exact fp32 inner product, `rc_dense_search_q`) -> <out_query_dir>/run.tsv -> `pytrec_evaluate` ->
metric.json.  `--index_metric l2` searches by squared Euclidean distance instead and writes the scores -d.  An existing
metric.json skips the search.  Only the main process reads caches, searches and writes files.
`--search_threads` is accepted with no effect (no OpenMP pool).
"""
import json
import logging
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch
import transformers
from transformers import AutoConfig, AutoTokenizer, HfArgumentParser, TrainingArguments, set_seed
from transformers.trainer_utils import is_main_process

from ..models.dense import AutoDense
from ..models.dense.evaluate_dense import (INDEX_METRICS, batch_dense_search, check_index_options, create_index,
                                           encode_dense_corpus, encode_dense_query)
from ..utils.eval_utils import load_corpus, load_queries, pytrec_evaluate, write_run

logger = logging.getLogger(__name__)


@dataclass
class DataArguments:
    """run_dense_eval.py:36-50."""
    corpus_path: str = field()
    out_corpus_dir: str = field()
    query_path: str = field()
    out_query_dir: str = field()
    qrel_path: Optional[str] = field(default=None)
    save_corpus_embed: bool = field(default=False)
    save_query_embed: bool = field(default=False)


@dataclass
class ModelArguments:
    """run_dense_eval.py:53-57: `similarity_metric` / `pooling` override the model config when given."""
    model_name_or_path: str = field()
    max_seq_length: Optional[int] = field(default=512)
    similarity_metric: Optional[str] = field(default=None, metadata={"help": "if None, keep the config's value"})
    pooling: Optional[str] = field(default=None, metadata={"help": "if None, keep the config's value",
                                                           "choices": ["cls", "mean"]})


@dataclass
class EvalArguments(TrainingArguments):
    """run_dense_eval.py:60-68."""
    topk: int = field(default=100)
    search_threads: int = field(default=60)
    search_batch: int = field(default=1200)
    index_float16: bool = field(default=False, metadata={"help": "store the corpus as fp16 (half the memory; vectors and "
                                                                  "queries are rounded to fp16, the search stays exact)"})
    index_int8: bool = field(default=False, metadata={"help": "store the corpus as 8-bit scalar-quantiser codes (a quarter of the "
                                                               "memory; flat inner-product index only, trained on the corpus; "
                                                               "scores are exact for the decoded vectors)"})
    index_screen: str = field(default="fp32", metadata={"help": "fp32, or bf16x3: the fp32 index with its candidates chosen on "
                                                                "the bf16 matrix cores (same results; not with index_float16)"})
    index_metric: str = field(default="ip", metadata={"help": "ip: inner product; l2: squared Euclidean distance, smallest first "
                                                              "(run.tsv then holds the scores -d)",
                                                      "choices": list(INDEX_METRICS)})
    index_nlist: int = field(default=0, metadata={"help": "0: the flat index (every row is scored); > 0: an exact IVF index of that "
                                                          "many cells (IVFFlatIndex: only the rows of the probed cells are scored; "
                                                          "not with index_screen bf16x3)"})
    index_nprobe: int = field(default=8, metadata={"help": "cells probed per query when index_nlist > 0 (they should hold at "
                                                           "least topk rows)"})
    remove_unused_columns: Optional[bool] = field(default=False)


def load_or_encode_query(model, tokenizer, query_path, out_query_dir, model_args, data_args, eval_args):
    """(query_embeds, query_ids); non-main processes get (None, None) when the cache exists.  run_dense_eval.py:71-88."""
    out_query_embed_path = os.path.join(out_query_dir, "query_embeds.npy")
    out_query_ids_path = os.path.join(out_query_dir, "qids.npy")
    main_process = is_main_process(eval_args.local_rank)
    if os.path.exists(out_query_embed_path) and os.path.exists(out_query_ids_path):
        if not main_process:
            return None, None
        logger.info("Load pre-computed query representations")
        return np.load(out_query_embed_path), np.load(out_query_ids_path)
    queries = load_queries(query_path)
    query_embeds, query_ids = encode_dense_query(queries, model, tokenizer, model_args.max_seq_length, eval_args)
    if main_process and data_args.save_query_embed:
        os.makedirs(out_query_dir, exist_ok=True)
        np.save(out_query_embed_path, query_embeds)
        np.save(out_query_ids_path, query_ids)
    return query_embeds, query_ids


def load_or_encode_corpus(model, tokenizer, model_args, data_args, eval_args):
    """(corpus_embeds, corpus_ids); non-main processes get (None, None) when the cache exists.  run_dense_eval.py:91-108."""
    out_corpus_embed_path = os.path.join(data_args.out_corpus_dir, "corpus_embeds.npy")
    out_corpus_ids_path = os.path.join(data_args.out_corpus_dir, "corpus_ids.npy")
    main_process = is_main_process(eval_args.local_rank)
    if os.path.exists(out_corpus_embed_path) and os.path.exists(out_corpus_ids_path):
        if not main_process:
            return None, None
        logger.info("Load pre-computed corpus representations")
        return np.load(out_corpus_embed_path), np.load(out_corpus_ids_path)
    corpus = load_corpus(data_args.corpus_path, tokenizer.sep_token, verbose=main_process)
    corpus_embeds, corpus_ids = encode_dense_corpus(corpus, model, tokenizer, model_args.max_seq_length, eval_args)
    if main_process and data_args.save_corpus_embed:
        os.makedirs(data_args.out_corpus_dir, exist_ok=True)
        np.save(out_corpus_embed_path, corpus_embeds)
        np.save(out_corpus_ids_path, corpus_ids)
    return corpus_embeds, corpus_ids


def search_and_compute_metrics(corpus_embeds, corpus_ids, query_embeds, query_ids, out_metric_path, out_query_dir,
                               qrel_path, eval_args):
    """Exact search on the GPU, run.tsv, and with a qrels file metric.json.  run_dense_eval.py:111-127.  index_metric "l2":
    the scores written are -d, exactly: run.tsv and trec_eval rank by descending score."""
    metric = getattr(eval_args, "index_metric", "ip")
    index = create_index(corpus_embeds, use_float16=getattr(eval_args, "index_float16", False),
                         screen=getattr(eval_args, "index_screen", "fp32"), metric=metric,
                         nlist=getattr(eval_args, "index_nlist", 0), nprobe=getattr(eval_args, "index_nprobe", 8),
                         storage="int8" if getattr(eval_args, "index_int8", False) else None)
    all_topk_scores, all_topk_ids = batch_dense_search(query_ids, query_embeds, corpus_ids, index, eval_args.topk,
                                                       batch_size=eval_args.search_batch)
    if metric == "l2":
        all_topk_scores = -all_topk_scores
    out_run_path = os.path.join(out_query_dir, "run.tsv")
    write_run(out_run_path, query_ids, all_topk_scores, all_topk_ids)
    if qrel_path is None:
        return
    metric_scores = pytrec_evaluate(qrel_path, out_run_path)
    for k, v in metric_scores.items():
        if k != "perquery":
            logger.info(v)
    with open(out_metric_path, "w") as f:
        json.dump(metric_scores, f, indent=1)


def main(argv=None):
    parser = HfArgumentParser((ModelArguments, DataArguments, EvalArguments))
    model_args, data_args, eval_args = parser.parse_args_into_dataclasses(argv)
    check_index_options(eval_args.index_metric, eval_args.index_float16, eval_args.index_screen,
                        eval_args.index_nlist, "int8" if eval_args.index_int8 else None)                   # before encoding
    main_process = is_main_process(eval_args.local_rank)
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s -   %(message)s", datefmt="%m/%d/%Y %H:%M:%S",
                        level=logging.INFO if main_process else logging.WARN)
    if main_process:
        transformers.utils.logging.set_verbosity_info()
        transformers.utils.logging.enable_default_handler()
        transformers.utils.logging.enable_explicit_format()
    set_seed(2022)

    tokenizer = AutoTokenizer.from_pretrained(model_args.model_name_or_path)
    config = AutoConfig.from_pretrained(model_args.model_name_or_path)
    if model_args.similarity_metric is not None:
        config.similarity_metric = model_args.similarity_metric
    if model_args.pooling is not None:
        config.pooling = model_args.pooling
    model = AutoDense.from_pretrained(model_args.model_name_or_path, config=config).to(eval_args.device)

    corpus_embeds, corpus_ids = load_or_encode_corpus(model, tokenizer, model_args, data_args, eval_args)
    query_embeds, query_ids = load_or_encode_query(model, tokenizer, data_args.query_path, data_args.out_query_dir,
                                                   model_args, data_args, eval_args)
    out_metric_path = os.path.join(data_args.out_query_dir, "metric.json")
    torch.cuda.empty_cache()
    if main_process and not os.path.exists(out_metric_path):
        os.makedirs(data_args.out_query_dir, exist_ok=True)
        search_and_compute_metrics(corpus_embeds, corpus_ids, query_embeds, query_ids, out_metric_path,
                                   data_args.out_query_dir, data_args.qrel_path, eval_args)
    else:
        logger.info("Skip search process because metric.json file already exists. ")


if __name__ == "__main__":
    main()
