"""`python -m repconc.evaluate.run_repconc_eval`: evaluate a RepCONC model (the reference's evaluate/run_repconc_eval.py,
called by the recipes' MS MARCO dev, BEIR, hard-negative and after-JPQ steps) — same arguments, same module-level names and
positional signatures (the TCT-ColBERT / ANCE examples import `search_and_compute_metrics`).

Pipeline: <out_corpus_dir>/index + corpus_ids.npy (the IndexPQ file, repconc_amd.faiss_io) or, when absent, the corpus
encoded to codes by the doc encoder (`rc_pq_assign_nearest`); <out_query_dir>/codes.npy + qids.npy (the continuous query
embeddings, named as in the reference) or the queries encoded; the query encoder's centroids copied into the index;
`batch_search` (`rc_adc_search`) -> <out_query_dir>/run.tsv -> `pytrec_evaluate` -> metric.json.  Only the main process
writes caches and searches.  `--threads` is accepted with no effect (no OpenMP pool); `--cpu_search` is refused: there is
no CPU search path.
"""
import json
import logging
import os

import numpy as np
import transformers
from transformers import AutoTokenizer, HfArgumentParser, set_seed
from transformers.trainer_utils import is_main_process

from ..faiss_io import load_index_dir, save_index_dir
from ..models.repconc import RepCONC
from ..models.repconc.evaluate_repconc import (EvalArguments, ModelArguments, batch_search, encode_corpus, encode_query,
                                               from_pq_to_ivfpq, load_index_to_gpu)
from ..utils.eval_utils import (DataArguments, load_beir_corpus, load_beir_qrels, load_beir_queries, load_corpus,
                                load_queries, pytrec_evaluate, write_run)

logger = logging.getLogger(__name__)

CPU_SEARCH_REFUSED = "--cpu_search: this package has no CPU search path; the search runs on the GPU (drop the flag)"


def _load_texts(data_args: DataArguments, which: str, sep_token=None, verbose=True):
    if data_args.data_format == "msmarco":
        return load_corpus(data_args.corpus_path, sep_token, verbose) if which == "corpus" else load_queries(data_args.query_path)
    if data_args.data_format == "beir":
        return (load_beir_corpus(data_args.corpus_path, sep_token, verbose) if which == "corpus"
                else load_beir_queries(data_args.query_path))
    raise NotImplementedError(data_args.data_format)


def load_or_encode_corpus(model_args: ModelArguments, data_args: DataArguments, eval_args: EvalArguments):
    """(index, corpus_ids): the cached <out_corpus_dir>/index + corpus_ids.npy, else the corpus encoded by the doc encoder
    (cache written by the main process).  run_repconc_eval.py:38-60."""
    out_index_path = os.path.join(data_args.out_corpus_dir, "index")
    out_corpus_ids_path = os.path.join(data_args.out_corpus_dir, "corpus_ids.npy")
    if os.path.exists(out_index_path) and os.path.exists(out_corpus_ids_path):
        index, corpus_ids = load_index_dir(data_args.out_corpus_dir)
        logger.info("Load pre-computed corpus representations")
        return index, corpus_ids
    doc_tokenizer = AutoTokenizer.from_pretrained(model_args.doc_encoder_path)
    doc_encoder = RepCONC.from_pretrained(model_args.doc_encoder_path, False, None, None).to(eval_args.device)
    corpus = _load_texts(data_args, "corpus", doc_tokenizer.sep_token, is_main_process(eval_args.local_rank))
    index, corpus_ids = encode_corpus(corpus, doc_encoder, doc_tokenizer, model_args.max_seq_length, eval_args)
    if is_main_process(eval_args.local_rank):
        save_index_dir(index, corpus_ids, data_args.out_corpus_dir)
    return index, corpus_ids


def load_or_encode_queries(model_args: ModelArguments, data_args: DataArguments, eval_args: EvalArguments):
    """(query_embeds, query_ids): the cached <out_query_dir>/codes.npy + qids.npy, else the queries encoded by the query
    encoder.  run_repconc_eval.py:63-83."""
    out_query_code_path = os.path.join(data_args.out_query_dir, "codes.npy")
    out_query_ids_path = os.path.join(data_args.out_query_dir, "qids.npy")
    if os.path.exists(out_query_code_path) and os.path.exists(out_query_ids_path):
        logger.info("Load pre-computed query representations")
        return np.load(out_query_code_path), np.load(out_query_ids_path)
    query_tokenizer = AutoTokenizer.from_pretrained(model_args.query_encoder_path)
    query_encoder = RepCONC.from_pretrained(model_args.query_encoder_path, False, None, None).to(eval_args.device)
    queries = _load_texts(data_args, "queries")
    query_embeds, query_ids = encode_query(queries, query_encoder, query_tokenizer, model_args.max_seq_length, eval_args)
    if is_main_process(eval_args.local_rank):
        os.makedirs(data_args.out_query_dir, exist_ok=True)
        np.save(out_query_code_path, query_embeds)
        np.save(out_query_ids_path, query_ids)
    return query_embeds, query_ids


def search_and_compute_metrics(index, corpus_ids, query_embeds, query_ids, data_args: DataArguments,
                               eval_args: EvalArguments):
    """Search on the GPU, write run.tsv, and with a qrels file metric.json.  As the reference (run_repconc_eval.py:86-91),
    an existing metric.json is logged but the search still runs and both files are rewritten."""
    out_metric_path = os.path.join(data_args.out_query_dir, "metric.json")
    if os.path.exists(out_metric_path):
        logger.info("Skip search process because metric.json file already exists. ")
    if eval_args.cpu_search:
        raise ValueError(CPU_SEARCH_REFUSED)
    index = load_index_to_gpu(from_pq_to_ivfpq(index))
    all_topk_scores, all_topk_ids = batch_search(query_ids, query_embeds, corpus_ids, index, topk=eval_args.topk,
                                                 batch_size=eval_args.search_batch)
    os.makedirs(data_args.out_query_dir, exist_ok=True)
    out_run_path = os.path.join(data_args.out_query_dir, "run.tsv")
    write_run(out_run_path, query_ids, all_topk_scores, all_topk_ids)
    if data_args.qrel_path is None:
        return
    if data_args.data_format == "msmarco":
        qrels = data_args.qrel_path
    elif data_args.data_format == "beir":
        qrels = load_beir_qrels(data_args.qrel_path)
    else:
        raise NotImplementedError(data_args.data_format)
    metric_scores = pytrec_evaluate(qrels, out_run_path)
    for k, v in metric_scores.items():
        if k != "perquery":
            logger.info(v)
    with open(out_metric_path, "w") as f:
        json.dump(metric_scores, f, indent=1)


def replace_pq_centroids(index, query_encoder_path: str):
    """The query encoder's centroids into the index (the doc encoder's were used to code the corpus).
    run_repconc_eval.py:123-127."""
    query_encoder = RepCONC.from_pretrained(query_encoder_path, False, None, None)
    index.set_centroids(query_encoder.centroids.data)
    return index


def main(argv=None):
    parser = HfArgumentParser((ModelArguments, DataArguments, EvalArguments))
    model_args, data_args, eval_args = parser.parse_args_into_dataclasses(argv)
    if eval_args.cpu_search:
        parser.error(CPU_SEARCH_REFUSED)
    main_process = is_main_process(eval_args.local_rank)
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s -   %(message)s", datefmt="%m/%d/%Y %H:%M:%S",
                        level=logging.INFO if main_process else logging.WARN)
    if main_process:
        transformers.utils.logging.set_verbosity_info()
        transformers.utils.logging.enable_default_handler()
        transformers.utils.logging.enable_explicit_format()
    set_seed(2022)

    index, corpus_ids = load_or_encode_corpus(model_args, data_args, eval_args)
    query_embeds, query_ids = load_or_encode_queries(model_args, data_args, eval_args)
    index = replace_pq_centroids(index, model_args.query_encoder_path)
    if main_process:
        search_and_compute_metrics(index, corpus_ids, query_embeds, query_ids, data_args, eval_args)


if __name__ == "__main__":
    main()
