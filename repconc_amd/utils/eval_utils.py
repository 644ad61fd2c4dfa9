"""Data plumbing of the evaluation scripts, with the reference's names (utils/eval_utils.py): TSV and BEIR loaders, the
text dataset / collator pair the encoders are fed from, the TREC run writer and the rank metrics.  Harness code around
the hot path — kept small, no third-party metric package (the reference scores with pytrec_eval, which is not
installable offline): `pytrec_evaluate` restates trec_eval's measures (its docstring states the rules), and
`mrr_at_k` / `recall_at_k` restate the two numbers the recipes report: MRR@k = mean over queries of 1 / rank of the
first relevant hit within the top k, relevance >= 1, eval_utils.py:136-190)."""
from __future__ import annotations

import csv
import inspect
import json
import math
from dataclasses import dataclass, field
from operator import itemgetter
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch
from torch.utils.data import Dataset


@dataclass
class DataArguments:
    """eval_utils.py:16-30: the data side of evaluate/run_repconc_eval.py."""
    corpus_path: str = field()
    query_path: str = field()
    out_corpus_dir: str = field()
    out_query_dir: str = field()
    qrel_path: Optional[str] = field(default=None)
    data_format: Optional[str] = field(default="msmarco", metadata={"choices": ["msmarco", "beir"]})


def concat_title_body(doc: Dict[str, str]) -> str:
    """A BEIR document as one text: "title. body", or "title body" when the title already ends a sentence."""
    body = doc["text"].strip()
    title = (doc.get("title") or "").strip()
    if not title:
        return body
    return title + (" " if title[-1] in "!.?。！？" else ". ") + body


def load_beir_corpus(corpus_path: str, sep_token: str, verbose: bool = True) -> Dict[str, str]:
    """corpus.jsonl ({"_id", "title", "text"} per line) -> {_id: title + body, 10 000 characters kept}.  `sep_token` and
    `verbose` are accepted for the reference's signature; the title is joined as text, not with the separator."""
    corpus = {}
    with open(corpus_path, encoding="utf-8") as f:
        for line in f:
            doc = json.loads(line)
            corpus[doc["_id"]] = concat_title_body(doc)[:10000]
    return corpus


def load_beir_queries(query_path: str) -> Dict[str, str]:
    queries = {}
    with open(query_path, encoding="utf-8") as f:
        for line in f:
            q = json.loads(line)
            queries[q["_id"]] = q["text"].strip()
    return queries


def load_beir_qrels(qrel_path: str) -> Dict[str, Dict[str, int]]:
    """qrels/<split>.tsv: a header row, then query-id \\t corpus-id \\t score."""
    qrels: Dict[str, Dict[str, int]] = {}
    with open(qrel_path, encoding="utf-8", newline="") as f:
        reader = csv.reader(f, delimiter="\t", quoting=csv.QUOTE_MINIMAL)
        next(reader)
        for row in reader:
            qrels.setdefault(row[0], {})[row[1]] = int(row[2])
    return qrels


def load_corpus(corpus_path: str, sep_token: str, verbose: bool = True) -> Dict[str, str]:
    """id \\t field [\\t field ...] per line; fields joined with the tokenizer's separator, 10 000 characters kept."""
    corpus = {}
    with open(corpus_path) as f:
        for line in f:
            parts = line.strip().split("\t")
            corpus[parts[0]] = sep_token.join(p.strip() for p in parts[1:])[:10000]
    return corpus


def load_queries(query_path: str) -> Dict[str, str]:
    queries = {}
    with open(query_path) as f:
        for line in f:
            qid, text = line.split("\t")
            queries[qid] = text
    return queries


class TextDataset(Dataset):
    """A list of texts, optionally paired with integer ids that travel through the collator as `text_ids`."""

    def __init__(self, text_lst: List[str], text_ids: Optional[List[int]] = None):
        assert text_ids is None or len(text_ids) == len(text_lst)
        self.text_lst, self.text_ids = text_lst, text_ids

    def __len__(self):
        return len(self.text_lst)

    def __getitem__(self, i):
        return self.text_lst[i] if self.text_ids is None else (self.text_ids[i], self.text_lst[i])


def get_collator_func(tokenizer, max_length: int, input_text_type: str):
    """Batch of texts (or (id, text) pairs) -> input_ids / attention_mask (/ text_ids).  Tokenizers whose __call__ takes
    `input_text_type` (the TCT-ColBERT recipe's) are told whether they see queries or documents."""
    try:
        extra = {"input_text_type": input_text_type} if "input_text_type" in inspect.signature(tokenizer.__call__).parameters else {}
    except (TypeError, ValueError):
        extra = {}

    def collate(batch):
        paired = isinstance(batch[0], tuple)
        texts = [b[1] for b in batch] if paired else list(batch)
        enc = tokenizer(texts, padding=True, truncation=True, max_length=max_length, **extra)
        out = {"input_ids": torch.as_tensor(enc["input_ids"], dtype=torch.long),
               "attention_mask": torch.as_tensor(enc["attention_mask"], dtype=torch.long)}
        if paired:
            out["text_ids"] = torch.as_tensor([b[0] for b in batch], dtype=torch.long)
        return out
    return collate


def write_run(out_run_path: str, query_ids, all_topk_scores, all_topk_ids):
    """The TREC run file of both evaluation scripts: `qid \\t Q0 \\t docid \\t rank \\t score \\t System`, ranks from 1.
    Byte for byte the reference's per-element loop (run_repconc_eval.py:102-105, run_dense_eval.py:117-120): `.tolist()`
    turns an fp32 score into the same Python float as `.item()` (its float64 widening, written as its repr) and an id
    into the str / int that was loaded."""
    qids = np.asarray(query_ids).tolist()
    scores, ids = np.asarray(all_topk_scores).tolist(), np.asarray(all_topk_ids).tolist()
    assert len(qids) == len(scores) == len(ids)
    with open(out_run_path, "w") as out:
        for qid, row_scores, row_ids in zip(qids, scores, ids):
            out.write("".join(f"{qid}\tQ0\t{docid}\t{rank}\t{score}\tSystem\n"
                              for rank, (score, docid) in enumerate(zip(row_scores, row_ids), 1)))


def truncate_run(run: Dict[str, Dict[str, float]], topk: int) -> Dict[str, Dict[str, float]]:
    """Per query the `topk` best-scored documents; equal scores keep insertion order (file order for a parsed run)."""
    return {qid: dict(sorted(docs.items(), key=itemgetter(1), reverse=True)[:topk]) for qid, docs in run.items()}


def _parse_qrel(path: str) -> Dict[str, Dict[str, int]]:
    qrel: Dict[str, Dict[str, int]] = {}
    with open(path) as f:
        for line in f:
            parts = line.split()
            if parts:
                qrel.setdefault(parts[0], {})[parts[2]] = int(parts[3])
    return qrel


def _parse_run(path: str) -> Dict[str, Dict[str, float]]:
    run: Dict[str, Dict[str, float]] = {}
    qid, docs = None, None
    with open(path) as f:
        for line in f:
            parts = line.split()
            if not parts:
                continue
            if parts[0] != qid:                         # a run file lists a query's lines together: one lookup each
                qid = parts[0]
                docs = run.setdefault(qid, {})
            docs[parts[2]] = float(parts[4])
    return run


def _ranking(docs: Dict[str, float]) -> List[str]:
    """trec_eval's order: score descending, equal scores by docid descending (strcmp)."""
    return [d for d, _ in sorted(docs.items(), key=itemgetter(1, 0), reverse=True)]


def _cut_measures(ranked: List[str], judged: Dict[str, int], k_values, relevance_level: int) -> Dict[str, float]:
    """ndcg_cut_k / map_cut_k / recall_k / P_k of one query, one walk down the ranking."""
    num_rel = sum(1 for r in judged.values() if r >= relevance_level)
    ideal = sorted((r for r in judged.values() if r > 0), reverse=True)
    depth = max(k_values)
    hits_at, ap_at, dcg_at, idcg_at = [0], [0.0], [0.0], [0.0]      # prefix sums over ranks 1..depth
    for r in range(1, depth + 1):
        rel = judged.get(ranked[r - 1]) if r <= len(ranked) else None          # None: unjudged or not retrieved
        hit = rel is not None and rel >= relevance_level
        rel = rel or 0
        hits_at.append(hits_at[-1] + hit)
        ap_at.append(ap_at[-1] + (hits_at[-1] / r if hit else 0.0))
        dcg_at.append(dcg_at[-1] + (rel / math.log2(r + 1) if rel else 0.0))
        idcg_at.append(idcg_at[-1] + (ideal[r - 1] / math.log2(r + 1) if r <= len(ideal) else 0.0))
    out = {}
    for k in k_values:
        out[f"ndcg_cut_{k}"] = dcg_at[k] / idcg_at[k] if idcg_at[k] > 0 else 0.0
        out[f"map_cut_{k}"] = ap_at[k] / num_rel if num_rel else 0.0
        out[f"recall_{k}"] = hits_at[k] / num_rel if num_rel else 0.0
        out[f"P_{k}"] = hits_at[k] / k
    return out


def _recip_rank(ranked: List[str], judged: Dict[str, int], relevance_level: int) -> float:
    for r, d in enumerate(ranked, 1):
        if d in judged and judged[d] >= relevance_level:
            return 1.0 / r
    return 0.0


def pytrec_evaluate(qrel: Union[str, Dict[str, Dict[str, int]]], run: Union[str, Dict[str, Dict[str, float]]],
                    k_values=(1, 3, 5, 10, 100), mrr_k_values=(10, 100), relevance_level: int = 1) -> dict:
    """The reference's metric report (eval_utils.py:136-200) without pytrec_eval: trec_eval's measures restated.

    `qrel`: TREC qrels path (`qid 0 docid rel`) or {qid: {docid: rel}}; `run`: TREC run path
    (`qid Q0 docid rank score tag`) or {qid: {docid: score}}.  Ids are strings; a repeated (qid, docid) in a run keeps
    its first position and its last score.  Returns {"ndcg": {"NDCG@k"}, "map": {"MAP@k"}, "recall": {"Recall@k"},
    "precision": {"P@k"}, "mrr": {"MRR@c"}, "perquery": {qid: {ndcg_cut_k, map_cut_k, recall_k, P_k, recip_rank_c}}};
    the summaries are means over the evaluated queries, `round(x, 5)`.

    Semantics (trec_eval as pytrec_eval runs it):
      * a query is evaluated only if it is in both the run and the qrels;
      * ranking: score descending, equal scores by docid descending (byte-wise); the file's rank column is ignored;
      * binary relevance: a judged document with rel >= relevance_level; num_rel = the query's relevant qrels entries;
      * P_k = relevant in the top k / k (k even when fewer were retrieved); recall_k = relevant in the top k / num_rel;
        map_cut_k = sum over relevant documents at ranks r <= k of (relevant so far / r), / num_rel;
      * ndcg_cut_k = sum over r <= k of gain / log2(r + 1), gain = the qrels value (0 unjudged), over the same sum of
        the query's positive qrels values sorted descending, cut at k; 0 when that ideal sum is 0;
      * MRR@c = recip_rank (1 / rank of the first relevant document, else 0) on truncate_run(run, c);
      * a measure whose divisor is 0 is 0; float64, accumulated in rank order, one division at the end.
    """
    if isinstance(qrel, str):
        qrel = _parse_qrel(qrel)
    else:
        qrel = {str(q): {str(d): int(r) for d, r in docs.items()} for q, docs in qrel.items()}
    if isinstance(run, str):
        run = _parse_run(run)
    else:
        run = {str(q): {str(d): float(s) for d, s in docs.items()} for q, docs in run.items()}
    run = {qid: docs for qid, docs in run.items() if qid in qrel}
    n = max(len(run), 1)

    perquery = {qid: _cut_measures(_ranking(docs), qrel[qid], k_values, relevance_level) for qid, docs in run.items()}
    summary = {}
    for group, key, measure in (("ndcg", "NDCG@{}", "ndcg_cut_{}"), ("map", "MAP@{}", "map_cut_{}"),
                                ("recall", "Recall@{}", "recall_{}"), ("precision", "P@{}", "P_{}")):
        summary[group] = {key.format(k): round(sum(m[measure.format(k)] for m in perquery.values()) / n, 5)
                          for k in k_values}
    summary["mrr"] = {}
    for c in mrr_k_values:
        total = 0.0
        for qid, docs in truncate_run(run, c).items():
            rr = _recip_rank(_ranking(docs), qrel[qid], relevance_level)
            perquery[qid][f"recip_rank_{c}"] = rr
            total += rr
        summary["mrr"][f"MRR@{c}"] = round(total / n, 5)
    summary["perquery"] = perquery
    return summary


def mrr_at_k(run_ids: Sequence[Sequence], qrels: Dict, query_ids: Sequence, k: int = 10) -> float:
    """run_ids[i] = ranked document ids of query query_ids[i]; qrels[qid] = {doc id: relevance}."""
    total, n = 0.0, 0
    for qid, ranked in zip(query_ids, run_ids):
        rel = qrels.get(qid)
        if not rel:
            continue
        n += 1
        for r, did in enumerate(list(ranked)[:k]):
            if rel.get(did, 0) >= 1:
                total += 1.0 / (r + 1)
                break
    return round(total / max(n, 1), 5)


def recall_at_k(run_ids: Sequence[Sequence], qrels: Dict, query_ids: Sequence, k: int = 1000) -> float:
    total, n = 0.0, 0
    for qid, ranked in zip(query_ids, run_ids):
        rel = {d for d, s in qrels.get(qid, {}).items() if s >= 1}
        if not rel:
            continue
        n += 1
        total += len(rel.intersection(list(ranked)[:k])) / len(rel)
    return round(total / max(n, 1), 5)
