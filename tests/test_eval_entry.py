"""The evaluation entry points (repconc_amd/evaluate, the recipe helpers, utils/eval_utils' metric engine and loaders) and
`python -m repconc.X` through the compat alias package.

CPU: module entry through the alias, the import surface of the reference's entry scripts and examples, `pytrec_evaluate`
against hand-computed cases and against a deliberately naive restatement on random runs, the BEIR loaders, the run
writer's bytes, and the hard-negative / validation-set helpers.  GPU: the two evaluation scripts end to end in child
processes on a tiny checkpoint, against in-process calls of the same functions."""
import json
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "compat"), ROOT]), HF_HUB_OFFLINE="1",
           TRANSFORMERS_OFFLINE="1")

NEW_MODULES = ["repconc.evaluate.run_repconc_eval", "repconc.evaluate.run_dense_eval",
               "repconc.utils.customize_trained_dense", "repconc.train.run_extract_hardneg",
               "repconc.train.run_gen_valid_set"]


def _run_module(module, args, timeout=600, cwd=None):
    r = subprocess.run([sys.executable, "-m", module] + list(args), env=ENV, cwd=cwd or ROOT, capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, f"{module} exited {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return r


# ------------------------------------------------------------------------------------------- naive metric restatement
def naive_evaluate(qrel, run, k_values=(1, 3, 5, 10, 100), mrr_k_values=(10, 100), relevance_level=1):
    """trec_eval's rules written out query by query: sort, then loop — no shared code with pytrec_evaluate."""
    perquery = {}
    evaluated = [q for q in run if q in qrel]
    for q in evaluated:
        judged = qrel[q]
        # docid descending first, then a stable sort on score descending = (score desc, docid desc)
        order = sorted(run[q], reverse=True)
        order = sorted(order, key=lambda d: -run[q][d])
        num_rel = len([d for d in judged if judged[d] >= relevance_level])
        ideal = sorted([g for g in judged.values() if g > 0], reverse=True)
        m = {}
        for k in k_values:
            hits, ap, dcg, idcg = 0, 0.0, 0.0, 0.0
            for r in range(1, k + 1):
                if r <= len(order):
                    d = order[r - 1]
                    g = judged.get(d, 0)
                    if g >= relevance_level and d in judged:
                        hits += 1
                        ap += hits / r
                    if g:
                        dcg += g / math.log2(r + 1)
                if r <= len(ideal):
                    idcg += ideal[r - 1] / math.log2(r + 1)
            m[f"ndcg_cut_{k}"] = dcg / idcg if idcg > 0 else 0.0
            m[f"map_cut_{k}"] = ap / num_rel if num_rel > 0 else 0.0
            m[f"recall_{k}"] = hits / num_rel if num_rel > 0 else 0.0
            m[f"P_{k}"] = hits / k
        perquery[q] = m
    mrr = {}
    for c in mrr_k_values:
        total = 0.0
        for q in evaluated:
            kept = sorted(run[q], key=lambda d: -run[q][d])[:c]             # stable: file order among equal scores
            kept = sorted(sorted(kept, reverse=True), key=lambda d: -run[q][d])
            rr = 0.0
            for r, d in enumerate(kept, 1):
                if d in qrel[q] and qrel[q][d] >= relevance_level:
                    rr = 1.0 / r
                    break
            perquery[q][f"recip_rank_{c}"] = rr
            total += rr
        mrr[f"MRR@{c}"] = round(total / len(evaluated), 5)
    out = {}
    for group, key, measure in (("ndcg", "NDCG@", "ndcg_cut_"), ("map", "MAP@", "map_cut_"),
                                ("recall", "Recall@", "recall_"), ("precision", "P@", "P_")):
        out[group] = {}
        for k in k_values:
            total = 0.0
            for q in evaluated:
                total += perquery[q][f"{measure}{k}"]
            out[group][f"{key}{k}"] = round(total / len(evaluated), 5)
    out["mrr"] = mrr
    out["perquery"] = perquery
    return out


def _write_run_lines(path, lines):
    with open(path, "w") as f:
        for i, (q, d, s) in enumerate(lines):
            f.write(f"{q}\tQ0\t{d}\t{i + 1}\t{s!r}\tSystem\n")


def _write_qrels(path, qrels):
    with open(path, "w") as f:
        for q, docs in qrels.items():
            for d, r in docs.items():
                f.write(f"{q} 0 {d} {r}\n")


def _assert_same_metrics(got, want, tol=1e-12):
    assert {k: v for k, v in got.items() if k != "perquery"} == {k: v for k, v in want.items() if k != "perquery"}
    assert got["perquery"].keys() == want["perquery"].keys()
    for q, m in want["perquery"].items():
        assert got["perquery"][q].keys() == m.keys(), q
        for name, v in m.items():
            assert abs(got["perquery"][q][name] - v) <= tol, (q, name, got["perquery"][q][name], v)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_python_m_through_the_alias_package():
    """`python -m repconc.X` (how every recipe step starts) runs repconc_amd.X as __main__."""
    for module in ["repconc.train.run_warmup"] + NEW_MODULES:
        r = _run_module(module, ["--help"], timeout=300)
        assert "usage:" in r.stdout, module


def test_entry_script_import_surface_in_a_fresh_interpreter():
    code = r'''
import sys
from repconc.utils.eval_utils import (pytrec_evaluate, load_corpus, load_queries, DataArguments, load_beir_corpus,
    load_beir_qrels, load_beir_queries, TextDataset, get_collator_func, truncate_run, concat_title_body)
from repconc.evaluate.run_repconc_eval import (search_and_compute_metrics, load_or_encode_corpus,
    load_or_encode_queries, replace_pq_centroids, main)
from repconc.evaluate.run_dense_eval import (DataArguments as DenseDataArguments, ModelArguments, EvalArguments,
    load_or_encode_query, load_or_encode_corpus as dense_corpus, search_and_compute_metrics as dense_search_metrics)
import repconc_amd.evaluate.run_repconc_eval as real
assert sys.modules["repconc.evaluate.run_repconc_eval"] is real and real.search_and_compute_metrics is search_and_compute_metrics
d = DataArguments(corpus_path="c", query_path="q", out_corpus_dir="oc", out_query_dir="oq")
assert d.qrel_path is None and d.data_format == "msmarco"
dd = DenseDataArguments(corpus_path="c", out_corpus_dir="oc", query_path="q", out_query_dir="oq")
assert not dd.save_corpus_embed and not dd.save_query_embed
assert ModelArguments(model_name_or_path="m").max_seq_length == 512
e = EvalArguments(output_dir="o", report_to=[])
assert (e.topk, e.search_threads, e.search_batch, e.remove_unused_columns) == (100, 60, 1200, False)
assert "faiss" not in sys.modules
print("ok")
'''
    r = subprocess.run([sys.executable, "-c", code], env=ENV, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]


def test_cpu_search_is_refused_before_any_encoding(tmp_path):
    r = subprocess.run([sys.executable, "-m", "repconc.evaluate.run_repconc_eval", "--model_name_or_path",
                        str(tmp_path / "no_model"), "--corpus_path", "c", "--query_path", "q", "--out_corpus_dir",
                        str(tmp_path / "oc"), "--out_query_dir", str(tmp_path / "oq"), "--output_dir",
                        str(tmp_path / "o"), "--cpu_search"], env=ENV, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "no CPU search path" in r.stderr
    assert not (tmp_path / "oc").exists() and not (tmp_path / "oq").exists()


def test_pytrec_evaluate_worked_case_and_hand_computed_cases(tmp_path):
    from repconc_amd.utils.eval_utils import pytrec_evaluate
    qrel = {"q1": {"a": 2, "b": 1, "c": 0}}
    run = {"q1": {"a": 0.5, "b": 0.9, "d": 0.9, "e": 0.1}}          # ranking d, b, a, e ("d" > "b" in the tie)
    m = pytrec_evaluate(qrel, run, k_values=(1, 3, 10), mrr_k_values=(1, 10))
    assert m["precision"]["P@1"] == 0.0 and m["precision"]["P@3"] == 0.66667 and m["precision"]["P@10"] == 0.2
    assert m["recall"]["Recall@3"] == 1.0 and m["map"]["MAP@3"] == 0.58333 and m["ndcg"]["NDCG@3"] == 0.61991
    assert m["mrr"]["MRR@1"] == 1.0 and m["mrr"]["MRR@10"] == 0.5     # truncation keeps b (file order), P@1 = 0
    pq = m["perquery"]["q1"]
    assert pq["P_3"] == 2 / 3 and pq["map_cut_3"] == (1 / 2 + 2 / 3) / 2 and pq["recip_rank_1"] == 1.0
    assert pq["ndcg_cut_3"] == (1 / math.log2(3) + 2 / math.log2(4)) / (2 + 1 / math.log2(3))
    assert set(pq) == {f"{n}_{k}" for n in ("ndcg_cut", "map_cut", "recall", "P") for k in (1, 3, 10)} | {
        "recip_rank_1", "recip_rank_10"}
    # relevance_level = 2: only "a" is relevant (rank 3); NDCG keeps the graded gains
    m2 = pytrec_evaluate(qrel, run, k_values=(1, 3), mrr_k_values=(10,), relevance_level=2)
    assert m2["precision"]["P@3"] == 0.33333 and m2["recall"]["Recall@3"] == 1.0 and m2["map"]["MAP@3"] == 0.33333
    assert m2["ndcg"]["NDCG@3"] == 0.61991 and m2["mrr"]["MRR@10"] == 0.33333
    # graded NDCG: the ranking is the ideal one reversed
    g = pytrec_evaluate({"q": {"a": 3, "b": 2, "c": 1}}, {"q": {"a": 1.0, "b": 2.0, "c": 3.0}}, k_values=(2, 3),
                        mrr_k_values=(10,))
    assert g["perquery"]["q"]["ndcg_cut_3"] == (1 + 2 / math.log2(3) + 3 / 2) / (3 + 2 / math.log2(3) + 1 / 2)
    assert g["perquery"]["q"]["ndcg_cut_2"] == (1 + 2 / math.log2(3)) / (3 + 2 / math.log2(3))
    # a tie across the MRR cut: which one truncation keeps is file order; the ranking inside is docid-descending
    for first, want in (("x", 1.0), ("y", 0.0)):
        docs = {first: 1.0, ("y" if first == "x" else "x"): 1.0}
        t = pytrec_evaluate({"q": {"x": 1}}, {"q": docs}, k_values=(1,), mrr_k_values=(1, 2))
        assert t["mrr"]["MRR@1"] == want and t["mrr"]["MRR@2"] == 0.5 and t["precision"]["P@1"] == 0.0
    # a query only in the run is not evaluated; a query with no relevant document is, with zeros; fewer than k retrieved
    m3 = pytrec_evaluate({"q1": {"a": 1}, "q2": {"z": 0}, "q4": {"a": 1}},
                         {"q1": {"a": 3.0, "b": 2.0}, "q2": {"a": 1.0}, "q3": {"a": 1.0}}, k_values=(1, 10),
                         mrr_k_values=(10,))
    assert set(m3["perquery"]) == {"q1", "q2"}
    assert m3["perquery"]["q2"] == {"ndcg_cut_1": 0.0, "ndcg_cut_10": 0.0, "map_cut_1": 0.0, "map_cut_10": 0.0,
                                    "recall_1": 0.0, "recall_10": 0.0, "P_1": 0.0, "P_10": 0.0, "recip_rank_10": 0.0}
    assert m3["perquery"]["q1"]["P_10"] == 0.1 and m3["perquery"]["q1"]["recall_10"] == 1.0
    assert m3["precision"]["P@1"] == 0.5 and m3["precision"]["P@10"] == 0.05 and m3["mrr"]["MRR@10"] == 0.5
    # path input == dict input (a repeated line keeps the first position and the last score)
    _write_qrels(tmp_path / "qrels", qrel)
    _write_run_lines(tmp_path / "run", [("q1", "a", 0.5), ("q1", "b", 0.1), ("q1", "d", 0.9), ("q1", "e", 0.1),
                                        ("q1", "b", 0.9)])
    assert pytrec_evaluate(str(tmp_path / "qrels"), str(tmp_path / "run"), k_values=(1, 3, 10),
                           mrr_k_values=(1, 10)) == m


def test_pytrec_evaluate_random_runs_against_the_naive_restatement(tmp_path):
    from repconc_amd.utils.eval_utils import pytrec_evaluate
    rng = random.Random(2022)
    for trial in range(240):
        n_docs = rng.randint(1, 40)
        docs = [f"d{rng.randint(0, 10 ** rng.randint(1, 4))}" for _ in range(n_docs)]
        qids = [f"q{i}" for i in range(rng.randint(1, 8))]
        levels = [0.0, 0.25, 0.5, 1.0] if rng.random() < 0.7 else None   # mostly a few distinct scores: many ties
        lines = []
        for q in qids:
            for _ in range(rng.randint(0 if q != qids[0] else 1, 30)):
                s = rng.choice(levels) if levels else rng.uniform(-3, 3)
                lines.append((q, rng.choice(docs), s))                    # repeats of (qid, docid) happen
        qrel = {}
        for q in qids + ["q_only_in_qrels"]:
            if rng.random() < 0.85:
                qrel[q] = {rng.choice(docs): rng.choice([0, 1, 1, 2, 3]) for _ in range(rng.randint(1, 6))}
        run = {}
        for q, d, s in lines:
            run.setdefault(q, {})[d] = s
        if not any(q in qrel for q in run):
            continue
        k_values = tuple(sorted(rng.sample([1, 2, 3, 5, 10, 20, 50], 3)))
        mrr_k = tuple(sorted(rng.sample([1, 2, 3, 10, 100], 2)))
        level = rng.choice([1, 1, 2])
        want = naive_evaluate(qrel, run, k_values, mrr_k, level)
        got = pytrec_evaluate(qrel, run, k_values, mrr_k, level)
        _assert_same_metrics(got, want)
        if trial % 8 == 0:                                                    # and through the file parsers
            _write_qrels(tmp_path / "qrels", qrel)
            _write_run_lines(tmp_path / "run", lines)
            _assert_same_metrics(pytrec_evaluate(str(tmp_path / "qrels"), str(tmp_path / "run"), k_values, mrr_k,
                                                 level), want)


def test_beir_loaders(tmp_path):
    from repconc_amd.utils.eval_utils import concat_title_body, load_beir_corpus, load_beir_qrels, load_beir_queries
    docs = [{"_id": "doc-a", "title": "Why?", "text": " body a "},
            {"_id": "doc-b", "title": "  Plain title ", "text": "body b"},
            {"_id": "doc-c", "title": "   ", "text": "body c\n"},
            {"_id": "doc-d", "text": "no title"},
            {"_id": "doc-e", "title": "终わり。", "text": "x"},
            {"_id": "doc-f", "title": "Long", "text": "y" * 12000}]
    (tmp_path / "corpus.jsonl").write_text("".join(json.dumps(d) + "\n" for d in docs), encoding="utf-8")
    corpus = load_beir_corpus(str(tmp_path / "corpus.jsonl"), "[SEP]")
    assert corpus["doc-a"] == "Why? body a" and corpus["doc-b"] == "Plain title. body b"
    assert corpus["doc-c"] == "body c" and corpus["doc-d"] == "no title" and corpus["doc-e"] == "终わり。 x"
    assert corpus["doc-f"] == ("Long. " + "y" * 12000)[:10000] and len(corpus["doc-f"]) == 10000
    assert concat_title_body({"text": "t", "title": "Wow!"}) == "Wow! t"
    (tmp_path / "queries.jsonl").write_text(json.dumps({"_id": "q-1", "text": "  what?  "}) + "\n"
                                            + json.dumps({"_id": "q-2", "text": "b", "metadata": {}}) + "\n")
    assert load_beir_queries(str(tmp_path / "queries.jsonl")) == {"q-1": "what?", "q-2": "b"}
    (tmp_path / "test.tsv").write_text("query-id\tcorpus-id\tscore\nq-1\tdoc-a\t2\nq-1\tdoc-b\t0\nq-2\tdoc-c\t1\n")
    assert load_beir_qrels(str(tmp_path / "test.tsv")) == {"q-1": {"doc-a": 2, "doc-b": 0}, "q-2": {"doc-c": 1}}


def test_run_writer_bytes_equal_the_reference_loop(tmp_path):
    from repconc_amd.utils.eval_utils import write_run
    scores = np.array([[0.1, -2.5, 3e-7], [1.0, np.finfo(np.float32).max, 0.1]], dtype=np.float32)
    for qids, ids in ((np.array(["q7", "1048585"]), np.array([["d1", "d22", "x"], ["a", "b", "c"]])),
                      (np.array([7, 1048585]), np.array([[1, 22, 333], [4, 5, 6]], dtype=np.int64))):
        want = "".join(f"{qid.item()}\tQ0\t{docid.item()}\t{i + 1}\t{score.item()}\tSystem\n"
                       for qid, s_row, d_row in zip(qids, scores, ids) for i, (score, docid) in enumerate(zip(s_row, d_row)))
        write_run(str(tmp_path / "run.tsv"), qids, scores, ids)
        got = (tmp_path / "run.tsv").read_bytes()
        assert got == want.encode()
    lines = got.decode().splitlines()
    assert lines[0] == "7\tQ0\t1\t1\t0.10000000149011612\tSystem"
    assert lines[1].split("\t")[4] == "-2.5" and lines[4].split("\t")[4] == "3.4028234663852886e+38"
    assert lines[2].split("\t")[4] == repr(float(np.float32(3e-7))) and lines[3].split("\t")[4] == "1.0"


def test_extract_hardneg_and_gen_valid_set(tmp_path):
    (tmp_path / "qrels").write_text("1 0 10 1\n1 0 11 0\n2 0 20 2\n9 0 90 1\n")
    run = ["1 Q0 12 1 9.0 S", "1 Q0 10 2 8.0 S", "1 Q0 11 3 7.0 S", "1 Q0 13 4 6.0 S",
           "2 Q0 21 1 5.0 S", "2 Q0 20 2 4.0 S", "2 Q0 22 3 3.0 S", "3 Q0 30 1 1.0 S", "3 Q0 31 2 0.5 S"]
    (tmp_path / "run.tsv").write_text("\n".join(r.replace(" ", "\t") for r in run) + "\n")
    out = tmp_path / "new" / "dir" / "hardneg.json"
    _run_module("repconc.train.run_extract_hardneg", ["--run_path", str(tmp_path / "run.tsv"), "--qrel_path",
                                                      str(tmp_path / "qrels"), "--topk", "3", "--output_path", str(out)])
    assert json.loads(out.read_text()) == {"1": ["12", "11"], "2": ["21", "22"], "3": ["30", "31"]}
    assert list(json.loads(out.read_text())) == ["1", "2", "3"]

    corpus = "".join(f"{pid}\ttext of {pid}\textra\n" for pid in ("30", "22", "10", "21", "90", "13", "12", "11", "20"))
    (tmp_path / "corpus.tsv").write_text(corpus)
    (tmp_path / "queries.tsv").write_text("1\tq one\n2\tq two\n3\tq three\n")
    o = tmp_path / "valid"
    r = _run_module("repconc.train.run_gen_valid_set", [
        "--input_corpus_path", str(tmp_path / "corpus.tsv"), "--input_query_path", str(tmp_path / "queries.tsv"),
        "--input_qrel_path", str(tmp_path / "qrels"), "--input_run_path", str(tmp_path / "run.tsv"), "--topk", "2",
        "--output_corpus_path", str(o / "corpus.tsv"), "--output_query_path", str(o / "q" / "queries.tsv"),
        "--output_qrel_path", str(o / "qrels")])
    # qrels docids 10 11 20 90 + run rank <= 2 for qrels queries 1, 2: 12 10 21 20 (query 3 is not in the qrels)
    assert (o / "corpus.tsv").read_text() == "".join(f"{pid}\ttext of {pid}\textra\n"
                                                     for pid in ("10", "21", "90", "12", "11", "20"))
    assert (o / "qrels").read_bytes() == (tmp_path / "qrels").read_bytes()
    assert (o / "q" / "queries.tsv").read_bytes() == (tmp_path / "queries.tsv").read_bytes()
    assert "Write Cnt: 6, Sample Cnt: 6" in r.stdout


def test_checkpoints_reload_on_cpu(tmp_path):
    """What the entry modules load: a RepCONC checkpoint (RepCONC.save_pretrained) and a dense one (save_pretrained of
    BertDense), each with the generated-vocabulary tokenizer, read back with the same weights."""
    import torch
    from transformers import AutoTokenizer
    from repconc_amd.models.dense import AutoDense, BertDense
    from repconc_amd.models.repconc import RepCONC
    ckpt = str(tmp_path / "ckpt")
    _repconc_checkpoint(ckpt)
    model = RepCONC.from_pretrained(ckpt, False, None, None)
    saved = torch.load(os.path.join(ckpt, "pytorch_model.bin"), map_location="cpu")
    assert model.config.MCQ_M == 48 and all(torch.equal(v, saved[k]) for k, v in model.state_dict().items())
    tok = AutoTokenizer.from_pretrained(ckpt)
    assert tok(["w1 w299 zz"])["input_ids"] == [[2, 6, 304, 1, 3]] and tok.sep_token == "[SEP]"
    dense = BertDense(_bert_config())
    dense.save_pretrained(str(tmp_path / "dense"))
    back = AutoDense.from_pretrained(str(tmp_path / "dense"))
    assert type(back) is BertDense and back.config.pooling == "mean"
    assert all(torch.equal(v, back.state_dict()[k]) for k, v in dense.state_dict().items())


# ---------------------------------------------------------------------------------------------------------------- GPU
VOCAB =["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(300)]


def _bert_config():
    from transformers import BertConfig
    cfg = BertConfig(hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=128,
                     vocab_size=len(VOCAB), max_position_embeddings=40, hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0)
    cfg.similarity_metric, cfg.pooling = "METRIC_IP", "mean"
    return cfg


def _save_tokenizer(ckpt_dir):
    """A BertTokenizerFast built from a vocabulary file written next to the checkpoint (nothing from the hub)."""
    from transformers import BertTokenizerFast
    os.makedirs(ckpt_dir, exist_ok=True)
    with open(os.path.join(ckpt_dir, "vocab.txt"), "w") as f:
        f.write("\n".join(VOCAB) + "\n")
    BertTokenizerFast.from_pretrained(ckpt_dir).save_pretrained(ckpt_dir)


def _repconc_checkpoint(ckpt_dir):
    import torch
    from repconc_amd.models.dense import BertDense
    from repconc_amd.models.repconc import RepCONC
    torch.manual_seed(1)
    cfg = _bert_config()
    cfg.MCQ_M, cfg.MCQ_K = 48, 256
    model = RepCONC(cfg, BertDense(cfg), False, None, None)
    with torch.no_grad():
        model.centroids.mul_(0.05)
        model.rotation.copy_(torch.linalg.qr(torch.randn(768, 768))[0])
    model.save_pretrained(ckpt_dir)
    _save_tokenizer(ckpt_dir)


def _texts(seed, n_docs=300, n_queries=20):
    rng = np.random.default_rng(seed)
    words = [f"w{i}" for i in range(300)]
    docs = [" ".join(rng.choice(words, rng.integers(3, 25))) for _ in range(n_docs)]
    queries = [" ".join(rng.choice(words, rng.integers(2, 8))) for _ in range(n_queries)]
    qrels = [(qi, int(di), int(rel)) for qi in range(n_queries)
             for di, rel in zip(rng.choice(n_docs, 3, replace=False), rng.choice([0, 1, 2, 3], 3))]
    return docs, queries, qrels


def _msmarco_dataset(root):
    docs, queries, qrels = _texts(7)
    os.makedirs(root, exist_ok=True)
    with open(os.path.join(root, "corpus.tsv"), "w") as f:
        f.write("".join(f"{1000 + i}\t{t}\n" for i, t in enumerate(docs)))
    with open(os.path.join(root, "queries.tsv"), "w") as f:
        f.write("".join(f"{50 + i}\t{t}\n" for i, t in enumerate(queries)))
    with open(os.path.join(root, "qrels.tsv"), "w") as f:
        f.write("".join(f"{50 + q} 0 {1000 + d} {rel}\n" for q, d, rel in qrels))
    return {k: os.path.join(root, v) for k, v in (("corpus", "corpus.tsv"), ("queries", "queries.tsv"),
                                                   ("qrels", "qrels.tsv"))}


def _reference_run_text(query_ids, scores, ids):
    """The reference's per-element loop (run_repconc_eval.py:102-105)."""
    return "".join(f"{qid.item()}\tQ0\t{docid.item()}\t{i + 1}\t{score.item()}\tSystem\n"
                   for qid, s_row, d_row in zip(query_ids, scores, ids) for i, (score, docid) in enumerate(zip(s_row, d_row)))


def _check_metrics(metric_path, qrels_for_eval, run_path):
    from repconc_amd.utils.eval_utils import _parse_run, pytrec_evaluate
    with open(metric_path) as f:
        got = json.load(f)
    assert got == pytrec_evaluate(qrels_for_eval, run_path)
    qrel = qrels_for_eval
    if isinstance(qrel, str):
        qrel = {}
        for line in open(qrels_for_eval):
            q, _, d, r = line.split()
            qrel.setdefault(q, {})[d] = int(r)
    _assert_same_metrics(got, naive_evaluate(qrel, _parse_run(run_path)))
    return got


def _repconc_eval_in_process(ckpt, corpus, queries, topk, batch):
    """The same encoders and search, called in this process."""
    import torch
    from transformers import AutoTokenizer
    from repconc_amd.models.repconc import RepCONC
    from repconc_amd.models.repconc.evaluate_repconc import (EvalArguments, batch_search, encode_corpus, encode_query,
                                                             load_index_to_gpu)
    tok = AutoTokenizer.from_pretrained(ckpt)
    model = RepCONC.from_pretrained(ckpt, False, None, None).to(torch.device("cuda", 0))
    eargs = EvalArguments(output_dir=os.path.join(ckpt, "unused"), per_device_eval_batch_size=batch, report_to=[])
    index, corpus_ids = encode_corpus(corpus, model, tok, 32, eargs)
    qemb, qids = encode_query(queries, model, tok, 32, eargs)
    index.set_centroids(model.centroids.data)
    scores, ids = batch_search(qids, qemb, corpus_ids, load_index_to_gpu(index), topk, batch_size=7)
    return qemb, qids, corpus_ids, index, scores, ids


def _repconc_cli(ckpt, corpus_path, query_path, qrel_path, out, fmt, timeout=600):
    return _run_module("repconc.evaluate.run_repconc_eval", [
        "--model_name_or_path", ckpt, "--max_seq_length", "32", "--corpus_path", corpus_path, "--query_path", query_path,
        "--qrel_path", qrel_path, "--out_corpus_dir", os.path.join(out, "corpus"), "--out_query_dir",
        os.path.join(out, "query"), "--data_format", fmt, "--topk", "50", "--search_batch", "7",
        "--per_device_eval_batch_size", "16", "--output_dir", os.path.join(out, "trainer"), "--report_to", "none",
        "--threads", "4"], timeout=timeout)


def _check_repconc_eval(tmp_path, ckpt, data, fmt, load_corpus_fn, load_queries_fn, qrels_for_eval, n_queries):
    import torch
    out = str(tmp_path / "out")
    _repconc_cli(ckpt, data["corpus"], data["queries"], data["qrels"], out, fmt)
    run_path = os.path.join(out, "query", "run.tsv")
    run_text = open(run_path).read()
    assert len(run_text.splitlines()) == n_queries * 50
    corpus, queries = load_corpus_fn(data["corpus"]), load_queries_fn(data["queries"])
    qemb, qids, corpus_ids, index, scores, ids = _repconc_eval_in_process(ckpt, corpus, queries, 50, 16)
    assert np.array_equal(np.load(os.path.join(out, "query", "qids.npy")), qids)
    assert np.array_equal(np.load(os.path.join(out, "query", "codes.npy")), qemb)
    assert np.array_equal(np.load(os.path.join(out, "corpus", "corpus_ids.npy")), corpus_ids)
    from repconc_amd.faiss_io import read_index
    cached = read_index(os.path.join(out, "corpus", "index"))
    assert torch.equal(cached.codes, index.codes)
    assert run_text == _reference_run_text(qids, scores, ids)
    got = _check_metrics(os.path.join(out, "query", "metric.json"), qrels_for_eval, run_path)
    assert len(got["perquery"]) == n_queries                    # every query is judged and retrieved
    # second invocation: the corpus and query files are gone, the caches answer; run.tsv is rewritten byte for byte
    for k in ("corpus", "queries"):
        os.rename(data[k], data[k] + ".moved")
    os.remove(run_path)
    r = _repconc_cli(ckpt, data["corpus"], data["queries"], data["qrels"], out, fmt)
    assert "Load pre-computed corpus representations" in r.stderr and "Load pre-computed query representations" in r.stderr
    assert "Skip search process because metric.json file already exists" in r.stderr
    assert open(run_path).read() == run_text


@pytest.mark.gpu
def test_run_repconc_eval_module_msmarco(tmp_path):
    from repconc_amd.utils.eval_utils import load_corpus, load_queries
    ckpt = str(tmp_path / "ckpt")
    _repconc_checkpoint(ckpt)
    data = _msmarco_dataset(str(tmp_path / "data"))
    from transformers import AutoTokenizer
    sep = AutoTokenizer.from_pretrained(ckpt).sep_token
    _check_repconc_eval(tmp_path, ckpt, data, "msmarco", lambda p: load_corpus(p, sep), load_queries, data["qrels"], 20)


@pytest.mark.gpu
def test_run_repconc_eval_module_beir(tmp_path):
    from repconc_amd.utils.eval_utils import load_beir_corpus, load_beir_qrels, load_beir_queries
    ckpt = str(tmp_path / "ckpt")
    _repconc_checkpoint(ckpt)
    docs, queries, qrels = _texts(11, n_queries=12)
    root = tmp_path / "beir"
    (root / "qrels").mkdir(parents=True)
    titles = ["Title {}{}".format(i, ["", ".", "?", "!"][i % 4]) for i in range(len(docs))]
    with open(root / "corpus.jsonl", "w") as f:
        for i, t in enumerate(docs):
            f.write(json.dumps({"_id": f"doc-{i:04x}", "title": titles[i] if i % 5 else "", "text": t}) + "\n")
    with open(root / "queries.jsonl", "w") as f:
        for i, t in enumerate(queries):
            f.write(json.dumps({"_id": f"query_{chr(97 + i)}", "text": " " + t + " "}) + "\n")
    with open(root / "qrels" / "test.tsv", "w") as f:
        f.write("query-id\tcorpus-id\tscore\n")
        f.write("".join(f"query_{chr(97 + q)}\tdoc-{d:04x}\t{rel}\n" for q, d, rel in qrels))
    data = {"corpus": str(root / "corpus.jsonl"), "queries": str(root / "queries.jsonl"),
            "qrels": str(root / "qrels" / "test.tsv")}
    _check_repconc_eval(tmp_path, ckpt, data, "beir", lambda p: load_beir_corpus(p, "[SEP]"), load_beir_queries,
                        load_beir_qrels(data["qrels"]), 12)


@pytest.mark.gpu
def test_customize_then_run_dense_eval_modules(tmp_path):
    import torch
    from transformers import AutoTokenizer
    from repconc_amd.models.dense import AutoDense, BertDense
    from repconc_amd.models.dense.evaluate_dense import (batch_dense_search, create_index, encode_dense_corpus,
                                                         encode_dense_query)
    from repconc_amd.utils.eval_utils import load_corpus, load_queries
    torch.manual_seed(3)
    trained = str(tmp_path / "trained")
    BertDense(_bert_config()).save_pretrained(trained)
    _save_tokenizer(trained)
    custom = str(tmp_path / "custom")
    _run_module("repconc.utils.customize_trained_dense", ["--model_name_or_path", trained, "--similarity_metric",
                                                          "METRIC_COS", "--pooling", "mean", "--output_dir", custom])
    with open(os.path.join(custom, "config.json")) as f:
        cfg = json.load(f)
    assert cfg["similarity_metric"] == "METRIC_COS" and cfg["pooling"] == "mean"
    data = _msmarco_dataset(str(tmp_path / "data"))
    out = tmp_path / "out"
    args = ["--model_name_or_path", custom, "--max_seq_length", "32", "--corpus_path", data["corpus"], "--query_path",
            data["queries"], "--qrel_path", data["qrels"], "--out_corpus_dir", str(out / "corpus"), "--out_query_dir",
            str(out / "query"), "--save_corpus_embed", "--save_query_embed", "--topk", "50", "--search_batch", "7",
            "--per_device_eval_batch_size", "16", "--output_dir", str(out / "trainer"), "--report_to", "none"]
    _run_module("repconc.evaluate.run_dense_eval", args)
    run_path = str(out / "query" / "run.tsv")
    run_text = open(run_path).read()
    assert len(run_text.splitlines()) == 20 * 50
    corpus_embeds, corpus_ids = np.load(out / "corpus" / "corpus_embeds.npy"), np.load(out / "corpus" / "corpus_ids.npy")
    query_embeds, query_ids = np.load(out / "query" / "query_embeds.npy"), np.load(out / "query" / "qids.npy")
    # the saved embeddings are the customized model's outputs (cosine: unit rows)
    tok = AutoTokenizer.from_pretrained(custom)
    model = AutoDense.from_pretrained(custom).to(torch.device("cuda", 0))
    assert model.config.similarity_metric == "METRIC_COS" and model.config.pooling == "mean"
    eargs = SimpleArgs()
    want_c, want_cids = encode_dense_corpus(load_corpus(data["corpus"], tok.sep_token), model, tok, 32, eargs)
    want_q, want_qids = encode_dense_query(load_queries(data["queries"]), model, tok, 32, eargs)
    assert np.array_equal(corpus_ids, want_cids) and np.array_equal(query_ids, want_qids)
    np.testing.assert_allclose(corpus_embeds, want_c, rtol=0, atol=1e-6)
    np.testing.assert_allclose(query_embeds, want_q, rtol=0, atol=1e-6)
    np.testing.assert_allclose(np.linalg.norm(corpus_embeds, axis=1), 1.0, rtol=0, atol=1e-5)
    # run.tsv: the in-process exact search of the saved embeddings, in the reference's bytes
    scores, ids = batch_dense_search(query_ids, query_embeds, corpus_ids, create_index(corpus_embeds), 50, batch_size=7)
    assert run_text == _reference_run_text(query_ids, scores, ids)
    _check_metrics(str(out / "query" / "metric.json"), data["qrels"], run_path)
    # second invocation: metric.json exists, the search is skipped and run.tsv is left alone
    os.remove(run_path)
    r = _run_module("repconc.evaluate.run_dense_eval", args)
    assert "Skip search process because metric.json file already exists" in r.stderr
    assert "Load pre-computed corpus representations" in r.stderr and not os.path.exists(run_path)


class SimpleArgs:
    per_device_eval_batch_size, fp16, bf16 = 16, False, False
