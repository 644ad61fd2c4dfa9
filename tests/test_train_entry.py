"""The training entry points (repconc_amd/train/run_train_conc, run_train_jpq), the in-training validation and checkpoint
layout of both trainers, and the stage-2 trainer's dataset / collator / arguments / callback.

CPU: import surface (directly and through the compat alias), the recipes' step 7 and step 9 flags parsed on the installed
transformers, the output-directory rule, `QueryDataset`, `FinetuneQueryCollator`, the CPU refusal.  GPU: `evaluate` of
both trainers against the hand-made composition of the same calls (exact), whole runs of both entry points with validation,
best-model reload and resume, the index kept in step with the centroids after every step, and one run through
`python -m repconc.train.run_train_jpq` in a child process.  Every model is a one-layer encoder written by the test itself;
nothing is read from outside the test's temporary directories."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

ENV = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "compat"), ROOT]), HF_HUB_OFFLINE="1",
           TRANSFORMERS_OFFLINE="1")
gpu = pytest.mark.gpu

VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + [f"w{i}" for i in range(300)]


# ------------------------------------------------------------------------------------------------------------ helpers
def _bert_config(metric="METRIC_IP"):
    from transformers import BertConfig
    cfg = BertConfig(hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=128,
                     vocab_size=len(VOCAB), max_position_embeddings=40, hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0)
    cfg.similarity_metric, cfg.pooling = metric, "mean"
    return cfg


def _save_tokenizer(ckpt_dir):
    """A BertTokenizerFast built from a vocabulary file written next to the checkpoint (nothing from the hub)."""
    from transformers import BertTokenizerFast
    os.makedirs(ckpt_dir, exist_ok=True)
    with open(os.path.join(ckpt_dir, "vocab.txt"), "w") as f:
        f.write("\n".join(VOCAB) + "\n")
    BertTokenizerFast.from_pretrained(ckpt_dir).save_pretrained(ckpt_dir)


def _repconc_model(M=48, metric="METRIC_IP", use_constraint=False):
    import torch
    from repconc_amd.models.dense import BertDense
    from repconc_amd.models.repconc import RepCONC
    torch.manual_seed(1)
    cfg = _bert_config(metric)
    cfg.MCQ_M, cfg.MCQ_K = M, 256
    model = RepCONC(cfg, BertDense(cfg), use_constraint, 0.003 if use_constraint else None, 20 if use_constraint else None)
    with torch.no_grad():
        if metric != "METRIC_CENTROID_COS":
            model.centroids.mul_(0.05)
        model.rotation.copy_(torch.linalg.qr(torch.randn(768, 768))[0])
    return model


def _repconc_checkpoint(ckpt_dir, M=48):
    _repconc_model(M).save_pretrained(ckpt_dir)
    _save_tokenizer(ckpt_dir)
    return ckpt_dir


def _write_dataset(root, n_docs=300, n_train=24, n_valid=12):
    """corpus (300 lines), training queries / qrels (one query has two positives) / hard negatives, validation queries /
    qrels over the same corpus; texts of at most 30 generated words.  A query repeats words of its first positive, so that
    even a randomly initialised encoder ranks some positives high and others not: the validation measures are neither 0 nor 1."""
    rng = np.random.default_rng(7)
    words = [f"w{i}" for i in range(300)]
    docs = [list(rng.choice(words, rng.integers(6, 30))) for _ in range(n_docs)]
    os.makedirs(root, exist_ok=True)
    p = {k: os.path.join(root, k) for k in ("corpus.tsv", "query.train", "qrels.train", "hardneg.json", "query.dev",
                                           "qrels.dev")}

    def query_of(doc, noise):
        kept = list(rng.choice(docs[doc], rng.integers(3, 7)))
        return " ".join(kept + list(rng.choice(words, noise)))
    with open(p["corpus.tsv"], "w") as f:
        f.write("".join(f"{1000 + i}\t{' '.join(t)}\n" for i, t in enumerate(docs)))
    pos = rng.choice(n_docs, n_train, replace=False)
    with open(p["query.train"], "w") as f:
        f.write("".join(f"{50 + i}\t{query_of(int(pos[i]), 2)}\n" for i in range(n_train)))
    with open(p["qrels.train"], "w") as f:
        f.write("".join(f"{50 + q} 0 {1000 + int(d)} 1\n" for q, d in enumerate(pos)))
        f.write(f"53 0 {1000 + int(pos[9])} 2\n53 0 {1000 + int(pos[10])} 0\n")       # a second positive, a non-positive
    hard = {str(50 + q): [str(1000 + int(d)) for d in rng.choice(np.delete(np.arange(n_docs), pos[q]), 5, replace=False)]
            for q in range(n_train)}
    with open(p["hardneg.json"], "w") as f:
        json.dump(hard, f)
    judged = [rng.choice(n_docs, 3, replace=False) for _ in range(n_valid)]
    with open(p["query.dev"], "w") as f:
        f.write("".join(f"{900 + i}\t{query_of(int(judged[i][0]), i % 4)}\n" for i in range(n_valid)))
    with open(p["qrels.dev"], "w") as f:
        f.write("".join(f"{900 + q} 0 {1000 + int(d)} {rel}\n" for q in range(n_valid)
                        for d, rel in zip(judged[q], (1, 2, 0))))
    return p


# the flags of recipe step 7 (examples/*/repconc/7_run_conc_train.sh) and step 9 (9_run_jpq_train.sh), values as paths / numbers
def _step7_flags(d, model, out):
    return ["--qrel_path", d["qrels.train"], "--query_path", d["query.train"], "--corpus_path", d["corpus.tsv"],
            "--valid_qrel_path", d["qrels.dev"], "--valid_query_path", d["query.dev"], "--valid_corpus_path", d["corpus.tsv"],
            "--output_dir", out, "--model_name_or_path", model, "--logging_steps", "5", "--max_query_len", "16",
            "--max_doc_len", "128", "--per_device_train_batch_size", "4096", "--per_device_eval_batch_size", "32",
            "--temperature", "1", "--gradient_accumulation_steps", "1", "--fp16", "--negative_per_query", "11",
            "--dynamic_topk_hard_negative", "11", "--learning_rate", "2e-5", "--centroid_learning_rate", "5e-4",
            "--num_train_epochs", "4", "--dataloader_drop_last", "--overwrite_output_dir", "--dataloader_num_workers", "0",
            "--weight_decay", "0", "--lr_scheduler_type", "constant", "--cache_chunk_size", "64", "--mse_loss_weight", "1e-4",
            "--negative", d["hardneg.json"], "--sk_epsilon", "0.003", "--sk_iters", "100", "--metric_for_best_model",
            "MRR@10", "--save_total_limit", "2", "--evaluation_strategy", "steps", "--save_strategy", "steps",
            "--eval_steps", "40", "--save_steps", "40", "--load_best_model_at_end", "--optim", "adamw_torch"]


def _step9_flags(d, model, index_dir, out):
    return ["--qrel_path", d["qrels.train"], "--query_path", d["query.train"], "--valid_qrel_path", d["qrels.dev"],
            "--valid_query_path", d["query.dev"], "--output_dir", out, "--model_name_or_path", model, "--index_input_dir",
            index_dir, "--logging_steps", "100", "--max_query_len", "16", "--per_device_train_batch_size", "128",
            "--temperature", "1", "--gradient_accumulation_steps", "1", "--learning_rate", "2e-6",
            "--centroid_learning_rate", "2e-5", "--num_train_epochs", "4", "--dataloader_drop_last", "--overwrite_output_dir",
            "--dataloader_num_workers", "0", "--weight_decay", "0", "--lr_scheduler_type", "constant",
            "--metric_for_best_model", "MRR@10", "--save_total_limit", "2", "--evaluation_strategy", "steps",
            "--save_strategy", "steps", "--save_steps", "1000", "--eval_steps", "1000", "--load_best_model_at_end", "--optim",
            "adamw_torch"]


_FAKE = {k: k for k in ("corpus.tsv", "query.train", "qrels.train", "hardneg.json", "query.dev", "qrels.dev")}


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_import_surface_and_help_directly_and_through_the_alias():
    code = r'''
import sys
from repconc.train.run_train_conc import ModelArguments as ConcModelArguments, load_validation_set, main
from repconc.train.run_train_jpq import ModelArguments as JPQModelArguments, main as jpq_main
from repconc.models.jpq.finetune_jpq import (JPQ, QueryDataset, JPQFinetuneArguments, FinetuneQueryCollator, JPQFinetuner,
    DataTrainingArguments, JPQ_SyncIndex_Callback, jpq_step_end)
from repconc.models.repconc.finetune_repconc import (RepCONCFinetuner, RepCONCFinetuneArguments, QDRelDataset,
    FinetuneCollator, DataTrainingArguments as ConcData, RepCONC_Norm_Centroid_Callback)
import repconc_amd.train.run_train_conc as conc, repconc_amd.train.run_train_jpq as jpq
import repconc_amd.models.jpq.finetune_jpq as fj
assert sys.modules["repconc.train.run_train_conc"] is conc and sys.modules["repconc.train.run_train_jpq"] is jpq
assert fj.JPQFinetuner is JPQFinetuner and conc.main is main and jpq.main is jpq_main
assert callable(RepCONCFinetuner.evaluate) and "evaluate" in RepCONCFinetuner.__dict__ and "evaluate" in JPQFinetuner.__dict__
assert [f for f in DataTrainingArguments.__dataclass_fields__] == ["qrel_path", "query_path", "valid_qrel_path",
                                                                   "valid_query_path", "max_query_len"]
a = JPQFinetuneArguments(output_dir="o")
assert (a.dynamic_topk_negative, a.centroid_learning_rate, a.temperature, a.seed, a.remove_unused_columns, a.head,
        a.deterministic_decode, a.overwrite_output_dir) == (200, 1e-3, 1.0, 2023, False, "decode", False, False)
assert a.report_to in ([], "none", None) and RepCONCFinetuneArguments(output_dir="o").report_to in ([], "none", None)
assert "faiss" not in sys.modules
print("ok")
'''
    r = subprocess.run([sys.executable, "-c", code], env=ENV, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]
    for module in ("repconc.train.run_train_conc", "repconc.train.run_train_jpq"):
        r = subprocess.run([sys.executable, "-m", module, "--help"], env=ENV, cwd=ROOT, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0 and "usage:" in r.stdout and "--evaluation_strategy" in r.stdout, (module, r.stderr[-2000:])


def test_recipe_flags_parse_on_the_installed_transformers(tmp_path):
    from transformers import HfArgumentParser
    from repconc_amd.models.jpq.finetune_jpq import DataTrainingArguments as JPQData, JPQFinetuneArguments
    from repconc_amd.models.repconc.finetune_repconc import DataTrainingArguments, RepCONCFinetuneArguments
    from repconc_amd.train import run_train_conc, run_train_jpq
    d = {k: str(tmp_path / v) for k, v in _FAKE.items()}
    parser = HfArgumentParser((run_train_conc.ModelArguments, DataTrainingArguments, RepCONCFinetuneArguments))
    m, data, t = parser.parse_args_into_dataclasses(_step7_flags(d, str(tmp_path / "warmup"), str(tmp_path / "out7")))
    assert (m.model_name_or_path, m.sk_epsilon, m.sk_iters) == (str(tmp_path / "warmup"), 0.003, 100)
    assert (data.max_query_len, data.max_doc_len, data.valid_corpus_path) == (16, 128, d["corpus.tsv"])
    assert t.eval_strategy == "steps" and t.overwrite_output_dir is True and t.metric_for_best_model == "MRR@10"
    assert t.load_best_model_at_end and t.greater_is_better and (t.eval_steps, t.save_steps, t.save_total_limit) == (40, 40, 2)
    assert (t.negative, t.negative_per_query, t.dynamic_topk_hard_negative, t.cache_chunk_size) == (d["hardneg.json"], 11, 11, 64)
    assert t.fp16 and t.dataloader_drop_last and t.report_to in ([], "none", None) and t.dataloader_num_workers == 0
    parser = HfArgumentParser((run_train_jpq.ModelArguments, JPQData, JPQFinetuneArguments))
    m, data, t = parser.parse_args_into_dataclasses(_step9_flags(d, str(tmp_path / "enc"), str(tmp_path / "idx"),
                                                                 str(tmp_path / "out9")))
    assert (m.model_name_or_path, m.index_input_dir, data.max_query_len) == (str(tmp_path / "enc"), str(tmp_path / "idx"), 16)
    assert t.eval_strategy == "steps" and t.overwrite_output_dir is True and t.metric_for_best_model == "MRR@10"
    assert (t.centroid_learning_rate, t.learning_rate, t.eval_steps, t.head, t.deterministic_decode) == (2e-5, 2e-6, 1000, "decode", False)
    assert t.report_to in ([], "none", None)
    # both names of the strategy: equal is accepted, different is an error; the new name alone still works
    for cls in (RepCONCFinetuneArguments, JPQFinetuneArguments):
        one = HfArgumentParser((cls,))
        base = ["--output_dir", str(tmp_path / "o"), "--eval_steps", "2"]
        with pytest.raises(ValueError, match="disagree"):
            one.parse_args_into_dataclasses(base + ["--evaluation_strategy", "steps", "--eval_strategy", "epoch"])
        assert one.parse_args_into_dataclasses(base + ["--evaluation_strategy", "steps", "--eval_strategy", "steps"])[0].eval_strategy == "steps"
        assert one.parse_args_into_dataclasses(base + ["--eval_strategy", "steps"])[0].eval_strategy == "steps"
        plain = one.parse_args_into_dataclasses(base)[0]
        assert plain.eval_strategy == "no" and plain.overwrite_output_dir is False
    fused = HfArgumentParser((JPQFinetuneArguments,)).parse_args_into_dataclasses(
        ["--output_dir", str(tmp_path / "o"), "--head", "fused", "--deterministic_decode"])[0]
    assert fused.head == "fused" and fused.deterministic_decode is True
    # a single *.json argument is read as a json file
    from repconc_amd.train.entry_common import parse_arguments
    (tmp_path / "args.json").write_text(json.dumps({"output_dir": str(tmp_path / "o"), "evaluation_strategy": "steps",
                                                    "eval_steps": 3, "head": "fused"}))
    (t,) = parse_arguments(HfArgumentParser((JPQFinetuneArguments,)), [str(tmp_path / "args.json")])
    assert t.eval_strategy == "steps" and t.eval_steps == 3 and t.head == "fused"


def test_output_directory_rule(tmp_path):
    from repconc_amd.models.jpq.finetune_jpq import JPQFinetuneArguments
    from repconc_amd.train import run_train_conc
    from repconc_amd.train.entry_common import resume_from_output_dir
    used, fresh, logs = tmp_path / "used", tmp_path / "fresh", tmp_path / "logs"
    (used / "checkpoint-3").mkdir(parents=True)
    logs.mkdir()
    (logs / "05-01-12:00.log").write_text("the recipes tee their log into the output directory\n")
    with pytest.raises(ValueError, match="overwrite_output_dir"):
        resume_from_output_dir(JPQFinetuneArguments(output_dir=str(used)))
    assert resume_from_output_dir(JPQFinetuneArguments(output_dir=str(used), overwrite_output_dir=True)) is True
    for out in (fresh, logs):
        for flag in (False, True):
            assert resume_from_output_dir(JPQFinetuneArguments(output_dir=str(out), overwrite_output_dir=flag)) is False
    # through the entry point: the rule is applied before any file of the run is opened
    d = {k: str(tmp_path / v) for k, v in _FAKE.items()}
    flags = [f for f in _step7_flags(d, str(tmp_path / "no_model"), str(used)) if f != "--overwrite_output_dir"]
    with pytest.raises(ValueError, match="overwrite_output_dir"):
        run_train_conc.main(flags)


def test_query_dataset(tmp_path):
    from repconc_amd.models.jpq.finetune_jpq import QueryDataset
    (tmp_path / "queries").write_text("q5\t five \nq2\ttwo words\nq8\teight\nq1\tone\n")
    (tmp_path / "qrels").write_text("q8 0 d7 1\nq2 0 d9 1\nq2 0 d3 2\nq5 0 d1 0\nq1 0 d3 1\n")
    index_doc_ids = np.array(["d7", "d3", "d9", "d1"])
    ds = QueryDataset(None, str(tmp_path / "qrels"), str(tmp_path / "queries"), 16, index_doc_ids, verbose=False)
    assert ds.get_qrels() == {2: [0], 1: [2, 1], 3: [1]} and ds.qids == [1, 2, 3] and len(ds) == 3
    assert [ds[i] for i in range(3)] == [{"query": "two words", "qid": 1}, {"query": "eight", "qid": 2},
                                         {"query": "one", "qid": 3}]
    assert ds.max_query_len == 16
    strict = QueryDataset(None, str(tmp_path / "qrels"), str(tmp_path / "queries"), 16, index_doc_ids, rel_threshold=2,
                          verbose=False)
    assert strict.get_qrels() == {1: [1]} and strict.qids == [1]
    # integer ids (corpus_ids.npy of an MS MARCO index) address the same way
    (tmp_path / "iq").write_text("11\ta\n12\tb\n")
    (tmp_path / "ir").write_text("12 0 1003 1\n11 0 1001 1\n")
    ints = QueryDataset(None, str(tmp_path / "ir"), str(tmp_path / "iq"), 16, np.array([1003, 1002, 1001]), verbose=False)
    assert ints.get_qrels() == {1: [0], 0: [2]} and ints.qids == [0, 1]
    for line, named in (("q9 0 d1 1\n", "q9"), ("q2 0 d99 1\n", "d99")):
        (tmp_path / "bad").write_text("q8 0 d7 1\n" + line)
        with pytest.raises(ValueError, match=named) as e:
            QueryDataset(None, str(tmp_path / "bad"), str(tmp_path / "queries"), 16, index_doc_ids, verbose=False)
        assert not isinstance(e.value, KeyError) and "bad:2" in str(e.value)


class _StubTokenizer:
    """Whitespace tokenizer with the keyword surface the collators use; records the keywords of the last call."""
    sep_token = "[SEP]"

    def __init__(self):
        self.last = None

    def _encode(self, texts, max_length):
        import torch
        rows = [[1] + [3 + len(w) for w in t.split()][: max_length - 2] + [2] for t in texts]
        L = max(map(len, rows))
        return {"input_ids": torch.tensor([r + [0] * (L - len(r)) for r in rows], dtype=torch.long),
                "attention_mask": torch.tensor([[1] * len(r) + [0] * (L - len(r)) for r in rows], dtype=torch.long)}

    def __call__(self, texts, padding=True, return_tensors=None, add_special_tokens=True, return_attention_mask=True,
                 return_token_type_ids=False, truncation=True, max_length=32):
        self.last = dict(return_tensors=return_tensors, max_length=max_length, truncation=truncation)
        return self._encode(texts, max_length)


class _TypedStubTokenizer(_StubTokenizer):
    def __call__(self, texts, input_text_type=None, max_length=32, **kw):
        self.last = dict(kw, input_text_type=input_text_type, max_length=max_length)
        return self._encode(texts, max_length)


def test_finetune_query_collator():
    import torch
    from repconc_amd.models.jpq.finetune_jpq import FinetuneQueryCollator
    feats = [{"query": "a bb ccc", "qid": 7}, {"query": "one two three four five six seven", "qid": 2}, {"query": "x", "qid": 40}]
    tok = _StubTokenizer()
    batch = FinetuneQueryCollator(tok, 6)(feats)
    assert set(batch) == {"query_input_ids", "query_attention_mask", "qids"}
    assert all(v.dtype == torch.int64 for v in batch.values())
    assert batch["query_input_ids"].shape == batch["query_attention_mask"].shape == (3, 6) and batch["qids"].tolist() == [7, 2, 40]
    assert batch["query_attention_mask"].sum(1).tolist() == [5, 6, 3]
    assert tok.last == {"return_tensors": "pt", "max_length": 6, "truncation": True}
    typed = _TypedStubTokenizer()
    FinetuneQueryCollator(typed, 9)(feats)
    assert typed.last["input_text_type"] == "query" and typed.last["max_length"] == 9 and typed.last["return_tensors"] == "pt"


def test_run_train_jpq_refuses_a_cpu_device_before_anything_is_loaded(tmp_path, capsys):
    from repconc_amd.train import run_train_jpq
    from repconc_amd.train.entry_common import CPU_REFUSED
    d = {k: str(tmp_path / v) for k, v in _FAKE.items()}                   # none of these files exists: nothing may be opened
    flags = _step9_flags(d, str(tmp_path / "no_model"), str(tmp_path / "no_index"), str(tmp_path / "out")) + ["--use_cpu"]
    with pytest.raises(SystemExit) as e:
        run_train_jpq.main(flags)
    assert e.value.code != 0
    assert "the PQ head and the index live on the GPU" in CPU_REFUSED and CPU_REFUSED in capsys.readouterr().err
    assert not (tmp_path / "out").exists()


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """The dataset files, one M = 48 checkpoint with its tokenizer, and the validation triple — written once."""
    root = tmp_path_factory.mktemp("train_entry")
    d = _write_dataset(str(root / "data"))
    ckpt = _repconc_checkpoint(str(root / "warmup"))
    return {"root": root, "data": d, "ckpt": ckpt}


def _validation(d, sep="[SEP]"):
    from repconc_amd.utils.eval_utils import _parse_qrel, load_corpus, load_queries
    return load_corpus(d["corpus.tsv"], sep), load_queries(d["query.dev"]), _parse_qrel(d["qrels.dev"])


def _by_hand(model, tok, args, queries, qrels, corpus=None, index=None, corpus_ids=None):
    """What `evaluate` is specified to compute, composed from the package's functions on the same model and arguments."""
    from repconc_amd.models.repconc.evaluate_repconc import batch_search, encode_corpus, encode_query, load_index_to_gpu
    from repconc_amd.utils.eval_utils import pytrec_evaluate
    assert not args.fp16 and not args.bf16
    if corpus is not None:
        constraint, model.use_constraint = model.use_constraint, False
        index, corpus_ids = encode_corpus(corpus, model, tok, 40, args)
        model.use_constraint = constraint
        index = load_index_to_gpu(index, index.device.index)
    qemb, qids = encode_query(queries, model, tok, 40, args)
    scores, ids = batch_search(qids, qemb, corpus_ids, index, topk=10, batch_size=512)
    run = {}
    for qid, s_row, d_row in zip(qids, scores, ids):
        for s, did in zip(s_row, d_row):
            run.setdefault(str(qid.item()), {})[str(did.item())] = s.item()
    got = pytrec_evaluate(qrels, run, k_values=(10,), mrr_k_values=(10,))
    return {f"eval_{name}": v for cat, ms in got.items() if cat != "perquery" for name, v in ms.items()}


@gpu
def test_stage1_evaluate_equals_the_hand_made_composition_and_restores_its_switches(work, tmp_path, monkeypatch):
    import torch
    from transformers import AutoTokenizer
    from repconc_amd.models.repconc import evaluate_repconc
    from repconc_amd.models.repconc.finetune_repconc import (FinetuneCollator, RepCONCFinetuneArguments, RepCONCFinetuner,
                                                             validation_max_length)
    tok = AutoTokenizer.from_pretrained(work["ckpt"])
    model = _repconc_model(use_constraint=True).to("cuda:0")
    assert validation_max_length(model.config) == 40          # the reference's 512, capped by the encoder's 40 positions
    corpus, queries, qrels = _validation(work["data"])
    args = RepCONCFinetuneArguments(output_dir=str(tmp_path / "o"), per_device_train_batch_size=8, cache_chunk_size=8,
                                    per_device_eval_batch_size=64, save_strategy="no", report_to=[],
                                    dataloader_drop_last=True, max_steps=1)
    trainer = RepCONCFinetuner(qrels={0: [0]}, model=model, args=args, train_dataset=[{"x": 0}] * 8,
                               data_collator=FinetuneCollator(tok, 16, 32), tokenizer=tok,
                               eval_dataset=(corpus, queries, qrels))
    assert trainer.tokenizer is tok and trainer.processing_class is tok and trainer.eval_dataset[0] is corpus
    same = RepCONCFinetuner(qrels={}, model=model, args=args, train_dataset=[{"x": 0}] * 8, tokenizer=tok, processing_class=tok)
    assert same.tokenizer is tok
    with pytest.raises(ValueError, match="two different"):
        RepCONCFinetuner(qrels={}, model=model, args=args, train_dataset=[{"x": 0}] * 8, tokenizer=tok,
                         processing_class=AutoTokenizer.from_pretrained(work["ckpt"]))
    want = _by_hand(model, tok, args, queries, qrels, corpus=corpus)
    assert set(want) >= {"eval_MRR@10", "eval_NDCG@10", "eval_Recall@10"}
    assert 0 < want["eval_MRR@10"] < 1 and 0 < want["eval_Recall@10"] < 1          # the comparison is not one of zeros

    seen = []
    real_corpus, real_query = evaluate_repconc.encode_corpus, evaluate_repconc.encode_query

    def spy(fn):
        def wrapped(texts, m, tokenizer, max_seq_length, eval_args):
            seen.append((fn.__name__, m.use_constraint, eval_args.fp16, eval_args.bf16, eval_args.dataloader_drop_last,
                         max_seq_length, tokenizer is tok))
            return fn(texts, m, tokenizer, max_seq_length, eval_args)
        return wrapped
    monkeypatch.setattr(evaluate_repconc, "encode_corpus", spy(real_corpus))
    monkeypatch.setattr(evaluate_repconc, "encode_query", spy(real_query))
    args.bf16 = True                        # only read by evaluate here: nothing trains in this test
    got = trainer.evaluate()
    assert got == want, (got, want)
    assert seen == [("encode_corpus", False, False, False, False, 40, True), ("encode_query", False, False, False, False, 40, True)]
    assert (model.use_constraint, args.fp16, args.bf16, args.dataloader_drop_last) == (True, False, True, True)
    logged = trainer.state.log_history[-1]
    assert all(logged[k] == v for k, v in want.items())
    assert trainer.evaluate(metric_key_prefix="test") == {"test" + k[4:]: v for k, v in want.items()}

    def broken(*a, **k):
        raise RuntimeError("query encoding failed")
    monkeypatch.setattr(evaluate_repconc, "encode_query", broken)
    with pytest.raises(RuntimeError, match="query encoding failed"):
        trainer.evaluate()
    assert (model.use_constraint, args.fp16, args.bf16, args.dataloader_drop_last) == (True, False, True, True)


def _conc_flags(work, out, max_steps, extra=()):
    d = work["data"]
    return ["--qrel_path", d["qrels.train"], "--query_path", d["query.train"], "--corpus_path", d["corpus.tsv"],
            "--valid_qrel_path", d["qrels.dev"], "--valid_query_path", d["query.dev"], "--valid_corpus_path", d["corpus.tsv"],
            "--output_dir", out, "--model_name_or_path", work["ckpt"], "--logging_steps", "1", "--max_query_len", "16",
            "--max_doc_len", "32", "--per_device_train_batch_size", "16", "--per_device_eval_batch_size", "64",
            "--negative_per_query", "3", "--dynamic_topk_hard_negative", "3", "--learning_rate", "2e-5",
            "--centroid_learning_rate", "5e-4", "--max_steps", str(max_steps), "--dataloader_drop_last",
            "--dataloader_num_workers", "0", "--weight_decay", "0", "--lr_scheduler_type", "constant", "--cache_chunk_size",
            "8", "--mse_loss_weight", "1e-4", "--negative", d["hardneg.json"], "--sk_epsilon", "0.003", "--sk_iters", "20",
            "--report_to", "none"] + list(extra)


_VALIDATED = ["--metric_for_best_model", "MRR@10", "--save_total_limit", "2", "--evaluation_strategy", "steps",
              "--save_strategy", "steps", "--eval_steps", "2", "--save_steps", "2", "--load_best_model_at_end"]


def _state(out_dir):
    with open(os.path.join(out_dir, "trainer_state.json")) as f:
        return json.load(f)


def _check_validated_run(out, state_dir, n_evals):
    """Layout of the output directory and of its checkpoints, the evaluations in the trainer state, and the best model
    reloaded at the end."""
    import torch
    from transformers import AutoTokenizer
    from repconc_amd.models.repconc import RepCONC
    for d in [out] + [os.path.join(out, c) for c in os.listdir(out) if c.startswith("checkpoint-")]:
        for name in ("pytorch_model.bin", "config.json", "dense_encoder", "tokenizer_config.json", "tokenizer.json"):
            assert os.path.exists(os.path.join(d, name)), (d, name)
        assert AutoTokenizer.from_pretrained(d)(["w1 w299 zz"])["input_ids"] == [[2, 6, 304, 1, 3]]
    state = _state(state_dir)
    evals = [(e["step"], e["eval_MRR@10"]) for e in state["log_history"] if "eval_MRR@10" in e]
    assert len(evals) == n_evals and [s for s, _ in evals] == [2 * (i + 1) for i in range(n_evals)]
    assert all({"eval_NDCG@10", "eval_Recall@10"} <= set(e) for e in state["log_history"] if "eval_MRR@10" in e)
    best_step = max(evals, key=lambda e: (e[1], -e[0]))[0]                  # the larger one, the first at a tie
    assert state["best_model_checkpoint"] == os.path.join(out, f"checkpoint-{best_step}")
    assert state["best_metric"] == dict(evals)[best_step]
    final = torch.load(os.path.join(out, "pytorch_model.bin"), map_location="cpu")
    best = torch.load(os.path.join(out, f"checkpoint-{best_step}", "pytorch_model.bin"), map_location="cpu")
    assert set(final) == set(best) and {"rotation", "centroids"} <= set(final)
    assert any(k.startswith("dense_encoder.") for k in final) and all(torch.equal(final[k], best[k]) for k in final)
    model = RepCONC.from_pretrained(out, False, None, None)
    assert torch.equal(model.centroids.data, final["centroids"]) and torch.equal(model.rotation, final["rotation"])
    return state, final


@pytest.fixture(scope="module")
def conc_run(work):
    """One stage-1 run with validation through run_train_conc.main: 4 steps, evaluated and saved every 2."""
    from repconc_amd.train import run_train_conc
    out = str(work["root"] / "conc_out")
    trainer = run_train_conc.main(_conc_flags(work, out, 4, _VALIDATED))
    return {"out": out, "global_step": trainer.state.global_step, "wrapped": type(trainer.model_wrapped).__name__}


@gpu
def test_run_train_conc_with_validation_and_best_model(work, conc_run, tmp_path):
    import torch
    from repconc_amd.evaluate import run_repconc_eval
    out = conc_run["out"]
    assert conc_run["global_step"] == 4 and conc_run["wrapped"] == "RepCONC"            # not nn.DataParallel
    assert sorted(c for c in os.listdir(out) if c.startswith("checkpoint-")) == ["checkpoint-2", "checkpoint-4"]
    state, final = _check_validated_run(out, os.path.join(out, "checkpoint-4"), 2)
    assert [e["step"] for e in state["log_history"] if "loss" in e] == [1, 2, 3, 4]
    assert all(np.isfinite(e["loss"]) for e in state["log_history"] if "loss" in e)
    start = torch.load(os.path.join(work["ckpt"], "pytorch_model.bin"), map_location="cpu")
    assert not torch.equal(start["centroids"], final["centroids"]) and torch.equal(start["rotation"], final["rotation"])
    d = work["data"]
    run_repconc_eval.main(["--model_name_or_path", out, "--max_seq_length", "32", "--corpus_path", d["corpus.tsv"],
                           "--query_path", d["query.dev"], "--qrel_path", d["qrels.dev"], "--out_corpus_dir",
                           str(tmp_path / "corpus"), "--out_query_dir", str(tmp_path / "query"), "--topk", "10",
                           "--per_device_eval_batch_size", "64", "--output_dir", str(tmp_path / "trainer"), "--report_to",
                           "none"])
    assert len((tmp_path / "query" / "run.tsv").read_text().splitlines()) == 12 * 10
    with open(tmp_path / "query" / "metric.json") as f:
        assert "MRR@10" in json.load(f)["mrr"]


@gpu
@pytest.mark.parametrize("variant", [["--fp16"], ["--fused_contrastive_loss", "--deterministic_decode"]],
                         ids=["fp16", "fused_loss_det_decode"])
def test_run_train_conc_variants_give_a_finite_loss(work, tmp_path, variant):
    from repconc_amd.train import run_train_conc
    trainer = run_train_conc.main(_conc_flags(work, str(tmp_path / "out"), 2, ["--save_strategy", "no"] + variant))
    losses = [e["loss"] for e in trainer.state.log_history if "loss" in e]
    assert trainer.state.global_step == 2 and len(losses) == 2 and all(np.isfinite(x) for x in losses)
    assert trainer.model.deterministic_decode is (True if "--deterministic_decode" in variant else None)
    assert os.path.exists(tmp_path / "out" / "pytorch_model.bin")


@gpu
def test_run_train_conc_resumes_from_the_last_checkpoint(work, conc_run, tmp_path):
    from repconc_amd.train import run_train_conc
    out = str(tmp_path / "resumed")
    shutil.copytree(conc_run["out"], out)
    before = _state(os.path.join(out, "checkpoint-4"))
    with pytest.raises(ValueError, match="overwrite_output_dir"):
        run_train_conc.main(_conc_flags(work, out, 6, _VALIDATED))
    steps_run = []
    real = run_train_conc.RepCONCFinetuner.training_step

    def counting(self, *a, **k):
        steps_run.append(self.state.global_step + 1)
        return real(self, *a, **k)
    run_train_conc.RepCONCFinetuner.training_step = counting
    try:
        trainer = run_train_conc.main(_conc_flags(work, out, 6, _VALIDATED + ["--overwrite_output_dir"]))
    finally:
        run_train_conc.RepCONCFinetuner.training_step = real
    assert trainer.state.global_step == 6 and steps_run == [5, 6]
    history = trainer.state.log_history
    assert history[:len(before["log_history"])] == before["log_history"]               # steps 1-4 come from the checkpoint
    assert [e["step"] for e in history[len(before["log_history"]):] if "loss" in e] == [5, 6]
    assert [e["step"] for e in history if "eval_MRR@10" in e] == [2, 4, 6]
    assert os.path.isdir(os.path.join(out, "checkpoint-6"))


# ---------------------------------------------------------------------------------------------------------- stage 2
def _random_index(model, n_rows, seed=11):
    import torch
    from repconc_amd.index import PQIndex
    dev = model.centroids.device
    index = PQIndex(768, model.config.MCQ_M, device=dev)
    index.set_centroids(model.centroids.data)
    g = torch.Generator().manual_seed(seed)
    index.add_codes(torch.randint(0, 256, (n_rows, model.config.MCQ_M), generator=g, dtype=torch.uint8))
    return index


def _jpq_trainer(work, tmp_path, metric="METRIC_IP", n_rows=300, callbacks=(), **arg_kw):
    from transformers import AutoTokenizer
    from repconc_amd.models.jpq.finetune_jpq import JPQ, FinetuneQueryCollator, JPQFinetuneArguments, JPQFinetuner
    from repconc_amd.utils.eval_utils import _parse_qrel, load_queries
    tok = AutoTokenizer.from_pretrained(work["ckpt"])
    model = _repconc_model(metric=metric).to("cuda:0")
    index = _random_index(model, n_rows)
    rng = np.random.default_rng(5)
    words = [f"w{i}" for i in range(300)]
    train = [{"query": " ".join(rng.choice(words, rng.integers(2, 8))), "qid": i} for i in range(16)]
    qrels = {i: [int(r) for r in rng.choice(n_rows, 1 + i % 2, replace=False)] for i in range(16)}
    kw = dict(output_dir=str(tmp_path / "o"), per_device_train_batch_size=8, per_device_eval_batch_size=64, max_steps=3,
              learning_rate=1e-4, centroid_learning_rate=1e-3, weight_decay=0.01, lr_scheduler_type="constant",
              logging_steps=1, save_strategy="no", report_to=[], dataloader_num_workers=0)
    kw.update(arg_kw)
    args = JPQFinetuneArguments(**kw)
    jpq = JPQ(model, index, qrels, args.dynamic_topk_negative, args.temperature, 0, head=args.head)
    corpus_ids = np.array([str(1000 + i) for i in range(n_rows)])
    d = work["data"]
    valid = (corpus_ids, load_queries(d["query.dev"]), _parse_qrel(d["qrels.dev"]))
    trainer = JPQFinetuner(model=jpq, args=args, train_dataset=train, tokenizer=tok,
                           data_collator=FinetuneQueryCollator(tok, 16), eval_dataset=valid)
    for callback in callbacks:              # after the trainer's own: callbacks given to the constructor would run before them
        trainer.add_callback(callback)
    return trainer, jpq, index, tok, valid


def _step_checker(record):
    import torch
    from transformers import TrainerCallback
    from repconc_amd import ops

    class AfterEveryStep(TrainerCallback):
        """Added last, so it runs after the trainer's own normalise and sync callbacks."""

        def on_step_end(self, args, state, control, model=None, **kwargs):
            cent = model.repconc.centroids.data
            index = model.pq_index
            record.append({"step": state.global_step,
                           "table": torch.equal(index.pq.centroids, cent),
                           "decoded": torch.equal(index.reconstruct_n(0, index.ntotal),
                                                  ops.decode_raw(index.codes.contiguous(), cent)),
                           "centroids": cent.clone(),
                           "norms": cent.double().norm(dim=-1).cpu().numpy()})
    return AfterEveryStep()


@gpu
@pytest.mark.parametrize("metric", ["METRIC_IP", "METRIC_CENTROID_COS"])
def test_jpq_finetuner_keeps_the_index_in_step_with_the_centroids(work, tmp_path, metric):
    import torch
    from repconc_amd.models.jpq.finetune_jpq import JPQ_SyncIndex_Callback
    from repconc_amd.models.repconc.finetune_repconc import RepCONC_Norm_Centroid_Callback
    record = []
    trainer, jpq, index, tok, valid = _jpq_trainer(work, tmp_path, metric, callbacks=[_step_checker(record)])
    own = [type(c) if not isinstance(c, type) else c for c in trainer.callback_handler.callbacks]
    own = [c for c in own if c in (RepCONC_Norm_Centroid_Callback, JPQ_SyncIndex_Callback)]
    assert own == ([RepCONC_Norm_Centroid_Callback] if metric == "METRIC_CENTROID_COS" else []) + [JPQ_SyncIndex_Callback]
    assert trainer.floating_point_ops({}) == 0 and trainer.tokenizer is tok
    opt = trainer.create_optimizer()
    assert len(opt.param_groups) == 3
    assert len(opt.param_groups[2]["params"]) == 1 and opt.param_groups[2]["params"][0] is jpq.repconc.centroids
    assert opt.param_groups[2]["lr"] == 1e-3 and opt.param_groups[2]["weight_decay"] == 0.0
    assert opt.param_groups[0]["weight_decay"] == 0.01 and opt.param_groups[1]["weight_decay"] == 0.0
    assert opt.param_groups[0]["lr"] == 1e-4 and all(p.ndim >= 2 for p in opt.param_groups[0]["params"])
    grouped = {id(p) for g in opt.param_groups for p in g["params"]}
    assert grouped == {id(p) for p in jpq.parameters()} and id(jpq.repconc.rotation) not in grouped
    codes_before, start = index.codes.clone(), jpq.repconc.centroids.detach().clone()
    from repconc_amd.models.repconc.evaluate_repconc import batch_search, encode_query
    qemb, qids = encode_query(valid[1], jpq.repconc, tok, 40, trainer.args)
    ranked = batch_search(qids, qemb, valid[0], index, topk=10, batch_size=512)[1]
    judged = {str(q): {str(ranked[r][r % 10]): 1} for r, q in enumerate(qids.tolist())}
    out = trainer.train()
    assert out.global_step == 3 and np.isfinite(out.training_loss)
    assert [r["step"] for r in record] == [1, 2, 3] and all(r["table"] and r["decoded"] for r in record)
    assert not torch.equal(record[0]["centroids"], start) and not torch.equal(record[2]["centroids"], record[0]["centroids"])
    assert torch.equal(index.codes, codes_before) and index.ntotal == 300
    if metric == "METRIC_CENTROID_COS":
        for r in record:                # the band test_normalize_centroids pins on the normalised values
            np.testing.assert_allclose(r["norms"], 1.0, rtol=1e-6, atol=1e-7)
    # validation: the resident index, no second copy; equal to the hand-made composition.  The rows are random codes, so
    # the judged document of query r is taken from the ranking of the untrained model (rank r % 10 + 1): not all zeros
    trainer.eval_dataset = valid = (valid[0], valid[1], judged)
    want = _by_hand(jpq.repconc, tok, trainer.args, valid[1], valid[2], index=index, corpus_ids=valid[0])
    trainer.args.bf16, trainer.args.dataloader_drop_last = True, True
    got = trainer.evaluate()
    assert got == want and set(got) >= {"eval_MRR@10", "eval_NDCG@10", "eval_Recall@10"} and want["eval_MRR@10"] > 0
    assert (trainer.args.fp16, trainer.args.bf16, trainer.args.dataloader_drop_last) == (False, True, True)
    assert all(trainer.state.log_history[-1][k] == v for k, v in want.items())
    assert jpq.pq_index is index and torch.equal(index.codes, codes_before)


@gpu
def test_jpq_finetuner_switches_and_a_short_index(work, tmp_path):
    """head / deterministic_decode of the arguments reach the model; an index of 100 rows under dynamic_topk_negative = 200
    trains (the missing slots are padding), with both heads."""
    import torch
    for head in ("fused", "decode"):
        trainer, jpq, index, _, _ = _jpq_trainer(work, tmp_path / head, n_rows=100, head=head, deterministic_decode=True,
                                                 max_steps=2)
        assert jpq.head == head and jpq.neg_top_k == 200 and jpq.repconc.deterministic_decode is True
        start = jpq.repconc.centroids.detach().clone()
        out = trainer.train()
        assert out.global_step == 2 and np.isfinite(out.training_loss)
        assert not torch.equal(start, jpq.repconc.centroids.detach())
        assert torch.equal(index.pq.centroids, jpq.repconc.centroids.data)
    plain, jpq, _, _, _ = _jpq_trainer(work, tmp_path / "plain", n_rows=100)
    assert jpq.head == "decode" and jpq.repconc.deterministic_decode is None


class _EncodeArgs:
    per_device_eval_batch_size, fp16, bf16 = 64, False, False


def _index_dir(work, name, M=48):
    """A checkpoint and <dir>/index + corpus_ids.npy: the corpus coded by that checkpoint's model, as recipe step 8 leaves it."""
    from transformers import AutoTokenizer
    from repconc_amd.faiss_io import save_index_dir
    from repconc_amd.models.repconc.evaluate_repconc import encode_corpus
    from repconc_amd.utils.eval_utils import load_corpus
    ckpt = work["ckpt"] if M == 48 else _repconc_checkpoint(str(work["root"] / f"warmup_m{M}"), M)
    model = _repconc_model(M).to("cuda:0")
    index, corpus_ids = encode_corpus(load_corpus(work["data"]["corpus.tsv"], "[SEP]"), model,
                                      AutoTokenizer.from_pretrained(ckpt), 40, _EncodeArgs())
    path = str(work["root"] / name)
    save_index_dir(index, corpus_ids, path)
    return ckpt, path


def _jpq_flags(work, ckpt, index_dir, out, max_steps, extra=()):
    d = work["data"]
    return ["--qrel_path", d["qrels.train"], "--query_path", d["query.train"], "--valid_qrel_path", d["qrels.dev"],
            "--valid_query_path", d["query.dev"], "--output_dir", out, "--model_name_or_path", ckpt, "--index_input_dir",
            index_dir, "--logging_steps", "1", "--max_query_len", "16", "--per_device_train_batch_size", "8",
            "--per_device_eval_batch_size", "64", "--learning_rate", "1e-4", "--centroid_learning_rate", "1e-3",
            "--max_steps", str(max_steps), "--dataloader_drop_last", "--dataloader_num_workers", "0", "--weight_decay", "0",
            "--lr_scheduler_type", "constant", "--report_to", "none"] + list(extra)


def _file_bytes(index_dir):
    return {n: open(os.path.join(index_dir, n), "rb").read() for n in ("index", "corpus_ids.npy")}


@pytest.fixture(scope="module")
def jpq_run(work):
    """One stage-2 run with validation through run_train_jpq.main: 4 steps, evaluated and saved every 2."""
    from repconc_amd.train import run_train_jpq
    ckpt, index_dir = _index_dir(work, "index_m48")
    before = _file_bytes(index_dir)
    out = str(work["root"] / "jpq_out")
    trainer = run_train_jpq.main(_jpq_flags(work, ckpt, index_dir, out, 4, _VALIDATED))
    return {"out": out, "ckpt": ckpt, "index_dir": index_dir, "before": before, "global_step": trainer.state.global_step,
            "wrapped": type(trainer.model_wrapped).__name__,
            "model_centroids": trainer.model.repconc.centroids.data.cpu().clone(),
            "index_centroids": trainer.model.pq_index.pq.centroids.cpu().clone()}


@gpu
def test_run_train_jpq_with_validation_then_the_after_jpq_evaluation(work, jpq_run, tmp_path):
    import torch
    from repconc_amd.evaluate import run_repconc_eval
    out, ckpt, index_dir, before = (jpq_run[k] for k in ("out", "ckpt", "index_dir", "before"))
    assert jpq_run["global_step"] == 4 and jpq_run["wrapped"] == "JPQ"
    assert sorted(c for c in os.listdir(out) if c.startswith("checkpoint-")) == ["checkpoint-2", "checkpoint-4"]
    state, final = _check_validated_run(out, os.path.join(out, "checkpoint-4"), 2)
    assert [e["step"] for e in state["log_history"] if "loss" in e] == [1, 2, 3, 4]
    # the best checkpoint went through JPQ.load_state_dict: model and resident index hold it
    assert torch.equal(jpq_run["model_centroids"], final["centroids"])
    assert torch.equal(jpq_run["index_centroids"], final["centroids"])
    start = torch.load(os.path.join(ckpt, "pytorch_model.bin"), map_location="cpu")
    assert not torch.equal(start["centroids"], final["centroids"]) and torch.equal(start["rotation"], final["rotation"])
    assert _file_bytes(index_dir) == before and sorted(os.listdir(index_dir)) == ["corpus_ids.npy", "index"]
    # the after-JPQ evaluation (recipe step 10): corpus cache = the index directory, query encoder = the output
    d = work["data"]
    run_repconc_eval.main(["--doc_encoder_path", ckpt, "--query_encoder_path", out, "--max_seq_length", "32",
                           "--corpus_path", d["corpus.tsv"], "--query_path", d["query.dev"], "--qrel_path", d["qrels.dev"],
                           "--out_corpus_dir", index_dir, "--out_query_dir", str(tmp_path / "query"), "--topk", "10",
                           "--per_device_eval_batch_size", "64", "--output_dir", str(tmp_path / "trainer"), "--report_to",
                           "none"])
    with open(tmp_path / "query" / "metric.json") as f:
        assert "MRR@10" in json.load(f)["mrr"]
    assert _file_bytes(index_dir) == before and sorted(os.listdir(index_dir)) == ["corpus_ids.npy", "index"]


@gpu
def test_run_train_jpq_resumes_from_the_last_checkpoint(work, jpq_run, tmp_path):
    from repconc_amd.train import run_train_jpq
    ckpt, index_dir = jpq_run["ckpt"], jpq_run["index_dir"]
    out = str(tmp_path / "resumed")
    shutil.copytree(jpq_run["out"], out)
    with pytest.raises(ValueError, match="overwrite_output_dir"):
        run_train_jpq.main(_jpq_flags(work, ckpt, index_dir, out, 6, _VALIDATED))
    kept = _state(os.path.join(out, "checkpoint-4"))["log_history"]
    resumed = run_train_jpq.main(_jpq_flags(work, ckpt, index_dir, out, 6, _VALIDATED + ["--overwrite_output_dir"]))
    history = resumed.state.log_history
    assert resumed.state.global_step == 6 and history[:len(kept)] == kept
    assert [e["step"] for e in history[len(kept):] if "loss" in e] == [5, 6]
    assert [e["step"] for e in history if "eval_MRR@10" in e] == [2, 4, 6]
    assert os.path.isdir(os.path.join(out, "checkpoint-6")) and _file_bytes(index_dir) == jpq_run["before"]


@gpu
def test_run_train_jpq_m96(work, tmp_path):
    from repconc_amd.train import run_train_jpq
    ckpt, index_dir = _index_dir(work, "index_m96", M=96)
    before = _file_bytes(index_dir)
    out = str(tmp_path / "out")
    trainer = run_train_jpq.main(_jpq_flags(work, ckpt, index_dir, out, 4, _VALIDATED + ["--head", "fused"]))
    assert trainer.state.global_step == 4 and trainer.model.head == "fused" and trainer.model.repconc.config.MCQ_M == 96
    _, final = _check_validated_run(out, os.path.join(out, "checkpoint-4"), 2)
    assert tuple(final["centroids"].shape) == (96, 256, 8) and _file_bytes(index_dir) == before


@gpu
def test_python_m_run_train_jpq_through_the_alias_in_a_child(work, tmp_path):
    """One child, never retried: the module the recipes start, two steps, no validation."""
    from repconc_amd.train import run_train_jpq
    alias = "repconc." + run_train_jpq.__name__.split(".", 1)[1]
    assert alias == "repconc.train.run_train_jpq"
    ckpt, index_dir = _index_dir(work, "index_child")
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, "-m", alias]
                       + _jpq_flags(work, ckpt, index_dir, out, 2, ["--save_strategy", "no", "--overwrite_output_dir"]),
                       env=ENV, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    for name in ("pytorch_model.bin", "config.json", "dense_encoder", "tokenizer_config.json"):
        assert os.path.exists(os.path.join(out, name)), name
