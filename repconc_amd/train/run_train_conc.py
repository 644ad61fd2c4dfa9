"""`python -m repconc.train.run_train_conc`: stage-1 training of a RepCONC model (the reference's train/run_train_conc.py,
recipe step 7) — same arguments, same call order: tokenizer and warmed-up model, the validation triple, `QDRelDataset` +
`FinetuneCollator`, `RepCONCFinetuner.train(resume_from_checkpoint=...)`, `save_model()`.

The recipes' `--evaluation_strategy` and `--overwrite_output_dir` are fields of `RepCONCFinetuneArguments`; the validation
qrels are read by eval_utils' own parser (no pytrec_eval).  A CPU device is refused before anything is loaded.  One process
trains on one device.  Started by a launcher (`torchrun`), every rank runs this module and the trainer gathers the batch
across ranks — by construction only: more than one rank has not been run.
"""
import logging
from dataclasses import dataclass, field

from transformers import AutoTokenizer, HfArgumentParser, set_seed
from transformers.trainer_utils import is_main_process

from ..models.repconc import RepCONC
from ..models.repconc.finetune_repconc import (DataTrainingArguments, FinetuneCollator, QDRelDataset,
                                               RepCONCFinetuneArguments, RepCONCFinetuner)
from .entry_common import one_device_per_process, parse_arguments, refuse_cpu, resume_from_output_dir, setup_logging

logger = logging.getLogger(__name__)


@dataclass
class ModelArguments:
    model_name_or_path: str = field()
    sk_epsilon: float = field()
    sk_iters: int = field()


def load_validation_set(corpus_path, query_path, qrel_path, sep_token):
    """(corpus, queries, qrels) as `RepCONCFinetuner.evaluate` takes them.  run_train_conc.py:31-38."""
    from ..utils.eval_utils import _parse_qrel, load_corpus, load_queries
    return load_corpus(corpus_path, sep_token=sep_token), load_queries(query_path), _parse_qrel(qrel_path)


def main(argv=None):
    parser = HfArgumentParser((ModelArguments, DataTrainingArguments, RepCONCFinetuneArguments))
    model_args, data_args, training_args = parse_arguments(parser, argv)
    setup_logging(training_args)
    resume_from_checkpoint = resume_from_output_dir(training_args)
    refuse_cpu(parser, training_args)
    one_device_per_process(training_args)
    logger.warning("Process rank: %s, device: %s, n_gpu: %s, distributed training: %s, 16-bits training: %s",
                   training_args.local_rank, training_args.device, training_args.n_gpu,
                   bool(training_args.local_rank != -1), training_args.fp16)
    logger.info("Model parameters %s", model_args)
    logger.info("Data parameters %s", data_args)
    logger.info("Training parameters %s", training_args)
    set_seed(training_args.seed)

    tokenizer = AutoTokenizer.from_pretrained(model_args.model_name_or_path, use_fast=True)
    repconc = RepCONC.from_pretrained(model_args.model_name_or_path, not training_args.not_use_constraint,
                                      model_args.sk_epsilon, model_args.sk_iters)
    eval_dataset = load_validation_set(data_args.valid_corpus_path, data_args.valid_query_path, data_args.valid_qrel_path,
                                       sep_token=tokenizer.sep_token)
    train_set = QDRelDataset(tokenizer, qrel_path=data_args.qrel_path, query_path=data_args.query_path,
                             corpus_path=data_args.corpus_path, max_query_len=data_args.max_query_len,
                             max_doc_len=data_args.max_doc_len, negative=training_args.negative,
                             negative_per_query=training_args.negative_per_query, rel_threshold=1,
                             verbose=is_main_process(training_args.local_rank))
    data_collator = FinetuneCollator(tokenizer=tokenizer, max_query_len=data_args.max_query_len,
                                     max_doc_len=data_args.max_doc_len)
    trainer = RepCONCFinetuner(qrels=train_set.get_qrels(), model=repconc, args=training_args, train_dataset=train_set,
                               tokenizer=tokenizer, data_collator=data_collator, eval_dataset=eval_dataset)
    trainer.train(resume_from_checkpoint=resume_from_checkpoint)
    trainer.save_model()
    return trainer


if __name__ == "__main__":
    main()
