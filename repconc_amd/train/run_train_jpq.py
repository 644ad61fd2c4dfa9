"""`python -m repconc.train.run_train_jpq`: stage-2 (JPQ) training of the query encoder and the centroids against a fixed
code index (the reference's train/run_train_jpq.py, recipe step 9) — same arguments, same call order: tokenizer and model,
`<index_input_dir>/index` + `corpus_ids.npy`, the validation queries and qrels, `QueryDataset` + `FinetuneQueryCollator`,
`JPQ`, `JPQFinetuner.train(resume_from_checkpoint=...)`, `save_model()`.

The index is read onto the device once and stays there: nothing is written into `index_input_dir`.  The recipes'
`--evaluation_strategy` and `--overwrite_output_dir` are fields of `JPQFinetuneArguments`, next to this package's `--head`
and `--deterministic_decode`.  A CPU device is refused before anything is loaded; more than one process is refused as the
reference asserts (run_train_jpq.py:95).
"""
import logging
from dataclasses import dataclass, field

from transformers import AutoTokenizer, HfArgumentParser, set_seed
from transformers.trainer_utils import is_main_process

from ..faiss_io import load_index_dir
from ..models.jpq.finetune_jpq import (JPQ, DataTrainingArguments, FinetuneQueryCollator, JPQFinetuneArguments,
                                       JPQFinetuner, QueryDataset)
from ..models.repconc import RepCONC
from .entry_common import one_device_per_process, parse_arguments, refuse_cpu, resume_from_output_dir, setup_logging

logger = logging.getLogger(__name__)

MULTI_PROCESS_REFUSED = "JPQ training runs in one process on one device: start it without a launcher"


@dataclass
class ModelArguments:
    model_name_or_path: str = field()
    index_input_dir: str = field()


def load_validation_set(query_path, qrel_path):
    """(queries, qrels).  run_train_jpq.py:34-40."""
    from ..utils.eval_utils import _parse_qrel, load_queries
    return load_queries(query_path), _parse_qrel(qrel_path)


def main(argv=None):
    parser = HfArgumentParser((ModelArguments, DataTrainingArguments, JPQFinetuneArguments))
    model_args, data_args, training_args = parse_arguments(parser, argv)
    setup_logging(training_args)
    resume_from_checkpoint = resume_from_output_dir(training_args)
    refuse_cpu(parser, training_args)
    if training_args.world_size > 1:
        parser.error(MULTI_PROCESS_REFUSED)
    one_device_per_process(training_args)
    logger.warning("Process rank: %s, device: %s, n_gpu: %s, 16-bits training: %s", training_args.local_rank,
                   training_args.device, training_args.n_gpu, training_args.fp16)
    logger.info("Model parameters %s", model_args)
    logger.info("Data parameters %s", data_args)
    logger.info("Training parameters %s", training_args)
    set_seed(training_args.seed)

    tokenizer = AutoTokenizer.from_pretrained(model_args.model_name_or_path)
    repconc = RepCONC.from_pretrained(model_args.model_name_or_path, False, None, None).to(training_args.device)
    pq_index, corpus_ids = load_index_dir(model_args.index_input_dir, device=training_args.device)
    valid_queries, valid_qrels = load_validation_set(data_args.valid_query_path, data_args.valid_qrel_path)
    train_set = QueryDataset(tokenizer, qrel_path=data_args.qrel_path, query_path=data_args.query_path,
                             max_query_len=data_args.max_query_len, index_doc_ids=corpus_ids, rel_threshold=1,
                             verbose=is_main_process(training_args.local_rank))
    data_collator = FinetuneQueryCollator(tokenizer=tokenizer, max_query_len=data_args.max_query_len)
    jpq = JPQ(repconc=repconc, pq_index=pq_index, qrels=train_set.get_qrels(), neg_top_k=training_args.dynamic_topk_negative,
              temperature=training_args.temperature, gpu_id=training_args.device.index, head=training_args.head)
    trainer = JPQFinetuner(model=jpq, args=training_args, train_dataset=train_set, tokenizer=tokenizer,
                           data_collator=data_collator, eval_dataset=(corpus_ids, valid_queries, valid_qrels))
    trainer.train(resume_from_checkpoint=resume_from_checkpoint)
    trainer.save_model()
    return trainer


if __name__ == "__main__":
    main()
