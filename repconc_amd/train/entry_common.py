"""What the two training entry points (run_train_conc, run_train_jpq) share — the reference repeats these lines in both
scripts (run_train_conc.py:46-94, run_train_jpq.py:48-97): argument parsing with the single-json form, logging set-up, the
output-directory rule, and this package's two device rules (no CPU path; one process trains on one device)."""
from __future__ import annotations

import logging
import os
import sys

import transformers
from transformers.trainer_utils import is_main_process

CPU_REFUSED = ("training on a CPU device is not possible: the PQ head and the index live on the GPU "
               "(run on a ROCm device, without --use_cpu)")


def parse_arguments(parser, argv=None):
    """`parse_args_into_dataclasses`, or — a single `*.json` argument — `parse_json_file`."""
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) == 1 and str(argv[0]).endswith(".json"):
        return parser.parse_json_file(json_file=os.path.abspath(argv[0]))
    return parser.parse_args_into_dataclasses(argv)


def setup_logging(training_args):
    main_process = is_main_process(training_args.local_rank)
    logging.basicConfig(format="%(asctime)s-%(levelname)s-%(name)s- %(message)s", datefmt="%m/%d/%Y %H:%M:%S",
                        level=logging.INFO if main_process else logging.WARN)
    if main_process:
        transformers.utils.logging.set_verbosity_info()
        transformers.utils.logging.enable_default_handler()
        transformers.utils.logging.enable_explicit_format()


def resume_from_output_dir(training_args) -> bool:
    """The reference's output-directory rule: a directory that holds a `checkpoint*` entry is an error without
    `--overwrite_output_dir`; with the flag the run resumes from its last checkpoint.  Anything else is a fresh run."""
    out = training_args.output_dir
    if not (os.path.isdir(out) and any(x.startswith("checkpoint") for x in os.listdir(out))):
        return False
    if not training_args.overwrite_output_dir:
        raise ValueError(f"Output directory ({out}) already exists and is not empty. Use --overwrite_output_dir to overcome.")
    return True


def refuse_cpu(parser, training_args):
    """Ends the run (usage error) when the arguments resolve to a CPU device, before anything is loaded or encoded."""
    if training_args.device.type != "cuda":
        parser.error(CPU_REFUSED)


def one_device_per_process(training_args):
    """Several visible devices and no launcher: the stock Trainer would wrap the model in nn.DataParallel, which neither the
    cached-gradient step nor the resident index supports.  The process trains on its current device only."""
    if training_args.n_gpu > 1:
        logging.getLogger(__name__).warning("%d devices visible, no launcher: training on %s only", training_args.n_gpu,
                                            training_args.device)
        training_args._n_gpu = 1
