"""`python -m repconc.utils.customize_trained_dense` (recipe step 2): set how a trained dense model scores
(`similarity_metric`) and pools (`pooling`) in its config, then save the model and its tokenizer to `output_dir`.
The reference's utils/customize_trained_dense.py, same arguments."""
import logging
from dataclasses import dataclass, field

import transformers
from transformers import AutoConfig, AutoTokenizer, HfArgumentParser, set_seed

from ..models.dense import AutoDense


@dataclass
class ModelArguments:
    model_name_or_path: str = field(metadata={"help": "The dense model to customize"})
    similarity_metric: str = field(metadata={"help": "How the dense model computes similarity",
                                             "choices": ["METRIC_IP", "METRIC_COS"]})
    pooling: str = field(metadata={"help": "How the dense model pools token representations into a text embedding",
                                   "choices": ["cls", "mean"]})
    output_dir: str = field(metadata={"help": "Where to save the customized model"})


def main(argv=None):
    model_args, = HfArgumentParser(ModelArguments).parse_args_into_dataclasses(argv)
    logging.basicConfig(format="%(asctime)s - %(levelname)s - %(name)s -   %(message)s", datefmt="%m/%d/%Y %H:%M:%S",
                        level=logging.INFO)
    transformers.utils.logging.set_verbosity_info()
    transformers.utils.logging.enable_default_handler()
    transformers.utils.logging.enable_explicit_format()
    set_seed(2022)

    tokenizer = AutoTokenizer.from_pretrained(model_args.model_name_or_path)
    config = AutoConfig.from_pretrained(model_args.model_name_or_path)
    config.similarity_metric = model_args.similarity_metric
    config.pooling = model_args.pooling
    model = AutoDense.from_pretrained(model_args.model_name_or_path, config=config)
    tokenizer.save_pretrained(model_args.output_dir)
    model.save_pretrained(model_args.output_dir)


if __name__ == "__main__":
    main()
