"""`python -m repconc.train.run_gen_valid_set` (recipe step 4): a small validation set — the qrels and query files
copied, and the corpus cut to the documents the qrels judge (at any relevance) plus those a run ranks <= --topk for the
qrels' queries, kept in corpus order.  The reference's train/run_gen_valid_set.py, same arguments and count line."""
import argparse
import os
import shutil
from typing import Set


def sample_docs_from_topics(qrel_path: str, run_path: str, topk: int) -> Set[str]:
    qids, sampled = set(), set()
    with open(qrel_path) as f:
        for line in f:
            qid, _, docid, _ = line.split()
            qids.add(qid)
            sampled.add(docid)
    with open(run_path) as f:
        for line in f:
            qid, _, docid, rank, _, _ = line.split()
            if int(rank) <= topk and qid in qids:
                sampled.add(docid)
    return sampled


def output_corpus(in_corpus_path: str, out_corpus_path: str, sampled_docids: Set[str]):
    cnt = 0
    with open(in_corpus_path) as src, open(out_corpus_path, "w") as out:
        for line in src:
            if line.split("\t", 1)[0] in sampled_docids:
                out.write(line)
                cnt += 1
    print(f"Write Cnt: {cnt}, Sample Cnt: {len(sampled_docids)}")


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--input_corpus_path", type=str, required=True,
                        help="corpus: one document per line, tab separated, the id first")
    parser.add_argument("--input_query_path", type=str, required=True,
                        help="queries: one per line, tab separated, the id first")
    parser.add_argument("--input_qrel_path", type=str, required=True, help="TREC qrels")
    parser.add_argument("--input_run_path", type=str, required=True, help="TREC run")
    parser.add_argument("--topk", type=int, required=True, help="documents kept per query from the run")
    parser.add_argument("--output_corpus_path", type=str, required=True)
    parser.add_argument("--output_query_path", type=str, required=True)
    parser.add_argument("--output_qrel_path", type=str, required=True)
    args = parser.parse_args(argv)
    for path in (args.output_corpus_path, args.output_query_path, args.output_qrel_path):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    shutil.copyfile(args.input_qrel_path, args.output_qrel_path)
    shutil.copyfile(args.input_query_path, args.output_query_path)
    docids = sample_docs_from_topics(args.output_qrel_path, args.input_run_path, args.topk)
    output_corpus(args.input_corpus_path, args.output_corpus_path, docids)


if __name__ == "__main__":
    main()
