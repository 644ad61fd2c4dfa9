"""`python -m repconc.train.run_extract_hardneg` (recipe step 6): hard negatives from a TREC run — per query, the run's
documents ranked <= --topk (the file's rank column) that are not qrels positives (rel > 0), in file order, written as a
JSON dict {qid: [docid, ...]}.  The reference's train/run_extract_hardneg.py, same arguments."""
import argparse
import json
import os


def extract_hardneg(run_path: str, qrel_path: str, topk: int):
    positives = {}
    with open(qrel_path) as f:
        for line in f:
            qid, _, docid, rel = line.split()
            if int(rel) > 0:
                positives.setdefault(qid, set()).add(docid)
    hardneg = {}
    with open(run_path) as f:
        for line in f:
            qid, _, docid, rank, _, _ = line.split()
            if int(rank) <= topk and docid not in positives.get(qid, ()):
                hardneg.setdefault(qid, []).append(docid)
    return hardneg


def main(argv=None):
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--run_path", type=str, required=True)
    parser.add_argument("--qrel_path", type=str, required=True)
    parser.add_argument("--topk", type=int, required=True)
    parser.add_argument("--output_path", type=str, required=True)
    args = parser.parse_args(argv)
    os.makedirs(os.path.dirname(os.path.abspath(args.output_path)), exist_ok=True)
    hardneg = extract_hardneg(args.run_path, args.qrel_path, args.topk)
    with open(args.output_path, "w") as f:
        json.dump(hardneg, f)


if __name__ == "__main__":
    main()
