"""The L2 index over int8 scalar-quantised flat storage (csrc/dense_search_l2_sq8.hip) beside its three neighbours, in one
process on one card, on the same vectors, at the MS MARCO passage shape: 8 841 823 x 768, the 6 980 dev queries in batches of
1 163, k = 100 and 1000, and small batches of 1 / 32 / 128 queries.  Synthetic seeded data generated on the device; the int8
stores train on the first 2^20 rows.

    python tools/dense_l2_sq8_bench.py [--out profiles/dense_l2_sq8_bench.json] [--n N] [--passes 4] [--no-ivf]

Legs: `FlatL2SQ8Index` (int8 codes, L2), `FlatSQ8Index` (the same codes, inner product), `FlatL2F16Index` (fp16, L2) and the
int8 `IVFFlatIndex` under L2 with every one of its 8 cells probed (the exact chain over every row: what answered this search
before).  Every leg is warmed up first, then the legs run in `--passes` alternating passes; a figure is the median over the
passes, every pass is printed with it, and the L2 / inner-product time ratio of the two int8 legs is given per pass.  A pass
enqueues every batch before it reads the first result, as batch_dense_search does (the IVF leg answers batch by batch).  Per
leg: ms per batch, queries/s, queries repeated / answered by the exact route; for the two int8 flat legs the rows per query
that passed the screen.  A sample of the L2 int8 answers is checked against the exact route and the IVF leg."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8841823)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nq", type=int, default=6980)
    ap.add_argument("--batch", type=int, default=1163)
    ap.add_argument("--ks", default="100,1000")
    ap.add_argument("--small", default="1,32,128")
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--verify", type=int, default=8, help="L2 int8 queries checked against the exact route and the IVF leg")
    ap.add_argument("--no-ivf", action="store_true", help="leave the all-cells IVF leg out")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatL2F16Index, FlatL2SQ8Index, FlatSQ8Index
    from repconc_amd.index import METRIC_L2
    from repconc_amd.ivf_flat import IVFFlatIndex
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    step = 1 << 20
    nlist = 8
    legs = {"l2_int8": FlatL2SQ8Index(a.d, device=dev), "ip_int8": FlatSQ8Index(a.d, device=dev),
            "l2_float16": FlatL2F16Index(a.d, device=dev)}
    for index in legs.values():
        index.reserve(a.n)
    full = None if a.no_ivf else torch.empty((a.n, a.d), dtype=torch.float32, device=dev)
    for r0 in range(0, a.n, step):
        part = torch.randn((min(step, a.n - r0), a.d), generator=g, device=dev)
        if r0 == 0:
            legs["l2_int8"].train(part)
            legs["ip_int8"].train(part)
            first = part
        for index in legs.values():
            index.add(part)
        if full is not None:
            full[r0:r0 + part.shape[0]] = part
    if full is not None:
        ivf = IVFFlatIndex(a.d, nlist, device=dev, metric=METRIC_L2, storage="int8")
        ivf.train_sq(first)
        ivf.set_coarse(first[:nlist])
        ivf.set_lists(full, torch.arange(a.n, device=dev) % nlist)
        ivf.nprobe = nlist
        assert torch.equal(ivf._dec, legs["l2_int8"]._dec)
        legs["l2_int8_ivf_all_cells"] = ivf
    del part, first, full
    torch.cuda.empty_cache()
    assert torch.equal(legs["l2_int8"].xb, legs["ip_int8"].xb)
    q = torch.randn((a.nq, a.d), generator=g, device=dev)
    nb = -(-a.nq // a.batch)
    parts = list(torch.tensor_split(q, nb))
    ks = [int(v) for v in a.ks.split(",")]
    res = {"n": a.n, "d": a.d, "nq": a.nq, "batch": a.batch, "batches": nb, "passes": a.passes,
           "corpus_gb": {name: index.xb.numel() * index.xb.element_size() / 1e9 for name, index in legs.items()}, "runs": []}

    def one_pass(index, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = ex = 0
        if isinstance(index, IVFFlatIndex):
            for part in parts:
                index.search(part, k)
                ex += index.last_search_stats["fallback_queries"]
        else:
            pend, stats = [], []
            for part in parts:
                pend.append(index.search_async(part, k))
                stats.append(index.last_search)
            for f in pend:
                f()
            rep = sum(p.stats["retried_queries"] for p in stats)
            ex = sum(p.stats["exact_queries"] for p in stats)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, rep, ex

    for k in ks:
        for index in legs.values():                                   # warm-up: one batch per leg
            index.search(parts[0], k)
        times = {name: [] for name in legs}
        extra = {name: [0, 0] for name in legs}
        for _ in range(a.passes):
            for name, index in legs.items():
                t, rep, ex = one_pass(index, k)
                times[name].append(t)
                extra[name] = [extra[name][0] + rep, extra[name][1] + ex]
        for name in legs:
            t = statistics.median(times[name])
            run = {"k": k, "leg": name, "ms_per_batch": 1e3 * t / nb, "queries_per_s": a.nq / t,
                   "ms_per_batch_passes": [1e3 * v / nb for v in times[name]],
                   "retried_queries_all_passes": extra[name][0], "exact_queries_all_passes": extra[name][1]}
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
        row = {"k": k, "l2_over_ip_int8_per_pass": [x / y for x, y in zip(times["l2_int8"], times["ip_int8"])],
               "l2_int8_over_l2_float16_per_pass": [x / y for x, y in zip(times["l2_int8"], times["l2_float16"])]}
        # the rows per query that passed each int8 screen, first pass of every batch
        for name, search in (("l2_int8", ops.dense_search_l2_sq8), ("ip_int8", ops.dense_search_sq8)):
            sq, surv = legs[name], []
            norms = {"xsq": sq._xsq[: sq.ntotal]} if name == "l2_int8" else {}
            for part in parts:
                st = {}
                search(sq.xb, sq._dec, part, k, sel_slack=sq.sel_slack, cstat=sq._cstat, stats=st, **norms)
                surv += [c.cpu().numpy() for c in st["survivors"]]
            surv = np.concatenate(surv)
            row[name + "_survivors_per_query"] = {"mean": float(surv.mean()), "median": float(np.median(surv)),
                                                  "max": int(surv.max()), "over_16384": int((surv > 16384).sum())}
        res["runs"].append(row)
        print(json.dumps(row), flush=True)
    if a.verify:
        sq = legs["l2_int8"]
        sel = torch.linspace(0, a.nq - 1, a.verify).long().to(dev)
        got = sq.search(q[sel], ks[0])
        want = ops.dense_search_l2_sq8_exact(sq.xb, sq._dec, q[sel], ks[0])
        same = torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
        if not a.no_ivf:
            other = legs["l2_int8_ivf_all_cells"].search(q[sel], ks[0])
            same = same and torch.equal(got[1], other[1]) and torch.equal(got[0].view(torch.int32), other[0].view(torch.int32))
        res["verified_queries"], res["verified_equal"] = int(a.verify), bool(same)
        print("exact-route check:", res["verified_equal"], flush=True)
    res["small"] = []
    for nq in [int(v) for v in a.small.split(",")]:
        qq = q[:nq].contiguous()
        for index in legs.values():
            for _ in range(2):
                index.search(qq, 100)
        times = {name: [] for name in legs}
        for _ in range(a.passes):
            for name, index in legs.items():
                reps = 2 if isinstance(index, IVFFlatIndex) else 10
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    index.search(qq, 100)
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0) / reps)
        row = {"nq": nq, "k": 100}
        for name in legs:
            row[name] = {"ms": statistics.median(times[name]), "ms_passes": times[name]}
        res["small"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
