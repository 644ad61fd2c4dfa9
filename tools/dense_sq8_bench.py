"""The int8 scalar-quantised flat index (csrc/dense_search_sq8.hip) beside the fp16 and fp32 inner-product indexes, in one
process on one card, at the MS MARCO passage shape: 8 841 823 x 768, the 6 980 dev queries in batches of 1 163, k = 100 and
1000, and small batches of 1 / 32 / 128 queries.  Synthetic seeded data generated on the device; the int8 index trains on the
first 2^20 rows.

    python tools/dense_sq8_bench.py [--out profiles/dense_sq8_bench.json] [--n N] [--passes 4]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o sq8 -- python tools/dense_sq8_bench.py --trace-leg
    python tools/dense_sq8_bench.py --report DIR        # the screen launch alone against its two bounds

Every leg is warmed up first (one batch per k, which also loads the code objects and the retry path's operators), then the
legs run in `--passes` alternating passes (fp32, fp16, int8, fp32, ...): a figure is the median over the passes, the spread
is printed with it.  A pass enqueues every batch before it reads the first result, as batch_dense_search does.  Per leg:
ms per batch, queries/s, queries repeated / answered by the exact route; for the int8 leg the rows per query that passed
the screen.  A sample of the int8 answers is checked against the fmaf-chain oracle over the decoded rows."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_ACHIEVABLE_TBS = 6.3     # a streaming read on the MI355X (8.0 TB/s spec)
PEAK_I8_TOPS = 5000.0        # int8 matrix peak, dense: twice the f16 / bf16 rate


def report(d, n, dim, queries_per_call):
    """The FILTER launch of the int8 screen from a kernel trace of `--trace-leg`, against the time to read the corpus once at
    the achievable HBM rate and the time of its matrix work (two limbs: 2 x 2 nq N D operations) at the int8 peak."""
    path = [p for p in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)]
    rows = list(csv.DictReader(open(path[0])))
    out = {}
    for r in rows:
        name = r["Name"]
        for key, tag in (("screen", "dense_i8_gemm_kernelILi1E"), ("screen", "dense_i8_gemm_kernel<1"),
                         ("sample", "dense_i8_gemm_kernelILi0E"), ("sample", "dense_i8_gemm_kernel<0"),
                         ("prepass", "dense_i8_prepass_kernel"), ("rescore", "dense_sq8_rescore_kernel"),
                         ("certify", "dense_sq8_certify_kernel"), ("select", "adc_select_kernel"),
                         ("threshold", "adc_threshold_kernel")):
            if tag in name:
                out.setdefault(key, {"calls": 0, "ms_total": 0.0})
                out[key]["calls"] += int(r["Calls"])
                out[key]["ms_total"] += float(r["TotalDurationNs"]) / 1e6
                break
    for v in out.values():
        v["ms_each"] = v["ms_total"] / v["calls"]
    s = out["screen"]
    s["queries_per_call"] = queries_per_call
    s["hbm_bound_ms"] = n * dim / HBM_ACHIEVABLE_TBS / 1e9
    s["matrix_bound_ms"] = 2 * 2.0 * queries_per_call * n * dim / PEAK_I8_TOPS / 1e9
    s["over_hbm_bound"] = s["ms_each"] / s["hbm_bound_ms"]
    s["over_matrix_bound"] = s["ms_each"] / s["matrix_bound_ms"]
    s["limb_tops"] = 2 * 2.0 * queries_per_call * n * dim / (s["ms_each"] * 1e-3) / 1e12
    print(json.dumps(out, indent=1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8841823)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nq", type=int, default=6980)
    ap.add_argument("--batch", type=int, default=1163)
    ap.add_argument("--ks", default="100,1000")
    ap.add_argument("--small", default="1,32,128")
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--verify", type=int, default=8, help="int8 queries checked against the fmaf-chain oracle")
    ap.add_argument("--trace-leg", action="store_true", help="the int8 leg alone, k = 100, one warm-up and one pass: for a kernel trace")
    ap.add_argument("--report", default=None, help="the output directory of a rocprofv3 --kernel-trace --stats run of --trace-leg")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.report:
        report(a.report, a.n, a.d, a.batch)
        return
    import numpy as np
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatIPIndex, FlatSQ8Index
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    step = 1 << 20
    legs = {"int8": FlatSQ8Index(a.d, device=dev)}
    if not a.trace_leg:
        legs = {"float32": FlatIPIndex(a.d, device=dev), "float16": FlatIPIndex(a.d, device=dev, storage="float16"), **legs}
    for index in legs.values():
        index.reserve(a.n)
    for r0 in range(0, a.n, step):
        part = torch.randn((min(step, a.n - r0), a.d), generator=g, device=dev)
        if r0 == 0:
            legs["int8"].train(part)
        for index in legs.values():
            index.add(part)
    del part
    q = torch.randn((a.nq, a.d), generator=g, device=dev)
    nb = -(-a.nq // a.batch)
    parts = list(torch.tensor_split(q, nb))
    ks = [100] if a.trace_leg else [int(v) for v in a.ks.split(",")]
    res = {"n": a.n, "d": a.d, "nq": a.nq, "batch": a.batch, "batches": nb, "passes": a.passes,
           "corpus_gb": {name: index.xb.numel() * index.xb.element_size() / 1e9 for name, index in legs.items()}, "runs": []}

    def one_pass(index, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pend, stats = [], []
        for part in parts:
            pend.append(index.search_async(part, k))
            stats.append(index.last_search)
        outs = [f() for f in pend]
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        return t, sum(p.stats["retried_queries"] for p in stats), sum(p.stats["exact_queries"] for p in stats), outs

    for k in ks:
        for index in legs.values():                                   # warm-up: one batch per leg
            index.search(parts[0], k)
        times = {name: [] for name in legs}
        extra = {name: [0, 0] for name in legs}
        for _ in range(1 if a.trace_leg else a.passes):
            for name, index in legs.items():
                t, rep, ex, _ = one_pass(index, k)
                times[name].append(t)
                extra[name] = [extra[name][0] + rep, extra[name][1] + ex]
        for name in legs:
            t = statistics.median(times[name])
            run = {"k": k, "storage": name, "ms_per_batch": 1e3 * t / nb, "queries_per_s": a.nq / t,
                   "ms_per_batch_passes": [1e3 * v / nb for v in times[name]],
                   "retried_queries_all_passes": extra[name][0], "exact_queries_all_passes": extra[name][1]}
            res["runs"].append(run)
            print(json.dumps(run), flush=True)
        # the rows per query that passed the int8 screen, first pass of every batch
        sq = legs["int8"]
        surv = []
        for part in parts:
            st = {}
            ops.dense_search_sq8(sq.xb, sq._dec, part, k, sel_slack=sq.sel_slack, cstat=sq._cstat, stats=st)
            surv += [c.cpu().numpy() for c in st["survivors"]]
        surv = np.concatenate(surv)
        row = {"k": k, "int8_survivors_per_query": {"mean": float(surv.mean()), "median": float(np.median(surv)),
                                                    "max": int(surv.max()), "over_16384": int((surv > 16384).sum())}}
        res["runs"].append(row)
        print(json.dumps(row), flush=True)
    if a.trace_leg:
        return
    if a.verify:
        from test_dense_flat import oracle_topk
        sq = legs["int8"]
        sel = torch.linspace(0, a.nq - 1, a.verify).long().to(dev)
        got = sq.search(q[sel], ks[0])
        ws, wi = oracle_topk(sq.reconstruct_n(0, a.n), q[sel], ks[0], qblock=8, rblock=1 << 20)
        res["verified_queries"] = int(a.verify)
        res["verified_equal"] = bool(np.array_equal(got[1].cpu().numpy(), wi) and
                                     np.array_equal(got[0].cpu().numpy().view(np.uint32), ws.view(np.uint32)))
        print("oracle check:", res["verified_equal"], flush=True)
        torch.cuda.empty_cache()
    res["small"] = []
    for nq in [int(v) for v in a.small.split(",")]:
        qq = q[:nq].contiguous()
        for index in legs.values():
            for _ in range(2):
                index.search(qq, 100)
        times = {name: [] for name in legs}
        for _ in range(a.passes):
            for name, index in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    index.search(qq, 100)
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0) / 10)
        row = {"nq": nq, "k": 100}
        for name, index in legs.items():
            byts = index.xb.numel() * index.xb.element_size()
            row[name] = {"ms": statistics.median(times[name]), "ms_passes": times[name],
                         "hbm_bound_ms": byts / HBM_ACHIEVABLE_TBS / 1e9,
                         "corpus_read_tbs": byts / (statistics.median(times[name]) * 1e-3) / 1e12}
        res["small"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
