#!/usr/bin/env python3
"""The L2 ADC search beside the inner-product ADC search of the same process, on the SAME PQIndex storage (development tool,
GPU): the README's ADC shape — 8 841 823 x 48 B uniform codes, D = 768, 1200-query batches, k = 1000.

    python tools/adc_l2_bench.py [--n 8841823] [--m 48] [--batches 6] [--passes 4] [--k 1000]

The index is built once; a pass searches the same query batches under METRIC_INNER_PRODUCT and then under METRIC_L2 (the metric
is an attribute the search reads: codes, image and centroids are shared), all batches enqueued before the first result is read.
Prints, per pass, ms per batch of each and their ratio; then survivors (rows past the 8-bit screen) and candidates (rows kept by
the exact rescoring) per query from `stats`, the repeated / exact-route query counts, and the table kernels alone
(rc_adc_lut_l2 against rc_adc_lut, 1200 queries).  The inner-product search is the yardstick: the two share every kernel but
the table builder and a nq x k negate."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from repconc_amd import ops  # noqa: E402
from repconc_amd.index import METRIC_INNER_PRODUCT, METRIC_L2, PQIndex  # noqa: E402

NAMES = {METRIC_INNER_PRODUCT: "ip", METRIC_L2: "l2"}


def one_pass(index, batches, k, metric):
    """-> (ms per batch, survivors per query, candidates per query, repeated queries, exact-route queries)"""
    index.metric_type = metric
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pend = []
    for qb in batches:
        stats = {}
        pend.append((index.search_async(qb, k, stats=stats), index.last_search, stats))
    for finish, _, _ in pend:
        finish()
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / len(batches)
    nq = sum(qb.shape[0] for qb in batches)
    surv = sum(int(s["survivors"].sum().item()) for _, _, s in pend if "survivors" in s) / nq
    cand = sum(int(s["candidates"].sum().item()) for _, _, s in pend) / nq
    return ms, surv, cand, sum(p.stats["retried_queries"] for _, p, _ in pend), sum(p.stats["exact_queries"] for _, p, _ in pend)


def lut_alone(C, q, metric, reps=20):
    for _ in range(3):
        ops.adc_lut(C, q, metric)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        ops.adc_lut(C, q, metric)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8841823)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--m", type=int, default=48)
    ap.add_argument("--batch", type=int, default=1200)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--k", type=int, default=1000)
    a = ap.parse_args()
    dev = "cuda:0"
    g = torch.Generator(device=dev).manual_seed(20222)
    C = torch.randn(a.m, 256, a.d // a.m, device=dev, generator=g)
    index = PQIndex(a.d, a.m)
    index.set_centroids(C)
    index.add_codes(torch.randint(0, 256, (a.n, a.m), dtype=torch.uint8, device=dev, generator=g))
    batches = [torch.randn(a.batch, a.d, device=dev, generator=g) for _ in range(a.batches)]
    print(f"adc_l2_bench: N={a.n} M={a.m} D={a.d} k={a.k} {a.batches} batches of {a.batch} queries, {a.passes} alternating passes "
          f"(uniform codes, N(0,1) centroids and queries), {torch.cuda.get_device_name(0)}", flush=True)
    for metric in (METRIC_INNER_PRODUCT, METRIC_L2):          # warm both: code objects, the retry path's operators
        one_pass(index, batches[:1], a.k, metric)
    ratios = []
    for p in range(a.passes):
        row = {}
        for metric in (METRIC_INNER_PRODUCT, METRIC_L2):
            row[metric] = one_pass(index, batches, a.k, metric)
            ms, surv, cand, rep, ex = row[metric]
            print(f"pass {p} {NAMES[metric]}: {ms:7.3f} ms per batch ({a.batch / ms:6.1f} k queries/s), survivors per query {surv:8.1f}, "
                  f"candidates per query {cand:8.1f}, repeated {rep}, exact-route {ex}", flush=True)
        ratios.append(row[METRIC_L2][0] / row[METRIC_INNER_PRODUCT][0])
        print(f"pass {p} l2 / ip time ratio: {ratios[-1]:.4f}", flush=True)
    print(f"l2 / ip time ratio over {a.passes} passes: min {min(ratios):.4f} max {max(ratios):.4f} "
          f"mean {sum(ratios) / len(ratios):.4f}", flush=True)
    t_ip, t_l2 = lut_alone(C, batches[0], METRIC_INNER_PRODUCT), lut_alone(C, batches[0], METRIC_L2)
    print(f"tables alone, {a.batch} queries: rc_adc_lut {t_ip:.4f} ms, rc_adc_lut_l2 {t_l2:.4f} ms, ratio {t_l2 / t_ip:.3f}", flush=True)


if __name__ == "__main__":
    main()
