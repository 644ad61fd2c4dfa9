"""Dense flat inner-product search (csrc/dense_search.hip) at the reference's scale: the MS MARCO passage corpus shape
(8 841 823 x 768 fp32, 27.2 GB), the 6 980 dev queries in batches of 1 200 (evaluate_dense.py:93-112), k = 100 / 1000, and
small query batches (1, 32, 128) against the HBM bound.  Synthetic seeded data generated on the device.

    python tools/dense_bench.py [--out profiles/dense_bench.json] [--quick] [--no-torch] [--storage float16 [--f16-only]]
                                [--screen bf16x3 [--screen-only]]
    rocprofv3 --kernel-trace --stats -d DIR -o dense -- python tools/dense_bench.py --quick
    python tools/dense_bench.py --report DIR/.../dense_kernel_stats.csv      # the screen kernel's TFLOP/s from that run

Prints ms per batch, queries/s, repeated / exact query counts, the same search as a chunked torch.mm + torch.topk
composition on the same device (ids compared where the score margins allow), and a sample of queries checked against the
fmaf-chain oracle of tests/test_dense_flat.py.  The screen's TFLOP/s and the time outside it come from the kernel trace
(--report): a screen launch over nq queries does 2 nq N D flop.

--storage float16 (csrc/dense_search_f16.hip): the fp32 leg runs first, then the same vectors rounded to fp16 in the same
process on the same card; every figure is reported for both and the result carries the float16 / float32 ratios.
--f16-only skips the fp32 leg: --report on a trace of such a --quick run gives the f16 screen's TFLOP/s against the f16
matrix peak and the shares of the sample, threshold, rescoring, select and certificate kernels.

--screen bf16x3 (csrc/dense_search_bf16x3.hip): the fp32 leg runs first, then the SAME fp32 vectors through
FlatIPIndex(screen="bf16x3") in the same process on the same card; both legs' figures, their ratios, the small-query times side
by side and the repeated / exact-route query counts.  --screen-only skips the fp32 leg (a kernel trace of the new leg alone);
--report on such a trace gives the split pre-pass, sample, screen, threshold, rescoring, select and certificate per 1 200
queries and as shares, and the screen's TFLOP/s on the 2 nq N D convention and as 3x that against the bf16 matrix peak."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TF = 157.3          # fp32 matrix peak, MI355X
PEAK_F16_TF = 2500.0     # f16 matrix peak, dense
PEAK_BF16_TF = 2500.0    # bf16 matrix peak, dense
HBM_TBS = 8.0            # HBM3E peak


def report(path, n, d, batch, nq):
    """Kernel statistics of a `--quick` run: its screen launches cover the warm-up batch and the query set twice.  The
    select and threshold kernels are shared by both storages, so per-storage shares need a trace of one leg alone: the plain
    run for fp32, `--storage float16 --f16-only` for fp16.  A trace that holds both legs is reported with "mixed_legs"."""
    queries = batch + 2 * nq
    rows = list(csv.DictReader(open(path)))
    ms = lambda r: float(r["TotalDurationNs"]) / 1e6
    # the search's own kernels (the corpus generation and host copies of the run are not part of a search)
    # rocprofv3 leaves the template kernels mangled (_Z21dense_f16_gemm_kernelILi1ELb0EE...) and demangles the plain ones: a
    # kernel is found by its name and, where variants share it, one of the two spellings of the template argument that tells
    # them apart (dense_rescore_kernel / dense_certify_kernel, csrc/dense_screen.h, serve both screened searches)
    def hit(r, kernel, *targs):
        _, found, rest = r["Name"].partition(kernel)
        return bool(found) and (not targs or any(t in rest for t in targs))
    search = [r for r in rows if any(hit(r, t) for t in ("dense_gemm_kernel", "dense_f16_", "dense_bf16x3_", "dense_rescore_kernel",
                                                         "dense_certify_kernel", "adc_threshold_kernel", "adc_select_kernel",
                                                         "adc_exact_"))]
    tot = sum(ms(r) for r in search)
    has32 = any(hit(r, "dense_gemm_kernel", "<1", "ILi1E") for r in search)
    has16 = any(hit(r, "dense_f16_gemm_kernel", "<1", "ILi1E") for r in search)
    hasb3 = any(hit(r, "dense_bf16x3_gemm_kernel", "<1", "ILi1E") for r in search)
    out = {}
    if has32 + has16 + hasb3 > 1:
        out["mixed_legs"] = True
    if hasb3:
        b3 = {}
        for r in search:
            for key, tags in (("screen", ("dense_bf16x3_gemm_kernel", "<1", "ILi1E")),
                              ("sample", ("dense_bf16x3_gemm_kernel", "<0", "ILi0E")),
                              ("split", ("dense_bf16x3_split_kernel",)), ("rescore", ("dense_rescore_kernel", "float>", "EfE")),
                              ("certify", ("dense_certify_kernel", "dense_b3_variant")), ("select", ("adc_select_kernel",)),
                              ("threshold", ("adc_threshold_kernel",))):
                if hit(r, *tags):
                    b3[key + "_ms_total"] = b3.get(key + "_ms_total", 0.0) + ms(r)
                    b3[key + "_calls"] = b3.get(key + "_calls", 0) + int(r["Calls"])
        b3["screened_queries"] = queries
        b3["screen_tflops"] = 2.0 * queries * n * d / (b3["screen_ms_total"] * 1e-3) / 1e12
        b3["screen_mfma_tflops"] = 3.0 * b3["screen_tflops"]              # three bf16 MFMAs per product
        b3["screen_mfma_share_of_bf16_peak"] = b3["screen_mfma_tflops"] / PEAK_BF16_TF
        b3["screen_ms_per_1200_queries"] = 2.0 * 1200 * n * d / (b3["screen_tflops"] * 1e12) * 1e3
        if not (has32 or has16):
            b3["search_kernels_ms_total"] = tot
            for key in ("split", "sample", "screen", "threshold", "rescore", "select", "certify"):
                b3[key + "_share"] = b3.get(key + "_ms_total", 0.0) / tot
                b3[key + "_ms_per_1200_queries"] = b3.get(key + "_ms_total", 0.0) * 1200 / queries
        out["bf16x3"] = b3
    if has32:
        r = next(r for r in search if hit(r, "dense_gemm_kernel", "<1", "ILi1E"))
        out["screen_calls"] = int(r["Calls"])
        out["screen_ms_each"] = float(r["AverageNs"]) / 1e6
        out["screen_ms_total"] = ms(r)
        if not has16:
            out["search_kernels_ms_total"] = tot
            out["outside_screen_ms_total"] = tot - out["screen_ms_total"]
            out["outside_screen_ms_per_call"] = out["outside_screen_ms_total"] / out["screen_calls"]
        out["screened_queries"] = queries
        out["screen_tflops"] = 2.0 * queries * n * d / (out["screen_ms_total"] * 1e-3) / 1e12
        out["screen_share_of_peak"] = out["screen_tflops"] / PEAK_TF
        out["screen_ms_per_1200_queries"] = 2.0 * 1200 * n * d / (out["screen_tflops"] * 1e12) * 1e3
    if has16:
        f16 = {}
        for r in search:
            for key, tags in (("screen", ("dense_f16_gemm_kernel", "<1", "ILi1E")),
                              ("sample", ("dense_f16_gemm_kernel", "<0", "ILi0E")),
                              ("rescore", ("dense_rescore_kernel", "_Float16>", "EDF16_E")),
                              ("certify", ("dense_certify_kernel", "dense_f16_variant")),
                              ("select", ("adc_select_kernel",)), ("threshold", ("adc_threshold_kernel",))):
                if hit(r, *tags):
                    f16[key + "_ms_total"] = f16.get(key + "_ms_total", 0.0) + ms(r)
                    f16[key + "_calls"] = f16.get(key + "_calls", 0) + int(r["Calls"])
        f16["screened_queries"] = queries
        f16["screen_tflops"] = 2.0 * queries * n * d / (f16["screen_ms_total"] * 1e-3) / 1e12
        f16["screen_share_of_f16_peak"] = f16["screen_tflops"] / PEAK_F16_TF
        f16["screen_ms_per_1200_queries"] = 2.0 * 1200 * n * d / (f16["screen_tflops"] * 1e12) * 1e3
        if not has32:
            f16["search_kernels_ms_total"] = tot
            for key in ("screen", "sample", "threshold", "rescore", "select", "certify"):
                f16[key + "_share"] = f16.get(key + "_ms_total", 0.0) / tot
                f16[key + "_ms_per_1200_queries"] = f16.get(key + "_ms_total", 0.0) * 1200 / queries
        out["float16"] = f16
    print(json.dumps(out, indent=1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8841823)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nq", type=int, default=6980)
    ap.add_argument("--batch", type=int, default=1200)
    ap.add_argument("--ks", default="100,1000")
    ap.add_argument("--small", default="1,32,128")
    ap.add_argument("--verify", type=int, default=16, help="queries checked against the fmaf-chain oracle")
    ap.add_argument("--quick", action="store_true", help="k = 1000, one pass over the queries, no torch leg, no small batches")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--report", default=None, help="a rocprofv3 kernel_stats.csv of a --quick run")
    ap.add_argument("--storage", default="float32", choices=["float32", "float16"],
                    help="float16: the fp32 leg first, then the fp16-storage index in the same process, and their ratios")
    ap.add_argument("--f16-only", action="store_true",
                    help="with --storage float16: skip the fp32 leg (a kernel trace of the fp16 leg alone, or an A/B of two builds)")
    ap.add_argument("--screen", default="fp32", choices=["fp32", "bf16x3"],
                    help="bf16x3: the fp32 leg first, then the same vectors through the bf16x3-screened index, and their ratios")
    ap.add_argument("--repeat", type=int, default=3, help="with --screen bf16x3: further alternating passes of both legs (the spread)")
    ap.add_argument("--screen-only", action="store_true", help="with --screen bf16x3: skip the fp32 leg (a kernel trace of the new leg alone)")
    a = ap.parse_args()
    if a.screen == "bf16x3" and a.storage != "float32":
        ap.error("--screen bf16x3 needs --storage float32")
    if a.report:
        report(a.report, a.n, a.d, a.batch, a.nq)
        return
    import torch
    from repconc_amd import _lib
    from repconc_amd.dense_index import FlatIPIndex
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    step = 1 << 20
    q = None
    res = None
    if not ((a.storage == "float16" and a.f16_only) or (a.screen == "bf16x3" and a.screen_only)):
        index = FlatIPIndex(a.d, device=dev)
        index.reserve(a.n)
        for r0 in range(0, a.n, step):
            index.add(torch.randn((min(step, a.n - r0), a.d), generator=g, device=dev))
        q = torch.randn((a.nq, a.d), generator=g, device=dev)
        res = measure(a, index, q)
    if a.storage == "float16":
        half = FlatIPIndex(a.d, device=dev, storage="float16")
        half.reserve(a.n)
        if res is None:                                  # the same random stream as the fp32 leg draws
            for r0 in range(0, a.n, step):
                half.add(torch.randn((min(step, a.n - r0), a.d), generator=g, device=dev))
            q = torch.randn((a.nq, a.d), generator=g, device=dev)
        else:
            for r0 in range(0, a.n, step):
                half.add(index.xb[r0:r0 + step])
            del index
        torch.cuda.empty_cache()
        r16 = measure(a, half, q)
        r16["screen_form"] = "v_mfma_f32_%s_f16" % {32: "32x32x16", 16: "16x16x32"}[_lib.load().rc_dense_f16_screen_form()]
        if res is None:
            res = {"float16": r16}
        else:
            f32 = res
            res = {"float32": f32, "float16": r16, "float16_over_float32_queries_per_s": {
                str(u["k"]): v["queries_per_s"] / u["queries_per_s"] for u, v in zip(f32["runs"], r16["runs"])}}
            if "small" in r16:
                res["float16_over_float32_small_ms"] = {str(u["nq"]): v["ms"] / u["ms"] for u, v in zip(f32["small"], r16["small"])}
            print(json.dumps({k: v for k, v in res.items() if k.startswith("float16_over")}), flush=True)
    if a.screen == "bf16x3":
        b3 = FlatIPIndex(a.d, device=dev, screen="bf16x3")
        if res is None:                                  # the same random stream as the fp32 leg draws
            b3.reserve(a.n)
            for r0 in range(0, a.n, step):
                b3.add(torch.randn((min(step, a.n - r0), a.d), generator=g, device=dev))
            q = torch.randn((a.nq, a.d), generator=g, device=dev)
        else:                                            # the fp32 leg's vectors through add (its range check and norm)
            b3.reserve(a.n)
            for r0 in range(0, a.n, step):
                b3.add(index.xb[r0:r0 + step])
        rb3 = measure(a, b3, q)
        if res is None:
            res = {"bf16x3": rb3}
        else:
            f32 = res
            res = {"float32": f32, "bf16x3": rb3, "bf16x3_over_float32_queries_per_s": {
                str(u["k"]): v["queries_per_s"] / u["queries_per_s"] for u, v in zip(f32["runs"], rb3["runs"])}}
            if "small" in rb3:
                res["bf16x3_over_float32_small_ms"] = {str(u["nq"]): v["ms"] / u["ms"] for u, v in zip(f32["small"], rb3["small"])}
                res["small_ms_side_by_side"] = [{"nq": u["nq"], "float32_ms": u["ms"], "bf16x3_ms": v["ms"]}
                                                for u, v in zip(f32["small"], rb3["small"])]
            # the spread: both legs again, alternating, in this process; every ratio is of two neighbouring legs
            reps = [{"float32": measure(a, index, q, light=True)["runs"], "bf16x3": measure(a, b3, q, light=True)["runs"]}
                    for _ in range(a.repeat)]
            res["repeats"] = reps
            for j, u in enumerate(f32["runs"]):
                qps32 = [u["queries_per_s"]] + [r["float32"][j]["queries_per_s"] for r in reps]
                qpsb3 = [rb3["runs"][j]["queries_per_s"]] + [r["bf16x3"][j]["queries_per_s"] for r in reps]
                ratios = [y / x for x, y in zip(qps32, qpsb3)]
                res.setdefault("spread", {})[str(u["k"])] = {
                    "float32_queries_per_s": qps32, "bf16x3_queries_per_s": qpsb3, "ratios": ratios,
                    "float32_rel_range": (max(qps32) - min(qps32)) / min(qps32),
                    "bf16x3_rel_range": (max(qpsb3) - min(qpsb3)) / min(qpsb3),
                    "ratio_min": min(ratios), "ratio_max": max(ratios)}
            print(json.dumps({k: v for k, v in res.items() if k.startswith("bf16x3_over") or k.startswith("small_ms") or k == "spread"}), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


def measure(a, index, q, light=False):
    """Every figure of one index (fp32 or fp16 storage, fp32 or bf16x3 screen) over the query set `q`.
    light: only the timed batches of every k (a repeat of a leg, for the run-to-run spread)."""
    import numpy as np
    import torch
    from repconc_amd import ops
    from repconc_amd.models.dense.evaluate_dense import batch_dense_search
    f16 = index.storage == "float16"
    b3 = getattr(index, "screen", "fp32") == "bf16x3"
    esize = 2 if f16 else 4
    peak = PEAK_F16_TF if f16 else PEAK_BF16_TF / 3.0 if b3 else PEAK_TF
    search = (lambda qq, k: ops.dense_search_f16(index.xb, qq, k, xnorm_max=index._xnorm_max)) if f16 else \
        (lambda qq, k: ops.dense_search_bf16x3(index.xb, qq, k, xnorm_max=index._xnorm_max)) if b3 else \
        (lambda qq, k: ops.dense_search(index.xb, qq, k))
    qn = q.cpu().numpy()
    corpus_ids = np.arange(a.n)
    query_ids = np.arange(a.nq)
    ks = [1000] if a.quick else [int(v) for v in a.ks.split(",")]
    res = {"storage": index.storage, "screen": "bf16x3" if b3 else "fp32", "n": a.n, "d": a.d, "nq": a.nq, "batch": a.batch, "corpus_gb": a.n * a.d * esize / 1e9,
           "flop_per_batch_t": 2.0 * a.batch * a.n * a.d / 1e12, "roofline_ms_per_batch": 2.0 * a.batch * a.n * a.d / peak / 1e9,
           "hbm_bound_ms": a.n * a.d * esize / HBM_TBS / 1e9, "runs": []}
    nb = -(-a.nq // a.batch)
    for k in ks:
        batch_dense_search(query_ids[:a.batch], qn[:a.batch], corpus_ids, index, k, a.batch)      # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pend, pstats = [], []
        for part in np.array_split(qn, nb):
            pend.append(index.search_async(part, k))
            pstats.append(index.last_search)
        outs = [f() for f in pend]
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        ids = np.concatenate([o[1] for o in outs])
        sc = np.concatenate([o[0] for o in outs])
        run = {"k": k, "batches": nb, "s_total": t, "ms_per_batch": 1e3 * t / nb, "queries_per_s": a.nq / t,
               "retried_queries": sum(p.stats["retried_queries"] for p in pstats),
               "exact_queries": sum(p.stats["exact_queries"] for p in pstats)}
        if light:
            res["runs"].append(run)
            continue
        # the public path end to end (host numpy in / out, every batch enqueued first)
        t0 = time.perf_counter()
        bs, bi = batch_dense_search(query_ids, qn, corpus_ids, index, k, a.batch)
        run["batch_dense_search_s"] = time.perf_counter() - t0
        assert np.array_equal(bi, ids)
        if not (a.quick or a.no_torch or f16 or b3):
            # chunked torch.mm + torch.topk on the same device
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tops, topi = [], []
            x = index.xb
            for part in torch.split(q, a.batch):
                best_s, best_i = None, None
                for r0 in range(0, a.n, 1 << 21):
                    s = torch.mm(part, x[r0:r0 + (1 << 21)].T)
                    v, i = torch.topk(s, k, dim=1)
                    i += r0
                    if best_s is not None:
                        v, j = torch.topk(torch.cat([best_s, v], 1), k, dim=1)
                        i = torch.gather(torch.cat([best_i, i], 1), 1, j)
                    best_s, best_i = v, i
                tops.append(best_s)
                topi.append(best_i)
            ts, ti = torch.cat(tops).cpu().numpy(), torch.cat(topi).cpu().numpy()
            torch.cuda.synchronize()
            run["torch_mm_topk_s"] = time.perf_counter() - t0
            run["speedup_vs_torch"] = run["torch_mm_topk_s"] / run["batch_dense_search_s"]
            # ids compared at the ranks whose score differs from both neighbours by more than a chain error bound
            margin = 4 * a.d * 2.0 ** -24 * np.abs(sc).max()
            gap = np.minimum(np.abs(np.diff(sc, axis=1, prepend=np.inf)), np.abs(np.diff(sc, axis=1, append=-np.inf)))
            sure = gap > margin
            run["torch_ids_compared"] = int(sure.sum())
            run["torch_ids_equal"] = int((ti[sure] == ids[sure]).sum())
        res["runs"].append(run)
        print(json.dumps(run), flush=True)
    if light:
        return res
    if a.verify:
        from test_dense_flat import oracle_topk
        k = ks[-1]
        sel = np.linspace(0, a.nq - 1, a.verify).astype(int)
        # (fp16 storage: the oracle over the stored values widened and the rounded queries, rows widened block by block)
        ws, wi = oracle_topk(index.xb, q[sel].half().float() if f16 else q[sel], k, qblock=16, rblock=1 << 20)
        gs, gi = index.search(qn[sel], k)
        res["verified_queries"] = int(len(sel))
        res["verified_equal"] = bool(np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32)))
        print("oracle check:", res["verified_equal"], flush=True)
    if not a.quick:
        res["small"] = []
        for nq in [int(v) for v in a.small.split(",")]:
            qq = q[:nq].contiguous()
            for _ in range(2):
                search(qq, 100)
            torch.cuda.synchronize()
            reps = 10
            t0 = time.perf_counter()
            for _ in range(reps):
                search(qq, 100)
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / reps
            row = {"nq": nq, "k": 100, "ms": ms, "hbm_bound_ms": res["hbm_bound_ms"],
                   "corpus_read_tbs": a.n * a.d * esize / (ms * 1e-3) / 1e12,
                   "roofline_ms": max(res["hbm_bound_ms"], 2.0 * nq * a.n * a.d / peak / 1e9)}
            res["small"].append(row)
            print(json.dumps(row), flush=True)
    return res


if __name__ == "__main__":
    main()
