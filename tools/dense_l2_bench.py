"""Dense flat L2 search (csrc/dense_search_l2.hip, FlatL2Index) beside the inner-product search of the same process on the
same card, at the reference's scale: 8 841 823 x 768 fp32 synthetic seeded N(0, 1) vectors, 6 980 queries in 6 batches,
k = 100 and 1000.

    python tools/dense_l2_bench.py [--out profiles/dense_l2_bench.json] [--passes 4] [--quick] [--exact-only]
    rocprofv3 --kernel-trace --stats -d DIR -o dense_l2 -- python tools/dense_l2_bench.py --quick --l2-only

Prints one JSON line per figure: ms per batch and queries/s of both indexes over alternating passes, the L2 / IP time ratio
of every pass and its spread, the repeated / exact-route query counts, a sample of queries checked against the chain oracle
of tests/test_dense_l2.py, the same work as a chunked expanded torch.mm + torch.topk composition (ids compared where the
distance margin exceeds the chain's bound), the exact-route kernel alone at 1 200 x 131 072 x 768 against its vector-ALU
issue bound, and 1 / 32 / 128 queries at k = 100 beside the inner-product times.  --quick: one pass at k = 1000, no torch
leg, no small query sets.

    python tools/dense_l2_bench.py --storage float16 [--out profiles/dense_l2_f16_bench.json] [--quick] [--l2-only]

--storage float16: the fp16 L2 index (csrc/dense_search_l2_f16.hip, FlatL2F16Index) beside the fp32 L2 index and the fp16
inner-product index of the same process, the same alternating passes and small query sets, the fp16 L2 / fp32 L2 and fp16 L2 /
fp16 IP time ratios of every pass, a sample of queries checked against the chain oracle on the widened values.

    python tools/dense_l2_bench.py --screen bf16x3 [--out profiles/dense_l2_bf16x3_bench.json] [--quick] [--l2-only]

--screen bf16x3: the fp32 L2 index with the bf16x3 screen (csrc/dense_search_l2_bf16x3.hip, FlatL2Bf16x3Index) beside the fp32
L2 index and the bf16x3 inner-product index over the same fp32 tensor, the same alternating passes and small query sets, the
time ratios of every pass, a sample of queries checked against the chain oracle."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# vector-ALU issue bound of the exact-route kernel: 2 lane-operations (one subtraction, one fmaf) per (q, n, d); a wave64
# instruction issues in 2 cycles on a 32-lane SIMD, 4 SIMDs x 256 CUs, at the 2.4 GHz peak clock
VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def timed_batches(index, qn, k, nb):
    import numpy as np
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pend, stats = [], []
    for part in np.array_split(qn, nb):
        pend.append(index.search_async(part, k))
        stats.append(index.last_search)
    outs = [f() for f in pend]
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    return t, np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs]), \
        sum(p.stats["retried_queries"] for p in stats), sum(p.stats["exact_queries"] for p in stats)


def torch_l2_topk(x, xsq, q, k, batch):
    """The expanded form as a framework composition: ||x||^2 - 2 q.x by chunked mm, topk of the smallest, merged."""
    import torch
    tops, topi = [], []
    for part in torch.split(q, batch):
        best_s, best_i = None, None
        for r0 in range(0, x.shape[0], 1 << 21):
            s = torch.addmm(xsq[r0:r0 + (1 << 21)][None], part, x[r0:r0 + (1 << 21)].T, alpha=-2.0)
            v, i = torch.topk(s, k, dim=1, largest=False)
            i += r0
            if best_s is not None:
                v, j = torch.topk(torch.cat([best_s, v], 1), k, dim=1, largest=False)
                i = torch.gather(torch.cat([best_i, i], 1), 1, j)
            best_s, best_i = v, i
        tops.append(best_s + (part * part).sum(1, keepdim=True))
        topi.append(best_i)
    return torch.cat(tops).cpu().numpy(), torch.cat(topi).cpu().numpy()


def exact_kernel_alone(x, q, say):
    """The exact route at 1 200 x 131 072 x 768.  The kernel's own time comes from the framework's profiler when it can trace
    device kernels; the wall time of the whole exact search (kernel + radix select) is reported beside it either way."""
    import torch
    from repconc_amd import ops
    nq, (N, D) = q.shape[0], x.shape
    for _ in range(2):
        ops.dense_search_l2_exact(x, q, 100)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        ops.dense_search_l2_exact(x, q, 100)
    torch.cuda.synchronize()
    row = {"exact_route": True, "nq": nq, "n": N, "d": D, "whole_search_ms": 1e3 * (time.perf_counter() - t0) / reps,
           "valu_issue_bound_ms": 1e3 * 2.0 * nq * N * D / VALU_LANE_OPS_PER_S}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            ops.dense_search_l2_exact(x, q, 100)
            torch.cuda.synchronize()
        us = sum(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total
                 for e in prof.key_averages() if "dense_l2_exact_kernel" in e.key)
        if us > 0:
            row["kernel_ms"] = us / 1e3
            row["kernel_fraction_of_valu_issue_bound"] = row["valu_issue_bound_ms"] / row["kernel_ms"]
    except Exception as e:                                   # no device tracing in this build: the kernel alone stays unmeasured
        row["kernel_ms_unmeasured"] = repr(e)[:200]
    say(row)
    return row


def storage_f16(a, say, res):
    """--storage float16: the fp16 L2 index beside the fp32 L2 index (the same vectors before rounding) and the fp16
    inner-product index (the same fp16 tensor) of this process, alternating passes; then 1 / 32 / 128 queries at k = 100."""
    import numpy as np
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatIPIndex, FlatL2F16Index, FlatL2Index
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    h = FlatL2F16Index(a.d, device=dev)
    h.reserve(a.n)
    l2 = None if a.l2_only else FlatL2Index(a.d, device=dev)
    if l2 is not None:
        l2.reserve(a.n)
    for r0 in range(0, a.n, 1 << 20):
        part = torch.randn((min(1 << 20, a.n - r0), a.d), generator=g, device=dev)
        h.add(part)
        if l2 is not None:
            l2.add(part)
    q = torch.randn((a.nq, a.d), generator=g, device=dev)
    ip = None
    if not a.l2_only:
        ip = FlatIPIndex(a.d, device=dev, storage="float16")
        ip._x, ip.ntotal, ip._xnorm_max = h._x, h.ntotal, h._xnorm_max      # the same fp16 vectors (measurement only)
    legs = [("l2_f16", h), ("l2_f32", l2), ("ip_f16", ip)]
    legs = [(n, ix) for n, ix in legs if ix is not None]
    qn = q.cpu().numpy()
    nb = -(-a.nq // a.batch)
    ks = [1000] if a.quick else [int(v) for v in a.ks.split(",")]
    passes = 1 if a.quick else a.passes
    last = {}
    for k in ks:
        for _, index in legs:
            index.search(qn[:a.batch], k)                    # warm-up
        rows = []
        for p in range(passes):
            row = {"k": k, "pass": p, "batches": nb}
            for name, index in legs:
                t, sc, ids, retried, exact = timed_batches(index, qn, k, nb)
                row.update({f"{name}_ms_per_batch": 1e3 * t / nb, f"{name}_queries_per_s": a.nq / t,
                            f"{name}_retried_queries": retried, f"{name}_exact_queries": exact})
                if name == "l2_f16":
                    last[k] = (sc, ids)
            if len(legs) == 3:
                row["l2_f16_over_l2_f32_time"] = row["l2_f16_ms_per_batch"] / row["l2_f32_ms_per_batch"]
                row["l2_f16_over_ip_f16_time"] = row["l2_f16_ms_per_batch"] / row["ip_f16_ms_per_batch"]
            rows.append(row)
            say(row)
        summary = {"k": k}
        for name, _ in legs:
            summary[f"{name}_ms_per_batch_median"] = float(np.median([r[f"{name}_ms_per_batch"] for r in rows]))
            summary[f"{name}_queries_per_s_median"] = float(np.median([r[f"{name}_queries_per_s"] for r in rows]))
            summary[f"{name}_retried_queries"] = sum(r[f"{name}_retried_queries"] for r in rows)
            summary[f"{name}_exact_queries"] = sum(r[f"{name}_exact_queries"] for r in rows)
        for key in ("l2_f16_over_l2_f32_time", "l2_f16_over_ip_f16_time"):
            if key in rows[0]:
                v = [r[key] for r in rows]
                summary.update({key + "_median": float(np.median(v)), key + "_min": min(v), key + "_max": max(v)})
        say(summary)
        res["runs"].append({"passes": rows, "summary": summary})
    if a.verify:
        from test_dense_l2 import oracle_topk_l2
        k = ks[-1]
        sel = np.linspace(0, a.nq - 1, a.verify).astype(int)
        ws, wi = oracle_topk_l2(h.xb, q[sel].half().float(), k, qblock=16, rblock=1 << 20)    # the oracle widens block by block
        gs, gi = last[k][0][sel], last[k][1][sel]
        res["verified_queries"] = int(len(sel))
        res["verified_equal"] = bool(np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32)))
        say({"oracle_check_queries": int(len(sel)), "equal": res["verified_equal"]})
    if not a.quick:
        res["small"] = []
        for nq in [int(v) for v in a.small.split(",")]:
            qq = q[:nq].contiguous()
            row = {"nq": nq, "k": 100}
            fns = {"l2_f16": lambda: ops.dense_search_l2_f16(h.xb, qq, 100, xsq=h._xsq[: h.ntotal], xnorm_max=h._xnorm_max)}
            if l2 is not None:
                fns["l2_f32"] = lambda: ops.dense_search_l2(l2.xb, qq, 100, xsq=l2._xsq[: l2.ntotal], xnorm_max=l2._xnorm_max)
                fns["ip_f16"] = lambda: ops.dense_search_f16(h.xb, qq, 100, xnorm_max=h._xnorm_max)
            for name, fn in fns.items():
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
                row[name + "_ms"] = 1e3 * (time.perf_counter() - t0) / 10
            res["small"].append(row)
            say(row)


def screen_bf16x3(a, say, res):
    """--screen bf16x3: the bf16x3 L2 index beside the fp32 L2 index and the bf16x3 inner-product index, all three over the one
    fp32 tensor (and, for the two L2 indexes, the one tensor of squared norms), alternating passes; then 1 / 32 / 128 queries at
    k = 100."""
    import numpy as np
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatIPIndex, FlatL2Bf16x3Index, FlatL2Index
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    b3 = FlatL2Bf16x3Index(a.d, device=dev)
    b3.reserve(a.n)
    for r0 in range(0, a.n, 1 << 20):
        b3.add(torch.randn((min(1 << 20, a.n - r0), a.d), generator=g, device=dev))
    q = torch.randn((a.nq, a.d), generator=g, device=dev)
    l2 = ip = None
    if not a.l2_only:                                        # the same vectors and norms, not a second copy (measurement only)
        l2 = FlatL2Index(a.d, device=dev)
        l2._x, l2._xsq, l2.ntotal, l2._xnorm_max = b3._x, b3._xsq, b3.ntotal, b3._xnorm_max
        ip = FlatIPIndex(a.d, device=dev, screen="bf16x3")
        ip._x, ip.ntotal, ip._xnorm_max = b3._x, b3.ntotal, b3._xnorm_max
    legs = [(n, ix) for n, ix in (("l2_bf16x3", b3), ("l2_f32", l2), ("ip_bf16x3", ip)) if ix is not None]
    qn = q.cpu().numpy()
    nb = -(-a.nq // a.batch)
    ks = [1000] if a.quick else [int(v) for v in a.ks.split(",")]
    passes = 1 if a.quick else a.passes
    last = {}
    for k in ks:
        for _, index in legs:
            index.search(qn[:a.batch], k)                    # warm-up
        rows = []
        for p in range(passes):
            row = {"k": k, "pass": p, "batches": nb}
            for name, index in legs:
                t, sc, ids, retried, exact = timed_batches(index, qn, k, nb)
                row.update({f"{name}_ms_per_batch": 1e3 * t / nb, f"{name}_queries_per_s": a.nq / t,
                            f"{name}_retried_queries": retried, f"{name}_exact_queries": exact})
                if name == "l2_bf16x3":
                    last[k] = (sc, ids)
            if len(legs) == 3:
                row["l2_f32_over_l2_bf16x3_time"] = row["l2_f32_ms_per_batch"] / row["l2_bf16x3_ms_per_batch"]
                row["l2_bf16x3_over_ip_bf16x3_time"] = row["l2_bf16x3_ms_per_batch"] / row["ip_bf16x3_ms_per_batch"]
            rows.append(row)
            say(row)
        summary = {"k": k}
        for name, _ in legs:
            summary[f"{name}_ms_per_batch_median"] = float(np.median([r[f"{name}_ms_per_batch"] for r in rows]))
            summary[f"{name}_queries_per_s_median"] = float(np.median([r[f"{name}_queries_per_s"] for r in rows]))
            summary[f"{name}_retried_queries"] = sum(r[f"{name}_retried_queries"] for r in rows)
            summary[f"{name}_exact_queries"] = sum(r[f"{name}_exact_queries"] for r in rows)
        for key in ("l2_f32_over_l2_bf16x3_time", "l2_bf16x3_over_ip_bf16x3_time"):
            if key in rows[0]:
                v = [r[key] for r in rows]
                summary.update({key + "_median": float(np.median(v)), key + "_min": min(v), key + "_max": max(v)})
        say(summary)
        res["runs"].append({"passes": rows, "summary": summary})
    if a.verify:
        from test_dense_l2 import oracle_topk_l2
        k = ks[-1]
        sel = np.linspace(0, a.nq - 1, a.verify).astype(int)
        ws, wi = oracle_topk_l2(b3.xb, q[sel], k, qblock=16, rblock=1 << 20)
        gs, gi = last[k][0][sel], last[k][1][sel]
        res["verified_queries"] = int(len(sel))
        res["verified_equal"] = bool(np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32)))
        say({"oracle_check_queries": int(len(sel)), "equal": res["verified_equal"]})
    if not a.quick:
        res["small"] = []
        xsq = b3._xsq[: b3.ntotal]
        for nq in [int(v) for v in a.small.split(",")]:
            qq = q[:nq].contiguous()
            row = {"nq": nq, "k": 100}
            fns = {"l2_bf16x3": lambda: ops.dense_search_l2_bf16x3(b3.xb, qq, 100, xsq=xsq, xnorm_max=b3._xnorm_max)}
            if l2 is not None:
                fns["l2_f32"] = lambda: ops.dense_search_l2(b3.xb, qq, 100, xsq=xsq, xnorm_max=b3._xnorm_max)
                fns["ip_bf16x3"] = lambda: ops.dense_search_bf16x3(b3.xb, qq, 100, xnorm_max=b3._xnorm_max)
            for name, fn in fns.items():
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
                row[name + "_ms"] = 1e3 * (time.perf_counter() - t0) / 10
            res["small"].append(row)
            say(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--screen", default="fp32", choices=["fp32", "bf16x3"],
                    help="bf16x3: the bf16x3 L2 index beside the fp32 L2 index and the bf16x3 inner-product index (fp32 storage)")
    ap.add_argument("--storage", default="float32", choices=["float32", "float16"],
                    help="float16: the fp16 L2 index beside the fp32 L2 index and the fp16 inner-product index")
    ap.add_argument("--n", type=int, default=8841823)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nq", type=int, default=6980)
    ap.add_argument("--batch", type=int, default=1200)
    ap.add_argument("--ks", default="100,1000")
    ap.add_argument("--small", default="1,32,128")
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--verify", type=int, default=16, help="queries checked against the chain oracle")
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--l2-only", action="store_true", help="skip the inner-product legs (a kernel trace of the L2 search alone)")
    ap.add_argument("--exact-only", action="store_true", help="only the exact-route kernel at 1 200 x 131 072 x d")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatIPIndex, FlatL2Index
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    res = {"n": a.n, "d": a.d, "nq": a.nq, "batch": a.batch, "passes": a.passes, "runs": []}

    def say(row):
        print(json.dumps(row), flush=True)

    if a.screen == "bf16x3" and a.storage != "float32":
        ap.error("--screen bf16x3 needs --storage float32")
    if a.storage == "float16" or a.screen == "bf16x3":
        if a.screen == "bf16x3":
            res["screen"] = "bf16x3"
            screen_bf16x3(a, say, res)
        else:
            res["storage"] = "float16"
            storage_f16(a, say, res)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, "w"), indent=1)
        return
    if a.exact_only:
        x = torch.randn((131072, a.d), generator=g, device=dev)
        res["exact_kernel"] = exact_kernel_alone(x, torch.randn((1200, a.d), generator=g, device=dev), say)
        return
    l2 = FlatL2Index(a.d, device=dev)
    l2.reserve(a.n)
    for r0 in range(0, a.n, 1 << 20):
        l2.add(torch.randn((min(1 << 20, a.n - r0), a.d), generator=g, device=dev))
    q = torch.randn((a.nq, a.d), generator=g, device=dev)
    ip = None
    if not a.l2_only:
        ip = FlatIPIndex(a.d, device=dev)
        ip._x, ip.ntotal = l2._x, l2.ntotal                  # the same vectors, not a second copy (measurement only)
    qn = q.cpu().numpy()
    nb = -(-a.nq // a.batch)
    ks = [1000] if a.quick else [int(v) for v in a.ks.split(",")]
    passes = 1 if a.quick else a.passes
    last = {}
    for k in ks:
        for index in (l2, ip):
            if index is not None:
                index.search(qn[:a.batch], k)                # warm-up
        rows = []
        for p in range(passes):
            row = {"k": k, "pass": p, "batches": nb}
            for name, index in (("l2", l2), ("ip", ip)):
                if index is None:
                    continue
                t, sc, ids, retried, exact = timed_batches(index, qn, k, nb)
                row.update({f"{name}_ms_per_batch": 1e3 * t / nb, f"{name}_queries_per_s": a.nq / t,
                            f"{name}_retried_queries": retried, f"{name}_exact_queries": exact})
                if name == "l2":
                    last[k] = (sc, ids)
            if ip is not None:
                row["l2_over_ip_time"] = row["l2_ms_per_batch"] / row["ip_ms_per_batch"]
            rows.append(row)
            say(row)
        summary = {"k": k, "l2_ms_per_batch_median": float(np.median([r["l2_ms_per_batch"] for r in rows])),
                   "l2_queries_per_s_median": float(np.median([r["l2_queries_per_s"] for r in rows])),
                   "l2_retried_queries": sum(r["l2_retried_queries"] for r in rows),
                   "l2_exact_queries": sum(r["l2_exact_queries"] for r in rows)}
        if ip is not None:
            ratios = [r["l2_over_ip_time"] for r in rows]
            summary.update({"ip_ms_per_batch_median": float(np.median([r["ip_ms_per_batch"] for r in rows])),
                            "l2_over_ip_time_median": float(np.median(ratios)), "l2_over_ip_time_min": min(ratios),
                            "l2_over_ip_time_max": max(ratios)})
        say(summary)
        res["runs"].append({"passes": rows, "summary": summary})
    if a.verify:
        from test_dense_l2 import oracle_topk_l2
        k = ks[-1]
        sel = np.linspace(0, a.nq - 1, a.verify).astype(int)
        ws, wi = oracle_topk_l2(l2.xb, q[sel], k, qblock=16, rblock=1 << 20)
        gs, gi = last[k][0][sel], last[k][1][sel]
        res["verified_queries"] = int(len(sel))
        res["verified_equal"] = bool(np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32)))
        say({"oracle_check_queries": int(len(sel)), "equal": res["verified_equal"]})
    if not a.quick:
        k = ks[0]
        xsq = l2._xsq[: l2.ntotal]
        torch_l2_topk(l2.xb, xsq, q[:a.batch], k, a.batch)    # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ts, ti = torch_l2_topk(l2.xb, xsq, q, k, a.batch)
        torch.cuda.synchronize()
        tt = time.perf_counter() - t0
        tl = res["runs"][0]["summary"]["l2_ms_per_batch_median"] * nb / 1e3       # the same queries, host arrays in and out
        sc = last[k][0]
        # ids compared at the ranks whose distance differs from both neighbours by more than the chain's and the expanded
        # form's error together (the bound of the screen, ops.dense_l2_error_bound, at the norms of this data)
        margin = 2.0 * float(ops.dense_l2_error_bound(a.d, float(q.norm(dim=1).max()), float(l2._xnorm_max)))
        gap = np.minimum(np.abs(np.diff(sc, axis=1, prepend=-np.inf)), np.abs(np.diff(sc, axis=1, append=np.inf)))
        sure = gap > margin
        row = {"torch_composition": "addmm(xsq, q, x.T, alpha=-2) + topk(smallest), 2^21-row chunks", "k": k, "torch_s": tt,
               "l2_s": tl, "speedup_vs_torch": tt / tl, "ids_compared": int(sure.sum()),
               "ids_equal": int((ti[sure] == last[k][1][sure]).sum())}
        say(row)
        res["torch"] = row
        res["exact_kernel"] = exact_kernel_alone(l2.xb[:131072], q[:1200].contiguous(), say)
        res["small"] = []
        for nq in [int(v) for v in a.small.split(",")]:
            qq = q[:nq].contiguous()
            row = {"nq": nq, "k": 100}
            legs = [("l2", lambda: ops.dense_search_l2(l2.xb, qq, 100, xsq=xsq, xnorm_max=l2._xnorm_max))]
            if ip is not None:
                legs.append(("ip", lambda: ops.dense_search(ip.xb, qq, 100)))
            for name, fn in legs:
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
                row[name + "_ms"] = 1e3 * (time.perf_counter() - t0) / 10
            res["small"].append(row)
            say(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
