#!/usr/bin/env python3
"""The two backwards of `ops.decode` side by side (development tool, GPU): the fp32 atomic scatter (`rc_pq_decode_bwd`, the
default) and the fixed-order fp64 sums (`rc_pq_decode_bwd_det`, `deterministic=True`: a stable sort of the rows by code per
sub-quantiser, then one owner per output element).  One backward of decode alone — torch.autograd.grad of the decoded rows
w.r.t. the centroids for a given grad_out, which is the gradient buffer, the workspace and the kernels — at

    49 152 x 768 and 6 144 x 768, M = 48, constrained-style codes: every code equally often, a random permutation per column
                                          (a stage-1 batch and one of its gradient-cache chunks)
    25 728 x 768, M = 48, uniform codes   (the stage-2 decode head's 128 x 201 rows)

Per shape and path: median / min / max of `iters` HIP-event timings after `warmup` untimed calls, in the same run on the same
card, the paths alternating shape by shape; torch.cuda.max_memory_allocated above what was resident before the call; whether
`repeats` calls on the same input gave identical bits; and the largest difference between the two paths.

    python tools/decode_bwd_bench.py [--iters 50] [--warmup 10] [--repeats 5] [--shapes 49152,6144,25728] [--out profiles/decode_bwd_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {49152: "balanced", 6144: "balanced", 25728: "uniform"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=48)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="49152,6144,25728")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from repconc_amd import ops
    dev = torch.device("cuda", 0)
    D, M = 768, a.M
    g = torch.Generator(device=dev).manual_seed(2025)
    lines = [f"device {torch.cuda.get_device_name(0)}; one backward of ops.decode (autograd.grad w.r.t. the centroids), M = {M}, D = {D}; "
             f"{a.iters} timed calls after {a.warmup}, HIP events"]
    for n in (int(x) for x in a.shapes.split(",")):
        kind = SHAPES.get(n, "uniform")
        if kind == "balanced":      # every code n / 256 times (to within one) in every column, in a random order per column
            codes = torch.stack([torch.randperm(n, device=dev, generator=g) % 256 for _ in range(M)], 1).to(torch.uint8).contiguous()
        else:
            codes = torch.randint(0, 256, (n, M), device=dev, generator=g, dtype=torch.uint8)
        C = (0.05 * torch.randn((M, 256, D // M), device=dev, generator=g)).requires_grad_(True)
        go = torch.randn((n, D), device=dev, generator=g)
        outs = {False: ops.decode(codes, C, deterministic=False), True: ops.decode(codes, C, deterministic=True)}

        def bwd(det):
            return torch.autograd.grad(outs[det], C, go, retain_graph=True)[0]

        res, med = {}, {}
        for det in (False, True):
            for _ in range(a.warmup):
                bwd(det)
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                bwd(det)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            bwd(det)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            runs = [bwd(det).clone() for _ in range(a.repeats)]
            same = all(torch.equal(r, runs[0]) for r in runs)
            res[det], med[det] = runs[0], statistics.median(ms)
            name = "deterministic" if det else "atomics"
            lines.append(f"n={n:6d} {kind:8s} {name:13s}  median {med[det]:8.4f} ms  min {min(ms):8.4f} ms  max {max(ms):8.4f} ms  "
                         f"peak memory above resident {peak / 2 ** 20:8.2f} MiB (workspace {ops.decode_bwd_ws_bytes(n, M) / 2 ** 20 if det else 0:.2f} MiB)  "
                         f"{a.repeats} runs bit-identical: {same}")
        lines.append(f"n={n:6d} {kind:8s} deterministic / atomics = {med[True] / med[False]:.2f}x (medians); "
                     f"max |difference| {float((res[True] - res[False]).abs().max()):.3e}, max |grad_C| {float(res[True].abs().max()):.3e}")
        del outs, codes, go, C
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
