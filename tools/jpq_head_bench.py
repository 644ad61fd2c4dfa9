#!/usr/bin/env python3
"""The two scoring heads of the stage-2 (JPQ) step side by side (development tool, GPU): one forward + backward of
`head="decode"` (index_select -> ops.decode -> multiply -> sum, twice: negatives and positives; fp32 atomic scatter into the
centroid gradient) and of `head="fused"` (one ops.jpq_scores call; fixed-order fp64 sums, no atomics on values) at the
recipe's stage-2 shape: 128 queries x (1 positive + 200 negatives), M = 48, D = 768, over an index of synthetic uniform codes.
The search that picks the negatives is the same for both heads and is not timed: the ids are drawn once.

Per head: median / min of `iters` HIP-event timings after `warmup` untimed steps, torch.cuda.max_memory_allocated above what
was resident before the step, and whether `repeats` backward passes of the same step gave bit-identical gradients.

    python tools/jpq_head_bench.py [--rows 1048576] [--iters 50] [--warmup 10] [--repeats 5] [--out profiles/jpq_head_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--nq", type=int, default=128)
    ap.add_argument("--negatives", type=int, default=200)
    ap.add_argument("--M", type=int, default=48)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from repconc_amd import ops
    dev = torch.device("cuda", 0)
    D, M, nq, k, N = 768, a.M, a.nq, a.negatives, a.rows
    g = torch.Generator(device=dev).manual_seed(2024)
    codes = torch.randint(0, 256, (N, M), device=dev, generator=g, dtype=torch.uint8)
    C = (0.05 * torch.randn((M, 256, D // M), device=dev, generator=g)).requires_grad_(True)
    q = torch.randn((nq, D), device=dev, generator=g).requires_grad_(True)
    neg = torch.randint(0, N, (nq, k), device=dev, generator=g)
    pos = torch.randint(0, N, (nq,), device=dev, generator=g)
    labels = torch.zeros(nq, dtype=torch.long, device=dev)

    def decode_head():                                   # the lines of JPQ.forward, head="decode"
        negd = ops.decode(codes.index_select(0, neg.reshape(-1)), C).reshape(nq, k, -1)
        sn = (q.unsqueeze(1) * negd).sum(-1)
        sp = (q * ops.decode(codes.index_select(0, pos), C)).sum(-1, keepdim=True)
        return torch.nn.functional.cross_entropy(torch.hstack((sp, sn)), labels)

    def fused_head():                                    # head="fused"
        s = ops.jpq_scores(q, codes, torch.cat([pos[:, None], neg], 1), C)
        return torch.nn.functional.cross_entropy(s, labels)

    def step(head):
        q.grad = C.grad = None
        loss = head()
        loss.backward()
        return loss.detach(), q.grad, C.grad

    lines = [f"device {torch.cuda.get_device_name(0)}; {nq} queries x (1 + {k}) ids, M = {M}, D = {D}, {N} rows of uniform codes; "
             f"{a.iters} timed steps after {a.warmup}, HIP events around forward + backward"]
    res = {}
    for name, head in (("decode", decode_head), ("fused", fused_head)):
        for _ in range(a.warmup):
            step(head)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(head)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        q.grad = C.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step(head)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        runs = [tuple(t.clone() for t in step(head)) for _ in range(a.repeats)]
        same_q = all(torch.equal(r[1], runs[0][1]) for r in runs)
        same_c = all(torch.equal(r[2], runs[0][2]) for r in runs)
        res[name] = runs[0]
        lines.append(f"head={name:6s}  median {statistics.median(ms):8.4f} ms  min {min(ms):8.4f} ms  max {max(ms):8.4f} ms  "
                     f"peak memory above resident {peak / 2 ** 20:8.2f} MiB  {a.repeats} backward runs bit-identical: "
                     f"grad_q {same_q}, grad_C {same_c}")
    dl = abs(float(res["decode"][0]) - float(res["fused"][0]))
    dq = float((res["decode"][1] - res["fused"][1]).abs().max())
    dc = float((res["decode"][2] - res["fused"][2]).abs().max())
    lines.append(f"fused against decode: |loss difference| {dl:.3e}, max |grad_q difference| {dq:.3e}, max |grad_C difference| {dc:.3e}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
