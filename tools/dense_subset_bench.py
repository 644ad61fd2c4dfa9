"""Subset search of the flat dense searches (ops.dense_search*(rows=...)) against its yardsticks, at the README's corpus shape:
8 841 823 x 768, fp16 and fp32 storage, inner product, k = 100, batches of 1 163 queries (6 980 dev queries in six batches).
One process, one card, synthetic seeded data generated on the device.

    python tools/dense_subset_bench.py [--out profiles/dense_subset_bench.txt] [--n N] [--d D] [--passes 4] [--reps 3]
                                       [--storage float16 float32] [--fractions 0.1 0.5 1] [--no-small] [--check-rows]
    rocprofv3 --kernel-trace --stats -d DIR -o subset -- python tools/dense_subset_bench.py --storage float16 --fractions 0.1 \
                                       --no-small --passes 1        # which kernel a gap sits in: the MAP twins have names of their own

For each storage and each selection — a random 10 % and a random 50 % of the rows (sorted), and the identity — every pass times
  mapped      the search over the rows in place (rc_dense*_search_rows_q), and next to it
  yardstick   the existing search over a materialised copy x[rows] of the same rows (for the identity: the plain search of x),
`reps` batches each, alternating, `passes` times: ms per batch of both, their ratio per pass, and the queries repeated or
answered by the exact route.  The yardstick is always the other leg of the same process and pass, never the mapped search of
another run; the spread of a leg over its passes says what a ratio can resolve.  Before timing, the first batch's ids and
score bits of both legs are compared (the mapped ids against rows[copy ids]); that call verifies the row list
(check_rows=True).  The timed mapped calls pass check_rows=False, as the index classes do for a selector's list: the check is a
pass over the list and a host read per call, which --check-rows puts back into the timed legs.
The last line is the same comparison at D = 32 in fp16 (64-byte rows, shorter than the 128 bytes a gather wants), 50 % of rows.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from repconc_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8841823)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1163)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3, help="batches per timed leg")
    ap.add_argument("--storage", nargs="+", default=["float16", "float32"], choices=["float16", "float32"])
    ap.add_argument("--fractions", nargs="+", type=float, default=[0.1, 0.5, 1.0], help="shares of the rows selected; 1 = the identity")
    ap.add_argument("--check-rows", action="store_true", help="verify the row list in every timed call as well")
    ap.add_argument("--no-small", action="store_true", help="skip the D = 32 line")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def store(n, d, dtype, seed):
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        x = torch.empty((n, d), dtype=dtype, device=dev)
        step = 1 << 20
        for r0 in range(0, n, step):
            x[r0:r0 + step] = torch.randn((min(step, n - r0), d), generator=g, device=dev)
        q = [torch.randn((a.batch, d), generator=g, device=dev) for _ in range(a.reps)]
        return x, q

    def leg(search, x, q, **kw):
        """ms per batch over the `reps` batches, and the queries repeated / answered by the exact route"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pend = [search(x, qq, a.k, defer=True, **kw) for qq in q]
        for p in pend:
            p.result()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / len(q)
        return ms, sum(p.stats["retried_queries"] for p in pend), sum(p.stats["exact_queries"] for p in pend)

    def compare(search, x, q, what, fractions, norm):
        n = x.shape[0]
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        for frac in fractions:
            if frac >= 1.0:
                name, rows, y, ykw = "identity", torch.arange(n, dtype=torch.int64, device=dev), x, dict(norm)
            else:
                ns = int(round(frac * n))
                rows = torch.sort(torch.randperm(n, generator=g, device=dev)[:ns]).values.contiguous()
                name, y = f"{int(round(100 * frac))} % of the rows", x[rows]
                ykw = {"xnorm_max": ops.dense_xnorm_max(y)} if norm else {}
            mkw = dict(norm, rows=rows, check_rows=a.check_rows)
            s0, i0 = search(x, q[0], a.k, rows=rows, **norm)           # rows verified here; also the warm-up of both legs
            s1, i1 = search(y, q[0], a.k, **ykw)
            same = bool((i0 == rows[i1]).all()) and bool((s0.view(torch.int32) == s1.view(torch.int32)).all())
            say(f"{what}, {name} (ns = {rows.numel()}): ids and score bits of the first batch equal the yardstick's: {same}")
            tm, ty = [], []
            for p in range(a.passes):
                m = leg(search, x, q, **mkw)
                y_ = leg(search, y, q, **ykw)
                tm.append(m[0])
                ty.append(y_[0])
                say(f"  pass {p}: mapped {m[0]:8.2f} ms/batch (repeated {m[1]}, exact route {m[2]})   yardstick {y_[0]:8.2f} ms/batch "
                    f"(repeated {y_[1]}, exact route {y_[2]})   mapped / yardstick {m[0] / y_[0]:.4f}")
            spread = lambda t: (max(t) - min(t)) / min(t)
            ratios = [m_ / y_ for m_, y_ in zip(tm, ty)]
            say(f"  ratio min {min(ratios):.4f} max {max(ratios):.4f}; spread of a leg over its passes: mapped {100 * spread(tm):.2f} %, "
                f"yardstick {100 * spread(ty):.2f} %")
            del y, rows

    say(f"# tools/dense_subset_bench.py: N = {a.n}, D = {a.d}, k = {a.k}, batches of {a.batch} queries, {a.reps} batches per leg, "
        f"{a.passes} alternating passes; {torch.cuda.get_device_name(0)}")
    say("# yardstick: the existing search over a materialised copy x[rows] (identity: the plain search of x), same process and pass; "
        f"timed mapped calls: check_rows={a.check_rows}")
    for storage in a.storage:
        if storage == "float16":
            x, q = store(a.n, a.d, torch.float16, 1)
            compare(ops.dense_search_f16, x, q, f"fp16 {a.n} x {a.d}", a.fractions, {"xnorm_max": ops.dense_xnorm_max(x)})
        else:
            x, q = store(a.n, a.d, torch.float32, 2)
            compare(ops.dense_search, x, q, f"fp32 {a.n} x {a.d}", a.fractions, {})
        del x, q
        torch.cuda.empty_cache()
    if not a.no_small:
        x, q = store(a.n, 32, torch.float16, 3)
        compare(ops.dense_search_f16, x, q, f"fp16 {a.n} x 32 (64-byte rows)", (0.5,), {"xnorm_max": ops.dense_xnorm_max(x)})
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
