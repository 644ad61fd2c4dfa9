#!/usr/bin/env python3
"""Subset search of the PQ and IVF-PQ indexes (PQIndex / IVFPQIndex.search(params=SearchParameters(sel=...))) against its
yardsticks, at the README's shape (development tool, GPU): 8 841 823 x 48 B uniform codes, 1 200-query batches, k = 1000.

    python tools/adc_subset_bench.py [--n 8841823] [--m 48] [--passes 4] [--batches 2] [--min-ms 200] [--nlist 5000]
                                     [--out profiles/adc_subset_bench.txt]

Selections: a random sorted 10 % and 50 % of the rows (IDSelectorBatch) and the identity (IDSelectorRange over every id).  One
process, `passes` alternating passes per comparison; a timed leg runs its batches again and again until it spans `--min-ms`, the
same number of rounds in both legs, after one untimed round of both.

  search     index.search(q, k, params=...) with the selection cached on the selector, against the plain search of a MATERIALISED
             PQIndex that holds codes[rows] (identity: the plain search of the index itself).  The kernels are the same ones plus
             one nq x k id map: a leg passes within 1.07 of its yardstick; the pass-to-pass spread of both legs is printed beside the
             ratio.  Before timing, ids and score bits of the first batch are compared.
  build      ops.adc_select_rows (one kernel: compact codes + image) against the composition available without it,
             codes.index_select(0, rows) + rc_adc_scan_image over the copy, same pass; and against the byte bound
             ns (8 + M) read + 2 ns M written at 6.3 TB/s.  It has to be no slower than the yardstick beyond the yardstick's spread.
  fresh      a single-query search at 10 % through a selector that has nothing cached (selector -> rows -> selection -> search)
             against the same search with the selection cached.
  IVF        IVFPQIndex (uniformly random cells: the comparison is between two indexes of the same rows, not between probe
             qualities), nprobe 8 / 32 at 10 % and 50 %, against the IVFPQIndex built by set_lists over the selected rows; 1.07."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from repconc_amd import ops  # noqa: E402
from repconc_amd.index import PQIndex  # noqa: E402
from repconc_amd.ivf import IVFPQIndex  # noqa: E402
from repconc_amd.selector import IDSelectorBatch, IDSelectorRange, SearchParameters  # noqa: E402

DEV = "cuda:0"
BOUND = 1.07
HBM = 6.3e12
OUT = None


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


def timed(fn, items, rounds=1):
    """ms per item over `rounds` rounds of the items."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(rounds):
        for it in items:
            fn(it)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / (rounds * len(items))


def spread(t):
    return (max(t) - min(t)) / min(t)


def fmt(t, p=3):
    return " ".join(f"{v:.{p}f}" for v in t)


def compare(a, what, leg, yard, items, same, bound=BOUND):
    """`passes` alternating passes of two legs; returns (worst ratio, bound) and prints the line."""
    warm = max(timed(leg, items), timed(yard, items))
    rounds = max(1, int(-(-a.min_ms // (warm * len(items)))))
    tl, ty = [], []
    for _ in range(a.passes):
        tl.append(timed(leg, items, rounds))
        ty.append(timed(yard, items, rounds))
    ratios = [x / y for x, y in zip(tl, ty)]
    ok = max(ratios) <= bound
    say(f"  {what}: equal to the yardstick: {same}; subset {fmt(tl)} ms, yardstick {fmt(ty)} ms, ratio per pass {fmt(ratios, 4)}; "
        f"spread subset {100 * spread(tl):.2f} %, yardstick {100 * spread(ty):.2f} %; bound {bound:.2f} -> "
        f"{'within' if ok else 'OUTSIDE'} ({rounds} rounds per leg)")
    return max(ratios), bound, what


def equal(got, want, ids_of=None):
    s0, i0 = got
    s1, i1 = want
    if ids_of is not None:
        i1 = torch.where(i1 >= 0, ids_of[i1.clamp(min=0)], i1)
    return bool((i0 == i1).all()) and bool((s0.view(torch.int32) == s1.view(torch.int32)).all())


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8841823)
    ap.add_argument("--m", type=int, default=48)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1200)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--min-ms", type=float, default=200.0, help="least span of one timed leg")
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--nlist", type=int, default=5000)
    ap.add_argument("--nprobes", default="8,32")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        OUT = open(a.out, "w")
    N, M = a.n, a.m
    g = torch.Generator(device=DEV).manual_seed(20241)
    codes = torch.randint(0, 256, (N, M), dtype=torch.uint8, device=DEV, generator=g)
    cent = torch.randn((M, 256, a.d // M), device=DEV, generator=g)
    batches = [torch.randn((a.batch, a.d), device=DEV, generator=g) for _ in range(a.batches)]
    say(f"adc_subset_bench: N={N} M={M} k={a.k}, {a.batches} batches of {a.batch} queries per round, a leg = the rounds that span >= "
        f"{a.min_ms:.0f} ms, {a.passes} alternating passes, uniform codes, {torch.cuda.get_device_name(0)}")
    index = PQIndex(a.d, M)
    index.set_centroids(cent)
    index.add_codes(codes)
    kept = {f: torch.sort(torch.randperm(N, device=DEV, generator=g)[: int(round(f * N))]).values.contiguous() for f in (0.1, 0.5)}
    worst = []

    say("flat search, selection cached, against the plain search of a materialised PQIndex of the same rows (bound 1.07 per leg)")
    for name, rows in (("10 %", kept[0.1]), ("50 %", kept[0.5]), ("identity", None)):
        sel = IDSelectorRange(0, N) if rows is None else IDSelectorBatch(rows)
        params = SearchParameters(sel=sel)
        if rows is None:
            sub = index
        else:
            sub = PQIndex(a.d, M)
            sub.set_centroids(cent)
            sub.add_codes(codes[rows])
        leg = lambda qb: index.search(qb, a.k, params=params)                    # noqa: E731
        yard = lambda qb: sub.search(qb, a.k)                                    # noqa: E731
        same = equal(leg(batches[0]), yard(batches[0]), rows)
        st = dict(index.last_search.stats)
        worst.append(compare(a, f"flat {name}", leg, yard, batches, same))
        say(f"      repeated / exact-route queries of the subset leg's first batch: {st['retried_queries']} / {st['exact_queries']}; "
            f"cached selection: {0 if sel._adc[1] is None else (sel._adc[1].numel() + sel._adc[2].numel() + 8 * sel._adc[0].numel()) / 1e6:.1f} MB")
        if sub is not index:
            del sub
        torch.cuda.empty_cache()

    say("building a selection: ops.adc_select_rows against codes.index_select(0, rows) + rc_adc_scan_image over the copy")
    for name, rows in (("10 %", kept[0.1]), ("50 %", kept[0.5])):
        ns = rows.numel()

        def composed(_):
            c = codes.index_select(0, rows)
            img = torch.empty((ops.adc_image_bytes(ns, M),), dtype=torch.uint8, device=DEV)
            ops.adc_scan_image_(c, img)

        build = lambda _: ops.adc_select_rows(codes, rows, "flat", check_rows=False)     # noqa: E731
        sc, si = build(None)
        c = codes.index_select(0, rows)
        img = ops.adc_scan_image_(c, torch.zeros_like(si))
        written = ops.adc_scan_image_(torch.full_like(c, 255), torch.zeros_like(si)) != 0
        same = bool(torch.equal(sc, c)) and bool(torch.equal(si[written], img[written]))
        del c, img, written, sc, si
        warm = max(timed(build, [0]), timed(composed, [0]))
        rounds = max(1, int(-(-a.min_ms // warm)))
        tb, ty = [], []
        for _ in range(a.passes):
            tb.append(timed(build, [0], rounds))
            ty.append(timed(composed, [0], rounds))
        ratios = [x / y for x, y in zip(tb, ty)]
        bound = 1.0 + spread(ty)
        nbytes = ns * (8 + M) + 2 * ns * M
        floor_ms = 1e3 * nbytes / HBM
        ok = max(ratios) <= bound
        worst.append((max(ratios), bound, f"build {name}"))
        say(f"  build {name} ({ns} rows): equal to the yardstick: {same}; one kernel {fmt(tb)} ms, index_select + image {fmt(ty)} ms, "
            f"ratio per pass {fmt(ratios, 4)}; spread {100 * spread(tb):.2f} % / {100 * spread(ty):.2f} %; bound 1 + the yardstick's "
            f"spread = {bound:.4f} -> {'within' if ok else 'OUTSIDE'}; byte bound {nbytes / 1e6:.1f} MB at 6.3 TB/s = {floor_ms:.4f} ms: "
            f"{min(tb) / floor_ms:.2f} x the bound ({nbytes / min(tb) / 1e9:.2f} TB/s)")

    say("a fresh selector: single-query search at 10 %, nothing cached, against the same search with the selection cached")
    rows = kept[0.1]
    one = batches[0][:1]
    cached = SearchParameters(sel=IDSelectorBatch(rows))
    index.search(one, a.k, params=cached)
    t_cached, t_fresh = [], []
    for _ in range(a.passes):
        t_cached.append(timed(lambda _: index.search(one, a.k, params=cached), [0], 20))
        t_fresh.append(timed(lambda _: index.search(one, a.k, params=SearchParameters(sel=IDSelectorBatch(rows))), [0], 20))
    say(f"  cached {fmt(t_cached)} ms, fresh {fmt(t_fresh)} ms per single-query search: a fresh selector costs "
        f"{min(t_fresh) - min(t_cached):.3f} ms (ids -> sorted unique rows -> one kernel)")

    say(f"IVF-PQ, nlist={a.nlist}, uniformly random cells, against the IVFPQIndex of the selected rows (bound 1.07 per leg)")
    cells = torch.randint(0, a.nlist, (N,), device=DEV, generator=g)
    coarse = torch.randn((a.nlist, a.d), device=DEV, generator=g)
    ivf = IVFPQIndex(a.d, M, a.nlist)
    ivf.coarse = coarse
    ivf.set_centroids(cent)
    ivf.set_lists(codes, cells)
    for name, rows in (("10 %", kept[0.1]), ("50 %", kept[0.5])):
        sel = IDSelectorBatch(rows)
        params = SearchParameters(sel=sel)
        sub = IVFPQIndex(a.d, M, a.nlist)
        sub.coarse = coarse
        sub.set_centroids(cent)
        sub.set_lists(codes[rows], cells[rows])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ivf._selection(sel)
        torch.cuda.synchronize()
        say(f"  IVF selection of {rows.numel()} rows built in {1e3 * (time.perf_counter() - t0):.1f} ms (mask -> positions and offsets "
            f"per cell with the host copy of the sizes -> one kernel)")
        for nprobe in [int(v) for v in a.nprobes.split(",")]:
            leg = lambda qb: ivf.search(qb, a.k, nprobe, params=params)          # noqa: E731
            yard = lambda qb: sub.search(qb, a.k, nprobe)                        # noqa: E731
            same = equal(leg(batches[0]), yard(batches[0]), rows)
            worst.append(compare(a, f"IVF {name} nprobe {nprobe}", leg, yard, batches, same))
        del sub, sel, params
        torch.cuda.empty_cache()
    w = max(worst, key=lambda t: t[0] / t[1])
    say(f"worst leg against its bound: {w[2]}: ratio {w[0]:.4f}, bound {w[1]:.4f}; legs outside their bound: "
        f"{sum(1 for t in worst if t[0] > t[1])} of {len(worst)}")


if __name__ == "__main__":
    main()
