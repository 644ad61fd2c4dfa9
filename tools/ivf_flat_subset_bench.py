#!/usr/bin/env python3
"""Subset search of the IVF-flat index (IVFFlatIndex.search(params=SearchParameters(sel=...)), the MAP form of the scan of
csrc/ivf_flat.hip) against its yardstick, at the README's shape (development tool, GPU): 8 841 823 x 768 clustered rows in 5 000
trained cells, 1 200-query batches, k = 100; fp32, fp16 and int8 stores; nprobe 8 / 32 / 128 under the inner product and
nprobe 32 under L2 as well.

    python tools/ivf_flat_subset_bench.py [--n 8841823] [--stores fp32,fp16,int8] [--passes 4] [--batches 2]
                                          [--min-ms 200] [--out profiles/ivf_flat_subset_bench.txt]

Data, centroids and cells as tools/ivf_flat_bench.py makes them (clustered Gaussian rows, k-means on a seeded sample of 2^18
rows, every row assigned once).  Per store and selection — a random 10 % and a random 50 % of the ids (IDSelectorBatch), and the
identity (IDSelectorRange over every id) — every pass times
  subset      index.search(q, k, nprobe, params=SearchParameters(sel=...)) on the full index, in place, and next to it
  yardstick   the plain search of a MATERIALISED sub-index: an IVFFlatIndex with the same centroids (and codec range) that holds
              a copy of the selected rows under the same cells (for the identity: the plain search of the full index itself),
alternating, `passes` times in one process: ms per batch of both, the ratio per pass, the spread of each leg over its passes
(a timed leg runs its batches again and again until it spans at least `--min-ms`, the same number of rounds in both legs, after
one untimed round of both: a leg of two sub-millisecond batches would time the clock and the scheduler, not the search),
`fallback_queries`, and the rows and bytes the scan's tasks read per batch (both legs read the same rows: a task reads the
selected rows of its cell).  Before timing, the first batch's ids and score bits of both legs are compared (the sub-index ids
mapped through the selection).  The selection is built once per selector and store (cached on the selector): its cost is
printed on its own, for 10 %, 50 % and all 8.84 M ids, and is not part of the timed legs.  A leg passes if its ratio stays
within 1 + max(0.07, twice that run's own spread of the yardstick leg); every comparison also prints the scan kernel's own
device time in both legs (the library's profiling events), which says whether a gap sits in the scan or around it.
Both the full index and every sub-index are built through the index's own interface: `set_coarse` with the same centroids,
`train_sq` on all rows for the int8 store (so both hold the same range), `set_lists` with the rows and the cells assigned once."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from repconc_amd import _lib, ops  # noqa: E402
from repconc_amd.index import METRIC_INNER_PRODUCT, METRIC_L2  # noqa: E402
from repconc_amd.ivf import coarse_assign, coarse_kmeans  # noqa: E402
from repconc_amd.ivf_flat import IVFFlatIndex  # noqa: E402
from repconc_amd.selector import IDSelectorBatch, IDSelectorRange, SearchParameters  # noqa: E402

DEV = "cuda:0"
NAMES = {METRIC_INNER_PRODUCT: "ip", METRIC_L2: "l2"}
STORAGE = {"fp32": "float32", "fp16": "float16", "int8": "int8"}
OUT = None


def say(*a):
    line = " ".join(str(v) for v in a)
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


def clustered(n, d, g, chunk=1 << 19):
    centers = torch.randn(64, d, device=DEV, generator=g)
    x = torch.empty((n, d), dtype=torch.float32, device=DEV)
    for r0 in range(0, n, chunk):
        m = min(chunk, n - r0)
        a = torch.randint(0, 64, (m,), device=DEV, generator=g)
        x[r0:r0 + m] = 0.7 * centers[a] + 0.5 * torch.randn(m, d, device=DEV, generator=g)
    return x


def timed(fn, batches, rounds=1):
    """ms per batch over `rounds` rounds of the batches."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(rounds):
        for qb in batches:
            fn(qb)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / (rounds * len(batches))


def scan_ms(fn, qb):
    """Device ms of the scan kernel alone in one search of the batch (summed over its chunks)."""
    lib, h = _lib.load(), _lib.handle(0)
    n, ms = C.c_int(0), C.c_double(0.0)
    lib.rc_profile_enable(h, 1)
    lib.rc_profile_collect(h, 1, C.byref(n), C.byref(ms))
    fn(qb)
    torch.cuda.synchronize()
    lib.rc_profile_collect(h, 1, C.byref(n), C.byref(ms))
    lib.rc_profile_enable(h, 0)
    return ms.value


def work(index, qb, nprobe, sel_off):
    """(rows scored, rows read by the tasks) of one batch over the cells' sizes under `sel_off`: a task = a cell and up to 8 of
    the queries probing it, and reads the cell's (selected) rows once."""
    probes = index.probe(qb, nprobe, ordered=False).long()
    sizes = sel_off[1:] - sel_off[:-1]
    per_cell = torch.bincount(probes.reshape(-1), minlength=index.nlist)
    qg = ops.ivf_flat_query_group()
    return int((per_cell * sizes).sum()), int(((per_cell + qg - 1) // qg * sizes).sum())


def make_index(a, sname, coarse, x, rows, cells):
    """An index of this store with the given centroids, the int8 range of ALL rows x, and the fp32 rows `rows` under `cells`."""
    index = IVFFlatIndex(a.d, a.nlist, storage=STORAGE[sname])
    index.set_coarse(coarse)
    if sname == "int8":
        index.train_sq(x)
    index.set_lists(rows, cells)
    return index


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8841823)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1200)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--min-ms", type=float, default=200.0, help="least span of one timed leg")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nlist", type=int, default=5000)
    ap.add_argument("--nprobes", default="8,32,128")
    ap.add_argument("--stores", default="fp32,fp16,int8")
    ap.add_argument("--fractions", default="0.1,0.5,1", help="shares of the ids selected; 1 = the identity")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        OUT = open(a.out, "w")
    nprobes = [int(v) for v in a.nprobes.split(",")]
    configs = [(METRIC_INNER_PRODUCT, p) for p in nprobes] + [(METRIC_L2, 32)]
    g = torch.Generator(device=DEV).manual_seed(20231)
    x = clustered(a.n, a.d, g)
    pick = torch.randperm(a.n, device=DEV, generator=g)[: a.batch * a.batches]
    batches = [x[pick[i * a.batch:(i + 1) * a.batch]] + 0.3 * torch.randn(a.batch, a.d, device=DEV, generator=g)
               for i in range(a.batches)]
    say(f"ivf_flat_subset_bench: N={a.n} D={a.d} nlist={a.nlist} k={a.k}, {a.batches} batches of {a.batch} queries per round, a leg = the rounds "
        f"that span >= {a.min_ms:.0f} ms, {a.passes} alternating passes, clustered rows, {torch.cuda.get_device_name(0)}")
    say("yardstick: the plain search of a materialised sub-index of the same rows (same centroids, cells and range; identity: the "
        "plain search of the full index), same process and pass; a leg passes within 1 + max(0.07, 2 x the yardstick's spread)")
    train = torch.from_numpy(np.sort(np.random.default_rng(1234).permutation(a.n)[:1 << 18])).to(DEV)
    coarse = coarse_kmeans(x[train], a.nlist)
    cells = coarse_assign(x, coarse)
    fractions = [float(v) for v in a.fractions.split(",")]
    kept = {}
    for frac in fractions:
        if frac < 1.0:
            kept[frac] = torch.sort(torch.randperm(a.n, device=DEV, generator=g)[: int(round(frac * a.n))]).values
    worst = []
    for sname in a.stores.split(","):
        index = make_index(a, sname, coarse, x, x, cells)
        esz = index.xb.element_size()
        for frac in fractions:
            if frac >= 1.0:
                name, sel, sub, ids_of = "identity", IDSelectorRange(0, a.n), index, None
            else:
                name, sel, ids_of = f"{int(round(100 * frac))} % of the ids", IDSelectorBatch(kept[frac]), kept[frac]
                sub = make_index(a, sname, coarse, x, x[ids_of], cells[ids_of])
            params = SearchParameters(sel=sel)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows, sel_off, _ = index._selection(sel)
            torch.cuda.synchronize()
            first = 1e3 * (time.perf_counter() - t0)
            fresh = IDSelectorRange(0, a.n) if ids_of is None else IDSelectorBatch(ids_of)       # the same ids, nothing cached
            t0 = time.perf_counter()
            index._selection(fresh)
            torch.cuda.synchronize()
            say(f"{sname}, {name}: selection of {rows.numel()} rows built in {first:.1f} ms, again from a fresh selector of the same "
                f"ids in {1e3 * (time.perf_counter() - t0):.1f} ms (selector -> mask -> positions and offsets per cell, with its "
                f"host copy of the sizes; once per selector and store, not in the timed legs)")
            del fresh
            for metric, nprobe in configs:
                index.metric_type = sub.metric_type = metric
                mapped = lambda qb: index.search(qb, a.k, nprobe=nprobe, params=params)      # noqa: E731
                yard = lambda qb: sub.search(qb, a.k, nprobe=nprobe)                         # noqa: E731
                s0, i0 = mapped(batches[0])                             # the warm-up of both legs, and their comparison
                st_m = dict(index.last_search_stats)
                s1, i1 = yard(batches[0])
                st_y = dict(sub.last_search_stats)
                if ids_of is not None:
                    i1 = torch.where(i1 >= 0, ids_of[i1.clamp(min=0)], i1)
                same = bool((i0 == i1).all()) and bool((s0.view(torch.int32) == s1.view(torch.int32)).all())
                warm = max(timed(mapped, batches), timed(yard, batches))         # the untimed round of both legs
                rounds = max(1, int(np.ceil(a.min_ms / (warm * len(batches)))))
                tm, ty = [], []
                for _ in range(a.passes):
                    tm.append(timed(mapped, batches, rounds))
                    ty.append(timed(yard, batches, rounds))
                spread = lambda t: (max(t) - min(t)) / min(t)           # noqa: E731
                ratios = [m / y for m, y in zip(tm, ty)]
                bound = 1.0 + max(0.07, 2.0 * spread(ty))
                ok = max(ratios) <= bound
                pairs, read_rows = work(index, batches[0], nprobe, sel_off)
                km, ky = scan_ms(mapped, batches[0]), scan_ms(yard, batches[0])
                worst.append((max(ratios), bound, sname, name, NAMES[metric], nprobe))
                say(f"  {NAMES[metric]} {sname} nprobe {nprobe:3d}, {name}: ids and score bits equal the yardstick's: {same}; subset "
                    f"{' '.join(f'{v:.3f}' for v in tm)} ms/batch, yardstick {' '.join(f'{v:.3f}' for v in ty)} ms/batch, ratio per pass "
                    f"{' '.join(f'{v:.4f}' for v in ratios)}; spread subset {100 * spread(tm):.2f} %, yardstick {100 * spread(ty):.2f} %; "
                    f"bound {bound:.4f} -> {'within' if ok else 'OUTSIDE'} ({rounds} rounds per leg)")
                say(f"      scan kernel {km:.3f} ms subset, {ky:.3f} ms yardstick ({km / ky if ky else float('nan'):.4f}); {pairs / a.batch:.0f} rows "
                    f"scored per query, tasks read {read_rows} rows = {read_rows * a.d * esz / 1e9:.2f} GB per batch; chunks "
                    f"{st_m['chunks']} / {st_y['chunks']}, fallback_queries {st_m['fallback_queries']} / {st_y['fallback_queries']}")
            if sub is not index:
                del sub
            del rows, sel_off, sel, params
            torch.cuda.empty_cache()
        del index
        torch.cuda.empty_cache()
    w = max(worst, key=lambda t: t[0] / t[1])
    say(f"worst leg against its bound: {w[2]} {w[4]} nprobe {w[5]}, {w[3]}: ratio {w[0]:.4f}, bound {w[1]:.4f}; legs outside their "
        f"bound: {sum(1 for t in worst if t[0] > t[1])} of {len(worst)}")


if __name__ == "__main__":
    main()
