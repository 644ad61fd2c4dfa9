#!/usr/bin/env python3
"""Exact IVF search over dense rows (csrc/ivf_flat.hip, IVFFlatIndex) at the README's shape (development tool, GPU):
8 841 823 x 768 rows, nlist 5000 trained, 1200-query batches, k = 100; fp32, fp16 and int8 stores, the int8 store also with
residual encoding, both metrics.

    python tools/ivf_flat_bench.py [--n 8841823] [--batches 2] [--passes 4] [--stores fp32,fp16,int8,int8r] [--out profiles/ivf_flat_bench.txt]

Data: clustered Gaussian rows as in tools/dense_bench.py (0.7 centre + 0.5 noise, 64 centres), generated on the device in
chunks; the queries are corpus rows plus 0.3 N(0, 1).  The coarse centroids are fitted once on a seeded sample of 2^18 rows
(coarse_kmeans) and every row assigned once (coarse_assign); the fp32, the fp16 and the int8 index store their own list-major
copy.  The int8 store holds the 8-bit scalar-quantiser codes of the same rows (range trained on all of them); its flat
counterpart is FlatSQ8Index under the inner product, and there is none under L2 (nor a re-ranking flat index over codes: the
refined IVF-PQ line is left out for this store).  After the legs: the int8 / fp16 time ratio of every IVF run, per pass.
`int8r` (needs `int8`): IVFFlatIndex(storage="int8", by_residual=True) over the same rows and cells, the codes of x - coarse[cell]
under the range of all residuals.  Its searches run INSIDE the int8 leg, pass by pass beside the plain int8 ones (the yardstick of
its time is the plain leg of the same pass), with their top-10 overlap with the fp32 flat result; after the legs: the residual /
plain int8 time ratio of every IVF run, per pass.

Per storage and metric, on `--passes` alternating passes in one process, ms per batch of
  * IVFFlatIndex at nprobe 8 / 32 / 128,
  * the flat index of the same vectors,
  * RefineIndex(IVFPQIndex, flat) at nprobe 32 (M = 48 codes, k_factor 10),
with the top-10 overlap of each with the flat result of the same store and, beside it, with the fp32 flat result; and for the IVFFlatIndex runs the rows and bytes of the probed cells per
batch (every (cell, group of 8 queries) task reads its cell once), the chain steps, the scan kernel's own time (the library's
profiling events around its launch) and the two bounds it is held against: the cells' bytes at the achievable HBM rate
(6.3 TB/s; 8 TB/s peak) and the chain steps at the fp32 vector rate the guide measures for v_pk_fma_f32 (52 TFLOP/s = 26 T
steps/s for the inner product; an L2 step is a subtraction and an fma: half of that)."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from repconc_amd import _lib, ops  # noqa: E402
from repconc_amd.dense_index import (FlatIPIndex, FlatL2F16Index, FlatL2Index, FlatSQ8Index, sq8_encode,  # noqa: E402
                                     sq8_train_range)
from repconc_amd.index import METRIC_INNER_PRODUCT, METRIC_L2, PQIndex  # noqa: E402
from repconc_amd.ivf import IVFPQIndex, coarse_assign, coarse_kmeans  # noqa: E402
from repconc_amd.ivf_flat import IVFFlatIndex  # noqa: E402
from repconc_amd.refine_index import RefineIndex  # noqa: E402

DEV = "cuda:0"
HBM_ACHIEVABLE = 6.3e12
VALU_STEPS = {METRIC_INNER_PRODUCT: 26e12, METRIC_L2: 13e12}
NAMES = {METRIC_INNER_PRODUCT: "ip", METRIC_L2: "l2"}
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


def timed(fn, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = [fn(qb) for qb in batches]
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / len(batches), out


def overlap10(ids, exact):
    return (ids[:, :10].unsqueeze(2) == exact[:, :10].unsqueeze(1)).any(2).float().mean().item()


def hang(index, store, metric):
    """The flat index `index` over the shared rows `store` (no copy): what its `add` would have left.  This writes the private
    attributes of dense_index._FlatIndex / _FlatL2 (`_x`, `_xsq`, `_xnorm_max`), as tools/dense_rerank_bench.py does, because an
    `add` would hold a second 27 GB copy per index; main() likewise fills IVFFlatIndex through `_store` (one assignment pass for
    both storages) and switches `metric_type` on the live indexes, which keep nothing that depends on the metric.  A change of
    those internals has to be followed here."""
    index._x, index.ntotal = store, store.shape[0]
    if store.dtype == torch.int8:
        index._cstat = ops.dense_sq8_cstat(store, index._dec)
        return index
    if metric == METRIC_L2:
        index._xsq = ops.dense_row_sqnorms(store)
        index._xnorm_max = ops._dense_l2_xnorm_max(index._xsq)
    elif store.dtype == torch.float16:
        index._xnorm_max = ops.dense_f16_xnorm_max(store)
    return index


def scan_ms(index, qb, k, nprobe):
    """Device ms of the scan kernel alone in one search of the batch (summed over its chunks)."""
    lib, h = _lib.load(), _lib.handle(0)
    n, ms = C.c_int(0), C.c_double(0.0)
    lib.rc_profile_enable(h, 1)
    lib.rc_profile_collect(h, 1, C.byref(n), C.byref(ms))
    index.search(qb, k, nprobe=nprobe)
    torch.cuda.synchronize()
    lib.rc_profile_collect(h, 1, C.byref(n), C.byref(ms))
    lib.rc_profile_enable(h, 0)
    return ms.value, n.value


def work(index, qb, nprobe):
    """(rows scored, rows read by the tasks, tasks) of one batch: a task = a cell and up to 8 of the queries probing it."""
    probes = index.probe(qb, nprobe, ordered=False).long()
    sizes = index.list_off[1:] - index.list_off[:-1]
    per_cell = torch.bincount(probes.reshape(-1), minlength=index.nlist)
    qg = ops.ivf_flat_query_group()
    tasks = (per_cell + qg - 1) // qg
    return int((per_cell * sizes).sum()), int((tasks * sizes).sum()), int(tasks.sum()), int(((per_cell > 0) * sizes).sum())


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8841823)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--m", type=int, default=48)
    ap.add_argument("--batch", type=int, default=1200)
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--nlist", type=int, default=5000)
    ap.add_argument("--nprobes", default="8,32,128")
    ap.add_argument("--stores", default="fp32,fp16,int8,int8r")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        OUT = open(a.out, "w")
    nprobes = [int(v) for v in a.nprobes.split(",")]
    g = torch.Generator(device=DEV).manual_seed(20231)
    x = clustered(a.n, a.d, g)
    x16 = torch.empty((a.n, a.d), dtype=torch.float16, device=DEV)
    for r0 in range(0, a.n, 1 << 20):
        x16[r0:r0 + (1 << 20)] = x[r0:r0 + (1 << 20)].half()
    sel = torch.randperm(a.n, device=DEV, generator=g)[: a.batch * a.batches]
    batches = [x[sel[i * a.batch:(i + 1) * a.batch]] + 0.3 * torch.randn(a.batch, a.d, device=DEV, generator=g)
               for i in range(a.batches)]
    say(f"ivf_flat_bench: N={a.n} D={a.d} nlist={a.nlist} k={a.k}, {a.batches} batches of {a.batch} queries, {a.passes} alternating "
        f"passes, clustered rows, {torch.cuda.get_device_name(0)}")
    t0 = time.perf_counter()
    train = torch.from_numpy(np.sort(np.random.default_rng(1234).permutation(a.n)[:1 << 18])).to(DEV)
    coarse = coarse_kmeans(x[train], a.nlist)
    cells = coarse_assign(x, coarse)
    torch.cuda.synchronize()
    sizes = torch.bincount(cells, minlength=a.nlist)
    say(f"coarse quantiser: {time.perf_counter() - t0:.1f} s (k-means on 2^18 rows + assignment of all); cell sizes min {int(sizes.min())} "
        f"mean {a.n / a.nlist:.0f} max {int(sizes.max())}")
    # the PQ side of the comparison: M codes from sampled rows, the same cells
    dsub = a.d // a.m
    pq = PQIndex(a.d, a.m)
    pq.set_centroids(x[torch.randperm(a.n, device=DEV, generator=g)[:256]].view(256, a.m, dsub).permute(1, 0, 2).contiguous())
    for r0 in range(0, a.n, 1 << 20):
        pq.add(x[r0:r0 + (1 << 20)])
    ivfpq = IVFPQIndex(a.d, a.m, a.nlist)
    ivfpq.set_centroids(pq.pq.centroids)
    ivfpq.coarse = coarse
    ivfpq.set_lists(pq.codes, cells)
    ivfpq.nprobe = 32
    del pq

    stores = a.stores.split(",")
    x8 = vmin8 = dec8 = None
    if "int8" in stores:
        vmin8, dec8 = sq8_train_range(x, DEV)
        x8 = torch.empty((a.n, a.d), dtype=torch.int8, device=DEV)
        for r0 in range(0, a.n, 1 << 20):
            x8[r0:r0 + (1 << 20)] = sq8_encode(x[r0:r0 + (1 << 20)], vmin8, dec8[0])
    index_r = None
    if "int8r" in stores:
        if "int8" not in stores:
            raise SystemExit("--stores int8r runs beside the plain int8 leg: name int8 too")
        index_r = IVFFlatIndex(a.d, a.nlist, storage="int8", by_residual=True)
        index_r.set_coarse(coarse)
        resid = lambda r0: x[r0:r0 + (1 << 20)] - coarse[cells[r0:r0 + (1 << 20)]]
        ends = [torch.stack([r.amin(0), r.amax(0)]) for r in (resid(r0) for r0 in range(0, a.n, 1 << 20))]
        index_r.vmin, index_r._dec = sq8_train_range(torch.cat(ends), DEV)            # the range is the extremes' alone
        index_r.step, index_r.mid = index_r._dec[0], index_r._dec[1]
        x8r = torch.empty((a.n, a.d), dtype=torch.int8, device=DEV)
        for r0 in range(0, a.n, 1 << 20):
            x8r[r0:r0 + (1 << 20)] = sq8_encode(resid(r0), index_r.vmin, index_r.step)
        index_r._store(x8r, cells)
        del x8r
        say(f"residual int8 store: largest step {float(index_r.step.max()):.5f} against {float(dec8[0].max()):.5f} of the plain int8 store "
            f"(mean {float(index_r.step.mean()):.5f} against {float(dec8[0].mean()):.5f})")
    flat32, allms = {}, {}          # the fp32 flat ids per metric; ms per pass of every (store, metric, path)
    for sname, store in (("fp32", x), ("fp16", x16), ("int8", x8)):
        if sname not in stores:
            continue
        index = IVFFlatIndex(a.d, a.nlist, storage={"fp32": "float32", "fp16": "float16", "int8": "int8"}[sname])
        index.set_coarse(coarse)
        if sname == "int8":
            index.vmin, index._dec = vmin8, dec8
            index.step, index.mid = dec8[0], dec8[1]
        index._store(store, cells)
        esz = store.element_size()
        for metric in (METRIC_INNER_PRODUCT, METRIC_L2):
            index.metric_type = ivfpq.metric_type = metric
            flat = None
            if sname == "int8":
                if metric == METRIC_INNER_PRODUCT:
                    flat = FlatSQ8Index(a.d)
                    flat.vmin, flat._dec, flat.is_trained = vmin8, dec8, True
                    flat.step, flat.mid = dec8[0], dec8[1]
                    flat = hang(flat, store, metric)
            elif metric == METRIC_L2:
                flat = hang(FlatL2F16Index(a.d) if sname == "fp16" else FlatL2Index(a.d), store, metric)
            else:
                flat = hang(FlatIPIndex(a.d, storage="float16" if sname == "fp16" else "float32"), store, metric)
            paths = {f"ivf-flat nprobe {p}": (lambda qb, p=p: index.search(qb, a.k, nprobe=p)) for p in nprobes}
            legs = [(index, "ivf-flat", sname)]
            if sname == "int8" and index_r is not None:
                index_r.metric_type = metric
                paths.update({f"ivf-flat residual nprobe {p}": (lambda qb, p=p: index_r.search(qb, a.k, nprobe=p)) for p in nprobes})
                legs.append((index_r, "ivf-flat residual", "int8r"))
            if flat is not None:
                paths["flat"] = lambda qb: flat.search(qb, a.k)
            if sname != "int8":
                paths["ivf-pq refined nprobe 32"] = lambda qb: RefineIndex(ivfpq, flat, 10).search(qb, a.k)
            stats = {}
            for n, fn in paths.items():
                fn(batches[0])                                          # warm every code object and allocation
                if n.startswith("ivf-flat"):
                    stats[n] = dict((index_r if "residual" in n else index).last_search_stats)
            ms, out = {n: [] for n in paths}, {}
            for _ in range(a.passes):
                for n, fn in paths.items():
                    t, out[n] = timed(fn, batches)
                    ms[n].append(t)
            exact = torch.cat([o[1] for o in out["flat"]]) if flat is not None else None
            if sname == "fp32":
                flat32[metric] = exact
            for n in paths:
                v = ms[n]
                allms[(sname, metric, n)] = v
                ids = torch.cat([o[1] for o in out[n]])
                own = "no flat index over residual codes" if "residual" in n else "no flat index over this store and metric" \
                    if exact is None else f"top-10 overlap with the flat result {overlap10(ids, exact):.3f}"
                if sname != "fp32" and metric in flat32:
                    own += f", with the fp32 flat result {overlap10(ids, flat32[metric]):.3f}"
                say(f"e2e {NAMES[metric]} {sname} {n:26s}: {sum(v) / len(v):8.3f} ms per batch (min {min(v):.3f} max {max(v):.3f}) = "
                    f"{a.batch / (sum(v) / len(v)):7.1f} k queries/s, {own}")
            flat_ms = sum(ms["flat"]) / len(ms["flat"]) if flat is not None else None
            n32 = sum(ms["ivf-flat nprobe 32"]) / len(ms["ivf-flat nprobe 32"]) if 32 in nprobes and flat is not None else None
            if n32 is not None:
                say(f"  condition {NAMES[metric]} {sname}: nprobe 32 takes {n32:.3f} ms, the flat search of the same store {flat_ms:.3f} ms "
                    f"-> {'met' if n32 < flat_ms else 'NOT MET'}")
            for leg, path, lname in legs:
                for p in nprobes:
                    pairs, read_rows, tasks, cell_rows = work(leg, batches[0], p)
                    kms, launches = scan_ms(leg, batches[0], a.k, p)
                    nbytes, steps = read_rows * a.d * esz, pairs * a.d
                    t_hbm, t_valu = 1e3 * nbytes / HBM_ACHIEVABLE, 1e3 * steps / VALU_STEPS[metric]
                    st = stats[f"{path} nprobe {p}"]
                    say(f"  scan {NAMES[metric]} {lname} nprobe {p:3d}: {pairs / a.batch:9.0f} rows scored per query, {tasks} tasks read "
                        f"{read_rows} rows = {nbytes / 1e9:.2f} GB per batch ({cell_rows * a.d * esz / 1e9:.2f} GB of distinct cells), "
                        f"{steps / 1e9:.1f} G chain steps; scan kernel {kms:.3f} ms in {launches} launch(es), bounds: HBM {t_hbm:.3f} ms, "
                        f"vector ALU {t_valu:.3f} ms -> {kms / max(t_hbm, t_valu):.2f} x the larger bound; chunks {st['chunks']}, "
                        f"fallback queries {st['fallback_queries']}")
            del flat
        del index
        torch.cuda.empty_cache()
    if "int8" in stores and "fp16" in stores:
        for metric in (METRIC_INNER_PRODUCT, METRIC_L2):
            for p in nprobes:
                n = f"ivf-flat nprobe {p}"
                r = [i8 / f16 for i8, f16 in zip(allms[("int8", metric, n)], allms[("fp16", metric, n)])]
                say(f"int8 / fp16 time, {NAMES[metric]} nprobe {p:3d}: {sum(r) / len(r):.3f} over {len(r)} passes (min {min(r):.3f} "
                    f"max {max(r):.3f})")
    if index_r is not None:
        for metric in (METRIC_INNER_PRODUCT, METRIC_L2):
            for p in nprobes:
                res, plain = allms[("int8", metric, f"ivf-flat residual nprobe {p}")], allms[("int8", metric, f"ivf-flat nprobe {p}")]
                r = [a_ / b_ for a_, b_ in zip(res, plain)]
                say(f"residual / plain int8 time, {NAMES[metric]} nprobe {p:3d}: {sum(r) / len(r):.3f} over {len(r)} passes (min {min(r):.3f} "
                    f"max {max(r):.3f}; per pass {' '.join(f'{v:.3f}' for v in r)}; plain ms per pass "
                    f"{' '.join(f'{v:.3f}' for v in plain)})")


if __name__ == "__main__":
    main()
