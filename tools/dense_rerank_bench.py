#!/usr/bin/env python3
"""Exact re-ranking of candidate lists (csrc/dense_rerank.hip, RefineIndex) at the README's shapes (development tool, GPU):
8 841 823 x 768 rows, M = 48 codes, 1200-query batches, k = 100 from kc = 1000; fp32 and fp16 stores, both metrics.

    python tools/dense_rerank_bench.py [--n 8841823] [--batches 3] [--passes 3] [--variants lane=build/var/rerank_lane.so,...]

Data: clustered Gaussian rows by oracle.synth.clustered_embeddings' construction (0.7 centre + 0.5 noise, 64 centres), generated
on the device in chunks; PQ centroids are 256 sampled rows cut per sub-space (oracle.synth.sample_centroids' construction); the
queries are corpus rows plus 0.3 N(0, 1).  One fp32 and one fp16 copy of the rows serve every flat index (the tool hangs them
into the index objects instead of `add`-ing four copies).

Prints
  1. the re-rank stage alone (one rc_dense_rerank / rc_dense_f16_rerank call: gather + chain, select, L2 finish) on the base's own
     candidate ids, ms per batch, and its bytes nq kc D sizeof(T) over that time beside the achievable HBM rate (6.3 TB/s,
     MI355X: 8 TB/s peak); the shipped library and every --variants build (tools/mkvar.sh; e.g. the lane-per-row A/B form,
     -DDENSE_RERANK_LANE_PER_ROW) in this process on alternating passes, with the spread over the passes;
  2. RefineIndex(PQIndex, flat) and RefineIndex(IVFPQIndex, flat) end to end beside the base alone and the flat index alone;
  3. top-10 overlap with the exact flat search of the base alone and of the refined result."""
import argparse
import ctypes as C
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from repconc_amd import _lib, ops  # noqa: E402
from repconc_amd.dense_index import FlatIPIndex, FlatL2F16Index, FlatL2Index  # noqa: E402
from repconc_amd.index import METRIC_INNER_PRODUCT, METRIC_L2, PQIndex  # noqa: E402
from repconc_amd.ivf import IVFPQIndex  # noqa: E402
from repconc_amd.refine_index import RefineIndex  # noqa: E402

DEV = "cuda:0"
HBM_ACHIEVABLE = 6.3e12
NAMES = {METRIC_INNER_PRODUCT: "ip", METRIC_L2: "l2"}


def clustered(n, d, g, chunk=1 << 19):
    centers = torch.randn(64, d, device=DEV, generator=g)
    x = torch.empty((n, d), dtype=torch.float32, device=DEV)
    for r0 in range(0, n, chunk):
        m = min(chunk, n - r0)
        a = torch.randint(0, 64, (m,), device=DEV, generator=g)
        x[r0:r0 + m] = 0.7 * centers[a] + 0.5 * torch.randn(m, d, device=DEV, generator=g)
    return x


def open_lib(path):
    """A second build of the library in this process: (lib, handle) with the entries this tool calls typed."""
    lib = C.CDLL(os.path.abspath(path))
    for name in ("rc_create", "rc_dense_rerank_ws_bytes", "rc_dense_rerank", "rc_dense_f16_rerank"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.PROTOTYPES[name]
    h = C.c_void_p()
    _lib.check(lib.rc_create(C.byref(h), 0), "rc_create")
    return lib, h


def stage_ms(lib, h, x, q, cand, k, metric, reps):
    """ms per call of the re-rank entry of `lib` (device events around `reps` calls on the current stream)."""
    nq, kc = cand.shape
    f16 = x.dtype == torch.float16
    qq = q.to(x.dtype).contiguous()
    fn = lib.rc_dense_f16_rerank if f16 else lib.rc_dense_rerank
    wsb = lib.rc_dense_rerank_ws_bytes(nq, kc)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=DEV)
    scores = torch.empty((nq, k), dtype=torch.float32, device=DEV)
    ids = torch.empty((nq, k), dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        _lib.check(fn(h, p(x), x.stride(0), x.shape[0], x.shape[1], p(qq), nq, p(cand), cand.stride(0), kc, k, 0, metric,
                      p(scores), p(ids), p(ws), wsb, st), "rerank")
    call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        call()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps, scores, ids


def timed(fn, batches):
    """ms per batch of fn(batch) over the batches, results read at the end."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = [fn(qb) for qb in batches]
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / len(batches), out


def overlap10(ids, exact):
    return (ids[:, :10].unsqueeze(2) == exact[:, :10].unsqueeze(1)).any(2).float().mean().item()


def hang(index, store, metric):
    """The flat index `index` over the shared rows `store` (no copy): what its `add` would have left."""
    index._x, index.ntotal = store, store.shape[0]
    if metric == METRIC_L2:
        index._xsq = ops.dense_row_sqnorms(store)
        index._xnorm_max = ops._dense_l2_xnorm_max(index._xsq)
    elif store.dtype == torch.float16:
        index._xnorm_max = ops.dense_f16_xnorm_max(store)
    return index


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8841823)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--m", type=int, default=48)
    ap.add_argument("--batch", type=int, default=1200)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--kc", type=int, default=1000)
    ap.add_argument("--nlist", type=int, default=5000)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--variants", default="", help="name=path.so,... (tools/mkvar.sh builds)")
    a = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(20231)
    x = clustered(a.n, a.d, g)
    x16 = torch.empty((a.n, a.d), dtype=torch.float16, device=DEV)
    for r0 in range(0, a.n, 1 << 20):
        x16[r0:r0 + (1 << 20)] = x[r0:r0 + (1 << 20)].half()
    dsub = a.d // a.m
    rows = x[torch.randperm(a.n, device=DEV, generator=g)[:256]]
    cent = rows.view(256, a.m, dsub).permute(1, 0, 2).contiguous()
    pq = PQIndex(a.d, a.m)
    pq.set_centroids(cent)
    for r0 in range(0, a.n, 1 << 20):
        pq.add(x[r0:r0 + (1 << 20)])
    sel = torch.randperm(a.n, device=DEV, generator=g)[: a.batch * a.batches]
    batches = [x[sel[i * a.batch:(i + 1) * a.batch]] + 0.3 * torch.randn(a.batch, a.d, device=DEV, generator=g)
               for i in range(a.batches)]
    print(f"dense_rerank_bench: N={a.n} D={a.d} M={a.m} k={a.k} kc={a.kc}, {a.batches} batches of {a.batch} queries, {a.passes} "
          f"alternating passes, clustered rows, {torch.cuda.get_device_name(0)}", flush=True)

    # ---- 1. the stage alone -------------------------------------------------------------------------------------------
    libs = [("shipped", _lib.load(), _lib.handle(0))]
    for item in filter(None, a.variants.split(",")):
        name, path = item.split("=", 1)
        libs.append((name,) + open_lib(path))
    stores = {"fp32": x, "fp16": x16}
    for metric in (METRIC_INNER_PRODUCT, METRIC_L2):
        pq.metric_type = metric
        cand = pq.search(batches[0], a.kc)[1].contiguous()
        valid = float((cand >= 0).sum()) / cand.numel()
        print(f"candidates {NAMES[metric]}: {cand.numel()} slots, {torch.unique(cand).numel()} distinct rows (a row that several queries "
              f"name is read from HBM once and from the caches after that: the rate below counts every read)", flush=True)
        for sname, store in stores.items():
            nbytes = a.batch * a.kc * a.d * store.element_size()
            ref = None
            for name, lib, h in libs:                                  # warm every code object, and the outputs must agree
                _, s_, i_ = stage_ms(lib, h, store, batches[0], cand, a.k, metric, 1)
                if ref is None:
                    ref = (s_.clone(), i_.clone())
                elif not (torch.equal(ref[1], i_) and torch.equal(ref[0].view(torch.int32), s_.view(torch.int32))):
                    print(f"  !! {name} differs from shipped ({NAMES[metric]}, {sname})", flush=True)
            ms = {name: [] for name, _, _ in libs}
            for _ in range(a.passes):
                for name, lib, h in libs:
                    ms[name].append(stage_ms(lib, h, store, batches[0], cand, a.k, metric, a.reps)[0])
            for name, _, _ in libs:
                v = ms[name]
                rate = nbytes / (sum(v) / len(v) * 1e-3)
                print(f"stage {NAMES[metric]} {sname} {name:8s}: {sum(v) / len(v):7.3f} ms per batch (min {min(v):.3f} max {max(v):.3f} over "
                      f"{a.passes} passes), {nbytes / 1e9:.2f} GB ({valid:.3f} of the slots valid) -> {rate / 1e12:5.2f} TB/s = "
                      f"{rate / HBM_ACHIEVABLE:.2f} of {HBM_ACHIEVABLE / 1e12:.1f} TB/s achievable HBM", flush=True)

    # ---- 2. / 3. end to end, and what the re-ranking buys ---------------------------------------------------------------
    pq.metric_type = METRIC_INNER_PRODUCT
    ivf = IVFPQIndex.from_flat(pq, a.nlist, x=x)
    ivf.nprobe = a.nprobe
    for metric in (METRIC_INNER_PRODUCT, METRIC_L2):
        pq.metric_type = ivf.metric_type = metric
        for sname, store in stores.items():
            if metric == METRIC_L2:
                flat = hang(FlatL2F16Index(a.d) if sname == "fp16" else FlatL2Index(a.d), store, metric)
            else:
                flat = hang(FlatIPIndex(a.d, storage="float16" if sname == "fp16" else "float32"), store, metric)
            paths = {"flat alone": lambda qb: flat.search(qb, a.k),
                     "pq alone": lambda qb: pq.search(qb, a.k),
                     "pq refined": lambda qb: RefineIndex(pq, flat, a.kc / a.k).search(qb, a.k),
                     "ivf alone": lambda qb: ivf.search(qb, a.k),
                     "ivf refined": lambda qb: RefineIndex(ivf, flat, a.kc / a.k).search(qb, a.k)}
            for fn in paths.values():
                fn(batches[0])
            ms = {n: [] for n in paths}
            out = {}
            for _ in range(a.passes):
                for n, fn in paths.items():
                    t, out[n] = timed(fn, batches)
                    ms[n].append(t)
            exact = torch.cat([o[1] for o in out["flat alone"]])
            for n in paths:
                v = ms[n]
                ids = torch.cat([o[1] for o in out[n]])
                print(f"e2e {NAMES[metric]} {sname} {n:12s}: {sum(v) / len(v):8.3f} ms per batch (min {min(v):.3f} max {max(v):.3f}) = "
                      f"{a.batch / (sum(v) / len(v)):7.1f} k queries/s, top-10 overlap with the exact flat search {overlap10(ids, exact):.3f}",
                      flush=True)
            del flat


if __name__ == "__main__":
    main()
