"""Subset search of the PQ and IVF-PQ indexes: `index.search(x, k, params=SearchParameters(sel=...))` (DESIGN.md 4.6 "Subset
search, PQ").

Contract under test.  Flat: with rows = the selected rows ascending, ns of them, a subset search returns exactly what a PQIndex
with the same centroids, metric and sel_slack that holds codes[rows] returns — ids, score bits, the padding past ns, the counts
of repeated and exact-route queries — with every id i >= 0 replaced by id_offset + rows[i].  IVF: the answer of an IVFPQIndex with
the same coarse table and PQ centroids that holds only the selected vectors in their cells (`set_lists` over them), ids the
original corpus positions, under every method; probing every cell equals the flat subset search.  The selection is built by one
kernel (rc_adc_select_rows) whose image bytes are the existing image builders' for codes[rows], and no other byte.

The references are the library's own materialised indexes and image builders, and `ops.adc_search_exact` over codes[rows] for the
small selections; everything is compared bit for bit, so there is no tolerance anywhere in this file.  Seeded synthetic data."""
import ctypes as C
import functools
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from repconc_amd.selector import (IDSelectorBatch, IDSelectorBitmap, IDSelectorNot, IDSelectorRange, SearchParameters,
                                  SearchParametersIVF)

DEV = "cuda:0"
IP, L2 = 0, 1
D = 768
RC_OK, RC_EINVAL, RC_ESHAPE = 0, -1, -2
IMAGE_M = (16, 32, 48, 64, 96)
LAYOUTS = ("flat", "rows", "rows16")
SCREEN_MIN_N = 1 << 18


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _codes(seed, N, M):
    return torch.randint(0, 256, (N, M), dtype=torch.uint8, generator=_gen(seed))


def _centroids(seed, M):
    """gaussian sub-centroids with norms spread over a factor of 4 per code, so that L2 and inner product rank differently"""
    g = _gen(seed)
    c = torch.randn((M, 256, D // M), generator=g)
    return (c * (0.5 + 1.5 * torch.rand((M, 256, 1), generator=g))).contiguous()


def _queries(seed, nq):
    return torch.randn((nq, D), generator=_gen(seed))


def _sorted_rows(seed, N, ns):
    return torch.sort(torch.randperm(N, generator=_gen(seed))[:ns]).values.contiguous()


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def _same(got, want, what=""):
    assert np.array_equal(_np(got[1]), _np(want[1])), f"ids differ {what}"
    assert np.array_equal(_bits(got[0]), _bits(want[0])), f"score bits differ {what}"


def _pq(codes, cent, metric=IP, id_offset=0, sel_slack=None, device=DEV):
    from repconc_amd.index import PQIndex
    index = PQIndex(D, codes.shape[1], metric=metric, device=device)
    index.set_centroids(cent)
    index.add_codes(codes)
    index.id_offset = id_offset
    if sel_slack is not None:
        index.sel_slack = sel_slack
    return index


def _materialised(index, rows, q, k):
    """What the contract names: the PQIndex that holds codes[rows], its ids mapped; also its repeat / exact-route counts."""
    ref = _pq(index.codes[rows], index._centroids, index.metric_type, 0, index.sel_slack)
    s, i = ref.search(q, k)
    mapped = torch.where(i >= 0, index.id_offset + rows[i.clamp_min(0)], i)
    return (s, mapped), dict(ref.last_search.stats)


def _check_flat(index, rows, q, k, params=None, what=""):
    params = SearchParameters(sel=IDSelectorBatch(rows + index.id_offset)) if params is None else params
    got = index.search(q, k, params=params)
    stats = dict(index.last_search.stats)
    want, want_stats = _materialised(index, rows, q, k)
    _same(got, want, what)
    assert stats == want_stats, (what, stats, want_stats)
    return got, stats


# =============================================================================================================== CPU
def test_params_are_accepted_and_an_empty_index_answers_padding():
    """On the parent commit every call below is a TypeError: PQIndex.search / search_async and IVFPQIndex.search have no params."""
    from repconc_amd.index import PQIndex
    from repconc_amd.ivf import IVFPQIndex
    x = np.zeros((3, D), np.float32)
    sel = SearchParameters(sel=IDSelectorBatch([1, 2]))
    for metric, pad in ((IP, -np.inf), (L2, np.inf)):
        flat = PQIndex(D, 48, metric=metric, device="cpu")
        ivf = IVFPQIndex(D, 48, 8, device="cpu", metric=metric)
        for params in (None, SearchParameters(), sel, SearchParameters(sel=IDSelectorRange(0, 5)),
                       SearchParametersIVF(sel=IDSelectorNot(IDSelectorBatch([0])), nprobe=2)):
            answers = [ivf.search(x, 4, params=params)]
            if params is not None:                       # without params the flat index goes to the library, which has no CPU path
                answers += [flat.search(x, 4, params=params), flat.search_async(x, 4, params=params)(),
                            flat.search_async(x, 4, None, params)()]
                assert flat.last_search.stats == {"retried_queries": 0, "exact_queries": 0}
            for s, i in answers:
                assert isinstance(s, np.ndarray) and s.shape == (3, 4) and i.shape == (3, 4) and i.dtype == np.int64
                assert np.all(s == pad) and np.all(i == -1)
        s, i = flat.search(torch.zeros(2, D), 3, params=sel)                 # tensors in, tensors out
        assert isinstance(s, torch.Tensor) and tuple(s.shape) == (2, 3) and bool((i == -1).all())
        # a bare selector is no SearchParameters
        for call in (lambda: flat.search(x, 4, params=IDSelectorBatch([1])),
                     lambda: flat.search_async(x, 4, params=IDSelectorBatch([1])),
                     lambda: ivf.search(x, 4, params=IDSelectorRange(0, 3)), lambda: ivf.search(x, 4, params={"sel": None})):
            with pytest.raises(ValueError, match="params"):
                call()


def test_an_empty_selection_answers_padding_before_any_device_work():
    """A non-empty index on the CPU (no library call can serve it) and a selector that holds none of its ids."""
    index = _pq(_codes(1, 50, 8), _centroids(2, 8), L2, id_offset=1000, device="cpu")
    for sel in (IDSelectorBatch([3, 7, 999, 1050]), IDSelectorRange(0, 1000), IDSelectorNot(IDSelectorRange(1000, 1050))):
        s, i = index.search(np.zeros((2, D), np.float32), 5, params=SearchParameters(sel=sel))
        assert np.all(s == np.inf) and np.all(i == -1) and s.shape == (2, 5)
        assert sel._adc[0].numel() == 0 and sel._adc[1] is None


def test_row_lists_are_checked_before_any_library_call():
    from repconc_amd import ops
    N, M = 40, 16
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64)
    bad = {
        "unsorted": i64(5, 3, 9), "duplicated": i64(3, 3, 9), "negative": i64(-1, 3, 9), ">= N": i64(3, 9, N),
        "wrong dtype": torch.tensor([1, 2, 3], dtype=torch.int32), "float": torch.tensor([1.0, 2.0, 3.0]),
        "non-contiguous": torch.arange(0, 6, dtype=torch.int64)[::2], "two-dimensional": torch.zeros((3, 1), dtype=torch.int64),
        "more rows than N": torch.arange(0, N + 1, dtype=torch.int64), "a list": [1, 2, 3],
    }
    assert not bad["non-contiguous"].is_contiguous()
    store, cent, q = torch.zeros((N, M), dtype=torch.uint8), torch.zeros(M, 256, D // M), torch.zeros(2, D)
    for what, rows in bad.items():                # CPU tensors throughout: anything that reached the library would raise its own error
        with pytest.raises(ValueError, match="rows"):
            ops.adc_select_rows(store, rows)
        if what == ">= N":                        # a search over a selection knows the selection, not the store it came from
            continue
        sel_codes = torch.zeros((N if what == "more rows than N" else len(rows), M), dtype=torch.uint8)   # N + 1 rows for N codes
        for fn in (ops.adc_search, ops.adc_search_exact):
            with pytest.raises(ValueError, match="rows"):
                fn(sel_codes, cent, q, 1, rows=rows)
    for layout in ("tiles", "", None):
        with pytest.raises(ValueError, match="layout"):
            ops.adc_select_rows(store, i64(1, 2), layout=layout)
    with pytest.raises(ValueError):
        ops.adc_select_rows(store.to(torch.int8), i64(1, 2))
    with pytest.raises(TypeError):                # rows is keyword-only
        ops.adc_search_exact(store, cent, q, 1, 0, IP, i64(1, 2))


def test_new_entries_check_their_arguments_in_the_stated_order():
    from repconc_amd import _lib
    lib = _lib.load()
    z = None
    sel = lambda N=100, M=48, ns=10, layout=0, image=z: lib.rc_adc_select_rows(z, z, N, M, z, ns, layout, z, image, z)
    assert sel() == RC_EINVAL                                                  # fine shapes, no handle, no pointer
    for shape in (dict(N=1 << 32), dict(M=0), dict(M=1025), dict(layout=-1), dict(layout=3), dict(M=24, image=C.c_void_p(64))):
        assert sel(**shape) == RC_ESHAPE, shape
        assert sel(ns=0, **shape) == RC_ESHAPE and sel(ns=101 if "N" not in shape else (1 << 32) + 1, **shape) == RC_ESHAPE
    assert sel(N=(1 << 32) - 1) == RC_EINVAL and sel(M=1024) == RC_EINVAL and sel(layout=2) == RC_EINVAL
    for ns in (0, -1, 101):                                                    # ns outside [1, N], after the shapes
        assert sel(ns=ns) == RC_EINVAL
    assert sel(ns=100) == RC_EINVAL and sel(ns=1) == RC_EINVAL                 # fine ns: the NULL pointers
    assert lib.rc_map_ids(z, z, -1, z, 0, z) == RC_ESHAPE
    assert lib.rc_map_ids(z, z, 5, z, 0, z) == RC_EINVAL and lib.rc_map_ids(z, z, 0, z, 0, z) == RC_EINVAL
    hdr = open(os.path.join(ROOT, "include", "repconc_hip.h")).read()
    for name in ("rc_adc_select_rows", "rc_map_ids"):
        assert name in _lib.PROTOTYPES and re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert len(_lib.PROTOTYPES["rc_adc_select_rows"][1]) == 10 and len(_lib.PROTOTYPES["rc_map_ids"][1]) == 6


def test_signatures_and_the_shim_export_params():
    from repconc_amd import faiss_compat, ops
    from repconc_amd.index import PQIndex
    from repconc_amd.ivf import IVFPQIndex
    from repconc_amd.refine_index import RefineIndex
    for fn in (PQIndex.search, PQIndex.search_async, IVFPQIndex.search):
        assert inspect.signature(fn).parameters["params"].default is None
    assert list(inspect.signature(PQIndex.search_async).parameters)[:5] == ["self", "x", "k", "stats", "params"]
    assert list(inspect.signature(IVFPQIndex.search).parameters) == ["self", "x", "k", "nprobe", "method", "params"]
    for fn in (ops.adc_search, ops.adc_search_exact):
        assert inspect.signature(fn).parameters["rows"].kind is inspect.Parameter.KEYWORD_ONLY
    assert list(inspect.signature(ops.adc_select_rows).parameters) == ["codes", "rows", "layout", "check_rows"]
    assert inspect.signature(faiss_compat.IndexPQ).return_annotation in (PQIndex, "PQIndex")      # IndexPQ(...) is a PQIndex
    assert RefineIndex(PQIndex(D, 48, device="cpu"), _FakeFlat())._base_takes_params
    code = ("import inspect, faiss\n"
            "assert faiss.IndexIVFPQ is faiss.PQIndex if hasattr(faiss, 'PQIndex') else True\n"
            "assert 'params' in inspect.signature(faiss.IndexIVFPQ.search).parameters\n"
            "assert 'params' in inspect.signature(faiss.IndexIVFPQ.search_async).parameters\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "compat"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


class _FakeFlat:
    ntotal, d, metric_type = 0, D, IP

    def rerank(self, x, cand_ids, k):
        raise AssertionError("not reached")


# =============================================================================================================== GPU
BUILD_N = 80000
BUILD_NS = (1, 15, 16, 17, 127, 128, 129, 2047, 2048, 2049, 32767, 32768, 32769, 70001)


def _selections(N, ns, seed):
    """random, the first ns, the last ns, and every third row — the last where 3 ns rows exist (N = 80 000: up to ns = 2 049)"""
    yield "random", _sorted_rows(seed, N, ns)
    yield "first", torch.arange(0, ns, dtype=torch.int64)
    yield "last", torch.arange(N - ns, N, dtype=torch.int64)
    if 3 * ns <= N + 2:
        yield "every third", torch.arange(0, 3 * ns, 3, dtype=torch.int64)


def _written(ops, ns, M, layout):
    """bool mask over the image buffer of ns rows: the bytes the layout's builder writes (a buffer holds whole tiles / chunks)"""
    nbytes = ops.adc_image_bytes(ns, M) if layout == "flat" else ops.adc_image_rows_bytes(ns, M)
    ones = torch.full((ns, M), 255, dtype=torch.uint8, device=DEV)
    return ops.adc_scan_image_(ones, torch.zeros((nbytes,), dtype=torch.uint8, device=DEV), layout=layout) != 0


def _image_pair(ops, store, rows, layout):
    """(the new kernel's codes and whole image buffer, the existing builder's over codes[rows]) — both buffers zero-filled
    first, so a byte written outside the image of ns rows shows."""
    M, ns = store.shape[1], rows.numel()
    want_codes = store[rows].contiguous()
    nbytes = ops.adc_image_bytes(ns, M) if layout == "flat" else ops.adc_image_rows_bytes(ns, M)
    want = ops.adc_scan_image_(want_codes, torch.zeros((nbytes,), dtype=torch.uint8, device=DEV), layout=layout)
    got_codes = torch.zeros((ns, M), dtype=torch.uint8, device=DEV)
    got = torch.zeros((nbytes,), dtype=torch.uint8, device=DEV)
    from repconc_amd import _lib
    lib, h, s, _ = ops._ctx(store)
    rc = lib.rc_adc_select_rows(h, C.c_void_p(store.data_ptr()), store.shape[0], M, C.c_void_p(rows.data_ptr()), ns,
                                ops.ADC_IMAGE_LAYOUTS[layout], C.c_void_p(got_codes.data_ptr()), C.c_void_p(got.data_ptr()), s)
    _lib.check(rc, "rc_adc_select_rows", h)
    return (got_codes, got), (want_codes, want)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M", IMAGE_M)
def test_selection_kernel_writes_the_builders_bytes_and_no_other(M, layout):
    from repconc_amd import ops
    store = _codes(100 + M, BUILD_N, M).to(DEV)
    for ns in BUILD_NS:
        for name, rows in _selections(BUILD_N, ns, seed=ns + M):
            rows = rows.to(DEV)
            (got_codes, got), (want_codes, want) = _image_pair(ops, store, rows, layout)
            assert torch.equal(got_codes, want_codes), (M, layout, ns, name, "codes")
            assert torch.equal(got, want), (M, layout, ns, name, "image")
    # the public wrapper: same bytes over the image of ns rows, buffers of the builders' sizes
    rows = _sorted_rows(9, BUILD_N, 2049).to(DEV)
    sel_codes, sel_image = ops.adc_select_rows(store, rows, layout)
    (_, _), (want_codes, want) = _image_pair(ops, store, rows, layout)
    assert torch.equal(sel_codes, want_codes) and sel_image.numel() == want.numel()
    mask = _written(ops, 2049, M, layout)
    assert int(mask.sum()) == 2049 * M and torch.equal(sel_image[mask], want[mask])


@pytest.mark.gpu
@pytest.mark.parametrize("M", (8, 12, 24, 6))
def test_selection_kernel_compacts_the_codes_of_widths_without_an_image(M):
    from repconc_amd import ops
    store = _codes(200 + M, BUILD_N, M).to(DEV)
    for ns in BUILD_NS:
        for name, rows in _selections(BUILD_N, ns, seed=ns + M):
            rows = rows.to(DEV)
            for layout in LAYOUTS:
                sel_codes, sel_image = ops.adc_select_rows(store, rows, layout)
                assert sel_image is None and torch.equal(sel_codes, store[rows]), (M, ns, name)


@pytest.mark.gpu
@pytest.mark.parametrize("M", (16, 48, 24))
def test_selection_of_a_view_at_a_row_offset(M):
    from repconc_amd import ops
    buf = _codes(300 + M, 5000, M).to(DEV)
    for first in (1, 3, 16, 777):
        store = buf[first:first + 4000]
        assert store.is_contiguous() and store.data_ptr() != buf.data_ptr()
        rows = _sorted_rows(first, 4000, 1234).to(DEV)
        for layout in LAYOUTS:
            sel_codes, sel_image = ops.adc_select_rows(store, rows, layout)
            assert torch.equal(sel_codes, buf[first + rows])
            if sel_image is not None:
                want = ops.adc_scan_image_(buf[first + rows].contiguous(), torch.zeros_like(sel_image), layout=layout)
                mask = _written(ops, 1234, M, layout)
                assert torch.equal(sel_image[mask], want[mask])


# ------------------------------------------------------------------------------------------------------ flat search
FLAT_N = 300000


@functools.lru_cache(maxsize=None)
def _flat_case(M, N=FLAT_N):
    return _codes(400 + M, N, M).to(DEV), _centroids(500 + M, M).to(DEV), _queries(600 + M, 130).to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", (IP, L2))
@pytest.mark.parametrize("ns", (262143, 262144, 262145, 264209))
def test_flat_subset_search_around_the_screen_threshold(ns, metric):
    """ns straddles ADC_SCREEN_MIN_N = 2^18 (the route follows ns, not ntotal = 300 000): the filter scan below it, the screen at
    a whole-tile count, one row past it, and with a partial 2 048-row round."""
    codes, cent, q = _flat_case(16)
    assert ns <= FLAT_N and (262144 % 32768, 264209 % 2048) == (0, 17)
    index = _pq(codes, cent, metric, id_offset=7000)
    rows = _sorted_rows(ns, FLAT_N, ns).to(DEV)
    _check_flat(index, rows, q[:17], 10, what=f"ns {ns}")


@pytest.mark.gpu
@pytest.mark.parametrize("M,ns", [(48, 270001), (96, 266000), (24, 263000), (6, 40000), (12, 5000), (64, 19999)])
def test_flat_subset_search_at_every_kind_of_width(M, ns):
    """48 and 96 above 2^18: the phases, and the 48-wide phase pair of M = 96; 24: the round-1 screen on the compact codes; 6:
    the run-time-width scan; small selections also against the exact route over codes[rows]."""
    from repconc_amd import ops
    codes, cent, q = _flat_case(M, 280000 if ns > 100000 else 50000)
    N = codes.shape[0]
    for metric in (IP, L2):
        index = _pq(codes, cent, metric, id_offset=11)
        rows = _sorted_rows(M, N, ns).to(DEV)
        got, _ = _check_flat(index, rows, q[:9], 20, what=f"M {M} metric {metric}")
        if ns <= 20000:
            s, i = ops.adc_search_exact(codes[rows].contiguous(), cent, q[:9], 20, metric=metric)
            _same(got, (s, torch.where(i >= 0, 11 + rows[i.clamp_min(0)], i)), "against the exact route")
            _same(ops.adc_search_exact(codes[rows].contiguous(), cent, q[:9], 20, 11, metric, rows=rows), got, "rows= exact")


@pytest.mark.gpu
def test_flat_subset_search_edges_of_k_nq_and_ns():
    from repconc_amd import ops
    from oracle import c_oracle
    codes, cent, q = _flat_case(16)
    index = _pq(codes, cent, IP, id_offset=5)
    small = _sorted_rows(1, FLAT_N, 12000).to(DEV)
    for nq in (1, 17, 130):
        for k in (1, 1000):
            got, _ = _check_flat(index, small, q[:nq], k, what=f"nq {nq} k {k}")
    # ... and the C oracle over codes[rows]
    ws, wi = c_oracle.adc_search(_np(codes[small]), _np(cent), _np(q[:17]), 10)
    got = index.search(q[:17], 10, params=SearchParameters(sel=IDSelectorBatch(small + 5)))
    _same(got, (ws, 5 + _np(small)[wi]), "C oracle")
    # ns < k and ns = 1: padding past ns, under both metrics
    for metric, pad in ((IP, -np.inf), (L2, np.inf)):
        index = _pq(codes, cent, metric, id_offset=5)
        for ns in (1, 7):
            rows = _sorted_rows(ns + 40, FLAT_N, ns).to(DEV)
            (s, i), _ = _check_flat(index, rows, q[:3], 10)
            assert bool((i[:, ns:] == -1).all()) and bool((s[:, ns:] == pad).all()) and bool((i[:, :ns] >= 5).all())
            assert sorted(i[0, :ns].tolist()) == (rows + 5).tolist()
    # the identity: every row selected -> the plain search, with the index's own buffers (nothing compacted)
    everything = IDSelectorRange(0, 1 << 40)
    _same(index.search(q[:17], 10, params=SearchParameters(sel=everything)), index.search(q[:17], 10), "identity")
    assert everything._adc[1] is None and everything._adc[2] is None and everything._adc[0].numel() == FLAT_N
    _same(index.search(q[:17], 10, params=SearchParameters()), index.search(q[:17], 10), "no selector")
    # ops level: adc_search(rows=) over a selection maps once, deferred or not
    sel_codes, sel_image = ops.adc_select_rows(codes, small)
    want, _ = _materialised(index, small, q[:17], 10)
    _same(ops.adc_search(sel_codes, cent, q[:17], 10, id_offset=5, scan_image=sel_image, metric=L2, rows=small), want)
    pending = ops.adc_search(sel_codes, cent, q[:17], 10, id_offset=5, scan_image=sel_image, metric=L2, rows=small, defer=True)
    _same(pending.result(), want)
    _same(pending.result(), want, "a second result() maps nothing again")


@pytest.mark.gpu
def test_flat_subset_search_numpy_and_two_batches_in_flight():
    codes, cent, q = _flat_case(16)
    index = _pq(codes, cent, L2, id_offset=100)
    rows = _sorted_rows(77, FLAT_N, 263000).to(DEV)
    params = SearchParameters(sel=IDSelectorBatch(_np(rows) + 100))
    want_a, _ = _materialised(index, rows, q[:17], 10)
    want_b, _ = _materialised(index, rows, q[17:60], 10)
    s, i = index.search(_np(q[:17]), 10, params=params)
    assert isinstance(s, np.ndarray) and isinstance(i, np.ndarray)
    _same((s, i), want_a, "numpy")
    first = index.search_async(q[:17], 10, params=params)           # both enqueued before either is resolved
    second = index.search_async(q[17:60], 10, None, params)
    _same(second(), want_b, "second batch")
    _same(first(), want_a, "first batch")


# ------------------------------------------------------------------------------------------------------ repair paths
def _best_code(ops, cent, q0, metric):
    """the code row with the best possible score for query q0: per sub-quantiser the entry the tables rank first"""
    return ops.adc_lut(cent, q0[None], metric)[0].argmax(dim=1).to(torch.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", (IP, L2))
def test_a_lowered_sel_slack_repeats_queries_and_maps_once(metric):
    codes, cent, q = _flat_case(16)
    index = _pq(codes, cent, metric, id_offset=3)
    rows = _sorted_rows(5, FLAT_N, 264209).to(DEV)
    index.sel_slack = -50.0
    got, stats = _check_flat(index, rows, q[:17], 100, what="sel_slack -50")
    assert stats["retried_queries"] > 0
    index.sel_slack = 3.0
    _same(got, index.search(q[:17], 100, params=SearchParameters(sel=IDSelectorBatch(rows + 3))), "the default slack")
    assert bool((got[1] >= 3).all()) and bool(torch.isin(got[1] - 3, rows).all())


@pytest.mark.gpu
@pytest.mark.parametrize("metric", (IP, L2))
def test_identical_rows_go_to_the_exact_route_and_ties_follow_the_corpus_id(metric):
    from repconc_amd import ops
    codes, cent, q = _flat_case(16)
    codes = codes[:90000].clone()
    dup_rows = torch.arange(1000, 1000 + 3 * 17000, 3, device=DEV)                   # 17 000 > 16 384 copies, every third row
    codes[dup_rows] = _best_code(ops, cent, q[0], metric)
    index = _pq(codes, cent, metric, id_offset=50)
    others = torch.arange(2, 90000, 3, device=DEV)[:20000]
    rows = torch.sort(torch.cat([dup_rows[200:], others])).values.contiguous()       # the 200 lowest copies stay outside
    (s, i), stats = _check_flat(index, rows, q[:5], 300, what="identical rows")
    assert stats["exact_queries"] >= 1
    assert i[0].tolist() == (50 + dup_rows[200:500]).tolist()                        # equal scores: ascending corpus ids
    assert len(set(_bits(s[0]).tolist())) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,ns", [(16, FLAT_N, 264000), (48, 60000, 20000)])
def test_rows_outside_the_selection_never_come_back(M, N, ns):
    """Rows with the best score the tables allow sit in the store, next to selected rows, outside the selection."""
    from repconc_amd import ops
    codes, cent, q = _flat_case(M, N)
    for metric in (IP, L2):
        rows = _sorted_rows(M, N, ns).to(DEV)
        outside = torch.ones(N, dtype=torch.bool, device=DEV)
        outside[rows] = False
        planted = torch.nonzero(outside).flatten()[::7][:500]
        store = codes.clone()
        store[planted] = _best_code(ops, cent, q[0], metric)
        index = _pq(store, cent, metric)
        plain = index.search(q[:1], 10)
        assert bool(torch.isin(plain[1], planted).all())                             # the plain search does find them
        (s, i), _ = _check_flat(index, rows, q[:9], 50, what="planted rows")
        assert not bool(torch.isin(i, planted).any()) and bool(torch.isin(i, rows).all())


# ------------------------------------------------------------------------------------------------------ selectors
@pytest.mark.gpu
def test_every_selector_kind_and_the_cache():
    N, M = 30000, 16
    codes, cent, q = _flat_case(M, 50000)
    index = _pq(codes[:N], cent, IP, id_offset=1000)
    q = q[:9]
    ids = _np(_sorted_rows(3, N, 4000)) + 1000
    bits = np.zeros(((N + 1000) // 8 + 1,), np.uint8)
    np.bitwise_or.at(bits, ids >> 3, (1 << (ids & 7)).astype(np.uint8))
    with_strangers = np.concatenate([ids[::-1], ids[:10], [-5, 0, 999, N + 1000, N + 5000]])   # unsorted, repeated, outside
    cases = [(IDSelectorRange(900, 6000), np.arange(0, 5000)), (IDSelectorRange(20000, 10 ** 9), np.arange(19000, N)),
             (IDSelectorBatch(with_strangers), ids - 1000), (IDSelectorBitmap(bits), ids - 1000),
             (IDSelectorNot(IDSelectorBatch(ids)), np.setdiff1d(np.arange(N), ids - 1000)),
             (IDSelectorNot(IDSelectorRange(3000, N + 1000 - 7)), np.concatenate([np.arange(0, 2000), np.arange(N - 7, N)]))]
    for sel, rows in cases:
        rows = torch.from_numpy(rows.astype(np.int64)).to(DEV)
        _check_flat(index, rows, q, 10, SearchParameters(sel=sel), what=type(sel).__name__)
        assert torch.equal(sel._adc[0], rows) and torch.equal(sel._adc[1], index.codes[rows])
    # one entry, kept across searches and across set_centroids, rebuilt after add_codes
    sel, rows = cases[2]
    rows = torch.from_numpy(rows.astype(np.int64)).to(DEV)
    params = SearchParameters(sel=sel)
    held = sel._adc
    index.search(q, 10, params=params)
    assert sel._adc is held
    index.set_centroids(_centroids(77, M).to(DEV))
    _check_flat(index, rows, q, 10, params, what="new centroids")
    assert sel._adc is held
    sel2 = IDSelectorRange(0, 10 ** 9)
    index.search(q, 10, params=SearchParameters(sel=sel2))
    index.add_codes(codes[N:N + 500])
    grown = IDSelectorNot(IDSelectorRange(1000 + 100, 1000 + N))                     # rows 0 .. 99 and the 500 new ones
    grown_rows = torch.cat([torch.arange(0, 100), torch.arange(N, N + 500)]).to(DEV)
    _check_flat(index, grown_rows, q, 10, SearchParameters(sel=grown), what="after add_codes")
    _check_flat(index, rows, q, 10, params, what="the old selector after add_codes")
    assert sel._adc is not held
    _same(index.search(q, 10, params=SearchParameters(sel=sel2)), index.search(q, 10), "identity after add_codes")
    assert sel2._adc[0].numel() == N + 500
    # an index and an IVF index may take turns on one selector: each builds its own selection again
    other = _pq(codes[:N], cent, IP, id_offset=1000)
    _check_flat(other, rows, q, 10, params, what="another index")
    _check_flat(index, rows, q, 10, params, what="back")


# ------------------------------------------------------------------------------------------------------ IVF
IVF_N, NLIST = 60000, 64
METHODS = ("auto", "lists", "lists8", "lists16", "lists_host_plan", "scan")


@functools.lru_cache(maxsize=None)
def _ivf_case(M):
    codes = _codes(700 + M, IVF_N, M).to(DEV)
    cells = torch.randint(0, NLIST, (IVF_N,), generator=_gen(800 + M)).to(DEV)
    coarse = torch.randn((NLIST, D), generator=_gen(900 + M)).to(DEV)
    return codes, cells, coarse, _centroids(1000 + M, M).to(DEV), _queries(1100 + M, 9).to(DEV)


def _ivf(codes, cells, coarse, cent, metric):
    from repconc_amd.ivf import IVFPQIndex
    index = IVFPQIndex(D, codes.shape[1], NLIST, device=DEV, metric=metric)
    index.coarse = coarse
    index.set_centroids(cent)
    index.set_lists(codes, cells)
    return index


def _ivf_selection(name, cells):
    if name == "empties cells":                   # nothing of cells 0 .. 19, half of the others
        keep = (cells >= 20) & (torch.arange(IVF_N, device=DEV) % 2 == 0)
        return IDSelectorBatch(torch.nonzero(keep).flatten().cpu()), torch.nonzero(keep).flatten()
    if name == "one cell":
        rows = torch.nonzero(cells == 37).flatten()[5:400]
        return IDSelectorBatch(rows.cpu().numpy()[::-1].copy()), rows
    if name == "ten percent":
        rows = _sorted_rows(4, IVF_N, IVF_N // 10).to(DEV)
        return IDSelectorBatch(rows), rows
    rows = torch.cat([torch.arange(0, 1000), torch.arange(50000, IVF_N)]).to(DEV)
    return IDSelectorNot(IDSelectorRange(1000, 50000)), rows


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("empties cells", "one cell", "ten percent", "complement of a range"))
@pytest.mark.parametrize("metric", (IP, L2))
@pytest.mark.parametrize("M", (16, 96))
def test_ivf_subset_search_equals_the_index_of_the_selected_rows(M, metric, name):
    codes, cells, coarse, cent, q = _ivf_case(M)
    index = _ivf(codes, cells, coarse, cent, metric)
    sel, rows = _ivf_selection(name, cells)
    ref = _ivf(codes[rows], cells[rows], coarse, cent, metric)
    flat = _pq(codes, cent, metric)
    k = 10
    for nprobe in (1, 4, NLIST):
        want = None
        for method in METHODS:
            s, i = ref.search(q, k, nprobe, method)
            mapped = torch.where(i >= 0, rows[i.clamp_min(0)], i)
            got = index.search(q, k, nprobe, method, params=SearchParameters(sel=sel))
            _same(got, (s, mapped), f"{name} nprobe {nprobe} {method}")
            if want is not None:
                _same(got, want, f"{method} against the other methods")
            want = got
        sub = sel._adc                             # the selection: the index of the selected rows, ids the corpus positions
        assert sub is not index and sub.ntotal == rows.numel() and torch.equal(sub.ids, index.ids[torch.isin(index.ids, rows)])
        if nprobe == NLIST:                        # (the flat index takes the selector's one cache entry over)
            _same(want, flat.search(q, k, params=SearchParameters(sel=sel)), "every cell probed: the flat subset search")
    assert bool(torch.isin(want[1], rows).all())


@pytest.mark.gpu
def test_ivf_nprobe_precedence_numpy_and_the_edges():
    codes, cells, coarse, cent, q = _ivf_case(16)
    index = _ivf(codes, cells, coarse, cent, IP)
    sel, rows = _ivf_selection("ten percent", cells)
    index.nprobe = 2
    at = lambda n: index.search(q, 10, n, params=SearchParameters(sel=sel))
    _same(index.search(q, 10, params=SearchParameters(sel=sel)), at(2), "the attribute")
    _same(index.search(q, 10, params=SearchParametersIVF(sel=sel, nprobe=5)), at(5), "params.nprobe over the attribute")
    _same(index.search(q, 10, 3, params=SearchParametersIVF(sel=sel, nprobe=5)), at(3), "the argument over params.nprobe")
    _same(index.search(q, 10, params=SearchParametersIVF(sel=sel)), at(2), "no nprobe in params")
    assert not np.array_equal(_np(at(2)[1]), _np(at(5)[1]))
    _same(index.search(q, 10, params=SearchParametersIVF(nprobe=5)), index.search(q, 10, 5), "nprobe without a selector")
    s, i = index.search(_np(q), 10, 4, params=SearchParameters(sel=sel))
    assert isinstance(s, np.ndarray)
    _same((s, i), at(4), "numpy")
    # everything selected: the index itself; nothing selected, or no query: padding
    everything = IDSelectorRange(0, IVF_N)
    _same(index.search(q, 10, 4, params=SearchParameters(sel=everything)), index.search(q, 10, 4), "identity")
    assert everything._adc is index
    for metric, pad in ((IP, -np.inf), (L2, np.inf)):
        index = _ivf(codes, cells, coarse, cent, metric)
        s, i = index.search(q, 10, 4, params=SearchParameters(sel=IDSelectorRange(IVF_N, IVF_N + 9)))
        assert bool((s == pad).all()) and bool((i == -1).all()) and tuple(s.shape) == (9, 10)
        s, i = index.search(q[:0], 10, 4, params=SearchParameters(sel=sel))
        assert tuple(s.shape) == (0, 10) and tuple(i.shape) == (0, 10)
        # a selection smaller than k
        few = torch.tensor([5, 17, 40000], device=DEV)
        s, i = index.search(q, 10, NLIST, params=SearchParameters(sel=IDSelectorBatch(few)))
        assert bool((i[:, 3:] == -1).all()) and bool((s[:, 3:] == pad).all()) and sorted(i[0, :3].tolist()) == few.tolist()
    # set_lists builds the selection again
    index.search(q, 10, 4, params=SearchParameters(sel=sel))
    held = sel._adc
    index.search(q, 10, 4, params=SearchParameters(sel=sel))
    assert sel._adc is held
    index.set_lists(codes, (cells + 1) % NLIST)
    index.search(q, 10, 4, params=SearchParameters(sel=sel))
    assert sel._adc is not held and sel._adc.ntotal == held.ntotal


# ------------------------------------------------------------------------------------------------------ RefineIndex
@pytest.mark.gpu
@pytest.mark.parametrize("base_kind", ("pq", "ivfpq"))
def test_refine_index_over_a_pq_base_takes_params(base_kind):
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatIPIndex
    from repconc_amd.ivf import coarse_assign
    from repconc_amd.refine_index import RefineIndex
    N, M = 20000, 16
    x = torch.randn((N, D), generator=_gen(21)).to(DEV)
    cent = _centroids(22, M).to(DEV)
    q = _queries(23, 9).to(DEV)
    flat = FlatIPIndex(D, device=DEV)
    flat.add(x)
    codes = ops.assign_nearest(x, cent, torch.uint8)
    if base_kind == "pq":
        base, extra = _pq(codes, cent, IP), {}
    else:
        coarse = x[:NLIST].clone()
        base, extra = _ivf(codes, coarse_assign(x, coarse), coarse, cent, IP), {"nprobe": NLIST}
    refine = RefineIndex(base, flat, k_factor=8)
    rows = _sorted_rows(24, N, 80).to(DEV)
    params = SearchParameters(sel=IDSelectorBatch(rows))
    s, i = refine.search(q, 10, params=params, **extra)                     # kc = 80 covers the selection
    _same((s, i), flat.search(q, 10, params=params), "k_factor covers the selection: the flat subset search")
    wide = _sorted_rows(25, N, 5000).to(DEV)
    s, i = refine.search(q, 10, params=SearchParameters(sel=IDSelectorBatch(wide)), **extra)
    assert bool(torch.isin(i, wide).all()) and bool((i >= 0).all())
