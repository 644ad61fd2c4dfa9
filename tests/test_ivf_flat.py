"""Exact IVF search over dense vectors: csrc/ivf_flat.hip (rc_ivf_flat_search / rc_ivf_flat_f16_search), ops.ivf_flat_search,
ivf_flat.IVFFlatIndex, faiss_compat.IndexIVFFlat, create_index(nlist=...).

Oracles, none of them the code under test:
  (a) the emulated chain of tests/test_dense_flat.py (inner product) and tests/test_dense_l2.py (L2) over the rows of the probed
      cells, sorted by (score, corpus id) and cut / padded like tests/test_dense_rerank.py cuts — about 0.1 us per pair and
      dimension, so it is used at small D x rows x queries;
  (b) the flat indexes of dense_index and their `rerank` (ops.dense_rerank) on the same device, for D = 768 and D = 100.
Ids and score BITS are compared (assert_matches).  fp16 storage: the chain over x.half().float(), q.half().float()."""
import functools

import numpy as np
import pytest

from test_dense_flat import assert_matches, chain_scores, fmaf_emul  # noqa: F401  (fmaf_emul: the oracle's arithmetic)
from test_dense_l2 import chain_l2
from test_dense_rerank import cut

IP, L2 = 0, 1
METRICS = (IP, L2)
STORAGES = ("float32", "float16")
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------------------ helpers
def _randn(shape, seed, dev=DEV):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev, dtype=torch.float32)


def _values(t, storage):
    """The values a store of this type holds for t (and a search uses for queries t), as fp32 numpy."""
    import torch
    return (t.to(torch.float16).float() if storage == "float16" else t.float()).cpu().numpy()


def oracle_probed(xn, qn, cells, probes, metric):
    """(a): xn [N, D], qn [nq, D] fp32 numpy, cells [N] the cell of every corpus row, probes [nq, nprobe] -> per query the
    (scores, ids) of the rows of its probed cells in the search's order."""
    out = []
    for j in range(qn.shape[0]):
        ids = np.nonzero(np.isin(cells, probes[j]))[0].astype(np.int64)
        s = (chain_l2 if metric == L2 else chain_scores)(np.repeat(qn[j:j + 1], len(ids), 0), xn[ids]) if len(ids) \
            else np.zeros(0, np.float32)
        order = np.lexsort((ids, s.astype(np.float64) if metric == L2 else -s.astype(np.float64)))
        out.append((s[order], ids[order]))
    return out


def _flat(metric, storage, d):
    from repconc_amd.dense_index import FlatIPIndex, FlatL2F16Index, FlatL2Index
    if metric == L2:
        return (FlatL2F16Index if storage == "float16" else FlatL2Index)(d, device=DEV)
    return FlatIPIndex(d, device=DEV, storage=storage)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


# --------------------------------------------------------------------------------------------------------------- CPU
def test_ivf_flat_workspace_helper_needs_no_gpu():
    from repconc_amd import _lib, ops
    lib = _lib.load()
    for nq, nprobe, nlist, stride in ((1, 1, 1, 1), (7, 2, 12, 2567), (1200, 32, 5000, 160000), (50, 64, 64, 20000)):
        w = lib.rc_ivf_flat_search_ws_bytes(nq, nprobe, nlist, stride)
        assert w > 0 and w % 256 == 0 and w >= nq * (8 * stride + 16384 * 8)
        assert ops.ivf_flat_search_ws_bytes(nq, nprobe, nlist, stride) == w
    for bad in ((0, 4, 8, 100), (-1, 4, 8, 100), (5, 0, 8, 100), (5, -2, 8, 100), (5, 9, 8, 100), (5, 4, 8, 0), (5, 4, 8, -7)):
        assert lib.rc_ivf_flat_search_ws_bytes(*bad) == 0, bad
    w = [lib.rc_ivf_flat_search_ws_bytes(nq, 8, 64, 4096) for nq in (1, 2, 3, 50, 51, 1200)]
    assert w == sorted(w) and w[0] < w[-1]                                  # monotone in nq
    w = [lib.rc_ivf_flat_search_ws_bytes(50, 8, 64, s) for s in (1, 2, 63, 64, 65, 4096, 100000)]
    assert w == sorted(w) and w[0] < w[-1]                                  # ... and in stride
    assert ops.ivf_flat_query_group() == lib.rc_ivf_flat_query_group() and ops.ivf_flat_query_group() in (8, 16)


def test_ivf_flat_argument_errors_are_value_errors_with_cpu_tensors_only():
    import torch
    from repconc_amd.index import METRIC_INNER_PRODUCT
    from repconc_amd.ivf_flat import IVFFlatIndex
    with pytest.raises(ValueError, match="metric"):
        IVFFlatIndex(8, 4, device="cpu", metric=2)
    with pytest.raises(ValueError, match="storage"):
        IVFFlatIndex(8, 4, device="cpu", storage="bfloat16")
    with pytest.raises(ValueError, match="nlist"):
        IVFFlatIndex(8, 16385, device="cpu")
    index = IVFFlatIndex(8, 4, device="cpu")
    assert index.metric_type == METRIC_INNER_PRODUCT and index.nprobe == 8 and index.ntotal == 0 and not index.is_trained
    assert index.coarse is None and index.MAX_WS_BYTES == 4 << 30
    q = torch.zeros(3, 8)
    with pytest.raises(ValueError, match="train"):
        index.search(q, 5)                                                  # search before train
    with pytest.raises(ValueError, match="train"):
        index.add(torch.zeros(5, 8))
    with pytest.raises(ValueError, match="centroids"):
        index.set_coarse(torch.zeros(5, 8))
    index.set_coarse(torch.zeros(4, 8))
    assert index.is_trained
    for k in (0, -1, 8193):
        with pytest.raises(ValueError, match="k must be"):
            index.search(q, k)
        with pytest.raises(ValueError, match="k must be"):
            index._search_probes(q, torch.zeros(3, 1, dtype=torch.int32), k)
    with pytest.raises(ValueError, match="queries"):
        index.search(torch.zeros(3, 9), 5)                                  # D mismatch
    with pytest.raises(ValueError, match="vectors"):
        index.add(torch.zeros(5, 7))
    with pytest.raises(ValueError, match="vectors"):
        index.set_lists(torch.zeros(5, 9), torch.zeros(5, dtype=torch.int64))
    for cells in ([0, 1, 2, 3, 4], [0, 1, -1, 3, 2]):
        with pytest.raises(ValueError, match="cells must lie"):
            index.set_lists(torch.zeros(5, 8), torch.tensor(cells))
    with pytest.raises(ValueError, match="integer cells"):
        index.set_lists(torch.zeros(5, 8), torch.zeros(4, dtype=torch.int64))
    for probes in ([[0, 4]] * 3, [[1, 1]] * 3, [[-1, 2]] * 3):
        with pytest.raises(ValueError, match="distinct cells"):
            index._search_probes(q, torch.tensor(probes, dtype=torch.int32), 5)
    with pytest.raises(ValueError, match="probes"):
        index._search_probes(q, torch.zeros(2, 2, dtype=torch.int32), 5)
    assert index.ntotal == 0
    # an empty index and an empty query set answer without a launch: all padding
    s, i = index.search(q, 4)
    assert s.shape == (3, 4) and bool((s == float("-inf")).all()) and bool((i == -1).all())
    s, i = index.search(torch.zeros(0, 8), 4)
    assert s.shape == (0, 4) and i.shape == (0, 4)
    assert index.last_search_stats == {"queries": 0, "fallback_queries": 0, "chunks": 0}


def test_check_index_options_keeps_three_arguments_and_refuses_bf16x3_with_cells():
    from repconc_amd.models.dense.evaluate_dense import check_index_options
    for metric in ("ip", "l2"):
        check_index_options(metric, False, "fp32")
        check_index_options(metric, True, "fp32")
        check_index_options(metric, False, "bf16x3")
        check_index_options(metric, False, "fp32", 64)
        check_index_options(metric, True, "fp32", nlist=64)
        with pytest.raises(ValueError, match="bf16x3"):
            check_index_options(metric, False, "bf16x3", 64)
        with pytest.raises(ValueError, match="nlist"):
            check_index_options(metric, False, "fp32", -1)


def test_shim_exports_indexivfflat():
    import sys
    import os
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import faiss
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))
    import repconc_amd.faiss_compat as fc
    from repconc_amd.ivf_flat import IVFFlatIndex
    assert faiss.IndexIVFFlat is fc.IndexIVFFlat and issubclass(fc.IndexIVFFlat, IVFFlatIndex)
    with pytest.raises(ValueError, match="metric"):
        fc.IndexIVFFlat(None, 8, 4, 7)


# --------------------------------------------------------------------------------------------------------------- GPU
CELL_SIZES = [0, 1, 127, 128, 129, 0, 700, 15, 16, 17, 0]           # + the rest of the N = 3000 rows in cell 11


@functools.lru_cache(maxsize=None)
def _constructed(D):
    """N = 3000 rows in 12 cells of the sizes above under shuffled corpus ids, and 43 queries: 40 probing cells 6 + 4 (700 + 129
    rows), one probing the empty cells 0 + 5, one the 1-row cell 1 + the empty cell 10, one cells 11 + 2 (1867 + 127 rows:
    four row chunks of the scan)."""
    import torch
    N = 3000
    sizes = CELL_SIZES + [N - sum(CELL_SIZES)]
    rng = np.random.default_rng(100 + D)
    cells = np.repeat(np.arange(12), sizes)[rng.permutation(N)]         # cells[i]: the cell of corpus row i
    x, q = _randn((N, D), 7 + D), _randn((43, D), 8 + D)
    probes = np.array([[6, 4]] * 40 + [[0, 5], [1, 10], [11, 2]], dtype=np.int32)
    return x, q, torch.from_numpy(cells), cells, probes


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", (1, 5, 16, 40))
def test_constructed_cells_match_the_emulated_chain(D, metric, storage):
    import torch
    from repconc_amd import ops
    from repconc_amd.ivf_flat import IVFFlatIndex
    x, q, cells_t, cells, probes = _constructed(D)
    index = IVFFlatIndex(D, 12, device=DEV, metric=metric, storage=storage)
    index.set_coarse(torch.zeros(12, D))
    index.set_lists(x, cells_t)
    assert index.ntotal == 3000 and index.list_off.tolist() == np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=12))]).tolist()
    want = oracle_probed(_values(x, storage), _values(q, storage), cells, probes, metric)
    pt = torch.from_numpy(probes).to(DEV)
    QG = ops.ivf_flat_query_group()                 # the kernel's own group width, from the library
    for k in (1, 10, 829, 2000):
        for nq in (1, QG, QG + 1, 2 * QG + 3, 43):
            sel = np.arange(nq) if nq < 43 else np.arange(43)
            got = index._search_probes(q[:nq], pt[:nq], k)
            assert_matches(got, cut([want[j] for j in sel], k, metric))
            assert index.last_search_stats == {"queries": nq, "fallback_queries": 0, "chunks": 1}
        # the special queries alone, and in the other order of their probes
        got = index._search_probes(q[40:], pt[40:].flip(1), k)
        assert_matches(got, cut(want[40:], k, metric))
        assert index.last_search_stats["fallback_queries"] == 0
    s, i = index._search_probes(q[40:42], pt[40:42], 10)
    pad = float("inf") if metric == L2 else float("-inf")
    assert bool((s[0] == pad).all()) and bool((i[0] == -1).all())           # only empty cells: all padding
    assert int(i[1, 0]) == int(np.nonzero(cells == 1)[0][0]) and bool((i[1, 1:] == -1).all()) and bool((s[1, 1:] == pad).all())


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_a_cell_longer_than_the_scan_grid_is_walked_by_striding_blocks(metric, storage):
    """One cell of 5000 rows: more row chunks than the scan deals blocks to (8 x 512 rows), so a block takes a second chunk."""
    import torch
    from repconc_amd.ivf_flat import IVFFlatIndex
    D, N = 5, 5300
    x, q = _randn((N, D), 31), _randn((3, D), 32)
    cells = np.where(np.arange(N) % 53 == 0, 0, np.where(np.arange(N) % 53 == 1, 2, 1))
    index = IVFFlatIndex(D, 3, device=DEV, metric=metric, storage=storage)
    index.set_coarse(torch.zeros(3, D))
    index.set_lists(x, torch.from_numpy(cells))
    probes = np.array([[1, 2], [0, 1], [0, 2]], dtype=np.int32)
    want = oracle_probed(_values(x, storage), _values(q, storage), cells, probes, metric)
    for k in (7, 5200):
        assert_matches(index._search_probes(q, torch.from_numpy(probes), k), cut(want, k, metric))
    assert index.last_search_stats["fallback_queries"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
def test_a_probe_outside_the_index_or_a_short_score_row_sets_status_bit_2(storage):
    """What the header promises a direct caller of the ABI (the index validates its probes, so ops.ivf_flat_search is the way
    in): a probe outside [0, nlist) — the -1 padding of a probe row, or nlist itself — and a `stride` below the rows the probes
    hold are skipped / clipped on the device and reported in status bit 2; the call returns, a valid call afterwards is exact."""
    import torch
    from repconc_amd import ops
    from repconc_amd.ivf_flat import IVFFlatIndex
    D, N, k = 16, 1500, 10
    x, q = _randn((N, D), 111), _randn((9, D), 112)
    cells = np.random.default_rng(8).integers(0, 4, N)
    index = IVFFlatIndex(D, 4, device=DEV, storage=storage)
    index.set_coarse(torch.zeros(4, D))
    index.set_lists(x, torch.from_numpy(cells))
    good = np.array([[1, 3]] * 9, dtype=np.int32)
    full = (int(np.bincount(cells).max()) * 2 + 3) // 4 * 4
    for probes, stride in (([[-1, 3]] * 9, full), ([[1, 4]] * 9, full), ([[1, 3]] * 4 + [[-1, 2]] + [[1, 3]] * 4, full),
                           (good.tolist(), 400), (good.tolist(), 100)):
        pt = torch.tensor(probes, dtype=torch.int32, device=DEV)
        _, _, status, _ = ops.ivf_flat_search(index.xb, index.list_off, index.ids, q, pt, stride, k)
        assert int(status.item()) & 4, (probes[4], stride)
    want = oracle_probed(_values(x, storage), _values(q, storage), cells, good, IP)
    s, i, status, qstatus = ops.ivf_flat_search(index.xb, index.list_off, index.ids, q, torch.from_numpy(good).to(DEV), full, k)
    assert int(status.item()) == 0 and not bool(qstatus.any())
    assert_matches((s, i), cut(want, k, IP))


@functools.lru_cache(maxsize=None)
def _corpus(N, D, nq, seed):
    return _randn((N, D), seed), _randn((nq, D), seed + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", (768, 100))
def test_probing_every_cell_equals_the_flat_index(D, metric, storage):
    """D = 768: 16-byte aligned rows; D = 100: fp32 rows are aligned, fp16 rows (200 bytes) are not: the element-wise path."""
    import torch
    from repconc_amd.ivf_flat import IVFFlatIndex
    x, q = _corpus(20000, D, 33, 40 + D)
    index = IVFFlatIndex(D, 64, device=DEV, metric=metric, storage=storage)
    index.train(x)
    index.add(x)
    assert index.ntotal == 20000 and index.is_trained
    flat = _flat(metric, storage, D)
    flat.add(x)
    for k in (1, 100, 1000):
        ws, wi = flat.search(q, k)
        got = index.search(q, k, nprobe=64)
        assert_matches(got, (ws.cpu().numpy(), wi.cpu().numpy()))
        assert index.last_search_stats == {"queries": 33, "fallback_queries": 0, "chunks": 1}
        assert_matches(index.search(q, k, nprobe=1000), (ws.cpu().numpy(), wi.cpu().numpy()))      # nprobe is clipped to nlist
    # nprobe = 5 against the flat index's own re-ranking of the ids of the probed cells
    probes = index.probe(q, 5, ordered=False).cpu().numpy()
    cells = np.empty(20000, np.int64)
    cells[index.ids.cpu().numpy()] = np.repeat(np.arange(64), np.diff(index.list_off.cpu().numpy()))
    lists = [np.nonzero(np.isin(cells, probes[j]))[0] for j in range(33)]
    width = max(len(v) for v in lists)
    assert 0 < width <= 16384
    cand = np.full((33, width), -1, np.int64)
    for j, v in enumerate(lists):
        cand[j, :len(v)] = v
    cand = torch.from_numpy(cand).to(DEV)
    index.nprobe = 5
    for k in (1, 100, 1000):
        ws, wi = flat.rerank(q, cand, k)
        assert_matches(index.search(q, k), (ws.cpu().numpy(), wi.cpu().numpy()))
        assert index.last_search_stats["fallback_queries"] == 0
    # numpy in, numpy out
    s, i = index.search(q.cpu().numpy(), 10)
    assert isinstance(s, np.ndarray) and isinstance(i, np.ndarray)
    assert_matches((s, i), tuple(t.cpu().numpy() for t in flat.rerank(q, cand, 10)))


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_ties_go_to_the_lower_corpus_id_across_cells(metric, storage):
    """600 copies of one row in three cells whose ascending cell order is not ascending id order; k = 300 cuts the group."""
    import torch
    from repconc_amd.ivf_flat import IVFFlatIndex
    D, N = 8, 1500
    x, q = _randn((N, D), 51), _randn((3, D), 52)
    x[:600] = (q[0] if metric == L2 else 10.0 * q[0])          # best for query 0: L2 distance +0.0f, inner product 10 |q|^2
    cells = np.empty(N, np.int64)
    cells[:200], cells[200:400], cells[400:600] = 3, 1, 2
    cells[600:] = np.random.default_rng(5).integers(0, 4, N - 600)
    index = IVFFlatIndex(D, 4, device=DEV, metric=metric, storage=storage)
    index.set_coarse(torch.zeros(4, D))
    index.set_lists(x, torch.from_numpy(cells))
    probes = np.array([[0, 1, 2, 3]] * 3, dtype=np.int32)
    want = oracle_probed(_values(x, storage), _values(q, storage), cells, probes, metric)
    for k in (300, 599, 601):
        got = index._search_probes(q, torch.from_numpy(probes), k)
        assert_matches(got, cut(want, k, metric))
        assert index.last_search_stats["fallback_queries"] == 0
    s, i = index._search_probes(q, torch.from_numpy(probes), 300)
    assert i[0].tolist() == list(range(300))
    if metric == L2:
        assert bool((_bits(s[0]) == 0).all())                  # a zero distance is +0.0f


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_more_ties_than_the_candidate_list_holds_take_the_exact_route(metric, storage):
    """17 000 identical rows at the top of every query: more than 16384 rows tie at the 100th score, the status bit fires and
    every query is answered by the exact search over its probed rows — the flat index's answer."""
    import torch
    from repconc_amd.ivf_flat import IVFFlatIndex
    D, N, nq = 8, 20000, 5
    x = -_randn((N, D), 61).abs() - 0.5                        # every other row: negative components of magnitude >= 0.5
    x[1000:18000] = 0.0                                        # the group: inner product 0 with, distance |q|^2 from, every query
    q = _randn((nq, D), 62).abs() * (0.01 if metric == L2 else 1.0)       # positive components: the group ranks first
    cells = torch.from_numpy(np.random.default_rng(6).integers(0, 4, N))
    index = IVFFlatIndex(D, 4, device=DEV, metric=metric, storage=storage)
    index.set_coarse(torch.zeros(4, D))
    index.set_lists(x, cells)
    flat = _flat(metric, storage, D)
    flat.add(x)
    ws, wi = flat.search(q, 100)
    assert wi[:, 0].tolist() == [1000] * nq and wi[:, 99].tolist() == [1099] * nq          # the inputs do what they are meant to
    got = index.search(q, 100, nprobe=4)
    assert index.last_search_stats == {"queries": nq, "fallback_queries": nq, "chunks": 1}
    assert_matches(got, (ws.cpu().numpy(), wi.cpu().numpy()))


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_build_side_add_in_parts_set_lists_and_reset(metric, storage):
    import torch
    from repconc_amd.ivf import coarse_assign
    from repconc_amd.ivf_flat import IVFFlatIndex
    D, N = 64, 10000
    x, q = _corpus(N, D, 21, 70)
    one = IVFFlatIndex(D, 32, device=DEV, metric=metric, storage=storage)
    assert not one.is_trained and one.ntotal == 0
    one.train(x)
    assert one.is_trained and one.ntotal == 0
    one.add(x)
    parts = IVFFlatIndex(D, 32, device=DEV, metric=metric, storage=storage)
    parts.set_coarse(one.coarse)
    parts.add(x[:7000])
    assert parts.ntotal == 7000
    parts.add(x[7000:].cpu().numpy())
    given = IVFFlatIndex(D, 32, device=DEV, metric=metric, storage=storage)
    given.set_coarse(one.coarse)
    given.set_lists(x, coarse_assign(x, one.coarse))
    assert one.ntotal == parts.ntotal == given.ntotal == N
    for other in (parts, given):
        assert torch.equal(other.list_off, one.list_off) and torch.equal(other.ids, one.ids) and torch.equal(other.xb, one.xb)
    for k, nprobe in ((10, 4), (200, 32)):
        ws, wi = one.search(q, k, nprobe=nprobe)
        for other in (parts, given):
            gs, gi = other.search(q, k, nprobe=nprobe)
            assert torch.equal(gi, wi) and torch.equal(_bits(gs), _bits(ws))
    with pytest.raises(ValueError, match="65520|finite"):
        bad = x[:4].clone()
        bad[2, 3] = 70000.0 if storage == "float16" else float("inf")
        one.add(bad)
    assert one.ntotal == N
    one.reset()
    assert one.ntotal == 0 and one.is_trained
    s, i = one.search(q, 5)
    pad = float("inf") if metric == L2 else float("-inf")
    assert bool((s == pad).all()) and bool((i == -1).all())
    one.add(x[:100])                                           # ids start again from 0
    assert one.ntotal == 100 and sorted(one.ids.tolist()) == list(range(100))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_chunked_search_equals_the_unchunked_one(metric):
    import torch
    from repconc_amd import ops
    from repconc_amd.ivf_flat import IVFFlatIndex
    D, N = 64, 10000
    x, _ = _corpus(N, D, 21, 70)
    q = _randn((50, D), 81)
    index = IVFFlatIndex(D, 32, device=DEV, metric=metric)
    index.train(x)
    index.add(x)
    ws, wi = index.search(q, 50, nprobe=6)
    assert index.last_search_stats["chunks"] == 1
    stride = (max(4, int(index._sizes_desc[:6].sum())) + 3) // 4 * 4
    index.MAX_WS_BYTES = ops.ivf_flat_search_ws_bytes(13, 6, 32, stride)       # 13 queries per call: 50 go in four chunks
    gs, gi = index.search(q, 50, nprobe=6)
    assert index.last_search_stats == {"queries": 50, "fallback_queries": 0, "chunks": 4}
    assert torch.equal(gi, wi) and torch.equal(_bits(gs), _bits(ws))
    index.MAX_WS_BYTES = 1                                                      # never fewer than one query per chunk
    gs, gi = index.search(q[:5], 50, nprobe=6)
    assert index.last_search_stats["chunks"] == 5
    assert torch.equal(gi, wi[:5]) and torch.equal(_bits(gs), _bits(ws[:5]))
    assert IVFFlatIndex.MAX_WS_BYTES == 4 << 30


@pytest.mark.gpu
def test_three_runs_have_identical_bits():
    import torch
    from repconc_amd.ivf_flat import IVFFlatIndex
    x, q = _corpus(20000, 768, 33, 40 + 768)
    index = IVFFlatIndex(768, 64, device=DEV, metric=L2, storage="float16")
    index.train(x)
    index.add(x)
    runs = [index.search(q, 100, nprobe=5) for _ in range(3)]
    for s, i in runs[1:]:
        assert torch.equal(i, runs[0][1]) and torch.equal(_bits(s), _bits(runs[0][0]))


@pytest.mark.gpu
def test_refine_index_over_an_fp16_ivf_flat_base_returns_the_fp32_flat_top_k():
    import torch
    from repconc_amd.dense_index import FlatIPIndex
    from repconc_amd.ivf_flat import IVFFlatIndex
    from repconc_amd.refine_index import RefineIndex
    N, D, k, k_factor, nq = 5000, 64, 10, 10, 20
    x, q = _randn((N, D), 91), _randn((nq, D), 92)
    flat, flat16 = FlatIPIndex(D, device=DEV), FlatIPIndex(D, device=DEV, storage="float16")
    flat.add(x)
    flat16.add(x)
    ws, wi = flat.search(q, k)
    _, ci = flat16.search(q, k * k_factor)
    inside = np.array([set(wi[j].tolist()) <= set(ci[j].tolist()) for j in range(nq)])
    assert inside.all(), "the inputs must leave no query out: the fp32 top-10 lies inside the fp16 top-100"
    base = IVFFlatIndex(D, 16, device=DEV, storage="float16")
    base.train(x)
    base.add(x)
    refine = RefineIndex(base, flat, k_factor=k_factor)
    assert refine.ntotal == N and refine.d == D
    got = refine.search(q, k, nprobe=16)
    sel = np.nonzero(inside)[0]
    assert_matches((got[0][sel], got[1][sel]), (ws.cpu().numpy()[sel], wi.cpu().numpy()[sel]))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", ("ip", "l2"))
def test_create_index_with_cells_probing_all_of_them_equals_the_flat_entry(metric):
    import torch
    from repconc_amd.ivf_flat import IVFFlatIndex
    from repconc_amd.models.dense.evaluate_dense import batch_dense_search, create_index
    x, q = _randn((2000, 64), 95).cpu().numpy(), _randn((17, 64), 96)
    ivf, flat = create_index(x, nlist=16, nprobe=16, metric=metric), create_index(x, metric=metric)
    assert isinstance(ivf, IVFFlatIndex) and ivf.nprobe == 16 and ivf.nlist == 16 and ivf.ntotal == 2000
    assert not isinstance(flat, IVFFlatIndex)
    for k in (1, 50):
        ws, wi = flat.search(q, k)
        assert_matches(ivf.search(q, k), (ws.cpu().numpy(), wi.cpu().numpy()))
    with pytest.raises(ValueError, match="bf16x3"):
        create_index(x, screen="bf16x3", nlist=16)
    # the evaluation's batching takes the index as it takes the flat ones
    qids, cids = np.arange(17), np.arange(2000) + 5
    a = batch_dense_search(qids, q.cpu().numpy(), cids, ivf, 20, batch_size=6)
    b = batch_dense_search(qids, q.cpu().numpy(), cids, flat, 20, batch_size=6)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


@pytest.mark.gpu
def test_shim_index_takes_a_filled_quantizer_or_trains_one():
    import torch
    import repconc_amd.faiss_compat as fc
    from repconc_amd.index import METRIC_L2
    x, q = _randn((3000, 32), 97), _randn((9, 32), 98)
    quant = fc.IndexFlatL2(32)
    index = fc.IndexIVFFlat(quant, 32, 8)
    assert index.metric_type == METRIC_L2 and not index.is_trained     # Faiss's default metric
    index.train(x)
    assert index.is_trained and quant.ntotal == 8 and torch.equal(quant.xb, index.coarse)
    index.add(x)
    index.nprobe = 8
    flat = fc.IndexFlatL2(32)
    flat.add(x)
    ws, wi = flat.search(q, 10)
    assert_matches(index.search(q, 10), (ws.cpu().numpy(), wi.cpu().numpy()))
    again = fc.IndexIVFFlat(quant, 32, 8)                               # a quantizer that holds nlist vectors: trained
    assert again.is_trained and torch.equal(again.coarse, index.coarse)
    again.add(x)
    again.nprobe = 8
    assert_matches(again.search(q, 10), (ws.cpu().numpy(), wi.cpu().numpy()))
