"""METRIC_L2 on the PQ indexes: the L2 ADC search, flat and IVF, through every public layer.

Definition under test (include/repconc_hip.h "L2 metric"): sub-distance T[m][c] = the fp32 chain acc = +0.0f,
t = q[m dsub + j] - C[m][c][j], acc = acc + t * t for j ascending (no FMA); d(q, n) = fp32 sum over m ascending of
T[m][code[n][m]]; output d ascending, ties by the lower id, a zero is +0.0f, +inf / -1 past N.  The library works on s = -d
with tables S = 0.0f - T.

The oracle is numpy fp32, step by step: T, S = float32(0) - T, then the table-agnostic `pq_oracle.adc_scores` / `topk_desc`
(unchanged), then d = float32(0) - s.  Ids and distance BITS are compared.  Every case is seeded synthetic data; the centroids
carry clearly unequal norms so that the nearest rows are not the rows of the largest inner product."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import pq_oracle

F32 = np.float32
L2, IP = 1, 0
DEV = "cuda:0"
BIG_N = (1 << 18) + 777            # above the screen's minimum size (2^18), off every tile size


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _ids(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


# ---------------------------------------------------------------------------------------------------------------- oracle
def l2_tables(q, C):
    """S [nq, M, 256] = float32(0) - T, T the j-ascending fp32 chain of (q_j - c_j)^2 (numpy rounds the subtraction, the
    product and the sum separately)."""
    nq = q.shape[0]
    M, K, dsub = C.shape
    qs = q.reshape(nq, M, dsub).astype(F32)
    T = np.zeros((nq, M, K), F32)
    for j in range(dsub):
        t = qs[:, :, None, j] - C[None, :, :, j]
        T = T + t * t
    assert T.dtype == F32 and np.isfinite(T).all()
    return F32(0) - T


def l2_scores(q, C, codes):
    """s [nq, N] = the m-ascending fp32 sum of S (= -d)."""
    return pq_oracle.adc_scores(l2_tables(q, C), codes)


def l2_topk(s, k, ids=None):
    """(d [nq, k], ids [nq, k]) from score rows s = -d: d ascending, ties by the lower id, +inf / -1 past the row count."""
    ts, ti = pq_oracle.topk_desc(s, k)
    d = F32(0) - ts
    if ids is not None:
        ti = ids[ti]
    pad = k - d.shape[1]
    if pad > 0:
        d = np.concatenate([d, np.full((d.shape[0], pad), np.inf, F32)], 1)
        ti = np.concatenate([ti, np.full((ti.shape[0], pad), -1, np.int64)], 1)
    return d, ti


def l2_search(q, C, codes, k):
    return l2_topk(l2_scores(q, C, codes), k)


def _case(M, D, N, nq, seed):
    """Centroids with norms spread over a factor of 8 per sub-quantiser, gaussian queries, uniform codes."""
    rng = np.random.default_rng(seed)
    dsub = D // M
    C = (rng.standard_normal((M, 256, dsub)) * rng.uniform(0.25, 2.0, (M, 256, 1))).astype(F32)
    codes = rng.integers(0, 256, (N, M), dtype=np.uint8)
    q = rng.standard_normal((nq, D)).astype(F32)
    return C, codes, q


def _same(got, want, what=""):
    gs, gi = got
    ws, wi = want
    assert np.array_equal(_ids(gi), wi), what
    assert np.array_equal(_bits(gs), _bits(ws)), what


_cache = {}


def _big(M):
    """The screened cases (N = 2^18 + 777, D = 8 M, nq = 19 — off the 16-query group): inputs, device copies and the
    oracle's answer at k = 100, made once per module."""
    if M not in _cache:
        C, codes, q = _case(M, 8 * M, BIG_N, 19, 9000 + M)
        _cache[M] = SimpleNamespace(C=C, codes=codes, q=q, dC=_t(C), dcodes=_t(codes), dq=_t(q),
                                    want=l2_search(q, C, codes, 100))
    return _cache[M]


# ------------------------------------------------------------------------------------------------------------ CPU, no GPU
def test_merge_topk_ascending_on_hand_made_parts():
    from repconc_amd.sharded_search import merge_topk
    inf = float("inf")
    # two shards, two queries, k = 3; query 0: a tie at 1.0 between ids 7 and 2, an empty slot in shard 1;
    # query 1: only empty slots in shard 0
    s = torch.tensor([[[0.5, 1.0, 4.0], [inf, inf, inf]],
                      [[0.0, 1.0, inf], [0.25, 2.0, 3.0]]])
    i = torch.tensor([[[5, 7, 1], [-1, -1, -1]],
                      [[9, 2, -1], [4, 3, 8]]])
    ms, mi = merge_topk(s, i, 3, largest=False)
    assert mi.tolist() == [[9, 5, 2], [4, 3, 8]]
    assert ms.tolist() == [[0.0, 0.5, 1.0], [0.25, 2.0, 3.0]]
    ms, mi = merge_topk(s, i, 5, largest=False)
    assert mi.tolist() == [[9, 5, 2, 7, 1], [4, 3, 8, -1, -1]]
    assert ms.tolist() == [[0.0, 0.5, 1.0, 1.0, 4.0], [0.25, 2.0, 3.0, inf, inf]]
    # an id tie at +0.0 / a real row next to empty slots: -1 / +inf last even where k takes every slot
    ms, mi = merge_topk(s, i, 6, largest=False)
    assert mi[0].tolist() == [9, 5, 2, 7, 1, -1] and mi[1].tolist() == [4, 3, 8, -1, -1, -1]
    assert ms[0, 5].item() == inf


def test_merge_topk_descending_is_what_it_was():
    from repconc_amd.sharded_search import merge_topk
    ninf = float("-inf")
    s = torch.tensor([[[4.0, 1.0, 0.5], [ninf, ninf, ninf]],
                      [[3.0, 1.0, ninf], [2.0, 1.0, 0.25]]])
    i = torch.tensor([[[1, 7, 5], [-1, -1, -1]],
                      [[9, 2, -1], [4, 3, 8]]])
    for kwargs in ({}, {"largest": True}):
        ms, mi = merge_topk(s, i, 4, **kwargs)
        assert mi.tolist() == [[1, 9, 2, 7], [4, 3, 8, -1]]
        assert ms.tolist() == [[4.0, 3.0, 1.0, 1.0], [2.0, 1.0, 0.25, ninf]]
    # the default is positional-compatible: three arguments as before
    ms3, mi3 = merge_topk(s, i, 4)
    assert torch.equal(mi3, mi) and torch.equal(ms3, ms)


def test_header_and_prototypes_name_the_l2_entries():
    from repconc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "repconc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rc_[a-z0-9_]+)\s*\(", hdr))
    for name in ("rc_adc_lut_l2", "rc_adc_search_l2_q", "rc_adc_search_l2_exact", "rc_index_set_metric"):
        assert name in declared and name in _lib.PROTOTYPES, name
    assert _lib.PROTOTYPES["rc_adc_lut_l2"] == _lib.PROTOTYPES["rc_adc_lut"]
    assert _lib.PROTOTYPES["rc_adc_search_l2_q"] == _lib.PROTOTYPES["rc_adc_search_q"]
    assert _lib.PROTOTYPES["rc_adc_search_l2_exact"] == _lib.PROTOTYPES["rc_adc_search_exact"]


def test_indexes_refuse_a_metric_that_is_neither_ip_nor_l2():
    from repconc_amd.index import METRIC_INNER_PRODUCT, METRIC_L2, PQIndex
    from repconc_amd.ivf import IVFPQIndex
    assert (METRIC_INNER_PRODUCT, METRIC_L2) == (0, 1)
    for bad in (2, -1, 23):
        with pytest.raises(ValueError):
            PQIndex(16, 2, 8, bad, device=torch.device("cpu"))
        with pytest.raises(ValueError):
            IVFPQIndex(16, 2, 4, device=torch.device("cpu"), metric=bad)


def test_index_file_round_trips_metric_l2_without_a_device(tmp_path):
    from repconc_amd import faiss_io
    rng = np.random.default_rng(5)
    d, M, n = 16, 2, 7
    cent = torch.from_numpy(rng.standard_normal((M, 256, d // M)).astype(F32))
    codes = torch.from_numpy(rng.integers(0, 256, (n, M), dtype=np.uint8))
    for metric in (L2, IP):
        index = SimpleNamespace(pq=SimpleNamespace(d=d, M=M, nbits=8, centroids=cent), codes=codes, ntotal=n,
                                is_trained=True, metric_type=metric)
        path = str(tmp_path / f"ixpq{metric}")
        faiss_io.write_index(index, path)
        p = faiss_io.parse_index_file(path)
        assert p["metric"] == metric and p["ntotal"] == n and p["M"] == M
        assert np.array_equal(p["codes"], codes.numpy()) and np.array_equal(p["centroids"], cent.numpy())


# ------------------------------------------------------------------------------------------------------------------ table
@pytest.mark.gpu
@pytest.mark.parametrize("dsub", [8, 16, 96, 4, 20])          # 8 / 16 / 96: rows in registers; 4 / 20: the run-time-width kernel
def test_l2_table_bits(dsub):
    from repconc_amd import ops
    M, nq = 4, 33                                               # 33: crosses the 32-query chunk of the register form
    C, _, q = _case(M, M * dsub, 1, nq, 100 + dsub)
    got = ops.adc_lut(_t(C), _t(q), metric=L2)
    want = l2_tables(q, C)
    assert got.shape == (nq, M, 256)
    assert np.array_equal(_bits(got), _bits(want))
    assert (got <= 0).all() and not np.any(_bits(got) == 0x80000000)
    # the default metric is the inner-product table, unchanged
    assert np.array_equal(_bits(ops.adc_lut(_t(C), _t(q))), _bits(pq_oracle.adc_lut(q, C)))
    with pytest.raises(ValueError):
        ops.adc_lut(_t(C), _t(q), metric=2)


@pytest.mark.gpu
@pytest.mark.parametrize("dsub", [8, 20])
def test_l2_table_entry_of_a_query_slice_equal_to_a_centroid_is_plus_zero(dsub):
    from repconc_amd import ops
    M, nq = 4, 33
    C, _, q = _case(M, M * dsub, 1, nq, 200 + dsub)
    hits = [(0, 0, 0), (5, 1, 255), (32, 3, 17)]                # (query, sub-quantiser, centroid)
    for qi, m, c in hits:
        q[qi, m * dsub:(m + 1) * dsub] = C[m, c]
    got = _bits(ops.adc_lut(_t(C), _t(q), metric=L2))
    for qi, m, c in hits:
        assert got[qi, m, c] == 0x00000000, (qi, m, c, hex(got[qi, m, c]))
    assert np.array_equal(got, _bits(l2_tables(q, C)))


# ------------------------------------------------------------------------------------- exact route, run-time widths, padding
@pytest.mark.gpu
@pytest.mark.parametrize("M,D", [(6, 24), (8, 160), (24, 192), (48, 768)])     # 6: no screening kernel (run-time scan)
def test_l2_exact_route_and_small_index(M, D):
    from repconc_amd import ops
    N, nq = 5000, 9
    C, codes, q = _case(M, D, N, nq, 300 + M)
    s = l2_scores(q, C, codes)
    for k in (10, 6000):                                        # 6000 > N: +inf / -1 past N
        want = l2_topk(s, k)
        if k > N:
            assert np.isposinf(want[0][:, N:]).all() and (want[1][:, N:] == -1).all()
        _same(ops.adc_search_exact(_t(codes), _t(C), _t(q), k, metric=L2), want, ("exact", M, k))
        _same(ops.adc_search(_t(codes), _t(C), _t(q), k, metric=L2), want, ("search", M, k))
    wd, wi = l2_topk(s, 10)
    _same(ops.adc_search(_t(codes), _t(C), _t(q), 10, id_offset=1000, metric=L2), (wd, wi + 1000), "id_offset")


# ---------------------------------------------------------------------------------------------------------- screened route
@pytest.mark.gpu
@pytest.mark.parametrize("M", [16, 48, 96, 24])               # 16 / 48 / 96: the 16-query image screen; 24: the round-1 screen
def test_l2_screened_route(M):
    from repconc_amd import ops
    from repconc_amd.index import PQIndex
    c = _big(M)
    k = 100
    stats = {}
    pend = ops.adc_search(c.dcodes, c.dC, c.dq, k, metric=L2, defer=True, stats=stats)
    got = pend.result()
    assert pend.metric == L2
    assert "survivors" in stats, "the 8-bit screen did not run"
    surv, cand = stats["survivors"].cpu().numpy(), stats["candidates"].cpu().numpy()
    assert (surv < BIG_N).all() and (surv >= cand).all(), (surv, cand)
    _same(got, c.want, ("screened", M))
    _same(ops.adc_search_exact(c.dcodes, c.dC, c.dq, k, metric=L2), c.want, ("exact", M))
    if M in (48, 24):
        # through the index (resident image for M = 48, none for M = 24), numpy in / numpy out
        index = PQIndex(8 * M, M, 8, L2, device=torch.device(DEV))
        index.set_centroids(c.dC)
        index.add_codes(c.dcodes)
        _same(index.search(c.q, k), c.want, ("PQIndex", M))
        assert index.last_search.metric == L2


# ---------------------------------------------------------------------------------------------------------- zeros and ties
@pytest.mark.gpu
def test_l2_zero_distances_are_plus_zero_with_ids_ascending():
    from repconc_amd import ops
    M, k = 48, 100
    c = _big(M)
    rng = np.random.default_rng(77)
    codes = c.codes.copy()
    where = np.sort(rng.choice(BIG_N, (2, 64), replace=False), axis=1)      # two groups of 64 scattered duplicates
    rows = rng.integers(0, 256, (2, M), dtype=np.uint8)
    q = c.q.copy()
    for g in range(2):
        codes[where[g]] = rows[g]
        q[g] = pq_oracle.decode(rows[g:g + 1], c.C)[0]                      # the query IS the reconstruction of the rows
    dcodes, dq = _t(codes), _t(q)
    stats = {}
    fast = ops.adc_search(dcodes, c.dC, dq, k, metric=L2, stats=stats)
    assert "survivors" in stats and (stats["survivors"].cpu().numpy() < BIG_N).all()
    exact = ops.adc_search_exact(dcodes, c.dC, dq, k, metric=L2)
    for name, (s, i) in (("screened", fast), ("exact", exact)):
        b, i, s = _bits(s), _ids(i), s.cpu().numpy()
        for g in range(2):
            assert (b[g, :64] == 0x00000000).all(), (name, g, b[g, :64])
            assert np.array_equal(i[g, :64], where[g]), (name, g)
            assert (s[g, 64:] > 0).all()
    _same(fast, (exact[0].cpu().numpy(), exact[1].cpu().numpy()), "screened vs exact")


# ------------------------------------------------------------------------------------------------ retry and degenerate paths
@pytest.mark.gpu
def test_l2_repeated_queries_keep_the_answer():
    from repconc_amd import ops
    c = _big(16)
    # rank of the threshold in the 32768-row sample: mu = 100 * 32768 / N = 12.5 expected top-k rows, r = floor(mu - 3 sqrt(mu + 1)
    # + 4) + 1 = 6: a query keeps too few candidates unless its sample holds <= 5 of its top 100 (Poisson(12.5): 1.7 %)
    pend = ops.adc_search(c.dcodes, c.dC, c.dq, 100, sel_slack=-3.0, metric=L2, defer=True)
    got = pend.result()
    assert pend.stats["retried_queries"] > 0, pend.stats
    _same(got, c.want, "repeated")
    # ... and handed over to the exact route at once
    pend = ops.adc_search(c.dcodes, c.dC, c.dq, 100, sel_slack=-3.0, max_retries=0, metric=L2, defer=True)
    got = pend.result()
    assert pend.stats["exact_queries"] > 0 and pend.stats["retried_queries"] == 0, pend.stats
    _same(got, c.want, "handed over")


@pytest.mark.gpu
def test_l2_index_of_identical_rows_goes_to_the_exact_route():
    from repconc_amd import ops
    M, D, N, nq, k = 16, 128, (1 << 18) + 5, 3, 50
    C, codes, q = _case(M, D, 1, nq, 555)
    s1 = l2_scores(q, C, codes)                                              # [nq, 1]: the one distance of every query
    dcodes = _t(codes).expand(N, M).contiguous()
    pend = ops.adc_search(dcodes, _t(C), _t(q), k, metric=L2, defer=True)
    gs, gi = pend.result()
    assert pend.stats["exact_queries"] == nq, pend.stats
    assert np.array_equal(_ids(gi), np.broadcast_to(np.arange(k), (nq, k)))
    assert np.array_equal(_bits(gs), np.broadcast_to(_bits(F32(0) - s1), (nq, k)))


# -------------------------------------------------------------------------------------------------------- metric isolation
@pytest.mark.gpu
def test_metric_isolation_on_one_set_of_codes():
    from repconc_amd.index import METRIC_L2, PQIndex
    M, D, N, nq, k = 16, 128, 20000, 9, 20
    C, codes, q = _case(M, D, N, nq, 808)
    res = {}
    for metric in (IP, L2):
        index = PQIndex(D, M, 8, metric, device=torch.device(DEV))
        index.set_centroids(_t(C))
        index.add_codes(_t(codes))
        res[metric] = index.search(q, k)
    assert METRIC_L2 == L2
    _same(res[IP], pq_oracle.adc_search(q, C, codes, k), "inner product, as before")
    _same(res[L2], l2_search(q, C, codes, k), "L2")
    assert not np.array_equal(res[IP][1][:, 0], res[L2][1][:, 0])           # the nearest row is not the best-scoring row
    assert (np.diff(res[L2][0], axis=1) >= 0).all() and (np.diff(res[IP][0], axis=1) <= 0).all()


# -------------------------------------------------------------------------------------------------------------- handle API
@pytest.mark.gpu
def test_c_index_handle_with_metric_l2():
    from repconc_amd import _lib
    lib, h = _lib.load(), _lib.handle(0)
    M, D, N, nq, k = 16, 128, 20000, 7, 30
    C, codes, q = _case(M, D, N, nq, 909)
    idx = ctypes.c_void_p()
    assert lib.rc_index_create(h, D, M, 256, ctypes.byref(idx)) == 0
    try:
        dq, dC, dcodes = _t(q), _t(C), _t(codes)
        sc = torch.empty((nq, k), dtype=torch.float32, device=DEV)
        ids = torch.empty((nq, k), dtype=torch.int64, device=DEV)
        assert lib.rc_index_set_metric(idx, 2) == _lib.RC_EINVAL and lib.rc_index_set_metric(idx, -1) == _lib.RC_EINVAL
        assert lib.rc_index_set_metric(None, 1) == _lib.RC_EINVAL
        assert lib.rc_index_set_metric(idx, 1) == 0
        assert lib.rc_index_set_centroids(idx, dC.data_ptr(), None) == 0
        assert lib.rc_index_search(idx, dq.data_ptr(), nq, k, sc.data_ptr(), ids.data_ptr(), None) == 0
        assert bool((ids == -1).all()) and bool(torch.isposinf(sc).all())   # empty L2 index: +inf / -1
        assert lib.rc_index_add_codes(idx, dcodes[:777].data_ptr(), 777, None) == 0
        assert lib.rc_index_add_codes(idx, dcodes[777:].data_ptr(), N - 777, None) == 0
        torch.cuda.synchronize()
        assert lib.rc_index_search(idx, dq.data_ptr(), nq, k, sc.data_ptr(), ids.data_ptr(), None) == 0
        _same((sc, ids), l2_search(q, C, codes, k), "handle, L2")
        assert lib.rc_index_set_metric(idx, 0) == 0                          # and back: the index keeps no metric state
        assert lib.rc_index_search(idx, dq.data_ptr(), nq, k, sc.data_ptr(), ids.data_ptr(), None) == 0
        _same((sc, ids), pq_oracle.adc_search(q, C, codes, k), "handle, inner product")
    finally:
        assert lib.rc_index_destroy(idx) == 0


# ----------------------------------------------------------------------------------------------------------- shim and file
@pytest.mark.gpu
def test_faiss_shim_index_pq_l2_and_the_index_file(tmp_path):
    from repconc_amd import faiss_compat as faiss
    from repconc_amd.models.repconc.evaluate_repconc import load_index_to_gpu
    M, D, N, nq, k = 16, 128, 20000, 9, 20
    C, codes, q = _case(M, D, N, nq, 1010)
    want = l2_search(q, C, codes, k)
    index = faiss.IndexPQ(D, M, 8, faiss.METRIC_L2)
    assert index.metric_type == faiss.METRIC_L2 == 1
    faiss.copy_array_to_vector(C.ravel(), index.pq.centroids)
    index.add_codes(codes)
    _same(index.search(q, k), want, "IndexPQ(METRIC_L2)")
    path = str(tmp_path / "index")
    faiss.write_index(index, path)
    back = faiss.read_index(path)
    assert back.metric_type == faiss.METRIC_L2 and back.ntotal == N
    _same(back.search(q, k), want, "read_index")
    moved = load_index_to_gpu(back, 0)
    assert moved.metric_type == faiss.METRIC_L2
    _same(moved.search(q, k), want, "load_index_to_gpu")


# ---------------------------------------------------------------------------------------------- sharded / replicated, one device
@pytest.mark.gpu
def test_sharded_and_replicated_l2_on_one_device():
    from repconc_amd.index import PQIndex
    from repconc_amd.multi_index import ReplicatedPQIndex, ShardedPQIndex
    from repconc_amd.sharded_search import search_virtual_shards, sharded_search
    M, D, N, nq, k = 16, 128, 30000, 9, 40
    C, codes, q = _case(M, D, N, nq, 1111)
    flat = PQIndex(D, M, 8, L2, device=torch.device(DEV))
    flat.set_centroids(_t(C))
    flat.add_codes(_t(codes))
    want = flat.search(q, k)
    _same(want, l2_search(q, C, codes, k), "flat")
    sharded = ShardedPQIndex(flat, devices=[0, 0])
    assert sharded.metric_type == L2 and [p.metric_type for p in sharded.parts] == [L2, L2]
    _same(sharded.search(q, k), want, "sharded")
    _same(ReplicatedPQIndex(flat, devices=[0, 0]).search(q, k), want, "replicated")
    _same(search_virtual_shards(sharded.parts, _t(q), k), want, "virtual shards")
    _same(sharded_search(flat, _t(q), k), want, "sharded_search, one rank")
    # k larger than a shard: each part pads with +inf / -1, the merge keeps them last
    small = PQIndex(D, M, 8, L2, device=torch.device(DEV))
    small.set_centroids(_t(C))
    small.add_codes(_t(codes[:30]))
    _same(ShardedPQIndex(small, devices=[0, 0]).search(q, 25), l2_search(q, C, codes[:30], 25), "padded shards")


# --------------------------------------------------------------------------------------------------------------------- IVF
def _ivf_case():
    if "ivf" not in _cache:
        from repconc_amd.index import PQIndex
        from repconc_amd.ivf import IVFPQIndex
        M, D, N, nq, nlist = 16, 128, 60000, 19, 64
        C, codes, q = _case(M, D, N, nq, 1212)
        flat = PQIndex(D, M, 8, L2, device=torch.device(DEV))
        flat.set_centroids(_t(C))
        flat.add_codes(_t(codes))
        ivf = IVFPQIndex.from_flat(flat, nlist, iters=3)
        _cache["ivf"] = SimpleNamespace(C=C, codes=codes, q=q, flat=flat, ivf=ivf, nlist=nlist, N=N,
                                        s=l2_scores(q, C, codes))
    return _cache["ivf"]


@pytest.mark.gpu
def test_ivf_l2_probing_every_cell_is_the_flat_l2_result():
    from repconc_amd.ivf import IVFPQIndex
    c = _ivf_case()
    k = 50
    assert c.ivf.metric_type == L2                               # from_flat inherits the metric
    assert c.ivf.to(torch.device(DEV)).metric_type == L2         # ... and to() copies it
    assert IVFPQIndex(128, 16, 4, device=torch.device(DEV)).metric_type == IP
    want = c.flat.search(c.q, k)
    _same(want, l2_topk(c.s, k), "flat")
    for method in ("scan", "lists8", "lists16"):
        _same(c.ivf.search(c.q, k, c.nlist, method=method), want, method)
    _same(c.ivf.to(torch.device(DEV)).search(_t(c.q), k, c.nlist), want, "copy")


@pytest.mark.gpu
def test_ivf_l2_probed_cells_against_the_restricted_oracle():
    c = _ivf_case()
    ivf, k = c.ivf, 50
    corpus = ivf.ids.cpu().numpy()                               # list-major row -> corpus id
    cell_of = np.empty(c.N, np.int64)
    cell_of[corpus] = np.repeat(np.arange(c.nlist), np.diff(ivf.list_off.cpu().numpy()))
    for nprobe, kk in ((4, k), (1, 2500)):                       # nprobe = 1, k = 2500 > a cell: +inf / -1 in the unfilled slots
        probes = ivf.probe(_t(c.q), nprobe, ordered=False).cpu().numpy()
        wd = np.full((len(c.q), kk), np.inf, F32)
        wi = np.full((len(c.q), kk), -1, np.int64)
        for j in range(len(c.q)):
            rows = np.nonzero(np.isin(cell_of, probes[j]))[0]    # corpus ids ascending: the tie rule
            wd[j:j + 1], wi[j:j + 1] = l2_topk(c.s[j:j + 1, rows], kk, rows)
        if nprobe == 1:
            assert (wi[:, -1] == -1).all() and np.isposinf(wd[:, -1]).all() and (wi[:, 0] >= 0).all()
        got = {m: ivf.search(c.q, kk, nprobe, method=m) for m in ("scan", "lists8", "lists16")}
        for m in got:
            _same(got[m], (wd, wi), (m, nprobe))


@pytest.mark.gpu
def test_ivf_l2_probe_takes_the_nearest_cells_and_the_lower_id_of_two_equidistant():
    from repconc_amd.ivf import IVFPQIndex
    d = 16
    coarse = np.zeros((4, d), F32)
    coarse[0, :2] = (0, 10)
    coarse[1, :2] = (2, 1)
    coarse[2, :2] = (0, -3)
    coarse[3, :2] = (-2, 1)
    q = np.zeros((1, d), F32)
    q[0, 1] = 1                                                  # squared distances 81, 4, 16, 4; inner products 10, 1, -3, 1
    for metric, order in ((L2, [1, 3, 2, 0]), (IP, [0, 1, 3, 2])):
        ivf = IVFPQIndex(d, 16, 4, device=torch.device(DEV), metric=metric)
        ivf.coarse = _t(coarse)
        assert ivf.probe(_t(q), 4, ordered=True).cpu().numpy().tolist() == [order]
        for nprobe in (1, 2, 3):
            assert ivf.probe(_t(q), nprobe, ordered=True).cpu().numpy().tolist() == [order[:nprobe]]
            assert ivf.probe(_t(q), nprobe, ordered=False).cpu().numpy().tolist() == [sorted(order[:nprobe])]
    # the cached ||c||^2 follows the coarse table: a new tensor and an in-place write both count
    ivf = IVFPQIndex(d, 16, 4, device=torch.device(DEV), metric=L2)
    ivf.coarse = _t(coarse)
    assert ivf.probe(_t(q), 1).item() == 1
    ivf.coarse[1, 0] = 20.0
    assert ivf.probe(_t(q), 1).item() == 3
    ivf.coarse = _t(coarse[::-1].copy())
    assert ivf.probe(_t(q), 2).cpu().numpy().tolist() == [[0, 2]]


@pytest.mark.gpu
def test_ivf_inner_product_index_is_unchanged():
    from repconc_amd.ivf import IVFPQIndex
    M, D, N, nq, nlist, k, nprobe = 16, 128, 60000, 19, 64, 50, 4
    C, codes, q = _case(M, D, N, nq, 1313)
    rng = np.random.default_rng(1314)
    cells = rng.integers(0, nlist, N)
    coarse = rng.standard_normal((nlist, D)).astype(F32)
    ivf = IVFPQIndex(D, M, nlist, device=torch.device(DEV))
    assert ivf.metric_type == IP
    ivf.set_centroids(_t(C))
    ivf.coarse = _t(coarse)
    ivf.set_lists(_t(codes), _t(cells))
    want = pq_oracle.ivf_search(q, C, codes, cells, coarse, k, nprobe)
    for method in ("scan", "lists8", "lists16"):
        _same(ivf.search(q, k, nprobe, method=method), want, method)
