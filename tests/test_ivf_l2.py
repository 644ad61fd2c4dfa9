"""METRIC_L2 on the IVF-PQ index, off its clean path: probe selection against fp64, every route and every repair path of
`repconc_amd/ivf.py` with evidence that the path ran, the edges of the public surface under both metrics, and L2 tables that
strain the 8-bit screens, made by the real table kernel.

All comparisons are ids and uint32 distance bits against the numpy oracle (`oracle/pq_oracle.py`: `adc_lut_l2`,
`ivf_search(metric=1)` — cells of smallest fp64 ||q - c_l||^2, S = float32(0) - T scored m ascending in fp32, order (distance
asc, corpus id asc), d = float32(0) - s, +inf / -1 in unfilled slots).  The only tolerance is the rounding bound B of the probe
score, section 2, derived in `probe_bound`.

The oracle probes by fp64, the library by an fp32 expression through a library GEMM.  Wherever a search is compared with the
oracle, the test first checks on the CPU that the query's probe set is decisive (`_assert_decisive`: the fp64 gap at the
boundary exceeds 2 B), so a difference is the search's and not a coin toss between two cells."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import pq_oracle, synth
from test_adc_l2 import _case, l2_scores, l2_tables, l2_topk

F32, F64 = np.float32, np.float64
IP, L2 = 0, 1
DEV = "cuda:0"
U = 2.0 ** -24
METHODS = ("auto", "lists", "lists8", "lists16", "lists_host_plan", "scan")


def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)       # a copy: the shared cases are read-only


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def _bits(a):
    return np.ascontiguousarray(_np(a), dtype=F32).view(np.uint32)


def _same(got, want, what=""):
    assert np.array_equal(_np(got[1]), want[1]), what
    assert np.array_equal(_bits(got[0]), _bits(want[0])), what


def _index(C, coarse, codes, cells, metric=L2):
    from repconc_amd.ivf import IVFPQIndex
    M, _, dsub = C.shape
    ivf = IVFPQIndex(M * dsub, M, coarse.shape[0], device=torch.device(DEV), metric=metric)
    ivf.set_centroids(_t(C))
    ivf.coarse = _t(coarse)
    ivf.set_lists(_t(codes), _t(cells))
    return ivf


# ------------------------------------------------------------------------------------------------------- 1. the oracle, CPU
def test_l2_oracle_equals_the_composition_of_test_adc_l2():
    """`pq_oracle.adc_lut_l2` is `l2_tables` bit for bit, and `ivf_search(metric=1)` probing every cell / a subset is `l2_topk`
    of the scores of the probed rows (one small case; a zero distance and an unfilled tail included)."""
    M, D, N, nq, nlist, k = 4, 32, 300, 5, 6, 80
    C, codes, q = _case(M, D, N, nq, 4001)
    q[1] = pq_oracle.decode(codes[17:18], C)[0]                                   # a zero distance
    rng = np.random.default_rng(4002)
    cells = rng.integers(0, nlist, N)
    coarse = rng.standard_normal((nlist, D)).astype(F32)
    S = pq_oracle.adc_lut_l2(q, C)
    assert S.dtype == F32 and np.array_equal(S.view(np.uint32), l2_tables(q, C).view(np.uint32))
    assert not np.any(S.view(np.uint32) == 0x80000000) and (S <= 0).all()
    s = l2_scores(q, C, codes)
    d, i = pq_oracle.ivf_search(q, C, codes, cells, coarse, k, nlist, metric=1)
    wd, wi = l2_topk(s, k)
    assert np.array_equal(i, wi) and np.array_equal(d.view(np.uint32), wd.view(np.uint32))
    assert d[1, 0].view(np.uint32) == 0 and i[1, 0] == 17
    d64 = ((q.astype(F64)[:, None] - coarse.astype(F64)[None]) ** 2).sum(2)
    d, i = pq_oracle.ivf_search(q, C, codes, cells, coarse, k, 1, metric=1)       # one cell of ~50 rows: a tail
    for j in range(nq):
        rows = np.nonzero(cells == np.argmin(d64[j]))[0]
        wd, wi = l2_topk(s[j:j + 1, rows], k, rows)
        assert np.array_equal(i[j:j + 1], wi) and np.array_equal(d[j:j + 1].view(np.uint32), wd.view(np.uint32))
        assert len(rows) < k and np.isposinf(d[j, len(rows):]).all() and (i[j, len(rows):] == -1).all()
    with pytest.raises(ValueError):
        pq_oracle.ivf_search(q, C, codes, cells, coarse, k, 1, metric=2)


def test_oracle_metric_0_is_what_it_was():
    """`ivf_search(metric=0)` and the default on the degenerate-cell case of test_search_robust.py, against the inner-product
    search spelled out from the oracle's own parts as the function was before it took a metric."""
    M, nlist, N, nq, k, nprobe = 48, 16, 60000, 5, 200, 4
    C = synth.gaussian(31 + 1, (M, 256, 768 // M))
    base = synth.uniform_codes(31 + 2, 3, M)
    q = synth.gaussian(31 + 3, (nq, 768))
    rng = np.random.default_rng(32)
    codes = base[rng.integers(0, 3, N)]
    cells = rng.integers(0, nlist, N)
    coarse = synth.gaussian(33, (nlist, 768))
    cs = q.astype(F32) @ coarse.astype(F32).T
    order = np.lexsort((np.broadcast_to(np.arange(nlist), cs.shape), -cs.astype(F64)), axis=1)[:, :nprobe]
    lut = pq_oracle.adc_lut(q, C)
    ws = np.full((nq, k), -np.inf, F32)
    wi = np.full((nq, k), -1, np.int64)
    for j in range(nq):
        rows = np.nonzero(np.isin(cells, order[j]))[0]
        s = pq_oracle.adc_scores(lut[j:j + 1], codes[rows])[0]
        o = np.lexsort((rows, -s.astype(F64)))[:k]
        ws[j, :len(o)], wi[j, :len(o)] = s[o], rows[o]
    for got in (pq_oracle.ivf_search(q, C, codes, cells, coarse, k, nprobe),
                pq_oracle.ivf_search(q, C, codes, cells, coarse, k, nprobe, metric=0)):
        assert got[0].dtype == F32 and got[1].dtype == np.int64
        assert np.array_equal(got[1], wi) and np.array_equal(got[0].view(np.uint32), ws.view(np.uint32))


# ------------------------------------------------------------------------------------- 2. probe selection against fp64
PROBE_D, PROBE_NQ = 128, 16
PROBE_NLISTS = (64, 1000)
PROBE_FAMILIES = ("gaussian", "norms_x8", "offset30", "equidistant")


def probe_bound(q, coarse):
    """B [nq, nlist] with |fl32(2 q.c - ||c||^2) - (2 q.c - ||c||^2)| <= B for ANY order of fp32 accumulation, FMA or not.

    With u = 2^-24 and gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, ch. 3): a D-term fp32 dot product in any
    order (each product rounded or fused, D - 1 rounded additions: every term passes through at most D roundings) has
    |fl(q.c) - q.c| <= gamma_D sum_j |q_j c_j|; doubling is exact; the cached norm n = fl(sum_j c_j^2), any order, has
    |n - ||c||^2| <= gamma_D ||c||^2.  The last subtraction rounds once: fl(a - n) = (a - n)(1 + delta), |delta| <= u, with
    |a - n| <= (1 + gamma_D) A, A = 2 sum_j |q_j c_j| + ||c||^2.  Together
        error <= (gamma_D + u (1 + gamma_D)) A = (D + 1) u / (1 - D u) A <= (D + 2) u A      whenever D (D + 2) u <= 1, D <= 4094.
    No term is so small that fp32 underflow matters in these families; (D + 1) 2^-149 is added for it all the same.  A is
    evaluated in fp64 from the fp32 inputs.  Consequence used below, per query with B_q = max_l B[q, l]: if the library takes
    cell a and leaves cell b, fl(s_a) >= fl(s_b), so the exact distances satisfy d_a <= d_b + B_a + B_b <= d_b + 2 B_q."""
    q64, c64 = q.astype(F64), coarse.astype(F64)
    D = q.shape[1]
    assert D * (D + 2) * U <= 1
    A = 2.0 * (np.abs(q64)[:, None, :] * np.abs(c64)[None, :, :]).sum(2) + (c64 * c64).sum(1)[None, :]
    return (D + 2) * U * A + (D + 1) * 2.0 ** -149


@functools.lru_cache(maxsize=None)
def _probe_family(family, nlist):
    """(q [16, 128], coarse [nlist, 128], exact): seeded, read-only.  exact: every fp32 operation of the score is exact (small
    integers), the fp32 ranking IS the fp64 ranking and B counts as 0."""
    rng = np.random.default_rng(3000 + 10 * PROBE_FAMILIES.index(family) + PROBE_NLISTS.index(nlist))
    D, nq = PROBE_D, PROBE_NQ
    exact = False
    if family == "gaussian":
        q, c = rng.standard_normal((nq, D)), rng.standard_normal((nlist, D))
    elif family == "norms_x8":                                   # nearest is not largest inner product
        q, c = rng.standard_normal((nq, D)), rng.standard_normal((nlist, D)) * rng.uniform(0.25, 2.0, (nlist, 1))
    elif family == "offset30":                                   # cancellation: ||q - c||^2 ~ 1e4 from terms ~ 1e5 each
        q, c = 30.0 + rng.standard_normal((nq, D)), 30.0 + 8.0 * rng.standard_normal((nlist, D))
    else:
        # cell 0 = the origin, nearest to every query; cells 1 + i and 1 + P + i differ in the sign of coordinate 127, where
        # every query is 0: exactly equidistant from every query; the last cell is far.  The nearest 8 are then the origin,
        # three pairs and ONE of a pair: a tie at the boundary, the lower id must win.
        exact = True
        P = (nlist - 2) // 2
        q = rng.integers(-2, 3, (nq, D)).astype(F64)
        q[:, D - 1] = 0
        half = rng.integers(-3, 4, (P, D)).astype(F64)
        half[:, D - 1] = 1
        other = half.copy()
        other[:, D - 1] = -1
        c = np.concatenate([np.zeros((1, D)), half, other, np.full((1, D), 3.0)])
        assert c.shape[0] == nlist
    q, c = q.astype(F32), c.astype(F32)
    q.setflags(write=False)
    c.setflags(write=False)
    return q, c, exact


def _fp32_scores_in_four_orders(q, c):
    """fl32(2 q.c - ||c||^2) [nq, nlist] with products rounded and the two sums taken sequentially, reversed, pairwise and in
    blocks of 16 (block sums sequential, then the blocks sequential)."""
    p = q[:, None, :] * c[None, :, :]                            # fp32 products [nq, nlist, D]
    n = (c * c)[None]                                            # [1, nlist, D]

    def seq(x, idx):
        acc = np.zeros(x.shape[:2], F32)
        for j in idx:
            acc = acc + x[:, :, j]
        return acc

    def pairwise(x):
        while x.shape[2] > 1:
            x = x[:, :, 0::2] + x[:, :, 1::2]
        return x[:, :, 0]

    def blocked(x):
        parts = [seq(x, range(b, b + 16)) for b in range(0, x.shape[2], 16)]
        acc = np.zeros(x.shape[:2], F32)
        for part in parts:
            acc = acc + part
        return acc
    D = q.shape[1]
    sums = {"sequential": lambda x: seq(x, range(D)), "reversed": lambda x: seq(x, range(D - 1, -1, -1)),
            "pairwise": pairwise, "blocked": blocked}
    out = {}
    for name, f in sums.items():
        s = F32(2) * f(p) - f(n)
        assert s.dtype == F32
        out[name] = s
    return out


@pytest.mark.parametrize("family", PROBE_FAMILIES)
def test_probe_bound_holds_in_four_summation_orders(family):
    """The bound of `probe_bound` against numpy fp32 emulations of the library's expression in four accumulation orders; the
    reference is fp64.  The exact family must come out with no error at all."""
    for nlist in PROBE_NLISTS:
        q, c, exact = _probe_family(family, nlist)
        want = 2.0 * q.astype(F64) @ c.astype(F64).T - (c.astype(F64) ** 2).sum(1)[None]
        B = probe_bound(q, c)
        ratios = {}
        for name, s in _fp32_scores_in_four_orders(q, c).items():
            err = np.abs(s.astype(F64) - want)
            ratios[name] = float((err / B).max())
            if exact:
                assert (err == 0).all(), (family, nlist, name)
        print(f"\n[probe bound {family} nlist={nlist}] worst err / B: " + "  ".join(f"{n} {r:.3g}" for n, r in ratios.items()))
        assert max(ratios.values()) < 1.0, (family, nlist, ratios)


def _probe_truth(q, c, exact, nprobe):
    """(oracle cells nearest first [nq, nprobe], d64 [nq, nlist], kth [nq], B_q [nq], decisive [nq])"""
    order, d = pq_oracle.ivf_probe_l2(q, c, nprobe)
    nlist = c.shape[0]
    Bq = np.zeros(len(q)) if exact else probe_bound(q, c).max(1)
    ds = np.sort(d, 1)
    kth = ds[:, nprobe - 1]
    nxt = ds[:, nprobe] if nprobe < nlist else np.full(len(q), np.inf)
    decisive = np.ones(len(q), bool) if exact else (nxt - kth > 2 * Bq)
    return order, d, kth, Bq, decisive


def _assert_decisive(q, coarse, nprobe):
    _, _, _, _, decisive = _probe_truth(q, coarse, False, min(nprobe, coarse.shape[0]))
    assert decisive.all(), "a query's probe set is not decided by fp64: the comparison with the oracle would be a coin toss"


def _nprobes(nlist):
    return (1, 8, nlist - 1, nlist)


@pytest.mark.parametrize("family", PROBE_FAMILIES)
def test_probe_families_can_be_checked(family):
    """At least three quarters of the (query, nprobe) pairs of every family and list count are decisive — a family whose probe
    sets fp64 cannot decide would pass the GPU test without testing anything.  The equidistant family: a true tie at rank 8 | 9
    for every query, the origin nearest."""
    for nlist in PROBE_NLISTS:
        q, c, exact = _probe_family(family, nlist)
        dec = np.array([_probe_truth(q, c, exact, n)[4] for n in _nprobes(nlist)])
        if exact:
            d = np.sort(pq_oracle.ivf_probe_l2(q, c, nlist)[1], 1)
            assert (d[:, 7] == d[:, 8]).all() and (d[:, 0] < d[:, 1]).all()
            assert (pq_oracle.ivf_probe_l2(q, c, 1)[0][:, 0] == 0).all()
            dec = np.array([_probe_truth(q, c, False, n)[4] for n in _nprobes(nlist)])     # by the bound: the ties are NOT decisive
            assert not dec[1].any()
            continue
        print(f"\n[probe families {family} nlist={nlist}] decisive (query, nprobe) pairs: {dec.mean():.3f}")
        assert dec.mean() >= 0.75, (family, nlist, dec.mean(1))


@pytest.mark.gpu
@pytest.mark.parametrize("nlist", PROBE_NLISTS)
@pytest.mark.parametrize("family", PROBE_FAMILIES)
def test_l2_probes_against_fp64(family, nlist):
    """`IVFPQIndex.probe` under METRIC_L2 against the fp64 distances: every probed cell within 2 B_q of the nprobe-th smallest
    distance; where the gap to the next cell exceeds 2 B_q the set IS the oracle's; ordered=False = that set ascending;
    ordered=True = the same set, nearest first up to 2 B_q.  The exact family: the oracle's cells in the oracle's order, the
    lower id of two equidistant cells first and, at the boundary, alone."""
    from repconc_amd.ivf import IVFPQIndex
    q, c, exact = _probe_family(family, nlist)
    ivf = IVFPQIndex(PROBE_D, 16, nlist, device=torch.device(DEV), metric=L2)
    ivf.coarse = _t(c)
    dq = _t(q)
    rows = np.arange(len(q))[:, None]
    for nprobe in _nprobes(nlist):
        order, d, kth, Bq, decisive = _probe_truth(q, c, exact, nprobe)
        got = ivf.probe(dq, nprobe, ordered=False).cpu().numpy()
        assert got.shape == (len(q), nprobe) and got.dtype == np.int32
        assert (np.diff(got, axis=1) > 0).all() and got.min() >= 0 and got.max() < nlist
        assert (d[rows, got] <= (kth + 2 * Bq)[:, None]).all(), (family, nlist, nprobe)
        assert np.array_equal(got[decisive], np.sort(order, 1)[decisive]), (family, nlist, nprobe)
        ranked = ivf.probe(dq, nprobe, ordered=True).cpu().numpy()
        assert np.array_equal(np.sort(ranked, 1), got), (family, nlist, nprobe)
        dr = d[rows, ranked]
        assert (dr[:, :-1] <= dr[:, 1:] + 2 * Bq[:, None]).all(), (family, nlist, nprobe)
        if exact:
            assert np.array_equal(ranked, order), (family, nlist, nprobe)


@pytest.mark.gpu
def test_l2_norm_cache_follows_the_coarse_table():
    """The cached ||c_l||^2: a new `coarse` tensor, an in-place write and `to()` each give the probes of the table that is there;
    `to()` of an index whose cache is warm neither shares nor keeps it."""
    from repconc_amd.ivf import IVFPQIndex
    q, c, _ = _probe_family("norms_x8", 64)
    rng = np.random.default_rng(77)
    c2 = (rng.standard_normal(c.shape) * rng.uniform(0.25, 2.0, (64, 1))).astype(F32)           # other norms, other cells
    c3 = c.copy()
    c3[5] *= 0.125                                                                              # one cell pulled to the origin

    def check(ivf, table, what):
        for nprobe in (1, 8):
            order, _, _, _, decisive = _probe_truth(q, table, False, nprobe)
            assert decisive.mean() >= 0.75, what
            got = ivf.probe(_t(q), nprobe, ordered=False).cpu().numpy()
            assert np.array_equal(got[decisive], np.sort(order, 1)[decisive]), (what, nprobe)

    o1, o2, o3 = (np.sort(_probe_truth(q, t, False, 8)[0], 1) for t in (c, c2, c3))
    assert not np.array_equal(o1, o2) and not np.array_equal(o1, o3)                           # a stale cache would show
    ivf = IVFPQIndex(PROBE_D, 16, 64, device=torch.device(DEV), metric=L2)
    ivf.coarse = _t(c)
    check(ivf, c, "first table")
    ivf.coarse = _t(c2)
    check(ivf, c2, "new tensor")
    ivf.coarse.copy_(_t(c3))
    check(ivf, c3, "in-place write")
    moved = ivf.to(torch.device(DEV))                                                          # the source's cache is warm
    check(moved, c3, "to()")
    assert moved._coarse_sq[2] is None or moved._coarse_sq[2].data_ptr() != ivf._coarse_sq[2].data_ptr()
    moved.coarse.copy_(_t(c))                                                                  # the copy's table changes alone
    check(moved, c, "copy written in place")
    check(ivf, c3, "source after the copy was written")
    ivf.coarse.copy_(_t(c2))
    check(ivf, c2, "source written in place")
    check(moved, c, "copy after the source was written")
    check(ivf.to(torch.device(DEV)), c2, "second to()")


# ----------------------------------------------------------------------------------- 3. every route, every repair path
def _spy_search(monkeypatch):
    """Records (queries, k, method) of every `IVFPQIndex.search` call; the inner calls are the per-query scan of a repair path
    (method "scan", the k of the outer call) and the one-query warm-up of a list search (k <= 16)."""
    from repconc_amd.ivf import IVFPQIndex
    calls, orig = [], IVFPQIndex.search

    def spy(self, x, k, nprobe=None, method="auto"):
        calls.append((int(x.shape[0]), int(k), method))
        return orig(self, x, k, nprobe, method)
    monkeypatch.setattr(IVFPQIndex, "search", spy)
    return calls


def _spy_method(monkeypatch, name, record=lambda *a, **kw: 1):
    from repconc_amd.ivf import IVFPQIndex
    calls, orig = [], getattr(IVFPQIndex, name)

    def spy(self, *a, **kw):
        calls.append(record(*a, **kw))
        return orig(self, *a, **kw)
    monkeypatch.setattr(IVFPQIndex, name, spy)
    return calls


def _spy_lib(monkeypatch, *names):
    from repconc_amd import _lib
    lib, counts = _lib.load(), {}
    for name in names:
        counts[name] = 0

        def wrap(*a, _f=getattr(lib, name), _n=name):
            counts[_n] += 1
            return _f(*a)
        monkeypatch.setattr(lib, name, wrap)
    return counts


@functools.lru_cache(maxsize=None)
def _base():
    """M = 16, D = 128, 60 000 rows in 16 cells, 19 queries; the centroids of test_adc_l2._case (norms spread 0.25 .. 2: the
    nearest row is not the best-scoring row).  Read-only."""
    M, D, N, nlist, nq = 16, 128, 60000, 16, 19
    C, codes, q = _case(M, D, N, nq, 2100)
    rng = np.random.default_rng(2101)
    cells = rng.integers(0, nlist, N)
    coarse = rng.standard_normal((nlist, D)).astype(F32)
    for a in (C, codes, q, cells, coarse):
        a.setflags(write=False)
    return SimpleNamespace(M=M, D=D, N=N, nlist=nlist, nq=nq, C=C, codes=codes, q=q, cells=cells, coarse=coarse)


@functools.lru_cache(maxsize=None)
def _base_want(metric, k, nprobe):
    b = _base()
    if metric == L2:
        _assert_decisive(b.q, b.coarse, nprobe)
    return pq_oracle.ivf_search(b.q, b.C, b.codes, b.cells, b.coarse, k, nprobe, metric)


@functools.lru_cache(maxsize=None)
def _degenerate():
    b = _base()
    rng = np.random.default_rng(2201)
    three = rng.integers(0, 256, (3, b.M), dtype=np.uint8)
    codes = three[rng.integers(0, 3, b.N)]
    q = b.q[:5].copy()
    q[2] = pq_oracle.decode(three[1:2], b.C)[0]                  # query 2 IS the reconstruction of the second row
    want = {}
    for nprobe in (4, b.nlist):
        _assert_decisive(q, b.coarse, nprobe)
        want[nprobe] = pq_oracle.ivf_search(q, b.C, codes, b.cells, b.coarse, 200, nprobe, L2)
    return codes, q, want


@pytest.mark.gpu
@pytest.mark.parametrize("method", ["lists", "lists8", "lists16", "scan"])
def test_l2_degenerate_cells(method, monkeypatch):
    """Three distinct code rows over 60 000 rows in 16 cells, k = 200.  Probing every cell, ~20 000 rows tie at every query's k-th
    distance: the scan reports status bit 2 and `_search_exact_probed` answers (its `_flip` takes the flat entry's distances back
    to s); a list search flags every query and repairs it through that scan (`_flip` of the flagged-query repair).  One query is
    the reconstruction of one of the rows: its leading distances are +0.0f, ids ascending by corpus id across the cells."""
    b = _base()
    codes, q, want = _degenerate()
    ivf = _index(b.C, b.coarse, codes, b.cells)
    exact = _spy_method(monkeypatch, "_search_exact_probed", lambda q_, *a: int(q_.shape[0]))
    calls = _spy_search(monkeypatch)
    for nprobe in (4, b.nlist):
        del exact[:], calls[:]
        got = ivf.search(_t(q), 200, nprobe, method=method)
        wd, wi = want[nprobe]
        _same(got, want[nprobe], (method, nprobe))
        assert (wd.view(np.uint32)[2, :200] == 0).all() and (np.diff(wi[2]) > 0).all()          # (the oracle itself)
        assert len(set(b.cells[wi[2]].tolist())) > 1
        assert (_bits(got[0])[2] == 0x00000000).all() and (np.diff(_np(got[1])[2]) > 0).all()
        if nprobe == b.nlist:
            assert sum(exact) >= len(q), (method, exact)                                        # the path without any list ran
            if method != "scan":
                repairs = [c for c in calls if c[2] == "scan" and c[1] == 200]
                assert repairs and sum(c[0] for c in repairs) >= len(q), calls


@pytest.mark.gpu
def test_l2_one_degenerate_query_is_answered_alone(monkeypatch):
    """The geometry of test_ivf_one_degenerate_query_is_answered_alone built for L2, nprobe = 1: query 7 sits ON the centroid of
    a cell of 40 000 copies of one row and is flagged alone; the others keep the list search's answer.  Query 20 sits on the
    centroid of a cell of 5 rows: its tail is +inf / -1 after the repair wrote its rows of the shared output."""
    M, D, nlist, N, nq, k = 16, 128, 24, 150000, 33, 300
    C, codes, q = _case(M, D, N, nq, 2300)
    rng = np.random.default_rng(2301)
    cells = rng.integers(1, nlist - 1, N)
    cells[:40000] = 0
    codes[:40000] = codes[0]
    cells[40000:40005] = nlist - 1
    coarse = (0.5 * rng.standard_normal((nlist, D))).astype(F32)     # ~1.25 D from a query; q[7], q[20] are ~2 D from the others
    coarse[0], coarse[nlist - 1] = q[7], q[20]
    _assert_decisive(q, coarse, 1)
    want = pq_oracle.ivf_search(q, C, codes, cells, coarse, k, 1, L2)
    assert (want[1][7] == np.arange(k)).all() and len(set(want[0][7].tolist())) == 1
    assert (want[1][20, :5] >= 40000).all() and (want[1][20, 5:] == -1).all() and np.isposinf(want[0][20, 5:]).all()
    sizes = np.bincount(cells, minlength=nlist)
    assert (sizes[1:nlist - 1] > 4096).all()                          # the other queries are thresholded (KEEP_ALL_ROWS)
    ivf = _index(C, coarse, codes, cells)
    assert ivf.KEEP_ALL_ROWS == 4096
    calls = _spy_search(monkeypatch)
    for method in ("lists8", "lists16"):
        del calls[:]
        got = ivf.search(_t(q), k, 1, method=method)
        _same(got, want, method)
        gd, gi = _np(got[0]), _np(got[1])
        assert np.isposinf(gd[20, 5:]).all() and (gi[20, 5:] == -1).all()
        repairs = [c for c in calls if c[2] == "scan" and c[1] == k]
        print(f"\n[one degenerate query, {method}] inner search calls: {calls[1:]}")
        assert repairs and all(c[0] < nq // 2 for c in repairs), calls                         # the flagged few, and they ran


@pytest.mark.gpu
def test_l2_survivor_stream_overflow(monkeypatch):
    """RC_IVF_STREAM_CAP = 16: a wave's survivor stream holds 16 pairs, and the 24 x 500 rows the queries must keep exceed what all
    the streams of the call's 40-odd tasks hold together, whatever the slack.  Every attempt reports status bit 2, the search
    narrows the slack max_retries times and the per-query scan answers: the final `_flip` of `_search_lists` and of
    `_search_lists_host_plan` takes its distances back to s."""
    M, D, nlist, N, nq, k, nprobe = 16, 128, 40, 120000, 24, 500, 10
    C, codes, q = _case(M, D, N, nq, 2400)
    rng = np.random.default_rng(2401)
    cells = rng.integers(0, nlist, N)
    coarse = rng.standard_normal((nlist, D)).astype(F32)
    _assert_decisive(q, coarse, nprobe)
    want = pq_oracle.ivf_search(q, C, codes, cells, coarse, k, nprobe, L2)
    ivf = _index(C, coarse, codes, cells)
    monkeypatch.setenv("RC_IVF_STREAM_CAP", "16")
    entry = {"lists8": "rc_ivf_search_probes_q", "lists16": "rc_ivf_search_probes_q16", "lists_host_plan": "rc_ivf_search_lists"}
    counts = _spy_lib(monkeypatch, *entry.values())
    flips = _spy_method(monkeypatch, "_flip", lambda v: tuple(v.shape))
    calls = _spy_search(monkeypatch)
    for method in ("lists8", "lists16", "lists_host_plan"):
        del flips[:], calls[:]
        before = counts[entry[method]]
        _same(ivf.search(_t(q), k, nprobe, method=method), want, method)
        assert counts[entry[method]] - before == 4, (method, counts)                             # the first attempt and three retries
        assert (nq, k, "scan") in calls, (method, calls)                                        # then the scan, for every query
        # s -> d at the end of the inner scan call, d -> s in the fall-through, s -> d at the end of the outer call
        assert flips.count((nq, k)) == 3, (method, flips)


@pytest.mark.gpu
def test_l2_lists_host_plan(monkeypatch):
    """`lists_host_plan` under L2 equals `lists8` and the oracle; with a slack of -3 standard deviations (threshold rank 6 where
    12.5 of the 100 best are expected in the sample) queries keep too few candidates, the entry reports status bit 0 and the
    `st & 1` branch widens the slack: the entry runs more than once and no per-query scan is needed."""
    b = _base()
    k, nprobe = 100, 4
    want = _base_want(L2, k, nprobe)
    ivf = _index(b.C, b.coarse, b.codes, b.cells)
    dq = _t(b.q)
    _same(ivf.search(dq, k, nprobe, method="lists_host_plan"), want, "host plan")
    _same(ivf.search(dq, k, nprobe, method="lists8"), want, "lists8")
    counts = _spy_lib(monkeypatch, "rc_ivf_search_lists")
    calls = _spy_search(monkeypatch)
    probes = ivf.probe(dq, nprobe, ordered=False)
    s, i = ivf._search_lists_host_plan(dq, probes, k, nprobe, sel_slack=-3.0)
    assert counts["rc_ivf_search_lists"] >= 2 and not calls, (counts, calls)
    assert (_np(s)[:, 0] <= 0).all()                                                           # the internal form: s = -d
    _same((ivf._flip(s), i), want, "host plan, repeated")


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [IP, L2])
def test_search_scores_in_chunks(metric, monkeypatch):
    """MAX_QUERY_BATCH = 7 with 19 queries: three chunks, the same answer as the one call (and the oracle's)."""
    from repconc_amd.ivf import IVFPQIndex
    b = _base()
    k, nprobe = 50, 4
    want = _base_want(metric, k, nprobe)
    ivf = _index(b.C, b.coarse, b.codes, b.cells, metric)
    whole = {m: ivf.search(_t(b.q), k, nprobe, method=m) for m in ("lists8", "scan")}
    monkeypatch.setattr(IVFPQIndex, "MAX_QUERY_BATCH", 7)
    sizes = _spy_method(monkeypatch, "_search_scores", lambda q_, *a, **kw: int(q_.shape[0]))
    for m, one in whole.items():
        del sizes[:]
        got = ivf.search(_t(b.q), k, nprobe, method=m)
        assert sizes[0] == 19 and sorted(n for n in sizes[1:] if n > 1) == [5, 7, 7], sizes
        _same(got, (_np(one[0]), _np(one[1])), (m, "chunked vs whole"))
        _same(got, want, (m, "oracle"))


@pytest.mark.gpu
def test_l2_auto_routing_on_either_side_of_lists_min_bytes(monkeypatch):
    """`auto` takes the list search from LISTS_MIN_BYTES average probed code bytes per query (576 000: 36 000 rows at M = 16).
    60 000 rows in 16 cells at nprobe 10: 37 500 rows, the list search; 57 000 rows: 35 625, the per-query scan.  Same answers
    as the forced routes and the oracle."""
    b = _base()
    k, nprobe = 50, 10
    _assert_decisive(b.q, b.coarse, nprobe)
    lists = _spy_method(monkeypatch, "_search_lists")
    for N, route in ((b.N, "lists"), (57000, "scan")):
        ivf = _index(b.C, b.coarse, b.codes[:N], b.cells[:N])
        assert (N * nprobe / b.nlist * b.M >= ivf.LISTS_MIN_BYTES) == (route == "lists")
        want = pq_oracle.ivf_search(b.q, b.C, b.codes[:N], b.cells[:N], b.coarse, k, nprobe, L2)
        del lists[:]
        got = ivf.search(_t(b.q), k, nprobe)
        assert len(lists) == (1 if route == "lists" else 0), (N, route, lists)
        _same(got, want, ("auto", N))
        _same(ivf.search(_t(b.q), k, nprobe, method="scan"), want, ("scan", N))
        del lists[:]
        _same(ivf.search(_t(b.q), k, nprobe, method="lists"), want, ("lists", N))
        assert len(lists) == 1


@pytest.mark.gpu
def test_l2_replicated_index_and_add():
    """`IVFPQIndex.add` (nearest codes, nearest cell) then search, and `ReplicatedIVFPQIndex(ivf, devices=[0, 0])`, under L2:
    numpy in / numpy out and tensor in / tensor out, against the oracle on the codes and cells the index holds."""
    from repconc_amd.ivf import IVFPQIndex
    from repconc_amd.multi_index import ReplicatedIVFPQIndex
    from repconc_amd.sharded_search import sharded_search
    M, D, N, nq, nlist, k, nprobe = 16, 128, 20000, 9, 16, 50, 4
    C, codes0, q = _case(M, D, N, nq, 2500)
    rng = np.random.default_rng(2501)
    x = (pq_oracle.decode(codes0, C) + 0.05 * rng.standard_normal((N, D))).astype(F32)
    coarse = x[rng.choice(N, nlist, replace=False)].copy()
    ivf = IVFPQIndex(D, M, nlist, device=torch.device(DEV), metric=L2)
    ivf.set_centroids(_t(C))
    ivf.coarse = _t(coarse)
    ivf.add(x)
    assert ivf.ntotal == N
    corpus = ivf.ids.cpu().numpy()
    codes, cells = np.empty((N, M), np.uint8), np.empty(N, np.int64)
    codes[corpus] = ivf.codes.cpu().numpy()
    cells[corpus] = np.repeat(np.arange(nlist), np.diff(ivf.list_off.cpu().numpy()))
    assert np.array_equal(np.sort(corpus), np.arange(N)) and len(set(cells.tolist())) > 1
    _assert_decisive(q, coarse, nprobe)
    want = pq_oracle.ivf_search(q, C, codes, cells, coarse, k, nprobe, L2)
    assert (np.diff(want[0], axis=1) >= 0).all() and (want[0] >= 0).all()
    multi = ReplicatedIVFPQIndex(ivf, devices=[0, 0])
    assert multi.metric_type == L2 and [p.metric_type for p in multi.parts] == [L2, L2] and multi.ntotal == N
    for name, index in (("ivf", ivf), ("replicated", multi)):
        for method in ("auto", "lists8", "scan"):
            d, i = index.search(q, k, nprobe, method)                               # numpy in, numpy out
            assert isinstance(d, np.ndarray) and isinstance(i, np.ndarray) and d.dtype == F32 and i.dtype == np.int64
            _same((d, i), want, (name, method, "numpy"))
            d, i = index.search(_t(q), k, nprobe, method)                           # tensor in, tensor out
            assert isinstance(d, torch.Tensor) and isinstance(i, torch.Tensor) and d.is_cuda and i.is_cuda
            assert d.dtype == torch.float32 and i.dtype == torch.int64
            _same((d, i), want, (name, method, "tensor"))
    # the attribute `sharded_search` reads: one rank, the index's own answer
    multi.nprobe = nprobe
    _same(sharded_search(multi, _t(q), k), want, "sharded_search")


# ------------------------------------------------------------------------------- 4. edges of the public surface, both metrics
@functools.lru_cache(maxsize=None)
def _edge_index_case(metric):
    """3 000 rows in cells 0 .. 5 of 8; cells 6 and 7 are empty and query 5 probes exactly those two at nprobe = 2."""
    M, D, N, nq, nlist = 16, 128, 3000, 6, 8
    C, codes, q = _case(M, D, N, nq, 2600)
    rng = np.random.default_rng(2601)
    cells = rng.integers(0, 6, N)
    coarse = rng.standard_normal((nlist, D)).astype(F32)
    if metric == L2:
        coarse[6] = q[5]
        coarse[7] = q[5] + (0.01 * rng.standard_normal(D)).astype(F32)
        _assert_decisive(q, coarse, 2)
    else:
        coarse[6], coarse[7] = 8.0 * q[5], 7.0 * q[5]
        cs = np.sort(q.astype(F64) @ coarse.astype(F64).T, 1)
        assert (cs[:, -2] - cs[:, -3] > 1e-2).all()                  # the fp32 product decides the two best cells as fp64 does
    order = pq_oracle.ivf_probe_l2(q, coarse, 2)[0] if metric == L2 else np.argsort(-(q.astype(F64) @ coarse.astype(F64).T), 1)[:, :2]
    assert set(order[5].tolist()) == {6, 7}
    for a in (C, codes, q, cells, coarse):
        a.setflags(write=False)
    return C, codes, q, cells, coarse


def _empty_answer(got, nq, k, metric, tensor):
    d, i = got
    assert isinstance(d, torch.Tensor) == tensor and isinstance(i, torch.Tensor) == tensor
    d, i = _np(d), _np(i)
    assert d.shape == (nq, k) and i.shape == (nq, k) and d.dtype == F32 and i.dtype == np.int64
    assert (i == -1).all() and ((np.isposinf(d) if metric == L2 else np.isneginf(d))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [IP, L2])
def test_search_without_queries_or_without_rows(metric):
    """nq == 0 and ntotal == 0 (lists set from empty codes), every method: (nq, k) float32 / int64, -inf / -1 for the inner
    product and +inf / -1 for L2, no exception."""
    C, codes, q, cells, coarse = _edge_index_case(metric)
    q = q.copy()                                                                    # (numpy in: the shared case is read-only)
    ivf = _index(C, coarse, codes, cells, metric)
    empty = _index(C, coarse, codes[:0], cells[:0], metric)
    assert empty.ntotal == 0 and empty.list_off.cpu().numpy().tolist() == [0] * 9
    for method in METHODS:
        for index in (ivf, empty):
            _empty_answer(index.search(_t(q[:0]), 7, 2, method), 0, 7, metric, True)
            _empty_answer(index.search(q[:0], 7, 2, method), 0, 7, metric, False)
        _empty_answer(empty.search(_t(q), 7, 2, method), len(q), 7, metric, True)
        _empty_answer(empty.search(q, 7, 100, method), len(q), 7, metric, False)
    _empty_answer(ivf.search(_t(q[:0]), 7), 0, 7, metric, True)                     # the index's own nprobe
    with pytest.raises(ValueError):
        ivf.search(_t(q[:0]), 7, 2, "nonsense")


@pytest.mark.gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("metric", [IP, L2])
def test_search_edges_of_nprobe_k_and_empty_cells(metric, method):
    """nprobe > nlist (= every cell), a k larger than every probed row count, and a query that probes only empty cells — in a
    batch and alone: the oracle's rows, then -inf | +inf / -1."""
    C, codes, q, cells, coarse = _edge_index_case(metric)
    ivf = _index(C, coarse, codes, cells, metric)
    N, nlist = len(codes), coarse.shape[0]
    pad = np.isposinf if metric == L2 else np.isneginf
    want = pq_oracle.ivf_search(q, C, codes, cells, coarse, 40, nlist, metric)
    _same(ivf.search(_t(q), 40, nlist + 5, method), want, "nprobe > nlist")
    want = pq_oracle.ivf_search(q, C, codes, cells, coarse, N + 100, nlist, metric)
    assert (want[1][:, N:] == -1).all() and pad(want[0][:, N:]).all() and (want[1][:, N - 1] >= 0).all()
    _same(ivf.search(_t(q), N + 100, 100, method), want, "nprobe > nlist, k > N")
    want = pq_oracle.ivf_search(q, C, codes, cells, coarse, 2000, 2, metric)        # two cells: ~1000 rows
    # (under the inner product another query may take the two empty cells too: their centroids are long)
    assert (want[1][:, -1] == -1).all() and ((want[1][:5, 0] >= 0).all() if metric == L2 else (want[1][:5, 0] >= 0).sum() >= 3)
    assert (want[1][5] == -1).all() and pad(want[0][5]).all()                       # query 5: two empty cells
    _same(ivf.search(_t(q), 2000, 2, method), want, "k > probed rows, one query on empty cells")
    _same(ivf.search(_t(q[5:6]), 10, 2, method), (want[0][5:6, :10], want[1][5:6, :10]), "only empty cells, alone")


# ------------------------------------------------------------- 5. L2 tables that strain the screen, made by rc_adc_lut_l2
STRAIN_N = (1 << 18) + 16
STRAIN_IVF_N, STRAIN_NLIST, STRAIN_K = 60000, 16, 100
# group -> (families of 8 queries, nprobe of the IVF run).  A group shares one codebook, hence one index and one oracle run.
STRAIN_GROUPS = {"base": (("control", "offset_1e2", "offset_1e4"), 4),
                 "subspace_x1e3": (("subspace_x1e3",), 4),
                 "identical_subquantiser": (("identical_subquantiser",), 4),
                 "scaled_2^-70": (("scaled_2^-70",), STRAIN_NLIST),
                 "scaled_2^-80": (("scaled_2^-80",), STRAIN_NLIST),
                 "scaled_2^55": (("scaled_2^55",), STRAIN_NLIST)}


def _topk_l2(s, k, ids=None):
    """`l2_topk` of a long score row without sorting all of it: the rows at or above the k-th score, then the same lexsort."""
    nq, n = s.shape
    d = np.full((nq, k), np.inf, F32)
    out = np.full((nq, k), -1, np.int64)
    for j in range(nq):
        kk = min(k, n)
        thr = np.partition(s[j], n - kk)[n - kk]
        cand = np.nonzero(s[j] >= thr)[0]
        o = cand[np.lexsort((cand, -s[j, cand].astype(F64)))[:kk]]
        d[j, :kk] = F32(0) - s[j, o]
        out[j, :kk] = o if ids is None else ids[o]
    return d, out


@functools.lru_cache(maxsize=None)
def _strain(group):
    """Inputs of one group and the oracle's answers: flat over STRAIN_N rows, IVF over the first STRAIN_IVF_N rows in 16 cells.
    The coarse centroids are the first 16 unit vectors (scaled with the inputs where those are scaled by 2^55): the probe score
    2 q_l c - c^2 has ONE product, so fp32 orders the cells as fp64 does wherever the 4th and 5th largest q_l differ by more than
    rounding (checked); the scaled groups probe every cell."""
    M, D = 16, 128
    families, nprobe = STRAIN_GROUPS[group]
    C, codes, _ = _case(M, D, STRAIN_N, 1, 2700)
    rng = np.random.default_rng(2701)
    C = C.copy()
    scale = 1.0
    if group == "subspace_x1e3":
        C[5] *= F32(1e3)                                           # one dominant table range
    elif group == "identical_subquantiser":
        C[9] = C[9, 0]                                             # a table of zero range
    elif group.startswith("scaled_"):
        scale = {"scaled_2^-70": 2.0 ** -70, "scaled_2^-80": 2.0 ** -80, "scaled_2^55": 2.0 ** 55}[group]
        C = (C * F32(scale)).astype(F32)
    qs = []
    for fam in families:
        q = rng.standard_normal((8, D))
        if fam.startswith("offset_"):                              # at distance R from the whole codebook: a common offset in every table
            u = rng.standard_normal((8, D))
            q = q + float(fam[7:]) * u / np.linalg.norm(u, axis=1, keepdims=True)
        qs.append((q * scale).astype(F32))
    q = np.concatenate(qs)
    S = pq_oracle.adc_lut_l2(q, C)
    assert np.isfinite(S).all() and np.isfinite(q).all() and np.isfinite(C).all()
    s = pq_oracle.adc_scores(S, codes)
    assert np.isfinite(s).all()
    if group == "scaled_2^-80":
        assert (S.view(np.uint32) == 0).all() and (s.view(np.uint32) == 0).all()               # every T is +0.0f: every distance ties
    if group == "scaled_2^-70":
        assert (np.abs(S) < 2.0 ** -126).all() and (S != 0).any()                              # every T is subnormal: inexact, not zero
    if group == "scaled_2^55":
        assert s.min() < -2.0 ** 110
    flat = _topk_l2(s, STRAIN_K)
    cells = rng.integers(0, STRAIN_NLIST, STRAIN_IVF_N)
    coarse = np.zeros((STRAIN_NLIST, D), F32)
    coarse[np.arange(STRAIN_NLIST), np.arange(STRAIN_NLIST)] = F32(scale) if scale > 1 else F32(1)
    if nprobe < STRAIN_NLIST:
        ql = np.sort(q[:, :STRAIN_NLIST].astype(F64), 1)[:, ::-1]
        assert (ql[:, nprobe - 1] - ql[:, nprobe] > 1e-5 * (1.0 + np.abs(q).max())).all()
    probed, _ = pq_oracle.ivf_probe_l2(q, coarse, nprobe)
    dI = np.full((len(q), STRAIN_K), np.inf, F32)
    iI = np.full((len(q), STRAIN_K), -1, np.int64)
    for j in range(len(q)):
        rows = np.nonzero(np.isin(cells, probed[j]))[0]
        dI[j:j + 1], iI[j:j + 1] = _topk_l2(s[j:j + 1, rows], STRAIN_K, rows)
    for a in (C, codes, q, cells, coarse, *flat, dI, iI):
        a.setflags(write=False)
    return SimpleNamespace(C=C, codes=codes, q=q, cells=cells, coarse=coarse, families=families, nprobe=nprobe, flat=flat,
                           ivf=(dI, iI))


def test_strain_oracle_shortcut_equals_l2_topk():
    """`_topk_l2` (partition, then the oracle's lexsort on the rows at or above the k-th score) is `l2_topk` on rows with ties
    across the k-th place and on a row shorter than k."""
    rng = np.random.default_rng(2800)
    s = -rng.integers(0, 40, (4, 500)).astype(F32)
    for k in (1, 37, 100, 700):
        a, b = _topk_l2(s, k), l2_topk(s, k)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(STRAIN_GROUPS))
def test_l2_strained_tables_flat_screen(group):
    """The flat screened search at N = 2^18 + 16 on tables made by rc_adc_lut_l2 from chosen inputs: ids and distance bits, the
    screen ran (`stats` holds `survivors`).  Survivors and candidates per family are printed, not fixed — except survivors < N on
    the control.  Inputs scaled by 2^-80: every T is +0.0f, all distances tie, the exact route answers ids 0 .. k-1.  Scaled by
    2^-70 every T underflows to a subnormal — inexact but not zero, so the distances do NOT all tie: the oracle's answer holds."""
    from repconc_amd import ops
    c = _strain(group)
    stats = {}
    pend = ops.adc_search(_t(c.codes), _t(c.C), _t(c.q), STRAIN_K, metric=L2, defer=True, stats=stats)
    got = pend.result()
    assert "survivors" in stats, "the 8-bit screen did not run"
    surv, cand = stats["survivors"].cpu().numpy(), stats["candidates"].cpu().numpy()
    for f, fam in enumerate(c.families):
        print(f"\n[strained flat {fam}] survivors {surv[8 * f:8 * f + 8].tolist()} candidates {cand[8 * f:8 * f + 8].tolist()} "
              f"retried {pend.stats['retried_queries']} exact {pend.stats['exact_queries']}")
        if fam == "control":
            assert (surv[8 * f:8 * f + 8] < STRAIN_N).all()
    _same(got, c.flat, group)
    if group == "scaled_2^-80":
        assert pend.stats["exact_queries"] == len(c.q), pend.stats
        assert np.array_equal(_np(got[1]), np.broadcast_to(np.arange(STRAIN_K), (len(c.q), STRAIN_K)))
        assert (_bits(got[0]) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(STRAIN_GROUPS))
def test_l2_strained_tables_ivf_lists(group, monkeypatch):
    """The same tables through the IVF list search (both widths) at 60 000 rows in 16 cells."""
    c = _strain(group)
    ivf = _index(c.C, c.coarse, c.codes[:STRAIN_IVF_N], c.cells)
    calls = _spy_search(monkeypatch)
    for method in ("lists8", "lists16"):
        del calls[:]
        got = ivf.search(_t(c.q), STRAIN_K, c.nprobe, method=method)
        repaired = sum(n for n, k, m in calls if m == "scan" and k == STRAIN_K)
        print(f"\n[strained ivf {group} {method}] queries answered again by the per-query scan: {repaired} of {len(c.q)}")
        _same(got, c.ivf, (group, method))
    if group == "scaled_2^-80":
        assert np.array_equal(c.ivf[1], np.broadcast_to(np.arange(STRAIN_K), (len(c.q), STRAIN_K)))
