"""The 8-bit search screens on tables that strain their integer bound (adc_screen_tint, csrc/adc_common.h).

The flat ADC search (N >= 2^18) and the list-centric IVF search quantise a query's tables to bytes with one step per query,
sum bytes and keep a row when the integer sum reaches a threshold derived from the exact fp32 threshold tau_q.  The promise is
that no row whose exact score (fp32, accumulated m-ascending: the oracle's arithmetic) is >= tau_q is dropped.  Every other
search test draws centroids and queries from a zero-mean Gaussian; here the TABLES are chosen: with dsub = 768 / M, table
family j sits in coordinate j of every centroid, C[m, c, j] = table_j[m, c], and query j is 1.0 at coordinate j of every
sub-space, so LUT_j is table_j bit for bit and one index serves up to dsub families in one batch — queries of different
families share a 16-query group of the screen.

Families (FAMILIES): a control, a common offset of either sign and of a random sign per sub-space, a 1e7 offset in the first /
the last sub-space only, one dominant range, constant tables, sub-normal tables, a range that overflows fp32, entries that all
sit just below / just above the middle between two byte levels, and (without the
one-hot construction, through the real table kernel) centroids that share a large common vector.  Every comparison is of uint32
bit patterns against oracle.c_oracle.adc_search / oracle.pq_oracle.ivf_search; no tolerance appears in this file.

What the parent of this file's commit did with them ([MI355X], T_q = ceil((tau - sum lo) / Delta - M / 2) - 2): see the commit
message; in short the equal-sign offsets from 1e5 up returned answers that were not the oracle's with status 0.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle, pq_oracle

F32 = np.float32
DEV = "cuda"
gpu = pytest.mark.gpu

SAMPLE_MAX = 32768          # ADC_SAMPLE_MAX (csrc/topk.h)
CAND_CAP = 16384            # ADC_CAND_CAP (csrc/topk.h)
KBIG = 4096                 # the oracle is asked once per index for this many rows: serves every k and the candidate counts
N_ABOVE = (1 << 18) + 16    # just above ADC_SCREEN_MIN_N (8 whole tiles of 32 768 rows + 16 rows)
N_RAGGED = 300001           # not a multiple of the 32 768-row tile


# ------------------------------------------------------------------------------------------------------------ families
def _base(M, seed=3):
    return np.random.default_rng(1000 * M + seed).standard_normal((M, 256)).astype(F32)


def _signs(M):
    return np.random.default_rng(77 + M).choice([-1.0, 1.0], (M, 1)).astype(F32)


def _offset(o):
    return lambda M: (_base(M) + F32(o)).astype(F32)


def _offset_signed(o):
    return lambda M: (_base(M) + F32(o) * _signs(M)).astype(F32)


def _one_subspace(where, o=1e7):
    def f(M):
        t = _base(M)
        m = 0 if where == "first" else M - 1
        t[m] = (t[m] + F32(o)).astype(F32)          # ulp 1 at 1e7: the sub-space keeps a range of ~6 in whole numbers
        return t
    return f


def _dominant(M):
    t = _base(M)
    t[0] = t[0] * F32(1e6)                          # the other sub-spaces collapse to one or two byte levels
    return t


def _constant(M):
    return np.repeat(_base(M)[:, :1], 256, 1)       # zero range everywhere: the step falls back to 1, every score ties


def _subnormal(M):
    return np.ldexp(_base(M), -140).astype(F32)     # largest range / 255 is a sub-normal with four or five bits


def _overflow(M):
    t = np.zeros((M, 256), F32)
    t[0] = np.where(np.random.default_rng(5 + M).integers(0, 2, 256) == 1, F32(2e38), F32(-2e38))
    t[0, :2] = (2e38, -2e38)                        # hi - lo = inf in fp32, the scores themselves stay finite
    return t


def _grid(frac64):
    """Every entry sits frac64 / 64 of a step above a byte level (step 1/4, lo = -32; codes 0 and 1 pin lo and lo + 255 steps).
    31 / 64: each of a row's M bytes is rounded DOWN by almost the half step the bound allows for — a bound with less than
    M / 2 loses rows.  63 / 64: rounding to nearest goes up; a quantiser that rounds down loses almost M steps.  All values are
    multiples of 2^-8, so the fp32 sums are exact and the scores tie in large groups."""
    def f(M):
        j = np.random.default_rng(40 + M + frac64).integers(0, 255, (M, 256))
        t = (-32.0 + 0.25 * (j + frac64 / 64.0)).astype(F32)
        t[:, 0], t[:, 1] = -32.0, -32.0 + 0.25 * 255
        return t
    return f


FAMILIES = {"control": _offset(0.0)}
for _o in ("1e4", "1e5", "3e5", "1e6", "3e6"):
    FAMILIES["off+" + _o] = _offset(float(_o))
    FAMILIES["off-" + _o] = _offset(-float(_o))
FAMILIES.update({"sign1e5": _offset_signed(1e5), "sign1e6": _offset_signed(1e6), "first1e7": _one_subspace("first"),
                 "last1e7": _one_subspace("last"), "dominant": _dominant, "constant": _constant, "subnormal": _subnormal,
                 "overflow": _overflow, "grid31": _grid(31), "grid63": _grid(63)})
NAMES = list(FAMILIES)


def _table(name, M):
    return np.ascontiguousarray(FAMILIES[name](M) + F32(0.0))        # + 0.0: no -0.0 entry (0.0 + -0.0 = +0.0 in the LUT sum)


def _batches(M):
    """The families in index-sized batches: an index of width M carries dsub = 768 / M of them."""
    dsub = 768 // M
    return [NAMES[i:i + dsub] for i in range(0, len(NAMES), dsub)]


def _onehot(M, names):
    """Centroids [M, 256, dsub], one-hot queries [F, 768] and the tables [F, M, 256] they are meant to produce."""
    dsub = 768 // M
    assert len(names) <= dsub
    tabs = np.stack([_table(n, M) for n in names])
    C = np.zeros((M, 256, dsub), F32)
    q = np.zeros((len(names), 768), F32)
    for j in range(len(names)):
        C[:, :, j] = tabs[j]
        q[j].reshape(M, dsub)[:, j] = 1.0
    return C, q, tabs


def _codes(M, N, dup):
    codes = np.random.default_rng(31 * M + N).integers(0, 256, (N, M), dtype=np.uint8)
    if dup:
        codes[N // 2: N // 2 + 300] = codes[:300]      # duplicated rows: ties across the candidate boundary and rank k
    return codes


# --------------------------------------------------------------------------------- the search's own rules, restated
def _sample_rank(N, S, k, slack):
    """rc_adc_sample_rank (csrc/topk.hip): rank of the sample score that becomes tau."""
    if N <= CAND_CAP:
        return 0
    if S == N:
        return k
    mu = k * S / N
    r = int(mu + slack * np.sqrt(mu + 1.0) + 4.0) + 1
    r_cap = 0.8 * CAND_CAP * S / N
    if r > r_cap and r_cap >= mu + 2.5 * np.sqrt(mu + 1.0) + 2.0:
        r = int(r_cap)
    return max(1, min(r, S))


def _sample_rows(N):
    S = min(N, SAMPLE_MAX)
    return (np.arange(S, dtype=np.int64) * N) // S          # sample row i = corpus row floor(i N / S) (adc_scan_kernel<SAMPLE>)


def _tau(sample_scores, r):
    return F32(-np.inf) if r <= 0 else np.sort(sample_scores)[::-1][r - 1]


def _scores(tab, codes):
    """Exact scores of one table: fp32, m ascending from 0."""
    return pq_oracle.adc_scores(tab[None], codes)[0]


def parent_screen_model(tab, codes, s, k, slack=3.0):
    """numpy restatement of the screen BEFORE the accumulation term entered the bound: bytes by adc_quant8 (fp32 subtract, fp32
    divide, floor(x + 0.5), clamp), T = ceil((tau - sum lo) / Delta - M / 2) - 2 in double.  Returns (score >= tau, S_int >= T).
    Qualifies inputs on the CPU; never the expected value of a GPU test."""
    N, M = codes.shape
    lo = tab.min(1)
    delta = F32((tab.max(1) - lo).astype(F32).max() / F32(255.0))
    if not delta > 0:
        delta = F32(1.0)
    lv = np.floor(((tab - lo[:, None]).astype(F32) / delta).astype(F32) + F32(0.5)).astype(np.int64).clip(0, 255)
    S = np.zeros(N, np.int64)
    for m in range(M):
        S += lv[m, codes[:, m]]
    t = _tau(s[_sample_rows(N)], _sample_rank(N, min(N, SAMPLE_MAX), k, slack))
    T = np.ceil((float(t) - lo.astype(np.float64).sum()) / float(delta) - 0.5 * M) - 2
    return s >= t, S >= T


# ------------------------------------------------------------------------------------------------------- CPU tests
ALL_M = (8, 12, 16, 24, 32, 48, 64, 96)


@pytest.mark.parametrize("M", ALL_M)
def test_onehot_queries_reproduce_the_tables_bit_for_bit(M):
    for names in _batches(M):
        C, q, tabs = _onehot(M, names)
        lut = pq_oracle.adc_lut(q, C)
        assert np.array_equal(lut.view(np.uint32), tabs.view(np.uint32)), names


def test_families_are_what_they_are_meant_to_be():
    """Each family reaches the condition it is there for (asserted on the inputs, M = 96): the control and the small offset
    lose nothing under the parent's formula, the equal-sign offsets from 1e5 up lose rows with score >= tau (the cases have
    teeth), and the degenerate families have the step / range they were built for."""
    M, N, k = 96, N_RAGGED, 1000
    codes = _codes(M, N, False)
    lost = {}
    for name in ("control", "off+1e5", "off-1e5", "off+3e5", "off-3e5", "off+1e6", "off-1e6", "off+3e6", "off-3e6", "first1e7"):
        tab = _table(name, M)
        exact, screen = parent_screen_model(tab, codes, _scores(tab, codes), k)
        lost[name] = int((exact & ~screen).sum())
    print(lost)
    assert lost["control"] == 0
    for name, n in lost.items():
        if name != "control":
            assert n >= 1, (name, lost)
    rng = lambda t: (t.max(1) - t.min(1)).astype(F32)
    assert (rng(_table("constant", M)) == 0).all()
    d = F32(rng(_table("subnormal", M)).max() / F32(255.0))
    assert 0 < d < np.finfo(F32).tiny                                     # a sub-normal step
    with np.errstate(over="ignore"):
        assert np.isinf(rng(_table("overflow", M))[0]) and np.isfinite(_scores(_table("overflow", M), codes[:1000])).all()
    r = rng(_table("dominant", M))
    assert r[0] / 255 > r[1:].max()                                       # every other sub-space: at most two byte levels
    for name in ("first1e7", "last1e7"):
        t = _table(name, M)
        assert np.array_equal(t[0 if name == "first1e7" else M - 1], np.round(t[0 if name == "first1e7" else M - 1]))
    s = _signs(M)
    assert (s == 1).any() and (s == -1).any()
    for name, frac in (("grid31", 31 / 64), ("grid63", 63 / 64)):
        t = _table(name, M).astype(np.float64)
        steps = (t - t.min(1, keepdims=True)) / (rng(_table(name, M)).max() / F32(255.0))
        assert (rng(_table(name, M)) == 63.75).all() and (steps[:, 2:] - np.floor(steps[:, 2:]) == frac).all()
        sc = _scores(_table(name, M), codes[:4096])
        assert np.array_equal(sc.astype(np.float64), _table(name, M).astype(np.float64)[np.arange(M), codes[:4096]].sum(1))


def test_sample_rank_restatement():
    # values worked by hand from the formula in csrc/topk.hip
    assert _sample_rank(300001, 32768, 1000, 3.0) == int(109.2263 + 3 * np.sqrt(110.2263) + 4) + 1 == 145
    assert _sample_rank(300001, 32768, 1, 3.0) == 8 and _sample_rank(10000, 10000, 5, 3.0) == 0


# ------------------------------------------------------------------------------------------------ cases and oracle
class _Case:
    """One index (M, N, codes) with one batch of families, the oracle's answer for its distinct queries and, on demand, the
    number of rows at or above tau_q."""

    def __init__(self, M, N, dup, C, q, tabs, names, codes):
        self.M, self.N, self.C, self.q, self.tabs, self.names, self.codes = M, N, C, q, tabs, names, codes
        self.ws, self.wi = c_oracle.adc_search(codes, C, q, KBIG)
        self.lut = pq_oracle.adc_lut(q, C)
        self.sample = pq_oracle.adc_scores(self.lut, codes[_sample_rows(N)])
        self._full = {}

    def count_at_or_above_tau(self, j, k, slack):
        t = _tau(self.sample[j], _sample_rank(self.N, min(self.N, SAMPLE_MAX), k, slack))
        n = int((self.ws[j] >= t).sum())
        if n < KBIG:
            return n
        if j not in self._full:                                   # more than the oracle was asked for: all the scores
            self._full[j] = pq_oracle.adc_scores(self.lut[j:j + 1], self.codes)[0]
        return int((self._full[j] >= t).sum())


@functools.lru_cache(maxsize=3)
def _flat_case(M, N, dup, b):
    names = _batches(M)[b]
    C, q, tabs = _onehot(M, names)
    return _Case(M, N, dup, C, q, tabs, names, _codes(M, N, dup))


@functools.lru_cache(maxsize=3)
def _dev(M, N, dup, b):
    c = _flat_case(M, N, dup, b)
    return _t(c.codes), _t(c.C), _t(c.q)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _mismatch(scores, ids, case, qsel, k):
    """Queries (positions in qsel) whose answer is not the oracle's: ids and score bits."""
    s, i = scores.cpu().numpy(), ids.cpu().numpy()
    bad = []
    for p, j in enumerate(qsel):
        if not (np.array_equal(i[p], case.wi[j, :k]) and np.array_equal(s[p].view(np.uint32), case.ws[j, :k].view(np.uint32))):
            bad.append(p)
    return bad


SCREENS = {"q16": {}, "mfma": {}, "old": {"RC_ADC_OLD_SCREEN": "1"}, "valu": {}, "valu_env": {"RC_ADC_VALU_SCREEN": "1"}}
# (M, screen, N, duplicated block): the 16-query screen at every width it has, the round-1 matrix screen at the widths that
# have no image and as the A/B partner of a width that has one, the VALU screen at M = 12 and by its switch
FLAT_CONFIGS = [(16, "q16", N_ABOVE, False), (32, "q16", N_RAGGED, True), (48, "q16", N_ABOVE, True), (64, "q16", N_RAGGED, False),
                (96, "q16", N_RAGGED, True), (96, "q16", N_ABOVE, False), (8, "mfma", N_RAGGED, False), (24, "mfma", N_ABOVE, True),
                (96, "old", N_RAGGED, True), (48, "old", N_ABOVE, True), (12, "valu", N_RAGGED, True), (48, "valu_env", N_ABOVE, True)]


def _cyclic(F, nq):
    return [i % F for i in range(nq)]


@gpu
@pytest.mark.parametrize("M,screen,N,dup", FLAT_CONFIGS)
def test_flat_search_on_every_family(M, screen, N, dup, monkeypatch):
    """ops.adc_search and PQIndex.search: 33 and 17 queries (families repeated: every group of 16 mixes families, the last
    group is ragged), the family count and single queries, k = 1, 10, 1000.  With stats= the first pass reports how many rows
    the exact rescoring kept: for every query it did not flag, that is exactly #{n : score_n >= tau_q} — a lost row shows
    there even when it is outside the top-k."""
    from repconc_amd import ops
    from repconc_amd.index import PQIndex
    for name, v in SCREENS[screen].items():
        monkeypatch.setenv(name, v)
    wrong, miscounted = [], []
    for b in range(len(_batches(M))):
        case = _flat_case(M, N, dup, b)
        codes, C, q = _dev(M, N, dup, b)
        F = len(case.names)
        runs = [(_cyclic(F, 33), 1000), (_cyclic(F, 17), 10), (list(range(F)), 1)] + [([j], 10) for j in range(F)]
        for qsel, k in runs:
            st = {}
            pend = ops.adc_search(codes, C, q[qsel].contiguous(), k, defer=True, stats=st)
            flagged = pend._qstatus.cpu().numpy() != 0                       # the first pass's per-query status bits
            s, i = pend.result()
            for p in _mismatch(s, i, case, qsel, k):
                wrong.append((case.names[qsel[p]], len(qsel), k, "ops"))
            cand = st["candidates"].cpu().numpy()
            for p, j in enumerate(qsel):
                if not flagged[p]:
                    want = case.count_at_or_above_tau(j, k, ops.ADC_SEL_SLACK)
                    if int(cand[p]) != want:
                        miscounted.append((case.names[j], len(qsel), k, int(cand[p]), want))
        idx = PQIndex(768, M)
        idx.set_centroids(C)
        idx.add_codes(codes)
        for qsel, k in ((_cyclic(F, 33), 1000), (list(range(F)), 10)):
            s, i = idx.search(q[qsel].contiguous(), k)
            for p in _mismatch(s, i, case, qsel, k):
                wrong.append((case.names[qsel[p]], len(qsel), k, "PQIndex"))
    print("wrong answers (family, queries, k, entry):", sorted(set(wrong)))
    print("candidate counts (family, queries, k, got, want):", sorted(set(miscounted)))
    assert not wrong and not miscounted


def _raw_search(case, dev, qsel, k, slack):
    """rc_adc_search_q with its status word, per-query status bits and the first pass's candidate counts."""
    from repconc_amd import _lib
    lib, h = _lib.load(), _lib.handle(0)
    codes, C, q = dev
    qq = q[qsel].contiguous()
    n, M, N = len(qsel), case.M, case.N
    wsb = lib.rc_adc_search_ws_bytes(N, M, 256, n, k)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=DEV)
    sc = torch.empty((n, k), dtype=torch.float32, device=DEV)
    ids = torch.empty((n, k), dtype=torch.int64, device=DEV)
    status = torch.zeros((1,), dtype=torch.int32, device=DEV)
    qstatus = torch.zeros((n,), dtype=torch.int32, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.rc_adc_search_q(h, codes.data_ptr(), None, N, M, 256, C.data_ptr(), 768, qq.data_ptr(), n, k, 0, float(slack),
                             sc.data_ptr(), ids.data_ptr(), status.data_ptr(), qstatus.data_ptr(), ws.data_ptr(), wsb, stream)
    assert rc == 0
    torch.cuda.synchronize()
    so, co = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.rc_adc_search_ws_counts(N, M, 256, n, ctypes.byref(so), ctypes.byref(co)) == 0
    cand = ws[co.value:co.value + 4 * n].view(torch.int32).cpu().numpy()
    return sc, ids, int(status.item()), qstatus.cpu().numpy(), cand


RAW_CONFIGS = [(96, "q16", N_RAGGED, True), (48, "q16", N_ABOVE, True), (16, "q16", N_ABOVE, False), (24, "mfma", N_ABOVE, True),
               (12, "valu", N_RAGGED, True), (48, "old", N_ABOVE, True), (48, "valu_env", N_ABOVE, True)]


@gpu
@pytest.mark.parametrize("M,screen,N,dup", RAW_CONFIGS)
def test_raw_entry_status_zero_means_the_oracles_answer(M, screen, N, dup, monkeypatch):
    """rc_adc_search_q once per screen kernel, nothing repeated: a query whose answer is the oracle's may carry any status bit,
    a query with status 0 MUST equal the oracle, and its candidate count must be #{n : score_n >= tau_q}.  The status word is
    the OR of the per-query bits."""
    for name, v in SCREENS[screen].items():
        monkeypatch.setenv(name, v)
    silent, miscounted = [], []
    for b in range(len(_batches(M))):
        case = _flat_case(M, N, dup, b)
        F = len(case.names)
        for qsel, k in ((_cyclic(F, 33), 1000), (_cyclic(F, 17), 10), (list(range(F)), 1)):
            s, i, status, qstatus, cand = _raw_search(case, _dev(M, N, dup, b), qsel, k, 3.0)
            assert status == int(np.bitwise_or.reduce(qstatus)) and (qstatus & ~3 == 0).all()
            bad = set(_mismatch(s, i, case, qsel, k))
            for p, j in enumerate(qsel):
                if qstatus[p] != 0:
                    continue
                if p in bad:
                    silent.append((case.names[j], len(qsel), k))
                want = case.count_at_or_above_tau(j, k, 3.0)
                if int(cand[p]) != want:
                    miscounted.append((case.names[j], len(qsel), k, int(cand[p]), want))
    print("status 0 and not the oracle's answer (family, queries, k):", sorted(set(silent)))
    print("status 0 and a wrong candidate count (family, queries, k, got, want):", sorted(set(miscounted)))
    assert not silent and not miscounted


# ----------------------------------------------------------------------------------------------------------- IVF
IVF_N, IVF_NLIST = 70001, 12
IVF_P = [0.45, 0.3, 0.15, 0.05, 0.03, 0.0199, 0.0001, 0, 0, 0, 0, 0]          # a 31 k-row cell ... 7 rows, empty cells


def _ivf_coarse(M):
    """Coarse centroids whose inner products with the one-hot queries are small whole numbers (exact in any summation order,
    no ties): coordinate j of sub-space 0 holds a permutation of 1 .. nlist, everything else is 0."""
    dsub = 768 // M
    coarse = np.zeros((IVF_NLIST, 768), F32)
    rng = np.random.default_rng(900 + M)
    for j in range(dsub):
        coarse[:, j] = rng.permutation(IVF_NLIST) + 1
    return coarse


def _ivf_index(M, C, codes, cells, coarse):
    from repconc_amd.ivf import IVFPQIndex
    ivf = IVFPQIndex(768, M, IVF_NLIST, device=DEV)
    ivf.set_centroids(_t(C))
    ivf.coarse = _t(coarse)
    ivf.set_lists(_t(codes), _t(cells))
    return ivf


def _ivf_compare(ivf, q, qsel, want, k, nprobe, names, wrong):
    qd = _t(q[qsel])
    for method in ("lists8", "lists16", "scan"):
        s, i = ivf.search(qd, k, nprobe, method=method)
        s, i = s.cpu().numpy(), i.cpu().numpy()
        for p, j in enumerate(qsel):
            if not (np.array_equal(i[p], want[1][j]) and np.array_equal(s[p].view(np.uint32), want[0][j].view(np.uint32))):
                wrong.append((names[j], method, nprobe, k))


@gpu
@pytest.mark.parametrize("M", [16, 32, 48, 64, 96])
def test_ivf_search_on_every_family(M):
    """IVFPQIndex.search, both widths of the list-centric screen and the per-query scan, on a handful of cells of very unequal
    size (several rounds per task, a cell smaller than a chunk, empty cells), few probes and all cells, 33 queries with the
    families repeated."""
    rng = np.random.default_rng(4100 + M)
    codes = _codes(M, IVF_N, True)
    cells = rng.choice(IVF_NLIST, IVF_N, p=IVF_P)
    coarse = _ivf_coarse(M)
    wrong = []
    for names in _batches(M):
        C, q, _ = _onehot(M, names)
        ivf = _ivf_index(M, C, codes, cells, coarse)
        for nprobe, k in ((2, 10), (IVF_NLIST, 300)):
            want = pq_oracle.ivf_search(q, C, codes, cells, coarse, k, nprobe)
            _ivf_compare(ivf, q, _cyclic(len(names), 33), want, k, nprobe, names, wrong)
    print("wrong answers (family, method, nprobe, k):", sorted(set(wrong)))
    assert not wrong


# --------------------------------------------------------------------- a common vector, through the real table kernel
def _plausible(M, ratio, nq=17):
    """C = c0 + e: e standard normal, c0 a common vector whose norm is `ratio` times that of a row of e; dense Gaussian
    queries and queries parallel to c0 (both directions, Gaussian-sized and ten times that)."""
    rng = np.random.default_rng(7000 + M + int(ratio))
    dsub = 768 // M
    e = rng.standard_normal((M, 256, dsub)).astype(F32)
    c0 = rng.standard_normal(768)
    c0 = (c0 / np.linalg.norm(c0) * ratio * np.sqrt(768.0)).astype(F32)
    C = (e + c0.reshape(M, 1, dsub)).astype(F32)
    q = rng.standard_normal((nq, 768)).astype(F32)
    unit = c0 / np.linalg.norm(c0) * np.sqrt(768.0)
    for p, f in enumerate((1.0, -1.0, 10.0, -10.0, 0.5, 3.0, -3.0, 1.0)):
        q[nq - 1 - p] = (unit * f + (0 if p < 4 else 1) * q[nq - 1 - p] * 0.1).astype(F32)
    return C, q


@gpu
@pytest.mark.parametrize("ratio", [10.0, 100.0, 1000.0])
@pytest.mark.parametrize("M,screen", [(96, "q16"), (48, "q16"), (24, "mfma"), (12, "valu")])
def test_flat_search_with_a_common_centroid_vector(M, screen, ratio):
    from repconc_amd import ops
    N = N_RAGGED
    C, q = _plausible(M, ratio)
    codes = _codes(M, N, True)
    dcodes, dC, dq = _t(codes), _t(C), _t(q)
    ws, wi = c_oracle.adc_search(codes, C, q, 1000)
    for k in (1000, 10):
        s, i = ops.adc_search(dcodes, dC, dq, k)
        assert np.array_equal(i.cpu().numpy(), wi[:, :k]), (M, ratio, k)
        assert np.array_equal(s.cpu().numpy().view(np.uint32), ws[:, :k].view(np.uint32)), (M, ratio, k)


@gpu
@pytest.mark.parametrize("ratio", [10.0, 100.0, 1000.0])
@pytest.mark.parametrize("M", [32, 96])
def test_ivf_search_with_a_common_centroid_vector(M, ratio):
    C, q = _plausible(M, ratio)
    rng = np.random.default_rng(4300 + M)
    codes = _codes(M, IVF_N, True)
    cells = rng.choice(IVF_NLIST, IVF_N, p=IVF_P)
    coarse = rng.standard_normal((IVF_NLIST, 768)).astype(F32)
    ivf = _ivf_index(M, C, codes, cells, coarse)
    wrong = []
    for nprobe, k in ((2, 10), (IVF_NLIST, 300)):
        want = pq_oracle.ivf_search(q, C, codes, cells, coarse, k, nprobe)
        _ivf_compare(ivf, q, list(range(q.shape[0])), want, k, nprobe, ["q%d" % j for j in range(q.shape[0])], wrong)
    assert not wrong, wrong
