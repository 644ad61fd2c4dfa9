"""The shared top-k stage (csrc/topk.h, csrc/topk.hip) on score columns built to break it.

The handle is the dense search.  Its score is the fp32 fmaf chain over d ascending from +0.0f, so for a one-hot query
q = c e_d (c a power of two) over a finite corpus every other term is fmaf(0, x, s) = s and s(q, n) = fl(c x[n][d]) exactly,
with -0.0 turned into +0.0.  A corpus whose columns are hand-made score distributions therefore runs the sample, threshold,
filter, select and exact-select kernels on exactly those fp32 values, and the expected answer is two lines of numpy
(`ref_scores`, `ref_order`): no emulation of the kernels.  The CPU tests check that identity against the fmaf-chain oracle
of test_dense_flat.py and assert, on the INPUTS only, that every column still reaches the branch it was built for.

One exception to "every other term leaves s alone": a product that UNDERFLOWS to zero from below is -0.0, and
fmaf(0, x, -0.0) keeps -0.0 when 0 * x is -0.0 too.  Every corpus here therefore ends in a strictly positive column that is
only queried with |c| = 1 (0 * positive = +0.0, and -0.0 + +0.0 = +0.0), and the identity test would notice a lapse."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

from conftest import ROOT
from test_dense_flat import assert_matches, chain_scores

_TOPK_H = open(os.path.join(ROOT, "repconc_amd", "csrc", "topk.h")).read()


def _define(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, _TOPK_H).group(1))


ADC_SAMPLE_MAX = _define("ADC_SAMPLE_MAX")
ADC_KTH_LIST = _define("ADC_KTH_LIST")
ADC_CAND_CAP = _define("ADC_CAND_CAP")
DENSE_EXACT_MAX_N = 4 * ADC_SAMPLE_MAX            # dense_search.hip: up to here every call takes the exact route
K0 = 100                                          # the k the k-dependent columns (two_*, tie_*) are built around
KMAX = 8192
BIG_N = (262144, 300007)                          # sampled route: stride exactly 8, and a stride that is no integer
SLACK = 3.0                                       # ops.DENSE_SEL_SLACK; PendingSearch: bit0 -> 11, 35; bit1 -> 1, 1/3
SLACK_FEW, SLACK_MANY = (11.0, 35.0), (1.0, 1.0 / 3.0)


# ------------------------------------------------------------------------------------------------------- the reference
def ref_scores(col, c):
    with np.errstate(over="ignore", under="ignore"):
        return (np.float32(c) * col) + np.float32(0)          # one fp32 rounding; -0 -> +0


def ref_order_plain(s):
    return np.argsort(-s, kind="stable")[:KMAX]               # score descending, row ascending


def ref_order(s):
    """ref_order_plain without sorting the whole row (a CPU test compares the two on every column): the rows that reach the
    KMAX-th best score, ties included, in row order, then the same stable sort."""
    ns = -s
    if ns.size <= KMAX:
        return ref_order_plain(s)
    idx = np.nonzero(ns <= np.partition(ns, KMAX - 1)[KMAX - 1])[0]
    return idx[np.argsort(ns[idx], kind="stable")][:KMAX]


def sample_rows(N):
    """Corpus rows of the strided sample (dense_search.hip, fast route step 1): j -> j N / S."""
    S = min(N, ADC_SAMPLE_MAX)
    return (np.arange(S, dtype=np.int64) * N) // S


def sample_rank(N, k, slack):
    """The rank formula quoted in include/repconc_hip.h: r = floor(mu + slack sqrt(mu + 1) + 4) + 1, mu = k S / N."""
    S = min(N, ADC_SAMPLE_MAX)
    mu = k * S / N
    return min(int(mu + slack * np.sqrt(mu + 1.0) + 4.0) + 1, S)


# --------------------------------------------------------------------------------------------------- column generators
# each: (N, rng) -> fp32 [N], all values finite; they work for any N >= 1 (sizes are clipped)
def g_gauss(N, rng):
    return rng.standard_normal(N).astype(np.float32)


def g_const(N, rng):
    return np.full(N, 0.75, np.float32)


def g_two(h):
    def gen(N, rng):
        x = np.zeros(N, np.float32)
        x[rng.choice(N, min(h, N), replace=False)] = 1.0
        return x
    return gen


def g_two_retry(N, rng):
    """1.0 on 200 rows, exactly 24 of them at sampled positions: at k = 100 the default threshold (sample rank 28) is 0.0 and
    every list overflows, the first bit-1 retry (slack 1: rank 21) lands on 1.0 and keeps the 200."""
    x = np.zeros(N, np.float32)
    sr = sample_rows(N)
    rest = np.setdiff1d(np.arange(N), sr)
    x[rng.choice(sr, min(24, sr.size), replace=False)] = 1.0
    if rest.size:
        x[rng.choice(rest, min(176, rest.size), replace=False)] = 1.0
    return x


def g_two_edge(N, rng):
    """1.0 on exactly r sampled rows, r the default sample rank at k = 100, and on 100 rows outside the sample: the r-th largest
    sample score is the LAST key of its bin in every histogram pass (the suffix sum equals the rank exactly): an off-by-one
    in adc_pick_bin moves the threshold down to 0.0 and the list overflows."""
    x = np.zeros(N, np.float32)
    sr = sample_rows(N)
    rest = np.setdiff1d(np.arange(N), sr)
    x[rng.choice(sr, min(sample_rank(N, K0, SLACK), sr.size), replace=False)] = 1.0
    if rest.size:
        x[rng.choice(rest, min(K0, rest.size), replace=False)] = 1.0
    return x


TIE_V, TIE_ABOVE = np.float32(2.5), K0 // 2


def g_tie(G):
    def gen(N, rng):
        perm = rng.permutation(N)
        a = min(TIE_ABOVE, N)
        g = min(G, N - a)
        x = (TIE_V - 1 - np.abs(rng.standard_normal(N))).astype(np.float32)
        x[perm[:a]] = (TIE_V + 1 + rng.permutation(a) / 64.0).astype(np.float32)      # distinct, above
        x[perm[a:a + g]] = TIE_V
        return x
    return gen


def g_cluster(N, rng):
    x = (1 + rng.integers(0, 2 ** 13 + 1, N) * 2.0 ** -23).astype(np.float32)         # [1, 1 + 2^-10]
    sr = sample_rows(N)                                          # ~20 outliers of both signs, 10 of them in the sample
    out = np.unique(np.concatenate([rng.choice(sr, min(10, sr.size), replace=False), rng.choice(N, min(10, N), replace=False)]))
    x[out] = (np.where(np.arange(out.size) % 2 == 0, 1, -1) * 1e30 * (1 + np.arange(out.size) / 32.0)).astype(np.float32)
    return x


def g_overflow(N, rng):
    x = rng.standard_normal(N)
    u = rng.random(N)
    big = 3e38 * (0.95 + 0.1 * rng.random(N))
    x = np.where(u < 0.25, big, np.where(u < 0.5, -big, x))
    return x.astype(np.float32)


def g_subn(N, rng):
    return (rng.integers(-2 ** 20, 2 ** 20 + 1, N) * 2.0 ** -149).astype(np.float32)


def g_subn_pos(N, rng):
    return (rng.integers(1, 1025, N) * 2.0 ** -149).astype(np.float32)


def g_lowbits(nj):
    def gen(N, rng):
        return (1 + rng.integers(0, nj, N) * 2.0 ** -23).astype(np.float32)
    return gen


def g_ints(N, rng):
    return rng.integers(-3, 4, N).astype(np.float32)


def g_ramp_up(N, rng):
    return np.arange(N, dtype=np.float32)


def g_ramp_down(N, rng):
    return np.arange(N, dtype=np.float32)[::-1].copy()


def g_blind(N, rng):
    x = rng.standard_normal(N).astype(np.float32)
    x[(sample_rows(N) + 1) % N] += np.float32(100)            # N = 262144: the rows n % 8 == 1
    return x


FLAT_H = 500


def g_flattered(N, rng):
    x = rng.standard_normal(N).astype(np.float32)
    sr = sample_rows(N)
    x[rng.choice(sr, min(FLAT_H, sr.size), replace=False)] += np.float32(100)
    return x


# the two strictly positive columns come last: they close the corpora (module docstring).  lowbits6: 1 + j 2^-23, j < 56 (six
# low bits, and more than 4096 rows per value at both N: one tie group that does not fit the select's LDS)
GENERATORS = [
    ("gauss", g_gauss), ("overflow", g_overflow), ("const", g_const),
    ("two_99", g_two(K0 - 1)), ("two_100", g_two(K0)), ("two_101", g_two(K0 + 1)), ("two_5000", g_two(5000)),
    ("two_20000", g_two(20000)), ("two_retry", g_two_retry), ("two_edge", g_two_edge),
    ("tie_3000", g_tie(3000)), ("tie_6000", g_tie(6000)), ("tie_20000", g_tie(20000)),
    ("cluster", g_cluster), ("subn", g_subn), ("subn_pos", g_subn_pos), ("ints", g_ints),
    ("ramp_up", g_ramp_up), ("ramp_down", g_ramp_down), ("blind", g_blind), ("flattered", g_flattered),
    ("lowbits6", g_lowbits(56)), ("lowbits10", g_lowbits(1024)),
]
TAILS = ("lowbits6", "lowbits10")
# scaled queries: scores quantised into sub-normals with huge tie groups (2^-140 on a Gaussian column: |s| is a multiple of
# 2^-149 below ~2^-138; 2^-100 only moves the exponent, its scores stay normal), and +-inf scores from finite inputs
SCALED = (("gauss", 2.0 ** -140), ("gauss", -2.0 ** -140), ("gauss", 2.0 ** -100),
          ("overflow", 2.0 ** 100), ("overflow", -2.0 ** 100))

_COLS, _REF = {}, {}


def columns(N):
    if N not in _COLS:
        _COLS[N] = {name: gen(N, np.random.default_rng([N, zlib.crc32(name.encode())])) for name, gen in GENERATORS}
        for name, col in _COLS[N].items():
            assert col.dtype == np.float32 and col.shape == (N,) and np.isfinite(col).all(), name
    return _COLS[N]


def reference(N, name, c):
    """(scores fp32 [N], the first KMAX rows of the (score desc, row asc) order) of query c e_name."""
    key = (N, name, float(c))
    if key not in _REF:
        s = ref_scores(columns(N)[name], c)
        _REF[key] = (s, ref_order(s))
    return _REF[key]


def corpora(N, D):
    """The columns packed into corpora of width D: D - 1 of them and a strictly positive tail; a short last corpus repeats
    earlier columns.  -> [(names [D], X fp32 [N, D])]"""
    cols = columns(N)
    body = [n for n, _ in GENERATORS if n not in TAILS]
    if D == 1:
        return [([n], cols[n][:, None].copy()) for n in ("ints",)]
    out = []
    for ci, c0 in enumerate(range(0, len(body), D - 1)):
        names = body[c0:c0 + D - 1]
        names += body[:D - 1 - len(names)]
        names.append(TAILS[ci % len(TAILS)])
        out.append((names, np.stack([cols[n] for n in names], axis=1)))
    return out


MANY_SCALES = [sg * 2.0 ** j for j in (0, 1, -1, 2, -2, 3) for sg in (1, -1)]


def many_queries(names):
    """+-2^j e_d for every column; the closing column keeps |c| = 1."""
    return [(d, c) for d, c in queries(names, scales=MANY_SCALES) if d != len(names) - 1 or abs(c) == 1.0]


def queries(names, scales=(1.0, -1.0), scaled=True):
    """[(column, c)] of one call: +-e_d for every column of the corpus, then the scaled ones whose column is present."""
    ql = [(d, c) for d in range(len(names)) for c in scales]
    if scaled:
        ql += [(names.index(n), c) for n, c in SCALED if n in names[:-1]]
    return ql


def query_matrix(ql, D):
    q = np.zeros((len(ql), D), np.float32)
    for i, (d, c) in enumerate(ql):
        q[i, d] = c
    return q


def expected(N, names, ql, k):
    ws = np.full((len(ql), k), -np.inf, np.float32)
    wi = np.full((len(ql), k), -1, np.int64)
    kk = min(k, N)
    for i, (d, c) in enumerate(ql):
        s, order = reference(N, names[d], c)
        wi[i, :kk] = order[:kk]
        ws[i, :kk] = s[order[:kk]]
    return ws, wi


# ------------------------------------------------------------------------------- what the sampled route does to a column
def first_pass(N, s, k, slack):
    """(sample rank, threshold, candidate count, status bits) of one pass of the sampled route over the score row s, from
    the header's rank formula and the data: bit 0 = fewer than min(k, N) candidates, bit 1 = more than ADC_CAND_CAP."""
    r = sample_rank(N, k, slack)
    assert r <= 0.8 * ADC_CAND_CAP * min(N, ADC_SAMPLE_MAX) / N or k > 1000      # (the large-k cap of the rank is not in play)
    thr = np.sort(s[sample_rows(N)])[::-1][r - 1]
    cnt = int((s >= thr).sum())
    return r, thr, cnt, (1 if cnt < min(k, N) else 0) | (2 if cnt > ADC_CAND_CAP else 0)


def value_bin_members(keys_scores, rank):
    """The first cut of adc_kth_largest_v as a property of the input: (fp32 scale 256 / (max - min), members of the one of
    256 equal bins over [min, max] that holds the rank-th largest)."""
    s = np.asarray(keys_scores, np.float32)
    smin, smax = s.min(), s.max()
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        scale = np.float32(256) / (smax - smin)
        if not np.isfinite(scale) or scale == 0:
            return scale, None
        b = np.minimum(255, ((s - smin) * scale).astype(np.int64))
    kth_bin = b[np.argsort(-s, kind="stable")[rank - 1]]
    return scale, int((b == kth_bin).sum())


# the status of ONE call at the default slack, columns queried with +e_d, k = 100 and k = 1000 (raw-entry test).
# ints belongs to the overflows, not to the zeros, although its values are harmless: a seventh of the corpus scores 3.0, the
# threshold can only be 3.0 and that tie group (> 37 000 rows) overflows the list.
STATUS_ZERO = ("gauss", "tie_3000", "tie_6000", "cluster", "overflow", "subn", "subn_pos", "lowbits6", "lowbits10", "ramp_up",
               "ramp_down")
STATUS_MANY = ("const", "tie_20000", "blind", "ints")
STATUS_FEW = ("flattered",)


# ----------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("D", [16, 12])
def test_one_hot_queries_make_the_chain_score_the_column(D):
    """s(c e_d, n) of the fmaf-chain oracle == fl(c x[n][d]) + 0, bit for bit, for every column and every scaled query: the
    licence for the plain reference of the GPU tests."""
    N = 4096
    seen = set()
    for ci, (names, X) in enumerate(corpora(N, D)):
        assert (X[:, -1] > 0).all()                                  # the closing column (module docstring)
        for d, c in (many_queries(names) if ci == 0 else queries(names)):
            assert d != D - 1 or abs(c) == 1.0
            q = np.zeros(D, np.float32)
            q[d] = c
            with np.errstate(all="ignore"):
                got = chain_scores(np.broadcast_to(q, X.shape), X)
            want = reference(N, names[d], c)[0]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (names[d], c)
            assert not np.signbit(want[want == 0]).any()
            seen.add(names[d])
    assert seen == {n for n, _ in GENERATORS}


def test_reference_order_is_score_descending_then_row_ascending():
    s = np.array([1, 3, 3, -np.inf, 0.0, 3, np.inf, 1], np.float32)
    assert ref_order(s).tolist() == [6, 1, 2, 5, 0, 7, 4, 3]
    N = BIG_N[1]
    for name, c in [(n, c) for n, _ in GENERATORS for c in (1.0, -1.0)] + list(SCALED):
        s = ref_scores(columns(N)[name], c)
        assert np.array_equal(ref_order(s), ref_order_plain(s)), (name, c)
    assert ref_scores(np.array([0.0, 2.0], np.float32), -1.0).view(np.uint32).tolist() == [0, 0xC0000000]


@pytest.mark.parametrize("N", BIG_N)
def test_columns_reach_the_branches_they_were_built_for(N):
    """Preconditions of the GPU cases, on the inputs alone."""
    cols = columns(N)
    S = ADC_SAMPLE_MAX
    sr = sample_rows(N)
    assert N > DENSE_EXACT_MAX_N and sr.size == S and np.unique(sr).size == S
    if N == 262144:
        assert (sr % 8 == 0).all()
    sampled = np.zeros(N, bool)
    sampled[sr] = True

    # adc_kth_largest_v in the threshold kernel (list_cap = ADC_KTH_LIST), rank by rank
    for k in (1, K0, 1000):
        r = sample_rank(N, k, SLACK)
        # control: the value-space cut is taken and the selected bin is a short list
        scale, members = value_bin_members(cols["gauss"][sr], r)
        assert np.isfinite(scale) and members <= ADC_KTH_LIST // 8
        # cluster + outliers: the bin of the r-th largest holds nearly the whole sample -> bit-radix select over everything
        for c in (1.0, -1.0):
            scale, members = value_bin_members(ref_scores(cols["cluster"], c)[sr], r)
            assert np.isfinite(scale) and scale > 0 and members > ADC_KTH_LIST
            # small signed integers: seven bins of ~S / 7 > ADC_KTH_LIST members, keys of both signs (top = 31), a rank
            # inside a tie group
            scale, members = value_bin_members(ref_scores(cols["ints"], c)[sr], r)
            assert members > ADC_KTH_LIST
        # keys that differ in six low bits: one value per bin, the list is one tie group (the early return of
        # adc_kth_largest for all-equal keys); in ten low bits: four values per bin, the list's keys differ in the two
        # lowest bits (top = 1: ONE pass, 2 bits wide)
        _, members = value_bin_members(cols["lowbits6"][sr], r)
        assert 0 < members <= ADC_KTH_LIST
        s10 = cols["lowbits10"][sr]
        _, members = value_bin_members(s10, r)
        kth = np.sort(s10)[::-1][r - 1]
        near = np.unique(s10[np.abs(s10 - kth) < 4 * 2.0 ** -23].view(np.uint32))
        assert 0 < members <= ADC_KTH_LIST and near.size >= 2
    with np.errstate(over="ignore"):
        # constant: min == max, the early return of adc_kth_largest_v
        assert np.ptp(cols["const"]) == 0
        # range that overflows: max - min is inf in fp32, scale == 0: no value bins, the bit-radix select over everything
        o = cols["overflow"][sr]
        assert np.isinf(o.max() - o.min()) and np.float32(256) / (o.max() - o.min()) == 0 and S > ADC_KTH_LIST
        # sub-normals only: fl(256 / (max - min)) is inf -> bit-radix select, keys of both signs: top = 31, four 8-bit passes
        for name in ("subn", "subn_pos"):
            v = cols[name][sr]
            assert (np.abs(cols[name]) < 2.0 ** -126).all() and np.isinf(np.float32(256) / (v.max() - v.min()))
        assert (cols["subn"][sr] < 0).any() and (cols["subn"][sr] > 0).any()
        # positive sub-normals m 2^-149, m <= 1024: the keys differ in bits [0, 11): passes of 8 and 3 bits
        kb = cols["subn_pos"][sr].view(np.uint32)
        assert int(kb.max() ^ kb.min()).bit_length() == 11
        # scaled queries: scores quantised into sub-normals (tie groups of hundreds of rows), and +-inf from finite inputs
        sq = reference(N, "gauss", 2.0 ** -140)[0]
        assert (np.abs(sq) < 2.0 ** -126).all() and np.unique(sq).size < N // 50
        si = reference(N, "overflow", 2.0 ** 100)[0]
        assert np.isposinf(si).sum() > ADC_CAND_CAP and np.isneginf(si).sum() > ADC_CAND_CAP and not np.isnan(si).any()

    # the status of the first pass, k = 100 and k = 1000 (raw-entry test), and what the retries do (stats assertions)
    for k in (K0, 1000):
        for name in STATUS_ZERO:
            assert first_pass(N, cols[name], k, SLACK)[3] == 0, (name, k)
        for name in STATUS_MANY:
            assert first_pass(N, cols[name], k, SLACK)[3] == 2, (name, k)
            for slack in SLACK_MANY:                                   # bit 1 retries tighten: still an overflow -> exact route
                assert first_pass(N, cols[name], k, slack)[3] == 2, (name, k, slack)
        assert first_pass(N, cols["flattered"], k, SLACK)[3] == 1
    for k in (1, K0, 1000, KMAX):
        for c in (1.0, -1.0):
            assert first_pass(N, ref_scores(cols["gauss"], c), k, SLACK)[3] == 0, (k, c)      # control: no retry at any k

    # tie group straddling the k-th rank (k = 100): TIE_ABOVE rows above v, G rows at v, about G / 8 of them sampled
    for G in (3000, 6000, 20000):
        x = cols["tie_%d" % G]
        assert (x > TIE_V).sum() == TIE_ABOVE < K0 and (x == TIE_V).sum() == G
        assert G // 16 < (sampled & (x == TIE_V)).sum() < G // 4
        for k in (K0, 1000):
            r, thr, cnt, _ = first_pass(N, x, k, SLACK)
            assert thr == TIE_V and cnt == TIE_ABOVE + G                # the candidates: the rows above and the whole tie group
    # adc_select_kernel at k = 100 / 1000 (cap = 4096): cnt > 2048 and cnt > 2 k -> the cut; survivors (= every candidate, the
    # k-th score is v) <= cap: sorted in LDS; > cap: the bitonic sort in global memory; G = 20 000: the list overflows
    assert 2048 < TIE_ABOVE + 3000 <= 4096 < TIE_ABOVE + 6000 <= ADC_CAND_CAP < TIE_ABOVE + 20000
    # lowbits6 at k = 100: the candidates are ONE tie group of > 4096 rows: all-equal keys in the cut, global-memory sort
    _, thr, cnt, _ = first_pass(N, cols["lowbits6"], K0, SLACK)
    assert thr == cols["lowbits6"].max() and 4096 < cnt <= ADC_CAND_CAP

    # two values: |H| = k - 1, k, k + 1 around k = 100; 5 000 fits the list, 20 000 does not
    for h in (K0 - 1, K0, K0 + 1, 5000, 20000):
        assert (cols["two_%d" % h] == 1).sum() == h and (cols["two_%d" % h] == 0).sum() == N - h
    assert first_pass(N, cols["two_5000"], K0, SLACK)[2] == 5000
    # two_retry at k = 100: overflow at the default slack, 200 candidates at the first bit-1 retry
    x = cols["two_retry"]
    assert (sampled & (x == 1)).sum() == 24 and (x == 1).sum() == 200
    assert first_pass(N, x, K0, SLACK)[3] == 2 and first_pass(N, x, K0, SLACK_MANY[0])[2:] == (200, 0)

    # two_edge at k = 100: exactly r sampled rows score 1.0, the threshold is 1.0, r + 100 candidates, no status bit
    x = cols["two_edge"]
    r, thr, cnt, st = first_pass(N, x, K0, SLACK)
    assert (sampled & (x == 1)).sum() == r and (thr, cnt, st) == (1.0, r + K0, 0)
    assert np.sort(x[sr])[::-1][r] == 0.0                              # the next sample score is in another bin

    # sample-blind: none of the 32 768 good rows is sampled, and they are the whole top-k
    x = cols["blind"]
    good = x > 50
    assert good.sum() == S and not (good & sampled).any()
    assert good[reference(N, "blind", 1.0)[1][:KMAX]].all()
    # sample-flattered: the 500 good rows are all sampled
    x = cols["flattered"]
    good = x > 50
    assert good.sum() == FLAT_H and sampled[good].all()
    passes = [first_pass(N, x, 1000, sl) for sl in (SLACK,) + SLACK_FEW]
    assert all(p[3] == 1 for p in passes)                              # too few at every slack -> the exact route answers
    if N == 262144:                                                    # mu = 125
        assert [p[0] for p in passes] == [163, 253, 522]
        assert [p[2] for p in passes[:2]] == [163, 253]                # thresholds among the 500
        assert not good[x >= passes[2][1]].all() and FLAT_H < passes[2][2] < 1000      # the third among the ordinary rows
    # at k = 100 the second bit-0 retry (slack 35) collects enough: answered by a retry, not by the exact route
    p100 = [first_pass(N, x, K0, sl) for sl in (SLACK,) + SLACK_FEW]
    assert [p[3] for p in p100] == [1, 1, 0]

    # ramps are exact in fp32
    assert N < 2 ** 24 and np.array_equal(cols["ramp_up"].astype(np.int64), np.arange(N))
    assert np.array_equal(cols["ramp_down"], cols["ramp_up"][::-1])


def test_exact_route_sizes_put_the_kth_rank_inside_tie_groups_decided_by_id_bytes():
    """Passes 4-7 of the 8-pass select decide between rows of equal score by id; the id bytes roll over at N > 255, 65 535."""
    for N in EXACT_N:
        assert N <= DENSE_EXACT_MAX_N
        cols = columns(N)
        assert np.ptp(cols["const"]) == 0                               # every rank is inside the one tie group
        vals, counts = np.unique(cols["ints"], return_counts=True)
        assert N < 50 or (vals.size == 7 and counts.min() > N // 14)
    assert [n for n in EXACT_N if n > 255] and [n for n in EXACT_N if n > 65535]


# ----------------------------------------------------------------------------------------------------------------- GPU
EXACT_N = (1, 255, 256, 257, 65535, 65537, 131072)
BIG_OFFSET = 2 ** 40 + 7


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _check(x, names, ql, k, N, method="auto", id_offset=0):
    """One call with every query of ql; -> the PendingSearch's stats."""
    from repconc_amd import ops
    q = _dev(query_matrix(ql, x.shape[1]))
    pending = ops.dense_search(x, q, k, id_offset=id_offset, method=method, defer=True)
    got = pending.result()
    assert got[0].shape == (len(ql), k)
    assert_matches(got, expected(N, names, ql, k), id_offset=id_offset)
    return pending.stats


def _alone(x, names, name, k, N, c=1.0):
    return _check(x, names, [(names.index(name), c)], k, N)


def _sampled_matrix(N, D, k):
    for names, X in corpora(N, D):
        x = _dev(X)
        ql = queries(names)
        _check(x, names, ql, k, N)
        _check(x, names, ql, k, N, method="exact")
        yield x, names


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, K0, 1000, 3000, KMAX])
@pytest.mark.parametrize("D", [16, 12])
@pytest.mark.parametrize("N", BIG_N)
def test_sampled_route_on_every_column(N, D, k):
    """Well-behaved and degenerate queries in ONE call (threshold, filter and select blocks side by side), ids and score bits
    against the reference, by the sampled route with its retries and by the exact route; then, query by query, which route
    answered.  The select's LDS capacity: 4096 keys / 512 threads up to k = 1000, 8192 / 512 at k = 3000, 16384 / 1024 at
    k = 8192.  k = 1 is rank 1 of the cut (lowbits6: > 2048 candidates, all tied); lists of <= 2048 or <= 2 k keys (gauss,
    ramps, sub-normals) take the straight LDS sort."""
    seen = set()
    for x, names in _sampled_matrix(N, D, k):
        for c in (1.0, -1.0):
            if "gauss" in names:
                st = _alone(x, names, "gauss", k, N, c)
                assert st == {"retried_queries": 0, "exact_queries": 0}
        if k not in (K0, 1000):
            continue
        # const: every row tied; tie_20000: the tie group at the k-th score overflows the list at any slack; blind: the
        # sample shows none of the 32 768 good rows, every threshold admits them all -> bit 1, two tighter retries, exact route
        for name in ("const", "tie_20000", "blind", "ints"):
            if name in names and name not in seen:
                seen.add(name)
                assert _alone(x, names, name, k, N) == {"retried_queries": 2, "exact_queries": 1}
        if "flattered" in names and "flattered" not in seen:
            seen.add("flattered")
            st = _alone(x, names, "flattered", k, N)
            # bit 0 at slack 3, 11 and 35 (k = 1000) -> exact route; k = 100: the second wider retry collects enough
            assert st == ({"retried_queries": 2, "exact_queries": 1} if k == 1000 else {"retried_queries": 2, "exact_queries": 0})
        if "two_retry" in names and k == K0 and "two_retry" not in seen:
            seen.add("two_retry")
            assert _alone(x, names, "two_retry", k, N) == {"retried_queries": 1, "exact_queries": 0}
    if k in (K0, 1000):
        assert seen >= {"const", "tie_20000", "blind", "ints", "flattered"}


@pytest.mark.gpu
@pytest.mark.parametrize("k", [K0, 1000, KMAX])
@pytest.mark.parametrize("D", [16, 12])
@pytest.mark.parametrize("N", BIG_N)
def test_sampled_route_with_a_1024_key_select(N, D, k, monkeypatch):
    """RC_ADC_SELECT_CAP=1024 (read on every call): every list longer than 1024 keys takes the cut, every survivor set longer
    than 1024 (all of them at k >= 1000) the bitonic sort in global memory; list_cap of the cut's value bin is 2048.  A list
    of 1024 < cnt <= k keys (k = 8192; flattered's first pass, the two_* columns) asks the cut for rank = n, the smallest key."""
    monkeypatch.setenv("RC_ADC_SELECT_CAP", "1024")
    for _ in _sampled_matrix(N, D, k):
        pass


@pytest.mark.gpu
@pytest.mark.parametrize("k", [K0, 1000])
@pytest.mark.parametrize("N,D", [(262144, 16), (300007, 12)])
def test_raw_entry_status_bits_and_first_pass_results(N, D, k):
    """rc_dense_search_q through ctypes: one pass, no retry.  A query whose status is 0 has its final answer already: the
    only place where the two middle paths of the select (tie_3000: cut, survivors sorted in LDS; tie_6000 and lowbits6:
    survivors sorted in global memory) are known to have produced it themselves."""
    import torch
    from repconc_amd import _lib
    lib, h = _lib.load(), _lib.handle(0)
    p = lambda t: C.c_void_p(t.data_ptr())
    listed = {}
    for names, X in corpora(N, D):
        x = _dev(X)
        ql = queries(names)
        q = _dev(query_matrix(ql, D))
        nq = len(ql)
        wsb = lib.rc_dense_search_ws_bytes(N, D, nq, k)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=x.device)
        scores = torch.empty((nq, k), dtype=torch.float32, device=x.device)
        ids = torch.empty((nq, k), dtype=torch.int64, device=x.device)
        status = torch.zeros((1,), dtype=torch.int32, device=x.device)
        qstatus = torch.zeros((nq,), dtype=torch.int32, device=x.device)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.rc_dense_search_q(h, p(x), x.stride(0), N, D, p(q), nq, k, 0, SLACK, p(scores), p(ids), p(status),
                                     p(qstatus), p(ws), wsb, s) == 0
        torch.cuda.synchronize()
        qs = qstatus.cpu().numpy()
        assert int(status.item()) == int(np.bitwise_or.reduce(qs))
        # the threshold is the r-th largest sample score exactly: the candidate count's two status bits follow from the data
        want_qs = np.array([first_pass(N, reference(N, names[d], c)[0], k, SLACK)[3] for d, c in ql])
        assert np.array_equal(qs, want_qs), [(names[d], c, a, b) for (d, c), a, b in zip(ql, qs, want_qs) if a != b]
        ok = np.nonzero(qs == 0)[0]
        ws_, wi_ = expected(N, names, ql, k)
        assert_matches((scores[ok], ids[ok]), (ws_[ok], wi_[ok]))
        for i, (d, c) in enumerate(ql):
            if c == 1.0:
                listed[names[d]] = int(qs[i])
    assert all(listed[n] == 0 for n in STATUS_ZERO), listed
    assert all(listed[n] == 2 for n in STATUS_MANY), listed
    assert all(listed[n] == 1 for n in STATUS_FEW), listed
    assert k != K0 or listed["two_edge"] == 0, listed


def _exact_corpus(N, D):
    cols = columns(N)
    names = (["const", "two_99", "two_100", "two_101", "two_5000", "ints", "ramp_down", "gauss", "tie_3000", "two_20000",
              "subn", "ints", "const", "two_5000", "cluster"][:D - 1] + ["lowbits6"]) if D > 1 else ["ints"]
    return names, np.stack([cols[n] for n in names], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 12, 1])
@pytest.mark.parametrize("N", EXACT_N)
def test_exact_route_ties_are_decided_by_the_id_bytes(N, D):
    """const, two_* and ints put the k-th rank inside a tie group at every k: the answer depends on passes 4-7 of the radix
    select (the ~id half of the key).  k > N gives (-inf, -1) past N."""
    names, X = _exact_corpus(N, D)
    x = _dev(X)
    ql = queries(names, scaled=False)
    for k in sorted({1, 255, 256, 257, min(N, KMAX)}):
        st = _check(x, names, ql, k, N)
        assert st["exact_queries"] == 0 and st["retried_queries"] == 0
    _check(x, names, ql, 256, N, id_offset=BIG_OFFSET)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 12])
def test_many_queries_in_one_call_and_a_large_id_offset(D):
    """The column set with the scales +-2^j (more than 128 queries): the second query tile of the GEMM, as many threshold and
    select blocks; id_offset = 2^40 + 7 on both routes.  (2^j on `overflow` gives +-inf scores, 2^-j on `subn` rounds
    sub-normals; the closing column keeps |c| = 1.)"""
    N, k = 262144, K0
    names, X = corpora(N, D)[0]
    x = _dev(X)
    ql = many_queries(names)
    assert len(ql) > 128
    _check(x, names, ql, k, N, id_offset=BIG_OFFSET)
    _check(x, names, ql, k, N, method="exact", id_offset=BIG_OFFSET)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [262144, 65537])
@pytest.mark.parametrize("D", [16, 12])
def test_corpus_as_a_strided_view(N, D):
    """ldx != D: x = big[:, :D] of an [N, 32] tensor is searched in place (ops._dense_args accepts it), the other 32 - D
    columns must never be read into a score."""
    import torch
    from repconc_amd import ops
    names, X = corpora(N, D)[0]
    big = np.full((N, 32), 1e6, np.float32)
    big[:, D:] *= np.random.default_rng(5).standard_normal((N, 32 - D)).astype(np.float32)
    big[:, :D] = X
    big = _dev(big)
    x = big[:, :D]
    assert x.stride(0) == 32 and not x.is_contiguous() and ops._dense_args(x, x[:1], 1)[0].data_ptr() == big.data_ptr()
    ql = queries(names)
    for k in (K0, 1000):
        _check(x, names, ql, k, N)
        _check(x, names, ql, k, N, method="exact")
    del big
    torch.cuda.synchronize()
