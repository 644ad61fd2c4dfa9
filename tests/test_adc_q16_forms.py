"""The two block -> (query group, tile) maps of the flat ADC screen (adc_screen_q16_kernel, csrc/adc_screen16.h).

With groups = ceil(nq / 16) the launch (adc_launch_scans, csrc/adc_search.hip) takes the TILE-dealt map (every XCD all groups and
the tiles == x (mod 8)) when groups < 8 or groups <= RC_ADC_Q16_TILESPLIT_GROUPS (default 64 / (M / 16)), and the GROUP-dealt
map (XCD x owns the groups == x (mod 8) and walks every tile; gpx = ceil(groups / 8) group slots per XCD, the slots past `groups`
idle) from there on: 161 queries at M = 96, 257 at 64, 337 at 48, 513 at 32, 1025 at 16.  Every other test of this kernel asks
for at most 33 queries, so this file is where the group-dealt map runs, and where the tile-dealt one meets many groups.

Which map a case takes is ASSERTED, on the host, by rc_adc_q16_by_tiles(M, nq): the function the launch itself calls.  The cases
named "groups" return 0 from it, the cases named "tiles" 1 (test_every_case_takes_the_form_it_is_named_for, no GPU).

What is compared: ids and uint32 score bits against oracle.c_oracle.adc_search for every query, and for every query the first
pass did not flag the number of rows its exact rescoring kept against #{n : score_n >= tau_q} — an integer that a (group, tile)
pair visited twice or never changes even when the query's top-k survives.  tau_q is the oracle's r-th best score over the
search's sample rows (r = rc_adc_sample_rank, restated in test_screen_bound.py), the count is taken among the oracle's best
KBIG = 4096 rows of the whole index and must stay below KBIG.  No tolerance appears in this file.

Inputs: centroids synth.gaussian(SEED + 1), codes synth.uniform_codes(SEED + 2), queries synth.gaussian(SEED + 3), one set per
(M, N); a smaller query set is a prefix of the largest one.  N = 2^18 + 16 (nine tiles, the last holds 16 rows) and 300 001
(ten tiles, the last ragged)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import c_oracle, pq_oracle, synth
from test_adc_l2 import l2_search, l2_tables
from test_screen_bound import CAND_CAP, KBIG, N_ABOVE, N_RAGGED, SAMPLE_MAX, _raw_search, _sample_rank, _sample_rows

F32 = np.float32
DEV = "cuda"
gpu = pytest.mark.gpu
SEED = 7
KNOB = "RC_ADC_Q16_TILESPLIT_GROUPS"
SLACK = 3.0                      # ops.ADC_SEL_SLACK, asserted where ops is imported
TILES, GROUPS = 1, 0             # what rc_adc_q16_by_tiles returns

# (a) the default switch on both sides, no environment: (M, N, k, nq, form)
DEFAULT_CASES = [
    (96, N_ABOVE, 1000, 160, TILES), (96, N_ABOVE, 1000, 161, GROUPS), (96, N_ABOVE, 1000, 176, GROUPS),     # 11 groups, gpx 2, 5 idle slots
    (48, N_RAGGED, 1000, 336, TILES), (48, N_RAGGED, 1000, 337, GROUPS), (48, N_RAGGED, 1000, 352, GROUPS),  # 22 groups, gpx 3, 2 idle
    (16, N_ABOVE, 10, 1024, TILES), (16, N_ABOVE, 10, 1025, GROUPS), (16, N_ABOVE, 10, 1040, GROUPS),        # 65 groups, gpx 9, 7 idle
    (64, N_RAGGED, 100, 257, GROUPS),
    (32, N_ABOVE, 100, 513, GROUPS),
    (48, N_ABOVE, 100, 1200, GROUPS),                                                                          # 75 groups, gpx 10, 5 idle
]
# (b) both maps forced on the same inputs, M = 16: 8 groups with a last group of one query / full, 9 (seven idle slots), 15, 16, 17
FORCED_M, FORCED_N, FORCED_K = 16, N_ABOVE, 10
FORCED_NQ = [113, 128, 129, 240, 256, 257]
FORCED_KNOBS = [("0", GROUPS), ("1000000", TILES)]
BATCH = (48, N_ABOVE, 100, 1200)                 # the 1200-query batch: tile-dealt at 75 groups with the knob at 1000000
# (c), (d): M = 96
C_M, C_N, C_K, C_NQ, C_CUT = 96, N_ABOVE, 1000, 176, 100003
L2_NQ, L2_K = 161, 100
ZERO_Q = 87                                      # group 5, column 7


def _env_cases():
    """Every run of this file as (M, N, k, nq, knob or None, form)."""
    out = [(M, N, k, nq, None, form) for M, N, k, nq, form in DEFAULT_CASES]
    out += [(FORCED_M, FORCED_N, FORCED_K, nq, knob, form) for nq in FORCED_NQ for knob, form in FORCED_KNOBS]
    out.append(BATCH + ("1000000", TILES))
    out += [(C_M, C_N, L2_K, L2_NQ, None, GROUPS), (C_M, C_N, C_K, C_NQ, "0", GROUPS)]       # (c) L2, (d); their default runs: above
    return out


def _set_knob(monkeypatch, knob):
    if knob is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, knob)


def _form(M, nq):
    from repconc_amd import _lib
    return _lib.load().rc_adc_q16_by_tiles(M, nq)


# ------------------------------------------------------------------------------------------------- inputs and oracle
_NQ_MAX = {}
for _M, _N, _k, _nq, _knob, _f in _env_cases():
    _NQ_MAX[(_M, _N)] = max(_NQ_MAX.get((_M, _N), 0), _nq)
_inputs, _oracles, _devs = {}, {}, {}


def _case(M, N):
    """Inputs of one index, once per module: the largest query set of (M, N); a case takes q[:nq]."""
    if (M, N) not in _inputs:
        _inputs[(M, N)] = SimpleNamespace(M=M, N=N, C=synth.gaussian(SEED + 1, (M, 256, 768 // M)),
                                          codes=synth.uniform_codes(SEED + 2, N, M),
                                          q=synth.gaussian(SEED + 3, (_NQ_MAX[(M, N)], 768)))
    return _inputs[(M, N)]


def _oracle(M, N, k):
    """The oracle's best KBIG rows of every query and the expected candidate count of the first pass at this k: two
    c_oracle.adc_search calls (whole index; the search's sample rows), computed once and left unchanged."""
    if (M, N, k) not in _oracles:
        c = _case(M, N)
        ws, wi = c_oracle.adc_search(c.codes, c.C, c.q, KBIG)
        r = _sample_rank(N, min(N, SAMPLE_MAX), k, SLACK)
        tau = c_oracle.adc_search(c.codes[_sample_rows(N)], c.C, c.q, r)[0][:, r - 1]
        count = (ws >= tau[:, None]).sum(1)
        assert (count < KBIG).all(), (M, N, k, int(count.max()))          # else the count is only a lower bound
        for a in (ws, wi, count):
            a.setflags(write=False)
        _oracles[(M, N, k)] = SimpleNamespace(ws=ws, wi=wi, count=count)
    return _oracles[(M, N, k)]


def _dev(M, N):
    if (M, N) not in _devs:
        c = _case(M, N)
        _devs[(M, N)] = tuple(torch.from_numpy(a).to(DEV) for a in (c.codes, c.C, c.q))
    return _devs[(M, N)]


def _l2_oracle(codes, C, q, k):
    """(d [nq, k], ids [nq, k]) of test_adc_l2.l2_search, by the C oracle instead of a numpy pass over nq x N scores: the tables
    S = 0.0f - T are that file's l2_tables; they are handed to c_oracle.adc_search as the centroids of an index of sub-vector
    width nq, C'[m][c][j] = S_j[m][c], with query j = 1.0 at coordinate j of every sub-space — its inner-product table is then
    S_j bit for bit (0 x finite = +-0, and S holds no -0.0f), and the scan and the order (score descending, lower id first) are the
    oracle's own.  d = 0.0f - s.  test_l2_oracle_by_tables_is_test_adc_l2s_oracle holds the two against each other."""
    nq, (M, K, _) = q.shape[0], C.shape
    S = l2_tables(q, C)                                       # [nq, M, 256]
    Ct = np.ascontiguousarray(S.transpose(1, 2, 0))           # [M, 256, nq]
    onehot = np.zeros((nq, M, nq), F32)
    onehot[np.arange(nq), :, np.arange(nq)] = 1.0
    s, i = c_oracle.adc_search(codes, Ct, onehot.reshape(nq, M * nq), k)
    return F32(0) - s, i


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- CPU, no GPU
@pytest.mark.parametrize("M,N,k,nq,knob,form", _env_cases())
def test_every_case_takes_the_form_it_is_named_for(M, N, k, nq, knob, form, monkeypatch):
    _set_knob(monkeypatch, knob)
    assert _form(M, nq) == form
    groups = -(-nq // 16)
    assert groups >= 8 or form == TILES


def test_default_limit_is_64_over_the_phase_count(monkeypatch):
    from repconc_amd import _lib
    monkeypatch.delenv(KNOB, raising=False)
    first_group_dealt = {96: 161, 64: 257, 48: 337, 32: 513, 16: 1025}
    for M, nq in first_group_dealt.items():
        limit = 64 // (M // 16)
        assert nq == 16 * limit + 1 and limit >= 8
        assert [_form(M, n) for n in (1, 16 * limit - 15, 16 * limit, nq, nq + 15, nq + 16, 100000)] == [1, 1, 1, 0, 0, 0, 0], M
    for M in (8, 12, 24, 40):
        assert _form(M, 176) == _lib.RC_ESHAPE                  # no image, no 16-query screen
    assert _form(48, 0) == _lib.RC_EINVAL
    monkeypatch.setenv(KNOB, "")                                # an empty value is no value
    assert _form(96, 160) == 1 and _form(96, 161) == 0


def test_fewer_than_eight_groups_are_tile_dealt_whatever_the_knob(monkeypatch):
    for knob in ("0", "-5", "3"):
        monkeypatch.setenv(KNOB, knob)
        for M in (16, 32, 48, 64, 96):
            assert _form(M, 112) == 1 and _form(M, 1) == 1      # 7 groups, 1 group
            assert _form(M, 113) == 0                           # 8 groups: the knob decides
    monkeypatch.setenv(KNOB, "8")                               # read on every call
    assert _form(96, 128) == 1 and _form(96, 129) == 0


def test_a_smaller_query_set_is_a_prefix_of_the_largest():
    c = _case(C_M, C_N)
    assert c.q.shape[0] == C_NQ
    assert np.array_equal(c.q[:L2_NQ].view(np.uint32), synth.gaussian(SEED + 3, (L2_NQ, 768)).view(np.uint32))


def test_fixture_candidate_counts_lie_between_k_and_the_list_size():
    """The condition the count checks rest on: for every case at least 99 % of the queries have k <= #{score >= tau} <= 16384
    in the oracle, i.e. the first pass neither keeps too few rows nor overflows a list, and answers them unflagged."""
    seen = set()
    for M, N, k, nq, _, _ in _env_cases():
        if (M, N, k, nq) in seen or k == L2_K and nq == L2_NQ:         # the L2 run has its own scores
            continue
        seen.add((M, N, k, nq))
        count = _oracle(M, N, k).count[:nq]
        outside = int(((count < k) | (count > CAND_CAP)).sum())
        print(M, N, k, nq, "counts", int(count.min()), "..", int(count.max()), "outside", outside)
        assert 100 * outside <= nq, (M, N, k, nq, outside)


def test_l2_oracle_by_tables_is_test_adc_l2s_oracle():
    M, N, nq, k = 96, 3001, 21, 40
    c = _case(C_M, C_N)
    codes, q = c.codes[:N].copy(), c.q[:nq].copy()
    codes[7], codes[2000] = codes[3], codes[3]                         # ties: the lower id first
    q[5] = pq_oracle.decode(codes[3:4], c.C)[0]                        # a zero distance: +0.0f
    gd, gi = _l2_oracle(codes, c.C, q, k)
    wd, wi = l2_search(q, c.C, codes, k)
    assert np.array_equal(gi, wi) and np.array_equal(_bits(gd), _bits(wd))
    assert gi[5, :3].tolist() == [3, 7, 2000] and (_bits(gd[5, :3]) == 0).all()


# ------------------------------------------------------------------------------------------------------------ GPU
def _search(M, N, k, nq, form, q=None, skip=()):
    """One ops.adc_search of the case's first nq queries (or of `q`): asserts the form, the oracle's ids and score bits for
    every query, the expected candidate count for every query whose lists did not overflow in the first pass, and that at most
    1 % are flagged (`skip`: queries left to the caller).  Returns the counts, the flags, the answer and the pending search."""
    from repconc_amd import ops
    assert ops.ADC_SEL_SLACK == SLACK
    assert _form(M, nq) == form, "the case does not take the map it is here for"
    want = _oracle(M, N, k)
    dcodes, dC, dq = _dev(M, N)
    st = {}
    pend = ops.adc_search(dcodes, dC, dq[:nq] if q is None else q, k, defer=True, stats=st)
    qstatus = pend._qstatus.cpu().numpy()                       # the first pass's per-query status bits
    flagged = qstatus != 0
    s, i = pend.result()
    s, i = s.cpu().numpy(), i.cpu().numpy()
    keep = np.ones(nq, bool)
    keep[np.array(list(skip), dtype=np.int64)] = False
    wrong = [j for j in np.nonzero(keep)[0]
             if not (np.array_equal(i[j], want.wi[j, :k]) and np.array_equal(_bits(s[j]), _bits(want.ws[j, :k])))]
    cand = st["candidates"].cpu().numpy().astype(np.int64)
    surv = st["survivors"].cpu().numpy().astype(np.int64)
    assert cand.shape == surv.shape == (nq,)
    # every unflagged query, and every query flagged for too few candidates alone (bit 0): while no list overflowed (bit 1) the
    # first pass's count is exact, so a query whose pairs were never visited does not escape by being flagged and repeated
    check = keep & ((qstatus & 2) == 0)
    miscounted = [(int(j), int(j) // 16, int(cand[j]), int(want.count[j])) for j in np.nonzero(check)[0] if cand[j] != want.count[j]]
    print("flagged", np.nonzero(flagged)[0].tolist(), "wrong answers", wrong)
    print("candidate counts (query, group, got, want):", miscounted)
    assert not wrong and not miscounted
    assert (surv[check] >= cand[check]).all()
    assert 100 * int(flagged[keep].sum()) <= nq, "too many flagged queries: the count check would be skipped"
    return SimpleNamespace(cand=cand, surv=surv, flagged=flagged, pend=pend, s=s, i=i)


@gpu
@pytest.mark.parametrize("M,N,k,nq,form", DEFAULT_CASES)
def test_default_switch_on_both_sides(M, N, k, nq, form, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    _search(M, N, k, nq, form)


@gpu
@pytest.mark.parametrize("nq", FORCED_NQ)
def test_both_forms_forced_on_the_same_inputs(nq, monkeypatch):
    runs = []
    for knob, form in FORCED_KNOBS:
        monkeypatch.setenv(KNOB, knob)
        runs.append(_search(FORCED_M, FORCED_N, FORCED_K, nq, form))
    # the integer test and the threshold do not depend on the map
    assert np.array_equal(runs[0].surv, runs[1].surv) and np.array_equal(runs[0].cand, runs[1].cand)


@gpu
def test_tile_dealt_form_at_75_groups(monkeypatch):
    M, N, k, nq = BATCH
    monkeypatch.setenv(KNOB, "1000000")
    tiles = _search(M, N, k, nq, TILES)
    monkeypatch.delenv(KNOB)
    groups = _search(M, N, k, nq, GROUPS)
    assert np.array_equal(tiles.surv, groups.surv) and np.array_equal(tiles.cand, groups.cand)


@gpu
def test_index_with_an_image_extended_in_place_and_the_l2_metric(monkeypatch):
    from repconc_amd.index import METRIC_INNER_PRODUCT, METRIC_L2, PQIndex
    monkeypatch.delenv(KNOB, raising=False)
    c = _case(C_M, C_N)
    dcodes, dC, dq = _dev(C_M, C_N)
    idx = PQIndex(768, C_M)
    idx.set_centroids(dC)
    idx.add_codes(dcodes[:C_CUT])
    idx.add_codes(dcodes[C_CUT:])                               # the cached image is extended in place, off a tile edge
    assert idx.ntotal == C_N and _form(C_M, C_NQ) == GROUPS and _form(C_M, L2_NQ) == GROUPS
    want = _oracle(C_M, C_N, C_K)
    s, i = idx.search(dq[:C_NQ], C_K)
    assert np.array_equal(i.cpu().numpy(), want.wi[:C_NQ, :C_K])
    assert np.array_equal(_bits(s.cpu().numpy()), _bits(want.ws[:C_NQ, :C_K]))
    assert idx.metric_type == METRIC_INNER_PRODUCT
    idx.metric_type = METRIC_L2                                 # the same codes and image under the other metric
    wd, wi = _l2_oracle(c.codes, c.C, c.q[:L2_NQ], L2_K)
    st = {}
    d, i = idx.search_async(dq[:L2_NQ], L2_K, stats=st)()
    assert "survivors" in st and idx.last_search.metric == METRIC_L2
    assert np.array_equal(i.cpu().numpy(), wi)
    assert np.array_equal(_bits(d.cpu().numpy()), _bits(wd))


@gpu
def test_raw_entry_in_the_group_dealt_form(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    assert _form(C_M, C_NQ) == GROUPS
    want = _oracle(C_M, C_N, C_K)
    s, i, status, qstatus, cand = _raw_search(SimpleNamespace(M=C_M, N=C_N), _dev(C_M, C_N), list(range(C_NQ)), C_K, SLACK)
    assert status == int(np.bitwise_or.reduce(qstatus)) and (qstatus & ~3 == 0).all()
    s, i = s.cpu().numpy(), i.cpu().numpy()
    ok = qstatus == 0
    assert 100 * int((~ok).sum()) <= C_NQ
    assert np.array_equal(i[ok], want.wi[:C_NQ, :C_K][ok]) and np.array_equal(_bits(s[ok]), _bits(want.ws[:C_NQ, :C_K][ok]))
    exact = (qstatus & 2) == 0                                  # no list overflowed: the count is exact
    assert np.array_equal(cand[exact].astype(np.int64), want.count[:C_NQ][exact])


@gpu
@pytest.mark.parametrize("knob", ["0", None])
def test_a_zero_query_among_many_groups(knob, monkeypatch):
    """Query 87 (group 5, column 7) is all zeros: every row ties at +0.0, its list overflows, the exact route answers it — and
    its fifteen neighbours in the group, and every other group, are answered as without it."""
    _set_knob(monkeypatch, knob)
    _, _, dq = _dev(C_M, C_N)
    q = dq[:C_NQ].clone()
    q[ZERO_Q] = 0.0
    r = _search(C_M, C_N, C_K, C_NQ, GROUPS, q=q, skip=(ZERO_Q,))
    assert r.flagged[ZERO_Q]
    assert r.pend.stats["exact_queries"] == 1, r.pend.stats
    assert np.array_equal(r.i[ZERO_Q], np.arange(C_K))
    assert (_bits(r.s[ZERO_Q]) == 0).all()                      # +0.0f
