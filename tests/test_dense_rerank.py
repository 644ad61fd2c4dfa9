"""Exact re-ranking of candidate lists: csrc/dense_rerank.hip (rc_dense_rerank / rc_dense_f16_rerank), ops.dense_rerank and
`rerank` of the flat indexes.

The oracle is the emulated chain of tests/test_dense_flat.py (inner product) and tests/test_dense_l2.py (L2), applied to the
valid (query, candidate row) pairs and followed by a lexicographic sort on (score, id): score descending for the inner
product, distance ascending for L2, the lower id first among equals.  fp16 storage: the chain over x.half().float(),
q.half().float().

Shapes.  The emulated fmaf costs about 0.1 us per pair and dimension, so the grid of the issue (D x kc x k x nq) is covered by
a set of (D, kc, nq) in which every value occurs — each with every k of {1, 10, kc, min(2 kc, 8192)} that the select allows —
instead of the cross product; the oracle of a (D, kc, nq, metric, storage) is computed once and cut to every k.  N = 5000
except at kc = 16384, where 16384 DISTINCT ids need a larger store: N = 20000 there."""
import numpy as np
import pytest

from test_dense_flat import assert_matches, chain_scores, fmaf_emul  # noqa: F401  (fmaf_emul: the oracle's arithmetic)
from test_dense_l2 import chain_l2

IP, L2 = 0, 1
PAD = {IP: -np.inf, L2: np.inf}


# ------------------------------------------------------------------------------------------------------------ oracle
def oracle_sorted(xn, qn, cand, metric, id_offset=0):
    """xn [N, D], qn [nq, D] fp32 numpy (the stored values, widened), cand [nq, kc] int64 -> per query the (scores, ids) of
    its valid candidates, sorted by the search's order."""
    N = xn.shape[0]
    r = cand - id_offset
    valid = (r >= 0) & (r < N)
    out = []
    qi, ci = np.nonzero(valid)
    s = (chain_l2 if metric == L2 else chain_scores)(qn[qi], xn[r[qi, ci]]) if qi.size else np.zeros(0, np.float32)
    ids = cand[qi, ci]
    key = s.astype(np.float64) if metric == L2 else -s.astype(np.float64)
    order = np.lexsort((ids, key, qi))
    qi, s, ids = qi[order], s[order], ids[order]
    starts = np.searchsorted(qi, np.arange(cand.shape[0] + 1))
    for j in range(cand.shape[0]):
        out.append((s[starts[j]:starts[j + 1]], ids[starts[j]:starts[j + 1]]))
    return out


def cut(sorted_lists, k, metric):
    """The [nq, k] arrays of a search for k: the first k of every list, then the metric's padding."""
    nq = len(sorted_lists)
    ws = np.full((nq, k), PAD[metric], dtype=np.float32)
    wi = np.full((nq, k), -1, dtype=np.int64)
    for j, (s, i) in enumerate(sorted_lists):
        n = min(k, len(s))
        ws[j, :n], wi[j, :n] = s[:n], i[:n]
    return ws, wi


def _randn(shape, seed):
    import torch
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device="cuda:0", dtype=torch.float32)


def _store(x, storage):
    """(the tensor ops.dense_rerank takes, its values as fp32 numpy, a function that gives the queries' values)."""
    import torch
    if storage == "float16":
        xs = x.to(torch.float16)
        return xs, xs.float().cpu().numpy(), lambda q: q.to(torch.float16).float().cpu().numpy()
    return x, x.cpu().numpy(), lambda q: q.cpu().numpy()


def _distinct(rng, N, nq, kc):
    return np.stack([rng.permutation(N)[:kc] for _ in range(nq)]).astype(np.int64)


def _check(got, want):
    assert_matches(got, want)           # ids and score bits


# --------------------------------------------------------------------------------------------------------------- CPU
def test_rerank_workspace_helper_needs_no_gpu():
    from repconc_amd import _lib, ops
    lib = _lib.load()
    for nq, kc in ((1, 1), (7, 1000), (1200, 1000), (2048, 16384)):
        w = lib.rc_dense_rerank_ws_bytes(nq, kc)
        assert w > 0 and w % 256 == 0 and w >= nq * 16384 * 8
        assert ops.dense_rerank_ws_bytes(nq, kc) == w
    assert lib.rc_dense_rerank_ws_bytes(8, 16385) == 0
    assert lib.rc_dense_rerank_ws_bytes(8, 0) == 0 and lib.rc_dense_rerank_ws_bytes(0, 8) == 0


def test_rerank_argument_errors_are_value_errors_before_any_device_work():
    import torch
    from repconc_amd import _lib, ops
    x, q = torch.zeros(10, 8), torch.zeros(3, 8)
    c = torch.zeros(3, 5, dtype=torch.int64)
    bad = [
        (dict(x=torch.zeros(10)), "rank of x"),
        (dict(q=torch.zeros(3, 8, 1)), "rank of q"),
        (dict(q=torch.zeros(3, 9)), "D mismatch"),
        (dict(k=0), "k = 0"),
        (dict(k=8193), "k above the select's cap"),
        (dict(c=torch.zeros(3, 0, dtype=torch.int64)), "kc = 0"),
        (dict(c=torch.zeros(3, 16385, dtype=torch.int64)), "kc above the cap"),
        (dict(c=torch.zeros(3, 5, dtype=torch.int32)), "int32 candidates"),
        (dict(c=torch.zeros(3, 5)), "float candidates"),
        (dict(c=torch.zeros(15, dtype=torch.int64)), "rank of cand_ids"),
        (dict(c=torch.zeros(4, 5, dtype=torch.int64)), "cand_ids.shape[0] != nq"),
        (dict(metric=2), "unknown metric"),
        (dict(metric="l2"), "unknown metric"),
        (dict(x=torch.zeros(10, 8, dtype=torch.float64)), "fp64 store"),
        (dict(x=torch.zeros(10, 8, dtype=torch.bfloat16)), "bf16 store"),
        (dict(x=torch.zeros(10, 8, dtype=torch.int8)), "int8 store"),
    ]
    for kw, what in bad:
        a = dict(x=x, q=q, c=c, k=2, metric=IP)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.dense_rerank(a["x"], a["q"], a["c"], a["k"], metric=a["metric"])
            pytest.fail(what)
    for xx in (x, x.half()):                                     # valid arguments on the CPU: rejected, no fallback
        with pytest.raises(_lib.RepconcHipError):
            ops.dense_rerank(xx, q, c, 2)
        with pytest.raises(_lib.RepconcHipError):
            ops.dense_rerank(xx, q, c, 2, metric=L2, id_offset=5)


def test_rerank_entry_checks_shapes_before_pointers():
    """The C entries: an unknown metric and the limits are RC_ESHAPE whatever the pointers are; null pointers RC_EINVAL."""
    from repconc_amd import _lib
    lib = _lib.load()
    for fn in (lib.rc_dense_rerank, lib.rc_dense_f16_rerank):
        args = lambda metric=0, k=10, kc=100, N=1000: (None, None, 8, N, 8, None, 1, None, kc, kc, k, 0, metric, None, None,
                                                       None, 0, None)
        assert fn(*args(metric=2)) == _lib.RC_ESHAPE and fn(*args(metric=-1)) == _lib.RC_ESHAPE
        assert fn(*args(k=8193)) == _lib.RC_ESHAPE and fn(*args(kc=16385)) == _lib.RC_ESHAPE
        assert fn(*args(N=1 << 32)) == _lib.RC_ESHAPE
        assert fn(*args()) == _lib.RC_EINVAL


# --------------------------------------------------------------------------------------------------------------- GPU
METRICS = [IP, L2]
STORAGES = ["float32", "float16"]

# (D, kc, nq): every D of {1, 7, 64, 100, 768, 1030}, kc of {1, 63, 64, 65, 257, 1000, 16384}, nq of {1, 3, 130}
GRID = [
    (1, 63, 3),
    (7, 64, 130),
    (64, 1, 1),
    (64, 16384, 1),         # the cap; N = 20000 (module docstring)
    (100, 65, 130),         # fp32: staged, D cuts the last slice; fp16: 200-byte pitch, the lane-per-row path
    (768, 1000, 3),
    (768, 257, 1),
    (1030, 257, 3),         # a second chunk of staged query values
]


def _ks(kc):
    return sorted({k for k in (1, 10, kc, min(2 * kc, 8192)) if k <= 8192})


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D,kc,nq", GRID)
def test_rerank_ids_and_score_bits_equal_the_oracle(D, kc, nq, metric, storage):
    import torch
    from repconc_amd import ops
    N = 20000 if kc > 5000 else 5000
    x = _randn((N, D), 100 + D)
    q = _randn((nq, D), 200 + D + nq)
    xs, xn, qvals = _store(x, storage)
    cand = _distinct(np.random.default_rng(D * 131 + kc + nq), N, nq, kc)
    lists = oracle_sorted(xn, qvals(q), cand, metric)
    cd = torch.from_numpy(cand).cuda()
    for k in _ks(kc):
        got = ops.dense_rerank(xs, q, cd, k, metric=metric)
        assert got[0].shape == (nq, k) and got[0].dtype == torch.float32 and got[1].dtype == torch.int64
        _check(got, cut(lists, k, metric))


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_rerank_of_a_permutation_of_all_ids_equals_the_full_search(metric, storage):
    import torch
    from repconc_amd import ops
    full = {(IP, "float32"): ops.dense_search_exact, (L2, "float32"): ops.dense_search_l2_exact,
            (IP, "float16"): ops.dense_search_f16_exact, (L2, "float16"): ops.dense_search_l2_f16_exact}[(metric, storage)]
    for N, D, nq, k, off in ((3000, 96, 5, 100, 0), (16384, 32, 2, 8192, 77), (200, 40, 3, 300, 5)):
        x, q = _randn((N, D), 300 + N), _randn((nq, D), 400 + N)
        xs = x.half() if storage == "float16" else x
        rng = np.random.default_rng(N)
        cand = torch.from_numpy(np.stack([rng.permutation(N) for _ in range(nq)]).astype(np.int64) + off).cuda()
        want = full(xs, q, k, id_offset=off)
        got = ops.dense_rerank(xs, q, cand, k, metric=metric, id_offset=off)
        assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_rerank_skips_holes_and_foreign_ids_and_pads(metric, storage):
    import torch
    from repconc_amd import ops
    N, D, nq, kc, k = 700, 48, 6, 130, 100
    x, q = _randn((N, D), 501), _randn((nq, D), 502)
    xs, xn, qvals = _store(x, storage)
    for off in (0, 13, 10 ** 9):
        rng = np.random.default_rng(off % 1000)
        cand = _distinct(rng, N, nq, kc) + off
        kind = rng.integers(0, 4, (nq, kc))                       # 0: valid, 1: -1, 2: below id_offset, 3: past the store
        cand[kind == 1] = -1
        cand[kind == 2] = off - 1 - rng.integers(0, 50, int((kind == 2).sum()))
        cand[kind == 3] = off + N + rng.integers(0, 50, int((kind == 3).sum()))
        cand[1] = -1                                              # a row of holes only: all padding
        cand[2, 7:] = -1                                          # 7 slots of which some are valid: fewer than k
        cand[3, :] = off + N                                      # the first id past the store, only
        cand[4, 1:] = off - 1                                     # ... and the last one before it (with off = 0: -1)
        lists = oracle_sorted(xn, qvals(q), cand, metric, id_offset=off)
        assert len(lists[1][0]) == 0 and len(lists[3][0]) == 0 and 0 < len(lists[0][0]) < k and len(lists[2][0]) <= 7
        want = cut(lists, k, metric)
        got = ops.dense_rerank(xs, q, torch.from_numpy(cand).cuda(), k, metric=metric, id_offset=off)
        _check(got, want)
        gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert (gi[1] == -1).all() and (gs[1] == PAD[metric]).all()
        assert (gi[0, len(lists[0][0]):] == -1).all() and (gs[0, len(lists[0][0]):] == PAD[metric]).all()
    # an empty store: every candidate is foreign
    got = ops.dense_rerank(xs[:0], q, torch.zeros((nq, 4), dtype=torch.int64, device="cuda:0"), 3, metric=metric)
    assert (got[1] == -1).all() and (got[0] == PAD[metric]).all()
    got = ops.dense_rerank(xs, q[:0], torch.zeros((0, 4), dtype=torch.int64, device="cuda:0"), 3, metric=metric)
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_rerank_treats_a_candidate_list_as_a_multiset(metric, storage):
    import torch
    from repconc_amd import ops
    N, D, nq, kc = 400, 64, 4, 90
    x, q = _randn((N, D), 601), _randn((nq, D), 602)
    xs, xn, qvals = _store(x, storage)
    rng = np.random.default_rng(6)
    cand = _distinct(rng, N, nq, kc)
    cand[:, 50:70] = cand[:, 0:20]                               # 20 ids twice
    cand[:, 70:80] = cand[:, 0:10]                               # 10 of them three times
    cand[3, :] = cand[3, 0]                                      # one id, 90 times
    lists = oracle_sorted(xn, qvals(q), cand, metric)
    for k in (5, kc, 2 * kc):
        got = ops.dense_rerank(xs, q, torch.from_numpy(cand).cuda(), k, metric=metric)
        _check(got, cut(lists, k, metric))
    gs, gi = (t.cpu().numpy() for t in got)
    for j in range(3):
        ids, counts = np.unique(gi[j, :kc], return_counts=True)
        assert sorted(counts.tolist()) == [1] * 40 + [2] * 10 + [3] * 10     # 90 slots: 40 + 2 x 10 + 3 x 10
        for i in ids[counts > 1]:
            at = np.nonzero(gi[j] == i)[0]
            assert (np.diff(at) == 1).all() and len(set(gs[j, at].view(np.uint32).tolist())) == 1     # adjacent, equal bits
    assert (gi[3, :kc] == cand[3, 0]).all() and len(set(gs[3, :kc].view(np.uint32).tolist())) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_rerank_ties_take_the_lower_id_also_across_position_k(metric, storage):
    import torch
    from repconc_amd import ops
    N, D, nq, kc, k = 600, 64, 3, 300, 20
    x, q = _randn((N, D), 701), _randn((nq, D), 702)
    q = q.half().float()                                         # the self-match below must survive the fp16 rounding
    x[100:140] = x[5]                                            # 41 equal rows, ids 5 and 100 .. 139
    x[300:310] = x[6]
    x[7] = q[0]                                                  # query 0's self-match: L2 distance +0.0
    x[400:430] = q[1] if metric == L2 else 64.0 * q[1]           # query 1's best 30 rows (nearest / largest score): a tie
    #                                                              group that straddles position k = 20
    xs, xn, qvals = _store(x, storage)
    rng = np.random.default_rng(7)
    rest = np.setdiff1d(np.arange(N), np.r_[5:8, 100:140, 300:310, 400:430])
    cand = np.stack([rng.permutation(np.r_[5:8, 100:140, 300:310, 400:430, rng.permutation(rest)[:kc - 83]])
                     for _ in range(nq)]).astype(np.int64)
    lists = oracle_sorted(xn, qvals(q), cand, metric)
    assert (lists[1][1][:30] == np.arange(400, 430)).all()       # the group leads query 1's list, ids ascending
    for kk in (k, kc):
        got = ops.dense_rerank(xs, q, torch.from_numpy(cand).cuda(), kk, metric=metric)
        _check(got, cut(lists, kk, metric))
    gs, gi = (t.cpu().numpy() for t in got)
    for j in range(nq):
        at = np.nonzero(np.isin(gi[j], np.r_[5, 100:140]))[0]
        assert len(at) == 41 and (np.diff(at) == 1).all() and (np.diff(gi[j, at]) > 0).all()
        assert len(set(gs[j, at].view(np.uint32).tolist())) == 1
    if metric == L2:
        z = gs[0, 0]
        assert gi[0, 0] == 7 and z == 0.0 and z.view(np.uint32) == 0                  # +0.0f, sign bit clear
        assert (gs[1, :30].view(np.uint32) == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_rerank_store_and_candidate_layouts(metric, storage):
    import torch
    from repconc_amd import ops
    dt = torch.float16 if storage == "float16" else torch.float32
    esz = 2 if storage == "float16" else 4
    N, nq, kc, k = 900, 5, 200, 50
    rng = np.random.default_rng(8)

    def run(xs, q, cand_t, cand_np):
        xn = xs.float().cpu().numpy()
        qn = (q.to(dt).float() if storage == "float16" else q).cpu().numpy()
        got = ops.dense_rerank(xs, q, cand_t, k, metric=metric)
        _check(got, cut(oracle_sorted(xn, qn, cand_np, metric), k, metric))

    # a column slice of a wider matrix: ldx > D; D = 100 of 104: the pitch is a multiple of 16 bytes in both storages, so the
    # staged kernel runs, and D cuts a slice and (fp16: D % 8 != 0) a 16-byte piece
    wide = _randn((N, 104), 801).to(dt)
    xs = wide[:, :100]
    assert xs.stride(0) == 104 and (xs.stride(0) * esz) % 16 == 0 and xs.data_ptr() % 16 == 0
    q = _randn((nq, 100), 802)
    cand = _distinct(rng, N, nq, kc)
    cand[0, :3] = N - 1                                          # the last row: what follows its D values is not the store's
    run(xs, q, torch.from_numpy(cand).cuda(), cand)
    # ... the same at an odd pitch (lane-per-row path) and fp16 with D % 8 != 0 and a dense pitch
    for W, D in ((103, 100), (77, 77)):
        xs = _randn((N, W), 803 + W).to(dt)[:, :D]
        run(xs, _randn((nq, D), 804), torch.from_numpy(cand).cuda(), cand)
    # a base that is 4-byte but not 16-byte aligned
    D = 64
    flat = _randn((N * D + 16,), 805).to(dt)
    xs = flat[4 // esz: 4 // esz + N * D].view(N, D)
    assert xs.data_ptr() % 16 == 4
    q = _randn((nq, D), 806)
    run(xs, q, torch.from_numpy(cand).cuda(), cand)
    # candidates as column slices of a wider matrix: unit stride (passed through ldc) and stride 2 (made contiguous)
    big = torch.from_numpy(rng.integers(0, N, (nq, 2 * kc + 9)).astype(np.int64)).cuda()
    aligned = _randn((N, D), 807).to(dt)
    for view in (big[:, 5:5 + kc], big[:, 1:1 + 2 * kc:2]):
        assert not view.is_contiguous()
        run(aligned, q, view, view.cpu().numpy())
    # one query past the chunk of a library call
    nq2 = ops.DENSE_QCHUNK + 1
    x2, q2 = _randn((N, 16), 808).to(dt), _randn((nq2, 16), 809)
    cand2 = rng.integers(-3, N + 3, (nq2, 8)).astype(np.int64)
    xn = x2.float().cpu().numpy()
    qn = (q2.to(dt).float() if storage == "float16" else q2).cpu().numpy()
    got = ops.dense_rerank(x2, q2, torch.from_numpy(cand2).cuda(), 8, metric=metric)
    _check(got, cut(oracle_sorted(xn, qn, cand2, metric), 8, metric))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_rerank_store_above_4_gib(metric):
    """1 100 000 x 1024 fp32 = 4.5 GB: byte offsets past 2^32, candidates in the last rows."""
    import torch
    from repconc_amd import ops
    N, D, nq, kc, k = 1100000, 1024, 4, 70, 20
    x = _randn((N, D), 901)
    q = _randn((nq, D), 902)
    rng = np.random.default_rng(9)
    cand = np.stack([N - 1 - rng.permutation(5000)[:kc] for _ in range(nq)]).astype(np.int64)
    cand[0, 0], cand[1, 0] = N - 1, N - 2
    cand[2, :5] = rng.integers(0, 1000, 5)                      # and a few of the first rows
    rows = np.unique(cand)
    remap = np.searchsorted(rows, cand)                          # the oracle sees only the rows that are candidates
    xn = x[torch.from_numpy(rows).cuda()].cpu().numpy()
    lists = oracle_sorted(xn, q.cpu().numpy(), remap, metric)
    lists = [(s, rows[i]) for s, i in lists]                     # rows ascending = remapped ids ascending: the order holds
    assert all(len(i) == kc for _, i in lists) and rows[-1] == N - 1 and rows[0] < 1000
    got = ops.dense_rerank(x, q, torch.from_numpy(cand).cuda(), k, metric=metric)
    _check(got, cut(lists, k, metric))
    del x


@pytest.mark.gpu
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("metric", METRICS)
def test_rerank_is_deterministic_and_runs_on_the_current_stream(metric, storage):
    import torch
    from repconc_amd import ops
    N, D, nq, kc, k = 4000, 128, 40, 3000, 500
    x, q = _randn((N, D), 1001), _randn((nq, D), 1002)
    x[1000:1500] = x[0:500]                                      # ties: the list's arrival order must not show
    xs = x.half() if storage == "float16" else x
    cand = torch.from_numpy(_distinct(np.random.default_rng(10), N, nq, kc)).cuda()
    a = ops.dense_rerank(xs, q, cand, k, metric=metric)
    b = ops.dense_rerank(xs, q, cand, k, metric=metric)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = ops.dense_rerank(xs, q, cand, k, metric=metric)
    side.synchronize()
    assert torch.equal(a[1], c[1]) and torch.equal(a[0].view(torch.int32), c[0].view(torch.int32))


@pytest.mark.gpu
def test_flat_index_rerank_on_every_class():
    """The class's own metric and storage decide the entry; numpy in -> numpy out; the index's id_offset; an empty index
    or query set returns the padded shape."""
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatIPIndex, FlatL2Bf16x3Index, FlatL2F16Index, FlatL2Index
    N, D, nq, kc, k = 1500, 64, 6, 120, 30
    x, q = _randn((N, D), 1101), _randn((nq, D), 1102)
    rng = np.random.default_rng(11)
    made = [(FlatIPIndex(D), IP, "float32"), (FlatIPIndex(D, storage="float16"), IP, "float16"),
            (FlatIPIndex(D, screen="bf16x3"), IP, "float32"), (FlatL2Index(D), L2, "float32"),
            (FlatL2F16Index(D), L2, "float16"), (FlatL2Bf16x3Index(D), L2, "float32")]
    for index, metric, storage in made:
        empty = index.rerank(q, torch.zeros((nq, 4), dtype=torch.int64, device="cuda:0"), 3)
        assert (empty[1] == -1).all() and (empty[0] == PAD[metric]).all() and empty[0].shape == (nq, 3)
        index.add(x)
        index.id_offset = 1000
        cand = _distinct(rng, N, nq, kc) + 1000
        cand[:, ::9] = -1
        _, xn, qvals = _store(x, storage)
        want = cut(oracle_sorted(xn, qvals(q), cand, metric, id_offset=1000), k, metric)
        got = index.rerank(q, torch.from_numpy(cand).cuda(), k)
        assert isinstance(got[0], torch.Tensor)
        _check(got, want)
        got = index.rerank(q.cpu().numpy(), cand, k)
        assert isinstance(got[0], np.ndarray) and isinstance(got[1], np.ndarray)
        _check(got, want)
        none = index.rerank(q[:0], torch.zeros((0, 4), dtype=torch.int64, device="cuda:0"), 3)
        assert none[0].shape == (0, 3) and none[1].shape == (0, 3)
        with pytest.raises(ValueError):
            index.rerank(q[:, :8], torch.from_numpy(cand).cuda(), k)
        with pytest.raises(ValueError):
            index.rerank(q, torch.from_numpy(cand[:2]).cuda(), k)
