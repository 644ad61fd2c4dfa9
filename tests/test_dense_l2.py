"""Exact dense L2 search (faiss.IndexFlatL2, evaluate_repconc.py:102 / run_warmup.py:102,107): csrc/dense_search_l2.hip,
ops.dense_search_l2, dense_index.FlatL2Index and the Faiss shim.

The oracle is in this file.  A distance is the fp32 chain t = q_j - x_j (one fp32 subtraction), acc = fmaf(t, t, acc) over j
ascending from +0.0f, with the exact fmaf emulation of tests/test_dense_flat.py.  For large N only the rows that can reach the
top-k are chain-scored: an fp64 ranking by the expanded form, and an inclusion radius of the chain's own bound
1.01 (D + 2) u / (1 - (D + 2) u) d plus the fp64 ranking's error, 4 (D + 8) 2^-53 (||q|| + ||x||)^2 (a dot product of any
summation order is off by at most D 2^-53 ||q|| ||x||, it enters twice, the two squared norms by D 2^-53 of themselves, two
additions: (1.5 D + 4) 2^-53 (||q|| + ||x||)^2 in all; it dominates when distances are tiny)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_dense_flat import assert_matches, chain_scores, fmaf_emul

U = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ oracle
def chain_l2(qp, xp):
    """qp, xp: [P, D] fp32 -> the fp32 chain distance of every pair, [P]."""
    qp = np.ascontiguousarray(qp, dtype=np.float32)
    xp = np.ascontiguousarray(xp, dtype=np.float32)
    s = np.zeros(qp.shape[0], dtype=np.float32)
    for d in range(qp.shape[1]):
        t = qp[:, d] - xp[:, d]                       # one fp32 subtraction
        s = fmaf_emul(t, t, s)
    return s


def chain_gamma(D):
    return 1.01 * (D + 2) * U / (1 - (D + 2) * U)


def oracle_topk_l2(x, q, k, qblock=256, rblock=1 << 18):
    """x: device fp32 [N, D], q: device fp32 [nq, D] -> (distances fp32 [nq, k], ids int64 [nq, k]) of the chain, sorted
    (distance asc, row asc), +inf / -1 past N."""
    import torch
    N, D = x.shape
    nq = q.shape[0]
    g = chain_gamma(D)
    e64 = 4.0 * (D + 8) * 2.0 ** -53
    out_s = np.full((nq, k), np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    kk = min(k, N)
    xx = torch.empty((N,), dtype=torch.float64, device=x.device)
    for r0 in range(0, N, rblock):
        xx[r0:r0 + rblock] = x[r0:r0 + rblock].double().square_().sum(1)
    for q0 in range(0, nq, qblock):
        qb = q[q0:q0 + qblock].double()
        qq = (qb * qb).sum(1)
        S = torch.empty((qb.shape[0], N), dtype=torch.float64, device=x.device)
        for r0 in range(0, N, rblock):
            S[:, r0:r0 + rblock] = qb @ x[r0:r0 + rblock].double().T
        S.mul_(-2.0).add_(qq[:, None]).add_(xx[None, :])                       # the expanded form in fp64
        E = (qq.sqrt()[:, None] + xx.sqrt()[None, :]).square_().mul_(e64)      # its own error
        up = (S.clamp_min(0.0) + E) * (1.0 + g)
        lo = (S - E).clamp_min_(0.0) * (1.0 - g)
        del S, E
        kth = torch.topk(up, kk, dim=1, largest=False).values[:, -1:]
        qi, ri = torch.nonzero(lo <= kth, as_tuple=True)
        del up, lo
        s = chain_l2(q[q0:q0 + qblock][qi].cpu().numpy(), x[ri].cpu().numpy())
        qi, ri = qi.cpu().numpy(), ri.cpu().numpy()
        order = np.lexsort((ri, s.astype(np.float64), qi))
        qi, ri, s = qi[order], ri[order], s[order]
        starts = np.searchsorted(qi, np.arange(qb.shape[0]))
        for j in range(qb.shape[0]):
            a = starts[j]
            assert a + kk <= len(qi) and qi[a + kk - 1] == j
            out_s[q0 + j, :kk] = s[a:a + kk]
            out_i[q0 + j, :kk] = ri[a:a + kk]
    return out_s, out_i


# ---- the families of the bound: pairs (q, x), [P, D] each --------------------------------------------------------------
def _families(rng, P, D):
    f32 = np.float32
    n = lambda: rng.standard_normal((P, D))
    q = n().astype(f32)
    fam = {"N(0,1)": (q, n().astype(f32))}
    fam["x = q + 1e-4 noise"] = (q, (q + 1e-4 * n()).astype(f32))
    fam["x = q"] = (q, q.copy())
    fam["magnitudes 2^-30..2^30"] = ((n() * 2.0 ** rng.integers(-30, 31, (P, D))).astype(f32),
                                     (n() * 2.0 ** rng.integers(-30, 31, (P, D))).astype(f32))
    fam["|x| = 1000 |q|"] = (q, (1000.0 * n()).astype(f32))
    fam["fp32 subnormals"] = ((n() * 2.0 ** -130).astype(f32), (n() * 2.0 ** -130).astype(f32))
    fam["x subnormal"] = ((n() * 2.0 ** -100).astype(f32), (n() * 2.0 ** -130).astype(f32))
    fam["one ulp apart"] = (q, np.nextafter(q, np.where(rng.random((P, D)) < 0.5, np.inf, -np.inf).astype(f32)))
    return fam


def _sqnorm32(x):
    """fp32 [P]: the fp64 sum of squares rounded to nearest, what ops.dense_row_sqnorms stores."""
    return (x.astype(np.float64) ** 2).sum(1).astype(np.float32)


def _ratio(sigma, q, x, d_chain, D):
    """|sigma - ||q||^2 + d_chain| / E_q per pair, with each row's own norm as X."""
    from repconc_amd import ops
    q64, x64 = q.astype(np.float64), x.astype(np.float64)
    qq = (q64 * q64).sum(1)
    err = np.abs(sigma.astype(np.float64) - qq + d_chain.astype(np.float64))
    E = ops.dense_l2_error_bound(D, np.sqrt(qq), np.sqrt((x64 * x64).sum(1)))
    assert np.all(E > 0)
    return err / E


# --------------------------------------------------------------------------------------------------------------- CPU
def test_chain_oracle_agrees_with_fp64_within_its_bound_and_is_not_the_rounded_fp64_value():
    rng = np.random.default_rng(3)
    for D in (16, 100, 768):
        q = rng.standard_normal((256, D)).astype(np.float32)
        x = rng.standard_normal((256, D)).astype(np.float32)
        x[:64] = (q[:64] + 1e-3 * rng.standard_normal((64, D))).astype(np.float32)
        ch = chain_l2(q, x)
        d64 = ((q.astype(np.float64) - x.astype(np.float64)) ** 2).sum(1)
        assert np.all(ch >= 0) and np.all(np.abs(ch - d64) <= chain_gamma(D) * d64)
        if D >= 100:
            assert np.any(ch != d64.astype(np.float32))
    z = chain_l2(q[:4], q[:4])
    assert np.all(z == 0) and not np.any(np.signbit(z))                       # a self-match is +0.0f


def test_l2_error_constants_are_the_librarys():
    from repconc_amd import ops
    c = ops.dense_l2_error_constants()
    assert c == (2.0, 4 * 2.0 ** -126, 4 * 2.0 ** -149)
    assert ops.dense_l2_error_bound(100, 3.0, 5.0) == 2 * 112 * U * 64.0 + c[1] * 112 ** 0.5 * 8.0 + c[2] * 112


def test_l2_error_bound_covers_the_screen_against_the_chain():
    """sigma from the emulated fmaf chain of the dot product (what the fp32 matrix cores compute) and the fp64-rounded norm."""
    rng = np.random.default_rng(17)
    P = 256
    worst_all = 0.0
    for D in (16, 100, 768, 4096):
        fam = _families(rng, P, D)
        q = np.concatenate([v[0] for v in fam.values()])
        x = np.concatenate([v[1] for v in fam.values()])
        dot = chain_scores(q, x)
        sigma = fmaf_emul(np.full(dot.shape, 2.0, np.float32), dot, -_sqnorm32(x))
        r = _ratio(sigma, q, x, chain_l2(q, x), D).reshape(len(fam), P).max(1)
        for name, w in zip(fam, r):
            print(f"D={D} {name}: worst |sigma - ||q||^2 + d| / E_q = {w:.4g}")
        assert np.all(r < 1.0)
        worst_all = max(worst_all, float(r.max()))
    print(f"worst ratio {worst_all:.4f}")


def test_l2_workspace_helpers_and_argument_errors_need_no_gpu():
    import torch
    from repconc_amd import _lib, ops
    from repconc_amd.dense_index import FlatL2Index
    lib = _lib.load()
    N, D = 8841823, 768
    assert lib.rc_dense_l2_search_ws_bytes(N, D, 1200, 1000) >= 1200 * (32768 * 4 + 16384 * 8)
    assert lib.rc_dense_l2_search_ws_bytes(1000, D, 1200, 10) == lib.rc_dense_l2_search_exact_ws_bytes(1000, D, 1200, 10)
    assert lib.rc_dense_l2_search_exact_ws_bytes(N, D, 7, 100) == lib.rc_dense_search_exact_ws_bytes(N, D, 7, 100)
    for args in ((N, D, 1200, 8193), (1 << 32, D, 4, 10), (0, D, 4, 10), (N, 0, 4, 10), (N, D, 0, 10), (N, D, 4, 0)):
        assert lib.rc_dense_l2_search_ws_bytes(*args) == 0 and lib.rc_dense_l2_search_exact_ws_bytes(*args) == 0
    RC_ESHAPE, RC_EINVAL = -2, -1
    z = None
    assert lib.rc_dense_l2_search_q(z, z, D, N, D, z, 4, z, z, 8193, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_search_q(z, z, D, 1 << 32, D, z, 4, z, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_search_exact(z, z, D, N, D, z, 4, 8193, 0, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_search_q(z, z, D, N, D, z, 4, z, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_EINVAL
    assert lib.rc_dense_l2_scores(z, z, D, N, D, z, 4, z, z, z) == RC_EINVAL
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_search_l2(torch.zeros(10, 16), torch.zeros(2, 16), 1)
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_search_l2_exact(torch.zeros(10, 16), torch.zeros(2, 16), 1)
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_l2_scores(torch.zeros(10, 16), torch.zeros(2, 16))
    with pytest.raises(TypeError):
        FlatL2Index(16, storage="float16")
    with pytest.raises(TypeError):
        FlatL2Index(16, screen="bf16x3")
    for k in (0, 8193):
        with pytest.raises(ValueError):
            ops.dense_search_l2(torch.zeros(10, 16), torch.zeros(2, 16), k)
    with pytest.raises(ValueError):
        ops.dense_search_l2(torch.zeros(10, 16), torch.zeros(2, 16), 1, method="fast")
    index = FlatL2Index(16, device="cpu")                       # holds nothing: the width is checked before any device work
    assert index.metric_type == 1 and index.ntotal == 0
    with pytest.raises(ValueError):
        index.add(np.zeros((3, 17), np.float32))
    with pytest.raises(ValueError):
        index.search(np.zeros((3, 17), np.float32), 1)


def test_compat_exports_indexflatl2():
    code = r'''
import faiss
import repconc_amd.faiss_compat as fc
from repconc_amd.dense_index import FlatIPIndex, FlatL2Index
assert faiss.IndexFlatL2 is fc.IndexFlatL2 is FlatL2Index
assert faiss.IndexFlatIP is FlatIPIndex and not issubclass(FlatL2Index, FlatIPIndex)
assert faiss.METRIC_L2 == fc.METRIC_L2 == 1 and faiss.METRIC_INNER_PRODUCT == 0
print("ok")
'''
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "compat"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]


# --------------------------------------------------------------------------------------------------------------- GPU
def _randn(shape, seed, dev="cuda:0"):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev, dtype=torch.float32)


FAST_SHAPES = [
    (140001, 768, 257, 10),     # fast route, ragged rows and queries
    (140001, 100, 1, 8192),     # padded D on the screen, the largest k
    (140001, 384, 128, 1000),
    (140001, 101, 64, 100),     # unaligned rows: the element-wise rescoring
]
SHAPES = [
    (1, 768, 1, 10),            # padding: +inf / -1
    (5, 100, 7, 8),             # k > N, padded D
    (1000, 384, 128, 1000),     # k = N
    (65537, 1024, 7, 100),      # exact kernel over many row tiles, ragged last tile
    (65537, 768, 257, 1),       # exact kernel, query tiles with a last one that holds one query
] + FAST_SHAPES
_fast_route_counts = {}         # shape -> (queries, retried + exact) of the auto search, for the pooled test below


@pytest.mark.gpu
@pytest.mark.parametrize("N,D,nq,k", SHAPES)
def test_l2_search_ids_and_distance_bits_equal_the_oracle(N, D, nq, k):
    from repconc_amd import ops
    x = _randn((N, D), 1000 + N + D)
    q = _randn((nq, D), 2000 + nq + D)
    want = oracle_topk_l2(x, q, k)
    assert np.all(want[0] >= 0) and np.all(want[0][:, 1:] >= want[0][:, :-1])
    pending = ops.dense_search_l2(x, q, k, id_offset=7, defer=True)
    got = pending.result()
    assert got[0].shape == (nq, k) and got[1].dtype.is_floating_point is False
    assert_matches(got, want, id_offset=7)
    _fast_route_counts[(N, D, nq, k)] = (nq, pending.stats["retried_queries"] + pending.stats["exact_queries"])
    assert_matches(ops.dense_search_l2(x, q, k, id_offset=7, method="exact"), want, id_offset=7)
    assert_matches(ops.dense_search_l2_exact(x, q, k, id_offset=7), want, id_offset=7)


@pytest.mark.gpu
def test_l2_fast_route_is_really_taken():
    """Pooled over the fast-route shapes: at most 1 % of the queries are repeated or answered by the exact route (a condition:
    the certificate's bound leaves room — a CPU simulation of sample, rank, threshold and certificate flagged 0 of 1 395)."""
    from repconc_amd import ops
    for shape in FAST_SHAPES:
        if shape not in _fast_route_counts:                 # run alone: the search again, without the oracle
            N, D, nq, k = shape
            pending = ops.dense_search_l2(_randn((N, D), 1000 + N + D), _randn((nq, D), 2000 + nq + D), k, defer=True)
            pending.result()
            _fast_route_counts[shape] = (nq, pending.stats["retried_queries"] + pending.stats["exact_queries"])
    total = sum(_fast_route_counts[s][0] for s in FAST_SHAPES)
    flagged = sum(_fast_route_counts[s][1] for s in FAST_SHAPES)
    print(f"fast route: {flagged} of {total} queries repeated or answered by the exact route")
    assert flagged <= 0.01 * total


@pytest.mark.gpu
def test_l2_search_row_pitch_wider_than_d():
    """100-wide rows at a pitch of 104: 16-byte aligned rows with a tail after the last whole vector."""
    from repconc_amd import ops
    N, D, nq, k = 140001, 100, 33, 10
    buf = _randn((N, 104), 71)
    x = buf[:, :D]
    q = _randn((nq, D), 72)
    want = oracle_topk_l2(x.contiguous(), q, k)
    assert x.stride(0) == 104
    assert_matches(ops.dense_search_l2(x, q, k), want)
    assert_matches(ops.dense_search_l2(x, q, k, method="exact"), want)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 100, 768, 1024])
def test_l2_screen_error_stays_inside_the_certificate_bound(D):
    """The raw sigma of the matrix cores against chain - ||q||^2: 16 x 16 pairs per family."""
    import torch
    from repconc_amd import ops
    rng = np.random.default_rng(100 + D)
    worst = 0.0
    for name, (q, x) in _families(rng, 16, D).items():
        xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
        xsq = ops.dense_row_sqnorms(xd)
        assert np.array_equal(xsq.cpu().numpy().view(np.uint32), _sqnorm32(x).view(np.uint32))
        sigma = ops.dense_l2_scores(xd, qd, xsq).cpu().numpy()              # [16 queries][16 rows]
        qp, xp = np.repeat(q, 16, axis=0), np.tile(x, (16, 1))
        r = _ratio(sigma.reshape(-1), qp, xp, chain_l2(qp, xp), D)
        print(f"D={D} {name}: max |sigma - ||q||^2 + d| / E_q = {r.max():.5f}, max |sigma| = {np.abs(sigma).max():.3e}")
        assert r.max() <= 1.0
        worst = max(worst, float(r.max()))
    print(f"D={D}: largest screen-error ratio {worst:.5f}")


_CHUNK_SEEDS = {"l2": 7000, "bf16x3": 7100, "f16": 7200}      # of the corpus; the queries' is one more


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1040, 1029])
@pytest.mark.parametrize("search", ["l2", "bf16x3", "f16"])
def test_rescoring_walks_a_second_query_chunk_in_every_screened_search(search, D):
    """One rescoring kernel body serves the three screened searches and stages the query in chunks of 1024 values.  D = 1040:
    an aligned second chunk of two 8-wide steps on the 16-byte loads; D = 1029: unaligned rows, element-wise loads and a tail
    that crosses the chunk boundary.  A query handed to the exact route never met the rescorer: none may be."""
    from repconc_amd import ops
    from test_dense_flat import oracle_topk
    N, nq, k = 140001, 5, 10
    x = _randn((N, D), _CHUNK_SEEDS[search] + D)
    q = _randn((nq, D), _CHUNK_SEEDS[search] + D + 1)
    if search == "l2":
        want = oracle_topk_l2(x, q, k)
        pending = ops.dense_search_l2(x, q, k, defer=True)
    elif search == "bf16x3":
        want = oracle_topk(x, q, k)
        pending = ops.dense_search_bf16x3(x, q, k, defer=True)
    else:
        x16 = x.half()
        want = oracle_topk(x16.float(), q.half().float(), k)     # the rounded values: what the fp16 search scores
        pending = ops.dense_search_f16(x16, q, k, defer=True)
    assert_matches(pending.result(), want)
    print(f"{search} D={D}: {pending.stats}")
    assert pending.stats["exact_queries"] == 0, pending.stats


@pytest.mark.gpu
def test_l2_self_matches_are_plus_zero_and_ties_take_the_lower_id():
    import torch
    from repconc_amd import ops
    N, D, nq, k = 150000, 64, 32, 10
    x = _randn((N, D), 31)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(32)
    perm = torch.randperm(N, generator=g, device="cuda:0")
    src, dst = perm[: N // 20], perm[N // 20: 2 * (N // 20)]   # 5 % of the rows are copies of other rows, each copied once
    x[dst] = x[src].clone()
    q = x[dst[:nq]].clone()                                   # every query equals a row that has a duplicate
    want = oracle_topk_l2(x, q, k)
    got = ops.dense_search_l2(x, q, k)
    assert_matches(got, want)
    d, i = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.all(d[:, :2].view(np.uint32) == 0)             # the two zero distances are +0.0f
    assert np.all(i[:, 0] < i[:, 1]) and np.all(d[:, 2] > 0)
    assert_matches(ops.dense_search_l2(x, q, k, method="exact"), want)


@pytest.mark.gpu
def test_l2_tie_group_across_the_kth_distance_falls_back_to_the_exact_route():
    """20 000 identical rows whose distance sits inside every query's top-100: the group overflows the candidate list
    whatever the slack, the exact route answers."""
    from repconc_amd import ops
    N, D, nq, k = 150000, 64, 4, 100
    x = _randn((N, D), 35)
    q = 0.05 * _randn((nq, D), 36)
    v = _randn((D,), 37)
    x[90000:110000] = (v * (32.0 ** 0.5 / v.norm()))[None]   # |v|^2 = 32: a few dozen of the gaussian rows (|x|^2 ~ chi2_64) are nearer
    want = oracle_topk_l2(x, q, k)
    tied = (want[1] >= 90000) & (want[1] < 110000)
    assert tied.any(1).all() and (~tied).any(1).all()        # the tie group straddles the k-th distance of every query
    pending = ops.dense_search_l2(x, q, k, defer=True)
    assert_matches(pending.result(), want)
    assert pending.stats["exact_queries"] > 0
    assert_matches(ops.dense_search_l2(x, q, k, method="exact"), want)


@pytest.mark.gpu
def test_l2_certificate_refuses_distances_closer_than_the_screen_error():
    """Every row and query is one vector of norm ~30 plus 1e-4 noise: all distance differences are far below E_q, no answer
    of the fast route can be certified, every query ends on the exact route with the oracle's result."""
    from repconc_amd import ops
    N, D, nq, k = 200000, 64, 8, 10
    base = _randn((D,), 81)
    base *= 30.0 / base.norm()
    x = base[None] + 1e-4 * _randn((N, D), 82)
    q = base[None] + 1e-4 * _randn((nq, D), 83)
    want = oracle_topk_l2(x, q, k)
    eq = ops.dense_l2_error_bound(D, 30.0, 30.0)
    assert float(want[0].max()) < 1e-2 * eq
    pending = ops.dense_search_l2(x, q, k, defer=True)
    assert bool(((pending._qstatus & 4) != 0).all())          # bit 2 on every query of the first pass
    assert_matches(pending.result(), want)
    assert pending.stats["exact_queries"] == nq


@pytest.mark.gpu
def test_l2_negative_slack_forces_retries_with_unchanged_results():
    from repconc_amd import ops
    N, D, nq, k = 140001, 128, 64, 100
    x, q = _randn((N, D), 41), _randn((nq, D), 42)
    want = oracle_topk_l2(x, q, k)
    pending = ops.dense_search_l2(x, q, k, sel_slack=-50.0, defer=True)
    got = pending.result()
    assert pending.stats["retried_queries"] > 0
    assert_matches(got, want)
    assert_matches(ops.dense_search_l2(x, q, k), want)


@pytest.mark.gpu
def test_l2_search_corpus_above_4_gib():
    """1 500 000 x 768 fp32 = 4.6 GB: byte offsets past 2^32 in the screen, the rescoring and the exact kernel; the nearest
    rows of queries 0 and 1 are the last two."""
    from repconc_amd import ops
    N, D, nq, k = 1500000, 768, 16, 10
    x = _randn((N, D), 51)
    q = _randn((nq, D), 52)
    x[N - 1] = q[0] + 1e-3
    x[N - 2] = q[1] + 1e-3
    want = oracle_topk_l2(x, q, k, qblock=16, rblock=1 << 19)
    assert want[1][0, 0] == N - 1 and want[1][1, 0] == N - 2
    pending = ops.dense_search_l2(x, q, k, defer=True)
    assert_matches(pending.result(), want)
    assert pending.stats["exact_queries"] == 0
    assert_matches(ops.dense_search_l2(x, q[:2], k, method="exact"), (want[0][:2], want[1][:2]))
    del x


@pytest.mark.gpu
def test_flat_l2_index_add_grow_reset_search_and_batching():
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatL2Index
    from repconc_amd.faiss_compat import METRIC_L2, IndexFlatL2
    N, D, nq, k = 3000, 100, 50, 20
    xb = _randn((N, D), 61).cpu().numpy()
    qb = _randn((nq, D), 62).cpu().numpy()
    one = IndexFlatL2(D)
    assert isinstance(one, FlatL2Index) and one.is_trained and one.metric_type == METRIC_L2 == 1 and one.d == D
    s0, i0 = one.search(qb[:3], 5)                                   # the empty index
    assert np.all(i0 == -1) and np.all(np.isposinf(s0))
    one.add(xb)
    assert one.ntotal == N and one._x.shape[0] == N and one._xsq.shape[0] == N      # the first add allocates exactly
    three = FlatL2Index(D, device="cuda")
    three.add(xb[:1000])
    three.add(torch.from_numpy(xb[1000:1100]).cuda())
    assert three._x.shape[0] == 1500 and three._xsq.shape[0] == 1500                # growth 1.5x, the norms with it
    three.add(xb[1100:])
    assert three.ntotal == N and tuple(three.xb.shape) == (N, D)
    whole = ops.dense_row_sqnorms(torch.from_numpy(xb).cuda())
    for ix in (one, three):
        assert torch.equal(ix._xsq[:N].view(torch.int32), whole.view(torch.int32))
        assert float(ix._xnorm_max) >= float(whole.max().sqrt())
    want = oracle_topk_l2(torch.from_numpy(xb).cuda(), torch.from_numpy(qb).cuda(), k)
    s1, i1 = one.search(qb, k)
    s3, i3 = three.search(qb, k)
    assert isinstance(s1, np.ndarray) and isinstance(i1, np.ndarray) and i1.dtype == np.int64
    assert_matches((s1, i1), want)
    assert_matches((s3, i3), want)
    st, it = one.search(torch.from_numpy(qb).cuda(), k)
    assert isinstance(st, torch.Tensor) and st.is_cuda and it.is_cuda
    assert_matches((st, it), want)
    # several batches enqueued before any is finished
    fins = [one.search_async(part, k) for part in np.array_split(qb, 4)]
    parts = [f() for f in fins]
    assert_matches((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), want)
    assert one.last_search.stats == {"retried_queries": 0, "exact_queries": 0}
    one.id_offset = 1000
    assert_matches(one.search(qb, k), want, id_offset=1000)
    one.id_offset = 0
    one.reserve(5000)
    assert one._x.shape[0] == 5000 and one._xsq.shape[0] == 5000
    assert torch.equal(one._xsq[:N].view(torch.int32), whole.view(torch.int32))
    assert_matches(one.search(qb, k), want)
    one.reset()
    assert one.ntotal == 0 and one._xnorm_max is None
    s0, i0 = one.search(torch.from_numpy(qb[:3]).cuda(), 5)
    assert bool((i0 == -1).all()) and bool(torch.isposinf(s0).all())
    one.add(xb[:10])
    assert_matches(one.search(qb[:3], 5), oracle_topk_l2(torch.from_numpy(xb[:10]).cuda(), torch.from_numpy(qb[:3]).cuda(), 5))


@pytest.mark.gpu
def test_flat_l2_index_above_the_exact_route_uses_its_cached_norms():
    """An index large enough for the fast route, added in three uneven pieces: the search reads the cached xsq / xnorm_max."""
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatL2Index
    N, D, nq, k = 140001, 64, 16, 10
    x, q = _randn((N, D), 91), _randn((nq, D), 92)
    index = FlatL2Index(D, device="cuda")
    for a, b in ((0, 50000), (50000, 50007), (50007, N)):
        index.add(x[a:b])
    assert torch.equal(index._xsq[:N].view(torch.int32), ops.dense_row_sqnorms(x).view(torch.int32))
    want = oracle_topk_l2(x, q, k)
    assert_matches(index.search(q, k), want)
    assert index.last_search.stats == {"retried_queries": 0, "exact_queries": 0}
