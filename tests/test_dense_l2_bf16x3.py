"""bf16x3 matrix-core screen of the fp32 exact dense L2 search: csrc/dense_search_l2_bf16x3.hip, ops.dense_search_l2_bf16x3,
dense_index.FlatL2Bf16x3Index, create_index(metric="l2") and run_dense_eval's --index_metric.

The contract: the corpus stays fp32 and nothing is rounded in the result; ids and distance bits equal `ops.dense_search_l2`
and the chain oracle of test_dense_l2.py on the same arrays.  The bf16 matrix cores only screen, with
sigma~ = fmaf(2, s~, -xsq), s~ = sum_d (q_h x_h + q_h x_l + q_l x_h) of the round-to-nearest-even splits; its error against
chain - ||q||^2 must stay inside the bound the certificate uses (ops.dense_l2_bf16x3_error_bound),
    E = (5 D_pad 2^-24 + 2 * 2^-16) (||q|| + X)^2 + 4 * 2^-126 sqrt(D_pad) (||q|| + X) + 8 D_pad 2^-149."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from test_dense_flat import assert_matches, fmaf_emul
from test_dense_l2 import _families, _randn, _sqnorm32, chain_l2, oracle_topk_l2
from test_dense_bf16x3 import _accumulate, _split

U = 2.0 ** -24


def _ratio(sigma, q, x, d_chain, D):
    """|sigma~ - ||q||^2 + d_chain| / E_q per pair, with each row's own norm as X."""
    from repconc_amd import ops
    q64, x64 = q.astype(np.float64), x.astype(np.float64)
    qq = (q64 * q64).sum(1)
    err = np.abs(sigma.astype(np.float64) - qq + d_chain.astype(np.float64))
    E = ops.dense_l2_bf16x3_error_bound(D, np.sqrt(qq), np.sqrt((x64 * x64).sum(1)))
    assert np.all(E > 0)
    return err / E


# --------------------------------------------------------------------------------------------------------------- CPU
def test_l2_bf16x3_error_constants_are_the_librarys():
    import ctypes
    from repconc_amd import _lib, ops
    c = (ctypes.c_double * 4)()
    _lib.load().rc_dense_l2_bf16x3_error_constants(c)
    assert tuple(c) == (5.0, 2.0, 4 * 2.0 ** -126, 8 * 2.0 ** -149)
    assert ops.dense_l2_bf16x3_error_constants() == tuple(c)
    # D = 100 -> D_pad = 112, ||q|| + X = 8, R = 64
    assert ops.dense_l2_bf16x3_error_bound(100, 3.0, 5.0) == \
        (5 * 112 * U + 2 * 2.0 ** -16) * 64.0 + 4 * 2.0 ** -126 * 112 ** 0.5 * 8.0 + 8 * 2.0 ** -149 * 112
    assert ops.dense_l2_bf16x3_error_bound(16, 0.0, 0.0) == 128 * 2.0 ** -149


def _screen_terms(q, x):
    """The 3 D products of the screen, [P, 3 D] fp32.  Each is checked exact in fp32 unless it underflows (below 2^-126 it is
    rounded to a multiple of 2^-149, to nearest: what the bound's E_under charges)."""
    qh, ql = _split(q)
    xh, xl = _split(x)
    terms = []
    for a, b in ((qh, xh), (qh, xl), (ql, xh)):
        p64 = a.astype(np.float64) * b.astype(np.float64)                   # 16 significant bits: exact in fp64
        p = p64.astype(np.float32)
        normal = np.abs(p64) >= 2.0 ** -126
        assert np.array_equal(p.astype(np.float64)[normal], p64[normal])
        assert np.all(np.abs(p.astype(np.float64) - p64)[~normal] <= 2.0 ** -150)
        terms.append(p)
    return np.concatenate(terms, axis=1)


@pytest.mark.parametrize("D", [16, 100, 768, 4096])
def test_l2_bf16x3_error_bound_covers_an_emulated_screen(D):
    """s~ as an fp32 accumulation of the split products in 8 random orders and groupings (depth 1 / 2 / 8 / 32, sequential or
    pairwise inside a group, every addition rounded to nearest or truncated), sigma~ as an fp32 fma with the fp64-rounded xsq,
    against chain - ||q||^2: every family of test_dense_l2.py."""
    rng = np.random.default_rng(18000 + D)
    P = 32
    fam = _families(rng, P, D)
    q = np.concatenate([v[0] for v in fam.values()])
    x = np.concatenate([v[1] for v in fam.values()])
    terms = _screen_terms(q, x)
    assert terms.shape == (len(fam) * P, 3 * D)
    chain = chain_l2(q, x)
    nxs = -_sqnorm32(x)
    worst = np.zeros(len(fam))
    for trial in range(8):
        depth, pairwise, truncate = (1, 32, 8, 2)[trial // 2], (trial // 2) % 2 == 1, bool(trial % 2)
        dot = _accumulate(terms, rng, depth, pairwise=pairwise, truncate=truncate)
        sigma = fmaf_emul(np.full(dot.shape, 2.0, np.float32), dot, nxs)
        worst = np.maximum(worst, _ratio(sigma, q, x, chain, D).reshape(len(fam), P).max(1))
    for name, w in zip(fam, worst):
        print(f"D={D} {name}: worst |sigma~ - ||q||^2 + d| / E_q over 8 accumulations = {w:.4g}")
    assert np.all(worst < 1.0)


def test_l2_bf16x3_workspace_helpers_and_argument_errors_need_no_gpu():
    import torch
    from repconc_amd import _lib, ops
    lib = _lib.load()
    N, D = 8841823, 768
    prev = 0
    for nq in (1, 7, 128, 1200, 2048):
        ws = lib.rc_dense_l2_bf16x3_search_ws_bytes(N, D, nq, 1000)
        assert ws > prev
        assert ws >= lib.rc_dense_l2_search_ws_bytes(N, D, nq, 1000) + nq * D * 4      # the two bf16 planes of the queries
        assert ws == lib.rc_dense_bf16x3_search_ws_bytes(N, D, nq, 1000)
        prev = ws
    assert lib.rc_dense_l2_bf16x3_search_ws_bytes(1000, D, 1200, 10) == lib.rc_dense_l2_search_exact_ws_bytes(1000, D, 1200, 10)
    for args in ((N, D, 1200, 8193), (1 << 32, D, 4, 10), (0, D, 4, 10), (N, 0, 4, 10), (N, D, 0, 10), (N, D, 4, 0)):
        assert lib.rc_dense_l2_bf16x3_search_ws_bytes(*args) == 0
    assert lib.rc_dense_l2_bf16x3_scores_ws_bytes(100, 8) >= 2 * 8 * 128 * 2
    assert lib.rc_dense_l2_bf16x3_scores_ws_bytes(0, 8) == 0 and lib.rc_dense_l2_bf16x3_scores_ws_bytes(100, 0) == 0
    RC_ESHAPE, RC_EINVAL = -2, -1
    z = None
    # shapes before pointers
    assert lib.rc_dense_l2_bf16x3_search_q(z, z, D, N, D, z, 4, z, z, 8193, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_bf16x3_search_q(z, z, D, 1 << 32, D, z, 4, z, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_bf16x3_search_q(z, z, D, N, D, z, 4, z, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_EINVAL
    assert lib.rc_dense_l2_bf16x3_scores(z, z, D, 1 << 32, D, z, 4, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_bf16x3_scores(z, z, D, N, D, z, 4, z, z, z, 0, z) == RC_EINVAL
    x, q = torch.zeros(10, 16), torch.zeros(2, 16)
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_search_l2_bf16x3(x, q, 1)                       # CPU tensors
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_l2_bf16x3_scores(x, q)
    for k in (0, 8193):
        with pytest.raises(ValueError):
            ops.dense_search_l2_bf16x3(x, q, k)
    with pytest.raises(ValueError):
        ops.dense_search_l2_bf16x3(x, q, 1, method="fast")


def test_l2_bf16x3_index_and_create_index_options_need_no_gpu():
    import torch
    from repconc_amd.dense_index import FlatL2Bf16x3Index, FlatL2Index
    from repconc_amd.models.dense.evaluate_dense import check_index_options, create_index
    xb = np.zeros((4, 16), np.float32)
    for kw in (dict(metric="cos"), dict(metric="l2", use_float16=True, screen="bf16x3"),
               dict(metric="ip", use_float16=True, screen="bf16x3"), dict(metric="l2", screen="fp8"), dict(screen="fp8")):
        with pytest.raises(ValueError):
            create_index(xb, **kw)                                # raised before any device is looked at
        with pytest.raises(ValueError):
            check_index_options(kw.get("metric", "ip"), kw.get("use_float16", False), kw.get("screen", "fp32"))
    for metric in ("ip", "l2"):
        for f16, screen in ((False, "fp32"), (True, "fp32"), (False, "bf16x3")):
            check_index_options(metric, f16, screen)
    index = FlatL2Bf16x3Index(16, device="cpu")                   # holds nothing: the width is checked before any device work
    assert index.metric_type == 1 and index.ntotal == 0 and index._x.dtype == torch.float32
    assert not isinstance(index, FlatL2Index)
    with pytest.raises(ValueError):
        index.add(np.zeros((3, 17), np.float32))
    with pytest.raises(ValueError):
        index.search(np.zeros((3, 17), np.float32), 1)
    with pytest.raises(TypeError):
        FlatL2Bf16x3Index(16, screen="bf16x3")


def test_eval_arguments_parse_index_metric(tmp_path):
    from transformers import HfArgumentParser
    from repconc_amd.evaluate import run_dense_eval as rde
    out = str(tmp_path / "o")
    (e,) = HfArgumentParser((rde.EvalArguments,)).parse_args_into_dataclasses(["--output_dir", out, "--report_to", "none"])
    assert e.index_metric == "ip"
    (e,) = HfArgumentParser((rde.EvalArguments,)).parse_args_into_dataclasses(
        ["--output_dir", out, "--report_to", "none", "--index_metric", "l2", "--index_screen", "bf16x3"])
    assert e.index_metric == "l2" and e.index_screen == "bf16x3"
    # refused before anything is loaded or encoded: the model path does not exist
    base = ["--model_name_or_path", str(tmp_path / "no_model"), "--corpus_path", "c", "--out_corpus_dir", str(tmp_path / "oc"),
            "--query_path", "q", "--out_query_dir", str(tmp_path / "oq"), "--output_dir", out, "--report_to", "none"]
    with pytest.raises(SystemExit):
        rde.main(base + ["--index_metric", "cos"])
    with pytest.raises(ValueError):
        rde.main(base + ["--index_metric", "l2", "--index_float16", "--index_screen", "bf16x3"])
    assert not os.path.exists(tmp_path / "oc") and not os.path.exists(tmp_path / "oq")


# --------------------------------------------------------------------------------------------------------------- GPU
def _assert_same_bits(got, ref):
    a = [np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in got]
    b = [np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in ref]
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


FAST_SHAPES = [
    (140001, 768, 257, 10),     # fast route, ragged rows and queries
    (140001, 100, 1, 8192),     # the PAD instantiation of the screen, the largest k
    (140001, 384, 128, 1000),
    (140001, 101, 64, 100),     # unaligned rows: the element-wise rescoring
]
SHAPES = [
    (5, 100, 7, 8),             # k > N, padded D: +inf / -1
    (1000, 384, 128, 1000),     # k = N
] + FAST_SHAPES
_fast_route_counts = {}         # shape -> (queries, retried + exact) of the auto search, for the pooled test below


@pytest.mark.gpu
@pytest.mark.parametrize("N,D,nq,k", SHAPES)
def test_l2_bf16x3_search_ids_and_distance_bits_equal_the_oracle_and_the_fp32_search(N, D, nq, k):
    from repconc_amd import ops
    x = _randn((N, D), 1000 + N + D)
    q = _randn((nq, D), 2000 + nq + D)
    want = oracle_topk_l2(x, q, k)
    pending = ops.dense_search_l2_bf16x3(x, q, k, id_offset=7, defer=True)
    got = pending.result()
    assert got[0].shape == (nq, k) and got[1].dtype.is_floating_point is False
    assert_matches(got, want, id_offset=7)
    _assert_same_bits(got, ops.dense_search_l2(x, q, k, id_offset=7))
    _fast_route_counts[(N, D, nq, k)] = (nq, pending.stats["retried_queries"] + pending.stats["exact_queries"])
    assert_matches(ops.dense_search_l2_bf16x3(x, q, k, id_offset=7, method="exact"), want, id_offset=7)


@pytest.mark.gpu
def test_l2_bf16x3_fast_route_is_really_taken():
    """Pooled over the fast-route shapes: at most 1 % of the queries are repeated or answered by the exact route (a condition:
    the certificate's bound leaves room; measured on the MI355X: 0 of 450, profiles/dense_l2_bf16x3_pytest_gpu.txt)."""
    from repconc_amd import ops
    for shape in FAST_SHAPES:
        if shape not in _fast_route_counts:                 # run alone: the search again, without the oracle
            N, D, nq, k = shape
            pending = ops.dense_search_l2_bf16x3(_randn((N, D), 1000 + N + D), _randn((nq, D), 2000 + nq + D), k, defer=True)
            pending.result()
            _fast_route_counts[shape] = (nq, pending.stats["retried_queries"] + pending.stats["exact_queries"])
    total = sum(_fast_route_counts[s][0] for s in FAST_SHAPES)
    flagged = sum(_fast_route_counts[s][1] for s in FAST_SHAPES)
    print(f"fast route: {flagged} of {total} queries repeated or answered by the exact route")
    assert flagged <= 0.01 * total


@pytest.mark.gpu
def test_l2_bf16x3_search_row_pitch_wider_than_d():
    """100-wide rows at a pitch of 104: 16-byte aligned rows with a tail after the last whole vector."""
    from repconc_amd import ops
    N, D, nq, k = 140001, 100, 33, 10
    buf = _randn((N, 104), 71)
    x = buf[:, :D]
    q = _randn((nq, D), 72)
    want = oracle_topk_l2(x.contiguous(), q, k)
    assert x.stride(0) == 104
    assert_matches(ops.dense_search_l2_bf16x3(x, q, k), want)
    assert_matches(ops.dense_search_l2_bf16x3(x, q, k, method="exact"), want)


@pytest.mark.gpu
def test_l2_bf16x3_row_norms_that_grow_with_the_row_index():
    """x_i = g_i (0.5 + 1.5 i / N): the squared norm of sample row j is that of corpus row j N / S, far from that of row j.  A
    sample pass that read xsq[j] would put the threshold where no row reaches it and flag every query."""
    import torch
    from repconc_amd import ops
    N, D, nq = 140001, 64, 64
    x = _randn((N, D), 93) * (0.5 + 1.5 * torch.arange(N, device="cuda:0", dtype=torch.float32) / N)[:, None]
    q = _randn((nq, D), 94)
    for k in (10, 100):
        want = oracle_topk_l2(x, q, k)
        pending = ops.dense_search_l2_bf16x3(x, q, k, defer=True)
        assert_matches(pending.result(), want)
        assert pending.stats == {"retried_queries": 0, "exact_queries": 0}, (k, pending.stats)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 100, 768, 1024])
def test_l2_bf16x3_screen_error_stays_inside_the_certificate_bound(D):
    """The raw sigma~ of the matrix cores against chain - ||q||^2: 16 x 16 pairs per family of test_dense_l2.py."""
    import torch
    from repconc_amd import ops
    rng = np.random.default_rng(100 + D)
    worst = 0.0
    for name, (q, x) in _families(rng, 16, D).items():
        xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(q).cuda()
        xsq = ops.dense_row_sqnorms(xd)
        sigma = ops.dense_l2_bf16x3_scores(xd, qd, xsq).cpu().numpy()       # [16 queries][16 rows]
        assert np.all(np.isfinite(sigma))
        qp, xp = np.repeat(q, 16, axis=0), np.tile(x, (16, 1))
        r = _ratio(sigma.reshape(-1), qp, xp, chain_l2(qp, xp), D)
        print(f"D={D} {name}: max |sigma~ - ||q||^2 + d| / E_q = {r.max():.5f}, max |sigma~| = {np.abs(sigma).max():.3e}")
        assert r.max() <= 1.0
        worst = max(worst, float(r.max()))
    print(f"D={D}: largest screen-error ratio {worst:.5f}")


@pytest.mark.gpu
def test_l2_bf16x3_self_matches_are_plus_zero_and_ties_take_the_lower_id():
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
    got = ops.dense_search_l2_bf16x3(x, q, k)
    assert_matches(got, want)
    d, i = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.all(d[:, :2].view(np.uint32) == 0)             # the two zero distances are +0.0f
    assert np.all(i[:, 0] < i[:, 1]) and np.all(d[:, 2] > 0)


@pytest.mark.gpu
def test_l2_bf16x3_tie_group_across_the_kth_distance_falls_back_to_the_exact_route():
    """20 000 identical rows whose distance sits inside every query's top-100: the group overflows the candidate list
    whatever the slack, the exact route answers."""
    from repconc_amd import ops
    N, D, nq, k = 150000, 64, 4, 100
    x = _randn((N, D), 35)
    q = 0.05 * _randn((nq, D), 36)
    v = _randn((D,), 37)
    x[90000:110000] = (v * (32.0 ** 0.5 / v.norm()))[None]   # |v|^2 = 32: a few dozen of the gaussian rows are nearer
    want = oracle_topk_l2(x, q, k)
    tied = (want[1] >= 90000) & (want[1] < 110000)
    assert tied.any(1).all() and (~tied).any(1).all()        # the tie group straddles the k-th distance of every query
    pending = ops.dense_search_l2_bf16x3(x, q, k, defer=True)
    assert_matches(pending.result(), want)
    assert pending.stats["exact_queries"] > 0


@pytest.mark.gpu
def test_l2_bf16x3_certificate_refuses_distances_closer_than_the_screen_error():
    """Every row and query is one vector of norm ~30 plus 1e-4 noise: all distance differences are far below E_q, no answer
    of the fast route can be certified, every query ends on the exact route with the oracle's result."""
    from repconc_amd import ops
    N, D, nq, k = 200000, 64, 8, 10
    base = _randn((D,), 81)
    base *= 30.0 / base.norm()
    x = base[None] + 1e-4 * _randn((N, D), 82)
    q = base[None] + 1e-4 * _randn((nq, D), 83)
    want = oracle_topk_l2(x, q, k)
    eq = ops.dense_l2_bf16x3_error_bound(D, 30.0, 30.0)
    assert float(want[0].max()) < 1e-2 * eq
    pending = ops.dense_search_l2_bf16x3(x, q, k, defer=True)
    assert bool(((pending._qstatus & 4) != 0).all())          # bit 2 on every query of the first pass
    assert_matches(pending.result(), want)
    assert pending.stats["exact_queries"] == nq


@pytest.mark.gpu
def test_l2_bf16x3_negative_slack_forces_retries_with_unchanged_results():
    from repconc_amd import ops
    N, D, nq, k = 140001, 128, 64, 100
    x, q = _randn((N, D), 41), _randn((nq, D), 42)
    want = oracle_topk_l2(x, q, k)
    pending = ops.dense_search_l2_bf16x3(x, q, k, sel_slack=-50.0, defer=True)
    got = pending.result()
    assert pending.stats["retried_queries"] > 0
    assert_matches(got, want)
    assert_matches(ops.dense_search_l2_bf16x3(x, q, k), want)


@pytest.mark.gpu
def test_flat_l2_bf16x3_index_add_grow_reset_search_equal_the_fp32_index():
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatL2Bf16x3Index, FlatL2Index
    N, D, nq, k = 3000, 100, 50, 20
    xb = _randn((N, D), 61).cpu().numpy()
    qb = _randn((nq, D), 62).cpu().numpy()
    ref = FlatL2Index(D, device="cuda")
    ref.add(xb)
    one = FlatL2Bf16x3Index(D)
    assert one.is_trained and one.metric_type == 1 and one.d == D
    s0, i0 = one.search(qb[:3], 5)                                   # the empty index
    assert np.all(i0 == -1) and np.all(np.isposinf(s0))
    one.add(xb)
    assert one.ntotal == N and one._x.shape[0] == N and one._xsq.shape[0] == N and one._x.dtype == torch.float32
    three = FlatL2Bf16x3Index(D, device="cuda")
    three.add(xb[:1000])
    three.add(torch.from_numpy(xb[1000:1100]).cuda())
    assert three._x.shape[0] == 1500 and three._xsq.shape[0] == 1500                # growth 1.5x, the norms with it
    three.add(xb[1100:])
    assert three.ntotal == N and bool((three.xb == ref.xb).all())
    whole = ops.dense_row_sqnorms(torch.from_numpy(xb).cuda())
    for ix in (one, three):
        assert torch.equal(ix._xsq[:N].view(torch.int32), whole.view(torch.int32))
        assert float(ix._xnorm_max) >= float(whole.max().sqrt())
    sr, ir = ref.search(qb, k)
    s1, i1 = one.search(qb, k)
    assert isinstance(s1, np.ndarray) and isinstance(i1, np.ndarray) and i1.dtype == np.int64 and s1.dtype == np.float32
    _assert_same_bits((s1, i1), (sr, ir))
    _assert_same_bits(three.search(qb, k), (sr, ir))
    assert_matches((s1, i1), oracle_topk_l2(torch.from_numpy(xb).cuda(), torch.from_numpy(qb).cuda(), k))
    st, it = one.search(torch.from_numpy(qb).cuda(), k)
    assert isinstance(st, torch.Tensor) and st.is_cuda and it.is_cuda
    _assert_same_bits((st, it), (sr, ir))
    fins = [one.search_async(part, k) for part in np.array_split(qb, 4)]         # enqueued before any is finished
    parts = [f() for f in fins]
    _assert_same_bits((np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])), (sr, ir))
    for bad in (3.4e38, float("inf"), float("nan")):                             # >= 2^128 - 2^119 rounds to a bf16 inf
        xbad = np.zeros((2, D), np.float32)
        xbad[1, 5] = bad
        with pytest.raises(ValueError):
            one.add(xbad)
        assert one.ntotal == N and one._x.shape[0] == N and one._xsq.shape[0] == N   # nothing stored, nothing grown
    one.reset()
    assert one.ntotal == 0 and one._xnorm_max is None and one._xsq.shape[0] == 0
    s0, i0 = one.search(torch.from_numpy(qb[:3]).cuda(), 5)
    assert bool((i0 == -1).all()) and bool(torch.isposinf(s0).all())
    one.add(xb[:10])
    assert_matches(one.search(qb[:3], 5), oracle_topk_l2(torch.from_numpy(xb[:10]).cuda(), torch.from_numpy(qb[:3]).cuda(), 5))


@pytest.mark.gpu
def test_flat_l2_bf16x3_index_above_the_exact_route_uses_its_cached_norms():
    """An index large enough for the fast route, added in three uneven pieces: the search reads the cached xsq / xnorm_max."""
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatL2Bf16x3Index
    N, D, nq, k = 140001, 64, 16, 10
    x, q = _randn((N, D), 91), _randn((nq, D), 92)
    index = FlatL2Bf16x3Index(D, device="cuda")
    for a, b in ((0, 50000), (50000, 50007), (50007, N)):
        index.add(x[a:b])
    assert torch.equal(index._xsq[:N].view(torch.int32), ops.dense_row_sqnorms(x).view(torch.int32))
    want = oracle_topk_l2(x, q, k)
    assert_matches(index.search(q, k), want)
    assert index.last_search.stats == {"retried_queries": 0, "exact_queries": 0}
    index._xnorm_max = torch.full_like(index._xnorm_max, float("inf"))      # the cached bound is what the certificate reads:
    assert_matches(index.search(q, k), want)                                # with it infinite nothing is certified
    assert index.last_search.stats["exact_queries"] == nq


@pytest.mark.gpu
def test_create_index_l2_returns_the_three_classes_and_batches_like_the_loop():
    import torch
    from repconc_amd.dense_index import FlatL2Bf16x3Index, FlatL2F16Index, FlatL2Index
    from repconc_amd.models.dense.evaluate_dense import batch_dense_search, create_index, dense_search
    N, D, nq, k = 3000, 384, 50, 20
    xb = _randn((N, D), 61).cpu().numpy()
    qb = _randn((nq, D), 62).cpu().numpy()
    plain = create_index(xb, metric="l2")
    half = create_index(xb, metric="l2", use_float16=True)
    b3 = create_index(xb, metric="l2", screen="bf16x3")
    assert type(plain) is FlatL2Index and type(half) is FlatL2F16Index and type(b3) is FlatL2Bf16x3Index
    assert plain.ntotal == half.ntotal == b3.ntotal == N and half._x.dtype == torch.float16
    corpus_ids = np.array([f"d{i}" for i in range(N)])
    qids = np.arange(nq)
    got = {}
    for name, index in (("plain", plain), ("half", half), ("b3", b3)):
        bs, bi = batch_dense_search(qids, qb, corpus_ids, index, k, batch_size=16)
        loop = [dense_search(a, b, corpus_ids, index, k) for a, b in zip(np.array_split(qids, 4), np.array_split(qb, 4))]
        assert np.array_equal(bi, np.concatenate([g[1] for g in loop]))
        assert np.array_equal(bs.view(np.uint32), np.concatenate([g[0] for g in loop]).view(np.uint32))
        assert np.all(bs[:, 1:] >= bs[:, :-1]) and np.all(bs >= 0)
        got[name] = (bs, bi)
    assert np.array_equal(got["b3"][1], got["plain"][1])
    assert np.array_equal(got["b3"][0].view(np.uint32), got["plain"][0].view(np.uint32))
    want = oracle_topk_l2(torch.from_numpy(xb).cuda(), torch.from_numpy(qb).cuda(), k)
    assert np.array_equal(got["b3"][1], corpus_ids[want[1]])


@pytest.mark.gpu
@pytest.mark.parametrize("screen", ["fp32", "bf16x3"])
def test_search_and_compute_metrics_with_the_l2_metric_writes_negated_distances(tmp_path, screen):
    """Planted relevance: query j is document 7 j plus noise, its second judged document lies farther away; rows have norms
    between 1 and 30, so the inner product would rank by norm.  run.tsv holds -d, descending, and metric.json equals the
    metrics of the L2 ranking computed directly."""
    import torch
    from repconc_amd import ops
    from repconc_amd.evaluate.run_dense_eval import search_and_compute_metrics
    from repconc_amd.utils.eval_utils import pytrec_evaluate
    N, D, nq, k = 2000, 32, 20, 10
    rng = np.random.default_rng(5)
    xb = (rng.standard_normal((N, D)) * rng.uniform(1.0, 30.0, (N, 1)) / np.sqrt(D)).astype(np.float32)
    qb = (xb[7 * np.arange(nq)] + 0.01 * rng.standard_normal((nq, D))).astype(np.float32)
    xb[7 * np.arange(nq) + 1] = (qb + 0.05 * rng.standard_normal((nq, D))).astype(np.float32)
    corpus_ids = np.array([f"d{i}" for i in range(N)])
    qids = np.arange(100, 100 + nq)
    qrel = {str(100 + j): {f"d{7 * j}": 2, f"d{7 * j + 1}": 1, f"d{7 * j + 2}": 1} for j in range(nq)}
    with open(tmp_path / "qrels", "w") as f:
        for qid, docs in qrel.items():
            for d, r in docs.items():
                f.write(f"{qid} 0 {d} {r}\n")
    args = SimpleNamespace(index_metric="l2", index_float16=False, index_screen=screen, topk=k, search_batch=7)
    search_and_compute_metrics(xb, corpus_ids, qb, qids, str(tmp_path / "metric.json"), str(tmp_path), str(tmp_path / "qrels"),
                               args)
    dist, ids = ops.dense_search_l2_exact(torch.from_numpy(xb).cuda(), torch.from_numpy(qb).cuda(), k)
    dist, ids = dist.cpu().numpy(), ids.cpu().numpy()
    assert np.all(ids[:, 0] == 7 * np.arange(nq)) and np.all(ids[:, 1] == 7 * np.arange(nq) + 1)
    lines = [ln.rstrip("\n").split("\t") for ln in open(tmp_path / "run.tsv")]
    assert len(lines) == nq * k
    for j in range(nq):
        rows = lines[j * k:(j + 1) * k]
        assert [r[0] for r in rows] == [str(100 + j)] * k and [int(r[3]) for r in rows] == list(range(1, k + 1))
        assert [r[2] for r in rows] == [f"d{i}" for i in ids[j]]
        scores = [float(r[4]) for r in rows]
        assert scores == [-float(v) for v in dist[j]]               # the exact negation, written as its repr
        assert all(a >= b for a, b in zip(scores, scores[1:])) and scores[0] <= 0.0
    direct = {str(100 + j): {f"d{i}": -float(v) for i, v in zip(ids[j], dist[j])} for j in range(nq)}
    want = pytrec_evaluate(qrel, direct)
    got = json.load(open(tmp_path / "metric.json"))
    assert got == json.loads(json.dumps(want))
    assert got["mrr"]["MRR@10"] == 1.0 and got["recall"]["Recall@10"] < 1.0
