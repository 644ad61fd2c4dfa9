"""fp16 corpus storage of the exact dense L2 search: csrc/dense_search_l2_f16.hip, ops.dense_search_l2_f16,
dense_index.FlatL2F16Index.

The contract: values and queries are rounded to IEEE fp16 (round to nearest even); a distance is the fp32 chain of
tests/test_dense_l2.py over the widened values, so ids and distance bits equal the fp32 L2 search (and its oracle) on
x16.float(), q.half().float().  The f16 matrix cores only screen with sigma = fmaf(2, dot, -xsq): its error against
chain - ||q||^2 must stay inside the bound the certificate uses, E = 2.5 D_pad 2^-24 (||q|| + X)^2
(ops.dense_l2_f16_error_bound; derivation in the header of csrc/dense_search_l2_f16.hip)."""
import numpy as np
import pytest

from test_dense_f16 import _accumulate
from test_dense_flat import assert_matches, fmaf_emul
from test_dense_l2 import _sqnorm32, chain_l2, oracle_topk_l2

U = 2.0 ** -24


def _f16(a):
    """fp64 -> the nearest finite fp16, as fp32."""
    return np.clip(np.asarray(a, dtype=np.float64), -65504, 65504).astype(np.float16).astype(np.float32)


def _families(rng, P, D):
    """fp16-representable pairs (q, x), [P, D] fp32 each."""
    n = lambda: rng.standard_normal((P, D))
    q = _f16(n())
    fam = {"N(0,1)": (q, _f16(n()))}
    fam["x = q"] = (q, q.copy())
    up = np.where(rng.random((P, D)) < 0.5, np.inf, -np.inf).astype(np.float16)
    fam["x = q + one fp16 ulp"] = (q, np.nextafter(q.astype(np.float16), up).astype(np.float32))
    fam["x = q + 1e-3 noise"] = (q, _f16(q + 1e-3 * n()))
    fam["|x| = 1000 |q|"] = (q, _f16(1000.0 * n()))
    fam["magnitudes 2^-24..6e4"] = (_f16(n() * 2.0 ** rng.integers(-24, 16, (P, D))),
                                    _f16(n() * 2.0 ** rng.integers(-24, 16, (P, D))))
    fam["both subnormal"] = (_f16(rng.integers(-1023, 1024, (P, D)) * 2.0 ** -24),
                             _f16(rng.integers(-1023, 1024, (P, D)) * 2.0 ** -24))
    fam["x subnormal"] = (q, _f16(rng.integers(-1023, 1024, (P, D)) * 2.0 ** -24))
    for a, b in fam.values():
        assert np.isfinite(a).all() and np.isfinite(b).all()
        assert np.array_equal(a, a.astype(np.float16).astype(np.float32)) and np.array_equal(b, b.astype(np.float16).astype(np.float32))
    return fam


def _ratio(sigma, q, x, d_chain, D):
    """|sigma - ||q||^2 + d_chain| / E_q per pair, with each row's own norm as X."""
    from repconc_amd import ops
    q64, x64 = q.astype(np.float64), x.astype(np.float64)
    qq = (q64 * q64).sum(1)
    err = np.abs(sigma.astype(np.float64) - qq + d_chain.astype(np.float64))
    E = ops.dense_l2_f16_error_bound(D, np.sqrt(qq), np.sqrt((x64 * x64).sum(1)))
    ok = E > 0
    assert np.all(err[~ok] == 0)                                   # q = x = 0: nothing to bound, nothing off
    return np.where(ok, err / np.where(ok, E, 1.0), 0.0)


# --------------------------------------------------------------------------------------------------------------- CPU
def test_l2_f16_error_constants_are_the_librarys():
    from repconc_amd import _lib, ops
    c = (_lib.C.c_double * 2)()
    _lib.load().rc_dense_l2_f16_error_constants(c)
    assert tuple(c) == (2.5, 65536.0) == ops.dense_l2_f16_error_constants()
    assert ops.dense_l2_f16_error_bound(100, 3.0, 5.0) == 2.5 * 112 * U * 64.0                 # D_pad = D up to 16
    assert ops.dense_l2_f16_error_bound(768, 2.0, 3.0) == 2.5 * 768 * U * 25.0
    e = ops.dense_l2_f16_error_bound(16, np.array([1.0, 2.0]), np.array([3.0, 2.0]))
    assert e.shape == (2,) and e[0] == e[1] == 2.5 * 16 * U * 16.0


def test_l2_f16_error_bound_covers_any_fp32_accumulation_of_the_exact_products():
    """sigma = fmaf(2, dot, -xsq) with dot from adversarial fp32 accumulations of the exact fp16 products (random orders and
    groupings, additions rounded to nearest or truncated) and the fp64-rounded norm, against chain - ||q||^2."""
    rng = np.random.default_rng(2317)
    P = 16
    worst_all = 0.0
    for D in (16, 100, 768, 4096):
        fam = _families(rng, P, D)
        q = np.concatenate([v[0] for v in fam.values()])
        x = np.concatenate([v[1] for v in fam.values()])
        prod = (q.astype(np.float64) * x.astype(np.float64)).astype(np.float32)
        assert np.array_equal(prod.astype(np.float64), q.astype(np.float64) * x.astype(np.float64))     # exact in fp32
        d = chain_l2(q, x)
        nxs = -_sqnorm32(x)
        worst = np.zeros(len(fam))
        for trial in range(8):
            dot = _accumulate(prod, rng, truncate=bool(trial % 2))
            sigma = fmaf_emul(np.full(dot.shape, 2.0, np.float32), dot, nxs)
            worst = np.maximum(worst, _ratio(sigma, q, x, d, D).reshape(len(fam), P).max(1))
        for name, w in zip(fam, worst):
            print(f"D={D} {name}: worst |sigma - ||q||^2 + d| / E_q over 8 accumulations = {w:.4g}")
        assert np.all(worst < 1.0)
        worst_all = max(worst_all, float(worst.max()))
    print(f"worst ratio {worst_all:.4f}")


def test_l2_f16_workspace_helpers_and_argument_errors_need_no_gpu():
    import torch
    from repconc_amd import _lib, ops
    from repconc_amd.dense_index import FlatL2F16Index, FlatL2Index
    lib = _lib.load()
    N, D = 8841823, 768
    assert lib.rc_dense_l2_f16_search_ws_bytes(N, D, 1200, 1000) >= 1200 * (32768 * 4 + 16384 * 8)
    assert lib.rc_dense_l2_f16_search_ws_bytes(N, D, 1200, 1000) == lib.rc_dense_l2_search_ws_bytes(N, D, 1200, 1000)
    assert lib.rc_dense_l2_f16_search_ws_bytes(1000, D, 1200, 10) == lib.rc_dense_l2_f16_search_exact_ws_bytes(1000, D, 1200, 10)
    assert lib.rc_dense_l2_f16_search_exact_ws_bytes(N, D, 7, 100) == lib.rc_dense_search_exact_ws_bytes(N, D, 7, 100)
    for args in ((N, D, 1200, 8193), (1 << 32, D, 4, 10), (0, D, 4, 10), (N, 0, 4, 10), (N, D, 0, 10), (N, D, 4, 0)):
        assert lib.rc_dense_l2_f16_search_ws_bytes(*args) == 0 and lib.rc_dense_l2_f16_search_exact_ws_bytes(*args) == 0
    RC_ESHAPE, RC_EINVAL = -2, -1
    z = None
    assert lib.rc_dense_l2_f16_search_q(z, z, D, N, D, z, 4, z, z, 8193, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_f16_search_q(z, z, D, 1 << 32, D, z, 4, z, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_f16_search_exact(z, z, D, N, D, z, 4, 8193, 0, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_f16_search_q(z, z, D, N, D, z, 4, z, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_EINVAL
    assert lib.rc_dense_l2_f16_search_exact(z, z, D, N, D, z, 4, 10, 0, z, z, z, 0, z) == RC_EINVAL
    assert lib.rc_dense_l2_f16_scores(z, z, D, 1 << 32, D, z, 4, z, z, z) == RC_ESHAPE
    assert lib.rc_dense_l2_f16_scores(z, z, D, N, D, z, 4, z, z, z) == RC_EINVAL
    x16, q = torch.zeros(10, 16, dtype=torch.float16), torch.zeros(2, 16)
    with pytest.raises(ValueError):
        ops.dense_search_l2_f16(x16.float(), q, 1)                   # an fp32 corpus
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_search_l2_f16(x16, q, 1)                           # CPU tensors
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_search_l2_f16_exact(x16, q, 1)
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_l2_f16_scores(x16, q.half())
    for k in (0, 8193):
        with pytest.raises(ValueError):
            ops.dense_search_l2_f16(x16, q, k)
    with pytest.raises(ValueError):
        ops.dense_search_l2_f16(x16, q, 1, method="fast")
    index = FlatL2F16Index(16, device="cpu")                         # holds nothing: checked before any device work
    assert index.metric_type == 1 and index.ntotal == 0 and index.PAD == float("inf")
    assert index._x.dtype == torch.float16 and index.xb.dtype == torch.float16 and index._xsq.dtype == torch.float32
    assert not isinstance(index, FlatL2Index)
    with pytest.raises(ValueError):
        index.add(np.zeros((3, 17), np.float32))
    with pytest.raises(ValueError):
        index.search(np.zeros((3, 17), np.float32), 1)
    for bad in (65520.0, -65520.0, float("inf"), float("nan")):
        xb = np.zeros((2, 16), dtype=np.float32)
        xb[1, 5] = bad
        with pytest.raises(ValueError):
            index.add(xb)
        assert index.ntotal == 0 and index._x.shape[0] == 0 and index._xsq.shape[0] == 0       # nothing stored, nothing grown
    ok = np.full((4, 16), 65504.0, dtype=np.float32)
    ok[1, 3] = 65519.0                                               # still rounds to 65504
    index.add(ok)
    assert index.ntotal == 4 and float(index.xb.float().max()) == 65504.0
    assert np.array_equal(index._xsq.numpy(), _sqnorm32(np.full((4, 16), 65504.0, np.float32)))
    assert 65504.0 * 4.0 <= float(index._xnorm_max) < 65504.0 * 4.0 * 1.001
    index.reset()
    assert index.ntotal == 0 and index._x.dtype == torch.float16 and index._xnorm_max is None and index._xsq.shape[0] == 0


# --------------------------------------------------------------------------------------------------------------- GPU
def _inputs(N, D, nq):
    """The search tests' inputs, made on the CPU (so that the fast-route condition below can be simulated without a GPU) and
    copied to the device: (x16 fp16 [N, D], q fp32 [nq, D])."""
    import torch
    g = torch.Generator().manual_seed(N + D + nq)
    x = torch.randn(N, D, generator=g).half()
    q = torch.randn(nq, D, generator=g)
    return x.cuda(), q.cuda()


def _randn(shape, seed, dev="cuda:0"):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev, dtype=torch.float32)


FAST_SHAPES = [
    (140001, 768, 257, 10),     # fast route, ragged rows and queries
    (140001, 100, 1, 8192),     # D % 8 != 0: the PAD screen, the largest k
    (140001, 384, 128, 1000),
    (140001, 101, 64, 100),     # odd pitch: element-wise rescoring
    (140001, 104, 33, 10),      # D % 8 == 0 but a partly filled K stage of the screen (and K chunk of the exact kernel)
    (140001, 1040, 5, 10),      # a second 1024-value query chunk in the rescorer
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
def test_l2_f16_search_ids_and_distance_bits_equal_the_oracle_and_the_fp32_search(N, D, nq, k):
    from repconc_amd import ops
    x16, q = _inputs(N, D, nq)
    xw, qw = x16.float(), q.half().float()                           # the widened values: what the search scores
    want = oracle_topk_l2(xw, qw, k)
    assert np.all(want[0] >= 0) and np.all(want[0][:, 1:] >= want[0][:, :-1])
    pending = ops.dense_search_l2_f16(x16, q, k, id_offset=7, defer=True)
    got = pending.result()
    assert got[0].shape == (nq, k) and got[1].dtype.is_floating_point is False
    assert_matches(got, want, id_offset=7)
    _fast_route_counts[(N, D, nq, k)] = (nq, pending.stats["retried_queries"] + pending.stats["exact_queries"])
    assert_matches(ops.dense_search_l2_f16(x16, q, k, id_offset=7, method="exact"), want, id_offset=7)
    assert_matches(ops.dense_search_l2_f16_exact(x16, q, k, id_offset=7), want, id_offset=7)
    ref = ops.dense_search_l2(xw, qw, k, id_offset=7)                # the contract: the fp32 L2 search on the widened values
    assert_matches(got, (ref[0].cpu().numpy(), ref[1].cpu().numpy() - 7), id_offset=7)


@pytest.mark.gpu
def test_l2_f16_fast_route_is_really_taken():
    """Pooled over the six fast-route shapes: at most 1 % of the 488 queries are repeated or answered by the exact route.  A
    condition, not a measurement: a CPU simulation of sample, rank formula, threshold, list capacity and certificate on exactly
    these inputs flags 0 of 488 with E = 2.5 D_pad 2^-24 R, the constant the unit's header proves (smallest margin 7.9 E, on
    the D = 384 shape)."""
    from repconc_amd import ops
    for shape in FAST_SHAPES:
        if shape not in _fast_route_counts:                 # run alone: the search again, without the oracle
            N, D, nq, k = shape
            x16, q = _inputs(N, D, nq)
            pending = ops.dense_search_l2_f16(x16, q, k, defer=True)
            pending.result()
            _fast_route_counts[shape] = (nq, pending.stats["retried_queries"] + pending.stats["exact_queries"])
    total = sum(_fast_route_counts[s][0] for s in FAST_SHAPES)
    flagged = sum(_fast_route_counts[s][1] for s in FAST_SHAPES)
    print(f"fast route: {flagged} of {total} queries repeated or answered by the exact route")
    assert total == 488 and flagged <= 0.01 * total


@pytest.mark.gpu
def test_l2_f16_search_row_pitch_wider_than_d():
    """100-wide rows at a pitch of 104 halves: 16-byte aligned rows with a tail after the last whole vector."""
    from repconc_amd import ops
    N, D, nq, k = 140001, 100, 33, 10
    buf = _randn((N, 104), 71).half()
    x16 = buf[:, :D]
    q = _randn((nq, D), 72)
    want = oracle_topk_l2(x16.float().contiguous(), q.half().float(), k)
    assert x16.stride(0) == 104
    assert_matches(ops.dense_search_l2_f16(x16, q, k), want)
    assert_matches(ops.dense_search_l2_f16(x16, q, k, method="exact"), want)


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 100, 768, 1024])
def test_l2_f16_screen_error_stays_inside_the_certificate_bound(D):
    """The raw sigma of the f16 matrix cores against chain - ||q||^2: 16 x 16 pairs per family, the subnormal ones included (a
    matrix core that read an fp16 subnormal as zero would show here)."""
    import torch
    from repconc_amd import ops
    rng = np.random.default_rng(100 + D)
    worst = 0.0
    for name, (q, x) in _families(rng, 16, D).items():
        xd, qd = torch.from_numpy(x).cuda().half(), torch.from_numpy(q).cuda().half()
        xsq = ops.dense_row_sqnorms(xd)
        assert np.array_equal(xsq.cpu().numpy().view(np.uint32), _sqnorm32(x).view(np.uint32))
        sigma = ops.dense_l2_f16_scores(xd, qd, xsq).cpu().numpy()          # [16 queries][16 rows]
        qp, xp = np.repeat(q, 16, axis=0), np.tile(x, (16, 1))
        r = _ratio(sigma.reshape(-1), qp, xp, chain_l2(qp, xp), D)
        print(f"D={D} {name}: max |sigma - ||q||^2 + d| / E_q = {r.max():.5f}, max |sigma| = {np.abs(sigma).max():.3e}")
        assert r.max() <= 1.0
        worst = max(worst, float(r.max()))
    print(f"D={D}: largest screen-error ratio {worst:.5f}")


@pytest.mark.gpu
def test_l2_f16_self_matches_are_plus_zero_and_ties_take_the_lower_id():
    import torch
    from repconc_amd import ops
    N, D, nq, k = 150000, 64, 32, 10
    x16 = _randn((N, D), 31).half()
    g = torch.Generator(device="cuda:0")
    g.manual_seed(32)
    perm = torch.randperm(N, generator=g, device="cuda:0")
    src, dst = perm[: N // 20], perm[N // 20: 2 * (N // 20)]   # 5 % of the rows are copies of other rows, each copied once
    x16[dst] = x16[src].clone()
    q = x16[dst[:nq]].float()                                 # every query equals a row that has a duplicate
    want = oracle_topk_l2(x16.float(), q, k)
    got = ops.dense_search_l2_f16(x16, q, k)
    assert_matches(got, want)
    d, i = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.all(d[:, :2].view(np.uint32) == 0)             # the two zero distances are +0.0f
    assert np.all(i[:, 0] < i[:, 1]) and np.all(d[:, 2] > 0)
    assert_matches(ops.dense_search_l2_f16(x16, q, k, method="exact"), want)


@pytest.mark.gpu
def test_l2_f16_tie_group_across_the_kth_distance_falls_back_to_the_exact_route():
    """20 000 identical rows whose distance sits inside every query's top-100: the group overflows the candidate list
    whatever the slack, the exact route answers."""
    from repconc_amd import ops
    N, D, nq, k = 150000, 64, 4, 100
    x16 = _randn((N, D), 35).half()
    q = (0.05 * _randn((nq, D), 36)).half().float()
    v = _randn((D,), 37)
    x16[90000:110000] = (v * (32.0 ** 0.5 / v.norm())).half()[None]      # |v|^2 = 32: a few dozen of the gaussian rows are nearer
    want = oracle_topk_l2(x16.float(), q, k)
    tied = (want[1] >= 90000) & (want[1] < 110000)
    assert tied.any(1).all() and (~tied).any(1).all()        # the tie group straddles the k-th distance of every query
    pending = ops.dense_search_l2_f16(x16, q, k, defer=True)
    assert_matches(pending.result(), want)
    assert pending.stats["exact_queries"] > 0
    assert_matches(ops.dense_search_l2_f16(x16, q, k, method="exact"), want)


@pytest.mark.gpu
def test_l2_f16_certificate_refuses_distances_closer_than_the_screen_error():
    """Every row and query is one fp16 vector of norm ~30 moved by at most one fp16 ulp per coordinate: all distances are far
    below E_q, no answer of the fast route can be certified, every query ends on the exact route with the oracle's result."""
    import torch
    from repconc_amd import ops
    N, D, nq, k = 200000, 64, 8, 10
    base = _randn((D,), 81)
    base = (base * (30.0 / base.norm())).half()

    def near(n, seed):                                        # base + {-1, 0, 1} fp16 ulps per coordinate
        g = torch.Generator(device="cuda:0")
        g.manual_seed(seed)
        step = torch.randint(-1, 2, (n, D), generator=g, device="cuda:0")
        bits = base.view(torch.int16)[None].to(torch.int32) + step          # sign-magnitude: +-1 is one ulp either way
        return bits.to(torch.int16).view(torch.float16)

    x16, q = near(N, 82), near(nq, 83).float()
    assert bool(torch.isfinite(x16).all()) and float((x16.float() - base.float()[None]).abs().max()) <= 2.0 ** -6
    want = oracle_topk_l2(x16.float(), q, k)
    eq = ops.dense_l2_f16_error_bound(D, 30.0, 30.0)
    assert float(want[0].max()) < 0.1 * eq
    pending = ops.dense_search_l2_f16(x16, q, k, defer=True)
    assert bool(((pending._qstatus & 4) != 0).all())          # bit 2 on every query of the first pass
    assert_matches(pending.result(), want)
    assert pending.stats["exact_queries"] == nq


@pytest.mark.gpu
def test_l2_f16_negative_slack_forces_retries_with_unchanged_results():
    from repconc_amd import ops
    N, D, nq, k = 140001, 128, 64, 100
    x16, q = _randn((N, D), 41).half(), _randn((nq, D), 42)
    want = oracle_topk_l2(x16.float(), q.half().float(), k)
    pending = ops.dense_search_l2_f16(x16, q, k, sel_slack=-50.0, defer=True)
    got = pending.result()
    assert pending.stats["retried_queries"] > 0
    assert_matches(got, want)
    assert_matches(ops.dense_search_l2_f16(x16, q, k), want)


@pytest.mark.gpu
def test_l2_f16_search_corpus_above_4_gib():
    """2 100 000 x 1024 fp16 = 4.3 GB: byte offsets past 2^32 in the screen, the rescoring and the exact kernel; the nearest
    rows of queries 0 and 1 are the last two."""
    import torch
    from repconc_amd import ops
    N, D, nq, k = 2100000, 1024, 3, 10
    x16 = torch.empty((N, D), dtype=torch.float16, device="cuda:0")
    for r0 in range(0, N, 1 << 19):
        x16[r0:r0 + (1 << 19)] = _randn((min(1 << 19, N - r0), D), 51 + r0)
    assert x16.numel() * x16.element_size() > 1 << 32
    q = _randn((nq, D), 52).half().float()
    x16[N - 1] = (q[0] + 2.0 ** -6).half()
    x16[N - 2] = (q[1] + 2.0 ** -6).half()
    want = oracle_topk_l2(x16, q, k, qblock=16, rblock=1 << 19)       # the oracle widens block by block
    assert want[1][0, 0] == N - 1 and want[1][1, 0] == N - 2
    pending = ops.dense_search_l2_f16(x16, q, k, defer=True)
    assert_matches(pending.result(), want)
    assert pending.stats["exact_queries"] == 0
    assert_matches(ops.dense_search_l2_f16(x16, q[:2], k, method="exact"), (want[0][:2], want[1][:2]))
    del x16


@pytest.mark.gpu
def test_flat_l2_f16_index_add_grow_reset_search_and_batching():
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatL2F16Index
    N, D, nq, k = 3000, 100, 50, 20
    xb = _randn((N, D), 61).cpu().numpy()
    qb = _randn((nq, D), 62).cpu().numpy()
    x16 = torch.from_numpy(xb).cuda().half()
    one = FlatL2F16Index(D)
    assert one.is_trained and one.metric_type == 1 and one.d == D and one.device.type == "cuda"
    s0, i0 = one.search(qb[:3], 5)                                   # the empty index
    assert np.all(i0 == -1) and np.all(np.isposinf(s0))
    one.add(xb)
    assert one.ntotal == N and one._x.shape[0] == N and one._xsq.shape[0] == N      # the first add allocates exactly
    assert one._x.dtype == torch.float16 and torch.equal(one.xb, x16)
    three = FlatL2F16Index(D, device="cuda")
    three.add(xb[:1000])
    three.add(torch.from_numpy(xb[1000:1100]).cuda())
    assert three._x.shape[0] == 1500 and three._xsq.shape[0] == 1500                # growth 1.5x, the norms with it
    three.add(xb[1100:])
    assert three.ntotal == N and tuple(three.xb.shape) == (N, D)
    whole = ops.dense_row_sqnorms(x16)                                              # of the rounded rows
    for ix in (one, three):
        assert torch.equal(ix._xsq[:N].view(torch.int32), whole.view(torch.int32))
        assert float(ix._xnorm_max) >= float(whole.max().sqrt())
    with pytest.raises(ValueError):
        one.add(np.full((1, D), 65520.0, np.float32))
    assert one.ntotal == N
    qw = torch.from_numpy(qb).cuda().half().float()
    want = oracle_topk_l2(x16.float(), qw, k)
    s1, i1 = one.search(qb, k)
    s3, i3 = three.search(qb, k)
    assert isinstance(s1, np.ndarray) and isinstance(i1, np.ndarray) and i1.dtype == np.int64
    assert_matches((s1, i1), want)
    assert_matches((s3, i3), want)
    st, it = one.search(torch.from_numpy(qb).cuda(), k)
    assert isinstance(st, torch.Tensor) and st.is_cuda and it.is_cuda
    assert_matches((st, it), want)
    fins = [one.search_async(part, k) for part in np.array_split(qb, 4)]           # several batches enqueued before any finishes
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
    assert_matches(one.search(qb[:3], 5), oracle_topk_l2(x16[:10].float(), qw[:3], 5))


@pytest.mark.gpu
def test_flat_l2_f16_index_above_the_exact_route_uses_its_cached_norms():
    """An index large enough for the fast route, added in three uneven pieces: the search reads the cached xsq / xnorm_max and
    returns what the ops call with freshly computed norms returns."""
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatL2F16Index
    N, D, nq, k = 140001, 64, 16, 10
    x, q = _randn((N, D), 91), _randn((nq, D), 92)
    index = FlatL2F16Index(D, device="cuda")
    for a, b in ((0, 50000), (50000, 50007), (50007, N)):
        index.add(x[a:b])
    x16 = x.half()
    assert torch.equal(index.xb, x16)
    assert torch.equal(index._xsq[:N].view(torch.int32), ops.dense_row_sqnorms(x16).view(torch.int32))
    want = oracle_topk_l2(x16.float(), q.half().float(), k)
    got = index.search(q, k)
    assert_matches(got, want)
    assert index.last_search.stats == {"retried_queries": 0, "exact_queries": 0}
    fresh = ops.dense_search_l2_f16(x16, q, k)
    assert torch.equal(got[0].view(torch.int32), fresh[0].view(torch.int32)) and torch.equal(got[1], fresh[1])
