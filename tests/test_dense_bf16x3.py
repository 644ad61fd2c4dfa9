"""bf16x3 matrix-core screen of the fp32 exact dense inner-product search: csrc/dense_search_bf16x3.hip,
ops.dense_search_bf16x3, FlatIPIndex(screen="bf16x3"), create_index(screen="bf16x3").

The contract: the corpus stays fp32 and nothing is rounded in the result — ids and score bits equal `ops.dense_search` (and the
oracle of test_dense_flat.py) on the same arrays.  The bf16 matrix cores only screen, with s~ = sum_d (q_h x_h + q_h x_l + q_l x_h)
of the round-to-nearest-even splits a_h = bf16(a), a_l = bf16(a - a_h); their error against the chain must stay inside the
bound the search's certificate uses (ops.dense_bf16x3_error_bound),
    E = (8 D_pad 2^-24 + 4 * 2^-16) ||q|| X + 2^-133 sqrt(D_pad) (||q|| + X) + 4 D_pad 2^-149."""
import numpy as np
import pytest

from test_dense_flat import SHAPES, _randn, assert_matches, chain_scores, oracle_topk
from test_dense_f16 import _add32


# --------------------------------------------------------------------------------------------------------------- CPU
def test_screen_argument_and_bf16_range_are_validated_without_a_gpu():
    import torch
    from repconc_amd.dense_index import FlatIPIndex
    with pytest.raises(ValueError):
        FlatIPIndex(16, screen="fp8")                            # raised before any device is looked at
    with pytest.raises(ValueError):
        FlatIPIndex(16, storage="float16", screen="bf16x3")
    with pytest.raises(ValueError):
        FlatIPIndex(16, device="cpu", storage="float16", screen="bf16x3")
    plain = FlatIPIndex(16, device="cpu")
    assert plain.screen == "fp32" and plain.storage == "float32"
    index = FlatIPIndex(16, device="cpu", screen="bf16x3")
    assert index.screen == "bf16x3" and index.storage == "float32" and index._x.dtype == torch.float32
    with pytest.raises(ValueError):
        index.add(np.zeros((3, 8), dtype=np.float32))            # wrong width, as the default index
    ok = np.full((4, 16), 2.0, dtype=np.float32)
    ok[1, 3] = 3.38e38                                           # rounds to a finite bf16 (the largest is 3.3895e38)
    index.add(ok)
    assert index.ntotal == 4 and index._x.dtype == torch.float32 and float(index.xb.max()) == np.float32(3.38e38)
    norm = float(index._xnorm_max)
    assert norm >= 3.38e38 or np.isinf(norm)                     # >= the largest row norm, as an fp32
    for bad in (3.4e38, -3.4e38, float("inf"), float("-inf"), float("nan")):
        x = np.zeros((2, 16), dtype=np.float32)
        x[1, 5] = bad
        with pytest.raises(ValueError):
            index.add(x)
        assert index.ntotal == 4 and index._x.shape[0] == 4      # nothing stored, nothing grown
    index.reset()
    assert index.ntotal == 0 and index._x.dtype == torch.float32 and index._xnorm_max is None
    index.add(np.ones((2, 16), dtype=np.float32))
    assert 4.0 <= float(index._xnorm_max) < 4.0 * 1.001


def test_bf16x3_entry_points_reject_bad_arguments_without_a_gpu():
    import torch
    from repconc_amd import _lib, ops
    lib = _lib.load()
    N, D = 8841823, 768
    prev = 0
    for nq in (1, 7, 128, 1200, 2048):
        ws = lib.rc_dense_bf16x3_search_ws_bytes(N, D, nq, 1000)
        assert ws > prev
        assert ws >= lib.rc_dense_search_ws_bytes(N, D, nq, 1000) + nq * D * 4        # the two bf16 planes of the queries
        prev = ws
    assert lib.rc_dense_bf16x3_search_ws_bytes(N, D, 1200, 1000) >= 1200 * (32768 * 4 + 16384 * 8)
    assert lib.rc_dense_bf16x3_search_ws_bytes(1000, D, 1200, 10) == lib.rc_dense_search_exact_ws_bytes(1000, D, 1200, 10)
    for args in ((N, D, 1200, 8193), (1 << 32, D, 4, 10), (0, D, 4, 10), (N, 0, 4, 10), (N, D, 0, 10), (N, D, 4, 0)):
        assert lib.rc_dense_bf16x3_search_ws_bytes(*args) == 0
    assert lib.rc_dense_bf16x3_scores_ws_bytes(100, 8) >= 2 * 8 * 128 * 2 and lib.rc_dense_bf16x3_scores_ws_bytes(0, 8) == 0
    RC_ESHAPE, RC_EINVAL = -2, -1
    z = None
    assert lib.rc_dense_bf16x3_search_q(z, z, D, N, D, z, 4, z, 8193, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_bf16x3_search_q(z, z, D, 1 << 32, D, z, 4, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_bf16x3_search_q(z, z, D, N, D, z, 4, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_EINVAL
    assert lib.rc_dense_bf16x3_scores(z, z, D, 1 << 32, D, z, 4, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_bf16x3_scores(z, z, D, N, D, z, 4, z, z, 0, z) == RC_EINVAL
    x, q = torch.zeros(10, 16), torch.zeros(2, 16)
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_search_bf16x3(x, q, 1)
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_bf16x3_scores(x, q)
    with pytest.raises(ValueError):
        ops.dense_search_bf16x3(x, q, 1, method="fast")
    # the generalised norm helper: any floating dtype, the old name unchanged
    a = torch.tensor([[3.0, 4.0], [0.5, 0.5]])
    for t in (a, a.half(), a.double(), a.bfloat16()):
        v = ops.dense_xnorm_max(t)
        assert v.dtype == torch.float32 and v.shape == (1,) and 5.0 <= float(v) < 5.0001
    assert float(ops.dense_f16_xnorm_max(a.half())) == float(ops.dense_xnorm_max(a.half()))
    with pytest.raises(ValueError):
        ops.dense_xnorm_max(torch.zeros(2, 2, dtype=torch.int32))


def _bf16_rne(a):
    """fp32 -> the nearest bf16 (ties to even) as an fp32 array, by bit arithmetic; finite inputs below the bf16 overflow."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32)


def _split(a):
    """a = h + l + r: h = bf16(a), l = bf16(a - h); asserts that the fp32 subtraction is exact."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    h = _bf16_rne(a)
    d = a - h
    assert np.array_equal(d.astype(np.float64), a.astype(np.float64) - h.astype(np.float64))
    return h, _bf16_rne(d)


def _screen_terms(q, x):
    """The 3 D products of the screen, [P, 3 D] fp32; asserts that each is exact in fp32."""
    qh, ql = _split(q)
    xh, xl = _split(x)
    terms = []
    for a, b in ((qh, xh), (qh, xl), (ql, xh)):
        p64 = a.astype(np.float64) * b.astype(np.float64)
        p = p64.astype(np.float32)
        assert np.array_equal(p.astype(np.float64), p64)
        terms.append(p)
    return np.concatenate(terms, axis=1)


def _accumulate(terms, rng, g, pairwise, truncate):
    """One fp32 accumulation of terms [P, T] in a random order: groups of g terms summed pairwise or sequentially (all groups at
    once), the group sums added to one accumulator in sequence — what a matrix instruction of depth g does."""
    P, T = terms.shape
    t = terms[:, rng.permutation(T)]
    pad = (-T) % g
    if pad:
        t = np.concatenate([t, np.zeros((P, pad), dtype=np.float32)], axis=1)          # adding +0 is exact in both roundings
    t = t.reshape(P, -1, g)
    ng = t.shape[1]
    if pairwise:
        while t.shape[2] > 1:
            t = _add32(t[:, :, 0::2].reshape(-1), t[:, :, 1::2].reshape(-1), truncate).reshape(P, ng, -1)
        grp = t[:, :, 0]
    else:
        grp = t[:, :, 0]
        for e in range(1, g):
            grp = _add32(grp.reshape(-1), t[:, :, e].reshape(-1), truncate).reshape(P, ng)
    acc = np.zeros(P, dtype=np.float32)
    for i in range(ng):
        acc = _add32(acc, np.ascontiguousarray(grp[:, i]), truncate)
    return acc


def _cancelling(rng, rows, D):
    """fp32 rows whose every coordinate has a partner of the opposite sign one fp32 ulp apart, somewhere else in the row."""
    h = (D + 1) // 2
    m = (rng.standard_normal((rows, h)) * 2.0 ** rng.integers(-8, 8, (rows, h))).astype(np.float32)
    up = np.nextafter(m, np.float32(np.inf) * np.sign(m)).astype(np.float32)
    x = np.empty((rows, 2 * h), dtype=np.float32)
    x[:, 0::2], x[:, 1::2] = m, -up
    return x[:, :D]


def _boundary(rng, shape):
    """+-(1 + 2^-8 - 2^-23) 2^e: the mantissa just under the bf16 rounding boundary."""
    return (rng.choice([-1.0, 1.0], shape) * (1.0 + 2.0 ** -8 - 2.0 ** -23) * 2.0 ** rng.integers(-6, 7, shape)).astype(np.float32)


def _cpu_pairs(rng, P, D):
    q, x = np.empty((P, D), dtype=np.float32), np.empty((P, D), dtype=np.float32)
    for i in range(P):
        kind = i % 5
        if kind == 0:
            q[i], x[i] = rng.standard_normal(D), rng.standard_normal(D)
        elif kind == 1:
            q[i] = rng.standard_normal(D) * 2.0 ** rng.integers(-20, 21, D)
            x[i] = rng.standard_normal(D) * 2.0 ** rng.integers(-20, 21, D)
        elif kind == 2:
            q[i], x[i] = np.abs(rng.standard_normal(D)) + 0.5, np.abs(rng.standard_normal(D)) + 0.5
        elif kind == 3:
            perm = rng.permutation(D)
            x[i] = _cancelling(rng, 1, D)[0][perm]
            q[i] = np.repeat(rng.standard_normal((D + 1) // 2) * 2.0 ** rng.integers(-4, 4, (D + 1) // 2), 2)[:D][perm]
        else:
            q[i], x[i] = _boundary(rng, D), _boundary(rng, D)
    return q, x


def test_error_bound_reads_the_constants_the_certificate_kernel_was_compiled_with():
    import ctypes
    from repconc_amd import _lib, ops
    c = (ctypes.c_double * 4)()
    _lib.load().rc_dense_bf16x3_error_constants(c)
    assert tuple(c) == (8.0, 4.0, 2.0 ** -133, 4 * 2.0 ** -149)
    assert ops.dense_bf16x3_error_constants() == tuple(c)
    rel = lambda dpad: 8 * dpad * 2.0 ** -24 + 4 * 2.0 ** -16
    assert ops.dense_bf16x3_error_bound(768, 2.0, 3.0) == rel(768) * 2.0 * 3.0 + 2.0 ** -133 * 768 ** 0.5 * 5.0 + 4 * 2.0 ** -149 * 768
    assert ops.dense_bf16x3_error_bound(100, 1.0, 1.0) == rel(112) + 2.0 ** -133 * 112 ** 0.5 * 2.0 + 4 * 2.0 ** -149 * 112
    assert ops.dense_bf16x3_error_bound(16, 0.0, 0.0) == 64 * 2.0 ** -149


@pytest.mark.parametrize("D", [16, 100, 768, 4096])
def test_error_bound_covers_any_fp32_accumulation_of_the_split_products(D):
    from repconc_amd import ops
    rng = np.random.default_rng(8000 + D)
    P = 40
    q, x = _cpu_pairs(rng, P, D)
    terms = _screen_terms(q, x)
    assert terms.shape == (P, 3 * D)
    chain = chain_scores(q, x).astype(np.float64)
    q64, x64 = q.astype(np.float64), x.astype(np.float64)
    E = ops.dense_bf16x3_error_bound(D, np.sqrt((q64 ** 2).sum(1)), np.sqrt((x64 ** 2).sum(1)))
    assert E.shape == (P,) and np.all(E > 0)
    # the part of the products the split drops, alone
    drop = np.abs(terms.astype(np.float64).sum(1) - (q64 * x64).sum(1)) / (np.abs(q64 * x64).sum(1) * 2.0 ** -16)
    worst = 0.0
    depths = [1, 2, 4, 8, 16, 32, 64]
    for trial in range(28):
        got = _accumulate(terms, rng, depths[trial % 7], pairwise=bool((trial // 7) % 2), truncate=bool(trial % 2)).astype(np.float64)
        ratio = np.abs(got - chain) / E
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0), (D, trial, float(ratio.max()))
    print(f"D={D}: largest |acc - chain| / E over 28 accumulations = {worst:.4f}; dropped part <= {drop.max():.3f} * 2^-16 sum|q x|")


# --------------------------------------------------------------------------------------------------------------- GPU
# SHAPES has no sampled-route case with D % 4 != 0: (300007, 101, 7, 10) puts the screen on its element-by-element loader and
# the rescoring on its unaligned instantiation (rows of 101 floats); the D % 8 == 0 shapes run the 16-byte ones
@pytest.mark.gpu
@pytest.mark.parametrize("N,D,nq,k", SHAPES + [(300007, 101, 7, 10)])
def test_bf16x3_search_ids_and_score_bits_equal_the_oracle_and_the_fp32_search(N, D, nq, k):
    """(a) parity with the oracle and with `ops.dense_search` on the same fp32 arrays, both routes; above 131 072 rows the fast
    route answers every query: nothing repeated, nothing sent to the exact route."""
    from repconc_amd import ops
    x = _randn((N, D), 1000 + N + D)
    q = _randn((nq, D), 2000 + nq + D)
    want = oracle_topk(x, q, k)
    ref = ops.dense_search(x, q, k, id_offset=7)
    assert_matches(ref, want, id_offset=7)
    for method in ("auto", "exact"):
        pending = ops.dense_search_bf16x3(x, q, k, id_offset=7, method=method, defer=True)
        got = pending.result()
        assert got[0].shape == (nq, k) and got[0].dtype.is_floating_point and not got[1].dtype.is_floating_point
        assert_matches(got, want, id_offset=7)
        assert bool((got[1] == ref[1]).all())
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), ref[0].cpu().numpy().view(np.uint32))
        if method == "auto" and N > 131072:
            assert pending.stats == {"retried_queries": 0, "exact_queries": 0}, pending.stats


@pytest.mark.gpu
def test_bf16x3_search_row_pitch_wider_than_d():
    """Rows of 100 floats at a pitch of 104 (a column slice of a wider matrix, as the C ABI allows): 16-byte aligned rows with
    D % 8 != 0 — the screen's element-by-element loader with the rescoring's 16-byte loads and scalar tail."""
    from repconc_amd import ops
    N, D, nq, k = 200003, 100, 5, 10
    wide = _randn((N, 104), 81)
    x = wide[:, :D]
    q = _randn((nq, D), 82)
    assert x.stride(0) == 104 and x.data_ptr() % 16 == 0
    want = oracle_topk(x.contiguous(), q, k)
    pending = ops.dense_search_bf16x3(x, q, k, defer=True)
    assert_matches(pending.result(), want)
    assert pending.stats == {"retried_queries": 0, "exact_queries": 0}, pending.stats


@pytest.mark.gpu
def test_bf16x3_search_ties_take_the_lower_id_and_fall_back_to_the_exact_route():
    """(b) the tie construction of test_dense_flat.py: 5 % duplicated rows and 20 000 identical rows inside every query's
    top-100."""
    import torch
    from repconc_amd import ops
    N, D, nq, k = 200000, 384, 16, 100
    x = _randn((N, D), 31)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(32)
    src = torch.randint(0, N, (N // 20,), generator=g, device="cuda:0")
    dst = torch.randint(0, N, (N // 20,), generator=g, device="cuda:0")
    x[dst] = x[src].clone()
    u = _randn((D,), 33)
    u /= u.norm()
    noise = _randn((nq, D), 34)
    noise -= (noise @ u)[:, None] * u[None]
    q = 20.0 * u[None] + noise
    qn = float(q.norm(dim=1).mean())
    x[90000:110000] = (3.48 * qn / 20.0) * u[None]
    want = oracle_topk(x, q, k)
    tied = (want[1] >= 90000) & (want[1] < 110000)
    assert tied.any(1).all() and (~tied).any(1).all()
    pending = ops.dense_search_bf16x3(x, q, k, defer=True)
    got = pending.result()
    assert_matches(got, want)
    assert pending.stats["exact_queries"] > 0
    assert_matches(ops.dense_search_bf16x3(x, q, k, method="exact"), want)


@pytest.mark.gpu
def test_bf16x3_certificate_refuses_scores_closer_than_the_screen_error():
    """(c) 20 000 rows that differ from a base row by one fp32 ulp in one coordinate straddle the k-th score: their exact scores
    lie within a few 1e-6 of each other, far less than E_q ~ 0.15, so no threshold inside the group can be certified — bit 2 on
    the first pass for every query — and the answer still equals the oracle."""
    import torch
    from repconc_amd import ops
    N, D, nq, k = 200000, 384, 8, 100
    x = _randn((N, D), 71)
    u = _randn((D,), 73)
    u /= u.norm()
    noise = _randn((nq, D), 74)
    noise -= (noise @ u)[:, None] * u[None]
    q = 20.0 * u[None] + noise
    qn = float(q.norm(dim=1).mean())
    base = (3.48 * qn / 20.0) * u
    group = base[None].repeat(20000, 1)
    bits = group.view(torch.int32)
    rows = torch.arange(20000, device="cuda:0")
    bits[rows, rows % D] += 1                                    # the next fp32 away from zero in coordinate i % D
    assert bool(torch.isfinite(group).all()) and int((group != base[None]).sum()) == 20000
    x[90000:110000] = group
    want = oracle_topk(x, q, k)
    tied = (want[1] >= 90000) & (want[1] < 110000)
    assert tied.any(1).all() and (~tied).any(1).all()            # the group straddles the k-th score of every query
    sc = q.double() @ x[90000:110000].double().T
    E = ops.dense_bf16x3_error_bound(D, q.double().norm(dim=1), float(x.double().norm(dim=1).max()))
    assert bool(((sc.max(1).values - sc.min(1).values) < 0.2 * E).all())
    pending = ops.dense_search_bf16x3(x, q, k, defer=True)
    first = pending._qstatus.clone()
    assert bool(((first & 4) != 0).all()), first.tolist()
    got = pending.result()
    assert_matches(got, want)
    assert pending.stats["retried_queries"] > 0 or pending.stats["exact_queries"] > 0


def _screen_families(D):
    """(name, q [8, D], x [32, D]) fp32 numpy: the inputs that could break the split or an fp32 accumulation of its products."""
    rng = np.random.default_rng(9500 + D)
    sign = lambda *s: rng.choice([-1.0, 1.0], s)
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32)
    sub = lambda *s: f32(rng.integers(-(1 << 23) + 1, 1 << 23, s) * 2.0 ** -149)           # every fp32 subnormal magnitude
    low = lambda *s: f32(sign(*s) * (1.0 + rng.random(s)) * 2.0 ** rng.integers(-124, -116, s))      # a_l is a bf16 subnormal
    fams = [("x subnormal", f32(rng.standard_normal((8, D))), sub(32, D)),
            ("q subnormal", sub(8, D), f32(rng.standard_normal((32, D)))),
            ("both subnormal", sub(8, D), sub(32, D)),
            ("x in 2^-124..2^-116", f32(rng.standard_normal((8, D))), low(32, D)),
            ("q in 2^-124..2^-116", low(8, D), f32(rng.standard_normal((32, D))))]
    perm = rng.permutation(D)
    qc = np.repeat(rng.standard_normal((8, (D + 1) // 2)) * 2.0 ** rng.integers(-4, 4, (8, (D + 1) // 2)), 2, axis=1)[:, :D]
    fams.append(("cancelling pairs", f32(qc[:, perm]), _cancelling(rng, 32, D)[:, perm]))
    qh, xh = 1e-15 * sign(8, D), 1e-15 * sign(32, D)
    for r in range(8):
        qh[r, rng.choice(D, 3, replace=False)] = 1e15 * sign(3)
    for r in range(32):
        xh[r, rng.choice(D, 3, replace=False)] = 1e15 * sign(3)
    fams.append(("1e15 among 1e-15", f32(qh), f32(xh)))
    fams.append(("all magnitudes", f32(rng.standard_normal((8, D)) * 2.0 ** rng.integers(-60, 41, (8, D))),
                 f32(rng.standard_normal((32, D)) * 2.0 ** rng.integers(-60, 41, (32, D)))))
    fams.append(("boundary mantissas", _boundary(rng, (8, D)), _boundary(rng, (32, D))))
    return fams


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 100, 768, 1024])
def test_bf16x3_screen_error_stays_inside_the_certificate_bound(D):
    """(d) |s~ - s_chain| <= E_q for every pair, E_q from the query's norm and the largest row norm of the family it is run
    against (one call per family, so a family of small rows is held to its own small bound).  The subnormal families decide
    whether the conversion or the matrix instruction flushes: a flushed operand would put the error far above the bound's
    absolute part.  Prints the largest ratio per family: the figures DESIGN.md section 4.9 quotes."""
    import torch
    from repconc_amd import ops
    worst, lines = 0.0, []
    for name, qf, xf in _screen_families(D):
        approx = ops.dense_bf16x3_scores(torch.from_numpy(xf).cuda(), torch.from_numpy(qf).cuda()).cpu().numpy().astype(np.float64)
        chain = chain_scores(np.repeat(qf, 32, axis=0), np.tile(xf, (8, 1))).reshape(8, 32).astype(np.float64)
        qn = np.sqrt((qf.astype(np.float64) ** 2).sum(1))
        xn = np.sqrt((xf.astype(np.float64) ** 2).sum(1))
        E = ops.dense_bf16x3_error_bound(D, qn, float(xn.max()))[:, None]
        err = np.abs(approx - chain)
        assert np.all(np.isfinite(approx))
        ratio = float((err / E).max())
        lines.append(f"D={D} {name}: max |s~ - s| / E_q = {ratio:.5f}, max |s| = {np.abs(chain).max():.3e}, "
                     f"max err = {err.max():.3e}, min E_q = {E.min():.3e}, zero s~ = {int((approx == 0).sum())}/256")
        worst = max(worst, ratio)
    print("\n".join(lines))
    print(f"D={D}: largest screen-error ratio {worst:.5f}")
    assert worst <= 1.0, lines


@pytest.mark.gpu
def test_bf16x3_index_add_reserve_reset_search_and_batching():
    """(e) the screened index keeps fp32 and the kept norm through add / reserve / growth / reset; numpy and tensor inputs agree
    bit for bit; create_index(screen="bf16x3") with batch_dense_search equals the per-batch loop and the default index; a
    negative slack forces retries."""
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatIPIndex
    from repconc_amd.models.dense.evaluate_dense import batch_dense_search, create_index, dense_search
    N, D, nq, k = 3000, 384, 50, 20
    xb = _randn((N, D), 61).cpu().numpy()
    qb = _randn((nq, D), 62).cpu().numpy()
    with pytest.raises(ValueError):
        create_index(xb, screen="fp8")
    with pytest.raises(ValueError):
        create_index(xb, use_float16=True, screen="bf16x3")
    one = create_index(xb, screen="bf16x3")
    default = create_index(xb)
    assert default.screen == "fp32" and default._xnorm_max is None
    assert one.screen == "bf16x3" and one.storage == "float32" and one.ntotal == N and one._x.shape[0] == N
    assert one._x.dtype == torch.float32 and bool((one.xb == torch.from_numpy(xb).cuda()).all())
    three = FlatIPIndex(D, device="cuda", screen="bf16x3")
    three.add(xb[:1000])
    three.add(torch.from_numpy(xb[1000:1100]).cuda())
    assert three._x.shape[0] == 1500 and three._x.dtype == torch.float32       # growth 1.5x
    three.add(xb[1100:])
    assert three.ntotal == N and bool((three.xb == one.xb).all())
    assert float(three._xnorm_max) == float(one._xnorm_max) >= float(one.xb.double().norm(dim=1).max())
    s1, i1 = one.search(qb, k)
    s3, i3 = three.search(qb, k)
    sd, idd = default.search(qb, k)
    assert isinstance(s1, np.ndarray) and i1.dtype == np.int64 and s1.dtype == np.float32
    assert np.array_equal(i1, i3) and np.array_equal(s1.view(np.uint32), s3.view(np.uint32))
    assert np.array_equal(i1, idd) and np.array_equal(s1.view(np.uint32), sd.view(np.uint32))
    st, it = one.search(torch.from_numpy(qb).cuda(), k)
    assert isinstance(st, torch.Tensor) and st.is_cuda and it.is_cuda
    assert np.array_equal(it.cpu().numpy(), i1) and np.array_equal(st.cpu().numpy().view(np.uint32), s1.view(np.uint32))
    assert_matches((s1, i1), oracle_topk(torch.from_numpy(xb).cuda(), torch.from_numpy(qb).cuda(), k))
    corpus_ids = np.array([f"d{i}" for i in range(N)])
    qids = np.arange(nq)
    bs, bi = batch_dense_search(qids, qb, corpus_ids, one, k, batch_size=16)
    loop = [dense_search(a, b, corpus_ids, one, k) for a, b in zip(np.array_split(qids, 4), np.array_split(qb, 4))]
    assert np.array_equal(bi, np.concatenate([g[1] for g in loop])) and np.array_equal(bi, corpus_ids[i1])
    assert np.array_equal(bs.view(np.uint32), np.concatenate([g[0] for g in loop]).view(np.uint32))
    ds, di = batch_dense_search(qids, qb, corpus_ids, default, k, batch_size=16)
    assert np.array_equal(bi, di) and np.array_equal(bs.view(np.uint32), ds.view(np.uint32))
    kept = float(one._xnorm_max)
    one.reserve(5000)
    assert one._x.shape[0] == 5000 and one._x.dtype == torch.float32 and float(one._xnorm_max) == kept
    assert np.array_equal(one.search(qb, k)[1], i1)
    with pytest.raises(ValueError):
        one.add(np.full((1, D), 3.4e38, dtype=np.float32))
    assert one.ntotal == N
    one.reset()
    assert one.ntotal == 0 and one._x.dtype == torch.float32 and one._xnorm_max is None
    s0, i0 = one.search(qb[:3], 5)
    assert np.all(i0 == -1) and np.all(np.isneginf(s0))
    one.add(xb[:10])
    assert np.array_equal(one.search(qb[:3], 5)[1], oracle_topk(torch.from_numpy(xb[:10]).cuda(), torch.from_numpy(qb[:3]).cuda(), 5)[1])
    # the sampled-threshold route of the index, and a negative slack: retries, unchanged results
    N2, D2, nq2, k2 = 200000, 768, 64, 100
    x2, q2 = _randn((N2, D2), 41), _randn((nq2, D2), 42)
    want = oracle_topk(x2, q2, k2)
    big = FlatIPIndex(D2, screen="bf16x3")
    big.add(x2[:120000])
    big.add(x2[120000:])
    assert float(big._xnorm_max) >= float(x2.double().norm(dim=1).max())
    del x2
    assert_matches(big.search(q2, k2), want)
    assert big.last_search.stats == {"retried_queries": 0, "exact_queries": 0}
    big.sel_slack = -0.5
    got = big.search(q2, k2)
    assert big.last_search.stats["retried_queries"] > 0
    assert_matches(got, want)
    pending = ops.dense_search_bf16x3(big.xb, q2, k2, sel_slack=-0.5, defer=True, xnorm_max=big._xnorm_max)
    assert_matches(pending.result(), want)
    assert pending.stats["retried_queries"] > 0
    # a query value that rounds to a bf16 inf: no certificate, the exact route's answer
    q3 = q2[:4].clone()
    q3[1, 5] = 3.4e38
    pending = ops.dense_search_bf16x3(big.xb, q3, k2, defer=True, xnorm_max=big._xnorm_max)
    first = pending._qstatus.clone()
    assert bool(first[1] & 4) and not bool(first[0]) and not bool(first[2:].any())
    got = pending.result()
    ref = ops.dense_search_exact(big.xb, q3, k2)
    assert np.array_equal(got[1].cpu().numpy(), ref[1].cpu().numpy())
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), ref[0].cpu().numpy().view(np.uint32))


@pytest.mark.gpu
def test_bf16x3_search_corpus_above_4_gib():
    """(f) 1 500 000 x 768 fp32 = 4.6 GB: byte offsets past 2^32; query 0's best row is the last one."""
    from repconc_amd import ops
    N, D, nq, k = 1500000, 768, 16, 100
    x = _randn((N, D), 51)
    q = _randn((nq, D), 52)
    x[N - 1] = 2.0 * q[0]
    x[N - 2] = 2.0 * q[1]
    assert x.numel() * x.element_size() > 4 << 30
    want = oracle_topk(x, q, k, qblock=16, rblock=1 << 19)
    assert want[1][0, 0] == N - 1 and want[1][1, 0] == N - 2
    pending = ops.dense_search_bf16x3(x, q, k, defer=True)
    assert_matches(pending.result(), want)
    assert pending.stats == {"retried_queries": 0, "exact_queries": 0}
    del x
