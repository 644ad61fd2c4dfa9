"""fp16 corpus storage of the exact dense inner-product search: csrc/dense_search_f16.hip, ops.dense_search_f16,
FlatIPIndex(storage="float16"), create_index(use_float16=True).

The contract: values and queries are rounded to IEEE fp16 (round to nearest even); a score is the fp32 fmaf chain over the
widened values, so ids and score bits equal the fp32 search (and the oracle of test_dense_flat.py) on x.half().float(),
q.half().float().  The f16 matrix cores only screen: their error against the chain must stay inside the bound the search's
certificate uses, E = 4 D_pad 2^-24 ||q|| X (ops.dense_f16_error_bound)."""
import numpy as np
import pytest

from test_dense_flat import SHAPES, _randn, assert_matches, chain_scores, oracle_topk


# --------------------------------------------------------------------------------------------------------------- CPU
def test_storage_argument_and_float16_range_are_validated_without_a_gpu():
    import torch
    from repconc_amd.dense_index import FlatIPIndex
    with pytest.raises(ValueError):
        FlatIPIndex(16, device="cpu", storage="bfloat16")
    with pytest.raises(ValueError):
        FlatIPIndex(16, storage="float64")                       # raised before any device is looked at
    assert FlatIPIndex(16, device="cpu").storage == "float32" and FlatIPIndex(16, device="cpu")._x.dtype == torch.float32
    index = FlatIPIndex(16, device="cpu", storage="float16")
    assert index._x.dtype == torch.float16 and index.xb.dtype == torch.float16 and index._x.element_size() == 2
    with pytest.raises(ValueError):
        index.add(np.zeros((3, 8), dtype=np.float32))            # wrong width, as the fp32 index
    ok = np.full((4, 16), 65504.0, dtype=np.float32)
    ok[1, 3] = 65519.0                                           # still rounds to 65504
    index.add(ok)
    assert index.ntotal == 4 and float(index.xb.float().max()) == 65504.0
    norm = float(index._xnorm_max)
    assert norm >= 65504.0 * 4.0 and norm < 65504.0 * 4.0 * 1.001
    for bad in (65520.0, -65520.0, 1e9, float("inf"), float("nan")):
        x = np.zeros((2, 16), dtype=np.float32)
        x[1, 5] = bad
        with pytest.raises(ValueError):
            index.add(x)
        assert index.ntotal == 4 and index._x.shape[0] == 4      # nothing stored, nothing grown
    index.reset()
    assert index.ntotal == 0 and index._x.dtype == torch.float16 and index._xnorm_max is None


def test_f16_entry_points_reject_bad_arguments_without_a_gpu():
    import torch
    from repconc_amd import _lib, ops
    lib = _lib.load()
    N, D = 8841823, 768
    prev = 0
    for nq in (1, 7, 128, 1200, 2048):
        ws = lib.rc_dense_f16_search_ws_bytes(N, D, nq, 1000)
        ex = lib.rc_dense_f16_search_exact_ws_bytes(N, D, nq, 1000)
        assert ws > prev and ex > 0
        prev = ws
    assert lib.rc_dense_f16_search_ws_bytes(N, D, 1200, 1000) >= 1200 * (32768 * 4 + 16384 * 8)
    assert lib.rc_dense_f16_search_ws_bytes(1000, D, 1200, 10) == lib.rc_dense_f16_search_exact_ws_bytes(1000, D, 1200, 10)
    exs = [lib.rc_dense_f16_search_exact_ws_bytes(300007, D, nq, 100) for nq in (1, 2, 50, 200, 1200)]
    assert exs == sorted(exs) and exs[0] < exs[-1]
    for args in ((N, D, 1200, 8193), (1 << 32, D, 4, 10), (0, D, 4, 10), (N, 0, 4, 10), (N, D, 0, 10), (N, D, 4, 0)):
        assert lib.rc_dense_f16_search_ws_bytes(*args) == 0 and lib.rc_dense_f16_search_exact_ws_bytes(*args) == 0
    RC_ESHAPE, RC_EINVAL = -2, -1
    z = None
    assert lib.rc_dense_f16_search_q(z, z, D, N, D, z, 4, z, 8193, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_f16_search_q(z, z, D, 1 << 32, D, z, 4, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_f16_search_exact(z, z, D, N, D, z, 4, 8193, 0, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_f16_search_q(z, z, D, N, D, z, 4, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_EINVAL
    assert lib.rc_dense_f16_scores(z, z, D, 1 << 32, D, z, 4, z, z) == RC_ESHAPE
    assert lib.rc_dense_f16_scores(z, z, D, N, D, z, 4, z, z) == RC_EINVAL
    x16, q = torch.zeros(10, 16, dtype=torch.float16), torch.zeros(2, 16)
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_search_f16(x16, q, 1)
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_search_f16_exact(x16, q, 1)
    with pytest.raises(ValueError):
        ops.dense_search_f16(x16, q, 1, method="fast")


def _f16(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float32)


def _add32(a, b, truncate):
    """fp32 a + b elementwise, rounded to nearest even or truncated toward zero (exact TwoSum in fp64, then one rounding)."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    s = a64 + b64
    bb = s - a64
    e = (a64 - (s - bb)) + (b64 - bb)                 # a + b = s + e exactly
    if not truncate:
        fix = (e != 0) & ((s.view(np.int64) & 1) == 0)       # round to odd, then to fp32: no double rounding
        s = s.copy()
        s[fix] = np.nextafter(s[fix], np.where(e[fix] > 0, np.inf, -np.inf))
        return s.astype(np.float32)
    r = s.astype(np.float32)
    over = (r.astype(np.float64) - s) - e             # sign of r - (a + b)
    v_pos = (s > 0) | ((s == 0) & (e > 0))
    back = ((over > 0) & v_pos) | ((over < 0) & ~v_pos)      # |r| > |a + b|: one step toward zero
    r = r.copy()
    r[back] = np.nextafter(r[back], np.float32(0))
    return r


def _accumulate(prod, rng, truncate):
    """One fp32 accumulation of the exact products prod [P, D] in a random order and grouping: groups of g products summed
    sequentially or pairwise, the group sums added to one accumulator — what a matrix instruction of depth g does."""
    P, D = prod.shape
    p = prod[:, rng.permutation(D)]
    g = int(rng.choice([1, 2, 4, 8, 16, 32, 64]))
    pairwise = bool(rng.integers(0, 2))
    acc = np.zeros(P, dtype=np.float32)
    for d0 in range(0, D, g):
        terms = [p[:, d] for d in range(d0, min(d0 + g, D))]
        if pairwise:
            while len(terms) > 1:
                nxt = [_add32(terms[i], terms[i + 1], truncate) for i in range(0, len(terms) - 1, 2)]
                if len(terms) % 2:
                    nxt.append(terms[-1])
                terms = nxt
            grp = terms[0]
        else:
            grp = terms[0]
            for t in terms[1:]:
                grp = _add32(grp, t, truncate)
        acc = _add32(acc, grp, truncate)
    return acc


def _adversarial_pairs(rng, P, D):
    """fp16-rounded (q, x) pairs [P, D]: gaussian; heavy cancellation; magnitudes from the fp16 subnormals to 6e4."""
    q, x = np.empty((P, D)), np.empty((P, D))
    for i in range(P):
        kind = i % 5
        if kind == 0:
            q[i], x[i] = rng.standard_normal(D), rng.standard_normal(D)
        elif kind == 1:                                          # every product has a partner of the opposite sign that
            m = rng.standard_normal((D + 1) // 2) * 2.0 ** rng.integers(-8, 8, (D + 1) // 2)      # differs in its last bits,
            x[i] = np.repeat(m, 2)[:D] * np.tile([1.0, -1.0], (D + 1) // 2)[:D]                    # somewhere else in the row
            x[i] *= 1.0 + 2.0 ** -10 * rng.integers(0, 2, D)
            q[i] = np.repeat(rng.standard_normal((D + 1) // 2) * 2.0 ** rng.integers(-4, 4, (D + 1) // 2), 2)[:D]
            perm = rng.permutation(D)
            q[i], x[i] = q[i][perm], x[i][perm]
        elif kind == 2:                                          # every magnitude fp16 has, sign random
            q[i] = rng.standard_normal(D) * 2.0 ** rng.integers(-24, 16, D)
            x[i] = rng.standard_normal(D) * 2.0 ** rng.integers(-24, 16, D)
        elif kind == 3:                                          # subnormals against normals
            q[i] = rng.integers(-1023, 1024, D) * 2.0 ** -24
            x[i] = rng.standard_normal(D) * (1.0 if i % 2 else 2.0 ** -20)
        else:                                                    # a few coordinates at 6e4, the rest at 1e-4
            q[i] = 1e-4 * rng.choice([-1.0, 1.0], D)
            x[i] = 1e-4 * rng.choice([-1.0, 1.0], D)
            hot = rng.choice(D, 4, replace=False)
            q[i, hot] = 6e4 * rng.choice([-1.0, 1.0], 4)
            x[i, hot] = 6e4 * rng.choice([-1.0, 1.0], 4)
    return _f16(np.clip(q, -65504, 65504)), _f16(np.clip(x, -65504, 65504))


@pytest.mark.parametrize("D", [16, 100, 768, 4096])
def test_error_bound_covers_any_fp32_accumulation_of_the_exact_products(D):
    from repconc_amd import ops
    rng = np.random.default_rng(7000 + D)
    P = 40
    q, x = _adversarial_pairs(rng, P, D)
    prod = (q.astype(np.float64) * x.astype(np.float64)).astype(np.float32)
    assert np.array_equal(prod.astype(np.float64), q.astype(np.float64) * x.astype(np.float64))     # products are exact in fp32
    chain = chain_scores(q, x).astype(np.float64)
    E = ops.dense_f16_error_bound(D, np.sqrt((q.astype(np.float64) ** 2).sum(1)), np.sqrt((x.astype(np.float64) ** 2).sum(1)))
    assert E.shape == (P,) and np.all(E > 0)
    assert ops.dense_f16_error_bound(100, 2.0, 3.0) == 4 * 112 * 2.0 ** -24 * 6.0                    # D_pad = D up to 16
    worst = 0.0
    for trial in range(24):
        got = _accumulate(prod, rng, truncate=bool(trial % 2)).astype(np.float64)
        ratio = np.abs(got - chain) / E
        worst = max(worst, float(ratio.max()))
        assert np.all(ratio <= 1.0), (D, trial, float(ratio.max()))
    print(f"D={D}: largest |acc - chain| / E over 24 accumulations = {worst:.4f}")


# --------------------------------------------------------------------------------------------------------------- GPU
def _rounded(x, q):
    return x.half().float(), q.half().float()


def test_error_bound_uses_the_constant_the_certificate_kernel_was_compiled_with():
    """The library exports the factor of E_q that dense_f16_certify_kernel uses; `dense_f16_error_bound` (what the bound test
    above and GPU test (e) hold the arithmetic to) reads that copy, so the two cannot drift apart.  The factor is 4."""
    from repconc_amd import _lib, ops
    c = _lib.load().rc_dense_f16_error_constant()
    assert c == 4.0
    assert ops.dense_f16_error_constant() == c
    assert ops.dense_f16_error_bound(768, 2.0, 3.0) == c * 768 * 2.0 ** -24 * 2.0 * 3.0
    assert ops.dense_f16_error_bound(100, 1.0, 1.0) == c * 112 * 2.0 ** -24
    assert _lib.load().rc_dense_f16_screen_form() in (16, 32)


@pytest.mark.gpu
@pytest.mark.parametrize("N,D,nq,k", SHAPES)
def test_f16_search_ids_and_score_bits_equal_the_oracle_and_the_fp32_search(N, D, nq, k):
    """(a) parity with the oracle and with the fp32 search on the rounded arrays, both routes; (b) above 131 072 rows the
    fast route answers every query: nothing repeated, nothing sent to the exact route."""
    from repconc_amd import ops
    x = _randn((N, D), 1000 + N + D) * 1.0003
    q = _randn((nq, D), 2000 + nq + D) * 1.0003
    xr, qr = _rounded(x, q)
    assert not bool((xr == x).all())                             # the rounding matters
    x16 = x.half()
    del x
    want = oracle_topk(xr, qr, k)
    ref = ops.dense_search(xr, qr, k, id_offset=7)
    assert_matches(ref, want, id_offset=7)
    for method in ("auto", "exact"):
        pending = ops.dense_search_f16(x16, q, k, id_offset=7, method=method, defer=True)
        got = pending.result()
        assert got[0].shape == (nq, k) and got[0].dtype.is_floating_point and not got[1].dtype.is_floating_point
        assert_matches(got, want, id_offset=7)
        assert bool((got[1] == ref[1]).all())
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), ref[0].cpu().numpy().view(np.uint32))
        if method == "auto" and N > 131072:
            assert pending.stats == {"retried_queries": 0, "exact_queries": 0}, pending.stats


@pytest.mark.gpu
def test_f16_search_ties_take_the_lower_id_and_fall_back_to_the_exact_route():
    """(c) the tie construction of test_dense_flat.py on rounded data: 5 % duplicated rows and 20 000 identical rows inside
    every query's top-100."""
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
    xr, qr = _rounded(x, q)
    want = oracle_topk(xr, qr, k)
    tied = (want[1] >= 90000) & (want[1] < 110000)
    assert tied.any(1).all() and (~tied).any(1).all()
    pending = ops.dense_search_f16(x.half(), q, k, defer=True)
    got = pending.result()
    assert_matches(got, want)
    assert pending.stats["exact_queries"] > 0
    assert_matches(ops.dense_search_f16(x.half(), q, k, method="exact"), want)


@pytest.mark.gpu
def test_f16_certificate_refuses_scores_closer_than_the_screen_error():
    """(d) 20 000 rows that differ in the last fp16 bit of one coordinate straddle the k-th score: their exact scores differ by
    at most ~3e-3, far less than E_q ~ 0.05, so no threshold inside the group can be certified — bit 2 on the first pass — and the
    answer still equals the oracle."""
    import torch
    from repconc_amd import ops
    N, D, nq, k = 200000, 384, 8, 100
    x16 = (_randn((N, D), 71) * 1.0003).half()
    u = _randn((D,), 73)
    u /= u.norm()
    noise = _randn((nq, D), 74)
    noise -= (noise @ u)[:, None] * u[None]
    q = 20.0 * u[None] + noise
    qn = float(q.norm(dim=1).mean())
    base = ((3.48 * qn / 20.0) * u).half()
    group = base[None].repeat(20000, 1)
    bits = group.view(torch.int16)
    rows = torch.arange(20000, device="cuda:0")
    bits[rows, rows % D] += 1                                    # the next fp16 away from zero in coordinate i % D
    assert bool(torch.isfinite(group).all()) and int((group != base[None]).sum()) == 20000
    x16[90000:110000] = group
    xr, qr = x16.float(), q.half().float()
    want = oracle_topk(xr, qr, k)
    tied = (want[1] >= 90000) & (want[1] < 110000)
    assert tied.any(1).all() and (~tied).any(1).all()            # the group straddles the k-th score of every query
    sc = (qr.double() @ xr[90000:110000].double().T)
    E = ops.dense_f16_error_bound(D, qr.double().norm(dim=1), float(xr.double().norm(dim=1).max()))
    assert bool(((sc.max(1).values - sc.min(1).values) < 0.2 * E).all())
    pending = ops.dense_search_f16(x16, q, k, defer=True)
    first = pending._qstatus.clone()
    assert bool(((first & 4) != 0).all()), first.tolist()
    got = pending.result()
    assert_matches(got, want)
    assert pending.stats["retried_queries"] > 0 or pending.stats["exact_queries"] > 0


def _screen_families(D, dev):
    """fp16 (name, q [8, D], x [32, D]) on the device: the inputs that could break an fp32 accumulation of fp16 products."""
    import torch
    rng = np.random.default_rng(9000 + D)
    sign = lambda *s: rng.choice([-1.0, 1.0], s)
    fams = []
    sub = lambda *s: rng.integers(-1023, 1024, s) * 2.0 ** -24
    fams.append(("x subnormal", rng.standard_normal((8, D)), sub(32, D)))
    fams.append(("q subnormal", sub(8, D), rng.standard_normal((32, D))))
    fams.append(("both subnormal", sub(8, D), sub(32, D)))
    h = (D + 1) // 2
    m = rng.standard_normal((32, h)) * 2.0 ** rng.integers(-8, 8, (32, h))
    xc = np.repeat(m, 2, axis=1)[:, :D] * np.tile([1.0, -1.0], h)[:D] * (1.0 + 2.0 ** -10 * rng.integers(0, 2, (32, D)))
    qc = np.repeat(rng.standard_normal((8, h)) * 2.0 ** rng.integers(-4, 4, (8, h)), 2, axis=1)[:, :D]
    perm = rng.permutation(D)                                    # partners of opposite sign, last bits apart, not adjacent
    xc, qc = xc[:, perm], qc[:, perm]
    fams.append(("cancelling pairs", qc, xc))
    qh, xh = 1e-4 * sign(8, D), 1e-4 * sign(32, D)
    for r in range(8):
        qh[r, rng.choice(D, 3, replace=False)] = 6e4 * sign(3)
    for r in range(32):
        xh[r, rng.choice(D, 3, replace=False)] = 6e4 * sign(3)
    fams.append(("6e4 among 1e-4", qh, xh))
    fams.append(("all magnitudes", rng.standard_normal((8, D)) * 2.0 ** rng.integers(-24, 16, (8, D)),
                 rng.standard_normal((32, D)) * 2.0 ** rng.integers(-24, 16, (32, D))))
    to16 = lambda a: torch.from_numpy(np.clip(a, -65504, 65504)).to(dev).half()
    return [(n, to16(a), to16(b)) for n, a, b in fams]


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 100, 768, 1024])
def test_f16_screen_error_stays_inside_the_certificate_bound(D):
    """(e) |s~ - s_chain| <= E_q for every pair, E_q from the query's norm and the largest row norm of the corpus it is run
    against (one call per family of inputs, so a family of small rows is held to its own small bound).  Prints the largest
    ratio: the figure DESIGN.md section 4.9 quotes."""
    from repconc_amd import ops
    worst, lines = 0.0, []
    for name, q16, x16 in _screen_families(D, "cuda:0"):
        approx = ops.dense_f16_scores(x16, q16).cpu().numpy().astype(np.float64)            # [8, 32]
        qf, xf = q16.float().cpu().numpy(), x16.float().cpu().numpy()
        chain = chain_scores(np.repeat(qf, 32, axis=0), np.tile(xf, (8, 1))).reshape(8, 32).astype(np.float64)
        qn = np.sqrt((qf.astype(np.float64) ** 2).sum(1))
        xn = np.sqrt((xf.astype(np.float64) ** 2).sum(1))
        E = ops.dense_f16_error_bound(D, qn, float(xn.max()))[:, None]
        err = np.abs(approx - chain)
        ratio = float((err / E).max())
        pair = float((err / np.maximum(ops.dense_f16_error_bound(D, qn[:, None], xn[None, :]), 1e-300)).max())
        lines.append(f"D={D} {name}: max |s~ - s| / E_q = {ratio:.5f} (against the pair's own norms {pair:.5f}), "
                     f"max |s| = {np.abs(chain).max():.3e}, max err = {err.max():.3e}")
        worst = max(worst, ratio)
    print("\n".join(lines))
    print(f"D={D}: largest screen-error ratio {worst:.5f}")
    assert worst <= 1.0, lines


@pytest.mark.gpu
def test_f16_index_add_reserve_reset_search_and_batching():
    """(f) the index keeps fp16 through add / reserve / growth / reset; numpy and tensor inputs agree bit for bit;
    create_index(use_float16=True) with batch_dense_search equals the per-batch loop; a negative slack forces retries."""
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatIPIndex
    from repconc_amd.models.dense.evaluate_dense import batch_dense_search, create_index, dense_search
    N, D, nq, k = 3000, 384, 50, 20
    xb = (_randn((N, D), 61) * 1.0003).cpu().numpy()
    qb = (_randn((nq, D), 62) * 1.0003).cpu().numpy()
    one = create_index(xb, use_float16=True)
    assert one.storage == "float16" and one.ntotal == N and one._x.shape[0] == N
    assert one._x.dtype == torch.float16 and one._x.element_size() == 2 and one.xb.dtype == torch.float16
    three = FlatIPIndex(D, device="cuda", storage="float16")
    three.add(xb[:1000])
    three.add(torch.from_numpy(xb[1000:1100]).cuda())
    assert three._x.shape[0] == 1500 and three._x.dtype == torch.float16       # growth 1.5x keeps the type
    three.add(xb[1100:])
    assert three.ntotal == N and bool((three.xb == one.xb).all())
    assert bool((one.xb == torch.from_numpy(xb).cuda().half()).all())
    assert float(three._xnorm_max) == float(one._xnorm_max) >= float(one.xb.double().norm(dim=1).max())
    s1, i1 = one.search(qb, k)
    s3, i3 = three.search(qb, k)
    assert isinstance(s1, np.ndarray) and i1.dtype == np.int64 and s1.dtype == np.float32
    assert np.array_equal(i1, i3) and np.array_equal(s1.view(np.uint32), s3.view(np.uint32))
    st, it = one.search(torch.from_numpy(qb).cuda(), k)
    assert isinstance(st, torch.Tensor) and st.is_cuda and it.is_cuda
    assert np.array_equal(it.cpu().numpy(), i1) and np.array_equal(st.cpu().numpy().view(np.uint32), s1.view(np.uint32))
    xr, qr = _rounded(torch.from_numpy(xb).cuda(), torch.from_numpy(qb).cuda())
    assert_matches((s1, i1), oracle_topk(xr, qr, k))
    corpus_ids = np.array([f"d{i}" for i in range(N)])
    qids = np.arange(nq)
    bs, bi = batch_dense_search(qids, qb, corpus_ids, one, k, batch_size=16)
    loop = [dense_search(a, b, corpus_ids, one, k) for a, b in zip(np.array_split(qids, 4), np.array_split(qb, 4))]
    assert np.array_equal(bi, np.concatenate([g[1] for g in loop])) and np.array_equal(bi, corpus_ids[i1])
    assert np.array_equal(bs.view(np.uint32), np.concatenate([g[0] for g in loop]).view(np.uint32))
    one.reserve(5000)
    assert one._x.shape[0] == 5000 and one._x.dtype == torch.float16 and np.array_equal(one.search(qb, k)[1], i1)
    with pytest.raises(ValueError):
        one.add(np.full((1, D), 7e4, dtype=np.float32))
    assert one.ntotal == N
    one.reset()
    assert one.ntotal == 0 and one._x.dtype == torch.float16 and one._xnorm_max is None
    s0, i0 = one.search(qb[:3], 5)
    assert np.all(i0 == -1) and np.all(np.isneginf(s0))
    one.add(xb[:10])
    assert np.array_equal(one.search(qb[:3], 5)[1], oracle_topk(xr[:10], qr[:3], 5)[1])
    # the sampled-threshold route of the index, and a negative slack: retries, unchanged results
    N2, D2, nq2, k2 = 200000, 768, 64, 100
    x2, q2 = _randn((N2, D2), 41) * 1.0003, _randn((nq2, D2), 42) * 1.0003
    want = oracle_topk(*_rounded(x2, q2), k2)
    big = FlatIPIndex(D2, storage="float16")
    big.add(x2[:120000])
    big.add(x2[120000:])
    del x2
    assert_matches(big.search(q2, k2), want)
    assert big.last_search.stats == {"retried_queries": 0, "exact_queries": 0}
    big.sel_slack = -50.0
    got = big.search(q2, k2)
    assert big.last_search.stats["retried_queries"] > 0
    assert_matches(got, want)
    pending = ops.dense_search_f16(big.xb, q2, k2, sel_slack=-50.0, defer=True, xnorm_max=big._xnorm_max)
    assert_matches(pending.result(), want)
    assert pending.stats["retried_queries"] > 0


@pytest.mark.gpu
def test_f16_search_corpus_above_4_gib():
    """(g) 3 000 000 x 768 fp16 = 4.6 GB: byte offsets past 2^32; query 0's best row is the last one."""
    from repconc_amd import ops
    N, D, nq, k = 3000000, 768, 16, 100
    x16 = _randn((N, D), 51).mul_(1.0003).half()
    q = _randn((nq, D), 52) * 1.0003
    x16[N - 1] = (2.0 * q[0]).half()
    x16[N - 2] = (2.0 * q[1]).half()
    assert x16.numel() * x16.element_size() > 4 << 30
    xr = x16.float()
    want = oracle_topk(xr, q.half().float(), k, qblock=16, rblock=1 << 19)
    del xr
    assert want[1][0, 0] == N - 1 and want[1][1, 0] == N - 2
    pending = ops.dense_search_f16(x16, q, k, defer=True)
    assert_matches(pending.result(), want)
    assert pending.stats == {"retried_queries": 0, "exact_queries": 0}
    del x16
