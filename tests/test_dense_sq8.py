"""8-bit scalar-quantised storage of the exact dense inner-product search: csrc/dense_search_sq8.hip, csrc/dense_i8_gemm.h,
ops.dense_search_sq8, dense_index.FlatSQ8Index, faiss_compat.IndexScalarQuantizer, create_index(storage="int8").

The contract: training takes the per-dimension range, step = fp32((vmax - vmin) / 255), mid = fp32(vmin + 128.5 step); a value
is stored as c - 128, c = clamp(floor((x - vmin) / step), 0, 255), and IS its decoded value fmaf(c - 128, step, mid); a score
is the fp32 fmaf chain over the decoded values, so ids and score bits equal the fp32 search (and the oracle of
test_dense_flat.py) on reconstruct_n(0, N).  The int8 matrix cores only screen: their error against the chain must stay
inside the bound the search's certificate uses (ops.dense_sq8_error_bound)."""
import numpy as np
import pytest

from test_dense_flat import SHAPES, _randn, assert_matches, chain_scores, fmaf_emul, oracle_topk

f32, f64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------- numpy restatements (CPU)
def sq8_train(x):
    vmin, vmax = x.min(0).astype(f32), x.max(0).astype(f32)
    step = ((vmax.astype(f64) - vmin.astype(f64)) / 255.0).astype(f32)
    mid = (vmin.astype(f64) + 128.5 * step.astype(f64)).astype(f32)
    return vmin, step, mid


def sq8_encode(x, vmin, step):
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.floor((x.astype(f32) - vmin) / step)
    c = np.where(step == 0, f32(0), np.clip(c, 0, 255))
    return (c - 128).astype(np.int8)


def sq8_decode(c8, step, mid):
    return fmaf_emul(c8.astype(f32), np.broadcast_to(step, c8.shape), np.broadcast_to(mid, c8.shape))


def sq8_prepass(q, step, mid, qmax):
    """The query pre-pass of csrc/dense_i8_gemm.h: (w, alpha, bias, h, l) of every row of q."""
    w = (q.astype(f32) * step.astype(f32)).astype(f32)
    bias = (q.astype(f64) * mid.astype(f64)).sum(1).astype(f32)
    alpha = (np.abs(w).max(1) / f32(qmax)).astype(f32)
    safe = np.where(alpha > 0, alpha, f32(1)).astype(f64)[:, None]
    v = np.clip(np.rint(w.astype(f64) / safe), -qmax, qmax).astype(np.int64)
    v[alpha == 0] = 0
    h = np.floor_divide(v + 128, 256)
    return w, alpha, bias, h, v - 256 * h


def sq8_screen(c8, alpha, bias, h, l):
    """The screen GEMM and its epilogue, exactly: s~ [nq, N]."""
    c = c8.astype(np.int64)
    ah, al = h @ c.T, l @ c.T
    assert np.abs(ah).max(initial=0) < 2 ** 31 and np.abs(al).max(initial=0) < 2 ** 31
    t = fmaf_emul(np.full(ah.shape, 256, f32), ah.astype(f32), al.astype(f32))
    return fmaf_emul(np.broadcast_to(alpha[:, None], t.shape), t, np.broadcast_to(bias[:, None], t.shape))


def sq8_bound(D, q, c8, step, mid, w, alpha):
    """E_q [nq] of ops.dense_sq8_error_bound from the quantities the certificate kernel and `add` compute."""
    from repconc_amd import ops
    xhat = sq8_decode(c8, step, mid).astype(f64)
    c1 = float(np.abs(c8.astype(np.int64)).sum(1).max())
    X = float(np.sqrt((xhat ** 2).sum(1)).max()) * (1 + 2.0 ** -20)
    w1 = np.abs(w.astype(f64)).sum(1)
    b1 = np.abs(q.astype(f64) * mid.astype(f64)).sum(1)
    qn = np.sqrt((q.astype(f64) ** 2).sum(1))
    return ops.dense_sq8_error_bound(D, alpha.astype(f64), w1, b1, qn, c1, X)


def sq8_chain(q, c8, step, mid):
    """The contract's scores [nq, N]: the fmaf chain over the decoded rows."""
    xhat = sq8_decode(c8, step, mid)
    nq, N = q.shape[0], c8.shape[0]
    return chain_scores(np.repeat(q.astype(f32), N, axis=0), np.tile(xhat, (nq, 1))).reshape(nq, N)


def families(D, seed=0):
    """(name, q [8, D] fp32, c8 [32, D] int8, step [D], mid [D]): the inputs that strain the screen's bound."""
    rng = np.random.default_rng(4000 + D + seed)
    sign = lambda *s: rng.choice([-1.0, 1.0], s)
    out = []
    x = rng.standard_normal((32, D)) * (1.0 + 9.0 * (np.arange(D) % 7 == 0))       # anisotropic
    vmin, step, mid = sq8_train(x.astype(f32))
    out.append(("gaussian", rng.standard_normal((8, D)), sq8_encode(x, vmin, step), step, mid))
    ext = np.where(sign(32, D) > 0, 127, -128).astype(np.int8)                     # codes at the ends of the range,
    qa = np.abs(rng.standard_normal((8, D))) * np.sign(ext[:8].astype(f64) + 0.5)  # queries aligned with their signs
    out.append(("extreme codes, aligned queries", qa, ext, step, mid))
    out.append(("all codes -128", rng.standard_normal((8, D)), np.full((32, D), -128, np.int8), step, mid))
    out.append(("all codes 127, equal w", np.ones((8, D)) / np.maximum(step, 1e-30), np.full((32, D), 127, np.int8), step, mid))
    qh = rng.standard_normal((8, D))
    qh[np.arange(8), rng.integers(0, D, 8)] = 2.0 ** 20 * sign(8)
    out.append(("one huge component", qh, sq8_encode(x, vmin, step), step, mid))
    tiny = (step * 1e-20).astype(f32)
    out.append(("tiny steps", rng.standard_normal((8, D)), sq8_encode(x, vmin, step), tiny, mid))
    xc = x.copy()
    xc[:, ::3] = xc[0, ::3]                                                        # constant dimensions: step = 0
    vminc, stepc, midc = sq8_train(xc.astype(f32))
    assert (stepc[::3] == 0).all() and (midc[::3] == vminc[::3]).all()
    out.append(("constant dimensions", rng.standard_normal((8, D)) * 100.0, sq8_encode(xc, vminc, stepc), stepc, midc))
    out.append(("zero query", np.zeros((8, D)), sq8_encode(x, vmin, step), step, mid))
    big = (mid + 1e4).astype(f32)                                                  # the bias swamps the codes' part
    out.append(("large mid", rng.standard_normal((8, D)), sq8_encode(x, vmin, step), step, big))
    return [(n, q.astype(f32), c, s.astype(f32), m.astype(f32)) for n, q, c, s, m in out]


# --------------------------------------------------------------------------------------------------------------- CPU
def test_sq8_entry_points_and_options_are_validated_without_a_gpu():
    import sys
    import os
    import torch
    from conftest import ROOT
    from repconc_amd import _lib, faiss_compat, ops
    from repconc_amd.dense_index import FlatSQ8Index
    from repconc_amd.index import METRIC_INNER_PRODUCT, METRIC_L2
    from repconc_amd.models.dense.evaluate_dense import check_index_options, create_index
    lib = _lib.load()
    N, D = 8841823, 768
    prev = 0
    for nq in (1, 7, 128, 1200, 2048):
        ws = lib.rc_dense_sq8_search_ws_bytes(N, D, nq, 1000)
        assert ws > prev and lib.rc_dense_sq8_search_exact_ws_bytes(N, D, nq, 1000) > 0
        prev = ws
    # the fast layout of its siblings plus alpha, bias and two planes of D rounded up to 64 bytes per query
    assert lib.rc_dense_sq8_search_ws_bytes(N, 100, 1200, 10) >= lib.rc_dense_search_ws_bytes(N, 100, 1200, 10) + 1200 * (8 + 2 * 128)
    assert lib.rc_dense_sq8_search_ws_bytes(1000, D, 1200, 10) == lib.rc_dense_sq8_search_exact_ws_bytes(1000, D, 1200, 10)
    assert lib.rc_dense_sq8_search_ws_bytes(N, 65536, 4, 10) > 0
    for args in ((N, D, 1200, 8193), (1 << 32, D, 4, 10), (0, D, 4, 10), (N, 0, 4, 10), (N, D, 0, 10), (N, D, 4, 0),
                 (N, 65537, 4, 10)):
        assert lib.rc_dense_sq8_search_ws_bytes(*args) == 0 and lib.rc_dense_sq8_search_exact_ws_bytes(*args) == 0
    assert lib.rc_dense_sq8_scores_ws_bytes(65537, 4) == 0 and lib.rc_dense_sq8_scores_ws_bytes(D, 0) == 0
    assert lib.rc_dense_sq8_scores_ws_bytes(100, 3) % 256 == 0 and lib.rc_dense_sq8_scores_ws_bytes(100, 3) >= 3 * 2 * 128
    assert lib.rc_dense_sq8_qmax() == 127 * 256 + 127 == ops.dense_sq8_qmax() and lib.rc_dense_sq8_max_d() == 65536
    assert ops.dense_sq8_error_constants() == (0.5, 520.0, 194.0, 515.0, 2.1, 1.02, 1.0)
    # the order of the checks: shapes, then pointers (a live pointer stands in: nothing is dereferenced before the checks end)
    RC_ESHAPE, RC_EINVAL = -2, -1
    z = None
    assert lib.rc_dense_sq8_search_q(z, z, D, N, D, z, 4, z, z, 8193, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_sq8_search_q(z, z, D, 1 << 32, D, z, 4, z, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_sq8_search_q(z, z, 65537, N, 65537, z, 4, z, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_sq8_search_exact(z, z, D, N, D, z, 4, z, 8193, 0, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_sq8_search_exact(z, z, 65537, N, 65537, z, 4, z, 10, 0, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_sq8_search_q(z, z, D, N, D, z, 4, z, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_EINVAL
    assert lib.rc_dense_sq8_search_exact(z, z, D, N, D, z, 4, z, 10, 0, z, z, z, 0, z) == RC_EINVAL
    assert lib.rc_dense_sq8_scores(z, z, D, 1 << 32, D, z, 4, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_sq8_scores(z, z, D, N, D, z, 4, z, z, z, 0, z) == RC_EINVAL
    assert lib.rc_dense_sq8_decode(z, z, D, N, 65537, z, z, z) == RC_ESHAPE
    assert lib.rc_dense_sq8_decode(z, z, D, N, D, z, z, z) == RC_EINVAL
    x8, dec, q = torch.zeros(10, 16, dtype=torch.int8), torch.ones(2, 16), torch.zeros(2, 16)
    for call in (lambda: ops.dense_search_sq8(x8, dec, q, 1), lambda: ops.dense_search_sq8_exact(x8, dec, q, 1),
                 lambda: ops.dense_sq8_scores(x8, dec, q), lambda: ops.dense_sq8_decode(x8, dec)):
        with pytest.raises(_lib.RepconcHipError):
            call()
    for call in (lambda: ops.dense_search_sq8(x8.float(), dec, q, 1), lambda: ops.dense_search_sq8(x8, dec, q, 8193),
                 lambda: ops.dense_search_sq8(x8, dec[:1], q, 1), lambda: ops.dense_search_sq8(x8, dec, q[:, :8], 1)):
        with pytest.raises(ValueError):
            call()
    # the index: refusals before any device work
    for bad in (lambda: FlatSQ8Index(16, metric=METRIC_L2), lambda: FlatSQ8Index(65537), lambda: FlatSQ8Index(0),
                lambda: faiss_compat.IndexScalarQuantizer(16, faiss_compat.ScalarQuantizer.QT_8bit),          # Faiss's default: L2
                lambda: faiss_compat.IndexScalarQuantizer(16, faiss_compat.ScalarQuantizer.QT_4bit, METRIC_INNER_PRODUCT),
                lambda: faiss_compat.IndexScalarQuantizer(16, faiss_compat.ScalarQuantizer.QT_fp16, METRIC_INNER_PRODUCT)):
        with pytest.raises(ValueError):
            bad()
    index = faiss_compat.IndexScalarQuantizer(16, faiss_compat.ScalarQuantizer.QT_8bit, METRIC_INNER_PRODUCT, device="cpu")
    assert isinstance(index, FlatSQ8Index) and not index.is_trained and index.metric_type == METRIC_INNER_PRODUCT
    assert index._x.dtype == torch.int8 and index.ntotal == 0 and faiss_compat.ScalarQuantizer.QT_8bit == 0
    for early in (lambda: index.add(np.zeros((3, 16), f32)), lambda: index.search(np.zeros((3, 16), f32), 2),
                  lambda: index.reconstruct_n(0, 0)):
        with pytest.raises(ValueError):
            early()
    for bad in (np.zeros((0, 16), f32), np.zeros((3, 8), f32), np.full((3, 16), np.nan, f32), np.full((3, 16), np.inf, f32)):
        with pytest.raises(ValueError):
            index.train(bad)
        assert not index.is_trained
    for kw in (dict(use_float16=True), dict(screen="bf16x3"), dict(nlist=4), dict(metric="l2")):
        a = dict(metric="ip", use_float16=False, screen="fp32", nlist=0)
        a.update(kw)
        with pytest.raises(ValueError):
            check_index_options(a["metric"], a["use_float16"], a["screen"], a["nlist"], "int8")
        with pytest.raises(ValueError):
            create_index(np.zeros((4, 16), f32), storage="int8", **kw)            # before a device is looked at
    with pytest.raises(ValueError):
        check_index_options("ip", False, "fp32", 0, "int4")
    check_index_options("ip", False, "fp32", 0, "int8")
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import faiss
        assert faiss.IndexScalarQuantizer is faiss_compat.IndexScalarQuantizer and faiss.ScalarQuantizer.QT_8bit == 0
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))


def test_sq8_training_and_encoding_equal_their_definition_on_the_cpu():
    """train / add of the index on the CPU device (they are torch operators) against the numpy restatement: range, step, mid,
    codes, clamping outside the trained range, a constant dimension, refusal of non-finite rows, reset keeps the training."""
    import torch
    from repconc_amd.dense_index import FlatSQ8Index
    rng = np.random.default_rng(11)
    D = 24
    x = (rng.standard_normal((500, D)) * (1.0 + np.arange(D))).astype(f32)
    x[:, 5] = 3.25                                                                 # a constant dimension
    vmin, step, mid = sq8_train(x)
    assert step[5] == 0 and mid[5] == f32(3.25)
    index = FlatSQ8Index(D, device="cpu")
    index.train(x)
    assert index.is_trained
    assert np.array_equal(index.vmin.numpy(), vmin) and np.array_equal(index.step.numpy(), step)
    assert np.array_equal(index.mid.numpy(), mid)
    index.add(x[:200])
    index.add(torch.from_numpy(x[200:]))
    assert index.ntotal == 500 and index._x.dtype == torch.int8 and index._x.shape[0] == 500
    want = sq8_encode(x, vmin, step)
    assert np.array_equal(index.xb.numpy(), want)
    assert want.min() == -128 and want.max() == 127 and (want[:, 5] == -128).all()
    # every trained value lies in its bin: the decoded centre is within step / 2 (+ roundings)
    err = np.abs(sq8_decode(want, step, mid).astype(f64) - x)
    assert (err <= 0.5 * step.astype(f64) * (1 + 1e-5) + 1e-6 * np.abs(x)).all()
    out = np.vstack([x.min(0) - 100.0, x.max(0) + 100.0, x[0]]).astype(f32)        # outside the trained range: clamped
    index.add(out)
    got = index.xb.numpy()[500:]
    keep = np.arange(D) != 5
    assert (got[0] == -128).all() and (got[1][keep] == 127).all() and got[1][5] == -128 and np.array_equal(got[2], want[0])
    c1, X = index._cstat.tolist()
    codes = index.xb.numpy()
    assert c1 == float(np.abs(codes.astype(np.int64)).sum(1).max())
    xn = np.sqrt((sq8_decode(codes, step, mid).astype(f64) ** 2).sum(1)).max()
    assert xn <= X <= xn * (1 + 1e-5)
    for bad in (np.nan, np.inf, -np.inf):
        rows = x[:3].copy()
        rows[1, 7] = bad
        with pytest.raises(ValueError):
            index.add(rows)
        assert index.ntotal == 503 and np.array_equal(index.xb.numpy(), codes)     # nothing stored
        assert index._cstat.tolist() == [c1, X]
    index.reserve(2000)
    assert index._x.shape[0] == 2000 and np.array_equal(index.xb.numpy(), codes)
    index.reset()
    assert index.ntotal == 0 and index.is_trained and index._cstat is None and np.array_equal(index.step.numpy(), step)
    s0, i0 = index.search(x[:2], 3)
    assert np.all(i0 == -1) and np.all(np.isneginf(s0))
    with pytest.raises(ValueError):
        index.rerank(x[:2], np.zeros((2, 4), np.int64), 2)


def test_sq8_query_split_stays_in_int8_and_within_half_a_step():
    """The pre-pass's split for random and extreme w: both planes inside int8, 256 h + l within QMAX, and
    |w_d - alpha (256 h_d + l_d)| <= alpha / 2 (checked in fp64; the 2^-30 covers the fp64 quotient's rounding at a tie and this
    check's own arithmetic)."""
    from repconc_amd import ops
    qmax = ops.dense_sq8_qmax()
    assert qmax == 32639 and round(32767 / 256) == 128            # why the cap is not 32767
    rng = np.random.default_rng(5)
    D = 512
    one = np.ones(D, f32)
    cases = [rng.standard_normal((64, D)), rng.standard_normal((64, D)) * 2.0 ** rng.integers(-40, 40, (64, 1)),
             np.ones((4, D)), -np.ones((4, D)), np.zeros((4, D)),
             np.where(np.arange(D) == 7, 1e6, 1e-3)[None] * np.ones((4, 1)),                       # one dominant
             np.where(np.arange(D) % 2 == 0, 3.5, -3.5)[None] * np.ones((2, 1)),                   # +-max
             (rng.integers(-qmax, qmax + 1, (64, D)) + rng.choice([-0.5, 0.5, 0.4999, 0.0], (64, D))),   # at the ties
             rng.standard_normal((8, D)) * 1e-25, rng.standard_normal((8, D)) * 1e30]     # alpha inside the certificate's range
    for q in cases:
        w, alpha, _, h, l = sq8_prepass(q.astype(f32), one, one, qmax)
        assert h.min() >= -128 and h.max() <= 127 and l.min() >= -128 and l.max() <= 127
        v = 256 * h + l
        assert np.abs(v).max() <= qmax
        a64 = alpha.astype(f64)[:, None]
        assert (np.abs(w.astype(f64) - a64 * v) <= 0.5 * a64 * (1 + 2.0 ** -30)).all()
        hit = np.abs(w).max(1) > 0
        assert (np.abs(v).max(1)[hit] == qmax).all() and (v[~hit] == 0).all()      # the largest |w| takes the whole range
    # every v in the range splits into int8 limbs
    v = np.arange(-qmax, qmax + 1)
    h = np.floor_divide(v + 128, 256)
    l = v - 256 * h
    assert h.min() == -127 and h.max() == 127 and l.min() == -128 and l.max() == 127


@pytest.mark.parametrize("D", [16, 100, 768, 4096])
def test_sq8_error_bound_covers_the_exact_integer_screen(D):
    """|s~ - chain| <= E_q for the screen emulated exactly in integer numpy, on the adversarial families, with the constants
    read from the library."""
    from repconc_amd import ops
    qmax = ops.dense_sq8_qmax()
    worst = 0.0
    for name, q, c8, step, mid in families(D):
        w, alpha, bias, h, l = sq8_prepass(q, step, mid, qmax)
        approx = sq8_screen(c8, alpha, bias, h, l).astype(f64)
        chain = sq8_chain(q, c8, step, mid).astype(f64)
        E = sq8_bound(D, q, c8, step, mid, w, alpha)[:, None]
        assert np.isfinite(E).all() and (E > 0).all()
        ratio = float((np.abs(approx - chain) / E).max())
        print(f"D={D} {name}: max |s~ - s| / E_q = {ratio:.5f}, max |s| = {np.abs(chain).max():.3e}")
        assert ratio <= 1.0, (D, name, ratio)
        worst = max(worst, ratio)
    print(f"D={D}: largest emulated screen-error ratio {worst:.5f}")


# --------------------------------------------------------------------------------------------------------------- GPU
def _index(x, **kw):
    from repconc_amd.dense_index import FlatSQ8Index
    index = FlatSQ8Index(x.shape[1], **kw)
    index.train(x)
    index.add(x)
    return index


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("N,D,nq,k", SHAPES)
def test_sq8_search_ids_and_score_bits_equal_the_oracle_and_the_fp32_index(N, D, nq, k):
    """Parity with the oracle on reconstruct_n and with FlatIPIndex over the same decoded rows, both routes; above 131 072
    rows the fast route answers every query of gaussian data: nothing repeated, nothing sent to the exact route."""
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatIPIndex
    x = _randn((N, D), 1000 + N + D)
    q = _randn((nq, D), 2000 + nq + D)
    index = _index(x)
    del x
    xr = index.reconstruct_n(0, N)
    assert np.array_equal(xr[:64].cpu().numpy(), sq8_decode(index.xb[:64].cpu().numpy(), index.step.cpu().numpy(),
                                                            index.mid.cpu().numpy()))
    want = oracle_topk(xr, q, k)
    flat = FlatIPIndex(D)
    flat.add(xr)
    ref = flat.search(q, k)
    assert_matches(ref, want)
    for method in ("auto", "exact"):
        pending = ops.dense_search_sq8(index.xb, index._dec, q, k, id_offset=7, method=method, defer=True, cstat=index._cstat)
        got = pending.result()
        assert got[0].shape == (nq, k) and got[0].dtype.is_floating_point and not got[1].dtype.is_floating_point
        assert_matches(got, want, id_offset=7)
        assert np.array_equal(_bits(got[0]), _bits(ref[0]))
        if method == "auto" and N > 131072:
            assert pending.stats == {"retried_queries": 0, "exact_queries": 0}, pending.stats
    assert_matches(index.search(q, k), want)


@pytest.mark.gpu
@pytest.mark.parametrize("N,D,nq,k,pitch", [
    (131072, 15, 17, 10, 0),        # the largest N of the exact route
    (131073, 15, 17, 10, 0),        # the smallest of the fast route; D below one 16-byte chunk
    (131073, 1, 129, 5, 0),         # D = 1; a second query tile with one query
    (131201, 100, 1, 8192, 0),      # rows off the 128-row tile, D off the K stage, the largest k
    (131201, 100, 129, 3, 101),     # an odd row pitch
    (140001, 32, 17, 7, 33),        # D % 16 == 0 under a pitch that is not: the byte-wise form
    (140001, 32, 17, 7, 48),        # ... and under an aligned pitch wider than D: the 16-byte form
])
def test_sq8_search_off_the_tile_multiples(N, D, nq, k, pitch):
    import torch
    from repconc_amd import ops
    x = _randn((N, D), 3000 + N + D)
    q = _randn((nq, D), 4000 + nq + D)
    index = _index(x)
    del x
    codes = index.xb
    if pitch:
        wide = torch.full((N, pitch), 77, dtype=torch.int8, device=codes.device)
        wide[:, :D] = codes
        codes = wide[:, :D]
        assert codes.stride(0) == pitch
    want = oracle_topk(index.reconstruct_n(0, N), q, k)
    pending = ops.dense_search_sq8(codes, index._dec, q, k, defer=True, cstat=index._cstat)
    assert_matches(pending.result(), want)
    print(f"N={N} D={D} nq={nq} k={k} pitch={pitch}: {pending.stats}")
    assert_matches(ops.dense_search_sq8_exact(codes, index._dec, q, k), want)


def _directed(N, D, nq, seed, quiet=0):
    """The tie construction of test_dense_flat.py: queries 20 u + noise, and the row value c u whose score lies inside every
    query's top-100 of N gaussian rows.  The first `quiet` dimensions carry a hundredth of the queries' noise and none of u."""
    x = _randn((N, D), seed)
    u = _randn((D,), seed + 2)
    u[:quiet] = 0.0
    u /= u.norm()
    noise = _randn((nq, D), seed + 3)
    noise -= (noise @ u)[:, None] * u[None]
    noise[:, :quiet] *= 0.01
    q = 20.0 * u[None] + noise
    qn = float(q.norm(dim=1).mean())
    return x, q, (3.48 * qn / 20.0) * u


@pytest.mark.gpu
def test_sq8_search_ties_take_the_lower_id_and_fall_back_to_the_exact_route():
    """5 % duplicated rows come back in id order; 20 000 identical rows inside every query's top-100 leave no threshold that
    keeps fewer than 16 384 candidates: the exact route answers.  A corpus of identical rows terminates the same way."""
    import torch
    from repconc_amd import ops
    N, D, nq, k = 200000, 384, 16, 100
    x, q, row = _directed(N, D, nq, 31)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(32)
    src = torch.randint(0, N, (N // 20,), generator=g, device="cuda:0")
    dst = torch.randint(0, N, (N // 20,), generator=g, device="cuda:0")
    x[dst] = x[src].clone()
    x[90000:110000] = row[None]
    index = _index(x)
    del x
    want = oracle_topk(index.reconstruct_n(0, N), q, k)
    tied = (want[1] >= 90000) & (want[1] < 110000)
    assert tied.any(1).all() and (~tied).any(1).all()
    got = index.search(q, k)
    assert_matches(got, want)
    assert index.last_search.stats["exact_queries"] > 0
    assert_matches(ops.dense_search_sq8(index.xb, index._dec, q, k, method="exact"), want)
    same = _index(_randn((1, 32), 35).repeat(140000, 1) + 0.0)
    s, i = same.search(q[:3, :32], 10)
    assert same.last_search.stats["exact_queries"] == 3
    assert bool((i == torch.arange(10, device=i.device)[None]).all()) and bool((s == s[:, :1]).all())
    assert_matches((s, i), oracle_topk(same.reconstruct_n(0, 140000), q[:3, :32].contiguous(), 10))


@pytest.mark.gpu
def test_sq8_certificate_refuses_scores_closer_than_the_screen_error():
    """20 000 rows that differ by one to four code steps in one of 32 coordinates where the queries are small straddle the k-th
    score: their exact scores differ by far less than E_q, so no threshold inside the group can be certified — bit 2 on the first
    pass — and the answer still equals the oracle."""
    import torch
    from repconc_amd import ops
    N, D, nq, k = 200000, 384, 8, 100
    x, q, row = _directed(N, D, nq, 71, quiet=32)
    x[90000:110000] = row[None]
    index = _index(x)
    del x
    rows = torch.arange(20000, device="cuda:0")
    group = index._x[90000:110000]
    assert int(group.max()) < 120
    group[rows, rows % 32] += (1 + (rows // 32) % 4).to(torch.int8)      # one to four codes up in coordinate i % 32
    index._cstat = ops.dense_sq8_cstat(index.xb, index._dec)             # the rows changed behind add's back
    xr = index.reconstruct_n(0, N)
    want = oracle_topk(xr, q, k)
    tied = (want[1] >= 90000) & (want[1] < 110000)
    assert tied.any(1).all() and (~tied).any(1).all()            # the group straddles the k-th score of every query
    step, mid = index.step.cpu().numpy(), index.mid.cpu().numpy()
    qc = q.cpu().numpy()
    w, alpha, _, _, _ = sq8_prepass(qc, step, mid, ops.dense_sq8_qmax())
    c1, X = index._cstat.tolist()
    E = ops.dense_sq8_error_bound(D, alpha.astype(f64), np.abs(w.astype(f64)).sum(1), np.abs(qc.astype(f64) * mid).sum(1),
                                  np.sqrt((qc.astype(f64) ** 2).sum(1)), c1, X)
    sc = (q.double() @ xr[90000:110000].double().T).cpu().numpy()
    assert ((sc.max(1) - sc.min(1)) < 0.2 * E).all(), (sc.max(1) - sc.min(1), E)
    pending = ops.dense_search_sq8(index.xb, index._dec, q, k, defer=True, cstat=index._cstat)
    first = pending._qstatus.clone()
    assert bool(((first & 4) != 0).all()), first.tolist()
    assert_matches(pending.result(), want)
    assert pending.stats["retried_queries"] > 0 or pending.stats["exact_queries"] > 0
    print(f"E_q = {E.min():.4f} .. {E.max():.4f}; stats {pending.stats}")


@pytest.mark.gpu
def test_sq8_queries_the_bound_cannot_cover():
    """A zero query: every score is +0, every row ties, the list overflows and the exact route answers.  A query with one
    component 2^30 times the rest over a corpus that is binary in that dimension: the screen keeps nothing of the other
    components, half the corpus ties within E_q and the certificate is never given.  Non-finite and huge queries are refused
    and get the chain's own scores from the exact route."""
    import torch
    from repconc_amd import ops
    N, D, k = 140000, 64, 10
    x = _randn((N, D), 81)
    x[:, 5] = torch.where(x[:, 5] > 0, 1.0, -1.0)
    index = _index(x)
    del x
    xr = index.reconstruct_n(0, N)
    q = _randn((4, D), 82)
    q[0] = 0.0
    q[1, 5] = 2.0 ** 30
    q[2, 5] = -(2.0 ** 30)
    want = oracle_topk(xr, q, k)
    assert (want[0][0] == 0).all() and (want[1][0] == np.arange(k)).all()
    pending = ops.dense_search_sq8(index.xb, index._dec, q, k, defer=True, cstat=index._cstat)
    first = pending._qstatus.clone().tolist()
    assert first[0] & 2 and first[1] & 4 and first[2] & 4 and first[3] == 0, first
    assert_matches(pending.result(), want)
    assert pending.stats["exact_queries"] == 3, pending.stats
    # outside the certificate's range: refused whatever the scores are
    q2 = _randn((4, D), 83)
    q2[0, 3] = float("inf")
    q2[1, 3] = float("nan")
    q2[2, 3] = 2.0 ** 101
    pending = ops.dense_search_sq8(index.xb, index._dec, q2, k, defer=True, cstat=index._cstat)
    first = pending._qstatus.clone().tolist()
    assert first[0] & 4 and first[1] & 4 and first[2] & 4 and first[3] == 0, first
    got = pending.result()
    assert pending.stats["exact_queries"] == 3
    ex = ops.dense_search_sq8_exact(index.xb, index._dec, q2, k)
    assert np.array_equal(_bits(got[0]), _bits(ex[0])) and bool((got[1] == ex[1]).all())
    assert_matches((got[0][2:], got[1][2:]), oracle_topk(xr, q2[2:].contiguous(), k))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 100, 768, 1024])
def test_sq8_screen_error_stays_inside_the_certificate_bound(D):
    """|s~ - s_chain| <= E_q for every pair of the CPU test's families, s~ from rc_dense_sq8_scores.  Prints the largest ratio:
    the figure DESIGN.md section 4.9 quotes."""
    import torch
    from repconc_amd import ops
    qmax = ops.dense_sq8_qmax()
    worst, lines = 0.0, []
    for name, q, c8, step, mid in families(D):
        dec = torch.from_numpy(np.stack([step, mid])).cuda()
        approx = ops.dense_sq8_scores(torch.from_numpy(c8).cuda(), dec, torch.from_numpy(q).cuda()).cpu().numpy().astype(f64)
        chain = sq8_chain(q, c8, step, mid).astype(f64)
        w, alpha, bias, h, l = sq8_prepass(q, step, mid, qmax)
        E = sq8_bound(D, q, c8, step, mid, w, alpha)[:, None]
        err = np.abs(approx - chain)
        ratio = float((err / E).max())
        emul = float(np.abs(approx - sq8_screen(c8, alpha, bias, h, l).astype(f64)).max())
        lines.append(f"D={D} {name}: max |s~ - s| / E_q = {ratio:.5f}, max |s| = {np.abs(chain).max():.3e}, "
                     f"max err = {err.max():.3e}, max |s~ - emulated s~| = {emul:.3e}")
        worst = max(worst, ratio)
    print("\n".join(lines))
    print(f"D={D}: largest screen-error ratio {worst:.5f}")
    assert worst <= 1.0, lines


@pytest.mark.gpu
def test_sq8_index_train_add_reserve_reset_search_and_batching():
    """The index keeps int8 through add in pieces / reserve / growth / reset; numpy and tensor inputs agree bit for bit; the GPU
    encodes what the numpy restatement encodes; create_index(storage="int8") with batch_dense_search equals the per-batch
    loop; rows outside the trained range clamp; a negative slack forces retries."""
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatSQ8Index
    from repconc_amd.models.dense.evaluate_dense import batch_dense_search, create_index, dense_search
    N, D, nq, k = 3000, 384, 50, 20
    xb = _randn((N, D), 61).cpu().numpy()
    xb[:, 9] = -0.75                                              # a constant dimension
    qb = _randn((nq, D), 62).cpu().numpy()
    one = create_index(xb, storage="int8")
    assert isinstance(one, FlatSQ8Index) and one.is_trained and one.ntotal == N and one._x.shape[0] == N
    assert one._x.dtype == torch.int8 and one._x.element_size() == 1 and one.xb.dtype == torch.int8
    vmin, step, mid = sq8_train(xb)
    assert np.array_equal(one.step.cpu().numpy(), step) and np.array_equal(one.mid.cpu().numpy(), mid)
    assert np.array_equal(one.vmin.cpu().numpy(), vmin) and step[9] == 0
    assert np.array_equal(one.xb.cpu().numpy(), sq8_encode(xb, vmin, step))
    xr = one.reconstruct_n(0, N)
    assert np.array_equal(xr.cpu().numpy(), sq8_decode(one.xb.cpu().numpy(), step, mid)) and bool((xr[:, 9] == -0.75).all())
    assert np.array_equal(one.reconstruct_n(10, 5).cpu().numpy(), xr[10:15].cpu().numpy())
    three = FlatSQ8Index(D, device="cuda")
    three.train(torch.from_numpy(xb).cuda())
    three.add(xb[:1000])
    three.add(torch.from_numpy(xb[1000:1100]).cuda())
    assert three._x.shape[0] == 1500 and three._x.dtype == torch.int8         # growth 1.5x keeps the type
    three.add(xb[1100:])
    assert three.ntotal == N and bool((three.xb == one.xb).all())
    assert three._cstat.tolist() == one._cstat.tolist()
    assert float(one._cstat[1]) >= float(xr.double().norm(dim=1).max())
    s1, i1 = one.search(qb, k)
    s3, i3 = three.search(qb, k)
    assert isinstance(s1, np.ndarray) and i1.dtype == np.int64 and s1.dtype == np.float32
    assert np.array_equal(i1, i3) and np.array_equal(s1.view(np.uint32), s3.view(np.uint32))
    st, it = one.search(torch.from_numpy(qb).cuda(), k)
    assert isinstance(st, torch.Tensor) and st.is_cuda and it.is_cuda
    assert np.array_equal(it.cpu().numpy(), i1) and np.array_equal(st.cpu().numpy().view(np.uint32), s1.view(np.uint32))
    assert_matches((s1, i1), oracle_topk(xr, torch.from_numpy(qb).cuda(), k))
    corpus_ids = np.array([f"d{i}" for i in range(N)])
    qids = np.arange(nq)
    bs, bi = batch_dense_search(qids, qb, corpus_ids, one, k, batch_size=16)
    loop = [dense_search(a, b, corpus_ids, one, k) for a, b in zip(np.array_split(qids, 4), np.array_split(qb, 4))]
    assert np.array_equal(bi, np.concatenate([g[1] for g in loop])) and np.array_equal(bi, corpus_ids[i1])
    assert np.array_equal(bs.view(np.uint32), np.concatenate([g[0] for g in loop]).view(np.uint32))
    one.reserve(5000)
    assert one._x.shape[0] == 5000 and one._x.dtype == torch.int8 and np.array_equal(one.search(qb, k)[1], i1)
    far = np.vstack([xb.min(0) - 50.0, xb.max(0) + 50.0]).astype(f32)           # outside the trained range: clamped
    one.add(far)
    ends = one.xb[N:].cpu().numpy()
    keep = np.arange(D) != 9
    assert (ends[0] == -128).all() and (ends[1][keep] == 127).all() and one.ntotal == N + 2
    assert_matches(one.search(qb, k), oracle_topk(one.reconstruct_n(0, N + 2), torch.from_numpy(qb).cuda(), k))
    with pytest.raises(ValueError):
        one.add(np.full((1, D), np.nan, dtype=f32))
    assert one.ntotal == N + 2
    one.reset()
    assert one.ntotal == 0 and one.is_trained and one._x.dtype == torch.int8 and one._cstat is None
    s0, i0 = one.search(qb[:3], 5)
    assert np.all(i0 == -1) and np.all(np.isneginf(s0))
    one.add(xb[:10])
    assert np.array_equal(one.search(qb[:3], 5)[1], oracle_topk(xr[:10], torch.from_numpy(qb[:3]).cuda(), 5)[1])
    # the sampled-threshold route of the index, and a negative slack: retries, unchanged results
    N2, D2, nq2, k2 = 200000, 768, 64, 100
    x2, q2 = _randn((N2, D2), 41), _randn((nq2, D2), 42)
    big = FlatSQ8Index(D2)
    big.train(x2)
    big.add(x2[:120000])
    big.add(x2[120000:])
    del x2
    want = oracle_topk(big.reconstruct_n(0, N2), q2, k2)
    assert_matches(big.search(q2, k2), want)
    assert big.last_search.stats == {"retried_queries": 0, "exact_queries": 0}
    big.sel_slack = -50.0
    got = big.search(q2, k2)
    assert big.last_search.stats["retried_queries"] > 0
    assert_matches(got, want)
    pending = ops.dense_search_sq8(big.xb, big._dec, q2, k2, sel_slack=-50.0, defer=True)     # the statistics computed per call
    assert_matches(pending.result(), want)
    assert pending.stats["retried_queries"] > 0


@pytest.mark.gpu
def test_sq8_search_corpus_above_4_gib():
    """5 700 000 x 768 int8 = 4.4 GB: byte offsets past 2^32; query 0's best row is the last one."""
    from repconc_amd.dense_index import FlatSQ8Index
    N, D, nq, k = 5700000, 768, 16, 100
    q = _randn((nq, D), 52)
    index = FlatSQ8Index(D)
    index.train(_randn((100000, D), 50) * 1.3)
    index.reserve(N)
    for r0 in range(0, N, 950000):
        part = _randn((950000, D), 51 + r0)
        if r0 + 950000 == N:
            part[-1], part[-2] = 1.2 * q[0], 1.2 * q[1]
        index.add(part)
    assert index.ntotal == N and index._x.shape[0] == N
    assert index.xb.numel() * index.xb.element_size() > 4 << 30
    xr = index.reconstruct_n(0, N)
    want = oracle_topk(xr, q, k, qblock=16, rblock=1 << 19)
    del xr
    assert want[1][0, 0] == N - 1 and want[1][1, 0] == N - 2
    got = index.search(q, k)
    assert_matches(got, want)
    assert index.last_search.stats == {"retried_queries": 0, "exact_queries": 0}
