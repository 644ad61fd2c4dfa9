"""Exact L2 search over 8-bit scalar-quantised flat storage: csrc/dense_search_l2_sq8.hip, the L2 forms of csrc/dense_i8_gemm.h
and csrc/dense_sq8_chain.h, ops.dense_search_l2_sq8, dense_index.FlatL2SQ8Index.

The contract: the store is FlatSQ8Index's (c - 128 as int8, a row IS fmaf(c - 128, step, mid)) and a distance is the chain of
dense_search_l2 over the decoded values, so ids and distance bits equal ops.dense_search_l2 on reconstruct_n(0, N) and the int8
IVFFlatIndex under L2 with every cell probed.  The int8 matrix cores only screen with sigma = fmaf(2, s~, -xsq): its error
against ||q||^2 - d must stay inside the bound the certificate uses (ops.dense_l2_sq8_error_bound)."""
import numpy as np
import pytest

from test_dense_flat import _randn, fmaf_emul
from test_dense_l2 import chain_l2
from test_dense_sq8 import families, sq8_decode, sq8_encode, sq8_prepass, sq8_screen, sq8_train

f32, f64 = np.float32, np.float64
EXACT_MAX_N = 131072


# ------------------------------------------------------------------------------------------- numpy restatements (CPU)
def sqnorm32(xhat):
    """fp32 [N]: the fp64 sum of squares of the decoded rows rounded once, the rule of ops.dense_row_sqnorms."""
    return (xhat.astype(f64) ** 2).sum(1).astype(f32)


def l2_families(D):
    """The seven families of the int8 inner-product tests (test_dense_sq8.families holds nine inputs for them) plus queries
    that equal decoded rows (d = 0)."""
    fam = families(D)
    name, q, c8, step, mid = fam[0]
    fam.append(("query = a decoded row", sq8_decode(c8[:8], step, mid), c8, step, mid))
    return fam


def l2_sigma(c8, alpha, bias, h, l, xsq):
    """The L2 screen exactly: sigma [nq, N] = fmaf(2, s~, -xsq) over the integer emulation of the int8 screen."""
    st = sq8_screen(c8, alpha, bias, h, l)
    return fmaf_emul(np.full(st.shape, 2, f32), st, np.broadcast_to(-xsq[None, :], st.shape))


def l2_bound(D, q, c8, step, mid, w, alpha):
    """E_q [nq] of ops.dense_l2_sq8_error_bound from the quantities the certificate kernel and `add` compute."""
    from repconc_amd import ops
    xhat = sq8_decode(c8, step, mid).astype(f64)
    c1 = float(np.abs(c8.astype(np.int64)).sum(1).max())
    X = float(np.sqrt((xhat ** 2).sum(1)).max()) * (1 + 2.0 ** -20)
    w1 = np.abs(w.astype(f64)).sum(1)
    b1 = np.abs(q.astype(f64) * mid.astype(f64)).sum(1)
    qn = np.sqrt((q.astype(f64) ** 2).sum(1))
    return ops.dense_l2_sq8_error_bound(D, alpha.astype(f64), w1, b1, qn, c1, X)


def l2_chain(q, c8, step, mid):
    """The contract's distances [nq, N]: the chain of squared differences over the decoded rows."""
    xhat = sq8_decode(c8, step, mid)
    nq, N = q.shape[0], c8.shape[0]
    return chain_l2(np.repeat(q.astype(f32), N, axis=0), np.tile(xhat, (nq, 1))).reshape(nq, N)


def restated_bound(D, alpha, w1, b1, qn, c1, X):
    """The header's formula (csrc/dense_search_l2_sq8.hip), written out with its own numbers."""
    u = 2.0 ** -24
    dpad = (D + 15) // 16 * 16
    R = (qn + X) ** 2
    rel = 1.0 * alpha * c1 + u * (1040.0 * w1 + 388.0 * alpha * D + 1030.0 * alpha * c1 + 4.2 * b1 + 1.01 * (dpad + 5) * R)
    e = (rel + 2.0 ** -149 * (dpad + np.sqrt(dpad) * qn + c1 + 3)) * (1 + 2.0 ** -20)
    return np.where((R < 2.0 ** 126) & (e < 2.0 ** 124), e, np.inf)


# --------------------------------------------------------------------------------------------------------------- CPU
def test_l2_sq8_error_constants_are_the_librarys_and_the_bound_is_the_headers_formula():
    from repconc_amd import _lib, ops
    import ctypes as C
    c = (C.c_double * 9)()
    _lib.load().rc_dense_l2_sq8_error_constants(c)
    assert tuple(c) == ops.dense_l2_sq8_error_constants() == (1.0, 1040.0, 388.0, 1030.0, 4.2, 1.01, 1.0, 2.0 ** 126, 2.0 ** 124)
    # twice the int8 inner-product unit's screen constants: its terms enter sigma twice
    ip = ops.dense_sq8_error_constants()
    assert tuple(c)[:5] == tuple(2 * v for v in ip[:5])
    rng = np.random.default_rng(1)
    for D in (1, 16, 100, 768, 65536):
        alpha, w1, b1, qn, c1, X = (rng.random(5) * 10.0 ** rng.integers(-6, 6, 5) for _ in range(6))
        got = ops.dense_l2_sq8_error_bound(D, alpha, w1, b1, qn, c1, X)
        assert np.array_equal(got, restated_bound(D, alpha, w1, b1, qn, c1, X)) and np.isfinite(got).all() and (got > 0).all()
    # outside the range nothing is certified
    assert np.isinf(ops.dense_l2_sq8_error_bound(16, 1e-6, 1.0, 1.0, 2.0 ** 63, 100.0, 1.0))
    assert np.isinf(ops.dense_l2_sq8_error_bound(16, 2.0 ** 110, 1.0, 1.0, 1.0, 2.0 ** 20, 1.0))
    assert np.isfinite(ops.dense_l2_sq8_error_bound(16, 1e-6, 1.0, 1.0, 2.0 ** 62, 100.0, 1.0))


@pytest.mark.parametrize("D", [16, 100, 768, 4096])
def test_l2_sq8_error_bound_covers_the_exact_integer_screen(D):
    """|sigma - ||q||^2 + d| <= E_q for the screen emulated exactly in integer numpy, xsq by the stated rule, ||q||^2 in fp64 and
    d the chain over the decoded rows, on the adversarial families.  Largest ratio: D=16 0.39642 (gaussian), D=100
    0.18635 and D=768 0.05342 (a query that is a decoded row), D=4096 0.01462 (large mid)."""
    from repconc_amd import ops
    qmax = ops.dense_sq8_qmax()
    worst = 0.0
    for name, q, c8, step, mid in l2_families(D):
        w, alpha, bias, h, l = sq8_prepass(q, step, mid, qmax)
        xhat = sq8_decode(c8, step, mid)
        sigma = l2_sigma(c8, alpha, bias, h, l, sqnorm32(xhat)).astype(f64)
        d = l2_chain(q, c8, step, mid).astype(f64)
        if name == "query = a decoded row":
            assert (np.diag(d[:, :8]) == 0).all()
        qq = (q.astype(f64) ** 2).sum(1)[:, None]
        E = l2_bound(D, q, c8, step, mid, w, alpha)[:, None]
        assert np.isfinite(E).all() and (E > 0).all()
        ratio = float((np.abs(sigma - qq + d) / E).max())
        print(f"D={D} {name}: max |sigma - ||q||^2 + d| / E_q = {ratio:.5f}, max d = {d.max():.3e}")
        assert ratio <= 1.0, (D, name, ratio)
        worst = max(worst, ratio)
    print(f"D={D}: largest emulated screen-error ratio {worst:.5f}")


def test_l2_sq8_workspace_helpers_and_argument_errors_need_no_gpu():
    import torch
    from repconc_amd import _lib, ops
    lib = _lib.load()
    N, D = 8841823, 768
    prev = 0
    for nq in (1, 7, 128, 1200, 2048):
        ws = lib.rc_dense_l2_sq8_search_ws_bytes(N, D, nq, 1000)
        assert ws > prev and lib.rc_dense_l2_sq8_search_exact_ws_bytes(N, D, nq, 1000) > 0
        assert ws == lib.rc_dense_sq8_search_ws_bytes(N, D, nq, 1000)           # the same layout: the norms are the caller's
        prev = ws
    assert lib.rc_dense_l2_sq8_search_ws_bytes(1000, D, 1200, 10) == lib.rc_dense_l2_sq8_search_exact_ws_bytes(1000, D, 1200, 10)
    assert lib.rc_dense_l2_sq8_search_ws_bytes(N, 65536, 4, 10) > 0
    for args in ((N, D, 1200, 8193), (1 << 32, D, 4, 10), (0, D, 4, 10), (N, 0, 4, 10), (N, D, 0, 10), (N, D, 4, 0),
                 (N, 65537, 4, 10)):
        assert lib.rc_dense_l2_sq8_search_ws_bytes(*args) == 0 and lib.rc_dense_l2_sq8_search_exact_ws_bytes(*args) == 0
    assert lib.rc_dense_l2_sq8_scores_ws_bytes(65537, 4) == 0 and lib.rc_dense_l2_sq8_scores_ws_bytes(D, 0) == 0
    assert lib.rc_dense_l2_sq8_scores_ws_bytes(100, 3) == lib.rc_dense_sq8_scores_ws_bytes(100, 3) > 0
    # the order of the checks: shapes, then pointers
    RC_ESHAPE, RC_EINVAL = -2, -1
    z = None
    assert lib.rc_dense_l2_sq8_search_q(z, z, D, N, D, z, 4, z, z, z, 8193, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_sq8_search_q(z, z, D, 1 << 32, D, z, 4, z, z, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_sq8_search_q(z, z, 65537, N, 65537, z, 4, z, z, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_sq8_search_exact(z, z, D, N, D, z, 4, z, 8193, 0, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_sq8_search_exact(z, z, 65537, N, 65537, z, 4, z, 10, 0, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_sq8_search_q(z, z, D, N, D, z, 4, z, z, z, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_EINVAL
    assert lib.rc_dense_l2_sq8_search_exact(z, z, D, N, D, z, 4, z, 10, 0, z, z, z, 0, z) == RC_EINVAL
    assert lib.rc_dense_l2_sq8_scores(z, z, D, 1 << 32, D, z, 4, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_l2_sq8_scores(z, z, D, N, D, z, 4, z, z, z, z, 0, z) == RC_EINVAL
    assert lib.rc_dense_sq8_row_sqnorms(z, z, D, N, 65537, z, z, z) == RC_ESHAPE
    assert lib.rc_dense_sq8_row_sqnorms(z, z, D, N, D, z, z, z) == RC_EINVAL
    off = __import__("ctypes").c_size_t(7)
    assert lib.rc_dense_l2_sq8_search_ws_counts(N, D, 4, 8193, off) == RC_ESHAPE and off.value == 0
    assert lib.rc_dense_l2_sq8_search_ws_counts(N, D, 4, 10, off) == 0 and off.value > 0
    assert lib.rc_dense_l2_sq8_search_ws_counts(1000, D, 4, 10, off) == 0 and off.value == 0
    x8, dec, q = torch.zeros(10, 16, dtype=torch.int8), torch.ones(2, 16), torch.zeros(2, 16)
    for call in (lambda: ops.dense_search_l2_sq8(x8, dec, q, 1), lambda: ops.dense_search_l2_sq8_exact(x8, dec, q, 1),
                 lambda: ops.dense_l2_sq8_scores(x8, dec, q)):
        with pytest.raises(_lib.RepconcHipError):
            call()
    for call in (lambda: ops.dense_search_l2_sq8(x8.float(), dec, q, 1), lambda: ops.dense_search_l2_sq8(x8, dec, q, 8193),
                 lambda: ops.dense_search_l2_sq8(x8, dec, q, 0), lambda: ops.dense_search_l2_sq8(x8, dec[:1], q, 1),
                 lambda: ops.dense_search_l2_sq8(x8, dec, q[:, :8], 1), lambda: ops.dense_sq8_row_sqnorms(x8.float(), dec),
                 lambda: ops.dense_sq8_row_sqnorms(x8, dec[:1])):
        with pytest.raises(ValueError):
            call()


def test_flat_l2_sq8_index_on_the_cpu_keeps_the_norms_of_the_decoded_rows():
    """train / add of the index on the CPU device against the numpy restatement: the codes, and _xsq = the fp64 sum of squares of
    the decoded rows rounded once, bit for bit, whether the rows arrive at once or in pieces; refusals store nothing; reset
    keeps the training."""
    import torch
    from repconc_amd.dense_index import FlatL2SQ8Index, FlatSQ8Index
    from repconc_amd.index import METRIC_L2
    from repconc_amd.refine_index import RefineIndex
    from repconc_amd.dense_index import FlatL2Index
    rng = np.random.default_rng(12)
    D = 24
    x = (rng.standard_normal((500, D)) * (1.0 + np.arange(D))).astype(f32)
    x[:, 5] = 3.25                                                                 # a constant dimension
    x[:, 7] += 1e4                                                                 # mid swamps the codes' part: the decode rounds
    vmin, step, mid = sq8_train(x)
    for bad in (0, 65537, -3):
        with pytest.raises(ValueError):
            FlatL2SQ8Index(bad, device="cpu")
    index = FlatL2SQ8Index(D, device="cpu")
    assert not index.is_trained and index.metric_type == METRIC_L2 and index.ntotal == 0 and index._x.dtype == torch.int8
    assert not isinstance(index, FlatSQ8Index)
    for early in (lambda: index.add(x[:3]), lambda: index.search(x[:3], 2), lambda: index.reconstruct_n(0, 0)):
        with pytest.raises(ValueError):
            early()
    index.train(x)
    assert index.is_trained and np.array_equal(index.step.numpy(), step) and np.array_equal(index.mid.numpy(), mid)
    index.add(x[:200])
    index.add(torch.from_numpy(x[200:]))
    codes = sq8_encode(x, vmin, step)
    want = sqnorm32(sq8_decode(codes, step, mid))
    assert index.ntotal == 500 and np.array_equal(index.xb.numpy(), codes)
    assert index._xsq.dtype == torch.float32 and index._xsq.shape[0] == index._x.shape[0]
    assert np.array_equal(index._xsq[:500].numpy().view(np.uint32), want.view(np.uint32))
    whole = FlatL2SQ8Index(D, device="cpu")
    whole.train(x)
    whole.ROWS_PER_STEP = 128                                                      # several chunks inside one add
    whole.add(x)
    assert np.array_equal(whole._xsq[:500].numpy().view(np.uint32), want.view(np.uint32))
    assert whole._cstat.tolist() == index._cstat.tolist()
    for bad in (np.nan, np.inf, -np.inf):
        rows = x[:3].copy()
        rows[1, 7] = bad
        with pytest.raises(ValueError):
            index.add(rows)
        assert index.ntotal == 500 and np.array_equal(index.xb.numpy(), codes)     # nothing stored
        assert np.array_equal(index._xsq[:500].numpy().view(np.uint32), want.view(np.uint32))
    index.reserve(2000)
    assert index._x.shape[0] == 2000 and index._xsq.shape[0] == 2000 and np.array_equal(index.xb.numpy(), codes)
    assert np.array_equal(index._xsq[:500].numpy().view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        index.rerank(x[:2], np.zeros((2, 4), np.int64), 2)
    refine = FlatL2Index(D, device="cpu")
    assert RefineIndex(index, refine).metric_type == METRIC_L2                     # a base of a RefineIndex
    index.reset()
    assert index.ntotal == 0 and index.is_trained and index._cstat is None and index._xsq.shape[0] == 0
    assert np.array_equal(index.step.numpy(), step)
    d0, i0 = index.search(x[:2], 3)
    assert np.all(i0 == -1) and np.all(np.isposinf(d0))


# --------------------------------------------------------------------------------------------------------------- GPU
def _index(x, **kw):
    from repconc_amd.dense_index import FlatL2SQ8Index
    index = FlatL2SQ8Index(x.shape[1], **kw)
    index.train(x)
    index.add(x)
    return index


def _same(got, want, id_offset=0):
    """ids and distance bits of two device results."""
    import torch
    assert got[0].shape == want[0].shape and got[1].dtype == torch.int64
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
    assert torch.equal(got[1], torch.where(want[1] >= 0, want[1] + id_offset, want[1]))


def _sorted_l2(got):
    d, i = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert (d >= 0).all() and not np.signbit(d).any()
    assert ((d[:, 1:] > d[:, :-1]) | ((d[:, 1:] == d[:, :-1]) & ((i[:, 1:] > i[:, :-1]) | (i[:, 1:] == -1)))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("D,nq,k", [(16, 1, 1), (64, 7, 10), (100, 130, 100), (768, 33, 100)])
def test_l2_sq8_fast_route_ids_and_distance_bits_equal_the_l2_search_over_the_decoded_rows(D, nq, k):
    """N just above the exact route's limit and off the 128-row tile.  Three references: ops.dense_search_l2 over
    reconstruct_n, the exact route, and (one shape) the int8 IVF index under L2 with every cell probed.  On gaussian data the
    fast route answers every query of the (64, 7, 10) and (768, 33, 100) shapes itself: a bound so loose that queries end on
    the exact route would show here."""
    import torch
    from repconc_amd import ops
    from repconc_amd.index import METRIC_L2
    from repconc_amd.ivf_flat import IVFFlatIndex
    N = 133001
    x = _randn((N, D), 1000 + N + D)
    q = _randn((nq, D), 2000 + nq + D)
    index = _index(x)
    xr = index.reconstruct_n(0, N)
    want = ops.dense_search_l2(xr, q, k, method="exact")
    pending = ops.dense_search_l2_sq8(index.xb, index._dec, q, k, id_offset=7, defer=True, xsq=index._xsq[:N], cstat=index._cstat)
    first = int(((pending._qstatus & 4) != 0).sum())
    got = pending.result()
    print(f"D={D} nq={nq} k={k}: bit 2 on the first pass for {first} queries, {pending.stats}")
    _same(got, want, id_offset=7)
    _sorted_l2(got)
    if (D, nq, k) in ((64, 7, 10), (768, 33, 100)):
        assert pending.stats["exact_queries"] == 0, pending.stats
    _same(ops.dense_search_l2_sq8_exact(index.xb, index._dec, q, k), want)
    _same(ops.dense_search_l2_sq8(index.xb, index._dec, q, k), want)                # norms and statistics computed per call
    _same(index.search(q, k), want)
    if D == 64:
        ivf = IVFFlatIndex(D, 8, metric=METRIC_L2, storage="int8")
        ivf.train(x)
        ivf.add(x)
        assert torch.equal(ivf._dec, index._dec)
        _same(ivf.search(q, k, nprobe=8), want)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 1000])
def test_l2_sq8_exact_route_and_padding_past_n(N):
    import torch
    from repconc_amd import ops
    D, nq, k = 100, 9, 1200
    x = _randn((max(N, 50), D), 3000 + N)
    q = _randn((nq, D), 3100 + N)
    index = _index(x)
    codes = index.xb[:N]
    xr = index.reconstruct_n(0, N)
    want = ops.dense_search_l2(xr, q, k)
    for got in (ops.dense_search_l2_sq8(codes, index._dec, q, k), ops.dense_search_l2_sq8_exact(codes, index._dec, q, k)):
        _same(got, want)
        assert bool(torch.isposinf(got[0][:, N:]).all()) and bool((got[1][:, N:] == -1).all())
        assert bool((got[1][:, :N].sort(1).values == torch.arange(N, device=q.device)[None]).all())
    _same(ops.dense_search_l2_sq8(codes, index._dec, q, 1), (want[0][:, :1], want[1][:, :1]))


@pytest.mark.gpu
@pytest.mark.parametrize("pitch,off", [(80, 0), (67, 0), (80, 1), (64, 3)])
def test_l2_sq8_row_pitch_and_base_alignment_do_not_change_a_bit(pitch, off):
    """A row pitch wider than D (a multiple of 16 and not) and a base pointer off 16 bytes: the screen's byte-wise form and the
    rescorer's element-wise path give the bits of the aligned forms."""
    import torch
    from repconc_amd import ops
    N, D, nq, k = 133001, 64, 9, 20
    x = _randn((N, D), 4000 + D)
    q = _randn((nq, D), 4100 + D)
    index = _index(x)
    want = ops.dense_search_l2_sq8(index.xb, index._dec, q, k, xsq=index._xsq[:N], cstat=index._cstat)
    buf = torch.full((N * pitch + 16,), 77, dtype=torch.int8, device=q.device)
    wide = buf[off:off + N * pitch].view(N, pitch)
    wide[:, :D] = index.xb
    codes = wide[:, :D]
    assert codes.stride(0) == pitch and codes.data_ptr() % 16 == off % 16
    pending = ops.dense_search_l2_sq8(codes, index._dec, q, k, defer=True, xsq=index._xsq[:N], cstat=index._cstat)
    _same(pending.result(), want)
    assert pending.stats["exact_queries"] == 0
    _same(ops.dense_search_l2_sq8_exact(codes, index._dec, q, k), want)
    assert torch.equal(ops.dense_sq8_row_sqnorms(codes[:5000], index._dec).view(torch.int32), index._xsq[:5000].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 100, 768, 1024])
def test_l2_sq8_screen_equals_its_emulation_and_stays_inside_the_certificate_bound(D):
    """rc_dense_l2_sq8_scores equals the integer numpy emulation bit for bit on every family of the CPU test, hence
    |sigma - ||q||^2 + d| <= E_q; the norm kernel gives the stated rule's bits.  Prints the largest ratio: the figure DESIGN.md
    section 4.9 quotes."""
    import torch
    from repconc_amd import ops
    qmax = ops.dense_sq8_qmax()
    worst, lines = 0.0, []
    for name, q, c8, step, mid in l2_families(D):
        dec = torch.from_numpy(np.stack([step, mid])).cuda()
        xsq = sqnorm32(sq8_decode(c8, step, mid))
        got_xsq = ops.dense_sq8_row_sqnorms(torch.from_numpy(c8).cuda(), dec).cpu().numpy()
        assert np.array_equal(got_xsq.view(np.uint32), xsq.view(np.uint32)), name
        sigma = ops.dense_l2_sq8_scores(torch.from_numpy(c8).cuda(), dec, torch.from_numpy(q).cuda(),
                                        xsq=torch.from_numpy(xsq).cuda()).cpu().numpy()
        w, alpha, bias, h, l = sq8_prepass(q, step, mid, qmax)
        assert np.array_equal(sigma.view(np.uint32), l2_sigma(c8, alpha, bias, h, l, xsq).view(np.uint32)), name
        d = l2_chain(q, c8, step, mid).astype(f64)
        qq = (q.astype(f64) ** 2).sum(1)[:, None]
        E = l2_bound(D, q, c8, step, mid, w, alpha)[:, None]
        err = np.abs(sigma.astype(f64) - qq + d)
        ratio = float((err / E).max())
        lines.append(f"D={D} {name}: max |sigma - ||q||^2 + d| / E_q = {ratio:.5f}, max d = {d.max():.3e}, "
                     f"max err = {err.max():.3e}")
        worst = max(worst, ratio)
    print("\n".join(lines))
    print(f"D={D}: largest screen-error ratio {worst:.5f}")
    assert worst <= 1.0, lines


@pytest.mark.gpu
def test_l2_sq8_self_matches_are_plus_zero_and_ties_take_the_lower_id():
    import torch
    from repconc_amd import ops
    N, D, nq, k = 150000, 64, 32, 10
    x = _randn((N, D), 31)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(32)
    perm = torch.randperm(N, generator=g, device="cuda:0")
    src, dst = perm[: N // 20], perm[N // 20: 2 * (N // 20)]   # 5 % of the rows are copies of other rows, each copied once
    x[dst] = x[src].clone()
    index = _index(x)
    xr = index.reconstruct_n(0, N)
    q = xr[dst[:nq]].clone()                                  # every query equals a decoded row that has a duplicate
    want = ops.dense_search_l2(xr, q, k, method="exact")
    got = index.search(q, k)
    _same(got, want)
    d, i = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert np.all(d[:, :2].view(np.uint32) == 0)             # the zero distances are +0.0f
    assert np.all(i[:, 0] < i[:, 1]) and set(i[:, 0]) | set(i[:, 1]) >= set(dst[:nq].tolist())
    _same(ops.dense_search_l2_sq8(index.xb, index._dec, q, k, method="exact"), want)


@pytest.mark.gpu
def test_l2_sq8_tie_group_across_the_kth_distance_falls_back_to_the_exact_route():
    """20 000 identical rows whose distance sits inside every query's top-100: the group overflows the candidate list whatever
    the slack, the exact route answers with the oracle's ids."""
    from repconc_amd import ops
    N, D, nq, k = 150000, 64, 4, 100
    x = _randn((N, D), 35)
    q = 0.05 * _randn((nq, D), 36)
    v = _randn((D,), 37)
    x[90000:110000] = (v * (32.0 ** 0.5 / v.norm()))[None]   # |v|^2 = 32: a few dozen of the gaussian rows are nearer
    index = _index(x)
    want = ops.dense_search_l2(index.reconstruct_n(0, N), q, k, method="exact")
    tied = (want[1] >= 90000) & (want[1] < 110000)
    assert bool(tied.any(1).all()) and bool((~tied).any(1).all())     # the group straddles the k-th distance of every query
    got = index.search(q, k)
    _same(got, want)
    assert index.last_search.stats["exact_queries"] > 0


@pytest.mark.gpu
def test_l2_sq8_certificate_refuses_distances_closer_than_the_screen_error_and_a_negative_slack_retries():
    """Every row and query is one vector of norm ~30 plus 1e-4 noise: all distances are far below E_q, no answer of the fast
    route can be certified — bit 2 on every query of the first pass — and the exact route gives the oracle's result.  On
    gaussian data a negative slack forces retries and changes nothing."""
    from repconc_amd import ops
    N, D, nq, k = 140001, 64, 8, 10
    base = _randn((D,), 81)
    base *= 30.0 / base.norm()
    x = base[None] + 1e-4 * _randn((N, D), 82)
    q = base[None] + 1e-4 * _randn((nq, D), 83)
    index = _index(x)
    xr = index.reconstruct_n(0, N)
    want = ops.dense_search_l2(xr, q, k, method="exact")
    qc = q.cpu().numpy()
    step, mid = index.step.cpu().numpy(), index.mid.cpu().numpy()
    w, alpha, _, _, _ = sq8_prepass(qc, step, mid, ops.dense_sq8_qmax())
    c1, X = index._cstat.tolist()
    E = ops.dense_l2_sq8_error_bound(D, alpha.astype(f64), np.abs(w.astype(f64)).sum(1), np.abs(qc.astype(f64) * mid).sum(1),
                                     np.sqrt((qc.astype(f64) ** 2).sum(1)), c1, X)
    dall = (q.double()[:, None, :] - xr.double()[None, ::7, :]).square().sum(2)
    assert float(dall.max()) < 1e-2 * E.min(), (float(dall.max()), E)
    pending = ops.dense_search_l2_sq8(index.xb, index._dec, q, k, defer=True, xsq=index._xsq[:N], cstat=index._cstat)
    assert bool(((pending._qstatus & 4) != 0).all())          # bit 2 on every query of the first pass
    _same(pending.result(), want)
    assert pending.stats["exact_queries"] == nq
    x2, q2 = _randn((N, 128), 41), _randn((64, 128), 42)
    gauss = _index(x2)
    want2 = ops.dense_search_l2(gauss.reconstruct_n(0, N), q2, 100, method="exact")
    _same(gauss.search(q2, 100), want2)
    assert gauss.last_search.stats == {"retried_queries": 0, "exact_queries": 0}
    gauss.sel_slack = -50.0
    got = gauss.search(q2, 100)
    assert gauss.last_search.stats["retried_queries"] > 0
    _same(got, want2)


@pytest.mark.gpu
def test_flat_l2_sq8_index_above_the_exact_route_uses_its_cached_norms(monkeypatch):
    """An index large enough for the fast route, added in uneven pieces through growth, and again after a reset: the cached
    norms are the kernel's over the whole store, and a search computes none."""
    import torch
    from repconc_amd import ops
    from repconc_amd.dense_index import FlatL2SQ8Index
    N, D, nq, k = 140001, 64, 16, 10
    x, q = _randn((N, D), 91), _randn((nq, D), 92)
    index = FlatL2SQ8Index(D, device="cuda")
    index.train(x)
    for a, b in ((0, 50000), (50000, 50007), (50007, N)):
        index.add(x[a:b])
    assert index._xsq.shape[0] == index._x.shape[0] >= N
    norms = ops.dense_sq8_row_sqnorms(index.xb, index._dec)
    assert torch.equal(index._xsq[:N].view(torch.int32), norms.view(torch.int32))
    assert torch.equal(norms.view(torch.int32), ops.dense_row_sqnorms(index.reconstruct_n(0, N)).view(torch.int32))
    want = ops.dense_search_l2(index.reconstruct_n(0, N), q, k, method="exact")

    def refuse(*a, **kw):
        raise AssertionError("the search recomputed the norms")
    with monkeypatch.context() as m:
        m.setattr(ops, "dense_sq8_row_sqnorms", refuse)
        m.setattr(ops, "dense_sq8_cstat", refuse)
        _same(index.search(q, k), want)
        assert index.last_search.stats == {"retried_queries": 0, "exact_queries": 0}
    index.reset()
    assert index.ntotal == 0 and index.is_trained and index._xsq.shape[0] == 0
    index.add(x[:N - 1])
    index.add(x[N - 1:])
    assert torch.equal(index._xsq[:N].view(torch.int32), norms.view(torch.int32))
    with monkeypatch.context() as m:
        m.setattr(ops, "dense_sq8_row_sqnorms", refuse)
        _same(index.search(q, k), want)
