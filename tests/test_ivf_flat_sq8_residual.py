"""Residual encoding of the 8-bit IVF index: IVFFlatIndex(storage="int8", by_residual=True), ops.ivf_flat_sq8r_search and the
residual form of the coded scan of csrc/ivf_flat.hip (rc_ivf_flat_sq8r_search).

The contract: a row is stored as the code of r = fp32(x - coarse[cell]) under dense_index's scalar quantiser with one range for
all cells, a stored row IS x^ = fp32(fmaf(c - 128, step, mid) + coarse[cell]) (the decode's rounding, then the addition's), and a
search returns what the flat fp32 index of the same metric returns over those rows, restricted to the probed cells: ids and
score BITS, ties to the lower corpus id.

Every test uses non-zero centroids that differ per cell and per dimension: with zero centroids the residual form IS the plain
one and a wrong centroid would go unnoticed.

Oracles, none of them the code under test: the numpy restatements of the codec (tests/test_dense_sq8.py) followed by numpy's
fp32 addition of the centroid, the emulated chains over those rows (oracle_probed of tests/test_ivf_flat.py), and, where the
issue asks for it, the flat indexes of dense_index over reconstruct_n(0, ntotal) — after reconstruct_n itself was held against
the numpy restatement."""
import numpy as np
import pytest

from test_dense_flat import assert_matches
from test_dense_rerank import cut
from test_dense_sq8 import sq8_decode, sq8_encode, sq8_train
from test_ivf_flat import DEV, IP, L2, METRICS, _bits, _randn, oracle_probed
from test_ivf_flat_sq8 import _codes_in_corpus_order, _constructed, _corpus, _list_major, _stride

f32, f64 = np.float32, np.float64
RC_EINVAL, RC_ESHAPE = -1, -2


# ------------------------------------------------------------------------------------------------------------ helpers
def _nearest(x, c):
    """numpy: the L2-nearest centroid of every row, first minimum (fp64: the fixtures have no near ties)."""
    d2 = (c.astype(f64) ** 2).sum(1)[None, :] - 2.0 * x.astype(f64) @ c.astype(f64).T
    return d2.argmin(1)


def _cells_of(index):
    """The cell of every corpus row, from the list-major store."""
    cells = np.empty(index.ntotal, np.int64)
    cells[index.ids.cpu().numpy()] = np.repeat(np.arange(index.nlist), np.diff(index.list_off.cpu().numpy()))
    return cells


def _reconstructed(index, cells=None):
    """numpy: fp32(sq8_decode(codes) + coarse[cell]) of the rows the index holds, in corpus order, from its codes, its own
    step / mid and its centroids."""
    cells = _cells_of(index) if cells is None else np.asarray(cells)
    rhat = sq8_decode(_codes_in_corpus_order(index), index.step.cpu().numpy(), index.mid.cpu().numpy())
    return (rhat + index.coarse.cpu().numpy()[cells]).astype(f32)


def _same_bits(t, want):
    return np.array_equal(t.cpu().numpy().view(np.uint32), want.view(np.uint32))


def _residual_index(D, nlist, metric, x, coarse=None, cells=None, dev=DEV):
    """A residual int8 index over the rows x: trained and filled by `add` (coarse None), or the given centroids with the range of
    x's residuals and `add` (cells None) / the given cells."""
    from repconc_amd.ivf_flat import IVFFlatIndex
    index = IVFFlatIndex(D, nlist, device=dev, metric=metric, storage="int8", by_residual=True)
    if coarse is None:
        index.train(x)
        index.add(x)
        return index
    index.set_coarse(coarse)
    index.train_sq(x)
    if cells is None:
        index.add(x)
    else:
        index.set_lists(x, cells)
    return index


def _centroids(nlist, D, seed, scale=2.0):
    import torch
    return torch.from_numpy((np.random.default_rng(seed).standard_normal((nlist, D)) * scale).astype(f32))


# --------------------------------------------------------------------------------------------------------------- CPU
def test_construction_and_refusals_without_a_gpu():
    import os
    import sys
    import torch
    from conftest import ROOT
    import repconc_amd.faiss_compat as fc
    from repconc_amd.index import METRIC_L2
    from repconc_amd.ivf_flat import IVFFlatIndex
    for storage in ("float32", "float16"):
        with pytest.raises(ValueError, match="int8"):
            IVFFlatIndex(8, 4, device="cpu", storage=storage, by_residual=True)
    with pytest.raises(ValueError, match="int8"):
        IVFFlatIndex(8, 4, device="cpu", by_residual=True)
    with pytest.raises(TypeError):
        IVFFlatIndex(8, 4, "cpu", 0, "int8", True)                          # keyword-only
    assert IVFFlatIndex(8, 4, device="cpu").by_residual is False
    assert IVFFlatIndex(8, 4, device="cpu", storage="int8").by_residual is False
    index = IVFFlatIndex(8, 4, device="cpu", storage="int8", by_residual=True)
    assert index.by_residual is True and index.storage == "int8" and not index.is_trained
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((40, 8)).astype(f32))
    with pytest.raises(ValueError, match="centroids"):
        index.train_sq(x)                                                   # the residuals need the centroids first
    assert index._dec is None
    c = _centroids(4, 8, 2)
    index.set_coarse(c)
    assert not index.is_trained
    index.train_sq(x)
    assert index.is_trained
    index.set_coarse(c + 1.0)                                               # nothing stored: the centroids may still change
    index.set_coarse(c)
    index.set_lists(x, np.arange(40) % 4)
    with pytest.raises(ValueError, match="reset"):
        index.set_coarse(c)
    with pytest.raises(ValueError, match="reset"):
        index.train_sq(x)
    with pytest.raises(ValueError, match="reset"):
        index.train(x)
    assert index.ntotal == 40 and torch.equal(index.coarse, c)
    index.reset()
    index.set_coarse(c + 1.0)
    assert torch.equal(index.coarse, c + 1.0)
    # every other index keeps taking new centroids over stored rows
    for storage in ("float32", "int8"):
        plain = IVFFlatIndex(8, 4, device="cpu", storage=storage)
        plain.set_coarse(c)
        if storage == "int8":
            plain.train_sq(x)
        plain.set_lists(x, np.arange(40) % 4)
        plain.set_coarse(c + 1.0)
        assert plain.ntotal == 40 and torch.equal(plain.coarse, c + 1.0)
    # the shim keeps refusing Faiss's default
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import faiss
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))
    assert faiss.IndexIVFScalarQuantizer is fc.IndexIVFScalarQuantizer
    QT = fc.ScalarQuantizer
    for args in ((None, 8, 4, QT.QT_8bit, METRIC_L2, True), (None, 8, 4, QT.QT_8bit, METRIC_L2), (None, 8, 4)):
        with pytest.raises(ValueError, match="by_residual=False"):
            fc.IndexIVFScalarQuantizer(*args)
    with pytest.raises(ValueError, match="by_residual=False"):
        fc.IndexIVFScalarQuantizer(fc.IndexFlatL2(8, device="cpu"), 8, 4, QT.QT_8bit, by_residual=True)
    assert fc.IndexIVFScalarQuantizer(fc.IndexFlatL2(8, device="cpu"), 8, 4, QT.QT_8bit, by_residual=False).by_residual is False


def test_build_side_equals_the_numpy_restatement_on_the_cpu_device():
    """set_coarse + train_sq + set_lists / add on the CPU device (torch operators) against numpy: the range of the residuals, the
    codes, reconstruct_n in bits, add in parts against one set_lists, refusal of non-finite rows with nothing stored, clamping,
    reset."""
    import torch
    from repconc_amd.ivf_flat import IVFFlatIndex
    rng = np.random.default_rng(12)
    D, N, nlist = 24, 500, 7
    c = (rng.standard_normal((nlist, D)) * 2.0).astype(f32)
    x = (rng.standard_normal((N, D)) * (1.0 + np.arange(D))).astype(f32)
    c[:, 5] = np.arange(nlist, dtype=f32) * f32(0.5) - f32(1.25)            # quarters: c + 3.25 and its residual are exact
    for _ in range(20):                                                     # a constant dimension OF THE RESIDUAL ...
        near = _nearest(x, c)
        x[:, 5] = c[near, 5] + f32(3.25)
        if np.array_equal(near, _nearest(x, c)):
            break
    near = _nearest(x, c)
    r = (x - c[near]).astype(f32)
    assert (r[:, 5] == r[0, 5]).all() and len(set(x[:, 5].tolist())) > 1   # ... which the rows themselves do not have
    vmin, step, mid = sq8_train(r)
    assert step[5] == 0 and mid[5] == r[0, 5]
    index = IVFFlatIndex(D, nlist, device="cpu", storage="int8", by_residual=True)
    index.set_coarse(torch.from_numpy(c))
    index.train_sq(x)
    assert index.is_trained
    assert np.array_equal(index.vmin.numpy(), vmin) and np.array_equal(index.step.numpy(), step)
    assert np.array_equal(index.mid.numpy(), mid) and np.array_equal(index._dec.numpy(), np.stack([step, mid]))
    plain_range = sq8_train(x)
    assert not np.array_equal(plain_range[1], step)                         # not the range of the vectors themselves
    # set_lists: the residual against the centroid of the cell GIVEN
    given = rng.integers(0, nlist, N)
    index.set_lists(x, given)
    want = sq8_encode((x - c[given]).astype(f32), vmin, step)
    assert index.ntotal == N and index.xb.dtype == torch.int8
    assert np.array_equal(_codes_in_corpus_order(index), want)
    wxb, woff, wids = _list_major(want, given, nlist)
    assert np.array_equal(index.xb.numpy(), wxb) and index.list_off.tolist() == woff.tolist() and index.ids.tolist() == wids.tolist()
    assert np.array_equal(_cells_of(index), given)
    xhat = (sq8_decode(want, step, mid) + c[given]).astype(f32)
    assert _same_bits(index.reconstruct_n(0, N), xhat) and _same_bits(index.reconstruct_n(), xhat)
    assert _same_bits(index.reconstruct_n(17, 5), xhat[17:22]) and index.reconstruct_n(N, 0).shape == (0, D)
    assert not np.array_equal(xhat, sq8_decode(want, step, mid))            # the centroid is in it
    with pytest.raises(ValueError, match="outside"):
        index.reconstruct_n(N - 2, 3)
    # add: the residual against the centroid of the L2-nearest cell; two parts = one set_lists with those cells
    index.reset()
    index.add(x[:300])
    assert index.ntotal == 300
    held = _codes_in_corpus_order(index)
    assert np.array_equal(held, sq8_encode(r[:300], vmin, step)) and np.array_equal(_cells_of(index), near[:300])
    index.add(x[300:])
    codes = _codes_in_corpus_order(index)
    assert np.array_equal(codes[:300], held)                                # re-sorted, not re-encoded
    assert np.array_equal(codes, sq8_encode(r, vmin, step))
    assert want.min() == -128 and codes.min() == -128 and codes.max() == 127 and (codes[:, 5] == -128).all()
    one = IVFFlatIndex(D, nlist, device="cpu", storage="int8", by_residual=True)
    one.set_coarse(torch.from_numpy(c))
    one.train_sq(x)
    one.set_lists(x, near)
    assert torch.equal(one.xb, index.xb) and torch.equal(one.ids, index.ids) and torch.equal(one.list_off, index.list_off)
    assert _same_bits(index.reconstruct_n(0, N), (sq8_decode(codes, step, mid) + c[near]).astype(f32))
    # a non-finite row is refused and nothing is stored; so is a finite row whose residual is not
    before = (index.xb.clone(), index.ids.clone(), index.list_off.clone())
    for bad in (np.nan, np.inf, -np.inf):
        rows = x[:3].copy()
        rows[1, 7] = bad
        for call in (lambda: index.set_lists(rows, np.array([0, 1, 2])), lambda: index.add(rows)):
            with pytest.raises(ValueError, match="finite"):
                call()
            assert index.ntotal == N and all(torch.equal(a, b) for a, b in zip(before, (index.xb, index.ids, index.list_off)))
    huge = IVFFlatIndex(2, 2, device="cpu", storage="int8", by_residual=True)
    huge.set_coarse(torch.tensor([[3e38, 1.0], [-3e38, 2.0]]))
    huge.train_sq(torch.tensor([[3e38, 0.0], [-3e38, 1.0]]))
    with pytest.raises(ValueError, match="finite"):
        huge.set_lists(torch.tensor([[3e38, 0.0]]), np.array([1]))          # 3e38 - (-3e38) overflows fp32
    assert huge.ntotal == 0
    # values far outside the trained range clamp
    out = np.vstack([c[3] + vmin - 100.0, c[3] + r.max(0) + 100.0, x[0]]).astype(f32)
    index.set_lists(out, np.array([3, 3, near[0]]))
    got = _codes_in_corpus_order(index)
    keep = np.arange(D) != 5
    assert (got[0] == -128).all() and (got[1][keep] == 127).all() and got[1][5] == -128 and np.array_equal(got[2], codes[0])
    index.reset()
    assert index.ntotal == 0 and index.is_trained and np.array_equal(index.step.numpy(), step) and index.xb.shape == (0, D)
    assert np.array_equal(index.coarse.numpy(), c) and np.array_equal(index.vmin.numpy(), vmin)
    # train(): the centroids it fits, then the range of the training rows' residuals against them
    trained = IVFFlatIndex(D, nlist, device="cpu", storage="int8", by_residual=True)
    fitted = torch.from_numpy(c) + 0.5
    import repconc_amd.ivf_flat as mod
    kmeans, mod.coarse_kmeans = mod.coarse_kmeans, lambda xt, nlist_, iters, seed: fitted    # k-means itself runs on the GPU only
    try:
        trained.train(x)
    finally:
        mod.coarse_kmeans = kmeans
    cf = fitted.numpy()
    tv, ts, tm = sq8_train((x - cf[_nearest(x, cf)]).astype(f32))
    assert trained.is_trained and np.array_equal(trained.coarse.numpy(), cf)
    assert np.array_equal(trained.vmin.numpy(), tv) and np.array_equal(trained._dec.numpy(), np.stack([ts, tm]))


def test_ops_and_raw_abi_refuse_bad_arguments_without_a_gpu():
    import torch
    from repconc_amd import _lib, ops
    N, D, nq = 10, 16, 3
    x8, dec, q = torch.zeros(N, D, dtype=torch.int8), torch.ones(2, D), torch.zeros(nq, D)
    coarse = torch.ones(2, D)
    off, ids = torch.tensor([0, 4, 10]), torch.arange(N)
    pr = torch.zeros(nq, 1, dtype=torch.int32)
    bad = [
        (dict(xb8=x8.float()), "int8"), (dict(xb8=x8.to(torch.uint8)), "int8"), (dict(xb8=x8[0]), "same D"),
        (dict(q=q[:, :8]), "same D"), (dict(q=q.double()), "float32"), (dict(q=q.half()), "float32"),
        (dict(dec=dec[:1]), "dec"), (dict(dec=dec.double()), "dec"), (dict(dec=torch.ones(2, D + 1)), "dec"),
        (dict(coarse=coarse.double()), "coarse"), (dict(coarse=coarse.half()), "coarse"), (dict(coarse=torch.ones(3, D)), "coarse"),
        (dict(coarse=torch.ones(2, D + 1)), "coarse"), (dict(coarse=torch.ones(2 * D)), "coarse"), (dict(coarse=None), "coarse"),
        (dict(coarse=coarse[:1]), "coarse"),
        (dict(list_off=off.int()), "list_off"), (dict(list_off=torch.zeros(1, dtype=torch.int64)), "list_off"),
        (dict(ids=ids.int()), "ids"), (dict(ids=ids[:5]), "ids"),
        (dict(probes=pr.long()), "probes"), (dict(probes=pr[:2]), "probes"), (dict(probes=torch.zeros(nq, 3, dtype=torch.int32)), "probes"),
        (dict(k=0), "k must be"), (dict(k=8193), "k must be"), (dict(stride=0), "stride"), (dict(metric=2), "metric"),
        (dict(xb8=torch.zeros(0, D, dtype=torch.int8), ids=ids[:0]), "N"),
    ]
    for change, match in bad:
        kw = dict(xb8=x8, dec=dec, coarse=coarse, list_off=off, ids=ids, q=q, probes=pr, stride=8, k=2, metric=0)
        kw.update(change)
        with pytest.raises(ValueError, match=match):
            ops.ivf_flat_sq8r_search(**kw)
    wide = torch.zeros(2, 65537, dtype=torch.int8)
    with pytest.raises(ValueError, match="65536"):
        ops.ivf_flat_sq8r_search(wide, torch.ones(2, 65537), torch.ones(1, 65537), torch.tensor([0, 2]), torch.arange(2),
                                 torch.zeros(1, 65537), torch.zeros(1, 1, dtype=torch.int32), 4, 1)
    with pytest.raises(_lib.RepconcHipError, match="GPU only"):             # valid arguments on the CPU: loud, as every op
        ops.ivf_flat_sq8r_search(x8, dec, coarse, off, ids, q, pr, 8, 2)
    # the raw entry: the width limit is a shape error and comes first, null pointers (coarse among them) are RC_EINVAL
    lib = _lib.load()
    z = None
    call = lambda D_, ldx, ldc, k=2, nprobe=1: lib.rc_ivf_flat_sq8r_search(z, z, ldx, z, z, N, 2, D_, z, nq, z, z, ldc, z, nprobe, 8,
                                                                          k, 0, z, z, z, z, z, 0, z)
    assert call(65537, 65537, 65537) == RC_ESHAPE and call(65537, 65537, 1) == RC_ESHAPE
    assert call(65536, 65536, 65536) == RC_EINVAL and call(D, D, D) == RC_EINVAL
    assert call(D, D, D, k=0) == RC_EINVAL and call(D, D - 1, D) == RC_EINVAL and call(D, D, D - 1) == RC_EINVAL
    assert call(D, D, D, nprobe=3) == RC_EINVAL


def test_residual_codes_reconstruct_clustered_rows_more_closely_than_plain_codes():
    """The point of the feature, on clustered rows (8 centres N(0, 1), within-cell sd 0.25, D = 32, 3000 rows).

    The bound on a value.  Let c be the row's centroid, r = fp32(x - c), r^ the decoded code of r, x^ = fp32(r^ + c).  The range
    is trained on these residuals, so r lies inside it and the centre of its code's interval is within step_d / 2 of it.  Three
    fp32 roundings come on top, each at most 2^-24 times the magnitude of its result (round to nearest, normal numbers): of
    x - c (|r|), of the decode (|r^|) and of r^ + c (|x^|):
        |x - x^| <= step_d / 2 + 2^-24 (|r| + |r^| + |x^|).
    The numpy restatement of the codec meets it on this fixture with the rounding allowance used to 57 % at the worst value.

    The factor of one half between the two forms is a condition, not a measurement: a residual path that silently encodes the
    vectors themselves has the plain form's error and fails it.  The numpy restatement gives 0.0040 against 0.0129 (0.31)."""
    import torch
    from repconc_amd.ivf_flat import IVFFlatIndex
    rng = np.random.default_rng(4)
    centres = rng.standard_normal((8, 32)).astype(f32)
    labels = rng.integers(0, 8, 3000)
    x = (centres[labels] + rng.standard_normal((3000, 32)).astype(f32) * f32(0.25)).astype(f32)
    built = {}
    for by_residual in (False, True):
        index = IVFFlatIndex(32, 8, device="cpu", storage="int8", by_residual=by_residual)
        index.set_coarse(torch.from_numpy(centres))
        index.train_sq(x)
        index.add(x)
        built[by_residual] = index
    plain, res = built[False], built[True]
    cells = _cells_of(res)
    assert np.array_equal(cells, _nearest(x, centres)) and np.array_equal(_cells_of(plain), cells)
    xhat = res.reconstruct_n(0, 3000).numpy()
    assert _same_bits(res.reconstruct_n(0, 3000), _reconstructed(res))
    c = centres[cells]
    r = (x - c).astype(f32)
    rhat = sq8_decode(_codes_in_corpus_order(res), res.step.numpy(), res.mid.numpy())
    err = np.abs(x.astype(f64) - xhat.astype(f64))
    bound = res.step.numpy().astype(f64) / 2.0 + 2.0 ** -24 * (np.abs(r).astype(f64) + np.abs(rhat) + np.abs(xhat))
    worst_res = float(err.max())
    worst_plain = float(np.abs(x.astype(f64) - plain.reconstruct_n(0, 3000).numpy().astype(f64)).max())
    print(f"largest reconstruction error: residual {worst_res:.6f}, plain {worst_plain:.6f}, ratio {worst_res / worst_plain:.3f}; "
          f"smallest slack to the bound {float((bound - err).min()):.3e}")
    assert (err <= bound).all()
    assert worst_res <= 0.5 * worst_plain


# --------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", (1, 5, 16, 17, 40, 48))
def test_constructed_cells_match_the_chain_over_the_reconstructed_rows(D, metric):
    """D = 16, 48: rows of whole 16-byte pieces (the vector path); the others the byte path with a partial last K chunk, where
    the centroid's dimension index is clamped as the step's and the mid's are."""
    import torch
    from repconc_amd import ops
    x, q, cells_t, cells, probes = _constructed(D)
    coarse = _centroids(12, D, 900 + D)
    index = _residual_index(D, 12, metric, x, coarse, cells_t)
    assert index.ntotal == 3000 and index.xb.dtype == torch.int8 and index.by_residual
    assert np.array_equal(_cells_of(index), cells)
    xn, cn = x.cpu().numpy(), coarse.numpy()
    vmin, step, mid = sq8_train((xn - cn[_nearest(xn, cn)]).astype(f32))    # train_sq: the residuals against the nearest cells
    if D % 16:                                                              # (D % 16 == 0: the matrix-core assignment, not restated here)
        assert np.array_equal(index.step.cpu().numpy(), step) and np.array_equal(index.mid.cpu().numpy(), mid)
    assert np.array_equal(_codes_in_corpus_order(index),
                          sq8_encode((xn - cn[cells]).astype(f32), index.vmin.cpu().numpy(), index.step.cpu().numpy()))
    xhat = _reconstructed(index, cells)
    assert _same_bits(index.reconstruct_n(0, 3000), xhat) and _same_bits(index.reconstruct_n(100, 7), xhat[100:107])
    want = oracle_probed(xhat, q.cpu().numpy(), cells, probes, metric)
    pt = torch.from_numpy(probes).to(DEV)
    QG = ops.ivf_flat_query_group()
    for k in (1, 10, 829, 2000):
        for nq in (1, QG + 1, 43):
            got = index._search_probes(q[:nq], pt[:nq], k)
            assert_matches(got, cut(want[:nq], k, metric))
            assert index.last_search_stats == {"queries": nq, "fallback_queries": 0, "chunks": 1}
        got = index._search_probes(q[40:], pt[40:].flip(1), k)              # the special queries alone, probes in the other order
        assert_matches(got, cut(want[40:], k, metric))
    s, i = index._search_probes(q[40:42], pt[40:42], 10)
    pad = float("inf") if metric == L2 else float("-inf")
    assert bool((s[0] == pad).all()) and bool((i[0] == -1).all())           # only empty cells: all padding
    assert int(i[1, 0]) == int(np.nonzero(cells == 1)[0][0]) and bool((i[1, 1:] == -1).all()) and bool((s[1, 1:] == pad).all())


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", (5, 16))
def test_adjacent_tasks_of_different_cells_take_their_own_centroids(D, metric):
    """Three cells, every query probes two of them: one launch walks tasks of different cells side by side.  Cell 1 holds 5100
    rows, more than 512 x 8, so the blocks that stride over its row chunks all have to use that cell's centroid."""
    import torch
    N = 5300
    x, q = _randn((N, D), 931 + D), _randn((3, D), 932 + D)
    cells = np.where(np.arange(N) % 53 == 0, 0, np.where(np.arange(N) % 53 == 1, 2, 1))
    assert (cells == 1).sum() > 512 * 8
    index = _residual_index(D, 3, metric, x, _centroids(3, D, 933 + D), torch.from_numpy(cells))
    xhat = _reconstructed(index, cells)
    assert _same_bits(index.reconstruct_n(0, N), xhat)
    probes = np.array([[1, 2], [0, 1], [0, 2]], dtype=np.int32)
    want = oracle_probed(xhat, q.cpu().numpy(), cells, probes, metric)
    for k in (7, 5200):
        assert_matches(index._search_probes(q, torch.from_numpy(probes), k), cut(want, k, metric))
    assert index.last_search_stats["fallback_queries"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("pitch,shift", ((80, 0), (72, 0), (80, 1), (64, 0)))
def test_a_column_slice_of_a_wider_code_matrix_is_read_in_place(pitch, shift, metric):
    """D = 64: pitch 80 and 64 keep the 16-byte loads, pitch 72 and a base offset by one byte take the byte path; the centroids
    are a column slice of a wider matrix too (pitch 75 floats, offset 5)."""
    import ctypes as C
    import torch
    from repconc_amd import _lib, ops
    D, N, k = 64, 1500, 20
    rng = np.random.default_rng(500 + pitch + shift)
    codes = rng.integers(-128, 128, (N, D)).astype(np.int8)
    step, mid = (rng.random(D) * 0.1 + 0.01).astype(f32), rng.standard_normal(D).astype(f32)
    cen = (rng.standard_normal((4, D)) * 2.0).astype(f32)
    cells = rng.integers(0, 4, N)
    q = rng.standard_normal((9, D)).astype(f32)
    probes = np.array([[1, 3]] * 8 + [[0, 2]], dtype=np.int32)
    xb, off, ids = _list_major(codes, cells, 4)
    wide = torch.from_numpy(rng.integers(-128, 128, (N, pitch + shift)).astype(np.int8)).to(DEV)
    wide[:, shift:shift + D] = torch.from_numpy(xb).to(DEV)
    view = wide[:, shift:shift + D]
    assert view.stride(0) == pitch + shift and view.data_ptr() % 16 == (shift % 16)
    cwide = torch.from_numpy(rng.standard_normal((4, D + 11)).astype(f32)).to(DEV)
    cwide[:, 5:5 + D] = torch.from_numpy(cen).to(DEV)
    cview = cwide[:, 5:5 + D]
    assert cview.stride(0) == D + 11 and not cview.is_contiguous()
    xhat = (sq8_decode(codes, step, mid) + cen[cells]).astype(f32)
    want = oracle_probed(xhat, q, cells, probes, metric)
    args = (view, torch.from_numpy(np.stack([step, mid])).to(DEV), cview, torch.from_numpy(off).to(DEV),
            torch.from_numpy(ids).to(DEV), torch.from_numpy(q).to(DEV), torch.from_numpy(probes).to(DEV), _stride(cells, probes, 4), k)
    s, i, status, _ = ops.ivf_flat_sq8r_search(*args, metric=metric)
    assert int(status.item()) == 0
    assert_matches((s, i), cut(want, k, metric))
    # the raw entry with everything in place but the centroids: RC_EINVAL before any launch
    if (pitch, shift) == (64, 0):
        lib, h = _lib.load(), _lib.handle(0)
        p = lambda t: C.c_void_p(t.data_ptr())
        dense = [t.contiguous() for t in args[:7]]
        out = (torch.empty((9, k), device=DEV), torch.empty((9, k), dtype=torch.int64, device=DEV),
               torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(9, dtype=torch.int32, device=DEV))
        wsb = lib.rc_ivf_flat_search_ws_bytes(9, 2, 4, args[7])
        ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
        raw = lambda coarse, ldc: lib.rc_ivf_flat_sq8r_search(h, p(dense[0]), D, p(dense[3]), p(dense[4]), N, 4, D, p(dense[5]), 9,
                                                              p(dense[1]), coarse, ldc, p(dense[6]), 2, args[7], k, metric,
                                                              p(out[0]), p(out[1]), p(out[2]), p(out[3]), p(ws), wsb, None)
        assert raw(None, D) == RC_EINVAL and raw(p(dense[2]), D - 1) == RC_EINVAL
        assert raw(p(dense[2]), D) == 0
        torch.cuda.synchronize()
        assert_matches((out[0], out[1]), cut(want, k, metric))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", (768, 100))
def test_probing_every_cell_equals_the_flat_index_over_the_reconstructed_rows(D, metric):
    """Trained centroids (k-means of 16 cells: non-zero, different in every cell and dimension); D = 768: 16-byte pieces,
    D = 100: the byte path."""
    from repconc_amd.dense_index import FlatIPIndex, FlatL2Index
    N, nlist = 20000, 16
    x, q = _corpus(N, D, 50, 540 + D)
    index = _residual_index(D, nlist, metric, x)
    assert index.ntotal == N and index.is_trained
    cn = index.coarse.cpu().numpy()
    assert (cn != 0).all() and len(np.unique(cn)) == cn.size
    rec = index.reconstruct_n(0, N)
    assert _same_bits(rec, _reconstructed(index))
    flat = (FlatL2Index if metric == L2 else FlatIPIndex)(D, device=DEV)
    flat.add(rec)
    for k in (10, 100):
        ws, wi = flat.search(q, k)
        got = index.search(q, k, nprobe=nlist)
        assert_matches(got, (ws.cpu().numpy(), wi.cpu().numpy()))
        assert index.last_search_stats == {"queries": 50, "fallback_queries": 0, "chunks": 1}
    # a part of the cells: the fp32 flat index's own re-ranking of the ids in the probed cells
    import torch
    probes = index.probe(q, 3, ordered=False).cpu().numpy()
    cells = _cells_of(index)
    lists = [np.nonzero(np.isin(cells, probes[j]))[0] for j in range(50)]
    width = max(len(v) for v in lists)
    assert 0 < width <= 16384
    cand = np.full((50, width), -1, np.int64)
    for j, v in enumerate(lists):
        cand[j, :len(v)] = v
    ws, wi = flat.rerank(q, torch.from_numpy(cand).to(DEV), 100)
    assert_matches(index.search(q, 100, nprobe=3), (ws.cpu().numpy(), wi.cpu().numpy()))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_equal_reconstructed_rows_in_different_cells_take_the_lower_corpus_id(metric):
    """400 rows of one value in cells 3 and 1, whose centroids are equal: the same residual, the same code row, the same
    reconstructed row in two cells whose ascending cell order is not ascending id order; k cuts the group."""
    import torch
    D, N = 8, 1500
    x, q = _randn((N, D), 951), _randn((3, D), 952)
    x[:400] = (q[0] if metric == L2 else q[0] * (8.0 / q[0].norm()))           # one row, the best for query 0 (others: <q, x> ~ 3.5 |q| at most)
    coarse = _centroids(4, D, 953, 0.5)
    coarse[1] = coarse[3] = x[0].cpu() - torch.linspace(0.05, 0.12, D)      # the group's nearest centroid, in two cells
    cells = np.empty(N, np.int64)
    cells[:200], cells[200:400] = 3, 1
    cells[400:] = np.random.default_rng(5).integers(0, 4, N - 400)
    index = _residual_index(D, 4, metric, x, coarse, torch.from_numpy(cells))
    codes = _codes_in_corpus_order(index)
    assert (codes[:400] == codes[0]).all()
    xhat = _reconstructed(index, cells)
    assert _same_bits(index.reconstruct_n(0, N), xhat) and (xhat[:400].view(np.uint32) == xhat[0].view(np.uint32)).all()
    probes = np.array([[0, 1, 2, 3]] * 3, dtype=np.int32)
    want = oracle_probed(xhat, q.cpu().numpy(), cells, probes, metric)
    assert sorted(want[0][1][:400].tolist()) == list(range(400))            # the inputs do what they are meant to
    for k in (300, 399, 401):
        got = index._search_probes(q, torch.from_numpy(probes), k)
        assert_matches(got, cut(want, k, metric))
        assert index.last_search_stats["fallback_queries"] == 0
    s, i = index._search_probes(q, torch.from_numpy(probes), 300)
    assert i[0].tolist() == list(range(300))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_more_ties_than_the_candidate_list_holds_take_the_exact_route(metric):
    """17 000 rows of one value in ONE cell (equal residuals, equal reconstructed rows) at the top of every query: more than
    16384 probed rows tie at the 100th score, the status bit fires and every query is answered by the exact search over its
    probed rows, reconstructed with their centroids — the flat fp32 index's answer."""
    import torch
    from repconc_amd.dense_index import FlatIPIndex, FlatL2Index
    D, N, nq = 8, 20000, 5
    x = -_randn((N, D), 961).abs() - 0.5                       # every other row: negative components of magnitude >= 0.5
    x[1000:18000] = 0.0                                        # the group
    q = _randn((nq, D), 962).abs() * (0.01 if metric == L2 else 1.0)
    coarse = -_centroids(4, D, 963, 0.5).abs() - 0.3
    coarse[2] = torch.linspace(0.01, 0.08, D) * torch.tensor([1.0, -1.0] * (D // 2))       # the group's cell: its nearest
    cells = np.random.default_rng(6).integers(0, 4, N)
    cells[1000:18000] = 2
    index = _residual_index(D, 4, metric, x, coarse, torch.from_numpy(cells))
    rec = index.reconstruct_n(0, N)
    assert _same_bits(rec, _reconstructed(index, cells))
    flat = (FlatL2Index if metric == L2 else FlatIPIndex)(D, device=DEV)
    flat.add(rec)
    ws, wi = flat.search(q, 100)
    assert wi[:, 0].tolist() == [1000] * nq and wi[:, 99].tolist() == [1099] * nq          # the inputs do what they are meant to
    got = index.search(q, 100, nprobe=4)
    assert index.last_search_stats == {"queries": nq, "fallback_queries": nq, "chunks": 1}
    assert_matches(got, (ws.cpu().numpy(), wi.cpu().numpy()))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_chunked_search_equals_the_unchunked_one(metric):
    import torch
    from repconc_amd import ops
    from repconc_amd.ivf_flat import IVFFlatIndex
    D, N = 64, 10000
    x, _ = _corpus(N, D, 21, 270)
    q = _randn((50, D), 281)
    index = _residual_index(D, 32, metric, x)
    ws, wi = index.search(q, 50, nprobe=6)
    assert index.last_search_stats["chunks"] == 1
    stride = (max(4, int(index._sizes_desc[:6].sum())) + 3) // 4 * 4
    index.MAX_WS_BYTES = ops.ivf_flat_search_ws_bytes(13, 6, 32, stride)       # 13 queries per call: 50 go in four chunks
    gs, gi = index.search(q, 50, nprobe=6)
    assert index.last_search_stats == {"queries": 50, "fallback_queries": 0, "chunks": 4}
    assert torch.equal(gi, wi) and torch.equal(_bits(gs), _bits(ws))
    assert IVFFlatIndex.MAX_WS_BYTES == 4 << 30


@pytest.mark.gpu
def test_three_runs_have_identical_bits():
    import torch
    x, q = _corpus(20000, 768, 50, 540 + 768)
    index = _residual_index(768, 16, L2, x)
    runs = [index.search(q, 100, nprobe=3) for _ in range(3)]
    for s, i in runs[1:]:
        assert torch.equal(i, runs[0][1]) and torch.equal(_bits(s), _bits(runs[0][0]))


@pytest.mark.gpu
def test_add_in_parts_on_the_device_equals_one_set_lists_and_never_re_encodes():
    """The build side on the GPU (coarse_assign's matrix-core assignment): add in two parts = one add = set_lists with the cells
    coarse_assign gives."""
    import torch
    from repconc_amd.ivf import coarse_assign
    from repconc_amd.ivf_flat import IVFFlatIndex
    D, N = 64, 10000
    x, q = _corpus(N, D, 21, 270)
    one =_residual_index(D, 32, IP, x)
    parts = IVFFlatIndex(D, 32, device=DEV, storage="int8", by_residual=True)
    parts.set_coarse(one.coarse)
    parts.train_sq(x)
    parts.add(x[:7000])
    assert parts.ntotal == 7000
    held = _codes_in_corpus_order(parts)
    parts.add(x[7000:].cpu().numpy())
    assert np.array_equal(_codes_in_corpus_order(parts)[:7000], held)
    cells = coarse_assign(x, one.coarse)
    given = _residual_index(D, 32, IP, x, one.coarse, cells)
    assert torch.equal(one._dec, parts._dec) and torch.equal(one._dec, given._dec)
    for other in (parts, given):
        assert torch.equal(other.list_off, one.list_off) and torch.equal(other.ids, one.ids) and torch.equal(other.xb, one.xb)
    xn, cn, cl = x.cpu().numpy(), one.coarse.cpu().numpy(), cells.cpu().numpy()
    r = (xn - cn[cl]).astype(f32)
    vmin, step, mid = sq8_train(r)
    assert np.array_equal(one.step.cpu().numpy(), step) and np.array_equal(one.mid.cpu().numpy(), mid)
    assert np.array_equal(_codes_in_corpus_order(one), sq8_encode(r, vmin, step))
    ws, wi = one.search(q, 10, nprobe=4)
    gs, gi = parts.search(q, 10, nprobe=4)
    assert torch.equal(gi, wi) and torch.equal(_bits(gs), _bits(ws))


@pytest.mark.gpu
def test_refine_index_over_a_residual_int8_ivf_base_returns_the_fp32_flat_top_k():
    from repconc_amd.dense_index import FlatIPIndex
    from repconc_amd.refine_index import RefineIndex
    N, D, k, k_factor, nq = 5000, 64, 10, 500, 20                           # k * k_factor = N: the candidates cover the corpus
    x, q = _randn((N, D), 291), _randn((nq, D), 292)
    flat = FlatIPIndex(D, device=DEV)
    flat.add(x)
    ws, wi = flat.search(q, k)
    base = _residual_index(D, 16, IP, x)
    assert base.by_residual and base.ntotal == N
    refine = RefineIndex(base, flat, k_factor=k_factor)
    assert refine.ntotal == N and refine.d == D
    got = refine.search(q, k, nprobe=16)
    assert_matches(got, (ws.cpu().numpy(), wi.cpu().numpy()))
