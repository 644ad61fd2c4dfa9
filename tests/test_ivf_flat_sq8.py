"""8-bit scalar-quantised storage of the exact IVF search: the coded scan of csrc/ivf_flat.hip (rc_ivf_flat_sq8_search),
ops.ivf_flat_sq8_search, ivf_flat.IVFFlatIndex(storage="int8"), faiss_compat.IndexIVFScalarQuantizer.

The contract: the store holds the codes of dense_index's scalar quantiser (c - 128 as int8), a stored row IS its decoded value
fmaf(c - 128, step, mid), and a search returns what the flat fp32 index of the same metric returns over the decoded rows,
restricted to the probed cells: ids and score BITS, ties to the lower corpus id.

Oracles, none of them the code under test: the numpy restatements of the codec (tests/test_dense_sq8.py), the emulated chains of
tests/test_dense_flat.py / test_dense_l2.py over the numpy-decoded rows of the probed cells (oracle_probed of
tests/test_ivf_flat.py), and, at D = 768 and D = 100, the flat indexes of dense_index on the same device."""
import functools

import numpy as np
import pytest

from test_dense_flat import assert_matches
from test_dense_rerank import cut
from test_dense_sq8 import families, sq8_decode, sq8_encode, sq8_train
from test_ivf_flat import CELL_SIZES, DEV, IP, L2, METRICS, _bits, _randn, oracle_probed

f32 = np.float32
RC_EINVAL, RC_ESHAPE = -1, -2


# ------------------------------------------------------------------------------------------------------------ helpers
def _list_major(codes, cells, nlist):
    """numpy codes [N, D] in corpus order and their cells -> (xb, list_off, ids) of a list-major store (stable sort)."""
    order = np.argsort(cells, kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(cells, minlength=nlist))]).astype(np.int64)
    return codes[order], off, order.astype(np.int64)


def _stride(cells, probes, nlist):
    sizes = np.bincount(cells, minlength=nlist)
    return (max(4, int(sizes[probes].sum(1).max())) + 3) // 4 * 4


def _codes_in_corpus_order(index):
    codes = np.empty((index.ntotal, index.d), np.int8)
    codes[index.ids.cpu().numpy()] = index.xb.cpu().numpy()
    return codes


def _decoded(index):
    """The numpy-decoded rows of the index in corpus order, from the codes it holds and its own step / mid."""
    return sq8_decode(_codes_in_corpus_order(index), index.step.cpu().numpy(), index.mid.cpu().numpy())


def _int8_index(D, nlist, metric, x, cells=None, dev=DEV):
    """An int8 index over the rows x: zero coarse centroids and the given cells, or trained and filled by `add`."""
    import torch
    from repconc_amd.ivf_flat import IVFFlatIndex
    index = IVFFlatIndex(D, nlist, device=dev, metric=metric, storage="int8")
    if cells is None:
        index.train(x)
        index.add(x)
    else:
        index.set_coarse(torch.zeros(nlist, D))
        index.train_sq(x)
        index.set_lists(x, cells)
    return index


# --------------------------------------------------------------------------------------------------------------- CPU
def test_int8_storage_constructs_and_refuses_what_it_cannot_serve_without_a_gpu():
    import torch
    from repconc_amd import ops
    from repconc_amd.ivf_flat import IVFFlatIndex
    index = IVFFlatIndex(8, 4, device="cpu", storage="int8")
    assert index.storage == "int8" and index.xb.dtype == torch.int8 and index.ntotal == 0 and not index.is_trained
    for storage in ("bfloat16", "int4", "uint8"):
        with pytest.raises(ValueError, match="storage"):
            IVFFlatIndex(8, 4, device="cpu", storage=storage)
    with pytest.raises(ValueError, match="65536"):
        IVFFlatIndex(65537, 4, device="cpu", storage="int8")
    IVFFlatIndex(65537, 4, device="cpu")                                    # the other storages keep taking any d
    IVFFlatIndex(65536, 4, device="cpu", storage="int8")
    # the coarse centroids alone do not make it trained, and nothing works before the range exists
    index.set_coarse(torch.zeros(4, 8))
    assert not index.is_trained
    x = torch.randn(20, 8)
    for call in (lambda: index.add(x), lambda: index.set_lists(x, torch.zeros(20, dtype=torch.int64)),
                 lambda: index.search(x[:2], 3), lambda: index.reconstruct_n(0, 0),
                 lambda: index._search_probes(x[:2], torch.zeros(2, 1, dtype=torch.int32), 3)):
        with pytest.raises(ValueError, match="train_sq"):
            call()
    assert index.ntotal == 0
    index.train_sq(x)
    assert index.is_trained
    with pytest.raises(ValueError, match="int8"):
        IVFFlatIndex(8, 4, device="cpu").train_sq(x)                        # no range to train for a float store
    with pytest.raises(ValueError, match="vectors"):
        index.train_sq(torch.zeros(5, 7))
    with pytest.raises(ValueError, match="no rows"):
        index.train_sq(torch.zeros(0, 8))
    with pytest.raises(ValueError, match="finite"):
        index.train_sq(torch.full((3, 8), float("nan")))
    # the range without the centroids is not enough either
    other = IVFFlatIndex(8, 4, device="cpu", storage="int8")
    other.train_sq(x)
    assert not other.is_trained
    with pytest.raises(ValueError, match="train"):
        other.add(x)
    # an empty trained index answers with padding, without a launch
    s, i = index.search(x[:3], 4)
    assert bool((s == float("-inf")).all()) and bool((i == -1).all())


def test_shim_class_refuses_other_quantisers_and_residuals_and_is_exported():
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        import faiss
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))
    import repconc_amd.faiss_compat as fc
    from repconc_amd.index import METRIC_L2
    from repconc_amd.ivf_flat import IVFFlatIndex
    assert faiss.IndexIVFScalarQuantizer is fc.IndexIVFScalarQuantizer and issubclass(fc.IndexIVFScalarQuantizer, IVFFlatIndex)
    QT = fc.ScalarQuantizer
    for qtype in (QT.QT_4bit, QT.QT_8bit_uniform, QT.QT_fp16, QT.QT_8bit_direct, QT.QT_6bit):
        with pytest.raises(ValueError, match="QT_8bit"):
            fc.IndexIVFScalarQuantizer(None, 8, 4, qtype, METRIC_L2, False)
    with pytest.raises(ValueError, match="by_residual=False"):
        fc.IndexIVFScalarQuantizer(None, 8, 4, QT.QT_8bit, METRIC_L2)       # Faiss's default: residual encoding
    with pytest.raises(ValueError, match="by_residual=False"):
        fc.IndexIVFScalarQuantizer(None, 8, 4)
    with pytest.raises(ValueError, match="metric"):
        fc.IndexIVFScalarQuantizer(None, 8, 4, QT.QT_8bit, 7, False)
    quant = fc.IndexFlatL2(8, device="cpu")
    index = fc.IndexIVFScalarQuantizer(quant, 8, 4, QT.QT_8bit, by_residual=False)
    assert index.storage == "int8" and index.metric_type == METRIC_L2 and not index.is_trained and index.by_residual is False
    assert index.device.type == "cpu" and index.quantizer is quant
    with pytest.raises(ValueError, match="width"):
        fc.IndexIVFScalarQuantizer(quant, 9, 4, QT.QT_8bit, by_residual=False)
    # IndexIVFFlat keeps its storage
    assert fc.IndexIVFFlat._STORAGE == "float32"


def test_ops_and_raw_abi_refuse_bad_arguments_without_a_gpu():
    import torch
    from repconc_amd import _lib, ops
    N, D, nq = 10, 16, 3
    x8, dec, q = torch.zeros(N, D, dtype=torch.int8), torch.ones(2, D), torch.zeros(nq, D)
    off, ids = torch.tensor([0, 4, 10]), torch.arange(N)
    pr = torch.zeros(nq, 1, dtype=torch.int32)
    bad = [
        (dict(xb8=x8.float()), "int8"), (dict(xb8=x8.to(torch.uint8)), "int8"), (dict(xb8=x8[0]), "same D"),
        (dict(q=q[:, :8]), "same D"), (dict(q=q.double()), "float32"), (dict(q=q.half()), "float32"),
        (dict(dec=dec[:1]), "dec"), (dict(dec=dec.double()), "dec"), (dict(dec=torch.ones(2, D + 1)), "dec"),
        (dict(dec=torch.ones(2 * D)), "dec"),
        (dict(list_off=off.int()), "list_off"), (dict(list_off=torch.zeros(1, dtype=torch.int64)), "list_off"),
        (dict(ids=ids.int()), "ids"), (dict(ids=ids[:5]), "ids"),
        (dict(probes=pr.long()), "probes"), (dict(probes=pr[:2]), "probes"), (dict(probes=torch.zeros(nq, 3, dtype=torch.int32)), "probes"),
        (dict(k=0), "k must be"), (dict(k=8193), "k must be"), (dict(stride=0), "stride"), (dict(metric=2), "metric"),
        (dict(xb8=torch.zeros(0, D, dtype=torch.int8), ids=ids[:0]), "N"),
    ]
    for change, match in bad:
        kw = dict(xb8=x8, dec=dec, list_off=off, ids=ids, q=q, probes=pr, stride=8, k=2, metric=0)
        kw.update(change)
        with pytest.raises(ValueError, match=match):
            ops.ivf_flat_sq8_search(**kw)
    wide = torch.zeros(2, 65537, dtype=torch.int8)
    with pytest.raises(ValueError, match="65536"):
        ops.ivf_flat_sq8_search(wide, torch.ones(2, 65537), torch.tensor([0, 2]), torch.arange(2), torch.zeros(1, 65537),
                                torch.zeros(1, 1, dtype=torch.int32), 4, 1)
    with pytest.raises(_lib.RepconcHipError, match="GPU only"):             # valid arguments on the CPU: loud, as every op
        ops.ivf_flat_sq8_search(x8, dec, off, ids, q, pr, 8, 2)
    # ivf_flat_search keeps refusing everything but fp32 / fp16 stores
    with pytest.raises(ValueError, match="float32 or float16"):
        ops.ivf_flat_search(x8, off, ids, q, pr, 8, 2)
    # the raw entry: the width limit is a shape error and comes first, null pointers are RC_EINVAL
    lib = _lib.load()
    z = None
    call = lambda D_, ldx, k=2, nprobe=1: lib.rc_ivf_flat_sq8_search(z, z, ldx, z, z, N, 2, D_, z, nq, z, z, nprobe, 8, k, 0, z, z, z,
                                                                    z, z, 0, z)
    assert call(65537, 65537) == RC_ESHAPE
    assert call(65536, 65536) == RC_EINVAL and call(D, D) == RC_EINVAL
    assert call(D, D, k=0) == RC_EINVAL and call(D, D - 1) == RC_EINVAL and call(D, D, nprobe=3) == RC_EINVAL


def test_int8_build_side_equals_the_codec_definition_on_the_cpu_device():
    """set_coarse + train_sq + set_lists on the CPU device (torch operators) against the numpy restatement of the codec: range,
    step, mid, the stored codes read back in corpus order, a constant dimension, clamping outside the range, refusal of
    non-finite rows with nothing stored, reset keeps the range; and FlatSQ8Index trained on the same rows holds the same."""
    import torch
    from repconc_amd.dense_index import FlatSQ8Index, sq8_encode as enc, sq8_train_range
    from repconc_amd.ivf_flat import IVFFlatIndex
    rng = np.random.default_rng(12)
    D, N, nlist = 24, 500, 7
    x = (rng.standard_normal((N, D)) * (1.0 + np.arange(D))).astype(f32)
    x[:, 5] = 3.25                                                          # a constant dimension
    cells = rng.integers(0, nlist, N)
    vmin, step, mid = sq8_train(x)
    assert step[5] == 0 and mid[5] == f32(3.25)
    index = IVFFlatIndex(D, nlist, device="cpu", storage="int8")
    index.set_coarse(torch.zeros(nlist, D))
    index.train_sq(x)
    assert index.is_trained
    assert np.array_equal(index.vmin.numpy(), vmin) and np.array_equal(index.step.numpy(), step)
    assert np.array_equal(index.mid.numpy(), mid) and np.array_equal(index._dec.numpy(), np.stack([step, mid]))
    index.set_lists(x, cells)
    want = sq8_encode(x, vmin, step)
    assert index.ntotal == N and index.xb.dtype == torch.int8
    assert np.array_equal(_codes_in_corpus_order(index), want)
    wxb, woff, wids = _list_major(want, cells, nlist)
    assert np.array_equal(index.xb.numpy(), wxb) and index.list_off.tolist() == woff.tolist() and index.ids.tolist() == wids.tolist()
    assert want.min() == -128 and want.max() == 127 and (want[:, 5] == -128).all()
    # the flat int8 index trained on the same rows: the same range and the same codes (one codec)
    flat = FlatSQ8Index(D, device="cpu")
    flat.train(x)
    flat.add(x)
    assert torch.equal(flat._dec, index._dec) and torch.equal(flat.vmin, index.vmin)
    assert np.array_equal(flat.xb.numpy(), want)
    v2, d2 = sq8_train_range(torch.from_numpy(x), "cpu")
    assert torch.equal(v2, index.vmin) and torch.equal(d2, index._dec)
    assert torch.equal(enc(torch.from_numpy(x), v2, d2[0]), torch.from_numpy(want))
    # values outside the trained range clamp
    out = np.vstack([x.min(0) - 100.0, x.max(0) + 100.0, x[0]]).astype(f32)
    index.set_lists(out, np.array([3, 3, 0]))
    got = _codes_in_corpus_order(index)
    keep = np.arange(D) != 5
    assert (got[0] == -128).all() and (got[1][keep] == 127).all() and got[1][5] == -128 and np.array_equal(got[2], want[0])
    # a non-finite row is refused and nothing is stored
    index.set_lists(x, cells)
    before = (index.xb.clone(), index.ids.clone(), index.list_off.clone())
    for bad in (np.nan, np.inf, -np.inf):
        rows = x[:3].copy()
        rows[1, 7] = bad
        with pytest.raises(ValueError, match="finite"):
            index.set_lists(rows, np.array([0, 1, 2]))
        assert index.ntotal == N and all(torch.equal(a, b) for a, b in zip(before, (index.xb, index.ids, index.list_off)))
    # a new range under stored codes would change what they mean
    with pytest.raises(ValueError, match="reset"):
        index.train_sq(x)
    index.reset()
    assert index.ntotal == 0 and index.is_trained and np.array_equal(index.step.numpy(), step) and index.xb.shape == (0, D)
    # reconstruct_n of a float store on the CPU device: the stored rows in corpus order
    plain = IVFFlatIndex(D, nlist, device="cpu")
    plain.set_coarse(torch.zeros(nlist, D))
    plain.set_lists(x, cells)
    assert np.array_equal(plain.reconstruct_n(0, N).numpy(), x) and np.array_equal(plain.reconstruct_n(17, 5).numpy(), x[17:22])
    with pytest.raises(ValueError, match="outside"):
        plain.reconstruct_n(N - 2, 3)


# --------------------------------------------------------------------------------------------------------------- GPU
@functools.lru_cache(maxsize=None)
def _constructed(D):
    """tests/test_ivf_flat.py's constructed cells: N = 3000 rows in 12 cells of sizes 0, 1, 127, 128, 129, 0, 700, 15, 16, 17, 0
    and the rest, under shuffled corpus ids; 43 queries (40 probing cells 6 + 4, one two empty cells, one the 1-row cell and an
    empty one, one cells 11 + 2: four row chunks of the scan)."""
    import torch
    N = 3000
    sizes = CELL_SIZES + [N - sum(CELL_SIZES)]
    rng = np.random.default_rng(300 + D)
    cells = np.repeat(np.arange(12), sizes)[rng.permutation(N)]
    x, q = _randn((N, D), 207 + D) * 3.0, _randn((43, D), 208 + D)
    probes = np.array([[6, 4]] * 40 + [[0, 5], [1, 10], [11, 2]], dtype=np.int32)
    return x, q, torch.from_numpy(cells), cells, probes


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", (1, 5, 16, 17, 40, 48))
def test_constructed_cells_match_the_chain_over_the_decoded_rows(D, metric):
    """D = 16, 48: rows of whole 16-byte pieces (the vector path); the others the byte path with a partial last chunk."""
    import torch
    from repconc_amd import ops
    x, q, cells_t, cells, probes = _constructed(D)
    index = _int8_index(D, 12, metric, x, cells_t)
    assert index.ntotal == 3000 and index.xb.dtype == torch.int8
    vmin, step, mid = sq8_train(x.cpu().numpy())
    assert np.array_equal(index.step.cpu().numpy(), step) and np.array_equal(index.mid.cpu().numpy(), mid)
    xhat = _decoded(index)
    assert np.array_equal(index.reconstruct_n(0, 3000).cpu().numpy().view(np.uint32), xhat.view(np.uint32))
    assert np.array_equal(index.reconstruct_n(100, 7).cpu().numpy().view(np.uint32), xhat[100:107].view(np.uint32))
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
@pytest.mark.parametrize("D", (16, 40))
def test_strained_value_families_match_the_chain(D, metric):
    """The rows and ranges of tests/test_dense_sq8.py's families in the constructed cells: codes at both extremes, a constant
    dimension (step = 0), steps of 1e-22, mids of 1e4, one dominant query component, a zero query — what strains the decode's
    single rounding.  The 32 rows of a family are dealt over the 3000 positions, so equal rows meet in and across cells."""
    import torch
    from repconc_amd import ops
    _, _, _, cells, probes = _constructed(D)
    rng = np.random.default_rng(77 + D)
    pick, qpick = rng.integers(0, 32, 3000), np.arange(43) % 8
    stride = _stride(cells, probes, 12)
    pt = torch.from_numpy(np.sort(probes, axis=1)).to(DEV)                  # the op takes a query's probes in ascending order
    for name, q8, c32, step, mid in families(D):
        codes, q = c32[pick], q8[qpick]
        xb, off, ids = _list_major(codes, cells, 12)
        want = oracle_probed(sq8_decode(codes, step, mid), q, cells, probes, metric)
        args = (torch.from_numpy(xb).to(DEV), torch.from_numpy(np.stack([step, mid])).to(DEV), torch.from_numpy(off).to(DEV),
                torch.from_numpy(ids).to(DEV), torch.from_numpy(q).to(DEV), pt, stride)
        for k in (1, 100, 900):
            s, i, status, qstatus = ops.ivf_flat_sq8_search(*args, k, metric=metric)
            assert int(status.item()) == 0 and not bool(qstatus.any()), name
            try:
                assert_matches((s, i), cut(want, k, metric))
            except AssertionError as e:
                raise AssertionError(f"family {name!r}, k = {k}: {e}") from e


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("pitch,shift", ((80, 0), (72, 0), (80, 1), (64, 0)))
def test_a_column_slice_of_a_wider_matrix_is_read_in_place(pitch, shift, metric):
    """D = 64: pitch 80 and 64 keep the 16-byte loads, pitch 72 and a base offset by one byte take the byte path."""
    import torch
    from repconc_amd import ops
    D, N, k = 64, 1500, 20
    rng = np.random.default_rng(400 + pitch + shift)
    codes = rng.integers(-128, 128, (N, D)).astype(np.int8)
    step, mid = (rng.random(D) * 0.1 + 0.01).astype(f32), rng.standard_normal(D).astype(f32)
    cells = rng.integers(0, 4, N)
    q = rng.standard_normal((9, D)).astype(f32)
    probes = np.array([[1, 3]] * 8 + [[0, 2]], dtype=np.int32)
    xb, off, ids = _list_major(codes, cells, 4)
    wide = torch.from_numpy(rng.integers(-128, 128, (N, pitch + shift)).astype(np.int8)).to(DEV)
    wide[:, shift:shift + D] = torch.from_numpy(xb).to(DEV)
    view = wide[:, shift:shift + D]
    assert view.stride(0) == pitch + shift and view.data_ptr() % 16 == (shift % 16)
    want = oracle_probed(sq8_decode(codes, step, mid), q, cells, probes, metric)
    s, i, status, _ = ops.ivf_flat_sq8_search(view, torch.from_numpy(np.stack([step, mid])).to(DEV), torch.from_numpy(off).to(DEV),
                                              torch.from_numpy(ids).to(DEV), torch.from_numpy(q).to(DEV),
                                              torch.from_numpy(probes).to(DEV), _stride(cells, probes, 4), k, metric=metric)
    assert int(status.item()) == 0
    assert_matches((s, i), cut(want, k, metric))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_a_cell_longer_than_the_scan_grid_is_walked_by_striding_blocks(metric):
    """One cell of 5100 rows of N = 5300: more row chunks than the scan deals blocks to, so a block takes a second chunk."""
    import torch
    D, N = 5, 5300
    x, q = _randn((N, D), 231), _randn((3, D), 232)
    cells = np.where(np.arange(N) % 53 == 0, 0, np.where(np.arange(N) % 53 == 1, 2, 1))
    index = _int8_index(D, 3, metric, x, torch.from_numpy(cells))
    probes = np.array([[1, 2], [0, 1], [0, 2]], dtype=np.int32)
    want = oracle_probed(_decoded(index), q.cpu().numpy(), cells, probes, metric)
    for k in (7, 5200):
        assert_matches(index._search_probes(q, torch.from_numpy(probes), k), cut(want, k, metric))
    assert index.last_search_stats["fallback_queries"] == 0


@functools.lru_cache(maxsize=None)
def _corpus(N, D, nq, seed):
    return _randn((N, D), seed), _randn((nq, D), seed + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("D", (768, 100))
def test_probing_every_cell_equals_the_flat_index(D, metric):
    """Inner product: FlatSQ8Index trained on the same rows; L2: FlatL2Index over reconstruct_n(0, N) — the exact L2 search over
    int8 codes.  D = 768: 16-byte pieces; D = 100: the byte path."""
    from repconc_amd.dense_index import FlatIPIndex, FlatL2Index, FlatSQ8Index
    N, nlist = 20000, 16
    x, q = _corpus(N, D, 50, 540 + D)
    index = _int8_index(D, nlist, metric, x)
    assert index.ntotal == N and index.is_trained
    rec = index.reconstruct_n(0, N)
    if metric == IP:
        flat = FlatSQ8Index(D, device=DEV)
        flat.train(x)
        flat.add(x)
        assert np.array_equal(_codes_in_corpus_order(index), flat.xb.cpu().numpy())
        assert np.array_equal(flat.reconstruct_n(0, N).cpu().numpy().view(np.uint32), rec.cpu().numpy().view(np.uint32))
        fp32 = FlatIPIndex(D, device=DEV)
    else:
        flat = fp32 = FlatL2Index(D, device=DEV)
    fp32.add(rec)
    for k in (10, 100):
        ws, wi = flat.search(q, k)
        got = index.search(q, k, nprobe=nlist)
        assert_matches(got, (ws.cpu().numpy(), wi.cpu().numpy()))
        assert index.last_search_stats == {"queries": 50, "fallback_queries": 0, "chunks": 1}
        if fp32 is not flat:                                                # and the fp32 flat index over the decoded rows
            ws, wi = fp32.search(q, k)
            assert_matches(got, (ws.cpu().numpy(), wi.cpu().numpy()))
    # a part of the cells: the fp32 flat index's own re-ranking of the ids in the probed cells
    import torch
    probes = index.probe(q, 3, ordered=False).cpu().numpy()
    cells = np.empty(N, np.int64)
    cells[index.ids.cpu().numpy()] = np.repeat(np.arange(nlist), np.diff(index.list_off.cpu().numpy()))
    lists = [np.nonzero(np.isin(cells, probes[j]))[0] for j in range(50)]
    width = max(len(v) for v in lists)
    assert 0 < width <= 16384
    cand = np.full((50, width), -1, np.int64)
    for j, v in enumerate(lists):
        cand[j, :len(v)] = v
    ws, wi = fp32.rerank(q, torch.from_numpy(cand).to(DEV), 100)
    assert_matches(index.search(q, 100, nprobe=3), (ws.cpu().numpy(), wi.cpu().numpy()))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_identical_code_rows_in_different_cells_take_the_lower_corpus_id(metric):
    """600 rows of one code row in three cells whose ascending cell order is not ascending id order; k cuts the group."""
    import torch
    D, N = 8, 1500
    x, q = _randn((N, D), 251), _randn((3, D), 252)
    x[:600] = (q[0] if metric == L2 else 2.0 * q[0])           # one row, the best for query 0 (the range covers it: it is trained on x)
    cells = np.empty(N, np.int64)
    cells[:200], cells[200:400], cells[400:600] = 3, 1, 2
    cells[600:] = np.random.default_rng(5).integers(0, 4, N - 600)
    index = _int8_index(D, 4, metric, x, torch.from_numpy(cells))
    codes = _codes_in_corpus_order(index)
    assert (codes[:600] == codes[0]).all()
    probes = np.array([[0, 1, 2, 3]] * 3, dtype=np.int32)
    want = oracle_probed(_decoded(index), q.cpu().numpy(), cells, probes, metric)
    assert sorted(want[0][1][:600].tolist()) == list(range(600))            # the inputs do what they are meant to
    for k in (300, 599, 601):
        got = index._search_probes(q, torch.from_numpy(probes), k)
        assert_matches(got, cut(want, k, metric))
        assert index.last_search_stats["fallback_queries"] == 0
    s, i = index._search_probes(q, torch.from_numpy(probes), 300)
    assert i[0].tolist() == list(range(300))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_more_ties_than_the_candidate_list_holds_take_the_exact_route(metric):
    """17 000 rows of one code row at the top of every query: more than 16384 probed rows tie at the 100th score, the status
    bit fires and every query is answered by the exact search over its decoded probed rows — the flat fp32 index's answer."""
    import torch
    from repconc_amd.dense_index import FlatIPIndex, FlatL2Index
    D, N, nq = 8, 20000, 5
    x = -_randn((N, D), 261).abs() - 0.5                       # every other row: negative components of magnitude >= 0.5
    x[1000:18000] = 0.0                                        # the group: one code row, the top of the range
    q = _randn((nq, D), 262).abs() * (0.01 if metric == L2 else 1.0)
    cells = torch.from_numpy(np.random.default_rng(6).integers(0, 4, N))
    index = _int8_index(D, 4, metric, x, cells)
    flat = (FlatL2Index if metric == L2 else FlatIPIndex)(D, device=DEV)
    flat.add(index.reconstruct_n(0, N))
    ws, wi = flat.search(q, 100)
    assert wi[:, 0].tolist() == [1000] * nq and wi[:, 99].tolist() == [1099] * nq          # the inputs do what they are meant to
    got = index.search(q, 100, nprobe=4)
    assert index.last_search_stats == {"queries": nq, "fallback_queries": nq, "chunks": 1}
    assert_matches(got, (ws.cpu().numpy(), wi.cpu().numpy()))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_add_in_parts_equals_one_set_lists_and_never_re_encodes(metric):
    import torch
    from repconc_amd.ivf import coarse_assign
    from repconc_amd.ivf_flat import IVFFlatIndex
    D, N = 64, 10000
    x, q = _corpus(N, D, 21, 270)
    one = _int8_index(D, 32, metric, x)
    parts = IVFFlatIndex(D, 32, device=DEV, metric=metric, storage="int8")
    parts.set_coarse(one.coarse)
    parts.train_sq(x)
    assert parts.is_trained
    parts.add(x[:7000])
    assert parts.ntotal == 7000
    held = _codes_in_corpus_order(parts)
    parts.add(x[7000:].cpu().numpy())
    assert np.array_equal(_codes_in_corpus_order(parts)[:7000], held)       # the codes held are re-sorted, not re-encoded
    given = IVFFlatIndex(D, 32, device=DEV, metric=metric, storage="int8")
    given.set_coarse(one.coarse)
    given.train_sq(x)
    given.set_lists(x, coarse_assign(x, one.coarse))
    assert one.ntotal == parts.ntotal == given.ntotal == N
    vmin, step, mid = sq8_train(x.cpu().numpy())
    assert np.array_equal(one.step.cpu().numpy(), step) and np.array_equal(one.mid.cpu().numpy(), mid)
    for other in (parts, given):
        assert torch.equal(other.list_off, one.list_off) and torch.equal(other.ids, one.ids) and torch.equal(other.xb, one.xb)
    for k, nprobe in ((10, 4), (200, 32)):
        ws, wi = one.search(q, k, nprobe=nprobe)
        for other in (parts, given):
            gs, gi = other.search(q, k, nprobe=nprobe)
            assert torch.equal(gi, wi) and torch.equal(_bits(gs), _bits(ws))
    bad = x[:4].clone()
    bad[2, 3] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        one.add(bad)
    assert one.ntotal == N
    # values outside the trained range clamp to the ends of the range
    one.add(torch.stack([x.amin(0) - 50.0, x.amax(0) + 50.0]))
    codes = _codes_in_corpus_order(one)
    assert one.ntotal == N + 2 and (codes[N] == -128).all() and (codes[N + 1] == 127).all()
    one.reset()
    assert one.ntotal == 0 and one.is_trained and np.array_equal(one.step.cpu().numpy(), step)
    s, i = one.search(q, 5)
    pad = float("inf") if metric == L2 else float("-inf")
    assert bool((s == pad).all()) and bool((i == -1).all())
    one.add(x[:100])                                                        # ids start again from 0
    assert one.ntotal == 100 and sorted(one.ids.tolist()) == list(range(100))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_chunked_search_equals_the_unchunked_one(metric):
    import torch
    from repconc_amd import ops
    from repconc_amd.ivf_flat import IVFFlatIndex
    D, N = 64, 10000
    x, _ = _corpus(N, D, 21, 270)
    q = _randn((50, D), 281)
    index = _int8_index(D, 32, metric, x)
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
    index = _int8_index(768, 16, L2, x)
    runs = [index.search(q, 100, nprobe=3) for _ in range(3)]
    for s, i in runs[1:]:
        assert torch.equal(i, runs[0][1]) and torch.equal(_bits(s), _bits(runs[0][0]))


@pytest.mark.gpu
def test_a_probe_outside_the_index_or_a_short_score_row_sets_status_bit_2():
    import torch
    from repconc_amd import ops
    D, N, k = 16, 1500, 10
    x, q = _randn((N, D), 311), _randn((9, D), 312)
    cells = np.random.default_rng(8).integers(0, 4, N)
    index = _int8_index(D, 4, IP, x, torch.from_numpy(cells))
    good = np.array([[1, 3]] * 9, dtype=np.int32)
    full = (int(np.bincount(cells).max()) * 2 + 3) // 4 * 4
    for probes, stride in (([[-1, 3]] * 9, full), ([[1, 4]] * 9, full), ([[1, 3]] * 4 + [[-1, 2]] + [[1, 3]] * 4, full),
                           (good.tolist(), 400), (good.tolist(), 100)):
        pt = torch.tensor(probes, dtype=torch.int32, device=DEV)
        _, _, status, _ = ops.ivf_flat_sq8_search(index.xb, index._dec, index.list_off, index.ids, q, pt, stride, k)
        assert int(status.item()) & 4, (probes[4], stride)
    want = oracle_probed(_decoded(index), q.cpu().numpy(), cells, good, IP)
    s, i, status, qstatus = ops.ivf_flat_sq8_search(index.xb, index._dec, index.list_off, index.ids, q,
                                                    torch.from_numpy(good).to(DEV), full, k)
    assert int(status.item()) == 0 and not bool(qstatus.any())
    assert_matches((s, i), cut(want, k, IP))


@pytest.mark.gpu
def test_refine_index_over_an_int8_ivf_base_returns_the_fp32_flat_top_k():
    from repconc_amd.dense_index import FlatIPIndex
    from repconc_amd.refine_index import RefineIndex
    N, D, k, k_factor, nq = 5000, 64, 10, 50, 20
    x, q = _randn((N, D), 291), _randn((nq, D), 292)
    flat = FlatIPIndex(D, device=DEV)
    flat.add(x)
    ws, wi = flat.search(q, k)
    base = _int8_index(D, 16, IP, x)
    decoded = FlatIPIndex(D, device=DEV)
    decoded.add(base.reconstruct_n(0, N))
    _, ci = decoded.search(q, k * k_factor)
    inside = np.array([set(wi[j].tolist()) <= set(ci[j].tolist()) for j in range(nq)])
    assert inside.all(), "the inputs must leave no query out: the fp32 top-10 lies inside the int8 top-500"
    refine = RefineIndex(base, flat, k_factor=k_factor)
    assert refine.ntotal == N and refine.d == D
    got = refine.search(q, k, nprobe=16)
    assert_matches(got, (ws.cpu().numpy(), wi.cpu().numpy()))


@pytest.mark.gpu
def test_shim_index_trains_adds_and_searches_under_the_l2_metric():
    import torch
    import repconc_amd.faiss_compat as fc
    from repconc_amd.index import METRIC_L2
    x, q = _randn((3000, 32), 297), _randn((9, 32), 298)
    quant = fc.IndexFlatL2(32)
    index = fc.IndexIVFScalarQuantizer(quant, 32, 8, fc.ScalarQuantizer.QT_8bit, METRIC_L2, by_residual=False)
    assert index.metric_type == METRIC_L2 and not index.is_trained and index.storage == "int8"
    index.train(x)
    assert index.is_trained and quant.ntotal == 8 and torch.equal(quant.xb, index.coarse)
    index.add(x)
    index.nprobe = 8
    flat = fc.IndexFlatL2(32)
    flat.add(index.reconstruct_n(0, 3000))
    ws, wi = flat.search(q, 10)
    assert_matches(index.search(q, 10), (ws.cpu().numpy(), wi.cpu().numpy()))
    again = fc.IndexIVFScalarQuantizer(quant, 32, 8, fc.ScalarQuantizer.QT_8bit, METRIC_L2, by_residual=False)
    assert again.coarse is not None and not again.is_trained                # the centroids come from the quantizer, the range is missing
    again.train(x)                                                          # ... and training sets the range alone
    assert again.is_trained and torch.equal(again.coarse, index.coarse) and torch.equal(again._dec, index._dec)
    again.add(x)
    again.nprobe = 8
    assert_matches(again.search(q, 10), (ws.cpu().numpy(), wi.cpu().numpy()))
