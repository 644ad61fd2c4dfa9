"""In-place subset search of the IVF-flat index: `IVFFlatIndex.search(x, k, params=SearchParameters(sel=...))`, the MAP form of
ivf_flat_scan_kernel (csrc/ivf_flat.hip), the rc_ivf_flat*_search_rows entries, ops.ivf_flat_search(rows=, sel_off=),
IVFFlatIndex._selection, selector.SearchParametersIVF and RefineIndex(params=).

The contract: with a selector the result is what an IVFFlatIndex with the same coarse centroids (and the same codec range) would
return if it held only the selected vectors, each under the cell it has here: the same probes, ids and score BITS equal, ties to
the lower corpus id, padding where the probed cells hold fewer than k selected rows.

Oracles, none of them the code under test:
  (a) the emulated chain of tests/test_ivf_flat.py (`oracle_probed`) with every unselected row moved to a cell nobody probes;
  (b) a second IVFFlatIndex built from the selected vectors alone (`set_coarse` + `set_lists`), searched by the plain route;
  (c) the flat indexes under the same selector, and ops.dense_search(_l2)(rows=) over reconstruct_n(0, ntotal) for the int8 forms.
"""
import functools

import numpy as np
import pytest

from test_dense_flat import assert_matches
from test_dense_rerank import cut
from test_ivf_flat import DEV, IP, L2, METRICS, _bits, _flat, _randn, _values, oracle_probed

STORES = ("float32", "float16", "int8", "int8r")           # int8r: storage="int8", by_residual=True


# ------------------------------------------------------------------------------------------------------------ helpers
def _index(store, D, nlist, metric, dev=DEV):
    from repconc_amd.ivf_flat import IVFFlatIndex
    storage = "int8" if store.startswith("int8") else store
    return IVFFlatIndex(D, nlist, device=dev, metric=metric, storage=storage, by_residual=store == "int8r")


def _filled(store, D, nlist, metric, coarse, train_rows, x, cells):
    """An index of this store with the given centroids, the codec range of `train_rows` (int8 forms) and the rows x under the
    cells given."""
    index = _index(store, D, nlist, metric)
    index.set_coarse(coarse)
    if store.startswith("int8"):
        index.train_sq(train_rows)
    index.set_lists(x, cells)
    return index


def _stored_values(index, store, x):
    """fp32 numpy [N, D]: the values the index scores for the corpus rows x."""
    if store.startswith("int8"):
        return index.reconstruct_n(0, index.ntotal).cpu().numpy()
    return _values(x, store)


def _query_values(q, store):
    return _values(q, "float16" if store == "float16" else "float32")


def _params(ids):
    from repconc_amd.selector import IDSelectorBatch, SearchParameters
    return SearchParameters(sel=IDSelectorBatch(ids))


def _brute_selection(ids_listmajor, list_off, member):
    """numpy: (rows, sel_off, sizes_desc) of a membership array over CORPUS ids, for a list-major store."""
    rows = np.array([r for r in range(len(ids_listmajor)) if member[ids_listmajor[r]]], dtype=np.int64)
    sel_off = np.array([int((rows < o).sum()) for o in list_off], dtype=np.int64)
    return rows, sel_off, np.sort(np.diff(sel_off))[::-1]


# --------------------------------------------------------------------------------------------------------------- CPU
def _cpu_index(N=400, D=8, nlist=7, seed=3):
    import torch
    from repconc_amd.ivf_flat import IVFFlatIndex
    g = torch.Generator().manual_seed(seed)
    index = IVFFlatIndex(D, nlist, device="cpu")
    index.set_coarse(torch.randn(nlist, D, generator=g))
    x = torch.randn(N, D, generator=g)
    index.add(x)
    return index, x, g


def test_selection_equals_a_numpy_brute_force_on_the_cpu_device():
    import torch
    from repconc_amd.selector import (IDSelectorBatch, IDSelectorBitmap, IDSelectorNot, IDSelectorRange)
    index, x, g = _cpu_index()
    N = index.ntotal
    ids_lm, off = index.ids.numpy(), index.list_off.numpy()
    rng = np.random.default_rng(5)
    some = rng.choice(N, 90, replace=False)
    bits = rng.integers(0, 256, (N + 7) // 8 - 3).astype(np.uint8)           # a bitmap shorter than the index: the tail is out
    bitmember = np.zeros(N, bool)
    for i in range(min(N, 8 * len(bits))):
        bitmember[i] = (bits[i >> 3] >> (i & 7)) & 1

    def member_of(ids):
        m = np.zeros(N, bool)
        m[[i for i in ids if 0 <= i < N]] = True
        return m

    cases = [
        (IDSelectorRange(37, 251), member_of(range(37, 251))),
        (IDSelectorRange(-5, N + 9), np.ones(N, bool)),                                             # the identity
        (IDSelectorBatch(np.concatenate([some, some[:20], [-3, N, N + 77]])), member_of(some)),      # repeats, foreign ids
        (IDSelectorBitmap(bits), bitmember),
        (IDSelectorNot(IDSelectorBatch(some)), ~member_of(some)),
        (IDSelectorBatch(np.zeros(0, np.int64)), np.zeros(N, bool)),                                 # empty
        (IDSelectorBatch([N + 1, -1]), np.zeros(N, bool)),                                           # only foreign ids: empty
    ]
    for sel, member in cases:
        rows, sel_off, sizes_desc = index._selection(sel)
        want_rows, want_off, want_sizes = _brute_selection(ids_lm, off, member)
        assert rows.dtype == torch.int64 and sel_off.dtype == torch.int64 and rows.is_contiguous() and sel_off.is_contiguous()
        assert rows.tolist() == want_rows.tolist(), type(sel).__name__
        assert bool((rows[1:] > rows[:-1]).all())
        assert sel_off.tolist() == want_off.tolist() and sel_off.shape == (index.nlist + 1,)
        assert isinstance(sizes_desc, np.ndarray) and sizes_desc.tolist() == want_sizes.tolist()
        # inside a cell the selected rows ascend by corpus id (the store is stably sorted)
        for c in range(index.nlist):
            seg = ids_lm[rows[sel_off[c]:sel_off[c + 1]].numpy()]
            assert np.all(np.diff(seg) > 0) and np.all((off[c] <= rows[sel_off[c]:sel_off[c + 1]].numpy()))
    # the cache: the same store gives the same objects; a grown index builds the selection again
    sel = IDSelectorNot(IDSelectorBatch(some))
    first = index._selection(sel)
    assert index._selection(sel)[0] is first[0] and index._selection(sel)[1] is first[1]
    index.add(torch.randn(50, index.d, generator=g))
    grown = index._selection(sel)
    assert grown[0] is not first[0] and grown[0].numel() == first[0].numel() + 50                    # Not(...) takes the new ids
    want_rows, want_off, _ = _brute_selection(index.ids.numpy(), index.list_off.numpy(),
                                              np.concatenate([~member_of(some), np.ones(50, bool)]))
    assert grown[0].tolist() == want_rows.tolist() and grown[1].tolist() == want_off.tolist()
    # another index of the same size does not reuse it (one entry per selector: the key moves to the other index)
    other, _, _ = _cpu_index(seed=4)
    assert other._selection(sel)[0] is not grown[0]
    again = index._selection(sel)
    assert again[0] is not grown[0] and again[0].tolist() == grown[0].tolist()                       # the key went to `other`


def test_ops_rows_argument_errors_are_value_errors_with_cpu_tensors_only():
    import torch
    from repconc_amd import ops
    index, x, _ = _cpu_index()
    N, nlist = index.ntotal, index.nlist
    q = torch.zeros(3, index.d)
    probes = torch.zeros(3, 2, dtype=torch.int32)
    probes[:, 1] = 1
    rows, sel_off, _ = index._selection(_params(np.arange(0, N, 3)).sel)

    def call(rows=None, sel_off=None, **kw):
        return ops.ivf_flat_search(index.xb, index.list_off, index.ids, q, probes, 64, 5, rows=rows, sel_off=sel_off, **kw)

    with pytest.raises(ValueError, match="come together"):
        call(rows=rows)
    with pytest.raises(ValueError, match="come together"):
        call(sel_off=sel_off)
    swapped = rows.clone()
    swapped[[4, 5]] = swapped[[5, 4]]
    with pytest.raises(ValueError, match="ascending"):
        call(swapped, sel_off)                                              # not ascending
    twice = rows.clone()
    twice[7] = twice[6]
    with pytest.raises(ValueError, match="ascending"):
        call(twice, sel_off)                                                # a repeated row
    past = rows.clone()
    past[-1] = N
    with pytest.raises(ValueError, match="ascending"):
        call(past, sel_off)                                                 # a row >= N
    with pytest.raises(ValueError, match="sel_off"):
        call(rows, sel_off[:-1])                                            # the wrong length
    with pytest.raises(ValueError, match="sel_off"):
        call(rows, sel_off.to(torch.int32))
    with pytest.raises(ValueError, match="int64"):
        call(rows.to(torch.int32), sel_off)
    # a row listed under the wrong cell: the first row of segment c + 1 moved into segment c
    c = next(c for c in range(nlist - 1) if sel_off[c + 2] > sel_off[c + 1])
    wrong = sel_off.clone()
    wrong[c + 1] += 1
    with pytest.raises(ValueError, match="segment"):
        call(rows, wrong)
    bad_end = sel_off.clone()
    bad_end[-1] -= 1
    with pytest.raises(ValueError, match="segment"):
        call(rows, bad_end)
    # the positional order did not move, and the coded forms take the same keywords
    with pytest.raises(ValueError, match="come together"):
        ops.ivf_flat_sq8_search(index.xb.to(torch.int8), torch.zeros(2, index.d), index.list_off, index.ids, q, probes, 64, 5,
                                rows=rows)
    with pytest.raises(ValueError, match="come together"):
        ops.ivf_flat_sq8r_search(index.xb.to(torch.int8), torch.zeros(2, index.d), index.coarse, index.list_off, index.ids, q,
                                 probes, 64, 5, sel_off=sel_off)
    with pytest.raises(TypeError):
        ops.ivf_flat_search(index.xb, index.list_off, index.ids, q, probes, 64, 5, 0, rows, sel_off)      # keyword only
    # a valid pair passes every check and only then meets "the searches are GPU only"
    from repconc_amd._lib import RepconcHipError
    with pytest.raises(RepconcHipError):
        call(rows, sel_off)


def test_rows_entries_are_exported_and_check_their_arguments_without_a_gpu():
    import ctypes
    from repconc_amd import _lib
    lib = _lib.load()
    RC_EINVAL, RC_ESHAPE = -1, -2
    z = None
    one = ctypes.c_void_p(16)                   # a non-null DATA pointer: never followed, the argument checks return first
    # The handle IS followed before any check: the entry's device guard reads h->device once a device exists.  So it is a zeroed
    # buffer longer than the handle's leading ints (device = 0: nothing to switch to), with or without a GPU.
    zeroed = ctypes.create_string_buffer(4096)
    handle = ctypes.cast(zeroed, ctypes.c_void_p)
    side = {"rc_ivf_flat_search_rows": (), "rc_ivf_flat_f16_search_rows": (), "rc_ivf_flat_sq8_search_rows": (one,),
            "rc_ivf_flat_sq8r_search_rows": (one, one, 16)}
    N, nlist, D = 1000, 8, 16
    for name, s in side.items():
        fn = getattr(lib, name)
        assert name in _lib.PROTOTYPES and name[:-5] in _lib.PROTOTYPES
        assert len(_lib.PROTOTYPES[name][1]) == len(_lib.PROTOTYPES[name[:-5]][1]) + 3

        def call(h=handle, N=N, k=10, rows=one, ns=5, sel_off=one):
            return fn(h, one, D, one, one, N, nlist, D, one, 4, *s, one, 2, 64, k, 0, one, one, one, one, one, 0, z, rows, ns,
                      sel_off)
        assert call(h=z) == RC_EINVAL                                       # the twin's checks come first ...
        assert call(k=8193, rows=z) == RC_ESHAPE
        assert call(N=1 << 32, ns=0) == RC_ESHAPE
        for kw in (dict(rows=z), dict(sel_off=z), dict(ns=0), dict(ns=-1), dict(ns=N + 1)):
            assert call(**kw) == RC_EINVAL, (name, kw)                      # ... then rows, sel_off and ns
    # (a call that passes these checks goes on to the workspace check: not made here, it would need a device)


def test_search_parameters_ivf_and_the_params_argument():
    import torch
    from repconc_amd.selector import IDSelectorBatch, SearchParameters, SearchParametersIVF
    p = SearchParametersIVF()
    assert isinstance(p, SearchParameters) and p.sel is None and p.nprobe is None
    sel = IDSelectorBatch([1, 2])
    p = SearchParametersIVF(sel=sel, nprobe=3)
    assert p.sel is sel and p.nprobe == 3
    with pytest.raises(ValueError):
        SearchParametersIVF(sel=[1, 2])
    with pytest.raises(ValueError):
        SearchParametersIVF(nprobe=0)
    index, x, _ = _cpu_index()
    q = torch.zeros(2, index.d)
    with pytest.raises(ValueError, match="params"):
        index.search(q, 3, params=sel)                                      # a selector is not a SearchParameters
    with pytest.raises(ValueError, match="params"):
        index._search_probes(q, torch.zeros(2, 1, dtype=torch.int32), 3, params=sel)
    # precedence of nprobe: the argument, then params.nprobe, then the attribute (seen through the probe call)
    seen = []

    class Probed(Exception):
        pass

    def probe(qd, nprobe, ordered=False):
        seen.append(nprobe)
        raise Probed

    index.probe = probe
    index.nprobe = 5
    for kwargs, want in ((dict(), 5), (dict(params=SearchParameters(sel=sel)), 5), (dict(params=SearchParametersIVF(nprobe=3)), 3),
                         (dict(nprobe=2, params=SearchParametersIVF(sel=sel, nprobe=3)), 2), (dict(nprobe=2), 2),
                         (dict(params=SearchParametersIVF(nprobe=1000)), index.nlist)):
        with pytest.raises(Probed):
            index.search(q, 3, **kwargs)
        assert seen[-1] == want, kwargs
    del index.probe
    # an empty index, no query and an empty selection answer without a launch: all padding
    s, i = index.search(q, 4, params=SearchParameters(sel=IDSelectorBatch([index.ntotal + 5])))
    assert s.shape == (2, 4) and bool((s == float("-inf")).all()) and bool((i == -1).all())
    assert index.last_search_stats == {"queries": 2, "fallback_queries": 0, "chunks": 0, "rows_selected": 0}
    s, i = index.search(torch.zeros(0, index.d), 4, params=SearchParameters(sel=sel))
    assert s.shape == (0, 4) and index.last_search_stats["rows_selected"] == 2
    index.reset()
    s, i = index.search(q.numpy(), 4, params=SearchParameters(sel=sel))
    assert isinstance(s, np.ndarray) and np.all(np.isinf(s)) and np.all(i == -1)
    assert index.last_search_stats["rows_selected"] == 0


def test_a_selector_reaches_the_ivf_flat_search():
    """Without the subset search `IVFFlatIndex.search` has no `params`: this call is a TypeError there."""
    import torch
    from repconc_amd.selector import IDSelectorRange, SearchParameters
    index, x, _ = _cpu_index()
    index.reset()
    s, i = index.search(torch.zeros(3, index.d), 2, params=SearchParameters(sel=IDSelectorRange(0, 5)))
    assert s.shape == (3, 2) and bool((i == -1).all())


def test_shims_export_search_parameters_ivf():
    import os
    import subprocess
    import sys
    from conftest import ROOT
    code = ("import faiss, repconc_amd.faiss_compat as fc, repconc_amd.selector as s\n"
            "assert faiss.SearchParametersIVF is fc.SearchParametersIVF is s.SearchParametersIVF\n"
            "assert issubclass(faiss.SearchParametersIVF, faiss.SearchParameters)\n"
            "p = faiss.SearchParametersIVF(sel=faiss.IDSelectorRange(0, 4), nprobe=7)\n"
            "assert p.nprobe == 7\n")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "compat"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_refine_index_refuses_params_for_a_base_that_takes_none():
    import torch
    from repconc_amd.dense_index import FlatIPIndex
    from repconc_amd.refine_index import RefineIndex

    class Base:                                 # the shape of PQIndex.search: no params
        ntotal = 0

        def search(self, x, k):
            raise AssertionError("not reached")

    with pytest.raises(ValueError, match="params"):
        RefineIndex(Base(), FlatIPIndex(8, device="cpu")).search(torch.zeros(1, 8), 1, params=_params([1]))


# --------------------------------------------------------------------------------------------------------------- GPU
SEL_SIZES = [0, 1, 511, 512, 513, 8 * 512 + 3]             # selected rows per cell; the last walks the striding y blocks
CELL_SIZES = [3, 2, 1022, 1024, 1026, 2 * (8 * 512 + 3) - 1]           # about twice as long: every other row is selected
SHAPES = [(s, 16) for s in STORES] + [("float32", 20), ("float16", 24), ("int8", 100), ("int8r", 100)]


@functools.lru_cache(maxsize=None)
def _constructed(D):
    """N = 11274 rows in 6 cells of CELL_SIZES under shuffled corpus ids; the selection takes every other row of a cell (by
    corpus id, the order inside a cell), none of cell 0; in the last cell that ends on the LAST ROW OF THE STORE.  9 queries."""
    import torch
    N = sum(CELL_SIZES)
    rng = np.random.default_rng(300 + D)
    cells = np.repeat(np.arange(6), CELL_SIZES)[rng.permutation(N)]
    selected = []
    for c in range(1, 6):
        selected.append(np.nonzero(cells == c)[0][::2])
    selected = np.sort(np.concatenate(selected))
    assert [int((cells[selected] == c).sum()) for c in range(6)] == SEL_SIZES
    assert selected.max() == np.nonzero(cells == 5)[0].max()             # the last row of the store is selected
    x, q = _randn((N, D), 17 + D), _randn((9, D), 18 + D)
    coarse = torch.from_numpy((rng.standard_normal((6, D)) * 0.5).astype(np.float32))
    return x, q, cells, selected, coarse


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("store, D", SHAPES, ids=[f"{s}-{d}" for s, d in SHAPES])
def test_constructed_cells_match_the_emulated_chain(store, D, metric):
    """D = 16: one K stage; 20 fp32 / 24 fp16 (a 48-byte row) / 100 int8: the element-wise paths.  9 queries of one cell: a task of
    8 and a task of 1."""
    import torch
    from repconc_amd.selector import IDSelectorBatch, SearchParameters
    x, q, cells, selected, coarse = _constructed(D)
    index = _filled(store, D, 6, metric, coarse, x, x, torch.from_numpy(cells))
    assert int(index.ids[-1]) == int(selected.max())
    params = SearchParameters(sel=IDSelectorBatch(selected))
    rows, sel_off, sizes_desc = index._selection(params.sel)
    assert np.diff(sel_off.cpu().numpy()).tolist() == SEL_SIZES and int(rows[-1]) == index.ntotal - 1
    masked = np.where(np.isin(np.arange(len(cells)), selected), cells, -1)      # an unselected row is in no probed cell
    xn, qn = _stored_values(index, store, x), _query_values(q, store)
    probes3 = np.array([[2, 4, 5], [1, 3, 5]] * 4 + [[0, 1, 5]], dtype=np.int32)
    for probes in (probes3, np.array([[0, 1, 2, 3, 4, 5]] * 9, dtype=np.int32)):
        want = oracle_probed(xn, qn, masked, probes, metric)
        pt = torch.from_numpy(probes).to(DEV)
        for k in (10, 5000):
            got = index._search_probes(q, pt, k, params=params)
            assert_matches(got, cut(want, k, metric))
            assert index.last_search_stats == {"queries": 9, "fallback_queries": 0, "chunks": 1, "rows_selected": sum(SEL_SIZES)}
    # one query of empty (0 selected) and 1-row cells
    got = index._search_probes(q[:1], torch.tensor([[0, 1]], dtype=torch.int32), 4, params=params)
    assert_matches(got, cut(oracle_probed(xn, qn[:1], masked, np.array([[0, 1]]), metric), 4, metric))
    assert int(got[1][0, 0]) == int(selected[cells[selected] == 1][0]) and bool((got[1][0, 1:] == -1).all())


@functools.lru_cache(maxsize=None)
def _clustered():
    """20 000 x 64 rows, 40 queries, 32 trained centroids and the cell of every row."""
    import torch
    from repconc_amd.ivf import coarse_assign, coarse_kmeans
    x, q = _randn((20000, 64), 401), _randn((40, 64), 402)
    coarse = coarse_kmeans(x, 32, 6, 1234)
    cells = coarse_assign(x, coarse)
    rng = np.random.default_rng(9)
    tenth = np.sort(rng.choice(20000, 2000, replace=False))
    half = np.sort(rng.choice(20000, 10000, replace=False))
    return x, q, coarse, cells, tenth, half


@functools.lru_cache(maxsize=None)
def _clustered_index(store, metric):
    x, q, coarse, cells, _, _ = _clustered()
    return _filled(store, 64, 32, metric, coarse, x, x, cells)


def _selections():
    from repconc_amd.selector import IDSelectorBatch, IDSelectorNot, IDSelectorRange
    _, _, _, _, tenth, half = _clustered()
    everything = np.arange(20000)
    return (("10%", IDSelectorBatch(tenth), tenth), ("50%", IDSelectorBatch(half), half),
            ("not 10%", IDSelectorNot(IDSelectorBatch(tenth)), np.setdiff1d(everything, tenth)),
            ("identity", IDSelectorRange(0, 20000), everything))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("store", STORES)
def test_equals_a_sub_index_of_the_selected_rows(store, metric):
    import torch
    from repconc_amd.selector import SearchParameters, SearchParametersIVF
    x, q, coarse, cells, _, _ = _clustered()
    index = _clustered_index(store, metric)
    for name, sel, kept in _selections():
        kept_t = torch.from_numpy(kept).to(DEV)
        sub = _filled(store, 64, 32, metric, coarse, x, x[kept_t], cells[kept_t])           # the range: the same training rows
        params = SearchParameters(sel=sel)
        for nprobe in (1, 4, 32):
            for k in (10, 1000):
                ws, wi = sub.search(q, k, nprobe=nprobe)
                wi = torch.where(wi >= 0, kept_t[wi.clamp(min=0)], wi)
                gs, gi = index.search(q, k, nprobe=nprobe, params=params)
                assert torch.equal(gi, wi) and torch.equal(_bits(gs), _bits(ws)), (name, nprobe, k)
                assert index.last_search_stats["rows_selected"] == len(kept) and index.last_search_stats["fallback_queries"] == 0
                if name == "identity":
                    ps, pi = index.search(q, k, nprobe=nprobe)
                    assert torch.equal(gi, pi) and torch.equal(_bits(gs), _bits(ps)), (nprobe, k)
                    assert "rows_selected" not in index.last_search_stats
        # nprobe of the params, numpy in and out
        gs, gi = index.search(q.cpu().numpy(), 10, params=SearchParametersIVF(sel=sel, nprobe=4))
        ws, wi = sub.search(q, 10, nprobe=4)
        assert_matches((gs, gi), (ws.cpu().numpy(), torch.where(wi >= 0, kept_t[wi.clamp(min=0)], wi).cpu().numpy()))
    # k = 1000 at nprobe = 1 under the 10 % selection: more than a probe set holds, the tail is padding
    gs, gi = index.search(q, 1000, nprobe=1, params=SearchParameters(sel=_selections()[0][1]))
    pad = float("inf") if metric == L2 else float("-inf")
    assert bool((gi[:, -1] == -1).all()) and bool((gs[:, -1] == pad).all()) and bool((gi[:, 0] >= 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("store", STORES)
def test_probing_every_cell_equals_the_flat_search_under_the_same_selector(store, metric):
    import torch
    from repconc_amd import ops
    from repconc_amd.selector import SearchParameters
    x, q, _, _, _, _ = _clustered()
    index = _clustered_index(store, metric)
    if store.startswith("int8"):
        recon = index.reconstruct_n(0, index.ntotal)
        flat = None
    else:
        flat = _flat(metric, store, 64)
        flat.add(x)
    for name, sel, kept in _selections():
        params = SearchParameters(sel=sel)
        for k in (10, 1000):
            if flat is None:
                ws, wi = (ops.dense_search_l2 if metric == L2 else ops.dense_search)(
                    recon, q, k, rows=sel.rows(index.ntotal, 0, index.device))
            else:
                ws, wi = flat.search(q, k, params=params)
            gs, gi = index.search(q, k, nprobe=32, params=params)
            assert torch.equal(gi, wi) and torch.equal(_bits(gs), _bits(ws)), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("storage", ("float32", "float16"))
@pytest.mark.parametrize("metric", METRICS)
def test_ties_go_to_the_lower_corpus_id_among_the_selected_rows(metric, storage):
    """600 copies of one row in three cells whose ascending cell order is not ascending id order; every third is selected."""
    import torch
    from repconc_amd.ivf_flat import IVFFlatIndex
    D, N = 8, 1500
    x, q = _randn((N, D), 51), _randn((3, D), 52)
    x[:600] = (q[0] if metric == L2 else 10.0 * q[0])
    cells = np.empty(N, np.int64)
    cells[:200], cells[200:400], cells[400:600] = 3, 1, 2
    cells[600:] = np.random.default_rng(5).integers(0, 4, N - 600)
    index = IVFFlatIndex(D, 4, device=DEV, metric=metric, storage=storage)
    index.set_coarse(torch.zeros(4, D))
    index.set_lists(x, torch.from_numpy(cells))
    selected = np.concatenate([np.arange(1, 600, 3), np.arange(600, N, 2)])
    params = _params(selected)
    masked = np.where(np.isin(np.arange(N), selected), cells, -1)
    probes = np.array([[0, 1, 2, 3]] * 3, dtype=np.int32)
    want = oracle_probed(_values(x, storage), _values(q, storage), masked, probes, metric)
    for k in (100, 199, 201):
        got = index._search_probes(q, torch.from_numpy(probes), k, params=params)
        assert_matches(got, cut(want, k, metric))
        assert index.last_search_stats["fallback_queries"] == 0
    s, i = index._search_probes(q, torch.from_numpy(probes), 100, params=params)
    assert i[0].tolist() == list(range(1, 300, 3))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("store", STORES)
def test_more_selected_ties_than_the_candidate_list_holds_take_the_exact_route(store, metric):
    """17 000 selected identical rows tie at the 100th score beside 17 000 UNSELECTED identical rows that score better: the status
    bit fires, the exact fall-back gathers the selected rows of the probed cells only, and no unselected id is returned."""
    import torch
    from repconc_amd import ops
    from repconc_amd.selector import IDSelectorNot, IDSelectorRange, SearchParameters
    D, N, nq = 8, 40000, 5
    x = -_randn((N, D), 61).abs() - 0.5
    x[:17000] = 1.0 if metric == IP else 0.25                          # unselected, better than ...
    x[20000:37000] = 0.0                                               # ... the selected group (int8: several steps apart)
    q = _randn((nq, D), 62).abs() * (0.01 if metric == L2 else 1.0) + (0.25 if metric == L2 else 0.0)
    cells = torch.from_numpy(np.random.default_rng(6).integers(0, 4, N))
    index = _filled(store, D, 4, metric, torch.zeros(4, D), x, x, cells)
    params = SearchParameters(sel=IDSelectorNot(IDSelectorRange(0, 17000)))
    rows_sel = params.sel.rows(N, 0, index.device)
    if store.startswith("int8"):
        recon = index.reconstruct_n(0, N)
        assert bool((recon[20000:37000] == recon[20000]).all()) and bool((recon[:17000] == recon[0]).all())
        plain = (ops.dense_search_l2 if metric == L2 else ops.dense_search)(recon, q, 1)
        ws, wi = (ops.dense_search_l2 if metric == L2 else ops.dense_search)(recon, q, 100, rows=rows_sel)
    else:
        flat = _flat(metric, store, D)
        flat.add(x)
        plain = flat.search(q, 1)
        ws, wi = flat.search(q, 100, params=params)
    assert plain[1][:, 0].tolist() == [0] * nq                          # the inputs do what they are meant to: without the
    assert wi[:, 0].tolist() == [20000] * nq and wi[:, 99].tolist() == [20099] * nq      # selector the unselected group wins
    gs, gi = index.search(q, 100, nprobe=4, params=params)
    assert index.last_search_stats["fallback_queries"] > 0
    assert index.last_search_stats == {"queries": nq, "fallback_queries": nq, "chunks": 1, "rows_selected": N - 17000}
    assert bool((gi >= 17000).all())
    assert torch.equal(gi, wi) and torch.equal(_bits(gs), _bits(ws))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_a_query_whose_probed_cells_hold_no_selected_row_is_all_padding(metric):
    import torch
    from repconc_amd import ops
    x, q, coarse, cells, _, _ = _clustered()
    index = _clustered_index("float32", metric)
    cells_n = cells.cpu().numpy()
    kept = np.nonzero(cells_n >= 3)[0]                                  # nothing of cells 0, 1, 2 is selected
    params = _params(kept)
    probes = np.array([[0, 1, 2], [0, 2, 5], [7, 8, 9]] * 3, dtype=np.int32)
    pt = torch.from_numpy(probes).to(DEV)
    s, i = index._search_probes(q[:9], pt, 10, params=params)           # status bit 2 would be a RuntimeError here
    pad = float("inf") if metric == L2 else float("-inf")
    for j in (0, 3, 6):
        assert bool((i[j] == -1).all()) and bool((s[j] == pad).all())
    assert bool((i[1] >= 0).all()) and set(cells_n[i[1].cpu().numpy()]) == {5}
    assert bool((i[2] >= 0).all()) and set(cells_n[i[2].cpu().numpy()]) <= {7, 8, 9}
    rows, sel_off, sizes_desc = index._selection(params.sel)
    stride = (int(sizes_desc[:3].sum()) + 3) // 4 * 4
    rs, ri, status, qstatus = ops.ivf_flat_search(index.xb, index.list_off, index.ids, q[:9], pt, stride, 10, metric=metric,
                                                  rows=rows, sel_off=sel_off)          # check_rows=True: the pair passes it
    assert int(status.item()) == 0 and not bool(qstatus.any())
    assert torch.equal(ri, i) and torch.equal(_bits(rs), _bits(s))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", METRICS)
def test_chunked_subset_search_equals_the_unchunked_one(metric):
    import torch
    from repconc_amd import ops
    from repconc_amd.ivf_flat import IVFFlatIndex
    x, q, coarse, cells, tenth, half = _clustered()
    index = _filled("float32", 64, 32, metric, coarse, x, x, cells)     # its own index: MAX_WS_BYTES is patched below
    params = _params(half)
    ws, wi = index.search(q, 50, nprobe=6, params=params)
    assert index.last_search_stats["chunks"] == 1
    sizes_desc = index._selection(params.sel)[2]
    stride = (max(4, int(sizes_desc[:6].sum())) + 3) // 4 * 4
    assert stride < (int(index._sizes_desc[:6].sum()) + 3) // 4 * 4     # the score rows follow the selection
    index.MAX_WS_BYTES = ops.ivf_flat_search_ws_bytes(13, 6, 32, stride)        # 13 queries per call: 40 go in four chunks
    gs, gi = index.search(q, 50, nprobe=6, params=params)
    assert index.last_search_stats == {"queries": 40, "fallback_queries": 0, "chunks": 4, "rows_selected": len(half)}
    assert torch.equal(gi, wi) and torch.equal(_bits(gs), _bits(ws))
    assert IVFFlatIndex.MAX_WS_BYTES == 4 << 30


@pytest.mark.gpu
def test_three_subset_runs_have_identical_bits():
    import torch
    x, q, _, _, tenth, _ = _clustered()
    index = _clustered_index("float16", L2)
    params = _params(tenth)
    runs = [index.search(q, 100, nprobe=8, params=params) for _ in range(3)]
    for s, i in runs[1:]:
        assert torch.equal(i, runs[0][1]) and torch.equal(_bits(s), _bits(runs[0][0]))


@pytest.mark.gpu
def test_refine_index_over_an_ivf_base_forwards_the_selector():
    import torch
    from repconc_amd.dense_index import FlatIPIndex
    from repconc_amd.refine_index import RefineIndex
    x, q, _, _, tenth, _ = _clustered()
    base = _clustered_index("float16", IP)
    flat = FlatIPIndex(64, device=DEV)
    flat.add(x)
    refine = RefineIndex(base, flat, k_factor=4)
    params = _params(tenth)
    s, i = refine.search(q, 20, nprobe=32, params=params)
    assert bool(torch.isin(i, torch.from_numpy(tenth).to(DEV)).all())
    ws, wi = flat.search(q, 20, params=params)
    # the fp16 base ranks 80 candidates of the selection, fp32 re-ranks them: the flat subset search's top 20 are among them
    assert torch.equal(i, wi) and torch.equal(_bits(s), _bits(ws))
    s, i = refine.search(q, 20, nprobe=2, params=params)
    assert bool(torch.isin(i[i >= 0], torch.from_numpy(tenth).to(DEV)).all())
