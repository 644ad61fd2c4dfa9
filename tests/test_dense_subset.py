"""Subset search of the flat dense indexes: `ops.dense_search*(rows=...)`, the selectors of `repconc_amd.selector` and
`index.search(x, k, params=SearchParameters(sel=...))`.

The definition under test: for an ascending, duplicate-free row list `rows`, a subset search returns exactly what the search of
the same variant returns over `x[rows]`, with every id i replaced by id_offset + rows[i] — ids AND score bits, the padding past
len(rows) included, on the fast route, the repeated queries and the exact route.  Every comparison is bit for bit against
  (a) the existing search of the variant over the materialised copy `x[rows].contiguous()` (its norms recomputed from the
      copy), ids mapped on the host, and
  (b) for small cases the numpy chain oracles of the suite (test_dense_flat.oracle_topk, test_dense_l2.oracle_topk_l2) over
      the selected rows.
No test hands the library a row list that is not valid (ascending, unique, in range); the invalid lists of the CPU tests are
refused by `check_rows` before the library is loaded.
"""
import numpy as np
import pytest
import torch

from repconc_amd.selector import (IDSelectorArray, IDSelectorBatch, IDSelectorBitmap, IDSelectorNot, IDSelectorRange,
                                  SearchParameters)
from test_dense_flat import assert_matches, oracle_topk
from test_dense_l2 import oracle_topk_l2
from test_search_arg_order import FLAT, SCORES
from test_search_arg_order import T as ORDER_T
from test_search_arg_order import VALUE as ORDER_VALUE
from test_search_arg_order import _check as check_order

SERVED = ("f32", "f16", "l2", "l2_f16")


def _variant(name):
    """(search, exact search, the store of fp32 rows, the variant's fp32 view of queries, numpy oracle, l2)"""
    from repconc_amd import ops
    half = name.endswith("f16")
    store = (lambda x: x.half()) if half else (lambda x: x)
    seen = (lambda t: t.half().float()) if half else (lambda t: t.float())
    if name in ("f32", "f16"):
        return (ops.dense_search_f16 if half else ops.dense_search, ops.dense_search_f16_exact if half else ops.dense_search_exact,
                store, seen, oracle_topk, False)
    return (ops.dense_search_l2_f16 if half else ops.dense_search_l2,
            ops.dense_search_l2_f16_exact if half else ops.dense_search_l2_exact, store, seen, oracle_topk_l2, True)


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_selectors_turn_external_ids_into_ascending_unique_rows_inside_the_index():
    n, off = 20, 100
    rows = lambda sel, ntotal=n, id_offset=off: sel.rows(ntotal, id_offset, "cpu").tolist()
    assert IDSelectorArray is IDSelectorBatch
    # Range: half-open, clipped to the index, empty when it misses it
    assert rows(IDSelectorRange(103, 107)) == [3, 4, 5, 6]
    assert rows(IDSelectorRange(90, 102)) == [0, 1] and rows(IDSelectorRange(118, 500)) == [18, 19]
    assert rows(IDSelectorRange(0, 100)) == [] and rows(IDSelectorRange(120, 130)) == [] and rows(IDSelectorRange(107, 103)) == []
    assert IDSelectorRange(103, 107).span(n, off) == (3, 7) and IDSelectorRange(0, 50).span(n, off) == (0, 0)
    # Batch: duplicates collapse, ids below id_offset and at or above id_offset + ntotal are ignored, any order and int type
    b = IDSelectorBatch(np.array([119, 105, 105, 99, 120, 100, 3, -1, 105], dtype=np.int32))
    assert rows(b) == [0, 5, 19]
    assert rows(IDSelectorBatch(torch.tensor([100, 119]))) == [0, 19] and rows(IDSelectorBatch(np.array([], np.int64))) == []
    assert rows(IDSelectorBatch([7, 8]), id_offset=0) == [7, 8] and rows(IDSelectorBatch(np.array([99, 120]))) == []
    # Bitmap, Faiss's layout: id i is bit i & 7 of byte i >> 3; a bitmap shorter than the index selects nothing past its end
    ids = [101, 108, 109, 115, 119]
    bits = np.zeros((15,), np.uint8)                                # ids 0 .. 119
    for i in ids:
        bits[i >> 3] |= 1 << (i & 7)
    bits[0] |= 1                                                     # id 0: below id_offset
    assert rows(IDSelectorBitmap(bits)) == [1, 8, 9, 15, 19]
    assert rows(IDSelectorBitmap(bits[:14])) == [1, 8, 9]           # ids 112 .. are past the bitmap
    assert rows(IDSelectorBitmap(bits), id_offset=0) == [0]         # only id 0 is below ntotal = 20
    assert rows(IDSelectorBitmap(np.zeros((0,), np.uint8))) == []
    # Not: over Batch, over Range, over Not
    assert rows(IDSelectorNot(b)) == [r for r in range(n) if r not in (0, 5, 19)]
    assert rows(IDSelectorNot(IDSelectorRange(0, 1000))) == [] and rows(IDSelectorNot(IDSelectorRange(0, 50))) == list(range(n))
    assert rows(IDSelectorNot(IDSelectorNot(b))) == [0, 5, 19]
    # every list: int64, contiguous, strictly ascending, inside [0, ntotal)
    for sel in (b, IDSelectorBitmap(bits), IDSelectorNot(b), IDSelectorRange(90, 111)):
        r = sel.rows(n, off, "cpu")
        assert r.dtype == torch.int64 and r.is_contiguous() and r.dim() == 1
        assert bool((r[1:] > r[:-1]).all()) and int(r[0]) >= 0 and int(r[-1]) < n
    # the cache: one list per (ntotal, id_offset, device), rebuilt when the index has grown
    grow = IDSelectorNot(IDSelectorBatch([100, 101]))
    first = grow.rows(4, off, "cpu")
    assert grow.rows(4, off, "cpu") is first and first.tolist() == [2, 3]
    assert grow.rows(6, off, "cpu").tolist() == [2, 3, 4, 5] and grow.rows(6, 101, "cpu").tolist() == [1, 2, 3, 4, 5]
    with pytest.raises(ValueError):
        SearchParameters(sel=[1, 2, 3])
    with pytest.raises(ValueError):
        IDSelectorBitmap(np.zeros((3,), np.int32))
    with pytest.raises(ValueError):
        IDSelectorBatch(np.zeros((3,), np.float32))
    assert SearchParameters().sel is None and SearchParameters(sel=b).sel is b


# ---- the two new kinds of ops._dense_call, position by position against orders written out by hand from the header
ROWS_T = dict(ORDER_T, rows=torch.zeros((9,), dtype=torch.int64))
ROWS_VALUE = dict(ORDER_VALUE, rows=ROWS_T["rows"].data_ptr(), ns=9)
assert len(set(ROWS_VALUE.values())) == len(ROWS_VALUE)          # no two arguments can stand in for each other
ROWS_ORDER = [
    ("_DENSE_F32",
     "rc_dense_search_rows_q",
     "h, x, ldx, N, D, q, nq, rows, ns, k, id_offset, sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream",
     "rc_dense_search_rows_exact", "h, x, ldx, N, D, q, nq, rows, ns, k, id_offset, scores, ids, ws, ws_bytes, stream"),
    ("_DENSE_F16",
     "rc_dense_f16_search_rows_q",
     "h, x, ldx, N, D, q, nq, xnorm_max, rows, ns, k, id_offset, sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream",
     "rc_dense_f16_search_rows_exact", "h, x, ldx, N, D, q, nq, rows, ns, k, id_offset, scores, ids, ws, ws_bytes, stream"),
    ("_DENSE_L2",
     "rc_dense_l2_search_rows_q",
     "h, x, ldx, N, D, q, nq, xsq, xnorm_max, rows, ns, k, id_offset, sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream",
     "rc_dense_l2_search_rows_exact", "h, x, ldx, N, D, q, nq, rows, ns, k, id_offset, scores, ids, ws, ws_bytes, stream"),
    ("_DENSE_L2_F16",
     "rc_dense_l2_f16_search_rows_q",
     "h, x, ldx, N, D, q, nq, xsq, xnorm_max, rows, ns, k, id_offset, sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream",
     "rc_dense_l2_f16_search_rows_exact", "h, x, ldx, N, D, q, nq, rows, ns, k, id_offset, scores, ids, ws, ws_bytes, stream"),
]


@pytest.mark.parametrize("variant, q_name, q_order, e_name, e_order", ROWS_ORDER, ids=[r[0] for r in ROWS_ORDER])
def test_rows_entries_argument_order(variant, q_name, q_order, e_name, e_order):
    from repconc_amd import _lib, ops
    v = getattr(ops, variant)
    H, STREAM, K, OFF, SLACK = (ORDER_VALUE[n] for n in ("h", "stream", "k", "id_offset", "sel_slack"))
    for kind, want_name, order in (("search_rows_q", q_name, q_order), ("search_rows_exact", e_name, e_order)):
        name, args = ops._dense_call(v, kind, H, ROWS_T["x"], ROWS_T["q"], ROWS_T, STREAM, K, OFF, SLACK)
        assert name == want_name
        assert [getattr(a, "value", a) for a in args] == [ROWS_VALUE[n] for n in order.split(", ")], name
        assert len(args) == len(_lib.PROTOTYPES[name][1]), name


def test_the_three_old_kinds_of_dense_call_are_unchanged_for_all_eight_variants():
    """With a "rows" entry in the table or without: the hand-written orders of tests/test_search_arg_order.py."""
    from repconc_amd import ops
    H, STREAM, K, OFF, SLACK = (ORDER_VALUE[n] for n in ("h", "stream", "k", "id_offset", "sel_slack"))
    assert len(FLAT) == 8
    for t in (ORDER_T, ROWS_T):
        for variant, q_name, q_order, e_name, e_order in FLAT:
            v = getattr(ops, variant)
            check_order(*ops._dense_call(v, "search_q", H, t["x"], t["q"], t, STREAM, K, OFF, SLACK), q_name, q_order)
            check_order(*ops._dense_call(v, "search_exact", H, t["x"], t["q"], t, STREAM, K, OFF), e_name, e_order)
        for variant, name, order in SCORES:
            v = getattr(ops, variant)
            tt = {n: t[n] for n in t if n != "ws" or v.scores_ws}
            check_order(*ops._dense_call(v, "scores", H, tt["x"], tt["q"], tt, STREAM), name, order)


def test_check_rows_refuses_an_invalid_list_before_the_library_is_loaded(monkeypatch):
    from repconc_amd import _lib, ops

    def reached(*a, **k):
        pytest.fail("the library was reached with an invalid row list")
    monkeypatch.setattr(_lib, "load", reached)
    monkeypatch.setattr(_lib, "handle", reached)
    N, D = 10, 16
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64)
    bad = {
        "unsorted": i64(1, 5, 3),
        "repeated": i64(1, 3, 3, 7),
        "minus one": i64(-1, 2, 4),
        "N": i64(2, 4, N),
        "int32": torch.tensor([1, 2, 3], dtype=torch.int32),
        "non-contiguous": torch.arange(0, 10, dtype=torch.int64)[::2],
        "two-dimensional": torch.zeros((2, 2), dtype=torch.int64),
        "more rows than the corpus": torch.arange(0, N + 1, dtype=torch.int64),
    }
    assert not bad["non-contiguous"].is_contiguous()
    fronts = []
    for name in SERVED:
        search, exact, store, _, _, _ = _variant(name)
        fronts += [(search, store), (exact, store)]
    for what, rows in bad.items():
        for fn, store in fronts:
            with pytest.raises(ValueError):
                fn(store(torch.zeros(N, D)), torch.zeros(2, D), 1, rows=rows)
    # the variants that serve no subset search take no such keyword at all
    for fn in (ops.dense_search_bf16x3, ops.dense_search_l2_bf16x3):
        with pytest.raises(TypeError):
            fn(torch.zeros(N, D), torch.zeros(2, D), 1, rows=i64(1, 2))
    for fn in (ops.dense_search_sq8, ops.dense_search_l2_sq8):
        with pytest.raises(TypeError):
            fn(torch.zeros((N, D), dtype=torch.int8), torch.zeros(2, D), torch.zeros(2, D), 1, rows=i64(1, 2))
    with pytest.raises(ValueError):
        ops._dense_search(ops._DENSE_BF16X3, torch.zeros(N, D), torch.zeros(2, D), 1, 0, None, False, "auto", 2, rows=i64(1, 2))


def test_rows_entries_shape_and_pointer_checks_need_no_gpu():
    from repconc_amd import _lib
    from repconc_amd.dense_index import (FlatIPIndex, FlatL2Bf16x3Index, FlatL2F16Index, FlatL2Index, FlatL2SQ8Index,
                                         FlatSQ8Index)
    lib = _lib.load()
    N, D = 1000, 16
    RC_ESHAPE, RC_EINVAL = -2, -1
    z = None
    side = {"dense": (), "dense_f16": (z,), "dense_l2": (z, z), "dense_l2_f16": (z, z)}
    for entry, s in side.items():
        rows_q = getattr(lib, f"rc_{entry}_search_rows_q")
        rows_exact = getattr(lib, f"rc_{entry}_search_rows_exact")
        for ns in (0, N + 1, 5):              # ns = 0, ns = N + 1, and a fine ns with rows == NULL (every pointer is)
            assert rows_q(z, z, D, N, D, z, 4, *s, z, ns, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_EINVAL
            assert rows_exact(z, z, D, N, D, z, 4, z, ns, 10, 0, z, z, z, 0, z) == RC_EINVAL
        # the shape limits come first, as in the entries without rows
        assert rows_q(z, z, D, N, D, z, 4, *s, z, 0, 8193, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
        assert rows_q(z, z, D, 1 << 32, D, z, 4, *s, z, 5, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
        assert rows_exact(z, z, D, N, D, z, 4, z, N + 1, 8193, 0, z, z, z, 0, z) == RC_ESHAPE
        assert rows_exact(z, z, D, 1 << 32, D, z, 4, z, 5, 10, 0, z, z, z, 0, z) == RC_ESHAPE
    # the indexes that serve no subset search say so, by name, before any device work (they hold nothing, on no device)
    sel = SearchParameters(sel=IDSelectorBatch([1, 2]))
    unserved = [FlatIPIndex(D, device="cpu", screen="bf16x3"), FlatL2Bf16x3Index(D, device="cpu"), FlatSQ8Index(D, device="cpu"),
                FlatL2SQ8Index(D, device="cpu")]
    for index in unserved:
        for params in (sel, SearchParameters(sel=IDSelectorRange(0, 5))):
            with pytest.raises(ValueError, match=type(index).__name__):
                index.search(np.zeros((3, D), np.float32), 1, params=params)
            with pytest.raises(ValueError, match=type(index).__name__):
                index.search_async(np.zeros((3, D), np.float32), 1, params=params)
    # ... and the served ones take it: an empty index answers with padding, a wrong params object is refused
    for index in (FlatIPIndex(D, device="cpu"), FlatIPIndex(D, device="cpu", storage="float16"), FlatL2Index(D, device="cpu"),
                  FlatL2F16Index(D, device="cpu")):
        for params in (None, SearchParameters(), sel, SearchParameters(sel=IDSelectorRange(0, 5))):
            s, i = index.search(np.zeros((3, D), np.float32), 2, params=params)
            assert s.shape == (3, 2) and np.all(i == -1) and np.all(np.isinf(s))
        with pytest.raises(ValueError):
            index.search(np.zeros((3, D), np.float32), 2, params=IDSelectorBatch([1]))


def test_compat_shims_export_the_selector_names():
    import os
    import subprocess
    import sys
    from conftest import ROOT
    code = r'''
import faiss
import repconc_amd.faiss_compat as fc
from repconc_amd import selector
for n in ("IDSelectorRange", "IDSelectorBatch", "IDSelectorArray", "IDSelectorBitmap", "IDSelectorNot", "SearchParameters"):
    assert getattr(faiss, n) is getattr(fc, n) is getattr(selector, n), n
print("ok")
'''
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "compat"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]


# ---------------------------------------------------------------------------------------------------------------- GPU
DEV = "cuda:0"
OFF = 1000                       # id_offset of the direct calls
_cache = {}


def _randn(shape, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device=DEV, dtype=torch.float32)


def _data(N, D, nq, seed):
    """One gaussian corpus and query set per shape, generated once and never written to."""
    key = (N, D, nq, seed)
    if key not in _cache:
        _cache[key] = (_randn((N, D), seed), _randn((nq, D), seed + 1))
    return _cache[key]


def _random_rows(N, ns, seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return torch.sort(torch.randperm(N, generator=g, device=DEV)[:ns]).values.contiguous()


def _copy_search(name, xs, q, k, rows, id_offset=OFF, **kw):
    """Expectation (a): the variant's existing search over the materialised rows, ids mapped on the host; and its stats."""
    search = _variant(name)[0]
    pending = search(xs[rows].contiguous(), q, k, defer=True, **kw)
    s, i = pending.result()
    i = i.cpu()
    mapped = torch.where(i >= 0, id_offset + rows.cpu()[i.clamp_min(0)], torch.full_like(i, -1))
    return (s.cpu(), mapped), pending.stats


def _same(got, want, what=""):
    gs, gi = got[0].cpu(), got[1].cpu()
    ws, wi = want[0].cpu(), want[1].cpu()
    assert gs.shape == ws.shape and gi.shape == wi.shape and gi.dtype == torch.int64 and gs.dtype == torch.float32, what
    bad = torch.nonzero((gi != wi).any(1) | (gs.view(torch.int32) != ws.view(torch.int32)).any(1)).flatten()
    assert bad.numel() == 0, f"{what}: {bad.numel()} queries differ, first {int(bad[0])}: ids {gi[bad[0]][:8].tolist()} vs " \
                             f"{wi[bad[0]][:8].tolist()}, scores {gs[bad[0]][:4].tolist()} vs {ws[bad[0]][:4].tolist()}"


def _oracle(name, x, q, k, rows, id_offset=OFF):
    """Expectation (b): the numpy chain oracle over the selected rows, ids mapped."""
    _, _, _, seen, oracle, _ = _variant(name)
    ws, wi = oracle(seen(x[rows]).contiguous(), seen(q), k)
    r = rows.cpu().numpy()
    return ws, np.where(wi >= 0, id_offset + r[np.maximum(wi, 0)], -1)


def _selections(N):
    """name -> rows: a random half, every 7th row, one row, {0, N - 1}, the 128-row block tile edges, fewer rows than k can
    be, the identity."""
    sel = {
        "half": _random_rows(N, N // 2, 11),
        "every 7th": torch.arange(3, N, 7, dtype=torch.int64, device=DEV),
        "one row": torch.tensor([N // 3], dtype=torch.int64, device=DEV),
        "first and last": torch.tensor([0, N - 1], dtype=torch.int64, device=DEV),
        "ns 7 (< k)": _random_rows(N, 7, 12),
        "identity": torch.arange(N, dtype=torch.int64, device=DEV),
    }
    for ns in (127, 128, 129):
        sel[f"ns {ns}"] = _random_rows(N, ns, 100 + ns)
    return sel


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 100])          # 100: the PAD path of the fp32 kernels, and D % 8 != 0 for fp16
@pytest.mark.parametrize("name", SERVED)
def test_exact_route_subset_equals_the_search_of_the_copy(name, D):
    search, exact, store, _, _, l2 = _variant(name)
    N = 5000
    x, qall = _data(N, D, 130, 500 + D)
    xs = store(x)
    pad = float("inf") if l2 else float("-inf")
    for what, rows in _selections(N).items():
        ns = rows.numel()
        for nq in (1, 37, 130):                   # 130 crosses the 128-query tile
            q = qall[:nq]
            for k in (1, 10, 100):
                tag = f"{name} D={D} {what} nq={nq} k={k}"
                want, _ = _copy_search(name, xs, q, k, rows)
                pending = search(xs, q, k, id_offset=OFF, rows=rows, defer=True)
                got = pending.result()
                _same(got, want, tag)
                assert pending.stats == {"retried_queries": 0, "exact_queries": 0}
                _same(exact(xs, q, k, id_offset=OFF, rows=rows), want, tag + " exact")
                if ns < k:                        # padding past ns
                    assert bool((got[1][:, ns:] == -1).all()) and bool((got[0][:, ns:] == pad).all()), tag
                    assert bool((got[1][:, :ns] >= OFF).all()), tag
                if what == "identity":            # ... and the unmapped search itself, bit for bit
                    _same(got, search(xs, q, k, id_offset=OFF), tag + " unmapped")
                if nq == 37 and k == 10 and what in ("half", "ns 129", "ns 7 (< k)", "first and last"):
                    assert_matches(got, _oracle(name, x, q, k, rows))
    # check_rows off (a list valid by construction) and an empty selection: padding, no call
    rows = _selections(N)["every 7th"]
    _same(search(xs, qall[:5], 10, id_offset=OFF, rows=rows, check_rows=False), _copy_search(name, xs, qall[:5], 10, rows)[0])
    s, i = search(xs, qall[:5], 3, rows=rows[:0])
    assert s.shape == (5, 3) and bool((i == -1).all()) and bool((s == pad).all())
    s, i = exact(xs, qall[:5], 3, rows=rows[:0])
    assert bool((i == -1).all()) and bool((s == pad).all())


FAST_N, FAST_D, FAST_NQ = 300000, 32, 70


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [131072, 131073, 133001])      # the last exact-route size, the first fast-route size, a ragged one
@pytest.mark.parametrize("name", SERVED)
def test_fast_route_subset_equals_the_search_of_the_copy(name, ns):
    search, _, store, _, _, _ = _variant(name)
    x, q = _data(FAST_N, FAST_D, FAST_NQ, 900)
    xs = store(x)
    rows = _random_rows(FAST_N, ns, 2000 + ns)
    for k in (10, 100):
        want, want_stats = _copy_search(name, xs, q, k, rows)
        pending = search(xs, q, k, id_offset=OFF, rows=rows, defer=True)
        _same(pending.result(), want, f"{name} ns={ns} k={k}")
        print(f"{name} ns={ns} k={k}: mapped {pending.stats}, copy {want_stats}")
        if ns > 131072:
            assert pending.stats == {"retried_queries": 0, "exact_queries": 0}      # gaussian data: the fast route answers alone
        else:
            assert pending.stats["exact_queries"] == 0
    assert_matches(search(xs, q[:8], 10, id_offset=OFF, rows=rows), _oracle(name, x, q[:8], 10, rows))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SERVED)
def test_fast_route_subset_with_a_row_pitch_wider_than_d(name):
    """32-wide rows at a pitch of 40 elements (a strided view): rows[] times the PITCH is the row's address."""
    search, _, store, _, _, _ = _variant(name)
    x, q = _data(FAST_N, FAST_D, FAST_NQ, 900)
    buf = torch.empty((FAST_N, 40), dtype=store(x[:1]).dtype, device=DEV)
    buf.fill_(float("nan"))                                   # what lies between the rows must never be read as a value
    view = buf[:, :FAST_D]
    view.copy_(store(x))
    assert view.stride(0) == 40 and not view.is_contiguous()
    rows = _random_rows(FAST_N, 133001, 4133001)
    want, _ = _copy_search(name, store(x), q, 10, rows)
    pending = search(view, q, 10, id_offset=OFF, rows=rows, defer=True)
    _same(pending.result(), want, name)
    assert pending.stats == {"retried_queries": 0, "exact_queries": 0}


@pytest.mark.gpu
@pytest.mark.parametrize("name", SERVED)
def test_rows_outside_the_selection_do_not_leak_and_ties_take_the_lower_selected_id(name):
    """The best rows of the whole store (for the inner product: the queries scaled up; for L2: the queries themselves) are
    planted OUTSIDE the selection.  One selected row s per query, the best inside, has an exact duplicate at a lower
    unselected row and at a higher selected row."""
    search, _, store, _, _, l2 = _variant(name)
    N, D, nq, k = FAST_N, FAST_D, 16, 10
    x, q = _data(N, D, FAST_NQ, 900)
    x, q = x.clone(), q[:nq].clone()
    rows = _random_rows(N, 140000, 77)
    inside = torch.zeros((N,), dtype=torch.bool, device=DEV)
    inside[rows] = True
    outside = torch.nonzero(~inside).flatten()
    scale = (lambda t: t) if l2 else (lambda t: 3.0 * t)
    best = outside[torch.arange(nq, device=DEV) * 5 + 4000]                 # planted outsiders: the global winners
    x[best] = scale(q)
    lower_out = outside[torch.arange(nq, device=DEV) * 3 + 100]             # an unselected duplicate at a LOWER row than s
    s_row = rows[torch.arange(nq, device=DEV) * 11 + 60000]
    higher_in = rows[torch.arange(nq, device=DEV) * 11 + 90000]             # a selected duplicate at a HIGHER row than s
    assert bool((lower_out < s_row).all()) and bool((higher_in > s_row).all())
    near = scale(q) * 0.9 if not l2 else q + 0.01                            # the best row inside the selection
    x[s_row], x[lower_out], x[higher_in] = near, near, near
    xs = store(x)
    full = search(xs, q, k, id_offset=0)
    assert bool((full[1][:, 0] == best).all())                               # the whole store does prefer the outsiders
    assert bool((higher_in < rows[131071]).all())
    for r in (rows, rows[:131072].contiguous()):                             # the fast route, the exact route
        want, _ = _copy_search(name, xs, q, k, r, id_offset=0)
        got = search(xs, q, k, id_offset=0, rows=r)
        _same(got, want, name)
        ids = got[1]
        assert bool(inside[ids.flatten()].all())                             # nothing from outside the selection
        assert bool((ids[:, 0] == s_row).all()) and bool((ids[:, 1] == higher_in).all())
        assert bool((got[0][:, 0].view(torch.int32) == got[0][:, 1].view(torch.int32)).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["l2", "l2_f16"])
def test_l2_norms_are_read_at_the_mapped_row_on_the_fast_route(name):
    """The row norm grows about 30-fold with the row number: a screen that read xsq[j] instead of xsq[rows[j]] would rank by a
    wrong sigma.  The results must be those of the copy WITH no query repeated or handed to the exact route: the rescorer
    would otherwise repair the ids and hide a wrong norm."""
    search, _, store, _, _, _ = _variant(name)
    N, D, nq, k = FAST_N, FAST_D, 64, 10
    x, _ = _data(N, D, FAST_NQ, 900)
    grow = 1.0 + 29.0 * torch.arange(N, device=DEV, dtype=torch.float32) / (N - 1)
    x = x * grow[:, None]
    rows = _random_rows(N, 150001, 88)
    pick = rows[torch.linspace(0, rows.numel() - 1, nq, device=DEV).long()]    # queries near selected rows all over the store
    q = x[pick] + 0.05 * grow[pick][:, None] * _randn((nq, D), 89)
    xs = store(x)
    want, want_stats = _copy_search(name, xs, q, k, rows)
    pending = search(xs, q, k, id_offset=OFF, rows=rows, defer=True)
    _same(pending.result(), want, name)
    print(f"{name}: mapped {pending.stats}, copy {want_stats}")
    assert pending.stats == {"retried_queries": 0, "exact_queries": 0}
    assert bool((pending.result()[1][:, 0] == pick + OFF).all())
    assert_matches(pending.result(), _oracle(name, x, q, k, rows))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["f32", "l2_f16"])
def test_repeated_queries_and_the_exact_route_carry_the_rows(name):
    search, _, store, _, _, l2 = _variant(name)
    N, D, nq, k = FAST_N, FAST_D, 32, 100
    x, q = _data(N, D, FAST_NQ, 900)
    q = q[:nq]
    xs = store(x)
    rows = _random_rows(N, 140000, 99)
    want, _ = _copy_search(name, xs, q, k, rows)
    # a negative slack: the threshold admits too few candidates, the queries are repeated — over the same rows
    pending = search(xs, q, k, id_offset=OFF, rows=rows, sel_slack=-50.0, defer=True)
    got = pending.result()
    assert pending.stats["retried_queries"] > 0
    _same(got, want, name + " retried")
    # a tie group of 20 000 selected identical rows straddling the k-th score: the exact route answers, over the same rows
    x = x.clone()
    if l2:
        q = 0.05 * q[:4]
        v = _randn((D,), 37)
        x[90000:110000] = (v * (11.3 ** 0.5 / v.norm()))[None]      # |v|^2 = 11.3: a few dozen of the rows (|x|^2 ~ chi2_32) are nearer
    else:
        u = _randn((D,), 33)
        u /= u.norm()
        noise = q[:4] - (q[:4] @ u)[:, None] * u[None]
        q = 20.0 * u[None] + noise
        x[90000:110000] = (3.6 * float(q.norm(dim=1).mean()) / 20.0) * u[None]   # z = 3.6: ~25 of 160 000 gaussian rows score higher
    xs = store(x)
    g = torch.zeros((N,), dtype=torch.bool, device=DEV)
    g[rows] = True
    g[90000:110000] = True
    rows = torch.nonzero(g).flatten()
    want, _ = _copy_search(name, xs, q, k, rows)
    tied = (want[1] >= OFF + 90000) & (want[1] < OFF + 110000)
    assert bool(tied.any(1).all()) and bool((~tied).any(1).all())               # the group straddles the k-th score
    pending = search(xs, q, k, id_offset=OFF, rows=rows, defer=True)
    _same(pending.result(), want, name + " tie group")
    assert pending.stats["exact_queries"] > 0


def _index(name, d):
    from repconc_amd.dense_index import FlatIPIndex, FlatL2F16Index, FlatL2Index
    return {"f32": lambda: FlatIPIndex(d, device=DEV), "f16": lambda: FlatIPIndex(d, device=DEV, storage="float16"),
            "l2": lambda: FlatL2Index(d, device=DEV), "l2_f16": lambda: FlatL2F16Index(d, device=DEV)}[name]()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [5000, 140000])              # the exact route, the fast route
@pytest.mark.parametrize("name", SERVED)
def test_index_search_with_selectors(name, N):
    D, nq, k, off = FAST_D, 20, 10, 70000
    xall, qall = _data(FAST_N, FAST_D, FAST_NQ, 900)
    x, q = xall[:N], qall[:nq]
    index = _index(name, D)
    index.id_offset = off
    index.add(x[: N - 1000])

    def fresh(xrows, ids):
        """The same class over just those vectors; its row numbers turned into the ids given."""
        other = _index(name, D)
        other.add(xrows)
        s, i = other.search(q, k)
        i = i.cpu()
        return s.cpu(), torch.where(i >= 0, ids.cpu()[i.clamp_min(0)], torch.full_like(i, -1))

    plain = index.search(q, k)
    _same(index.search(q, k, params=None), plain)
    _same(index.search(q, k, params=SearchParameters()), plain)
    # external ids: a batch holding ids below id_offset, past the index and twice
    held = torch.arange(off, off + index.ntotal, device=DEV)
    g = torch.Generator(device=DEV)
    g.manual_seed(5)
    some = held[torch.randperm(index.ntotal, generator=g, device=DEV)[: index.ntotal // 3]]
    batch = IDSelectorBatch(torch.cat([some, some[:50], torch.tensor([3, off - 1, off + N + 5], device=DEV)]))
    kept = torch.sort(some).values
    got = index.search(q, k, params=SearchParameters(sel=batch))
    _same(got, fresh(x[kept - off], kept), f"{name} batch")
    assert index.last_search.stats == {"retried_queries": 0, "exact_queries": 0}
    # numpy in -> numpy out
    s_np, i_np = index.search(q.cpu().numpy(), k, params=SearchParameters(sel=batch))
    assert isinstance(s_np, np.ndarray) and isinstance(i_np, np.ndarray)
    _same((torch.from_numpy(s_np), torch.from_numpy(i_np)), got)
    # a range equals the batch of the same ids, and takes no row list
    lo, hi = off + 1234, off + index.ntotal - 321
    rng = IDSelectorRange(lo, hi)
    by_range = index.search(q, k, params=SearchParameters(sel=rng))
    _same(by_range, index.search(q, k, params=SearchParameters(sel=IDSelectorBatch(torch.arange(lo, hi)))), f"{name} range")
    _same(by_range, fresh(x[lo - off:hi - off], torch.arange(lo, hi)), f"{name} range, fresh index")
    assert rng._rows is None
    # Not(Batch(the top ids)) removes exactly those
    top = plain[1][:, :3].flatten()
    without = index.search(q, k, params=SearchParameters(sel=IDSelectorNot(IDSelectorBatch(top))))
    keep = torch.ones((index.ntotal,), dtype=torch.bool, device=DEV)
    keep[top - off] = False
    rest = torch.nonzero(keep).flatten()
    _same(without, fresh(x[rest], rest + off), f"{name} not")
    assert not bool(torch.isin(without[1], top).any())
    # a bitmap over the external ids
    bits = np.zeros(((off + N) // 8 + 1,), np.uint8)
    chosen = kept.cpu().numpy()[::2]
    np.bitwise_or.at(bits, chosen >> 3, (1 << (chosen & 7)).astype(np.uint8))
    _same(index.search(q, k, params=SearchParameters(sel=IDSelectorBitmap(bits))), fresh(x[kept[::2] - off], kept[::2]), f"{name} bitmap")
    # `add` after a selector was first used: the complement grows with the index, the batch now finds the ids it was refused
    neg = IDSelectorNot(IDSelectorBatch(top))
    index.search(q, k, params=SearchParameters(sel=neg))
    before = neg._rows.numel()
    index.add(x[N - 1000:])
    grown = index.search(q, k, params=SearchParameters(sel=neg))
    assert neg._rows.numel() == before + 1000
    keep = torch.ones((N,), dtype=torch.bool, device=DEV)
    keep[top - off] = False
    rest = torch.nonzero(keep).flatten()
    _same(grown, fresh(x[rest], rest + off), f"{name} not, after add")
    # an empty selection: padding
    s, i = index.search(q, k, params=SearchParameters(sel=IDSelectorBatch([1, 2, 3])))
    assert bool((i == -1).all()) and bool(torch.isinf(s).all())
    s, i = index.search(q, k, params=SearchParameters(sel=IDSelectorRange(0, off)))
    assert bool((i == -1).all()) and bool(torch.isinf(s).all())


@pytest.mark.gpu
def test_unserved_indexes_refuse_a_selector_with_rows_held():
    from repconc_amd.dense_index import FlatIPIndex, FlatL2Bf16x3Index, FlatL2SQ8Index, FlatSQ8Index
    x, q = _data(5000, 16, 130, 516)
    for index in (FlatIPIndex(16, device=DEV, screen="bf16x3"), FlatL2Bf16x3Index(16, device=DEV), FlatSQ8Index(16, device=DEV),
                  FlatL2SQ8Index(16, device=DEV)):
        if hasattr(index, "train"):
            index.train(x)
        index.add(x)
        plain = index.search(q[:4], 5)
        with pytest.raises(ValueError, match=type(index).__name__):
            index.search(q[:4], 5, params=SearchParameters(sel=IDSelectorBatch([1, 2, 3])))
        _same(index.search(q[:4], 5, params=SearchParameters()), plain)
        _same(index.search(q[:4], 5, params=None), plain)
