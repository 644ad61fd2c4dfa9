"""RefineIndex (repconc_amd/refine_index.py): candidates from a compressed index, re-ranked exactly by a flat index — the GPU
faiss.IndexRefineFlat — and `encode_corpus_to_index(..., refine=flat)`, which fills both from one pass over the corpus.

The oracle of the re-ranking is the one of tests/test_dense_rerank.py: the emulated chain over the candidates' rows and a
lexicographic sort on (score, id)."""
from types import SimpleNamespace

import numpy as np
import pytest

from test_dense_rerank import IP, L2, PAD, _check, cut, oracle_sorted

DEV = "cuda:0"


# --------------------------------------------------------------------------------------------------------------- CPU
class _Base:
    def __init__(self, ntotal=100, metric_type=None):
        self.ntotal = ntotal
        if metric_type is not None:
            self.metric_type = metric_type
        self.calls = []

    def search(self, x, k, **kw):
        self.calls.append((x, k, kw))
        return "base scores", ("ids", k)


class _Refine:
    d = 8

    def __init__(self, ntotal=100, metric_type=None):
        self.ntotal = ntotal
        if metric_type is not None:
            self.metric_type = metric_type
        self.calls = []

    def rerank(self, x, cand_ids, k):
        self.calls.append((x, cand_ids, k))
        return "refined", cand_ids


def test_refine_index_candidate_count_and_forwarding_on_stubs():
    from repconc_amd.refine_index import RefineIndex
    base, refine = _Base(), _Refine()
    ri = RefineIndex(base, refine)
    assert ri.k_factor == 1.0 and ri.ntotal == 100 and ri.d == 8
    x = object()
    for k_factor, k, kc in ((1.0, 10, 10), (2.5, 10, 25), (2.5, 3, 8), (0.5, 10, 10), (5.0, 1000, 5000), (100.0, 1000, 8192),
                            (1.0001, 8192, 8192), (400, 10, 4000)):
        ri.k_factor = k_factor                                   # a plain attribute
        assert ri.candidates(k) == kc
        out = ri.search(x, k)
        assert base.calls[-1] == (x, kc, {}) and refine.calls[-1] == (x, ("ids", kc), k) and out == ("refined", ("ids", kc))
    xr = object()
    ri.k_factor = 2.0
    ri.search(x, 7, x_refine=xr, nprobe=3, method="scan")
    assert base.calls[-1] == (x, 14, {"nprobe": 3, "method": "scan"})          # base_kwargs reach the base, x_refine does not
    assert refine.calls[-1] == (xr, ("ids", 14), 7)                            # the refine stage sees x_refine
    with pytest.raises(ValueError):
        ri.search(x, 0)


def test_refine_index_rejects_mismatched_parts():
    from repconc_amd.refine_index import RefineIndex
    ri = RefineIndex(_Base(100), _Refine(99))                     # checked at search time: the owners fill the parts
    n = len(ri.base.calls)
    with pytest.raises(ValueError):
        ri.search(object(), 5)
    assert len(ri.base.calls) == n                                # before the base runs
    ri.refine.ntotal = 100
    ri.search(object(), 5)
    with pytest.raises(ValueError):
        RefineIndex(_Base(metric_type=IP), _Refine(metric_type=L2))
    ok = RefineIndex(_Base(metric_type=L2), _Refine(metric_type=L2))
    assert ok.metric_type == L2
    ok.base.metric_type = IP                                     # ... and again when it searches
    with pytest.raises(ValueError):
        ok.search(object(), 5)
    RefineIndex(_Base(), _Refine(metric_type=L2))                 # one side without a metric: nothing to compare
    with pytest.raises(ValueError):
        RefineIndex(SimpleNamespace(ntotal=3), _Refine())         # no search
    with pytest.raises(ValueError):
        RefineIndex(_Base(), _Base())                             # no rerank: not a flat index
    assert not hasattr(RefineIndex, "add")


def test_encode_corpus_to_index_keeps_its_signature_default():
    import inspect
    from repconc_amd.encode import encode_corpus_to_index
    assert inspect.signature(encode_corpus_to_index).parameters["refine"].default is None


# --------------------------------------------------------------------------------------------------------------- GPU
def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _corpus(N, D, M, seed):
    from oracle import synth
    x = synth.clustered_embeddings(seed, N, D=D, n_clusters=32)
    C = synth.sample_centroids(seed + 1, x, M)
    q = (x[np.random.default_rng(seed + 2).permutation(N)[:9]] + 0.3 * synth.gaussian(seed + 3, (9, D))).astype(np.float32)
    return x, C, q


def _flat(metric, D, storage="float32"):
    from repconc_amd.dense_index import FlatIPIndex, FlatL2F16Index, FlatL2Index
    if metric == L2:
        return FlatL2F16Index(D) if storage == "float16" else FlatL2Index(D)
    return FlatIPIndex(D, storage=storage)


def _pq(metric, x, C):
    from repconc_amd.index import PQIndex
    M, _, dsub = C.shape
    base = PQIndex(M * dsub, M, 8, metric)
    base.set_centroids(_t(C))
    base.add(_t(x))
    return base


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [IP, L2])
def test_refine_over_every_row_equals_the_flat_search(metric):
    """N = 4000, k = 10, k_factor = 400: kc = 4000 = N, the base returns every row and the result is the flat index's own."""
    import torch
    from repconc_amd.refine_index import RefineIndex
    N, D, M, k = 4000, 64, 8, 10
    x, C, q = _corpus(N, D, M, 11)
    for storage in ("float32", "float16"):
        flat = _flat(metric, D, storage)
        flat.add(_t(x))
        ri = RefineIndex(_pq(metric, x, C), flat, k_factor=400)
        assert ri.candidates(k) == N
        got, want = ri.search(_t(q), k), flat.search(_t(q), k)
        assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
        got = ri.search(q, k)                                    # numpy in -> numpy out
        assert isinstance(got[0], np.ndarray) and np.array_equal(got[1], want[1].cpu().numpy())
        assert np.array_equal(got[0].view(np.uint32), want[0].cpu().numpy().view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [IP, L2])
def test_refine_of_a_flat_pq_base(metric):
    """N = 20 000, D = 64, M = 8, k_factor = 5: every id returned is one of the base's kc, the scores are the chain's bits in
    the right order, and the result is ops.dense_rerank on the base's ids."""
    import torch
    from repconc_amd import ops
    from repconc_amd.refine_index import RefineIndex
    N, D, M, k = 20000, 64, 8, 10
    x, C, q = _corpus(N, D, M, 21)
    base = _pq(metric, x, C)
    flat = _flat(metric, D)
    flat.add(_t(x))
    ri = RefineIndex(base, flat, k_factor=5)
    qd = _t(q)
    got = ri.search(qd, k)
    _, bids = base.search(qd, 50)
    bn = bids.cpu().numpy()
    assert bn.shape == (9, 50) and (bn >= 0).all()
    gi = got[1].cpu().numpy()
    assert all(np.isin(gi[j], bn[j]).all() for j in range(9))
    _check(got, cut(oracle_sorted(x, q, bn, metric), k, metric))
    direct = ops.dense_rerank(flat.xb, qd, bids, k, metric=metric)
    assert torch.equal(got[1], direct[1]) and torch.equal(got[0].view(torch.int32), direct[0].view(torch.int32))
    # the refined list is at least as good as the base's own top-k, measured by the exact score
    exact = flat.search(qd, k)
    hits = lambda ids: np.mean([len(np.intersect1d(ids[j], exact[1][j].cpu().numpy())) for j in range(9)])
    assert hits(gi) >= hits(bn[:, :k])


@pytest.mark.gpu
@pytest.mark.parametrize("metric", [IP, L2])
def test_refine_of_an_ivf_base_skips_its_holes(metric):
    """One probed cell of 128 holds about 30 rows: a search for kc = 200 returns -1 in most slots, fewer than k = 100 ids for
    some queries.  The output is the top-k of the valid candidates, padded."""
    import torch
    from repconc_amd.ivf import IVFPQIndex
    from repconc_amd.refine_index import RefineIndex
    N, D, M, nlist, k = 4000, 128, 16, 128, 100
    x, C, q = _corpus(N, D, M, 31)
    ivf = IVFPQIndex(D, M, nlist, device=torch.device(DEV), metric=metric)
    ivf.set_centroids(_t(C))
    ivf.coarse = _t(x[np.random.default_rng(32).choice(N, nlist, replace=False)].copy())
    ivf.add(_t(x))
    flat = _flat(metric, D)
    flat.add(_t(x))
    ri = RefineIndex(ivf, flat, k_factor=2.0)
    qd = _t(q)
    _, bids = ivf.search(qd, 200, nprobe=1)
    bn = bids.cpu().numpy()
    valid = (bn >= 0).sum(1)
    assert (valid < k).any() and (valid > 0).any()
    got = ri.search(qd, k, nprobe=1)
    _check(got, cut(oracle_sorted(x, q, bn, metric), k, metric))
    gs, gi = (t.cpu().numpy() for t in got)
    for j in range(9):
        n = min(k, valid[j])
        assert (gi[j, :n] >= 0).all() and (gi[j, n:] == -1).all() and (gs[j, n:] == PAD[metric]).all()
    wider = ri.search(qd, k, nprobe=4)                           # nprobe reaches the base: more cells, more candidates
    assert ((wider[1] >= 0).sum(1).cpu().numpy() >= np.minimum(valid, k)).all()
    assert ((wider[1] >= 0).sum() > (got[1] >= 0).sum())


class _StubModel:
    """What encode_corpus_to_index needs of a RepCONC model: centroids, config, and a call that returns continuous_embeds."""

    def __init__(self, table, C):
        self.table = table
        self.centroids = torch_parameter(C)
        self.config = SimpleNamespace(hidden_size=table.shape[1], MCQ_M=C.shape[0])

    def __call__(self, input_ids, attention_mask):
        return SimpleNamespace(continuous_embeds=self.table[input_ids[:, 0]])


def torch_parameter(C):
    import torch
    return torch.nn.Parameter(_t(C), requires_grad=False)


@pytest.mark.gpu
def test_encode_corpus_to_index_fills_the_refine_index_in_order():
    import torch
    from repconc_amd.dense_index import FlatIPIndex
    from repconc_amd.encode import encode_corpus_to_index
    from repconc_amd.refine_index import RefineIndex
    N, D, M = 1000, 64, 8
    x, C, q = _corpus(N, D, M, 41)
    model = _StubModel(_t(x), C)

    def batches():
        for a in range(0, N, 300):                               # 300, 300, 300, 100
            ids = torch.arange(a, min(a + 300, N), device=DEV)[:, None].repeat(1, 4)
            yield ids, torch.ones_like(ids)

    plain = encode_corpus_to_index(model, batches())
    flat = FlatIPIndex(D)
    index = encode_corpus_to_index(model, batches(), refine=flat)
    assert flat.ntotal == N and torch.equal(flat.xb, _t(x))       # exactly the embeddings, in order
    assert index.ntotal == N and torch.equal(index.codes, plain.codes)
    ri = RefineIndex(index, flat, k_factor=1000)                 # kc = min(10 000, 8192) >= N: the flat search's answer
    got, want = ri.search(_t(q), 10), flat.search(_t(q), 10)
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
