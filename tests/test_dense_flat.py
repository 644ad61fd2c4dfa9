"""Exact dense inner-product search (faiss.IndexFlatIP of models/dense/evaluate_dense.py:84-129): csrc/dense_search.hip,
ops.dense_search, dense_index.FlatIPIndex, models/dense/evaluate_dense.py and the Faiss shim.

The oracle is in this file.  A score is the fp32 fmaf chain over d ascending from +0.0f; fmaf is emulated exactly in numpy
(exact fp64 product, TwoSum, round-to-odd in fp64, then one rounding to fp32: correct because 53 >= 24 + 2) and checked
against the C library's fmaf.  For large N only the rows that can reach the top-k are chain-scored: an fp64 ranking, the
chain's error bound gamma_D * sum_d |q_d x_d|, and every row whose upper bound reaches the k-th largest lower bound."""
import ctypes
import ctypes.util
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT


# ------------------------------------------------------------------------------------------------------------ oracle
def fmaf_emul(a, b, c):
    """Correctly rounded fp32 fma, elementwise (numpy float32 arrays in, float32 out)."""
    a64 = np.asarray(a, dtype=np.float32).astype(np.float64)
    b64 = np.asarray(b, dtype=np.float32).astype(np.float64)
    c64 = np.asarray(c, dtype=np.float32).astype(np.float64)
    p = a64 * b64                                    # exact: 24 + 24 significant bits
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)                  # TwoSum: p + c = s + e exactly
    s = np.atleast_1d(s).copy()
    e = np.atleast_1d(e)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)  # inexact and even: the odd neighbour on e's side
    if fix.any():
        s[fix] = np.nextafter(s[fix], np.where(e[fix] > 0, np.inf, -np.inf))
    return s.astype(np.float32).reshape(np.shape(p))


def chain_scores(qp, xp):
    """qp, xp: [P, D] fp32 -> the fp32 fmaf chain of every pair, [P]."""
    qp = np.ascontiguousarray(qp, dtype=np.float32)
    xp = np.ascontiguousarray(xp, dtype=np.float32)
    s = np.zeros(qp.shape[0], dtype=np.float32)
    for d in range(qp.shape[1]):
        s = fmaf_emul(qp[:, d], xp[:, d], s)
    return s


def oracle_topk(x, q, k, qblock=256, rblock=1 << 18):
    """x: device fp32 [N, D], q: device fp32 [nq, D] -> (scores fp32 [nq, k], ids int64 [nq, k]) of the chain, sorted
    (score desc, row asc), -inf / -1 past N."""
    import torch
    N, D = x.shape
    nq = q.shape[0]
    u = 2.0 ** -24
    gamma = 1.01 * D * u / (1 - D * u) + 1e-12       # fp32 chain error bound factor (+ the fp64 ranking's own error)
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_i = np.full((nq, k), -1, dtype=np.int64)
    kk = min(k, N)
    for q0 in range(0, nq, qblock):
        qb = q[q0:q0 + qblock].double()
        S = torch.empty((qb.shape[0], N), dtype=torch.float64, device=x.device)
        A = torch.empty_like(S)
        for r0 in range(0, N, rblock):
            xb = x[r0:r0 + rblock].double()
            S[:, r0:r0 + rblock] = qb @ xb.T
            A[:, r0:r0 + rblock] = qb.abs() @ xb.abs().T
        A.mul_(gamma)
        kth = torch.topk(S - A, kk, dim=1).values[:, -1:]
        qi, ri = torch.nonzero(S + A >= kth, as_tuple=True)
        del S, A
        s = chain_scores(q[q0:q0 + qblock][qi].cpu().numpy(), x[ri].cpu().numpy())
        qi, ri = qi.cpu().numpy(), ri.cpu().numpy()
        order = np.lexsort((ri, -s.astype(np.float64), qi))
        qi, ri, s = qi[order], ri[order], s[order]
        starts = np.searchsorted(qi, np.arange(qb.shape[0]))
        for j in range(qb.shape[0]):
            a = starts[j]
            assert a + kk <= len(qi) and (a + kk == len(qi) or qi[a + kk - 1] == j)
            out_s[q0 + j, :kk] = s[a:a + kk]
            out_i[q0 + j, :kk] = ri[a:a + kk]
    return out_s, out_i


def assert_matches(got, want, id_offset=0):
    gs, gi = (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t) for t in got)
    ws, wi = want
    wi = np.where(wi >= 0, wi + id_offset, -1)
    bad = np.nonzero((gi != wi).any(1) | (gs.view(np.uint32) != ws.view(np.uint32)).any(1))[0]
    assert bad.size == 0, f"{bad.size} queries differ, first {bad[0]}: ids {gi[bad[0]][:8]} vs {wi[bad[0]][:8]}, " \
                          f"scores {gs[bad[0]][:4]} vs {ws[bad[0]][:4]}"


# --------------------------------------------------------------------------------------------------------------- CPU
def test_fmaf_emulation_matches_the_c_library():
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    fmaf = libm.fmaf
    fmaf.argtypes = [ctypes.c_float] * 3
    fmaf.restype = ctypes.c_float
    rng = np.random.default_rng(11)
    n = 30000
    parts = []
    # random magnitudes over a wide exponent range, both signs
    parts.append([(rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)).astype(np.float32) for _ in range(3)])
    # products with bits down to 2^-24 (many exact fp32 midpoints: ties to even), small addends
    i, j = rng.integers(0, 4096, n), rng.integers(0, 4096, n)
    a = (1 + i * 2.0 ** -12).astype(np.float32)
    b = (1 + j * 2.0 ** -12).astype(np.float32) * np.where(rng.random(n) < 0.5, -1, 1).astype(np.float32)
    c = np.where(rng.random(n) < 0.5, 0.0, rng.integers(-8, 8, n) * 2.0 ** -24).astype(np.float32)
    parts.append([a, b, c])
    # exact cancellation: c = -(a b) exactly (12-bit mantissas), and c = -fl(a b)
    a = (rng.integers(1, 4096, n) * 2.0 ** rng.integers(-20, 0, n)).astype(np.float32)
    b = (rng.integers(1, 4096, n) * 2.0 ** rng.integers(-20, 0, n)).astype(np.float32)
    c = -(a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)
    parts.append([a, b, c])
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    parts.append([a, b, -(a * b)])
    # subnormal products, addends and results
    a = (rng.standard_normal(n) * 2.0 ** -70).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** -70).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-149, -126, n)).astype(np.float32)
    parts.append([a, b, c])
    parts.append([np.zeros(4, np.float32), np.array([0, -1, 1, -0.0], np.float32), np.array([0, 0, -0.0, -0.0], np.float32)])
    A, B, Cc = (np.concatenate([p[t] for p in parts]) for t in range(3))
    assert A.size >= 100000
    got = fmaf_emul(A, B, Cc)
    want = np.array([fmaf(float(x), float(y), float(z)) for x, y, z in zip(A, B, Cc)], dtype=np.float32)
    diff = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert diff.size == 0, (A[diff[:3]], B[diff[:3]], Cc[diff[:3]], got[diff[:3]], want[diff[:3]])
    # the chain is not a correctly rounded dot product: it differs from fl(fp64 dot) on some rows
    q = rng.standard_normal((64, 768)).astype(np.float32)
    x = rng.standard_normal((64, 768)).astype(np.float32)
    ch = chain_scores(q, x)
    assert np.all(np.abs(ch - (q.astype(np.float64) * x).sum(1)) <= 768 * 2.0 ** -24 * np.abs(q * x).sum(1))


def test_compat_exports_indexflatip_and_evaluate_dense():
    code = r'''
import faiss
import repconc_amd.faiss_compat as fc
from repconc_amd.dense_index import FlatIPIndex
assert faiss.IndexFlatIP is fc.IndexFlatIP is FlatIPIndex
assert not hasattr(faiss, "index_factory")
from repconc.models.dense.evaluate_dense import (DenseEvaluater, encode_dense_corpus, encode_dense_query, dense_search,
    batch_dense_search, create_index)
import repconc.models.dense.evaluate_dense as alias, repconc_amd.models.dense.evaluate_dense as real
assert alias is real
print("ok")
'''
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, "compat"), ROOT]))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-3000:]


def test_dense_workspace_helpers_and_shape_errors_need_no_gpu():
    from repconc_amd import _lib
    lib = _lib.load()
    N, D = 8841823, 768
    ws = lib.rc_dense_search_ws_bytes(N, D, 1200, 1000)
    assert ws >= 1200 * (32768 * 4 + 16384 * 8)                  # sample scores + candidate keys
    assert lib.rc_dense_search_ws_bytes(1000, D, 1200, 10) == lib.rc_dense_search_exact_ws_bytes(1000, D, 1200, 10)
    ex = lib.rc_dense_search_exact_ws_bytes(N, D, 7, 100)
    assert 7 * N * 4 <= ex <= 256 * 2 ** 20 + 8 * 16384 * 8 + 8192   # score rows of one round, bounded
    for args in ((N, D, 1200, 8193), (1 << 32, D, 4, 10), (0, D, 4, 10), (N, 0, 4, 10), (N, D, 0, 10), (N, D, 4, 0)):
        assert lib.rc_dense_search_ws_bytes(*args) == 0 and lib.rc_dense_search_exact_ws_bytes(*args) == 0
    RC_ESHAPE, RC_EINVAL = -2, -1
    z = None
    assert lib.rc_dense_search_q(z, z, D, N, D, z, 4, 8193, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_search_q(z, z, D, 1 << 32, D, z, 4, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_search_exact(z, z, D, N, D, z, 4, 8193, 0, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_search_exact(z, z, D, 1 << 32, D, z, 4, 10, 0, z, z, z, 0, z) == RC_ESHAPE
    assert lib.rc_dense_search_q(z, z, D, N, D, z, 4, 10, 0, 3.0, z, z, z, z, z, 0, z) == RC_EINVAL


def test_dense_search_rejects_cpu_tensors():
    import torch
    from repconc_amd import _lib, ops
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_search(torch.zeros(10, 16), torch.zeros(2, 16), 1)
    with pytest.raises(_lib.RepconcHipError):
        ops.dense_search_exact(torch.zeros(10, 16), torch.zeros(2, 16), 1)


# --------------------------------------------------------------------------------------------------------------- GPU
def _randn(shape, seed, dev="cuda:0"):
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev, dtype=torch.float32)


# every value of N {1, 5, 1000, 65537, 300007}, D {768, 384, 1024, 100}, nq {1, 7, 128, 1201}, k {1, 10, 100, 1000, 8192}
SHAPES = [
    (1, 768, 1, 10),            # k > N: -inf / -1 padding
    (5, 100, 7, 8),             # k > N, D padded to the K chunk
    (1000, 384, 128, 1000),     # k = N
    (65537, 1024, 7, 100),
    (65537, 768, 1201, 1),
    (300007, 768, 1201, 10),    # sampled-threshold route
    (300007, 100, 1, 8192),     # padded D on the screen, the largest k
    (300007, 384, 128, 1000),
]


@pytest.mark.gpu
@pytest.mark.parametrize("N,D,nq,k", SHAPES)
def test_dense_search_ids_and_score_bits_equal_the_oracle(N, D, nq, k):
    from repconc_amd import ops
    x = _randn((N, D), 1000 + N + D)
    q = _randn((nq, D), 2000 + nq + D)
    want = oracle_topk(x, q, k)
    for method in ("auto", "exact"):
        got = ops.dense_search(x, q, k, id_offset=7, method=method)
        assert got[0].shape == (nq, k) and got[1].dtype.is_floating_point is False
        assert_matches(got, want, id_offset=7)


@pytest.mark.gpu
def test_dense_search_ties_take_the_lower_id_and_fall_back_to_the_exact_route():
    """5 % of the rows duplicated, and 20 000 identical rows whose score sits inside every query's top-100 (about 50 rows
    score higher): the tie group overflows the candidate list whatever the slack, the fallback answers."""
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
    x[90000:110000] = (3.48 * qn / 20.0) * u[None]          # z = 3.48: ~50 of 200 000 gaussian rows score higher
    want = oracle_topk(x, q, k)
    tied = (want[1] >= 90000) & (want[1] < 110000)
    assert tied.any(1).all() and (~tied).any(1).all()        # the tie group straddles the k-th score of every query
    pending = ops.dense_search(x, q, k, defer=True)
    got = pending.result()
    assert_matches(got, want)
    assert pending.stats["exact_queries"] > 0
    assert_matches(ops.dense_search(x, q, k, method="exact"), want)


@pytest.mark.gpu
def test_dense_search_negative_slack_forces_retries_with_unchanged_results():
    from repconc_amd import ops
    N, D, nq, k = 200000, 768, 64, 100
    x, q = _randn((N, D), 41), _randn((nq, D), 42)
    want = oracle_topk(x, q, k)
    pending = ops.dense_search(x, q, k, sel_slack=-50.0, defer=True)
    got = pending.result()
    assert pending.stats["retried_queries"] > 0
    assert_matches(got, want)
    plain = ops.dense_search(x, q, k, defer=True)
    assert_matches(plain.result(), want)


@pytest.mark.gpu
def test_dense_search_corpus_above_4_gib():
    """1 500 000 x 768 fp32 = 4.6 GB: byte offsets past 2^32; query 0's best row is the last one."""
    from repconc_amd import ops
    N, D, nq, k = 1500000, 768, 16, 100
    x = _randn((N, D), 51)
    q = _randn((nq, D), 52)
    x[N - 1] = 2.0 * q[0]
    x[N - 2] = 2.0 * q[1]
    want = oracle_topk(x, q, k, qblock=16, rblock=1 << 19)
    assert want[1][0, 0] == N - 1 and want[1][1, 0] == N - 2
    assert_matches(ops.dense_search(x, q, k), want)
    del x


@pytest.mark.gpu
def test_flat_ip_index_add_reset_search_and_batching():
    import torch
    from repconc_amd.dense_index import FlatIPIndex
    from repconc_amd.faiss_compat import IndexFlatIP
    from repconc_amd.models.dense.evaluate_dense import batch_dense_search, dense_search
    N, D, nq, k = 3000, 384, 50, 20
    xb = _randn((N, D), 61).cpu().numpy()
    qb = _randn((nq, D), 62).cpu().numpy()
    one = IndexFlatIP(D)
    assert isinstance(one, FlatIPIndex) and one.is_trained and one.metric_type == 0 and one.d == D
    one.add(xb)
    assert one.ntotal == N and one._x.shape[0] == N                 # the first add allocates exactly
    three = FlatIPIndex(D, device="cuda")
    three.add(xb[:1000])
    three.add(torch.from_numpy(xb[1000:1100]).cuda())
    assert three._x.shape[0] == 1500                               # growth 1.5x
    three.add(xb[1100:])
    assert three.ntotal == N
    s1, i1 = one.search(qb, k)
    s3, i3 = three.search(qb, k)
    assert isinstance(s1, np.ndarray) and isinstance(i1, np.ndarray) and i1.dtype == np.int64
    assert np.array_equal(i1, i3) and np.array_equal(s1.view(np.uint32), s3.view(np.uint32))
    st, it = one.search(torch.from_numpy(qb).cuda(), k)
    assert isinstance(st, torch.Tensor) and st.is_cuda and it.is_cuda
    assert np.array_equal(it.cpu().numpy(), i1) and np.array_equal(st.cpu().numpy().view(np.uint32), s1.view(np.uint32))
    assert_matches((s1, i1), oracle_topk(torch.from_numpy(xb).cuda(), torch.from_numpy(qb).cuda(), k))
    # batched search: every batch enqueued first, same answer as the reference's per-batch loop
    corpus_ids = np.array([f"d{i}" for i in range(N)])
    qids = np.arange(nq)
    bs, bi = batch_dense_search(qids, qb, corpus_ids, one, k, batch_size=16)
    loop = [dense_search(a, b, corpus_ids, one, k) for a, b in zip(np.array_split(qids, 4), np.array_split(qb, 4))]
    assert np.array_equal(bi, np.concatenate([g[1] for g in loop])) and np.array_equal(bi, corpus_ids[i1])
    assert np.array_equal(bs.view(np.uint32), np.concatenate([g[0] for g in loop]).view(np.uint32))
    one.reserve(5000)
    assert one._x.shape[0] == 5000 and np.array_equal(one.search(qb, k)[1], i1)
    one.reset()
    assert one.ntotal == 0
    s0, i0 = one.search(qb[:3], 5)
    assert np.all(i0 == -1) and np.all(np.isneginf(s0))
    one.add(xb[:10])
    assert np.array_equal(one.search(qb[:3], 5)[1], oracle_topk(torch.from_numpy(xb[:10]).cuda(),
                                                                torch.from_numpy(qb[:3]).cuda(), 5)[1])


class _WordTokenizer:
    """'w<n>' -> token n + 3 ([CLS] = 1, [SEP] = 2, pad = 0), truncated to max_length."""

    def __call__(self, texts, padding=True, truncation=True, max_length=32):
        ids = [[1] + [3 + int(w[1:]) for w in t.split()][: max_length - 2] + [2] for t in texts]
        L = max(map(len, ids))
        return {"input_ids": [i + [0] * (L - len(i)) for i in ids],
                "attention_mask": [[1] * len(i) + [0] * (L - len(i)) for i in ids]}


@pytest.mark.gpu
def test_dense_eval_end_to_end_with_a_random_bert():
    import torch
    from transformers import BertConfig
    from repconc_amd.models.dense import BertDense
    from repconc_amd.models.dense.evaluate_dense import (batch_dense_search, create_index, encode_dense_corpus,
                                                         encode_dense_query)
    from repconc_amd.utils.eval_utils import get_collator_func
    torch.manual_seed(0)
    cfg = BertConfig(hidden_size=64, num_hidden_layers=1, num_attention_heads=4, intermediate_size=128, vocab_size=200,
                     max_position_embeddings=64)
    model = BertDense(cfg).cuda().eval()
    rng = np.random.default_rng(5)
    corpus = {f"doc{i}": " ".join(f"w{v}" for v in rng.integers(0, 190, rng.integers(1, 30))) for i in range(400)}
    queries = {int(i): " ".join(f"w{v}" for v in rng.integers(0, 190, rng.integers(1, 8))) for i in rng.permutation(37)}
    tok = _WordTokenizer()
    args = SimpleNamespace(per_device_eval_batch_size=16, fp16=False, bf16=False)
    corpus_embeds, corpus_ids = encode_dense_corpus(corpus, model, tok, 32, args, split_corpus_num=7)
    assert corpus_embeds.dtype == np.float32 and corpus_embeds.shape == (400, 64) and sorted(corpus_ids) == sorted(corpus)
    lens = [len(corpus[c].split()) for c in corpus_ids]
    assert lens == sorted(lens, reverse=True)                        # longest first
    query_embeds, query_ids = encode_dense_query(queries, model, tok, 32, args)
    assert list(query_ids) == sorted(queries)
    collate = get_collator_func(tok, 32, "doc")
    with torch.no_grad():
        for j in (0, 137, 399):
            one = model(**{k: v.cuda() for k, v in collate([corpus[corpus_ids[j]]]).items()}).float().cpu().numpy()[0]
            assert np.allclose(corpus_embeds[j], one, atol=1e-4, rtol=1e-4)
        oneq = model(**{k: v.cuda() for k, v in collate([queries[query_ids[3]]]).items()}).float().cpu().numpy()[0]
        assert np.allclose(query_embeds[3], oneq, atol=1e-4, rtol=1e-4)
    index = create_index(corpus_embeds)
    assert index.ntotal == 400 and index.device.index == torch.cuda.current_device()
    scores, ids = batch_dense_search(query_ids, query_embeds, corpus_ids, index, 10, batch_size=8)
    ws, wi = oracle_topk(torch.from_numpy(corpus_embeds).cuda(), torch.from_numpy(query_embeds).cuda(), 10)
    assert np.array_equal(ids, corpus_ids[wi]) and np.array_equal(scores.view(np.uint32), ws.view(np.uint32))
    args16 = SimpleNamespace(per_device_eval_batch_size=16, fp16=False, bf16=True)
    e16, _ = encode_dense_query(queries, model, tok, 32, args16)
    assert e16.dtype == np.float32 and np.allclose(e16, query_embeds, atol=0.1)
