"""The fused JPQ scoring head (csrc/jpq_head.hip -> ops.jpq_scores -> JPQ(head="fused")): scores of (query, document id)
pairs straight from the resident uint8 codes, and their gradients w.r.t. the queries and the centroids.

The arithmetic is fixed on the output (include/repconc_hip.h, rc_jpq_head_*): every product is of two fp32 values taken in
fp64 (exact, 24 + 24 <= 53 bits), every sum is fp64, sequential from 0.0 in a stated order, rounded to fp32 once.  So the
yardstick is `restate` below: plain numpy loops over j, m, t and p in exactly those orders on float64 arrays, vectorised over
the other axes only, and the GPU results must equal it BIT FOR BIT (torch.equal; no tolerance in this file except the two the
issue names: rtol 1e-12 for the yardstick's own self-check against float64 autograd, and the existing band of the module
step, rtol 1e-4 / atol 1e-5 / loss 1e-4 relative, for fused against decode).

Pair counts off the kernels' chunk sizes (csrc/jpq_head.hip): the sort walks the nq*k pairs in tiles of JH_TILE = 1024, a wave
stepping 64 pairs at a time, and the forward gives a block 16 pairs; so nq*k = 1 (one lane of one step), 1023 and 1025 (one
less / one more than a tile: the last step is short / a second tile holds one pair), and the prime 1031 (no chunk size divides
it, two tiles).
"""
import functools
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import synth

gpu = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------ the yardstick
def restate(q, codes, pids, C, g=None):
    """float64 (scores, grad_q, grad_C) BEFORE the final rounding to fp32, in the orders of the header."""
    nq, D = q.shape
    M, K, dsub = C.shape
    N, k = codes.shape[0], pids.shape[1]
    q64, C64 = q.astype(F64), C.astype(F64)
    ok = (pids >= 0) & (pids < N)                                     # a hole: id outside [0, N)
    cd = codes[np.where(ok, pids, 0)] if N else np.zeros((nq, k, M), np.uint8)      # [nq, k, M]
    scores = np.zeros((nq, k), F64)
    for m in range(M):                                                # m ascending
        s = np.zeros((nq, k), F64)
        for j in range(dsub):                                         # j ascending
            s = s + q64[:, m * dsub + j][:, None] * C64[m, cd[:, :, m], j]
        scores = scores + s
    scores = np.where(ok, scores, 0.0)
    if g is None:
        return scores, None, None
    g64 = g.astype(F64)
    gq = np.zeros((nq, D), F64)
    for t in range(k):                                                # t ascending, holes skipped
        dec = C64[np.arange(M)[None, :], cd[:, t, :], :].reshape(nq, D)
        gq = np.where(ok[:, t][:, None], gq + g64[:, t][:, None] * dec, gq)
    gC = np.zeros((M, K, dsub), F64)
    marange = np.arange(M)
    for p in range(nq * k):                                           # flat pair index ascending, holes skipped
        i, t = divmod(p, k)
        if ok[i, t]:
            gC[marange, cd[i, t], :] = gC[marange, cd[i, t], :] + g64[i, t] * q64[i].reshape(M, dsub)
    return scores, gq, gC


def _rand_case(seed, D, M, N, nq, k):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nq, D), dtype=F32)
    C = rng.standard_normal((M, 256, D // M), dtype=F32)
    codes = rng.integers(0, 256, size=(N, M), dtype=np.uint8)
    pids = rng.integers(0, max(N, 1), size=(nq, k)).astype(np.int64)
    g = rng.standard_normal((nq, k), dtype=F32)
    return q, codes, pids, C, g


# ------------------------------------------------------------------------------------------------------ CPU tests
def test_yardstick_equals_float64_autograd_on_a_small_case():
    D, M, N, nq, k = 24, 4, 50, 3, 7
    q, codes, pids, C, g = _rand_case(11, D, M, N, nq, k)
    pids[1, 2] = -1                                                   # one hole
    pids[2, 5] = pids[2, 1]                                           # one repeated id
    s, gq, gC = restate(q, codes, pids, C, g)
    tq = torch.from_numpy(q).double().requires_grad_(True)
    tC = torch.from_numpy(C).double().requires_grad_(True)
    ok = torch.from_numpy((pids >= 0) & (pids < N))
    rows = torch.from_numpy(codes.astype(np.int64))[torch.from_numpy(np.where(ok.numpy(), pids, 0)).reshape(-1)]
    dec = torch.cat([tC[m, rows[:, m]] for m in range(M)], dim=1).reshape(nq, k, D)
    ts = (tq.unsqueeze(1) * dec).sum(-1) * ok
    (ts * torch.from_numpy(g).double()).sum().backward()
    np.testing.assert_allclose(s, ts.detach().numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(gq, tq.grad.numpy(), rtol=1e-12, atol=0)
    np.testing.assert_allclose(gC, tC.grad.numpy(), rtol=1e-12, atol=0)
    assert s[1, 2] == 0.0 and int((gC != 0).any(-1).sum()) <= (nq * k - 1) * M


def test_abi_exports_the_head_and_its_size_helper_needs_no_gpu():
    from repconc_amd import _lib
    lib = _lib.load()
    for name in ("rc_jpq_head_fwd", "rc_jpq_head_bwd", "rc_jpq_head_ws_bytes"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    M = 48
    sizes = [lib.rc_jpq_head_ws_bytes(nq, k, M) for nq, k in ((1, 1), (1, 2), (3, 7), (12, 50), (33, 31), (25, 41), (128, 201),
                                                              (4096, 1000))]
    assert sizes[0] >= 4 * M and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    assert sizes[-1] >= 4 * M * 4096 * 1000                       # one uint32 slot per (sub-quantiser, pair)
    assert lib.rc_jpq_head_ws_bytes(0, 5, M) == 0 and lib.rc_jpq_head_ws_bytes(5, 0, M) == 0
    from repconc_amd import ops
    assert ops.jpq_head_ws_bytes(12, 50, M) == sizes[3]


def test_op_and_module_refuse_bad_arguments():
    from repconc_amd import _lib, ops
    from repconc_amd.models.jpq import JPQ
    q, codes, pids, C = torch.zeros(3, 32), torch.zeros(10, 4, dtype=torch.uint8), torch.zeros(3, 5, dtype=torch.int64), torch.zeros(4, 256, 8)
    with pytest.raises(_lib.RepconcHipError):
        ops.jpq_scores(q, codes, pids, C)                             # CPU tensors
    for bad in ((q[0], codes, pids, C), (q, codes[0], pids, C), (q, codes, pids[0], C), (q, codes, pids, C[0]),      # ranks
                (q, codes.long(), pids, C), (q, codes.int(), pids, C),                                               # codes dtype
                (q, codes, pids.int(), C), (q, codes, pids.float(), C),                                              # pids dtype
                (q, codes, pids, torch.zeros(4, 128, 8)), (q, codes, pids, torch.zeros(4, 256, 4)),                  # centroids
                (q, codes, pids, torch.zeros(8, 256, 4)), (q, codes, pids[:2], C)):
        with pytest.raises(ValueError):
            ops.jpq_scores(*bad)
    with pytest.raises(ValueError):
        JPQ(None, None, {}, 10, 1.0, head="nope")


# ------------------------------------------------------------------------------------------------------ GPU tests
def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # a copy: the shared cases stay as they are


def _run(q, codes, pids, C, g, want_q=True, want_c=True):
    from repconc_amd import ops
    tq, tC = _t(q).requires_grad_(want_q), _t(C).requires_grad_(want_c)
    s = ops.jpq_scores(tq, _t(codes), _t(pids), tC)
    s.backward(_t(g))
    return s.detach().cpu(), (tq.grad.cpu() if want_q else tq.grad), (tC.grad.cpu() if want_c else tC.grad)


def _check(q, codes, pids, C, g):
    """scores, grad_q and grad_C bit-equal to the restatement; returns the three GPU results."""
    ws, wq, wc = restate(q, codes, pids, C, g)
    s, gq, gc = _run(q, codes, pids, C, g)
    assert s.dtype == gq.dtype == gc.dtype == torch.float32
    assert torch.equal(s, torch.from_numpy(ws.astype(F32)))
    assert torch.equal(gq, torch.from_numpy(wq.astype(F32)))
    assert torch.equal(gc, torch.from_numpy(wc.astype(F32)))
    return s, gq, gc


@functools.lru_cache(maxsize=None)
def _ordinary():
    """D = 768, M = 48, N = 2000 clustered documents under their nearest codes, 12 queries x 50 ids."""
    from repconc_amd import ops
    D, M, N, nq, k = 768, 48, 2000, 12, 50
    docs = synth.clustered_embeddings(901, N)
    C = synth.sample_centroids(902, docs, M)
    codes = ops.assign_nearest(_t(docs), _t(C), torch.uint8).cpu().numpy()
    rng = np.random.default_rng(903)
    q = docs[rng.integers(0, N, nq)] + 0.05 * rng.standard_normal((nq, D), dtype=F32)
    pids = rng.integers(0, N, size=(nq, k)).astype(np.int64)
    g = rng.standard_normal((nq, k), dtype=F32)
    for a in (q, codes, pids, C, g):
        a.setflags(write=False)
    return q, codes, pids, C, g


@gpu
def test_ordinary_shape_is_bit_equal_and_repeats_bit_identically():
    case = _ordinary()
    _, gq0, gc0 = _check(*case)
    for _ in range(4):                                                # five backward runs in all
        _, gq, gc = _run(*case)
        assert torch.equal(gq, gq0) and torch.equal(gc, gc0)


@gpu
@pytest.mark.parametrize("D,M", [(768, 96), (768, 128), (24, 24), (16, 1)])
def test_widths_where_indexing_can_go_wrong(D, M):
    _check(*_rand_case(1000 + M, D, M, 500, 5, 9))


@gpu
def test_one_long_segment_and_255_empty_ones_with_the_sign_of_zero():
    D, M, N, nq, k = 768, 48, 300, 8, 64
    q, codes, pids, C, g = _rand_case(77, D, M, N, nq, k)
    codes[:] = codes[0]                                               # every row identical: one segment of 512 pairs per m
    _, _, gc = _check(q, codes, pids, C, g)
    hit = np.zeros((M, 256), bool)
    hit[np.arange(M), codes[0]] = True
    empty = gc.numpy()[~hit]
    assert empty.shape == (M * 255, D // M)
    assert (empty == 0).all() and not np.signbit(empty).any()          # exactly +0.0


@gpu
def test_repeats_and_holes():
    D, M, N, nq, k = 768, 48, 400, 6, 10
    q, codes, pids, C, g = _rand_case(78, D, M, N, nq, k)
    pids[:, 0] = 17                                                   # the same id in several queries
    pids[1, 3] = pids[1, 7] = 123                                     # the same id twice in one row
    pids[2, 4], pids[2, 5], pids[0, 9] = -1, N, N + 5                 # holes below and above
    pids[4, :] = np.where(np.arange(k) % 2 == 0, -1, N)               # a whole row of holes
    s, gq, _ = _check(q, codes, pids, C, g)
    holes = (pids < 0) | (pids >= N)
    sn = s.numpy()
    assert (sn[holes] == 0).all() and not np.signbit(sn[holes]).any()
    assert (gq.numpy()[4] == 0).all() and not np.signbit(gq.numpy()[4]).any()
    # a NaN centroid that only holes could "read" must not leak: code 0 is what a hole's lane would fetch
    C2 = C.copy()
    C2[:, 0, :] = np.nan
    codes2 = np.where(codes == 0, 1, codes).astype(np.uint8)
    s2, gq2, gc2 = _check(q, codes2, pids, C2, g)
    assert torch.isfinite(s2).all() and torch.isfinite(gq2).all() and torch.isfinite(gc2).all()


@gpu
@pytest.mark.parametrize("nq,k", [(5, 1), (1, 9)])
def test_single_column_and_single_query(nq, k):
    _check(*_rand_case(300 + nq, 64, 8, 200, nq, k))


@gpu
@pytest.mark.parametrize("nq,k", [(0, 4), (3, 0)])
def test_empty_outputs_have_the_right_shape_and_dtype(nq, k):
    q, codes, pids, C, g = _rand_case(5, 64, 8, 200, nq, k)
    s, gq, gc = _run(q, codes, pids, C, g)
    assert s.shape == (nq, k) and s.dtype == torch.float32
    assert gq.shape == (nq, 64) and gq.dtype == torch.float32 and not gq.any()
    assert gc.shape == (8, 256, 8) and gc.dtype == torch.float32 and not gc.any()


@gpu
def test_non_contiguous_inputs_and_one_sided_gradients():
    from repconc_amd import ops
    D, M, N, nq, k = 96, 8, 300, 7, 11
    q, codes, pids, C, g = _rand_case(41, D, M, N, nq, k)
    ws, wq, wc = restate(q, codes, pids, C, g)
    wide = np.concatenate([np.full((nq, 3), 9.0, F32), q, np.full((nq, 5), 9.0, F32)], 1)
    base_q = _t(wide).requires_grad_(True)
    qv = base_q[:, 3:3 + D]                                           # a column slice: row stride D + 8
    padded = np.full((k + 3, nq + 2), N - 1, np.int64)
    padded[2:2 + k, 1:1 + nq] = pids.T
    pv = _t(padded).t()[1:1 + nq, 2:2 + k]                            # transposed, then sliced
    assert not qv.is_contiguous() and not pv.is_contiguous()
    tC = _t(C).requires_grad_(True)
    dcodes = _t(codes)
    s = ops.jpq_scores(qv, dcodes, pv, tC)
    saved = [x.data_ptr() for x in s.grad_fn.saved_tensors]
    s.backward(_t(g))
    assert torch.equal(s.detach().cpu(), torch.from_numpy(ws.astype(F32)))
    assert torch.equal(base_q.grad[:, 3:3 + D].cpu(), torch.from_numpy(wq.astype(F32)))
    assert not base_q.grad[:, :3].any() and not base_q.grad[:, 3 + D:].any()
    assert torch.equal(tC.grad.cpu(), torch.from_numpy(wc.astype(F32)))
    # the tensors kept for the backward are the caller's, not copies
    cp = _t(pids)
    s3 = ops.jpq_scores(_t(q).requires_grad_(True), dcodes, cp, tC)
    saved3 = [x.data_ptr() for x in s3.grad_fn.saved_tensors]
    assert dcodes.data_ptr() in saved and dcodes.data_ptr() in saved3 and cp.data_ptr() in saved3
    # one-sided gradients
    _, gq, gc = _run(q, codes, pids, C, g, want_q=False)
    assert gq is None and torch.equal(gc, torch.from_numpy(wc.astype(F32)))
    _, gq, gc = _run(q, codes, pids, C, g, want_c=False)
    assert gc is None and torch.equal(gq, torch.from_numpy(wq.astype(F32)))
    with torch.no_grad():
        assert torch.equal(ops.jpq_scores(_t(q), dcodes, cp, _t(C)).cpu(), torch.from_numpy(ws.astype(F32)))


@gpu
@pytest.mark.parametrize("nq,k", [(1, 1), (33, 31), (25, 41), (1, 1031), (1031, 1)])
def test_pair_counts_off_every_chunk_size(nq, k):
    """nq*k = 1, 1023 = JH_TILE - 1, 1025 = JH_TILE + 1 and the prime 1031 (as one long row and as 1031 rows of one pair);
    few codes per sub-quantiser, so segments are long and cross the tile and the 64-pair step boundaries."""
    q, codes, pids, C, g = _rand_case(500 + nq, 48, 6, 300, nq, k)
    codes %= 5
    if nq * k > 1:
        pids.reshape(-1)[::97] = -1                                    # holes scattered over the steps
    _check(q, codes, pids, C, g)


# ------------------------------------------------------------------------------------------------------ module
@functools.lru_cache(maxsize=None)
def _module_inputs():
    N = 20000
    docs = synth.clustered_embeddings(515, N)
    C = synth.sample_centroids(516, docs[:4096], 48)
    return docs, C


def _module_step(head, N):
    """One JPQ step of the fixture of test_gpu_parity's module test (M = 48, nq = 12, k = 50, the table encoder) over the first
    N documents; everything seeded, so two calls see the same model, negatives and positives."""
    from repconc_amd.index import PQIndex
    from repconc_amd.models.jpq import JPQ
    from repconc_amd.models.repconc import RepCONC
    M, nq, k = 48, 12, 50
    docs_np, C_np = _module_inputs()
    docs, C = _t(docs_np[:N]), _t(C_np)
    torch.manual_seed(7)
    cfg = SimpleNamespace(MCQ_M=M, MCQ_K=256, hidden_size=768, similarity_metric="METRIC_IP")

    class _Enc(torch.nn.Module):
        def __init__(self, table):
            super().__init__()
            self.table = torch.nn.Parameter(table.clone())
            self.config = SimpleNamespace(hidden_size=768)

        def forward(self, input_ids, attention_mask):
            return self.table[input_ids[:, 0]]

    qtable = docs[torch.randperm(max(N, 64), device=DEV)[:64] % N] + 0.05 * torch.randn(64, 768, device=DEV)
    model = RepCONC(cfg, _Enc(qtable), False, 0.003, 100).to(DEV)
    with torch.no_grad():
        model.centroids.copy_(C)
    index = PQIndex(768, M, device=DEV)
    index.set_centroids(C)
    index.add(docs)
    codes_ptr = index.codes.data_ptr()
    qrels = {q: [int(3 * q) % N, int(3 * q + 1) % N] for q in range(64)}
    jpq = JPQ(model, index, qrels, neg_top_k=k, temperature=1.0, head=head)
    qids = torch.arange(nq, device=DEV)
    ids = qids[:, None].repeat(1, 4)
    random.seed(99)
    loss = jpq(ids, torch.ones_like(ids), qids)["loss"]
    loss.backward()
    assert index.codes.data_ptr() == codes_ptr
    return loss.detach().cpu(), model.dense_encoder.table.grad.cpu(), model.centroids.grad.cpu()


@gpu
@pytest.mark.parametrize("N", [20000, 30])
def test_module_fused_head_agrees_with_decode_head_and_is_reproducible(N):
    """N = 30 < k = 50: the search pads with -1, holes of the fused head, which must not move the loss."""
    ld, td, cd = _module_step("decode", N)
    lf, tf, cf = _module_step("fused", N)
    assert torch.isfinite(lf) and abs(float(lf) - float(ld)) < 1e-4 * max(1.0, abs(float(ld)))
    torch.testing.assert_close(tf, td, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(cf, cd, rtol=1e-4, atol=1e-5)
    l2, t2, c2 = _module_step("fused", N)
    assert torch.equal(l2, lf) and torch.equal(t2, tf) and torch.equal(c2, cf)
