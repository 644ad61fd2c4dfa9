"""The deterministic backward of decode (csrc/decode_det.hip + csrc/code_sort.h -> rc_pq_decode_bwd_det ->
ops.decode(..., deterministic=True) -> RepCONC.deterministic_decode / JPQ(head="decode")): the centroid gradient summed in a
fixed order, without atomics on values.

The arithmetic is fixed on the output (include/repconc_hip.h, rc_pq_decode_bwd_det):

    grad_C[m, c, j] = fp32( sum over the rows r with (codes[r, m] & 255) == c, r ascending, of (double) grad_out[r, m*dsub + j] )

every sum fp64, sequential from 0.0, rounded to fp32 once; an (m, c) no row hits is +0.0f.  The yardstick is `restate` below:
a plain numpy loop over the rows in ascending order on a float64 array (vectorised over m and j only: the elements of different
m or j are different sums, so this is the per-m loop of the contract), and the GPU result must equal it BIT FOR BIT — torch.equal
plus the sign bits; there is no tolerance in this file except the three that are stated where they are used: rtol 1e-12 for the
yardstick's own self-check against float64 autograd, the derived bound of the atomics path, (count + 1) * 2^-24 * sum|grad_out|,
and the decode head's existing band of the module step (rtol 1e-4, atol 1e-5).

Row counts off the sort's chunk sizes (csrc/code_sort.h): tiles of CS_TILE = 1024 rows, a wave stepping 64 rows at a time, four
waves (sub-quantisers) per block.
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
def restate(codes, go, M, dsub):
    """float64 grad_C [M, 256, dsub] BEFORE the final rounding to fp32: rows in ascending order, every add in float64."""
    n = codes.shape[0]
    cd = codes.astype(np.int64) & 255                                 # the low 8 bits of either dtype (-1 reads as 255)
    go64 = np.ascontiguousarray(go).reshape(n, M, dsub).astype(F64)
    gC = np.zeros((M, 256, dsub), F64)
    ma = np.arange(M)
    for r in range(n):                                                # r ascending; (m, cd[r, m]) is a different element per m
        gC[ma, cd[r]] = gC[ma, cd[r]] + go64[r]
    return gC


def _case(seed, n, M, dsub, few=True):
    """uint8 codes and fp32 grad_out; with `few`, every other column holds 5 codes only, so segments are long and cross the
    64-row steps and the tiles."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, size=(n, M), dtype=np.uint8)
    if few:
        codes[:, ::2] %= 5
    go = rng.standard_normal((n, M * dsub), dtype=F32)
    return codes, go


def ws_formula(n, M):
    up = lambda v: (v + 255) // 256 * 256
    return up(4 * M * ((n + 1023) // 1024) * 256) + 2 * up(4 * M * 256) + up(4 * M * n)


# ------------------------------------------------------------------------------------------------------ CPU tests
def test_yardstick_equals_float64_autograd_of_the_gather_on_a_small_case():
    n, M, dsub = 50, 4, 6
    codes, go = _case(3, n, M, dsub, few=False)
    codes[:, 2] = 9                                                   # one repeated code column: a segment of all 50 rows
    got = restate(codes, go, M, dsub)
    tC = torch.zeros(M, 256, dsub, dtype=torch.float64, requires_grad=True)
    idx = torch.from_numpy(codes.astype(np.int64))
    dec = torch.cat([tC[m, idx[:, m]] for m in range(M)], dim=1)      # the gather of modeling_repconc.py:175
    dec.backward(torch.from_numpy(go).double())
    np.testing.assert_allclose(got, tC.grad.numpy(), rtol=1e-12, atol=0)
    assert (got[2, 9] != 0).all() and not got[2, :9].any() and not got[2, 10:].any()


def test_abi_has_the_two_entries_and_the_size_helper_is_the_stated_formula():
    from repconc_amd import _lib, ops
    lib = _lib.load()
    for name in ("rc_pq_decode_bwd_det", "rc_pq_decode_bwd_det_ws_bytes"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    for n, M in ((1, 1), (1024, 48), (1025, 48), (49152, 96)):
        assert lib.rc_pq_decode_bwd_det_ws_bytes(n, M) == ws_formula(n, M) == ops.decode_bwd_ws_bytes(n, M)
    assert lib.rc_pq_decode_bwd_det_ws_bytes(0, 48) == 0 and lib.rc_pq_decode_bwd_det_ws_bytes(5, 0) == 0
    assert lib.rc_pq_decode_bwd_det_ws_bytes(2 ** 31, 48) == 0 and lib.rc_pq_decode_bwd_det_ws_bytes(2 ** 31 - 1, 1) > 0
    # the same sort, the same workspace: n rows here are nq * k pairs of the JPQ head
    assert lib.rc_pq_decode_bwd_det_ws_bytes(25728, 48) == lib.rc_jpq_head_ws_bytes(128, 201, 48)


def test_cpu_tensors_are_rejected_loudly_with_the_switch_too():
    from repconc_amd import _lib, ops
    from repconc_amd.models.repconc import decode
    codes = torch.zeros(4, 48, dtype=torch.int64)
    for C in (torch.zeros(48, 256, 16), torch.zeros(48, 256, 16, requires_grad=True)):
        for det in (True, False, None):
            with pytest.raises(_lib.RepconcHipError):
                ops.decode(codes, C, deterministic=det)
        with pytest.raises(_lib.RepconcHipError):
            decode(codes, C, deterministic=True)


def test_the_switch_is_a_plain_attribute_and_a_training_argument():
    import dataclasses
    import inspect
    from repconc_amd.models.repconc import RepCONC
    from repconc_amd.models.repconc.finetune_repconc import RepCONCFinetuneArguments
    assert RepCONC.deterministic_decode is None
    assert "deterministic_decode" not in inspect.signature(RepCONC.__init__).parameters
    f = {x.name: x for x in dataclasses.fields(RepCONCFinetuneArguments)}["deterministic_decode"]
    assert f.default is False


# ------------------------------------------------------------------------------------------------------ GPU helpers
def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # a copy: the shared cases stay as they are


def _entry(codes, go, M, dsub, prefill=float("nan")):
    """rc_pq_decode_bwd_det called directly on a grad_C pre-filled with `prefill`: the entry overwrites."""
    from repconc_amd import ops
    tc, tg = _t(codes), _t(go)
    n = tc.shape[0]
    gC = torch.full((M, 256, dsub), prefill, dtype=torch.float32, device=DEV)
    lib, h, s, _ = ops._ctx(tg)
    wsb = lib.rc_pq_decode_bwd_det_ws_bytes(n, M)
    ws = torch.empty((max(wsb, 1),), dtype=torch.uint8, device=DEV)
    rc = lib.rc_pq_decode_bwd_det(h, ops._p(tc), ops._code_dtype(tc), ops._p(tg), n, M, 256, dsub, ops._p(gC), ops._p(ws), wsb, s)
    assert rc == 0, rc
    return gC.cpu()


def _autograd(codes, go, M, dsub, deterministic):
    from repconc_amd import ops
    C = torch.zeros(M, 256, dsub, device=DEV, requires_grad=True)
    ops.decode(_t(codes), C, deterministic=deterministic).backward(go if isinstance(go, torch.Tensor) else _t(go))
    return C.grad.cpu()


def _same_bits(got, want64):
    want = want64.astype(F32)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    g = got.numpy()
    assert torch.equal(got, torch.from_numpy(want)), f"{int((g != want).sum())} of {want.size} elements differ"
    assert np.array_equal(np.signbit(g), np.signbit(want))


def _check(codes, go, M, dsub):
    got = _entry(codes, go, M, dsub)
    _same_bits(got, restate(codes, go, M, dsub))
    return got


# ------------------------------------------------------------------------------------------------------ GPU tests
@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 1031, 2049])
def test_row_counts_off_the_tile_and_the_wave_step(n):
    _check(*_case(100 + n, n, 48, 16), 48, 16)


@gpu
@pytest.mark.parametrize("M,dsub", [(96, 8), (128, 6), (24, 1), (1, 16), (3, 4), (5, 4)])
def test_widths_where_indexing_can_go_wrong(M, dsub):
    """dsub = 6 is no multiple of 4, dsub = 1 makes D = M; M = 1, 3, 5 are off the four waves of a sort block (dead waves)."""
    _check(*_case(200 + M, 1031, M, dsub), M, dsub)


@gpu
def test_one_segment_beside_255_empty_ones_overwrites_with_plus_zero():
    n, M, dsub = 1025, 48, 16
    codes, go = _case(31, n, M, dsub)
    codes[:] = codes[0]                                               # every row the same code: one segment of 1025 rows per m
    want = restate(codes, go, M, dsub)
    hit = np.zeros((M, 256), bool)
    hit[np.arange(M), codes[0]] = True
    for prefill in (0.0, float("nan")):
        got = _entry(codes, go, M, dsub, prefill=prefill)
        _same_bits(got, want)
        empty = got.numpy()[~hit]
        assert empty.shape == (M * 255, dsub)
        assert (empty == 0).all() and not np.signbit(empty).any()      # exactly +0.0f, whatever grad_C held before


@gpu
def test_sorted_reversed_and_alternating_code_columns():
    n, M, dsub = 1031, 6, 8
    codes, go = _case(41, n, M, dsub, few=False)
    r = np.arange(n)
    codes[:, 0] = np.sort(codes[:, 0])                                # ascending: every segment one contiguous run
    codes[:, 1] = np.sort(codes[:, 1])[::-1]                          # descending
    codes[:, 2] = np.where(r % 2 == 0, 7, 200)                        # two codes alternating inside every 64-row step
    codes[:, 3] = np.where((r // 3) % 2 == 0, 255, 0)                 # ... in runs of three, the extreme codes
    codes[:, 4] = (r % 64) * 4                                        # 64 different codes in every step
    _check(codes, go, M, dsub)


@gpu
def test_int64_codes_with_high_bits_read_as_their_low_byte():
    n, M, dsub = 1031, 5, 4
    low, go = _case(51, n, M, dsub)
    rng = np.random.default_rng(52)
    wide = low.astype(np.int64) + 256 * rng.integers(-2 ** 40, 2 ** 40, size=low.shape)
    wide[::7, 1] = -1                                                 # reads as code 255
    wide[3::11, 3] = -256                                             # reads as code 0
    low8 = (wide & 255).astype(np.uint8)
    assert (wide < 0).any() and (wide > 2 ** 32).any() and low8[0, 1] == 255
    g64 = _check(wide, go, M, dsub)
    g8 = _check(low8, go, M, dsub)
    assert torch.equal(g64, g8) and np.array_equal(np.signbit(g64.numpy()), np.signbit(g8.numpy()))


@gpu
def test_cancellation_denormals_and_minus_zero_need_the_stated_order_in_fp64():
    """Segments of +2^24, +1, -2^24 in several orders: the fp64 sum is 1 in any order, an fp32 sum is 0 or 1 depending on the
    order, so only fp64 accumulation gives the yardstick's bits.  Plus segments of denormals, of -0.0 alone (+0.0: the sum
    starts from +0.0) and one whose sum is a denormal reached through normal terms."""
    big, tiny = F32(2.0 ** 24), F32(1e-45)
    segs = {
        0: [big, 1, -big], 1: [1, big, -big], 2: [big, -big, 1], 3: [big, 1, 1, -big, 1], 4: [-big, -1, big, 1, 1],
        5: [tiny, tiny, tiny], 6: [-0.0, -0.0], 7: [F32(2.0 ** -126), tiny, -F32(2.0 ** -126)], 8: [-0.0, tiny, -tiny],
        9: [big, F32(0.5), F32(0.5), -big], 10: [F32(3.0e38), F32(3.0e38), -F32(3.0e38)],      # the partial sum leaves fp32's range
    }
    # segments interleaved round-robin; each keeps its own order
    rows = [(c, vals[i]) for i in range(max(map(len, segs.values()))) for c, vals in segs.items() if i < len(vals)]
    n, M, dsub = len(rows), 3, 2
    codes = np.zeros((n, M), np.uint8)
    go = np.zeros((n, M * dsub), F32)
    for r, (c, v) in enumerate(rows):
        codes[r] = (c, c + 100, 255 - c)
        go[r] = F32(v)
    for c, vals in segs.items():                                      # each segment kept its order
        assert [float(go[r, 0]) for r in range(n) if codes[r, 0] == c] == [float(F32(v)) for v in vals]
    want = restate(codes, go, M, dsub)
    assert np.isfinite(want.astype(F32)).all()
    naive = np.zeros((M, 256, dsub), F32)                             # the same order in fp32: other bits
    with np.errstate(over="ignore"):
        for r in range(n):
            naive[np.arange(M), codes[r]] += go[r].reshape(M, dsub)
    assert (naive != want.astype(F32)).any()
    got = _entry(codes, go, M, dsub)
    _same_bits(got, want)
    g = got.numpy()
    assert g[0, 0, 0] == 1 and g[0, 1, 0] == 1 and g[0, 3, 0] == 3 and g[0, 9, 0] == 1
    assert g[0, 5, 0] == 3 * tiny and g[0, 7, 0] == tiny and g[0, 10, 0] == F32(3.0e38)
    assert g[0, 6, 0] == 0 and not np.signbit(g[0, 6, 0]) and g[0, 8, 0] == 0 and not np.signbit(g[0, 8, 0])


@functools.lru_cache(maxsize=None)
def _long_case():
    n, M, dsub = 70001, 48, 4
    codes, go = _case(71, n, M, dsub)
    want = restate(codes, go, M, dsub)
    for a in (codes, go, want):
        a.setflags(write=False)
    return codes, go, want


@gpu
@pytest.mark.parametrize("max_grid", [None, 3])
def test_grid_stride_walk(max_grid, monkeypatch):
    """n = 70 001 rows (69 tiles, a last tile of 369 rows, a last step of 49), M = 48.  The caps of the launch grids are
    CS_MAX_GRID = 65536 blocks (csrc/code_sort.h) for the sort and the reducer alike; at this shape the sort has 69 * 12 = 828
    work items, the scan 48 and the reducer 192 blocks, all below the cap, so the second run forces the grids small through
    the entry's hook, RC_DECODE_DET_MAX_GRID = 3 blocks per launch (read on every call): every kernel then walks its
    grid-stride loop many times, with a remainder (828, 48 and 192 are multiples of 3; 70 001 rows are not of anything)."""
    codes, go, want = _long_case()
    if max_grid is not None:
        monkeypatch.setenv("RC_DECODE_DET_MAX_GRID", str(max_grid))
    _same_bits(_entry(codes, go, 48, 4), want)


@functools.lru_cache(maxsize=None)
def _step_case():
    """One chunk of a stage-1 step: 6 144 rows, M = 48, D = 768, uniform codes (segments of ~24 rows)."""
    n, M, dsub = 6144, 48, 16
    codes, go = _case(81, n, M, dsub, few=False)
    want = restate(codes, go, M, dsub)
    for a in (codes, go, want):
        a.setflags(write=False)
    return codes, go, want


@gpu
def test_five_backward_calls_give_identical_bits():
    codes, go, want = _step_case()
    first = _entry(codes, go, 48, 16)
    _same_bits(first, want)
    for _ in range(4):
        again = _entry(codes, go, 48, 16)
        assert torch.equal(again, first) and np.array_equal(np.signbit(again.numpy()), np.signbit(first.numpy()))


def _atomic_bound(codes, go, M, dsub):
    """(count + 1) * 2^-24 * sum|grad_out| per element, count and the sum over the element's segment: every fp32 add of the
    atomics path errs by at most half an ulp of a partial sum no larger than sum|.| (count adds), plus the final rounding of
    the deterministic result."""
    count = np.stack([np.bincount(codes[:, m].astype(np.int64) & 255, minlength=256) for m in range(M)])      # [M, 256]
    return (count[:, :, None] + 1) * 2.0 ** -24 * restate(codes, np.abs(go), M, dsub)


@gpu
def test_atomics_path_is_within_its_derived_bound_of_the_deterministic_one():
    codes, go, want = _step_case()
    det = _entry(codes, go, 48, 16).numpy().astype(F64)
    atomic = _autograd(codes, go, 48, 16, deterministic=False).numpy().astype(F64)
    bound = _atomic_bound(codes, go, 48, 16)
    assert (np.abs(det - atomic) <= bound).all(), float((np.abs(det - atomic) - bound).max())


@gpu
def test_refusals_of_the_entry():
    from repconc_amd import _lib, ops
    codes, go = _case(91, 10, 4, 4)
    tc, tg = _t(codes), _t(go)
    gC = torch.full((4, 256, 4), 7.0, device=DEV)
    lib, h, s, _ = ops._ctx(tg)
    wsb = lib.rc_pq_decode_bwd_det_ws_bytes(10, 4)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=DEV)
    call = lambda n=10, M=4, K=256, dsub=4, w=ws, wb=wsb, dt=_lib.RC_CODE_U8, g=gC: lib.rc_pq_decode_bwd_det(
        h, ops._p(tc), dt, ops._p(tg), n, M, K, dsub, ops._p(g), ops._p(w), wb, s)
    assert call(wb=wsb - 1) == _lib.RC_EWORKSPACE and call(w=None) == _lib.RC_EWORKSPACE
    assert call(n=2 ** 31) == _lib.RC_ESHAPE and call(K=128) == _lib.RC_ESHAPE
    assert call(n=-1) == _lib.RC_EINVAL and call(M=0) == _lib.RC_EINVAL and call(dsub=0) == _lib.RC_EINVAL
    assert call(dt=7) == _lib.RC_EINVAL and call(g=None) == _lib.RC_EINVAL
    assert call(n=0, w=None, wb=0) == _lib.RC_OK
    torch.cuda.synchronize()
    assert (gC == 7.0).all()                                          # nothing above wrote grad_C
    assert call() == _lib.RC_OK
    _same_bits(gC.cpu(), restate(codes, go, 4, 4))


@gpu
def test_through_autograd_with_the_keyword():
    n, M, dsub = 1031, 48, 16
    codes, go = _case(101, n, M, dsub)
    want = restate(codes, go, M, dsub)
    _same_bits(_autograd(codes, go, M, dsub, deterministic=True), want)
    wide = torch.full((n, 2 * M * dsub), 9.0, device=DEV)
    wide[:, ::2] = _t(go)
    strided = wide[:, ::2]                                            # a non-contiguous grad_out
    assert not strided.is_contiguous()
    _same_bits(_autograd(codes, strided, M, dsub, deterministic=True), want)
    _same_bits(_autograd(codes.astype(np.int64), go, M, dsub, deterministic=True), want)
    empty = _autograd(codes[:0], go[:0], M, dsub, deterministic=True)
    assert empty.shape == (M, 256, dsub) and empty.dtype == torch.float32 and not empty.any()
    assert not np.signbit(empty.numpy()).any()


@gpu
def test_none_follows_the_deterministic_algorithms_flag(monkeypatch):
    from repconc_amd import _lib, ops
    n, M, dsub = 1031, 48, 16
    codes, go = _case(111, n, M, dsub)
    want = restate(codes, go, M, dsub)
    tc, tg = _t(codes), _t(go)
    C = torch.zeros(M, 256, dsub, device=DEV, requires_grad=True)
    assert not torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:                                                              # nothing but ops.decode and its backward runs under the flag
        ops.decode(tc, C, deterministic=None).backward(tg)
    finally:
        torch.use_deterministic_algorithms(False)
    _same_bits(C.grad.cpu(), want)
    # flag off: the atomics.  Which entry ran is counted; a block of NaNs freed just before (the allocator hands it out again)
    # must not matter, since that path adds into a zeroed buffer; and the result is within the atomics' bound of the yardstick
    lib = _lib.load()
    calls = {"det": 0, "atomic": 0}
    real_det, real_atomic = lib.rc_pq_decode_bwd_det, lib.rc_pq_decode_bwd
    monkeypatch.setattr(lib, "rc_pq_decode_bwd_det", lambda *a: (calls.__setitem__("det", calls["det"] + 1), real_det(*a))[1])
    monkeypatch.setattr(lib, "rc_pq_decode_bwd", lambda *a: (calls.__setitem__("atomic", calls["atomic"] + 1), real_atomic(*a))[1])
    C2 = torch.zeros(M, 256, dsub, device=DEV, requires_grad=True)
    out = ops.decode(tc, C2, deterministic=None)
    junk = torch.full((M, 256, dsub), float("nan"), device=DEV)
    del junk
    out.backward(tg)
    assert calls == {"det": 0, "atomic": 1}
    atomic = C2.grad.cpu().numpy().astype(F64)
    assert np.isfinite(atomic).all()
    assert (np.abs(atomic - want.astype(F32).astype(F64)) <= _atomic_bound(codes, go, M, dsub)).all()
    C3 = torch.zeros(M, 256, dsub, device=DEV, requires_grad=True)
    ops.decode(tc, C3, deterministic=True).backward(tg)
    assert calls == {"det": 1, "atomic": 1}
    _same_bits(C3.grad.cpu(), want)


# ------------------------------------------------------------------------------------------------------ modules
class _Enc(torch.nn.Module):
    def __init__(self, table):
        super().__init__()
        self.table = torch.nn.Parameter(table.clone())
        self.config = SimpleNamespace(hidden_size=768)

    def forward(self, input_ids, attention_mask):
        return self.table[input_ids[:, 0]]


def _cfg(M):
    return SimpleNamespace(MCQ_M=M, MCQ_K=256, hidden_size=768, similarity_metric="METRIC_IP")


@gpu
def test_repconc_decode_with_the_attribute_gives_a_reproducible_mse_gradient():
    from repconc_amd.models.repconc import RepCONC
    n, M, dsub = 1500, 48, 16
    rng = np.random.default_rng(121)
    codes = rng.integers(0, 256, size=(n, M)).astype(np.int64)
    codes[:, ::3] %= 4
    torch.manual_seed(5)
    model = RepCONC(_cfg(M), _Enc(torch.zeros(4, 768)), False, 0.003, 100).to(DEV)
    assert model.deterministic_decode is None
    model.deterministic_decode = True
    assert "deterministic_decode" not in model.state_dict()
    target = _t(rng.standard_normal((n, M * dsub), dtype=F32))
    grads, seen = [], []
    for _ in range(2):
        model.centroids.grad = None
        dec = model.decode(_t(codes))
        dec.register_hook(lambda g: seen.append(g.detach().cpu().numpy()))
        torch.nn.functional.mse_loss(dec, target).backward()
        grads.append(model.centroids.grad.cpu())
    assert np.array_equal(seen[0], seen[1])
    assert torch.equal(grads[0], grads[1]) and np.array_equal(np.signbit(grads[0].numpy()), np.signbit(grads[1].numpy()))
    _same_bits(grads[0], restate(codes, seen[0], M, dsub))


@functools.lru_cache(maxsize=None)
def _module_inputs():
    N = 20000
    docs = synth.clustered_embeddings(515, N)
    C = synth.sample_centroids(516, docs[:4096], 48)
    return docs, C


def _jpq_step(deterministic):
    """One JPQ(head="decode") step over the index of tests/test_jpq_head.py's module test (20 000 clustered documents, M = 48,
    nq = 12, k = 50, the table encoder); everything seeded, so two calls see the same model, negatives and positives."""
    from repconc_amd.index import PQIndex
    from repconc_amd.models.jpq import JPQ
    from repconc_amd.models.repconc import RepCONC
    M, nq, k, N = 48, 12, 50, 20000
    docs_np, C_np = _module_inputs()
    docs, C = _t(docs_np), _t(C_np)
    torch.manual_seed(7)
    qtable = docs[torch.randperm(N, device=DEV)[:64] % N] + 0.05 * torch.randn(64, 768, device=DEV)
    model = RepCONC(_cfg(M), _Enc(qtable), False, 0.003, 100).to(DEV)
    if deterministic is not None:
        model.deterministic_decode = deterministic
    with torch.no_grad():
        model.centroids.copy_(C)
    index = PQIndex(768, M, device=DEV)
    index.set_centroids(C)
    index.add(docs)
    qrels = {q: [int(3 * q) % N, int(3 * q + 1) % N] for q in range(64)}
    jpq = JPQ(model, index, qrels, neg_top_k=k, temperature=1.0, head="decode")
    qids = torch.arange(nq, device=DEV)
    ids = qids[:, None].repeat(1, 4)
    random.seed(99)
    loss = jpq(ids, torch.ones_like(ids), qids)["loss"]
    loss.backward()
    return loss.detach().cpu(), model.centroids.grad.cpu()


@gpu
def test_jpq_decode_head_step_is_reproducible_with_the_attribute_and_stays_in_its_band_without():
    l1, c1 = _jpq_step(True)
    l2, c2 = _jpq_step(True)
    assert torch.isfinite(l1) and torch.equal(l1, l2)
    assert torch.equal(c1, c2) and np.array_equal(np.signbit(c1.numpy()), np.signbit(c2.numpy()))
    assert c1.abs().sum() > 0
    l0, c0 = _jpq_step(None)                                          # the attribute left alone: the atomics
    assert torch.equal(l0, l1)
    torch.testing.assert_close(c0, c1, rtol=1e-4, atol=1e-5)
