"""The quantiser's forward path at sub-vector widths off the divisors of 768: the three run-time-width routines of
csrc/pq_distance.hip (sqdist_exact_rt, dist_table_rt_kernel, assign_nearest_rt_kernel) behind ops.dist_table,
ops.assign_nearest (the exact entry and the fall-through of the fast one) and ops.assign_sinkhorn.

Every comparison is of fp32 bit patterns or of codes.  The only excuse rule is part C's: a constrained code may differ from the
C restatement where the reference's own fp64 plan ties (pq_oracle.codes_equal_up_to_fp64_ties, rtol 1e-9), at most CAP = 8
codes per case, as in tests/test_sinkhorn_strain.py.  Generators are module level, seeded, numpy on the CPU; the CPU tests check
that the inputs and the oracles are what they claim, and the oracle results are computed once per process and shared.

INPUTS.  Width cases: Gaussian rows x [B, M dsub] and Gaussian centroids C [M, 256, dsub], one (M, dsub) per entry of WIDTHS
(the reason for every width stands next to it there) and of REAL_SHAPES (a 312-wide and a 1024-wide encoder; 384 / 3).  M is 1,
3 or 5 on the WIDTHS so that D stays small and the offset m dsub takes unaligned values.  Rows: ROW_COUNTS, cut at
WORK_CAP = 3e8 element operations of the numpy oracle (dsub 8191: B <= 33); the table of the largest count is computed once,
a smaller count is its first rows.  B = 16384 + 77 (the 128-rows-per-block strip) runs at (M, dsub) = (3, 20) and at the
specialised (3, 16) only.

A (CPU).  pq_oracle.dist_table against torch-CPU's expression of the reference, bit for bit, at every width; the C oracle's
table and nearest codes against the numpy oracle; four wrong variants of the sum order (wrong_rowsum: a plain running sum, no
cascade, left-over vectors dealt to accumulator v % 4, the tail added after the lanes), each of which must change at least one
table entry of these very inputs at the widths meant to catch it (catches() states which and why: e.g. a cascade that fires
at the last round, dsub 519 / 520, or one round before it, 544, is the same sum as none, so only full >= 18 tells them apart);
the tie and non-finite families of part D under the numpy oracle.  No wrong kernel was built.
B (GPU).  ops.dist_table (d as uint32, minmax), ops.centre_, ops.assign_nearest (uint8 / int64, "exact" / "auto") at every width
and row count; a padded pitch ldx = D + 3 with NaN in the padding (which the wrapper copies: the pitch is no multiple of 4) and
the next pitch that is a multiple of 4 (which reaches the kernels); a contiguous view 4 bytes past a 16-byte boundary.
C (GPU).  ops.assign_sinkhorn at SK_SHAPES x SK_ROWS x SK_SETTINGS, Gaussian rows, centroids = 256 rows of the batch, against
c_oracle.quantize; RepCONC at hidden size 312, MCQ_M 8 and 24.  The CPU twin asserts that the C and numpy restatements agree
on every code of all 40 cases with nothing excused.
D (GPU).  Ties and non-finite values through the wave-shuffle reduction of assign_nearest_rt_kernel at dsub 20 and 39:
duplicate centroids at TIE_PAIRS (same wave, neighbouring waves, first and last wave), the upper copy one ulp nearer / farther
in coordinate 0, all 256 equal, NaN / +inf / -inf in one coordinate of the centroid at NONFINITE_POS, a row of NaN.  A NaN
distance is compared as a NaN (its payload is not part of the arithmetic contract), everything else as bits; minmax on finite
tables only.
E (GPU, launches nothing).  dsub 8192 is refused by ops.dist_table, ops.assign_nearest and ops.assign_sinkhorn.  Read first:
rc_pq_dist_table and rc_pq_assign_nearest return RC_ESHAPE from their argument checks; rc_pq_assign_nearest_fast hands a width
without a screen to rc_pq_assign_nearest before touching its workspace; rc_pq_assign_sinkhorn (and its multi-rank twin) now
checks the width next to D % M, before rc_solve_chains enqueues anything.  In the parent rc_solve_chains enqueued one 4-byte
memset and then met rc_pq_dist_table's refusal, and at B = 1 it answered code 0 without looking at the width; the refusal is
tested at B = 2 and B = 1.

The wrapper sends a width without a matrix-core screen straight to the exact entry (defect 2), so the fall-through of
rc_pq_assign_nearest_fast is called directly (_fast_entry) wherever _check_fp32_stage runs at such a width: the same codes, and
a workspace filled with 0xFF comes back untouched.

SUSPECTED DEFECTS, what was found and what changed.
1. oracle/pq_oracle.c kept the squares of one sub-vector in float sq[1024]: CONFIRMED by reading (the loop fills it up to dsub; the
   issue saw "stack smashing detected" at 1031; the parent's library was not run here).  The buffer holds 8191 floats now (orc_dsub_max, the HIP side's RC_DSUB_RT_MAX),
   orc_dist_table and orc_quantize return -1 and write nothing for a wider call, and c_oracle.dist_table / quantize raise
   ValueError first (test_c_oracle_refuses_a_width_past_its_buffer).
2. ops.assign_nearest(..., stats=d) at a width without a matrix-core screen read the doubt count from a workspace nothing had
   written: CONFIRMED on the MI355X (the parent's wrapper: method "mfma", doubtful -1, overflow True).  Such a width goes
   straight to rc_pq_assign_nearest now: no workspace, method "exact", doubtful 0 (test_statistics_at_a_width_without_a_screen).
3. ops._rows_f32 returned a contiguous tensor at a misaligned storage offset as it was: CONFIRMED on the MI355X (the parent's
   wrapper at the specialised width 16: "rc_pq_dist_table: invalid argument"; at the run-time widths 39 and 20 it passed, those
   kernels load scalars).  It clones now, as _centroids does (test_view_four_bytes_past_a_boundary).
4. ops.dist_table at B = 0 handed the entry a null pointer: CONFIRMED on the MI355X (the parent's wrapper: "rc_pq_dist_table:
   invalid argument" at both widths).  It launches nothing now and returns d [M, 0, 256] and the range (-inf, +inf) per
   sub-quantiser, the neutral pair solve_fill_range_kernel writes (test_empty_batch).
No kernel of csrc/pq_distance.hip changed.

WHAT THE PARENT COMMIT DID WITH THESE INPUTS.  CPU: the numpy oracle equals torch-CPU at every width; the C oracle died from
dsub 1025 on (defect 1).  GPU [MI355X]: profiles/quantize_widths_pytest_gpu.txt is this commit's run of this file (192 passed,
no constrained code excused, the slowest case 1.5 s).  profiles/quantize_widths_parent_wrappers_pytest_gpu.txt is the run of
the three wrapper tests with the parent's repconc_amd/ops.py over this commit's library: 5 of 7 cases fail, as quoted above.
The parent's kernels are this commit's (the only change to the library is the width check of E), so the bit comparisons of B,
C and D were not run a second time on the parent.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle, pq_oracle

gpu = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
K = 256
WORK_CAP = 3e8                                            # element operations of the numpy oracle in one case
DSUB_MAX = 8191                                           # RC_DSUB_RT_MAX
CAP = 8                                                   # excused fp64-tie mismatches per case (tests/test_sinkhorn_strain.py)
TIE = 1e-9                                                # pq_oracle.codes_equal_up_to_fp64_ties' rtol

# dsub -> (M, what it is the smallest width to reach).  nv = dsub // 8 vectors, full = nv // 4 rounds of four, tail = dsub % 8;
# rt = 8192 // dsub rows fit one staging pass through LDS (the table kernel stages 32 rows, the assignment kernel 8).
WIDTHS = {
    5: (5, "scalar twin, full = 1 and 1 left-over scalar"),
    7: (3, "scalar twin, full = 1 and 3 left-over scalars"),
    9: (5, "one vector, full = 0, tail 1"),
    15: (3, "tail 7"),
    20: (3, "two vectors, tail 4"),
    39: (5, "full = 1, tail 7"),
    40: (3, "full = 1, one left-over vector, no tail"),
    56: (5, "three left-over vectors"),
    100: (3, "full = 3, tail 4"),
    257: (3, "rt = 31 < 32: second staging pass of the table kernel, last pass one row"),
    519: (3, "full = 16: the cascade fires with no rounds after it; tail 7"),
    520: (3, "full = 16, one left-over vector"),
    544: (1, "cascade, then one round"),
    1000: (1, "full = 31, one left-over vector"),
    1025: (3, "rt = 7 < 8: second staging pass of the assignment kernel"),
    1031: (3, "two cascades, tail 7"),
    2080: (1, "rt = 3"),
    8191: (3, "the maximum: rt = 1, full = 255, three left-over vectors, tail 7"),
}
REAL_SHAPES = ((8, 39), (24, 13), (8, 128), (1, 1024), (3, 128))        # 312 / 8, 312 / 24, 1024 / 8, 1024 / 1, 384 / 3
SHAPES = tuple((M, dsub) for dsub, (M, _) in WIDTHS.items()) + REAL_SHAPES
# 1; around ASSIGN_RT_ROWS = 8; around the 32 table rows of a block; several blocks, the last one partial
ROW_COUNTS = (1, 7, 8, 9, 31, 32, 33, 300)
STRIP_B = 16384 + 77                                      # dist_rows_per_block: 128 rows per block from B = 16384
STRIP_SHAPES = ((3, 20), (3, 16))


def row_counts(M, dsub):
    return tuple(B for B in ROW_COUNTS if B * M * K * dsub <= WORK_CAP)


def np_table(x, C):
    """pq_oracle.dist_table in chunks of at most 2^24 squares."""
    M, _, dsub = C.shape
    return pq_oracle.dist_table(x, C, chunk=max(1, (1 << 24) // (M * K * dsub)))


def nearest_of(d):
    """pq_oracle.quantize(.., False) from a table: first minimum, a NaN never wins."""
    return np.argmin(np.where(np.isnan(d), F32(np.inf), d), axis=-1).T.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def width_case(M, dsub):
    """x [B, M dsub], C [M, 256, dsub], the numpy oracle's table [M, B, 256] and the C oracle's nearest codes [B, M] at the
    largest row count of (M, dsub); every smaller count is the first rows of these."""
    B = max(row_counts(M, dsub))
    rng = np.random.default_rng(100000 + 10 * dsub + M)
    x = rng.standard_normal((B, M * dsub)).astype(F32)
    C = rng.standard_normal((M, K, dsub)).astype(F32)
    return x, C, np_table(x, C), c_oracle.quantize(x, C, False)[0]


@functools.lru_cache(maxsize=None)
def strip_case(M, dsub):
    rng = np.random.default_rng(7000 + dsub)
    x = rng.standard_normal((STRIP_B, M * dsub)).astype(F32)
    C = rng.standard_normal((M, K, dsub)).astype(F32)
    return x, C, np_table(x, C), c_oracle.quantize(x, C, False)[0]


# ------------------------------------------------------------------------------------------------ A3. wrong sum orders
WRONG = ("running", "no_cascade", "dealt", "tail_last")


def wrong_rowsum(sq, kind):
    """pq_oracle._rowsum_torch_cpu_order with ONE rule replaced (kind None: none, the oracle itself restated):
    running: a plain running sum over j; no_cascade: the rounds accumulate on one level; dealt: left-over vector v goes to
    accumulator v % 4, not to 0; tail_last: the tail scalars are added after the eight lanes, not before."""
    dsub, lead = sq.shape[-1], sq.shape[:-1]
    if kind == "running":
        r = np.zeros(lead, F32)
        for j in range(dsub):
            r = r + sq[..., j]
        return r
    if dsub < 8:
        return pq_oracle._rowsum_torch_cpu_order(sq)
    nv, tail = dsub // 8, dsub % 8
    full = nv // 4
    rounds = [sq[..., 32 * i: 32 * i + 32] for i in range(full)]
    if kind == "no_cascade":
        acc = np.zeros(lead + (32,), F32)
        for r in rounds:
            acc = acc + r
    else:
        acc = pq_oracle._multi_row_sum(rounds)
        acc = np.zeros(lead + (32,), F32) if acc is None else acc
    a = [acc[..., 8 * j: 8 * j + 8] for j in range(4)]
    for v in range(4 * full, nv):
        j = v % 4 if kind == "dealt" else 0
        a[j] = a[j] + sq[..., 8 * v: 8 * v + 8]
    t = a[0] + a[1]
    t = t + a[2]
    t = t + a[3]
    r = np.zeros(lead, F32)
    if kind != "tail_last":
        for j in range(tail):
            r = r + sq[..., nv * 8 + j]
    for lane in range(8):
        r = r + t[..., lane]
    if kind == "tail_last":
        for j in range(tail):
            r = r + sq[..., nv * 8 + j]
    return r


def catches(kind, dsub):
    """Whether the wrong order `kind` is a different sum at this width at all.
    running: always (from dsub 5 the oracle adds out of order).  no_cascade: the cascade's level moves are additions of +0
    until a second round follows one (full = 16: a0 = 0 + a1; full = 17: r16 + S against S + r16), so full >= 18.
    dealt: a full round and at least two left-over vectors (one goes to accumulator 0 either way; with full = 0 the
    accumulators are merged in the order the vectors would have been added).  tail_last: a tail, at a vector width."""
    nv, tail = dsub // 8, dsub % 8
    full = nv // 4
    return {"running": dsub >= 5, "no_cascade": full >= 18, "dealt": full >= 1 and nv - 4 * full >= 2,
            "tail_last": dsub >= 8 and tail >= 1}[kind]


MUST_CATCH = {"running": (5, 7, 9, 20, 40, 8191), "no_cascade": (1000, 1025, 1031, 2080, 8191), "dealt": (56, 8191),
              "tail_last": (9, 15, 20, 39, 100, 257, 519, 1025, 1031, 8191)}


# ------------------------------------------------------------------------------------------------ C. the constrained path
SK_SHAPES = ((5, 7), (4, 9), (24, 13), (16, 20), (8, 39), (6, 40), (7, 72), (3, 100), (2, 520), (1, 1000))
SK_ROWS = (600, 777)
SK_SETTINGS = ((0.003, 100), (0.05, 30))
SK_CASES = [(M, dsub, B, eps, T) for M, dsub in SK_SHAPES for B in SK_ROWS for eps, T in SK_SETTINGS]


def _sk_id(case):
    return "m%d-dsub%d-b%d-eps%g-t%d" % case


@functools.lru_cache(maxsize=None)
def sk_inputs(M, dsub, B):
    """Gaussian rows; the centroids are 256 rows of the batch."""
    rng = np.random.default_rng(31000 + 100 * dsub + M + B)
    x = rng.standard_normal((B, M * dsub)).astype(F32)
    pick = rng.permutation(B)[:K]
    return x, np.ascontiguousarray(x[pick].reshape(K, M, dsub).transpose(1, 0, 2))


@functools.lru_cache(maxsize=None)
def sk_c_codes(M, dsub, B, eps, T):
    x, C = sk_inputs(M, dsub, B)
    return c_oracle.quantize(x, C, True, eps, T)


def sk_pq(M, dsub, B, eps, T):
    """(codes uint8, flags, plan Q [M, B, K] fp64) of the numpy restatement."""
    x, C = sk_inputs(M, dsub, B)
    codes, inter = pq_oracle.quantize(x, C, True, eps, T, return_intermediates=True)
    return codes.astype(np.uint8), inter["flags"], inter["Q"]


# ------------------------------------------------------------------------------------------------ D. ties, non-finite
RT_TIE_WIDTHS = (20, 39)
TIE_PAIRS = ((3, 4), (10, 74), (63, 64), (0, 255), (191, 192))   # same wave; neighbouring waves (twice); first and last wave
TIE_NUDGES = (0, -1, 1)                                   # the upper copy: a duplicate, one ulp nearer, one ulp farther
TIE_B = 41                                                # five blocks of 8 rows and one row
TIE_OFF = 2.0 ** -10
NONFINITE_POS = (0, 63, 64, 255)


def tie_slots():
    return [(pair, n) for pair in TIE_PAIRS for n in TIE_NUDGES] + [(None, 0)]       # the last one: all 256 equal


@functools.lru_cache(maxsize=None)
def tie_case(dsub):
    """x [41, 16 dsub], C [16, 256, dsub], want [41, 16]: sub-quantiser m holds slot m.  Every row of a sub-quantiser sits at
    the slot's base centroid + 2^-10 in coordinate 0 and +- 2^-10 elsewhere; coordinate 0 of the base lies in [1, 1.5), so one
    ulp there is 2^-23 and moves the square of coordinate 0 by 2^-32, a hundred ulps of a sum near dsub 2^-20."""
    rng = np.random.default_rng(4100 + dsub)
    slots = tie_slots()
    M = len(slots)
    C = rng.standard_normal((M, K, dsub)).astype(F32)
    x = np.empty((TIE_B, M, dsub), F32)
    want = np.empty((TIE_B, M), np.uint8)
    for m, (pair, n) in enumerate(slots):
        base = rng.standard_normal(dsub).astype(F32)
        base[0] = F32(1.0 + 0.5 * rng.random())
        if pair is None:
            C[m, :] = base
            want[:, m] = 0
        else:
            lo, up = pair
            C[m, lo] = C[m, up] = base
            if n:                                         # the rows lie above the base in coordinate 0: nearer is upwards
                C[m, up, 0] = np.nextafter(base[0], F32(np.inf if n < 0 else -np.inf))
            want[:, m] = up if n < 0 else lo
        off = np.where(rng.random((TIE_B, dsub)) < 0.5, -TIE_OFF, TIE_OFF).astype(F32)
        off[:, 0] = TIE_OFF
        x[:, m] = base[None] + off
    return x.reshape(TIE_B, M * dsub), C, want, slots


@functools.lru_cache(maxsize=None)
def nonfinite_case(dsub):
    """x [42, 12 dsub], C [12, 256, dsub], bad [(m, position)]: Gaussian codebooks, rows next to centroids; sub-quantiser i
    holds NaN / +inf / -inf in coordinate (3 i) mod dsub of the centroid at one of NONFINITE_POS.  The last row holds a NaN in
    every sub-vector; the others are finite."""
    rng = np.random.default_rng(4200 + dsub)
    combos = [(p, v) for v in (np.nan, np.inf, -np.inf) for p in NONFINITE_POS]
    M, B = len(combos), TIE_B + 1
    C = rng.standard_normal((M, K, dsub)).astype(F32)
    pick = rng.integers(0, K, (B, M))
    x = C[np.arange(M)[None, :], pick] + F32(0.05) * rng.standard_normal((B, M, dsub)).astype(F32)
    for i, (p, v) in enumerate(combos):
        C[i, p, (3 * i) % dsub] = v
        x[B - 1, i, (5 * i) % dsub] = np.nan
    return x.reshape(B, M * dsub).astype(F32), C, [(i, p) for i, (p, _) in enumerate(combos)]


def same_bits_nan_as_nan(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ================================================================================================ CPU tests
def test_the_widths_reach_what_they_claim():
    """The structural figures behind WIDTHS' reasons, from the kernels' own rules."""
    def fig(dsub):
        nv = dsub // 8
        return nv, nv // 4, nv - 4 * (nv // 4), dsub % 8, 8192 // dsub    # vectors, full, left-over vectors, tail, rt
    assert fig(9) == (1, 0, 1, 1, 910) and fig(15)[3] == 7 and fig(20)[:4] == (2, 0, 2, 4)
    assert fig(39)[:4] == (4, 1, 0, 7) and fig(40)[:4] == (5, 1, 1, 0) and fig(56)[:4] == (7, 1, 3, 0)
    assert fig(100)[:4] == (12, 3, 0, 4) and fig(256)[4] == 32 and fig(257)[4] == 31 and 33 - 31 == 2 and 32 - 31 == 1
    assert fig(519)[:4] == (64, 16, 0, 7) and fig(520)[:4] == (65, 16, 1, 0) and fig(544)[:4] == (68, 17, 0, 0)
    assert fig(1000)[:4] == (125, 31, 1, 0) and fig(1024)[4] == 8 and fig(1025)[4] == 7
    assert fig(1031)[:4] == (128, 32, 0, 7) and fig(2080)[4] == 3 and fig(8191) == (1023, 255, 3, 7, 1)
    for M, dsub in SHAPES:
        assert 1 <= dsub <= DSUB_MAX and max(row_counts(M, dsub)) >= 33
        assert dsub not in (8, 12, 16, 24, 32, 48, 64, 96)                # none has a specialised kernel
    assert {M for M, _ in SHAPES[:len(WIDTHS)]} == {1, 3, 5}
    assert max(row_counts(3, 8191)) == 33 and STRIP_B * 3 * K * 20 <= WORK_CAP


@pytest.mark.parametrize("M,dsub", SHAPES)
def test_numpy_sum_order_equals_torch_cpu(M, dsub):
    """modeling_repconc.py:50 evaluated by torch-CPU against the numpy oracle, every bit (as
    test_distance_order_equals_torch_cpu_for_every_divisor_of_768 does for the divisors), on the first rows of the case: as
    many as keep torch's [M, B, 256, dsub] temporary under 2^25 floats."""
    x, C, d, _ = width_case(M, dsub)
    B = max(1, min(33, x.shape[0], (1 << 25) // (M * K * dsub)))
    xt, Ct = torch.from_numpy(x[:B]), torch.from_numpy(C)
    t = ((xt.reshape(B, M, 1, -1).transpose(0, 1) - Ct.unsqueeze(1)) ** 2).sum(-1).numpy()
    assert np.array_equal(d[:, :B].view(np.uint32), t.view(np.uint32))


@pytest.mark.parametrize("M,dsub", SHAPES)
def test_c_oracle_equals_the_numpy_oracle(M, dsub):
    x, C, d, codes = width_case(M, dsub)
    assert np.array_equal(c_oracle.dist_table(x, C).view(np.uint32), d.view(np.uint32))
    assert np.array_equal(codes, nearest_of(d))
    assert len(np.unique(codes)) > 1


def test_c_oracle_refuses_a_width_past_its_buffer():
    x, C = np.zeros((1, DSUB_MAX + 1), F32), np.zeros((1, K, DSUB_MAX + 1), F32)
    with pytest.raises(ValueError):
        c_oracle.dist_table(x, C)
    with pytest.raises(ValueError):
        c_oracle.quantize(x, C, False)
    with pytest.raises(ValueError):
        c_oracle.quantize(x, C, True, 0.05, 3)


@pytest.mark.parametrize("dsub", sorted(WIDTHS))
def test_wrong_sum_orders_change_the_table_of_these_inputs(dsub):
    """Sensitivity on the model: the restated oracle order reproduces the table; each wrong order changes at least one entry
    of the first rows of this very case where it is a different sum at all (catches), and reproduces it where it is not."""
    M = WIDTHS[dsub][0]
    x, C, d, _ = width_case(M, dsub)
    B = min(4, x.shape[0])
    diff = x[:B].reshape(B, M, 1, dsub).transpose(1, 0, 2, 3) - C[:, None]
    sq = diff * diff
    want = d[:, :B].view(np.uint32)
    assert np.array_equal(wrong_rowsum(sq, None).view(np.uint32), want)
    for kind in WRONG:
        changed = int((wrong_rowsum(sq, kind).view(np.uint32) != want).sum())
        print("dsub %d %s: %d of %d entries differ" % (dsub, kind, changed, want.size))
        assert (changed > 0) == catches(kind, dsub), (kind, dsub, changed)
        if dsub in MUST_CATCH[kind]:
            assert changed > 0


def test_every_wrong_order_is_caught_where_it_is_meant_to_be():
    for kind in WRONG:
        assert all(w in WIDTHS and catches(kind, w) for w in MUST_CATCH[kind]), kind
    # what cannot tell a cascade from none: the widths that only strain the loop bounds around it
    assert not catches("no_cascade", 519) and not catches("no_cascade", 520) and not catches("no_cascade", 544)
    assert not catches("dealt", 20) and not catches("dealt", 40) and not catches("dealt", 1000)


@pytest.mark.parametrize("dsub", RT_TIE_WIDTHS)
def test_tie_and_non_finite_families_are_what_they_claim(dsub):
    x, C, want, slots = tie_case(dsub)
    d = np_table(x, C)                                    # [16, 41, 256]
    bits = d.view(np.uint32)
    assert np.isfinite(d).all() and np.array_equal(nearest_of(d), want)
    assert np.array_equal(c_oracle.quantize(x, C, False)[0], want)
    for m, (pair, n) in enumerate(slots):
        if pair is None:                                  # all 256 equal: one bit pattern per row
            assert (bits[m] == bits[m][:, :1]).all()
            continue
        lo, up = pair
        rest = np.delete(d[m], pair, axis=1)
        assert (rest > 1000 * d[m][:, [lo]]).all() and (rest > 1000 * d[m][:, [up]]).all()
        if n == 0:
            assert np.array_equal(bits[m][:, lo], bits[m][:, up])
        else:                                             # n = -1: the upper copy is strictly nearer; +1: strictly farther
            assert (np.sign(d[m][:, up] - d[m][:, lo]) == n).all(), (pair, n)
    assert {s for s in slots} == {(p, n) for p in TIE_PAIRS for n in TIE_NUDGES} | {(None, 0)}

    x, C, bad = nonfinite_case(dsub)
    assert np.isfinite(x[:-1]).all() and np.isnan(x[-1]).sum() == len(bad)
    assert len(bad) == 12 and np.isnan(C).sum() == 4 and np.isinf(C).sum() == 8
    d = np_table(x, C)
    codes = c_oracle.quantize(x, C, False)[0]
    assert np.array_equal(codes, nearest_of(d)) and np.array_equal(codes, pq_oracle.quantize(x, C, False))
    assert same_bits_nan_as_nan(c_oracle.dist_table(x, C), d)
    for m, p in bad:                                      # a non-finite centroid never wins (its distance is NaN or +inf)
        assert not np.isfinite(d[m, :-1, p]).any()
        if p:
            assert (codes[:, m] != p).all()
        else:                                             # position 0 is also the code of a row without a finite distance
            assert (codes[:-1, m] != p).all()
    assert np.isnan(d[:, -1]).all() and (codes[-1] == 0).all()
    assert len(np.unique(codes[:-1])) > 100


@pytest.mark.parametrize("case", SK_CASES, ids=_sk_id)
def test_constrained_restatements_agree_on_every_code(case):
    """The yardstick of part C: no flags, and the C and the numpy restatement of the reference agree on every code, with
    nothing excused (B >= 600: at B < 256 the two differ at their own tie level)."""
    want, cfl = sk_c_codes(*case)
    got, pfl, _ = sk_pq(*case)
    assert cfl == 0 and pfl == 0
    assert np.array_equal(got, want), "%d codes differ" % int((got != want).sum())


# ================================================================================================ GPU tests
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _check_fp32_stage(xt, Ct, d, codes, finite=True):
    """ops.dist_table, its minmax, ops.centre_ and the four forms of ops.assign_nearest on the device tensors xt, Ct against
    the numpy oracle's table d [M, B, 256] and the C oracle's codes [B, M]."""
    from repconc_amd import ops
    got_d, mm = ops.dist_table(xt, Ct)
    gd = got_d.cpu().numpy()
    assert gd.shape == d.shape
    if finite:
        assert np.array_equal(gd.view(np.uint32), d.view(np.uint32))
        mx, mn = pq_oracle.minmax_per_m(d)
        assert np.array_equal(_bits(mm), np.concatenate([mx, mn]).view(np.uint32))
        assert np.array_equal(_bits(ops.centre_(got_d, mm)), pq_oracle.centre(d, mx, mn).view(np.uint32))
    else:
        assert same_bits_nan_as_nan(gd, d)
    for dtype in (torch.uint8, torch.int64):
        for method in ("exact", "auto"):
            got = ops.assign_nearest(xt, Ct, dtype, method=method)
            assert got.dtype == dtype and np.array_equal(got.cpu().numpy(), codes.astype(got.cpu().numpy().dtype)), (dtype, method)
        if Ct.shape[2] not in ops.SUPPORTED_DSUB:         # the wrapper no longer takes the fast entry here: call it
            got, ws = _fast_entry(xt, Ct, dtype)
            assert np.array_equal(got.cpu().numpy(), codes.astype(got.cpu().numpy().dtype)), dtype
            assert bool((ws == 0xFF).all())               # the fall-through writes nothing into the workspace


def _fast_entry(xt, Ct, dtype):
    """rc_pq_assign_nearest_fast itself, on the rows and centroids as the wrapper would hand them over, with a workspace
    filled with 0xFF: (codes, workspace)."""
    import ctypes
    from repconc_amd import _lib, ops
    x, c = ops._rows_f32(xt), ops._centroids(Ct)
    B, D, M, _ = ops._shape(x, c)
    lib, h, s, _ = ops._ctx(x)
    codes = torch.empty((B, M), dtype=dtype, device=x.device)
    n = lib.rc_pq_assign_nearest_fast_ws_bytes(B, M)
    ws = torch.full((n,), 0xFF, dtype=torch.uint8, device=x.device)
    null = ctypes.c_void_p(0)
    u8, i64 = (ops._p(codes), null) if dtype == torch.uint8 else (null, ops._p(codes))
    _lib.check(lib.rc_pq_assign_nearest_fast(h, ops._p(x), x.stride(0), ops._p(c), B, D, M, K, u8, i64, ops._p(ws), n, s),
               "rc_pq_assign_nearest_fast", h)
    return codes, ws


@gpu
@pytest.mark.parametrize("M,dsub", SHAPES)
def test_fp32_stage_bit_for_bit_at_every_row_count(M, dsub):
    x, C, d, codes = width_case(M, dsub)
    xt, Ct = _t(x), _t(C)
    for B in row_counts(M, dsub):
        _check_fp32_stage(xt[:B], Ct, d[:, :B], codes[:B])


@gpu
@pytest.mark.parametrize("M,dsub", STRIP_SHAPES)
def test_fp32_stage_on_the_128_row_strip(M, dsub):
    x, C, d, codes = strip_case(M, dsub)
    _check_fp32_stage(_t(x), _t(C), d, codes)


@gpu
@pytest.mark.parametrize("M,dsub", [(5, 39), (3, 20), (3, 1025), (3, 16)])
def test_padded_row_pitch(M, dsub):
    """ldx = D + 3 (no multiple of 4: the wrapper copies the rows) and the next multiple of 4 above D (taken as it is), NaN
    in the padding."""
    if dsub == 16:
        x, C, d, codes = strip_case(M, dsub)
        x, d, codes = x[:300], d[:, :300], codes[:300]
    else:
        x, C, d, codes = width_case(M, dsub)
    B, D = x.shape
    for pad in (3, 4 - D % 4):
        buf = torch.full((B, D + pad), float("nan"), device=DEV)
        buf[:, :D] = _t(x)
        view = buf[:, :D]
        assert view.stride(0) == D + pad and view.data_ptr() % 16 == 0
        _check_fp32_stage(view, _t(C), d, codes)


@gpu
@pytest.mark.parametrize("M,dsub", [(5, 39), (3, 20), (3, 16)])
def test_view_four_bytes_past_a_boundary(M, dsub):
    """A contiguous view whose storage starts 4 bytes past a 16-byte boundary, rows and centroids alike (defect 3: at the
    specialised width 16 the entries answered RC_EINVAL for such rows)."""
    from repconc_amd import ops
    if dsub == 16:
        x, C, d, codes = strip_case(M, dsub)
        x, d, codes = x[:300], d[:, :300], codes[:300]
    else:
        x, C, d, codes = width_case(M, dsub)
    B, D = x.shape
    buf = torch.zeros(1 + B * D + 3, device=DEV)
    buf[1:1 + B * D] = _t(x).reshape(-1)
    view = buf[1:1 + B * D].view(B, D)
    cbuf = torch.zeros(1 + C.size, device=DEV)
    cbuf[1:] = _t(C).reshape(-1)
    cview = cbuf[1:].view(M, K, dsub)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and cview.is_contiguous() and cview.data_ptr() % 16 == 4
    _check_fp32_stage(view, cview, d, codes)
    eps, T = 0.05, 30
    got, flags = ops.assign_sinkhorn(view, cview, eps, T, torch.uint8)
    want, _ = ops.assign_sinkhorn(_t(x), _t(C), eps, T, torch.uint8)
    assert int(flags.item()) == 0 and torch.equal(got, want)


@gpu
@pytest.mark.parametrize("M,dsub", [(3, 20), (1, 1000)])
def test_statistics_at_a_width_without_a_screen(M, dsub):
    """Defect 2: the fast entry falls through to the exact kernel and writes no doubt count, which the wrapper then read; the
    statistics must say "exact".  A freed tensor of the workspace's size, filled with 0xFF, stands where the allocator would
    most likely put a workspace.  D is a multiple of 4 at both shapes, so the parent's wrapper did take the fast entry."""
    from repconc_amd import _lib, ops
    x, C, _, codes = width_case(M, dsub)
    B = 33
    xt, Ct = _t(x[:B]), _t(C)
    n = _lib.load().rc_pq_assign_nearest_fast_ws_bytes(B, M)
    for method in ("auto", "mfma"):
        junk = torch.full((n,), 0xFF, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        del junk
        st = {}
        got = ops.assign_nearest(xt, Ct, torch.uint8, method=method, stats=st)
        assert np.array_equal(got.cpu().numpy(), codes[:B])
        assert st["method"] == "exact" and st["doubtful"] == 0 and not st.get("overflow", False), st
    st = {}
    ops.assign_nearest(xt, Ct, torch.uint8, method="exact", stats=st)
    assert st["method"] == "exact" and st["doubtful"] == 0


@gpu
@pytest.mark.parametrize("M,dsub", [(5, 39), (3, 16)])
def test_empty_batch(M, dsub):
    """Defect 4: no rows, no launch: d [M, 0, 256] and the neutral range (-inf, +inf) of solve_fill_range_kernel."""
    from repconc_amd import ops
    C = _t(np.random.default_rng(1).standard_normal((M, K, dsub)).astype(F32))
    x = torch.empty((0, M * dsub), device=DEV)
    d, mm = ops.dist_table(x, C)
    assert d.shape == (M, 0, K) and d.dtype == torch.float32 and d.is_cuda
    assert mm.is_cuda and mm.dtype == torch.float32
    assert np.array_equal(mm.cpu().numpy(), np.array([-np.inf] * M + [np.inf] * M, F32))
    d, mm = ops.dist_table(x, C, with_minmax=False)
    assert d.shape == (M, 0, K) and mm is None
    assert ops.assign_nearest(x, C, torch.uint8).shape == (0, M)
    codes, flags = ops.assign_sinkhorn(x, C, 0.05, 3, torch.uint8)
    assert codes.shape == (0, M) and int(flags.item()) == 0


# ------------------------------------------------------------------------------------------------ C
@gpu
@pytest.mark.parametrize("case", SK_CASES, ids=_sk_id)
def test_constrained_codes_at_run_time_widths(case):
    from repconc_amd import ops
    M, dsub, B, eps, T = case
    x, C = sk_inputs(M, dsub, B)
    want, cfl = sk_c_codes(*case)
    codes, flags = ops.assign_sinkhorn(_t(x), _t(C), eps, T, torch.uint8)
    got = codes.cpu().numpy()
    nbad = int((got != want).sum())
    print("[C] %s: %d codes differ from the C restatement" % (_sk_id(case), nbad))
    assert cfl == 0 and int(flags.item()) == 0
    if nbad:                                              # the numpy restatement's plan, only now
        pq, pfl, Q = sk_pq(*case)
        ok, n = pq_oracle.codes_equal_up_to_fp64_ties(got, pq, Q, rtol=TIE)
        assert pfl == 0 and np.array_equal(pq, want)
        assert ok and n <= CAP, (ok, n)
    i64, flags = ops.assign_sinkhorn(_t(x), _t(C), eps, T)
    assert i64.dtype == torch.int64 and int(flags.item()) == 0 and torch.equal(i64, codes.long())


class _TableEncoder(torch.nn.Module):
    def __init__(self, table):
        super().__init__()
        from types import SimpleNamespace
        self.register_buffer("table", table)
        self.config = SimpleNamespace(hidden_size=table.shape[1])

    def forward(self, input_ids, attention_mask):
        return self.table[input_ids[:, 0]]


@gpu
@pytest.mark.parametrize("M", [8, 24])
def test_repconc_at_hidden_size_312(M):
    """What test_every_divisor_of_the_hidden_size_is_a_valid_mcq_m does for 768, at a 312-wide encoder: dsub 39 and 13."""
    from types import SimpleNamespace
    from repconc_amd.models.repconc import RepCONC
    eps, T, B, dsub = 0.003, 100, 600, 312 // M
    x, C = sk_inputs(M, dsub, B)
    cfg = SimpleNamespace(MCQ_M=M, MCQ_K=256, hidden_size=312, similarity_metric="METRIC_IP")
    model = RepCONC(cfg, _TableEncoder(torch.zeros(1, 312)), False, eps, T).to(DEV)
    with torch.no_grad():
        model.centroids.copy_(_t(C))
    near = model.quantize(_t(x)).cpu().numpy()
    assert near.shape == (B, M) and near.dtype == np.int64
    assert np.array_equal(near.astype(np.uint8), c_oracle.quantize(x, C, False)[0])
    model.use_constraint = True
    got = model.quantize(_t(x)).cpu().numpy().astype(np.uint8)
    want = sk_c_codes(M, dsub, B, eps, T)[0]
    if not np.array_equal(got, want):
        pq, _, Q = sk_pq(M, dsub, B, eps, T)
        ok, n = pq_oracle.codes_equal_up_to_fp64_ties(got, pq, Q, rtol=TIE)
        assert np.array_equal(pq, want) and ok and n <= CAP
    dec = model.decode(_t(near)).detach().cpu().numpy()
    assert np.array_equal(dec.view(np.uint32), pq_oracle.decode(near, C).view(np.uint32))
    assert np.array_equal(dec, c_oracle.decode(near.astype(np.uint8), C))


# ------------------------------------------------------------------------------------------------ D
@gpu
@pytest.mark.parametrize("dsub", RT_TIE_WIDTHS)
def test_ties_through_the_run_time_width_reduction(dsub):
    x, C, want, _ = tie_case(dsub)
    codes = c_oracle.quantize(x, C, False)[0]
    assert np.array_equal(codes, want)
    xt, Ct = _t(x), _t(C)
    for B in (TIE_B, 8, 1):
        _check_fp32_stage(xt[:B], Ct, np_table(x[:B], C), want[:B])


@gpu
@pytest.mark.parametrize("dsub", RT_TIE_WIDTHS)
def test_non_finite_values_through_the_run_time_width_reduction(dsub):
    from repconc_amd import ops
    x, C, bad = nonfinite_case(dsub)
    codes = c_oracle.quantize(x, C, False)[0]
    _check_fp32_stage(_t(x), _t(C), np_table(x, C), codes, finite=False)
    got = ops.assign_nearest(_t(x), _t(C), torch.uint8, method="exact").cpu().numpy()
    for m, p in bad:
        assert (got[:-1, m] != p).all()
    assert (got[-1] == 0).all()


# ------------------------------------------------------------------------------------------------ E
@gpu
def test_a_width_past_the_maximum_is_refused_before_any_launch():
    from repconc_amd import _lib, ops
    refused = (_lib.RepconcHipError, ValueError)
    dsub = DSUB_MAX + 1
    x = torch.zeros((2, dsub), device=DEV)
    C = torch.zeros((1, K, dsub), device=DEV)
    with pytest.raises(refused):
        ops.dist_table(x, C)
    for method in ("exact", "auto"):
        for dtype in (torch.uint8, torch.int64):
            with pytest.raises(refused):
                ops.assign_nearest(x, C, dtype, method=method)
    for B in (2, 1):
        for dtype in (torch.uint8, torch.int64):
            with pytest.raises(refused):
                ops.assign_sinkhorn(x[:B], C, 0.05, 3, dtype)
    torch.cuda.synchronize()
    xs, Cs, d, codes = width_case(5, 39)                  # an ordinary call still works
    _check_fp32_stage(_t(xs[:9]), _t(Cs), d[:, :9], codes[:9])
