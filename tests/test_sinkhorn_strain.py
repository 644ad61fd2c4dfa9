"""The constrained assignment (ops.assign_sinkhorn -> rc_pq_assign_sinkhorn; sweeps and argmax in csrc/sinkhorn.hip, the solve
driver in csrc/comm.hip) on inputs built to strain it.  Every other Sinkhorn test feeds clustered or i.i.d. Gaussian rows at
eps in {0.003, 0.01, 0.05}; here the batch is small (three ragged shapes on three specialised widths) and the DATA is chosen.

Families (FAMILIES; (M, B) -> (x, C)):
  control        clustered rows, centroids = rows of the batch              gauss          i.i.d. N(0, 1) rows and centroids
  dup_rows       the second half of the batch repeats the first: plan entries whose two best values differ by 1e-9 .. 1e-6 are
                 routine (the sweep's exp is good to ~1e-13)
  dup_centroids  centroids 128..255 are a permutation of 0..127: EXACT ties whose partners sit in another lane or another group of
                 four of the permuted k layout (sk_kidx); the first maximum is always < 128
  outlier_row    one row x 100: every other centred distance sits in a sliver of [-1, 1]
  dead_centroids 64 centroids x 50: never nearest to anything, their row potentials run away
  offset         x + 1000, C + 1000 (cancellation in the fp32 table)      tiny           x, C x 1e-20: the squares are fp32
                 subnormals, the centred table is ~1e-33, every plan entry ties and every code is 0
  one_cluster    every row within 1e-3 of one point                          nan_row / inf_row   one non-finite element

Parts.  A: for eps >= 0.003 the uint8 codes equal the C restatement of the reference (oracle.c_oracle) — exactly, or where a
code differs the REFERENCE's own plan (oracle.pq_oracle, fp64) holds a tie at its rounding level (codes_equal_up_to_fp64_ties,
rtol 1e-9), at most CAP = 8 such codes per case (0.1 % of the smallest case; the two restatements and the fp64 potentials form
agree on every code of every case here, test E).  B: the fp32 stage bit for bit.  C: the kernel variants and the two-shard
choreography under criterion A.  D: below the reference's underflow edge and on non-finite input.  E (no GPU): the inputs and
the oracles themselves.

The underflow edge: the reference's plan starts as exp(out / eps) / tot with centred distances reaching +-1, so its smallest
entries become subnormal or zero once 2 / eps + ln(B K) > ~708, eps < ~0.00288 — below that its codes depend on its own
underflow of single entries, which the potentials form the HIP path uses does not share.  There (D) the HIP path is held to the fp64 potentials
restatement, oracle.pq_oracle.sinkhorn_codes_logdomain: a code differs from it only where the restatement's score is within
1e-9 (the project's tie figure, in log units: d log Q = dQ / Q) of its maximum.

What the parent of this file's commit did with them [MI355X]: every assertion of A, B and C held with no excused tie — except
dup_rows at (0.003, 3) on the two ragged shapes, where 30 / 12 codes differ, all ties of the reference's plan, more than CAP: cases
the reference itself cannot decide (UNDECIDED below, with the figures), held to D's rule instead of the cap.  No kernel changed.  D: flags 0 and the restatement's codes everywhere except outlier_row (flags 3: its whole column underflows in the
potentials form too, see test_below_the_edge_where_the_reference_itself_warns).  Sensitivity, measured once on builds made wrong on
purpose: a tie rule that keeps the HIGHER k in the argmax's rotate steps fails 24 cases (all of dup_centroids and tiny); a 1e-4
relative error in the slope of the exp polynomial (1.7e-8 per entry) changes no code of any case — the file pins the tie rule,
the range logic, the reduction order and the fp32 stage, not the last digits of exp.
"""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from oracle import c_oracle, pq_oracle, synth

gpu = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64

SHAPES = [(8, 1024), (48, 600), (12, 777)]              # dsub 96 / 16 / 64; ragged against 16-column groups and the block split
A_SETTINGS = [(0.003, 100), (0.003, 3), (0.01, 30), (0.3, 100), (1.0, 10)]      # (eps, T); (0.003, 3): structural ties
D_SETTINGS = [(0.002, 30), (0.0015, 100)]
CAP = 8                                                 # excused fp64-tie mismatches per case
TIE = 1e-9                                              # pq_oracle.codes_equal_up_to_fp64_ties' rtol; score deficit in D
RC_FLAG_NONFINITE, RC_FLAG_RANGE = 1, 2                 # include/repconc_hip.h


# ------------------------------------------------------------------------------------------------------------ families
def _control(M, B):
    x = synth.clustered_embeddings(9001, B)
    return x, synth.sample_centroids(9101, x, M)


def _gauss(M, B):
    return synth.gaussian(3, (B, 768)), synth.gaussian(4, (M, 256, 768 // M))


def _dup_rows(M, B):
    x, C = _control(M, B)
    x[B // 2:] = x[:B - B // 2]
    return x, C


def _dup_centroids(M, B):
    x, C = _control(M, B)
    C[:, 128:] = C[:, np.random.default_rng(5).permutation(128)]
    return x, C


def _outlier_row(M, B):
    x, C = _control(M, B)
    x[7] *= F32(100)
    return x, C


def _dead_centroids(M, B):
    x, C = _control(M, B)
    C[:, 192:] *= F32(50)
    return x, C


def _offset(M, B):
    x, C = _control(M, B)
    return x + F32(1000), C + F32(1000)


def _tiny(M, B):
    x, C = _control(M, B)
    return x * F32(1e-20), C * F32(1e-20)


def _one_cluster(M, B):
    x, C = _control(M, B)                               # the centroids stay rows of the original batch
    return (x[:1] + F32(1e-3) * synth.gaussian(5, (B, 768))).astype(F32), C


def _with(value):
    def f(M, B):
        x, C = _control(M, B)
        x[5, 40] = value
        return x, C
    return f


FAMILIES = {"control": _control, "gauss": _gauss, "dup_rows": _dup_rows, "dup_centroids": _dup_centroids,
            "outlier_row": _outlier_row, "dead_centroids": _dead_centroids, "offset": _offset, "tiny": _tiny,
            "one_cluster": _one_cluster, "nan_row": _with(np.nan), "inf_row": _with(np.inf)}
FINITE = [f for f in FAMILIES if f not in ("nan_row", "inf_row")]

# (family, M, B, eps, T), a family's cases of one shape next to each other (the caches below hold two tables)
A_CASES = [(f, M, B, eps, T) for f in FINITE for (M, B) in SHAPES
           for (eps, T) in (A_SETTINGS if (M, B) == SHAPES[0] else A_SETTINGS[:3])]   # the last two: (8, 1024) only
E_CASES = [(f, M, B, eps, T) for f in FINITE for (M, B) in SHAPES
           for (eps, T) in (A_SETTINGS if (M, B) == SHAPES[0] else A_SETTINGS[:1])]


# Cases of A that the reference itself cannot decide; they keep every assertion of A except the cap, which part D's rule
# replaces (flags 0; a code differs from the fp64 potentials restatement only within 1e-9 of its best score).  Both are
# dup_rows after THREE iterations at a ragged shape: 300 / 389 distinct rows against 256 centroids.  Measured on the CPU, the
# reference's own fp64 plan holds 28 / 18 columns whose two largest entries are EXACTLY equal and 70 / 26 within 1e-13 (at
# (8, 1024): 0 and 2), so its first maximum there is decided by the last bit of its in-place arithmetic: the fp64 potentials
# restatement already differs from it in 12 / 8 codes (plan ratios within 1.8e-14 of 1), and the HIP path [MI355X] in 30 / 12,
# every one a tie of the reference's plan at rtol 1e-9.  With the cap of 8 these two cases fail; nothing else in A does.
UNDECIDED = {("dup_rows", 48, 600, 0.003, 3), ("dup_rows", 12, 777, 0.003, 3)}


def _id(case):
    return "%s-m%d-b%d-eps%g-T%d" % case if len(case) == 5 else "%s-m%d-b%d" % case


# ------------------------------------------------------------------------------------------------------------- oracles
@functools.lru_cache(maxsize=4)
def _inputs(family, M, B):
    x, C = FAMILIES[family](M, B)
    x, C = np.ascontiguousarray(x, F32), np.ascontiguousarray(C, F32)
    x.setflags(write=False)
    C.setflags(write=False)
    return x, C


@functools.lru_cache(maxsize=None)
def _c_codes(family, M, B, eps, T):
    """(codes uint8 [B, M], flags) of the C restatement of the reference."""
    x, C = _inputs(family, M, B)
    codes, flags = c_oracle.quantize(x, C, True, eps, T)
    codes.setflags(write=False)
    return codes, flags


def _per_m(fn, M):
    """[fn(m) for m in range(M)] on a few threads.  Every reduction of quantize is per sub-quantiser, so the numpy restatement
    run on one sub-quantiser at a time does the same arithmetic in the same order (E checks that against the one-piece call)."""
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as ex:
        return list(ex.map(fn, range(M)))


@functools.lru_cache(maxsize=2)
def _pq_centred(family, M, B):
    """Centred table [M, B, K] fp32 of the numpy restatement (pq_oracle.dist_table / minmax_per_m / centre)."""
    x, C = _inputs(family, M, B)
    dsub = 768 // M
    d = np.concatenate(_per_m(lambda m: pq_oracle.dist_table(x[:, m * dsub:(m + 1) * dsub], C[m:m + 1]), M), 0)
    mx, mn = pq_oracle.minmax_per_m(d)
    dc = pq_oracle.centre(d, mx, mn)
    dc.setflags(write=False)
    return dc


def _pq_plan(family, M, B, eps, T):
    """(codes int64 [B, M], Q [M, B, K] fp64, flags) of the numpy restatement: what pq_oracle.quantize(x, C, True, eps, T,
    return_intermediates=True) returns, from the cached table."""
    dc = _pq_centred(family, M, B)
    Q = np.concatenate(_per_m(lambda m: pq_oracle.sinkhorn_q([-(dc[m:m + 1].astype(F64)).transpose(0, 2, 1)], eps, T)[0]
                              .transpose(0, 2, 1), M), 0)
    with np.errstate(invalid="ignore"):
        codes = np.argmax(Q, axis=-1).T.copy()
    return codes, Q, int(np.isnan(Q).any()) | (int(np.isinf(Q).any()) << 1)


@functools.lru_cache(maxsize=None)
def _pq_codes(family, M, B, eps, T):
    codes, _, flags = _pq_plan(family, M, B, eps, T)
    return codes, flags


def _restatement(family, M, B, eps, T):
    """(codes int64 [B, M], scores L + f [M, B, K]) of the fp64 potentials form."""
    dc = _pq_centred(family, M, B)
    with np.errstate(all="ignore"):
        parts = _per_m(lambda m: pq_oracle.sinkhorn_codes_logdomain(dc[m:m + 1], eps, T, return_scores=True), M)
    return np.concatenate([p[0] for p in parts], 1), np.concatenate([p[1] for p in parts], 0)


def _score_deficit(got, S):
    """Per code, how far the restatement's score of `got` [B, M] lies below the restatement's best score of that column."""
    g = np.take_along_axis(S, np.asarray(got).astype(np.int64).T[:, :, None], axis=2)[:, :, 0]
    return (S.max(axis=2) - g).T


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # a copy: the cached inputs are read-only


def _criterion_a(got, flags, case, what=""):
    """Criterion A on uint8 codes `got` [B, M] and the flags word of one HIP solve of `case`."""
    family = case[0]
    want, cfl = _c_codes(*case)
    got = np.asarray(got)
    n = int((got != want).sum())
    print("[A] %s%s: flags %d, %d of %d codes differ from the C restatement" % (_id(case), what, flags, n, got.size))
    assert cfl == 0 and flags == 0
    assert got.dtype == np.uint8 and got.shape == want.shape
    if n:                                               # the numpy restatement's plan, only now
        _, Q, _ = _pq_plan(*case)
        ok, nbad = pq_oracle.codes_equal_up_to_fp64_ties(got, want, Q, rtol=TIE)
        print("[A] %s%s: %d mismatches, all fp64-level ties of the reference's plan: %s" % (_id(case), what, nbad, ok))
        assert ok
        if case in UNDECIDED:                           # part D's rule in place of the cap
            assert _compare_with_the_restatement(got.astype(np.int64), case)
        else:
            assert nbad <= CAP
    B = got.shape[0]
    if family == "dup_rows":
        assert np.array_equal(got[:B // 2], got[B // 2:2 * (B // 2)])     # odd B: the last row repeats nothing
    if family == "dup_centroids":
        assert int(got.max()) < 128
    if family == "tiny":
        assert not got.any()


# ------------------------------------------------------------------------------------------- A: parity inside the band
@gpu
@pytest.mark.parametrize("case", A_CASES, ids=_id)
def test_codes_equal_the_reference_for_eps_from_0_003(case):
    from repconc_amd import ops
    family, M, B, eps, T = case
    x, C = _inputs(family, M, B)
    codes, flags = ops.assign_sinkhorn(_t(x), _t(C), eps, T, torch.uint8)
    _criterion_a(codes.cpu().numpy(), int(flags.item()), case)


# ------------------------------------------------------------------------------------------------- B: the fp32 stage
@gpu
@pytest.mark.parametrize("case", [(f, M, B) for f in FINITE for (M, B) in SHAPES[:2]], ids=_id)
def test_fp32_stage_bitwise(case):
    """Distance table, per-m max / min and the centred table as uint32 against the C restatement, which is compiled without
    contraction and without flush-to-zero: a flushed subnormal (`tiny`) is a finding about the kernel."""
    from repconc_amd import ops
    family, M, B = case
    x, C = _inputs(family, M, B)
    ref = c_oracle.dist_table(x, C)
    rmm = c_oracle.minmax(ref)
    d, mm = ops.dist_table(_t(x), _t(C))
    assert np.array_equal(d.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(mm.cpu().numpy().view(np.uint32), rmm.view(np.uint32))
    ops.centre_(d, mm)
    c_oracle.centre_(ref, rmm)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), ref.view(np.uint32))
    if family == "tiny":                                # the family does what it is there for
        assert 0 < float((x * x).max()) < float(np.finfo(F32).tiny)


# -------------------------------------------------------------------- C: kernel variants, the sharded choreography
VARIANTS = {"default": {}, "fklds0": {"RC_SK_FKLDS": "0"}, "nb7": {"RC_SK_NB": "7"},
            "v1-cpb64": {"RC_SK_V1": "1", "RC_SK_CPB": "64"}, "unfused-centre": {"RC_FUSE_CENTRE": "0"},
            "no-graph": {"RC_GRAPH": "0"}}
SWITCHES = ("RC_SK_V1", "RC_SK_FKLDS", "RC_SK_NB", "RC_SK_CPB", "RC_FUSE_CENTRE", "RC_GRAPH", "RC_SK_PRIO")
C_FAMILIES = ["dup_rows", "dup_centroids", "dead_centroids", "outlier_row"]


@gpu
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("family", C_FAMILIES)
def test_every_sweep_variant_meets_the_same_criterion(family, variant, monkeypatch):
    """The switches are read on every call (csrc/rc_common.h rc_env_int)."""
    from repconc_amd import ops
    for key in SWITCHES:
        monkeypatch.delenv(key, raising=False)
    for key, val in VARIANTS[variant].items():
        monkeypatch.setenv(key, val)
    case = (family,) + SHAPES[0] + A_SETTINGS[0]
    x, C = _inputs(*case[:3])
    codes, flags = ops.assign_sinkhorn(_t(x), _t(C), case[3], case[4], torch.uint8)
    _criterion_a(codes.cpu().numpy(), int(flags.item()), case, " [%s]" % variant)


@gpu
@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("family", ["dup_rows", "dead_centroids"])
def test_two_virtual_shards_meet_the_same_criterion(family, split):
    """Rank-ordered sum of the gathered row sums on two virtual ranks; in dup_rows each row's duplicate is on the other rank."""
    from repconc_amd.sharded import assign_sinkhorn_virtual
    case = (family,) + SHAPES[0] + A_SETTINGS[0]
    x, C = _inputs(*case[:3])
    half = x.shape[0] // 2
    codes, flags = assign_sinkhorn_virtual([_t(x[:half]), _t(x[half:])], _t(C), case[3], case[4], dtype=torch.uint8,
                                           split=split)
    fl = 0
    for f in flags:
        fl |= int(f.item())
    _criterion_a(torch.cat(codes, 0).cpu().numpy(), fl, case, " [2 shards, split=%s]" % split)


# ------------------------------------------------------------------------- D: below the band, non-finite input
def _solve_i64(x, C, eps, T):
    from repconc_amd import ops
    codes, flags = ops.assign_sinkhorn(_t(x), _t(C), eps, T, torch.int64)
    return codes.cpu().numpy(), int(flags.item())


def _compare_with_the_restatement(got, case):
    rc, S = _restatement(*case)
    if not np.isfinite(S).all():
        print("[D] %s: the fp64 potentials restatement is not finite, nothing to compare" % _id(case))
        return False
    deficit = _score_deficit(got, S)
    n = int((got != rc).sum())
    print("[D] %s: %d codes differ from the potentials restatement, largest score deficit %.3e" % (_id(case), n, deficit.max()))
    assert float(deficit.max()) <= TIE
    return True


@gpu
@pytest.mark.parametrize("setting", D_SETTINGS, ids=lambda s: "eps%g-T%d" % s)
@pytest.mark.parametrize("family", ["control", "gauss", "offset", "dup_rows"])
def test_below_the_references_underflow_edge_the_codes_are_the_potentials_forms(family, setting):
    """eps 0.002 and 0.0015 at (8, 1024): 2 / eps + ln(B K) = 1012 / 1346 > 708, so entries of the reference's plan are
    subnormal or zero from the start and its argmax depends on which (measured on the CPU for dup_rows at 0.0015: the
    reference and the fp64 potentials form disagree on 8 codes, 4 of them with a plan ratio of 0 or 0.81).  The HIP path's
    specification here is the potentials form, which loses no single entry (a whole column can still underflow, next test): flags 0, and every code the restatement's or within 1e-9 of its
    best score.  The number of codes that differ from the reference's restatement is printed, not asserted."""
    M, B = SHAPES[0]
    case = (family, M, B) + setting
    x, C = _inputs(family, M, B)
    got, flags = _solve_i64(x, C, *setting)
    ref, rfl = _c_codes(*case)
    print("[D] %s: flags %d (C restatement of the reference: %d), %d of %d codes differ from the reference's"
          % (_id(case), flags, rfl, int((got != ref).sum()), got.size))
    assert flags == 0
    assert got.min() >= 0 and got.max() < 256
    assert _compare_with_the_restatement(got, case)


@gpu
@pytest.mark.parametrize("setting", D_SETTINGS, ids=lambda s: "eps%g-T%d" % s)
@pytest.mark.parametrize("family", ["outlier_row", "dead_centroids", "one_cluster"])
def test_below_the_edge_where_the_reference_itself_warns(family, setting):
    """On these three the reference's plan holds NaN at both settings (its "Sinkhorn Algorithm returns nan/inf values" case;
    the C restatement returns flag 1): it cannot decide the codes.  Promised: the call returns, the int64 codes are in range and
    repeat from call to call with the flags; and if the HIP flags are 0 and the potentials restatement is finite, the codes are
    that restatement's up to ties.

    [MI355X] dead_centroids and one_cluster: flags 0 at both settings and every code the restatement's.  outlier_row: flags 3
    at both.  The outlier's column has max_k (L + f) = -2 / eps + 6 after sweep 0 (-988 / -1315), below the -745 where exp()
    is 0 in fp64: the column sum of sweep 1 is 0 in the potentials form as well (the restatement is not finite from
    eps < ~0.00265 down; at 0.003 the column sits at -661 and test A passes with flags 0).  RC_FLAG_RANGE is then raised by the
    NaN row potentials of the next sweep (the bound is tested as !(need < 2^26), csrc/sinkhorn.hip), not by the bound proper:
    with |L| <= 1 / eps and f within ~2 / eps of -1 / eps, need <= ~3 / eps x 4096 / ln 2 = 1.2e7 < 2^26 for eps >= 0.0015.
    Hence the assertion that the range flag never comes alone here."""
    M, B = SHAPES[0]
    case = (family, M, B) + setting
    x, C = _inputs(family, M, B)
    got, flags = _solve_i64(x, C, *setting)
    again, flags2 = _solve_i64(x, C, *setting)
    _, rfl = _c_codes(*case)
    print("[D] %s: flags %d (C restatement of the reference: %d)" % (_id(case), flags, rfl))
    assert got.dtype == np.int64 and got.shape == (B, M)
    assert got.min() >= 0 and got.max() < 256
    assert np.array_equal(got, again) and flags == flags2
    assert not (flags & RC_FLAG_RANGE) or (flags & RC_FLAG_NONFINITE)
    if flags == 0:
        _compare_with_the_restatement(got, case)


@gpu
@pytest.mark.parametrize("family", ["nan_row", "inf_row"])
def test_a_non_finite_element_is_reported_and_the_codes_stay_in_range(family):
    """One NaN / inf in the batch: the reference's whole plan of that sub-quantiser is NaN and it warns.  The sweep's table
    index is masked and the argmax starts from lane index 0, so nothing is read or written out of bounds."""
    M, B = SHAPES[0]
    x, C = _inputs(family, M, B)
    got, flags = _solve_i64(x, C, *A_SETTINGS[0])
    print("[D] %s: flags %d" % (family, flags))
    assert flags & RC_FLAG_NONFINITE
    assert got.dtype == np.int64 and got.shape == (B, M)
    assert got.min() >= 0 and got.max() < 256


# -------------------------------------------------------------------------------------- E: the inputs, without a GPU
@pytest.mark.parametrize("case", E_CASES, ids=_id)
def test_inputs_and_oracles_agree_without_a_gpu(case):
    """The reference alone stays far inside criterion A: no flags, its C and numpy restatements agree on every code, and the
    fp64 potentials form differs in at most CAP codes, each an fp64-level tie of the reference's plan.

    At the two ragged shapes only (0.003, 100) is checked here.  Measured once at (0.003, 3) on all nine families there: the two
    restatements of the reference agree on every code and raise no flag, and the potentials form stays within CAP, ties only,
    except dup_rows at (48, 600): 12 of 28 800 codes (8 of 9 324 at (12, 777)), every one a tie of the reference's plan at rtol
    1e-9 (300 distinct rows against 256 centroids after three iterations: the structural ties codes_equal_up_to_fp64_ties
    describes).  Those two are the UNDECIDED cases of test A."""
    family, M, B, eps, T = case
    want, cfl = _c_codes(*case)
    pq, pfl = _pq_codes(*case)
    assert cfl == 0 and pfl == 0
    assert np.array_equal(want, pq)
    rc, S = _restatement(*case)
    if family == "dup_rows" and (eps, T) == A_SETTINGS[0]:
        # the family does what it is there for: columns whose two best scores nearly tie (gap = log of the plan ratio)
        top = np.sort(S, axis=2)[:, :, -2:]
        gap = top[:, :, 1] - top[:, :, 0]
        print("[E] %s: %d columns with a score gap < 1e-6, %d < 1e-4, smallest %.2e"
              % (_id(case), int((gap < 1e-6).sum()), int((gap < 1e-4).sum()), gap.min()))
        assert int((gap < 1e-6).sum()) >= 1
    if (rc != want).any():
        _, Q, _ = _pq_plan(*case)
        ok, nbad = pq_oracle.codes_equal_up_to_fp64_ties(rc, want, Q, rtol=TIE)
        assert ok and nbad <= CAP
    if family == "dup_rows":
        assert np.array_equal(want[:B // 2], want[B // 2:2 * (B // 2)])
    if family == "dup_centroids":
        assert int(want.max()) == 127
    if family == "tiny":
        assert not want.any()


def test_the_per_sub_quantiser_oracle_calls_equal_the_one_piece_call():
    case = ("dup_rows",) + SHAPES[2] + A_SETTINGS[2]
    x, C = _inputs(*case[:3])
    codes, im = pq_oracle.quantize(x, C, True, case[3], case[4], return_intermediates=True)
    mine, Q, flags = _pq_plan(*case)
    assert np.array_equal(im["centred"].view(np.uint32), _pq_centred(*case[:3]).view(np.uint32))
    assert np.array_equal(im["Q"], Q) and np.array_equal(codes, mine) and flags == im["flags"]
    rc, S = _restatement(*case)
    assert np.array_equal(rc, pq_oracle.sinkhorn_codes_logdomain(im["centred"], case[3], case[4]))
    assert _score_deficit(rc, S).max() == 0.0
