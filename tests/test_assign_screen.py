"""The matrix-core assignment screen (rc_pq_assign_nearest_fast, csrc/pq_assign_mfma.hip) where its margin is tight, and
across every structural boundary of its epilogue.

Every GPU comparison is of codes, bit for bit, with ops.assign_nearest(method="exact") on all rows and with the C oracle
(oracle.c_oracle.quantize; on a stated row subset where B is large).  No tolerance appears in a GPU assertion.  The margin
is read from the library (ops.assign_margin), never restated.  Generators are module level, seeded, numpy on the CPU; the
CPU tests check that the inputs are what they claim.

1. THE SPLIT AND THE MODEL (CPU).  bf16_round / split2 restate mf_split2: round to nearest even to 8 significant bits, then the
   same of the fp32 remainder (which is exact).  Over every fp32 in [1, 1 + 2^-6), i.e. every pattern of the 16 low bits,
   max |rest| / |v| = 1.996 * 2^-18 and max |vl| / |v| = 1.992 * 2^-9; over the binade the bounds 2^-17 and 2^-8 hold.
   screen_model is the three kept products  wh.xh + wh.xl + wl.xh  (w = -2 c) in fp64 with nothing else rounded: its error e
   against ||c||^2 - 2 <c, x> is exactly the products the screen drops.

2. THE MARGIN UNDER STRAIN.  Coherent family (dsub 8 / 16 / 96 at M = 16 / 48 / 8, B = 300): every row coordinate is
   P+ = 0x3f807f40, where vl and rest are both positive and near their maxima.  Centroid A is P+ plus whole steps of 2^-7 (one
   bf16 ulp: the low bits stay), centroid B is P- = 0x3f8080c0 (both pieces negative) plus whole steps.  The nearer of the two
   carries no steps, the farther one carries steps on its first four coordinates whose sum of squares n (four_squares) puts
   the reference gap at g * margin * scale, g in RUNGS, to within one step of n: 2^-14 / scale, at most 0.03 margins (dsub 8);
   the fp32 oracle gap equals the fp64 one to that precision.  At g = 0 the pair is (P+, P-) itself: A is the row, B lies
   9 dsub 2^-32 away, 1e-5 margins.  Which of the two is nearer alternates with the sub-quantiser, the positions walk over
   AB_POSITIONS, and sub-quantisers are multiplied, rows and centroids alike, by 1, 2^-20, 2^10 and 2^40.  The other 254
   centroids are the negated pattern, 2 per coordinate away, of the same norm, so max ||c||^2 does not loosen the scale.
   On the model e_A / scale >= 2.93e-5 and e_B / scale <= -1.43e-5 on every rung (3.01e-5 and -1.49e-5 without steps at
   dsub 96; the bound is 3.05e-5): asserted at 2.9e-5 and -1.4e-5, which qualifies the inputs and does not involve the margin.
   GPU: codes equal the planted ones, the exact kernel and the oracle; every pair at g = 0 is doubtful; none at g >= 3 is (a
   true gap of 3 margins less a screen error of at most 2 E = 1 margin exceeds the margin).  Observed on the MI355X, as the
   model predicts (model lead of the right centroid at g = 0.9 / 1.1: 0.52 / 0.71 margins where A is nearer, 1.28 / 1.47 where
   B is): all doubtful up to g = 0.6, exactly the A-nearer half at 0.9 and 1.1, none from 1.6.
   Common-offset family (B = 600, M = 48, dsub 16): Gaussian rows and centroids plus one vector of 10, 100, 1000 times the
   spread per sub-quantiser; codes exact, the doubtful count does not decrease (observed 5975, 28800, 28800 of 28800).

3. STRUCTURE.  Positions are k = 32 tile + (r & 3) + 8 (r >> 2) + 4 half; the epilogue folds r in pairs (dsub 8, 16, 64), in
   pairs and singles (dsub 32) or in singles (dsub 96).  Every position wins everywhere: B = 845, (M, dsub) = (48, 16) and
   (12, 64), row b next to centroid (37 b + 11 m) mod 256: all 256 positions in every block, 32 different ones in every column
   set, every tile and both half-waves in every column; doubtful below B M / 20.  Ties: TIE_PAIRS / TIE_TRIPLES, copies of one
   base centroid with coordinate 0 moved by 0 or +-1 ulp; per pair: duplicates (the first index wins), the upper one ulp
   farther, the upper one ulp nearer, and both mirrored; per triple: two duplicates and a third one ulp farther / nearer, in
   both position orders; 57 slots dealt to the sub-quantisers of (M, dsub) = (48, 16), (24, 32), (8, 96).  The CPU test checks
   with the numpy oracle that equal nudges are exact ties, different ones strictly ordered, everything else 1000 times
   farther.  Every pair of these calls must be doubtful.  Non-finite centroids: NaN, +inf, -inf in one coordinate of the
   centroid at position 0, 31, 32, 255, finite rows; the rule is that of the exact kernel: a NaN or infinite distance never
   wins, the first minimum does.

4. GEOMETRY.  B in ROW_COUNTS at M = 48 and 96, uint8 and int64.  Ragged chunks: mc_rule restates the host's MC loop from the
   device's CU count; rows_for picks the smallest B with a 77-row last block that lands on each MC of RAGGED: a ragged last
   chunk (M = 5: 3 + 2 and 2 + 2 + 1; M = 7: 4 + 3 and 2 + 2 + 2 + 1; M = 3: 2 + 1), MC = 1, and whole rows (mc == M: the
   16-byte store with its byte tail).  At most 233 k rows (304 CUs); the oracle judges oracle_rows(B).  Padded pitch: a view
   with ldx = D + 4, NaN in the padding, at M = 5; the method stays "mfma".

What writing this file found.  (1) The header of pq_assign_mfma.hip derived the dropped products with a bf16 unit round-off of
2^-9; it is 2^-8, the term is 8 * 2^-18 = 3.05e-5 of the scale, not 1.2e-5, and the constant 1.8e-5 that carried it is 3.63e-5
now.  No wrong code was observed with the earlier constant and the model does not predict one: the coherent family's screen
error, 4.47e-5 of the scale between A and B, is 0.56 / 0.53 / 0.15 of the EARLIER margin at dsub 8 / 16 / 96 (0.38 / 0.37 /
0.14 of the present one); the accumulation allowance covered what the first term lacked.  (2) orc_argmin of the C oracle
started its scan from d[0], so a NaN distance at k = 0 won by standing first while a NaN anywhere else never won, and both
kernels let it win nowhere; the scan starts from +inf now, and pq_oracle.quantize (np.argmin: the first NaN won) masks NaN the
same way.  A NaN row, where every distance is NaN, gives code 0 as before.

Sensitivity, on the model only (test_margin_sensitivity_on_the_split_model; no weakened kernel was built or run).  At g = 0 the
reference prefers A by 1e-5 margins and the model screen prefers B by 4.47e-5 of the scale.  A screen whose margin is below
that decides the pair, for the wrong centroid: that is any margin below 0.38 / 0.37 / 0.14 of the compiled one at dsub 8 / 16 /
96.  HALF the compiled margin (5.85e-5 / 6.04e-5 / 1.66e-4) is still above it, so halving the present constant is NOT noticed
by this family, at g = 1.1 or elsewhere: at g = 1.1 half a margin lets the screen decide the A-nearer pairs (lead 0.71
margins), for the right centroid.  Half the EARLIER margin (4.02e-5 / 4.21e-5 at dsub 8 / 16) is below it: a kernel with the
earlier derivation and half its margin would have coded the g = 0 rung wrongly, which the GPU test would report.
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
ROWS_PER_BLOCK = 256                                      # MF_ROWS_PER_BLOCK
STEP = 2.0 ** -7                                          # one bf16 ulp in [1, 2)
P_PLUS, P_MINUS = 0x3F807F40, 0x3F8080C0                  # 1.0038834 (vl, rest > 0, near their maxima), 1.0039291 (both < 0)
RUNGS = (0.0, 0.3, 0.6, 0.9, 1.1, 1.6, 3.0, 6.0)
COHERENT = ((8, 16), (16, 48), (96, 8))                   # (dsub, M)
COHERENT_B = 300                                          # two blocks, the second partial
SCALES = (0, -20, 10, 40)                                 # powers of two, by sub-quantiser
# (position of A, position of B): the ends, a folded pair, the half-waves, two tiles, the first and the last tile
AB_POSITIONS = ((0, 255), (255, 0), (2, 3), (36, 32), (31, 63), (250, 5), (128, 127), (19, 212))


def bits(u):
    return np.array(u, np.uint32).view(F32)[()]


# ------------------------------------------------------------------------------------------------ 1. the split, restated
def bf16_round(v):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32; finite inputs (v_cvt_pk_bf16_f32 as mf_split2 uses it)."""
    u = np.ascontiguousarray(v, F32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(F32)


def split2(v, rnd=bf16_round):
    """mf_split2: (vh, vl, rest) with v = vh + vl + rest; vh, vl bf16 values, v - vh exact in fp32, rest in fp64."""
    v = np.ascontiguousarray(v, F32)
    vh = rnd(v)
    r = v - vh
    assert np.array_equal(r.astype(F64), v.astype(F64) - vh.astype(F64))
    vl = rnd(r)
    return vh, vl, r.astype(F64) - vl.astype(F64)


def screen_model(x, c, rnd=bf16_round):
    """The three kept products in fp64, nothing else rounded: S[k] = ||c_k||^2 + wh.xh + wh.xl + wl.xh, w = -2 c, for one
    sub-vector x [dsub] and centroids c [n, dsub].  Returns (S, e) with e = S - (||c||^2 - 2 <c, x>), the dropped terms."""
    xh, xl, _ = split2(x, rnd)
    wh, wl, _ = split2((F32(-2) * np.asarray(c, F32)).astype(F32), rnd)
    xh, xl, wh, wl = (a.astype(F64) for a in (xh, xl, wh, wl))
    c64, x64 = np.asarray(c, F64), np.asarray(x, F64)
    cn = (c64 * c64).sum(-1)
    S = cn + (wh * xh + wh * xl + wl * xh).sum(-1)
    return S, S - (cn - 2.0 * (c64 * x64).sum(-1))


# ------------------------------------------------------------------------------------------------ 2. the coherent family
@functools.lru_cache(maxsize=None)
def four_squares(n):
    """n = p^2 + q^2 + r^2 + s^2, p >= q >= r >= s >= 0 (Lagrange), the first found with p as small as possible."""
    p = int(np.ceil(np.sqrt(n / 4.0)))
    while p * p <= n:
        for q in range(min(p, int(np.sqrt(n - p * p))), -1, -1):
            for r in range(min(q, int(np.sqrt(n - p * p - q * q))), -1, -1):
                s2 = n - p * p - q * q - r * r
                s = int(round(np.sqrt(s2)))
                if s * s == s2 and s <= r:
                    return (p, q, r, s)
        p += 1
    raise AssertionError(n)


def far_steps(n, dsub):
    """Whole steps of the farther centroid with sum of squares n: on the first four coordinates only, so that even the widest
    rung moves its norm, and with it the scale, by little."""
    return np.array(four_squares(n) + (0,) * (dsub - 4), np.int64)


@functools.lru_cache(maxsize=None)
def coherent_pair(dsub, g, near_is_a, margin):
    """(A, B) as fp32 vectors for the row P+: the nearer one is its pattern without steps, the farther one carries
    far_steps(n), n chosen so that d_far - d_near, in exact arithmetic, is as close to g * margin * scale as whole steps
    allow.  At g = 0 that is n = 0 for either role: A = P+ is the row itself and B = P- lies dsub (3 * 2^-16)^2 away."""
    pa, pb = F64(bits(P_PLUS)), F64(bits(P_MINUS))
    x = np.full(dsub, pa)

    def build(n):
        st = far_steps(n, dsub) * STEP
        A, B = x + (0 if near_is_a else st), np.full(dsub, pb) + (st if near_is_a else 0)
        gap = ((x - B) ** 2).sum() - ((x - A) ** 2).sum()
        scale = (x * x).sum() + max((A * A).sum(), (B * B).sum())
        return A, B, (gap if near_is_a else -gap) - g * margin * scale

    if g == 0.0:
        return tuple(v.astype(F32) for v in build(0)[:2])
    n = int(g * margin * 2 * dsub / STEP ** 2)
    for _ in range(4):                                    # the cross term with P- - P+ and the scale move with the steps
        n = max(0, n - int(round(build(n)[2] / STEP ** 2)))
    best = min((build(k) for k in range(max(0, n - 40), n + 41)), key=lambda t: abs(t[2]))
    return best[0].astype(F32), best[1].astype(F32)


def coherent_layout(m):
    """(A is the nearer one, position of A, position of B, power of two) of sub-quantiser m."""
    ka, kb = AB_POSITIONS[(m + m // len(AB_POSITIONS)) % len(AB_POSITIONS)]
    return m % 2 == 0, ka, kb, SCALES[(m // 2) % len(SCALES)]


@functools.lru_cache(maxsize=None)
def coherent_case(dsub, M, g, margin):
    """x [B, M dsub], C [M, 256, dsub], want [B, M]: every sub-quantiser holds one (A, B) pair at rung g; the positions, which
    of the two is nearer and the binade vary with the sub-quantiser (coherent_layout); the other 254 centroids are the negated
    pattern with steps 0 .. 2 on the first four coordinates: about 2 per coordinate away, and of the pair's norm."""
    rng = np.random.default_rng(1000 * dsub + int(10 * g))
    pa = bits(P_PLUS)
    x = np.empty((COHERENT_B, M, dsub), F32)
    C = np.empty((M, K, dsub), F32)
    want = np.empty((COHERENT_B, M), np.uint8)
    for m in range(M):
        near_is_a, ka, kb, e = coherent_layout(m)
        two = F32(2.0) ** e
        A, B = coherent_pair(dsub, g, near_is_a, margin)
        far = np.full((K, dsub), pa, F32)
        far[:, :4] += F32(STEP) * rng.integers(0, 3, (K, 4)).astype(F32)
        C[m] = -far * two
        C[m, ka], C[m, kb] = A * two, B * two
        x[:, m] = pa * two
        want[:, m] = ka if (near_is_a or g == 0.0) else kb
    return x.reshape(COHERENT_B, M * dsub), C, want


def reference_gap(x, C, m):
    """(d[B] - d[A]) / (||x_m||^2 + max_k ||c_mk||^2) of row 0: in fp64 from the fp32 inputs, and with the numpy oracle's fp32
    distances."""
    _, ka, kb, _ = coherent_layout(m)
    dsub = C.shape[2]
    x32 = np.ascontiguousarray(x.reshape(x.shape[0], -1, dsub)[:1, m])
    xm, c = x32[0].astype(F64), C[m].astype(F64)
    scale = (xm * xm).sum() + (c * c).sum(-1).max()
    d = ((xm - c[[ka, kb]]) ** 2).sum(-1)
    d32 = pq_oracle.dist_table(x32, np.ascontiguousarray(C[m:m + 1, (ka, kb)]))[0, 0].astype(F64)
    return (d[1] - d[0]) / scale, (d32[1] - d32[0]) / scale


def model_at_rung(dsub, M, g, margin, m):
    """(reference-nearest position, the model screen's best position, |S_B - S_A| / scale, (e_A, e_B) / scale) of
    sub-quantiser m."""
    x, C, want = coherent_case(dsub, M, g, margin)
    _, ka, kb, _ = coherent_layout(m)
    xm = np.ascontiguousarray(x.reshape(x.shape[0], M, dsub)[0, m])
    c = C[m].astype(F64)
    scale = (xm.astype(F64) ** 2).sum() + (c * c).sum(-1).max()
    S, e = screen_model(xm, C[m][[ka, kb]])
    return int(want[0, m]), (ka if S[0] <= S[1] else kb), abs(S[1] - S[0]) / scale, e / scale


# --------------------------------------------------------------------------------------- 2b. the common-offset family
OFFSET_LADDER = (10.0, 100.0, 1000.0)
OFFSET_SHAPE = (600, 48, 16)                              # B, M, dsub


@functools.lru_cache(maxsize=None)
def offset_case(f):
    """Gaussian rows and centroids (clipped at 4 standard deviations) plus, in every sub-quantiser, one common vector of norm
    f sqrt(dsub), f times the spread: the margin grows with f^2, the gaps do not."""
    B, M, dsub = OFFSET_SHAPE
    rng = np.random.default_rng(4242)                     # the same Gaussian part on every rung
    x = np.clip(rng.standard_normal((B, M, dsub)), -4, 4)
    C = np.clip(rng.standard_normal((M, K, dsub)), -4, 4)
    v = rng.standard_normal((M, dsub))
    v *= f * np.sqrt(dsub) / np.linalg.norm(v, axis=1, keepdims=True)
    return (x + v[None]).astype(F32).reshape(B, M * dsub), (C + v[:, None]).astype(F32)


# ------------------------------------------------------------------------------------------------ 3. structure
EVERY_B = 256 * 3 + 77
EVERY_SHAPES = ((48, 16), (12, 64))                       # (M, dsub)


@functools.lru_cache(maxsize=None)
def every_position_case(M, dsub):
    """Row b of sub-quantiser m sits 1e-3 standard deviations from centroid (37 b + 11 m) mod 256 of a Gaussian codebook."""
    rng = np.random.default_rng(31 * M + dsub)
    C = rng.standard_normal((M, K, dsub)).astype(F32)
    want = ((37 * np.arange(EVERY_B)[:, None] + 11 * np.arange(M)[None, :]) % K).astype(np.uint8)
    x = C[np.arange(M)[None, :], want] + F32(1e-3) * rng.standard_normal((EVERY_B, M, dsub)).astype(F32)
    return x.reshape(EVERY_B, M * dsub).astype(F32), C, want


# Positions k = 32 tile + (r & 3) + 8 (r >> 2) + 4 half.  Pairs: the two values of a folded pair (r = 0, 1), two pairs
# (r = 1, 2), across r >> 2 (r = 3, 4), the half-waves, two tiles, the first and the last tile, the ends, inside the last tile
# (whose epilogue is a step of its own), the last tile across its halves.
TIE_PAIRS = ((0, 1), (1, 2), (3, 8), (0, 4), (5, 37), (6, 230), (0, 255), (254, 255), (227, 251))
TIE_TRIPLES = ((0, 1, 2), (2, 1, 0), (3, 8, 40), (40, 8, 3), (0, 4, 255), (255, 4, 0))
TIE_SHAPES = ((48, 16), (24, 32), (8, 96))                # (M, dsub): pairs only / pairs and singles / singles in the fold
TIE_B = 256 + 77
TIE_OFF = 2.0 ** -10


def tie_slots():
    """[(positions, nudges)]: the centroids at `positions` are copies of one base centroid, coordinate 0 moved by `nudge` ulps
    away from the rows (+1: one ulp farther, -1: one ulp nearer, 0: an exact duplicate)."""
    slots = []
    for i, j in TIE_PAIRS:
        slots += [((i, j), n) for n in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0))]
    for i, j, l in TIE_TRIPLES:                           # i, j duplicates; l within one ulp
        slots += [((i, j, l), (0, 0, 1)), ((i, j, l), (0, 0, -1))]
    return slots


def tie_expected(pos, nudge):
    best = min(nudge)
    return min(p for p, n in zip(pos, nudge) if n == best)


@functools.lru_cache(maxsize=None)
def tie_cases(M, dsub):
    """[(x, C, want, slots)]: the slots dealt to the sub-quantisers, M per call, the last call filled up from the front.  Every row
    of a sub-quantiser sits at its base centroid + 2^-10 in coordinate 0 and +- 2^-10 elsewhere; coordinate 0 of the base lies
    in [1, 1.5), so one ulp there is 2^-23 and moves the fp32 distance by 2^-33, 64 ulps of a sum near 2^-16."""
    rng = np.random.default_rng(7 * M + dsub)
    slots = tie_slots()
    out = []
    for s0 in range(0, len(slots), M):
        C = rng.standard_normal((M, K, dsub)).astype(F32)
        x = np.empty((TIE_B, M, dsub), F32)
        want = np.empty((TIE_B, M), np.uint8)
        for m in range(M):
            pos, nudge = slots[(s0 + m) % len(slots)]
            base = rng.standard_normal(dsub).astype(F32)
            base[0] = F32(1.0 + 0.5 * rng.random())
            for p, n in zip(pos, nudge):
                C[m, p] = base
                for _ in range(abs(n)):
                    C[m, p, 0] = np.nextafter(C[m, p, 0], F32(-np.inf if n > 0 else np.inf))
            off = np.where(rng.random((TIE_B, dsub)) < 0.5, -TIE_OFF, TIE_OFF).astype(F32)
            off[:, 0] = TIE_OFF
            x[:, m] = base[None] + off
            want[:, m] = tie_expected(pos, nudge)
        out.append((x.reshape(TIE_B, M * dsub), C, want, [slots[(s0 + m) % len(slots)] for m in range(M)]))
    return out


NONFINITE_POS = (0, 31, 32, 255)
NONFINITE_SHAPES = ((48, 16), (8, 96))
NONFINITE_B = 256 + 77


@functools.lru_cache(maxsize=None)
def nonfinite_case(M, dsub):
    """Gaussian codebooks, finite rows next to centroids; (position, value) for the 12 combinations of NONFINITE_POS and
    NaN / +inf / -inf are dealt to the sub-quantisers, one coordinate of that centroid each: to every fourth one at M = 48,
    round-robin at M = 8, where a sub-quantiser holds two of them (in sub-quantisers 0 to 3 in one centroid)."""
    rng = np.random.default_rng(99 + M)
    C = rng.standard_normal((M, K, dsub)).astype(F32)
    pick = rng.integers(0, K, (NONFINITE_B, M))
    x = C[np.arange(M)[None, :], pick] + F32(0.05) * rng.standard_normal((NONFINITE_B, M, dsub)).astype(F32)
    combos = [(p, v) for v in (np.nan, np.inf, -np.inf) for p in NONFINITE_POS]
    bad = []
    for i, (p, v) in enumerate(combos):
        m = i * M // len(combos) if M >= len(combos) else i % M
        C[m, p, (3 * i) % dsub] = v
        bad.append((m, p))
    return x.reshape(NONFINITE_B, M * dsub).astype(F32), C, bad


# ------------------------------------------------------------------------------------------------ 4. geometry
ROW_COUNTS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
RAGGED = {(5, 16): (3, 2, 1, 5), (7, 8): (4, 2, 1, 7), (3, 96): (2, 1, 3)}     # (M, dsub) -> the MC values to land on
RAGGED_MAX_ROWS = 400000


def mc_rule(B, M, cus):
    """rc_pq_assign_nearest_fast: sub-quantisers per block, halved while the grid is under 3 blocks per CU."""
    nblk = -(-B // ROWS_PER_BLOCK)
    MC = M
    while MC > 1 and nblk * (-(-M // MC)) < 3 * cus:
        MC = (MC + 1) // 2
    return MC


def rows_for(M, mc, cus):
    """The smallest B with a partial last block at which the rule gives mc; None when no B up to RAGGED_MAX_ROWS does."""
    for nblk in range(2, RAGGED_MAX_ROWS // ROWS_PER_BLOCK + 1):
        B = nblk * ROWS_PER_BLOCK - 179
        if mc_rule(B, M, cus) == mc:
            return B
    return None


def oracle_rows(B):
    """The rows the oracle judges when B is large: the first and the last two 256-row blocks and every (B // 2000)-th row."""
    if B <= 4096:
        return np.arange(B)
    return np.unique(np.concatenate([np.arange(512), np.arange(B - 512, B), np.arange(0, B, B // 2000)]))


# ================================================================================================ CPU tests
def test_split_model_round_off_over_a_binade():
    v = np.arange(0x3F800000, 0x3F800000 + (1 << 17), dtype=np.uint32).view(F32)       # [1, 1 + 2^-6): every low-bit pattern
    vh, vl, rest = split2(v)
    assert np.array_equal(vh.view(np.uint32) & 0xFFFF, np.zeros(v.size, np.uint32))
    assert np.array_equal(vl.view(np.uint32) & 0xFFFF, np.zeros(v.size, np.uint32))
    r_rest, r_vl = (np.abs(rest) / v).max() * 2.0 ** 18, (np.abs(vl) / v).max() * 2.0 ** 9
    print("max |rest| / |v| = %.4f * 2^-18, max |vl| / |v| = %.4f * 2^-9" % (r_rest, r_vl))
    assert 1.9 < r_rest <= 2.0 and 1.9 < r_vl <= 2.0
    whole = np.arange(0x3F800000, 0x40000000, 1 << 4, dtype=np.uint32).view(F32)       # the whole binade, every 16th value
    _, wl, wrest = split2(whole)
    assert (np.abs(wrest) / whole).max() <= 2.0 ** -17 and (np.abs(wl) / whole).max() <= 2.0 ** -8
    # the two patterns of the coherent family: both pieces positive at P+, both negative at P-
    for pat, sign in ((P_PLUS, 1), (P_MINUS, -1)):
        _, pl, prest = split2(np.array([bits(pat)], F32))
        assert sign * pl[0] > 0.98 * 2.0 ** -9 and sign * prest[0] > 0.98 * 2.0 ** -18


@pytest.mark.parametrize("dsub,M", COHERENT)
def test_coherent_family_strains_the_dropped_terms(dsub, M):
    from repconc_amd import ops
    margin = ops.assign_margin(dsub)
    for g in RUNGS:
        for m in range(min(M, 16)):
            _, _, _, e = model_at_rung(dsub, M, g, margin, m)
            assert e[0] >= 2.9e-5 and e[1] <= -1.4e-5, (g, m, e)


@pytest.mark.parametrize("dsub,M", COHERENT)
def test_coherent_gaps_are_what_they_state(dsub, M):
    """Every rung's reference gap is g * margin * scale to within one step of the construction, 2^-14 in the row's units, in
    fp64 and in the oracle's fp32 arithmetic alike; the oracle's codes are the planted ones."""
    from repconc_amd import ops
    margin = ops.assign_margin(dsub)
    for g in RUNGS:
        x, C, want = coherent_case(dsub, M, g, margin)
        assert np.array_equal(pq_oracle.quantize(x[:2], C, False), want[:2])
        for m in range(M):
            near_is_a = coherent_layout(m)[0]
            g64, g32 = reference_gap(x, C, m)
            quantum = STEP ** 2 / (2 * dsub)              # scale >= 2 dsub in the row's units
            sign = 1.0 if (near_is_a or g == 0.0) else -1.0
            assert abs(sign * g64 - g * margin) <= quantum and abs(sign * g32 - g * margin) <= quantum, (g, m, g64, g32)
            if g == 0.0:                                  # A is the row itself, B is 9 dsub 2^-32 away: A wins, by a hair
                assert 0 < g64 < 1e-4 * margin and g32 > 0


def test_margin_sensitivity_on_the_split_model():
    """What the coherent family can notice, on the model (no kernel is weakened for this).  At g = 0 the reference prefers A
    by a hair and the model screen prefers B by (e_A - e_B) = 4.4e-5 of the scale: a screen whose margin is below that
    decides the pair, wrongly.  The compiled margin is above it at every width (the pair goes to the judge), half the
    constant the kernel had before its derivation was corrected is below it at dsub 8 and 16."""
    from repconc_amd import ops
    for dsub, M in COHERENT:
        margin = ops.assign_margin(dsub)
        kp = (dsub + 15) // 16 * 16
        earlier = 2 * (1.8e-5 + (3 * kp + 7) * 3.6e-7 + (2 * dsub + 4) * 1.2e-7)
        for m in (0, 1):
            ref, scr, lead, _ = model_at_rung(dsub, M, 0.0, margin, m)
            _, ka, kb, _ = coherent_layout(m)
            print("dsub %d: model lead of B at g = 0: %.3e = %.3f margins (%.3f of the earlier constant)"
                  % (dsub, lead, lead / margin, lead / earlier))
            assert ref == ka and scr == kb and 4.3e-5 < lead < margin
            if dsub <= 16:
                assert lead > 0.5 * earlier
        # at g = 1.1 the model screen leads with the right centroid; where A is the nearer one its lead is below the margin
        # (the judge decides), where B is, the dropped terms widen the lead beyond it (the screen decides)
        for m in (0, 1):
            ref, scr, lead, _ = model_at_rung(dsub, M, 1.1, margin, m)
            near_is_a = coherent_layout(m)[0]
            assert ref == scr and (lead < margin) == near_is_a


def test_tie_constructions_are_ties_in_the_oracle_arithmetic():
    assert len(tie_slots()) == 5 * len(TIE_PAIRS) + 2 * len(TIE_TRIPLES)
    for M, dsub in TIE_SHAPES:
        seen = set()
        for x, C, want, slots in tie_cases(M, dsub):
            d = pq_oracle.dist_table(x[:5], C)                                  # [M, 5, 256]
            assert np.array_equal(np.argmin(d, -1).T, want[:5])
            for m, (pos, nudge) in enumerate(slots):
                seen.add((pos, nudge))
                rest = np.delete(d[m], pos, axis=1)
                for p, n in zip(pos, nudge):              # equal where the nudges are equal, strictly ordered where not
                    assert (rest > 1000 * d[m][:, p:p + 1]).all()
                    for q, k in zip(pos, nudge):
                        assert (np.sign(d[m][:, p] - d[m][:, q]) == np.sign(n - k)).all(), (pos, nudge)
        assert len(seen) == len(tie_slots())


def test_every_position_and_non_finite_inputs_are_what_they_claim():
    for M, dsub in EVERY_SHAPES:
        x, C, want = every_position_case(M, dsub)
        for m in range(M):
            for b0 in range(0, EVERY_B - ROWS_PER_BLOCK + 1, ROWS_PER_BLOCK):   # all 256 positions win in every block ...
                assert len(np.unique(want[b0:b0 + ROWS_PER_BLOCK, m])) == K
            for b0 in range(0, EVERY_B - 31, 32):                               # ... 32 different ones in every column set
                assert len(np.unique(want[b0:b0 + 32, m])) == 32
        for c in range(32):                               # ... and every column meets every tile, and both half-waves
            assert len(np.unique(want[c::32] // 32)) == 8 and len(np.unique(want[c::32] // 4 % 2)) == 2
        assert np.array_equal(pq_oracle.quantize(x[:64], C, False), want[:64])
    for M, dsub in NONFINITE_SHAPES:
        x, C, bad = nonfinite_case(M, dsub)
        assert np.isfinite(x).all() and len(bad) == 12 and np.isnan(C).sum() == 4 and np.isinf(C).sum() == 8
        codes, _ = c_oracle.quantize(x, C, False)
        assert np.array_equal(codes[:40], pq_oracle.quantize(x[:40], C, False))
        for m, p in bad:                                  # a non-finite centroid never wins
            assert (codes[:, m] != p).all()
        assert len(np.unique(codes)) == K


def test_restated_mc_rule_lands_where_intended():
    assert mc_rule(196353, 5, 256) == 5 and mc_rule(196352, 5, 256) == 3          # 768 blocks / 767
    assert mc_rule(98049, 5, 256) == 3 and mc_rule(98048, 5, 256) == 2            # 384 / 383
    assert mc_rule(65281, 5, 256) == 2 and mc_rule(65280, 5, 256) == 1            # 256 / 255
    assert mc_rule(1 << 20, 48, 256) == 48 and mc_rule(1000, 48, 256) == 1
    for cus in (256, 304):
        for (M, dsub), targets in RAGGED.items():
            for mc in targets:
                B = rows_for(M, mc, cus)
                assert B is not None and B <= RAGGED_MAX_ROWS and B % ROWS_PER_BLOCK == 77, (cus, M, mc, B)
                assert mc_rule(B, M, cus) == mc
                assert B * M * dsub * 4 <= 300 << 20
                ragged = M % mc != 0
                assert ragged == ((M, mc) in ((5, 3), (5, 2), (7, 4), (7, 2), (3, 2)))


# ================================================================================================ GPU tests
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _three_ways(x, C, dtype=torch.uint8, rows=None):
    """mfma codes (numpy) and statistics, after checking them against the exact kernel on all rows and the oracle on `rows`."""
    from repconc_amd import ops
    xt, Ct = (x if torch.is_tensor(x) else _t(x)), _t(C)
    st = {}
    fast = ops.assign_nearest(xt, Ct, dtype, method="mfma", stats=st)
    exact = ops.assign_nearest(xt, Ct, dtype, method="exact")
    assert st["method"] == "mfma" and not st["overflow"]
    assert fast.dtype == dtype and torch.equal(fast, exact)
    got = fast.cpu().numpy()
    if rows is None:
        xo = x.cpu().numpy() if torch.is_tensor(x) else x
        assert np.array_equal(got, c_oracle.quantize(xo, C, False)[0])
    else:
        xo = xt[torch.from_numpy(rows).to(DEV)].cpu().numpy()
        assert np.array_equal(got[rows], c_oracle.quantize(xo, C, False)[0])
    return got, st


@gpu
@pytest.mark.parametrize("g", RUNGS)
@pytest.mark.parametrize("dsub,M", COHERENT)
def test_coherent_family_on_the_kernel(dsub, M, g):
    from repconc_amd import ops
    x, C, want = coherent_case(dsub, M, g, ops.assign_margin(dsub))
    got, st = _three_ways(x, C)
    print("dsub %d g %.1f: doubtful %d of %d" % (dsub, g, st["doubtful"], COHERENT_B * M))
    assert np.array_equal(got, want)
    if g == 0.0:
        assert st["doubtful"] == COHERENT_B * M
    if g >= 3.0:                                          # a gap of 3 margins less a screen error of at most 2 E = 1 margin
        assert st["doubtful"] == 0


@gpu
def test_common_offset_ladder():
    B, M, dsub = OFFSET_SHAPE
    counts = []
    for f in OFFSET_LADDER:
        x, C = offset_case(f)
        _, st = _three_ways(x, C)
        counts.append(st["doubtful"])
    print("doubtful along the ladder:", counts, "of", B * M)
    assert counts == sorted(counts)


@gpu
@pytest.mark.parametrize("M,dsub", EVERY_SHAPES)
def test_every_position_wins_everywhere(M, dsub):
    x, C, want = every_position_case(M, dsub)
    got, st = _three_ways(x, C)
    assert np.array_equal(got, want)
    assert st["doubtful"] < EVERY_B * M // 20


@gpu
@pytest.mark.parametrize("M,dsub", TIE_SHAPES)
def test_ties_and_near_ties_across_every_boundary(M, dsub):
    for x, C, want, _ in tie_cases(M, dsub):
        got, st = _three_ways(x, C, torch.int64)
        assert np.array_equal(got, want)
        assert st["doubtful"] == TIE_B * M                # every pair here is a tie or one ulp from one


@gpu
@pytest.mark.parametrize("M,dsub", NONFINITE_SHAPES)
def test_non_finite_centroids(M, dsub):
    x, C, bad = nonfinite_case(M, dsub)
    got, _ = _three_ways(x, C)
    for m, p in bad:
        assert (got[:, m] != p).all()


@gpu
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
@pytest.mark.parametrize("M", [48, 96])
def test_row_counts(M, dtype):
    rng = np.random.default_rng(500 + M)
    x = rng.standard_normal((max(ROW_COUNTS), 768)).astype(F32)
    C = rng.standard_normal((M, K, 768 // M)).astype(F32)
    want = c_oracle.quantize(x, C, False)[0]
    for B in ROW_COUNTS:
        got, _ = _three_ways(x[:B], C, dtype)
        assert np.array_equal(got, want[:B])


def _ragged_params():
    return [(M, dsub, mc) for (M, dsub), targets in RAGGED.items() for mc in targets]


@gpu
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
@pytest.mark.parametrize("M,dsub,mc", _ragged_params())
def test_ragged_sub_quantiser_chunks(M, dsub, mc, dtype):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = rows_for(M, mc, cus)
    if B is None:
        pytest.skip("MC = %d at M = %d needs more than %d rows on a device with %d CUs" % (mc, M, RAGGED_MAX_ROWS, cus))
    assert mc_rule(B, M, cus) == mc
    gen = torch.Generator(device=DEV).manual_seed(1000 * M + mc)
    x = torch.randn((B, M * dsub), device=DEV, generator=gen)
    C = np.random.default_rng(M + mc).standard_normal((M, K, dsub)).astype(F32)
    _three_ways(x, C, dtype, rows=oracle_rows(B))


@gpu
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int64])
def test_padded_row_pitch_at_a_ragged_width(dtype):
    M, dsub = 5, 16
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = rows_for(M, 2, cus)
    assert B is not None and mc_rule(B, M, cus) == 2
    D = M * dsub
    buf = torch.full((B, D + 4), float("nan"), device=DEV)
    buf[:, :D] = torch.randn((B, D), device=DEV, generator=torch.Generator(device=DEV).manual_seed(8))
    x = buf[:, :D]
    assert x.stride(0) == D + 4 and x.data_ptr() % 16 == 0
    C = np.random.default_rng(8).standard_normal((M, K, dsub)).astype(F32)
    _, st = _three_ways(x, C, dtype, rows=oracle_rows(B))
    assert st["method"] == "mfma"                         # no realigning copy was taken
