"""The IVF build side on constructed cells, ties and sizes: the coarse assignment (rc_ivf_coarse_assign, csrc/ivf_search.hip), the
coarse centroid update (rc_ivf_coarse_update, csrc/kmeans.hip), the probe selection (rc_ivf_select_probes, csrc/ivf_lists.hip) and
what repconc_amd/ivf.py builds from them (coarse_assign, coarse_kmeans, IVFPQIndex.probe / set_lists / add).

Every tolerance of this file is bit equality, except BOUND below, which is derived.  Nothing is measured.  Generators are module
level, seeded, numpy on the CPU; the CPU tests check that the inputs are what they claim.

1. COARSE ASSIGNMENT.  Reference: a numpy restatement of the kernels' arithmetic (score_ref, cell_ref).
     cnorm[c]  lane l of 64 runs the fp32 fma chain s = fma(c_j, c_j, s) over j = l, l + 64, ...; then s += shfl_xor(s, o) for
               o = 32, 16, ..., 1.  fp32 addition commutes, so all 64 lanes hold the same tree: cnorm_ref is that tree.
     acc       the fp32 fma chain over d ascending from +0 (acc_ref; fmaf_emul of test_dense_flat.py, extended to non-finite
               operands by fma32, which a CPU test checks against the C library's fmaf).
     score     fl(cnorm - 2 acc); 2 acc is exact, so a contracted fma would give the same bits.
     cell      the first minimum over c; a NaN score never wins; cell 0 when no score compares below +inf.
   Families.  `ints`: integers |v| <= 8: every product, partial sum, norm and score is an integer below 2^24 for D <= 1024
   (|acc| <= 64 D, cnorm <= 64 D, |score| <= 192 D < 2^18), so every summation order gives the same bits and the fp64 argmin IS
   the reference (ints_ref); D in {16, 32, 48, 768, 1024}.  `gauss`: N(0, 1) with 2^-20 <= |v| <= 2^6, so every product lies in
   [2^-40, 2^12] and every partial sum is a multiple of 2^-63: nothing is ever subnormal; the chain restatement at B <= 257,
   nlist <= 300, D in {16, 64}, with pairs of centroids one ulp apart in one coordinate.
   Cases: every B in {1, 63, 64, 65, 127, 128, 129, 257} x nlist in {1, 127, 128, 129, 255, 256, 257, 300}; ldx = D + 4 (NaN in
   the padding) through a strided view and through the raw C entry; "every centroid wins somewhere" (the documents are the
   centroids, permuted: a slot-to-centroid formula that maps two of a lane's 16 slots to one centroid cannot pass);  exact ties
   at centroid distance 1, 4, 8, 32, 64, 128, 129 and (200, 299) with nlist = 300, the last valid cell of a ragged list tile -
   one per structural boundary of the kernel: the r & 3 neighbours, the half-wave (4 half; once with the lower cell in each
   half), r >> 2, the row tile a, the wave wr, the list tile, and a list tile plus one (lower cell in wave 1, upper in wave 0) -
   the lower cell expected; the mirror case (the document sits on the upper copy,
   the lower one is off in one coordinate by the family's smallest step): the upper cell expected.  The step is 1 for `ints`;
   for `gauss` the gap in distance is the square of the step, so it is the smallest power of two of ulps at which the
   restatement's fp32 scores tell the two apart (one-ulp pairs are in the sweep, where the restatement decides);  non-finite
   rows: a NaN entry, an all +inf and an all -inf row, a row whose products are finite and whose SUM overflows, a centroid whose
   squares are finite and whose NORM overflows, a centroid holding a NaN (never chosen, the other rows' cells are those of the
   restatement);  the D % 16 != 0 library fallback of coarse_assign at D = 24, `ints`, with ties: the same first minimum.
   BOUND (the property test kept from test_gpu_parity.py, D = 768 Gaussian): the chosen cell's fp64 score is the fp64 minimum up
   to  e(g) + e(b),  e(c) = (D + 2) u (||c||^2 + 2 sum_j |x_j c_j|),  u = 2^-24,  g the chosen and b the fp64-best cell.
   Derivation: the kernel picks g with fl-score(g) <= fl-score(b), so score(g) - score(b) <= |err(g)| + |err(b)|.  cnorm carries
   at most D / 64 + 6 roundings per term (all terms positive): (D / 64 + 6) u ||c||^2 (1 + O(u)).  A chain of D fmas carries at
   most D roundings per term: |acc - x.c| <= gamma(D) sum |x_j c_j|, gamma(D) = D u / (1 - D u), doubled exactly.  The final
   subtraction is one rounding of a value below (||c||^2 + 2 sum |x_j c_j|)(1 + gamma(D)).  Together below
   (D + 1) u (1 + D u)(...) <= (D + 2) u (...) because (D + 1) D u < 1 for D <= 1024.  The fp64 reference's own error, about
   D 2^-53 of the same magnitudes, is nine orders below it.  The CPU test checks the bound entry by entry on the restatement.

2. COARSE UPDATE.  `ints` data (integers |v| <= 1024, cells of at most 5000 rows): every fp64 partial sum is an integer below
   2^53, so fl32(sum / cnt) does not depend on the order: numpy add.at in int64, one fp64 division, one cast (update_ref).
   Cell sizes: every size 0 .. 70 in one call (both sides of the unrolled loop's i + 28 < cnt at 28 / 29, 32 / 33, 60 / 61) and
   2047, 2048, 2049, 4097 (IVFC_TILE = 2048), the cell labels permuted, laid out round-robin (every large cell spans every
   tile) and as contiguous runs (the large ones straddle tile edges), with rows assigned to -1, nlist, nlist + 5, INT_MIN and
   INT_MAX sprinkled in: ignored in the counts and in the means.  Geometry: n in {1, 2047, 2048, 2049, 20011}, nlist in {1, 255,
   256, 257, 700, 16384}, D in {4, 16, 768, 1024}, ldx = D + 4, counts_out given and NULL; one call with EVERY assignment out
   of range.  Empty cells: row splitmix64(seed ^ splitmix64(iter << 32 | cell)) mod n restated in Python integers, required bit
   for bit, for iter 0, a seed >= 2^63 (the argument is declared c_uint64 in _lib.PROTOTYPES), seed 2^64 - 1 and n no power of
   two.  Gaussian data: the kernel's order restated (four interleaved row lanes, each ascending, ((p0 + p1) + p2) + p3) for EVERY
   cell of the size sweep, and identical bits on a second call.

3. PROBE SELECTION.  Reference (probes_ref): lexsort by (key descending, cell ascending) on the float bits, the first nprobe,
   sorted ascending.  The key is the header's order: that of the numbers, -0.0 and +0.0 equal; a NaN by its bits (above +inf
   with the sign clear, below -inf with it set).  nlist in {1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 5000, 16384} (both sides
   of the 1024-thread chunking), nprobe in {1, 2, nlist // 3 + 1, nlist - 1, nlist}; families: all equal; two values; ascending
   and descending ramps; values that differ only in the lowest key byte (the fourth radix pass decides), the same with mixed
   signs; blocks of +inf and -inf; denormals; +-0 among positive and negative values.  Every output: exactly nprobe distinct
   cells, ascending, in [0, nlist).  For every family the set equals IVFPQIndex.probe(ordered=True) and probe(ordered=False) on
   the same index (both see the scores of the same library GEMM, coarse [nlist, 1] times q = [[1]]).

4. THE PIECES TOGETHER.  coarse_kmeans on `ints` data (n = 3000, D = 16, nlist = 40, iters 0, 1, 3) equals, bit for bit, the
   numpy loop of the references above (seeded permutation init, score_ref / cell_ref, update_ref with the empty-cell rule).  The
   initial centroids are rows of x, so none can be far from ALL the data; a cell is empty after the first assignment exactly
   when its centroid duplicates a lower cell's: three such pairs are planted, one of them a far outlier pair, so the empty
   rule fires at iteration 0.  Between two iterations without an empty cell the fp64 objective does not increase beyond the sum
   over the rows of BOUND for the two cells involved (plus the second-order term of the rounded mean).  set_lists / add with
   empty cells at the start, in the middle and at the end: list_off is the exclusive cumsum, ids the stable order, codes the
   cells' rows in corpus order, and search(nprobe = nlist) equals the flat search on both paths.

What writing this file found, and what is fixed with it.  (1) ivf_probe_select_kernel ordered the raw bits, so -0.0 ranked below
+0.0 and a lower cell holding -0.0 lost the boundary to a higher cell holding +0.0, against the header and against the
stable-sort branch of probe(ordered=True); the kernel now keys s + 0.0f (adc_order_key itself is unchanged: the top-k tests pin
it).  (2) rc_ivf_coarse_assign loaded float4 from x and cent without the alignment check its sibling has: a misaligned pointer
is now RC_ESHAPE before any launch (tested on the return code only; nothing is ever launched on a misaligned pointer), and
coarse_assign copies a centroid view at an odd storage offset.  (3) probe(ordered=True) selected with torch.topk below
nprobe <= nlist / 4; topk selects by the bits too (run on the MI355X against probes_ref: 10 of the 160 (family, nlist, nprobe)
cases tried differed, all of them in the two +-0 families) and promises nothing about WHICH of several equal scores it returns;
the path is a stable sort of the row now (no search uses it).  (4) The header now says how NaN scores order and what the
assignment does with NaN and +inf scores.

Sensitivity, shown once each on scratch builds of the library (memory-safe mutations of WHICH value is computed or compared):
8 (r >> 2) -> 4 (r >> 2) in the epilogue's centroid index fails 31 tests here (every assignment test but the fallback and the
refusal, k-means, add); the half-wave merge without `oi < bidx` fails the four direct tie cases (pair (20, 24)), the ints-16
sweep and k-means; the wave merge without its tie rule fails the four direct tie cases (pair (127, 256)) and the ints-48 sweep;
the cell-mean tail loop starting one stride late fails every update test but the all-empty one, and k-means; without + 0.0f
the probe families fail at every nlist >= 2.  The earlier tests noticed the first and the fourth, not the other three.
"""
import ctypes as C
import ctypes.util
import functools

import numpy as np
import pytest
import torch

from test_dense_flat import chain_scores, fmaf_emul

gpu = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
U = 2.0 ** -24                                            # unit roundoff of fp32
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
RC_ESHAPE = -2

ASSIGN_B = (1, 63, 64, 65, 127, 128, 129, 257)
ASSIGN_NLIST = (1, 127, 128, 129, 255, 256, 257, 300)
INTS_D = (16, 32, 48, 768, 1024)
GAUSS_D = (16, 64)
# (lower, upper) centroid pairs, nlist = 300: distance 1, 4, 4, 8, 32, 64, 128, 129, and the last valid cell of the ragged tile.
# (48, 52) has the lower cell in half-wave 0; (20, 24) has it in half-wave 1 (and the upper one a slot further in half-wave 0),
# the case in which the half-wave merge's tie rule decides.  (127, 256): the lower cell in wave wr = 1, the upper in wr = 0 of
# the third list tile, the case in which the wave merge's tie rule decides.
TIE_PAIRS = ((10, 11), (48, 52), (20, 24), (33, 41), (66, 98), (60, 124), (100, 228), (127, 256), (200, 299))
TIE_NLIST, TIE_B = 300, 257


# ------------------------------------------------------------------------------------------------ 1. assignment: reference
def fma32(a, b, c):
    """Correctly rounded fp32 fma, elementwise with broadcasting, non-finite operands included (fmaf_emul covers the finite
    ones; with an infinity or a NaN among the operands the fp64 expression a b + c is already the IEEE answer)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        exact = a.astype(F64) * b.astype(F64) + c.astype(F64)
        r = fmaf_emul(a, b, c)
        return np.where(np.isfinite(exact), r, exact.astype(F32)).astype(F32)


def cnorm_ref(cent):
    cent = np.asarray(cent, F32)
    L, D = cent.shape
    s = np.zeros((L, 64), F32)
    for j0 in range(0, D, 64):
        w = min(64, D - j0)
        s[:, :w] = fma32(cent[:, j0:j0 + w], cent[:, j0:j0 + w], s[:, :w])
    lanes = np.arange(64)
    with np.errstate(all="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
    assert (s.view(np.uint32) == s[:, :1].view(np.uint32)).all() or np.isnan(s).any()      # every lane holds the same tree
    return s[:, 0].copy()


def acc_ref(x, cent):
    x, cent = np.asarray(x, F32), np.asarray(cent, F32)
    s = np.zeros((x.shape[0], cent.shape[0]), F32)
    for d in range(x.shape[1]):
        s = fma32(x[:, d:d + 1], cent[None, :, d], s)
    return s


def score_ref(x, cent):
    with np.errstate(all="ignore"):
        return (cnorm_ref(cent)[None, :] - F32(2) * acc_ref(x, cent)).astype(F32)


def cell_ref(S):
    """First minimum; NaN never wins; 0 when nothing compares below +inf (argmin of an all-inf row is 0)."""
    return np.where(np.isnan(S), np.inf, S).argmin(1).astype(np.int32)


def ints_scores(x, cent):
    """||c||^2 - 2 <x, c> in fp64 on integer data: exact."""
    x64, c64 = x.astype(F64), cent.astype(F64)
    return (c64 * c64).sum(1)[None, :] - 2.0 * (x64 @ c64.T)


def ints_ref(x, cent):
    return ints_scores(x, cent).argmin(1).astype(np.int32)


def err_bound(x, cent):
    """e(c) of BOUND for every (row, cell), fp64 [B, nlist]."""
    x64, c64 = x.astype(F64), cent.astype(F64)
    D = x.shape[1]
    return (D + 2) * U * ((c64 * c64).sum(1)[None, :] + 2.0 * (np.abs(x64) @ np.abs(c64).T))


# ------------------------------------------------------------------------------------------------- 1. assignment: families
def ints_data(shape, seed, lim=8):
    return np.random.default_rng(seed).integers(-lim, lim + 1, size=shape).astype(F32)


def gauss_data(shape, seed):
    v = np.random.default_rng(seed).standard_normal(shape).astype(F32)
    mag = np.clip(np.abs(v), F32(2.0 ** -20), F32(2.0 ** 6))
    return np.where(np.signbit(v), -mag, mag).astype(F32)


FAMILY = {"ints": ints_data, "gauss": gauss_data}


def one_ulp_pairs(cent, seed):
    """Centroids 2 k + 1 (k < nlist // 8) become copies of 2 k moved one ulp in one coordinate: [(lower, upper, coordinate)]."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(cent.shape[0] // 8):
        j = int(rng.integers(0, cent.shape[1]))
        cent[2 * k + 1] = cent[2 * k]
        cent[2 * k + 1, j] = np.nextafter(cent[2 * k, j], F32(np.inf) if k % 2 else F32(-np.inf))
        out.append((2 * k, 2 * k + 1, j))
    return out


@functools.lru_cache(maxsize=None)
def sweep_case(family, D):
    """x [257, D], cent [300, D] and the full reference score matrix: the cell of (B, nlist) is the first minimum of its
    [:B, :nlist] corner, because a score depends on its own row and centroid only."""
    x = FAMILY[family]((max(ASSIGN_B), D), 100 + D)
    cent = FAMILY[family]((max(ASSIGN_NLIST), D), 200 + D)
    if family == "gauss":
        one_ulp_pairs(cent, 300 + D)
        x[:64] = cent[np.random.default_rng(400 + D).integers(0, 80, 64)]      # documents ON the one-ulp pairs (and others)
    else:
        x[:40] = cent[np.random.default_rng(400 + D).integers(0, cent.shape[0], 40)]
    S = ints_scores(x, cent) if family == "ints" else score_ref(x, cent)
    for a in (x, cent, S):
        a.setflags(write=False)
    return x, cent, S


def tie_case(family, D, mirror):
    """cent [300, D] with TIE_PAIRS duplicated, x [257, D]: row i sits on pair i % 11 (i % 11 >= 9: a random row), so every pair
    meets every column, half-wave, wave and block position.  mirror: the LOWER copy is moved by the family's smallest step
    (module docstring) in one coordinate and the document stays on the upper one.  -> x, cent, rows [(row, lower, upper)]."""
    cent = FAMILY[family]((TIE_NLIST, D), 500 + D)
    x = FAMILY[family]((TIE_B, D), 600 + D)
    rng = np.random.default_rng(700 + D)
    for lo, hi in TIE_PAIRS:
        cent[hi] = cent[lo]
        if mirror:
            j = int(rng.integers(0, D))
            if family == "ints":
                cent[lo, j] += F32(1) if cent[lo, j] < 8 else F32(-1)
            else:
                # the gap in distance is the SQUARE of the step: one ulp never reaches the fp32 score.  The smallest power of
                # two of ulps (away from zero: adding to the bits) at which the restatement tells the two scores apart
                base = cent[lo, j].view(np.uint32)
                for k in range(24):
                    cent[lo, j] = (base + np.uint32(1 << k)).view(F32)
                    s2 = score_ref(cent[hi:hi + 1], cent[[lo, hi]])[0]
                    if s2[1] < s2[0]:
                        break
                else:
                    raise AssertionError("no step separates the pair")
    rows = []
    for i in range(TIE_B):
        if i % 11 < 9:
            lo, hi = TIE_PAIRS[i % 11]
            x[i] = cent[hi]
            rows.append((i, lo, hi))
    return x, cent, rows


def nonfinite_case(D):
    """gauss x [70, D], cent [140, D] (two list tiles) with the non-finite rows of the docstring.  Centroids are clipped to
    |c| <= 3 so that 1e38 c is finite for every entry: row 12 overflows in the SUM only."""
    x = gauss_data((70, D), 800 + D)
    cent = np.clip(gauss_data((140, D), 900 + D), -3, 3).astype(F32)
    x[3, 5] = np.nan
    x[10, :] = np.inf
    x[11, :] = -np.inf
    x[12, :] = 1e38
    cent[20, :] = 3.0                       # <x12, c20> = D * 3e38: every product finite, the third partial sum is not
    cent[30, :] = 1.5e19                    # squares 2.25e38 finite, their sum is not: cnorm = +inf
    cent[7, 3] = np.nan
    cent[131, D - 1] = np.nan               # ... and one in the ragged second tile
    return x, cent


# ------------------------------------------------------------------------------------------------------- 2. update: reference
_M64 = (1 << 64) - 1


def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def empty_row(seed, it, cell, n):
    return splitmix64((seed & _M64) ^ splitmix64(((it & 0xFFFFFFFF) << 32) | (cell & 0xFFFFFFFF))) % n


def update_ref(x, assign, nlist, seed, it):
    """-> (cent fp32 [nlist, D], counts int64 [nlist]) for INTEGER x: exact sums, one fp64 division, one cast."""
    n, D = x.shape
    ok = (assign >= 0) & (assign < nlist)
    cnt = np.bincount(assign[ok].astype(np.int64), minlength=nlist)
    sums = np.zeros((nlist, D), np.int64)
    np.add.at(sums, assign[ok].astype(np.int64), x[ok].astype(np.int64))
    cent = np.empty((nlist, D), F32)
    nz = cnt > 0
    cent[nz] = (sums[nz].astype(F64) / cnt[nz, None].astype(F64)).astype(F32)
    for c in np.nonzero(~nz)[0]:
        cent[c] = x[empty_row(seed, it, int(c), n)]
    return cent, cnt


def update_ref_lanes(x, assign, nlist, seed, it):
    """The kernel's summation order for ANY x: four interleaved row lanes, each ascending, then ((p0 + p1) + p2) + p3."""
    n, D = x.shape
    x64 = x.astype(F64)
    cent = np.empty((nlist, D), F32)
    for c in range(nlist):
        rows = np.nonzero(assign == c)[0]
        if rows.size == 0:
            cent[c] = x[empty_row(seed, it, c, n)]
            continue
        parts = []
        for lane in range(4):
            acc = np.zeros(D)
            for r in rows[lane::4]:
                acc = acc + x64[r]
            parts.append(acc)
        cent[c] = ((((parts[0] + parts[1]) + parts[2]) + parts[3]) / F64(rows.size)).astype(F32)
    return cent


SWEEP_SIZES = tuple(range(71)) + (2047, 2048, 2049, 4097)


def OUT_OF_RANGE(nlist):
    return (-1, nlist, nlist + 5, INT_MIN, INT_MAX)


@functools.lru_cache(maxsize=None)
def sweep_assign(layout):
    """int32 assignments realising SWEEP_SIZES (cell labels permuted), `round_robin` or `runs`, with 40 out-of-range rows
    inserted at random places.  -> (assign, sizes by label)."""
    rng = np.random.default_rng(31)
    sizes = np.array(SWEEP_SIZES, np.int64)
    nlist = sizes.size
    cells = np.repeat(np.arange(nlist), sizes)
    if layout == "round_robin":
        pos = (np.concatenate([np.arange(m) for m in sizes]) + 0.5) / np.repeat(sizes, sizes)
        cells = cells[np.argsort(pos, kind="stable")]
    else:
        assert layout == "runs"
    label = rng.permutation(nlist)
    cells = label[cells]
    where = np.sort(rng.integers(0, cells.size + 1, 40))
    cells = np.insert(cells, where, np.resize(np.array(OUT_OF_RANGE(nlist), np.int64), 40))
    by_label = np.zeros(nlist, np.int64)
    by_label[label] = sizes
    out = cells.astype(np.int32)
    out.setflags(write=False)
    return out, by_label


def random_assign(n, nlist, seed, bad_every=97):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, nlist, n).astype(np.int64)
    bad = np.array(OUT_OF_RANGE(nlist), np.int64)
    idx = np.arange(0, n, bad_every)[1:]
    a[idx] = np.resize(bad, idx.size)
    return a.astype(np.int32)


# -------------------------------------------------------------------------------------------------------- 3. probes: reference
PROBE_NLIST = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 5000, 16384)


def probe_counts(nlist):
    return sorted({1, min(2, nlist), nlist // 3 + 1, max(nlist - 1, 1), nlist})


def order_key(s):
    """The documented order as an unsigned key: the numbers' order, -0.0 == +0.0, a NaN by its bits."""
    bits = np.ascontiguousarray(s, F32).view(np.uint32)
    bits = np.where((bits & np.uint32(0x7FFFFFFF)) == 0, np.uint32(0), bits)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def probes_ref(s, nprobe):
    """s fp32 [nlist] -> ascending int32 [nprobe]."""
    key = order_key(s).astype(np.int64)
    order = np.lexsort((np.arange(s.size), -key))            # key descending, cell ascending
    return np.sort(order[:nprobe]).astype(np.int32)


def _from_bits(bits):
    return np.asarray(bits, np.uint32).view(F32)


def score_families(nlist, seed=0):
    """name -> fp32 [nlist]."""
    rng = np.random.default_rng(4000 + 7 * nlist + seed)
    fam = {}
    fam["equal"] = np.full(nlist, 0.5, F32)
    two = np.full(nlist, 0.25, F32)
    two[rng.permutation(nlist)[:nlist // 2]] = 1.0
    fam["two"] = two
    fam["ramp_up"] = (np.arange(nlist) - nlist // 2).astype(F32)
    fam["ramp_down"] = fam["ramp_up"][::-1].copy()
    low = (np.uint32(0x40490F00) | rng.integers(0, 256, nlist).astype(np.uint32)).astype(np.uint32)
    fam["low_byte"] = _from_bits(low)
    fam["low_byte_signed"] = _from_bits(low | (rng.integers(0, 2, nlist).astype(np.uint32) << np.uint32(31)))
    inf = rng.standard_normal(nlist).astype(F32)
    a, b = nlist // 5, nlist // 3
    inf[a:a + nlist // 4] = np.inf
    inf[nlist - b:] = -np.inf
    inf[::7] = np.where(np.arange(nlist)[::7] % 2 == 0, np.inf, -np.inf)
    fam["inf_blocks"] = inf
    den = rng.integers(1, 0x800000, nlist).astype(np.uint32) | (rng.integers(0, 2, nlist).astype(np.uint32) << np.uint32(31))
    den[rng.permutation(nlist)[:nlist // 6]] = 0
    fam["denormal"] = _from_bits(den)
    z = rng.standard_normal(nlist).astype(F32)
    zi = rng.permutation(nlist)[:max(nlist // 2, min(nlist, 2))]
    z[zi] = np.where(rng.integers(0, 2, zi.size) == 0, F32(0.0), F32(-0.0))
    if nlist >= 2:                                             # always a -0.0 in a lower cell than a +0.0
        z[zi.min()], z[zi.max()] = F32(-0.0), F32(0.0)
    fam["zeros"] = z
    fam["zeros_only"] = np.where(rng.integers(0, 2, nlist) == 0, F32(0.0), F32(-0.0)).astype(F32)
    return fam


def nan_scores(nlist, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(nlist).astype(F32)
    idx = rng.permutation(nlist)
    k = max(nlist // 10, 2)
    bits = s.view(np.uint32).copy()
    bits[idx[:k]] = 0x7FC00000                                 # quiet NaN, sign clear: above +inf
    bits[idx[k:2 * k]] = 0xFFC00000                            # quiet NaN, sign set: below -inf
    bits[idx[2 * k:3 * k]] = 0x7F800000
    bits[idx[3 * k:4 * k]] = 0xFF800000
    return bits.view(F32), k


def check_selection(out, nlist, nprobe):
    out = np.asarray(out)
    assert out.dtype == np.int32 and out.shape[-1] == nprobe
    assert (out >= 0).all() and (out < nlist).all()
    assert (np.diff(out.astype(np.int64), axis=-1) > 0).all()            # ascending and distinct


# ------------------------------------------------------------------------------------------------- 4. k-means: reference
KM_N, KM_D, KM_NLIST, KM_SEED = 3000, 16, 40, 77
KM_DUP = ((0, 1), (7, 20), (38, 39))                                     # init cell `upper` duplicates init cell `lower`
KM_FAR = (4, 5)                                                          # ... and this pair sits far from everything else


@functools.lru_cache(maxsize=None)
def kmeans_data():
    x = ints_data((KM_N, KM_D), 5000, lim=8)
    perm = np.random.default_rng(KM_SEED).permutation(KM_N)[:KM_NLIST]
    for lo, hi in KM_DUP:
        x[perm[hi]] = x[perm[lo]]
    x[perm[KM_FAR[0]]] = 100.0
    x[perm[KM_FAR[1]]] = 100.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def kmeans_ref(iters):
    """-> (cent after `iters` iterations, [(cent before, assign, counts)] per iteration)."""
    x = kmeans_data()
    cent = x[np.random.default_rng(KM_SEED).permutation(KM_N)[:KM_NLIST]].copy()
    hist = []
    for it in range(iters):
        a = cell_ref(score_ref(x, cent))
        new, cnt = update_ref(x, a, KM_NLIST, KM_SEED, it)
        hist.append((cent, a, cnt))
        cent = new
    return cent, hist


def objective(x, cent, a):
    d = x.astype(F64) - cent.astype(F64)[a]
    return float((d * d).sum())


# ============================================================================================================ CPU tests
def test_fma32_matches_the_c_library_on_non_finite_operands():
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.fmaf.argtypes = [C.c_float] * 3
    libm.fmaf.restype = C.c_float
    vals = np.array([0.0, -0.0, 1.0, -2.5, 3e38, -3e38, 1e38, 1.5e19, np.inf, -np.inf, np.nan, 1e-30], F32)
    a, b, c = (g.ravel() for g in np.meshgrid(vals, vals, vals, indexing="ij"))
    got = fma32(a, b, c)
    want = np.array([libm.fmaf(float(p), float(q), float(r)) for p, q, r in zip(a, b, c)], F32)
    both_nan = np.isnan(got) & np.isnan(want)                             # a NaN's payload and sign are not pinned
    assert (both_nan | (got.view(np.uint32) == want.view(np.uint32))).all()


def test_ints_family_is_exact_in_every_order():
    """The largest |value| of the family bounds every intermediate below 2^24, and the chain restatement of a small case has the
    bits of the fp64 scores - so at the sizes the restatement cannot afford, the fp64 argmin is the reference."""
    for D in INTS_D:
        x, cent, S = sweep_case("ints", D)
        assert np.abs(x).max() <= 8 and np.abs(cent).max() <= 8 and (x == np.rint(x)).all() and (cent == np.rint(cent)).all()
        assert 3 * 64 * D < 2 ** 24                                       # |cnorm| + 2 |acc| <= 192 D
        assert (S == np.rint(S)).all() and np.abs(S).max() < 2 ** 24
    x, cent, S = sweep_case("ints", 48)
    chain = score_ref(x[:60], cent[:70])
    assert np.array_equal(chain.astype(F64), S[:60, :70])
    assert np.array_equal(cnorm_ref(cent).astype(F64), (cent.astype(F64) ** 2).sum(1))
    assert np.array_equal(cell_ref(chain), S[:60, :70].argmin(1))
    x, cent, _ = sweep_case("ints", 1024)                                  # cnorm at 16 chain steps per lane
    assert np.array_equal(cnorm_ref(cent[:9]).astype(F64), (cent[:9].astype(F64) ** 2).sum(1))


def test_gauss_family_has_no_subnormal_product_and_its_one_ulp_pairs_are_one_ulp_apart():
    for D in GAUSS_D:
        x, cent, S = sweep_case("gauss", D)
        for a in (x, cent):
            assert np.isfinite(a).all() and np.abs(a).min() >= 2.0 ** -20 and np.abs(a).max() <= 2.0 ** 6
        # products in [2^-40, 2^12]; every partial sum is a multiple of 2^-20 2^-20 2^-23: zero or normal (>= 2^-63 > 2^-126)
        assert np.isfinite(S).all()
        c2 = FAMILY["gauss"]((max(ASSIGN_NLIST), D), 200 + D)
        for lo, hi, j in one_ulp_pairs(c2, 300 + D):
            diff = np.nonzero(cent[lo].view(np.uint32) != cent[hi].view(np.uint32))[0]
            assert diff.tolist() == [j]
            assert abs(int(cent[lo, j].view(np.uint32)) - int(cent[hi, j].view(np.uint32))) == 1
        assert np.array_equal(c2.view(np.uint32), cent.view(np.uint32))
        # the acc restatement is the fmaf chain of test_dense_flat.py
        bi, ci = np.meshgrid(np.arange(20), np.arange(30), indexing="ij")
        assert np.array_equal(acc_ref(x[:20], cent[:30]).view(np.uint32),
                              chain_scores(x[bi.ravel()], cent[ci.ravel()]).reshape(20, 30).view(np.uint32))


@pytest.mark.parametrize("family", ["ints", "gauss"])
def test_tie_pairs_sit_at_the_stated_distances(family):
    assert [hi - lo for lo, hi in TIE_PAIRS[:-1]] == [1, 4, 4, 8, 32, 64, 128, 129]
    lo, hi = TIE_PAIRS[-1]
    assert hi == TIE_NLIST - 1 and TIE_NLIST % 128 != 0 and lo // 128 != hi // 128     # last valid cell of a ragged list tile
    flat = [c for p in TIE_PAIRS for c in p]
    assert len(set(flat)) == len(flat)
    # one pair per structural boundary: slot r = (c % 32) bits; 4 half = bit 2; r >> 2 = bits 3-4; a = bit 5; wr = bit 6; tile
    assert [lo ^ hi for lo, hi in TIE_PAIRS[:6]] == [1, 4, 12, 8, 32, 64]      # all but (20, 24) cross exactly ONE of them
    assert (48 >> 2) & 1 == 0 and (20 >> 2) & 1 == 1 and (127 >> 6) & 1 == 1 and (256 >> 6) & 1 == 0
    for D in (16, 64) if family == "gauss" else (16, 768):
        for mirror in (False, True):
            x, cent, rows = tie_case(family, D, mirror)
            assert len(rows) >= 9 * 23 and {r % 128 // 32 for r, _, _ in rows} == {0, 1, 2, 3} and any(r >= 256 for r, _, _ in rows)
            S = ints_scores(x, cent) if family == "ints" else score_ref(x, cent)
            want = S.argmin(1) if family == "ints" else cell_ref(S)
            for r, lo, hi in rows:
                assert np.array_equal(x[r].view(np.uint32), cent[hi].view(np.uint32))
                ndiff = int((cent[lo].view(np.uint32) != cent[hi].view(np.uint32)).sum())
                assert ndiff == (1 if mirror else 0)
                if not mirror:
                    assert want[r] == lo and S[r, lo] == S[r, hi]         # an exact tie, and it is the minimum
                elif family == "ints":
                    assert want[r] == hi and S[r, lo] - S[r, hi] == 1.0   # the smallest step: squared distance 1 against 0
                else:
                    assert want[r] == hi and S[r, hi] < S[r, lo]


def test_the_derived_bound_holds_for_the_restatement():
    for D in GAUSS_D:
        x, cent, S = sweep_case("gauss", D)
        exact = ints_scores(x, cent)                                       # fp64 ||c||^2 - 2 <x, c> (not integers here)
        e = err_bound(x, cent)
        assert (np.abs(S.astype(F64) - exact) <= e).all()
        g = cell_ref(S)
        b = exact.argmin(1)
        r = np.arange(x.shape[0])
        assert (exact[r, g] <= exact[r, b] + e[r, g] + e[r, b]).all()


def test_reference_rules_for_nan_and_infinite_scores():
    S = np.array([[np.nan, 5, 3, 3], [np.inf, np.inf, np.inf, np.inf], [np.nan, np.inf, np.nan, np.inf],
                  [np.inf, -np.inf, -np.inf, 0], [np.nan, np.nan, np.nan, np.nan], [np.inf, np.nan, 7, np.nan]], F32)
    assert cell_ref(S).tolist() == [2, 0, 0, 1, 0, 2]
    for D in GAUSS_D:
        x, cent = nonfinite_case(D)
        S = score_ref(x, cent)
        want = cell_ref(S)
        with np.errstate(all="ignore"):
            prod = x[12].astype(F64)[None, :] * cent.astype(F64)
            sq = cent[30].astype(F64) ** 2
        assert np.abs(prod[20]).max() < 3.4028234e38                       # 3e38: every product of (row 12, cell 20) is finite
        assert np.isinf(acc_ref(x[12:13], cent[20:21])).all()              # ... finite products, infinite sum
        assert sq.max() < 3.4028234e38 and np.isinf(cnorm_ref(cent[30:31])).all()
        assert np.isnan(S[3]).all() and want[3] == 0
        assert np.isnan(S[:, 7]).all() and np.isnan(S[:, 131]).all()
        assert not np.isin(want, (7, 30, 131)).any()
        plain = np.setdiff1d(np.arange(70), (3, 10, 11, 12))
        keep = np.setdiff1d(np.arange(140), (7, 131))
        assert np.isfinite(S[np.ix_(plain, np.setdiff1d(keep, (30,)))]).all()
        # the other rows are unaffected: their cell is the first minimum over the centroids that hold no NaN
        assert np.array_equal(want[plain], keep[cell_ref(score_ref(x[plain], cent[keep]))])


def test_splitmix_restatement_and_sweep_layouts():
    # splitmix64 test vectors (state 0 and 1 advanced once: the published first outputs of the generator)
    assert splitmix64(0) == 0xE220A8397B1DCDAF and splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert empty_row(2 ** 63 + 5, 3, 9, 20011) == splitmix64((2 ** 63 + 5) ^ splitmix64((3 << 32) | 9)) % 20011
    for layout in ("round_robin", "runs"):
        a, sizes = sweep_assign(layout)
        nlist = len(SWEEP_SIZES)
        ok = (a >= 0) & (a < nlist)
        assert (~ok).sum() == 40 and set(a[~ok].tolist()) == set(OUT_OF_RANGE(nlist))
        assert np.array_equal(np.bincount(a[ok], minlength=nlist), sizes) and sorted(sizes.tolist()) == sorted(SWEEP_SIZES)
        assert sizes.max() <= 5000
        tiles = -(-a.size // 2048)
        for c in np.nonzero(sizes >= 2047)[0]:
            rows = np.nonzero(a == c)[0]
            spanned = np.unique(rows // 2048).size
            if layout == "round_robin":
                assert spanned == tiles                                    # every large cell has rows in every tile
            else:
                assert rows[-1] - rows[0] <= rows.size + 40 and spanned >= 2      # one run, across a tile edge


def test_update_reference_orders_agree_on_integers():
    a, sizes = sweep_assign("runs")
    x = ints_data((a.size, 4), 32, lim=1024)
    cent, cnt = update_ref(x, a, len(SWEEP_SIZES), 9, 0)
    assert np.array_equal(cnt, sizes)
    assert np.array_equal(cent.view(np.uint32), update_ref_lanes(x, a, len(SWEEP_SIZES), 9, 0).view(np.uint32))


def test_score_families_are_what_they_claim():
    for nlist in (65, 1025):
        fam = score_families(nlist)
        key = {k: order_key(v) for k, v in fam.items()}
        assert np.unique(key["equal"]).size == 1 and np.unique(key["two"]).size == 2
        assert (np.diff(key["ramp_up"].astype(np.int64)) > 0).all() and (np.diff(key["ramp_down"].astype(np.int64)) < 0).all()
        assert np.unique(key["low_byte"] >> 8).size == 1 and np.unique(key["low_byte"]).size > 1
        assert np.array_equal(np.abs(fam["low_byte_signed"]), fam["low_byte"]) and (fam["low_byte_signed"] < 0).any()
        assert np.isposinf(fam["inf_blocks"]).sum() > 2 and np.isneginf(fam["inf_blocks"]).sum() > 2
        d = fam["denormal"]
        assert (np.abs(d) < 2.0 ** -126).all() and (d != 0).sum() > nlist // 2 and (d > 0).any() and (d < 0).any()
        for name in ("zeros", "zeros_only"):
            z = fam[name]
            neg0 = np.nonzero((z == 0) & np.signbit(z))[0]
            pos0 = np.nonzero((z == 0) & ~np.signbit(z))[0]
            assert neg0.size and pos0.size and neg0.min() < pos0.max()
            assert np.unique(order_key(z[z == 0])).size == 1                # the documented key: the two zeros tie
        # the reference is the stable descending sort of the numbers wherever no NaN is involved
        for name, s in fam.items():
            for nprobe in probe_counts(nlist):
                want = np.sort(np.argsort(-s.astype(F64), kind="stable")[:nprobe])
                assert np.array_equal(probes_ref(s, nprobe), want), (name, nprobe)
    s, k = nan_scores(300, 1)
    top = probes_ref(s, k)
    assert (s.view(np.uint32)[top] == 0x7FC00000).all()                    # NaN, sign clear: the best k
    rest = probes_ref(s, 300 - k)
    assert not (s.view(np.uint32)[rest] == 0xFFC00000).any()               # NaN, sign set: the worst k


def test_kmeans_reference_meets_the_empty_rule_and_the_objective_does_not_increase():
    x = kmeans_data()
    assert (x == np.rint(x)).all() and np.abs(x).max() <= 1024
    cent, hist = kmeans_ref(4)
    c0, a0, cnt0 = hist[0]
    empties = set(np.nonzero(cnt0 == 0)[0].tolist())
    assert empties == {hi for _, hi in KM_DUP} | {KM_FAR[1]}               # the planted duplicates, nothing else
    assert cnt0[KM_FAR[0]] == 2
    for c in empties:                                                      # ... and the rule gives them rows of x
        assert np.array_equal(hist[1][0][c], x[empty_row(KM_SEED, 0, c, KM_N)])
    checked = 0
    for t in range(len(hist) - 1):
        if (hist[t][2] == 0).any():
            continue
        c_new, a_new, _ = hist[t + 1]
        e = err_bound(x, c_new)
        r = np.arange(KM_N)
        slack = float((e[r, a_new] + e[r, hist[t][1]]).sum()) + KM_N * KM_D * (U * float(np.abs(c_new).max())) ** 2
        assert objective(x, c_new, a_new) <= objective(x, hist[t][0], hist[t][1]) + slack
        checked += 1
    assert checked >= 2


# ============================================================================================================ GPU helpers
def _t(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)            # a copy: the cached cases are read-only


def _ctx():
    from repconc_amd import _lib
    lib, h = _lib.load(), _lib.handle(0)
    return lib, h, C.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def _p(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def raw_assign(x_t, ldx, cent_t, B, D, nlist, x_off=0, cent_off=0):
    """The C entry as it is: -> (return code, cells int32 [B] pre-filled with -7)."""
    lib, h, s = _ctx()
    wsb = lib.rc_ivf_coarse_assign_ws_bytes(nlist)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=DEV)
    out = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    rc = lib.rc_ivf_coarse_assign(h, _p(x_t, x_off), ldx, _p(cent_t, cent_off), B, D, nlist, _p(out), _p(ws), wsb, s)
    return rc, out.cpu().numpy()


def gpu_update(x_t, assign, nlist, seed, it, counts=True):
    """rc_ivf_coarse_update on x_t (any row stride) -> (cent fp32 [nlist, D] pre-filled with NaN, counts or None)."""
    from repconc_amd import _lib
    lib, h, s = _ctx()
    n, D = x_t.shape
    a_t = _t(np.asarray(assign, np.int32))
    wsb = lib.rc_ivf_coarse_update_ws_bytes(n, nlist)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=DEV)
    cent = torch.full((nlist, D), float("nan"), dtype=torch.float32, device=DEV)
    cnt = torch.full((nlist,), -1, dtype=torch.int32, device=DEV) if counts else None
    _lib.check(lib.rc_ivf_coarse_update(h, _p(x_t), x_t.stride(0), _p(a_t), n, D, nlist, _p(cent), _p(cnt) if counts else None,
                                        seed, it, _p(ws), wsb, s), "rc_ivf_coarse_update", h)
    return cent.cpu().numpy(), (cnt.cpu().numpy() if counts else None)


def padded(a, pad=4):
    """Device [n, D] view with row stride D + pad; the padding holds NaN."""
    big = np.full((a.shape[0], a.shape[1] + pad), np.nan, F32)
    big[:, :a.shape[1]] = a
    v = _t(big)[:, :a.shape[1]]
    assert v.stride(0) == a.shape[1] + pad
    return v


def assert_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad[0].size == 0, f"{what}: {bad[0].size} entries differ, first at {[int(b[0]) for b in bad]}: " \
                             f"{got[tuple(b[0] for b in bad)]!r} vs {want[tuple(b[0] for b in bad)]!r}"


def assert_cells(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first row {bad[0]}: cell {got[bad[0]]} vs {want[bad[0]]}"


# ====================================================================================================== 1. assignment, GPU
@gpu
@pytest.mark.parametrize("family,D", [("ints", D) for D in INTS_D] + [("gauss", D) for D in GAUSS_D])
def test_assign_is_the_first_minimum_at_every_B_and_nlist(family, D):
    from repconc_amd.ivf import coarse_assign
    x, cent, S = sweep_case(family, D)
    x_t, c_t = _t(x), _t(cent)
    for nlist in ASSIGN_NLIST:
        want = S[:, :nlist].argmin(1) if family == "ints" else cell_ref(S[:, :nlist])
        for B in ASSIGN_B:
            got = coarse_assign(x_t[:B], c_t[:nlist])
            assert got.dtype == torch.int64
            assert_cells(got.cpu().numpy(), want[:B], (family, D, B, nlist))


@gpu
@pytest.mark.parametrize("family,D", [("ints", 48), ("ints", 768), ("gauss", 16), ("gauss", 64)])
def test_assign_with_padded_rows_through_the_view_and_the_raw_entry(family, D):
    from repconc_amd.ivf import coarse_assign
    x, cent, S = sweep_case(family, D)
    want = S.argmin(1) if family == "ints" else cell_ref(S)
    x_v, c_t = padded(x), _t(cent)
    assert_cells(coarse_assign(x_v, c_t).cpu().numpy(), want, "view")
    for B in (129, 257):
        rc, got = raw_assign(x_v, D + 4, c_t, B, D, cent.shape[0])
        assert rc == 0
        assert_cells(got, want[:B], ("raw", B))


@gpu
@pytest.mark.parametrize("family,D,nlist", [("ints", 16, 300), ("ints", 768, 257), ("ints", 1024, 128), ("ints", 32, 129),
                                            ("gauss", 16, 300), ("gauss", 64, 257)])
def test_every_centroid_wins_somewhere(family, D, nlist):
    from repconc_amd.ivf import coarse_assign
    cent = FAMILY[family]((nlist, D), 1000 + D + nlist)
    assert np.unique(cent, axis=0).shape[0] == nlist
    perm = np.random.default_rng(1).permutation(nlist)
    x = cent[perm]
    if family == "gauss":                                                  # the restatement agrees that each row is its own cell
        assert np.array_equal(cell_ref(score_ref(x, cent)), perm)
    got = coarse_assign(_t(x), _t(cent)).cpu().numpy()
    assert_cells(got, perm, (family, D, nlist))
    assert np.array_equal(np.sort(got), np.arange(nlist))


@gpu
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("family,D", [("ints", 16), ("ints", 768), ("gauss", 16), ("gauss", 64)])
def test_exact_ties_across_every_structural_boundary(family, D, mirror):
    from repconc_amd.ivf import coarse_assign
    x, cent, rows = tie_case(family, D, mirror)
    want = ints_ref(x, cent) if family == "ints" else cell_ref(score_ref(x, cent))
    got = coarse_assign(_t(x), _t(cent)).cpu().numpy()
    for r, lo, hi in rows:
        assert got[r] == (hi if mirror else lo), (family, D, mirror, r, lo, hi, int(got[r]))
    assert_cells(got, want, (family, D, mirror))


@gpu
@pytest.mark.parametrize("D", GAUSS_D)
def test_assign_on_non_finite_rows_and_centroids(D):
    from repconc_amd.ivf import coarse_assign
    x, cent = nonfinite_case(D)
    want = cell_ref(score_ref(x, cent))
    got = coarse_assign(_t(x), _t(cent)).cpu().numpy()
    assert not np.isin(got, (7, 30, 131)).any()
    assert got[3] == 0
    assert_cells(got, want, D)


@gpu
def test_assign_fallback_for_other_widths_keeps_the_first_minimum():
    from repconc_amd.ivf import coarse_assign
    D = 24
    x, cent, rows = tie_case("ints", D, False)
    got = coarse_assign(_t(x), _t(cent)).cpu().numpy()
    assert_cells(got, ints_ref(x, cent), "D = 24")
    for r, lo, hi in rows:
        assert got[r] == lo


@gpu
def test_assigned_cell_is_the_fp64_minimum_up_to_the_derived_bound():
    from repconc_amd.ivf import coarse_assign
    D = 768
    rng = np.random.default_rng(9)
    for B, nlist in ((257, 300), (1000, 129)):
        x = rng.standard_normal((B, D)).astype(F32)
        cent = rng.standard_normal((nlist, D)).astype(F32)
        x[:5] = cent[3] + 1e-3 * rng.standard_normal((5, D)).astype(F32)
        # near-duplicate centroids with documents beside them: fp64 gaps of about 1e-5 under a score whose ulp is 6e-5, so the
        # fp32 choice does differ from the fp64 argmin and the bound is what holds it
        for k in range(20, 60):
            cent[2 * k + 1] = cent[2 * k] + F32(1e-5) * rng.standard_normal(D).astype(F32)
            x[k] = cent[2 * k] + F32(1e-3) * rng.standard_normal(D).astype(F32)
        got = coarse_assign(_t(x), _t(cent)).cpu().numpy()
        exact, e = ints_scores(x, cent), err_bound(x, cent)
        b, r = exact.argmin(1), np.arange(B)
        excess = exact[r, got] - exact[r, b]
        print(f"B {B} nlist {nlist}: worst excess / bound {float((excess / (e[r, got] + e[r, b])).max()):.3g}, "
              f"agreement with the fp64 argmin {float((got == b).mean()):.4f}")
        assert (excess <= e[r, got] + e[r, b]).all()


@gpu
def test_assign_refuses_misaligned_pointers_before_any_launch():
    x, cent, _ = sweep_case("ints", 16)
    x_t, c_t = _t(np.concatenate([x, x[:1]])), _t(np.concatenate([cent, cent[:1]]))      # one spare row behind the offset
    rc, out = raw_assign(x_t, 16, c_t, 64, 16, 100)
    assert rc == 0 and (out >= 0).all()
    for x_off, c_off in ((4, 0), (0, 4), (8, 0), (0, 12)):
        rc, out = raw_assign(x_t, 16, c_t, 64, 16, 100, x_off, c_off)
        assert rc == RC_ESHAPE and (out == -7).all(), (x_off, c_off, rc)


# ========================================================================================================== 2. update, GPU
@gpu
@pytest.mark.parametrize("layout", ["round_robin", "runs"])
@pytest.mark.parametrize("D", [4, 16, 768, 1024])
def test_update_on_every_cell_size(D, layout):
    a, sizes = sweep_assign(layout)
    nlist = len(SWEEP_SIZES)
    x = ints_data((a.size, D), 40 + D, lim=1024)
    want, wcnt = update_ref(x, a, nlist, 2 ** 63 + 1234, 5)
    got, gcnt = gpu_update(_t(x), a, nlist, 2 ** 63 + 1234, 5)
    assert np.array_equal(gcnt, wcnt) and np.array_equal(wcnt, sizes)
    assert_bits(got, want, (D, layout))


GEOMETRY = [  # n, nlist, D, padded rows, counts_out
    (1, 1, 4, False, True), (1, 257, 16, False, True), (2047, 255, 16, False, False), (2048, 256, 4, True, True),
    (2049, 257, 768, True, True), (2049, 1, 1024, False, True), (20011, 700, 1024, False, False),
    (20011, 16384, 16, False, True), (2049, 16384, 4, True, False), (20011, 256, 768, True, True),
    (2048, 700, 16, False, True),
]


@gpu
@pytest.mark.parametrize("n,nlist,D,pad,counts", GEOMETRY)
def test_update_geometry(n, nlist, D, pad, counts):
    x = ints_data((n, D), 50 + n % 100 + nlist + D, lim=1024)
    a = random_assign(n, nlist, 60 + n % 100 + nlist)
    seed, it = (2 ** 64 - 1, 0) if nlist % 2 else (987654321, 11)
    want, wcnt = update_ref(x, a, nlist, seed, it)
    x_t = padded(x) if pad else _t(x)
    got, gcnt = gpu_update(x_t, a, nlist, seed, it, counts)
    if counts:
        assert np.array_equal(gcnt, wcnt)
    assert wcnt.max() <= 5000
    assert_bits(got, want, (n, nlist, D))


@gpu
@pytest.mark.parametrize("seed,it,n", [(1234, 0, 2049), (2 ** 63 + 12345, 3, 20011), (2 ** 64 - 1, 7, 3000), (0, 0, 1),
                                       (5, 2 ** 31 - 1, 4097)])
def test_update_with_every_assignment_out_of_range_takes_the_promised_rows(seed, it, n):
    nlist, D = 257, 16
    x = ints_data((n, D), 70 + n % 50, lim=1024) + np.arange(n, dtype=F32)[:, None] * F32(4096)     # every row different
    a = np.resize(np.array(OUT_OF_RANGE(nlist), np.int64), n).astype(np.int32)
    got, gcnt = gpu_update(_t(x), a, nlist, seed, it)
    assert (gcnt == 0).all()
    rows = [empty_row(seed, it, c, n) for c in range(nlist)]
    assert n == 1 or len(set(rows)) > 1
    assert_bits(got, x[rows], (seed, it, n))


@gpu
@pytest.mark.parametrize("layout", ["round_robin", "runs"])
def test_update_gaussian_is_the_four_lane_order_on_every_cell_and_repeats(layout):
    a, sizes = sweep_assign(layout)
    nlist, D = len(SWEEP_SIZES), 16
    x = np.random.default_rng(80).standard_normal((a.size, D)).astype(F32)
    want = update_ref_lanes(x, a, nlist, 4321, 1)
    x_t = padded(x)
    got, gcnt = gpu_update(x_t, a, nlist, 4321, 1)
    again, _ = gpu_update(x_t, a, nlist, 4321, 1)
    assert np.array_equal(gcnt, sizes)
    assert_bits(got, want, layout)
    assert_bits(again, got, "second call")


# ========================================================================================================== 3. probes, GPU
def raw_probes(s_t, nlist, nprobe):
    lib, h, s = _ctx()
    nq = s_t.shape[0]
    out = torch.full((nq, nprobe), -7, dtype=torch.int32, device=DEV)
    rc = lib.rc_ivf_select_probes(h, _p(s_t), nq, nlist, nprobe, _p(out), s)
    assert rc == 0
    return out.cpu().numpy()


@gpu
@pytest.mark.parametrize("nlist", PROBE_NLIST)
def test_probe_selection_on_every_family(nlist):
    from repconc_amd.ivf import IVFPQIndex
    fam = score_families(nlist)
    names = sorted(fam)
    S = np.stack([fam[k] for k in names])
    s_t = _t(S)
    ivf = IVFPQIndex(16, 16, nlist, device=DEV)
    one = torch.ones((1, 1), dtype=torch.float32, device=DEV)
    for nprobe in probe_counts(nlist):
        got = raw_probes(s_t, nlist, nprobe)
        check_selection(got, nlist, nprobe)
        for i, name in enumerate(names):
            assert np.array_equal(got[i], probes_ref(S[i], nprobe)), (name, nlist, nprobe)
            ivf.coarse = s_t[i].reshape(nlist, 1).contiguous()
            ranked = ivf.probe(one, nprobe, ordered=True).cpu().numpy()
            plain = ivf.probe(one, nprobe, ordered=False).cpu().numpy()
            assert ranked.dtype == np.int32 and ranked.shape == (1, nprobe)
            assert np.array_equal(np.sort(ranked[0]), plain[0]), (name, nlist, nprobe)
            if name != "denormal":            # a library GEMM may flush denormals: there the two paths are only compared
                assert np.array_equal(plain[0], got[i]), (name, nlist, nprobe)


@gpu
@pytest.mark.parametrize("nlist", [300, 1025])
def test_probe_selection_orders_nan_by_its_bits_and_stays_a_selection(nlist):
    s, k = nan_scores(nlist, nlist)
    s_t = _t(s[None, :])
    for nprobe in (1, k - 1, k, k + 3, nlist - k, nlist - k + 1, nlist - 1, nlist):
        got = raw_probes(s_t, nlist, nprobe)
        check_selection(got, nlist, nprobe)
        assert np.array_equal(got[0], probes_ref(s, nprobe)), (nlist, nprobe)
    all_nan = _t(np.full((2, nlist), np.nan, F32))
    for nprobe in (1, 7, nlist):
        got = raw_probes(all_nan, nlist, nprobe)
        check_selection(got, nlist, nprobe)
        assert np.array_equal(got[0], np.arange(nprobe))                   # all tied: the lowest cells


# ============================================================================================== 4. the pieces together, GPU
@gpu
@pytest.mark.parametrize("iters", [0, 1, 3])
def test_coarse_kmeans_is_the_numpy_loop_bit_for_bit(iters):
    from repconc_amd.ivf import coarse_assign, coarse_kmeans
    x = kmeans_data()
    want, hist = kmeans_ref(iters)
    got = coarse_kmeans(_t(x), KM_NLIST, iters, seed=KM_SEED)
    assert got.shape == (KM_NLIST, KM_D) and got.dtype == torch.float32
    assert_bits(got.cpu().numpy(), want, iters)
    if iters:
        assert (hist[0][2] == 0).sum() == 4                               # the empty-cell rule fired at iteration 0
        assert_cells(coarse_assign(_t(x), _t(hist[-1][0])).cpu().numpy(), hist[-1][1], "last assignment")
    assert torch.equal(got, coarse_kmeans(_t(x), KM_NLIST, iters, seed=KM_SEED))


@functools.lru_cache(maxsize=None)
def lists_case():
    """N = 3001 rows in 12 cells, cells 0, 5, 6 and 11 empty; integer embeddings whose cell (by the coarse centroids) is the
    same assignment."""
    N, D, nlist = 3001, 768, 12
    rng = np.random.default_rng(90)
    live = np.array([1, 2, 3, 4, 7, 8, 9, 10])
    cent = ints_data((nlist, D), 91, lim=2)
    cent[[0, 5, 6, 11]] = 8.0                                             # far from every row: never the nearest
    cells = live[rng.integers(0, live.size, N)]
    x = (cent[cells] + rng.integers(-1, 2, (N, D))).astype(F32)
    codes = rng.integers(0, 256, (N, 48), dtype=np.uint8)
    return x, cent, codes


@gpu
def test_set_lists_and_add_keep_corpus_order_and_empty_cells():
    from repconc_amd.index import PQIndex
    from repconc_amd.ivf import IVFPQIndex
    x, cent, codes = lists_case()
    N, nlist, M = x.shape[0], cent.shape[0], codes.shape[1]
    cells = ints_ref(x, cent).astype(np.int64)
    cnt = np.bincount(cells, minlength=nlist)
    assert (cnt[[0, 5, 6, 11]] == 0).all() and (cnt[[1, 2, 3, 4, 7, 8, 9, 10]] > 0).all()
    pq = np.random.default_rng(92).standard_normal((M, 256, 768 // M)).astype(F32)
    q = np.random.default_rng(93).standard_normal((6, 768)).astype(F32)
    flat = PQIndex(768, M, device=DEV)
    flat.set_centroids(pq)
    flat.add_codes(_t(codes))
    for how in ("set_lists", "add"):
        ivf = IVFPQIndex(768, M, nlist, device=DEV)
        ivf.set_centroids(pq)
        ivf.coarse = _t(cent)
        if how == "set_lists":
            ivf.set_lists(_t(codes), _t(cells))
        else:
            ivf.add(_t(x), _t(codes))
        off, ids, stored = ivf.list_off.cpu().numpy(), ivf.ids.cpu().numpy(), ivf.codes.cpu().numpy()
        assert ivf.ntotal == N and off.dtype == np.int64 and ids.dtype == np.int64
        assert np.array_equal(off, np.concatenate([[0], np.cumsum(cnt)]))                 # the exclusive cumsum
        assert np.array_equal(ids, np.argsort(cells, kind="stable"))                      # the stable order
        for c in range(nlist):
            rows = np.nonzero(cells == c)[0]                                              # ascending: corpus order
            assert np.array_equal(ids[off[c]:off[c + 1]], rows), (how, c)
            assert np.array_equal(stored[off[c]:off[c + 1]], codes[rows]), (how, c)
        for k in (10, 200):
            fs, fi = flat.search(_t(q), k)
            for method in ("scan", "lists"):
                s, i = ivf.search(_t(q), k, nprobe=nlist, method=method)
                assert torch.equal(i, fi) and torch.equal(s, fs), (how, k, method)
