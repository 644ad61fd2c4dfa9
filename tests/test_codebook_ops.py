"""The training-side codebook kernels on codes and values built to strain them: decode and its gradient (decode_kernel,
decode_scalar_kernel, decode_bwd_kernel), centroid normalisation, the code histogram (csrc/pq_misc.hip), the k-means centroid
update and the k-means statistics under skew (csrc/kmeans.hip), through their ops.py wrappers.

Inputs (module-level generators, seeded, numpy on the CPU).
  Code families (n, M, rng) -> uint8 [n, M]:  uniform;  one_code (every entry 255: all n rows of a column in ONE bin, the worst
  case for the fp32 atomics, the LDS bins and the statistics);  two_hot (99 % of the rows 255, the rest 0, shuffled);
  column_const (column m holds m % 256);  cyclic (row r holds (r + 7 m) % 256: for n <= 256 no bin has two members);  pairs
  (n = 512, every bin exactly two members).
  Gradient families (n, D, rng) -> fp32 [n, D]:  gauss;  ints (integers in [-4, 4]: every partial sum is an integer of magnitude
  <= 4 n < 2^24, exact in fp32 in ANY order);  cancel (rows alternate +1e4 / -1e4 plus N(0, 1) noise: inside a bin that holds
  consecutive rows - one_code, two_hot, column_const - the large parts cancel);  wide (magnitudes 2^-20 .. 2^20).
  Shapes (M, dsub): five float4 widths, four widths of the one-float-per-thread decode (dsub % 4 != 0), two with D != 768.
  Row counts: 0, 1, 3, 255, 4097, 70001 on a short list, and the pair that straddles the grid cap: grid_for() launches at most
  num_cus * 8 blocks of 256 threads, so a kernel with one thread per element starts its grid-stride loop at
  n = floor(num_cus * 8 * 256 / D) + 1 (straddle(); the float4 decode at four times that), num_cus read from the handle.

The only tolerances of this file are bit equality and the two bounds below (u = 2^-24, the unit roundoff of fp32).

BOUND 1 (gradient of decode; bwd_bound).  A bin's gradient is the sum of its c members, added by fp32 atomics in an order nobody
controls.  A recursive sum of c terms in ANY order carries at most c - 1 roundings on each term, so
    |fl(sum) - sum| <= gamma(c - 1) * sum |g_i|,    gamma(t) = t u / (1 - t u)            (Higham, Accuracy and Stability, §4.2)
and the fp64 reference is rounded once more when it is compared in fp32: + u |want|.  Nothing here is measured; test 10 checks
on the CPU that four summation orders of the same data obey it.  Consequences that are tested bit for bit: a bin with one member
is that member, a bin with two is their fp32 sum (addition commutes; the fp64 sum of two fp32 values rounded to fp32 is the
fp32 sum, 53 >= 2 * 24 + 2), an empty bin is +0, and with `ints` the whole tensor is the integer sum.

BOUND 2 (normalise; norm_bound).  The kernel squares dsub values (one rounding each), adds them j-ascending (dsub - 1 adds: at
most dsub roundings on any term, all terms positive, so the sum's relative error is below dsub u), takes one square root (halves
the error, adds one rounding) and divides (one rounding).  (dsub + 4) u covers dsub / 2 + 2 with room for the reference's own
fp64 rounding and the second-order terms; it is RELATIVE per element, because the norm is a common factor.  The edge rows follow
torch.nn.functional.normalize in fp32 (the contract is F.normalize, not the mathematically unit vector).

k-means update: (float)(sum / (double)count) is one correctly rounded fp64 division and one correctly rounded conversion, so it
is compared bit for bit with numpy's, on quotients placed within one fp64 ulp of a fp32 rounding tie.  Only the BITS of a NaN
result are left open (IEEE 754 does not fix the payload a division returns): there NaN is required, nothing else.

What writing this file found, by reading the code, and what is fixed with it: (1) normalize_kernel clamped the norm with
fmaxf, which returns its other operand when one is NaN, so a row holding one NaN came back as x / 1e-12 with a single NaN in it;
F.normalize's clamp_min keeps the NaN and the whole row becomes NaN.  Fixed in the kernel.  (2) A zero-row tensor has a null
data pointer, which the C entry points reject with RC_EINVAL: ops.decode_raw, the backward, ops.code_hist and ops.kmeans_stats
raised on n = 0.  Fixed in the wrappers (nothing is launched for n = 0).  (3) the wrapper checks of test 12 and the copy of
a centroid view at an unaligned storage offset.  On the MI355X every assertion holds; the printed worst err / bound of the
gradient is 0.66 (Gaussian, one_code), 0.41 (cancel), 0.61 (wide), of the normalisation 0.36 at dsub = 3 falling to 0.02 at 768.
"""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import pq_oracle, synth

gpu = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
U = 2.0 ** -24                                           # unit roundoff of fp32

VEC_SHAPES = [(48, 16), (8, 96), (96, 8), (192, 4), (1, 768)]
SCALAR_SHAPES = [(128, 6), (256, 3), (384, 2), (768, 1)]          # decode_scalar_kernel
ODD_SHAPES = [(5, 7), (3, 20)]                                    # D = 35 (scalar), D = 60 (float4)
SHAPES = VEC_SHAPES + SCALAR_SHAPES + ODD_SHAPES
FULL_SHAPES = [(48, 16), (128, 6), (5, 7)]                        # every family, and 70001 rows
HIST_M = [1, 2, 3, 5, 6, 7, 8, 48, 50]
HIST_N = [0, 1, 255, 4095, 4096, 4097, 8193, 70001]
NORM_DSUB = [1, 3, 16, 96, 768]
UPDATE_COUNTS = (-3, 0, 1, 2, 3, 7, 2 ** 31 + 1)


# ------------------------------------------------------------------------------------------------------------ families
def _uniform(n, M, rng):
    return rng.integers(0, 256, size=(n, M), dtype=np.uint8)


def _one_code(n, M, rng):
    return np.full((n, M), 255, np.uint8)


def _two_hot(n, M, rng):
    rows = np.full(n, 255, np.uint8)
    rows[:n // 100] = 0
    rng.shuffle(rows)
    return np.repeat(rows[:, None], M, axis=1)


def _column_const(n, M, rng):
    return np.repeat((np.arange(M) % 256).astype(np.uint8)[None, :], n, axis=0)


def _cyclic(n, M, rng):
    return ((np.arange(n)[:, None] + 7 * np.arange(M)[None, :]) % 256).astype(np.uint8)


def _pairs(n, M, rng):
    assert n == 512
    return _cyclic(n, M, rng)[rng.permutation(n)]


CODE_FAMILIES = {"uniform": _uniform, "one_code": _one_code, "two_hot": _two_hot, "column_const": _column_const,
                 "cyclic": _cyclic, "pairs": _pairs}


def _gauss(n, D, rng):
    return rng.standard_normal((n, D), dtype=F32)


def _ints(n, D, rng):
    return rng.integers(-4, 5, size=(n, D)).astype(F32)


def _cancel(n, D, rng):
    big = np.where(np.arange(n) % 2 == 0, F32(1e4), F32(-1e4)).astype(F32)
    return (big[:, None] + rng.standard_normal((n, D), dtype=F32)).astype(F32)


def _wide(n, D, rng):
    mag = np.ldexp(1.0 + rng.random((n, D)), rng.integers(-20, 20, size=(n, D)))
    return (mag * rng.choice([-1.0, 1.0], size=(n, D))).astype(F32)


GRAD_FAMILIES = {"gauss": _gauss, "ints": _ints, "cancel": _cancel, "wide": _wide}


def codes_of(family, n, M, seed=0):
    return CODE_FAMILIES[family](n, M, np.random.default_rng(1000 + seed))


def grad_of(family, n, D, seed=0):
    return GRAD_FAMILIES[family](n, D, np.random.default_rng(2000 + seed))


def straddle(num_cus, D, per_thread=1):
    """(n, n + 1): the largest row count one pass of the capped grid covers, and the first that makes it loop."""
    n = num_cus * 8 * 256 * per_thread // D
    return n, n + 1


SPECIAL_BITS = [0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000, 0xFF800000,
                0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF]      # +-0, subnormals, extremes, infinities, quiet / signalling NaNs


def bit_table(M, dsub):
    """fp32 [M, 256, dsub] whose elements all have different bits (an odd multiplier is a bijection of the 32-bit words), NaN
    payloads, both zeros, subnormals and infinities among them: a decode that reads the wrong element cannot go unnoticed."""
    n = M * 256 * dsub
    bits = ((np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    bits[np.linspace(0, n - 1, len(SPECIAL_BITS)).astype(np.int64)] = np.array(SPECIAL_BITS, np.uint32)
    return bits.reshape(M, 256, dsub)


# ------------------------------------------------------------------------------------------------------------ references
def scatter64(codes, go, M):
    """(want, A, c): per (m, k, j) the fp64 sum of the gradient rows with code k, the sum of their absolute values, and the
    member count per (m, k).  torch index_add_ in fp64, on whatever device the arguments live."""
    n, D = go.shape
    dsub = D // M
    dev = go.device
    idx = ((codes.long() & 255) + 256 * torch.arange(M, device=dev)[None, :]).reshape(-1)
    g = go.double().reshape(n * M, dsub)
    want = torch.zeros((M * 256, dsub), dtype=torch.float64, device=dev).index_add_(0, idx, g)
    A = torch.zeros((M * 256, dsub), dtype=torch.float64, device=dev).index_add_(0, idx, g.abs())
    c = torch.bincount(idx, minlength=M * 256)
    return want.view(M, 256, dsub), A.view(M, 256, dsub), c.view(M, 256)


def bwd_bound(c, A, want):
    """BOUND 1 of the module docstring; c [M, 256], A and want [M, 256, dsub], fp64."""
    t = (c - 1).clamp_min(0).double()[..., None] * U
    return t / (1.0 - t) * A + U * want.abs()


def _bits(t):
    return t.contiguous().view(torch.int32)


def check_gradient(got, codes, go, M, exact):
    """The assertions of test 2 on one gradient; returns the worst err / bound."""
    want, A, c = scatter64(codes, go, M)
    assert got.dtype == torch.float32 and got.shape == want.shape
    err = (got.double() - want).abs()
    bound = bwd_bound(c, A, want)
    assert bool((err <= bound).all()), "gradient outside gamma(c - 1) A + u |want|: worst excess %g" % float((err - bound).max())
    w32 = want.float()
    small = (c <= 2)[..., None].expand_as(got)
    assert torch.equal(_bits(got)[small], _bits(w32)[small]), "a bin of <= 2 members is not the fp32 sum"
    empty = (c == 0)[..., None].expand_as(got)
    assert not bool(_bits(got)[empty].any()), "an empty bin is not +0"
    if exact:
        assert torch.equal(_bits(got), _bits(w32)), "integer gradient: not the exact sum"
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0


def norm_bound(dsub):
    """BOUND 2 of the module docstring (relative, per element)."""
    return (dsub + 4) * U


def _fsum_stats(x, codes, M):
    """sums[m, k, j] = the correctly rounded real sum (math.fsum) of the rows with code k — what exact integer parts give."""
    n, D = x.shape
    dsub = D // M
    out = np.zeros((M, 256, dsub))
    xd = x.astype(F64).reshape(n, M, dsub)
    for m in range(M):
        order = np.argsort(codes[:, m], kind="stable")
        ks, starts = np.unique(codes[order, m], return_index=True)
        ends = list(starts[1:]) + [n]
        for k, a, b in zip(ks, starts, ends):
            blk = xd[order[a:b], m, :]
            for j in range(dsub):
                out[m, k, j] = math.fsum(blk[:, j].tolist())
    return out


def midpoint_cases(seed=7, per_count=24):
    """(sums fp64, counts int64, mid fp64): sums[i] / counts[i] lies within one fp64 ulp of mid[i], and mid[i] is the exact
    middle of two neighbouring fp32 values — a division or a conversion that is not correctly rounded picks the wrong one."""
    rng = np.random.default_rng(seed)
    S, Cn, Mid = [], [], []
    for c in (1, 2, 3, 7, 2 ** 31 + 1):
        f = (rng.standard_normal(per_count) * np.ldexp(1.0, rng.integers(-30, 30, per_count))).astype(F32)
        f = f[f != 0]
        mid = (f.astype(F64) + np.nextafter(f, F32(np.inf)).astype(F64)) / 2.0          # 25 significant bits: exact in fp64
        s0 = mid * float(c)
        for s in (s0, np.nextafter(s0, np.inf), np.nextafter(s0, -np.inf)):
            keep = np.abs(s / float(c) - mid) <= np.spacing(np.abs(mid))
            S.append(s[keep]); Cn.append(np.full(int(keep.sum()), c, np.int64)); Mid.append(mid[keep])
    return np.concatenate(S), np.concatenate(Cn), np.concatenate(Mid)


UPDATE_SPECIALS = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e300, -1e300, 1e-40, -3e-42, 1e-320, 5e-324, 3.0e38 * 7]


def update_case(seed=11, M=2, dsub=4):
    """(sums [M, 256, dsub] fp64, counts [M, 256] int64, old bits [M, 256, dsub] uint32) for test 7."""
    rng = np.random.default_rng(seed)
    counts = np.array(UPDATE_COUNTS, np.int64)[np.arange(M * 256) % len(UPDATE_COUNTS)].reshape(M, 256)
    sums = rng.standard_normal((M, 256, dsub)) * 100.0
    sums[0, 0, 0] = np.nan                                           # count -3: must not reach the centroid
    ms, mc, _ = midpoint_cases()
    for c in UPDATE_COUNTS:
        if c <= 0:
            continue
        pool = np.concatenate([ms[mc == c], np.array(UPDATE_SPECIALS)])
        where = np.argwhere(counts == c)
        flat = np.resize(pool, len(where) * dsub).reshape(len(where), dsub)
        for (m, k), row in zip(where, flat):
            sums[m, k] = row
    return sums, counts, bit_table(M, dsub)


def update_want_bits(sums, counts, old_bits):
    with np.errstate(all="ignore"):
        new = (sums / counts[..., None].astype(F64)).astype(F32)
    return np.where(counts[..., None] > 0, new.view(np.uint32), old_bits), np.isnan(new) & (counts[..., None] > 0)


# ------------------------------------------------------------------------------------------------------------ GPU helpers
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _num_cus():
    from repconc_amd import _lib
    return int(_lib.load().rc_num_cus(_lib.handle(0)))


def _table(M, dsub):
    return _t(bit_table(M, dsub).view(F32))


def _gather_bits(C, codes):
    """int32 [n, M * dsub]: C[arange(M), codes & 255] by torch indexing."""
    M = C.shape[0]
    idx = codes.long() & 255
    return _bits(C)[torch.arange(M, device=C.device), idx].reshape(codes.shape[0], M * C.shape[2])


def _sizes(M, dsub, vec4):
    D = M * dsub
    s = [0, 1, 3, 255, 4097, *straddle(_num_cus(), D)]
    if vec4 and dsub % 4 == 0:
        s += list(straddle(_num_cus(), D, 4))
    return s


def _decode_cases(M, dsub, vec4):
    cases = [(f, n) for n in _sizes(M, dsub, vec4) for f in ("uniform", "one_code")]
    if (M, dsub) in FULL_SHAPES:
        cases += [(f, n) for f in ("two_hot", "column_const", "cyclic") for n in (3, 255, 4097)]
        cases += [("pairs", 512), ("uniform", 70001), ("one_code", 70001)]
    return cases


# ------------------------------------------------------------------------------------------------------------ 1 decode
@gpu
@pytest.mark.parametrize("M,dsub", SHAPES)
def test_decode_forward_is_a_bit_exact_copy(M, dsub):
    from repconc_amd import ops
    C = _table(M, dsub)
    buf = torch.empty(C.numel() + 1, dtype=torch.float32, device=DEV)
    buf[1:] = C.reshape(-1)
    C_off = buf[1:].view(M, 256, dsub)                               # contiguous, one float into its storage: the copy path
    assert C_off.is_contiguous() and C_off.data_ptr() % 16 == 4
    for i, (family, n) in enumerate(_decode_cases(M, dsub, vec4=True)):
        c8 = _t(codes_of(family, n, M, seed=i))
        want = _gather_bits(C, c8)
        for codes in (c8, c8.long()):
            out = ops.decode_raw(codes, C)
            assert out.shape == (n, M * dsub) and out.dtype == torch.float32
            assert torch.equal(_bits(out), want), (family, n, codes.dtype)
        if n in (255, 4097):
            wider = torch.full((n, M + 5), 77, dtype=torch.uint8, device=DEV)
            wider[:, 3:3 + M] = c8
            assert torch.equal(_bits(ops.decode_raw(wider[:, 3:3 + M], C)), want), (family, n, "column slice")
            tr = c8.long().t().contiguous().t()                      # [n, M] with strides (1, n)
            assert not tr.is_contiguous() or M == 1 or n == 1
            assert torch.equal(_bits(ops.decode_raw(tr, C)), want), (family, n, "transposed view")
            assert torch.equal(_bits(ops.decode_raw(c8, C_off)), want), (family, n, "centroids at a 4-byte offset")


# ------------------------------------------------------------------------------------------------------------ 2 backward
def _backward(codes, C0, go):
    from repconc_amd import ops
    Cp = C0.clone().requires_grad_(True)
    ops.decode(codes, Cp).backward(go)
    return Cp.grad


def _bwd_cases(M, dsub):
    """(code family, gradient family, n, both code dtypes).  int64 codes go with the integer gradients, whose check is exact.
    Contended fp32 atomics on one cache line retire at about one per microsecond, so where D is small (all n rows of one_code on
    two or three lines) one_code keeps its exact integer check and leaves out the Gaussian one and the 70001 rows."""
    D = M * dsub
    cases = []
    for n in straddle(_num_cus(), D):
        cases += [("uniform", "ints", n, True), ("uniform", "gauss", n, False), ("one_code", "ints", n, D >= 256)]
        if D >= 256:
            cases += [("one_code", "gauss", n, False)]
    if (M, dsub) in FULL_SHAPES:
        cases += [(f, g, n, g == "ints") for f in ("uniform", "one_code", "two_hot", "column_const", "cyclic")
                  for g in GRAD_FAMILIES for n in (1, 3, 255, 4097)]
        cases += [("pairs", g, 512, g == "ints") for g in GRAD_FAMILIES]
        cases += [("uniform", "ints", 70001, True), ("uniform", "gauss", 70001, False)]
        if D >= 256:
            cases += [("one_code", "ints", 70001, False), ("one_code", "gauss", 70001, False)]
    return cases


@gpu
@pytest.mark.parametrize("M,dsub", SHAPES)
def test_decode_gradient_against_the_fp64_scatter(M, dsub):
    D = M * dsub
    C0 = _t(synth.gaussian(31, (M, 256, dsub)))
    worst = dict.fromkeys(GRAD_FAMILIES, 0.0)
    gos = {}                                                         # one gradient per (family, n), shared by the code families
    for i, (family, gfam, n, both) in enumerate(_bwd_cases(M, dsub)):
        c8 = _t(codes_of(family, n, M, seed=i))
        if (gfam, n) not in gos:
            gos[gfam, n] = _t(grad_of(gfam, n, D, seed=n))
        go = gos[gfam, n]
        for codes in (c8, c8.long()) if both else (c8,):
            grad = _backward(codes, C0, go)
            try:
                r = check_gradient(grad, c8, go, M, exact=(gfam == "ints"))
            except AssertionError as e:
                raise AssertionError(f"{family} / {gfam} / n = {n} / {codes.dtype}: {e}") from None
            worst[gfam] = max(worst[gfam], r)
    print(f"\n[decode_bwd M={M} dsub={dsub}] worst err / bound: " + "  ".join(f"{g} {worst[g]:.3g}" for g in worst))


# ------------------------------------------------------------------------------------------------------------ 3 autograd
@gpu
@pytest.mark.parametrize("M,dsub", FULL_SHAPES)
def test_decode_autograd_surface(M, dsub):
    from repconc_amd import ops
    D = M * dsub
    C0 = _t(synth.gaussian(32, (M, 256, dsub)))
    for family, n in (("uniform", 4097), ("one_code", 4097), ("two_hot", 70001), ("cyclic", 255)):
        for codes in (_t(codes_of(family, n, M)), _t(codes_of(family, n, M)).long()):
            Cp = C0.clone().requires_grad_(True)
            ops.decode(codes, Cp).sum().backward()                   # grad_out is a stride-0 expansion of one 1.0
            want = ops.code_hist(codes).float()[..., None].expand(M, 256, dsub)
            assert torch.equal(_bits(Cp.grad), _bits(want)), (family, n)
    # two decodes in one graph accumulate (integer gradients: exact)
    c1, c2 = _t(codes_of("uniform", 300, M, 1)), _t(codes_of("two_hot", 777, M, 2))
    g1, g2 = _t(grad_of("ints", 300, D, 1)), _t(grad_of("ints", 777, D, 2))
    Cp = C0.clone().requires_grad_(True)
    ((ops.decode(c1, Cp) * g1).sum() + (ops.decode(c2, Cp) * g2).sum()).backward()
    want = scatter64(c1, g1, M)[0] + scatter64(c2, g2, M)[0]
    assert torch.equal(_bits(Cp.grad), _bits(want.float()))
    # fp16 / bf16 centroids: the forward decodes Cp.float(), the gradient is the fp32 gradient cast once
    for dt in (torch.float16, torch.bfloat16):
        for family, gfam, n in (("cyclic", "gauss", 255), ("one_code", "ints", 4097), ("pairs", "wide", 512)):
            codes, go = _t(codes_of(family, n, M)), _t(grad_of(gfam, n, D))
            Ch = C0.to(dt).requires_grad_(True)
            out = ops.decode(codes, Ch)
            assert out.dtype == torch.float32 and torch.equal(_bits(out), _bits(ops.decode_raw(codes, Ch.detach().float())))
            out.backward(go)
            g32 = _backward(codes, C0, go)                           # order-free inputs: bins of <= 2 members, or integers
            assert Ch.grad.dtype == dt and torch.equal(Ch.grad, g32.to(dt)), (dt, family)
    # no rows
    for codes in (torch.empty((0, M), dtype=torch.uint8, device=DEV), torch.empty((0, M), dtype=torch.int64, device=DEV)):
        Cp = C0.clone().requires_grad_(True)
        out = ops.decode(codes, Cp)
        assert out.shape == (0, D) and out.dtype == torch.float32
        out.sum().backward()
        assert Cp.grad.shape == (M, 256, dsub) and not bool(_bits(Cp.grad).any())
        assert ops.decode_raw(codes, C0).shape == (0, D)


# ------------------------------------------------------------------------------------------------------------ 4 histogram
def _bincount(codes):
    M = codes.shape[1]
    idx = ((codes.long() & 255) + 256 * torch.arange(M, device=codes.device)[None, :]).reshape(-1)
    return torch.bincount(idx, minlength=M * 256).view(M, 256)


@gpu
@pytest.mark.parametrize("M", HIST_M)
def test_code_histogram_is_bincount(M):
    from repconc_amd import ops
    cases = [(f, n) for f in ("uniform", "one_code", "two_hot", "column_const", "cyclic") for n in HIST_N] + [("pairs", 512)]
    for i, (family, n) in enumerate(cases):
        c8 = _t(codes_of(family, n, M, seed=i))
        want = _bincount(c8)
        assert int(want.sum()) == n * M
        for codes in (c8, c8.long()):
            h1 = ops.code_hist(codes)
            h2 = ops.code_hist(codes)                                # same stream, the allocator hands back a used block
            assert h1.dtype == torch.int32 and h1.shape == (M, 256)
            assert torch.equal(h1.long(), want), (family, n, codes.dtype)
            assert torch.equal(h2, h1), "the histogram is overwritten, not accumulated"
    # into a buffer that holds an earlier, larger histogram
    big, small = _t(codes_of("one_code", 8193, M)), _t(codes_of("uniform", 255, M))
    ops.code_hist(big)
    assert torch.equal(ops.code_hist(small).long(), _bincount(small))


# ------------------------------------------------------------------------------------------------------------ 5 low byte
@gpu
@pytest.mark.parametrize("M,dsub", FULL_SHAPES)
def test_only_the_low_byte_of_an_int64_code_is_read(M, dsub):
    """Memory safety, not a recommendation: whatever an int64 code holds, the kernels index with code & 255."""
    from repconc_amd import ops
    n, D = 4097, M * dsub
    rng = np.random.default_rng(5)
    low = codes_of("uniform", n, M).astype(np.int64)
    high = rng.choice(np.array([0, 256, -256, 2 ** 40, -2 ** 40, 2 ** 62, -2 ** 63, 2 ** 32, 2 ** 31], np.int64), size=(n, M))
    wild = low + high                                                # same low byte (two's complement), wild upper bits
    assert np.array_equal(wild & 255, low) and (wild != low).sum() > n * M // 2
    wild[0, 0], wild[1, 0], wild[2, 0] = 256, -1, 2 ** 40 + 3
    cw, cl = _t(wild), _t(wild & 255)
    C = _table(M, dsub)
    assert torch.equal(_bits(ops.decode_raw(cw, C)), _bits(ops.decode_raw(cl, C)))
    assert torch.equal(_bits(ops.decode_raw(cw, C)), _gather_bits(C, cl))
    assert torch.equal(ops.code_hist(cw), ops.code_hist(cl)) and torch.equal(ops.code_hist(cw).long(), _bincount(cl))
    go = _t(grad_of("ints", n, D))
    C0 = _t(synth.gaussian(33, (M, 256, dsub)))
    gw = _backward(cw, C0, go)
    assert torch.equal(_bits(gw), _bits(_backward(cl, C0, go)))
    check_gradient(gw, cl, go, M, exact=True)


# ------------------------------------------------------------------------------------------------------------ 6 normalise
def _norm_rows(family, rows, dsub, seed):
    rng = np.random.default_rng(3000 + seed)
    if family == "wide":                                             # a row's norm anywhere in 2^-20 .. 2^20 as well
        return (_wide(rows, dsub, rng) * np.ldexp(1.0, rng.integers(-20, 20, size=(rows, 1)))).astype(F32)
    return GRAD_FAMILIES[family](rows, dsub, rng)


@gpu
@pytest.mark.parametrize("dsub", NORM_DSUB)
def test_normalize_against_fp64_within_the_derived_bound(dsub):
    from repconc_amd import ops
    M = 2
    for family in ("gauss", "wide", "cancel"):
        C = _norm_rows(family, M * 256, dsub, dsub).reshape(M, 256, dsub)
        got = ops.normalize_centroids_(_t(C).clone()).cpu().numpy().astype(F64)
        c64 = C.astype(F64)
        want = c64 / np.maximum(np.sqrt((c64 * c64).sum(-1, keepdims=True)), float(F32(1e-12)))
        excess = np.abs(got - want) - norm_bound(dsub) * np.abs(want)
        assert (excess <= 0).all(), (family, float(excess.max()))
        print(f"\n[normalize dsub={dsub} {family}] worst err / bound: "
              f"{float((np.abs(got - want) / (norm_bound(dsub) * np.abs(want) + 1e-300)).max()):.3g}")


def _edge_rows(dsub):
    z = np.zeros(dsub, F32)
    zero = z.copy(); zero[dsub // 2] = F32(-0.0)
    tiny = z.copy(); tiny[0], tiny[-1] = F32(3e-14), F32(-1e-14)                         # norm 3.2e-14 < 1e-12
    under = np.resize(np.array([1e-30, -1e-30, 1e-21], F32), dsub)                       # every square underflows (<= 1e-42)
    over = z.copy(); over[0], over[1], over[2] = F32(1e30), F32(-1e30), F32(1.0)         # 1e60 -> inf
    nan = np.random.default_rng(4).standard_normal(dsub).astype(F32); nan[1] = np.nan
    return {"zero": zero, "tiny": tiny, "under": under, "over": over, "nan": nan}


@gpu
@pytest.mark.parametrize("dsub", [3, 16, 96])
def test_normalize_edge_rows_follow_f_normalize(dsub):
    from repconc_amd import ops
    M = 2
    base = synth.gaussian(34, (M, 256, dsub))
    clean = ops.normalize_centroids_(_t(base).clone()).cpu().numpy()
    edges = _edge_rows(dsub)
    at = dict(zip(edges, [0, 7, 255, 256, 511]))                     # first row, both sides of a block boundary, last row
    C = base.copy().reshape(M * 256, dsub)
    for name, r in at.items():
        C[r] = edges[name]
    got = ops.normalize_centroids_(_t(C.reshape(M, 256, dsub)).clone()).cpu().numpy().reshape(M * 256, dsub)
    ref = torch.nn.functional.normalize(torch.from_numpy(C), p=2.0, dim=-1).numpy()
    others = np.setdiff1d(np.arange(M * 256), list(at.values()))
    assert np.array_equal(got[others].view(np.uint32), clean.reshape(M * 256, dsub)[others].view(np.uint32)), "a neighbour changed"
    b = lambda a: a.view(np.uint32)
    assert np.array_equal(b(got[at["zero"]]), b(edges["zero"])) and np.array_equal(b(got[at["zero"]]), b(ref[at["zero"]]))
    assert np.array_equal(b(got[at["tiny"]]), b(edges["tiny"] / F32(1e-12))) and np.array_equal(b(got[at["tiny"]]), b(ref[at["tiny"]]))
    g, w = got[at["under"]].astype(F64), ref[at["under"]].astype(F64)
    assert (np.abs(g - w) <= norm_bound(dsub) * np.abs(w)).all() and (w != 0).all()      # |w| = |x| / 1e-12: scaled by the clamp
    assert np.array_equal(b(got[at["over"]]), b(ref[at["over"]])) and not got[at["over"]].any()
    assert np.isnan(ref[at["nan"]]).all() and np.isnan(got[at["nan"]]).all()
    assert int(np.isnan(got).sum()) == dsub, "NaN outside its row"


# ------------------------------------------------------------------------------------------------------------ 7 update
@gpu
def test_kmeans_update_is_bit_exact():
    from repconc_amd import ops
    sums, counts, old_bits = update_case()
    want, want_nan = update_want_bits(sums, counts, old_bits)
    got = ops.kmeans_update_(_t(sums), _t(counts), _t(old_bits.view(F32)).clone())
    got_bits = got.cpu().numpy().view(np.uint32)
    keep = counts[..., None] <= 0
    assert np.array_equal(got_bits[np.broadcast_to(keep, got_bits.shape)], old_bits[np.broadcast_to(keep, got_bits.shape)])
    assert np.isnan(got.cpu().numpy()[want_nan]).all() and int(want_nan.sum()) > 0
    diff = (got_bits != want) & ~want_nan
    assert not diff.any(), [(tuple(i), counts[i[0], i[1]], sums[tuple(i)], hex(got_bits[tuple(i)]), hex(want[tuple(i)]))
                            for i in np.argwhere(diff)[:8]]


# ------------------------------------------------------------------------------------------------------------ 8 statistics
@functools.lru_cache(maxsize=None)
def _skew_case(family, M, n):
    x = synth.gaussian(80 + M, (n, 768))
    codes = codes_of(family, n, M)
    want = _fsum_stats(x, codes, M)
    cnt = np.stack([np.bincount(codes[:, m], minlength=256) for m in range(M)]).astype(np.int64)
    want.setflags(write=False); cnt.setflags(write=False)
    return x, codes, want, cnt


@gpu
@pytest.mark.parametrize("family", ["one_code", "two_hot"])
@pytest.mark.parametrize("M,n", [(48, 70001), (8, 5000)])
def test_kmeans_statistics_under_skew(family, M, n, monkeypatch):
    from repconc_amd import ops
    x, codes, want, cnt = _skew_case(family, M, n)
    xt, ct = _t(x), _t(codes)
    s1, c1 = ops.kmeans_stats(xt, ct)
    assert np.array_equal(c1.cpu().numpy(), cnt)
    assert np.array_equal(s1.cpu().numpy(), want), "not the correctly rounded sums"
    s2, c2 = ops.kmeans_stats(xt, ct, s1.clone(), c1.clone())       # accumulates: s + s is exact
    assert np.array_equal(s2.cpu().numpy(), 2.0 * want) and np.array_equal(c2.cpu().numpy(), 2 * cnt)
    monkeypatch.setenv("RC_KMEANS_STRIPS", "1")                      # the fixed-order strip kernels, at their test's tolerance
    s3, c3 = ops.kmeans_stats(xt, ct)
    assert np.array_equal(c3.cpu().numpy(), cnt)
    np.testing.assert_allclose(s3.cpu().numpy(), want, rtol=1e-12, atol=1e-9)


# ------------------------------------------------------------------------------------------------------------ 9 > 2^31
@gpu
def test_decode_gradient_and_histogram_past_2_31_elements():
    from repconc_amd import ops
    n, M, dsub = 2_796_300, 48, 16
    D, step = M * dsub, 1 << 17
    assert n * D > 2 ** 31 and 4 * n < 2 ** 24
    gen = torch.Generator(device=DEV)
    gen.manual_seed(9)
    codes = torch.randint(0, 256, (n, M), generator=gen, device=DEV, dtype=torch.uint8)
    C = _table(M, dsub)
    out = ops.decode_raw(codes, C)
    ob = out.view(torch.int32)
    for r0 in range(0, n, step):
        assert torch.equal(ob[r0:r0 + step], _gather_bits(C, codes[r0:r0 + step])), r0
    assert torch.equal(ob[n - 3:], _gather_bits(C, codes[n - 3:]))   # the rows past element 2^31
    assert (n - 3) * D > 2 ** 31
    del out, ob
    # histogram
    want_h = torch.zeros((M, 256), dtype=torch.int64, device=DEV)
    for r0 in range(0, n, step):
        want_h += _bincount(codes[r0:r0 + step])
    assert torch.equal(ops.code_hist(codes).long(), want_h)
    # backward: integers, exact in any order
    go8 = torch.randint(-4, 5, (n, D), generator=gen, device=DEV, dtype=torch.int8)
    go = go8.float()
    Cp = _t(synth.gaussian(35, (M, 256, dsub))).requires_grad_(True)
    ops.decode(codes, Cp).backward(go)
    del go
    ref = torch.zeros(M * 256 * dsub, dtype=torch.int32, device=DEV)
    col = ((torch.arange(M, device=DEV) * 256)[:, None] * dsub + torch.arange(dsub, device=DEV)[None, :])[None]     # [1, M, dsub]
    for r0 in range(0, n, step):
        idx = (codes[r0:r0 + step].long()[:, :, None] * dsub + col).reshape(-1)
        ref.index_add_(0, idx, go8[r0:r0 + step].reshape(-1).to(torch.int32))
        del idx
    assert torch.equal(_bits(Cp.grad), _bits(ref.float().view(M, 256, dsub)))
    del go8, ref, codes, Cp
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ 10 CPU: the bound
def _ordered_sum32(codes, go, M, order):
    """[M, 256, dsub] fp32: every bin's members added one by one in fp32, rows visited in `order`."""
    dsub = go.shape[1] // M
    acc = np.zeros((M, 256, dsub), F32)
    g = go.reshape(len(go), M, dsub)
    ar = np.arange(M)
    for r in order:
        acc[ar, codes[r]] += g[r]
    return acc


def _pairwise_sum32(codes, go, M):
    dsub = go.shape[1] // M
    acc = np.zeros((M, 256, dsub), F32)
    g = go.reshape(len(go), M, dsub)
    for m in range(M):
        for k in np.unique(codes[:, m]):
            a = g[codes[:, m] == k, m, :]
            while len(a) > 1:
                if len(a) % 2:
                    a = np.concatenate([a, np.zeros((1, dsub), F32)])
                a = a[0::2] + a[1::2]
            acc[m, k] = a[0]
    return acc


@pytest.mark.parametrize("gfam", list(GRAD_FAMILIES))
@pytest.mark.parametrize("family", ["one_code", "two_hot", "uniform"])
def test_bound_of_the_gradient_test_holds_for_four_summation_orders_on_the_cpu(family, gfam):
    n, M, dsub = 4097, 3, 4
    codes, go = codes_of(family, n, M), grad_of(gfam, n, M * dsub)
    want, A, c = scatter64(torch.from_numpy(codes), torch.from_numpy(go), M)
    bound = bwd_bound(c, A, want).numpy()
    sums = [_ordered_sum32(codes, go, M, range(n)), _ordered_sum32(codes, go, M, range(n - 1, -1, -1)),
            _ordered_sum32(codes, go, M, np.random.default_rng(6).permutation(n)), _pairwise_sum32(codes, go, M),
            pq_oracle.decode_bwd(codes, go, M, 256)]
    for s in sums:
        assert s.dtype == F32 and (np.abs(s.astype(F64) - want.numpy()) <= bound).all()
    if gfam == "ints":
        for s in sums:
            assert np.array_equal(s.view(np.uint32), want.numpy().astype(F32).view(np.uint32))
    elif family != "uniform":                                        # the orders really differ: the bound is not vacuous
        assert any(not np.array_equal(sums[0], s) for s in sums[1:4])


# ------------------------------------------------------------------------------------------------------------ 11 CPU: the inputs
def test_families_sizes_and_midpoints_are_what_they_claim():
    for M in (1, 5, 48):
        for n in (0, 1, 255, 4097):
            for f in ("uniform", "one_code", "two_hot", "column_const", "cyclic"):
                c = codes_of(f, n, M)
                assert c.shape == (n, M) and c.dtype == np.uint8
        h = pq_oracle.code_histogram(codes_of("one_code", 4097, M))
        assert (h[:, 255] == 4097).all() and h.sum() == 4097 * M
        h = pq_oracle.code_histogram(codes_of("two_hot", 4097, M))
        assert (h[:, 255] == 4097 - 40).all() and (h[:, 0] == 40).all()
        assert (pq_oracle.code_histogram(codes_of("pairs", 512, M)) == 2).all()
        assert pq_oracle.code_histogram(codes_of("cyclic", 256, M)).max() == 1
        assert pq_oracle.code_histogram(codes_of("cyclic", 255, M)).max() == 1
        h = pq_oracle.code_histogram(codes_of("column_const", 300, M))
        assert all(h[m, m % 256] == 300 for m in range(M))
    g = grad_of("ints", 4097, 12)
    assert np.array_equal(g, np.rint(g)) and np.abs(g).max() == 4
    w = np.abs(grad_of("wide", 4097, 12))
    assert w.min() >= 2.0 ** -20 and w.max() < 2.0 ** 20 and w.min() < 2.0 ** -18 and w.max() > 2.0 ** 18
    cz = grad_of("cancel", 4096, 4).astype(F64).sum(0)
    assert (np.abs(cz) < 1000).all()                                 # 4096 x 1e4 of magnitude, O(sqrt n) left
    # the straddling sizes: 256 CUs -> 2048 blocks of 256 threads
    assert straddle(256, 768) == (682, 683) and straddle(256, 768, 4) == (2730, 2731) and straddle(256, 35) == (14979, 14980)
    for cus in (64, 256, 304):
        for D in (35, 60, 768):
            lo, hi = straddle(cus, D)
            assert lo * D <= cus * 8 * 256 < hi * D
    # every element of a table has its own bits, the special ones included
    for M, dsub in SHAPES + [(2, 4)]:
        t = bit_table(M, dsub)
        assert np.unique(t).size == t.size and np.isin(np.array(SPECIAL_BITS, np.uint32), t).all()
    # test 7's quotients sit within an fp64 ulp of a fp32 tie, on both sides of it and on it
    s, c, mid = midpoint_cases()
    assert len(s) >= 100 and set(c.tolist()) == {1, 2, 3, 7, 2 ** 31 + 1}
    q = s / c.astype(F64)
    assert (np.abs(q - mid) <= np.spacing(np.abs(mid))).all()
    lo32 = mid.astype(F32)                                            # a tie rounds to one of its neighbours ...
    other = np.where(lo32.astype(F64) < mid, np.nextafter(lo32, F32(np.inf)), np.nextafter(lo32, F32(-np.inf)))
    assert (np.abs(lo32.astype(F64) - mid) == np.abs(other.astype(F64) - mid)).all() and (lo32 != other).all()   # ... equally far
    assert (q < mid).sum() > 10 and (q > mid).sum() > 10 and (q == mid).sum() > 10
    sums, counts, old = update_case()
    assert set(np.unique(counts).tolist()) == set(UPDATE_COUNTS)
    want, want_nan = update_want_bits(sums, counts, old)
    assert want_nan.any() and (want[counts <= 0] == old[counts <= 0]).all()
    assert np.isin(s[c == 7], sums[counts == 7]).all()               # the midpoint sums made it into the case


def test_header_states_the_low_byte_rule():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(open(os.path.join(root, "include", "repconc_hip.h")).read().split())
    assert text.count("low 8 bits of an int64 code are read") >= 2


# ------------------------------------------------------------------------------------------------------------ 12 CPU: wrappers
def test_wrappers_reject_bad_arguments_before_anything_is_launched():
    """ValueError on CPU tensors: the shape / dtype checks come before the device check, so nothing was launched.  The
    well-formed call on CPU tensors gets as far as the device check (RepconcHipError)."""
    from repconc_amd import _lib, ops
    M, dsub, n = 2, 4, 10
    C = torch.zeros(M, 256, dsub)
    s = torch.zeros(M, 256, dsub, dtype=torch.float64)
    c = torch.zeros(M, 256, dtype=torch.int64)
    bad_update = {
        "fp32 sums": (s.float(), c, C),
        "strided sums": (torch.zeros(M, 256, 2 * dsub, dtype=torch.float64)[..., ::2], c, C),
        "int32 counts": (s, c.int(), C),
        "strided counts": (s, torch.zeros(M, 512, dtype=torch.int64)[:, ::2], C),
        "sums of another width": (torch.zeros(M, 256, dsub + 1, dtype=torch.float64), c, C),
        "sums of another M": (torch.zeros(M + 1, 256, dsub, dtype=torch.float64), c, C),
        "counts [M, 255]": (s, torch.zeros(M, 255, dtype=torch.int64), C),
        "counts [M, 256, 1]": (s, c[..., None], C),
        "fp64 centroids": (s, c, C.double()),
        "strided centroids": (s, c, torch.zeros(M, 256, 2 * dsub)[..., ::2]),
        "2-D centroids": (s, c, torch.zeros(M * 256, dsub)),
    }
    for name, args in bad_update.items():
        with pytest.raises(ValueError):
            ops.kmeans_update_(*args)
            pytest.fail(name)
    with pytest.raises(_lib.RepconcHipError):
        ops.kmeans_update_(s, c, C)
    x, codes = torch.zeros(n, M * dsub), torch.zeros(n, M, dtype=torch.uint8)
    bad_stats = {
        "rows differ": (x, codes[:-1]),
        "D % M": (torch.zeros(n, M * dsub + 1), codes),
        "1-D codes": (x, codes[:, 0]),
        "1-D x": (x[0], codes),
        "fp32 sums": (x, codes, s.float(), c),
        "sums of another shape": (x, codes, torch.zeros(M, 256, dsub + 1, dtype=torch.float64), c),
        "strided sums": (x, codes, torch.zeros(M, 256, 2 * dsub, dtype=torch.float64)[..., ::2], c),
        "int32 counts": (x, codes, s, c.int()),
        "counts of another shape": (x, codes, s, torch.zeros(M, 255, dtype=torch.int64)),
        "strided counts": (x, codes, s, torch.zeros(M, 512, dtype=torch.int64)[:, ::2]),
    }
    for name, args in bad_stats.items():
        with pytest.raises(ValueError):
            ops.kmeans_stats(*args)
            pytest.fail(name)
    with pytest.raises(_lib.RepconcHipError):
        ops.kmeans_stats(x, codes, s, c)
    for codes_bad in (codes[:, 0], codes[None], torch.zeros((), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ops.code_hist(codes_bad)
    with pytest.raises(ValueError):
        ops.code_hist(codes.to(torch.int32))
    with pytest.raises(_lib.RepconcHipError):
        ops.code_hist(codes)
    for dt in (torch.int32, torch.int16, torch.int8, torch.float32):
        with pytest.raises(ValueError):
            ops.decode_raw(codes.to(dt), C)
    with pytest.raises(ValueError):
        ops.decode_raw(codes[:, :1], C)
    with pytest.raises(ValueError):
        ops.decode_raw(codes, torch.zeros(M, 255, dsub))
    with pytest.raises(_lib.RepconcHipError):
        ops.decode_raw(codes, C)


def test_centroid_views_at_an_unaligned_storage_offset_are_copied():
    """_centroids() hands the kernels a pointer they read with float4 loads: a contiguous view that starts one float into its
    storage is copied, an aligned one is passed through."""
    from repconc_amd import ops
    buf = torch.zeros(2 * 256 * 4 + 4)
    off = buf[1:1 + 2048].view(2, 256, 4)
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    got = ops._centroids(off)
    assert got.data_ptr() % 16 == 0 and got.data_ptr() != off.data_ptr() and torch.equal(got, off)
    ok = buf[4:4 + 2048].view(2, 256, 4)
    assert ops._centroids(ok).data_ptr() == ok.data_ptr()
