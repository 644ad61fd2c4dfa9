"""The argument order of the flat and IVF-flat search entries, as Python hands it to the library: the pure builders
`ops._dense_call` and `ops._ivf_flat_call` against the prototypes of include/repconc_hip.h, position by position.

The expected orders below are written out by hand from the header, one literal list per entry; they are not derived from
`ops._DenseVariant` or from `_lib.PROTOTYPES` (only the LENGTH of a tuple is also compared with PROTOTYPES).  Every tensor has
its own address and every scalar its own value, so a swapped, missing or extra argument shows: a folded table cannot silently
hand the library a [2, D] buffer where it reads [N] floats.  CPU tensors only: no GPU, no library.
"""
import pytest
import torch

from repconc_amd import _lib, ops

N, D, NQ, K, LDX = 5, 8, 3, 2, 12
ID_OFFSET, SEL_SLACK, H, STREAM, WS_BYTES = 7, 1.25, 101, 202, 13
NLIST, NPROBE, STRIDE, METRIC, LDC = 6, 4, 16, 1, 11


def _tensors():
    t = {"x": torch.zeros((N, LDX))[:, :D], "q": torch.zeros((NQ, D)), "dec": torch.zeros((2, D)), "xsq": torch.zeros((N,)),
         "xnorm_max": torch.zeros((1,)), "cstat": torch.zeros((2,)), "scores": torch.zeros((NQ, K)),
         "ids": torch.zeros((NQ, K), dtype=torch.int64), "status": torch.zeros((1,), dtype=torch.int32),
         "qstatus": torch.zeros((NQ,), dtype=torch.int32), "out": torch.zeros((NQ, N)),
         "ws": torch.zeros((WS_BYTES,), dtype=torch.uint8),
         # the IVF-flat entries
         "list_off": torch.zeros((NLIST + 1,), dtype=torch.int64), "row_ids": torch.zeros((N,), dtype=torch.int64),
         "probes": torch.zeros((NQ, NPROBE), dtype=torch.int32), "coarse": torch.zeros((NLIST, LDC))[:, :D]}
    assert len({v.data_ptr() for v in t.values()}) == len(t)
    return t


T = _tensors()
VALUE = dict({name: t.data_ptr() for name, t in T.items()}, h=H, ldx=LDX, N=N, D=D, nq=NQ, k=K, id_offset=ID_OFFSET,
             sel_slack=SEL_SLACK, ws_bytes=WS_BYTES, stream=STREAM, nlist=NLIST, nprobe=NPROBE, stride=STRIDE, metric=METRIC,
             ldc=LDC)
assert len(set(VALUE.values())) == len(VALUE)          # no two arguments can stand in for each other


def _check(name, args, want_name, order):
    assert name == want_name
    got = [getattr(a, "value", a) for a in args]        # c_void_p -> the address
    assert got == [VALUE[n] for n in order.split(", ")], name
    assert len(args) == len(_lib.PROTOTYPES[name][1]), name


# ---- the eight flat variants: (variant, its search entry and order, its exact entry and order) — include/repconc_hip.h
FLAT = [
    ("_DENSE_F32",
     "rc_dense_search_q",
     "h, x, ldx, N, D, q, nq, k, id_offset, sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream",
     "rc_dense_search_exact", "h, x, ldx, N, D, q, nq, k, id_offset, scores, ids, ws, ws_bytes, stream"),
    ("_DENSE_F16",
     "rc_dense_f16_search_q",
     "h, x, ldx, N, D, q, nq, xnorm_max, k, id_offset, sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream",
     "rc_dense_f16_search_exact", "h, x, ldx, N, D, q, nq, k, id_offset, scores, ids, ws, ws_bytes, stream"),
    ("_DENSE_BF16X3",
     "rc_dense_bf16x3_search_q",
     "h, x, ldx, N, D, q, nq, xnorm_max, k, id_offset, sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream",
     "rc_dense_search_exact", "h, x, ldx, N, D, q, nq, k, id_offset, scores, ids, ws, ws_bytes, stream"),
    ("_DENSE_SQ8",
     "rc_dense_sq8_search_q",
     "h, x, ldx, N, D, q, nq, dec, cstat, k, id_offset, sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream",
     "rc_dense_sq8_search_exact", "h, x, ldx, N, D, q, nq, dec, k, id_offset, scores, ids, ws, ws_bytes, stream"),
    ("_DENSE_L2",
     "rc_dense_l2_search_q",
     "h, x, ldx, N, D, q, nq, xsq, xnorm_max, k, id_offset, sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream",
     "rc_dense_l2_search_exact", "h, x, ldx, N, D, q, nq, k, id_offset, scores, ids, ws, ws_bytes, stream"),
    ("_DENSE_L2_F16",
     "rc_dense_l2_f16_search_q",
     "h, x, ldx, N, D, q, nq, xsq, xnorm_max, k, id_offset, sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream",
     "rc_dense_l2_f16_search_exact", "h, x, ldx, N, D, q, nq, k, id_offset, scores, ids, ws, ws_bytes, stream"),
    ("_DENSE_L2_BF16X3",
     "rc_dense_l2_bf16x3_search_q",
     "h, x, ldx, N, D, q, nq, xsq, xnorm_max, k, id_offset, sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream",
     "rc_dense_l2_search_exact", "h, x, ldx, N, D, q, nq, k, id_offset, scores, ids, ws, ws_bytes, stream"),
    ("_DENSE_L2_SQ8",
     "rc_dense_l2_sq8_search_q",
     "h, x, ldx, N, D, q, nq, dec, xsq, cstat, k, id_offset, sel_slack, scores, ids, status, qstatus, ws, ws_bytes, stream",
     "rc_dense_l2_sq8_search_exact", "h, x, ldx, N, D, q, nq, dec, k, id_offset, scores, ids, ws, ws_bytes, stream"),
]


@pytest.mark.parametrize("variant, q_name, q_order, e_name, e_order", FLAT, ids=[f[0] for f in FLAT])
def test_flat_search_entries(variant, q_name, q_order, e_name, e_order):
    v = getattr(ops, variant)
    _check(*ops._dense_call(v, "search_q", H, T["x"], T["q"], T, STREAM, K, ID_OFFSET, SEL_SLACK), q_name, q_order)
    _check(*ops._dense_call(v, "search_exact", H, T["x"], T["q"], T, STREAM, K, ID_OFFSET), e_name, e_order)


# ---- the scores hooks: x, ldx, N, D, q, nq, [dec], [xsq], out, [ws, ws_bytes], stream
SCORES = [
    ("_DENSE_F16", "rc_dense_f16_scores", "h, x, ldx, N, D, q, nq, out, stream"),
    ("_DENSE_BF16X3", "rc_dense_bf16x3_scores", "h, x, ldx, N, D, q, nq, out, ws, ws_bytes, stream"),
    ("_DENSE_SQ8", "rc_dense_sq8_scores", "h, x, ldx, N, D, q, nq, dec, out, ws, ws_bytes, stream"),
    ("_DENSE_L2", "rc_dense_l2_scores", "h, x, ldx, N, D, q, nq, xsq, out, stream"),
    ("_DENSE_L2_F16", "rc_dense_l2_f16_scores", "h, x, ldx, N, D, q, nq, xsq, out, stream"),
    ("_DENSE_L2_BF16X3", "rc_dense_l2_bf16x3_scores", "h, x, ldx, N, D, q, nq, xsq, out, ws, ws_bytes, stream"),
    ("_DENSE_L2_SQ8", "rc_dense_l2_sq8_scores", "h, x, ldx, N, D, q, nq, dec, xsq, out, ws, ws_bytes, stream"),
]


@pytest.mark.parametrize("variant, name, order", SCORES, ids=[s[1] for s in SCORES])
def test_scores_entries(variant, name, order):
    v = getattr(ops, variant)
    # as `ops._dense_scores` fills it: a workspace only where the entry takes one
    t = {n: T[n] for n in T if n != "ws" or v.scores_ws}
    assert v.scores_ws == ("ws" in order)
    _check(*ops._dense_call(v, "scores", H, T["x"], T["q"], t, STREAM), name, order)


# ---- the four IVF-flat entries
IVF = [
    ("rc_ivf_flat_search", torch.float32, False, False,
     "h, x, ldx, list_off, row_ids, N, nlist, D, q, nq, probes, nprobe, stride, k, metric, "
     "scores, ids, status, qstatus, ws, ws_bytes, stream"),
    ("rc_ivf_flat_f16_search", torch.float16, False, False,
     "h, x, ldx, list_off, row_ids, N, nlist, D, q, nq, probes, nprobe, stride, k, metric, "
     "scores, ids, status, qstatus, ws, ws_bytes, stream"),
    ("rc_ivf_flat_sq8_search", torch.int8, True, False,
     "h, x, ldx, list_off, row_ids, N, nlist, D, q, nq, dec, probes, nprobe, stride, k, metric, "
     "scores, ids, status, qstatus, ws, ws_bytes, stream"),
    ("rc_ivf_flat_sq8r_search", torch.int8, True, True,
     "h, x, ldx, list_off, row_ids, N, nlist, D, q, nq, dec, coarse, ldc, probes, nprobe, stride, k, metric, "
     "scores, ids, status, qstatus, ws, ws_bytes, stream"),
]


@pytest.mark.parametrize("name, dtype, coded, residual, order", IVF, ids=[i[0] for i in IVF])
def test_ivf_flat_entries(name, dtype, coded, residual, order):
    itemsize = torch.empty((), dtype=dtype).element_size()
    xb = T["x"].view(torch.uint8).view(dtype)[:, :D]      # the same address in the store's type: N rows, pitch LDX * 4 / itemsize
    value = dict(VALUE, ldx=LDX * 4 // itemsize)
    got_name, args = ops._ivf_flat_call(H, xb, T["list_off"], T["row_ids"], T["q"], T["dec"] if coded else None,
                                        T["coarse"] if residual else None, T["probes"], STRIDE, K, METRIC, T["scores"], T["ids"],
                                        T["status"], T["qstatus"], T["ws"], STREAM)
    assert got_name == name
    assert [getattr(a, "value", a) for a in args] == [value[n] for n in order.split(", ")]
    assert len(args) == len(_lib.PROTOTYPES[name][1])
