"""The argument checks of the dense flat search entries, in the order the C ABI promises: all 8 `rc_*_search_q`, 6
`rc_*_search_exact`, 8 `rc_*_search_rows_*` and 7 `rc_*_scores` entries of include/repconc_hip.h.

The order (csrc/dense_screen.h, "the entries"):
  unmapped   shapes (RC_ESHAPE: N > 2^32 - 1, k > 8192, int8: D > 65536), then pointers, sizes and the alignment of the rows
             (RC_EINVAL), then the nq == 0 success, then the workspace (RC_EWORKSPACE), then device work
  rows       RC_ESHAPE on N or k, RC_EINVAL for ns outside [1, N], the checks above with `rows` among the pointers, the
             nq == 0 success, the workspace sized by ns
  scores     as unmapped without k; only rc_dense_l2_scores asks for aligned rows, the other screens have a form for any pitch

No call below reaches a kernel launch: every one returns from a check, or from the nq == 0 success.  The argument lists are the
hand-written orders of tests/test_search_arg_order.py and tests/test_dense_subset.py.

Where the library differs from a documented order the library's behaviour is what is pinned: rc_dense_bf16x3_scores and
rc_dense_l2_bf16x3_scores have never checked the row pitch (their screen reads any pitch), so an unaligned pitch is accepted
there; and rc_dense_sq8_search_exact / rc_dense_l2_sq8_search_exact read nothing from the workspace with a 16-byte load and do
not check its alignment, so the misaligned workspace is tried on the search_q and scores entries alone.
"""
import ctypes as C

import pytest
import torch

from test_dense_subset import ROWS_ORDER
from test_search_arg_order import FLAT, SCORES

RC_OK, RC_EINVAL, RC_ESHAPE, RC_EWORKSPACE = 0, -1, -2, -4
N, D, NQ, K, NS = 64, 16, 4, 10, 32
POINTERS = ("h", "x", "q", "dec", "xsq", "xnorm_max", "cstat", "rows", "scores", "ids", "status", "qstatus", "out", "ws", "stream")
OPTIONAL = ("qstatus", "ws", "stream")                   # qstatus may be null, the workspace has a code of its own, stream 0 is a stream


def _entries():
    """name -> (kind, argument order); kinds: search_q, search_exact, search_rows_q, search_rows_exact, scores"""
    e = {}
    for _, q_name, q_order, x_name, x_order in FLAT:
        e[q_name] = ("search_q", q_order.split(", "))
        e[x_name] = ("search_exact", x_order.split(", "))
    for _, q_name, q_order, x_name, x_order in ROWS_ORDER:
        e[q_name] = ("search_rows_q", q_order.split(", "))
        e[x_name] = ("search_rows_exact", x_order.split(", "))
    for _, name, order in SCORES:
        e[name] = ("scores", order.split(", "))
    return e


ENTRIES = _entries()
assert {kind: sum(k == kind for k, _ in ENTRIES.values()) for kind in ("search_q", "search_exact", "scores")} == \
    {"search_q": 8, "search_exact": 6, "scores": 7} and len(ENTRIES) == 8 + 6 + 8 + 7
NAMES = sorted(ENTRIES)


def _coded(name):
    return "sq8" in name


def _call(lib, name, values, **over):
    v = dict(values, **over)
    args = [C.c_void_p(v[a]) if a in POINTERS else v[a] for a in ENTRIES[name][1]]
    return getattr(lib, name)(*args)


# ---------------------------------------------------------------------------------------------------------------- CPU
NULLS = dict({p: None for p in POINTERS}, ldx=D, N=N, D=D, nq=NQ, ns=NS, k=K, id_offset=0, sel_slack=3.0, ws_bytes=0)


@pytest.mark.parametrize("name", NAMES)
def test_shape_limits_come_before_the_pointers(name):
    from repconc_amd import _lib
    lib = _lib.load()
    kind, order = ENTRIES[name]
    assert _call(lib, name, NULLS) == RC_EINVAL                                  # fine shapes, no handle, no pointer
    assert _call(lib, name, NULLS, N=1 << 32) == RC_ESHAPE
    assert _call(lib, name, NULLS, N=(1 << 32) - 1) == RC_EINVAL
    if "k" in order:
        assert _call(lib, name, NULLS, k=8193) == RC_ESHAPE
        assert _call(lib, name, NULLS, k=8192) == RC_EINVAL
    # only the int8 screen bounds D
    assert _call(lib, name, NULLS, D=65537, ldx=65537) == (RC_ESHAPE if _coded(name) else RC_EINVAL)
    assert _call(lib, name, NULLS, D=65536, ldx=65536) == RC_EINVAL
    if "ns" in order:                                      # ns outside [1, N]: RC_EINVAL, and only after the shape test
        for ns in (0, -1, N + 1):
            assert _call(lib, name, NULLS, ns=ns) == RC_EINVAL
            assert _call(lib, name, NULLS, ns=ns, N=1 << 32) == RC_ESHAPE
            assert _call(lib, name, NULLS, ns=ns, k=8193) == RC_ESHAPE


# ---------------------------------------------------------------------------------------------------------------- GPU
DEV = "cuda:0"
PITCH = 24                                               # elements between the rows of the pitched store
_state = {}


def _gpu():
    """the library, and per storage type the values of a complete call: real buffers, generated once and never written to"""
    if not _state:
        from repconc_amd import _lib
        lib = _lib.load()
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)
        t = {"q32": z((NQ, D)), "q16": z((NQ, D), torch.float16), "dec": z((2, D)), "xsq": z((N,)), "xnorm_max": z((1,)),
             "cstat": z((2,)), "rows": torch.arange(NS, dtype=torch.int64, device=DEV), "scores": z((NQ, K)),
             "ids": z((NQ, K), torch.int64), "status": z((1,), torch.int32), "qstatus": z((NQ,), torch.int32), "out": z((NQ, N)),
             "x32": z((N, PITCH)), "x16": z((N, PITCH), torch.float16), "x8": z((N, PITCH), torch.int8)}
        values = {}
        for store, xq in (("f32", ("x32", "q32")), ("f16", ("x16", "q16")), ("i8", ("x8", "q32"))):
            values[store] = dict({n: t[n].data_ptr() for n in t if n in POINTERS}, x=t[xq[0]].data_ptr(), q=t[xq[1]].data_ptr(),
                                 h=_lib.handle(0).value, stream=torch.cuda.current_stream(DEV).cuda_stream, ws=None, ws_bytes=0,
                                 ldx=D, N=N, D=D, nq=NQ, ns=NS, k=K, id_offset=0, sel_slack=3.0)
        _state.update(lib=lib, t=t, values=values)
    return _state["lib"], _state["values"]


def _store(name):
    return "i8" if _coded(name) else "f16" if "f16" in name else "f32"


def _ws_bytes(lib, name, nq):
    """what the entry's *_ws_bytes companion asks for; the rows entries size theirs by ns"""
    kind = ENTRIES[name][0]
    if kind == "scores":
        fn = name + "_ws_bytes"
        return getattr(lib, fn)(D, nq) if "ws" in ENTRIES[name][1] else None
    n = NS if "rows" in kind else N
    fn = name.replace("_rows", "").replace("search_q", "search_ws_bytes").replace("search_exact", "search_exact_ws_bytes")
    return getattr(lib, fn)(n, D, nq, K)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_pointers_then_empty_batch_then_workspace(name):
    lib, values = _gpu()
    v = values[_store(name)]
    kind, order = ENTRIES[name]
    # a missing pointer is RC_EINVAL even where there is nothing to do; an empty batch with everything there succeeds without
    # a workspace
    for p in order:
        if p in POINTERS and p not in OPTIONAL:
            assert _call(lib, name, v, nq=0, **{p: None}) == RC_EINVAL, p
            assert _call(lib, name, v, **{p: None}) == RC_EINVAL, p
    assert _call(lib, name, v, nq=0) == RC_OK
    assert _call(lib, name, v, nq=0, qstatus=None) == RC_OK
    assert _call(lib, name, v, nq=-1) == RC_EINVAL
    if "ns" in order:
        for ns in (0, N + 1):
            assert _call(lib, name, v, nq=0, ns=ns) == RC_EINVAL
        assert _call(lib, name, v, nq=0, ns=N) == RC_OK
    # the workspace: missing, one byte short, misaligned
    need = _ws_bytes(lib, name, NQ)
    if need is None:
        return
    assert need > 0
    buf = torch.zeros((need + 16,), dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    assert _call(lib, name, v) == RC_EWORKSPACE
    assert _call(lib, name, v, ws=None, ws_bytes=need) == RC_EWORKSPACE
    assert _call(lib, name, v, ws=buf.data_ptr(), ws_bytes=need - 1) == RC_EWORKSPACE
    assert _call(lib, name, v, ws=buf.data_ptr(), ws_bytes=0) == RC_EWORKSPACE
    if ("bf16x3" in name or _coded(name)) and kind in ("search_q", "scores"):     # planes read with 16-byte loads
        assert _call(lib, name, v, ws=buf.data_ptr() + 8, ws_bytes=need) == RC_EWORKSPACE
    # a pointer is still missed before the workspace is looked at
    assert _call(lib, name, v, ws=buf.data_ptr(), ws_bytes=need - 1, x=None) == RC_EINVAL


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_row_pitch_that_is_not_16_byte_aligned(name):
    """D = 16, rows 17 elements apart, nq = 0: the check comes before the empty batch's success."""
    lib, values = _gpu()
    v = values[_store(name)]
    kind = ENTRIES[name][0]
    # every search over fp32 or fp16 storage reads its rows with 16-byte loads somewhere on its route; of the scores entries
    # only the fp32 L2 screen does; the int8 screen has a form for any pitch on every route
    wants_aligned = (kind != "scores" and not _coded(name)) or name == "rc_dense_l2_scores"
    assert _call(lib, name, v, nq=0, ldx=17) == (RC_EINVAL if wants_aligned else RC_OK)
    assert _call(lib, name, v, nq=0, ldx=PITCH) == RC_OK
    assert _call(lib, name, v, nq=0, ldx=D - 1) == RC_EINVAL                     # a pitch below D is refused everywhere
