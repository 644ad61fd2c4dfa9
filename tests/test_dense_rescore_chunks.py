"""The rescoring kernel of the screened dense searches (csrc/dense_screen.h, dense_rescore_kernel) stages the query in LDS in
chunks of 1024 values; every other dense GPU shape has D <= 1024 and runs that loop once.  D = 1032: a second chunk of exactly
one 8-wide step on the 16-byte loads; D = 1027: a second chunk on the element-by-element path, behind the padded screen."""
import numpy as np
import pytest

from test_dense_flat import _randn, assert_matches, oracle_topk


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1032, 1027])
@pytest.mark.parametrize("variant", ["f16", "bf16x3"])
def test_screened_search_rescoring_walks_a_second_query_chunk(variant, D):
    from repconc_amd import ops
    N, nq, k = 200000, 3, 10
    x = _randn((N, D), 3000 + D) * 1.0003
    q = _randn((nq, D), 4000 + D) * 1.0003
    if variant == "f16":
        x16 = x.half()
        x, q = x16.float(), q.half().float()                    # the rounded values: what the fp16 search scores
        pending = ops.dense_search_f16(x16, q, k, defer=True)
    else:
        pending = ops.dense_search_bf16x3(x, q, k, defer=True)
    got = pending.result()
    assert_matches(got, oracle_topk(x, q, k))
    ref = ops.dense_search(x, q, k)
    assert bool((got[1] == ref[1]).all())
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), ref[0].cpu().numpy().view(np.uint32))
    # the fast route, and with it the rescoring, produced the answer
    assert pending.stats["exact_queries"] == 0, pending.stats
