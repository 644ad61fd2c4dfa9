"""The fused stage-1 contrastive loss (csrc/contrastive.hip -> rc_contrastive_* -> ops.contrastive_loss ->
RepCONCFinetuneArguments.fused_contrastive_loss): duplicate and false-negative masks from the ids, the dynamic top-k cut, the
log-softmax cross-entropy and its gradient, everything after the similarity GEMM.

The arithmetic is fixed on the output (include/repconc_hip.h, rc_contrastive_*), and `restate` below is its numpy restatement:
fp32 for the logits z (one rounding per subtraction of 10000), a stable sort for the tie rule of the cut (the lower column
wins), float64 for the loss and the gradient before their one rounding to fp32.  The GPU's z must equal it BIT FOR BIT.  The
loss and the gradient go through the GPU's fp64 exp and log, which are not numpy's, so they get the two bands the issue names:
one fp32 ulp (np.spacing) of the yardstick's rounded value, plus for the gradient an absolute 1e-12 * |gout| / nq, the fp64
noise floor of exp and log.  The trainer comparison uses the band tests/test_gpu_parity.py already has for the same comparison
(loss 1e-4, gradients rtol 2e-3 / atol 2e-5).

Chunk sizes of the kernels (csrc/contrastive.hip): a keep word and a wave step are CL_WORD = 64 columns, the duplicate kernel
gives a block CL_DUP_COLS = 64 columns and stages CL_DUP_TILE = 256 earlier ids per step, a block of CL_THREADS = 256 threads
strides the row by 256 with CL_U = 4 loads in flight, i.e. 1024 columns per step, and each of the four waves owns a contiguous
quarter of the row's words.  So nd = 63 / 65, 255 / 257 and 1023 / 1025 sit one less / one more than each of them, next to the
issue's 63, 64, 65, 127, 129 and the prime 12 289.  A row keeps CL_REL_LDS = 64 positives in LDS and reads the rest from global
memory: rows with 63, 65 and 129 positives take both paths.

Magnitudes: N(0, 1) * 1e3 alone never spreads a row over 10 000, and then no column at -10000 has a non-zero exponential.  So
the 1e3 case also has `wide_rows_case`: rows built to spread over more than 10 000 in which masked columns land inside the
softmax's range, asserted on the yardstick before the GPU is compared with it.
"""
import functools
import types
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
MASKED = F32(10000.0)

Case = namedtuple("Case", "sim docids rel_off rel_ids")


# ------------------------------------------------------------------------------------------------------ the yardstick
def restate_logits(case, topk):
    """fp32 z [nq, nd] by steps 1-4 of the contract."""
    sim, docids, rel_off, rel_ids = case
    nq, nd = sim.shape
    seen, dup = set(), np.zeros(nd, bool)
    for j, d in enumerate(docids.tolist()):                           # 1: the later occurrences
        dup[j] = d in seen
        seen.add(d)
    mask = np.zeros((nq, nd), bool)
    for i in range(nq):                                               # 2
        mask[i] = dup | np.isin(docids, rel_ids[rel_off[i]:rel_off[i + 1]])
        mask[i, i] = False
    z1 = np.where(mask, sim - MASKED, sim).astype(F32)                # 3: one fp32 rounding
    if topk <= 0:
        return z1
    diag = np.arange(nq)
    neg = z1.copy()
    neg[diag, diag] = -MASKED
    order = np.argsort(-neg, axis=1, kind="stable")[:, :topk]         # 4: descending, ties to the lower j
    keep = np.zeros((nq, nd), bool)
    np.put_along_axis(keep, order, True, axis=1)
    keep[diag, diag] = True
    return np.where(keep, z1, z1 - MASKED).astype(F32)


def restate(case, topk, gout=None):
    """(z fp32, loss float64, grad float64 | None): loss and gradient BEFORE their final rounding to fp32 (steps 5-6)."""
    z = restate_logits(case, topk)
    nq, nd = z.shape
    diag = np.arange(nq)
    z64 = z.astype(F64)
    mx = z64.max(axis=1)
    e = np.exp(z64 - mx[:, None])
    e_off = e.copy()
    e_off[diag, diag] = 0.0
    off = e_off.sum(axis=1)
    tot = off + e[diag, diag]
    loss_i = (mx + np.log(tot)) - z64[diag, diag]
    acc = 0.0
    for v in loss_i.tolist():                                         # ascending i
        acc = acc + v
    loss = acc / nq
    if gout is None:
        return z, loss, None
    v = e / tot[:, None]
    v[diag, diag] = -(off / tot)                                      # the diagonal without cancellation
    return z, loss, (float(gout) * v) / nq


def kth_differs(case, topk):
    """The topk-th and (topk+1)-th largest of every row of neg differ: the cut has no tie."""
    z1 = restate_logits(case, 0)
    nq, nd = z1.shape
    if topk <= 0 or topk >= nd:
        return True
    neg = z1.copy()
    neg[np.arange(nq), np.arange(nq)] = -MASKED
    s = -np.sort(-neg, axis=1)
    return bool(np.all(s[:, topk - 1] != s[:, topk]))


# ------------------------------------------------------------------------------------------------------ the cases
def _csr(rel):
    off = np.zeros(len(rel) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rel])
    return off, np.array([d for r in rel for d in r], dtype=np.int64)


def make_case(seed, nq, nd, scale=1.0, ids="mixed"):
    """Random sim; ids = "mixed": one query without positives, one with five, a positive that sits at three columns, positives
    on the diagonal (they stay unmasked), and a later duplicate on a row's own diagonal (unmasked for that row only)."""
    rng = np.random.default_rng(seed)
    sim = (rng.standard_normal((nq, nd)) * scale).astype(F32)
    docids = (rng.permutation(16 * nd + 64)[:nd] + 1000).astype(np.int64)
    rel = [[] for _ in range(nq)]
    if ids == "equal":
        docids[:] = 77
        rel = [[77] if i % 2 else [] for i in range(nq)]
    elif ids == "huge":                                               # ids near +-2^62, differing in their low bits only
        docids = np.where(rng.integers(0, 2, nd) == 1, 2 ** 62, -(2 ** 62)).astype(np.int64) + rng.permutation(4 * nd)[:nd]
        if nd >= 4:
            docids[nd - 1] = docids[1]
        rel = [[int(docids[rng.integers(nd)]), int(docids[i]), 2 ** 62 - 1 - i] if i % 3 else [] for i in range(nq)]
    elif nd < 8:
        rel = [[int(docids[i])] + [int(d) for d in docids[nq:nq + 1]] for i in range(nq)]
    else:
        rows = list(range(1, nq)) if nq > 1 else [0]                  # row 0 keeps no positives when there is another row
        c = rng.choice(nd, 3, replace=False)
        docids[c] = docids[c[0]]                                      # one id at three columns ...
        rel[rows[0]].append(int(docids[c[0]]))                        # ... a positive of one row
        if nq > 1:
            i = nq - 1
            docids[i] = docids[rng.integers(0, i)]                    # a later duplicate on row i's diagonal
        five = rows[len(rows) // 2]                                   # five positives; the id 5 is in no column
        rel[five] = rel[five] + [int(d) for d in docids[rng.choice(nd, 4 - len(rel[five]), replace=False)]] + [5]
        for r in rows[::2]:
            if r != five:
                rel[r].append(int(docids[r]))                         # a positive on the diagonal
    off, flat = _csr(rel)
    return Case(sim, docids, off, flat)


def many_positives_case(seed, nq, nd, counts):
    """Rows with more positives than a block keeps in LDS; the matching ones sit at the END of each list.  The last row has
    every column among its positives: its label is its only unmasked column."""
    rng = np.random.default_rng(seed)
    sim = rng.standard_normal((nq, nd)).astype(F32)
    docids = (rng.permutation(8 * nd)[:nd] + 10).astype(np.int64)
    rel = []
    for i in range(nq):
        n = counts[i % len(counts)]
        hit = [int(d) for d in docids[rng.choice(nd, min(3, n), replace=False)]]
        rel.append([-(k + 1) for k in range(n - len(hit))] + hit)
    rel[nq - 1] = [int(d) for d in docids]
    off, flat = _csr(rel)
    return Case(sim, docids, off, flat)


def wide_rows_case(seed, nq, nd):
    """sim at the 1e3 scale with rows whose spread exceeds 10 000, so that columns at -10000 are NOT negligible.  Six columns
    repeat an earlier id (masked for every row) and every row from 2 on has three more positives in the batch.  Rows 0 and 1 are
    plain N(0, 1) * 1e3.  In every later row the unmasked columns, the label included, sit at -6000 +- a few units and the
    masked ones at +4000 +- a few units: after the subtraction they land at -6000 too, inside the softmax's range, and compete
    with the unmasked columns for the places of the cut.  The last row has every id among its positives: its label is its only
    unmasked column, and all the others contribute."""
    assert nq >= 4 and nd >= 63
    rng = np.random.default_rng(seed)
    sim = (rng.standard_normal((nq, nd)) * 1e3).astype(F32)
    docids = (rng.permutation(8 * nd)[:nd] + 10).astype(np.int64)
    late = rng.choice(np.arange(nq + 8, nd), 6, replace=False)
    docids[late] = docids[late - 7]
    rel = [[int(docids[i])] for i in range(nq)]
    for i in range(2, nq):
        rel[i] = rel[i] + [int(d) for d in docids[rng.choice(nd, 3, replace=False)]]
    rel[nq - 1] = [int(d) for d in docids]
    off, flat = _csr(rel)
    case = Case(sim, docids, off, flat)
    masked = restate_logits(case, 0) != sim
    for i in range(2, nq):
        sim[i] = np.where(masked[i], 4000.0, -6000.0) + rng.standard_normal(nd) * 3.0
        sim[i, np.flatnonzero(masked[i])[0]] = 4020.0                 # -5980 after the subtraction: the first place of any cut
    return case, masked


def ties_case():
    """nd = 200, topk = 11.  Row 0: five distinct large values, then twenty columns at exactly 1.0 scattered over the row — six
    of them are kept, the six with the lowest j.  Row 1: only four unmasked columns besides the label, every other column is a
    duplicate with sim 0.0, i.e. neg = -10000 exactly, as is the diagonal's: the cut falls among equal masked values.  Row 2:
    +0.0 and -0.0 straddle the cut (one key).  Row 3: every value equal."""
    nq, nd = 4, 200
    rng = np.random.default_rng(40)
    sim = (-2.0 - rng.random((nq, nd))).astype(F32)
    docids = np.arange(nd, dtype=np.int64) + 500
    big = rng.choice(np.arange(4, nd), 25, replace=False)
    sim[0, big[:5]] = [9.0, 8.0, 7.0, 6.0, 5.0]
    sim[0, big[5:]] = 1.0
    sim[2, big[:5]] = [9.0, 8.0, 7.0, 6.0, 5.0]
    sim[2, big[5:15]] = 0.0
    sim[2, big[15:]] = -0.0
    sim[3, :] = 0.25
    case = Case(sim, docids, np.zeros(nq + 1, np.int64), np.zeros(0, np.int64))
    # row 1 lives in a batch of its own ids: columns 10.. repeat column 9's id
    d2 = docids.copy()
    d2[10:] = d2[9]
    s2 = sim.copy()
    s2[1, 10:] = 0.0
    return case, Case(s2, d2, np.zeros(nq + 1, np.int64), np.zeros(0, np.int64))


SHAPES = ([(1, 1), (1, 2)] + [(nq, nd) for nd in (63, 64, 65, 127, 129) for nq in (1, 5, nd)]
          + [(5, nd) for nd in (255, 257, 1023, 1025)] + [(8, 12289)])


def _topks(nd):
    return sorted({k for k in (0, 1, 11, nd - 1, nd) if 0 <= k <= nd})


# ------------------------------------------------------------------------------------------------------ the composition
def _composition(qrels, topk, temperature=1.0, metric="METRIC_IP", M=48, fused=False):
    """A stand-in for the trainer that carries what compute_contrastive_loss reads, and the trainer class."""
    from repconc_amd.models.repconc.finetune_repconc import RepCONCFinetuner
    stub = SimpleNamespace(qrels=qrels, model=SimpleNamespace(config=SimpleNamespace(similarity_metric=metric, MCQ_M=M)),
                           args=SimpleNamespace(temperature=temperature, dynamic_topk_hard_negative=topk,
                                                fused_contrastive_loss=fused))
    for name in ("_compute_mask_for_false_negative", "_compute_mask_for_duplicate_negative", "_fused_contrastive_loss"):
        setattr(stub, name, types.MethodType(getattr(RepCONCFinetuner, name), stub))
    return functools.partial(RepCONCFinetuner.compute_contrastive_loss, stub)


def _capture_composition_logits(monkeypatch):
    """The logits the composition hands to F.cross_entropy, appended to the returned list."""
    from repconc_amd.models.repconc import finetune_repconc as fr
    seen = []

    def cross_entropy(logits, labels):
        seen.append(logits.detach())
        return torch.nn.functional.cross_entropy(logits, labels)
    monkeypatch.setattr(fr, "F", SimpleNamespace(cross_entropy=cross_entropy))
    return seen


def _qrels(case):
    return {i: case.rel_ids[case.rel_off[i]:case.rel_off[i + 1]].tolist() for i in range(case.sim.shape[0])}


# ------------------------------------------------------------------------------------------------------ CPU tests
def test_yardstick_logits_equal_the_torch_composition_on_cpu(monkeypatch):
    seen = _capture_composition_logits(monkeypatch)
    checked = 0
    for seed, (nq, nd) in enumerate([(1, 1), (1, 2), (5, 65), (17, 129), (8, 300), (40, 40)]):
        for ids in ("mixed", "huge"):
            case = make_case(200 + seed, nq, nd, ids=ids)
            for topk in sorted({0, 1, 11, nd // 2, nd - 1, nd}):
                if not 0 <= topk <= nd:
                    continue
                assert kth_differs(case, topk)                        # a tie-free cut: torch.topk's tie order is not specified
                loss_fn = _composition(_qrels(case), topk)
                # q = sim, d = I: the composition's GEMM returns sim itself (sums of one value and zeros)
                loss = loss_fn(torch.from_numpy(case.sim), torch.eye(nd), torch.arange(nq), torch.from_numpy(case.docids))
                got = seen.pop()
                z, want_loss, _ = restate(case, topk)
                assert got.dtype == torch.float32 and torch.equal(got, torch.from_numpy(z)), (nq, nd, ids, topk)
                assert abs(float(loss) - want_loss) <= 1e-5 * max(1.0, abs(want_loss))
                checked += 1
    assert checked >= 50 and not seen


def test_yardstick_gradient_is_the_float64_autograd_of_its_loss():
    """A self-check of the yardstick alone (it runs none of the feature's code and passes without it): steps 5-6 of `restate`
    against torch's float64 autograd of cross_entropy on the yardstick's own logits."""
    case = make_case(7, 6, 70, scale=3.0)
    z, loss, grad = restate(case, 11, gout=2.5)
    t = torch.from_numpy(z).double().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(t, torch.arange(6))
    (ref * 2.5).backward()
    np.testing.assert_allclose(loss, float(ref.detach()), rtol=1e-13)
    np.testing.assert_allclose(grad, t.grad.numpy(), rtol=1e-7, atol=1e-18)


WIDE = [(6, 129, 0), (6, 129, 11), (6, 129, 60), (5, 1025, 0), (5, 1025, 11)]


def _wide_contributors(case, masked, topk):
    """Per row of the yardstick: the spread of sim, and how many masked columns have exp(z - max) > 0 in float64."""
    z, _, _ = restate(case, topk)
    z64 = z.astype(F64)
    e = np.exp(z64 - z64.max(axis=1)[:, None])
    return case.sim.max(axis=1) - case.sim.min(axis=1), ((e > 0) & masked).sum(axis=1)


def test_wide_rows_put_masked_columns_inside_the_softmax():
    """The magnitude case at 1e3 as the issue states it, checked on the yardstick (no feature code runs here): every planted row
    spreads over more than 10 000 and has masked columns whose exp(z - max) is not zero, without a cut and — the masked columns
    that win a place of the cut — with one.  A column the cut drops can never contribute: some kept negative has a z1 at least
    as large, so the dropped column's z is at least 10 000 below the row maximum and its exponential is exactly 0."""
    for nq, nd, topk in WIDE:
        case, masked = wide_rows_case(70 + nd, nq, nd)
        spread, contributing = _wide_contributors(case, masked, topk)
        assert np.all(spread[2:] > 10000), (nd, topk, spread)
        assert np.all(contributing[2:] >= 1), (nd, topk, contributing)
        assert masked[nq - 1].sum() == nd - 1 and contributing[nq - 1] >= (min(topk, nd - 1) if topk else nd - 1)
        if topk:
            z = restate_logits(case, topk)
            dropped = z < -15000
            assert dropped.any() and np.all(np.exp(z.astype(F64) - z.astype(F64).max(axis=1)[:, None])[dropped] == 0)


def test_workspace_size_needs_no_gpu_and_grows_with_the_keep_bits():
    from repconc_amd import _lib, ops
    lib = _lib.load()
    for name in ("rc_contrastive_ws_bytes", "rc_contrastive_fwd", "rc_contrastive_bwd"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    bits = lambda nq, nd: nq * nd // 8
    for nq, nd in ((512, 6144), (4096, 49152), (64, 8192), (1024, 262144)):
        ws = lib.rc_contrastive_ws_bytes(nq, nd)
        # keep bits + one flag byte per column + four doubles per row, each block rounded up to 256 bytes
        assert bits(nq, nd) <= ws <= bits(nq, nd) + nd + 32 * nq + 3 * 256, (nq, nd)
        assert ops.contrastive_ws_bytes(nq, nd) == ws
    assert lib.rc_contrastive_ws_bytes(4096, 49152) > 7 * lib.rc_contrastive_ws_bytes(512, 49152)
    assert lib.rc_contrastive_ws_bytes(1, 1) > 0 and lib.rc_contrastive_ws_bytes(64, 65) > lib.rc_contrastive_ws_bytes(64, 64)    # a second word
    # outside the contract: nothing to size
    assert lib.rc_contrastive_ws_bytes(0, 5) == 0 and lib.rc_contrastive_ws_bytes(5, 0) == 0
    assert lib.rc_contrastive_ws_bytes(6, 5) == 0                     # nq > nd
    assert lib.rc_contrastive_ws_bytes(1, 262145) == 0                # the all-pairs duplicate kernel's limit


def test_op_rejects_cpu_tensors_loudly():
    from repconc_amd import _lib, ops
    case = make_case(1, 3, 9)
    with pytest.raises(_lib.RepconcHipError):
        ops.contrastive_loss(*(torch.from_numpy(a) for a in case), topk=2)


def test_trainer_names_its_argument_when_the_cut_exceeds_the_batch():
    loss_fn = _composition({0: [1], 1: [2]}, 9, fused=True)
    with pytest.raises(ValueError, match="dynamic_topk_hard_negative"):
        loss_fn(torch.zeros(2, 4), torch.zeros(8, 4), torch.arange(2), torch.arange(8))


def test_trainer_argument_defaults_to_the_composition():
    import dataclasses
    from repconc_amd.models.repconc.finetune_repconc import RepCONCFinetuneArguments
    f = {x.name: x for x in dataclasses.fields(RepCONCFinetuneArguments)}["fused_contrastive_loss"]
    assert f.type in (bool, "bool") and f.default is False


# ------------------------------------------------------------------------------------------------------ GPU tests
def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)                  # a copy: the shared cases stay as they are


def _run(case, topk, gout=None):
    """(z, loss, grad | None) as CPU numpy arrays from ops.contrastive_loss."""
    from repconc_amd import ops
    sim = _t(case.sim).requires_grad_(gout is not None)
    loss, z = ops.contrastive_loss(sim, _t(case.docids), _t(case.rel_off), _t(case.rel_ids), topk, return_logits=True)
    grad = None
    if gout is not None:
        (loss * float(gout)).backward()
        grad = sim.grad.cpu().numpy()
    assert loss.dtype == torch.float32 and loss.dim() == 0 and z.dtype == torch.float32 and not z.requires_grad
    return z.detach().cpu().numpy(), loss.detach().cpu().numpy(), grad


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_loss_and_grad(case, topk, gout, tag):
    z, loss, grad = _run(case, topk, gout)
    wz, wloss, wgrad = restate(case, topk, gout)
    nq = case.sim.shape[0]
    assert _same_bits(z, wz), tag
    l32 = F32(wloss)
    assert abs(F64(loss) - F64(l32)) <= np.spacing(np.abs(l32)), (tag, float(loss), wloss)
    g32 = wgrad.astype(F32)
    err = np.abs(grad.astype(F64) - g32.astype(F64))
    band = np.spacing(np.abs(g32)).astype(F64) + 1e-12 * abs(gout) / nq
    assert np.all(err <= band), (tag, float((err - band).max()))
    if case.sim.shape[1] >= 63:                                       # (1, 2) can have its one negative masked: a zero gradient
        assert np.any(grad != 0)


@gpu
@pytest.mark.parametrize("nq,nd", SHAPES, ids=lambda v: str(v))
def test_logits_equal_the_yardstick_bit_for_bit(nq, nd):
    case = make_case(1000 + nq * 7 + nd, nq, nd)
    for topk in _topks(nd):
        z, _, _ = _run(case, topk)
        assert _same_bits(z, restate_logits(case, topk)), (nq, nd, topk)


@gpu
@pytest.mark.parametrize("ids", ["equal", "huge"])
def test_logits_on_equal_and_on_huge_ids(ids):
    for nq, nd in ((1, 2), (5, 65), (129, 129), (7, 257)):
        case = make_case(50 + nd, nq, nd, ids=ids)
        for topk in _topks(nd):                                       # "equal": 11 is above the number of unmasked columns
            z, _, _ = _run(case, topk)
            assert _same_bits(z, restate_logits(case, topk)), (ids, nq, nd, topk)


@gpu
def test_rows_with_more_positives_than_the_block_stages():
    case = many_positives_case(3, 6, 129, counts=(63, 64, 65, 129, 0))
    want_unmasked = restate_logits(case, 0)[5] > -5000
    assert want_unmasked.sum() == 1 and want_unmasked[5]             # the last row: the label alone is unmasked
    for topk in (0, 1, 11, 128, 129):                                 # 11 is above the last row's unmasked columns
        z, _, _ = _run(case, topk)
        assert _same_bits(z, restate_logits(case, topk)), topk
    for gout in (1.0, 65536.0):
        _check_loss_and_grad(case, 11, gout, ("many", gout))


@gpu
def test_ties_at_the_cut_go_to_the_lower_column():
    plain, masked = ties_case()
    for case in (plain, masked):
        for topk in (11, 1, 5, 12, 150, 199):
            z, _, _ = _run(case, topk)
            assert _same_bits(z, restate_logits(case, topk)), topk
    # the yardstick's own answer on row 0: of the twenty columns at 1.0 the six lowest are kept
    z = restate_logits(plain, 11)
    ones = np.flatnonzero(plain.sim[0] == 1.0)
    assert len(ones) == 20 and np.all(z[0, ones[:6]] == 1.0) and np.all(z[0, ones[6:]] == F32(1.0) - MASKED)
    # ... and on the masked batch's row 1: columns 10.. are duplicates at -10000, as is the diagonal's neg; the 9 unmasked
    # negatives (0, 2..9 — column 1 is the label) leave 2 places for the lowest of the equal keys: j = 1 (the diagonal) and 10
    z = restate_logits(masked, 11)
    assert z[1, 10] == -MASKED and np.all(z[1, 11:] == -MASKED - MASKED)
    _check_loss_and_grad(plain, 11, 1.0, "ties")


@gpu
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_loss_and_gradient_within_one_ulp_of_the_yardstick(scale):
    for nq, nd, topk in ((1, 1, 0), (1, 2, 1), (5, 65, 11), (129, 129, 11), (5, 1025, 0), (5, 1025, 11), (8, 12289, 11)):
        case = make_case(2000 + nd, nq, nd, scale=scale)
        for gout in (1.0, 65536.0):
            _check_loss_and_grad(case, topk, gout, (scale, nq, nd, topk, gout))


@gpu
@pytest.mark.parametrize("nq,nd,topk", WIDE)
def test_loss_and_gradient_when_masked_columns_are_not_negligible(nq, nd, topk):
    """sim at the 1e3 scale, rows spreading over more than 10 000: columns at -10000 carry weight in the sum, in `off` and in
    the gradient (test_wide_rows_put_masked_columns_inside_the_softmax shows it on the yardstick; asserted again here)."""
    case, masked = wide_rows_case(70 + nd, nq, nd)
    spread, contributing = _wide_contributors(case, masked, topk)
    assert np.all(spread[2:] > 10000) and np.all(contributing[2:] >= 1)
    for gout in (1.0, 65536.0):
        _check_loss_and_grad(case, topk, gout, ("wide", nq, nd, topk, gout))
    _, _, grad = _run(case, topk, 1.0)
    assert np.all((np.abs(grad) * masked).sum(axis=1)[2:] > 0)        # the GPU's gradient reaches masked columns too


@gpu
def test_loss_and_gradient_repeat_bit_for_bit():
    from repconc_amd import ops
    case = make_case(9, 64, 4099, scale=4.0)
    args = [_t(a) for a in case]
    outs = []
    for _ in range(2):
        sim = args[0].clone().requires_grad_(True)
        loss = ops.contrastive_loss(sim, *args[1:], topk=11)
        (loss * 65536.0).backward()
        outs.append((loss.detach().clone(), sim.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert torch.isfinite(outs[0][0]) and float(outs[0][1].abs().sum()) > 0


@gpu
def test_op_and_entry_refuse_what_the_contract_excludes():
    from repconc_amd import _lib, ops
    case = make_case(2, 4, 70)
    sim, docids, off, rel = (_t(a) for a in case)
    for bad in ((sim.double(), docids, off, rel), (sim, docids.int(), off, rel), (sim, docids[:-1], off, rel),
                (sim, docids, off[:-1], rel), (sim.t().contiguous(), docids[:4], torch.zeros(71, dtype=torch.int64, device=DEV), rel)):
        with pytest.raises(ValueError):
            ops.contrastive_loss(*bad)
    with pytest.raises(ValueError):
        ops.contrastive_loss(sim, docids, off, rel, topk=71)
    lib, h, s, _ = ops._ctx(sim)
    loss = torch.zeros((), device=DEV)
    wsb = lib.rc_contrastive_ws_bytes(4, 70)
    ws = torch.zeros(wsb, dtype=torch.uint8, device=DEV)
    call = lambda nq=4, nd=70, topk=3, w=ws, wb=wsb: lib.rc_contrastive_fwd(
        h, ops._p(sim), ops._p(docids), ops._p(off), ops._p(rel), rel.numel(), nq, nd, topk, ops._p(loss), ops._p(None), ops._p(w), wb, s)
    assert call() == _lib.RC_OK
    assert call(wb=wsb - 1) == _lib.RC_EWORKSPACE and call(w=None) == _lib.RC_EWORKSPACE
    assert call(topk=71) == _lib.RC_EINVAL and call(topk=-1) == _lib.RC_EINVAL and call(nq=0) == _lib.RC_EINVAL
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ against the composition
def _embedding_batch(seed, nq, nd, D):
    """Unit-scale embeddings whose GEMM has no tie at the cut, with a duplicate and a false negative among the ids."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((nq, D)).astype(F32)
    d = rng.standard_normal((nd, D)).astype(F32)
    docids = np.arange(nd, dtype=np.int64) + 1000
    docids[nd - 3] = docids[2]
    qrels = {i: [1000 + i] for i in range(nq)}
    qrels[1].append(int(docids[nd - 5]))
    qrels[nq - 1] = []
    return q, d, docids, qrels


@gpu
@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "fp16-autocast"])
@pytest.mark.parametrize("setting", ["plain", "cos-m48-t0.5"])
def test_trainer_paths_give_the_same_logits_bits(monkeypatch, autocast, setting):
    """compute_contrastive_loss with and without fused_contrastive_loss: the similarity, / MCQ_M and / temperature are the same
    torch ops on both sides, so the logits must agree in every bit wherever the cut has no tie."""
    from repconc_amd import ops
    seen = _capture_composition_logits(monkeypatch)
    fused_z = []
    real = ops.contrastive_loss

    def spy(sim, docids, rel_off, rel_ids, topk=0, return_logits=False):
        assert sim.dtype == torch.float32
        loss, z = real(sim, docids, rel_off, rel_ids, topk, return_logits=True)
        fused_z.append(z)
        return loss
    monkeypatch.setattr(ops, "contrastive_loss", spy)
    kw = dict(temperature=0.5, metric="METRIC_CENTROID_COS", M=48) if setting != "plain" else {}
    topk, nq, nd = 11, 24, 200
    ctx = (lambda: torch.autocast("cuda", dtype=torch.float16)) if autocast else (lambda: torch.autocast("cuda", enabled=False))
    found = 0
    for seed in range(8):                                             # fp16 similarities can tie: take batches whose cut is tie-free
        q, d, docids, qrels = _embedding_batch(300 + seed, nq, nd, 64)
        tq, td, tids, qids = _t(q), _t(d), _t(docids), torch.arange(nq, device=DEV)
        with ctx():                                                   # the similarity as both paths compute it
            sim = tq @ td.T
            if kw:
                sim = sim / 48 / 0.5
        case = Case(sim.float().cpu().numpy(), docids, *_csr([qrels[i] for i in range(nq)]))
        if not kth_differs(case, topk):
            continue
        with ctx():
            want_loss = _composition(qrels, topk, **kw)(tq, td, qids, tids)
            got_loss = _composition(qrels, topk, fused=True, **kw)(tq, td, qids, tids)
        want, got = seen.pop(), fused_z.pop()
        assert want.dtype == torch.float32 and torch.equal(got, want), (setting, autocast, seed)
        assert _same_bits(got.cpu().numpy(), restate_logits(case, topk))
        assert abs(float(got_loss) - float(want_loss)) <= 1e-5 * max(1.0, abs(float(want_loss)))
        found += 1
        if found == 2:
            break
    assert found == 2


@gpu
def test_fused_path_allocates_no_mask_sized_tensor():
    """nq = 64, nd = 8192: S = nq * nd * 4 = 2 MiB.  Forward + backward to grad_q and grad_d through the fused path may raise the
    peak by 3 S + 1 MiB (sim, its gradient, one spare full-size buffer, the keep bits at S / 32, the per-row vectors); the
    composition's duplicate compare alone is nd^2 = 64 MiB."""
    nq, nd, D = 64, 8192, 32
    q, d, docids, qrels = _embedding_batch(5, nq, nd, D)
    tq, td = _t(q).requires_grad_(True), _t(d).requires_grad_(True)
    tids, qids = _t(docids), torch.arange(nq, device=DEV)
    S = nq * nd * 4

    def rise(fused):
        loss_fn = _composition(qrels, 11, fused=fused)
        peak = 0
        for measured in (False, True):                               # once to warm the GEMM's workspace up, then measured
            tq.grad = td.grad = None
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            loss = loss_fn(tq, td, qids, tids)
            loss.backward()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            assert tq.grad is not None and td.grad is not None and torch.isfinite(loss)
            del loss
        return peak
    fused, composed = rise(True), rise(False)
    print(f"peak rise: fused {fused / 2 ** 20:.2f} MiB, composition {composed / 2 ** 20:.2f} MiB (S = {S / 2 ** 20:.0f} MiB)")
    assert fused <= 3 * S + 2 ** 20, fused
    assert composed > nd * nd, composed


# ------------------------------------------------------------------------------------------------------ the trainer
class _PtHashTokenizer:
    """Whitespace tokenizer over a 500-word vocabulary (ids by hash); pads to the longest text of the batch."""
    sep_token = "[SEP]"

    def __call__(self, texts, padding=True, truncation=True, max_length=32, return_tensors=None, **_unused):
        import zlib
        rows = [[1] + [3 + (zlib.crc32(w.encode()) % 490) for w in t.split()][: max_length - 2] + [2] for t in texts]
        L = max(map(len, rows))
        enc = {"input_ids": [r + [0] * (L - len(r)) for r in rows], "attention_mask": [[1] * len(r) + [0] * (L - len(r)) for r in rows]}
        return {k: torch.tensor(v, dtype=torch.long) for k, v in enc.items()} if return_tensors == "pt" else enc


@gpu
def test_finetuner_step_with_the_fused_loss(tmp_path):
    """The batch of test_repconc_finetuner_on_transformers5_gradients_and_train_loop (a duplicate and a false negative among
    its ids), dropout 0, dynamic_topk_hard_negative = 7: one training_step with the composition, one with the fused loss."""
    from transformers import BertConfig
    from repconc_amd.models.dense import BertDense
    from repconc_amd.models.repconc import RepCONC
    from repconc_amd.models.repconc.finetune_repconc import FinetuneCollator, RepCONCFinetuneArguments, RepCONCFinetuner
    torch.manual_seed(0)
    random_state = np.random.default_rng(3)
    cfg = BertConfig(hidden_size=768, num_hidden_layers=1, num_attention_heads=12, intermediate_size=128, vocab_size=500,
                     max_position_embeddings=40, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    cfg.MCQ_M, cfg.MCQ_K, cfg.similarity_metric, cfg.pooling = 48, 256, "METRIC_IP", "mean"
    model = RepCONC(cfg, BertDense(cfg), True, 0.003, 20).to(DEV)
    with torch.no_grad():
        model.centroids.mul_(0.05)
    words = [f"w{i}" for i in range(200)]
    text = lambda lo, hi: " ".join(random_state.choice(words, random_state.integers(lo, hi)))
    nq, npq = 16, 3
    feats = [{"query": text(2, 6), "pos_doc": text(5, 20), "qid": i, "pos_docid": 1000 + i,
              "neg_docs": [text(5, 20) for _ in range(npq)], "neg_docids": [2000 + npq * i + j for j in range(npq)]}
             for i in range(nq)]
    feats[5]["neg_docids"][0] = feats[3]["pos_docid"]                 # a duplicate ...
    qrels = {i: [1000 + i] for i in range(nq)}
    qrels[2].append(feats[7]["neg_docids"][1])                        # ... and a false negative
    args = RepCONCFinetuneArguments(output_dir=str(tmp_path / "o"), per_device_train_batch_size=nq, cache_chunk_size=6,
                                    mse_loss_weight=1e-2, dynamic_topk_hard_negative=7, centroid_learning_rate=5e-4,
                                    learning_rate=2e-5, max_steps=2, logging_steps=1, save_strategy="no", report_to=[],
                                    dataloader_drop_last=True, seed=2022)
    assert args.fused_contrastive_loss is False
    trainer = RepCONCFinetuner(qrels=qrels, model=model, args=args, train_dataset=feats,
                               data_collator=FinetuneCollator(_PtHashTokenizer(), 8, 24))
    batch = trainer.data_collator(feats)

    def step():
        model.zero_grad()
        loss = trainer.training_step(model, batch)
        return float(loss), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    want_loss, want = step()
    trainer.args.fused_contrastive_loss = True
    got_loss, got = step()
    assert np.isfinite(got_loss) and abs(got_loss - want_loss) < 1e-4
    assert set(got) == set(want) and float(got["centroids"].abs().sum()) > 0
    for name, grad in got.items():
        assert torch.allclose(grad, want[name], rtol=2e-3, atol=2e-5), name
    # with the deterministic decode backward the centroid gradient of a step repeats bit for bit
    model.deterministic_decode = True
    _, first = step()
    _, second = step()
    assert torch.equal(first["centroids"], second["centroids"])
