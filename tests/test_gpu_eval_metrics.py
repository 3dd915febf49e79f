"""``ddpx_eval_metrics`` (``csrc/kernels/eval_metrics.hip``) against the numpy fp64 reference of ``tests/_eval_ref.py``.

Counts are exact.  The loss sum's bound is ``1e-5 * max(m_valid, 1)``: per row with ``|z| <= 8`` the exponent's
argument carries at most 16 u ~ 1e-6 relative error into each ``exp``, ``__expf`` / ``__logf`` add a few ulp, so a
row is off by a few 1e-6, and the rows are summed in fp64.
"""
import numpy as np
import pytest
import torch

from ddpx.ops.head import EvalAccumulator, accuracy_count, eval_metrics
from ddpx.runtime import native
from tests._eval_ref import gaussian_logits, grid_logits, ref_metrics, ties_at_k

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 10, 1), (17, 10, 5), (64, 16, 16), (65, 17, 5), (33, 100, 5), (16, 128, 128), (5, 130, 3)]
LOSS_TOL = 1e-5


def _logits(kind, M, C):
    return (gaussian_logits if kind == "gaussian" else grid_logits)(M, C, seed=M * 1000 + C)


def _run(dev, z, t, k, m_valid=None, acc=None):
    acc = acc if acc is not None else EvalAccumulator(dev)
    eval_metrics(torch.from_numpy(z).to(dev), torch.from_numpy(t).to(dev), acc, k, m_valid)
    return acc


def _check(acc, z, t, k, m_valid=None):
    loss, h1, hk, rows, _ = ref_metrics(z, t, k, m_valid)
    got = acc.read()
    assert got[1:] == (h1, hk, rows), (got, (h1, hk, rows))
    assert abs(got[0] - loss) <= LOSS_TOL * max(rows, 1), (got[0], loss, rows)
    assert int(acc.counts[3].item()) == 0  # reserved
    return got


@pytest.mark.parametrize("kind", ["gaussian", "grid"])
@pytest.mark.parametrize("M,C,k", SHAPES)
def test_counts_and_loss(gpu, M, C, k, kind):
    z, t = _logits(kind, M, C)
    got = _check(_run(gpu, z, t, k), z, t, k)
    # top-1 is ddpx_accuracy's count on the same tensors
    correct = torch.zeros((), dtype=torch.int32, device=gpu)
    accuracy_count(torch.from_numpy(z).to(gpu), torch.from_numpy(t).to(gpu), correct)
    assert int(correct.item()) == got[1]
    # the same bits on a second run
    again = _run(gpu, z, t, k)
    assert torch.equal(again.loss_sum, _run(gpu, z, t, k).loss_sum) and again.read() == got


def test_the_grid_logits_put_ties_at_the_k_boundary():
    # (the reference itself: the tie rule decides top-k hits in the cases above)
    n = {(M, C, k): ties_at_k(*_logits("grid", M, C), k) for M, C, k in SHAPES}
    # both work layouts (C <= 16 and above); k = C leaves no boundary, and the shapes of a few rows may have none
    assert n[(17, 10, 5)] > 0 and n[(65, 17, 5)] > 0 and n[(33, 100, 5)] > 0, n
    assert all(ties_at_k(*(a[:19] for a in _logits("grid", 32, C)), k) > 0 for C, k in [(10, 5), (100, 5)])


@pytest.mark.parametrize("kind", ["gaussian", "grid"])
@pytest.mark.parametrize("C,k", [(10, 3), (100, 5)])
def test_row_stride_wider_than_the_classes(gpu, C, k, kind):
    M, ld = 37, C + 7
    z, t = _logits(kind, M, C)
    wide = torch.full((M, ld), float("nan"), device=gpu)
    wide[:, :C] = torch.from_numpy(z).to(gpu)
    acc = EvalAccumulator(gpu)
    eval_metrics(wide[:, :C], torch.from_numpy(t).to(gpu), acc, k)
    assert wide[:, :C].stride(0) == ld
    _check(acc, z, t, k)


@pytest.mark.parametrize("kind", ["gaussian", "grid"])
@pytest.mark.parametrize("C,k", [(10, 5), (100, 5)])
@pytest.mark.parametrize("m_valid", [0, 1, 19, 32])
def test_rows_past_m_valid_change_nothing(gpu, m_valid, C, k, kind):
    z, t = _logits(kind, 32, C)
    zp, tp = z.copy(), t.copy()
    zp[m_valid:] = np.nan  # poisoned logits and out-of-range targets in the padding
    tp[m_valid:] = C + 5
    _check(_run(gpu, zp, tp, k, m_valid), z, t, k, m_valid)


@pytest.mark.parametrize("C,k", [(16, 4), (100, 5)])
def test_three_launches_accumulate(gpu, C, k):
    parts = [grid_logits(33, C, seed=1), gaussian_logits(64, C, seed=2), grid_logits(5, C, seed=3)]
    acc = EvalAccumulator(gpu)
    for z, t in parts:
        _run(gpu, z, t, k, acc=acc)
    _check(acc, np.concatenate([z for z, _ in parts]), np.concatenate([t for _, t in parts]), k)
    acc.zero_()
    assert acc.read() == (0.0, 0, 0, 0)


@pytest.mark.parametrize("C,k", [(10, 5), (100, 5)])
@pytest.mark.parametrize("bad", [-1, 10_000, 2 ** 40])
def test_out_of_range_target_is_a_miss_with_no_loss(gpu, C, k, bad):
    z, t = gaussian_logits(21, C, seed=9)
    z[7] = 8.0  # every class ties: the row would count under any in-range target
    t[7] = bad
    got = _check(_run(gpu, z, t, k), z, t, k)
    keep = np.arange(21) != 7
    loss, h1, hk, _, _ = ref_metrics(z[keep], t[keep], k)
    assert got[1:] == (h1, hk, 21) and abs(got[0] - loss) <= LOSS_TOL * 20


def test_non_finite_logits_do_not_fault(gpu):
    z, t = gaussian_logits(20, 100, seed=4)
    z[3, 5], z[4, :], z[6, 2] = np.nan, -np.inf, np.inf
    acc = _run(gpu, z, t, 5)
    torch.cuda.synchronize()
    assert acc.read()[3] == 20


def test_bad_arguments_return_negative_codes_and_launch_nothing(gpu):
    lib = native.kernels()
    M, C = 8, 10
    z = torch.zeros(M, C, device=gpu)
    t = torch.zeros(M, dtype=torch.int64, device=gpu)
    acc = EvalAccumulator(gpu)
    scratch = torch.empty(int(lib.ddpx_eval_metrics_scratch(M)), device=gpu)
    tickets = torch.zeros(int(lib.ddpx_eval_metrics_tickets(M)), dtype=torch.int32, device=gpu)
    good = dict(ld=C, M=M, mv=M, C=C, k=1, counts=acc.counts.data_ptr(), loss=acc.loss_sum.data_ptr(),
                scratch=scratch.data_ptr(), tickets=tickets.data_ptr())

    def call(**kw):
        a = dict(good, **kw)
        return lib.ddpx_eval_metrics(z.data_ptr(), a["ld"], t.data_ptr(), a["M"], a["mv"], a["C"], a["k"], a["counts"],
                                     a["loss"], a["scratch"], a["tickets"], native.stream_handle())

    for kw in (dict(k=C + 1), dict(k=0), dict(mv=M + 1), dict(mv=-1), dict(counts=None), dict(loss=None),
               dict(scratch=None), dict(tickets=None), dict(C=0), dict(ld=C - 1)):
        assert call(**kw) < 0, kw
    torch.cuda.synchronize()
    assert acc.read() == (0.0, 0, 0, 0) and int(tickets.sum().item()) == 0
    assert call() == 0
    assert acc.read()[3] == M
    with pytest.raises(ValueError):
        eval_metrics(z, t, acc, C + 1)
