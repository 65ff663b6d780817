"""The MSM passes of a multi-row call without a device: the library's planner (kzg_test_msm_passes) is the arithmetic that
commit_open_batch_dev and multi_msms_finish each carried before there was one planner, and every plan it makes puts each scalar
set into exactly one pass, in set order, within what one sort can carry.

(No hook reaches msm_core without a device, so its refusal of a malformed scalar-set description -- no sets, a count without
scalars, more sets than the sort's key carries -- is not tested here.)"""
import ctypes
import itertools

import pytest

from zkp_subnet_amd import _native
from zkp_subnet_amd.build import build
from zkp_subnet_amd.engine import msm_passes_of

MSM_MAX_SETS = 17          # csrc/msm.hip.h
WINDOWS = range(4, 25)     # what kzg_set_window accepts
CASES = [(c, long_rows, k, m) for c in WINDOWS for long_rows in (False, True) for k in range(17) for m in range(5) if k + m]


@pytest.fixture(scope="module")
def lib():
    build()
    return _native.load()


def sort_max_sets(c):
    """msm_sort_max_sets: the sort's key has 24 bits, c - 1 of them the digit."""
    room = 24 - (c - 1)
    return MSM_MAX_SETS if room >= 5 else 1 << room


def parent_arithmetic(c, long_rows, k, m):
    """The `per` computation and the pass loop of multi_msms_finish as they stood before the planner, transcribed line by line
    (commit_open_batch_dev held the same two with m = 1); pass p ran on the second lane when rows were long and p odd."""
    nbuckets = 1 << (c - 1)
    per = min(MSM_MAX_SETS, sort_max_sets(c))
    while per > 2 and per * nbuckets > (1 << 22):
        per -= 1
    if long_rows:
        per = 1
    sets = k + m
    passes = (sets + per - 1) // per
    out = []
    for p in range(passes):
        a, b = p * per, min(sets, p * per + per)
        nr = min(b, k) - min(a, k)
        q0, nq = max(a, k) - k, (b - max(a, k) if b > k else 0)
        out.append((a, nr, q0, nq, p & 1 if long_rows and passes > 1 else 0))
    return out


def test_planner_is_the_arithmetic_it_replaced(lib):
    assert len(CASES) == 21 * 2 * (17 * 5 - 1)
    for c, long_rows, k, m in CASES:
        got = msm_passes_of(c, long_rows, k, m)
        want = parent_arithmetic(c, long_rows, k, m)
        # the parent named a pass by its first SET a (results at res + a); the plan names first row and first tail set
        assert [(r0 + q0, nr, q0, nq, lane) for r0, nr, q0, nq, lane in got] == want, (c, long_rows, k, m)
        assert all(r0 == min(a, k) for (r0, *_), (a, *_) in zip(got, want))
    # shapes the GPU suites run: 17 sets in one pass at c = 16, 20 sets in two; the bucket cap at c = 20 (8 sets) and c = 22 (2)
    assert msm_passes_of(16, False, 16, 1) == [(0, 16, 0, 1, 0)]
    assert msm_passes_of(16, False, 16, 4) == [(0, 16, 0, 1, 0), (16, 0, 1, 3, 0)]
    assert msm_passes_of(20, False, 8, 2) == [(0, 8, 0, 0, 0), (8, 0, 0, 2, 0)]
    assert msm_passes_of(22, False, 3, 3) == [(0, 2, 0, 0, 0), (2, 1, 0, 1, 0), (3, 0, 1, 2, 0)]
    assert msm_passes_of(16, True, 2, 1) == [(0, 1, 0, 0, 0), (1, 1, 0, 0, 1), (2, 0, 0, 1, 0)]


def test_every_plan_holds_each_set_once_in_order_within_one_sort(lib):
    for c, long_rows, k, m in CASES:
        plan = msm_passes_of(c, long_rows, k, m)
        rows = list(itertools.chain.from_iterable(range(r0, r0 + nr) for r0, nr, _, _, _ in plan))
        tails = list(itertools.chain.from_iterable(range(q0, q0 + nq) for _, _, q0, nq, _ in plan))
        assert rows == list(range(k)) and tails == list(range(m)), (c, long_rows, k, m)
        # set order across passes: no pass takes a row once a pass has taken a tail set
        seen_tail = False
        for _, nr, _, nq, _ in plan:
            assert nr + nq >= 1 and not (seen_tail and nr)
            seen_tail = seen_tail or nq > 0
        for p, (_, nr, _, nq, lane) in enumerate(plan):
            assert nr + nq <= min(MSM_MAX_SETS, sort_max_sets(c))
            assert (nr + nq) << (c - 1) <= 1 << 22 or nr + nq <= 2
            assert lane == (p & 1 if long_rows else 0) and (not long_rows or nr + nq == 1)


def test_hook_refuses_what_no_call_can_ask(lib):
    out, n = (ctypes.c_uint32 * 100)(), ctypes.c_int()
    for bad in ((3, 0, 1, 1), (25, 0, 1, 1), (16, 0, 17, 0), (16, 0, 0, 5)):
        assert lib.kzg_test_msm_passes(*bad, out, ctypes.byref(n)) == _native.KZG_E_ARG, bad
    assert lib.kzg_test_msm_passes(16, 0, 1, 1, None, None) == _native.KZG_E_ARG
    assert msm_passes_of(16, False, 0, 0) == []
