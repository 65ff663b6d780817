"""GPU tests (`-m gpu`) of the recurrence scan of csrc/fr_recur.hip through kzg_test_recur_run alone: no SRS, no MSM, n <= 2^12.
Caller plans (l0, top_max) reach every geometry of the ladder at small sizes -- the top kernel alone, one level under it, three
levels, every level-0 chunk, ragged last chunks at every level, a top level of one map -- and every plan is compared with the
definition in Python integers (tests/recur_ref.py) on all n values and on the closing value, bit for bit."""
import functools
import random

import pytest

from tests import recur_ref as rref
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu

TOP_ONLY = [(n, 2, 2048) for n in (1, 2, 5, 255, 256, 257, 2048)]
ONE_UNDER = [(4096, 2, 2048), (4096, 3, 1024), (4096, 4, 256), (2049, 2, 2048), (17, 4, 16)]
THREE_LEVELS = [(4096, 2, 16)]
EACH_L0 = [(4096, 3, 16), (4096, 4, 16)]
RAGGED = ([(4097 - k, 2, 16) for k in range(1, 6)] + [(4097 - k, 3, 7) for k in (1, 2, 9)] + [(4097 - k, 4, 3) for k in (1, 17)]
          + [((16 << l0) * m + d, l0, 16) for l0 in (2, 3, 4) for m in (1, 4) for d in (-1, 1)])
TOP_ONE = [(4096, 2, 1), (5, 2, 1), (1, 3, 1), (16, 4, 1), (17, 4, 1)]
LIBRARY = [(1, -1, -1), (2048, -1, -1), (4096, -1, -1), (4095, -1, -1)]
PLANS = TOP_ONLY + ONE_UNDER + THREE_LEVELS + EACH_L0 + RAGGED + TOP_ONE + LIBRARY
FAMILIES = ["random", "all r - 1", "zero A", "zero B", "A = 1", "boundary zeros"]


@pytest.fixture(scope="module")
def eng(hip):
    return hip()


@functools.lru_cache(maxsize=None)
def instance(family, n, l0):
    """(a, b, start, v[0 .. n]) -- computed once per case and shared"""
    rnd = random.Random(hash((FAMILIES.index(family), n)) & 0xffffffff)
    a = [rnd.randrange(R) for _ in range(n)]
    b = [rnd.randrange(R) for _ in range(n)]
    start = rnd.randrange(R)
    if family == "all r - 1":
        a, b, start = [R - 1] * n, [R - 1] * n, R - 1
    elif family == "zero A":
        a = [0] * n
    elif family == "zero B":
        b, start = [0] * n, rnd.randrange(1, R)
    elif family == "A = 1":
        a, start = [1] * n, 0
    elif family == "boundary zeros":
        # a restart on the first and on the last map of level-0 chunks and of 16-chunk groups, and on the very last map
        c = 1 << max(l0, 2)
        for t in range(n):
            if t % (16 * c) in (0, 16 * c - 1) or (t // c) % 3 == 1 and t % c in (0, c - 1):
                a[t] = 0
        a[n - 1] = 0 if n % 2 else a[n - 1]
    return a, b, start, rref.scan(a, b, start)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n,l0,top_max", PLANS)
def test_plan_against_the_reference(eng, n, l0, top_max, family):
    a, b, start, v = instance(family, n, l0)
    got_v, got_cl = eng.test_recur_run(row_bytes(a), row_bytes(b), be(start), n, (l0, top_max))
    assert got_cl == be(v[n])
    if got_v != row_bytes(v[:n]):
        bad = [t for t in range(n) if got_v[32 * t:32 * t + 32] != be(v[t])]
        raise AssertionError(f"{len(bad)} of {n} values differ, the first at {bad[0]}")


def test_the_plans_reach_every_geometry():
    """the claim of the list above, from the plan function itself (host only)"""
    from zkp_subnet_amd.engine import recur_plan_of
    ks = {(n, l0, tm): recur_plan_of(n, l0, tm) for n, l0, tm in PLANS}
    assert all(ks[p]["K"] == 0 for p in TOP_ONLY) and all(ks[p]["K"] == 1 for p in ONE_UNDER)
    assert ks[(4096, 2, 16)]["K"] == 3 and ks[(4096, 2, 16)]["n"] == [4096, 1024, 64, 4]
    assert ks[(4096, 3, 16)]["n"] == [4096, 512, 32, 2] and ks[(4096, 4, 16)]["n"] == [4096, 256, 16]
    assert ks[(4096, 2, 1)]["n"] == [4096, 1024, 64, 4, 1] and ks[(5, 2, 1)]["n"] == [5, 2, 1]
    assert any(pl["n"][k] % (1 << pl["l"][k]) for pl in ks.values() for k in range(pl["K"]) if k >= 1)   # ragged above level 0
    assert ks[(4096, -1, -1)]["K"] == 1 and ks[(1, -1, -1)]["K"] == 0


def test_start_values_and_a_refused_plan_leave_the_context_serving(eng):
    n = 300
    a, b, _, _ = instance("random", n, 2)
    for start in (0, 1, R - 1):
        v = rref.scan(a, b, start)
        got_v, got_cl = eng.test_recur_run(row_bytes(a), row_bytes(b), be(start), n, (2, 16))
        assert got_v == row_bytes(v[:n]) and got_cl == be(v[n])
    arg_error(lambda: eng.test_recur_run(row_bytes(a), row_bytes(b), be(0), n, (5, 16)), "level-0 chunk")
    arg_error(lambda: eng.test_recur_run(row_bytes(a), row_bytes(b), be(0), n, (2, 4096)), "1 .. 2048")
    arg_error(lambda: eng.test_recur_run(row_bytes(a), row_bytes(b), R.to_bytes(32, "big"), n, (2, 16)), "canonical")
    bad = row_bytes(a[:7]) + R.to_bytes(32, "big") + row_bytes(a[8:])           # (be() reduces: r itself goes in as raw bytes)
    arg_error(lambda: eng.test_recur_run(bad, row_bytes(b), be(0), n, (2, 16)), code=_native.KZG_E_SCALAR)
    v = rref.scan(a, b, 5)
    assert eng.test_recur_run(row_bytes(a), row_bytes(b), be(5), n) == (row_bytes(v[:n]), be(v[n]))
