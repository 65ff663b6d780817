"""GPU tests (`-m gpu`) of the product scan of csrc/fr_prod.hip, the batched inversion behind it and the additive scan of
csrc/fr_lookup.hip through kzg_test_scan_run alone: no SRS, no MSM, n <= 2^12 + 1.  Caller plans (l0, top_max) reach every geometry
of the ladder at small sizes -- a top level that leaves lanes idle or gives them unequal shares, two to four levels, every level-0
chunk, ragged last chunks at every level, a top level of one value -- and every plan is run in every form (0 product, 1 chained
product, 2 1 / a into W, 3 b / a into P, 4 sum) and compared with the definition in Python integers (tests/scan_ref.py) on all n
values, the closing value and the zero-denominator flag, bit for bit."""
import functools
import random

import pytest

from tests import scan_ref as sref
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu

# one level under the top; the top m = 1, 1, 2, 64, 64, 65, 256, 257, 512, 513, 1024, 1025 values for 256 lanes
ONE_UNDER = [(n, 2, 2048) for n in (1, 2, 5, 255, 256, 257, 1023, 1025, 2048, 2049, 4096, 4097)]
DEEP = [(4096, 2, 16), (4096, 3, 16), (4096, 4, 16), (4096, 2, 1)]
RAGGED = ([(4097 - k, 2, 16) for k in range(0, 6)] + [(4097 - k, 3, 7) for k in (1, 2, 9)] + [(4097 - k, 4, 3) for k in (1, 17)]
          + [((16 << l0) * m + d, l0, 16) for l0 in (2, 3, 4) for m in (1, 4) for d in (-1, 1)])
TOP_ONE = [(5, 2, 1), (1, 3, 1), (16, 4, 1), (17, 4, 1)]
LIBRARY = [(1, -1, -1), (4095, -1, -1), (4096, -1, -1)]
PLANS = ONE_UNDER + DEEP + RAGGED + TOP_ONE + LIBRARY
FORMS = [0, 1, 2, 3, 4]
FAMILIES = ["random", "all r - 1", "ones"]
ZERO32 = bytes(32)

# one pair of random vectors of nonzero values serves every n as its prefix, so that every inverse is computed once
NMAX = max(n for n, _, _ in PLANS)
_rnd = random.Random(0x5ca9)
BASE_A = [_rnd.randrange(1, R) for _ in range(NMAX)]
BASE_B = [_rnd.randrange(1, R) for _ in range(NMAX)]
START = _rnd.randrange(1, R)
inv = functools.lru_cache(maxsize=None)(sref.inverse)


@pytest.fixture(scope="module")
def eng(hip):
    return hip()


def chunk_of(l0):
    return 1 << (2 if l0 < 0 else l0)


@functools.lru_cache(maxsize=None)
def vectors(family, n):
    """(a, b) -- computed once per (family, n), never changed"""
    if family == "random":
        return tuple(BASE_A[:n]), tuple(BASE_B[:n])
    if family == "all r - 1":
        return (R - 1,) * n, (R - 1,) * n
    assert family == "ones"
    return (1,) * n, (1,) * n


@functools.lru_cache(maxsize=None)
def inputs(family, n):
    a, b = vectors(family, n)
    return row_bytes(a), row_bytes(b)


@functools.lru_cache(maxsize=None)
def expected(form, family, n, start=START):
    """(the n values, the closing value) as bytes"""
    a, b = vectors(family, n)
    out, cl = sref.run(form, a, b, start, inv)
    return row_bytes(out), be(cl)


def same(got, want, n):
    """all n values, the closing value and the flag, bit for bit"""
    got_v, got_cl, got_zf = got
    want_v, want_cl, want_zf = want
    assert got_zf == want_zf, f"zero flag {got_zf}, expected {want_zf}"
    if got_v != want_v:
        bad = [t for t in range(n) if got_v[32 * t:32 * t + 32] != want_v[32 * t:32 * t + 32]]
        raise AssertionError(f"{len(bad)} of {n} values differ, the first at {bad[0]}")
    assert got_cl == want_cl, "the closing value differs"


def good_run(eng, form=0):
    """a run that must be exact, whatever the context served before"""
    n = 300
    a, b = inputs("random", n)
    same(eng.test_scan_run(form, a, b, be(START), n, (2, 16)), expected(form, "random", n) + (0,), n)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,l0,top_max", PLANS)
def test_plan_against_the_reference(eng, n, l0, top_max, form, family):
    a, b = inputs(family, n)
    same(eng.test_scan_run(form, a, b, be(START), n, (l0, top_max)), expected(form, family, n) + (0,), n)


def test_the_plans_reach_every_geometry():
    """the claim of the list above, from the plan function itself (host only)"""
    from zkp_subnet_amd.engine import scan_plan_of
    ks = {(n, l0, tm): scan_plan_of(n, l0, tm) for n, l0, tm in PLANS}
    assert all(ks[p]["K"] == 1 for p in ONE_UNDER)
    assert [ks[p]["n"][1] for p in ONE_UNDER] == [1, 1, 2, 64, 64, 65, 256, 257, 512, 513, 1024, 1025]
    assert {pl["K"] for pl in ks.values()} == {1, 2, 3, 4}
    assert ks[(4096, 2, 16)]["n"] == [4096, 1024, 64, 4] and ks[(4096, 3, 16)]["n"] == [4096, 512, 32, 2]
    assert ks[(4096, 4, 16)]["n"] == [4096, 256, 16] and ks[(4096, 2, 1)]["n"] == [4096, 1024, 64, 4, 1]
    assert ks[(5, 2, 1)]["n"] == [5, 2, 1] and ks[(1, 3, 1)]["n"] == [1, 1] and ks[(17, 4, 1)]["n"] == [17, 2, 1]
    for l0 in (2, 3, 4):   # a ragged last chunk at level 0, and at some level k >= 1 (the expansions' clamp), for every level-0 chunk
        mine = [pl for pl in ks.values() if pl["l"][0] == l0]
        assert any(pl["n"][0] % (1 << l0) for pl in mine)
        assert any(pl["n"][k] % (1 << pl["l"][k]) for pl in mine for k in range(1, pl["K"]))
    assert any(pl["n"][k] % 16 for pl in ks.values() for k in range(1, pl["K"] - 1))           # ... and under a further expansion
    tops = {pl["n"][-1] for pl in ks.values()}
    assert 1 in tops and any(m % 256 and m > 256 for m in tops) and any(m < 256 for m in tops) and 2 in tops
    assert ks[(4096, -1, -1)]["K"] == 1 and ks[(1, -1, -1)]["n"] == [1, 1]


def numerator_zeros(n, l0):
    """the first and the last element of level-0 chunks and of 16-chunk groups, from the middle of the vector on, and n - 1"""
    c = chunk_of(l0)
    mid = n // 2 // (16 * c) * (16 * c)
    spots = [mid, mid + 16 * c - 1, mid + 16 * c, mid + 5 * c, mid + 6 * c - 1, n // 2 // c * c, n // 2 // c * c + c - 1, 0, c - 1, n - 1]
    return sorted({t for t in spots if 0 <= t < n})


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("n,l0,top_max", PLANS)
def test_a_zero_numerator_zeroes_everything_behind_it(eng, n, l0, top_max, form):
    """a[p] = 0 at one border after the other: the values up to p are those of the vector without the zero (an exclusive product
    does not hold its own element), every value behind p and the closing value are 0, and the flag stays 0"""
    a, b = inputs("random", n)
    want_v, _ = expected(form, "random", n)
    for p in numerator_zeros(n, l0):
        got = eng.test_scan_run(form, a[:32 * p] + ZERO32 + a[32 * p + 32:], b, be(START), n, (l0, top_max))
        same(got, (want_v[:32 * (p + 1)] + bytes(32 * (n - p - 1)), ZERO32, 0), n)


def test_the_zero_numerator_expectation_is_the_reference_s():
    """(host only) what the test above expects, from the definition"""
    n, p = 37, 14
    a, b = list(BASE_A[:n]), BASE_B[:n]
    out, cl = sref.run(1, a, b, START, inv)
    a[p] = 0
    assert sref.run(1, a, b, START, inv) == (out[:p + 1] + [0] * (n - p - 1), 0) and out[p] != 0


@pytest.mark.parametrize("n,l0,top_max", PLANS)
def test_zero_numerators_of_the_fractions_zero_exactly_their_own_values(eng, n, l0, top_max):
    """form 3, zeros in P on every border at once: exactly those values are 0"""
    a, b = vectors("random", n)
    zeros = numerator_zeros(n, l0)
    b = [0 if t in zeros else x for t, x in enumerate(b)]
    out, cl = sref.run(3, a, b, None, inv)
    assert [t for t in range(n) if out[t] == 0] == zeros and cl == 1
    same(eng.test_scan_run(3, inputs("random", n)[0], row_bytes(b), None, n, (l0, top_max)), (row_bytes(out), be(cl), 0), n)


@pytest.mark.parametrize("form", [0, 1, 2, 3])
@pytest.mark.parametrize("n,l0,top_max", PLANS)
def test_a_zero_denominator_raises_the_flag(eng, n, l0, top_max, form):
    """one 0 in D (forms 0, 1) or in Q (forms 2, 3) at element 0, at a chunk border and at n - 1: the flag is 1 and the call
    answers; nothing is said about the values.  The context then serves an exact run."""
    a, b = inputs("random", n)
    c = chunk_of(l0)
    for p in sorted({0, min(c - 1, n - 1), min(c, n - 1), n - 1}):
        if form in (0, 1):
            got = eng.test_scan_run(form, a, b[:32 * p] + ZERO32 + b[32 * p + 32:], be(START), n, (l0, top_max))
        else:
            got = eng.test_scan_run(form, a[:32 * p] + ZERO32 + a[32 * p + 32:], b, None, n, (l0, top_max))
        assert got[2] == 1 and len(got[0]) == 32 * n, p
    good_run(eng, form)


@pytest.mark.parametrize("n,l0,top_max", [(257, 2, 2048), (4093, 2, 16), (4096, 4, 16), (17, 4, 1), (4096, -1, -1)])
def test_start_values(eng, n, l0, top_max):
    a, b = inputs("random", n)
    for start in (1, R - 1, BASE_A[7]):
        same(eng.test_scan_run(1, a, b, be(start), n, (l0, top_max)), expected(1, "random", n, start) + (0,), n)
    # start = 1 is the plain product
    assert expected(1, "random", n, 1) == expected(0, "random", n)
    # refused as kzg_rows_commit_grand_product_chain refuses them: k_gp_chain_start takes start as canonical and not 0
    arg_error(lambda: eng.test_scan_run(1, a, b, ZERO32, n, (l0, top_max)), "other than 0")
    arg_error(lambda: eng.test_scan_run(1, a, b, R.to_bytes(32, "big"), n, (l0, top_max)), "canonical")
    arg_error(lambda: eng.test_scan_run(1, a, b, None, n, (l0, top_max)), "no data")
    good_run(eng, 1)


def test_errors_leave_the_context_serving(eng):
    n = 300
    a, b = inputs("random", n)
    bad = a[:32 * 7] + R.to_bytes(32, "big") + a[32 * 8:]            # (be() reduces: r itself goes in as raw bytes)
    for form in FORMS:
        arg_error(lambda: eng.test_scan_run(form, a, b, be(START), n, (5, 16)), "level-0 chunk")
        arg_error(lambda: eng.test_scan_run(form, a, b, be(START), n, (2, 4096)), "1 .. 2048")
        arg_error(lambda: eng.test_scan_run(form, a, b, be(START), n, (2, 0)), "1 .. 2048")
        arg_error(lambda: eng.test_scan_run(form, b"", b"", be(START), 0, (2, 16)), "no elements")
        arg_error(lambda: eng.test_scan_run(form, b"", b"", be(START), 0), "no elements")
        good_run(eng, form)
        arg_error(lambda: eng.test_scan_run(form, bad, b, be(START), n, (2, 16)), code=_native.KZG_E_SCALAR)
        good_run(eng, form)
        if form in (0, 1, 3):
            arg_error(lambda: eng.test_scan_run(form, a, bad, be(START), n, (2, 16)), code=_native.KZG_E_SCALAR)
            arg_error(lambda: eng.test_scan_run(form, a, None, be(START), n, (2, 16)), "no data")
            good_run(eng, form)
    arg_error(lambda: eng.test_scan_run(5, a, b, be(START), n, (2, 16)), "form must be")
    good_run(eng)
