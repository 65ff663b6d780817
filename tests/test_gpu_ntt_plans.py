"""GPU parity tests (`-m gpu`): the NTT through explicit pass plans (kzg_test_ntt_run) and at every small size.

Both kernel forms -- k_fr_ntt_pass (radix 2) and k_fr_ntt_pass4 (register-blocked) -- are run on plans chosen by the test instead of
by the launcher: every plan there is for 2^1 .. 2^5, every one- and two-pass plan for 2^6 .. 2^8, and for each per-workgroup geometry
(form, first / middle / last / only pass, S, logC) that a production plan of any size 2^1 .. 2^28 and any tile holds, the smallest plan
that holds it (tests/ntt_ref.py; at most 2^12 elements).  Inputs are the families of tests/ntt_ref.py -- zero, constants, deltas,
geometric sequences, alternating, the fuzz's edge pool, uniform -- with closed-form outputs where there are any.  A zero vector is the
input with the largest lazy limbs (stage 0 subtracts nothing from the 4r constant) and takes row 2^S - 1 of a first-pass tile to exactly
r (3S + 1) through the representatives 0 and r of zero (scripts/models/ntt_lazy_model.py).  Everything is integer arithmetic: bit-exact,
no tolerance.  A failure names the plan, the
family, the direction and the first differing index."""
from functools import lru_cache

import pytest

from tests import ntt_ref as nr

pytestmark = pytest.mark.gpu

SHORT = ["uniform", "zero", "constant r-1"]                  # what the exhaustive part runs


@pytest.fixture(scope="module")
def eng(hip):
    return hip()


@lru_cache(maxsize=None)
def _input(log_n, name):
    return nr.to_bytes(nr.families(log_n)[name].a)


@lru_cache(maxsize=None)
def _expected(log_n, name, inverse):
    return nr.to_bytes(nr.families(log_n)[name].expected(inverse))


def _same(got, want, what):
    if got != want:
        n = len(want) // 32
        k = next((i for i in range(n) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]), n)
        bad = sum(got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32] for i in range(n))
        raise AssertionError(f"{what}: {bad} of {n} elements differ, the first at index {k}: got {got[32 * k:32 * k + 32].hex()}, "
                             f"expected {want[32 * k:32 * k + 32].hex()}")


def _run_plan(eng, log_n, kernel, passes, names):
    for name in names:
        for inverse in (False, True):
            got = eng.test_ntt_run(_input(log_n, name), inverse, kernel, [S for S, _ in passes], [c for _, c in passes])
            _same(got, _expected(log_n, name, inverse),
                  f"plan {nr.plan_name(log_n, kernel, passes)}, {'inverse' if inverse else 'forward'}, family {name!r}")


# ------------------------------------------------------------------------------------------------------------ the size sweep
@pytest.mark.parametrize("log_n", range(0, 17))
def test_every_size_up_to_2_16_every_family_both_directions_and_round_trip(eng, log_n):
    """eng.ntt itself (the production plan of the size): 2^0 .. 2^16 without a gap -- the one-pass sizes with workgroups narrower
    than their 256 lanes, 2^9 (the first two-pass split), twiddle tables of fewer than 64 entries per lane."""
    for name, fam in nr.families(log_n).items():
        fwd = eng.ntt(_input(log_n, name), False)
        _same(fwd, _expected(log_n, name, False), f"2^{log_n} forward, family {name!r}")
        _same(eng.ntt(_input(log_n, name), True), _expected(log_n, name, True), f"2^{log_n} inverse, family {name!r}")
        _same(eng.ntt(fwd, True), _input(log_n, name), f"2^{log_n} round trip, family {name!r}")


# -------------------------------------------------------------------------------------------------- every plan of a small size
@pytest.mark.parametrize("log_n", range(1, 9))
@pytest.mark.parametrize("kernel", [0, 1], ids=["blocked", "radix2"])
def test_every_valid_plan_of_a_small_size(eng, kernel, log_n):
    """2^1 .. 2^5: every plan of up to three passes the kernels admit; 2^6 .. 2^8: every plan of up to two."""
    plans = nr.valid_plans(log_n, kernel, 3 if log_n <= 5 else 2)
    assert len(plans) >= (1 if log_n == 1 else 5)
    for passes in plans:
        _run_plan(eng, log_n, kernel, passes, SHORT)


# ------------------------------------------------------------------------------------- every geometry production plans hold
@pytest.mark.parametrize("log_n", range(1, 14))
@pytest.mark.parametrize("kernel", [0, 1], ids=["blocked", "radix2"])
def test_covering_plans_every_family(eng, kernel, log_n):
    """for each (form, position, S, logC) of a production plan -- sizes 2^1 .. 2^28, tiles 2^8 .. 2^11 -- the smallest plan with it"""
    for lg, k, passes in nr.covering_plans():
        if (lg, k) == (log_n, kernel):
            _run_plan(eng, lg, k, passes, list(nr.families(lg)))


def test_covering_plans_are_all_run():
    assert {(lg, k) for lg, k, _ in nr.covering_plans()} <= {(lg, k) for lg in range(1, 14) for k in (0, 1)}


# -------------------------------------------------------------------------------------------------------------- lazy bounds
# the longest pass each kernel admits, in first, middle and last position
LAZY = [(1, (8, 1)), (1, (1, 8)), (1, (2, 8, 1)), (0, (9, 2)), (0, (2, 9)), (0, (2, 9, 2)), (0, (8, 2)), (0, (2, 8))]


def _with_columns(kernel, stages, widest):
    log_n, out, s0 = sum(stages), [], 0
    for p, S in enumerate(stages):
        out.append((S, min(nr.TILE_LOG[kernel] - S, log_n - S if p == 0 else s0) if widest else 0))
        s0 += S
    assert nr.plan_invalid(log_n, kernel, out) is None
    return log_n, tuple(out)


@pytest.mark.parametrize("kernel,stages", LAZY, ids=[nr.FORMS[k] + "-" + "+".join(map(str, s)) for k, s in LAZY])
def test_lazy_bounds_zero_and_constant_vectors_through_the_longest_passes(eng, kernel, stages):
    """Zero input: every intermediate is a multiple of r carried as a lazy value -- 0 x w is the representative 0, (c r) x w the
    representative r -- and the all-'minus' row of a first-pass tile ends at r (3S + 1), 28r at S = 9, with the largest limbs any
    input produces (scripts/models/ntt_lazy_model.py); it leaves through fr9_reduce_approx to `mid`, or through the final reduction,
    and must come out as 0.  Constant vectors cancel to zero in every 'minus' output.  Tiles of one column and of as many columns
    as fit."""
    for widest in (False, True):
        log_n, passes = _with_columns(kernel, stages, widest)
        _run_plan(eng, log_n, kernel, passes, ["zero", "constant 1", "constant r-1", "constant (r-1)/2"])


# ------------------------------------------------------------------------------------------------ one answer from every plan
def test_every_covering_plan_of_2_10_returns_the_bytes_of_the_production_transform(eng):
    plans = [(k, passes) for lg, k, passes in nr.covering_plans() if lg == 10]
    assert len(plans) >= 8 and {k for k, _ in plans} == {0, 1}
    a = _input(10, "uniform")
    for inverse in (False, True):
        want = eng.ntt(a, inverse)
        _same(want, _expected(10, "uniform", inverse), "2^10 production transform")
        for k, passes in plans:
            got = eng.test_ntt_run(a, inverse, k, [S for S, _ in passes], [c for _, c in passes])
            _same(got, want, f"plan {nr.plan_name(10, k, passes)} against the production plan, {'inverse' if inverse else 'forward'}")


def test_a_malformed_plan_is_refused_with_a_context_too(eng):
    from zkp_subnet_amd import KzgError

    for kernel, S, logC in ((1, [5, 4], [2, 2]), (1, [9, 1], [0, 0]), (0, [5, 5], [2, 7]), (0, [5, 5], [6, 2]), (0, [], [])):
        with pytest.raises(KzgError) as e:
            eng.test_ntt_run(_input(10, "uniform"), False, kernel, S, logC)
        assert e.value.code == -1 and "ntt plan" in str(e.value)
