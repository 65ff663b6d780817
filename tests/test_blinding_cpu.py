"""CPU tests of the blinding-rows layout (tests/blinding_ref.py, the reference of tests/test_gpu_blinding.py): a circuit that
is satisfied on its first `usable` rows and carries RANDOM values behind them has a polynomial quotient exactly when the
permutation and lookup relations are masked by the active column A -- whatever the padding holds -- and the quotient stops
being a polynomial as soon as one usable cell is altered.  T = 16 and 32; no GPU."""
import random

import pytest

from tests import blinding_ref as br
from tests import grand_product_ref as gp
from tests import lookup_ref as lr
from tests import multiplicities_ref as mr
from tests import quotient_ref as qr

R = br.R
EXT_LOG, PIECES = 3, 4
SHAPES = [(16, 10), (16, 15), (32, 26), (32, 1)]


@pytest.fixture(scope="module")
def instances():
    cache = {}

    def get(T, u):
        if (T, u) not in cache:
            inst = br.Instance(T, u, 7 * T + u)
            cache[(T, u)] = (inst, inst.coeff_rows())
        return cache[(T, u)]

    return get


def fresh(T, u):
    return br.Instance(T, u, 7 * T + u)


def value_fn(coeffs, T, x):
    w = gp.omega(T)
    return lambda j, rot: qr.poly_eval(coeffs[j], pow(w, rot % T, R) * x % R)


@pytest.mark.parametrize("T,u", SHAPES)
def test_the_builders_follow_their_definitions(T, u):
    inst = fresh(T, u)
    sig = [inst.fixed[br.S1], inst.fixed[br.S2], inst.fixed[br.S3]]
    assert (inst.z_closing, inst.S_closing, inst.missing) == (1, 0, 0)
    # z, S and m by the recurrences, row by row
    N, D = gp.factors(inst.wires, sig, inst.shifts, inst.beta, inst.gamma)
    assert inst.z[0] == 1 and inst.S[0] == 0
    for t in range(u):
        assert inst.z[t + 1] * D[t] % R == inst.z[t] * N[t] % R
    term = lr.terms([inst.wires[2][:u]], [inst.fixed[br.TAB][:u]], inst.m[:u], 1, 1, inst.theta, inst.lbeta)
    for t in range(u):
        assert (inst.S[t + 1] - inst.S[t] - term[t]) % R == 0
    assert inst.z[u] == 1 and inst.S[u] == 0 and inst.m[u] == 0
    assert inst.z[u + 1:] == inst.tails["z"] and inst.S[u + 1:] == inst.tails["S"] and inst.m[u + 1:] == inst.tails["m"]
    assert sum(inst.m[:u]) == u
    # the plain builders over all T rows see the padding: the join misses its cells and neither running value closes
    _, missing = mr.multiplicities([inst.wires[2]], [inst.fixed[br.TAB]], 1, 1)
    assert missing == T - u
    assert gp.grand_product(inst.wires, sig, inst.shifts, inst.beta, inst.gamma)[1] != 1
    # u = T - 1 with nothing behind: the plain grand product's rows, its last step left out
    z_plain, _ = gp.grand_product(inst.wires, sig, inst.shifts, inst.beta, inst.gamma)
    z_last, _ = br.grand_product_zk(inst.wires, sig, inst.shifts, inst.beta, inst.gamma, T - 1, [])
    assert z_last == z_plain


@pytest.mark.parametrize("T,u", SHAPES)
def test_a_zero_denominator_counts_only_on_usable_rows(T, u):
    inst = fresh(T, u)
    sig = [inst.fixed[br.S1], inst.fixed[br.S2], inst.fixed[br.S3]]
    for t, raises in ((u, False), (T - 1, False), (u - 1, True), (0, True)):
        gamma = -(inst.wires[1][t] + inst.beta * sig[1][t]) % R
        beta = -inst.wires[2][t] % R
        if raises:
            with pytest.raises(ZeroDivisionError):
                br.grand_product_zk(inst.wires, sig, inst.shifts, inst.beta, gamma, u, inst.tails["z"])
            with pytest.raises(ZeroDivisionError):
                br.lookup_sum_zk([inst.wires[2]], [inst.fixed[br.TAB]], inst.m, 1, 1, inst.theta, beta, u, inst.tails["S"])
        else:
            br.grand_product_zk(inst.wires, sig, inst.shifts, inst.beta, gamma, u, inst.tails["z"])
            br.lookup_sum_zk([inst.wires[2]], [inst.fixed[br.TAB]], inst.m, 1, 1, inst.theta, beta, u, inst.tails["S"])
            with pytest.raises(ZeroDivisionError):
                gp.grand_product(inst.wires, sig, inst.shifts, inst.beta, gamma)


def check_divisible(inst, coeffs, rnd):
    T = inst.T
    t, rem = br.quotient(coeffs, inst.terms, inst.perm, inst.lookup, inst.active, EXT_LOG)
    assert not any(rem)
    assert len(t) <= PIECES * T                     # fewer than P T coefficients: the pieces hold it
    zeta = rnd.randrange(R)
    num = br.num_at(value_fn(coeffs, T, zeta), inst.terms, inst.perm, inst.lookup, inst.active, zeta, T)
    assert num == qr.poly_eval(t, zeta) * (pow(zeta, T, R) - 1) % R
    return t


@pytest.mark.parametrize("T,u", SHAPES)
def test_the_masked_quotient_is_a_polynomial_whatever_the_padding(instances, T, u):
    inst, coeffs = instances(T, u)
    rnd = random.Random(T + u)
    t0 = check_divisible(inst, coeffs, rnd)
    other = fresh(T, u).pad(991)                    # every padding cell of every wire, and the three tails, redrawn
    assert all(a[:u] == b[:u] and a[u:] != b[u:] for a, b in zip(inst.wires, other.wires))
    assert (other.z_closing, other.S_closing, other.missing) == (1, 0, 0)
    t1 = check_divisible(other, other.coeff_rows(), rnd)
    assert t0 != t1                                 # (the padding does reach t: it is what hides the witness)


@pytest.mark.parametrize("T,u", SHAPES)
def test_one_altered_usable_cell_makes_the_division_inexact(T, u):
    bad = fresh(T, u).broken()
    _, rem = br.quotient(bad.coeff_rows(), bad.terms, bad.perm, bad.lookup, bad.active, EXT_LOG)
    assert any(rem)


@pytest.mark.parametrize("T,u", [(16, 10), (32, 26)])
def test_without_the_active_factor_the_padding_breaks_the_division(instances, T, u):
    """the same satisfied instance under the plain numerator (no A on P1 and LK1): the random rows violate both relations"""
    inst, coeffs = instances(T, u)
    _, rem = br.quotient(coeffs, inst.terms, inst.perm, inst.lookup, None, EXT_LOG)
    assert any(rem)
    _, rem = br.quotient(coeffs, inst.terms, inst.perm, None, None, EXT_LOG)            # the permutation part alone
    assert any(rem)
    lk_terms = [x for x in inst.terms if br.Z_ not in x[1] and x[1] != [br.LU]]
    _, rem = br.quotient(coeffs, lk_terms, None, inst.lookup, None, EXT_LOG)            # the lookup part alone
    assert any(rem)
    _, rem = br.quotient(coeffs, lk_terms, None, inst.lookup, inst.active, EXT_LOG)     # ... and masked: divisible
    assert not any(rem)


def test_the_numerator_with_a_all_ones_is_the_plain_numerator(instances):
    T, u = 16, 10
    inst, coeffs = instances(T, u)
    rows = list(coeffs)
    rows[br.ACT] = qr.coeffs_of([1] * T)
    want = br.numerator(rows, inst.terms, inst.perm, inst.lookup, None, EXT_LOG)
    got = br.numerator(rows, inst.terms, inst.perm, inst.lookup, br.ACT, EXT_LOG)
    assert qr.trim(got) == qr.trim(want)
    x = 0x1234567
    val = value_fn(rows, T, x)
    assert br.num_at(val, inst.terms, inst.perm, inst.lookup, br.ACT, x, T) == qr.poly_eval(want, x)
