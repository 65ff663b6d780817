"""CPU tests (no GPU) that pin tests/lookup_sel_ref.py, the reference of the lookup builders with per-row selectors: without
selectors and with all-ones selectors it IS the plain references, a built instance closes only because of its selectors, one
broken enabled cell is one miss and an open sum, and a selector of arbitrary field elements follows the weighted definition
computed here from scratch."""
import random

import pytest

from tests import blinding_ref as br
from tests import lookup_ref as lr
from tests import lookup_sel_ref as ls
from tests import multiplicities_ref as mr

R = ls.R
LAYOUTS = [(4, None), (4, 11), (6, None), (6, 59)]
layout_id = lambda s: f"T2^{s[0]}-u{s[1]}"   # noqa: E731


def tail_of(T, u, seed):
    rnd = random.Random(seed)
    return [] if u is None else [rnd.randrange(R) for _ in range(T - u - 1)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=layout_id)
def test_no_selector_and_all_ones_are_the_plain_references(layout):
    lg, u = layout
    T, L, w = 1 << lg, 3, 2
    rnd = random.Random(lg)
    inputs, table, _ = lr.lookup_instance(L, w, T, 50 + lg, duplicates=True)
    inputs[1][3] = (inputs[1][3] + 1) % R   # one miss, so that `missing` is compared too
    theta, beta, tail = rnd.randrange(R), rnd.randrange(R), tail_of(T, u, 7)
    if u is None:
        m, missing = mr.multiplicities(inputs, table, L, w)
        S, closing = lr.lookup_sum(inputs, table, m, L, w, theta, beta)
    else:
        m, missing = br.multiplicities_zk(inputs, table, L, w, u, tail)
        S, closing = br.lookup_sum_zk(inputs, table, m, L, w, theta, beta, u, tail)
    assert missing == 1
    ones = [1] * T
    for sels in ([None] * L, [ones] * L, [None, ones, None]):
        assert ls.multiplicities_sel(inputs, table, sels, L, w, u, tail) == (m, missing)
        assert ls.lookup_sum_sel(inputs, table, m, sels, L, w, theta, beta, u, tail) == (S, closing)


@pytest.mark.parametrize("layout", LAYOUTS, ids=layout_id)
def test_a_built_instance_closes_because_of_its_selectors(layout):
    lg, u = layout
    T, L, w = 1 << lg, 2, 2
    n = T if u is None else u
    rnd = random.Random(10 + lg)
    inputs, table, sels = ls.sel_instance(L, w, T, 70 + lg, u)
    for q in sels:
        assert {0, 1} == set(q[:n])
    theta, beta, tail = rnd.randrange(R), rnd.randrange(R), tail_of(T, u, 8)
    m, missing = ls.multiplicities_sel(inputs, table, sels, L, w, u, tail)
    assert missing == 0 and sum(m[:n]) == sum(sum(q[:n]) for q in sels)
    S, closing = ls.lookup_sum_sel(inputs, table, m, sels, L, w, theta, beta, u, tail)
    assert closing == 0 and S[0] == 0
    if u is not None:
        assert S[u] == 0 and S[u + 1:] == tail and m[u] == 0 and m[u + 1:] == tail
    # the same rows WITHOUT selectors: the disabled cells are misses and the sum stays open
    m0, missing0 = ls.multiplicities_sel(inputs, table, [None] * L, L, w, u, tail)
    assert missing0 == sum(q[:n].count(0) for q in sels) > 0 and m0[:n] == m[:n]
    assert ls.lookup_sum_sel(inputs, table, m0, [None] * L, L, w, theta, beta, u, tail)[1] != 0
    # one enabled cell broken: one miss, and the sum does not close
    broken = ls.break_enabled_cell(inputs, table, sels, w, 5, u)
    mb, missing_b = ls.multiplicities_sel(broken, table, sels, L, w, u, tail)
    assert missing_b == 1 and sum(mb[:n]) == sum(m[:n]) - 1
    assert ls.lookup_sum_sel(broken, table, mb, sels, L, w, theta, beta, u, tail)[1] != 0


def test_an_all_zero_selector_switches_everything_off():
    T, L, w, u = 16, 2, 1, 11
    inputs, table, _ = ls.sel_instance(L, w, T, 3, u)
    tail = tail_of(T, u, 9)
    zero = [0] * T
    m, missing = ls.multiplicities_sel(inputs, table, [zero] * L, L, w, u, tail)
    assert (m[:u + 1], missing) == ([0] * (u + 1), 0)
    S, closing = ls.lookup_sum_sel(inputs, table, m, [zero] * L, L, w, 5, 6, u, tail)
    assert (S[:u + 1], closing) == ([0] * (u + 1), 0)


def test_a_selector_of_field_elements_follows_the_weighted_definition():
    T, L, w = 16, 2, 2
    rnd = random.Random(77)
    rows = lambda k: [[rnd.randrange(R) for _ in range(T)] for _ in range(k)]   # noqa: E731
    inputs, table, mult = rows(L * w), rows(w), rows(1)[0]
    q = [0, 1, R - 1] + [rnd.randrange(R) for _ in range(T - 3)]
    sels = [q, None]
    theta, beta = rnd.randrange(R), rnd.randrange(R)
    S, closing = ls.lookup_sum_sel(inputs, table, mult, sels, L, w, theta, beta)
    acc = 0
    for t in range(T):
        assert S[t] == acc
        F0 = (inputs[0][t] + theta * inputs[1][t]) % R
        F1 = (inputs[2][t] + theta * inputs[3][t]) % R
        Tb = (table[0][t] + theta * table[1][t]) % R
        acc = (acc + q[t] * pow(beta + F0, -1, R) + pow(beta + F1, -1, R) - mult[t] * pow(beta + Tb, -1, R)) % R
    assert closing == acc
    # m counts the NONZERO cells, whatever their value
    m, missing = ls.multiplicities_sel(inputs, table, sels, L, w)
    assert missing == (T - 1) + T and sum(m) == 0


def test_a_zero_denominator_counts_on_a_disabled_row_too():
    T, L, w = 16, 1, 1
    inputs, table, sels = ls.sel_instance(L, w, T, 21)
    t = sels[0].index(0)
    m, _ = ls.multiplicities_sel(inputs, table, sels, L, w)
    with pytest.raises(ZeroDivisionError):
        ls.lookup_sum_sel(inputs, table, m, sels, L, w, 0, (-inputs[0][t]) % R)


# ---------------------------------------------------------------------------------------------------- the quotient
QSHAPES = [(1, 1, 1, None), (3, 2, 2, None), (2, 2, 2, 11)]   # L, w, ext_log, usable


@pytest.mark.parametrize("shape", QSHAPES, ids=lambda s: f"L{s[0]}w{s[1]}e{s[2]}u{s[3]}")
def test_the_quotient_with_selectors(shape):
    L, w, ext_log, u = shape
    T = 16
    inst = ls.QuotInstance(L, w, T, 30 + L, u)
    assert (inst.missing, inst.closing) == (0, 0)
    rows = inst.coeff_rows()
    t, rem = ls.quotient_sel(rows, inst.terms, None, inst.lookup, inst.sel_rows, inst.active, ext_log)
    assert not any(rem) and len(t) <= (1 << ext_log) * T
    # num(x) = t(x) Z_H(x) at a random x, from the rows' values alone
    from tests import quotient_ref as qr
    rnd = random.Random(L)
    x, wT = rnd.randrange(R), pow(7, (R - 1) // T, R)
    val = lambda j, rot: qr.poly_eval(rows[j], x * pow(wT, rot, R) % R)   # noqa: E731
    assert ls.num_at_sel(val, inst.terms, None, inst.lookup, inst.sel_rows, inst.active, x, T) == \
        qr.poly_eval(t, x) * (pow(x, T, R) - 1) % R
    # without the selectors in LK1 the same rows leave a remainder; so does one broken enabled cell with them
    assert any(br.quotient(rows, inst.terms, None, inst.lookup, inst.active, ext_log)[1])
    bad = ls.QuotInstance(L, w, T, 30 + L, u, broken=True)
    assert bad.missing == 1 and bad.closing != 0
    assert any(ls.quotient_sel(bad.coeff_rows(), bad.terms, None, bad.lookup, bad.sel_rows, bad.active, ext_log)[1])
    # sentinels, and all-ones selector rows, are the numerator without selectors
    plain = br.numerator(rows, inst.terms, None, inst.lookup, inst.active, ext_log)
    assert ls.numerator_sel(rows, inst.terms, None, inst.lookup, [None] * L, inst.active, ext_log) == plain
    ones = rows + [qr.coeffs_of([1] * T)]
    from tests.quotient_ref import trim
    assert trim(ls.numerator_sel(ones, inst.terms, None, inst.lookup, [len(rows)] * L, inst.active, ext_log)) == trim(plain)
