"""CPU tests of the shuffle argument's host side.  They pin the reference tests/shuffle_ref.py against the definition, check
the gate terms of shuffle_quotient_terms against the quotient reference (a true instance divides, a broken one leaves a
remainder, an expansion beyond the quotient call's caps is refused) and drive the Client's argument parser over a stub engine:
a bad shape or a non-canonical scalar is refused before any device call."""
import random

import pytest

from tests import quotient_ext_ref as qx
from tests import quotient_ref as qr
from tests import shuffle_ref as sr
from tests.gpu_common import R, be
from zkp_subnet_amd import codec
from zkp_subnet_amd.client import Client
from zkp_subnet_amd.engine import shuffle_quotient_terms

T = 16


# ---------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("G,w", [(1, 1), (1, 3), (2, 2), (4, 4)])
@pytest.mark.parametrize("sel", [False, True])
def test_reference_closes_on_true_instances_and_not_on_broken_ones(G, w, sel):
    rnd = random.Random(10 * G + w)
    theta, gamma = rnd.randrange(R), rnd.randrange(R)
    inst = sr.shuffle_instance(G, w, T, 7 * G + w, sel=sel)
    z, closing = sr.shuffle_product(inst[0], inst[1], G, w, theta, gamma, inst[2], inst[3])
    assert closing == 1 and z[0] == 1
    N, D = sr.factors(inst[0], inst[1], G, w, theta, gamma, inst[2], inst[3])
    for t in range(T):   # the step relation on every row, the wrap-around to z_0 = 1 included
        assert (z[(t + 1) % T] * D[t] - z[t] * N[t]) % R == 0
    bad = sr.broken(*inst, seed=3)
    zb, closing_b = sr.shuffle_product(bad[0], bad[1], G, w, theta, gamma, bad[2], bad[3])
    assert closing_b != 1 and zb[0] == 1


@pytest.mark.parametrize("u", [T - 1, T - 2, 5])
def test_reference_blinding_layout(u):
    G, w = 2, 2
    rnd = random.Random(u)
    theta, gamma = rnd.randrange(R), rnd.randrange(R)
    tail = [rnd.randrange(R) for _ in range(T - u - 1)]
    ins, shs, qi, qs = sr.shuffle_instance(G, w, T, 40 + u, usable=u, sel=True)
    z, closing = sr.shuffle_product(ins, shs, G, w, theta, gamma, qi, qs, u, tail)
    assert closing == 1 and z[0] == 1 and z[u] == closing and z[u + 1:] == tail
    N, D = sr.factors(ins, shs, G, w, theta, gamma, qi, qs)
    for t in range(u):
        assert (z[t + 1] * D[t] - z[t] * N[t]) % R == 0
    # what lies at or behind row u is ignored, a zero denominator there included
    shs2 = [r[:] for r in shs]
    qs2 = [None, qs[1]]
    shs2[0][u] = (-gamma - theta * shs2[1][u]) % R          # df_0(w^u) = 0 without a selector
    assert sr.factors(ins, shs2, G, w, theta, gamma, qi, qs2)[1][u] == 0
    ins3, shs3, _, _ = sr.shuffle_instance(G, w, T, 40 + u, usable=u, sel=True)
    for r in ins3 + shs3:
        r[u:] = [rnd.randrange(R) for _ in range(T - u)]
    assert sr.shuffle_product(ins3, shs3, G, w, theta, gamma, qi, qs, u, tail) == (z, closing)
    with pytest.raises(ZeroDivisionError):
        shs4 = [r[:] for r in shs]
        shs4[0][u - 1] = (-gamma - theta * shs4[1][u - 1]) % R
        sr.shuffle_product(ins, shs4, G, w, theta, gamma, qi, [None, qs[1]], u, tail)


def test_reference_identities():
    rnd = random.Random(5)
    theta, gamma = rnd.randrange(R), rnd.randrange(R)
    ins = [[rnd.randrange(R) for _ in range(T)] for _ in range(4)]
    shs = [[rnd.randrange(R) for _ in range(T)] for _ in range(4)]
    plain = sr.shuffle_product(ins, shs, 2, 2, theta, gamma)
    ones = [1] * T
    assert sr.shuffle_product(ins, shs, 2, 2, theta, gamma, [ones, None], [ones, ones]) == plain
    assert sr.shuffle_product(ins[:1], shs[:1], 1, 1, theta, gamma) == sr.shuffle_product(ins[:1], shs[:1], 1, 1, 0, gamma)
    assert sr.shuffle_product(ins, ins, 2, 2, theta, gamma) == ([1] * T, 1)
    zero = [0] * T                                        # everything disabled: every factor is 1
    assert sr.shuffle_product(ins, shs, 2, 2, theta, gamma, [zero, zero], [zero, zero]) == ([1] * T, 1)


# ---------------------------------------------------------------------------------------------------- the gate terms
def _argument(G, w, sel, active, seed, breakit=False):
    """rows z | inputs | shuffles | selectors (2 G) | A | L_0 | L_u and the complete argument's terms over them"""
    rnd = random.Random(seed)
    theta, gamma, alpha = rnd.randrange(R), rnd.randrange(R), rnd.randrange(R)
    u = T - 3 if active else None
    inst = sr.shuffle_instance(G, w, T, seed, usable=u, sel=sel)
    if breakit:
        inst = sr.broken(*inst, seed=seed)
    ins, shs, qi, qs = inst
    z, closing = sr.shuffle_product(ins, shs, G, w, theta, gamma, qi, qs, u, [rnd.randrange(R) for _ in range(2)] if active else ())
    assert (closing == 1) != breakit
    rows = [z] + ins + shs
    in_rows, sh_rows = list(range(1, 1 + G * w)), list(range(1 + G * w, 1 + 2 * G * w))
    isel = ssel = None
    if sel:
        isel, ssel = list(range(len(rows), len(rows) + G)), list(range(len(rows) + G, len(rows) + 2 * G))
        rows += qi + qs
    a_row = None
    if active:
        a_row = len(rows)
        rows.append([int(t < u) for t in range(T)])
    l0 = len(rows)
    rows.append([int(t == 0) for t in range(T)])
    terms = shuffle_quotient_terms(0, in_rows, sh_rows, G, w, be(theta), be(gamma), be(alpha), a_row, isel, ssel, ext_log=2)
    terms = [(int.from_bytes(c, "big"), fs) for c, fs in terms]
    terms += [(1, [(0, 0), (l0, 0)]), (R - 1, [(l0, 0)])]                       # (z - 1) L_0
    if active:
        lu = len(rows)
        rows.append([int(t == u) for t in range(T)])
        a2 = alpha * alpha % R
        terms += [(a2, [(0, 0), (lu, 0)]), (-a2 % R, [(lu, 0)])]                # alpha^2 (z - 1) L_u
    return rows, terms


@pytest.mark.parametrize("G,w,sel,active", [(1, 2, False, False), (1, 2, True, False), (1, 2, False, True), (1, 2, True, True),
                                            (2, 1, False, False)])
def test_terms_divide_on_a_true_instance_and_not_on_a_broken_one(G, w, sel, active):
    rows, terms = _argument(G, w, sel, active, 100 * G + 10 * w + 2 * sel + active)
    assert len(terms) <= 16 and max(len(fs) for _, fs in terms) <= 5
    t, rem = qx.quotient([qr.coeffs_of(r) for r in rows], terms, None, None, 2)
    assert not any(rem)
    assert qr.degree(t) < 3 * T                      # the pieces an n_pieces = 3 call would commit
    rows, terms = _argument(G, w, sel, active, 100 * G + 10 * w + 2 * sel + active, breakit=True)
    _, rem = qx.quotient([qr.coeffs_of(r) for r in rows], terms, None, None, 2)
    assert any(rem)


def test_terms_are_the_relation_at_a_random_point():
    """the expansion against the factored relation, evaluated on random row values (no instance needed)"""
    rnd = random.Random(9)
    G, w = 2, 1
    theta, gamma, coeff = rnd.randrange(R), rnd.randrange(R), rnd.randrange(R)
    vals = {(j, rot): rnd.randrange(R) for j in range(20) for rot in (0, 1)}
    in_rows, sh_rows, isel, ssel = [1, 2], [5, 6], [9, None], [None, 10]
    terms = shuffle_quotient_terms(0, in_rows, sh_rows, G, w, be(theta), be(gamma), be(coeff), 11, isel, ssel, ext_log=3)
    got = 0
    for c, fs in terms:
        p = int.from_bytes(c, "big")
        for f in fs:
            p = p * vals[f] % R
        got = (got + p) % R

    def side(rows, sels):
        out = 1
        for g in range(G):
            f = (gamma + sum(pow(theta, c, R) * vals[(rows[g * w + c], 0)] for c in range(w))) % R
            if sels[g] is not None:
                f = (1 + vals[(sels[g], 0)] * (f - 1)) % R
            out = out * f % R
        return out

    want = coeff * vals[(11, 0)] % R * (vals[(0, 1)] * side(sh_rows, ssel) - vals[(0, 0)] * side(in_rows, isel)) % R
    assert got == want


def test_terms_beyond_the_quotient_caps_are_refused():
    s = be(3)
    with pytest.raises(codec.CodecError, match="KZG_MAX_GATE_TERMS"):                      # 2 * (8 + 1) = 18 terms
        shuffle_quotient_terms(0, list(range(1, 9)), list(range(9, 17)), 1, 8, s, s, s)
    with pytest.raises(codec.CodecError, match=r"2\^ext_log \+ 1"):                        # z, A, two selectors, two input rows
        shuffle_quotient_terms(0, [1, 2], [3, 4], 2, 1, s, s, s, 5, [6, 7], None, ext_log=2)
    assert len(shuffle_quotient_terms(0, [1, 2], [3, 4], 2, 1, s, s, s, 5, [6, 7], None, ext_log=3)) == 13
    with pytest.raises(codec.CodecError, match="input and shuffle rows"):
        shuffle_quotient_terms(0, [1, 2], [3], 1, 2, s, s, s)
    with pytest.raises(codec.CodecError, match="canonical"):
        shuffle_quotient_terms(0, [1], [2], 1, 1, s, R.to_bytes(32, "big"), s)


def test_client_form_of_the_terms():
    fr = lambda v: codec.be32_to_fr(be(v))   # noqa: E731
    got = Client.shuffle_quotient_terms(0, [1, 2], [3, 4], 1, 2, fr(5), fr(6), fr(7), active_row=8)
    want = shuffle_quotient_terms(0, [1, 2], [3, 4], 1, 2, be(5), be(6), be(7), 8)
    assert got == [[codec.be32_to_fr(c), [list(f) for f in fs]] for c, fs in want]


# ---------------------------------------------------------------------------------------------------- the Client's parser
class _StubSet:
    handle, commitments = 77, [bytes(48)]


class _StubEngine:
    def __init__(self):
        self.calls = []

    def commit_shuffle(self, *args):
        self.calls.append(args)
        return _StubSet(), be(1)


FR = lambda v: codec.be32_to_fr(v.to_bytes(32, "big"))   # noqa: E731


def test_client_passes_a_good_call_on_in_the_engines_order():
    eng = _StubEngine()
    c = Client(engine=eng)
    r = c.worker_commit_shuffle([1, 2], [3], 2, 2, FR(5), FR(6))
    assert r.status_code == 200 and r.json() == {"handle": 77, "commitment": codec.g1_to_b64(bytes(48)), "closing": FR(1)}
    assert eng.calls == [([1, 2], [3], 2, 2, be(5), be(6), [], None, None, None, [])]
    r = c.worker_commit_shuffle([1], [3], 2, 1, FR(5), FR(6), sel_handles=[9], input_sel=[0, None], shuffle_sel=None, usable=12,
                                tail=[FR(8), FR(9)])
    assert r.status_code == 200
    assert eng.calls[1] == ([1], [3], 2, 1, be(5), be(6), [9], [0, None], None, 12, [be(8), be(9)])


@pytest.mark.parametrize("kw,why", [
    (dict(n_groups=0), "n_lookups = 0"),
    (dict(n_groups=3, width=6), "<= 16"),
    (dict(n_groups="x"), "integers"),
    (dict(theta=FR(R)), "canonical"),
    (dict(gamma=FR(R + 5)), "canonical"),
    (dict(gamma="!!"), "base64"),
    (dict(input_handles=[]), "handles"),
    (dict(shuffle_handles=list(range(17))), "handles"),
    (dict(input_sel=[0, None]), "no selector handle"),
    (dict(sel_handles=[9], shuffle_sel=[0]), "n_lookups = 2 entries"),
    (dict(sel_handles=[9], input_sel=[0, 16]), "row index below 16"),
    (dict(usable=-1), "negative"),
    (dict(usable=12, tail=[FR(R)]), "canonical"),
    (dict(usable="u"), "integer"),
])
def test_client_refuses_bad_arguments_before_any_device_call(kw, why):
    eng = _StubEngine()
    args = dict(input_handles=[1, 2], shuffle_handles=[3], n_groups=2, width=2, theta=FR(5), gamma=FR(6))
    args.update(kw)
    r = Client(engine=eng).worker_commit_shuffle(**args)
    assert r.status_code == 400 and why in r.json()["error"], r.json()
    assert r.json()["error"].startswith("worker_commit_shuffle") or "handles" in why or "base64" in why
    assert eng.calls == []
