"""GPU parity tests (`-m gpu`): the opening scan -- y = f(alpha) and q = (f - y) / (X - alpha), csrc/fr_poly.hip -- through explicit
level plans (kzg_test_poly_run) and at every small length.

The kernels are run on plans chosen by the test instead of by the launcher: for every signature that a single kernel instance of a
production plan of any length up to 2^28 can distinguish -- level kernel (alpha as argument or from memory, chunk length, partial last
chunk, single / rows / pairs grid), fr9_pow2k exponent per kernel, scan (lanes, values per lane, idle lanes, short last lane), expand
(partial last group), quotient (strided / LDS-staged / Montgomery, fill of the last chunk) -- the first plan of tests/poly_ref.py's
candidate lengths that holds it, none longer than 2^16 + 1; five levels and the exponents 12, 16 and 20 among them, which production
reaches from 2^19, 2^23 and 2^27 coefficients.  The hook uploads, runs the library's own launcher with the caller's plan and downloads
the evaluation and the RAW quotient buffer: no SRS, no MSM, every coefficient compared, slot n - 1 included.  The reference is
Horner's rule and synthetic division in Python integers (closed forms: tests/test_poly_plans_cpu.py).  Bit-exact, no tolerance.  A
failure names the plan, the form, the family, the point and the first differing index."""
import pytest

from oracle.bls12_381 import R
from tests import poly_ref as pr
from tests.ntt_ref import to_bytes

pytestmark = pytest.mark.gpu

ALL_FORMS = tuple(pr.FORMS)
PLANS = list(pr.covering_plans()) + [(n, plan, ALL_FORMS) for n, plan in pr.extra_plans()]
IDS = [pr.plan_name(n, plan).replace(" ", "-") for n, plan, _ in PLANS]
MONT_INV = pow(pr.MONT, -1, R)


@pytest.fixture(scope="module")
def eng(hip):
    return hip()


def be(*vals):
    return b"".join(v.to_bytes(32, "big") for v in vals)


def le(vals):
    return b"".join(v.to_bytes(32, "little") for v in vals)


def _same(got, want, what):
    if got != want:
        n = len(want) // 32
        k = next((i for i in range(n) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]), n)
        bad = sum(got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32] for i in range(n))
        raise AssertionError(f"{what}: {bad} of {n} elements differ, the first at index {k}: got {got[32 * k:32 * k + 32].hex()}, "
                             f"expected {want[32 * k:32 * k + 32].hex()}")


def _open(eng, n, plan, name, pname, alpha, form=0):
    """one family at one point through form 0 (y and every quotient slot) or form 1 (y)"""
    what = f"plan {pr.plan_name(n, plan)}, form {form} ({pr.FORMS[form]}), family {name!r}, point {pname}"
    y, q = pr.expected(n, name, alpha)
    got_y, got_q = eng.test_poly_run(form, pr.input_bytes(n, name), n, be(alpha), plan)
    _same(got_y, be(y), what + ", y")
    if form == 0:
        assert len(got_q) == 32 * n and got_q[32 * (n - 1):] == bytes(32), what + f": slot n - 1 holds {got_q[32 * (n - 1):].hex()}"
        _same(got_q, le(q), what + ", quotient")
        if n <= 512:                                      # where it is cheap: the closed form too, from no division at all
            c = pr.families(n)[name].closed(alpha)
            assert c is None or (be(c[0]), le(c[1])) == (got_y, got_q), what + ", closed form"
    else:
        assert got_q == b""


def _family_runs(n):
    rnd = pr.points(n)["random"]
    for name, fam in pr.families(n).items():
        yield (name, "own", fam.point) if fam.point is not None else (name, "random", rnd)


# ------------------------------------------------------------------------------------------- every listed plan through form 0
@pytest.mark.parametrize("n,plan,forms", PLANS, ids=IDS)
def test_listed_plan_opens_every_family_and_every_point(eng, n, plan, forms):
    assert pr.plan_invalid(n, plan) is None
    for name, pname, alpha in _family_runs(n):
        _open(eng, n, plan, name, pname, alpha)
    for pname, alpha in pr.points(n).items():
        _open(eng, n, plan, "uniform", pname, alpha)
    _open(eng, n, plan, "constant r-1", "r-1", R - 1)     # (the family `all r-1 at r-1` by its other name)


# ---------------------------------------------------------------------------------------------------------------- forms 1 - 5
def _with(form):
    sel = [(p, i) for p, i in zip(PLANS, IDS) if form in p[2]]
    return pytest.mark.parametrize("n,plan", [p[:2] for p, _ in sel], ids=[i for _, i in sel])


def _rows(n, rows):
    """`rows` vectors of n coefficients: the families in their order, round and round"""
    names = list(pr.families(n))
    return [names[(3 * j + 7) % len(names)] for j in range(rows)]


@_with(1)
def test_form_1_alpha_from_memory_no_quotient(eng, n, plan):
    for name, pname, alpha in _family_runs(n):
        _open(eng, n, plan, name, pname, alpha, form=1)
    _open(eng, n, plan, "uniform", "0", 0, form=1)


@_with(2)
def test_form_2_rows_side_by_side(eng, n, plan):
    alpha = pr.points(n)["random"]
    for rows in (1, 2, 16):
        names = _rows(n, rows)
        got_y, _ = eng.test_poly_run(2, b"".join(pr.input_bytes(n, nm) for nm in names), n, be(alpha), plan, rows=rows)
        _same(got_y, be(*[pr.expected(n, nm, alpha)[0] for nm in names]),
              f"plan {pr.plan_name(n, plan)}, form 2 (rows), {rows} rows {names}, random point, y per row")


PAIR_SETS = {"point 2 left out": [(0, 0), (2, 0), (4, 0), (1, 1), (0, 3), (1, 3), (2, 3), (3, 3), (4, 3)],
             "point 0 left out": [(4, 1), (3, 2), (0, 2), (1, 3)],
             "every row at every point": [(j, p) for p in range(4) for j in range(5)],
             "one pair": [(3, 2)]}


@_with(3)
def test_form_3_pairs_of_rows_and_points(eng, n, plan):
    names = _rows(n, 5)
    pts = [pr.points(n)[k] for k in ("random", "r-1", "root of unity", "2")]
    f = b"".join(pr.input_bytes(n, nm) for nm in names)
    for tag, pairs in PAIR_SETS.items():
        pairs = sorted(pairs, key=lambda rp: rp[1])                      # point-major, the rows of a point in the order given
        got_y, _ = eng.test_poly_run(3, f, n, be(*pts), plan, rows=5, pairs=pairs)
        _same(got_y, be(*[pr.expected(n, names[j], pts[p])[0] for j, p in pairs]),
              f"plan {pr.plan_name(n, plan)}, form 3 (pairs), rows {names}, pairs {pairs} ({tag}), y per pair")


@_with(4)
def test_form_4_vectors_at_their_points_canonical_quotients(eng, n, plan):
    for m in (1, 2, 4):
        names = _rows(n, m)
        pts = [pr.points(n)[k] for k in ("random", "root of unity", "r-1", "0")][:m]
        got_y, got_q = eng.test_poly_run(4, b"".join(pr.input_bytes(n, nm) for nm in names), n, be(*pts), plan, rows=m)
        what = f"plan {pr.plan_name(n, plan)}, form 4 (points), {m} vectors {names}"
        _same(got_y, be(*[pr.expected(n, nm, a)[0] for nm, a in zip(names, pts)]), what + ", y per vector")
        for p, (nm, a) in enumerate(zip(names, pts)):
            _same(got_q[32 * n * p:32 * n * (p + 1)], le(pr.expected(n, nm, a)[1]), what + f", quotient of vector {p}")


@_with(5)
def test_form_5_chained_division_montgomery_quotients(eng, n, plan):
    """two vectors divided by one point each through a map, the quotients left in Montgomery form; then those quotients, read
    back as they are, divided by the other point: the two steps of a kzg_rows_commit_shplonk group with two points"""
    names = ["uniform", "edge pool"]
    a = [pr.points(n)["random"], pr.points(n)["root of unity"]]
    what = f"plan {pr.plan_name(n, plan)}, form 5 (chain), vectors {names}"
    y1, q1 = eng.test_poly_run(5, b"".join(pr.input_bytes(n, nm) for nm in names), n, be(*a), plan, rows=2, pts=[1, 0])
    want1 = [pr.expected(n, names[0], a[1]), pr.expected(n, names[1], a[0])]
    _same(y1, be(want1[0][0], want1[1][0]), what + ", first division, y")
    mont = pr.words_to_ints(q1)
    assert all(v < R for v in mont), what + ": a Montgomery quotient coefficient is not reduced below r"
    _same(le([v * MONT_INV % R for v in mont]), le(want1[0][1] + want1[1][1]), what + ", first division, quotient times R^-1")
    # the second division reads the Montgomery residues the first one wrote
    y2, q2 = eng.test_poly_run(5, be(*mont), n, be(*a), plan, rows=2, pts=[0, 1], f_mont=True)
    want2 = [pr.open_at(list(want1[0][1]), a[0]), pr.open_at(list(want1[1][1]), a[1])]
    _same(y2, be(want2[0][0], want2[1][0]), what + ", second division, y")
    _same(le([v * MONT_INV % R for v in pr.words_to_ints(q2)]), le(want2[0][1] + want2[1][1]),
          what + ", second division, quotient times R^-1")


# ------------------------------------------------------------------------------------------------------- the production plan
_LONG = {}


def _uniform_prefix(n):
    """the first n of one seeded vector of 2^17 + 5 coefficients, as bytes and as integers"""
    if not _LONG:
        import random

        rnd = random.Random(0xE7A1)
        _LONG["f"] = [rnd.randrange(R) for _ in range((1 << 17) + 5)]
        _LONG["b"] = to_bytes(_LONG["f"])
    return _LONG["b"][:32 * n], _LONG["f"][:n]


EVAL_GROUPS = {"1..80": list(range(1, 81)), **{f"2^{k}": [(1 << k) - 1, 1 << k, (1 << k) + 1] for k in range(7, 17)},
               "2^17": [1 << 17, (1 << 17) + 5]}


@pytest.mark.parametrize("group", list(EVAL_GROUPS))
def test_production_plan_evaluates_every_small_length(eng, group):
    """eng.eval itself: every length 1 .. 80, 2^k - 1, 2^k, 2^k + 1 up to 2^16, and 2^17 and 2^17 + 5, the lengths with 8-long
    level-0 chunks (full and partial) that nothing ran before"""
    for n in EVAL_GROUPS[group]:
        raw, f = _uniform_prefix(n)
        for pname in ("random", "root of unity") if n > 80 else ("random", "0", "1", "r-1", "root of unity", "2"):
            alpha = pr.points(n)[pname]
            _same(eng.eval(raw, be(alpha)), be(pr.horner(f, alpha)), f"eng.eval, {n} coefficients (production plan), point {pname}")
    assert group != "2^17" or [pr.production_plan(n)[0] for n in EVAL_GROUPS[group]] == [3, 3]


@pytest.mark.parametrize("n", [1 << k for k in range(0, 17)] + [1 << 17, (1 << 17) + 5], ids=lambda n: f"n={n}")
def test_production_plan_opens_powers_of_two_and_the_8_long_chunks(eng, n):
    raw, f = _uniform_prefix(n)
    alpha = pr.points(n)["random"]
    y, q = pr.open_at(f, alpha)
    got_y, got_q = eng.test_poly_run(0, raw, n, be(alpha))
    _same(got_y, be(y), f"production plan, form 0, {n} coefficients, y")
    _same(got_q, le(q), f"production plan, form 0, {n} coefficients, quotient")
    assert q[n - 1] == 0


# --------------------------------------------------------------------------------------------------------- the LDS quotient
@pytest.mark.parametrize("n", [1024, 2048, 3072])
@pytest.mark.parametrize("scan_max", [2048, 8])
def test_lds_staged_quotient_at_its_smallest_inputs(eng, n, scan_max):
    """one, two and three workgroups of k_poly_quotient16_lds -- the shift down by two 16-byte units, gu >= 2 in workgroup 0 only, the
    zero of slot n - 1 from the last lane of the last workgroup, the four phases -- and k_poly_quotient on the same input: each
    against the reference, not against the other"""
    for lds in (1, 0):
        plan = (4, scan_max, 256, lds)
        for name, pname, alpha in _family_runs(n):
            _open(eng, n, plan, name, pname, alpha)
        for pname, alpha in pr.points(n).items():
            _open(eng, n, plan, "uniform", pname, alpha)
    # and once per point of form 4, where the LDS kernel is launched vector by vector
    names, pts = _rows(n, 3), [pr.points(n)[k] for k in ("random", "1", "2")]
    got_y, got_q = eng.test_poly_run(4, b"".join(pr.input_bytes(n, nm) for nm in names), n, be(*pts), (4, scan_max, 256, 1), rows=3)
    for p, (nm, a) in enumerate(zip(names, pts)):
        _same(got_q[32 * n * p:32 * n * (p + 1)], le(pr.expected(n, nm, a)[1]), f"LDS quotient, form 4, n={n}, vector {p} ({nm})")
    _same(got_y, be(*[pr.expected(n, nm, a)[0] for nm, a in zip(names, pts)]), f"LDS quotient, form 4, n={n}, y")


# ------------------------------------------------------------------------------------------------------------------ the hook
def test_every_form_is_run_on_some_listed_plan_and_a_malformed_plan_is_refused_with_a_context_too(eng):
    from zkp_subnet_amd import KzgError

    for form in pr.FORMS:
        assert sum(form in forms for _, _, forms in pr.covering_plans()) >= 3, form
    raw, _ = _uniform_prefix(1024)
    for plan in ((5, 8, 256, 0), (2, 0, 256, 0), (2, 8, 128, 0), (2, 8, 256, 1), (3, 8, 256, 1)):
        with pytest.raises(KzgError) as e:
            eng.test_poly_run(0, raw, 1024, be(5), plan)
        assert e.value.code == -1 and "poly plan" in str(e.value)
    with pytest.raises(KzgError) as e:                                   # a point that is no scalar: the library's own check
        eng.test_poly_run(0, raw, 1024, be(R))
    assert e.value.code == -2
