"""GPU tests (`-m gpu`) of kzg_rows_commit_expr: columns that are sums of products of rotated resident columns, evaluated on
the domain, counted, and committed on the device; and the same arithmetic as a check that commits nothing.  The expected rows
and counts come from the definition in Python integers (tests/expr_ref.py) and are committed with the C oracle, never with the
library under test.  Every case compares the commitments byte for byte, the values at probe indices and at one random point
through eval_rows, and the counts and first indices exactly.  No case goes above 2^12 rows.  Each test leaves rows_stats() where
it found it."""
import ctypes
import random

import pytest

from oracle import cpu as oc
from tests import expr_ref as xref
from tests import grand_product_ref as gp
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, q_call, release, srs_cache
from tests.test_gpu_derived import check_set, probes_of, rand_col
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0xE7B2FED1, 0xE7B2FED2
SHAPE_MSG = "the constraints do not hold"
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def bx(exprs):
    """integer-valued entries -> the engine's: 32-byte coefficients"""
    return [([(be(c), fs) for c, fs in e[0]],) + tuple(e[1:]) for e in exprs]


def run(eng, srs, cols, exprs, rnd, usable=None, tail=(), sizes=None, ef=True, probes=None, keep=False):
    """commit `cols`, evaluate on the device, check the new set, the counts and the first indices against the reference;
    returns (rows, nonzero, first), with keep also the source sets and the new set (the caller releases them)"""
    T = len(cols[0])
    want, nonzero, first = xref.expr_columns(cols, exprs, usable, tail)
    S = commit_sets(eng, cols, sizes or (len(cols),), ef)
    out = None
    try:
        out, gnz, gfirst = eng.commit_expr(S, bx(exprs), usable, bt(tail))
        assert (gnz, gfirst) == (nonzero, first), (gnz, gfirst, nonzero, first)
        if want:
            check_set(eng, srs, out, want, rnd, probes or probes_of(T, rnd, usable))
        else:
            assert out is None
    finally:
        if not keep:
            release(S + ([out] if out is not None else []))
    return (want, nonzero, first, S, out) if keep else (want, nonzero, first)


# ---------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("lg", [1, 2, 6, 8, 10, 12])
def test_geometry_product_sum_copy_and_constant(engines, srs_of, lg):
    """T = 2 and 4 (part of a wave), 2^6 (one wave), 2^8 (one workgroup), 2^10 and 2^12 (several)"""
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(100 + lg)
    cols = [rand_col(T, rnd) for _ in range(3)]
    k = rnd.randrange(1, R)
    exprs = [([(1, [0, 1])],), ([(1, [0, 1]), (1, [2])],), ([(1, [0])],), ([(k, [])],)]
    want, nz, first, S, out = run(eng, srs, cols, exprs, rnd, probes=range(T) if T <= 16 else None, keep=True)
    try:
        assert want[0] == [a * b % R for a, b in zip(cols[0], cols[1])] and want[3] == [k] * T
        assert out.commitments[2] == S[0].commitments[0]            # the copy commits to what its source committed to
        assert nz[3] == T and first[3] == 0
    finally:
        release(S + [out])
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- rotations
@pytest.mark.parametrize("lg", [1, 8, 10])
def test_rotations_reduce_mod_T_and_equal_residues_give_equal_bytes(engines, srs_of, lg):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(200 + lg)
    cols = [rand_col(T, rnd), rand_col(T, rnd)]
    rots = [0, 1, -1, T - 1, T + 1, T, INT32_MIN, INT32_MAX]
    exprs = [([(1, [(0, rot)])],) for rot in rots]
    exprs.append(([(1, [0, (0, 1)]), (3, [(1, -1), (0, T - 1)])],))             # one row at two rotations in one term
    want, _, _, S, out = run(eng, srs, cols, exprs, rnd, probes=range(T) if T <= 16 else None, keep=True)
    try:
        for a in range(len(rots)):
            for b in range(a):
                assert (out.commitments[a] == out.commitments[b]) == ((rots[a] - rots[b]) % T == 0), (rots[a], rots[b])
        assert want[1] == cols[0][1:] + cols[0][:1] and want[2] == cols[0][-1:] + cols[0][:-1]
        assert out.commitments[0] == S[0].commitments[0]
    finally:
        release(S + [out])
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- bounds
def test_lazy_sum_and_operand_class_bounds(engines, srs_of):
    lg = 8
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(300)
    # 16 terms of 8 factors, every cell and every coefficient r - 1: each term is (-1)^9, the sum -16
    cols = [[R - 1] * T for _ in range(8)]
    full = [(R - 1, list(range(8)))] * 16
    want, nz, first = run(eng, srs, cols, [(full,), (full, True)], rnd)
    assert want == [[R - 16] * T] and nz == [T, T] and first == [0, 0]
    # the same terms with random cells, and 16 bare coefficients r - 1
    cols = [rand_col(T, rnd) for _ in range(8)]
    run(eng, srs, cols, [(full,), ([(R - 1, [])] * 16,)], rnd)
    # coefficients 0 and 1; a term naming one row 8 times
    a = rand_col(T, rnd)
    want, nz, first = run(eng, srs, [a, rand_col(T, rnd)], [([(0, [1]), (1, [0])],), ([(0, [0, 1])],), ([(1, [0] * 8)],)], rnd)
    assert want[0] == a and want[1] == [0] * T and want[2] == [pow(x, 8, R) for x in a]
    assert nz[1] == 0 and first[1] is None
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- sources
def test_sources_repeated_handles_two_sets_coefficient_form_and_unnamed_rows(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(400)
    cols = [rand_col(T, rnd) for _ in range(4)]
    exprs = [([(1, [0, 3]), (2, [(3, 1)])],), ([(5, [0, 0])], True)]              # rows 1 and 2: no term names them
    for sizes, ef in (((4,), True), ((1, 3), True), ((2, 2), False)):
        run(eng, srs, cols, exprs, rnd, sizes=sizes, ef=ef)
    # a handle named twice: rows 0 and 1 are the same column
    S = commit_sets(eng, cols[:1], (1,))
    try:
        out, nz, first = eng.commit_expr([S[0], S[0]], bx([([(1, [0, 1])],), ([(1, [0]), (R - 1, [1])], True)]))
        try:
            check_set(eng, srs, out, [[x * x % R for x in cols[0]]], rnd, probes_of(T, rnd))
            assert nz[1] == 0 and first[1] is None
        finally:
            out.release()
    finally:
        release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- counts
@pytest.mark.parametrize("lg", [1, 10])
def test_counts_and_first_indices(engines, srs_of, lg):
    """non-zero nowhere, at {0}, at {T - 1}, on a whole wave (cells 128 .. 191), at {20, 63, 64} across a wave border, and
    everywhere: as checks and, in the same call, as committed copies"""
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(500 + lg)
    sets = [set(), {0}, {T - 1}, set(range(T))]
    if T >= 256:
        sets += [set(range(128, 192)), {20, 63, 64}, {T - 2, 300, 255, 256}]
    cols = [[rnd.randrange(1, R) if t in s else 0 for t in range(T)] for s in sets]
    exprs = [([(1, [j])], True) for j in range(len(sets))] + [([(1, [j])],) for j in range(len(sets))]
    _, nz, first = run(eng, srs, cols, exprs, rnd, probes=range(T) if T <= 16 else None)
    assert nz == [len(s) for s in sets] * 2
    assert first == [min(s) if s else None for s in sets] * 2
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- checks
def test_checks_find_the_wrong_cell_and_commit_nothing(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(600)
    a, b = rand_col(T, rnd), rand_col(T, rnd)
    gate = [(1, [0, 1]), (R - 1, [2])]                                          # a b - c
    want, _, _, S, C = run(eng, srs, [a, b], [([(1, [0, 1])],)], rnd, keep=True)
    made = S + [C]
    try:
        live = eng.rows_stats()
        assert eng.commit_expr(S + [C], bx([(gate, True)])) == (None, [0], [None])
        assert eng.rows_stats() == live                                         # an all-check call creates no set
        for t in (0, 63, 64, 700, T - 1):
            c = list(want[0])
            c[t] = (c[t] + 1) % R
            W = commit_sets(eng, [c], (1,))
            made += W
            assert eng.commit_expr(S + W, bx([(gate, True)])) == (None, [1], [t])
        # committed and check expressions in one call: only the committed ones become rows
        mixed = [(gate, True), ([(1, [0, 1])],), ([(1, [2])], True), ([(1, [2]), (R - 1, [(2, 1)])],)]
        cols = [a, b, want[0]]
        rows, nz, first = xref.expr_columns(cols, mixed)
        out, gnz, gfirst = eng.commit_expr(S + [C], bx(mixed))
        made.append(out)
        assert (gnz, gfirst) == (nz, first) and gnz[0] == 0 and len(rows) == 2
        check_set(eng, srs, out, rows, rnd, probes_of(T, rnd))
        assert out.commitments[0] == C.commitments[0]
    finally:
        release(made)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- composition
def test_an_expression_column_passes_the_quotient_of_its_gate_and_opens(engines):
    lg = 10
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(700)
    a, b = rand_col(T, rnd), rand_col(T, rnd)
    gate = [(1, [0, 1]), (R - 1, [2])]
    S = commit_sets(eng, [a, b], (2,))
    made = list(S)
    try:
        C, nz, first = eng.commit_expr(S, bx([([(1, [0, 1])],)]))
        made.append(C)
        made.append(q_call(eng, S + [C], gate, None, 1, 1))
        sets = S + [C]
        com = [c for s in sets for c in s.commitments]
        P, opened, gam = [be(rnd.randrange(R))], [[0, 1, 2]], [be(rnd.randrange(R))]
        Y, Pf = eng.open_rows(sets, P, opened, gam)
        assert eng.verify_open_multi(0, com, P, opened, gam, Y, Pf)
        ya, yb, yc = (int.from_bytes(y, "big") for y in Y[0])
        assert yc != ya * yb % R                                    # (off the domain c is its own polynomial, not a b)
        # the gate means something: against another column it does not hold
        D, _, _ = eng.commit_expr(S, bx([([(1, [0, 1]), (1, [])],)]))
        made.append(D)
        arg_error(lambda: q_call(eng, S + [D], gate, None, 1, 1), SHAPE_MSG)
    finally:
        release(made)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the layout
@pytest.mark.parametrize("lg,u", [(10, (1 << 10) - 1), (10, (1 << 10) - 32), (2, 1), (2, 3)])
def test_usable_layout(engines, srs_of, lg, u):
    """The source cells at and behind `usable` hold r - 1: a rotated factor of a usable row reads them, no count sees them; the
    tails are checked in place, column-major over the committed columns only."""
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(800 + u)
    cols = [rand_col(u, rnd) + [R - 1] * (T - u), [0] * u + [R - 1] * (T - u)]
    exprs = [([(1, [0, (0, 1)])],), ([(1, [1])], True), ([(1, [(1, 1)])],), ([(1, [(1, -1)])], True), ([(7, []), (1, [1])],)]
    tail = rand_col(3 * (T - u), rnd)
    probes = set(probes_of(T, rnd, u)) | set(range(u, T))
    want, nz, first = run(eng, srs, cols, exprs, rnd, u, tail, probes=probes)
    for c in range(3):
        assert want[c][u:] == tail[c * (T - u):(c + 1) * (T - u)]
    assert want[0][u - 1] == cols[0][u - 1] * (R - 1) % R             # row u - 1 reads cell u
    assert (nz[1], first[1]) == (0, None)                           # the cells r - 1 behind `usable` are not counted
    assert (nz[2], first[2]) == (1, u - 1)                          # ... but read by the rotated factor of row u - 1
    assert (nz[3], first[3]) == (1, 0)                              # row 0 reads cell T - 1
    assert (nz[4], first[4]) == (u, 0)
    # checks alone under a layout: no tail, no set
    S = commit_sets(eng, cols, (2,))
    try:
        assert eng.commit_expr(S, bx([exprs[1], exprs[3]]), u) == (None, [0, 1], [None, 0])
        arg_error(lambda: eng.commit_expr(S, bx(exprs), u, bt(tail[:-1])), "exactly")
    finally:
        release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 6
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    srs = oc.srs_gen(be(SEED_X), be(SEED_Y), lg + 1, 1, 0)
    rnd = random.Random(900)
    cols = [rand_col(T, rnd) for _ in range(3)]
    exprs = [([(1, [0, 1]), (2, [(2, -1)])],), ([(1, [0]), (R - 1, [0])], True)]
    want, want_nz, want_first = xref.expr_columns(cols, exprs)
    want_c = [oc.commit(srs, row_bytes(r), True) for r in want]

    def fresh_ok(sets):
        out, nz, first = eng.commit_expr(sets, bx(exprs))
        out.release()
        assert out.commitments == want_c and (nz, first) == (want_nz, want_first)

    I = commit_sets(eng, cols, (1, 2))
    fresh_ok(I)
    live = eng.rows_stats()
    lib = _native.load()
    E_ARG = _native.KZG_E_ARG
    hi = (ctypes.c_uint64 * 2)(I[0].handle, I[1].handle)
    c, h = ctypes.create_string_buffer(48 * 16), ctypes.c_uint64(0)
    nzb, fb = (ctypes.c_uint64 * 32)(), (ctypes.c_uint64 * 32)()
    ONE, BIG = be(1), R.to_bytes(32, "big")
    keep = []

    def ex(terms, flags=0, coeffs=True, lens=True, rows=True, rots=True, n_terms=None):
        """one kzg_expr from (coefficient bytes, [(row, rot)]) terms; False leaves that array NULL"""
        flat = [f for _, fs in terms for f in fs]
        la = (ctypes.c_uint32 * max(len(terms), 1))(*[len(fs) for _, fs in terms])
        ra = (ctypes.c_uint32 * max(len(flat), 1))(*[j for j, _ in flat])
        ro = (ctypes.c_int32 * max(len(flat), 1))(*[rot for _, rot in flat])
        keep.append((la, ra, ro))
        return _native.Expr(_native.QuotientTerms(len(terms) if n_terms is None else n_terms,
                                                  b"".join(cf for cf, _ in terms) if coeffs else None, la if lens else None,
                                                  ra if rows else None, ro if rots else None), flags)

    def raw(es, opts=None, n=2, n_exprs=None, com=c):
        arr = (_native.Expr * max(len(es), 1))(*es)
        return lib.kzg_rows_commit_expr(eng._h, n, hi, len(es) if n_exprs is None else n_exprs, arr,
                                        ctypes.byref(opts) if opts else None, com, nzb, fb, ctypes.byref(h))

    def refused(rc, why):
        msg = lib.kzg_last_error(eng._h)
        assert rc == E_ARG and msg.startswith(b"expr: ") and why in msg, (rc, msg)
        assert eng.rows_stats() == live
        fresh_ok(I)

    good = ex([(ONE, [(0, 0)])])
    # the expressions
    refused(raw([], n_exprs=0), b"n_exprs")
    refused(raw([good] * 17), b"n_exprs")
    refused(raw([ex([], n_terms=0)]), b"n_terms")
    refused(raw([ex([(ONE, [])] * 17)]), b"n_terms")
    refused(raw([ex([(ONE, [(0, 0)] * 9)])]), b"KZG_MAX_EXPR_FACTORS")
    refused(raw([ex([(ONE, [(0, 0)])], flags=2)]), b"flags")
    refused(raw([good, ex([(ONE, [(0, 0)])], flags=3)]), b"flags")
    refused(raw([ex([(ONE, [(3, 0)])])]), b"a row must index")                     # 3 rows: 0 .. 2
    refused(raw([good, ex([(ONE, [(0, 0), (2 ** 31, 1)])], flags=1)]), b"a row must index")
    refused(raw([ex([(BIG, [(0, 0)])])]), b"canonical")
    refused(raw([ex([(ONE, []), (b"\xff" * 32, [])], flags=1)]), b"canonical")
    refused(raw([ex([(ONE, [(0, 0)])], coeffs=False)]), b"must not be null")
    refused(raw([ex([(ONE, [(0, 0)])], lens=False)]), b"must not be null")
    refused(raw([ex([(ONE, [(0, 0)])], rows=False)]), b"must not be null")
    refused(raw([good], n=0), b"number of handles")
    refused(raw([good], n=17), b"number of handles")
    # a NULL rotation array is every rotation 0, and a constant needs no row array
    assert raw([ex([(ONE, [(0, 5)])], rots=False), ex([(ONE, [])], flags=1, rows=False)]) == 0
    assert list(nzb[:2]) == [T, T] and list(fb[:2]) == [0, 0] and c.raw[:48] == I[0].commitments[0]
    eng.release_rows(h.value)
    # the layout: every tail error of the derived call
    recs = [ex([(ONE, [(0, 0), (1, 0)])]), ex([(ONE, [(2, 1)])]), ex([(ONE, [(0, 0)])], flags=1)]
    tl = b"".join(bt(rand_col(2 * 4, rnd)))
    for usable, tail, why in ((T, tl, b"usable must be in"), (2 ** 40, tl, b"usable must be in"),
                              (T - 33, tl, b"KZG_MAX_BLIND_ROWS"), (T - 4, None, b"tail_be32 must be given"),
                              (0, tl, b"plain layout"), (T - 4, tl[:-32] + BIG, b"canonical"),
                              (T - 4, b"\xff" * 32 + tl[32:], b"canonical")):
        refused(raw(recs, _native.ExprOpts(usable, tail)), why)
    arg_error(lambda: eng.commit_expr(I, bx(exprs), 0), "usable")
    arg_error(lambda: eng.commit_expr(I, bx(exprs), T - 4, [be(1)] * 3), "exactly")
    arg_error(lambda: eng.commit_expr(I, bx(exprs), None, [be(1)]), "tail needs usable")
    assert raw(recs, _native.ExprOpts(0, None)) == 0               # usable = 0 spelled out: the plain layout
    assert h.value != 0
    eng.release_rows(h.value)
    # checks alone: no handle, no commitment buffer, nothing live
    assert raw([ex([(ONE, [(0, 0)])], flags=1)], com=None) == 0 and h.value == 0
    assert raw([ex([(ONE, [(0, 0)])], flags=1)], _native.ExprOpts(T - 4, None), com=None) == 0 and h.value == 0
    assert list(nzb[:1]) == [T - 4]
    assert eng.rows_stats() == live
    # handles
    other = commit_sets(eng, cols[1:], (2,), i=1)                  # another worker
    arg_error(lambda: eng.commit_expr([I[0]] + other, bx(exprs)), "one worker")
    short = eng.commit_rows(0, [row_bytes(r[:T // 2]) for r in cols[1:]])      # another length
    arg_error(lambda: eng.commit_expr([I[0], short], bx(exprs)), "one worker and have one row length")
    release(other + [short])
    gone = commit_sets(eng, cols[1:], (2,))
    release(gone)
    arg_error(lambda: eng.commit_expr([I[0]] + gone, bx(exprs)), "released")
    arg_error(lambda: eng.commit_expr([2 ** 40], bx(exprs[1:])), "unknown")
    arg_error(lambda: eng.commit_expr(I * 6, bx(exprs)), "KZG_MAX_BATCH_OPEN rows")    # 18 rows
    fresh_ok(I)
    # the 65th live set: a committing call is refused, a call of checks alone is not
    fill = [eng.commit_rows(0, [row_bytes(cols[0])]) for _ in range(_native.KZG_MAX_ROW_SETS - 2)]
    assert eng.rows_stats()[0] == _native.KZG_MAX_ROW_SETS
    arg_error(lambda: eng.commit_expr(I, bx(exprs)), "KZG_MAX_ROW_SETS", code=_native.KZG_E_BUSY)
    assert eng.commit_expr(I, bx(exprs[1:])) == (None, [0], [None])
    fill.pop().release()
    fresh_ok(I)
    release(fill)
    # stale after an SRS load
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.commit_expr(I, bx(exprs)), "SRS")
    release(I)
    I = commit_sets(eng, cols, (3,))
    out, nz, first = eng.commit_expr(I, bx(exprs))
    assert out.commitments == want_c and (nz, first) == (want_nz, want_first)
    # the new set goes stale and releases like any other
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.eval_rows([out], [be(3)], [[0]]), "SRS")
    release(I + [out])
    arg_error(lambda: eng.release_rows(out.handle))
    assert eng.rows_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------------- routing
def test_client_multi_handle_and_multi_device_client_return_the_engine_bytes(hip):
    from zkp_subnet_amd import Client, MultiDeviceClient, codec
    from zkp_subnet_amd.engine import lagrange_factor

    lib = _native.load()
    scale, ms = 8, 1
    T, M = 1 << (scale - ms), 1 << ms
    tx, ty = 0xABCDEF0777, 0x13579BF7
    rnd = random.Random(1000)
    exprs = [([(1, [0, 1]), (R - 2, [(1, -1)])],), ([(1, [0]), (R - 1, [0])], True), ([(3, []), (1, [(0, 1), 1])],)]
    keep = []

    def c_exprs():
        out = []
        for e in exprs:
            flat = [xref.factor(f) for _, fs in e[0] for f in fs]
            la = (ctypes.c_uint32 * len(e[0]))(*[len(fs) for _, fs in e[0]])
            ra = (ctypes.c_uint32 * max(len(flat), 1))(*[j for j, _ in flat])
            ro = (ctypes.c_int32 * max(len(flat), 1))(*[rot for _, rot in flat])
            keep.append((la, ra, ro))
            out.append(_native.Expr(_native.QuotientTerms(len(e[0]), b"".join(be(cf) for cf, _ in e[0]), la, ra, ro),
                                    _native.KZG_EXPR_CHECK if xref.is_check(e) else 0))
        return (_native.Expr * len(out))(*out)

    arr = c_exprs()
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(1, (ctypes.c_int * 1)(0), ctypes.byref(mh)) == 0
    u = T - 3
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    NONE = _native.KZG_EXPR_NONE
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        c, cc = ctypes.create_string_buffer(48 * 2), ctypes.create_string_buffer(96)
        nzb, fb = (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 3)()
        made = {}
        for i in range(M):
            cols = [rand_col(T, rnd), rand_col(T, rnd)]
            tail = b"".join(bt(rand_col(2 * (T - u), rnd)))
            I = commit_sets(single, cols, (2,), i=i)
            plain, pn, pf = single.commit_expr(I, bx(exprs))
            lay, ln, lf = single.commit_expr(I, bx(exprs), u, [tail[j:j + 32] for j in range(0, len(tail), 32)])
            release(I + [plain, lay])
            hi, hz = ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 2, b"".join(row_bytes(r) for r in cols), T, 1, cc, ctypes.byref(hi)) == 0
            ai = (ctypes.c_uint64 * 1)(hi.value)
            assert lib.kzg_multi_rows_commit_expr(mh, i, 1, ai, 3, arr, None, c, nzb, fb, ctypes.byref(hz)) == 0, i
            assert c.raw == b"".join(plain.commitments) and list(nzb) == pn
            assert [None if v == NONE else v for v in fb] == pf
            made[i] = [hi.value, hz.value]
            opts = _native.ExprOpts(u, tail)
            assert lib.kzg_multi_rows_commit_expr(mh, i, 1, ai, 3, arr, ctypes.byref(opts), c, nzb, fb, ctypes.byref(hz)) == 0, i
            assert c.raw == b"".join(lay.commitments) and list(nzb) == ln
            assert [None if v == NONE else v for v in fb] == lf
            made[i].append(hz.value)
        ai = (ctypes.c_uint64 * 1)(made[1][0])                     # worker 1's set under index 0
        assert lib.kzg_multi_rows_commit_expr(mh, 0, 1, ai, 3, arr, None, c, nzb, fb, ctypes.byref(hz)) == _native.KZG_E_ARG
        for i in range(M):
            for hh in made[i]:
                assert lib.kzg_multi_rows_release(mh, i, hh) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)

    # the text clients over the engine: the same bytes as a commit of the reference rows
    def wire(es):
        return [[[[codec.be32_to_fr(be(cf)), [list(f) if isinstance(f, tuple) else f for f in fs]] for cf, fs in e[0]]]
                + ([True] if xref.is_check(e) else []) for e in es]

    def through(client, workers):
        for i in workers:
            cols = [rand_col(T, rnd), rand_col(T, rnd)]
            tail = rand_col(2 * (T - u), rnd)
            a = client.worker_commit_rows(i, [fr(col) for col in cols]).json()["handle"]
            for usable, tl in ((None, []), (u, tail)):
                want, nz, first = xref.expr_columns(cols, exprs, usable, tl)
                ref = client.worker_commit_rows(i, [fr(col) for col in want]).json()
                r = client.worker_commit_expr([a], wire(exprs), usable, fr(tl))
                assert r.status_code == 200, r.json()
                assert r.json()["commitments"] == ref["commitments"]
                assert (r.json()["nonzero"], r.json()["first"]) == (nz, first)
                for hh in (ref["handle"], r.json()["handle"]):
                    assert client.worker_release_rows(hh).status_code == 200
            r = client.worker_commit_expr([a], wire(exprs[1:2]))
            assert r.status_code == 200 and r.json() == {"handle": None, "commitments": [], "nonzero": [0], "first": [None]}
            assert client.worker_commit_expr([a], [["sqrt"]]).status_code == 400
            assert client.worker_commit_expr([a], wire([([(1, [0] * 9)],)])).status_code == 400
            assert client.worker_commit_expr([a], wire([([(1, [5])],)])).status_code == 400
            assert client.worker_commit_expr([a], wire(exprs[:1]), None, fr([1])).status_code == 400
            assert client.worker_release_rows(a).status_code == 200
            assert client.worker_commit_expr([a], wire(exprs[:1])).status_code == 400

    single.close()
    for client in (Client(seed=79), MultiDeviceClient(devices=[0], seed=79)):
        client.start(scale=scale, machines_scale=ms)
        try:
            through(client, range(M))
        finally:
            client.stop()
