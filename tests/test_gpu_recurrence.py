"""GPU tests (`-m gpu`) of kzg_rows_commit_recurrence: columns v[t + 1] = A[t] v[t] + B[t] with A and B expressions in resident
columns, scanned and committed on the device.  The expected rows and closing values come from the definition in Python integers
(tests/recur_ref.py) and are committed with the C oracle, never with the library under test.  Every case compares the
commitments byte for byte, the values at probe rows and at one random point through eval_rows, and the closing values exactly.
No case goes above 2^14 rows.  Each test leaves rows_stats() where it found it."""
import ctypes
import random

import pytest

from oracle import cpu as oc
from tests import expr_ref as xref
from tests import recur_ref as rref
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release, srs_cache, x_call
from tests.test_gpu_derived import check_set, probes_of, rand_col
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0xEC0221D1, 0xEC0221D2
SHAPE_MSG = "the constraints do not hold"


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def bside(terms):
    return [(be(c), fs) for c, fs in terms]


def bx(recs):
    """integer-valued entries -> the engine's: 32-byte coefficients and starts"""
    return [(bside(m), bside(a), be(s)) for m, a, s in recs]


def run(eng, srs, cols, recs, rnd, usable=None, tail=(), sizes=None, ef=True, probes=None, keep=False):
    """commit `cols`, run the recurrences on the device, check the new set and the closing values against the reference;
    returns (rows, closings), with keep also the source sets and the new set (the caller releases them)"""
    T = len(cols[0])
    want, closings = rref.recurrence_columns(cols, recs, usable, tail)
    S = commit_sets(eng, cols, sizes or (len(cols),), ef)
    out = None
    try:
        out, got = eng.commit_recurrence(S, bx(recs), usable, bt(tail))
        assert got == [be(c) for c in closings]
        check_set(eng, srs, out, want, rnd, probes or probes_of(T, rnd, usable))
    finally:
        if not keep:
            release(S + ([out] if out is not None else []))
    return (want, closings, S, out) if keep else (want, closings)


def three_shapes(rnd):
    """a general recurrence, a running sum, a running product"""
    k = rnd.randrange(R)
    return [([(1, [0])], [(1, [1, 2]), (k, [])], rnd.randrange(R)), ([], [(1, [0])], rnd.randrange(R)), ([(1, [0])], [], rnd.randrange(1, R))]


# ---------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("lg", [1, 2, 6, 8, 10, 12, 14])
def test_geometry_general_sum_and_product(engines, srs_of, lg):
    """T = 2 and 4 (part of a wave), 2^6, 2^8 (one map per lane of the top kernel), 2^10 and 2^12 (the top kernel under one level),
    2^14 (the library's plan has a level between level 0 and the top)"""
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(100 + lg)
    cols = [rand_col(T, rnd) for _ in range(3)]
    recs = three_shapes(rnd)[:1 if lg == 14 else 3]
    want, closings = run(eng, srs, cols, recs, rnd, probes=range(T) if T <= 16 else None)
    assert want[0][0] == recs[0][2] and want[0][1] == (cols[0][0] * recs[0][2] + cols[1][0] * cols[2][0] + recs[0][1][1][0]) % R
    if lg < 14:
        assert want[1][T - 1] == (recs[1][2] + sum(cols[0][:T - 1])) % R and closings[1] == (recs[1][2] + sum(cols[0])) % R
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the usable layout
@pytest.mark.parametrize("lg,back", [(8, 1), (8, 32), (8, 5), (2, 1), (12, 32)])
def test_usable_layout_closing_row_tail_and_poisoned_rows(engines, srs_of, lg, back):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    u = T - back
    before = eng.rows_stats()
    rnd = random.Random(200 + 40 * lg + back)
    cols = [rand_col(T, rnd) for _ in range(3)]
    recs = three_shapes(rnd)
    tail = rand_col(3 * (T - u - 1), rnd)
    want, closings = run(eng, srs, cols, recs, rnd, u, tail, probes=range(T) if T <= 16 else None)
    for c in range(3):
        assert want[c][u] == closings[c]                                       # the closing row holds the returned value
        assert want[c][u + 1:] == tail[c * (T - u - 1):(c + 1) * (T - u - 1)]  # the tail sits behind it
    # the source rows at or behind u do not enter: poisoned, they give the same rows and closings
    poisoned = [col[:u] + [R - 1] * (T - u) for col in cols]
    again, cl2 = run(eng, srs, poisoned, recs, rnd, u, tail)
    assert again == want and cl2 == closings
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- counts of recurrences
def test_sixteen_recurrences_in_one_call_and_seventeen_refused(engines, srs_of):
    lg = 6
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(300)
    cols = [rand_col(T, rnd) for _ in range(2)]
    recs = [([(rnd.randrange(R), [0])], [(rnd.randrange(R), [1]), (e, [])], rnd.randrange(R)) for e in range(16)]
    u = T - 3
    run(eng, srs, cols, recs, rnd)
    run(eng, srs, cols, recs, rnd, u, rand_col(16 * 2, rnd))
    S = commit_sets(eng, cols, (2,))
    try:
        arg_error(lambda: eng.commit_recurrence(S, bx(recs + recs[:1])), "1 .. 16")
    finally:
        release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- rotations and sources
def test_rotated_factors_in_both_expressions(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(400)
    cols = [rand_col(T, rnd) for _ in range(2)]
    recs = [([(1, [(0, 1)]), (2, [(1, -1), 0])], [(1, [(1, T - 1)]), (R - 1, [(0, -(1 << 31))])], rnd.randrange(R)),
            ([(3, [(0, T + 1)])], [(1, [(1, 2), (1, -2)])], 7)]
    u = T - 9
    run(eng, srs, cols, recs, rnd)
    # a rotated factor of a row below u reads across u: the cells behind u matter here, and only through the rotation
    want, _ = run(eng, srs, cols, recs, rnd, u, rand_col(2 * 8, rnd))
    other = [col[:u + 1] + [5] * (T - u - 1) for col in cols]
    diff, _ = rref.recurrence_columns(other, recs, u, [0] * 16)
    assert diff[0][:u + 1] != want[0][:u + 1]
    assert eng.rows_stats() == before


def test_sources_over_two_sets_coefficient_form_and_a_repeated_handle(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(500)
    cols = [rand_col(T, rnd) for _ in range(4)]
    recs = [([(1, [0]), (1, [3])], [(2, [(3, 1), 0])], 11), ([], [(1, [3, 3])], 0)]   # rows 1 and 2: no term names them
    for sizes, ef in (((4,), True), ((1, 3), True), ((2, 2), False)):
        run(eng, srs, cols, recs, rnd, sizes=sizes, ef=ef)
    S = commit_sets(eng, cols[:1], (1,))
    try:
        out, cl = eng.commit_recurrence([S[0], S[0]], bx([([(1, [0])], [(1, [1])], 3)]))   # rows 0 and 1 are the same column
        try:
            want, closings = rref.recurrence_columns([cols[0], cols[0]], [([(1, [0])], [(1, [1])], 3)])
            check_set(eng, srs, out, want, rnd, probes_of(T, rnd))
            assert cl == [be(closings[0])]
        finally:
            out.release()
    finally:
        release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("lg", [1, 8, 12])
def test_start_zero_start_r_minus_one_zero_multipliers_and_extreme_cells(engines, srs_of, lg):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(600 + lg)
    a = rand_col(T, rnd)
    for t in range(0, T, 5):
        a[t] = 0                                                                # restarts, the first row among them
    cols = [a, rand_col(T, rnd), [R - 1] * T, [0] * T]
    recs = [([(1, [0])], [(1, [1])], 0), ([(1, [0])], [(1, [1])], R - 1),
            ([(R - 1, [2])], [(R - 1, [2, 2]), (R - 1, [])], R - 1),             # every cell and every coefficient r - 1
            ([(1, [3])], [(1, [1])], 9), ([(1, [0])], [(1, [3])], 9)]            # A = 0 everywhere; B = 0 everywhere
    want, closings = run(eng, srs, cols, recs, rnd, probes=range(T) if T <= 16 else None)
    assert want[0][1:] == want[1][1:]                                           # row 0 restarts: the start does not matter
    assert want[3][1:] == cols[1][:T - 1] and closings[3] == cols[1][T - 1]
    assert want[4][0] == 9 and want[4][1:] == [0] * (T - 1)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the use case
def test_running_sum_decomposition_with_segment_restarts_over_derived_limbs(engines, srs_of):
    """Every 8 rows a 32-bit value x_s sits in cell 8 s of X.  kzg_rows_commit_derived gives its four 8-bit limbs as four columns;
    the running sum z' = (z - k) 2^-8 walks them along the rows of the segment (limb j read at rotation -j under the selector
    S_j), reaches 0 after the fourth limb, stays 0, and restarts at x_(s+1) on the segment's last row."""
    lg = 8
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(700)
    X = [rnd.randrange(1 << 32) if t % 8 == 0 else 0 for t in range(T)]
    X[8] = (1 << 32) - 1
    S = [[int(t % 8 == j) for t in range(T)] for j in range(4)]
    q = [int(t % 8 < 4) for t in range(T)]
    rs = [int(t % 8 == 7) for t in range(T)]
    inv = pow(1 << 8, -1, R)
    base = commit_sets(eng, [X, q, rs] + S, (7,))
    made = list(base)
    try:
        limbs, counts = eng.commit_derived(base[:1], [("limbs", 0, 8, 4)])
        made.append(limbs)
        assert counts == [0]
        limb_cols = [[(x >> (8 * j)) & 255 for x in X] for j in range(4)]
        mul = [(inv, [1])]
        add = [(R - inv, [3 + j, (7 + j, -j)]) for j in range(4)] + [(1, [2, (0, 1)])]
        want, closings = rref.recurrence_columns([X, q, rs] + S + limb_cols, [(mul, add, X[0])])
        assert all(want[0][8 * s] == X[8 * s] and want[0][8 * s + 4:8 * s + 8] == [0] * 4 for s in range(T // 8))
        assert closings == [X[0]]                                               # the last segment restarts at x_0: the column is cyclic
        out, cl = eng.commit_recurrence([base[0], limbs], bx([(mul, add, X[0])]))
        made.append(out)
        check_set(eng, srs, out, want, rnd, probes_of(T, rnd))
        assert cl == [be(X[0])]
        # a value of 33 bits: the fourth limb leaves a remainder, the segment's final value is not 0
        X2 = list(X)
        X2[16] = 1 << 32
        limbs2 = [[(x >> (8 * j)) & 255 for x in X2] for j in range(4)]
        want2, _ = rref.recurrence_columns([X2, q, rs] + S + limbs2, [(mul, add, X[0])])
        assert want2[0][20] == (1 << 32) * pow(inv, 4, R) % R == 1
    finally:
        release(made)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- end to end
def test_a_cyclic_column_passes_the_quotient_of_its_gate_and_a_changed_cell_is_refused(engines):
    lg = 10
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(800)
    a, b, start = rand_col(T, rnd), rand_col(T, rnd), rnd.randrange(R)
    v = rref.scan(a[:T - 1], b[:T - 1], start)
    b[T - 1] = (start - a[T - 1] * v[T - 1]) % R                                # v[T] = start: the relation holds on all of H
    gate = [(1, [(2, 1)]), (R - 1, [0, 2]), (R - 1, [1])]
    rec = [([(1, [0])], [(1, [1])], start)]
    made = []
    try:
        S = commit_sets(eng, [a, b], (2,))
        made += S
        V, cl = eng.commit_recurrence(S, bx(rec))
        made.append(V)
        assert cl == [be(start)]
        made.append(x_call(eng, S + [V], gate, None, None, 1, 1))
        b2 = list(b)
        b2[T // 2] = (b2[T // 2] + 1) % R
        S2 = commit_sets(eng, [a, b2], (2,))
        made += S2
        arg_error(lambda: x_call(eng, S2 + [V], gate, None, None, 1, 1), SHAPE_MSG)
        W, cl2 = eng.commit_recurrence(S2, bx(rec))                             # the changed column is no longer cyclic
        made.append(W)
        assert cl2 != [be(start)]
        arg_error(lambda: x_call(eng, S2 + [W], gate, None, None, 1, 1), SHAPE_MSG)
    finally:
        release(made)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- refusals
def raw32(v):
    """32 big-endian bytes WITHOUT a reduction (be() reduces: a scalar >= r has to reach the library as it is)"""
    return int(v).to_bytes(32, "big")


def c_side(terms, keep, rots=True):
    if not terms:
        return _native.QuotientTerms(0, None, None, None, None)
    flat = [xref.factor(f) for _, fs in terms for f in fs]
    la = (ctypes.c_uint32 * len(terms))(*[len(fs) for _, fs in terms])
    ra = (ctypes.c_uint32 * max(len(flat), 1))(*[j for j, _ in flat])
    ro = (ctypes.c_int32 * max(len(flat), 1))(*[rot for _, rot in flat]) if rots else None
    keep.append((la, ra, ro))
    return _native.QuotientTerms(len(terms), b"".join(raw32(c) for c, _ in terms), la, ra, ro)


def c_recs(recs, keep):
    return (_native.Recurrence * len(recs))(*[_native.Recurrence(c_side(m, keep), c_side(a, keep), raw32(s)) for m, a, s in recs])


def test_every_refusal_leaves_the_context_serving(engines, srs_of):
    lg = 6
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(900)
    cols = [rand_col(T, rnd) for _ in range(2)]
    good = [([(1, [0])], [(1, [1])], 5)]
    S = commit_sets(eng, cols, (2,))
    lib, keep = eng._lib, []
    hs = (ctypes.c_uint64 * 1)(S[0].handle)
    c, cl, h = ctypes.create_string_buffer(48 * 16), ctypes.create_string_buffer(32 * 16), ctypes.c_uint64(0)

    def raw(recs_arr, n, opts=None, handles=hs, nh=1):
        rc = lib.kzg_rows_commit_recurrence(eng._h, nh, handles, n, recs_arr, ctypes.byref(opts) if opts is not None else None,
                                            c, cl, ctypes.byref(h))
        return rc, lib.kzg_last_error(eng._h).decode()

    def refused(recs, why, opts=None, n=None):
        arr = c_recs(recs, keep) if not isinstance(recs, ctypes.Array) else recs
        rc, msg = raw(arr, len(recs) if n is None else n, opts)
        assert rc == _native.KZG_E_ARG and msg.startswith("recur:") and why in msg, (rc, msg)

    try:
        refused(good, "n_recs", n=0)
        refused(c_recs(good * 17, keep), "n_recs", n=17)
        refused([([], [], 5)], "both be empty")
        refused([([(1, [0])] * 17, [], 5)], "n_terms")
        refused([([(1, [0] * 9)], [], 5)], "KZG_MAX_EXPR_FACTORS")
        refused([([(1, [0])], [(1, [2])], 5)], "a row must index")
        refused([([(R, [0])], [], 5)], "canonical")
        refused([([(1, [0])], [(R, [])], 5)], "canonical")
        refused([([(1, [0])], [], R)], "start must be a canonical")
        arr = c_recs(good, keep)
        arr[0].start_be32 = None
        refused(arr, "start_be32")
        arr = c_recs(good, keep)
        arr[0].add.term_lens = None
        refused(arr, "term_lens")
        arr = c_recs(good, keep)
        arr[0].mul.term_rows = None
        refused(arr, "term_rows")
        tail1 = be(1)
        refused(good, "usable must be in [1, T - 1]", _native.RecurrenceOpts(T, None))
        refused(good, "KZG_MAX_BLIND_ROWS", _native.RecurrenceOpts(T - 33, b"".join(bt([1] * 32))))
        refused(good, "may be null only when usable = T - 1", _native.RecurrenceOpts(T - 2, None))
        refused(good, "tail scalars must be canonical", _native.RecurrenceOpts(T - 2, raw32(R)))
        refused(good, "must be null in the plain layout", _native.RecurrenceOpts(0, tail1))
        rc, msg = raw(c_recs(good, keep), 1, handles=(ctypes.c_uint64 * 1)(0xdead))
        assert rc == _native.KZG_E_ARG, (rc, msg)
        # null outputs and no handles: refused before anything is read
        assert lib.kzg_rows_commit_recurrence(eng._h, 1, hs, 1, c_recs(good, keep), None, None, cl, ctypes.byref(h)) == _native.KZG_E_ARG
        assert lib.kzg_rows_commit_recurrence(eng._h, 1, hs, 1, c_recs(good, keep), None, c, None, ctypes.byref(h)) == _native.KZG_E_ARG
        assert raw(c_recs(good, keep), 1, nh=0)[0] == _native.KZG_E_ARG
        # term_rots NULL: every rotation 0; and the context still serves
        arr = (_native.Recurrence * 1)(_native.Recurrence(c_side(good[0][0], keep, False), c_side(good[0][1], keep, False), be(5)))
        rc, msg = raw(arr, 1)
        assert rc == 0, msg
        want, closings = rref.recurrence_columns(cols, good)
        assert cl.raw[:32] == be(closings[0]) and c.raw[:48] == oc.commit(srs, row_bytes(want[0]), True)
        assert lib.kzg_rows_release(eng._h, h.value) == 0
        # the engine's own refusals
        arg_error(lambda: eng.commit_recurrence(S, bx(good), T - 2, []), "exactly")
        arg_error(lambda: eng.commit_recurrence(S, bx(good), None, bt([1])), "a tail needs usable")
        arg_error(lambda: eng.commit_recurrence(S, bx([([], [], 5)])), "both be empty")
        run(eng, srs, cols, good, rnd)
    finally:
        release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the other layers
def test_client_multi_handle_and_multi_device_client_return_the_engine_bytes(hip):
    from zkp_subnet_amd import Client, MultiDeviceClient, codec
    from zkp_subnet_amd.engine import lagrange_factor

    lib = _native.load()
    scale, ms = 8, 1
    T, M = 1 << (scale - ms), 1 << ms
    tx, ty = 0xABCDEF0999, 0x13579BF9
    rnd = random.Random(1000)
    recs = [([(1, [0]), (R - 2, [(1, -1)])], [(1, [0, 1])], 17), ([], [(3, []), (1, [(0, 1), 1])], R - 1), ([(2, [1])], [], 1)]
    keep = []
    arr = c_recs(recs, keep)
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(1, (ctypes.c_int * 1)(0), ctypes.byref(mh)) == 0
    u = T - 3
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        c, cl, cc = ctypes.create_string_buffer(48 * 3), ctypes.create_string_buffer(32 * 3), ctypes.create_string_buffer(96)
        made = {}
        for i in range(M):
            cols = [rand_col(T, rnd), rand_col(T, rnd)]
            tail = b"".join(bt(rand_col(3 * (T - u - 1), rnd)))
            I = commit_sets(single, cols, (2,), i=i)
            plain, pc = single.commit_recurrence(I, bx(recs))
            lay, lc = single.commit_recurrence(I, bx(recs), u, [tail[j:j + 32] for j in range(0, len(tail), 32)])
            want, closings = rref.recurrence_columns(cols, recs)
            assert pc == [be(x) for x in closings]
            release(I + [plain, lay])
            hi, hz = ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 2, b"".join(row_bytes(r) for r in cols), T, 1, cc, ctypes.byref(hi)) == 0
            ai = (ctypes.c_uint64 * 1)(hi.value)
            assert lib.kzg_multi_rows_commit_recurrence(mh, i, 1, ai, 3, arr, None, c, cl, ctypes.byref(hz)) == 0, i
            assert c.raw == b"".join(plain.commitments) and cl.raw == b"".join(pc)
            made[i] = [hi.value, hz.value]
            opts = _native.RecurrenceOpts(u, tail)
            assert lib.kzg_multi_rows_commit_recurrence(mh, i, 1, ai, 3, arr, ctypes.byref(opts), c, cl, ctypes.byref(hz)) == 0, i
            assert c.raw == b"".join(lay.commitments) and cl.raw == b"".join(lc)
            made[i].append(hz.value)
        ai = (ctypes.c_uint64 * 1)(made[1][0])                     # worker 1's set under index 0
        assert lib.kzg_multi_rows_commit_recurrence(mh, 0, 1, ai, 3, arr, None, c, cl, ctypes.byref(hz)) == _native.KZG_E_ARG
        for i in range(M):
            for hh in made[i]:
                assert lib.kzg_multi_rows_release(mh, i, hh) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)

    # the text clients over the engine: the same bytes as a commit of the reference rows
    def wside(terms):
        return [[codec.be32_to_fr(be(cf)), [list(f) if isinstance(f, tuple) else f for f in fs]] for cf, fs in terms]

    def wire(rs):
        return [[wside(m), wside(a), codec.be32_to_fr(be(s))] for m, a, s in rs]

    def through(client, workers):
        for i in workers:
            cols = [rand_col(T, rnd), rand_col(T, rnd)]
            tail = rand_col(3 * (T - u - 1), rnd)
            a = client.worker_commit_rows(i, [fr(col) for col in cols]).json()["handle"]
            for usable, tl in ((None, []), (u, tail)):
                want, closings = rref.recurrence_columns(cols, recs, usable, tl)
                ref = client.worker_commit_rows(i, [fr(col) for col in want]).json()
                r = client.worker_commit_recurrence([a], wire(recs), usable, fr(tl))
                assert r.status_code == 200, r.json()
                assert r.json()["commitments"] == ref["commitments"]
                assert r.json()["closings"] == fr(closings)
                for hh in (ref["handle"], r.json()["handle"]):
                    assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_recurrence([a], [["sqrt"]]).status_code == 400
            assert client.worker_commit_recurrence([a], wire([([], [], 1)])).status_code == 400
            assert client.worker_commit_recurrence([a], wire([([(1, [0] * 9)], [], 1)])).status_code == 400
            assert client.worker_commit_recurrence([a], wire([([(1, [5])], [], 1)])).status_code == 400
            assert client.worker_commit_recurrence([a], wire(recs[:1]), None, fr([1])).status_code == 400
            assert client.worker_release_rows(a).status_code == 200
            assert client.worker_commit_recurrence([a], wire(recs[:1])).status_code == 400

    single.close()
    for client in (Client(seed=81), MultiDeviceClient(devices=[0], seed=81)):
        client.start(scale=scale, machines_scale=ms)
        try:
            through(client, range(M))
        finally:
            client.stop()
