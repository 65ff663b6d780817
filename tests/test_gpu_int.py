"""GPU tests (`-m gpu`) of kzg_rows_commit_int: bitwise ops, add / sub with carry and borrow, the two words of a product,
quotient and remainder, and the split at a shift, computed from the canonical integers of resident columns and committed on the
device.  The expected rows come from the definition in Python integers (tests/int_ref.py) and are committed with the C oracle,
never with the library under test.  Every case compares the commitments byte for byte, the values at probe indices and at one
random point through eval_rows, and the counts and first rows exactly.  Row lengths 2 .. 2^12: one lane per cell and 256 lanes
per workgroup, so 2^10 and 2^12 run 4 and 16 workgroups per op.  Each test leaves rows_stats() where it found it."""
import ctypes
import random

import pytest

from oracle import cpu as oc
from tests import grand_product_ref as gp
from tests import int_ref as iref
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release, srs_cache
from zkp_subnet_amd import _native
from zkp_subnet_amd.engine import HipEngine

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x1A7C0DE1, 0x1A7C0DE2


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def probes_of(T, rnd, usable=None):
    """the ends, the borders of the half waves, waves and workgroups, the rows around `usable` and three random rows"""
    ps = {0, 1 % T, T - 1} | {rnd.randrange(T) for _ in range(3)}
    ps |= {t for t in (31, 32, 63, 64, 255, 256) if t < T}
    if usable is not None:
        ps |= {max(usable - 1, 0), usable, min(usable + 1, T - 1)}
    return sorted(ps)


def check_set(eng, srs, rset, want, rnd, probes, i=0):
    """the set `rset` against its expected evaluation rows `want` (integers)"""
    w, T = len(want), len(want[0])
    assert (rset.k, rset.i, rset.T, len(rset.commitments)) == (w, i, T, w)
    wb = [row_bytes(r) for r in want]
    for c in range(w):
        assert rset.commitments[c] == oc.commit(srs, wb[c], True), c
    om = gp.omega(T)
    ts = sorted(set(probes))
    for t0 in range(0, len(ts), 4):
        part = ts[t0:t0 + 4]
        Y = eng.eval_rows([rset], [be(pow(om, t, R)) for t in part], [list(range(w))] * len(part))
        for t, ys in zip(part, Y):
            assert ys == [be(want[c][t]) for c in range(w)], t
    x = be(rnd.randrange(R))
    assert eng.eval_rows([rset], [x], [list(range(w))])[0] == [oc.fr_eval(oc.fr_ntt(b, True), x) for b in wb]


def run(eng, srs, cols, ops, rnd, usable=None, tail=(), sizes=None, ef=True):
    """commit `cols`, build on the device, check the new set, the counts and the first rows against the reference; returns
    (rows, counts, firsts)"""
    T = len(cols[0])
    want, counts, firsts = iref.int_columns(cols, ops, usable, tail)
    S = commit_sets(eng, cols, sizes or (len(cols),), ef)
    try:
        out, got_counts, got_firsts = eng.commit_int(S, ops, usable, bt(tail))
        try:
            assert got_counts == counts, (got_counts, counts)
            assert got_firsts == firsts, (got_firsts, firsts)
            probes = set(range(T)) if T <= 16 else set(probes_of(T, rnd, usable))
            if usable is not None:
                probes |= set(range(usable, T))
            check_set(eng, srs, out, want, rnd, probes)
        finally:
            out.release()
    finally:
        release(S)
    return want, counts, firsts


def edges(w):
    M = 1 << w
    return [0, 1, M - 1, M, (1 << 64) - 1, 1 << 64, R - 1]


def mixed_col(T, w, rnd):
    """random values below M, with the edge operands 0, 1, M - 1, M, 2^64 - 1, 2^64, r - 1 at random rows (all seven from
    T = 16 on, a random choice of them below)"""
    col = [rnd.randrange(1 << w) for _ in range(T)]
    es = edges(w)
    rnd.shuffle(es)
    for t, e in zip(rnd.sample(range(T), min(T, len(es)) if T >= 16 else T // 2), es):
        col[t] = e
    return col


def shift_col(T, w, rnd):
    """shifts in [0, w], with 0, w and the out-of-range w + 1 among them"""
    col = [rnd.randrange(w + 1) for _ in range(T)]
    for t, s in zip(rnd.sample(range(T), min(T, 3)), (w, 0, w + 1)):
        col[t] = s
    return col


# ---------------------------------------------------------------------------------------------------- every kind
@pytest.mark.parametrize("w", [1, 8, 32, 33, 64])
@pytest.mark.parametrize("lg", [1, 2, 4, 10, 12])
def test_every_kind(engines, srs_of, lg, w):
    """all eight kinds at one (T, w): the two-row kinds with both rows in one call (13 output rows) and with the first row alone
    in another; the columns mix values below M with the edge operands, so both calls count out-of-range cells"""
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(100 * lg + w)
    cols = [mixed_col(T, w, rnd), mixed_col(T, w, rnd), shift_col(T, w, rnd)]
    both = [("and", w, 0, 1), ("or", w, 0, 1), ("xor", w, 0, 1), ("add", w, 0, 1, 2), ("sub", w, 0, 1, 2), ("mul", w, 0, 1, 2),
            ("divmod", w, 0, 1, 2), ("split", w, 0, 2, 2)]
    want, counts, _ = run(eng, srs, cols, both, rnd)
    assert len(want) == 13
    M = 1 << w
    for t in range(T):
        a, b, s = cols[0][t] % M, cols[1][t] % M, min(cols[2][t], w)
        assert a + b == want[3][t] + want[4][t] * M and a - b == want[5][t] - want[6][t] * M
        assert a * b == want[7][t] + want[8][t] * M and a == want[11][t] * (1 << s) + want[12][t]
        assert (a == want[9][t] * b + want[10][t] and want[10][t] < b) if b else (want[9][t], want[10][t]) == (M - 1, a)
    if T >= 16:
        assert all(c >= 3 for c in counts)                         # M, 2^64 and r - 1 in a at least (2^64 - 1 too below w = 64)
    first = [(k, w, 0, 2 if k == "split" else 1) for k in ("add", "sub", "mul", "divmod", "split")]
    want1, counts1, _ = run(eng, srs, cols, first, rnd)
    assert want1 == [want[c] for c in (3, 5, 7, 9, 11)] and counts1 == counts[3:]
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- operands
@pytest.mark.parametrize("w", [32, 64])
def test_row_and_immediate_operands_and_one_row_as_both(engines, srs_of, w):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(2000 + w)
    M = 1 << w
    cols = [mixed_col(T, w, rnd), mixed_col(T, w, rnd)]
    k = rnd.randrange(1, M)
    for ops in ([("and", w, 0, ("imm", k)), ("or", w, 1, ("imm", 0)), ("xor", w, 0, ("imm", M - 1)), ("add", w, 0, ("imm", k), 2),
                 ("sub", w, 1, ("imm", k), 2), ("mul", w, 0, ("imm", M - 1), 2), ("divmod", w, 1, ("imm", k), 2),
                 ("divmod", w, 0, ("imm", 0), 2)],
                [("xor", w, 0, 0), ("and", w, 1, 1), ("add", w, 0, 0, 2), ("sub", w, 1, 1, 2), ("mul", w, 0, 0, 2),
                 ("divmod", w, 1, 1, 2), ("split", w, 0, 0, 2), ("or", w, 1, 0), ("or", w, 0, 1)]):
        want, counts, firsts = run(eng, srs, cols, ops, rnd)
        over = [sum(1 for x in c if x >= M) for c in cols]
        if ops[0][3] == 0:                                         # one row as both operands: a cell is counted once
            assert want[0] == [0] * T and want[1] == [x % M for x in cols[1]]
            assert want[4] == [0] * T and want[5] == [0] * T       # a - a, no borrow
            assert want[8] == [1 if x % M else M - 1 for x in cols[1]] and want[9] == [0] * T      # b / b; 0 / 0
            assert want[12] == want[13]
            assert counts[:6] == [over[0], over[1], over[0], over[1], over[0], over[1]]
        else:
            assert counts == [over[0], over[1], over[0], over[0], over[1], over[0], over[1], over[0]]
            assert want[11] == [M - 1] * T and want[12] == [x % M for x in cols[0]]
    assert eng.rows_stats() == before


@pytest.mark.parametrize("w", [8, 32, 64])
def test_divmod_zero_divisors_and_the_edges_of_the_quotient(engines, srs_of, w):
    """zero divisors at rows 0 and T - 1 and on a whole 64-lane group; divisor 1, divisor M - 1 and a < b elsewhere.  Every
    operand is below M: nothing is counted, a zero divisor least of all"""
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(3000 + w)
    M = 1 << w
    a = [rnd.randrange(M) for _ in range(T)]
    b = [rnd.randrange(1, M) for _ in range(T)]
    for t in [0, T - 1] + list(range(128, 192)):
        b[t] = 0
    for t in range(200, 232):
        b[t] = 1
    for t in range(300, 332):
        b[t] = M - 1
    a[300], a[301] = M - 1, M - 2
    for t in range(400, 464):
        a[t], b[t] = sorted((a[t], b[t]))[0], max(a[t], b[t], 1)   # a <= b
    a[400] = b[400] = M - 1
    want, counts, firsts = run(eng, srs, [a, b], [("divmod", w, 0, 1, 2), ("divmod", w, 0, 1)], rnd)
    assert counts == [0, 0] and firsts == [None, None]
    assert all(want[0][t] == M - 1 and want[1][t] == a[t] for t in [0, T - 1] + list(range(128, 192)))
    assert all(want[0][t] == a[t] and want[1][t] == 0 for t in range(200, 232))
    assert (want[0][300], want[1][300], want[0][301], want[1][301]) == (1, 0, 0, M - 2)
    assert all(want[0][t] == 0 and want[1][t] == a[t] for t in range(401, 464) if a[t] < b[t])
    assert want[2] == want[0]
    assert eng.rows_stats() == before


@pytest.mark.parametrize("w", [8, 33, 64])
def test_split_by_immediates_and_by_a_shift_column(engines, srs_of, w):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(4000 + w)
    M = 1 << w
    a = [rnd.randrange(M) for _ in range(T)]
    a[:3] = [M - 1, 0, 1]
    s = [(0, w, w + 1)[t % 3] for t in range(T)]                   # w + 1 is counted and taken as w
    ops = [("split", w, 0, ("imm", sh), 2) for sh in (0, 1, w - 1, w)] + [("split", w, 0, 1, 2), ("split", w, 0, 1)]
    want, counts, firsts = run(eng, srs, [a, s], ops, rnd)
    assert want[0] == a and want[1] == [0] * T                     # s = 0
    assert want[2] == [x >> 1 for x in a] and want[3] == [x & 1 for x in a]
    assert want[4] == [x >> (w - 1) for x in a] and want[5] == [x % (M >> 1) for x in a]
    assert want[6] == [0] * T and want[7] == a                     # s = w
    assert want[8] == [x if t % 3 == 0 else 0 for t, x in enumerate(a)] and want[10] == want[8]
    assert want[9] == [0 if t % 3 == 0 else x for t, x in enumerate(a)]
    n_over = len([t for t in range(T) if t % 3 == 2])
    assert counts == [0, 0, 0, 0, n_over, n_over] and firsts == [None] * 4 + [2, 2]
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- out of range
@pytest.mark.parametrize("lg", [2, 10])
def test_out_of_range_cells_are_reduced_counted_once_and_the_first_is_named(engines, srs_of, lg):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(5000 + lg)
    w, M = 32, 1 << 32
    clean = lambda: [rnd.randrange(M) for _ in range(T)]          # noqa: E731
    big = lambda: rnd.choice([M, M + 5, (1 << 64) - 1, 1 << 64, (1 << 64) + 7, R - 1, rnd.randrange(M, R)])   # noqa: E731
    ops = [("add", w, 0, 1, 2), ("xor", w, 0, 1), ("mul", w, 1, 0, 2)]
    for rows_a, rows_b in (([0], []), ([], [T - 1]), ([1], [1]), ([0, T - 1], [0, T - 2]), ([T - 1], []), ([], [])):
        a, b = clean(), clean()
        for t in rows_a:
            a[t] = big()
        for t in rows_b:
            b[t] = big()
        want, counts, firsts = run(eng, srs, [a, b], ops, rnd)
        flagged = sorted(set(rows_a) | set(rows_b))
        assert counts == [len(flagged)] * 3 and firsts == [flagged[0] if flagged else None] * 3
        assert want[2] == [(x ^ y) % M for x, y in zip(a, b)]       # the low w bits, whatever lies above them
    if T > 256:      # a flagged cell in every workgroup, and in the last one only
        a, b = clean(), clean()
        for t in (70, 300, 600, 1000):
            a[t] = big()
        assert run(eng, srs, [a, b], ops, rnd)[1:] == ([4] * 3, [70] * 3)
        a, b = clean(), clean()
        b[1000] = big()
        assert run(eng, srs, [a, b], ops, rnd)[1:] == ([1] * 3, [1000] * 3)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- mixed calls
def test_a_call_mixing_all_kinds_over_two_handles_gives_sixteen_rows(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(6000)
    cols = [mixed_col(T, 32, rnd), mixed_col(T, 32, rnd), shift_col(T, 32, rnd), mixed_col(T, 64, rnd), mixed_col(T, 8, rnd)]
    ops = [("xor", 32, 0, 1), ("add", 32, 0, 1, 2), ("sub", 32, 1, 0, 2), ("mul", 64, 3, 3, 2), ("divmod", 32, 0, 1, 2),
           ("split", 32, 0, 2, 2), ("and", 8, 4, ("imm", 0x0f)), ("or", 8, 4, 0), ("xor", 64, 3, 0), ("add", 32, 0, 1, 2)]
    want = None
    for sizes, ef in (((5,), True), ((2, 3), True), ((4, 1), False)):      # one set, two sets, coefficient form
        got, counts, _ = run(eng, srs, cols, ops, rnd, sizes=sizes, ef=ef)
        assert len(got) == 16 and (want is None or got == want)
        want = got
        assert got[1] == got[14] and got[2] == got[15]             # a source row named by several ops yields identical rows
    # one of the sets in coefficient form, the other in evaluation form; a handle named twice: rows 0 and 1 are one column
    S = commit_sets(eng, cols[:2], (2,), True) + commit_sets(eng, cols[2:], (3,), False)
    D = commit_sets(eng, cols[:1], (1,))
    try:
        out, counts, firsts = eng.commit_int(S, ops)
        try:
            assert (counts, firsts) == iref.int_columns(cols, ops)[1:]
            check_set(eng, srs, out, want, rnd, probes_of(T, rnd))
        finally:
            out.release()
        out, counts, firsts = eng.commit_int([D[0], D[0]], [("sub", 32, 0, 1, 2), ("xor", 32, 1, 0)])
        try:
            assert counts[0] == counts[1] == sum(1 for x in cols[0] if x >> 32)
            check_set(eng, srs, out, [[0] * T] * 3, rnd, probes_of(T, rnd))
        finally:
            out.release()
    finally:
        release(S + D)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the layout
@pytest.mark.parametrize("lg,u", [(4, 11), (10, (1 << 10) - 31)])
def test_usable_layout(engines, srs_of, lg, u):
    """The source rows behind `usable` hold out-of-range cells and a zero divisor, which would be counted (and would change the
    quotient row) if they were read; the tails are checked in place, column-major"""
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(7000 + lg)
    w, M = 32, 1 << 32
    a = [rnd.randrange(M) for _ in range(u)] + [R - 1, 1 << 64, M] * T
    b = [rnd.randrange(1, M) for _ in range(u)] + [0, R - 2, M + 1] * T
    s = [rnd.randrange(w + 1) for _ in range(u)] + [w + 1] * T
    cols = [a[:T], b[:T], s[:T]]
    ops = [("divmod", w, 0, 1, 2), ("xor", w, 0, 1), ("split", w, 0, 2, 2), ("add", w, 1, ("imm", M - 1), 2)]
    n_out = iref.n_out(ops)
    tail = [rnd.randrange(R) for _ in range(n_out * (T - u))]
    want, counts, firsts = run(eng, srs, cols, ops, rnd, u, tail)
    assert counts == [0] * 4 and firsts == [None] * 4
    for c in range(n_out):
        assert want[c][u:] == tail[c * (T - u):(c + 1) * (T - u)]
    # the last row read is out of range: it is counted, the row behind it is not
    cols[0][u - 1] = 1 << 64
    _, counts, firsts = run(eng, srs, cols, ops, rnd, u, tail)
    assert counts == [1, 1, 1, 0] and firsts == [u - 1, u - 1, u - 1, None]
    # read in full, the same columns count their rows behind `usable` too
    _, counts, firsts = run(eng, srs, cols, ops, rnd)
    assert counts == [T - u + 1] * 3 + [sum(1 for x in cols[1][u:] if x >= M)] and firsts == [u - 1] * 3 + [u + 1]
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 6
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    srs = oc.srs_gen(be(SEED_X), be(SEED_Y), lg + 1, 1, 0)
    rnd = random.Random(8000)
    cols = [mixed_col(T, 32, rnd), mixed_col(T, 32, rnd), shift_col(T, 32, rnd)]
    ops = [("mul", 32, 0, 1, 2), ("split", 32, 1, 2), ("xor", 32, 0, ("imm", 0xffff))]
    want, want_counts, want_firsts = iref.int_columns(cols, ops)
    want_c = [oc.commit(srs, row_bytes(r), True) for r in want]

    def fresh_ok(sets):
        out, counts, firsts = eng.commit_int(sets, ops)
        out.release()
        assert out.commitments == want_c and counts == want_counts and firsts == want_firsts

    I = commit_sets(eng, cols, (1, 2))
    fresh_ok(I)
    live = eng.rows_stats()
    lib = _native.load()
    E_ARG = _native.KZG_E_ARG
    hi = (ctypes.c_uint64 * 2)(I[0].handle, I[1].handle)
    c, h = ctypes.create_string_buffer(48 * 16), ctypes.c_uint64(0)
    cnt, fst = (ctypes.c_uint64 * 32)(), (ctypes.c_uint64 * 32)()
    AND, XOR, ADD, MUL, SPLIT, IMM = (_native.KZG_INT_AND, _native.KZG_INT_XOR, _native.KZG_INT_ADD, _native.KZG_INT_MUL,
                                      _native.KZG_INT_SPLIT, _native.KZG_INT_IMM)

    def raw(recs, opts=None, n=2, n_ops=None):
        arr = (_native.IntOp * max(len(recs), 1))(*[_native.IntOp(*r) for r in recs])
        return lib.kzg_rows_commit_int(eng._h, n, hi, len(recs) if n_ops is None else n_ops, arr,
                                       ctypes.byref(opts) if opts else None, c, cnt, fst, ctypes.byref(h))

    def refused(rc, why):
        msg = lib.kzg_last_error(eng._h)
        assert rc == E_ARG and msg.startswith(b"int: ") and why in msg, (rc, msg)
        assert eng.rows_stats() == live
        fresh_ok(I)

    # the ops: (kind, width, a, b, imm, flags, count)
    refused(raw([], n_ops=0), b"n_ops")
    refused(raw([(AND, 8, 0, 0, 0, 0, 1)] * 17), b"n_ops")
    refused(raw([(ADD, 8, 0, 1, 0, 0, 2)] * 8 + [(AND, 8, 0, 0, 0, 0, 1)]), b"n_out")            # 17 output rows
    refused(raw([(0, 8, 0, 1, 0, 0, 1)]), b"unknown kind")
    refused(raw([(9, 8, 0, 1, 0, 0, 1)]), b"unknown kind")
    refused(raw([(ADD, 0, 0, 1, 0, 0, 1)]), b"width must be in [1, 64]")
    refused(raw([(ADD, 65, 0, 1, 0, 0, 1)]), b"width must be in [1, 64]")
    refused(raw([(ADD, 8, 0, 1, 0, 0, 0)]), b"count must be")
    refused(raw([(ADD, 8, 0, 1, 0, 0, 3)]), b"count must be")
    for kind in (AND, _native.KZG_INT_OR, XOR):
        refused(raw([(kind, 8, 0, 1, 0, 0, 2)]), b"count must be")
    refused(raw([(ADD, 8, 3, 1, 0, 0, 1)]), b"a row must index")                                 # 3 rows: 0 .. 2
    refused(raw([(ADD, 8, 0, 3, 0, 0, 1)]), b"a row must index")
    refused(raw([(ADD, 8, 0, 1, 0, 0, 1), (MUL, 8, 2 ** 31, 0, 0, 0, 1)]), b"a row must index")
    refused(raw([(ADD, 8, 0, 0, 256, IMM, 1)]), b"immediate must be below")
    refused(raw([(MUL, 63, 0, 0, 1 << 63, IMM, 1)]), b"immediate must be below")
    refused(raw([(SPLIT, 8, 0, 0, 9, IMM, 1)]), b"immediate must be below")
    refused(raw([(SPLIT, 64, 0, 0, 65, IMM, 2)]), b"immediate must be below")
    refused(raw([(ADD, 8, 0, 1, 0, 2, 1)]), b"flags")
    refused(raw([(ADD, 8, 0, 1, 5, IMM, 1)]), b"row b must be 0")
    refused(raw([(ADD, 8, 0, 1, 5, 0, 1)]), b"immediate must be 0")
    refused(raw([(ADD, 8, 0, 1, 0, 0, 1)], n=0), b"number of handles")
    refused(raw([(ADD, 8, 0, 1, 0, 0, 1)], n=17), b"number of handles")
    # the largest immediates that fit are taken
    assert raw([(ADD, 64, 0, 0, (1 << 64) - 1, IMM, 2), (SPLIT, 64, 0, 0, 64, IMM, 2), (AND, 8, 0, 0, 255, IMM, 1)]) == 0
    eng.release_rows(h.value)
    assert eng.rows_stats() == live
    # the layout: every tail error of the derived call
    recs = [(MUL, 32, 0, 1, 0, 0, 2), (XOR, 32, 0, 2, 0, 0, 1)]
    tl = b"".join(bt([rnd.randrange(R) for _ in range(3 * 4)]))
    big = R.to_bytes(32, "big")
    for usable, tail, why in ((T, tl, b"usable must be in"), (2 ** 40, tl, b"usable must be in"),
                              (T - 33, tl, b"KZG_MAX_BLIND_ROWS"), (T - 4, None, b"tail_be32 must be given"),
                              (0, tl, b"plain layout"), (T - 4, tl[:-32] + big, b"canonical"),
                              (T - 4, b"\xff" * 32 + tl[32:], b"canonical")):
        refused(raw(recs, _native.DeriveOpts(usable, tail)), why)
    arg_error(lambda: eng.commit_int(I, ops, 0), "usable")
    arg_error(lambda: eng.commit_int(I, ops, T - 4, [be(1)] * 11), "exactly")
    arg_error(lambda: eng.commit_int(I, ops, None, [be(1)]), "tail needs usable")
    arg_error(lambda: eng.commit_int(I, [("nand", 8, 0, 1)]), "int: unknown kind")
    assert raw(recs, _native.DeriveOpts(0, None)) == 0             # usable = 0 spelled out: the plain layout
    ref = iref.int_columns(cols, [("mul", 32, 0, 1, 2), ("xor", 32, 0, 2)])
    assert list(cnt[:2]) == ref[1] and [None if v == _native.KZG_INT_NONE else v for v in fst[:2]] == ref[2]
    eng.release_rows(h.value)
    assert eng.rows_stats() == live
    # handles
    other = commit_sets(eng, cols[1:], (2,), i=1)                  # another worker
    arg_error(lambda: eng.commit_int([I[0]] + other, ops), "one worker")
    short = eng.commit_rows(0, [row_bytes(r[:T // 2]) for r in cols[1:]])      # another length
    arg_error(lambda: eng.commit_int([I[0], short], ops), "one worker and have one row length")
    release(other + [short])
    gone = commit_sets(eng, cols[1:], (2,))
    release(gone)
    arg_error(lambda: eng.commit_int([I[0]] + gone, ops), "released")
    arg_error(lambda: eng.commit_int([2 ** 40], [("and", 8, 0, 0)]), "unknown")
    arg_error(lambda: eng.commit_int(I * 6, ops), "KZG_MAX_BATCH_OPEN rows")    # 18 rows
    fresh_ok(I)
    # the 65th live set
    fill = [eng.commit_rows(0, [row_bytes(cols[0])]) for _ in range(_native.KZG_MAX_ROW_SETS - 2)]
    assert eng.rows_stats()[0] == _native.KZG_MAX_ROW_SETS
    arg_error(lambda: eng.commit_int(I, ops), "KZG_MAX_ROW_SETS", code=_native.KZG_E_BUSY)
    fill.pop().release()
    fresh_ok(I)
    release(fill)
    # stale after an SRS load
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.commit_int(I, ops), "SRS")
    release(I)
    I = commit_sets(eng, cols, (3,))
    out, counts, firsts = eng.commit_int(I, ops)
    assert out.commitments == want_c and counts == want_counts and firsts == want_firsts
    # the new set opens and combines like any other, goes stale and releases like any other
    x = be(rnd.randrange(R))
    ys, proofs = eng.open_rows([out], [x], [[0, 1, 2, 3]], [be(rnd.randrange(R))])[:2]
    assert ys[0] == [oc.fr_eval(oc.fr_ntt(row_bytes(r), True), x) for r in want] and len(proofs) == 1
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
    rnd = random.Random(9000)
    ops = [("mul", 32, 0, 1, 2), ("divmod", 32, 1, 0, 2), ("xor", 32, 0, ("imm", 0xff00ff00))]
    recs = HipEngine.int_ops(ops)
    arr = (_native.IntOp * len(recs))(*[_native.IntOp(*r) for r in recs])
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(1, (ctypes.c_int * 1)(0), ctypes.byref(mh)) == 0
    u = T - 3
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    none = lambda vs: [None if v == _native.KZG_INT_NONE else v for v in vs]   # noqa: E731
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        c, cc = ctypes.create_string_buffer(48 * 5), ctypes.create_string_buffer(96)
        cnt, fst = (ctypes.c_uint64 * 3)(), (ctypes.c_uint64 * 3)()
        made = {}
        for i in range(M):
            cols = [mixed_col(T, 32, rnd), mixed_col(T, 32, rnd)]
            tail = b"".join(bt([rnd.randrange(R) for _ in range(5 * (T - u))]))
            I = commit_sets(single, cols, (2,), i=i)
            plain, pc, pf = single.commit_int(I, ops)
            lay, lc, lf = single.commit_int(I, ops, u, [tail[j:j + 32] for j in range(0, len(tail), 32)])
            release(I + [plain, lay])
            hi, hz = ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 2, b"".join(row_bytes(r) for r in cols), T, 1, cc, ctypes.byref(hi)) == 0
            ai = (ctypes.c_uint64 * 1)(hi.value)
            assert lib.kzg_multi_rows_commit_int(mh, i, 1, ai, 3, arr, None, c, cnt, fst, ctypes.byref(hz)) == 0, i
            assert c.raw == b"".join(plain.commitments) and list(cnt) == pc and none(fst) == pf
            made[i] = [hi.value, hz.value]
            opts = _native.DeriveOpts(u, tail)
            assert lib.kzg_multi_rows_commit_int(mh, i, 1, ai, 3, arr, ctypes.byref(opts), c, cnt, fst, ctypes.byref(hz)) == 0, i
            assert c.raw == b"".join(lay.commitments) and list(cnt) == lc and none(fst) == lf
            made[i].append(hz.value)
        ai = (ctypes.c_uint64 * 1)(made[1][0])                     # worker 1's set under index 0
        assert lib.kzg_multi_rows_commit_int(mh, 0, 1, ai, 3, arr, None, c, cnt, fst, ctypes.byref(hz)) == _native.KZG_E_ARG
        for i in range(M):
            for hh in made[i]:
                assert lib.kzg_multi_rows_release(mh, i, hh) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)

    # the text clients over the engine: the same bytes as a commit of the reference rows
    def through(client, workers):
        for i in workers:
            cols = [mixed_col(T, 32, rnd), mixed_col(T, 32, rnd)]
            tail = [rnd.randrange(R) for _ in range(5 * (T - u))]
            a = client.worker_commit_rows(i, [fr(col) for col in cols]).json()["handle"]
            for usable, tl in ((None, []), (u, tail)):
                want, counts, firsts = iref.int_columns(cols, ops, usable, tl)
                ref = client.worker_commit_rows(i, [fr(col) for col in want]).json()
                r = client.worker_commit_int([a], [[op[0], op[1], op[2], list(op[3]) if isinstance(op[3], tuple) else op[3]]
                                                   + list(op[4:]) for op in ops], usable, fr(tl))
                assert r.status_code == 200, r.json()
                body = r.json()
                assert body["commitments"] == ref["commitments"] and body["counts"] == counts and body["first"] == firsts
                for hh in (ref["handle"], body["handle"]):
                    assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_int([a], [["nand", 8, 0, 1]]).status_code == 400
            assert client.worker_commit_int([a], [["and", 65, 0, 1]]).status_code == 400
            assert client.worker_commit_int([a], [["and", 8, 0, ["imm", 256]]]).status_code == 400
            assert client.worker_commit_int([a], [["and", 8, 0, 2]]).status_code == 400        # 2 rows: 0 and 1
            assert client.worker_commit_int([a], [["and", 8, 0, 1]], None, fr([1])).status_code == 400
            assert client.worker_release_rows(a).status_code == 200
            assert client.worker_commit_int([a], [["and", 8, 0, 1]]).status_code == 400

    single.close()
    for client in (Client(seed=79), MultiDeviceClient(devices=[0], seed=79)):
        client.start(scale=scale, machines_scale=ms)
        try:
            through(client, range(M))
        finally:
            client.stop()

