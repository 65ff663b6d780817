"""GPU tests (`-m gpu`) of kzg_rows_commit_fetch: columns read out of a resident table by key (the hash join of the
multiplicities call, walked by a probe that copies) or by row index, built and committed on the device.  The expected rows come
from the definition in Python integers (tests/fetch_ref.py: a dict from key tuple to the smallest row) and are committed with the
C oracle, never with the library under test.  Every case compares the commitments byte for byte, the values at probe indices
and at one random point through eval_rows, and `missing` / `first_missing` exactly.  Row lengths 2 .. 2^12: the join has no
path that depends on a larger size.  Each test leaves rows_stats() where it found it."""
import ctypes
import random

import pytest

from oracle import cpu as oc
from tests import fetch_ref as fref
from tests import sorted_ref as sref
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release, srs_cache
from tests.test_gpu_derived import check_set, probes_of, rand_col
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0xFE7C4ED1, 0xFE7C4ED2
ONE = be(1)


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def run(eng, srs, ins, table, n_reads, n_keys, index, rnd, usable=None, tail=(), in_sizes=None, tab_sizes=None, ef=True,
        probes=None):
    """commit `ins` and `table`, fetch on the device, check the new set and the counts against the reference; returns (rows,
    missing, first_missing)"""
    T = len(table[0])
    want, missing, first = fref.fetched_columns(ins, table, n_reads, n_keys, index, usable, tail)
    I = commit_sets(eng, ins, in_sizes or (len(ins),), ef)
    TB = commit_sets(eng, table, tab_sizes or (len(table),), ef)
    try:
        out, got_m, got_f = eng.commit_fetch(I, TB, n_reads, n_keys, index, usable, bt(tail))
        try:
            assert (got_m, got_f) == (missing, first), (got_m, got_f, missing, first)
            check_set(eng, srs, out, want, rnd, probes or (range(T) if T <= 16 else probes_of(T, rnd, usable)))
        finally:
            out.release()
    finally:
        release(I + TB)
    return want, missing, first


def small(rnd):
    """a key entry: mostly from a small domain (so that tuples repeat and hit), sometimes a full-width value"""
    return rnd.randrange(4) if rnd.randrange(8) else rnd.randrange(R)


def key_table(T, n_keys, n_pay, rnd):
    return [[small(rnd) for _ in range(T)] for _ in range(n_keys)] + [rand_col(T, rnd) for _ in range(n_pay)]


def reads_of(table, T, n_keys, n_reads, rnd, hit=0.75):
    """n_reads * n_keys input columns: a cell copies the key of a random table row, or is drawn like a table key"""
    ins = []
    for _ in range(n_reads):
        cols = [[0] * T for _ in range(n_keys)]
        for t in range(T):
            q = rnd.randrange(T) if rnd.random() < hit else None
            for c in range(n_keys):
                cols[c][t] = table[c][q] if q is not None else small(rnd)
        ins += cols
    return ins


# ---------------------------------------------------------------------------------------------------- by key
SHAPES = [(1, 1, 1, False), (2, 1, 2, False), (1, 3, 1, True), (3, 0, 1, True), (1, 15, 1, False), (4, 1, 3, False)]


@pytest.mark.parametrize("lg", [1, 2, 4, 10, 12])
@pytest.mark.parametrize("n_keys,n_pay,n_reads,index", SHAPES, ids=["1k1p", "2k1p2r", "1k3p+i", "3k0p+i", "1k15p", "4k1p3r"])
def test_by_key(engines, srs_of, lg, n_keys, n_pay, n_reads, index):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(100 * lg + 10 * n_keys + n_pay + n_reads)
    table = key_table(T, n_keys, n_pay, rnd)
    ins = reads_of(table, T, n_keys, n_reads, rnd)
    want, missing, _ = run(eng, srs, ins, table, n_reads, n_keys, index, rnd)
    assert len(want) == n_reads * (n_pay + index)
    if lg >= 10:
        assert all(0 < m < T for m in missing)                    # both branches ran in every read
    assert eng.rows_stats() == before


def test_tables_and_inputs_that_can_break_a_join(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(2000)
    pay = rand_col(T, rnd)
    # every cell hits its own row (distinct keys, a permutation of them asked for); every cell misses
    keys = rnd.sample(range(1 << 40), T)
    asked = keys[:]
    rnd.shuffle(asked)
    want, missing, first = run(eng, srs, [asked], [keys, pay], 1, 1, True, rnd)
    assert missing == [0] and first == [None] and sorted(want[0]) == list(range(T))
    want, missing, first = run(eng, srs, [[k + (1 << 41) for k in asked]], [keys, pay], 1, 1, True, rnd)
    assert missing == [T] and first == [0] and want == [[0] * T, [0] * T]
    # one key at rows {0, T - 1} and another inside one wave (rows 5 and 9): the index column shows the smaller row
    keys2 = keys[:]
    keys2[T - 1] = keys2[0]
    keys2[9] = keys2[5]
    asked2 = [keys2[0], keys2[T - 1], keys2[9], keys2[5]] * (T // 4)
    want, missing, _ = run(eng, srs, [asked2], [keys2, pay], 1, 1, True, rnd)
    assert missing == [0] and want[0][:4] == [0, 0, 5, 5] and want[1][:4] == [pay[0], pay[0], pay[5], pay[5]]
    # keys that differ in one limb only (all eight words), and tuples that differ in the last key column only
    base = rnd.randrange(1 << 250)
    limb_keys = [base ^ (1 << (31 * (t % 8) + t // 8 % 31)) for t in range(T)]       # one of 248 bits, in every 32-bit word
    assert len(set(limb_keys)) == 248 and max(limb_keys) < R
    asked3 = [limb_keys[rnd.randrange(T)] for _ in range(T - 1)] + [base]          # base itself is no row
    want, missing, first = run(eng, srs, [asked3], [limb_keys, pay], 1, 1, True, rnd)
    assert missing == [1] and first == [T - 1] and all(q < 248 for q in want[0])
    same = [base] * T
    last = list(range(T))
    want, missing, _ = run(eng, srs, [same, same, [T - 1 - t for t in range(T)]], [same, same, last, pay], 1, 3, False, rnd)
    assert missing == [0] and want[0] == pay[::-1]
    # keys 0 and r - 1; payload 0 on a hit: only the count tells it from a miss
    ends = [0, R - 1] + rnd.sample(range(1, 1 << 30), T - 2)
    zpay = [0, 0] + pay[2:]
    asked4 = [(0, R - 1, 1 << 31, R - 2)[t % 4] for t in range(T)]
    want, missing, first = run(eng, srs, [asked4], [ends, zpay], 1, 1, False, rnd)
    assert want == [[0] * T] and missing == [T // 2] and first == [2]
    assert eng.rows_stats() == before


def test_counting_borders(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(3000)
    keys, pay = list(range(7, 7 + T)), rand_col(T, rnd)

    def read(misses):
        return [0 if t in misses else keys[rnd.randrange(T)] for t in range(T)]

    borders = {0, 63, 64, 255, 256, T - 1}
    _, missing, first = run(eng, srs, [read(borders)], [keys, pay], 1, 1, False, rnd, probes=sorted(borders | {1, 62, 65, 254, 257}))
    assert missing == [6] and first == [0]
    # the first miss in the second workgroup only; a whole wave of misses; two reads with different counts, one without a miss
    wave = set(range(320, 384))
    _, missing, first = run(eng, srs, [read({300, 700}), read(wave), read(set()), read({T - 1})], [keys, pay], 4, 1, True, rnd)
    assert missing == [2, 64, 0, 1] and first == [300, 320, None, T - 1]
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- by row index
@pytest.mark.parametrize("lg", [1, 4, 10, 12])
def test_by_index(engines, srs_of, lg):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(4000 + lg)
    table = [rand_col(T, rnd) for _ in range(2)]
    special = [0, T - 1, T, (1 << 32) + 3, 1 << 64, R - 1, (1 << 32) + T - 1, 1 << 27, (1 << 255) % R]
    addr = (special + [rnd.randrange(T) for _ in range(T)])[:T]
    want, missing, first = run(eng, srs, [addr], table, 1, 0, False, rnd, probes=range(min(T, 16)))
    assert missing == [sum(1 for a in addr if a >= T)] and first == [next((t for t, a in enumerate(addr) if a >= T), None)]
    if T >= 16:
        assert want[0][:9] == [table[0][0], table[0][T - 1]] + [0] * 7 and missing == [7] and first == [2]
    # a permutation of range(T), read through its inverse, and two reads in one call
    perm = list(range(T))
    rnd.shuffle(perm)
    inv = [0] * T
    for q, t in enumerate(perm):
        inv[t] = q
    want, missing, first = run(eng, srs, [inv, perm], [perm], 2, 0, False, rnd)
    assert want[0] == list(range(T)) and missing == [0, 0] and first == [None, None]
    assert eng.rows_stats() == before


def test_by_index_with_sixteen_payload_columns(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(4100)
    table = [rand_col(T, rnd) for _ in range(16)]
    addr = [rnd.randrange(T + T // 8) for _ in range(T)]
    want, missing, _ = run(eng, srs, [addr], table, 1, 0, False, rnd, tab_sizes=(5, 11))
    assert len(want) == 16 and 0 < missing[0] < T
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the layout
@pytest.mark.parametrize("u", [1, (1 << 10) - 32, (1 << 10) - 1])
def test_usable_layout(engines, srs_of, u):
    """The cells behind `usable` ask for keys that stand in the table, and the table rows behind `usable` hold keys that cells
    below it ask for: both would show in the rows and the counts if they were read.  The tails are checked in place,
    column-major.  T - usable <= KZG_MAX_BLIND_ROWS is part of the call's contract: usable = 1 is its refusal at T = 2^10 and runs
    at T = 4."""
    rnd = random.Random(5000 + u)
    for lg in (10, 2):
        eng, srs, T = engines(lg), srs_of(lg), 1 << lg
        before = eng.rows_stats()
        if u >= T:
            continue
        keys = list(range(100, 100 + T))
        table = [keys, rand_col(T, rnd), rand_col(T, rnd)]
        asked = [keys[rnd.randrange(u)] for _ in range(T)]
        asked[0] = keys[u]                                           # stands in the table, but behind `usable`: a miss
        asked[u // 2] = keys[T - 1]
        n_cols = 2 * 3 + 2                                           # by key: 2 reads of index + 2 payload; by index: 2 columns
        tail = rand_col(n_cols * (T - u), rnd)
        addr = [rnd.randrange(u) for _ in range(T)]
        addr[0], addr[u - 1] = u, T - 1                              # addressable in the plain layout only
        if T - u > _native.KZG_MAX_BLIND_ROWS:
            S = commit_sets(eng, [asked] + table, (1, 3))
            arg_error(lambda: eng.commit_fetch(S[:1], S[1:], 1, 1, True, u, bt(tail[:3 * (T - u)])), "KZG_MAX_BLIND_ROWS")
            release(S)
        else:
            probes = set(probes_of(T, rnd, u)) | set(range(u, T))
            want, missing, first = run(eng, srs, [asked, keys], table, 2, 1, True, rnd, u, tail[:6 * (T - u)], probes=probes)
            assert missing == [len({0, u // 2}), 0] and first == [0, None]
            for c in range(6):
                assert want[c][u:] == tail[c * (T - u):(c + 1) * (T - u)]
            want, missing, first = run(eng, srs, [addr], table[1:], 1, 0, False, rnd, u, tail[6 * (T - u):], probes=probes)
            assert missing == [len({0, u - 1})] and first == [0]
            assert want[1][u:] == tail[7 * (T - u):]
        assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- sets
def test_one_set_several_sets_coefficient_form_and_shared_handles(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(6000)
    table = key_table(T, 2, 2, rnd)
    ins = reads_of(table, T, 2, 2, rnd)
    ref = None
    for in_sizes, tab_sizes, ef in (((4,), (4,), True), ((1, 3), (2, 2), True), ((2, 2), (1, 1, 2), False)):
        got = run(eng, srs, ins, table, 2, 2, True, rnd, in_sizes=in_sizes, tab_sizes=tab_sizes, ef=ef)
        assert ref is None or got == ref
        ref = got
    # a handle named twice: both reads are the same columns; and the table and the input being the same set: every cell of
    # column 0 finds itself, or the first row that holds its key
    S = commit_sets(eng, table[:1] + table[2:3], (2,))
    try:
        out, missing, first = eng.commit_fetch([S[0]], [S[0]], 2, 1, True)
        try:
            want, wm, wf = fref.fetched_columns([table[0], table[2]], [table[0], table[2]], 2, 1, True)
            assert (missing, first) == (wm, wf) and missing[0] == 0 and want[0] == [table[0].index(k) for k in table[0]]
            check_set(eng, srs, out, want, rnd, probes_of(T, rnd))
        finally:
            out.release()
        out, missing, _ = eng.commit_fetch([S[0], S[0]], [S[0]], 4, 1)
        try:
            assert out.k == 4 and out.commitments[0] == out.commitments[2] and out.commitments[1] == out.commitments[3]
            assert missing[0] == missing[2] == 0 and missing[1] == missing[3]
        finally:
            out.release()
    finally:
        release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- end to end
def copy_rows(eng, sets, order):
    """the rows `order` of the concatenated sets as a new set (commit_expr of the one-factor terms): handles name whole sets"""
    out, _, _ = eng.commit_expr(sets, [([(ONE, [j])],) for j in order])
    return out


def test_xor_from_the_byte_columns_to_the_closed_lookup_sum(engines, srs_of):
    """two 8-bit columns -> their nibbles (limbs of 4 bits) -> ONE fetch of two reads, one per nibble pair, against the resident
    256-row table (a, b, a ^ b) padded with repeats of row 0 -> the multiplicities of (a, b, c) -> a running sum that closes"""
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(7000)
    x, y = rand_col(T, rnd, 256), rand_col(T, rnd, 256)
    ta = [q >> 4 if q < 256 else 0 for q in range(T)]
    tb = [q & 15 if q < 256 else 0 for q in range(T)]
    X, TAB = commit_sets(eng, [x, y, ta, tb, [a ^ b for a, b in zip(ta, tb)]], (2, 3))
    made = [X, TAB]
    try:
        N, over = eng.commit_derived([X], [("limbs", 0, 4, 2), ("limbs", 1, 4, 2)])      # x_lo, x_hi, y_lo, y_hi
        made.append(N)
        assert over == [0, 0]
        C, missing, first = eng.commit_fetch([N], [TAB], 2, 2)
        made.append(C)
        assert missing == [0, 0] and first == [None, None]
        check_set(eng, srs, C, [[(v & 15) ^ (v >> 4) for v in col] for col in (x, y)], rnd, probes_of(T, rnd))
        W = copy_rows(eng, [N, C], (0, 1, 4, 2, 3, 5))                # lookup-major: (x_lo, x_hi, c_x), (y_lo, y_hi, c_y)
        made.append(W)
        m, mm = eng.commit_multiplicities([W], [TAB], 2, 3)
        made.append(m)
        assert mm == 0
        s, closing = eng.commit_lookup_sum([W], [TAB], m, 2, 3, be(rnd.randrange(R)), be(rnd.randrange(R)))
        made.append(s)
        assert closing == be(0)
        # one nibble forced to 16: no table row answers, the cell reads 0 and every count shows it
        t = 700
        nib = [[v & 15 for v in x], [v >> 4 for v in x], [v & 15 for v in y], [v >> 4 for v in y]]
        nib[1][t] = 16
        B = commit_sets(eng, nib, (4,))[0]
        made.append(B)
        C2, missing, first = eng.commit_fetch([B], [TAB], 2, 2)
        made.append(C2)
        assert missing == [1, 0] and first == [t, None]
        want = [[a ^ b for a, b in zip(nib[0], nib[1])], [a ^ b for a, b in zip(nib[2], nib[3])]]
        want[0][t] = 0
        check_set(eng, srs, C2, want, rnd, probes_of(T, rnd) + [t])
        W2 = copy_rows(eng, [B, C2], (0, 1, 4, 2, 3, 5))
        made.append(W2)
        m2, mm = eng.commit_multiplicities([W2], [TAB], 2, 3)
        made.append(m2)
        assert mm == 1
    finally:
        release(made)
    assert eng.rows_stats() == before


def test_unsort_returns_the_original_columns_and_the_inverse_permutation(engines, srs_of):
    """the row number built by a recurrence travels through commit_sorted as a payload column; a fetch keyed by it, asked for the
    row numbers in program order, gives back the original key and value columns byte for byte, and its index column is the
    inverse of the sort's permutation"""
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(7100)
    key, value = rand_col(T, rnd, 64), rand_col(T, rnd)               # many equal keys: the sort is stable
    KV = commit_sets(eng, [key, value], (2,))[0]
    made = [KV]
    try:
        RN, closings = eng.commit_recurrence([KV], [([], [(ONE, [])], be(0))])          # v' = v + 1 from 0: the row number
        made.append(RN)
        assert closings == [be(T)]
        IN = copy_rows(eng, [KV, RN], (0, 2, 1))                       # (key, row number, value)
        made.append(IN)
        SRT = eng.commit_sorted([IN], 3, 1)
        made.append(SRT)
        TB = copy_rows(eng, [SRT], (1, 0, 2))                          # the row number leads: it is the fetch's key
        made.append(TB)
        OUT, missing, first = eng.commit_fetch([RN], [TB], 1, 1, True)
        made.append(OUT)
        assert missing == [0] and first == [None]
        assert OUT.commitments[1:] == KV.commitments
        _, perm = sref.sorted_columns([key, list(range(T)), value], 1)
        inv = [0] * T
        for q, t in enumerate(perm):
            inv[t] = q
        check_set(eng, srs, OUT, [inv, key, value], rnd, probes_of(T, rnd))
    finally:
        release(made)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 6
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    srs = oc.srs_gen(be(SEED_X), be(SEED_Y), lg + 1, 1, 0)
    rnd = random.Random(8000)
    table = key_table(T, 2, 1, rnd)
    ins = reads_of(table, T, 2, 2, rnd)
    want, want_m, want_f = fref.fetched_columns(ins, table, 2, 2, True)
    want_c = [oc.commit(srs, row_bytes(r), True) for r in want]

    def fresh_ok(I, TB):
        out, missing, first = eng.commit_fetch(I, TB, 2, 2, True)
        out.release()
        assert out.commitments == want_c and (missing, first) == (want_m, want_f)

    I = commit_sets(eng, ins, (1, 3))
    TB = commit_sets(eng, table, (2, 1))
    fresh_ok(I, TB)
    live = eng.rows_stats()
    lib = _native.load()
    E_ARG = _native.KZG_E_ARG
    hi = (ctypes.c_uint64 * 17)(I[0].handle, I[1].handle, *([I[1].handle] * 15))      # 1, 3, 3, 3 .. rows
    ht = (ctypes.c_uint64 * 17)(TB[0].handle, TB[1].handle, *([TB[0].handle] * 15))   # 2, 1, 2, 2 .. rows
    c, h = ctypes.create_string_buffer(48 * 16), ctypes.c_uint64(0)
    miss, first = (ctypes.c_uint64 * 16)(), (ctypes.c_uint64 * 16)()
    INDEX = _native.KZG_FETCH_INDEX

    def raw(n_reads=2, n_keys=2, flags=INDEX, opts=None, ni=2, nt=2):
        return lib.kzg_rows_commit_fetch(eng._h, ni, hi, nt, ht, n_reads, n_keys, flags, ctypes.byref(opts) if opts else None, c,
                                         miss, first, ctypes.byref(h))

    def refused(rc, why):
        msg = lib.kzg_last_error(eng._h)
        assert rc == E_ARG and msg.startswith(b"fetch:") and why in msg, (rc, msg)
        assert eng.rows_stats() == live
        fresh_ok(I, TB)

    refused(raw(n_reads=0), b"n_reads")
    refused(raw(n_keys=4, n_reads=1), b"n_keys must be at most")                       # 3 table rows
    refused(raw(n_keys=3, n_reads=1, flags=0, ni=1, nt=2), b"nothing to output")    # (1 + 3 input rows would be wrong too)
    refused(raw(flags=2), b"flags")
    refused(raw(flags=INDEX | 4), b"flags")
    refused(raw(n_keys=0, n_reads=4, flags=INDEX), b"KZG_FETCH_INDEX needs n_keys")
    refused(raw(nt=9), b"table: more than KZG_MAX_BATCH_OPEN rows")                  # 2 + 1 + 7 x 2 = 17 table rows
    refused(raw(ni=7), b"inputs: more than KZG_MAX_BATCH_OPEN rows")                 # 1 + 3 + 5 x 3 = 19 input rows
    refused(raw(n_reads=9), b"input rows")                                           # 18 input rows asked for
    refused(raw(n_reads=17, n_keys=0, flags=0), b"input rows")
    refused(raw(n_reads=16, n_keys=0, flags=0), b"output rows")                      # 16 reads x 3 payload rows
    refused(raw(n_reads=1), b"exactly n_reads")                                      # 4 rows for one read of 2
    refused(raw(n_reads=2, n_keys=1, flags=0, ni=1), b"exactly n_reads")             # 1 row for 2 reads
    refused(raw(ni=0), b"number of handles")
    refused(raw(nt=0), b"number of handles")
    refused(raw(ni=17), b"number of handles")
    # the layout: every tail error of the derived call
    tl = b"".join(bt(rand_col(4 * 4, rnd)))
    big = R.to_bytes(32, "big")
    for usable, tail, why in ((T, tl, b"usable must be in"), (2 ** 40, tl, b"usable must be in"),
                              (T - 33, tl, b"KZG_MAX_BLIND_ROWS"), (T - 4, None, b"tail_be32 must be given"),
                              (0, tl, b"plain layout"), (T - 4, tl[:-32] + big, b"canonical"),
                              (T - 4, b"\xff" * 32 + tl[32:], b"canonical")):
        refused(raw(opts=_native.DeriveOpts(usable, tail)), why)
    arg_error(lambda: eng.commit_fetch(I, TB, 2, 2, True, 0), "usable")
    arg_error(lambda: eng.commit_fetch(I, TB, 2, 2, True, T - 4, [be(1)] * 15), "exactly")
    arg_error(lambda: eng.commit_fetch(I, TB, 2, 2, True, None, [be(1)]), "tail needs usable")
    assert raw(opts=_native.DeriveOpts(0, None)) == 0              # usable = 0 spelled out: the plain layout
    assert (list(miss[:2]), [None if v == _native.KZG_FETCH_NONE else v for v in first[:2]]) == (want_m, want_f)
    assert c.raw[:48 * 4] == b"".join(want_c)
    eng.release_rows(h.value)
    assert eng.rows_stats() == live
    # handles
    other = commit_sets(eng, table, (3,), i=1)                     # another worker
    arg_error(lambda: eng.commit_fetch(I, other, 2, 2, True), "one worker")
    short = eng.commit_rows(0, [row_bytes(r[:T // 2]) for r in table])         # another length
    arg_error(lambda: eng.commit_fetch(I, [short], 2, 2, True), "one worker and have one row length")
    release(other + [short])
    gone = commit_sets(eng, table, (3,))
    release(gone)
    arg_error(lambda: eng.commit_fetch(I, gone, 2, 2, True), "released")
    arg_error(lambda: eng.commit_fetch([2 ** 40], TB, 1, 1), "unknown")
    fresh_ok(I, TB)
    # the 65th live set
    fill = [eng.commit_rows(0, [row_bytes(table[0])]) for _ in range(_native.KZG_MAX_ROW_SETS - 4)]
    assert eng.rows_stats()[0] == _native.KZG_MAX_ROW_SETS
    arg_error(lambda: eng.commit_fetch(I, TB, 2, 2, True), "KZG_MAX_ROW_SETS", code=_native.KZG_E_BUSY)
    fill.pop().release()
    fresh_ok(I, TB)
    release(fill)
    # stale after an SRS load
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.commit_fetch(I, TB, 2, 2, True), "SRS")
    release(I + TB)
    I, TB = commit_sets(eng, ins, (4,)), commit_sets(eng, table, (3,))
    out, missing, first_m = eng.commit_fetch(I, TB, 2, 2, True)
    assert out.commitments == want_c and (missing, first_m) == (want_m, want_f)
    # the new set goes stale and releases like any other
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.eval_rows([out], [be(3)], [[0]]), "SRS")
    release(I + TB + [out])
    arg_error(lambda: eng.release_rows(out.handle))
    assert eng.rows_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------------- routing
def test_client_multi_handle_and_multi_device_client_return_the_engine_bytes(hip):
    from zkp_subnet_amd import Client, MultiDeviceClient, codec
    from zkp_subnet_amd.engine import lagrange_factor

    lib = _native.load()
    scale, ms = 8, 1
    T, M = 1 << (scale - ms), 1 << ms
    tx, ty = 0xABCDEF0AAA, 0x13579BFA
    rnd = random.Random(9000)
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(1, (ctypes.c_int * 1)(0), ctypes.byref(mh)) == 0
    u = T - 3
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        c, cc = ctypes.create_string_buffer(48 * 4), ctypes.create_string_buffer(48 * 3)
        miss, first = (ctypes.c_uint64 * 2)(), (ctypes.c_uint64 * 2)()
        none = lambda vs: [None if v == _native.KZG_FETCH_NONE else v for v in vs]   # noqa: E731
        made = {}
        for i in range(M):
            table = key_table(T, 1, 1, rnd)
            ins = reads_of(table, T, 1, 2, rnd)
            tail = b"".join(bt(rand_col(4 * (T - u), rnd)))
            I, TB = commit_sets(single, ins, (2,), i=i), commit_sets(single, table, (2,), i=i)
            plain, pm, pf = single.commit_fetch(I, TB, 2, 1, True)
            lay, lm, lf = single.commit_fetch(I, TB, 2, 1, True, u, [tail[j:j + 32] for j in range(0, len(tail), 32)])
            release(I + TB + [plain, lay])
            hi, ht, hz = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 2, b"".join(row_bytes(r) for r in ins), T, 1, cc, ctypes.byref(hi)) == 0
            assert lib.kzg_multi_rows_commit(mh, i, 2, b"".join(row_bytes(r) for r in table), T, 1, cc, ctypes.byref(ht)) == 0
            ai, at = (ctypes.c_uint64 * 1)(hi.value), (ctypes.c_uint64 * 1)(ht.value)
            INDEX = _native.KZG_FETCH_INDEX
            assert lib.kzg_multi_rows_commit_fetch(mh, i, 1, ai, 1, at, 2, 1, INDEX, None, c, miss, first, ctypes.byref(hz)) == 0, i
            assert c.raw == b"".join(plain.commitments) and (list(miss), none(first)) == (pm, pf)
            made[i] = [hi.value, ht.value, hz.value]
            opts = _native.DeriveOpts(u, tail)
            assert lib.kzg_multi_rows_commit_fetch(mh, i, 1, ai, 1, at, 2, 1, INDEX, ctypes.byref(opts), c, miss, first,
                                                   ctypes.byref(hz)) == 0, i
            assert c.raw == b"".join(lay.commitments) and (list(miss), none(first)) == (lm, lf)
            made[i].append(hz.value)
        ai, at = (ctypes.c_uint64 * 1)(made[1][0]), (ctypes.c_uint64 * 1)(made[1][1])   # worker 1's sets under index 0
        assert lib.kzg_multi_rows_commit_fetch(mh, 0, 1, ai, 1, at, 2, 1, 0, None, c, miss, first, ctypes.byref(hz)) == _native.KZG_E_ARG
        for i in range(M):
            for hh in made[i]:
                assert lib.kzg_multi_rows_release(mh, i, hh) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)

    # the text clients over the engine: the same bytes as a commit of the reference rows
    def through(client, workers):
        for i in workers:
            table = key_table(T, 1, 2, rnd)
            ins = reads_of(table, T, 1, 2, rnd)
            a = client.worker_commit_rows(i, [fr(col) for col in ins]).json()["handle"]
            b = client.worker_commit_rows(i, [fr(col) for col in table]).json()["handle"]
            for n_keys, index, usable in ((1, True, None), (1, False, u), (0, False, None)):
                n = fref.n_out(3, 2, n_keys, index)
                tl = rand_col(n * (T - u), rnd) if usable else []
                want, missing, first_m = fref.fetched_columns(ins, table, 2, n_keys, index, usable, tl)
                ref = client.worker_commit_rows(i, [fr(col) for col in want]).json()
                r = client.worker_commit_fetch([a], [b], 2, n_keys, index, usable, fr(tl))
                assert r.status_code == 200, r.json()
                assert r.json()["commitments"] == ref["commitments"]
                assert (r.json()["missing"], r.json()["first_missing"]) == (missing, first_m)
                for hh in (ref["handle"], r.json()["handle"]):
                    assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_fetch([a], [b], 0, 1).status_code == 400
            assert client.worker_commit_fetch([a], [b], 2, 0, True).status_code == 400
            assert client.worker_commit_fetch([a], [b], 2, 3).status_code == 400            # nothing to output
            assert client.worker_commit_fetch([a], [b], 1, 1).status_code == 400            # 2 input rows for one read of 1
            assert client.worker_commit_fetch([a], [b], 2, 1, False, None, fr([1])).status_code == 400
            assert client.worker_release_rows(b).status_code == 200
            assert client.worker_commit_fetch([a], [b], 2, 1).status_code == 400
            assert client.worker_release_rows(a).status_code == 200

    single.close()
    for client in (Client(seed=83), MultiDeviceClient(devices=[0], seed=83)):
        client.start(scale=scale, machines_scale=ms)
        try:
            through(client, range(M))
        finally:
            client.stop()
