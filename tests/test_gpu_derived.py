"""GPU tests (`-m gpu`) of kzg_rows_commit_derived: inverse-or-zero (with its bit row) and limb decomposition of resident
columns, built and committed on the device.  The expected rows come from the definition in Python integers
(tests/derived_ref.py) and are committed with the C oracle, never with the library under test.  Every case compares the
commitments byte for byte, the values at probe indices and at one random point through eval_rows, and the counts exactly.
Row lengths 2 .. 2^12 for the single ops; 2^16 only where the shared inversion's element count decides the path (its level 0
folds 4, 8 or 16 elements per lane from 2^17 and 2^18 elements on), over four source columns whose reference rows and oracle
commitments are computed once for the module.  Each test leaves rows_stats() where it found it."""
import ctypes
import random

import pytest

from oracle import cpu as oc
from tests import derived_ref as dref
from tests import grand_product_ref as gp
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, q_call, release, srs_cache
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0xDE21FED1, 0xDE21FED2
SHAPE_MSG = "the constraints do not hold"


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def probes_of(T, rnd, usable=None):
    """the ends, the borders of the mask words and of the waves, the rows around `usable` and three random rows"""
    ps = {0, 1 % T, T - 1} | {rnd.randrange(T) for _ in range(3)}
    ps |= {t for t in (31, 32, 63, 64, 255, 256) if t < T}
    if usable is not None:
        ps |= {max(usable - 1, 0), usable, min(usable + 1, T - 1)}
    return sorted(ps)


def check_set(eng, srs, rset, want, rnd, probes, i=0, want_c=None):
    """the set `rset` against its expected evaluation rows `want` (integers); want_c: their oracle commitments, where known"""
    w, T = len(want), len(want[0])
    assert (rset.k, rset.i, rset.T, len(rset.commitments)) == (w, i, T, w)
    wb = [row_bytes(r) for r in want]
    for c in range(w):
        assert rset.commitments[c] == (want_c[c] if want_c else oc.commit(srs, wb[c], True)), c
    om = gp.omega(T)
    ts = sorted(set(probes))
    for t0 in range(0, len(ts), 4):
        part = ts[t0:t0 + 4]
        Y = eng.eval_rows([rset], [be(pow(om, t, R)) for t in part], [list(range(w))] * len(part))
        for t, ys in zip(part, Y):
            assert ys == [be(want[c][t]) for c in range(w)], t
    x = be(rnd.randrange(R))
    assert eng.eval_rows([rset], [x], [list(range(w))])[0] == [oc.fr_eval(oc.fr_ntt(b, True), x) for b in wb]


def run(eng, srs, cols, ops, rnd, usable=None, tail=(), sizes=None, ef=True, probes=None):
    """commit `cols`, derive on the device, check the new set and the counts against the reference; returns (rows, counts)"""
    T = len(cols[0])
    want, counts = dref.derived_columns(cols, ops, usable, tail)
    S = commit_sets(eng, cols, sizes or (len(cols),), ef)
    try:
        out, got = eng.commit_derived(S, ops, usable, bt(tail))
        try:
            assert got == counts, (got, counts)
            check_set(eng, srs, out, want, rnd, probes or probes_of(T, rnd, usable))
        finally:
            out.release()
    finally:
        release(S)
    return want, counts


def rand_col(T, rnd, bound=R):
    return [rnd.randrange(bound) for _ in range(T)]


# ---------------------------------------------------------------------------------------------------- inverse-or-zero
def inv0_columns(T, rnd):
    """(name, column) pairs: random, all zero, zero at {0}, {T - 1}, {0, T - 1}, zero on a whole 64-cell lane group, 1 and r - 1"""
    cols = [("random", [rnd.randrange(1, R) for _ in range(T)]), ("all zero", [0] * T)]
    for name, zs in (("zero at 0", {0}), ("zero at T - 1", {T - 1}), ("zero at both ends", {0, T - 1})):
        cols.append((name, [0 if t in zs else rnd.randrange(1, R) for t in range(T)]))
    if T >= 256:
        cols.append(("a zero lane group", [0 if 128 <= t < 192 else rnd.randrange(1, R) for t in range(T)]))
        cols.append(("zeros across a word border", [0 if 20 <= t < 45 or t == 63 else rnd.randrange(1, R) for t in range(T)]))
    cols.append(("1 and r - 1", [(1, R - 1)[t & 1] for t in range(T)]))
    return cols


@pytest.mark.parametrize("lg", [1, 2, 4, 10, 12])
@pytest.mark.parametrize("with_bit", [False, True])
def test_inv0(engines, srs_of, lg, with_bit):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(100 + 2 * lg + with_bit)
    for name, col in inv0_columns(T, rnd):
        op = ("inv0", 0, True) if with_bit else ("inv0", 0)
        want, counts = run(eng, srs, [col], [op], rnd, probes=range(T) if T <= 16 else None)
        assert counts == [col.count(0)], name
        assert all(x * y % R == (1 if x else 0) for x, y in zip(col, want[0])), name
        if name == "all zero":
            assert want[0] == [0] * T
        if with_bit:
            assert want[1] == [0 if x else 1 for x in col], name
    assert eng.rows_stats() == before


LG_BIG = 16


@pytest.fixture(scope="module")
def big(engines, srs_of):
    """four source columns of 2^16 cells (zeros at the ends, on a lane group and sprinkled), resident in one set; their
    inverse-or-zero rows, zero counts and oracle commitments, computed once for the cases below"""
    eng, srs, T = engines(LG_BIG), srs_of(LG_BIG), 1 << LG_BIG
    rnd = random.Random(1600)
    cols = []
    for j in range(4):
        zs = {0, T - 1} | set(range(4096 * j + 64, 4096 * j + 128)) | {rnd.randrange(T) for _ in range(50 * j)}
        cols.append([0 if t in zs else rnd.randrange(1, R) for t in range(T)])
    refs = [dref.inv0(col) for col in cols]
    want_c = [oc.commit(srs, row_bytes(inv), True) for inv, _, _ in refs]
    S = commit_sets(eng, cols, (1, 3))
    yield eng, srs, S, refs, want_c
    release(S)


@pytest.mark.parametrize("sources", [[2], [0, 1], [0, 1, 0], [0, 1, 2, 3], [0, 1, 2, 3, 3, 2, 1, 0]],
                         ids=["2^16", "2^17", "3x2^16", "2^18", "2^19"])
def test_inv0_ops_share_one_inversion_over_all_their_elements(big, sources):
    """n_inv = 1, 2, 3, 4 and 8 ops at T = 2^16: 2^16, 2^17, 3 * 2^16 (no power of two), 2^18 and 2^19 elements in the one
    inversion.  From three ops on a source row is named twice: it is transformed once and yields identical rows."""
    eng, srs, S, refs, want_c = big
    before = eng.rows_stats()
    T = 1 << LG_BIG
    rnd = random.Random(1700 + len(sources))
    out, counts = eng.commit_derived(S, [("inv0", j) for j in sources])
    try:
        assert counts == [refs[j][2] for j in sources]
        check_set(eng, srs, out, [refs[j][0] for j in sources], rnd, probes_of(T, rnd), want_c=[want_c[j] for j in sources])
        for a in range(len(sources)):
            for b in range(a):
                assert (out.commitments[a] == out.commitments[b]) == (sources[a] == sources[b])
    finally:
        out.release()
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- limbs
LIMB_SHAPES = [(1, 16), (8, 4), (16, 4), (16, 16), (32, 8), (13, 5), (31, 3)]    # the last two straddle word borders


def limb_column(T, b, L, rnd):
    """below 2^(b L), the boundary values 2^(b L) - 1 and 2^(b L), r - 1, and random full-width values"""
    top = 1 << (b * L)
    col = [0, top - 1 if top <= R else R - 1, top % R if top < R else 1, R - 1]
    col += [rnd.randrange(min(top, R)) for _ in range(T // 2 - 2)] + [rnd.randrange(R) for _ in range(T // 2 - 2)]
    assert len(col) == T
    return col


@pytest.mark.parametrize("lg", [2, 10])
@pytest.mark.parametrize("b,L", LIMB_SHAPES)
def test_limbs(engines, srs_of, lg, b, L):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(2000 + 100 * b + L + lg)
    col = limb_column(T, b, L, rnd)
    want, counts = run(eng, srs, [col], [("limbs", 0, b, L)], rnd, probes=range(T) if T <= 16 else None)
    top = 1 << (b * L)
    assert counts == [sum(1 for x in col if x >= top)]
    if b * L == 256:
        assert counts == [0]                                       # no overflow by construction: every value is below r < 2^256
    else:
        assert counts[0] >= 2                                      # 2^(b L) and r - 1 at least
    for t, x in enumerate(col):
        assert sum(want[l][t] << (b * l) for l in range(L)) == x % top
    # values below 2^(b L) only: nothing is counted
    low = [rnd.randrange(min(top, R)) for _ in range(T)]
    assert run(eng, srs, [low], [("limbs", 0, b, L)], rnd)[1] == [0]
    assert eng.rows_stats() == before


def test_mixed_ops_keep_their_order_and_their_own_counts(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(3000)
    cols = [rand_col(T, rnd, 1 << 33), [0 if t % 7 == 0 else rnd.randrange(R) for t in range(T)], rand_col(T, rnd, 1 << 16)]
    ops = [("limbs", 0, 16, 2), ("inv0", 1, True), ("limbs", 2, 8, 2), ("inv0", 0), ("limbs", 1, 32, 8), ("inv0", 1)]
    for sizes, ef in (((3,), True), ((1, 2), False), ((2, 1), True)):      # one set, two sets, coefficient form
        want, counts = run(eng, srs, cols, ops, rnd, sizes=sizes, ef=ef)
        assert len(want) == 16                                     # 2 + 2 + 2 + 1 + 8 + 1: a full set
        assert counts == [sum(1 for x in cols[0] if x >> 32), cols[1].count(0), 0, cols[0].count(0), 0, cols[1].count(0)]
        assert counts[0] > 0 and counts[1] > 0 and want[2] == want[15]
    # a handle named twice: rows 0 and 1 are the same column
    S = commit_sets(eng, cols[1:2], (1,))
    try:
        out, counts = eng.commit_derived([S[0], S[0]], [("inv0", 0), ("inv0", 1)])
        try:
            inv, _, zeros = dref.inv0(cols[1])
            assert counts == [zeros, zeros]
            check_set(eng, srs, out, [inv, inv], rnd, probes_of(T, rnd))
        finally:
            out.release()
    finally:
        release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the layout
@pytest.mark.parametrize("u", [1, (1 << 10) - 32, (1 << 10) - 1])
def test_usable_layout(engines, srs_of, u):
    """The source rows behind `usable` hold zeros and over-range values, which would be counted if they were read; the tails are
    checked in place, column-major.  T - usable <= KZG_MAX_BLIND_ROWS is part of the call's contract: usable = 1 is its refusal
    at T = 2^10 and runs at T = 4."""
    rnd = random.Random(4000 + u)
    ops = [("inv0", 0, True), ("limbs", 1, 16, 2), ("inv0", 1)]
    n_out = dref.n_out(ops)
    for lg in (10, 2):
        eng, srs, T = engines(lg), srs_of(lg), 1 << lg
        before = eng.rows_stats()
        if u >= T:
            continue
        cols = [[rnd.randrange(1, R) for _ in range(u)] + [0] * (T - u), rand_col(u, rnd, 1 << 32) + [0, R - 1] * ((T - u + 1) // 2)]
        cols[1] = cols[1][:T]
        cols[0][u // 2] = 0
        tail = rand_col(n_out * (T - u), rnd)
        if T - u > _native.KZG_MAX_BLIND_ROWS:
            S = commit_sets(eng, cols, (2,))
            arg_error(lambda: eng.commit_derived(S, ops, u, bt(tail)), "KZG_MAX_BLIND_ROWS")
            release(S)
        else:
            probes = set(probes_of(T, rnd, u)) | set(range(u, T))
            want, counts = run(eng, srs, cols, ops, rnd, u, tail, probes=probes)
            assert counts == [1, 0, cols[1][:u].count(0)]
            for c in range(n_out):
                assert want[c][u:] == tail[c * (T - u):(c + 1) * (T - u)]
        assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- end to end
def test_range_check_from_the_value_column_to_the_quotient(engines):
    """a 32-bit value column -> limbs (16, 2) on the device -> multiplicities against a resident table -> the running sum -> the
    quotient of the gate x - limb_0 - 2^16 limb_1, with nothing row-sized returning to the host in between"""
    lg = 10
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(5000)
    x = [rnd.randrange(T) | (rnd.randrange(T) << 16) for _ in range(T)]      # both limbs below 2^10: the table fits T rows
    X, TAB = commit_sets(eng, [x, list(range(T))], (1, 1))
    made = [X, TAB]
    try:
        L, counts = eng.commit_derived([X], [("limbs", 0, 16, 2)])
        made.append(L)
        assert counts == [0]
        m, missing = eng.commit_multiplicities([L], [TAB], 2, 1)
        made.append(m)
        assert missing == 0
        s, closing = eng.commit_lookup_sum([L], [TAB], m, 2, 1, be(rnd.randrange(R)), be(rnd.randrange(R)))
        made.append(s)
        assert closing == be(0)
        gate = [(1, [0]), (R - 1, [1]), (R - (1 << 16), [2])]
        made.append(q_call(eng, [X, L], gate, None, 1, 1))
        # the gate means something: against limbs of another width it does not hold
        L8, _ = eng.commit_derived([X], [("limbs", 0, 8, 2)])
        made.append(L8)
        arg_error(lambda: q_call(eng, [X, L8], gate, None, 1, 1), SHAPE_MSG)
    finally:
        release(made)
    assert eng.rows_stats() == before


def test_zero_test_gates_accept_the_derived_rows_and_refuse_a_wrong_inverse(engines):
    lg = 10
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(5100)
    x = [0 if rnd.randrange(3) == 0 else rnd.randrange(R) for _ in range(T)]
    y = rnd.randrange(1, R)                                       # the gates x bit and 1 - bit - x inv, combined by y
    gate = [(1, [0, 2]), (y, []), (R - y, [2]), (R - y, [0, 1])]
    X = commit_sets(eng, [x], (1,))[0]
    made = [X]
    try:
        D, counts = eng.commit_derived([X], [("inv0", 0, True)])
        made.append(D)
        assert counts == [x.count(0)] and counts[0] > 0
        made.append(q_call(eng, [X, D], gate, None, 1, 1))
        # the same rows uploaded, one cell of inv wrong: the quotient's shape check refuses them
        inv, bit, _ = dref.inv0(x)
        t = next(t for t in range(T // 2, T) if x[t])
        inv[t] = (inv[t] + 1) % R
        B = commit_sets(eng, [inv, bit], (2,))[0]
        made.append(B)
        arg_error(lambda: q_call(eng, [X, B], gate, None, 1, 1), SHAPE_MSG)
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
    rnd = random.Random(6000)
    cols = [rand_col(T, rnd, 1 << 40), [0 if t % 5 == 0 else rnd.randrange(R) for t in range(T)], rand_col(T, rnd)]
    ops = [("limbs", 0, 16, 2), ("inv0", 1, True)]
    want, want_counts = dref.derived_columns(cols, ops)
    want_c = [oc.commit(srs, row_bytes(r), True) for r in want]

    def fresh_ok(sets):
        out, counts = eng.commit_derived(sets, ops)
        out.release()
        assert out.commitments == want_c and counts == want_counts

    I = commit_sets(eng, cols, (1, 2))
    fresh_ok(I)
    live = eng.rows_stats()
    lib = _native.load()
    E_ARG = _native.KZG_E_ARG
    hi = (ctypes.c_uint64 * 2)(I[0].handle, I[1].handle)
    c, h, cnt = ctypes.create_string_buffer(48 * 16), ctypes.c_uint64(0), (ctypes.c_uint64 * 32)()
    INV0, LIMBS = _native.KZG_DERIVE_INV0, _native.KZG_DERIVE_LIMBS

    def raw(recs, opts=None, n=2, n_ops=None):
        arr = (_native.DeriveOp * max(len(recs), 1))(*[_native.DeriveOp(*r) for r in recs])
        return lib.kzg_rows_commit_derived(eng._h, n, hi, len(recs) if n_ops is None else n_ops, arr,
                                           ctypes.byref(opts) if opts else None, c, cnt, ctypes.byref(h))

    def refused(rc, why):
        msg = lib.kzg_last_error(eng._h)
        assert rc == E_ARG and msg.startswith(b"derived: ") and why in msg, (rc, msg)
        assert eng.rows_stats() == live
        fresh_ok(I)

    # the ops
    refused(raw([], n_ops=0), b"n_ops")
    refused(raw([(LIMBS, 0, 8, 16), (INV0, 1, 0, 1)]), b"n_out")                    # 17 output rows
    refused(raw([(INV0, 0, 0, 2)] * 9), b"n_out")
    refused(raw([(0, 0, 0, 1)]), b"unknown kind")
    refused(raw([(3, 0, 8, 1)]), b"unknown kind")
    refused(raw([(INV0, 3, 0, 1)]), b"a row must index")                            # 3 rows: 0 .. 2
    refused(raw([(LIMBS, 0, 8, 2), (LIMBS, 2 ** 31, 8, 2)]), b"a row must index")
    refused(raw([(LIMBS, 0, 0, 4)]), b"bits must be in [1, 32]")
    refused(raw([(LIMBS, 0, 33, 1)]), b"bits must be in [1, 32]")
    refused(raw([(LIMBS, 0, 8, 0)]), b"count must be in [1, KZG_MAX_BATCH_OPEN]")
    refused(raw([(LIMBS, 0, 1, 17)]), b"count must be in [1, KZG_MAX_BATCH_OPEN]")
    refused(raw([(LIMBS, 0, 32, 9)]), b"bits * count")
    refused(raw([(LIMBS, 0, 17, 16)]), b"bits * count")
    refused(raw([(INV0, 0, 8, 1)]), b"bits must be 0")
    refused(raw([(INV0, 0, 0, 0)]), b"count must be 1 or 2")
    refused(raw([(INV0, 0, 0, 3)]), b"count must be 1 or 2")
    refused(raw([(INV0, 0, 0, 1)], n=0), b"number of handles")
    refused(raw([(INV0, 0, 0, 1)], n=17), b"number of handles")
    # the layout: every tail error of the sorted call
    recs = [(LIMBS, 0, 16, 2), (INV0, 1, 0, 1)]
    tl = b"".join(bt(rand_col(3 * 4, rnd)))
    big = R.to_bytes(32, "big")
    for usable, tail, why in ((T, tl, b"usable must be in"), (2 ** 40, tl, b"usable must be in"),
                              (T - 33, tl, b"KZG_MAX_BLIND_ROWS"), (T - 4, None, b"tail_be32 must be given"),
                              (0, tl, b"plain layout"), (T - 4, tl[:-32] + big, b"canonical"),
                              (T - 4, b"\xff" * 32 + tl[32:], b"canonical")):
        refused(raw(recs, _native.DeriveOpts(usable, tail)), why)
    arg_error(lambda: eng.commit_derived(I, ops, 0), "usable")
    arg_error(lambda: eng.commit_derived(I, ops, T - 4, [be(1)] * 11), "exactly")
    arg_error(lambda: eng.commit_derived(I, ops, None, [be(1)]), "tail needs usable")
    assert raw(recs, _native.DeriveOpts(0, None)) == 0             # usable = 0 spelled out: the plain layout
    assert list(cnt[:2]) == [want_counts[0], want_counts[1]]
    eng.release_rows(h.value)
    assert eng.rows_stats() == live
    # handles
    other = commit_sets(eng, cols[1:], (2,), i=1)                  # another worker
    arg_error(lambda: eng.commit_derived([I[0]] + other, ops), "one worker")
    short = eng.commit_rows(0, [row_bytes(r[:T // 2]) for r in cols[1:]])      # another length
    arg_error(lambda: eng.commit_derived([I[0], short], ops), "one worker and have one row length")
    release(other + [short])
    gone = commit_sets(eng, cols[1:], (2,))
    release(gone)
    arg_error(lambda: eng.commit_derived([I[0]] + gone, ops), "released")
    arg_error(lambda: eng.commit_derived([2 ** 40], [("inv0", 0)]), "unknown")
    arg_error(lambda: eng.commit_derived(I * 6, ops), "KZG_MAX_BATCH_OPEN rows")    # 18 rows
    fresh_ok(I)
    # the 65th live set
    fill = [eng.commit_rows(0, [row_bytes(cols[0])]) for _ in range(_native.KZG_MAX_ROW_SETS - 2)]
    assert eng.rows_stats()[0] == _native.KZG_MAX_ROW_SETS
    arg_error(lambda: eng.commit_derived(I, ops), "KZG_MAX_ROW_SETS", code=_native.KZG_E_BUSY)
    fill.pop().release()
    fresh_ok(I)
    release(fill)
    # stale after an SRS load
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.commit_derived(I, ops), "SRS")
    release(I)
    I = commit_sets(eng, cols, (3,))
    out, counts = eng.commit_derived(I, ops)
    assert out.commitments == want_c and counts == want_counts
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
    tx, ty = 0xABCDEF0999, 0x13579BF9
    rnd = random.Random(7000)
    ops = [("inv0", 1, True), ("limbs", 0, 13, 3)]
    recs = [(_native.KZG_DERIVE_INV0, 1, 0, 2), (_native.KZG_DERIVE_LIMBS, 0, 13, 3)]
    arr = (_native.DeriveOp * 2)(*[_native.DeriveOp(*r) for r in recs])
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(1, (ctypes.c_int * 1)(0), ctypes.byref(mh)) == 0
    u = T - 3
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        c, cc, cnt = ctypes.create_string_buffer(48 * 5), ctypes.create_string_buffer(96), (ctypes.c_uint64 * 2)()
        made = {}
        for i in range(M):
            cols = [rand_col(T, rnd, 1 << 40), [0 if t % 3 == 0 else rnd.randrange(R) for t in range(T)]]
            tail = b"".join(bt(rand_col(5 * (T - u), rnd)))
            I = commit_sets(single, cols, (2,), i=i)
            plain, pc = single.commit_derived(I, ops)
            lay, lc = single.commit_derived(I, ops, u, [tail[j:j + 32] for j in range(0, len(tail), 32)])
            release(I + [plain, lay])
            hi, hz = ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 2, b"".join(row_bytes(r) for r in cols), T, 1, cc, ctypes.byref(hi)) == 0
            ai = (ctypes.c_uint64 * 1)(hi.value)
            assert lib.kzg_multi_rows_commit_derived(mh, i, 1, ai, 2, arr, None, c, cnt, ctypes.byref(hz)) == 0, i
            assert c.raw == b"".join(plain.commitments) and list(cnt) == pc
            made[i] = [hi.value, hz.value]
            opts = _native.DeriveOpts(u, tail)
            assert lib.kzg_multi_rows_commit_derived(mh, i, 1, ai, 2, arr, ctypes.byref(opts), c, cnt, ctypes.byref(hz)) == 0, i
            assert c.raw == b"".join(lay.commitments) and list(cnt) == lc
            made[i].append(hz.value)
        ai = (ctypes.c_uint64 * 1)(made[1][0])                     # worker 1's set under index 0
        assert lib.kzg_multi_rows_commit_derived(mh, 0, 1, ai, 2, arr, None, c, cnt, ctypes.byref(hz)) == _native.KZG_E_ARG
        for i in range(M):
            for hh in made[i]:
                assert lib.kzg_multi_rows_release(mh, i, hh) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)

    # the text clients over the engine: the same bytes as a commit of the reference rows
    def through(client, workers):
        for i in workers:
            cols = [rand_col(T, rnd, 1 << 40), [0 if t % 3 == 0 else rnd.randrange(R) for t in range(T)]]
            tail = rand_col(5 * (T - u), rnd)
            a = client.worker_commit_rows(i, [fr(col) for col in cols]).json()["handle"]
            for usable, tl in ((None, []), (u, tail)):
                want, counts = dref.derived_columns(cols, ops, usable, tl)
                ref = client.worker_commit_rows(i, [fr(col) for col in want]).json()
                r = client.worker_commit_derived([a], [list(op) for op in ops], usable, fr(tl))
                assert r.status_code == 200, r.json()
                assert r.json()["commitments"] == ref["commitments"] and r.json()["counts"] == counts
                for hh in (ref["handle"], r.json()["handle"]):
                    assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_derived([a], [["sqrt", 0]]).status_code == 400
            assert client.worker_commit_derived([a], [["limbs", 0, 40, 1]]).status_code == 400
            assert client.worker_commit_derived([a], [["inv0", 0]], None, fr([1])).status_code == 400
            assert client.worker_release_rows(a).status_code == 200
            assert client.worker_commit_derived([a], [["inv0", 0]]).status_code == 400

    single.close()
    for client in (Client(seed=79), MultiDeviceClient(devices=[0], seed=79)):
        client.start(scale=scale, machines_scale=ms)
        try:
            through(client, range(M))
        finally:
            client.stop()
