"""GPU tests (`-m gpu`) of kzg_rows_commit_alu: machine-word arithmetic whose kind an op-code column picks per row, computed
from the canonical integers of resident columns and committed on the device.  The expected rows come from the definition in
Python integers (tests/alu_ref.py) and are committed with the C oracle, never with the library under test; on a constant
op-code column the eight shared kinds are also compared with kzg_rows_commit_int.  Every case compares the commitments byte
for byte, EVERY cell of every output row through read_rows, and the four statistics exactly.  Row lengths 2 .. 2^12: one lane
per cell and 256 lanes per workgroup, so 2^10 runs 4 workgroups per unit.  Each test leaves rows_stats() where it found it."""
import ctypes
import random
import struct

import pytest

from oracle import cpu as oc
from tests import alu_ref as aref
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release, srs_cache
from tests.test_gpu_int import check_set, probes_of, shift_col
from zkp_subnet_amd import _native
from zkp_subnet_amd.engine import HipEngine

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x1A7C0DE3, 0x1A7C0DE4
NK = len(aref.KINDS)


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def read_all(eng, rset, usable=None):
    """every cell of every row of `rset` below `usable` as integers (the outputs of the call are machine words)"""
    n = rset.T if usable is None else usable
    rows = []
    for c in range(rset.k):
        raw, overflow, _ = eng.read_rows([rset], c, 0, n, "u64")
        assert overflow == 0
        rows.append(list(struct.unpack(f"<{n}Q", raw)))
    return rows


def run(eng, srs, cols, program, units, rnd, usable=None, tail=(), sizes=None, ef=True):
    """commit `cols`, build on the device, check the new set and the statistics against the reference; returns (rows, stats)"""
    T = len(cols[0])
    want, stats = aref.alu_columns(cols, program, units, usable, tail)
    S = commit_sets(eng, cols, sizes or (len(cols),), ef)
    try:
        out, got = eng.commit_alu(S, program, units, usable, bt(tail))
        try:
            assert got == stats, (got, stats)
            n = T if usable is None else usable
            assert read_all(eng, out, usable) == [r[:n] for r in want]             # every cell, no row left unchecked
            probes = set(range(T)) if T <= 16 else set(probes_of(T, rnd, usable))
            if usable is not None:
                probes |= set(range(usable, T))
            check_set(eng, srs, out, want, rnd, probes)                            # the commitments against the oracle's
        finally:
            out.release()
    finally:
        release(S)
    return want, stats


def edges(w):
    """0, 1, M/2 - 1, M/2, M - 1 clipped to [0, M): five values (with repeats at w = 1), so 25 pairs"""
    M = 1 << w
    return [min(max(v, 0), M - 1) for v in (0, 1, M // 2 - 1, M // 2, M - 1)]


def wide(w, rnd):
    """a value at or above 2^w"""
    M = 1 << w
    return rnd.choice([M, M + 5, 1 << 64, (1 << 64) + 7, R - 1, rnd.randrange(max(M, 1 << 64), R)])


def every_kind_cols(T, widths, rnd):
    """op, a, b: row t < 23 * 25 takes op-code t mod 23 and the edge pair t div 23 (of the width of its entry); the rows behind
    are random, with op-codes that also hit the idle entry 23 and the codes 24 and 25 beyond the program, and with every
    twelfth operand out of range"""
    assert T >= NK * 25
    op, a, b = [], [], []
    for t in range(T):
        if t < NK * 25:
            c, w = t % NK, widths[t % NK]
            e = edges(w)
            x, y = e[(t // NK) // 5], e[(t // NK) % 5]
        else:
            c = rnd.randrange(NK + 3)
            w = widths[c] if c < NK else 8
            x, y = rnd.randrange(1 << w), rnd.randrange(1 << w)
            if rnd.randrange(12) == 0:
                x = wide(w, rnd)
            if rnd.randrange(12) == 0:
                y = wide(w, rnd)
        op.append(c)
        a.append(x)
        b.append(y)
    return [op, a, b]


# ---------------------------------------------------------------------------------------------------- against commit_int
@pytest.mark.parametrize("w", [1, 33, 64])
@pytest.mark.parametrize("lg", [1, 10])
@pytest.mark.parametrize("kind", aref.SHARED)
def test_a_constant_op_code_column_gives_commit_int_s_bytes(engines, kind, lg, w):
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(1000 * lg + 10 * w + aref.KINDS.index(kind))
    a = [rnd.randrange(1 << w) if rnd.randrange(8) else wide(w, rnd) for _ in range(T)]
    b = shift_col(T, w, rnd) if kind == "split" else [rnd.randrange(1 << w) if rnd.randrange(8) else wide(w, rnd) for _ in range(T)]
    count = 1 if kind in aref.ONE_ROW else 2
    S = commit_sets(eng, [[0] * T, a, b], (3,))
    try:
        ref, counts, first = eng.commit_int(S, [(kind, w, 1, 2, count)])
        out, st = eng.commit_alu(S, [(kind, w)], [(0, 1, 2, count)])
        assert out.commitments == ref.commitments
        assert st == {"counts": counts, "first": first, "unknown": [0], "first_unknown": [None]}
        release([ref, out])
    finally:
        release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- every kind in one column
MIXED = [(8, 32, 64)[k % 3] for k in range(NK)]


@pytest.mark.parametrize("widths", [[1] * NK, [8] * NK, [32] * NK, [33] * NK, [64] * NK, MIXED],
                         ids=["w1", "w8", "w32", "w33", "w64", "mixed"])
def test_every_kind_in_one_column(engines, srs_of, widths):
    """All 23 kinds meet all 25 edge pairs in ONE column of 2^10 rows (four workgroups, every wave divergent), with both rows
    and with row 0 alone; the mixed program gives the entries the widths 8, 32 and 64 in turn"""
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    assert T >= 575
    before = eng.rows_stats()
    rnd = random.Random(sum(widths))
    cols = every_kind_cols(T, widths, rnd)
    program = [(k, widths[c]) for c, k in enumerate(aref.KINDS)] + [None]
    want2, st2 = run(eng, srs, cols, program, [(0, 1, 2, 2)], rnd)
    want1, st1 = run(eng, srs, cols, program, [(0, 1, 2)], rnd)
    assert want1 == want2[:1] and st1 == st2
    assert st2["unknown"][0] > 0 and st2["first_unknown"][0] >= 575 and st2["counts"][0] > 0
    for t in range(575):                                                       # the edge rows are the reference's cells
        x0, x1, _ = aref.cell(aref.KINDS[t % NK], widths[t % NK], cols[1][t], cols[2][t])
        assert (want2[0][t], want2[1][t]) == (x0, x1)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("lg,w", [(1, 32), (2, 1), (4, 33), (12, 64)])
def test_sizes(engines, srs_of, lg, w):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(2000 + lg)
    program = [(k, w) for k in aref.KINDS] + [None]
    op = [rnd.randrange(NK + 2) for _ in range(T)]
    a = [rnd.randrange(1 << w) if rnd.randrange(10) else wide(w, rnd) for _ in range(T)]
    b = [rnd.randrange(1 << w) if rnd.randrange(10) else wide(w, rnd) for _ in range(T)]
    run(eng, srs, [op, a, b], program, [(0, 1, 2, 2)], rnd)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- immediates
def test_entries_with_immediates_neither_read_nor_count_column_b(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(3000)
    w, M = 32, 1 << 32
    program = [("srl", w, ("imm", 7)), ("sext", w, ("imm", 8)), ("sext", w, ("imm", 16)), ("add", w), ("split", w, ("imm", 32)),
               ("rotl", w, ("imm", 33))]
    op = [t % 6 for t in range(T)]
    a = [rnd.randrange(M) for _ in range(T)]
    b = [rnd.randrange(M) if c == 3 else wide(w, rnd) for c in op]             # junk wherever the entry has an immediate
    a[9], b[15] = wide(w, rnd), wide(w, rnd)                                   # add rows: a out of range, b out of range
    a[13] = wide(w, rnd)                                                       # a out of range on a row with an immediate
    want, st = run(eng, srs, [op, a, b], program, [(0, 1, 2, 2)], rnd)
    assert st == {"counts": [3], "first": [9], "unknown": [0], "first_unknown": [None]}
    assert want[0][0] == a[0] >> 7 and want[1][0] == a[0] % 128
    lo = a[1] % 256
    assert want[0][1] == (lo - ((lo >> 7) << 8)) % M and want[1][1] == lo >> 7
    assert want[0][4] == 0 and want[1][4] == a[4] and want[0][5] == ((a[5] << 1) % M) + (a[5] >> 31)
    # a program of immediates alone: column b is not even transformed, whatever it holds
    want, st = run(eng, srs, [op, a, b], [program[0], program[1]], [(0, 1, 2, 2)], rnd)
    assert st["unknown"] == [sum(1 for c in op if c >= 2)] and st["first_unknown"] == [2]
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- out of range, unknown
@pytest.mark.parametrize("lg", [2, 10])
def test_out_of_range_operands_and_unknown_op_codes(engines, srs_of, lg):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(4000 + lg)
    w, M = 32, 1 << 32
    program = [("xor", w), ("mulh", w), None, ("div", w)]
    clean = lambda: [rnd.randrange(M) for _ in range(T)]          # noqa: E731
    for rows_a, rows_b, rows_u in (([0], [], []), ([], [T - 1], [0]), ([1], [1], [T - 1]), ([0, T - 1], [0, T - 2], [1, 2]),
                                   ([], [], [])):
        op, a, b = [rnd.choice([0, 1, 3]) for _ in range(T)], clean(), clean()
        for t in rows_a:
            a[t] = wide(w, rnd)
        for t in rows_b:
            b[t] = wide(w, rnd)
        for t, code in zip(rows_u, ((1 << 32) + 3, 4, R - 1)):                 # 2^32 + 3 is unknown, not op-code 3
            op[t] = code
        want, st = run(eng, srs, [op, a, b], program, [(0, 1, 2, 2)], rnd)
        flagged = sorted((set(rows_a) | set(rows_b)) - set(rows_u))            # an unknown cell reads no operand
        assert st == {"counts": [len(flagged)], "first": [flagged[0] if flagged else None], "unknown": [len(rows_u)],
                      "first_unknown": [min(rows_u) if rows_u else None]}
        assert all(want[0][t] == 0 and want[1][t] == 0 for t in rows_u)
        for t in flagged:                                                      # reduced, not refused
            assert (want[0][t], want[1][t]) == aref.cell(program[op[t]][0], w, a[t] % M, b[t] % M)[:2]
    if T > 256:      # an idle row holding junk counts nothing; a flagged cell in the last workgroup only
        op, a, b = [2] * T, [wide(w, rnd) for _ in range(T)], [wide(w, rnd) for _ in range(T)]
        op[1000], op[1001] = 0, 77
        want, st = run(eng, srs, [op, a, b], program, [(0, 1, 2, 2)], rnd)
        assert st == {"counts": [1], "first": [1000], "unknown": [1], "first_unknown": [1001]}
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- units
def test_eight_units_over_two_handles_share_one_program_and_give_sixteen_rows(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(5000)
    program = [(k, (8, 32, 64)[c % 3]) for c, k in enumerate(aref.KINDS)] + [None]
    cols = every_kind_cols(T, [e[1] for e in program[:NK]], rnd)
    cols += [[rnd.randrange(NK + 2) for _ in range(T)], [rnd.randrange(1 << 32) for _ in range(T)]]
    units = [(0, 1, 2, 2), (3, 4, 1, 2), (3, 3, 3, 2), (0, 2, 1, 2), (3, 1, 4, 2), (0, 1, 2, 2), (0, 4, 4, 2), (3, 2, 2, 2)]
    want = None
    for sizes, ef in (((5,), True), ((2, 3), True), ((4, 1), False)):          # one set, two sets, coefficient form
        got, _ = run(eng, srs, cols, program, units, rnd, sizes=sizes, ef=ef)
        assert len(got) == 16 and (want is None or got == want)
        want = got
    assert want[0] == want[10] and want[1] == want[11]                         # two units over the same rows
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the layout
@pytest.mark.parametrize("lg,u", [(4, 11), (10, (1 << 10) - 31)])
def test_usable_layout(engines, srs_of, lg, u):
    """The source rows behind `usable` hold unknown op-codes and out-of-range operands, which would be counted if they were
    read; the tails are checked in place, column-major; there is no closing row"""
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(6000 + lg)
    w, M = 32, 1 << 32
    program = [("sra", w), ("rem", w), ("lt", w), None]
    op = [rnd.randrange(4) for _ in range(u)] + [99, 0, 1] * T
    a = [rnd.randrange(M) for _ in range(u)] + [R - 1, 1 << 64, M] * T
    b = [rnd.randrange(M) for _ in range(u)] + [0, R - 2, M + 1] * T
    cols = [op[:T], a[:T], b[:T]]
    units = [(0, 1, 2, 2), (0, 2, 1)]
    tail = [rnd.randrange(R) for _ in range(3 * (T - u))]
    want, st = run(eng, srs, cols, program, units, rnd, u, tail)
    assert st == {"counts": [0, 0], "first": [None, None], "unknown": [0, 0], "first_unknown": [None, None]}
    for c in range(3):
        assert want[c][u:] == tail[c * (T - u):(c + 1) * (T - u)]
    cols[0][u - 1], cols[1][u - 1] = 0, 1 << 64                                # the last row read is out of range
    _, st = run(eng, srs, cols, program, units, rnd, u, tail)
    assert st["counts"] == [1, 1] and st["first"] == [u - 1, u - 1] and st["unknown"] == [0, 0]
    _, st = run(eng, srs, cols, program, units, rnd)                           # read in full, the rows behind count too
    assert st["unknown"] == [len([c for c in cols[0][u:] if c == 99])] * 2 and st["first_unknown"] == [u, u]
    assert st["counts"][0] > 1
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 6
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    srs = oc.srs_gen(be(SEED_X), be(SEED_Y), lg + 1, 1, 0)
    rnd = random.Random(7000)
    program = [("mulhsu", 32), None, ("sext", 32, ("imm", 8)), ("rotr", 33)]
    cols = [[rnd.randrange(5) for _ in range(T)], [rnd.randrange(1 << 34) for _ in range(T)], [rnd.randrange(1 << 33) for _ in range(T)]]
    units = [(0, 1, 2, 2), (0, 2, 1)]
    want, want_st = aref.alu_columns(cols, program, units)
    want_c = [oc.commit(srs, row_bytes(r), True) for r in want]

    def fresh_ok(sets):
        out, st = eng.commit_alu(sets, program, units)
        out.release()
        assert out.commitments == want_c and st == want_st

    I = commit_sets(eng, cols, (1, 2))
    fresh_ok(I)
    live = eng.rows_stats()
    lib = _native.load()
    E_ARG = _native.KZG_E_ARG
    hi = (ctypes.c_uint64 * 2)(I[0].handle, I[1].handle)
    c, h = ctypes.create_string_buffer(48 * 16), ctypes.c_uint64(0)
    st4 = [(ctypes.c_uint64 * 16)() for _ in range(4)]
    AND, ADD, SPLIT, SEXT, IMM = _native.KZG_ALU_AND, _native.KZG_ALU_ADD, _native.KZG_ALU_SPLIT, _native.KZG_ALU_SEXT, _native.KZG_ALU_IMM
    good_p, good_u = [(ADD, 8, 0, 0, 0)], [(0, 1, 2, 1)]

    def raw(prog, us, opts=None, n=2, n_entries=None, n_units=None):
        pa = (_native.AluEntry * max(len(prog), 1))(*[_native.AluEntry(*r) for r in prog])
        ua = (_native.AluUnit * max(len(us), 1))(*[_native.AluUnit(*r) for r in us])
        return lib.kzg_rows_commit_alu(eng._h, n, hi, len(prog) if n_entries is None else n_entries, pa,
                                       len(us) if n_units is None else n_units, ua, ctypes.byref(opts) if opts else None, c,
                                       st4[0], st4[1], st4[2], st4[3], ctypes.byref(h))

    def refused(rc, why):
        msg = lib.kzg_last_error(eng._h)
        assert rc == E_ARG and msg.startswith(b"alu: ") and why in msg, (rc, msg)
        assert eng.rows_stats() == live
        fresh_ok(I)

    # the program: (kind, width, imm, flags, pad)
    refused(raw([], good_u, n_entries=0), b"n_entries")
    refused(raw(good_p * 65, good_u), b"n_entries")
    refused(raw([(24, 8, 0, 0, 0)], good_u), b"unknown kind")
    refused(raw([(ADD, 0, 0, 0, 0)], good_u), b"width must be in [1, 64]")
    refused(raw([(ADD, 65, 0, 0, 0)], good_u), b"width must be in [1, 64]")
    refused(raw([(ADD, 8, 0, 2, 0)], good_u), b"flags")
    refused(raw([(ADD, 8, 0, 0, 1)], good_u), b"pad")
    refused(raw([(0, 8, 0, 0, 0)], good_u), b"idle entry")
    refused(raw([(0, 0, 1, 0, 0)], good_u), b"idle entry")
    refused(raw([(0, 0, 0, IMM, 0)], good_u), b"idle entry")
    refused(raw([(ADD, 8, 256, IMM, 0)], good_u), b"immediate must be below")
    refused(raw([(ADD, 63, 1 << 63, IMM, 0)], good_u), b"immediate must be below")
    refused(raw([(SPLIT, 8, 9, IMM, 0)], good_u), b"immediate must be below")
    refused(raw([(SEXT, 64, 65, IMM, 0)], good_u), b"immediate must be below")
    refused(raw([(SEXT, 8, 0, IMM, 0)], good_u), b"immediate must be below")
    refused(raw([(ADD, 8, 5, 0, 0)], good_u), b"immediate must be 0")
    # the units: (op_row, a, b, count)
    refused(raw(good_p, [], n_units=0), b"n_units")
    refused(raw(good_p, good_u * 9), b"n_units")
    refused(raw(good_p, [(0, 1, 2, 0)]), b"count must be")
    refused(raw(good_p, [(0, 1, 2, 3)]), b"count must be")
    refused(raw([(AND, 8, 0, 0, 0), (0, 0, 0, 0, 0)], [(0, 1, 2, 2)]), b"count must be")
    refused(raw(good_p, [(3, 1, 2, 1)]), b"a row must index")                                    # 3 rows: 0 .. 2
    refused(raw(good_p, [(0, 3, 2, 1)]), b"a row must index")
    refused(raw(good_p, [(0, 1, 2, 1), (0, 1, 2 ** 31, 1)]), b"a row must index")
    refused(raw(good_p, good_u, n=0), b"number of handles")
    refused(raw(good_p, good_u, n=17), b"number of handles")
    # the largest immediates that fit are taken; a program of idle entries alone writes zero rows
    assert raw([(ADD, 64, (1 << 64) - 1, IMM, 0), (SPLIT, 64, 64, IMM, 0), (SEXT, 8, 8, IMM, 0), (0, 0, 0, 0, 0)], [(0, 1, 2, 2)]) == 0
    eng.release_rows(h.value)
    assert raw([(0, 0, 0, 0, 0)] * 64, [(0, 1, 2, 1)]) == 0
    assert c.raw[:48] == oc.commit(srs, row_bytes([0] * T), True)
    eng.release_rows(h.value)
    assert eng.rows_stats() == live
    # the layout: every tail error of the integer call
    tl = b"".join(bt([rnd.randrange(R) for _ in range(4)]))
    big = R.to_bytes(32, "big")
    for usable, tail, why in ((T, tl, b"usable must be in"), (2 ** 40, tl, b"usable must be in"),
                              (T - 33, tl, b"KZG_MAX_BLIND_ROWS"), (T - 4, None, b"tail_be32 must be given"),
                              (0, tl, b"plain layout"), (T - 4, tl[:-32] + big, b"canonical"),
                              (T - 4, b"\xff" * 32 + tl[32:], b"canonical")):
        refused(raw(good_p, good_u, _native.DeriveOpts(usable, tail)), why)
    arg_error(lambda: eng.commit_alu(I, program, units, 0), "usable")
    arg_error(lambda: eng.commit_alu(I, program, units, T - 4, [be(1)] * 11), "exactly")
    arg_error(lambda: eng.commit_alu(I, program, units, None, [be(1)]), "tail needs usable")
    arg_error(lambda: eng.commit_alu(I, [("nand", 8)], units), "alu: unknown kind")
    assert raw(good_p, good_u, _native.DeriveOpts(0, None)) == 0             # usable = 0 spelled out: the plain layout
    eng.release_rows(h.value)
    assert eng.rows_stats() == live
    # handles
    other = commit_sets(eng, cols[1:], (2,), i=1)                  # another worker
    arg_error(lambda: eng.commit_alu([I[0]] + other, program, units), "one worker")
    short = eng.commit_rows(0, [row_bytes(r[:T // 2]) for r in cols[1:]])      # another length
    arg_error(lambda: eng.commit_alu([I[0], short], program, units), "one worker and have one row length")
    release(other + [short])
    gone = commit_sets(eng, cols[1:], (2,))
    release(gone)
    arg_error(lambda: eng.commit_alu([I[0]] + gone, program, units), "released")
    arg_error(lambda: eng.commit_alu([2 ** 40], [("and", 8)], [(0, 0, 0)]), "unknown")
    arg_error(lambda: eng.commit_alu(I * 6, program, units), "KZG_MAX_BATCH_OPEN rows")    # 18 rows
    fresh_ok(I)
    # the 65th live set
    fill = [eng.commit_rows(0, [row_bytes(cols[0])]) for _ in range(_native.KZG_MAX_ROW_SETS - 2)]
    assert eng.rows_stats()[0] == _native.KZG_MAX_ROW_SETS
    arg_error(lambda: eng.commit_alu(I, program, units), "KZG_MAX_ROW_SETS", code=_native.KZG_E_BUSY)
    fill.pop().release()
    fresh_ok(I)
    release(fill)
    # stale after an SRS load; the new set opens, goes stale and releases like any other
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.commit_alu(I, program, units), "SRS")
    release(I)
    I = commit_sets(eng, cols, (3,))
    out, st = eng.commit_alu(I, program, units)
    assert out.commitments == want_c and st == want_st
    x = be(rnd.randrange(R))
    ys, proofs = eng.open_rows([out], [x], [[0, 1, 2]], [be(rnd.randrange(R))])[:2]
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
    tx, ty = 0xABCDEF0778, 0x13579BF9
    rnd = random.Random(8000)
    program = [("mulh", 32), ("div", 32), None, ("sra", 32, ("imm", 5)), ("lt", 64)]
    units = [(0, 1, 2, 2), (0, 2, 1)]
    recs = HipEngine.alu_program(program)
    pa = (_native.AluEntry * len(recs))(*[_native.AluEntry(*r) for r in recs])
    ua = (_native.AluUnit * 2)(*[_native.AluUnit(*u) for u in HipEngine.alu_units(units, recs)])
    mk = lambda: [[rnd.randrange(6) for _ in range(T)], [rnd.randrange(1 << 33) for _ in range(T)],   # noqa: E731
                  [rnd.randrange(1 << 32) for _ in range(T)]]
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(1, (ctypes.c_int * 1)(0), ctypes.byref(mh)) == 0
    u = T - 3
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    none = lambda vs: [None if v == _native.KZG_ALU_NONE else v for v in vs]   # noqa: E731
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        c, cc = ctypes.create_string_buffer(48 * 3), ctypes.create_string_buffer(48 * 3)
        st4 = [(ctypes.c_uint64 * 2)() for _ in range(4)]
        made = {}
        for i in range(M):
            cols = mk()
            tail = b"".join(bt([rnd.randrange(R) for _ in range(3 * (T - u))]))
            I = commit_sets(single, cols, (3,), i=i)
            plain, ps = single.commit_alu(I, program, units)
            lay, ls = single.commit_alu(I, program, units, u, [tail[j:j + 32] for j in range(0, len(tail), 32)])
            release(I + [plain, lay])
            hi, hz = ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 3, b"".join(row_bytes(r) for r in cols), T, 1, cc, ctypes.byref(hi)) == 0
            ai = (ctypes.c_uint64 * 1)(hi.value)
            made[i] = [hi.value]
            for opts, ref, rs in ((None, plain, ps), (_native.DeriveOpts(u, tail), lay, ls)):
                assert lib.kzg_multi_rows_commit_alu(mh, i, 1, ai, len(recs), pa, 2, ua, ctypes.byref(opts) if opts else None, c,
                                                     st4[0], st4[1], st4[2], st4[3], ctypes.byref(hz)) == 0, i
                assert c.raw == b"".join(ref.commitments)
                assert {"counts": list(st4[0]), "first": none(st4[1]), "unknown": list(st4[2]), "first_unknown": none(st4[3])} == rs
                made[i].append(hz.value)
        ai = (ctypes.c_uint64 * 1)(made[1][0])                     # worker 1's set under index 0
        assert lib.kzg_multi_rows_commit_alu(mh, 0, 1, ai, len(recs), pa, 2, ua, None, c, st4[0], st4[1], st4[2], st4[3],
                                             ctypes.byref(hz)) == _native.KZG_E_ARG
        for i in range(M):
            for hh in made[i]:
                assert lib.kzg_multi_rows_release(mh, i, hh) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)

    # the text clients over the engine: the same bytes as a commit of the reference rows
    jp = [None if e is None else [e[0], e[1]] + ([list(e[2])] if len(e) == 3 else []) for e in program]
    ju = [list(un) for un in units]

    def through(client, workers):
        for i in workers:
            cols = mk()
            tail = [rnd.randrange(R) for _ in range(3 * (T - u))]
            a = client.worker_commit_rows(i, [fr(col) for col in cols]).json()["handle"]
            for usable, tl in ((None, []), (u, tail)):
                want, st = aref.alu_columns(cols, program, units, usable, tl)
                ref = client.worker_commit_rows(i, [fr(col) for col in want]).json()
                r = client.worker_commit_alu([a], jp, ju, usable, fr(tl))
                assert r.status_code == 200, r.json()
                body = r.json()
                assert body["commitments"] == ref["commitments"]
                assert {k: body[k] for k in st} == st
                cells = client.worker_read_rows([body["handle"]], 1, 0, 8, "u64").json()["cells"]
                assert cells == want[1][:8]
                for hh in (ref["handle"], body["handle"]):
                    assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_alu([a], [["nand", 8]], ju).status_code == 400
            assert client.worker_commit_alu([a], [["and", 65]], ju).status_code == 400
            assert client.worker_commit_alu([a], [["and", 8, ["imm", 256]]], ju).status_code == 400
            assert client.worker_commit_alu([a], jp, [[0, 1, 3]]).status_code == 400           # 3 rows: 0 .. 2
            assert client.worker_commit_alu([a], jp, ju, None, fr([1])).status_code == 400
            assert client.worker_release_rows(a).status_code == 200
            assert client.worker_commit_alu([a], jp, ju).status_code == 400

    single.close()
    for client in (Client(seed=79), MultiDeviceClient(devices=[0], seed=79)):
        client.start(scale=scale, machines_scale=ms)
        try:
            through(client, range(M))
        finally:
            client.stop()
