"""GPU tests (`-m gpu`) of kzg_rows_commit_sha256: the SHA-256 compression of resident rows, one per row, as a check against
expected rows, or as the chained round trace in blocks of P >= 72 rows, computed and committed on the device.  The expected
rows come from the definition in Python integers (tests/sha256_ref.py), which tests/test_sha256_cpu.py pins against hashlib and
the gate identities.  Every committed set is compared with commit_rows of the reference rows byte for byte and cell by cell
through read_rows.  (The refusal of T above 2^32 cannot be reached with a set that fits a device.)"""
import ctypes
import hashlib
import random

import pytest

from tests import sha256_ref as sr
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x5A256D01, 0x5A256D02
M32 = 0xffffffff
ALL = list(sr.NAMES)


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


def read_all(eng, rset):
    out = []
    for c in range(rset.k):
        raw = eng.read_rows([rset], c, 0, rset.T, "fr")[0]
        out.append([int.from_bytes(raw[32 * t:32 * t + 32], "big") for t in range(rset.T)])
    return out


def run(eng, cols, units, usable=None, tail=(), sizes=None):
    """commit `cols`, build on the device, compare statistics, commitments and cells with the reference; returns (rows, stats)"""
    want, stats = sr.columns(cols, units, usable, tail)
    T = len(cols[0])
    S = commit_sets(eng, cols, sizes or (len(cols),))
    try:
        inside = eng.rows_stats()
        out, got = eng.commit_sha256(S, units, usable, bt(tail))
        if not want:
            assert out is None and got == stats and eng.rows_stats() == inside, (got, stats)
            return want, stats
        try:
            assert got == stats, (got, stats)
            assert (out.k, out.T, len(out.commitments)) == (len(want), T, len(want))
            ref = eng.commit_rows(0, [row_bytes(r) for r in want])
            try:
                assert out.commitments == ref.commitments
            finally:
                ref.release()
            assert read_all(eng, out) == want
        finally:
            out.release()
    finally:
        release(S)
    return want, stats


def words(k, T, rnd):
    """k columns of random 32-bit words whose first rows hold the edges"""
    cols = [[rnd.randrange(1 << 32) for _ in range(T)] for _ in range(k)]
    for j, c in enumerate(cols):
        c[0], c[1], c[2] = 0, M32, (0 if j % 2 else M32)
    return cols


def rounds(**kw):
    return dict({"mode": "rounds", "msg": 0, "start": None, "period": 72, "iv": None, "cols": ["w", "a", "e"]}, **kw)


def chaining_value(rows, q):
    """(A[71], .., A[68], E[71], .., E[68]) of the block at row q from the columns a, e"""
    a, e = rows
    return [a[q + 71], a[q + 70], a[q + 69], a[q + 68], e[q + 71], e[q + 70], e[q + 69], e[q + 68]]


# ---------------------------------------------------------------------------------------------------- rounds: tails, alignment
@pytest.mark.parametrize("lg,P,usable,blocks", [(8, 72, None, 3), (8, 73, None, 3), (8, 128, None, 2), (6, 72, None, 0), (8, 80, 230, 2)])
def test_rounds_tails_and_alignment(engines, lg, P, usable, blocks):
    """T = 256 with P = 72: three blocks and 40 zero rows; P = 73 and 128 leave zero rows behind every block; T = 64 holds no
    block at all: every column zero; usable = 230 with P = 80 cuts the third block [160, 240), which is not started, and the
    tail follows (at most KZG_MAX_BLIND_ROWS = 32 rows may lie behind `usable`, so that usable = 200 of 256 rows is refused)"""
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(100 + P + lg)
    cols = words(2, T, rnd)
    cols[1] = [rnd.randrange(2) for _ in range(T)]
    tail = [rnd.randrange(R) for _ in range(12 * (T - usable))] if usable else ()
    want, st = run(eng, cols, [rounds(start=1, period=P, cols=ALL)], usable, tail)
    n = usable or T
    assert st["blocks"] == [blocks] and st["counts"] == [0] and len(want) == 12
    assert all(not any(row[blocks * P:n]) for row in want)
    if not blocks:
        assert want == [[0] * T] * 12 and st["messages"] == [0]
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- rounds: chaining
def message_columns(messages, P, T):
    msg, start, ends = [0] * T, [0] * T, []
    b = 0
    for m in messages:
        for k, blk in enumerate(sr.pad(m)):
            start[b * P] = (k == 0) * (1 + b)   # (any non-zero word starts a message)
            msg[b * P + 4:b * P + 20] = blk
            b += 1
        ends.append((b - 1) * P)
    assert b * P <= T
    return msg, start, ends, b


def test_chained_messages_give_hashlib_digests(engines):
    """messages of 1, 2, 1, 3 and 2 blocks one after another (an irregular start column): the rows 68 .. 71 of each last block"""
    eng, P = engines(10), 73
    messages = [b"", bytes(range(56)), b"abc", bytes(range(120)), bytes(64)]
    msg, start, ends, b = message_columns(messages, P, 1 << 10)
    want, st = run(eng, [msg, start], [rounds(start=1, period=P, cols=["a", "e"])])
    assert st["messages"] == [len(messages)] and st["blocks"] == [(1 << 10) // P]   # (the zero blocks behind continue the last one)
    for m, q in zip(messages, ends):
        assert sr.digest_bytes(chaining_value(want, q)) == hashlib.sha256(m).digest()


@pytest.mark.parametrize("shape", ["null", "zero", "alternating", "irregular_sha224"])
def test_start_conventions(engines, shape):
    eng, T, P = engines(9), 512, 72
    rnd = random.Random(300)
    cols = words(2, T, rnd)
    iv = None
    if shape == "null":
        unit = rounds(cols=["e", "w", "a"])
    else:
        cols[1] = [0] * T
        if shape == "alternating":
            for b in range(0, 7, 2):
                cols[1][b * P] = M32
        elif shape == "irregular_sha224":
            iv = list(sr.IV224)
            for b in (1, 2, 5):
                cols[1][b * P] = b
            cols[1][3 * P + 1] = 1   # not at a block's first row: not read
        unit = rounds(start=1, iv=iv, cols=["e", "w", "a"])
    want, st = run(eng, cols, [unit])
    assert st["messages"] == [{"null": 7, "zero": 1, "alternating": 4, "irregular_sha224": 4}[shape]]
    if shape == "irregular_sha224":   # blocks 2 .. 4 are one three-block message from the SHA-224 initial value
        H = list(sr.IV224)
        for b in (2, 3, 4):
            H = sr.compress(H, cols[0][b * P + 4:b * P + 20])
        assert chaining_value([want[2], want[0]], 4 * P) == H


@pytest.mark.parametrize("single", [False, True])
def test_rounds_past_one_workgroup(engines, single):
    """T = 2^15, P = 72: 455 blocks, so that block indices cross a workgroup boundary: every block a start (455 lanes), and one
    message over all blocks (one lane walks them)"""
    eng, T = engines(15), 1 << 15
    rnd = random.Random(400)
    cols = [[rnd.randrange(1 << 32) for _ in range(T)], [0] * T]
    _, st = run(eng, cols, [rounds(start=1 if single else None, cols=["a", "w", "e"])])
    assert st["blocks"] == [455] and st["messages"] == [1 if single else 455]


# ---------------------------------------------------------------------------------------------------- rounds: columns
@pytest.mark.parametrize("names", [ALL[0:4], ALL[4:8], ALL[8:12]])
def test_every_column_name_alone(engines, names):
    eng, T = engines(8), 256
    cols = words(2, T, random.Random(500))
    cols[1] = [0] * T
    want, _ = run(eng, cols, [rounds(start=1, cols=[name]) for name in names])
    assert len(want) == 4


def test_all_twelve_columns_and_a_subset_out_of_order(engines):
    eng, T = engines(8), 256
    cols = words(1, T, random.Random(600))
    full, _ = run(eng, cols, [rounds(cols=ALL)])
    part, _ = run(eng, cols, [rounds(cols=["ch", "cw", "a", "sig1", "ce"])])
    assert part == [full[ALL.index(name)] for name in ("ch", "cw", "a", "sig1", "ce")]
    assert max(full[3]) <= 3 and max(full[4]) <= 6 and max(full[5]) <= 5 and any(full[3]) and any(full[4]) and any(full[5])


# ---------------------------------------------------------------------------------------------------- row units
@pytest.mark.parametrize("lg,usable", [(8, None), (9, 490)])
def test_row_units(engines, lg, usable):
    """T = 256 is one full workgroup; T = 512 with usable = 490 a full and a partial one, with the tail behind (usable = 300
    would leave more than KZG_MAX_BLIND_ROWS rows behind it)"""
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(700 + lg)
    cols = words(16, T, rnd)
    if usable:
        for c in cols:
            c[usable:] = [R - 1 - t for t in range(T - usable)]   # would be counted were they read
    units = [{"mode": "row", "state": "iv", "msg": list(range(16)), "out": list(range(8))},
             {"mode": "row", "state": list(range(8)), "msg": list(reversed(range(16))), "out": [7, 0, 3]}]
    tail = [rnd.randrange(R) for _ in range(11 * (T - usable))] if usable else ()
    want, st = run(eng, cols, units, usable, tail, sizes=(7, 9))
    assert st["blocks"] == [usable or T] * 2 and st["counts"] == [0, 0] and st["messages"] == [0, 0]
    assert [want[j][5] for j in range(8)] == sr.compress(sr.IV, [cols[j][5] for j in range(16)])
    assert eng.rows_stats() == before


def test_immediates_mixed_with_rows_and_one_row_in_several_slots(engines):
    eng, T = engines(6), 64
    cols = words(3, T, random.Random(800))
    units = [{"mode": "row", "state": [0, ("imm", 0), 1, ("imm", M32), 0, 0, 2, ("imm", 7)],
              "msg": [2, 2, ("imm", 1 << 31), 0, 1] + [("imm", j) for j in range(10)] + [0], "out": [1, 6]},
             {"mode": "row", "state": "iv", "msg": [1] * 16, "out": [0]}]
    run(eng, cols, units)


def test_a_unit_of_immediates_alone_gives_the_digest_of_abc(engines):
    eng, T = engines(6), 64
    cols = words(1, T, random.Random(900))
    unit = {"mode": "row", "state": "iv", "msg": [("imm", w) for w in sr.pad(b"abc")[0]], "out": list(range(8))}
    want, st = run(eng, cols, [unit])
    assert st["counts"] == [0] and st["blocks"] == [T]
    for t in (0, 1, T - 1):
        assert sr.digest_bytes([want[j][t] for j in range(8)]).hex() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"


def test_a_merkle_node_is_two_calls(engines):
    """the 2-to-1 hash of 32-byte nodes, per row: the first call from the standard initial value over the 16 words, the second
    from the first call's set with the padding block as immediates; the digests against hashlib.sha256 of the 64 bytes"""
    eng, T = engines(6), 64
    cols = words(16, T, random.Random(1000))
    S = commit_sets(eng, cols, (16,))
    first, _ = eng.commit_sha256(S, [{"mode": "row", "state": "iv", "msg": list(range(16)), "out": list(range(8))}])
    padding = sr.pad(bytes(64))[1]
    second, st = eng.commit_sha256([first], [{"mode": "row", "state": list(range(8)), "msg": [("imm", w) for w in padding],
                                             "out": list(range(8))}])
    try:
        got = read_all(eng, second)
        assert st["counts"] == [0]
        for t in range(T):
            node = b"".join(cols[j][t].to_bytes(4, "big") for j in range(16))
            assert sr.digest_bytes([got[j][t] for j in range(8)]) == hashlib.sha256(node).digest(), t
    finally:
        release(S + [first, second])


# ---------------------------------------------------------------------------------------------------- checks
def test_check_mode(engines):
    """a clean check: mismatch 0, no set, kzg_rows_stats unchanged; one corrupted expected cell is found with its row"""
    eng, T = engines(9), 512
    before = eng.rows_stats()
    cols = words(14, T, random.Random(1100))
    unit = {"mode": "row", "state": "iv", "msg": list(range(14)) + [("imm", 1), ("imm", M32)], "out": [0, 5]}   # 14 + 2 rows: sixteen
    h, _ = sr.columns(cols, [unit])
    _, st = run(eng, cols + h, [dict(unit, expect=[14, 15])], sizes=(14, 2))
    assert st["mismatch"] == [0] and st["first_mismatch"] == [None]
    h[1][300] ^= 1
    _, st = run(eng, cols + h, [dict(unit, expect=[14, 15]), dict(unit, out=[5, 0], expect=[15, 14]), dict(unit, out=[0], expect=[14])],
                sizes=(14, 2))
    assert st["mismatch"] == [1, 1, 0] and st["first_mismatch"] == [300, 300, None]
    h[0][299], h[0][7] = R - 1, (1 << 32) + h[0][7]   # an expected cell beyond 2^32 differs: it is compared, not reduced
    h[1][495] ^= 1                                     # behind `usable`: not compared
    _, st = run(eng, cols + h, [dict(unit, expect=[14, 15])], 490, sizes=(14, 2))
    assert st["mismatch"] == [3] and st["first_mismatch"] == [7] and st["blocks"] == [490] and st["counts"] == [0]
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- over-range cells
def test_over_range_cells_are_reduced_and_counted_once_per_cell(engines):
    eng, T, P = engines(9), 512, 72
    rnd = random.Random(1200)
    cols = words(4, T, rnd)
    cols[0][9], cols[0][300], cols[1][9], cols[2][511] = 1 << 32, (1 << 32) + 3, R - 1, (1 << 32) + 5
    # row units: column 0 serves three slots and is counted once; unit 1 reads column 3 only
    units = [{"mode": "row", "state": [2] + [("imm", 1)] * 7, "msg": [0, 0, 1, 0] + [("imm", 0)] * 12, "out": [0]},
             {"mode": "row", "state": "iv", "msg": [3] * 16, "out": [1]}]
    _, st = run(eng, cols, units)
    assert st["counts"] == [4, 0] and st["first"] == [9, None]
    _, st = run(eng, cols, units, 490, [1, 2] * 22)
    assert st["counts"] == [3, 0] and st["first"] == [9, None]   # (row 511 lies behind `usable`: never read)
    # a rounds unit reads msg at rows b P + 4 .. b P + 19 and start at rows b P only
    msg, start = cols[3], [0] * T
    msg[3], msg[20], msg[72], msg[P + 4], msg[2 * P + 19] = R - 1, 1 << 32, 1 << 32, (1 << 32) + 3, R - 1   # the last two are read
    start[1], start[P], start[3 * P] = R - 1, 1 << 32, (1 << 33) + 1   # the last two are read; 2^32 reduces to 0: no start
    want, st = run(eng, [msg, start], [rounds(start=1, cols=["w"])])
    assert st["counts"] == [4] and st["first"] == [P] and st["messages"] == [2]
    assert want[0][P + 4] == 3 and want[0][2 * P + 19] == (R - 1) & M32


# ---------------------------------------------------------------------------------------------------- several units
def test_several_units_fill_sixteen_rows_in_order(engines):
    eng, T = engines(8), 256
    before = eng.rows_stats()
    cols = words(16, T, random.Random(1300))
    cols[15] = [int(t % 144 == 0) for t in range(T)]
    units = [{"mode": "row", "state": "iv", "msg": list(range(16)), "out": [3, 1, 0, 2]},
             rounds(msg=2, start=15, period=72, cols=["sum1", "w", "a", "e", "ca"]),
             {"mode": "row", "state": [1] * 8, "msg": [0] * 16, "out": [7]},
             rounds(msg=0, period=100, iv=list(sr.IV224), cols=["e", "ce", "maj", "cw", "sig0", "ch"])]
    want, st = run(eng, cols, units, sizes=(5, 11))
    assert len(want) == 16 and st["blocks"] == [256, 3, 256, 2] and st["messages"] == [0, 2, 0, 2]
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_their_order_and_leak_free_recovery(hip):
    eng = hip()
    lg = 7
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg, 0)
    cols = words(4, T, random.Random(1400))
    units = [{"mode": "row", "state": "iv", "msg": [0, 1, ("imm", 3)] + [2] * 13, "out": [1, 0]}, rounds(msg=3, start=2, cols=["a", "cw"])]
    want, stats = sr.columns(cols, units)
    I = commit_sets(eng, cols, (4,))

    def fresh_ok():
        out, got = eng.commit_sha256(I, units)
        try:
            assert got == stats and read_all(eng, out) == want
        finally:
            out.release()

    fresh_ok()
    live = eng.rows_stats()
    lib = _native.load()
    hi = (ctypes.c_uint64 * 1)(I[0].handle)
    c, h = ctypes.create_string_buffer(48 * 16), ctypes.c_uint64(0)
    st = [(ctypes.c_uint64 * 8)() for _ in range(6)]
    row, rnds = eng.sha256_call(units)
    IMM = _native.KZG_SHA256_IMM
    names = ("mode", "flags", "n_out", "period", "start", "state", "state_imm", "msg", "msg_imm", "out", "expect")
    edit = lambda base, **kw: tuple(kw.get(f, v) for f, v in zip(names, base))   # noqa: E731

    def raw(recs, opts=None, n_units=None, handles=hi, n_handles=1):
        arr = (_native.Sha256Unit * max(len(recs), 1))(*[eng.sha256_unit_struct(r) for r in recs])
        return lib.kzg_rows_commit_sha256(eng._h, n_handles, handles, len(recs) if n_units is None else n_units, arr,
                                          ctypes.byref(opts) if opts else None, c, *st, ctypes.byref(h))

    def refused(rc, text):
        msg = lib.kzg_last_error(eng._h)
        assert rc == _native.KZG_E_ARG and msg == b"sha256: " + text, (rc, msg)
        assert eng.rows_stats() == live

    z8, z16 = [0] * 8, [0] * 16
    refused(raw([row], n_handles=0), b"the number of handles must be in [1, KZG_MAX_BATCH_OPEN]")
    refused(raw([], n_units=0), b"n_units must be in [1, KZG_SHA256_MAX_UNITS]")
    refused(raw([row] * 5), b"n_units must be in [1, KZG_SHA256_MAX_UNITS]")
    refused(raw([edit(row, mode=0)]), b"unknown mode (KZG_SHA256_ROW or KZG_SHA256_ROUNDS)")
    refused(raw([edit(row, mode=3, flags=4)]), b"unknown mode (KZG_SHA256_ROW or KZG_SHA256_ROUNDS)")   # mode before flags
    refused(raw([edit(row, flags=4)]), b"flags must be a combination of KZG_SHA256_CHECK and KZG_SHA256_STD_IV")
    refused(raw([edit(rnds, flags=3, period=3)]), b"expect (KZG_SHA256_CHECK) belongs to ROW units, not to ROUNDS")   # before the period
    refused(raw([edit(rnds, period=71, n_out=0)]), b"the period P of a ROUNDS unit must be at least 72 (0 on a ROW unit)")
    refused(raw([edit(row, period=72)]), b"the period P of a ROUNDS unit must be at least 72 (0 on a ROW unit)")
    refused(raw([edit(row, n_out=0)]), b"n_out must be in [1, 8] on a ROW unit and in [1, 12] on a ROUNDS unit")
    refused(raw([edit(row, n_out=9)]), b"n_out must be in [1, 8] on a ROW unit and in [1, 12] on a ROUNDS unit")
    refused(raw([edit(rnds, n_out=13)]), b"n_out must be in [1, 8] on a ROW unit and in [1, 12] on a ROUNDS unit")
    refused(raw([edit(row, out=[8] + [0] * 11)]), b"an out index must be below 8 (ROUNDS: a column id below KZG_SHA256_N_COLS)")
    refused(raw([edit(rnds, out=[11, 12] + [0] * 10)]), b"an out index must be below 8 (ROUNDS: a column id below KZG_SHA256_N_COLS)")
    refused(raw([edit(row, out=[1, 1] + [0] * 10, state=z8)]), b"an out index is repeated")   # before the state
    refused(raw([edit(row, state=[0] + [IMM] * 7)]), b"a state entry must be KZG_SHA256_IMM on a ROUNDS unit and with KZG_SHA256_STD_IV")
    refused(raw([edit(rnds, state=[0] + [IMM] * 7)]), b"a state entry must be KZG_SHA256_IMM on a ROUNDS unit and with KZG_SHA256_STD_IV")
    refused(raw([edit(row, state_imm=[1] + [0] * 7)]), b"the immediate must be 0 with KZG_SHA256_STD_IV")
    refused(raw([edit(row, flags=0, state=z8, state_imm=[1] + [0] * 7)]), b"the immediate must be 0 beside a row")
    refused(raw([edit(row, msg_imm=[5] + [0] * 15)]), b"the immediate must be 0 beside a row")
    refused(raw([edit(rnds, msg=[IMM] + [0] * 15)]), b"the message of a ROUNDS unit is a row, not an immediate")
    refused(raw([edit(rnds, msg=[3, 1] + [0] * 14)]), b"msg[1 .. 15] and msg_imm must be 0 on a ROUNDS unit")
    refused(raw([edit(row, start=0)]), b"start belongs to ROUNDS units (KZG_SHA256_ABSENT on a ROW unit)")
    many = edit(row, flags=0, state=list(range(8)), msg=list(range(8, 24)), msg_imm=z16)
    refused(raw([many]), b"a call reads at most KZG_MAX_BATCH_OPEN distinct input rows")
    refused(raw([edit(row, n_out=8, out=list(range(8)) + [0] * 4)] * 2 + [rnds]),
            b"n_out, the committed columns of all units, must be at most KZG_MAX_BATCH_OPEN")
    # behind the host checks: the handles, then the rows, then the row length and the layout
    bad_handle = (ctypes.c_uint64 * 1)(2 ** 40)
    rc = raw([edit(row, msg=[4] + [IMM] * 15)], handles=bad_handle)
    assert rc == _native.KZG_E_ARG and lib.kzg_last_error(eng._h).startswith(b"sha256: ") and eng.rows_stats() == live
    refused(raw([edit(row, msg=[4] + [IMM] * 15)]), b"a row must index the concatenated rows of the input sets")
    refused(raw([edit(row, flags=3, expect=[0, 4] + [0] * 6)]), b"a row must index the concatenated rows of the input sets")
    refused(raw([edit(rnds, start=4)], opts=_native.DeriveOpts(T, None)), b"a row must index the concatenated rows of the input sets")
    big = R.to_bytes(32, "big")
    tl = b"".join(bt([random.Random(5).randrange(R) for _ in range(4 * 4)]))
    for usable, tail, text in ((T, tl, b"usable must be in [1, T - 1] (0: all T rows are read)"),
                               (T - 33, tl, b"at most KZG_MAX_BLIND_ROWS rows may lie at or behind row `usable`"),
                               (T - 4, None, b"tail_be32 must be given when usable > 0"),
                               (0, tl, b"tail_be32 must be null in the plain layout (usable = 0)"),
                               (T - 4, tl[:-32] + big, b"tail scalars must be canonical (< r)")):
        refused(raw([row, rnds], opts=_native.DeriveOpts(usable, tail)), text)
    assert raw([edit(row, flags=3, expect=[0, 1] + [0] * 6)], opts=_native.DeriveOpts(T - 4, None)) == 0   # a check needs no tail
    assert h.value == 0 and eng.rows_stats() == live
    fresh_ok()
    for bad, why in ((dict(units[0], mode="sponge"), "unknown mode"), (dict(units[0], out=[8]), "out index"),
                     (dict(units[0], out=[1, 1]), "repeated"), (dict(units[1], period=71), "period P"),
                     (dict(units[1], expect=[0]), "expect belongs"), (dict(units[0], msg=[4] * 16), "concatenated rows"),
                     (dict(units[0], msg=[("imm", 1 << 32)] * 16), "below 2^32"), (dict(units[1], iv=[1 << 32] * 8), "iv must be"),
                     (dict(units[1], cols=["w", "w"]), "repeated"), (dict(units[1], cols=["x"]), "unknown column"),
                     (dict(units[1], cols=[]), "cols must hold"), (dict(units[0], foo=1), "unknown field")):
        arg_error(lambda: eng.commit_sha256(I, [bad]), why)
    arg_error(lambda: eng.commit_sha256(I, units, None, [be(1)]), "tail")
    arg_error(lambda: eng.commit_sha256([2 ** 40], units), "unknown")
    fresh_ok()
    release(I)
    assert eng.rows_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------------- routing
def test_client_and_multi_device_client_return_the_engine_bytes(hip):
    from zkp_subnet_amd import Client, MultiDeviceClient, codec

    scale, ms = 8, 0
    T = 1 << scale
    cols = words(3, T, random.Random(1500))
    cols[2] = [int(t == 72) for t in range(T)]
    units = [{"mode": "row", "state": "iv", "msg": [0, ["imm", 5], 1] + [0] * 13, "out": [1, 0]},
             {"mode": "rounds", "msg": 1, "start": 2, "period": 72, "iv": None, "cols": ["a", "e", "ca"]}]
    plain = [dict(units[0], msg=[0, ("imm", 5), 1] + [0] * 13), units[1]]
    want, stats = sr.columns(cols, plain)
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    for client in (Client(seed=84), MultiDeviceClient(devices=[0], seed=84)):
        client.start(scale=scale, machines_scale=ms)
        try:
            a = client.worker_commit_rows(0, [fr(col) for col in cols]).json()["handle"]
            ref = client.worker_commit_rows(0, [fr(col) for col in want]).json()
            r = client.worker_commit_sha256([a], units)
            assert r.status_code == 200, r.json()
            body = r.json()
            assert body["commitments"] == ref["commitments"]
            assert {k: body[k] for k in stats} == stats
            chk = client.worker_commit_sha256([a, ref["handle"]], [dict(units[0], expect=[3, 4]), dict(units[0], expect=[4, 3])])
            assert chk.status_code == 200, chk.json()
            assert chk.json()["handle"] is None and chk.json()["commitments"] == []
            assert chk.json()["mismatch"][0] == 0 and chk.json()["first_mismatch"] == [None, 0]
            assert client.worker_commit_sha256([a], [dict(units[0], mode="sponge")]).status_code == 400
            assert client.worker_commit_sha256([a], [dict(units[1], period=71)]).status_code == 400
            assert client.worker_commit_sha256([a], units, None, fr([1])).status_code == 400
            for hh in (ref["handle"], body["handle"], a):
                assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_sha256([a], units).status_code == 400
        finally:
            client.stop()
