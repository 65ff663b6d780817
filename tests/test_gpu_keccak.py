"""GPU tests (`-m gpu`) of kzg_rows_commit_keccak: Keccak-f[1600] of resident rows, one per row, as a check against expected
rows, or as the chained round trace in blocks of P >= 125 rows, computed and committed on the device.  The expected rows come
from the definition in Python integers (tests/keccak_ref.py), which tests/test_keccak_cpu.py pins against hashlib and the trace
identities.  Every committed set is compared with commit_rows of the reference rows byte for byte and cell by cell through
read_rows.  (The refusal of T above 2^32 cannot be reached with a set that fits a device.)"""
import ctypes
import hashlib
import random

import pytest

from tests import keccak_ref as kr
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x6EC4A601, 0x6EC4A602
M64 = (1 << 64) - 1
ALL = list(kr.NAMES)
EMPTY_KECCAK256 = "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
STATE = [f"a{x}" for x in range(5)]


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
    want, stats = kr.columns(cols, units, usable, tail)
    T = len(cols[0])
    S = commit_sets(eng, cols, sizes or (len(cols),))
    try:
        inside = eng.rows_stats()
        out, got = eng.commit_keccak(S, units, usable, bt(tail))
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


def lanes(k, T, rnd):
    """k columns of random 64-bit lanes whose first rows hold the edges"""
    cols = [[rnd.randrange(1 << 64) for _ in range(T)] for _ in range(k)]
    for j, c in enumerate(cols):
        c[0], c[1], c[2] = 0, M64, (0 if j % 2 else M64)
    return cols


def rounds(**kw):
    return dict({"mode": "rounds", "msg": [0, 1, 2, 3, 4], "rate": 17, "start": None, "period": 125, "cols": list(STATE)}, **kw)


def outgoing(rows, q):
    """the outgoing state of the block at row q from the columns a0 .. a4"""
    return [rows[x][q + 120 + y] for y in range(5) for x in range(5)]


# ---------------------------------------------------------------------------------------------------- rounds: tails, alignment
@pytest.mark.parametrize("lg,P,usable,blocks", [(8, 125, None, 2), (8, 126, None, 2), (8, 128, None, 2), (6, 125, None, 0),
                                                (8, 125, 250, 2), (8, 125, 249, 1), (8, 125, 230, 1)])
def test_rounds_tails_and_alignment(engines, lg, P, usable, blocks):
    """T = 256 with P = 125: two blocks and six zero rows; P = 126 and 128 leave zero rows behind every block; T = 64 holds no
    block at all: every column zero; usable = 250 holds two blocks exactly, usable = 249 cuts the second, which is not started,
    usable = 230 likewise, and the tail follows (at most KZG_MAX_BLIND_ROWS = 32 rows may lie behind `usable`).  All 25 columns,
    sixteen and nine: a call commits at most sixteen"""
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(100 + P + lg + (usable or 0))
    cols = lanes(6, T, rnd)
    cols[5] = [rnd.randrange(2) for _ in range(T)]
    n = usable or T
    for names in (ALL[:16], ALL[16:]):
        tail = [rnd.randrange(R) for _ in range(len(names) * (T - usable))] if usable else ()
        want, st = run(eng, cols, [rounds(start=5, period=P, cols=names)], usable, tail)
        assert st["perms"] == [blocks] and st["counts"] == [0] and len(want) == len(names)
        assert all(not any(row[blocks * P:n]) for row in want)
        if not blocks:
            assert want == [[0] * T] * len(names) and st["messages"] == [0]
        else:
            assert all(any(row[(blocks - 1) * P:(blocks - 1) * P + 120]) for row in want)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- rounds: chaining
def message_columns(messages, rate, suffix, P, T):
    cols, ends = [[0] * T for _ in range(6)], []
    b = 0
    for m in messages:
        for k, blk in enumerate(kr.pad(m, rate, suffix)):
            cols[5][b * P] = (k == 0) * (1 + b)   # (any non-zero lane starts a message)
            for i, v in enumerate(blk):
                cols[i % 5][b * P + i // 5] = v
            b += 1
        ends.append((b - 1) * P)
    assert b * P <= T
    return cols, ends, b


@pytest.mark.parametrize("rate,suffix,nbytes,ref", [(17, 0x06, 32, lambda m: hashlib.sha3_256(m).digest()),
                                                    (9, 0x06, 64, lambda m: hashlib.sha3_512(m).digest()),
                                                    (21, 0x1f, 32, lambda m: hashlib.shake_128(m).digest(32))],
                         ids=["sha3_256", "sha3_512", "shake_128"])
def test_chained_messages_give_hashlib_digests(engines, rate, suffix, nbytes, ref):
    """T = 1024, P = 125: eight blocks, messages of 1, 2, 1, 3 and 1 blocks one after another (an irregular start column) whose
    lengths straddle the rate: the rows 120 .. 124 of each last block.  The cells of lanes at or above the rate hold values
    at or above 2^64: neither read nor counted"""
    eng, P, nb = engines(10), 125, 8 * rate
    messages = [bytes(range(5)), bytes(k % 251 for k in range(nb)), bytes(k % 7 for k in range(nb - 1)),
                bytes(k % 13 for k in range(2 * nb + 1)), b""]
    cols, ends, b = message_columns(messages, rate, suffix, P, 1 << 10)
    assert b == 8
    for blk in range(8):
        for i in range(rate, 25):
            cols[i % 5][blk * P + i // 5] = (1 << 64) + i
    want, st = run(eng, cols, [rounds(rate=rate, start=5)])
    assert st["messages"] == [len(messages)] and st["perms"] == [8] and st["counts"] == [0] and st["first"] == [None]
    for m, q in zip(messages, ends):
        assert kr.digest_bytes(outgoing(want, q), nbytes) == ref(m)


def test_keccak256_of_the_empty_message(engines):
    eng, T = engines(7), 128
    cols, ends, _ = message_columns([b""], 17, 0x01, 125, T)
    want, st = run(eng, cols, [rounds(start=5)])
    assert kr.digest_bytes(outgoing(want, 0), 32).hex() == EMPTY_KECCAK256 and st["perms"] == [1]


@pytest.mark.parametrize("shape", ["null", "zero", "alternating"])
def test_start_conventions(engines, shape):
    eng, T, P = engines(9), 512, 125
    cols = lanes(6, T, random.Random(300))
    if shape == "null":
        unit = rounds(cols=["t2", "a0", "b4", "p3", "d1"])
    else:
        cols[5] = [0] * T
        if shape == "alternating":
            for b in (0, 2):
                cols[5][b * P] = M64
            cols[5][P + 1] = 1   # not at a block's first row: not read
        unit = rounds(start=5, cols=["t2", "a0", "b4", "p3", "d1"])
    want, st = run(eng, cols, [unit])
    assert st["messages"] == [{"null": 4, "zero": 1, "alternating": 2}[shape]] and st["perms"] == [4]


@pytest.mark.parametrize("single", [False, True])
def test_rounds_past_one_workgroup(engines, single):
    """T = 2^15, P = 125: 262 blocks, so that block indices cross a workgroup boundary: every block a start (262 lanes), and one
    message over all blocks (one lane walks them)"""
    eng, T = engines(15), 1 << 15
    rnd = random.Random(400)
    cols = [[rnd.randrange(1 << 64) for _ in range(T)] for _ in range(5)] + [[0] * T]
    _, st = run(eng, cols, [rounds(start=5 if single else None, cols=["a0", "b3"])])
    assert st["perms"] == [262] and st["messages"] == [1 if single else 262]


# ---------------------------------------------------------------------------------------------------- row units
def merkle_unit(suffix=0x01):
    return {"mode": "row", "in": list(range(8)) + [("imm", suffix)] + [("imm", 0)] * 7 + [("imm", 1 << 63)] + [("imm", 0)] * 8,
            "out": [0, 1, 2, 3]}


def test_sixteen_rows_nine_immediates_sixteen_outputs(engines):
    eng, T = engines(6), 64
    before = eng.rows_stats()
    rnd = random.Random(700)
    cols = lanes(16, T, rnd)
    slots = list(range(16)) + [("imm", v) for v in (0, M64, 1, 1 << 63, 0x0123456789abcdef, 1 << 32, (1 << 32) - 1, 0, 5)]
    rnd.shuffle(slots)
    out = rnd.sample(range(25), 16)
    want, st = run(eng, cols, [{"mode": "row", "in": slots, "out": out}], sizes=(7, 9))
    assert st["perms"] == [T] and st["counts"] == [0] and st["messages"] == [0]
    state = kr.permute([s[1] if isinstance(s, tuple) else cols[s][5] for s in slots])
    assert [want[c][5] for c in range(16)] == [state[j] for j in out]
    assert eng.rows_stats() == before


def test_the_merkle_shape_gives_keccak256_and_sha3_256(engines):
    """Keccak-256 of two 32-byte nodes is one call: 8 rows, 0x01 in lane 8, 2^63 in lane 16, zeros in the capacity"""
    eng, T = engines(6), 64
    cols = lanes(8, T, random.Random(800))
    want, st = run(eng, cols, [merkle_unit(), merkle_unit(0x06)])
    assert st["counts"] == [0, 0] and len(want) == 8
    for t in (0, 1, 2, 17, T - 1):
        node = b"".join(cols[j][t].to_bytes(8, "little") for j in range(8))
        assert kr.digest_bytes([want[j][t] for j in range(4)], 32) == kr.sponge(node, 17, 0x01, 32)
        assert kr.digest_bytes([want[4 + j][t] for j in range(4)], 32) == hashlib.sha3_256(node).digest()


def test_row_unit_with_usable_and_tail_past_one_workgroup(engines):
    """T = 512 with usable = 490: a full workgroup and a partial one, the tail behind; the cells behind `usable` would be
    counted were they read"""
    eng, T, usable = engines(9), 512, 490
    rnd = random.Random(900)
    cols = lanes(8, T, rnd)
    for c in cols:
        c[usable:] = [R - 1 - t for t in range(T - usable)]
    tail = [rnd.randrange(R) for _ in range(4 * (T - usable))]
    want, st = run(eng, cols, [merkle_unit()], usable, tail)
    assert st["perms"] == [usable] and st["counts"] == [0] and want[3][usable:] == tail[3 * (T - usable):]


def test_over_range_and_edge_cells(engines):
    """edge cells 0, 2^64 - 1, 2^64 and r - 1; one row serving two slots is counted once per cell"""
    eng, T = engines(6), 64
    cols = lanes(3, T, random.Random(1000))
    cols[0][3], cols[0][4], cols[0][40], cols[1][4], cols[2][63] = 1 << 64, R - 1, (1 << 64) + 3, R - 1, (1 << 64) + 5
    units = [{"mode": "row", "in": [0, 0, 1, 0, 2] + [("imm", j) for j in range(20)], "out": [0, 24]},
             {"mode": "row", "in": [1] * 16 + [("imm", 0)] * 9, "out": [7]}]
    want, st = run(eng, cols, units)
    assert st["counts"] == [5, 1] and st["first"] == [3, 4]
    assert want[0][3] == kr.permute([0, 0, cols[1][3], 0, cols[2][3]] + list(range(20)))[0]
    assert want[2][4] == kr.permute([(R - 1) & M64] * 16 + [0] * 9)[7]
    _, st = run(eng, cols, units, 60, [1, 2, 3] * 4)
    assert st["counts"] == [4, 1] and st["first"] == [3, 4]   # (row 63 lies behind `usable`: never read)
    # a rounds unit reads msg[x] at block row y for x + 5 y < rate only, and start at the rows b P only; the start column
    # among the message columns is one cell at row b P, counted once
    T, P = 256, 125
    eng = engines(8)
    cols = lanes(5, T, random.Random(1001))
    cols[0][0], cols[0][P], cols[0][P + 1], cols[1][P + 1], cols[2][1], cols[3][P - 1] = (1 << 64) + 9, 1 << 64, R - 1, R - 1, R - 1, R - 1
    want, st = run(eng, cols, [rounds(rate=7, start=0, cols=["a0", "a1", "a2"])])
    # read and over range: (0, 0) once, (0, P) once: it reduces to 0 and starts nothing, (0, P + 1), (1, P + 1); (2, 1) is lane 7
    assert st["counts"] == [4] and st["first"] == [0] and st["messages"] == [1]
    assert want[0][0] == 9


# ---------------------------------------------------------------------------------------------------- checks
def test_check_mode(engines):
    """a clean check: mismatch 0, no set, kzg_rows_stats unchanged; one corrupted expected cell in the last usable row is found
    with its row"""
    eng, T, usable = engines(8), 256, 250
    before = eng.rows_stats()
    cols = lanes(8, T, random.Random(1100))
    unit = merkle_unit()
    h, _ = kr.columns(cols, [unit])
    good = [list(r) for r in h]
    exp = dict(unit, expect=[8, 9, 10, 11])
    _, st = run(eng, cols + h, [exp], sizes=(8, 4))
    assert st["mismatch"] == [0] and st["first_mismatch"] == [None] and st["perms"] == [T]
    h[2][T - 1] ^= 1 << 63
    _, st = run(eng, cols + h, [exp, dict(unit, out=[2, 0], expect=[10, 8]), dict(unit, out=[0], expect=[8])], sizes=(8, 4))
    assert st["mismatch"] == [1, 1, 0] and st["first_mismatch"] == [T - 1, T - 1, None]
    h[2][T - 1] ^= 1 << 63
    h[1][usable - 1] ^= 1                               # the last usable row
    h[0][99], h[0][7] = R - 1, (1 << 64) + h[0][7]      # an expected cell beyond 2^64 differs: it is compared, not reduced
    h[3][usable + 3] ^= 1                               # behind `usable`: not compared
    _, st = run(eng, cols + h, [exp], usable, sizes=(8, 4))
    assert st["mismatch"] == [3] and st["first_mismatch"] == [7] and st["perms"] == [usable] and st["counts"] == [0]
    h[0][99], h[0][7] = good[0][99], good[0][7]
    _, st = run(eng, cols + h, [exp], usable, sizes=(8, 4))
    assert st["mismatch"] == [1] and st["first_mismatch"] == [usable - 1]
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- several units
def test_a_row_unit_and_a_rounds_unit_in_one_call_over_two_handles(engines):
    eng, T = engines(8), 256
    before = eng.rows_stats()
    cols = lanes(14, T, random.Random(1300))
    cols[13] = [int(t == 0) for t in range(T)]
    units = [dict(merkle_unit(), out=[3, 1, 0, 2]),
             rounds(msg=[8, 9, 10, 11, 12], start=13, rate=21, cols=["p4", "a0", "t1", "b2", "d3", "a4"]),
             {"mode": "row", "in": [1] * 25, "out": [24]},
             rounds(msg=[0, 0, 1, 1, 2], period=128, rate=24, cols=["b0", "t0", "d0", "p0", "a3"])]
    want, st = run(eng, cols, units, sizes=(5, 9))
    assert len(want) == 16 and st["perms"] == [256, 2, 256, 2] and st["messages"] == [0, 1, 0, 2]
    arg_error(lambda: eng.commit_keccak([1], units[:2] + [dict(units[2], out=[24, 0]), units[3]]), "n_out")
    arg_error(lambda: eng.commit_keccak([1], [{"mode": "row", "in": list(range(17)) + [("imm", 0)] * 8, "out": [0]}]), "distinct input rows")
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals_their_order_and_leak_free_recovery(hip):
    eng = hip()
    lg = 8
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg, 0)
    cols = lanes(7, T, random.Random(1400))
    units = [{"mode": "row", "in": [0, 1, ("imm", 3)] + [2] * 13 + [("imm", 0)] * 9, "out": [1, 0]},
             rounds(msg=[2, 3, 4, 5, 6], start=0, cols=["a0", "d4"])]
    want, stats = kr.columns(cols, units)
    I = commit_sets(eng, cols, (7,))

    def fresh_ok():
        out, got = eng.commit_keccak(I, units)
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
    row, rnds = eng.keccak_call(units)
    IMM = _native.KZG_KECCAK_IMM
    names = ("mode", "flags", "n_out", "period", "rate", "start", "imm", "in", "out", "expect")
    edit = lambda base, **kw: tuple(kw.get(f, v) for f, v in zip(names, base))   # noqa: E731

    def raw(recs, opts=None, n_units=None, handles=hi, n_handles=1):
        arr = (_native.KeccakUnit * max(len(recs), 1))(*[eng.keccak_unit_struct(r) for r in recs])
        return lib.kzg_rows_commit_keccak(eng._h, n_handles, handles, len(recs) if n_units is None else n_units, arr,
                                          ctypes.byref(opts) if opts else None, c, *st, ctypes.byref(h))

    def refused(rc, text):
        msg = lib.kzg_last_error(eng._h)
        assert rc == _native.KZG_E_ARG and msg == b"keccak: " + text, (rc, msg)
        assert eng.rows_stats() == live

    z16, z25 = [0] * 16, [0] * 25
    refused(raw([row], n_handles=0), b"the number of handles must be in [1, KZG_MAX_BATCH_OPEN]")
    refused(raw([], n_units=0), b"n_units must be in [1, KZG_KECCAK_MAX_UNITS]")
    refused(raw([row] * 5), b"n_units must be in [1, KZG_KECCAK_MAX_UNITS]")
    refused(raw([edit(row, mode=0)]), b"unknown mode (KZG_KECCAK_ROW or KZG_KECCAK_ROUNDS)")
    refused(raw([edit(row, mode=3, flags=4)]), b"unknown mode (KZG_KECCAK_ROW or KZG_KECCAK_ROUNDS)")   # mode before flags
    refused(raw([edit(row, flags=2)]), b"flags must be 0 or KZG_KECCAK_CHECK")
    refused(raw([edit(rnds, flags=1, period=3)]), b"expect (KZG_KECCAK_CHECK) belongs to ROW units, not to ROUNDS")   # before the period
    refused(raw([edit(rnds, period=124, rate=0)]), b"the period P of a ROUNDS unit must be at least 125 (0 on a ROW unit)")
    refused(raw([edit(row, period=125)]), b"the period P of a ROUNDS unit must be at least 125 (0 on a ROW unit)")
    refused(raw([edit(rnds, rate=0, n_out=0)]), b"the rate of a ROUNDS unit must be in [1, 24] lanes (0 on a ROW unit)")
    refused(raw([edit(rnds, rate=25)]), b"the rate of a ROUNDS unit must be in [1, 24] lanes (0 on a ROW unit)")
    refused(raw([edit(row, rate=17)]), b"the rate of a ROUNDS unit must be in [1, 24] lanes (0 on a ROW unit)")
    refused(raw([edit(row, n_out=0)]), b"n_out must be in [1, KZG_KECCAK_MAX_OUT]")
    refused(raw([edit(row, n_out=17)]), b"n_out must be in [1, KZG_KECCAK_MAX_OUT]")
    refused(raw([edit(rnds, n_out=17)]), b"n_out must be in [1, KZG_KECCAK_MAX_OUT]")
    refused(raw([edit(row, out=[25] + [0] * 15)]), b"a lane index must be below 25 (ROUNDS: a column id below KZG_KECCAK_N_COLS)")
    refused(raw([edit(rnds, out=[24, 25] + [0] * 14)]), b"a lane index must be below 25 (ROUNDS: a column id below KZG_KECCAK_N_COLS)")
    refused(raw([edit(row, out=[1, 1] + [0] * 14, imm=[1] * 25)]), b"a lane index or column id is repeated")   # before the slots
    refused(raw([edit(rnds, out=[7, 7] + [0] * 14)]), b"a lane index or column id is repeated")
    refused(raw([edit(row, imm=[5] + [0] * 24)]), b"the immediate must be 0 beside a row")
    refused(raw([edit(rnds, **{"in": [2, 3, IMM, 5, 6] + [0] * 20})]), b"the message columns of a ROUNDS unit are rows, not immediates")
    refused(raw([edit(rnds, **{"in": [2, 3, 4, 5, 6, 1] + [0] * 19})]), b"in[5 .. 24] and imm must be 0 on a ROUNDS unit")
    refused(raw([edit(rnds, imm=[0] * 24 + [1])]), b"in[5 .. 24] and imm must be 0 on a ROUNDS unit")
    refused(raw([edit(row, start=0)]), b"start belongs to ROUNDS units (KZG_KECCAK_ABSENT on a ROW unit)")
    many = edit(row, imm=z25, **{"in": list(range(17)) + [IMM] * 8})
    refused(raw([many]), b"a call reads at most KZG_MAX_BATCH_OPEN distinct input rows")
    refused(raw([edit(row, flags=1, n_out=16, out=list(range(16)), expect=list(range(3, 19)))]),
            b"a call reads at most KZG_MAX_BATCH_OPEN distinct input rows")
    refused(raw([edit(row, n_out=16, out=list(range(16))), rnds]),
            b"n_out, the committed columns of all units, must be at most KZG_MAX_BATCH_OPEN")
    # behind the host checks: the handles, then the rows, then the row length and the layout
    bad_handle = (ctypes.c_uint64 * 1)(2 ** 40)
    one = [7] + [IMM] * 24
    rc = raw([edit(row, **{"in": one})], handles=bad_handle)
    assert rc == _native.KZG_E_ARG and lib.kzg_last_error(eng._h).startswith(b"keccak: ") and eng.rows_stats() == live
    refused(raw([edit(row, imm=z25, **{"in": one})]), b"a row must index the concatenated rows of the input sets")
    refused(raw([edit(row, flags=1, expect=[0, 7] + [0] * 14)]), b"a row must index the concatenated rows of the input sets")
    refused(raw([edit(rnds, start=7)], opts=_native.DeriveOpts(T, None)), b"a row must index the concatenated rows of the input sets")
    refused(raw([edit(rnds, **{"in": [2, 3, 4, 5, 7] + [0] * 20})]), b"a row must index the concatenated rows of the input sets")
    big = R.to_bytes(32, "big")
    tl = b"".join(bt([random.Random(5).randrange(R) for _ in range(4 * 4)]))
    for usable, tail, text in ((T, tl, b"usable must be in [1, T - 1] (0: all T rows are read)"),
                               (T - 33, tl, b"at most KZG_MAX_BLIND_ROWS rows may lie at or behind row `usable`"),
                               (T - 4, None, b"tail_be32 must be given when usable > 0"),
                               (0, tl, b"tail_be32 must be null in the plain layout (usable = 0)"),
                               (T - 4, tl[:-32] + big, b"tail scalars must be canonical (< r)")):
        refused(raw([row, rnds], opts=_native.DeriveOpts(usable, tail)), text)
    assert raw([edit(row, flags=1, expect=[0, 1] + [0] * 14)], opts=_native.DeriveOpts(T - 4, None)) == 0   # a check needs no tail
    assert h.value == 0 and eng.rows_stats() == live
    fresh_ok()
    for bad, why in ((dict(units[0], mode="sponge"), "unknown mode"), (dict(units[0], out=[25]), "lane index"),
                     (dict(units[0], out=[1, 1]), "repeated"), (dict(units[1], period=124), "period P"),
                     (dict(units[1], rate=25), "rate"), (dict(units[1], expect=[0]), "expect belongs"),
                     (dict(units[0], **{"in": [7] * 25}), "concatenated rows"),
                     (dict(units[0], **{"in": [("imm", 1 << 64)] * 25}), "below 2^64"),
                     (dict(units[1], cols=["a0", "a0"]), "repeated"), (dict(units[1], cols=["x"]), "unknown column"),
                     (dict(units[1], cols=[]), "cols must hold"), (dict(units[0], foo=1), "unknown field")):
        arg_error(lambda: eng.commit_keccak(I, [bad]), why)
    arg_error(lambda: eng.commit_keccak(I, units, None, [be(1)]), "tail")
    arg_error(lambda: eng.commit_keccak([2 ** 40], units), "unknown")
    fresh_ok()
    release(I)
    assert eng.rows_stats() == (0, 0)
    arg_error(lambda: eng.commit_keccak([I[0].handle], units), "keccak: ")   # a released input handle


# ---------------------------------------------------------------------------------------------------- routing
def test_multi_handle_client_and_multi_device_client_return_the_engine_bytes(hip):
    from zkp_subnet_amd import Client, MultiDeviceClient, codec
    from zkp_subnet_amd.engine import lagrange_factor

    lib = _native.load()
    scale, ms = 8, 0
    T = 1 << scale
    tx, ty = 0x6EC4A6778, 0x13579BF9
    cols = lanes(7, T, random.Random(1500))
    cols[6] = [int(t == 125) for t in range(T)]
    units = [{"mode": "row", "in": [0, ["imm", 5], 1] + [0] * 13 + [["imm", M64]] * 9, "out": [1, 0]},
             {"mode": "rounds", "msg": [1, 2, 3, 4, 5], "rate": 17, "start": 6, "period": 125, "cols": ["a0", "b1", "t4"]}]
    plain = [dict(units[0], **{"in": [tuple(s) if isinstance(s, list) else s for s in units[0]["in"]]}), units[1]]
    u = T - 3
    tail = [random.Random(6).randrange(R) for _ in range(5 * (T - u))]
    # the kzg_multi_ twin on one device against the engine's call
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    recs = single.keccak_call(plain)
    ua = (_native.KeccakUnit * 2)(*[single.keccak_unit_struct(r) for r in recs])
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(1, (ctypes.c_int * 1)(0), ctypes.byref(mh)) == 0
    none = lambda vs: [None if v == _native.KZG_KECCAK_NONE else v for v in vs]   # noqa: E731
    try:
        s0 = lagrange_factor(0, ms, ty).to_bytes(32, "big")
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        I = commit_sets(single, cols, (7,))
        c, cc = ctypes.create_string_buffer(48 * 5), ctypes.create_string_buffer(48 * 7)
        hi, hz = ctypes.c_uint64(0), ctypes.c_uint64(0)
        assert lib.kzg_multi_rows_commit(mh, 0, 7, b"".join(row_bytes(r) for r in cols), T, 1, cc, ctypes.byref(hi)) == 0
        ai = (ctypes.c_uint64 * 1)(hi.value)
        made = [hi.value]
        st6 = [(ctypes.c_uint64 * 2)() for _ in range(6)]
        tb = b"".join(bt(tail))
        for opts, usable, tl in ((None, None, ()), (_native.DeriveOpts(u, tb), u, tail)):
            ref, rs = single.commit_keccak(I, plain, usable, bt(tl))
            want, stats = kr.columns(cols, plain, usable, tl)
            assert rs == stats and read_all(single, ref) == want
            assert lib.kzg_multi_rows_commit_keccak(mh, 0, 1, ai, 2, ua, ctypes.byref(opts) if opts else None, c, *st6,
                                                    ctypes.byref(hz)) == 0
            assert c.raw == b"".join(ref.commitments)
            assert {"perms": list(st6[0]), "messages": list(st6[1]), "counts": list(st6[2]), "first": none(st6[3]),
                    "mismatch": list(st6[4]), "first_mismatch": none(st6[5])} == rs
            made.append(hz.value)
            ref.release()
        for hh in made:
            assert lib.kzg_multi_rows_release(mh, 0, hh) == 0
        release(I)
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)

    # the text clients over the engine: the same bytes as a commit of the reference rows
    want, stats = kr.columns(cols, plain)
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    for client in (Client(seed=84), MultiDeviceClient(devices=[0], seed=84)):
        client.start(scale=scale, machines_scale=ms)
        try:
            a = client.worker_commit_rows(0, [fr(col) for col in cols]).json()["handle"]
            ref = client.worker_commit_rows(0, [fr(col) for col in want]).json()
            r = client.worker_commit_keccak([a], units)
            assert r.status_code == 200, r.json()
            body = r.json()
            assert body["commitments"] == ref["commitments"]
            assert {k: body[k] for k in stats} == stats
            chk = client.worker_commit_keccak([a, ref["handle"]], [dict(units[0], expect=[7, 8]), dict(units[0], expect=[8, 7])])
            assert chk.status_code == 200, chk.json()
            assert chk.json()["handle"] is None and chk.json()["commitments"] == []
            assert chk.json()["mismatch"][0] == 0 and chk.json()["first_mismatch"] == [None, 0]
            assert client.worker_commit_keccak([a], [dict(units[0], mode="sponge")]).status_code == 400
            assert client.worker_commit_keccak([a], [dict(units[1], period=124)]).status_code == 400
            assert client.worker_commit_keccak([a], [dict(units[0], **{"in": [["imm", 1 << 64]] * 25})]).status_code == 400
            assert client.worker_commit_keccak([a], units, None, fr([1])).status_code == 400
            for hh in (ref["handle"], body["handle"], a):
                assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_keccak([a], units).status_code == 400
        finally:
            client.stop()
