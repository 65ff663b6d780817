"""kzg_rows_commit_keccak without a GPU.  The reference in Python integers (tests/keccak_ref.py) is pinned twice over: against
hashlib's SHA-3 and SHAKE (padding done by the reference's helper, blocks chained through the round trace and through the row
layout), which fixes the 24 round constants and the 25 rotation offsets, and against the trace identities of the chip, written
here independently of the generator.  Then the zero cells, the continuation of a message over blocks, every refusal the Python
layer makes, the struct layout and the header's constants against _native.py, and the compiler's resource report of the
kernel."""
import ctypes
import hashlib
import os
import random
import re

import pytest

from tests import keccak_ref as kr
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import HipEngine

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kzg_mi355x.h")
M64 = (1 << 64) - 1
EMPTY_KECCAK256 = "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
# (rate in lanes, domain suffix, digest bytes, hashlib's function): one-block and multi-block messages whose lengths straddle
# the rate of each
HASHES = [(17, 0x06, 32, lambda m: hashlib.sha3_256(m).digest()), (9, 0x06, 64, lambda m: hashlib.sha3_512(m).digest()),
          (21, 0x1f, 32, lambda m: hashlib.shake_128(m).digest(32))]
LENGTHS = (0, 1, 71, 72, 73, 135, 136, 137, 167, 168, 169, 300)
message = lambda n: bytes((7 * k + n) % 256 for k in range(n))   # noqa: E731


def trace_of(messages, rate, suffix, P, T=None):
    """the five msg columns and the start column of the padded messages one after another in blocks of P rows, the 25 trace
    columns, and the blocks as (lanes, first)"""
    blocks = [(blk, k == 0) for m in messages for k, blk in enumerate(kr.pad(m, rate, suffix))]
    T = T or len(blocks) * P
    cols = [[0] * T for _ in range(6)]
    for b, (blk, first) in enumerate(blocks):
        cols[5][b * P] = int(first)
        for i, v in enumerate(blk):
            cols[i % 5][b * P + i // 5] = v
    unit = {"mode": "rounds", "msg": [0, 1, 2, 3, 4], "rate": rate, "start": 5, "period": P, "cols": list(kr.NAMES)}
    got, n_blocks, n_messages, seen = kr.rounds_unit(cols, unit, T)
    assert (n_blocks, n_messages, seen.count) == (T // P, len(messages), 0)
    return dict(zip(kr.NAMES, got)), blocks


def outgoing(col, q):
    """the outgoing state of the block at row q from the a columns"""
    return [col[f"a{x}"][q + 120 + y] for y in range(5) for x in range(5)]


# ---------------------------------------------------------------------------------------------------- against hashlib
@pytest.mark.parametrize("rate,suffix,nbytes,ref", HASHES, ids=["sha3_256", "sha3_512", "shake_128"])
def test_the_sponge_over_permute_gives_hashlib_digests(rate, suffix, nbytes, ref):
    for n in LENGTHS:
        m = message(n)
        assert kr.sponge(m, rate, suffix, nbytes) == ref(m), n
        assert len(kr.pad(m, rate, suffix)) == n // (8 * rate) + 1


def test_permute_is_the_round_trace_without_its_columns():
    rnd = random.Random(3)
    for _ in range(5):
        A = [rnd.randrange(1 << 64) for _ in range(25)]
        S = list(A)
        for q in range(24):
            S = kr.round_trace(S, q)[1]
        assert kr.permute(A) == S == kr.block_trace(A)[1]


def test_keccak256_of_the_empty_message():
    assert kr.sponge(b"", 17, 0x01, 32).hex() == EMPTY_KECCAK256
    assert kr.pad(b"", 17, 0x01) == [[1] + [0] * 15 + [1 << 63]]


@pytest.mark.parametrize("P", [125, 128])
@pytest.mark.parametrize("rate,suffix,nbytes,ref", HASHES, ids=["sha3_256", "sha3_512", "shake_128"])
def test_chained_blocks_of_the_round_trace_give_hashlib_digests(rate, suffix, nbytes, ref, P):
    messages = [message(n) for n in (0, 135, 136, 137, 72, 300)]
    col, _ = trace_of(messages, rate, suffix, P)
    b = 0
    for m in messages:
        b += len(kr.pad(m, rate, suffix))
        assert kr.digest_bytes(outgoing(col, (b - 1) * P), nbytes) == ref(m), len(m)


def test_the_row_layout_gives_the_keccak256_of_a_merkle_node():
    """two 32-byte nodes: 8 rows, the immediate 0x01 in lane 8, 2^63 in lane 16, zeros in the capacity"""
    rnd = random.Random(5)
    node = rnd.randbytes(64)
    cols = [[int.from_bytes(node[8 * j:8 * j + 8], "little")] for j in range(8)]
    unit = {"mode": "row", "in": list(range(8)) + [("imm", 1)] + [("imm", 0)] * 7 + [("imm", 1 << 63)] + [("imm", 0)] * 8, "out": [0, 1, 2, 3]}
    out, seen = kr.row_unit(cols, unit, 1)
    assert kr.digest_bytes([c[0] for c in out], 32) == kr.sponge(node, 17, 0x01, 32) and seen.count == 0
    # SHA3-256 of the same node differs by the suffix only, and hashlib knows it
    out, _ = kr.row_unit(cols, dict(unit, **{"in": unit["in"][:8] + [("imm", 6)] + unit["in"][9:]}), 1)
    assert kr.digest_bytes([c[0] for c in out], 32) == hashlib.sha3_256(node).digest()


# ---------------------------------------------------------------------------------------------------- the trace identities
def rotl(v, k):
    return ((v << k) | (v >> (64 - k))) % (1 << 64) if k % 64 else v


@pytest.mark.parametrize("P,rate", [(125, 17), (131, 9), (125, 24)])
def test_trace_identities_hold_on_every_row(P, rate):
    """written from the chip's description, not from the generator: rows by their place in the block"""
    rnd = random.Random(9 + P)
    col, blocks = trace_of([rnd.randbytes(n) for n in (0, 8 * rate - 1, 8 * rate, 20 * rate + 3)], rate, 0x06, P)
    a = [col[f"a{x}"] for x in range(5)]
    p = [col[f"p{x}"] for x in range(5)]
    d = [col[f"d{x}"] for x in range(5)]
    t = [col[f"t{x}"] for x in range(5)]
    bb = [col[f"b{x}"] for x in range(5)]
    for k, (blk, first) in enumerate(blocks):
        o = k * P
        for q in range(24):
            r0 = o + 5 * q
            for x in range(5):
                acc = 0
                for y in range(5):   # p is a running XOR, and C at y = 4
                    acc ^= a[x][r0 + y]
                    assert p[x][r0 + y] == acc
            C = [p[x][r0 + 4] for x in range(5)]
            for x in range(5):
                for y in range(5):
                    assert d[x][r0 + y] == C[(x - 1) % 5] ^ rotl(C[(x + 1) % 5], 1)
                    assert t[x][r0 + y] == rotl(a[x][r0 + y] ^ d[x][r0 + y], kr.ROT[x][y])
                    assert bb[y][r0 + (2 * x + 3 * y) % 5] == t[x][r0 + y]   # b is the pi permutation of t
            for x in range(5):
                for y in range(5):   # chi and iota are row-local
                    want = bb[x][r0 + y] ^ ((bb[(x + 1) % 5][r0 + y] ^ M64) & bb[(x + 2) % 5][r0 + y])
                    assert a[x][r0 + y + 5] == want ^ (kr.RC[q] if x == y == 0 else 0)
        # the absorbed state: the incoming one XOR the message lanes below the rate
        S = [0] * 25 if first else outgoing(col, o - P)
        for i in range(25):
            assert a[i % 5][o + i // 5] == S[i] ^ (blk[i] if i < rate else 0)
        # zero cells: p, d, t, b on rows 120 .. 124, everything behind
        for name in kr.NAMES:
            assert not any(col[name][o + 125:o + P]), name
            if name[0] != "a":
                assert not any(col[name][o + 120:o + 125]), name
    assert all(0 <= v <= M64 for name in kr.NAMES for v in col[name])


def test_tail_rows_and_a_block_cut_by_n_are_zero():
    cols = [[random.Random(j).randrange(1 << 64) for _ in range(256)] for j in range(5)]
    unit = {"mode": "rounds", "msg": [0, 1, 2, 3, 4], "rate": 17, "start": None, "period": 125, "cols": ["a0", "t3"]}
    got, blocks, messages, _ = kr.rounds_unit(cols, unit, 256)
    assert (blocks, messages) == (2, 2) and not any(got[0][250:]) and not any(got[1][250:]) and any(got[1][125:245])
    got, blocks, messages, _ = kr.rounds_unit(cols, unit, 249)
    assert (blocks, messages) == (1, 1) and not any(got[0][125:]) and not any(got[1][125:])
    got, blocks, messages, _ = kr.rounds_unit(cols, unit, 64)
    assert (blocks, messages) == (0, 0) and got == [[0] * 256] * 2
    want, st = kr.columns(cols, [unit], 249, list(range(1, 15)))
    assert want[0][249:] == list(range(1, 8)) and want[1][249:] == list(range(8, 15)) and st["perms"] == [1]


def test_over_range_cells_are_reduced_and_counted_once_per_cell():
    R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
    cols = [[5, 1 << 64, (1 << 64) + 3, R - 1] for _ in range(2)]
    unit = {"mode": "row", "in": [0] * 15 + [1] + [("imm", 0)] * 9, "out": [0]}
    want, st = kr.columns(cols, [unit])
    assert (st["counts"], st["first"], st["perms"], st["messages"]) == ([6], [1], [4], [0])
    assert want[0][1] == kr.permute([0] * 25)[0] and want[0][3] == kr.permute([(R - 1) & M64] * 16 + [0] * 9)[0]
    # a rounds unit: the cells of lanes below the rate only; the start column among the message rows is one cell, counted once
    msg = [[1 << 64] * 250 for _ in range(5)]
    msg[0][125], msg[0][126] = (1 << 64) + 1, 1 << 70
    unit = {"mode": "rounds", "msg": [0, 1, 2, 3, 4], "rate": 7, "start": 0, "period": 125, "cols": ["a0"]}
    rows, st = kr.columns(msg, [unit])
    assert (st["counts"], st["first"], st["messages"]) == ([14], [0], [2])
    assert rows[0][125] == 1 and rows[0][0] == 0


# ---------------------------------------------------------------------------------------------------- the encoder
ROW = {"mode": "row", "in": list(range(16)) + [("imm", j) for j in range(9)], "out": [0]}
RND = {"mode": "rounds", "msg": [0, 1, 2, 3, 4], "rate": 17, "start": 5, "period": 125, "cols": ["a0", "p1", "b4"]}


def test_the_encoder_fills_the_struct_fields():
    recs = HipEngine.keccak_call([dict(ROW, **{"in": [("imm", M64)] + list(range(1, 25))[:15] + [("imm", 0)] * 9}, out=[24, 0], expect=[3, 4]),
                                  dict(RND, start=None, rate=9, cols=["b4", "a0"])])
    IMM = _native.KZG_KECCAK_IMM
    assert recs[0] == (_native.KZG_KECCAK_ROW, _native.KZG_KECCAK_CHECK, 2, 0, 0, _native.KZG_KECCAK_ABSENT, [M64] + [0] * 24,
                       [IMM] + list(range(1, 16)) + [IMM] * 9, [24, 0] + [0] * 14, [3, 4] + [0] * 14)
    assert recs[1] == (_native.KZG_KECCAK_ROUNDS, 0, 2, 125, 9, _native.KZG_KECCAK_ABSENT, [0] * 25, [0, 1, 2, 3, 4] + [0] * 20,
                       [24, 0] + [0] * 14, [0] * 16)
    assert HipEngine.keccak_call([RND])[0][5] == 5 and HipEngine.keccak_call([RND])[0][8][:3] == [0, 6, 24]
    u = HipEngine.keccak_unit_struct(recs[0])
    assert (u.mode, u.flags, u.n_out, u.period, u.rate, u.start) == (1, 1, 2, 0, 0, IMM)
    assert (u.imm[0], u.in_[0], u.in_[15], u.in_[24], u.out[0], u.expect[1]) == (M64, IMM, 15, IMM, 24, 4)


@pytest.mark.parametrize("units,why", [
    ([], "n_units"), ([ROW] * 5, "n_units"), ("x", "n_units"), ([5], "a unit is a mapping"),
    ([dict(ROW, mode="sponge")], "unknown mode"), ([dict(ROW, foo=1)], "unknown field"), ([dict(ROW, period=125)], "unknown field"),
    ([dict(ROW, rate=17)], "unknown field"), ([dict(RND, **{"in": [0] * 25})], "unknown field"),
    ([dict(ROW, **{"in": [0] * 24})], "in must hold 25"), ([dict(ROW, **{"in": "x"})], "in must hold 25"),
    ([dict(ROW, **{"in": [0] * 24 + [-1]})], "a slot must be"), ([dict(ROW, **{"in": [0] * 24 + [("im", 1)]})], "immediate is"),
    ([dict(ROW, **{"in": [0] * 24 + [("imm", 1 << 64)]})], "below 2^64"), ([dict(ROW, **{"in": [0] * 24 + [("imm", -1)]})], "below 2^64"),
    ([dict(ROW, out=[])], "out must hold"), ([dict(ROW, out=list(range(17)))], "out must hold"),
    ([dict(ROW, out=[25])], "lane index must be"), ([dict(ROW, out=[1, 1])], "repeated"),
    ([dict(ROW, expect=[1, 2])], "one row per entry"), ([dict(ROW, expect=["a"])], "entry of expect"),
    ([dict(RND, expect=[0])], "expect belongs to row units"), ([dict(RND, period=124)], "period P"),
    ([dict(RND, period=None)], "period P"), ([dict(RND, period=1 << 32)], "period P"),
    ([dict(RND, rate=0)], "rate"), ([dict(RND, rate=25)], "rate"), ([dict(RND, rate=None)], "rate"),
    ([dict(RND, msg=[0, 1, 2, 3])], "msg of a rounds unit"), ([dict(RND, msg=[0, 1, 2, 3, ("imm", 1)])], "msg of a rounds unit"),
    ([dict(RND, msg=0)], "msg of a rounds unit"), ([dict(RND, start="x")], "start must be"),
    ([dict(RND, cols=[])], "cols must hold"), ([dict(RND, cols=list(kr.NAMES[:17]))], "cols must hold"),
    ([dict(RND, cols=["a0", "x"])], "unknown column name"), ([dict(RND, cols=["a0", "a5"])], "unknown column name"),
    ([dict(RND, cols=["a0", "p0", "a0"])], "column name is repeated"),
    ([dict(ROW, out=list(range(16))), dict(RND, cols=["a0"])], "n_out"),
    ([ROW, dict(ROW, **{"in": [16] + ROW["in"][1:]})], "distinct input rows"),
    ([ROW, dict(ROW, expect=[16])], "distinct input rows"),
    ([dict(ROW, out=list(range(16)))], None),
])
def test_python_refusals(units, why):
    if why is None:   # sixteen output rows and sixteen distinct input rows fit
        assert len(HipEngine.keccak_call(units)) == 1
        return
    with pytest.raises(KzgError) as ei:
        HipEngine.keccak_call(units)
    assert ei.value.code == _native.KZG_E_ARG and "keccak: " in str(ei.value) and why in str(ei.value), str(ei.value)


# ---------------------------------------------------------------------------------------------------- the header
def test_struct_layout_against_the_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct kzg_keccak_unit \{(.*?)\} kzg_keccak_unit;", text, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|uint64_t)\s+(\w+)(?:\[(\d+)\])?;", body, re.M)
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    want = [(name, ctype[ty], int(k) if k else 1) for ty, name, k in fields]
    is_array = lambda ty: issubclass(ty, ctypes.Array)   # noqa: E731
    got = [(name.rstrip("_"), ty._type_ if is_array(ty) else ty, ty._length_ if is_array(ty) else 1)
           for name, ty in _native.KeccakUnit._fields_]
    assert got == want and len(want) == 10

    class InC(ctypes.Structure):   # the header's fields laid out by the C rules
        _fields_ = [(name, ty * k if k > 1 else ty) for name, ty, k in want]

    assert ctypes.sizeof(_native.KeccakUnit) == ctypes.sizeof(InC) == 456
    for name, _ in _native.KeccakUnit._fields_:
        assert getattr(_native.KeccakUnit, name).offset == getattr(InC, name.rstrip("_")).offset, name
    assert _native.KeccakUnit.imm.offset == 24 and _native.KeccakUnit.in_.offset == 224


def test_header_constants_and_symbols():
    text = open(HEADER).read()
    for name in ("KZG_KECCAK_ROW", "KZG_KECCAK_ROUNDS", "KZG_KECCAK_CHECK", "KZG_KECCAK_IMM", "KZG_KECCAK_ABSENT", "KZG_KECCAK_NONE",
                 "KZG_KECCAK_MAX_UNITS", "KZG_KECCAK_MIN_PERIOD", "KZG_KECCAK_MAX_OUT", "KZG_KECCAK_N_COLS"):
        m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, text)
        assert m and int(m.group(1), 0) == getattr(_native, name), name
    for k, kind in enumerate("apdtb"):
        m = re.search(r"#define\s+KZG_KECCAK_COL_%s\s+(\d+)" % kind.upper(), text)
        assert m and int(m.group(1)) == 5 * k and _native.KZG_KECCAK_COLS[5 * k:5 * k + 5] == tuple(f"{kind}{x}" for x in range(5))
    assert _native.KZG_KECCAK_COLS == kr.NAMES and _native.KZG_KECCAK_MIN_PERIOD == kr.MIN_PERIOD
    for sym in ("kzg_rows_commit_keccak", "kzg_multi_rows_commit_keccak"):
        assert sym in _native.SYMBOLS and re.search(r"\bint %s\(" % sym, text)
    assert len(_native.SYMBOLS["kzg_multi_rows_commit_keccak"][1]) == len(_native.SYMBOLS["kzg_rows_commit_keccak"][1]) + 1
    for word in ("padding and byte packing", "bit columns", "Keccak-f[800]", "squeezing more than one block", "typed inputs",
                 "nothing here is a proof", "has its own call, kzg_rows_commit_keccak"):
        assert word in text, word
    from zkp_subnet_amd import Client, MultiDeviceClient
    assert callable(Client.worker_commit_keccak) and callable(MultiDeviceClient.worker_commit_keccak)
    assert callable(HipEngine.commit_keccak)


def test_the_kernel_tables_are_the_generated_constants():
    """csrc/fr_keccak.hip's RC and r[x][y] against the rules of FIPS 202 as tests/keccak_ref.py generates them (which the hashlib
    tests above pin)"""
    from zkp_subnet_amd import build as kb

    src = open(os.path.join(kb.CSRC, "fr_keccak.hip")).read()
    assert [int(x, 16) for x in re.findall(r"0x([0-9a-f]{16})ull", src)] == kr.RC
    rot = [int(x) for x in re.search(r"KEC_ROT\[25\] = \{([^}]*)\}", src).group(1).split(",")]
    assert rot == [kr.ROT[i % 5][i // 5] for i in range(25)]
    assert (kr.RC[0], kr.RC[1], kr.RC[23], kr.ROT[1][0], kr.ROT[0][1], kr.ROT[4][4]) == (1, 0x8082, 0x8000000080008008, 1, 36, 14)


# ---------------------------------------------------------------------------------------------------- the kernel's resources
def test_the_kernel_does_not_spill():
    """the compiler's report (-Rpass-analysis=kernel-resource-usage, gfx950): the 25 lanes of the state stay in registers"""
    from tests.test_lookup_sel_resources import report

    rep = {k: v for k, v in report("fr_keccak.hip").items() if "k_fr_keccak" in k}
    assert len(rep) == 1
    for name, r in rep.items():
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)
