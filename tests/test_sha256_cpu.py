"""kzg_rows_commit_sha256 without a GPU.  The reference in Python integers (tests/sha256_ref.py) is pinned twice over: against
hashlib.sha256 (padding done here, blocks chained through the round trace and through the row layout) and against the gate
identities of the chip, written here independently of the generator: for every row, left side = right side + carry 2^32 with
the carry column.  Then the carry bounds, the zero cells, the continuation of a message over blocks, every refusal the Python
layer makes, and the header's constants against _native.py."""
import ctypes
import hashlib
import os
import random
import re

import pytest

from tests import sha256_ref as sr
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import HipEngine

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kzg_mi355x.h")
MESSAGES = [b"", b"a", b"abc"] + [bytes((7 * k + n) % 256 for k in range(n)) for n in (55, 56, 63, 64, 119, 120)]
M32 = 0xffffffff


def trace_of(messages, P, T=None, iv=None):
    """the msg and start columns of the padded messages one after another in blocks of P rows, and the twelve trace columns"""
    blocks = [(blk, k == 0) for m in messages for k, blk in enumerate(sr.pad(m))]
    T = T or len(blocks) * P
    msg, start = [0] * T, [0] * T
    for b, (blk, first) in enumerate(blocks):
        start[b * P] = int(first)
        msg[b * P + 4:b * P + 20] = blk
    unit = {"mode": "rounds", "msg": 0, "start": 1, "period": P, "iv": iv, "cols": list(sr.NAMES)}
    cols, n_blocks, n_messages, seen = sr.rounds_unit([msg, start], unit, T)
    assert (n_blocks, n_messages, seen.count) == (T // P, len(messages), 0)
    return dict(zip(sr.NAMES, cols)), blocks


# ---------------------------------------------------------------------------------------------------- against hashlib
@pytest.mark.parametrize("P", [72, 73, 128])
def test_chained_blocks_of_the_round_trace_give_hashlib_digests(P):
    col, blocks = trace_of(MESSAGES, P)
    b = 0
    for m in MESSAGES:
        b += len(sr.pad(m))
        q = (b - 1) * P
        H = [col["a"][q + 71], col["a"][q + 70], col["a"][q + 69], col["a"][q + 68], col["e"][q + 71], col["e"][q + 70],
             col["e"][q + 69], col["e"][q + 68]]
        assert sr.digest_bytes(H) == hashlib.sha256(m).digest(), len(m)


@pytest.mark.parametrize("m", MESSAGES, ids=lambda m: str(len(m)))
def test_the_row_layout_chained_by_hand_gives_hashlib_digests(m):
    H = list(sr.IV)
    for blk in sr.pad(m):
        cols = [[w] for w in H + blk]
        out, seen = sr.row_unit(cols, {"mode": "row", "state": list(range(8)), "msg": list(range(8, 24)), "out": list(range(8))}, 1)
        H = [c[0] for c in out]
        assert seen.count == 0
    assert sr.digest_bytes(H) == hashlib.sha256(m).digest()
    assert len(sr.pad(m)) == (len(m) + 8) // 64 + 1


def test_abc_known_answer_and_the_sha224_initial_value():
    assert sr.digest_bytes(sr.compress(sr.IV, sr.pad(b"abc")[0])).hex() == \
        "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
    for m in (b"", b"abc", bytes(100)):
        H = list(sr.IV224)
        for blk in sr.pad(m):
            H = sr.compress(H, blk)
        assert sr.digest_bytes(H)[:28] == hashlib.sha224(m).digest()


def test_a_merkle_node_is_two_row_calls():
    rnd = random.Random(5)
    left, right = rnd.randbytes(32), rnd.randbytes(32)
    words = [int.from_bytes((left + right)[4 * j:4 * j + 4], "big") for j in range(16)]
    first, _ = sr.row_unit([[w] for w in words], {"mode": "row", "state": "iv", "msg": list(range(16)), "out": list(range(8))}, 1)
    padding = sr.pad(left + right)[1]
    second, _ = sr.row_unit(first, {"mode": "row", "state": list(range(8)), "msg": [("imm", w) for w in padding],
                                    "out": list(range(8))}, 1)
    assert sr.digest_bytes([c[0] for c in second]) == hashlib.sha256(left + right).digest()


# ---------------------------------------------------------------------------------------------------- the gates
def rotr(x, k):
    return ((x >> k) | (x << (32 - k))) % (1 << 32)


@pytest.mark.parametrize("P", [72, 75])
def test_gate_identities_hold_on_every_row_with_the_carry_columns(P):
    """written from the chip's description, not from the generator: selectors by the row's place in its block"""
    rnd = random.Random(9)
    col, blocks = trace_of(MESSAGES + [rnd.randbytes(200), bytes([255]) * 64], P)
    W, A, E = col["w"], col["a"], col["e"]
    top = {"cw": 0, "ca": 0, "ce": 0}
    for b, (blk, first) in enumerate(blocks):
        o = b * P
        for q in range(o + 4, o + 68):
            t = q - o - 4
            if t < 16:
                assert W[q] == blk[t] and (col["cw"][q], col["sig0"][q], col["sig1"][q]) == (0, 0, 0)
            else:
                x, y = W[q - 15], W[q - 2]
                assert col["sig0"][q] == rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3) and col["sig1"][q] == rotr(y, 17) ^ rotr(y, 19) ^ (y >> 10)
                assert col["sig1"][q] + W[q - 7] + col["sig0"][q] + W[q - 16] == W[q] + (col["cw"][q] << 32)
            a, bb, c, d = A[q - 1], A[q - 2], A[q - 3], A[q - 4]
            e, f, g, h = E[q - 1], E[q - 2], E[q - 3], E[q - 4]
            assert col["sum0"][q] == rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22) and col["sum1"][q] == rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)
            assert col["maj"][q] == (a & bb) | (a & c) | (bb & c) and col["ch"][q] == (e & f) | ((e ^ M32) & g)
            t1 = h + col["sum1"][q] + col["ch"][q] + sr.K[t] + W[q]
            assert t1 + col["sum0"][q] + col["maj"][q] == A[q] + (col["ca"][q] << 32)
            assert d + t1 == E[q] + (col["ce"][q] << 32)
        for j in range(4):
            assert A[o + j] + A[o + 64 + j] == A[o + 68 + j] + (col["ca"][o + 68 + j] << 32)
            assert E[o + j] + E[o + 64 + j] == E[o + 68 + j] + (col["ce"][o + 68 + j] << 32)
            assert col["ca"][o + 68 + j] <= 1 and col["ce"][o + 68 + j] <= 1
        H = sr.IV if first else [A[o - P + 71 - i] for i in range(4)] + [E[o - P + 71 - i] for i in range(4)]
        assert [A[o + j] for j in range(4)] == [H[3 - j] for j in range(4)] and [E[o + j] for j in range(4)] == [H[7 - j] for j in range(4)]
        if not first:   # a continuing block's rows 0 .. 3 repeat rows 68 .. 71 of the block before
            assert A[o:o + 4] == A[o - P + 68:o - P + 72] and E[o:o + 4] == E[o - P + 68:o - P + 72]
        # zero cells where a column is undefined
        for name in sr.NAMES:
            assert not any(col[name][o + 72:o + P]), name
            if name not in ("a", "e"):
                assert not any(col[name][o:o + 4]), name
            if name not in ("a", "e", "ca", "ce"):
                assert not any(col[name][o + 68:o + 72]), name
        for name in top:
            top[name] = max(top[name], max(col[name][o:o + 72]))
    assert all(0 <= v <= M32 for name in sr.NAMES for v in col[name])
    assert top["cw"] <= 3 and top["ca"] <= 6 and top["ce"] <= 5 and top["cw"] >= 2 and top["ca"] >= 3 and top["ce"] >= 3, top


def test_carry_bounds_are_reached_by_their_sums_only():
    """four words below 2^32 carry at most 3, seven at most 6, six at most 5"""
    for terms, bound in ((4, 3), (7, 6), (6, 5)):
        assert (terms * M32) >> 32 == bound


def test_tail_rows_and_a_block_cut_by_n_are_zero():
    msg, start = [0] * 256, [0] * 256
    msg[4:20] = sr.pad(b"abc")[0]
    unit = {"mode": "rounds", "msg": 0, "start": None, "period": 72, "iv": None, "cols": ["a", "w"]}
    got, blocks, messages, _ = sr.rounds_unit([msg, start], unit, 200)
    assert (blocks, messages) == (2, 2) and not any(got[0][144:]) and not any(got[1][144:])
    got, blocks, messages, _ = sr.rounds_unit([msg, start], unit, 64)
    assert (blocks, messages) == (0, 0) and got == [[0] * 256] * 2
    want, st = sr.columns([msg, start], [unit], 200, list(range(1, 2 * 56 + 1)))
    assert want[0][200:] == list(range(1, 57)) and want[1][200:] == list(range(57, 113)) and st["blocks"] == [2]


def test_over_range_cells_are_reduced_and_counted_once_per_cell():
    R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
    cols = [[5, 1 << 32, (1 << 32) + 3, R - 1] for _ in range(2)]
    unit = {"mode": "row", "state": "iv", "msg": [0] * 15 + [1], "out": [0]}
    want, st = sr.columns(cols, [unit])
    assert (st["counts"], st["first"], st["blocks"], st["messages"]) == ([6], [1], [4], [0])
    assert want[0][1] == sr.compress(sr.IV, [0] * 16)[0] and want[0][3] == sr.compress(sr.IV, [(R - 1) & M32] * 16)[0]
    msg = [1 << 32] * 144
    start = [0] * 144
    start[72], start[73] = (1 << 32) + 1, 1 << 40   # (R - 1 ends in 32 zero bits: it would start nothing)
    rows, st = sr.columns([msg, start], [{"mode": "rounds", "msg": 0, "start": 1, "period": 72, "iv": None, "cols": ["w"]}])
    assert (st["counts"], st["first"], st["messages"]) == ([33], [4], [2])   # 2 x 16 message cells and one start cell


# ---------------------------------------------------------------------------------------------------- the encoder
ROW = {"mode": "row", "state": "iv", "msg": list(range(16)), "out": [0]}
RND = {"mode": "rounds", "msg": 0, "start": 1, "period": 72, "iv": None, "cols": ["w", "a", "e"]}


def test_the_encoder_fills_the_struct_fields():
    recs = HipEngine.sha256_call([dict(ROW, state=[("imm", 7)] + list(range(1, 8)), out=[7, 0], expect=[3, 4]),
                                  dict(RND, start=None, iv=sr.IV224, cols=["ch", "w"])])
    IMM = _native.KZG_SHA256_IMM
    assert recs[0] == (_native.KZG_SHA256_ROW, _native.KZG_SHA256_CHECK, 2, 0, _native.KZG_SHA256_ABSENT, [IMM] + list(range(1, 8)),
                       [7] + [0] * 7, list(range(16)), [0] * 16, [7, 0] + [0] * 10, [3, 4] + [0] * 6)
    assert recs[1] == (_native.KZG_SHA256_ROUNDS, 0, 2, 72, _native.KZG_SHA256_ABSENT, [IMM] * 8, sr.IV224, [0] * 16, [0] * 16,
                       [11, 0] + [0] * 10, [0] * 8)
    assert HipEngine.sha256_call([ROW])[0][1] == _native.KZG_SHA256_STD_IV and HipEngine.sha256_call([RND])[0][4] == 1
    u = HipEngine.sha256_unit_struct(recs[0])
    assert (u.mode, u.flags, u.n_out, u.state[0], u.state_imm[0], u.msg[15], u.out[0], u.expect[1]) == (1, 1, 2, IMM, 7, 15, 7, 4)
    assert ctypes.sizeof(_native.Sha256Unit) == 4 * (5 + 8 + 8 + 16 + 16 + 12 + 8)


@pytest.mark.parametrize("units,why", [
    ([], "n_units"), ([ROW] * 5, "n_units"), ("x", "n_units"), ([5], "a unit is a mapping"),
    ([dict(ROW, mode="sponge")], "unknown mode"), ([dict(ROW, foo=1)], "unknown field"), ([dict(ROW, period=72)], "unknown field"),
    ([dict(ROW, state=[0] * 7)], "state"), ([dict(ROW, state="IV")], "state"), ([dict(ROW, msg=[0] * 15)], "msg must hold 16"),
    ([dict(ROW, msg=[0] * 15 + [-1])], "a slot must be"), ([dict(ROW, msg=[0] * 15 + [("im", 1)])], "immediate is"),
    ([dict(ROW, msg=[0] * 15 + [("imm", 1 << 32)])], "below 2^32"), ([dict(ROW, msg=[0] * 15 + [("imm", -1)])], "below 2^32"),
    ([dict(ROW, out=[])], "out must hold"), ([dict(ROW, out=list(range(8)) + [0])], "out must hold"),
    ([dict(ROW, out=[8])], "out index must be"), ([dict(ROW, out=[1, 1])], "repeated"),
    ([dict(ROW, expect=[1, 2])], "one row per entry"), ([dict(ROW, expect=["a"])], "entry of expect"),
    ([dict(RND, expect=[0])], "expect belongs to row units"), ([dict(RND, period=71)], "period P"),
    ([dict(RND, period=None)], "period P"), ([dict(RND, period=1 << 32)], "period P"), ([dict(RND, msg=("imm", 1))], "msg of a rounds unit"),
    ([dict(RND, start="x")], "start must be"), ([dict(RND, iv=[0] * 7)], "iv must be"), ([dict(RND, iv=[1 << 32] + [0] * 7)], "iv must be"),
    ([dict(RND, cols=[])], "cols must hold"), ([dict(RND, cols=["w", "x"])], "unknown column name"),
    ([dict(RND, cols=["w", "a", "w"])], "column name is repeated"),
    ([dict(ROW, out=list(range(8)))] * 2 + [dict(RND, cols=["w"])], "n_out"),
    ([ROW, dict(ROW, msg=[16] + list(range(1, 16)))], "distinct input rows"),
    ([dict(ROW, out=list(range(8)))] * 2, None),
])
def test_python_refusals(units, why):
    if why is None:   # sixteen output rows and sixteen distinct input rows fit
        assert len(HipEngine.sha256_call(units)) == 2
        return
    with pytest.raises(KzgError) as ei:
        HipEngine.sha256_call(units)
    assert ei.value.code == _native.KZG_E_ARG and "sha256: " in str(ei.value) and why in str(ei.value), str(ei.value)


def test_header_constants_and_symbols():
    text = open(HEADER).read()
    for name in ("KZG_SHA256_ROW", "KZG_SHA256_ROUNDS", "KZG_SHA256_CHECK", "KZG_SHA256_STD_IV", "KZG_SHA256_IMM", "KZG_SHA256_ABSENT",
                 "KZG_SHA256_NONE", "KZG_SHA256_MAX_UNITS", "KZG_SHA256_MIN_PERIOD", "KZG_SHA256_N_COLS"):
        m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, text)
        assert m and int(m.group(1), 0) == getattr(_native, name), name
    for k, name in enumerate(_native.KZG_SHA256_COLS):
        m = re.search(r"#define\s+KZG_SHA256_COL_%s\s+(\d+)" % name.upper(), text)
        assert m and int(m.group(1)) == k, name
    assert _native.KZG_SHA256_COLS == sr.NAMES and _native.KZG_SHA256_MIN_PERIOD == sr.MIN_PERIOD
    for sym in ("kzg_rows_commit_sha256", "kzg_multi_rows_commit_sha256"):
        assert sym in _native.SYMBOLS and re.search(r"\bint %s\(" % sym, text)
    assert len(_native.SYMBOLS["kzg_multi_rows_commit_sha256"][1]) == len(_native.SYMBOLS["kzg_rows_commit_sha256"][1]) + 1
    for word in ("padding, and packing bytes into words", "bit columns", "SHA-512, Keccak, Blake", "periods below 72",
                 "more than one start convention", "nothing here is a proof"):
        assert word in text, word
    from zkp_subnet_amd import Client, MultiDeviceClient
    assert callable(Client.worker_commit_sha256) and callable(MultiDeviceClient.worker_commit_sha256)
    assert callable(HipEngine.commit_sha256)
