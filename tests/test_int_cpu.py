"""CPU checks around kzg_rows_commit_int: the Python reference (tests/int_ref.py) against the gate identities a caller proves
the rows with, the counts and first rows of hand-made columns, the engine's op encoder and dispatch over a recording stub
library, the text client, and the header's declarations.  No device."""
import ctypes
import os
import random
import re

import pytest

from tests import int_ref as iref
from tests.gpu_common import R
from zkp_subnet_amd import _native
from zkp_subnet_amd.engine import HipEngine, RowSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 8
S = bytes(31) + b"\x01"
WIDTHS = [1, 8, 31, 32, 33, 63, 64]


def edges(w):
    M = 1 << w
    return [0, 1, M - 1, M, (1 << 64) - 1, 1 << 64, R - 1]


# ---------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("kind", iref.KINDS)
def test_the_reference_satisfies_the_gates_on_the_reduced_operands(kind, w):
    """every pair of edge operands (0, 1, M - 1, M, 2^64 - 1, 2^64, r - 1) and 200 random pairs, a third of them out of range:
    the identities hold on x mod M, y mod M, every output lies in its range, and `over` says exactly whether an operand did not"""
    M = 1 << w
    rnd = random.Random(1000 * w + iref.KINDS.index(kind))
    pairs = [(x, y) for x in edges(w) for y in edges(w)]
    pairs += [(rnd.randrange(M), rnd.randrange(M)) for _ in range(130)] + [(rnd.randrange(R), rnd.randrange(R)) for _ in range(70)]
    if kind == "split":
        pairs += [(x, s) for x in edges(w) for s in (0, 1, w - 1, w, w + 1)]
    for x, y in pairs:
        r0, r1, over = iref.cell(kind, w, x, y)
        a = x % M
        if kind == "split":
            s = min(y, w)
            assert over == (x >= M or y > w)
            assert a == r0 * (1 << s) + r1 and 0 <= r1 < 1 << s and 0 <= r0 < max(M >> s, 1)
            continue
        b = y % M
        assert over == (x >= M or y >= M), (x, y)
        assert 0 <= r0 < M
        if kind in ("and", "or", "xor"):
            assert r1 is None
            bits = [(((a >> j) & 1), ((b >> j) & 1), ((r0 >> j) & 1)) for j in range(w)]
            f = {"and": lambda p, q: p * q, "or": lambda p, q: p + q - p * q, "xor": lambda p, q: p + q - 2 * p * q}[kind]
            assert all(c == f(p, q) for p, q, c in bits)
        elif kind == "add":
            assert a + b == r0 + r1 * M and r1 in (0, 1)
        elif kind == "sub":
            assert a - b == r0 - r1 * M and r1 == int(a < b)
        elif kind == "mul":
            assert a * b == r0 + r1 * M and 0 <= r1 < M
        elif b:
            assert a == r0 * b + r1 and 0 <= r1 < b                      # rem < b: the borrow of the SUB rem - b is 1
            assert iref.cell("sub", w, r1, b)[1] == 1
        else:
            assert (r0, r1) == (M - 1, a)                                # the RISC-V convention


def test_counts_and_firsts_of_hand_made_columns():
    w, M = 8, 256
    a = [1, 2, M, 4, 5, 6, 7, R - 1]
    b = [0, M + 1, M, 3, 2, 1, 0, 9]
    s = [0, 8, 9, 1, 2, 3, 4, 1 << 64]
    ops = [("xor", w, 0, 1), ("add", w, 0, 1, 2), ("divmod", w, 1, 0, 2), ("split", w, 0, 2, 2), ("and", w, 1, ("imm", 15)),
           ("sub", w, 1, 1, 2), ("split", w, 1, ("imm", 8), 2), ("mul", w, 3, 3)]
    cols = [a, b, s, [3] * T]
    rows, counts, firsts = iref.int_columns(cols, ops)
    assert len(rows) == iref.n_out(ops) == 13 and all(len(r) == T for r in rows)
    # a is out of range at rows 2 and 7 (r - 1 ends in a zero byte), b at rows 1 and 2, s at rows 2 and 7: a row where both
    # operands are out of range is counted once
    assert counts == [3, 3, 3, 2, 2, 2, 2, 0]
    assert firsts == [1, 1, 1, 2, 1, 1, 1, None]
    lo_a, lo_b = [1, 2, 0, 4, 5, 6, 7, 0], [0, 1, 0, 3, 2, 1, 0, 9]
    assert rows[0] == [1, 3, 0, 7, 7, 7, 7, 9]                                # xor
    assert rows[1] == [1, 3, 0, 7, 7, 7, 7, 9] and rows[2] == [0] * T         # add: no carry anywhere
    assert rows[3] == [0, 0, M - 1, 0, 0, 0, 0, M - 1]                        # b / a: the divisor is 0 at rows 2 and 7
    assert rows[4] == [0, 1, 0, 3, 2, 1, 0, 9]                                # the remainder there is the dividend
    assert rows[5] == [1, 0, 0, 2, 1, 0, 0, 0]                                # a >> s; s = 9 and s = 2^64 are taken as w
    assert rows[6] == [0, 2, 0, 0, 1, 6, 7, 0]                                # a mod 2^s
    assert rows[7] == lo_b                                                    # and 15
    assert rows[8] == [0] * T and rows[9] == [0] * T                          # b - b, no borrow
    assert rows[10] == [0] * T and rows[11] == lo_b                           # split at s = w
    assert rows[12] == [9] * T
    assert [x % M for x in a] == lo_a
    # behind `usable` nothing is read or counted, and the tail lands column-major
    tail = list(range(100, 100 + 13 * 3))
    rows_u, counts_u, firsts_u = iref.int_columns(cols, ops, 5, tail)
    assert counts_u == [2, 2, 2, 1, 2, 2, 2, 0] and firsts_u == [1, 1, 1, 2, 1, 1, 1, None]
    for c in range(13):
        assert rows_u[c][:5] == rows[c][:5] and rows_u[c][5:] == tail[3 * c:3 * c + 3]
    assert iref.int_columns([[1, 2], [3, 0]], [("divmod", 4, 0, 1, 2)])[1:] == ([0], [None])   # a zero divisor is not counted


# ---------------------------------------------------------------------------------------------------- the dispatch
class _Recorder:
    """a library whose every attribute is a function that records its call and returns KZG_OK"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return _native.KZG_OK
        return fn


@pytest.fixture
def eng():
    e = HipEngine.__new__(HipEngine)
    e._lib, e._h, e._set_len, e.verifier = _Recorder(), ctypes.c_void_p(1), {}, None
    return e


def _sets(e, n, first=1):
    return [RowSet(e, first + j, 3, 1, T, [bytes(48)]) for j in range(n)]


def test_the_encoder_gives_the_struct_fields_and_n_out():
    ops = [("and", 8, 0, 1), ["or", 1, 1, 1, 1], ("xor", 64, 0, ("imm", (1 << 64) - 1)), ("add", 32, 0, 1, 2),
           ("sub", 33, 1, ["imm", 0], 2), ("mul", 64, 0, 0, 2), ("divmod", 31, 0, ("imm", 7)), ("split", 64, 1, ("imm", 64), 2),
           ("split", 8, 0, 1)]
    recs = HipEngine.int_ops(ops)
    I = _native.KZG_INT_IMM
    assert recs == [(1, 8, 0, 1, 0, 0, 1), (2, 1, 1, 1, 0, 0, 1), (3, 64, 0, 0, (1 << 64) - 1, I, 1), (4, 32, 0, 1, 0, 0, 2),
                    (5, 33, 1, 0, 0, I, 2), (6, 64, 0, 0, 0, 0, 2), (7, 31, 0, 0, 7, I, 1), (8, 64, 1, 0, 64, I, 2),
                    (8, 8, 0, 1, 0, 0, 1)]
    assert sum(r[6] for r in recs) == iref.n_out(ops) == 13
    assert [iref.KINDS[r[0] - 1] for r in recs] == [op[0] for op in ops]      # the kinds' numbers follow the reference's order
    HipEngine.int_ops([("add", 8, 0, 1, 2)] * 8)                              # 16 output rows fit
    HipEngine.int_ops([("and", 8, 0, 1)] * 16)


def test_a_good_call_reaches_exactly_the_export_of_its_own_name(eng):
    ops = [("xor", 32, 0, 1), ("mul", 64, 1, ("imm", 5), 2)]
    rset, counts, first = eng.commit_int(_sets(eng, 2), ops)
    assert [name for name, _ in eng._lib.calls] == ["kzg_rows_commit_int"]
    args = eng._lib.calls[0][1]
    assert len(args) == len(_native.SYMBOLS["kzg_rows_commit_int"][1])
    assert args[1] == 2 and args[3] == 2 and args[5] is None
    assert [(o.kind, o.width, o.a, o.b, o.imm, o.flags, o.count) for o in args[4]] == [(3, 32, 0, 1, 0, 0, 1), (6, 64, 1, 0, 5, 1, 2)]
    assert (rset.k, rset.i, rset.T, len(rset.commitments)) == (3, 3, T, 3) and counts == [0, 0]
    assert first == [0, 0]                                        # (the stub wrote nothing; the sentinel is the library's)
    # the usable layout rides in the options struct; bare handles of unknown length are accepted by the plain form
    eng._lib.calls.clear()
    u = T - 2
    s1 = b"\x01" * 32                          # (no zero byte: the field reads back as a C string)
    eng.commit_int(_sets(eng, 1), [("add", 8, 0, 0, 2)], u, [s1] * 4)
    opts = eng._lib.calls[0][1][5]._obj
    assert (opts.usable, opts.tail_be32) == (u, s1 * 4)
    out, _, _ = eng.commit_int([100, 101], [("and", 1, 1, 0)])
    assert (out.i, out.T) == (None, None)


def test_none_is_the_header_s_sentinel(eng):
    class _Lib:
        def kzg_rows_commit_int(self, *args):
            args[7][0], args[7][1] = 4, 0
            args[8][0], args[8][1] = 2, _native.KZG_INT_NONE
            return _native.KZG_OK

    eng._lib = _Lib()
    _, counts, first = eng.commit_int(_sets(eng, 1), [("and", 8, 0, 0), ("or", 8, 0, 0)])
    assert counts == [4, 0] and first == [2, None]


BAD = {
    "no ops (n_ops = 0)": (lambda h: (h(1), []), "n_ops"),
    "ops not a list": (lambda h: (h(1), None), "n_ops"),
    "17 ops": (lambda h: (h(1), [("and", 8, 0, 0)] * 17), "n_ops"),
    "17 output rows": (lambda h: (h(1), [("add", 8, 0, 0, 2)] * 8 + [("and", 8, 0, 0)]), "n_out"),
    "an unknown kind": (lambda h: (h(1), [("nand", 8, 0, 0)]), "unknown kind"),
    "a kind that is a number": (lambda h: (h(1), [(1, 8, 0, 0)]), "unknown kind"),
    "an op that is no tuple": (lambda h: (h(1), ["and"]), "an op is"),
    "an op too short": (lambda h: (h(1), [("and", 8, 0)]), "an op is"),
    "an op too long": (lambda h: (h(1), [("add", 8, 0, 0, 2, 1)]), "an op is"),
    "w = 0": (lambda h: (h(1), [("and", 0, 0, 0)]), "width"),
    "w = 65": (lambda h: (h(1), [("and", 65, 0, 0)]), "width"),
    "w a bool": (lambda h: (h(1), [("and", True, 0, 0)]), "width"),
    "count 0": (lambda h: (h(1), [("add", 8, 0, 0, 0)]), "count"),
    "count 3": (lambda h: (h(1), [("add", 8, 0, 0, 3)]), "count"),
    "count 2 on and": (lambda h: (h(1), [("and", 8, 0, 0, 2)]), "count"),
    "count 2 on or": (lambda h: (h(1), [("or", 8, 0, 0, 2)]), "count"),
    "count 2 on xor": (lambda h: (h(1), [("xor", 8, 0, 0, 2)]), "count"),
    "a negative row": (lambda h: (h(1), [("and", 8, -1, 0)]), "a row"),
    "a row that is no integer": (lambda h: (h(1), [("and", 8, "0", 0)]), "a row"),
    "a second row that is no integer": (lambda h: (h(1), [("and", 8, 0, "0")]), "second operand"),
    "a second row of 2^32": (lambda h: (h(1), [("and", 8, 0, 1 << 32)]), "second operand"),
    "an immediate of 2^w": (lambda h: (h(1), [("and", 8, 0, ("imm", 256))]), "immediate"),
    "an immediate of 2^64": (lambda h: (h(1), [("add", 64, 0, ("imm", 1 << 64))]), "immediate"),
    "a negative immediate": (lambda h: (h(1), [("add", 64, 0, ("imm", -1))]), "immediate"),
    "a shift of w + 1": (lambda h: (h(1), [("split", 8, 0, ("imm", 9))]), "immediate"),
    "an immediate with another tag": (lambda h: (h(1), [("and", 8, 0, ("const", 1))]), "immediate"),
    "a tail without usable": (lambda h: (h(1), [("and", 8, 0, 0)], None, [S]), "tail"),
    "usable 0": (lambda h: (h(1), [("and", 8, 0, 0)], 0), "usable"),
    "a short tail scalar": (lambda h: (h(1), [("and", 8, 0, 0)], T - 1, [S[:31]]), "32 bytes"),
    "a tail of the wrong length": (lambda h: (h(1), [("add", 8, 0, 0, 2)], T - 1, [S]), "exactly"),
    "usable over bare handles": (lambda h: ([100], [("and", 8, 0, 0)], T - 1, [S]), "unknown"),
    "no handles": (lambda h: ([], [("and", 8, 0, 0)]), ""),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_a_bad_shape_is_refused_under_the_method_s_name_before_any_native_call(eng, case):
    make, why = BAD[case]
    with pytest.raises(_native.KzgError) as err:
        eng.commit_int(*make(lambda n: _sets(eng, n)))
    assert err.value.code == _native.KZG_E_ARG
    msg = str(err.value).split(": ", 1)[1]
    assert msg.startswith("commit_int") and why in msg, str(err.value)
    assert eng._lib.calls == [], "a bad shape must be refused before any native call"


def test_the_text_client_refuses_malformed_ops_before_the_engine_and_passes_good_ones_on():
    from zkp_subnet_amd import Client, codec
    from zkp_subnet_amd.multi import MultiDeviceClient

    class _Engine:
        def commit_int(self, hs, ops, usable, tail):
            self.got = (hs, ops, usable, tail)
            return RowSet(self, 77, 0, 3, T, [bytes([0xc0]) + bytes(47)] * 3), [2, 0], [5, None]

    client = Client.__new__(Client)
    client.engine = _Engine()
    r = client.worker_commit_int([5, 6], [["xor", 32, 0, 1], ["mul", 64, 1, ["imm", 5], 2]])
    assert r.status_code == 200, r.json()
    assert client.engine.got == ([5, 6], [("xor", 32, 0, 1), ("mul", 64, 1, ("imm", 5), 2)], None, [])
    body = r.json()
    assert (body["handle"], body["counts"], body["first"], len(body["commitments"])) == (77, [2, 0], [5, None], 3)
    one = codec.be32_to_fr(S)
    client.engine.got = None
    for args in (([], [["and", 8, 0, 0]]), ([1], []), ([1], ["and"]), ([1], [["and", 8, 0]]), ([1], [["and", 8, 0, ["imm"]]]),
                 ([1], [["and", 8, 0, ["const", 1]]]), ([1], [["and", "w", 0, 0]]), ([1], [["and", 8, 0, 0]], None, [one]),
                 ([1], [["and", 8, 0, 0]], 0), ([1], 7)):
        r = client.worker_commit_int(*args)
        assert r.status_code == 400 and "error" in r.json(), args
    assert client.engine.got is None
    assert callable(getattr(MultiDeviceClient, "worker_commit_int"))


# ---------------------------------------------------------------------------------------------------- the header
def test_header_declares_the_symbols_the_struct_and_the_constants():
    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in ("kzg_rows_commit_int", "kzg_multi_rows_commit_int"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _native.SYMBOLS
    assert len(_native.SYMBOLS["kzg_multi_rows_commit_int"][1]) == len(_native.SYMBOLS["kzg_rows_commit_int"][1]) + 1
    consts = dict(re.findall(r"#define\s+(KZG_INT_[A-Z0-9]+)\s+(\w+)", hdr))
    names = ["AND", "OR", "XOR", "ADD", "SUB", "MUL", "DIVMOD", "SPLIT"]
    assert consts == {**{"KZG_INT_" + n: str(getattr(_native, "KZG_INT_" + n)) for n in names}, "KZG_INT_IMM": "1u",
                      "KZG_INT_NONE": "0xffffffffffffffffull"}
    assert [getattr(_native, "KZG_INT_" + n) for n in names] == list(range(1, 9)) and _native.KZG_INT_IMM == 1
    assert _native.KZG_INT_NONE == (1 << 64) - 1
    body = re.search(r"typedef struct kzg_int_op \{(.*?)\} kzg_int_op;", hdr, re.S).group(1)
    fields = re.findall(r"(uint32_t|uint64_t)\s+(\w+);", body)
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    assert [(f, ctype[t]) for t, f in fields] == list(_native.IntOp._fields_)
    assert ctypes.sizeof(_native.IntOp) == 32 and _native.IntOp.imm.offset == 16 and _native.IntOp.count.offset == 28
    block = hdr[hdr.index("THE INTEGER ALU COLUMNS"):hdr.index("int kzg_rows_commit_int")]
    for word in ("OUT OF SCOPE", "SOUNDNESS", "signed variants", "widths above 64", "three-operand", "per-row selectors",
                 "zero divisors", "RISC-V", "a + b = s + carry M", "a b = lo + hi M", "a = q b + rem", "a = hi 2^s + lo", '"int:"'):
        assert word in block, word
    for sibling in ("THE DERIVED COLUMNS", "THE FETCH"):
        start = hdr.index(sibling) if sibling in hdr else None
        assert start is not None, sibling
        scope = hdr[start:].split("OUT OF SCOPE", 1)[1].split("SOUNDNESS", 1)[0]
        assert "kzg_rows_commit_int" in scope, sibling
