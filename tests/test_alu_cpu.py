"""CPU checks around kzg_rows_commit_alu: the Python reference (tests/alu_ref.py) against the gate identities a caller proves
the rows with, against tests/int_ref.py on the eight shared kinds and against hand-written known answers; the statistics of
hand-made columns; the engine's encoders and dispatch over a recording stub library; the text client; the header.  No device."""
import ctypes
import os
import random
import re

import pytest

from tests import alu_ref as aref
from tests import int_ref as iref
from tests.gpu_common import R
from zkp_subnet_amd import _native
from zkp_subnet_amd.engine import HipEngine, RowSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 8
S = bytes(31) + b"\x01"
WIDTHS = [1, 2, 8, 31, 32, 33, 63, 64]
NEW = aref.KINDS[8:]


def edges(w):
    M = 1 << w
    return sorted({min(max(v, 0), M - 1) for v in (0, 1, M // 2 - 1, M // 2, M - 1)})


def operands(kind, w, seed):
    M = 1 << w
    rnd = random.Random(seed)
    pairs = [(x, y) for x in edges(w) for y in edges(w)] + [(rnd.randrange(M), rnd.randrange(M)) for _ in range(150)]
    if kind in aref.SHIFTS:
        pairs += [(x, s % M) for x in edges(w) + [rnd.randrange(M) for _ in range(8)] for s in (0, 1, w - 1, w)]
    return pairs


# ---------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("kind", NEW)
def test_the_reference_satisfies_the_gates(kind, w):
    M = 1 << w
    sgn = lambda x: aref.sgn(x, w)   # noqa: E731
    pairs = operands(kind, w, 100 * w + aref.KINDS.index(kind))
    if kind == "sext":
        pairs = [(x, f) for x, _ in pairs for f in {1, (w + 1) // 2, w}]
    for a, b in pairs:
        r0, r1, over = aref.cell(kind, w, a, b)
        assert not over and 0 <= r0 < M and 0 <= r1 < M, (a, b)
        s = b % w
        if kind in ("ltu", "lt", "eq"):
            assert r0 == {"ltu": int(a < b), "lt": int(sgn(a) < sgn(b)), "eq": int(a == b)}[kind]
            assert (r1 - (a - b)) % M == 0
        elif kind == "sll":
            assert a << s == r1 * M + r0
        elif kind == "srl":
            assert a == r0 * (1 << s) + r1 and r1 < 1 << s
        elif kind == "sra":
            assert sgn(r0) * (1 << s) + r1 == sgn(a) and r1 < 1 << s
        elif kind == "rotl":
            assert ((r0 >> s) | (r0 << (w - s))) % M == a and r1 == (a >> (w - s) if s else 0)
        elif kind == "rotr":
            assert ((r0 << s) | (r0 >> (w - s))) % M == a and r1 == a % (1 << s)
        elif kind == "mulhu":
            assert a * b == r0 * M + r1
        elif kind == "mulh":
            assert sgn(a) * sgn(b) == sgn(r0) * M + r1
        elif kind == "mulhsu":
            assert sgn(a) * b == sgn(r0) * M + r1
        elif kind in ("div", "rem"):
            q, r = (r0, r1) if kind == "div" else (r1, r0)
            if b == 0:
                assert (q, r) == (M - 1, a)
            elif a == M // 2 and b == M - 1:
                assert (q, r) == (M // 2, 0)                                  # the overflow
            else:
                assert sgn(a) == sgn(q) * sgn(b) + sgn(r) and abs(sgn(r)) < abs(sgn(b))
                assert r == 0 or (sgn(r) < 0) == (sgn(a) < 0)
        elif kind == "remu":
            assert (r0, r1) == (a, M - 1) if b == 0 else (a == r1 * b + r0 and r0 < b)
        else:                                                                 # sext: b is the field width f
            assert (r0 - a) % (1 << b) == 0 and -(1 << (b - 1)) <= sgn(r0) < 1 << (b - 1) and r1 == (a >> (b - 1)) & 1


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("kind", aref.SHARED)
def test_the_shared_kinds_equal_the_integer_reference(kind, w):
    M = 1 << w
    rnd = random.Random(w)
    outside = [M, (1 << 64) - 1, 1 << 64, R - 1]
    pairs = [(x, y) for x in edges(w) + outside for y in edges(w) + outside + [w, w + 1]]
    pairs += [(rnd.randrange(M), rnd.randrange(M)) for _ in range(100)] + [(rnd.randrange(R), rnd.randrange(R)) for _ in range(50)]
    for x, y in pairs:
        want = iref.cell(kind, w, x, y)
        assert aref.cell(kind, w, x, y) == (want[0], 0 if want[1] is None else want[1], want[2]), (x, y)
    assert aref.KINDS[:8] == iref.KINDS


def test_known_answers_at_32_bits():
    w, M = 32, 1 << 32
    neg = lambda v: v % M   # noqa: E731
    assert aref.cell("div", w, neg(-7), 2)[:2] == (neg(-3), neg(-1))
    assert aref.cell("rem", w, neg(-7), 2)[:2] == (neg(-1), neg(-3))
    for a in (0, 5, 0x80000000, M - 1):
        assert aref.cell("div", w, a, 0)[:2] == (M - 1, a) and aref.cell("remu", w, a, 0)[:2] == (a, M - 1)
    assert aref.cell("div", w, 0x80000000, neg(-1))[:2] == (0x80000000, 0)
    assert aref.cell("sra", w, 0x80000000, 31)[:2] == (0xFFFFFFFF, 0)
    assert aref.cell("mulh", w, neg(-1), neg(-1))[:2] == (0, 1)
    assert aref.cell("mulhsu", w, neg(-1), 0xFFFFFFFF)[:2] == (0xFFFFFFFF, 1)
    assert aref.cell("mulhu", w, M - 1, M - 1)[:2] == (M - 2, 1)
    assert aref.cell("sll", w, 0x80000001, 33)[:2] == (2, 1)                  # s = 33 mod 32
    assert aref.cell("rotr", w, 1, 1)[:2] == (0x80000000, 1)
    assert aref.cell("lt", w, 0x80000000, 1)[0] == 1 and aref.cell("ltu", w, 0x80000000, 1)[0] == 0
    assert aref.cell("sext", w, 0x1280, 8)[:2] == (0xFFFFFF80, 1) and aref.cell("sext", w, 0x1280, 16)[:2] == (0x1280, 0)
    assert aref.cell("sext", w, 5, 0) == (5, 0, True) and aref.cell("sext", w, 5, 33) == (5, 0, True)
    # w = 1: sgn 1 = -1, every shift amount is 0
    assert aref.cell("div", 1, 1, 1)[:2] == (1, 0) and aref.cell("lt", 1, 1, 0)[0] == 1 and aref.cell("sra", 1, 1, 1)[:2] == (1, 0)
    assert aref.cell("mulh", 1, 1, 1)[:2] == (0, 1) and aref.cell("sext", 1, 1, 1)[:2] == (1, 1)


def test_statistics_of_hand_made_columns():
    program = [("add", 8), None, ("sll", 8, ("imm", 3)), ("sext", 8)]
    op = [0, 1, 2, 3, 9, 0, 1 << 32, 3]
    a = [255, R - 1, 1, 0x85, 7, 300, 1, 0x85]
    b = [1, 1 << 64, 1 << 70, 4, 7, 1, 1, 9]
    r0, r1, st = aref.rows(program, [op, a, b], (0, 1, 2, 2), T)
    assert r0 == [0, 0, 8, 5, 0, 45, 0, 0x85] and r1 == [1, 0, 0, 0, 0, 0, 0, 1]
    # row 1 is idle and row 2 has an immediate: their out-of-range a and b cells count nothing; rows 5 (a) and 7 (f = 9) do
    assert st == {"counts": 2, "first": 5, "unknown": 2, "first_unknown": 4}
    cols, stats = aref.alu_columns([op, a, b], program, [(0, 1, 2, 2), (0, 1, 2)], 6, [90, 91, 92, 93, 94, 95])
    assert cols == [r0[:6] + [90, 91], r1[:6] + [92, 93], r0[:6] + [94, 95]]
    assert stats == {"counts": [1, 1], "first": [5, 5], "unknown": [1, 1], "first_unknown": [4, 4]}
    # a constant op-code column: the cells of a at or above 2^8 are rows 1 and 5
    assert aref.rows([("and", 8)], [[0] * T, a, b], (0, 1, 1), T)[2] == {"counts": 2, "first": 1, "unknown": 0,
                                                                        "first_unknown": None}


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


def test_the_encoders_give_the_struct_fields():
    program = [("and", 8), None, ["sra", 64, ["imm", (1 << 64) - 1]], ("sext", 32, ("imm", 16)), ("split", 8, ("imm", 8)),
               ("mulhsu", 1), ("sext", 5)]
    recs = HipEngine.alu_program(program)
    I = _native.KZG_ALU_IMM
    assert recs == [(1, 8, 0, 0, 0), (0, 0, 0, 0, 0), (14, 64, (1 << 64) - 1, I, 0), (23, 32, 16, I, 0), (8, 8, 8, I, 0),
                    (19, 1, 0, 0, 0), (23, 5, 0, 0, 0)]
    assert [HipEngine._ALU_KINDS[k] for k in aref.KINDS] == list(range(1, 24))
    assert HipEngine.alu_units([(0, 1, 2), [2, 2, 2, 2]], recs) == [(0, 1, 2, 1), (2, 2, 2, 2)]
    HipEngine.alu_units([(0, 1, 2, 2)] * 8, recs)                            # 16 output rows fit
    HipEngine.alu_program([None] * 64)


def test_a_good_call_reaches_exactly_the_export_of_its_own_name(eng):
    rset, st = eng.commit_alu(_sets(eng, 3), [("add", 32), None, ("srl", 32, ("imm", 5))], [(0, 1, 2, 2), (2, 2, 2)])
    assert [name for name, _ in eng._lib.calls] == ["kzg_rows_commit_alu"]
    args = eng._lib.calls[0][1]
    assert len(args) == len(_native.SYMBOLS["kzg_rows_commit_alu"][1])
    assert (args[1], args[3], args[5], args[7]) == (3, 3, 2, None)
    assert [(e.kind, e.width, e.imm, e.flags, e.pad) for e in args[4]] == [(4, 32, 0, 0, 0), (0, 0, 0, 0, 0), (13, 32, 5, 1, 0)]
    assert [(u.op_row, u.a, u.b, u.count) for u in args[6]] == [(0, 1, 2, 2), (2, 2, 2, 1)]
    assert (rset.k, rset.i, rset.T, len(rset.commitments)) == (3, 3, T, 3)
    assert st == {"counts": [0, 0], "first": [0, 0], "unknown": [0, 0], "first_unknown": [0, 0]}   # (the stub wrote nothing)
    eng._lib.calls.clear()
    s1 = b"\x01" * 32
    eng.commit_alu(_sets(eng, 1), [("add", 8)], [(0, 0, 0, 2)], T - 2, [s1] * 4)
    opts = eng._lib.calls[0][1][7]._obj
    assert (opts.usable, opts.tail_be32) == (T - 2, s1 * 4)


def test_none_is_the_header_s_sentinel(eng):
    class _Lib:
        def kzg_rows_commit_alu(self, *args):
            args[9][0], args[10][0], args[11][0], args[12][0] = 4, 2, 0, _native.KZG_ALU_NONE
            return _native.KZG_OK

    eng._lib = _Lib()
    _, st = eng.commit_alu(_sets(eng, 1), [("and", 8)], [(0, 0, 0)])
    assert st == {"counts": [4], "first": [2], "unknown": [0], "first_unknown": [None]}


P = [("add", 8), ("and", 8)]
U = [(0, 0, 0)]
BAD = {
    "an empty program": (lambda h: (h(1), [], U), "n_entries"),
    "a program that is no list": (lambda h: (h(1), None, U), "n_entries"),
    "65 entries": (lambda h: (h(1), [("and", 8)] * 65, U), "n_entries"),
    "an unknown kind": (lambda h: (h(1), [("nand", 8)], U), "unknown kind"),
    "a kind that is a number": (lambda h: (h(1), [(1, 8)], U), "unknown kind"),
    "an entry that is no tuple": (lambda h: (h(1), ["and"], U), "an entry is"),
    "an entry too long": (lambda h: (h(1), [("and", 8, ("imm", 1), 1)], U), "an entry is"),
    "w = 0": (lambda h: (h(1), [("and", 0)], U), "width"),
    "w = 65": (lambda h: (h(1), [("and", 65)], U), "width"),
    "w a bool": (lambda h: (h(1), [("and", True)], U), "width"),
    "an immediate of 2^w": (lambda h: (h(1), [("and", 8, ("imm", 256))], U), "immediate"),
    "an immediate of 2^64": (lambda h: (h(1), [("add", 64, ("imm", 1 << 64))], U), "immediate"),
    "a negative immediate": (lambda h: (h(1), [("add", 64, ("imm", -1))], U), "immediate"),
    "a split at w + 1": (lambda h: (h(1), [("split", 8, ("imm", 9))], U), "immediate"),
    "a sext from w + 1": (lambda h: (h(1), [("sext", 8, ("imm", 9))], U), "immediate"),
    "a sext from 0": (lambda h: (h(1), [("sext", 8, ("imm", 0))], U), "immediate"),
    "an immediate with another tag": (lambda h: (h(1), [("and", 8, ("const", 1))], U), "immediate"),
    "no units": (lambda h: (h(1), P, []), "n_units"),
    "9 units": (lambda h: (h(1), P, U * 9), "n_units"),
    "units that are no list": (lambda h: (h(1), P, 7), "n_units"),
    # (more than 16 output rows need a ninth unit, since a unit has at most two: the n_out check cannot be reached alone)
    "18 output rows in 9 units": (lambda h: (h(1), P, [(0, 0, 0, 2)] * 9), "n_units"),
    "a unit too short": (lambda h: (h(1), P, [(0, 0)]), "a unit is"),
    "a unit too long": (lambda h: (h(1), P, [(0, 0, 0, 1, 1)]), "a unit is"),
    "a negative row": (lambda h: (h(1), P, [(0, -1, 0)]), "a row"),
    "a row of 2^32": (lambda h: (h(1), P, [(1 << 32, 0, 0)]), "a row"),
    "a row that is no integer": (lambda h: (h(1), P, [(0, 0, "0")]), "a row"),
    "count 0": (lambda h: (h(1), P, [(0, 0, 0, 0)]), "count"),
    "count 3": (lambda h: (h(1), P, [(0, 0, 0, 3)]), "count"),
    "count 2 on and": (lambda h: (h(1), [("and", 8), None, ("xor", 8)], [(0, 0, 0, 2)]), "count"),
    "a tail without usable": (lambda h: (h(1), P, U, None, [S]), "tail"),
    "usable 0": (lambda h: (h(1), P, U, 0), "usable"),
    "a short tail scalar": (lambda h: (h(1), P, U, T - 1, [S[:31]]), "32 bytes"),
    "a tail of the wrong length": (lambda h: (h(1), P, [(0, 0, 0, 2)], T - 1, [S]), "exactly"),
    "usable over bare handles": (lambda h: ([100], P, U, T - 1, [S]), "unknown"),
    "no handles": (lambda h: ([], P, U), ""),
}

@pytest.mark.parametrize("case", sorted(BAD))
def test_a_bad_shape_is_refused_under_the_method_s_name_before_any_native_call(eng, case):
    make, why = BAD[case]
    with pytest.raises(_native.KzgError) as err:
        eng.commit_alu(*make(lambda n: _sets(eng, n)))
    assert err.value.code == _native.KZG_E_ARG
    msg = str(err.value).split(": ", 1)[1]
    assert msg.startswith("commit_alu") and why in msg, str(err.value)
    assert eng._lib.calls == [], "a bad shape must be refused before any native call"


def test_the_text_client_refuses_malformed_input_before_the_engine_and_passes_good_input_on():
    from zkp_subnet_amd import Client, codec
    from zkp_subnet_amd.multi import MultiDeviceClient

    class _Engine:
        def commit_alu(self, hs, program, units, usable, tail):
            self.got = (hs, program, units, usable, tail)
            return (RowSet(self, 77, 0, 3, T, [bytes([0xc0]) + bytes(47)] * 3),
                    {"counts": [2, 0], "first": [5, None], "unknown": [0, 1], "first_unknown": [None, 3]})

    client = Client.__new__(Client)
    client.engine = _Engine()
    r = client.worker_commit_alu([5, 6], [["add", 32], None, ["srl", 32, ["imm", 5]]], [[0, 1, 2, 2], [2, 2, 2]])
    assert r.status_code == 200, r.json()
    assert client.engine.got == ([5, 6], [("add", 32), None, ("srl", 32, ("imm", 5))], [(0, 1, 2, 2), (2, 2, 2)], None, [])
    body = r.json()
    assert (body["handle"], body["counts"], body["first"], body["unknown"], body["first_unknown"], len(body["commitments"])) == (
        77, [2, 0], [5, None], [0, 1], [None, 3], 3)
    one = codec.be32_to_fr(S)
    client.engine.got = None
    ok_p, ok_u = [["and", 8]], [[0, 0, 0]]
    for args in (([], ok_p, ok_u), ([1], [], ok_u), ([1], ok_p, []), ([1], ["and"], ok_u), ([1], [["and"]], ok_u),
                 ([1], [["and", 8, ["imm"]]], ok_u), ([1], [["and", 8, ["const", 1]]], ok_u), ([1], [["and", "w"]], ok_u),
                 ([1], ok_p, [[0, 0]]), ([1], ok_p, ["000"]), ([1], ok_p, ok_u * 9), ([1], ok_p * 65, ok_u), ([1], 7, ok_u),
                 ([1], ok_p, ok_u, None, [one]), ([1], ok_p, ok_u, 0)):
        r = client.worker_commit_alu(*args)
        assert r.status_code == 400 and "error" in r.json(), args
        assert "worker_commit_alu" in r.json()["error"] or args[0] == [], r.json()
    assert client.engine.got is None
    assert callable(getattr(MultiDeviceClient, "worker_commit_alu"))


# ---------------------------------------------------------------------------------------------------- the header
def test_header_declares_the_symbols_the_structs_and_the_constants():
    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in ("kzg_rows_commit_alu", "kzg_multi_rows_commit_alu"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _native.SYMBOLS
    assert len(_native.SYMBOLS["kzg_multi_rows_commit_alu"][1]) == len(_native.SYMBOLS["kzg_rows_commit_alu"][1]) + 1
    consts = dict(re.findall(r"#define\s+(KZG_ALU_[A-Z0-9_]+)\s+(\w+)", hdr))
    names = [k.upper() for k in aref.KINDS]
    assert consts == {**{"KZG_ALU_" + n: str(getattr(_native, "KZG_ALU_" + n)) for n in names}, "KZG_ALU_IDLE": "0",
                      "KZG_ALU_IMM": "1u", "KZG_ALU_NONE": "0xffffffffffffffffull", "KZG_ALU_MAX_PROGRAM": "64",
                      "KZG_ALU_MAX_UNITS": "8"}
    assert [getattr(_native, "KZG_ALU_" + n) for n in names] == list(range(1, 24))
    assert [getattr(_native, "KZG_ALU_" + n) for n in names[:8]] == [getattr(_native, "KZG_INT_" + n) for n in names[:8]]
    assert (_native.KZG_ALU_IDLE, _native.KZG_ALU_IMM, _native.KZG_ALU_NONE) == (0, 1, (1 << 64) - 1)
    assert (_native.KZG_ALU_MAX_PROGRAM, _native.KZG_ALU_MAX_UNITS) == (64, 8)
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    for struct, cls, size in (("kzg_alu_entry", _native.AluEntry, 24), ("kzg_alu_unit", _native.AluUnit, 16)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        fields = re.findall(r"(uint32_t|uint64_t)\s+(\w+);", body)
        assert [(f, ctype[t]) for t, f in fields] == list(cls._fields_) and ctypes.sizeof(cls) == size
    assert _native.AluEntry.imm.offset == 8
    block = hdr[hdr.index("THE ALU COLUMN WITH AN OP-CODE COLUMN"):hdr.index("int kzg_rows_commit_alu")]
    for word in ("OUT OF SCOPE", "SOUNDNESS", "widths above 64", "three-operand", "per-row width", "per-row\n * count", "clz",
                 "min / max", "zero divisors or overflows", "any proof", "RISC-V", '"alu:"', "b mod w", "UNKNOWN", "idle"):
        assert word in block, word
    int_block = hdr[hdr.index("THE INTEGER ALU COLUMNS"):hdr.index("int kzg_rows_commit_int")]
    assert "kzg_rows_commit_alu" in int_block.split("OUT OF SCOPE", 1)[1].split("SOUNDNESS", 1)[0]
