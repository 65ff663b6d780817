"""CPU checks around kzg_rows_commit_derived: the Python reference (tests/derived_ref.py) against brute force, the engine's
dispatch over a recording stub library, and the header's declarations.  No device."""
import ctypes
import os
import random
import re

import pytest

from tests import derived_ref as dref
from zkp_subnet_amd import _native
from zkp_subnet_amd.engine import HipEngine, RowSet

R = dref.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 8
S = bytes(31) + b"\x01"


# ---------------------------------------------------------------------------------------------------- the reference
def test_modulus_is_the_library_s():
    from tests.gpu_common import R as R_common

    assert R == R_common


def test_inv0_against_brute_force():
    rnd = random.Random(1)
    col = [0, 1, R - 1, 2, 0] + [rnd.randrange(R) for _ in range(59)] + [0]
    inv, bit, zeros = dref.inv0(col)
    assert zeros == 3 and sum(bit) == 3
    for x, y, b in zip(col, inv, bit):
        assert x * y % R == (0 if x == 0 else 1) and b == 1 - x * y % R
        assert y == (pow(x, R - 2, R) if x else 0)
        assert x * b % R == 0
    assert dref.inv0([0] * 4) == ([0] * 4, [1] * 4, 4)
    assert dref.inv0([1, R - 1]) == ([1, R - 1], [0, 0], 0)
    assert dref.batch_inverse([]) == []


@pytest.mark.parametrize("b,L", [(1, 16), (8, 4), (16, 4), (16, 16), (32, 8), (13, 5), (31, 3), (1, 1), (32, 1)])
def test_limbs_recompose_to_the_value_modulo_their_width(b, L):
    rnd = random.Random(100 * b + L)
    top = 1 << (b * L)
    col = [0, 1, top - 1, min(top, R - 1), R - 1] + [rnd.randrange(R) for _ in range(40)] + [rnd.randrange(min(top, R)) for _ in range(20)]
    ls, over = dref.limbs(col, b, L)
    assert len(ls) == L and all(len(c) == len(col) for c in ls)
    for t, x in enumerate(col):
        assert all(0 <= ls[l][t] < 1 << b for l in range(L))
        assert sum(ls[l][t] << (b * l) for l in range(L)) == x % top
    assert over == sum(1 for x in col if x >= top)
    if b * L >= 255:
        assert over == 0


def test_overflow_count_on_hand_made_columns():
    assert dref.limbs([0, 255, 256, 257, 65535, 65536], 8, 1) == ([[0, 255, 0, 1, 255, 0]], 4)
    assert dref.limbs([0, 255, 256, 257, 65535, 65536], 8, 2) == ([[0, 255, 0, 1, 255, 0], [0, 0, 1, 1, 255, 0]], 1)
    assert dref.limbs([(1 << 65) - 1, 1 << 65, R - 1], 13, 5)[1] == 2
    assert dref.limbs([R - 1] * 3, 16, 16)[1] == 0
    assert dref.limbs([R - 1, 1 << 31, (1 << 31) - 1], 31, 1) == ([[(R - 1) & 0x7FFFFFFF, 0, 0x7FFFFFFF]], 2)


def test_layout_and_order_of_mixed_ops():
    rnd = random.Random(3)
    cols = [[rnd.randrange(1 << 20) for _ in range(T)], [0, 5, 0, 7, 0, 0, 9, 1]]
    ops = [("limbs", 0, 8, 2), ("inv0", 1, True), ("inv0", 0), ("limbs", 1, 2, 1)]
    assert dref.n_out(ops) == 6
    out, counts = dref.derived_columns(cols, ops)
    assert len(out) == 6 and counts == [sum(1 for x in cols[0] if x >> 16), 4, cols[0].count(0), 3]
    assert out[0] == [x & 255 for x in cols[0]] and out[1] == [(x >> 8) & 255 for x in cols[0]]
    assert out[3] == [0 if x else 1 for x in cols[1]] and out[5] == [x & 3 for x in cols[1]]
    # usable: the rows behind are neither read nor counted, the tail is column-major
    u = 5
    tail = list(range(1000, 1000 + 6 * (T - u)))
    out_u, counts_u = dref.derived_columns(cols, ops, u, tail)
    assert counts_u == [sum(1 for x in cols[0][:u] if x >> 16), 3, cols[0][:u].count(0), 2]
    for c in range(6):
        assert out_u[c][:u] == out[c][:u] and out_u[c][u:] == tail[c * (T - u):(c + 1) * (T - u)]


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


def test_a_good_call_reaches_exactly_the_export_of_its_own_name(eng):
    ops = [("inv0", 0), ("inv0", 1, True), ("limbs", 0, 16, 4)]
    rset, counts = eng.commit_derived(_sets(eng, 2), ops)
    assert [name for name, _ in eng._lib.calls] == ["kzg_rows_commit_derived"]
    args = eng._lib.calls[0][1]
    assert len(args) == len(_native.SYMBOLS["kzg_rows_commit_derived"][1])
    assert args[1] == 2 and args[3] == 3 and args[5] is None
    assert [(o.kind, o.row, o.bits, o.count) for o in args[4]] == [(1, 0, 0, 1), (1, 1, 0, 2), (2, 0, 16, 4)]
    assert (rset.k, rset.i, rset.T, len(rset.commitments)) == (7, 3, T, 7) and counts == [0, 0, 0]
    # the usable layout rides in the options struct; bare handles of unknown length are accepted by the plain form
    eng._lib.calls.clear()
    u = T - 2
    s1 = b"\x01" * 32                          # (no zero byte: the field reads back as a C string)
    eng.commit_derived(_sets(eng, 1), [("inv0", 0, False)], u, [s1] * 2)
    opts = eng._lib.calls[0][1][5]._obj
    assert (opts.usable, opts.tail_be32) == (u, s1 * 2)
    out, _ = eng.commit_derived([100, 101], [("limbs", 1, 1, 1)])
    assert (out.i, out.T) == (None, None)


BAD = {
    "no ops": lambda h: (h(1), []),
    "ops not a list": lambda h: (h(1), None),
    "unknown kind": lambda h: (h(1), [("sqrt", 0)]),
    "an op that is no tuple": lambda h: (h(1), ["inv0"]),
    "inv0 with bits": lambda h: (h(1), [("inv0", 0, 8, 1)]),
    "inv0 with a flag that is no bool": lambda h: (h(1), [("inv0", 0, 2)]),
    "limbs too short": lambda h: (h(1), [("limbs", 0, 8)]),
    "bits 0": lambda h: (h(1), [("limbs", 0, 0, 4)]),
    "bits 33": lambda h: (h(1), [("limbs", 0, 33, 1)]),
    "count 0": lambda h: (h(1), [("limbs", 0, 8, 0)]),
    "count 17": lambda h: (h(1), [("limbs", 0, 8, 17)]),
    "b * L > 256": lambda h: (h(1), [("limbs", 0, 32, 9)]),
    "a negative row": lambda h: (h(1), [("inv0", -1)]),
    "a row that is no integer": lambda h: (h(1), [("inv0", "0")]),
    "17 output rows": lambda h: (h(1), [("limbs", 0, 8, 16), ("inv0", 0)]),
    "a tail without usable": lambda h: (h(1), [("inv0", 0)], None, [S]),
    "usable 0": lambda h: (h(1), [("inv0", 0)], 0),
    "a short tail scalar": lambda h: (h(1), [("inv0", 0)], T - 1, [S[:31]]),
    "a tail of the wrong length": lambda h: (h(1), [("inv0", 0, True)], T - 1, [S]),
    "usable over bare handles": lambda h: ([100], [("inv0", 0)], T - 1, [S]),
    "no handles": lambda h: ([], [("inv0", 0)]),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_a_bad_shape_is_refused_under_the_method_s_name_before_any_native_call(eng, case):
    with pytest.raises(_native.KzgError) as err:
        eng.commit_derived(*BAD[case](lambda n: _sets(eng, n)))
    assert err.value.code == _native.KZG_E_ARG
    assert str(err.value).split(": ", 1)[1].startswith("commit_derived"), str(err.value)
    assert eng._lib.calls == [], "a bad shape must be refused before any native call"


# ---------------------------------------------------------------------------------------------------- the header
def test_header_declares_the_symbol_the_structs_and_the_constants():
    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in ("kzg_rows_commit_derived", "kzg_multi_rows_commit_derived"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _native.SYMBOLS
    assert len(_native.SYMBOLS["kzg_multi_rows_commit_derived"][1]) == len(_native.SYMBOLS["kzg_rows_commit_derived"][1]) + 1
    consts = dict(re.findall(r"#define\s+(KZG_DERIVE_[A-Z0-9]+)\s+(\d+)", hdr))
    assert consts == {"KZG_DERIVE_INV0": str(_native.KZG_DERIVE_INV0), "KZG_DERIVE_LIMBS": str(_native.KZG_DERIVE_LIMBS)}
    assert re.search(r"\}\s*kzg_derive_op;", hdr) and re.search(r"\}\s*kzg_derive_opts;", hdr)
    body = re.search(r"typedef struct kzg_derive_op \{(.*?)\} kzg_derive_op;", hdr, re.S).group(1)
    assert re.findall(r"uint32_t\s+(\w+);", body) == [f for f, _ in _native.DeriveOp._fields_]
    assert ctypes.sizeof(_native.DeriveOp) == 16 and ctypes.sizeof(_native.DeriveOpts) == ctypes.sizeof(_native.SortedOpts)
    assert [f for f, _ in _native.DeriveOpts._fields_] == [f for f, _ in _native.SortedOpts._fields_]
