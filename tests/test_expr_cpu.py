"""CPU checks around kzg_rows_commit_expr: the header's declarations against the ctypes bindings, the methods of the three
Python layers, the Python reference (tests/expr_ref.py) against hand-computed cases, the engine's dispatch over a recording stub
library and the Python-side refusals.  No device."""
import ctypes
import os
import re

import pytest

from tests import expr_ref as xref
from tests.gpu_common import R
from zkp_subnet_amd import _native, codec
from zkp_subnet_amd.client import Client
from zkp_subnet_amd.engine import HipEngine, RowSet
from zkp_subnet_amd.multi import MultiDeviceClient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 8
S = b"\x01" * 32                              # (no zero byte: a tail field reads back as a C string)
ONE = bytes(31) + b"\x01"


# ---------------------------------------------------------------------------------------------------- the header
def _header():
    return open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()


def test_header_declares_the_call_the_structs_and_the_three_defines():
    hdr = _header()
    for name in ("kzg_rows_commit_expr", "kzg_multi_rows_commit_expr"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert re.search(r"#define\s+KZG_MAX_EXPR_FACTORS\s+8\b", hdr) and _native.KZG_MAX_EXPR_FACTORS == 8
    assert re.search(r"#define\s+KZG_EXPR_CHECK\s+1u\b", hdr) and _native.KZG_EXPR_CHECK == 1
    assert re.search(r"#define\s+KZG_EXPR_NONE\s+0xffffffffffffffffull\b", hdr) and _native.KZG_EXPR_NONE == 2 ** 64 - 1
    assert re.search(r"\}\s*kzg_expr;", hdr) and re.search(r"\}\s*kzg_expr_opts;", hdr)
    # the derived call no longer names the expression rows as missing; the new call states what it leaves out and what it proves
    derived = hdr[hdr.index("THE DERIVED COLUMNS"):hdr.index("THE EXPRESSION COLUMNS")]
    assert "kzg_rows_commit_expr" in derived.split("OUT OF SCOPE")[1].split("SOUNDNESS")[0]
    text = hdr[hdr.index("THE EXPRESSION COLUMNS"):hdr.index("#define KZG_MAX_EXPR_FACTORS")]
    assert "OUT OF SCOPE" in text and "SOUNDNESS" in text and "checked on the HOST" in text


def test_native_binds_both_symbols_with_the_header_s_struct_layouts():
    hdr = _header()
    one, multi = _native.SYMBOLS["kzg_rows_commit_expr"], _native.SYMBOLS["kzg_multi_rows_commit_expr"]
    assert one[0] is ctypes.c_int and multi[0] is ctypes.c_int
    assert len(one[1]) == 10 and multi[1] == [one[1][0], ctypes.c_uint32] + one[1][1:]
    for sym, ctype in (("kzg_rows_commit_expr", one), ("kzg_multi_rows_commit_expr", multi)):
        decl = re.search(r"\bint\s+" + sym + r"\s*\((.*?)\);", hdr, re.S).group(1)
        decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
        assert len(decl.split(",")) == len(ctype[1]), sym
    # kzg_expr: the existing terms struct, then the flags
    body = re.search(r"typedef struct kzg_expr \{(.*?)\} kzg_expr;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("kzg_quotient_terms", "terms"), ("uint32_t", "flags")]
    assert [f for f, _ in _native.Expr._fields_] == ["terms", "flags"]
    assert _native.Expr._fields_[0][1] is _native.QuotientTerms and _native.Expr._fields_[1][1] is ctypes.c_uint32
    tbody = re.search(r"typedef struct kzg_quotient_terms \{(.*?)\} kzg_quotient_terms;", hdr, re.S).group(1)
    tbody = re.sub(r"/\*.*?\*/", "", tbody, flags=re.S)
    assert re.findall(r"(\w+);", tbody) == [f for f, _ in _native.QuotientTerms._fields_]
    assert ctypes.sizeof(_native.QuotientTerms) == 40 and ctypes.sizeof(_native.Expr) == 48
    assert _native.Expr.flags.offset == 40
    # kzg_expr_opts: as kzg_derive_opts
    obody = re.search(r"typedef struct kzg_expr_opts \{(.*?)\} kzg_expr_opts;", hdr, re.S).group(1)
    obody = re.sub(r"/\*.*?\*/", "", obody, flags=re.S)
    assert re.findall(r"(\w+);", obody) == [f for f, _ in _native.ExprOpts._fields_] == [f for f, _ in _native.DeriveOpts._fields_]
    assert ctypes.sizeof(_native.ExprOpts) == ctypes.sizeof(_native.DeriveOpts) == 16


def test_the_three_python_layers_have_the_methods():
    assert callable(getattr(HipEngine, "commit_expr"))
    assert callable(getattr(Client, "worker_commit_expr"))
    assert callable(getattr(MultiDeviceClient, "worker_commit_expr"))


# ---------------------------------------------------------------------------------------------------- the reference
A = [3, 5, 7, 11, 13, 17, 19, 23]
B = [2, 0, R - 1, 4, 1, 0, 6, 9]


def test_reference_constant_copy_and_square():
    rows, nz, first = xref.expr_columns([A], [([(42, [])],), ([(1, [0])],), ([(1, [0, 0])],)])
    assert rows == [[42] * T, A, [a * a for a in A]]
    assert nz == [T, T, T] and first == [0, 0, 0]
    # the constant 0, and r as a coefficient (reduced): nothing is non-zero
    assert xref.expr_columns([A], [([(0, [])],), ([(R, [0])],)])[1:] == ([0, 0], [None, None])


def test_reference_rotations_wrap_and_reduce_mod_T():
    nxt, prv = A[1:] + A[:1], A[-1:] + A[:-1]
    rows = xref.expr_columns([A], [([(1, [(0, 1)])],), ([(1, [(0, -1)])],), ([(1, [(0, T)])],), ([(1, [(0, T + 1)])],),
                                   ([(1, [(0, -2 ** 31)])],), ([(1, [(0, 2 ** 31 - 1)])],)])[0]
    assert rows[0] == nxt and rows[1] == prv and rows[2] == A and rows[3] == nxt
    assert rows[4] == A and rows[5] == prv                          # -2^31 = 0 and 2^31 - 1 = -1 (mod 8)
    # a * b - c with c = a * b: zero everywhere; one cell of c off by one: one non-zero cell, there
    c = [a * b % R for a, b in zip(A, B)]
    gate = [(1, [0, 1]), (R - 1, [2])]
    assert xref.expr_columns([A, B, c], [(gate, True)]) == ([], [0], [None])
    c[5] = (c[5] + 1) % R
    assert xref.expr_columns([A, B, c], [(gate, True)]) == ([], [1], [5])
    # one row at two rotations in one term: a[t] a[t + 1]
    assert xref.expr_columns([A], [([(1, [0, (0, 1)])],)])[0] == [[A[t] * A[(t + 1) % T] for t in range(T)]]


def test_reference_sums_products_and_counts():
    rows, nz, first = xref.expr_columns([A, B], [([(1, [0, 1])],), ([(2, [0, 1]), (R - 1, [1])], True), ([(1, [1])],)])
    assert rows == [[a * b % R for a, b in zip(A, B)], B]          # the check yields no row
    assert nz == [6, 6, 6] and first == [0, 0, 0]
    assert rows[0][2] == (7 * (R - 1)) % R == R - 7
    assert xref.expr_columns([[0, 0, 0, 9]], [([(1, [0])], True)]) == ([], [1], [3])


def test_reference_tail_layout_and_the_rows_behind_usable():
    u = 5
    cols = [A, B[:u] + [R - 1] * (T - u)]
    exprs = [([(1, [0, 1])],), ([(1, [1])], True), ([(1, [(1, 1)])],)]
    tail = list(range(100, 100 + 2 * (T - u)))
    rows, nz, first = xref.expr_columns(cols, exprs, u, tail)
    assert xref.n_out(exprs) == 2 and len(rows) == 2
    assert rows[0] == [a * b % R for a, b in zip(A[:u], B[:u])] + [100, 101, 102]     # column-major: column 0's tail first
    assert rows[1][u:] == [103, 104, 105]
    assert rows[1][:u] == [B[1], B[2], B[3], B[4], R - 1]          # a rotated factor reads across `usable`
    assert nz == [4, 4, 4] and first == [0, 0, 1]                  # the cells r - 1 behind `usable` are not counted
    with pytest.raises(AssertionError):
        xref.expr_columns(cols, exprs, u, tail[:-1])


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
    exprs = [([(ONE, [0, (1, -1)]), (S, [])],), ([(ONE, [1])], True), ([(S, [(0, 2 ** 31 - 1)])], False)]
    rset, nz, first = eng.commit_expr(_sets(eng, 2), exprs)
    assert [name for name, _ in eng._lib.calls] == ["kzg_rows_commit_expr"]
    args = eng._lib.calls[0][1]
    assert len(args) == len(_native.SYMBOLS["kzg_rows_commit_expr"][1])
    assert args[1] == 2 and args[3] == 3 and args[5] is None
    e0, e1, e2 = args[4][0], args[4][1], args[4][2]
    assert (e0.flags, e1.flags, e2.flags) == (0, _native.KZG_EXPR_CHECK, 0)
    assert e0.terms.n_terms == 2 and list(e0.terms.term_lens[:2]) == [2, 0]
    assert list(e0.terms.term_rows[:2]) == [0, 1] and list(e0.terms.term_rots[:2]) == [0, -1]
    assert e2.terms.term_rots[0] == 2 ** 31 - 1
    assert (rset.k, rset.i, rset.T, len(rset.commitments)) == (2, 3, T, 2)
    assert nz == [0, 0, 0] and first == [0, 0, 0]                  # (the stub writes nothing: zeros, not KZG_EXPR_NONE)
    # checks alone: no set, no commitment buffer
    eng._lib.calls.clear()
    rset, nz, first = eng.commit_expr(_sets(eng, 1), [([(ONE, [0])], True)], T - 2)
    assert rset is None and eng._lib.calls[0][1][6] is None
    opts = eng._lib.calls[0][1][5]._obj
    assert (opts.usable, opts.tail_be32) == (T - 2, None)
    # the usable layout rides in the options struct, the tail over the committed columns only
    eng._lib.calls.clear()
    eng.commit_expr(_sets(eng, 1), [([(ONE, [0])],), ([(ONE, [0])], True)], T - 2, [S] * 2)
    opts = eng._lib.calls[0][1][5]._obj
    assert (opts.usable, opts.tail_be32) == (T - 2, S * 2)
    out, _, _ = eng.commit_expr([100, 101], [([(ONE, [1])],)])
    assert (out.i, out.T) == (None, None)


GOOD = [(ONE, [0])]
BAD = {
    "no exprs": lambda h: (h(1), []),
    "exprs not a list": lambda h: (h(1), None),
    "17 exprs": lambda h: (h(1), [(GOOD,)] * 17),
    "an entry that is no tuple": lambda h: (h(1), [GOOD[0]]),
    "an entry of three": lambda h: (h(1), [(GOOD, True, 1)]),
    "a check flag that is no bool": lambda h: (h(1), [(GOOD, 1)]),
    "no terms": lambda h: (h(1), [([],)]),
    "17 terms": lambda h: (h(1), [(GOOD * 17,)]),
    "9 factors": lambda h: (h(1), [([(ONE, [0] * 9)],)]),
    "a short coefficient": lambda h: (h(1), [([(ONE[:31], [0])],)]),
    "a negative row": lambda h: (h(1), [([(ONE, [-1])],)]),
    "a row that is no integer": lambda h: (h(1), [([(ONE, ["a"])],)]),
    "a factor of three": lambda h: (h(1), [([(ONE, [(0, 1, 2)])],)]),
    "a rotation beyond int32": lambda h: (h(1), [([(ONE, [(0, 2 ** 31)])],)]),
    "a term that is no pair": lambda h: (h(1), [([ONE],)]),
    "a tail without usable": lambda h: (h(1), [(GOOD,)], None, [S]),
    "usable 0": lambda h: (h(1), [(GOOD,)], 0),
    "a short tail scalar": lambda h: (h(1), [(GOOD,)], T - 1, [S[:31]]),
    "a tail of the wrong length": lambda h: (h(1), [(GOOD,), (GOOD,)], T - 1, [S]),
    "a tail for checks alone": lambda h: (h(1), [(GOOD, True)], T - 1, [S]),
    "usable over bare handles": lambda h: ([100], [(GOOD,)], T - 1, [S]),
    "no handles": lambda h: ([], [(GOOD,)]),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_a_bad_shape_is_refused_under_the_method_s_name_before_any_native_call(eng, case):
    with pytest.raises(_native.KzgError) as err:
        eng.commit_expr(*BAD[case](lambda n: _sets(eng, n)))
    assert err.value.code == _native.KZG_E_ARG
    assert str(err.value).split(": ", 1)[1].startswith("commit_expr"), str(err.value)
    assert eng._lib.calls == [], "a bad shape must be refused before any native call"


class _Engine:
    """an engine that records commit_expr and answers a set of two rows, or none"""

    def __init__(self):
        self.calls = []

    def commit_expr(self, hs, recs, usable, tb):
        self.calls.append((hs, recs, usable, tb))
        n_out = sum(1 for _, chk in recs if not chk)
        rs = RowSet(self, 77, 0, n_out, T, [bytes(48)] * n_out) if n_out else None
        return rs, [0] * len(recs), [None] * len(recs)


def test_client_turns_the_wire_form_into_the_engine_s_and_refuses_malformed_input():
    cl = Client.__new__(Client)
    cl.engine = _Engine()
    one = codec.be32_to_fr(ONE)
    r = cl.worker_commit_expr([5], [[[[one, [0, [1, -1]]]]], [[[one, []]], True]])
    assert r.status_code == 200, r.json()
    assert r.json()["handle"] == 77 and len(r.json()["commitments"]) == 1
    assert r.json()["nonzero"] == [0, 0] and r.json()["first"] == [None, None]
    hs, recs, usable, tb = cl.engine.calls[0]
    assert hs == [5] and usable is None and tb == []
    assert recs == [([(ONE, [(0, 0), (1, -1)])], False), ([(ONE, [])], True)]
    r = cl.worker_commit_expr([5], [[[[one, [0]]], True]])
    assert r.status_code == 200 and r.json()["handle"] is None and r.json()["commitments"] == []
    n = len(cl.engine.calls)
    big = codec.be32_to_fr(R.to_bytes(32, "big"))                   # a coefficient that is not canonical
    for bad in ([], None, [[]], ["x"], [[[[one, [0]]], 1]], [[[[one, [0]]], True, 2]], [[[[one, [[0, 1, 2]]]]]], [[[[one]]]],
                [[[["zz", [0]]]]], [[[[big, [0]]]]]):
        assert cl.worker_commit_expr([5], bad).status_code == 400, bad
    assert cl.worker_commit_expr([5], [[[[one, [0]]]]], None, [one]).status_code == 400      # a tail without usable
    assert cl.worker_commit_expr([5], [[[[one, [0]]]]], 0, []).status_code == 400
    assert cl.worker_commit_expr([], [[[[one, [0]]]]]).status_code == 400
    assert len(cl.engine.calls) == n, "malformed input must not reach the engine"
