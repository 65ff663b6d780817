"""CPU checks around kzg_rows_commit_recurrence: the headers' declarations against the ctypes bindings, the methods of the three
Python layers, the Python reference (tests/recur_ref.py) against hand-computed cases, the engine's dispatch over a recording
stub library, the Python-side refusals, and the plan function of the scan (kzg_test_recur_plan_of, host only).  No device."""
import ctypes
import os
import re

import pytest

from tests import recur_ref as rref
from tests.gpu_common import R
from zkp_subnet_amd import _native, codec
from zkp_subnet_amd.client import Client
from zkp_subnet_amd.engine import HipEngine, RowSet, recur_plan_of
from zkp_subnet_amd.multi import MultiDeviceClient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 8
S = b"\x01" * 32                              # (no zero byte: a tail field reads back as a C string)
ONE = bytes(31) + b"\x01"


# ---------------------------------------------------------------------------------------------------- the headers
def _header(name="kzg_mi355x.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def _args(hdr, sym):
    decl = re.search(r"\bint\s+" + sym + r"\s*\((.*?)\);", hdr, re.S).group(1)
    return re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")


def test_header_declares_the_call_the_structs_and_points_the_two_old_sentences_at_it():
    hdr = _header()
    for name in ("kzg_rows_commit_recurrence", "kzg_multi_rows_commit_recurrence"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
    assert re.search(r"\}\s*kzg_recurrence;", hdr) and re.search(r"\}\s*kzg_recurrence_opts;", hdr)
    text = hdr[hdr.index("THE RECURRENCE COLUMNS"):hdr.index("typedef struct kzg_recurrence {")]
    for phrase in ("OUT OF SCOPE", "SOUNDNESS", "checked on the HOST", "second-order", "division", "boundary gate", "WORKSPACE",
                   '"recur:"'):
        assert phrase in text, phrase
    derived = hdr[hdr.index("THE DERIVED COLUMNS"):hdr.index("THE EXPRESSION COLUMNS")]
    expr = hdr[hdr.index("THE EXPRESSION COLUMNS"):hdr.index("#define KZG_MAX_EXPR_FACTORS")]
    for block in (derived, expr):
        scope = block.split("OUT OF SCOPE")[1].split("SOUNDNESS")[0]
        assert "running-sum decomposition" in scope and "kzg_rows_commit_recurrence" in scope


def test_native_binds_both_symbols_with_the_header_s_struct_layouts():
    hdr = _header()
    one, multi = _native.SYMBOLS["kzg_rows_commit_recurrence"], _native.SYMBOLS["kzg_multi_rows_commit_recurrence"]
    assert one[0] is ctypes.c_int and multi[0] is ctypes.c_int
    assert len(one[1]) == 9 and multi[1] == [one[1][0], ctypes.c_uint32] + one[1][1:]
    for sym, ctype in (("kzg_rows_commit_recurrence", one), ("kzg_multi_rows_commit_recurrence", multi)):
        assert len(_args(hdr, sym)) == len(ctype[1]), sym
    body = re.search(r"typedef struct kzg_recurrence \{(.*?)\} kzg_recurrence;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*\*?\s*(\w+);", body) == [("kzg_quotient_terms", "mul"), ("kzg_quotient_terms", "add"),
                                                         ("uint8_t", "start_be32")]
    assert [f for f, _ in _native.Recurrence._fields_] == ["mul", "add", "start_be32"]
    assert _native.Recurrence._fields_[0][1] is _native.QuotientTerms and _native.Recurrence._fields_[1][1] is _native.QuotientTerms
    assert ctypes.sizeof(_native.Recurrence) == 88 and _native.Recurrence.add.offset == 40 and _native.Recurrence.start_be32.offset == 80
    obody = re.search(r"typedef struct kzg_recurrence_opts \{(.*?)\} kzg_recurrence_opts;", hdr, re.S).group(1)
    obody = re.sub(r"/\*.*?\*/", "", obody, flags=re.S)
    assert re.findall(r"(\w+);", obody) == [f for f, _ in _native.RecurrenceOpts._fields_] == ["usable", "tail_be32"]
    assert ctypes.sizeof(_native.RecurrenceOpts) == 16


def test_the_plan_hooks_are_declared_in_their_own_header_bound_and_exported():
    hooks_hdr, test_hdr = _header("kzg_mi355x_recur_test.h"), _header("kzg_mi355x_test.h")
    assert '#include "kzg_mi355x_recur_test.h"' in test_hdr
    declared = set(re.findall(r"\bint\s+(kzg_[a-z0-9_]+)\s*\(", hooks_hdr))
    assert declared == set(_native.RECUR_HOOKS) == {"kzg_test_recur_plan_of", "kzg_test_recur_run"}
    lib = _native.load()
    for sym, (res, args) in _native.RECUR_HOOKS.items():
        assert res is ctypes.c_int and len(_args(hooks_hdr, sym)) == len(args), sym
        assert getattr(lib, sym).argtypes == args
    assert not (declared & set(_native.SYMBOLS)) and "kzg_test_" not in _header()


def test_the_three_python_layers_have_the_methods():
    assert callable(getattr(HipEngine, "commit_recurrence"))
    assert callable(getattr(Client, "worker_commit_recurrence"))
    assert callable(getattr(MultiDeviceClient, "worker_commit_recurrence"))


def test_the_translation_unit_is_built_and_listed():
    from zkp_subnet_amd import build
    assert "fr_recur.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "fr_recur.hip"))
    assert "fr_recur.hip" in open(os.path.join(build.CSRC, "ctx.hip.h")).read().split("#pragma once")[0]


# ---------------------------------------------------------------------------------------------------- the reference
A = [3, 5, 7, 11, 13, 17, 19, 23]
B = [2, 0, R - 1, 4, 1, 0, 6, 9]


def test_reference_running_sum_and_running_product():
    rows, closings = rref.recurrence_columns([A], [([], [(1, [0])], 10), ([(1, [0])], [], 2)])
    assert rows[0] == [10, 13, 18, 25, 36, 49, 66, 85] and closings[0] == 108
    assert rows[1] == [2, 6, 30, 210, 2310, 30030, 510510, 9699690] and closings[1] == 223092870
    assert rref.recurrence_columns([B], [([], [(1, [0])], 0)]) == ([[0, 2, 2, 1, 5, 6, 6, 12]], [21])   # r - 1 is -1
    with pytest.raises(AssertionError):
        rref.recurrence_columns([A], [([], [], 1)])


def test_reference_horner_is_a_polynomial_evaluation():
    x = 1000003
    rows, closings = rref.recurrence_columns([A], [([(x, [])], [(1, [0])], 0)])
    # acc' = acc x + a[t]: after n steps the polynomial with coefficients a[0] .. a[n - 1], highest first
    for n in range(T + 1):
        want = sum(a * pow(x, n - 1 - j, R) for j, a in enumerate(A[:n])) % R
        assert (rows[0] + closings)[n] == want
    assert rows[0][:3] == [0, 3, 3 * x + 5]


def test_reference_restart_at_a_zero_multiplier():
    sel = [1, 1, 0, 1, 1, 1, 0, 1]
    rows, closings = rref.recurrence_columns([A, sel], [([(1, [1])], [(1, [0])], 100)])
    assert rows[0] == [100, 103, 108, 7, 18, 31, 48, 19] and closings == [42]
    # the value behind a zero multiplier is the addend, whatever stood before it
    other, _ = rref.recurrence_columns([A, sel], [([(1, [1])], [(1, [0])], 5)])
    assert other[0][3:] == rows[0][3:] and other[0][:3] != rows[0][:3]


def test_reference_both_layouts_closing_row_tail_and_rotations():
    u = 5
    recs = [([], [(1, [0])], 1), ([(1, [(1, 1)])], [(2, [])], 1)]
    plain, pc = rref.recurrence_columns([A, B], recs)
    assert plain[0] == [1, 4, 9, 16, 27, 40, 57, 76] and pc[0] == 99
    assert plain[1][:3] == [1, 2, (2 * (R - 1) + 2) % R] == [1, 2, 0]           # B rotated by one: 0, r - 1, 4, ..
    tail = [100, 101, 200, 201]
    rows, closings = rref.recurrence_columns([A, B], recs, u, tail)
    assert rows[0] == [1, 4, 9, 16, 27, 40, 100, 101] and closings[0] == 40    # row u is the closing row, the tail behind it
    assert rows[1][u] == closings[1] and rows[1][u + 1:] == [200, 201]           # column-major: column 1's tail second
    assert rows[1][:u + 1] == plain[1][:u + 1]                                  # the same steps, only fewer
    # a cell at or behind u is read only where a rotation lands on it: row u - 1 of recurrence 1 reads B[u]
    poisoned = [A[:u] + [R - 1] * (T - u), B[:u + 1] + [R - 1] * (T - u - 1)]
    assert rref.recurrence_columns(poisoned, recs, u, tail) == (rows, closings)
    moved = [A, B[:u] + [7] + B[u + 1:]]
    assert rref.recurrence_columns(moved, recs, u, tail)[1][1] != closings[1]
    for bad_u, bad_tail in ((u, tail[:-1]), (0, []), (T, [])):
        with pytest.raises(AssertionError):
            rref.recurrence_columns([A, B], recs, bad_u, bad_tail)


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
    recs = [([(ONE, [0, (1, -1)]), (S, [])], [(ONE, [1])], S), ([], [(S, [(0, 2 ** 31 - 1)])], ONE), ([(ONE, [0])], [], ONE)]
    rset, closings = eng.commit_recurrence(_sets(eng, 2), recs)
    assert [name for name, _ in eng._lib.calls] == ["kzg_rows_commit_recurrence"]
    args = eng._lib.calls[0][1]
    assert len(args) == len(_native.SYMBOLS["kzg_rows_commit_recurrence"][1])
    assert args[1] == 2 and args[3] == 3 and args[5] is None
    r0, r1, r2 = args[4][0], args[4][1], args[4][2]
    assert (r0.mul.n_terms, r0.add.n_terms, r1.mul.n_terms, r1.add.n_terms, r2.mul.n_terms, r2.add.n_terms) == (2, 1, 0, 1, 1, 0)
    assert list(r0.mul.term_lens[:2]) == [2, 0] and list(r0.mul.term_rows[:2]) == [0, 1] and list(r0.mul.term_rots[:2]) == [0, -1]
    assert r1.add.term_rots[0] == 2 ** 31 - 1 and not r1.mul.term_lens and r1.mul.coeffs_be32 is None
    assert r0.start_be32 == S
    assert (rset.k, rset.i, rset.T, len(rset.commitments)) == (3, 3, T, 3)
    assert closings == [bytes(32)] * 3                                          # (the stub writes nothing)
    # the usable layout rides in the options struct: T - usable - 1 tail scalars per recurrence, none at usable = T - 1
    eng._lib.calls.clear()
    eng.commit_recurrence(_sets(eng, 1), recs[:2], T - 3, [S] * 4)
    opts = eng._lib.calls[0][1][5]._obj
    assert (opts.usable, opts.tail_be32) == (T - 3, S * 4)
    eng._lib.calls.clear()
    eng.commit_recurrence(_sets(eng, 1), recs[:2], T - 1)
    opts = eng._lib.calls[0][1][5]._obj
    assert (opts.usable, opts.tail_be32) == (T - 1, None)
    out, _ = eng.commit_recurrence([100, 101], recs[2:])
    assert (out.i, out.T) == (None, None)


GOOD = ([(ONE, [0])], [(ONE, [1])], ONE)
BAD = {
    "no recs": lambda h: (h(1), []),
    "recs not a list": lambda h: (h(1), None),
    "17 recs": lambda h: (h(1), [GOOD] * 17),
    "an entry that is no tuple": lambda h: (h(1), [ONE]),
    "an entry of two": lambda h: (h(1), [GOOD[:2]]),
    "an entry of four": lambda h: (h(1), [GOOD + (1,)]),
    "a short start": lambda h: (h(1), [(GOOD[0], GOOD[1], ONE[:31])]),
    "a start that is no bytes": lambda h: (h(1), [(GOOD[0], GOOD[1], 1)]),
    "both expressions empty": lambda h: (h(1), [([], [], ONE)]),
    "17 terms": lambda h: (h(1), [(GOOD[0] * 17, [], ONE)]),
    "17 terms in add": lambda h: (h(1), [([], GOOD[1] * 17, ONE)]),
    "9 factors": lambda h: (h(1), [([(ONE, [0] * 9)], [], ONE)]),
    "a short coefficient": lambda h: (h(1), [([(ONE[:31], [0])], [], ONE)]),
    "a negative row": lambda h: (h(1), [([], [(ONE, [-1])], ONE)]),
    "a row that is no integer": lambda h: (h(1), [([(ONE, ["a"])], [], ONE)]),
    "a factor of three": lambda h: (h(1), [([(ONE, [(0, 1, 2)])], [], ONE)]),
    "a rotation beyond int32": lambda h: (h(1), [([(ONE, [(0, 2 ** 31)])], [], ONE)]),
    "a term that is no pair": lambda h: (h(1), [([ONE], [], ONE)]),
    "a tail without usable": lambda h: (h(1), [GOOD], None, [S]),
    "usable 0": lambda h: (h(1), [GOOD], 0),
    "a short tail scalar": lambda h: (h(1), [GOOD], T - 2, [S[:31]]),
    "a tail of the wrong length": lambda h: (h(1), [GOOD, GOOD], T - 2, [S]),
    "a tail at usable = T - 1": lambda h: (h(1), [GOOD], T - 1, [S]),
    "usable over bare handles": lambda h: ([100], [GOOD], T - 2, [S]),
    "no handles": lambda h: ([], [GOOD]),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_a_bad_shape_is_refused_under_the_method_s_name_before_any_native_call(eng, case):
    with pytest.raises(_native.KzgError) as err:
        eng.commit_recurrence(*BAD[case](lambda n: _sets(eng, n)))
    assert err.value.code == _native.KZG_E_ARG
    assert str(err.value).split(": ", 1)[1].startswith("commit_recurrence"), str(err.value)
    assert eng._lib.calls == [], "a bad shape must be refused before any native call"


class _Engine:
    """an engine that records commit_recurrence and answers a set of one row per recurrence"""

    def __init__(self):
        self.calls = []

    def commit_recurrence(self, hs, recs, usable, tb):
        self.calls.append((hs, recs, usable, tb))
        return RowSet(self, 77, 0, len(recs), T, [bytes(48)] * len(recs)), [ONE] * len(recs)


def test_client_turns_the_wire_form_into_the_engine_s_and_refuses_malformed_input():
    cl = Client.__new__(Client)
    cl.engine = _Engine()
    one = codec.be32_to_fr(ONE)
    r = cl.worker_commit_recurrence([5], [[[[one, [0, [1, -1]]]], [], one], [[], [[one, []]], one]])
    assert r.status_code == 200, r.json()
    assert r.json()["handle"] == 77 and len(r.json()["commitments"]) == 2 and r.json()["closings"] == [one, one]
    hs, recs, usable, tb = cl.engine.calls[0]
    assert hs == [5] and usable is None and tb == []
    assert recs == [([(ONE, [(0, 0), (1, -1)])], [], ONE), ([], [(ONE, [])], ONE)]
    r = cl.worker_commit_recurrence([5], [[[], [[one, [0]]], one]], T - 3, [one, one])
    assert r.status_code == 200 and cl.engine.calls[1][2:] == (T - 3, [ONE, ONE])
    n = len(cl.engine.calls)
    big = codec.be32_to_fr(R.to_bytes(32, "big"))                   # a scalar that is not canonical
    ok = [[one, [0]]]
    for bad in ([], None, [[]], ["x"], [[ok, ok]], [[ok, ok, one, 1]], [[[], [], one]], [[[[one, [[0, 1, 2]]]], [], one]], [[[[one]], [], one]],
                [[[["zz", [0]]], [], one]], [[[[big, [0]]], [], one]], [[[], [[big, []]], one]], [[ok, [], big]], [[ok, [], "zz"]]):
        assert cl.worker_commit_recurrence([5], bad).status_code == 400, bad
    assert cl.worker_commit_recurrence([5], [[ok, [], one]], None, [one]).status_code == 400      # a tail without usable
    assert cl.worker_commit_recurrence([5], [[ok, [], one]], 0, []).status_code == 400
    assert cl.worker_commit_recurrence([5], [[ok, [], one]], T - 3, [big]).status_code == 400
    assert cl.worker_commit_recurrence([], [[ok, [], one]]).status_code == 400
    assert len(cl.engine.calls) == n, "malformed input must not reach the engine"


# ---------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("n", [1, 4, 2048, 2049, 8192, 8193, 1 << 14, 1 << 17, 1 << 18, 1 << 20, (1 << 17) - 1, (1 << 18) - 1])
def test_the_library_s_plan(n):
    pl = recur_plan_of(n)
    assert pl == rref.plan(n)
    l0 = 2 if n < 1 << 17 else 3 if n < 1 << 18 else 4
    assert pl["n"][0] == n and pl["n"][-1] <= 2048 and all(m > 2048 for m in pl["n"][:-1])
    assert pl["l"][:-1] == ([l0] + [4] * (pl["K"] - 1))[:pl["K"]] and pl["l"][-1] == 0
    for k in range(pl["K"]):
        assert pl["n"][k + 1] == -(-pl["n"][k] // (1 << pl["l"][k]))
    # the stacked levels above level 0 lie one behind the other inside the scratch the library allocates
    assert pl["off"][:2] == [0, 0][:pl["K"] + 1]
    for k in range(1, pl["K"]):
        assert pl["off"][k + 1] == pl["off"][k] + pl["n"][k]
    if pl["K"]:
        assert pl["off"][-1] + pl["n"][-1] <= (n + 3) // 4 * 3 // 2 + 64


def test_the_library_s_plan_at_the_named_sizes():
    assert recur_plan_of(1)["K"] == 0 and recur_plan_of(4)["n"] == [4]
    assert recur_plan_of(8192) == {"K": 1, "l": [2, 0], "n": [8192, 2048], "off": [0, 0]}
    assert recur_plan_of(8193)["n"] == [8193, 2049, 129]
    assert recur_plan_of(1 << 14)["n"] == [1 << 14, 4096, 256]      # the smallest power of two with a level under the top
    assert recur_plan_of(1 << 13)["K"] == 1
    assert recur_plan_of(1 << 17)["l"] == [3, 4, 0] and recur_plan_of(1 << 18)["l"] == [4, 4, 0]
    assert recur_plan_of(1 << 20) == {"K": 3, "l": [4, 4, 4, 0], "n": [1 << 20, 1 << 16, 4096, 256], "off": [0, 0, 65536, 69632]}


def test_a_caller_s_plan_and_every_precondition_refusal():
    assert recur_plan_of(4096, 2, 16) == rref.plan(4096, 2, 16) == {"K": 3, "l": [2, 4, 4, 0], "n": [4096, 1024, 64, 4],
                                                                  "off": [0, 0, 1024, 1088]}
    assert recur_plan_of(4096, 4, 1)["n"] == [4096, 256, 16, 1] and recur_plan_of(5, 3, 2048)["K"] == 0
    for args, why in (((0, 2, 16), "no rows"), (((1 << 32) + 1, 2, 16), "2^32"), ((4096, 1, 16), "level-0 chunk"),
                      ((4096, 5, 16), "level-0 chunk"), ((4096, -1, 16), "level-0 chunk"), ((4096, 2, 0), "1 .. 2048"),
                      ((4096, 2, -1), "1 .. 2048"), ((4096, 2, 2049), "1 .. 2048")):
        with pytest.raises(_native.KzgError) as err:
            recur_plan_of(*args)
        assert err.value.code == _native.KZG_E_ARG and why in str(err.value), (args, str(err.value))
    lib = _native.load()
    K = ctypes.c_int(0)
    arr_l, arr_n = (ctypes.c_int * 16)(), (ctypes.c_uint64 * 16)()
    assert lib.kzg_test_recur_plan_of(4, -1, -1, ctypes.byref(K), arr_l, arr_n, None) == _native.KZG_E_ARG
    # the run hook judges the plan before it looks at the context: no device is needed to be refused
    assert lib.kzg_test_recur_run(None, 7, 16, None, None, None, 4, None, None) == _native.KZG_E_ARG
    assert b"level-0 chunk" in lib.kzg_last_error(None)
    assert lib.kzg_test_recur_run(None, -1, -1, None, None, None, 4, None, None) == _native.KZG_E_ARG
    assert b"no context" in lib.kzg_last_error(None)
