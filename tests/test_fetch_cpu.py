"""CPU checks around kzg_rows_commit_fetch: the Python reference (tests/fetch_ref.py) against hand-made cases, the engine's
dispatch over a recording stub library, and the header's declarations.  No device."""
import ctypes
import os
import random
import re

import pytest

from tests import fetch_ref as fref
from tests.gpu_common import R
from zkp_subnet_amd import _native
from zkp_subnet_amd.engine import HipEngine, RowSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 8
S = bytes(31) + b"\x01"


# ---------------------------------------------------------------------------------------------------- the reference
def test_xor_table_by_two_keys():
    a = [0, 1, 2, 3, 0, 1, 2, 3]
    b = [0, 0, 0, 0, 1, 1, 1, 1]
    table = [a, b, [x ^ y for x, y in zip(a, b)]]
    ina, inb = [3, 3, 0, 1, 2, 2, 1, 0], [1, 0, 0, 1, 1, 0, 2, 0]       # (1, 2) at cell 6 is no table row
    out, missing, first = fref.fetched_columns([ina, inb], table, 1, 2)
    assert out == [[2, 3, 0, 0, 3, 2, 0, 0]] and missing == [1] and first == [6]
    out, missing, first = fref.fetched_columns([ina, inb], table, 1, 2, with_index=True)
    assert out[0] == [7, 3, 0, 5, 6, 2, 0, 0] and out[1] == [2, 3, 0, 0, 3, 2, 0, 0]
    # two reads, read-major: the second one has no miss
    out, missing, first = fref.fetched_columns([ina, inb, a, b], table, 2, 2)
    assert out[1] == table[2] and missing == [1, 0] and first == [6, None]
    assert fref.n_out(3, 2, 2) == 2 and fref.n_out(3, 2, 2, True) == 4 and fref.n_out(16, 1, 0) == 16


def test_the_first_copy_of_a_repeated_key_answers():
    table = [[5, 7, 5, 9, 7, 5, 0, 5], [10, 11, 12, 13, 14, 15, 16, 17]]
    out, missing, first = fref.fetched_columns([[5, 7, 9, 0, 5, 7, 1, 5]], table, 1, 1, with_index=True)
    assert out == [[0, 1, 3, 6, 0, 1, 0, 0], [10, 11, 13, 16, 10, 11, 0, 10]]
    assert missing == [1] and first == [6]
    assert fref.first_rows(table, 1, 8) == {(5,): 0, (7,): 1, (9,): 3, (0,): 6}
    assert fref.first_rows(table, 1, 2) == {(5,): 0, (7,): 1}


def test_a_payload_of_zero_on_a_hit_differs_from_a_miss_only_in_the_count():
    table = [[1, 2, 3, 4], [0, 0, 9, 9]]
    assert fref.fetched_columns([[1, 2, 1, 2]], table, 1, 1) == ([[0, 0, 0, 0]], [0], [None])
    assert fref.fetched_columns([[5, 6, 5, 6]], table, 1, 1) == ([[0, 0, 0, 0]], [4], [0])


def test_keys_that_differ_in_the_last_column_only():
    table = [[1, 1, 1, 1], [2, 2, 2, 2], [0, 1, 2, R - 1], [40, 41, 42, 43]]
    ins = [[1] * 4, [2] * 4, [R - 1, 2, 1, 3]]
    assert fref.fetched_columns(ins, table, 1, 3) == ([[43, 42, 41, 0]], [1], [3])


def test_by_index_compares_the_whole_integer():
    rows = 8
    table = [list(range(100, 108)), list(range(200, 208))]
    addr = [0, rows - 1, rows, (1 << 32) + 3, 1 << 64, R - 1, 3, 3]
    out, missing, first = fref.fetched_columns([addr], table, 1, 0)
    assert out == [[100, 107, 0, 0, 0, 0, 103, 103], [200, 207, 0, 0, 0, 0, 203, 203]]
    assert missing == [4] and first == [2]
    # under `usable` the addressable rows end there
    u = 6
    tail = list(range(1000, 1000 + 2 * (rows - u)))
    out, missing, first = fref.fetched_columns([[5, 6, 7, u - 1, u, 0, 0, 0]], table, 1, 0, usable=u, tail=tail)
    assert out == [[105, 0, 0, 105, 0, 100, 1000, 1001], [205, 0, 0, 205, 0, 200, 1002, 1003]]
    assert missing == [3] and first == [1]
    # a permutation read through its inverse is the identity
    rnd = random.Random(1)
    perm = list(range(rows))
    rnd.shuffle(perm)
    inv = [perm.index(q) for q in range(rows)]
    assert fref.fetched_columns([inv], [perm], 1, 0) == ([list(range(rows))], [0], [None])


def test_layout_reads_and_matches_nothing_behind_usable():
    u = 5
    table = [[1, 2, 3, 4, 5, 6, 7, 8], [11, 12, 13, 14, 15, 16, 17, 18]]
    ins = [[6, 1, 5, 7, 2, 1, 1, 1]]                     # 6 and 7 stand in the table, but behind `usable`
    tail = list(range(500, 500 + 2 * (T - u)))
    out, missing, first = fref.fetched_columns(ins, table, 1, 1, True, u, tail)
    assert out == [[0, 0, 4, 0, 1, 500, 501, 502], [0, 11, 15, 0, 12, 503, 504, 505]]
    assert missing == [2] and first == [0]
    plain, pm, _ = fref.fetched_columns(ins, table, 1, 1, True)
    assert pm == [0] and plain[1][:u] == [16, 11, 15, 17, 12]
    with pytest.raises(AssertionError):
        fref.fetched_columns(ins, table, 1, 1, True, u, tail[:-1])


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
    e._lib, e._h, e._set_len, e._set_rows, e.verifier = _Recorder(), ctypes.c_void_p(1), {}, {}, None
    return e


def _sets(e, n, first=1, k=1):
    return [RowSet(e, first + j, 3, k, T, [bytes(48)] * k) for j in range(n)]


def test_a_good_call_reaches_exactly_the_export_of_its_own_name(eng):
    ins, tab = _sets(eng, 2), _sets(eng, 1, first=10, k=3)
    rset, missing, first = eng.commit_fetch(ins, tab, 1, 2)
    assert [name for name, _ in eng._lib.calls] == ["kzg_rows_commit_fetch"]
    args = eng._lib.calls[0][1]
    assert len(args) == len(_native.SYMBOLS["kzg_rows_commit_fetch"][1])
    assert (args[1], args[3], args[5], args[6], args[7], args[8]) == (2, 1, 1, 2, 0, None)
    assert (rset.k, rset.i, rset.T, len(rset.commitments)) == (1, 3, T, 1)
    assert missing == [0] and first == [0]                 # (the stub leaves the zeros of the buffers)
    # the index flag, the usable layout in the options struct, and bare handles of sets this engine made
    eng._lib.calls.clear()
    u = T - 2
    s1 = b"\x01" * 32                          # (no zero byte: the field reads back as a C string)
    rset, _, _ = eng.commit_fetch([1, 2, 1, 2], [10], 2, 2, True, u, [s1] * (4 * 2))
    args = eng._lib.calls[0][1]
    assert (args[1], args[5], args[6], args[7]) == (4, 2, 2, _native.KZG_FETCH_INDEX)
    assert (args[8]._obj.usable, args[8]._obj.tail_be32) == (u, s1 * 8)
    assert (rset.k, rset.i, rset.T) == (4, 3, T)
    # by row index: every table row is payload
    rset, _, _ = eng.commit_fetch(ins[:1], tab, 1, 0)
    assert rset.k == 3
    # a released set's row count is forgotten with its length
    tab[0].release()
    assert 10 not in eng._set_rows and 10 not in eng._set_len


def test_first_missing_none_is_the_header_s_sentinel(eng):
    class _Lib(_Recorder):
        def kzg_rows_commit_fetch(self, *args):
            args[10][0], args[11][0] = 2, 5
            args[10][1], args[11][1] = 0, _native.KZG_FETCH_NONE
            return _native.KZG_OK

    eng._lib = _Lib()
    _, missing, first = eng.commit_fetch(_sets(eng, 2), _sets(eng, 1, first=10, k=2), 2, 1)
    assert missing == [2, 0] and first == [5, None]


BAD = {
    "no reads": lambda h, t: (h(1), t(2), 0, 1),
    "a negative key count": lambda h, t: (h(1), t(2), 1, -1),
    "n_reads that is no integer": lambda h, t: (h(1), t(2), "1", 1),
    "n_keys that is a bool": lambda h, t: (h(1), t(2), 1, True),
    "with_index that is no bool": lambda h, t: (h(1), t(2), 1, 1, 1),
    "17 input rows": lambda h, t: (h(1), t(2), 9, 2),
    "more keys than table rows": lambda h, t: (h(1), t(2), 1, 3),
    "nothing to output": lambda h, t: (h(1), t(2), 1, 2),
    "the index by row index": lambda h, t: (h(1), t(2), 1, 0, True),
    "17 output rows": lambda h, t: (h(1), t(9), 2, 0),
    "32 output rows with the index": lambda h, t: (h(2), t(16), 2, 1, True),
    "a table of unknown width": lambda h, t: (h(1), [100], 1, 1),
    "a tail without usable": lambda h, t: (h(1), t(2), 1, 1, False, None, [S]),
    "usable 0": lambda h, t: (h(1), t(2), 1, 1, False, 0),
    "a short tail scalar": lambda h, t: (h(1), t(2), 1, 1, False, T - 1, [S[:31]]),
    "a tail of the wrong length": lambda h, t: (h(1), t(2), 1, 1, True, T - 1, [S]),
    "no input handles": lambda h, t: ([], t(2), 1, 1),
    "no table handles": lambda h, t: (h(1), [], 1, 1),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_a_bad_shape_is_refused_under_the_method_s_name_before_any_native_call(eng, case):
    with pytest.raises(_native.KzgError) as err:
        eng.commit_fetch(*BAD[case](lambda n: _sets(eng, n), lambda k: _sets(eng, 1, first=50, k=k)))
    assert err.value.code == _native.KZG_E_ARG
    assert str(err.value).split(": ", 1)[1].startswith("commit_fetch"), str(err.value)
    assert eng._lib.calls == [], "a bad shape must be refused before any native call"


def test_the_text_client_refuses_malformed_arguments_before_the_engine():
    from zkp_subnet_amd import Client

    class _Engine:
        def __getattr__(self, name):
            raise AssertionError(f"the engine was reached: {name}")

    client = Client.__new__(Client)
    client.engine = _Engine()
    for args in (([1], [2], 0, 1), ([1], [2], 1, -1), ([1], [2], "1", 1), ([1], [2], 1, 0, True), ([1], [2], 9, 2),
                 ([1], [2], 1, 1, "yes"), ([], [2], 1, 1), ([1], ["x"], 1, 1), ([1], [2], 1, 1, False, None, ["1"]),
                 ([1], [2], 1, 1, False, 0, []), ([1], [2], 1, 1, False, 3, [str(R)])):
        r = client.worker_commit_fetch(*args)
        assert r.status_code == 400 and "error" in r.json(), args


# ---------------------------------------------------------------------------------------------------- the header
def test_header_declares_the_symbols_and_the_constants():
    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in ("kzg_rows_commit_fetch", "kzg_multi_rows_commit_fetch"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _native.SYMBOLS
    assert len(_native.SYMBOLS["kzg_multi_rows_commit_fetch"][1]) == len(_native.SYMBOLS["kzg_rows_commit_fetch"][1]) + 1
    assert re.search(r"#define\s+KZG_FETCH_INDEX\s+1u", hdr) and _native.KZG_FETCH_INDEX == 1
    assert re.search(r"#define\s+KZG_FETCH_NONE\s+0xffffffffffffffffull", hdr) and _native.KZG_FETCH_NONE == (1 << 64) - 1
    assert "returning the permutation" not in hdr
    block = hdr[hdr.index("THE FETCHED COLUMNS"):hdr.index("#define KZG_FETCH_INDEX")]
    for word in ("OUT OF SCOPE", "SOUNDNESS", "WORKSPACE", '"fetch:"'):
        assert word in block, word
