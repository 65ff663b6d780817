"""CPU tests of the typed columns: the reference itself at the extreme values (tests/typed_ref.py), and every argument check of
the Python layers that needs no device -- the buffer formats taken, the shapes refused, the calls a good request reaches."""
import array
import ctypes
import os
import re

import numpy as np
import pytest

from oracle.bls12_381 import R
from tests import typed_ref as tr
from zkp_subnet_amd import _native
from zkp_subnet_amd.engine import HipEngine, RowSet, typed_column

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KINDS = ["u8", "u16", "u32", "u64", "i32", "i64"]


# ---------------------------------------------------------------------------------------------------- the reference
def test_extreme_values_map_to_the_residues_the_issue_pins():
    assert tr.residues("u8", [0, 255]) == [0, 255]
    assert tr.residues("u16", [65535]) == [65535]
    assert tr.residues("u32", [2**32 - 1]) == [2**32 - 1]
    assert tr.residues("u64", [2**64 - 1]) == [2**64 - 1]
    assert tr.residues("i32", [-1, 2**31 - 1, -2**31]) == [R - 1, 2**31 - 1, R - 2**31]
    assert tr.residues("i64", [-1, 2**63 - 1, -2**63]) == [R - 1, 2**63 - 1, R - 2**63]
    assert tr.residues("fr", [0, R - 1]) == [0, R - 1]


def test_fill_and_empty_columns():
    assert tr.residues("u8", [], 4) == [0, 0, 0, 0]
    assert tr.residues("u8", [], 3, R - 1) == [R - 1] * 3
    assert tr.residues("i32", [-5], 3, 7) == [R - 5, 7, 7]
    assert tr.be32_row([1, R - 1]) == (1).to_bytes(32, "big") + (R - 1).to_bytes(32, "big")


@pytest.mark.parametrize("kind", INT_KINDS)
def test_pack_residues_narrow_round_trip_at_the_extremes(kind):
    cells = tr.extremes(kind)
    raw = tr.pack(kind, cells)
    assert len(raw) == len(cells) * tr.KINDS[kind][0] and tr.unpack(kind, raw) == cells
    assert tr.narrow(kind, tr.residues(kind, cells)) == (cells, 0, None)


def test_narrow_counts_what_does_not_fit_and_writes_zero():
    vals = list(range(1 << 12))
    cells, n, first = tr.narrow("u8", vals)
    assert (n, first) == ((1 << 12) - 256, 256) and cells[:256] == vals[:256] and set(cells[256:]) == {0}
    assert tr.narrow("i32", [R - 1]) == ([-1], 0, None)
    assert tr.narrow("i32", [R - 2**31]) == ([-2**31], 0, None)
    assert tr.narrow("i32", [R - 2**31 - 1, 5, 2**31]) == ([0, 5, 0], 2, 0)
    assert tr.narrow("i64", [R - 2**63, 2**63 - 1, 2**63]) == ([-2**63, 2**63 - 1, 0], 1, 2)
    assert tr.narrow("u64", [2**64 - 1, 2**64, R - 1]) == ([2**64 - 1, 0, 0], 2, 1)
    assert tr.narrow("fr", [R - 1, 0]) == ([R - 1, 0], 0, None)


# ---------------------------------------------------------------------------------------------------- buffers
@pytest.mark.parametrize("dtype, kind", [(np.uint8, _native.KZG_COL_U8), (np.uint16, _native.KZG_COL_U16),
                                         (np.uint32, _native.KZG_COL_U32), (np.uint64, _native.KZG_COL_U64),
                                         (np.int32, _native.KZG_COL_I32), (np.int64, _native.KZG_COL_I64)])
def test_numpy_dtypes_map_to_their_kinds(dtype, kind):
    a = np.arange(5, dtype=dtype)
    k, n, mv, fill = typed_column(a)
    assert (k, n, mv.nbytes, fill) == (kind, 5, 5 * a.itemsize, None)
    assert typed_column((a, bytes(32)))[3] == bytes(32)


def test_array_array_and_bytes_columns():
    for code, kind in (("B", _native.KZG_COL_U8), ("H", _native.KZG_COL_U16), ("I", _native.KZG_COL_U32),
                       ("Q", _native.KZG_COL_U64), ("i", _native.KZG_COL_I32), ("q", _native.KZG_COL_I64)):
        assert typed_column(array.array(code, [1, 2, 3]))[:2] == (kind, 3)
    assert typed_column(array.array("L", [1]))[0] == _native.KZG_COL_U64 and array.array("L").itemsize == 8
    assert typed_column(bytes(64))[:2] == (_native.KZG_COL_BE32, 2)
    assert typed_column(bytearray(32))[:2] == (_native.KZG_COL_BE32, 1)
    assert typed_column(b"")[:2] == (_native.KZG_COL_BE32, 0)
    assert typed_column(memoryview(bytes(3)))[:2] == (_native.KZG_COL_U8, 3)     # a view is a buffer, not a be32 row


BAD_COLUMNS = {
    "a strided view": lambda: np.arange(8, dtype=np.uint32)[::2],
    "two dimensions": lambda: np.zeros((2, 2), dtype=np.uint8),
    "int8": lambda: np.zeros(4, dtype=np.int8),
    "int16": lambda: np.zeros(4, dtype=np.int16),
    "float32": lambda: np.zeros(4, dtype=np.float32),
    "big-endian": lambda: np.zeros(4, dtype=">u4"),
    "a list": lambda: [1, 2, 3],
    "bytes of no whole cell": lambda: bytes(33),
    "a short fill": lambda: (np.zeros(4, dtype=np.uint8), bytes(31)),
    "a fill that is no bytes": lambda: (np.zeros(4, dtype=np.uint8), 0),
}


@pytest.mark.parametrize("case", sorted(BAD_COLUMNS))
def test_unusable_columns_are_refused(case):
    with pytest.raises(_native.KzgError) as err:
        typed_column(BAD_COLUMNS[case]())
    assert err.value.code == _native.KZG_E_ARG and "commit_rows_typed" in str(err.value)


# ---------------------------------------------------------------------------------------------------- the engine's checks
class _Recorder:
    """stands in for the loaded library: records the calls, answers KZG_OK"""

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


def test_a_good_commit_reaches_the_export_with_the_columns_in_place(eng):
    a = np.array([1, 2, 3], dtype=np.uint32)
    b = array.array("B", [7, 8])
    fill = b"\x01" * 32                        # (no zero byte: the field reads back as a C string)
    rs = eng.commit_rows_typed(3, [a, (b, fill), bytes(32 * 4)])
    (name, args), = eng._lib.calls
    assert name == "kzg_rows_commit_typed" and len(args) == len(_native.SYMBOLS[name][1])
    assert (args[1], args[2], args[4], args[5]) == (3, 3, 4, 1)          # T: the longest column
    cols = args[3]
    assert [(c.count, c.kind) for c in cols] == [(3, _native.KZG_COL_U32), (2, _native.KZG_COL_U8), (4, _native.KZG_COL_BE32)]
    assert cols[0].data == a.ctypes.data and cols[1].data == b.buffer_info()[0]       # nothing was copied
    assert cols[0].fill_be32 is None and cols[1].fill_be32 == fill
    assert (rs.k, rs.i, rs.T, len(rs.commitments)) == (3, 3, 4, 3)
    eng._lib.calls.clear()
    ro = np.arange(4, dtype=np.uint16)
    ro.setflags(write=False)
    rs = eng.commit_rows_typed(0, [ro, np.zeros(0, dtype=np.int64)], False, T=6)      # a read-only and an empty column
    args = eng._lib.calls[0][1]
    assert (args[2], args[4], args[5]) == (2, 6, 0) and args[3][1].data is None and rs.T == 6
    # a read-only window of a larger bytes object: the cells handed over are the window's, not the object's first ones
    eng._lib.calls.clear()
    whole = bytes(range(1, 41))
    eng.commit_rows_typed(0, [memoryview(whole)[2:6], memoryview(whole)[8:].cast("I"), memoryview(whole), whole[:32]])
    cols = eng._lib.calls[0][1][3]
    assert [(c.count, c.kind) for c in cols] == [(4, _native.KZG_COL_U8), (8, _native.KZG_COL_U32), (40, _native.KZG_COL_U8),
                                                 (1, _native.KZG_COL_BE32)]
    assert ctypes.string_at(cols[0].data, 4) == whole[2:6] and ctypes.string_at(cols[1].data, 32) == whole[8:]
    assert ctypes.string_at(cols[2].data, 40) == whole and ctypes.string_at(cols[3].data, 32) == whole[:32]
    ro = np.arange(10, dtype=np.uint32)
    ro.setflags(write=False)
    eng._lib.calls.clear()
    eng.commit_rows_typed(0, [ro[3:7]])
    assert ctypes.string_at(eng._lib.calls[0][1][3][0].data, 16) == ro[3:7].tobytes()


BAD_COMMITS = {
    "k = 0": lambda: ([],),
    "k = 17": lambda: ([np.zeros(2, dtype=np.uint8)] * 17,),
    "a column longer than T": lambda: ([np.zeros(2, dtype=np.uint8), np.zeros(5, dtype=np.uint8)], True, 4),
    "T = 0": lambda: ([np.zeros(0, dtype=np.uint8)],),
    "T that is no integer": lambda: ([np.zeros(2, dtype=np.uint8)], True, 2.0),
    "a column that is no buffer": lambda: ([np.zeros(2, dtype=np.uint8), None],),
}


@pytest.mark.parametrize("case", sorted(BAD_COMMITS))
def test_a_bad_commit_is_refused_before_any_native_call(eng, case):
    with pytest.raises(_native.KzgError) as err:
        eng.commit_rows_typed(0, *BAD_COMMITS[case]())
    assert err.value.code == _native.KZG_E_ARG and "commit_rows_typed" in str(err.value)
    assert eng._lib.calls == []


def test_a_good_read_reaches_the_export_and_decodes_the_sentinel(eng):
    class _Lib(_Recorder):
        def kzg_rows_read(self, *args):
            self.calls.append(("kzg_rows_read", args))
            ctypes.memmove(args[8], b"\x01\x00\x02\x00", 4)
            args[9][0], args[9][1] = (0, _native.KZG_READ_NONE) if len(self.calls) == 1 else (3, 9)
            return _native.KZG_OK

    eng._lib = _Lib()
    rs = RowSet(eng, 5, 0, 2, 16, [bytes(48)] * 2)
    assert eng.read_rows([rs], 1, 4, 2, "u16") == (b"\x01\x00\x02\x00", 0, None)
    args = eng._lib.calls[0][1]
    assert len(args) == len(_native.SYMBOLS["kzg_rows_read"][1])
    assert (args[1], args[3], args[4], args[5], args[6], args[7]) == (1, 1, 4, 2, _native.KZG_COL_U16, 1)
    assert eng.read_rows([5], 0, 0, 2, _native.KZG_COL_U16, False)[1:] == (3, 9)
    assert eng._lib.calls[1][1][7] == 0


@pytest.mark.parametrize("args", [(0, 0, 1, "u128"), (0, 0, 1, 7), (0, 0, 1, True), (-1, 0, 1, "u8"), (16, 0, 1, "u8"),
                                  (0, -1, 1, "u8"), (0, 0, 1 << 64, "u8"), (0, 0, 1.0, "u8"), (0, 16, 1, "u8"),
                                  (0, (1 << 64) - 1, 2, "u8")])
def test_a_bad_read_is_refused_before_any_native_call(eng, args):
    rs = RowSet(eng, 5, 0, 2, 16, [bytes(48)] * 2)
    with pytest.raises(_native.KzgError) as err:
        eng.read_rows([rs], *args)
    assert err.value.code == _native.KZG_E_ARG and "read_rows" in str(err.value) and eng._lib.calls == []
    with pytest.raises(_native.KzgError):
        eng.read_rows([], 0, 0, 1, "u8")


def test_a_count_no_row_can_hold_is_e_arg_for_a_handle_this_engine_does_not_know(eng):
    for count in ((1 << 64) - 1, 1 << 62, (1 << 32) + 1):
        with pytest.raises(_native.KzgError) as err:
            eng.read_rows([77], 0, 0, count, "fr")
        assert err.value.code == _native.KZG_E_ARG and eng._lib.calls == []


# ---------------------------------------------------------------------------------------------------- the text client
class _Engine:
    """the engine a Client drives, recording what reaches it"""

    def __init__(self):
        self.calls = []

    def commit_rows_typed(self, i, cols, ef, T):
        self.calls.append(("commit", i, cols, ef, T))
        return RowSet(object(), 9, i, len(cols), T, [bytes(48)] * len(cols))

    def read_rows(self, hs, row, first, count, kind, ef):
        self.calls.append(("read", hs, row, first, count, kind, ef))
        width, signed = _native.COL_KINDS[kind]
        if kind == _native.KZG_COL_BE32:
            return tr.be32_row([R - 1, 2][:count]), 0, None
        return tr.pack({(4, True): "i32", (1, False): "u8"}[(width, signed)], [-1, 2][:count]
                       if signed else [255, 2][:count]), 1, 1


@pytest.fixture
def client():
    from zkp_subnet_amd import Client

    c = Client.__new__(Client)
    c.engine, c._slice = _Engine(), lambda i: i
    return c


def test_the_client_mixes_wire_strings_with_typed_columns(client):
    from zkp_subnet_amd import codec

    a = np.array([1, 2, 3, 4], dtype=np.uint8)
    wire = codec.be32_to_fr_list(tr.be32_row([5, R - 1]))
    r = client.worker_commit_rows_typed(2, [a, wire], [None, wire[1]])
    assert r.status_code == 200 and r.json()["handle"] == 9 and len(r.json()["commitments"]) == 2
    (_, i, cols, ef, T), = client.engine.calls
    assert (i, ef, T) == (2, True, None) and cols[0][0] is a and cols[0][1] is None
    assert cols[1] == (tr.be32_row([5, R - 1]), (R - 1).to_bytes(32, "big"))
    for bad in (([],), ([a] * 17,), ([a], [None, None]), ([a], None, 0), ([["!"]],), ([a], [str(R)])):
        assert client.worker_commit_rows_typed(0, *bad).status_code == 400, bad
    assert len(client.engine.calls) == 1


def test_the_client_returns_integers_or_wire_strings(client):
    from zkp_subnet_amd import codec

    r = client.worker_read_rows([9], 0, 3, 2, "i32")
    assert r.status_code == 200 and r.json() == {"cells": [-1, 2], "overflow": 1, "first_overflow": 1}
    assert client.engine.calls[-1] == ("read", [9], 0, 3, 2, _native.KZG_COL_I32, True)
    assert client.worker_read_rows([9], 0, 0, 2, "u8").json()["cells"] == [255, 2]
    r = client.worker_read_rows([9], 1, 0, 2).json()
    assert r["cells"] == codec.be32_to_fr_list(tr.be32_row([R - 1, 2])) and r["first_overflow"] is None
    n = len(client.engine.calls)
    for bad in (([9], 0, 0, 1, "u128"), ([9], 0, 0, 1, 3), ([9], -1, 0, 1, "u8"), ([9], 0, True, 1, "u8"), ([], 0, 0, 1, "u8"),
                (["x"], 0, 0, 1, "u8"), ([9], 0, 0, "1", "u8")):
        assert client.worker_read_rows(*bad).status_code == 400, bad
    assert len(client.engine.calls) == n
    assert sorted(_native.COL_DTYPES) == ["fr", "i32", "i64", "u16", "u32", "u64", "u8"]


def test_the_multi_device_client_routes_commits_by_worker_and_reads_by_owner():
    from zkp_subnet_amd.client import Response
    from zkp_subnet_amd.multi import MultiDeviceClient

    class _C:
        def __init__(self, tag):
            self.tag, self.calls = tag, []

        def worker_commit_rows_typed(self, i, columns, fills, T):
            self.calls.append(("commit", i))
            return Response(200, {"handle": 100 + self.tag, "commitments": []})

        def worker_read_rows(self, handles, row, first, count, dtype):
            self.calls.append(("read", list(handles), dtype))
            return Response(200, {"cells": [], "overflow": 0, "first_overflow": None})

    m = MultiDeviceClient.__new__(MultiDeviceClient)
    m.clients, m._row_owner = [_C(0), _C(1)], {}
    assert m.worker_commit_rows_typed(3, [b""]).status_code == 200 and m.clients[1].calls == [("commit", 3)]
    assert m.worker_read_rows([101], 0, 0, 0, "u8").status_code == 200 and m.clients[1].calls[-1] == ("read", [101], "u8")
    assert m.worker_read_rows([55], 0, 0, 0).status_code == 400 and m.clients[0].calls == []


# ---------------------------------------------------------------------------------------------------- the header
def test_header_declares_the_calls_the_kinds_and_the_struct():
    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in ("kzg_rows_commit_typed", "kzg_rows_read"):
        multi = name.replace("kzg_", "kzg_multi_")
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr) and re.search(r"\bint\s+" + multi + r"\s*\(", hdr)
        assert len(_native.SYMBOLS[multi][1]) == len(_native.SYMBOLS[name][1]) + (1 if name == "kzg_rows_read" else 0)
    kinds = re.search(r"enum\s*\{\s*KZG_COL_BE32\s*=\s*0([^}]*)\}", hdr).group(1)
    assert [w.strip() for w in kinds.split(",") if w.strip()] == ["KZG_COL_U8", "KZG_COL_U16", "KZG_COL_U32", "KZG_COL_U64",
                                                                   "KZG_COL_I32", "KZG_COL_I64"]
    assert (_native.KZG_COL_BE32, _native.KZG_COL_U8, _native.KZG_COL_I64) == (0, 1, 6)
    assert [f[0] for f in _native.Col._fields_] == ["data", "count", "kind", "fill_be32"] and ctypes.sizeof(_native.Col) == 32
