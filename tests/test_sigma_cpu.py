"""CPU checks around kzg_rows_commit_sigma and kzg_rows_check_copies: the Python reference (tests/sigma_ref.py) against its own
definition and the host grand-product reference, the engine's dispatch over a recording stub library, the text client's
refusals, and the header's declarations.  No device."""
import ctypes
import os
import random
import re

import pytest

from tests import grand_product_ref as gp
from tests import sigma_ref as sref
from tests.gpu_common import R
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import SigmaOpts
from zkp_subnet_amd.engine import HipEngine, RowSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 8
S = bytes(31) + b"\x01"
FREE = R - 1


def _labels(k, T_, seed, ids=None, free_every=0):
    rnd = random.Random(seed)
    ids = ids or max(1, k * T_ // 2)
    cols = [[rnd.randrange(ids) for _ in range(T_)] for _ in range(k)]
    if free_every:
        for c in range(k):
            for t in range(0, T_, free_every):
                cols[c][t] = FREE
    return cols


def _witness(labels, seed, usable=None, free_label=None):
    """wire values constant on the classes, random on the free cells and behind `usable`"""
    rnd = random.Random(seed)
    n = len(labels[0]) if usable is None else usable
    value = {}
    return [[rnd.randrange(R) if t >= n or lab == free_label else value.setdefault(lab, rnd.randrange(R))
             for t, lab in enumerate(col)] for col in labels]


# ---------------------------------------------------------------------------------------------------- the reference
def test_hand_made_classes_link_in_ascending_flat_index():
    #           t = 0  1  2  3
    labels = [[5, 9, 5, 7],          # flat 0 .. 3
              [9, 5, 8, 9]]          # flat 4 .. 7
    img, classes, fixed = sref.images(labels)
    assert img == [2, 4, 5, 3, 7, 0, 6, 1]      # 5: 0 -> 2 -> 5 -> 0; 9: 1 -> 4 -> 7 -> 1; 7 and 8 alone
    assert (classes, fixed) == (4, 2)
    assert sref.cycles(img) == [(0, 2, 5), (1, 4, 7), (3,), (6,)]
    # the free label: its cells stand alone and are no class
    img, classes, fixed = sref.images(labels, free_label=9)
    assert img == [2, 1, 5, 3, 4, 0, 6, 7] and (classes, fixed) == (3, 5)
    # usable = 2: rows 2 and 3 map to themselves and their labels join nothing
    img, classes, fixed = sref.images(labels, usable=2)
    assert img == [5, 4, 2, 3, 1, 0, 6, 7] and (classes, fixed) == (2, 0)
    shifts = [1, 7]
    cols, stats = sref.sigma_columns(labels, shifts, usable=2)
    dom = gp.domain(4)
    assert cols[0] == [7 * dom[1] % R, 7 * dom[0] % R, dom[2], dom[3]] and stats == {"classes": 2, "fixed": 0}


@pytest.mark.parametrize("k, T_, usable, free", [(1, 1, None, None), (1, 8, None, None), (3, 8, None, FREE), (3, 16, 11, FREE),
                                                 (4, 4, 1, None), (2, 8, 7, FREE), (16, 2, None, None)])
def test_sigma_is_a_permutation_of_the_identity_values_and_its_cycles_are_the_classes(k, T_, usable, free):
    labels = _labels(k, T_, 100 * k + T_, free_every=3 if free is not None else 0)
    shifts = [pow(7, c, R) for c in range(k)]
    cols, stats = sref.sigma_columns(labels, shifts, usable, free)
    dom = gp.domain(T_)
    ident = [shifts[c] * dom[t] % R for c in range(k) for t in range(T_)]
    assert len(set(ident)) == k * T_
    assert sorted(v for col in cols for v in col) == sorted(ident)
    n = T_ if usable is None else usable
    want = {}
    for c in range(k):
        for t in range(T_):
            lab = labels[c][t]
            key = ("class", lab) if t < n and lab != free else ("alone", c, t)
            want.setdefault(key, []).append(c * T_ + t)
    img, classes, fixed = sref.images(labels, usable, free)
    assert sref.cycles(img) == sorted(tuple(v) for v in want.values())
    assert classes == sum(1 for key in want if key[0] == "class") == stats["classes"]
    assert fixed == sum(1 for key, v in want.items() if len(v) == 1 and v[0] % T_ < n) == stats["fixed"]
    for cyc in sref.cycles(img):                     # ascending: every cell but the largest maps upwards
        assert all(img[j] > j for j in cyc[:-1]) and img[cyc[-1]] == cyc[0]


@pytest.mark.parametrize("k, T_, usable, free", [(3, 8, None, None), (3, 16, 12, FREE), (2, 4, None, FREE)])
def test_the_grand_product_closes_exactly_when_the_witness_respects_the_classes(k, T_, usable, free):
    labels = _labels(k, T_, 7 * k + T_, free_every=4 if free is not None else 0)
    shifts = [pow(7, c, R) for c in range(k)]
    cols, _ = sref.sigma_columns(labels, shifts, usable, free)
    wires = _witness(labels, 5, usable, free)
    assert sref.copy_violations(wires, labels, usable, free) == {"violations": 0, "first": None}
    beta, gamma = 0x1234567, 0x7654321
    assert gp.grand_product(wires, cols, shifts, beta, gamma)[1] == 1
    # one cell of a class of two or more, not its head
    img, _, _ = sref.images(labels, usable, free)
    cyc = next(c for c in sref.cycles(img) if len(c) >= 2)
    j = cyc[1]
    wires[j // T_][j % T_] = (wires[j // T_][j % T_] + 1) % R
    assert sref.copy_violations(wires, labels, usable, free) == {"violations": 1, "first": (j // T_, j % T_)}
    assert gp.grand_product(wires, cols, shifts, beta, gamma)[1] != 1


def test_a_changed_head_makes_every_other_cell_of_its_class_a_violation():
    labels = [[3, 3, 1, 3], [3, 2, 3, 1]]
    wires = _witness(labels, 9)
    wires[0][0] = (wires[0][0] + 1) % R            # the head of class 3 (m = 5 cells)
    assert sref.copy_violations(wires, labels) == {"violations": 4, "first": (0, 1)}
    assert sref.copy_violations(wires, labels, free_label=3) == {"violations": 0, "first": None}
    assert sref.copy_violations(wires, labels, usable=1) == {"violations": 1, "first": (1, 0)}


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
    labs = _sets(eng, 1, k=3)
    commitments, rset, stats = eng.commit_sigma(labs, [S, S, S])
    assert [name for name, _ in eng._lib.calls] == ["kzg_rows_commit_sigma"]
    args = eng._lib.calls[0][1]
    assert len(args) == len(_native.SYMBOLS["kzg_rows_commit_sigma"][1])
    assert (args[1], args[3], args[4], args[5]) == (1, 3, S * 3, None)
    assert (rset.k, rset.i, rset.T, len(rset.commitments)) == (3, 3, T, 3) and commitments == rset.commitments
    assert stats == {"classes": 0, "fixed": 0}        # (the stub leaves the zeros of the buffers)
    # the options struct: the usable layout and the free label, with bare handles of sets this engine made
    eng._lib.calls.clear()
    fl = b"\x73" * 32                                  # (no zero byte: the field reads back as a C string)
    eng.commit_sigma([1], [S, S, S], usable=T - 3, free_label=fl)
    args = eng._lib.calls[0][1]
    assert (args[5]._obj.usable, args[5]._obj.free_label_be32) == (T - 3, fl)
    eng._lib.calls.clear()
    eng.commit_sigma([1], [S, S, S], free_label=fl)
    assert (eng._lib.calls[0][1][5]._obj.usable, eng._lib.calls[0][1][5]._obj.free_label_be32) == (0, fl)
    # the check: k is what the label sets hold
    eng._lib.calls.clear()
    wires = _sets(eng, 3, first=20)
    res = eng.check_copies(wires, labs, usable=2)
    assert [name for name, _ in eng._lib.calls] == ["kzg_rows_check_copies"]
    args = eng._lib.calls[0][1]
    assert len(args) == len(_native.SYMBOLS["kzg_rows_check_copies"][1])
    assert (args[1], args[3], args[5], args[6]._obj.usable, args[6]._obj.free_label_be32) == (3, 1, 3, 2, None)
    assert res == {"violations": 0, "first": (0, 0)}


def test_first_is_split_into_column_and_row_and_none_is_the_header_s_sentinel(eng):
    class _Lib(_Recorder):
        first = 2 * T + 5

        def kzg_rows_check_copies(self, *args):
            args[7][0], args[7][1] = 4, self.first
            return _native.KZG_OK

        def kzg_rows_commit_sigma(self, *args):
            args[7][0], args[7][1] = 11, 6
            return _native.KZG_OK

    eng._lib = _Lib()
    labs, wires = _sets(eng, 1, k=3), _sets(eng, 1, first=9, k=3)
    assert eng.check_copies(wires, labs) == {"violations": 4, "first": (2, 5)}
    eng._lib.first = (1 << 64) - 1
    assert eng.check_copies(wires, labs) == {"violations": 4, "first": None}
    assert eng.commit_sigma(labs, [S] * 3)[2] == {"classes": 11, "fixed": 6}


BAD_SIGMA = {
    "no handles": lambda h: ([], [S]),
    "17 handles": lambda h: (h(17), [S]),
    "no shifts": lambda h: (h(1), []),
    "17 shifts": lambda h: (h(1), [S] * 17),
    "a short shift": lambda h: (h(1), [S[:31]]),
    "usable 0": lambda h: (h(1), [S], 0),
    "usable that is a bool": lambda h: (h(1), [S], True),
    "usable that is no integer": lambda h: (h(1), [S], "3"),
    "a short free label": lambda h: (h(1), [S], None, S[:31]),
}
BAD_CHECK = {
    "no wire handles": lambda h: ([], h(1)),
    "no label handles": lambda h: (h(1), []),
    "labels of unknown width": lambda h: (h(1), [100]),
    "usable 0": lambda h: (h(1), h(1), 0),
    "a long free label": lambda h: (h(1), h(1), None, S + b"\x00"),
}


@pytest.mark.parametrize("case", sorted(BAD_SIGMA))
def test_a_bad_sigma_shape_is_refused_under_the_method_s_name_before_any_native_call(eng, case):
    with pytest.raises(_native.KzgError) as err:
        eng.commit_sigma(*BAD_SIGMA[case](lambda n: _sets(eng, n)))
    assert err.value.code == _native.KZG_E_ARG
    assert str(err.value).split(": ", 1)[1].startswith("commit_sigma"), str(err.value)
    assert eng._lib.calls == [], "a bad shape must be refused before any native call"


@pytest.mark.parametrize("case", sorted(BAD_CHECK))
def test_a_bad_check_shape_is_refused_under_the_method_s_name_before_any_native_call(eng, case):
    with pytest.raises(_native.KzgError) as err:
        eng.check_copies(*BAD_CHECK[case](lambda n: _sets(eng, n)))
    assert err.value.code == _native.KZG_E_ARG
    assert str(err.value).split(": ", 1)[1].startswith("check_copies"), str(err.value)
    assert eng._lib.calls == [], "a bad shape must be refused before any native call"


def test_the_text_client_refuses_malformed_arguments_before_the_engine():
    from zkp_subnet_amd import Client, codec

    class _Engine:
        def __getattr__(self, name):
            raise AssertionError(f"the engine was reached: {name}")

    client = Client.__new__(Client)
    client.engine = _Engine()
    one, big = codec.be32_to_fr(S), codec.be32_to_fr(R.to_bytes(32, "big"))
    for args in (([], [one]), (["x"], [one]), ([1], []), ([1], [one] * 17), ([1], [big]), ([1], ["1"]), ([1], [one], 0),
                 ([1], [one], "3"), ([1], [one], True), ([1], [one], None, big), ([1], [one], None, "no scalar")):
        r = client.worker_commit_sigma(*args)
        assert r.status_code == 400 and "error" in r.json(), args
    for args in (([], [1]), ([1], []), ([1], ["x"]), ([1], [2], 0), ([1], [2], None, big)):
        r = client.worker_check_copies(*args)
        assert r.status_code == 400 and "error" in r.json(), args


def test_the_text_client_and_the_multi_device_client_pass_the_call_on():
    from zkp_subnet_amd import Client, codec
    from zkp_subnet_amd.multi import MultiDeviceClient

    class _Engine:
        def commit_sigma(self, hl, sh, usable, fl):
            self.got = (hl, sh, usable, fl)
            return [bytes([0xc0]) + bytes(47)] * len(sh), RowSet(self, 77, 0, len(sh), T, []), {"classes": 2, "fixed": 1}

        def check_copies(self, hw, hl, usable, fl):
            self.got = (hw, hl, usable, fl)
            return {"violations": 3, "first": (1, 4)}

    client = Client.__new__(Client)
    client.engine = _Engine()
    fr = lambda v: codec.be32_to_fr(v.to_bytes(32, "big"))   # noqa: E731
    r = client.worker_commit_sigma([5, 6], [fr(1), fr(7)], 6, fr(R - 1))
    assert r.status_code == 200, r.json()
    assert client.engine.got == ([5, 6], [(1).to_bytes(32, "big"), (7).to_bytes(32, "big")], 6, (R - 1).to_bytes(32, "big"))
    body = r.json()
    assert (body["handle"], body["classes"], body["fixed"], len(body["commitments"])) == (77, 2, 1, 2)
    r = client.worker_check_copies([8], [5, 6])
    assert r.status_code == 200 and r.json() == {"violations": 3, "first": [1, 4]}
    assert client.engine.got == ([8], [5, 6], None, None)
    for name in ("worker_commit_sigma", "worker_check_copies"):
        assert callable(getattr(MultiDeviceClient, name))


# ---------------------------------------------------------------------------------------------------- the header
def test_header_declares_the_symbols_and_the_struct():
    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x.h")).read()
    for name in ("kzg_rows_commit_sigma", "kzg_rows_check_copies"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert re.search(r"\bint\s+" + name.replace("kzg_", "kzg_multi_") + r"\s*\(", hdr), name
        assert len(_native.SYMBOLS[name.replace("kzg_", "kzg_multi_")][1]) == len(_native.SYMBOLS[name][1]) + 1
    assert re.search(r"typedef struct kzg_sigma_opts \{\s*uint64_t usable;[^}]*const uint8_t\* free_label_be32;[^}]*\} kzg_sigma_opts;",
                     hdr)
    assert [f[0] for f in SigmaOpts._fields_] == ["usable", "free_label_be32"]
    block = hdr[hdr.index("THE SIGMA COLUMNS"):hdr.index("int kzg_rows_check_copies")]
    for word in ("OUT OF SCOPE", "SOUNDNESS", "union-find", "convinces no verifier", "2^27", "kzg_rows_commit_grand_product_chain"):
        assert word in block, word
