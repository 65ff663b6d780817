"""CPU checks of the level plan that the product scan (csrc/fr_prod.hip: the grand products, the shuffle, the batched inversion)
and the additive scan (csrc/fr_lookup.hip: the logUp running sum) share: the hooks' header against the ctypes bindings, the plan
function (kzg_test_scan_plan_of, host only) against the model of tests/scan_ref.py for the library's plan and for callers' plans,
the facts that pin today's plan, the Python reference against hand-computed cases, and every refusal through both hooks with no
context.  No device."""
import ctypes
import os
import re

import pytest

from tests import scan_ref as sref
from tests.gpu_common import R
from zkp_subnet_amd import _native
from zkp_subnet_amd.engine import HipEngine, scan_plan_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = sorted(set(range(1, 71)) | {(1 << k) + d for k in range(33) for d in (-1, 0, 1) if 1 <= (1 << k) + d <= 1 << 32}
               | {3 << 16, 5 << 16, 3 << 18})


def scratch_elems(n):
    """elements of each scratch array the library allocates for n"""
    return (n + 3) // 4 * 3 // 2 + 64


def _header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _args(hdr, sym):
    decl = re.search(r"\bint\s+" + sym + r"\s*\((.*?)\);", hdr, re.S).group(1)
    return re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")


# ---------------------------------------------------------------------------------------------------- the header
def test_the_plan_hooks_are_declared_in_their_own_header_bound_and_exported():
    hooks_hdr, test_hdr = _header("kzg_mi355x_scan_test.h"), _header("kzg_mi355x_test.h")
    assert '#include "kzg_mi355x_scan_test.h"' in test_hdr
    declared = set(re.findall(r"\bint\s+(kzg_[a-z0-9_]+)\s*\(", hooks_hdr))
    assert declared == set(_native.SCAN_HOOKS) == {"kzg_test_scan_plan_of", "kzg_test_scan_run"}
    lib = _native.load()
    for sym, (res, args) in _native.SCAN_HOOKS.items():
        assert res is ctypes.c_int and len(_args(hooks_hdr, sym)) == len(args), sym
        assert getattr(lib, sym).argtypes == args
    assert not (declared & set(_native.SYMBOLS)) and not (declared & set(_native.RECUR_HOOKS))
    assert "kzg_test_" not in _header("kzg_mi355x.h")
    for name in ("kzg_test_scan_plan_of", "kzg_test_scan_run"):     # the list of hooks in the test header's comment
        assert name in test_hdr.split("#ifndef KZG_MI355X_TEST_H")[0], name
    assert callable(getattr(HipEngine, "test_scan_run"))


# ---------------------------------------------------------------------------------------------------- the reference itself
def test_the_reference_on_hand_computed_cases():
    assert sref.product([2, 3, 4], [1, 1, 2]) == ([1, 2, 6], 12)
    assert sref.product([2, 3, 4], [1, 1, 2], 5) == ([5, 10, 30], 60)
    out, cl = sref.product([1, 1], [2, 4])
    assert out[1] * 2 % R == 1 and cl * 8 % R == 1
    assert sref.product([3, 0, 7], [1, 1, 1]) == ([1, 3, 0], 0)                     # every value behind a zero numerator is 0
    inv, cl = sref.inverses([2, R - 1])
    assert inv == [(R + 1) // 2, R - 1] and cl == 1
    assert sref.inverses([2, 4], [6, 0]) == ([3, 0], 1)
    assert sref.sums([1, 2, R - 1]) == ([0, 1, 3], 2)
    assert sref.run(0, [2], [1]) == ([1], 2) and sref.run(1, [2], [1], 3) == ([3], 6) and sref.run(4, [9]) == ([0], 9)
    assert sref.run(2, [2]) == ([(R + 1) // 2], 1) and sref.run(3, [2], [4]) == ([2], 1)
    assert sref.plan(1) == {"K": 1, "l": [2, 0], "n": [1, 1], "off": [0, 0]}
    assert sref.plan(4096, 2, 16) == {"K": 3, "l": [2, 4, 4, 0], "n": [4096, 1024, 64, 4], "off": [0, 0, 1024, 1088]}
    assert sref.plan(17, 4, 1) == {"K": 2, "l": [4, 4, 0], "n": [17, 2, 1], "off": [0, 0, 2]}


# ---------------------------------------------------------------------------------------------------- the plan
@pytest.mark.parametrize("n", SIZES)
def test_the_library_s_plan(n):
    pl = scan_plan_of(n)
    assert pl == sref.plan(n)
    l0 = 2 if n < 1 << 17 else 3 if n < 1 << 18 else 4
    assert pl["K"] >= 1 and pl["n"][0] == n and pl["n"][-1] <= 2048 and all(m > 2048 for m in pl["n"][1:-1])
    assert pl["l"] == [l0] + [4] * (pl["K"] - 1) + [0]
    for k in range(pl["K"]):
        assert pl["n"][k + 1] == -(-pl["n"][k] // (1 << pl["l"][k]))
    # level 1 starts the scratch, the levels above lie one behind the other, all inside what the library allocates
    assert pl["off"][:2] == [0, 0]
    for k in range(1, pl["K"]):
        assert pl["off"][k + 1] == pl["off"][k] + pl["n"][k]
    for k in range(1, pl["K"] + 1):
        assert pl["off"][k] + pl["n"][k] <= scratch_elems(n), k


@pytest.mark.parametrize("top_max", [1, 3, 7, 16, 256, 2048])
@pytest.mark.parametrize("l0", [2, 3, 4])
def test_a_caller_s_plan(l0, top_max):
    for n in SIZES:
        pl = scan_plan_of(n, l0, top_max)
        assert pl == sref.plan(n, l0, top_max), n
        assert pl["K"] >= 1 and pl["n"][-1] <= top_max and all(m > top_max for m in pl["n"][1:-1]), n
        assert pl["off"][-1] + pl["n"][-1] <= scratch_elems(n), n


def test_the_library_s_plan_at_the_named_sizes():
    # l0 changes exactly at 2^17 and 2^18
    assert [scan_plan_of(n)["l"][0] for n in ((1 << 17) - 1, 1 << 17, (1 << 18) - 1, 1 << 18, 1 << 32)] == [2, 3, 3, 4, 4]
    # no K = 0 form: one level under the top from n = 1 up to 2^13
    assert scan_plan_of(1) == {"K": 1, "l": [2, 0], "n": [1, 1], "off": [0, 0]}
    assert scan_plan_of(1 << 13) == {"K": 1, "l": [2, 0], "n": [8192, 2048], "off": [0, 0]}
    assert scan_plan_of((1 << 13) + 1)["n"] == [8193, 2049, 129]
    # two up to 2^19, three first in 2^19 + 1 .. 2^20
    for n in ((1 << 17) - 1, 1 << 17, (1 << 18) - 1, 1 << 18, 1 << 19):
        assert scan_plan_of(n)["K"] == 2, n
    assert scan_plan_of((1 << 19) + 1)["n"] == [(1 << 19) + 1, 32769, 2049, 129]
    assert scan_plan_of(1 << 20) == {"K": 3, "l": [4, 4, 4, 0], "n": [1 << 20, 1 << 16, 4096, 256], "off": [0, 0, 65536, 69632]}
    assert scan_plan_of(3 << 18)["n"] == [3 << 18, 49152, 3072, 192]      # n_inv T of a three-column inversion
    assert max(scan_plan_of(n)["K"] for n in SIZES) == 6 == scan_plan_of(1 << 32)["K"]


def test_a_caller_s_plan_at_the_named_sizes_and_every_precondition_refusal():
    assert scan_plan_of(4096, 2, 16) == {"K": 3, "l": [2, 4, 4, 0], "n": [4096, 1024, 64, 4], "off": [0, 0, 1024, 1088]}
    assert scan_plan_of(4096, 4, 1)["n"] == [4096, 256, 16, 1]
    assert scan_plan_of(5, 3, 2048) == {"K": 1, "l": [3, 0], "n": [5, 1], "off": [0, 0]}      # (the recurrence scan: K = 0)
    assert scan_plan_of(1 << 32, 2, 1)["K"] == 9                                               # the most levels any n takes
    refusals = (((0, 2, 16), "no elements"), ((0, -1, -1), "no elements"), (((1 << 32) + 1, 2, 16), "2^32"),
                (((1 << 32) + 1, -1, -1), "2^32"), ((4096, 1, 16), "level-0 chunk"), ((4096, 5, 16), "level-0 chunk"),
                ((4096, -1, 16), "level-0 chunk"), ((4096, 2, 0), "1 .. 2048"), ((4096, 2, -1), "1 .. 2048"),
                ((4096, 2, 2049), "1 .. 2048"))
    for args, why in refusals:
        with pytest.raises(_native.KzgError) as err:
            scan_plan_of(*args)
        assert err.value.code == _native.KZG_E_ARG and why in str(err.value), (args, str(err.value))
    lib = _native.load()
    K, zf = ctypes.c_int(0), ctypes.c_uint32(0)
    arr_l, arr_n = (ctypes.c_int * 16)(), (ctypes.c_uint64 * 16)()
    assert lib.kzg_test_scan_plan_of(4, -1, -1, ctypes.byref(K), arr_l, arr_n, None) == _native.KZG_E_ARG
    assert b"null output" in lib.kzg_last_error(None)
    # the run hook judges the plan, and then its other arguments, before it looks at the context: no device is needed to be refused
    for (n, l0, top_max), why in refusals:
        assert lib.kzg_test_scan_run(None, 0, l0, top_max, None, None, None, n, None, None, ctypes.byref(zf)) == _native.KZG_E_ARG
        assert why.encode() in lib.kzg_last_error(None), (n, l0, top_max)
    assert lib.kzg_test_scan_run(None, 0, -1, -1, None, None, None, (1 << 22) + 1, None, None, None) == _native.KZG_E_ARG
    assert b"2^22" in lib.kzg_last_error(None)
    for form in (-1, 5):
        assert lib.kzg_test_scan_run(None, form, -1, -1, None, None, None, 4, None, None, None) == _native.KZG_E_ARG
        assert b"form must be" in lib.kzg_last_error(None)
    assert lib.kzg_test_scan_run(None, 0, -1, -1, None, None, None, 4, None, None, None) == _native.KZG_E_ARG
    assert b"no context" in lib.kzg_last_error(None)
