"""The opening scan's level plans without a device: the library's plan function (kzg_test_poly_plan_of) is the launcher arithmetic
it had before plan and execution were separated, every plan it makes satisfies the kernels' preconditions and fits the scratch the
library allocates, the small plans of tests/poly_ref.py hold every signature those plans hold, the closed forms of the input
families agree with Horner's rule and synthetic division, and kzg_test_poly_run refuses a malformed plan before it looks at its
context."""
import ctypes

import pytest

from oracle.bls12_381 import R
from tests import poly_ref as pr
from zkp_subnet_amd import KzgError, _native
from zkp_subnet_amd.build import build
from zkp_subnet_amd.engine import poly_plan_of


@pytest.fixture(scope="module")
def lib():
    build()
    lib = _native.load()
    lib.kzg_last_error.restype = ctypes.c_char_p
    return lib


def test_plan_function_is_the_launcher_arithmetic_it_replaced(lib, monkeypatch):
    monkeypatch.delenv("KZG_POLY_NO_LDS", raising=False)
    monkeypatch.delenv("KZG_POLY_LDS_MIN_LOG", raising=False)
    lengths = sorted(set(range(1, (1 << 14) + 1)) | set(pr.production_lengths()))
    assert lengths[-1] == 1 << pr.MAX_LOG
    for n in lengths:
        got = poly_plan_of(n)
        assert got == pr.plan_of(n, pr.PRODUCTION), n
        # the stacked levels fit the scratch every caller allocates (poly_level_words), shown and not assumed
        assert (got["off"][-1] + got["n"][-1]) * 8 <= pr.level_words(n), n
        assert pr.plan_invalid(n, pr.production_plan(n)) is None, n
    # what the issue that asked for this quotes: the level-0 chunk, the levels and the scan's lanes by length
    assert [pr.lchunk(n) for n in ((1 << 17) - 1, 1 << 17, (1 << 18) - 1, 1 << 18)] == [2, 3, 3, 4]
    assert [poly_plan_of(n)["K"] for n in (8192, 8193, 1 << 19, (1 << 19) + 1, 1 << 23, (1 << 23) + 1, 1 << 27, (1 << 27) + 1)] == \
        [1, 2, 2, 3, 3, 4, 4, 5]
    assert [poly_plan_of(n)["scan_nt"] for n in (4096, 4097, 8192, 8193, (1 << 16) + 1, 1 << 17)] == [256, 1024, 1024, 256, 1024, 256]
    assert poly_plan_of((1 << 16) + 1) == {"K": 2, "l": [2, 4, 0], "sq": [0, 2, 6], "n": [65537, 16385, 1025], "off": [0, 0, 16385],
                                           "scan_nt": 1024, "lds": 0}
    assert [poly_plan_of(n)["lds"] for n in (1 << 20, 1 << 21, (1 << 21) + 1024, (1 << 21) + 512, 1 << 22)] == [0, 1, 1, 0, 1]
    assert poly_plan_of(1 << 28)["sq"] == [0, 4, 8, 12, 16, 20]


def test_a_callers_plan_is_the_same_arithmetic_with_its_own_parameters(lib):
    for n, plan, _ in pr.covering_plans():
        assert poly_plan_of(n, *plan) == pr.plan_of(n, plan), pr.plan_name(n, plan)
    for n in (1, 2, 17, 1000, 1024, 4097, 65537, 1 << 17):
        for l0 in (2, 3, 4):
            for scan_max in (1, 2, 16, 17, 255, 2048, 1 << 20):
                for scan_nt in (256, 1024):
                    plan = (l0, scan_max, scan_nt, 0)
                    assert poly_plan_of(n, *plan) == pr.plan_of(n, plan), pr.plan_name(n, plan)
    # five levels, and the exponents 12, 16 and 20 that production reaches from 2^19, 2^23 and 2^27 only, inside 2^16 + 1
    assert poly_plan_of(65537, 4, 1, 256, 0) == {"K": 5, "l": [4, 4, 4, 4, 4, 0], "sq": [0, 4, 8, 12, 16, 20],
                                                 "n": [65537, 4097, 257, 17, 2, 1], "off": [0, 0, 4097, 4354, 4371, 4373],
                                                 "scan_nt": 256, "lds": 0}


_KNOBS = r'''
import sys
sys.path.insert(0, %r)
from zkp_subnet_amd.engine import poly_plan_of
print([poly_plan_of(n)["lds"] for n in (1024, 1 << 18, 1 << 20, 1 << 21, (1 << 21) + 16, 1 << 22)])
'''


def test_the_two_environment_knobs_still_steer_the_production_plan(lib):
    """KZG_POLY_NO_LDS / KZG_POLY_LDS_MIN_LOG are read once per process, by poly_plan alone: each setting in an interpreter of its
    own (no device)"""
    import os
    import subprocess
    import sys

    from tests.gpu_common import ROOT

    def run(**env):
        base = {k: v for k, v in os.environ.items() if k not in ("KZG_POLY_NO_LDS", "KZG_POLY_LDS_MIN_LOG")}
        out = subprocess.run([sys.executable, "-c", _KNOBS % ROOT], capture_output=True, text=True, timeout=300, env=dict(base, **env))
        assert out.returncode == 0, out.stderr[-2000:]
        return out.stdout.strip()

    def want(**kw):
        return str([pr.production_plan(n, **kw)[3] for n in (1024, 1 << 18, 1 << 20, 1 << 21, (1 << 21) + 16, 1 << 22)])

    assert run() == want() == "[0, 0, 0, 1, 0, 1]"
    assert run(KZG_POLY_NO_LDS="1") == want(no_lds=True) == "[0, 0, 0, 0, 0, 0]"
    assert run(KZG_POLY_LDS_MIN_LOG="18") == want(lds_min_log=18) == "[0, 1, 1, 1, 0, 1]"
    # the threshold can go below 2^18, the chunk length cannot: l0 = 4 starts there, and the plan stays a valid one
    assert run(KZG_POLY_LDS_MIN_LOG="10") == want(lds_min_log=10) == "[0, 1, 1, 1, 0, 1]"
    assert run(KZG_POLY_LDS_MIN_LOG="22", KZG_POLY_NO_LDS="") == want(no_lds=True)


def _refusal_of_plan(n, *plan):
    with pytest.raises(KzgError) as e:
        poly_plan_of(n, *plan)
    assert e.value.code == _native.KZG_E_ARG
    return str(e.value).split("E_ARG: ")[-1]


L0, SCAN, LANES, LEVELS, LDS, NONE = ("poly plan: level-0 chunk outside 2^2 .. 2^4", "poly plan: the scan must be left at least one value",
                                      "poly plan: the scan runs 256 or 1024 lanes", "poly plan: more than 14 levels",
                                      "poly plan: the LDS-staged quotient needs 16-long chunks and whole blocks of 1024 coefficients",
                                      "poly plan: no coefficients")
BAD_PLANS = [((100, 1, 8, 256, 0), L0), ((100, 5, 8, 256, 0), L0), ((100, 0, 8, 256, 0), L0), ((100, -1, 8, 256, 0), L0),
             ((100, 2, 0, 256, 0), SCAN), ((100, 2, -1, 256, 0), SCAN), ((100, 2, -5, 256, 0), SCAN),
             ((100, 2, 8, 0, 0), LANES), ((100, 2, 8, 64, 0), LANES), ((100, 2, 8, 512, 0), LANES), ((100, 2, 8, 2048, 0), LANES),
             ((100, 2, 8, -1, 0), LANES),
             ((1 << 62, 2, 1, 256, 0), LEVELS), ((1 << 60, 4, 3, 1024, 0), LEVELS),
             ((1024, 2, 8, 256, 1), LDS), ((2048, 3, 8, 256, 1), LDS), ((1000, 4, 8, 256, 1), LDS), ((1024 + 16, 4, 8, 256, 1), LDS),
             ((512, 4, 8, 256, 1), LDS), ((16, 4, 8, 256, 1), LDS),
             ((100, 2, 8, 256, 2), "poly plan: lds must be 0 or 1"), ((100, 2, 8, 256, -1), "poly plan: lds must be 0 or 1"),
             ((0, 2, 8, 256, 0), NONE), ((0, -1, -1, -1, -1), NONE)]


def test_every_refusal_of_the_plan_check(lib):
    for args, why in BAD_PLANS:
        assert _refusal_of_plan(*args) == why, args
        assert (pr.plan_invalid(args[0], args[1:]) is not None), args
    # the neighbours that are plans
    for args in ((100, 2, 1, 256, 0), (100, 4, 1, 1024, 0), (1024, 4, 1, 256, 1), (3072, 4, 2048, 1024, 1), (1 << 54, 2, 1, 256, 0)):
        assert poly_plan_of(*args)["K"] >= 1 and pr.plan_invalid(args[0], args[1:]) is None, args
    assert poly_plan_of(1 << 54, 2, 1, 256, 0)["K"] == 14 and _refusal_of_plan((1 << 54) + 1, 2, 1, 256, 0) == LEVELS
    # the last precondition -- the stacked levels inside poly_level_words(n) -- is refused by no parameter there is: with chunks of
    # at least 4 and 16 the levels hold at most ceil(n / 4) (1 + 1/16 + 1/256 + ...) + 14 values, and the scratch ceil(n / 4) 3/2 + 64.
    # Checked here on every plan shape of every length up to 2^12 and around every power of two, where the rounding weighs most
    for n in sorted(set(range(1, 4097)) | {(1 << k) + d for k in range(12, 29) for d in (-1, 0, 1)}):
        for l0 in (2, 3, 4):
            lv = pr.levels(n, l0, 1)
            assert lv["n"][lv["K"]] == 1 and (lv["off"][lv["K"]] + 1) * 8 <= pr.level_words(n), (n, l0)
    assert lib.kzg_test_poly_plan_of(100, -1, -1, -1, -1, None, None, None, None, None, None, None) == _native.KZG_E_ARG


def _refusal_of_run(lib, form, n, plan, rows=1, pairs=(), pts=None, nalphas=1, data=True, ctx=None):
    f = ctypes.create_string_buffer(32 * max(1, rows * min(n, 1 << 12))) if data else None
    alphas = ctypes.create_string_buffer(32 * max(1, nalphas))
    y, q = ctypes.create_string_buffer(32 * 64), ctypes.create_string_buffer(32 * max(1, rows * min(n, 1 << 12)))
    pr_, pp = bytes(r for r, _ in pairs), bytes(p for _, p in pairs)
    rc = lib.kzg_test_poly_run(ctx, form, *plan, ctypes.addressof(f) if data else None, n, rows, 0, pr_, pp, len(pairs),
                               bytes(pts) if pts is not None else None, ctypes.addressof(alphas), nalphas, ctypes.addressof(y),
                               ctypes.addressof(q))
    assert rc == _native.KZG_E_ARG, (form, n, plan, rc)
    assert q.raw == bytes(len(q.raw)) and y.raw == bytes(len(y.raw))
    return lib.kzg_last_error(None).decode()


def test_run_hook_refuses_a_null_context_and_every_malformed_plan_without_a_device(lib):
    none = "poly run: no context or no data"
    # a valid plan gets as far as the context, and no further
    for n, plan, forms in pr.covering_plans():
        assert _refusal_of_run(lib, 0, n, plan) == none, pr.plan_name(n, plan)
    assert _refusal_of_run(lib, 0, 1000, pr.PRODUCTION) == none and _refusal_of_run(lib, 1, 1000, pr.PRODUCTION) == none
    assert _refusal_of_run(lib, 2, 100, pr.PRODUCTION, rows=16) == none
    assert _refusal_of_run(lib, 3, 100, pr.PRODUCTION, rows=3, pairs=[(2, 0), (0, 1), (1, 1)], nalphas=2) == none
    assert _refusal_of_run(lib, 4, 100, pr.PRODUCTION, rows=4, nalphas=4) == none
    assert _refusal_of_run(lib, 5, 100, pr.PRODUCTION, rows=2, pts=[1, 1], nalphas=2) == none
    assert _refusal_of_run(lib, 0, 100, pr.PRODUCTION, data=False) == none
    # the plan is judged before anything else, whatever else is wrong with the call
    for args, why in BAD_PLANS:
        assert _refusal_of_run(lib, 0, args[0], args[1:]) == why, args
        assert _refusal_of_run(lib, 9, args[0], args[1:], rows=0, nalphas=0, data=False) == why, args
    # then the call
    assert _refusal_of_run(lib, -1, 100, pr.PRODUCTION) == _refusal_of_run(lib, 6, 100, pr.PRODUCTION) == "poly run: form outside [0, 5]"
    rows_msg = "poly run: 1 row (forms 0, 1), up to 16 (2, 3) or 4 (4, 5), at most 2^22 coefficients in all"
    for form, rows in ((0, 2), (1, 2), (2, 17), (3, 17), (4, 5), (5, 5), (0, 0), (2, 0)):
        assert _refusal_of_run(lib, form, 100, pr.PRODUCTION, rows=rows, nalphas=min(max(rows, 1), 4)) == rows_msg, (form, rows)
    assert _refusal_of_run(lib, 0, (1 << 22) + 1, pr.PRODUCTION) == rows_msg and _refusal_of_run(lib, 2, 1 << 19, pr.PRODUCTION, rows=16) == rows_msg
    pts_msg = "poly run: one point (forms 0 - 2), up to 4 (3, 5), one per vector (4)"
    assert _refusal_of_run(lib, 0, 100, pr.PRODUCTION, nalphas=2) == pts_msg and _refusal_of_run(lib, 0, 100, pr.PRODUCTION, nalphas=0) == pts_msg
    assert _refusal_of_run(lib, 3, 100, pr.PRODUCTION, rows=2, pairs=[(0, 0)], nalphas=5) == pts_msg
    assert _refusal_of_run(lib, 4, 100, pr.PRODUCTION, rows=3, nalphas=2) == pts_msg
    pair_msg = "poly run: a pair names no row or no point, or the pairs are not point-major"
    assert _refusal_of_run(lib, 3, 100, pr.PRODUCTION, rows=2, pairs=[(2, 0)], nalphas=1) == pair_msg
    assert _refusal_of_run(lib, 3, 100, pr.PRODUCTION, rows=2, pairs=[(0, 1)], nalphas=1) == pair_msg
    assert _refusal_of_run(lib, 3, 100, pr.PRODUCTION, rows=2, pairs=[(0, 1), (1, 0)], nalphas=2) == pair_msg
    assert _refusal_of_run(lib, 3, 100, pr.PRODUCTION, rows=2, pairs=[], nalphas=2) == "poly run: 1 .. 64 pairs"
    assert _refusal_of_run(lib, 3, 100, pr.PRODUCTION, rows=2, pairs=[(0, 0)] * 65, nalphas=2) == "poly run: 1 .. 64 pairs"
    assert _refusal_of_run(lib, 5, 100, pr.PRODUCTION, rows=2, nalphas=2) == "poly run: form 5 takes a map of points"
    assert _refusal_of_run(lib, 5, 100, pr.PRODUCTION, rows=2, pts=[0, 2], nalphas=2) == "poly run: the map names no point"


def test_covering_plans_hold_every_production_signature_within_2_17(lib):
    want, cover = pr.production_signatures(), pr.covering_plans()
    held = set()
    for n, plan, forms in cover:
        assert n <= pr.CAP and pr.plan_invalid(n, plan) is None and forms, pr.plan_name(n, plan)
        assert poly_plan_of(n, *plan) == pr.plan_of(n, plan)
        for form in forms:
            held |= pr.signatures(n, plan, form)
    assert want <= held, sorted(want - held, key=str)                # a condition: an unheld signature fails, nothing is skipped
    assert max(n for n, _, _ in cover) == 65537 and len(cover) <= 64
    # what production reaches at single sizes, or not at all under a test so far
    for sig in [("sq", k, v) for k in ("level", "expand") for v in (2, 3, 4, 8, 12, 16)] + [("sq", "scan", v) for v in (2, 6, 7, 8, 12, 16, 20)]:
        assert sig in want, sig
    for sig in (("scan", 1024, 2, False, False), ("scan", 1024, 2, True, True), ("scan", 1024, 2, False, True), ("scan", 256, 4, True, True),
                ("scan", 256, 4, False, True), ("scan", 256, 1, True, False), ("scan", 256, 3, False, True),
                ("quot", "lds", "single", 4, 0), ("quot", "lds", "pairs", 4, 0), ("quot", "mont", "pairs", 3, 5), ("quot", "strided", "single", 3, 1),
                ("level", True, 3, True, "single"), ("level", True, 3, True, "pairs"), ("level", False, 3, False, "pairs"),
                ("level", True, 4, True, "rows"), ("level", False, 4, True, "rows"), ("expand", 4, True), ("expand", 4, False)):
        assert sig in want, sig
    # every length of the production enumeration holds only signatures of the list (the list is closed under what was enumerated)
    for n in (1 << 17, (1 << 17) + 5, 1 << 22, (1 << 27) + 1):
        for form in pr.FORMS:
            assert pr.signatures(n, pr.PRODUCTION, form) <= held
    # the extra plans are plans
    for n, plan in pr.extra_plans():
        assert pr.plan_invalid(n, plan) is None and n <= pr.CAP and poly_plan_of(n, *plan)["n"][1] > 768


def test_closed_forms_equal_horner_and_synthetic_division():
    for n in (1, 2, 3, 4, 5, 7, 16, 17, 64, 100, 257):
        fams = pr.families(n)
        assert {"zero", "constant r-1", "delta r-1 at 0", f"delta r-1 at {n - 1}", "geometric", "multiple of X - a", "all r-1 at r-1",
                "edge pool", "uniform"} <= set(fams)
        for name, f in fams.items():
            assert len(f.f) == n and all(0 <= v < R for v in f.f)
            for pname, alpha in list(pr.points(n).items()) + ([("own", f.point)] if f.point is not None else []):
                y, q = pr.open_at(f.f, alpha)
                assert len(q) == n and q[n - 1] == 0 and y == pr.horner(f.f, alpha)
                assert pr.expected(n, name, alpha) == (y, tuple(q))
                # the definition itself: f = q (X - alpha) + y, coefficient by coefficient
                assert all(((q[j - 1] if j else y) - alpha * q[j] - f.f[j]) % R == 0 for j in range(n))
                c = f.closed(alpha)
                assert c is None or (c[0], list(c[1])) == (y, q), (n, name, pname)
        assert fams["multiple of X - a"].closed(fams["multiple of X - a"].point) is not None
        assert pr.open_at(fams["multiple of X - a"].f, fams["multiple of X - a"].point)[0] == 0
        assert fams["all r-1 at r-1"].point == R - 1 and fams["all r-1 at r-1"].closed(R - 1) is not None
    w = pr.points(100)["root of unity"]
    assert pow(w, 128, R) == 1 and pow(w, 64, R) == R - 1 and pr.points(1)["root of unity"] == 1
    assert pr.words_to_ints((5).to_bytes(32, "little") + (R - 1).to_bytes(32, "little")) == [5, R - 1]
    assert pr.MONT == pow(2, 261, R)
