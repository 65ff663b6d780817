"""The inputs of tests/test_gpu_fp_classes.py are legitimate and its reference is right (no GPU): every generated operand lies
inside the class its operation documents (csrc/fp28.hip.h, fr29.hip.h, fp_lp.hip.h, g1.hip.h), the reference's output lies inside
the documented output class, the reference agrees with the stand-alone limb models of scripts/models/ -- value and number of
normalisation rounds -- and the constant tables of the headers are the integers they claim to be.  A failure of the GPU module is
then the kernel's."""
import importlib.util
import os
import re

import pytest

from tests import fp28_ref as ref
from tests.fp28_ref import FP, FR, MASK, P, RMOD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", "models", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lp_model():
    return _model("lp_mul_model")


@pytest.mark.parametrize("name", sorted(ref.OPS))
def test_every_input_is_inside_its_class_and_the_reference_output_inside_the_output_class(name):
    op = ref.OPS[name]
    fam, exp = ref.family(name), ref.expected(name)
    assert 0 < len(fam) <= 4000 and len(fam) == len(exp)
    assert all(len(x) == op.arity and all(len(l) == (14 if op.field == 0 else 9) for l in x) for x in fam)
    bad = [i for i, x in enumerate(fam) if not op.pre(*x)]
    assert not bad, f"{name}: inputs {bad[:5]} break the documented precondition"
    bad = [i for i, (x, e) in enumerate(zip(fam, exp)) if not op.post(x, e)]
    assert not bad, f"{name}: reference outputs {bad[:5]} break the documented postcondition"
    assert all(0 <= v < (1 << 32) for e in exp for v in e)


def test_families_sit_on_the_class_bounds():
    """the corners the issue names are present, not merely admitted"""
    top = (1 << 30) - 1
    for name in ("fp_mul", "fp_mul_inline", "lp_mul"):
        fam = ref.family(name)
        c = FP.corner(top, 32 * P)
        assert (c, c) in fam and FP.value(c) < 32 * P <= FP.value(c) + (1 << FP.top)
    for name in ("fp_sqr", "fp_sqr_inline", "fp_canon_mont"):
        assert (FP.corner(top, 32 * P),) in ref.family(name)
    corners = tuple(FP.corner(lm, k * P) for lm, k in zip(ref.MUL2_LIMB, ref.MUL2_K))
    assert corners in ref.family("fp_mul2_inline")
    assert [c[0] for c in corners] == [3 << 28, 3 << 28, (1 << 29) - 1, (1 << 28) - 1]
    assert all(k * P - (1 << FP.top) <= FP.value(c) < k * P for c, k in zip(corners, ref.MUL2_K))
    for name, k in (("fp_sub4", 2), ("fp_sub8", 6), ("fp_sub16", 14)):
        subs = [b for _, b in ref.family(name)]
        assert FP.pack(k * P - 1) in subs and FP.pack(0) in subs and FP.corner(MASK, k * P) in subs
        assert any(a == [(1 << 31) - 1] * 14 for a, _ in ref.family(name))
    a = FR.corner((1 << 31) - 1, 64 * RMOD)
    seconds = [FR.value(b) for x, b in ref.family("fr9_mul") if x == a]
    assert max(seconds) == (FR.R * RMOD - 1) // FR.value(a) and min(seconds) == 0


def test_both_representatives_of_zero():
    """a = 0 gives limbs 0; a = p times any nonzero b gives exactly p; fp_is_zero_n says yes to both and no to their neighbours"""
    z, p = FP.pack(0), FP.pack(P)
    for name in ("fp_mul", "fp_mul_inline", "lp_mul"):
        seen = {0: 0, P: 0}
        for (a, b), e in zip(ref.family(name), ref.expected(name)):
            if FP.value(a) == 0:
                assert e == z
                seen[0] += 1
            elif a == p and FP.value(b):
                assert e == p
                seen[P] += 1
        assert seen[0] > 5 and seen[P] > 5, seen
    yes_no = {tuple(a): e[0] for (a,), e in zip(ref.family("fp_is_zero_n"), ref.expected("fp_is_zero_n"))}
    assert yes_no[tuple(z)] == 1 and yes_no[tuple(p)] == 1
    assert [yes_no[tuple(FP.pack(v))] for v in (2 * P - 1, P - 1, P + 1, 1)] == [0, 0, 0, 0]
    assert sum(yes_no.values()) == 2 and len(yes_no) > 500


def test_reference_agrees_with_the_lane_parallel_model(lp_model):
    """scripts/models/lp_mul_model.py, the limb-exact model lp_mul was transcribed from: same limbs, same number of rounds of the
    closing normalisation, for every pair of the lp_mul family; the zero-run products need every count up to 13"""
    hist = {}
    for (a, b), e in zip(ref.family("lp_mul"), ref.expected("lp_mul")):
        stats = {"max_acc": 0, "max_rounds": 0, "rounds_hist": {}}
        t = lp_model.lp_mul(a + [0, 0], b + [0, 0], stats)
        mine, rounds = ref.lp_mul_model(a, b)
        assert t[:14] == e == mine and t[14:] == [0, 0] and stats["max_rounds"] == rounds
        assert stats["max_acc"] < (1 << 64)
        hist[rounds] = hist.get(rounds, 0) + 1
    assert hist.get(13, 0) >= 3 and sum(v for k, v in hist.items() if 2 <= k <= 12) >= 20, hist


def test_ripple_family_reaches_thirteen_rounds_in_the_model(lp_model):
    hist = {}
    for (lo, hi), e in zip(ref.family("lp_norm"), ref.expected("lp_norm")):
        t = [l | (h << 32) for l, h in zip(lo, hi)]
        got, rounds = lp_model.lp_norm(t + [0, 0])
        mine, mine_rounds = ref.lp_norm_model(t)
        assert got[:14] == e == mine and got[14:] == [0, 0] and rounds == mine_rounds
        hist[rounds] = hist.get(rounds, 0) + 1
    assert set(range(14)) <= set(hist), hist                    # every number of rounds from none to 13 occurs
    first = ref.ripple(0, 12)
    assert first[1:13] == [MASK] * 12 and first[0] > MASK and lp_model.lp_norm(first + [0, 0])[1] == 13
    assert max(max(l | (h << 32) for l, h in zip(lo, hi)) for lo, hi in ref.family("lp_norm")) == ref.LP_COLUMN_MAX


def test_reference_agrees_with_the_fr_model():
    m = _model("fr29_model")
    for (a, b), e in zip(ref.family("fr9_mul"), ref.expected("fr9_mul")):
        assert m.mul(a, b) == e
    for (a,), e in zip(ref.family("fr9_norm"), ref.expected("fr9_norm")):
        assert m.norm(a) == e
    assert m.M4 == FR.dominating(4) and m.M8 == FR.dominating(8)


def _tables(header, macro):
    src = open(os.path.join(ROOT, "zkp_subnet_amd", "csrc", header)).read()
    return {name: [int(x.rstrip("u"), 16) for x in re.findall(r"0x[0-9a-fA-F]+u", body)]
            for name, body in re.findall(macro + r"\((\w+),([^)]*)\)", src) if name != "name"}


def test_header_constant_tables_are_the_integers_they_claim():
    fp = _tables("fp28.hip.h", "FP28_TABLE")
    assert fp == {"fp28_p": FP.pack(P), "fp28_one": FP.pack(FP.one), "fp28_r2": FP.pack(FP.r2), "fp28_m4": FP.dominating(4),
                  "fp28_m8": FP.dominating(8), "fp28_m16": FP.dominating(16)}
    fr = _tables("fr29.hip.h", "FR9_TABLE")
    assert fr == {"fr9_r": FR.pack(RMOD), "fr9_one_c": FR.pack(FR.one), "fr9_r2": FR.pack(FR.r2), "fr9_m4": FR.dominating(4),
                  "fr9_m8": FR.dominating(8)}
    src = open(os.path.join(ROOT, "zkp_subnet_amd", "csrc", "fp28.hip.h")).read()
    assert int(re.search(r"#define FP28_PINV (0x[0-9a-f]+)u", src).group(1), 16) == FP.ninv & MASK
    # a dominating multiple covers its class: limb-wise M - b never borrows for a normalised b below 2 / 6 / 14 times the modulus
    for F, pairs in ((FP, ((4, 2), (8, 6), (16, 14))), (FR, ((4, 2), (8, 6)))):
        for k, bound in pairs:
            m = F.dominating(k)
            assert all(x >= F.mask for x in m[:-1]) and m[-1] >= (bound * F.mod - 1) >> F.top and max(m) < (1 << (F.w + 1))


def test_hook_codes_match_the_test_header():
    hdr = open(os.path.join(ROOT, "include", "kzg_mi355x_test.h")).read()
    flat = " ".join(hdr.split()).replace("* ", "")
    for name, code in list(ref.FP_CODES.items()) + list(ref.FR_CODES.items()):
        if name in ("fp_sub4", "fp_sub8", "fp_sub16"):
            continue
        assert re.search(rf"\b{code} {name}\b", flat), (code, name)
    assert "5 / 6 / 7 fp_sub4 / fp_sub8 / fp_sub16" in flat
    for text in ("0 g1_add<false>", "1 g1_add<true>", "2 g1_madd<false>", "3 g1_madd<true>", "4 g1_dbl", "5 lp_add", "6 lp_dbl"):
        assert text in flat, text
    assert list(ref.G1_CODES.values()) == list(range(7))


def test_point_family_represents_its_points_inside_the_stored_classes():
    from oracle import bls12_381 as o

    fam = ref.point_family()
    assert len(fam) == 64 * 5
    rinv = pow(FP.R, -1, P)

    def affine(l56):
        if not any(l56):
            return None
        x, y, zz, zzz = (FP.value(l56[14 * i:14 * i + 14]) * rinv % P for i in range(4))
        assert zz * zz * zz % P == zzz * zzz % P
        return (x * pow(zz, -1, P) % P, y * pow(zzz, -1, P) % P)

    tops = [0, 0, 0, 0]
    for pa, pb, a, b, b_aff in fam:
        assert ref.stored_pre(a) and ref.stored_pre(b)
        assert affine(a) == pa and affine(b) == pb and (pa is None or o.is_on_curve(pa))
        if pb is None:
            assert not any(b_aff)
        else:
            assert (FP.value(b_aff[:14]) * rinv % P, FP.value(b_aff[14:28]) * rinv % P) == pb
            assert ref.fp_norm_below(1)(b_aff[:14]) and ref.fp_norm_below(1)(b_aff[14:28]) and not any(b_aff[28:])
        for rec in (a, b):
            for i, k in enumerate(ref.STORED_K):
                tops[i] = max(tops[i], FP.value(rec[14 * i:14 * i + 14]) // P)
    assert tops == list(ref.STORED_K)                          # every coordinate reaches the top multiple of its class
    kinds = [(pa is None, pb is None, pa == pb, pa is not None and pb == o.g1_neg(pa)) for pa, pb, *_ in fam]
    assert {(False, False, True, False), (False, False, False, True), (True, False, False, False), (False, True, False, False),
            (True, True, True, False), (False, False, False, False)} <= set(kinds)
