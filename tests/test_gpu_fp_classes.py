"""GPU parity tests (`-m gpu`), field layer at its class bounds: every operation of csrc/fp28.hip.h (Fp, 14 x 28-bit limbs),
csrc/fr29.hip.h (Fr, 9 x 29-bit limbs) and csrc/fp_lp.hip.h (one limb per lane of a DPP row), and the point formulas of g1.hip.h
on raw XYZZ coordinates, run on raw limbs through kzg_test_fp_raw / kzg_test_g1_raw -- no conversion in front of the operation
and none behind it -- on inputs that sit ON the documented bounds (tests/fp28_ref.py: class corners, both representatives of zero,
carry ripples of every length, every admitted multiple of p on a stored coordinate).  tests/test_fp_classes_cpu.py shows that the
inputs are inside the documented classes, so a mismatch here is the kernel's.  Every output limb is compared for equality with the
plain-integer reference, every point byte for byte with the oracle; no tolerance, no case filtered."""
import pytest

from oracle import bls12_381 as o
from tests import fp28_ref as ref

pytestmark = pytest.mark.gpu


def check_group(eng, group):
    for name in ref.GROUPS[group]:
        op = ref.OPS[name]
        fam, exp = ref.family(name), ref.expected(name)
        got = eng.test_fp_raw(op.field, op.code, *[[x[i] for x in fam] for i in range(op.arity)])
        assert len(got) == len(exp)
        bad = [j for j in range(len(exp)) if got[j] != exp[j]]
        print(f"{name}: {len(exp)} inputs, {len(bad)} mismatches")
        assert not bad, (f"{name}: {len(bad)} of {len(exp)} outputs differ, first at input {bad[0]}: operands "
                         f"{[[hex(v) for v in l] for l in fam[bad[0]]]} gave {[hex(v) for v in got[bad[0]]]}, expected "
                         f"{[hex(v) for v in exp[bad[0]]]}")


def test_fp_one_lane_products_at_the_loose_class_bounds(hip):
    """fp_mul / fp_sqr (call form) and fp_mul_inline / fp_sqr_inline: limbs up to 2^30 - 1, values up to 32p - 1, 0 and p"""
    check_group(hip(), "fp_one_lane")


def test_fp_mul2_inline_at_all_four_operand_bounds(hip):
    """(ab + cd) / R with one reduction: a, b at 1.5 * 2^29, c at 2^29 - 1, d at 2^28 - 1, values just under 10p, 18p, 8p, 2p"""
    check_group(hip(), "fp_mul2")


def test_fp_subtractions_and_helpers(hip):
    """fp_sub4 / 8 / 16 against subtrahends at 2p - 1 / 6p - 1 / 14p - 1, all-ones limbs and zero; fp_neg8, fp_canon, fp_canon_mont,
    fp_neg_canon; fp_is_zero_n on 0, p and their neighbours"""
    check_group(hip(), "fp_sub_and_helpers")


def test_lp_mul_four_rows_per_wave(hip):
    """the lane-parallel product, four independent elements per wave: class corners, zero operands and products whose closing
    normalisation needs 7 .. 13 rounds, shuffled so that different patterns share a wave (a row that leaked would show)"""
    check_group(hip(), "lp_mul")


def test_lp_norm_carry_ripples(hip):
    """lp_norm on raw 64-bit lane values: chains of every length 1 .. 12 from every lane, two chains in a row, lanes at the
    column bound 2^37 - 1, sums shaped like x3 of lp_add"""
    check_group(hip(), "lp_norm")


def test_fr_operations_at_the_lazy_class_bounds(hip):
    """fr9_mul with a first operand at limbs 2^31 - 1 / value 64r - 1 against the largest admitted second operand; fr9_sub4 /
    fr9_sub8; fr9_norm, fr9_reduce, fr9_reduce_approx on every k r - 1, k r, k r + 1 up to 64r"""
    check_group(hip(), "fr")


def test_point_formulas_do_not_depend_on_the_representative(hip):
    """g1_add<false / true>, g1_madd<false / true>, g1_dbl, lp_add, lp_dbl on (x z^2, y z^3, z^2, z^3) + multiples of p up to the
    stored classes (X + 13p, Y + 5p, ZZ + p, ZZZ + p): every representative pair gives the oracle's affine point, P + P, P + (-P)
    and infinity operands included (there the equal-x detection rests on fp_is_zero_n seeing p)"""
    eng = hip()
    fam = ref.point_family()
    a = [f[2] for f in fam]
    b = [f[3] for f in fam]
    b_aff = [f[4] for f in fam]
    memo = {}

    def oracle(kind, pa, pb):
        key = (kind, pa, pb)
        if key not in memo:
            memo[key] = o.g1_to_be96(o.g1_add(pa, pa) if kind == "dbl" else o.g1_add(pa, pb))
        return memo[key]

    for name, code in ref.G1_CODES.items():
        kind = "dbl" if name.endswith("dbl") else "add"
        second = None if kind == "dbl" else b_aff if "madd" in name else b
        got = eng.test_g1_raw(code, a, second)
        bad = [j for j, f in enumerate(fam) if got[96 * j:96 * j + 96] != oracle(kind, f[0], f[1])]
        print(f"{name}: {len(fam)} representative pairs, {len(bad)} mismatches")
        assert not bad, (f"{name}: {len(bad)} of {len(fam)} points differ from the oracle, first at point pair {bad[0] // 5}, "
                         f"representative choice {bad[0] % 5}")
