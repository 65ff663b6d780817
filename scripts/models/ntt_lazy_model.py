"""Limb-exact model of ONE tile of an NTT pass (csrc/fr_ntt.hip, k_fr_ntt_pass: the radix-2 butterflies with their lazy sums) on top
of fr29_model.py.  It answers, in plain integers, what the documented lazy bounds of a pass are worth:

  * a zero vector: fr9_mul(0, w) is the representative 0 (all limbs zero), but fr9_mul(c r, w) is the representative r for every
    other multiple c r < 64 r of r and every w != 0 (the quotient digits come to R - c w, so the result is r ceil(c w / R) = r).
    Stage 0 of a first pass has no product and leaves 0 and 4r; from stage 1 on the 'minus' output of a pair of nonzero
    multiples is u + 4r - r.  The all-'minus' row of a first-pass tile therefore ends at exactly r (3 S + 1) -- 28 r at S = 9 --
    and not at the 4 r S that "a value grows by at most 4r per stage" allows: the zero vector is the input with the LARGEST
    limbs (nothing is subtracted from the K r constant in stage 0) but not one that rides the value bound.  Between passes the
    value goes through fr9_reduce_approx, which leaves the representative 0 or r.
  * the normalisation period: the kernel normalises every second stage ("limbs stay below 2^31").  What arithmetic needs is
    less: limbs that fit a 32-bit word and a product accumulator below 2^64.  worst_case(period) bounds both from the limb
    tables alone; a period of 3 still satisfies them (limbs < 2^29 + 3 * 2^30, accumulator < 2^64), so a kernel that normalised
    every third stage would return the same bytes for EVERY input: no test can tell it from the shipped one.  A period of 4 has
    no such guarantee (2^29 + 4 * (2^30 - 33) > 2^32: a large limb that meets four small product limbs in a row leaves the word).

    python scripts/models/ntt_lazy_model.py"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fr29_model import M4, MASK, N, R_MOD, RL, RR, canon, limbs, mul, norm, value  # noqa: E402

WORD = 1 << 32


def reduce_approx(a):
    """fr9_reduce_approx: normalised, < 64r -> the same residue below 2r"""
    m = (1 << 52) // (RL[8] + 1)
    q = (a[8] * m) >> 52
    out, carry = [], 0
    for i in range(N):
        acc = a[i] - q * RL[i] + carry
        out.append(acc & MASK if i < 8 else acc)
        carry = acc >> 29
    assert value(out) == value(a) - q * R_MOD and 0 <= value(out) < 2 * R_MOD
    return out


def mont(v):
    return limbs(v * RR % R_MOD)


def brev(v, bits):
    return int(format(v, f"0{bits}b")[::-1], 2) if bits else 0


def first_pass_tile(vals, log_n, period=2, stats=None):
    """the 2^S-point network of a first pass on one tile (S = log2(len(vals)) stages, twiddles of a 2^log_n transform): `vals`
    canonical Montgomery limb vectors in natural order of the SUB-transform; returns the lazy, normalised limb vectors"""
    S = len(vals).bit_length() - 1
    w = pow(7, (R_MOD - 1) >> log_n, R_MOD)
    tile = [list(vals[brev(i, S)]) for i in range(len(vals))]
    for l in range(S):
        half = 1 << l
        renorm = (S - 1 - l) % period == 0
        for i in range(len(tile)):
            if i & half:
                continue
            k = i & (half - 1)
            u, v = tile[i], tile[i + half]
            if stats is not None:
                stats["max_operand_limb"] = max(stats["max_operand_limb"], max(v))
            t = v if l == 0 else mul(v, mont(pow(w, k << (log_n - l - 1), R_MOD)), stats)
            a = [u[j] + t[j] for j in range(N)]
            b = [u[j] + (M4[j] - t[j]) for j in range(N)]
            for x in (a, b):
                if stats is not None:
                    stats["max_limb"] = max(stats["max_limb"], max(x))
                if max(x) >= WORD:
                    raise OverflowError(f"stage {l}: a limb leaves the 32-bit word")
            tile[i], tile[i + half] = (norm(a), norm(b)) if renorm else (a, b)
    return tile


def worst_case(period):
    """(largest limb before a normalisation, largest product accumulator) over ALL inputs, from the tables alone: a normalised limb is
    < 2^29, a stage adds at most max(M4) to a limb, the product's second operand and its quotient digits are < 2^29"""
    grow = max(M4[:8])
    limb = MASK + period * grow                      # `period` stages since the last normalisation, the last one included
    operand = MASK + (period - 1) * grow             # what the last of them multiplies
    acc = 9 * operand * MASK + 8 * MASK * max(RL) + (1 << 36)
    return limb, acc


def main():
    rnd = random.Random(11)
    zero, r_limbs = [0] * N, limbs(R_MOD)
    for _ in range(200):
        wv = mont(rnd.randrange(1, R_MOD))
        assert mul(zero, wv) == zero                 # the representative 0 stays 0 ...
        assert mul(r_limbs, wv) == r_limbs           # ... and the representative r stays r
        assert mul(limbs(rnd.randrange(1, 64) * R_MOD), wv) == r_limbs      # ... which every other multiple of r becomes
    for S in range(1, 10):
        tile = first_pass_tile([zero] * (1 << S), max(S, 2))
        assert max(value(x) for x in tile) == value(tile[-1]) == R_MOD * (3 * S + 1), S
        assert all(value(x) % R_MOD == 0 for x in tile)
        assert value(reduce_approx(tile[-1])) in (0, R_MOD)
    print("zero vector: row 2^S - 1 of a first-pass tile is exactly r (3 S + 1) for S = 1 .. 9 (28 r at S = 9; 4 r S is not reached)")
    for period in (2, 3, 4, 5):
        limb, acc = worst_case(period)
        print(f"normalising every {period}. stage: limbs < 2^{limb.bit_length()} ({'fit' if limb < WORD else 'LEAVE'} the word), "
              f"accumulator < 2^{acc.bit_length()} ({'fits' if acc < (1 << 64) else 'LEAVES'} 64 bits)")
    assert worst_case(2)[0] < WORD and worst_case(3)[0] < WORD and worst_case(3)[1] < (1 << 64) and worst_case(4)[0] >= WORD
    # ... and limb-exactly on inputs: the same canonical results at periods 2 and 3
    fams = {"zero": [0] * 256, "constant r-1": [R_MOD - 1] * 256, "uniform": [rnd.randrange(R_MOD) for _ in range(256)]}
    for name, a in fams.items():
        vals = [mont(v) for v in a]
        stats = {"max_acc": 0, "max_limb": 0, "max_operand_limb": 0}
        want = [value(canon(reduce_approx(x))) for x in first_pass_tile(vals, 8, 2)]
        got = [value(canon(reduce_approx(x))) for x in first_pass_tile(vals, 8, 3, stats)]
        assert got == want, name
        try:
            first_pass_tile(vals, 8, 4)
            four = "stays inside the word"
        except (OverflowError, AssertionError) as e:
            four = f"fails ({e})"
        print(f"{name}: period 3 gives period 2's values (largest limb 2^{stats['max_limb'].bit_length()}, largest operand limb "
              f"2^{stats['max_operand_limb'].bit_length()}, accumulator 2^{stats['max_acc'].bit_length()}); period 4 {four}")
    print("ntt lazy model ok")


if __name__ == "__main__":
    main()
