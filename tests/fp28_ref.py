"""Plain-integer reference of the two unsaturated-limb field representations (csrc/fp28.hip.h: Fp on 14 limbs of 28 bits,
R = 2^392; csrc/fr29.hip.h: Fr on 9 limbs of 29 bits, R = 2^261) and of the lane-parallel forms (csrc/fp_lp.hip.h), for the raw-limb
hooks kzg_test_fp_raw / kzg_test_g1_raw.  For fixed inputs a Montgomery result (ab + m p) / R with m = -ab p^-1 mod R is ONE integer
whatever the scanning order, and "limbs 0..n-2 normalised, the top limb keeps the excess" then fixes every output limb: all
comparisons are equalities.

Every operation is an `Op`: its code in the hook, its documented PRECONDITION on the inputs (limb bounds and value bounds), the
expected output limbs, its documented POSTCONDITION, and a seeded input family that sits on the class bounds: canonical edges, class
corners (every limb at its maximum, the value just under its bound), denormalised randoms, both representatives of zero and carry
ripples.  tests/test_fp_classes_cpu.py checks families and reference against the predicates and against the stand-alone models in
scripts/models/; tests/test_gpu_fp_classes.py runs the same inputs through the HIP code."""
import random
from collections import namedtuple

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
RMOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
U32 = 1 << 32


class Field:
    def __init__(self, w, n, mod):
        self.w, self.n, self.mod = w, n, mod
        self.mask = (1 << w) - 1
        self.R = 1 << (w * n)
        self.top = w * (n - 1)                      # bit offset of the top limb
        self.ninv = (-pow(mod, -1, self.R)) % self.R
        self.one = self.R % mod
        self.r2 = self.R * self.R % mod

    # ---- limbs
    def pack(self, v):
        """normalised limbs: limbs 0..n-2 < 2^w, the top limb keeps the excess"""
        return [(v >> (self.w * i)) & self.mask for i in range(self.n - 1)] + [v >> self.top]

    def value(self, l):
        return sum(x << (self.w * i) for i, x in enumerate(l))

    def denorm(self, v, kmax, rnd):
        """the limbs of v with up to kmax units of limb i+1 pushed down into limb i: limbs <= mask + kmax 2^w, same value
        (limbs(v, loose_bits, rnd) of scripts/models/lp_mul_model.py)"""
        l = self.pack(v)
        for i in range(self.n - 1):
            k = min(l[i + 1], rnd.randrange(kmax + 1))
            l[i + 1] -= k
            l[i] += k << self.w
        return l

    def corner(self, limb_max, bound):
        """limbs 0..n-2 at limb_max, the top limb the largest one <= limb_max that keeps the value below `bound`"""
        low = self.value([limb_max] * (self.n - 1))
        top = min(limb_max, (bound - 1 - low) >> self.top)
        assert top >= 0
        return [limb_max] * (self.n - 1) + [top]

    def normalise(self, l):
        """fp_norm / fr9_norm: sequential carry propagation in 32-bit words (a word that overflows is a broken precondition)"""
        out, c = [], 0
        for i in range(self.n - 1):
            v = l[i] + c
            assert v < U32
            out.append(v & self.mask)
            c = v >> self.w
        assert l[-1] + c < U32
        return out + [l[-1] + c]

    def is_normalised(self, l):
        return all(x <= self.mask for x in l[:-1]) and l[-1] < U32

    def dominating(self, k):
        """k * mod with limbs 0..n-2 >= 2^w - 1: limb-wise K - b never borrows against a normalised b (the M4 / M8 / M16 tables)"""
        e = self.pack(k * self.mod - ((1 << self.top) - 1))
        out = [self.mask + x for x in e[:-1]] + [e[-1]]
        assert self.value(out) == k * self.mod
        return out

    # ---- Montgomery
    def mont(self, a, b):
        """(a b + ((-a b mod^-1) mod R) mod) / R, exact"""
        return self.mont2(a, b, 0, 0)

    def mont2(self, a, b, c, d):
        t = a * b + c * d
        m = t * self.ninv % self.R
        assert (t + m * self.mod) % self.R == 0
        return (t + m * self.mod) // self.R

    def sub_norm(self, a, b, k):
        """fp_sub4 / 8 / 16 (k = 4 / 8 / 16) followed by the normalisation: limb-wise a + (M_k - b) in 32-bit words, then carries"""
        return self.normalise(self.sub_raw(a, b, k))

    def sub_raw(self, a, b, k):
        m = self.dominating(k)
        out = []
        for x, mi, y in zip(a, m, b):
            assert mi >= y and x + mi - y < U32
            out.append(x + mi - y)
        return out


FP = Field(28, 14, P)
FR = Field(29, 9, RMOD)
MASK = FP.mask

# the operation codes of kzg_test_fp_raw (include/kzg_mi355x_test.h)
FP_CODES = {"fp_mul": 0, "fp_mul_inline": 1, "fp_sqr": 2, "fp_sqr_inline": 3, "fp_mul2_inline": 4, "fp_sub4": 5, "fp_sub8": 6,
            "fp_sub16": 7, "fp_neg8": 8, "fp_canon": 9, "fp_canon_mont": 10, "fp_neg_canon": 11, "fp_is_zero_n": 12, "lp_mul": 13,
            "lp_norm": 14}
FR_CODES = {"fr9_mul": 0, "fr9_sub4": 1, "fr9_sub8": 2, "fr9_norm": 3, "fr9_reduce": 4, "fr9_reduce_approx": 5}
# kzg_test_g1_raw
G1_CODES = {"g1_add": 0, "g1_add_inl": 1, "g1_madd": 2, "g1_madd_inl": 3, "g1_dbl": 4, "lp_add": 5, "lp_dbl": 6}

# name, field (0 Fp / 1 Fr), hook code, number of operands, pre(*operand limbs) -> bool, ref(*operand limbs) -> output limbs,
# post(operands, output limbs) -> bool, family(rnd) -> list of operand tuples
Op = namedtuple("Op", "name field code arity pre ref post family")


# ------------------------------------------------------------------ predicates
def limbs_below(l, bound):
    return all(0 <= x < bound for x in l)


def in_class(F, l, limb_bound, value_bound, top_bound=None):
    """limbs 0..n-2 < limb_bound, top limb < top_bound (limb_bound when None), value < value_bound"""
    return (limbs_below(l[:-1], limb_bound) and 0 <= l[-1] < (limb_bound if top_bound is None else top_bound)
            and F.value(l) < value_bound)


def fp_loose(l):                # fp28.hip.h "loose": limbs < 2^30, value < 32p -- the legal product input
    return in_class(FP, l, 1 << 30, 32 * P)


def fp_lp_loose(l):             # fp_lp.hip.h lp_mul: limbs < 2^30 + 2^28, value < 32p
    return in_class(FP, l, (1 << 30) + (1 << 28), 32 * P)


def fp_norm_below(k):           # normalised limbs, value < k p
    return lambda l: in_class(FP, l, 1 << 28, k * P, U32)


def fp_class_n(l):              # fp28.hip.h "N": every product output
    return fp_norm_below(2)(l)


def fr_lazy(l):                 # fr29.hip.h "lazy": limbs < 2^31, value < 64r -- the legal FIRST operand of fr9_mul
    return in_class(FR, l, 1 << 31, 64 * RMOD)


def fr_norm_below(k):
    return lambda l: in_class(FR, l, 1 << 29, k * RMOD, U32)


def fr_class_n(l):
    return fr_norm_below(2)(l)


# a minuend of the limb-wise subtractions: the headers bound only the subtrahend.  The words are 32 bits wide and the dominating
# multiples have limbs < 2^(w+1) <= 2^30, so a_i + M_i - b_i + carry < 2^32 holds for every a_i < 2^31 (the longest chain in
# g1.hip.h, RR - PPP - 2Q, reaches 2^28 + 3 * 2^29 before its fp_norm).
def fp_minuend(l):
    return limbs_below(l, 1 << 31)


def fr_minuend(l):
    return limbs_below(l, 1 << 31)


# ------------------------------------------------------------------ family pieces
def fp_edges(bound_k):
    """canonical edges, and where the class (value < bound_k p) admits them p, p + 1, 2p - 1 and the largest admitted multiple"""
    e = [0, 1, P - 1, FP.one, FP.r2]
    e += [v for v in (P, P + 1, 2 * P - 1, (bound_k - 1) * P, bound_k * P - 1) if v < bound_k * P]
    return sorted(set(e))


def fr_edges(bound_k):
    e = [0, 1, RMOD - 1, FR.one, FR.r2]
    e += [v for v in (RMOD, RMOD + 1, 2 * RMOD - 1, (bound_k - 1) * RMOD, bound_k * RMOD - 1) if v < bound_k * RMOD]
    return sorted(set(e))


def fp_product_singles(rnd, limb_max=(1 << 30) - 1, bound_k=32, kmax=3):
    """operands of a product at the edges and corners of the loose class"""
    s = [FP.pack(v) for v in fp_edges(bound_k)]
    s.append(FP.corner(limb_max, bound_k * P))                         # every limb at its maximum, value just under the bound
    s.append([limb_max] * 13 + [0])                                    # the limb corner alone
    s.append(FP.pack(bound_k * P - 1))                                 # the value corner alone
    s.append([MASK] * 13 + [0x1A011])                                  # all-ones limbs
    s.append(FP.denorm(bound_k * P - 1, kmax, rnd))
    return s


def fp_product_family(rnd, n_random=1500):
    s = fp_product_singles(rnd)
    fam = [(a, b) for a in s for b in s]
    for _ in range(n_random):
        fam.append((FP.denorm(rnd.randrange(32 * P), 3, rnd), FP.denorm(rnd.randrange(32 * P), 3, rnd)))
    return fam


def fp_sqr_family(rnd, n_random=1500):
    return [(a,) for a in fp_product_singles(rnd)] + [(FP.denorm(rnd.randrange(32 * P), 3, rnd),) for _ in range(n_random)]


# fp_mul2_inline (fp28.hip.h): a, b limbs <= 1.5 * 2^29, c limbs < 2^29, d limbs < 2^28; a < 10p, b < 18p, c < 8p, d < 2p
MUL2_LIMB = (3 << 28, (3 << 28), (1 << 29) - 1, (1 << 28) - 1)          # the largest admitted limb of a, b, c, d
MUL2_K = (10, 18, 8, 2)
MUL2_KMAX = (2, 2, 1, 0)                                                # denormalisation that stays inside the limb bounds


def fp_mul2_pre(a, b, c, d):
    return all(in_class(FP, x, lm + 1, k * P) for x, lm, k in zip((a, b, c, d), MUL2_LIMB, MUL2_K))


def fp_mul2_family(rnd, n_random=1500):
    choices = []
    for lm, k, km in zip(MUL2_LIMB, MUL2_K, MUL2_KMAX):
        choices.append([FP.corner(lm, k * P),            # limb bound and value bound at once
                        [lm] * 13 + [0],                 # limb bound alone
                        FP.pack(k * P - 1),              # value bound alone
                        FP.pack(0), FP.pack(P), FP.pack(FP.one),
                        FP.denorm(rnd.randrange(k * P), km, rnd)])
    fam = [(a, b, c, d) for a in choices[0] for b in choices[1] for c in choices[2] for d in choices[3]]
    for _ in range(n_random):
        fam.append(tuple(FP.denorm(rnd.randrange(k * P), km, rnd) for k, km in zip(MUL2_K, MUL2_KMAX)))
    return fam


def subtrahends(F, bound_k, rnd, n_random):
    """normalised limbs, value < bound_k * mod: zero, the edges, the bound itself, all-ones limbs"""
    s = [F.pack(v) for v in (fp_edges(bound_k) if F is FP else fr_edges(bound_k))]
    s.append(F.corner(F.mask, bound_k * F.mod))                         # all-ones limbs, the largest admitted top limb
    s.append([F.mask] * (F.n - 1) + [0])
    s += [F.pack(rnd.randrange(bound_k * F.mod)) for _ in range(n_random)]
    return s


def minuends(F, rnd, n_random):
    s = [F.pack(0), [(1 << 31) - 1] * F.n, [(1 << 30) - 1] * F.n, F.pack(F.mod - 1), F.pack(F.one)]
    bound = 32 * P if F is FP else 64 * RMOD
    s += [F.denorm(rnd.randrange(bound), 3, rnd) for _ in range(n_random)]
    return s


def sub_family(F, bound_k):
    def family(rnd):
        a_s, b_s = minuends(F, rnd, 12), subtrahends(F, bound_k, rnd, 12)
        fam = [(a, b) for a in a_s for b in b_s]
        fam += [(F.denorm(rnd.randrange(32 * F.mod), 3, rnd), F.pack(rnd.randrange(bound_k * F.mod))) for _ in range(1500)]
        return fam
    return family


def fp_canon_family(rnd):
    s = [FP.pack(v) for v in fp_edges(2)] + [FP.corner(MASK, 2 * P), [MASK] * 13 + [0]]
    s += [FP.pack(P + d) for d in (-2, 2)] + [FP.pack(P - (1 << (28 * k))) for k in range(1, 14)]
    s += [FP.pack(P + (1 << (28 * k))) for k in range(1, 14)]
    s += [FP.pack(rnd.randrange(2 * P)) for _ in range(1500)]
    return [(a,) for a in s]


def fp_neg_canon_family(rnd):
    s = [0, 1, 2, P - 1, P - 2, FP.one, FP.r2, (P + 1) // 2]
    for k in range(1, 14):                                             # borrow chains: low limbs equal to p's, or zero, or one above
        low = P & ((1 << (28 * k)) - 1)
        s += [low, low + 1, low - 1, 1 << (28 * k), (1 << (28 * k)) - 1, P - (1 << (28 * k)), P - low]
    s += [rnd.randrange(P) for _ in range(1500)]
    return [(FP.pack(v % P),) for v in s]


def fp_is_zero_family(rnd):
    s = [FP.pack(v) for v in (0, P, 1, P - 1, P + 1, 2 * P - 1, 2, P - 2, P + 2, FP.one, FP.r2)]
    for i in range(14):                                                # near misses of both representatives, limb by limb
        for base in (0, P):
            for near in (lambda x: x + 1, lambda x: x - 1, lambda x: x ^ (1 << 27 if i < 13 else 1 << 10)):
                l = FP.pack(base)
                l[i] = near(l[i])
                if fp_class_n(l):
                    s.append(l)
    s += [FP.pack(rnd.randrange(2 * P)) for _ in range(500)]
    return [(a,) for a in s]


# ------------------------------------------------------------------ lane-parallel forms
LP_COLUMN_MAX = (1 << 37) - 1                                           # the model's column bound (scripts/models/lp_mul_model.py)


def lp_norm_model(t):
    """fp_lp.hip.h lp_norm on 14 lane values (lanes 14 / 15 hold zero): (limbs, number of carry rounds executed)"""
    t = list(t)
    rounds = 0
    while any(x > MASK for x in t[:13]):
        lo = [(x & MASK) if j < 13 else x % U32 for j, x in enumerate(t)]
        hi = [(x >> 28) if j < 13 else 0 for j, x in enumerate(t)]
        assert all(h < U32 for h in hi)
        t = [lo[j] + (hi[j - 1] if j else 0) for j in range(14)]
        rounds += 1
    return [x % U32 for x in t], rounds


def lp_mul_model(a, b):
    """fp_lp.hip.h lp_mul, operand scanning across the row: (limbs, carry rounds of the closing lp_norm)"""
    pl = FP.pack(P)
    pinv = FP.ninv & MASK
    t = [0] * 14
    for i in range(14):
        t = [t[j] + a[j] * b[i] for j in range(14)]
        q = ((t[0] % U32) * pinv) & MASK
        t = [t[j] + q * pl[j] for j in range(14)]
        assert max(t) < (1 << 64) and t[0] & MASK == 0
        t = [(t[j] >> 28) + ((t[j + 1] & MASK) if j < 13 else 0) for j in range(14)]
    assert max(t) <= LP_COLUMN_MAX
    return lp_norm_model(t)


def lp_norm_pre(lo, hi):
    t = [l | (h << 32) for l, h in zip(lo, hi)]
    return limbs_below(t[:13], LP_COLUMN_MAX + 1) and FP.value(t) >> FP.top < U32


def lp_norm_ref(lo, hi):
    t = [l | (h << 32) for l, h in zip(lo, hi)]
    return FP.pack(FP.value(t))


def lanes64(t):
    return [x & (U32 - 1) for x in t], [x >> 32 for x in t]


def ripple(start, length, x=5, top=0x1234, fill=0x0123456):
    """a carry chain: lane `start` overflows by one unit, the next `length` lanes hold 2^28 - 1, so the carry moves one lane per
    round: length + 1 rounds (the chain ends in lane 13, which only receives, or in a lane that absorbs it)"""
    assert 0 <= start and start + length <= 13
    t = [fill] * 13 + [top]
    t[start] = (1 << 28) + x
    for j in range(start + 1, start + 1 + length):
        if j < 13:
            t[j] = MASK
    return t


def lp_norm_family(rnd):
    fam = [ripple(0, 12)]                                               # [2^28 + x, MASK, ..., MASK, top]: 12 further rounds
    fam += [ripple(s, 12 - s) for s in range(13)]                       # the same chain started at every lane 0..12
    fam += [ripple(0, n) for n in range(1, 13)] + [ripple(3, n) for n in range(1, 10)]   # chains of every length 1..12
    for s1, n1, s2, n2 in ((0, 3, 6, 4), (0, 5, 7, 5), (1, 1, 4, 8), (2, 4, 8, 4)):      # two disjoint chains in one row
        t = ripple(s1, n1)
        u = ripple(s2, n2)
        fam.append(t[:s2] + u[s2:])
    fam.append([LP_COLUMN_MAX] * 13 + [0x1A011])                        # every lane at the column bound
    fam.append([LP_COLUMN_MAX] * 13 + [U32 - 1 - (LP_COLUMN_MAX >> 28) - 1])   # ... and the top word filled to its last unit
    fam.append([0] * 14)
    fam.append([MASK] * 13 + [7])                                       # already normalised: no round
    fam += [[(1 << 28) + MASK * (j == s) for j in range(13)] + [1] for s in range(13)]
    for _ in range(40):                                                 # a large head over a chain: the carry is wider than one bit
        s = rnd.randrange(12)
        t = ripple(s, 12 - s, x=rnd.randrange(1 << 20))
        t[s] = rnd.randrange(1 << 28, LP_COLUMN_MAX + 1)
        fam.append(t)
    m4 = FP.dominating(4)
    ones = [MASK] * 13 + [0x34021]
    for rr, ppp, q in [(ones, FP.pack(0), FP.pack(0)), (FP.pack(0), ones, ones), (ones, ones, ones),
                       (FP.pack(2 * P - 1), FP.pack(0), FP.pack(2 * P - 1))]:
        fam.append([rr[j] + (m4[j] - ppp[j]) + 2 * (m4[j] - q[j]) for j in range(14)])
    for _ in range(600):                                                # sums shaped like x3 of lp_add: RR + (M4 - PPP) + 2 (M4 - Q)
        rr, ppp, q = (FP.pack(rnd.randrange(2 * P)) for _ in range(3))
        fam.append([rr[j] + (m4[j] - ppp[j]) + 2 * (m4[j] - q[j]) for j in range(14)])
    for _ in range(600):
        fam.append([rnd.randrange(LP_COLUMN_MAX + 1) for _ in range(13)] + [rnd.randrange(1 << 22)])
    # four different patterns share the four rows of a wave: the order interleaves chains, flat rows and random rows
    rnd.shuffle(fam)
    return [lanes64(t) for t in fam]


def lp_zero_run_products(rnd, n_per_target=3):
    """operand pairs whose product has a run of zero limbs: a = target R / b mod p for a random b.  A zero limb of the normalised
    result that sits under a nonzero incoming carry (the columns before lp_norm are ~2^36, so every lane hands ~2^8 upwards) can only
    come from a lane that wraps at 2^28, and the unit which that emits meets 2^28 - 1 in the next zero limb: k zero limbs in a row
    take k + 1 rounds of lp_norm.  The result is the target itself when target >= a b / R; a, b < 9p makes a b / R < 2^-4 p, so
    every target carries a top limb of at least 0x2000."""
    targets = [(0x1A011 << 364) + 9]                                                    # limbs 1..12 zero: 13 rounds
    targets += [(0x2000 << 364) + (1 << (28 * k)) for k in range(13)]                   # two runs, every split
    targets += [(0x9000 << 364) + (0xABCDEF << (28 * s)) + 7 for s in (3, 6, 9)]
    fam = []
    for tgt in targets:
        for _ in range(n_per_target):
            b = rnd.randrange(1, P)
            a = tgt * FP.R % P * pow(b, -1, P) % P
            k = rnd.randrange(3)
            fam.append((FP.denorm(a + rnd.randrange(8) * P, k, rnd), FP.denorm(b + rnd.randrange(8) * P, k, rnd)))
    return fam


def lp_mul_family(rnd):
    lp_max = (1 << 30) + (1 << 28) - 1
    s = fp_product_singles(rnd) + [FP.corner(lp_max, 32 * P), [lp_max] * 13 + [0]]
    fam = [(a, b) for a in s for b in s]
    fam += lp_zero_run_products(rnd)
    for _ in range(1200):
        fam.append((FP.denorm(rnd.randrange(32 * P), 4, rnd), FP.denorm(rnd.randrange(32 * P), 4, rnd)))
    rnd.shuffle(fam)                  # corners, zero runs and randoms share waves; the count is left as it falls (no multiple of 4 needed)
    return fam


# ------------------------------------------------------------------ Fr
def fr_mul_pre(a, b):
    return fr_lazy(a) and limbs_below(b, 1 << 29) and FR.value(a) * FR.value(b) < FR.R * RMOD


def fr_second_max(a):
    """the largest second operand of fr9_mul beside a: all nine limbs < 2^29 and a b < 2^261 r"""
    va = FR.value(a)
    return min(FR.R - 1, (FR.R * RMOD - 1) // va) if va else FR.R - 1


def fr_mul_family(rnd):
    firsts = [FR.pack(v) for v in fr_edges(64)]
    firsts.append(FR.corner((1 << 31) - 1, 64 * RMOD))                  # limbs 2^31 - 1 and value just under 64r
    firsts.append([(1 << 31) - 1] * 8 + [0])
    firsts.append(FR.denorm(64 * RMOD - 1, 3, rnd))
    fam = []
    for a in firsts:
        bmax = fr_second_max(a)
        for v in (0, 1, RMOD - 1, RMOD, RMOD + 1, 2 * RMOD - 1, FR.one, FR.r2, FR.value([FR.mask] * 9), bmax, bmax - 1):
            if 0 <= v <= bmax:
                fam.append((a, FR.pack(v)))
    for _ in range(2000):
        a = FR.denorm(rnd.randrange(64 * RMOD), 3, rnd)
        fam.append((a, FR.pack(rnd.randrange(fr_second_max(a) + 1))))
    return fam


def fr_lazy_family(rnd, normalised):
    s = []
    for k in range(1, 65):
        s += [k * RMOD - 1, k * RMOD, k * RMOD + 1]
    s = [0, 1, FR.one, FR.r2] + [v for v in s if v < 64 * RMOD]
    fam = [FR.pack(v) for v in s] + [FR.corner(FR.mask, 64 * RMOD), [FR.mask] * 8 + [0]]
    if not normalised:
        fam += [FR.corner((1 << 31) - 1, 64 * RMOD), [(1 << 31) - 1] * 8 + [0], [(1 << 29) + 5] + [FR.mask] * 7 + [3]]
        fam += [[FR.mask] * s0 + [(1 << 29) + 1] + [FR.mask] * (7 - s0) + [9] for s0 in range(8)]
        fam += [FR.denorm(v, 3, rnd) for v in s]
    for _ in range(1500):
        v = rnd.randrange(64 * RMOD)
        fam.append(FR.pack(v) if normalised else FR.denorm(v, 3, rnd))
    return [(a,) for a in fam]


def fr_reduce_approx_ref(a):
    """fr9_reduce_approx: the quotient estimated from limb 8, then v - q r"""
    m = (1 << 52) // ((RMOD >> 232) + 1)
    q = (a[8] * m) >> 52
    v = FR.value(a) - q * RMOD
    assert v >= 0
    return FR.pack(v)


# ------------------------------------------------------------------ the operations
def _mont_op(F, name, code, pre, family, square=False):
    def ref(*ops):
        a = F.value(ops[0])
        return F.pack(F.mont(a, a if square else F.value(ops[1])))

    def post(ops, out):
        a = F.value(ops[0])
        b = a if square else F.value(ops[1])
        cls = fp_class_n if F is FP else fr_class_n
        return cls(out) and (F.value(out) * F.R - a * b) % F.mod == 0
    return Op(name, 0 if F is FP else 1, code, 1 if square else 2, pre, ref, post, family)


def _sub_op(F, name, code, k, bound_k, normalised):
    minu, below = (fp_minuend, fp_norm_below) if F is FP else (fr_minuend, fr_norm_below)

    def ref(a, b):
        return F.sub_norm(a, b, k) if normalised else F.sub_raw(a, b, k)

    def post(ops, out):
        a, b = ops
        return (F.value(out) == F.value(a) + k * F.mod - F.value(b) and limbs_below(out, U32)
                and (not normalised or F.is_normalised(out)))
    return Op(name, 0 if F is FP else 1, code, 2, lambda a, b: minu(a) and below(bound_k)(b), ref, post, sub_family(F, bound_k))


def _canon(F, v):
    return F.pack(v - F.mod if v >= F.mod else v)


def build_ops():
    ops = []
    both = lambda a, b: fp_loose(a) and fp_loose(b)     # noqa: E731
    for name in ("fp_mul", "fp_mul_inline"):
        ops.append(_mont_op(FP, name, FP_CODES[name], both, fp_product_family))
    for name in ("fp_sqr", "fp_sqr_inline"):
        ops.append(_mont_op(FP, name, FP_CODES[name], fp_loose, fp_sqr_family, square=True))
    ops.append(Op("fp_mul2_inline", 0, FP_CODES["fp_mul2_inline"], 4, fp_mul2_pre,
                  lambda a, b, c, d: FP.pack(FP.mont2(*(FP.value(x) for x in (a, b, c, d)))),
                  lambda o, out: fp_class_n(out) and (FP.value(out) * FP.R - FP.value(o[0]) * FP.value(o[1])
                                                      - FP.value(o[2]) * FP.value(o[3])) % P == 0,
                  fp_mul2_family))
    ops.append(_sub_op(FP, "fp_sub4", FP_CODES["fp_sub4"], 4, 2, True))
    ops.append(_sub_op(FP, "fp_sub8", FP_CODES["fp_sub8"], 8, 6, True))
    ops.append(_sub_op(FP, "fp_sub16", FP_CODES["fp_sub16"], 16, 14, True))
    m8 = FP.dominating(8)
    ops.append(Op("fp_neg8", 0, FP_CODES["fp_neg8"], 1, fp_norm_below(6),
                  lambda b: [m - x for m, x in zip(m8, b)],
                  lambda o, out: limbs_below(out, 1 << 29) and FP.value(out) == 8 * P - FP.value(o[0]) and FP.value(out) <= 8 * P,
                  lambda rnd: [(b,) for b in subtrahends(FP, 6, rnd, 1500)]))
    ops.append(Op("fp_canon", 0, FP_CODES["fp_canon"], 1, fp_class_n, lambda a: _canon(FP, FP.value(a)),
                  lambda o, out: fp_norm_below(1)(out) and (FP.value(out) - FP.value(o[0])) % P == 0, fp_canon_family))
    ops.append(Op("fp_canon_mont", 0, FP_CODES["fp_canon_mont"], 1, fp_loose,
                  lambda a: _canon(FP, FP.mont(FP.value(a), FP.one)),
                  lambda o, out: fp_norm_below(1)(out) and (FP.value(out) - FP.value(o[0])) % P == 0, fp_sqr_family))
    ops.append(Op("fp_neg_canon", 0, FP_CODES["fp_neg_canon"], 1, fp_norm_below(1),
                  lambda a: FP.pack((P - FP.value(a)) % P),
                  lambda o, out: fp_norm_below(1)(out) and (FP.value(out) + FP.value(o[0])) % P == 0, fp_neg_canon_family))
    ops.append(Op("fp_is_zero_n", 0, FP_CODES["fp_is_zero_n"], 1, fp_class_n,
                  lambda a: [int(FP.value(a) % P == 0)] + [0] * 13,
                  lambda o, out: out[0] in (0, 1) and not any(out[1:]), fp_is_zero_family))
    ops.append(_mont_op(FP, "lp_mul", FP_CODES["lp_mul"], lambda a, b: fp_lp_loose(a) and fp_lp_loose(b), lp_mul_family))
    ops.append(Op("lp_norm", 0, FP_CODES["lp_norm"], 2, lp_norm_pre, lp_norm_ref,
                  lambda o, out: FP.is_normalised(out) and out == lp_norm_ref(*o), lp_norm_family))

    ops.append(_mont_op(FR, "fr9_mul", FR_CODES["fr9_mul"], fr_mul_pre, fr_mul_family))
    ops.append(_sub_op(FR, "fr9_sub4", FR_CODES["fr9_sub4"], 4, 2, False))
    ops.append(_sub_op(FR, "fr9_sub8", FR_CODES["fr9_sub8"], 8, 6, False))
    ops.append(Op("fr9_norm", 1, FR_CODES["fr9_norm"], 1, fr_lazy, lambda a: FR.normalise(a),
                  lambda o, out: FR.is_normalised(out) and FR.value(out) == FR.value(o[0]),
                  lambda rnd: fr_lazy_family(rnd, False)))
    ops.append(Op("fr9_reduce", 1, FR_CODES["fr9_reduce"], 1, fr_lazy, lambda a: FR.pack(FR.value(a) % RMOD),
                  lambda o, out: fr_norm_below(1)(out) and (FR.value(out) - FR.value(o[0])) % RMOD == 0,
                  lambda rnd: fr_lazy_family(rnd, False)))
    ops.append(Op("fr9_reduce_approx", 1, FR_CODES["fr9_reduce_approx"], 1, fr_norm_below(64), fr_reduce_approx_ref,
                  lambda o, out: fr_class_n(out) and (FR.value(out) - FR.value(o[0])) % RMOD == 0,
                  lambda rnd: fr_lazy_family(rnd, True)))
    return {op.name: op for op in ops}


OPS = build_ops()
GROUPS = {                                                              # one GPU test per group
    "fp_one_lane": ["fp_mul", "fp_mul_inline", "fp_sqr", "fp_sqr_inline"],
    "fp_mul2": ["fp_mul2_inline"],
    "fp_sub_and_helpers": ["fp_sub4", "fp_sub8", "fp_sub16", "fp_neg8", "fp_canon", "fp_canon_mont", "fp_neg_canon", "fp_is_zero_n"],
    "lp_mul": ["lp_mul"],
    "lp_norm": ["lp_norm"],
    "fr": ["fr9_mul", "fr9_sub4", "fr9_sub8", "fr9_norm", "fr9_reduce", "fr9_reduce_approx"],
}
_FAMILIES = {}


def family(name):
    """the seeded input family of an operation (built once, shared by the CPU and the GPU tests, never modified)"""
    if name not in _FAMILIES:
        _FAMILIES[name] = OPS[name].family(random.Random("fp28_ref:" + name))
    return _FAMILIES[name]


_EXPECTED = {}


def expected(name):
    if name not in _EXPECTED:
        op = OPS[name]
        _EXPECTED[name] = [op.ref(*x) for x in family(name)]
    return _EXPECTED[name]


# ------------------------------------------------------------------ points on raw XYZZ coordinates
STORED_K = (13, 5, 1, 1)        # g1.hip.h stored classes: X < 14p, Y < 6p, ZZ / ZZZ < 2p -> the largest multiple of p to add


def xyzz_of(pt, z, ks):
    """4 x 14 normalised limbs of (x z^2, y z^3, z^2, z^3) in Montgomery form, each residue plus ks[i] p; infinity: zeros"""
    if pt is None:
        return [0] * 56
    x, y = pt
    z2, z3 = z * z % P, z * z * z % P
    out = []
    for v, k, kmax in zip((x * z2, y * z3, z2, z3), ks, STORED_K):
        assert 0 <= k <= kmax
        out += FP.pack(v * FP.R % P + k * P)
    return out


def aff_of(pt):
    """the affine operand of g1_madd: canonical Montgomery x, y (2 x 14 limbs), padded to the 56 words of the hook's record"""
    if pt is None:
        return [0] * 56
    return FP.pack(pt[0] * FP.R % P) + FP.pack(pt[1] * FP.R % P) + [0] * 28


def stored_pre(l56):
    """the stored-coordinate classes (or the all-zero infinity)"""
    c = [l56[14 * i:14 * i + 14] for i in range(4)]
    if not any(l56):
        return True
    return all(fp_norm_below(k + 1)(x) for x, k in zip(c, STORED_K)) and FP.value(c[2]) % P != 0


def point_family():
    """64 point pairs (random, P + P, P + (-P), infinity operands) times five choices of representative: (a affine, b affine,
    a XYZZ limbs, b XYZZ limbs, b affine limbs)"""
    from oracle import bls12_381 as o

    rnd = random.Random("fp28_ref:points")
    tb = o.g1_table()
    pairs = []
    for i in range(64):
        pa, pb = tb.mul(rnd.randrange(1, o.R)), tb.mul(rnd.randrange(1, o.R))
        if 40 <= i < 48:
            pb = pa                                                     # P + P: the two sides carry different representatives
        elif 48 <= i < 56:
            pb = o.g1_neg(pa)
        elif 56 <= i < 59:
            pa = None
        elif 59 <= i < 62:
            pb = None
        elif i >= 62:
            pa = pb = None
        pairs.append((pa, pb))
    fam = []
    for pa, pb in pairs:
        for rep in range(5):
            if rep == 0:
                ka, kb = (0, 0, 0, 0), (0, 0, 0, 0)
            elif rep == 1:
                ka, kb = STORED_K, STORED_K                              # every coordinate in the top multiple of its class
            elif rep == 2:
                ka, kb = STORED_K, (0, 0, 0, 0)
            else:
                ka, kb = (tuple(rnd.randrange(k + 1) for k in STORED_K) for _ in range(2))
            za, zb = (1 if rep == 0 else rnd.randrange(1, P)), rnd.randrange(1, P)
            fam.append((pa, pb, xyzz_of(pa, za, ka), xyzz_of(pb, zb, kb), aff_of(pb)))
    return fam
