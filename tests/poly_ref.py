"""Reference, input families, points and level plans of the opening-scan tests (tests/test_poly_plans_cpu.py,
tests/test_gpu_poly_plans.py).  Plain Python integers; nothing here needs a device.

The operation by its definition: y = f(alpha) by Horner's rule and q = (f - y) / (X - alpha) by synthetic division, n - 1 coefficients
and a zero in slot n - 1 (the quotient rides as a length-n scalar set).  Every input family carries its closed form where one
exists, so that most expectations come from no division code at all.

A plan is (l0, scan_max, scan_nt, lds) (csrc/fr_kernels.hip.h, PolyPlan): level 0 folds chunks of 2^l0 coefficients, every level
above it chunks of 16 values, until at most scan_max values are left for one workgroup of scan_nt lanes; lds picks the LDS-staged
quotient kernel.  `levels` is the launcher's arithmetic as it stood before plan and execution were separated, `plan_invalid` the
kernels' preconditions, `signatures` what the single kernel instances of a run can tell apart, and `covering_plans` for every
signature that a production plan of any admitted length holds, in any of the six forms of kzg_test_poly_run, the first plan of a fixed
ascending list of candidate lengths (all of them <= 2^17) that holds it too."""
import random
from functools import lru_cache

from oracle.bls12_381 import R
from tests.ntt_ref import EDGE_POOL, to_bytes

MONT = (1 << 261) % R                # the device's Montgomery radix (csrc/fr29.hip.h: nine limbs of 29 bits)
MAX_LOG = 28                         # the longest rows production plans are enumerated for (as the NTT's plans)
CAP = 1 << 17                        # no covering plan is longer
LUP = 4                              # log2 chunk of the levels above the first
FORMS = {0: "open", 1: "eval", 2: "rows", 3: "pairs", 4: "points", 5: "chain"}
PRODUCTION = (-1, -1, -1, -1)


# ------------------------------------------------------------------------------------------------------------- the operation
def horner(f, alpha):
    s = 0
    for c in reversed(f):
        s = (s * alpha + c) % R
    return s


def open_at(f, alpha):
    """(y, q): q[j - 1] = sum_{k >= j} f_k alpha^(k - j) for 1 <= j < n, q[n - 1] = 0; y = the same sum at j = 0"""
    n = len(f)
    q, s = [0] * n, 0
    for j in range(n - 1, 0, -1):
        s = (s * alpha + f[j]) % R
        q[j - 1] = s
    return (s * alpha + f[0]) % R, q


def words_to_ints(raw):
    """the raw quotient buffer (8 little-endian 32-bit words per element) as integers"""
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


# ------------------------------------------------------------------------------------------------------------------ families
class Family:
    """One seeded coefficient vector.  closed(alpha): (y, q) in closed form, or None where there is none (or none at this
    alpha).  point: the family's own point, where it has one (it then runs there instead of at the random point)."""

    def __init__(self, name, f, closed=None, point=None):
        self.name, self.f, self._closed, self.point = name, f, closed, point

    def closed(self, alpha):
        return self._closed(alpha) if self._closed else None


def _geometric_sum(x, k):
    """sum_{t < k} x^t"""
    return k % R if x == 1 else (pow(x, k, R) - 1) * pow(x - 1, -1, R) % R


def _geometric(n, c, g):
    """f_k = c g^k: q[j - 1] = c g^j sum_{t < n - j} (g alpha)^t"""
    def closed(alpha):
        x = g * alpha % R
        q = [c * pow(g, j, R) * _geometric_sum(x, n - j) % R for j in range(1, n)] + [0]
        return c * _geometric_sum(x, n) % R, q
    return closed


def _delta(n, j, v):
    """v X^j: y = v alpha^j, q = v (alpha^(j - 1), ..., alpha, 1, 0, ...)"""
    def closed(alpha):
        return v * pow(alpha, j, R) % R, [v * pow(alpha, j - 1 - i, R) % R if i < j else 0 for i in range(n)]
    return closed


@lru_cache(maxsize=64)
def families(n):
    """name -> Family for n coefficients, in a fixed order"""
    rnd = random.Random(0x9017 + n)
    fams = [Family("zero", [0] * n, lambda alpha: (0, [0] * n)),
            Family("constant r-1", [R - 1] * n, _geometric(n, R - 1, 1))]
    for j in sorted({0, n // 3, n - 1}):
        fams.append(Family(f"delta r-1 at {j}", [R - 1 if i == j else 0 for i in range(n)], _delta(n, j, R - 1)))
    g = rnd.randrange(2, R)
    pw, cur = [], 1
    for _ in range(n):
        pw.append(cur)
        cur = cur * g % R
    fams.append(Family("geometric", pw, _geometric(n, 1, g)))
    # (X - a) g for a seeded a, run AT a: y = 0 and q = g, every suffix value a representative of a multiple of (X - a)
    a, gq = rnd.randrange(R), [rnd.randrange(R) for _ in range(n - 1)]
    mult = [(-a * gq[0]) % R] + [(gq[k - 1] - a * gq[k]) % R for k in range(1, n - 1)] + [gq[n - 2]] if n >= 2 else [0]
    fams.append(Family("multiple of X - a", mult, lambda alpha: (0, gq + [0]) if alpha == a else None, point=a))
    # the largest lazy running values of the chunk loops and of the Hillis-Steele scan: every coefficient, alpha and so every
    # power of alpha at r - 1 or 1
    fams.append(Family("all r-1 at r-1", [R - 1] * n, _geometric(n, R - 1, 1), point=R - 1))
    fams.append(Family("edge pool", [EDGE_POOL[(i + n) % len(EDGE_POOL)] for i in range(n)]))
    fams.append(Family("uniform", [rnd.randrange(R) for _ in range(n)]))
    return {f.name: f for f in fams}


def points(n):
    """name -> point: a seeded one, 0, 1, r - 1, a primitive root of unity of the padded length, 2"""
    log_n = max(n - 1, 0).bit_length()
    return {"random": random.Random(0xA1FA + n).randrange(R), "0": 0, "1": 1, "r-1": R - 1,
            "root of unity": pow(7, (R - 1) >> log_n, R), "2": 2}


@lru_cache(maxsize=256)
def expected(n, name, alpha):
    """(y, q) of family `name` at alpha by Horner and synthetic division -- computed once, shared, never changed (tuples)"""
    y, q = open_at(families(n)[name].f, alpha)
    return y, tuple(q)


@lru_cache(maxsize=256)
def input_bytes(n, name):
    return to_bytes(families(n)[name].f)


# --------------------------------------------------------------------------------------------------------------------- plans
def lchunk(n):
    l = 2
    while l < 4 and (n >> (l + 1)) >= 16384:
        l += 1
    return l


def levels(n, l0, scan_max):
    """poly_up's level arithmetic as it stood inside the launcher, line by line: K, and l / sq / n / off of levels 0 .. K"""
    l, sq, cnt, off = [l0], [0], [n], [0]
    cnt.append((n + (1 << l0) - 1) >> l0)
    sq.append(l0)
    off.append(0)
    K = 1
    while cnt[K] > scan_max and K < 14:
        l.append(LUP)
        cnt.append((cnt[K] + (1 << LUP) - 1) >> LUP)
        sq.append(sq[K] + LUP)
        off.append(off[K] + cnt[K])
        K += 1
    l.append(0)
    return {"K": K, "l": l, "sq": sq, "n": cnt, "off": off}


def production_plan(n, no_lds=False, lds_min_log=21):
    """what the launchers picked for n: (l0, 2048, 256 or 1024 lanes, lds)"""
    l0 = lchunk(n)
    lv = levels(n, l0, 2048)
    return (l0, 2048, 256 if lv["n"][lv["K"]] <= 1024 else 1024,
            int(not no_lds and l0 == 4 and n % 1024 == 0 and n >= 1 << lds_min_log))


def plan_of(n, plan):
    """the dictionary kzg_test_poly_plan_of answers with"""
    l0, scan_max, scan_nt, lds = production_plan(n) if plan == PRODUCTION else plan
    return dict(levels(n, l0, scan_max), scan_nt=scan_nt, lds=lds)


def level_words(n):
    return ((n + 3) // 4 + (n + 3) // 4 // 2 + 64) * 8


def plan_invalid(n, plan):
    """the kernels' preconditions (csrc/fr_poly.hip, poly_plan_invalid), restated; None: valid"""
    l0, scan_max, scan_nt, lds = plan
    if n < 1:
        return "no coefficients"
    if l0 not in (2, 3, 4):
        return "l0"
    if scan_max < 1:
        return "scan_max"
    if scan_nt not in (256, 1024):
        return "scan_nt"
    lv = levels(n, l0, scan_max)
    if lv["n"][lv["K"]] > scan_max:
        return "levels"
    if lds not in (0, 1) or (lds and (l0 != 4 or n % 1024 or n < 1024)):
        return "lds"
    if (lv["off"][lv["K"]] + lv["n"][lv["K"]]) * 8 > level_words(n):
        return "scratch"
    return None


def plan_name(n, plan):
    if plan == PRODUCTION:
        return f"n={n} production"
    return f"n={n} l0={plan[0]} scan_max={plan[1]} scan_nt={plan[2]}" + (" lds" if plan[3] else "")


# ---------------------------------------------------------------------------------------------------------------- signatures
_GRID = {0: "single", 1: "single", 2: "rows", 3: "pairs", 4: "pairs", 5: "pairs"}


def signatures(n, plan, form):
    """What the kernel instances of one run can distinguish:
      ("level", ARG, lchunk, partial last chunk, grid)            k_poly_chunk_eval / k_poly_pairs_eval, one per level
      ("sq", kernel, value)                                       the fr9_pow2k exponent of a level, per kernel that takes one
      ("scan", lanes, values per lane, idle lanes, short last lane)
      ("expand", group length, partial last group)                forms with a quotient
      ("quot", strided / lds / mont, grid, l0, n mod 2^l0)        n mod 2^l0: the fill of the last chunk; 1: it holds the zero slot alone"""
    l0, scan_max, scan_nt, lds = production_plan(n) if plan == PRODUCTION else plan
    lv = levels(n, l0, scan_max)
    K, cnt, sq = lv["K"], lv["n"], lv["sq"]
    grid = _GRID[form]
    out = {("level", form in (0, 2, 3), l0, n % (1 << l0) != 0, grid)}
    for k in range(1, K):
        out.add(("level", False, LUP, cnt[k] % (1 << LUP) != 0, grid))
        out.add(("sq", "level", sq[k]))
    top = cnt[K]
    m = (top + scan_nt - 1) // scan_nt
    out.add(("sq", "scan", sq[K]))
    out.add(("scan", scan_nt, m, (top + m - 1) // m < scan_nt, top % m != 0))
    if form in (0, 4, 5):
        for k in range(1, K):
            out.add(("expand", LUP, cnt[k] % (1 << LUP) != 0))
            out.add(("sq", "expand", sq[k]))
        kind = "mont" if form == 5 else "lds" if lds else "strided"
        out.add(("quot", kind, grid, l0, n % (1 << l0)))
    return out


@lru_cache(maxsize=None)
def production_lengths():
    """all powers of two up to 2^MAX_LOG, each - 1 and + 1 (and - 5, - 9), each + 1024 * odd, and a seeded sample between them"""
    rnd = random.Random(0x51A7)
    out = set()
    for k in range(0, MAX_LOG + 1):
        out.update({(1 << k) - 1, 1 << k, (1 << k) + 1})
        out.update({(1 << k) - 5, (1 << k) - 9})      # (a top level one and two values short of full lanes)
        out.update((1 << k) + 1024 * odd for odd in (1, 3, 5, 7, 33))
        if k:
            out.update(rnd.randrange(1 << (k - 1), 1 << k) for _ in range(24))
    return sorted(v for v in out if 1 <= v <= 1 << MAX_LOG)


@lru_cache(maxsize=None)
def production_signatures():
    out = set()
    for n in production_lengths():
        for form in FORMS:
            out |= signatures(n, PRODUCTION, form)
    return frozenset(out)


@lru_cache(maxsize=None)
def candidate_lengths():
    """where covering plans are looked for, ascending: every length up to 320; around every power of two up to the cap; four
    times (and four times, less one) the top-level counts at which a scan changes its lanes, its values per lane or its fill;
    whole LDS blocks"""
    out = set(range(1, 321))
    for k in range(8, 18):
        out.update((1 << k) + d for d in (-2, -1, 0, 1, 2, 15, 16, 17))
    for t in (*range(255, 261), *range(510, 517), *range(765, 773), *range(1019, 1028), *range(2046, 2050)):
        out.update({4 * t, 4 * t - 1})
    out.update({1024, 2048, 3072})
    return sorted(v for v in out if 1 <= v <= CAP)


@lru_cache(maxsize=None)
def covering_plans():
    """[(n, plan, forms)]: for every production signature the first (candidate length, levels, lanes, lds, form) that holds it;
    `forms` the forms a plan is listed for.  Raises nothing when a signature stays unheld: test_poly_plans_cpu.py compares."""
    want = production_signatures()
    held, found = set(), {}
    for n in candidate_lengths():
        for l0 in (2, 3, 4):
            full = levels(n, l0, 1)
            for K in range(1, full["K"] + 1):
                scan_max = full["n"][K]          # the least that stops the ladder at level K
                if K > 1 and full["n"][K - 1] <= scan_max:
                    continue
                for scan_nt in (256, 1024):
                    for lds in (0, 1):
                        plan = (l0, scan_max, scan_nt, lds)
                        if plan_invalid(n, plan):
                            continue
                        for form in FORMS:
                            new = (signatures(n, plan, form) & want) - held
                            if new:
                                held |= new
                                found.setdefault((n, plan), set()).add(form)
        if held == want:
            break
    return tuple((n, plan, tuple(sorted(forms))) for (n, plan), forms in sorted(found.items()))


def covered_signatures():
    out = set()
    for n, plan, forms in covering_plans():
        for form in forms:
            out |= signatures(n, plan, form)
    return out


def extra_plans():
    """beside the covering list: level 0 of every chunk length over more than three workgroups with a partial last chunk (a
    signature does not say how many workgroups a kernel ran), two and three levels above it"""
    return tuple((768 * (1 << l0) + 5 + 16 * l0, (l0, scan_max, 256, 0)) for l0 in (2, 3, 4) for scan_max in (64, 3))
