"""Reference, input families and pass plans of the NTT tests (tests/test_ntt_plans_cpu.py, tests/test_gpu_ntt_plans.py).  Plain
Python integers; nothing here needs a device.

The transform is the definition X_k = sum_j a_j w^(jk) with w = 7^((r - 1) / n) (inverse: w^-1 and a factor 1 / n), summed term
by term up to n = 2^8; above that the C oracle's, which the CPU module checks against the definition up to 2^8.  Every input
family carries its closed-form output where one exists, so that most expectations do not come from any transform code at all.

A pass plan is (kernel, ((S, logC), ...)): kernel 0 the register-blocked form (k_fr_ntt_pass4), 1 the radix-2 form
(k_fr_ntt_pass); pass p runs S stages on tiles of 2^S rows x 2^logC columns.  plan_invalid restates the kernels' preconditions
(csrc/fr_ntt.hip, next to run_fr_ntt_plan)."""
import random
from functools import lru_cache

from oracle.bls12_381 import R

DEF_MAX_LOG = 8                      # the definition is summed term by term up to here
MAX_S = {0: 9, 1: 8}                 # stages per pass: register-blocked, radix-2
TILE_LOG = {0: 11, 1: 10}            # log2 of the largest tile
FORMS = {0: "blocked", 1: "radix2"}
# the `edge` pool of tests/fuzz_gpu.py
EDGE_POOL = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, (1 << 254), (1 << 255) % R] + \
            [(1 << k) - 1 for k in (8, 16, 20, 28, 32, 64, 128, 200)] + [(1 << k) for k in (7, 15, 19, 27, 31, 63, 127)]


def root(log_n, inverse=False):
    w = pow(7, (R - 1) >> log_n, R)
    return pow(w, -1, R) if inverse else w


def powers(w, n):
    out, cur = [], 1
    for _ in range(n):
        out.append(cur)
        cur = cur * w % R
    return out


def ntt_by_definition(a, inverse=False):
    """X_k = sum_j a_j w^(jk), every term; the inverse with w^-1 and 1 / n.  n <= 2^8."""
    n = len(a)
    log_n = n.bit_length() - 1
    assert n == 1 << log_n and log_n <= DEF_MAX_LOG
    pw = powers(root(log_n, inverse), n)
    scale = pow(n, -1, R) if inverse else 1
    return [sum(a[j] * pw[j * k % n] for j in range(n)) * scale % R for k in range(n)]


def ntt(a, inverse=False):
    """the reference transform: the definition up to 2^8, the C oracle's above"""
    if len(a) <= 1 << DEF_MAX_LOG:
        return ntt_by_definition(a, inverse)
    from oracle import cpu as oc

    raw = oc.fr_ntt(to_bytes(a), inverse)
    return [int.from_bytes(raw[i:i + 32], "big") for i in range(0, len(raw), 32)]


def to_bytes(a):
    return b"".join(v.to_bytes(32, "big") for v in a)


# ---------------------------------------------------------------------------------------------------------------- families
class Family:
    """One seeded input vector; closed(inverse) is its transform in closed form, or None where there is none."""

    def __init__(self, name, a, closed=None):
        self.name, self.a, self._closed = name, a, closed

    def closed(self, inverse=False):
        return self._closed(inverse) if self._closed else None

    @lru_cache(maxsize=None)
    def expected(self, inverse=False):
        c = self.closed(inverse)
        return tuple(c if c is not None else ntt(self.a, inverse))


def _sparse(n, k, v):
    out = [0] * n
    out[k] = v % R
    return out


@lru_cache(maxsize=None)
def families(log_n):
    """name -> Family for 2^log_n elements (log_n >= 0), in a fixed order"""
    n = 1 << log_n
    inv_n = pow(n, -1, R)
    rnd = random.Random(0x4E7700 + log_n)
    fams = [Family("zero", [0] * n, lambda inverse: [0] * n)]
    for tag, c in (("1", 1), ("r-1", R - 1), ("(r-1)/2", (R - 1) // 2)):
        # sum_j c w^(jk) = n c at k = 0 and 0 elsewhere; the inverse divides by n
        fams.append(Family(f"constant {tag}", [c] * n, lambda inverse, c=c: _sparse(n, 0, c if inverse else n * c)))
    for j in sorted({0, 1 % n, n // 2, n - 1}):
        for tag, v in (("1", 1), ("r-1", R - 1)):
            def closed(inverse, j=j, v=v):      # v w^(jk), the inverse v w^(-jk) / n
                s = inv_n if inverse else 1
                return [v * s % R * p % R for p in powers(pow(root(log_n, inverse), j, R), n)] if log_n else [v]
            fams.append(Family(f"delta {tag} at {j}", _sparse(n, j, v), closed))
    for j in sorted({1 % n, n - 1}):
        # a_i = w^(-ji): the forward transform is n at k = j; the inverse sums w^(-i (j + k)) / n: 1 at k = -j mod n
        a = powers(pow(root(log_n, True), j, R), n) if log_n else [1]
        fams.append(Family(f"geometric {j}", a, lambda inverse, j=j: _sparse(n, (n - j) % n if inverse else j, 1 if inverse else n)))
    fams.append(Family("alternating", [(R - 1) if i % 2 == 0 else 0 for i in range(n)]))
    fams.append(Family("edge pool", [EDGE_POOL[(i + log_n) % len(EDGE_POOL)] for i in range(n)]))
    fams.append(Family("uniform", [rnd.randrange(R) for _ in range(n)]))
    return {f.name: f for f in fams}


# ------------------------------------------------------------------------------------------------------------------- plans
def plan_invalid(log_n, kernel, passes):
    """None for a plan the kernels admit, otherwise what is wrong with it (csrc/fr_ntt.hip, ntt_plan_invalid)"""
    if kernel not in (0, 1) or not passes:
        return "no kernel form or no pass"
    s0 = 0
    for p, (S, logC) in enumerate(passes):
        if not 1 <= S <= MAX_S[kernel]:
            return f"pass {p}: S = {S}"
        if logC < 0 or S + logC > TILE_LOG[kernel]:
            return f"pass {p}: tile 2^{S + logC}"
        if logC > (log_n - S if p == 0 else s0):
            return f"pass {p}: logC = {logC} columns do not exist"
        s0 += S
    return None if s0 == log_n else f"stages sum to {s0}"


def position(p, passes):
    return "only" if passes == 1 else "first" if p == 0 else "last" if p == passes - 1 else "middle"


def plan_tuples(kernel, passes):
    """the per-workgroup geometries of a plan: (kernel, position, S, logC) per pass"""
    return [(kernel, position(p, len(passes)), S, logC) for p, (S, logC) in enumerate(passes)]


def plan_name(log_n, kernel, passes):
    return f"2^{log_n} {FORMS[kernel]} " + "+".join(f"{S}x{logC}" for S, logC in passes)


@lru_cache(maxsize=None)
def valid_plans(log_n, kernel, max_passes=3):
    """every plan of at most max_passes passes that satisfies the preconditions, as tuples of (S, logC)"""
    out = []

    def extend(prefix, s0):
        if s0 == log_n:
            out.append(tuple(prefix))
            return
        if len(prefix) == max_passes:
            return
        for S in range(1, min(MAX_S[kernel], log_n - s0) + 1):
            if len(prefix) == max_passes - 1 and s0 + S != log_n:
                continue
            for logC in range(0, min(TILE_LOG[kernel] - S, s0 if prefix else log_n - S) + 1):
                extend(prefix + [(S, logC)], s0 + S)

    extend([], 0)
    assert all(plan_invalid(log_n, kernel, pl) is None for pl in out)
    return tuple(out)


def _halves(kernel, total):
    """`total` stages as one pass, or as two where one pass cannot hold them"""
    return [total] if total <= MAX_S[kernel] else [total - total // 2, total // 2]


def smallest_plan_with(tup):
    """(log_n, kernel, passes): a valid plan of the smallest log_n that holds the geometry `tup` at its position.  A first pass
    needs logC <= log_n - S and company, a later pass s0 >= logC stages in front of it, a middle pass one more behind it; the
    passes that only complete the plan take as many columns as exist and fit, four at the most."""
    kernel, pos, S, logC = tup
    if pos == "only":
        stages, at = [S], 0
    elif pos == "first":
        stages, at = [S] + _halves(kernel, max(logC, 1)), 0
    else:
        head = _halves(kernel, max(logC, 1))
        stages, at = head + [S] + ([1] if pos == "middle" else []), len(head)
    log_n, passes, s0 = sum(stages), [], 0
    for p, fs in enumerate(stages):
        avail = log_n - fs if p == 0 else s0
        passes.append((fs, logC) if p == at else (fs, min(TILE_LOG[kernel] - fs, avail, 2)))
        s0 += fs
    why = plan_invalid(log_n, kernel, passes)
    if why or position(at, len(passes)) != pos:
        raise ValueError(f"{tup}: {plan_name(log_n, kernel, passes)} does not hold it: {why}")
    return log_n, kernel, tuple(passes)


def library_plan_of(log_n, kernel, tile_log):
    from zkp_subnet_amd.engine import ntt_plan_of

    return ntt_plan_of(log_n, kernel, tile_log)


def production_tuples(plan_of=library_plan_of):
    """every geometry the library's own plans hold: log_n 1 .. 28, both forms, tile_log 8 .. 11"""
    tuples = set()
    for log_n in range(1, 29):
        for kernel in (0, 1):
            for tile_log in (8, 9, 10, 11):
                form, passes = plan_of(log_n, kernel, tile_log)
                assert form == kernel
                tuples.update(plan_tuples(kernel, passes))
    return tuples


_COVERING = {}


def covering_plans(plan_of=library_plan_of):
    """for every geometry of production_tuples, one valid plan of the smallest log_n that holds it (duplicates dropped);
    a list of (log_n, kernel, passes), sorted"""
    if plan_of not in _COVERING:
        _COVERING[plan_of] = sorted({smallest_plan_with(t) for t in production_tuples(plan_of)})
    return _COVERING[plan_of]
