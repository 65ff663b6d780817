"""Pure-Python reference of the SHPLONK (BDFG20) opening over the C oracle: h by schoolbook division of Python-int
polynomials, the round-B scalars, r_j(u) and v, and a prover built only from oc.commit / oc.open_ of host-combined polynomials.
Nothing here touches the library under test.

Conventions (include/kzg_mi355x.h, kzg_rows_commit_shplonk): rows f_j as lists of T coefficients; points a_p pairwise
distinct; opened[p] the rows opened at a_p; S_j = {p : j in opened[p]}; c_j one scalar per row, c_j = 0 leaves the row out."""
from oracle import bls12_381 as o
from oracle import cpu as oc
from tests.gpu_common import be, ints, row_bytes  # noqa: F401  (re-exported for the tests)

R = o.R


def coeffs_of(row_be32, ef):
    """the T coefficients (ints) of a row given in either form"""
    return ints(oc.fr_ntt(row_be32, True) if ef else row_be32)


def point_sets(k, opened):
    return [[p for p in range(len(opened)) if j in opened[p]] for j in range(k)]


def divide_linear(f, a):
    """(quotient, remainder) of f by (X - a): schoolbook synthetic division from the top coefficient down"""
    q, carry = [0] * (len(f) - 1), 0
    for t in range(len(f) - 1, 0, -1):
        carry = (f[t] + carry * a) % R
        q[t - 1] = carry
    return q, (f[0] + carry * a) % R


def divide_by_points(f, pts):
    """quot(f, prod (X - a)), the remainder discarded; padded with zeros to len(f) coefficients"""
    g = list(f)
    for a in pts:
        g, _ = divide_linear(g, a)
    return g + [0] * (len(f) - len(g))


def poly_eval(f, x):
    acc = 0
    for c in reversed(f):
        acc = (acc * x + c) % R
    return acc


def interpolant_at(xs, ys, u):
    """r(u) for the interpolant r of the points (xs[t], ys[t]): the Lagrange formula"""
    acc = 0
    for t, (x, y) in enumerate(zip(xs, ys)):
        num = den = 1
        for s, x2 in enumerate(xs):
            if s != t:
                num = num * (u - x2) % R
                den = den * (x - x2) % R
        acc = (acc + y * num * pow(den, -1, R)) % R
    return acc


def h_poly(F, points, opened, c):
    """h = sum_{j : c_j != 0} c_j (f_j - r_j) / Z_{S_j}, row by row (the first form of the header), T coefficients"""
    T = len(F[0])
    S = point_sets(len(F), opened)
    h = [0] * T
    for j, f in enumerate(F):
        if c[j] % R == 0:
            continue
        q = divide_by_points(f, [points[p] for p in S[j]])
        h = [(a + c[j] * b) % R for a, b in zip(h, q)]
    return h


def finish_coeffs(points, opened, c, u):
    """lambda_j = c_j Z_{P \\ S_j}(u) for j < k, lambda_k = -Z_P(u)"""
    S = point_sets(len(c), opened)
    lam = []
    for j, cj in enumerate(c):
        z = 1
        for p, a in enumerate(points):
            if p not in S[j]:
                z = z * (u - a) % R
        lam.append(cj * z % R)
    zp = 1
    for a in points:
        zp = zp * (u - a) % R
    return lam + [(-zp) % R]


def evaluations(F, points, opened):
    """y_{j,p} in eval_rows' shape: [[f_j(a_p) for j in opened[p]] for p]"""
    return [[poly_eval(F[j], a) for j in js] for a, js in zip(points, opened)]


def value_v(points, opened, c, evals, u):
    """v = sum_j c_j Z_{P \\ S_j}(u) r_j(u) from the evaluations alone: what the verifier computes"""
    k = len(c)
    S = point_sets(k, opened)
    lam = finish_coeffs(points, opened, c, u)
    v = 0
    for j in range(k):
        if c[j] % R == 0:
            continue
        ys = [evals[p][opened[p].index(j)] for p in S[j]]
        v = (v + lam[j] * interpolant_at([points[p] for p in S[j]], ys, u)) % R
    return v


def combine(F, lam):
    out = [0] * len(F[0])
    for f, l in zip(F, lam):
        if l:
            out = [(a + l * b) % R for a, b in zip(out, f)]
    return out


def prove(srs, F, points, opened, c, u):
    """(commitments, evals, W, v, pi, h) with the C oracle's commit / open_ on host-combined coefficient rows"""
    comms = [oc.commit(srs, row_bytes(f), False) for f in F]
    h = h_poly(F, points, opened, c)
    W = oc.commit(srs, row_bytes(h), False)
    lam = finish_coeffs(points, opened, c, u)
    L = combine(F + [h], lam)
    v, pi = oc.open_(srs, row_bytes(L), be(u), False)
    return comms, evaluations(F, points, opened), W, v, pi, h


# the four shapes of the tests: name -> (k, opened).  one: one point set {zeta}; plonk: {zeta}, {zeta, zeta w}; three: three
# point sets that share a point; eight: m = 8 with row 0 opened at all eight
SHAPES = {
    "one": (3, [[0, 1, 2]]),
    "plonk": (5, [[0, 1, 2, 3, 4], [3]]),
    "three": (6, [[0, 1, 2, 3, 4, 5], [2, 3], [4, 5], [4, 5]]),
    "eight": (4, [[0, 1, 2, 3], [0, 1], [0, 1], [0], [0], [0], [0], [0, 3]]),
}
