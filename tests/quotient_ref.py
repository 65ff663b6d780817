"""The PLONK quotient of kzg_rows_commit_quotient from its definition, by a DIFFERENT route than the device: the rows'
coefficients (the oracle's inverse NTT), polynomial products through the C oracle's NTT on the PLAIN domain of length
>= (E + 1) T (no coset anywhere), and exact synthetic division by X^T - 1, which also returns the remainder -- the reference of
tests/test_quotient_cpu.py (which pins it against schoolbook multiplication) and tests/test_gpu_quotient.py (which compares
the GPU with it) -- and a builder of satisfied standard-PLONK instances."""
import random

from oracle import cpu
from tests import grand_product_ref as gp

R = gp.R
be, ints, row_bytes = gp.be, gp.ints, gp.row_bytes


def coeffs_of(evals):
    """coefficients of the row given by its T evaluations on the library's domain"""
    return ints(cpu.fr_ntt(row_bytes(evals), True))


def evals_of(coeffs):
    return ints(cpu.fr_ntt(row_bytes(coeffs), False))


def pad(c, n):
    assert len(c) <= n or not any(c[n:])
    return (list(c) + [0] * n)[:n]


def trim(c):
    c = list(c)
    while c and c[-1] == 0:
        c.pop()
    return c


def degree(c):
    return len(trim(c)) - 1


def poly_eval(c, x):
    acc = 0
    for v in reversed(c):
        acc = (acc * x + v) % R
    return acc


def add(a, b):
    n = max(len(a), len(b))
    return [(x + y) % R for x, y in zip(pad(a, n), pad(b, n))]


def sub(a, b):
    n = max(len(a), len(b))
    return [(x - y) % R for x, y in zip(pad(a, n), pad(b, n))]


def scale(a, s):
    return [v * s % R for v in a]


def mul_schoolbook(a, b):
    out = [0] * (len(a) + len(b) - 1) if a and b else []
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % R
    return out


class Domain:
    """pointwise products on the plain domain of n points (n a power of two that bounds every degree formed)"""

    def __init__(self, n):
        assert n & (n - 1) == 0
        self.n = n

    def ev(self, coeffs):
        return ints(cpu.fr_ntt(row_bytes(pad(coeffs, self.n)), False))

    def back(self, evals):
        return ints(cpu.fr_ntt(row_bytes(evals), True))


def shift_arg(c, s):
    """coefficients of f(sX)"""
    out, p = [], 1
    for v in c:
        out.append(v * p % R)
        p = p * s % R
    return out


def numerator(rows, terms, perm, ext_log):
    """coefficients of num = Gate + alpha P1 + alpha^2 P2 over the coefficient rows `rows` (lists of T integers).
    terms: [(c_u, [row indices])]; perm: None or dict(wires, sigmas, z, shifts, beta, gamma, alpha) of integers."""
    T = len(rows[0])
    E = 1 << ext_log
    n = 1
    while n < (E + 1) * T:
        n *= 2
    D = Domain(n)
    ev = {}

    def row_ev(j):
        if j not in ev:
            ev[j] = D.ev(rows[j])
        return ev[j]

    acc = [0] * n
    for c, idx in terms:
        assert len(idx) <= E + 1
        p = [c % R] * n
        for j in idx:
            p = [x * y % R for x, y in zip(p, row_ev(j))]
        acc = [(x + y) % R for x, y in zip(acc, p)]
    if perm:
        k = len(perm["wires"])
        assert 1 <= k <= E
        beta, gamma, alpha = perm["beta"], perm["gamma"], perm["alpha"]
        w = gp.omega(T)
        zc = rows[perm["z"]]
        z, zw = D.ev(zc), D.ev(shift_arg(zc, w))
        xs = D.ev([0, 1])
        A, B = z[:], zw[:]
        for a_j, s_j, sh in zip(perm["wires"], perm["sigmas"], perm["shifts"]):
            a, sg = row_ev(a_j), row_ev(s_j)
            A = [p * (av + beta * sh % R * x + gamma) % R for p, av, x in zip(A, a, xs)]
            B = [p * (av + beta * s + gamma) % R for p, av, s in zip(B, a, sg)]
        l0 = D.ev([pow(T, -1, R)] * T)   # L_0 = (X^T - 1) / (T (X - 1)) = (1 / T) sum_{i < T} X^i
        for t in range(n):
            acc[t] = (acc[t] + alpha * (A[t] - B[t]) + alpha * alpha % R * (z[t] - 1) % R * l0[t]) % R
    return D.back(acc)


def divide_by_vanishing(num, T):
    """(quotient, remainder) of num by X^T - 1, exact synthetic division"""
    c = list(num)
    q = [0] * max(len(c) - T, 0)
    for i in range(len(c) - 1, T - 1, -1):
        q[i - T] = c[i]
        c[i - T] = (c[i - T] + c[i]) % R
        c[i] = 0
    return q, c[:T]


def quotient(rows, terms, perm, ext_log):
    """(t's coefficients, trimmed; the remainder's T coefficients)"""
    T = len(rows[0])
    q, rem = divide_by_vanishing(numerator(rows, terms, perm, ext_log), T)
    return trim(q), rem


def pieces(t, T, P):
    """t split into P rows of T coefficients; AssertionError when it does not fit"""
    assert len(trim(t)) <= P * T
    c = pad(trim(t), P * T)
    return [c[p * T:(p + 1) * T] for p in range(P)]


# row order of the standard circuit: a b c | qL qR qO qM qC | sigma1 sigma2 sigma3 | z | PI
A_, B_, C_, QL, QR, QO, QM, QC, S1, S2, S3, Z_, PI_ = range(13)
STD_TERMS = [(1, [QL, A_]), (1, [QR, B_]), (1, [QO, C_]), (1, [QM, A_, B_]), (1, [QC]), (1, [PI_])]


def standard_instance(T, seed, beta=None, gamma=None, alpha=None):
    """a SATISFIED standard PLONK instance as 13 evaluation rows (lists of T integers) in the order above, with the terms
    and the permutation part that describe it: wires and sigmas of a real permutation, z its grand product, random
    selectors and public-input row with qC solved per row so that the gate holds"""
    rnd = random.Random(seed * 7919 + T)
    wires, sigmas, shifts = gp.permutation_instance(3, T, seed)
    beta = rnd.randrange(R) if beta is None else beta
    gamma = rnd.randrange(R) if gamma is None else gamma
    alpha = rnd.randrange(R) if alpha is None else alpha
    while True:
        try:
            z, closing = gp.grand_product(wires, sigmas, shifts, beta, gamma)
            break
        except ZeroDivisionError:   # (2^-255 per row: only for chosen challenges)
            gamma = (gamma + 1) % R
    assert closing == 1
    a, b, c = wires
    ql, qr, qo, qm = ([rnd.randrange(R) for _ in range(T)] for _ in range(4))
    pi = [rnd.randrange(R) for _ in range(T)]
    qc = [-(ql[t] * a[t] + qr[t] * b[t] + qo[t] * c[t] + qm[t] * a[t] % R * b[t] + pi[t]) % R for t in range(T)]
    rows = [a, b, c, ql, qr, qo, qm, qc, sigmas[0], sigmas[1], sigmas[2], z, pi]
    perm = {"wires": [A_, B_, C_], "sigmas": [S1, S2, S3], "z": Z_, "shifts": shifts, "beta": beta, "gamma": gamma,
            "alpha": alpha}
    return rows, list(STD_TERMS), perm
