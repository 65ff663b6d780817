"""The quotient of kzg_rows_commit_quotient_ext from its definition, by a DIFFERENT route than the device, built on
tests/quotient_ref.py: products on the PLAIN domain (no coset anywhere), a rotated factor f(w^rot X) as the coefficient
list shift_arg(f, w^rot) (no index arithmetic), LK1 and LK2 written out as the header states them (every product of
denominators formed explicitly, no running fraction), and exact synthetic division by X^T - 1 with the remainder returned
-- the reference of tests/test_quotient_ext_cpu.py (which pins it against schoolbook multiplication) and
tests/test_gpu_quotient_ext.py (which compares the GPU with it) -- and builders of satisfied instances."""
import random

from tests import grand_product_ref as gp
from tests import lookup_ref as lr
from tests import quotient_ref as qr

R = gp.R


def factor(f):
    """(row, rot) of a gate factor given as a row index or a (row, rot) pair"""
    return (f[0], f[1]) if isinstance(f, (tuple, list)) else (f, 0)


def rotated(coeffs, rot):
    """coefficients of f(w^rot X), w the T-th root of unity of the library's domain"""
    T = len(coeffs)
    return qr.shift_arg(coeffs, pow(gp.omega(T), rot % T, R))


def numerator(rows, terms, perm, lookup, ext_log):
    """coefficients of num = Gate + alpha P1 + alpha^2 P2 + alpha^3 LK1 + alpha^4 LK2 over the coefficient rows `rows`.
    terms: [(c_u, [row or (row, rot)])]; perm as in quotient_ref.numerator; lookup: None or dict(inputs, table, mult, sum,
    width, theta, beta, alpha) of integers and row indices."""
    T = len(rows[0])
    E = 1 << ext_log
    n = 1
    while n < (E + 1) * T:
        n *= 2
    D = qr.Domain(n)
    ev = {}

    def row_ev(j, rot=0):
        key = (j, rot % T)
        if key not in ev:
            ev[key] = D.ev(rotated(rows[j], rot))
        return ev[key]

    acc = [0] * n
    for c, fs in terms:
        assert len(fs) <= E + 1
        p = [c % R] * n
        for f in fs:
            p = [x * y % R for x, y in zip(p, row_ev(*factor(f)))]
        acc = [(x + y) % R for x, y in zip(acc, p)]
    if lookup:
        w, theta, beta, alpha = lookup["width"], lookup["theta"], lookup["beta"], lookup["alpha"]
        ins, tab = lookup["inputs"], lookup["table"]
        L = len(ins) // w
        assert L * w == len(ins) and len(tab) == w and 1 <= L <= E - 1
        groups = [tab] + [ins[l * w:(l + 1) * w] for l in range(L)]   # D_0 .. D_L
        dens = []
        for g in groups:
            d = [beta] * n
            for c, j in enumerate(g):
                tc = pow(theta, c, R)
                d = [(x + tc * y) % R for x, y in zip(d, row_ev(j))]
            dens.append(d)
        m, S, Sw = row_ev(lookup["mult"]), row_ev(lookup["sum"]), row_ev(lookup["sum"], 1)
        l0 = D.ev([pow(T, -1, R)] * T)
        a3, a4 = pow(alpha, 3, R), pow(alpha, 4, R)

        def prod_except(t, skip):
            p = 1
            for l, d in enumerate(dens):
                if l not in skip:
                    p = p * d[t] % R
            return p

        for t in range(n):
            bracket = (sum(prod_except(t, {l}) for l in range(1, L + 1)) - m[t] * prod_except(t, {0})) % R
            lk1 = ((Sw[t] - S[t]) * prod_except(t, set()) - bracket) % R
            acc[t] = (acc[t] + a3 * lk1 + a4 * S[t] % R * l0[t]) % R
    num = D.back(acc)
    if perm:
        num = qr.add(num, qr.numerator(rows, [], perm, ext_log))
    return num


def quotient(rows, terms, perm, lookup, ext_log):
    """(t's coefficients, trimmed; the remainder's T coefficients)"""
    q, rem = qr.divide_by_vanishing(numerator(rows, terms, perm, lookup, ext_log), len(rows[0]))
    return qr.trim(q), rem


def num_at(val, terms, perm, lookup, x, T):
    """num(x) from row values alone: val(j, rot) = f_j(w^rot x) as an integer"""
    acc = 0
    for c, fs in terms:
        p = c
        for f in fs:
            p = p * val(*factor(f)) % R
        acc += p
    l0 = (pow(x, T, R) - 1) * pow(T * (x - 1) % R, -1, R) % R
    if perm:
        beta, gamma, alpha = perm["beta"], perm["gamma"], perm["alpha"]
        A, B = val(perm["z"], 0), val(perm["z"], 1)
        for a, s, sh in zip(perm["wires"], perm["sigmas"], perm["shifts"]):
            A = A * (val(a, 0) + beta * sh % R * x + gamma) % R
            B = B * (val(a, 0) + beta * val(s, 0) + gamma) % R
        acc += alpha * (A - B) + alpha * alpha % R * (val(perm["z"], 0) - 1) % R * l0
    if lookup:
        w, theta, beta, alpha = lookup["width"], lookup["theta"], lookup["beta"], lookup["alpha"]
        ins = lookup["inputs"]
        L = len(ins) // w
        dens = [(beta + sum(pow(theta, c, R) * val(j, 0) for c, j in enumerate(g))) % R
                for g in [lookup["table"]] + [ins[l * w:(l + 1) * w] for l in range(L)]]
        prod = lambda skip: _prod(d for l, d in enumerate(dens) if l not in skip)   # noqa: E731
        bracket = sum(prod({l}) for l in range(1, L + 1)) - val(lookup["mult"], 0) * prod({0})
        S = val(lookup["sum"], 0)
        acc += pow(alpha, 3, R) * ((val(lookup["sum"], 1) - S) * prod(set()) - bracket) + pow(alpha, 4, R) * S % R * l0
    return acc % R


def _prod(it):
    p = 1
    for v in it:
        p = p * v % R
    return p


# ---------------------------------------------------------------------------------------------------- instances
A_, B_, C_, Q_ = range(4)
# a(wX) b(X) + a(w^-1 X) + c(w^2 X) c(X) + q(X) = 0: the next, the previous and the second-next row, wrap included


def next_row_terms(T=None, wrapped=False):
    """the next-row gate's terms; wrapped: the rotations given as T + 1, T - 1 and T + 2 instead of 1, -1 and 2"""
    up, dn, up2 = (T + 1, T - 1, T + 2) if wrapped else (1, -1, 2)
    return [(1, [(A_, up), B_]), (1, [(A_, dn)]), (1, [(C_, up2), (C_, 0)]), (1, [Q_])]


def next_row_instance(T, seed):
    """a SATISFIED instance of the gate above as 4 evaluation rows a b c q, q solved per row"""
    rnd = random.Random(seed * 104729 + T)
    a, b, c = ([rnd.randrange(R) for _ in range(T)] for _ in range(3))
    q = [-(a[(t + 1) % T] * b[t] + a[(t - 1) % T] + c[(t + 2) % T] * c[t]) % R for t in range(T)]
    return [a, b, c, q]


def lookup_rows(L, w, T, seed, theta=None, beta=None, alpha=None, first_row=0):
    """a lookup instance as evaluation rows inputs (L w) | table (w) | m | S, with the lookup part that names them from
    row index first_row on"""
    rnd = random.Random(seed * 15485863 + T)
    ins, tab, mult = lr.lookup_instance(L, w, T, seed)
    theta = rnd.randrange(R) if theta is None else theta
    beta = rnd.randrange(R) if beta is None else beta
    alpha = rnd.randrange(R) if alpha is None else alpha
    S, closing = lr.lookup_sum(ins, tab, mult, L, w, theta, beta)
    assert closing == 0
    o = first_row
    lookup = {"inputs": list(range(o, o + L * w)), "table": list(range(o + L * w, o + L * w + w)), "mult": o + L * w + w,
              "sum": o + L * w + w + 1, "width": w, "theta": theta, "beta": beta, "alpha": alpha}
    return ins + tab + [mult, S], lookup


def shuffled_table(col, rnd):
    """(a table row holding col's values in another order, the multiplicities: every count on a value's first copy)"""
    table = list(col)
    rnd.shuffle(table)
    first = {}
    for t, v in enumerate(table):
        first.setdefault(v, t)
    mult = [0] * len(col)
    for v in col:
        mult[first[v]] += 1
    return table, mult


def round_instance(T, seed):
    """the 16-row circuit of scripts/bench_quotient_ext.py: the standard 13 rows, then a table row (a shuffle of wire c's
    values), m and S; one lookup of width 1 whose input is wire c.  Gate, permutation and lookup share alpha."""
    rows, terms, perm = qr.standard_instance(T, seed)
    rnd = random.Random(seed * 32452843 + T)
    c = rows[qr.C_]
    table, mult = shuffled_table(c, rnd)
    theta, beta = rnd.randrange(R), rnd.randrange(R)
    S, closing = lr.lookup_sum([c], [table], mult, 1, 1, theta, beta)
    assert closing == 0
    lookup = {"inputs": [qr.C_], "table": [13], "mult": 14, "sum": 15, "width": 1, "theta": theta, "beta": beta,
              "alpha": perm["alpha"]}
    return rows + [table, mult, S], terms, perm, lookup
