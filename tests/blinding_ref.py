"""The blinding-rows builders (kzg_rows_commit_*_zk) from their definitions, in Python integers, on top of the plain
references (tests/grand_product_ref.py, lookup_ref.py, multiplicities_ref.py, quotient_ext_ref.py: imported, not edited) --
the reference of tests/test_blinding_cpu.py (which pins it) and tests/test_gpu_blinding.py (which compares the GPU with it).
With u = usable < T: rows [0, u) carry the circuit, row u closes the running values, rows u + 1 .. T - 1 hold random values.
The numerator with the active column A is put together from the plain references' numerators by their dependence on alpha:
alpha P1 + alpha^2 P2 at alpha = 1 and alpha = -1 gives P1 and P2 apart (likewise LK1 and LK2 from alpha^3, alpha^4)."""
import random

from tests import grand_product_ref as gp
from tests import lookup_ref as lr
from tests import multiplicities_ref as mr
from tests import quotient_ext_ref as qx
from tests import quotient_ref as qr

R = gp.R
be, row_bytes = gp.be, gp.row_bytes
INV2 = pow(2, -1, R)


# ---------------------------------------------------------------------------------------------------- the three builders
def grand_product_zk(wires, sigmas, shifts, beta, gamma, usable, tail):
    """(z's T evaluations, closing): z_0 = 1, z_{t+1} = z_t N_t / D_t for t < usable, z_usable = closing, the tail behind.
    Rows >= usable of the wires and sigmas are not read; ZeroDivisionError when some D_t, t < usable, is 0."""
    T = len(wires[0])
    assert 1 <= usable < T and len(tail) == T - usable - 1
    N, D = gp.factors(wires, sigmas, shifts, beta, gamma)
    Dinv = gp.batch_inverse(D[:usable])
    z, acc = [], 1
    for t in range(usable):
        z.append(acc)
        acc = acc * N[t] % R * Dinv[t] % R
    return z + [acc] + [v % R for v in tail], acc


def lookup_sum_zk(inputs, table, mult, n_lookups, width, theta, beta, usable, tail):
    """(S's T evaluations, closing): S_0 = 0, S_{t+1} = S_t + term_t for t < usable, S_usable = closing, the tail behind.
    ZeroDivisionError when a denominator of a row < usable is 0."""
    T = len(mult)
    assert 1 <= usable < T and len(tail) == T - usable - 1
    cut = lambda rows: [r[:usable] for r in rows]   # noqa: E731
    term = lr.terms(cut(inputs), cut(table), mult[:usable], n_lookups, width, theta, beta)
    S, acc = [], 0
    for x in term:
        S.append(acc)
        acc = (acc + x) % R
    return S + [acc] + [v % R for v in tail], acc


def multiplicities_zk(inputs, table, n_lookups, width, usable, tail):
    """(m's T evaluations, missing): the join over table rows and input cells < usable only, m_usable = 0, the tail behind"""
    T = len(table[0])
    assert 1 <= usable < T and len(tail) == T - usable - 1
    m, missing = mr.multiplicities([r[:usable] for r in inputs], [r[:usable] for r in table], n_lookups, width)
    return m + [0] + [v % R for v in tail], missing


def active_row(T, usable):
    """A: 1 on the usable rows, 0 elsewhere"""
    return [1] * usable + [0] * (T - usable)


def last_row(T, usable):
    """L_u on the domain: 1 at row usable, 0 elsewhere"""
    return [int(t == usable) for t in range(T)]


# ---------------------------------------------------------------------------------------------------- the quotient
def _odd_even(f):
    """f(alpha) = alpha^o X + alpha^(o+1) Y with o odd -> (X, Y) from f(1) and f(-1)"""
    plus, minus = f(1), f(R - 1)
    return qr.scale(qr.sub(plus, minus), INV2), qr.scale(qr.add(plus, minus), INV2)


def _mul(a, b, n):
    D = qr.Domain(n)
    return D.back([x * y % R for x, y in zip(D.ev(a), D.ev(b))])


def numerator(rows, terms, perm, lookup, active, ext_log):
    """coefficients of num = Gate + alpha A P1 + alpha^2 P2 + alpha^3 A LK1 + alpha^4 LK2 over the coefficient rows `rows`;
    active: the row index of A, or None for the plain numerator of quotient_ext_ref"""
    if active is None:
        return qx.numerator(rows, terms, perm, lookup, ext_log)
    T, E = len(rows[0]), 1 << ext_log
    n = 1
    while n < (E + 1) * T:
        n *= 2
    num = qx.numerator(rows, terms, None, None, ext_log)
    if perm:
        assert len(perm["wires"]) <= E - 1            # A P1 has k + 2 factors
        alpha = perm["alpha"]
        P1, P2 = _odd_even(lambda a: qr.numerator(rows, [], dict(perm, alpha=a), ext_log))
        num = qr.add(num, qr.add(qr.scale(_mul(rows[active], P1, n), alpha), qr.scale(P2, alpha * alpha % R)))
    if lookup:
        assert len(lookup["inputs"]) // lookup["width"] <= E - 2   # A LK1 has L + 3 factors
        alpha = lookup["alpha"]
        LK1, LK2 = _odd_even(lambda a: qx.numerator(rows, [], None, dict(lookup, alpha=a), ext_log))
        num = qr.add(num, qr.add(qr.scale(_mul(rows[active], LK1, n), pow(alpha, 3, R)), qr.scale(LK2, pow(alpha, 4, R))))
    return num


def quotient(rows, terms, perm, lookup, active, ext_log):
    """(t's coefficients, trimmed; the remainder's T coefficients)"""
    q, rem = qr.divide_by_vanishing(numerator(rows, terms, perm, lookup, active, ext_log), len(rows[0]))
    return qr.trim(q), rem


def num_at(val, terms, perm, lookup, active, x, T):
    """num(x) with the A factors from row values alone: val(j, rot) = f_j(w^rot x) as an integer"""
    if active is None:
        return qx.num_at(val, terms, perm, lookup, x, T)
    acc, A = qx.num_at(val, terms, None, None, x, T), val(active, 0)
    if perm:
        f = lambda a: qx.num_at(val, [], dict(perm, alpha=a), None, x, T)   # noqa: E731
        P1, P2 = (f(1) - f(R - 1)) * INV2, (f(1) + f(R - 1)) * INV2
        acc += perm["alpha"] * A % R * P1 + pow(perm["alpha"], 2, R) * P2
    if lookup:
        f = lambda a: qx.num_at(val, [], None, dict(lookup, alpha=a), x, T)   # noqa: E731
        LK1, LK2 = (f(1) - f(R - 1)) * INV2, (f(1) + f(R - 1)) * INV2
        acc += pow(lookup["alpha"], 3, R) * A % R * LK1 + pow(lookup["alpha"], 4, R) * LK2
    return acc % R


# ---------------------------------------------------------------------------------------------------- an instance
# row order: a b c | qM qL qC | sigma1 sigma2 sigma3 | A L_u | table | m z S
A_, B_, C_, QM, QL, QC, S1, S2, S3, ACT, LU, TAB, M_, Z_, SUM = range(15)
WIRES, FIXED = (A_, B_, C_), (QM, QL, QC, S1, S2, S3, ACT, LU, TAB)
# the gate qM a b + qL (a + b) - A c + qC = 0: every selector (A among them) is 0 on the padding rows


class Instance:
    """a SATISFIED circuit on the first `usable` of T rows -- 3 wires under a permutation of the 3 * usable usable cells,
    one width-1 lookup of wire c in a fixed table column -- with RANDOM padding: the wires' rows >= usable, and the tails of
    m, z and S.  rows: the 15 evaluation rows in the order above; terms / perm / lookup / active: what the quotient takes
    (integers), the two L_u relations included as gate terms with alpha^5 and alpha^6."""

    def __init__(self, T, usable, seed):
        self.T, self.usable, self.seed = T, usable, seed
        rnd = random.Random(seed * 49979687 + 1000 * T + usable)
        u, dom = usable, gp.domain(T)
        self.shifts = [pow(7, j, R) for j in range(3)]
        cells = [(j, t) for j in range(3) for t in range(u)]
        image = cells[:]
        rnd.shuffle(image)
        pm = dict(zip(cells, image))
        wires = [[None] * u for _ in range(3)]
        for c in cells:
            if wires[c[0]][c[1]] is None:
                v, x = rnd.randrange(R), c
                while wires[x[0]][x[1]] is None:
                    wires[x[0]][x[1]] = v
                    x = pm[x]
        sig = [[self.shifts[pm[(j, t)][0]] * dom[pm[(j, t)][1]] % R for t in range(u)] + [rnd.randrange(R) for _ in range(T - u)]
               for j in range(3)]
        a, b, c = wires
        qm, ql = ([rnd.randrange(R) for _ in range(u)] for _ in range(2))
        qc = [-(qm[t] * a[t] % R * b[t] + ql[t] * (a[t] + b[t]) - c[t]) % R for t in range(u)]
        pad0 = [0] * (T - u)
        table = list(c)
        rnd.shuffle(table)
        table += [rnd.randrange(R) for _ in range(T - u)]     # a fixed column: its padding is public, and not read
        self.beta, self.gamma, self.theta, self.lbeta, self.alpha = (rnd.randrange(R) for _ in range(5))
        self.fixed = {QM: qm + pad0, QL: ql + pad0, QC: qc + pad0, S1: sig[0], S2: sig[1], S3: sig[2],
                      ACT: active_row(T, u), LU: last_row(T, u), TAB: table}
        self.usable_wires = wires
        al = self.alpha
        self.terms = [(1, [QM, A_, B_]), (1, [QL, A_]), (1, [QL, B_]), (R - 1, [ACT, C_]), (1, [QC]),
                      (pow(al, 5, R), [Z_, LU]), (-pow(al, 5, R) % R, [LU]), (pow(al, 6, R), [SUM, LU])]
        self.perm = {"wires": [A_, B_, C_], "sigmas": [S1, S2, S3], "z": Z_, "shifts": self.shifts, "beta": self.beta,
                     "gamma": self.gamma, "alpha": al}
        self.lookup = {"inputs": [C_], "table": [TAB], "mult": M_, "sum": SUM, "width": 1, "theta": self.theta,
                       "beta": self.lbeta, "alpha": al}
        self.active = ACT
        self.pad(seed)

    def pad(self, pad_seed, wires=None):
        """(re)draws every random padding value -- the wires' rows >= usable and the tails of m, z and S -- and rebuilds m, z
        and S; wires: other usable wire values (a broken instance)"""
        rnd = random.Random(pad_seed * 86028121 + 17)
        T, u = self.T, self.usable
        w = wires or self.usable_wires
        self.wires = [list(col) + [rnd.randrange(R) for _ in range(T - u)] for col in w]
        self.tails = {name: [rnd.randrange(R) for _ in range(T - u - 1)] for name in ("m", "z", "S")}
        sig = [self.fixed[S1], self.fixed[S2], self.fixed[S3]]
        self.m, self.missing = multiplicities_zk([self.wires[2]], [self.fixed[TAB]], 1, 1, u, self.tails["m"])
        self.z, self.z_closing = grand_product_zk(self.wires, sig, self.shifts, self.beta, self.gamma, u, self.tails["z"])
        self.S, self.S_closing = lookup_sum_zk([self.wires[2]], [self.fixed[TAB]], self.m, 1, 1, self.theta, self.lbeta, u,
                                               self.tails["S"])
        return self

    def broken(self, pad_seed=None):
        """the same padding (or a new one) with ONE usable cell of wire a altered"""
        w = [list(col) for col in self.usable_wires]
        w[0][self.usable // 2] = (w[0][self.usable // 2] + 1) % R
        return self.pad(self.seed if pad_seed is None else pad_seed, w)

    @property
    def rows(self):
        out = [None] * 15
        out[A_], out[B_], out[C_] = self.wires
        for j, v in self.fixed.items():
            out[j] = v
        out[M_], out[Z_], out[SUM] = self.m, self.z, self.S
        return out

    def coeff_rows(self):
        return [qr.coeffs_of(r) for r in self.rows]
