"""The quotient in parts (kzg_rows_quotient_part / _finish) and the chained grand product (kzg_rows_commit_grand_product_chain)
from their definitions, in Python integers, on top of the references that exist (tests/blinding_ref.py, quotient_ext_ref.py,
quotient_ref.py, grand_product_ref.py: imported, not edited) -- the reference of tests/test_quotient_parts_cpu.py (which pins
it) and tests/test_gpu_quotient_parts.py (which compares the GPU with it).
A part is a dict: rows (its OWN list of coefficient rows, numbered from 0), terms, perm, lookup, active, link, scale.  The whole
numerator is sum_p scale_p num_p.  The linked P2, (z - f_prev(w^rot X)) L_0, goes by another route than the device's: the
unlinked numerator of blinding_ref plus the gate terms +alpha^2 L_0 and -alpha^2 f_prev(w^rot X) L_0 over an explicit row that
holds L_0's evaluations (1 at row 0)."""
import random

from tests import blinding_ref as br
from tests import grand_product_ref as gp
from tests import quotient_ext_ref as qx
from tests import quotient_ref as qr

R = gp.R
be, row_bytes = gp.be, gp.row_bytes


def part(rows, terms, perm=None, lookup=None, active=None, link=None, scale=1):
    return {"rows": rows, "terms": terms, "perm": perm, "lookup": lookup, "active": active, "link": link, "scale": scale}


def part_numerator(p, ext_log):
    """coefficients of one part's numerator (before its scale)"""
    rows, terms = p["rows"], list(p["terms"])
    if p["link"] is not None:
        prev, rot = p["link"]
        T = len(rows[0])
        l0 = len(rows)
        rows = list(rows) + [qr.coeffs_of([1] + [0] * (T - 1))]
        a2 = pow(p["perm"]["alpha"], 2, R)
        terms += [(a2, [l0]), (-a2 % R, [(prev, rot), l0])]
    return br.numerator(rows, terms, p["perm"], p["lookup"], p["active"], ext_log)


def numerator(parts, ext_log):
    acc = [0]
    for p in parts:
        acc = qr.add(acc, qr.scale(part_numerator(p, ext_log), p["scale"] % R))
    return acc


def quotient(parts, ext_log):
    """(t's coefficients, trimmed; the remainder's T coefficients)"""
    q, rem = qr.divide_by_vanishing(numerator(parts, ext_log), len(parts[0]["rows"][0]))
    return qr.trim(q), rem


def num_at(parts_vals, x, T):
    """sum_p scale_p num_p(x) from row values alone: parts_vals = [(part, val)], val(j, rot) = the part's row j at w^rot x"""
    acc = 0
    for p, val in parts_vals:
        v = br.num_at(val, p["terms"], p["perm"], p["lookup"], p["active"], x, T)
        if p["link"] is not None:
            prev, rot = p["link"]
            l0 = (pow(x, T, R) - 1) * pow(T * (x - 1) % R, -1, R) % R
            v += pow(p["perm"]["alpha"], 2, R) * (1 - val(prev, rot)) % R * l0
        acc += p["scale"] * v
    return acc % R


def grand_product_chain(wires, sigmas, shifts, beta, gamma, usable, tail, start):
    """(z's T evaluations, closing): grand_product_zk scaled by start on the rows <= usable, the tail untouched"""
    assert 0 < start < R
    z, closing = br.grand_product_zk(wires, sigmas, shifts, beta, gamma, usable, tail)
    return [start * v % R for v in z[:usable + 1]] + z[usable + 1:], start * closing % R


# ---------------------------------------------------------------------------------------------------- a wide instance
# 20 distinct rows: w0 .. w5 | sigma0 .. sigma5 | qM qL qR qC | A L_u | z0 z1
W0, W1, W2, W3, W4, W5, G0, G1, G2, G3, G4, G5, QM, QL, QR, QC, ACT, LU, Z0, Z1 = range(20)
NAMES = 20


class WideInstance:
    """a SATISFIED circuit on the first `usable` of T rows that fits no single quotient call: 6 wires under ONE permutation
    of the 6 * usable usable cells, split into two chunks of 3 = E - 1 columns at ext_log = 2 with the active column, each
    chunk with its own z_c, chained by z_1(1) = z_0(w^u) and closed by (z_1 - 1) L_u (a gate term); the gate qM w0 w1 +
    qL (w2 + w3) + qR w4 - A w5 + qC = 0 with selectors that vanish on the padding rows; RANDOM padding (the wires' rows >=
    usable and both tails).  parts(): three parts -- gate, chunk 0, chunk 1 -- each with its own rows and row numbering, 20
    distinct rows among them.  all_rows: the 20 evaluation rows by the names above."""

    def __init__(self, T, usable, seed):
        self.T, self.usable, self.seed = T, usable, seed
        rnd = random.Random(seed * 7368787 + 1000 * T + usable)
        u, dom = usable, gp.domain(T)
        self.shifts = [pow(7, j, R) for j in range(6)]
        cells = [(j, t) for j in range(6) for t in range(u)]
        image = cells[:]
        rnd.shuffle(image)
        pm = dict(zip(cells, image))
        wires = [[None] * u for _ in range(6)]
        for c in cells:
            if wires[c[0]][c[1]] is None:
                v, x = rnd.randrange(R), c
                while wires[x[0]][x[1]] is None:
                    wires[x[0]][x[1]] = v
                    x = pm[x]
        self.sig = [[self.shifts[pm[(j, t)][0]] * dom[pm[(j, t)][1]] % R for t in range(u)] + [rnd.randrange(R) for _ in range(T - u)]
                    for j in range(6)]
        w = wires
        qm, ql, qrr = ([rnd.randrange(R) for _ in range(u)] for _ in range(3))
        qc = [-(qm[t] * w[0][t] % R * w[1][t] + ql[t] * (w[2][t] + w[3][t]) + qrr[t] * w[4][t] - w[5][t]) % R for t in range(u)]
        pad0 = [0] * (T - u)
        self.sel = [qm + pad0, ql + pad0, qrr + pad0, qc + pad0]
        self.beta, self.gamma, self.alpha = (rnd.randrange(R) for _ in range(3))
        self.scales = [1] + [rnd.randrange(1, R) for _ in range(2)]
        self.usable_wires = wires
        self.link_rot = u
        self.start1 = None            # None: z_0's closing value
        self.pad(seed)

    def pad(self, pad_seed, wires=None):
        rnd = random.Random(pad_seed * 2750159 + 29)
        T, u = self.T, self.usable
        w = wires or self.usable_wires
        self.wires = [list(col) + [rnd.randrange(R) for _ in range(T - u)] for col in w]
        self.tails = [[rnd.randrange(R) for _ in range(T - u - 1)] for _ in range(2)]
        self.build_z()
        return self

    def build_z(self):
        u = self.usable
        self.z0, self.closing0 = grand_product_chain(self.wires[:3], self.sig[:3], self.shifts[:3], self.beta, self.gamma, u,
                                                     self.tails[0], 1)
        s1 = self.closing0 if self.start1 is None else self.start1
        self.z1, self.closing1 = grand_product_chain(self.wires[3:], self.sig[3:], self.shifts[3:], self.beta, self.gamma, u,
                                                     self.tails[1], s1)
        return self

    def denominators_nonzero(self):
        """no D_t = 0 for t < usable in either chunk"""
        for c in (0, 1):
            _, D = gp.factors(self.wires[3 * c:3 * c + 3], self.sig[3 * c:3 * c + 3], self.shifts[3 * c:3 * c + 3], self.beta,
                              self.gamma)
            if any(d == 0 for d in D[:self.usable]):
                return False
        return True

    def broken_cell(self):
        """ONE usable cell of a chunk-2 wire altered (z_0, z_1 rebuilt honestly from the altered wires)"""
        w = [list(col) for col in self.usable_wires]
        w[4][self.usable // 2] = (w[4][self.usable // 2] + 1) % R
        return self.pad(self.seed, w)

    def broken_start(self):
        """z_1 started somewhere else than z_0 closed"""
        self.start1 = (self.closing0 + 1) % R or 1
        return self.build_z()

    def broken_rot(self):
        """the link reads z_0 one row too early"""
        self.link_rot = self.usable - 1
        return self

    @property
    def all_rows(self):
        return self.wires + self.sig + self.sel + [br.active_row(self.T, self.usable), br.last_row(self.T, self.usable),
                                                   self.z0, self.z1]

    # each part: (names of its rows in its own order, terms / perm / link in ITS numbering)
    GATE_ROWS = (W0, W1, W2, W3, W4, W5, QM, QL, QR, QC, ACT)
    CH0_ROWS = (W0, W1, W2, G0, G1, G2, ACT, Z0)
    CH1_ROWS = (Z0, LU, W3, W4, W5, G3, G4, G5, ACT, Z1)

    def layout(self):
        """[(row names, terms, perm, active, link, scale)] in each part's own numbering"""
        al = self.alpha
        g = {n: j for j, n in enumerate(self.GATE_ROWS)}
        gate_terms = [(1, [g[QM], g[W0], g[W1]]), (1, [g[QL], g[W2]]), (1, [g[QL], g[W3]]), (1, [g[QR], g[W4]]),
                      (R - 1, [g[ACT], g[W5]]), (1, [g[QC]])]
        perm0 = {"wires": [0, 1, 2], "sigmas": [3, 4, 5], "z": 7, "shifts": self.shifts[:3], "beta": self.beta,
                 "gamma": self.gamma, "alpha": al}
        perm1 = {"wires": [2, 3, 4], "sigmas": [5, 6, 7], "z": 9, "shifts": self.shifts[3:], "beta": self.beta,
                 "gamma": self.gamma, "alpha": al}
        a3 = pow(al, 3, R)
        close = [(a3, [9, 1]), (-a3 % R, [1])]       # alpha^3 (z_1 - 1) L_u
        return [(self.GATE_ROWS, gate_terms, None, None, None, self.scales[0]),
                (self.CH0_ROWS, [], perm0, 6, None, self.scales[1]),
                (self.CH1_ROWS, close, perm1, 8, (0, self.link_rot), self.scales[2])]

    def parts(self):
        coeff = [qr.coeffs_of(r) for r in self.all_rows]
        return [part([coeff[n] for n in names], terms, perm, None, active, link, scale)
                for names, terms, perm, active, link, scale in self.layout()]


# the instances tests/test_gpu_quotient_parts.py runs on the device, as (lg, usable, seed); tests/test_quotient_parts_cpu.py
# checks their preconditions without one
GPU_WIDE = [(8, (1 << 8) - 5, 21), (16, (1 << 16) - 6, 23)]
GPU_CLIENT = (6, 58, 25)     # the round through the Client's text forms
GPU_SPLIT = [(4, 11, 31), (8, (1 << 8) - 6, 32), (10, (1 << 10) - 6, 33)]     # blinding_ref.Instance, split into three parts
