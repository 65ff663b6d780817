"""The definition of kzg_rows_commit_ec in Python integers: a b^-1 mod p, the affine addition of two points with the doubling,
and the accumulator trace of a chain, over an odd modulus p that need not be prime.  A wide value is L consecutive limb rows of
b bits, little-endian; a cell is its canonical integer reduced to b bits; an operand at or above p is reduced mod p; a row with
either is counted once per unit.  The inverse is pow(x, -1, p) guarded by math.gcd.  tests/test_ec_cpu.py pins this file
against the group law of secp256k1."""
import math

ADD_NAMES = ("lam", "x3", "y3")
CHAIN_NAMES = ("ax", "ay", "lam")
STATS = ("counts", "first", "singular", "first_singular", "mismatch", "first_mismatch", "unknown", "first_unknown", "segments")

# secp256k1: y^2 = x^3 + 7 over p, the generator G of order n
SECP_P = 2**256 - 2**32 - 977
SECP_N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
SECP_GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
SECP_GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
SECP = {"bits": 64, "limbs": 4, "p": SECP_P, "a": 0}


def inverse(x, p):
    """x^-1 mod p, or None where gcd(x mod p, p) != 1 (x = 0 mod p included)"""
    x %= p
    return pow(x, -1, p) if math.gcd(x, p) == 1 else None


def div(curve, a, b):
    """(a b^-1 mod p, singular)"""
    p = curve["p"]
    i = inverse(b, p)
    return (0, True) if i is None else (a % p * i % p, False)


def add(curve, x1, y1, x2, y2):
    """(lam, x3, y3, exceptional) of (x1, y1) + (x2, y2): the chord where x1 != x2, the tangent where the points are equal, and
    the exceptional row (zeros) where the denominator has no inverse"""
    p, a = curve["p"], curve["a"]
    x1, y1, x2, y2 = x1 % p, y1 % p, x2 % p, y2 % p
    if x1 != x2:
        num, den = y2 - y1, x2 - x1
    elif y1 == y2:
        num, den = 3 * x1 * x1 + a, 2 * y1
    else:
        return 0, 0, 0, True
    i = inverse(den, p)
    if i is None:
        return 0, 0, 0, True
    lam = num * i % p
    x3 = (lam * lam - x1 - x2) % p
    return lam, x3, (lam * (x1 - x3) - y1) % p, False


def limbs(v, curve):
    b = curve["bits"]
    return [(v >> (b * l)) & ((1 << b) - 1) for l in range(curve["limbs"])]


def value(cols, first, curve, t):
    """(the wide value of the rows first .. first + L - 1 at row t, reduced mod p; whether a limb or the value was out of range)"""
    b, mask = curve["bits"], (1 << curve["bits"]) - 1
    cells = [cols[first + l][t] for l in range(curve["limbs"])]
    v = sum((c & mask) << (b * l) for l, c in enumerate(cells))
    return v % curve["p"], any(c > mask for c in cells) or v >= curve["p"]


def wide_rows(values, curve):
    """the L limb rows of a list of values"""
    per = [limbs(v, curve) for v in values]
    return [[per[t][l] for t in range(len(values))] for l in range(curve["limbs"])]


class Seen:
    def __init__(self):
        self.rows = {k: [] for k in ("counts", "singular", "mismatch", "unknown")}
        self.segments = 0

    def stats(self):
        out = {"segments": self.segments}
        for k, first in (("counts", "first"), ("singular", "first_singular"), ("mismatch", "first_mismatch"),
                         ("unknown", "first_unknown")):
            out[k], out[first] = len(self.rows[k]), (min(self.rows[k]) if self.rows[k] else None)
        return out


def unit_values(cols, curve, unit, n, seen):
    """the named values of a unit, {name: list of n integers}"""
    mode = unit["mode"]
    if mode == "div":
        r = []
        for t in range(n):
            a, over = value(cols, unit["a"], curve, t)
            if isinstance(unit["b"], (list, tuple)):
                b = unit["b"][1] % curve["p"]
            else:
                b, o = value(cols, unit["b"], curve, t)
                over |= o
            q, sing = div(curve, a, b)
            r.append(q)
            if over:
                seen.rows["counts"].append(t)
            if sing:
                seen.rows["singular"].append(t)
        return {"r": r}
    if mode == "add":
        out = {k: [] for k in ADD_NAMES}
        for t in range(n):
            ops = [value(cols, unit[k], curve, t) for k in ("x1", "y1", "x2", "y2")]
            lam, x3, y3, sing = add(curve, *[v for v, _ in ops])
            for k, v in zip(ADD_NAMES, (lam, x3, y3)):
                out[k].append(v)
            if any(o for _, o in ops):
                seen.rows["counts"].append(t)
            if sing:
                seen.rows["singular"].append(t)
        return out
    assert mode == "chain"
    out = {k: [] for k in CHAIN_NAMES}
    ax = ay = 0
    for t in range(n):
        code = cols[unit["op"]][t]
        out["ax"].append(ax)
        out["ay"].append(ay)
        lam = 0
        if t == 0 or code == 1:
            seen.segments += 1
        if code in (1, 2):
            (px, o1), (py, o2) = value(cols, unit["px"], curve, t), value(cols, unit["py"], curve, t)
            if o1 or o2:
                seen.rows["counts"].append(t)
            if code == 1:
                ax, ay = px, py
            else:
                lam, ax, ay, sing = add(curve, ax, ay, px, py)
                if sing:
                    seen.rows["singular"].append(t)
        elif code == 3:
            lam, ax, ay, sing = add(curve, ax, ay, ax, ay)
            if sing:
                seen.rows["singular"].append(t)
        elif code != 0:
            seen.rows["unknown"].append(t)
        out["lam"].append(lam)
    return out


def columns(cols, curve, units, usable=None, tail=()):
    """what commit_ec returns for these units over the evaluation columns `cols`: (the committed rows in unit order with the
    caller's tail behind `usable`, the statistics)"""
    T = len(cols[0])
    n = T if usable is None else usable
    rows = []
    st = {k: [] for k in STATS}
    for unit in units:
        seen = Seen()
        vals = unit_values(cols, curve, unit, n, seen)
        names = ("r",) if unit["mode"] == "div" else ADD_NAMES if unit["mode"] == "add" else CHAIN_NAMES
        if unit.get("expect") is not None:
            for t in range(n):
                for k, first in zip(names, unit["expect"]):
                    if first is not None and [cols[first + l][t] for l in range(curve["limbs"])] != limbs(vals[k][t], curve):
                        seen.rows["mismatch"].append(t)
                        break
        else:
            picked = names if unit["mode"] == "div" else unit["out" if unit["mode"] == "add" else "cols"]
            for k in names:
                if k in picked:
                    rows += [r + [0] * (T - n) for r in wide_rows(vals[k], curve)]
        for k, v in seen.stats().items():
            st[k].append(v)
    for c, row in enumerate(rows):
        if usable is not None:
            row[n:] = tail[c * (T - n):(c + 1) * (T - n)]
    return rows, st


def scalar_mul_ops(k):
    """the op-codes of k P by double-and-add from the top bit: a load, then per lower bit a doubling and, where the bit is set,
    an addition"""
    assert k >= 1
    ops = [1]
    for bit in bin(k)[3:]:
        ops.append(3)
        if bit == "1":
            ops.append(2)
    return ops
