"""kzg_rows_commit_edwards in Python integers: the definition the device is tested against.

A coordinate is one cell, a field element of Fr (the BLS12-381 scalar field, modulus R).  The curve is A x^2 + y^2 = 1 + D x^2
y^2; the law, with tau = D x1 x2 y1 y2, is x3 = (x1 y2 + y1 x2) / (1 + tau), y3 = (y1 y2 - A x1 x2) / (1 - tau) for EVERY pair
of pairs, equal ones included; tau = 1 or -1 is exceptional.  There is no on-curve check.  The two parameter sets below are
Jubjub and Bandersnatch; test_edwards_cpu.py pins this file by identities that do not use it (the group orders, the group
axioms, an independent double-and-add)."""
from __future__ import annotations

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001

JUBJUB = {"a": R - 1, "d": 0x2a9318e74bfa2b48f5fd9207e6bd7fd4292d7f6d37579d2601065fd6d6343eb1}
JUBJUB_ORDER = 8 * 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7
BANDERSNATCH = {"a": R - 5, "d": 0x6389c12633c267cbc66e3bf86be3b6d8cb66677177e54f92b369f2f5188d58e7}
BANDERSNATCH_ORDER = 4 * 0x1cfb69d4ca675f520cce760202687600ff8f87007419047174fd06b52876e7e1

ADD_NAMES = ("x3", "y3")
CHAIN_NAMES = ("ax", "ay")
STATS = ("singular", "first_singular", "mismatch", "first_mismatch", "unknown", "first_unknown", "segments")
NEUTRAL = (0, 1)


def scalar(v):
    """a coefficient or an immediate as the integer it names: an int, a decimal or 0x string, or 32 big-endian bytes"""
    if isinstance(v, (bytes, bytearray)):
        return int.from_bytes(v, "big")
    return int(v, 0) if isinstance(v, str) else int(v)


def add(curve, x1, y1, x2, y2):
    """(x3, y3, exceptional) of (x1, y1) + (x2, y2); an exceptional pair gives (0, 0, True)"""
    a, d = scalar(curve["a"]), scalar(curve["d"])
    tau = d * x1 * x2 % R * y1 * y2 % R
    if tau in (1, R - 1):
        return 0, 0, True
    x3 = (x1 * y2 + y1 * x2) * pow(1 + tau, -1, R) % R
    y3 = (y1 * y2 - a * x1 * x2) * pow(1 - tau, -1, R) % R
    return x3, y3, False


def on_curve(curve, x, y):
    a, d = scalar(curve["a"]), scalar(curve["d"])
    return (a * x * x + y * y - 1 - d * x * x % R * y * y) % R == 0


def sqrt(v):
    """a square root of v mod R, or None (Tonelli and Shanks: R - 1 = 2^32 q)"""
    v %= R
    if v == 0:
        return 0
    if pow(v, (R - 1) // 2, R) != 1:
        return None
    q, s = R - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (R - 1) // 2, R) != R - 1:
        z += 1
    m, c, t, r = s, pow(z, q, R), pow(v, q, R), pow(v, (q + 1) // 2, R)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % R, i + 1
        b = pow(c, 1 << (m - i - 1), R)
        m, c, t, r = i, b * b % R, t * b * b % R, r * b % R
    return r


def point(curve, seed):
    """a point of the curve: the first y >= seed whose x^2 = (1 - y^2) / (A - D y^2) is a square"""
    a, d = scalar(curve["a"]), scalar(curve["d"])
    y = seed % R
    while True:
        den = (a - d * y * y) % R
        if den:
            x = sqrt((1 - y * y) * pow(den, -1, R))
            if x is not None:
                return x, y
        y = (y + 1) % R


def slot_value(cols, slot, t):
    return scalar(slot[1]) if isinstance(slot, (list, tuple)) else cols[slot][t]


class Seen:
    def __init__(self):
        self.rows = {k: [] for k in ("singular", "mismatch", "unknown")}
        self.segments = 0

    def stats(self):
        out = {"segments": self.segments}
        for k in ("singular", "mismatch", "unknown"):
            out[k], out["first_" + k] = len(self.rows[k]), (min(self.rows[k]) if self.rows[k] else None)
        return out


def unit_values(cols, curve, unit, n, seen):
    """the named values of a unit, {name: list of n integers}"""
    if unit["mode"] == "add":
        out = {k: [] for k in ADD_NAMES}
        for t in range(n):
            x3, y3, sing = add(curve, *[slot_value(cols, unit[k], t) for k in ("x1", "y1", "x2", "y2")])
            out["x3"].append(x3)
            out["y3"].append(y3)
            if sing:
                seen.rows["singular"].append(t)
        return out
    assert unit["mode"] == "chain"
    out = {k: [] for k in CHAIN_NAMES}
    ax, ay = NEUTRAL
    for t in range(n):
        code = cols[unit["op"]][t]
        out["ax"].append(ax)
        out["ay"].append(ay)
        if t == 0 or code == 1:
            seen.segments += 1
        if code == 1:
            ax, ay = slot_value(cols, unit["px"], t), slot_value(cols, unit["py"], t)
        elif code in (2, 3, 4):
            if code == 3:
                px, py = ax, ay
            else:
                px, py = slot_value(cols, unit["px"], t), slot_value(cols, unit["py"], t)
                if code == 4:
                    px = -px % R
            ax, ay, sing = add(curve, ax, ay, px, py)
            if sing:
                seen.rows["singular"].append(t)
                ax, ay = NEUTRAL
        elif code != 0:
            seen.rows["unknown"].append(t)
    return out


def columns(cols, curve, units, usable=None, tail=()):
    """what commit_edwards returns for these units over the evaluation columns `cols`: (the committed rows in unit order, each
    unit's in the order of its names, with the caller's tail behind `usable`, the statistics)"""
    T = len(cols[0])
    n = T if usable is None else usable
    rows = []
    st = {k: [] for k in STATS}
    for unit in units:
        seen = Seen()
        vals = unit_values(cols, curve, unit, n, seen)
        if unit.get("expect") is not None:
            for t in range(n):
                if any(row is not None and cols[row][t] != vals[k][t] for k, row in zip(ADD_NAMES, unit["expect"])):
                    seen.rows["mismatch"].append(t)
        else:
            for k in unit["out" if unit["mode"] == "add" else "cols"]:
                rows.append(list(vals[k]) + [0] * (T - n))
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
