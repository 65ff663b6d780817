"""The definition of kzg_rows_commit_recurrence in Python integers.  cols: the source columns, T integers in [0, r) each, cell t
the column's value at w_T^t.  recs: a list of (mul_terms, add_terms, start) entries; both term lists in the format of
tests/expr_ref.py ((coefficient, factors) per term, a factor a row index or a (row, rot) pair); an empty mul_terms is A = 1, an
empty add_terms is B = 0.  With n = T in the plain layout and n = usable otherwise
    v[0] = start,   v[t + 1] = A[t] v[t] + B[t]   for 0 <= t < n,
A[t] and B[t] the expressions' values at row t (a rotated factor reads the cell it lands on, even at or behind `usable`; no
cell is read on behalf of a row t >= n).  Plain layout: the output row is v[0] .. v[T - 1] and the closing value v[T].  Usable
layout: rows 0 .. usable are v[0] .. v[usable], the last of them the closing value, and row usable + 1 + s of column c is
tail[c * (T - usable - 1) + s] (column-major over the recurrences)."""
from tests import expr_ref as xref
from tests.gpu_common import R


def scan(a, b, start):
    """[v[0], .., v[n]] of v[t + 1] = a[t] v[t] + b[t]"""
    v = [start % R]
    for x, y in zip(a, b):
        v.append((x * v[-1] + y) % R)
    return v


def sides(cols, rec, n):
    """(A[0 .. n), B[0 .. n)) of one recurrence"""
    mul, add = rec[0], rec[1]
    assert mul or add, "both expressions empty"
    a = xref.evaluate(cols, mul, n) if mul else [1] * n
    b = xref.evaluate(cols, add, n) if add else [0] * n
    return a, b


def recurrence_columns(cols, recs, usable=None, tail=()):
    """(the output rows, the closing values)"""
    T = len(cols[0])
    n = T if usable is None else usable
    assert all(len(c) == T for c in cols)
    assert usable is None or 1 <= usable <= T - 1
    per = 0 if usable is None else T - usable - 1
    assert len(tail) == len(recs) * per, (len(tail), len(recs), per)
    rows, closings = [], []
    for c, rec in enumerate(recs):
        a, b = sides(cols, rec, n)
        v = scan(a, b, rec[2])
        closings.append(v[n])
        if usable is None:
            rows.append(v[:T])
        else:
            rows.append(v[:n + 1] + [x % R for x in tail[c * per:(c + 1) * per]])
        assert len(rows[-1]) == T
    return rows, closings


def plan(n, l0=None, top_max=2048):
    """the level plan as the header states it: {"K", "l", "n", "off"}; l0 = None: 2 below 2^17, 3 below 2^18, else 4"""
    if l0 is None:
        l0 = 2 if n < 1 << 17 else 3 if n < 1 << 18 else 4
    ls, ns, offs = [], [n], [0]
    while ns[-1] > top_max:
        l = l0 if len(ns) == 1 else 4
        ls.append(l)
        offs.append(offs[-1] + ns[-1] if len(ns) > 1 else 0)
        ns.append((ns[-1] + (1 << l) - 1) >> l)
    return {"K": len(ls), "l": ls + [0], "n": ns, "off": offs}
