"""The definition of kzg_rows_commit_expr in Python integers.  cols: the source columns, T integers in [0, r) each, cell t the
column's value at w_T^t.  exprs: a list of (terms,) or (terms, check) entries; terms: (coefficient, factors) per term, a factor
a row index or a (row, rot) pair.  For every row t < n (n = usable, or T in the plain layout)
    v_e[t] = sum_u c_u prod_f cols[row(u,f)][(t + rot(u,f)) mod T]       (a term with no factors is the constant c_u)
A rotated factor reads the cell it lands on, even at or behind `usable`; no cell is read on behalf of a row t >= n.  The entries
without check = True become, in order, the output rows: T integers each, with row usable + s of committed column c equal to
tail[c * (T - usable) + s] (column-major over the committed columns, no closing row).  Every entry, committed or not, yields
the number of rows t < n with v_e[t] != 0 and the smallest such t (None: none)."""
from tests.gpu_common import R


def factor(f):
    """(row, rot) of a factor given as a row index or a (row, rot) pair"""
    return (int(f[0]), int(f[1])) if isinstance(f, (tuple, list)) else (int(f), 0)


def is_check(entry):
    return len(entry) == 2 and bool(entry[1])


def n_out(exprs):
    return sum(1 for e in exprs if not is_check(e))


def evaluate(cols, terms, n):
    """v[t] for t < n"""
    T = len(cols[0])
    out = []
    for t in range(n):
        v = 0
        for c, fs in terms:
            p = c % R
            for f in fs:
                j, rot = factor(f)
                p = p * cols[j][(t + rot) % T] % R
            v += p
        out.append(v % R)
    return out


def expr_columns(cols, exprs, usable=None, tail=()):
    """(the committed rows, nonzero per entry, first per entry)"""
    T = len(cols[0])
    n = T if usable is None else usable
    assert 1 <= n <= T and all(len(c) == T for c in cols)
    w = n_out(exprs)
    assert len(tail) == w * (T - n), (len(tail), w, T, n)
    rows, nonzero, first = [], [], []
    for entry in exprs:
        v = evaluate(cols, entry[0], n)
        nz = [t for t in range(n) if v[t]]
        nonzero.append(len(nz))
        first.append(nz[0] if nz else None)
        if not is_check(entry):
            c = len(rows)
            rows.append(v + [x % R for x in tail[c * (T - n):(c + 1) * (T - n)]])
    return rows, nonzero, first
