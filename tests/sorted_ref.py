"""The definition of kzg_rows_commit_sorted in Python integers: the stable sort of the rows' tuples, the gather of every column
through it, and the caller's tail behind `usable`.  Columns are lists of canonical integers (evaluations at w_T^t)."""


def sort_perm(cols, n_keys, n):
    """the source row of every output row: rows [0, n) by their first n_keys columns, column 0 first, ties by source row"""
    return sorted(range(n), key=lambda t: (tuple(cols[c][t] for c in range(n_keys)), t))


def sorted_columns(cols, n_keys=None, usable=None, tail=()):
    """(the w output columns, the permutation).  usable = None: all T rows are sorted; otherwise rows [0, usable) are, the source
    rows behind are not read, and output row usable + s of column c is tail[c * (T - usable) + s]"""
    w, T = len(cols), len(cols[0])
    n_keys = w if n_keys is None else n_keys
    n = T if usable is None else usable
    assert 1 <= n_keys <= w and 1 <= n <= T and len(tail) == w * (T - n)
    perm = sort_perm(cols, n_keys, n)
    out = [[col[t] for t in perm] + list(tail[c * (T - n):(c + 1) * (T - n)]) for c, col in enumerate(cols)]
    return out, perm
