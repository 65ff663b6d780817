"""The definition of kzg_rows_commit_fetch in Python integers: a dict from key tuple to the SMALLEST table row that holds it, the
payload of that row copied to every cell that asks for the key, zeros and a count where no row answers, and the caller's tail
behind `usable`.  Columns are lists of canonical integers (evaluations at w_T^t)."""


def first_rows(table, n_keys, rows):
    """key tuple -> the smallest of the table's first `rows` rows that holds it"""
    first = {}
    for q in range(rows):
        first.setdefault(tuple(table[c][q] for c in range(n_keys)), q)
    return first


def n_out(w_tab, n_reads, n_keys, with_index=False):
    return n_reads * (w_tab - n_keys + int(with_index))


def fetched_columns(inputs, table, n_reads, n_keys, with_index=False, usable=None, tail=()):
    """(the output columns in read order -- inside a read the index first, then the payload in table order --, missing per read,
    first_missing per read or None).  inputs: n_reads * max(n_keys, 1) columns, read-major; table: w_tab columns, the first
    n_keys of them the key.  n_keys = 0: a read's one column holds row indices, compared as whole integers.  usable = None: all T
    cells are read and all T table rows can answer; otherwise only those below `usable`, and output row usable + s of column c is
    tail[c * (T - usable) + s]"""
    w_tab, T = len(table), len(table[0])
    n = T if usable is None else usable
    n_in = max(n_keys, 1)
    n_pay = w_tab - n_keys
    assert 0 <= n_keys <= w_tab and 1 <= n <= T and len(inputs) == n_reads * n_in and not (with_index and n_keys == 0)
    assert n_pay + int(with_index) >= 1 and len(tail) == n_out(w_tab, n_reads, n_keys, with_index) * (T - n)
    first = first_rows(table, n_keys, n) if n_keys else None
    out, missing, first_missing = [], [], []
    for l in range(n_reads):
        cols = inputs[l * n_in:(l + 1) * n_in]
        qs = []
        for t in range(n):
            if n_keys:
                qs.append(first.get(tuple(col[t] for col in cols)))
            else:
                qs.append(cols[0][t] if cols[0][t] < n else None)
        miss = [t for t, q in enumerate(qs) if q is None]
        missing.append(len(miss))
        first_missing.append(miss[0] if miss else None)
        if with_index:
            out.append([0 if q is None else q for q in qs])
        for p in range(n_pay):
            out.append([0 if q is None else table[n_keys + p][q] for q in qs])
    for c, col in enumerate(out):
        col.extend(tail[c * (T - n):(c + 1) * (T - n)])
    return out, missing, first_missing
