"""The lookup (logUp) running sum of kzg_rows_commit_lookup_sum from its definition, in Python integers -- the reference of
tests/test_lookup_sum_cpu.py (which pins it) and tests/test_gpu_lookup_sum.py (which compares the GPU with it) -- and a
builder of real lookup instances (a table of T random w-tuples, L input columns drawn from its rows, the counts as m)."""
import random

from tests.grand_product_ref import R, batch_inverse, be, domain, row_bytes  # noqa: F401  (re-exported for the tests)


def compress(cols, theta):
    """sum_c theta^c cols[c][t] for every t (cols: w lists of T integers)"""
    T = len(cols[0])
    out = [0] * T
    for col in reversed(cols):   # Horner in c
        out = [(o * theta + v) % R for o, v in zip(out, col)]
    return out


def terms(inputs, table, mult, n_lookups, width, theta, beta):
    """term_t = sum_l 1 / (beta + F_l(w^t)) - m(w^t) / (beta + Tb(w^t)) from the rows' evaluations: inputs holds
    n_lookups * width lists (lookup-major), table width lists, mult one list.  ZeroDivisionError when a denominator is 0."""
    assert len(inputs) == n_lookups * width and len(table) == width
    T = len(mult)
    dens = []
    for l in range(n_lookups):
        dens += [(beta + f) % R for f in compress(inputs[l * width:(l + 1) * width], theta)]
    dens += [(beta + f) % R for f in compress(table, theta)]
    inv = batch_inverse(dens)
    out = []
    for t in range(T):
        s = sum(inv[l * T + t] for l in range(n_lookups)) - mult[t] * inv[n_lookups * T + t]
        out.append(s % R)
    return out


def lookup_sum(inputs, table, mult, n_lookups, width, theta, beta):
    """S(w^t) for t in [0, T) and the closing value: S_0 = 0, S_{t+1} = S_t + term_t, closing = sum_t term_t"""
    S, acc = [], 0
    for x in terms(inputs, table, mult, n_lookups, width, theta, beta):
        S.append(acc)
        acc = (acc + x) % R
    return S, acc


def lookup_instance(n_lookups, width, T, seed, duplicates=False):
    """(inputs, table, mult) as evaluation lists: a table of T random width-tuples, n_lookups input tuples per row drawn
    from the table's rows, mult[t] = how many input cells hit table row t.  duplicates: the table's second half repeats
    rows of its first half; the counts of a repeated tuple are all put on its first copy."""
    rnd = random.Random(seed)
    rows = [tuple(rnd.randrange(R) for _ in range(width)) for _ in range(T)]
    if duplicates:
        for t in range(T // 2, T):
            rows[t] = rows[rnd.randrange(T // 2)]
    first = {}
    for t, tup in enumerate(rows):
        first.setdefault(tup, t)
    mult = [0] * T
    inputs = [[0] * T for _ in range(n_lookups * width)]
    for l in range(n_lookups):
        for t in range(T):
            tup = rows[rnd.randrange(T)]
            mult[first[tup]] += 1
            for c in range(width):
                inputs[l * width + c][t] = tup[c]
    table = [[rows[t][c] for t in range(T)] for c in range(width)]
    return inputs, table, mult


def break_instance(inputs, table, width, seed):
    """a copy of inputs in which one cell's tuple is replaced by a tuple that is not in the table"""
    rnd = random.Random(seed)
    T = len(inputs[0])
    have = {tuple(table[c][t] for c in range(width)) for t in range(T)}
    while True:
        tup = tuple(rnd.randrange(R) for _ in range(width))
        if tup not in have:
            break
    out = [col[:] for col in inputs]
    l, t = rnd.randrange(len(inputs) // width), rnd.randrange(T)
    for c in range(width):
        out[l * width + c][t] = tup[c]
    return out
