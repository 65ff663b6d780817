"""The lookup calls with per-row selectors (kzg_rows_commit_multiplicities_sel, kzg_rows_commit_lookup_sum_sel and, at the end,
the numerator, quotient and num_at of kzg_rows_commit_quotient_sel with q_l in LK1) from their definitions, in Python integers, on top of the plain references (tests/lookup_ref.py, multiplicities_ref.py, blinding_ref.py:
imported, not edited) -- the reference of tests/test_lookup_sel_cpu.py (which pins it) and tests/test_gpu_lookup_sel.py (which
compares the GPU with it).  `sels` holds one entry per lookup: None (no selector, the constant 1) or the selector row's T
evaluations.  usable = None is the plain layout (all T rows, no closing row); with u = usable < T rows [0, u) carry the
circuit, row u closes and the tail follows, as in blinding_ref."""
import random

from tests import blinding_ref as br   # noqa: F401  (the identities are pinned against it)
from tests import lookup_ref as lr
from tests import multiplicities_ref as mr   # noqa: F401

R = lr.R
be, row_bytes = lr.be, lr.row_bytes


def _layout(T, usable, tail):
    if usable is None:
        assert not tail
        return T
    assert 1 <= usable < T and len(tail) == T - usable - 1
    return usable


def multiplicities_sel(inputs, table, sels, n_lookups, width, usable=None, tail=()):
    """(m's T evaluations, missing): cell (l, t) is probed exactly when sels[l] is None or sels[l][t] != 0 mod r; a probed
    cell counts 1 on the first copy of its tuple, or 1 in `missing`.  Every table row below the layout's bound is built."""
    assert len(inputs) == n_lookups * width and len(table) == width and len(sels) == n_lookups
    T = len(table[0])
    n = _layout(T, usable, tail)
    first = {}
    for t in range(n):
        first.setdefault(tuple(col[t] for col in table), t)
    mult, missing = [0] * n, 0
    for l in range(n_lookups):
        cols = inputs[l * width:(l + 1) * width]
        for t in range(n):
            if sels[l] is not None and sels[l][t] % R == 0:
                continue
            at = first.get(tuple(col[t] for col in cols))
            if at is None:
                missing += 1
            else:
                mult[at] += 1
    if usable is None:
        return mult, missing
    return mult + [0] + [v % R for v in tail], missing


def terms_sel(inputs, table, mult, sels, n_lookups, width, theta, beta, n=None):
    """term_t = sum_l q_l(w^t) / (beta + F_l(w^t)) - m(w^t) / (beta + Tb(w^t)) for t < n (all rows when n is None), q_l = 1
    for a lookup without a selector.  ZeroDivisionError when a denominator of a row < n is 0, enabled or not."""
    assert len(inputs) == n_lookups * width and len(table) == width and len(sels) == n_lookups
    n = len(mult) if n is None else n
    dens = []
    for l in range(n_lookups):
        dens += [(beta + f) % R for f in lr.compress([c[:n] for c in inputs[l * width:(l + 1) * width]], theta)]
    dens += [(beta + f) % R for f in lr.compress([c[:n] for c in table], theta)]
    inv = lr.batch_inverse(dens)
    out = []
    for t in range(n):
        s = sum((1 if sels[l] is None else sels[l][t]) * inv[l * n + t] for l in range(n_lookups))
        out.append((s - mult[t] * inv[n_lookups * n + t]) % R)
    return out


def lookup_sum_sel(inputs, table, mult, sels, n_lookups, width, theta, beta, usable=None, tail=()):
    """(S's T evaluations, closing): S_0 = 0, S_{t+1} = S_t + term_t below the layout's bound; plain layout: closing =
    sum_t term_t and no closing row; _zk layout: S_usable = closing and the tail behind"""
    T = len(mult)
    n = _layout(T, usable, tail)
    S, acc = [], 0
    for x in terms_sel(inputs, table, mult, sels, n_lookups, width, theta, beta, n):
        S.append(acc)
        acc = (acc + x) % R
    if usable is None:
        return S, acc
    return S + [acc] + [v % R for v in tail], acc


def sel_instance(n_lookups, width, T, seed, usable=None):
    """(inputs, table, sels): a satisfied instance.  A table of T distinct random width-tuples; per lookup a random 0/1
    selector column with both values present among the rows that count; enabled cells drawn from the table rows that count,
    DISABLED cells filled with random tuples that are not in the table.  Rows at and behind `usable` (cells, table rows and
    selector values alike) hold random field elements: no call may read them."""
    rnd = random.Random(seed)
    n = T if usable is None else usable
    assert n >= 2
    rows, have = [], set()
    while len(rows) < T:
        tup = tuple(rnd.randrange(R) for _ in range(width))
        if tup not in have:
            have.add(tup)
            rows.append(tup)
    table = [[rows[t][c] for t in range(T)] for c in range(width)]
    inputs = [[0] * T for _ in range(n_lookups * width)]
    sels = []
    for l in range(n_lookups):
        q = [rnd.randrange(2) for _ in range(n)]
        a, b = rnd.sample(range(n), 2)
        q[a], q[b] = 0, 1
        q += [rnd.randrange(R) for _ in range(T - n)]
        sels.append(q)
        for t in range(T):
            if t < n and q[t]:
                tup = rows[rnd.randrange(n)]
            else:
                while True:
                    tup = tuple(rnd.randrange(R) for _ in range(width))
                    if tup not in have:
                        break
            for c in range(width):
                inputs[l * width + c][t] = tup[c]
    return inputs, table, sels


def break_enabled_cell(inputs, table, sels, width, seed, usable=None):
    """a copy of inputs in which ONE enabled cell that counts carries a tuple that is not in the table"""
    rnd = random.Random(seed)
    T = len(table[0])
    n = T if usable is None else usable
    have = {tuple(col[t] for col in table) for t in range(T)}
    cells = [(l, t) for l in range(len(sels)) for t in range(n) if sels[l] is None or sels[l][t] % R]
    l, t = cells[rnd.randrange(len(cells))]
    while True:
        tup = tuple(rnd.randrange(R) for _ in range(width))
        if tup not in have:
            break
    out = [col[:] for col in inputs]
    for c in range(width):
        out[l * width + c][t] = tup[c]
    return out


# ---------------------------------------------------------------------------------------------------- the quotient
# LK1 is linear in the selectors: with D_0 = beta + Tb and D_l = beta + F_l,
#   LK1(q) = LK1(1) + sum_l (1 - q_l) prod_{l' != l, l' = 0..L} D_l'
# so the numerator and num_at are blinding_ref's plus alpha^3 [A] times that correction.
from tests import quotient_ref as qr   # noqa: E402


def _dens(lookup, at):
    """[D_0, D_1, .., D_L] from at(row) -> the row's value(s): integers, or lists of pointwise values"""
    w, theta, beta = lookup["width"], lookup["theta"], lookup["beta"]
    groups = [lookup["table"]] + [lookup["inputs"][l * w:(l + 1) * w] for l in range(len(lookup["inputs"]) // w)]
    out = []
    for g in groups:
        vals = [at(j) for j in g]
        if isinstance(vals[0], list):
            out.append([(beta + sum(pow(theta, c, R) * v[t] for c, v in enumerate(vals))) % R for t in range(len(vals[0]))])
        else:
            out.append((beta + sum(pow(theta, c, R) * v for c, v in enumerate(vals))) % R)
    return out


def _correction(D, q_of, sels):
    """sum over the selected lookups of (1 - q_l) prod_{l' != l} D_l' from integers"""
    acc = 0
    for l, j in enumerate(sels):
        if j is None:
            continue
        p = 1
        for lp, d in enumerate(D):
            if lp != l + 1:
                p = p * d % R
        acc += (1 - q_of(j)) * p
    return acc % R


def numerator_sel(rows, terms, perm, lookup, sels, active, ext_log):
    """coefficients of num with q_l in LK1 over the coefficient rows `rows`; sels: per lookup a row index or None"""
    num = br.numerator(rows, terms, perm, lookup, active, ext_log)
    if sels is None or all(j is None for j in sels):
        return num
    T, E = len(rows[0]), 1 << ext_log
    n = 1
    while n < (E + 1) * T:
        n *= 2
    dom = qr.Domain(n)
    ev = {}
    at = lambda j: ev.setdefault(j, dom.ev(rows[j]))   # noqa: E731
    D = _dens(lookup, at)
    A = at(active) if active is not None else None
    corr = []
    for t in range(n):
        c = _correction([d[t] for d in D], lambda j: at(j)[t], sels)
        corr.append(c * A[t] % R if A is not None else c)
    return qr.add(num, qr.scale(dom.back(corr), pow(lookup["alpha"], 3, R)))


def quotient_sel(rows, terms, perm, lookup, sels, active, ext_log):
    """(t's coefficients, trimmed; the remainder's T coefficients)"""
    q, rem = qr.divide_by_vanishing(numerator_sel(rows, terms, perm, lookup, sels, active, ext_log), len(rows[0]))
    return qr.trim(q), rem


def num_at_sel(val, terms, perm, lookup, sels, active, x, T):
    """num(x) from row values alone: val(j, rot) = f_j(w^rot x) as an integer"""
    acc = br.num_at(val, terms, perm, lookup, active, x, T)
    if sels is None or all(j is None for j in sels):
        return acc
    c = _correction(_dens(lookup, lambda j: val(j, 0)), lambda j: val(j, 0), sels)
    if active is not None:
        c = c * val(active, 0) % R
    return (acc + pow(lookup["alpha"], 3, R) * c) % R


class QuotInstance:
    """a satisfied lookup-only circuit for the quotient: rows (evaluations) in the order inputs (L w) | table (w) | selectors
    (L) | A | L_u | m | S.  usable = None: the plain layout, no active column (A and L_u are still rows, unused).  With usable
    the closing relation S L_u is a gate term with alpha^5, as in blinding_ref."""

    def __init__(self, L, w, T, seed, usable=None, broken=False):
        rnd = random.Random(seed * 7919 + T)
        self.L, self.w, self.T, self.usable = L, w, T, usable
        inputs, table, sels = sel_instance(L, w, T, seed, usable)
        if broken:
            inputs = break_enabled_cell(inputs, table, sels, w, seed, usable)
        self.theta, self.beta, self.alpha = (rnd.randrange(R) for _ in range(3))
        tail = lambda: [] if usable is None else [rnd.randrange(R) for _ in range(T - usable - 1)]   # noqa: E731
        self.m, self.missing = multiplicities_sel(inputs, table, sels, L, w, usable, tail())
        self.S, self.closing = lookup_sum_sel(inputs, table, self.m, sels, L, w, self.theta, self.beta, usable, tail())
        u = T if usable is None else usable
        A, Lu = br.active_row(T, u), (br.last_row(T, usable) if usable is not None else [0] * T)
        self.rows = inputs + table + sels + [A, Lu, self.m, self.S]
        n_in = L * w
        self.sel_rows = [n_in + w + l for l in range(L)]
        self.active = n_in + w + L if usable is not None else None
        lu, self.m_row, self.s_row = n_in + w + L + 1, n_in + w + L + 2, n_in + w + L + 3
        self.lookup = {"inputs": list(range(n_in)), "table": list(range(n_in, n_in + w)), "mult": self.m_row, "sum": self.s_row,
                       "width": w, "theta": self.theta, "beta": self.beta, "alpha": self.alpha}
        self.terms = [(pow(self.alpha, 5, R), [self.s_row, lu])] if usable is not None else []

    def coeff_rows(self):
        return [qr.coeffs_of(r) for r in self.rows]
