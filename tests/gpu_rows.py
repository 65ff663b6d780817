"""Row-set helpers of the `-m gpu` test modules, each defined once: the engine and SRS caches behind the modules' fixtures,
committing and releasing sets, random rows and tails, the error check, the one-row checker and the piece checker, and the
byte forms and call wrappers of the quotient builders.  Importing this module needs no device: the checkers only call
`eval_rows` on the engine they are given and read `k`, `i`, `T` and `commitments` of the set, and
tests/test_gpu_harness_cpu.py runs them against stubs built from the C oracle."""
import ctypes
import functools
import random

import pytest

from oracle import cpu as oc
from tests import grand_product_ref as gp
from tests import quotient_ext_ref as qx
from tests import quotient_ref as qr
from tests.gpu_common import R, be, ints, rand_scalars_bytes, row_bytes
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError


# ---------------------------------------------------------------------------------------------------- fixtures' bodies
def engine_cache(hip, seed_x, seed_y):
    """one context per log2 row length, holding worker 0's slice of a 2^lg-point SRS (machines_scale 0)"""
    cache = {}

    def get(lg):
        if lg not in cache:
            eng = hip()
            eng.gen_srs(seed_x + lg, seed_y, lg, 0)
            cache[lg] = eng
        return cache[lg]

    return get


def srs_cache(seed_x, seed_y):
    """the oracle's SRS slice of engine_cache's context of the same seeds, one per log2 row length"""
    cache = {}

    def get(lg):
        if lg not in cache:
            cache[lg] = oc.srs_gen(be(seed_x + lg), be(seed_y), lg, 0, 0)
        return cache[lg]

    return get


# ---------------------------------------------------------------------------------------------------- rows and sets
def rand_rows(k, T, seed):
    return [ints(rand_scalars_bytes(T, seed + j)) for j in range(k)]


def tail_of(T, u, seed):
    """the T - u - 1 random blinding values behind the closing row u (u = None, the plain layout: none)"""
    rnd = random.Random(seed)
    return [] if u is None else [rnd.randrange(R) for _ in range(T - u - 1)]


def bt(tail):
    return [be(v) for v in tail]


def commit_sets(eng, rows, sizes, ef=True, i=0):
    """`rows` over len(sizes) sets of sizes[n] rows each.  Rows given as bytes are committed as they are, in the form `ef`
    names.  Rows given as lists of integers are evaluations: committed in evaluation form or (through the oracle's INTT) in
    coefficient form."""
    assert sum(sizes) == len(rows), (sizes, len(rows))
    if rows and not isinstance(rows[0], (bytes, bytearray)):
        rows = [row_bytes(v) for v in rows]
        if not ef:
            rows = [oc.fr_ntt(r, True) for r in rows]
    sets, o = [], 0
    for s in sizes:
        sets.append(eng.commit_rows(i, rows[o:o + s], ef))
        o += s
    return sets


def release(sets):
    for s in sets:
        s.release()


def split_first(k):
    """k rows over two sets: the first row alone"""
    return (k,) if k < 3 else (1, k - 1)


def split_halves(k):
    """k rows over two sets of (almost) equal size"""
    return (k,) if k < 3 else (k // 2, k - k // 2)


def arg_error(fn, why=None, code=_native.KZG_E_ARG):
    """fn() raises KzgError with `code` and, where given, `why` in its message; returns the error"""
    with pytest.raises(KzgError) as ei:
        fn()
    assert ei.value.code == code, ei.value
    if why:
        assert why in str(ei.value), str(ei.value)
    return ei.value


# ---------------------------------------------------------------------------------------------------- the checkers
def probes_ends(T, rnd):
    """{0, 1 % T, T - 1} and three random domain indices (three draws from rnd)"""
    return sorted({0, 1 % T, T - 1} | {rnd.randrange(T) for _ in range(3)})


def probes_closing(T, u):
    """the ends and the indices around the closing row u (u = None, the plain layout: T - 1)"""
    u = T - 1 if u is None else u
    return sorted({0, u - 1, u, min(u + 1, T - 1), T - 1})


def check_one_row(eng, srs, rset, row, rnd, *, probes, i=0, want_commitment=None):
    """the one-row set `rset` against its expected evaluations `row` (integers): its shape, the oracle's commitment of the
    row (want_commitment: that commitment, where the caller has it already), the values at the domain indices `probes` and
    the value at one random point (one draw from rnd) against the oracle's evaluation of the inverse transform"""
    T = len(row)
    rb = row_bytes(row)
    assert (rset.k, rset.i, rset.T, len(rset.commitments)) == (1, i, T, 1)
    assert rset.commitments[0] == (want_commitment or oc.commit(srs, rb, True))
    w = gp.omega(T)
    ts = sorted(set(probes))
    for t0 in range(0, len(ts), 4):
        part = ts[t0:t0 + 4]
        Y = eng.eval_rows([rset], [be(pow(w, t, R)) for t in part], [[0]] * len(part))
        assert [y[0] for y in Y] == [be(row[t]) for t in part], part
    x = be(rnd.randrange(R))
    assert eng.eval_rows([rset], [x], [[0]])[0][0] == oc.fr_eval(oc.fr_ntt(rb, True), x)


def check_pieces(eng, srs, tset, want, rnd, i=0):
    """the set of quotient pieces `tset` against the expected coefficient rows `want`: its shape, the commitments against
    the oracle's, the evaluations at domain points and at a random point against the oracle's"""
    P, T = len(want), len(want[0])
    assert (tset.k, tset.i, tset.T, len(tset.commitments)) == (P, i, T, P)
    wb = [row_bytes(w) for w in want]
    for p in range(P):
        assert tset.commitments[p] == oc.commit(srs, wb[p], False), p
    w = gp.omega(T)
    pts = [be(pow(w, t, R)) for t in (0, T - 1, rnd.randrange(T))] + [be(rnd.randrange(R))]
    Y = eng.eval_rows([tset], pts, [list(range(P))] * len(pts))
    for x, ys in zip(pts, Y):
        assert ys == [oc.fr_eval(wb[p], x) for p in range(P)]


# ---------------------------------------------------------------------------------------------------- the quotient builders
def b_terms(terms):
    return [(be(c), fs) for c, fs in terms]


def b_perm(perm):
    if perm is None:
        return None
    out = dict(perm)
    out["shifts"] = [be(s) for s in perm["shifts"]]
    for name in ("beta", "gamma", "alpha"):
        out[name] = be(perm[name])
    return out


def b_lookup(lookup):
    if lookup is None:
        return None
    out = dict(lookup)
    for name in ("theta", "beta", "alpha"):
        out[name] = be(lookup[name])
    return out


def q_call(eng, sets, terms, perm, ext_log=2, n_pieces=3):
    return eng.commit_quotient(sets, b_terms(terms), b_perm(perm), ext_log, n_pieces)


def x_call(eng, sets, terms, perm=None, lookup=None, ext_log=2, n_pieces=3):
    return eng.commit_quotient_ext(sets, b_terms(terms), b_perm(perm), b_lookup(lookup), ext_log, n_pieces)


def zk_call(eng, sets, terms, perm=None, lookup=None, active=None, ext_log=2, n_pieces=3):
    return eng.commit_quotient_zk(sets, b_terms(terms), b_perm(perm), b_lookup(lookup), active, ext_log, n_pieces)


def c_args(terms, perm, lookup, rots=True):
    """the three argument structs from byte-valued parts (and everything that must outlive the call)"""
    lens = (ctypes.c_uint32 * max(len(terms), 1))(*[len(fs) for _, fs in terms])
    flat = [qx.factor(f) for _, fs in terms for f in fs]
    tr = (ctypes.c_uint32 * max(len(flat), 1))(*[j for j, _ in flat])
    ro = (ctypes.c_int32 * max(len(flat), 1))(*[rot for _, rot in flat]) if rots else None
    gate = _native.QuotientTerms(len(terms), b"".join(c for c, _ in terms), lens, tr, ro)
    pm = lk = None
    if perm:
        pm = _native.QuotientPerm(len(perm["wires"]), perm["z"], (ctypes.c_uint32 * 16)(*perm["wires"]),
                                  (ctypes.c_uint32 * 16)(*perm["sigmas"]), b"".join(perm["shifts"]), perm["beta"], perm["gamma"],
                                  perm["alpha"])
    if lookup:
        w = lookup["width"]
        lk = _native.QuotientLookup(lookup.get("L", len(lookup["inputs"]) // max(w, 1)), w,
                                    (ctypes.c_uint32 * 32)(*lookup["inputs"]), (ctypes.c_uint32 * 32)(*lookup["table"]),
                                    lookup["mult"], lookup["sum"], lookup["theta"], lookup["beta"], lookup["alpha"])
    ref = lambda x: ctypes.byref(x) if x is not None else None   # noqa: E731
    return ref(gate), ref(pm), ref(lk), (gate, pm, lk, lens, tr, ro)


def reference_pieces(rows, terms, perm, ext_log, P):
    """the P piece rows of t over the evaluation rows `rows`, from tests/quotient_ref.py; the remainder must vanish"""
    t, rem = qr.quotient([qr.coeffs_of(r) for r in rows], terms, perm, ext_log)
    assert not any(rem)
    return qr.pieces(t, len(rows[0]), P)


def reference_pieces_ext(rows, terms, perm, lookup, ext_log, P):
    """the same with rotated factors and the lookup part, from tests/quotient_ext_ref.py"""
    t, rem = qx.quotient([qr.coeffs_of(r) for r in rows], terms, perm, lookup, ext_log)
    assert not any(rem)
    return qr.pieces(t, len(rows[0]), P)


@functools.lru_cache(maxsize=None)
def standard(lg, seed=1):
    rows, terms, perm = qr.standard_instance(1 << lg, seed)
    return rows, terms, perm, reference_pieces(rows, terms, perm, 2, 3)
