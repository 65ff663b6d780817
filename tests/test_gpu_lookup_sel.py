"""GPU tests (`-m gpu`) of the lookup calls with per-row selectors: kzg_rows_commit_multiplicities_sel,
kzg_rows_commit_lookup_sum_sel, kzg_rows_commit_quotient_sel and kzg_rows_quotient_part_sel (the quotient at lg 4 and 8).  The expected rows come from the definitions in Python integers (tests/lookup_sel_ref.py) and
are committed with the C oracle, never with the library under test: commitments, closing values, `missing` and evaluations
are compared bit for bit.  Shapes: T = 2^4 (less than one wave) with usable = 11, T = 2^10 (four 256-lane workgroups, a
multi-level scan) with usable = T - 5 and in the plain layout, the join additionally at 2^12; nothing larger is needed, a
selector changes no transform and no MSM.  The identities against the existing calls' bytes, built instances, mixed and
shared selectors, selectors of arbitrary field elements, the breaker, the zero denominator on a disabled row, rows picked out
of a larger fixed set, every new error, threads, the multi-GPU handle, the structural check (no upload span inside a call)
and one round through the Client follow.  Each test leaves rows_stats() where it found it."""
import ctypes
import hashlib
import random
import threading

import pytest

from oracle import cpu as oc
from tests import grand_product_ref as gp
from tests import lookup_ref as lr
from tests import lookup_sel_ref as ls
from tests.gpu_common import val
from tests.gpu_rows import (arg_error, bt, check_one_row, commit_sets, engine_cache, probes_closing, rand_rows, release,
                            srs_cache, tail_of)
from zkp_subnet_amd import _native, codec
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import lagrange_factor

pytestmark = pytest.mark.gpu
R = ls.R
be, row_bytes = ls.be, ls.row_bytes
E_ARG = _native.KZG_E_ARG
NOSEL = _native.KZG_NO_SELECTOR
SEED_X, SEED_Y = 0x5E1EC7, 0x5E1EC8
LAYOUTS = [(4, 11), (10, (1 << 10) - 5), (10, None)]
layout_id = lambda s: f"T2^{s[0]}-u{s[1]}"   # noqa: E731


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def check_row(eng, srs, rset, row, u, rnd):
    """the one-row set against the expected evaluations: the oracle's commitment of the reference's row, the values around
    the closing row and at the ends, and the value at a random point"""
    check_one_row(eng, srs, rset, row, rnd, probes=probes_closing(len(row), u))


def run(eng, srs, inputs, table, sels, L, w, theta, beta, u, tail, rnd, mult=None):
    """both _sel builders over one selector set that holds the distinct selector rows, against the reference:
    (m, missing, S, closing).  mult: the multiplicity row to sum over (default: the one the join gives)"""
    rows, index = [], []
    for q in sels:
        if q is None:
            index.append(None)
            continue
        at = next((j for j, r in enumerate(rows) if r is q), None)
        if at is None:
            rows.append(q)
            at = len(rows) - 1
        index.append(at)
    m, missing = ls.multiplicities_sel(inputs, table, sels, L, w, u, tail)
    mult = m if mult is None else mult
    F, Tb = commit_sets(eng, inputs, (L * w,)), commit_sets(eng, table, (w,), ef=False)
    Q = commit_sets(eng, rows, (len(rows),)) if rows else []
    M = commit_sets(eng, [mult], (1,))
    try:
        mset, miss = eng.commit_multiplicities_sel(F, Tb, Q, index, L, w, u, bt(tail))
        try:
            assert miss == missing
            check_row(eng, srs, mset, m, u, rnd)
        finally:
            mset.release()
        try:
            S, closing = ls.lookup_sum_sel(inputs, table, mult, sels, L, w, theta, beta, u, tail)
        except ZeroDivisionError:
            S = closing = None
        if S is not None:
            sset, cl = eng.commit_lookup_sum_sel(F, Tb, M[0], Q, index, L, w, be(theta), be(beta), u, bt(tail))
            try:
                assert cl == be(closing)
                check_row(eng, srs, sset, S, u, rnd)
            finally:
                sset.release()
    finally:
        release(F + Tb + Q + M)
    return m, missing, S, closing


# ---------------------------------------------------------------------------------------------------- the identities
@pytest.mark.parametrize("layout", LAYOUTS, ids=layout_id)
def test_no_selector_and_all_ones_are_the_existing_calls(engines, layout):
    """every entry KZG_NO_SELECTOR, then an all-ones selector row (for every lookup, and for one of them): the bytes of
    kzg_rows_commit_multiplicities / _lookup_sum (plain layout) or of their _zk forms"""
    lg, u = layout
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    L, w = 2, 2
    inputs, table, _ = lr.lookup_instance(L, w, T, 100 + lg, duplicates=True)
    inputs[1][3] = (inputs[1][3] + 1) % R
    theta, beta, tail = be(0x7E7A + lg), be(0xBE7A + lg), bt(tail_of(T, u, lg))
    F, Tb, One = commit_sets(eng, inputs, (1, 3)), commit_sets(eng, table, (w,)), commit_sets(eng, [[1] * T], (1,))
    try:
        if u is None:
            mset, miss = eng.commit_multiplicities(F, Tb, L, w)
            sset, cl = eng.commit_lookup_sum(F, Tb, mset, L, w, theta, beta)
        else:
            mset, miss = eng.commit_multiplicities_zk(F, Tb, L, w, u, tail)
            sset, cl = eng.commit_lookup_sum_zk(F, Tb, mset, L, w, theta, beta, u, tail)
        try:
            assert miss >= 1
            x = be(0x1234567 + lg)
            want = (mset.commitments, miss, eng.eval_rows([mset], [x], [[0]]))
            want_s = (sset.commitments, cl, eng.eval_rows([sset], [x], [[0]]))
            for Q, index in (([], [None, None]), (One, [0, 0]), (One, [None, 0])):
                m2, miss2 = eng.commit_multiplicities_sel(F, Tb, Q, index, L, w, u, tail)
                s2, cl2 = eng.commit_lookup_sum_sel(F, Tb, mset, Q, index, L, w, theta, beta, u, tail)
                got = (m2.commitments, miss2, eng.eval_rows([m2], [x], [[0]]))
                got_s = (s2.commitments, cl2, eng.eval_rows([s2], [x], [[0]]))
                release([m2, s2])
                assert got == want and got_s == want_s, index
        finally:
            release([mset, sset])
    finally:
        release(F + Tb + One)
    assert eng.rows_stats() == before


@pytest.mark.parametrize("layout", LAYOUTS, ids=layout_id)
def test_all_zero_selectors_switch_everything_off(engines, srs_of, layout):
    lg, u = layout
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    L, w = 2, 1
    rnd = random.Random(lg)
    zero = [0] * T
    inputs, table = rand_rows(L * w, T, 200 + lg), rand_rows(w, T, 300 + lg)
    n = T if u is None else u
    m, missing, S, closing = run(eng, srs, inputs, table, [zero, zero], L, w, 5, 6, u, tail_of(T, u, 2), rnd)
    assert (m[:n], missing, S[:n], closing) == ([0] * n, 0, [0] * n, 0)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- built instances
@pytest.mark.parametrize("shape", [(1, 1), (3, 2)], ids=lambda s: f"L{s[0]}w{s[1]}")
@pytest.mark.parametrize("layout", LAYOUTS, ids=layout_id)
def test_built_instances_bit_exact(engines, srs_of, layout, shape):
    """satisfied instances whose disabled cells hold tuples that are in no table row: missing = 0 and the sum closes; the
    same rows without selectors miss every disabled cell; one broken enabled cell is one miss and an open sum"""
    lg, u = layout
    L, w = shape
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(1000 * lg + 10 * L + w)
    n = T if u is None else u
    inputs, table, sels = ls.sel_instance(L, w, T, 400 + 10 * lg + L, u)
    theta, beta, tail = rnd.randrange(R), rnd.randrange(R), tail_of(T, u, 3)
    m, missing, S, closing = run(eng, srs, inputs, table, sels, L, w, theta, beta, u, tail, rnd)
    assert (missing, closing) == (0, 0)
    _, missing0, _, closing0 = run(eng, srs, inputs, table, [None] * L, L, w, theta, beta, u, tail, rnd)
    assert missing0 == sum(q[:n].count(0) for q in sels) and closing0 != 0
    broken = ls.break_enabled_cell(inputs, table, sels, w, 6, u)
    _, missing1, _, closing1 = run(eng, srs, broken, table, sels, L, w, theta, beta, u, tail, rnd)
    assert missing1 == 1 and closing1 != 0
    assert eng.rows_stats() == before


def test_the_join_at_two_to_the_twelve(engines, srs_of):
    """sixteen workgroups per probe, the plain layout and a usable bound that is no multiple of the workgroup"""
    lg, L, w = 12, 2, 2
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    for u in (None, T - 7):
        inputs, table, sels = ls.sel_instance(L, w, T, 1200 + (u or 0), u)
        tail = tail_of(T, u, 4)
        m, missing = ls.multiplicities_sel(inputs, table, sels, L, w, u, tail)
        assert missing == 0
        F, Tb, Q = commit_sets(eng, inputs, (L * w,)), commit_sets(eng, table, (w,)), commit_sets(eng, sels, (L,))
        try:
            mset, miss = eng.commit_multiplicities_sel(F, Tb, Q, [0, 1], L, w, u, bt(tail))
            try:
                assert miss == 0
                check_row(eng, srs, mset, m, u, random.Random(12))
            finally:
                mset.release()
        finally:
            release(F + Tb + Q)
    assert eng.rows_stats() == before


@pytest.mark.parametrize("layout", LAYOUTS, ids=layout_id)
def test_mixed_and_shared_selectors(engines, srs_of, layout):
    """three lookups: the first and the third share ONE selector row, the second has none"""
    lg, u = layout
    L, w = 3, 2
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(31 * lg)
    n = T if u is None else u
    inputs, table, sels = ls.sel_instance(L, w, T, 500 + lg, u)
    q = sels[0]
    have = {tuple(col[t] for col in table) for t in range(T)}
    for t in range(T):   # lookup 1 loses its selector: every cell that counts holds a table tuple; lookup 2 follows q
        for l, on in ((1, t < n), (2, t < n and q[t] == 1)):
            if on:
                src = rnd.randrange(n)
                tup = tuple(table[c][src] for c in range(w))
            else:
                while True:
                    tup = tuple(rnd.randrange(R) for _ in range(w))
                    if tup not in have:
                        break
            for c in range(w):
                inputs[l * w + c][t] = tup[c]
    sels = [q, None, q]
    # (sel_instance's q is 0 or 1 on the n rows that count, so its enabled cells number sum(q[:n]); what q holds behind row n is
    # random, and `t < n` above keeps those rows out: lookup 1 hits on all n rows, lookups 0 and 2 on the enabled ones)
    assert set(q[:n]) == {0, 1}
    m, missing, S, closing = run(eng, srs, inputs, table, sels, L, w, rnd.randrange(R), rnd.randrange(R), u, tail_of(T, u, 5), rnd)
    assert (missing, closing) == (0, 0) and sum(m[:n]) == n + 2 * sum(q[:n])
    assert eng.rows_stats() == before


@pytest.mark.parametrize("layout", LAYOUTS, ids=layout_id)
def test_a_selector_of_field_elements(engines, srs_of, layout):
    """0, 1, r - 1 and random elements: the sum follows the weighted definition bit for bit (it has no reason to close), m
    counts the nonzero cells"""
    lg, u = layout
    L, w = 2, 2
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(41 * lg)
    inputs, table, _ = lr.lookup_instance(L, w, T, 600 + lg)
    q = [0, 1, R - 1, 0] + [rnd.randrange(R) for _ in range(T - 4)]
    n = T if u is None else u
    mult = rand_rows(1, T, 650 + lg)[0]
    m, missing, S, closing = run(eng, srs, inputs, table, [q, None], L, w, rnd.randrange(R), rnd.randrange(R), u, tail_of(T, u, 6),
                                 rnd, mult=mult)
    assert sum(m[:n]) + missing == 2 * n - q[:n].count(0) and q[:n].count(0) == 2 and S is not None
    assert eng.rows_stats() == before


def test_rows_picked_out_of_a_larger_fixed_set_and_a_repeated_handle(engines, srs_of):
    """the caller names its whole fixed set (five rows over two sets, one handle given twice) and picks rows 6 and 1"""
    lg, u, L, w = 10, (1 << 10) - 5, 2, 1
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(77)
    inputs, table, sels = ls.sel_instance(L, w, T, 700, u)
    tail = tail_of(T, u, 7)
    theta, beta = rnd.randrange(R), rnd.randrange(R)
    m, missing = ls.multiplicities_sel(inputs, table, sels, L, w, u, tail)
    S, closing = ls.lookup_sum_sel(inputs, table, m, sels, L, w, theta, beta, u, tail)
    other = rand_rows(3, T, 710)
    A = commit_sets(eng, [other[0], sels[1], other[1]], (3,))[0]          # rows 0 1 2, and again 5 6 7
    B = commit_sets(eng, [other[2], sels[0]], (2,), ef=False)[0]          # rows 3 4
    Bb = commit_sets(eng, [sels[0]], (1,))[0]
    F, Tb = commit_sets(eng, inputs, (1, 1)), commit_sets(eng, table, (1,))
    try:
        for Q, index in (([A, B, A], [4, 6]), ([A, B], [4, 1]), ([Bb, A], [0, 2])):
            mset, miss = eng.commit_multiplicities_sel(F, Tb, Q, index, L, w, u, bt(tail))
            try:
                assert miss == missing == 0
                check_row(eng, srs, mset, m, u, rnd)
                sset, cl = eng.commit_lookup_sum_sel(F, Tb, mset, Q, index, L, w, be(theta), be(beta), u, bt(tail))
                try:
                    assert cl == be(closing) == be(0)
                    check_row(eng, srs, sset, S, u, rnd)
                finally:
                    sset.release()
            finally:
                mset.release()
    finally:
        release([A, B, Bb] + F + Tb)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- errors
def test_a_zero_denominator_on_a_disabled_row_is_an_error(engines, srs_of):
    """beta = -F_0 at a DISABLED usable row: KZG_E_ARG, no set, and the context keeps serving; the same zero on a row
    behind `usable` is no error"""
    lg, u, L, w = 10, (1 << 10) - 5, 1, 1
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    inputs, table, sels = ls.sel_instance(L, w, T, 800, u)
    tail = tail_of(T, u, 8)
    m, _ = ls.multiplicities_sel(inputs, table, sels, L, w, u, tail)
    t = sels[0].index(0)
    assert t < u
    F, Tb, Q, M = (commit_sets(eng, x, (1,)) for x in (inputs, table, sels, [m]))
    try:
        for layout in ((u, bt(tail)), (None, [])):
            arg_error(lambda: eng.commit_lookup_sum_sel(F, Tb, M[0], Q, [0], L, w, be(0), be(-inputs[0][t] % R), *layout),
                       "zero denominator")
            assert eng.rows_stats()[0] == before[0] + 4
        beta = -inputs[0][u + 1] % R
        S, closing = ls.lookup_sum_sel(inputs, table, m, sels, L, w, 0, beta, u, tail)
        sset, cl = eng.commit_lookup_sum_sel(F, Tb, M[0], Q, [0], L, w, be(0), be(beta), u, bt(tail))
        try:
            assert cl == be(closing)
            check_row(eng, srs, sset, S, u, random.Random(8))
        finally:
            sset.release()
    finally:
        release(F + Tb + Q + M)
    assert eng.rows_stats() == before


def test_errors_leave_the_context_serving(engines, srs_of, hip):
    lg, u, L, w = 4, 11, 2, 1
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    lib = _native.load()
    inputs, table, sels = ls.sel_instance(L, w, T, 900, u)
    tail = tail_of(T, u, 9)
    m, _ = ls.multiplicities_sel(inputs, table, sels, L, w, u, tail)
    F, Tb, Q, M = commit_sets(eng, inputs, (2,)), commit_sets(eng, table, (1,)), commit_sets(eng, sels, (2,)), commit_sets(eng, [m], (1,))
    other = hip()
    other.gen_srs(SEED_X + 5, SEED_Y, 5, 0)
    long_set = other.commit_rows(0, [row_bytes([1] * 32)], True)
    gone = commit_sets(eng, sels, (2,))[0]
    gone.release()
    tb = bt(tail)
    mul = lambda Qs, idx, uu=u, tl=tb: eng.commit_multiplicities_sel(F, Tb, Qs, idx, L, w, uu, tl)   # noqa: E731
    lks = lambda Qs, idx, uu=u, tl=tb: eng.commit_lookup_sum_sel(F, Tb, M[0], Qs, idx, L, w, be(3), be(4), uu, tl)   # noqa: E731

    def good():
        mset, miss = mul(Q, [0, 1])
        sset, cl = lks(Q, [0, 1])
        release([mset, sset])
        assert (miss, cl) == (0, be(0))
        assert mset.commitments[0] == oc.commit(srs, row_bytes(m), True)

    try:
        good()
        for call in (mul, lks):
            arg_error(lambda: call(Q, [0, 2]), "sel_index")            # out of range
            arg_error(lambda: call(Q, [0, NOSEL - 1]), "sel_index")
            arg_error(lambda: call([], [0, None]), "sel_index")         # a real index with no selector set
            arg_error(lambda: call([gone.handle], [0, 1]), "unknown or released")
            arg_error(lambda: call([0xDEAD], [0, 1]), "unknown or released")
            arg_error(lambda: call(Q, [0]))                             # not n_lookups entries (refused by the binding)
            arg_error(lambda: call(Q, [0, 1], T, tb), "usable")         # usable = T goes with no tail only
            arg_error(lambda: call(Q, [0, 1], 0, []))
            good()
        # a selector set of another row length is a set of another context here: unknown to this one
        arg_error(lambda: mul([long_set.handle], [0, 0]), "unknown or released")
        # the C entry points themselves: null sel_index, null sel_handles with a count, too many handles
        c, cl, h, miss = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.c_uint64(0), ctypes.c_uint64(0)
        arr = lambda *xs: (ctypes.c_uint64 * len(xs))(*[int(getattr(x, "handle", x)) for x in xs])   # noqa: E731
        idx = (ctypes.c_uint32 * 2)(0, 1)
        tailb = b"".join(tb)
        for sel_n, sel_h, sel_i in ((1, arr(Q[0]), None), (1, None, idx), (17, arr(*[Q[0]] * 17), idx)):
            assert lib.kzg_rows_commit_multiplicities_sel(eng._h, 1, arr(F[0]), 1, arr(Tb[0]), sel_n, sel_h, sel_i, L, w, u, tailb,
                                                          c, ctypes.byref(miss), ctypes.byref(h)) == E_ARG
            assert lib.kzg_rows_commit_lookup_sum_sel(eng._h, 1, arr(F[0]), 1, arr(Tb[0]), M[0].handle, sel_n, sel_h, sel_i, L, w,
                                                      be(3), be(4), u, tailb, c, cl, ctypes.byref(h)) == E_ARG
        good()
    finally:
        long_set.release()
        release(F + Tb + Q + M)
    assert eng.rows_stats() == before


def test_a_selector_of_another_worker(hip):
    """one context, workers 0 and 1 of a 2^5-point SRS (T = 16): a selector set of the other worker is refused"""
    eng = hip()
    eng.gen_srs(SEED_X, SEED_Y, 5, 1, [0, 1])
    T, L, w = 16, 1, 1
    inputs, table, sels = ls.sel_instance(L, w, T, 950)
    F, Tb, Q = (commit_sets(eng, x, (1,)) for x in (inputs, table, sels))
    Q1 = commit_sets(eng, sels, (1,), i=1)
    try:
        arg_error(lambda: eng.commit_multiplicities_sel(F, Tb, Q1, [0], L, w), "one worker")
        mset, miss = eng.commit_multiplicities_sel(F, Tb, Q, [0], L, w)
        arg_error(lambda: eng.commit_lookup_sum_sel(F, Tb, mset, Q1, [0], L, w, be(3), be(4)), "one worker")
        sset, cl = eng.commit_lookup_sum_sel(F, Tb, mset, Q, [0], L, w, be(3), be(4))
        release([mset, sset])
        assert (miss, cl) == (0, be(0))
    finally:
        release(F + Tb + Q + Q1)
    assert eng.rows_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------------- threads, multi, structure
def test_four_threads_run_different_sel_calls(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    u = T - 5
    before = eng.rows_stats()
    L, w = 2, 1
    inputs, table, sels = ls.sel_instance(L, w, T, 1100, u)
    tl = tail_of(T, u, 11)
    com = lambda row: oc.commit(srs, row_bytes(row), True)   # noqa: E731
    mz, _ = ls.multiplicities_sel(inputs, table, sels, L, w, u, tl)
    Sz, cz = ls.lookup_sum_sel(inputs, table, mz, sels, L, w, 13, 14, u, tl)
    mp, missp = ls.multiplicities_sel(inputs, table, sels, L, w)
    mult = rand_rows(1, T, 1150)[0]
    Sp, cp = ls.lookup_sum_sel(inputs, table, mult, [sels[0], None], L, w, 15, 16)
    F, Tb, Q = commit_sets(eng, inputs, (2,)), commit_sets(eng, table, (1,)), commit_sets(eng, sels, (2,))
    Mz, Mp = commit_sets(eng, [mz], (1,)), commit_sets(eng, [mult], (1,))
    jobs = [(lambda: eng.commit_multiplicities_sel(F, Tb, Q, [0, 1], L, w, u, bt(tl)), ([com(mz)], 0)),
            (lambda: eng.commit_lookup_sum_sel(F, Tb, Mz[0], Q, [0, 1], L, w, be(13), be(14), u, bt(tl)), ([com(Sz)], be(cz))),
            (lambda: eng.commit_multiplicities_sel(F, Tb, Q, [0, 1], L, w), ([com(mp)], missp)),
            (lambda: eng.commit_lookup_sum_sel(F, Tb, Mp[0], Q, [0, None], L, w, be(15), be(16)), ([com(Sp)], be(cp)))]
    errors = []

    def work(j):
        try:
            for _ in range(3):
                rset, extra = jobs[j][0]()
                rset.release()
                assert (rset.commitments, extra) == jobs[j][1], j
        except Exception as ex:   # noqa: BLE001
            errors.append(repr(ex))

    ths = [threading.Thread(target=work, args=(j,)) for j in range(4)]
    for x in ths:
        x.start()
    for x in ths:
        x.join()
    release(F + Tb + Q + Mz + Mp)
    assert not errors, errors
    assert cz == 0
    assert eng.rows_stats() == before


def test_multi_handle_returns_the_context_bytes(hip):
    lib = _native.load()
    scale, ms, G = 7, 1, 2
    T, M = 1 << (scale - ms), 1 << ms
    u, L, w = T - 5, 2, 1
    tx, ty = 0x5E1ABCD, 0x5E11357
    devs = (ctypes.c_int * G)(0, 0)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(G, devs, ctypes.byref(mh)) == 0
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        i = 1
        srs = oc.srs_gen(be(tx), be(ty), scale, ms, i)
        inputs, table, sels = ls.sel_instance(L, w, T, 1300, u)
        tail = tail_of(T, u, 13)
        m, missing = ls.multiplicities_sel(inputs, table, sels, L, w, u, tail)
        S, closing = ls.lookup_sum_sel(inputs, table, m, sels, L, w, 21, 22, u, tail)
        cc, c, cl = ctypes.create_string_buffer(48 * 16), ctypes.create_string_buffer(48), ctypes.create_string_buffer(32)
        hh = [ctypes.c_uint64(0) for _ in range(6)]
        commit = lambda rows, h, wi=i: lib.kzg_multi_rows_commit(mh, wi, len(rows), b"".join(row_bytes(r) for r in rows), T, 1, cc,  # noqa: E731
                                                                 ctypes.byref(h))
        assert commit(inputs, hh[0]) == 0 and commit(table, hh[1]) == 0 and commit(sels, hh[2]) == 0
        assert commit(sels, hh[3], 0) == 0   # the same selectors under the other worker
        arr = lambda *hs: (ctypes.c_uint64 * len(hs))(*[x.value for x in hs])   # noqa: E731
        idx, tb = (ctypes.c_uint32 * 2)(0, 1), b"".join(bt(tail))
        miss = ctypes.c_uint64(9)
        assert lib.kzg_multi_rows_commit_multiplicities_sel(mh, i, 1, arr(hh[0]), 1, arr(hh[1]), 1, arr(hh[2]), idx, L, w, u, tb, c,
                                                            ctypes.byref(miss), ctypes.byref(hh[4])) == 0
        assert (miss.value, c.raw) == (0, oc.commit(srs, row_bytes(m), True))
        assert lib.kzg_multi_rows_commit_lookup_sum_sel(mh, i, 1, arr(hh[0]), 1, arr(hh[1]), hh[4].value, 1, arr(hh[2]), idx, L, w,
                                                        be(21), be(22), u, tb, c, cl, ctypes.byref(hh[5])) == 0
        assert (c.raw, cl.raw) == (oc.commit(srs, row_bytes(S), True), be(closing)) and closing == 0
        # the other worker's selector set, and the other worker's index, are refused
        h = ctypes.c_uint64(0)
        assert lib.kzg_multi_rows_commit_multiplicities_sel(mh, i, 1, arr(hh[0]), 1, arr(hh[1]), 1, arr(hh[3]), idx, L, w, u, tb, c,
                                                            ctypes.byref(miss), ctypes.byref(h)) == E_ARG
        assert lib.kzg_multi_rows_commit_lookup_sum_sel(mh, 0, 1, arr(hh[0]), 1, arr(hh[1]), hh[4].value, 1, arr(hh[2]), idx, L, w,
                                                        be(21), be(22), u, tb, c, cl, ctypes.byref(h)) == E_ARG
        for k, x in enumerate(hh):
            assert lib.kzg_multi_rows_release(mh, 0 if k == 3 else i, x.value) == 0
    finally:
        lib.kzg_multi_destroy(mh)


def test_no_row_sized_copy_inside_the_calls(engines):
    """structural: with stage profiling on, no _sel call opens an upload span (only upload_fr opens KZG_T_DECODE), while the
    transforms, the builders' kernels and the MSM's accumulate all ran; the results are those of the unprofiled calls"""
    lg = 10
    eng, T = engines(lg), 1 << lg
    u = T - 5
    before = eng.rows_stats()
    L, w = 2, 1
    inputs, table, sels = ls.sel_instance(L, w, T, 1400, u)
    tl = bt(tail_of(T, u, 14))
    F, Tb, Q = commit_sets(eng, inputs, (2,)), commit_sets(eng, table, (1,)), commit_sets(eng, sels, (2,))
    M = commit_sets(eng, rand_rows(1, T, 1450), (1,))
    calls = {"multiplicities": lambda: eng.commit_multiplicities_sel(F, Tb, Q, [0, 1], L, w, u, tl)[0],
             "lookup sum": lambda: eng.commit_lookup_sum_sel(F, Tb, M[0], Q, [1, 0], L, w, be(13), be(14), u, tl)[0]}
    lib = _native.load()
    try:
        for name, call in calls.items():
            plain = call()
            plain.release()
            assert lib.kzg_set_profiling(eng._h, 1) == 0
            try:
                rs = call()
                rs.release()
                tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
                assert lib.kzg_get_timings(eng._h, tms, len(tms)) == 0
            finally:
                assert lib.kzg_set_profiling(eng._h, 0) == 0
            t = dict(zip(_native.TIMING_NAMES, tms))
            print(name, "_sel stage times (ms):", {k: round(v, 4) for k, v in t.items()})
            assert t["decode"] == 0, name
            assert t["ntt"] > 0 and t["poly"] > 0 and t["accumulate"] > 0, name
            assert rs.commitments == plain.commitments, name
    finally:
        release(F + Tb + Q + M)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- through the Client
def test_the_lookup_rounds_through_the_client():
    """commit the wires and the fixed rows (selectors and table in ONE fixed set), build m, derive theta and beta by hashing
    the commitments, build S: it closes, and both rows are the reference's"""
    from zkp_subnet_amd.client import Client

    lg, u, seed, L, w = 6, 58, 2025, 2, 2
    T = 1 << lg
    cl = Client(seed=seed)
    cl.start(lg, 0)
    fr = lambda v: codec.be32_to_fr(be(v))   # noqa: E731
    unfr = lambda s: val(codec.fr_to_be32(s))   # noqa: E731
    poly = lambda row: [fr(v) for v in row]   # noqa: E731

    def ok(r):
        assert r.status_code == 200, r.json()
        return r.json()

    def challenge(tag, *parts):
        return int.from_bytes(hashlib.sha256(tag + b"".join(p.encode() for p in parts)).digest(), "big") % R

    try:
        assert cl.engine.rows_stats() == (0, 0)
        inputs, table, sels = ls.sel_instance(L, w, T, 1500, u)
        tails = {k: tail_of(T, u, 150 + j) for j, k in enumerate("mS")}
        wires = ok(cl.worker_commit_rows(0, [poly(r) for r in inputs]))
        fixed = ok(cl.worker_commit_rows(0, [poly(r) for r in table + sels]))       # rows: t_0 t_1 q_0 q_1
        tab = ok(cl.worker_commit_rows(0, [poly(r) for r in table]))
        m = ok(cl.worker_commit_multiplicities_sel([wires["handle"]], [tab["handle"]], [fixed["handle"]], [2, 3], L, w, u,
                                                   [fr(v) for v in tails["m"]]))
        theta = challenge(b"theta", *wires["commitments"], *fixed["commitments"], m["commitment"])
        beta = challenge(b"beta", *wires["commitments"], *fixed["commitments"], m["commitment"])
        s = ok(cl.worker_commit_lookup_sum_sel([wires["handle"]], [tab["handle"]], m["handle"], [fixed["handle"]], [2, 3], L, w,
                                               fr(theta), fr(beta), u, [fr(v) for v in tails["S"]]))
        assert (m["missing"], unfr(s["closing"])) == (0, 0)
        want_m, _ = ls.multiplicities_sel(inputs, table, sels, L, w, u, tails["m"])
        want_S, _ = ls.lookup_sum_sel(inputs, table, want_m, sels, L, w, theta, beta, u, tails["S"])
        wT = gp.omega(T)
        pts = [fr(pow(wT, t, R)) for t in (0, u - 1, u, T - 1)]
        ev = ok(cl.worker_eval_rows([m["handle"], s["handle"]], pts, [[0, 1]] * 4))["evals"]
        assert [[unfr(y) for y in e] for e in ev] == [[want_m[t], want_S[t]] for t in (0, u - 1, u, T - 1)]
        # without the selectors the same rows miss their disabled cells; a bad request is a 400 and the client keeps serving
        m0 = ok(cl.worker_commit_multiplicities_sel([wires["handle"]], [tab["handle"]], [], [None, None], L, w, u,
                                                    [fr(v) for v in tails["m"]]))
        assert m0["missing"] == sum(q[:u].count(0) for q in sels)
        bad = cl.worker_commit_multiplicities_sel([wires["handle"]], [tab["handle"]], [fixed["handle"]], [2, 4], L, w, u,
                                                  [fr(v) for v in tails["m"]])
        assert bad.status_code == 400 and "sel_index" in bad.json()["error"]
        bad = cl.worker_commit_lookup_sum_sel([wires["handle"]], [tab["handle"]], m["handle"], [], [2, None], L, w, fr(theta),
                                              fr(beta))
        assert bad.status_code == 400
        # the plain layout through the same methods
        mp = ok(cl.worker_commit_multiplicities_sel([wires["handle"]], [tab["handle"]], [fixed["handle"]], [2, 3], L, w))
        sp = ok(cl.worker_commit_lookup_sum_sel([wires["handle"]], [tab["handle"]], mp["handle"], [fixed["handle"]], [2, 3], L, w,
                                                fr(theta), fr(beta)))
        for r in (wires, fixed, tab, m, s, m0, mp, sp):
            ok(cl.worker_release_rows(r["handle"]))
        assert cl.engine.rows_stats() == (0, 0)
    finally:
        cl.stop()


# ---------------------------------------------------------------------------------------------------- the quotient
from tests import blinding_ref as br   # noqa: E402
from tests import quotient_ref as qr   # noqa: E402

QSHAPES = [(1, 1, 1, 2, False), (3, 2, 2, 4, False), (2, 2, 2, 4, True)]   # L, w, ext_log, P, with an active column
qshape_id = lambda s: f"L{s[0]}w{s[1]}e{s[2]}P{s[3]}{'A' if s[4] else ''}"   # noqa: E731


def q_args(inst):
    """the engine's forms of a QuotInstance's terms and lookup part"""
    lookup = dict(inst.lookup, theta=be(inst.theta), beta=be(inst.beta), alpha=be(inst.alpha))
    return [(be(c), fs) for c, fs in inst.terms], lookup


def want_pieces(srs, inst, sels, ext_log, P):
    t, rem = ls.quotient_sel(inst.coeff_rows(), inst.terms, None, inst.lookup, sels, inst.active, ext_log)
    assert not any(rem)
    return [oc.commit(srs, row_bytes(p), False) for p in qr.pieces(t, inst.T, P)]


@pytest.mark.parametrize("shape", QSHAPES, ids=qshape_id)
@pytest.mark.parametrize("lg", [4, 8])
def test_quotient_sel_bit_exact(engines, srs_of, lg, shape):
    """the pieces of a satisfied instance against the reference; sentinels and an all-ones row are _quotient_zk's bytes; two
    parts plus finish are the single call; without the selectors, and with one broken enabled cell, no set is created"""
    L, w, ext_log, P, act = shape
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    inst = ls.QuotInstance(L, w, T, 40 + lg + L, T - 5 if act else None)
    assert (inst.missing, inst.closing) == (0, 0)
    terms, lookup = q_args(inst)
    n = len(inst.rows)
    sets = commit_sets(eng, inst.rows + [[1] * T], (n - 2, 3))   # (the last row: all ones)
    try:
        want = want_pieces(srs, inst, inst.sel_rows, ext_log, P)
        rs = eng.commit_quotient_sel(sets, terms, None, lookup, inst.sel_rows, inst.active, ext_log, P)
        rs.release()
        assert rs.commitments == want
        # the same rows without the selectors (sentinels, or the all-ones row n): the relation does not hold, no set is created
        # (asked for P - 1 < E pieces: with P = E pieces there is no coefficient above them to find nonzero)
        for sel in ([None] * L, [n] * L):
            with pytest.raises(KzgError) as ei:
                eng.commit_quotient_sel(sets, terms, None, lookup, sel, inst.active, ext_log, P - 1)
            assert ei.value.code == E_ARG and "do not hold" in str(ei.value)
            with pytest.raises(KzgError):
                eng.commit_quotient_zk(sets, terms, None, lookup, inst.active, ext_log, P - 1)
        # two parts (the whole relation twice, each with the scale 1 / 2) plus finish = the single call
        half = be(pow(2, -1, R))
        acc = eng.quotient_part_sel(sets, terms, None, lookup, inst.sel_rows, inst.active, None, ext_log, half)
        acc = eng.quotient_part_sel(sets, terms, None, lookup, inst.sel_rows, inst.active, None, ext_log, half, acc)
        fin = eng.quotient_finish(acc, P)
        fin.release()
        assert fin.commitments == want
    finally:
        release(sets)
    # one broken enabled cell: with P - 1 < E pieces the nonzero coefficients above them are found, no set is created
    bad = ls.QuotInstance(L, w, T, 40 + lg + L, T - 5 if act else None, broken=True)
    sets = commit_sets(eng, bad.rows, (n,))
    try:
        terms, lookup = q_args(bad)
        with pytest.raises(KzgError) as ei:
            eng.commit_quotient_sel(sets, terms, None, lookup, bad.sel_rows, bad.active, ext_log, max(P - 1, 1))
        assert ei.value.code == E_ARG and "do not hold" in str(ei.value)
    finally:
        release(sets)
    assert eng.rows_stats() == before


@pytest.mark.parametrize("act", [False, True], ids=["plain", "active"])
def test_quotient_sel_identities(engines, act):
    """on rows that satisfy the lookup WITHOUT selectors: selectors None, all sentinels and an all-ones row give the bytes of
    _quotient_zk, and a part with them the bytes of _quotient_part + finish"""
    lg, L, w, ext_log, P = 8, 2, 2, 2, 4
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    u = T - 5 if act else None
    inst = ls.QuotInstance(L, w, T, 77, u)
    ones = [1] * T
    rnd = random.Random(5)
    n_in = L * w
    have_n = T if u is None else u
    for l in range(L):   # every cell that counts now holds a table tuple, and the selector rows become all ones
        for t in range(T):
            src = rnd.randrange(have_n)
            for c in range(w):
                inst.rows[l * w + c][t] = inst.rows[n_in + c][src]
        inst.rows[inst.sel_rows[l]] = ones
    tail = lambda k: [] if u is None else tail_of(T, u, k)   # noqa: E731
    m, missing = ls.multiplicities_sel(inst.rows[:n_in], inst.rows[n_in:n_in + w], [None] * L, L, w, u, tail(1))
    S, closing = ls.lookup_sum_sel(inst.rows[:n_in], inst.rows[n_in:n_in + w], m, [None] * L, L, w, inst.theta, inst.beta, u, tail(2))
    assert (missing, closing) == (0, 0)
    inst.rows[inst.m_row], inst.rows[inst.s_row] = m, S
    terms, lookup = q_args(inst)
    sets = commit_sets(eng, inst.rows, (len(inst.rows),))
    try:
        base = eng.commit_quotient_zk(sets, terms, None, lookup, inst.active, ext_log, P)
        base.release()
        acc = eng.quotient_part(sets, terms, None, lookup, inst.active, None, ext_log, be(7))
        pbase = eng.quotient_finish(acc, P)
        pbase.release()
        for sel in (None, [None] * L, inst.sel_rows, [inst.sel_rows[0], None]):
            rs = eng.commit_quotient_sel(sets, terms, None, lookup, sel, inst.active, ext_log, P)
            rs.release()
            assert rs.commitments == base.commitments, sel
            acc = eng.quotient_part_sel(sets, terms, None, lookup, sel, inst.active, None, ext_log, be(7))
            fin = eng.quotient_finish(acc, P)
            fin.release()
            assert fin.commitments == pbase.commitments, sel
    finally:
        release(sets)
    assert eng.rows_stats() == before


def test_quotient_sel_errors_leave_the_context_serving(engines, srs_of):
    lg, L, w, ext_log, P = 4, 1, 1, 1, 2
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    lib = _native.load()
    inst = ls.QuotInstance(L, w, T, 88)
    terms, lookup = q_args(inst)
    n = len(inst.rows)
    sets = commit_sets(eng, inst.rows, (n,))
    want = want_pieces(srs, inst, inst.sel_rows, ext_log, P)

    def good():
        rs = eng.commit_quotient_sel(sets, terms, None, lookup, inst.sel_rows, None, ext_log, P)
        rs.release()
        assert rs.commitments == want

    try:
        good()
        arg_error(lambda: eng.commit_quotient_sel(sets, terms, None, lookup, [n], None, ext_log, P), "row index")
        arg_error(lambda: eng.quotient_part_sel(sets, terms, None, lookup, [n + 3], None, None, ext_log), "row index")
        good()
        # the C entry points: selectors without a lookup part, and a null selector_rows
        _, hs, gate, _, lk, _ = eng._quotient_args("t", sets, [(be(1), [0])], None, lookup, None, ext_log, P)
        arr = (ctypes.c_uint32 * 1)(inst.sel_rows[0])
        sel, nul = _native.QuotientSelectors(arr), _native.QuotientSelectors(None)
        c, h = ctypes.create_string_buffer(48 * P), ctypes.c_uint64(0)
        assert lib.kzg_rows_commit_quotient_sel(eng._h, 1, hs, ctypes.byref(gate), None, None, ctypes.byref(sel), None, ext_log, P,
                                                c, ctypes.byref(h)) == E_ARG
        assert lib.kzg_rows_commit_quotient_sel(eng._h, 1, hs, ctypes.byref(gate), None, ctypes.byref(lk), ctypes.byref(nul), None,
                                                ext_log, P, c, ctypes.byref(h)) == E_ARG
        assert lib.kzg_rows_quotient_part_sel(eng._h, 1, hs, ctypes.byref(gate), None, None, None, ctypes.byref(sel), None, ext_log,
                                              None, ctypes.byref(h)) == E_ARG
        assert h.value == 0
        good()
    finally:
        release(sets)
    assert eng.rows_stats() == before


def test_the_whole_round_through_the_client():
    """wires and fixed rows -> m -> theta, beta -> S -> alpha -> the quotient with the S L_u closing term -> zeta -> the
    evaluations at zeta and zeta w -> num(zeta) = t(zeta) Z_H(zeta) from them alone -> the linearised opening, verified"""
    from zkp_subnet_amd.client import Client

    lg, L, w, ext_log, P = 6, 2, 2, 2, 4
    T = 1 << lg
    u = T - 6
    cl = Client(seed=2026)
    cl.start(lg, 0)
    fr = lambda v: codec.be32_to_fr(be(v))   # noqa: E731
    unfr = lambda s: val(codec.fr_to_be32(s))   # noqa: E731
    poly = lambda row: [fr(v) for v in row]   # noqa: E731

    def ok(r):
        assert r.status_code == 200, r.json()
        return r.json()

    def challenge(tag, *parts):
        return int.from_bytes(hashlib.sha256(tag + b"".join(p.encode() for p in parts)).digest(), "big") % R

    try:
        inputs, table, sels = ls.sel_instance(L, w, T, 1600, u)
        n_in = L * w
        tm, ts = tail_of(T, u, 161), tail_of(T, u, 162)
        wires = ok(cl.worker_commit_rows(0, [poly(r) for r in inputs]))
        fixed = ok(cl.worker_commit_rows(0, [poly(r) for r in table + sels + [br.active_row(T, u), br.last_row(T, u)]]))
        hw, hf = wires["handle"], fixed["handle"]
        tab = ok(cl.worker_commit_rows(0, [poly(r) for r in table]))["handle"]
        m = ok(cl.worker_commit_multiplicities_sel([hw], [tab], [hf], [w, w + 1], L, w, u, [fr(v) for v in tm]))
        seen = wires["commitments"] + fixed["commitments"] + [m["commitment"]]
        theta, beta = challenge(b"theta", *seen), challenge(b"beta", *seen)
        s = ok(cl.worker_commit_lookup_sum_sel([hw], [tab], m["handle"], [hf], [w, w + 1], L, w, fr(theta), fr(beta), u,
                                               [fr(v) for v in ts]))
        assert (m["missing"], unfr(s["closing"])) == (0, 0)
        alpha = challenge(b"alpha", *seen, s["commitment"])
        # rows of [wires, fixed, m, S]: inputs | table | q_0 q_1 | A | L_u | m | S
        sel_rows, act, lu, mrow, srow = [n_in + w, n_in + w + 1], n_in + w + L, n_in + w + L + 1, n_in + w + L + 2, n_in + w + L + 3
        hs = [hw, hf, m["handle"], s["handle"]]
        iterms = [(pow(alpha, 5, R), [srow, lu])]
        ilookup = {"inputs": list(range(n_in)), "table": list(range(n_in, n_in + w)), "mult": mrow, "sum": srow, "width": w,
                   "theta": theta, "beta": beta, "alpha": alpha}
        lookup = dict(ilookup, theta=fr(theta), beta=fr(beta), alpha=fr(alpha))
        q = ok(cl.worker_commit_quotient_sel(hs, [[fr(c), fs] for c, fs in iterms], None, lookup, sel_rows, act, ext_log, P))
        zeta = challenge(b"zeta", *seen, s["commitment"], *q["commitments"])
        wT = gp.omega(T)
        nrows = srow + 1
        ev = ok(cl.worker_eval_rows(hs, [fr(zeta), fr(zeta * wT % R)], [list(range(nrows))] * 2))["evals"]
        at = {(j, rot): unfr(ev[rot][j]) for j in range(nrows) for rot in (0, 1)}
        num = ls.num_at_sel(lambda j, rot: at[(j, rot)], iterms, None, ilookup, sel_rows, act, zeta, T)
        tp = [unfr(y) for y in ok(cl.worker_eval_rows([q["handle"]], [fr(zeta)], [list(range(P))]))["evals"][0]]
        assert num == sum(pow(zeta, p * T, R) * y for p, y in enumerate(tp)) % R * (pow(zeta, T, R) - 1) % R
        # the quotient without the selectors does not exist for these rows
        assert cl.worker_commit_quotient_sel(hs, [[fr(c), fs] for c, fs in iterms], None, lookup, None, act, ext_log,
                                             P - 1).status_code == 400
        # the pieces open through their combination sum_p zeta^(pT) t_p, and the opening verifies
        coeffs = [[fr(pow(zeta, p * T, R)) for p in range(P)]]
        op = ok(cl.worker_open_rows_lincomb([q["handle"]], [fr(zeta)], coeffs))
        vr = ok(cl.worker_verify_open_lincomb(0, op["proofs"], [fr(zeta)], coeffs, op["values"], q["commitments"]))
        assert vr["valid"] is True
        assert unfr(op["values"][0]) == sum(pow(zeta, p * T, R) * y for p, y in enumerate(tp)) % R
        for h in hs + [tab, q["handle"]]:
            ok(cl.worker_release_rows(h))
        assert cl.engine.rows_stats() == (0, 0)
    finally:
        cl.stop()


# ---------------------------------------------------------------------------------------------------- the quotient: more cases
def field_selector_instance(T, u, seed):
    """L = 2, w = 2 with an active column: lookup 0's selector holds 0, 1, r - 1 and random field elements, lookup 1 has a 0/1
    one.  S is the weighted running sum over whatever m the join gives, so A LK1 holds on every row without the sum closing
    (the closing term S L_u is left out: terms = [])"""
    inst = ls.QuotInstance(2, 2, T, seed, u)
    rnd = random.Random(seed)
    q = [0, 1, R - 1, 0] + [rnd.randrange(R) for _ in range(T - 4)]
    inst.rows[inst.sel_rows[0]] = q
    sels = [q, inst.rows[inst.sel_rows[1]]]
    inst.S, inst.closing = ls.lookup_sum_sel(inst.rows[:4], inst.rows[4:6], inst.m, sels, 2, 2, inst.theta, inst.beta, u,
                                             tail_of(T, u, seed + 1))
    inst.rows[inst.s_row] = inst.S
    inst.terms = []
    return inst


@pytest.mark.parametrize("lg", [4, 8])
def test_quotient_sel_with_a_selector_of_field_elements(engines, srs_of, lg):
    """the pieces are bit-exact for a selector of arbitrary field elements: the single call, and two parts with scales 1 / 3
    and 2 / 3 plus finish, at P = E"""
    ext_log, P = 2, 4
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    inst = field_selector_instance(T, T - 5, 60 + lg)
    assert inst.closing != 0
    terms, lookup = q_args(inst)
    want = want_pieces(srs, inst, inst.sel_rows, ext_log, P)
    sets = commit_sets(eng, inst.rows, (len(inst.rows),))
    try:
        rs = eng.commit_quotient_sel(sets, terms, None, lookup, inst.sel_rows, inst.active, ext_log, P)
        rs.release()
        assert rs.commitments == want
        third = pow(3, -1, R)
        acc = eng.quotient_part_sel(sets, terms, None, lookup, inst.sel_rows, inst.active, None, ext_log, be(third))
        acc = eng.quotient_part_sel(sets, terms, None, lookup, inst.sel_rows, inst.active, None, ext_log, be(2 * third % R), acc)
        fin = eng.quotient_finish(acc, P)
        fin.release()
        assert fin.commitments == want
    finally:
        release(sets)
    assert eng.rows_stats() == before


def test_quotient_sel_threads_and_no_row_sized_copy(engines, srs_of):
    """four threads run the single call and the part + finish, with and without an active column, three times each; then, with
    stage profiling on, neither call opens an upload span while the transforms, the pointwise kernel and the MSM all ran"""
    lg, ext_log, P = 8, 2, 4
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    insts = [ls.QuotInstance(2, 2, T, 71, None), ls.QuotInstance(2, 2, T, 72, T - 5)]
    sets = [commit_sets(eng, x.rows, (len(x.rows),)) for x in insts]
    args = [q_args(x) for x in insts]
    wants = [want_pieces(srs, x, x.sel_rows, ext_log, P) for x in insts]

    def single(k):
        rs = eng.commit_quotient_sel(sets[k], args[k][0], None, args[k][1], insts[k].sel_rows, insts[k].active, ext_log, P)
        rs.release()
        return rs

    def parts(k):
        acc = eng.quotient_part_sel(sets[k], args[k][0], None, args[k][1], insts[k].sel_rows, insts[k].active, None, ext_log)
        rs = eng.quotient_finish(acc, P)
        rs.release()
        return rs

    jobs = [(single, 0), (single, 1), (parts, 0), (parts, 1)]
    errors = []

    def work(j):
        try:
            for _ in range(3):
                assert jobs[j][0](jobs[j][1]).commitments == wants[jobs[j][1]], j
        except Exception as ex:   # noqa: BLE001
            errors.append(repr(ex))

    ths = [threading.Thread(target=work, args=(j,)) for j in range(4)]
    for x in ths:
        x.start()
    for x in ths:
        x.join()
    lib = _native.load()
    try:
        assert not errors, errors
        for name, call in (("quotient_sel", lambda: single(1)),
                           ("quotient_part_sel", lambda: eng.quotient_part_sel(sets[1], args[1][0], None, args[1][1],
                                                                               insts[1].sel_rows, insts[1].active, None, ext_log))):
            assert lib.kzg_set_profiling(eng._h, 1) == 0
            try:
                out = call()
                tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
                assert lib.kzg_get_timings(eng._h, tms, len(tms)) == 0
            finally:
                assert lib.kzg_set_profiling(eng._h, 0) == 0
            t = dict(zip(_native.TIMING_NAMES, tms))
            print(name, "stage times (ms):", {k: round(v, 4) for k, v in t.items()})
            assert t["decode"] == 0 and t["ntt"] > 0 and t["poly"] > 0, name
            if name == "quotient_sel":
                assert t["accumulate"] > 0 and out.commitments == wants[1]
            else:
                fin = eng.quotient_finish(out, P)
                fin.release()
                assert fin.commitments == wants[1]
    finally:
        release(sets[0] + sets[1])
    assert eng.rows_stats() == before


def test_multi_handle_and_multi_client_quotient_sel():
    """kzg_multi_rows_commit_quotient_sel / kzg_multi_rows_quotient_part_sel return the reference's bytes and refuse the other
    worker's index; MultiDeviceClient routes worker_commit_quotient_sel / worker_quotient_part_sel by the sets' worker"""
    from tests.test_gpu_quotient_ext import b_lookup, b_terms, c_args
    from zkp_subnet_amd.client import derive_taus
    from zkp_subnet_amd.multi import MultiDeviceClient

    lib = _native.load()
    scale, ms, G, ext_log, P = 7, 1, 2, 2, 4
    T, M = 1 << (scale - ms), 1 << ms
    inst = ls.QuotInstance(2, 2, T, 81, T - 5)
    n = len(inst.rows)
    t, rem = ls.quotient_sel(inst.coeff_rows(), inst.terms, None, inst.lookup, inst.sel_rows, inst.active, ext_log)
    assert not any(rem)
    pieces = [row_bytes(p) for p in qr.pieces(t, T, P)]
    tx, ty = 0x5E1ABCE, 0x5E11358
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(G, (ctypes.c_int * G)(0, 0), ctypes.byref(mh)) == 0
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        i = 1
        srs = oc.srs_gen(be(tx), be(ty), scale, ms, i)
        want = b"".join(oc.commit(srs, p, False) for p in pieces)
        cc, c = ctypes.create_string_buffer(48 * 16), ctypes.create_string_buffer(48 * P)
        hs, hq, acc = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        assert lib.kzg_multi_rows_commit(mh, i, n, b"".join(row_bytes(r) for r in inst.rows), T, 1, cc, ctypes.byref(hs)) == 0
        gate, _, lk, _keep = c_args(b_terms(inst.terms), None, b_lookup(inst.lookup))
        arr = (ctypes.c_uint32 * 2)(*inst.sel_rows)
        sel, act = _native.QuotientSelectors(arr), _native.QuotientActive(inst.active)
        one = (ctypes.c_uint64 * 1)(hs.value)
        assert lib.kzg_multi_rows_commit_quotient_sel(mh, i, 1, one, gate, None, lk, ctypes.byref(sel), ctypes.byref(act), ext_log, P,
                                                      c, ctypes.byref(hq)) == 0
        assert c.raw == want
        assert lib.kzg_multi_rows_quotient_part_sel(mh, i, 1, one, gate, None, None, lk, ctypes.byref(sel), ctypes.byref(act),
                                                    ext_log, None, ctypes.byref(acc)) == 0
        hf = ctypes.c_uint64(0)
        assert lib.kzg_multi_rows_quotient_finish(mh, i, acc.value, P, c, ctypes.byref(hf)) == 0
        assert c.raw == want
        h2 = ctypes.c_uint64(0)
        assert lib.kzg_multi_rows_commit_quotient_sel(mh, 0, 1, one, gate, None, lk, ctypes.byref(sel), ctypes.byref(act), ext_log, P,
                                                      c, ctypes.byref(h2)) == E_ARG
        acc2 = ctypes.c_uint64(0)
        assert lib.kzg_multi_rows_quotient_part_sel(mh, 0, 1, one, gate, None, None, lk, ctypes.byref(sel), ctypes.byref(act),
                                                    ext_log, None, ctypes.byref(acc2)) == E_ARG
        for h in (hs, hq, hf):
            assert lib.kzg_multi_rows_release(mh, i, h.value) == 0
    finally:
        lib.kzg_multi_destroy(mh)

    fr = lambda v: codec.be32_to_fr(be(v))   # noqa: E731
    multi = MultiDeviceClient(devices=[0, 0], seed=83)
    multi.start(scale=scale, machines_scale=ms)
    try:
        txb, tyb = (x.to_bytes(32, "big") for x in derive_taus(83))
        terms = [[fr(cf), fs] for cf, fs in inst.terms]
        lookup = dict(inst.lookup, theta=fr(inst.theta), beta=fr(inst.beta), alpha=fr(inst.alpha))
        for i in range(M):
            srs = oc.srs_gen(txb, tyb, scale, ms, i)
            want = [oc.commit(srs, p, False) for p in pieces]
            r = multi.worker_commit_rows(i, [[fr(v) for v in row] for row in inst.rows])
            assert r.status_code == 200, r.json()
            h = r.json()["handle"]
            q = multi.worker_commit_quotient_sel([h], terms, None, lookup, inst.sel_rows, inst.active, ext_log, P)
            assert q.status_code == 200, q.json()
            assert [codec.g1_from_b64(x) for x in q.json()["commitments"]] == want
            a = multi.worker_quotient_part_sel([h], terms, None, lookup, inst.sel_rows, inst.active, None, ext_log)
            assert a.status_code == 200, a.json()
            f = multi.worker_quotient_finish(a.json()["acc"], P)
            assert f.status_code == 200 and [codec.g1_from_b64(x) for x in f.json()["commitments"]] == want
            for x in (h, q.json()["handle"], f.json()["handle"]):
                assert multi.worker_release_rows(x).status_code == 200
        assert multi.worker_commit_quotient_sel([12345], terms, None, lookup, inst.sel_rows, inst.active, ext_log, P).status_code == 400
    finally:
        multi.stop()
