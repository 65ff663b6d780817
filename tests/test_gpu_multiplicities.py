"""GPU tests (`-m gpu`) of kzg_rows_commit_multiplicities: the multiplicity row m of the lookup argument, joined on the device
from committed row sets.  The expected m and `missing` come from the definition in Python (tests/multiplicities_ref.py) and m
is committed with the C oracle, never with the library under test: commitment, `missing` and m's evaluations are compared
exactly.  Built instances with and without repeated table rows, keys chosen against a weak hash or a partial comparison,
misses, repeated handles, the hand-over to the lookup sum, determinism, every documented error, a racing release, the
multi-GPU handle and the stage times follow.  Each test leaves rows_stats() where it found it."""
import ctypes
import random
import threading

import numpy as np
import pytest

from oracle import cpu as oc
from tests import lookup_ref as lk
from tests.gpu_rows import (arg_error as rows_arg_error, check_one_row, commit_sets, engine_cache, probes_ends, rand_rows,
                            release, split_first as split, srs_cache)
from tests.multiplicities_ref import multiplicities
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import lagrange_factor

pytestmark = pytest.mark.gpu
R = lk.R
be, row_bytes = lk.be, lk.row_bytes
SEED_X, SEED_Y = 0x3017A1, 0x3017A2
SHAPES = [(1, 1), (3, 2), (16, 1), (1, 16), (2, 8)]


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def instance(L, w, T, seed, duplicates=False):
    """(inputs, table): a table of T random w-tuples (duplicates: its second half repeats rows of its first half) and L
    input tuples per row drawn from the table's rows -- the shape of lookup_ref.lookup_instance, fast at 2^16"""
    rng = np.random.default_rng(seed)
    table = rand_rows(w, T, 31 * seed)
    if duplicates and T > 1:
        src = rng.integers(0, T // 2, size=T - T // 2)
        for col in table:
            col[T // 2:] = [col[j] for j in src]
    inputs = []
    for l in range(L):
        pick = rng.integers(0, T, size=T)
        inputs += [[col[j] for j in pick] for col in table]
    return inputs, table


def check_against_reference(eng, srs, mset, missing, mult, want_missing, rnd, want_commitment=None):
    assert missing == want_missing
    check_one_row(eng, srs, mset, mult, rnd, probes=probes_ends(len(mult), rnd), want_commitment=want_commitment)


def run_both_forms(eng, srs, inputs, table, L, w, rnd, want=None):
    """the device call over the sources committed in evaluation form in one set each, then in coefficient form split over
    several sets, against the reference; `want`: what the case itself knows (mult, missing) must be"""
    T = len(table[0])
    before = eng.rows_stats()
    mult, missing = multiplicities(inputs, table, L, w)
    if want is not None:
        assert (mult, missing) == want
    assert sum(mult) + missing == L * T
    want_c = oc.commit(srs, row_bytes(mult), True)
    for ef, one_set in ((True, True), (False, False)):
        F = commit_sets(eng, inputs, (L * w,) if one_set else split(L * w), ef)
        Tb = commit_sets(eng, table, (w,) if one_set else split(w)[::-1], ef)
        try:
            mset, miss = eng.commit_multiplicities(F, Tb, L, w)
            try:
                assert eng.rows_stats()[0] == before[0] + len(F) + len(Tb) + 1
                assert (mset.i, mset.T) == (0, T)
                check_against_reference(eng, srs, mset, miss, mult, missing, rnd, want_c)
            finally:
                mset.release()
        finally:
            release(F + Tb)
    assert eng.rows_stats() == before
    return mult, missing


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"L{s[0]}w{s[1]}")
@pytest.mark.parametrize("lg", [4, 8, 10, 12, 16])
def test_built_instances(engines, srs_of, lg, shape):
    """every other (L + w + lg) the table repeats rows, and the hits of a repeated tuple must all land on its first copy"""
    L, w = shape
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    rnd = random.Random(100 * lg + 10 * L + w)
    inputs, table = instance(L, w, T, 7000 * lg + 10 * L + w, duplicates=(L + w + lg) % 2 == 1)
    _, missing = run_both_forms(eng, srs, inputs, table, L, w, rnd)
    assert missing == 0


def test_the_smallest_rows(hip):
    """every shape at the two smallest row lengths a row set accepts"""
    done = 0
    for lg in (0, 1, 2, 3, 4):
        eng = hip()
        T = 1 << lg
        try:
            eng.gen_srs(SEED_X + lg, SEED_Y, lg, 0)
            probe = eng.commit_rows(0, [row_bytes([1] * T)], True)
        except KzgError:
            continue   # the row sets themselves refuse this length
        probe.release()
        srs = oc.srs_gen(be(SEED_X + lg), be(SEED_Y), lg, 0, 0)
        rnd = random.Random(lg)
        for L, w in SHAPES:
            inputs, table = instance(L, w, T, 90 + lg + L, duplicates=w == 1)
            _, missing = run_both_forms(eng, srs, inputs, table, L, w, rnd)
            assert missing == 0
            _, missing = run_both_forms(eng, srs, rand_rows(L * w, T, 95 + lg), table, L, w, rnd)
            assert missing == L * T
        assert eng.rows_stats() == (0, 0)
        done += 1
        if done == 2:
            break
    assert done == 2


def test_reproduces_the_lookup_instance_builder(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    for L, w, dup in ((3, 2, False), (2, 3, True)):
        inputs, table, mult = lk.lookup_instance(L, w, T, 4100 + L, duplicates=dup)
        run_both_forms(eng, srs, inputs, table, L, w, random.Random(L), want=(mult, 0))


def test_row_indices_beyond_16_bits(engines):
    """2^17: the first length whose row indices do not fit 16 bits.  The expected commitment comes through the trapdoor
    (the oracle's [s0 m(tau)] G), which needs no 2^17-point SRS on the CPU"""
    lg, L, w = 17, 2, 1
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    inputs, table = instance(L, w, T, 1717)
    inputs[1][5], inputs[0][T - 1] = table[0][T - 1], table[0][0x10001]
    mult, missing = multiplicities(inputs, table, L, w)
    assert missing == 0 and mult[T - 1] >= 1 and mult[0x10001] >= 1
    F, Tb = commit_sets(eng, inputs, (2,)), commit_sets(eng, table, (1,))
    try:
        mset, miss = eng.commit_multiplicities(F, Tb, L, w)
        try:
            mc = oc.fr_ntt(row_bytes(mult), True)
            s0 = lagrange_factor(0, 0, SEED_Y)
            want = oc.g1_mul_gen(be(s0 * int.from_bytes(oc.fr_eval(mc, be(SEED_X + lg)), "big") % R))
            assert mset.commitments[0] == want and miss == 0
            wr = pow(7, (R - 1) // T, R)
            ts = [0, 1, T - 1, 0x10001]
            Y = eng.eval_rows([mset], [be(pow(wr, t, R)) for t in ts], [[0]] * 4)
            assert [int.from_bytes(y[0], "big") for y in Y] == [mult[t] for t in ts]
        finally:
            mset.release()
    finally:
        release(F + Tb)
    assert eng.rows_stats() == before


@pytest.mark.parametrize("lg", [8, 12])
def test_a_range_table(engines, srs_of, lg):
    """t_0 = 0 .. T - 1: keys that differ only in the lowest limb"""
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    rnd = random.Random(lg)
    table = [list(range(T))]
    inputs = [[rnd.randrange(T) for _ in range(T)] for _ in range(3)]
    inputs[0][0], inputs[1][1], inputs[2][T - 1] = 0, T - 1, T - 1                 # rows 0 and T - 1 are hit
    mult, missing = run_both_forms(eng, srs, inputs, table, 3, 1, rnd)
    assert missing == 0 and mult[0] >= 1 and mult[T - 1] >= 2
    inputs[1][7] = T                                                                # just outside the range
    _, missing = run_both_forms(eng, srs, inputs, table, 3, 1, rnd)
    assert missing == 1


def test_keys_that_differ_only_in_the_top_limb(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    rnd = random.Random(224)
    table = [[(j << 224) % R for j in range(T)]]
    assert len(set(table[0])) == T
    inputs = [[table[0][rnd.randrange(T)] for _ in range(T)] for _ in range(2)]
    inputs[0][3] = (5 << 224) + 1                                                   # differs from row 5 in the lowest bit
    _, missing = run_both_forms(eng, srs, inputs, table, 2, 1, rnd)
    assert missing == 1


def test_tuples_that_differ_only_in_the_last_column(engines, srs_of):
    lg, L, w = 10, 2, 3
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    rnd = random.Random(3)
    a, b = rnd.randrange(R), rnd.randrange(R)
    last = rand_rows(1, T, 333)[0]
    table = [[a] * T, [b] * T, last]
    picks = [[rnd.randrange(T) for _ in range(T)] for _ in range(L)]
    inputs = []
    for l in range(L):
        inputs += [[a] * T, [b] * T, [last[j] for j in picks[l]]]
    want = [0] * T
    for l in range(L):
        for j in picks[l]:
            want[j] += 1
    run_both_forms(eng, srs, inputs, table, L, w, rnd, want=(want, 0))
    inputs[5][9] = (last[picks[1][9]] + 1) % R                                      # equal in columns 0 and 1 only
    want[picks[1][9]] -= 1
    run_both_forms(eng, srs, inputs, table, L, w, rnd, want=(want, 1))


def test_a_swapped_pair_is_a_miss(engines, srs_of):
    lg, L, w = 8, 1, 2
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    rnd = random.Random(2)
    table = rand_rows(2, T, 222)
    inputs = [table[0][:], table[1][:]]                                             # cell t looks up row t ...
    inputs[0][17], inputs[1][17] = table[1][17], table[0][17]                       # ... but cell 17 holds (b, a)
    want = [1] * T
    want[17] = 0
    run_both_forms(eng, srs, inputs, table, L, w, rnd, want=(want, 1))


def test_zero_and_r_minus_one_and_the_all_zero_tuple(engines, srs_of):
    lg = 8
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    rnd = random.Random(9)
    table = rand_rows(1, T, 99)
    table[0][0], table[0][T - 1], table[0][5] = 0, R - 1, 1
    inputs = [[0] * T, [R - 1] * T, [table[0][t] for t in range(T)]]
    want = [1] * T
    want[0] += T
    want[T - 1] += T
    run_both_forms(eng, srs, inputs, table, 3, 1, rnd, want=(want, 0))
    # width 2: the all-zero tuple is a row like any other, (0, x) and (x, 0) are not it
    table = rand_rows(2, T, 98)
    table[0][T - 1] = table[1][T - 1] = 0
    x = table[0][3]
    inputs = [[0] * T, [0] * T]
    inputs[1][1], inputs[0][2] = x, x
    want = [0] * T
    want[T - 1] = T - 2
    run_both_forms(eng, srs, inputs, table, 1, 2, rnd, want=(want, 2))


def test_a_table_of_one_repeated_tuple_and_inputs_of_one_tuple(engines, srs_of):
    lg, L, w = 12, 3, 2
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    rnd = random.Random(12)
    a, b = rnd.randrange(R), rnd.randrange(R)
    # the whole table is one tuple T times: every build lane meets the same slot, row 0 wins
    table = [[a] * T, [b] * T]
    inputs = [[a] * T, [b] * T] * L
    run_both_forms(eng, srs, inputs, table, L, w, rnd, want=([L * T] + [0] * (T - 1), 0))
    # a random table, every input cell the same tuple (row T - 1): one counter takes L T additions
    table = rand_rows(2, T, 1212)
    inputs = [[table[0][T - 1]] * T, [table[1][T - 1]] * T] * L
    run_both_forms(eng, srs, inputs, table, L, w, rnd, want=([0] * (T - 1) + [L * T], 0))


def test_the_breaker_misses_once_and_random_inputs_miss_everywhere(engines, srs_of):
    lg, L, w = 10, 3, 2
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    rnd = random.Random(41)
    inputs, table, mult = lk.lookup_instance(L, w, T, 4141)
    broken = lk.break_instance(inputs, table, w, 4142)
    (l, t), = [(j // w, t) for j in range(0, L * w, w) for t in range(T) if any(broken[j + c][t] != inputs[j + c][t] for c in range(w))]
    first = {}
    for u in range(T):
        first.setdefault(tuple(col[u] for col in table), u)
    want = mult[:]
    want[first[tuple(inputs[l * w + c][t] for c in range(w))]] -= 1                 # the rest of m is unchanged
    run_both_forms(eng, srs, broken, table, L, w, rnd, want=(want, 1))
    # random inputs against a random table: nothing is found, m is the zero row
    mult, missing = run_both_forms(eng, srs, rand_rows(L * w, T, 4143), table, L, w, rnd, want=([0] * T, L * T))
    F, Tb = commit_sets(eng, rand_rows(L * w, T, 4143), (L * w,)), commit_sets(eng, table, (w,))
    try:
        mset, miss = eng.commit_multiplicities(F, Tb, L, w)
        mset.release()
        assert mset.commitments[0] == oc.commit(srs, row_bytes([0] * T), True) and miss == L * T
    finally:
        release(F + Tb)


def test_a_repeated_handle(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(43)
    f, two = rand_rows(1, T, 4300), rand_rows(2, T, 4310)
    A, B = commit_sets(eng, f, (1,)), commit_sets(eng, two, (2,))
    try:
        # one set as the input and as the table: every cell finds its own row
        mset, miss = eng.commit_multiplicities(A, A, 1, 1)
        try:
            check_against_reference(eng, srs, mset, miss, [1] * T, 0, rnd)
        finally:
            mset.release()
        # one two-row set four times as the inputs (L = 4, w = 2) and once as the table
        mult, missing = multiplicities(two * 4, two, 4, 2)
        assert (mult, missing) == ([4] * T, 0)
        mset, miss = eng.commit_multiplicities(B * 4, B, 4, 2)
        try:
            check_against_reference(eng, srs, mset, miss, mult, 0, rnd)
        finally:
            mset.release()
        # the one-row set twice as a width-2 table and as a width-2 input, and (L = 2, w = 1) against itself
        mset, miss = eng.commit_multiplicities(A * 2, A * 2, 1, 2)
        try:
            check_against_reference(eng, srs, mset, miss, [1] * T, 0, rnd)
        finally:
            mset.release()
        mset, miss = eng.commit_multiplicities(A * 2, A, 2, 1)
        try:
            check_against_reference(eng, srs, mset, miss, [2] * T, 0, rnd)
        finally:
            mset.release()
    finally:
        release(A + B)
    assert eng.rows_stats() == before


def test_the_handle_goes_straight_into_the_lookup_sum(engines, srs_of):
    lg, L, w = 10, 2, 2
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(31)
    inputs, table, mult = lk.lookup_instance(L, w, T, 77, duplicates=True)
    theta, beta = rnd.randrange(R), rnd.randrange(R)
    S, closing = lk.lookup_sum(inputs, table, mult, L, w, theta, beta)
    assert closing == 0
    F, Tb, M = commit_sets(eng, inputs, (4,)), commit_sets(eng, table, (2,)), commit_sets(eng, [mult], (1,))
    try:
        mset, miss = eng.commit_multiplicities(F, Tb, L, w)
        try:
            assert miss == 0 and mset.commitments == M[0].commitments
            dev, dev_cl = eng.commit_lookup_sum(F, Tb, mset, L, w, be(theta), be(beta))
            dev.release()
            host, host_cl = eng.commit_lookup_sum(F, Tb, M[0], L, w, be(theta), be(beta))
            host.release()
            assert dev_cl == host_cl == be(0)
            assert dev.commitments[0] == host.commitments[0] == oc.commit(srs, row_bytes(S), True)
        finally:
            mset.release()
    finally:
        release(F + Tb + M)
    assert eng.rows_stats() == before


def test_determinism_in_a_row_and_from_four_threads(engines, srs_of):
    lg, L, w = 12, 3, 2
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    inputs, table = instance(L, w, T, 801, duplicates=True)
    inputs = lk.break_instance(inputs, table, w, 802)
    mult, missing = multiplicities(inputs, table, L, w)
    want = (oc.commit(srs, row_bytes(mult), True), missing)
    assert missing == 1
    F, Tb = commit_sets(eng, inputs, (2, 4)), commit_sets(eng, table, (2,))
    wr = pow(7, (R - 1) // T, R)
    pts = [be(pow(wr, t, R)) for t in (0, T // 2 + 1, T - 1)]

    def one():
        ms, miss = eng.commit_multiplicities(F, Tb, L, w)
        try:
            return ms.commitments[0], miss, eng.eval_rows([ms], pts, [[0]] * 3)
        finally:
            ms.release()

    runs = [one() for _ in range(3)]
    assert runs[0][:2] == want and runs[1] == runs[0] and runs[2] == runs[0]
    errors, got = [], []

    def work():
        try:
            for _ in range(3):
                got.append(one())
        except Exception as ex:   # noqa: BLE001
            errors.append(repr(ex))

    ths = [threading.Thread(target=work) for _ in range(4)]
    for x in ths:
        x.start()
    for x in ths:
        x.join()
    assert not errors, errors
    assert len(got) == 12 and all(g == runs[0] for g in got)
    release(F + Tb)
    assert eng.rows_stats() == before


def arg_error(fn, why=None, code=_native.KZG_E_ARG):
    """every error of this builder names it"""
    assert "multiplicities" in str(rows_arg_error(fn, why, code))


def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 8
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    srs = oc.srs_gen(be(SEED_X), be(SEED_Y), lg + 1, 1, 0)
    L, w = 2, 2
    inputs, table = instance(L, w, T, 701)
    mult, missing = multiplicities(inputs, table, L, w)
    want = (oc.commit(srs, row_bytes(mult), True), missing)
    call = eng.commit_multiplicities

    def fresh_ok(F, Tb):
        ms, miss = call(F, Tb, L, w)
        ms.release()
        assert (ms.commitments[0], miss) == want

    F, Tb = commit_sets(eng, inputs, (1, 3)), commit_sets(eng, table, (2,))
    fresh_ok(F, Tb)
    arg_error(lambda: call(F[:1], Tb, L, w), "n_lookups * width rows")             # 1 input row for 4
    arg_error(lambda: call(F, Tb, 4, 1), "width rows")                              # 2 table rows for w = 1
    arg_error(lambda: call(F, Tb + Tb, L, w), "width rows")                         # 4 table rows for w = 2
    arg_error(lambda: call(F, Tb, 0, w))                                            # L = 0
    arg_error(lambda: call(F, Tb, L, 0))                                            # w = 0
    hf, ht = (ctypes.c_uint64 * 2)(F[0].handle, F[1].handle), (ctypes.c_uint64 * 1)(Tb[0].handle)
    c, ms, h = ctypes.create_string_buffer(48), ctypes.c_uint64(0), ctypes.c_uint64(0)
    lib = _native.load()
    f = lib.kzg_rows_commit_multiplicities
    E = _native.KZG_E_ARG
    assert f(eng._h, 2, hf, 1, ht, 0, 2, c, ctypes.byref(ms), ctypes.byref(h)) == E
    assert f(eng._h, 2, hf, 1, ht, 2, 0, c, ctypes.byref(ms), ctypes.byref(h)) == E
    assert f(eng._h, 2, hf, 1, ht, 17, 1, c, ctypes.byref(ms), ctypes.byref(h)) == E
    assert f(eng._h, 2, hf, 1, ht, 9, 2, c, ctypes.byref(ms), ctypes.byref(h)) == E
    assert f(eng._h, 2, hf, 1, ht, 2 ** 31, 2, c, ctypes.byref(ms), ctypes.byref(h)) == E      # L w wraps in 32 bits
    assert f(eng._h, 0, hf, 1, ht, 2, 2, c, ctypes.byref(ms), ctypes.byref(h)) == E
    assert f(eng._h, 2, hf, 17, ht, 2, 2, c, ctypes.byref(ms), ctypes.byref(h)) == E
    assert f(eng._h, 2, hf, 1, ht, 2, 2, c, None, ctypes.byref(h)) == E                        # nowhere to put `missing`
    assert f(eng._h, 2, hf, 1, ht, 2, 2, c, ctypes.byref(ms), ctypes.byref(h)) == 0            # (the same call, in range)
    assert (c.raw, ms.value) == want
    eng.release_rows(h.value)
    arg_error(lambda: call(F * 6, Tb, 8, 2), "KZG_MAX_BATCH_OPEN rows")             # 24 input rows
    other = commit_sets(eng, table, (2,), i=1)                                       # another worker
    arg_error(lambda: call(F, other, L, w), "one worker")
    short = eng.commit_rows(0, [row_bytes(r[:T // 2]) for r in table])               # another length
    arg_error(lambda: call(F, [short], L, w), "one worker and have one row length")
    odd = [eng.commit_rows(0, [row_bytes(r[:T - 1]) for r in table], False), eng.commit_rows(0, [row_bytes(r[:T - 1]) for r in inputs], False)]
    arg_error(lambda: call(odd[1:], odd[:1], L, w), "power of two")                 # coefficient rows of length T - 1
    release(other + [short] + odd)
    gone = commit_sets(eng, table, (2,))
    release(gone)
    arg_error(lambda: call(F, gone, L, w), "released")
    arg_error(lambda: call([2 ** 40], Tb, L, w), "unknown")
    arg_error(lambda: call(F, [2 ** 40], L, w), "unknown")
    fresh_ok(F, Tb)
    # the 65th live set
    fill = [eng.commit_rows(0, [row_bytes(table[0])]) for _ in range(_native.KZG_MAX_ROW_SETS - 3)]
    assert eng.rows_stats()[0] == _native.KZG_MAX_ROW_SETS
    arg_error(lambda: call(F, Tb, L, w), "KZG_MAX_ROW_SETS", code=_native.KZG_E_BUSY)
    fill.pop().release()
    fresh_ok(F, Tb)
    release(fill)
    # stale after an SRS load, the new set with its sources
    keep, _ = call(F, Tb, L, w)
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: call(F, Tb, L, w), "SRS")
    arg_error(lambda: call([keep], [keep], 1, 1), "SRS")
    release(F + Tb + [keep])
    F, Tb = commit_sets(eng, inputs, (1, 3)), commit_sets(eng, table, (2,))
    fresh_ok(F, Tb)
    release(F + Tb)
    assert eng.rows_stats() == (0, 0)


def test_a_racing_release(engines, srs_of):
    lg, L, w = 12, 3, 1
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    inputs, table = instance(L, w, T, 811)
    mult, missing = multiplicities(inputs, table, L, w)
    want = (oc.commit(srs, row_bytes(mult), True), missing)
    F, Tb = commit_sets(eng, inputs[:2], (2,)), commit_sets(eng, table, (1,))
    for n in range(6):
        victim = commit_sets(eng, inputs[2:], (1,))[0]
        out = []

        def call():
            try:
                ms, miss = eng.commit_multiplicities([F[0], victim], Tb, L, w)
                ms.release()
                out.append((ms.commitments[0], miss))
            except KzgError as ex:
                out.append(ex.code)

        th = threading.Thread(target=call)
        th.start()
        if n % 2:
            threading.Event().wait(0.0002 * n)
        victim.release()
        th.join()
        assert out[0] in (want, _native.KZG_E_ARG), out
    release(F + Tb)
    assert eng.rows_stats() == before


def test_multi_handle_returns_the_reference_bytes(hip):
    lib = _native.load()
    scale, ms = 12, 2
    T, M, G = 1 << (scale - ms), 1 << ms, 3
    tx, ty = 0xABCDEF0123, 0x13579BDF
    devs = (ctypes.c_int * G)(0, 0, 0)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(G, devs, ctypes.byref(mh)) == 0
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        c, cc, miss = ctypes.create_string_buffer(48), ctypes.create_string_buffer(96), ctypes.c_uint64(0)
        made = {}
        for i in range(M):
            inputs, table = instance(2, 1, T, 900 + i, duplicates=True)
            inputs[1][i] = R - 1 - i                                                       # one miss
            mult, missing = multiplicities(inputs, table, 2, 1)
            assert missing == 1
            srs = oc.srs_gen(be(tx), be(ty), scale, ms, i)
            hf, ht, hm = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 2, b"".join(row_bytes(r) for r in inputs), T, 1, cc, ctypes.byref(hf)) == 0
            assert lib.kzg_multi_rows_commit(mh, i, 1, row_bytes(table[0]), T, 1, cc, ctypes.byref(ht)) == 0
            af, at = (ctypes.c_uint64 * 1)(hf.value), (ctypes.c_uint64 * 1)(ht.value)
            assert lib.kzg_multi_rows_commit_multiplicities(mh, i, 1, af, 1, at, 2, 1, c, ctypes.byref(miss),
                                                            ctypes.byref(hm)) == 0, i
            assert (c.raw, miss.value) == (oc.commit(srs, row_bytes(mult), True), 1)
            made[i] = (hf.value, ht.value, hm.value)
        # worker 3 shares worker 0's device, worker 1 lives elsewhere: both are refused under index 0
        hz = ctypes.c_uint64(0)
        for wrong in (3, 1):
            af, at = (ctypes.c_uint64 * 1)(made[wrong][0]), (ctypes.c_uint64 * 1)(made[wrong][1])
            assert lib.kzg_multi_rows_commit_multiplicities(mh, 0, 1, af, 1, at, 2, 1, c, ctypes.byref(miss),
                                                            ctypes.byref(hz)) == _native.KZG_E_ARG
        for i in range(M):
            for h in made[i]:
                assert lib.kzg_multi_rows_release(mh, i, h) == 0
    finally:
        lib.kzg_multi_destroy(mh)


def test_no_row_sized_copy_inside_the_call(engines):
    """structural: with stage profiling on, the call opens no upload span (only upload_fr opens KZG_T_DECODE), while the
    transforms, the join kernels and the one MSM's accumulate all ran"""
    lg = 12
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    inputs, table = instance(2, 2, T, 1101)
    F, Tb = commit_sets(eng, inputs, (4,)), commit_sets(eng, table, (2,))
    lib = _native.load()
    try:
        plain, plain_miss = eng.commit_multiplicities(F, Tb, 2, 2)
        plain.release()
        assert lib.kzg_set_profiling(eng._h, 1) == 0
        try:
            ms, miss = eng.commit_multiplicities(F, Tb, 2, 2)
            ms.release()
            tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
            assert lib.kzg_get_timings(eng._h, tms, len(tms)) == 0
        finally:
            assert lib.kzg_set_profiling(eng._h, 0) == 0
        t = dict(zip(_native.TIMING_NAMES, tms))
        print("multiplicities stage times (ms):", {k: round(v, 4) for k, v in t.items()})
        assert t["decode"] == 0
        assert t["ntt"] > 0 and t["poly"] > 0 and t["accumulate"] > 0
        assert (ms.commitments[0], miss) == (plain.commitments[0], plain_miss)
    finally:
        release(F + Tb)
    assert eng.rows_stats() == before
