"""GPU tests (`-m gpu`) of kzg_rows_commit_lookup_sum: the logUp running sum S built on the device from committed row sets.
The expected S comes from the definition in Python integers (tests/lookup_ref.py) and is committed with the C oracle, never
with the library under test: commitment, closing value and S's evaluations are compared bit for bit; built instances close,
broken ones do not; edge values, the zero denominator, every documented error, threads, a racing release, the multi-GPU
handle, the batched inversion alone (kzg_test_field, Fr op 9) and the opening of S beside its sources follow.  Each test
leaves rows_stats() where it found it."""
import ctypes
import random
import threading

import pytest

from oracle import cpu as oc
from tests import lookup_ref as lk
from tests.gpu_common import ints, rand_scalars_bytes
from tests.gpu_rows import (arg_error, check_one_row, commit_sets, engine_cache, probes_ends, rand_rows, release,
                            split_first as split, srs_cache)
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import lagrange_factor

pytestmark = pytest.mark.gpu
R = lk.R
be, row_bytes = lk.be, lk.row_bytes
SEED_X, SEED_Y = 0x10C0B1, 0x10C0B2
ZERO, ONE = be(0), be(1)
SHAPES = [(1, 1), (2, 1), (4, 3), (16, 1), (1, 16)]


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def lk_call(eng, F, Tb, M, L, w, theta, beta):
    return eng.commit_lookup_sum(F, Tb, M, L, w, be(theta), be(beta))


def check_against_reference(eng, srs, sset, closing, S, want_closing, rnd, want_commitment=None):
    assert closing == be(want_closing)
    check_one_row(eng, srs, sset, S, rnd, probes=probes_ends(len(S), rnd), want_commitment=want_commitment)


def run_both_forms(eng, srs, inputs, table, mult, L, w, theta, beta, rnd, closes):
    """the device call over the sources committed in evaluation form in one set each, then in coefficient form split over
    several sets, against the reference"""
    T = len(mult)
    before = eng.rows_stats()
    S, closing = lk.lookup_sum(inputs, table, mult, L, w, theta, beta)
    assert (closing == 0) == closes
    want_c = oc.commit(srs, row_bytes(S), True)
    for ef, one_set in ((True, True), (False, False)):
        F = commit_sets(eng, inputs, (L * w,) if one_set else split(L * w), ef)
        Tb = commit_sets(eng, table, (w,) if one_set else split(w)[::-1], ef)
        M = commit_sets(eng, [mult], (1,), ef)
        try:
            sset, cl = lk_call(eng, F, Tb, M[0], L, w, theta, beta)
            try:
                assert eng.rows_stats()[0] == before[0] + len(F) + len(Tb) + 2
                assert (sset.i, sset.T) == (0, T)
                check_against_reference(eng, srs, sset, cl, S, closing, rnd, want_c)
            finally:
                sset.release()
        finally:
            release(F + Tb + M)
    assert eng.rows_stats() == before


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"L{s[0]}w{s[1]}")
@pytest.mark.parametrize("lg", [4, 10, 12, 16])
def test_bit_exact_against_the_oracle_random_rows(engines, srs_of, lg, shape):
    L, w = shape
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    rnd = random.Random(100 * lg + 10 * L + w)
    inputs, table, mult = rand_rows(L * w, T, 1000 * lg + L), rand_rows(w, T, 2000 * lg + w), rand_rows(1, T, 3000 * lg)[0]
    run_both_forms(eng, srs, inputs, table, mult, L, w, rnd.randrange(R), rnd.randrange(R), rnd, closes=False)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"L{s[0]}w{s[1]}")
@pytest.mark.parametrize("lg", [4, 10, 12, 16])
def test_bit_exact_against_the_oracle_built_instances(engines, srs_of, lg, shape):
    L, w = shape
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    rnd = random.Random(200 * lg + 10 * L + w)
    inputs, table, mult = lk.lookup_instance(L, w, T, 7000 * lg + 10 * L + w, duplicates=(L + w) % 2 == 1)
    run_both_forms(eng, srs, inputs, table, mult, L, w, rnd.randrange(R), rnd.randrange(R), rnd, closes=True)


def test_the_breaker_does_not_close(engines, srs_of):
    lg, L, w = 10, 4, 3
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    rnd = random.Random(41)
    inputs, table, mult = lk.lookup_instance(L, w, T, 4141)
    broken = lk.break_instance(inputs, table, w, 4142)
    run_both_forms(eng, srs, broken, table, mult, L, w, rnd.randrange(R), rnd.randrange(R), rnd, closes=False)


def test_a_repeated_handle(engines, srs_of):
    """the same one-row set as the input, the table and the multiplicities: term = (1 - f) / (beta + f)"""
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(43)
    f = rand_rows(1, T, 4300)
    A = commit_sets(eng, f, (1,))
    two = commit_sets(eng, rand_rows(2, T, 4310), (2,))
    try:
        theta, beta = rnd.randrange(R), rnd.randrange(R)
        S, closing = lk.lookup_sum(f, f, f[0], 1, 1, theta, beta)
        sset, cl = lk_call(eng, A, A, A[0], 1, 1, theta, beta)
        try:
            check_against_reference(eng, srs, sset, cl, S, closing, rnd)
        finally:
            sset.release()
        # one two-row set four times as the inputs (L = 4, w = 2) and once as the table
        rows2 = rand_rows(2, T, 4310)
        S, closing = lk.lookup_sum(rows2 * 4, rows2, f[0], 4, 2, theta, beta)
        sset, cl = lk_call(eng, two * 4, two, A[0], 4, 2, theta, beta)
        try:
            check_against_reference(eng, srs, sset, cl, S, closing, rnd)
        finally:
            sset.release()
    finally:
        release(A + two)
    assert eng.rows_stats() == before


def test_edge_values(engines, srs_of):
    lg, L, w = 10, 2, 3
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(5)
    inputs, table, mult = rand_rows(L * w, T, 501), rand_rows(w, T, 502), rand_rows(1, T, 503)[0]
    inputs[1] = [R - 1] * T                                                     # a row holding r - 1
    table[2] = [R - 1] * T
    F, Tb = commit_sets(eng, inputs, (L * w,)), commit_sets(eng, table, (1, 2))
    M, M0, Mr = commit_sets(eng, [mult], (1,)), commit_sets(eng, [[0] * T], (1,)), commit_sets(eng, [[R - 1] * T], (1,))
    try:
        cases = [(0, rnd.randrange(1, R), M, mult),                             # theta = 0: only column 0 counts
                 (rnd.randrange(1, R), 0, M, mult),                             # beta = 0 (random rows: no denominator is 0)
                 (0, 0, M, mult),
                 (R - 1, R - 1, M, mult),
                 (rnd.randrange(R), rnd.randrange(R), M0, [0] * T),             # m all zero
                 (rnd.randrange(R), rnd.randrange(R), Mr, [R - 1] * T)]         # m = -1 everywhere
        for theta, beta, Ms, mv in cases:
            S, closing = lk.lookup_sum(inputs, table, mv, L, w, theta, beta)
            sset, cl = lk_call(eng, F, Tb, Ms[0], L, w, theta, beta)
            try:
                check_against_reference(eng, srs, sset, cl, S, closing, rnd)
            finally:
                sset.release()
    finally:
        release(F + Tb + M + M0 + Mr)
    assert eng.rows_stats() == before


def test_the_smallest_rows(hip):
    """T = 2 and T = 4, or the smallest row lengths a row set accepts"""
    done = 0
    for lg in (1, 2, 3, 4):
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
        for L, w in ((1, 1), (3, 2)):
            inputs, table, mult = lk.lookup_instance(L, w, T, 90 + lg)
            run_both_forms(eng, srs, inputs, table, mult, L, w, rnd.randrange(R), rnd.randrange(R), rnd, closes=True)
            inputs = rand_rows(L * w, T, 95 + lg)
            run_both_forms(eng, srs, inputs, table, mult, L, w, rnd.randrange(R), rnd.randrange(R), rnd, closes=False)
        assert eng.rows_stats() == (0, 0)
        done += 1
        if done == 2:
            break
    assert done == 2


def test_large_row_through_the_trapdoor(engines):
    lg, L, w = 20, 2, 2
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    inputs, table, mult = rand_rows(L * w, T, 20001), rand_rows(w, T, 20002), rand_rows(1, T, 20003)[0]
    theta, beta = 0x7E20, 0xBE20
    S, closing = lk.lookup_sum(inputs, table, mult, L, w, theta, beta)
    F, Tb, M = commit_sets(eng, inputs, (1, 3)), commit_sets(eng, table, (w,)), commit_sets(eng, [mult], (1,))
    try:
        sset, cl = lk_call(eng, F, Tb, M[0], L, w, theta, beta)
        try:
            sc = oc.fr_ntt(row_bytes(S), True)
            s0 = lagrange_factor(0, 0, SEED_Y)
            want = oc.g1_mul_gen(be(s0 * int.from_bytes(oc.fr_eval(sc, be(SEED_X + lg)), "big")))   # [s0 S(tau)] G
            assert sset.commitments[0] == want
            assert cl == be(closing)
            wr = pow(7, (R - 1) // T, R)
            ts = [0, 1, T - 1, 0x5A5A5]
            Y = eng.eval_rows([sset], [be(pow(wr, t, R)) for t in ts], [[0]] * 4)
            assert [y[0] for y in Y] == [be(S[t]) for t in ts]
        finally:
            sset.release()
    finally:
        release(F + Tb + M)
    assert eng.rows_stats() == before


def test_zero_denominator_is_detected_on_the_device(engines, srs_of):
    lg, L, w = 12, 2, 2
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(12)
    inputs, table, mult = rand_rows(L * w, T, 601), rand_rows(w, T, 602), rand_rows(1, T, 603)[0]
    theta = rnd.randrange(R)
    F, Tb, M = commit_sets(eng, inputs, (L * w,)), commit_sets(eng, table, (w,), ef=False), commit_sets(eng, [mult], (1,))
    try:
        live = eng.rows_stats()
        for cols in (inputs[2:4], table):                       # planted in the second lookup, then in the table
            comp = lk.compress(cols, theta)
            for t in (0, 1234, T - 1):
                beta = -comp[t] % R
                with pytest.raises(ZeroDivisionError):
                    lk.lookup_sum(inputs, table, mult, L, w, theta, beta)
                arg_error(lambda: lk_call(eng, F, Tb, M[0], L, w, theta, beta), "zero denominator")
                assert eng.rows_stats() == live
        beta = rnd.randrange(R)
        S, closing = lk.lookup_sum(inputs, table, mult, L, w, theta, beta)
        sset, cl = lk_call(eng, F, Tb, M[0], L, w, theta, beta)
        try:
            check_against_reference(eng, srs, sset, cl, S, closing, rnd)
        finally:
            sset.release()
    finally:
        release(F + Tb + M)
    assert eng.rows_stats() == before


def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 8
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    srs = oc.srs_gen(be(SEED_X), be(SEED_Y), lg + 1, 1, 0)
    L, w, theta, beta = 2, 2, 5, 6
    inputs, table, mult = rand_rows(4, T, 701), rand_rows(2, T, 702), rand_rows(1, T, 703)[0]
    S, closing = lk.lookup_sum(inputs, table, mult, L, w, theta, beta)
    want = (oc.commit(srs, row_bytes(S), True), be(closing))

    def fresh_ok(F, Tb, M):
        ss, cl = lk_call(eng, F, Tb, M, L, w, theta, beta)
        ss.release()
        assert (ss.commitments[0], cl) == want

    F, Tb, M = commit_sets(eng, inputs, (1, 3)), commit_sets(eng, table, (2,)), commit_sets(eng, [mult], (1,))[0]
    fresh_ok(F, Tb, M)
    arg_error(lambda: lk_call(eng, F[:1], Tb, M, L, w, theta, beta), "n_lookups * width rows")     # 1 input row for 4
    arg_error(lambda: lk_call(eng, F, Tb, M, 4, 1, theta, beta), "width rows")                      # 2 table rows for w = 1
    arg_error(lambda: lk_call(eng, F, Tb + Tb, M, L, w, theta, beta), "width rows")                 # 4 table rows for w = 2
    arg_error(lambda: lk_call(eng, F, Tb, Tb[0], L, w, theta, beta), "exactly one row")             # a two-row m
    arg_error(lambda: lk_call(eng, F, Tb, M, 0, w, theta, beta))                                    # L = 0
    arg_error(lambda: lk_call(eng, F, Tb, M, L, 0, theta, beta))                                    # w = 0
    hf, ht = (ctypes.c_uint64 * 2)(F[0].handle, F[1].handle), (ctypes.c_uint64 * 1)(Tb[0].handle)
    c, cl, h = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.c_uint64(0)
    lib = _native.load()
    f = lib.kzg_rows_commit_lookup_sum
    assert f(eng._h, 2, hf, 1, ht, M.handle, 0, 2, ONE, ONE, c, cl, ctypes.byref(h)) == _native.KZG_E_ARG
    assert f(eng._h, 2, hf, 1, ht, M.handle, 2, 0, ONE, ONE, c, cl, ctypes.byref(h)) == _native.KZG_E_ARG
    assert f(eng._h, 2, hf, 1, ht, M.handle, 17, 1, ONE, ONE, c, cl, ctypes.byref(h)) == _native.KZG_E_ARG
    assert f(eng._h, 2, hf, 1, ht, M.handle, 9, 2, ONE, ONE, c, cl, ctypes.byref(h)) == _native.KZG_E_ARG
    assert f(eng._h, 2, hf, 1, ht, M.handle, 2 ** 31, 2, ONE, ONE, c, cl, ctypes.byref(h)) == _native.KZG_E_ARG   # L w wraps in 32 bits
    assert f(eng._h, 0, hf, 1, ht, M.handle, 2, 2, ONE, ONE, c, cl, ctypes.byref(h)) == _native.KZG_E_ARG
    assert f(eng._h, 2, hf, 17, ht, M.handle, 2, 2, ONE, ONE, c, cl, ctypes.byref(h)) == _native.KZG_E_ARG
    assert f(eng._h, 2, hf, 1, ht, M.handle, 2, 2, ONE, ONE, c, cl, ctypes.byref(h)) == 0              # (the same call, in range)
    eng.release_rows(h.value)
    arg_error(lambda: lk_call(eng, F * 6, Tb, M, 8, 2, theta, beta), "KZG_MAX_BATCH_OPEN rows")      # 24 input rows
    big = R.to_bytes(32, "big")
    arg_error(lambda: eng.commit_lookup_sum(F, Tb, M, L, w, big, be(6)), "canonical")
    arg_error(lambda: eng.commit_lookup_sum(F, Tb, M, L, w, be(5), b"\xff" * 32), "canonical")
    other = commit_sets(eng, table, (2,), i=1)                                                        # another worker
    arg_error(lambda: lk_call(eng, F, other, M, L, w, theta, beta), "one worker")
    other_m = commit_sets(eng, [mult], (1,), i=1)
    arg_error(lambda: lk_call(eng, F, Tb, other_m[0], L, w, theta, beta), "one worker")
    short = eng.commit_rows(0, [row_bytes(r[:T // 2]) for r in table])                                # another length
    arg_error(lambda: lk_call(eng, F, [short], M, L, w, theta, beta), "one worker and have one row length")
    release(other + other_m + [short])
    gone = commit_sets(eng, table, (2,))
    release(gone)
    arg_error(lambda: lk_call(eng, F, gone, M, L, w, theta, beta), "released")
    arg_error(lambda: lk_call(eng, [2 ** 40], Tb, M, L, w, theta, beta), "unknown")
    arg_error(lambda: lk_call(eng, F, Tb, 2 ** 40, L, w, theta, beta), "unknown")
    fresh_ok(F, Tb, M)
    # the 65th live set
    fill = [eng.commit_rows(0, [row_bytes(mult)]) for _ in range(_native.KZG_MAX_ROW_SETS - 4)]
    assert eng.rows_stats()[0] == _native.KZG_MAX_ROW_SETS
    arg_error(lambda: lk_call(eng, F, Tb, M, L, w, theta, beta), "KZG_MAX_ROW_SETS", code=_native.KZG_E_BUSY)
    fill.pop().release()
    fresh_ok(F, Tb, M)
    release(fill)
    # stale after an SRS load
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: lk_call(eng, F, Tb, M, L, w, theta, beta), "SRS")
    release(F + Tb + [M])
    F, Tb, M = commit_sets(eng, inputs, (1, 3)), commit_sets(eng, table, (2,)), commit_sets(eng, [mult], (1,))[0]
    fresh_ok(F, Tb, M)
    release(F + Tb + [M])
    assert eng.rows_stats() == (0, 0)


def test_threads_and_a_racing_release(engines, srs_of):
    lg, L, w = 12, 3, 1
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    inputs, table, mult = rand_rows(3, T, 801), rand_rows(1, T, 802), rand_rows(1, T, 803)[0]
    F, Tb, M = commit_sets(eng, inputs, (2, 1)), commit_sets(eng, table, (1,)), commit_sets(eng, [mult], (1,))[0]
    chal = {t: (1000 + t, 2000 + t) for t in range(4)}
    want = {}
    for t, (th, b) in chal.items():
        S, closing = lk.lookup_sum(inputs, table, mult, L, w, th, b)
        want[t] = (oc.commit(srs, row_bytes(S), True), be(closing))
    errors = []

    def work(t):
        try:
            for _ in range(4):
                ss, cl = lk_call(eng, F, Tb, M, L, w, *chal[t])
                ss.release()
                assert (ss.commitments[0], cl) == want[t]
        except Exception as ex:   # noqa: BLE001
            errors.append(repr(ex))

    ths = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for x in ths:
        x.start()
    for x in ths:
        x.join()
    assert not errors, errors
    # a release of a source set racing the call: correct bytes or KZG_E_ARG, never anything else
    for n in range(6):
        victim = commit_sets(eng, inputs[2:], (1,))[0]
        out = []

        def call():
            try:
                ss, cl = lk_call(eng, [F[0], victim], Tb, M, L, w, *chal[0])
                ss.release()
                out.append((ss.commitments[0], cl))
            except KzgError as ex:
                out.append(ex.code)

        th = threading.Thread(target=call)
        th.start()
        if n % 2:
            threading.Event().wait(0.0002 * n)
        victim.release()
        th.join()
        assert out[0] in (want[0], _native.KZG_E_ARG), out
    release(F + Tb + [M])
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
        theta, beta = 21, 22
        c, cl, cc = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.create_string_buffer(96)
        made = {}
        for i in range(M):
            inputs, table, mult = lk.lookup_instance(2, 1, T, 900 + i)
            S, closing = lk.lookup_sum(inputs, table, mult, 2, 1, theta, beta)
            srs = oc.srs_gen(be(tx), be(ty), scale, ms, i)
            hf, ht, hm, hz = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 2, b"".join(row_bytes(r) for r in inputs), T, 1, cc, ctypes.byref(hf)) == 0
            assert lib.kzg_multi_rows_commit(mh, i, 1, row_bytes(table[0]), T, 1, cc, ctypes.byref(ht)) == 0
            assert lib.kzg_multi_rows_commit(mh, i, 1, row_bytes(mult), T, 1, cc, ctypes.byref(hm)) == 0
            af, at = (ctypes.c_uint64 * 1)(hf.value), (ctypes.c_uint64 * 1)(ht.value)
            assert lib.kzg_multi_rows_commit_lookup_sum(mh, i, 1, af, 1, at, hm.value, 2, 1, be(theta), be(beta), c, cl,
                                                        ctypes.byref(hz)) == 0, i
            assert (c.raw, cl.raw) == (oc.commit(srs, row_bytes(S), True), be(closing)) and closing == 0
            made[i] = (hf.value, ht.value, hm.value, hz.value)
        # worker 3 shares worker 0's device, worker 1 lives elsewhere: both are refused under index 0
        for wrong in (3, 1):
            af, at = (ctypes.c_uint64 * 1)(made[wrong][0]), (ctypes.c_uint64 * 1)(made[wrong][1])
            assert lib.kzg_multi_rows_commit_lookup_sum(mh, 0, 1, af, 1, at, made[wrong][2], 2, 1, be(theta), be(beta), c, cl,
                                                        ctypes.byref(hz)) == _native.KZG_E_ARG
        for i in range(M):
            for h in made[i]:
                assert lib.kzg_multi_rows_release(mh, i, h) == 0
    finally:
        lib.kzg_multi_destroy(mh)


def test_batched_inversion_hook(hip):
    eng = hip()
    rnd = random.Random(99)
    special = [1, R - 1, pow(2, 255, R), 2, (R + 1) // 2, 7]
    for n in (1, 2, 255, 256, 257, 2 ** 12 + 1, 2 ** 20):
        if n <= 4097:
            vals = [rnd.randrange(1, R) for _ in range(n)]
        else:
            vals = [v or 1 for v in ints(rand_scalars_bytes(n, 9900 + n))]
        for j, v in enumerate(special[:n]):
            vals[(j * 41) % n if n > len(special) else j] = v
        vals[-1] = special[(n - 1) % 3]
        out = eng.test_fr_batch_inv(b"".join(be(v) for v in vals))
        got = ints(out)
        if n <= 4097:
            assert got == [pow(v, -1, R) for v in vals], n
        else:
            assert got == lk.batch_inverse(vals), n           # (one pow; the reference is pinned by the sizes above)
            for j in (0, 1, n // 2, n - 1):
                assert got[j] == pow(vals[j], -1, R)
    for n, at in ((1, 0), (300, 0), (300, 299), (5000, 2500)):
        vals = [rnd.randrange(1, R) for _ in range(n)]
        vals[at] = 0
        arg_error(lambda: eng.test_fr_batch_inv(b"".join(be(v) for v in vals)), "zero")
    assert ints(eng.test_fr_batch_inv(be(3) + be(5))) == [pow(3, -1, R), pow(5, -1, R)]    # the context keeps serving
    out, zero = eng.test_fr_inv(be(0) + be(3))                                              # ops 7 / 8 as before
    assert zero == [1, 0] and ints(out) == [0, pow(3, -1, R)]


def test_the_sum_opens_with_its_sources_and_verifies(engines):
    lg, L, w = 10, 2, 2
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(31)
    inputs, table, mult = lk.lookup_instance(L, w, T, 77)
    theta, beta = rnd.randrange(R), rnd.randrange(R)
    S, closing = lk.lookup_sum(inputs, table, mult, L, w, theta, beta)
    term = lk.terms(inputs, table, mult, L, w, theta, beta)
    assert closing == 0
    F, Tb, M = commit_sets(eng, inputs, (4,)), commit_sets(eng, table, (2,)), commit_sets(eng, [mult], (1,))
    try:
        sset, cl = lk_call(eng, F, Tb, M[0], L, w, theta, beta)
        try:
            assert cl == ZERO
            wr = lk.domain(T)[1]
            zeta = rnd.randrange(R)
            P = [be(zeta), be(zeta * wr)]
            sets = F + Tb + M + [sset]                              # rows: f00 f01 f10 f11 | t0 t1 | m | S
            C = [c for s in sets for c in s.commitments]
            lam = [[be(rnd.randrange(R)) for _ in range(8)], [ZERO] * 7 + [ONE]]
            V, Pl = eng.open_rows_lincomb(sets, P, lam)
            assert eng.verify_open_lincomb(0, C, P, lam, V, Pl)
            sc = oc.fr_ntt(row_bytes(S), True)
            assert V[1] == oc.fr_eval(sc, P[1])
            bad = [V[0], be((int.from_bytes(V[1], "big") + 1) % R)]
            assert not eng.verify_open_lincomb(0, C, P, lam, bad, Pl)
            # the step relation S(wX) - S(X) = term(X) holds on ALL of the domain (the sum closes): sampled w^t
            for t in (0, 1, T // 2, T - 2, T - 1, rnd.randrange(T)):
                x = pow(wr, t, R)
                E = eng.eval_rows([sset], [be(x), be(x * wr)], [[0], [0]])
                st, stw = int.from_bytes(E[0][0], "big"), int.from_bytes(E[1][0], "big")
                assert (st, stw) == (S[t], S[(t + 1) % T])
                assert (stw - st - term[t]) % R == 0
        finally:
            sset.release()
    finally:
        release(F + Tb + M)
    assert eng.rows_stats() == before


def test_no_row_sized_copy_inside_the_call(engines):
    """structural: with stage profiling on, the call opens no upload span (only upload_fr opens KZG_T_DECODE), while the
    transforms, the fraction / inversion / scan kernels and the one MSM's accumulate all ran"""
    lg = 12
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    inputs, table, mult = rand_rows(4, T, 1101), rand_rows(2, T, 1102), rand_rows(1, T, 1103)
    F, Tb, M = commit_sets(eng, inputs, (4,)), commit_sets(eng, table, (2,)), commit_sets(eng, mult, (1,))
    lib = _native.load()
    try:
        plain, plain_cl = lk_call(eng, F, Tb, M[0], 2, 2, 3, 4)
        plain.release()
        assert lib.kzg_set_profiling(eng._h, 1) == 0
        try:
            ss, cl = lk_call(eng, F, Tb, M[0], 2, 2, 3, 4)
            ss.release()
            tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
            assert lib.kzg_get_timings(eng._h, tms, len(tms)) == 0
        finally:
            assert lib.kzg_set_profiling(eng._h, 0) == 0
        t = dict(zip(_native.TIMING_NAMES, tms))
        print("lookup sum stage times (ms):", {k: round(v, 4) for k, v in t.items()})
        assert t["decode"] == 0
        assert t["ntt"] > 0 and t["poly"] > 0 and t["accumulate"] > 0
        assert (ss.commitments[0], cl) == (plain.commitments[0], plain_cl)
    finally:
        release(F + Tb + M)
    assert eng.rows_stats() == before
