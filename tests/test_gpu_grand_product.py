"""GPU tests (`-m gpu`) of kzg_rows_commit_grand_product: the permutation accumulator z built on the device from committed
row sets.  The expected z comes from the definition in Python integers (tests/grand_product_ref.py) and is committed with
the C oracle, never with the library under test: commitment, closing value and z's evaluations are compared bit for bit;
a real permutation closes, opens with the wire sets and verifies; edge values, the zero denominator, every documented
error, threads, a racing release and the multi-GPU handle follow.  Each test leaves rows_stats() where it found it."""
import ctypes
import random
import threading

import pytest

from oracle import cpu as oc
from tests import grand_product_ref as gp
from tests.gpu_common import ints
from tests.gpu_rows import (arg_error, check_one_row, commit_sets, engine_cache, probes_ends, rand_rows, release,
                            split_first as split, srs_cache)
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import lagrange_factor

pytestmark = pytest.mark.gpu
R = gp.R
be, row_bytes = gp.be, gp.row_bytes
SEED_X, SEED_Y = 0x6A0D01, 0x6A0D02
ONE = be(1)


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def gp_call(eng, W, S, shifts, beta, gamma):
    return eng.commit_grand_product(W, S, [be(s) for s in shifts], be(beta), be(gamma))


def check_against_reference(eng, srs, zset, closing, z, want_closing, rnd):
    assert closing == be(want_closing)
    check_one_row(eng, srs, zset, z, rnd, probes=probes_ends(len(z), rnd))


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("lg", [4, 10, 12, 16])
def test_bit_exact_against_the_oracle(engines, srs_of, lg, k):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(100 * lg + k)
    wires, sigmas = rand_rows(k, T, 1000 * lg + k), rand_rows(k, T, 2000 * lg + k)
    shifts = [rnd.randrange(R) for _ in range(k)]
    beta, gamma = rnd.randrange(R), rnd.randrange(R)
    z, closing = gp.grand_product(wires, sigmas, shifts, beta, gamma)
    for ef, one_set in ((True, True), (False, False)):
        W = commit_sets(eng, wires, (k,) if one_set else split(k), ef)
        S = commit_sets(eng, sigmas, (k,) if one_set else split(k)[::-1], ef)
        try:
            zset, cl = gp_call(eng, W, S, shifts, beta, gamma)
            try:
                assert eng.rows_stats()[0] == before[0] + len(W) + len(S) + 1
                assert (zset.i, zset.T) == (0, T)
                check_against_reference(eng, srs, zset, cl, z, closing, rnd)
            finally:
                zset.release()
        finally:
            release(W + S)
    assert eng.rows_stats() == before


def test_large_row_through_the_trapdoor(engines):
    lg, k = 20, 3
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    wires, sigmas = rand_rows(k, T, 20001), rand_rows(k, T, 20002)
    shifts, beta, gamma = [1, 7, 49], 0xB20, 0x6A20
    z, closing = gp.grand_product(wires, sigmas, shifts, beta, gamma)
    W, S = commit_sets(eng, wires, (k,)), commit_sets(eng, sigmas, (1, 2))
    try:
        zset, cl = gp_call(eng, W, S, shifts, beta, gamma)
        try:
            zc = oc.fr_ntt(row_bytes(z), True)
            s0 = lagrange_factor(0, 0, SEED_Y)
            want = oc.g1_mul_gen(be(s0 * int.from_bytes(oc.fr_eval(zc, be(SEED_X + lg)), "big")))   # [s0 z(tau)] G
            assert zset.commitments[0] == want
            assert cl == be(closing)
            w = gp.omega(T)
            ts = [0, 1, T - 1, 0x5A5A5]
            Y = eng.eval_rows([zset], [be(pow(w, t, R)) for t in ts], [[0]] * 4)
            assert [y[0] for y in Y] == [be(z[t]) for t in ts]
        finally:
            zset.release()
    finally:
        release(W + S)
    assert eng.rows_stats() == before


def test_real_permutation_closes_opens_and_verifies(engines):
    lg, k = 10, 3
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(31)
    wires, sigmas, shifts = gp.permutation_instance(k, T, 77)
    beta, gamma = rnd.randrange(R), rnd.randrange(R)
    z, closing = gp.grand_product(wires, sigmas, shifts, beta, gamma)
    assert closing == 1
    W, S = commit_sets(eng, wires, (k,)), commit_sets(eng, sigmas, (k,))
    try:
        zset, cl = gp_call(eng, W, S, shifts, beta, gamma)
        try:
            assert cl == ONE
            w = gp.omega(T)
            zeta = rnd.randrange(R)
            P = [be(zeta), be(zeta * w)]
            sets = W + S + [zset]                                   # rows: a0 a1 a2 | s0 s1 s2 | z
            C = [c for s in sets for c in s.commitments]
            opened, G = [list(range(7)), [6]], [be(rnd.randrange(R)), be(rnd.randrange(R))]
            Y, Pf = eng.open_rows(sets, P, opened, G)
            assert eng.verify_open_multi(0, C, P, opened, G, Y, Pf)
            L = [[be(rnd.randrange(R)) for _ in range(7)], [be(0)] * 6 + [ONE]]
            V, Pl = eng.open_rows_lincomb(sets, P, L)
            assert eng.verify_open_lincomb(0, C, P, L, V, Pl)
            assert V[1] == Y[1][0]
            # the step relation holds on the domain (not at a random zeta): sampled w^t, evaluations from the device
            N, D = gp.factors(wires, sigmas, shifts, beta, gamma)
            for t in (0, 1, T // 2, T - 2, T - 1, rnd.randrange(T)):
                x = pow(w, t, R)
                E = eng.eval_rows(sets, [be(x), be(x * w)], [list(range(7)), [6]])
                a, sg, zt, ztw = [int.from_bytes(y, "big") for y in E[0][:3]], [int.from_bytes(y, "big") for y in E[0][3:6]], \
                    int.from_bytes(E[0][6], "big"), int.from_bytes(E[1][0], "big")
                n = d = 1
                for j in range(k):
                    n = n * (a[j] + beta * shifts[j] % R * x + gamma) % R
                    d = d * (a[j] + beta * sg[j] + gamma) % R
                assert (n, d) == (N[t], D[t])
                assert (ztw * d - zt * n) % R == 0
        finally:
            zset.release()
    finally:
        release(W + S)
    assert eng.rows_stats() == before


def test_edge_values(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(5)
    wires, sigmas = rand_rows(3, T, 501), rand_rows(3, T, 502)
    wires[1] = [0] * T                                                          # a zero wire row
    cases = [([1, R - 1, 5], 0, rnd.randrange(1, R)),                           # beta = 0; shifts 1 and r - 1
             ([1, R - 1, 5], rnd.randrange(1, R), 0),                           # gamma = 0 (random sigma rows: D_t != 0)
             ([R - 1, 1, 0], R - 1, R - 1)]
    W, S = commit_sets(eng, wires, (3,)), commit_sets(eng, sigmas, (2, 1))
    try:
        for shifts, beta, gamma in cases:
            z, closing = gp.grand_product(wires, sigmas, shifts, beta, gamma)
            zset, cl = gp_call(eng, W, S, shifts, beta, gamma)
            try:
                check_against_reference(eng, srs, zset, cl, z, closing, rnd)
            finally:
                zset.release()
        # a repeated handle: the one-row set S[1] three times as the sigma rows, W[0]'s rows as the wires
        sig3 = [sigmas[2]] * 3
        z, closing = gp.grand_product(wires, sig3, [3, 4, 5], 11, 12)
        zset, cl = gp_call(eng, W, [S[1]] * 3, [3, 4, 5], 11, 12)
        try:
            check_against_reference(eng, srs, zset, cl, z, closing, rnd)
        finally:
            zset.release()
        # wires == sigma with shifts that make N == D: sigma_j = s_j w^t, so z == 1 everywhere
        dom = gp.domain(T)
        ident = [[s * x % R for x in dom] for s in (1, 7)]
        I = commit_sets(eng, ident, (2,))
        try:
            zset, cl = gp_call(eng, I, I, [1, 7], rnd.randrange(R), rnd.randrange(R))
            try:
                assert cl == ONE
                assert zset.commitments[0] == oc.commit(srs, ONE * T, True)
            finally:
                zset.release()
        finally:
            release(I)
    finally:
        release(W + S)
    assert eng.rows_stats() == before


def test_zero_denominator_is_detected_on_the_device(engines, srs_of):
    lg = 12
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(12)
    wires, sigmas = rand_rows(2, T, 601), rand_rows(2, T, 602)
    shifts, beta = [1, 7], rnd.randrange(R)
    W, S = commit_sets(eng, wires, (2,)), commit_sets(eng, sigmas, (2,), ef=False)
    try:
        live = eng.rows_stats()
        for t in (0, 1234, T - 1):
            gamma = -(wires[0][t] + beta * sigmas[0][t]) % R
            arg_error(lambda: gp_call(eng, W, S, shifts, beta, gamma), "zero denominator")
            assert eng.rows_stats() == live
        gamma = rnd.randrange(R)
        z, closing = gp.grand_product(wires, sigmas, shifts, beta, gamma)
        zset, cl = gp_call(eng, W, S, shifts, beta, gamma)
        try:
            check_against_reference(eng, srs, zset, cl, z, closing, rnd)
        finally:
            zset.release()
    finally:
        release(W + S)
    assert eng.rows_stats() == before


def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 8
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    srs = oc.srs_gen(be(SEED_X), be(SEED_Y), lg + 1, 1, 0)
    rnd = random.Random(8)
    wires, sigmas = rand_rows(3, T, 701), rand_rows(3, T, 702)
    shifts, beta, gamma = [1, 2, 3], 5, 6
    z, closing = gp.grand_product(wires, sigmas, shifts, beta, gamma)
    want = (oc.commit(srs, row_bytes(z), True), be(closing))

    def fresh_ok(W, S):
        zs, cl = gp_call(eng, W, S, shifts, beta, gamma)
        zs.release()
        assert (zs.commitments[0], cl) == want

    W, S = commit_sets(eng, wires, (3,)), commit_sets(eng, sigmas, (1, 2))
    fresh_ok(W, S)
    arg_error(lambda: gp_call(eng, W, S[:1], shifts, beta, gamma), "exactly k rows")           # 3 wire rows, 1 sigma row
    arg_error(lambda: gp_call(eng, W, S, shifts[:2], beta, gamma), "exactly k rows")            # k = 2, 3 rows each
    arg_error(lambda: eng.commit_grand_product(W, S, [], be(beta), be(gamma)))                  # k = 0
    hw, hs = (ctypes.c_uint64 * 1)(W[0].handle), (ctypes.c_uint64 * 2)(S[0].handle, S[1].handle)
    c, cl, h = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.c_uint64(0)
    lib = _native.load()
    assert lib.kzg_rows_commit_grand_product(eng._h, 1, hw, 2, hs, 0, ONE * 3, ONE, ONE, c, cl, ctypes.byref(h)) == _native.KZG_E_ARG
    assert lib.kzg_rows_commit_grand_product(eng._h, 1, hw, 2, hs, 17, ONE * 17, ONE, ONE, c, cl, ctypes.byref(h)) == _native.KZG_E_ARG
    arg_error(lambda: gp_call(eng, W * 6, S, [1] * 16, beta, gamma), "KZG_MAX_BATCH_OPEN rows")  # 18 wire rows
    big = R.to_bytes(32, "big")
    arg_error(lambda: eng.commit_grand_product(W, S, [be(1), big, be(3)], be(5), be(6)), "canonical")
    arg_error(lambda: eng.commit_grand_product(W, S, [be(1)] * 3, big, be(6)), "canonical")
    arg_error(lambda: eng.commit_grand_product(W, S, [be(1)] * 3, be(5), b"\xff" * 32), "canonical")
    other = commit_sets(eng, sigmas, (3,), i=1)                                                   # another worker
    arg_error(lambda: gp_call(eng, W, other, shifts, beta, gamma), "one worker")
    short = eng.commit_rows(0, [row_bytes(r[:T // 2]) for r in sigmas])                            # another length
    arg_error(lambda: gp_call(eng, W, [short], shifts, beta, gamma), "one worker and have one row length")
    release(other + [short])
    gone = commit_sets(eng, sigmas, (3,))
    release(gone)
    arg_error(lambda: gp_call(eng, W, gone, shifts, beta, gamma), "released")
    arg_error(lambda: gp_call(eng, [2 ** 40], S, shifts, beta, gamma), "unknown")
    fresh_ok(W, S)
    # the 65th live set
    fill = [eng.commit_rows(0, [row_bytes(wires[0])]) for _ in range(_native.KZG_MAX_ROW_SETS - 3)]
    assert eng.rows_stats()[0] == _native.KZG_MAX_ROW_SETS
    arg_error(lambda: gp_call(eng, W, S, shifts, beta, gamma), "KZG_MAX_ROW_SETS", code=_native.KZG_E_BUSY)
    fill.pop().release()
    fresh_ok(W, S)
    release(fill)
    # stale after an SRS load
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: gp_call(eng, W, S, shifts, beta, gamma), "SRS")
    release(W + S)
    W, S = commit_sets(eng, wires, (3,)), commit_sets(eng, sigmas, (1, 2))
    fresh_ok(W, S)
    release(W + S)
    assert eng.rows_stats() == (0, 0)


def test_threads_and_a_racing_release(engines):
    lg = 12
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    wires, sigmas = rand_rows(3, T, 801), rand_rows(3, T, 802)
    shifts = [1, 7, 49]
    W, S = commit_sets(eng, wires, (3,)), commit_sets(eng, sigmas, (2, 1))
    chal = {t: (1000 + t, 2000 + t) for t in range(4)}
    want = {}
    for t, (b, g) in chal.items():
        zs, cl = gp_call(eng, W, S, shifts, b, g)
        zs.release()
        want[t] = (zs.commitments[0], cl)
    errors = []

    def work(t):
        try:
            for _ in range(4):
                zs, cl = gp_call(eng, W, S, shifts, *chal[t])
                zs.release()
                assert (zs.commitments[0], cl) == want[t]
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
        victim = commit_sets(eng, sigmas[2:], (1,))[0]
        out = []

        def call():
            try:
                zs, cl = gp_call(eng, W, [S[0], victim], shifts, *chal[0])
                zs.release()
                out.append((zs.commitments[0], cl))
            except KzgError as ex:
                out.append(ex.code)

        th = threading.Thread(target=call)
        th.start()
        if n % 2:
            threading.Event().wait(0.0002 * n)
        victim.release()
        th.join()
        assert out[0] in (want[0], _native.KZG_E_ARG), out
    release(W + S)
    assert eng.rows_stats() == before


def test_multi_handle_returns_the_context_bytes(hip):
    lib = _native.load()
    scale, ms = 12, 2
    T, M, G = 1 << (scale - ms), 1 << ms, 3
    tx, ty = 0xABCDEF0123, 0x13579BDF
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    devs = (ctypes.c_int * G)(0, 0, 0)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(G, devs, ctypes.byref(mh)) == 0
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        shifts, beta, gamma = b"".join(be(s) for s in (1, 7)), be(21), be(22)
        c, cl, cc = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.create_string_buffer(96)
        made = {}
        for i in range(M):
            wires, sigmas = rand_rows(2, T, 900 + i), rand_rows(2, T, 950 + i)
            W, S = commit_sets(single, wires, (2,), i=i), commit_sets(single, sigmas, (2,), i=i)
            zs, want_cl = single.commit_grand_product(W, S, [be(1), be(7)], beta, gamma)
            release(W + S + [zs])
            hw, hs, hz = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 2, b"".join(row_bytes(r) for r in wires), T, 1, cc, ctypes.byref(hw)) == 0
            assert lib.kzg_multi_rows_commit(mh, i, 2, b"".join(row_bytes(r) for r in sigmas), T, 1, cc, ctypes.byref(hs)) == 0
            aw, as_ = (ctypes.c_uint64 * 1)(hw.value), (ctypes.c_uint64 * 1)(hs.value)
            assert lib.kzg_multi_rows_commit_grand_product(mh, i, 1, aw, 1, as_, 2, shifts, beta, gamma, c, cl,
                                                           ctypes.byref(hz)) == 0, i
            assert (c.raw, cl.raw) == (zs.commitments[0], want_cl)
            made[i] = (hw.value, hs.value, hz.value)
        # worker 3 shares worker 0's device, worker 1 lives elsewhere: both are refused under index 0
        for wrong in (3, 1):
            aw, as_ = (ctypes.c_uint64 * 1)(made[wrong][0]), (ctypes.c_uint64 * 1)(made[wrong][1])
            assert lib.kzg_multi_rows_commit_grand_product(mh, 0, 1, aw, 1, as_, 2, shifts, beta, gamma, c, cl,
                                                           ctypes.byref(hz)) == _native.KZG_E_ARG
        for i in range(M):
            for h in made[i]:
                assert lib.kzg_multi_rows_release(mh, i, h) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)


def test_no_row_sized_copy_inside_the_call(engines):
    """structural: with stage profiling on, the call opens no upload span (only upload_fr opens KZG_T_DECODE), while the
    transforms, the product kernels and the one MSM's accumulate all ran"""
    lg = 12
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    wires, sigmas = rand_rows(3, T, 1101), rand_rows(3, T, 1102)
    W, S = commit_sets(eng, wires, (3,)), commit_sets(eng, sigmas, (3,))
    lib = _native.load()
    try:
        plain, plain_cl = gp_call(eng, W, S, [1, 7, 49], 3, 4)
        plain.release()
        assert lib.kzg_set_profiling(eng._h, 1) == 0
        try:
            zs, cl = gp_call(eng, W, S, [1, 7, 49], 3, 4)
            zs.release()
            tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
            assert lib.kzg_get_timings(eng._h, tms, len(tms)) == 0
        finally:
            assert lib.kzg_set_profiling(eng._h, 0) == 0
        t = dict(zip(_native.TIMING_NAMES, tms))
        print("grand product stage times (ms):", {k: round(v, 4) for k, v in t.items()})
        assert t["decode"] == 0
        assert t["ntt"] > 0 and t["poly"] > 0 and t["accumulate"] > 0
        assert (zs.commitments[0], cl) == (plain.commitments[0], plain_cl)
    finally:
        release(W + S)
    assert eng.rows_stats() == before


def test_inversion_hook(hip):
    eng = hip()
    rnd = random.Random(99)
    vals = [1, R - 1, 2, (R + 1) // 2, 7] + [rnd.randrange(1, R) for _ in range(123)]
    out, zero = eng.test_fr_inv(b"".join(be(v) for v in vals))
    assert zero == [0] * len(vals)
    assert ints(out) == [pow(v, -1, R) for v in vals]
    out, zero = eng.test_fr_inv(be(0) + be(3) + be(0))
    assert zero == [1, 0, 1]
    assert ints(out) == [0, pow(3, -1, R), 0]
