"""GPU tests (`-m gpu`) of kzg_rows_commit_shuffle: the running product z of a shuffle argument built on the device from
committed row sets.  The expected z comes from the definition in Python integers (tests/shuffle_ref.py) and is committed with
the C oracle, never with the library under test: commitment, closing value and z's evaluations are compared bit for bit; a
true shuffle closes, opens with its source sets and verifies; selectors, blinding rows, edge values, the zero denominator,
every documented error, threads, a racing release, the multi-GPU handle and the argument end to end through the existing
quotient call follow.  Each test leaves rows_stats() where it found it."""
import ctypes
import random
import threading

import pytest

from oracle import cpu as oc
from tests import shuffle_ref as sr
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import (arg_error, bt, check_one_row, check_pieces, commit_sets, engine_cache, probes_closing, probes_ends,
                            rand_rows, reference_pieces_ext, release, split_first as split, srs_cache, tail_of)
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import lagrange_factor, shuffle_quotient_terms

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x5FF1E01, 0x5FF1E02
ONE = be(1)


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def sh_call(eng, I, S, G, w, theta, gamma, Q=None, input_sel=None, shuffle_sel=None, usable=None, tail=()):
    return eng.commit_shuffle(I, S, G, w, be(theta), be(gamma), Q, input_sel, shuffle_sel, usable, bt(tail))


def pick(rows, idx):
    """the selector rows a list of indices (or None) names"""
    return None if idx is None else [None if j is None else rows[j] for j in idx]


def check_against_reference(eng, srs, zset, closing, z, want_closing, rnd, u=None, blind=False):
    assert closing == be(want_closing)
    check_one_row(eng, srs, zset, z, rnd, probes=probes_closing(len(z), u) if blind else probes_ends(len(z), rnd))


# (one case at the long row: the scan is the grand product's, tested there up to 2^20)
@pytest.mark.parametrize("lg,G,w", [(lg, G, w) for lg in (4, 10, 12) for G, w in ((1, 1), (1, 3), (2, 2), (4, 4))] + [(16, 1, 1)])
def test_bit_exact_against_the_oracle(engines, srs_of, lg, G, w):
    eng, srs, T, k = engines(lg), srs_of(lg), 1 << lg, G * w
    before = eng.rows_stats()
    rnd = random.Random(100 * lg + 10 * G + w)
    ins, shs = rand_rows(k, T, 3000 * lg + k), rand_rows(k, T, 4000 * lg + k)
    theta, gamma = rnd.randrange(R), rnd.randrange(R)
    z, closing = sr.shuffle_product(ins, shs, G, w, theta, gamma)
    assert closing != 1
    for ef, one_set in ((True, True), (False, False)):
        I = commit_sets(eng, ins, (k,) if one_set else split(k), ef)
        S = commit_sets(eng, shs, (k,) if one_set else split(k)[::-1], ef)
        try:
            zset, cl = sh_call(eng, I, S, G, w, theta, gamma)
            try:
                assert eng.rows_stats()[0] == before[0] + len(I) + len(S) + 1
                assert (zset.i, zset.T) == (0, T)
                check_against_reference(eng, srs, zset, cl, z, closing, rnd)
            finally:
                zset.release()
        finally:
            release(I + S)
    assert eng.rows_stats() == before


def test_true_shuffle_closes_opens_and_verifies(engines):
    lg, G, w = 10, 2, 2
    eng, T, k = engines(lg), 1 << lg, 4
    before = eng.rows_stats()
    rnd = random.Random(41)
    ins, shs, _, _ = sr.shuffle_instance(G, w, T, 78)
    theta, gamma = rnd.randrange(R), rnd.randrange(R)
    z, closing = sr.shuffle_product(ins, shs, G, w, theta, gamma)
    assert closing == 1
    I, S = commit_sets(eng, ins, (k,)), commit_sets(eng, shs, (1, 3))
    try:
        zset, cl = sh_call(eng, I, S, G, w, theta, gamma)
        try:
            assert cl == ONE
            om = sr.omega(T)
            zeta = rnd.randrange(R)
            P = [be(zeta), be(zeta * om % R)]
            sets = I + S + [zset]                                   # rows: a (4) | b (4) | z
            C = [c for s in sets for c in s.commitments]
            opened, gam = [list(range(9)), [8]], [be(rnd.randrange(R)), be(rnd.randrange(R))]
            Y, Pf = eng.open_rows(sets, P, opened, gam)
            assert eng.verify_open_multi(0, C, P, opened, gam, Y, Pf)
            # the step relation holds on the domain: sampled w^t, every evaluation from the device
            N, D = sr.factors(ins, shs, G, w, theta, gamma)
            for t in (0, 1, T // 2, T - 2, T - 1, rnd.randrange(T)):
                x = pow(om, t, R)
                E = eng.eval_rows(sets, [be(x), be(x * om % R)], [list(range(9)), [8]])
                v = [int.from_bytes(y, "big") for y in E[0]]
                ztw = int.from_bytes(E[1][0], "big")
                n, d = sr.factors([[a] for a in v[:4]], [[b] for b in v[4:8]], G, w, theta, gamma)
                assert (n[0], d[0]) == (N[t], D[t])
                assert (ztw * d[0] - v[8] * n[0]) % R == 0
        finally:
            zset.release()
    finally:
        release(I + S)
    assert eng.rows_stats() == before


def test_selectors(engines, srs_of):
    lg, G, w = 10, 2, 2
    eng, srs, T, k = engines(lg), srs_of(lg), 1 << lg, 4
    before = eng.rows_stats()
    rnd = random.Random(51)
    theta, gamma = rnd.randrange(R), rnd.randrange(R)
    ins, shs = rand_rows(k, T, 5100), rand_rows(k, T, 5200)
    # selector rows: two 0/1 rows, all ones, a non-boolean one
    qrows = [[rnd.randrange(2) for _ in range(T)], [rnd.randrange(2) for _ in range(T)], [1] * T, rand_rows(1, T, 5300)[0]]
    I, S, Q = commit_sets(eng, ins, (k,)), commit_sets(eng, shs, (2, 2), ef=False), commit_sets(eng, qrows, (1, 3))
    try:
        plain, plain_cl = sh_call(eng, I, S, G, w, theta, gamma)
        plain.release()
        cases = [([0, 1], None), (None, [1, 0]), ([0, None], [None, 1]), ([0, 1], [1, 0]),
                 ([0, 0], [0, 0]),                                  # one row serving both sides of both groups
                 ([3, None], [0, 3])]                               # a non-boolean selector: the formula as written
        for isel, ssel in cases:
            z, closing = sr.shuffle_product(ins, shs, G, w, theta, gamma, pick(qrows, isel), pick(qrows, ssel))
            zset, cl = sh_call(eng, I, S, G, w, theta, gamma, Q, isel, ssel)
            try:
                check_against_reference(eng, srs, zset, cl, z, closing, rnd)
            finally:
                zset.release()
        # all ones, and "none" spelled out: the bytes of the call without selectors
        for isel, ssel in (([2, 2], [2, None]), ([None, None], [None, None])):
            zset, cl = sh_call(eng, I, S, G, w, theta, gamma, Q, isel, ssel)
            zset.release()
            assert (zset.commitments[0], cl) == (plain.commitments[0], plain_cl)
    finally:
        release(I + S + Q)
    # a true instance whose disabled cells hold garbage closes
    ins, shs, qi, qs = sr.shuffle_instance(G, w, T, 79, sel=True)
    z, closing = sr.shuffle_product(ins, shs, G, w, theta, gamma, qi, qs)
    assert closing == 1
    I, S, Q = commit_sets(eng, ins, (k,)), commit_sets(eng, shs, (k,)), commit_sets(eng, qi + qs, (4,))
    try:
        zset, cl = sh_call(eng, I, S, G, w, theta, gamma, Q, [0, 1], [2, 3])
        try:
            check_against_reference(eng, srs, zset, cl, z, 1, rnd)
        finally:
            zset.release()
    finally:
        release(I + S + Q)
    assert eng.rows_stats() == before


def test_blinding_rows(engines, srs_of):
    lg, G, w = 10, 1, 2
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(61)
    theta, gamma = rnd.randrange(R), rnd.randrange(R)
    ins, shs = rand_rows(2, T, 6100), rand_rows(2, T, 6200)
    shs[0][T - 1] = (-gamma - theta * shs[1][T - 1]) % R            # df = 0 at the last row: behind every u below
    early = [r[:] for r in shs]
    early[0][3] = (-gamma - theta * early[1][3]) % R                # and the same at row 3
    I, S, S3 = commit_sets(eng, ins, (2,)), commit_sets(eng, shs, (2,)), commit_sets(eng, early, (1, 1))
    try:
        live = eng.rows_stats()
        for u in (T - 1, T - 2, T - 31):
            tail = tail_of(T, u, 600 + u)
            z, closing = sr.shuffle_product(ins, shs, G, w, theta, gamma, usable=u, tail=tail)
            zset, cl = sh_call(eng, I, S, G, w, theta, gamma, usable=u, tail=tail)
            try:
                check_against_reference(eng, srs, zset, cl, z, closing, rnd, u, blind=True)
            finally:
                zset.release()
            arg_error(lambda: sh_call(eng, I, S3, G, w, theta, gamma, usable=u, tail=tail), "zero denominator")
            assert eng.rows_stats() == live
        arg_error(lambda: sh_call(eng, I, S, G, w, theta, gamma), "zero denominator")   # the plain layout counts row T - 1
        # a true instance under blinding with selectors: closing 1 at row u, garbage behind u ignored
        u = T - 5
        ins2, shs2, qi, qs = sr.shuffle_instance(G, w, T, 80, usable=u, sel=True)
        tail = tail_of(T, u, 66)
        z, closing = sr.shuffle_product(ins2, shs2, G, w, theta, gamma, qi, qs, u, tail)
        assert closing == 1 and z[u] == 1
        J = commit_sets(eng, ins2 + shs2 + qi + qs, (2, 2, 2))
        try:
            zset, cl = sh_call(eng, J[:1], J[1:2], G, w, theta, gamma, J[2:], [0], [1], u, tail)
            try:
                check_against_reference(eng, srs, zset, cl, z, 1, rnd, u, blind=True)
            finally:
                zset.release()
        finally:
            release(J)
    finally:
        release(I + S + S3)
    assert eng.rows_stats() == before


def test_edge_values(engines, srs_of):
    lg, G, w = 10, 1, 3
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(71)
    ins, shs = rand_rows(3, T, 7100), rand_rows(3, T, 7200)
    ins[1] = [0] * T                                                # an all-zero input row
    I, S = commit_sets(eng, ins, (3,)), commit_sets(eng, shs, (2, 1))
    try:
        for theta, gamma in ((0, rnd.randrange(1, R)), (rnd.randrange(1, R), 0), (R - 1, R - 1)):
            z, closing = sr.shuffle_product(ins, shs, G, w, theta, gamma)
            zset, cl = sh_call(eng, I, S, G, w, theta, gamma)
            try:
                check_against_reference(eng, srs, zset, cl, z, closing, rnd)
            finally:
                zset.release()
        # a repeated handle: the one-row set S[1] three times as the shuffle rows
        z, closing = sr.shuffle_product(ins, [shs[2]] * 3, G, w, 11, 12)
        zset, cl = sh_call(eng, I, [S[1]] * 3, G, w, 11, 12)
        try:
            check_against_reference(eng, srs, zset, cl, z, closing, rnd)
        finally:
            zset.release()
        # input set == shuffle set: z == 1 everywhere
        zset, cl = sh_call(eng, I, I, G, w, rnd.randrange(R), rnd.randrange(R))
        zset.release()
        assert cl == ONE
        assert zset.commitments[0] == oc.commit(srs, ONE * T, True)
    finally:
        release(I + S)
    assert eng.rows_stats() == before


def test_zero_denominator_is_detected_on_the_device(engines, srs_of):
    lg, G, w = 12, 1, 2
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(12)
    ins, shs = rand_rows(2, T, 8100), rand_rows(2, T, 8200)
    theta = rnd.randrange(R)
    I, S = commit_sets(eng, ins, (2,)), commit_sets(eng, shs, (2,), ef=False)
    try:
        live = eng.rows_stats()
        for t in (0, 1234, T - 1):
            gamma = -(shs[0][t] + theta * shs[1][t]) % R
            arg_error(lambda: sh_call(eng, I, S, G, w, theta, gamma), "zero denominator")
            assert eng.rows_stats() == live
        gamma = rnd.randrange(R)
        z, closing = sr.shuffle_product(ins, shs, G, w, theta, gamma)
        zset, cl = sh_call(eng, I, S, G, w, theta, gamma)
        try:
            check_against_reference(eng, srs, zset, cl, z, closing, rnd)
        finally:
            zset.release()
    finally:
        release(I + S)
    assert eng.rows_stats() == before


def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg, G, w = 8, 1, 3
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    srs = oc.srs_gen(be(SEED_X), be(SEED_Y), lg + 1, 1, 0)
    ins, shs, qrows = rand_rows(3, T, 9100), rand_rows(3, T, 9200), rand_rows(2, T, 9300)
    theta, gamma = 5, 6
    z, closing = sr.shuffle_product(ins, shs, G, w, theta, gamma)
    want = (oc.commit(srs, row_bytes(z), True), be(closing))

    def fresh_ok(I, S):
        zs, cl = sh_call(eng, I, S, G, w, theta, gamma)
        zs.release()
        assert (zs.commitments[0], cl) == want

    I, S, Q = commit_sets(eng, ins, (3,)), commit_sets(eng, shs, (1, 2)), commit_sets(eng, qrows, (2,))
    fresh_ok(I, S)
    live = eng.rows_stats()
    # shapes
    arg_error(lambda: sh_call(eng, I, S[:1], G, w, theta, gamma), "exactly n_groups * width rows")      # 3 input rows, 1 shuffle row
    arg_error(lambda: sh_call(eng, I, S, 1, 2, theta, gamma), "exactly n_groups * width rows")          # G w = 2, 3 rows each
    arg_error(lambda: sh_call(eng, I, S, 0, 3, theta, gamma), "n_groups")
    arg_error(lambda: sh_call(eng, I, S, 3, 0, theta, gamma), "n_groups")
    arg_error(lambda: sh_call(eng, I, S, 2, 9, theta, gamma), "n_groups")
    lib = _native.load()
    hi, hs = (ctypes.c_uint64 * 1)(I[0].handle), (ctypes.c_uint64 * 2)(S[0].handle, S[1].handle)
    c, cl, h = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.c_uint64(0)

    def raw(G_, w_, opts=None, th=ONE, ga=ONE):
        return lib.kzg_rows_commit_shuffle(eng._h, 1, hi, 2, hs, G_, w_, th, ga, ctypes.byref(opts) if opts else None, c, cl,
                                           ctypes.byref(h))

    E_ARG = _native.KZG_E_ARG
    assert raw(0, 3) == E_ARG and b"n_groups" in lib.kzg_last_error(eng._h)
    assert raw(1, 17) == E_ARG and b"KZG_MAX_BATCH_OPEN" in lib.kzg_last_error(eng._h)
    arg_error(lambda: sh_call(eng, I * 6, S, 1, 16, theta, gamma), "KZG_MAX_BATCH_OPEN rows")           # 18 input rows
    # scalars
    big = R.to_bytes(32, "big")
    arg_error(lambda: eng.commit_shuffle(I, S, G, w, big, be(6)), "canonical")
    arg_error(lambda: eng.commit_shuffle(I, S, G, w, be(5), b"\xff" * 32), "canonical")
    arg_error(lambda: eng.commit_shuffle(I, S, G, w, be(5), be(6), usable=T - 3, tail=[be(1), big]), "canonical")
    # selectors
    arg_error(lambda: sh_call(eng, I, S, G, w, theta, gamma, Q, [2], None), "index the concatenated rows")
    arg_error(lambda: sh_call(eng, I, S, G, w, theta, gamma, Q, None, [7]), "index the concatenated rows")
    arg_error(lambda: sh_call(eng, I, S, G, w, theta, gamma, None, [0], None), "no selector handles")
    arg_error(lambda: sh_call(eng, I, S, G, w, theta, gamma, Q, [0, 1], None), "n_lookups entries")       # the engine's own check
    arg_error(lambda: sh_call(eng, I, S, G, w, theta, gamma, [2 ** 41], [0], None), "unknown")
    # the blinding rows' range, as in the _zk calls
    idx = (ctypes.c_uint32 * 1)(0)
    tl = b"".join(bt(tail_of(T, T - 4, 91)))
    for usable, tail, why in ((T, tl, b"usable"), (2 ** 40, tl, b"usable"), (T - 33, tl, b"KZG_MAX_BLIND_ROWS"),
                              (T - 4, None, b"null"), (0, tl, b"plain layout")):
        opts = _native.ShuffleOpts(0, None, None, None, usable, tail)
        assert raw(1, 3, opts) == E_ARG and why in lib.kzg_last_error(eng._h), (usable, lib.kzg_last_error(eng._h))
    opts = _native.ShuffleOpts(0, None, idx, None, 0, None)                                               # an index, no handles
    assert raw(1, 3, opts) == E_ARG and b"no selector handles" in lib.kzg_last_error(eng._h)
    arg_error(lambda: sh_call(eng, I, S, G, w, theta, gamma, usable=0), "usable")
    arg_error(lambda: sh_call(eng, I, S, G, w, theta, gamma, usable=T - 4, tail=[1, 2]), "exactly")
    assert raw(1, 3, _native.ShuffleOpts(0, None, None, None, T - 1, None)) == 0                          # NULL tail, u = T - 1
    eng.release_rows(h.value)
    assert eng.rows_stats() == live
    # handles
    other = commit_sets(eng, shs, (3,), i=1)                                                              # another worker
    arg_error(lambda: sh_call(eng, I, other, G, w, theta, gamma), "one worker")
    arg_error(lambda: sh_call(eng, I, S, G, w, theta, gamma, other, [0], None), "one worker")
    short = eng.commit_rows(0, [row_bytes(r[:T // 2]) for r in shs])                                      # another length
    arg_error(lambda: sh_call(eng, I, [short], G, w, theta, gamma), "one worker and have one row length")
    release(other + [short])
    gone = commit_sets(eng, shs, (3,))
    release(gone)
    arg_error(lambda: sh_call(eng, I, gone, G, w, theta, gamma), "released")
    arg_error(lambda: sh_call(eng, [2 ** 40], S, G, w, theta, gamma), "unknown")
    fresh_ok(I, S)
    # the 65th live set
    fill = [eng.commit_rows(0, [row_bytes(ins[0])]) for _ in range(_native.KZG_MAX_ROW_SETS - 4)]
    assert eng.rows_stats()[0] == _native.KZG_MAX_ROW_SETS
    arg_error(lambda: sh_call(eng, I, S, G, w, theta, gamma), "KZG_MAX_ROW_SETS", code=_native.KZG_E_BUSY)
    fill.pop().release()
    fresh_ok(I, S)
    release(fill)
    # stale after an SRS load
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: sh_call(eng, I, S, G, w, theta, gamma), "SRS")
    release(I + S + Q)
    I, S = commit_sets(eng, ins, (3,)), commit_sets(eng, shs, (1, 2))
    fresh_ok(I, S)
    release(I + S)
    assert eng.rows_stats() == (0, 0)


def test_threads_and_a_racing_release(engines):
    lg, G, w = 12, 1, 3
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    ins, shs = rand_rows(3, T, 10100), rand_rows(3, T, 10200)
    I, S = commit_sets(eng, ins, (3,)), commit_sets(eng, shs, (2, 1))
    chal = {t: (1000 + t, 2000 + t) for t in range(4)}
    want = {}
    for t, (th, ga) in chal.items():
        zs, cl = sh_call(eng, I, S, G, w, th, ga)
        zs.release()
        want[t] = (zs.commitments[0], cl)
    assert len(set(want.values())) == 4
    errors = []

    def work(t):
        try:
            for _ in range(4):
                zs, cl = sh_call(eng, I, S, G, w, *chal[t])
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
        victim = commit_sets(eng, shs[2:], (1,))[0]
        out = []

        def call():
            try:
                zs, cl = sh_call(eng, I, [S[0], victim], G, w, *chal[0])
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
    release(I + S)
    assert eng.rows_stats() == before


def test_multi_handle_returns_the_context_bytes(hip):
    lib = _native.load()
    scale, ms = 12, 2
    T, M, ndev = 1 << (scale - ms), 1 << ms, 3
    tx, ty = 0xABCDEF0321, 0x13579BFD
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    devs = (ctypes.c_int * ndev)(0, 0, 0)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(ndev, devs, ctypes.byref(mh)) == 0
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        theta, gamma = be(21), be(22)
        u = T - 3
        tail = bt(tail_of(T, u, 17))
        idx = (ctypes.c_uint32 * 1)(1)
        c, cl, cc = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.create_string_buffer(96)
        made = {}
        for i in range(M):
            ins, shs = rand_rows(2, T, 1900 + i), rand_rows(2, T, 1950 + i)
            I, S = commit_sets(single, ins, (2,), i=i), commit_sets(single, shs, (2,), i=i)
            zs, want_cl = single.commit_shuffle(I, S, 1, 2, theta, gamma)
            zq, want_clq = single.commit_shuffle(I, S, 1, 2, theta, gamma, I, None, [1], u, tail)   # q' = input row 1
            release(I + S + [zs, zq])
            hi, hs, hz = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 2, b"".join(row_bytes(r) for r in ins), T, 1, cc, ctypes.byref(hi)) == 0
            assert lib.kzg_multi_rows_commit(mh, i, 2, b"".join(row_bytes(r) for r in shs), T, 1, cc, ctypes.byref(hs)) == 0
            ai, as_ = (ctypes.c_uint64 * 1)(hi.value), (ctypes.c_uint64 * 1)(hs.value)
            assert lib.kzg_multi_rows_commit_shuffle(mh, i, 1, ai, 1, as_, 1, 2, theta, gamma, None, c, cl, ctypes.byref(hz)) == 0, i
            assert (c.raw, cl.raw) == (zs.commitments[0], want_cl)
            made[i] = [hi.value, hs.value, hz.value]
            opts = _native.ShuffleOpts(1, ai, None, idx, u, b"".join(tail))
            assert lib.kzg_multi_rows_commit_shuffle(mh, i, 1, ai, 1, as_, 1, 2, theta, gamma, ctypes.byref(opts), c, cl,
                                                     ctypes.byref(hz)) == 0, i
            assert (c.raw, cl.raw) == (zq.commitments[0], want_clq)
            made[i].append(hz.value)
        # worker 3 shares worker 0's device, worker 1 lives elsewhere: both are refused under index 0
        for wrong in (3, 1):
            ai, as_ = (ctypes.c_uint64 * 1)(made[wrong][0]), (ctypes.c_uint64 * 1)(made[wrong][1])
            assert lib.kzg_multi_rows_commit_shuffle(mh, 0, 1, ai, 1, as_, 1, 2, theta, gamma, None, c, cl,
                                                     ctypes.byref(hz)) == _native.KZG_E_ARG
        for i in range(M):
            for hh in made[i]:
                assert lib.kzg_multi_rows_release(mh, i, hh) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)


def test_no_row_sized_copy_inside_the_call(engines):
    """structural: with stage profiling on, the call opens no upload span (only upload_fr opens KZG_T_DECODE), while the
    transforms, the factor kernels and the one MSM's accumulate all ran"""
    lg, G, w = 12, 2, 2
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    ins, shs, q = rand_rows(4, T, 11101), rand_rows(4, T, 11102), rand_rows(1, T, 11103)
    I, S, Q = commit_sets(eng, ins, (4,)), commit_sets(eng, shs, (4,)), commit_sets(eng, q, (1,))
    lib = _native.load()
    try:
        u = T - 3
        tail = tail_of(T, u, 111)
        kw = dict(Q=Q, input_sel=[0, None], shuffle_sel=[None, 0], usable=u, tail=tail)
        plain, plain_cl = sh_call(eng, I, S, G, w, 3, 4, **kw)
        plain.release()
        assert lib.kzg_set_profiling(eng._h, 1) == 0
        try:
            zs, cl = sh_call(eng, I, S, G, w, 3, 4, **kw)
            zs.release()
            tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
            assert lib.kzg_get_timings(eng._h, tms, len(tms)) == 0
        finally:
            assert lib.kzg_set_profiling(eng._h, 0) == 0
        t = dict(zip(_native.TIMING_NAMES, tms))
        print("shuffle stage times (ms):", {k: round(v, 4) for k, v in t.items()})
        assert t["decode"] == 0
        assert t["ntt"] > 0 and t["poly"] > 0 and t["accumulate"] > 0
        assert (zs.commitments[0], cl) == (plain.commitments[0], plain_cl)
    finally:
        release(I + S + Q)
    assert eng.rows_stats() == before


def test_the_argument_end_to_end_through_the_quotient(engines, srs_of):
    """rows a (2) | b (2) | q q' | A | L_0 | L_u | z: z from the new call, the relation from shuffle_quotient_terms plus
    (z - 1) L_0 and (z - 1) L_u, the quotient from the existing call with n_pieces < E, so that its shape check is live"""
    lg, G, w, ext_log, P = 10, 1, 2, 2, 3
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(121)
    theta, gamma, alpha = rnd.randrange(R), rnd.randrange(R), rnd.randrange(R)
    u = T - 4
    tail = tail_of(T, u, 122)
    fixed = [[int(t < u) for t in range(T)], [int(t == 0) for t in range(T)], [int(t == u) for t in range(T)]]
    a2, a3 = alpha * alpha % R, pow(alpha, 3, R)
    terms = [(int.from_bytes(c, "big"), fs) for c, fs in
             shuffle_quotient_terms(9, [0, 1], [2, 3], G, w, be(theta), be(gamma), be(alpha), 6, [4], [5], ext_log)]
    terms += [(a2, [(9, 0), (7, 0)]), (-a2 % R, [(7, 0)]), (a3, [(9, 0), (8, 0)]), (-a3 % R, [(8, 0)])]
    assert len(terms) <= _native.KZG_MAX_GATE_TERMS
    inst = sr.shuffle_instance(G, w, T, 123, usable=u, sel=True)
    for breakit in (False, True):
        ins, shs, qi, qs = sr.broken(*inst, seed=124) if breakit else inst
        z, closing = sr.shuffle_product(ins, shs, G, w, theta, gamma, qi, qs, u, tail)
        assert (closing == 1) != breakit
        sets = commit_sets(eng, ins + shs + qi + qs + fixed, (2, 2, 2, 3))
        try:
            zset, cl = sh_call(eng, sets[:1], sets[1:2], G, w, theta, gamma, sets[2:3], [0], [1], u, tail)
            try:
                assert cl == be(closing)
                assert zset.commitments[0] == oc.commit(srs, row_bytes(z), True)
                call = lambda: eng.commit_quotient_ext(sets + [zset], [(be(c), fs) for c, fs in terms], None, None, ext_log, P)  # noqa: E731
                if breakit:
                    arg_error(call)
                else:
                    want = reference_pieces_ext(ins + shs + qi + qs + fixed + [z], terms, None, None, ext_log, P)
                    tset = call()
                    try:
                        check_pieces(eng, srs, tset, want, rnd)
                    finally:
                        tset.release()
            finally:
                zset.release()
        finally:
            release(sets)
    assert eng.rows_stats() == before
