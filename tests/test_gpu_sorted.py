"""GPU tests (`-m gpu`) of kzg_rows_commit_sorted: the columns of committed sets, stably sorted as tuples on the device.  The
expected rows come from the definition in Python integers (tests/sorted_ref.py) and are committed with the C oracle, never with
the library under test.  Every case compares three things against the oracle: the w commitments byte for byte, the values at
probe indices through eval_rows, and the value at one random point.  Row lengths 1, 2, 2^6, 2^10 and 2^13 (4 and 32 for the
smallest `usable`); the per-pass kernels take tiles of 2048 positions, so 2^13 spans four tiles and `usable` gives the lengths
that end inside a tile.  Not exercised on the device: the T > 2^27 refusal, which needs an 8 GB row set.  Each test leaves
rows_stats() where it found it."""
import ctypes
import random
import threading

import pytest

from oracle import cpu as oc
from tests import grand_product_ref as gp
from tests import sorted_ref as sref
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release, srs_cache, tail_of
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x5027ED01, 0x5027ED02
TILE = 2048


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def probes_of(T, rnd, usable=None):
    """the ends, the tile borders, the rows around `usable` and three random rows"""
    ps = {0, 1 % T, T - 1} | {rnd.randrange(T) for _ in range(3)}
    ps |= {t for b in range(TILE, T, TILE) for t in (b - 1, b)}
    if usable is not None:
        ps |= {max(usable - 1, 0), usable, min(usable + 1, T - 1)}
    return sorted(ps)


def check_set(eng, srs, rset, want, rnd, probes, i=0):
    """the w-row set `rset` against its expected evaluation rows `want` (integers)"""
    w, T = len(want), len(want[0])
    assert (rset.k, rset.i, rset.T, len(rset.commitments)) == (w, i, T, w)
    wb = [row_bytes(r) for r in want]
    for c in range(w):
        assert rset.commitments[c] == oc.commit(srs, wb[c], True), c
    om = gp.omega(T)
    ts = sorted(set(probes))
    for t0 in range(0, len(ts), 4):
        part = ts[t0:t0 + 4]
        Y = eng.eval_rows([rset], [be(pow(om, t, R)) for t in part], [list(range(w))] * len(part))
        for t, ys in zip(part, Y):
            assert ys == [be(want[c][t]) for c in range(w)], t
    x = be(rnd.randrange(R))
    assert eng.eval_rows([rset], [x], [list(range(w))])[0] == [oc.fr_eval(oc.fr_ntt(b, True), x) for b in wb]


def run(eng, srs, cols, rnd, n_keys=None, usable=None, tail=(), sizes=None, ef=True, probes=None):
    """commit `cols`, sort them on the device, check the new set against the reference; returns the expected rows"""
    w, T = len(cols), len(cols[0])
    want, _ = sref.sorted_columns(cols, n_keys, usable, tail)
    S = commit_sets(eng, cols, sizes or (w,), ef)
    try:
        out = eng.commit_sorted(S, w, n_keys, usable, bt(tail))
        try:
            check_set(eng, srs, out, want, rnd, probes or probes_of(T, rnd, usable))
        finally:
            out.release()
    finally:
        release(S)
    return want


def rand_col(T, rnd, bound=R):
    return [rnd.randrange(bound) for _ in range(T)]


# ---------------------------------------------------------------------------------------------------- keys
@pytest.mark.parametrize("lg,w,n_keys", [(0, 1, 1), (1, 1, 1), (6, 1, 1), (10, 1, 1), (13, 1, 1), (1, 3, 3), (6, 3, 3), (10, 3, 3),
                                         (13, 3, 3), (6, 16, 16)])
def test_uniform_255_bit_keys(engines, srs_of, lg, w, n_keys):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(100 * lg + w)
    run(eng, srs, [rand_col(T, rnd) for _ in range(w)], rnd, n_keys)
    assert eng.rows_stats() == before


@pytest.mark.parametrize("lg,bits", [(10, 8), (10, 16), (13, 8), (13, 16)])
def test_small_keys_take_the_skipped_pass_path(engines, srs_of, lg, bits):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(200 * lg + bits)
    run(eng, srs, [rand_col(T, rnd, 1 << bits)], rnd)
    run(eng, srs, [rand_col(T, rnd, 1 << bits), list(range(T)), rand_col(T, rnd)], rnd, 1)      # with the source row as payload
    assert eng.rows_stats() == before


@pytest.mark.parametrize("lg", [10, 13])
def test_heavy_duplicates_are_sorted_stably(engines, srs_of, lg):
    """w = 3, n_keys = 2, the payload is the source row: an unstable scatter fails"""
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(300 + lg)
    want = run(eng, srs, [rand_col(T, rnd, 4), rand_col(T, rnd, 3), list(range(T))], rnd, 2)
    for t in range(T - 1):
        if (want[0][t], want[1][t]) == (want[0][t + 1], want[1][t + 1]):
            assert want[2][t] < want[2][t + 1]
    # the same keys at the top of the field: the duplicates differ from each other only in the last passes
    big = [R - 1 - v for v in range(4)]
    run(eng, srs, [[big[rnd.randrange(4)] for _ in range(T)], rand_col(T, rnd, 3), list(range(T))], rnd, 2)
    assert eng.rows_stats() == before


def test_column_one_decides_only_among_equal_column_zero(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(400)
    heads = [rnd.randrange(R) for _ in range(5)]
    cols = [[heads[rnd.randrange(5)] for _ in range(T)], rand_col(T, rnd)]
    want = run(eng, srs, cols, rnd, 2)
    assert want[0] == sorted(cols[0]) and want[1] != sorted(cols[1])
    assert run(eng, srs, cols, rnd, 1)[1] != want[1]                                             # as a payload it keeps the source order
    assert eng.rows_stats() == before


def test_word_and_byte_order(engines, srs_of):
    """column 0 holds values that differ only in the top byte, only in the lowest byte, or only in one middle 32-bit word, and
    the values around every word border; column 1 is the source row"""
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(500)
    base = rnd.randrange(1 << 248) & ~(0xFF | (0xFFFFFFFF << 96))
    vals = [0, 1, R - 1] + [v for j in range(1, 8) for v in ((1 << (32 * j)) - 1, 1 << (32 * j))]
    vals += [base + (k << 248) for k in range(0x73)]                                             # the top byte alone (all below r)
    vals += [base + k for k in range(256)]                                                       # the lowest byte alone
    vals += [base + (rnd.randrange(1 << 32) << 96) for _ in range(300)]                          # one middle word alone
    assert len(vals) <= T and max(vals) < R
    vals += [vals[rnd.randrange(len(vals))] for _ in range(T - len(vals))]
    rnd.shuffle(vals)
    want = run(eng, srs, [vals, list(range(T))], rnd, 1, probes=range(0, T, 7))
    assert want[0] == sorted(vals)
    eng6, srs6 = engines(6), srs_of(6)
    run(eng6, srs6, [vals[:64], list(range(64))], rnd, 1, probes=range(64))
    assert eng.rows_stats() == before


@pytest.mark.parametrize("lg", [6, 13])
def test_fixed_patterns(engines, srs_of, lg):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(600 + lg)
    step, rows = R // T, list(range(T))
    for col in ([R - 1] * T, [0] * T, [t * step for t in rows], [(T - 1 - t) * step for t in rows], [T - 1 - t for t in rows]):
        want = run(eng, srs, [col, rows], rnd, 1)
        assert want[0] == sorted(col)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- layouts
def test_input_layouts(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(700)
    cols = [rand_col(T, rnd, 1 << 12), rand_col(T, rnd), rand_col(T, rnd, 7)]
    for ef in (True, False):                                       # evaluation form and coefficient form, two sets
        run(eng, srs, cols, rnd, 2, sizes=(1, 2), ef=ef)
    run(eng, srs, cols, rnd, 3, sizes=(2, 1))
    # a handle named twice: two equal columns
    S = commit_sets(eng, cols[:1], (1,))
    try:
        out = eng.commit_sorted([S[0], S[0]], 2)
        try:
            check_set(eng, srs, out, [sorted(cols[0])] * 2, rnd, probes_of(T, rnd))
        finally:
            out.release()
    finally:
        release(S)
    assert eng.rows_stats() == before


@pytest.mark.parametrize("lg", [2, 5, 6, 10])
def test_usable_layout(engines, srs_of, lg):
    """usable in {1, 2, T - 32, T - 1}.  The source rows behind `usable` hold zeros, which would sort first if they were read;
    the tails are checked in place.  T - usable <= KZG_MAX_BLIND_ROWS is part of the call's contract, so usable = 1 and 2 sort
    one and two rows at T = 4 and 32 and are the KZG_MAX_BLIND_ROWS refusal at 2^6 and 2^10."""
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(800 + lg)
    for u in sorted({1, 2, max(T - 32, 1), T - 1}):
        cols = [[1 + v for v in rand_col(u, rnd, 1 << 20)] + [0] * (T - u), rand_col(u, rnd) + [0] * (T - u)]
        tail = rand_col(2 * (T - u), rnd)
        if T - u > _native.KZG_MAX_BLIND_ROWS:
            S = commit_sets(eng, cols, (2,))
            arg_error(lambda: eng.commit_sorted(S, 2, 1, u, bt(tail)), "KZG_MAX_BLIND_ROWS")
            release(S)
            continue
        probes = set(probes_of(T, rnd, u)) | set(range(u, T))
        want = run(eng, srs, cols, rnd, 1, u, tail, probes=probes)
        assert want[0][u:] == tail[:T - u] and want[1][u:] == tail[T - u:] and 0 not in want[0][:u]
    assert eng.rows_stats() == before


def test_usable_ends_inside_a_tile(engines, srs_of):
    lg = 13
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(900)
    u = T - 21                                                     # three full tiles and a partial one
    cols = [rand_col(T, rnd, 1 << 16), list(range(T))]
    run(eng, srs, cols, rnd, 1, u, rand_col(2 * (T - u), rnd))
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg, w = 6, 3
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    srs = oc.srs_gen(be(SEED_X), be(SEED_Y), lg + 1, 1, 0)
    rnd = random.Random(1000)
    cols = [rand_col(T, rnd, 9), rand_col(T, rnd), rand_col(T, rnd)]
    want, _ = sref.sorted_columns(cols, 2)
    want_c = [oc.commit(srs, row_bytes(r), True) for r in want]

    def fresh_ok(sets):
        out = eng.commit_sorted(sets, w, 2)
        out.release()
        assert out.commitments == want_c

    I = commit_sets(eng, cols, (1, 2))
    fresh_ok(I)
    live = eng.rows_stats()
    lib = _native.load()
    E_ARG = _native.KZG_E_ARG
    hi = (ctypes.c_uint64 * 2)(I[0].handle, I[1].handle)
    c, h = ctypes.create_string_buffer(48 * 16), ctypes.c_uint64(0)

    def raw(width, n_keys, opts=None, n=2):
        return lib.kzg_rows_commit_sorted(eng._h, n, hi, width, n_keys, ctypes.byref(opts) if opts else None, c, ctypes.byref(h))

    def refused(rc, why):
        assert rc == E_ARG and why in lib.kzg_last_error(eng._h), (rc, lib.kzg_last_error(eng._h))

    # shapes
    refused(raw(0, 1), b"width must be in")
    refused(raw(17, 1), b"width must be in")
    refused(raw(3, 0), b"n_keys must be in")
    refused(raw(3, 4), b"n_keys must be in")
    refused(raw(3, 1, n=0), b"number of handles")
    refused(raw(3, 1, n=17), b"number of handles")
    refused(raw(2, 1), b"exactly width rows")                      # 3 rows, width 2
    arg_error(lambda: eng.commit_sorted(I[:1], 3, 1), "exactly width rows")
    arg_error(lambda: eng.commit_sorted(I * 6, 16), "KZG_MAX_BATCH_OPEN rows")    # 18 rows
    # the layout
    tl = b"".join(bt(rand_col(3 * 4, rnd)))
    big = R.to_bytes(32, "big")
    for usable, tail, why in ((T, tl, b"usable must be in"), (2 ** 40, tl, b"usable must be in"),
                              (T - 33, tl, b"KZG_MAX_BLIND_ROWS"), (T - 4, None, b"tail_be32 must be given"),
                              (0, tl, b"plain layout"), (T - 4, tl[:-32] + big, b"canonical"),
                              (T - 4, b"\xff" * 32 + tl[32:], b"canonical")):
        refused(raw(3, 1, _native.SortedOpts(usable, tail)), why)
    arg_error(lambda: eng.commit_sorted(I, w, 1, 0), "usable")
    arg_error(lambda: eng.commit_sorted(I, w, 1, T - 4, [be(1)] * 11), "exactly")
    arg_error(lambda: eng.commit_sorted(I, w, 1, None, [be(1)]), "tail needs usable")
    assert raw(3, 1, _native.SortedOpts(0, None)) == 0             # usable = 0 spelled out: the plain layout
    eng.release_rows(h.value)
    assert eng.rows_stats() == live
    # handles
    other = commit_sets(eng, cols[1:], (2,), i=1)                  # another worker
    arg_error(lambda: eng.commit_sorted([I[0]] + other, w), "one worker")
    short = eng.commit_rows(0, [row_bytes(r[:T // 2]) for r in cols[1:]])      # another length
    arg_error(lambda: eng.commit_sorted([I[0], short], w), "one worker and have one row length")
    release(other + [short])
    gone = commit_sets(eng, cols[1:], (2,))
    release(gone)
    arg_error(lambda: eng.commit_sorted([I[0]] + gone, w), "released")
    arg_error(lambda: eng.commit_sorted([2 ** 40], 1), "unknown")
    fresh_ok(I)
    # the 65th live set
    fill = [eng.commit_rows(0, [row_bytes(cols[0])]) for _ in range(_native.KZG_MAX_ROW_SETS - 2)]
    assert eng.rows_stats()[0] == _native.KZG_MAX_ROW_SETS
    arg_error(lambda: eng.commit_sorted(I, w, 2), "KZG_MAX_ROW_SETS", code=_native.KZG_E_BUSY)
    fill.pop().release()
    fresh_ok(I)
    release(fill)
    # stale after an SRS load
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.commit_sorted(I, w, 2), "SRS")
    release(I)
    I = commit_sets(eng, cols, (3,))
    out = eng.commit_sorted(I, w, 2)
    assert out.commitments == want_c
    # the new set goes stale and releases like any other
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.eval_rows([out], [be(3)], [[0]]), "SRS")
    release(I + [out])
    arg_error(lambda: eng.release_rows(out.handle))
    assert eng.rows_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------------- the argument
@pytest.mark.parametrize("usable", [None, (1 << 10) - 5])
def test_the_sorted_set_closes_the_shuffle_over_its_inputs(engines, usable):
    lg, w = 10, 3
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(1100)
    cols = [rand_col(T, rnd, 50), rand_col(T, rnd, 1 << 30), rand_col(T, rnd)]
    n = T if usable is None else usable
    tail = rand_col(w * (T - n), rnd)
    theta, gamma = be(rnd.randrange(R)), be(rnd.randrange(R))
    ztail = bt(tail_of(T, usable, 1101))
    I = commit_sets(eng, cols, (1, 2))
    try:
        S = eng.commit_sorted(I, w, 2, usable, bt(tail))
        try:
            z, closing = eng.commit_shuffle(I, [S], 1, w, theta, gamma, usable=usable, tail=ztail)
            z.release()
            assert closing == be(1)
            # one output value perturbed, through a separately committed set: the product no longer closes
            want, _ = sref.sorted_columns(cols, 2, usable, tail)
            want[1][n // 2] = (want[1][n // 2] + 1) % R
            B = commit_sets(eng, want, (w,))
            try:
                z, closing = eng.commit_shuffle(I, B, 1, w, theta, gamma, usable=usable, tail=ztail)
                z.release()
                assert closing != be(1)
            finally:
                release(B)
        finally:
            S.release()
    finally:
        release(I)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- routing and threads
def test_multi_handle_and_multi_device_client_return_the_context_bytes(hip):
    from zkp_subnet_amd import MultiDeviceClient, codec
    from zkp_subnet_amd.engine import lagrange_factor

    lib = _native.load()
    scale, ms = 8, 1
    T, M = 1 << (scale - ms), 1 << ms
    tx, ty = 0xABCDEF0777, 0x13579BF7
    rnd = random.Random(1200)
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(1, (ctypes.c_int * 1)(0), ctypes.byref(mh)) == 0
    u = T - 3
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        c, cc = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
        made = {}
        for i in range(M):
            cols = [rand_col(T, rnd, 300), rand_col(T, rnd)]
            tail = b"".join(bt(rand_col(2 * (T - u), rnd)))
            I = commit_sets(single, cols, (2,), i=i)
            plain = single.commit_sorted(I, 2, 1)
            lay = single.commit_sorted(I, 2, 1, u, [tail[j:j + 32] for j in range(0, len(tail), 32)])
            release(I + [plain, lay])
            hi, hz = ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 2, b"".join(row_bytes(r) for r in cols), T, 1, cc, ctypes.byref(hi)) == 0
            ai = (ctypes.c_uint64 * 1)(hi.value)
            assert lib.kzg_multi_rows_commit_sorted(mh, i, 1, ai, 2, 1, None, c, ctypes.byref(hz)) == 0, i
            assert c.raw == b"".join(plain.commitments)
            made[i] = [hi.value, hz.value]
            opts = _native.SortedOpts(u, tail)
            assert lib.kzg_multi_rows_commit_sorted(mh, i, 1, ai, 2, 1, ctypes.byref(opts), c, ctypes.byref(hz)) == 0, i
            assert c.raw == b"".join(lay.commitments)
            made[i].append(hz.value)
        ai = (ctypes.c_uint64 * 1)(made[1][0])                     # worker 1's set under index 0
        assert lib.kzg_multi_rows_commit_sorted(mh, 0, 1, ai, 2, 1, None, c, ctypes.byref(hz)) == _native.KZG_E_ARG
        for i in range(M):
            for hh in made[i]:
                assert lib.kzg_multi_rows_release(mh, i, hh) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)
    single.close()

    multi = MultiDeviceClient(devices=[0], seed=78)
    multi.start(scale=scale, machines_scale=ms)
    try:
        fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
        for i in range(M):
            cols = [rand_col(T, rnd, 300), rand_col(T, rnd)]
            tail = rand_col(2 * (T - u), rnd)
            a = multi.worker_commit_rows(i, [fr(col) for col in cols]).json()["handle"]
            for usable, tl in ((None, []), (u, tail)):
                want, _ = sref.sorted_columns(cols, 1, usable, tl)
                ref = multi.worker_commit_rows(i, [fr(col) for col in want]).json()
                r = multi.worker_commit_sorted([a], 2, 1, usable, fr(tl))
                assert r.status_code == 200, r.json()
                assert r.json()["commitments"] == ref["commitments"]
                for hh in (ref["handle"], r.json()["handle"]):
                    assert multi.worker_release_rows(hh).status_code == 200
            assert multi.worker_release_rows(a).status_code == 200
            assert multi.worker_commit_sorted([a], 2, 1).status_code == 400
    finally:
        multi.stop()


def test_two_threads_on_one_context_give_the_serial_bytes(engines):
    lg = 10
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(1300)
    jobs = [([rand_col(T, rnd, 1 << 16), rand_col(T, rnd)], 1), ([rand_col(T, rnd), rand_col(T, rnd, 5), rand_col(T, rnd)], 3)]
    sets = [commit_sets(eng, cols, (len(cols),)) for cols, _ in jobs]
    want = []
    for S, (cols, nk) in zip(sets, jobs):
        out = eng.commit_sorted(S, len(cols), nk)
        out.release()
        want.append(out.commitments)
    assert want[0] != want[1][:2]
    errors = []

    def work(j):
        try:
            for _ in range(4):
                out = eng.commit_sorted(sets[j], len(jobs[j][0]), jobs[j][1])
                out.release()
                assert out.commitments == want[j]
        except Exception as ex:   # noqa: BLE001
            errors.append(repr(ex))

    ths = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for x in ths:
        x.start()
    for x in ths:
        x.join()
    assert not errors, errors
    for S in sets:
        release(S)
    assert eng.rows_stats() == before
