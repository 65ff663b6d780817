"""GPU tests (`-m gpu`) of the SHPLONK opening on committed row sets: kzg_rows_commit_shplonk's W, the new set's evaluations,
the finish's v and pi against the Python reference (tests/shplonk_ref.py, T <= 2^12) byte for byte; the identity
h(x) = sum_j c_j (f_j(x) - r_j(x)) / Z_{S_j}(x) from eval_rows alone at every row length where the division kernels change
shape; the one-group case against kzg_rows_open; errors answer KZG_E_ARG and leave the context serving; no upload inside
round A; threads and the multi-GPU handle return the same bytes.  Every comparison is bit-exact."""
import ctypes
import random
import threading

import pytest

from oracle import cpu as oc
from tests import shplonk_ref as ref
from tests.gpu_common import R, be, rand_scalars_bytes, val as ib
from tests.gpu_rows import arg_error, commit_sets, engine_cache, release, split_halves as split, srs_cache
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import _root_of_unity, lagrange_factor

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x5A9107, 0x5A9108
INF = bytes([0xC0]) + bytes(47)

# more than four groups (a second batch on the device): six rows, six different point sets over three points
SIX = (6, [[0, 3, 4, 5], [1, 3, 5], [2, 4, 5]])
# the special rows of the byte test: rows 0-2 at {0}, 3-4 at {0,1}, 5-6 at {0,1,2}, 7 at {0,3}
SPECIAL = (8, [[0, 1, 2, 3, 4, 5, 6, 7], [3, 4, 5, 6], [5, 6], [7]])


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


oracle_srs = srs_cache(SEED_X, SEED_Y)


def points_for(rnd, T, m, special=False):
    w = _root_of_unity(T)
    zeta = rnd.randrange(1, R)
    pts = [zeta * pow(w, p, R) % R for p in range(m)]
    if special:
        pts[0], pts[1] = 0, pow(w, 3, R)             # alpha = 0 and alpha a T-th root of unity
    return pts


def pick_u(rnd, pts):
    u = rnd.randrange(R)
    while u in pts:
        u = rnd.randrange(R)
    return u


def eval_many(eng, sets, pts, opened):
    """eval_rows for any number of points (four per call; a point that opens nothing is skipped), as ints"""
    out = [[] for _ in pts]
    live = [p for p in range(len(pts)) if opened[p]]
    for o in range(0, len(live), 4):
        ps = live[o:o + 4]
        for p, ys in zip(ps, eng.eval_rows(sets, [be(pts[p]) for p in ps], [opened[p] for p in ps])):
            out[p] = [ib(y) for y in ys]
    return out


def shplonk(eng, sets, pts, opened, c, u):
    W, hs = eng.commit_shplonk(sets, [be(a) for a in pts], opened, [be(x) for x in c])
    v, pi = eng.open_shplonk_finish(sets, hs, [be(a) for a in pts], opened, [be(x) for x in c], be(u))
    return W, hs, v, pi


def verify(eng, sets, pts, opened, c, evals, W, u, pi):
    comms = [x for s in sets for x in s.commitments]
    return eng.verify_open_shplonk(0, comms, [be(a) for a in pts], opened, [be(x) for x in c],
                                   [[be(y) for y in ev] for ev in evals], W, be(u), pi)


# ------------------------------------------------------------------------------------- 1. bytes against the reference
CASES = [(lg, name, ef) for lg in (4, 10) for name in list(ref.SHAPES) + ["special", "zero"] for ef in (True, False)] + \
        [(12, "special", True), (12, "special", False), (12, "eight", True), (12, "six", False)]


@pytest.mark.parametrize("lg,name,ef", CASES)
def test_bytes_against_the_reference(engines, lg, name, ef):
    eng, T = engines(lg), 1 << lg
    rnd = random.Random(1000 * lg + len(name) + ef)
    k, opened = {"special": SPECIAL, "zero": ref.SHAPES["three"], "six": SIX}.get(name) or ref.SHAPES[name]
    rows = [rand_scalars_bytes(T, 7000 + 100 * lg + j) for j in range(k)]
    c = [rnd.randrange(1, R) for _ in range(k)]
    if name == "special":
        rows[1] = bytes(32 * T)                      # a zero row
        rows[2] = rows[0]                            # a duplicated row
        c[0] = 0                                     # a row left out
        rows[4], c[4] = rows[3], R - c[3]            # the group {0, 1} cancels to the zero polynomial
    if name == "zero":
        rows = [bytes(32 * T)] * k                   # every row zero: W is the point at infinity
    pts = points_for(rnd, T, len(opened), special=(name == "special"))
    u = pick_u(rnd, pts)
    F = [ref.coeffs_of(r, ef) for r in rows]
    srs = oracle_srs(lg)
    h = ref.h_poly(F, pts, opened, c)
    sets = commit_sets(eng, rows, split(k), ef)
    try:
        W, hs, v, pi = shplonk(eng, sets, pts, opened, c, u)
        try:
            assert W == oc.commit(srs, ref.row_bytes(h), False) == hs.commitments[0]
            if name == "zero":
                assert W == INF
            xs = [rnd.randrange(R), rnd.randrange(R)]
            assert eng.eval_rows([hs], [be(x) for x in xs], [[0], [0]]) == \
                [[oc.fr_eval(ref.row_bytes(h), be(x))] for x in xs]
            evals = eval_many(eng, sets, pts, opened)
            assert evals == ref.evaluations(F, pts, opened)
            assert v == be(ref.value_v(pts, opened, c, evals, u))
            L = ref.combine(F + [h], ref.finish_coeffs(pts, opened, c, u))
            assert (v, pi) == oc.open_(srs, ref.row_bytes(L), be(u), False)
            assert verify(eng, sets, pts, opened, c, evals, W, u, pi)
            assert not verify(eng, sets, pts, opened, c, evals, W[:47] + bytes([W[47] ^ 1]), u, pi)
        finally:
            hs.release()
    finally:
        release(sets)
    assert eng.rows_stats() == (0, 0)


# ------------------------------------------------------------------------------------- 2. the identity at every T
@pytest.mark.parametrize("lg,shape", [(4, "six"), (10, "six"), (12, "six"), (13, "six"), (14, "six"), (18, "six"),
                                      (13, "eight"), (14, "three")])
def test_identity_from_eval_rows(engines, lg, shape):
    """no Python polynomial arithmetic: h(x) and v are rebuilt from eval_rows of the source rows"""
    eng, T = engines(lg), 1 << lg
    rnd = random.Random(31 * lg + len(shape))
    k, opened = SIX if shape == "six" else ref.SHAPES[shape]
    rows = [rand_scalars_bytes(T, 9000 + 100 * lg + j) for j in range(k)]
    c = [rnd.randrange(1, R) for _ in range(k)]
    pts = points_for(rnd, T, len(opened))
    u, x = pick_u(rnd, pts), pick_u(rnd, pts)
    S = ref.point_sets(k, opened)
    sets = commit_sets(eng, rows, split(k), False)
    try:
        W, hs, v, pi = shplonk(eng, sets, pts, opened, c, u)
        try:
            evals = eval_many(eng, sets, pts, opened)
            fx = eval_many(eng, sets, [x], [list(range(k))])[0]
            want = 0
            for j in range(k):
                xs = [pts[p] for p in S[j]]
                ys = [evals[p][opened[p].index(j)] for p in S[j]]
                z = 1
                for a in xs:
                    z = z * (x - a) % R
                want = (want + c[j] * (fx[j] - ref.interpolant_at(xs, ys, x)) * pow(z, -1, R)) % R
            assert eng.eval_rows([hs], [be(x)], [[0]]) == [[be(want)]]
            assert v == be(ref.value_v(pts, opened, c, evals, u))
            assert verify(eng, sets, pts, opened, c, evals, W, u, pi)
        finally:
            hs.release()
    finally:
        release(sets)
    assert eng.rows_stats() == (0, 0)


# ------------------------------------------------------------------------------------- 3. against kzg_rows_open
@pytest.mark.parametrize("lg", [10, 14])
def test_one_group_with_gamma_powers_is_the_gwc_proof(engines, lg):
    eng, T = engines(lg), 1 << lg
    rnd = random.Random(lg)
    k = 5
    rows = [rand_scalars_bytes(T, 300 + j) for j in range(k)]
    a, g = rnd.randrange(R), rnd.randrange(R)
    c = [pow(g, j, R) for j in range(k)]
    sets = commit_sets(eng, rows, (2, 3))
    try:
        ys, proofs = eng.open_rows(sets, [be(a)], [list(range(k))], [be(g)])
        u = pick_u(rnd, [a])
        W, hs, v, pi = shplonk(eng, sets, [a], [list(range(k))], c, u)
        try:
            assert W == proofs[0]
            assert verify(eng, sets, [a], [list(range(k))], c, [[ib(y) for y in ys[0]]], W, u, pi)
        finally:
            hs.release()
        # m = 1: a second group would be rows opened nowhere
        with pytest.raises(KzgError) as ei:
            eng.commit_shplonk(sets, [be(a)], [[0, 1, 2]], [be(x) for x in c])
        assert ei.value.code == _native.KZG_E_ARG and "no point" in str(ei.value)
        # a repeated handle numbers its rows twice: the same bytes as two sets holding the same rows
        copy = eng.commit_rows(0, rows[2:], True)
        try:
            opened, cc = [[0, 1, 2, 3, 4, 5], [1, 4]], [rnd.randrange(1, R) for _ in range(6)]
            P = [be(a), be(a + 1)]
            W1, h1 = eng.commit_shplonk([sets[1], sets[1]], P, opened, [be(x) for x in cc])
            W2, h2 = eng.commit_shplonk([sets[1], copy], P, opened, [be(x) for x in cc])
            release([h1, h2])
            assert W1 == W2
        finally:
            copy.release()
    finally:
        release(sets)
    assert eng.rows_stats() == (0, 0)


# ------------------------------------------------------------------------------------- 4. errors
def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 4
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    rows = [rand_scalars_bytes(T, 4040 + j) for j in range(4)]
    P = [be(11), be(12)]
    opened, C = [[0, 1, 2, 3], [3]], [be(5), be(6), be(0), be(7)]
    big = R.to_bytes(32, "big")
    lib = _native.load()
    rs = eng.commit_rows(0, rows)
    want, hs = eng.commit_shplonk([rs], P, opened, C)
    hs.release()

    def good():
        w, h = eng.commit_shplonk([rs], P, opened, C)
        h.release()
        assert w == want and eng.rows_stats()[0] == 1

    def raw(k, m, masks, pts=b"".join(P), cf=b"".join(C)):
        c48, h = ctypes.create_string_buffer(48), ctypes.c_uint64(0)
        hsv = (ctypes.c_uint64 * 1)(rs.handle)
        rc = lib.kzg_rows_commit_shplonk(eng._h, 1, hsv, k, m, pts, (ctypes.c_uint32 * 9)(*masks), cf, c48, ctypes.byref(h))
        return rc, lib.kzg_last_error(eng._h).decode()

    for args, needle in (((3, 2, [7, 4]), "k must equal"), ((0, 2, [0, 0]), "KZG_MAX_SHPLONK_ROWS"),
                         ((16, 2, [1, 1], b"".join(P), be(1) * 16), "KZG_MAX_SHPLONK_ROWS"),
                         ((4, 0, [0]), "KZG_MAX_SHPLONK_POINTS"), ((4, 9, [15] * 9, be(1) * 9), "KZG_MAX_SHPLONK_POINTS"),
                         ((4, 2, [15, 8], P[0] + big), "canonical"), ((4, 2, [15, 8], b"".join(P), C[0] + big + C[2] + C[3]), "canonical"),
                         ((4, 2, [15, 8], P[0] + P[0]), "distinct"), ((4, 2, [15, 16]), "row >= k"),
                         ((4, 2, [7, 0]), "no point"), ((4, 2, [15, 8], b"".join(P), be(0) * 4), "zero")):
        rc, msg = raw(*args)
        assert rc == _native.KZG_E_ARG and needle in msg, (args[:3], rc, msg)
        good()
    # |S_j| >= T: a four-coefficient row opened at four points
    small = hip()
    small.gen_srs(SEED_X, SEED_Y, 2, 0)
    with small.commit_rows(0, [rand_scalars_bytes(4, 1)], False) as tiny:
        arg_error(lambda: small.commit_shplonk([tiny], [be(1), be(2), be(3), be(4)], [[0]] * 4, [be(1)]), "T or more")
        w, h = small.commit_shplonk([tiny], [be(1), be(2), be(3)], [[0]] * 3, [be(1)])   # three points: a constant h
        h.release()
    # handles: released, another worker, mixed workers
    gone = eng.commit_rows(0, rows)
    gone.release()
    arg_error(lambda: eng.commit_shplonk([gone], P, opened, C), "released")
    good()
    with eng.commit_rows(1, rows[:2]) as other:
        arg_error(lambda: eng.commit_shplonk([rs, other], P, [[0, 1, 2, 3, 4, 5], [3]], C + [be(1), be(2)]), "one worker")
    good()
    # KZG_E_BUSY at the 65th set
    held = [eng.commit_rows(0, rows[:1]) for _ in range(_native.KZG_MAX_ROW_SETS - 1)]
    with pytest.raises(KzgError) as ei:
        eng.commit_shplonk([rs], P, opened, C)
    assert ei.value.code == _native.KZG_E_BUSY
    release(held)
    good()
    # a source set made stale by an SRS load
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.commit_shplonk([rs], P, opened, C), "SRS")
    rs.release()
    rs = eng.commit_rows(0, rows)
    good()
    rs.release()
    assert eng.rows_stats() == (0, 0)


# ------------------------------------------------------------------------------------- 5. structure and threads
def test_no_row_sized_copy_inside_round_a(engines):
    """structural: with stage profiling on, round A opens no upload span (only upload_fr opens KZG_T_DECODE) and no
    transform, while the division kernels and the one MSM's accumulate ran"""
    lg = 12
    eng, T = engines(lg), 1 << lg
    k, opened = SIX
    rows = [rand_scalars_bytes(T, 1100 + j) for j in range(k)]
    P, C = [be(21 + p) for p in range(3)], [be(31 + j) for j in range(k)]
    sets = commit_sets(eng, rows, (k,), False)
    lib = _native.load()
    try:
        plain, hp = eng.commit_shplonk(sets, P, opened, C)
        hp.release()
        assert lib.kzg_set_profiling(eng._h, 1) == 0
        try:
            W, hs = eng.commit_shplonk(sets, P, opened, C)
            hs.release()
            tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
            assert lib.kzg_get_timings(eng._h, tms, len(tms)) == 0
        finally:
            assert lib.kzg_set_profiling(eng._h, 0) == 0
        t = dict(zip(_native.TIMING_NAMES, tms))
        print("shplonk round A stage times (ms):", {n: round(v, 4) for n, v in t.items()})
        assert t["decode"] == 0 and t["ntt"] == 0
        assert t["poly"] > 0 and t["accumulate"] > 0
        assert W == plain
    finally:
        release(sets)
    assert eng.rows_stats() == (0, 0)


def test_threads_on_shared_sets_return_identical_bytes(engines):
    lg = 10
    eng, T = engines(lg), 1 << lg
    k, opened = SIX
    rows = [rand_scalars_bytes(T, 8100 + j) for j in range(k)]
    P, C, u = [be(41 + p) for p in range(3)], [be(51 + j) for j in range(k)], be(99)
    sets = commit_sets(eng, rows, (2, 4))
    try:
        W, hs = eng.commit_shplonk(sets, P, opened, C)
        want = (W,) + eng.open_shplonk_finish(sets, hs, P, opened, C, u)
        hs.release()
        errors = []

        def work():
            try:
                for _ in range(4):
                    w, h = eng.commit_shplonk(sets, P, opened, C)
                    try:
                        assert (w,) + eng.open_shplonk_finish(sets, h, P, opened, C, u) == want
                    finally:
                        h.release()
            except Exception as ex:   # noqa: BLE001
                errors.append(repr(ex))

        ths = [threading.Thread(target=work) for _ in range(4)]
        for x in ths:
            x.start()
        for x in ths:
            x.join()
        assert not errors, errors
    finally:
        release(sets)
    assert eng.rows_stats() == (0, 0)


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
        pts, cfs = be(61) + be(62), b"".join(be(71 + j) for j in range(3))
        masks = (ctypes.c_uint32 * 2)(7, 2)
        c, cc = ctypes.create_string_buffer(48), ctypes.create_string_buffer(48 * 3)
        made = {}
        for i in range(M):
            rows = [rand_scalars_bytes(T, 900 + 10 * i + j) for j in range(3)]
            with single.commit_rows(i, rows) as rs:
                want, hs = single.commit_shplonk([rs], [be(61), be(62)], [[0, 1, 2], [1]], [be(71 + j) for j in range(3)])
                hs.release()
            h, hz = ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 3, b"".join(rows), T, 1, cc, ctypes.byref(h)) == 0
            ha = (ctypes.c_uint64 * 1)(h.value)
            assert lib.kzg_multi_rows_commit_shplonk(mh, i, 1, ha, 3, 2, pts, masks, cfs, c, ctypes.byref(hz)) == 0, i
            assert c.raw == want
            made[i] = (h.value, hz.value)
        # the multi form's limits: k = 0, k > 15, m = 0, m > 8, a mask bit >= k, equal points
        ha = (ctypes.c_uint64 * 1)(made[0][0])
        m9, p9, c16 = (ctypes.c_uint32 * 9)(*[1] * 9), b"".join(be(61 + p) for p in range(9)), be(1) * 16
        for k_, m_, ms_, pt_ in ((0, 2, masks, pts), (16, 2, masks, pts), (3, 0, masks, pts), (3, 9, m9, p9),
                                 (3, 2, (ctypes.c_uint32 * 2)(15, 2), pts), (3, 2, masks, be(61) + be(61))):
            assert lib.kzg_multi_rows_commit_shplonk(mh, 0, 1, ha, k_, m_, pt_, ms_, c16, c, ctypes.byref(hz)) == \
                _native.KZG_E_ARG, (k_, m_)
        assert lib.kzg_multi_rows_commit_shplonk(mh, 0, 1, ha, 3, 2, pts, masks, cfs, c, ctypes.byref(hz)) == 0
        assert lib.kzg_multi_rows_release(mh, 0, hz.value) == 0
        # worker 3 shares worker 0's device, worker 1 lives elsewhere: both are refused under index 0
        for wrong in (3, 1):
            ha = (ctypes.c_uint64 * 1)(made[wrong][0])
            assert lib.kzg_multi_rows_commit_shplonk(mh, 0, 1, ha, 3, 2, pts, masks, cfs, c, ctypes.byref(hz)) == \
                _native.KZG_E_ARG
        for i in range(M):
            for h in made[i]:
                assert lib.kzg_multi_rows_release(mh, i, h) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)
