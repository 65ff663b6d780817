"""GPU tests (`-m gpu`) of evaluate-then-open on committed row sets: kzg_rows_eval returns exactly the evaluations of
kzg_rows_open (and the oracle's), kzg_rows_open_lincomb with gamma powers returns exactly kzg_rows_open's proofs and with any
coefficients exactly kzg_open of the host-combined polynomial; a Fiat-Shamir PLONK-shaped round runs end to end and
verifies; errors answer KZG_E_ARG and leave the context serving; threads and the multi-GPU handle return the same bytes."""
import ctypes
import hashlib
import random
import threading

import pytest

from oracle import cpu as oc
from tests.gpu_common import R, be, rand_scalars_bytes, val as ib
from tests.gpu_rows import arg_error, commit_sets, engine_cache, release
from zkp_subnet_amd import _native
from zkp_subnet_amd.engine import _root_of_unity

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x11C0B1, 0x11C0B2


def make_rows(T, k, seed):
    rows = [rand_scalars_bytes(T, seed + j) for j in range(k)]
    if k >= 3:
        rows[1] = bytes(32 * T)      # a zero row
        rows[2] = rows[0]            # a duplicated row
    return rows


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


def gamma_coeffs(k, opened, gammas):
    """lambda_{p,j} = gamma_p^t for the t-th row j of opened[p], 0 elsewhere: the combination kzg_rows_open proves"""
    out = []
    for js, g in zip(opened, gammas):
        lam = [0] * k
        for t, j in enumerate(js):
            lam[j] = pow(ib(g), t, R)
        out.append([be(x) for x in lam])
    return out


def combine(rows, lam):
    cols = [[ib(r[32 * t:32 * t + 32]) for t in range(len(r) // 32)] for r in rows]
    out = [0] * len(cols[0])
    for c, l in zip(cols, lam):
        if l:
            out = [(a + l * b) % R for a, b in zip(out, c)]
    return b"".join(be(v) for v in out)


@pytest.mark.parametrize("lg,k,sizes", [(4, 3, (1, 2)), (10, 5, (2, 3)), (12, 4, (4,)), (16, 6, (3, 3)), (20, 9, (4, 5))])
def test_eval_rows_equals_open_rows_and_oracle(engines, lg, k, sizes):
    eng = engines(lg)
    T = 1 << lg
    rows = make_rows(T, k, 1000 * lg + k)
    rnd = random.Random(lg)
    w = _root_of_unity(T)
    zeta = rnd.randrange(R)
    P = [be(zeta), be(zeta * w), be(rnd.randrange(R))]
    G = [be(rnd.randrange(R)) for _ in P]
    opened = [list(range(k)), [k - 1], list(range(0, k, 2))]   # lg 20: 9 + 1 + 5 pairs, in two groups
    for ef in (True, False):
        sets = commit_sets(eng, rows, sizes, ef)
        try:
            Y = eng.eval_rows(sets, P, opened)
            assert Y == eng.open_rows(sets, P, opened, G)[0]
            if lg <= 12:
                coeffs = [oc.fr_ntt(r, True) if ef else r for r in rows]
                assert Y == [[oc.fr_eval(coeffs[j], a) for j in js] for a, js in zip(P, opened)]
            # a repeated handle: its rows twice in the numbering
            twice = [sets[-1], sets[-1]]
            kk = 2 * sizes[-1]
            assert eng.eval_rows(twice, P[:2], [list(range(kk)), [kk - 1]]) == \
                eng.open_rows(twice, P[:2], [list(range(kk)), [kk - 1]], G[:2])[0]
        finally:
            release(sets)
    assert eng.rows_stats() == (0, 0)


@pytest.mark.parametrize("lg", [10, 16])
def test_lincomb_with_gamma_powers_is_open_rows(engines, lg):
    eng = engines(lg)
    T = 1 << lg
    k = 5
    rows = make_rows(T, k, 77 + lg)
    rnd = random.Random(3 * lg)
    P = [be(rnd.randrange(R)) for _ in range(3)]
    G = [be(rnd.randrange(R)) for _ in range(3)]
    opened = [list(range(k)), [4], [0, 3]]
    sets = commit_sets(eng, rows, (2, 3))
    try:
        Y, Pf = eng.open_rows(sets, P, opened, G)
        V, Pl = eng.open_rows_lincomb(sets, P, gamma_coeffs(k, opened, G))
        assert Pl == Pf
        assert V == [be(sum(pow(ib(g), t, R) * ib(y) for t, y in enumerate(ys))) for ys, g in zip(Y, G)]
        C = [c for s in sets for c in s.commitments]
        assert eng.verify_open_lincomb(0, C, P, gamma_coeffs(k, opened, G), V, Pl)
        assert eng.verify_open_multi(0, C, P, opened, G, Y, Pl)
    finally:
        release(sets)


@pytest.mark.parametrize("lg,k", [(12, 6), (16, 4), (20, 3)])
def test_lincomb_random_coefficients_is_kzg_open(engines, lg, k):
    eng = engines(lg)
    T = 1 << lg
    rows = make_rows(T, k, 555 + lg)
    rnd = random.Random(7 * lg)
    m = 4 if lg < 20 else 2
    P = [be(rnd.randrange(R)) for _ in range(m)]
    lams = []
    for p in range(m):
        lam = [rnd.choice([0, 1, R - 1, rnd.randrange(R)]) for _ in range(k)]
        lam[p % k] = lam[p % k] or rnd.randrange(1, R)
        lams.append(lam)
    sets = commit_sets(eng, rows, (k,), ef=False)
    try:
        V, Pf = eng.open_rows_lincomb(sets, P, [[be(x) for x in lam] for lam in lams])
        for p in range(m):
            assert (V[p], Pf[p]) == eng.open(0, combine(rows, lams[p]), P[p], evaluation_form=False), p
        assert eng.verify_open_lincomb(0, sets[0].commitments, P, [[be(x) for x in lam] for lam in lams], V, Pf)
    finally:
        release(sets)


def _transcript(*parts):
    h = hashlib.sha256()
    for x in parts:
        h.update(x)
    return ib(h.digest()) % R


def test_fiat_shamir_plonk_round(engines):
    lg = 12
    eng = engines(lg)
    T = 1 << lg
    w = _root_of_unity(T)
    # wires a, b, c | accumulator Z | selectors qL, qR, qO, qM, qC | sigma1..3 | quotient pieces t_lo, t_mid, t_hi
    groups = [make_rows(T, n, s) for n, s in ((3, 10), (1, 20), (5, 30), (3, 40), (3, 50))]
    S = [eng.commit_rows(0, g) for g in groups]
    try:
        C = [c for s in S for c in s.commitments]
        zeta = _transcript(b"plonk", *C)
        P = [be(zeta), be(zeta * w)]
        A, B, Cw, Z, QL, QR, QO, QM, QC, S1, S2, S3, TL, TM, TH = range(15)
        opened = [[A, B, Cw, S1, S2], [Z]]

        def round5(Y):
            a, b, c, s1, s2 = (ib(y) for y in Y[0])
            zw = ib(Y[1][0])
            v = _transcript(b"evals", *[y for ys in Y for y in ys])
            beta, gamma, alpha = _transcript(b"beta", *C), _transcript(b"gamma", *C), _transcript(b"alpha", *C)
            zh = (pow(zeta, T, R) - 1) % R
            lam = [0] * 15
            lam[QL], lam[QR], lam[QO], lam[QM], lam[QC] = a, b, c, a * b % R, 1
            lam[Z] = alpha * (a + beta * zeta + gamma) * (b + beta * 5 * zeta + gamma) * (c + beta * 7 * zeta + gamma) % R
            lam[S3] = -alpha * beta * zw * (a + beta * s1 + gamma) * (b + beta * s2 + gamma) % R
            lam[TL], lam[TM], lam[TH] = -zh % R, -zh * pow(zeta, T, R) % R, -zh * pow(zeta, 2 * T, R) % R
            for t, j in enumerate((A, B, Cw, S1, S2)):
                lam[j] = pow(v, t + 1, R)
            at_zw = [0] * 15
            at_zw[Z] = 1
            return [[be(x) for x in lam], [be(x) for x in at_zw]]

        Y = eng.eval_rows(S, P, opened)
        coeffs = round5(Y)
        V, Pf = eng.open_rows_lincomb(S, P, coeffs)
        assert eng.verify_open_lincomb(0, C, P, coeffs, V, Pf)
        assert V[1] == Y[1][0]
        full = eng.eval_rows(S, P[:1], [list(range(15))])[0]
        assert V[0] == be(sum(ib(l) * ib(y) for l, y in zip(coeffs[0], full)))
        # a flipped evaluation changes v (and the scalars): the old proof no longer verifies under them
        bad = [list(Y[0]), list(Y[1])]
        bad[0][0] = be(ib(bad[0][0]) + 1)
        coeffs2 = round5(bad)
        assert coeffs2 != coeffs
        assert not eng.verify_open_lincomb(0, C, P, coeffs2, V, Pf)
    finally:
        release(S)


def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 8
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    rows = make_rows(T, 4, 4040)
    rnd = random.Random(40)
    P = [be(rnd.randrange(R)) for _ in range(2)]
    L = [[be(rnd.randrange(R)) for _ in range(4)], [be(0), be(1), be(0), be(2)]]
    opened = [[0, 1, 2, 3], [1]]
    with eng.commit_rows(0, rows) as rs:
        want = (eng.eval_rows([rs], P, opened), eng.open_rows_lincomb([rs], P, L))

    def fresh_ok():
        with eng.commit_rows(0, rows) as rs_:
            assert (eng.eval_rows([rs_], P, opened), eng.open_rows_lincomb([rs_], P, L)) == want

    rs = eng.commit_rows(0, rows)
    rs.release()
    arg_error(lambda: eng.eval_rows([rs], P, opened), "released")
    arg_error(lambda: eng.open_rows_lincomb([rs], P, L), "released")
    fresh_ok()
    with eng.commit_rows(0, rows) as rs:
        arg_error(lambda: eng.open_rows_lincomb([rs], P, [L[0], L[1][:3] + [R.to_bytes(32, "big")]]), "canonical")
        arg_error(lambda: eng.open_rows_lincomb([rs], P, [L[0], [be(0)] * 4]), "nonzero")
        arg_error(lambda: eng.open_rows_lincomb([rs], P, [x[:3] for x in L]), "k must equal")
        arg_error(lambda: eng.open_rows_lincomb([rs], [P[0], R.to_bytes(32, "big")], L), "canonical")
        arg_error(lambda: eng.eval_rows([rs], [P[0], R.to_bytes(32, "big")], opened), "canonical")
        arg_error(lambda: eng.eval_rows([rs], P, [[0, 4], [1]]))
        with eng.commit_rows(1, rows[:2]) as other:
            arg_error(lambda: eng.eval_rows([rs, other], P[:1], [[0]]), "one worker")
            arg_error(lambda: eng.open_rows_lincomb([rs, other], P[:1], [L[0] + L[0][:2]]), "one worker")
        assert (eng.eval_rows([rs], P, opened), eng.open_rows_lincomb([rs], P, L)) == want
    fresh_ok()
    st = eng.commit_rows(0, rows)
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.eval_rows([st], P, opened), "SRS")
    arg_error(lambda: eng.open_rows_lincomb([st], P, L), "SRS")
    st.release()
    fresh_ok()
    assert eng.rows_stats() == (0, 0)


def test_threads_mix_eval_and_lincomb(engines):
    lg = 10
    eng = engines(lg)
    T = 1 << lg
    rnd = random.Random(81)
    rows = make_rows(T, 6, 8181)
    P = [be(rnd.randrange(R)) for _ in range(2)]
    opened = [list(range(6)), [5]]
    Ls = {t: [[be(rnd.randrange(R)) for _ in range(6)], [be(0)] * 5 + [be(t + 1)]] for t in range(8)}
    sets = commit_sets(eng, rows, (2, 4))
    try:
        want_y = eng.eval_rows(sets, P, opened)
        want = {t: eng.open_rows_lincomb(sets, P, Ls[t]) for t in range(8)}
        errors = []

        def work(t):
            try:
                for n in range(6):
                    if (n + t) % 2:
                        assert eng.eval_rows(sets, P, opened) == want_y
                    else:
                        assert eng.open_rows_lincomb(sets, P, Ls[t]) == want[t]
            except Exception as ex:   # noqa: BLE001
                errors.append(repr(ex))

        ths = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        for x in ths:
            x.start()
        for x in ths:
            x.join()
        assert not errors, errors
    finally:
        release(sets)
    assert eng.rows_stats() == (0, 0)


def test_multi_routing(hip):
    from zkp_subnet_amd.engine import lagrange_factor

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
        pts = [be(4444), be(4445)]
        opened = [[0, 1, 2, 3], [0, 3]]
        masks = (ctypes.c_uint32 * 2)(15, 9)
        L = [[be(3), be(0), be(5), be(R - 1)], [be(1), be(0), be(0), be(0)]]
        c, e = ctypes.create_string_buffer(48 * 4), ctypes.create_string_buffer(32 * 6)
        v, p = ctypes.create_string_buffer(64), ctypes.create_string_buffer(96)
        handles = {}
        for i in range(M):
            rows = make_rows(T, 4, 900 + i)
            with single.commit_rows(i, rows) as rs:
                Y = single.eval_rows([rs], pts, opened)
                V, Pf = single.open_rows_lincomb([rs], pts, L)
            h = ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 4, b"".join(rows), T, 1, c, ctypes.byref(h)) == 0, i
            hs = (ctypes.c_uint64 * 1)(h.value)
            assert lib.kzg_multi_rows_eval(mh, i, 1, hs, 2, b"".join(pts), masks, e) == 0, i
            assert [e.raw[32 * t:32 * t + 32] for t in range(6)] == Y[0] + Y[1]
            flat = b"".join(x for lam in L for x in lam)
            assert lib.kzg_multi_rows_open_lincomb(mh, i, 1, hs, 4, 2, b"".join(pts), flat, v, p) == 0, i
            assert [v.raw[:32], v.raw[32:]] == V and [p.raw[:48], p.raw[48:]] == Pf
            handles[i] = h.value
        flat = b"".join(x for lam in L for x in lam)
        for wrong in (handles[3], handles[1]):            # worker 3 shares worker 0's device; worker 1 lives elsewhere
            hs = (ctypes.c_uint64 * 1)(wrong)
            assert lib.kzg_multi_rows_eval(mh, 0, 1, hs, 2, b"".join(pts), masks, e) == _native.KZG_E_ARG
            assert lib.kzg_multi_rows_open_lincomb(mh, 0, 1, hs, 4, 2, b"".join(pts), flat, v, p) == _native.KZG_E_ARG
        for i in range(M):
            assert lib.kzg_multi_rows_release(mh, i, handles[i]) == 0
    finally:
        lib.kzg_multi_destroy(mh)
