"""GPU tests (`-m gpu`) of committed row sets: kzg_rows_commit keeps k rows on the device, kzg_rows_open opens rows of one or
more sets at up to 4 points.  Every commitment equals kzg_commit of its row and every open equals kzg_commit_open_multi on
the concatenated rows, bit for bit (one shape also against the C oracle); the lifecycle rules (release, stale sets after an
SRS reload, the set cap, mixed workers or lengths) answer KZG_E_ARG / KZG_E_BUSY and leave the context serving."""
import ctypes
import random
import threading

import pytest

from oracle import cpu as oc
from tests.gpu_common import R, be, rand_scalars_bytes
from tests.gpu_rows import arg_error, commit_sets, engine_cache, release
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import _root_of_unity

pytestmark = pytest.mark.gpu
TH = 16
SEED_X, SEED_Y = 0x5EED01, 0x5EED02


def make_rows(T, k, seed):
    rows = [rand_scalars_bytes(T, seed + j) for j in range(k)]
    if k >= 3:
        rows[1] = bytes(32 * T)      # a zero row
        rows[2] = rows[0]            # a duplicated row
    return rows


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


def chalk(rnd, m):
    return [be(rnd.randrange(R)) for _ in range(m)], [be(rnd.randrange(R)) for _ in range(m)]


def opened_for(k, m):
    """m = 1: every row; m = 2: every row at zeta, the last also at zeta * omega; m = 4: mixed masks"""
    if m == 1:
        return [list(range(k))]
    if m == 2:
        return [list(range(k)), [k - 1]]
    return [list(range(k)), [0], list(range(0, k, 2)), [k - 1]]


@pytest.mark.parametrize("lg,k,m", [(4, 1, 1), (4, 16, 4), (10, 3, 2), (10, 8, 4), (12, 8, 2), (12, 16, 1),
                                    (16, 16, 4), (16, 3, 2), (16, 1, 1)])
def test_parity_with_commit_open_multi(engines, lg, k, m):
    eng = engines(lg)
    T = 1 << lg
    rows = make_rows(T, k, 10_000 * lg + 100 * k + m)
    opened = opened_for(k, m)
    rnd = random.Random(lg * 1000 + k * 10 + m)
    for ef in (True, False):
        P, G = chalk(rnd, m)
        C, Y, Pf = eng.commit_open_multi(0, rows, P, opened, G, ef)
        assert C == [eng.commit(0, r, ef) for r in rows]
        sizes = [s for s in (1, k - 3, 2) if s] if k >= 3 else [k]   # one set, and the same rows over several
        for sz in ([k], sizes):
            sets = commit_sets(eng, rows, sz, ef)
            try:
                assert [c for s in sets for c in s.commitments] == C
                assert eng.open_rows(sets, P, opened, G) == (Y, Pf)
            finally:
                release(sets)
    assert eng.rows_stats() == (0, 0)


def test_oracle_parity(engines):
    lg, k = 10, 3
    eng = engines(lg)
    T = 1 << lg
    srs = oc.srs_gen(be(SEED_X + lg), be(SEED_Y), lg, 0, 0)
    rows = make_rows(T, k, 4242)
    w = _root_of_unity(T)
    zeta = 0x1234567890ABCDEF
    P, G = [be(zeta), be(zeta * w)], [be(777), be(0)]
    opened = [[0, 1, 2], [2]]
    with eng.commit_rows(0, rows) as rs:
        assert rs.commitments == [oc.commit(srs, r, True, threads=TH) for r in rows]
        Y, Pf = eng.open_rows([rs], P, opened, G)
    assert Y == [[oc.fr_eval(oc.fr_ntt(rows[j], True), a) for j in js] for a, js in zip(P, opened)]

    def combine(rs_, gamma):
        cols = [[int.from_bytes(r[32 * t:32 * t + 32], "big") for t in range(T)] for r in rs_]
        out = [0] * T
        for col in reversed(cols):
            out = [(a * gamma + b) % R for a, b in zip(out, col)]
        return b"".join(be(v) for v in out)

    assert Pf == [oc.open_(srs, combine([rows[j] for j in js], int.from_bytes(g, "big")), a, True, threads=TH)[1]
                  for a, js, g in zip(P, opened, G)]
    assert eng.verify_open_multi(0, rs.commitments, P, opened, G, Y, Pf)


def test_plonk_flow_over_four_sets(engines):
    lg = 12
    eng = engines(lg)
    T = 1 << lg
    w = _root_of_unity(T)
    wires, acc, quot, pre = (make_rows(T, n, s) for n, s in ((3, 100), (1, 200), (3, 300), (5, 400)))
    rnd = random.Random(5)
    S = [eng.commit_rows(0, r) for r in (wires, acc, quot, pre)]   # the rounds: each set committed before the next challenge
    try:
        zeta = rnd.randrange(R)
        P, G = [be(zeta), be(zeta * w)], [be(rnd.randrange(R)), be(rnd.randrange(R))]
        rows = wires + acc + quot + pre
        opened = [list(range(12)), [3]]
        Y, Pf = eng.open_rows(S, P, opened, G)
        C = [c for s in S for c in s.commitments]
        assert (C, Y, Pf) == eng.commit_open_multi(0, rows, P, opened, G)
        assert eng.verify_open_multi(0, C, P, opened, G, Y, Pf)
        bad = [list(y) for y in Y]
        bad[1][0] = be(int.from_bytes(bad[1][0], "big") + 1)
        assert not eng.verify_open_multi(0, C, P, opened, G, bad, Pf)
        # a handle listed twice: its rows appear twice in the numbering
        S2 = [S[0], S[1], S[2], S[1]]
        rows2 = wires + acc + quot + acc
        opened2 = [list(range(8)), [3, 7]]
        Y2, Pf2 = eng.open_rows(S2, P, opened2, G)
        C2 = [c for s in S2 for c in s.commitments]
        assert (C2, Y2, Pf2) == eng.commit_open_multi(0, rows2, P, opened2, G)
        assert eng.verify_open_multi(0, C2, P, opened2, G, Y2, Pf2)
    finally:
        release(S)


def test_reopening_one_set_at_two_point_sets(engines):
    lg = 12
    eng = engines(lg)
    rows = make_rows(1 << lg, 5, 909)
    rnd = random.Random(9)
    with eng.commit_rows(0, rows) as rs:
        for opened in ([[0, 1, 2, 3, 4], [4]], [[1, 3], [0, 2, 4], [4], [0]]):
            P, G = chalk(rnd, len(opened))
            _, Y, Pf = eng.commit_open_multi(0, rows, P, opened, G)
            assert eng.open_rows([rs], P, opened, G) == (Y, Pf)
        P, G = chalk(rnd, 1)
        assert eng.open_rows([rs.handle], P, [[2]], G) == eng.commit_open_multi(0, rows, P, [[2]], G)[1:]


def test_long_rows_two_lane_commit(engines):
    lg = 19
    eng = engines(lg)
    rows = make_rows(1 << lg, 3, 1919)
    rnd = random.Random(19)
    P, G = chalk(rnd, 2)
    opened = [[0, 1, 2], [2]]
    C, Y, Pf = eng.commit_open_multi(0, rows, P, opened, G)
    with eng.commit_rows(0, rows) as rs:
        assert rs.commitments == C
        assert rs.commitments[0] == eng.commit(0, rows[0])
        assert eng.open_rows([rs], P, opened, G) == (Y, Pf)


def test_lifecycle(hip):
    eng = hip()
    lg = 8
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers, slices of 2^8 points
    rnd = random.Random(88)
    rows = make_rows(T, 4, 8080)
    P, G = chalk(rnd, 2)
    opened = [[0, 1, 2, 3], [1]]
    want = eng.commit_open_multi(0, rows, P, opened, G)

    def fresh_ok():                                   # after any error the next call is bit-exact
        with eng.commit_rows(0, rows) as rs:
            assert (rs.commitments,) + eng.open_rows([rs], P, opened, G) == want

    # open after release, double release
    rs = eng.commit_rows(0, rows)
    rs.release()
    arg_error(lambda: eng.open_rows([rs], P, opened, G))
    arg_error(lambda: eng.release_rows(rs.handle))
    arg_error(lambda: eng.release_rows(0))
    fresh_ok()
    # handles are not reused
    a = eng.commit_rows(0, rows[:1])
    a.release()
    b = eng.commit_rows(0, rows[:1])
    assert b.handle != a.handle
    b.release()
    # sets of two workers, sets of two lengths
    s0, s1 = eng.commit_rows(0, rows[:2]), eng.commit_rows(1, rows[2:])
    arg_error(lambda: eng.open_rows([s0, s1], P, opened, G), "one worker")
    short = eng.commit_rows(0, [r[:32 * (T // 2)] for r in rows[2:]])
    arg_error(lambda: eng.open_rows([s0, short], P, opened, G), "one row length")
    release([s0, s1, short])
    fresh_ok()
    # more than 16 rows in all
    big = [eng.commit_rows(0, make_rows(T, 9, 1)), eng.commit_rows(0, make_rows(T, 8, 2))]
    arg_error(lambda: eng.open_rows(big, P[:1], [[0]], G[:1]), "KZG_MAX_BATCH_OPEN")
    # a mask past the concatenated rows; the single set still opens
    arg_error(lambda: eng.open_rows(big[1:], P[:1], [[8]], G[:1]))
    release(big)
    fresh_ok()
    # argument checks of the commit
    arg_error(lambda: eng.commit_rows(2, rows))                               # worker outside the SRS
    arg_error(lambda: eng.commit_rows(0, make_rows(T, 17, 3)))                # k = 17
    arg_error(lambda: eng.commit_rows(0, [r + r for r in rows]))             # longer than the slice
    arg_error(lambda: eng.commit_rows(0, [r[:32 * 3] for r in rows]))        # evaluation form of length 3
    fresh_ok()
    # the cap: KZG_MAX_ROW_SETS live sets, then KZG_E_BUSY until one is released
    cap = []
    try:
        for n in range(_native.KZG_MAX_ROW_SETS):
            cap.append(eng.commit_rows(n % 2, rows[:1]))
        live, nbytes = eng.rows_stats()
        assert live == _native.KZG_MAX_ROW_SETS and nbytes >= live * 32 * T
        with pytest.raises(KzgError) as ei:
            eng.commit_rows(0, rows[:1])
        assert ei.value.code == _native.KZG_E_BUSY
        assert eng.rows_stats()[0] == _native.KZG_MAX_ROW_SETS
        cap.pop(5).release()
        cap.append(eng.commit_rows(0, rows))                                      # larger than the freed buffer
        assert (cap[-1].commitments,) + eng.open_rows([cap[-1]], P, opened, G) == want
        assert eng.commit_open_multi(0, rows, P, opened, G) == want
    finally:
        release(cap)
    assert eng.rows_stats() == (0, 0)
    # an SRS reload makes every live set stale; its release still succeeds
    st = eng.commit_rows(0, rows)
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.open_rows([st], P, opened, G), "SRS")
    assert eng.rows_stats()[0] == 1
    st.release()
    assert eng.rows_stats() == (0, 0)
    fresh_ok()
    # kzg_destroy with live sets
    other = hip()
    other.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    keep = [other.commit_rows(0, rows), other.commit_rows(1, rows[:2])]
    assert other.rows_stats()[0] == 2
    other.close()
    assert keep[0].handle != keep[1].handle
    fresh_ok()


def test_threads(engines):
    lg = 10
    eng = engines(lg)
    T = 1 << lg
    rnd = random.Random(31)
    P, G = chalk(rnd, 2)
    opened = [[0, 1, 2], [2]]
    rows = {t: make_rows(T, 3, 3000 + 10 * t) for t in range(8)}
    want = {t: eng.commit_open_multi(0, rows[t], P, opened, G) for t in range(8)}
    errors = []

    def work(t):
        try:
            for n in range(6):
                if (n + t) % 3 == 2:
                    assert eng.commit_open_multi(0, rows[t], P, opened, G) == want[t]
                    continue
                with eng.commit_rows(0, rows[t]) as rs:
                    assert rs.commitments == want[t][0]
                    assert eng.open_rows([rs], P, opened, G) == want[t][1:]
                    assert eng.open_rows([rs], P, opened, G) == want[t][1:]
        except Exception as ex:   # noqa: BLE001
            errors.append(repr(ex))

    ths = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for x in ths:
        x.start()
    for x in ths:
        x.join()
    assert not errors, errors
    assert eng.rows_stats() == (0, 0)

    # a release racing opens of the same set: every open returns the right bytes or KZG_E_ARG, nothing else
    rs = eng.commit_rows(0, rows[0])
    outcomes = []
    started = threading.Event()

    def opener():
        for _ in range(20):
            started.set()
            try:
                outcomes.append(eng.open_rows([rs.handle], P, opened, G) == want[0][1:])
            except KzgError as ex:
                outcomes.append("arg" if ex.code == _native.KZG_E_ARG else repr(ex))

    th = threading.Thread(target=opener)
    th.start()
    started.wait()
    rs.release()
    th.join()
    assert outcomes and all(o is True or o == "arg" for o in outcomes), outcomes
    assert eng.rows_stats() == (0, 0)
    with eng.commit_rows(0, rows[1]) as again:          # the reclaimed buffer serves the next set
        assert (again.commitments,) + eng.open_rows([again], P, opened, G) == want[1]


def test_multi_handle_routing(hip):
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
        pts, gms = [be(4444), be(4445)], [be(5555), be(5556)]
        opened = [[0, 1, 2, 3], [0, 3]]
        masks = (ctypes.c_uint32 * 2)(15, 9)
        c, e, p = ctypes.create_string_buffer(48 * 4), ctypes.create_string_buffer(32 * 6), ctypes.create_string_buffer(96)
        handles = {}
        for i in range(M):
            rows = make_rows(T, 4, 600 + i)
            C, Y, Pf = single.commit_open_multi(i, rows, pts, opened, gms)
            h = ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 4, b"".join(rows), T, 1, c, ctypes.byref(h)) == 0, i
            assert [c.raw[48 * j:48 * j + 48] for j in range(4)] == C
            hs = (ctypes.c_uint64 * 1)(h.value)
            assert lib.kzg_multi_rows_open(mh, i, 1, hs, 2, b"".join(pts), masks, b"".join(gms), e, p) == 0, i
            assert [e.raw[32 * t:32 * t + 32] for t in range(6)] == Y[0] + Y[1]
            assert [p.raw[:48], p.raw[48:]] == Pf
            handles[i] = h.value
        # worker 3 lives on worker 0's device (3 mod 3 == 0): its sets are not worker 0's
        hs = (ctypes.c_uint64 * 1)(handles[3])
        assert lib.kzg_multi_rows_open(mh, 0, 1, hs, 2, b"".join(pts), masks, b"".join(gms), e, p) == _native.KZG_E_ARG
        assert lib.kzg_multi_rows_release(mh, 0, handles[3]) == _native.KZG_E_ARG
        hs = (ctypes.c_uint64 * 1)(handles[1])                  # another device's handle
        assert lib.kzg_multi_rows_open(mh, 0, 1, hs, 2, b"".join(pts), masks, b"".join(gms), e, p) == _native.KZG_E_ARG
        for i in range(M):
            assert lib.kzg_multi_rows_release(mh, i, handles[i]) == 0
            assert lib.kzg_multi_rows_release(mh, i, handles[i]) == _native.KZG_E_ARG
        assert lib.kzg_multi_rows_commit(mh, M, 4, b"".join(rows), T, 1, c, ctypes.byref(h)) == _native.KZG_E_ARG
    finally:
        lib.kzg_multi_destroy(mh)


def test_multi_device_client_and_text(hip):
    from zkp_subnet_amd import MultiDeviceClient, codec
    from zkp_subnet_amd.client import Client

    scale, ms = 12, 2
    T = 1 << (scale - ms)
    multi = MultiDeviceClient(devices=[0, 0], seed=77)
    multi.start(scale=scale, machines_scale=ms)
    try:
        xs = [codec.be32_to_fr(be(8080)), codec.be32_to_fr(be(8081))]
        gs = [codec.be32_to_fr(be(9090)), codec.be32_to_fr(be(9091))]
        opened = [[0, 1, 2], [1]]
        for i in range(1 << ms):
            rows = make_rows(T, 3, 700 + i)
            polys = [codec.be32_to_fr_list(r) for r in rows]
            ref = multi.worker_commit_open_multi(i, polys, xs, opened, gs).json()
            a = multi.worker_commit_rows(i, polys[:1])
            b = multi.worker_commit_rows(i, polys[1:])
            assert a.status_code == 200 and b.status_code == 200, (a.json(), b.json())
            hs = [a.json()["handle"], b.json()["handle"]]
            r = multi.worker_open_rows(hs, xs, opened, gs)
            assert r.status_code == 200, r.json()
            C = a.json()["commitments"] + b.json()["commitments"]
            assert C == ref["commitments"] and r.json() == {"evals": ref["evals"], "proofs": ref["proofs"]}
            v = multi.worker_verify_open_multi(i, r.json()["proofs"], xs, opened, gs, r.json()["evals"], C)
            assert v.status_code == 200 and v.json() == {"valid": True}
            assert multi.worker_open_rows(hs, xs, [[0, 1, 3], [1]], gs).status_code == 400
            for h in hs:
                assert multi.worker_release_rows(h).status_code == 200
            assert multi.worker_open_rows(hs, xs, opened, gs).status_code == 400
    finally:
        multi.stop()

    cl = Client(seed=99)
    cl.start(scale=12, machines_scale=1)
    try:
        rows = make_rows(1 << 11, 4, 808)
        polys = [codec.be32_to_fr_list(r) for r in rows]
        pts = [be(1234567), be(1234568), be(1234569)]
        gms = [be(7654321), be(7654322), be(7654323)]
        opened = [[0, 1, 2, 3], [3], [0, 2]]
        X, Gs = [codec.be32_to_fr(x) for x in pts], [codec.be32_to_fr(g) for g in gms]
        r = cl.worker_commit_rows(1, polys)
        assert r.status_code == 200, r.json()
        C, Y, Pf = cl.engine.commit_open_multi(1, rows, pts, opened, gms)
        assert [codec.g1_from_b64(c) for c in r.json()["commitments"]] == C
        o = cl.worker_open_rows([r.json()["handle"]], X, opened, Gs)
        assert o.status_code == 200, o.json()
        assert [[codec.fr_to_be32(e) for e in ev] for ev in o.json()["evals"]] == Y
        assert [codec.g1_from_b64(p) for p in o.json()["proofs"]] == Pf
        assert cl.worker_release_rows(r.json()["handle"]).json() == {"released": True}
        assert cl.worker_release_rows(r.json()["handle"]).status_code == 400
        assert cl.engine.rows_stats() == (0, 0)
    finally:
        cl.stop()
