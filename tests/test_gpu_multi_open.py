"""GPU tests (`-m gpu`) of the multi-point opening (kzg_commit_open_multi): k rows of one worker at m <= 4 points, point p
opening the rows opened[p] with one proof for h_p = sum_t gamma_p^t f_{j_t}.  Every commitment, evaluation and proof is
compared bit for bit with the C oracle (commit, fr_eval, open_ on h_p) or with the batched / single-row paths that the
oracle already pins, and every proof passes kzg_vk_verify_open_multi."""
import ctypes
import random
import threading

import pytest

from oracle import cpu as oc
from tests.gpu_common import be, rand_scalars_bytes
from zkp_subnet_amd import _native
from zkp_subnet_amd.engine import R_MODULUS as R, _root_of_unity

pytestmark = pytest.mark.gpu
TH = 16


def combine(rows, gamma):
    T = len(rows[0]) // 32
    cols = [[int.from_bytes(r[32 * t:32 * t + 32], "big") for t in range(T)] for r in rows]
    out = [0] * T
    for col in reversed(cols):
        out = [(a * gamma + b) % R for a, b in zip(out, col)]
    return b"".join(be(v) for v in out)


def oracle_eval(row, alpha32, ef):
    return oc.fr_eval(oc.fr_ntt(row, True) if ef else row, alpha32)


def make_rows(T, k, seed):
    rows = [rand_scalars_bytes(T, seed + j) for j in range(k)]
    if k >= 3:
        rows[1] = bytes(32 * T)      # a zero row
        rows[2] = rows[0]            # a duplicated row
    return rows


def engine(hip, scale, ms, i, window=0):
    eng = hip(window)
    eng.gen_srs(0xC0FFEE + scale, 0xBADC0DE, scale, ms, [i])   # resident slice 0 = worker i
    return eng, oc.srs_gen(be(0xC0FFEE + scale), be(0xBADC0DE), scale, ms, i)


def check(eng, srs, rows, points, opened, gammas, ef, commits=None):
    """one multi-point call against the oracle; returns the oracle commitments (they depend on the rows only)"""
    P, G = [be(a) for a in points], [be(g) for g in gammas]
    C, Y, Pf = eng.commit_open_multi(0, rows, P, opened, G, ef)
    if commits is None:
        commits = [oc.commit(srs, r, ef, threads=TH) for r in rows]
    assert C == commits
    assert Y == [[oracle_eval(rows[j], a, ef) for j in js] for a, js in zip(P, opened)]
    assert Pf == [oc.open_(srs, combine([rows[j] for j in js], g), a, ef, threads=TH)[1]
                  for a, js, g in zip(P, opened, gammas)]
    assert eng.verify_open_multi(0, C, P, opened, G, Y, Pf)
    return commits


def shape_opened(k, m, T):
    """m = 2 on a k-row shape: every row at zeta, the last row (the permutation accumulator) also at zeta * omega; m = 4:
    full masks.  The points: zeta and zeta * omega, then two more."""
    if m == 2:
        return [list(range(k)), [k - 1]]
    return [list(range(k))] * m


@pytest.mark.parametrize("scale,ms,i,k,m", [(10, 2, 3, 3, 2), (12, 0, 0, 8, 2), (16, 4, 9, 4, 4), (16, 0, 0, 15, 2),
                                            (16, 0, 0, 16, 4)])
def test_oracle_parity(hip, scale, ms, i, k, m):
    """(16,0,0,15,2): 17 sets in one pass; (16,0,0,16,4): 20 sets, two passes."""
    eng, srs = engine(hip, scale, ms, i)
    T = 1 << (scale - ms)
    rnd = random.Random(scale * 100 + k * 10 + m)
    rows = make_rows(T, k, 1000 * scale + k)
    opened = shape_opened(k, m, T)
    w = _root_of_unity(T)
    alphas = [0, pow(w, 3, R), R - 1, rnd.randrange(R)]
    gammas = [0, 1, rnd.randrange(R)]
    zeta = rnd.randrange(R)
    cases = [([zeta, zeta * w % R] + alphas[:m - 2], [rnd.randrange(R) for _ in range(m)])]
    if T <= 1 << 12:   # every (alpha, gamma) value at every point position on short rows
        for a in alphas:
            for g in gammas:
                cases.append(([a] + alphas[:m - 1], [g] + gammas[:m - 1]))
    else:              # the long ones: alpha 0 and w^3 with gamma 0 and 1 (m = 4: every alpha)
        cases.append(((alphas * 2)[:m], (gammas * 2)[:m]))
    for ef in (True, False):
        commits = None
        for pts, gms in cases:
            commits = check(eng, srs, rows, pts, opened, gms, ef, commits)


@pytest.mark.parametrize("lg", [10, 16])
def test_m1_full_mask_is_commit_open_batch(hip, lg):
    eng, _ = engine(hip, lg, 0, 0)
    T = 1 << lg
    rows = make_rows(T, 5, 500 + lg)
    rnd = random.Random(lg)
    alpha, gamma = be(rnd.randrange(R)), be(rnd.randrange(R))
    for ef in (True, False):
        C, Y, P = eng.commit_open_batch(0, rows, alpha, gamma, ef)
        assert eng.commit_open_multi(0, rows, [alpha], [list(range(5))], [gamma], ef) == (C, [Y], [P])


def test_subset_mask_is_commit_open_batch_on_those_rows(hip):
    eng, _ = engine(hip, 12, 0, 0)
    T = 1 << 12
    rows = make_rows(T, 6, 4646)
    rnd = random.Random(46)
    a0, a1, g0, g1 = (be(rnd.randrange(R)) for _ in range(4))
    opened = [[0, 2, 5], [1, 3, 4]]
    C, Y, P = eng.commit_open_multi(0, rows, [a0, a1], opened, [g0, g1])
    for a, g, js, y, p in zip((a0, a1), (g0, g1), opened, Y, P):
        Cb, Yb, Pb = eng.commit_open_batch(0, [rows[j] for j in js], a, g)
        assert (Yb, Pb) == (y, p)
        assert Cb == [C[j] for j in js]
    # two equal points keep their own proofs
    C2, Y2, P2 = eng.commit_open_multi(0, rows, [a0, a0], opened, [g0, g1])
    assert P2[0] == P[0] and Y2[0] == Y[0]
    assert P2[1] == eng.commit_open_batch(0, [rows[j] for j in opened[1]], a0, g1)[2]
    assert eng.verify_open_multi(0, C2, [a0, a0], opened, [g0, g1], Y2, P2)


def test_long_rows(hip):
    """T = 2^20 (past KZG_BATCHED_ROW_MAX): the evaluations in groups, k + m single-set MSMs over two lanes; the batched
    and single-row paths are oracle-pinned at this size."""
    eng, _ = engine(hip, 20, 0, 0)
    T = 1 << 20
    rows = make_rows(T, 3, 2020)
    rnd = random.Random(20)
    pts = [be(rnd.randrange(R)) for _ in range(2)]
    gms = [be(rnd.randrange(R)) for _ in range(2)]
    opened = [[0, 1, 2], [2]]
    for ef in (True, False):
        C, Y, P = eng.commit_open_multi(0, rows, pts, opened, gms, ef)
        assert eng.commit_open_multi_joined(0, b"".join(rows), 3, pts, opened, gms, ef) == (C, Y, P)
        Cb, Yb, Pb = eng.commit_open_batch(0, rows, pts[0], gms[0], ef)
        assert (C, Y[0], P[0]) == (Cb, Yb, Pb)
        assert [Y[1][0], P[1]] == list(eng.open(0, rows[2], pts[1], ef))
        assert eng.verify_open_multi(0, C, pts, opened, gms, Y, P)


@pytest.mark.parametrize("window,k,m", [(20, 8, 2), (22, 3, 3)])
def test_forced_window_splits_the_sets_over_passes(hip, window, k, m):
    """A wide forced window leaves the sort's key (or the bucket memory) room for fewer sets than k + m: several passes."""
    eng, srs = engine(hip, 10, 0, 0, window=window)
    assert eng.window == window
    rows = make_rows(1 << 10, k, 3000 + window)
    rnd = random.Random(window)
    opened = [list(range(k))] + [[j for j in range(k) if j % (p + 2) == 0] for p in range(m - 1)]
    check(eng, srs, rows, [rnd.randrange(R) for _ in range(m)], opened, [rnd.randrange(R) for _ in range(m)], True)


def test_argument_errors_leave_the_context_serving(hip):
    eng, srs = engine(hip, 10, 0, 0)
    lib, h = eng._lib, eng._h
    T = 1 << 10
    rows = make_rows(T, 3, 4242)
    blob = b"".join(rows)
    pts, gms = be(99) + be(98), be(7) + be(8)
    rbig = R.to_bytes(32, "big")
    c, e, p = ctypes.create_string_buffer(48 * 17), ctypes.create_string_buffer(32 * 80), ctypes.create_string_buffer(48 * 5)

    def masks(*v):
        return (ctypes.c_uint32 * max(len(v), 1))(*v)

    cases = [(0, 0, blob, T, 1, 2, pts, masks(7, 1), gms),            # k = 0
             (0, 17, blob * 6, T, 1, 2, pts, masks(7, 1), gms),      # k > 16
             (0, 3, blob, T, 1, 0, pts, masks(7), gms),              # m = 0
             (0, 3, blob, T, 1, 5, pts * 3, masks(7, 1, 1, 1, 1), gms * 3),   # m > 4
             (0, 3, blob, T, 1, 2, pts, masks(7, 0), gms),           # a zero mask
             (0, 3, blob, T, 1, 2, pts, masks(7, 8), gms),           # a mask bit >= k
             (0, 3, blob, T, 1, 2, be(99) + rbig, masks(7, 1), gms),  # a point >= r
             (0, 3, blob, T, 1, 2, pts, masks(7, 1), rbig + be(8)),   # a gamma >= r
             (1, 3, blob, T, 1, 2, pts, masks(7, 1), gms),           # worker outside the context
             (0, 1, blob, 2 * T, 1, 2, pts, masks(1, 1), gms),       # row longer than the slice
             (0, 1, blob, 3, 1, 2, pts, masks(1, 1), gms),           # evaluation form, not a power of two
             (0, 3, blob, 0, 1, 2, pts, masks(7, 1), gms)]           # T = 0
    for args in cases:
        assert lib.kzg_commit_open_multi(h, *args, c, e, p) == _native.KZG_E_ARG, args[:6]
        check(eng, srs, rows, [99, 98], [[0, 1, 2], [0]], [7, 8], True)


def test_threads_interleave_multi_batch_and_single_calls(hip):
    eng, srs = engine(hip, 12, 0, 0)
    T = 1 << 12
    rows = make_rows(T, 5, 5151)
    alpha, beta, gamma, delta = be(31337), be(4242), be(271828), be(161803)
    opened = [[0, 1, 2, 3, 4], [1, 4]]
    want_m = eng.commit_open_multi(0, rows, [alpha, beta], opened, [gamma, delta])
    assert want_m[2][1] == oc.open_(srs, combine([rows[1], rows[4]], 161803), beta, True, threads=TH)[1]
    want_b = eng.commit_open_batch(0, rows, alpha, gamma)
    want_s = [eng.commit_open(0, r, alpha) for r in rows]
    errors = []

    def work(t):
        try:
            for n in range(9):
                sel = (n + t) % 3
                if sel == 0:
                    assert eng.commit_open_multi(0, rows, [alpha, beta], opened, [gamma, delta]) == want_m
                elif sel == 1:
                    assert eng.commit_open_batch(0, rows, alpha, gamma) == want_b
                else:
                    j = (n + t) % len(rows)
                    assert eng.commit_open(0, rows[j], alpha) == want_s[j]
        except Exception as ex:   # noqa: BLE001
            errors.append(repr(ex))

    ths = [threading.Thread(target=work, args=(t,)) for t in range(8)]
    for x in ths:
        x.start()
    for x in ths:
        x.join()
    assert not errors, errors


def test_multi_handle_and_multi_device_client(hip):
    from zkp_subnet_amd import MultiDeviceClient, codec
    from zkp_subnet_amd.client import derive_taus
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
        for i in range(M):
            rows = make_rows(T, 4, 600 + i)
            C, Y, P = single.commit_open_multi(i, rows, pts, opened, gms)
            assert lib.kzg_multi_commit_open_multi(mh, i, 4, b"".join(rows), T, 1, 2, b"".join(pts), masks, b"".join(gms),
                                                   c, e, p) == 0, i
            assert [c.raw[48 * j:48 * j + 48] for j in range(4)] == C
            assert [e.raw[32 * t:32 * t + 32] for t in range(6)] == Y[0] + Y[1]
            assert [p.raw[:48], p.raw[48:]] == P
        assert lib.kzg_multi_commit_open_multi(mh, M, 4, b"".join(rows), T, 1, 2, b"".join(pts), masks, b"".join(gms),
                                               c, e, p) == _native.KZG_E_ARG
    finally:
        lib.kzg_multi_destroy(mh)

    multi = MultiDeviceClient(devices=[0, 0], seed=77)
    multi.start(scale=scale, machines_scale=ms)
    try:
        txb, tyb = (t.to_bytes(32, "big") for t in derive_taus(77))
        xs = [codec.be32_to_fr(be(8080)), codec.be32_to_fr(be(8081))]
        gs = [codec.be32_to_fr(be(9090)), codec.be32_to_fr(be(9091))]
        opened = [[0, 1, 2], [1]]
        for i in range(M):
            rows = make_rows(T, 3, 700 + i)
            polys = [codec.be32_to_fr_list(r) for r in rows]
            r = multi.worker_commit_open_multi(i, polys, xs, opened, gs)
            assert r.status_code == 200, r.json()
            srs = oc.srs_gen(txb, tyb, scale, ms, i)
            body = r.json()
            assert [codec.g1_from_b64(cm) for cm in body["commitments"]] == [oc.commit(srs, rw, True) for rw in rows]
            assert [[codec.fr_to_be32(ev) for ev in evs] for evs in body["evals"]] == \
                [[oracle_eval(rows[j], be(a), True) for j in js] for a, js in zip((8080, 8081), opened)]
            assert [codec.g1_from_b64(pf) for pf in body["proofs"]] == \
                [oc.open_(srs, combine(rows, 9090), be(8080), True)[1], oc.open_(srs, rows[1], be(8081), True)[1]]
            v = multi.worker_verify_open_multi(i, body["proofs"], xs, opened, gs, body["evals"], body["commitments"])
            assert v.status_code == 200 and v.json() == {"valid": True}
            v = multi.worker_verify_open_multi(i, body["proofs"], xs, opened, [codec.be32_to_fr(be(9092)), gs[1]],
                                               body["evals"], body["commitments"])
            assert v.json() == {"valid": False}
        assert multi.worker_commit_open_multi(0, [polys[0], polys[1][:-1]], xs, opened, gs).status_code == 400
        assert multi.worker_commit_open_multi(0, polys, xs, [[0, 1, 2], [3]], gs).status_code == 400
    finally:
        multi.stop()


def test_client_from_text_equals_engine_bytes(hip):
    from zkp_subnet_amd import codec
    from zkp_subnet_amd.client import Client

    cl = Client(seed=99)
    cl.start(scale=12, machines_scale=1)
    try:
        T = 1 << 11
        rows = make_rows(T, 4, 808)
        polys = [codec.be32_to_fr_list(r) for r in rows]
        pts = [be(1234567), be(1234568), be(1234569)]
        gms = [be(7654321), be(7654322), be(7654323)]
        opened = [[0, 1, 2, 3], [3], [0, 2]]
        X, G = [codec.be32_to_fr(x) for x in pts], [codec.be32_to_fr(g) for g in gms]
        r = cl.worker_commit_open_multi(1, polys, X, opened, G)
        assert r.status_code == 200, r.json()
        C, Y, P = cl.engine.commit_open_multi(1, rows, pts, opened, gms)
        body = r.json()
        assert [codec.g1_from_b64(c) for c in body["commitments"]] == C
        assert [[codec.fr_to_be32(e) for e in ev] for ev in body["evals"]] == Y
        assert [codec.g1_from_b64(p) for p in body["proofs"]] == P
        assert cl.worker_commit_open_multi(1, polys * 4 + polys[:1], X, opened, G).status_code == 400   # k = 17
        assert cl.worker_commit_open_multi(1, [], X, opened, G).status_code == 400
        assert cl.worker_commit_open_multi(1, polys, X * 2, opened * 2, G * 2).status_code == 400   # m = 6
        assert cl.worker_commit_open_multi(1, polys, X, [[0, 1, 2, 3], [], [0, 2]], G).status_code == 400
    finally:
        cl.stop()
