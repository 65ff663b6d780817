"""GPU tests (`-m gpu`) of the batched opening (kzg_commit_open_batch): k rows of one worker at one point alpha, one proof
for h = sum_j gamma^j f_j.  Every commitment, evaluation and proof is compared bit for bit with the C oracle (commit, open_
on h, fr_eval) or with the single-row paths that the oracle already pins, and every proof passes kzg_vk_verify_open_batch."""
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


def check(eng, srs, rows, alpha, gamma, ef, commits=None):
    """one batched call against the oracle; returns the oracle commitments (they do not depend on alpha / gamma)"""
    a, g = be(alpha), be(gamma)
    C, Y, P = eng.commit_open_batch(0, rows, a, g, ef)
    if commits is None:
        commits = [oc.commit(srs, r, ef, threads=TH) for r in rows]
    assert C == commits
    assert Y == [oracle_eval(r, a, ef) for r in rows]
    assert P == oc.open_(srs, combine(rows, gamma), a, ef, threads=TH)[1]
    assert eng.verify_open_batch(0, C, Y, a, g, P)
    return commits


@pytest.mark.parametrize("lg", [10, 16])
def test_k1_is_commit_open(hip, lg):
    eng, _ = engine(hip, lg, 0, 0)
    T = 1 << lg
    row = rand_scalars_bytes(T, 500 + lg)
    alpha = be(random.Random(lg).randrange(R))
    for ef in (True, False):
        c, y, p = eng.commit_open(0, row, alpha, ef)
        C, Y, P = eng.commit_open_batch(0, [row], alpha, be(random.Random(7).randrange(R)), ef)
        assert (C, Y, P) == ([c], [y], p)
        assert eng.verify_open_batch(0, C, Y, alpha, be(5), P)


@pytest.mark.parametrize("scale,ms,i,k", [(10, 2, 3, 3), (12, 0, 0, 2), (16, 4, 9, 4), (14, 0, 0, 7), (16, 0, 0, 16)])
def test_oracle_parity(hip, scale, ms, i, k):
    eng, srs = engine(hip, scale, ms, i)
    T = 1 << (scale - ms)
    rnd = random.Random(scale * 100 + k)
    rows = make_rows(T, k, 1000 * scale + k)
    alphas = [0, pow(_root_of_unity(T), 3, R), R - 1, rnd.randrange(R)]
    gammas = [0, 1, rnd.randrange(R)]
    full = T <= 1 << 12    # every (alpha, gamma) pair on short rows; four pairs covering both lists on the long ones
    pairs = [(a, g) for a in alphas for g in gammas] if full else list(zip(alphas, gammas + [rnd.randrange(R)]))
    for ef in (True, False):
        commits = None
        for a, g in pairs:
            commits = check(eng, srs, rows, a, g, ef, commits)


def test_gamma_zero_is_the_first_rows_proof(hip):
    eng, _ = engine(hip, 12, 0, 0)
    rows = make_rows(1 << 12, 4, 77)
    alpha = be(12345)
    _, _, P = eng.commit_open_batch(0, rows, alpha, be(0))
    assert P == eng.commit_open(0, rows[0], alpha)[2]


def test_long_rows_spread_over_lanes(hip):
    """T = 2^20 (past KZG_BATCHED_ROW_MAX): k + 1 single-set MSMs spread over two lanes; both single-row paths are
    oracle-pinned at this size."""
    eng, _ = engine(hip, 20, 0, 0)
    T = 1 << 20
    rows = make_rows(T, 3, 2020)
    rnd = random.Random(20)
    alpha, gamma = be(rnd.randrange(R)), rnd.randrange(R)
    for ef in (True, False):
        C, Y, P = eng.commit_open_batch(0, rows, alpha, be(gamma), ef)
        assert eng.commit_open_batch_joined(0, b"".join(rows), 3, alpha, be(gamma), ef) == (C, Y, P)
        h = combine(rows, gamma)
        assert P == eng.commit_open(0, h, alpha, ef)[2]
        assert C == [eng.commit(0, r, ef) for r in rows]
        assert Y == [eng.open(0, r, alpha, ef)[0] for r in rows]
        assert eng.verify_open_batch(0, C, Y, alpha, be(gamma), P)


@pytest.mark.parametrize("window,k", [(20, 8), (22, 3)])
def test_forced_window_splits_the_sets_over_passes(hip, window, k):
    """A wide forced window leaves the sort's key (or the bucket memory) room for fewer sets than k + 1: several passes."""
    eng, srs = engine(hip, 10, 0, 0, window=window)
    assert eng.window == window
    rows = make_rows(1 << 10, k, 3000 + window)
    rnd = random.Random(window)
    check(eng, srs, rows, rnd.randrange(R), rnd.randrange(R), True)


def test_argument_errors_leave_the_context_serving(hip):
    eng, srs = engine(hip, 10, 0, 0)
    lib, h = eng._lib, eng._h
    T = 1 << 10
    rows = make_rows(T, 3, 4242)
    blob = b"".join(rows)
    a, g = be(99), be(7)
    c, e, p = ctypes.create_string_buffer(48 * 17), ctypes.create_string_buffer(32 * 17), ctypes.create_string_buffer(48)
    cases = [(0, 0, blob, T, 1, a, g), (0, 17, blob * 6, T, 1, a, g), (0, 3, blob, T, 1, be(0)[:0] + R.to_bytes(32, "big"), g),
             (0, 3, blob, T, 1, a, R.to_bytes(32, "big")), (1, 3, blob, T, 1, a, g), (0, 1, blob, 2 * T, 1, a, g),
             (0, 1, blob, 3, 1, a, g), (0, 3, blob, 0, 1, a, g)]
    for args in cases:
        assert lib.kzg_commit_open_batch(h, *args, c, e, p) == _native.KZG_E_ARG, args
        check(eng, srs, rows, 99, 7, True)


def test_threads_interleave_batched_and_single_calls(hip):
    eng, srs = engine(hip, 12, 0, 0)
    T = 1 << 12
    rows = make_rows(T, 5, 5151)
    alpha, gamma = be(31337), 271828
    want_b = eng.commit_open_batch(0, rows, alpha, be(gamma))
    assert want_b[2] == oc.open_(srs, combine(rows, gamma), alpha, True, threads=TH)[1]
    want_s = [eng.commit_open(0, r, alpha) for r in rows]
    errors = []

    def work(t):
        try:
            for n in range(12):
                if (n + t) % 2:
                    assert eng.commit_open_batch(0, rows, alpha, be(gamma)) == want_b
                else:
                    j = (n + t) % len(rows)
                    assert eng.commit_open(0, rows[j], alpha) == want_s[j]
        except Exception as ex:   # noqa: BLE001
            errors.append(repr(ex))

    ths = [threading.Thread(target=work, args=(t,)) for t in range(4)]
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
    m = ctypes.c_void_p()
    assert lib.kzg_multi_create(G, devs, ctypes.byref(m)) == 0
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(m, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        a, g = be(4444), be(5555)
        c, e, p = ctypes.create_string_buffer(48 * 4), ctypes.create_string_buffer(32 * 4), ctypes.create_string_buffer(48)
        for i in range(M):
            rows = make_rows(T, 4, 600 + i)
            C, Y, P = single.commit_open_batch(i, rows, a, g)
            assert lib.kzg_multi_commit_open_batch(m, i, 4, b"".join(rows), T, 1, a, g, c, e, p) == 0, i
            assert ([c.raw[48 * j:48 * j + 48] for j in range(4)], [e.raw[32 * j:32 * j + 32] for j in range(4)], p.raw) \
                == (C, Y, P), i
        assert lib.kzg_multi_commit_open_batch(m, M, 4, b"".join(rows), T, 1, a, g, c, e, p) == _native.KZG_E_ARG
    finally:
        lib.kzg_multi_destroy(m)

    multi = MultiDeviceClient(devices=[0, 0], seed=77)
    multi.start(scale=scale, machines_scale=ms)
    try:
        txb, tyb = (t.to_bytes(32, "big") for t in derive_taus(77))
        x, gamma = codec.be32_to_fr(be(8080)), codec.be32_to_fr(be(9090))
        for i in range(M):
            rows = make_rows(T, 3, 700 + i)
            polys = [codec.be32_to_fr_list(r) for r in rows]
            r = multi.worker_commit_open_batch(i, polys, x, gamma)
            assert r.status_code == 200, r.json()
            srs = oc.srs_gen(txb, tyb, scale, ms, i)
            body = r.json()
            assert [codec.g1_from_b64(cm) for cm in body["commitments"]] == [oc.commit(srs, rw, True) for rw in rows]
            assert [codec.fr_to_be32(ev) for ev in body["evals"]] == [oracle_eval(rw, be(8080), True) for rw in rows]
            assert codec.g1_from_b64(body["proof"]) == oc.open_(srs, combine(rows, 9090), be(8080), True)[1]
            v = multi.worker_verify_open_batch(i, body["proof"], x, gamma, body["evals"], body["commitments"])
            assert v.status_code == 200 and v.json() == {"valid": True}
            v = multi.worker_verify_open_batch(i, body["proof"], x, codec.be32_to_fr(be(9091)), body["evals"],
                                               body["commitments"])
            assert v.json() == {"valid": False}
        bad = multi.worker_commit_open_batch(0, [polys[0], polys[1][:-1]], x, gamma)
        assert bad.status_code == 400
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
        x, gamma = be(1234567), be(7654321)
        r = cl.worker_commit_open_batch(1, polys, codec.be32_to_fr(x), codec.be32_to_fr(gamma))
        assert r.status_code == 200, r.json()
        C, Y, P = cl.engine.commit_open_batch(1, rows, x, gamma)
        body = r.json()
        assert [codec.g1_from_b64(c) for c in body["commitments"]] == C
        assert [codec.fr_to_be32(e) for e in body["evals"]] == Y
        assert codec.g1_from_b64(body["proof"]) == P
        assert cl.worker_commit_open_batch(1, polys + polys + polys + polys + polys[:1], codec.be32_to_fr(x),
                                           codec.be32_to_fr(gamma)).status_code == 400   # k = 17
        assert cl.worker_commit_open_batch(1, [], codec.be32_to_fr(x), codec.be32_to_fr(gamma)).status_code == 400
    finally:
        cl.stop()
