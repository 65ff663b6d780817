"""GPU tests (`-m gpu`) of kzg_rows_commit_quotient: the PLONK quotient pieces built on the device from committed row sets.
The expected t comes from the definition by another route (tests/quotient_ref.py: plain-domain products through the C
oracle's NTT, synthetic division) and is committed with the C oracle, never with the library under test: piece commitments
and evaluations are compared bit for bit; the whole round opens and verifies and the quotient identity holds at zeta; other
shapes, the unsatisfied instance, every documented error, threads, a racing release, the multi-GPU handle and one large row
through the SRS trapdoor follow.  Each test leaves rows_stats() where it found it."""
import ctypes
import random
import threading

import pytest

from oracle import cpu as oc
from tests import grand_product_ref as gp
from tests import quotient_ref as qr
from tests.gpu_common import val
from tests.gpu_rows import (arg_error, b_perm, b_terms, check_pieces, commit_sets, engine_cache, q_call, reference_pieces,
                            release, srs_cache, standard)
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import lagrange_factor

pytestmark = pytest.mark.gpu
R = gp.R
be, row_bytes = gp.be, gp.row_bytes
SEED_X, SEED_Y = 0x7A0D01, 0x7A0D02


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def num_at(vals, terms, perm, x, zw, T):
    """num(x) from the rows' values at x (vals, integers) and z(w x)"""
    acc = 0
    for c, idx in terms:
        p = c
        for j in idx:
            p = p * vals[j] % R
        acc += p
    if perm:
        beta, gamma, alpha = perm["beta"], perm["gamma"], perm["alpha"]
        A, B = vals[perm["z"]], zw
        for a, s, sh in zip(perm["wires"], perm["sigmas"], perm["shifts"]):
            A = A * (vals[a] + beta * sh % R * x + gamma) % R
            B = B * (vals[a] + beta * vals[s] + gamma) % R
        l0 = (pow(x, T, R) - 1) * pow(T * (x - 1) % R, -1, R) % R
        acc += alpha * (A - B) + alpha * alpha % R * (vals[perm["z"]] - 1) % R * l0
    return acc % R


@pytest.mark.parametrize("lg", [4, 10, 12, 16])
def test_standard_plonk_bit_exact_and_the_whole_round(engines, srs_of, lg):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(300 + lg)
    rows, terms, perm, want = standard(lg)
    assert qr.degree(sum(want, [])) == 3 * T - 4
    for ef, sizes in ((True, (13,)), (True, (3, 5, 3, 2)), (False, (13,)), (False, (3, 5, 3, 2))):
        sets = commit_sets(eng, rows, sizes, ef)
        try:
            tset = q_call(eng, sets, terms, perm, 2, 3)
            try:
                assert eng.rows_stats()[0] == before[0] + len(sets) + 1
                assert (tset.i, tset.T, tset.k) == (0, T, 3)
                check_pieces(eng, srs, tset, want, rnd)
                # the whole round: 13 rows and 3 pieces at zeta, z at zeta w; verify; the quotient identity from the answers
                zeta = rnd.randrange(R)
                P = [be(zeta), be(zeta * gp.omega(T))]
                allsets = sets + [tset]
                C = [c for s in allsets for c in s.commitments]
                opened, G = [list(range(16)), [qr.Z_]], [be(rnd.randrange(R)), be(rnd.randrange(R))]
                Y, Pf = eng.open_rows(allsets, P, opened, G)
                assert eng.verify_open_multi(0, C, P, opened, G, Y, Pf)
                vals = [val(y) for y in Y[0]]
                tz = sum(pow(zeta, p * T, R) * vals[13 + p] for p in range(3)) % R
                assert tz * (pow(zeta, T, R) - 1) % R == num_at(vals[:13], terms, perm, zeta, val(Y[1][0]), T)
            finally:
                tset.release()
        finally:
            release(sets)
    assert eng.rows_stats() == before


def vanishing_row(T, f, rows):
    """the evaluation row -f(rows at t) on the domain"""
    return [-f(*[r[t] for r in rows]) % R for t in range(T)]


def test_other_shapes(engines, srs_of):
    lg = 8
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(41)
    rr = lambda: [rnd.randrange(R) for _ in range(T)]   # noqa: E731
    # gate only (k = 0), E = 2, P = 1, with a constant term: a b + c + 5 = 0 on the domain
    a, b = rr(), rr()
    rows = [a, b, vanishing_row(T, lambda x, y: x * y + 5, [a, b])]
    terms = [(1, [0, 1]), (1, [2]), (5, [])]
    cases = [(rows, terms, None, 1, 1)]
    # a degree-5 custom term over one repeated row index, E = 4, P = 4: 3 a^5 + q = 0
    rows5 = [a, vanishing_row(T, lambda x: 3 * pow(x, 5, R), [a])]
    cases.append((rows5, [(3, [0, 0, 0, 0, 0]), (1, [1])], None, 2, 4))
    # k = 4 wires, E = 8: the permutation part alone, then with a gate
    wires, sigmas, shifts = gp.permutation_instance(4, T, 17)
    beta, gamma, alpha = rnd.randrange(R), rnd.randrange(R), rnd.randrange(R)
    z, closing = gp.grand_product(wires, sigmas, shifts, beta, gamma)
    assert closing == 1
    perm4 = {"wires": [0, 1, 2, 3], "sigmas": [4, 5, 6, 7], "z": 8, "shifts": shifts, "beta": beta, "gamma": gamma,
             "alpha": alpha}
    rows4 = wires + sigmas + [z]
    cases.append((rows4, [], perm4, 3, 4))
    rows4g = rows4 + [vanishing_row(T, lambda w, x, y, zz: w * x % R * y % R * zz, wires)]
    cases.append((rows4g, [(1, [0, 1, 2, 3]), (1, [9])], perm4, 3, 8))        # P = E: nothing checked, all pieces kept
    # zero and r - 1 challenges on the standard circuit
    for bt, gm, al in ((0, rnd.randrange(R), 0), (R - 1, R - 1, R - 1), (rnd.randrange(R), 0, 1), (0, 0, 0)):
        srows, sterms, sperm = qr.standard_instance(T, 23, bt, gm, al)
        cases.append((srows, sterms, sperm, 2, 3))
    for rows, terms, perm, ext_log, P in cases:
        want = reference_pieces(rows, terms, perm, ext_log, P)
        sets = commit_sets(eng, rows, (len(rows),))
        try:
            tset = q_call(eng, sets, terms, perm, ext_log, P)
            try:
                check_pieces(eng, srs, tset, want, rnd)
            finally:
                tset.release()
        finally:
            release(sets)
    # a repeated handle: the one-row set twice gives rows 0 and 1 = a, a; a a - sq = 0
    sq = [-x * x % R for x in a]
    sa, ss = commit_sets(eng, [a], (1,))[0], commit_sets(eng, [sq], (1,))[0]
    try:
        want = reference_pieces([a, a, sq], [(1, [0, 1]), (1, [2])], None, 1, 1)
        tset = q_call(eng, [sa, sa, ss], [(1, [0, 1]), (1, [2])], None, 1, 1)
        try:
            check_pieces(eng, srs, tset, want, rnd)
        finally:
            tset.release()
    finally:
        release([sa, ss])
    assert eng.rows_stats() == before


def test_unsatisfied_instance_creates_no_set(engines, srs_of):
    lg = 12
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(12)
    rows, terms, perm, want = standard(lg)
    broken = [list(r) for r in rows]
    broken[qr.QC][1234] = (broken[qr.QC][1234] + 1) % R
    good, bad = commit_sets(eng, rows, (13,)), commit_sets(eng, broken, (8, 5))
    try:
        live = eng.rows_stats()
        # ONE message for both causes: the device sees a nonzero coefficient above P T and cannot tell which it is
        msg = "the constraints do not hold on the domain, or n_pieces is too small"
        arg_error(lambda: q_call(eng, bad, terms, perm, 2, 3), msg)                 # one qC changed
        assert eng.rows_stats() == live
        arg_error(lambda: q_call(eng, good, terms, perm, 2, 2), msg)                # satisfied, but t needs three pieces
        assert eng.rows_stats() == live
        wrong_z = dict(perm, z=qr.A_)                                                # not the accumulator
        arg_error(lambda: q_call(eng, good, terms, wrong_z, 2, 3), msg)
        assert eng.rows_stats() == live
        tset = q_call(eng, good, terms, perm, 2, 3)
        try:
            check_pieces(eng, srs, tset, want, rnd)
        finally:
            tset.release()
    finally:
        release(good + bad)
    assert eng.rows_stats() == before


def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 8
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    srs = oc.srs_gen(be(SEED_X), be(SEED_Y), lg + 1, 1, 0)
    rows, terms, perm = qr.standard_instance(T, 5)
    want = [oc.commit(srs, row_bytes(p), False) for p in reference_pieces(rows, terms, perm, 2, 3)]

    def fresh_ok(sets):
        ts = q_call(eng, sets, terms, perm, 2, 3)
        ts.release()
        assert ts.commitments == want

    S = commit_sets(eng, rows, (3, 5, 3, 2))
    fresh_ok(S)
    bt, bp = b_terms(terms), b_perm(perm)
    call = lambda **kw: eng.commit_quotient(kw.get("sets", S), kw.get("terms", bt), kw.get("perm", bp),   # noqa: E731
                                            kw.get("ext_log", 2), kw.get("n_pieces", 3))
    lib = _native.load()
    hs = (ctypes.c_uint64 * 4)(*[s.handle for s in S])
    c, h = ctypes.create_string_buffer(48 * 8), ctypes.c_uint64(0)

    def raw(terms=bt, perm=bp, ext_log=2, n_pieces=3):
        """the C call itself, past the Python checks"""
        lens = (ctypes.c_uint32 * max(len(terms), 1))(*[len(r) for _, r in terms])
        flat = [j for _, r in terms for j in r]
        tr = (ctypes.c_uint32 * max(len(flat), 1))(*flat)
        gate = _native.QuotientGate(len(terms), b"".join(x for x, _ in terms), lens, tr)
        pm = None
        if perm:
            k = len(perm["wires"])
            pm = _native.QuotientPerm(k, perm["z"], (ctypes.c_uint32 * 16)(*perm["wires"]), (ctypes.c_uint32 * 16)(*perm["sigmas"]),
                                      b"".join(perm["shifts"]), perm["beta"], perm["gamma"], perm["alpha"])
        rc = lib.kzg_rows_commit_quotient(eng._h, 4, hs, ctypes.byref(gate), ctypes.byref(pm) if pm else None, ext_log,
                                          n_pieces, c, ctypes.byref(h))
        if rc == 0:
            eng.release_rows(h.value)
        return rc

    E_ARG = _native.KZG_E_ARG
    assert raw() == 0
    assert raw(ext_log=0) == E_ARG and raw(ext_log=4) == E_ARG
    assert raw(n_pieces=0) == E_ARG and raw(n_pieces=5) == E_ARG
    assert raw(terms=bt[:3] + [(be(1), [qr.QM] * 6)]) == E_ARG                       # six factors at E = 4
    assert raw(terms=[(be(1), [13])]) == E_ARG                                       # row index == n
    assert raw(terms=[(be(1), [2 ** 32 - 1])], perm=None) == E_ARG
    assert raw(terms=[], perm=None) == E_ARG                                         # nothing to compute
    assert raw(perm=dict(bp, z=13)) == E_ARG
    assert raw(perm=dict(bp, wires=[0, 1, 99])) == E_ARG
    assert raw(ext_log=1, n_pieces=1) == E_ARG                                       # k = 3 > E = 2
    big = R.to_bytes(32, "big")
    assert raw(terms=[(big, [0])] + bt[1:]) == E_ARG
    for name in ("beta", "gamma", "alpha"):
        assert raw(perm=dict(bp, **{name: big})) == E_ARG
    assert raw(perm=dict(bp, shifts=[be(1), b"\xff" * 32, be(3)])) == E_ARG
    assert raw(terms=bt * 3) == E_ARG                                                # 18 terms
    assert raw() == 0
    # the same through the Python layer, with the messages
    arg_error(lambda: call(ext_log=4))
    arg_error(lambda: call(n_pieces=5))
    arg_error(lambda: call(terms=[(be(1), [13])]), "row index")
    arg_error(lambda: call(perm=dict(bp, z=40)), "row index")
    arg_error(lambda: call(terms=[(big, [0])]), "canonical")
    arg_error(lambda: call(sets=S * 5))                                             # 20 handles
    arg_error(lambda: call(sets=S + S[:2]), "KZG_MAX_BATCH_OPEN rows")              # 13 + 3 + 5 rows
    other = commit_sets(eng, rows[:3], (3,), i=1)                                    # another worker
    arg_error(lambda: call(sets=S[:3] + other), "one worker")
    short = eng.commit_rows(0, [row_bytes(r[:T // 2]) for r in rows[:2]])            # another length
    arg_error(lambda: call(sets=S[:3] + [short]), "one worker and have one row length")
    release(other + [short])
    gone = commit_sets(eng, rows[11:], (2,))
    release(gone)
    arg_error(lambda: call(sets=S[:3] + gone), "released")
    arg_error(lambda: call(sets=S[:3] + [2 ** 40]), "unknown")
    fresh_ok(S)
    # the 65th live set
    fill = [eng.commit_rows(0, [row_bytes(rows[0])]) for _ in range(_native.KZG_MAX_ROW_SETS - 4)]
    assert eng.rows_stats()[0] == _native.KZG_MAX_ROW_SETS
    arg_error(lambda: call(), "KZG_MAX_ROW_SETS", code=_native.KZG_E_BUSY)
    fill.pop().release()
    fresh_ok(S)
    release(fill)
    # stale after an SRS load
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: call(), "SRS")
    release(S)
    S = commit_sets(eng, rows, (13,))
    fresh_ok(S)
    release(S)
    assert eng.rows_stats() == (0, 0)


def test_threads_and_a_racing_release(engines):
    lg = 12
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rows, terms, perm, _ = standard(lg)
    S = commit_sets(eng, rows, (11, 2))
    # (alpha alone may vary over a fixed z: the instance stays satisfied)
    chal = {t: dict(perm, alpha=5000 + t) for t in range(4)}
    want = {}
    for t, pm in chal.items():
        ts = q_call(eng, S, terms, pm)
        ts.release()
        want[t] = ts.commitments
    assert len({tuple(w) for w in want.values()}) == 4
    errors = []

    def work(t):
        try:
            for _ in range(3):
                ts = q_call(eng, S, terms, chal[t])
                ts.release()
                assert ts.commitments == want[t]
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
        victim = commit_sets(eng, rows[11:], (2,))[0]
        out = []

        def call():
            try:
                ts = q_call(eng, [S[0], victim], terms, chal[0])
                ts.release()
                out.append(ts.commitments)
            except KzgError as ex:
                out.append(ex.code)

        th = threading.Thread(target=call)
        th.start()
        if n % 2:
            threading.Event().wait(0.0002 * n)
        victim.release()
        th.join()
        assert out[0] in (want[0], _native.KZG_E_ARG), out
    release(S)
    assert eng.rows_stats() == before


def test_multi_handle_returns_the_context_bytes(hip):
    lib = _native.load()
    scale, ms = 10, 2
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
        c, cc = ctypes.create_string_buffer(48 * 3), ctypes.create_string_buffer(48 * 13)
        made = {}

        def args(terms, perm):
            bt, bp = b_terms(terms), b_perm(perm)
            lens = (ctypes.c_uint32 * len(bt))(*[len(r) for _, r in bt])
            flat = [j for _, r in bt for j in r]
            gate = _native.QuotientGate(len(bt), b"".join(x for x, _ in bt), lens, (ctypes.c_uint32 * len(flat))(*flat))
            pm = _native.QuotientPerm(3, bp["z"], (ctypes.c_uint32 * 3)(*bp["wires"]), (ctypes.c_uint32 * 3)(*bp["sigmas"]),
                                      b"".join(bp["shifts"]), bp["beta"], bp["gamma"], bp["alpha"])
            return gate, pm, (lens, flat)

        for i in range(M):
            rows, terms, perm = qr.standard_instance(T, 60 + i)
            S = commit_sets(single, rows, (13,), i=i)
            ts = single.commit_quotient(S, b_terms(terms), b_perm(perm))
            release(S + [ts])
            hr, ht = ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 13, b"".join(row_bytes(r) for r in rows), T, 1, cc, ctypes.byref(hr)) == 0
            gate, pm, keep = args(terms, perm)
            ah = (ctypes.c_uint64 * 1)(hr.value)
            assert lib.kzg_multi_rows_commit_quotient(mh, i, 1, ah, ctypes.byref(gate), ctypes.byref(pm), 2, 3, c,
                                                      ctypes.byref(ht)) == 0, i
            assert [c.raw[48 * p:48 * p + 48] for p in range(3)] == ts.commitments
            made[i] = (hr.value, ht.value, gate, pm, keep)
        # worker 3 shares worker 0's device, worker 1 lives elsewhere: both are refused under index 0
        for wrong in (3, 1):
            ah = (ctypes.c_uint64 * 1)(made[wrong][0])
            ht = ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit_quotient(mh, 0, 1, ah, ctypes.byref(made[wrong][2]), ctypes.byref(made[wrong][3]),
                                                      2, 3, c, ctypes.byref(ht)) == _native.KZG_E_ARG
        for i in range(M):
            for hh in made[i][:2]:
                assert lib.kzg_multi_rows_release(mh, i, hh) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)


def test_no_row_sized_copy_inside_the_call(engines):
    """structural: with stage profiling on, the call opens no upload span (only upload_fr opens KZG_T_DECODE), while the
    transforms, the pointwise kernels and the MSM pass's accumulate all ran"""
    lg = 12
    eng = engines(lg)
    before = eng.rows_stats()
    rows, terms, perm, _ = standard(lg)
    S = commit_sets(eng, rows, (13,))
    lib = _native.load()
    try:
        plain = q_call(eng, S, terms, perm)
        plain.release()
        assert lib.kzg_set_profiling(eng._h, 1) == 0
        try:
            ts = q_call(eng, S, terms, perm)
            ts.release()
            tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
            assert lib.kzg_get_timings(eng._h, tms, len(tms)) == 0
        finally:
            assert lib.kzg_set_profiling(eng._h, 0) == 0
        t = dict(zip(_native.TIMING_NAMES, tms))
        print("quotient stage times (ms):", {k: round(v, 4) for k, v in t.items()})
        assert t["decode"] == 0
        assert t["ntt"] > 0 and t["poly"] > 0 and t["accumulate"] > 0
        assert ts.commitments == plain.commitments
    finally:
        release(S)
    assert eng.rows_stats() == before


def test_large_row_through_the_trapdoor(engines):
    """2^18 rows, E = 4 (a work domain of 2^20 points).  The reference of the sweep would take minutes here, so the pieces are
    checked through the synthetic SRS's trapdoor tau: commitment p must be [s0 t_p(tau)] G for the piece's value at tau, and
    sum_p tau^(pT) t_p(tau) (tau^T - 1) must equal num(tau) computed from the ORACLE's evaluations of the input rows -- tau is
    a point the device never sees, so by Schwartz-Zippel the pieces are t's."""
    lg = 18
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rows, terms, perm = qr.standard_instance(T, 18)
    tau = SEED_X + lg
    S = commit_sets(eng, rows, (13,))
    try:
        tset = q_call(eng, S, terms, perm, 2, 3)
        try:
            coef = [oc.fr_ntt(row_bytes(r), True) for r in rows]
            vals = [val(oc.fr_eval(c, be(tau))) for c in coef]
            zw = val(oc.fr_eval(coef[qr.Z_], be(tau * gp.omega(T))))
            tp = [val(y) for y in eng.eval_rows([tset], [be(tau)], [[0, 1, 2]])[0]]
            s0 = lagrange_factor(0, 0, SEED_Y)
            for p in range(3):
                assert tset.commitments[p] == oc.g1_mul_gen(be(s0 * tp[p])), p
            tz = sum(pow(tau, p * T, R) * tp[p] for p in range(3)) % R
            assert tz * (pow(tau, T, R) - 1) % R == num_at(vals, terms, perm, tau, zw, T)
        finally:
            tset.release()
    finally:
        release(S)
    assert eng.rows_stats() == before
