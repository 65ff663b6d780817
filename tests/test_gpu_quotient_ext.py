"""GPU tests (`-m gpu`) of kzg_rows_commit_quotient_ext: the quotient with rotated gate factors and the logUp relation,
built on the device from committed row sets.  The expected t comes from the definition by another route
(tests/quotient_ext_ref.py: plain-domain products, a rotation as a change of argument, LK1 and LK2 written out, synthetic
division) and is committed with the C oracle, never with the library under test.  Equivalence with the plain call byte for
byte; rotations; the lookup shapes with S built on the device and from the reference; the whole round of the 16-row
circuit; one case on the transform's large path checked through the quotient identity; unsatisfied instances; every
documented error; threads; the multi-GPU handle.  Each test leaves rows_stats() where it found it."""
import ctypes
import functools
import random
import threading

import pytest

from oracle import cpu as oc
from tests import grand_product_ref as gp
from tests import lookup_ref as lr
from tests import quotient_ext_ref as qx
from tests import quotient_ref as qr
from tests.gpu_common import val
from tests.gpu_rows import (arg_error, b_lookup, b_perm, b_terms, c_args, check_pieces, commit_sets, engine_cache, q_call,
                            reference_pieces_ext as reference_pieces, release, srs_cache, standard, x_call)
from zkp_subnet_amd import _native
from zkp_subnet_amd.engine import lagrange_factor

pytestmark = pytest.mark.gpu
R = gp.R
be, row_bytes = gp.be, gp.row_bytes
E_ARG = _native.KZG_E_ARG
SEED_X, SEED_Y = 0x7A0D01, 0x7A0D02         # those of tests/test_gpu_quotient.py: the two modules' contexts hold the same SRS
SHAPE_MSG = "the constraints do not hold on the domain, or n_pieces is too small"


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


# ---------------------------------------------------------------------------------------------------- equivalence
@pytest.mark.parametrize("lg", [4, 10])
def test_no_rotation_and_no_lookup_is_the_plain_call(engines, lg):
    eng = engines(lg)
    before = eng.rows_stats()
    rows, terms, perm, _ = standard(lg)
    S = commit_sets(eng, rows, (3, 5, 3, 2))
    lib = _native.load()
    try:
        plain = q_call(eng, S, terms, perm, 2, 3)
        plain.release()
        zero = x_call(eng, S, [(c, [(j, 0) for j in idx]) for c, idx in terms], perm, None, 2, 3)   # every rot 0
        zero.release()
        assert zero.commitments == plain.commitments and (zero.k, zero.T) == (3, 1 << lg)
        hs = (ctypes.c_uint64 * 4)(*[s.handle for s in S])
        c, h = ctypes.create_string_buffer(48 * 3), ctypes.c_uint64(0)
        gate, pm, lk, _keep = c_args(b_terms(terms), b_perm(perm), None, rots=False)                # term_rots NULL
        assert lib.kzg_rows_commit_quotient_ext(eng._h, 4, hs, gate, pm, lk, 2, 3, c, ctypes.byref(h)) == 0
        eng.release_rows(h.value)
        assert [c.raw[48 * p:48 * p + 48] for p in range(3)] == plain.commitments
    finally:
        release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- rotations
TRIPLE = (3, [(qx.A_, 1), (qx.A_, -1), (qx.A_, 0)])   # one row at three rotations in one term


@functools.lru_cache(maxsize=None)
def rotated_cases(lg):
    """(rows, terms, terms with the rotations given past T, ext_log, P, expected pieces): the next-row gate at E = 2, and at
    E = 4 with the term 3 a(wX) a(w^-1 X) a(X) added (q solved for it too)"""
    T = 1 << lg
    rows = qx.next_row_instance(T, 70 + lg)
    a, q = rows[qx.A_], rows[qx.Q_]
    rows3 = rows[:3] + [[(q[t] - 3 * a[(t + 1) % T] * a[(t - 1) % T] % R * a[t]) % R for t in range(T)]]
    t1, t1w = qx.next_row_terms(), qx.next_row_terms(T, wrapped=True)
    tw3 = (3, [(qx.A_, T + 1), (qx.A_, T - 1), (qx.A_, -T)])
    return [(rows, t1, t1w, 1, 1, reference_pieces(rows, t1, None, None, 1, 1)),
            (rows3, t1 + [TRIPLE], t1w + [tw3], 2, 2, reference_pieces(rows3, t1 + [TRIPLE], None, None, 2, 2))]


@pytest.mark.parametrize("lg", [4, 8, 12])
def test_rotated_gate_bit_exact(engines, srs_of, lg):
    eng, srs = engines(lg), srs_of(lg)
    before = eng.rows_stats()
    rnd = random.Random(500 + lg)
    for rows, terms, wrapped, ext_log, P, want in rotated_cases(lg):
        for ef, sizes in ((True, (4,)), (False, (1, 2, 1))):
            sets = commit_sets(eng, rows, sizes, ef)
            try:
                tset = x_call(eng, sets, terms, None, None, ext_log, P)
                try:
                    check_pieces(eng, srs, tset, want, rnd)
                    again = x_call(eng, sets, wrapped, None, None, ext_log, P)   # T + 1, T - 1, T + 2: the same bytes
                    again.release()
                    assert again.commitments == tset.commitments
                finally:
                    tset.release()
            finally:
                release(sets)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the lookup part
@pytest.mark.parametrize("lg", [4, 8])
@pytest.mark.parametrize("L,w,ext_log,P", [(1, 1, 1, 2), (3, 2, 2, 4), (2, 3, 2, 3), (7, 1, 3, 8)])
def test_lookup_shapes_bit_exact(engines, srs_of, lg, L, w, ext_log, P):
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(600 + lg + L)
    rows, lookup = qx.lookup_rows(L, w, T, 80 + lg + L)
    want = reference_pieces(rows, [], None, lookup, ext_log, P)
    ins, tab, m, s_ref = commit_sets(eng, rows, (L * w, w, 1, 1))
    try:
        s_dev, closing = eng.commit_lookup_sum([ins], [tab], m, L, w, be(lookup["theta"]), be(lookup["beta"]))
        try:
            assert val(closing) == 0 and s_dev.commitments == s_ref.commitments
            for s_set in (s_dev, s_ref):           # S built on the device, S committed from the reference's evaluations
                tset = x_call(eng, [ins, tab, m, s_set], [], None, lookup, ext_log, P)
                try:
                    check_pieces(eng, srs, tset, want, rnd)
                finally:
                    tset.release()
        finally:
            s_dev.release()
    finally:
        release([ins, tab, m, s_ref])
    assert eng.rows_stats() == before


def identity_holds(eng, allsets, tset, terms, perm, lookup, T, rnd, rots):
    """t(zeta) (zeta^T - 1) == num(zeta) from the library's evaluations of the source rows at zeta w^rot (rot in rots, at
    most 4) and of the pieces at zeta"""
    zeta, w = rnd.randrange(R), gp.omega(T)
    n = sum(s.k for s in allsets)
    pts = [be(zeta * pow(w, rot % T, R) % R) for rot in rots]
    Y = eng.eval_rows(allsets, pts, [list(range(n))] * len(pts))
    tp = [val(y) for y in eng.eval_rows([tset], [be(zeta)], [list(range(tset.k))])[0]]
    at = lambda j, rot: val(Y[rots.index(rot)][j])   # noqa: E731
    tz = sum(pow(zeta, p * T, R) * v for p, v in enumerate(tp)) % R
    return tz * (pow(zeta, T, R) - 1) % R == qx.num_at(at, terms, perm, lookup, zeta, T)


def test_the_whole_round_of_the_16_row_circuit(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(77)
    rows, terms, perm, lookup = qx.round_instance(T, 4)
    want = reference_pieces(rows, terms, perm, lookup, 2, 3)
    assert qr.degree(sum(want, [])) == 3 * T - 4
    src = commit_sets(eng, rows[:15], (2, 1, 10, 1, 1))           # a b | c | the other ten | table | m
    try:
        s_set, closing = eng.commit_lookup_sum([src[1]], [src[3]], src[4], 1, 1, be(lookup["theta"]), be(lookup["beta"]))
        allsets = src + [s_set]
        try:
            assert val(closing) == 0
            tset = x_call(eng, allsets, terms, perm, lookup, 2, 3)   # gate, permutation and lookup in one call
            try:
                check_pieces(eng, srs, tset, want, rnd)
                # every row at zeta, z and S also at zeta w; the pieces at zeta; both openings verify
                zeta = rnd.randrange(R)
                P = [be(zeta), be(zeta * gp.omega(T) % R)]
                opened, G = [list(range(16)), [qr.Z_, 15]], [be(rnd.randrange(R)), be(rnd.randrange(R))]
                Y, Pf = eng.open_rows(allsets, P, opened, G)
                assert eng.verify_open_multi(0, [c for s in allsets for c in s.commitments], P, opened, G, Y, Pf)
                Yt, Pt = eng.open_rows([tset], P[:1], [[0, 1, 2]], G[:1])
                assert eng.verify_open_multi(0, tset.commitments, P[:1], [[0, 1, 2]], G[:1], Yt, Pt)
                at = lambda j, rot: val(Y[1][opened[1].index(j)] if rot else Y[0][j])   # noqa: E731
                tz = sum(pow(zeta, p * T, R) * val(y) for p, y in enumerate(Yt[0])) % R
                assert tz * (pow(zeta, T, R) - 1) % R == qx.num_at(at, terms, perm, lookup, zeta, T)
            finally:
                tset.release()
        finally:
            s_set.release()
    finally:
        release(src)
    assert eng.rows_stats() == before


def test_large_transform_path_through_the_identity(engines):
    """T = 2^16, E = 4: N = 2^18, the size from which the transform's large path runs.  A three-row next-row gate
    a(wX) b(X) + a(w^-1 X) + q(X) = 0 and one lookup of b in a shuffle of b.  No Python reference at this size: the shape
    check passed (P = 2 < E), and t(zeta) (zeta^T - 1) = num(zeta) from the library's own evaluations at a random zeta."""
    lg = 16
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(1616)
    a, b = ([rnd.randrange(R) for _ in range(T)] for _ in range(2))
    q = [-(a[(t + 1) % T] * b[t] + a[t - 1]) % R for t in range(T)]
    table, mult = qx.shuffled_table(b, rnd)
    terms = [(1, [(0, 1), 1]), (1, [(0, -1)]), (1, [2])]
    lookup = {"inputs": [1], "table": [3], "mult": 4, "sum": 5, "width": 1, "theta": rnd.randrange(R), "beta": rnd.randrange(R),
              "alpha": rnd.randrange(R)}
    src = commit_sets(eng, [a, b, q, table, mult], (1, 1, 1, 1, 1))
    try:
        s_set, closing = eng.commit_lookup_sum([src[1]], [src[3]], src[4], 1, 1, be(lookup["theta"]), be(lookup["beta"]))
        try:
            assert val(closing) == 0
            tset = x_call(eng, src + [s_set], terms, None, lookup, 2, 2)
            try:
                assert (tset.k, tset.T) == (2, T)
                assert identity_holds(eng, src + [s_set], tset, terms, None, lookup, T, rnd, [0, 1, -1])
            finally:
                tset.release()
        finally:
            s_set.release()
    finally:
        release(src)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- unsatisfied instances
def test_unsatisfied_instances_create_no_set(engines):
    lg = 8
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    # an input tuple outside the table, L = 1, E = 4, P = 2: S is the broken sum's own (it does not close)
    ins, tab, mult = lr.lookup_instance(1, 2, T, 31)
    broken = lr.break_instance(ins, tab, 2, 32)
    _, lookup = qx.lookup_rows(1, 2, T, 31)                    # rows: f_0 f_1 | t_0 t_1 | m | S
    good, bad, tset, mset = commit_sets(eng, ins + broken + tab + [mult], (2, 2, 2, 1))
    made = []
    try:
        for src, closes in ((bad, False), (good, True)):
            s_set, closing = eng.commit_lookup_sum([src], [tset], mset, 1, 2, be(lookup["theta"]), be(lookup["beta"]))
            made.append(s_set)
            assert (val(closing) == 0) == closes
            live = eng.rows_stats()
            if closes:
                ts = x_call(eng, [src, tset, mset, s_set], [], None, lookup, 2, 2)
                ts.release()
            else:
                arg_error(lambda: x_call(eng, [src, tset, mset, s_set], [], None, lookup, 2, 2), SHAPE_MSG)
            assert eng.rows_stats() == live
        # a next-row gate broken in row T - 1 only: the row that reads rows 0 and 1 through the wrap
        rows = qx.next_row_instance(T, 33)
        rows[qx.Q_][T - 1] = (rows[qx.Q_][T - 1] + 1) % R
        sets = commit_sets(eng, rows, (4,))
        made += sets
        live = eng.rows_stats()
        arg_error(lambda: x_call(eng, sets, qx.next_row_terms(), None, None, 2, 1), SHAPE_MSG)
        assert eng.rows_stats() == live
    finally:
        release([good, bad, tset, mset] + made)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- documented errors
def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 8
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    srs = oc.srs_gen(be(SEED_X), be(SEED_Y), lg + 1, 1, 0)
    rows, terms, perm, lookup = qx.round_instance(T, 5)
    want = [oc.commit(srs, row_bytes(p), False) for p in reference_pieces(rows, terms, perm, lookup, 2, 3)]
    S = commit_sets(eng, rows, (3, 5, 3, 2, 3))
    bt, bp, bl = b_terms(terms), b_perm(perm), b_lookup(lookup)

    def fresh_ok():
        ts = eng.commit_quotient_ext(S, bt, bp, bl, 2, 3)
        ts.release()
        assert ts.commitments == want

    fresh_ok()
    lib = _native.load()
    hs = (ctypes.c_uint64 * 5)(*[s.handle for s in S])
    c, h = ctypes.create_string_buffer(48 * 8), ctypes.c_uint64(0)
    NONE = object()

    def raw(terms=bt, perm=bp, lookup=bl, ext_log=2, n_pieces=3, null=None):
        """the C call itself, past the Python checks; null: a field of the lookup part or of the gate set to NULL"""
        gate, pm, lk, keep = c_args(terms, None if perm is NONE else perm, None if lookup is NONE else lookup)
        if null:
            setattr(keep[2] if hasattr(keep[2], null) else keep[0], null, None)
        rc = lib.kzg_rows_commit_quotient_ext(eng._h, 5, hs, gate, pm, lk, ext_log, n_pieces, c, ctypes.byref(h))
        if rc == 0:
            eng.release_rows(h.value)
        return rc

    assert raw() == 0
    # the lookup part
    assert raw(lookup=dict(bl, inputs=[], L=0)) == E_ARG                              # L = 0
    assert raw(lookup=dict(bl, width=0, L=1)) == E_ARG                                # w = 0
    assert raw(lookup=dict(bl, inputs=[2] * 4)) == E_ARG                              # L = 4 > E - 1
    assert raw(lookup=dict(bl, inputs=[2] * 2), perm=NONE, ext_log=1, n_pieces=2) == E_ARG   # L = 2 > E - 1 = 1
    assert raw(lookup=dict(bl, inputs=[2] * 18, table=[13] * 6, width=6), ext_log=3) == E_ARG   # L w = 18 > 16
    for name in ("inputs", "table"):
        assert raw(lookup=dict(bl, **{name: [16]})) == E_ARG                          # row index == n
    for name in ("mult", "sum"):
        assert raw(lookup=dict(bl, **{name: 16})) == E_ARG
        assert raw(lookup=dict(bl, **{name: 2 ** 32 - 1})) == E_ARG
    big = R.to_bytes(32, "big")
    for name in ("theta", "beta", "alpha"):
        assert raw(lookup=dict(bl, **{name: big}), perm=NONE) == E_ARG
    assert raw(lookup=dict(bl, alpha=be(lookup["alpha"] ^ 1))) == E_ARG               # two alphas
    assert raw(terms=[], perm=NONE, lookup=NONE) == E_ARG                             # nothing to compute
    for name in ("input_rows", "table_rows", "theta_be32", "beta_be32", "alpha_be32", "coeffs_be32", "term_lens", "term_rows"):
        assert raw(null=name) == E_ARG, name
    # the old ones on the new entry point
    assert raw(ext_log=0) == E_ARG and raw(ext_log=4) == E_ARG
    assert raw(n_pieces=0) == E_ARG and raw(n_pieces=5) == E_ARG
    assert raw(terms=bt[:3] + [(be(1), [(qr.QM, 1)] * 6)]) == E_ARG                   # six factors at E = 4
    assert raw(terms=[(be(1), [(16, 1)])]) == E_ARG                                   # row index == n
    assert raw(terms=[(big, [0])] + bt[1:]) == E_ARG
    assert raw(perm=dict(bp, z=16)) == E_ARG
    assert raw(perm=dict(bp, gamma=big)) == E_ARG
    assert raw(terms=bt * 3) == E_ARG                                                 # 18 terms
    assert raw(perm=NONE, lookup=NONE, ext_log=1, n_pieces=1, terms=[(be(1), [(0, 1)] * 4)]) == E_ARG
    assert raw() == 0
    # through the Python layer, with the messages
    call = lambda **kw: eng.commit_quotient_ext(kw.get("sets", S), kw.get("terms", bt), kw.get("perm", bp),   # noqa: E731
                                                kw.get("lookup", bl), kw.get("ext_log", 2), kw.get("n_pieces", 3))
    arg_error(lambda: call(lookup=dict(bl, sum=40)), "row index")
    arg_error(lambda: call(terms=[(be(1), [(13, -1), (16, 0)])]), "row index")
    arg_error(lambda: call(lookup=dict(bl, theta=big)), "canonical")
    arg_error(lambda: call(lookup=dict(bl, alpha=be(1))), "one alpha")
    arg_error(lambda: call(lookup=dict(bl, inputs=[2] * 4)), "n_lookups")
    arg_error(lambda: call(lookup=dict(bl, sum=qr.A_)), SHAPE_MSG)                   # not the running sum
    arg_error(lambda: call(n_pieces=2), SHAPE_MSG)
    other = commit_sets(eng, rows[:3], (3,), i=1)                                     # another worker
    arg_error(lambda: call(sets=S[:4] + other), "one worker")
    short = eng.commit_rows(0, [row_bytes(r[:T // 2]) for r in rows[:3]])             # another length
    arg_error(lambda: call(sets=S[:4] + [short]), "one worker and have one row length")
    release(other + [short])
    gone = commit_sets(eng, rows[13:], (3,))
    release(gone)
    arg_error(lambda: call(sets=S[:4] + gone), "released")
    arg_error(lambda: call(sets=S[:4] + [2 ** 40]), "unknown")
    arg_error(lambda: call(sets=S + S[:1]), "KZG_MAX_BATCH_OPEN rows")
    fresh_ok()
    # stale after an SRS load
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: call(), "SRS")
    release(S)
    S = commit_sets(eng, rows, (16,))
    fresh_ok()
    release(S)
    assert eng.rows_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------------- threads
def test_four_threads_with_different_calls(engines):
    lg = 10
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rows, terms, perm, lookup = qx.round_instance(T, 6)
    gate_rows = qx.next_row_instance(T, 7)
    S, G = commit_sets(eng, rows, (13, 3)), commit_sets(eng, gate_rows, (4,))
    # four different calls (alpha may vary over fixed z and S: the instance stays satisfied)
    calls = {0: lambda: x_call(eng, S, terms, perm, lookup, 2, 3),
             1: lambda: x_call(eng, S, terms, dict(perm, alpha=9001), dict(lookup, alpha=9001), 2, 3),
             2: lambda: x_call(eng, S, [], None, dict(lookup, alpha=9002), 1, 2),
             3: lambda: x_call(eng, G, qx.next_row_terms(), None, None, 1, 1)}
    want = {}
    for t, fn in calls.items():
        ts = fn()
        ts.release()
        want[t] = ts.commitments
    assert len({tuple(w) for w in want.values()}) == 4
    errors = []

    def work(t):
        try:
            for _ in range(3):
                ts = calls[t]()
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
    release(S + G)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the multi handle
def test_multi_handle_returns_the_context_bytes(hip):
    lib = _native.load()
    scale, ms = 6, 2
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
        c, cc = ctypes.create_string_buffer(48 * 2), ctypes.create_string_buffer(48 * 8)
        made = {}
        for i in range(M):
            gate_rows = qx.next_row_instance(T, 90 + i)
            lk_rows, lookup = qx.lookup_rows(1, 1, T, 95 + i, first_row=4)
            rows, terms = gate_rows + lk_rows, qx.next_row_terms()
            S = commit_sets(single, rows, (8,), i=i)
            ts = x_call(single, S, terms, None, lookup, 2, 2)
            release(S + [ts])
            hr, ht = ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, 8, b"".join(row_bytes(r) for r in rows), T, 1, cc, ctypes.byref(hr)) == 0
            gate, pm, lk, keep = c_args(b_terms(terms), None, b_lookup(lookup))
            ah = (ctypes.c_uint64 * 1)(hr.value)
            assert lib.kzg_multi_rows_commit_quotient_ext(mh, i, 1, ah, gate, pm, lk, 2, 2, c, ctypes.byref(ht)) == 0, i
            assert [c.raw[48 * p:48 * p + 48] for p in range(2)] == ts.commitments
            made[i] = (hr.value, ht.value, gate, lk, keep)
        # worker 3 shares worker 0's device, worker 1 lives elsewhere: both are refused under index 0
        for wrong in (3, 1):
            ah = (ctypes.c_uint64 * 1)(made[wrong][0])
            ht = ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit_quotient_ext(mh, 0, 1, ah, made[wrong][2], None, made[wrong][3], 2, 2, c,
                                                          ctypes.byref(ht)) == E_ARG
        for i in range(M):
            for hh in made[i][:2]:
                assert lib.kzg_multi_rows_release(mh, i, hh) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)
