"""GPU tests (`-m gpu`) of the blinding-rows builders kzg_rows_commit_{grand_product,lookup_sum,multiplicities,quotient}_zk.
The expected rows come from the definitions in Python integers (tests/blinding_ref.py) and are committed with the C oracle,
never with the library under test: commitments, closing values, `missing` and evaluations are compared bit for bit.  Shapes:
the smallest at which the mask boundary and the scan levels can go wrong -- T = 2^5 with u over the whole range of the cap
(1, 2, 27: no multiple of the level-0 chunk of 4, 31), T = 2^10 with u = T - 6, T = 2^14 (two scan levels above the top) with
u = T - 32 and T - 1.  Then the zero denominator on either side of u, the quotient's equivalences and degree rules, the whole
hidden round through the Client, every documented error, threads, the multi-GPU handle and the structural check (no upload
span inside a call).  Each test leaves rows_stats() where it found it."""
import ctypes
import functools
import random
import threading

import pytest

from oracle import cpu as oc
from tests import blinding_ref as br
from tests import gpu_rows
from tests import grand_product_ref as gp
from tests import lookup_ref as lr
from tests import quotient_ref as qr
from tests.gpu_common import ints, val
from tests.gpu_rows import (arg_error, b_lookup, b_perm, b_terms, bt, c_args, check_one_row, check_pieces, commit_sets,
                            engine_cache, probes_closing, release, srs_cache, standard, tail_of, x_call, zk_call)
from zkp_subnet_amd import _native, codec
from zkp_subnet_amd.engine import lagrange_factor

pytestmark = pytest.mark.gpu
R = br.R
be, row_bytes = br.be, br.row_bytes
E_ARG = _native.KZG_E_ARG
SEED_X, SEED_Y = 0xB11D01, 0xB11D02
SHAPES = [(5, 1), (5, 2), (5, 27), (5, 31), (10, (1 << 10) - 6), (14, (1 << 14) - 32), (14, (1 << 14) - 1)]
shape_id = lambda s: f"T2^{s[0]}-u{s[1]}"   # noqa: E731
SHAPE_MSG = "the constraints do not hold on the domain, or n_pieces is too small"


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


rand_rows = functools.lru_cache(maxsize=None)(gpu_rows.rand_rows)   # the tests share rows and none of them writes to one


def check_row(eng, srs, rset, row, u, rnd):
    """the one-row set against the expected evaluations: the oracle's commitment, the values at w^u, w^(u+1), w^(T-1) and
    at a random point"""
    check_one_row(eng, srs, rset, row, rnd, probes=probes_closing(len(row), u))


# ---------------------------------------------------------------------------------------------------- the three builders
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_grand_product_zk_bit_exact(engines, srs_of, shape):
    lg, u = shape
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(100 * lg + u)
    k = 2
    wires, sigmas = rand_rows(k, T, 1000 * lg), rand_rows(k, T, 2000 * lg)
    shifts, beta, gamma = [1, 7], rnd.randrange(R), rnd.randrange(R)
    tail = tail_of(T, u, 31 * lg + u)
    z, closing = br.grand_product_zk(wires, sigmas, shifts, beta, gamma, u, tail)
    W, S = commit_sets(eng, wires, (k,)), commit_sets(eng, sigmas, (1, 1), ef=False)
    try:
        zset, cl = eng.commit_grand_product_zk(W, S, [be(s) for s in shifts], be(beta), be(gamma), u, bt(tail))
        try:
            assert cl == be(closing)
            check_row(eng, srs, zset, z, u, rnd)
            if u == T - 1:   # nothing masked but the last step and no tail: the plain call's row
                plain, _ = eng.commit_grand_product(W, S, [be(s) for s in shifts], be(beta), be(gamma))
                plain.release()
                assert plain.commitments == zset.commitments
        finally:
            zset.release()
    finally:
        release(W + S)
    assert eng.rows_stats() == before


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_lookup_sum_zk_bit_exact(engines, srs_of, shape):
    lg, u = shape
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(200 * lg + u)
    L, w = 2, 2
    inputs, table, mult = rand_rows(L * w, T, 3000 * lg), rand_rows(w, T, 4000 * lg), rand_rows(1, T, 5000 * lg)[0]
    theta, beta = rnd.randrange(R), rnd.randrange(R)
    tail = tail_of(T, u, 37 * lg + u)
    S, closing = br.lookup_sum_zk(inputs, table, mult, L, w, theta, beta, u, tail)
    F, Tb, M = commit_sets(eng, inputs, (1, 3)), commit_sets(eng, table, (w,), ef=False), commit_sets(eng, [mult], (1,))
    try:
        sset, cl = eng.commit_lookup_sum_zk(F, Tb, M[0], L, w, be(theta), be(beta), u, bt(tail))
        try:
            assert cl == be(closing)
            check_row(eng, srs, sset, S, u, rnd)
        finally:
            sset.release()
    finally:
        release(F + Tb + M)
    assert eng.rows_stats() == before


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_multiplicities_zk_bit_exact(engines, srs_of, shape):
    """a lookup that is satisfied on the usable rows; the padding cells hold tuples that are in no table row, and padding
    table rows repeat usable ones: neither is counted"""
    lg, u = shape
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(300 * lg + u)
    L, w = 2, 2
    inputs, table, _ = lr.lookup_instance(L, w, T, 6000 * lg, duplicates=True)
    inputs, table = [list(r) for r in inputs], [list(r) for r in table]
    for t in range(T):     # the usable cells look up usable table rows only
        for l in range(L):
            src = rnd.randrange(u) if t < u else None
            for c in range(w):
                inputs[l * w + c][t] = table[c][src] if t < u else rnd.randrange(R)
    for t in range(u, T):
        src = rnd.randrange(u)
        for c in range(w):
            table[c][t] = table[c][src] if t % 2 else rnd.randrange(R)
    tail = tail_of(T, u, 41 * lg + u)
    m, missing = br.multiplicities_zk(inputs, table, L, w, u, tail)
    assert missing == 0 and sum(m[:u]) == L * u
    F, Tb = commit_sets(eng, inputs, (L * w,)), commit_sets(eng, table, (1, 1), ef=False)
    try:
        mset, miss = eng.commit_multiplicities_zk(F, Tb, L, w, u, bt(tail))
        try:
            assert miss == 0
            check_row(eng, srs, mset, m, u, rnd)
        finally:
            mset.release()
        plain, miss_plain = eng.commit_multiplicities(F, Tb, L, w)       # the plain call does see the padding cells
        plain.release()
        assert miss_plain == L * (T - u)
        # one usable cell that is in no table row is counted, a padding one still is not
        broken = [list(r) for r in inputs]
        broken[0][u - 1] = (broken[0][u - 1] + 1) % R
        m2, missing2 = br.multiplicities_zk(broken, table, L, w, u, tail)
        assert missing2 == 1
        F2 = commit_sets(eng, broken, (L * w,))
        try:
            mset, miss = eng.commit_multiplicities_zk(F2, Tb, L, w, u, bt(tail))
            mset.release()
            assert miss == 1 and mset.commitments[0] == oc.commit(srs, row_bytes(m2), True)
        finally:
            release(F2)
    finally:
        release(F + Tb)
    assert eng.rows_stats() == before


def test_a_zero_denominator_counts_only_on_usable_rows(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    u = T - 6
    before = eng.rows_stats()
    rnd = random.Random(77)
    wires, sigmas = rand_rows(2, T, 7100), rand_rows(2, T, 7200)
    inputs, table, mult = rand_rows(2, T, 7300), rand_rows(1, T, 7400), rand_rows(1, T, 7500)[0]
    shifts, beta, theta = [1, 7], rnd.randrange(R), rnd.randrange(R)
    zt, st = tail_of(T, u, 71), tail_of(T, u, 72)
    W, Sg = commit_sets(eng, wires, (2,)), commit_sets(eng, sigmas, (2,))
    F, Tb, M = commit_sets(eng, inputs, (2,)), commit_sets(eng, table, (1,)), commit_sets(eng, [mult], (1,))
    bs = [be(s) for s in shifts]
    try:
        live = eng.rows_stats()
        for t, usable_row in ((u, False), (T - 1, False), (u - 1, True), (0, True), (517, True)):
            gamma = -(wires[1][t] + beta * sigmas[1][t]) % R          # D_t = 0
            lbeta = -inputs[1][t] % R                                  # beta + F_2(w^t) = 0 (L = 2, w = 1)
            arg_error(lambda: eng.commit_grand_product(W, Sg, bs, be(beta), be(gamma)), "zero denominator")
            arg_error(lambda: eng.commit_lookup_sum(F, Tb, M[0], 2, 1, be(theta), be(lbeta)), "zero denominator")
            if usable_row:
                arg_error(lambda: eng.commit_grand_product_zk(W, Sg, bs, be(beta), be(gamma), u, bt(zt)), "zero denominator")
                arg_error(lambda: eng.commit_lookup_sum_zk(F, Tb, M[0], 2, 1, be(theta), be(lbeta), u, bt(st)),
                           "zero denominator")
                assert eng.rows_stats() == live                        # no set was created
                continue
            z, closing = br.grand_product_zk(wires, sigmas, shifts, beta, gamma, u, zt)
            zset, cl = eng.commit_grand_product_zk(W, Sg, bs, be(beta), be(gamma), u, bt(zt))
            zset.release()
            assert (zset.commitments[0], cl) == (oc.commit(srs, row_bytes(z), True), be(closing))
            S, closing = br.lookup_sum_zk(inputs, table, mult, 2, 1, theta, lbeta, u, st)
            sset, cl = eng.commit_lookup_sum_zk(F, Tb, M[0], 2, 1, be(theta), be(lbeta), u, bt(st))
            sset.release()
            assert (sset.commitments[0], cl) == (oc.commit(srs, row_bytes(S), True), be(closing))
            assert eng.rows_stats() == live
    finally:
        release(W + Sg + F + Tb + M)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the quotient
def raw_zk(lib, eng, sets, terms, perm, lookup, active, ext_log, P):
    """kzg_rows_commit_quotient_zk itself (active: a row index, or None for a NULL pointer) -> (status, commitments)"""
    hs = (ctypes.c_uint64 * len(sets))(*[s.handle for s in sets])
    c, h = ctypes.create_string_buffer(48 * P), ctypes.c_uint64(0)
    gate, pm, lk, _keep = c_args(b_terms(terms), b_perm(perm), b_lookup(lookup))
    act = _native.QuotientActive(active) if active is not None else None
    rc = lib.kzg_rows_commit_quotient_zk(eng._h, len(sets), hs, gate, pm, lk, ctypes.byref(act) if act is not None else None,
                                         ext_log, P, c, ctypes.byref(h))
    if rc == 0:
        eng.release_rows(h.value)
    return rc, [c.raw[48 * p:48 * p + 48] for p in range(P)]


@pytest.mark.parametrize("lg", [5, 10])
def test_without_active_and_with_an_all_ones_column_it_is_the_ext_call(engines, lg):
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rows, terms, perm, _ = standard(lg)                     # 13 rows, k = 3 = E - 1 at ext_log = 2
    S = commit_sets(eng, rows + [[1] * T], (3, 5, 3, 2, 1))
    lib = _native.load()
    try:
        ext = x_call(eng, S, terms, perm, None, 2, 3)
        ext.release()
        rc, cs = raw_zk(lib, eng, S, terms, perm, None, None, 2, 3)         # active == NULL
        assert rc == 0 and cs == ext.commitments
        ones = zk_call(eng, S, terms, perm, None, 13, 2, 3)                 # A = 1 everywhere
        ones.release()
        assert ones.commitments == ext.commitments and (ones.k, ones.T) == (3, T)
        rc, cs = raw_zk(lib, eng, S, terms, perm, None, 13, 2, 3)
        assert rc == 0 and cs == ext.commitments
    finally:
        release(S)
    assert eng.rows_stats() == before


def test_degree_rules_with_an_active_column(engines):
    lg = 5
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rows, terms, perm, _ = standard(lg)
    S = commit_sets(eng, rows + [[1] * T], (14,))
    lib = _native.load()
    try:
        live = eng.rows_stats()
        # k = E: legal without the column (ext_log = 2 takes 4 wires), KZG_E_ARG with it
        four = dict(perm, wires=perm["wires"] + [qr.A_], sigmas=perm["sigmas"] + [qr.S1], shifts=perm["shifts"] + [1])
        rc, _ = raw_zk(lib, eng, S, terms, four, None, 13, 2, 4)
        assert rc == E_ARG and b"k + 2 factors" in lib.kzg_last_error(eng._h)
        rc, _ = raw_zk(lib, eng, S, terms, perm, None, 13, 2, 3)            # k = E - 1: accepted
        assert rc == 0
        # L = E - 1: legal without the column, KZG_E_ARG with it (refused before the rows are looked at)
        lookup = {"inputs": [0], "table": [1], "mult": 2, "sum": 3, "width": 1, "theta": 5, "beta": 6, "alpha": perm["alpha"]}
        rc, _ = raw_zk(lib, eng, S, [], None, lookup, 13, 1, 2)
        assert rc == E_ARG and b"n_lookups + 3 factors" in lib.kzg_last_error(eng._h)
        rc, _ = raw_zk(lib, eng, S, terms, perm, None, 14, 2, 3)            # an active row that is not there
        assert rc == E_ARG and b"row index" in lib.kzg_last_error(eng._h)
        assert eng.rows_stats() == live
    finally:
        release(S)
    assert eng.rows_stats() == before


def test_the_masked_quotient_bit_exact(engines, srs_of):
    """the 15-row instance of tests/blinding_ref.py at T = 2^5: the pieces against the reference's, then the shape check on
    an altered usable cell and on redrawn padding"""
    lg, u = 5, 26
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(55)
    inst = br.Instance(T, u, 501)
    t, rem = br.quotient(inst.coeff_rows(), inst.terms, inst.perm, inst.lookup, inst.active, 3)
    assert not any(rem)
    want = qr.pieces(t, T, 4)
    S = commit_sets(eng, inst.rows, (3, 9, 3))
    try:
        tset = zk_call(eng, S, inst.terms, inst.perm, inst.lookup, inst.active, 3, 4)
        try:
            check_pieces(eng, srs, tset, want, rnd)
        finally:
            tset.release()
        arg_error(lambda: x_call(eng, S, inst.terms, inst.perm, inst.lookup, 3, 4), SHAPE_MSG)   # unmasked: the padding binds
    finally:
        release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the whole hidden round
def test_the_whole_hidden_round_through_the_client():
    from zkp_subnet_amd.client import Client

    lg, u, seed = 6, 58, 2024
    T = 1 << lg
    cl = Client(seed=seed)
    cl.start(lg, 0)
    fr = lambda v: codec.be32_to_fr(be(v))   # noqa: E731
    unfr = lambda s: val(codec.fr_to_be32(s))   # noqa: E731
    poly = lambda row: [fr(v) for v in row]   # noqa: E731

    def ok(r):
        assert r.status_code == 200, r.json()
        return r.json()

    try:
        assert cl.engine.rows_stats() == (0, 0)
        inst = br.Instance(T, u, 909)
        fixed = ok(cl.worker_commit_rows(0, [poly(inst.fixed[j]) for j in br.FIXED]))["handle"]

        def prove(inst, n_pieces=4):
            """commit the wires, build m, z and S with their random tails, then the quotient: (handles, response)"""
            hw = ok(cl.worker_commit_rows(0, [poly(r) for r in inst.wires]))["handle"]
            tails = {k: [fr(v) for v in t] for k, t in inst.tails.items()}
            # the fixed set's rows, in its own numbering: qM qL qC s1 s2 s3 A Lu table
            sig = ok(cl.worker_commit_rows(0, [poly(inst.fixed[j]) for j in (br.S1, br.S2, br.S3)]))["handle"]
            tab = ok(cl.worker_commit_rows(0, [poly(inst.fixed[br.TAB])]))["handle"]
            cw = ok(cl.worker_commit_rows(0, [poly(inst.wires[2])]))["handle"]
            m = ok(cl.worker_commit_multiplicities_zk([cw], [tab], 1, 1, u, tails["m"]))
            z = ok(cl.worker_commit_grand_product_zk([hw], [sig], [fr(s) for s in inst.shifts], fr(inst.beta), fr(inst.gamma),
                                                     u, tails["z"]))
            s = ok(cl.worker_commit_lookup_sum_zk([cw], [tab], m["handle"], 1, 1, fr(inst.theta), fr(inst.lbeta), u, tails["S"]))
            made = [hw, sig, tab, cw, m["handle"], z["handle"], s["handle"]]
            hs = [hw, fixed, m["handle"], z["handle"], s["handle"]]       # rows 0 .. 14 in the order of blinding_ref
            terms = [[fr(c), fs] for c, fs in inst.terms]
            perm = dict(inst.perm, shifts=[fr(x) for x in inst.shifts], beta=fr(inst.beta), gamma=fr(inst.gamma),
                        alpha=fr(inst.alpha))
            lookup = dict(inst.lookup, theta=fr(inst.theta), beta=fr(inst.lbeta), alpha=fr(inst.alpha))
            q = cl.worker_commit_quotient_zk(hs, terms, perm, lookup, inst.active, 3, n_pieces)
            return made, hs, (m, z, s), q

        made, hs, (m, z, s), q = prove(inst)
        assert (m["missing"], unfr(z["closing"]), unfr(s["closing"])) == (0, 1, 0)
        hq = ok(q)["handle"]
        # the verifier's identity at zeta, from the evaluations at zeta and zeta w alone
        rnd = random.Random(4)
        zeta, w = rnd.randrange(R), gp.omega(T)
        ev = ok(cl.worker_eval_rows(hs, [fr(zeta), fr(zeta * w % R)], [list(range(15))] * 2))["evals"]
        at = {(j, rot): unfr(ev[rot][j]) for j in range(15) for rot in (0, 1)}
        num = br.num_at(lambda j, rot: at[(j, rot)], inst.terms, inst.perm, inst.lookup, inst.active, zeta, T)
        tp = [unfr(y) for y in ok(cl.worker_eval_rows([hq], [fr(zeta)], [[0, 1, 2, 3]]))["evals"][0]]
        t_zeta = sum(pow(zeta, p * T, R) * y for p, y in enumerate(tp)) % R
        assert num == t_zeta * (pow(zeta, T, R) - 1) % R
        for h in made + [hq]:
            ok(cl.worker_release_rows(h))
        # other padding, the same circuit: still a polynomial quotient
        made, _, parts, q = prove(br.Instance(T, u, 909).pad(31337))
        assert (parts[0]["missing"], unfr(parts[1]["closing"]), unfr(parts[2]["closing"])) == (0, 1, 0)
        for h in made + [ok(q)["handle"]]:
            ok(cl.worker_release_rows(h))
        # one altered usable cell: the shape check refuses
        made, _, _, q = prove(br.Instance(T, u, 909).broken())
        assert q.status_code == 400 and SHAPE_MSG in q.json()["error"]
        for h in made + [fixed]:
            ok(cl.worker_release_rows(h))
        assert cl.engine.rows_stats() == (0, 0)
    finally:
        cl.stop()


# ---------------------------------------------------------------------------------------------------- errors and structure
def test_errors_leave_the_context_serving(engines, srs_of):
    lg = 5
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    wires, sigmas = rand_rows(2, T, 8100), rand_rows(2, T, 8200)
    mult = rand_rows(1, T, 8300)[0]
    W, Sg, M = commit_sets(eng, wires, (2,)), commit_sets(eng, sigmas, (2,)), commit_sets(eng, [mult], (1,))
    big = commit_sets(engines(10), rand_rows(2, 1 << 10, 8400), (2,))
    lib = _native.load()
    hw, hs, hb = ((ctypes.c_uint64 * 1)(x[0].handle) for x in (W, Sg, big))
    c, cl, h, miss = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.c_uint64(0), ctypes.c_uint64(0)
    sh, one = be(1) + be(7), be(1)
    u = T - 6
    tail = b"".join(bt(tail_of(T, u, 81)))

    def gpz(e, a, b, usable, tl):
        return lib.kzg_rows_commit_grand_product_zk(e._h, 1, a, 1, b, 2, sh, one, one, usable, tl, c, cl, ctypes.byref(h))

    def lkz(usable, tl):
        return lib.kzg_rows_commit_lookup_sum_zk(eng._h, 1, hw, 1, hs, M[0].handle, 1, 2, one, one, usable, tl, c, cl,
                                                 ctypes.byref(h))

    def mlz(usable, tl):
        return lib.kzg_rows_commit_multiplicities_zk(eng._h, 1, hw, 1, hs, 1, 2, usable, tl, c, ctypes.byref(miss),
                                                     ctypes.byref(h))

    try:
        live = eng.rows_stats()
        z, closing = br.grand_product_zk(wires, sigmas, [1, 7], 1, 1, u, ints(tail))
        want = (oc.commit(srs, row_bytes(z), True), be(closing))

        def fresh_ok():
            assert gpz(eng, hw, hs, u, tail) == 0
            eng.release_rows(h.value)
            assert (c.raw, cl.raw) == want

        fresh_ok()
        bad_tail = tail[:64] + R.to_bytes(32, "big") + tail[96:]
        for call in (lambda us, tl: gpz(eng, hw, hs, us, tl), lkz, mlz):
            assert call(0, tail) == E_ARG and b"usable" in lib.kzg_last_error(eng._h)                  # u = 0
            assert call(T, tail) == E_ARG and b"usable" in lib.kzg_last_error(eng._h)                  # u = T
            assert call(2 ** 40, tail) == E_ARG
            assert call(u, bad_tail) == E_ARG and b"canonical" in lib.kzg_last_error(eng._h)           # a tail scalar >= r
            assert call(u, None) == E_ARG and b"null" in lib.kzg_last_error(eng._h)                    # NULL tail, u < T - 1
            assert call(T - 1, None) == 0                                                               # NULL tail, u = T - 1
            eng.release_rows(h.value)
            assert eng.rows_stats() == live
        assert gpz(engines(10), hb, hb, (1 << 10) - 33, tail) == E_ARG                                  # T - u > 32
        assert b"KZG_MAX_BLIND_ROWS" in lib.kzg_last_error(engines(10)._h)
        # the engine checks the tail's length before the library reads it
        bs = [be(1), be(7)]
        arg_error(lambda: eng.commit_grand_product_zk(W, Sg, bs, one, one, u, bt(ints(tail))[:-1]), "exactly")
        arg_error(lambda: eng.commit_grand_product_zk(W, Sg, bs, one, one, u, []), "exactly")
        arg_error(lambda: eng.commit_grand_product_zk([W[0].handle], [Sg[0].handle], bs, one, one, 0, []), "usable")
        fresh_ok()
        assert eng.rows_stats() == live
    finally:
        release(W + Sg + M + big)
    assert eng.rows_stats() == before


def test_four_threads_run_different_zk_calls(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    u = T - 6
    before = eng.rows_stats()
    wires, sigmas = rand_rows(2, T, 9100), rand_rows(2, T, 9200)
    inputs, table, mult = rand_rows(2, T, 9300), rand_rows(1, T, 9400), rand_rows(1, T, 9500)[0]
    rows, terms, perm, _ = standard(lg)
    W, Sg = commit_sets(eng, wires, (2,)), commit_sets(eng, sigmas, (2,))
    F, Tb, M = commit_sets(eng, inputs, (2,)), commit_sets(eng, table, (1,)), commit_sets(eng, [mult], (1,))
    Q = commit_sets(eng, rows + [[1] * T], (14,))
    tl = tail_of(T, u, 91)
    bs = [be(1), be(7)]
    z, zc = br.grand_product_zk(wires, sigmas, [1, 7], 11, 12, u, tl)
    S, sc = br.lookup_sum_zk(inputs, table, mult, 2, 1, 13, 14, u, tl)
    m, mm = br.multiplicities_zk(inputs, table, 2, 1, u, tl)
    ext = x_call(eng, Q, terms, perm, None, 2, 3)
    ext.release()
    com = lambda row: oc.commit(srs, row_bytes(row), True)   # noqa: E731
    jobs = [(lambda: eng.commit_grand_product_zk(W, Sg, bs, be(11), be(12), u, bt(tl)), ([com(z)], be(zc))),
            (lambda: eng.commit_lookup_sum_zk(F, Tb, M[0], 2, 1, be(13), be(14), u, bt(tl)), ([com(S)], be(sc))),
            (lambda: eng.commit_multiplicities_zk(F, Tb, 2, 1, u, bt(tl)), ([com(m)], mm)),
            (lambda: (zk_call(eng, Q, terms, perm, None, 13, 2, 3), None), (ext.commitments, None))]
    errors = []

    def work(j):
        try:
            for _ in range(3):
                rset, extra = jobs[j][0]()
                rset.release()
                assert (rset.commitments, extra) == jobs[j][1], j
        except Exception as ex:   # noqa: BLE001
            errors.append(repr(ex))

    ths = [threading.Thread(target=work, args=(j,)) for j in range(4)]
    for x in ths:
        x.start()
    for x in ths:
        x.join()
    release(W + Sg + F + Tb + M + Q)
    assert not errors, errors
    assert eng.rows_stats() == before


def test_multi_handle_returns_the_context_bytes(hip):
    lib = _native.load()
    scale, ms, G = 7, 1, 2
    T, M = 1 << (scale - ms), 1 << ms
    u = T - 6
    tx, ty = 0xB11DABCD, 0xB11D1357
    devs = (ctypes.c_int * G)(0, 0)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(G, devs, ctypes.byref(mh)) == 0
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        i = 1
        srs = oc.srs_gen(be(tx), be(ty), scale, ms, i)
        inst = br.Instance(T, u, 1212)
        tails = {k: b"".join(bt(v)) for k, v in inst.tails.items()}
        cc, c, cl = ctypes.create_string_buffer(48 * 16), ctypes.create_string_buffer(48 * 4), ctypes.create_string_buffer(32)
        hh = [ctypes.c_uint64(0) for _ in range(8)]
        commit = lambda rows, h: lib.kzg_multi_rows_commit(mh, i, len(rows), b"".join(row_bytes(r) for r in rows), T, 1, cc,  # noqa: E731
                                                           ctypes.byref(h))
        assert commit(inst.wires, hh[0]) == 0 and commit([inst.fixed[j] for j in br.FIXED], hh[1]) == 0
        assert commit([inst.fixed[j] for j in (br.S1, br.S2, br.S3)], hh[2]) == 0
        assert commit([inst.fixed[br.TAB]], hh[3]) == 0 and commit([inst.wires[2]], hh[4]) == 0
        arr = lambda *hs: (ctypes.c_uint64 * len(hs))(*[x.value for x in hs])   # noqa: E731
        miss = ctypes.c_uint64(9)
        assert lib.kzg_multi_rows_commit_multiplicities_zk(mh, i, 1, arr(hh[4]), 1, arr(hh[3]), 1, 1, u, tails["m"], c,
                                                           ctypes.byref(miss), ctypes.byref(hh[5])) == 0
        assert (miss.value, c.raw[:48]) == (0, oc.commit(srs, row_bytes(inst.m), True))
        assert lib.kzg_multi_rows_commit_grand_product_zk(mh, i, 1, arr(hh[0]), 1, arr(hh[2]), 3,
                                                          b"".join(be(s) for s in inst.shifts), be(inst.beta), be(inst.gamma), u,
                                                          tails["z"], c, cl, ctypes.byref(hh[6])) == 0
        assert (c.raw[:48], cl.raw) == (oc.commit(srs, row_bytes(inst.z), True), be(1))
        assert lib.kzg_multi_rows_commit_lookup_sum_zk(mh, i, 1, arr(hh[4]), 1, arr(hh[3]), hh[5].value, 1, 1, be(inst.theta),
                                                       be(inst.lbeta), u, tails["S"], c, cl, ctypes.byref(hh[7])) == 0
        assert (c.raw[:48], cl.raw) == (oc.commit(srs, row_bytes(inst.S), True), be(0))
        t, rem = br.quotient(inst.coeff_rows(), inst.terms, inst.perm, inst.lookup, inst.active, 3)
        assert not any(rem)
        gate, pm, lk, _keep = c_args(b_terms(inst.terms), b_perm(inst.perm), b_lookup(inst.lookup))
        act, hq = _native.QuotientActive(inst.active), ctypes.c_uint64(0)
        sets = arr(hh[0], hh[1], hh[5], hh[6], hh[7])
        assert lib.kzg_multi_rows_commit_quotient_zk(mh, i, 5, sets, gate, pm, lk, ctypes.byref(act), 3, 4, c,
                                                     ctypes.byref(hq)) == 0
        assert [c.raw[48 * p:48 * p + 48] for p in range(4)] == [oc.commit(srs, row_bytes(p), False) for p in qr.pieces(t, T, 4)]
        # under the other worker's index the sets are refused
        assert lib.kzg_multi_rows_commit_quotient_zk(mh, 0, 5, sets, gate, pm, lk, ctypes.byref(act), 3, 4, c,
                                                     ctypes.byref(hq)) == E_ARG
        for h in hh + [hq]:
            assert lib.kzg_multi_rows_release(mh, i, h.value) == 0
    finally:
        lib.kzg_multi_destroy(mh)


def test_no_row_sized_copy_inside_the_calls(engines):
    """structural: with stage profiling on, no _zk call opens an upload span (only upload_fr opens KZG_T_DECODE), while the
    transforms, the builders' kernels and the MSM's accumulate all ran; the results are those of the unprofiled calls"""
    lg = 10
    eng, T = engines(lg), 1 << lg
    u = T - 6
    before = eng.rows_stats()
    wires, sigmas = rand_rows(2, T, 9100), rand_rows(2, T, 9200)
    inputs, table, mult = rand_rows(2, T, 9300), rand_rows(1, T, 9400), rand_rows(1, T, 9500)[0]
    rows, terms, perm, _ = standard(lg)
    W, Sg = commit_sets(eng, wires, (2,)), commit_sets(eng, sigmas, (2,))
    F, Tb, M = commit_sets(eng, inputs, (2,)), commit_sets(eng, table, (1,)), commit_sets(eng, [mult], (1,))
    Q = commit_sets(eng, rows + [[1] * T], (14,))
    tl, bs = bt(tail_of(T, u, 93)), [be(1), be(7)]
    calls = {"grand product": lambda: eng.commit_grand_product_zk(W, Sg, bs, be(11), be(12), u, tl)[0],
             "lookup sum": lambda: eng.commit_lookup_sum_zk(F, Tb, M[0], 2, 1, be(13), be(14), u, tl)[0],
             "multiplicities": lambda: eng.commit_multiplicities_zk(F, Tb, 2, 1, u, tl)[0],
             "quotient": lambda: zk_call(eng, Q, terms, perm, None, 13, 2, 3)}
    lib = _native.load()
    try:
        for name, call in calls.items():
            plain = call()
            plain.release()
            assert lib.kzg_set_profiling(eng._h, 1) == 0
            try:
                rs = call()
                rs.release()
                tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
                assert lib.kzg_get_timings(eng._h, tms, len(tms)) == 0
            finally:
                assert lib.kzg_set_profiling(eng._h, 0) == 0
            t = dict(zip(_native.TIMING_NAMES, tms))
            print(name, "_zk stage times (ms):", {k: round(v, 4) for k, v in t.items()})
            assert t["decode"] == 0, name
            assert t["ntt"] > 0 and t["poly"] > 0 and t["accumulate"] > 0, name
            assert rs.commitments == plain.commitments, name
    finally:
        release(W + Sg + F + Tb + M + Q)
    assert eng.rows_stats() == before
