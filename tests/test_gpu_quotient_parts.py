"""GPU tests (`-m gpu`) of the quotient in parts (kzg_rows_quotient_part / _finish) and the chained grand product
(kzg_rows_commit_grand_product_chain).  The expected pieces and rows come from the definitions in Python integers
(tests/quotient_parts_ref.py) and are committed with the C oracle, never with the library under test; where one call of the
library is the specification (one part = the call, three parts = the call) the bytes of the two are compared.  Everything is
bit-exact: canonical field elements and compressed points.
Degrees: with the active column A P1 has k + 2 = 5 factors of degree T - 1 for a chunk of k = 3 wires, so t has degree up to
4 T - 5 and takes 4 pieces.  At ext_log = 2 that is E pieces and no shape check; the tests that need the shape check to speak
(broken instances) run the same parts at ext_log = 3 with 4 < E pieces.  Each test leaves rows_stats() where it found it."""
import ctypes
import random
import threading

import pytest

from oracle import cpu as oc
from tests import blinding_ref as br
from tests import grand_product_ref as gp
from tests import quotient_parts_ref as qp
from tests import quotient_ref as qr
from tests.gpu_common import val
from tests.gpu_rows import (arg_error, b_lookup, b_perm, b_terms, bt, c_args, check_pieces, commit_sets, engine_cache, q_call,
                            release, srs_cache, standard, x_call, zk_call)
from tests.quotient_parts_ref import GPU_CLIENT, GPU_SPLIT, GPU_WIDE
from zkp_subnet_amd import _native, codec
from zkp_subnet_amd.engine import QuotientAcc, lagrange_factor

pytestmark = pytest.mark.gpu
R = qp.R
be, row_bytes = qp.be, qp.row_bytes
E_ARG, E_BUSY = _native.KZG_E_ARG, _native.KZG_E_BUSY
SEED_X, SEED_Y = 0xB11D01, 0xB11D02         # those of tests/test_gpu_blinding.py: the two modules' contexts hold the same SRS


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def part_call(eng, sets, terms, perm=None, lookup=None, active=None, link=None, ext_log=2, scale=None, acc=None):
    return eng.quotient_part(sets, b_terms(terms), b_perm(perm), b_lookup(lookup), active, link, ext_log,
                             None if scale is None else be(scale), acc)


def evals_at(eng, tset, x):
    k = tset.k
    return eng.eval_rows([tset], [be(x)], [list(range(k))])[0]


def one_by_one(eng, rows):
    """every row its own one-row set"""
    return commit_sets(eng, rows, (1,) * len(rows))


def split_sets(inst, S):
    """blinding_ref.Instance over one-row sets S (by row name) as three parts: (sets, terms, perm, lookup, active)"""
    gate_names = [br.A_, br.B_, br.C_, br.QM, br.QL, br.QC, br.ACT, br.LU, br.Z_, br.SUM]
    g = {n: j for j, n in enumerate(gate_names)}
    pn = [br.A_, br.B_, br.C_, br.S1, br.S2, br.S3, br.Z_, br.ACT]
    ln = [br.C_, br.TAB, br.M_, br.SUM, br.ACT]
    return [([S[n] for n in gate_names], [(c, [g[f] for f in fs]) for c, fs in inst.terms], None, None, None),
            ([S[n] for n in pn], [], dict(inst.perm, wires=[0, 1, 2], sigmas=[3, 4, 5], z=6), None, 7),
            ([S[n] for n in ln], [], None, dict(inst.lookup, inputs=[0], table=[1], mult=2, sum=3), 4)]


# ---------------------------------------------------------------------------------------------------- 1. one part = the call
@pytest.mark.parametrize("lg", [4, 10])
def test_one_part_and_finish_equal_the_single_call(engines, lg):
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(4100 + lg)
    zeta = rnd.randrange(R)
    rows, terms, perm, _ = standard(lg)
    a, b = ([rnd.randrange(R) for _ in range(T)] for _ in range(2))
    q = [-(a[(t + 1) % T] * b[t] + a[t - 1]) % R for t in range(T)]
    xterms = [(1, [(0, 1), 1]), (1, [(0, -1)]), (1, [2])]
    inst = br.Instance(T, T - 5 if lg == 4 else T - 6, 4200 + lg)
    shapes = [(commit_sets(eng, rows, (3, 5, 3, 2)), lambda S: q_call(eng, S, terms, perm, 2, 3), (terms, perm, None, None, 2, 3)),
              (commit_sets(eng, [a, b, q], (3,)), lambda S: x_call(eng, S, xterms, None, None, 2, 2), (xterms, None, None, None, 2, 2)),
              (commit_sets(eng, inst.rows, (15,)),
               lambda S: zk_call(eng, S, inst.terms, inst.perm, inst.lookup, inst.active, 3, 4),
               (inst.terms, inst.perm, inst.lookup, inst.active, 3, 4))]
    try:
        for S, single, (tt, pp, ll, act, ext_log, P) in shapes:
            one = single(S)
            want = (one.commitments, evals_at(eng, one, zeta))
            one.release()
            held = eng.rows_stats()
            acc = part_call(eng, S, tt, pp, ll, act, None, ext_log)
            assert isinstance(acc, QuotientAcc) and (acc.T, acc.ext_log) == (T, ext_log)
            live = eng.rows_stats()
            assert live[0] == held[0] + 1 and live[1] - held[1] >= (T << ext_log) * 32      # an entry of the set table
            tset = eng.quotient_finish(acc, P)
            try:
                assert (tset.commitments, evals_at(eng, tset, zeta)) == want and (tset.k, tset.T) == (P, T)
                assert eng.rows_stats()[0] == live[0]        # the accumulator is consumed, the piece set is live
                arg_error(lambda: eng.release_rows(acc.handle))
            finally:
                tset.release()
    finally:
        for S, _, _ in shapes:
            release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- 2. three parts = one call
@pytest.mark.parametrize("shape", GPU_SPLIT, ids=lambda s: f"T2^{s[0]}")
def test_three_parts_equal_the_single_zk_call(engines, shape):
    lg, u, seed = shape
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    inst = br.Instance(T, u, seed)
    whole = commit_sets(eng, inst.rows, (15,))
    S = one_by_one(eng, inst.rows)
    try:
        one = zk_call(eng, whole, inst.terms, inst.perm, inst.lookup, inst.active, 3, 4)
        one.release()
        acc = None
        for sets, tt, pp, ll, act in split_sets(inst, S):
            acc = part_call(eng, sets, tt, pp, ll, act, None, 3, 1, acc)
        tset = eng.quotient_finish(acc, 4)
        tset.release()
        assert tset.commitments == one.commitments
    finally:
        release(whole + S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- 3. scales
def test_two_scaled_parts_against_the_reference(engines, srs_of):
    lg = 4
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(4300)
    inst = br.Instance(T, 11, 43)
    S = one_by_one(eng, inst.rows)
    coeff = inst.coeff_rows()
    scales = [rnd.randrange(1, R), rnd.randrange(1, R)]
    try:
        split = split_sets(inst, S)[:2]
        acc, ref_parts = None, []
        for (sets, tt, pp, ll, act), sc in zip(split, scales):
            acc = part_call(eng, sets, tt, pp, ll, act, None, 3, sc, acc)
            names = [S.index(s) for s in sets]
            ref_parts.append(qp.part([coeff[n] for n in names], tt, pp, ll, act, None, sc))
        t, rem = qp.quotient(ref_parts, 3)
        assert not any(rem)
        tset = eng.quotient_finish(acc, 4)
        try:
            check_pieces(eng, srs, tset, qr.pieces(t, T, 4), rnd)
        finally:
            tset.release()
    finally:
        release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- 4 - 7. the wide circuit
def wide_sets(eng, w, chain=True):
    """the 18 caller rows as one-row sets by name, and z_0, z_1 built on the device by the chain call (start = 1, then z_0's
    closing value, or w.start1 for a broken instance) -> (sets by name, closing values)"""
    rows = w.all_rows
    S = one_by_one(eng, rows[:qp.Z0])
    bs = [be(s) for s in w.shifts]
    z0, c0 = eng.commit_grand_product_chain(S[qp.W0:qp.W3], S[qp.G0:qp.G3], bs[:3], be(w.beta), be(w.gamma), w.usable,
                                            bt(w.tails[0]), be(1))
    start1 = c0 if w.start1 is None else be(w.start1)
    z1, c1 = eng.commit_grand_product_chain(S[qp.W3:qp.G0], S[qp.G3:qp.QM], bs[3:], be(w.beta), be(w.gamma), w.usable,
                                            bt(w.tails[1]), start1)
    return S + [z0, z1], (c0, c1)


def wide_parts(eng, w, S, ext_log):
    acc = None
    for names, terms, perm, active, link, scale in w.layout():
        acc = part_call(eng, [S[n] for n in names], terms, perm, None, active, link, ext_log, scale, acc)
    return acc


def wide_identity(eng, w, S, tset, T, P, rnd):
    """num(zeta) = t(zeta) (zeta^T - 1) from the library's evaluations alone, at a random zeta and its rotations"""
    zeta, om = rnd.randrange(R), gp.omega(T)
    rots = [0, 1, w.link_rot]
    pts = [be(pow(om, r, R) * zeta % R) for r in rots]
    table = {}
    for lo in range(0, len(S), 16):
        part = S[lo:lo + 16]
        Y = eng.eval_rows(part, pts, [list(range(len(part)))] * len(pts))
        for p, r in enumerate(rots):
            for j in range(len(part)):
                table[(lo + j, r)] = val(Y[p][j])
    vals = [(qp.part(None, terms, perm, None, active, link, scale),
             (lambda names: lambda j, rot: table[(names[j], rot % T)])(names))
            for names, terms, perm, active, link, scale in w.layout()]
    tz = [val(y) for y in evals_at(eng, tset, zeta)]
    t_at = sum(pow(zeta, p * T, R) * tz[p] for p in range(P)) % R
    return qp.num_at(vals, zeta, T) == t_at * (pow(zeta, T, R) - 1) % R


def test_wide_circuit_chain_parts_and_identity(engines, srs_of):
    lg, u, seed = GPU_WIDE[0]
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(4400)
    w = qp.WideInstance(T, u, seed)
    S, (c0, c1) = wide_sets(eng, w)
    try:
        # the chain: start = 1 is the _zk call byte for byte; the second starts at the first's closing; the last closes at 1
        bs = [be(s) for s in w.shifts]
        zk, czk = eng.commit_grand_product_zk(S[qp.W0:qp.W3], S[qp.G0:qp.G3], bs[:3], be(w.beta), be(w.gamma), u, bt(w.tails[0]))
        zk.release()
        assert (zk.commitments, czk) == (S[qp.Z0].commitments, c0)
        assert (c0, c1) == (be(w.closing0), be(1)) and w.closing0 != 1
        assert S[qp.Z0].commitments[0] == oc.commit(srs, row_bytes(w.z0), True)
        assert S[qp.Z1].commitments[0] == oc.commit(srs, row_bytes(w.z1), True)
        # three parts and a finish against the reference: 20 distinct rows, no part above 11
        t, rem = qp.quotient(w.parts(), 2)
        assert not any(rem)
        acc = wide_parts(eng, w, S, 2)
        tset = eng.quotient_finish(acc, 4)
        try:
            check_pieces(eng, srs, tset, qr.pieces(t, T, 4), rnd)
            assert wide_identity(eng, w, S, tset, T, 4, rnd)
        finally:
            tset.release()
        # the same parts where the shape check speaks (4 < E = 8 pieces): the same pieces
        acc = wide_parts(eng, w, S, 3)
        t8 = eng.quotient_finish(acc, 4)
        t8.release()
        assert t8.commitments == tset.commitments
    finally:
        release(S)
    assert eng.rows_stats() == before


def test_the_wide_round_through_the_client():
    """the text forms over a real engine: chain, three parts, finish, and num(zeta) = t(zeta) (zeta^T - 1) recomputed from
    worker_eval_rows' answers alone"""
    from zkp_subnet_amd.client import Client

    lg, u, seed = GPU_CLIENT
    T = 1 << lg
    cl = Client(seed=seed)
    cl.start(lg, 0)
    fr = lambda v: codec.be32_to_fr(be(v))   # noqa: E731
    unfr = lambda s: val(codec.fr_to_be32(s))   # noqa: E731

    def ok(r):
        assert r.status_code == 200, r.json()
        return r.json()

    try:
        assert cl.engine.rows_stats() == (0, 0)
        w = qp.WideInstance(T, u, seed)
        H = [ok(cl.worker_commit_rows(0, [[fr(v) for v in row]]))["handle"] for row in w.all_rows[:qp.Z0]]
        sh, tails = [fr(s) for s in w.shifts], [[fr(v) for v in t] for t in w.tails]
        z0 = ok(cl.worker_commit_grand_product_chain(H[qp.W0:qp.W3], H[qp.G0:qp.G3], sh[:3], fr(w.beta), fr(w.gamma), u, tails[0],
                                                     fr(1)))
        z1 = ok(cl.worker_commit_grand_product_chain(H[qp.W3:qp.G0], H[qp.G3:qp.QM], sh[3:], fr(w.beta), fr(w.gamma), u, tails[1],
                                                     z0["closing"]))
        assert (unfr(z0["closing"]), unfr(z1["closing"])) == (w.closing0, 1)
        H += [z0["handle"], z1["handle"]]
        acc = None
        for names, terms, perm, active, link, scale in w.layout():
            pt = None if perm is None else dict(perm, shifts=[fr(x) for x in perm["shifts"]], beta=fr(perm["beta"]),
                                                gamma=fr(perm["gamma"]), alpha=fr(perm["alpha"]))
            acc = ok(cl.worker_quotient_part([H[n] for n in names], [[fr(c), fs] for c, fs in terms], pt, None, active,
                                             None if link is None else list(link), 2, fr(scale), acc))["acc"]
        assert cl.engine.rows_stats()[0] == len(H) + 1
        t = ok(cl.worker_quotient_finish(acc, 4))
        assert len(t["commitments"]) == 4 and cl.engine.rows_stats()[0] == len(H) + 1
        assert cl.worker_quotient_finish(acc, 4).status_code == 400          # consumed
        # the identity from the evaluations alone
        rnd = random.Random(4900)
        zeta, om = rnd.randrange(R), gp.omega(T)
        rots = [0, 1, w.link_rot]
        pts = [fr(pow(om, r, R) * zeta % R) for r in rots]
        table = {}
        for lo in range(0, len(H), 16):
            hs = H[lo:lo + 16]
            Y = ok(cl.worker_eval_rows(hs, pts, [list(range(len(hs)))] * len(pts)))["evals"]
            for p, r in enumerate(rots):
                for j in range(len(hs)):
                    table[(lo + j, r)] = unfr(Y[p][j])
        vals = [(qp.part(None, terms, perm, None, active, link, scale),
                 (lambda names: lambda j, rot: table[(names[j], rot % T)])(names))
                for names, terms, perm, active, link, scale in w.layout()]
        tz = [unfr(y) for y in ok(cl.worker_eval_rows([t["handle"]], [fr(zeta)], [[0, 1, 2, 3]]))["evals"][0]]
        t_at = sum(pow(zeta, p * T, R) * tz[p] for p in range(4)) % R
        assert qp.num_at(vals, zeta, T) == t_at * (pow(zeta, T, R) - 1) % R
        for h in H + [t["handle"]]:
            ok(cl.worker_release_rows(h))
        assert cl.engine.rows_stats() == (0, 0)
    finally:
        cl.stop()


def test_large_transforms_through_the_identity(engines):
    """T = 2^16, E = 4: N = 2^18, the size from which the transform's large path runs; no Python quotient at this size"""
    lg, u, seed = GPU_WIDE[1]
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(4500)
    w = qp.WideInstance(T, u, seed)
    S, (c0, c1) = wide_sets(eng, w)
    try:
        assert (c0, c1) == (be(w.closing0), be(1))
        acc = wide_parts(eng, w, S, 2)
        tset = eng.quotient_finish(acc, 4)
        try:
            assert wide_identity(eng, w, S, tset, T, 4, rnd)
        finally:
            tset.release()
    finally:
        release(S)
    assert eng.rows_stats() == before


@pytest.mark.parametrize("breaker", ["broken_cell", "broken_start", "broken_rot"])
def test_broken_wide_instances_fail_the_finish_and_keep_the_accumulator(engines, breaker):
    lg, u, seed = GPU_WIDE[0]
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    w = getattr(qp.WideInstance(T, u, seed), breaker)()
    S, _ = wide_sets(eng, w)
    try:
        acc = wide_parts(eng, w, S, 3)
        live = eng.rows_stats()
        assert live[0] == before[0] + len(S) + 1
        arg_error(lambda: eng.quotient_finish(acc, 4), "the constraints do not hold")
        assert eng.rows_stats() == live and not acc.released      # no set was created, the accumulator is still there
        acc.release()
        assert eng.rows_stats()[0] == live[0] - 1
    finally:
        release(S)
    assert eng.rows_stats() == before


def test_chain_with_a_random_start(engines, srs_of):
    lg = 10
    eng, srs, T = engines(lg), srs_of(lg), 1 << lg
    u = T - 6
    before = eng.rows_stats()
    rnd = random.Random(4700)
    w = qp.WideInstance(T, u, 47)
    S = one_by_one(eng, w.wires[:3] + w.sig[:3])
    bs = [be(s) for s in w.shifts[:3]]
    start = rnd.randrange(1, R)
    try:
        z, closing = br.grand_product_zk(w.wires[:3], w.sig[:3], w.shifts[:3], w.beta, w.gamma, u, w.tails[0])
        zc, cc = qp.grand_product_chain(w.wires[:3], w.sig[:3], w.shifts[:3], w.beta, w.gamma, u, w.tails[0], start)
        zset, cl = eng.commit_grand_product_chain(S[:3], S[3:], bs, be(w.beta), be(w.gamma), u, bt(w.tails[0]), be(start))
        try:
            assert cl == be(cc) == be(start * closing % R)
            assert zset.commitments[0] == oc.commit(srs, row_bytes(zc), True)
            om = gp.omega(T)
            ts = [0, u, u + 1, T - 1]
            Y = eng.eval_rows([zset], [be(pow(om, t, R)) for t in ts], [[0]] * 4)
            assert [val(y[0]) for y in Y] == [start, cc, z[u + 1], z[T - 1]]       # rows <= u scaled, the tail untouched
        finally:
            zset.release()
    finally:
        release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- 8. errors
def test_errors_leave_the_context_serving(hip, engines):
    eng = hip()
    eng.gen_srs(0xE44, 0xE45, 5, 1)             # two workers, T = 16
    T = 16
    other = engines(5)                           # T = 32
    rnd = random.Random(4800)
    rows = [[rnd.randrange(R) for _ in range(T)] for _ in range(3)]
    terms, bad_r = [(1, [0, 1]), (R - 1, [2])], R.to_bytes(32, "big")
    perm = {"wires": [0], "sigmas": [1], "z": 2, "shifts": [1], "beta": 3, "gamma": 5, "alpha": 7}
    before = eng.rows_stats()
    A = commit_sets(eng, rows, (3,))
    B = commit_sets(eng, rows, (3,), i=1)
    lib = _native.load()
    try:
        acc = part_call(eng, A, terms)
        live = eng.rows_stats()
        assert live[0] == before[0] + 3 and live[1] - before[1] >= 2 * 3 * T * 32 + 4 * T * 32     # counted, with its N * 32 bytes
        arg_error(lambda: part_call(eng, B, terms, acc=acc), "worker")                     # another worker
        arg_error(lambda: part_call(eng, A, terms, ext_log=3, acc=acc), "ext_log")         # another ext_log
        arg_error(lambda: part_call(eng, A, terms, link=(0, 1)))                           # a link without a permutation
        gate, pm, lk, _keep = c_args(b_terms(terms), None, None)
        hs = (ctypes.c_uint64 * 1)(A[0].handle)
        ln, h = _native.QuotientLink(0, 1), ctypes.c_uint64(acc.handle)
        assert lib.kzg_rows_quotient_part(eng._h, 1, hs, gate, None, ctypes.byref(ln), None, None, 2, None, ctypes.byref(h)) == E_ARG
        assert lib.kzg_rows_quotient_part(eng._h, 1, hs, gate, None, None, None, None, 2, bad_r, ctypes.byref(h)) == E_ARG
        arg_error(lambda: eng.quotient_part(A, b_terms(terms), None, None, None, None, 2, bad_r, acc), "scale")   # scale >= r
        # start of 0 or >= r
        for start in (bytes(32), bad_r):
            arg_error(lambda: eng.commit_grand_product_chain(A[:1], A[:1], [be(1)] * 3, be(3), be(5), T - 3, bt([1, 2]), start))
        # an accumulator is no row set, and a row set no accumulator
        arg_error(lambda: eng.eval_rows([acc], [be(5)], [[0]]), "accumulator")
        arg_error(lambda: eng.open_rows([acc], [be(5)], [[0]], [be(1)]), "accumulator")
        arg_error(lambda: eng.commit_grand_product_zk([acc], A[:1], [be(1)], be(3), be(5), T - 3, bt([1, 2])))
        arg_error(lambda: part_call(eng, [acc], terms), "accumulator")
        fake = QuotientAcc(eng, A[0].handle, 0, T, 2)
        arg_error(lambda: part_call(eng, A, terms, acc=fake), "row set")
        arg_error(lambda: eng.quotient_finish(fake, 2), "row set")
        fake.released = True
        # n_pieces outside [1, E]
        c, hh = ctypes.create_string_buffer(48 * 8), ctypes.c_uint64(0)
        for P in (0, 5):
            assert lib.kzg_rows_quotient_finish(eng._h, acc.handle, P, c, ctypes.byref(hh)) == E_ARG
        assert eng.rows_stats() == live
        # a part over rows of another length; through another context the handle is unknown
        H8 = commit_sets(eng, [[1] * 8], (1,))
        O = commit_sets(other, [[1] * 32], (1,))
        try:
            arg_error(lambda: part_call(eng, H8, [(1, [0])], acc=acc), "row length")
            arg_error(lambda: part_call(other, O, [(1, [0])], acc=QuotientAcc(other, acc.handle, 0, 32, 2)))
        finally:
            release(H8 + O)
        assert eng.rows_stats() == live
        # a released accumulator
        acc.release()
        arg_error(lambda: part_call(eng, A, terms, acc=QuotientAcc(eng, acc.handle, 0, T, 2)), "accumulator")
        assert lib.kzg_rows_quotient_finish(eng._h, acc.handle, 2, c, ctypes.byref(hh)) == E_ARG
        # the 65th live object
        fill = []
        while eng.rows_stats()[0] < _native.KZG_MAX_ROW_SETS:
            fill += commit_sets(eng, rows[:1], (1,))
        arg_error(lambda: part_call(eng, A, terms), code=E_BUSY)
        release(fill)
        # an accumulator made stale by an SRS reload
        acc = part_call(eng, A, terms, perm)
        eng.gen_srs(0xE46, 0xE47, 5, 1)
        arg_error(lambda: eng.quotient_finish(acc, 4), "stale")
        acc.release()
        # ... and the context keeps serving
        A2 = commit_sets(eng, rows, (3,))
        acc = part_call(eng, A2, [(1, [0]), (R - 1, [0])])
        tset = eng.quotient_finish(acc, 1)
        tset.release()
        release(A2)
    finally:
        release(A + B)
    assert eng.rows_stats()[0] == before[0]


# ---------------------------------------------------------------------------------------------------- 9. threads
def test_four_threads_add_to_one_accumulator(engines):
    lg, u, seed = GPU_SPLIT[2]
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    inst = br.Instance(T, u, seed)
    S = one_by_one(eng, inst.rows)
    split = split_sets(inst, S)
    jobs = [(split[0], 3), (split[1], 5), (split[2], 7), (split[0], 11)]
    try:
        def run(order, threaded):
            sets, tt, pp, ll, act = split[1]
            acc = part_call(eng, sets, tt, pp, ll, act, None, 3, 2)      # the accumulator exists before the threads start
            errors = []

            def work(j):
                try:
                    (sets, tt, pp, ll, act), sc = jobs[j]
                    part_call(eng, sets, tt, pp, ll, act, None, 3, sc, acc)
                except Exception as ex:   # noqa: BLE001
                    errors.append(repr(ex))

            if threaded:
                ths = [threading.Thread(target=work, args=(j,)) for j in order]
                for x in ths:
                    x.start()
                for x in ths:
                    x.join()
            else:
                for j in order:
                    work(j)
            assert not errors, errors
            tset = eng.quotient_finish(acc, 8)       # (a sum that is no satisfied circuit's quotient: every piece is kept)
            tset.release()
            return tset.commitments

        assert run(range(4), True) == run(range(4), False) == run(reversed(range(4)), False)
    finally:
        release(S)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- 10. the multi handle
def test_multi_handle_returns_the_context_bytes(hip):
    lib = _native.load()
    scale, ms, G = 5, 1, 2
    T, M = 1 << (scale - ms), 1 << ms
    u = T - 5
    tx, ty = 0xB22DABCD, 0xB22D1357
    eng = hip()
    eng.gen_srs(tx, ty, scale, ms)
    w = qp.WideInstance(T, u, 51)
    devs = (ctypes.c_int * G)(0, 0)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(G, devs, ctypes.byref(mh)) == 0
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        i = 1
        # the context's bytes
        S = commit_sets(eng, w.all_rows[:qp.Z0], (1,) * qp.Z0, i=i)
        bs = [be(s) for s in w.shifts]
        z0, c0 = eng.commit_grand_product_chain(S[qp.W3:qp.G0], S[qp.G3:qp.QM], bs[3:], be(w.beta), be(w.gamma), u, bt(w.tails[1]),
                                                be(w.closing0))
        names, terms, perm, active, link, scale_p = w.layout()[1]
        acc = part_call(eng, [S[n] if n < qp.Z0 else z0 for n in names], terms, perm, None, active, None, 2, scale_p)
        tset = eng.quotient_finish(acc, 4)
        want = (z0.commitments[0], c0, tset.commitments)
        release(S + [z0, tset])
        # the multi handle's
        cc, c, cl = ctypes.create_string_buffer(48), ctypes.create_string_buffer(48 * 4), ctypes.create_string_buffer(32)
        hh = [ctypes.c_uint64(0) for _ in range(qp.Z0)]
        for n in range(qp.Z0):
            assert lib.kzg_multi_rows_commit(mh, i, 1, row_bytes(w.all_rows[n]), T, 1, cc, ctypes.byref(hh[n])) == 0
        arr = lambda hs: (ctypes.c_uint64 * len(hs))(*[x.value for x in hs])   # noqa: E731
        hz = ctypes.c_uint64(0)
        tail = b"".join(bt(w.tails[1]))
        assert lib.kzg_multi_rows_commit_grand_product_chain(mh, i, 3, arr(hh[qp.W3:qp.G0]), 3, arr(hh[qp.G3:qp.QM]), 3,
                                                             b"".join(bs[3:]), be(w.beta), be(w.gamma), u, tail, be(w.closing0),
                                                             cc, cl, ctypes.byref(hz)) == 0
        assert (cc.raw, cl.raw) == want[:2]
        gate, pm, lk, _keep = c_args(b_terms(terms), b_perm(perm), None)
        act, ha, ht = _native.QuotientActive(active), ctypes.c_uint64(0), ctypes.c_uint64(0)
        sets = arr([hh[n] if n < qp.Z0 else hz for n in names])
        sc = be(scale_p)
        assert lib.kzg_multi_rows_quotient_part(mh, i, len(names), sets, gate, pm, None, None, ctypes.byref(act), 2, sc,
                                                ctypes.byref(ha)) == 0
        # under the other worker's index the sets and the accumulator are refused
        hb = ctypes.c_uint64(ha.value)
        assert lib.kzg_multi_rows_quotient_part(mh, 0, len(names), sets, gate, pm, None, None, ctypes.byref(act), 2, sc,
                                                ctypes.byref(hb)) == E_ARG
        assert lib.kzg_multi_rows_quotient_finish(mh, 0, ha.value, 4, c, ctypes.byref(ht)) == E_ARG
        assert lib.kzg_multi_rows_quotient_finish(mh, i, ha.value, 4, c, ctypes.byref(ht)) == 0
        assert [c.raw[48 * p:48 * p + 48] for p in range(4)] == want[2]
        assert lib.kzg_multi_rows_release(mh, i, ha.value) == E_ARG          # consumed
        for h in hh + [hz, ht]:
            assert lib.kzg_multi_rows_release(mh, i, h.value) == 0
    finally:
        lib.kzg_multi_destroy(mh)
