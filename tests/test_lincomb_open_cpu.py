"""CPU-only tests of evaluate-then-open on committed row sets (kzg_rows_eval, kzg_rows_open_lincomb, their kzg_multi_ forms,
kzg_vk_verify_open_lincomb; HipEngine.eval_rows / open_rows_lincomb, the text forms on Client and MultiDeviceClient): the
C-ABI's argument checks without a device, the verifier against openings built entirely with the C oracle (commit for every
C_j, open_ of the host-combined h_p = sum_j lambda_{p,j} f_j for every v_p and pi_p), and the host logic -- JSON shapes,
400 on ragged input, routing of handles to the device of their worker -- over a fake engine defined here."""
import ctypes
import hashlib
import itertools
import os
import random
import re

import pytest

from oracle import bls12_381 as o
from oracle import cpu as oc
from tests.gpu_common import be
from zkp_subnet_amd import MultiDeviceClient, _native, codec
from zkp_subnet_amd.build import build
from zkp_subnet_amd.client import Client
from zkp_subnet_amd.codec import be32_to_fr, g1_to_b64
from zkp_subnet_amd.engine import RowSet, lagrange_factor
from zkp_subnet_amd.verifier import Verifier

R = o.R
E_ARG = _native.KZG_E_ARG
_HANDLES = itertools.count(1)


@pytest.fixture(scope="module")
def lib():
    build()
    return _native.load()


def test_c_abi_null_context_or_handles(lib):
    ev, vals, pf = ctypes.create_string_buffer(32 * 64), ctypes.create_string_buffer(32 * 4), ctypes.create_string_buffer(48 * 4)
    pts, cfs = bytes(32 * 4), (1).to_bytes(32, "big") * 4
    masks = (ctypes.c_uint32 * 1)(1)
    hs = (ctypes.c_uint64 * 1)(1)
    ok = ctypes.c_int(7)
    assert lib.kzg_rows_eval(None, 1, hs, 1, pts, masks, ev) == E_ARG
    assert lib.kzg_rows_eval(None, 1, None, 1, pts, masks, ev) == E_ARG
    assert lib.kzg_rows_open_lincomb(None, 1, hs, 1, 1, pts, cfs, vals, pf) == E_ARG
    assert lib.kzg_rows_open_lincomb(None, 1, None, 1, 1, pts, cfs, vals, pf) == E_ARG
    assert lib.kzg_multi_rows_eval(None, 0, 1, hs, 1, pts, masks, ev) == E_ARG
    assert lib.kzg_multi_rows_eval(None, 0, 1, None, 1, pts, masks, ev) == E_ARG
    assert lib.kzg_multi_rows_open_lincomb(None, 0, 1, hs, 1, 1, pts, cfs, vals, pf) == E_ARG
    assert lib.kzg_multi_rows_open_lincomb(None, 0, 1, None, 1, 1, pts, cfs, vals, pf) == E_ARG
    assert lib.kzg_vk_verify_open_lincomb(None, 0, 1, bytes(48), 1, pts, cfs, pts, bytes(48), ctypes.byref(ok)) == E_ARG


def test_header_limits_match_python():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kzg_mi355x.h")).read()
    assert int(re.search(r"#define KZG_MAX_BATCH_OPEN (\d+)", hdr).group(1)) == _native.KZG_MAX_BATCH_OPEN
    assert int(re.search(r"#define KZG_MAX_OPEN_POINTS (\d+)", hdr).group(1)) == _native.KZG_MAX_OPEN_POINTS
    for name in ("kzg_rows_eval", "kzg_rows_open_lincomb", "kzg_vk_verify_open_lincomb", "kzg_multi_rows_eval",
                 "kzg_multi_rows_open_lincomb"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _native.SYMBOLS, name


# ---------------------------------------------------------------------------------------------------- the verifier
def combine(rows, lams):
    """h = sum_j lam_j f_j element by element (either form: the INTT is linear)."""
    T = len(rows[0]) // 32
    out = []
    for t in range(T):
        acc = 0
        for r, lam in zip(rows, lams):
            acc = (acc + lam * int.from_bytes(r[32 * t:32 * t + 32], "big")) % R
        out.append(be(acc))
    return b"".join(out)


def lincomb_open(srs, rows, points, lams, ef=True):
    comms = [oc.commit(srs, r, ef) for r in rows]
    vals, proofs = [], []
    for a, lam in zip(points, lams):
        v, pi = oc.open_(srs, combine(rows, lam), be(a), ef)
        vals.append(v)
        proofs.append(pi)
    return comms, vals, proofs


@pytest.fixture(scope="module")
def setup():
    build()
    oc.build()
    rnd = random.Random(91)
    tx, ty = rnd.randrange(1, R), rnd.randrange(1, R)
    scale, ms = 6, 2
    vk = Verifier.synthetic(tx, [lagrange_factor(i, ms, ty) for i in range(1 << ms)])
    srs = {i: oc.srs_gen(be(tx), be(ty), scale, ms, i) for i in range(1 << ms)}
    yield rnd, vk, srs, 1 << (scale - ms)
    vk.close()


def rows_for(rnd, k, T):
    return [b"".join(be(rnd.randrange(R)) for _ in range(T)) for _ in range(k)]


def coeffs_for(rnd, k, m):
    """random scalars with zeros, ones and r - 1 mixed in; every point keeps a nonzero one"""
    out = []
    for p in range(m):
        lam = [rnd.choice([0, 1, R - 1, rnd.randrange(R), rnd.randrange(R)]) for _ in range(k)]
        if not any(lam):
            lam[p % k] = rnd.randrange(1, R)
        out.append(lam)
    return out


def enc(lams):
    return [[be(x) for x in lam] for lam in lams]


@pytest.mark.parametrize("i,k,m,ef", [(0, 1, 1, True), (1, 3, 2, True), (3, 5, 4, False), (2, 16, 2, True)])
def test_oracle_lincomb_openings_verify(setup, i, k, m, ef):
    rnd, vk, srs, T = setup
    rows = rows_for(rnd, k, T)
    points, lams = [rnd.randrange(R) for _ in range(m)], coeffs_for(rnd, k, m)
    comms, vals, proofs = lincomb_open(srs[i], rows, points, lams, ef)
    assert vk.verify_open_lincomb(i, comms, [be(a) for a in points], enc(lams), vals, proofs)


def test_gamma_powers_agree_with_verify_open_multi(setup):
    rnd, vk, srs, T = setup
    i, k = 2, 4
    rows = rows_for(rnd, k, T)
    a, g = rnd.randrange(R), rnd.randrange(R)
    lam = [0, 1, g, 0]                                  # rows 1 and 2 with gamma powers: the multi-point opening's h
    comms, vals, proofs = lincomb_open(srs[i], rows, [a], [lam])
    ys = [oc.open_(srs[i], rows[j], be(a))[0] for j in (1, 2)]
    assert vals[0] == be(int.from_bytes(ys[0], "big") + g * int.from_bytes(ys[1], "big"))
    assert vk.verify_open_multi(i, comms, [be(a)], [[1, 2]], [be(g)], [ys], proofs)
    assert vk.verify_open_lincomb(i, comms, [be(a)], enc([lam]), vals, proofs)


def test_tampered_lincomb_openings_are_rejected(setup):
    rnd, vk, srs, T = setup
    i, k, m = 3, 4, 3
    rows = rows_for(rnd, k, T)
    points, lams = [rnd.randrange(R) for _ in range(m)], coeffs_for(rnd, k, m)
    comms, vals, proofs = lincomb_open(srs[i], rows, points, lams)
    P, L = [be(a) for a in points], enc(lams)
    assert vk.verify_open_lincomb(i, comms, P, L, vals, proofs)

    def rejected(c=comms, p=P, cf=L, v=vals, pf=proofs, idx=i):
        return not vk.verify_open_lincomb(idx, c, p, cf, v, pf)

    v2 = list(vals)
    v2[1] = be(int.from_bytes(v2[1], "big") + 1)
    assert rejected(v=v2)                                                   # one value
    L2 = [list(x) for x in L]
    L2[0][2] = be(lams[0][2] + 1)
    assert rejected(cf=L2)                                                  # one coefficient
    assert rejected(pf=[proofs[1], proofs[0], proofs[2]])                   # two proofs swapped
    assert rejected(p=[P[0], be(points[1] + 1), P[2]])                      # a wrong point
    c2 = list(comms)
    c2[3] = oc.commit(srs[i], rows[0])
    assert rejected(c=c2)                                                   # a wrong commitment
    assert rejected(idx=0)                                                  # another worker's basis
    # malformed bytes: valid = 0, not an error
    assert rejected(pf=[proofs[0], b"\x00" * 48, proofs[2]])
    assert rejected(c=[b"\xff" * 48] + comms[1:])
    assert rejected(pf=[proofs[0], proofs[1], proofs[2][:47]])
    # argument errors are errors
    for bad, code in ((lambda: vk.verify_open_lincomb(i, comms, [P[0], P[1], R.to_bytes(32, "big")], L, vals, proofs),
                       _native.KZG_E_SCALAR),
                      (lambda: vk.verify_open_lincomb(i, comms, P, [L[0], L[1][:3] + [R.to_bytes(32, "big")], L[2]], vals,
                                                      proofs), _native.KZG_E_SCALAR),
                      (lambda: vk.verify_open_lincomb(i, comms, P, L, [vals[0], vals[1], R.to_bytes(32, "big")], proofs),
                       _native.KZG_E_SCALAR),
                      (lambda: vk.verify_open_lincomb(9, comms, P, L, vals, proofs), E_ARG),
                      (lambda: vk.verify_open_lincomb(i, comms, P, [L[0], [be(0)] * k, L[2]], vals, proofs), E_ARG)):
        with pytest.raises(_native.KzgError) as ei:
            bad()
        assert ei.value.code == code, ei.value
    with pytest.raises(ValueError):
        vk.verify_open_lincomb(i, comms, P, [L[0], L[1][:3], L[2]], vals, proofs)


def test_c_abi_argument_limits(setup):
    rnd, vk, srs, T = setup
    lib = _native.load()
    ok = ctypes.c_int(7)
    z48, one = bytes(48 * 17), (1).to_bytes(32, "big")

    def call(k, m, i=0, cf=None):
        cf = cf if cf is not None else one * (max(k, 1) * max(m, 1))
        return lib.kzg_vk_verify_open_lincomb(vk._h, i, k, z48, m, bytes(32 * 5), cf, bytes(32 * 5), z48,
                                              ctypes.byref(ok))

    assert call(0, 1) == E_ARG                                           # k = 0
    assert call(17, 1) == E_ARG                                          # k > 16
    assert call(2, 0) == E_ARG                                           # m = 0
    assert call(2, 5) == E_ARG                                           # m > 4
    assert call(2, 1, i=4) == E_ARG                                      # worker outside the key
    assert call(2, 2, cf=one * 2 + bytes(64)) == E_ARG                   # point 1: every coefficient zero
    assert call(2, 1, cf=one + R.to_bytes(32, "big")) == _native.KZG_E_SCALAR
    assert ok.value == 0
    # the well-formed call on all-zero bytes: not a point, so valid = 0 and no error
    assert call(2, 1) == _native.KZG_OK and ok.value == 0


# ---------------------------------------------------------------------------------------------------- host logic
class FakeEngine:
    """The set semantics of the library over stand-in arithmetic: a 'value' / 'proof' is a hash of what it depends on, so
    the text forms hand the right rows, points and coefficients through exactly when they match these."""

    def __init__(self):
        self.sets = {}
        self.calls = []
        self.workers = None

    def gen_srs(self, tau_x, tau_y, scale, machines_scale, workers=None):
        self.workers = list(workers) if workers is not None else list(range(1 << machines_scale))

    def commit_rows(self, i, rows, evaluation_form=True):
        self.calls.append(("commit", i))
        h = next(_HANDLES)
        self.sets[h] = (i, list(rows))
        return RowSet(self, h, i, len(rows), len(rows[0]) // 32,
                      [hashlib.sha384(b"C" + bytes([i]) + r).digest() for r in rows])

    def _rows(self, sets):
        hs = [int(getattr(x, "handle", x)) for x in sets]
        if any(h not in self.sets for h in hs):
            raise _native.KzgError(E_ARG, "unknown or released handle")
        if len({self.sets[h][0] for h in hs}) != 1:
            raise _native.KzgError(E_ARG, "all sets must belong to one worker")
        return hs, self.sets[hs[0]][0], [r for h in hs for r in self.sets[h][1]]

    def eval_rows(self, sets, points, opened):
        hs, i, rows = self._rows(sets)
        self.calls.append(("eval", tuple(hs)))
        _native.open_masks(opened, len(rows))
        return [[hashlib.sha256(b"Y" + a + rows[j]).digest() for j in js] for a, js in zip(points, opened)]

    def open_rows_lincomb(self, sets, points, coeffs):
        hs, i, rows = self._rows(sets)
        self.calls.append(("lincomb", tuple(hs)))
        if any(len(c) != len(rows) for c in coeffs):
            raise _native.KzgError(E_ARG, "k must equal the rows of the concatenation")
        blob = [b"".join(c + r for c, r in zip(cs, rows)) for cs in coeffs]
        return ([hashlib.sha256(b"V" + a + b).digest() for a, b in zip(points, blob)],
                [hashlib.sha384(b"P" + bytes([i]) + a + b).digest() for a, b in zip(points, blob)])

    def verify_open_lincomb(self, i, commitments, points, coeffs, values, proofs):
        self.calls.append(("verify", i, len(commitments), len(points)))
        return all(v == hashlib.sha256(b"ok" + p).digest()[:32] for v, p in zip(values, points))

    def release_rows(self, handle):
        if self.sets.pop(int(handle), None) is None:
            raise _native.KzgError(E_ARG, "unknown or already released handle")


def fr(v):
    return be32_to_fr(v.to_bytes(32, "big"))


def polys(k, T, seed):
    return [[fr(seed * 1000 + j * 100 + t) for t in range(T)] for j in range(k)]


def client(engine, machines_scale=2):
    cl = Client(engine=engine)
    cl.machines_scale, cl._slice_of = machines_scale, None   # what start() leaves for a synthetic setup
    return cl


def test_client_json_shapes():
    eng = FakeEngine()
    cl = client(eng)
    a = cl.worker_commit_rows(1, polys(3, 8, 1)).json()["handle"]
    b = cl.worker_commit_rows(1, polys(1, 8, 2)).json()["handle"]
    X = [fr(11), fr(12)]
    r = cl.worker_eval_rows([a, b], X, [[0, 1, 2, 3], [3]])
    assert r.status_code == 200, r.json()
    assert set(r.json()) == {"evals"} and [len(e) for e in r.json()["evals"]] == [4, 1]
    assert all(isinstance(y, str) and len(y) == 43 for ev in r.json()["evals"] for y in ev)
    assert eng.calls[-1] == ("eval", (a, b))
    rows = [codec.fr_list_to_be32(p) for p in polys(3, 8, 1) + polys(1, 8, 2)]
    assert r.json()["evals"][1] == [be32_to_fr(hashlib.sha256(b"Y" + codec.fr_to_be32(X[1]) + rows[3]).digest())]
    L = [[fr(1), fr(0), fr(5), fr(7)], [fr(0), fr(0), fr(0), fr(1)]]
    o_ = cl.worker_open_rows_lincomb([a, b], X, L)
    assert o_.status_code == 200, o_.json()
    assert set(o_.json()) == {"values", "proofs"} and len(o_.json()["values"]) == 2 and len(o_.json()["proofs"]) == 2
    vals, pfs = eng.open_rows_lincomb([a, b], [codec.fr_to_be32(x) for x in X], [[codec.fr_to_be32(c) for c in cs] for cs in L])
    assert o_.json() == {"values": [be32_to_fr(v) for v in vals], "proofs": [g1_to_b64(p) for p in pfs]}
    C = cl.worker_commit_rows(1, polys(1, 8, 3)).json()["commitments"] * 4
    good = [be32_to_fr(hashlib.sha256(b"ok" + codec.fr_to_be32(x)).digest()) for x in X]
    v = cl.worker_verify_open_lincomb(1, o_.json()["proofs"], X, L, good, C)
    assert v.status_code == 200 and v.json() == {"valid": True}
    assert eng.calls[-1] == ("verify", 1, 4, 2)
    assert cl.worker_verify_open_lincomb(1, o_.json()["proofs"], X, L, o_.json()["values"], C).json() == {"valid": False}


def test_client_ragged_input_is_400():
    eng = FakeEngine()
    cl = client(eng)
    h = cl.worker_commit_rows(0, polys(2, 4, 3)).json()["handle"]
    X, L = [fr(5)], [[fr(1), fr(2)]]
    assert cl.worker_open_rows_lincomb([h], X, L).status_code == 200
    assert cl.worker_open_rows_lincomb([h], X, [[fr(1)]]).status_code == 400          # k != rows of the set
    assert cl.worker_open_rows_lincomb([h], X * 2, [L[0], [fr(1)]]).status_code == 400   # ragged coefficients
    assert cl.worker_open_rows_lincomb([h], X * 2, L).status_code == 400              # one list for two points
    assert cl.worker_open_rows_lincomb([h], X * 5, L * 5).status_code == 400          # m = 5
    assert cl.worker_open_rows_lincomb([h], [], []).status_code == 400                # m = 0
    assert cl.worker_open_rows_lincomb([h], X, [[]]).status_code == 400               # k = 0
    assert cl.worker_open_rows_lincomb([h], X, [[fr(1)] * 17]).status_code == 400     # k = 17
    assert cl.worker_open_rows_lincomb([], X, L).status_code == 400                   # no handle
    assert cl.worker_open_rows_lincomb(["x"], X, L).status_code == 400                # not a handle
    assert cl.worker_open_rows_lincomb([h], ["not base64!"], L).status_code == 400    # not a scalar
    assert cl.worker_eval_rows([h], X, [[0, 1]]).status_code == 200
    assert cl.worker_eval_rows([h], X, [[1, 0]]).status_code == 400                   # rows not increasing
    assert cl.worker_eval_rows([h], X, [[0, 2]]).status_code == 400                   # row 2 of a 2-row set
    assert cl.worker_eval_rows([h], X, [[0], [1]]).status_code == 400                 # ragged points / opened
    assert cl.worker_eval_rows([h], X * 5, [[0]] * 5).status_code == 400              # m = 5
    assert cl.worker_eval_rows([h] * 17, X, [[0]]).status_code == 400                 # more than 16 sets
    other = cl.worker_commit_rows(1, polys(1, 4, 8)).json()["handle"]
    assert cl.worker_eval_rows([h, other], X, [[0]]).status_code == 400               # two workers
    assert cl.worker_open_rows_lincomb([h, other], X, [[fr(1)] * 3]).status_code == 400
    P = [g1_to_b64(bytes(48))]
    C = [g1_to_b64(bytes(48))] * 2
    assert cl.worker_verify_open_lincomb(0, P, X, L, [fr(1)], C).status_code == 200
    assert cl.worker_verify_open_lincomb(0, P, X, [[fr(1)]], [fr(1)], C).status_code == 400   # k != commitments
    assert cl.worker_verify_open_lincomb(0, P * 2, X, L, [fr(1)], C).status_code == 400       # two proofs, one point
    assert cl.worker_verify_open_lincomb(0, P, X, L, [], C).status_code == 400                # no value
    assert cl.worker_verify_open_lincomb(0, [], [], [], [], C).status_code == 400             # m = 0
    assert Client(engine=None).worker_eval_rows([h], X, [[0]]).status_code == 503


def test_multi_device_client_routes_by_worker():
    engines = [FakeEngine(), FakeEngine(), FakeEngine()]
    multi = MultiDeviceClient(devices=[0, 1, 2], seed=5, engines=engines)
    assert multi.worker_verify_open_lincomb(0, [], [], [], [], []).status_code == 503   # not started yet
    assert multi.worker_eval_rows([1], [fr(1)], [[0]]).status_code == 400              # no set is known yet
    multi.start(scale=7, machines_scale=2)
    try:
        X = [fr(31), fr(32)]
        for i in range(4):
            a = multi.worker_commit_rows(i, polys(2, 8, 20 + i)).json()["handle"]
            b = multi.worker_commit_rows(i, polys(1, 8, 30 + i)).json()["handle"]
            g = i % 3
            r = multi.worker_eval_rows([a, b], X, [[0, 1, 2], [2]])
            assert r.status_code == 200, r.json()
            assert engines[g].calls[-1] == ("eval", (a, b))
            L = [[fr(1), fr(0), fr(9)], [fr(0), fr(0), fr(1)]]
            o_ = multi.worker_open_rows_lincomb([a, b], X, L)
            assert o_.status_code == 200, o_.json()
            assert engines[g].calls[-1] == ("lincomb", (a, b))
            local = engines[g].workers.index(i)                                     # the device's resident slice
            v = multi.worker_verify_open_lincomb(i, o_.json()["proofs"], X, L, o_.json()["values"],
                                                 [g1_to_b64(bytes(48))] * 3)
            assert v.status_code == 200 and engines[g].calls[-1] == ("verify", local, 3, 2)
            assert multi.worker_release_rows(b).status_code == 200
            assert multi.worker_eval_rows([a, b], X, [[0], [1]]).status_code == 400   # a released handle
            assert multi.worker_open_rows_lincomb([a], X[:1], [[fr(1), fr(2)]]).status_code == 200
        h0 = multi.worker_commit_rows(0, polys(1, 8, 50)).json()["handle"]
        h1 = multi.worker_commit_rows(1, polys(1, 8, 51)).json()["handle"]
        assert multi.worker_eval_rows([h0, h1], X[:1], [[0, 1]]).status_code == 400          # two workers
        assert multi.worker_open_rows_lincomb([h0, h1], X[:1], [[fr(1)] * 2]).status_code == 400
        assert multi.worker_eval_rows([10 ** 9], X[:1], [[0]]).status_code == 400            # unknown handle
        assert multi.worker_open_rows_lincomb([10 ** 9], X[:1], [[fr(1)]]).status_code == 400
        assert multi.worker_open_rows_lincomb([h0], X[:1], [[fr(1)], [fr(2)]]).status_code == 400   # ragged
    finally:
        multi.stop()
