"""CPU-only tests of the SHPLONK opening (kzg_rows_commit_shplonk, its kzg_multi_ form, kzg_vk_verify_open_shplonk;
HipEngine.commit_shplonk / open_shplonk_finish / verify_open_shplonk, shplonk_finish_coeffs, the text forms on Client and
MultiDeviceClient): the C-ABI's argument checks without a device, the round-B scalars against the reference, the verifier
against proofs built entirely with the C oracle (tests/shplonk_ref.py), the algebraic identity behind round B on integers
alone, and the host logic over a fake engine defined here.  Without a device the ctx and multi forms can only be reached
with a null handle (creating either needs a GPU): their limit checks are in tests/test_gpu_shplonk.py
(test_errors_leave_the_context_serving, test_multi_handle_returns_the_context_bytes); the vk form's are here."""
import ctypes
import hashlib
import itertools
import os
import random
import re

import pytest

from oracle import cpu as oc
from tests import shplonk_ref as ref
from zkp_subnet_amd import MultiDeviceClient, _native
from zkp_subnet_amd.build import build
from zkp_subnet_amd.client import Client
from zkp_subnet_amd.codec import be32_to_fr, fr_to_be32, g1_to_b64
from zkp_subnet_amd.engine import RowSet, lagrange_factor
from zkp_subnet_amd.verifier import Verifier, shplonk_finish_coeffs

R = ref.R
be = ref.be
E_ARG = _native.KZG_E_ARG
_HANDLES = itertools.count(1)


@pytest.fixture(scope="module")
def lib():
    build()
    return _native.load()


def test_c_abi_null_pointers(lib):
    c48, h = ctypes.create_string_buffer(48), ctypes.c_uint64(0)
    pts, cfs = bytes(32), (1).to_bytes(32, "big")
    masks, hs = (ctypes.c_uint32 * 1)(1), (ctypes.c_uint64 * 1)(1)
    ok = ctypes.c_int(7)
    assert lib.kzg_rows_commit_shplonk(None, 1, hs, 1, 1, pts, masks, cfs, c48, ctypes.byref(h)) == E_ARG
    assert lib.kzg_rows_commit_shplonk(None, 1, None, 1, 1, pts, masks, cfs, c48, ctypes.byref(h)) == E_ARG
    assert lib.kzg_multi_rows_commit_shplonk(None, 0, 1, hs, 1, 1, pts, masks, cfs, c48, ctypes.byref(h)) == E_ARG
    assert lib.kzg_multi_rows_commit_shplonk(None, 0, 1, None, 1, 1, pts, masks, cfs, c48, ctypes.byref(h)) == E_ARG
    assert lib.kzg_vk_verify_open_shplonk(None, 0, 1, bytes(48), 1, pts, masks, cfs, pts, bytes(48), cfs, bytes(48),
                                          ctypes.byref(ok)) == E_ARG


def test_header_limits_match_python():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kzg_mi355x.h")).read()
    assert int(re.search(r"#define KZG_MAX_SHPLONK_POINTS (\d+)", hdr).group(1)) == _native.KZG_MAX_SHPLONK_POINTS == 8
    assert re.search(r"#define KZG_MAX_SHPLONK_ROWS\s+\(KZG_MAX_BATCH_OPEN - 1\)", hdr)
    assert _native.KZG_MAX_SHPLONK_ROWS == _native.KZG_MAX_BATCH_OPEN - 1
    for name in ("kzg_rows_commit_shplonk", "kzg_multi_rows_commit_shplonk", "kzg_vk_verify_open_shplonk"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _native.SYMBOLS, name


# ------------------------------------------------------------------------------------------------- the round-B scalars
def case(rnd, T, name, zero_coeff=True):
    """(F, points, opened, c, u) of a shape: points zeta w^p on the first shapes' lines, random coefficient rows"""
    k, opened = ref.SHAPES[name]
    F = [[rnd.randrange(R) for _ in range(T)] for _ in range(k)]
    zeta = rnd.randrange(1, R)
    points = [zeta * pow(7, p, R) % R for p in range(len(opened))]
    c = [rnd.randrange(1, R) for _ in range(k)]
    u = rnd.randrange(R)
    while u in points:
        u = rnd.randrange(R)
    return F, points, opened, c, u


@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_finish_coeffs_match_the_reference(name):
    rnd = random.Random(500 + list(ref.SHAPES).index(name))
    F, points, opened, c, u = case(rnd, 16, name)
    c[0] = 0
    lam = shplonk_finish_coeffs([be(a) for a in points], opened, [be(x) for x in c], be(u))
    assert lam == [be(x) for x in ref.finish_coeffs(points, opened, c, u)]
    assert len(lam) == len(c) + 1 and lam[0] == be(0)
    with pytest.raises(ValueError):
        shplonk_finish_coeffs([be(a) for a in points], opened, [be(x) for x in c], be(points[-1]))     # u among the points
    with pytest.raises(ValueError):
        shplonk_finish_coeffs([be(a) for a in points], opened, [be(x) for x in c], R.to_bytes(32, "big"))
    with pytest.raises(ValueError):
        shplonk_finish_coeffs([be(a) for a in points], opened[:-1] + [], [be(x) for x in c], be(u)) if len(opened) > 1 \
            else shplonk_finish_coeffs([be(a) for a in points], [], [be(x) for x in c], be(u))


@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_round_b_identity_on_integers(name):
    """Z_P(u) h(u) = sum_j c_j Z_{P \\ S_j}(u) (f_j(u) - r_j(u)), hence L(u) = v: guards the reference itself"""
    rnd = random.Random(77)
    F, points, opened, c, u = case(rnd, 16, name)
    c[-1] = 0
    h = ref.h_poly(F, points, opened, c)
    assert h[-1] == 0                                       # degree <= T - 2
    lam = ref.finish_coeffs(points, opened, c, u)
    evals = ref.evaluations(F, points, opened)
    v = ref.value_v(points, opened, c, evals, u)
    assert ref.poly_eval(ref.combine(F + [h], lam), u) == v
    # h is a polynomial identity, not only one at u: (f_j - r_j) is divisible by Z_{S_j}, so at any x outside P
    x = rnd.randrange(R)
    S = ref.point_sets(len(F), opened)
    want = 0
    for j, f in enumerate(F):
        xs = [points[p] for p in S[j]]
        ys = [evals[p][opened[p].index(j)] for p in S[j]]
        z = 1
        for a in xs:
            z = z * (x - a) % R
        want = (want + c[j] * (ref.poly_eval(f, x) - ref.interpolant_at(xs, ys, x)) * pow(z, -1, R)) % R
    assert ref.poly_eval(h, x) == want


# ---------------------------------------------------------------------------------------------------- the verifier
@pytest.fixture(scope="module")
def setup():
    build()
    oc.build()
    rnd = random.Random(92)                                 # the key material only: each test seeds its own data
    tx, ty = rnd.randrange(1, R), rnd.randrange(1, R)
    keys = {}
    for scale, ms in ((6, 2), (8, 2)):                      # T = 16 and 64
        vk = Verifier.synthetic(tx, [lagrange_factor(i, ms, ty) for i in range(1 << ms)])
        srs = {i: oc.srs_gen(be(tx), be(ty), scale, ms, i) for i in (1, 3)}
        keys[1 << (scale - ms)] = (vk, srs)
    yield keys
    for vk, _ in keys.values():
        vk.close()


def verify(vk, i, comms, points, opened, c, evals, W, u, pi):
    return vk.verify_open_shplonk(i, comms, [be(a) for a in points], opened, [be(x) for x in c],
                                  [[be(y) for y in ev] for ev in evals], W, be(u), pi)


@pytest.mark.parametrize("T", [16, 64])
@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_verifier_accepts_reference_proofs(setup, T, name):
    rnd, keys = random.Random(1000 + T + list(ref.SHAPES).index(name)), setup
    vk, srs = keys[T]
    i = 1 if name in ("one", "three") else 3
    F, points, opened, c, u = case(rnd, T, name)
    if name == "plonk":
        c[1] = 0                                            # a row left out
    comms, evals, W, v, pi, h = ref.prove(srs[i], F, points, opened, c, u)
    assert v == be(ref.value_v(points, opened, c, evals, u))
    assert verify(vk, i, comms, points, opened, c, evals, W, u, pi)
    assert not verify(vk, 4 - i, comms, points, opened, c, evals, W, u, pi)          # another worker's basis


def test_verifier_rejects_any_one_change(setup):
    rnd, keys = random.Random(2001), setup
    vk, srs = keys[16]
    i = 3
    F, points, opened, c, u = case(rnd, 16, "three")
    comms, evals, W, v, pi, h = ref.prove(srs[i], F, points, opened, c, u)
    assert verify(vk, i, comms, points, opened, c, evals, W, u, pi)
    other = oc.commit(srs[i], ref.row_bytes(F[0][::-1]), False)
    assert not verify(vk, i, comms, points, opened, c, evals, other, u, pi)          # W
    assert not verify(vk, i, comms, points, opened, c, evals, W, u, other)          # pi
    e2 = [list(ev) for ev in evals]
    e2[1][0] = (e2[1][0] + 1) % R
    assert not verify(vk, i, comms, points, opened, c, e2, W, u, pi)                # one evaluation
    assert not verify(vk, i, comms, points, opened, c, evals, W, (u + 1) % R, pi)   # u
    c2 = list(c)
    c2[4] = (c2[4] + 1) % R
    assert not verify(vk, i, comms, points, opened, c2, evals, W, u, pi)            # one coefficient
    # one mask bit: row 5 no longer opened at point 3 (its evaluation leaves the list with it)
    o2 = [list(js) for js in opened]
    o2[3] = [4]
    e3 = [list(ev) for ev in evals]
    e3[3] = e3[3][:1]
    assert not verify(vk, i, comms, points, o2, c, e3, W, u, pi)
    cm = list(comms)
    cm[2] = comms[0]
    assert not verify(vk, i, cm, points, opened, c, evals, W, u, pi)                # one commitment
    # malformed group elements: ok = 0, not an error
    assert not verify(vk, i, comms, points, opened, c, evals, b"\xff" * 48, u, pi)
    assert not verify(vk, i, comms, points, opened, c, evals, W, u, bytes(48))
    assert not verify(vk, i, comms, points, opened, c, evals, W[:47], u, pi)


def test_verifier_argument_errors(setup):
    rnd, keys = random.Random(2002), setup
    vk, srs = keys[16]
    i = 1
    F, points, opened, c, u = case(rnd, 16, "plonk")
    comms, evals, W, v, pi, h = ref.prove(srs[i], F, points, opened, c, u)

    def code(fn):
        with pytest.raises(_native.KzgError) as ei:
            fn()
        return ei.value.code

    assert code(lambda: verify(vk, i, comms, [points[0], points[0]], opened, c, evals, W, u, pi)) == E_ARG   # equal points
    assert code(lambda: verify(vk, i, comms, points, opened, c, evals, W, points[1], pi)) == E_ARG           # u in P
    o2, e2 = [[0, 1, 2, 3], [3]], [evals[0][:4], evals[1]]
    assert code(lambda: verify(vk, i, comms, points, o2, c, e2, W, u, pi)) == E_ARG      # c_4 != 0, S_4 empty
    c0 = list(c)
    c0[4] = 0
    assert verify(vk, i, comms, points, o2, c0, e2, W, u, pi) is False                   # ... and fine once c_4 = 0
    assert code(lambda: verify(vk, i, comms, points, opened, [0] * 5, evals, W, u, pi)) == E_ARG   # all c_j zero
    assert code(lambda: verify(vk, 9, comms, points, opened, c, evals, W, u, pi)) == E_ARG
    lib = _native.load()
    ok = ctypes.c_int(7)
    one, z48 = (1).to_bytes(32, "big"), bytes(48 * 16)
    pts9 = b"".join(be(p + 1) for p in range(9))
    EVALS = bytes(32 * 16 * 9)   # more than any mask set below can name (k <= 16 bits, m <= 9 masks)

    def call(k, m, masks, pts=pts9, cf=None, u32=be(1000), idx=0):
        ms = (ctypes.c_uint32 * 9)(*masks)
        return lib.kzg_vk_verify_open_shplonk(vk._h, idx, k, z48, m, pts, ms, cf or one * 16, EVALS, z48, u32, z48,
                                              ctypes.byref(ok))

    assert call(0, 1, [1]) == E_ARG and call(16, 1, [0xffff]) == E_ARG               # k = 0, k > 15
    assert call(1, 0, [1]) == E_ARG and call(1, 9, [1] * 9) == E_ARG                 # m = 0, m > 8
    assert call(2, 1, [7]) == E_ARG                                                  # a mask bit >= k
    assert call(1, 1, [1], pts=R.to_bytes(32, "big")) == E_ARG                       # a point >= r
    assert call(1, 1, [1], cf=R.to_bytes(32, "big")) == E_ARG                        # a coefficient >= r
    assert call(1, 1, [1], u32=R.to_bytes(32, "big")) == _native.KZG_E_SCALAR
    assert call(1, 1, [1], idx=4) == E_ARG
    assert ok.value == 0
    assert call(15, 8, [0x7fff] * 8) == _native.KZG_OK and ok.value == 0              # well-formed, not points: ok = 0


# ---------------------------------------------------------------------------------------------------- host logic
class FakeEngine:
    """The set semantics of the library over stand-in arithmetic: W, v and pi are hashes of what they depend on."""

    def __init__(self):
        self.sets = {}
        self.calls = []
        self.workers = None

    def gen_srs(self, tau_x, tau_y, scale, machines_scale, workers=None):
        self.workers = list(workers) if workers is not None else list(range(1 << machines_scale))

    def commit_rows(self, i, rows, evaluation_form=True):
        h = next(_HANDLES)
        self.sets[h] = (i, list(rows))
        return RowSet(self, h, i, len(rows), len(rows[0]) // 32, [hashlib.sha384(b"C" + bytes([i]) + r).digest() for r in rows])

    def _rows(self, sets):
        hs = [int(getattr(x, "handle", x)) for x in sets]
        if any(h not in self.sets for h in hs):
            raise _native.KzgError(E_ARG, "unknown or released handle")
        if len({self.sets[h][0] for h in hs}) != 1:
            raise _native.KzgError(E_ARG, "all sets must belong to one worker")
        return hs, self.sets[hs[0]][0], [r for h in hs for r in self.sets[h][1]]

    def commit_shplonk(self, sets, points, opened, coeffs):
        hs, i, rows = self._rows(sets)
        self.calls.append(("shplonk", tuple(hs)))
        if len(coeffs) != len(rows):
            raise _native.KzgError(E_ARG, "k must equal the rows of the concatenation")
        _native.shplonk_masks(opened, len(rows))
        blob = b"".join(points) + repr(opened).encode() + b"".join(c + r for c, r in zip(coeffs, rows))
        h = next(_HANDLES)
        self.sets[h] = (i, [hashlib.sha256(blob).digest() * (len(rows[0]) // 32)])
        w = hashlib.sha384(b"W" + blob).digest()
        return w, RowSet(self, h, i, 1, len(rows[0]) // 32, [w])

    def open_shplonk_finish(self, sets, h_set, points, opened, coeffs, u):
        hs, i, rows = self._rows(list(sets) + [h_set])
        self.calls.append(("finish", tuple(hs)))
        lam = shplonk_finish_coeffs(points, opened, coeffs, u)
        blob = u + b"".join(l + r for l, r in zip(lam, rows))
        return hashlib.sha256(b"V" + blob).digest(), hashlib.sha384(b"P" + blob).digest()

    def verify_open_shplonk(self, i, commitments, points, opened, coeffs, evals, w, u, proof):
        self.calls.append(("verify", i, len(commitments), len(points)))
        return proof == hashlib.sha384(b"good" + w + u).digest()

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
    X, opened, C, u = [fr(11), fr(12), fr(13)], [[0, 1, 2, 3], [3], []], [fr(5), fr(0), fr(6), fr(7)], fr(99)
    r = cl.worker_commit_shplonk([a, b], X, opened, C)
    assert r.status_code == 200, r.json()
    assert set(r.json()) == {"handle", "w"} and isinstance(r.json()["w"], str)
    assert eng.calls[-1] == ("shplonk", (a, b))
    w, hset = eng.commit_shplonk([a, b], [fr_to_be32(x) for x in X], opened, [fr_to_be32(c) for c in C])
    assert r.json()["w"] == g1_to_b64(w)
    h = r.json()["handle"]
    f = cl.worker_open_shplonk_finish([a, b], h, X, opened, C, u)
    assert f.status_code == 200, f.json()
    assert set(f.json()) == {"value", "proof"}
    assert eng.calls[-1] == ("finish", (a, b, h))
    # the fake's W depends on every input, so the second round-A call made the same set contents: same v and pi
    v, pi = eng.open_shplonk_finish([a, b], hset, [fr_to_be32(x) for x in X], opened, [fr_to_be32(c) for c in C], fr_to_be32(u))
    assert f.json() == {"value": be32_to_fr(v), "proof": g1_to_b64(pi)}
    comms = [g1_to_b64(bytes(48))] * 4
    evals = [[fr(1)] * 4, [fr(2)], []]
    good = g1_to_b64(hashlib.sha384(b"good" + w + fr_to_be32(u)).digest())
    ok = cl.worker_verify_open_shplonk(1, r.json()["w"], good, u, X, opened, C, evals, comms)
    assert ok.status_code == 200 and ok.json() == {"valid": True}
    assert eng.calls[-1] == ("verify", 1, 4, 3)
    assert cl.worker_verify_open_shplonk(1, r.json()["w"], f.json()["proof"], u, X, opened, C, evals, comms).json() == \
        {"valid": False}


def test_client_ragged_input_is_400():
    eng = FakeEngine()
    cl = client(eng)
    h = cl.worker_commit_rows(0, polys(2, 4, 3)).json()["handle"]
    X, O, C = [fr(5), fr(6)], [[0, 1], [1]], [fr(1), fr(2)]
    r = cl.worker_commit_shplonk([h], X, O, C)
    assert r.status_code == 200
    hh = r.json()["handle"]
    assert cl.worker_commit_shplonk([h], X, O[:1], C).status_code == 400            # one row list for two points
    assert cl.worker_commit_shplonk([h], X, O, C[:1]).status_code == 400            # k != rows of the set
    assert cl.worker_commit_shplonk([h], X, [[1, 0], [1]], C).status_code == 400    # rows not increasing
    assert cl.worker_commit_shplonk([h], X, [[0, 2], [1]], C).status_code == 400    # row 2 of 2 coefficients
    assert cl.worker_commit_shplonk([h], X, [["x"], [1]], C).status_code == 400     # not an index
    assert cl.worker_commit_shplonk([h], [], [], C).status_code == 400              # m = 0
    assert cl.worker_commit_shplonk([h], [fr(t) for t in range(9)], [[0]] * 9, C).status_code == 400   # m = 9
    assert cl.worker_commit_shplonk([h], X, O, []).status_code == 400               # k = 0
    assert cl.worker_commit_shplonk([h], X, [[0], [1]], [fr(1)] * 16).status_code == 400   # k = 16
    assert cl.worker_commit_shplonk([], X, O, C).status_code == 400                 # no handle
    assert cl.worker_commit_shplonk(["x"], X, O, C).status_code == 400              # not a handle
    assert cl.worker_commit_shplonk([h], ["not base64!", fr(1)], O, C).status_code == 400
    assert cl.worker_open_shplonk_finish([h], hh, X, O, C, fr(9)).status_code == 200
    assert cl.worker_open_shplonk_finish([h], hh, X, O, C, X[1]).status_code == 400   # u among the points
    assert cl.worker_open_shplonk_finish([h], "x", X, O, C, fr(9)).status_code == 400
    assert cl.worker_open_shplonk_finish([h], hh, X, O[:1], C, fr(9)).status_code == 400
    other = cl.worker_commit_rows(1, polys(1, 4, 8)).json()["handle"]
    assert cl.worker_commit_shplonk([h, other], X, O, C + [fr(1)]).status_code == 400   # two workers
    P, Cm, E = g1_to_b64(bytes(48)), [g1_to_b64(bytes(48))] * 2, [[fr(1), fr(2)], [fr(3)]]
    assert cl.worker_verify_open_shplonk(0, P, P, fr(9), X, O, C, E, Cm).status_code == 200
    assert cl.worker_verify_open_shplonk(0, P, P, fr(9), X, O, C, E, Cm[:1]).status_code == 400    # k != commitments
    assert cl.worker_verify_open_shplonk(0, P, P, fr(9), X, O, C, [E[0][:1], E[1]], Cm).status_code == 400
    assert cl.worker_verify_open_shplonk(0, P, P, fr(9), X, O, C, E[:1], Cm).status_code == 400
    assert Client(engine=None).worker_commit_shplonk([h], X, O, C).status_code == 503


def test_multi_device_client_routes_by_worker():
    engines = [FakeEngine(), FakeEngine(), FakeEngine()]
    multi = MultiDeviceClient(devices=[0, 1, 2], seed=5, engines=engines)
    assert multi.worker_verify_open_shplonk(0, "", "", "", [], [], [], [], []).status_code == 503   # not started yet
    assert multi.worker_commit_shplonk([1], [fr(1)], [[0]], [fr(1)]).status_code == 400            # no set is known yet
    multi.start(scale=7, machines_scale=2)
    try:
        X, O, C = [fr(31), fr(32)], [[0, 1, 2], [2]], [fr(1), fr(0), fr(9)]
        for i in range(4):
            a = multi.worker_commit_rows(i, polys(2, 8, 20 + i)).json()["handle"]
            b = multi.worker_commit_rows(i, polys(1, 8, 30 + i)).json()["handle"]
            g = i % 3
            r = multi.worker_commit_shplonk([a, b], X, O, C)
            assert r.status_code == 200, r.json()
            assert engines[g].calls[-1] == ("shplonk", (a, b))
            h = r.json()["handle"]
            f = multi.worker_open_shplonk_finish([a, b], h, X, O, C, fr(77))
            assert f.status_code == 200, f.json()
            assert engines[g].calls[-1] == ("finish", (a, b, h))
            local = engines[g].workers.index(i)
            v = multi.worker_verify_open_shplonk(i, r.json()["w"], f.json()["proof"], fr(77), X, O, C,
                                                 [[fr(1)] * 3, [fr(2)]], [g1_to_b64(bytes(48))] * 3)
            assert v.status_code == 200 and engines[g].calls[-1] == ("verify", local, 3, 2)
            assert multi.worker_release_rows(h).status_code == 200                          # h is a set like any other
            assert multi.worker_open_shplonk_finish([a, b], h, X, O, C, fr(77)).status_code == 400
        h0 = multi.worker_commit_rows(0, polys(1, 8, 50)).json()["handle"]
        h1 = multi.worker_commit_rows(1, polys(1, 8, 51)).json()["handle"]
        assert multi.worker_commit_shplonk([h0, h1], X[:1], [[0, 1]], [fr(1)] * 2).status_code == 400   # two workers
        assert multi.worker_commit_shplonk([10 ** 9], X[:1], [[0]], [fr(1)]).status_code == 400        # unknown handle
        hs = multi.worker_commit_shplonk([h0], X[:1], [[0]], [fr(1)]).json()["handle"]
        assert multi.worker_open_shplonk_finish([h1], hs, X[:1], [[0]], [fr(1)], fr(3)).status_code == 400   # h elsewhere
    finally:
        multi.stop()
