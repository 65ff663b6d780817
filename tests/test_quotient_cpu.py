"""CPU-only tests of the device-built PLONK quotient (kzg_rows_commit_quotient, its kzg_multi_ form,
HipEngine.commit_quotient, the text forms on Client and MultiDeviceClient): the Python reference (tests/quotient_ref.py)
pinned against schoolbook multiplication before the GPU is compared with it, the C-ABI's argument checks without a device,
header / ctypes / Python signature agreement, and the host logic over a fake engine defined here."""
import ctypes
import hashlib
import inspect
import itertools
import os
import re

import pytest

from tests import grand_product_ref as gp
from tests import quotient_ref as qr
from zkp_subnet_amd import MultiDeviceClient, _native
from zkp_subnet_amd.build import build
from zkp_subnet_amd.client import Client
from zkp_subnet_amd.codec import be32_to_fr, fr_to_be32, g1_to_b64
from zkp_subnet_amd.engine import HipEngine, RowSet

R = gp.R
E_ARG = _native.KZG_E_ARG
_HANDLES = itertools.count(1)
be = gp.be


@pytest.fixture(scope="module")
def lib():
    build()
    return _native.load()


# ---------------------------------------------------------------------------------------------------- the reference
def schoolbook_numerator(rows, terms, perm):
    """num from the definition with schoolbook products of coefficient lists (no transform anywhere)"""
    T = len(rows[0])
    acc = []
    for c, idx in terms:
        p = [c % R]
        for j in idx:
            p = qr.mul_schoolbook(p, rows[j])
        acc = qr.add(acc, p)
    if perm:
        beta, gamma, alpha = perm["beta"], perm["gamma"], perm["alpha"]
        z = rows[perm["z"]]
        A, B = z, qr.shift_arg(z, gp.omega(T))
        for a, s, sh in zip(perm["wires"], perm["sigmas"], perm["shifts"]):
            A = qr.mul_schoolbook(A, qr.add(rows[a], [gamma, beta * sh % R]))
            B = qr.mul_schoolbook(B, qr.add(qr.add(rows[a], qr.scale(rows[s], beta)), [gamma]))
        l0 = [pow(T, -1, R)] * T
        p2 = qr.mul_schoolbook(qr.sub(z, [1]), l0)
        acc = qr.add(acc, qr.add(qr.scale(qr.sub(A, B), alpha), qr.scale(p2, alpha * alpha % R)))
    return acc


@pytest.mark.parametrize("T,seed", [(4, 1), (8, 2), (16, 3)])
def test_reference_against_schoolbook_and_the_degree(T, seed):
    rows, terms, perm = qr.standard_instance(T, seed)
    coef = [qr.coeffs_of(r) for r in rows]
    assert [qr.evals_of(c) for c in coef] == rows
    num = qr.numerator(coef, terms, perm, 2)
    want = schoolbook_numerator(coef, terms, perm)
    assert qr.trim(num) == qr.trim(want)
    t, rem = qr.quotient(coef, terms, perm, 2)
    assert not any(rem)
    assert qr.degree(t) == 3 * T - 4
    # t (X^T - 1) == num, by schoolbook
    assert qr.trim(qr.mul_schoolbook(t, [R - 1] + [0] * (T - 1) + [1])) == qr.trim(want)
    ps = qr.pieces(t, T, 3)
    assert len(ps) == 3 and all(len(p) == T for p in ps) and sum(ps, [])[:len(t)] == t
    with pytest.raises(AssertionError):
        qr.pieces(t, T, 2)
    # L_0's closed form, as the header states it
    x = 0x1234567
    assert qr.poly_eval([pow(T, -1, R)] * T, x) == (pow(x, T, R) - 1) * pow(T * (x - 1), -1, R) % R


@pytest.mark.parametrize("T", [8, 16])
def test_reference_remainder_is_nonzero_after_one_qc_changes(T):
    rows, terms, perm = qr.standard_instance(T, 11)
    rows[qr.QC][3] = (rows[qr.QC][3] + 1) % R
    coef = [qr.coeffs_of(r) for r in rows]
    t, rem = qr.quotient(coef, terms, perm, 2)
    assert any(rem)
    # what the device sees instead: the interpolant of num / Z_H on a coset of the work domain has full degree
    E, g = 4, 7
    N = E * T
    wN = gp.omega(N)
    num = qr.numerator(coef, terms, perm, 2)
    ys = []
    for i in range(N):
        x = g * pow(wN, i, R) % R
        ys.append(qr.poly_eval(num, x) * pow(pow(x, T, R) - 1, -1, R) % R)
    c = qr.ints(qr.cpu.fr_ntt(qr.row_bytes(ys), True))
    c = [v * pow(g, -i, R) % R for i, v in enumerate(c)]
    assert qr.degree(c) == N - 1


def test_reference_other_shapes_and_division():
    q, rem = qr.divide_by_vanishing([5, 6, 7, 8, 9, 10, 11], 2)            # by X^2 - 1
    assert qr.trim(qr.add(qr.mul_schoolbook(q, [R - 1, 0, 1]), rem)) == [5, 6, 7, 8, 9, 10, 11]
    T = 8
    a = [3 + 5 * t for t in range(T)]
    rows = [qr.coeffs_of(a), qr.coeffs_of([-3 * pow(x, 5, R) % R for x in a])]
    t, rem = qr.quotient(rows, [(3, [0] * 5), (1, [1])], None, 2)           # a degree-5 term, a repeated index
    assert not any(rem) and qr.degree(t) <= 4 * T - 5
    t, rem = qr.quotient(rows, [(3, [0] * 5), (1, [1]), (1, [])], None, 2)  # + the constant 1: no longer vanishes
    assert any(rem)


# ---------------------------------------------------------------------------------------------------- the C ABI
def _gate(terms):
    lens = (ctypes.c_uint32 * max(len(terms), 1))(*[len(r) for _, r in terms])
    flat = [j for _, r in terms for j in r]
    rows = (ctypes.c_uint32 * max(len(flat), 1))(*flat)
    return _native.QuotientGate(len(terms), b"".join(c for c, _ in terms), lens, rows), (lens, rows)


def test_c_abi_null_context_or_pointers(lib):
    hs = (ctypes.c_uint64 * 1)(1)
    gate, _keep = _gate([(be(1), [0])])
    c, h = ctypes.create_string_buffer(48 * 3), ctypes.c_uint64(0)
    f, m = lib.kzg_rows_commit_quotient, lib.kzg_multi_rows_commit_quotient
    assert f(None, 1, hs, ctypes.byref(gate), None, 2, 3, c, ctypes.byref(h)) == E_ARG
    assert f(None, 1, None, None, None, 2, 3, None, None) == E_ARG
    assert m(None, 0, 1, hs, ctypes.byref(gate), None, 2, 3, c, ctypes.byref(h)) == E_ARG
    assert m(None, 0, 1, None, None, None, 2, 3, c, None) == E_ARG
    assert h.value == 0


def test_header_symbols_and_python_signatures_agree():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "kzg_mi355x.h")).read()
    assert int(re.search(r"#define KZG_MAX_GATE_TERMS (\d+)", hdr).group(1)) == _native.KZG_MAX_GATE_TERMS == 16
    for name, extra in (("kzg_rows_commit_quotient", 0), ("kzg_multi_rows_commit_quotient", 1)):
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert proto, name
        assert name in _native.SYMBOLS, name
        res, args = _native.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == proto.group(1).count(",") + 1 == 9 + extra
    # the argument structs: the same fields in the same order, pointers where the header has pointers
    for cname, cls in (("kzg_quotient_gate", _native.QuotientGate), ("kzg_quotient_perm", _native.QuotientPerm)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        fields = re.findall(r"(const \w+\*|uint32_t)\s+(\w+);", body)
        assert [n for _, n in fields] == [n for n, _ in cls._fields_], cname
        for (ctype, _), (_, pytype) in zip(fields, cls._fields_):
            assert (ctype == "uint32_t") == (pytype is ctypes.c_uint32), (cname, ctype)
    for text in ("SHAPE CHECK", "NECESSARY condition, NOT A PROOF", "When P = E nothing can be checked",
                 "alpha must be drawn AFTER z's commitment is fixed", "adds NO BLINDING here either"):
        assert text in hdr, text
    # no new timing stage, no new test hook
    assert len(_native.TIMING_NAMES) == 12 and re.search(r"KZG_T_COLLECTIVE[^,]*,\s*KZG_T_COUNT", hdr)
    thdr = open(os.path.join(root, "include", "kzg_mi355x_test.h")).read()
    assert "quotient" not in thdr
    assert list(inspect.signature(HipEngine.commit_quotient).parameters) == ["self", "sets", "terms", "perm", "ext_log", "n_pieces"]
    sig = inspect.signature(HipEngine.commit_quotient).parameters
    assert (sig["perm"].default, sig["ext_log"].default, sig["n_pieces"].default) == (None, 2, 3)
    assert list(inspect.signature(MultiDeviceClient.worker_commit_quotient).parameters) == \
        ["self", "handles", "terms", "perm", "ext_log", "n_pieces"]


# ---------------------------------------------------------------------------------------------------- host logic
class NoDevice(HipEngine):
    """HipEngine's own argument validation, with no library behind it: reaching the C call is an AssertionError"""

    def __init__(self):   # noqa: D107
        self._h = None

        class Lib:
            def __getattr__(self, name):
                raise AssertionError("the call reached the library: " + name)

        self._lib = Lib()

    def close(self):
        pass

    __del__ = close


def test_engine_argument_validation():
    eng = NoDevice()
    one = be(1)
    perm = {"wires": [0, 1, 2], "sigmas": [3, 4, 5], "z": 6, "shifts": [one] * 3, "beta": one, "gamma": one, "alpha": one}
    bad = [
        dict(sets=[], terms=[(one, [0])]),
        dict(sets=[1] * 17, terms=[(one, [0])]),
        dict(sets=[1], terms=[(one, [0])], ext_log=0),
        dict(sets=[1], terms=[(one, [0])], ext_log=4),
        dict(sets=[1], terms=[(one, [0])], n_pieces=0),
        dict(sets=[1], terms=[(one, [0])], n_pieces=5),
        dict(sets=[1], terms=[(one, [0])] * 17),
        dict(sets=[1], terms=[(one[:31], [0])]),
        dict(sets=[1], terms=[(one, [0] * 6)]),                             # E + 2 factors
        dict(sets=[1], terms=[(one, [-1])]),
        dict(sets=[1], terms=[]),                                           # nothing to compute
        dict(sets=[1], terms=[], perm=dict(perm, sigmas=[3, 4])),
        dict(sets=[1], terms=[], perm=dict(perm, shifts=[one] * 2)),
        dict(sets=[1], terms=[], perm=dict(perm, beta=b"\x01")),
        dict(sets=[1], terms=[], perm=dict(perm, z=-1)),
        dict(sets=[1], terms=[], perm=perm, ext_log=1, n_pieces=1),         # k = 3 > E = 2
        dict(sets=[1], terms=[], perm=dict(perm, wires=[], sigmas=[], shifts=[])),     # k = 0 and no term: nothing to compute
        dict(sets=[1], terms=[(one, [0])], perm=dict(perm, wires=[])),                 # sigma rows without wires
        dict(sets=[1], terms=[], perm={key: v for key, v in perm.items() if key != "z"}),   # a missing key is KZG_E_ARG too
        dict(sets=[1], terms=[], perm=dict(perm, wires=["x", 1, 2])),
    ]
    for kw in bad:
        with pytest.raises(_native.KzgError) as ei:
            eng.commit_quotient(**kw)
        assert ei.value.code == E_ARG, kw
    with pytest.raises(AssertionError, match="reached the library"):
        eng.commit_quotient([1], [(one, [0])], perm)
    # k = 0 switches the permutation part off, as perm->k == 0 does in C: the call goes through as gate-only
    with pytest.raises(AssertionError, match="reached the library"):
        eng.commit_quotient([1], [(one, [0])], {"wires": [], "sigmas": []})


class FakeEngine:
    """The set semantics of the library over stand-in arithmetic: the 'commitments' are hashes of what they depend on, so
    the text forms hand the right handles, indices and scalars through exactly when they match these."""

    def __init__(self):
        self.sets = {}
        self.calls = []
        self.workers = None

    def gen_srs(self, tau_x, tau_y, scale, machines_scale, workers=None):
        self.workers = list(workers) if workers is not None else list(range(1 << machines_scale))

    def commit_rows(self, i, rows, evaluation_form=True):
        h = next(_HANDLES)
        self.sets[h] = (i, list(rows))
        return RowSet(self, h, i, len(rows), len(rows[0]) // 32, [hashlib.sha384(b"C" + r).digest() for r in rows])

    def commit_quotient(self, sets, terms, perm=None, ext_log=2, n_pieces=3):
        hs = [int(x) for x in sets]
        self.calls.append(("quot", tuple(hs), ext_log, n_pieces))
        if any(h not in self.sets for h in hs):
            raise _native.KzgError(E_ARG, "unknown or released handle")
        if len({self.sets[h][0] for h in hs}) != 1:
            raise _native.KzgError(E_ARG, "all sets must belong to one worker")
        rows = [r for h in hs for r in self.sets[h][1]]
        named = [j for _, idx in terms for j in idx] + (perm["wires"] + perm["sigmas"] + [perm["z"]] if perm else [])
        if any(j >= len(rows) for j in named):
            raise _native.KzgError(E_ARG, "a row index is not below the number of rows named")
        blob = b"".join(rows) + repr((terms, perm, ext_log)).encode()
        i, h = self.sets[hs[0]][0], next(_HANDLES)
        self.sets[h] = (i, [hashlib.sha256(b"T%d" % p + blob).digest() * (len(rows[0]) // 32) for p in range(n_pieces)])
        return RowSet(self, h, i, n_pieces, len(rows[0]) // 32, [hashlib.sha384(b"T%d" % p + blob).digest() for p in range(n_pieces)])

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


TERMS = [[fr(1), [3, 0]], [fr(1), [4, 0, 1]], [fr(9), []]]


def text_perm(**kw):
    p = {"wires": [0, 1, 2], "sigmas": [5, 6, 7], "z": 8, "shifts": [fr(1), fr(7), fr(49)], "beta": fr(5), "gamma": fr(6),
         "alpha": fr(4)}
    p.update(kw)
    return p


def test_client_json_shape_and_400s():
    eng = FakeEngine()
    cl = client(eng)
    a = cl.worker_commit_rows(1, polys(5, 8, 1)).json()["handle"]
    b = cl.worker_commit_rows(1, polys(4, 8, 2)).json()["handle"]
    r = cl.worker_commit_quotient(handles=[a, b], terms=TERMS, perm=text_perm(), ext_log=2, n_pieces=3)
    assert r.status_code == 200, r.json()
    assert set(r.json()) == {"commitments", "handle"}
    assert eng.calls[-1] == ("quot", (a, b), 2, 3)
    bt = [(fr_to_be32(c), idx) for c, idx in TERMS]
    tp = text_perm()
    bp = dict(tp, shifts=[fr_to_be32(x) for x in tp["shifts"]], beta=fr_to_be32(tp["beta"]), gamma=fr_to_be32(tp["gamma"]),
              alpha=fr_to_be32(tp["alpha"]))
    rs = eng.commit_quotient([a, b], bt, bp, 2, 3)
    assert r.json()["commitments"] == [g1_to_b64(c) for c in rs.commitments] and len(r.json()["commitments"]) == 3
    assert isinstance(r.json()["handle"], int)
    assert cl.worker_release_rows(r.json()["handle"]).status_code == 200       # the new set releases like the others
    r = cl.worker_commit_quotient([a], TERMS[:1])                              # the defaults: gate only, E = 4, P = 3
    assert r.status_code == 200 and eng.calls[-1] == ("quot", (a,), 2, 3)
    ok = lambda *x, **kw: cl.worker_commit_quotient(*x, **kw).status_code   # noqa: E731
    big = be32_to_fr(R.to_bytes(32, "big"))
    n_calls = len(eng.calls)
    assert ok([a, b], [[big, [0]]]) == 400                                     # a coefficient >= r
    for name in ("beta", "gamma", "alpha"):
        assert ok([a, b], TERMS, text_perm(**{name: big})) == 400
    assert ok([a, b], TERMS, text_perm(shifts=[fr(1), big, fr(3)])) == 400
    assert ok([a, b], [["not base64!", [0]]]) == 400
    assert ok([a, b], [[fr(1), ["x"]]]) == 400                                 # not an index
    assert ok([a, b], [[fr(1)]]) == 400                                        # a term without its row list
    assert ok([a, b], TERMS, {"wires": [0]}) == 400                            # an incomplete permutation part
    assert ok([], TERMS) == 400                                                # no handle
    assert ok(["x"], TERMS) == 400
    assert ok([a] * 17, TERMS) == 400
    assert ok([a, b], TERMS, None, "two", 3) == 400
    assert len(eng.calls) == n_calls                                            # none of these reached the engine
    assert ok([a, b], [[fr(1), [9]]]) == 400                                   # row index == n
    assert ok([a, 10 ** 9], TERMS) == 400                                      # unknown handle
    other = cl.worker_commit_rows(0, polys(4, 8, 4)).json()["handle"]
    assert ok([a, other], TERMS) == 400                                        # two workers
    assert Client(engine=None).worker_commit_quotient([a], TERMS).status_code == 503
    assert ok([a, b], TERMS, text_perm(beta=fr(0), gamma=fr(0), alpha=fr(0))) == 200   # zero challenges are scalars too


def test_multi_device_client_routes_by_worker():
    engines = [FakeEngine(), FakeEngine(), FakeEngine()]
    multi = MultiDeviceClient(devices=[0, 1, 2], seed=5, engines=engines)
    assert multi.worker_commit_quotient([1], TERMS[:1]).status_code == 400     # no set is known yet
    multi.start(scale=7, machines_scale=2)
    try:
        made = {}
        for i in range(4):
            a = multi.worker_commit_rows(i, polys(9, 8, 20 + i)).json()["handle"]
            r = multi.worker_commit_quotient([a], TERMS, text_perm(), 2, 3)
            assert r.status_code == 200, r.json()
            assert engines[i % 3].calls[-1] == ("quot", (a,), 2, 3)
            t = r.json()["handle"]
            # the new set is owned by the same worker: usable as a source, and released through the router
            assert multi.worker_commit_quotient([a, t], [[fr(1), [9, 10, 11]]], None, 1, 2).status_code == 200
            made[i] = (a, t)
        (a0, t0), (a1, _) = made[0], made[1]
        assert multi.worker_commit_quotient([a0, a1], TERMS).status_code == 400            # two workers
        assert multi.worker_commit_quotient([10 ** 9], TERMS).status_code == 400
        assert multi.worker_commit_quotient(["x"], TERMS).status_code == 400
        assert multi.worker_release_rows(t0).status_code == 200
        assert multi.worker_commit_quotient([a0, t0], TERMS).status_code == 400            # released
    finally:
        multi.stop()
