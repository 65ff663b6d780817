"""CPU-only tests of the quotient with rotated gate factors and the logUp relation (kzg_rows_commit_quotient_ext, its
kzg_multi_ form, HipEngine.commit_quotient_ext, the text forms on Client and MultiDeviceClient): the Python reference
(tests/quotient_ext_ref.py) pinned against schoolbook multiplication before the GPU is compared with it, what the two
lookup constraints and a next-row gate say about satisfied and broken instances, the C-ABI's argument checks without a
device, header / ctypes / Python signature agreement, and the host logic over a fake engine defined here."""
import ctypes
import hashlib
import inspect
import itertools
import os
import re

import pytest

from tests import grand_product_ref as gp
from tests import lookup_ref as lr
from tests import quotient_ext_ref as qx
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
def schoolbook_numerator(rows, terms, lookup):
    """Gate + alpha^3 LK1 + alpha^4 LK2 from the definition with schoolbook products of coefficient lists"""
    T = len(rows[0])
    w_T = gp.omega(T)
    mul = qr.mul_schoolbook
    acc = []
    for c, fs in terms:
        p = [c % R]
        for f in fs:
            j, rot = qx.factor(f)
            p = mul(p, qr.shift_arg(rows[j], pow(w_T, rot % T, R)))
        acc = qr.add(acc, p)
    if lookup:
        w, theta, beta, alpha = lookup["width"], lookup["theta"], lookup["beta"], lookup["alpha"]
        ins = lookup["inputs"]
        L = len(ins) // w
        dens = []
        for g in [lookup["table"]] + [ins[l * w:(l + 1) * w] for l in range(L)]:
            d = [beta]
            for c, j in enumerate(g):
                d = qr.add(d, qr.scale(rows[j], pow(theta, c, R)))
            dens.append(d)

        def prod(skip):
            p = [1]
            for l, d in enumerate(dens):
                if l not in skip:
                    p = mul(p, d)
            return p

        S = rows[lookup["sum"]]
        bracket = qr.scale(mul(rows[lookup["mult"]], prod({0})), R - 1)
        for l in range(1, L + 1):
            bracket = qr.add(bracket, prod({l}))
        lk1 = qr.sub(mul(qr.sub(qr.shift_arg(S, w_T), S), prod(set())), bracket)
        lk2 = mul(S, [pow(T, -1, R)] * T)
        acc = qr.add(acc, qr.add(qr.scale(lk1, pow(alpha, 3, R)), qr.scale(lk2, pow(alpha, 4, R))))
    return acc


@pytest.mark.parametrize("L,w,ext_log", [(1, 1, 1), (2, 2, 2), (3, 1, 2)])
def test_reference_against_schoolbook(L, w, ext_log):
    T = 8
    gate_rows = qx.next_row_instance(T, 5)
    lk_rows, lookup = qx.lookup_rows(L, w, T, 6, first_row=4)
    coef = [qr.coeffs_of(r) for r in gate_rows + lk_rows]
    terms = qx.next_row_terms() if ext_log >= 2 else [(1, [(qx.A_, 3), (qx.B_, -2)]), (5, [])]   # (not satisfied: num only)
    num = qx.numerator(coef, terms, None, lookup, ext_log)
    assert qr.trim(num) == qr.trim(schoolbook_numerator(coef, terms, lookup))
    # the rotated-factor route itself: f(w^rot X) takes the value of row t + rot at w^t
    a = gate_rows[0]
    for rot in (1, -1, 2, T + 1, -T - 3):
        assert qr.evals_of(qx.rotated(coef[0], rot)) == [a[(t + rot) % T] for t in range(T)]
    assert qx.rotated(coef[0], -1) == qx.rotated(coef[0], T - 1)
    # with a permutation part the reference adds quotient_ref's own numerator, pinned in test_quotient_cpu.py
    rows, sterms, perm, lk = qx.round_instance(T, 3)
    coef = [qr.coeffs_of(r) for r in rows]
    whole = qx.numerator(coef, sterms, perm, lk, 2)
    assert qr.trim(whole) == qr.trim(qr.add(qr.numerator(coef, sterms, perm, 2), schoolbook_numerator(coef, [], lk)))
    t, rem = qx.quotient(coef, sterms, perm, lk, 2)
    assert not any(rem) and qr.degree(t) == 3 * T - 4
    # num_at agrees with the polynomial at a point off the domain
    x = 0x1234567
    val = lambda j, rot: qr.poly_eval(coef[j], x * pow(gp.omega(T), rot % T, R) % R)   # noqa: E731
    assert qx.num_at(val, sterms, perm, lk, x, T) == qr.poly_eval(whole, x)


@pytest.mark.parametrize("L,w,ext_log,T", [(1, 1, 1, 8), (3, 2, 2, 16), (2, 3, 2, 8), (7, 1, 3, 8)])
def test_lk1_vanishes_exactly_for_a_real_lookup(L, w, ext_log, T):
    rows, lookup = qx.lookup_rows(L, w, T, 40 + L)
    coef = [qr.coeffs_of(r) for r in rows]
    t, rem = qx.quotient(coef, [], None, lookup, ext_log)
    assert not any(rem)
    assert qr.degree(t) <= (L + 1) * T - 1               # the lookup part alone fits L + 1 pieces
    qr.pieces(t, T, L + 1)
    # one input tuple outside the table: S no longer closes, and whichever S the prover picks LK1 or LK2 fails
    ins, tab, mult = lr.lookup_instance(L, w, T, 40 + L)
    broken = lr.break_instance(ins, tab, w, 9)
    S, closing = lr.lookup_sum(broken, tab, mult, L, w, lookup["theta"], lookup["beta"])
    assert closing != 0
    for S_row in (S, rows[-1]):                          # the broken sum's own S (wrap fails), the honest S (a row fails)
        bad = [qr.coeffs_of(r) for r in broken + tab + [mult, S_row]]
        _, rem = qx.quotient(bad, [], None, lookup, ext_log)
        assert any(rem)
    # LK2 alone: S(1) != 0 is caught even when the differences are right
    shifted = [(v + 1) % R for v in rows[-1]]
    _, rem = qx.quotient(coef[:-1] + [qr.coeffs_of(shifted)], [], None, lookup, ext_log)
    assert any(rem)


@pytest.mark.parametrize("T", [8, 16])
def test_next_row_gate_and_one_changed_cell(T):
    rows = qx.next_row_instance(T, 21)
    for terms in (qx.next_row_terms(), qx.next_row_terms(T, wrapped=True)):
        t, rem = qx.quotient([qr.coeffs_of(r) for r in rows], terms, None, None, 1)
        assert not any(rem) and qr.degree(t) <= T - 2
    for cell in (0, T - 1):                              # row T - 1 reads rows 0 and 1: the wrap
        bad = [list(r) for r in rows]
        bad[qx.Q_][cell] = (bad[qx.Q_][cell] + 1) % R
        _, rem = qx.quotient([qr.coeffs_of(r) for r in bad], qx.next_row_terms(), None, None, 1)
        assert any(rem)
    # without the rotations the same rows do not satisfy the gate
    flat = [(c, [qx.factor(f)[0] for f in fs]) for c, fs in qx.next_row_terms()]
    _, rem = qx.quotient([qr.coeffs_of(r) for r in rows], flat, None, None, 1)
    assert any(rem)


# ---------------------------------------------------------------------------------------------------- the C ABI
def _terms(terms):
    lens = (ctypes.c_uint32 * max(len(terms), 1))(*[len(r) for _, r in terms])
    flat = [qx.factor(f) for _, r in terms for f in r]
    rows = (ctypes.c_uint32 * max(len(flat), 1))(*[j for j, _ in flat])
    rots = (ctypes.c_int32 * max(len(flat), 1))(*[rot for _, rot in flat])
    return _native.QuotientTerms(len(terms), b"".join(c for c, _ in terms), lens, rows, rots), (lens, rows, rots)


def test_c_abi_null_context_or_pointers(lib):
    hs = (ctypes.c_uint64 * 1)(1)
    gate, _keep = _terms([(be(1), [(0, 1)])])
    one = (ctypes.c_uint32 * 1)(0)
    lk = _native.QuotientLookup(1, 1, one, one, 0, 0, be(1), be(2), be(3))
    c, h = ctypes.create_string_buffer(48 * 3), ctypes.c_uint64(0)
    f, m = lib.kzg_rows_commit_quotient_ext, lib.kzg_multi_rows_commit_quotient_ext
    assert f(None, 1, hs, ctypes.byref(gate), None, ctypes.byref(lk), 2, 3, c, ctypes.byref(h)) == E_ARG
    assert f(None, 1, None, None, None, None, 2, 3, None, None) == E_ARG
    assert m(None, 0, 1, hs, ctypes.byref(gate), None, ctypes.byref(lk), 2, 3, c, ctypes.byref(h)) == E_ARG
    assert m(None, 0, 1, None, None, None, None, 2, 3, c, None) == E_ARG
    assert h.value == 0


def test_header_symbols_and_python_signatures_agree():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "kzg_mi355x.h")).read()
    for name, extra in (("kzg_rows_commit_quotient_ext", 0), ("kzg_multi_rows_commit_quotient_ext", 1)):
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert proto, name
        assert name in _native.SYMBOLS, name
        res, args = _native.SYMBOLS[name]
        plain = re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S)
        assert res is ctypes.c_int and len(args) == plain.count(",") + 1 == 10 + extra
    for cname, cls in (("kzg_quotient_terms", _native.QuotientTerms), ("kzg_quotient_lookup", _native.QuotientLookup)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), hdr, re.S).group(1)
        fields = re.findall(r"(const \w+\*|uint32_t)\s+(\w+);", body)
        assert [n for _, n in fields] == [n for n, _ in cls._fields_], cname
        for (ctype, _), (_, pytype) in zip(fields, cls._fields_):
            assert (ctype == "uint32_t") == (pytype is ctypes.c_uint32), (cname, ctype)
    assert dict(_native.QuotientTerms._fields_)["term_rots"] is ctypes.POINTER(ctypes.c_int32)
    # the plain call's structs are untouched, and the gate struct is a prefix of the new one
    assert [n for n, _ in _native.QuotientTerms._fields_][:4] == [n for n, _ in _native.QuotientGate._fields_]
    for text in ("The powers 3 and 4 of alpha are FIXED", "so L <= E - 1", "NULL: every rotation 0",
                 "alpha must be drawn AFTER the commitments of S and z are fixed",
                 "is the lookup part of\n * kzg_rows_commit_quotient_ext"):
        assert text in hdr, text
    assert len(_native.TIMING_NAMES) == 12 and re.search(r"KZG_T_COLLECTIVE[^,]*,\s*KZG_T_COUNT", hdr)
    assert list(inspect.signature(HipEngine.commit_quotient_ext).parameters) == \
        ["self", "sets", "terms", "perm", "lookup", "ext_log", "n_pieces"]
    sig = inspect.signature(HipEngine.commit_quotient_ext).parameters
    assert (sig["perm"].default, sig["lookup"].default, sig["ext_log"].default, sig["n_pieces"].default) == (None, None, 2, 3)
    assert list(inspect.signature(MultiDeviceClient.worker_commit_quotient_ext).parameters) == \
        ["self", "handles", "terms", "perm", "lookup", "ext_log", "n_pieces"]


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
    lk = {"inputs": [0], "table": [1], "mult": 2, "sum": 3, "width": 1, "theta": one, "beta": one, "alpha": one}
    bad = [
        dict(sets=[], terms=[(one, [0])]),
        dict(sets=[1], terms=[(one, [0])], ext_log=0),
        dict(sets=[1], terms=[(one, [0])], n_pieces=5),
        dict(sets=[1], terms=[(one, [0])] * 17),
        dict(sets=[1], terms=[(one, [(0, 1)] * 6)]),                        # E + 2 factors
        dict(sets=[1], terms=[(one, [(0, 1, 2)])]),                         # not a pair
        dict(sets=[1], terms=[(one, [(0, 1 << 31)])]),                      # not an int32
        dict(sets=[1], terms=[(one, [(-1, 0)])]),
        dict(sets=[1], terms=[(one, ["x"])]),
        dict(sets=[1], terms=[]),                                           # nothing to compute
        dict(sets=[1], terms=[], perm=dict(perm, sigmas=[3, 4])),
        dict(sets=[1], terms=[], lookup=dict(lk, inputs=[])),               # L = 0
        dict(sets=[1], terms=[], lookup=dict(lk, width=0)),
        dict(sets=[1], terms=[], lookup=dict(lk, inputs=[0, 1, 2], width=2, table=[1, 2])),   # not L * w rows
        dict(sets=[1], terms=[], lookup=dict(lk, table=[1, 2])),
        dict(sets=[1], terms=[], lookup=dict(lk, inputs=[0] * 4)),          # L = 4 > E - 1 = 3
        dict(sets=[1], terms=[], lookup=dict(lk, inputs=[0, 1]), ext_log=1, n_pieces=2),      # L = 2 > E - 1 = 1
        dict(sets=[1], terms=[], lookup=dict(lk, inputs=[0] * 18, table=[1] * 6, width=6)),   # L w > 16
        dict(sets=[1], terms=[], lookup=dict(lk, theta=b"\x01")),
        dict(sets=[1], terms=[], lookup=dict(lk, mult=-1)),
        dict(sets=[1], terms=[], lookup={key: v for key, v in lk.items() if key != "sum"}),
        dict(sets=[1], terms=[], perm=perm, lookup=dict(lk, alpha=be(2))),  # two alphas
    ]
    for kw in bad:
        with pytest.raises(_native.KzgError) as ei:
            eng.commit_quotient_ext(**kw)
        assert ei.value.code == E_ARG, kw
    for kw in (dict(terms=[(one, [0, (1, -1)])]), dict(terms=[], lookup=lk), dict(terms=[], perm=perm, lookup=lk),
               dict(terms=[(one, [(0, 5)])], perm={"wires": [], "sigmas": []})):
        with pytest.raises(AssertionError, match="reached the library: kzg_rows_commit_quotient_ext"):
            eng.commit_quotient_ext([1], **kw)


class FakeEngine:
    """The set semantics of the library over stand-in arithmetic: the 'commitments' are hashes of what they depend on, so
    the text forms hand the right handles, indices, rotations and scalars through exactly when they match these."""

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

    def commit_quotient_ext(self, sets, terms, perm=None, lookup=None, ext_log=2, n_pieces=3):
        hs = [int(x) for x in sets]
        self.calls.append(("quot_ext", tuple(hs), ext_log, n_pieces))
        if any(h not in self.sets for h in hs):
            raise _native.KzgError(E_ARG, "unknown or released handle")
        if len({self.sets[h][0] for h in hs}) != 1:
            raise _native.KzgError(E_ARG, "all sets must belong to one worker")
        rows = [r for h in hs for r in self.sets[h][1]]
        named = [qx.factor(f)[0] for _, fs in terms for f in fs] + (perm["wires"] + perm["sigmas"] + [perm["z"]] if perm else [])
        named += lookup["inputs"] + lookup["table"] + [lookup["mult"], lookup["sum"]] if lookup else []
        if any(j >= len(rows) for j in named):
            raise _native.KzgError(E_ARG, "a row index is not below the number of rows named")
        blob = b"".join(rows) + repr((terms, perm, lookup, ext_log)).encode()
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


TERMS = [[fr(1), [3, [0, 1]]], [fr(1), [[4, -1], 0, 1]], [fr(9), []]]


def text_perm(**kw):
    p = {"wires": [0, 1, 2], "sigmas": [5, 6, 7], "z": 8, "shifts": [fr(1), fr(7), fr(49)], "beta": fr(5), "gamma": fr(6),
         "alpha": fr(4)}
    p.update(kw)
    return p


def text_lookup(**kw):
    p = {"inputs": [2], "table": [3], "mult": 4, "sum": 8, "width": 1, "theta": fr(2), "beta": fr(3), "alpha": fr(4)}
    p.update(kw)
    return p


def test_client_json_shape_and_400s():
    eng = FakeEngine()
    cl = client(eng)
    a = cl.worker_commit_rows(1, polys(5, 8, 1)).json()["handle"]
    b = cl.worker_commit_rows(1, polys(4, 8, 2)).json()["handle"]
    r = cl.worker_commit_quotient_ext(handles=[a, b], terms=TERMS, perm=text_perm(), lookup=text_lookup(), ext_log=2, n_pieces=3)
    assert r.status_code == 200, r.json()
    assert set(r.json()) == {"commitments", "handle"}
    assert eng.calls[-1] == ("quot_ext", (a, b), 2, 3)
    bt = [(fr_to_be32(c), [qx.factor(f) for f in fs]) for c, fs in TERMS]
    tp, tl = text_perm(), text_lookup()
    bp = dict(tp, shifts=[fr_to_be32(x) for x in tp["shifts"]], beta=fr_to_be32(tp["beta"]), gamma=fr_to_be32(tp["gamma"]),
              alpha=fr_to_be32(tp["alpha"]))
    bl = dict(tl, theta=fr_to_be32(tl["theta"]), beta=fr_to_be32(tl["beta"]), alpha=fr_to_be32(tl["alpha"]))
    rs = eng.commit_quotient_ext([a, b], bt, bp, bl, 2, 3)
    assert r.json()["commitments"] == [g1_to_b64(c) for c in rs.commitments] and len(r.json()["commitments"]) == 3
    assert isinstance(r.json()["handle"], int)
    assert cl.worker_release_rows(r.json()["handle"]).status_code == 200       # the new set releases like the others
    r = cl.worker_commit_quotient_ext([a], TERMS[:1])                          # the defaults: gate only, E = 4, P = 3
    assert r.status_code == 200 and eng.calls[-1] == ("quot_ext", (a,), 2, 3)
    assert cl.worker_commit_quotient_ext([a, b], [], None, text_lookup()).status_code == 200   # the lookup part alone
    ok = lambda *x, **kw: cl.worker_commit_quotient_ext(*x, **kw).status_code   # noqa: E731
    big = be32_to_fr(R.to_bytes(32, "big"))
    n_calls = len(eng.calls)
    assert ok([a, b], [[big, [0]]]) == 400                                     # a coefficient >= r
    for name in ("theta", "beta", "alpha"):
        assert ok([a, b], TERMS, None, text_lookup(**{name: big})) == 400
    assert ok([a, b], TERMS, text_perm(beta=big)) == 400
    assert ok([a, b], [["not base64!", [0]]]) == 400
    assert ok([a, b], [[fr(1), [["x", 1]]]]) == 400                            # not an index
    assert ok([a, b], [[fr(1), [[0, "up"]]]]) == 400                           # not a rotation
    assert ok([a, b], [[fr(1), [[0, 1, 2]]]]) == 400                           # not a pair
    assert ok([a, b], [[fr(1)]]) == 400                                        # a term without its factor list
    assert ok([a, b], TERMS, None, {"inputs": [0]}) == 400                     # an incomplete lookup part
    assert ok([a, b], TERMS, None, text_lookup(width="one")) == 400
    assert ok([], TERMS) == 400                                                # no handle
    assert ok(["x"], TERMS) == 400
    assert ok([a, b], TERMS, None, None, "two", 3) == 400
    assert len(eng.calls) == n_calls                                            # none of these reached the engine
    assert ok([a, b], [[fr(1), [[9, 1]]]]) == 400                              # row index == n
    assert ok([a, b], TERMS, None, text_lookup(sum=9)) == 400
    assert ok([a, 10 ** 9], TERMS) == 400                                      # unknown handle
    other = cl.worker_commit_rows(0, polys(4, 8, 4)).json()["handle"]
    assert ok([a, other], TERMS) == 400                                        # two workers
    assert Client(engine=None).worker_commit_quotient_ext([a], TERMS).status_code == 503
    # the engine's own checks answer 400 through the same route: two alphas, L > E - 1
    real = client(NoDevice())
    assert real.worker_commit_quotient_ext([1], TERMS, text_perm(), text_lookup(alpha=fr(5))).status_code == 400
    assert real.worker_commit_quotient_ext([1], TERMS, None, text_lookup(inputs=[0, 1]), 1, 2).status_code == 400


def test_multi_device_client_routes_by_worker():
    engines = [FakeEngine(), FakeEngine(), FakeEngine()]
    multi = MultiDeviceClient(devices=[0, 1, 2], seed=5, engines=engines)
    assert multi.worker_commit_quotient_ext([1], TERMS[:1]).status_code == 400     # no set is known yet
    multi.start(scale=7, machines_scale=2)
    try:
        made = {}
        for i in range(4):
            a = multi.worker_commit_rows(i, polys(9, 8, 20 + i)).json()["handle"]
            r = multi.worker_commit_quotient_ext([a], TERMS, text_perm(), text_lookup(), 2, 3)
            assert r.status_code == 200, r.json()
            assert engines[i % 3].calls[-1] == ("quot_ext", (a,), 2, 3)
            t = r.json()["handle"]
            # the new set is owned by the same worker: usable as a source, and released through the router
            assert multi.worker_commit_quotient_ext([a, t], [[fr(1), [[9, 1], 10, [11, -1]]]], None, None, 1, 2).status_code == 200
            made[i] = (a, t)
        (a0, t0), (a1, _) = made[0], made[1]
        assert multi.worker_commit_quotient_ext([a0, a1], TERMS).status_code == 400            # two workers
        assert multi.worker_commit_quotient_ext([10 ** 9], TERMS).status_code == 400
        assert multi.worker_commit_quotient_ext(["x"], TERMS).status_code == 400
        assert multi.worker_release_rows(t0).status_code == 200
        assert multi.worker_commit_quotient_ext([a0, t0], TERMS).status_code == 400            # released
    finally:
        multi.stop()
