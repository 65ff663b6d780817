"""CPU-only tests of the device-built permutation grand product (kzg_rows_commit_grand_product, its kzg_multi_ form,
HipEngine.commit_grand_product, the text forms on Client and MultiDeviceClient): the C-ABI's argument checks without a
device, header / ctypes / Python signature agreement, the host logic over a fake engine defined here, and the Python
reference (tests/grand_product_ref.py) itself, pinned on real permutations before the GPU is compared with it."""
import ctypes
import hashlib
import inspect
import itertools
import os
import re

import pytest

from tests import grand_product_ref as gp
from zkp_subnet_amd import MultiDeviceClient, _native
from zkp_subnet_amd.build import build
from zkp_subnet_amd.client import Client
from zkp_subnet_amd.codec import be32_to_fr, fr_to_be32, g1_to_b64
from zkp_subnet_amd.engine import HipEngine, RowSet, _root_of_unity

R = gp.R
E_ARG = _native.KZG_E_ARG
_HANDLES = itertools.count(1)
be = gp.be


@pytest.fixture(scope="module")
def lib():
    build()
    return _native.load()


def test_c_abi_null_context_or_pointers(lib):
    hs = (ctypes.c_uint64 * 1)(1)
    one = (1).to_bytes(32, "big")
    c, cl, h = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.c_uint64(0)
    f, m = lib.kzg_rows_commit_grand_product, lib.kzg_multi_rows_commit_grand_product
    assert f(None, 1, hs, 1, hs, 1, one, one, one, c, cl, ctypes.byref(h)) == E_ARG
    assert f(None, 1, None, 1, hs, 1, one, one, one, c, cl, ctypes.byref(h)) == E_ARG
    assert f(None, 1, hs, 1, None, 1, None, None, None, None, None, None) == E_ARG
    assert m(None, 0, 1, hs, 1, hs, 1, one, one, one, c, cl, ctypes.byref(h)) == E_ARG
    assert m(None, 0, 1, None, 1, None, 1, one, one, one, c, cl, None) == E_ARG
    assert h.value == 0


def test_header_symbols_and_python_signatures_agree():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "kzg_mi355x.h")).read()
    assert int(re.search(r"#define KZG_MAX_BATCH_OPEN (\d+)", hdr).group(1)) == _native.KZG_MAX_BATCH_OPEN
    assert int(re.search(r"#define KZG_MAX_ROW_SETS\s+(\d+)", hdr).group(1)) == _native.KZG_MAX_ROW_SETS
    for name, extra in (("kzg_rows_commit_grand_product", 0), ("kzg_multi_rows_commit_grand_product", 1)):
        proto = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert proto, name
        assert name in _native.SYMBOLS, name
        res, args = _native.SYMBOLS[name]
        assert res is ctypes.c_int and len(args) == proto.group(1).count(",") + 1 == 12 + extra
    assert "SOUNDNESS: beta and gamma must be drawn AFTER the wire commitments" in hdr and "NO BLINDING" in hdr
    thdr = open(os.path.join(root, "include", "kzg_mi355x_test.h")).read()
    assert "7 a^-1" in thdr and "zero flag" in thdr          # the inversion's hook: two Fr ops of kzg_test_field
    # the KZG_T_* enum is what the benchmark reads: no new stage
    assert len(_native.TIMING_NAMES) == 12 and re.search(r"KZG_T_COLLECTIVE[^,]*,\s*KZG_T_COUNT", hdr)
    assert list(inspect.signature(HipEngine.commit_grand_product).parameters) == \
        ["self", "wire_sets", "sigma_sets", "shifts_be32", "beta_be32", "gamma_be32"]
    # (Client's methods sit behind its error guard: test_client_json_shape_and_400s calls that one by keyword)
    assert list(inspect.signature(MultiDeviceClient.worker_commit_grand_product).parameters) == \
        ["self", "wire_handles", "sigma_handles", "shifts", "beta", "gamma"]


# ---------------------------------------------------------------------------------------------------- the reference
def test_reference_root_and_batch_inverse():
    for T in (1, 2, 16, 1 << 12):
        assert gp.omega(T) == _root_of_unity(T)
        assert pow(gp.omega(T), T, R) == 1 and (T == 1 or pow(gp.omega(T), T // 2, R) == R - 1)
    vals = [1, R - 1, 5, 0x1234567 << 200]
    assert gp.batch_inverse(vals) == [pow(v, -1, R) for v in vals]
    with pytest.raises(ZeroDivisionError):
        gp.batch_inverse([3, 0, 4])


@pytest.mark.parametrize("k,T,seed", [(1, 4, 1), (3, 16, 2), (5, 8, 3), (3, 64, 4)])
def test_reference_closes_on_a_real_permutation(k, T, seed):
    wires, sigmas, shifts = gp.permutation_instance(k, T, seed)
    dom = gp.domain(T)
    # the instance is what it claims to be: sigma is a bijection of the identity values, wires follow it
    ident = {shifts[j] * dom[t] % R: (j, t) for j in range(k) for t in range(T)}
    assert len(ident) == k * T
    assert sorted(v for row in sigmas for v in row) == sorted(ident)
    for j in range(k):
        for t in range(T):
            jj, tt = ident[sigmas[j][t]]
            assert wires[j][t] == wires[jj][tt]
    beta, gamma = 0xBE7A + seed, 0x6A44A + seed
    z, closing = gp.grand_product(wires, sigmas, shifts, beta, gamma)
    assert z[0] == 1 and closing == 1 and len(z) == T
    N, D = gp.factors(wires, sigmas, shifts, beta, gamma)
    for t in range(T):   # the step relation on the domain, the last step closing the cycle
        assert z[(t + 1) % T] * D[t] % R == z[t] * N[t] % R
    # the one-inversion identity the device path uses
    inv, pre, suf = pow(_prod(D), -1, R), 1, _prod(D)
    for t in range(T):
        assert z[t] == pre * suf % R * inv % R
        pre, suf = pre * N[t] % R, suf * pow(D[t], -1, R) % R
    # one wire value changed on a cycle of two or more cells: a copy constraint is broken and the product no longer closes
    j, t = next((j, t) for j in range(k) for t in range(T) if ident[sigmas[j][t]] != (j, t))
    wires[j][t] = (wires[j][t] + 1) % R
    z2, closing2 = gp.grand_product(wires, sigmas, shifts, beta, gamma)
    assert z2[0] == 1 and closing2 != 1


def _prod(vals):
    acc = 1
    for v in vals:
        acc = acc * v % R
    return acc


def test_reference_zero_denominator_raises():
    wires, sigmas, shifts = gp.permutation_instance(2, 8, 9)
    beta = 77
    gamma = -(wires[0][3] + beta * sigmas[0][3]) % R
    with pytest.raises(ZeroDivisionError):
        gp.grand_product(wires, sigmas, shifts, beta, gamma)


# ---------------------------------------------------------------------------------------------------- host logic
class FakeEngine:
    """The set semantics of the library over stand-in arithmetic: the 'commitment' and 'closing' are hashes of what they
    depend on, so the text forms hand the right handles and scalars through exactly when they match these."""

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

    def _rows(self, hs):
        if any(h not in self.sets for h in hs):
            raise _native.KzgError(E_ARG, "unknown or released handle")
        return [r for h in hs for r in self.sets[h][1]]

    def commit_grand_product(self, wire_sets, sigma_sets, shifts, beta, gamma):
        hw, hs = [int(x) for x in wire_sets], [int(x) for x in sigma_sets]
        self.calls.append(("gp", tuple(hw), tuple(hs)))
        a, sg = self._rows(hw), self._rows(hs)
        if len({self.sets[h][0] for h in hw + hs}) != 1:
            raise _native.KzgError(E_ARG, "all sets must belong to one worker")
        if len(a) != len(shifts) or len(sg) != len(shifts):
            raise _native.KzgError(E_ARG, "the wire sets and the sigma sets must each hold exactly k rows")
        blob = b"".join(a + sg + list(shifts)) + beta + gamma
        i, h = self.sets[hw[0]][0], next(_HANDLES)
        self.sets[h] = (i, [hashlib.sha256(b"Z" + blob).digest() * (len(a[0]) // 32)])
        return RowSet(self, h, i, 1, len(a[0]) // 32, [hashlib.sha384(b"Z" + blob).digest()]), hashlib.sha256(b"cl" + blob).digest()

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


def test_client_json_shape_and_400s():
    eng = FakeEngine()
    cl = client(eng)
    a = cl.worker_commit_rows(1, polys(2, 8, 1)).json()["handle"]
    b = cl.worker_commit_rows(1, polys(1, 8, 2)).json()["handle"]
    s = cl.worker_commit_rows(1, polys(3, 8, 3)).json()["handle"]
    S = [fr(1), fr(7), fr(49)]
    r = cl.worker_commit_grand_product(wire_handles=[a, b], sigma_handles=[s], shifts=S, beta=fr(5), gamma=fr(6))
    assert r.status_code == 200, r.json()
    assert set(r.json()) == {"commitment", "closing", "handle"}
    assert eng.calls[-1] == ("gp", (a, b), (s,))
    rs, closing = eng.commit_grand_product([a, b], [s], [fr_to_be32(x) for x in S], fr_to_be32(fr(5)), fr_to_be32(fr(6)))
    assert r.json()["commitment"] == g1_to_b64(rs.commitments[0]) and r.json()["closing"] == be32_to_fr(closing)
    assert isinstance(r.json()["handle"], int) and len(r.json()["closing"]) == 43
    assert cl.worker_release_rows(r.json()["handle"]).status_code == 200       # the new set releases like the others
    ok = lambda *x: cl.worker_commit_grand_product(*x).status_code   # noqa: E731
    assert ok([a, b], [s], S[:2], fr(5), fr(6)) == 400                          # two shifts for three rows
    assert ok([a, b], [s], S + [fr(2)], fr(5), fr(6)) == 400                    # four shifts
    assert ok([a], [s], S, fr(5), fr(6)) == 400                                 # ragged lists: 2 wire rows, 3 sigma rows
    assert ok([a, b], [s], [], fr(5), fr(6)) == 400                             # k = 0
    assert ok([a, b], [s], [fr(1)] * 17, fr(5), fr(6)) == 400                   # k = 17
    big = be32_to_fr(R.to_bytes(32, "big"))
    n_calls = len(eng.calls)
    assert ok([a, b], [s], S, big, fr(6)) == 400                                # beta >= r
    assert ok([a, b], [s], S, fr(5), big) == 400                                # gamma >= r
    assert ok([a, b], [s], [fr(1), big, fr(3)], fr(5), fr(6)) == 400            # a shift >= r
    assert ok([a, b], [s], S, "not base64!", fr(6)) == 400
    assert ok([], [s], S, fr(5), fr(6)) == 400                                  # no wire handle
    assert ok([a, b], ["x"], S, fr(5), fr(6)) == 400                            # not a handle
    assert ok([a] * 17, [s], S, fr(5), fr(6)) == 400                            # more than 16 handles
    assert len(eng.calls) == n_calls                                            # none of these reached the engine
    assert ok([a, b], [10 ** 9], S, fr(5), fr(6)) == 400                        # unknown handle
    other = cl.worker_commit_rows(0, polys(3, 8, 4)).json()["handle"]
    assert ok([a, b], [other], S, fr(5), fr(6)) == 400                          # two workers
    assert Client(engine=None).worker_commit_grand_product([a], [s], S, fr(5), fr(6)).status_code == 503
    assert ok([a, b], [s], S, fr(0), fr(0)) == 200                              # zero challenges are scalars like any other


def test_multi_device_client_routes_by_worker():
    engines = [FakeEngine(), FakeEngine(), FakeEngine()]
    multi = MultiDeviceClient(devices=[0, 1, 2], seed=5, engines=engines)
    assert multi.worker_commit_grand_product([1], [1], [fr(1)], fr(2), fr(3)).status_code == 400   # no set is known yet
    multi.start(scale=7, machines_scale=2)
    try:
        made = {}
        for i in range(4):
            a = multi.worker_commit_rows(i, polys(2, 8, 20 + i)).json()["handle"]
            s = multi.worker_commit_rows(i, polys(2, 8, 30 + i)).json()["handle"]
            r = multi.worker_commit_grand_product([a], [s], [fr(1), fr(7)], fr(8), fr(9))
            assert r.status_code == 200, r.json()
            assert engines[i % 3].calls[-1] == ("gp", (a,), (s,))
            z = r.json()["handle"]
            # the new set is owned by the same worker: usable as a source, and released through the router
            assert multi.worker_commit_grand_product([a], [z, z], [fr(1), fr(7)], fr(8), fr(9)).status_code == 200
            made[i] = (a, s, z)
        (a0, s0, z0), (a1, s1, _) = made[0], made[1]
        assert multi.worker_commit_grand_product([a0], [s1], [fr(1), fr(7)], fr(8), fr(9)).status_code == 400   # two workers
        assert multi.worker_commit_grand_product([a0, a1], [s0, s0], [fr(1)] * 4, fr(8), fr(9)).status_code == 400
        assert multi.worker_commit_grand_product([10 ** 9], [s0], [fr(1), fr(7)], fr(8), fr(9)).status_code == 400
        assert multi.worker_commit_grand_product(["x"], [s0], [fr(1), fr(7)], fr(8), fr(9)).status_code == 400
        assert multi.worker_release_rows(z0).status_code == 200
        assert multi.worker_commit_grand_product([a0], [z0, z0], [fr(1), fr(7)], fr(8), fr(9)).status_code == 400   # released
    finally:
        multi.stop()
