"""CPU-only tests of the device-built lookup running sum (kzg_rows_commit_lookup_sum, its kzg_multi_ form,
HipEngine.commit_lookup_sum, the text forms on Client and MultiDeviceClient): the C-ABI's argument checks without a device,
the host logic over a fake engine defined here, and the Python reference (tests/lookup_ref.py) itself, pinned on real lookup
instances before the GPU is compared with it."""
import ctypes
import hashlib
import inspect
import itertools

import pytest

from tests import lookup_ref as lk
from zkp_subnet_amd import MultiDeviceClient, _native
from zkp_subnet_amd.build import build
from zkp_subnet_amd.client import Client
from zkp_subnet_amd.codec import be32_to_fr, fr_to_be32, g1_to_b64
from zkp_subnet_amd.engine import HipEngine, RowSet

R = lk.R
E_ARG = _native.KZG_E_ARG
_HANDLES = itertools.count(1)


@pytest.fixture(scope="module")
def lib():
    build()
    return _native.load()


def test_c_abi_null_context_or_pointers(lib):
    hs = (ctypes.c_uint64 * 1)(1)
    one = (1).to_bytes(32, "big")
    c, cl, h = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.c_uint64(0)
    f, m = lib.kzg_rows_commit_lookup_sum, lib.kzg_multi_rows_commit_lookup_sum
    assert f(None, 1, hs, 1, hs, 1, 1, 1, one, one, c, cl, ctypes.byref(h)) == E_ARG
    assert f(None, 1, None, 1, None, 1, 1, 1, None, None, None, None, None) == E_ARG
    assert m(None, 0, 1, hs, 1, hs, 1, 1, 1, one, one, c, cl, ctypes.byref(h)) == E_ARG


def test_python_signatures():
    want = ["input_sets", "table_sets", "mult_set", "n_lookups", "width", "theta_be32", "beta_be32"]
    assert list(inspect.signature(HipEngine.commit_lookup_sum).parameters)[1:] == want
    assert list(inspect.signature(MultiDeviceClient.worker_commit_lookup_sum).parameters)[1:] == \
        ["input_handles", "table_handles", "mult_handle", "n_lookups", "width", "theta", "beta"]


# ---------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("width", [1, 3])
@pytest.mark.parametrize("n_lookups", [1, 2, 4])
@pytest.mark.parametrize("T", [8, 16, 64])
def test_reference_closes_on_built_instances_and_not_after_the_breaker(T, n_lookups, width):
    for dup in (False, True):
        inputs, table, mult = lk.lookup_instance(n_lookups, width, T, 1000 * T + 10 * n_lookups + width, duplicates=dup)
        assert sum(mult) == n_lookups * T
        theta, beta = 0x7E7A + T, 0xBE7A + width
        S, closing = lk.lookup_sum(inputs, table, mult, n_lookups, width, theta, beta)
        assert closing == 0 and S[0] == 0 and len(S) == T
        term = lk.terms(inputs, table, mult, n_lookups, width, theta, beta)
        for t in range(T):
            assert (S[(t + 1) % T] - S[t] - term[t]) % R == 0    # (the wrap-around step holds because the sum closes)
        # term_t from the definition, one pow per denominator
        F = [lk.compress(inputs[l * width:(l + 1) * width], theta) for l in range(n_lookups)]
        Tb = lk.compress(table, theta)
        for t in (0, T // 2, T - 1):
            want = sum(pow(beta + F[l][t], -1, R) for l in range(n_lookups)) - mult[t] * pow(beta + Tb[t], -1, R)
            assert term[t] == want % R
        broken = lk.break_instance(inputs, table, width, T + n_lookups)
        S2, closing2 = lk.lookup_sum(broken, table, mult, n_lookups, width, theta, beta)
        assert S2[0] == 0 and closing2 != 0
        term2 = lk.terms(broken, table, mult, n_lookups, width, theta, beta)
        for t in range(T - 1):
            assert (S2[t + 1] - S2[t] - term2[t]) % R == 0


def test_reference_compress_is_the_power_sum():
    cols = [[3, 4], [5, 6], [7, 8]]
    assert lk.compress(cols, 10) == [3 + 50 + 700, 4 + 60 + 800]
    assert lk.compress(cols[:1], 12345) == cols[0]


def test_reference_duplicates_put_the_counts_on_the_first_copy():
    inputs, table, mult = lk.lookup_instance(2, 1, 16, 5, duplicates=True)
    seen = set()
    for t in range(16):
        if table[0][t] in seen:
            assert mult[t] == 0
        seen.add(table[0][t])
    assert len(seen) < 16


def test_reference_zero_denominator_raises():
    inputs, table, mult = lk.lookup_instance(2, 3, 8, 9)
    theta = 77
    for cols in (inputs[3:6], table):
        beta = -lk.compress(cols, theta)[5] % R
        with pytest.raises(ZeroDivisionError):
            lk.lookup_sum(inputs, table, mult, 2, 3, theta, beta)


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

    def commit_lookup_sum(self, input_sets, table_sets, mult_set, n_lookups, width, theta, beta):
        hi, ht, hm = [int(x) for x in input_sets], [int(x) for x in table_sets], int(mult_set)
        self.calls.append(("lk", tuple(hi), tuple(ht), hm, n_lookups, width))
        f, t, m = self._rows(hi), self._rows(ht), self._rows([hm])
        if len({self.sets[h][0] for h in hi + ht + [hm]}) != 1:
            raise _native.KzgError(E_ARG, "all sets must belong to one worker")
        if len(f) != n_lookups * width or len(t) != width or len(m) != 1:
            raise _native.KzgError(E_ARG, "the input sets must hold exactly n_lookups * width rows")
        blob = b"".join(f + t + m) + theta + beta
        i, h = self.sets[hi[0]][0], next(_HANDLES)
        self.sets[h] = (i, [hashlib.sha256(b"S" + blob).digest() * (len(f[0]) // 32)])
        return RowSet(self, h, i, 1, len(f[0]) // 32, [hashlib.sha384(b"S" + blob).digest()]), hashlib.sha256(b"cl" + blob).digest()

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
    a = cl.worker_commit_rows(1, polys(4, 8, 1)).json()["handle"]     # two lookups of width 2 ...
    b = cl.worker_commit_rows(1, polys(2, 8, 2)).json()["handle"]     # ... and a third
    t = cl.worker_commit_rows(1, polys(2, 8, 3)).json()["handle"]
    m = cl.worker_commit_rows(1, polys(1, 8, 4)).json()["handle"]
    r = cl.worker_commit_lookup_sum(input_handles=[a, b], table_handles=[t], mult_handle=m, n_lookups=3, width=2,
                                    theta=fr(5), beta=fr(6))
    assert r.status_code == 200, r.json()
    assert set(r.json()) == {"commitment", "closing", "handle"}
    assert eng.calls[-1] == ("lk", (a, b), (t,), m, 3, 2)
    rs, closing = eng.commit_lookup_sum([a, b], [t], m, 3, 2, fr_to_be32(fr(5)), fr_to_be32(fr(6)))
    assert r.json()["commitment"] == g1_to_b64(rs.commitments[0]) and r.json()["closing"] == be32_to_fr(closing)
    assert isinstance(r.json()["handle"], int) and len(r.json()["closing"]) == 43
    assert cl.worker_release_rows(r.json()["handle"]).status_code == 200       # the new set releases like the others
    ok = lambda *x: cl.worker_commit_lookup_sum(*x).status_code   # noqa: E731
    assert ok([a, b], [t], m, 2, 2, fr(5), fr(6)) == 400                        # six input rows for L w = 4
    assert ok([a, b], [t], m, 2, 3, fr(5), fr(6)) == 400                        # two table rows for w = 3
    assert ok([a, b], [t], t, 3, 2, fr(5), fr(6)) == 400                        # a two-row multiplicity set
    big = be32_to_fr(R.to_bytes(32, "big"))
    n_calls = len(eng.calls)
    assert ok([a, b], [t], m, 0, 2, fr(5), fr(6)) == 400                        # L = 0
    assert ok([a, b], [t], m, 3, 0, fr(5), fr(6)) == 400                        # w = 0
    assert ok([a, b], [t], m, 9, 2, fr(5), fr(6)) == 400                        # L w = 18
    assert ok([a, b], [t], m, 17, 1, fr(5), fr(6)) == 400                       # L = 17
    assert ok([a, b], [t], m, "three", 2, fr(5), fr(6)) == 400                  # not a number
    assert ok([a, b], [t], m, 3, 2, big, fr(6)) == 400                          # theta >= r
    assert ok([a, b], [t], m, 3, 2, fr(5), big) == 400                          # beta >= r
    assert ok([a, b], [t], m, 3, 2, "not base64!", fr(6)) == 400
    assert ok([], [t], m, 3, 2, fr(5), fr(6)) == 400                            # no input handle
    assert ok([a, b], [], m, 3, 2, fr(5), fr(6)) == 400                         # no table handle
    assert ok([a, b], ["x"], m, 3, 2, fr(5), fr(6)) == 400                      # not a handle
    assert ok([a, b], [t], "x", 3, 2, fr(5), fr(6)) == 400
    assert ok([a] * 17, [t], m, 3, 2, fr(5), fr(6)) == 400                      # more than 16 handles
    assert len(eng.calls) == n_calls                                            # none of these reached the engine
    assert ok([a, b], [10 ** 9], m, 3, 2, fr(5), fr(6)) == 400                  # unknown handle
    other = cl.worker_commit_rows(0, polys(1, 8, 5)).json()["handle"]
    assert ok([a, b], [t], other, 3, 2, fr(5), fr(6)) == 400                    # two workers
    assert Client(engine=None).worker_commit_lookup_sum([a], [t], m, 1, 2, fr(5), fr(6)).status_code == 503
    assert ok([a, b], [t], m, 3, 2, fr(0), fr(0)) == 200                        # zero challenges are scalars like any other


def test_multi_device_client_routes_by_worker():
    engines = [FakeEngine(), FakeEngine(), FakeEngine()]
    multi = MultiDeviceClient(devices=[0, 1, 2], seed=5, engines=engines)
    assert multi.worker_commit_lookup_sum([1], [1], 1, 1, 1, fr(2), fr(3)).status_code == 400   # no set is known yet
    multi.start(scale=7, machines_scale=2)
    try:
        made = {}
        for i in range(4):
            a = multi.worker_commit_rows(i, polys(2, 8, 20 + i)).json()["handle"]
            t = multi.worker_commit_rows(i, polys(1, 8, 30 + i)).json()["handle"]
            m = multi.worker_commit_rows(i, polys(1, 8, 40 + i)).json()["handle"]
            r = multi.worker_commit_lookup_sum([a], [t], m, 2, 1, fr(8), fr(9))
            assert r.status_code == 200, r.json()
            assert engines[i % 3].calls[-1] == ("lk", (a,), (t,), m, 2, 1)
            s = r.json()["handle"]
            # the new set is owned by the same worker: usable as a source, and released through the router
            assert multi.worker_commit_lookup_sum([s, s], [t], s, 2, 1, fr(8), fr(9)).status_code == 200
            made[i] = (a, t, m, s)
        (a0, t0, m0, s0), (a1, t1, m1, _) = made[0], made[1]
        assert multi.worker_commit_lookup_sum([a0], [t1], m0, 2, 1, fr(8), fr(9)).status_code == 400   # two workers
        assert multi.worker_commit_lookup_sum([a0], [t0], m1, 2, 1, fr(8), fr(9)).status_code == 400
        assert multi.worker_commit_lookup_sum([10 ** 9], [t0], m0, 2, 1, fr(8), fr(9)).status_code == 400
        assert multi.worker_commit_lookup_sum(["x"], [t0], m0, 2, 1, fr(8), fr(9)).status_code == 400
        assert multi.worker_commit_lookup_sum([a0], [t0], None, 2, 1, fr(8), fr(9)).status_code == 400
        assert multi.worker_release_rows(s0).status_code == 200
        assert multi.worker_commit_lookup_sum([a0], [t0], s0, 2, 1, fr(8), fr(9)).status_code == 400   # released
    finally:
        multi.stop()
