"""CPU-only checks of kzg_rows_commit_multiplicities: the Python reference (tests/multiplicities_ref.py) against an O(T^2)
brute force and against the instance builder of the lookup sum, the lookup sum closing over the reference's m, the library's
export, prototype and status code without a device, and the text forms on Client and MultiDeviceClient over a fake engine."""
import ctypes
import hashlib
import inspect
import itertools
import random

import pytest

from tests import lookup_ref as lk
from tests.multiplicities_ref import multiplicities
from zkp_subnet_amd import MultiDeviceClient, _native
from zkp_subnet_amd.build import build
from zkp_subnet_amd.client import Client
from zkp_subnet_amd.codec import be32_to_fr, g1_to_b64
from zkp_subnet_amd.engine import HipEngine

R = lk.R
_HANDLES = itertools.count(1)   # one numbering over every fake engine, as the library has one per process


def brute(inputs, table, L, w):
    """the definition, with no dictionary: every cell against every table row, the first equal row takes the hit"""
    T = len(table[0])
    mult, missing = [0] * T, 0
    for l in range(L):
        for t in range(T):
            cell = [inputs[l * w + c][t] for c in range(w)]
            for u in range(T):
                if all(table[c][u] == cell[c] for c in range(w)):
                    mult[u] += 1
                    break
            else:
                missing += 1
    return mult, missing


@pytest.mark.parametrize("T", [8, 32])
@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (2, 3)], ids=lambda s: f"L{s[0]}w{s[1]}")
@pytest.mark.parametrize("duplicates", [False, True])
@pytest.mark.parametrize("misses", [0, 1, 5])
def test_reference_against_brute_force(T, shape, duplicates, misses):
    L, w = shape
    inputs, table, _ = lk.lookup_instance(L, w, T, 17 * T + 3 * L + w, duplicates=duplicates)
    for n in range(misses):
        inputs = lk.break_instance(inputs, table, w, 900 + n)
    mult, missing = multiplicities(inputs, table, L, w)
    assert (mult, missing) == brute(inputs, table, L, w)
    assert sum(mult) + missing == L * T
    assert missing <= misses and (missing > 0) == (misses > 0)
    if duplicates:
        rows = [tuple(col[t] for col in table) for t in range(T)]
        assert all(mult[t] == 0 for t in range(T) if rows.index(rows[t]) != t)   # a later copy takes nothing


def test_reference_sees_a_swapped_pair_as_a_miss():
    table = [[1, 2, 3, 4], [5, 6, 7, 8]]
    inputs = [[5, 2, 3, 4], [1, 6, 7, 8]]                                   # (5, 1) where the table holds (1, 5)
    assert multiplicities(inputs, table, 1, 2) == ([0, 1, 1, 1], 1)


@pytest.mark.parametrize("duplicates", [False, True])
def test_reference_reproduces_the_instance_builder(duplicates):
    for L, w, T in ((1, 1, 16), (3, 2, 64), (2, 3, 32)):
        inputs, table, mult = lk.lookup_instance(L, w, T, 5 + L + w, duplicates=duplicates)
        assert multiplicities(inputs, table, L, w) == (mult, 0)


def test_the_lookup_sum_closes_over_the_reference_multiplicities():
    rnd = random.Random(7)
    for L, w, T in ((1, 1, 8), (3, 2, 32)):
        inputs, table, _ = lk.lookup_instance(L, w, T, 70 + L, duplicates=True)
        mult, missing = multiplicities(inputs, table, L, w)
        assert missing == 0
        assert lk.lookup_sum(inputs, table, mult, L, w, rnd.randrange(R), rnd.randrange(R))[1] == 0
        broken = lk.break_instance(inputs, table, w, 71)
        mult, missing = multiplicities(broken, table, L, w)
        assert missing == 1
        assert lk.lookup_sum(broken, table, mult, L, w, rnd.randrange(R), rnd.randrange(R))[1] != 0


def test_the_library_exports_the_call_and_answers_a_status_code_without_a_device():
    build()
    lib = _native.load()
    for name in ("kzg_rows_commit_multiplicities", "kzg_multi_rows_commit_multiplicities"):
        assert hasattr(lib, name) and name in _native.SYMBOLS
    h = (ctypes.c_uint64 * 1)(1)
    c, miss, out = ctypes.create_string_buffer(48), ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib.kzg_rows_commit_multiplicities(None, 1, h, 1, h, 1, 1, c, ctypes.byref(miss), ctypes.byref(out)) == _native.KZG_E_ARG
    assert lib.kzg_multi_rows_commit_multiplicities(None, 0, 1, h, 1, h, 1, 1, c, ctypes.byref(miss),
                                                    ctypes.byref(out)) == _native.KZG_E_ARG


# ---------------------------------------------------------------------------------------------------- host logic
class FakeEngine:
    """The set semantics of the library over the Python reference: m really is the multiplicity row of the stored rows, its
    'commitment' a hash of it, so the text forms hand the right handles through exactly when the counts match."""

    def __init__(self):
        self.sets, self.calls, self.workers = {}, [], None

    def gen_srs(self, tau_x, tau_y, scale, machines_scale, workers=None):
        self.workers = list(workers) if workers is not None else list(range(1 << machines_scale))

    def commit_rows(self, i, rows, evaluation_form=True):
        from zkp_subnet_amd.engine import RowSet

        h = next(_HANDLES)
        self.sets[h] = (i, list(rows))
        return RowSet(self, h, i, len(rows), len(rows[0]) // 32, [hashlib.sha384(b"C" + r).digest() for r in rows])

    def _rows(self, hs):
        if any(h not in self.sets for h in hs):
            raise _native.KzgError(_native.KZG_E_ARG, "multiplicities: unknown or released handle")
        return [r for h in hs for r in self.sets[h][1]]

    def commit_multiplicities(self, input_sets, table_sets, n_lookups, width):
        from zkp_subnet_amd.engine import RowSet

        hi, ht = [int(x) for x in input_sets], [int(x) for x in table_sets]
        self.calls.append(("mult", tuple(hi), tuple(ht), n_lookups, width))
        f, t = self._rows(hi), self._rows(ht)
        if len({self.sets[h][0] for h in hi + ht}) != 1:
            raise _native.KzgError(_native.KZG_E_ARG, "multiplicities: all sets must belong to one worker")
        if len(f) != n_lookups * width or len(t) != width:
            raise _native.KzgError(_native.KZG_E_ARG, "multiplicities: the input sets must hold exactly n_lookups * width rows")
        cells = lambda r: [r[j:j + 32] for j in range(0, len(r), 32)]   # noqa: E731
        mult, missing = multiplicities([cells(r) for r in f], [cells(r) for r in t], n_lookups, width)
        row = b"".join(m.to_bytes(32, "big") for m in mult)
        i, h = self.sets[hi[0]][0], next(_HANDLES)
        self.sets[h] = (i, [row])
        return RowSet(self, h, i, 1, len(mult), [hashlib.sha384(b"C" + row).digest()]), missing

    def release_rows(self, handle):
        if self.sets.pop(int(handle), None) is None:
            raise _native.KzgError(_native.KZG_E_ARG, "unknown or already released handle")


def fr(v):
    return be32_to_fr(v.to_bytes(32, "big"))


def client(engine, machines_scale=2):
    cl = Client(engine=engine)
    cl.machines_scale, cl._slice_of = machines_scale, None   # what start() leaves for a synthetic setup
    return cl


def test_python_signatures():
    assert list(inspect.signature(HipEngine.commit_multiplicities).parameters)[1:] == ["input_sets", "table_sets", "n_lookups", "width"]
    assert list(inspect.signature(MultiDeviceClient.worker_commit_multiplicities).parameters)[1:] == \
        ["input_handles", "table_handles", "n_lookups", "width"]


def test_client_json_shape_and_400s():
    eng = FakeEngine()
    cl = client(eng)
    tab = [[fr(10 + t) for t in range(8)], [fr(20 + t) for t in range(8)]]
    a = cl.worker_commit_rows(1, [tab[0][::-1], tab[1][::-1], tab[0], tab[1]]).json()["handle"]   # two lookups of width 2 ...
    b = cl.worker_commit_rows(1, [tab[0], [fr(99)] * 8]).json()["handle"]                         # ... and a third that misses
    t = cl.worker_commit_rows(1, tab).json()["handle"]
    r = cl.worker_commit_multiplicities(input_handles=[a, b], table_handles=[t], n_lookups=3, width=2)
    assert r.status_code == 200, r.json()
    assert set(r.json()) == {"commitment", "missing", "handle"}
    assert eng.calls[-1] == ("mult", (a, b), (t,), 3, 2)
    assert r.json()["missing"] == 8 and isinstance(r.json()["handle"], int)
    m = eng.sets[r.json()["handle"]][1][0]
    assert [int.from_bytes(m[j:j + 32], "big") for j in range(0, 256, 32)] == [2] * 8
    assert r.json()["commitment"] == g1_to_b64(hashlib.sha384(b"C" + m).digest())
    assert cl.worker_release_rows(r.json()["handle"]).status_code == 200       # the new set releases like the others
    ok = lambda *x: cl.worker_commit_multiplicities(*x).status_code   # noqa: E731
    assert ok([a], [t], 2, 2) == 200
    assert ok([a, b], [t], 2, 2) == 400                                        # six input rows for L w = 4
    assert ok([a, b], [t], 2, 3) == 400                                        # two table rows for w = 3
    n_calls = len(eng.calls)
    assert ok([a, b], [t], 0, 2) == 400                                        # L = 0
    assert ok([a, b], [t], 3, 0) == 400                                        # w = 0
    assert ok([a, b], [t], 9, 2) == 400                                        # L w = 18
    assert ok([a, b], [t], "three", 2) == 400                                  # not a number
    assert ok([], [t], 3, 2) == 400                                            # no input handle
    assert ok([a, b], [], 3, 2) == 400                                         # no table handle
    assert ok([a, b], ["x"], 3, 2) == 400                                      # not a handle
    assert ok([a] * 17, [t], 3, 2) == 400                                      # more than 16 handles
    assert len(eng.calls) == n_calls                                           # none of these reached the engine
    assert ok([a, b], [10 ** 9], 3, 2) == 400                                  # unknown handle
    other = cl.worker_commit_rows(0, tab).json()["handle"]
    assert ok([a, b], [other], 3, 2) == 400                                    # two workers
    assert Client(engine=None).worker_commit_multiplicities([a], [t], 2, 2).status_code == 503


def test_multi_device_client_routes_by_worker():
    engines = [FakeEngine(), FakeEngine(), FakeEngine()]
    multi = MultiDeviceClient(devices=[0, 1, 2], seed=5, engines=engines)
    assert multi.worker_commit_multiplicities([1], [1], 1, 1).status_code == 400   # no set is known yet
    multi.start(scale=7, machines_scale=2)
    try:
        made = {}
        for i in range(4):
            col = [fr(100 * i + t) for t in range(8)]
            a = multi.worker_commit_rows(i, [col, col[::-1]]).json()["handle"]
            t = multi.worker_commit_rows(i, [col]).json()["handle"]
            r = multi.worker_commit_multiplicities([a], [t], 2, 1)
            assert r.status_code == 200, r.json()
            assert engines[i % 3].calls[-1] == ("mult", (a,), (t,), 2, 1) and r.json()["missing"] == 0
            m = r.json()["handle"]
            # the new set is owned by the same worker: usable as a source, and released through the router
            assert multi.worker_commit_multiplicities([m], [m], 1, 1).status_code == 200
            made[i] = (a, t, m)
        (a0, t0, m0), (a1, t1, _) = made[0], made[1]
        assert multi.worker_commit_multiplicities([a0], [t1], 2, 1).status_code == 400   # two workers
        assert multi.worker_commit_multiplicities([10 ** 9], [t0], 2, 1).status_code == 400
        assert multi.worker_commit_multiplicities(["x"], [t0], 2, 1).status_code == 400
        assert multi.worker_commit_multiplicities(None, [t0], 2, 1).status_code == 400
        assert multi.worker_release_rows(m0).status_code == 200
        assert multi.worker_commit_multiplicities([m0], [t0], 1, 1).status_code == 400   # released
    finally:
        multi.stop()
