"""CPU-only tests of committed row sets (kzg_rows_* / kzg_multi_rows_*, HipEngine.commit_rows / open_rows, the text forms on
Client and MultiDeviceClient): the C-ABI's argument checks without a device, and the host logic -- JSON shapes, 400 on bad
input, routing of handles to the device of their worker -- over a fake engine with the library's set semantics."""
import ctypes
import hashlib
import itertools

import pytest

from zkp_subnet_amd import MultiDeviceClient, _native, codec
from zkp_subnet_amd.build import build
from zkp_subnet_amd.client import Client
from zkp_subnet_amd.codec import be32_to_fr, g1_to_b64
from zkp_subnet_amd.engine import RowSet

E_ARG = _native.KZG_E_ARG
_HANDLES = itertools.count(1)   # process-wide, as the library's


@pytest.fixture(scope="module")
def lib():
    build()
    return _native.load()


def test_c_abi_null_context_or_handles(lib):
    c48, ev, pf = ctypes.create_string_buffer(48 * 16), ctypes.create_string_buffer(32 * 64), ctypes.create_string_buffer(48 * 4)
    h = ctypes.c_uint64(0)
    rows, pts, gms = bytes(32 * 4), bytes(32), bytes(32)
    masks = (ctypes.c_uint32 * 1)(1)
    hs = (ctypes.c_uint64 * 1)(1)
    st = (ctypes.c_uint64 * 2)()
    assert lib.kzg_rows_commit(None, 0, 1, rows, 4, 1, c48, ctypes.byref(h)) == E_ARG
    assert lib.kzg_rows_open(None, 1, hs, 1, pts, masks, gms, ev, pf) == E_ARG
    assert lib.kzg_rows_open(None, 1, None, 1, pts, masks, gms, ev, pf) == E_ARG
    assert lib.kzg_rows_release(None, 1) == E_ARG
    assert lib.kzg_rows_stats(None, st) == E_ARG
    assert lib.kzg_multi_rows_commit(None, 0, 1, rows, 4, 1, c48, ctypes.byref(h)) == E_ARG
    assert lib.kzg_multi_rows_open(None, 0, 1, hs, 1, pts, masks, gms, ev, pf) == E_ARG
    assert lib.kzg_multi_rows_open(None, 0, 1, None, 1, pts, masks, gms, ev, pf) == E_ARG
    assert lib.kzg_multi_rows_release(None, 0, 1) == E_ARG
    assert h.value == 0


def test_header_limit_matches_python():
    import os
    import re

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kzg_mi355x.h")).read()
    assert int(re.search(r"#define KZG_MAX_ROW_SETS (\d+)", hdr).group(1)) == _native.KZG_MAX_ROW_SETS


class FakeEngine:
    """The set semantics of the library over stand-in arithmetic: a 'commitment' / 'evaluation' / 'proof' is a hash of
    what it depends on, so an open of sets equals commit_open_multi on the concatenated rows exactly when the host logic
    hands the right rows, points, masks and gammas through."""

    def __init__(self):
        self.sets = {}
        self.calls = []
        self.workers = None

    def gen_srs(self, tau_x, tau_y, scale, machines_scale, workers=None):
        self.workers = list(workers) if workers is not None else list(range(1 << machines_scale))

    @staticmethod
    def _c(i, row):
        return hashlib.sha384(b"C" + bytes([i]) + row).digest()

    @staticmethod
    def _y(row, a):
        return hashlib.sha256(b"Y" + a + row).digest()

    @staticmethod
    def _pi(i, rows, a, g):
        return hashlib.sha384(b"P" + bytes([i]) + a + g + b"".join(rows)).digest()

    def commit_rows(self, i, rows, evaluation_form=True):
        self.calls.append(("commit", i))
        h = next(_HANDLES)
        self.sets[h] = (i, list(rows))
        return RowSet(self, h, i, len(rows), len(rows[0]) // 32, [self._c(i, r) for r in rows])

    def commit_open_multi(self, i, rows, points, opened, gammas, evaluation_form=True):
        masks, _ = _native.open_masks(opened, len(rows))
        evals = [[self._y(rows[j], a) for j in js] for a, js in zip(points, opened)]
        proofs = [self._pi(i, [rows[j] for j in js], a, g) for a, js, g in zip(points, opened, gammas)]
        return [self._c(i, r) for r in rows], evals, proofs

    def open_rows(self, sets, points, opened, gammas):
        hs = [int(getattr(x, "handle", x)) for x in sets]
        self.calls.append(("open", tuple(hs)))
        if any(h not in self.sets for h in hs):
            raise _native.KzgError(E_ARG, "row-set opening: unknown or released handle")
        if len({(self.sets[h][0], len(self.sets[h][1][0])) for h in hs}) != 1:
            raise _native.KzgError(E_ARG, "row-set opening: all sets must belong to one worker and have one row length")
        i = self.sets[hs[0]][0]
        rows = [r for h in hs for r in self.sets[h][1]]
        if len(rows) > _native.KZG_MAX_BATCH_OPEN:
            raise _native.KzgError(E_ARG, "row-set opening: more than KZG_MAX_BATCH_OPEN rows in all")
        _, evals, proofs = self.commit_open_multi(i, rows, points, opened, gammas)
        return evals, proofs

    def release_rows(self, handle):
        self.calls.append(("release", handle))
        if self.sets.pop(int(handle), None) is None:
            raise _native.KzgError(E_ARG, "row-set release: unknown or already released handle")


def fr(v):
    return be32_to_fr(v.to_bytes(32, "big"))


def polys(k, T, seed):
    return [[fr(seed * 1000 + j * 100 + t) for t in range(T)] for j in range(k)]


def client(engine, machines_scale=2):
    cl = Client(engine=engine)
    cl.machines_scale, cl._slice_of = machines_scale, None   # what start() leaves for a synthetic setup
    return cl


def test_client_json_shapes_and_parity_with_commit_open_multi():
    eng = FakeEngine()
    cl = client(eng)
    wires, acc = polys(3, 8, 1), polys(1, 8, 2)
    a = cl.worker_commit_rows(1, wires)
    b = cl.worker_commit_rows(1, acc)
    assert a.status_code == 200 and b.status_code == 200, (a.json(), b.json())
    assert set(a.json()) == {"handle", "commitments"} and isinstance(a.json()["handle"], int)
    assert len(a.json()["commitments"]) == 3 and all(isinstance(c, str) for c in a.json()["commitments"])
    X, G = [fr(11), fr(12)], [fr(21), fr(22)]
    opened = [[0, 1, 2, 3], [3]]
    r = cl.worker_open_rows([a.json()["handle"], b.json()["handle"]], X, opened, G)
    assert r.status_code == 200, r.json()
    assert set(r.json()) == {"evals", "proofs"}
    assert [len(e) for e in r.json()["evals"]] == [4, 1] and len(r.json()["proofs"]) == 2
    ref = cl.worker_commit_open_multi(1, wires + acc, X, opened, G).json()
    assert r.json() == {"evals": ref["evals"], "proofs": ref["proofs"]}
    assert a.json()["commitments"] + b.json()["commitments"] == ref["commitments"]
    # a handle listed twice: its rows twice
    r2 = cl.worker_open_rows([b.json()["handle"], b.json()["handle"]], X[:1], [[0, 1]], G[:1])
    assert r2.json() == {k: v for k, v in cl.worker_commit_open_multi(1, acc + acc, X[:1], [[0, 1]], G[:1]).json().items()
                         if k != "commitments"}


def test_client_bad_input_is_400():
    eng = FakeEngine()
    cl = client(eng)
    h = cl.worker_commit_rows(0, polys(2, 4, 3)).json()["handle"]
    X, G = [fr(5)], [fr(6)]
    assert cl.worker_open_rows([h], X, [[1, 0]], G).status_code == 400          # rows not increasing
    assert cl.worker_open_rows([h], X, [[]], G).status_code == 400              # a point opening nothing
    assert cl.worker_open_rows([h], X, [[0, 2]], G).status_code == 400          # row 2 of a 2-row set
    assert cl.worker_open_rows([h], X * 5, [[0]] * 5, G * 5).status_code == 400   # m = 5
    assert cl.worker_open_rows([h], X, [[0], [1]], G).status_code == 400        # ragged points / opened
    assert cl.worker_open_rows([], X, [[0]], G).status_code == 400              # no handle
    assert cl.worker_open_rows(["x"], X, [[0]], G).status_code == 400           # not a handle
    assert cl.worker_open_rows([h] * 17, X, [[0]], G).status_code == 400        # more than 16 sets
    assert cl.worker_commit_rows(0, []).status_code == 400
    assert cl.worker_commit_rows(0, polys(17, 2, 4)).status_code == 400
    assert cl.worker_commit_rows(0, [polys(1, 4, 5)[0], polys(1, 3, 6)[0]]).status_code == 400
    assert cl.worker_commit_rows(9, polys(1, 4, 7)).status_code == 400          # worker outside 2^machines_scale
    other = cl.worker_commit_rows(1, polys(1, 4, 8)).json()["handle"]
    assert cl.worker_open_rows([h, other], X, [[0]], G).status_code == 400      # two workers in one open
    assert cl.worker_open_rows([h], X, [[0, 1]], G).status_code == 200


def test_release_and_context_manager():
    eng = FakeEngine()
    cl = client(eng)
    h = cl.worker_commit_rows(2, polys(2, 4, 9)).json()["handle"]
    X, G = [fr(5)], [fr(6)]
    assert cl.worker_open_rows([h], X, [[0, 1]], G).status_code == 200
    r = cl.worker_release_rows(h)
    assert r.status_code == 200 and r.json() == {"released": True}
    assert cl.worker_release_rows(h).status_code == 400                        # double release
    assert cl.worker_open_rows([h], X, [[0, 1]], G).status_code == 400         # open after release
    assert cl.worker_release_rows("nope").status_code == 400
    with eng.commit_rows(0, [bytes(64)]) as rs:
        assert rs.handle in eng.sets and rs.k == 1 and rs.T == 2
    assert rs.handle not in eng.sets and rs.released
    rs.release()                                                               # idempotent on the Python side
    assert Client(engine=None).worker_commit_rows(0, polys(1, 4, 1)).status_code == 503


def test_multi_device_client_routes_handles_to_their_workers_device():
    engines = [FakeEngine(), FakeEngine(), FakeEngine()]
    multi = MultiDeviceClient(devices=[0, 1, 2], seed=5, engines=engines)
    assert multi.worker_commit_rows(0, polys(1, 4, 1)).status_code == 503      # not started yet
    multi.start(scale=7, machines_scale=2)
    try:
        assert [e.workers for e in engines] == [[0, 3], [1], [2]]
        X, G = [fr(31), fr(32)], [fr(41), fr(42)]
        for i in range(4):
            ps = polys(3, 8, 20 + i)
            a, b = multi.worker_commit_rows(i, ps[:2]), multi.worker_commit_rows(i, ps[2:])
            assert a.status_code == 200 and b.status_code == 200
            g = i % 3
            local = engines[g].workers.index(i)                                 # the device's resident slice of worker i
            assert engines[g].calls[-2:] == [("commit", local), ("commit", local)]
            hs = [a.json()["handle"], b.json()["handle"]]
            r = multi.worker_open_rows(hs, X, [[0, 1, 2], [2]], G)
            assert r.status_code == 200, r.json()
            assert engines[g].calls[-1] == ("open", tuple(hs))
            ref = engines[g].commit_open_multi(local, [codec.fr_list_to_be32(p) for p in ps],
                                               [codec.fr_to_be32(x) for x in X], [[0, 1, 2], [2]],
                                               [codec.fr_to_be32(x) for x in G])
            assert r.json()["proofs"] == [g1_to_b64(p) for p in ref[2]]
            assert multi.worker_release_rows(hs[1]).status_code == 200
            assert engines[g].calls[-1] == ("release", hs[1])
            assert multi.worker_release_rows(hs[1]).status_code == 400
            assert multi.worker_open_rows(hs, X, [[0, 1, 2], [2]], G).status_code == 400
            assert multi.worker_open_rows(hs[:1], X[:1], [[0, 1]], G[:1]).status_code == 200
        h0 = multi.worker_commit_rows(0, polys(1, 8, 50)).json()["handle"]
        h1 = multi.worker_commit_rows(1, polys(1, 8, 51)).json()["handle"]
        assert multi.worker_open_rows([h0, h1], X[:1], [[0, 1]], G[:1]).status_code == 400   # two workers
        assert multi.worker_open_rows([10 ** 9], X[:1], [[0]], G[:1]).status_code == 400    # unknown handle
        assert multi.worker_release_rows(10 ** 9).status_code == 400
        assert multi.worker_open_rows([h0], X[:1], [[1]], G[:1]).status_code == 400          # bad opened
    finally:
        multi.stop()
