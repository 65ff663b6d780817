"""CPU tests of the sorted columns' host side.  They pin the reference tests/sorted_ref.py against the definition (a
permutation, ordered, stable, the tail in place), drive HipEngine.commit_sorted over a stub library (a bad argument is refused
under the method's name before any native call, a good one reaches kzg_rows_commit_sorted with the export's argument count) and
the Client's and the MultiDeviceClient's parsers over stub engines."""
import ctypes
import random

import pytest

from tests import sorted_ref as sref
from tests.gpu_common import R, be
from zkp_subnet_amd import MultiDeviceClient, _native, codec
from zkp_subnet_amd.client import Client
from zkp_subnet_amd.engine import HipEngine, RowSet

T = 16
S = bytes(31) + b"\x01"
FR = lambda v: codec.be32_to_fr(v.to_bytes(32, "big"))   # noqa: E731


# ---------------------------------------------------------------------------------------------------- the reference
def _columns(w, seed, small):
    rnd = random.Random(seed)
    return [[rnd.randrange(4 if small else R) for _ in range(T)] for _ in range(w)]


@pytest.mark.parametrize("w,n_keys,small", [(1, 1, False), (1, 1, True), (3, 3, False), (3, 2, True), (3, 1, True), (16, 16, True)])
def test_reference_is_an_ordered_stable_permutation(w, n_keys, small):
    cols = _columns(w, 10 * w + n_keys, small)
    out, perm = sref.sorted_columns(cols, n_keys)
    assert sorted(perm) == list(range(T))
    tup = lambda cs, t: tuple(cs[c][t] for c in range(w))   # noqa: E731
    assert [tup(out, t) for t in range(T)] == [tup(cols, perm[t]) for t in range(T)]          # whole rows travel
    keys = [tuple(out[c][t] for c in range(n_keys)) for t in range(T)]
    assert all(keys[t] <= keys[t + 1] for t in range(T - 1))                                   # ordered on the keys
    assert all(perm[t] < perm[t + 1] for t in range(T - 1) if keys[t] == keys[t + 1])          # ties keep the source order
    assert sorted(tup(out, t) for t in range(T)) == sorted(tup(cols, t) for t in range(T))     # the same multiset
    if small and n_keys < w:
        assert any(keys[t] == keys[t + 1] for t in range(T - 1))                               # (the ties were there)


def test_reference_orders_integers_and_column_zero_first():
    big, top = (1 << 224) + 5, R - 1
    out, perm = sref.sorted_columns([[top, 1 << 32, big, 0, (1 << 32) - 1, 1]])
    assert out == [[0, 1, (1 << 32) - 1, 1 << 32, big, top]] and perm == [3, 5, 4, 1, 2, 0]
    out, _ = sref.sorted_columns([[2, 1, 2, 1], [0, 9, 1, 3]], 2)
    assert out == [[1, 1, 2, 2], [3, 9, 0, 1]]                                                 # column 1 decides among equal column 0
    out, _ = sref.sorted_columns([[2, 1, 2, 1], [0, 9, 1, 3]], 1)
    assert out == [[1, 1, 2, 2], [9, 3, 0, 1]]                                                 # a payload keeps the source order


@pytest.mark.parametrize("u", [1, 2, T - 3, T - 1])
def test_reference_usable_layout(u):
    rnd = random.Random(u)
    cols = _columns(2, 30 + u, True)
    for col in cols:
        col[u:] = [0] * (T - u)                               # zeros behind `usable` would sort first if they were read
    cols[0][:u] = [1 + v for v in cols[0][:u]]
    tail = [rnd.randrange(R) for _ in range(2 * (T - u))]
    out, perm = sref.sorted_columns(cols, 1, u, tail)
    assert sorted(perm) == list(range(u))
    assert [len(c) for c in out] == [T, T]
    assert out[0][u:] == tail[:T - u] and out[1][u:] == tail[T - u:]
    assert out[0][:u] == sorted(cols[0][:u]) and 0 not in out[0][:u]
    other = [c[:u] + [rnd.randrange(R) for _ in range(T - u)] for c in cols]
    assert sref.sorted_columns(other, 1, u, tail) == (out, perm)                               # the rows behind are not read


# ---------------------------------------------------------------------------------------------------- the engine's checks
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return _native.KZG_OK
        return fn


@pytest.fixture
def eng():
    e = HipEngine.__new__(HipEngine)
    e._lib, e._h, e._set_len, e.verifier = _Recorder(), ctypes.c_void_p(1), {}, None
    return e


def _sets(e, n):
    return [RowSet(e, 1 + j, 3, 1, T, [bytes(48)]) for j in range(n)]


def test_engine_reaches_the_export_of_its_own_name(eng):
    out = eng.commit_sorted(_sets(eng, 3), 3)
    (name, args), = eng._lib.calls
    assert name == "kzg_rows_commit_sorted" and len(args) == len(_native.SYMBOLS[name][1])
    assert args[1] == 3 and list(args[2]) == [1, 2, 3] and (args[3], args[4], args[5]) == (3, 3, None)    # n_keys = None: width
    assert (out.k, out.i, out.T, len(out.commitments)) == (3, 3, T, 3)
    bare = eng.commit_sorted([100, 101], 2, 1)                                                            # bare handles, plain layout
    assert (bare.k, bare.i, bare.T) == (2, None, None) and eng._lib.calls[1][1][3:5] == (2, 1)
    eng.commit_sorted(_sets(eng, 2), 2, 1, T - 2, [S] * 4)
    opts = ctypes.cast(eng._lib.calls[2][1][5], ctypes.POINTER(_native.SortedOpts)).contents
    tail_at = ctypes.c_void_p.from_address(ctypes.addressof(opts) + _native.SortedOpts.tail_be32.offset).value
    assert opts.usable == T - 2 and ctypes.string_at(tail_at, 128) == S * 4
    assert ctypes.sizeof(_native.SortedOpts) == 16


@pytest.mark.parametrize("args,why", [
    (lambda s: ([], 1), "sets"),
    (lambda s: (s(2), 0), "width must be in"),
    (lambda s: (s(2), 17), "width must be in"),
    (lambda s: (s(2), 2, 0), "n_keys must be in"),
    (lambda s: (s(2), 2, 3), "n_keys must be in"),
    (lambda s: (s(2), 2, 1, None, [S]), "tail needs usable"),
    (lambda s: (s(2), 2, 1, 0, [S]), "usable must be in"),
    (lambda s: (s(2), 2, 1, -3), "usable must be in"),
    (lambda s: (s(2), 2, 1, T - 2, [S] * 3), "exactly width * (T - usable) = 4"),
    (lambda s: (s(2), 2, 1, T - 2, [S, S, S, b"\x01"]), "32 bytes"),
    (lambda s: ([100, 101], 2, 1, T - 2, [S] * 4), "row length of the sets is unknown"),
])
def test_engine_refuses_bad_arguments_before_any_native_call(eng, args, why):
    with pytest.raises(_native.KzgError) as err:
        eng.commit_sorted(*args(lambda n: _sets(eng, n)))
    assert err.value.code == _native.KZG_E_ARG and why in str(err.value), str(err.value)
    assert "commit_sorted: " in str(err.value)
    assert eng._lib.calls == []


# ---------------------------------------------------------------------------------------------------- the Client's parser
class _StubSet:
    handle, commitments = 77, [bytes(48), bytes(48)]


class _StubEngine:
    def __init__(self):
        self.calls = []

    def commit_sorted(self, *args):
        self.calls.append(args)
        return _StubSet()

    def commit_rows(self, i, rows, ef):
        self.calls.append(("rows", i, len(rows)))
        return _StubSet()

    def gen_srs(self, *a, **kw):
        pass

    def set_verifier_key(self, *a, **kw):
        pass

    def close(self):
        pass


def test_client_method_surface():
    import inspect

    sig = inspect.signature(MultiDeviceClient.worker_commit_sorted)
    assert list(sig.parameters) == ["self", "input_handles", "width", "n_keys", "usable", "tail"]
    assert [sig.parameters[p].default for p in ("n_keys", "usable", "tail")] == [None, None, ()]
    e = _StubEngine()                                         # (Client's methods are wrapped: the same names by keyword)
    r = Client(engine=e).worker_commit_sorted(input_handles=[4], width=2, n_keys=None, usable=None, tail=())
    assert r.status_code == 200 and e.calls == [([4], 2, 2, None, [])]
    assert Client().worker_commit_sorted([4], 2).status_code == 503                                  # not started


def test_client_passes_a_good_call_on_in_the_engines_order():
    e = _StubEngine()
    c = Client(engine=e)
    r = c.worker_commit_sorted([1, 2], 2)
    assert r.status_code == 200 and r.json() == {"handle": 77, "commitments": [codec.g1_to_b64(bytes(48))] * 2}
    assert e.calls == [([1, 2], 2, 2, None, [])]                                                # n_keys = None means width
    r = c.worker_commit_sorted([1], 3, n_keys=2, usable=12, tail=[FR(8), FR(9)])
    assert r.status_code == 200 and e.calls[1] == ([1], 3, 2, 12, [be(8), be(9)])


@pytest.mark.parametrize("kw,why", [
    (dict(input_handles=[]), "handles"),
    (dict(input_handles=list(range(17))), "handles"),
    (dict(width=0), "width must be in"),
    (dict(width=17), "width must be in"),
    (dict(width="x"), "integers"),
    (dict(n_keys=0), "n_keys in [1, width]"),
    (dict(n_keys=3), "n_keys in [1, width]"),
    (dict(tail=[FR(1)]), "tail needs usable"),
    (dict(usable=0, tail=[FR(1)]), "usable must be in"),
    (dict(usable=-1), "negative"),
    (dict(usable="u"), "integer"),
    (dict(usable=12, tail=[FR(R)]), "canonical"),
    (dict(usable=12, tail=["!!"]), "base64"),
])
def test_client_refuses_bad_arguments_before_any_device_call(kw, why):
    e = _StubEngine()
    args = dict(input_handles=[1, 2], width=2)
    args.update(kw)
    r = Client(engine=e).worker_commit_sorted(**args)
    assert r.status_code == 400 and why in r.json()["error"], r.json()
    assert r.json()["error"].startswith("worker_commit_sorted") or "handles" in why or "base64" in why
    assert e.calls == []


def test_multi_device_client_routes_by_worker():
    engines = [_StubEngine(), _StubEngine()]
    multi = MultiDeviceClient(devices=[0, 1], seed=5, engines=engines)
    assert multi.worker_commit_sorted([1], 1).status_code == 400                                # no set is known yet
    multi.start(scale=7, machines_scale=2)
    try:
        fr = [FR(v) for v in range(8)]
        for i in range(4):
            _StubSet.handle = 200 + 2 * i
            a = multi.worker_commit_rows(i, [fr, fr]).json()["handle"]
            _StubSet.handle = 201 + 2 * i
            r = multi.worker_commit_sorted([a], 2, 1)
            assert r.status_code == 200, r.json()
            assert engines[i % 2].calls[-1] == ([a], 2, 1, None, [])
            assert multi.worker_commit_sorted([r.json()["handle"]], 2).status_code == 200       # the new set is owned like its source
        assert multi.worker_commit_sorted([200, 202], 2).status_code == 400                     # two workers
    finally:
        _StubSet.handle = 77
        multi.stop()
