"""GPU tests (`-m gpu`) of kzg_rows_commit_typed and kzg_rows_read: integer columns of their natural width in, cells of resident
rows back out.  A typed commit is checked against commit_rows of the reference's 32-byte rows (tests/typed_ref.py) byte for
byte -- commitments, and evaluations and proofs of an opening at two points -- and a read against the integers that went in,
against the reference's overflow rule, and in coefficient form against tests/ntt_ref.py.  Row lengths 1 .. 2^12: the decode and
the narrowing are one lane per cell, with no path that depends on a larger size.  Each test leaves rows_stats() where it
found it."""
import ctypes
import random
import threading

import numpy as np
import pytest

from tests import ntt_ref
from tests import typed_ref as tr
from tests.gpu_common import R, be
from tests.gpu_rows import arg_error, b_terms, commit_sets, engine_cache, release
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x7E9ED001, 0x7E9ED002
ALL = ["fr", "u8", "u16", "u32", "u64", "i32", "i64"]
INTS = ALL[1:]
NP = {"u8": np.uint8, "u16": np.uint16, "u32": np.uint32, "u64": np.uint64, "i32": np.int32, "i64": np.int64}
KIND = _native.COL_DTYPES
E_ARG = _native.KZG_E_ARG
R_BE = R.to_bytes(32, "big")     # (gpu_common.be reduces mod r)


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


def lg_of(T):
    return max(1, (T - 1).bit_length())


def cells_of(kind, n, rnd):
    """n cells of a kind: its extreme values first (as many as fit), then random ones over its whole range"""
    if kind == "fr":
        head = [0, 1, R - 1, R - 2]
        return (head + [rnd.randrange(R) for _ in range(n)])[:n]
    lo, hi = tr.lo_hi(kind)
    return (tr.extremes(kind) + [rnd.randint(lo, hi) for _ in range(n)])[:n]


def buffer_of(kind, cells):
    return tr.pack("fr", cells) if kind == "fr" else np.array(cells, dtype=NP[kind])


def ref_rows(kinds, cols, T, fills):
    return [tr.be32_row(tr.residues(kd, c, T, f or 0)) for kd, c, f in zip(kinds, cols, fills)]


def commit_both(eng, kinds, cols, T, fills=None, ef=True, buffers=None, only=None):
    """the typed set and the set of the reference's be32 rows (only = 0 / 1: that one alone)"""
    fills = fills or [None] * len(kinds)
    bufs = buffers or [buffer_of(kd, c) for kd, c in zip(kinds, cols)]
    typed = lambda: eng.commit_rows_typed(0, [(b, None if f is None else be(f)) for b, f in zip(bufs, fills)], ef, T)   # noqa: E731
    ref = lambda: eng.commit_rows(0, ref_rows(kinds, cols, T, fills), ef)   # noqa: E731
    return (typed(), ref()) if only is None else (typed, ref)[only]()


def same_set(eng, typed, ref, rnd):
    """commitments, and the evaluations and proofs of an opening at two points: every row at the first, row 0 at the second"""
    assert (typed.k, typed.i, typed.T) == (ref.k, ref.i, ref.T)
    assert typed.commitments == ref.commitments
    pts, gam = [be(rnd.randrange(R)) for _ in range(2)], [be(rnd.randrange(1, R)) for _ in range(2)]
    opened = [list(range(typed.k)), [0]]
    assert eng.open_rows([typed], pts, opened, gam) == eng.open_rows([ref], pts, opened, gam)


def check(eng, kinds, cols, T, rnd, fills=None, ef=True, buffers=None):
    before = eng.rows_stats()
    # the accounting is commit_rows': each set alone, one after the other (the second finds the free list the first found)
    deltas = []
    for which in (0, 1):
        one = commit_both(eng, kinds, cols, T, fills, ef, buffers, only=which)
        live = eng.rows_stats()
        deltas.append((live[0] - before[0], live[1] - before[1]))
        one.release()
        assert eng.rows_stats() == before
    assert deltas[0] == deltas[1] and deltas[0][0] == 1 and deltas[0][1] >= len(kinds) * T * 32, deltas
    typed, ref = commit_both(eng, kinds, cols, T, fills, ef, buffers)
    try:
        live = eng.rows_stats()
        assert live[0] == before[0] + 2 and live[1] - before[1] >= 2 * typed.k * T * 32     # counted like the other set
        same_set(eng, typed, ref, rnd)
    finally:
        release([typed, ref])
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- commit
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("T", [1, 2, 4, 32, 1024, 4096])
def test_mixed_kinds_commit_to_the_bytes_of_their_be32_rows(engines, T, k):
    rnd = random.Random(1000 * T + k)
    kinds = [ALL[(j + T) % 7] for j in range(k)]
    check(engines(lg_of(T)), kinds, [cells_of(kd, T, rnd) for kd in kinds], T, rnd)


@pytest.mark.parametrize("kind", ALL)
def test_each_kind_alone(engines, kind):
    rnd = random.Random(900 + ALL.index(kind))
    for T, k in ((1, 1), (32, 3), (1024, 2)):
        check(engines(lg_of(T)), [kind] * k, [cells_of(kind, T, rnd) for _ in range(k)], T, rnd)


@pytest.mark.parametrize("fill", [None, R - 1, 12345])
def test_short_u8_and_u16_columns_dword_tails_and_odd_neighbours(engines, fill):
    """every count whose bytes end inside a dword, next to neighbours of odd length: the packing offsets and the fill"""
    T = 32
    eng, rnd = engines(5), random.Random(77)
    counts = [0, 1, 3, 5, 7, T - 1, T]
    for kind in ("u8", "u16"):
        kinds = [kind] * len(counts) + ["u8", "u32", "fr"]
        cols = [cells_of(kind, c, rnd) for c in counts] + [cells_of("u8", 3, rnd), cells_of("u32", 5, rnd), cells_of("fr", 9, rnd)]
        check(eng, kinds, cols, T, rnd, [fill] * len(kinds))
    # the same counts in reverse order: every column behind an odd-length one
    kinds = ["u8", "u16"] * 3 + ["u8"]
    check(eng, kinds, [cells_of(kd, c, rnd) for kd, c in zip(kinds, reversed(counts))], T, rnd, [fill] * 7)


def misaligned(kind, cells, off):
    """the cells in a buffer that starts `off` bytes behind a 16-byte boundary, as a slice of a larger array"""
    dt = np.dtype(NP[kind])
    raw = np.zeros(len(cells) * dt.itemsize + 64, dtype=np.uint8)
    start = (-raw.ctypes.data) % 16 + off
    view = raw[start:start + len(cells) * dt.itemsize].view(dt)
    view[:] = cells
    assert view.ctypes.data % 16 == off
    return view


def test_host_buffers_off_a_16_byte_boundary(engines):
    T = 64
    eng, rnd = engines(6), random.Random(78)
    kinds = ["u8", "u32", "u64", "u16"]
    cols = [cells_of(kd, n, rnd) for kd, n in zip(kinds, (T, T - 3, T, 9))]
    bufs = [misaligned(kd, c, off) for kd, c, off in zip(kinds, cols, (1, 4, 4, 2))]
    check(eng, kinds, cols, T, rnd, [None, 7, None, R - 1], buffers=bufs)


def test_coefficient_form_with_a_length_that_is_no_power_of_two(engines):
    T = 6
    eng, rnd = engines(3), random.Random(79)
    check(eng, ALL, [cells_of(kd, n, rnd) for kd, n in zip(ALL, (6, 6, 5, 6, 0, 6, 3))], T, rnd, [None, 1, R - 1, None, 5, None, 9],
          ef=False)
    arg_error(lambda: eng.commit_rows_typed(0, [np.zeros(6, dtype=np.uint8)], True), "power of two")


def test_extreme_values_of_every_kind(engines):
    eng, rnd = engines(3), random.Random(80)
    cols = [tr.extremes(kd) for kd in INTS]
    T = 8
    assert all(len(c) <= T for c in cols) and [-1 in c for c in cols] == [False] * 4 + [True] * 2
    check(eng, INTS, cols, T, rnd, [R - 1] * 6)
    typed = eng.commit_rows_typed(0, [np.array([-1, -2**63], dtype=np.int64), np.array([-2**31], dtype=np.int32)], True, 2)
    try:
        assert eng.read_rows([typed], 0, 0, 2, "fr")[0] == be(R - 1) + be(R - 2**63)
        assert eng.read_rows([typed], 1, 0, 2, "fr")[0] == be(R - 2**31) + be(0)
    finally:
        typed.release()


def raw_commit(eng, cols, k, T, ef=1, i=0):
    """the export itself, for shapes the Python layer refuses: (status, handle)"""
    arr = (_native.Col * max(len(cols), 1))()
    keep = []
    for c, (data, count, kind, fill) in enumerate(cols):
        keep.append(data)
        arr[c].data = None if data is None else ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p)
        arr[c].count, arr[c].kind, arr[c].fill_be32 = count, kind, fill
    c48, h = ctypes.create_string_buffer(48 * 17), ctypes.c_uint64(0)
    return eng._lib.kzg_rows_commit_typed(eng._h, i, k, arr, T, ef, c48, ctypes.byref(h)), h.value


def test_every_refusal_is_e_arg_and_leaves_nothing_behind(engines):
    T = 16
    eng = engines(4)
    before = eng.rows_stats()
    u8 = (bytes(T), T, KIND["u8"], None)
    assert raw_commit(eng, [u8], 0, T)[0] == E_ARG                                          # k = 0
    assert raw_commit(eng, [u8] * 17, 17, T)[0] == E_ARG                                    # k = 17
    assert raw_commit(eng, [(bytes(T), T, 7, None)], 1, T)[0] == E_ARG                      # an unknown kind
    assert raw_commit(eng, [(bytes(T + 1), T + 1, KIND["u8"], None)], 1, T)[0] == E_ARG     # count > T
    assert raw_commit(eng, [(None, 1, KIND["u8"], None)], 1, T)[0] == E_ARG                 # cells without data
    assert raw_commit(eng, [(bytes(T), 3, KIND["u8"], R_BE)], 1, T)[0] == E_ARG            # a fill >= r
    assert raw_commit(eng, [u8, (be(1) + R_BE, 2, KIND["fr"], None)], 2, T)[0] == E_ARG    # a be32 cell >= r
    assert raw_commit(eng, [u8], 1, 0)[0] == E_ARG                                          # the checks of kzg_rows_commit:
    assert raw_commit(eng, [u8], 1, 2 * T)[0] == E_ARG                                      # T = 0, T beyond the slice,
    assert raw_commit(eng, [(bytes(12), 12, KIND["u8"], None)], 1, 12, ef=1)[0] == E_ARG    # evaluation form, T = 12,
    assert raw_commit(eng, [u8], 1, T, i=1)[0] == E_ARG                                     # a worker that is not resident
    assert eng._lib.kzg_rows_commit_typed(eng._h, 0, 1, None, T, 1, ctypes.create_string_buffer(48), None) == E_ARG
    arg_error(lambda: eng.commit_rows_typed(0, [R_BE]), "canonical")
    arg_error(lambda: eng.commit_rows_typed(0, [(np.zeros(3, dtype=np.uint8), R_BE)], True, 4), "fill")
    assert eng.rows_stats() == before
    rc, h = raw_commit(eng, [(None, 0, KIND["i64"], None)], 1, T)                           # no cells: data may be null
    assert rc == 0 and eng.read_rows([h], 0, 0, T, "u8")[0] == bytes(T)
    eng.release_rows(h)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- read
@pytest.mark.parametrize("T", [1, 32, 4096])
def test_a_read_returns_what_was_committed(engines, T):
    eng, rnd = engines(lg_of(T)), random.Random(T + 5)
    before = eng.rows_stats()
    cols = [cells_of(kd, T, rnd) for kd in ALL]
    typed = eng.commit_rows_typed(0, [buffer_of(kd, c) for kd, c in zip(ALL, cols)])
    try:
        for row, kd in enumerate(ALL):
            res = tr.residues(kd, cols[row])
            assert eng.read_rows([typed], row, 0, T, kd) == (tr.pack(kd, cols[row]), 0, None), kd
            assert eng.read_rows([typed], row, 0, T, "fr") == (tr.be32_row(res), 0, None), kd
            coeffs = ntt_ref.ntt(res, inverse=True) if T > 1 else res
            assert eng.read_rows([typed], row, 0, T, "fr", False) == (tr.be32_row(coeffs), 0, None), kd
            for other in INTS:      # every row at every kind: the reference's overflow rule
                cells, n, first = tr.narrow(other, res)
                assert eng.read_rows([typed], row, 0, T, other) == (tr.pack(other, cells), n, first), (kd, other)
    finally:
        typed.release()
    assert eng.rows_stats() == before


def raw_read(eng, handles, row, first, count, kind, ef=1, room=64):
    hs = (ctypes.c_uint64 * len(handles))(*handles)
    out, ovf = ctypes.create_string_buffer(room), (ctypes.c_uint64 * 2)(5, 5)
    return eng._lib.kzg_rows_read(eng._h, len(handles), hs, row, first, count, kind, ef, out, ovf), out.raw, list(ovf)


def test_windows(engines):
    T = 32
    eng, rnd = engines(5), random.Random(81)
    col = cells_of("u16", T, rnd)
    typed = eng.commit_rows_typed(0, [np.array(col, dtype=np.uint16)])
    try:
        for first, count in ((0, T), (T - 1, 1), (5, 0), (3, 9), (T, 0)):
            assert eng.read_rows([typed], 0, first, count, "u16") == (tr.pack("u16", col[first:first + count]), 0, None)
        rc, raw, ovf = raw_read(eng, [typed.handle], 0, 5, 0, KIND["u16"])
        assert rc == 0 and raw == bytes(64) and ovf == [0, _native.KZG_READ_NONE]            # count = 0 touches nothing
        assert eng._lib.kzg_rows_read(eng._h, 1, (ctypes.c_uint64 * 1)(typed.handle), 0, 5, 0, KIND["u16"], 1, None,
                                      (ctypes.c_uint64 * 2)()) == 0                          # ... and needs no buffer
        for first, count in ((0, T + 1), (T, 1), (3, T - 2), ((1 << 64) - 1, 2), (T + 1, 0), (2, (1 << 64) - 1)):
            rc, raw, _ = raw_read(eng, [typed.handle], 0, first, count, KIND["u16"])
            assert rc == E_ARG and raw == bytes(64), (first, count)
        arg_error(lambda: eng.read_rows([typed], 0, 1, T, "u16"), "row length")
        assert raw_read(eng, [typed.handle], 1, 0, 1, KIND["u16"])[0] == E_ARG                # a row outside the set
        assert raw_read(eng, [typed.handle], 0, 0, 1, 7)[0] == E_ARG                          # an unknown kind
        assert raw_read(eng, [], 0, 0, 1, KIND["u8"])[0] == E_ARG
    finally:
        typed.release()
    six = eng.commit_rows_typed(0, [np.arange(6, dtype=np.uint8)], False)
    try:
        assert eng.read_rows([six], 0, 1, 4, "u8", False)[0] == bytes([1, 2, 3, 4])
        arg_error(lambda: eng.read_rows([six], 0, 0, 6, "u8", True), "power of two")
    finally:
        six.release()


def test_overflow_is_counted_and_reads_zero(engines):
    T = 1 << 12
    eng = engines(12)
    typed = eng.commit_rows_typed(0, [np.arange(T, dtype=np.uint16), tr.be32_row([R - 1, R - 2**31 - 1, R - 2**31, 2**31])], True, T)
    try:
        raw, n, first = eng.read_rows([typed], 0, 0, T, "u8")
        assert (n, first) == (T - 256, 256) and raw == bytes(range(256)) + bytes(T - 256)
        assert eng.read_rows([typed], 0, 300, 5, "u8") == (bytes(5), 5, 300)                  # the row index, not the offset
        assert eng.read_rows([typed], 1, 0, 1, "i32") == (tr.pack("i32", [-1]), 0, None)
        assert eng.read_rows([typed], 1, 1, 1, "i32") == (tr.pack("i32", [0]), 1, 1)
        assert eng.read_rows([typed], 1, 0, 5, "i32") == (tr.pack("i32", [-1, 0, -2**31, 0, 0]), 2, 1)
        assert eng.read_rows([typed], 1, 0, 4, "i64") == (tr.pack("i64", [-1, -2**31 - 1, -2**31, 2**31]), 0, None)
    finally:
        typed.release()


def test_a_read_observes_what_a_builder_wrote_and_addresses_a_concatenation(engines):
    T = 1 << 10
    eng, rnd = engines(10), random.Random(82)
    before = eng.rows_stats()
    col = np.array([rnd.randrange(1 << 32) for _ in range(T)], dtype=np.uint32)
    a = eng.commit_rows_typed(0, [col])
    b = eng.commit_rows_typed(0, [np.arange(T, dtype=np.uint16), np.full(T, -3, dtype=np.int32)])
    s = eng.commit_sorted([a], 1)
    try:
        assert eng.read_rows([s], 0, 0, T, "u32") == (np.sort(col).tobytes(), 0, None)
        assert eng.read_rows([a, b], 2, 0, 4, "i32") == (tr.pack("i32", [-3] * 4), 0, None)
        assert eng.read_rows([b, a, s], 2, 0, T, "u32")[0] == col.tobytes()
        assert eng.read_rows([b, a, s], 3, T - 1, 1, "u32")[0] == np.sort(col)[-1:].tobytes()
        assert eng.read_rows([b, b], 2, 7, 2, "u8")[0] == bytes([7, 8])
        arg_error(lambda: eng.read_rows([a, b], 3, 0, 1, "u8"), "row")
    finally:
        release([a, b, s])
    assert eng.rows_stats() == before


def test_handles_an_accumulator_a_released_set_and_reads_beside_opens(engines):
    T = 1 << 10
    eng, rnd = engines(10), random.Random(83)
    before = eng.rows_stats()
    col = np.array([rnd.randrange(1 << 64) for _ in range(T)], dtype=np.uint64)
    typed = eng.commit_rows_typed(0, [col, np.arange(T, dtype=np.uint8)])
    plain = commit_sets(eng, [[rnd.randrange(R) for _ in range(T)] for _ in range(3)], (3,))
    acc = eng.quotient_part(plain, b_terms([(1, [0, 1]), (R - 1, [2])]), None, None, None, None, 2, None, None)
    try:
        arg_error(lambda: eng.read_rows([acc], 0, 0, 1, "fr"), "accumulator")
        pts, gam, opened = [be(11), be(13)], [be(3), be(5)], [[0, 1], [1]]
        want_open, want = eng.open_rows([typed], pts, opened, gam), col.tobytes()
        got, errs = [], []

        def opens():
            try:
                for _ in range(4):
                    got.append(eng.open_rows([typed], pts, opened, gam))
            except Exception as e:   # noqa: BLE001
                errs.append(e)

        th = threading.Thread(target=opens)
        th.start()
        reads = [eng.read_rows([typed], 0, 0, T, "u64") for _ in range(6)]
        th.join()
        assert not errs and got == [want_open] * 4 and reads == [(want, 0, None)] * 6
        assert eng.open_rows([typed], pts, opened, gam) == want_open                       # the set is unchanged by reads
        ref = eng.commit_rows(0, [tr.be32_row([int(v) for v in col]), tr.be32_row([t % 256 for t in range(T)])])
        assert ref.commitments == typed.commitments
        ref.release()
    finally:
        acc.release()
        release(plain)
        typed.release()
    arg_error(lambda: eng.read_rows([typed.handle], 0, 0, 1, "u8"), "released")
    assert eng.rows_stats() == before


def test_a_stale_set_is_refused(hip):
    eng = hip()
    eng.gen_srs(SEED_X, SEED_Y, 4, 0)
    typed = eng.commit_rows_typed(0, [np.arange(16, dtype=np.uint8)])
    assert eng.read_rows([typed], 0, 0, 16, "u8")[0] == bytes(range(16))
    eng.gen_srs(SEED_X + 1, SEED_Y, 4, 0)
    arg_error(lambda: eng.read_rows([typed], 0, 0, 16, "u8"), "SRS")
    typed.release()
    assert eng.rows_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------------- through the layers
def test_the_text_client_and_the_multi_device_client(hip):
    from zkp_subnet_amd import Client, MultiDeviceClient, codec

    scale, ms = 7, 1
    T = 1 << (scale - ms)
    rnd = random.Random(84)
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731

    def through(client, i):
        wire, u16, i64 = cells_of("fr", T, rnd), cells_of("u16", T - 5, rnd), cells_of("i64", T, rnd)
        fill = 77
        r = client.worker_commit_rows_typed(i, [fr(wire), np.array(u16, dtype=np.uint16), np.array(i64, dtype=np.int64)],
                                            [None, fr([fill])[0], None])
        assert r.status_code == 200, r.json()
        rows = [tr.residues("fr", wire), tr.residues("u16", u16, T, fill), tr.residues("i64", i64)]
        ref = client.worker_commit_rows(i, [fr(v) for v in rows]).json()
        assert r.json()["commitments"] == ref["commitments"]
        h = r.json()["handle"]
        assert client.worker_read_rows([h], 2, 0, T, "i64").json() == {"cells": i64, "overflow": 0, "first_overflow": None}
        assert client.worker_read_rows([h], 1, 0, T, "u16").json()["cells"] == u16 + [fill] * 5
        assert client.worker_read_rows([h], 0, 2, 3).json()["cells"] == fr(wire[2:5])
        assert client.worker_read_rows([ref["handle"], h], 4, T - 6, 2, "u8").json() == {
            "cells": [u16[-1] if u16[-1] < 256 else 0, fill], "overflow": int(u16[-1] >= 256),
            "first_overflow": T - 6 if u16[-1] >= 256 else None}
        assert client.worker_read_rows([h], 3, 0, 1, "u8").status_code == 400
        assert client.worker_read_rows([h], 0, 0, T + 1, "u8").status_code == 400
        assert client.worker_commit_rows_typed(i, [np.zeros(T + 1, dtype=np.uint8)], None, T).status_code == 400
        for hh in (h, ref["handle"]):
            assert client.worker_release_rows(hh).status_code == 200
        assert client.worker_read_rows([h], 0, 0, 1, "u8").status_code == 400

    for client in (Client(seed=85), MultiDeviceClient(devices=[0], seed=85)):
        client.start(scale=scale, machines_scale=ms)
        try:
            for i in range(1 << ms):
                through(client, i)
        finally:
            client.stop()


def test_the_multi_context_twins_route_by_worker(hip):
    from zkp_subnet_amd.engine import lagrange_factor

    lib = _native.load()
    scale, ms = 6, 1
    T, tx, ty = 1 << (scale - ms), 0x7E9ED0AA, 0x7E9ED0BB
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(1, (ctypes.c_int * 1)(0), ctypes.byref(mh)) == 0
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(1 << ms))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        for i in range(1 << ms):
            col = np.arange(T, dtype=np.int32) - 7
            want = single.commit_rows_typed(i, [col])
            arr = (_native.Col * 1)()
            arr[0].data, arr[0].count, arr[0].kind = col.ctypes.data, T, KIND["i32"]
            c48, h = ctypes.create_string_buffer(48), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit_typed(mh, i, 1, arr, T, 1, c48, ctypes.byref(h)) == 0
            assert c48.raw == want.commitments[0]
            want.release()
            hs, out, ovf = (ctypes.c_uint64 * 1)(h.value), ctypes.create_string_buffer(4 * T), (ctypes.c_uint64 * 2)()
            assert lib.kzg_multi_rows_read(mh, i, 1, hs, 0, 0, T, KIND["i32"], 1, out, ovf) == 0
            assert out.raw == col.tobytes() and list(ovf) == [0, _native.KZG_READ_NONE]
            assert lib.kzg_multi_rows_read(mh, 1 - i, 1, hs, 0, 0, T, KIND["i32"], 1, out, ovf) == E_ARG    # another worker's set
            assert lib.kzg_multi_rows_release(mh, i, h.value) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)
