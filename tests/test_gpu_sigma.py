"""GPU tests (`-m gpu`) of kzg_rows_commit_sigma and kzg_rows_check_copies: the permutation's sigma columns built on the device
from variable labels, and the copy constraints of the same labels checked cell by cell.  The expected columns come from the
definition in Python integers (tests/sigma_ref.py: sort (label, flat index), link cyclically).  Every case compares the
commitments byte for byte with commit_rows of the reference sigma, every cell through read_rows, and the stats exactly.  Row
lengths 1 .. 2^12; the number of participating cells k * n is moved around the sort's tile through `usable`.  Each test leaves
rows_stats() where it found it."""
import array
import ctypes
import random
import threading

import pytest

from tests import sigma_ref as sref
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, commit_sets, engine_cache, release
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x51C3A001, 0x51C3A002
FREE = R - 1
TILE = 2048          # fr_sort_tile(): the positions of one workgroup of the sort's passes
LGS = [0, 1, 2, 4, 8, 12]


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


def shifts_of(k):
    return [pow(7, c, R) for c in range(k)]


def run(eng, labels, shifts=None, usable=None, free=None, sizes=None, sets=None):
    """commit `labels` (or take `sets`, which hold them), build sigma on the device and check the new set against commit_rows
    of the reference, cell for cell, and the stats; returns (the reference columns, the stats)"""
    k, T = len(labels), len(labels[0])
    shifts = shifts_of(k) if shifts is None else shifts
    want, stats = sref.sigma_columns(labels, shifts, usable, free)
    L = sets or commit_sets(eng, labels, sizes or (k,))
    ref = eng.commit_rows(0, [row_bytes(r) for r in want], True)
    try:
        cs, out, got = eng.commit_sigma(L, [be(s) for s in shifts], usable, None if free is None else be(free))
        try:
            assert (out.k, out.i, out.T) == (k, 0, T)
            assert cs == ref.commitments == out.commitments
            assert got == stats, (got, stats)
            for c in range(k):
                assert eng.read_rows([out], c, 0, T, "fr")[0] == row_bytes(want[c]), c
        finally:
            out.release()
    finally:
        release(([] if sets else L) + [ref])
    return want, stats


def id_labels(k, T, rnd, ids=None, free_share=0.0):
    ids = ids or max(1, k * T // 2)
    return [[FREE if rnd.random() < free_share else rnd.randrange(ids) for _ in range(T)] for _ in range(k)]


def witness(labels, rnd, usable=None, free=None):
    """wire values constant on the classes, random on the free cells and behind `usable`"""
    n = len(labels[0]) if usable is None else usable
    value = {}
    return [[rnd.randrange(R) if t >= n or lab == free else value.setdefault(lab, rnd.randrange(R))
             for t, lab in enumerate(col)] for col in labels]


# ---------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("lg", LGS)
@pytest.mark.parametrize("k", [1, 3, 8, 16])
def test_parity_with_the_reference(engines, lg, k):
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(100 * lg + k)
    labels = id_labels(k, T, rnd, free_share=0.1)
    _, stats = run(eng, labels, free=FREE, sizes=(k,) if k < 3 else (1, k - 1))
    if k * T >= 256:
        assert 0 < stats["classes"] < k * T and 0 < stats["fixed"] < k * T          # classes of several sizes and free cells
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- label shapes
@pytest.mark.parametrize("lg", LGS)
def test_all_labels_equal_is_one_cycle_and_all_distinct_is_the_identity(engines, lg):
    eng, T, k = engines(lg), 1 << lg, 3
    before = eng.rows_stats()
    # one label everywhere: no radix pass moves anything (the null permutation), one cycle of length k T
    for lab in (0, 77, R - 1):
        want, stats = run(eng, [[lab] * T for _ in range(k)])
        assert stats == {"classes": 1, "fixed": 0}
        img, _, _ = sref.images([[lab] * T for _ in range(k)])
        assert sref.cycles(img) == [tuple(range(k * T))]
    # all distinct: the identity
    rnd = random.Random(lg)
    labs = rnd.sample(range(1 << 60), k * T)
    want, stats = run(eng, [labs[c * T:(c + 1) * T] for c in range(k)])
    assert stats == {"classes": k * T, "fixed": k * T}
    assert want == sref.sigma_columns([[0] * T] * k, shifts_of(k), free_label=0)[0]
    assert eng.rows_stats() == before


@pytest.mark.parametrize("lg", [1, 2, 4, 8, 12])
def test_two_cell_classes_across_columns_reach_every_row_of_both_twiddle_halves(engines, lg):
    """class t is the cells (0, t) and (1, pi(t)): every cell is an image, so t' = 0, T/2 - 1, T/2 and T - 1 all occur, under
    the shifts 1, 7, 49 and 0"""
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(200 + lg)
    pi = list(range(T))
    rnd.shuffle(pi)
    col1 = [0] * T
    for t in range(T):
        col1[pi[t]] = t
    labels = [list(range(T)), col1, [T + t // 2 for t in range(T)], [2 * T + (t % 2) for t in range(T)]]
    for shifts in ([1, 7, 49, 0], [0, 49, 7, 1]):
        want, stats = run(eng, labels, shifts)
        assert stats == {"classes": T + T // 2 + 2, "fixed": 2 if T == 2 else 0}
    img, _, _ = sref.images(labels)
    assert {img[t] % T for t in range(T)} >= {0, T // 2 - 1, T // 2, T - 1} and all(img[t] // T == 1 for t in range(T))
    assert eng.rows_stats() == before


def test_labels_that_differ_in_one_word_or_byte_only_and_runs_at_both_ends_of_the_order(engines):
    lg, k = 8, 3
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(300)
    near = [5, 5 + (1 << 32), 5 + (1 << 64), 5 + (1 << 200), 5 + (1 << 248), 5 + (0x73 << 248), 0, 1, R - 1, R - 2, 1 << 32, 1 << 31]
    labels = [[rnd.choice(near) for _ in range(T)] for _ in range(k)]
    want, stats = run(eng, labels)
    assert stats == {"classes": len(near), "fixed": 0}
    # label 0 opens the sorted order and r - 1 closes it: a run that starts at position 0 and one that ends at the last,
    # as classes, as singletons and with r - 1 free
    labels = [[0, 0] + [10 + t for t in range(T - 4)] + [R - 1, R - 1], [0] + [5000 + t for t in range(T - 2)] + [R - 1]]
    for free in (None, FREE, 0):
        run(eng, labels, free=free)
    labels = [[0] + [10 + t for t in range(T - 2)] + [R - 1]]
    _, stats = run(eng, labels)
    assert stats == {"classes": T, "fixed": T}
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- sizes
def sizes_around_the_tile():
    """(k, n): k n one below, at and above a multiple of the tile where k divides such a number; for k = 8 and 16, whose k n
    moves in steps of k, one ROW below and above"""
    out = [(1, TILE - 1), (1, TILE), (1, TILE + 1), (3, 1365), (3, TILE), (3, 683)]        # 3 n = 4095, 6144, 2049
    for k in (8, 16):
        out += [(k, TILE // k - 1), (k, TILE // k), (k, TILE // k + 1), (k, 2 * TILE // k + 1)]
    return out


@pytest.mark.parametrize("k,n", sizes_around_the_tile())
def test_cell_counts_around_the_sort_s_tile(engines, k, n):
    lg = n.bit_length()                      # the smallest T > n
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(1000 * k + n)
    labels = id_labels(k, T, rnd, ids=k * n // 3, free_share=0.05)
    _, stats = run(eng, labels, usable=n, free=FREE)
    assert stats["classes"] > 0
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- free label and layout
@pytest.mark.parametrize("lg", [2, 4, 8, 12])
def test_free_label_set_absent_and_carried_by_every_cell(engines, lg):
    eng, T, k = engines(lg), 1 << lg, 3
    before = eng.rows_stats()
    rnd = random.Random(400 + lg)
    labels = id_labels(k, T, rnd, free_share=0.3)
    _, with_free = run(eng, labels, free=FREE)
    _, without = run(eng, labels)                                  # r - 1 is then a class like any other
    assert without["classes"] == with_free["classes"] + 1 and without["fixed"] < with_free["fixed"]
    _, absent = run(eng, labels, free=R - 2)                       # a free label that no cell carries
    assert absent == without
    _, stats = run(eng, [[FREE] * T for _ in range(k)], free=FREE)
    assert stats == {"classes": 0, "fixed": k * T}
    _, stats = run(eng, [[0] * T for _ in range(k)], free=0)       # the free label may be any field element
    assert stats == {"classes": 0, "fixed": k * T}
    assert eng.rows_stats() == before


@pytest.mark.parametrize("lg", [1, 2, 4, 8, 12])
def test_rows_behind_usable_map_to_themselves_whatever_their_labels(engines, lg):
    eng, T, k = engines(lg), 1 << lg, 3
    before = eng.rows_stats()
    rnd = random.Random(500 + lg)
    for usable in sorted({1, T - 1, max(1, T // 2 - 1)}):
        labels = id_labels(k, T, rnd, ids=max(2, usable), free_share=0.1)   # the rows behind hold labels of live classes
        want, stats = run(eng, labels, usable=usable, free=FREE)
        ident = sref.sigma_columns([[0] * T] * k, shifts_of(k), free_label=0)[0]
        assert all(want[c][usable:] == ident[c][usable:] for c in range(k))
        assert stats["fixed"] <= k * usable
        # the same cells with other labels behind `usable`: the same sigma
        other = [col[:usable] + [rnd.randrange(R) for _ in range(T - usable)] for col in labels]
        assert run(eng, other, usable=usable, free=FREE)[0] == want
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- handles and errors
def test_a_repeated_handle_is_two_equal_label_columns(engines):
    lg = 8
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(600)
    col, other = id_labels(1, T, rnd, ids=T // 3)[0], id_labels(1, T, rnd, ids=T // 3)[0]
    A, B = commit_sets(eng, [col, other], (1, 1))
    for usable in (None, T - 9):
        _, stats = run(eng, [col, other, col], usable=usable, sets=[A, B, A])
        assert stats["fixed"] == 0 or usable is not None
    wires = witness([col, other, col], rnd)
    W = commit_sets(eng, wires, (3,))
    assert eng.check_copies(W, [A, B, A]) == {"violations": 0, "first": None}
    assert eng.check_copies([A, B, A], [A, B, A]) == {"violations": 0, "first": None}     # a handle in both lists
    release([A, B] + W)
    assert eng.rows_stats() == before


def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg, k = 6, 3
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    rnd = random.Random(700)
    labels = id_labels(k, T, rnd, free_share=0.1)
    wires = witness(labels, rnd, free=FREE)
    sh = [be(s) for s in shifts_of(k)]
    want, want_stats = sref.sigma_columns(labels, shifts_of(k), None, FREE)
    ref = eng.commit_rows(0, [row_bytes(r) for r in want], True)
    want_c = ref.commitments
    ref.release()
    L, W = commit_sets(eng, labels, (1, 2)), commit_sets(eng, wires, (3,))

    def fresh_ok(L, W):
        cs, out, stats = eng.commit_sigma(L, sh, None, be(FREE))
        out.release()
        assert cs == want_c and stats == want_stats
        assert eng.check_copies(W, L, None, be(FREE)) == {"violations": 0, "first": None}

    fresh_ok(L, W)
    live = eng.rows_stats()
    lib = _native.load()
    hl = (ctypes.c_uint64 * 2)(L[0].handle, L[1].handle)
    hw = (ctypes.c_uint64 * 1)(W[0].handle)
    c, h, st, out2 = ctypes.create_string_buffer(48 * 16), ctypes.c_uint64(0), (ctypes.c_uint64 * 2)(), (ctypes.c_uint64 * 2)()
    big = R.to_bytes(32, "big")

    def raw(k_=k, shifts=b"".join(sh), opts=None, n=2):
        return lib.kzg_rows_commit_sigma(eng._h, n, hl, k_, shifts + bytes(32 * 16), ctypes.byref(opts) if opts else None, c, st,
                                         ctypes.byref(h))

    def raw_check(k_=k, opts=None, nw=1, nl=2):
        return lib.kzg_rows_check_copies(eng._h, nw, hw, nl, hl, k_, ctypes.byref(opts) if opts else None, out2)

    def refused(rc, why):
        assert rc == _native.KZG_E_ARG and why in lib.kzg_last_error(eng._h), (rc, lib.kzg_last_error(eng._h))
        assert eng.rows_stats() == live

    refused(raw(0), b"k must be in")
    refused(raw(17), b"k must be in")
    refused(raw(n=0), b"number of handles")
    refused(raw(n=17), b"number of handles")
    refused(raw(2), b"exactly k rows")                                   # 3 label rows, k = 2
    refused(raw(4), b"exactly k rows")
    refused(raw(shifts=sh[0] + big + sh[2]), b"shifts must be canonical")
    refused(raw(shifts=sh[0] + sh[1] + b"\xff" * 32), b"shifts must be canonical")
    for usable in (T, T + 1, 2 ** 40):
        refused(raw(opts=_native.SigmaOpts(usable, None)), b"usable must be in")
    refused(raw(opts=_native.SigmaOpts(0, big)), b"free label must be a canonical")
    refused(raw(opts=_native.SigmaOpts(3, b"\xff" * 32)), b"free label must be a canonical")
    refused(raw_check(0), b"k must be in")
    refused(raw_check(17), b"k must be in")
    refused(raw_check(nw=0), b"number of handles")
    refused(raw_check(nl=17), b"number of handles")
    refused(raw_check(2), b"exactly k rows")
    refused(raw_check(opts=_native.SigmaOpts(T, None)), b"usable must be in")
    refused(raw_check(opts=_native.SigmaOpts(0, big)), b"free label must be a canonical")
    arg_error(lambda: eng.check_copies(W, L[:1]), "exactly k rows")     # 3 wire rows against 1 label row
    arg_error(lambda: eng.commit_sigma(L * 6, sh + sh[:1] * 13), "KZG_MAX_BATCH_OPEN rows")      # 18 rows
    assert raw(opts=_native.SigmaOpts(0, None)) == 0                    # usable = 0 spelled out: the plain layout, no free label
    eng.release_rows(h.value)
    assert raw(opts=_native.SigmaOpts(T - 1, be(FREE))) == 0            # no bound on T - usable: usable = 1 is served as well
    eng.release_rows(h.value)
    assert raw(opts=_native.SigmaOpts(1, be(FREE))) == 0
    eng.release_rows(h.value)
    assert eng.rows_stats() == live
    # handles
    other = commit_sets(eng, labels[1:], (2,), i=1)                     # another worker
    arg_error(lambda: eng.commit_sigma([L[0]] + other, sh), "one worker")
    other_w = commit_sets(eng, wires, (3,), i=1)
    arg_error(lambda: eng.check_copies(other_w, L), "one worker")
    short = eng.commit_rows(0, [row_bytes(r[:T // 2]) for r in labels[1:]])       # another length
    arg_error(lambda: eng.commit_sigma([L[0], short], sh), "one worker and have one row length")
    arg_error(lambda: eng.check_copies([L[0], short], L), "one worker and have one row length")
    release(other + other_w + [short])
    gone = commit_sets(eng, labels[1:], (2,))
    release(gone)
    arg_error(lambda: eng.commit_sigma([L[0]] + gone, sh), "released")
    arg_error(lambda: eng.check_copies(W, [L[0]] + gone), "released")
    arg_error(lambda: eng.commit_sigma([2 ** 40], sh[:1]), "unknown")
    fresh_ok(L, W)
    # the 65th live set: the builder is refused, the check creates no set and is served
    fill = [eng.commit_rows(0, [row_bytes(labels[0])]) for _ in range(_native.KZG_MAX_ROW_SETS - 3)]
    assert eng.rows_stats()[0] == _native.KZG_MAX_ROW_SETS
    arg_error(lambda: eng.commit_sigma(L, sh), "KZG_MAX_ROW_SETS", code=_native.KZG_E_BUSY)
    assert eng.check_copies(W, L, None, be(FREE)) == {"violations": 0, "first": None}
    fill.pop().release()
    fresh_ok(L, W)
    release(fill)
    # stale after an SRS load
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.commit_sigma(L, sh), "SRS")
    arg_error(lambda: eng.check_copies(W, L), "SRS")
    release(L + W)
    L, W = commit_sets(eng, labels, (3,)), commit_sets(eng, wires, (3,))
    cs, out, _ = eng.commit_sigma(L, sh, None, be(FREE))
    ref = eng.commit_rows(0, [row_bytes(r) for r in want], True)
    assert cs == ref.commitments
    # the new set evaluates, goes stale and releases like any other
    assert eng.eval_rows([out], [be(3)], [[0, 1, 2]]) == eng.eval_rows([ref], [be(3)], [[0, 1, 2]])
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)
    arg_error(lambda: eng.eval_rows([out], [be(3)], [[0]]), "SRS")
    release(L + W + [out, ref])
    arg_error(lambda: eng.release_rows(out.handle))
    assert eng.rows_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------------- concurrency
def test_threads_and_a_racing_release(engines):
    lg = 10
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(800)
    jobs = [(id_labels(2, T, rnd), None), (id_labels(3, T, rnd, ids=40, free_share=0.2), T - 100)]
    sets = [commit_sets(eng, labels, (len(labels),)) for labels, _ in jobs]
    wsets = [commit_sets(eng, witness(labels, rnd, u, FREE), (len(labels),)) for labels, u in jobs]
    want = []
    for S, (labels, u) in zip(sets, jobs):
        cs, out, stats = eng.commit_sigma(S, [be(s) for s in shifts_of(len(labels))], u, be(FREE))
        out.release()
        want.append((cs, stats))
    errors = []

    def work(j):
        try:
            labels, u = jobs[j]
            for _ in range(4):
                cs, out, stats = eng.commit_sigma(sets[j], [be(s) for s in shifts_of(len(labels))], u, be(FREE))
                out.release()
                assert (cs, stats) == want[j]
                assert eng.check_copies(wsets[j], sets[j], u, be(FREE)) == {"violations": 0, "first": None}
        except Exception as ex:   # noqa: BLE001
            errors.append(repr(ex))

    ths = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for x in ths:
        x.start()
    for x in ths:
        x.join()
    assert not errors, errors
    # a release of a source set racing the call: the right bytes or KZG_E_ARG, never anything else
    labels, _ = jobs[0]
    sh3 = [be(1), be(7), be(49)]
    spare = commit_sets(eng, labels[1:], (1,))[0]
    want_cs, rs, _ = eng.commit_sigma([sets[0][0], spare], sh3)             # the columns l0, l1, l1
    release([rs, spare])
    for n in range(6):
        victim = commit_sets(eng, labels[1:], (1,))[0]
        out = []

        def call():
            try:
                if n < 3:
                    cs, rs, stats = eng.commit_sigma([sets[0][0], victim], sh3)
                    rs.release()
                    out.append(cs)
                else:
                    out.append(eng.check_copies([sets[0][0], victim], [sets[0][0], victim])["violations"])
            except KzgError as ex:
                out.append(ex.code)

        th = threading.Thread(target=call)
        th.start()
        victim.release()
        th.join()
        assert out[0] in (want_cs, 0, _native.KZG_E_ARG), out
    for S in sets + wsets:
        release(S)
    assert eng.rows_stats() == before


def test_multi_handle_and_the_text_clients_return_the_engine_bytes(hip):
    from zkp_subnet_amd import Client, MultiDeviceClient, codec
    from zkp_subnet_amd.engine import lagrange_factor

    lib = _native.load()
    scale, ms, k = 8, 1, 3
    T, M = 1 << (scale - ms), 1 << ms
    tx, ty = 0xABCDEF0BBB, 0x13579BFB
    rnd = random.Random(900)
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(1, (ctypes.c_int * 1)(0), ctypes.byref(mh)) == 0
    u = T - 5
    sh = b"".join(be(s) for s in shifts_of(k))
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    try:
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        c, cc = ctypes.create_string_buffer(48 * k), ctypes.create_string_buffer(48 * k)
        st, res = (ctypes.c_uint64 * 2)(), (ctypes.c_uint64 * 2)()
        made = {}
        for i in range(M):
            labels = id_labels(k, T, rnd, free_share=0.1)
            wires = witness(labels, rnd, u, FREE)
            wires[1][3] = (wires[1][3] + 1) % R
            L, W = commit_sets(single, labels, (k,), i=i), commit_sets(single, wires, (k,), i=i)
            cs, out, stats = single.commit_sigma(L, [sh[32 * j:32 * j + 32] for j in range(k)], u, be(FREE))
            viol = single.check_copies(W, L, u, be(FREE))
            release(L + W + [out])
            hl, hw, hz = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
            assert lib.kzg_multi_rows_commit(mh, i, k, b"".join(row_bytes(r) for r in labels), T, 1, cc, ctypes.byref(hl)) == 0
            assert lib.kzg_multi_rows_commit(mh, i, k, b"".join(row_bytes(r) for r in wires), T, 1, cc, ctypes.byref(hw)) == 0
            al, aw = (ctypes.c_uint64 * 1)(hl.value), (ctypes.c_uint64 * 1)(hw.value)
            opts = _native.SigmaOpts(u, be(FREE))
            assert lib.kzg_multi_rows_commit_sigma(mh, i, 1, al, k, sh, ctypes.byref(opts), c, st, ctypes.byref(hz)) == 0, i
            assert c.raw == b"".join(cs) and {"classes": st[0], "fixed": st[1]} == stats
            assert lib.kzg_multi_rows_check_copies(mh, i, 1, aw, 1, al, k, ctypes.byref(opts), res) == 0, i
            first = None if res[1] == (1 << 64) - 1 else (res[1] // T, res[1] % T)
            assert {"violations": res[0], "first": first} == viol == sref.copy_violations(wires, labels, u, FREE)
            made[i] = [hl.value, hw.value, hz.value]
        al = (ctypes.c_uint64 * 1)(made[1][0])                          # worker 1's set under index 0
        assert lib.kzg_multi_rows_commit_sigma(mh, 0, 1, al, k, sh, None, c, st, ctypes.byref(hz)) == _native.KZG_E_ARG
        assert lib.kzg_multi_rows_check_copies(mh, 0, 1, al, 1, al, k, None, res) == _native.KZG_E_ARG
        for i in range(M):
            for hh in made[i]:
                assert lib.kzg_multi_rows_release(mh, i, hh) == 0
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)

    # the text clients over the engine: the same bytes as a commit of the reference rows
    def through(client, workers):
        for i in workers:
            labels = id_labels(k, T, rnd, free_share=0.1)
            wires = witness(labels, rnd, None, FREE)
            wires[2][T - 1] = (wires[2][T - 1] + 1) % R
            a = client.worker_commit_rows(i, [fr(col) for col in labels]).json()["handle"]
            b = client.worker_commit_rows(i, [fr(col) for col in wires]).json()["handle"]
            for usable in (None, u):
                want, stats = sref.sigma_columns(labels, shifts_of(k), usable, FREE)
                ref = client.worker_commit_rows(i, [fr(col) for col in want]).json()
                r = client.worker_commit_sigma([a], fr(shifts_of(k)), usable, fr([FREE])[0])
                assert r.status_code == 200, r.json()
                assert r.json()["commitments"] == ref["commitments"]
                assert {"classes": r.json()["classes"], "fixed": r.json()["fixed"]} == stats
                v = client.worker_check_copies([b], [a], usable, fr([FREE])[0])
                assert v.status_code == 200, v.json()
                wantv = sref.copy_violations(wires, labels, usable, FREE)
                assert v.json() == {"violations": wantv["violations"], "first": None if wantv["first"] is None else list(wantv["first"])}
                for hh in (ref["handle"], r.json()["handle"]):
                    assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_sigma([a], fr([1, 7])).status_code == 400              # 3 rows, 2 shifts
            assert client.worker_commit_sigma([a], fr(shifts_of(k)), T).status_code == 400
            assert client.worker_check_copies([b], [a], T).status_code == 400
            assert client.worker_release_rows(b).status_code == 200
            assert client.worker_check_copies([b], [a]).status_code == 400
            assert client.worker_release_rows(a).status_code == 200
            assert client.worker_commit_sigma([a], fr(shifts_of(k))).status_code == 400

    single.close()
    for client in (Client(seed=84), MultiDeviceClient(devices=[0], seed=84)):
        client.start(scale=scale, machines_scale=ms)
        try:
            through(client, range(M))
        finally:
            client.stop()


# ---------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("usable", [None, (1 << 10) - 6])
def test_from_variable_ids_to_the_closed_grand_product(engines, usable):
    """labels as i32 variable ids (-1: free) through commit_rows_typed; wires the variables' values: the check reports 0 and the
    grand product over the device's sigma closes to 1; one altered cell is found by (column, row) and the product opens"""
    lg, k = 10, 3
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(1100)
    n = T if usable is None else usable
    n_vars = k * n // 3
    ids = [[-1 if rnd.random() < 0.1 else rnd.randrange(n_vars) for _ in range(T)] for _ in range(k)]
    values = [rnd.randrange(R) for _ in range(n_vars)]
    labels = [[v % R for v in col] for col in ids]
    wires = [[values[v] if v >= 0 and t < n else rnd.randrange(R) for t, v in enumerate(col)] for col in ids]
    L = [eng.commit_rows_typed(0, [array.array("i", col) for col in ids])]
    sh = [be(s) for s in shifts_of(k)]
    beta, gamma = be(rnd.randrange(R)), be(rnd.randrange(R))
    cs, S, stats = eng.commit_sigma(L, sh, usable, be(FREE))
    assert stats == sref.sigma_columns(labels, shifts_of(k), usable, FREE)[1]
    img, _, _ = sref.images(labels, usable, FREE)
    cyc = max(sref.cycles(img), key=len)
    m = len(cyc)
    assert m >= 3

    def outcome(rows):
        W = commit_sets(eng, rows, (k,))
        try:
            viol = eng.check_copies(W, L, usable, be(FREE))
            assert viol == sref.copy_violations(rows, labels, usable, FREE)
            # (under `usable` the rows behind are the identity on both sides: the product over all T rows closes as well)
            z, closing = eng.commit_grand_product(W, [S], sh, beta, gamma)
            z.release()
        finally:
            release(W)
        return viol, closing

    assert outcome(wires) == ({"violations": 0, "first": None}, be(1))
    # one non-head cell
    j = cyc[1]
    bent = [col[:] for col in wires]
    bent[j // T][j % T] = (bent[j // T][j % T] + 1) % R
    viol, closing = outcome(bent)
    assert viol == {"violations": 1, "first": (j // T, j % T)} and closing != be(1)
    # the head of a class of m cells: the other m - 1 differ from it, the second cell first
    j = cyc[0]
    bent = [col[:] for col in wires]
    bent[j // T][j % T] = (bent[j // T][j % T] + 1) % R
    viol, closing = outcome(bent)
    assert viol == {"violations": m - 1, "first": (cyc[1] // T, cyc[1] % T)} and closing != be(1)
    release(L + [S])
    assert eng.rows_stats() == before


def test_the_check_creates_no_set_and_runs_no_msm(engines):
    lg, k = 12, 3
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(1200)
    labels = id_labels(k, T, rnd, free_share=0.1)
    wires = witness(labels, rnd, None, FREE)
    wires[1][77] = (wires[1][77] + 1) % R
    want = sref.copy_violations(wires, labels, None, FREE)
    L, W = commit_sets(eng, labels, (k,)), commit_sets(eng, wires, (k,))
    live = eng.rows_stats()
    lib = _native.load()
    try:
        assert eng.check_copies(W, L, None, be(FREE)) == want
        assert lib.kzg_set_profiling(eng._h, 1) == 0
        try:
            assert eng.check_copies(W, L, None, be(FREE)) == want
            tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
            assert lib.kzg_get_timings(eng._h, tms, len(tms)) == 0
            t = dict(zip(_native.TIMING_NAMES, tms))
            cs, out, _ = eng.commit_sigma(L, [be(s) for s in shifts_of(k)], None, be(FREE))
            out.release()
            tms2 = (ctypes.c_float * len(_native.TIMING_NAMES))()
            assert lib.kzg_get_timings(eng._h, tms2, len(tms2)) == 0
            t2 = dict(zip(_native.TIMING_NAMES, tms2))
        finally:
            assert lib.kzg_set_profiling(eng._h, 0) == 0
        print("check_copies stage times (ms):", {n: round(v, 4) for n, v in t.items()})
        print("commit_sigma stage times (ms):", {n: round(v, 4) for n, v in t2.items()})
        assert eng.rows_stats() == live
        assert t["ntt"] > 0 and t["poly"] > 0 and t["decode"] == 0
        assert all(t[s] == 0 for s in ("digits", "scan", "scatter", "accumulate", "fixup", "tree", "final"))
        assert t2["ntt"] > 0 and t2["poly"] > 0 and t2["accumulate"] > 0 and t2["decode"] == 0     # no row-sized upload
    finally:
        release(L + W)
    assert eng.rows_stats() == before
