"""CPU checks of tests/join_ref.py, the model of the hash join of csrc/fr_join.hip: the hash port against a byte-oriented
MurmurHash3 written from its published definition, the occupied-slot model against a literal insertion, every input family at
every shape that runs on the GPU against the facts it claims (tests/test_gpu_join.py relies on them: a family that stops
meeting its facts fails here, before any GPU call), the Python references of the builders against the families' own counts,
and kzg_test_join's argument check, which runs before the context is looked at."""
import ctypes
import random

import pytest

from oracle.bls12_381 import R
from tests import fetch_ref as fref
from tests import join_ref as jr
from tests import lookup_sel_ref as sref
from tests.multiplicities_ref import multiplicities
from tests.poly_ref import MONT
from zkp_subnet_amd import _native
from zkp_subnet_amd.build import build

ALL_SHAPES = tuple(dict.fromkeys(jr.HOOK_SHAPES + jr.E2E_SHAPES))


# ---------------------------------------------------------------------------------------------------- the hash
def murmur3_32(data, seed):
    """MurmurHash3_x86_32 over bytes, from the published definition (blocks, tail, length, finaliser), in Python integers"""
    M = 0xFFFFFFFF
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & M   # noqa: E731
    h = seed
    nblocks = len(data) // 4
    for i in range(nblocks):
        k = int.from_bytes(data[4 * i:4 * i + 4], "little")
        k = rotl(k * 0xCC9E2D51 & M, 15) * 0x1B873593 & M
        h = (rotl(h ^ k, 13) * 5 + 0xE6546B64) & M
    tail = data[4 * nblocks:]
    if tail:
        k = int.from_bytes(tail, "little")
        h ^= rotl(k * 0xCC9E2D51 & M, 15) * 0x1B873593 & M
    h ^= len(data)
    h ^= h >> 16
    h = h * 0x85EBCA6B & M
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M
    return h ^ (h >> 16)


def test_the_byte_oriented_murmur3_meets_the_published_vectors():
    assert murmur3_32(b"", 0) == 0 and murmur3_32(b"", 1) == 0x514E28B7 and murmur3_32(b"", 0xFFFFFFFF) == 0x81F16F39
    assert murmur3_32(b"test", 0) == 0xBA6BD213 and murmur3_32(b"abc", 0) == 0xB3DD93FA
    assert murmur3_32(b"Hello, world!", 0x9747B28C) == 0x24884CBA
    assert murmur3_32(b"The quick brown fox jumps over the lazy dog", 0x9747B28C) == 0x2FA826CD


def test_hash_port_equals_the_byte_oriented_murmur3():
    rnd = random.Random(1)
    edge = [0, 1, 2, R - 1, R - 2, (1 << 200), (1 << 32) - 1, 1 << 32, MONT, pow(MONT, -1, R)]
    for w in (1, 2, 3, 4):
        tuples = [tuple(rnd.choice(edge) for _ in range(w)) for _ in range(40)]
        tuples += [tuple(rnd.randrange(R) for _ in range(w)) for _ in range(40)] + [jr.candidate(v, w) for v in range(1, 21)]
        if w == 3:
            tuples += [jr.candidate(v, 3, True) for v in range(1, 21)]
        got = jr.join_hash([list(c) for c in zip(*tuples)])
        for tup, h in zip(tuples, got):
            data = b"".join((v * MONT % R).to_bytes(32, "little") for v in tup)
            assert len(data) == 32 * w and int(h) == murmur3_32(data, jr.SEED), tup
        for cap in (1, 32, 2048):
            assert jr.homes_of(tuples, cap) == [int(h) & (cap - 1) for h in got]
    assert [int(x) for x in jr.words([1])[0]] == [MONT >> (32 * j) & 0xFFFFFFFF for j in range(8)]
    assert not jr.words([0, R]).any()


def test_key_search_returns_distinct_keys_with_the_home_asked_for():
    for w, last in ((1, False), (3, False), (3, True)):
        keys = jr.keys_at(63, 64, 12, w, last)
        assert len(set(keys)) == 12 and set(jr.homes_of(list(keys), 64)) == {63}
        assert jr.keys_at(63, 64, 5, w, last) == keys[:5]                      # consecutive candidates: a prefix
        if last:
            assert {k[:2] for k in keys} == {jr.LAST_FIXED}
    with pytest.raises(AssertionError):
        jr.keys_at(5, 4, 1)


# ---------------------------------------------------------------------------------------------------- the table model
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=jr.shape_id)
def test_occupied_equals_a_literal_insertion_in_twenty_orders(shape):
    f = jr.family(*shape)
    tuples = f.tuples()
    distinct = list(dict.fromkeys(tuples))
    occ = jr.occupied(jr.homes_of(distinct, f.cap), f.cap)
    assert occ == f.chain
    for seed in range(20):
        order = list(range(f.rows))
        random.Random(seed).shuffle(order)
        slots = jr.simulate_build(tuples, f.cap, order)
        assert {s for s, q in enumerate(slots) if q != jr.EMPTY} == occ
        where = jr.check_slots(slots, tuples, f.cap)
        assert set(where.values()) == occ
    # the checker itself bites: a slot that keeps a later row, a tuple in two slots, a hole in front of a tuple
    slots = jr.simulate_build(tuples, f.cap, range(f.rows))
    s = next(s for s, q in enumerate(slots) if q != jr.EMPTY and tuples.count(tuples[q]) > 1) if len(distinct) < f.rows else None
    if s is not None:
        bad = list(slots)
        bad[s] = max(t for t in range(f.rows) if tuples[t] == tuples[slots[s]])
        with pytest.raises(AssertionError):
            jr.check_slots(bad, tuples, f.cap)
    if len(occ) < f.cap:
        bad = list(slots)
        bad[next(s for s in range(f.cap) if s not in occ)] = slots[min(occ)]
        with pytest.raises(AssertionError):
            jr.check_slots(bad, tuples, f.cap)


# ---------------------------------------------------------------------------------------------------- the families' facts
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=jr.shape_id)
def test_family_meets_the_facts_it_claims(shape):
    name, args = shape
    f = jr.family(*shape)
    T, rows, cap = f.T, f.rows, f.cap
    assert cap & (cap - 1) == 0 and rows <= cap <= 4096 and len(f.table) == f.w and len(f.table[0]) == T
    tuples = f.tuples()
    present = set(tuples)
    D = len(present)
    homes = dict(zip(f.keys, jr.homes_of(f.keys, cap)))
    occ = jr.occupied([homes[k] for k in present], cap)
    assert occ == f.chain and len(occ) == D
    # what every cell below `rows` is said to be, against the model: hits on table tuples, misses that walk as far as claimed
    seen = {}
    for t in range(rows):
        key, lab = f.keys[f.cells[t]], f.labels[t]
        seen.setdefault(lab, set()).add(key)
        walk = jr.miss_walk(homes[key], occ, cap)
        if lab == jr.HIT:
            assert key in present
        else:
            assert key not in present
        if lab in (jr.MISS_HOME, jr.DEAD):
            assert homes[key] == cap - 1 and walk == D                # behind the whole chain, through the wrap
        elif lab == jr.MISS_INSIDE:
            assert homes[key] in occ and 1 <= walk < D + (name == "staircase")
        elif lab == jr.MISS_ELSEWHERE:
            assert walk == 0
        elif lab == jr.ABSENT_FULL:
            assert walk == cap == D                                   # no empty slot: the walk ends at its bound
    if name == "full":                    # four cells go to the absent tuples (the GPU test also asks for the table itself)
        assert seen[jr.HIT] < present and len(seen[jr.HIT]) == D - 4
    else:
        assert seen[jr.HIT] == present                                # every tuple is asked for: a hit at every depth
    if name in ("one_home", "last_column", "rows_cut"):
        assert {homes[k] for k in present} == {cap - 1}
        assert occ == {cap - 1} | set(range(D - 1)) and D >= 2        # the chain wraps from slot cap - 1 to slot 0
        assert len(seen[jr.MISS_HOME]) == 3
        assert {homes[k] for k in seen[jr.MISS_ELSEWHERE]} >= {D - 1}  # the first empty slot behind the cluster
    if name == "one_home":
        assert D == args[2] and all(tuples.count(k) == args[3] for k in present)
        assert {homes[k] for k in seen[jr.MISS_INSIDE]} == {0, D // 2, D - 2} & occ - {cap - 1}
        assert {homes[k] for k in seen[jr.MISS_ELSEWHERE]} == {D - 1, cap - 2}
        if T >= 1024:                        # one cluster, rows of all four workgroups, most tuples with copies in two of them
            groups = {}
            for t, key in enumerate(tuples):
                groups.setdefault(key, set()).add(t // 256)
            assert set().union(*groups.values()) == {0, 1, 2, 3} and sum(len(g) > 1 for g in groups.values()) >= D // 2
    if name == "staircase":
        k = args[2]
        h0 = cap - k // 2
        by_home = {}
        for key in present:
            by_home.setdefault(homes[key], []).append(key)
        assert sorted(by_home) == sorted((h0 + i) % cap for i in range(k)) and all(len(v) == 2 for v in by_home.values())
        assert occ == {(h0 + d) % cap for d in range(2 * k)} and 0 in occ and cap - 1 in occ
        # every group but the first is displaced by the groups before it: no tuple of home h0 + i can sit below slot h0 + 2 i
        walks = sorted(jr.miss_walk(homes[key], occ, cap) for key in seen[jr.MISS_INSIDE])
        assert walks == list(range(k + 1, 2 * k + 1))                 # one absent probe per home, each to the cluster's end
        assert {homes[key] for key in seen[jr.MISS_ELSEWHERE]} == {(h0 + 2 * k) % cap, h0 - 1}
    if name == "last_column":
        assert f.w == 3 and {key[:2] for key in present} == {jr.LAST_FIXED} and len({key[2] for key in present}) == D
        assert all(key[:2] == jr.LAST_FIXED for lab in (jr.MISS_HOME, jr.MISS_INSIDE, jr.MISS_ELSEWHERE) for key in seen.get(lab, ()))
        assert len(seen[jr.MISS_COLUMN]) == 2
        assert all(any(key[1:] == p[1:] and key[0] != p[0] for p in present) for key in seen[jr.MISS_COLUMN])
    if name == "rows_cut":
        assert rows % 64 and rows < T
        behind = {f.keys[k] for k in f.assign[rows:]}
        dead, both = behind - present, behind & present
        assert dead and both and present - behind and seen[jr.DEAD] == dead
        assert all(max(t for t in range(T) if f.assign[t] == f.keys.index(k)) >= rows for k in both)
        labs = set(f.labels[rows:])
        assert jr.HIT in labs and labs - {jr.HIT}                     # cells behind `rows` that would count and would miss
    if name == "full":
        assert cap == rows == T == D and f.expect(T)[3] == 1 and len(seen[jr.ABSENT_FULL]) == 4
    else:
        assert f.expect(rows)[3] == 0


# ---------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("shape", ALL_SHAPES, ids=jr.shape_id)
def test_references_agree_with_the_counts_of_the_construction(shape):
    f = jr.family(*shape)
    T, rows, w = f.T, f.rows, f.w
    table, probes = f.table, f.probes
    cnt, missing, first, overrun = f.expect(rows)
    if shape[0] == "full":
        # the references know no capacity: they count the absent cells as missing, the device raises the overrun word instead
        absent = [t for t in range(T) if f.labels[t] == jr.ABSENT_FULL]
        assert (cnt, len(absent)) == multiplicities(probes, table, 1, w) and (missing, overrun) == (0, 1)
        return
    sel = f.selector()
    usable, tail = (None, ()) if rows == T else (rows, [0] * (T - rows - 1))
    if rows == T:
        assert (cnt, missing) == multiplicities(probes, table, 1, w)
    mult, miss = sref.multiplicities_sel(probes, table, [None], 1, w, usable, tail)
    assert (mult[:rows], miss) == (cnt[:rows], missing) and not any(cnt[rows:])
    cnt_s, missing_s, _, _ = f.expect(rows, sel)
    mult, miss = sref.multiplicities_sel(probes, table, [sel], 1, w, usable, tail)
    assert (mult[:rows], miss) == (cnt_s[:rows], missing_s)
    off_chain = [t for t in range(rows) if f.labels[t] == jr.MISS_HOME]
    assert (off_chain or shape[0] == "staircase") and all(sel[t] == 0 for t in off_chain)
    assert missing_s <= missing - len(off_chain)
    assert {1, R - 1, 1 << 200} <= set(sel[:rows])
    for index in (False, True):
        n_out = 2 + index
        cols, m, fm = fref.fetched_columns(probes, table + f.payload, 1, w, index, usable, [0] * (n_out * (T - rows)))
        assert (m, fm) == ([missing], [first])
        for t in range(rows):
            q = f.first_row.get(f.cells[t])
            assert [c[t] for c in cols] == ([0] * n_out if q is None else [q] * index + [f.payload[0][q], f.payload[1][q]])


# ---------------------------------------------------------------------------------------------------- the hook's refusals
@pytest.fixture(scope="module")
def lib():
    build()
    return _native.load()


def test_join_hook_refuses_bad_arguments_before_it_looks_at_the_context(lib):
    lib.kzg_last_error.restype = ctypes.c_char_p
    buf = ctypes.create_string_buffer(32 * 16 * 64)
    out = ctypes.create_string_buffer(4 * 4096 * 4)
    m, fi, ov = ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint32(7)

    def refusal(build_=0, walk=0, T=64, rows=64, w=1, n_pay=0, index=0, cap=128, sel=False, data=True):
        a = ctypes.addressof
        rc = lib.kzg_test_join(None, build_, walk, a(buf) if data else None, a(buf), a(buf) if sel else None, T, rows, w, n_pay, index,
                               cap, a(out), a(out), a(out), a(out), ctypes.byref(m), ctypes.byref(fi), ctypes.byref(ov))
        assert rc == _native.KZG_E_ARG
        return lib.kzg_last_error(None)

    none = b"join: no context or no data"
    # valid arguments get as far as the context, and no further
    for kw in ({}, {"build_": 1, "walk": 1, "rows": 33}, {"walk": 2, "sel": True}, {"walk": 3, "n_pay": 2}, {"walk": 3, "index": 1},
               {"cap": 64}, {"build_": 1, "walk": 3, "rows": 1, "cap": 1, "index": 1}, {"T": 4096, "rows": 4096, "cap": 4096},
               {"w": 16}, {"w": 1, "n_pay": 15, "walk": 3}, {"data": False}):
        assert refusal(**kw) == none, kw
    for kw, why in (({"build_": 2}, b"build must be"), ({"build_": -1}, b"build must be"), ({"walk": 4}, b"walk must be"),
                    ({"walk": -1}, b"walk must be"), ({"T": 0, "rows": 0}, b"T outside"), ({"T": 4097, "rows": 4097}, b"T outside"),
                    ({"build_": 1, "walk": 1, "rows": 0}, b"rows outside"), ({"build_": 1, "walk": 1, "rows": 65}, b"rows outside"),
                    ({"rows": 63}, b"rows must be T"), ({"build_": 1, "rows": 63}, b"rows must be T"),
                    ({"walk": 1, "rows": 63}, b"rows must be T"), ({"cap": 0}, b"cap must be"), ({"cap": 96}, b"cap must be"),
                    ({"cap": 32}, b"cap must be"), ({"cap": 8192}, b"cap must be"), ({"cap": 1 << 31}, b"cap must be"),
                    ({"w": 0}, b"w >= 1"), ({"w": 17}, b"w >= 1"), ({"w": 2, "n_pay": 15}, b"w >= 1"),
                    ({"n_pay": 0xFFFFFFFF}, b"w >= 1"), ({"index": 2}, b"index must be"), ({"index": 1}, b"fetch only"),
                    ({"walk": 3}, b"payload column or the index"), ({"sel": True}, b"selector column"),
                    ({"walk": 2}, b"selector column"), ({"walk": 3, "n_pay": 1, "sel": True}, b"selector column")):
        assert why in refusal(**kw), (kw, why)
    assert (m.value, fi.value, ov.value) == (7, 7, 7) and out.raw == bytes(len(out.raw))
    cnt = (ctypes.c_uint32 * 4)(1, 2, 3, 4)
    for n, why in ((0, b"n outside"), (4097, b"n outside"), (4, b"no context or no data")):
        assert lib.kzg_test_join_counts(None, cnt, n, ctypes.addressof(out)) == _native.KZG_E_ARG
        assert why in lib.kzg_last_error(None)
