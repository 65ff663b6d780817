"""GPU tests (`-m gpu`) of the hash join of csrc/fr_join.hip on inputs CONSTRUCTED so that a named path is certain to run
(tests/join_ref.py; tests/test_join_cpu.py proves the construction without a device): chains of up to 512 slots, walks that pass
from slot cap - 1 to slot 0, duplicates of many tuples from four workgroups in one cluster, misses that end only behind a whole
cluster, tuples of one home that differ in their last column only, a table cut at `rows`, a full table.

Hook level (kzg_test_join: both builds and all four walks through the library's own launchers, the slot table itself read back):
every statement is schedule-independent -- WHICH slots are occupied, that a slot holds the smallest row of its tuple, that a
tuple sits in one slot with no empty slot between its home and it, and every counter, count and fetched byte.  Which tuple of a
cluster sits in which of its slots is the schedule's choice and is not compared.  End to end the same families go through
commit_multiplicities, _zk, _sel and commit_fetch at the builders' own capacity 2 T, against the Python references and the C oracle."""
import random

import pytest

from oracle import cpu as oc
from tests import fetch_ref as fref
from tests import join_ref as jr
from tests import lookup_sel_ref as sref
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release, srs_cache
from tests.multiplicities_ref import multiplicities
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x701A11, 0x701A12
BUILD, BUILD_ROWS = 0, 1
PROBE, PROBE_ROWS, PROBE_SEL, FETCH = 0, 1, 2, 3


@pytest.fixture(scope="module")
def eng(hip):
    return hip()                       # the hook needs no SRS


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def srs_of():
    return srs_cache(SEED_X, SEED_Y)


def cols_bytes(cols):
    return b"".join(row_bytes(c) for c in cols)


def run_hook(eng, f, build, walk, index=False, probes=None):
    """one build and one walk over family f through kzg_test_join, every output checked; returns the outputs"""
    T, rows, cap, w = f.T, f.rows, f.cap, f.w
    probes = f.probes if probes is None else probes
    sel = f.selector() if walk == PROBE_SEL else None
    n_pay = 2 if walk == FETCH else 0
    out = eng.test_join(build, walk, cols_bytes(f.table + f.payload[:n_pay]), cols_bytes(probes), T, rows, w, cap, n_pay, index,
                        row_bytes(sel) if sel else None)
    # the device's home slots are the model's: if not, the PORT of the hash in tests/join_ref.py is wrong
    assert out["home_tab"] == jr.homes_of(list(zip(*f.table)), cap)
    assert out["home_in"] == jr.homes_of(list(zip(*probes)), cap)
    # the table: the model's occupied set, the smallest row of every tuple in exactly one slot, no hole in front of it
    where = jr.check_slots(out["slots"], f.tuples(), cap)
    assert set(where.values()) == f.chain
    return out


def check_walk(out, f, walk, index=False):
    """counters, missing, first, overrun and the fetched bytes of run_hook's outputs over f's own probe cells"""
    T, rows = f.T, f.rows
    n_cells = T if walk == PROBE else rows
    cnt, missing, first, overrun = f.expect(n_cells, f.selector() if walk == PROBE_SEL else None)
    assert out["overrun"] == overrun and out["missing"] == missing
    if walk != FETCH:
        assert out["cnt"] == cnt and out["first"] is None and out["fetched"] == []
        return
    assert not any(out["cnt"]) and out["first"] == first
    usable = None if rows == T else rows
    want, ref_missing, ref_first = fref.fetched_columns(f.probes, f.table + f.payload, 1, f.w, index, usable,
                                                        [0] * ((2 + index) * (T - rows)))
    if not overrun:
        assert ([missing], [first]) == (ref_missing, ref_first)
    assert len(out["fetched"]) == len(want) == 2 + index
    for got, col in zip(out["fetched"], want):
        assert got[:32 * rows] == row_bytes(col[:rows])
        assert len({got[32 * t:32 * t + 32] for t in range(rows, T)}) <= 1      # behind `rows`: the fill pattern, untouched
        assert got[32 * rows:32 * rows + 32] not in (be(0), be(col[0]))


def forms(f):
    builds = (BUILD, BUILD_ROWS) if f.rows == f.T else (BUILD_ROWS,)
    walks = (PROBE, PROBE_ROWS, PROBE_SEL, FETCH) if f.rows == f.T else (PROBE_ROWS, PROBE_SEL, FETCH)
    return [(b, wk) for b in builds for wk in walks]


# ---------------------------------------------------------------------------------------------------- the hook
@pytest.mark.parametrize("shape", jr.HOOK_SHAPES, ids=jr.shape_id)
def test_both_builds_and_all_four_walks(eng, shape):
    f = jr.family(*shape)
    for build, walk in forms(f):
        for index in ((False, True) if walk == FETCH else (False,)):
            check_walk(run_hook(eng, f, build, walk, index), f, walk, index)
    if shape[0] == "full":
        # every tuple of a full table is a hit, at whatever depth its slot lies: no overrun, no miss
        for build, walk in forms(f):
            out = run_hook(eng, f, build, walk, probes=f.table)
            assert (out["overrun"], out["missing"], out["first"]) == (0, 0, None)
            if walk in (PROBE, PROBE_ROWS):
                assert out["cnt"] == [1] * f.T                       # distinct tuples: every row counts its own cell
    else:
        assert 0 in f.chain and f.cap - 1 in f.chain                # the cluster wraps (tests/test_join_cpu.py: and the rest)


def test_selector_turns_off_the_cells_that_would_walk_the_whole_chain(eng):
    f = jr.family("one_home", (256, 512, 64, 4))
    sel = f.selector()
    off = [t for t in range(f.T) if f.labels[t] == jr.MISS_HOME]
    assert off and not any(sel[t] for t in off) and {R - 1, 1 << 200} <= set(sel)
    plain = run_hook(eng, f, BUILD, PROBE_ROWS)
    out = run_hook(eng, f, BUILD, PROBE_SEL)
    cnt, missing, _, _ = f.expect(f.T, sel)
    assert (out["cnt"], out["missing"], out["overrun"]) == (cnt, missing, 0)
    mult, miss = sref.multiplicities_sel(f.probes, f.table, [sel], 1, 1)
    assert (out["cnt"], out["missing"]) == (mult, miss)
    # the cells that are off are neither counted nor missed: the plain probe's answers less those cells' own
    assert plain["missing"] - out["missing"] == sum(1 for t in range(f.T) if not sel[t] and f.cells[t] not in f.first_row)
    assert sum(plain["cnt"]) - sum(out["cnt"]) == sum(1 for t in range(f.T) if not sel[t] and f.cells[t] in f.first_row)
    # r - 1 and 2^200 count as on: cells under each of them hit and miss, and the counts above hold them
    for v in (R - 1, 1 << 200):
        assert {f.cells[t] in f.first_row for t in range(f.T) if sel[t] == v} == {True, False}


def test_three_runs_give_the_same_answers_and_the_same_table(eng):
    """Which tuple of a cluster sits in which of its slots is the schedule's choice (512 tuples of four workgroups claim one
    home), so the slot words are compared as a set with their places checked by the invariants of run_hook; everything a caller can
    see is compared as it is."""
    f = jr.family("one_home", (1024, 2048, 512, 2))
    runs = [run_hook(eng, f, BUILD, FETCH, True) for _ in range(3)]
    for out in runs:
        check_walk(out, f, FETCH, True)
    for out in runs[1:]:
        assert {k: v for k, v in out.items() if k != "slots"} == {k: v for k, v in runs[0].items() if k != "slots"}
        assert sorted(out["slots"]) == sorted(runs[0]["slots"])
        assert [q == jr.EMPTY for q in out["slots"]] == [q == jr.EMPTY for q in runs[0]["slots"]]
    probes = [run_hook(eng, f, BUILD, PROBE) for _ in range(3)]
    assert all(p["cnt"] == probes[0]["cnt"] and p["missing"] == probes[0]["missing"] for p in probes)


def test_counters_split_at_bit_29_come_back_as_their_integers(eng):
    words = [0, 1, (1 << 29) - 1, 1 << 29, (1 << 29) + 1, 1 << 31, (1 << 32) - 1]
    assert eng.test_join_counts(words) == row_bytes(words)
    rnd = random.Random(29)
    more = [rnd.randrange(1 << 32) for _ in range(300)] + [(1 << k) - d for k in range(28, 33) for d in (0, 1) if (1 << k) - d < 1 << 32]
    assert eng.test_join_counts(more) == row_bytes(more)


def test_hook_errors_leave_the_context_serving(eng):
    f = jr.family("one_home", (32, 64, 8, 4))
    tab, cells = cols_bytes(f.table), cols_bytes(f.probes)
    arg_error(lambda: eng.test_join(BUILD, PROBE, tab, cells, 32, 32, 1, 16), "cap must be")
    arg_error(lambda: eng.test_join(BUILD, PROBE_ROWS, tab, cells, 32, 20, 1, 64), "rows must be T")
    arg_error(lambda: eng.test_join(BUILD, FETCH, tab, cells, 32, 32, 1, 64), "payload column or the index")
    arg_error(lambda: eng.test_join(BUILD, PROBE, tab, cells, 32, 32, 1, 64, sel_be32=cells), "selector column")
    arg_error(lambda: eng.test_join(BUILD, PROBE, tab[32:], cells, 32, 32, 1, 64), "table cells")
    bad = R.to_bytes(32, "big") + tab[32:]
    arg_error(lambda: eng.test_join(BUILD, PROBE, bad, cells, 32, 32, 1, 64), code=_native.KZG_E_SCALAR)
    arg_error(lambda: eng.test_join_counts([]), "n outside")
    check_walk(run_hook(eng, f, BUILD, PROBE), f, PROBE)


# ---------------------------------------------------------------------------------------------------- end to end
def check_rows(eng, srs, rset, want, stats, want_stats):
    """the new set against its expected evaluation rows: the statistics, the oracle's commitments, every cell through read_rows"""
    assert stats == want_stats, (stats, want_stats)
    T = len(want[0])
    assert (rset.k, rset.T, len(rset.commitments)) == (len(want), T, len(want))
    for c, col in enumerate(want):
        assert rset.commitments[c] == oc.commit(srs, row_bytes(col), True), c
        assert eng.read_rows([rset], c, 0, T, "fr") == (row_bytes(col), 0, None), c


@pytest.mark.parametrize("shape", jr.E2E_SHAPES, ids=jr.shape_id)
def test_builders_at_their_own_capacity(engines, srs_of, shape):
    f = jr.family(*shape)
    T, w = f.T, f.w
    assert f.cap == 2 * T                                             # the families rebuilt for the builders' one capacity
    lg = T.bit_length() - 1
    eng, srs = engines(lg), srs_of(lg)
    before = eng.rows_stats()
    rnd = random.Random(T + w)
    table, probes, sel = f.table, f.probes, f.selector()
    u = f.rows if f.rows < T else T - 5                               # the _zk layout: T - u within the 32 blinding rows
    tail = [rnd.randrange(R) for _ in range(T - u - 1)]
    made = commit_sets(eng, probes + table + f.payload + [sel], (w, w, 2, 1))
    F, KEY, PAY, S = ([s] for s in made)
    try:
        def built(call, want, want_stats):
            rset, *stats = call()
            made.append(rset)
            check_rows(eng, srs, rset, want, tuple(stats), want_stats)

        mult, missing = multiplicities(probes, table, 1, w)
        if f.rows == T:
            assert (mult, missing) == f.expect(T)[:2]
        built(lambda: eng.commit_multiplicities(F, KEY, 1, w), [mult], (missing,))
        mult, missing = sref.multiplicities_sel(probes, table, [None], 1, w, u, tail)
        if f.rows < T:
            assert (mult[:u], missing) == (f.expect(u)[0][:u], f.expect(u)[1])
        built(lambda: eng.commit_multiplicities_zk(F, KEY, 1, w, u, bt(tail)), [mult], (missing,))
        for usable, tl in ((None, []), (u, tail)):
            mult, missing = sref.multiplicities_sel(probes, table, [sel], 1, w, usable, tl)
            assert missing < sref.multiplicities_sel(probes, table, [None], 1, w, usable, tl)[1]
            built(lambda: eng.commit_multiplicities_sel(F, KEY, S, [0], 1, w, usable, bt(tl)), [mult], (missing,))
        for index in (False, True):
            for usable in (None, u):
                n = T if usable is None else usable
                tl = [rnd.randrange(R) for _ in range((2 + index) * (T - n))]
                want, miss, first = fref.fetched_columns(probes, table + f.payload, 1, w, index, usable, tl)
                if n == f.rows:
                    assert (miss, first) == ([f.expect(n)[1]], [f.expect(n)[2]])
                built(lambda: eng.commit_fetch(F, KEY + PAY, 1, w, index, usable, bt(tl)), want, (miss, first))
    finally:
        release(made)
    assert eng.rows_stats() == before
