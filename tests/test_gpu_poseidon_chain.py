"""GPU tests (`-m gpu`) of kzg_rows_commit_poseidon_chain: Poseidon sponges and Merkle paths chained from block to block along
resident rows, computed and committed on the device.  The expected rows come from tests/poseidon_chain_ref.py, which
tests/test_poseidon_chain_cpu.py pins by identities.  Every committed set is compared as tests/test_gpu_poseidon.py compares
its sets: commitments byte for byte against commit_rows of the reference rows, evaluations at block and segment boundaries
through eval_rows, and all cells through read_rows.  Row lengths 2^4 .. 2^10; the longest serial walk is 1024 permutations."""
import ctypes
import random

import pytest

from tests import poseidon_chain_ref as pc
from tests import poseidon_ref as pr
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release
from tests.test_gpu_poseidon import cells, probe, read_all
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x905E1D11, 0x905E1D12


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


def run(eng, cols, params, units, usable=None, tail=(), boundaries=()):
    """commit `cols`, build on the device, compare statistics, commitments, probes and cells with the reference; returns
    (rows, stats)"""
    want, stats = pc.columns(cols, params, units, usable, tail)
    T = len(cols[0])
    S = commit_sets(eng, cols, (len(cols),))
    try:
        inside = eng.rows_stats()
        out, got = eng.commit_poseidon_chain(S, params, units, usable, bt(tail))
        if not want:
            assert out is None and got == stats and eng.rows_stats() == inside, (got, stats)
            return want, stats
        try:
            assert got == stats, (got, stats)
            assert (out.k, out.T, len(out.commitments)) == (len(want), T, len(want))
            ref = eng.commit_rows(0, [row_bytes(r) for r in want])
            try:
                assert out.commitments == ref.commitments
            finally:
                ref.release()
            edge = [0, 1, T - 1, (usable or T) - 1, usable or 0] + list(boundaries)
            probe(eng, out, want, edge)
            for c in range(out.k):
                for t in sorted({e % T for e in edge}):
                    assert cells(eng, out, c, t, 1) == [want[c][t]], (c, t)
            assert read_all(eng, out) == want
        finally:
            out.release()
    finally:
        release(S)
    return want, stats


def rand_cols(k, T, rnd):
    return [[rnd.randrange(R) for _ in range(T)] for _ in range(k)]


def start_col(T, P, starts):
    """a start column: the cells of the blocks in `starts` (a map block -> value) at their first rows, zero elsewhere"""
    col = [0] * T
    for b, v in starts.items():
        col[b * P] = v
    return col


# ---------------------------------------------------------------------------------------------------- sponges
@pytest.mark.parametrize("t,full,partial", [(2, 2, 1), (3, 2, 0), (3, 2, 1), (5, 2, 1), (8, 2, 1)])
def test_a_sponge_without_a_start_column_is_the_rounds_unit_byte_for_byte(engines, t, full, partial):
    eng, T = engines(6), 64
    rnd = random.Random(100 + 10 * t + partial)
    params = pr.make_params(t, full, partial, 600 + t)
    P = full + partial + 2
    cols = rand_cols(t, T, rnd)
    ins = [("imm", R - 1)] + list(range(1, t))
    S = commit_sets(eng, cols, (t,))
    try:
        a, ast = eng.commit_poseidon(S, params, [{"mode": "rounds", "in": ins, "period": P}])
        b, bst = eng.commit_poseidon_chain(S, params, [{"mode": "sponge", "in": ins, "start": None, "period": P, "layout": "trace"}])
        try:
            assert a.commitments == b.commitments and read_all(eng, a) == read_all(eng, b)
            assert bst["blocks"] == ast["perms"] == [T // P] and bst["segments"] == [T // P]
        finally:
            release([a, b])
    finally:
        release(S)


@pytest.mark.parametrize("t,full,partial", [(2, 2, 1), (3, 2, 0), (3, 2, 1), (5, 2, 1), (8, 2, 1)])
@pytest.mark.parametrize("shape", ["every_block", "one_segment", "mixed"])
def test_sponge_segments_and_wrapping_sums(engines, t, full, partial, shape):
    """every block a start; one segment over the whole column; start cells of 1, r - 1 and 0 with a segment that ends at the
    last block.  Message cells 0 and r - 1 meet every carry: r - 1 + out wraps unless out is 0"""
    eng, T = engines(6), 64
    rnd = random.Random(200 + 10 * t + partial + len(shape))
    params = pr.make_params(t, full, partial, 610 + t)
    P = full + partial + 1
    nb = T // P
    cols = rand_cols(t, T, rnd)
    for j in range(1, t):
        for b in range(nb):
            cols[j][b * P] = (0, R - 1, rnd.randrange(R))[(b + j) % 3]
    starts = {"every_block": {b: 1 + b for b in range(nb)}, "one_segment": {},
              "mixed": {0: 0, 2: 1, 3: R - 1, nb - 2: 7}}[shape]
    cols[0] = start_col(T, P, starts)
    ins = [("imm", 5)] + list(range(1, t))
    units = [{"mode": "sponge", "in": ins, "start": 0, "period": P, "layout": "trace"}]
    _, st = run(eng, cols, params, units, boundaries=[b * P + d for b in (0, 1, 2, 3, nb - 1) for d in (-1, 0, P - 1)])
    assert st["segments"] == [{"every_block": nb, "one_segment": 1, "mixed": 4}[shape]] and st["blocks"] == [nb]


def test_flat_segments_across_workgroups(engines):
    """T = 1024, P = 1, t = 3: segments [0, 255), [255, 258), [258, 1024): the lane of block 255 walks into the next workgroup's
    blocks, and the last segment is a serial walk of 766 permutations"""
    eng, T = engines(10), 1 << 10
    rnd = random.Random(300)
    params = pr.make_params(3, 2, 1, 620)
    cols = rand_cols(3, T, rnd)
    cols[0] = start_col(T, 1, {255: R - 1, 258: 1})
    units = [{"mode": "sponge", "in": [("imm", 0), 1, 2], "start": 0, "period": 1, "layout": "flat", "cols": ["out1", "in2", "out0"]}]
    _, st = run(eng, cols, params, units, boundaries=(254, 255, 256, 257, 258, 259, 511, 512))
    assert st["segments"] == [3] and st["blocks"] == [T]


def test_the_full_round_numbers_once(engines):
    """t = 3, R_F = 8, R_P = 57 at T = 1024: a trace sponge at P = 128 (8 blocks, two messages) and a flat path at P = 1 (32
    paths of depth 32)"""
    eng, T = engines(10), 1 << 10
    rnd = random.Random(400)
    params = pr.make_params(3, 8, 57, 630)
    cols = rand_cols(5, T, rnd)
    cols[0] = start_col(T, 128, {5: 1})
    cols[3] = [rnd.randrange(2) for _ in range(T)]
    cols[4] = [int(r % 32 == 0) for r in range(T)]
    units = [{"mode": "sponge", "in": [("imm", 1), 1, 2], "start": 0, "period": 128, "layout": "trace"},
             {"mode": "path", "cap": ("imm", 2), "leaf": 1, "sib": [2], "pos": 3, "digest": 1, "start": 4, "period": 1,
              "layout": "flat", "cols": ["out1"]}]
    _, st = run(eng, cols, params, units, boundaries=(65, 66, 127, 128, 5 * 128 + 65, 31, 32, 33))
    assert st["segments"] == [2, 32] and st["blocks"] == [8, T]


# ---------------------------------------------------------------------------------------------------- paths
@pytest.mark.parametrize("a", [2, 4, 7])
def test_paths_at_every_position_and_bad_positions(engines, a):
    """pos runs through 0 .. a - 1 on starting and continuing blocks; a, r - 1 and 2^32 + 1 are position 0 and counted; cap and
    leaf as rows, and as immediates"""
    eng, T, t = engines(6), 64, a + 1
    rnd = random.Random(500 + a)
    params = pr.make_params(t, 2, 1, 640 + a)
    cols = rand_cols(4 + a - 1, T, rnd)                                # 0 start, 1 leaf, 2 pos, 3 cap, 4 .. siblings
    cols[0] = [int(r % 3 == 0) for r in range(T)]
    cols[2] = [r % a for r in range(T)]
    for r, v in ((10, a), (11, R - 1), (12, (1 << 32) + 1), (40, a + 1)):
        cols[2][r] = v
    sib = list(range(4, 4 + a - 1))
    names = [f"in{j}" for j in range(1, t)] + ["out1", "out0"]
    base = {"mode": "path", "sib": sib, "pos": 2, "digest": 1, "start": 0, "period": 1, "layout": "flat", "cols": names[:8]}
    _, st = run(eng, cols, params, [dict(base, cap=3, leaf=1)], boundaries=(9, 10, 11, 12, 13, 40))
    assert st["bad_pos"] == [4] and st["first_bad_pos"] == [10]
    _, st = run(eng, cols, params, [dict(base, cap=("imm", R - 1), leaf=("imm", 0), digest=0, cols=["out0", "in1", f"in{a}"])])
    assert st["bad_pos"] == [4] and st["segments"] == [22]


def test_a_trace_path_over_two_workgroups_with_a_cut_block(engines):
    """t = 3, R = 2, P = 3 at T = 1024 with usable: 339 whole blocks, the last segment ends at the cut block; the tail follows"""
    eng, T, P = engines(10), 1 << 10, 3
    u = T - 5
    rnd = random.Random(600)
    params = pr.make_params(3, 2, 0, 650)
    cols = rand_cols(4, T, rnd)
    nb = u // P
    cols[0] = start_col(T, P, {b: 1 for b in range(0, nb, 5)})
    cols[3] = [rnd.randrange(2) for _ in range(T)]
    for c in cols:
        c[u:] = [R - 1 - r for r in range(T - u)]
    units = [{"mode": "path", "cap": ("imm", 0), "leaf": 1, "sib": [2], "pos": 3, "digest": 2, "start": 0, "period": P, "layout": "trace"}]
    tail = [rnd.randrange(R) for _ in range(3 * (T - u))]
    last = nb * P
    want, st = run(eng, cols, params, units, u, tail, boundaries=(767, 768, 769, last - 1, last, last + 1, u - 1, u, u + 1))
    assert u % P and st["blocks"] == [nb] and st["segments"] == [(nb + 4) // 5]
    assert all(want[j][r] == 0 for j in range(3) for r in range(last, u))


# ---------------------------------------------------------------------------------------------------- the smallest rows
@pytest.mark.parametrize("usable", [None, 13])
def test_sixteen_rows(engines, usable):
    """T = 2^4, (3, 2, 0): a trace sponge at P = R + 1 = 3 (5 blocks and a leftover row; with usable = 13 four blocks, the cut
    block beside the tail), a flat path at P = 1, and a check of that path beside them, one digest planted wrong"""
    eng, T = engines(4), 16
    before = eng.rows_stats()
    rnd = random.Random(1100 + (usable or 0))
    params = pr.make_params(3, 2, 0, 700)
    n = usable or T
    cols = rand_cols(6, T, rnd)                                        # 0, 1 data; 2 pos; 3 start (P = 3); 4 start (P = 1); 5 expect
    cols[2] = [r % 2 for r in range(T)]
    cols[3] = start_col(T, 3, {2: R - 1, 3: 1})
    cols[4] = [int(r % 4 == 0) for r in range(T)]
    path = {"mode": "path", "cap": ("imm", 6), "leaf": 0, "sib": [1], "pos": 2, "digest": 1, "start": 4, "period": 1}
    tail1 = [0] * (T - n) if usable else ()
    flat, _ = pc.columns(cols, params, [dict(path, layout="flat", cols=["out1"])], usable, tail1)
    cols[5] = list(flat[0])
    cols[5][7] = (cols[5][7] + 1) % R                                  # the path of rows 4 .. 7 ends at row 7
    units = [{"mode": "sponge", "in": [("imm", 2), 0, 1], "start": 3, "period": 3, "layout": "trace"},
             dict(path, layout="flat", cols=["out1", "in1", "in2"]), dict(path, expect=5)]
    tail = [rnd.randrange(R) for _ in range(6 * (T - n))] if usable else ()
    last = (n // 3) * 3
    want, st = run(eng, cols, params, units, usable, tail, boundaries=(2, 3, 5, 6, 7, 8, 9, last - 1, last, n - 1))
    assert st["blocks"] == [n // 3, n, n] and st["segments"] == [3, (n + 3) // 4, (n + 3) // 4]
    assert st["mismatch"] == [0, 0, 1] and st["first_mismatch"] == [None, None, 7]
    assert all(want[j][r] == 0 for j in range(3) for r in range(last, n))
    # the same check alone: no set
    rows, st = run(eng, cols, params, [dict(path, expect=5)], usable)
    assert rows == [] and st["mismatch"] == [1] and st["segments"] == [(n + 3) // 4]
    assert eng.rows_stats() == before


@pytest.mark.parametrize("lg", [7, 8, 9])
def test_row_lengths_between(engines, lg):
    """T = 2^7 .. 2^9, (5, 2, 1): messages of 3 blocks at P = 4 as a trace, and arity-4 paths of depth 5 at P = 1"""
    eng, T = engines(lg), 1 << lg
    rnd = random.Random(1200 + lg)
    params = pr.make_params(5, 2, 1, 710)
    cols = rand_cols(8, T, rnd)                                        # 0 .. 3 data; 4 pos; 5 start (P = 4); 6 start (P = 1); 7 cap
    cols[4] = [rnd.randrange(4) for _ in range(T)]
    cols[5] = start_col(T, 4, {b: 1 for b in range(0, T // 4, 3)})
    cols[6] = [int(r % 5 == 0) for r in range(T)]
    units = [{"mode": "sponge", "in": [("imm", 0), 0, 1, 2, 3], "start": 5, "period": 4, "layout": "trace"},
             {"mode": "path", "cap": 7, "leaf": 0, "sib": [1, 2, 3], "pos": 4, "digest": 4, "start": 6, "period": 1, "layout": "flat",
              "cols": ["out4", "in4"]}]
    _, st = run(eng, cols, params, units, boundaries=(3, 4, 11, 12, 255, 256, 257, T - 4))
    assert st["segments"] == [(T // 4 + 2) // 3, (T + 4) // 5]


# ---------------------------------------------------------------------------------------------------- several units, checks
def test_four_units_of_mixed_modes(engines):
    eng, T = engines(5), 32
    before = eng.rows_stats()
    rnd = random.Random(700)
    params = pr.make_params(4, 2, 1, 660)
    cols = rand_cols(7, T, rnd)
    cols[0] = start_col(T, 4, {3: 1, 4: 2})
    cols[6] = [r % 3 for r in range(T)]
    want0, _ = pc.columns(cols, params, [{"mode": "sponge", "in": [1, 2, ("imm", 3), 4], "start": 0, "period": 4, "layout": "flat",
                                          "cols": ["out2"]}])
    exp = list(want0[0])
    exp[2 * 4] = (exp[2 * 4] + 1) % R                                  # the segment of blocks 0 .. 2 ends at row 8
    cols.append(exp)
    units = [{"mode": "sponge", "in": [1, 2, ("imm", 3), 4], "start": 0, "period": 4, "layout": "trace"},
             {"mode": "path", "cap": 5, "leaf": 1, "sib": [2, 4], "pos": 6, "digest": 3, "start": None, "period": 2, "layout": "flat",
              "cols": ["in1", "in2", "in3", "out3"]},
             {"mode": "sponge", "in": [1, 2, ("imm", 3), 4], "start": 0, "period": 4, "digest": 2, "expect": 7},
             {"mode": "path", "cap": 5, "leaf": 1, "sib": [2, 4], "pos": 6, "digest": 3, "start": 0, "period": 4, "layout": "trace"}]
    want, st = run(eng, cols, params, units, boundaries=(3, 4, 7, 8, 11, 12, 15, 16, 28))
    assert len(want) == 12 and st["segments"] == [3, 16, 3, 3]
    assert st["mismatch"] == [0, 0, 1, 0] and st["first_mismatch"] == [None, None, 8, None]
    assert eng.rows_stats() == before


@pytest.mark.parametrize("planted", [None, 0, 5, 9])
def test_a_call_of_checks_alone_makes_no_set(engines, planted):
    """ten paths of depth 3 at P = 2 over a binary tree's levels written by hand; expect holds the root at each path's last
    block; a mismatch planted at a chosen path is found with its row"""
    eng, T, P, depth = engines(6), 64, 2, 3
    before = eng.rows_stats()
    rnd = random.Random(800)
    params = pr.make_params(3, 2, 1, 670)
    cols = rand_cols(5, T, rnd)                                        # 0 start, 1 leaf, 2 sibling, 3 pos, 4 expect
    cols[3] = [rnd.randrange(2) for _ in range(T)]
    cols[0] = start_col(T, P, {b: 1 for b in range(0, 30, depth)})
    unit = {"mode": "path", "cap": ("imm", 9), "leaf": 1, "sib": [2], "pos": 3, "digest": 1, "start": 0, "period": P}
    flat, _ = pc.columns(cols, params, [dict(unit, layout="flat", cols=["out1"])], usable=60, tail=[0] * 4)
    cols[4] = [flat[0][r] if (r // P) % depth == depth - 1 else rnd.randrange(R) for r in range(T)]
    if planted is not None:
        cols[4][(planted * depth + depth - 1) * P] ^= 1
    rows, st = run(eng, cols, params, [dict(unit, expect=4), {"mode": "sponge", "in": [1, 2, 3], "start": 0, "period": P,
                                                             "digest": 0, "expect": 4}], usable=60)
    assert rows == [] and st["segments"] == [10, 10] and st["blocks"] == [30, 30]
    assert st["mismatch"] == [int(planted is not None), 10]
    assert st["first_mismatch"] == [None if planted is None else (planted * depth + depth - 1) * P, (depth - 1) * P]
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 5
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg, 0)
    rnd = random.Random(900)
    params = pr.make_params(3, 2, 1, 680)
    cols = rand_cols(4, T, rnd)
    cols[3] = [r % 2 for r in range(T)]
    units = [{"mode": "sponge", "in": [0, 1, ("imm", 3)], "start": 3, "period": 4, "layout": "trace"},
             {"mode": "path", "cap": ("imm", 1), "leaf": 0, "sib": [1], "pos": 3, "digest": 1, "start": 2, "period": 1, "layout": "flat",
              "cols": ["out1", "in1"]}]
    want, stats = pc.columns(cols, params, units)
    I = commit_sets(eng, cols, (4,))

    def fresh_ok():
        out, got = eng.commit_poseidon_chain(I, params, units)
        try:
            assert got == stats and read_all(eng, out) == want
        finally:
            out.release()

    fresh_ok()
    live = eng.rows_stats()
    lib = _native.load()
    hi = (ctypes.c_uint64 * 1)(I[0].handle)
    c, h = ctypes.create_string_buffer(48 * 16), ctypes.c_uint64(0)
    st = [(ctypes.c_uint64 * 16)() for _ in range(6)]
    par, recs = eng.poseidon_chain_call(params, units)
    IMM = A = _native.KZG_POSEIDON_CHAIN_ABSENT

    def raw(recs, par=par, opts=None, n_units=None, reserved=0):
        pp = _native.PoseidonParams(*par)
        arr = (_native.PoseidonChainUnit * max(len(recs), 1))(*[eng.poseidon_chain_unit_struct(r) for r in recs])
        if reserved:
            arr[0].reserved = reserved
        return lib.kzg_rows_commit_poseidon_chain(eng._h, 1, hi, ctypes.byref(pp), len(recs) if n_units is None else n_units, arr,
                                                  ctypes.byref(opts) if opts else None, c, *st, ctypes.byref(h))

    def refused(rc, why):
        msg = lib.kzg_last_error(eng._h)
        assert rc == _native.KZG_E_ARG and msg.startswith(b"poseidon_chain: ") and why in msg, (rc, msg)
        assert eng.rows_stats() == live

    names = ("mode", "flags", "layout", "period", "start", "pos", "digest", "expect", "n_out", "in_", "out", "imm")
    edit = lambda base, **kw: tuple(kw.get(f, v) for f, v in zip(names, base))   # noqa: E731
    pedit = lambda **kw: tuple(kw.get(f, v) for f, v in zip(("t", "full", "partial", "rc", "mds"), par))   # noqa: E731
    sp, pa = recs
    big, z = R.to_bytes(32, "big"), bytes(32)
    pad = lambda xs, n: list(xs) + [0] * (n - len(xs))   # noqa: E731
    refused(raw([sp], pedit(t=1)), b"width t")
    refused(raw([sp], pedit(t=9)), b"width t")
    refused(raw([sp], pedit(full=3)), b"R_F must be even")
    refused(raw([sp], pedit(partial=129)), b"R_P")
    refused(raw([sp], pedit(rc=par[3][:-32] + big)), b"round constants must be canonical")
    refused(raw([sp], pedit(mds=big + par[4][32:])), b"matrix entries must be canonical")
    refused(raw([], n_units=0), b"n_units")
    refused(raw([sp] * 5), b"n_units")
    refused(raw([edit(sp, mode=0)]), b"unknown mode")
    refused(raw([edit(sp, mode=3)]), b"unknown mode")
    refused(raw([edit(sp, flags=2)]), b"flags")
    refused(raw([sp], reserved=1), b"flags")
    p2 = pr.make_params(2, 2, 1, 681)
    par2, recs2 = eng.poseidon_chain_call(p2, [{"mode": "sponge", "in": [0, 1], "start": None, "period": 4, "layout": "trace"}])
    refused(raw([edit(recs2[0], mode=2, pos=3, digest=1)], par2), b"t >= 3")
    refused(raw([edit(sp, period=0)]), b"period P")
    refused(raw([edit(sp, period=3)]), b"at least R + 1")
    refused(raw([edit(sp, layout=0)]), b"unknown layout")
    refused(raw([edit(sp, layout=3)]), b"unknown layout")
    refused(raw([edit(sp, n_out=2)]), b"n_out must be")
    refused(raw([edit(pa, n_out=0)]), b"n_out must be")
    refused(raw([edit(pa, n_out=7)]), b"n_out must be")
    refused(raw([edit(pa, out=pad([3], 16), n_out=1)]), b"unknown column id")
    refused(raw([edit(pa, out=pad([16], 16), n_out=1)]), b"unknown column id")
    refused(raw([edit(sp, out=pad([0, 2, 1], 16))]), b"unknown column id")
    refused(raw([edit(pa, out=pad([9, 9], 16))]), b"repeated")
    refused(raw([edit(sp, flags=1, expect=0, digest=0)]), b"beside KZG_POSEIDON_CHAIN_CHECK")
    refused(raw([edit(sp, flags=1, layout=0, n_out=0, digest=0)]), b"expect must be a row")
    refused(raw([edit(sp, expect=0)]), b"expect belongs")
    refused(raw([edit(sp, flags=1, layout=0, n_out=0, expect=0)]), b"digest must be")
    refused(raw([edit(sp, digest=1)]), b"digest belongs")
    refused(raw([edit(pa, digest=3)]), b"digest must be")
    refused(raw([edit(pa, digest=A)]), b"digest must be")
    refused(raw([edit(pa, pos=A)]), b"pos must be a row")
    refused(raw([edit(sp, pos=1)]), b"pos belongs")
    refused(raw([edit(pa, in_=pad([IMM, 0, IMM], 8))]), b"sibling")
    refused(raw([edit(sp, in_=pad([0, 1, 2, 3], 8), imm=[z] * 8)]), b"above t must be 0")
    refused(raw([edit(sp, in_=pad([0, 4, IMM], 8))]), b"concatenated rows")
    refused(raw([edit(sp, start=4)]), b"concatenated rows")
    refused(raw([edit(pa, pos=9)]), b"concatenated rows")
    refused(raw([edit(sp, flags=1, layout=0, n_out=0, digest=0, expect=4)]), b"concatenated rows")
    refused(raw([edit(sp, imm=[z, z, big] + [z] * 5)]), b"immediates must be canonical")
    refused(raw([edit(sp, imm=[z, be(1), be(3)] + [z] * 5)]), b"0 beside a row")
    refused(raw([edit(pa, out=pad([0, 1, 2, 8, 9, 10], 16), n_out=6)] * 3), b"n_out")
    wide = pr.make_params(8, 2, 0, 682)
    wpar, wrecs = eng.poseidon_chain_call(wide, [{"mode": "sponge", "in": list(range(8)), "start": 8, "period": 1, "layout": "flat",
                                                  "cols": ["out0"]}])
    second = edit(wrecs[0], in_=list(range(9, 17)))                    # 8 + 1 + 8 = 17 distinct rows
    refused(raw([wrecs[0], second], wpar), b"distinct input rows")
    tl = b"".join(bt([rnd.randrange(R) for _ in range(5 * 4)]))
    for usable, tail, why in ((T, tl, b"usable must be in"), (T - 4, None, b"tail_be32 must be given"), (0, tl, b"plain layout"),
                              (T - 4, tl[:-32] + big, b"canonical")):
        refused(raw([sp, pa], opts=_native.DeriveOpts(usable, tail)), why)
    fresh_ok()
    assert raw([edit(sp, imm=[z, z, be(R - 1)] + [z] * 5)]) == 0      # the largest immediate that is canonical
    eng.release_rows(h.value)
    for bad, why in ((dict(units[0], mode="rounds"), "unknown mode"), (dict(units[0], sib=[1]), "does not take"),
                     (dict(units[1], digest=3), "digest must be"), (dict(units[0], period=3), "at least R + 1"),
                     (dict(units[1], cols=["out3"]), "unknown column name"), (dict(units[0], **{"in": [0, 4, 1]}), "concatenated rows"),
                     (dict(units[0], **{"in": [0, 1, ("imm", R)]}), "canonical"), (dict(units[1], sib=[("imm", 1)]), "not an immediate")):
        arg_error(lambda: eng.commit_poseidon_chain(I, params, [bad]), why)
    arg_error(lambda: eng.commit_poseidon_chain(I, dict(params, full=3), units), "R_F must be even")
    arg_error(lambda: eng.commit_poseidon_chain(I, params, units, None, [be(1)]), "tail")
    arg_error(lambda: eng.commit_poseidon_chain([2 ** 40], params, units), "unknown")
    fresh_ok()
    release(I)
    assert eng.rows_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------------- routing
def test_client_and_multi_device_client_return_the_engine_bytes(hip):
    from zkp_subnet_amd import Client, MultiDeviceClient, codec

    scale, ms = 6, 0
    T = 1 << scale
    rnd = random.Random(1000)
    params = pr.make_params(3, 2, 2, 690)
    cols = rand_cols(4, T, rnd)
    cols[0] = start_col(T, 8, {2: 1, 5: 3})
    cols[3] = [r % 2 for r in range(T)]
    units = [{"mode": "sponge", "in": [1, ["imm", str(R - 1)], 2], "start": 0, "period": 8, "layout": "trace"},
             {"mode": "path", "cap": ["imm", "0x7"], "leaf": 1, "sib": [2], "pos": 3, "digest": 1, "start": 0, "period": 8,
              "layout": "flat", "cols": ["out1"]}]
    want, stats = pc.columns(cols, params, units)
    wire = dict(params, rc=[hex(v) for v in params["rc"]], mds=[str(v) for v in params["mds"]])
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    for client in (Client(seed=84), MultiDeviceClient(devices=[0], seed=84)):
        client.start(scale=scale, machines_scale=ms)
        try:
            a = client.worker_commit_rows(0, [fr(col) for col in cols]).json()["handle"]
            ref = client.worker_commit_rows(0, [fr(col) for col in want]).json()
            r = client.worker_commit_poseidon_chain([a], wire, units)
            assert r.status_code == 200, r.json()
            body = r.json()
            assert body["commitments"] == ref["commitments"]
            assert {k: body[k] for k in stats} == stats
            chk = client.worker_commit_poseidon_chain([a, ref["handle"]], wire, [
                {"mode": "path", "cap": ["imm", "0x7"], "leaf": 1, "sib": [2], "pos": 3, "digest": 1, "start": 0, "period": 8, "expect": 7},
                {"mode": "path", "cap": ["imm", "0x7"], "leaf": 1, "sib": [2], "pos": 3, "digest": 1, "start": 0, "period": 8, "expect": 4}])
            assert chk.status_code == 200, chk.json()
            assert chk.json()["handle"] is None and chk.json()["commitments"] == []
            assert chk.json()["mismatch"] == [0, 3] and chk.json()["first_mismatch"] == [None, 8]
            assert client.worker_commit_poseidon_chain([a], wire, [dict(units[0], mode="rounds")]).status_code == 400
            assert client.worker_commit_poseidon_chain([a], dict(wire, full=3), units).status_code == 400
            assert client.worker_commit_poseidon_chain([a], wire, units, None, fr([1])).status_code == 400
            for hh in (ref["handle"], body["handle"], a):
                assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_poseidon_chain([a], wire, units).status_code == 400
        finally:
            client.stop()
