"""GPU tests (`-m gpu`) of kzg_rows_commit_poseidon: the Poseidon permutation (x^5, the caller's constants) of resident rows, one
per row, as a check against expected rows, or as the round trace in blocks of P rows, computed and committed on the device.
The expected rows come from the definition in Python integers (tests/poseidon_ref.py), which tests/test_poseidon_cpu.py pins
by identities: no published known-answer vector is available here.  Round constants are seeded random scalars, the matrix is a
Cauchy matrix.  Every committed set is compared three ways: its commitments byte for byte against commit_rows of the reference
rows, its evaluations at domain points (the first, the last and the block-boundary rows) through eval_rows, and its cells
through read_rows.  Row lengths 2^4 .. 2^10.  (The refusal of T above 2^32 cannot be reached with a set that fits a device.)"""
import ctypes
import random

import pytest

from tests import grand_product_ref as gp
from tests import poseidon_ref as pr
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release, split_first, split_halves
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x905E1D01, 0x905E1D02


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


def cells(eng, rset, c, first, count):
    raw = eng.read_rows([rset], c, first, count, "fr")[0]
    return [int.from_bytes(raw[32 * t:32 * t + 32], "big") for t in range(count)]


def read_all(eng, rset):
    return [cells(eng, rset, c, 0, rset.T) for c in range(rset.k)]


def probe(eng, rset, want, rows_at):
    """the set's evaluations at the domain points of the rows `rows_at`, every column, against the expected cells"""
    T, k = rset.T, rset.k
    w = gp.omega(T)
    ts = sorted({t % T for t in rows_at})
    for t0 in range(0, len(ts), 4):
        part = ts[t0:t0 + 4]
        Y = eng.eval_rows([rset], [be(pow(w, t, R)) for t in part], [list(range(k))] * len(part))
        assert Y == [[be(want[c][t]) for c in range(k)] for t in part], part


def run(eng, cols, params, units, usable=None, tail=(), sizes=None, boundaries=()):
    """commit `cols`, build on the device, compare statistics, commitments, probes and cells with the reference; returns
    (rows, stats)"""
    want, stats = pr.columns(cols, params, units, usable, tail)
    T = len(cols[0])
    S = commit_sets(eng, cols, sizes or (len(cols),))
    try:
        out, got = eng.commit_poseidon(S, params, units, usable, bt(tail))
        if not want:
            assert out is None and got == stats, (got, stats)
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


def input_cols(k, T, rnd):
    """k columns whose first rows hold 0 and r - 1 in every combination of neighbours, random below"""
    cols = [[rnd.randrange(R) for _ in range(T)] for _ in range(k)]
    for j, c in enumerate(cols):
        c[0], c[1], c[2], c[3] = 0, R - 1, (0 if j % 2 else R - 1), (R - 1 if j % 2 else 0)
    return cols


# ---------------------------------------------------------------------------------------------------- row units
@pytest.mark.parametrize("lg", [4, 9])
@pytest.mark.parametrize("t,full,partial", [(2, 2, 0), (2, 2, 1), (3, 2, 0), (3, 2, 1), (4, 2, 0), (4, 2, 1), (8, 2, 0), (8, 2, 1)])
def test_row_units_every_width(engines, lg, t, full, partial):
    """every state element out, in reversed order (out reorders the state); T = 512 runs two workgroups of 256 lanes"""
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(1000 * t + 10 * partial + lg)
    params = pr.make_params(t, full, partial, 40 + t)
    cols = input_cols(t, T, rnd)
    _, st = run(eng, cols, params, [{"mode": "row", "in": list(range(t)), "out": list(reversed(range(t)))}])
    assert st["perms"] == [T]
    assert eng.rows_stats() == before


@pytest.mark.parametrize("lg", [4, 6])
def test_row_unit_at_the_full_round_numbers(engines, lg):
    """t = 3, R_F = 8, R_P = 57: the round numbers of a 128-bit instance, 195 constants in LDS"""
    eng, T = engines(lg), 1 << lg
    rnd = random.Random(2000 + lg)
    params = pr.make_params(3, 8, 57, 43)
    run(eng, input_cols(3, T, rnd), params, [{"mode": "row", "in": [0, 1, 2], "out": [0, 2]}])


@pytest.mark.parametrize("t", [2, 3, 4, 8])
def test_an_immediate_in_every_slot_and_one_row_in_two_slots(engines, t):
    """unit p holds an immediate in slot p (0, r - 1 and random ones) and one row in all the others"""
    eng, T = engines(4), 16
    rnd = random.Random(3000 + t)
    params = pr.make_params(t, 2, 1, 50 + t)
    cols = input_cols(2, T, rnd)
    imms = [0, R - 1] + [rnd.randrange(R) for _ in range(t)]
    units = [{"mode": "row", "in": [("imm", imms[p]) if j == p else (j + p) % 2 for j in range(t)], "out": [p, (p + 1) % t]}
             for p in range(t)]
    run(eng, cols, params, units)
    run(eng, cols, params, [{"mode": "row", "in": [("imm", v) for v in imms[:t]], "out": [0]}])   # no row at all


@pytest.mark.parametrize("split", [split_first, split_halves])
def test_inputs_split_over_two_sets(engines, split):
    eng, T = engines(4), 16
    rnd = random.Random(4000)
    params = pr.make_params(4, 2, 1, 60)
    cols = input_cols(6, T, rnd)
    units = [{"mode": "row", "in": [5, 0, 3, 1], "out": [1, 3]}, {"mode": "rounds", "in": [2, 4, 0, ("imm", 9)], "period": 4}]
    run(eng, cols, params, units, sizes=split(6), boundaries=(3, 4, 12))


def test_several_units_fill_sixteen_rows(engines):
    eng, T = engines(4), 16
    before = eng.rows_stats()
    rnd = random.Random(5000)
    params = pr.make_params(4, 2, 1, 61)
    cols = input_cols(4, T, rnd)
    units = [{"mode": "row", "in": [0, 1, 2, 3], "out": [3, 1, 0, 2]}, {"mode": "rounds", "in": [3, 2, 1, 0], "period": 5},
             {"mode": "row", "in": [1, 1, 1, 1], "out": [2]}, {"mode": "rounds", "in": [0, ("imm", 1), 0, 2], "period": 16},
             {"mode": "row", "in": [2, 3, 0, 1], "out": [0, 1, 3]}]
    want, st = run(eng, cols, params, units, boundaries=(4, 5, 9, 10, 14, 15))
    assert len(want) == 16 and st["perms"] == [16, 3, 16, 1, 16]
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- rounds units
@pytest.mark.parametrize("P,blocks", [(5, 3), (16, 1), (17, 0), (7, 2), (1 << 32 - 1, 0)])
def test_rounds_units_at_sixteen_rows(engines, P, blocks):
    """R_F = 2, R_P = 2: P = R + 1 = 5 gives three blocks and a leftover row; P = n one block; P > n none, an all-zero set whose
    commitments are those of zero rows; P = R + 3 = 7 leaves the zero gap behind each block"""
    eng, T = engines(4), 16
    rnd = random.Random(6000 + P % 97)
    params = pr.make_params(3, 2, 2, 62)
    cols = input_cols(3, T, rnd)
    want, st = run(eng, cols, params, [{"mode": "rounds", "in": [0, 1, 2], "period": P}],
                   boundaries=[b * P + d for b in range(blocks + 1) for d in (-1, 0, 4, 5) if 0 <= b * P + d < T])
    assert st["perms"] == [blocks]
    for b in range(blocks):
        assert [want[j][b * P] for j in range(3)] == [cols[j][b * P] for j in range(3)]
        assert [want[j][b * P + 4] for j in range(3)] == pr.permute(params, [cols[j][b * P] for j in range(3)])
        assert all(want[j][r] == 0 for j in range(3) for r in range(b * P + 5, min(b * P + P, T)))
    assert all(want[j][r] == 0 for j in range(3) for r in range(blocks * P, T))
    if not blocks:
        assert want == [[0] * T] * 3


@pytest.mark.parametrize("t", [2, 8])
def test_rounds_units_over_more_than_one_workgroup(engines, t):
    """T = 1024, R = 2, P = 3: 341 blocks and a leftover row -- more than 256 lanes with a lane per block or with t lanes"""
    eng, T = engines(10), 1 << 10
    rnd = random.Random(7000 + t)
    params = pr.make_params(t, 2, 0, 63)
    cols = input_cols(t, T, rnd)
    _, st = run(eng, cols, params, [{"mode": "rounds", "in": list(range(t)), "period": 3}],
                boundaries=(2, 3, 767, 768, 769, 1020, 1021, 1022))
    assert st["perms"] == [341]


# ---------------------------------------------------------------------------------------------------- the usable layout
@pytest.mark.parametrize("lg,u", [(4, 13), (10, (1 << 10) - 31)])
def test_usable_layout_with_garbage_behind(engines, lg, u):
    """rows at and behind `usable` hold values that would show in the result were they read; P = 5 and P = 6 cut a block at
    `usable` (13 = 2 * 5 + 3, 993 = 165 * 6 + 3): it is not started, its rows are 0, and the tail follows"""
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(8000 + lg)
    params = pr.make_params(3, 2, 2, 64)
    cols = input_cols(3, T, rnd)
    for c in cols:
        c[u:] = [R - 1 - t for t in range(T - u)]
    P = 5 if lg == 4 else 6
    units = [{"mode": "row", "in": [0, 1, 2], "out": [2, 0]}, {"mode": "rounds", "in": [2, 1, 0], "period": P},
             {"mode": "row", "in": [0, 1, 2], "out": [1], "expect": [0]}]
    tail = [rnd.randrange(R) for _ in range(5 * (T - u))]
    last = (u // P) * P
    want, st = run(eng, cols, params, units, u, tail, boundaries=(last - 1, last, last + 4, last + 5, u - 1, u, u + 1))
    assert st["perms"] == [u, u // P, u] and st["mismatch"][2] == u
    assert all(want[c][u:] == tail[c * (T - u):(c + 1) * (T - u)] for c in range(5))
    assert u % P and all(want[2 + j][r] == 0 for j in range(3) for r in range(last, u))
    _, st = run(eng, cols, params, units)
    assert st["perms"] == [T, T // P, T]
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- checks
@pytest.mark.parametrize("lg", [4, 9])
def test_checks_count_the_rows_that_differ_and_find_the_smallest(engines, lg):
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(9000 + lg)
    params = pr.make_params(3, 2, 1, 65)
    cols = input_cols(3, T, rnd)
    h, _ = pr.columns(cols, params, [{"mode": "row", "in": [0, 1, 2], "out": [2, 0]}])
    u = T - 3
    planted = {"none": [], "row0": [0], "last": [T - 1], "second_wg": [T - 2, 300 % T], "behind_usable": [u, T - 1],
               "both_ends": [T - 1, 0, 7]}
    exp = list(cols) + h
    for name, where in planted.items():
        wrong = [list(h[0]), list(h[1])]
        for k, r in enumerate(where):
            wrong[k % 2][r] = (wrong[k % 2][r] + 1) % R
        units = [{"mode": "row", "in": [0, 1, 2], "out": [2, 0], "expect": [3, 4]},
                 {"mode": "row", "in": [0, 1, 2], "out": [0, 2], "expect": [6, 5]},
                 {"mode": "row", "in": [0, 1, 2], "out": [2], "expect": [5]}]
        usable = u if name == "behind_usable" else None
        live = eng.rows_stats()
        S = commit_sets(eng, exp + wrong, (3, 4))
        try:
            inside = eng.rows_stats()
            out, st = eng.commit_poseidon(S, params, units, usable)
            assert out is None and eng.rows_stats() == inside          # a call of checks alone: no set, nothing counted
        finally:
            release(S)
        assert eng.rows_stats() == live
        n = usable or T
        seen = sorted(r for r in set(where) if r < n)
        first = seen[0] if seen else None
        in_col0 = sorted(r for k, r in enumerate(where) if k % 2 == 0 and r < n)
        assert st == {"perms": [n] * 3, "mismatch": [0, len(seen), len(in_col0)],
                      "first_mismatch": [None, first, in_col0[0] if in_col0 else None]}, (name, st)
    assert eng.rows_stats() == before


def test_a_check_beside_committing_units(engines):
    eng, T = engines(4), 16
    rnd = random.Random(9500)
    params = pr.make_params(2, 2, 1, 66)
    cols = input_cols(2, T, rnd)
    h, _ = pr.columns(cols, params, [{"mode": "row", "in": [0, 1], "out": [1]}])
    h[0][11] = 5
    want, st = run(eng, cols + h, params, [{"mode": "row", "in": [0, 1], "out": [1], "expect": [2]},
                                           {"mode": "row", "in": [0, 1], "out": [1]},
                                           {"mode": "rounds", "in": [0, 1], "period": 8}], boundaries=(3, 4, 7, 8, 11))
    assert len(want) == 3 and st["mismatch"] == [1, 0, 0] and st["first_mismatch"] == [11, None, None]


# ---------------------------------------------------------------------------------------------------- end to end
def test_the_round_gate_holds_on_the_committed_trace(engines):
    """t = 2, R_F = 2, R_P = 2, P = 8: the trace from a rounds unit; the caller's fixed columns rc_0, rc_1, q_full, q_partial
    through commit_rows; the helper columns u_i = s_i + rc_i from commit_expr; then the gates
    q_full (M_j0 u_0^5 + M_j1 u_1^5 - s_j[+1]) and q_partial (M_j0 u_0^5 + M_j1 u_1 - s_j[+1]) as commit_expr checks: 0 non-zero
    rows.  With s_0 changed at one row rho = 2 of a block (both neighbours partial rounds) and the trace committed through
    commit_rows: the gate of j = 0 fails at rho = 1 (its s_0[+1]) and at rho = 2 (its u_0), the gate of j = 1 at rho = 2 only"""
    eng, T, P = engines(4), 16, 8
    before = eng.rows_stats()
    rnd = random.Random(10000)
    params = pr.make_params(2, 2, 2, 67)
    M, rc = params["mds"], params["rc"]
    cols = input_cols(2, T, rnd)
    fixed = [[0] * T for _ in range(4)]                                # rc_0, rc_1, q_full, q_partial
    for b in range(T // P):
        for rho in range(4):
            fixed[0][b * P + rho], fixed[1][b * P + rho] = rc[2 * rho], rc[2 * rho + 1]
            fixed[2 if pr.is_full(params, rho) else 3][b * P + rho] = 1
    I, F = commit_sets(eng, cols, (2,)), commit_sets(eng, fixed, (4,))
    TR, st = eng.commit_poseidon(I, params, [{"mode": "rounds", "in": [0, 1], "period": P}])
    assert st["perms"] == [2]
    # rows of a gate call: s_0 s_1 | rc_0 rc_1 q_full q_partial | u_0 u_1
    helper = [([(be(1), [0]), (be(1), [2])],), ([(be(1), [1]), (be(1), [3])],)]
    gates = []
    for q, partial in ((4, False), (5, True)):
        for j in range(2):
            gates.append(([(be(M[2 * j]), [q] + [6] * 5), (be(M[2 * j + 1]), [q] + [7] * (1 if partial else 5)),
                           (be(R - 1), [q, (j, 1)])], True))

    def count(trace_sets):
        U, _, _ = eng.commit_expr(trace_sets + F, helper)
        try:
            none, nonzero, first = eng.commit_expr(trace_sets + F + [U], gates)
            assert none is None
            return nonzero, first
        finally:
            U.release()

    assert count([TR]) == ([0] * 4, [None] * 4)
    rows = read_all(eng, TR)
    rows[0][P + 2] = (rows[0][P + 2] + 1) % R
    BAD = commit_sets(eng, rows, (2,))
    assert count(BAD) == ([0, 0, 2, 1], [None, None, P + 1, P + 2])
    release([TR] + I + F + BAD)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 5
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg, 0)
    rnd = random.Random(11000)
    params = pr.make_params(3, 2, 1, 68)
    cols = input_cols(4, T, rnd)
    units = [{"mode": "row", "in": [0, 1, ("imm", 3)], "out": [1, 0]}, {"mode": "rounds", "in": [2, 3, 0], "period": 4}]
    want, stats = pr.columns(cols, params, units)
    I = commit_sets(eng, cols, (4,))

    def fresh_ok():
        out, got = eng.commit_poseidon(I, params, units)
        try:
            assert got == stats and read_all(eng, out) == want
        finally:
            out.release()

    fresh_ok()
    live = eng.rows_stats()
    lib = _native.load()
    hi = (ctypes.c_uint64 * 1)(I[0].handle)
    c, h = ctypes.create_string_buffer(48 * 16), ctypes.c_uint64(0)
    st = [(ctypes.c_uint64 * 16)() for _ in range(3)]
    par, recs = eng.poseidon_call(params, units)
    IMM = _native.KZG_POSEIDON_IMM

    def raw(recs, par=par, opts=None, n_units=None):
        pp = _native.PoseidonParams(*par)
        arr = (_native.PoseidonUnit * max(len(recs), 1))(*[eng.poseidon_unit_struct(r) for r in recs])
        return lib.kzg_rows_commit_poseidon(eng._h, 1, hi, ctypes.byref(pp), len(recs) if n_units is None else n_units, arr,
                                            ctypes.byref(opts) if opts else None, c, st[0], st[1], st[2], ctypes.byref(h))

    def refused(rc, why):
        msg = lib.kzg_last_error(eng._h)
        assert rc == _native.KZG_E_ARG and msg.startswith(b"poseidon: ") and why in msg, (rc, msg)
        assert eng.rows_stats() == live

    names = ("mode", "flags", "n_out", "period", "in_", "out", "expect", "imm")
    edit = lambda base, **kw: tuple(kw.get(f, v) for f, v in zip(names, base))   # noqa: E731
    row, rnds = recs
    big = R.to_bytes(32, "big")
    z = bytes(32)
    pedit = lambda **kw: tuple(kw.get(f, v) for f, v in zip(("t", "full", "partial", "rc", "mds"), par))   # noqa: E731
    refused(raw([row], pedit(t=1)), b"width t")
    refused(raw([row], pedit(t=9)), b"width t")
    refused(raw([row], pedit(full=3)), b"R_F must be even")
    refused(raw([row], pedit(full=0)), b"R_F")
    refused(raw([row], pedit(full=18)), b"R_F")
    refused(raw([row], pedit(partial=129)), b"R_P")
    refused(raw([row], pedit(rc=par[3][:-32] + big)), b"round constants must be canonical")
    refused(raw([row], pedit(mds=big + par[4][32:])), b"matrix entries must be canonical")
    refused(raw([], n_units=0), b"n_units")
    refused(raw([row] * 9), b"n_units")
    refused(raw([edit(row, mode=0)]), b"unknown mode")
    refused(raw([edit(row, mode=3)]), b"unknown mode")
    refused(raw([edit(row, flags=2)]), b"flags")
    refused(raw([edit(rnds, flags=1)]), b"belongs to ROW units")
    refused(raw([edit(rnds, period=3)]), b"at least R + 1")
    refused(raw([edit(row, period=4)]), b"at least R + 1")
    refused(raw([edit(row, n_out=0)]), b"n_out must be")
    refused(raw([edit(row, n_out=4)]), b"n_out must be")
    refused(raw([edit(rnds, n_out=2)]), b"n_out must be")
    refused(raw([edit(row, out=[3, 0, 0, 0, 0, 0, 0, 0])]), b"below t")
    refused(raw([edit(row, out=[1, 1, 0, 0, 0, 0, 0, 0])]), b"repeated")
    refused(raw([edit(row, in_=[0, 4, IMM, 0, 0, 0, 0, 0])]), b"concatenated rows")
    refused(raw([edit(row, flags=1, expect=[0, 4, 0, 0, 0, 0, 0, 0])]), b"concatenated rows")
    refused(raw([edit(row, imm=[z, z, big] + [z] * 5)]), b"immediates must be canonical")
    refused(raw([edit(row, imm=[z, be(1), be(3)] + [z] * 5)]), b"0 beside a row")
    refused(raw([edit(row, n_out=3, out=[0, 1, 2, 0, 0, 0, 0, 0])] * 6), b"n_out")
    wide = pr.make_params(8, 2, 0, 69)
    wpar, wrecs = eng.poseidon_call(wide, [{"mode": "row", "in": list(range(8)), "out": [0], "expect": [8]}])
    second = edit(wrecs[0], in_=list(range(9, 17)))                    # 8 + 1 + 8 = 17 distinct rows
    refused(raw([wrecs[0], second], wpar), b"distinct input rows")
    tl = b"".join(bt([rnd.randrange(R) for _ in range(5 * 4)]))
    for usable, tail, why in ((T, tl, b"usable must be in"), (T - 4, None, b"tail_be32 must be given"), (0, tl, b"plain layout"),
                              (T - 4, tl[:-32] + big, b"canonical")):
        refused(raw([row, rnds], opts=_native.DeriveOpts(usable, tail)), why)
    fresh_ok()
    assert raw([edit(row, imm=[z, z, be(R - 1)] + [z] * 5)]) == 0      # the largest immediate that is canonical
    eng.release_rows(h.value)
    for bad, why in ((dict(units[0], mode="sponge"), "unknown mode"), (dict(units[0], out=[3]), "out index"),
                     (dict(units[0], out=[1, 1]), "repeated"), (dict(units[1], period=3), "period P"),
                     (dict(units[1], expect=[0, 1, 2]), "expect belongs"), (dict(units[0], **{"in": [0, 4, 1]}), "concatenated rows"),
                     (dict(units[0], **{"in": [0, 1, ("imm", R)]}), "canonical"), (dict(units[0], foo=1), "unknown field")):
        arg_error(lambda: eng.commit_poseidon(I, params, [bad]), why)
    arg_error(lambda: eng.commit_poseidon(I, dict(params, full=3), units), "R_F must be even")
    arg_error(lambda: eng.commit_poseidon(I, dict(params, rc=[R] + params["rc"][1:]), units), "canonical")
    arg_error(lambda: eng.commit_poseidon(I, params, units, None, [be(1)]), "tail")
    arg_error(lambda: eng.commit_poseidon([2 ** 40], params, units), "unknown")
    fresh_ok()
    release(I)
    assert eng.rows_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------------- routing
def test_client_and_multi_device_client_return_the_engine_bytes(hip):
    from zkp_subnet_amd import Client, MultiDeviceClient, codec

    scale, ms = 6, 0
    T = 1 << scale
    rnd = random.Random(12000)
    params = pr.make_params(3, 2, 2, 70)
    cols = input_cols(3, T, rnd)
    units = [{"mode": "row", "in": [0, ["imm", str(R - 1)], 2], "out": [1, 0]}, {"mode": "rounds", "in": [2, 1, 0], "period": 9}]
    want, stats = pr.columns(cols, params, units)
    wire = dict(params, rc=[hex(v) for v in params["rc"]], mds=[str(v) for v in params["mds"]])
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    for client in (Client(seed=83), MultiDeviceClient(devices=[0], seed=83)):
        client.start(scale=scale, machines_scale=ms)
        try:
            a = client.worker_commit_rows(0, [fr(col) for col in cols]).json()["handle"]
            ref = client.worker_commit_rows(0, [fr(col) for col in want]).json()
            r = client.worker_commit_poseidon([a], wire, units)
            assert r.status_code == 200, r.json()
            body = r.json()
            assert body["commitments"] == ref["commitments"]
            assert {k: body[k] for k in stats} == stats
            chk = client.worker_commit_poseidon([a, ref["handle"]], wire, [dict(units[0], expect=[3, 4]),
                                                                          dict(units[0], expect=[4, 3])])
            assert chk.status_code == 200, chk.json()
            assert chk.json()["handle"] is None and chk.json()["commitments"] == []
            assert chk.json()["mismatch"][0] == 0 and chk.json()["first_mismatch"] == [None, 0]
            assert client.worker_commit_poseidon([a], wire, [dict(units[0], mode="sponge")]).status_code == 400
            assert client.worker_commit_poseidon([a], dict(wire, full=3), units).status_code == 400
            assert client.worker_commit_poseidon([a], wire, units, None, fr([1])).status_code == 400
            for hh in (ref["handle"], body["handle"], a):
                assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_poseidon([a], wire, units).status_code == 400
        finally:
            client.stop()
