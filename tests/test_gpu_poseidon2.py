"""GPU tests (`-m gpu`) of kzg_rows_commit_poseidon2: the Poseidon2 permutation (x^5, the caller's constants) of resident rows,
one per row, as a check against expected rows, or as the round trace in blocks of P >= R + 2 rows, computed and committed on the
device.  The expected rows come from the definition in Python integers (tests/poseidon2_ref.py), which
tests/test_poseidon2_cpu.py pins by identities: no published known-answer vector is available here.  Every committed set is
compared three ways: its commitments byte for byte against commit_rows of the reference rows, its evaluations at domain points
(the first, the last and the block-boundary rows) through eval_rows, and its cells through read_rows."""
import ctypes
import random

import pytest

from tests import grand_product_ref as gp
from tests import poseidon2_ref as p2
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x905E1D21, 0x905E1D22


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
    want, stats = p2.columns(cols, params, units, usable, tail)
    T = len(cols[0])
    S = commit_sets(eng, cols, sizes or (len(cols),))
    try:
        out, got = eng.commit_poseidon2(S, params, units, usable, bt(tail))
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
    """every state element out, in reversed order; T = 512 runs two workgroups of 256 lanes"""
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(1000 * t + 10 * partial + lg)
    params = p2.make_params(t, full, partial, 40 + t)
    cols = input_cols(t, T, rnd)
    _, st = run(eng, cols, params, [{"mode": "row", "in": list(range(t)), "out": list(reversed(range(t)))}])
    assert st["perms"] == [T]
    assert eng.rows_stats() == before


@pytest.mark.parametrize("t,full,partial", [(3, 8, 56), (8, 8, 57)])
def test_row_unit_at_the_real_round_numbers(engines, t, full, partial):
    eng, T = engines(4), 16
    rnd = random.Random(2000 + t)
    params = p2.make_params(t, full, partial, 43)
    run(eng, input_cols(t, T, rnd), params, [{"mode": "row", "in": list(range(t)), "out": [0, t - 1]}])


@pytest.mark.parametrize("t", [2, 3, 4, 8])
def test_an_immediate_in_every_slot_and_one_row_in_two_slots(engines, t):
    """unit p holds an immediate in slot p and one row in all the others; the t + 2 immediates are 0, r - 1 and t random ones,
    and t more units walk the list on, so that every slot sees 0, r - 1 and a random one at every t (t = 2 included)"""
    eng, T = engines(4), 16
    rnd = random.Random(3000 + t)
    params = p2.make_params(t, 2, 1, 50 + t)
    cols = input_cols(2, T, rnd)
    imms = [0, R - 1] + [rnd.randrange(R) for _ in range(t)]
    units = [{"mode": "row", "in": [("imm", imms[p]) if j == p else (j + p) % 2 for j in range(t)], "out": [p, (p + 1) % t]}
             for p in range(t)]
    run(eng, cols, params, units)
    for shift in (1, 2):                                       # slot p now holds imms[p + shift]: r - 1 or a random one, then random
        more = [{"mode": "row", "in": [("imm", imms[(p + shift) % (t + 2)]) if j == p else (j + p) % 2 for j in range(t)], "out": [p]}
                for p in range(t)]
        run(eng, cols, params, more)
    for k in (0, 2):                                           # no row at all: (0, r - 1, ..), then random ones only
        run(eng, cols, params, [{"mode": "row", "in": [("imm", imms[(k + j) % (t + 2)]) for j in range(t)], "out": [0]}])


def test_eight_units_in_one_call(engines):
    """row units, a check and rounds units with different periods side by side: 3 + 4 + 1 + 0 + 4 + 2 + 1 + 1 = 16 columns"""
    eng, T = engines(5), 32
    before = eng.rows_stats()
    rnd = random.Random(5000)
    params = p2.make_params(4, 2, 1, 61)
    cols = input_cols(4, T, rnd)
    h, _ = p2.columns(cols, params, [{"mode": "row", "in": [0, 1, 2, 3], "out": [2]}])
    units = [{"mode": "row", "in": [0, 1, 2, 3], "out": [3, 1, 0]}, {"mode": "rounds", "in": [3, 2, 1, 0], "period": 5},
             {"mode": "row", "in": [1, 1, 1, 1], "out": [2]}, {"mode": "row", "in": [0, 1, 2, 3], "out": [2], "expect": [4]},
             {"mode": "rounds", "in": [0, ("imm", 1), 0, 2], "period": 32}, {"mode": "row", "in": [2, 3, 0, 1], "out": [0, 1]},
             {"mode": "row", "in": [("imm", R - 1), 3, 0, 1], "out": [3]}, {"mode": "row", "in": [3, 3, 0, 0], "out": [1]}]
    want, st = run(eng, cols + h, params, units, boundaries=(4, 5, 9, 10, 29, 30))
    assert len(want) == 16 and st["perms"] == [32, 6, 32, 32, 1, 32, 32, 32] and st["mismatch"] == [0] * 8
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- rounds units
@pytest.mark.parametrize("P,blocks", [(6, 2), (16, 1), (17, 0), (7, 2), (1 << 32 - 1, 0)])
def test_rounds_units_at_sixteen_rows(engines, P, blocks):
    """R_F = 2, R_P = 2: P = R + 2 = 6 gives two blocks and four leftover rows; P = n one block; P > n none, an all-zero set;
    P = 7 does not divide T and leaves the zero gap behind each block"""
    eng, T = engines(4), 16
    rnd = random.Random(6000 + P % 97)
    params = p2.make_params(3, 2, 2, 62)
    cols = input_cols(3, T, rnd)
    want, st = run(eng, cols, params, [{"mode": "rounds", "in": [0, 1, 2], "period": P}],
                   boundaries=[b * P + d for b in range(blocks + 1) for d in (-1, 0, 1, 5, 6) if 0 <= b * P + d < T])
    assert st["perms"] == [blocks]
    for b in range(blocks):
        s = [cols[j][b * P] for j in range(3)]
        assert [want[j][b * P] for j in range(3)] == s
        assert [want[j][b * P + 1] for j in range(3)] == p2.external(3, s)
        assert [want[j][b * P + 5] for j in range(3)] == p2.permute(params, s)
        assert all(want[j][r] == 0 for j in range(3) for r in range(b * P + 6, min(b * P + P, T)))
    assert all(want[j][r] == 0 for j in range(3) for r in range(blocks * P, T))
    if not blocks:
        assert want == [[0] * T] * 3


@pytest.mark.parametrize("t", [2, 8])
def test_rounds_units_over_more_than_one_workgroup(engines, t):
    """a row unit beside a rounds unit: T = 512, R = 2, P = R + 2 = 4 gives 128 blocks, the row unit 512 lanes, so the rounds
    unit's second workgroup leaves at once (P >= 4 allows no more than 128 blocks at 2^9 rows: the case of more than 256 blocks
    is the next test, at 2^11)"""
    eng, T = engines(9), 1 << 9
    rnd = random.Random(7000 + t)
    params = p2.make_params(t, 2, 0, 63)
    cols = input_cols(t, T, rnd)
    _, st = run(eng, cols, params, [{"mode": "rounds", "in": list(range(t)), "period": 4},
                                    {"mode": "row", "in": list(reversed(range(t))), "out": [0]}],
                boundaries=(3, 4, 5, 255, 256, 257, 508, 509))
    assert st["perms"] == [128, T]


def test_rounds_units_with_more_than_256_blocks(engines):
    """T = 2^11, R = 2, P = 5: 409 blocks and three leftover rows -- two workgroups of lanes with one lane per block"""
    eng, T = engines(11), 1 << 11
    rnd = random.Random(7100)
    params = p2.make_params(3, 2, 0, 64)
    cols = input_cols(3, T, rnd)
    _, st = run(eng, cols, params, [{"mode": "rounds", "in": [0, 1, 2], "period": 5}],
                boundaries=(4, 5, 1279, 1280, 1281, 2044, 2045, 2046))
    assert st["perms"] == [409]


# ---------------------------------------------------------------------------------------------------- the usable layout
@pytest.mark.parametrize("lg,u,n_tail", [(4, 15, None), (6, 13, "most")])
def test_usable_layout_with_garbage_behind(engines, lg, u, n_tail):
    """usable = T - 1, and a small usable with the largest tail the layout allows (KZG_MAX_BLIND_ROWS rows at and behind
    usable); rows at and behind `usable` hold values that would show in the result were they read"""
    eng, T = engines(lg), 1 << lg
    if n_tail == "most":
        u = T - _native.KZG_MAX_BLIND_ROWS
    before = eng.rows_stats()
    rnd = random.Random(8000 + lg)
    params = p2.make_params(3, 2, 2, 64)
    cols = input_cols(3, T, rnd)
    for c in cols:
        c[u:] = [R - 1 - t for t in range(T - u)]
    P = 6 if u % 6 else 7
    units = [{"mode": "row", "in": [0, 1, 2], "out": [2, 0]}, {"mode": "rounds", "in": [2, 1, 0], "period": P},
             {"mode": "row", "in": [0, 1, 2], "out": [1], "expect": [0]}]
    tail = [rnd.randrange(R) for _ in range(5 * (T - u))]
    last = (u // P) * P
    want, st = run(eng, cols, params, units, u, tail, boundaries=(last - 1, last, last + 5, last + 6, u - 1, u, u + 1))
    assert st["perms"] == [u, u // P, u] and st["mismatch"][2] == u
    assert all(want[c][u:] == tail[c * (T - u):(c + 1) * (T - u)] for c in range(5))
    assert u % P and all(want[2 + j][r] == 0 for j in range(3) for r in range(last, u))
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- checks
@pytest.mark.parametrize("lg", [4, 9])
def test_checks_count_the_rows_that_differ_and_find_the_smallest(engines, lg):
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(9000 + lg)
    params = p2.make_params(3, 2, 1, 65)
    cols = input_cols(3, T, rnd)
    h, _ = p2.columns(cols, params, [{"mode": "row", "in": [0, 1, 2], "out": [2, 0]}])
    planted = {"none": [], "row0": [0], "last": [T - 1], "second_wg": [T - 2, 256 % T], "both_ends": [T - 1, 0, 7]}
    exp = list(cols) + h
    for name, where in planted.items():
        wrong = [list(h[0]), list(h[1])]
        for k, r in enumerate(where):
            wrong[k % 2][r] = (wrong[k % 2][r] + 1) % R
        units = [{"mode": "row", "in": [0, 1, 2], "out": [2, 0], "expect": [3, 4]},
                 {"mode": "row", "in": [0, 1, 2], "out": [0, 2], "expect": [6, 5]},
                 {"mode": "row", "in": [0, 1, 2], "out": [2], "expect": [5]}]
        live = eng.rows_stats()
        S = commit_sets(eng, exp + wrong, (3, 4))
        try:
            inside = eng.rows_stats()
            out, st = eng.commit_poseidon2(S, params, units)
            assert out is None and eng.rows_stats() == inside          # a call of checks alone: no set, nothing counted
        finally:
            release(S)
        assert eng.rows_stats() == live
        seen = sorted(set(where))
        in_col0 = sorted(r for k, r in enumerate(where) if k % 2 == 0)
        assert st == {"perms": [T] * 3, "mismatch": [0, len(seen), len(in_col0)],
                      "first_mismatch": [None, seen[0] if seen else None, in_col0[0] if in_col0 else None]}, (name, st)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the tie
def test_the_degenerate_tie_to_commit_poseidon_on_the_device(engines):
    """t = 3, diag = 1 (I = E): commit_poseidon2 of the input columns equals commit_poseidon, with mds the dense E and rc the
    merged constants, of the E-image columns, commitment for commitment"""
    eng, T = engines(4), 16
    rnd = random.Random(9700)
    params = dict(p2.make_params(3, 2, 2, 66), diag=[1, 1, 1])
    half = 3
    rc = params["rc_full"][:half] + [v for c in params["rc_partial"] for v in (c, 0, 0)] + params["rc_full"][half:]
    tied = {"t": 3, "full": 2, "partial": 2, "rc": rc, "mds": p2.dense_external(3)}
    cols = input_cols(3, T, rnd)
    image = [list(c) for c in zip(*[p2.external(3, [cols[j][r] for j in range(3)]) for r in range(T)])]
    unit = [{"mode": "row", "in": [0, 1, 2], "out": [0, 1, 2]}]
    A, B = commit_sets(eng, cols, (3,)), commit_sets(eng, image, (3,))
    try:
        x, _ = eng.commit_poseidon2(A, params, unit)
        y, _ = eng.commit_poseidon(B, tied, unit)
        try:
            assert x.commitments == y.commitments and read_all(eng, x) == read_all(eng, y)
        finally:
            x.release()
            y.release()
    finally:
        release(A + B)


# ---------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 5
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg + 1, 1)           # two workers
    rnd = random.Random(11000)
    params = p2.make_params(3, 2, 1, 68)
    cols = input_cols(4, T, rnd)
    units = [{"mode": "row", "in": [0, 1, ("imm", 3)], "out": [1, 0]}, {"mode": "rounds", "in": [2, 3, 0], "period": 5}]
    want, stats = p2.columns(cols, params, units)
    I = commit_sets(eng, cols, (4,))

    def fresh_ok():
        out, got = eng.commit_poseidon2(I, params, units)
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
    par, recs = eng.poseidon2_call(params, units)
    IMM = _native.KZG_POSEIDON_IMM

    def raw(recs, par=par, opts=None, n_units=None, handles=hi):
        pp = _native.Poseidon2Params(*par)
        arr = (_native.PoseidonUnit * max(len(recs), 1))(*[eng.poseidon_unit_struct(r) for r in recs])
        return lib.kzg_rows_commit_poseidon2(eng._h, len(handles), handles, ctypes.byref(pp), len(recs) if n_units is None else n_units,
                                             arr, ctypes.byref(opts) if opts else None, c, st[0], st[1], st[2], ctypes.byref(h))

    def refused(rc, why):
        msg = lib.kzg_last_error(eng._h)
        assert rc == _native.KZG_E_ARG and msg.startswith(b"poseidon2: ") and why in msg, (rc, msg)
        assert eng.rows_stats() == live

    names = ("mode", "flags", "n_out", "period", "in_", "out", "expect", "imm")
    edit = lambda base, **kw: tuple(kw.get(f, v) for f, v in zip(names, base))   # noqa: E731
    row, rnds = recs
    big = R.to_bytes(32, "big")
    z = bytes(32)
    pedit = lambda **kw: tuple(kw.get(f, v) for f, v in zip(("t", "full", "partial", "rc_full", "rc_partial", "diag"), par))   # noqa: E731
    for t in (0, 1, 5, 6, 7, 9, 33):
        refused(raw([row], pedit(t=t)), b"the width t must be 2, 3, 4 or 8")
    refused(raw([row], pedit(full=3)), b"R_F must be even")
    refused(raw([row], pedit(full=0)), b"R_F")
    refused(raw([row], pedit(full=18)), b"R_F")
    refused(raw([row], pedit(partial=129)), b"R_P")
    refused(raw([row], pedit(rc_partial=None)), b"must not be null")
    refused(raw([row], pedit(rc_full=par[3][:-32] + big)), b"round constants must be canonical")
    refused(raw([row], pedit(rc_partial=big)), b"round constants must be canonical")
    refused(raw([row], pedit(diag=big + par[5][32:])), b"diagonal entries must be canonical")
    refused(raw([], n_units=0), b"n_units")
    refused(raw([row] * 9), b"n_units")
    refused(raw([edit(row, mode=0)]), b"unknown mode")
    refused(raw([edit(row, flags=2)]), b"flags")
    refused(raw([edit(rnds, flags=1)]), b"belongs to ROW units")
    refused(raw([edit(rnds, period=4)]), b"at least R + 2")
    refused(raw([edit(row, period=5)]), b"at least R + 2")
    refused(raw([edit(row, n_out=0)]), b"n_out must be")
    refused(raw([edit(rnds, n_out=2)]), b"n_out must be")
    refused(raw([edit(row, out=[3, 0, 0, 0, 0, 0, 0, 0])]), b"below t")
    refused(raw([edit(row, out=[1, 1, 0, 0, 0, 0, 0, 0])]), b"repeated")
    refused(raw([edit(row, in_=[0, 4, IMM, 0, 0, 0, 0, 0])]), b"concatenated rows")
    refused(raw([edit(row, flags=1, expect=[0, 4, 0, 0, 0, 0, 0, 0])]), b"concatenated rows")
    refused(raw([edit(row, imm=[z, z, big] + [z] * 5)]), b"immediates must be canonical")
    refused(raw([edit(row, imm=[z, be(1), be(3)] + [z] * 5)]), b"0 beside a row")
    refused(raw([edit(row, n_out=3, out=[0, 1, 2, 0, 0, 0, 0, 0])] * 6), b"n_out")          # 18 outputs
    wide = p2.make_params(8, 2, 0, 69)
    wpar, wrecs = eng.poseidon2_call(wide, [{"mode": "row", "in": list(range(8)), "out": [0], "expect": [8]}])
    second = edit(wrecs[0], in_=list(range(9, 17)))                    # 8 + 1 + 8 = 17 distinct rows
    refused(raw([wrecs[0], second], wpar), b"distinct input rows")
    tl = b"".join(bt([rnd.randrange(R) for _ in range(5 * 4)]))
    for usable, tail, why in ((T, tl, b"usable must be in"), (T - 4, None, b"tail_be32 must be given"), (0, tl, b"plain layout"),
                              (T - 4, tl[:-32] + big, b"canonical")):
        refused(raw([row, rnds], opts=_native.DeriveOpts(usable, tail)), why)
    fresh_ok()
    assert raw([edit(row, imm=[z, z, be(R - 1)] + [z] * 5)]) == 0      # the largest immediate that is canonical
    eng.release_rows(h.value)
    other = commit_sets(eng, cols[1:3], (2,), i=1)                     # another worker's handle
    arg_error(lambda: eng.commit_poseidon2([I[0]] + other, params, units), "one worker")
    release(other)
    for bad, why in ((dict(units[0], mode="sponge"), "unknown mode"), (dict(units[0], out=[3]), "out index"),
                     (dict(units[1], period=4), "period P"), (dict(units[0], **{"in": [0, 4, 1]}), "concatenated rows"),
                     (dict(units[0], **{"in": [0, 1, ("imm", R)]}), "canonical"), (dict(units[0], foo=1), "unknown field")):
        arg_error(lambda: eng.commit_poseidon2(I, params, [bad]), why)
    arg_error(lambda: eng.commit_poseidon2(I, dict(params, t=5), units), "width t")
    arg_error(lambda: eng.commit_poseidon2(I, dict(params, diag=[R] + params["diag"][1:]), units), "canonical")
    arg_error(lambda: eng.commit_poseidon2(I, params, units, None, [be(1)]), "tail")
    arg_error(lambda: eng.commit_poseidon2([2 ** 40], params, units), "unknown")
    fresh_ok()
    release(I)
    assert eng.rows_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------------- routing
def test_client_and_multi_device_client_return_the_engine_bytes(hip):
    from zkp_subnet_amd import Client, MultiDeviceClient, codec

    scale, ms = 6, 0
    T = 1 << scale
    rnd = random.Random(12000)
    params = p2.make_params(3, 2, 2, 70)
    cols = input_cols(3, T, rnd)
    units = [{"mode": "row", "in": [0, ["imm", str(R - 1)], 2], "out": [1, 0]}, {"mode": "rounds", "in": [2, 1, 0], "period": 9}]
    want, stats = p2.columns(cols, params, units)
    wire = dict(params, rc_full=[hex(v) for v in params["rc_full"]], diag=[str(v) for v in params["diag"]])
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    for client in (Client(seed=83), MultiDeviceClient(devices=[0], seed=83)):
        client.start(scale=scale, machines_scale=ms)
        try:
            a = client.worker_commit_rows(0, [fr(col) for col in cols]).json()["handle"]
            ref = client.worker_commit_rows(0, [fr(col) for col in want]).json()
            r = client.worker_commit_poseidon2([a], wire, units)
            assert r.status_code == 200, r.json()
            body = r.json()
            assert body["commitments"] == ref["commitments"]
            assert {k: body[k] for k in stats} == stats
            chk = client.worker_commit_poseidon2([a, ref["handle"]], wire, [dict(units[0], expect=[3, 4]),
                                                                           dict(units[0], expect=[4, 3])])
            assert chk.status_code == 200, chk.json()
            assert chk.json()["handle"] is None and chk.json()["commitments"] == []
            assert chk.json()["mismatch"][0] == 0 and chk.json()["first_mismatch"] == [None, 0]
            assert client.worker_commit_poseidon2([a], wire, [dict(units[0], mode="sponge")]).status_code == 400
            assert client.worker_commit_poseidon2([a], dict(wire, t=5), units).status_code == 400
            assert client.worker_commit_poseidon2([a], wire, [dict(units[1], period=5)]).status_code == 400
            assert client.worker_commit_poseidon2([a], wire, units, None, fr([1])).status_code == 400
            for hh in (ref["handle"], body["handle"], a):
                assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_poseidon2([a], wire, units).status_code == 400
        finally:
            client.stop()
