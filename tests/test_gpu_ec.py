"""GPU tests (`-m gpu`) of kzg_rows_commit_ec: a b^-1 mod p, the affine point addition with the doubling and the accumulator trace
of a chain, over an odd modulus that is not the scalar field, computed and committed on the device.  The expected rows come
from the definition in Python integers (tests/ec_ref.py), which tests/test_ec_cpu.py pins against the group law of secp256k1.
Every committed set is compared with commit_rows of the reference rows byte for byte and cell by cell through read_rows."""
import ctypes
import random

import pytest

from tests import ec_ref as er
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x0EC0A601, 0x0EC0A602
CURVES = {
    "secp256k1": er.SECP,
    "b32x4": {"bits": 32, "limbs": 4, "p": 2**128 - 159, "a": 5},
    "b52x4": {"bits": 52, "limbs": 4, "p": 2**200 - 75, "a": 2**199 + 12345},
    "m61": {"bits": 64, "limbs": 1, "p": 2**61 - 1, "a": 2**61 - 4},
    "p251": {"bits": 8, "limbs": 1, "p": 251, "a": 3},
}


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


def read_all(eng, rset):
    out = []
    for c in range(rset.k):
        raw = eng.read_rows([rset], c, 0, rset.T, "fr")[0]
        out.append([int.from_bytes(raw[32 * t:32 * t + 32], "big") for t in range(rset.T)])
    return out


def run(eng, cols, curve, units, usable=None, tail=(), sizes=None):
    """commit `cols`, build on the device, compare statistics, commitments and cells with the reference; returns (rows, stats)"""
    want, stats = er.columns(cols, curve, units, usable, tail)
    T = len(cols[0])
    S = commit_sets(eng, cols, sizes or (len(cols),))
    try:
        inside = eng.rows_stats()
        out, got = eng.commit_ec(S, curve, units, usable, bt(tail))
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
            assert read_all(eng, out) == want
        finally:
            out.release()
    finally:
        release(S)
    return want, stats


def wide_cols(values, curve):
    """the L limb columns of a list of values below 2^W"""
    return er.wide_rows(values, curve)


def operands(k, T, curve, rnd):
    """k wide operands of T random values below p, as k L columns"""
    return [c for _ in range(k) for c in wide_cols([rnd.randrange(curve["p"]) for _ in range(T)], curve)]


def add_unit(L, **kw):
    return dict({"mode": "add", "x1": 0, "y1": L, "x2": 2 * L, "y2": 3 * L, "out": ["lam", "x3", "y3"]}, **kw)


def plant_points(cols, curve, rnd):
    """rows 1 .. 4 of four operand runs: equal points, opposite points, a point of order two doubled, equal x and other y"""
    L, p = curve["limbs"], curve["p"]
    x, y = rnd.randrange(p), rnd.randrange(1, p)
    for t, (x2, y2, y1) in enumerate([(x, y, y), (x, p - y, y), (x, 0, 0), (x, (y + 1) % p, y)], start=1):
        for w, v in enumerate((x, y1, x2, y2)):
            for l, limb in enumerate(er.limbs(v, curve)):
                cols[w * L + l][t] = limb


# ---------------------------------------------------------------------------------------------------- add and div: sizes, curves
@pytest.mark.parametrize("name,lg,usable", [("secp256k1", 8, None), ("secp256k1", 9, None), ("secp256k1", 8, 230), ("secp256k1", 9, 490),
                                            ("b32x4", 8, None), ("b52x4", 8, 230), ("m61", 8, None), ("m61", 9, 490), ("p251", 8, None),
                                            ("p251", 8, 230)])
def test_add_and_div_over_every_limb_shape(engines, name, lg, usable):
    """T = 256 and 512, plain and with usable = 230 and 490 (a full and a partial workgroup, the tail behind): the addition with
    all three outputs and, in the same call, the division of x1 by x2 where the rows fit (L = 1); L = 4 takes the division in
    a call of its own over the same rows, which serve both"""
    eng, T, curve = engines(lg), 1 << lg, CURVES[name]
    L = curve["limbs"]
    rnd = random.Random(lg * 1000 + (usable or 0) + L)
    cols = operands(4, T, curve, rnd)
    plant_points(cols, curve, rnd)
    div = {"mode": "div", "a": 0, "b": 2 * L, "out": True}
    calls = [[add_unit(L), div]] if L == 1 else [[add_unit(L), div], [dict(div, a=3 * L, b=L), add_unit(L, out=["y3", "lam"])]]
    for units in calls:
        n_out = sum((len(u["out"]) if u["mode"] == "add" else 1) * L for u in units)
        tail = [rnd.randrange(R) for _ in range(n_out * (T - usable))] if usable else ()
        want, st = run(eng, cols, curve, units, usable, tail, sizes=(L, 3 * L))
        assert st["counts"] == [0] * len(units) and len(want) == n_out
        k = [u["mode"] for u in units].index("add")
        assert st["singular"][k] >= 3 and st["first_singular"][k] <= 2   # the planted rows 2, 3 and 4


def test_sixteen_output_rows_of_four_units(engines):
    """four units in one call, 16 output rows: two additions over 52-bit limbs of L = 2 with two names each, a division and a
    chain with its three columns"""
    eng, T = engines(8), 256
    curve = {"bits": 52, "limbs": 2, "p": 2**104 - 17, "a": 7}
    rnd = random.Random(77)
    cols = operands(4, T, curve, rnd) + [[rnd.choice([0, 1, 2, 3]) for _ in range(T)]]
    plant_points(cols, curve, rnd)
    units = [add_unit(2, out=["x3", "y3"]), {"mode": "div", "a": 2, "b": 6, "out": True},
             {"mode": "chain", "px": 0, "py": 2, "op": 8, "cols": ["ax", "ay", "lam"]}, add_unit(2, x2=0, y2=2, out=["lam", "y3"])]
    want, st = run(eng, cols, curve, units, sizes=(4, 5))
    assert len(want) == 16 and st["segments"][2] == len({0} | {t for t in range(T) if cols[8][t] == 1})


# ---------------------------------------------------------------------------------------------------- a tiny curve, exhaustively
def test_every_pair_of_points_of_a_tiny_curve(engines):
    """y^2 = x^3 + x + 11 over p = 13 has a point with y = 0 (x = 1).  Every ordered pair of its affine points in one column:
    equal points, opposite points, the point of order two and x1 = x2 all occur; every row that is not exceptional lands on the
    curve again"""
    p, a, c = 13, 1, 11
    curve = {"bits": 8, "limbs": 1, "p": p, "a": a}
    pts = [(x, y) for x in range(p) for y in range(p) if (y * y - x * x * x - a * x - c) % p == 0]
    assert (1, 0) in pts and len(pts) ** 2 <= 512
    pairs = [(P, Q) for P in pts for Q in pts]
    T = 512
    pad = [((0, 0), (0, 0))] * (T - len(pairs))
    cols = [[pq[i][j] for pq in pairs + pad] for i in (0, 1) for j in (0, 1)]
    want, st = run(engines(9), cols, curve, [add_unit(1)])
    on = 0
    for t, (P, Q) in enumerate(pairs):
        lam, x3, y3 = want[0][t], want[1][t], want[2][t]
        opposite = P[0] == Q[0] and (P[1] + Q[1]) % p == 0
        if opposite:
            assert (lam, x3, y3) == (0, 0, 0)
        else:
            assert (y3 * y3 - x3 * x3 * x3 - a * x3 - c) % p == 0
            on += 1
    assert st["singular"][0] == len(pairs) - on + len(pad) and on > 0 and st["counts"] == [0]


# ---------------------------------------------------------------------------------------------------- singular rows, extremes
def test_planted_denominators_without_an_inverse_under_a_composite_modulus(engines):
    q = 2**32 + 15
    p = 15 * q
    curve = {"bits": 18, "limbs": 2, "p": p, "a": 1}
    assert p < 2**36
    rnd = random.Random(5)
    T = 256
    vals = [[rnd.randrange(p) for _ in range(T)] for _ in range(4)]
    for t, d in enumerate([3, 5, 15, q, 3 * q, 0, 9, 25, p - 3], start=7):
        vals[2][t] = (vals[0][t] + d) % p   # x2 - x1 = d
        vals[3][t] = d                      # the divisor of the div unit below
    cols = [c for v in vals for c in wide_cols(v, curve)]
    units = [add_unit(2), {"mode": "div", "a": 0, "b": 6, "out": True}]
    want, st = run(engines(8), cols, curve, units)
    import math
    assert st["singular"][1] == sum(math.gcd(v, p) != 1 for v in vals[3]) >= 9 and st["first_singular"][0] <= 7
    assert all(want[6][t] == 0 and want[7][t] == 0 for t in range(7, 16))


@pytest.mark.parametrize("name", ["secp256k1", "p251", "b52x4"])
def test_extreme_operands(engines, name):
    """0, 1, p - 1, p, 2^W - 1 in every combination of two operands, and limbs at or above 2^b: reduced, and the row counted once"""
    curve = CURVES[name]
    b, L, p = curve["bits"], curve["limbs"], curve["p"]
    W = b * L
    ext = [0, 1, p - 1, p, min(p + 1, 2**W - 1), 2**W - 1]
    T = 64
    rnd = random.Random(9)
    pairs = [(u, v) for u in ext for v in ext]
    vals = [[pairs[t][0] if t < 36 else rnd.randrange(p) for t in range(T)], [pairs[t][1] if t < 36 else rnd.randrange(p) for t in range(T)]]
    cols = [c for v in vals for c in wide_cols(v, curve)]
    for t, (l, extra) in enumerate([(0, 1 << b), (L - 1, 1 << 64), (L, (1 << 200) + 5), (2 * L - 1, ((R - 1) >> b << b) - (1 << b))], start=40):
        cols[l][t] += extra   # a limb at or above 2^b, the last one just below r: the cell stays canonical
        assert cols[l][t] < R
    units = [{"mode": "div", "a": 0, "b": L, "out": True}, add_unit(L, x1=0, y1=L, x2=L, y2=0, out=["x3"]),
             add_unit(L, x1=0, y1=L, x2=0, y2=L, out=["lam"])]
    want, st = run(engines(6), cols, curve, units)
    over = sum(u >= p or v >= p for u, v in pairs) + 4
    assert st["counts"] == [over] * 3 and st["first"] == [3] * 3


def test_immediates_for_b(engines):
    curve = CURVES["secp256k1"]
    p = curve["p"]
    cols = operands(1, 64, curve, random.Random(11))
    for imm in (1, 2, p - 1, p + 2, 2**256 - 1):
        want, st = run(engines(6), cols, curve, [{"mode": "div", "a": 0, "b": ("imm", imm), "out": True}])
        assert st["counts"] == [0] and st["singular"] == [0]
        x = sum(want[l][5] << (64 * l) for l in range(4))
        assert x * imm % p == sum(cols[l][5] << (64 * l) for l in range(4))
    for imm in (0, p):
        want, st = run(engines(6), cols, curve, [{"mode": "div", "a": 0, "b": ("imm", imm), "out": True}])
        assert st["singular"] == [64] and want == [[0] * 64] * 4


# ---------------------------------------------------------------------------------------------------- checks
def test_checks_alone_create_no_set(engines):
    eng, curve = engines(8), CURVES["b32x4"]
    T, L = 256, 4
    rnd = random.Random(13)
    cols = operands(4, T, curve, rnd)
    plant_points(cols, curve, rnd)
    # too many rows for the operands and all three expected values: check x3 and y3 of a doubling, whose rows serve twice
    dbl = add_unit(L, x2=0, y2=L)
    want, _ = er.columns(cols[:8], curve, [dbl])
    good = cols[:8] + want[4:12]
    chk = {"mode": "add", "x1": 0, "y1": L, "x2": 0, "y2": L, "expect": [None, 8, 12]}
    rows, st = run(eng, good, curve, [chk], sizes=(8, 8))
    assert rows == [] and st["mismatch"] == [0] and st["first_mismatch"] == [None]
    bad = [list(c) for c in good]
    bad[9][200] ^= 1
    bad[15][17] += 1 << 40   # an expected limb at or above 2^b is another integer
    bad[12][17] ^= 2         # the same row again: counted once
    rows, st = run(eng, bad, curve, [chk, {"mode": "div", "a": 0, "b": 4, "expect": [8]}], 230)
    assert rows == [] and st["mismatch"][0] == 2 and st["first_mismatch"][0] == 17 and st["mismatch"][1] > 200
    # a check beside a committing unit: the set holds the committing unit's rows alone
    rows, st = run(eng, good, curve, [chk, {"mode": "div", "a": 0, "b": 4, "out": True}])
    assert len(rows) == 4 and st["mismatch"] == [0, 0]


# ---------------------------------------------------------------------------------------------------- chains
G = (er.SECP_GX, er.SECP_GY)
CHAIN = {"mode": "chain", "px": 0, "py": 4, "op": 8, "cols": ["ax", "ay", "lam"]}


def chain_cols(ops, T, pts=None):
    cols = [[0] * T for _ in range(9)]
    for t, code in enumerate(ops):
        cols[8][t] = code
        x, y = pts[t] if pts else G
        if pts or code in (1, 2):
            for l in range(4):
                cols[l][t], cols[4 + l][t] = er.limbs(x, er.SECP)[l], er.limbs(y, er.SECP)[l]
    return cols


def test_double_and_add_of_n_minus_one_ends_in_minus_g(engines):
    """(n - 1) G by double-and-add from the top bit in 512 rows: the accumulator before the row behind the last step is -G; one
    more add of G meets its opposite and is exceptional"""
    ops = er.scalar_mul_ops(er.SECP_N - 1) + [2, 0]
    k = len(ops) - 2
    want, st = run(engines(9), chain_cols(ops, 512), er.SECP, [CHAIN])
    val = lambda c, t: sum(want[4 * c + l][t] << (64 * l) for l in range(4))   # noqa: E731
    assert (val(0, k), val(1, k)) == (G[0], er.SECP_P - G[1]) and (val(0, k + 1), val(1, k + 1), val(2, k)) == (0, 0, 0)
    assert st["singular"] == [1] and st["first_singular"] == [k] and st["segments"] == [1] and st["counts"] == [0]


def small_chain(T, ops, rnd, curve=CURVES["m61"]):
    p = curve["p"]
    return [[rnd.randrange(p) for _ in range(T)], [rnd.randrange(p) for _ in range(T)], ops]


def test_segments_of_many_lengths(engines):
    """segments of 1, 2, 63, 64 and 65 rows and one of 100 rows that crosses the workgroup boundary at row 256; the rows
    between the loads hold adds, doublings, holds"""
    T, rnd = 512, random.Random(21)
    starts = [0, 1, 3, 66, 130, 195, 295]
    ops = [rnd.choice([0, 2, 2, 3]) for _ in range(T)]
    for s in starts:
        ops[s] = 1
    curve = CURVES["m61"]
    cols = small_chain(T, ops, rnd)
    for cols_named in (["ax", "ay", "lam"], ["lam"]):
        want, st = run(engines(9), cols, curve, [{"mode": "chain", "px": 0, "py": 1, "op": 2, "cols": cols_named}])
        assert st["segments"] == [len(starts)] and st["unknown"] == [0]
    assert want[0][195] == 0 and any(want[0][196:295])   # lam: 0 on a load row; the segment across the boundary has steps


@pytest.mark.parametrize("case", ["no_load", "unknown", "usable", "one_segment"])
def test_the_remaining_chain_cases(engines, case):
    T, rnd = 256, random.Random(31)
    curve = CURVES["p251"]
    ops = [rnd.choice([0, 1, 2, 2, 3]) for _ in range(T)]
    usable = None
    if case == "no_load":   # the accumulator stays (0, 0): 0 + P has x1 != x2 unless px = 0, doubling (0, 0) is exceptional
        ops = [rnd.choice([0, 2, 3]) for _ in range(T)]
    elif case == "unknown":
        ops[0], ops[40], ops[41], ops[255] = (1 << 32) + 2, (1 << 32) + 2, R - 1, 4
    elif case == "usable":
        usable = 230
        ops[229], ops[230], ops[231] = 2, 1, 1
    else:
        ops = [1] + [rnd.choice([2, 3, 3, 0]) for _ in range(T - 1)]
    cols = small_chain(T, ops, rnd, curve)
    if case == "unknown":
        cols[0][40] = cols[1][41] = 1 << 70   # not read on a row whose op is unknown
        cols[0][3] += 1 << 8
        ops[3] = 2
    tail = [rnd.randrange(R) for _ in range(3 * (T - usable))] if usable else ()
    want, st = run(engines(8), cols, curve, [{"mode": "chain", "px": 0, "py": 1, "op": 2, "cols": ["ax", "ay", "lam"]}], usable, tail)
    if case == "no_load":
        assert st["segments"] == [1]
    elif case == "unknown":
        assert st["unknown"] == [4] and st["first_unknown"] == [0] and st["counts"] == [1] and st["first"] == [3]
    elif case == "usable":
        assert st["segments"] == [len({0} | {t for t in range(230) if ops[t] == 1})]
    else:
        assert st["segments"] == [1]


# ---------------------------------------------------------------------------------------------------- refusals on the device side
def test_refusals_reach_the_caller_and_leave_nothing_behind(engines):
    eng, curve = engines(6), CURVES["p251"]
    before = eng.rows_stats()
    I = commit_sets(eng, [[1] * 64, [2] * 64], (2,))
    try:
        ok = {"mode": "div", "a": 0, "b": 1, "out": True}
        arg_error(lambda: eng.commit_ec(I, curve, [dict(ok, b=2)]), "reaches beyond")
        arg_error(lambda: eng.commit_ec([I[0].handle], curve, [dict(ok, b=2)]), "ec: an operand run")   # the C call's own check
        arg_error(lambda: eng.commit_ec(I, dict(curve, p=250), [ok]), "odd")
        arg_error(lambda: eng.commit_ec(I, curve, [ok], None, [be(1)]), "tail")
        arg_error(lambda: eng.commit_ec(I, curve, [ok], 60, ()), "tail")
        arg_error(lambda: eng.commit_ec(I, curve, [ok], 10, ()), "KZG_MAX_BLIND_ROWS")
        arg_error(lambda: eng.commit_ec([2 ** 40], curve, [ok]), "unknown")
        # the struct as C sees it: what the encoder cannot produce
        cv, recs = eng.ec_call(curve, [ok])
        lib = _native.load()
        hi = (ctypes.c_uint64 * 1)(I[0].handle)
        st = [(ctypes.c_uint64 * 1)() for _ in range(9)]
        c, h = ctypes.create_string_buffer(48), ctypes.c_uint64(0)

        def raw(mutate_curve=None, mutate_unit=None):
            cs, arr = eng.ec_structs(cv, recs)
            if mutate_curve:
                mutate_curve(cs)
            if mutate_unit:
                mutate_unit(arr[0])
            return lib.kzg_rows_commit_ec(eng._h, 1, hi, ctypes.byref(cs), 1, arr, None, c, *st, ctypes.byref(h))

        def set_(obj, name, v, idx=None):
            if idx is None:
                setattr(obj, name, v)
            else:
                getattr(obj, name)[idx] = v

        for mc, mu in [(lambda s: set_(s, "bits", 0), None), (lambda s: set_(s, "limbs", 5), None), (lambda s: set_(s, "p", 250, 0), None),
                       (lambda s: set_(s, "p", 1, 1), None), (lambda s: set_(s, "a", 251, 0), None), (None, lambda u: set_(u, "mode", 4)),
                       (None, lambda u: set_(u, "flags", 4)), (None, lambda u: set_(u, "cols", 2)), (None, lambda u: set_(u, "cols", 0)),
                       (None, lambda u: set_(u, "op", 0)), (None, lambda u: set_(u, "in_", 0, 2)), (None, lambda u: set_(u, "imm", 1, 0)),
                       (None, lambda u: set_(u, "expect", 0, 0)), (None, lambda u: set_(u, "reserved", 1)),
                       (None, lambda u: set_(u, "in_", _native.KZG_EC_ABSENT, 1))]:
            assert raw(mc, mu) == _native.KZG_E_ARG
            assert lib.kzg_last_error(eng._h).startswith(b"ec: "), lib.kzg_last_error(eng._h)
        assert raw() == 0
        assert lib.kzg_rows_release(eng._h, h.value) == 0
    finally:
        release(I)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- the multi route
def test_multi_twin_and_text_clients(hip):
    from zkp_subnet_amd import Client, MultiDeviceClient, codec
    from zkp_subnet_amd.engine import lagrange_factor

    lib = _native.load()
    scale, ms = 8, 0
    T = 1 << scale
    tx, ty = 0x0EC0A6778, 0x13579BF9
    curve = CURVES["m61"]
    rnd = random.Random(1500)
    cols = operands(4, T, curve, rnd) + [[rnd.choice([0, 1, 2, 3]) for _ in range(T)]]
    plant_points(cols, curve, rnd)
    units = [{"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "out": ["lam", "y3"]},
             {"mode": "div", "a": 0, "b": ["imm", "0x1234567"], "out": True},
             {"mode": "chain", "px": 2, "py": 3, "op": 4, "cols": ["ax", "ay"]}]
    plain = [units[0], dict(units[1], b=("imm", 0x1234567)), units[2]]
    u = T - 3
    tail = [random.Random(6).randrange(R) for _ in range(5 * (T - u))]
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    cv, recs = single.ec_call(curve, plain)
    cs, ua = single.ec_structs(cv, recs)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(1, (ctypes.c_int * 1)(0), ctypes.byref(mh)) == 0
    none = lambda vs: [None if v == _native.KZG_EC_NONE else v for v in vs]   # noqa: E731
    try:
        s0 = lagrange_factor(0, ms, ty).to_bytes(32, "big")
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        I = commit_sets(single, cols, (5,))
        c, cc = ctypes.create_string_buffer(48 * 5), ctypes.create_string_buffer(48 * 5)
        hi, hz = ctypes.c_uint64(0), ctypes.c_uint64(0)
        assert lib.kzg_multi_rows_commit(mh, 0, 5, b"".join(row_bytes(r) for r in cols), T, 1, cc, ctypes.byref(hi)) == 0
        ai = (ctypes.c_uint64 * 1)(hi.value)
        made = [hi.value]
        st9 = [(ctypes.c_uint64 * 3)() for _ in range(9)]
        tb = b"".join(bt(tail))
        for opts, usable, tl in ((None, None, ()), (_native.DeriveOpts(u, tb), u, tail)):
            ref, rs = single.commit_ec(I, curve, plain, usable, bt(tl))
            want, stats = er.columns(cols, curve, plain, usable, tl)
            assert rs == stats and read_all(single, ref) == want
            assert lib.kzg_multi_rows_commit_ec(mh, 0, 1, ai, ctypes.byref(cs), 3, ua, ctypes.byref(opts) if opts else None, c, *st9,
                                                ctypes.byref(hz)) == 0
            assert c.raw == b"".join(ref.commitments)
            got = {k: (none(list(v)) if k.startswith("first") else list(v)) for k, v in zip(er.STATS, st9)}
            assert got == rs
            made.append(hz.value)
            ref.release()
        for hh in made:
            assert lib.kzg_multi_rows_release(mh, 0, hh) == 0
        release(I)
    finally:
        lib.kzg_multi_destroy(mh)
    assert single.rows_stats() == (0, 0)

    want, stats = er.columns(cols, curve, plain)
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    text_curve = dict(curve, p=str(curve["p"]), a=hex(curve["a"]))
    for client in (Client(seed=85), MultiDeviceClient(devices=[0], seed=85)):
        client.start(scale=scale, machines_scale=ms)
        try:
            a = client.worker_commit_rows(0, [fr(col) for col in cols]).json()["handle"]
            ref = client.worker_commit_rows(0, [fr(col) for col in want]).json()
            r = client.worker_commit_ec([a], text_curve, units)
            assert r.status_code == 200, r.json()
            body = r.json()
            assert body["commitments"] == ref["commitments"]
            assert {k: body[k] for k in stats} == stats
            chk = client.worker_commit_ec([a, ref["handle"]], curve, [{"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "expect": [5, None, 6]},
                                                                      {"mode": "div", "a": 0, "b": ["imm", 0x1234567], "expect": [6]}])
            assert chk.status_code == 200, chk.json()
            assert chk.json()["handle"] is None and chk.json()["commitments"] == []
            assert chk.json()["mismatch"][0] == 0 and chk.json()["mismatch"][1] > 0
            assert client.worker_commit_ec([a], curve, [dict(units[0], mode="sub")]).status_code == 400
            assert client.worker_commit_ec([a], dict(curve, p=2**61), units).status_code == 400
            assert client.worker_commit_ec([a], curve, [dict(units[0], x1=5)]).status_code == 400   # beyond the five rows
            assert client.worker_commit_ec([a], curve, units, None, fr([1])).status_code == 400
            for hh in (ref["handle"], body["handle"], a):
                assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_ec([a], curve, units).status_code == 400
        finally:
            client.stop()
