"""GPU tests (`-m gpu`) of kzg_rows_commit_edwards: the addition on a twisted Edwards curve over the scalar field itself and the
accumulator trace of a chain, computed and committed on the device.  The expected rows come from the definition in Python
integers (tests/edwards_ref.py), which tests/test_edwards_cpu.py pins against the group orders and the group axioms of Jubjub
and Bandersnatch.  Every committed set is compared with commit_rows of the reference rows byte for byte and cell by cell through
read_rows.  The shapes are T = 256 and 512, plain and with usable = 230 and 490: a full and a partial workgroup of 256 lanes."""
import ctypes
import random

import pytest

from tests import edwards_ref as er
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x0ED0A601, 0x0ED0A602
CURVES = {"jubjub": er.JUBJUB, "bandersnatch": er.BANDERSNATCH}
ADD = {"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "out": ["x3", "y3"]}
SING_ROWS = (6, 7)   # where plant() puts tau = +1 and tau = -1


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
        out, got = eng.commit_edwards(S, curve, units, usable, bt(tail))
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


def inv(v):
    return pow(v, -1, R)


def pairs(T, curve, rnd, on):
    """four columns x1, y1, x2, y2 of T pairs of pairs: curve points, or any field elements"""
    if on:
        pts = [er.point(curve, rnd.randrange(R)) for _ in range(8)]
        pts += [(-x % R, y) for x, y in pts]
        ps = [(rnd.choice(pts), rnd.choice(pts)) for _ in range(T)]
        return [[pq[i][j] for pq in ps] for i in (0, 1) for j in (0, 1)]
    return [[rnd.randrange(R) for _ in range(T)] for _ in range(4)]


def plant(cols, curve, rnd):
    """rows 1 .. 7 of the four operand columns: equal points, opposite points, the neutral element on either side, the point of
    order two (0, -1), tau = +1 and tau = -1 (both off the curve)"""
    d = er.scalar(curve["d"])
    (px, py), (qx, qy) = er.point(curve, rnd.randrange(R)), er.point(curve, rnd.randrange(R))
    x1, y1, x2 = (rnd.randrange(1, R) for _ in range(3))
    y2 = inv(d * x1 * x2 * y1)
    rows = [(px, py, px, py), (px, py, -px % R, py), (0, 1, qx, qy), (px, py, 0, 1), (0, R - 1, qx, qy), (x1, y1, x2, y2),
            (x1, y1, x2, -y2 % R)]
    for t, vals in enumerate(rows, start=1):
        for w, v in enumerate(vals):
            cols[w][t] = v


def tail_for(n_out, T, usable, rnd):
    return [rnd.randrange(R) for _ in range(n_out * (T - usable))] if usable else ()


# ---------------------------------------------------------------------------------------------------- add: sizes, curves, names
@pytest.mark.parametrize("name,lg,usable,on,out", [("jubjub", 8, None, True, ["x3", "y3"]), ("jubjub", 9, 490, False, ["y3", "x3"]),
                                                    ("bandersnatch", 8, 230, True, ["x3"]), ("bandersnatch", 9, None, False, ["y3"]),
                                                    ("jubjub", 8, 230, False, ["x3", "y3"]),
                                                    ("bandersnatch", 9, 490, True, ["y3", "x3"])])
def test_add_on_both_curves(engines, name, lg, usable, on, out):
    """on-curve and off-curve pairs with the planted rows, one name, both and the reverse order, the inputs over two sets"""
    eng, T, curve = engines(lg), 1 << lg, CURVES[name]
    rnd = random.Random(lg * 1000 + (usable or 0) + len(out))
    cols = pairs(T, curve, rnd, on)
    plant(cols, curve, rnd)
    want, st = run(eng, cols, curve, [dict(ADD, out=out)], usable, tail_for(len(out), T, usable, rnd), sizes=(1, 3))
    assert st["singular"] == [2] and st["first_singular"] == [6] and len(want) == len(out)
    x3 = want[out.index("x3")] if "x3" in out else None
    if x3:
        assert x3[2] == 0 and x3[3] == cols[2][3] and x3[4] == cols[0][4] and x3[6] == x3[7] == 0   # P - P, 0 + Q, P + 0
    if on and x3 and "y3" in out:
        y3 = want[out.index("y3")]
        assert all(er.on_curve(curve, x3[t], y3[t]) for t in range(usable or T) if t not in SING_ROWS)


def test_four_units_with_an_immediate_in_each_slot(engines):
    """four units in one call, eight output rows, the batched inversion over 4 T elements; unit w takes slot w from an
    immediate: a constant point on either side, and half of one"""
    eng, T, curve = engines(8), 256, er.JUBJUB
    rnd = random.Random(41)
    cols = pairs(T, curve, rnd, True)
    plant(cols, curve, rnd)
    bx, by = er.point(curve, 99)
    units = [dict(ADD, **{k: ("imm", v)}) for k, v in zip(("x1", "y1", "x2", "y2"), (bx, by, hex(bx), be(by)))]
    want, st = run(eng, cols, curve, units, sizes=(2, 2))
    assert len(want) == 8 and st["segments"] == [0] * 4
    both = [dict(ADD, x1=("imm", 0), y1=("imm", 1)), dict(ADD, x2=("imm", bx), y2=("imm", by), out=["y3"])]
    want, st = run(eng, cols, curve, both, 230, tail_for(3, T, 230, rnd))
    assert want[0][:230] == cols[2][:230] and want[1][:230] == cols[3][:230]   # the neutral element on the left


def test_a_row_serves_two_slots_and_the_doubling(engines):
    """the same rows named twice double a column; one row in two slots of one pair"""
    eng, T, curve = engines(9), 512, er.BANDERSNATCH
    rnd = random.Random(42)
    cols = pairs(T, curve, rnd, True)[:2]
    units = [dict(ADD, x2=0, y2=1), dict(ADD, y1=0, x2=1, y2=1, out=["y3", "x3"])]
    want, st = run(eng, cols, curve, units, 490, tail_for(4, T, 490, rnd))
    assert st["singular"][0] == 0 and all(er.on_curve(curve, want[0][t], want[1][t]) for t in range(490))


# ---------------------------------------------------------------------------------------------------- add as a check
@pytest.mark.parametrize("lg,usable,beside", [(8, None, False), (9, 490, False), (8, 230, True), (9, None, True)])
def test_check_counts_the_rows_that_differ(engines, lg, usable, beside):
    """both cells wrong, one wrong and neither; an exceptional row computes 0.  Alone the call creates no set and leaves
    rows_stats as it was (run() asserts both); beside a committing unit the set holds that unit's rows only"""
    eng, T, curve = engines(lg), 1 << lg, er.JUBJUB
    rnd = random.Random(lg + (usable or 0))
    cols = pairs(T, curve, rnd, lg == 8)
    plant(cols, curve, rnd)
    (x3, y3), _ = er.columns(cols, curve, [ADD])
    x3, y3 = list(x3), list(y3)
    x3[10], y3[10] = (x3[10] + 1) % R, (y3[10] + 1) % R   # both wrong
    x3[20] = (x3[20] + 1) % R                             # x alone
    y3[30] = (y3[30] + 1) % R                             # y alone
    y3[7] = 5                                             # an exceptional row computes 0
    x3[T - 1] = (x3[T - 1] + 1) % R                       # behind usable: not compared there
    cols += [x3, y3]
    units = [dict(ADD, out=None, expect=[4, 5]), dict(ADD, out=None, expect=[4, None]), dict(ADD, out=None, expect=[None, 5])]
    for u in units:
        del u["out"]
    last = 0 if usable else 1
    if beside:
        units = [units[0], dict(ADD, out=["y3"]), units[2]]
        want, st = run(eng, cols, curve, units, usable, tail_for(1, T, usable, rnd), sizes=(4, 2))
        assert len(want) == 1 and st["mismatch"] == [4 + last, 0, 3] and st["first_mismatch"] == [7, None, 7]
    else:
        want, st = run(eng, cols, curve, units, usable, (), sizes=(4, 2))
        assert want == [] and st["mismatch"] == [4 + last, 2 + last, 3] and st["first_mismatch"] == [7, 10, 7]
    assert st["singular"] == [2] * 3


# ---------------------------------------------------------------------------------------------------- the gate, without the reference
@pytest.mark.parametrize("name,on", [("jubjub", False), ("bandersnatch", True)])
def test_the_two_addition_gates_vanish_on_the_committed_output(engines, name, on):
    """independent of tests/edwards_ref.py: x3 (1 + D x1 x2 y1 y2) - x1 y2 - y1 x2 and y3 (1 - D x1 x2 y1 y2) - y1 y2 + A x1 x2,
    evaluated by kzg_rows_commit_expr over the inputs and the device's output, are 0 on every row (none is exceptional)"""
    eng, T, curve = engines(8), 256, CURVES[name]
    a, d = er.scalar(curve["a"]), er.scalar(curve["d"])
    cols = pairs(T, curve, random.Random(7), on)
    S = commit_sets(eng, cols, (4,))
    try:
        out, st = eng.commit_edwards(S, curve, [ADD])
        try:
            assert st["singular"] == [0]
            gx = [(be(1), [4]), (be(d), [4, 0, 2, 1, 3]), (be(R - 1), [0, 3]), (be(R - 1), [1, 2])]
            gy = [(be(1), [5]), (be(R - d), [5, 0, 2, 1, 3]), (be(R - 1), [1, 3]), (be(a), [0, 2])]
            none, nonzero, first = eng.commit_expr(S + [out], [(gx, True), (gy, True)])
            assert none is None and nonzero == [0, 0] and first == [None, None]
            bad = [(be(1), [4]), (be(d), [4, 0, 2, 1, 3]), (be(R - 1), [0, 3]), (be(R - 2), [1, 2])]   # (the check can fail)
            assert eng.commit_expr(S + [out], [(bad, True)])[1][0] > 0
        finally:
            out.release()
    finally:
        release(S)


# ---------------------------------------------------------------------------------------------------- chains
def chain_unit(**kw):
    return dict({"mode": "chain", "px": 0, "py": 1, "op": 2, "cols": ["ax", "ay"]}, **kw)


def point_cols(T, curve, rnd):
    pts = [er.point(curve, rnd.randrange(R)) for _ in range(6)]
    ps = [rnd.choice(pts) for _ in range(T)]
    return [[p[0] for p in ps], [p[1] for p in ps]]


@pytest.mark.parametrize("case", ["random", "short", "one_segment", "imm_base", "exceptional", "off_curve"])
def test_chain_segment_layouts(engines, case):
    rnd = random.Random(sum(map(ord, case)))
    curve = er.BANDERSNATCH if case in ("short", "imm_base") else er.JUBJUB
    T, usable, unit = 512, None, chain_unit()
    cols = point_cols(T, curve, rnd)
    if case == "random":   # every op-code, unknown ones among them; loads wherever they fall
        usable = 490
        ops = [rnd.choice([0, 1, 2, 2, 3, 3, 4, 4, 5, 2**32 + 2, R - 1, 2**64 + 1]) for _ in range(T)]
    elif case == "short":   # segments of length 1 and 2, a load at row 0, at the workgroup seam and at row n - 1
        ops = [1 if t % 3 != 2 else rnd.choice([2, 3, 4]) for t in range(T)]
        ops[0] = ops[255] = ops[256] = ops[T - 1] = 1
        unit = chain_unit(cols=["ay"])
    elif case == "one_segment":   # no load: one lane walks all 512 rows
        ops = [rnd.choice([0, 2, 3, 4]) for _ in range(T)]
        unit = chain_unit(cols=["ax"])
    elif case == "imm_base":   # a fixed base point; a load at row n - 1 of the usable layout
        T, usable = 256, 230
        bx, by = er.point(curve, 5)
        cols = [[0] * T, [0] * T]
        ops = [rnd.choice([0, 1, 2, 3, 4]) for _ in range(T)]
        ops[usable - 1] = 1
        unit = chain_unit(px=("imm", bx), py=("imm", hex(by)), cols=["ay", "ax"])
    elif case == "exceptional":   # tau = +1 at row 6 and tau = -1 at row 40, inside segments; the walk goes on from (0, 1)
        ops = [rnd.choice([0, 2, 3, 4]) for _ in range(T)]
        d = er.scalar(curve["d"])
        for t0, sign in ((5, 1), (39, R - 1)):
            x1, y1, x2 = (rnd.randrange(1, R) for _ in range(3))
            cols[0][t0], cols[1][t0], ops[t0] = x1, y1, 1
            cols[0][t0 + 1], cols[1][t0 + 1], ops[t0 + 1] = x2, sign * inv(d * x1 * x2 * y1) % R, 2
            ops[t0 + 2] = 2
    else:   # pairs that lie on no curve
        ops = [rnd.choice([0, 1, 2, 3, 4]) for _ in range(T)]
        cols = [[rnd.randrange(R) for _ in range(T)] for _ in range(2)]
    cols.append(ops)
    n = usable or T
    want, st = run(engines(9 if T == 512 else 8), cols, curve, [unit], usable, tail_for(len(unit["cols"]), T, usable, rnd),
                   sizes=(2, 1))
    assert st["segments"] == [len({0} | {t for t in range(n) if ops[t] == 1})]
    assert st["mismatch"] == [0] and st["first_mismatch"] == [None]
    if case == "random":
        unk = [t for t in range(n) if ops[t] > 4]
        assert st["unknown"] == [len(unk)] and st["first_unknown"] == [unk[0]]
    elif case == "exceptional":
        assert st["singular"] == [2] and st["first_singular"] == [6]
        assert (want[0][7], want[1][7]) == (0, 1) and (want[0][8], want[1][8]) == (cols[0][7], cols[1][7])
    elif case == "one_segment":
        assert st["segments"] == [1] and st["unknown"] == [0]


def test_chain_beside_an_add_and_a_check(engines):
    """the three unit forms in one call: the chain's denominators and the addition's share one inversion"""
    eng, T, curve = engines(8), 256, er.JUBJUB
    rnd = random.Random(55)
    cols = pairs(T, curve, rnd, True)
    plant(cols, curve, rnd)
    cols.append([rnd.choice([0, 1, 2, 3, 4, 7]) for _ in range(T)])
    (x3, _), _ = er.columns(cols, curve, [ADD])
    cols.append(list(x3))
    units = [chain_unit(px=2, py=3, op=4, cols=["ay", "ax"]), {"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "expect": [5, None]},
             dict(ADD, out=["y3", "x3"]), chain_unit(px=0, py=1, op=4, cols=["ax"])]
    want, st = run(eng, cols, curve, units, 230, tail_for(5, T, 230, rnd), sizes=(3, 3))
    assert len(want) == 5 and st["mismatch"] == [0] * 4 and st["unknown"][0] == st["unknown"][3] > 0 and st["unknown"][1:3] == [0, 0]


def test_sixteen_bit_double_and_add(engines):
    """ops 1, then 3 and 2 per bit: the accumulator behind the last step is k P, computed here by a double-and-add of its own"""
    eng, T, curve = engines(8), 256, er.JUBJUB
    P, k = er.point(curve, 1234), 0xB6E5
    ops = er.scalar_mul_ops(k)
    assert k.bit_length() == 16 and len(ops) < T
    cols = [[P[0]] * T, [P[1]] * T, ops + [0] * (T - len(ops))]
    want, st = run(eng, cols, curve, [chain_unit()])
    acc = er.NEUTRAL
    for bit in bin(k)[2:]:
        acc = er.add(curve, *acc, *acc)[:2]
        if bit == "1":
            acc = er.add(curve, *acc, *P)[:2]
    assert (want[0][len(ops)], want[1][len(ops)]) == acc == (want[0][T - 1], want[1][T - 1])
    assert st["segments"] == [1] and st["singular"] == [0]


# ---------------------------------------------------------------------------------------------------- refusals on the device side
def test_refusals_reach_the_caller_and_leave_nothing_behind(engines):
    eng, curve = engines(6), er.JUBJUB
    before = eng.rows_stats()
    I = commit_sets(eng, [[1] * 64, [2] * 64], (2,))
    try:
        ok = {"mode": "add", "x1": 0, "y1": 1, "x2": 1, "y2": 0, "out": ["x3"]}
        arg_error(lambda: eng.commit_edwards(I, curve, [dict(ok, x2=2)]), "reaches beyond")
        arg_error(lambda: eng.commit_edwards([I[0].handle], curve, [dict(ok, x2=2)]), "edwards: a row")   # the C call's own check
        arg_error(lambda: eng.commit_edwards(I, dict(curve, d=curve["a"]), [ok]), "differ")
        arg_error(lambda: eng.commit_edwards(I, curve, [ok], None, [be(1)]), "tail")
        arg_error(lambda: eng.commit_edwards(I, curve, [ok], 60, ()), "tail")
        arg_error(lambda: eng.commit_edwards(I, curve, [ok], 10, ()), "KZG_MAX_BLIND_ROWS")
        arg_error(lambda: eng.commit_edwards([2 ** 40], curve, [ok]), "unknown")
        stale = commit_sets(eng, [[3] * 64], (1,))
        release(stale)
        arg_error(lambda: eng.commit_edwards([stale[0].handle], curve, [dict(ok, y1=0, x2=0)]))
        # the struct as C sees it: what the encoder cannot produce
        cv, recs = eng.edwards_call(curve, [ok])
        lib = _native.load()
        hi = (ctypes.c_uint64 * 1)(I[0].handle)
        st = [(ctypes.c_uint64 * 1)() for _ in range(7)]
        c, h = ctypes.create_string_buffer(48), ctypes.c_uint64(0)

        def raw(mutate_curve=None, mutate_unit=None):
            cs, arr = eng.edwards_structs(cv, recs)
            if mutate_curve:
                mutate_curve(cs)
            if mutate_unit:
                mutate_unit(arr[0])
            return lib.kzg_rows_commit_edwards(eng._h, 1, hi, ctypes.byref(cs), 1, arr, None, c, *st, ctypes.byref(h))

        def set_(obj, name, v, idx=None):
            if idx is None:
                setattr(obj, name, v)
            else:
                getattr(obj, name)[idx] = v

        def fill(arr32, bs):
            arr32[:] = list(bs)

        ABSENT, IMM = _native.KZG_EDWARDS_ABSENT, _native.KZG_EDWARDS_IMM
        for mc, mu in [(lambda s: fill(s.a_be32, R.to_bytes(32, "big")), None), (lambda s: fill(s.d_be32, bytes(32)), None),
                       (lambda s: fill(s.a_be32, bytes(32)), None), (lambda s: fill(s.a_be32, bytes(s.d_be32)), None),
                       (None, lambda u: set_(u, "mode", 3)), (None, lambda u: set_(u, "flags", 2)), (None, lambda u: set_(u, "cols", 4)),
                       (None, lambda u: set_(u, "cols", 0)), (None, lambda u: set_(u, "cols", 3)), (None, lambda u: set_(u, "op", 0)),
                       (None, lambda u: set_(u, "in_", ABSENT, 2)), (None, lambda u: fill(u.imm_be32[0], be(1))),
                       (None, lambda u: (set_(u, "in_", IMM, 0), fill(u.imm_be32[0], R.to_bytes(32, "big")))),
                       (None, lambda u: set_(u, "expect", 0, 0)), (None, lambda u: set_(u, "out_order", 1, 0)),
                       (None, lambda u: set_(u, "out_order", 0, 1)), (None, lambda u: set_(u, "out_order", ABSENT, 0)),
                       (None, lambda u: (set_(u, "mode", _native.KZG_EDWARDS_CHAIN), set_(u, "flags", 1)))]:
            assert raw(mc, mu) == _native.KZG_E_ARG
            assert lib.kzg_last_error(eng._h).startswith(b"edwards: "), lib.kzg_last_error(eng._h)
        assert raw() == 0
        assert lib.kzg_rows_release(eng._h, h.value) == 0
        run(eng, [[1] * 64, [2] * 64], curve, [ok])   # a good call still passes
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
    tx, ty = 0x0ED0A6778, 0x13579BF9
    curve = er.JUBJUB
    rnd = random.Random(1600)
    cols = pairs(T, curve, rnd, True) + [[rnd.choice([0, 1, 2, 3, 4]) for _ in range(T)]]
    plant(cols, curve, rnd)
    bx, by = er.point(curve, 17)
    units = [{"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "out": ["y3", "x3"]},
             {"mode": "add", "x1": 0, "y1": 1, "x2": ["imm", hex(bx)], "y2": ["imm", str(by)], "out": ["x3"]},
             {"mode": "chain", "px": 2, "py": 3, "op": 4, "cols": ["ax", "ay"]}]
    plain = [units[0], dict(units[1], x2=("imm", bx), y2=("imm", by)), units[2]]
    u = T - 3
    tail = [random.Random(6).randrange(R) for _ in range(5 * (T - u))]
    single = hip()
    single.gen_srs(tx, ty, scale, ms)
    cv, recs = single.edwards_call(curve, plain)
    cs, ua = single.edwards_structs(cv, recs)
    mh = ctypes.c_void_p()
    assert lib.kzg_multi_create(1, (ctypes.c_int * 1)(0), ctypes.byref(mh)) == 0
    none = lambda vs: [None if v == _native.KZG_EDWARDS_NONE else v for v in vs]   # noqa: E731
    try:
        s0 = lagrange_factor(0, ms, ty).to_bytes(32, "big")
        assert lib.kzg_multi_gen_srs(mh, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        I = commit_sets(single, cols, (5,))
        c, cc = ctypes.create_string_buffer(48 * 5), ctypes.create_string_buffer(48 * 5)
        hi, hz = ctypes.c_uint64(0), ctypes.c_uint64(0)
        assert lib.kzg_multi_rows_commit(mh, 0, 5, b"".join(row_bytes(r) for r in cols), T, 1, cc, ctypes.byref(hi)) == 0
        ai = (ctypes.c_uint64 * 1)(hi.value)
        made = [hi.value]
        st7 = [(ctypes.c_uint64 * 3)() for _ in range(7)]
        tb = b"".join(bt(tail))
        for opts, usable, tl in ((None, None, ()), (_native.DeriveOpts(u, tb), u, tail)):
            ref, rs = single.commit_edwards(I, curve, plain, usable, bt(tl))
            want, stats = er.columns(cols, curve, plain, usable, tl)
            assert rs == stats and read_all(single, ref) == want
            assert lib.kzg_multi_rows_commit_edwards(mh, 0, 1, ai, ctypes.byref(cs), 3, ua, ctypes.byref(opts) if opts else None, c,
                                                     *st7, ctypes.byref(hz)) == 0
            assert c.raw == b"".join(ref.commitments)
            got = {k: (none(list(v)) if k.startswith("first") else list(v)) for k, v in zip(er.STATS, st7)}
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
    text_curve = {"a": str(curve["a"]), "d": hex(curve["d"])}
    for client in (Client(seed=86), MultiDeviceClient(devices=[0], seed=86)):
        client.start(scale=scale, machines_scale=ms)
        try:
            a = client.worker_commit_rows(0, [fr(col) for col in cols]).json()["handle"]
            ref = client.worker_commit_rows(0, [fr(col) for col in want]).json()
            r = client.worker_commit_edwards([a], text_curve, units)
            assert r.status_code == 200, r.json()
            body = r.json()
            assert body["commitments"] == ref["commitments"]
            assert {k: body[k] for k in stats} == stats
            chk = client.worker_commit_edwards([a, ref["handle"]], curve, [{"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "expect": [6, 5]},
                                                                           {"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "expect": [5, None]}])
            assert chk.status_code == 200, chk.json()
            assert chk.json()["handle"] is None and chk.json()["commitments"] == []
            assert chk.json()["mismatch"][0] == 0 and chk.json()["mismatch"][1] > 0
            assert client.worker_commit_edwards([a], curve, [dict(units[0], mode="sub")]).status_code == 400
            assert client.worker_commit_edwards([a], dict(curve, d=0), units).status_code == 400
            assert client.worker_commit_edwards([a], curve, [dict(units[0], x1=5)]).status_code == 400   # beyond the five rows
            assert client.worker_commit_edwards([a], curve, units, None, fr([1])).status_code == 400
            for hh in (ref["handle"], body["handle"], a):
                assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_edwards([a], curve, units).status_code == 400
        finally:
            client.stop()
