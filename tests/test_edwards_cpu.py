"""CPU tests of kzg_rows_commit_edwards: tests/edwards_ref.py (the definition the GPU tests compare with) is pinned by identities
that do not use it -- the group orders of Jubjub and Bandersnatch on points found by a square root, closure, the group axioms,
an independent double-and-add -- and the encoder, the refusals the host can decide, the symbol table and the header's wording
are checked without a device."""
import ctypes
import os
import random
import re

import pytest

from tests import edwards_ref as er
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import HipEngine

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kzg_mi355x.h")
R = er.R
CURVES = [(er.JUBJUB, er.JUBJUB_ORDER), (er.BANDERSNATCH, er.BANDERSNATCH_ORDER)]
IDS = ["jubjub", "bandersnatch"]
ADD = {"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "out": ["x3", "y3"]}
CHAIN = {"mode": "chain", "px": 0, "py": 1, "op": 2, "cols": ["ax", "ay"]}


def padd(curve, p, q):
    x3, y3, sing = er.add(curve, p[0], p[1], q[0], q[1])
    assert not sing
    return x3, y3


def mul(curve, k, pt):
    """k pt by a double-and-add of this file's own, from the top bit"""
    acc = er.NEUTRAL
    for bit in bin(k)[2:]:
        acc = padd(curve, acc, acc)
        if bit == "1":
            acc = padd(curve, acc, pt)
    return acc


# ---------------------------------------------------------------------------------------------------- the reference is the group law
def test_the_parameter_sets():
    assert er.JUBJUB["a"] == R - 1 and er.JUBJUB["d"] == -10240 * pow(10241, -1, R) % R
    assert er.BANDERSNATCH["a"] == R - 5
    for curve, _ in CURVES:
        assert pow(curve["d"], (R - 1) // 2, R) == R - 1          # D is not a square on either
    assert pow(er.JUBJUB["a"], (R - 1) // 2, R) == 1 and pow(er.BANDERSNATCH["a"], (R - 1) // 2, R) == R - 1


@pytest.mark.parametrize("curve,order", CURVES, ids=IDS)
def test_the_group_order_annihilates_points_found_by_a_square_root(curve, order):
    rnd = random.Random(order % 1000)
    for _ in range(3):
        y = rnd.randrange(R)
        while True:   # this test's own search: x^2 = (1 - y^2) / (A - D y^2)
            x = er.sqrt((1 - y * y) * pow(curve["a"] - curve["d"] * y * y, -1, R))
            if x is not None:
                break
            y += 1
        assert (x * x - (1 - y * y) * pow(curve["a"] - curve["d"] * y * y, -1, R)) % R == 0 and er.on_curve(curve, x, y)
        # the cofactor first: A is not a square on Bandersnatch, whose law is complete on the subgroup of prime order only (two
        # of its points of order two lie at infinity, and a multiple that lands on one of them is an exceptional step)
        cof = 8 if curve is er.JUBJUB else 4
        assert order % cof == 0 and pow(2, order // cof - 1, order // cof) == 1
        small = mul(curve, cof, (x, y))
        assert small != er.NEUTRAL and mul(curve, order // cof, small) == er.NEUTRAL


@pytest.mark.parametrize("curve,order", CURVES, ids=IDS)
def test_closure_commutativity_associativity_and_the_inverse(curve, order):
    P, Q, S = (er.point(curve, s) for s in (11, 2222, 333333))
    for A, B in ((P, Q), (Q, S), (P, P), (P, er.NEUTRAL), ((0, R - 1), Q)):
        C = padd(curve, A, B)
        assert er.on_curve(curve, *C) and C == padd(curve, B, A)
    assert padd(curve, padd(curve, P, Q), S) == padd(curve, P, padd(curve, Q, S))
    assert padd(curve, P, er.NEUTRAL) == P and padd(curve, er.NEUTRAL, Q) == Q
    assert padd(curve, P, (-P[0] % R, P[1])) == er.NEUTRAL
    assert padd(curve, (0, R - 1), (0, R - 1)) == er.NEUTRAL                 # the point of order two
    assert padd(curve, P, P) == mul(curve, 2, P) and padd(curve, padd(curve, P, P), P) == mul(curve, 3, P)


@pytest.mark.parametrize("curve,order", CURVES, ids=IDS)
def test_a_chain_of_a_load_then_doublings_and_additions_ends_on_k_p(curve, order):
    P, k = er.point(curve, 77), 0xD00D
    ops = er.scalar_mul_ops(k) + [0, 0]
    T = len(ops)
    (ax, ay), st = er.columns([[P[0]] * T, [P[1]] * T, ops], curve, [CHAIN])
    assert (ax[0], ay[0]) == er.NEUTRAL and (ax[1], ay[1]) == P
    assert (ax[-1], ay[-1]) == mul(curve, k, P)
    assert st["segments"] == [1] and st["singular"] == [0] and st["unknown"] == [0] and st["first_unknown"] == [None]


def test_op_four_undoes_op_two_and_unknown_codes_hold():
    curve = er.JUBJUB
    P, Q = er.point(curve, 5), er.point(curve, 6)
    ops = [1, 2, 4, 4, 2, 2**32 + 2, 5, 0, 1, 3]
    px = [P[0], Q[0], Q[0], Q[0], Q[0], 9, 9, 9, Q[0], 9]
    py = [P[1], Q[1], Q[1], Q[1], Q[1], 9, 9, 9, Q[1], 9]
    (ax, ay), st = er.columns([px, py, ops], curve, [CHAIN])
    acc = list(zip(ax, ay))
    assert acc[1] == P and acc[2] == padd(curve, P, Q) and acc[3] == P and acc[5] == P
    assert acc[4] == padd(curve, P, (-Q[0] % R, Q[1]))
    assert acc[6] == acc[7] == acc[8] == P and acc[9] == Q
    assert st["unknown"] == [2] and st["first_unknown"] == [5] and st["segments"] == [2]
    only_ay, _ = er.columns([px, py, ops], curve, [dict(CHAIN, cols=["ay"])])
    assert only_ay == [ay]


@pytest.mark.parametrize("curve,order", CURVES, ids=IDS)
def test_off_curve_pairs_with_tau_one_or_minus_one_are_exceptional(curve, order):
    rnd = random.Random(3)
    x1, y1, x2 = (rnd.randrange(1, R) for _ in range(3))
    y2 = pow(curve["d"] * x1 * x2 * y1, -1, R)
    assert not er.on_curve(curve, x1, y1)
    for yy in (y2, -y2 % R):
        assert er.add(curve, x1, y1, x2, yy) == (0, 0, True)
    cols = [[x1, x1, x1], [y1, y1, y1], [x2, x2, x2], [y2, -y2 % R, 1]]
    rows, st = er.columns(cols, curve, [ADD, dict(ADD, out=["y3", "x3"])])
    assert rows[0][:2] == rows[1][:2] == [0, 0] and rows[0][2] != 0 and rows[0] == rows[3] and rows[1] == rows[2]
    assert st["singular"] == [2, 2] and st["first_singular"] == [0, 0]
    # in a chain the accumulator restarts from the neutral element
    ops = [1, 2, 2, 0]
    (ax, ay), st = er.columns([[x1, x2, x2, 0], [y1, y2, 7, 0], ops], curve, [CHAIN])
    assert (ax[2], ay[2]) == er.NEUTRAL and (ax[3], ay[3]) == (x2, 7) and st["singular"] == [1] and st["first_singular"] == [1]


def test_a_check_counts_rows_and_commits_nothing_and_the_tail_lies_behind_usable():
    curve = er.BANDERSNATCH
    rnd = random.Random(9)
    cols = [[rnd.randrange(R) for _ in range(8)] for _ in range(4)]
    (x3, y3), _ = er.columns(cols, curve, [ADD])
    bad_x, bad_y = list(x3), list(y3)
    bad_x[2] += 1
    bad_y[2] += 1
    bad_y[5] += 1
    bad_x[7] += 1
    rows, st = er.columns(cols + [bad_x, bad_y], curve, [dict(ADD, out=None, expect=[4, 5]), dict(ADD, out=None, expect=[4, None])], 6, ())
    assert rows == [] and st["mismatch"] == [2, 1] and st["first_mismatch"] == [2, 2]
    rows, st = er.columns(cols, curve, [dict(ADD, out=["y3"])], 6, [101, 102])
    assert rows == [y3[:6] + [101, 102]]
    imm, _ = er.columns(cols, curve, [dict(ADD, x1=("imm", 0), y1=("imm", "0x1"))])
    assert imm == [cols[2], cols[3]]


# ---------------------------------------------------------------------------------------------------- the encoder
def test_the_encoder_fills_the_struct_fields():
    A_, I_ = _native.KZG_EDWARDS_ABSENT, _native.KZG_EDWARDS_IMM
    units = [dict(ADD, y1=("imm", 5), out=["y3", "x3"]), dict(CHAIN, px=("imm", "0x10"), cols=["ay"]),
             {"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "expect": [None, 4]}]
    cv, recs = HipEngine.edwards_call({"a": str(er.JUBJUB["a"]), "d": er.JUBJUB["d"].to_bytes(32, "big")}, units, n_rows=5)
    assert cv == (er.JUBJUB["a"].to_bytes(32, "big"), er.JUBJUB["d"].to_bytes(32, "big"))
    assert recs[0][:7] == (_native.KZG_EDWARDS_ADD, 0, 3, A_, [0, I_, 2, 3], [A_, A_], [1, 0])
    assert recs[0][7][1] == (5).to_bytes(32, "big") and recs[0][7][0] == bytes(32)
    assert recs[1][:7] == (_native.KZG_EDWARDS_CHAIN, 0, 2, 2, [I_, 1, A_, A_], [A_, A_], [1, A_])
    assert recs[1][7][0] == (16).to_bytes(32, "big")
    assert recs[2][:7] == (_native.KZG_EDWARDS_ADD, _native.KZG_EDWARDS_CHECK, 2, A_, [0, 1, 2, 3], [A_, 4], [A_, A_])
    assert HipEngine.edwards_n_out(recs) == 3
    cs, arr = HipEngine.edwards_structs(cv, recs)
    assert bytes(cs.a_be32) == cv[0] and bytes(cs.d_be32) == cv[1]
    assert (arr[0].mode, arr[0].cols, arr[0].op, list(arr[0].in_), list(arr[0].out_order)) == (1, 3, A_, [0, I_, 2, 3], [1, 0])
    assert bytes(arr[0].imm_be32[1]) == (5).to_bytes(32, "big") and bytes(arr[1].imm_be32[0])[-1] == 16
    assert (arr[2].flags, list(arr[2].expect)) == (1, [A_, 4])


BAD = [
    ({"a": 1}, [ADD], "exactly a and d"),
    ({"a": 1, "d": 2, "c": 3}, [ADD], "exactly a and d"),
    ({"a": R, "d": 2}, [ADD], "canonical"),
    ({"a": 1, "d": -1}, [ADD], "non-negative"),
    ({"a": 0, "d": 2}, [ADD], "must not be 0"),
    ({"a": 3, "d": 0}, [ADD], "must not be 0"),
    ({"a": 7, "d": "0x7"}, [ADD], "must differ"),
    ({"a": "x", "d": 2}, [ADD], "integer"),
    (er.JUBJUB, [], "1 .. 4"),
    (er.JUBJUB, [ADD] * 5, "1 .. 4"),
    (er.JUBJUB, [{"x1": 0}], "mode"),
    (er.JUBJUB, [dict(ADD, mode="sub")], "unknown mode"),
    (er.JUBJUB, [dict(ADD, lam=1)], "unknown field"),
    (er.JUBJUB, [dict(CHAIN, expect=[1, 2])], "not to chain"),
    (er.JUBJUB, [dict(CHAIN, out=["ax"])], "unknown field"),
    (er.JUBJUB, [dict(ADD, x1=None)], "row index"),
    (er.JUBJUB, [dict(ADD, x1=-1)], "must be a row"),
    (er.JUBJUB, [dict(ADD, x1=2**32 - 2)], "must be a row"),
    (er.JUBJUB, [dict(ADD, y2=("imm",))], "immediate"),
    (er.JUBJUB, [dict(ADD, y2=("imm", R))], "canonical"),
    (er.JUBJUB, [dict(ADD, out=[])], "1 .. 2 names"),
    (er.JUBJUB, [dict(ADD, out=["x3", "x3"])], "repeated"),
    (er.JUBJUB, [dict(ADD, out=["ax"])], "unknown name"),
    (er.JUBJUB, [dict(ADD, expect=[4, 5])], "out together with expect"),
    (er.JUBJUB, [{"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3}], "needs out"),
    (er.JUBJUB, [{"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "expect": [4]}], "two entries"),
    (er.JUBJUB, [{"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "expect": [None, None]}], "at least one"),
    (er.JUBJUB, [dict(CHAIN, op=("imm", 1))], "op must be a row"),
    (er.JUBJUB, [dict(CHAIN, cols=["x3"])], "unknown name"),
    (er.JUBJUB, [dict(CHAIN, cols=None)], "1 .. 2 column names"),
    (er.JUBJUB, [dict(ADD, x1=4 * u, y1=4 * u + 1, x2=4 * u + 2, y2=4 * u + 3) for u in range(4)] [:3] +
     [dict(ADD, x1=12, y1=13, x2=14, y2=15, out=None, expect=[16, None])], "distinct input rows"),
]


@pytest.mark.parametrize("curve,units,why", BAD)
def test_python_refusals(curve, units, why):
    with pytest.raises(KzgError) as ei:
        HipEngine.edwards_call(curve, units)
    assert ei.value.code == _native.KZG_E_ARG and "edwards:" in str(ei.value) and why in str(ei.value), str(ei.value)


def test_a_row_beyond_the_concatenation_is_refused_where_the_length_is_known():
    assert HipEngine.edwards_call(er.JUBJUB, [ADD], n_rows=4)
    for units in ([ADD], [dict(CHAIN, op=3)], [{"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 2, "expect": [None, 3]}]):
        with pytest.raises(KzgError) as ei:
            HipEngine.edwards_call(er.JUBJUB, units, n_rows=3)
        assert "reaches beyond the 3 concatenated rows" in str(ei.value)


def test_sixteen_output_rows_fit_and_seventeen_do_not():
    """the output limit cannot be reached by four units of two names each: eight rows are the most a call commits"""
    _, recs = HipEngine.edwards_call(er.JUBJUB, [ADD, CHAIN, ADD, CHAIN])
    assert HipEngine.edwards_n_out(recs) == 8 <= _native.KZG_MAX_BATCH_OPEN


def test_the_host_refuses_before_a_context_is_touched():
    """kzg_rows_commit_edwards decides these on the host before it takes a lane: a buffer of zeros stands in for the context,
    which a refused call never reads"""
    lib = _native.load()
    fake = ctypes.create_string_buffer(1 << 12)
    cv, recs = HipEngine.edwards_call(er.JUBJUB, [dict(ADD, out=["x3"])])
    hi = (ctypes.c_uint64 * 1)(1)
    st = [(ctypes.c_uint64 * 1)() for _ in range(7)]
    c, h = ctypes.create_string_buffer(48), ctypes.c_uint64(0)
    big = R.to_bytes(32, "big")
    A_, I_ = _native.KZG_EDWARDS_ABSENT, _native.KZG_EDWARDS_IMM

    def fill(arr32, bs):
        arr32[:] = list(bs)

    def idx(name, k, v):
        return lambda u: getattr(u, name).__setitem__(k, v)

    cases = [(lambda s: fill(s.a_be32, big), None, "canonical"), (lambda s: fill(s.d_be32, big), None, "canonical"),
             (lambda s: fill(s.a_be32, bytes(32)), None, "must not be 0"), (lambda s: fill(s.d_be32, bytes(32)), None, "must not be 0"),
             (lambda s: fill(s.a_be32, bytes(s.d_be32)), None, "differ"),
             (None, lambda u: setattr(u, "mode", 3), "unknown mode"), (None, lambda u: setattr(u, "flags", 2), "flags"),
             (None, lambda u: setattr(u, "cols", 4), "cols"), (None, lambda u: setattr(u, "cols", 0), "cols"),
             (None, lambda u: setattr(u, "cols", 3), "out_order"), (None, lambda u: setattr(u, "op", 0), "op belongs"),
             (None, idx("in_", 2, A_), "operand"), (None, lambda u: fill(u.imm_be32[0], (1).to_bytes(32, "big")), "beside a row"),
             (None, lambda u: (idx("in_", 0, I_)(u), fill(u.imm_be32[0], big)), "immediates must be canonical"),
             (None, idx("expect", 0, 0), "expect"), (None, idx("out_order", 0, 1), "out_order"),
             (None, idx("out_order", 1, 0), "out_order"), (None, idx("out_order", 0, A_), "out_order"),
             (None, lambda u: (setattr(u, "flags", 1), idx("expect", 0, 0)(u)), "out_order"),
             (None, lambda u: (setattr(u, "mode", 2), setattr(u, "flags", 1)), "not to CHAIN"),
             (None, lambda u: (setattr(u, "mode", 2), idx("in_", 2, A_)(u), idx("in_", 3, A_)(u)), "op belongs"),
             (None, lambda u: (setattr(u, "mode", 2), idx("in_", 2, A_)(u), idx("in_", 3, A_)(u), setattr(u, "op", I_)), "op must be a row")]
    for mc, mu, why in cases:
        cs, arr = HipEngine.edwards_structs(cv, recs)
        if mc:
            mc(cs)
        if mu:
            mu(arr[0])
        rc = lib.kzg_rows_commit_edwards(fake, 1, hi, ctypes.byref(cs), 1, arr, None, c, *st, ctypes.byref(h))
        msg = lib.kzg_last_error(fake).decode()
        assert rc == _native.KZG_E_ARG and msg.startswith("edwards: ") and why in msg, (why, rc, msg)
    cs, arr = HipEngine.edwards_structs(cv, recs)
    assert lib.kzg_rows_commit_edwards(fake, 0, hi, ctypes.byref(cs), 1, arr, None, c, *st, ctypes.byref(h)) == _native.KZG_E_ARG
    assert lib.kzg_rows_commit_edwards(fake, 1, hi, ctypes.byref(cs), 5, arr, None, c, *st, ctypes.byref(h)) == _native.KZG_E_ARG
    assert lib.kzg_last_error(fake).decode().startswith("edwards: n_units")
    assert lib.kzg_rows_commit_edwards(fake, 1, hi, None, 1, arr, None, c, *st, ctypes.byref(h)) == _native.KZG_E_ARG
    assert lib.kzg_rows_commit_edwards(None, 1, hi, ctypes.byref(cs), 1, arr, None, c, *st, ctypes.byref(h)) == _native.KZG_E_ARG


# ---------------------------------------------------------------------------------------------------- the header
def test_struct_layout_against_the_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct kzg_edwards_unit \{(.*?)\} kzg_edwards_unit;", text, re.S).group(1)
    fields = re.findall(r"^\s*(uint32_t|uint8_t)\s+(\w+)((?:\[\d+\])*);", body, re.M)
    assert [(n, ty, [int(k) for k in re.findall(r"\d+", dims)]) for ty, n, dims in fields] == [
        ("mode", "uint32_t", []), ("flags", "uint32_t", []), ("cols", "uint32_t", []), ("op", "uint32_t", []),
        ("in", "uint32_t", [4]), ("expect", "uint32_t", [2]), ("out_order", "uint32_t", [2]), ("imm_be32", "uint8_t", [4, 32])]
    assert [n.rstrip("_") for n, _ in _native.EdwardsUnit._fields_] == [n for _, n, _ in fields]
    assert ctypes.sizeof(_native.EdwardsUnit) == 48 + 128 and _native.EdwardsUnit.imm_be32.offset == 48
    assert _native.EdwardsUnit.in_.offset == 16 and _native.EdwardsUnit.expect.offset == 32 and _native.EdwardsUnit.out_order.offset == 40
    body = re.search(r"typedef struct kzg_edwards_curve \{(.*?)\} kzg_edwards_curve;", text, re.S).group(1)
    assert re.findall(r"uint8_t\s+(\w+)\[32\];", body) == ["a_be32", "d_be32"] == [n for n, _ in _native.EdwardsCurve._fields_]
    assert ctypes.sizeof(_native.EdwardsCurve) == 64


def test_header_constants_symbols_and_wording():
    text = open(HEADER).read()
    for name in ("KZG_EDWARDS_ADD", "KZG_EDWARDS_CHAIN", "KZG_EDWARDS_CHECK", "KZG_EDWARDS_IMM", "KZG_EDWARDS_ABSENT",
                 "KZG_EDWARDS_NONE", "KZG_EDWARDS_MAX_UNITS"):
        m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, text)
        assert m and int(m.group(1), 0) == getattr(_native, name), name
    for names, macros in ((_native.KZG_EDWARDS_ADD_NAMES, ("X3", "Y3")), (_native.KZG_EDWARDS_CHAIN_NAMES, ("AX", "AY"))):
        for k, macro in enumerate(macros):
            m = re.search(r"#define\s+KZG_EDWARDS_%s\s+(\d+)u" % macro, text)
            assert m and int(m.group(1)) == 1 << k, macro
    assert _native.KZG_EDWARDS_ADD_NAMES == er.ADD_NAMES and _native.KZG_EDWARDS_CHAIN_NAMES == er.CHAIN_NAMES
    for sym in ("kzg_rows_commit_edwards", "kzg_multi_rows_commit_edwards"):
        assert sym in _native.SYMBOLS and re.search(r"\bint %s\(" % sym, text)
    one, twin = _native.SYMBOLS["kzg_rows_commit_edwards"][1], _native.SYMBOLS["kzg_multi_rows_commit_edwards"][1]
    assert len(twin) == len(one) + 1 == 17 and twin[0] == one[0] and twin[2:] == one[1:]
    call = text[text.index("THE NATIVE TWISTED-EDWARDS COLUMNS"):text.index("#define KZG_EDWARDS_ADD")]
    for word in ("OUT OF SCOPE: Montgomery and short-Weierstrass forms over Fr", "a per-row scalar multiplication",
                 "a helper column for tau", "on-curve and subgroup checks", "windowed or\n * signed-digit op-codes beyond 4",
                 "parallelism inside one segment", "SOUNDNESS: nothing here is a proof", "two addition gates",
                 "under the op-code's selector", "The\n * library generates no curve and ships no constant", "2^32 + 2",
                 'begins "edwards:"'):
        assert word in call, word
    # the sibling's scope note points here and keeps its own sentences
    ec = text[text.index("THE NON-NATIVE ELLIPTIC-CURVE COLUMNS"):text.index("#define KZG_EC_DIV")]
    for word in ("Edwards and Montgomery forms; projective coordinates; the point at infinity", "kzg_rows_commit_edwards",
                 "is correct, and slow (DESIGN.md)"):
        assert word in ec, word
    from zkp_subnet_amd import Client, MultiDeviceClient
    assert callable(Client.worker_commit_edwards) and callable(MultiDeviceClient.worker_commit_edwards)
    assert callable(HipEngine.commit_edwards)
    from zkp_subnet_amd.build import SOURCES
    assert "fr_edwards.hip" in SOURCES


# ---------------------------------------------------------------------------------------------------- the kernels' resources
def test_the_kernels_do_not_spill():
    """the compiler's report (-Rpass-analysis=kernel-resource-usage, gfx950): the projective accumulator, the operand and the
    temporaries of the unified addition stay in registers"""
    from tests.test_lookup_sel_resources import report

    rep = {k: v for k, v in report("fr_edwards.hip").items() if "k_edwards" in k}
    assert len(rep) == 2
    for name, r in rep.items():
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)
