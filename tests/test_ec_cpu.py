"""kzg_rows_commit_ec without a GPU.  The reference in Python integers (tests/ec_ref.py) is pinned against identities that do
not come from it: the curve equation and the group law of secp256k1 with its standard generator and order, the known x of
2 G, and (n - 1) G = -G.  Then: the encoder's fields and every refusal, the struct layouts and constants against the header,
and the compiler's report of the kernel."""
import ctypes
import os
import random
import re

import pytest

from tests import ec_ref as er
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import HipEngine

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kzg_mi355x.h")
P, N, G = er.SECP_P, er.SECP_N, (er.SECP_GX, er.SECP_GY)
TWO_G_X = 0xc6047f9441ed7d6d3045406e95c07cd85c778e4b8cef3ca7abac09b95c709ee5


def on_curve(x, y):
    return (y * y - x * x * x - 7) % P == 0


def padd(a, b):
    lam, x3, y3, sing = er.add(er.SECP, a[0], a[1], b[0], b[1])
    assert not sing and on_curve(x3, y3)
    return x3, y3


def mul(k, pt=G):
    acc = None
    for bit in bin(k)[2:]:
        acc = padd(acc, acc) if acc else None
        if bit == "1":
            acc = padd(acc, pt) if acc else pt
    return acc


# ---------------------------------------------------------------------------------------------------- the reference is the group law
def test_the_generator_and_the_double_of_it():
    assert on_curve(*G) and P == 2**256 - 2**32 - 977
    assert padd(G, G)[0] == TWO_G_X and mul(2) == padd(G, G)


def test_addition_commutes_and_associates_on_random_multiples():
    rnd = random.Random(1)
    for _ in range(6):
        a, b, c = (mul(rnd.randrange(1, N)) for _ in range(3))
        assert padd(a, b) == padd(b, a)
        assert padd(padd(a, b), c) == padd(a, padd(b, c))


def chain_columns(ops, T):
    cols = [[0] * T for _ in range(9)]   # px (4 limb rows), py (4), op
    for t, code in enumerate(ops):
        cols[8][t] = code
        if code in (1, 2):
            for l, (a, b) in enumerate(zip(er.limbs(G[0], er.SECP), er.limbs(G[1], er.SECP))):
                cols[l][t], cols[4 + l][t] = a, b
    return cols


CHAIN = {"mode": "chain", "px": 0, "py": 4, "op": 8, "cols": ["ax", "ay", "lam"]}


def test_a_chain_of_n_minus_one_gives_minus_g_and_one_more_add_is_exceptional():
    ops = er.scalar_mul_ops(N - 1) + [2, 0]
    assert len(ops) <= 512
    seen = er.Seen()
    v = er.unit_values(chain_columns(ops, 512), er.SECP, CHAIN, 512, seen)
    k = len(ops) - 2   # the row of the extra add: the accumulator before it is (n - 1) G
    assert (v["ax"][k], v["ay"][k]) == (G[0], P - G[1])
    assert (v["ax"][k + 1], v["ay"][k + 1], v["lam"][k]) == (0, 0, 0)
    assert seen.stats()["singular"] == 1 and seen.stats()["first_singular"] == k and seen.segments == 1
    assert all(on_curve(x, y) for x, y in zip(v["ax"][1:k + 1], v["ay"][1:k + 1]))


def test_chain_equals_repeated_add_and_counts_segments():
    rnd = random.Random(2)
    T = 64
    pts = [mul(rnd.randrange(1, N)) for _ in range(T)]
    ops = [rnd.choice([0, 1, 2, 2, 3, 3]) for _ in range(T)]
    ops[5], ops[9] = 7, (1 << 32) + 2
    cols = [[0] * T for _ in range(9)]
    for t, (x, y) in enumerate(pts):
        for l in range(4):
            cols[l][t], cols[4 + l][t] = er.limbs(x, er.SECP)[l], er.limbs(y, er.SECP)[l]
    cols[8] = ops
    seen = er.Seen()
    v = er.unit_values(cols, er.SECP, CHAIN, T, seen)
    acc = (0, 0)
    for t in range(T):
        assert (v["ax"][t], v["ay"][t]) == acc
        if ops[t] == 1:
            acc = pts[t]
        elif ops[t] in (2, 3):
            q = pts[t] if ops[t] == 2 else acc
            lam, x3, y3, _ = er.add(er.SECP, acc[0], acc[1], q[0], q[1])
            assert v["lam"][t] == lam
            acc = (x3, y3)
        else:
            assert v["lam"][t] == 0
    st = seen.stats()
    assert st["segments"] == len({0} | {t for t in range(T) if ops[t] == 1})
    assert st["unknown"] == 2 and st["first_unknown"] == 5


# ---------------------------------------------------------------------------------------------------- div
@pytest.mark.parametrize("p", [15, 2**61 - 1, P])
def test_div_is_the_inverse_of_the_product_and_singular_rows(p):
    rnd = random.Random(p % 1000)
    cv = {"bits": 64, "limbs": 4, "p": p, "a": 0}
    for _ in range(200):
        a, b = rnd.randrange(p), rnd.randrange(p)
        r, sing = er.div(cv, a, b)
        import math
        assert sing == (math.gcd(b, p) != 1)
        assert r == 0 if sing else r * b % p == a
    assert er.div(cv, 5, 0) == (0, True) and er.div(cv, 5, p) == (0, True)
    if p == 15:
        assert [er.div(cv, 1, b)[1] for b in range(15)] == [b % 3 == 0 or b % 5 == 0 for b in range(15)]


def test_over_range_rows_are_counted_once():
    cv = {"bits": 8, "limbs": 2, "p": 251, "a": 1}
    #        ok   limb    value >= p   both operands bad   value = p
    cols = [[5, 0x100 + 7, 252, 0x1ff, 251],
            [0, 0, 0, 1, 0],
            [3, 3, 3, 0x200 + 3, 3],
            [0, 0, 0, 0, 0]]
    rows, st = er.columns(cols, cv, [{"mode": "div", "a": 0, "b": 2, "out": True}])
    assert st["counts"] == [4] and st["first"] == [1] and st["singular"] == [0]
    assert [rows[0][t] * 3 % 251 for t in range(5)] == [5, 7, 1, (0xff + 256) % 251, 0] and rows[1] == [0] * 5


def test_a_check_counts_rows_not_cells_and_commits_nothing():
    cv = {"bits": 8, "limbs": 1, "p": 251, "a": 0}
    cols = [[10, 20, 30], [2, 4, 5], [5, 5, 7], [5, 6, 1 << 64]]
    rows, st = er.columns(cols, cv, [{"mode": "div", "a": 0, "b": 1, "expect": [2]}, {"mode": "div", "a": 0, "b": 1, "expect": [3]}])
    assert rows == [] and st["mismatch"] == [1, 2] and st["first_mismatch"] == [2, 1]


# ---------------------------------------------------------------------------------------------------- the encoder
CV = {"bits": 64, "limbs": 4, "p": P, "a": 0}
DIV = {"mode": "div", "a": 0, "b": 4, "out": True}
ADD = {"mode": "add", "x1": 0, "y1": 4, "x2": 8, "y2": 12, "out": ["lam", "x3", "y3"]}
SMALL = {"bits": 8, "limbs": 1, "p": 251, "a": 3}


def test_the_encoder_fills_the_struct_fields():
    A = _native.KZG_EC_ABSENT
    cv, recs = HipEngine.ec_call(dict(CV, p=hex(P)), [dict(DIV, b=("imm", 7)), {"mode": "add", "x1": 0, "y1": 4, "x2": 0, "y2": 4, "expect": [None, 8, 12]},
                                                      dict(CHAIN, cols=["lam", "ax"])])
    assert cv == (64, 4, P, 0)
    assert recs[0] == (_native.KZG_EC_DIV, _native.KZG_EC_IMM_B, 1, A, [0, A, A, A], [A, A, A], 7)
    assert recs[1] == (_native.KZG_EC_ADD, _native.KZG_EC_CHECK, 6, A, [0, 4, 0, 4], [A, 8, 12], 0)
    assert recs[2] == (_native.KZG_EC_CHAIN, 0, 5, 8, [0, 4, A, A], [A, A, A], 0)
    assert HipEngine.ec_n_out(cv, recs) == 4 + 0 + 8
    cs, arr = HipEngine.ec_structs(cv, recs)
    assert (cs.bits, cs.limbs, cs.p[0], cs.p[3], cs.a[0]) == (64, 4, P & (2**64 - 1), 2**64 - 1, 0)
    assert (arr[0].mode, arr[0].flags, arr[0].imm[0], arr[0].in_[1], arr[2].op, arr[2].cols, arr[1].expect[2]) == (1, 2, 7, A, 8, 5, 12)


@pytest.mark.parametrize("curve,units,why", [
    (CV, [], "n_units"), (CV, [DIV] * 5, "n_units"), (CV, "x", "n_units"), (CV, [5], "a unit is a mapping"),
    (5, [DIV], "the curve is a mapping"), (dict(CV, c=7), [DIV], "unknown field 'c' of the curve"),
    (dict(CV, bits=0), [DIV], "limb width b"), (dict(CV, bits=65), [DIV], "limb width b"),
    (dict(CV, limbs=0), [DIV], "number of limbs L"), (dict(CV, limbs=5), [DIV], "number of limbs L"),
    (dict(CV, bits=52, limbs=4, p=P), [DIV], "below 2^W"), ({"bits": 64, "limbs": 4, "p": P}, [DIV], "must give the modulus"),
    (dict(CV, bits=64, limbs=4, p=P - 1), [DIV], "odd"), (dict(CV, p=1), [DIV], "odd and at least 3"),
    (dict(CV, p="zz"), [DIV], "decimal or 0x string"), (dict(CV, p=-3), [DIV], "non-negative"),
    (dict(SMALL, p=257), [DIV], "below 2^W"), (dict(SMALL, a=251), [DIV], "a must be below p"),
    ({"bits": 33, "limbs": 8, "p": 3, "a": 0}, [DIV], "number of limbs L"), ({"bits": 65, "limbs": 4, "p": 3, "a": 0}, [DIV], "limb width"),
    ({"bits": 60, "limbs": 4, "p": 3, "a": 0}, [DIV], None), (dict(CV, bits=64, limbs=4), [dict(DIV, mode="sub")], "unknown mode"),
    (CV, [dict(DIV, foo=1)], "unknown field"), (CV, [dict(DIV, x1=0)], "unknown field"), (CV, [dict(ADD, a=0)], "unknown field"),
    (CV, [dict(CHAIN, out=["ax"])], "unknown field"), (CV, [dict(CHAIN, expect=[0])], "expect belongs to div and add"),
    (CV, [dict(DIV, a=None)], "a must be a first row"), (CV, [dict(DIV, a=-1)], "a must be a first row"),
    (CV, [dict(DIV, b=("im", 1))], "immediate is"), (CV, [dict(DIV, b=("imm", 1 << 256))], "immediate must be below 2^W"),
    (SMALL, [dict(DIV, a=0, b=("imm", 256))], "immediate must be below 2^W"), (CV, [dict(DIV, b=("imm", "q"))], "decimal or 0x"),
    (CV, [dict(DIV, expect=[8])], "out together with expect"), (CV, [{"mode": "div", "a": 0, "b": 4}], "needs out, or expect"),
    (CV, [{"mode": "div", "a": 0, "b": 4, "expect": [8, 12]}], "wrong number of expect rows"),
    (CV, [{"mode": "add", "x1": 0, "y1": 4, "x2": 8, "y2": 12, "expect": [0]}], "wrong number of expect rows"),
    (CV, [{"mode": "add", "x1": 0, "y1": 4, "x2": 8, "y2": 12, "expect": [None] * 3}], "at least one"),
    (CV, [{"mode": "div", "a": 0, "b": 4, "expect": ["x"]}], "an entry of expect"), (CV, [dict(DIV, out=["r"])], "out of a div unit is True"),
    (CV, [dict(ADD, out=[])], "out must hold"), (CV, [dict(ADD, out=["ax"])], "unknown name"), (CV, [dict(ADD, out=["x3", "x3"])], "repeated"),
    (CV, [dict(ADD, y2=None)], "y2 must be a first row"), (CV, [dict(CHAIN, cols=[])], "cols must hold"),
    (CV, [dict(CHAIN, cols=["x3"])], "unknown name"), (CV, [dict(CHAIN, op=None)], "op must be"),
    (CV, [ADD, DIV], None), (CV, [ADD, DIV, dict(DIV, a=4, b=8)], "n_out"),(CV, [ADD, dict(CHAIN, px=16, py=20, op=24, cols=["lam"])], "distinct input rows"),
    (CV, [ADD, {"mode": "div", "a": 0, "b": 4, "expect": [13]}], "distinct input rows"),
    (CV, [ADD, {"mode": "div", "a": 0, "b": 4, "expect": [12]}], None),
    (SMALL, [dict(ADD, x1=0, y1=1, x2=2, y2=3)] * 4 + [], None),
])
def test_python_refusals(curve, units, why):
    if why is None:
        assert len(HipEngine.ec_call(curve, units)[1]) == len(units)
        return
    with pytest.raises(KzgError) as ei:
        HipEngine.ec_call(curve, units)
    assert ei.value.code == _native.KZG_E_ARG and "ec: " in str(ei.value) and why in str(ei.value), str(ei.value)


def test_an_operand_run_beyond_the_concatenation_is_refused_where_the_length_is_known():
    assert HipEngine.ec_call(CV, [ADD], n_rows=16)
    for units in ([ADD], [dict(DIV, b=12)], [dict(CHAIN, op=15)], [{"mode": "div", "a": 0, "b": 4, "expect": [12]}]):
        with pytest.raises(KzgError) as ei:
            HipEngine.ec_call(CV, units, n_rows=15)
        assert "reaches beyond the 15 concatenated rows" in str(ei.value)


# ---------------------------------------------------------------------------------------------------- the header
def fields_of(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    return [(n, ctype[ty], int(k) if k else 1) for ty, n, k in re.findall(r"^\s*(uint32_t|uint64_t)\s+(\w+)(?:\[(\d+)\])?;", body, re.M)]


@pytest.mark.parametrize("name,struct,size,count", [("kzg_ec_curve", _native.EcCurve, 72, 4), ("kzg_ec_unit", _native.EcUnit, 80, 8)])
def test_struct_layout_against_the_header(name, struct, size, count):
    want = fields_of(open(HEADER).read(), name)
    is_array = lambda ty: issubclass(ty, ctypes.Array)   # noqa: E731
    got = [(n.rstrip("_"), ty._type_ if is_array(ty) else ty, ty._length_ if is_array(ty) else 1) for n, ty in struct._fields_]
    assert got == want and len(want) == count

    class InC(ctypes.Structure):   # the header's fields laid out by the C rules
        _fields_ = [(n, ty * k if k > 1 else ty) for n, ty, k in want]

    assert ctypes.sizeof(struct) == ctypes.sizeof(InC) == size
    for n, _ in struct._fields_:
        assert getattr(struct, n).offset == getattr(InC, n.rstrip("_")).offset, n


def test_header_constants_and_symbols():
    text = open(HEADER).read()
    for name in ("KZG_EC_DIV", "KZG_EC_ADD", "KZG_EC_CHAIN", "KZG_EC_CHECK", "KZG_EC_IMM_B", "KZG_EC_ABSENT", "KZG_EC_NONE",
                 "KZG_EC_MAX_UNITS", "KZG_EC_MAX_LIMBS"):
        m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, text)
        assert m and int(m.group(1), 0) == getattr(_native, name), name
    for names, macros in ((_native.KZG_EC_ADD_NAMES, ("LAM", "X3", "Y3")), (_native.KZG_EC_CHAIN_NAMES, ("AX", "AY", "CLAM"))):
        for k, macro in enumerate(macros):
            m = re.search(r"#define\s+KZG_EC_%s\s+(\d+)u" % macro, text)
            assert m and int(m.group(1)) == 1 << k, macro
        assert len(names) == 3
    assert _native.KZG_EC_ADD_NAMES == er.ADD_NAMES and _native.KZG_EC_CHAIN_NAMES == er.CHAIN_NAMES
    for sym in ("kzg_rows_commit_ec", "kzg_multi_rows_commit_ec"):
        assert sym in _native.SYMBOLS and re.search(r"\bint %s\(" % sym, text)
    assert len(_native.SYMBOLS["kzg_multi_rows_commit_ec"][1]) == len(_native.SYMBOLS["kzg_rows_commit_ec"][1]) + 1
    for word in ("OUT OF SCOPE: L > 4", "projective coordinates", "the point at infinity", "on-curve check", "per-row moduli",
                 "nothing here is a proof", "they have their own call, the DIV unit of\n * kzg_rows_commit_ec"):
        assert word in text, word
    from zkp_subnet_amd import Client, MultiDeviceClient
    assert callable(Client.worker_commit_ec) and callable(MultiDeviceClient.worker_commit_ec)
    assert callable(HipEngine.commit_ec)


# ---------------------------------------------------------------------------------------------------- the kernel's resources
def test_the_kernel_does_not_spill():
    """the compiler's report (-Rpass-analysis=kernel-resource-usage, gfx950): the operands and the four values of the inversion
    stay in registers"""
    from tests.test_lookup_sel_resources import report

    rep = {k: v for k, v in report("fr_ec.hip").items() if "k_fr_ec" in k}
    assert len(rep) == 1
    for name, r in rep.items():
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)
