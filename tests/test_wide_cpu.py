"""kzg_rows_commit_wide without a GPU: the reference in Python integers (tests/wide_ref.py) against the identities it must
satisfy, the word-level model of the kernel's long division and the paths its test vectors take, the op encoder, every refusal
the Python layer makes, and the header's constants against _native.py."""
import ctypes
import os
import random
import re

import pytest

from tests import wide_ref as wr
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import HipEngine

SHAPES = [(1, 1), (8, 4), (29, 5), (32, 8), (64, 4), (64, 8), (56, 8)]
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kzg_mi355x.h")


def edge_values(W, m, rnd, n=40):
    top = (1 << W) - 1
    es = [0, 1, top, (m - 1) & top, m & top, (m + 1) & top]
    return es + [rnd.getrandbits(rnd.randrange(1, W + 1)) for _ in range(n)]


def limb_cols(vals, b, L):
    return [[(v >> (b * l)) & ((1 << b) - 1) for v in vals] for l in range(L)]


def value_at(rows, t, b):
    return sum(r[t] << (b * l) for l, r in enumerate(rows))


def moduli(W, rnd):
    out = [1, (1 << W) - 1, rnd.getrandbits(W) | 1]
    if W >= 256:
        out.append(wr.SECP256K1_P)
    if W >= 384:
        out.append(wr.BLS12_381_P)
    return [m for m in out if 1 <= m < 1 << W]


# ---------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("b,L", SHAPES)
def test_reference_identities(b, L):
    rnd = random.Random(100 * b + L)
    W = b * L
    for m in moduli(W, rnd):
        av, bv = edge_values(W, m, rnd), list(reversed(edge_values(W, m, rnd)))
        T = len(av)
        cols = limb_cols(av, b, L) + limb_cols(bv, b, L)
        base = dict(bits=b, limbs=L, a=0, b=L)
        rows, st = wr.wide_columns(cols, [dict(base, kind="add", count=L + 1), dict(base, kind="sub", count=L + 1),
                                          dict(base, kind="mul", count=2 * L), dict(base, kind="divmod", count=2 * L)])
        assert st["counts"] == [0] * 4 and st["qover"] == [0] * 4
        add, sub, mul, dm = rows[:L + 1], rows[L + 1:2 * L + 2], rows[2 * L + 2:4 * L + 2], rows[4 * L + 2:]
        for t in range(T):
            x, y = av[t], bv[t]
            assert value_at(add[:L], t, b) + (add[L][t] << W) == x + y and add[L][t] in (0, 1)
            assert value_at(sub[:L], t, b) - (sub[L][t] << W) == x - y and sub[L][t] == int(x < y)
            assert value_at(mul, t, b) == x * y
            q, rem = value_at(dm[:L], t, b), value_at(dm[L:], t, b)
            assert (x == q * y + rem and rem < y) if y else (q, rem) == ((1 << W) - 1, x)
        for neg in (False, True):
            op = dict(base, kind="mulmod", m=m, c=L, neg_c=neg, count=2 * L)
            rows, st = wr.wide_columns(cols, [op])
            for t in range(T):
                x, y, c = av[t], bv[t], bv[t]
                d = m - (c % m) if neg else c
                r, q = value_at(rows[:L], t, b), value_at(rows[L:], t, b)
                full_q = (x * y + d) // m
                assert r < m and x * y + d == full_q * m + r and q == full_q % (1 << W)
                assert 1 <= d <= m if neg else d == c
            assert st["qover"][0] == sum(1 for t in range(T) if (av[t] * bv[t] + (m - bv[t] % m if neg else bv[t])) // m >> W)
            assert st["counts"][0] == (sum(1 for c in bv if c > m) if neg else 0)


@pytest.mark.parametrize("b,L", [s for s in SHAPES if s[0] <= 56])
def test_the_carry_recurrence_closes_exactly_on_the_reference_quotient_and_remainder(b, L):
    rnd = random.Random(200 * b + L)
    W = b * L
    for m in moduli(W, rnd):
        av = [x % m for x in edge_values(W, m, rnd)]
        bv = [x % m for x in reversed(edge_values(W, m, rnd))]
        cv = [rnd.randrange(m + 1) for _ in av]
        cv[:2] = [0, m]
        for neg in (False, True):
            cols = limb_cols(av, b, L) + limb_cols(bv, b, L) + limb_cols(cv, b, L)
            rq, _ = wr.wide_columns(cols, [dict(kind="mulmod", bits=b, limbs=L, a=0, b=L, c=2 * L, m=m, neg_c=neg, count=2 * L)])
            cols += rq                                               # r at 3 L, q at 4 L
            op = dict(kind="carry", bits=b, limbs=L, a=0, b=L, c=2 * L, r=3 * L, q=4 * L, m=m, neg_c=neg)
            rows, st = wr.wide_columns(cols, [op])
            assert len(rows) == 2 * L - 1 and st["qover"] == [0] and st["counts"] == [0]
            signed = [[v if v < wr.R // 2 else v - wr.R for v in row] for row in rows]
            assert all(-(1 << 63) <= v < 1 << 63 for row in signed for v in row)
            cols[3 * L][4] ^= 1                                      # a wrong r: inexact, named
            _, st = wr.wide_columns(cols, [op])
            assert st["qover"] == [1] and st["first_qover"] == [4]


def test_out_of_range_limbs_are_reduced_and_counted_once_per_row():
    b, L, T = 8, 2, 8
    cols = [[1] * T, [2] * T, [3] * T, [4] * T]
    cols[0][2] = 256 + 7
    cols[1][2] = wr.R - 1
    cols[3][5] = 1 << 200
    rows, st = wr.wide_columns(cols, [dict(kind="add", bits=b, limbs=L, a=0, b=2), dict(kind="mul", bits=b, limbs=L, a=0, b=0)])
    assert st["counts"] == [2, 1] and st["first"] == [2, 2]
    assert rows[0][2] == (7 + 3) % 256 and rows[0][5] == 4
    rows, st = wr.wide_columns(cols, [dict(kind="add", bits=b, limbs=L, a=0, b=2)], 2, [9, 10, 11, 12, 13, 14] * 2)
    assert st["counts"] == [0] and rows[0][2:] == [9, 10, 11, 12, 13, 14] and rows[1][2:] == [9, 10, 11, 12, 13, 14]


# ---------------------------------------------------------------------------------------------------- the long division
@pytest.mark.parametrize("N", [4, 8, 16])
def test_division_model_and_the_paths_of_its_vectors(N):
    rnd = random.Random(300 + N)
    for _ in range(400):
        v = rnd.getrandbits(rnd.randrange(1, 32 * N + 1)) or 1
        u = rnd.getrandbits(rnd.randrange(1, 64 * N + 1))
        q, r, _ = wr.knuth_divrem(u, v, N)
        assert (q, r) == divmod(u, v)
    seen = set()
    W = 32 * N
    for u, v, path in wr.division_vectors(N):
        q, r, paths = wr.knuth_divrem(u, v, N)
        assert (q, r) == divmod(u, v) and (path is None or path in paths), (path, paths)
        seen |= paths
        # the dividend a GPU mulmod really divides, a b + c, takes the path too (the all-ones dividend aside)
        a, bq, c = wr.mulmod_operands(u, W)
        if a * bq + c == u:
            assert path is None or path in wr.knuth_divrem(a * bq + c, v, N)[2]
        # and divmod divides each half
        for half in (u >> W, u & ((1 << W) - 1)):
            assert wr.knuth_divrem(half, v, N)[:2] == divmod(half, v)
    assert {"shift0", "shift31", "cap", "fix", "fix2", "addback"} <= seen
    one_word = [v for _, v, _ in wr.division_vectors(N) if v < 1 << 32]
    assert len(one_word) == 2
    mm = [wr.mulmod_operands(u, W) for u, v, p in wr.division_vectors(N) if p in ("fix", "addback")]
    assert all(a * b + c == u for (a, b, c), (u, v, p) in zip(mm, [x for x in wr.division_vectors(N) if x[2] in ("fix", "addback")]))


# ---------------------------------------------------------------------------------------------------- the encoder
def test_op_encoder():
    p = wr.SECP256K1_P
    recs = HipEngine.wide_ops([dict(kind="mulmod", bits=32, limbs=8, a=0, b=8, m=hex(p), count=16)])
    recs += HipEngine.wide_ops([dict(kind="carry", bits=32, limbs=2, a=0, b=("imm", "7"), q=2, r=4, c=6, m=11, neg_c=True),
                                dict(kind="add", bits=64, limbs=8, a=3, b=("imm", (1 << 512) - 1), count=9),
                                dict(kind="mulmod", bits=8, limbs=1, a=1, m=255)])
    NO = _native.KZG_WIDE_ABSENT
    assert recs[0] == (_native.KZG_WIDE_MULMOD, 32, 8, 16, 0, 0, 8, NO, NO, NO, bytes(64), p.to_bytes(64, "big"))
    assert recs[1] == (_native.KZG_WIDE_CARRY, 32, 2, 3, _native.KZG_WIDE_IMM_B | _native.KZG_WIDE_NEG_C, 0, NO, 6, 2, 4,
                       (7).to_bytes(64, "big"), (11).to_bytes(64, "big"))
    assert recs[2] == (_native.KZG_WIDE_ADD, 64, 8, 9, _native.KZG_WIDE_IMM_B, 3, NO, NO, NO, NO, b"\xff" * 64, bytes(64))
    assert recs[3][3] == 1 and recs[3][6] == NO and recs[3][4] == 0
    st = HipEngine.wide_op_struct(recs[1])
    assert (st.kind, st.bits, st.limbs, st.count, st.flags, st.a, st.b, st.c, st.q, st.r) == recs[1][:10]
    assert bytes(st.imm_be64) == recs[1][10] and bytes(st.m_be64) == recs[1][11]
    assert ctypes.sizeof(_native.WideOp) == 40 + 128


OK = dict(kind="mulmod", bits=32, limbs=4, a=0, b=4, m=97)


@pytest.mark.parametrize("ops,why", [
    ([], "n_ops"), ([OK] * 9, "n_ops"), ("x", "n_ops"), ([dict(OK, count=8)] * 3, "n_out"), ([5], "mapping"),
    ([dict(OK, kind="nand")], "unknown kind"), ([dict(OK, kind=3)], "unknown kind"), ([dict(OK, foo=1)], "unknown field"),
    ([dict(OK, bits=0)], "limb width"), ([dict(OK, bits=65)], "limb width"), ([dict(OK, bits=True)], "limb width"),
    ([dict(OK, limbs=0)], "number of limbs"), ([dict(OK, limbs=9)], "number of limbs"),
    ([dict(OK, bits=64, limbs=8, kind="carry", q=0, r=0)], "at most 56"), ([dict(OK, bits=57, kind="carry", q=0, r=0)], "at most 56"),
    ([dict(OK, count=5)], "count must be"), ([dict(OK, kind="add", m=None, count=8)], "count must be"),
    ([dict(OK, kind="carry", q=0, r=0, count=8)], "count must be"),
    ([dict(OK, a=None)], "operand a"), ([dict(OK, a=-1)], "operand a"), ([dict(OK, c="x")], "operand c"),
    ([dict(OK, b=("im", 1))], "immediate is"), ([dict(OK, b=("imm", 1 << 128))], "immediate must be below"),
    ([dict(OK, b=("imm", "zz"))], "decimal or 0x"), ([dict(OK, b=("imm", -1))], "non-negative"),
    ([dict(OK, kind="mul", m=None, b=None)], "operand b must be given"),
    ([dict(OK, m=None)], "m must be given"), ([dict(OK, m=0)], "must not be 0"), ([dict(OK, m=1 << 128)], "below 2^W"),
    ([dict(OK, neg_c=1)], "boolean"),
    ([dict(OK, kind="add")], "does not take"), ([dict(OK, kind="sub", m=None, c=0)], "does not take"),
    ([dict(OK, kind="divmod", m=None, neg_c=True)], "does not take"), ([dict(OK, q=0)], "does not take"),
    ([dict(OK, kind="mul", m=None, r=0)], "does not take"), ([dict(OK, kind="carry", q=0)], "q and r must be given"),
])
def test_python_refusals(ops, why):
    with pytest.raises(KzgError) as ei:
        HipEngine.wide_ops(ops)
    assert ei.value.code == _native.KZG_E_ARG and "wide: " in str(ei.value) and why in str(ei.value), str(ei.value)


def test_header_constants_and_symbols():
    text = open(HEADER).read()
    for name in ("KZG_WIDE_ADD", "KZG_WIDE_SUB", "KZG_WIDE_MUL", "KZG_WIDE_DIVMOD", "KZG_WIDE_MULMOD", "KZG_WIDE_CARRY",
                 "KZG_WIDE_IMM_B", "KZG_WIDE_NEG_C", "KZG_WIDE_ABSENT", "KZG_WIDE_MAX_OPS", "KZG_WIDE_MAX_LIMBS"):
        m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, text)
        assert m and int(m.group(1), 0) == getattr(_native, name), name
    for sym in ("kzg_rows_commit_wide", "kzg_multi_rows_commit_wide"):
        assert sym in _native.SYMBOLS and re.search(r"\bint %s\(" % sym, text)
    assert len(_native.SYMBOLS["kzg_multi_rows_commit_wide"][1]) == len(_native.SYMBOLS["kzg_rows_commit_wide"][1]) + 1
    for word in ("OUT OF SCOPE: L > 8", "a per-row modulus", "modular inversion and division", "signed operands", "an op-code column"):
        assert word in text
    from zkp_subnet_amd import Client, MultiDeviceClient
    assert callable(Client.worker_commit_wide) and callable(MultiDeviceClient.worker_commit_wide)
    assert callable(HipEngine.commit_wide)
