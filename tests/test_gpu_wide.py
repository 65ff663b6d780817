"""GPU tests (`-m gpu`) of kzg_rows_commit_wide: multi-limb add, sub, mul, divmod, mulmod and the carry columns of the limb
identity, computed from runs of resident limb rows and committed on the device.  The expected rows come from the definition
in Python integers (tests/wide_ref.py).  Every case is bit-exact two ways: the commitments against commit_rows of the reference
rows, and every cell through read_rows; the four statistics are compared exactly.  Row lengths 2^5 .. 2^10.  A call reads at
most 16 concatenated rows (the limit of every builder): a carry with a, q and r on DISTINCT runs of rows has L <= 5 (L <= 4
with b as a row too), and at L = 6 .. 8 a row serves several operands (test_carry_at_full_length_over_shared_operand_rows)."""
import ctypes
import random

import pytest

from tests import wide_ref as wr
from tests.gpu_common import R, be, row_bytes
from tests.gpu_rows import arg_error, bt, commit_sets, engine_cache, release
from zkp_subnet_amd import _native

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x51DE0001, 0x51DE0002
SHAPES = [(1, 1), (8, 4), (29, 5), (32, 8), (64, 4), (64, 8)]
MODULI = {256: wr.SECP256K1_P, 512: wr.BLS12_381_P}


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


def sizes_of(k):
    return tuple([16] * (k // 16) + ([k % 16] if k % 16 else []))


def read_all(eng, rset):
    T = rset.T
    out = []
    for c in range(rset.k):
        raw = eng.read_rows([rset], c, 0, T, "fr")[0]
        out.append([int.from_bytes(raw[32 * t:32 * t + 32], "big") for t in range(T)])
    return out


def run(eng, cols, ops, usable=None, tail=(), sizes=None):
    """commit `cols`, build on the device, compare commitments, cells and statistics with the reference; returns (rows, stats)"""
    want, stats = wr.wide_columns(cols, ops, usable, tail)
    S = commit_sets(eng, cols, sizes or sizes_of(len(cols)))
    try:
        out, got = eng.commit_wide(S, ops, usable, bt(tail))
        try:
            assert got == stats, (got, stats)
            assert read_all(eng, out) == want
            ref = eng.commit_rows(0, [row_bytes(r) for r in want])
            try:
                assert out.commitments == ref.commitments
            finally:
                ref.release()
        finally:
            out.release()
    finally:
        release(S)
    return want, stats


def wide_cols(vals, b, L):
    """the L limb columns of a list of values"""
    return [[(v >> (b * l)) & ((1 << b) - 1) for v in vals] for l in range(L)]


def operands(T, W, m, rnd):
    """T operand pairs: the edges 0, 1, 2^W - 1, m - 1, m, m + 1 against each other first, then random ones of every length"""
    top = (1 << W) - 1
    es = sorted({0, 1, top, (m - 1) & top, m & top, (m + 1) & top})
    pairs = [(x, y) for x in es for y in es]
    while len(pairs) < T:
        pairs.append((rnd.getrandbits(rnd.randrange(1, W + 1)), rnd.getrandbits(rnd.randrange(1, W + 1))))
    rnd.shuffle(pairs)
    return [p[0] for p in pairs[:T]], [p[1] for p in pairs[:T]]


# ---------------------------------------------------------------------------------------------------- every kind
@pytest.mark.parametrize("b,L", SHAPES)
def test_every_kind(engines, b, L):
    """add, sub, mul, divmod and mulmod with all their rows in one call, and with the first part alone in another; the operands
    hold the edges, zero divisors among them"""
    lg = 5 if L == 1 else 6
    eng, T, W = engines(lg), 1 << lg, b * L
    before = eng.rows_stats()
    rnd = random.Random(1000 * b + L)
    m = MODULI.get(W, ((1 << W) - 1) if W < 3 else rnd.getrandbits(W) | (1 << (W - 1)) | 1)
    av, bv = operands(T, W, m, rnd)
    cols = wide_cols(av, b, L) + wide_cols(bv, b, L)
    base = dict(bits=b, limbs=L, a=0, b=L)
    full = [dict(base, kind="add", count=L + 1), dict(base, kind="sub", count=L + 1), dict(base, kind="mul", count=2 * L),
            dict(base, kind="divmod", count=2 * L), dict(base, kind="mulmod", count=2 * L, m=m, c=0),
            dict(base, kind="mulmod", count=2 * L, m=m, c=L, neg_c=True)]
    per_call = max(1, 16 // (2 * L))
    for o in range(0, len(full), per_call):
        run(eng, cols, full[o:o + per_call])
    first = [dict(op, count=L) for op in full]
    for o in range(0, len(first), 16 // L):
        run(eng, cols, first[o:o + 16 // L])
    assert eng.rows_stats() == before


@pytest.mark.parametrize("b,L,wide", [(1, 1, None), (8, 3, None), (8, 4, None), (29, 5, None), (32, 4, None), (56, 4, None),
                                      (56, 5, None), (56, 4, (64, 4)), (56, 4, (64, 8))])
def test_carry_closes_on_the_quotient_and_remainder_of_mulmod(engines, b, L, wide):
    """carry fed the q and r of the reference's mulmod: exact; with one r cell changed the row is inexact.  b is a row where
    four operands fit the 16 rows of a call (and c a fifth where five do), else an immediate; `wide` adds an op over the same
    rows that selects a wider instantiation of the kernel"""
    lg = 5
    eng, T, W = engines(lg), 1 << lg, b * L
    before = eng.rows_stats()
    rnd = random.Random(2000 * b + L + (wide[1] if wide else 0))
    m = 1 if W < 3 else rnd.getrandbits(W) | (1 << (W - 1)) | 1
    av, bv = operands(T, W, m, rnd)
    av, bv = [x % m for x in av], [x % m for x in bv]
    b_row, has_c = 4 * L <= 16, 5 * L <= 16
    kb = rnd.randrange(m)
    cv = [rnd.randrange(m + 1) for _ in range(T)] if has_c else [0] * T
    cv[:2] = [0, m] if has_c else cv[:2]
    for neg in (False, True):
        d = [(m - (c % m)) if neg else c for c in cv]
        t = [x * (y if b_row else kb) + dd for x, y, dd in zip(av, bv, d)]
        cols = wide_cols(av, b, L) + wide_cols([x // m for x in t], b, L) + wide_cols([x % m for x in t], b, L)
        op = dict(kind="carry", bits=b, limbs=L, a=0, q=L, r=2 * L, m=m, neg_c=neg, b=("imm", kb))
        if b_row:
            cols += wide_cols(bv, b, L)
            op.update(b=3 * L)
        if has_c:
            cols += wide_cols(cv, b, L)
            op.update(c=4 * L)
        ops = [op] + ([dict(kind="add", bits=wide[0], limbs=wide[1], a=0, b=0, count=wide[1])] if wide else [])
        want, stats = run(eng, cols, ops)
        assert stats["qover"][0] == 0 and stats["counts"][0] == 0
        for k in range(2 * L - 1):                                   # s_k = carry_k 2^b: the last carry row closes the identity
            assert all(-(1 << 63) <= (v if v < R // 2 else v - R) < 1 << 63 for v in want[k])
        bad = [list(c) for c in cols]
        bad[2 * L][3] ^= 1
        want, stats = run(eng, bad, ops)
        assert stats["qover"][0] == 1 and stats["first_qover"][0] == 3
    assert eng.rows_stats() == before


@pytest.mark.parametrize("b,L", [(56, 8), (56, 7), (56, 6), (32, 8), (8, 8)])
def test_carry_at_full_length_over_shared_operand_rows(engines, b, L):
    """carry at L = 6 .. 8, where a, q and r as distinct runs of rows pass the 16 rows of a call: a row serves several operands.
    a = q = r with b = m + 1 is exact (a (m + 1) = a m + a); a apart from q = r is exact on the rows where the second run
    repeats the first and inexact elsewhere, the carries compared cell for cell all the same; neg_c with c on a's rows holds
    values above m, which are counted and reduced by the division; b as a row on a's rows.  (56, L >= 6) runs the 16-word
    instantiation, (32, 8) the 8-word and (8, 8) the 4-word one"""
    lg = 5
    eng, T, W = engines(lg), 1 << lg, b * L
    before = eng.rows_stats()
    rnd = random.Random(2500 * b + L)
    m = (rnd.getrandbits(W) | (1 << (W - 1)) | 1) & ~2                # m + 1 < 2^W
    av = [x % m for x in operands(T, W, m, rnd)[0]]
    base = dict(kind="carry", bits=b, limbs=L, a=0, m=m)
    want, stats = run(eng, wide_cols(av, b, L), [dict(base, q=0, r=0, b=("imm", m + 1))])
    assert len(want) == 2 * L - 1 and stats == {"counts": [0], "first": [None], "qover": [0], "first_qover": [None]}
    negative = any(v > R // 2 for row in want for v in row)
    qv = [x if t % 3 == 0 else rnd.randrange(m) for t, x in enumerate(av)]
    cols = wide_cols(av, b, L) + wide_cols(qv, b, L)
    want, stats = run(eng, cols, [dict(base, q=L, r=L, b=("imm", m + 1))])
    off = [t for t in range(T) if qv[t] != av[t]]
    assert stats["qover"] == [len(off)] and stats["first_qover"] == [off[0]] and stats["counts"] == [0]
    negative |= any(v > R // 2 for row in want for v in row)
    big = [rnd.getrandbits(W) if t % 2 else x for t, x in enumerate(av)]
    cols = wide_cols(big, b, L) + wide_cols(qv, b, L)
    want, stats = run(eng, cols, [dict(base, c=0, q=L, r=L, b=("imm", rnd.randrange(m)), neg_c=True)])
    assert stats["counts"] == [sum(1 for x in big if x > m)] and stats["counts"][0] > 0
    negative |= any(v > R // 2 for row in want for v in row)
    cols[L][7] += 1 << b                                              # a limb of q = r out of range: counted once
    want, stats = run(eng, cols, [dict(base, b=0, c=L, q=L, r=L)])
    assert stats["counts"] == [1] and stats["first"] == [7]
    assert negative or any(v > R // 2 for row in want for v in row)
    assert all(-(1 << 63) <= (v if v < R // 2 else v - R) < 1 << 63 for row in want for v in row)
    assert eng.rows_stats() == before


@pytest.mark.parametrize("b,L", [(8, 4), (29, 5), (32, 8), (64, 4), (64, 8)])
def test_mulmod_at_the_edge_moduli(engines, b, L):
    """m = 1 (a one-word divisor shifted by N - 1 words and 31 bits; every quotient at or above 2^W is counted), m = 2, m =
    2^W - 1, and the curve primes that fit, over the edge operands"""
    lg = 6
    eng, T, W = engines(lg), 1 << lg, b * L
    rnd = random.Random(2700 * b + L)
    moduli = [1, 2, (1 << W) - 1] + [p for p in (wr.SECP256K1_P, wr.BN254_P, wr.BLS12_381_P) if p >> W == 0 and W >= 256]
    for m in moduli:
        av, bv = operands(T, W, m, rnd)
        cols = wide_cols(av, b, L) + wide_cols(bv, b, L)
        want, stats = run(eng, cols, [dict(kind="mulmod", bits=b, limbs=L, a=0, b=L, c=0, m=m, count=2 * L)])
        if m == 1:
            assert want[:L] == [[0] * T] * L and stats["qover"] == [sum(1 for x, y in zip(av, bv) if (x * y + x) >> W)]
            assert stats["qover"][0] > 0


# ---------------------------------------------------------------------------------------------------- the long division
@pytest.mark.parametrize("b,L", [(32, 4), (64, 2), (32, 8), (64, 4), (64, 8)])
def test_long_division_edges(engines, b, L):
    """the vectors that the word-level model sends through every path of the division (tests/test_wide_cpu.py asserts the
    paths): no shift, a shift of 31, a one-word divisor under a full dividend, the corrected and the capped estimate, add-back"""
    lg = 5
    eng, T, W = engines(lg), 1 << lg, b * L
    N = wr.words_for(W)
    vec = wr.division_vectors(N, W)
    rnd = random.Random(3000 + W)
    # divmod divides a W-bit a; mulmod divides the 2 W-bit a b + c: u = a b + c with b = 2^W - 1 where that can be had
    av = [u >> W for u, v, _ in vec] + [u & ((1 << W) - 1) for u, v, _ in vec]
    dv = [v for u, v, _ in vec] * 2
    while len(av) < T:
        av.append(rnd.getrandbits(W))
        dv.append(rnd.getrandbits(rnd.randrange(1, W + 1)) or 1)
    dv[T - 1] = dv[T - 2] = 0                                        # b = 0 rows inside the column
    cols = wide_cols(av, b, L) + wide_cols(dv, b, L)
    run(eng, cols, [dict(kind="divmod", bits=b, limbs=L, a=0, b=L, count=2 * L)])
    top = (1 << W) - 1
    for u, v, path in vec:                                           # the 2 W-bit dividends: u = (2^W - 1) b + c, m = v
        _, bq, c = wr.mulmod_operands(u, W)
        cols = wide_cols([top] * T, b, L) + wide_cols([c] * (T - 1) + [0], b, L)
        run(eng, cols, [dict(kind="mulmod", bits=b, limbs=L, a=0, b=("imm", bq), c=L, m=v, count=2 * L)])


# ---------------------------------------------------------------------------------------------------- counts, layout, mix
def test_out_of_range_limbs_quotients_over_and_a_row_as_two_operands(engines):
    lg = 10
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(4000)
    b, L, W = 32, 4, 128
    av, bv = [rnd.getrandbits(W) for _ in range(T)], [rnd.getrandbits(W) for _ in range(T)]
    cols = wide_cols(av, b, L) + wide_cols(bv, b, L)
    for row, t, x in ((0, 300, 1 << 32), (3, 300, R - 1), (5, 300, 1 << 64), (2, 70, (1 << 200) + 5), (6, 1000, 1 << 33)):
        cols[row][t] = x                                             # row 300 three times over: counted once
    ops = [dict(kind="add", bits=b, limbs=L, a=0, b=L), dict(kind="mul", bits=b, limbs=L, a=0, b=0),
           dict(kind="mulmod", bits=b, limbs=L, a=L, b=L, m=5, count=L), dict(kind="sub", bits=b, limbs=L, a=L, b=("imm", 7))]
    want, stats = run(eng, cols, ops, sizes=(3, 5))
    assert stats["counts"] == [3, 2, 2, 2] and stats["first"] == [70, 70, 300, 300]
    assert stats["qover"][2] > T // 2 and stats["first_qover"][2] is not None      # m = 5: q does not fit 128 bits
    assert want[L:2 * L] == wide_cols([(x % (1 << W)) ** 2 % (1 << W) for x in
                                               [sum((cols[l][t] % (1 << b)) << (b * l) for l in range(L)) for t in range(T)]], b, L)
    assert eng.rows_stats() == before


@pytest.mark.parametrize("lg,u", [(5, 27), (10, (1 << 10) - 31)])
def test_usable_layout_with_garbage_behind(engines, lg, u):
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(5000 + lg)
    b, L = 64, 4
    av, bv = [rnd.getrandbits(256) for _ in range(T)], [rnd.getrandbits(256) or 1 for _ in range(T)]
    cols = wide_cols(av, b, L) + wide_cols(bv, b, L)
    for c in cols:
        c[u:] = [R - 1 - t for t in range(T - u)]                    # out of range, were it read
    ops = [dict(kind="divmod", bits=b, limbs=L, a=0, b=L, count=2 * L),
           dict(kind="mulmod", bits=b, limbs=L, a=0, b=L, m=wr.SECP256K1_P, count=2 * L)]
    tail = [rnd.randrange(R) for _ in range(16 * (T - u))]
    want, stats = run(eng, cols, ops, u, tail)
    assert stats["counts"] == [0, 0] and stats["first"] == [None, None]
    assert all(want[c][u:] == tail[c * (T - u):(c + 1) * (T - u)] for c in range(16))
    _, stats = run(eng, cols, ops)
    assert stats["counts"] == [T - u] * 2 and stats["first"] == [u] * 2
    assert eng.rows_stats() == before


def test_eight_ops_fill_sixteen_rows(engines):
    lg = 8
    eng, T = engines(lg), 1 << lg
    rnd = random.Random(6000)
    cols = [[rnd.getrandbits(16) for _ in range(T)] for _ in range(16)]
    m = 0xfff1
    ops = [dict(kind="add", bits=16, limbs=1, a=0, b=1, count=2), dict(kind="sub", bits=16, limbs=1, a=2, b=3, count=2),
           dict(kind="mul", bits=8, limbs=2, a=4, b=6, count=4), dict(kind="divmod", bits=16, limbs=1, a=8, b=9, count=2),
           dict(kind="mulmod", bits=16, limbs=1, a=10, b=11, c=12, m=m, count=2), dict(kind="mulmod", bits=16, limbs=1, a=13, m=m),
           dict(kind="add", bits=16, limbs=2, a=14, b=("imm", 0xffffffff), count=2), dict(kind="sub", bits=16, limbs=1, a=0, b=0)]
    want, stats = run(eng, cols, ops, sizes=(7, 9))
    assert len(want) == 16 and want[15] == [0] * T


# ---------------------------------------------------------------------------------------------------- end to end
def test_mulmod_then_carry_then_the_limb_gate_holds_on_the_committed_columns(engines):
    """b = 32, L = 3 with b an immediate -- a, r, q and the five carries are 14 of the 16 rows that one commit_expr call reads
    (the gate at L = 8 would need 47): mulmod, then carry, then checks of s_k - carry_k 2^b = 0 over the committed columns
    report nonzero = 0; after one r cell is changed they report nonzero > 0"""
    lg = 6
    eng, T = engines(lg), 1 << lg
    before = eng.rows_stats()
    rnd = random.Random(7000)
    b, L, W = 32, 3, 96
    m = rnd.getrandbits(W) | (1 << (W - 1)) | 1
    kb = rnd.randrange(1 << (W - 1), m)
    av = [rnd.randrange(m) for _ in range(T)]
    I = commit_sets(eng, wide_cols(av, b, L), (L,))
    ml, bl = wr.limbs_of(m, b, L), wr.limbs_of(kb, b, L)
    gates = []                                                        # rows: a 0.., r L.., q 2 L.., carries 3 L..
    for k in range(2 * L):
        terms = [(be(bl[k - i]), [i]) for i in range(L) if 0 <= k - i < L and bl[k - i]]
        terms += [(be(R - ml[k - i]), [2 * L + i]) for i in range(L) if 0 <= k - i < L and ml[k - i]]
        if k < L:
            terms.append((be(R - 1), [L + k]))
        if k >= 1:
            terms.append((be(1), [3 * L + k - 1]))
        if k < 2 * L - 1:
            terms.append((be(R - (1 << b)), [3 * L + k]))
        gates.append((terms, True))
    carry = dict(kind="carry", bits=b, limbs=L, a=0, b=("imm", kb), r=L, q=2 * L, m=m)
    QR, st = eng.commit_wide(I, [dict(kind="mulmod", bits=b, limbs=L, a=0, b=("imm", kb), m=m, count=2 * L)])   # r then q
    assert st["counts"] == [0] and st["qover"] == [0]
    CY, st = eng.commit_wide(I + [QR], [carry])
    assert st == {"counts": [0], "first": [None], "qover": [0], "first_qover": [None]}
    none, nonzero, first = eng.commit_expr(I + [QR, CY], gates)
    assert none is None and nonzero == [0] * (2 * L) and first == [None] * (2 * L)
    rows = read_all(eng, QR)
    rows[1][5] = (rows[1][5] + 1) % (1 << b)                          # one r cell changed
    BAD = commit_sets(eng, rows, (2 * L,))
    CY2, st = eng.commit_wide(I + BAD, [carry])
    assert st["qover"] == [1] and st["first_qover"] == [5]
    none, nonzero, first = eng.commit_expr(I + BAD + [CY2], gates)
    assert sum(nonzero) > 0 and 5 in first
    release([CY, CY2, QR] + I + BAD)
    assert eng.rows_stats() == before


# ---------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_context_serving(hip):
    eng = hip()
    lg = 5
    T = 1 << lg
    eng.gen_srs(SEED_X, SEED_Y, lg, 0)
    rnd = random.Random(8000)
    cols = [[rnd.getrandbits(32) for _ in range(T)] for _ in range(8)]
    ops = [dict(kind="mulmod", bits=32, limbs=4, a=0, b=4, m=(1 << 127) - 1, count=8)]
    want, stats = wr.wide_columns(cols, ops)
    I = commit_sets(eng, cols, (8,))

    def fresh_ok():
        out, got = eng.commit_wide(I, ops)
        try:
            assert got == stats and read_all(eng, out) == want
        finally:
            out.release()

    fresh_ok()
    live = eng.rows_stats()
    lib = _native.load()
    hi = (ctypes.c_uint64 * 1)(I[0].handle)
    c, h = ctypes.create_string_buffer(48 * 16), ctypes.c_uint64(0)
    st = [(ctypes.c_uint64 * 16)() for _ in range(4)]
    NO = _native.KZG_WIDE_ABSENT
    ADD, SUB, MUL, DIVMOD, MULMOD, CARRY = range(1, 7)
    z = bytes(64)
    one = (1).to_bytes(64, "big")

    def raw(recs, opts=None, n_ops=None):
        arr = (_native.WideOp * max(len(recs), 1))(*[eng.wide_op_struct(r) for r in recs])
        return lib.kzg_rows_commit_wide(eng._h, 1, hi, len(recs) if n_ops is None else n_ops, arr,
                                        ctypes.byref(opts) if opts else None, c, st[0], st[1], st[2], st[3], ctypes.byref(h))

    def refused(rc, why):
        msg = lib.kzg_last_error(eng._h)
        assert rc == _native.KZG_E_ARG and msg.startswith(b"wide: ") and why in msg, (rc, msg)
        assert eng.rows_stats() == live

    # (kind, bits, limbs, count, flags, a, b, c, q, r, imm, m)
    ok = (ADD, 32, 4, 4, 0, 0, 4, NO, NO, NO, z, z)
    edit = lambda base, **kw: tuple(kw.get(f, v) for f, v in zip(  # noqa: E731
        ("kind", "bits", "limbs", "count", "flags", "a", "b", "c", "q", "r", "imm", "m"), base))
    refused(raw([], n_ops=0), b"n_ops")
    refused(raw([ok] * 9), b"n_ops")
    refused(raw([edit(ok, count=5)] * 4), b"n_out")
    refused(raw([edit(ok, kind=0)]), b"unknown kind")
    refused(raw([edit(ok, kind=7)]), b"unknown kind")
    refused(raw([edit(ok, flags=4)]), b"flags")
    refused(raw([edit(ok, bits=0)]), b"limb width b")
    refused(raw([edit(ok, bits=65)]), b"limb width b")
    refused(raw([edit(ok, limbs=0, count=1)]), b"number of limbs")
    refused(raw([edit(ok, limbs=9, count=9)]), b"number of limbs")
    refused(raw([edit(ok, bits=64, limbs=8, count=8, kind=CARRY)]), b"CARRY must be at most 56")
    refused(raw([edit(ok, bits=57, kind=CARRY, count=7, q=0, r=0, m=one)]), b"at most 56")
    refused(raw([edit(ok, count=6)]), b"count must be")
    refused(raw([edit(ok, kind=MUL, count=5)]), b"count must be")
    refused(raw([edit(ok, kind=CARRY, count=8, q=0, r=0, m=one)]), b"count must be")
    refused(raw([edit(ok, a=NO)]), b"operand a")
    refused(raw([edit(ok, a=5)]), b"inside the concatenated rows")
    refused(raw([edit(ok, b=8)]), b"inside the concatenated rows")
    refused(raw([edit(ok, kind=MULMOD, c=6, m=one)]), b"inside the concatenated rows")
    refused(raw([edit(ok, b=NO)]), b"operand b must be given")
    refused(raw([edit(ok, flags=1)]), b"KZG_WIDE_ABSENT beside")
    refused(raw([edit(ok, flags=1, b=NO, imm=(1 << 128).to_bytes(64, "big"))]), b"immediate must be below")
    refused(raw([edit(ok, imm=one)]), b"immediate must be 0")
    refused(raw([edit(ok, c=0)]), b"does not take")
    refused(raw([edit(ok, m=one)]), b"does not take")
    refused(raw([edit(ok, flags=2)]), b"does not take")
    refused(raw([edit(ok, q=0)]), b"does not take")
    refused(raw([edit(ok, kind=MULMOD, r=0, m=one)]), b"does not take")
    refused(raw([edit(ok, kind=MULMOD)]), b"must not be 0")
    refused(raw([edit(ok, kind=MULMOD, m=(1 << 128).to_bytes(64, "big"))]), b"m must be below")
    refused(raw([edit(ok, kind=CARRY, count=7, m=one)]), b"q and r must be given")
    tl = b"".join(bt([rnd.randrange(R) for _ in range(4 * 4)]))
    for usable, tail, why in ((T, tl, b"usable must be in"), (T - 4, None, b"tail_be32 must be given"), (0, tl, b"plain layout"),
                              (T - 4, tl[:-32] + R.to_bytes(32, "big"), b"canonical")):
        refused(raw([ok], _native.DeriveOpts(usable, tail)), why)
    fresh_ok()
    assert raw([edit(ok, flags=1, b=NO, imm=((1 << 128) - 1).to_bytes(64, "big"), count=5)]) == 0      # the largest that fits
    eng.release_rows(h.value)
    for bad, why in ((dict(ops[0], kind="nand"), "unknown kind"), (dict(ops[0], bits=65), "limb width"),
                     (dict(ops[0], m=0), "must not be 0"), (dict(ops[0], m=1 << 128), "below 2^W"),
                     (dict(ops[0], q=0), "does not take"), (dict(ops[0], a=5), "inside the concatenated"),
                     (dict(ops[0], b=("imm", 1 << 128)), "immediate must be below"), (dict(ops[0], foo=1), "unknown field")):
        arg_error(lambda: eng.commit_wide(I, [bad]), why)
    arg_error(lambda: eng.commit_wide(I, ops, None, [be(1)]), "tail")
    arg_error(lambda: eng.commit_wide([2 ** 40], ops), "unknown")
    fresh_ok()
    release(I)
    assert eng.rows_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------------- routing
def test_client_and_multi_device_client_return_the_engine_bytes(hip):
    from zkp_subnet_amd import Client, MultiDeviceClient, codec

    scale, ms = 6, 0
    T = 1 << scale
    rnd = random.Random(9000)
    b, L = 64, 4
    p = wr.SECP256K1_P
    av, bv = [rnd.randrange(p) for _ in range(T)], [rnd.randrange(p) for _ in range(T)]
    cols = wide_cols(av, b, L) + wide_cols(bv, b, L)
    ops = [{"kind": "mulmod", "bits": b, "limbs": L, "a": 0, "b": L, "m": hex(p), "count": 2 * L},
           {"kind": "add", "bits": b, "limbs": L, "a": 0, "b": ["imm", str(p)], "count": L + 1}]
    want, stats = wr.wide_columns(cols, ops)
    fr = lambda col: [codec.be32_to_fr(be(v)) for v in col]   # noqa: E731
    for client in (Client(seed=81), MultiDeviceClient(devices=[0], seed=81)):
        client.start(scale=scale, machines_scale=ms)
        try:
            a = client.worker_commit_rows(0, [fr(col) for col in cols]).json()["handle"]
            ref = client.worker_commit_rows(0, [fr(col) for col in want]).json()
            r = client.worker_commit_wide([a], ops)
            assert r.status_code == 200, r.json()
            body = r.json()
            assert body["commitments"] == ref["commitments"]
            assert {k: body[k] for k in stats} == stats
            cells = client.worker_read_rows([body["handle"]], 3, 0, T, "u64").json()
            assert cells["cells"] == want[3] and cells["overflow"] == 0
            assert client.worker_commit_wide([a], [dict(ops[0], kind="nand")]).status_code == 400
            assert client.worker_commit_wide([a], [dict(ops[0], m=0)]).status_code == 400
            assert client.worker_commit_wide([a], ops, None, fr([1])).status_code == 400
            for hh in (ref["handle"], body["handle"], a):
                assert client.worker_release_rows(hh).status_code == 200
            assert client.worker_commit_wide([a], ops).status_code == 400
        finally:
            client.stop()
