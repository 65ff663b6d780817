"""kzg_rows_commit_wide in Python integers: limbs in, rows out.  A wide value is L consecutive columns, limb l in column
first + l, each cell reduced to its low b bits.  `wide_columns` is the definition the device builder is tested against;
`knuth_divrem` is a word-level model of the long division the kernel runs (32-bit digits, a 2N-word dividend by an N-word
divisor shifted until its top bit is set), which reports the paths a vector takes."""
R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
KINDS = ("add", "sub", "mul", "divmod", "mulmod", "carry")
SECP256K1_P = (1 << 256) - (1 << 32) - 977
BN254_P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
BLS12_381_P = 0x1a0111ea397fe69a4b1ba7b6434bacd764774b84f38512bf6730d2a0f6b0f6241eabfffeb153ffffb9feffffffffaaab


def big(v):
    return int(v, 0) if isinstance(v, str) else int(v)


def counts_of(op):
    L = op["limbs"]
    return (2 * L - 1,) if op["kind"] == "carry" else (L, L + 1) if op["kind"] in ("add", "sub") else (L, 2 * L)


def count_of(op):
    return op.get("count", counts_of(op)[0])


def n_out(ops):
    return sum(count_of(op) for op in ops)


def limbs_of(x, b, L):
    return [(x >> (b * l)) & ((1 << b) - 1) for l in range(L)]


def carries(A, B, Q, Mm, D, Rr, b):
    """the 2 L carries of the limb identity over limb lists of one length L, and whether the row is exact"""
    L = len(A)
    out, carry, exact = [], 0, True
    for k in range(2 * L):
        s = sum(A[i] * B[k - i] - Q[i] * Mm[k - i] for i in range(L) if 0 <= k - i < L) + carry
        if k < L:
            s += D[k] - Rr[k]
        exact &= s % (1 << b) == 0
        carry = s >> b            # (floor, towards minus infinity)
        out.append(carry)
    return out, exact and out[-1] == 0


def wide_row(op, read):
    """one row of one op.  read(first) -> (value, over) packs the L limbs at `first`.  Returns (output cells as signed
    integers, over, qover)"""
    kind, b, L = op["kind"], op["bits"], op["limbs"]
    W = b * L
    cnt = count_of(op)
    a, over = read(op["a"])
    vb = op.get("b")
    if isinstance(vb, (list, tuple)):
        bv = big(vb[1])
    elif vb is None:
        bv = 1
    else:
        bv, o = read(vb)
        over |= o
    if kind == "add":
        s = a + bv
        return (limbs_of(s, b, L) + [s >> W])[:cnt], over, False
    if kind == "sub":
        return (limbs_of((a - bv) % (1 << W), b, L) + [int(a < bv)])[:cnt], over, False
    if kind == "mul":
        return limbs_of(a * bv, b, 2 * L)[:cnt], over, False
    if kind == "divmod":
        q, rem = (a // bv, a % bv) if bv else ((1 << W) - 1, a)
        return (limbs_of(q, b, L) + limbs_of(rem, b, L))[:cnt], over, False
    m = big(op["m"])
    c = 0
    if op.get("c") is not None:
        c, o = read(op["c"])
        over |= o
    if op.get("neg_c"):
        over |= c > m
        d = m - (c % m)
    else:
        d = c
    if kind == "mulmod":
        t = a * bv + d
        q, r = divmod(t, m)
        return (limbs_of(r, b, L) + limbs_of(q, b, L))[:cnt], over, q >> W != 0
    q, o1 = read(op["q"])
    r, o2 = read(op["r"])
    over |= o1 | o2
    cs, exact = carries(*[limbs_of(v, b, L) for v in (a, bv, q, m, d, r)], b)
    return cs[:2 * L - 1], over, not exact


def wide_columns(cols, ops, usable=None, tail=()):
    """the output rows (field elements), and per op counts, first, qover, first_qover"""
    T = len(cols[0])
    n = T if usable is None else usable
    rows, stats = [], {"counts": [], "first": [], "qover": [], "first_qover": []}
    for op in ops:
        b, L = op["bits"], op["limbs"]
        out = [[0] * T for _ in range(count_of(op))]
        ov, qo = [], []
        for t in range(n):
            def read(first):
                cells = [cols[first + l][t] for l in range(L)]
                return sum((x % (1 << b)) << (b * l) for l, x in enumerate(cells)), any(x >> b for x in cells)
            vals, over, qover = wide_row(op, read)
            for c, v in enumerate(vals):
                out[c][t] = v % R
            if over:
                ov.append(t)
            if qover:
                qo.append(t)
        rows += out
        stats["counts"].append(len(ov))
        stats["first"].append(ov[0] if ov else None)
        stats["qover"].append(len(qo))
        stats["first_qover"].append(qo[0] if qo else None)
    if usable is not None:
        for c, row in enumerate(rows):
            row[usable:] = tail[c * (T - usable):(c + 1) * (T - usable)]
    return rows, stats


# ---------------------------------------------------------------------------------------------------- the division, word by word
B32 = 1 << 32


def knuth_divrem(u, v, N):
    """u < 2^(64 N) by 0 < v < 2^(32 N) as the kernel divides: returns (q, r, paths) with paths the set of "shift0", "shift31",
    "cap" (u2 = d1: the digit estimate is capped), "fix" (the estimate corrected against the second word), "fix2" (twice) and
    "addback" that some digit step took"""
    assert 0 < v < 1 << (32 * N) and 0 <= u < 1 << (64 * N)
    paths = set()
    s = 32 * N - v.bit_length()
    paths |= {"shift0"} if s % 32 == 0 else set()
    paths |= {"shift31"} if s % 32 == 31 else set()
    V = [(v << s) >> (32 * i) & (B32 - 1) for i in range(N)]
    U = [(u << s) >> (32 * i) & (B32 - 1) for i in range(3 * N)]
    assert (u << s) >> (96 * N) == 0 and V[N - 1] >> 31
    d1, d0 = V[N - 1], V[N - 2]
    dinv = ((1 << 64) - 1) // d1 - B32
    q = 0
    for j in range(2 * N - 1, -1, -1):
        u2, u1, u0 = U[j + N], U[j + N - 1], U[j + N - 2]
        assert u2 <= d1
        if u2 >= d1:
            paths.add("cap")
            qhat, rhat = B32 - 1, u1 + d1
        else:                     # Moeller and Granlund's 2-by-1 step, all words mod 2^32
            e = dinv * u2 + (u2 << 32 | u1)
            q1, q0 = ((e >> 32) + 1) % B32, e % B32
            rr = (u1 - q1 * d1) % B32
            if rr > q0:
                q1, rr = (q1 - 1) % B32, (rr + d1) % B32
            if rr >= d1:
                q1, rr = q1 + 1, rr - d1
            assert (q1, rr) == divmod(u2 << 32 | u1, d1)
            qhat, rhat = q1, rr
        for rep in range(2):
            if rhat < B32 and qhat * d0 > (rhat << 32 | u0):
                paths.add("fix2" if rep else "fix")
                qhat, rhat = qhat - 1, rhat + d1
        win = sum(U[j + i] << (32 * i) for i in range(N + 1)) - qhat * (v << s)
        if win < 0:
            paths.add("addback")
            qhat, win = qhat - 1, win + (v << s)
        assert 0 <= win < v << s
        for i in range(N + 1):
            U[j + i] = win >> (32 * i) & (B32 - 1)
        q = q << 32 | qhat
    r = sum(U[i] << (32 * i) for i in range(N)) >> s
    return q, r, paths


def words_for(W):
    n = (W + 31) // 32
    return 4 if n <= 4 else 8 if n <= 8 else 16


def division_vectors(N, W=None):
    """(u, v, path) triples below 2^(2 W) and 2^W (W = 32 N unless given, W > 64) that drive the division of word count N
    through each path: no shift and a shift of 31, a one-word divisor under a full dividend, the corrected estimate, the
    capped estimate, and the add-back step"""
    W = 32 * N if W is None else W
    full, top = (1 << W) - 1, 1 << (W - 1)
    out = [((1 << 2 * W) - 1, full, "shift0" if W % 32 == 0 else None),
           ((1 << 2 * W) - 1, full >> 31, "shift31" if W % 32 == 0 else None),
           ((1 << 2 * W) - 1, 0xfffffffb, None), ((1 << 2 * W) - 1, 3, None)]
    # the estimate from the two top words is too large against the second divisor word: d1 = 2^31, d0 = 2^32 - 1
    v = top | ((B32 - 1) << (W - 64)) if W % 32 == 0 else None
    if v:
        out.append(((top - 1) << W, v, "fix"))
        out.append((((v >> (W - 32)) << (2 * W - 32)) | (1 << (2 * W - 64)), v, "cap"))
        # add-back: the top three words divide exactly by the top two, the words below make q V exceed the window
        v3 = top | (1 << (W - 64)) | ((1 << (W - 64)) - 1)
        qd = B32 - 3
        out.append((((qd * (v3 >> (W - 64))) << (W - 64)) << (W - 32), v3, "addback"))
    return out


def mulmod_operands(u, W):
    """(a, b, c) below 2^W with a b + c = u where that can be had with a = 2^W - 1, else the nearest such dividend"""
    top = (1 << W) - 1
    bq, c = divmod(u, top)
    if bq > top:
        bq, c = top, u - top * top
    if c > top:
        bq, c = top, top
    return top, bq, c
