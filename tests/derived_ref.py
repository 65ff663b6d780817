"""The definition of kzg_rows_commit_derived in Python integers: inverse-or-zero with its bit row, the limb decomposition, the
count of every op, and the caller's tail behind `usable`.  Columns are lists of canonical integers (evaluations at w_T^t)."""
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def batch_inverse(vals):
    """1 / v mod r for every v of vals (none of them zero), with ONE modular inversion: Montgomery's trick"""
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % R
    inv = pow(acc, -1, R) if vals else 1
    out = [0] * len(vals)
    for j in range(len(vals) - 1, -1, -1):
        out[j] = inv * pre[j] % R
        inv = inv * vals[j] % R
    return out


def inv0(col):
    """(1 / x or 0 where x = 0, the bit row: 1 where x = 0 else 0, the number of zero cells)"""
    nz = [t for t, x in enumerate(col) if x % R]
    inv = [0] * len(col)
    for t, y in zip(nz, batch_inverse([col[t] % R for t in nz])):
        inv[t] = y
    return inv, [0 if x % R else 1 for x in col], len(col) - len(nz)


def limbs(col, bits, count):
    """(the `count` limb columns of `bits` bits, least significant first; the number of cells at or above 2^(bits * count))"""
    assert 1 <= bits <= 32 and count >= 1 and bits * count <= 256
    m = (1 << bits) - 1
    return [[(x >> (bits * l)) & m for x in col] for l in range(count)], sum(1 for x in col if x >> (bits * count))


def n_out(ops):
    return sum((2 if len(op) == 3 and op[2] else 1) if op[0] == "inv0" else op[3] for op in ops)


def derived_columns(cols, ops, usable=None, tail=()):
    """(the output columns in the order of ops, one count per op).  ops as HipEngine.commit_derived takes them: ("inv0", row),
    ("inv0", row, True), ("limbs", row, bits, count).  usable = None: all T rows are read; otherwise rows [0, usable) are, the
    source rows behind are neither read nor counted, and output row usable + s of output column c is
    tail[c * (T - usable) + s]"""
    T = len(cols[0])
    n = T if usable is None else usable
    assert 1 <= n <= T and len(tail) == n_out(ops) * (T - n)
    out, counts = [], []
    for op in ops:
        src = cols[op[1]][:n]
        if op[0] == "inv0":
            inv, bit, zeros = inv0(src)
            out.append(inv)
            if len(op) == 3 and op[2]:
                out.append(bit)
            counts.append(zeros)
        else:
            ls, over = limbs(src, op[2], op[3])
            out += ls
            counts.append(over)
    return [col + list(tail[c * (T - n):(c + 1) * (T - n)]) for c, col in enumerate(out)], counts
