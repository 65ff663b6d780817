"""The definition of kzg_rows_commit_int in Python integers: machine-word arithmetic on the canonical integers of one or two
columns, each reduced to its low w bits, the out-of-range count and first row of every op, and the caller's tail behind
`usable`.  Columns are lists of canonical integers (evaluations at w_T^t)."""
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
KINDS = ("and", "or", "xor", "add", "sub", "mul", "divmod", "split")
TWO_ROWS = ("add", "sub", "mul", "divmod", "split")     # the kinds that have a second output row


def cell(kind, w, x, y):
    """(row 0, row 1, out of range?) of one cell: x and y are the operands' canonical integers as they lie in the columns (y of
    an immediate is the immediate); an operand at or above 2^w is out of range and is reduced to its low w bits, a split's
    shift above w is out of range and is taken as w"""
    assert kind in KINDS and 1 <= w <= 64
    M = 1 << w
    a = x % M
    if kind == "split":
        s = min(y, w)
        return a >> s, a % (1 << s), x >= M or y > w
    b = y % M
    over = x >= M or y >= M
    if kind == "and":
        return a & b, None, over
    if kind == "or":
        return a | b, None, over
    if kind == "xor":
        return a ^ b, None, over
    if kind == "add":
        return (a + b) % M, (a + b) >> w, over
    if kind == "sub":
        return (a - b) % M, int(a < b), over
    if kind == "mul":
        return (a * b) % M, (a * b) >> w, over
    return (a // b, a % b, over) if b else (M - 1, a, over)     # divmod: the RISC-V convention, a zero divisor is not counted


def parse(op):
    """(kind, w, a, b row or None, immediate or None, count) of an op as HipEngine.commit_int takes it"""
    kind, w, a, b = op[:4]
    count = op[4] if len(op) == 5 else 1
    assert count == 1 or (count == 2 and kind in TWO_ROWS)
    if isinstance(b, (tuple, list)):
        assert b[0] == "imm" and (0 <= b[1] <= w if kind == "split" else 0 <= b[1] < 1 << w)
        return kind, w, a, None, b[1], count
    return kind, w, a, b, None, count


def n_out(ops):
    return sum(parse(op)[5] for op in ops)


def int_columns(cols, ops, usable=None, tail=()):
    """(the output columns in the order of ops, the out-of-range count per op, the smallest out-of-range row per op or None).
    usable = None: all T rows are read; otherwise rows [0, usable) are, the source rows behind are neither read nor counted,
    and output row usable + s of output column c is tail[c * (T - usable) + s]"""
    T = len(cols[0])
    n = T if usable is None else usable
    assert 1 <= n <= T and len(tail) == n_out(ops) * (T - n)
    out, counts, firsts = [], [], []
    for op in ops:
        kind, w, a, b, imm, count = parse(op)
        cells = [cell(kind, w, cols[a][t], imm if b is None else cols[b][t]) for t in range(n)]
        out.append([c[0] for c in cells])
        if count == 2:
            out.append([c[1] for c in cells])
        flagged = [t for t, c in enumerate(cells) if c[2]]
        counts.append(len(flagged))
        firsts.append(flagged[0] if flagged else None)
    return [col + list(tail[c * (T - n):(c + 1) * (T - n)]) for c, col in enumerate(out)], counts, firsts
