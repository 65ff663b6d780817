"""The definition of kzg_rows_commit_alu in Python integers: machine-word arithmetic on the canonical integers of two columns,
the kind chosen per row by an op-code column through a program.  Columns are lists of canonical integers (evaluations at
w_T^t).  The eight kinds shared with kzg_rows_commit_int are written out again here, not imported: tests/test_alu_cpu.py checks
the two definitions against each other."""
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
KINDS = ("and", "or", "xor", "add", "sub", "mul", "divmod", "split", "ltu", "lt", "eq", "sll", "srl", "sra", "rotl", "rotr",
         "mulhu", "mulh", "mulhsu", "div", "rem", "remu", "sext")           # header order: KZG_ALU_<NAME> = index + 1
SHARED = KINDS[:8]                                                          # the kinds of kzg_rows_commit_int
SHIFTS = ("sll", "srl", "sra", "rotl", "rotr")                              # s = b mod w
ONE_ROW = ("and", "or", "xor")                                              # row 1 is 0


def sgn(x, w):
    return x - (1 << w) if x >> (w - 1) else x


def cell(kind, w, x, y):
    """(row 0, row 1, out of range?) of one cell: x and y are the operands' canonical integers as they lie in the columns (y of
    an entry with an immediate is the immediate)"""
    assert kind in KINDS and 1 <= w <= 64
    M = 1 << w
    a = x % M
    if kind == "split":
        s = min(y, w)
        return a >> s, a % (1 << s), x >= M or y > w
    if kind == "sext":
        bad = y == 0 or y > w
        f = w if bad else y
        lo = a % (1 << f)
        bit = lo >> (f - 1)
        return (lo - (bit << f)) % M, bit, x >= M or bad
    b = y % M
    over = x >= M or y >= M
    A, B = sgn(a, w), sgn(b, w)
    if kind in SHIFTS:
        s = b % w
        lo, top = a % (1 << s), (a >> (w - s) if s else 0)
        if kind == "sll":
            return (a << s) % M, top, over
        if kind == "srl":
            return a >> s, lo, over
        if kind == "sra":
            return (A >> s) % M, lo, over                                   # Python's >> floors
        if kind == "rotl":
            return (a << s) % M + top, top, over
        return ((a >> s) + (lo << (w - s)) if s else a), lo, over           # rotr
    if kind == "and":
        return a & b, 0, over
    if kind == "or":
        return a | b, 0, over
    if kind == "xor":
        return a ^ b, 0, over
    if kind == "add":
        return (a + b) % M, (a + b) >> w, over
    if kind == "sub":
        return (a - b) % M, int(a < b), over
    if kind == "mul":
        return (a * b) % M, (a * b) >> w, over
    if kind == "ltu":
        return int(a < b), (a - b) % M, over
    if kind == "lt":
        return int(A < B), (a - b) % M, over
    if kind == "eq":
        return int(a == b), (a - b) % M, over
    if kind == "mulhu":
        return (a * b) >> w, (a * b) % M, over
    if kind == "mulh":
        return ((A * B) >> w) % M, (a * b) % M, over
    if kind == "mulhsu":
        return ((A * b) >> w) % M, (a * b) % M, over
    if kind in ("divmod", "remu"):
        q, r = (a // b, a % b) if b else (M - 1, a)                         # the RISC-V convention, not counted
        return (q, r, over) if kind == "divmod" else (r, q, over)
    assert kind in ("div", "rem")
    if B == 0:
        q, r = M - 1, a
    else:
        q = abs(A) // abs(B) * (-1 if (A < 0) != (B < 0) else 1)            # truncation toward zero
        q, r = q % M, (A - q * B) % M                                       # (the overflow -M/2 / -1 wraps to M/2, remainder 0)
    return (q, r, over) if kind == "div" else (r, q, over)


def parse(entry):
    """(kind, w, immediate or None) of a program entry as HipEngine.commit_alu takes it; None for an idle entry"""
    if entry is None:
        return None
    kind, w = entry[:2]
    imm = None
    if len(entry) == 3:
        assert entry[2][0] == "imm"
        imm = entry[2][1]
        assert (1 - (kind == "split") <= imm <= w) if kind in ("split", "sext") else 0 <= imm < 1 << w
    return kind, w, imm


def rows(program, cols, unit, n):
    """(row 0, row 1, statistics) of one unit (op_row, a, b[, count]) over cells [0, n): both rows as lists of n integers
    whatever the unit's count, and {"counts", "first", "unknown", "first_unknown"}"""
    op, a, b = unit[:3]
    r0, r1, over, unk = [], [], [], []
    for t in range(n):
        c = cols[op][t]
        ent = parse(program[c]) if c < len(program) else None
        if c >= len(program):
            unk.append(t)
        if ent is None:
            r0.append(0)
            r1.append(0)
            continue
        kind, w, imm = ent
        x0, x1, o = cell(kind, w, cols[a][t], cols[b][t] if imm is None else imm)
        r0.append(x0)
        r1.append(x1)
        if o:
            over.append(t)
    return r0, r1, {"counts": len(over), "first": over[0] if over else None, "unknown": len(unk),
                    "first_unknown": unk[0] if unk else None}


def alu_columns(cols, program, units, usable=None, tail=()):
    """(the output columns unit by unit, {"counts": [...], "first": [...], "unknown": [...], "first_unknown": [...]}).  usable =
    None: all T rows are read; otherwise rows [0, usable) are and output row usable + s of output column c is
    tail[c * (T - usable) + s]"""
    T = len(cols[0])
    n = T if usable is None else usable
    out = []
    stats = {"counts": [], "first": [], "unknown": [], "first_unknown": []}
    for unit in units:
        r0, r1, st = rows(program, cols, unit, n)
        out.append(r0)
        if len(unit) == 4 and unit[3] == 2:
            out.append(r1)
        for k in stats:
            stats[k].append(st[k])
    assert 1 <= n <= T and len(tail) == len(out) * (T - n)
    return [col + list(tail[c * (T - n):(c + 1) * (T - n)]) for c, col in enumerate(out)], stats
