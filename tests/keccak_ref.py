"""The definition of kzg_rows_commit_keccak in Python integers: Keccak-f[1600] of FIPS 202 per row, and the round trace in
blocks of P >= 125 rows with its 25 columns.  All values are 64-bit lanes, lane (x, y) at the flat index x + 5 y; a source cell is
its integer reduced to its low 64 bits and a cell at or above 2^64 is counted.  The round constants and the rotation offsets are
GENERATED here by the rules of FIPS 202 (the LFSR of rc, the walk of rho), not copied from the kernel's tables.
tests/test_keccak_cpu.py pins this file against hashlib and against the trace identities; the GPU tests compare the device with
it byte for byte."""
M64 = (1 << 64) - 1
NAMES = tuple(f"{k}{x}" for k in "apdtb" for x in range(5))
MIN_PERIOD = 125


def _rc_bit(t):
    """rc(t) of FIPS 202, algorithm 5"""
    if t % 255 == 0:
        return 1
    R = [1, 0, 0, 0, 0, 0, 0, 0]
    for _ in range(t % 255):
        R = [0] + R
        R[0] ^= R[8]
        R[4] ^= R[8]
        R[5] ^= R[8]
        R[6] ^= R[8]
        R = R[:8]
    return R[0]


RC = [sum(_rc_bit(j + 7 * i) << ((1 << j) - 1) for j in range(7)) for i in range(24)]


def _offsets():
    r = [[0] * 5 for _ in range(5)]   # r[x][y]
    x, y = 1, 0
    for t in range(24):
        r[x][y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return r


ROT = _offsets()


def rotl(v, k):
    k %= 64
    return ((v << k) | (v >> (64 - k))) & M64 if k else v


def round_trace(A, q):
    """the 25 columns of round q on the state A (flat, x + 5 y): {name: 5 cells, one per plane y}, and the state after it"""
    col = {name: [0] * 5 for name in NAMES}
    C = [0] * 5
    for x in range(5):
        for y in range(5):
            col[f"a{x}"][y] = A[x + 5 * y]
            C[x] ^= A[x + 5 * y]
            col[f"p{x}"][y] = C[x]
    D = [C[(x - 1) % 5] ^ rotl(C[(x + 1) % 5], 1) for x in range(5)]
    B = [0] * 25
    for x in range(5):
        for y in range(5):
            t = rotl(A[x + 5 * y] ^ D[x], ROT[x][y])
            col[f"d{x}"][y] = D[x]
            col[f"t{x}"][y] = t
            B[y + 5 * ((2 * x + 3 * y) % 5)] = t
    for x in range(5):
        for y in range(5):
            col[f"b{x}"][y] = B[x + 5 * y]
    nxt = [B[x + 5 * y] ^ ((B[(x + 1) % 5 + 5 * y] ^ M64) & B[(x + 2) % 5 + 5 * y]) for y in range(5) for x in range(5)]
    nxt[0] ^= RC[q]
    return col, nxt


_RHO_PI = [(x + 5 * y, y + 5 * ((2 * x + 3 * y) % 5), ROT[x][y]) for x in range(5) for y in range(5)]


def permute(A):
    """Keccak-f[1600] of the 25 lanes A: round_trace without the columns (test_keccak_cpu.py holds the two together)"""
    A = list(A)
    B = [0] * 25
    for q in range(24):
        C = [A[x] ^ A[x + 5] ^ A[x + 10] ^ A[x + 15] ^ A[x + 20] for x in range(5)]
        D = [C[x - 1] ^ rotl(C[(x + 1) % 5], 1) for x in range(5)]
        for src, dst, k in _RHO_PI:
            B[dst] = rotl(A[src] ^ D[src % 5], k)
        for y in range(0, 25, 5):
            b0, b1, b2, b3, b4 = B[y:y + 5]
            A[y:y + 5] = b0 ^ (~b1 & b2), b1 ^ (~b2 & b3), b2 ^ (~b3 & b4), b3 ^ (~b4 & b0), b4 ^ (~b0 & b1)
        A[0] ^= RC[q]
    return A


def block_trace(A):
    """the 125 rows of one block from its absorbed state A: {name: 125 cells}, and the outgoing state"""
    col = {name: [0] * 125 for name in NAMES}
    for q in range(24):
        rnd, A = round_trace(A, q)
        for name in NAMES:
            col[name][5 * q:5 * q + 5] = rnd[name]
    for x in range(5):
        for y in range(5):
            col[f"a{x}"][120 + y] = A[x + 5 * y]
    return col, A


class Counter:
    """the over-range cells of a unit: how many, and the smallest row of one"""
    def __init__(self):
        self.count, self.first, self.cells = 0, None, set()

    def lane(self, cols, c, t):
        v = cols[c][t]
        if v >> 64 and (c, t) not in self.cells:
            self.cells.add((c, t))
            self.count += 1
            self.first = t if self.first is None else min(self.first, t)
        return v & M64


def rounds_unit(cols, unit, n):
    """the named columns of a rounds unit over the first n rows of `cols`: (columns of len(cols[0]) cells, blocks, messages,
    the Counter)"""
    T, P, rate = len(cols[0]), unit["period"], unit["rate"]
    out = {name: [0] * T for name in NAMES}
    seen, messages, S = Counter(), 0, None
    for b in range(n // P):
        starts = b == 0 or unit.get("start") is None
        if unit.get("start") is not None:
            starts |= seen.lane(cols, unit["start"], b * P) != 0
        if starts:
            messages += 1
            S = [0] * 25
        A = [S[i] ^ (seen.lane(cols, unit["msg"][i % 5], b * P + i // 5) if i < rate else 0) for i in range(25)]
        blk, S = block_trace(A)
        for name in NAMES:
            out[name][b * P:b * P + 125] = blk[name]
    return [out[name] for name in unit["cols"]], n // P, messages, seen


def row_unit(cols, unit, n):
    """(the columns of `out`, the Counter): one permutation per row t' < n, zero behind"""
    T = len(cols[0])
    seen = Counter()
    slot = lambda s, t: s[1] if isinstance(s, (list, tuple)) else seen.lane(cols, s, t)   # noqa: E731
    out = [[0] * T for _ in unit["out"]]
    for t in range(n):
        new = permute([slot(s, t) for s in unit["in"]])
        for c, j in enumerate(unit["out"]):
            out[c][t] = new[j]
    return out, seen


def columns(cols, units, usable=None, tail=()):
    """what commit_keccak returns for these units over the evaluation columns `cols`: (the committed rows in unit order with
    the caller's tail behind `usable`, the statistics)"""
    T = len(cols[0])
    n = T if usable is None else usable
    rows = []
    st = {k: [] for k in ("perms", "messages", "counts", "first", "mismatch", "first_mismatch")}
    for unit in units:
        mismatch = []
        if unit["mode"] == "rounds":
            got, perms, messages, seen = rounds_unit(cols, unit, n)
            rows += got
        else:
            got, seen = row_unit(cols, unit, n)
            perms, messages = n, 0
            if unit.get("expect") is not None:
                mismatch = [t for t in range(n) if any(cols[x][t] != got[c][t] for c, x in enumerate(unit["expect"]))]
            else:
                rows += got
        for k, v in (("perms", perms), ("messages", messages), ("counts", seen.count), ("first", seen.first),
                     ("mismatch", len(mismatch)), ("first_mismatch", mismatch[0] if mismatch else None)):
            st[k].append(v)
    for c, row in enumerate(rows):
        if usable is not None:
            row[n:] = tail[c * (T - n):(c + 1) * (T - n)]
    return rows, st


def pad(message, rate, suffix):
    """the padded message as a list of blocks of `rate` lanes: the domain suffix byte (0x01 Keccak, 0x06 SHA-3, 0x1f SHAKE)
    behind the message, zeros, and 0x80 into the last byte of the last block (pad10*1); a lane is the little-endian word of 8
    bytes"""
    nbytes = 8 * rate
    m = bytearray(message) + bytes([suffix])
    m += bytes(-len(m) % nbytes)
    m[-1] |= 0x80
    return [[int.from_bytes(m[o + 8 * j:o + 8 * j + 8], "little") for j in range(rate)] for o in range(0, len(m), nbytes)]


def sponge(message, rate, suffix, nbytes):
    """the first nbytes <= 8 rate bytes squeezed from the sponge over permute"""
    S = [0] * 25
    for blk in pad(message, rate, suffix):
        S = permute([s ^ (blk[i] if i < rate else 0) for i, s in enumerate(S)])
    return digest_bytes(S, nbytes)


def digest_bytes(lanes, nbytes):
    return b"".join(v.to_bytes(8, "little") for v in lanes)[:nbytes]
