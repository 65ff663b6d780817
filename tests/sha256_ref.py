"""The definition of kzg_rows_commit_sha256 in Python integers: the SHA-256 compression function of FIPS 180-4 per row, and the
round trace in blocks of P >= 72 rows with its helper columns and carries.  All values are 32-bit words; a source cell is its
integer reduced to its low 32 bits and a cell at or above 2^32 is counted.  tests/test_sha256_cpu.py pins this file against
hashlib and against the gate identities; the GPU tests compare the device with it byte for byte."""
K = [
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]
IV224 = [0xc1059ed8, 0x367cd507, 0x3070dd17, 0xf70e5939, 0xffc00b31, 0x68581511, 0x64f98fa7, 0xbefa4fa4]
M32 = 0xffffffff
NAMES = ("w", "a", "e", "cw", "ca", "ce", "sig0", "sig1", "sum0", "maj", "sum1", "ch")
MIN_PERIOD = 72


def rotr(x, k):
    return ((x >> k) | (x << (32 - k))) & M32


def sig0(x):
    return rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3)


def sig1(x):
    return rotr(x, 17) ^ rotr(x, 19) ^ (x >> 10)


def sum0(x):
    return rotr(x, 2) ^ rotr(x, 13) ^ rotr(x, 22)


def sum1(x):
    return rotr(x, 6) ^ rotr(x, 11) ^ rotr(x, 25)


def ch(e, f, g):
    return (e & f) ^ (~e & M32 & g)


def maj(a, b, c):
    return (a & b) ^ (a & c) ^ (b & c)


def block_trace(H, words):
    """the 72 rows of one block from the incoming chaining value H and the 16 message words: {name: 72 cells}, and the
    outgoing chaining value"""
    col = {name: [0] * 72 for name in NAMES}
    W, A, E = col["w"], col["a"], col["e"]
    for j in range(4):
        A[j], E[j] = H[3 - j], H[7 - j]
    for t in range(64):
        q = 4 + t
        if t < 16:
            W[q] = words[t]
        else:
            col["sig0"][q], col["sig1"][q] = sig0(W[q - 15]), sig1(W[q - 2])
            s = col["sig1"][q] + W[q - 7] + col["sig0"][q] + W[q - 16]
            W[q], col["cw"][q] = s & M32, s >> 32
        a, b, c, d = A[q - 1], A[q - 2], A[q - 3], A[q - 4]
        e, f, g, h = E[q - 1], E[q - 2], E[q - 3], E[q - 4]
        col["sum0"][q], col["maj"][q], col["sum1"][q], col["ch"][q] = sum0(a), maj(a, b, c), sum1(e), ch(e, f, g)
        t1 = h + col["sum1"][q] + col["ch"][q] + K[t] + W[q]
        sa, se = t1 + col["sum0"][q] + col["maj"][q], d + t1
        A[q], col["ca"][q] = sa & M32, sa >> 32
        E[q], col["ce"][q] = se & M32, se >> 32
    for j in range(4):
        fa, fe = A[j] + A[64 + j], E[j] + E[64 + j]
        A[68 + j], col["ca"][68 + j] = fa & M32, fa >> 32
        E[68 + j], col["ce"][68 + j] = fe & M32, fe >> 32
    return col, [A[71], A[70], A[69], A[68], E[71], E[70], E[69], E[68]]


def compress(H, words):
    """the new chaining value, feed-forward included"""
    return block_trace(H, words)[1]


class Counter:
    """the over-range cells of a unit: how many, and the smallest row of one"""
    def __init__(self):
        self.count, self.first, self.cells = 0, None, set()

    def word(self, cols, c, t):
        v = cols[c][t]
        if v >> 32 and (c, t) not in self.cells:
            self.cells.add((c, t))
            self.count += 1
            self.first = t if self.first is None else min(self.first, t)
        return v & M32


def rounds_unit(cols, unit, n):
    """the named columns of a rounds unit over the first n rows of `cols`: (columns of len(cols[0]) cells, blocks, messages,
    the Counter)"""
    T, P = len(cols[0]), unit["period"]
    out = {name: [0] * T for name in NAMES}
    seen, messages, H = Counter(), 0, None
    for b in range(n // P):
        starts = b == 0 or unit.get("start") is None
        if unit.get("start") is not None:
            starts |= seen.word(cols, unit["start"], b * P) != 0
        if starts:
            messages += 1
            H = list(unit.get("iv") or IV)
        blk, H = block_trace(H, [seen.word(cols, unit["msg"], b * P + 4 + t) for t in range(16)])
        for name in NAMES:
            out[name][b * P:b * P + 72] = blk[name]
    return [out[name] for name in unit["cols"]], n // P, messages, seen


def row_unit(cols, unit, n):
    """(the columns of `out`, the Counter): one compression per row t' < n, zero behind"""
    T = len(cols[0])
    seen = Counter()
    slot = lambda s, t: s[1] if isinstance(s, (list, tuple)) else seen.word(cols, s, t)   # noqa: E731
    out = [[0] * T for _ in unit["out"]]
    for t in range(n):
        H = list(IV) if unit["state"] == "iv" else [slot(s, t) for s in unit["state"]]
        new = compress(H, [slot(s, t) for s in unit["msg"]])
        for c, j in enumerate(unit["out"]):
            out[c][t] = new[j]
    return out, seen


def columns(cols, units, usable=None, tail=()):
    """what commit_sha256 returns for these units over the evaluation columns `cols`: (the committed rows in unit order with
    the caller's tail behind `usable`, the statistics)"""
    T = len(cols[0])
    n = T if usable is None else usable
    rows = []
    st = {k: [] for k in ("blocks", "messages", "counts", "first", "mismatch", "first_mismatch")}
    for unit in units:
        mismatch = []
        if unit["mode"] == "rounds":
            got, blocks, messages, seen = rounds_unit(cols, unit, n)
            rows += got
        else:
            got, seen = row_unit(cols, unit, n)
            blocks, messages = n, 0
            if unit.get("expect") is not None:
                mismatch = [t for t in range(n) if any(cols[x][t] != got[c][t] for c, x in enumerate(unit["expect"]))]
            else:
                rows += got
        for k, v in (("blocks", blocks), ("messages", messages), ("counts", seen.count), ("first", seen.first),
                     ("mismatch", len(mismatch)), ("first_mismatch", mismatch[0] if mismatch else None)):
            st[k].append(v)
    for c, row in enumerate(rows):
        if usable is not None:
            row[n:] = tail[c * (T - n):(c + 1) * (T - n)]
    return rows, st


def pad(message):
    """the padded message of FIPS 180-4 as a list of 16-word blocks"""
    m = message + b"\x80" + bytes((55 - len(message)) % 64) + (8 * len(message)).to_bytes(8, "big")
    return [[int.from_bytes(m[o + 4 * j:o + 4 * j + 4], "big") for j in range(16)] for o in range(0, len(m), 64)]


def digest_bytes(H):
    return b"".join(w.to_bytes(4, "big") for w in H)
