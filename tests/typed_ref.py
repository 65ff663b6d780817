"""Reference of the typed columns (kzg_rows_commit_typed / kzg_rows_read) in Python integers: a column of a kind and a fill
-> the T residues mod r and their 32-byte big-endian rows, and back from residues to the integers of a kind with the overflow
rule.  Nothing here touches the library."""
import struct

from oracle.bls12_381 import R

KINDS = {"fr": (32, False), "u8": (1, False), "u16": (2, False), "u32": (4, False), "u64": (8, False), "i32": (4, True),
         "i64": (8, True)}
_CODE = {"u8": "B", "u16": "H", "u32": "I", "u64": "Q", "i32": "i", "i64": "q"}


def lo_hi(kind):
    """the integers a cell of an integer kind can hold: [lo, hi]"""
    width, signed = KINDS[kind]
    bits = 8 * width
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)


def extremes(kind):
    """the values worth pinning for a kind: 0, 1, the ends of its range and, for the signed kinds, -1"""
    lo, hi = lo_hi(kind)
    return sorted({0, 1, hi, hi - 1, lo, lo + 1} | ({-1} if lo < 0 else set()))


def pack(kind, cells):
    """the column's bytes as the library takes them: native little-endian integers, or 32 big-endian bytes per cell"""
    if kind == "fr":
        return b"".join(int(v).to_bytes(32, "big") for v in cells)
    return struct.pack(f"<{len(cells)}{_CODE[kind]}", *cells)


def unpack(kind, raw):
    if kind == "fr":
        return [int.from_bytes(raw[o:o + 32], "big") for o in range(0, len(raw), 32)]
    return list(struct.unpack(f"<{len(raw) // KINDS[kind][0]}{_CODE[kind]}", raw))


def residues(kind, cells, T=None, fill=0):
    """the T values mod r of a column: a negative cell x is r - |x|, cells [len, T) take the fill"""
    T = len(cells) if T is None else T
    assert len(cells) <= T and 0 <= fill < R
    if kind == "fr":
        assert all(0 <= v < R for v in cells)
    else:
        lo, hi = lo_hi(kind)
        assert all(lo <= v <= hi for v in cells), kind
    return [v % R for v in cells] + [fill] * (T - len(cells))


def be32_row(vals):
    return b"".join(v.to_bytes(32, "big") for v in vals)


def narrow(kind, vals):
    """residues -> (the cells as a read of `kind` returns them, overflow, first_overflow or None): a value >= r - 2^(w-1) is
    negative for the signed kinds; a value that does not fit reads 0 and is counted"""
    if kind == "fr":
        return list(vals), 0, None
    lo, hi = lo_hi(kind)
    out, bad = [], []
    for t, v in enumerate(vals):
        assert 0 <= v < R
        x = v if v <= hi else v - R
        if lo <= x <= hi:
            out.append(x)
        else:
            out.append(0)
            bad.append(t)
    return out, len(bad), (bad[0] if bad else None)
