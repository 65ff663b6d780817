"""The definition of kzg_rows_commit_poseidon_chain in Python integers.  The permutation and its trace are those of
tests/poseidon_ref.py (pinned by tests/test_poseidon_cpu.py); this file adds only what the call adds: the blocks of P rows and
their segments, the sponge's carry, the path's arrangement of the children by the position cell, the two layouts, the checks,
and the usable layout with its tail.  tests/test_poseidon_chain_cpu.py pins it by identities: an absorb loop and a tree builder
written independently of it."""
from tests.poseidon_ref import R, permute, trace

MAX_UNITS = 4


def value(cols, slot, row):
    """a slot at `row`: a row index, or ("imm", value) with the value an int or a decimal / 0x string"""
    if isinstance(slot, (list, tuple)):
        return (int(slot[1], 0) if isinstance(slot[1], str) else slot[1]) % R
    return cols[slot][row]


def arrange(cols, params, un, row, prev):
    """(the state of the block whose first row is `row`, whether its pos cell is bad); prev: the output of the block before
    where this one continues it, else None"""
    t = params["t"]
    if un["mode"] == "sponge":
        if prev is None:
            return [value(cols, s, row) for s in un["in"]], False
        return [prev[j] if isinstance(s, (list, tuple)) else (prev[j] + cols[s][row]) % R for j, s in enumerate(un["in"])], False
    a = t - 1
    p = cols[un["pos"]][row]
    bad = p >= a
    if bad:
        p = 0
    cur = value(cols, un["leaf"], row) if prev is None else prev[un["digest"]]
    children = [cols[s][row] for s in un["sib"]]
    children.insert(p, cur)
    return [value(cols, un["cap"], row)] + children, bad


def columns(cols, params, units, usable=None, tail=()):
    """(the committed rows of all units in unit order, the six statistics per unit) as the device call returns them.  cols: the
    concatenated input rows as lists of T integers; tail: column-major over the committed columns"""
    T = len(cols[0])
    n = T if usable is None else usable
    t, Rn = params["t"], params["full"] + params["partial"]
    rows = []
    st = {k: [] for k in ("blocks", "segments", "bad_pos", "first_bad_pos", "mismatch", "first_mismatch")}
    for un in units:
        P, start = un["period"], un.get("start")
        check = un.get("expect") is not None
        nb = n // P
        if check:
            out = []
        elif un["layout"] == "trace":
            assert P >= Rn + 1
            out = [[0] * T for _ in range(t)]
        else:
            out = [[0] * T for _ in un["cols"]]
        segments, bad_rows, miss_rows, prev = 0, [], [], None
        for b in range(nb):
            row = b * P
            if b == 0 or start is None or cols[start][row] != 0:
                prev = None
                segments += 1
            state, bad = arrange(cols, params, un, row, prev)
            if bad:
                bad_rows.append(row)
            if check:
                prev = permute(params, state)
            elif un["layout"] == "trace":
                tr = trace(params, state)
                for rho, s in enumerate(tr):
                    for j in range(t):
                        out[j][row + rho] = s[j]
                prev = tr[-1]
            else:
                prev = permute(params, state)
                for c, name in enumerate(un["cols"]):
                    out[c][row] = state[int(name[2:])] if name.startswith("in") else prev[int(name[3:])]
            last = b + 1 >= nb or start is None or cols[start][row + P] != 0
            if check and last and prev[un["digest"]] != cols[un["expect"]][row]:
                miss_rows.append(row)
        rows += out
        st["blocks"].append(nb)
        st["segments"].append(segments)
        st["bad_pos"].append(len(bad_rows))
        st["first_bad_pos"].append(bad_rows[0] if bad_rows else None)
        st["mismatch"].append(len(miss_rows))
        st["first_mismatch"].append(miss_rows[0] if miss_rows else None)
    if usable is not None:
        tail = list(tail)
        assert len(tail) == len(rows) * (T - n)
        for c, r in enumerate(rows):
            r[n:] = tail[c * (T - n):(c + 1) * (T - n)]
    return rows, st
