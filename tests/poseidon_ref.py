"""The definition of kzg_rows_commit_poseidon in Python integers: the plain Hades schedule over the scalar field of BLS12-381
with the S-box x^5, the caller's round constants and matrix, in both layouts (one permutation per row; the round trace in blocks
of P rows), with the checks, the usable layout and its tail.

No Poseidon implementation and no published known-answer vector is available to this repository, and the library generates no
constants (no Grain LFSR): there is nothing to pin the permutation against but its definition.  tests/test_poseidon_cpu.py
therefore pins this file by identities: x^5 is a bijection, an inverse permutation undoes the forward one, the last row of a
trace block is the row layout's output, consecutive trace rows satisfy the round gate written as an independent expression,
and a second formulation through nested lists agrees."""
import random

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
MIN_T, MAX_T, MAX_FULL, MAX_PARTIAL, MAX_UNITS, MAX_ROWS = 2, 8, 16, 128, 8, 16


def cauchy(t, seed=0):
    """a t x t Cauchy matrix 1 / (x_i + y_j), row-major: x_i = seed + i, y_j = seed + t + j, all sums distinct and non-zero"""
    return [pow(seed + i + seed + t + j, R - 2, R) for i in range(t) for j in range(t)]


def make_params(t, full, partial, seed):
    """seeded random round constants and a Cauchy matrix"""
    rnd = random.Random(seed)
    return {"t": t, "full": full, "partial": partial, "rc": [rnd.randrange(R) for _ in range(t * (full + partial))],
            "mds": cauchy(t, 1 + seed % 97)}


def is_full(params, rho):
    half = params["full"] // 2
    return rho < half or rho >= half + params["partial"]


def round_of(params, rho, s):
    """one round: the constants, the S-box (every element in a full round, element 0 in a partial one), the matrix"""
    t, rc, M = params["t"], params["rc"], params["mds"]
    u = [(s[i] + rc[rho * t + i]) % R for i in range(t)]
    x = [pow(u[i], 5, R) if (is_full(params, rho) or i == 0) else u[i] for i in range(t)]
    return [sum(M[i * t + j] * x[j] for j in range(t)) % R for i in range(t)]


def trace(params, state):
    """the R + 1 states: before round 0 .. R - 1 and behind the last"""
    out = [list(state)]
    for rho in range(params["full"] + params["partial"]):
        out.append(round_of(params, rho, out[-1]))
    return out


def permute(params, state):
    return trace(params, state)[-1]


def state_at(cols, ins, row):
    """the state of a unit at `row`: an entry of `in` is a row index or ("imm", value), the value an int or a decimal / 0x string"""
    imm = lambda v: int(v, 0) if isinstance(v, str) else v   # noqa: E731
    return [imm(v[1]) % R if isinstance(v, (list, tuple)) else cols[v][row] for v in ins]


def columns(cols, params, units, usable=None, tail=()):
    """(the committed rows of all units in unit order, {"perms", "mismatch", "first_mismatch"} per unit) as the device call
    returns them.  cols: the concatenated input rows as lists of T integers; tail: column-major over the committed columns"""
    T = len(cols[0])
    n = T if usable is None else usable
    t, Rn = params["t"], params["full"] + params["partial"]
    rows, perms, mismatch, first = [], [], [], []
    for un in units:
        if un["mode"] == "rounds":
            P = un["period"]
            out = [[0] * T for _ in range(t)]
            for b in range(n // P):
                for rho, s in enumerate(trace(params, state_at(cols, un["in"], b * P))):
                    for j in range(t):
                        out[j][b * P + rho] = s[j]
            assert P >= Rn + 1
            rows += out
            perms.append(n // P)
            mismatch.append(0)
            first.append(None)
            continue
        res = [permute(params, state_at(cols, un["in"], r)) for r in range(n)]
        perms.append(n)
        if un.get("expect") is not None:
            badrows = [r for r in range(n) if any(cols[e][r] != res[r][j] for j, e in zip(un["out"], un["expect"]))]
            mismatch.append(len(badrows))
            first.append(badrows[0] if badrows else None)
        else:
            rows += [[res[r][j] for r in range(n)] + [0] * (T - n) for j in un["out"]]
            mismatch.append(0)
            first.append(None)
    if usable is not None:
        tail = list(tail)
        assert len(tail) == len(rows) * (T - n)
        for c, row in enumerate(rows):
            row[n:] = tail[c * (T - n):(c + 1) * (T - n)]
    return rows, {"perms": perms, "mismatch": mismatch, "first_mismatch": first}


# ---------------------------------------------------------------------------------------------------- the inverse, for the tests
def mat_inv(M, t):
    """the inverse of a t x t matrix over Fr (row-major), by Gauss-Jordan"""
    A = [[M[i * t + j] for j in range(t)] + [int(i == j) for j in range(t)] for i in range(t)]
    for c in range(t):
        p = next(r for r in range(c, t) if A[r][c])
        A[c], A[p] = A[p], A[c]
        inv = pow(A[c][c], R - 2, R)
        A[c] = [v * inv % R for v in A[c]]
        for r in range(t):
            if r != c and A[r][c]:
                f = A[r][c]
                A[r] = [(v - f * w) % R for v, w in zip(A[r], A[c])]
    return [A[i][t + j] for i in range(t) for j in range(t)]


FIFTH_ROOT = pow(5, -1, R - 1)   # (r - 1 is no multiple of 5: x -> x^5 is a bijection of Fr and x^(1/5) = x^FIFTH_ROOT)


def unpermute(params, state):
    """the inverse permutation: M^-1, the fifth root and the constants, rounds backwards"""
    t, rc = params["t"], params["rc"]
    Mi = mat_inv(params["mds"], t)
    s = list(state)
    for rho in reversed(range(params["full"] + params["partial"])):
        x = [sum(Mi[i * t + j] * s[j] for j in range(t)) % R for i in range(t)]
        u = [pow(x[i], FIFTH_ROOT, R) if (is_full(params, rho) or i == 0) else x[i] for i in range(t)]
        s = [(u[i] - rc[rho * t + i]) % R for i in range(t)]
    return s


def permute_nested(params, state):
    """a second formulation: the matrix and the constants as nested lists, matrix-vector products through zip"""
    t, full, partial = params["t"], params["full"], params["partial"]
    M = [params["mds"][i * t:(i + 1) * t] for i in range(t)]
    C = [params["rc"][k * t:(k + 1) * t] for k in range(full + partial)]
    kinds = ["full"] * (full // 2) + ["partial"] * partial + ["full"] * (full // 2)
    s = list(state)
    for kind, c in zip(kinds, C):
        s = [(a + b) % R for a, b in zip(s, c)]
        s = [v ** 5 % R for v in s] if kind == "full" else [s[0] ** 5 % R] + s[1:]
        s = [sum(m * v for m, v in zip(row, s)) % R for row in M]
    return s
