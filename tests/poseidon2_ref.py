"""The definition of kzg_rows_commit_poseidon2 in Python integers: the Poseidon2 permutation over the scalar field of BLS12-381
with the S-box x^5 and the caller's constants, in both layouts (one permutation per row; the round trace in blocks of P >= R + 2
rows), with the checks, the usable layout and its tail.

    s <- E(s); R_F / 2 full rounds; R_P partial rounds; R_F / 2 full rounds
    a full round     s_i += rc_full[rho' t + i]; s_i <- s_i^5 for every i; s <- E(s)   (rho' counts the full rounds of both halves)
    a partial round  s_0 += rc_partial[rho'']; s_0 <- s_0^5; s <- I(s)
    E  t = 2, 3: y_i = s_i + sum_j s_j; t = 4: M4; t = 8: circ(2 M4, M4), M4 by its addition chain
    I  y_i = diag_i s_i + sum_j s_j

No Poseidon2 implementation and no published known-answer vector is available to this repository, and the library generates no
constants: tests/test_poseidon2_cpu.py pins this file by identities (the chain against the dense M4, a dense second
formulation, an inverse permutation, the tie to tests/poseidon_ref.py where I = E, and the two gates of the trace)."""
import random

from tests.poseidon_ref import FIFTH_ROOT, R, mat_inv, state_at

WIDTHS, MAX_FULL, MAX_PARTIAL, MAX_UNITS, MAX_ROWS = (2, 3, 4, 8), 16, 128, 8, 16
M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]]


def make_params(t, full, partial, seed):
    """seeded random constants; the diagonal avoids 0 and -1, which no instance would use"""
    rnd = random.Random(seed)
    return {"t": t, "full": full, "partial": partial, "rc_full": [rnd.randrange(R) for _ in range(t * full)],
            "rc_partial": [rnd.randrange(R) for _ in range(partial)], "diag": [rnd.randrange(1, R - 1) for _ in range(t)]}


def m4_chain(x):
    """M4 x by the addition chain: no product"""
    x0, x1, x2, x3 = x
    a = x0 + x1
    b = x2 + x3
    c = 2 * x1 + b
    d = 2 * x3 + a
    e = 4 * b + d
    f = 4 * a + c
    return [(d + f) % R, f % R, (c + e) % R, e % R]


def external(t, s):
    if t in (2, 3):
        tot = sum(s)
        return [(v + tot) % R for v in s]
    if t == 4:
        return m4_chain(s)
    assert t == 8
    u = m4_chain(s[:4]) + m4_chain(s[4:])
    return [(u[4 * k + j] + u[j] + u[4 + j]) % R for k in range(2) for j in range(4)]


def internal(params, s):
    tot = sum(s)
    return [(d * v + tot) % R for d, v in zip(params["diag"], s)]


def n_rounds(params):
    return params["full"] + params["partial"]


def is_full(params, rho):
    half = params["full"] // 2
    return rho < half or rho >= half + params["partial"]


def round_of(params, rho, s):
    """round rho of the R = R_F + R_P rounds behind the first E"""
    t, half = params["t"], params["full"] // 2
    if is_full(params, rho):
        k = rho if rho < half else rho - params["partial"]
        return external(t, [pow((s[i] + params["rc_full"][k * t + i]) % R, 5, R) for i in range(t)])
    return internal(params, [pow((s[0] + params["rc_partial"][rho - half]) % R, 5, R)] + list(s[1:]))


def trace(params, state):
    """the R + 2 rows of a trace block: the input, E(input) = the state before round 0, .., the state behind the last round"""
    out = [list(state), external(params["t"], list(state))]
    for rho in range(n_rounds(params)):
        out.append(round_of(params, rho, out[-1]))
    return out


def permute(params, state):
    return trace(params, state)[-1]


def columns(cols, params, units, usable=None, tail=()):
    """(the committed rows of all units in unit order, {"perms", "mismatch", "first_mismatch"} per unit) as the device call
    returns them.  cols: the concatenated input rows as lists of T integers; tail: column-major over the committed columns"""
    T = len(cols[0])
    n = T if usable is None else usable
    t, Rn = params["t"], n_rounds(params)
    rows, perms, mismatch, first = [], [], [], []
    for un in units:
        if un["mode"] == "rounds":
            P = un["period"]
            assert P >= Rn + 2
            out = [[0] * T for _ in range(t)]
            for b in range(n // P):
                for k, s in enumerate(trace(params, state_at(cols, un["in"], b * P))):
                    for j in range(t):
                        out[j][b * P + k] = s[j]
            rows += out
            perms.append(n // P)
            mismatch.append(0)
            first.append(None)
            continue
        memo = {}
        res = []
        for r in range(n):
            key = tuple(state_at(cols, un["in"], r))
            if key not in memo:
                memo[key] = permute(params, list(key))
            res.append(memo[key])
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


# ---------------------------------------------------------------------------------------------------- for the identities
def dense_external(t):
    """E as a dense t x t matrix, row-major, written from the definition's matrices and not from the chain"""
    if t in (2, 3):
        return [2 if i == j else 1 for i in range(t) for j in range(t)]
    if t == 4:
        return [v for row in M4 for v in row]
    assert t == 8
    return [(2 if i // 4 == j // 4 else 1) * M4[i % 4][j % 4] for i in range(8) for j in range(8)]


def dense_internal(params):
    t = params["t"]
    return [(1 + params["diag"][i]) % R if i == j else 1 for i in range(t) for j in range(t)]


def mat_vec(M, t, s):
    return [sum(M[i * t + j] * s[j] for j in range(t)) % R for i in range(t)]


def permute_dense(params, state):
    """a second formulation: dense matrices for both layers, the rounds listed by kind"""
    t, full, partial = params["t"], params["full"], params["partial"]
    E, In = dense_external(t), dense_internal(params)
    s = mat_vec(E, t, list(state))
    kinds = ["full"] * (full // 2) + ["partial"] * partial + ["full"] * (full // 2)
    cf = [params["rc_full"][k * t:(k + 1) * t] for k in range(full)]
    cp = list(params["rc_partial"])
    for kind in kinds:
        if kind == "full":
            s = mat_vec(E, t, [(a + b) ** 5 % R for a, b in zip(s, cf.pop(0))])
        else:
            s = mat_vec(In, t, [(s[0] + cp.pop(0)) ** 5 % R] + s[1:])
    return s


def unpermute(params, state):
    """the inverse permutation: the inverted dense matrices, the fifth root and the constants, rounds backwards, then E^-1"""
    t, half = params["t"], params["full"] // 2
    Ei, Ii = mat_inv(dense_external(t), t), mat_inv(dense_internal(params), t)
    s = list(state)
    for rho in reversed(range(n_rounds(params))):
        if is_full(params, rho):
            k = rho if rho < half else rho - params["partial"]
            x = mat_vec(Ei, t, s)
            s = [(pow(x[i], FIFTH_ROOT, R) - params["rc_full"][k * t + i]) % R for i in range(t)]
        else:
            x = mat_vec(Ii, t, s)
            s = [(pow(x[0], FIFTH_ROOT, R) - params["rc_partial"][rho - half]) % R] + x[1:]
    return mat_vec(Ei, t, s)
