"""CPU tests (`-m "not gpu"`) of kzg_rows_commit_poseidon2: the reference in Python integers (tests/poseidon2_ref.py), the
engine's encoder poseidon2_call with every refusal, the header's constants and symbols, and the build list.

A search of this machine (the Python packages that import, the files of the tree) found no Poseidon2 implementation and no
published known-answer vector, and the library generates no constants.  The reference is therefore pinned by identities: (a)
the addition chain of M4 against the dense matrix, (b) a second formulation with dense matrices for both layers, (c) an
inverse permutation, (d) the tie to tests/poseidon_ref.py where diag = 1 makes I = E at t = 2, 3, and (e) the two gates of the
trace, written independently of permute.

The tests of the reference (the identities, the product counts and the `columns` self-test) exercise tests/poseidon2_ref.py
alone, so they pass on a tree without the feature once that file exists; they pin the definition the GPU tests compare with.
The encoder, refusal, header and build-list tests, and every GPU test, fail without the feature."""
import ctypes
import os
import random
import re

import pytest

from tests import poseidon2_ref as p2
from tests import poseidon_ref as pr
from zkp_subnet_amd import _native, build
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import HipEngine

R = pr.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "kzg_mi355x.h")
SHAPES = [(2, 2, 0), (2, 2, 1), (3, 2, 2), (3, 8, 56), (4, 2, 1), (4, 4, 3), (8, 2, 1), (8, 8, 5)]


def states(t, rnd, count=6):
    return [[0] * t, [R - 1] * t, [1] + [0] * (t - 1)] + [[rnd.randrange(R) for _ in range(t)] for _ in range(count)]


# ---------------------------------------------------------------------------------------------------- the reference
def test_the_product_counts_of_the_schedule():
    count = lambda t, f, p: f * 3 * t + p * (3 + t)   # noqa: E731
    assert (count(3, 8, 56), count(8, 8, 57)) == (408, 819)


def test_the_addition_chain_is_the_dense_m4():
    """(a) on random and extreme inputs"""
    rnd = random.Random(2)
    xs = [[0] * 4, [R - 1] * 4, [0, R - 1, 0, R - 1], [R - 1, 0, R - 1, 0]] + [[rnd.randrange(R) for _ in range(4)] for _ in range(50)]
    xs += [[(R - 1) * int(i == j) for j in range(4)] for i in range(4)]
    for x in xs:
        assert p2.m4_chain(x) == [sum(m * v for m, v in zip(row, x)) % R for row in p2.M4]


@pytest.mark.parametrize("t", p2.WIDTHS)
def test_the_external_layer_is_its_dense_matrix(t):
    rnd = random.Random(3 + t)
    E = p2.dense_external(t)
    if t == 8:
        assert E[:8] == [10, 14, 2, 6, 5, 7, 1, 3] and E[4 * 8:5 * 8] == [5, 7, 1, 3, 10, 14, 2, 6]
    for s in states(t, rnd):
        assert p2.external(t, s) == p2.mat_vec(E, t, s)


@pytest.mark.parametrize("t,full,partial", SHAPES)
def test_a_second_formulation_agrees(t, full, partial):
    """(b)"""
    rnd = random.Random(20 * t + full + partial)
    params = p2.make_params(t, full, partial, 200 + t)
    for s in states(t, rnd):
        assert p2.permute_dense(params, s) == p2.permute(params, s)


@pytest.mark.parametrize("t,full,partial", SHAPES)
def test_the_inverse_permutation_undoes_the_forward_one(t, full, partial):
    """(c)"""
    rnd = random.Random(10 * t + full + partial)
    params = p2.make_params(t, full, partial, 100 + t)
    for s in states(t, rnd):
        out = p2.permute(params, s)
        assert out != s and p2.unpermute(params, out) == s
        assert p2.permute(params, p2.unpermute(params, s)) == s


@pytest.mark.parametrize("t,full,partial", [(2, 2, 0), (2, 2, 3), (3, 2, 2), (3, 8, 56)])
def test_the_tie_to_the_poseidon_reference(t, full, partial):
    """(d) diag all ones makes I = E; then permute is poseidon_ref.permute with mds the dense E and rc the round-major merge
    of rc_full and (rc_partial[rho], 0, .., 0), applied to E(input)"""
    rnd = random.Random(40 * t + full + partial)
    params = dict(p2.make_params(t, full, partial, 400 + t), diag=[1] * t)
    assert p2.dense_internal(params) == p2.dense_external(t)
    for s in states(t, rnd):
        assert p2.permute(params, s) == pr.permute(tie_params(params), p2.external(t, s))


def tie_params(params):
    """the Poseidon parameters of identity (d)"""
    t, full, partial, half = params["t"], params["full"], params["partial"], params["full"] // 2
    rc = params["rc_full"][:half * t]
    for c in params["rc_partial"]:
        rc += [c] + [0] * (t - 1)
    rc += params["rc_full"][half * t:]
    return {"t": t, "full": full, "partial": partial, "rc": rc, "mds": p2.dense_external(t)}


@pytest.mark.parametrize("t,full,partial", SHAPES)
def test_trace_blocks_satisfy_the_two_gates_and_end_in_the_row_output(t, full, partial):
    """(e) the two layouts of columns() against each other; row 0 -> row 1 is the linear gate s[+1] = E s; row 1 + rho -> row 2 +
    rho the round gate, written with pow and the dense matrices and no helper of permute"""
    rnd = random.Random(30 * t + full + partial)
    params = p2.make_params(t, full, partial, 300 + t)
    Rn = full + partial
    P, T = Rn + 3, 4 * (Rn + 3) + 3
    cols = [[rnd.randrange(R) for _ in range(T)] for _ in range(t)]
    ins = list(range(t))
    rows, st = p2.columns(cols, params, [{"mode": "rounds", "in": ins, "period": P},
                                         {"mode": "row", "in": ins, "out": list(reversed(range(t)))}])
    tr, hashed = rows[:t], rows[t:][::-1]
    assert st == {"perms": [4, T], "mismatch": [0, 0], "first_mismatch": [None, None]}
    E, In, half = p2.dense_external(t), p2.dense_internal(params), full // 2
    for b in range(4):
        assert [tr[j][b * P] for j in range(t)] == [cols[j][b * P] for j in range(t)]
        assert [tr[j][b * P + 1 + Rn] for j in range(t)] == [hashed[j][b * P] for j in range(t)]
        assert all(tr[j][b * P + Rn + 2] == 0 for j in range(t))
        for j in range(t):
            assert (sum(E[j * t + k] * tr[k][b * P] for k in range(t)) - tr[j][b * P + 1]) % R == 0
        nf = 0
        for rho in range(Rn):
            at = b * P + 1 + rho
            sbox_all = rho < half or rho >= half + partial
            for j in range(t):
                acc = 0
                for k in range(t):
                    if sbox_all:
                        acc += E[j * t + k] * pow(tr[k][at] + params["rc_full"][nf * t + k], 5, R)
                    else:
                        acc += In[j * t + k] * (pow(tr[0][at] + params["rc_partial"][rho - half], 5, R) if k == 0 else tr[k][at])
                assert (acc - tr[j][at + 1]) % R == 0
            nf += sbox_all
        assert nf == full
    assert all(tr[j][r] == 0 for j in range(t) for r in range(4 * P, T))


def test_columns_checks_immediates_and_the_usable_layout():
    params = p2.make_params(3, 2, 1, 7)
    rnd = random.Random(7)
    T, u = 16, 13
    a = [rnd.randrange(R) for _ in range(T)]
    h = [p2.permute(params, [5, a[r], a[r]])[1] for r in range(T)]
    bad = list(h)
    bad[4], bad[9], bad[14] = 0, 1, 2
    units = [{"mode": "row", "in": [("imm", 5), 0, 0], "out": [1]},
             {"mode": "row", "in": [("imm", 5), 0, 0], "out": [1], "expect": [1]},
             {"mode": "row", "in": [("imm", 5), 0, 0], "out": [1], "expect": [2]},
             {"mode": "rounds", "in": [0, ("imm", 0), ("imm", R - 1)], "period": 5}]
    tail = [rnd.randrange(R) for _ in range(4 * (T - u))]
    rows, st = p2.columns([a, h, bad], params, units, u, tail)
    assert st == {"perms": [u, u, u, 2], "mismatch": [0, 0, 2, 0], "first_mismatch": [None, None, 4, None]}
    assert len(rows) == 4 and rows[0][:u] == h[:u] and rows[0][u:] == tail[:3] and rows[3][u:] == tail[9:]
    assert rows[1][10] == 0 and [rows[1 + j][5] for j in range(3)] == [a[5], 0, R - 1]
    rows, st = p2.columns([a, h, bad], params, units)
    assert st["perms"] == [T, T, T, 3] and st["mismatch"] == [0, 0, 3, 0]


# ---------------------------------------------------------------------------------------------------- the encoder
def test_call_encoder():
    params = p2.make_params(3, 2, 1, 9)
    b32 = lambda vs: b"".join(v.to_bytes(32, "big") for v in vs)   # noqa: E731
    par, recs = HipEngine.poseidon2_call(
        dict(params, rc_full=[hex(v) for v in params["rc_full"]], rc_partial=[str(v) for v in params["rc_partial"]],
             diag=[v.to_bytes(32, "big") for v in params["diag"]]),
        [{"mode": "row", "in": [2, ("imm", "7"), 2], "out": [2, 0]},
         {"mode": "row", "in": [0, 1, 2], "out": [1], "expect": [5]},
         {"mode": "rounds", "in": [("imm", R - 1), 0, 1], "period": 5}])
    IMM = _native.KZG_POSEIDON_IMM
    assert par == (3, 2, 1, b32(params["rc_full"]), b32(params["rc_partial"]), b32(params["diag"]))
    z = bytes(32)
    assert recs[0] == (_native.KZG_POSEIDON_ROW, 0, 2, 0, [2, IMM, 2, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0, 0, 0], [0] * 8,
                       [z, (7).to_bytes(32, "big")] + [z] * 6)
    assert recs[1][:4] == (_native.KZG_POSEIDON_ROW, _native.KZG_POSEIDON_CHECK, 1, 0) and recs[1][6][0] == 5
    assert recs[2][:4] == (_native.KZG_POSEIDON_ROUNDS, 0, 3, 5) and recs[2][5][:3] == [0, 1, 2]
    assert recs[2][7][0] == (R - 1).to_bytes(32, "big")
    pp = _native.Poseidon2Params(*par)
    assert (pp.t, pp.full, pp.partial) == (3, 2, 1)
    assert [f[0] for f in _native.Poseidon2Params._fields_] == ["t", "full", "partial", "rc_full_be32", "rc_partial_be32", "diag_be32"]
    assert ctypes.sizeof(_native.Poseidon2Params) == 16 + 3 * ctypes.sizeof(ctypes.c_void_p)
    par0, _ = HipEngine.poseidon2_call(p2.make_params(8, 2, 0, 1), [{"mode": "row", "in": list(range(8)), "out": [0]}])
    assert par0[:3] == (8, 2, 0) and par0[4] == b"" and len(par0[3]) == 32 * 16 and len(par0[5]) == 32 * 8


P3 = p2.make_params(3, 2, 1, 11)
ROW = {"mode": "row", "in": [0, 1, 2], "out": [0]}
RND = {"mode": "rounds", "in": [0, 1, 2], "period": 5}
HEAD = "kzg_mi355x E_ARG: commit_poseidon2: poseidon2: "
KEYS = "t, full, partial, rc_full, rc_partial, diag"


@pytest.mark.parametrize("params,units,why", [
    (dict(P3, t=1), [ROW], "the width t must be one of 2, 3, 4, 8"), (dict(P3, t=5), [ROW], "the width t must be one of 2, 3, 4, 8"),
    (dict(P3, t=6), [ROW], "the width t must be one of 2, 3, 4, 8"), (dict(P3, t=7), [ROW], "the width t must be one of 2, 3, 4, 8"),
    (dict(P3, t=9), [ROW], "the width t must be one of 2, 3, 4, 8"), (dict(P3, t=True), [ROW], "the width t must be one of 2, 3, 4, 8"),
    (dict(P3, t=1 << 40), [ROW], "the width t must be one of 2, 3, 4, 8"),
    (dict(P3, full=3), [ROW], "the number of full rounds R_F must be even and in [2, 16]"),
    (dict(P3, full=0), [ROW], "the number of full rounds R_F must be even and in [2, 16]"),
    (dict(P3, full=18), [ROW], "the number of full rounds R_F must be even and in [2, 16]"),
    (dict(P3, partial=129), [ROW], "the number of partial rounds R_P must be in [0, 128]"),
    (dict(P3, partial=-1), [ROW], "the number of partial rounds R_P must be in [0, 128]"),
    (dict(P3, rc_full=P3["rc_full"][:-1]), [ROW], "rc_full must be a list of t R_F = 6 scalars"),
    (dict(P3, rc_partial=P3["rc_partial"] + [1]), [ROW], "rc_partial must be a list of R_P = 1 scalars"),
    (dict(P3, rc_partial=None), [ROW], "rc_partial must be a list of R_P = 1 scalars"),
    (dict(P3, diag=P3["diag"] + [1]), [ROW], "diag must be a list of t = 3 scalars"),
    (dict(P3, rc_full=[R] + P3["rc_full"][1:]), [ROW], "a round constant must be a canonical scalar (< r)"),
    (dict(P3, rc_partial=[R + 5]), [ROW], "a round constant must be a canonical scalar (< r)"),
    (dict(P3, diag=P3["diag"][:-1] + [R]), [ROW], "a diagonal entry must be a canonical scalar (< r)"),
    (dict(P3, rc_full=["zz"] + P3["rc_full"][1:]), [ROW], "a round constant must be an integer, a decimal or 0x string, or 32 bytes"),
    (dict(P3, diag=[-1] + P3["diag"][1:]), [ROW], "a diagonal entry must be a non-negative integer"),
    (dict(P3, rc_partial=[b"12"]), [ROW], "a round constant given as bytes must be of 32 bytes"),
    ({k: v for k, v in P3.items() if k != "diag"}, [ROW], "params is a mapping with exactly " + KEYS),
    (dict(P3, mds=[1] * 9), [ROW], "params is a mapping with exactly " + KEYS),
    (P3, [], "units must be a list of 1 .. 8 entries (n_units)"), (P3, [ROW] * 9, "units must be a list of 1 .. 8 entries (n_units)"),
    (P3, "x", "units must be a list of 1 .. 8 entries (n_units)"),
    (P3, [5], "a unit is a mapping with mode, in and the fields of its mode"),
    (P3, [dict(ROW, mode="sponge")], "unknown mode 'sponge' (one of \"row\", \"rounds\")"),
    (P3, [dict(ROW, foo=1)], "unknown field 'foo' (the fields are mode, in, out, expect, period)"),
    (P3, [dict(ROW, **{"in": [0, 1]})], 'in must hold t = 3 entries, each a row index or ("imm", value)'),
    (P3, [dict(ROW, **{"in": [0, 1, -1]})], 'an entry of in must be a row index, an integer in [0, 2^32 - 1), or ("imm", value)'),
    (P3, [dict(ROW, **{"in": [0, 1, ("im", 1)]})], 'an immediate is ("imm", value)'),
    (P3, [dict(ROW, **{"in": [0, 1, ("imm", R)]})], "an immediate must be a canonical scalar (< r)"),
    (P3, [dict(ROW, out=[])], "out must hold 1 .. t = 3 state indices"),
    (P3, [dict(ROW, out=[0, 1, 2, 0])], "out must hold 1 .. t = 3 state indices"),
    (P3, [dict(ROW, out=[3])], "an out index must be an integer below t = 3"), (P3, [dict(ROW, out=[1, 1])], "an out index is repeated"),
    (P3, [dict(ROW, expect=[1, 2])], "expect must hold one row per entry of out"),
    (P3, [dict(ROW, expect=["a"])], "an entry of expect must be a row index, an integer in [0, 2^32 - 1)"),
    (P3, [dict(ROW, period=5)], "period belongs to rounds units, not to row"),
    (P3, [dict(RND, expect=[0, 1, 2])], "expect belongs to row units, not to rounds"),
    (P3, [dict(RND, out=[0])], "out belongs to row units: a rounds unit commits all t columns"),
    (P3, [dict(RND, period=4)], "the period P of a rounds unit must be an integer in [R + 2, 2^32), R + 2 = 5"),
    (P3, [dict(RND, period=None)], "the period P of a rounds unit must be an integer in [R + 2, 2^32), R + 2 = 5"),
    (P3, [dict(RND, period=1 << 32)], "the period P of a rounds unit must be an integer in [R + 2, 2^32), R + 2 = 5"),
    (P3, [dict(ROW, out=[0, 1, 2])] * 6, "n_out: the units give 18 output rows, at most 16 fit one call"),
    (P3, [RND] * 6, "n_out: the units give 18 output rows, at most 16 fit one call"),
    (P3, [dict(ROW, **{"in": [3 * k, 3 * k + 1, 3 * k + 2]}) for k in range(6)],
     "the units read 18 distinct input rows, at most 16 fit one call"),
    (P3, [dict(ROW, **{"in": [k, k, k]}, expect=[20 + k]) for k in range(8)], None),
])
def test_python_refusals_whole(params, units, why):
    if why is None:   # 8 inputs and 8 expected rows: exactly 16 distinct rows, and checks count nothing against n_out
        par, recs = HipEngine.poseidon2_call(params, units)
        assert len(recs) == 8 and all(r[1] == _native.KZG_POSEIDON_CHECK for r in recs)
        return
    with pytest.raises(KzgError) as ei:
        HipEngine.poseidon2_call(params, units)
    assert ei.value.code == _native.KZG_E_ARG and str(ei.value) == HEAD + why, str(ei.value)


def test_a_period_of_r_plus_two_is_taken_and_poseidon_keeps_r_plus_one():
    HipEngine.poseidon2_call(P3, [RND])
    q = pr.make_params(3, 2, 1, 11)
    HipEngine.poseidon_call(q, [dict(RND, period=4)])
    with pytest.raises(KzgError) as ei:
        HipEngine.poseidon_call(q, [dict(RND, period=3)])
    assert str(ei.value).endswith("the period P of a rounds unit must be an integer in [R + 1, 2^32), R + 1 = 4")


# ---------------------------------------------------------------------------------------------------- the header, the build
def test_header_constants_and_symbols():
    text = open(HEADER).read()
    for name in ("KZG_POSEIDON2_WIDTHS", "KZG_POSEIDON2_MAX_FULL", "KZG_POSEIDON2_MAX_PARTIAL", "KZG_POSEIDON2_MAX_UNITS"):
        m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, text)
        assert m and int(m.group(1), 0) == getattr(_native, name), name
    assert tuple(t for t in range(32) if _native.KZG_POSEIDON2_WIDTHS >> t & 1) == p2.WIDTHS == HipEngine._POSEIDON2_WIDTHS
    assert (_native.KZG_POSEIDON2_MAX_FULL, _native.KZG_POSEIDON2_MAX_PARTIAL, _native.KZG_POSEIDON2_MAX_UNITS,
            _native.KZG_MAX_BATCH_OPEN) == (p2.MAX_FULL, p2.MAX_PARTIAL, p2.MAX_UNITS, p2.MAX_ROWS)
    for sym in ("kzg_rows_commit_poseidon2", "kzg_multi_rows_commit_poseidon2"):
        assert sym in _native.SYMBOLS and re.search(r"\bint %s\(" % sym, text)
    assert len(_native.SYMBOLS["kzg_multi_rows_commit_poseidon2"][1]) == len(_native.SYMBOLS["kzg_rows_commit_poseidon2"][1]) + 1
    assert re.search(r"typedef struct kzg_poseidon2_params \{.*?rc_full_be32;.*?rc_partial_be32;.*?diag_be32;.*?\} kzg_poseidon2_params;",
                     text, re.S)
    for word in ("M4 = [[5, 7, 1, 3], [4, 6, 1, 1], [1, 3, 5, 7], [1, 1, 4, 6]]", "diag_i = mu_i - 1", "P >= R + 2", 'begins "poseidon2: "',
                 "generating constants and published instance tables", "t = 12 .. 24", "exponents other than 5",
                 "t lanes per block for traces", "any change to the Poseidon kernels"):
        assert word in re.sub(r"\s*\n \* ", " ", text), word
    from zkp_subnet_amd import Client, MultiDeviceClient
    assert callable(Client.worker_commit_poseidon2) and callable(MultiDeviceClient.worker_commit_poseidon2)
    assert callable(HipEngine.commit_poseidon2)


def test_the_kernel_file_is_built_and_mapped():
    assert "fr_poseidon2.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "fr_poseidon2.hip"))
    ctx = open(os.path.join(build.CSRC, "ctx.hip.h")).read()
    assert re.search(r"^//\s+fr_poseidon2\.hip\s+the kernel of kzg_rows_commit_poseidon2", ctx, re.M)
