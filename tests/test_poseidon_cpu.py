"""kzg_rows_commit_poseidon without a GPU.  No Poseidon implementation and no published known-answer vector is available here,
so the reference in Python integers (tests/poseidon_ref.py) is pinned by the identities it must satisfy: the S-box is a
bijection, an inverse permutation undoes the forward one, the trace's last row is the row layout's output, consecutive trace
rows satisfy the round gate written independently, and a second formulation agrees.  Then the encoder, every refusal the Python
layer makes, and the header's constants against _native.py."""
import ctypes
import os
import random
import re

import pytest

from tests import poseidon_ref as pr
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import HipEngine

R = pr.R
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kzg_mi355x.h")
SHAPES = [(2, 2, 0), (2, 2, 1), (3, 2, 2), (3, 8, 57), (4, 2, 1), (5, 4, 3), (8, 2, 1), (8, 8, 5)]


def states(t, rnd, count=6):
    return [[0] * t, [R - 1] * t, [1] + [0] * (t - 1)] + [[rnd.randrange(R) for _ in range(t)] for _ in range(count)]


# ---------------------------------------------------------------------------------------------------- the reference
def test_the_sbox_is_a_bijection():
    assert (R - 1) % 5 != 0 and 5 * pr.FIFTH_ROOT % (R - 1) == 1
    rnd = random.Random(1)
    for x in [0, 1, R - 1] + [rnd.randrange(R) for _ in range(50)]:
        assert pow(pow(x, 5, R), pr.FIFTH_ROOT, R) == x


@pytest.mark.parametrize("t,full,partial", SHAPES)
def test_the_inverse_permutation_undoes_the_forward_one(t, full, partial):
    rnd = random.Random(10 * t + full + partial)
    params = pr.make_params(t, full, partial, 100 + t)
    Mi = pr.mat_inv(params["mds"], t)
    for i in range(t):
        for j in range(t):
            assert sum(params["mds"][i * t + k] * Mi[k * t + j] for k in range(t)) % R == int(i == j)
    for s in states(t, rnd):
        out = pr.permute(params, s)
        assert out != s and pr.unpermute(params, out) == s
        assert pr.permute(params, pr.unpermute(params, s)) == s


@pytest.mark.parametrize("t,full,partial", SHAPES)
def test_a_second_formulation_agrees(t, full, partial):
    rnd = random.Random(20 * t + full + partial)
    params = pr.make_params(t, full, partial, 200 + t)
    for s in states(t, rnd):
        assert pr.permute_nested(params, s) == pr.permute(params, s)


@pytest.mark.parametrize("t,full,partial", SHAPES)
def test_trace_blocks_end_in_the_row_output_and_satisfy_the_round_gate(t, full, partial):
    """the two layouts of columns() against each other, and every pair of consecutive rows of a block against the gate
    s_j[+1] = sum_k M_jk (s_k + rc_k)^5 (partial rounds: k = 0 only under the S-box), written with pow and no helper"""
    rnd = random.Random(30 * t + full + partial)
    params = pr.make_params(t, full, partial, 300 + t)
    Rn = full + partial
    P, T = Rn + 2, 4 * (Rn + 2) + 3
    cols = [[rnd.randrange(R) for _ in range(T)] for _ in range(t)]
    ins = list(range(t))
    rows, st = pr.columns(cols, params, [{"mode": "rounds", "in": ins, "period": P},
                                         {"mode": "row", "in": ins, "out": list(reversed(range(t)))}])
    tr, hashed = rows[:t], rows[t:][::-1]
    assert st == {"perms": [4, T], "mismatch": [0, 0], "first_mismatch": [None, None]}
    half = full // 2
    for b in range(4):
        assert [tr[j][b * P] for j in range(t)] == [cols[j][b * P] for j in range(t)]
        assert [tr[j][b * P + Rn] for j in range(t)] == [hashed[j][b * P] for j in range(t)]
        assert all(tr[j][b * P + Rn + 1] == 0 for j in range(t))
        for rho in range(Rn):
            sbox_all = rho < half or rho >= half + partial
            for j in range(t):
                acc = 0
                for k in range(t):
                    u = tr[k][b * P + rho] + params["rc"][rho * t + k]
                    acc += params["mds"][j * t + k] * (pow(u, 5, R) if sbox_all or k == 0 else u)
                assert (acc - tr[j][b * P + rho + 1]) % R == 0
    assert all(tr[j][r] == 0 for j in range(t) for r in range(4 * P, T))


def test_columns_checks_immediates_and_the_usable_layout():
    params = pr.make_params(3, 2, 1, 7)
    rnd = random.Random(7)
    T, u = 16, 13
    a = [rnd.randrange(R) for _ in range(T)]
    h = [pr.permute(params, [5, a[r], a[r]])[1] for r in range(T)]
    bad = list(h)
    bad[4], bad[9], bad[14] = 0, 1, 2
    units = [{"mode": "row", "in": [("imm", 5), 0, 0], "out": [1]},
             {"mode": "row", "in": [("imm", 5), 0, 0], "out": [1], "expect": [1]},
             {"mode": "row", "in": [("imm", 5), 0, 0], "out": [1], "expect": [2]},
             {"mode": "rounds", "in": [0, ("imm", 0), ("imm", R - 1)], "period": 4}]
    tail = [rnd.randrange(R) for _ in range(4 * (T - u))]
    rows, st = pr.columns([a, h, bad], params, units, u, tail)
    assert st == {"perms": [u, u, u, 3], "mismatch": [0, 0, 2, 0], "first_mismatch": [None, None, 4, None]}
    assert len(rows) == 4 and rows[0][:u] == h[:u] and rows[0][u:] == tail[:3] and rows[3][u:] == tail[9:]
    assert rows[1][12] == 0 and [rows[1 + j][8] for j in range(3)] == [a[8], 0, R - 1]
    rows, st = pr.columns([a, h, bad], params, units)
    assert st["perms"] == [T, T, T, 4] and st["mismatch"] == [0, 0, 3, 0]


# ---------------------------------------------------------------------------------------------------- the encoder
def test_call_encoder():
    params = pr.make_params(3, 2, 1, 9)
    par, recs = HipEngine.poseidon_call(
        dict(params, rc=[hex(v) for v in params["rc"]], mds=[v.to_bytes(32, "big") for v in params["mds"]]),
        [{"mode": "row", "in": [2, ("imm", "7"), 2], "out": [2, 0]},
         {"mode": "row", "in": [0, 1, 2], "out": [1], "expect": [5]},
         {"mode": "rounds", "in": [("imm", R - 1), 0, 1], "period": 4}])
    IMM = _native.KZG_POSEIDON_IMM
    assert par == (3, 2, 1, b"".join(v.to_bytes(32, "big") for v in params["rc"]),
                   b"".join(v.to_bytes(32, "big") for v in params["mds"]))
    z = bytes(32)
    assert recs[0] == (_native.KZG_POSEIDON_ROW, 0, 2, 0, [2, IMM, 2, 0, 0, 0, 0, 0], [2, 0, 0, 0, 0, 0, 0, 0], [0] * 8,
                       [z, (7).to_bytes(32, "big")] + [z] * 6)
    assert recs[1][:4] == (_native.KZG_POSEIDON_ROW, _native.KZG_POSEIDON_CHECK, 1, 0) and recs[1][6][0] == 5
    assert recs[2][:4] == (_native.KZG_POSEIDON_ROUNDS, 0, 3, 4) and recs[2][5][:3] == [0, 1, 2]
    assert recs[2][7][0] == (R - 1).to_bytes(32, "big")
    st = HipEngine.poseidon_unit_struct(recs[0])
    assert (st.mode, st.flags, st.n_out, st.period, list(st.in_), list(st.out)) == recs[0][:4] + (recs[0][4], recs[0][5])
    assert bytes(st.imm_be32[1]) == (7).to_bytes(32, "big") and bytes(st.imm_be32[0]) == z
    assert ctypes.sizeof(_native.PoseidonUnit) == 16 + 3 * 32 + 8 * 32


P3 = pr.make_params(3, 2, 1, 11)
ROW = {"mode": "row", "in": [0, 1, 2], "out": [0]}
RND = {"mode": "rounds", "in": [0, 1, 2], "period": 4}


@pytest.mark.parametrize("params,units,why", [
    (dict(P3, t=1), [ROW], "width t"), (dict(P3, t=9), [ROW], "width t"), (dict(P3, t=True), [ROW], "width t"),
    (dict(P3, full=3), [ROW], "R_F must be even"), (dict(P3, full=0), [ROW], "R_F"), (dict(P3, full=18), [ROW], "R_F"),
    (dict(P3, partial=129), [ROW], "R_P"), (dict(P3, partial=-1), [ROW], "R_P"),
    (dict(P3, rc=P3["rc"][:-1]), [ROW], "rc must be a list"), (dict(P3, mds=P3["mds"] + [1]), [ROW], "mds must be a list"),
    (dict(P3, rc=[R] + P3["rc"][1:]), [ROW], "round constant must be a canonical"),
    (dict(P3, mds=P3["mds"][:-1] + [R + 5]), [ROW], "matrix entry must be a canonical"),
    (dict(P3, rc=["zz"] + P3["rc"][1:]), [ROW], "decimal or 0x"), (dict(P3, rc=[-1] + P3["rc"][1:]), [ROW], "non-negative"),
    (dict(P3, rc=[b"12"] + P3["rc"][1:]), [ROW], "32 bytes"),
    ({k: v for k, v in P3.items() if k != "mds"}, [ROW], "params is a mapping"), (dict(P3, alpha=5), [ROW], "params is a mapping"),
    (P3, [], "n_units"), (P3, [ROW] * 9, "n_units"), (P3, "x", "n_units"), (P3, [5], "a unit is a mapping"),
    (P3, [dict(ROW, mode="sponge")], "unknown mode"), (P3, [dict(ROW, foo=1)], "unknown field"),
    (P3, [dict(ROW, **{"in": [0, 1]})], "in must hold t"), (P3, [dict(ROW, **{"in": [0, 1, -1]})], "entry of in"),
    (P3, [dict(ROW, **{"in": [0, 1, ("im", 1)]})], "immediate is"), (P3, [dict(ROW, **{"in": [0, 1, ("imm", R)]})], "immediate must be a canonical"),
    (P3, [dict(ROW, out=[])], "out must hold"), (P3, [dict(ROW, out=[0, 1, 2, 0])], "out must hold"),
    (P3, [dict(ROW, out=[3])], "out index must be"), (P3, [dict(ROW, out=[1, 1])], "repeated"),
    (P3, [dict(ROW, expect=[1, 2])], "one row per entry"), (P3, [dict(ROW, expect=["a"])], "entry of expect"),
    (P3, [dict(ROW, period=4)], "period belongs"), (P3, [dict(RND, expect=[0, 1, 2])], "expect belongs to row units"),
    (P3, [dict(RND, out=[0])], "out belongs"), (P3, [dict(RND, period=3)], "period P"), (P3, [dict(RND, period=None)], "period P"),
    (P3, [dict(RND, period=1 << 32)], "period P"),
    (P3, [dict(ROW, out=[0, 1, 2])] * 6, "n_out"), (P3, [RND] * 6, "n_out"),
    (P3, [dict(ROW, **{"in": [3 * k, 3 * k + 1, 3 * k + 2]}) for k in range(6)], "distinct input rows"),
    (P3, [dict(ROW, **{"in": [k, k, k]}, expect=[20 + k]) for k in range(8)], None),
])
def test_python_refusals(params, units, why):
    if why is None:   # 8 inputs and 8 expected rows: exactly 16 distinct rows, and checks count nothing against n_out
        par, recs = HipEngine.poseidon_call(params, units)
        assert len(recs) == 8 and all(r[1] == _native.KZG_POSEIDON_CHECK for r in recs)
        return
    with pytest.raises(KzgError) as ei:
        HipEngine.poseidon_call(params, units)
    assert ei.value.code == _native.KZG_E_ARG and "poseidon: " in str(ei.value) and why in str(ei.value), str(ei.value)


def test_a_seventeenth_distinct_row_among_inputs_and_expected_rows_is_refused():
    units = [dict(ROW, **{"in": [k, k, k]}, expect=[20 + k]) for k in range(8)]
    units[7] = dict(units[7], **{"in": [7, 7, 40]})
    with pytest.raises(KzgError) as ei:
        HipEngine.poseidon_call(P3, units)
    assert "distinct input rows" in str(ei.value)


def test_header_constants_and_symbols():
    text = open(HEADER).read()
    for name in ("KZG_POSEIDON_ROW", "KZG_POSEIDON_ROUNDS", "KZG_POSEIDON_CHECK", "KZG_POSEIDON_IMM", "KZG_POSEIDON_NONE",
                 "KZG_POSEIDON_MIN_T", "KZG_POSEIDON_MAX_T", "KZG_POSEIDON_MAX_FULL", "KZG_POSEIDON_MAX_PARTIAL",
                 "KZG_POSEIDON_MAX_UNITS"):
        m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, text)
        assert m and int(m.group(1), 0) == getattr(_native, name), name
    assert (_native.KZG_POSEIDON_MIN_T, _native.KZG_POSEIDON_MAX_T, _native.KZG_POSEIDON_MAX_FULL, _native.KZG_POSEIDON_MAX_PARTIAL,
            _native.KZG_POSEIDON_MAX_UNITS, _native.KZG_MAX_BATCH_OPEN) == (pr.MIN_T, pr.MAX_T, pr.MAX_FULL, pr.MAX_PARTIAL,
                                                                           pr.MAX_UNITS, pr.MAX_ROWS)
    for sym in ("kzg_rows_commit_poseidon", "kzg_multi_rows_commit_poseidon"):
        assert sym in _native.SYMBOLS and re.search(r"\bint %s\(" % sym, text)
    assert len(_native.SYMBOLS["kzg_multi_rows_commit_poseidon"][1]) == len(_native.SYMBOLS["kzg_rows_commit_poseidon"][1]) + 1
    for word in ("s_i += rc[rho t + i]", "s'_i = sum_j M[i t + j] s_j", "generating constants (the Grain LFSR)",
                 "the inverse S-box", "the optimised partial-round form", "sponge chaining", "Poseidon2"):
        assert word in text, word
    from zkp_subnet_amd import Client, MultiDeviceClient
    assert callable(Client.worker_commit_poseidon) and callable(MultiDeviceClient.worker_commit_poseidon)
    assert callable(HipEngine.commit_poseidon)
