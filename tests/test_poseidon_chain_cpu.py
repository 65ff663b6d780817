"""kzg_rows_commit_poseidon_chain without a GPU.  The permutation is pinned by tests/test_poseidon_cpu.py; the reference of the
chains (tests/poseidon_chain_ref.py) is pinned here by identities: a sponge with no start column is the rounds unit of
tests/poseidon_ref.py, a sponge over k blocks is an absorb loop written here without it, every leaf of a tree built bottom-up
by a function written here reaches the root through its path chain, and the two layouts agree.  Then the encoder, every
refusal the Python layer makes, and the header's constants against _native.py."""
import ctypes
import os
import random
import re

import pytest

from tests import poseidon_chain_ref as pc
from tests import poseidon_ref as pr
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import HipEngine

R = pr.R
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kzg_mi355x.h")


def rand_cols(k, T, rnd):
    return [[rnd.randrange(R) for _ in range(T)] for _ in range(k)]


# ---------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("t,full,partial", [(2, 2, 1), (3, 2, 2), (3, 8, 57), (5, 4, 3), (8, 2, 1)])
def test_a_sponge_without_a_start_column_is_the_rounds_unit(t, full, partial):
    rnd = random.Random(t + full + partial)
    params = pr.make_params(t, full, partial, 500 + t)
    P = full + partial + 2
    T = 3 * P + 2
    cols = rand_cols(t, T, rnd)
    ins = [("imm", 7)] + list(range(1, t))
    want, wst = pr.columns(cols, params, [{"mode": "rounds", "in": ins, "period": P}])
    got, st = pc.columns(cols, params, [{"mode": "sponge", "in": ins, "start": None, "period": P, "layout": "trace"}])
    assert got == want and st["blocks"] == wst["perms"] == [3] and st["segments"] == [3]
    assert st["bad_pos"] == [0] and st["mismatch"] == [0] and st["first_mismatch"] == [None]


def absorb(params, tag, message):
    """the sponge written on its own: capacity element 0 starts at `tag`, the rate elements absorb t - 1 cells per block"""
    t = params["t"]
    state, outs = [tag] + [0] * (t - 1), []
    for k in range(0, len(message), t - 1):
        for j, m in enumerate(message[k:k + t - 1]):
            state[1 + j] = (state[1 + j] + m) % R
        state = pr.permute(params, state)
        outs.append(list(state))
    return outs


@pytest.mark.parametrize("t,k", [(2, 1), (2, 5), (3, 4), (5, 3)])
def test_a_sponge_over_k_blocks_is_an_absorb_loop(t, k):
    """two messages of k and k + 1 blocks side by side in one column, P = 2, flat; the tag immediate enters once per message"""
    rnd = random.Random(10 * t + k)
    params = pr.make_params(t, 2, 1, 510 + t)
    P, nb = 2, 2 * k + 1
    T = P * nb + 1
    msgs = [[rnd.randrange(R) for _ in range((t - 1) * k)], [rnd.randrange(R) for _ in range((t - 1) * (k + 1))]]
    msgs[1][0], msgs[1][t - 1] = R - 1, R - 1
    cols = [[0] * T for _ in range(t)]              # col 0: start, cols 1 .. t - 1: the rate cells
    b = 0
    for m in msgs:
        cols[0][b * P] = 1 + b
        for i in range(len(m) // (t - 1)):
            for j in range(t - 1):
                cols[1 + j][(b + i) * P] = m[i * (t - 1) + j]
        b += len(m) // (t - 1)
    names = [f"out{j}" for j in range(t)] + ["in0"]
    rows, st = pc.columns(cols, params, [{"mode": "sponge", "in": [("imm", 99)] + list(range(1, t)), "start": 0, "period": P,
                                          "layout": "flat", "cols": names}])
    assert st["blocks"] == [nb] and st["segments"] == [2]
    want = absorb(params, 99, msgs[0]) + absorb(params, 99, msgs[1])
    for i, w in enumerate(want):
        assert [rows[j][i * P] for j in range(t)] == w
        assert all(rows[j][i * P + 1] == 0 for j in range(t + 1))
    assert rows[t][0] == 99 and rows[t][k * P] == 99 and rows[t][(k + 1) * P] == want[k][0]   # a continuing block keeps out_0


def build_tree(params, cap, leaves, a):
    """the levels of an a-ary tree bottom-up, leaves first: a node is out[1] of the permutation of (cap, its a children)"""
    levels = [list(leaves)]
    while len(levels[-1]) > 1:
        below = levels[-1]
        levels.append([pr.permute(params, [cap] + below[i:i + a])[1] for i in range(0, len(below), a)])
    return levels


def path_columns(levels, a, depth, P, T, first_block=0, cols=None, leaf_index=None):
    """the start, leaf, pos, sibling and expect columns of the paths of the given leaves, `depth` blocks each"""
    n_leaves = len(levels[0])
    cols = cols or [[0] * T for _ in range(4 + a - 1)]   # 0 start, 1 leaf, 2 pos, 3 expect, 4 .. siblings
    b = first_block
    for leaf in (range(n_leaves) if leaf_index is None else leaf_index):
        idx = leaf
        for lvl in range(depth):
            row = (b + lvl) * P
            group = levels[lvl][idx - idx % a:idx - idx % a + a]
            cols[0][row] = int(lvl == 0) * (R - 1)
            cols[1][row] = levels[0][leaf] if lvl == 0 else 12345          # read on a starting block only
            cols[2][row] = idx % a
            cols[3][row] = levels[-1][0] if lvl == depth - 1 else 54321    # read at a segment's last block only
            for k, sib in enumerate(group[:idx % a] + group[idx % a + 1:]):
                cols[4 + k][row] = sib
            idx //= a
        b += depth
    return cols, b


@pytest.mark.parametrize("a", [2, 4, 7])
@pytest.mark.parametrize("depth", [1, 2, 3, 4])
def test_every_leaf_of_a_tree_reaches_the_root(a, depth):
    t = a + 1
    rnd = random.Random(100 * a + depth)
    params = pr.make_params(t, 2, 1, 520 + a)
    leaves = [rnd.randrange(R) for _ in range(a ** depth)]
    levels = build_tree(params, 3, leaves, a)
    assert len(levels) == depth + 1 and len(levels[-1]) == 1
    P = 1
    chosen = list(range(len(leaves)))
    if len(chosen) > 300:                                                  # a sample: both ends and random leaves between
        chosen = sorted(set(range(2 * a)) | set(range(len(leaves) - 2 * a, len(leaves))) | set(rnd.sample(chosen, 60)))
    T = len(chosen) * depth + 2
    cols, nb = path_columns(levels, a, depth, P, T, leaf_index=chosen)
    unit = {"mode": "path", "cap": ("imm", 3), "leaf": 1, "sib": list(range(4, 4 + a - 1)), "pos": 2, "digest": 1, "start": 0,
            "period": P}
    rows, st = pc.columns(cols, params, [dict(unit, expect=3)], usable=nb)
    assert rows == [] and st == {"blocks": [nb], "segments": [len(chosen)], "bad_pos": [0], "first_bad_pos": [None],
                                 "mismatch": [0], "first_mismatch": [None]}
    assert {cols[2][r] for r in range(nb)} == set(range(a))              # every position occurs
    # the flat layout shows the digests level by level
    rows, _ = pc.columns(cols, params, [dict(unit, layout="flat", cols=["out1"])], usable=nb, tail=[0] * (T - nb))
    assert rows[0][nb - 1] == levels[-1][0] and rows[0][nb - depth] == levels[1][(len(leaves) - 1) // a]
    # one altered sibling of one path misses the root, at the row of that path's last block
    victim = rnd.randrange(len(chosen))
    lvl = rnd.randrange(depth)
    cols[4 + rnd.randrange(a - 1)][(victim * depth + lvl) * P] += 1
    _, st = pc.columns(cols, params, [dict(unit, expect=3)], usable=nb)
    assert st["mismatch"] == [1] and st["first_mismatch"] == [(victim * depth + depth - 1) * P]


@pytest.mark.parametrize("mode", ["sponge", "path"])
def test_trace_and_flat_layouts_agree(mode):
    t, full, partial = 4, 2, 2
    Rn = full + partial
    rnd = random.Random(77)
    params = pr.make_params(t, full, partial, 530)
    nb = 6
    Pt, Pf = Rn + 2, 1
    src = rand_cols(6, nb, rnd)
    src[0] = [1, 0, 0, 5, 0, 1]
    src[5] = [0, 2, 1, 2, 0, 1]
    unit = ({"mode": "sponge", "in": [1, ("imm", 4), 2, 3], "start": 0} if mode == "sponge" else
            {"mode": "path", "cap": 1, "leaf": ("imm", 8), "sib": [2, 3], "pos": 5, "digest": 2, "start": 0})
    spread = [[0] * (nb * Pt) for _ in range(6)]
    for c in range(6):
        for b in range(nb):
            spread[c][b * Pt] = src[c][b]
    names = [f"in{j}" for j in range(t)] + [f"out{j}" for j in range(t)]
    flat, fs = pc.columns(src, params, [dict(unit, period=Pf, layout="flat", cols=names)])
    tr, ts = pc.columns(spread, params, [dict(unit, period=Pt, layout="trace")])
    assert fs == ts and fs["segments"] == [3]
    for b in range(nb):
        assert [tr[j][b * Pt] for j in range(t)] == [flat[j][b] for j in range(t)]
        assert [tr[j][b * Pt + Rn] for j in range(t)] == [flat[t + j][b] for j in range(t)]
        assert all(tr[j][b * Pt + Rn + 1] == 0 for j in range(t))


def test_usable_cuts_a_block_and_zeroes_it_and_the_tail_follows():
    params = pr.make_params(3, 2, 1, 540)
    rnd = random.Random(540)
    T, P, u = 16, 4, 11
    cols = rand_cols(4, T, rnd)
    cols[0] = [0] * T
    unit = {"mode": "sponge", "in": [1, 2, 3], "start": 0, "period": P, "layout": "trace"}
    tail = [rnd.randrange(R) for _ in range(3 * (T - u))]
    rows, st = pc.columns(cols, params, [unit], u, tail)
    full, fst = pc.columns(cols, params, [unit])
    assert st["blocks"] == [2] and fst["blocks"] == [4] and st["segments"] == fst["segments"] == [1]
    for c in range(3):
        assert rows[c][:8] == full[c][:8] and rows[c][8:u] == [0] * (u - 8) and rows[c][u:] == tail[c * (T - u):(c + 1) * (T - u)]
    assert any(full[c][8] for c in range(3))
    # a check whose segment ends at the cut block compares at the last whole block
    chk = dict(unit, digest=1, expect=1)
    del chk["layout"]
    _, cst = pc.columns(cols, params, [chk], u)
    assert cst["mismatch"] == [1] and cst["first_mismatch"] == [4]


@pytest.mark.parametrize("bad", [2, 3, R - 1, (1 << 32) + 1, 1 << 64])
def test_a_bad_pos_is_position_zero_and_counted(bad):
    params = pr.make_params(3, 2, 1, 550)
    rnd = random.Random(550)
    cols = rand_cols(4, 4, rnd)
    cols[2] = [1, bad, 0, bad]
    unit = {"mode": "path", "cap": ("imm", 0), "leaf": 0, "sib": [1], "pos": 2, "digest": 1, "start": None, "period": 1,
            "layout": "flat", "cols": ["in1", "in2", "out1"]}
    rows, st = pc.columns(cols, params, [unit])
    assert st["bad_pos"] == [2] and st["first_bad_pos"] == [1] and st["segments"] == [4]
    zero = list(cols)
    zero[2] = [1, 0, 0, 0]
    assert pc.columns(zero, params, [unit])[0] == rows
    assert [rows[0][1], rows[1][1]] == [cols[0][1], cols[1][1]] and [rows[0][0], rows[1][0]] == [cols[1][0], cols[0][0]]


# ---------------------------------------------------------------------------------------------------- the encoder
P3 = pr.make_params(3, 2, 1, 11)
P2 = pr.make_params(2, 2, 1, 12)
SP = {"mode": "sponge", "in": [0, 1, 2], "start": None, "period": 4, "layout": "trace"}
PA = {"mode": "path", "cap": ("imm", 1), "leaf": 0, "sib": [1], "pos": 2, "digest": 1, "start": 3, "period": 1, "layout": "flat",
      "cols": ["out1"]}


def test_call_encoder():
    par, recs = HipEngine.poseidon_chain_call(P3, [SP, PA, dict(SP, layout=None, digest=2, expect=5, start=4),
                                                   dict(PA, layout="trace", cols=None, period=9, cap=7, leaf=("imm", "0x10"))])
    assert par == HipEngine.poseidon_call(P3, [{"mode": "row", "in": [0, 1, 2], "out": [0]}])[0]
    N, IMM, A = _native, _native.KZG_POSEIDON_IMM, _native.KZG_POSEIDON_CHAIN_ABSENT
    z = bytes(32)
    assert recs[0] == (N.KZG_POSEIDON_CHAIN_SPONGE, 0, N.KZG_POSEIDON_CHAIN_TRACE, 4, A, A, A, A, 3, [0, 1, 2, 0, 0, 0, 0, 0],
                       [0, 1, 2] + [0] * 13, [z] * 8)
    assert recs[1] == (N.KZG_POSEIDON_CHAIN_PATH, 0, N.KZG_POSEIDON_CHAIN_FLAT, 1, 3, 2, 1, A, 1, [IMM, 0, 1, 0, 0, 0, 0, 0],
                       [N.KZG_POSEIDON_CHAIN_COL_OUT + 1] + [0] * 15, [(1).to_bytes(32, "big")] + [z] * 7)
    assert recs[2][:9] == (N.KZG_POSEIDON_CHAIN_SPONGE, N.KZG_POSEIDON_CHAIN_CHECK, 0, 4, 4, A, 2, 5, 0)
    assert recs[3][:9] == (N.KZG_POSEIDON_CHAIN_PATH, 0, N.KZG_POSEIDON_CHAIN_TRACE, 9, 3, 2, 1, A, 3)
    assert recs[3][9][:3] == [7, IMM, 1] and recs[3][11][1] == (16).to_bytes(32, "big")
    st = HipEngine.poseidon_chain_unit_struct(recs[1])
    assert (st.mode, st.flags, st.layout, st.period, st.start, st.pos, st.digest, st.expect, st.n_out) == recs[1][:9]
    assert st.reserved == 0 and list(st.in_) == recs[1][9] and list(st.out) == recs[1][10]
    assert bytes(st.imm_be32[0]) == (1).to_bytes(32, "big") and bytes(st.imm_be32[1]) == z
    assert ctypes.sizeof(_native.PoseidonChainUnit) == 40 + 32 + 64 + 256
    flat = HipEngine.poseidon_chain_call(P3, [dict(SP, layout="flat", cols=["out2", "in0", "in2", "out0"])])[1][0]
    assert flat[8] == 4 and flat[10][:4] == [10, 0, 2, 8]


@pytest.mark.parametrize("params,units,why", [
    (dict(P3, t=1), [SP], "width t"), (dict(P3, t=9), [SP], "width t"), (dict(P3, full=3), [SP], "R_F must be even"),
    (dict(P3, full=18), [SP], "R_F"), (dict(P3, partial=129), [SP], "R_P"), (dict(P3, rc=P3["rc"][:-1]), [SP], "rc must be a list"),
    (dict(P3, mds=P3["mds"] + [1]), [SP], "mds must be a list"),
    (dict(P3, rc=[R] + P3["rc"][1:]), [SP], "round constant must be a canonical"),
    (dict(P3, mds=P3["mds"][:-1] + [R + 5]), [SP], "matrix entry must be a canonical"),
    (dict(P3, alpha=5), [SP], "params is a mapping"),
    (P3, [], "n_units"), (P3, [SP] * 5, "n_units"), (P3, "x", "n_units"), (P3, [5], "a unit is a mapping"),
    (P3, [dict(SP, mode="rounds")], "unknown mode"), (P3, [dict(SP, mode="row")], "unknown mode"),
    (P3, [dict(SP, foo=1)], "unknown field"), (P3, [dict(PA, foo=1)], "unknown field"),
    (P3, [dict(SP, sib=[1])], "does not take"), (P3, [dict(SP, pos=1)], "does not take"), (P3, [dict(SP, cap=1)], "does not take"),
    (P3, [dict(PA, **{"in": [0, 1, 2]})], "does not take"),
    (P2, [dict(PA, sib=[])], "t >= 3"),
    (P3, [dict(PA, sib=[1, 2])], "sib must hold"), (P3, [dict(PA, sib=[])], "sib must hold"), (P3, [dict(PA, sib=None)], "sib must hold"),
    (P3, [dict(PA, sib=[("imm", 1)])], "not an immediate"), (P3, [dict(PA, pos=("imm", 1))], "not an immediate"),
    (P3, [dict(PA, start=("imm", 1))], "not an immediate"), (P3, [dict(SP, start=("imm", 0))], "not an immediate"),
    (P3, [dict(PA, pos=None)], "pos must be a row"), (P3, [dict(PA, pos=-1)], "pos must be a row"),
    (P3, [{k: v for k, v in PA.items() if k != "leaf"}], "needs cap and leaf"),
    (P3, [dict(PA, digest=3)], "digest must be"), (P3, [dict(PA, digest=None)], "needs digest"),
    (P3, [dict(SP, digest=1)], "digest belongs"), (P3, [dict(SP, layout=None, expect=3)], "expect needs digest"),
    (P3, [dict(SP, period=3)], "at least R + 1"), (P3, [dict(PA, layout="trace", cols=None, period=3)], "at least R + 1"),
    (P3, [dict(SP, period=0)], "period P"), (P3, [dict(SP, period=1 << 32)], "period P"), (P3, [dict(SP, period=None)], "period P"),
    (P3, [dict(PA, period=0)], "period P"),
    (P3, [dict(SP, layout="wide")], "unknown layout"), (P3, [dict(SP, layout=None)], "unknown layout"),
    (P3, [dict(SP, cols=["in0"])], "cols belongs"),
    (P3, [dict(PA, cols=["out3"])], "unknown column name"), (P3, [dict(PA, cols=["in"])], "unknown column name"),
    (P3, [dict(PA, cols=["out1", "out1"])], "repeated"), (P3, [dict(PA, cols=[])], "cols must hold"),
    (P3, [dict(PA, cols=None)], "cols must hold"),
    (P3, [dict(SP, digest=1, expect=3)], "refused beside expect"), (P3, [dict(PA, expect=3)], "refused beside expect"),
    (P3, [dict(PA, layout=None, cols=None, expect=("imm", 3))], "not an immediate"),
    (P3, [dict(SP, **{"in": [0, 1]})], "in must hold t"), (P3, [dict(SP, **{"in": [0, 1, -1]})], "entry of in"),
    (P3, [dict(SP, **{"in": [0, 1, ("im", 1)]})], "immediate is"),
    (P3, [dict(SP, **{"in": [0, 1, ("imm", R)]})], "immediate must be a canonical"), (P3, [dict(PA, cap=("imm", R))], "canonical"),
    (P3, [dict(SP, **{"in": [5 * k, 5 * k + 1, 5 * k + 2]}, start=5 * k + 3) for k in range(4)], None),
    (P3, [dict(SP, **{"in": [5 * k, 5 * k + 1, 5 * k + 2]}, start=5 * k + 3) for k in range(3)] +
     [dict(PA, leaf=15, sib=[16], pos=17, start=18, cap=19)], "distinct input rows"),
    (P3, [dict(SP, layout="flat", cols=["in0", "in1", "in2", "out0", "out1", "out2"])] * 3, "n_out"),
    (P3, [SP] * 4 + [], None), (pr.make_params(5, 2, 1, 13), [dict(SP, **{"in": [0] * 5})] * 4, "n_out"),
])
def test_python_refusals(params, units, why):
    if why is None:   # 16 distinct rows, and 12 output rows: both inside the limits
        par, recs = HipEngine.poseidon_chain_call(params, units)
        assert len(recs) == 4
        return
    with pytest.raises(KzgError) as ei:
        HipEngine.poseidon_chain_call(params, units)
    assert ei.value.code == _native.KZG_E_ARG and "poseidon_chain: " in str(ei.value) and why in str(ei.value), str(ei.value)


def test_header_constants_and_symbols():
    text = open(HEADER).read()
    for name in ("KZG_POSEIDON_CHAIN_SPONGE", "KZG_POSEIDON_CHAIN_PATH", "KZG_POSEIDON_CHAIN_CHECK", "KZG_POSEIDON_CHAIN_TRACE",
                 "KZG_POSEIDON_CHAIN_FLAT", "KZG_POSEIDON_CHAIN_ABSENT", "KZG_POSEIDON_CHAIN_COL_IN", "KZG_POSEIDON_CHAIN_COL_OUT",
                 "KZG_POSEIDON_CHAIN_MAX_UNITS"):
        m = re.search(r"#define\s+%s\s+(0x[0-9a-fA-F]+|\d+)" % name, text)
        assert m and int(m.group(1), 0) == getattr(_native, name), name
    assert _native.KZG_POSEIDON_CHAIN_MAX_UNITS == pc.MAX_UNITS and _native.KZG_POSEIDON_CHAIN_COL_OUT == _native.KZG_POSEIDON_MAX_T
    assert _native.KZG_POSEIDON_CHAIN_ABSENT == _native.KZG_POSEIDON_IMM
    for sym in ("kzg_rows_commit_poseidon_chain", "kzg_multi_rows_commit_poseidon_chain"):
        assert sym in _native.SYMBOLS and re.search(r"\bint %s\(" % sym, text)
    assert len(_native.SYMBOLS["kzg_multi_rows_commit_poseidon_chain"][1]) == \
        len(_native.SYMBOLS["kzg_rows_commit_poseidon_chain"][1]) + 1
    body = re.search(r"typedef struct kzg_poseidon_chain_unit \{(.*?)\} kzg_poseidon_chain_unit;", text, re.S).group(1)
    fields = re.findall(r"^\s*uint(?:32|8)_t\s+(\w+)", body, re.M)
    assert [("in_" if f == "in" else f) for f in fields] == [f[0] for f in _native.PoseidonChainUnit._fields_]
    # the scope note of kzg_rows_commit_poseidon keeps its words and points here; this call names its own limits
    for word in ("generating constants (the Grain LFSR)", "the inverse S-box", "the optimised partial-round form", "sponge chaining",
                 "Poseidon2", "kzg_rows_commit_poseidon_chain, below", "t cooperating lanes per segment", "arity-8 trees",
                 "padding and domain-tag conventions", "building whole trees level", "a carry across calls", "SEGMENT IS SERIAL"):
        assert word in text, word
    from zkp_subnet_amd import Client, MultiDeviceClient
    assert callable(Client.worker_commit_poseidon_chain) and callable(MultiDeviceClient.worker_commit_poseidon_chain)
    assert callable(HipEngine.commit_poseidon_chain)
