"""CPU tests of the six unit encoders' refusals: HipEngine.poseidon_call, poseidon_chain_call, sha256_call, keccak_call, ec_call
and edwards_call (and the params body the two Poseidon encoders share).  The other CPU modules pin substrings; this one pins
every message WHOLE, one case at least per place where an encoder refuses, and the order of two refusals where one call has two
faults.  The texts were recorded from the encoders as they stood before their field parsers were folded into one set; the
table must not be edited to fit the code.  Needs no device."""
import pytest

from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError
from zkp_subnet_amd.engine import HipEngine

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
DEL = object()   # a field taken out of the base


def W(base, **ch):
    """the mapping `base` with the fields of ch replaced (in_ stands for in), a DEL one removed"""
    d = dict(base)
    for k, v in ch.items():
        k = "in" if k == "in_" else k
        if v is DEL:
            d.pop(k, None)
        else:
            d[k] = v
    return d


def PAR(t=2, **ch):
    return W({"t": t, "full": 2, "partial": 0, "rc": [1] * (2 * t), "mds": [1] * (t * t)}, **ch)


IMM0 = ("imm", 0)
# poseidon
PROW = {"mode": "row", "in": [0, ("imm", 5)], "out": [0]}
PRND = {"mode": "rounds", "in": [0, 1], "period": 3}
# poseidon_chain (PATH under t = 3)
SP = {"mode": "sponge", "in": [0, ("imm", 1)], "start": None, "period": 1, "layout": "flat", "cols": ["out0"]}
PATH = {"mode": "path", "cap": IMM0, "leaf": 0, "sib": [1], "pos": 2, "digest": 0, "start": None, "period": 1,
        "layout": "flat", "cols": ["out0"]}
# sha256
SROW = {"mode": "row", "state": "iv", "msg": [IMM0] * 15 + [0], "out": [0]}
SRND = {"mode": "rounds", "msg": 0, "start": None, "period": 72, "iv": None, "cols": ["w"]}
# keccak
KROW = {"mode": "row", "in": [IMM0] * 24 + [0], "out": [0]}
KRND = {"mode": "rounds", "msg": [0, 1, 2, 3, 4], "rate": 17, "start": None, "period": 125, "cols": ["a0"]}
# ec
CV = {"bits": 8, "limbs": 1, "p": 251, "a": 1}
DIV = {"mode": "div", "a": 0, "b": 1, "out": True}
EADD = {"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "out": ["lam"]}
ECH = {"mode": "chain", "px": 0, "py": 1, "op": 2, "cols": ["ax"]}
# edwards
ED = {"a": 2, "d": 3}
DADD = {"mode": "add", "x1": 0, "y1": 1, "x2": 2, "y2": 3, "out": ["x3"]}
DCH = {"mode": "chain", "px": 0, "py": 1, "op": 2, "cols": ["ax"]}

pos = lambda params, units: ("poseidon_call", (params, units))                 # noqa: E731
pch = lambda params, units: ("poseidon_chain_call", (params, units))           # noqa: E731
sha = lambda units: ("sha256_call", (units,))                                  # noqa: E731
kec = lambda units: ("keccak_call", (units,))                                  # noqa: E731
ec = lambda curve, units, *n: ("ec_call", (curve, units, "commit_ec") + n)      # noqa: E731
edw = lambda curve, units, *n: ("edwards_call", (curve, units, "commit_edwards") + n)   # noqa: E731

# (encoder and arguments, the whole message)
CASES = [
    # ---- the params of both Poseidon encoders
    (pos(PAR(rc=[bytes(31), 1, 1, 1]), [PROW]), "commit_poseidon: poseidon: a round constant given as bytes must be of 32 bytes"),
    (pos(PAR(rc=["zz", 1, 1, 1]), [PROW]),
     "commit_poseidon: poseidon: a round constant must be an integer, a decimal or 0x string, or 32 bytes"),
    (pos(PAR(rc=[-1, 1, 1, 1]), [PROW]), "commit_poseidon: poseidon: a round constant must be a non-negative integer"),
    (pos(PAR(mds=[R, 1, 1, 1]), [PROW]), "commit_poseidon: poseidon: a matrix entry must be a canonical scalar (< r)"),
    (pos({}, [PROW]), "commit_poseidon: poseidon: params is a mapping with exactly t, full, partial, rc, mds"),
    (pos(PAR(t=1), [PROW]), "commit_poseidon: poseidon: the width t must be an integer in [2, 8]"),
    (pos(PAR(full=3), [PROW]), "commit_poseidon: poseidon: the number of full rounds R_F must be even and in [2, 16]"),
    (pos(PAR(partial=129), [PROW]), "commit_poseidon: poseidon: the number of partial rounds R_P must be in [0, 128]"),
    (pos(PAR(rc=[1]), [PROW]), "commit_poseidon: poseidon: rc must be a list of t (R_F + R_P) = 4 scalars, round-major"),
    (pos(PAR(mds=[1]), [PROW]), "commit_poseidon: poseidon: mds must be a list of t t = 4 scalars, row-major"),
    (pch(PAR(t=True), [SP]), "commit_poseidon_chain: poseidon_chain: the width t must be an integer in [2, 8]"),
    # ---- poseidon
    (pos(PAR(), []), "commit_poseidon: poseidon: units must be a list of 1 .. 8 entries (n_units)"),
    (pos(PAR(), [PROW] * 9), "commit_poseidon: poseidon: units must be a list of 1 .. 8 entries (n_units)"),
    (pos(PAR(), [5]), "commit_poseidon: poseidon: a unit is a mapping with mode, in and the fields of its mode"),
    (pos(PAR(), [W(PROW, zz=1)]), "commit_poseidon: poseidon: unknown field 'zz' (the fields are mode, in, out, expect, period)"),
    (pos(PAR(), [W(PROW, mode="x")]), "commit_poseidon: poseidon: unknown mode 'x' (one of \"row\", \"rounds\")"),
    (pos(PAR(), [W(PROW, in_=[0])]), "commit_poseidon: poseidon: in must hold t = 2 entries, each a row index or (\"imm\", value)"),
    (pos(PAR(), [W(PROW, in_=[0, ("imm",)])]), "commit_poseidon: poseidon: an immediate is (\"imm\", value)"),
    (pos(PAR(), [W(PROW, in_=[0, ("imm", R)])]), "commit_poseidon: poseidon: an immediate must be a canonical scalar (< r)"),
    (pos(PAR(), [W(PROW, in_=[0, -1])]),
     "commit_poseidon: poseidon: an entry of in must be a row index, an integer in [0, 2^32 - 1), or (\"imm\", value)"),
    (pos(PAR(), [W(PRND, expect=[0])]), "commit_poseidon: poseidon: expect belongs to row units, not to rounds"),
    (pos(PAR(), [W(PRND, out=[0])]), "commit_poseidon: poseidon: out belongs to row units: a rounds unit commits all t columns"),
    (pos(PAR(), [W(PRND, period=2)]),
     "commit_poseidon: poseidon: the period P of a rounds unit must be an integer in [R + 1, 2^32), R + 1 = 3"),
    (pos(PAR(), [W(PROW, period=3)]), "commit_poseidon: poseidon: period belongs to rounds units, not to row"),
    (pos(PAR(), [W(PROW, out=[])]), "commit_poseidon: poseidon: out must hold 1 .. t = 2 state indices"),
    (pos(PAR(), [W(PROW, out=[2])]), "commit_poseidon: poseidon: an out index must be an integer below t = 2"),
    (pos(PAR(), [W(PROW, out=[0, 0])]), "commit_poseidon: poseidon: an out index is repeated"),
    (pos(PAR(), [W(PROW, expect=[0, 1])]), "commit_poseidon: poseidon: expect must hold one row per entry of out"),
    (pos(PAR(), [W(PROW, expect=[-1])]),
     "commit_poseidon: poseidon: an entry of expect must be a row index, an integer in [0, 2^32 - 1)"),
    (pos(PAR(), [W(PROW, in_=[4 * u, 4 * u + 1], out=[0, 1], expect=[4 * u + 2, 4 * u + 3]) for u in range(5)]),
     "commit_poseidon: poseidon: the units read 20 distinct input rows, at most 16 fit one call"),
    (pos(PAR(3), [W(PROW, in_=[0, 0, 0], out=[0, 1, 2])] * 8),
     "commit_poseidon: poseidon: n_out: the units give 24 output rows, at most 16 fit one call"),
    # ---- poseidon_chain
    (pch(PAR(), [SP] * 5), "commit_poseidon_chain: poseidon_chain: units must be a list of 1 .. 4 entries (n_units)"),
    (pch(PAR(3), [W(PATH, sib=[("imm", 1)])]),
     "commit_poseidon_chain: poseidon_chain: an entry of sib must be a row, not an immediate"),
    (pch(PAR(3), [W(PATH, pos=-1)]), "commit_poseidon_chain: poseidon_chain: pos must be a row index, an integer in [0, 2^32 - 1)"),
    (pch(PAR(), [W(SP, start=True)]), "commit_poseidon_chain: poseidon_chain: start must be a row index, an integer in [0, 2^32 - 1)"),
    (pch(PAR(3), [W(PATH, cap=("imm", 1, 2))]), "commit_poseidon_chain: poseidon_chain: an immediate is (\"imm\", value)"),
    (pch(PAR(3), [W(PATH, leaf=None)]),
     "commit_poseidon_chain: poseidon_chain: leaf must be a row index, an integer in [0, 2^32 - 1), or (\"imm\", value)"),
    (pch(PAR(), [W(SP, in_=[0, 2**32 - 1])]),
     "commit_poseidon_chain: poseidon_chain: an entry of in must be a row index, an integer in [0, 2^32 - 1), or (\"imm\", value)"),
    (pch(PAR(), [[]]), "commit_poseidon_chain: poseidon_chain: a unit is a mapping with mode and the fields of its mode"),
    (pch(PAR(), [W(SP, mode="row")]), "commit_poseidon_chain: poseidon_chain: unknown mode 'row' (one of \"sponge\", \"path\")"),
    (pch(PAR(), [W(SP, cap=0)]),
     "commit_poseidon_chain: poseidon_chain: a field the mode does not take: 'cap' does not belong to a sponge unit"),
    (pch(PAR(), [W(SP, zz=0)]),
     "commit_poseidon_chain: poseidon_chain: unknown field 'zz' (the fields of a sponge unit are mode, in, start, period, layout, "
     "cols, digest, expect)"),
    (pch(PAR(), [W(SP, in_=0)]),
     "commit_poseidon_chain: poseidon_chain: in must hold t = 2 entries, each a row index or (\"imm\", value)"),
    (pch(PAR(), [PATH]), "commit_poseidon_chain: poseidon_chain: a path unit needs t >= 3: the arity is t - 1"),
    (pch(PAR(3), [W(PATH, cap=DEL)]),
     "commit_poseidon_chain: poseidon_chain: a path unit needs cap and leaf, each a row index or (\"imm\", value)"),
    (pch(PAR(3), [W(PATH, sib=[1, 2])]), "commit_poseidon_chain: poseidon_chain: sib must hold t - 2 = 1 rows"),
    (pch(PAR(), [W(SP, period=0)]), "commit_poseidon_chain: poseidon_chain: the period P must be an integer in [1, 2^32)"),
    (pch(PAR(3), [W(PATH, digest=3)]), "commit_poseidon_chain: poseidon_chain: digest must be a state index below t = 3"),
    (pch(PAR(), [W(SP, expect=1, digest=0)]),
     "commit_poseidon_chain: poseidon_chain: layout and cols are refused beside expect: a check commits nothing"),
    (pch(PAR(), [W(SP, expect=1, layout=DEL, cols=DEL)]),
     "commit_poseidon_chain: poseidon_chain: expect needs digest, the state index that is compared"),
    (pch(PAR(), [W(SP, expect=("imm", 1), digest=0, layout=DEL, cols=DEL)]),
     "commit_poseidon_chain: poseidon_chain: expect must be a row, not an immediate"),
    (pch(PAR(3), [W(PATH, digest=DEL)]),
     "commit_poseidon_chain: poseidon_chain: a path unit needs digest, the state index that a continuing block hashes"),
    (pch(PAR(), [W(SP, digest=0)]), "commit_poseidon_chain: poseidon_chain: digest belongs to path units and to checks (expect)"),
    (pch(PAR(), [W(SP, layout="wide")]), "commit_poseidon_chain: poseidon_chain: unknown layout 'wide' (one of \"trace\", \"flat\")"),
    (pch(PAR(), [W(SP, layout="trace", period=3)]),
     "commit_poseidon_chain: poseidon_chain: cols belongs to the flat layout: a trace commits all t columns"),
    (pch(PAR(), [W(SP, layout="trace", cols=DEL, period=2)]),
     "commit_poseidon_chain: poseidon_chain: the period P of a trace must be at least R + 1 = 3"),
    (pch(PAR(), [W(SP, cols=[])]),
     "commit_poseidon_chain: poseidon_chain: cols must hold 1 .. 2 t = 4 column names among in0, in1, out0, out1"),
    (pch(PAR(), [W(SP, cols=["out2"])]),
     "commit_poseidon_chain: poseidon_chain: unknown column name 'out2' (the names are in0, in1, out0, out1)"),
    (pch(PAR(), [W(SP, cols=["in0", "in0"])]), "commit_poseidon_chain: poseidon_chain: a column name is repeated"),
    (pch(PAR(8), [W(SP, in_=list(range(8 * u, 8 * u + 8))) for u in range(3)]),
     "commit_poseidon_chain: poseidon_chain: the units read 24 distinct input rows, at most 16 fit one call"),
    (pch(PAR(8), [W(SP, in_=[0] * 8, layout="trace", cols=DEL, period=3)] * 3),
     "commit_poseidon_chain: poseidon_chain: n_out: the units give 24 output rows, at most 16 fit one call"),
    # ---- sha256
    (sha(()), "commit_sha256: sha256: units must be a list of 1 .. 4 entries (n_units)"),
    (sha([W(SROW, msg=[0])]), "commit_sha256: sha256: msg must hold 16 slots, each a row index or (\"imm\", value)"),
    (sha([W(SROW, state=[0])]),
     "commit_sha256: sha256: state (\"iv\", or a list) must hold 8 slots, each a row index or (\"imm\", value)"),
    (sha([W(SROW, msg=[("im", 0)] + [0] * 15)]), "commit_sha256: sha256: an immediate is (\"imm\", value)"),
    (sha([W(SROW, msg=[("imm", 2**32)] + [0] * 15)]), "commit_sha256: sha256: an immediate must be an integer below 2^32"),
    (sha([W(SROW, msg=["0"] + [0] * 15)]),
     "commit_sha256: sha256: a slot must be a row index, an integer in [0, 2^32 - 1), or (\"imm\", value)"),
    (sha([None]), "commit_sha256: sha256: a unit is a mapping with mode and the fields of its mode"),
    (sha([W(SROW, mode=0)]), "commit_sha256: sha256: unknown mode 0 (one of \"row\", \"rounds\")"),
    (sha([W(SRND, expect=[0])]), "commit_sha256: sha256: expect belongs to row units, not to rounds"),
    (sha([W(SRND, out=[0])]),
     "commit_sha256: sha256: unknown field 'out' (the fields of a rounds unit are mode, msg, start, period, iv, cols)"),
    (sha([W(SROW, period=72)]),
     "commit_sha256: sha256: unknown field 'period' (the fields of a row unit are mode, state, msg, out, expect)"),
    (sha([W(SROW, out=list(range(9)))]), "commit_sha256: sha256: out must hold 1 .. 8 word indices"),
    (sha([W(SROW, out=[8])]), "commit_sha256: sha256: an out index must be an integer below 8"),
    (sha([W(SROW, out=[1, 1])]), "commit_sha256: sha256: an out index is repeated"),
    (sha([W(SROW, expect=[])]), "commit_sha256: sha256: expect must hold one row per entry of out"),
    (sha([W(SROW, expect=[2**32 - 1])]),
     "commit_sha256: sha256: an entry of expect must be a row index, an integer in [0, 2^32 - 1)"),
    (sha([W(SRND, msg=IMM0)]), "commit_sha256: sha256: the msg of a rounds unit must be a row index, an integer in [0, 2^32 - 1)"),
    (sha([W(SRND, start=-1)]), "commit_sha256: sha256: start must be a row index, an integer in [0, 2^32 - 1), or None"),
    (sha([W(SRND, period=71)]), "commit_sha256: sha256: the period P of a rounds unit must be an integer in [72, 2^32)"),
    (sha([W(SRND, iv=[0] * 7)]), "commit_sha256: sha256: iv must be None or 8 words, integers below 2^32"),
    (sha([W(SRND, cols=[])]), "commit_sha256: sha256: cols must hold 1 .. 12 column names"),
    (sha([W(SRND, cols=["x"])]),
     "commit_sha256: sha256: unknown column name 'x' (the names are w, a, e, cw, ca, ce, sig0, sig1, sum0, maj, sum1, ch)"),
    (sha([W(SRND, cols=["w", "w"])]), "commit_sha256: sha256: a column name is repeated"),
    (sha([W(SROW, state=list(range(16, 24)), msg=list(range(16)))]),
     "commit_sha256: sha256: the units read 24 distinct input rows, at most 16 fit one call"),
    (sha([W(SRND, cols=list(_native.KZG_SHA256_COLS))] * 2),
     "commit_sha256: sha256: n_out: the units give 24 output rows, at most 16 fit one call"),
    # ---- keccak
    (kec(None), "commit_keccak: keccak: units must be a list of 1 .. 4 entries (n_units)"),
    (kec([0]), "commit_keccak: keccak: a unit is a mapping with mode and the fields of its mode"),
    (kec([W(KROW, mode="chain")]), "commit_keccak: keccak: unknown mode 'chain' (one of \"row\", \"rounds\")"),
    (kec([W(KRND, expect=[0])]), "commit_keccak: keccak: expect belongs to row units, not to rounds"),
    (kec([W(KROW, rate=1)]), "commit_keccak: keccak: unknown field 'rate' (the fields of a row unit are mode, in, out, expect)"),
    (kec([W(KROW, in_=[0] * 24)]), "commit_keccak: keccak: in must hold 25 slots, each a row index or (\"imm\", value)"),
    (kec([W(KROW, in_=[()] + [0] * 24)]), "commit_keccak: keccak: an immediate is (\"imm\", value)"),
    (kec([W(KROW, in_=[("imm", 2**64)] + [0] * 24)]), "commit_keccak: keccak: an immediate must be an integer below 2^64"),
    (kec([W(KROW, in_=[None] + [0] * 24)]),
     "commit_keccak: keccak: a slot must be a row index, an integer in [0, 2^32 - 1), or (\"imm\", value)"),
    (kec([W(KROW, out=list(range(17)))]), "commit_keccak: keccak: out must hold 1 .. 16 lane indices (n_out)"),
    (kec([W(KROW, out=[25])]), "commit_keccak: keccak: a lane index must be an integer below 25"),
    (kec([W(KROW, out=[3, 3])]), "commit_keccak: keccak: a lane index is repeated"),
    (kec([W(KROW, expect=[0, 1])]), "commit_keccak: keccak: expect must hold one row per entry of out"),
    (kec([W(KROW, expect=[True])]), "commit_keccak: keccak: an entry of expect must be a row index, an integer in [0, 2^32 - 1)"),
    (kec([W(KRND, msg=[0, 1, 2, 3])]),
     "commit_keccak: keccak: the msg of a rounds unit must hold 5 row indices, integers in [0, 2^32 - 1)"),
    (kec([W(KRND, rate=25)]), "commit_keccak: keccak: the rate of a rounds unit must be an integer in [1, 24] lanes"),
    (kec([W(KRND, start=IMM0)]), "commit_keccak: keccak: start must be a row index, an integer in [0, 2^32 - 1), or None"),
    (kec([W(KRND, period=124)]), "commit_keccak: keccak: the period P of a rounds unit must be an integer in [125, 2^32)"),
    (kec([W(KRND, cols=list(_native.KZG_KECCAK_COLS[:17]))]), "commit_keccak: keccak: cols must hold 1 .. 16 column names (n_out)"),
    (kec([W(KRND, cols=["a5"])]),
     "commit_keccak: keccak: unknown column name 'a5' (the names are a0, a1, a2, a3, a4, p0, p1, p2, p3, p4, d0, d1, d2, d3, d4, t0, "
     "t1, t2, t3, t4, b0, b1, b2, b3, b4)"),
    (kec([W(KRND, cols=["b4", "b4"])]), "commit_keccak: keccak: a column name is repeated"),
    (kec([W(KROW, in_=list(range(25)))]), "commit_keccak: keccak: the units read 25 distinct input rows, at most 16 fit one call"),
    (kec([W(KRND, cols=list(_native.KZG_KECCAK_COLS[:16]))] * 2),
     "commit_keccak: keccak: n_out: the units give 32 output rows, at most 16 fit one call"),
    # ---- ec
    (ec(W(CV, p="q"), [DIV]), "commit_ec: ec: the modulus p must be an integer, or a decimal or 0x string"),
    (ec(W(CV, a=-1), [DIV]), "commit_ec: ec: the coefficient a must be a non-negative integer"),
    (ec(None, [DIV]), "commit_ec: ec: the curve is a mapping with bits, limbs, p and a"),
    (ec(W(CV, c=0), [DIV]), "commit_ec: ec: unknown field 'c' of the curve (the fields are bits, limbs, p, a)"),
    (ec(W(CV, bits=65), [DIV]), "commit_ec: ec: the limb width b (bits) must be an integer in [1, 64]"),
    (ec(W(CV, limbs=5), [DIV]), "commit_ec: ec: the number of limbs L (limbs) must be an integer in [1, 4]"),
    (ec(W(CV, bits=64, limbs=4, p=DEL), [DIV]), "commit_ec: ec: the curve must give the modulus p and the coefficient a"),
    (ec(W(CV, p=250), [DIV]), "commit_ec: ec: the modulus p must be odd and at least 3"),
    (ec(W(CV, p=257), [DIV]), "commit_ec: ec: the modulus p must be below 2^W"),
    (ec(W(CV, a=251), [DIV]), "commit_ec: ec: the coefficient a must be below p"),
    (ec(CV, []), "commit_ec: ec: units must be a list of 1 .. 4 entries (n_units)"),
    (ec(CV, [W(DIV, a=None)]), "commit_ec: ec: a must be a first row, an integer in [0, 2^32 - 1)"),
    (ec(CV, [DIV], 1), "commit_ec: ec: the operand run of b reaches beyond the 1 concatenated rows of the input sets"),
    (ec(CV, [()]), "commit_ec: ec: a unit is a mapping with mode and the fields of its mode"),
    (ec(CV, [W(DIV, mode=["div"])]), "commit_ec: ec: unknown mode ['div'] (one of \"div\", \"add\", \"chain\")"),
    (ec(CV, [W(ECH, expect=[0])]), "commit_ec: ec: expect belongs to div and add units, not to chain"),
    (ec(CV, [W(DIV, x1=0)]), "commit_ec: ec: unknown field 'x1' (the fields of a div unit are mode, a, b, out, expect)"),
    (ec(CV, [W(ECH, cols=[])]), "commit_ec: ec: cols must hold 1 .. 3 column names among ax, ay, lam"),
    (ec(CV, [W(DIV, b=("imm",))]), "commit_ec: ec: an immediate is (\"imm\", value)"),
    (ec(CV, [W(DIV, b=("imm", "k"))]), "commit_ec: ec: an immediate must be an integer, or a decimal or 0x string"),
    (ec(CV, [W(DIV, b=("imm", 256))]), "commit_ec: ec: the immediate must be below 2^W"),
    (ec(CV, [W(DIV, expect=[2])]), "commit_ec: ec: out together with expect: a unit commits, or it is a check"),
    (ec(CV, [W(EADD, out=DEL)]), "commit_ec: ec: a unit needs out, or expect for a check"),
    (ec(CV, [W(EADD, out=DEL, expect=[4])]),
     "commit_ec: ec: a wrong number of expect rows: one first row for div, three entries (lam, x3, y3; None: not compared) for add"),
    (ec(CV, [W(EADD, out=DEL, expect=[None] * 3)]), "commit_ec: ec: expect must name at least one first row"),
    (ec(CV, [W(EADD, out=DEL, expect=[None, -1, None])]),
     "commit_ec: ec: an entry of expect must be a first row, an integer in [0, 2^32 - 1)"),
    (ec(CV, [W(DIV, out=1)]), "commit_ec: ec: the out of a div unit is True"),
    (ec(CV, [W(EADD, out="lam")]), "commit_ec: ec: out must hold 1 .. 3 names among lam, x3, y3"),
    (ec(CV, [W(EADD, out=["ax"])]), "commit_ec: ec: unknown name 'ax' (the names of a add unit are lam, x3, y3)"),
    (ec(CV, [W(ECH, cols=["ay", "ay"])]), "commit_ec: ec: a name is repeated"),
    (ec(W(CV, limbs=4), [W(EADD, x1=0, y1=4, x2=8, y2=12), W(DIV, a=16, b=IMM0)]),
     "commit_ec: ec: the units read 20 distinct input rows, at most 16 fit one call"),
    (ec(W(CV, limbs=4), [W(EADD, x1=0, y1=4, x2=8, y2=12, out=["lam", "x3", "y3"])] * 2),
     "commit_ec: ec: n_out: the units give 24 output rows, at most 16 fit one call"),
    # ---- edwards
    (edw(W(ED, a=bytes(33)), [DADD]), "commit_edwards: edwards: the coefficient A given as bytes must be of 32 bytes"),
    (edw(W(ED, d="0y"), [DADD]), "commit_edwards: edwards: the coefficient D must be an integer, a decimal or 0x string, or 32 bytes"),
    (edw(W(ED, a=1.5), [DADD]), "commit_edwards: edwards: the coefficient A must be a non-negative integer"),
    (edw(W(ED, d=R), [DADD]), "commit_edwards: edwards: the coefficient D must be a canonical scalar (< r)"),
    (edw({"a": 2}, [DADD]), "commit_edwards: edwards: the curve is a mapping with exactly a and d"),
    (edw(W(ED, d="0x0"), [DADD]), "commit_edwards: edwards: the coefficients A and D must not be 0"),
    (edw(W(ED, d=bytes(31) + b"\x02"), [DADD]), "commit_edwards: edwards: the coefficients A and D must differ"),
    (edw(ED, [DADD] * 5), "commit_edwards: edwards: units must be a list of 1 .. 4 entries (n_units)"),
    (edw(ED, [W(DCH, op=2**32 - 2)]), "commit_edwards: edwards: op must be a row, an integer in [0, 2^32 - 2)"),
    (edw(ED, [DADD], 3), "commit_edwards: edwards: y2 reaches beyond the 3 concatenated rows of the input sets"),
    (edw(ED, [W(DADD, x1=("imm", 1, 1))]), "commit_edwards: edwards: an immediate is (\"imm\", value)"),
    (edw(ED, [W(DADD, x1=("imm", R))]), "commit_edwards: edwards: an immediate must be a canonical scalar (< r)"),
    (edw(ED, [W(DCH, px=DEL)]), "commit_edwards: edwards: px must be a row index, an integer in [0, 2^32 - 2), or (\"imm\", value)"),
    (edw(ED, [W(DADD, y1=-2)]), "commit_edwards: edwards: y1 must be a row, an integer in [0, 2^32 - 2)"),
    (edw(ED, ["add"]), "commit_edwards: edwards: a unit is a mapping with mode and the fields of its mode"),
    (edw(ED, [W(DADD, mode="div")]), "commit_edwards: edwards: unknown mode 'div' (one of \"add\", \"chain\")"),
    (edw(ED, [W(DCH, expect=[0, None])]), "commit_edwards: edwards: expect belongs to add units, not to chain: a chain is never a check"),
    (edw(ED, [W(DCH, out=["x3"])]), "commit_edwards: edwards: unknown field 'out' (the fields of a chain unit are mode, px, py, op, cols)"),
    (edw(ED, [W(DCH, cols=())]), "commit_edwards: edwards: cols must hold 1 .. 2 column names among ax, ay"),
    (edw(ED, [W(DADD, expect=[4, 5])]), "commit_edwards: edwards: out together with expect: a unit commits, or it is a check"),
    (edw(ED, [W(DADD, out=None)]), "commit_edwards: edwards: a unit needs out, or expect for a check"),
    (edw(ED, [W(DADD, out=DEL, expect=[4])]), "commit_edwards: edwards: expect must hold two entries (x3, y3; None: not compared)"),
    (edw(ED, [W(DADD, out=DEL, expect=[None, None])]), "commit_edwards: edwards: expect must name at least one row"),
    (edw(ED, [W(DADD, out=DEL, expect=[None, "4"])]), "commit_edwards: edwards: an entry of expect must be a row, an integer in [0, 2^32 - 2)"),
    (edw(ED, [W(DADD, out=[])]), "commit_edwards: edwards: out must hold 1 .. 2 names among x3, y3"),
    (edw(ED, [W(DADD, out=["ax"])]), "commit_edwards: edwards: unknown name 'ax' (the names of a add unit are x3, y3)"),
    (edw(ED, [W(DADD, out=["y3", "y3"])]), "commit_edwards: edwards: a name is repeated"),
    (edw(ED, [W(DADD, x1=6 * u, y1=6 * u + 1, x2=6 * u + 2, y2=6 * u + 3, out=DEL, expect=[6 * u + 4, 6 * u + 5]) for u in range(3)]),
     "commit_edwards: edwards: the units read 18 distinct input rows, at most 16 fit one call"),
    # ---- one call with two faults: the first refusal wins
    (pos(PAR(t=9), []), "commit_poseidon: poseidon: the width t must be an integer in [2, 8]"),
    (pos(PAR(mds=[R] * 4, rc=[R] * 4), [PROW]), "commit_poseidon: poseidon: a round constant must be a canonical scalar (< r)"),
    (pos(PAR(), [W(PROW, mode="x", zz=1)]), "commit_poseidon: poseidon: unknown field 'zz' (the fields are mode, in, out, expect, period)"),
    (pos(PAR(), [W(PROW, out=[2]), W(PROW, mode="x")]), "commit_poseidon: poseidon: an out index must be an integer below t = 2"),
    (pos(PAR(), [W(PROW, in_=[0, -1], out=[])]),
     "commit_poseidon: poseidon: an entry of in must be a row index, an integer in [0, 2^32 - 1), or (\"imm\", value)"),
    (pos(PAR(8), [W(PROW, in_=list(range(8 * u, 8 * u + 8)), out=list(range(8))) for u in range(3)]),
     "commit_poseidon: poseidon: the units read 24 distinct input rows, at most 16 fit one call"),
    (pch(PAR(), [W(SP, mode="x", zz=1)]), "commit_poseidon_chain: poseidon_chain: unknown mode 'x' (one of \"sponge\", \"path\")"),
    (pch(PAR(), [W(SP, in_=[0, None], period=0)]),
     "commit_poseidon_chain: poseidon_chain: an entry of in must be a row index, an integer in [0, 2^32 - 1), or (\"imm\", value)"),
    (pch(PAR(3), [W(PATH, pos=None, start=("imm", 0))]),
     "commit_poseidon_chain: poseidon_chain: pos must be a row index, an integer in [0, 2^32 - 1)"),
    (sha([W(SROW, state=[0], msg=[0])]),
     "commit_sha256: sha256: state (\"iv\", or a list) must hold 8 slots, each a row index or (\"imm\", value)"),
    (sha([W(SROW, msg=[0], out=[])]), "commit_sha256: sha256: msg must hold 16 slots, each a row index or (\"imm\", value)"),
    (sha([W(SRND, msg=-1, period=0, cols=[])]),
     "commit_sha256: sha256: the msg of a rounds unit must be a row index, an integer in [0, 2^32 - 1)"),
    (sha([W(SRND, iv=[], cols=[])]), "commit_sha256: sha256: iv must be None or 8 words, integers below 2^32"),
    (kec([W(KRND, rate=0, msg=[])]), "commit_keccak: keccak: the msg of a rounds unit must hold 5 row indices, integers in [0, 2^32 - 1)"),
    (kec([W(KROW, out=[25], expect=[])]), "commit_keccak: keccak: a lane index must be an integer below 25"),
    (kec([W(KRND, start=-1, period=0)]), "commit_keccak: keccak: start must be a row index, an integer in [0, 2^32 - 1), or None"),
    (ec(W(CV, bits=0, limbs=0), []), "commit_ec: ec: the limb width b (bits) must be an integer in [1, 64]"),
    (ec(CV, [W(DIV, b=-1, out=DEL)]), "commit_ec: ec: b must be a first row, an integer in [0, 2^32 - 1)"),
    (ec(CV, [W(ECH, op=None, cols=[])]), "commit_ec: ec: op must be a first row, an integer in [0, 2^32 - 1)"),
    (ec(CV, [W(EADD, out=["zz", "zz"])]), "commit_ec: ec: unknown name 'zz' (the names of a add unit are lam, x3, y3)"),
    (ec(CV, [W(DIV, a=5)], 2), "commit_ec: ec: the operand run of a reaches beyond the 2 concatenated rows of the input sets"),
    (edw(W(ED, a=0, d=0), []), "commit_edwards: edwards: the coefficients A and D must not be 0"),
    (edw(ED, [W(DADD, x1=None, out=DEL)]),
     "commit_edwards: edwards: x1 must be a row index, an integer in [0, 2^32 - 2), or (\"imm\", value)"),
    (edw(ED, [W(DCH, op=True, cols=[])]), "commit_edwards: edwards: op must be a row, an integer in [0, 2^32 - 2)"),
    (edw(ED, [W(DADD, out=DEL, expect=[None, 9])], 5),
     "commit_edwards: edwards: an entry of expect reaches beyond the 5 concatenated rows of the input sets"),
]


def _message(err):
    """the KzgError's text behind the status name that its constructor puts in front"""
    assert err.code == _native.KZG_E_ARG
    return str(err).split(": ", 1)[1]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_the_whole_message(case):
    (encoder, args), message = CASES[case]
    with pytest.raises(KzgError) as e:
        getattr(HipEngine, encoder)(*args)
    assert _message(e.value) == message


def test_the_cap_on_the_width_of_ec(monkeypatch):
    """64 bits in four limbs are 256, so the cap on W = b L is reached with the cap on limbs lifted"""
    monkeypatch.setattr(_native, "KZG_EC_MAX_LIMBS", 5)
    with pytest.raises(KzgError) as e:
        HipEngine.ec_call(W(CV, bits=64, limbs=5), [DIV])
    assert _message(e.value) == "commit_ec: ec: the width W = b L must be at most 256"


def test_the_cap_on_output_rows_of_edwards(monkeypatch):
    """Four units of two names each cannot pass 16 output rows, so the closing cap is reached with the cap on units lifted"""
    monkeypatch.setattr(_native, "KZG_EDWARDS_MAX_UNITS", 9)
    with pytest.raises(KzgError) as e:
        HipEngine.edwards_call(ED, [W(DADD, out=["x3", "y3"])] * 9)
    assert _message(e.value) == "commit_edwards: edwards: n_out: the units give 18 output rows, at most 16 fit one call"


def test_every_place_of_refusal_has_a_case():
    assert len({m for _, m in CASES}) >= 150
