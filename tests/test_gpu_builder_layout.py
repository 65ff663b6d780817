"""GPU tests (`-m gpu`) of what the fourteen column builders share: sorted, derived, int, alu, wide, poseidon, expr,
recurrence, fetch and the five further unit builders sha256, keccak, ec, edwards and poseidon_chain go through one call frame
and one check of the `usable` / `tail_be32` layout, and this module pins, for all fourteen, what that frame must keep and what
no builder's own module pins for every one of them: the five layout refusals with their WHOLE texts, the order of refusals as
a caller sees it, the calls that may omit the tail because nothing takes one, and that the engine serves the next call with no
set and no byte leaked after every refusal.

Every call goes through the raw binding (the engine's Python checks would answer first) with the builder's cheapest valid
arguments: one op, unit, expression or read over one or two committed rows; the five unit builders' structs come from the
engine's encoders and are spoilt afterwards.  T = 16 throughout, except where 33 rows must lie behind `usable`: T = 64 is the
smallest power of two at which more than KZG_MAX_BLIND_ROWS = 32 can."""
import ctypes

import pytest

from tests.gpu_common import R, be
from tests.gpu_rows import commit_sets, engine_cache, release
from zkp_subnet_amd import _native as N
from zkp_subnet_amd.engine import HipEngine

pytestmark = pytest.mark.gpu
SEED_X, SEED_Y = 0x1A7B111D, 0x1A7B111E
E_ARG = N.KZG_E_ARG
UNKNOWN = 2 ** 40          # a handle that names no set
OOB = 5                    # a row index outside the two rows of the input set


@pytest.fixture(scope="module")
def engines(hip):
    return engine_cache(hip, SEED_X, SEED_Y)


@pytest.fixture(scope="module")
def resident(engines):
    """per log2 row length: the engine and three sets of small integers -- `two` (rows 0 and 1), `one` and `tab` (one row each)"""
    cache = {}

    def get(lg):
        if lg not in cache:
            eng, T = engines(lg), 1 << lg
            rows = [[(3 * t + 1) % T for t in range(T)], [(5 * t + 2) % T for t in range(T)]]
            two, one, tab = commit_sets(eng, rows + [rows[0], rows[1]], (2, 1, 1))
            cache[lg] = (eng, {"two": two, "one": one, "tab": tab})
        return cache[lg]

    yield get
    for _, sets in cache.values():
        release(list(sets.values()))


# ------------------------------------------------------------------------------------------------ the fourteen raw calls
# Each takes the engine, the resident sets, the layout (usable, tail bytes or None) and what to get wrong: `row` -- a row index
# (or, where the builder has none, the row count) that does not fit the input sets; `op` -- the op, unit, flag or count that is
# refused before a lane is taken; `handle` -- a handle that names no set; `check` -- every unit only checks (expr, poseidon,
# poseidon_chain).
# Returns (status, handle of the new set).
def _u64s(vals):
    return (ctypes.c_uint64 * len(vals))(*vals)


def _outs():
    return ctypes.create_string_buffer(48 * 16), [(ctypes.c_uint64 * 32)() for _ in range(4)], ctypes.c_uint64(0)


def _handles(sets, name, handle):
    return _u64s([UNKNOWN if handle else sets[name].handle])


def _terms(rows):
    lens, tr = (ctypes.c_uint32 * 1)(len(rows)), (ctypes.c_uint32 * max(len(rows), 1))(*rows)
    return N.QuotientTerms(1, be(1), lens, tr, None), (lens, tr)


def call_sorted(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    c, _, h = _outs()
    opts = N.SortedOpts(usable, tail)
    rc = N.load().kzg_rows_commit_sorted(eng._h, 1, _handles(sets, "two", handle), 3 if row else 2, 0 if op else 1,
                                         ctypes.byref(opts), c, ctypes.byref(h))
    return rc, h.value


def call_derived(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    c, o, h = _outs()
    ops = (N.DeriveOp * 1)(N.DeriveOp(9 if op else N.KZG_DERIVE_INV0, OOB if row else 0, 0, 1))
    opts = N.DeriveOpts(usable, tail)
    rc = N.load().kzg_rows_commit_derived(eng._h, 1, _handles(sets, "two", handle), 1, ops, ctypes.byref(opts), c, o[0],
                                          ctypes.byref(h))
    return rc, h.value


def call_int(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    c, o, h = _outs()
    ops = (N.IntOp * 1)(N.IntOp(99 if op else N.KZG_INT_ADD, 8, OOB if row else 0, 1, 0, 0, 1))
    opts = N.DeriveOpts(usable, tail)
    rc = N.load().kzg_rows_commit_int(eng._h, 1, _handles(sets, "two", handle), 1, ops, ctypes.byref(opts), c, o[0], o[1],
                                      ctypes.byref(h))
    return rc, h.value


def call_alu(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    c, o, h = _outs()
    prog = (N.AluEntry * 1)(N.AluEntry(99 if op else N.KZG_ALU_ADD, 8, 0, 0, 0))
    units = (N.AluUnit * 1)(N.AluUnit(0, OOB if row else 0, 1, 1))
    opts = N.DeriveOpts(usable, tail)
    rc = N.load().kzg_rows_commit_alu(eng._h, 1, _handles(sets, "two", handle), 1, prog, 1, units, ctypes.byref(opts), c, o[0],
                                      o[1], o[2], o[3], ctypes.byref(h))
    return rc, h.value


def call_wide(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    c, o, h = _outs()
    A = N.KZG_WIDE_ABSENT
    ops = (N.WideOp * 1)(N.WideOp(99 if op else N.KZG_WIDE_ADD, 8, 1, 1, 0, OOB if row else 0, 1, A, A, A))
    opts = N.DeriveOpts(usable, tail)
    rc = N.load().kzg_rows_commit_wide(eng._h, 1, _handles(sets, "two", handle), 1, ops, ctypes.byref(opts), c, o[0], o[1], o[2],
                                       o[3], ctypes.byref(h))
    return rc, h.value


def call_poseidon(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    c, o, h = _outs()
    params = N.PoseidonParams(2, 2, 0, b"".join(be(v) for v in (1, 2, 3, 4)), b"".join(be(v) for v in (2, 1, 1, 3)))
    u = N.PoseidonUnit()
    u.mode, u.flags, u.n_out, u.period = (9 if op else N.KZG_POSEIDON_ROW), (N.KZG_POSEIDON_CHECK if check else 0), 1, 0
    u.in_[0], u.in_[1], u.out[0], u.expect[0] = (OOB if row else 0), 1, 0, 0
    units = (N.PoseidonUnit * 1)(u)
    opts = N.DeriveOpts(usable, tail)
    rc = N.load().kzg_rows_commit_poseidon(eng._h, 1, _handles(sets, "two", handle), ctypes.byref(params), 1, units,
                                           ctypes.byref(opts), c, o[0], o[1], o[2], ctypes.byref(h))
    return rc, h.value


def call_expr(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    c, o, h = _outs()
    terms, keep = _terms([OOB if row else 0])
    exprs = (N.Expr * 1)(N.Expr(terms, 2 if op else (N.KZG_EXPR_CHECK if check else 0)))
    opts = N.ExprOpts(usable, tail)
    rc = N.load().kzg_rows_commit_expr(eng._h, 1, _handles(sets, "two", handle), 1, exprs, ctypes.byref(opts), c, o[0], o[1],
                                       ctypes.byref(h))
    return rc, h.value


def call_recur(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    c, _, h = _outs()
    closing = ctypes.create_string_buffer(32 * 16)
    add, keep = _terms([OOB if row else 0])
    empty = N.QuotientTerms(0, None, None, None, None)
    recs = (N.Recurrence * 1)(N.Recurrence(empty, empty if op else add, be(1)))
    opts = N.RecurrenceOpts(usable, tail)
    rc = N.load().kzg_rows_commit_recurrence(eng._h, 1, _handles(sets, "two", handle), 1, recs, ctypes.byref(opts), c, closing,
                                             ctypes.byref(h))
    return rc, h.value


def call_fetch(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    c, o, h = _outs()
    opts = N.DeriveOpts(usable, tail)
    rc = N.load().kzg_rows_commit_fetch(eng._h, 1, _handles(sets, "two" if row else "one", handle), 1, _u64s([sets["tab"].handle]),
                                        1, 0, 2 if op else 0, ctypes.byref(opts), c, o[0], o[1], ctypes.byref(h))
    return rc, h.value


def _unit_call(fn, eng, sets, usable, tail, handle, lead, unit, n_stats):
    """one unit of a unit builder through its raw call `fn`; lead: the params or curve struct in front of the units, or None"""
    c, _, h = _outs()
    st = [(ctypes.c_uint64 * 1)() for _ in range(n_stats)]
    opts = N.DeriveOpts(usable, tail)
    rc = fn(eng._h, 1, _handles(sets, "two", handle), *(() if lead is None else (ctypes.byref(lead),)), 1, (type(unit) * 1)(unit),
            ctypes.byref(opts), c, *st, ctypes.byref(h))
    return rc, h.value


def call_sha256(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    rec, = HipEngine.sha256_call([{"mode": "row", "state": "iv", "msg": [("imm", 0)] * 15 + [0], "out": [0]}])
    u = HipEngine.sha256_unit_struct(rec)
    u.mode, u.msg[15] = (9 if op else u.mode), (OOB if row else 0)
    return _unit_call(N.load().kzg_rows_commit_sha256, eng, sets, usable, tail, handle, None, u, 6)


def call_keccak(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    rec, = HipEngine.keccak_call([{"mode": "row", "in": [("imm", 0)] * 24 + [0], "out": [0]}])
    u = HipEngine.keccak_unit_struct(rec)
    u.mode, u.in_[24] = (9 if op else u.mode), (OOB if row else 0)
    return _unit_call(N.load().kzg_rows_commit_keccak, eng, sets, usable, tail, handle, None, u, 6)


def call_ec(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    cv, recs = HipEngine.ec_call({"bits": 8, "limbs": 1, "p": 251, "a": 1}, [{"mode": "div", "a": 0, "b": 1, "out": True}])
    curve, arr = HipEngine.ec_structs(cv, recs)
    u = arr[0]
    u.mode, u.in_[0] = (9 if op else u.mode), (OOB if row else 0)
    return _unit_call(N.load().kzg_rows_commit_ec, eng, sets, usable, tail, handle, curve, u, 9)


def call_edwards(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    cv, recs = HipEngine.edwards_call({"a": 2, "d": 3}, [{"mode": "add", "x1": 0, "y1": 1, "x2": 1, "y2": 0, "out": ["x3"]}])
    curve, arr = HipEngine.edwards_structs(cv, recs)
    u = arr[0]
    u.mode, u.in_[0] = (9 if op else u.mode), (OOB if row else 0)
    return _unit_call(N.load().kzg_rows_commit_edwards, eng, sets, usable, tail, handle, curve, u, 7)


def call_poseidon_chain(eng, sets, usable, tail, row=False, op=False, handle=False, check=False):
    form = {"expect": 1, "digest": 0} if check else {"layout": "flat", "cols": ["out0"]}
    par, recs = HipEngine.poseidon_chain_call({"t": 2, "full": 2, "partial": 0, "rc": [1, 2, 3, 4], "mds": [2, 1, 1, 3]},
                                              [dict({"mode": "sponge", "in": [0, 1], "start": None, "period": 1}, **form)])
    u = HipEngine.poseidon_chain_unit_struct(recs[0])
    u.mode, u.in_[0] = (9 if op else u.mode), (OOB if row else 0)
    return _unit_call(N.load().kzg_rows_commit_poseidon_chain, eng, sets, usable, tail, handle, N.PoseidonParams(*par), u, 6)


ROW = "%s: a row must index the concatenated rows of the input sets"
READ, GIVEN = "all T rows are read", "%s: tail_be32 must be given when usable > 0"
# name -> (call, prefix, the phrase of the first refusal, the tail-missing text, committed columns, closing rows, the text of
#          the `row` mistake, the text of the `op` mistake)
BUILDERS = {
    "sorted": (call_sorted, "sorted", "all T rows are sorted", GIVEN, 2, 0, "sorted: the input sets must hold exactly width rows",
               "sorted: n_keys must be in [1, width]"),
    "derived": (call_derived, "derived", READ, GIVEN, 1, 0, ROW, "derived: unknown kind (KZG_DERIVE_INV0 or KZG_DERIVE_LIMBS)"),
    "int": (call_int, "int", READ, GIVEN, 1, 0, ROW, "int: unknown kind (KZG_INT_AND .. KZG_INT_SPLIT)"),
    "alu": (call_alu, "alu", READ, GIVEN, 1, 0, ROW, "alu: unknown kind (KZG_ALU_IDLE, KZG_ALU_AND .. KZG_ALU_SEXT)"),
    "wide": (call_wide, "wide", READ, GIVEN, 1, 0,
             "wide: the L rows of an operand must lie inside the concatenated rows of the input sets",
             "wide: unknown kind (KZG_WIDE_ADD .. KZG_WIDE_CARRY)"),
    "poseidon": (call_poseidon, "poseidon", READ, GIVEN, 1, 0, ROW,
                 "poseidon: unknown mode (KZG_POSEIDON_ROW or KZG_POSEIDON_ROUNDS)"),
    "expr": (call_expr, "expr", "all T rows are evaluated", GIVEN, 1, 0, ROW, "expr: flags must be 0 or KZG_EXPR_CHECK"),
    "recurrence": (call_recur, "recur", "the plain layout", "%s: tail_be32 may be null only when usable = T - 1", 1, 1, ROW,
                   "recur: mul and add must not both be empty (v would be the constant start)"),
    "fetch": (call_fetch, "fetch", READ, GIVEN, 1, 0, "fetch: the input sets must hold exactly n_reads * max(n_keys, 1) rows",
              "fetch: flags must be 0 or KZG_FETCH_INDEX"),
    "sha256": (call_sha256, "sha256", READ, GIVEN, 1, 0, ROW, "sha256: unknown mode (KZG_SHA256_ROW or KZG_SHA256_ROUNDS)"),
    "keccak": (call_keccak, "keccak", READ, GIVEN, 1, 0, ROW, "keccak: unknown mode (KZG_KECCAK_ROW or KZG_KECCAK_ROUNDS)"),
    "ec": (call_ec, "ec", READ, GIVEN, 1, 0, "ec: an operand run must lie inside the concatenated rows of the input sets",
           "ec: unknown mode (KZG_EC_DIV, KZG_EC_ADD or KZG_EC_CHAIN)"),
    "edwards": (call_edwards, "edwards", READ, GIVEN, 1, 0, ROW, "edwards: unknown mode (KZG_EDWARDS_ADD or KZG_EDWARDS_CHAIN)"),
    "poseidon_chain": (call_poseidon_chain, "poseidon_chain", READ, GIVEN, 1, 0, ROW,
                       "poseidon_chain: unknown mode (KZG_POSEIDON_CHAIN_SPONGE or KZG_POSEIDON_CHAIN_PATH)"),
}
NAMES = list(BUILDERS)


def text(pattern, prefix):
    return (pattern % prefix if "%s" in pattern else pattern).encode()


def tail_bytes(n_cols, per_col, last=7):
    """n_cols * per_col canonical scalars, the last of them `last`"""
    vals = [11 + j for j in range(n_cols * per_col)]
    return b"".join(be(v) for v in vals[:-1]) + last.to_bytes(32, "big")


class Served:
    """the engine, its sets and one builder: refusals with their whole text, each followed by the builder's valid call, with the
    live sets and bytes of rows_stats compared before and after"""

    def __init__(self, eng, sets, name):
        self.eng, self.sets = eng, sets
        self.call, self.prefix, self.phrase, self.no_tail, self.n_cols, self.closing, self.row_text, self.op_text = BUILDERS[name]
        self.valid()   # (the first call of a lane allocates its workspace and the set's buffer: not part of any comparison)
        self.live = eng.rows_stats()

    def valid(self, usable=0, tail=None, check=False, want_set=True):
        rc, h = self.call(self.eng, self.sets, usable, tail, check=check)
        assert rc == 0, (rc, N.load().kzg_last_error(self.eng._h))
        assert (h != 0) == want_set
        if h:
            self.eng.release_rows(h)

    def refused(self, want, usable=0, tail=None, **wrong):
        rc, _ = self.call(self.eng, self.sets, usable, tail, **wrong)
        msg = N.load().kzg_last_error(self.eng._h)
        assert rc == E_ARG and msg == want, (rc, msg, want)
        assert self.eng.rows_stats() == self.live
        self.valid()
        assert self.eng.rows_stats() == self.live


@pytest.mark.parametrize("name", NAMES)
def test_layout_refusals(resident, name):
    """the five refusals of the one layout check, in its order, each with its whole text"""
    eng, sets = resident(4)
    S, T = Served(eng, sets, name), 16
    p, per = S.prefix, 4 - S.closing
    tl = tail_bytes(S.n_cols, per)
    S.refused(b"%s: usable must be in [1, T - 1] (0: %s)" % (p.encode(), S.phrase.encode()), T, tl)
    S.refused(text(S.no_tail, p), T - 4, None)
    S.refused(b"%s: tail scalars must be canonical (< r)" % p.encode(), T - 4, tail_bytes(S.n_cols, per, last=R))
    S.refused(b"%s: tail_be32 must be null in the plain layout (usable = 0)" % p.encode(), 0, tl)
    S.valid(T - 4, tl)   # and the layout itself is served
    assert eng.rows_stats() == S.live


@pytest.mark.parametrize("name", NAMES)
def test_blind_rows_refusal(resident, name):
    """33 rows at or behind `usable`: T = 64, usable = 31"""
    eng, sets = resident(6)
    S = Served(eng, sets, name)
    S.refused(b"%s: at most KZG_MAX_BLIND_ROWS rows may lie at or behind row `usable`" % S.prefix.encode(), 64 - 33,
              tail_bytes(S.n_cols, 33))


@pytest.mark.parametrize("name", NAMES)
def test_refusal_order(resident, name):
    """two mistakes at once.  The builder's check between the lookup and the layout (a row index outside the input sets; for
    sorted and fetch, which take no row index, the number of rows the sets hold) answers before the layout's.  The op (for
    sorted n_keys, for fetch the flags, for recurrence two empty sides) is checked before a lane is taken in all the builders,
    so it answers before the unknown handle's "<p>: unknown or released handle"."""
    eng, sets = resident(4)
    S, T = Served(eng, sets, name), 16
    S.refused(text(S.row_text, S.prefix), T, tail_bytes(S.n_cols, 4), row=True)
    S.refused(text(S.op_text, S.prefix), op=True, handle=True)
    S.refused(b"%s: unknown or released handle" % (b"fetch: inputs" if name == "fetch" else S.prefix.encode()), handle=True)


@pytest.mark.parametrize("name", ["expr", "poseidon", "poseidon_chain"])
def test_checks_only_needs_no_tail(resident, name):
    """every unit a check: nothing is committed, so no column takes a tail -- null is accepted in the usable layout, the call
    returns handle 0 and the live sets stay as they were"""
    eng, sets = resident(4)
    S = Served(eng, sets, name)
    S.valid(16 - 4, None, check=True, want_set=False)
    assert eng.rows_stats() == S.live
    S.refused(text(S.no_tail, S.prefix), 16 - 4, None)   # the same layout with a committed column


def test_recurrence_closing_row_alone(resident):
    """usable = T - 1: the closing row is the last row, no tail scalar exists and the pointer may be null"""
    eng, sets = resident(4)
    S = Served(eng, sets, "recurrence")
    S.valid(16 - 1, None)
    assert eng.rows_stats() == S.live
