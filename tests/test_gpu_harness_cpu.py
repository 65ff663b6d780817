"""Device-free tests of the GPU tests' own checkers (tests/gpu_rows.py): check_one_row and check_pieces accept a truthful
engine and raise AssertionError for one wrong commitment byte, one wrong evaluation at any probed domain point, a wrong value
at the random point and a wrong k / T / i; the two probe rules yield the index sets the modules rely on; commit_sets splits
rows by `sizes`.  The engine and the sets are stubs built only from the C oracle, at T = 2^4."""
import functools
import random

import pytest

from oracle import cpu as oc
from tests import grand_product_ref as gp
from tests.gpu_common import R, be, ints, row_bytes, val
from tests.gpu_rows import (arg_error, check_one_row, check_pieces, commit_sets, probes_closing, probes_ends, rand_rows,
                            release, split_first, split_halves, srs_cache, tail_of)
from zkp_subnet_amd import _native
from zkp_subnet_amd._native import KzgError

LG, T, U = 4, 16, 11
SEED_X, SEED_Y = 0x4A12E5, 0x4A12E6
W = gp.omega(T)
srs_of = srs_cache(SEED_X, SEED_Y)


@functools.lru_cache(maxsize=None)
def oracle_commit(row, ef):
    return oc.commit(srs_of(LG), row, ef)


class StubSet:
    def __init__(self, i, coeffs, commitments):
        self.i, self.k, self.T, self.commitments = i, len(coeffs), len(coeffs[0]) // 32, commitments
        self.coeffs, self.released = coeffs, False

    def release(self):
        self.released = True


class StubEngine:
    """commit_rows and eval_rows from the oracle; `lie(x, j)` says where an evaluation comes back off by one"""

    def __init__(self, lie=lambda x, j: False):
        self.lie, self.made = lie, []

    def commit_rows(self, i, rows, ef=True):
        self.made.append(StubSet(i, [oc.fr_ntt(r, True) if ef else r for r in rows], [oracle_commit(r, ef) for r in rows]))
        return self.made[-1]

    def eval_rows(self, sets, points, opened):
        rows = [c for s in sets for c in s.coeffs]
        return [[be(val(oc.fr_eval(rows[j], x)) + self.lie(val(x), j)) for j in js] for x, js in zip(points, opened)]


ROW = rand_rows(1, T, 77)[0]
PIECES = rand_rows(3, T, 78)                    # three coefficient rows
PIECE_BYTES = [row_bytes(p) for p in PIECES]


def one_row_set(eng=None):
    return commit_sets(eng or StubEngine(), [ROW], (1,))[0]


def piece_set(eng=None):
    return commit_sets(eng or StubEngine(), PIECE_BYTES, (3,), ef=False)[0]


def rules():
    """(name, the indices the rule yields at T = 16 with the draws of Random(5))"""
    return [("ends", probes_ends(T, random.Random(5))), ("closing", probes_closing(T, U)), ("plain", probes_closing(T, None))]


def test_the_probe_rules():
    rnd, twin = random.Random(5), random.Random(5)
    assert probes_ends(T, rnd) == sorted({0, 1, T - 1} | {twin.randrange(T) for _ in range(3)})
    assert rnd.random() == twin.random()                                     # three draws, no more
    assert probes_ends(1, random.Random(1)) == [0] and probes_ends(2, random.Random(1)) == [0, 1]
    assert probes_closing(T, U) == [0, U - 1, U, U + 1, T - 1] == [0, 10, 11, 12, 15]
    assert probes_closing(T, None) == probes_closing(T, T - 1) == [0, T - 2, T - 1]
    assert probes_closing(T, 1) == [0, 1, 2, T - 1]
    assert probes_closing(T, T - 2) == [0, T - 3, T - 2, T - 1]


def test_the_shared_small_helpers():
    assert tail_of(T, U, 3) == tail_of(T, U, 3) and len(tail_of(T, U, 3)) == T - U - 1 and tail_of(T, None, 3) == []
    assert tail_of(T, T - 1, 3) == [] and all(0 <= v < R for v in tail_of(T, 1, 3))
    assert [split_first(k) for k in (1, 2, 3, 6)] == [(1,), (2,), (1, 2), (1, 5)]
    assert [split_halves(k) for k in (1, 2, 3, 6)] == [(1,), (2,), (1, 2), (3, 3)]
    assert ints(row_bytes([0, 1, R - 1, R + 5])) == [0, 1, R - 1, 5] and val(be(-1)) == R - 1

    def fail(code, msg):
        raise KzgError(code, msg)

    assert "stale" in str(arg_error(lambda: fail(_native.KZG_E_ARG, "a stale set"), "stale"))
    arg_error(lambda: fail(_native.KZG_E_BUSY, "full"), code=_native.KZG_E_BUSY)
    for bad in (lambda: fail(_native.KZG_E_BUSY, "a stale set"), lambda: fail(_native.KZG_E_ARG, "another message")):
        with pytest.raises(AssertionError):
            arg_error(bad, "stale")
    with pytest.raises(pytest.fail.Exception):
        arg_error(lambda: None)


def test_commit_sets_splits_rows_by_sizes():
    rows = rand_rows(5, T, 90)
    eng = StubEngine()
    sets = commit_sets(eng, rows, (2, 1, 2), i=3)
    assert [(s.k, s.i, s.T) for s in sets] == [(2, 3, T), (1, 3, T), (2, 3, T)] and eng.made == sets
    want = [oc.commit(srs_of(LG), row_bytes(r), True) for r in rows]
    assert [c for s in sets for c in s.commitments] == want
    # rows of integers are evaluations in either form (coefficient form goes through the oracle's INTT); rows of bytes are
    # committed as they are
    coeff = commit_sets(eng, rows, (5,), ef=False)[0]
    assert coeff.commitments == want and coeff.coeffs == [oc.fr_ntt(row_bytes(r), True) for r in rows]
    raw = commit_sets(eng, [row_bytes(r) for r in rows], (4, 1), ef=False)
    assert [c for s in raw for c in s.coeffs] == [row_bytes(r) for r in rows]
    assert commit_sets(eng, [row_bytes(r) for r in rows], (5,))[0].commitments == want
    release(sets)
    assert all(s.released for s in sets) and not coeff.released
    for sizes in ((2, 2), (3, 3), ()):
        fresh = StubEngine()
        with pytest.raises(AssertionError):
            commit_sets(fresh, rows, sizes)
        assert not fresh.made


def test_check_one_row_accepts_a_truthful_engine():
    for _, probes in rules():
        for ef in (True, False):
            eng = StubEngine()
            rset = commit_sets(eng, [ROW], (1,), ef)[0]
            rnd, twin = random.Random(9), random.Random(9)
            check_one_row(eng, srs_of(LG), rset, ROW, rnd, probes=probes)
            twin.randrange(R)
            assert rnd.random() == twin.random()                             # one draw: the random point
    eng = StubEngine()
    check_one_row(eng, srs_of(LG), commit_sets(eng, [ROW], (1,), i=2)[0], ROW, random.Random(9), probes=[0], i=2)
    check_one_row(eng, srs_of(LG), one_row_set(eng), ROW, random.Random(9), probes=[0], want_commitment=one_row_set().commitments[0])


def test_check_one_row_sees_each_fault():
    srs = srs_of(LG)
    ok = lambda eng, rset, probes, **kw: check_one_row(eng, srs, rset, ROW, random.Random(9), probes=probes, **kw)   # noqa: E731

    def refused(eng, rset, probes=(0,), **kw):
        with pytest.raises(AssertionError):
            ok(eng, rset, probes, **kw)

    # one wrong commitment byte (also when the caller hands the expected commitment in)
    rset = one_row_set()
    good = rset.commitments[0]
    rset.commitments = [good[:20] + bytes([good[20] ^ 1]) + good[21:]]
    refused(StubEngine(), rset)
    refused(StubEngine(), one_row_set(), want_commitment=rset.commitments[0])
    # one wrong evaluation at a probed domain point, for each rule and each of its points; elsewhere on the domain the rule
    # does not look
    domain = {pow(W, t, R): t for t in range(T)}
    for name, probes in rules():
        for t in range(T):
            eng = StubEngine(lambda x, j, t=t: domain.get(x) == t)
            if t in probes:
                refused(eng, one_row_set(eng), probes)
            else:
                ok(eng, one_row_set(eng), probes)
    # a wrong value at the random point
    eng = StubEngine(lambda x, j: x not in domain)
    refused(eng, one_row_set(eng), range(T))
    # a wrong k, T or i
    eng = StubEngine()
    refused(eng, commit_sets(eng, [ROW, ROW], (2,))[0])
    refused(eng, commit_sets(eng, [ROW], (1,), i=1)[0])
    refused(eng, one_row_set(eng), i=1)
    rset = one_row_set(eng)
    rset.T = T // 2
    refused(eng, rset)
    rset = one_row_set(eng)
    rset.commitments = rset.commitments * 2
    refused(eng, rset)


def check_pieces_with(eng, tset, **kw):
    check_pieces(eng, srs_of(LG), tset, PIECES, random.Random(9), **kw)


DRAWN = random.Random(9).randrange(T)           # the domain index check_pieces draws from Random(9)


def test_check_pieces_accepts_a_truthful_engine():
    eng = StubEngine()
    rnd, twin = random.Random(9), random.Random(9)
    check_pieces(eng, srs_of(LG), piece_set(eng), PIECES, rnd)
    assert twin.randrange(T) == DRAWN and twin.randrange(R) < R
    assert rnd.random() == twin.random()                                     # two draws: a domain index and a point
    check_pieces_with(eng, commit_sets(eng, PIECE_BYTES, (3,), ef=False, i=1)[0], i=1)
    # a wrong evaluation at a domain point the checker does not look at goes unseen
    domain = {pow(W, t, R): t for t in range(T)}
    quiet = next(t for t in range(1, T - 1) if t != DRAWN)
    eng = StubEngine(lambda x, j: domain.get(x) == quiet)
    check_pieces_with(eng, piece_set(eng))


def test_check_pieces_sees_each_fault():
    def refused(eng, tset, **kw):
        with pytest.raises(AssertionError):
            check_pieces_with(eng, tset, **kw)

    # one wrong commitment byte in any piece
    for p in range(3):
        tset = piece_set()
        c = tset.commitments[p]
        tset.commitments[p] = c[:47] + bytes([c[47] ^ 1])
        refused(StubEngine(), tset)
    # one wrong evaluation of one piece at each probed domain point, and a wrong value at the random point
    domain = {pow(W, t, R): t for t in range(T)}
    for p, t in enumerate((0, T - 1, DRAWN)):
        eng = StubEngine(lambda x, j, t=t, p=p: domain.get(x) == t and j == p)
        refused(eng, piece_set(eng))
    eng = StubEngine(lambda x, j: x not in domain and j == 2)
    refused(eng, piece_set(eng))
    # a wrong k, T or i
    eng = StubEngine()
    refused(eng, commit_sets(eng, PIECE_BYTES[:2], (2,), ef=False)[0])
    refused(eng, commit_sets(eng, PIECE_BYTES, (3,), ef=False, i=1)[0])
    refused(eng, piece_set(eng), i=1)
    tset = piece_set(eng)
    tset.T = 2 * T
    refused(eng, tset)
