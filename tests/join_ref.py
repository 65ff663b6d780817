"""Reference model of the hash join of csrc/fr_join.hip (no GPU; used by tests/test_join_cpu.py and tests/test_gpu_join.py).

The join is an open-addressing table: a tuple's walk starts at its HOME slot, hash & (cap - 1), and goes on with (s + 1) & mask.
Which tuple ends in which slot depends on the schedule; WHICH SLOTS are occupied does not (linear probing fills the same set in
every insertion order), and neither does anything a probe answers.  The model restates, in Python integers and numpy words,

  the 8 words of a cell       words          v * 2^261 mod r, little-endian (the canonical Montgomery words the join hashes)
  the hash                    join_hash      MurmurHash3 x86_32, seed 0x9747b28c, over the w * 32 bytes, no tail
  the occupied slots          occupied       from the homes of the distinct tuples alone
  a key search                keys_at        tuples with a GIVEN home, from consecutive small candidates

and builds input families in which a named path is certain to run: a chain of D slots that wraps from slot cap - 1 to slot 0, a
staircase of displaced groups, tuples that differ in their last column only, a table cut at `rows`, a full table.  Each family
states its facts (the occupied slots, how far every miss walks); tests/test_join_cpu.py checks them before any GPU call."""
import functools
import random

import numpy as np

from oracle.bls12_381 import R
from tests.poly_ref import MONT

SEED = 0x9747B28C
EMPTY = 0xFFFFFFFF
CHUNK = 1 << 16                      # candidates hashed at a time
CEILING = 1_500_000                  # candidates a search may look at (measured: 3.2 s, 754 keys at one home of 2048)
LAST_FIXED = (0x1234567, 0x89ABCDE)  # columns 0 and 1 of the last_column_only candidates


# ---------------------------------------------------------------------------------------------------- words and hash
def words(values):
    """(n, 8) uint32: the little-endian 32-bit words of v * 2^261 mod r"""
    raw = b"".join((v % R * MONT % R).to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype="<u4").reshape(-1, 8).astype(np.uint32)


def _rotl(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def join_hash(cols):
    """the hash of tuple t = (cols[0][t], .., cols[w - 1][t]) for every t, as fr_join.hip's join_hash computes it"""
    w, n = len(cols), len(cols[0])
    h = np.full(n, SEED, dtype=np.uint32)
    for col in cols:
        W = words(col)
        for j in range(8):
            k = W[:, j] * np.uint32(0xCC9E2D51)
            k = _rotl(k, 15) * np.uint32(0x1B873593)
            h = _rotl(h ^ k, 13) * np.uint32(5) + np.uint32(0xE6546B64)
    h = h ^ np.uint32(w * 32)
    h = (h ^ (h >> np.uint32(16))) * np.uint32(0x85EBCA6B)
    h = (h ^ (h >> np.uint32(13))) * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def home(cols, cap):
    assert cap >= 1 and cap & (cap - 1) == 0
    return join_hash(cols) & np.uint32(cap - 1)


def homes_of(tuples, cap):
    """the home slot of every tuple of a list of w-tuples, as Python integers"""
    if not tuples:
        return []
    return [int(h) for h in home([list(c) for c in zip(*tuples)], cap)]


# ---------------------------------------------------------------------------------------------------- the table
def occupied(homes_of_distinct_tuples, cap):
    """the slots that linear probing fills for distinct tuples with these homes: the same set in every insertion order"""
    assert len(homes_of_distinct_tuples) <= cap
    occ = set()
    for s in homes_of_distinct_tuples:
        while s in occ:
            s = (s + 1) % cap
        occ.add(s)
    return occ


def miss_walk(h, occ, cap):
    """how many occupied slots the walk of an absent tuple with home h passes before it meets an empty one (cap: none is empty)"""
    n = 0
    while n < cap and (h + n) % cap in occ:
        n += 1
    return n


def simulate_build(tuples, cap, order):
    """k_join_build with the lanes run one after the other in `order` (row indices of `tuples`): the slot words"""
    slots = [EMPTY] * cap
    hs = homes_of(tuples, cap)
    for t in order:
        s = hs[t]
        for _ in range(cap):
            if slots[s] == EMPTY:
                slots[s] = t
                break
            if tuples[slots[s]] == tuples[t]:
                slots[s] = min(slots[s], t)
                break
            s = (s + 1) % cap
        else:
            raise AssertionError("build overrun")
    return slots


def check_slots(slots, tuples, cap):
    """The schedule-independent facts of a built table over the rows `tuples` (the rows below `rows` only): the occupied slots
    are the model's set; every occupied slot holds the smallest row of its tuple; every distinct tuple sits in exactly one slot;
    all slots from a tuple's home to its slot, cyclically, are occupied.  Returns {tuple: slot}."""
    assert len(slots) == cap
    first = {}
    for t, tup in enumerate(tuples):
        first.setdefault(tup, t)
    distinct = list(first)
    hs = homes_of(distinct, cap)
    occ = {s for s, q in enumerate(slots) if q != EMPTY}
    assert occ == occupied(hs, cap), (sorted(occ ^ occupied(hs, cap))[:8], len(occ))
    where = {}
    for s in sorted(occ):
        q = slots[s]
        assert q < len(tuples), (s, q)
        assert first[tuples[q]] == q, f"slot {s} holds row {q}, the smallest row of its tuple is {first[tuples[q]]}"
        assert tuples[q] not in where, f"the tuple of row {q} sits in slots {where[tuples[q]]} and {s}"
        where[tuples[q]] = s
    assert set(where) == set(first)
    for tup, h in zip(distinct, hs):
        for d in range((where[tup] - h) % cap):
            assert (h + d) % cap in occ, f"an empty slot between home {h} and slot {where[tup]}"
    return where


# ---------------------------------------------------------------------------------------------------- the key search
def candidate(v, w, last_column_only=False):
    """candidate v >= 1 as a w-tuple: every column moves with v, or (w = 3) only the last one does"""
    if last_column_only:
        assert w == 3
        return LAST_FIXED + (v,)
    return tuple(v + (c << 40) for c in range(w))


@functools.lru_cache(maxsize=None)
def _hashes(w, last_column_only, chunk):
    """the full 32-bit hashes of candidates chunk * CHUNK + 1 .. (chunk + 1) * CHUNK (any cap masks them)"""
    vs = range(chunk * CHUNK + 1, (chunk + 1) * CHUNK + 1)
    return join_hash([list(c) for c in zip(*(candidate(v, w, last_column_only) for v in vs))])


@functools.lru_cache(maxsize=None)
def keys_at(home_slot, cap, count, w=1, last_column_only=False):
    """the first `count` candidates (distinct by construction) whose home in a table of `cap` slots is home_slot"""
    assert 0 <= home_slot < cap and cap & (cap - 1) == 0
    out = []
    for chunk in range(-(-CEILING // CHUNK)):
        hit = np.nonzero((_hashes(w, last_column_only, chunk) & np.uint32(cap - 1)) == home_slot)[0]
        out += [candidate(chunk * CHUNK + 1 + int(j), w, last_column_only) for j in hit[:count - len(out)]]
        if len(out) == count:
            return tuple(out)
    raise AssertionError(f"{count} keys at home {home_slot} of {cap}: not among {CEILING} candidates")


# ---------------------------------------------------------------------------------------------------- the families
HIT, DEAD, MISS_HOME, MISS_INSIDE, MISS_ELSEWHERE, MISS_COLUMN, ABSENT_FULL = (
    "hit", "dead", "miss behind the whole chain", "miss from inside the cluster", "miss at an empty home",
    "miss that differs in one column", "absent from a full table")


class Family:
    """One constructed input.  keys: every tuple that occurs; assign[t]: the key of table row t; cells[t], labels[t]: the key
    of probe cell t and what the construction says of it; chain: the slots the build must occupy; payload: two more table
    columns for the fetch.  Only the table rows and the cells below `rows` take part."""

    def __init__(self, name, T, rows, cap, w, keys, assign, cells, labels, chain, seed):
        assert len(assign) == len(cells) == len(labels) == T and 1 <= rows <= T and len(set(keys)) == len(keys)
        self.name, self.T, self.rows, self.cap, self.w = name, T, rows, cap, w
        self.keys, self.assign, self.cells, self.labels, self.chain = list(keys), list(assign), list(cells), list(labels), set(chain)
        rnd = random.Random(seed ^ 0x5EED)
        self.payload = [[rnd.randrange(R) for _ in range(T)] for _ in range(2)]
        self.first_row = {}
        for t in range(rows):
            self.first_row.setdefault(assign[t], t)

    def columns(self, ids):
        return [[self.keys[k][c] for k in ids] for c in range(self.w)]

    @property
    def table(self):
        return self.columns(self.assign)

    @property
    def probes(self):
        return self.columns(self.cells)

    def tuples(self):
        """the table rows below `rows` as tuples"""
        return [self.keys[k] for k in self.assign[:self.rows]]

    def selector(self):
        """a selector column: off on every cell that holds an absent key behind the whole chain and on every fifth cell, on with
        1, r - 1 or 2^200 elsewhere"""
        on = (1, R - 1, 1 << 200)
        return [0 if self.labels[t] == MISS_HOME or t % 5 == 4 else on[t % 3] for t in range(self.T)]

    def expect(self, n_cells, sel=None):
        """(counters, missing, first missing cell or None, overrun) over cells [0, n_cells) from the construction alone"""
        cnt, miss, overrun = [0] * self.T, [], 0
        for t in range(n_cells):
            if sel is not None and sel[t] % R == 0:
                continue
            if self.labels[t] == ABSENT_FULL:
                overrun = 1
            elif self.cells[t] in self.first_row:
                cnt[self.first_row[self.cells[t]]] += 1
            else:
                miss.append(t)
        return cnt, len(miss), (miss[0] if miss else None), overrun


def _cells(T, must, rnd):
    """T cells: every (key, label) of `must` at least once, the rest drawn from them, in a seeded order"""
    assert len(must) <= T, (len(must), T)
    picked = list(must) + [must[rnd.randrange(len(must))] for _ in range(T - len(must))]
    rnd.shuffle(picked)
    return [k for k, _ in picked], [lab for _, lab in picked]


def _absent(keys, cap, chain, homes):
    """(key id, label) of one absent probe per slot of `homes` (none of them the home of a table tuple), appended to `keys` and
    labelled by where its home lies"""
    out = []
    for h in sorted({h % cap for h in homes}):
        k = keys_at(h, cap, 1, len(keys[0]))[0]
        assert k not in keys
        keys.append(k)
        out.append((len(keys) - 1, MISS_INSIDE if h in chain else MISS_ELSEWHERE))
    return out


def one_home(T, cap, D, m, seed=1):
    """D distinct tuples, all with home cap - 1, each repeated m times in a seeded shuffle of the T = D m rows: the chain
    {cap - 1, 0, .., D - 2}.  Probes: every tuple (so a hit at every depth), three absent tuples with home cap - 1 (a miss behind D
    occupied slots, through the wrap), absent tuples with homes 0, D // 2 and D - 2 (inside the cluster), D - 1 and cap - 2 (empty)"""
    assert D * m == T and 2 <= D < cap
    rnd = random.Random(seed)
    keys = list(keys_at(cap - 1, cap, D + 3))
    chain = {(cap - 1 + d) % cap for d in range(D)}
    assign = [k for k in range(D) for _ in range(m)]
    rnd.shuffle(assign)
    must = [(k, HIT) for k in range(D)] + [(D + a, MISS_HOME) for a in range(3)]
    must += _absent(keys, cap, chain, ({0, D // 2, D - 2} & chain) | {D - 1, cap - 2})
    cells, labels = _cells(T, must, rnd)
    return Family(f"one_home T={T} cap={cap} D={D}", T, T, cap, 1, keys, assign, cells, labels, chain, seed)


def staircase(T, cap, k, seed=2):
    """two tuples at each of the homes h, h + 1, .., h + k - 1 with h = cap - k // 2, so that every group is displaced by the groups
    before it and the cluster {h, .., h + 2 k - 1} wraps.  Probes: every tuple, one absent tuple per home (it walks to the end of
    the cluster), absent tuples at the empty slots on both sides"""
    assert T % (2 * k) == 0 and 2 * k + 2 <= cap
    rnd = random.Random(seed)
    h0 = cap - k // 2
    keys, must = [], []
    for i in range(k):
        keys += keys_at((h0 + i) % cap, cap, 3)[:2]
    chain = {(h0 + d) % cap for d in range(2 * k)}
    for i in range(k):
        keys.append(keys_at((h0 + i) % cap, cap, 3)[2])
        must.append((len(keys) - 1, MISS_INSIDE))
    must += [(j, HIT) for j in range(2 * k)]
    must += _absent(keys, cap, chain, [h0 + 2 * k, h0 - 1])
    assign = [j for j in range(2 * k) for _ in range(T // (2 * k))]
    rnd.shuffle(assign)
    cells, labels = _cells(T, must, rnd)
    return Family(f"staircase T={T} cap={cap} k={k}", T, T, cap, 1, keys, assign, cells, labels, chain, seed)


def last_column(T, cap, D, m, seed=3):
    """w = 3, D tuples with home cap - 1 that differ in column 2 only.  Probes: every tuple; three tuples equal in columns 0 and 1,
    absent in column 2, with home cap - 1 (every slot of the chain is compared down to the last column) and two with other homes;
    tuples that equal a table row in columns 1 and 2 and differ in column 0"""
    assert D * m == T and 2 <= D < cap
    rnd = random.Random(seed)
    keys = list(keys_at(cap - 1, cap, D + 3, 3, True))
    chain = {(cap - 1 + d) % cap for d in range(D)}
    must = [(k, HIT) for k in range(D)] + [(D + a, MISS_HOME) for a in range(3)]
    for h in (D // 2, D - 1):
        keys.append(keys_at(h, cap, 1, 3, True)[0])
        must.append((len(keys) - 1, MISS_INSIDE if h in chain else MISS_ELSEWHERE))
    for j in (0, D - 1):
        keys.append((keys[j][0] + 1,) + keys[j][1:])
        must.append((len(keys) - 1, MISS_COLUMN))
    assign = [k for k in range(D) for _ in range(m)]
    rnd.shuffle(assign)
    cells, labels = _cells(T, must, rnd)
    return Family(f"last_column T={T} cap={cap} D={D}", T, T, cap, 3, keys, assign, cells, labels, chain, seed)


def rows_cut(T, rows, cap, seed=4):
    """The _rows build: only the table rows and the cells below `rows` take part.  All tuples have home cap - 1.  `dead` tuples
    have every copy at or behind `rows` (they must miss, behind the whole chain); `both` tuples have two copies below and one
    behind; `live` tuples lie below only.  The chain holds the live and the both tuples.  The cells behind `rows` hold keys that
    would hit and keys that would miss: neither may show."""
    above = T - rows
    n_dead = max(1, above // 4)
    n_both = above - 2 * n_dead
    n_live, odd = divmod(rows - 2 * n_both, 2)
    assert above >= 3 and n_both >= 1 and n_live >= 1
    rnd = random.Random(seed)
    D = n_live + n_both
    keys = list(keys_at(cap - 1, cap, D + n_dead + 3))
    live, both = list(range(n_live)), list(range(n_live, D))
    dead, absent = list(range(D, D + n_dead)), list(range(D + n_dead, D + n_dead + 3))
    below = live * 2 + both * 2 + live[:odd]
    behind = both + dead * 2
    rnd.shuffle(below)
    rnd.shuffle(behind)
    assert len(below) == rows and len(behind) == above
    chain = {(cap - 1 + d) % cap for d in range(D)}
    must = [(k, HIT) for k in live + both] + [(k, DEAD) for k in dead] + [(k, MISS_HOME) for k in absent]
    must += _absent(keys, cap, chain, [0, D - 2, D - 1, cap - 2])
    cells, labels = _cells(rows, must, rnd)
    tail = [must[rnd.randrange(len(must))] for _ in range(above)]
    cells += [k for k, _ in tail]
    labels += [lab for _, lab in tail]
    return Family(f"rows_cut T={T} rows={rows} cap={cap}", T, rows, cap, 1, keys, below + behind, cells, labels, chain, seed)


def full(D, seed=5):
    """cap = rows = T = D distinct tuples (load 1), for the hook only: every slot is occupied, every table tuple is a hit, and an
    absent tuple finds no empty slot -- its walk ends at the bound of cap steps, raises the overrun word and counts no miss"""
    assert D >= 4 and D & (D - 1) == 0
    rnd = random.Random(seed)
    keys = [candidate(v, 1) for v in range(1, D + 5)]
    assign = list(range(D))
    rnd.shuffle(assign)
    must = [(k, HIT) for k in range(D - 4)] + [(D + a, ABSENT_FULL) for a in range(4)]
    cells, labels = _cells(D, must, rnd)
    return Family(f"full D={D}", D, D, D, 1, keys, assign, cells, labels, set(range(D)), seed)


# ---------------------------------------------------------------------------------------------------- the shapes that run
# T = 2^5 (part of one workgroup), 2^8 (one workgroup), 2^10 (four workgroups: one cluster holds rows of all four); the hook runs
# at the builders' cap = 2 T and, once, at cap = T; rows_cut at a `rows` that is no multiple of 64.  The end-to-end calls take the
# same families at cap = 2 T (the one capacity the builders use), rows_cut with T - rows inside the builders' 32 blinding rows.
HOOK_SHAPES = (("one_home", (32, 64, 8, 4)), ("one_home", (32, 32, 16, 2)), ("one_home", (256, 512, 64, 4)),
               ("one_home", (1024, 2048, 512, 2)), ("staircase", (32, 64, 4)), ("staircase", (256, 512, 16)),
               ("staircase", (1024, 2048, 32)), ("last_column", (32, 64, 8, 4)), ("last_column", (256, 512, 64, 4)),
               ("last_column", (1024, 2048, 64, 16)), ("rows_cut", (512, 300, 1024)), ("full", (32,)), ("full", (256,)),
               ("full", (1024,)))
E2E_SHAPES = (("one_home", (32, 64, 8, 4)), ("one_home", (256, 512, 64, 4)), ("one_home", (1024, 2048, 512, 2)),
              ("last_column", (256, 512, 64, 4)), ("rows_cut", (512, 485, 1024)))
BUILDERS = {"one_home": one_home, "staircase": staircase, "last_column": last_column, "rows_cut": rows_cut, "full": full}


@functools.lru_cache(maxsize=None)
def family(name, args):
    """the family of one shape, built once per process (the key search is cached with it)"""
    return BUILDERS[name](*args)


def shape_id(shape):
    return shape[0] + "-" + "-".join(str(a) for a in shape[1])
