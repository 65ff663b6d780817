"""Reference model for MSMs over repeated, opposite and infinite points (no GPU; used by tests/test_msm_degenerate_cpu.py
and tests/test_gpu_msm_degenerate.py).

Every test point is a multiple [k_j]G whose discrete log k_j the test knows (k = 0 stands for infinity), so the expected
result of any MSM is ONE fixed-base multiplication of the oracle, [sum s_j k_j mod r]G, at any size, and every bucket, carry
and tree node of the Pippenger pipeline is a known integer mod r.  The model below restates, in Python integers, the parts
of the pipeline that decide WHICH kernel runs and WHICH additions are exceptional (equal, opposite or infinite operands):

  window layout      spec_window / choose_window             zkp_subnet_amd/csrc/srs.hip
  signed digits      signed_digit                            zkp_subnet_amd/csrc/msm_sort.hip
  chunking           pick_chunk, KZG_MIN_CHUNK               zkp_subnet_amd/csrc/pipeline.hip
  carry fold         launch_fold_step / launch_fold_heads /
                     msm_fold_bucket_ok                      zkp_subnet_amd/csrc/msm_accumulate.hip
  bucket tree        run_tree                                zkp_subnet_amd/csrc/pipeline.hip
                     launch_msm_tree_level, msm_tree_level2_ok,
                     the merge rule at the head of           zkp_subnet_amd/csrc/msm_tree.hip

The order of the entries INSIDE a bucket run is the sort's business and is not modelled: the facts about the accumulate
are those that hold for every order (a run of n copies of one point doubles at its second entry whatever the order)."""
import functools
import random
from collections import namedtuple

import numpy as np

from oracle import bls12_381 as o
from oracle import cpu as oc

R = o.R

# ------------------------------------------------------------------ thresholds that decide the kernel form
KZG_TREE_WIDE_MIN = 32768      # msm_tree.hip: more operations than this in a level -> k_msm_tree_level (one lane each)
LP_MAX_OPS = 3072              # fp_lp.hip.h: up to this many -> one wave per operation (k_msm_tree_level_lp / level2_lp)
KZG_FOLD_COOP_MAX = 65536      # msm_accumulate.hip: more chunks than this -> k_fold_step / k_fold_heads (one lane per carry)
KZG_FOLD_LP_MAX = LP_MAX_OPS   # msm_accumulate.hip: nchunks / 2d up to this -> k_fold_step_lp
KZG_FOLD_BUCKET_MAX = 4096     # msm_accumulate.hip: k_fold_bucket_lp up to this many buckets ...
KZG_FOLD_BUCKET_RUN = 24       # ... and this many carries in the longest run
KZG_MIN_CHUNK = 6              # pipeline.hip
ACC_LANES = 131072             # pipeline.hip: pick_chunk's `lanes`


def classify(ops):
    """The kernel form launch_msm_tree_level picks for a level of `ops` additions."""
    if ops > KZG_TREE_WIDE_MIN:
        return "wide"
    return "lp" if ops <= LP_MAX_OPS else "coop"


# ------------------------------------------------------------------ point sources with known discrete logs
POOL_LOGS = (1, 1, R - 1, 0, 5, R - 5, 2)          # G twice, -G, infinity, 5G, -5G, 2G
TAUS = {"one": 1,                                   # every point is G
        "minus_one": R - 1,                         # G, -G, G, -G, ...
        "zero": 0,                                  # G followed by infinities
        "fourth_root": pow(7, (R - 1) // 4, R)}     # four points, repeating (tau^2 = -1)


def record(k):
    """The 96-byte setup-file record of [k]G (96 zero bytes for k = 0)."""
    k %= R
    return o.g1_to_be96(o.g1_mul(o.G1, k) if k else None)


POOL_RECORDS = tuple(record(k) for k in POOL_LOGS)


def pool_srs(n, seed, arranged=False):
    """(records, logs) of n points drawn from the pool in seeded random order.  arranged: the first quarter is a block of
    infinities, the second quarter a block of the one point 5G, the rest random."""
    rnd = random.Random(seed)
    idx = [rnd.randrange(len(POOL_LOGS)) for _ in range(n)]
    if arranged:
        q = n // 4
        idx[:q] = [3] * q
        idx[q:2 * q] = [4] * q
    return b"".join(POOL_RECORDS[i] for i in idx), [POOL_LOGS[i] for i in idx]


def tau_logs(tx, n):
    """Logs of the synthetic SRS [tau^j]G, j < n (0^0 = 1: the first point of tau = 0 is G)."""
    out, v = [], 1
    for _ in range(n):
        out.append(v)
        v = v * tx % R
    return out


def expected(scalars, logs):
    """48-byte compressed MSM result: one fixed-base multiplication, no MSM."""
    return oc.g1_mul_gen((sum(s * k for s, k in zip(scalars, logs)) % R).to_bytes(32, "big"))


# ------------------------------------------------------------------ window layout and digits
def choose_window(lg):
    for top, c in ((9, 8), (11, 10), (13, 12), (15, 14), (19, 16), (22, 20), (25, 22)):
        if lg <= top:
            return c
    return 24


def window_offsets(lg, window=0):
    """Bit offset of every window plus the closing 256, as spec_window lays them out (what eng.window_offsets reports)."""
    c = window or choose_window(lg)
    nwin = (256 + c - 1) // c
    base, extra = divmod(256, nwin)
    offs, off = [], 0
    for w in range(nwin):
        offs.append(off)
        off += base + (1 if w < extra else 0)
    return offs + [256]


def nbuckets_of(offsets):
    return 1 << (max(b - a for a, b in zip(offsets, offsets[1:])) - 1)


def digits(s, offsets):
    """Signed digits of scalar s, one per window (0 = dropped): d = bits + carry, negative when d > 2^(c_w - 1) with
    magnitude 2^c_w - d and a carry into the next window.  The bucket index of a digit is |digit| - 1."""
    out, carry = [], 0
    for lo, hi in zip(offsets, offsets[1:]):
        c = hi - lo
        d = ((s >> lo) & ((1 << c) - 1)) + carry
        carry = int(d > (1 << (c - 1)))
        out.append(d - (1 << c) if carry else d)
    assert carry == 0, "a canonical scalar (< r < 2^255) leaves no carry behind its top window"
    return out


def digit_array(scalars, offsets):
    """digits() of many scalars at once: int64 array [n, nwin].  scalars: integers, or their big-endian bytes as an
    [n, 32] uint8 array."""
    raw = scalars if isinstance(scalars, np.ndarray) else \
        np.frombuffer(o.fr_to_be32(scalars), dtype=np.uint8).reshape(len(scalars), 32)
    limbs = np.ascontiguousarray(raw[:, ::-1]).view("<u8")                             # limbs[:, i] = bits 64 i .. 64 i + 63
    limbs = np.concatenate([limbs, np.zeros((len(raw), 1), dtype=np.uint64)], axis=1)
    out = np.empty((len(raw), len(offsets) - 1), dtype=np.int64)
    carry = np.zeros(len(raw), dtype=np.int64)
    for w, (lo, hi) in enumerate(zip(offsets, offsets[1:])):
        c, i, sh = hi - lo, lo >> 6, np.uint64(lo & 63)
        assert c <= 32
        v = limbs[:, i] >> sh
        if lo & 63:
            v = v | (limbs[:, i + 1] << np.uint64(64 - (lo & 63)))
        d = (v & np.uint64((1 << c) - 1)).astype(np.int64) + carry
        carry = (d > (1 << (c - 1))).astype(np.int64)
        out[:, w] = d - carry * (1 << c)
    assert not carry.any()
    return out


# ------------------------------------------------------------------ buckets
Buckets = namedtuple("Buckets", "logs kinds")
# logs[b]: the bucket's sum as an integer mod r; kinds[b]: {log of the (signed, window-shifted) point an entry adds: how
# many entries add it}, finite points only, for the buckets that have any


def _ids(values):
    distinct = sorted(set(values))
    index = {v: i for i, v in enumerate(distinct)}
    return distinct, np.fromiter((index[v] for v in values), dtype=np.int64, count=len(values))


def bucket_model(scalars, logs, offsets):
    """The value and the composition of every bucket.  Linear in the entries for many different scalars (one histogram
    per point value, sign and window), in the (scalar, point) pairs that occur for few."""
    return _bucket_model(scalars, _ids(scalars) if len(set(scalars)) <= 64 else None, _ids(logs), offsets)


def _bucket_model(scalars, compact, log_ids, offsets):
    nb = nbuckets_of(offsets)
    values, ids = log_ids
    assert len(values) <= 16, "the point sources of this module have a handful of different points"
    blog, kinds = [0] * nb, {}

    def put(b, k, sign, w, cnt):
        if k:
            v = ((k if sign > 0 else R - k) << offsets[w]) % R
            blog[b] = (blog[b] + v * cnt) % R
            mine = kinds.setdefault(b, {})
            mine[v] = mine.get(v, 0) + cnt

    if compact:
        svals, sid = compact
        pairs = np.bincount(sid * len(values) + ids, minlength=len(svals) * len(values)).reshape(len(svals), len(values))
        for si, s in enumerate(svals):
            for w, d in enumerate(digits(s, offsets)):
                for ki in np.flatnonzero(pairs[si]) if d else ():
                    put(abs(d) - 1, values[ki], d, w, int(pairs[si, ki]))
        return Buckets(blog, kinds)
    D = digit_array(scalars, offsets)
    for w in range(len(offsets) - 1):
        col = D[:, w]
        mag = np.abs(col)
        for ki, k in enumerate(values):
            for sign in (1, -1):
                cnt = np.bincount(mag[(ids == ki) & (col * sign > 0)] - 1, minlength=nb)
                for b in np.flatnonzero(cnt):
                    put(int(b), k, sign, w, int(cnt[b]))
    return Buckets(blog, kinds)


def bucket_logs(scalars, logs, offsets):
    """One integer mod r per bucket: sum of +-k_j 2^off_w over the entries (j, w) whose digit has the bucket's magnitude."""
    return bucket_model(scalars, logs, offsets).logs


# ------------------------------------------------------------------ accumulate and carry fold
def pick_chunk(entries):
    if entries <= ACC_LANES * 16:
        return max(KZG_MIN_CHUNK, (entries + ACC_LANES // 2 - 1) // (ACC_LANES // 2))
    rounds = (entries + ACC_LANES * 512 - 1) // (ACC_LANES * 512)
    return (entries + ACC_LANES * rounds - 1) // (ACC_LANES * rounds)


def fold_plan(counts, inf_counts, entries):
    """What the host launches behind the accumulate, from the entries per bucket alone (counts; inf_counts: those whose
    table row is infinity; entries: the host's bound n * nwin).  Returns a dict: chunk, nchunks, runs (carries per bucket),
    max_run (the fold-depth word: longest carry run, 0 when none exceeds one carry), kernels (one name per launch),
    acc_inf_entries, acc_inf_runs (non-empty runs of infinite rows only), fold_inf_carries (carries that are certainly
    infinity: a finite entry makes at most one carry of its run finite)."""
    chunk = pick_chunk(entries)
    nchunks = (entries + chunk - 1) // chunk
    ends = np.cumsum(counts)
    starts = ends - counts
    runs = np.where(counts > 0, (ends - 1) // chunk - starts // chunk, 0)
    max_run = int(runs.max()) if int(runs.max()) > 1 else 0
    if len(counts) <= KZG_FOLD_BUCKET_MAX and max_run <= KZG_FOLD_BUCKET_RUN:
        kernels = ["k_fold_bucket_lp"]
    else:
        kernels, d = [], 1
        while d < max_run:
            kernels.append("k_fold_step" if nchunks > KZG_FOLD_COOP_MAX else
                           "k_fold_step_lp" if nchunks // (2 * d) <= KZG_FOLD_LP_MAX else "k_fold_step_coop")
            d <<= 1
        kernels.append("k_fold_heads" if nchunks > KZG_FOLD_COOP_MAX else "k_fold_heads_coop")
    return {"chunk": chunk, "nchunks": nchunks, "runs": runs, "ends": ends, "max_run": max_run, "kernels": kernels,
            "acc_inf_entries": int(inf_counts.sum()), "acc_inf_runs": int(((counts > 0) & (inf_counts == counts)).sum()),
            "fold_inf_carries": int(np.maximum(0, runs - (counts - inf_counts)).sum())}


def run_census(kinds, counts, inf_counts, fold):
    """What is certain about the runs whatever order the sort leaves their entries in.  same: runs of >= 2 entries that
    all add the SAME finite point (the second entry doubles); pm: runs of >= 2 entries that all add +-one finite point (the
    second entry doubles or cancels); same_pairs: pairs (i, i + 1) of the first fold step whose two carries are full chunks
    of a `same` run (the step doubles, and so does every later step of that run, whose operands are again equal)."""
    same = pm = same_pairs = 0
    for b, mine in kinds.items():
        if counts[b] < 2 or inf_counts[b]:
            continue
        if len(mine) == 1:
            same += 1
            # carries sit at chunks t0 + 1 .. t1; all but the last are full chunks of this run, the last when the run ends
            # on a chunk boundary
            same_pairs += (int(fold["runs"][b]) - (0 if int(fold["ends"][b]) % fold["chunk"] == 0 else 1)) // 2
        if len(mine) == 1 or (len(mine) == 2 and sum(mine) % R == 0):
            pm += 1
    return {"same": same, "pm": pm, "same_pairs": same_pairs}


# ------------------------------------------------------------------ bucket tree
def merge_class(a, b):
    """None for an ordinary addition, else which exceptional path it takes."""
    if a == 0 or b == 0:
        return "inf"
    if a == b:
        return "dbl"
    return "cancel" if (a + b) % R == 0 else None


def tree_plan(nbuckets, stop=1):
    """The launches of run_tree from the bucket count alone: [{"level", "ops", "form" (classify(ops)), "paired" (first or
    second half of a k_msm_tree_level2_lp launch: "first" / "second" / None)}]."""
    out, n_in, level, pair_left = [], nbuckets, 0, 0
    while n_in > stop:
        ops = (n_in >> 1) * (level + 1)
        if pair_left:
            paired, pair_left = "second", 0
        elif (n_in >> 2) >= stop and n_in >= 4 and ops <= LP_MAX_OPS:      # run_tree + msm_tree_level2_ok
            paired, pair_left = "first", 1
        else:
            paired = None
        out.append(dict(level=level, ops=ops, form=classify(ops), paired=paired))
        n_in, level = n_in >> 1, level + 1
    return out


def tree_census(blogs, stop=1):
    """Follows the merge rule of msm_tree.hip over adjacent pairs until `stop` nodes are left.  A level-L node holds
    [P, T_0 .. T_{L-1}]; merging left and right: P = P_l + P_r, T_k = T_k_l + T_k_r for k < L (L + 1 additions), T_L = P_r
    (no addition).  Returns (levels, roots): levels[L] = {"level", "ops", "form" (classify(ops)), "paired" (the level is
    the first or second half of a k_msm_tree_level2_lp launch: "first" / "second" / None), "dbl", "cancel", "inf"} and
    roots = [[P, T_0 .. T_{nbits-1}] per root]."""
    n_in, levels = len(blogs), []
    nodes = {i: [v] for i, v in enumerate(blogs) if v}          # nodes with a finite component; every other is all infinity
    for plan in tree_plan(n_in, stop):
        level = plan["level"]
        parents = {i >> 1 for i in nodes}
        tally = {"dbl": 0, "cancel": 0, "inf": ((n_in >> 1) - len(parents)) * (level + 1)}
        zero, merged = [0] * (level + 1), {}
        for m in parents:
            lt, rt = nodes.get(2 * m, zero), nodes.get(2 * m + 1, zero)
            for a, b in zip(lt, rt):
                cls = merge_class(a, b)
                if cls:
                    tally[cls] += 1
            node = [(a + b) % R for a, b in zip(lt, rt)] + [rt[0]]
            if any(node):
                merged[m] = node
        levels.append(dict(plan, **tally))
        nodes, n_in = merged, n_in >> 1
    return levels, [nodes.get(m, [0] * (len(levels) + 1)) for m in range(n_in)]


def root_value(root):
    """P + sum 2^i T_i: the MSM's log, as k_msm_final_dbl_lp / k_msm_final_sum_lp combine a root."""
    return (root[0] + sum(t << i for i, t in enumerate(root[1:]))) % R


# ------------------------------------------------------------------ scalar families
EDGE_POOL = [0, 1, 2, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, (1 << 254), (1 << 255) % R] + \
            [(1 << k) - 1 for k in (8, 16, 20, 28, 32, 64, 128, 200)] + [(1 << k) for k in (7, 15, 19, 27, 31, 63, 127)]
# (the pool of tests/fuzz_gpu.py's "edge" kind)


def equal_scalar(offsets, seed=1):
    """One scalar whose digits are non-zero and differ in magnitude from window to window (so that every bucket run of
    the all-equal family is n copies of ONE table row); seeded search, positive and negative digits alike."""
    for t in range(10000):
        s = random.Random(seed * 10007 + t).randrange(1, R)
        mags = [abs(d) for d in digits(s, offsets)]
        if 0 not in mags and len(set(mags)) == len(mags):
            return s
    raise AssertionError("no scalar with pairwise different digits found")


def paired_scalars(offsets, seed=2):
    """(A, B): in every window w the digits of A and B are 2 m_w + 1 and 2 m_w + 2 (positive, no carries), the m_w all
    different: over n/2 copies of one point each, buckets 2 m_w and 2 m_w + 1 come out equal (or opposite, over P and -P)."""
    rnd = random.Random(seed)
    nwin = len(offsets) - 1
    top = (R >> offsets[nwin - 1]) - 1                       # the top window's digit must keep the scalar below r
    caps = [(1 << (offsets[w + 1] - offsets[w] - 1)) for w in range(nwin)]
    caps[-1] = min(caps[-1], top)
    ms, used = [], set()
    for w in range(nwin):
        while True:
            m = rnd.randrange((caps[w] - 2) // 2 + 1)        # 2 m + 2 <= cap
            if m not in used:
                break
        used.add(m)
        ms.append(m)
    a = sum((2 * m + 1) << offsets[w] for w, m in enumerate(ms))
    b = sum((2 * m + 2) << offsets[w] for w, m in enumerate(ms))
    assert a < R and b < R
    return a, b


def family(name, n, offsets, seed=0):
    """n scalars (integers below r) of one family: "uniform", "equal", "paired", "edge".  Cached: treat as read-only."""
    return _family(name, n, tuple(offsets), seed)


def family_raw(name, n, offsets, seed=0):
    """The same scalars as their 32-byte big-endian wire form, an [n, 32] uint8 array (cached: read-only)."""
    return _family_raw(name, n, tuple(offsets), seed)


@functools.lru_cache(maxsize=None)
def _family_compact(name, n, offsets, seed):
    """(the different scalars, which of them each of the n scalars is) of the families that have few"""
    if name == "equal":
        values, idx = [equal_scalar(offsets, seed + 1)], np.zeros(n, dtype=np.int64)
    elif name == "paired":
        values, idx = list(paired_scalars(offsets, seed + 2)), np.arange(n, dtype=np.int64) % 2
    elif name == "edge":
        rnd = random.Random(3000 + seed)
        values, idx = EDGE_POOL, np.array([rnd.randrange(len(EDGE_POOL)) for _ in range(n)], dtype=np.int64)
    else:
        raise ValueError(name)
    return values, idx


@functools.lru_cache(maxsize=None)
def _family_raw(name, n, offsets, seed):
    if name == "uniform":
        raw = np.random.default_rng(1000 + seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
        raw[:, 0] &= 0x3F                                     # < 2^254 < r: canonical
        return raw
    values, idx = _family_compact(name, n, offsets, seed)
    return np.frombuffer(o.fr_to_be32(values), dtype=np.uint8).reshape(len(values), 32)[idx]


@functools.lru_cache(maxsize=None)
def _family(name, n, offsets, seed):
    return o.fr_from_be32(_family_raw(name, n, offsets, seed).tobytes())


# ------------------------------------------------------------------ the cases of the GPU module and their preconditions
# (lg, window): what the shape is there to reach -- derivations in the docstring of tests/test_gpu_msm_degenerate.py
SHAPES = ((10, 0), (12, 0), (12, 16), (11, 18), (17, 13))
SRS_KINDS = ("one", "minus_one", "zero", "fourth_root", "pool", "pool_arranged")
FAMILIES = ("equal", "uniform", "edge", "paired")


@functools.lru_cache(maxsize=None)
def srs_logs(kind, n, want_records=False):
    """Logs of the n points of SRS `kind` (and the setup records of the two pool kinds).  Cached: treat as read-only."""
    if kind in TAUS:
        return tau_logs(TAUS[kind], n), None
    rec, logs = pool_srs(n, seed=n, arranged=kind == "pool_arranged")
    return logs, rec if want_records else None


@functools.lru_cache(maxsize=None)
def _srs_ids(kind, n):
    return _ids(srs_logs(kind, n)[0])


def cases_of(lg, window):
    """The (srs kind, family) pairs run at one shape: the four special taus with every family (no `paired` at 2^17: its
    tree has lane-parallel levels only, which 2^10 covers), the pool (up to 2^12 points; a 2^17-point file is not loaded)
    with uniform and equal scalars."""
    out = [(k, f) for k in TAUS for f in FAMILIES if f != "paired" or lg != 17]
    if lg <= 12:
        out += [(k, f) for k in ("pool", "pool_arranged") for f in ("uniform", "equal")]
    return out


class Case:
    """One MSM of the GPU module: n scalars of a family over points with the logs `logs`, at the window layout of (lg,
    window).  Everything beyond the inputs is computed when a precondition (or the test) first reads it, so that a case
    pays only for what it asserts: the entries per bucket and what follows from them (fold) cost a few array passes at any
    size; the value of every bucket (buckets), the runs' composition (runs) and the tree census (levels, roots) are linear
    in the entries in Python and are read by the cases with few different scalars only."""

    def __init__(self, lg, window, kind, fam, logs=None, n=None):
        self.lg, self.window, self.kind, self.family = lg, window, kind, fam
        self.n = n or 1 << lg
        self.offsets = window_offsets(lg, window)
        self.nwin, self.nbuckets = len(self.offsets) - 1, nbuckets_of(self.offsets)
        self.logs = srs_logs(kind, 1 << lg)[0][:self.n] if logs is None else logs
        assert len(self.logs) == self.n
        self.raw = family_raw(fam, self.n, self.offsets, seed=lg)
        self.compact = None if fam == "uniform" else _family_compact(fam, self.n, tuple(self.offsets), lg)
        self._log_ids = _srs_ids(kind, 1 << lg) if logs is None and self.n == 1 << lg else _ids(self.logs)
        self.plan = tree_plan(self.nbuckets)

    @functools.cached_property
    def scalars(self):
        return family(self.family, self.n, self.offsets, seed=self.lg)

    @functools.cached_property
    def scalar_bytes(self):
        return self.raw.tobytes()

    @functools.cached_property
    def total(self):
        """sum s_j k_j mod r: per point value, the byte columns of its scalars are summed first"""
        values, ids = self._log_ids
        out = 0
        for ki, k in enumerate(values):
            cols = self.raw[ids == ki].sum(axis=0, dtype=np.int64) if k else ()
            out += k * sum(int(c) << (8 * (31 - i)) for i, c in enumerate(cols))
        return out % R

    @functools.cached_property
    def expected(self):
        return oc.g1_mul_gen(self.total.to_bytes(32, "big"))

    @functools.cached_property
    def _counts(self):
        values, ids = self._log_ids
        inf_rows = ids == values.index(0) if 0 in values else np.zeros(self.n, dtype=bool)
        if self.compact:                     # few different scalars: their digits, weighted by how often each occurs
            svals, sid = self.compact
            counts, inf = np.zeros(self.nbuckets, dtype=np.int64), np.zeros(self.nbuckets, dtype=np.int64)
            often, often_inf = np.bincount(sid, minlength=len(svals)), np.bincount(sid[inf_rows], minlength=len(svals))
            for si, s in enumerate(svals):
                for d in digits(s, self.offsets):
                    if d:
                        counts[abs(d) - 1] += often[si]
                        inf[abs(d) - 1] += often_inf[si]
            return counts, inf
        mag = np.abs(digit_array(self.raw, self.offsets))
        mag_inf = mag[inf_rows]
        return np.bincount(mag[mag > 0] - 1, minlength=self.nbuckets), \
            np.bincount(mag_inf[mag_inf > 0] - 1, minlength=self.nbuckets)

    @property
    def counts(self):
        return self._counts[0]

    @property
    def inf_counts(self):
        return self._counts[1]

    @functools.cached_property
    def fold(self):
        return fold_plan(self.counts, self.inf_counts, self.n * self.nwin)

    @functools.cached_property
    def empty_level0_merges(self):
        """level-0 merges with an EMPTY bucket: an infinite operand whatever the values are"""
        return int(((self.counts[0::2] == 0) | (self.counts[1::2] == 0)).sum())

    @functools.cached_property
    def buckets(self):
        return _bucket_model(self.raw, self.compact, self._log_ids, self.offsets)

    @functools.cached_property
    def runs(self):
        return run_census(self.buckets.kinds, self.counts, self.inf_counts, self.fold)

    @functools.cached_property
    def _census(self):
        return tree_census(self.buckets.logs)

    @property
    def levels(self):
        return self._census[0]

    @property
    def roots(self):
        return self._census[1]

    def exceptional(self, form=None, paired=None, classes=("dbl", "cancel", "inf")):
        return sum(x[c] for x in self.levels for c in classes
                   if form in (None, x["form"]) and paired in (None, x["paired"]))


def build_case(lg, window, kind, fam, logs=None, n=None):
    return Case(lg, window, kind, fam, logs, n)


def _digits_differ(c):
    mags = [abs(d) for d in digits(c.compact[0][0], c.offsets)]
    return 0 not in mags and len(set(mags)) == len(mags)


def _fold_12_0(c):
    k = c.fold["kernels"]
    return k[:2] == ["k_fold_step_coop"] * 2 and set(k[2:-1]) == {"k_fold_step_lp"} and k[-1] == "k_fold_heads_coop" and \
        14000 < c.fold["nchunks"] < 16000 and c.fold["chunk"] == 6


# name -> (what it says, the whole-number fact).  Facts marked [census] read the value of every bucket and tree node.
CHECKS = {
    "root": ("[census] the model's root P + sum 2^i T_i is sum s_j k_j", lambda c: root_value(c.roots[0]) == c.total),
    "tree_lp_only": ("tree: lane-parallel levels only, launched in pairs and once singly",
                     lambda c: {x["form"] for x in c.plan} == {"lp"} and
                     {x["paired"] for x in c.plan} == {"first", "second", None}),
    "pair_exceptional": ("[census] k_msm_tree_level2_lp: an exceptional first-half result (held in LDS) feeds the second "
                         "addition", lambda c: c.exceptional(paired="first") >= 1),
    "fold_bucket": ("fold is the one launch k_fold_bucket_lp", lambda c: c.fold["kernels"] == ["k_fold_bucket_lp"]),
    "fold_coop_lp": ("fold: about 15 000 chunks of 6; two cooperative steps, lane-parallel steps, cooperative heads",
                     _fold_12_0),
    "coop_level0_empty": ("tree: level 0 is cooperative and merges with empty buckets (an infinite operand)",
                          lambda c: c.plan[0]["form"] == "coop" and c.empty_level0_merges >= 1),
    "coop_exceptional": ("[census] tree: exceptional additions at cooperative levels",
                         lambda c: c.exceptional(form="coop") >= 1),
    "wide_levels": ("tree: 2^17 buckets, levels 0-2 wide", lambda c: c.nbuckets == 1 << 17 and
                    [x["form"] for x in c.plan[:4]] == ["wide"] * 3 + ["coop"]),
    "big_chunks": ("more than 2^21 entries in 131072 chunks",
                   lambda c: c.n * c.nwin > 1 << 21 and c.fold["nchunks"] == 131072),
    "fold_plain": ("fold: plain steps and heads", lambda c: len(c.fold["kernels"]) > 1 and
                   set(c.fold["kernels"][:-1]) == {"k_fold_step"} and c.fold["kernels"][-1] == "k_fold_heads"),
    "digits_differ": ("equal: the scalar's digits are non-zero and differ from window to window", _digits_differ),
    "runs_same": ("[census] accumulate: every run is n copies of one row (its second entry doubles)",
                  lambda c: c.runs["same"] == c.nwin),
    "fold_same": ("[census] fold: equal full-chunk carries (a doubling at every step)",
                  lambda c: c.fold["max_run"] > 1 and c.runs["same_pairs"] >= c.nwin),
    "runs_pm": ("[census] accumulate: every run is n/2 copies of P and n/2 of -P (its second entry doubles or cancels)",
                lambda c: c.runs["pm"] == c.nwin),
    "all_infinity": ("[census] every bucket, tree node and root component is infinity; the final doubles infinite T_l",
                     lambda c: c.n % 4 == 0 and not any(c.buckets.logs) and not any(c.roots[0]) and
                     c.exceptional(classes=("inf",)) == sum(x["ops"] for x in c.plan)),
    "level0_dbl": ("[census] paired: tree level 0 has one doubling per window", lambda c: c.levels[0]["dbl"] == c.nwin),
    "level0_cancel": ("[census] paired: tree level 0 has one cancellation per window",
                      lambda c: c.levels[0]["cancel"] == c.nwin),
    "wide_dbl": ("[census] a doubling at a wide level", lambda c: c.exceptional("wide", classes=("dbl",)) >= 1),
    "wide_cancel": ("[census] a cancellation at a wide level", lambda c: c.exceptional("wide", classes=("cancel",)) >= 1),
    "zero_rows": ("all entries but those of the first point are infinite table rows",
                  lambda c: 0 < c.fold["acc_inf_entries"] >= int(c.counts.sum()) - c.nwin),
    "inf_runs": ("runs of infinite rows only (their first entry included)", lambda c: c.fold["acc_inf_runs"] >= 1),
    "inf_carries": ("carries that are certainly infinity", lambda c: c.fold["fold_inf_carries"] >= 1),
    "pool_inf_rows": ("pool: at least n / 14 entries are infinite table rows",
                      lambda c: c.fold["acc_inf_entries"] >= c.n // 14),
    "pool_mixed_runs": ("pool: infinite and finite rows share every run",
                        lambda c: c.fold["acc_inf_entries"] > 0 and c.fold["acc_inf_runs"] == 0),
}
# what the SHAPE is there to reach: for every case at it ("*"), and for one family
BY_SHAPE = {
    (10, 0): {"*": ["tree_lp_only"], "uniform": ["fold_bucket"], "equal": ["pair_exceptional"],
              "edge": ["pair_exceptional"], "paired": ["pair_exceptional"]},
    (12, 0): {"equal": ["fold_coop_lp"]},
    (12, 16): {"uniform": ["coop_level0_empty"], "equal": ["coop_exceptional"], "edge": ["coop_exceptional"],
               "paired": ["coop_exceptional"]},
    (11, 18): {"*": ["wide_levels"]},
    (17, 13): {"*": ["big_chunks"], "equal": ["fold_plain"]},
}
# what the POINT SOURCE and the scalar FAMILY are there to produce ("*": any family); every family but `uniform` also
# checks the model's root ("root"), see names_for
BY_SOURCE = {
    ("one", "equal"): ["digits_differ", "runs_same", "fold_same"],
    ("minus_one", "equal"): ["digits_differ", "runs_pm", "all_infinity"],
    ("fourth_root", "equal"): ["digits_differ", "all_infinity"],
    ("zero", "equal"): ["digits_differ", "zero_rows", "inf_carries"],
    ("zero", "*"): ["zero_rows"],
    ("zero", "uniform"): ["inf_runs"],
    ("zero", "edge"): ["inf_runs"],
    ("zero", "paired"): ["inf_runs"],
    ("one", "paired"): ["level0_dbl"],
    ("minus_one", "paired"): ["level0_cancel"],
    ("pool", "*"): ["pool_inf_rows"],
    ("pool_arranged", "*"): ["pool_inf_rows"],
    ("pool", "equal"): ["digits_differ", "pool_mixed_runs"],
    ("pool_arranged", "equal"): ["digits_differ", "pool_mixed_runs"],
}
BY_SHAPE_AND_SOURCE = {((11, 18), "one", "paired"): ["wide_dbl"], ((11, 18), "minus_one", "paired"): ["wide_cancel"],
                       ((10, 0), "zero", "uniform"): ["inf_carries", "pair_exceptional"]}


def names_for(lg, window, kind, fam):
    shape = BY_SHAPE.get((lg, window), {})
    names = ([] if fam == "uniform" else ["root"]) + shape.get("*", []) + shape.get(fam, []) + \
        BY_SOURCE.get((kind, "*"), []) + BY_SOURCE.get((kind, fam), []) + \
        BY_SHAPE_AND_SOURCE.get(((lg, window), kind, fam), [])
    return list(dict.fromkeys(names))


def preconditions(case):
    """[(what, holds)]: the whole-number facts a case must show BEFORE it is worth a GPU call -- which kernels it reaches
    and which exceptional additions it is certain to contain (the tables above).  A case that stops meeting them fails."""
    return [(CHECKS[name][0], bool(CHECKS[name][1](case))) for name in names_for(case.lg, case.window, case.kind, case.family)]
