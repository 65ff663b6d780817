"""The device-built fetched columns (worker_commit_fetch's engine call) against the routes they replace or extend, interleaved on
the same box, for T in {2^16, 2^20} and three shapes:

  xor      two keys, one payload, two reads: c = a ^ b read from the resident table (a, b, a ^ b) of T rows
  unsort   one key, three payloads, one read: the columns of a permuted table back in the order of its row-number column
  index    one read by row index from a one-column table (no join)

The table and the input columns are committed once, outside the timing.

  fetch    commit_fetch over the resident sets: w_tab + n_reads max(n_keys, 1) forward transforms, the join's build, one fetch
           per read, n_out inverse transforms, one MSM pass of n_out scalar sets.  Nothing row-sized crosses the host link
  route a  what a caller does without it: the rows computed on the host from its copies with a Python dict (a list for the
           index shape), packed to 32-byte scalars, then commit_rows of the n_out rows in evaluation form
  route b  commit_rows of the same n_out (precomputed) rows alone, upload included: the floor of route a
  route c  commit_multiplicities over the same inputs and the table's key columns: the same transforms of the keys and the same
           join with no output rows (one MSM of the multiplicity row); none for the index shape, which has no join

Routes a, b and c run code this builder does not touch.  One JSON line per point with the ratios and the profiled stage split of
the new call, stamped with the library identity like bench.py's lines.

    python scripts/bench_fetch.py [--rounds 3] [--reps 3] [--host-reps 1] [--sizes 16,20]"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib.common import identity  # noqa: E402
from zkp_subnet_amd import HipEngine, _native  # noqa: E402

SHAPES = ["xor", "unsort", "index"]


def instance(shape, lg, rnd):
    """(input columns, table columns, n_reads, n_keys)"""
    T = 1 << lg
    if shape == "xor":
        h = lg // 2
        ta, tb = [q >> h for q in range(T)], [q & ((1 << h) - 1) for q in range(T)]
        ins = [[rnd.randrange(1 << (lg - h)) if c % 2 == 0 else rnd.randrange(1 << h) for _ in range(T)] for c in range(4)]
        return ins, [ta, tb, [x ^ y for x, y in zip(ta, tb)]], 2, 2
    if shape == "unsort":
        perm = list(range(T))
        rnd.shuffle(perm)
        return [list(range(T))], [perm] + [[rnd.getrandbits(64) for _ in range(T)] for _ in range(3)], 1, 1
    return [[rnd.randrange(T) for _ in range(T)]], [[rnd.getrandbits(64) for _ in range(T)]], 1, 0


def host_rows(ins, table, n_reads, n_keys):
    """the fetched rows on the host: a dict from key tuple to the smallest row (every cell hits in these instances)"""
    T = len(table[0])
    if n_keys == 0:
        return [[col[q] for q in ins[l]] for l in range(n_reads) for col in table]
    first = {}
    for q in range(T):
        first.setdefault(tuple(table[c][q] for c in range(n_keys)), q)
    out = []
    for l in range(n_reads):
        qs = [first[k] for k in zip(*ins[l * n_keys:(l + 1) * n_keys])]
        out += [[col[q] for q in qs] for col in table[n_keys:]]
    return out


def pack(row):
    return b"".join(v.to_bytes(32, "big") for v in row)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed sample of the device routes (the median is reported)")
    ap.add_argument("--host-reps", type=int, default=1, help="calls per timed sample of route a (seconds each at 2^20)")
    ap.add_argument("--sizes", default="16,20")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        eng = HipEngine(0)
        eng.gen_srs(0xFE7C + lg, 0xFACADE, lg, 0)
        for shape in SHAPES:
            rnd = random.Random(1000 * lg + len(shape))
            ins, table, n_reads, n_keys = instance(shape, lg, rnd)
            I = eng.commit_rows(0, [pack(c) for c in ins])
            TB = eng.commit_rows(0, [pack(c) for c in table])
            K = eng.commit_rows(0, [pack(c) for c in table[:n_keys]]) if n_keys else None
            rows = [pack(r) for r in host_rows(ins, table, n_reads, n_keys)]

            def device():
                s, missing, _ = eng.commit_fetch([I], [TB], n_reads, n_keys)
                s.release()
                assert missing == [0] * n_reads
                return s.commitments

            def route_a():
                s = eng.commit_rows(0, [pack(r) for r in host_rows(ins, table, n_reads, n_keys)])
                s.release()
                return s.commitments

            def route_b():
                s = eng.commit_rows(0, rows)
                s.release()
                return s.commitments

            def route_c():
                s, missing = eng.commit_multiplicities([I], [K], n_reads, n_keys)
                s.release()
                assert missing == 0

            def timed(f, reps):
                samples = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    f()
                    samples.append(time.perf_counter() - t0)
                return median(samples) * 1e3

            def stages(f):
                eng._chk(lib.kzg_set_profiling(eng._h, 1))
                try:
                    f()
                    tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
                    eng._chk(lib.kzg_get_timings(eng._h, tms, len(tms)))
                finally:
                    eng._chk(lib.kzg_set_profiling(eng._h, 0))
                return {n: round(v, 4) for n, v in zip(_native.TIMING_NAMES, tms) if v}

            assert device() == route_b()                # (also the warm-up: buffers, twiddles; route a commits the same rows)
            device()
            if K:
                route_c()
            td, ta, tb, tc = [], [], [], []
            for _ in range(a.rounds):                   # interleaved: the routes see the same clock and thermal state
                td.append(timed(device, a.reps))
                ta.append(timed(route_a, a.host_reps))
                tb.append(timed(route_b, a.reps))
                if K:
                    tc.append(timed(route_c, a.reps))
            md, ma, mb, mc = median(td), median(ta), median(tb), median(tc) if K else None
            print(json.dumps({"metric": "fetch", "T_log2": lg, "shape": shape, "n_reads": n_reads, "n_keys": n_keys,
                              "n_out": len(rows), "fetch_ms": round(md, 4), "route_a_ms": round(ma, 4), "route_b_ms": round(mb, 4),
                              "route_c_ms": None if mc is None else round(mc, 4),
                              "fetch_over_route_a": round(md / ma, 4), "fetch_over_route_b": round(md / mb, 3),
                              "fetch_over_route_c": None if mc is None else round(md / mc, 3),
                              "fetch_rounds_ms": [round(x, 4) for x in td], "route_a_rounds_ms": [round(x, 4) for x in ta],
                              "route_b_rounds_ms": [round(x, 4) for x in tb], "route_c_rounds_ms": [round(x, 4) for x in tc],
                              "fetch_stages_ms": stages(device), **ident}), flush=True)
            for s in (I, TB, K):
                if s is not None:
                    s.release()
        eng.close()


if __name__ == "__main__":
    main()
