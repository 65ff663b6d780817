"""The device-built sorted columns (worker_commit_sorted's engine call) against the route they replace, interleaved on the same
box, for T in {2^16, 2^20}, w in {1, 3} (n_keys = w, the call's default) and two kinds of keys: uniform in [0, r) and uniform
in [0, 2^16).  The source set is committed once, outside the timing.

  sorted   commit_sorted over the resident set: w forward transforms, the key pass, the radix passes that move something, w
           gathers and inverse transforms, one MSM pass of w scalar sets.  Nothing row-sized crosses the host link
  route a  what a caller does without it: a numpy lexsort of the host copy of the columns (each 256-bit key as four big-endian
           u64 words, the cheapest exact host sort found), the gather, then commit_rows of the w sorted rows in evaluation form
  route b  commit_rows of the same w (already sorted) rows alone: the floor, since those inverse transforms and that MSM are
           inside the new call too (its upload is not)

Routes a and b run code this builder does not touch.  One JSON line per point with both ratios and the profiled stage split of
the new call, stamped with the library identity like bench.py's lines.

    python scripts/bench_sorted.py [--rounds 3] [--reps 3] [--sizes 16,20]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib.common import identity  # noqa: E402
from zkp_subnet_amd import HipEngine, _native  # noqa: E402


def rand_col(T, seed, small):
    """T big-endian 32-byte scalars as a (T, 32) u8 array: uniform below 2^254 (< r), or uniform below 2^16"""
    raw = np.random.default_rng(seed).integers(0, 256, size=(T, 32), dtype=np.uint8)
    if small:
        raw[:, :30] = 0
    else:
        raw[:, 0] &= 0x3F
    return raw


def host_sort(cols):
    """the stable permutation by the columns' integers, column 0 most significant (np.lexsort: the LAST key is primary)"""
    keys = []
    for col in reversed(cols):
        words = col.view(">u8")                       # (T, 4), word 0 most significant
        keys += [words[:, j] for j in (3, 2, 1, 0)]
    return np.lexsort(keys)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed sample (the median sample is reported)")
    ap.add_argument("--sizes", default="16,20")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x5027 + lg, 0xFACADE, lg, 0)
        for w in (1, 3):
            for small in (False, True):
                cols = [rand_col(T, 1000 * lg + 10 * w + j + (5 if small else 0), small) for j in range(w)]
                A = eng.commit_rows(0, [c.tobytes() for c in cols])
                perm = host_sort(cols)
                sorted_rows = [c[perm].tobytes() for c in cols]

                def device():
                    s = eng.commit_sorted([A], w)
                    s.release()
                    return s.commitments

                def route_a():
                    p = host_sort(cols)
                    s = eng.commit_rows(0, [c[p].tobytes() for c in cols])
                    s.release()
                    return s.commitments

                def route_b():
                    s = eng.commit_rows(0, sorted_rows)
                    s.release()
                    return s.commitments

                def timed(f):
                    samples = []
                    for _ in range(a.reps):
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

                assert device() == route_a() == route_b()   # (also the warm-up: buffers, twiddles)
                td, ta, tb = [], [], []
                for _ in range(a.rounds):                   # interleaved: the routes see the same clock and thermal state
                    td.append(timed(device))
                    ta.append(timed(route_a))
                    tb.append(timed(route_b))
                md, ma, mb = median(td), median(ta), median(tb)
                print(json.dumps({"metric": "sorted", "T_log2": lg, "width": w, "n_keys": w,
                                  "keys": "below 2^16" if small else "uniform", "sorted_ms": round(md, 4),
                                  "route_a_ms": round(ma, 4), "route_b_ms": round(mb, 4),
                                  "sorted_over_route_a": round(md / ma, 3), "sorted_over_route_b": round(md / mb, 3),
                                  "sorted_rounds_ms": [round(x, 4) for x in td], "route_a_rounds_ms": [round(x, 4) for x in ta],
                                  "route_b_rounds_ms": [round(x, 4) for x in tb], "sorted_stages_ms": stages(device), **ident}),
                      flush=True)
                A.release()
        eng.close()


if __name__ == "__main__":
    main()
