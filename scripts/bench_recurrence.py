"""The device-built recurrence columns (worker_commit_recurrence's engine call) against the routes they replace, interleaved on
the same box, for T in {2^16, 2^20} and three shapes over resident random columns (committed once, outside the timing):

  running sum      A empty, B one row:              v' = v + b
  horner           A a constant, B one row:         acc' = acc r + byte
  general          A and B three-term expressions over four columns, A zero on every 61st row (restarts)

  recur    commit_recurrence over the resident set: one forward transform per distinct source row named, two pointwise passes
           (A and B), the scan, one inverse transform and one MSM.  Nothing row-sized crosses the host link
  route a  what a caller does without it: the column computed on the host from its copy of the columns as Python integers,
           packed to 32-byte scalars, then commit_rows of it in evaluation form
  route b  commit_rows of the same (precomputed) column alone, upload included: the floor of route a
  route c  commit_expr committing A and B themselves: the same forward transforms and pointwise passes, no scan, and TWO rows
           transformed back and committed instead of one

Routes a, b and c run code this builder does not touch.  One JSON line per point with the ratios and the profiled stage split
of the new call, stamped with the library identity like bench.py's lines.

    python scripts/bench_recurrence.py [--rounds 3] [--reps 3] [--host-reps 1] [--sizes 16,20]"""
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
from scripts.bench_expr import R, be, host_eval, median, pack  # noqa: E402
from zkp_subnet_amd import HipEngine, _native  # noqa: E402

RLC = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF
# (name, number of source columns, multiplier terms, addend terms); column 3 of the general case is the restart selector
CASES = [
    ("running sum", 1, [], [(1, [0])]),
    ("horner", 1, [(RLC, [])], [(1, [0])]),
    ("general", 4, [(1, [0, 3]), (5, [3, (1, 1)]), (RLC, [3])], [(1, [1, 2]), (R - 2, [(0, -1)]), (7, [])]),
]


def host_scan(cols, mul, add, start):
    T = len(cols[0])
    a = host_eval(cols, mul) if mul else [1] * T
    b = host_eval(cols, add) if add else [0] * T
    v, out = start, []
    for t in range(T):
        out.append(v)
        v = (a[t] * v + b[t]) % R
    return out


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
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0xEC02 + lg, 0xFACADE, lg, 0)
        for name, k, mul, add in CASES:
            rnd = random.Random(1000 * lg + len(name))
            cols = [[rnd.getrandbits(254) for _ in range(T)] for _ in range(k)]
            if k == 4:
                cols[3] = [int(t % 61 != 0) for t in range(T)]
            start = rnd.getrandbits(254)
            S = eng.commit_rows(0, [pack(c) for c in cols])
            bmul, badd = [(be(c), fs) for c, fs in mul], [(be(c), fs) for c, fs in add]
            row = pack(host_scan(cols, mul, add, start))
            sides = [(bmul or [(be(1), [])],), (badd,)]   # (an empty multiplier as its constant: one term, no factor)

            def device():
                s, closings = eng.commit_recurrence([S], [(bmul, badd, be(start))])
                s.release()
                return s.commitments

            def route_a():
                s = eng.commit_rows(0, [pack(host_scan(cols, mul, add, start))])
                s.release()
                return s.commitments

            def route_b():
                s = eng.commit_rows(0, [row])
                s.release()
                return s.commitments

            def route_c():
                s, _, _ = eng.commit_expr([S], sides)
                s.release()
                return s.commitments

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

            assert device() == route_b()                # (also the warm-up: buffers, twiddles)
            route_c()
            device()
            td, ta, tb, tc = [], [], [], []
            for _ in range(a.rounds):                   # interleaved: the routes see the same clock and thermal state
                td.append(timed(device, a.reps))
                ta.append(timed(route_a, a.host_reps))
                tb.append(timed(route_b, a.reps))
                tc.append(timed(route_c, a.reps))
            md, ma, mb, mc = median(td), median(ta), median(tb), median(tc)
            print(json.dumps({"metric": "recurrence", "T_log2": lg, "case": name, "recur_ms": round(md, 4),
                              "route_a_ms": round(ma, 4), "route_b_ms": round(mb, 4), "route_c_ms": round(mc, 4),
                              "recur_over_route_a": round(md / ma, 5), "recur_over_route_b": round(md / mb, 3),
                              "recur_over_route_c": round(md / mc, 3),
                              "recur_rounds_ms": [round(x, 4) for x in td], "route_a_rounds_ms": [round(x, 4) for x in ta],
                              "route_b_rounds_ms": [round(x, 4) for x in tb], "route_c_rounds_ms": [round(x, 4) for x in tc],
                              "recur_stages_ms": stages(device), **ident}), flush=True)
            S.release()
        eng.close()


if __name__ == "__main__":
    main()
