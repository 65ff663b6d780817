"""The device-built integer ALU columns (worker_commit_int's engine call) against the routes they replace, interleaved on the
same box, for T in {2^16, 2^20} and five shapes: xor at w = 32 (one row), add with its carry (two rows), the low and high word
of a product at w = 64 (two rows), quotient and remainder at w = 32 (two rows), and eight mixed ops with sixteen rows.  The
source columns (uniform below 2^w; a divisor column with a zero in every 64th cell) are committed once, outside the timing.

  int      commit_int over the resident set: one forward transform per distinct source row, ONE launch for all ops, n_out
           inverse transforms, one MSM pass of n_out scalar sets.  Nothing row-sized crosses the host link
  route a  what a caller does without it: the rows computed on the host from its copy of the columns as Python integers,
           packed to 32-byte scalars, then commit_rows of the n_out rows in evaluation form
  route b  commit_rows of the same n_out (precomputed) rows alone, upload included: the floor of route a, and what the new call
           trades against its forward transforms and its one pointwise pass

Routes a and b run code this builder does not touch.  One JSON line per point with both ratios and the profiled stage split of
the new call, stamped with the library identity like bench.py's lines.

    python scripts/bench_int.py [--rounds 3] [--reps 3] [--host-reps 1] [--sizes 16,20]"""
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

# columns: 0, 1 below 2^32; 2 a divisor below 2^32 with zeros; 3, 4 below 2^64; 5 a shift in [0, 32]
CASES = [("xor w32", [("xor", 32, 0, 1)]),
         ("add + carry w32", [("add", 32, 0, 1, 2)]),
         ("mul lo/hi w64", [("mul", 64, 3, 4, 2)]),
         ("divmod w32", [("divmod", 32, 0, 2, 2)]),
         ("8 mixed ops, 16 rows", [("add", 32, 0, 1, 2), ("sub", 32, 0, 1, 2), ("mul", 64, 3, 4, 2), ("mul", 32, 0, 1, 2),
                                   ("divmod", 32, 0, 2, 2), ("split", 32, 0, 5, 2), ("add", 64, 3, 4, 2),
                                   ("split", 64, 3, ("imm", 13), 2)])]


def host_rows(cols, op):
    """the op's output rows over the integer columns, on the host (every operand is in range here)"""
    kind, w, a = op[0], op[1], cols[op[2]]
    b = [op[3][1]] * len(a) if isinstance(op[3], tuple) else cols[op[3]]
    M = 1 << w
    if kind == "and":
        rows = [[x & y for x, y in zip(a, b)]]
    elif kind == "or":
        rows = [[x | y for x, y in zip(a, b)]]
    elif kind == "xor":
        rows = [[x ^ y for x, y in zip(a, b)]]
    elif kind == "add":
        rows = [[(x + y) % M for x, y in zip(a, b)], [(x + y) >> w for x, y in zip(a, b)]]
    elif kind == "sub":
        rows = [[(x - y) % M for x, y in zip(a, b)], [int(x < y) for x, y in zip(a, b)]]
    elif kind == "mul":
        rows = [[(x * y) % M for x, y in zip(a, b)], [(x * y) >> w for x, y in zip(a, b)]]
    elif kind == "divmod":
        rows = [[x // y if y else M - 1 for x, y in zip(a, b)], [x % y if y else x for x, y in zip(a, b)]]
    else:
        rows = [[x >> s for x, s in zip(a, b)], [x & ((1 << s) - 1) for x, s in zip(a, b)]]
    return rows[:op[4] if len(op) == 5 else 1]


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
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x1A7C + lg, 0xFACADE, lg, 0)
        rnd = random.Random(1000 * lg)
        cols = [[rnd.randrange(1 << 32) for _ in range(T)] for _ in range(2)]
        cols.append([0 if t % 64 == 17 else rnd.randrange(1, 1 << 32) for t in range(T)])
        cols += [[rnd.randrange(1 << 64) for _ in range(T)] for _ in range(2)]
        cols.append([rnd.randrange(33) for _ in range(T)])
        A = eng.commit_rows(0, [pack(c) for c in cols])
        for name, ops in CASES:
            rows = [pack(r) for op in ops for r in host_rows(cols, op)]

            def device():
                s, counts, _ = eng.commit_int([A], ops)
                s.release()
                assert not any(counts)
                return s.commitments

            def route_a():
                s = eng.commit_rows(0, [pack(r) for op in ops for r in host_rows(cols, op)])
                s.release()
                return s.commitments

            def route_b():
                s = eng.commit_rows(0, rows)
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

            assert device() == route_b()                # (also the warm-up: buffers, twiddles; route a commits the same rows)
            device()
            td, ta, tb = [], [], []
            for _ in range(a.rounds):                   # interleaved: the routes see the same clock and thermal state
                td.append(timed(device, a.reps))
                ta.append(timed(route_a, a.host_reps))
                tb.append(timed(route_b, a.reps))
            md, ma, mb = median(td), median(ta), median(tb)
            print(json.dumps({"metric": "int", "T_log2": lg, "case": name, "n_out": len(rows), "int_ms": round(md, 4),
                              "route_a_ms": round(ma, 4), "route_b_ms": round(mb, 4),
                              "int_over_route_a": round(md / ma, 4), "int_over_route_b": round(md / mb, 3),
                              "int_rounds_ms": [round(x, 4) for x in td], "route_a_rounds_ms": [round(x, 4) for x in ta],
                              "route_b_rounds_ms": [round(x, 4) for x in tb], "int_stages_ms": stages(device), **ident}),
                  flush=True)
        A.release()
        eng.close()


if __name__ == "__main__":
    main()
