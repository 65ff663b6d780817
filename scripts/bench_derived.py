"""The device-built helper columns (worker_commit_derived's engine call) against the routes they replace, interleaved on the same
box, for T in {2^16, 2^20} and four cases: one inverse-or-zero column, the same with its bit row, 4 limbs of 16 bits, 8 limbs of
8 bits.  The source column (a third of its cells zero for the inv0 cases, uniform below 2^64 for the limb cases) is committed
once, outside the timing.

  derived  commit_derived over the resident set: one forward transform, the pointwise passes (for inv0 the batched inversion),
           n_out inverse transforms, one MSM pass of n_out scalar sets.  Nothing row-sized crosses the host link
  route a  what a caller does without it: the rows computed on the host from its copy of the column as Python integers -- the
           inverses with Montgomery's batch trick (one modular inversion, three products per cell: the fair host route), the
           limbs with shifts and masks -- packed to 32-byte scalars, then commit_rows of the n_out rows in evaluation form
  route b  commit_rows of the same n_out (precomputed) rows alone, upload included: the floor of route a, and what the new call
           trades against its forward transform and pointwise passes

Routes a and b run code this builder does not touch.  One JSON line per point with both ratios and the profiled stage split of
the new call, stamped with the library identity like bench.py's lines.

    python scripts/bench_derived.py [--rounds 3] [--reps 3] [--host-reps 1] [--sizes 16,20]"""
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

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
CASES = [("inv0", [("inv0", 0)]), ("inv0 + bit", [("inv0", 0, True)]), ("limbs 16 x 4", [("limbs", 0, 16, 4)]),
         ("limbs 8 x 8", [("limbs", 0, 8, 8)])]


def host_rows(col, op):
    """the op's output rows over the integers `col`, on the host"""
    if op[0] == "inv0":
        nz = [t for t, x in enumerate(col) if x]
        pre, acc = [], 1
        for t in nz:
            pre.append(acc)
            acc = acc * col[t] % R
        inv = pow(acc, -1, R)
        out = [0] * len(col)
        for j in range(len(nz) - 1, -1, -1):
            t = nz[j]
            out[t] = inv * pre[j] % R
            inv = inv * col[t] % R
        return [out, [0 if x else 1 for x in col]] if len(op) == 3 and op[2] else [out]
    m = (1 << op[2]) - 1
    return [[(x >> (op[2] * l)) & m for x in col] for l in range(op[3])]


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
        eng.gen_srs(0xDE21 + lg, 0xFACADE, lg, 0)
        for name, ops in CASES:
            rnd = random.Random(1000 * lg + len(name))
            if ops[0][0] == "inv0":
                col = [0 if rnd.randrange(3) == 0 else rnd.randrange(R) for _ in range(T)]
            else:
                col = [rnd.randrange(1 << 64) for _ in range(T)]
            A = eng.commit_rows(0, [pack(col)])
            rows = [pack(r) for r in host_rows(col, ops[0])]

            def device():
                s, _ = eng.commit_derived([A], ops)
                s.release()
                return s.commitments

            def route_a():
                s = eng.commit_rows(0, [pack(r) for r in host_rows(col, ops[0])])
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
            print(json.dumps({"metric": "derived", "T_log2": lg, "case": name, "n_out": len(rows), "derived_ms": round(md, 4),
                              "route_a_ms": round(ma, 4), "route_b_ms": round(mb, 4),
                              "derived_over_route_a": round(md / ma, 4), "derived_over_route_b": round(md / mb, 3),
                              "derived_rounds_ms": [round(x, 4) for x in td], "route_a_rounds_ms": [round(x, 4) for x in ta],
                              "route_b_rounds_ms": [round(x, 4) for x in tb], "derived_stages_ms": stages(device), **ident}),
                  flush=True)
            A.release()
        eng.close()


if __name__ == "__main__":
    main()
