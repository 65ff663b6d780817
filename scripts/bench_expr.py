"""The device-built expression columns (worker_commit_expr's engine call) against the routes they replace, interleaved on the
same box, for T in {2^16, 2^20} and three cases over resident random columns (committed once, outside the timing):

  c = a b          one committed expression of one term of two factors
  plonk gate       the check q_L a + q_R b + q_M a b + q_O c + q_C over eight resident columns that satisfy it: nothing is
                   committed, the answer is (0, none)
  4 x 3 terms      four committed expressions of three terms each over four columns (products, a rotated factor, a
                   theta-compressed tuple, constants)

  expr     commit_expr over the resident sets: one forward transform per distinct source row named, one pointwise pass per
           expression, and for the committed ones an inverse transform each and one MSM pass.  Nothing row-sized crosses the
           host link
  route a  what a caller does without it: the rows computed on the host from its copy of the columns as Python integers, packed
           to 32-byte scalars, then commit_rows of the rows in evaluation form (for the check: the host arithmetic alone)
  route b  commit_rows of the same (precomputed) rows alone, upload included: the floor of route a, and what the new call
           trades against its forward transforms and pointwise pass (committed cases only)
  quotient for the check: commit_quotient of the same gate over the same sets (ext_log = 1, two pieces) -- what a prover pays
           today to learn whether the gate holds, and without a row index when it does not

Routes a, b and the quotient run code this builder does not touch.  One JSON line per point with the ratios and the profiled
stage split of the new call, stamped with the library identity like bench.py's lines.

    python scripts/bench_expr.py [--rounds 3] [--reps 3] [--host-reps 1] [--sizes 16,20]"""
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
THETA = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF
# (name, number of source columns, expressions); the gate's column c is solved for so that the gate holds
CASES = [
    ("c = a b", 2, [([(1, [0, 1])],)]),
    ("plonk gate check", 8, [([(1, [0, 5]), (1, [1, 6]), (1, [2, 5, 6]), (1, [3, 7]), (1, [4])], True)]),
    ("4 x 3 terms", 4, [([(1, [0, 1]), (1, [2, 3]), (5, [])],), ([(1, [0, (1, 1)]), (1, [2]), (R - 1, [3])],),
                        ([(1, [0]), (THETA, [1]), (THETA * THETA % R, [2])],), ([(3, [0, 0]), (R - 2, [1, 2, 3]), (7, [])],)]),
]


def be(v):
    return (v % R).to_bytes(32, "big")


def host_eval(cols, terms):
    """one expression over the integer columns, on the host"""
    T = len(cols[0])
    out = [0] * T
    for c, fs in terms:
        fs = [(f, 0) if isinstance(f, int) else f for f in fs]
        if not fs:
            out = [(v + c) % R for v in out]
            continue
        vecs = [cols[j] if rot % T == 0 else cols[j][rot % T:] + cols[j][:rot % T] for j, rot in fs]
        for t in range(T):
            p = c
            for v in vecs:
                p = p * v[t] % R
            out[t] = (out[t] + p) % R
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
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0xE7B2 + lg, 0xFACADE, lg, 0)
        for name, k, exprs in CASES:
            rnd = random.Random(1000 * lg + len(name))
            cols = [[rnd.getrandbits(254) for _ in range(T)] for _ in range(k)]
            check = len(exprs[0]) == 2
            if check:   # q_O = -1 and c = q_L a + q_R b + q_M a b + q_C: the gate holds on every row
                cols[3] = [R - 1] * T
                cols[7] = host_eval(cols, [t for t in exprs[0][0] if t[1] != [3, 7]])
            S = eng.commit_rows(0, [pack(c) for c in cols])
            bexprs = [([(be(c), fs) for c, fs in e[0]],) + tuple(e[1:]) for e in exprs]
            rows = [] if check else [pack(host_eval(cols, e[0])) for e in exprs]

            def device():
                s, nz, first = eng.commit_expr([S], bexprs)
                if s is None:
                    return nz, first
                s.release()
                return s.commitments

            def route_a():
                if check:
                    v = host_eval(cols, exprs[0][0])
                    return [sum(1 for x in v if x)], [next((t for t, x in enumerate(v) if x), None)]
                s = eng.commit_rows(0, [pack(host_eval(cols, e[0])) for e in exprs])
                s.release()
                return s.commitments

            def route_b():
                s = eng.commit_rows(0, rows)
                s.release()
                return s.commitments

            def quotient():
                s = eng.commit_quotient_ext([S], bexprs[0][0], None, None, 1, 2)
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

            other = quotient if check else route_b
            if check:                                   # (also the warm-up: buffers, twiddles)
                assert device() == ([0], [None])
                quotient()
            else:
                assert device() == route_b()
            device()
            td, ta, tb = [], [], []
            for _ in range(a.rounds):                   # interleaved: the routes see the same clock and thermal state
                td.append(timed(device, a.reps))
                ta.append(timed(route_a, a.host_reps))
                tb.append(timed(other, a.reps))
            md, ma, mb = median(td), median(ta), median(tb)
            oname = "quotient" if check else "route_b"
            print(json.dumps({"metric": "expr", "T_log2": lg, "case": name, "n_out": len(rows), "expr_ms": round(md, 4),
                              "route_a_ms": round(ma, 4), oname + "_ms": round(mb, 4),
                              "expr_over_route_a": round(md / ma, 5), "expr_over_" + oname: round(md / mb, 3),
                              "expr_rounds_ms": [round(x, 4) for x in td], "route_a_rounds_ms": [round(x, 4) for x in ta],
                              oname + "_rounds_ms": [round(x, 4) for x in tb], "expr_stages_ms": stages(device), **ident}),
                  flush=True)
            S.release()
        eng.close()


if __name__ == "__main__":
    main()
