"""The device-built sigma columns (worker_commit_sigma's engine call) and the copy check against the routes they replace,
interleaved on the same box, for T in {2^16, 2^20} and k in {3, 8} label columns.  Labels are uniform variable ids below k T / 2
(about two cells per class), committed once as u32 rows outside the timing, like the wires (the variables' values).

  sigma    commit_sigma over the resident label set: k forward transforms, the sort of k T cells, one link launch, k inverse
           transforms, one MSM pass of k scalar sets.  Nothing row-sized crosses the host link
  route a  what a caller does without it: sigma computed on the host in Python integers (sort (label, flat index), link the
           classes, one product shift * w^t' per cell), packed to 32-byte scalars, then commit_rows of the k rows
  route b  commit_rows of the same k (precomputed) rows alone, upload included: the floor of route a
  route c  commit_sorted of ONE label column: the same sort over T cells instead of k T, with its gather and one MSM
  check    check_copies over the wires and the labels, against commit_grand_product over the same wires and the sigma set --
           what finding out whether a witness respects its copy constraints costs without the check

Routes a, b, c and the grand product run code this builder does not touch.  One JSON line per point with the ratios and the
profiled stage split of the two new calls, stamped with the library identity like bench.py's lines.

    python scripts/bench_sigma.py [--rounds 3] [--reps 3] [--host-reps 1] [--sizes 16,20] [--ks 3,8]"""
import argparse
import array
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


def host_sigma(labels, shifts):
    """the k sigma rows in Python integers: every class one cycle in ascending flat index"""
    k, T = len(labels), len(labels[0])
    w, dom, x = pow(7, (R - 1) // T, R), [], 1
    for _ in range(T):
        dom.append(x)
        x = x * w % R
    cells = sorted((lab, c * T + t) for c, col in enumerate(labels) for t, lab in enumerate(col))
    img = [0] * (k * T)
    p, N = 0, k * T
    while p < N:
        q = p
        while q + 1 < N and cells[q + 1][0] == cells[p][0]:
            img[cells[q][1]] = cells[q + 1][1]
            q += 1
        img[cells[q][1]] = cells[p][1]
        p = q + 1
    return [[shifts[j // T] * dom[j % T] % R for j in img[c * T:(c + 1) * T]] for c in range(k)]


def pack(row):
    return b"".join(v.to_bytes(32, "big") for v in row)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed sample of the device routes (the median is reported)")
    ap.add_argument("--host-reps", type=int, default=1, help="calls per timed sample of route a (tens of seconds each at 2^20)")
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--ks", default="3,8")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        eng = HipEngine(0)
        eng.gen_srs(0x51C3 + lg, 0xFACADE, lg, 0)
        T = 1 << lg
        for k in [int(x) for x in a.ks.split(",")]:
            rnd = random.Random(1000 * lg + k)
            labels = [[rnd.randrange(k * T // 2) for _ in range(T)] for _ in range(k)]
            values = [rnd.randrange(R) for _ in range(k * T // 2)]
            shifts = [pow(7, c, R) for c in range(k)]
            sh = [s.to_bytes(32, "big") for s in shifts]
            beta, gamma = rnd.randrange(R).to_bytes(32, "big"), rnd.randrange(R).to_bytes(32, "big")
            L = eng.commit_rows_typed(0, [array.array("I", col) for col in labels])
            L0 = eng.commit_rows_typed(0, [array.array("I", labels[0])])
            W = eng.commit_rows(0, [pack([values[v] for v in col]) for col in labels])
            rows = [pack(r) for r in host_sigma(labels, shifts)]
            S = eng.commit_rows(0, rows)

            def device():
                cs, s, _ = eng.commit_sigma([L], sh)
                s.release()
                return cs

            def route_a():
                s = eng.commit_rows(0, [pack(r) for r in host_sigma(labels, shifts)])
                s.release()
                return s.commitments

            def route_b():
                s = eng.commit_rows(0, rows)
                s.release()
                return s.commitments

            def route_c():
                eng.commit_sorted([L0], 1, 1).release()

            def check():
                assert eng.check_copies([W], [L])["violations"] == 0

            def grand_product():
                z, closing = eng.commit_grand_product([W], [S], sh, beta, gamma)
                z.release()
                assert closing == (1).to_bytes(32, "big")

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

            assert device() == route_b() == S.commitments   # (also the warm-up: buffers, twiddles; route a commits the same rows)
            for f in (device, route_c, check, grand_product):
                f()
            t = {name: [] for name in ("sigma", "a", "b", "c", "check", "gp")}
            for _ in range(a.rounds):                       # interleaved: the routes see the same clock and thermal state
                t["sigma"].append(timed(device, a.reps))
                t["a"].append(timed(route_a, a.host_reps))
                t["b"].append(timed(route_b, a.reps))
                t["c"].append(timed(route_c, a.reps))
                t["check"].append(timed(check, a.reps))
                t["gp"].append(timed(grand_product, a.reps))
            m = {name: median(v) for name, v in t.items()}
            print(json.dumps({"metric": "sigma", "T_log2": lg, "k": k, "sigma_ms": round(m["sigma"], 4),
                              "route_a_ms": round(m["a"], 4), "route_b_ms": round(m["b"], 4), "route_c_ms": round(m["c"], 4),
                              "check_ms": round(m["check"], 4), "grand_product_ms": round(m["gp"], 4),
                              "sigma_over_route_a": round(m["sigma"] / m["a"], 5), "sigma_over_route_b": round(m["sigma"] / m["b"], 3),
                              "sigma_over_route_c": round(m["sigma"] / m["c"], 3),
                              "check_over_grand_product": round(m["check"] / m["gp"], 3),
                              "rounds_ms": {name: [round(x, 4) for x in v] for name, v in t.items()},
                              "sigma_stages_ms": stages(device), "check_stages_ms": stages(check), **ident}), flush=True)
            for s in (L, L0, W, S):
                s.release()
        eng.close()


if __name__ == "__main__":
    main()
