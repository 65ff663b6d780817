"""The device-built Poseidon chains (worker_commit_poseidon_chain's engine call) against the routes beside them, interleaved on
the same box, for T in {2^16, 2^20} at t = 3, R_F = 8, R_P = 57 (seeded random constants, a Cauchy matrix).  The source columns
are committed once, outside the timing.  Shapes:

  flat path depth 32     path, P = 1, every 32nd block starts a path, cols out1: T / 32 segments of 32 permutations
  trace path depth 32    path, P = 128, every 32nd block starts a path, three trace columns: T / 4096 segments of 32
  trace sponge 8 blocks  sponge, P = 128, messages of 8 blocks, three trace columns
  trace, no start        sponge, P = 128, start null: the arithmetic of route c with no carry
  check                  the flat path as a check against its own resident digests: no set, no inverse transform, no MSM
  one segment            sponge, P = 128, ONE message over the whole column (time only, one call: seconds at 2^20;
                         --one-segment-max caps its size)

  route b   commit_rows of the same precomputed rows alone, upload included (the rows are read back from the device set once,
            outside the timing)
  route c   commit_poseidon's rounds unit (P = 128) over the same number of blocks: the same arithmetic with no carry; for the
            flat path, P = 1 has no rounds unit, so route c is the row unit with one output over the same T permutations

One JSON line per point with the ratios, the profiled stage split of the new call (`poly` holds the kernel) and, for chained
shapes, (chain - c) / (segment length - 1): the per-permutation latency the serial walk adds.

    python scripts/bench_poseidon_chain.py [--rounds 3] [--reps 3] [--sizes 16,20] [--one-segment-max 20] [--shapes a,b]"""
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

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
T_W, FULL, PARTIAL, PERIOD, DEPTH, MSG = 3, 8, 57, 128, 32, 8


def make_params(seed):
    rnd = random.Random(seed)
    return {"t": T_W, "full": FULL, "partial": PARTIAL, "rc": [rnd.randrange(R) for _ in range(T_W * (FULL + PARTIAL))],
            "mds": [pow(1 + i + T_W + j, R - 2, R) for i in range(T_W) for j in range(T_W)]}


def pack(row):
    return b"".join(v.to_bytes(32, "big") for v in row)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed sample (the median is reported)")
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--one-segment-max", type=int, default=20, help="the largest log2 T at which the one-segment shape runs")
    ap.add_argument("--shapes", default="", help="run only the shapes whose name contains one of these comma-separated words")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    params = make_params(0x905E1D1)
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x905F + lg, 0xFACADE, lg, 0)
        rnd = random.Random(1000 * lg)
        # rows: 0, 1 data; 2 pos (0 / 1); 3 .. 6 start columns: paths at P = 1, paths at P = 128, messages at P = 128, row 0 only
        cols = [[rnd.randrange(R) for _ in range(T)] for _ in range(2)] + [[rnd.randrange(2) for _ in range(T)]]
        cols.append([int(r % DEPTH == 0) for r in range(T)])
        cols.append([int(r % (DEPTH * PERIOD) == 0) for r in range(T)])
        cols.append([int(r % (MSG * PERIOD) == 0) for r in range(T)])
        cols.append([0] * T)
        A = eng.commit_rows(0, [pack(c) for c in cols])
        path = {"mode": "path", "cap": ("imm", 1), "leaf": 0, "sib": [1], "pos": 2, "digest": 1}
        flat = dict(path, start=3, period=1, layout="flat", cols=["out1"])
        E, _ = eng.commit_poseidon_chain([A], params, [flat])        # the digests the check expects, resident
        sponge = {"mode": "sponge", "in": [("imm", 1), 0, 1], "period": PERIOD, "layout": "trace"}
        rounds_c = {"mode": "rounds", "in": [("imm", 1), 0, 1], "period": PERIOD}
        row_c = {"mode": "row", "in": [("imm", 1), 0, 1], "out": [1]}
        shapes = [("flat path depth 32", [A], [flat], DEPTH, row_c), ("trace path depth 32", [A], [dict(path, start=4, period=PERIOD, layout="trace")], DEPTH, rounds_c),
                  ("trace sponge 8 blocks", [A], [dict(sponge, start=5)], MSG, rounds_c),
                  ("trace, no start", [A], [dict(sponge, start=None)], 1, rounds_c),
                  ("check", [A, E], [dict(path, start=3, period=1, expect=7)], DEPTH, None)]
        if lg <= a.one_segment_max:
            shapes.append(("one segment", [A], [dict(sponge, start=6)], T // PERIOD, rounds_c))
        if a.shapes:
            shapes = [s for s in shapes if any(w in s[0] for w in a.shapes.split(","))]
        flat_ms = None
        for name, sets, units, seg_len, c_unit in shapes:
            check = "expect" in units[0]

            def device():
                s, st = eng.commit_poseidon_chain(sets, params, units)
                assert st["mismatch"] == [0] and st["bad_pos"] == [0]
                if s is None:
                    return []
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

            line = {"metric": "poseidon_chain", "T_log2": lg, "case": name, "t": T_W, "full": FULL, "partial": PARTIAL,
                    "segment_blocks": seg_len}
            if name == "one segment":                   # time only: one call
                line["chain_ms"] = round(timed(device, 1), 2)
                line["ms_per_perm"] = round(line["chain_ms"] / seg_len, 4)
                print(json.dumps({**line, **ident}), flush=True)
                continue
            rows = []
            if not check:
                first = eng.commit_poseidon_chain(sets, params, units)[0]
                rows = [eng.read_rows([first], c, 0, T, "fr")[0] for c in range(first.k)]
                first.release()

            def route_b():
                s = eng.commit_rows(0, rows)
                s.release()
                return s.commitments

            def route_c():
                s, _ = eng.commit_poseidon([A], params, [c_unit])
                s.release()

            warm = device()
            assert check or warm == route_b()
            td, tb, tc = [], [], []
            for _ in range(a.rounds):                   # interleaved: the routes see the same clock and thermal state
                td.append(timed(device, a.reps))
                if not check:
                    tb.append(timed(route_b, a.reps))
                if c_unit:
                    tc.append(timed(route_c, a.reps))
            md = median(td)
            line.update(n_out=len(rows), chain_ms=round(md, 4), chain_rounds_ms=[round(x, 4) for x in td])
            if tb:
                line.update(route_b_ms=round(median(tb), 4), chain_over_route_b=round(md / median(tb), 3))
            if tc:
                mc = median(tc)
                line.update(route_c_ms=round(mc, 4), chain_over_route_c=round(md / mc, 3))
                if seg_len > 1:
                    line["added_ms_per_perm"] = round((md - mc) / (seg_len - 1), 4)
            if name == "flat path depth 32":
                flat_ms = md
            if check and flat_ms:
                line.update(committing_unit_ms=round(flat_ms, 4), check_over_committing_unit=round(md / flat_ms, 3))
            line["chain_stages_ms"] = stages(device)
            print(json.dumps({**line, **ident}), flush=True)
        E.release()
        A.release()
        eng.close()


if __name__ == "__main__":
    main()
