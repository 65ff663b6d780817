"""The device-built Keccak-f[1600] columns (worker_commit_keccak's engine call) against the routes they replace, interleaved on
the same box, for T in {2^16, 2^20} in five shapes: a row unit of the Merkle shape with 4 outputs (8 node columns, 0x01 in lane
8, 2^63 in lane 16: Keccak-256 of two 32-byte nodes per row); a rounds unit with a0 .. a4 at P = 125 and rate 17, every block a
message; the same with sixteen columns (a, p, d and t0); a check of the row unit's 4 expected columns; the single-message rounds
unit (a0 .. a4, a start column of zeros: ONE lane walks every block).  The source columns are committed once, outside the timing.

  keccak    commit_keccak over the resident sets: the forward transforms, ONE launch, n_out inverse transforms, one MSM pass of
            n_out scalar sets (a check: neither).  Nothing row-sized crosses the host link
  route a   the columns computed on the host by the Python reference (tests/keccak_ref.py), then commit_rows_typed of the n_out
            u64 columns.  The host part is TIMED OVER A SAMPLE of --host-blocks permutations, compared cell by cell with the
            device's rows, and scaled to the shape's number of permutations (the loop is linear in them); route a = that + b
  route b   commit_rows_typed of the same n_out precomputed u64 columns alone, upload included (the rows are read back from the
            device set once, outside the timing)
  route c   for the check: the row unit that commits

One JSON line per point with the ratios and the profiled stage split of the new call (`poly` holds the kernel).

    python scripts/bench_keccak.py [--rounds 3] [--reps 3] [--host-blocks 256] [--sizes 16,20]"""
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
from tests import keccak_ref as kr  # noqa: E402
from zkp_subnet_amd import HipEngine, _native  # noqa: E402

PERIOD, RATE = 125, 17
STATE = [f"a{x}" for x in range(5)]
SIXTEEN = list(kr.NAMES[:16])


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed sample of the device routes (the median is reported)")
    ap.add_argument("--host-blocks", type=int, default=256, help="permutations of route a's host part that are timed")
    ap.add_argument("--sizes", default="16,20")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x6EC4A6 + lg, 0xFACADE, lg, 0)
        rnd = random.Random(1000 * lg)
        cols = [array.array("Q", [rnd.getrandbits(64) for _ in range(T)]) for _ in range(8)]
        A = eng.commit_rows_typed(0, cols)
        Z = eng.commit_rows_typed(0, [array.array("Q", [0] * T)])      # the start column of the single message
        row_unit = {"mode": "row", "in": list(range(8)) + [("imm", 1)] + [("imm", 0)] * 7 + [("imm", 1 << 63)] + [("imm", 0)] * 8,
                    "out": [0, 1, 2, 3]}
        trace = lambda names, start=None: {"mode": "rounds", "msg": [0, 1, 2, 3, 4], "rate": RATE, "start": start,   # noqa: E731
                                           "period": PERIOD, "cols": names}
        E, _ = eng.commit_keccak([A], [row_unit])
        shapes = [("row 4 outputs", [A], row_unit, T), ("rounds a0..a4", [A], trace(STATE), T // PERIOD),
                  ("rounds 16 columns", [A], trace(SIXTEEN), T // PERIOD),
                  ("check 4 columns", [A, E], dict(row_unit, expect=[8, 9, 10, 11]), T),
                  ("rounds a0..a4, one message", [A, Z], trace(STATE, 8), T // PERIOD)]
        for name, sets, unit, blocks in shapes:
            check = "expect" in unit
            single = unit.get("start") is not None

            def device():
                s, st = eng.commit_keccak(sets, [unit])
                assert st["perms"] == [blocks] and st["mismatch"] == [0] and st["counts"] == [0]
                if s is None:
                    return []
                s.release()
                return s.commitments

            first = eng.commit_keccak([A] if check else sets, [row_unit if check else unit])[0]
            rows = [array.array("Q", eng.read_rows([first], c, 0, T, "u64")[0]) for c in range(first.k)]
            first.release()
            # route a's host part over a sample, checked against the device's cells
            hb = min(a.host_blocks, blocks)
            t0 = time.perf_counter()
            if unit["mode"] == "row":
                imm = [s[1] if isinstance(s, tuple) else None for s in unit["in"]]
                got = [kr.permute([cols[j][p] if imm[j] is None else imm[j] for j in range(25)]) for p in range(hb)]
                host_ms = (time.perf_counter() - t0) * 1e3 * blocks / hb
                for p in (0, hb // 2, hb - 1):
                    assert [rows[c][p] for c in range(4)] == got[p][:4]
            else:
                names, S, got = unit["cols"], [0] * 25, []
                for p in range(hb):
                    blk, nxt = kr.block_trace([S[i] ^ (cols[i % 5][p * PERIOD + i // 5] if i < RATE else 0) for i in range(25)])
                    S = nxt if single else [0] * 25
                    got.append(blk)
                host_ms = (time.perf_counter() - t0) * 1e3 * blocks / hb
                for p in (0, hb // 2, hb - 1):
                    for c, nm in enumerate(names):
                        assert list(rows[c][p * PERIOD:p * PERIOD + 125]) == got[p][nm], (p, nm)

            def route_b():
                s = eng.commit_rows_typed(0, rows)
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

            warm = device()                             # (also the warm-up)
            assert check or warm == route_b()
            device()
            td, tb = [], []
            for _ in range(a.rounds):                   # interleaved: the routes see the same clock and thermal state
                td.append(timed(device, a.reps))
                tb.append(timed(route_b, a.reps))
            md, mb = median(td), median(tb)
            line = {"metric": "keccak", "T_log2": lg, "case": name, "perms": blocks, "n_out": 0 if check else len(rows),
                    "keccak_ms": round(md, 4), "route_a_ms": round(host_ms + mb, 2), "route_a_host_ms_scaled": round(host_ms, 2),
                    "route_a_host_perms_timed": hb, "route_b_ms": round(mb, 4), "keccak_over_route_a": round(md / (host_ms + mb), 5),
                    "keccak_over_route_b": round(md / mb, 3), "keccak_rounds_ms": [round(x, 4) for x in td],
                    "route_b_rounds_ms": [round(x, 4) for x in tb], "keccak_stages_ms": stages(device), **ident}
            if check:                                   # route c: the row unit that commits; route b is its committed columns
                def route_c():
                    s, _ = eng.commit_keccak([A], [row_unit])
                    s.release()

                route_c()
                tc = [timed(route_c, a.reps) for _ in range(a.rounds)]
                line.update(route_c_ms=round(median(tc), 4), keccak_over_route_c=round(md / median(tc), 3))
            print(json.dumps(line), flush=True)
        for s in (E, Z, A):
            s.release()
        eng.close()


if __name__ == "__main__":
    main()
