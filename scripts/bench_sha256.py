"""The device-built SHA-256 columns (worker_commit_sha256's engine call) against the routes they replace, interleaved on the
same box, for T in {2^16, 2^20} in five shapes: a row unit with 8 outputs (16 message columns, the standard initial value); a
rounds unit with w, a, e at P = 72, every block a message; the same with all twelve columns; a check of 8 expected columns (8
message columns and 8 immediates: a call names at most 16 rows); the single-message rounds unit (w, a, e, a start column of
zeros: ONE lane walks every block).  The source columns are committed once, outside the timing.

  sha256    commit_sha256 over the resident sets: the forward transforms, ONE launch, n_out inverse transforms, one MSM pass of
            n_out scalar sets (a check: neither).  Nothing row-sized crosses the host link
  route a   the columns computed on the host by the Python reference (tests/sha256_ref.py), then commit_rows_typed of the n_out
            u32 columns.  The host part is TIMED OVER A SAMPLE of --host-blocks compressions, compared cell by cell with the
            device's rows, and scaled to the shape's number of compressions (the loop is linear in them); route a = that + b
  route b   commit_rows_typed of the same n_out precomputed u32 columns alone, upload included (the rows are read back from the
            device set once, outside the timing)
  route c   for the check: the row unit that commits

One JSON line per point with the ratios and the profiled stage split of the new call (`poly` holds the kernel).

    python scripts/bench_sha256.py [--rounds 3] [--reps 3] [--host-blocks 512] [--sizes 16,20]"""
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
from tests import sha256_ref as sr  # noqa: E402
from zkp_subnet_amd import HipEngine, _native  # noqa: E402

PERIOD = 72
ALL = list(sr.NAMES)


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed sample of the device routes (the median is reported)")
    ap.add_argument("--host-blocks", type=int, default=512, help="compressions of route a's host part that are timed")
    ap.add_argument("--sizes", default="16,20")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x5A256 + lg, 0xFACADE, lg, 0)
        rnd = random.Random(1000 * lg)
        cols = [array.array("I", [rnd.getrandbits(32) for _ in range(T)]) for _ in range(16)]
        A = eng.commit_rows_typed(0, cols)
        Z = eng.commit_rows_typed(0, [array.array("I", [0] * T)])      # the start column of the single message
        row_unit = {"mode": "row", "state": "iv", "msg": list(range(16)), "out": list(range(8))}
        trace = lambda names, start=None: {"mode": "rounds", "msg": 0, "start": start, "period": PERIOD, "iv": None,   # noqa: E731
                                           "cols": names}
        # a call names at most 16 rows in all, so the check reads 8 message columns (the other 8 words are immediates) and
        # its 8 expected columns, resident
        A8 = eng.commit_rows_typed(0, cols[:8])
        half_unit = dict(row_unit, msg=list(range(8)) + [("imm", 0x80000000 + j) for j in range(8)])
        E, _ = eng.commit_sha256([A8], [half_unit])
        shapes = [("row 8 outputs", [A], row_unit, T), ("rounds w a e", [A], trace(["w", "a", "e"]), T // PERIOD),
                  ("rounds 12 columns", [A], trace(ALL), T // PERIOD),
                  ("check 8 columns", [A8, E], dict(half_unit, expect=list(range(8, 16))), T),
                  ("rounds w a e, one message", [A8, Z], trace(["w", "a", "e"], 8), T // PERIOD)]
        for name, sets, unit, blocks in shapes:
            check = "expect" in unit
            single = unit.get("start") is not None

            def device():
                s, st = eng.commit_sha256(sets, [unit])
                assert st["blocks"] == [blocks] and st["mismatch"] == [0] and st["counts"] == [0]
                if s is None:
                    return []
                s.release()
                return s.commitments

            first = eng.commit_sha256([A8] if check else sets, [half_unit if check else unit])[0]
            rows = [array.array("I", eng.read_rows([first], c, 0, T, "u32")[0]) for c in range(first.k)]
            first.release()
            # route a's host part over a sample, checked against the device's cells
            hb = min(a.host_blocks, blocks)
            t0 = time.perf_counter()
            if unit["mode"] == "row":
                imm = [s[1] if isinstance(s, tuple) else None for s in unit["msg"]]
                got = [sr.compress(sr.IV, [cols[j][p] if imm[j] is None else imm[j] for j in range(16)]) for p in range(hb)]
                host_ms = (time.perf_counter() - t0) * 1e3 * blocks / hb
                for p in (0, hb // 2, hb - 1):
                    assert [rows[c][p] for c in range(8)] == got[p]
            else:
                names, H, got = unit["cols"], list(sr.IV), []
                for p in range(hb):
                    blk, nxt = sr.block_trace(H, list(cols[0][p * PERIOD + 4:p * PERIOD + 20]))
                    H = nxt if single else list(sr.IV)
                    got.append(blk)
                host_ms = (time.perf_counter() - t0) * 1e3 * blocks / hb
                for p in (0, hb // 2, hb - 1):
                    for c, nm in enumerate(names):
                        assert list(rows[c][p * PERIOD:p * PERIOD + 72]) == got[p][nm], (p, nm)

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
            line = {"metric": "sha256", "T_log2": lg, "case": name, "blocks": blocks, "n_out": 0 if check else len(rows),
                    "sha256_ms": round(md, 4), "route_a_ms": round(host_ms + mb, 2), "route_a_host_ms_scaled": round(host_ms, 2),
                    "route_a_host_blocks_timed": hb, "route_b_ms": round(mb, 4), "sha256_over_route_a": round(md / (host_ms + mb), 5),
                    "sha256_over_route_b": round(md / mb, 3), "sha256_rounds_ms": [round(x, 4) for x in td],
                    "route_b_rounds_ms": [round(x, 4) for x in tb], "sha256_stages_ms": stages(device), **ident}
            if check:                                   # route c: the row unit that commits; route b is its committed columns
                def route_c():
                    s, _ = eng.commit_sha256([A8], [half_unit])
                    s.release()

                route_c()
                tc = [timed(route_c, a.reps) for _ in range(a.rounds)]
                line.update(route_c_ms=round(median(tc), 4), sha256_over_route_c=round(md / median(tc), 3))
            print(json.dumps(line), flush=True)
        for s in (E, A8, Z, A):
            s.release()
        eng.close()


if __name__ == "__main__":
    main()
