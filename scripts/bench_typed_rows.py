"""Typed columns in and cells back out (commit_rows_typed / read_rows) against the route they shorten, interleaved on the same
box, for T in {2^16, 2^20} and k in {1, 4, 8} columns:

  typed    commit_rows_typed of k u8, u32 or u64 columns: k T width bytes cross the host link, one decode launch, then the
           transforms and the MSM pass of commit_rows
  route b  commit_rows of the same values written as 32-byte big-endian rows (precomputed, outside the timing), upload included:
           README's "route (b)" of every builder benchmark, code this change does not touch

and, per size, read_rows of one whole row of a resident set as u32 and as 32-byte scalars (one forward transform, one narrowing
launch, T width bytes back).  One JSON line per point with the ratios and the profiled stage split of the typed call, stamped
with the library identity like bench.py's lines.

    python scripts/bench_typed_rows.py [--rounds 3] [--reps 3] [--sizes 16,20] [--ks 1,4,8]"""
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

KINDS = {"u8": ("B", 8), "u32": ("I", 32), "u64": ("Q", 64)}


def median(xs):
    return sorted(xs)[len(xs) // 2]


def be32_row(col, width):
    """the column (an array of `width`-byte unsigned integers) as 32-byte big-endian scalars"""
    a = array.array(col.typecode, col)
    if width > 1:
        a.byteswap()
    raw, out = a.tobytes(), bytearray(32 * len(col))
    for j in range(width):
        out[32 - width + j::32] = raw[j::width]
    return bytes(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3, help="calls per timed sample (the median is reported)")
    ap.add_argument("--sizes", default="16,20")
    ap.add_argument("--ks", default="1,4,8")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()

    def timed(f, reps):
        samples = []
        for _ in range(reps):
            t0 = time.perf_counter()
            f()
            samples.append(time.perf_counter() - t0)
        return median(samples) * 1e3

    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x7E9ED + lg, 0xFACADE, lg, 0)

        def stages(f):
            eng._chk(lib.kzg_set_profiling(eng._h, 1))
            try:
                f()
                tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
                eng._chk(lib.kzg_get_timings(eng._h, tms, len(tms)))
            finally:
                eng._chk(lib.kzg_set_profiling(eng._h, 0))
            return {n: round(v, 4) for n, v in zip(_native.TIMING_NAMES, tms) if v}

        for k in [int(x) for x in a.ks.split(",")]:
            rnd = random.Random(100 * lg + k)
            for kind, (code, bits) in KINDS.items():
                cols = [array.array(code, rnd.randbytes(T * bits // 8)) for _ in range(k)]
                rows = [be32_row(c, bits // 8) for c in cols]

                def typed():
                    s = eng.commit_rows_typed(0, cols)
                    s.release()
                    return s.commitments

                def route_b():
                    s = eng.commit_rows(0, rows)
                    s.release()
                    return s.commitments

                assert typed() == route_b()             # (also the warm-up: buffers, twiddles)
                tt, tb = [], []
                for _ in range(a.rounds):               # interleaved: both routes see the same clock and thermal state
                    tt.append(timed(typed, a.reps))
                    tb.append(timed(route_b, a.reps))
                mt, mb = median(tt), median(tb)
                print(json.dumps({"metric": "typed_rows_commit", "T_log2": lg, "k": k, "kind": kind, "typed_ms": round(mt, 4),
                                  "route_b_ms": round(mb, 4), "typed_over_route_b": round(mt / mb, 3),
                                  "typed_rounds_ms": [round(x, 4) for x in tt], "route_b_rounds_ms": [round(x, 4) for x in tb],
                                  "upload_bytes": k * T * bits // 8, "route_b_upload_bytes": k * T * 32,
                                  "typed_stages_ms": stages(typed), **ident}), flush=True)
        rnd = random.Random(lg)
        col = array.array("I", rnd.randbytes(4 * T))
        s = eng.commit_rows_typed(0, [col])
        assert eng.read_rows([s], 0, 0, T, "u32") == (col.tobytes(), 0, None)
        res = {}
        for dtype in ("u32", "fr"):
            read = lambda: eng.read_rows([s], 0, 0, T, dtype)   # noqa: E731
            read()
            res[dtype] = median([timed(read, a.reps) for _ in range(a.rounds)])
        print(json.dumps({"metric": "typed_rows_read", "T_log2": lg, "read_u32_ms": round(res["u32"], 4),
                          "read_fr_ms": round(res["fr"], 4), "read_stages_ms": stages(lambda: eng.read_rows([s], 0, 0, T, "u32")),
                          **ident}), flush=True)
        s.release()
        eng.close()


if __name__ == "__main__":
    main()
