"""The device-built lookup multiplicities against today's route, interleaved on the same box, for T in {2^12, 2^16, 2^20}
and (L, w) in {(1, 1), (3, 1), (2, 3)}.  The input and table sets are committed once, outside the timing; the instance is a
real one (every input tuple is drawn from the table's rows, a quarter of the table repeats earlier rows).

  device  (a) kzg_rows_commit_multiplicities over the resident sets: (L + 1) w + 1 transforms, the hash join (build, L
              probes, counters -> Fr), one MSM; nothing row-sized crosses the host link
  upload  (b) kzg_rows_commit of the FINISHED m row in evaluation form from host bytes: today's route with the host's own
              join counted as FREE -- a floor under what a caller pays now
  stages  (c) the profiled stage split of (a): NTT (the transforms), POLY (the join), the MSM's stages
  host    (d) separately, the host's own join plus serialisation that (a) replaces: a dict of first occurrences over the
              table's T tuples, L T probes, T scalars to bytes -- over rows the host already holds as 32-byte strings

(a) transforms (L + 1) w rows that (b) does not and saves only the upload, so (a) >= (b) is possible; what it removes is
(d).  Before timing, (a)'s commitment is checked against (b)'s and its `missing` against 0.  One JSON line per point,
stamped with the library identity like bench.py's lines.

    python scripts/bench_multiplicities.py [--rounds 3] [--reps 5] [--sizes 12,16,20] [--shapes 1x1,3x1,2x3]"""
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


def median(xs):
    return sorted(xs)[len(xs) // 2]


def instance(L, w, T, seed):
    """(inputs, table) as lists of rows of T x 32 bytes: random table columns below 2^254, the last quarter of the table
    repeating rows of the first, every input tuple drawn from the table's rows"""
    rng = np.random.default_rng(seed)
    cols = []
    for _ in range(w):
        raw = rng.integers(0, 256, size=(T, 32), dtype=np.uint8)
        raw[:, 0] &= 0x3F   # < 2^254 < r
        cols.append(raw)
    q = T // 4
    if q:
        src = rng.integers(0, T - q, size=q)
        for raw in cols:
            raw[T - q:] = raw[src]
    inputs = []
    for _ in range(L):
        pick = rng.integers(0, T, size=T)
        inputs += [raw[pick].tobytes() for raw in cols]
    return inputs, [raw.tobytes() for raw in cols]


def host_join(inputs, table, L, w, T):
    """the host's route: first occurrences of the table's tuples, L T probes, m serialised as T x 32 bytes"""
    key = (lambda rows, t: rows[0][32 * t:32 * t + 32]) if w == 1 else \
        (lambda rows, t: b"".join(r[32 * t:32 * t + 32] for r in rows))
    first = {}
    for t in range(T):
        first.setdefault(key(table, t), t)
    mult, missing = [0] * T, 0
    for l in range(L):
        rows = inputs[l * w:(l + 1) * w]
        for t in range(T):
            at = first.get(key(rows, t))
            if at is None:
                missing += 1
            else:
                mult[at] += 1
    return b"".join(m.to_bytes(32, "big") for m in mult), missing


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed sample (the median sample is reported)")
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--shapes", default="1x1,3x1,2x3", help="n_lookups x width, comma-separated")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x5EED + lg, 0xFACADE, lg, 0)
        for L, w in [tuple(int(v) for v in x.split("x")) for x in a.shapes.split(",")]:
            inputs, table = instance(L, w, T, 100 * lg + 10 * L + w)
            t0 = time.perf_counter()
            mb, missing = host_join(inputs, table, L, w, T)
            host_ms = (time.perf_counter() - t0) * 1e3
            assert missing == 0
            F, Tb = eng.commit_rows(0, inputs), eng.commit_rows(0, table)

            def device():
                ms, miss = eng.commit_multiplicities([F], [Tb], L, w)
                ms.release()
                return ms.commitments[0], miss

            def upload():
                ms = eng.commit_rows(0, [mb])
                ms.release()
                return ms.commitments[0]

            ca, miss = device()
            assert ca == upload() and miss == 0, "device multiplicities != commit of the host-joined m"

            def timed(f):
                samples = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    f()
                    samples.append(time.perf_counter() - t0)
                return median(samples) * 1e3

            for f in (device, upload):   # warm-up: buffers, twiddles
                f()
            ta, tb = [], []
            for _ in range(a.rounds):    # interleaved: both forms see the same clock and thermal state
                ta.append(timed(device))
                tb.append(timed(upload))
            eng._chk(lib.kzg_set_profiling(eng._h, 1))
            try:
                device()
                tms = (ctypes.c_float * len(_native.TIMING_NAMES))()
                eng._chk(lib.kzg_get_timings(eng._h, tms, len(tms)))
            finally:
                eng._chk(lib.kzg_set_profiling(eng._h, 0))
            ma, mu = median(ta), median(tb)
            print(json.dumps({"metric": "multiplicities", "T_log2": lg, "n_lookups": L, "width": w, "device_ms": round(ma, 4),
                              "upload_ms": round(mu, 4), "device_over_upload": round(ma / mu, 3),
                              "host_join_ms": round(host_ms, 2),
                              "device_rounds_ms": [round(x, 4) for x in ta], "upload_rounds_ms": [round(x, 4) for x in tb],
                              "device_stages_ms": {n: round(v, 4) for n, v in zip(_native.TIMING_NAMES, tms) if v},
                              "checked": True, **ident}), flush=True)
            for s in (F, Tb):
                s.release()
        eng.close()


if __name__ == "__main__":
    main()
