"""The device-built lookup (logUp) running sum against today's route, interleaved on the same box, for T in {2^12, 2^16,
2^20} and (L, w) in {(1, 1), (4, 1), (4, 3)}.  The input, table and multiplicity sets are committed once, outside the timing.

  device  (a) kzg_rows_commit_lookup_sum over the resident sets: (L + 1) w + 2 transforms, the fraction kernels, the batched
              inversion (one device-side inversion), the additive scan, one MSM; nothing row-sized crosses the host link
  upload  (b) kzg_rows_commit of ONE precomputed S row in evaluation form from host bytes: today's route with the host's
              own arithmetic (T * (L + 1) inversions) counted as FREE -- a floor under what a caller pays now
  stages  (c) the profiled stage split of (a), and the batched inversion alone (its test hook, Fr op 9 at n = T, against the
              same hook call doing n products; and op 7, the lone-lane inversion, for one element)

(a) does transforms and scans that (b) does not and saves only the upload, so (a) >= (b) is possible; the ratio is reported
per size with the split that explains it.  Before timing, (a)'s commitment is checked against (b)'s (S computed here from
the definition in Python integers).  One JSON line per point, stamped with the library identity like bench.py's lines.

    python scripts/bench_lookup_sum.py [--rounds 3] [--reps 5] [--sizes 12,16,20] [--shapes 1x1,4x1,4x3]"""
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
from zkp_subnet_amd.engine import R_MODULUS as R  # noqa: E402


def rand_row(T, seed):
    raw = np.random.default_rng(seed).integers(0, 256, size=(T, 32), dtype=np.uint8)
    raw[:, 0] &= 0x3F   # < 2^254 < r
    return raw.tobytes()


def ints(b):
    return [int.from_bytes(b[i:i + 32], "big") for i in range(0, len(b), 32)]


def be(v):
    return (v % R).to_bytes(32, "big")


def median(xs):
    return sorted(xs)[len(xs) // 2]


def batch_inverse(vals):
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % R
    inv, out = pow(acc, -1, R), [0] * len(vals)
    for t in range(len(vals) - 1, -1, -1):
        out[t] = inv * pre[t] % R
        inv = inv * vals[t] % R
    return out


def s_row(inputs, table, mult, L, w, theta, beta):
    """S's T evaluations from the definition (one batch inversion), as the bytes route (b) uploads"""
    T = len(mult)

    def compress(cols):
        out = [0] * T
        for col in reversed(cols):
            out = [(o * theta + v) % R for o, v in zip(out, col)]
        return out

    dens = []
    for l in range(L):
        dens += [(beta + f) % R for f in compress(inputs[l * w:(l + 1) * w])]
    dens += [(beta + f) % R for f in compress(table)]
    inv = batch_inverse(dens)
    out, acc = [], 0
    for t in range(T):
        out.append(be(acc))
        acc = (acc + sum(inv[l * T + t] for l in range(L)) - mult[t] * inv[L * T + t]) % R
    return b"".join(out), acc


def hook_ms(eng, op, data, reps=11):
    """wall time of one kzg_test_field call (upload, kernels, read-back), median of `reps`"""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        eng.test_field(1, op, data, data)
        ts.append(time.perf_counter() - t0)
    return median(ts) * 1e3


def inversion_ms(eng, T):
    """(the batched inversion of T elements, one lone-lane inversion): each the wall time of its hook call minus that of the
    same call doing one product per element (same upload, launch, read-back)"""
    row, x = rand_row(T, 4242), be(0x7654321 << 200)
    for op, d in ((9, row), (0, row), (7, x), (0, x)):   # (the first launches page the code in)
        hook_ms(eng, op, d, 2)
    return max(hook_ms(eng, 9, row) - hook_ms(eng, 0, row), 0.0), max(hook_ms(eng, 7, x, 21) - hook_ms(eng, 0, x, 21), 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed sample (the median sample is reported)")
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--shapes", default="1x1,4x1,4x3", help="n_lookups x width, comma-separated")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x5EED + lg, 0xFACADE, lg, 0)
        binv_ms, inv_ms = inversion_ms(eng, T)
        for L, w in [tuple(int(v) for v in x.split("x")) for x in a.shapes.split(",")]:
            inputs = [rand_row(T, 100 * lg + j) for j in range(L * w)]
            table = [rand_row(T, 100 * lg + 50 + j) for j in range(w)]
            mult = rand_row(T, 100 * lg + 99)
            theta, beta = 0x7E7A + lg, 0xBE7A + L
            sb, closing = s_row([ints(r) for r in inputs], [ints(r) for r in table], ints(mult), L, w, theta, beta)
            F, Tb, M = eng.commit_rows(0, inputs), eng.commit_rows(0, table), eng.commit_rows(0, [mult])
            tb_, bb = be(theta), be(beta)

            def device():
                ss, cl = eng.commit_lookup_sum([F], [Tb], M, L, w, tb_, bb)
                ss.release()
                return ss.commitments[0], cl

            def upload():
                ss = eng.commit_rows(0, [sb])
                ss.release()
                return ss.commitments[0]

            ca, cl = device()
            assert ca == upload() and cl == be(closing), "device lookup sum != commit of the host-computed S"

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
            ma, mb = median(ta), median(tb)
            print(json.dumps({"metric": "lookup_sum", "T_log2": lg, "n_lookups": L, "width": w, "device_ms": round(ma, 4),
                              "upload_ms": round(mb, 4), "device_over_upload": round(ma / mb, 3),
                              "device_rounds_ms": [round(x, 4) for x in ta], "upload_rounds_ms": [round(x, 4) for x in tb],
                              "device_stages_ms": {n: round(v, 4) for n, v in zip(_native.TIMING_NAMES, tms) if v},
                              "batch_inversion_ms": round(binv_ms, 4), "inversion_ms": round(inv_ms, 4), "checked": True,
                              **ident}), flush=True)
            for s in (F, Tb, M):
                s.release()
        eng.close()


if __name__ == "__main__":
    main()
