"""The device-built permutation grand product against today's route, interleaved on the same box, for T in {2^12, 2^16,
2^20} and k in {3, 5}.  The wire and sigma sets are committed once, outside the timing.

  device  (a) kzg_rows_commit_grand_product over the resident sets: 2k + 1 transforms, the product kernels, one inversion,
              one MSM; nothing row-sized crosses the host link
  upload  (b) kzg_rows_commit of ONE precomputed z row in evaluation form from host bytes: today's route with the host's
              own arithmetic (T * 2k field products, T inversions) counted as FREE -- a floor under what a caller pays now
  stages  (c) the profiled stage split of (a), and the device-side inversion alone (its test hook, one lane, against the
              same hook call doing one product)

(a) does transforms and scans that (b) does not and saves only the upload, so (a) >= (b) is possible; the ratio is reported
per size with the split that explains it.  Before timing, (a)'s commitment is checked against (b)'s (z computed here from
the definition in Python integers).  One JSON line per point, stamped with the library identity like bench.py's lines.

    python scripts/bench_grand_product.py [--rounds 3] [--reps 5] [--sizes 12,16,20] [--ks 3,5]"""
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
from zkp_subnet_amd.engine import R_MODULUS as R, _root_of_unity  # noqa: E402


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


def z_row(wires, sigmas, shifts, beta, gamma):
    """z's T evaluations from the definition (one batch inversion), as the bytes route (b) uploads"""
    T = len(wires[0])
    w, x = _root_of_unity(T), 1
    N, D = [1] * T, [1] * T
    for t in range(T):
        for a, sg, s in zip(wires, sigmas, shifts):
            N[t] = N[t] * (a[t] + beta * s % R * x + gamma) % R
            D[t] = D[t] * (a[t] + beta * sg[t] + gamma) % R
        x = x * w % R
    pre, acc = [], 1
    for d in D:
        pre.append(acc)
        acc = acc * d % R
    inv, Dinv = pow(acc, -1, R), [0] * T
    for t in range(T - 1, -1, -1):
        Dinv[t] = inv * pre[t] % R
        inv = inv * D[t] % R
    out, acc = [], 1
    for n, di in zip(N, Dinv):
        out.append(be(acc))
        acc = acc * n % R * di % R
    return b"".join(out), acc


def inversion_ms(eng, reps=21):
    """one device-side inversion: the wall time of the one-element hook call minus that of the same call doing one product
    (same upload, launch, read-back), medians of `reps`"""
    x = be(0x7654321 << 200)

    def wall(op):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            eng.test_field(1, op, x, x)
            ts.append(time.perf_counter() - t0)
        return median(ts) * 1e3

    wall(7), wall(0)   # (the first launches page the code in)
    return max(wall(7) - wall(0), 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed sample (the median sample is reported)")
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--ks", default="3,5")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x5EED + lg, 0xFACADE, lg, 0)
        inv_ms = inversion_ms(eng)
        for k in [int(x) for x in a.ks.split(",")]:
            wires = [rand_row(T, 100 * lg + j) for j in range(k)]
            sigmas = [rand_row(T, 100 * lg + 50 + j) for j in range(k)]
            shifts, beta, gamma = [pow(7, j, R) for j in range(k)], 0xBE7A + lg, 0x6A44A + k
            zb, closing = z_row([ints(r) for r in wires], [ints(r) for r in sigmas], shifts, beta, gamma)
            W, S = eng.commit_rows(0, wires), eng.commit_rows(0, sigmas)
            sh, bb, gb = [be(s) for s in shifts], be(beta), be(gamma)

            def device():
                zs, cl = eng.commit_grand_product([W], [S], sh, bb, gb)
                zs.release()
                return zs.commitments[0], cl

            def upload():
                zs = eng.commit_rows(0, [zb])
                zs.release()
                return zs.commitments[0]

            ca, cl = device()
            assert ca == upload() and cl == be(closing), "device grand product != commit of the host-computed z"

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
            print(json.dumps({"metric": "grand_product", "T_log2": lg, "k": k, "device_ms": round(ma, 4),
                              "upload_ms": round(mb, 4), "device_over_upload": round(ma / mb, 3),
                              "device_rounds_ms": [round(x, 4) for x in ta], "upload_rounds_ms": [round(x, 4) for x in tb],
                              "device_stages_ms": {n: round(v, 4) for n, v in zip(_native.TIMING_NAMES, tms) if v},
                              "inversion_ms": round(inv_ms, 4), "checked": True, **ident}), flush=True)
            W.release()
            S.release()
        eng.close()


if __name__ == "__main__":
    main()
