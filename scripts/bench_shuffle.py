"""The device-built shuffle running product against the permutation grand product over the same number of rows, interleaved on
the same box, for T in {2^16, 2^20}.  Every set is committed once, outside the timing.

  shuffle        worker_commit_shuffle for (G, w) = (1, 1), (1, 3), (2, 2) without selectors, and (1, 3) with one selector
                 per side: 2 G w (+ 2) + 1 transforms, the Horner and factor kernels, the scans, one inversion, one MSM
  grand product  worker_commit_grand_product with k = G w: the same 2 G w + 1 transforms through k_gp_factors -- code the
                 shuffle does not touch, so it is the yardstick

Per configuration the two calls are timed in interleaved rounds and the profiled stage split of each (ntt / poly / accumulate
...) is reported beside the ratio, so that a gap can be laid at a kernel's door.  One JSON line per point, stamped with the
library identity like bench.py's lines.

    python scripts/bench_shuffle.py [--rounds 3] [--reps 5] [--sizes 16,20]"""
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
from zkp_subnet_amd import HipEngine, _native, codec  # noqa: E402
from zkp_subnet_amd.client import Client  # noqa: E402
from zkp_subnet_amd.engine import R_MODULUS as R  # noqa: E402

CONFIGS = [(1, 1, False), (1, 3, False), (2, 2, False), (1, 3, True)]   # (G, w, one selector per side)


def rand_row(T, seed):
    raw = np.random.default_rng(seed).integers(0, 256, size=(T, 32), dtype=np.uint8)
    raw[:, 0] &= 0x3F   # < 2^254 < r
    return raw.tobytes()


def bool_row(T, seed):
    raw = np.zeros((T, 32), dtype=np.uint8)
    raw[:, 31] = np.random.default_rng(seed).integers(0, 2, size=T, dtype=np.uint8)
    return raw.tobytes()


def fr(v):
    return codec.be32_to_fr((v % R).to_bytes(32, "big"))


def median(xs):
    return sorted(xs)[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed sample (the median sample is reported)")
    ap.add_argument("--sizes", default="16,20")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x5EED + lg, 0xFACADE, lg, 0)
        cl = Client(engine=eng)
        for G, w, sel in CONFIGS:
            k = G * w
            A = eng.commit_rows(0, [rand_row(T, 100 * lg + j) for j in range(k)])
            B = eng.commit_rows(0, [rand_row(T, 100 * lg + 50 + j) for j in range(k)])
            Q = eng.commit_rows(0, [bool_row(T, 100 * lg + 90), bool_row(T, 100 * lg + 91)]) if sel else None
            theta, gamma, beta = fr(0x7E7A + lg), fr(0x6A44A + k), fr(0xBE7A + lg)
            shifts = [fr(pow(7, j, R)) for j in range(k)]
            kw = dict(sel_handles=[Q.handle], input_sel=[0] * G, shuffle_sel=[1] * G) if sel else {}

            def call(r):
                assert r.status_code == 200, r.json()
                assert cl.worker_release_rows(r.json()["handle"]).status_code == 200
                return r.json()["commitment"]

            def shuffle():
                return call(cl.worker_commit_shuffle([A.handle], [B.handle], G, w, theta, gamma, **kw))

            def grand_product():
                return call(cl.worker_commit_grand_product([A.handle], [B.handle], shifts, beta, gamma))

            def timed(f):
                samples = []
                for _ in range(a.reps):
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

            assert shuffle() == shuffle()
            for f in (shuffle, grand_product):   # warm-up: buffers, twiddles
                f()
            ts, tg = [], []
            for _ in range(a.rounds):            # interleaved: both calls see the same clock and thermal state
                ts.append(timed(shuffle))
                tg.append(timed(grand_product))
            ms, mg = median(ts), median(tg)
            print(json.dumps({"metric": "shuffle", "T_log2": lg, "n_groups": G, "width": w, "selectors": sel,
                              "shuffle_ms": round(ms, 4), "grand_product_ms": round(mg, 4),
                              "shuffle_over_grand_product": round(ms / mg, 3),
                              "shuffle_rounds_ms": [round(x, 4) for x in ts], "grand_product_rounds_ms": [round(x, 4) for x in tg],
                              "shuffle_stages_ms": stages(shuffle), "grand_product_stages_ms": stages(grand_product),
                              **ident}), flush=True)
            for s in (A, B, Q):
                if s is not None:
                    s.release()
        eng.close()


if __name__ == "__main__":
    main()
