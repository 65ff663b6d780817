"""The device-built PLONK quotient against today's route, interleaved on the same box, for T in {2^12, 2^16, 2^20} and the
standard shape (13 rows, k = 3, ext_log = 2, three pieces).  The 13 rows are committed once, outside the timing.

  device  (a) kzg_rows_commit_quotient over the resident sets: 14 forward transforms of length 4T and one inverse, the
              pointwise kernels, one MSM pass of three scalar sets; nothing row-sized crosses the host link
  upload  (b) kzg_rows_commit of THREE precomputed piece rows in coefficient form from host bytes: today's route with the
              host's own arithmetic (a dozen size-4T transforms, 28 field products per point) counted as FREE -- a floor
              under what a caller pays now
  stages  (c) the profiled stage split of (a): NTT against POLY (and the MSM stages)

(a) does transforms that (b) does not and saves only the upload, so (a) >= (b) is possible; the ratio is reported per size
with the split that explains it.  The instance is a satisfied circuit with a NON-TRIVIAL permutation (three pairs of cells
swapped, with equal wire values; random wires, selectors and public inputs, qC solved per row), so that z is not constant,
P1 does not vanish and t has its full degree 3T - 4: all three pieces are dense, and the MSM of (a) carries three full
scalar sets (the MSM skips zero digits: an identity permutation would leave the third piece zero and flatter (a)).  z is
built on the device by kzg_rows_commit_grand_product, outside the timing; its closing value must be 1, the device's shape
check confirms the instance on every call, and the third commitment is checked not to be the point at infinity.  At sizes
up to --check-max the pieces are also computed here (tests/quotient_ref.py), (a)'s commitments are compared with (b)'s of
those rows and (b) is timed on them; above, (b) uploads three dense random rows of the same size (its time depends on
their density, not their values).  One JSON line per size, stamped with the library identity like bench.py's lines.

    python scripts/bench_quotient.py [--rounds 3] [--reps 5] [--sizes 12,16,20] [--check-max 16]"""
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
from zkp_subnet_amd.engine import R_MODULUS as R, _root_of_unity  # noqa: E402

# row order: a b c | qL qR qO qM qC PI | sigma1 sigma2 sigma3 | z  (three sets and the device-built z)
TERMS = [(1, [3, 0]), (1, [4, 1]), (1, [5, 2]), (1, [6, 0, 1]), (1, [7]), (1, [8])]
SHIFTS = [1, 7, 49]


def be(v):
    return (v % R).to_bytes(32, "big")


def median(xs):
    return sorted(xs)[len(xs) // 2]


def instance(T, seed):
    """(wires, selectors + PI, sigmas) as evaluation rows of a satisfied circuit: the identity permutation with three pairs
    of cells swapped (their wire values made equal), random wires, selectors and public inputs, qC solved per row"""
    rnd = random.Random(seed)
    rr = lambda: [rnd.getrandbits(254) for _ in range(T)]   # noqa: E731
    a, b, c, ql, qr_, qo, qm, pi = (rr() for _ in range(8))
    wires = [a, b, c]
    w, x, dom = _root_of_unity(T), 1, []
    for _ in range(T):
        dom.append(x)
        x = x * w % R
    sig = [[s * x % R for x in dom] for s in SHIFTS]
    ts = rnd.sample(range(T), 6)
    for (j1, t1), (j2, t2) in (((0, ts[0]), (1, ts[1])), ((2, ts[2]), (0, ts[3])), ((1, ts[4]), (1, ts[5]))):
        wires[j2][t2] = wires[j1][t1]
        sig[j1][t1], sig[j2][t2] = SHIFTS[j2] * dom[t2] % R, SHIFTS[j1] * dom[t1] % R
    qc = [-(ql[t] * a[t] + qr_[t] * b[t] + qo[t] * c[t] + qm[t] * a[t] % R * b[t] + pi[t]) % R for t in range(T)]
    return wires, [ql, qr_, qo, qm, qc, pi], sig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed sample (the median sample is reported)")
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--check-max", type=int, default=16, help="largest log2 size whose pieces are recomputed here and compared")
    a = ap.parse_args()
    ident = identity()
    lib = _native.load()
    for lg in [int(x) for x in a.sizes.split(",")]:
        T = 1 << lg
        eng = HipEngine(0)
        eng.gen_srs(0x5EED + lg, 0xFACADE, lg, 0)
        wires, sels, sig = instance(T, 77 + lg)
        perm = {"wires": [0, 1, 2], "sigmas": [9, 10, 11], "z": 12, "shifts": SHIFTS, "beta": 0xBE7A + lg, "gamma": 0x6A44A,
                "alpha": 0xA1FA + lg}
        rb = lambda rows: [b"".join(be(v) for v in r) for r in rows]   # noqa: E731
        W, Q, SG = eng.commit_rows(0, rb(wires)), eng.commit_rows(0, rb(sels)), eng.commit_rows(0, rb(sig))
        Z, closing = eng.commit_grand_product([W], [SG], [be(s) for s in SHIFTS], be(perm["beta"]), be(perm["gamma"]))
        assert closing == be(1), "the permutation does not close"
        S = [W, Q, SG, Z]
        bt = [(be(c), idx) for c, idx in TERMS]
        bp = dict(perm, shifts=[be(s) for s in SHIFTS], beta=be(perm["beta"]), gamma=be(perm["gamma"]), alpha=be(perm["alpha"]))
        checked = lg <= a.check_max
        if checked:
            from tests import grand_product_ref as gref, quotient_ref as qref
            z, cl = gref.grand_product(wires, sig, SHIFTS, perm["beta"], perm["gamma"])
            assert cl == 1 and len(set(z)) > 1
            t, rem = qref.quotient([qref.coeffs_of(r) for r in wires + sels + sig + [z]], TERMS, perm, 2)
            assert not any(rem) and qref.degree(t) == 3 * T - 4
            piece_rows = [qref.row_bytes(p) for p in qref.pieces(t, T, 3)]
        else:
            piece_rows = rb(wires)   # three dense rows of the same size
        del wires, sels, sig

        def device():
            ts = eng.commit_quotient(S, bt, bp, 2, 3)
            ts.release()
            return ts.commitments

        def upload():
            ts = eng.commit_rows(0, piece_rows, False)
            ts.release()
            return ts.commitments

        got = device()
        assert all(not c[0] & 0x40 for c in got), "a piece commitment is the point at infinity: the instance is degenerate"
        if checked:
            assert got == upload(), "device quotient pieces != commit of the host-computed pieces"

        def timed(f):
            samples = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                f()
                samples.append(time.perf_counter() - t0)
            return median(samples) * 1e3

        for f in (device, upload):   # warm-up: workspace, twiddles, constants
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
        st = dict(zip(_native.TIMING_NAMES, tms))
        ma, mb = median(ta), median(tb)
        print(json.dumps({"metric": "quotient", "T_log2": lg, "rows": 13, "k": 3, "ext_log": 2, "n_pieces": 3,
                          "device_ms": round(ma, 4), "upload_ms": round(mb, 4), "device_over_upload": round(ma / mb, 3),
                          "device_rounds_ms": [round(x, 4) for x in ta], "upload_rounds_ms": [round(x, 4) for x in tb],
                          "device_stages_ms": {n: round(v, 4) for n, v in st.items() if v},
                          "ntt_ms": round(st["ntt"], 4), "poly_ms": round(st["poly"], 4), "checked": checked, **ident}),
              flush=True)
        for x in S:
            x.release()
        eng.close()


if __name__ == "__main__":
    main()
