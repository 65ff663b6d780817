"""GPU parity tests (`-m gpu`), multi: several ranks / several contexts: the library's RCCL collective, the stream-chained pair, the plain-C caller, the multi-device handles -- and the device-count-gated tests that run on REAL N > 1 GPUs the moment they are visible.
Every result of the HIP path, obtained through the C-ABI, is compared bit-for-bit with the CPU oracle on the same seeded inputs,
with the committed golden fixtures, and -- at BASELINE.json's full sizes -- through size-independent properties (trapdoor
identity [f(tau)]G, linearity, NTT round trip).  All arithmetic is integer: the bar is bit-exact, no tolerance anywhere."""
import base64  # noqa: F401
import json  # noqa: F401
import os
import random  # noqa: F401

import numpy as np  # noqa: F401
import pytest

from oracle import bls12_381 as o  # noqa: F401
from oracle import cpu as oc  # noqa: F401
from tests.gpu_common import ROOT, H, ints, rand_scalars_bytes  # noqa: F401

pytestmark = pytest.mark.gpu


def test_two_processes_sharded_msm_on_one_gpu(hip):
    """Two REAL processes (fresh interpreters, torch.distributed gloo group), each with its own HipEngine on this GPU
    holding its own SRS segment, run zkp_subnet_amd.distributed.sharded_msm: the result of every rank equals the
    single-process MSM over the whole SRS and the trapdoor value."""
    import subprocess
    import sys

    lg = 17
    n = 1 << lg
    tx = 0xD157D157D157
    procs = []
    port = 29500 + (os.getpid() % 400)
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dist_hip_worker.py"), str(lg), hex(tx)],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT))
    outs = []
    for p in procs:
        so, se = p.communicate(timeout=900)
        assert p.returncode == 0, se[-3000:]
        outs.append(so.strip().splitlines()[-1])
    assert outs[0] == outs[1]
    eng = hip()
    eng.gen_srs(tx, 1, lg + 1, 0)
    whole = rand_scalars_bytes(n, 7000) + rand_scalars_bytes(n, 7001)
    assert eng.msm(whole, 0).hex() == outs[0]
    assert outs[0] == oc.g1_mul_gen(oc.fr_eval(whole, tx.to_bytes(32, "big"))).hex()
    eng.close()


def test_stream_chained_collective_step_one_rank_rccl(hip):
    """kzg_msm_sharded_begin / _finish (the engine's lane, torch's stream with RCCL behind it, and the lane again chained
    by events: one host synchronisation per MSM) against the blocking pair and the plain MSM, in a fresh process holding
    a one-rank RCCL group (N > 1 ranks cannot share this box's single GPU)."""
    import subprocess
    import sys

    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dist_rccl_onerank.py"), "29551"], capture_output=True,
                         text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])   # RCCL prints its banner after it
    assert set(rec) == {"6", "12", "16"}
    for lg, r in rec.items():
        assert r["chained_equal"] and r["blocking_equal"] and r["segment_equal"] and len(r["plain"]) == 96, (lg, r)


def test_library_collective_one_rank_no_torch(hip):
    """kzg_comm_init / kzg_msm_sharded (the all_gather is the LIBRARY's, enqueued on the lane's own stream)
    in a fresh process without torch: sharded == plain MSM == oracle, from four host threads, a forced timeout aborts the
    communicator with KZG_E_COMM inside the budget, and a rebuilt communicator serves again."""
    import subprocess
    import sys

    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "comm_onerank.py")], capture_output=True, text=True,
                         timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
    assert set(rec) == {"6", "12", "16", "20"}
    for lg, r in rec.items():
        n = 1 << int(lg)
        raw = np.random.default_rng(int(lg)).integers(0, 256, size=(n, 32), dtype=np.uint8)
        raw[:, 0] &= 0x3F
        want = oc.g1_mul_gen(oc.fr_eval(raw.tobytes(), (0x51AB1E + int(lg)).to_bytes(32, "big")))   # trapdoor: [f(tau)] G
        assert r["plain"] == want.hex(), lg
        assert r["without_comm"] is True and r["double_init"] is True, (lg, r)
        assert r["sharded_equal"] and r["segment_equal"] and r["threads_equal"], (lg, r)
        assert r["info"]["world"] == 1 and r["info"]["rank"] == 0 and r["info"]["rccl_version_code"] > 20000 and not r["info"]["broken"]
        assert r["collective_ms"] > 0 and r["world_after_destroy"] == 0, (lg, r)
    t = rec["12"]
    assert t["timeout"] is True and t["broken"] and t["after_abort"] is True and t["plain_after_abort"] and t["rebuilt_equal"], t
    # detected after the 100-ms budget; the call returns once its lane has drained (here: when the 400-ms stall kernel ends;
    # after a real abort the collective leaves the stream at once)
    assert 90 < t["timeout_after_ms"] < 3000, t


def _build_native_caller(tmp_path):
    import subprocess

    exe = str(tmp_path / "native_caller")
    libdir = os.path.join(ROOT, "zkp_subnet_amd")
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "native_caller.c"), "-o", exe, "-L", libdir, "-lkzg_mi355x", "-Wl,-rpath," + libdir,
           "-Wl,--allow-shlib-undefined"]      # (the sanitizer builds of the library resolve their runtime at load time)
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    return exe


def test_c_abi_from_a_native_caller(hip, tmp_path):
    """INTEGRATION.md section 3 as a real program: tests/native_caller.c (C99, gcc, the public header, no Python or torch
    in the process) drives kzg_create / kzg_gen_srs / kzg_msm / kzg_upload_fr / kzg_msm_resident / the library's own
    collective on a one-rank communicator / kzg_commit_open; every line it prints equals the CPU oracle's answer."""
    import subprocess

    lg = 12
    n = 1 << lg
    tau = 0xC0FFEE1234567
    scal = rand_scalars_bytes(n, 4242)
    path = tmp_path / "scalars.bin"
    path.write_bytes(scal)
    exe = _build_native_caller(tmp_path)
    out = subprocess.run([exe, str(lg), tau.to_bytes(32, "big").hex(), str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stdout[-1000:], out.stderr[-2000:])
    got = dict(ln.split(" ", 1) for ln in out.stdout.splitlines() if " " in ln)
    srs = oc.srs_gen(tau.to_bytes(32, "big"), (1).to_bytes(32, "big"), lg, 0, 0)
    want = oc.msm(srs, scal).hex()
    assert got["msm"] == got["msm_resident"] == got["msm_sharded"] == want
    alpha = scal[32:64]
    assert got["commitment"] == oc.commit(srs, scal, True).hex()
    ev, pf = oc.open_(srs, scal, alpha, True)
    assert (got["eval"], got["proof"]) == (ev.hex(), pf.hex())
    assert got["comm"].startswith("rank 0 world 1 rccl 2") and got["comm"].endswith("broken 0")
    assert got["sharded_without_comm"] == "-1" and got["bad_worker_index"] == "-1" and "gfx950" in got["version"]
    assert got["multi"] == "devices 2 device_of_1 0" and got["multi_commitment"] == got["commitment"] and got["multi_bad_index"] == "-1"


def test_native_multi_device_handle_routes_rows_by_worker_index(hip):
    """kzg_multi_* (SURVEY 8b's kzg_create(device_count, device_ids)): G contexts behind one handle, worker index i served by
    context i mod G holding only the slices it serves (here G = 3 contexts on this box's one GPU, 8 worker rows).  Every
    commit / open / commit+open equals the oracle's answer for THAT worker's slice; the rows of a challenge fan out with a
    status per row -- a bad row (non-canonical scalar) costs only itself."""
    import ctypes

    from zkp_subnet_amd import _native
    from zkp_subnet_amd.engine import lagrange_factor

    lib = _native.load()
    scale, ms = 13, 3
    T, M, G = 1 << (scale - ms), 1 << ms, 3
    tx, ty = 0xABCDEF0123, 0x13579BDF
    devs = (ctypes.c_int * G)(0, 0, 0)
    m = ctypes.c_void_p()
    assert lib.kzg_multi_create(G, devs, ctypes.byref(m)) == 0
    try:
        assert lib.kzg_multi_count(m) == G and lib.kzg_multi_device_of(m, 5) == 0
        out = ctypes.create_string_buffer(48)
        assert lib.kzg_multi_commit(m, 0, bytes(32 * T), T, 1, out) == _native.KZG_E_ARG          # nothing resident yet
        s0 = b"".join(lagrange_factor(i, ms, ty).to_bytes(32, "big") for i in range(M))
        assert lib.kzg_multi_gen_srs(m, tx.to_bytes(32, "big"), s0, scale, ms) == 0
        alpha = rand_scalars_bytes(1, 9100)
        rows = [rand_scalars_bytes(T, 9000 + i) for i in range(M)]
        want = []
        for i in range(M):
            srs = oc.srs_gen(tx.to_bytes(32, "big"), ty.to_bytes(32, "big"), scale, ms, i)
            want.append((oc.commit(srs, rows[i], True),) + oc.open_(srs, rows[i], alpha, True))
        c, e, p = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.create_string_buffer(48)
        for i in (0, 1, 2, 5, 7):
            assert lib.kzg_multi_commit(m, i, rows[i], T, 1, c) == 0 and c.raw == want[i][0], i
            assert lib.kzg_multi_open(m, i, rows[i], T, 1, alpha, e, p) == 0 and (e.raw, p.raw) == want[i][1:], i
            assert lib.kzg_multi_commit_open(m, i, rows[i], T, 1, alpha, c, e, p) == 0 and (c.raw, e.raw, p.raw) == want[i], i
        assert lib.kzg_multi_commit(m, M, rows[0], T, 1, c) == _native.KZG_E_ARG
        assert b"worker index" in lib.kzg_multi_last_error(m)
        # the rows of one challenge over all "devices" at once, in a shuffled order, one row poisoned
        order = [6, 1, 4, 7, 0, 3, 2, 5]
        idx = (ctypes.c_uint32 * M)(*order)
        blob = bytearray(b"".join(rows[i] for i in order))
        blob[32 * T * 2: 32 * T * 2 + 32] = b"\xff" * 32                       # row k = 2 (worker 4): a scalar >= r
        oc_, oe_, op_ = (ctypes.create_string_buffer(n * M) for n in (48, 32, 48))
        st = (ctypes.c_int * M)()
        rc = lib.kzg_multi_commit_open_rows(m, M, idx, bytes(blob), T, 1, alpha, oc_, oe_, op_, st)
        assert rc == _native.KZG_E_SCALAR and b"row 2 (worker 4)" in lib.kzg_multi_last_error(m)
        for k, i in enumerate(order):
            if k == 2:
                assert st[k] == _native.KZG_E_SCALAR
                continue
            assert st[k] == 0 and (oc_.raw[48 * k:48 * k + 48], oe_.raw[32 * k:32 * k + 32], op_.raw[48 * k:48 * k + 48]) == want[i], (k, i)
        # each context holds only the slices of its own workers: 8 rows over 3 contexts = 3 + 3 + 2 slices
        assert [lib.kzg_srs_points(lib.kzg_multi_ctx(m, g)) // T for g in range(G)] == [3, 3, 2]
        assert lib.kzg_multi_ctx(m, G) is None
    finally:
        lib.kzg_multi_destroy(m)


def test_multi_device_client_two_contexts_on_one_gpu():
    """MultiDeviceClient with G = 2 contexts (both on device 0: this box has one GPU; on a multi-GPU host the list names
    different devices): worker index i is served by context i mod 2, each context generated only its own slices, the four
    rows of a challenge run concurrently from host threads, and every commitment / evaluation / proof equals the C
    oracle's on the same slice."""
    from zkp_subnet_amd import MultiDeviceClient, codec
    from zkp_subnet_amd.client import derive_taus
    from zkp_subnet_amd.validator import generate_challenge, verify_all

    lg, ms = 12, 2
    multi = MultiDeviceClient(devices=[0, 0], seed=77)
    multi.start(scale=lg, machines_scale=ms)
    try:
        assert [c.workers for c in multi.clients] == [[0, 2], [1, 3]]
        ch = generate_challenge(multi, 4)
        answers = multi.commit_and_open_rows(range(4), ch.polys, ch.alpha)
        tx, ty = (t.to_bytes(32, "big") for t in derive_taus(77))
        alpha = codec.fr_to_be32(ch.alpha)
        for i, a in enumerate(answers):
            assert a.status_code == 200, a.json()
            srs = oc.srs_gen(tx, ty, lg, ms, i)
            row = codec.fr_list_to_be32(ch.polys[i])
            ev, pf = oc.open_(srs, row, alpha, True)
            assert codec.g1_from_b64(a.json()["commitment"]) == oc.commit(srs, row, True), i
            assert (codec.fr_to_be32(a.json()["eval"]), codec.g1_from_b64(a.json()["proof"])) == (ev, pf), i
            assert a.json()["eval"] == ch.evals[i]                 # the validator's own evaluation, from the other path
        from zkp_subnet_amd.protocol import Prove
        responses = [Prove(index=i, poly=[], commitment=a.json()["commitment"], proof=a.json()["proof"], eval=a.json()["eval"])
                     for i, a in enumerate(answers)]
        assert verify_all(multi, ch, responses, threads=4) == [True] * 4
    finally:
        multi.stop()


# ------------------------------------------------------------------ round 6: robustness of the collective, one handle over G contexts
def _last_json(stdout):
    return json.loads([ln for ln in stdout.splitlines() if ln.startswith("{")][-1])


def test_comm_init_with_an_absent_peer_gives_up_inside_its_budget_and_leaves_a_working_context():
    """kzg_comm_init_bounded: world = 2, rank 1 never arrives.  KZG_E_COMM after the 1.5-s budget (not a parked thread
    holding every lane), then plain MSMs, a fresh communicator + sharded MSM, close() and a NORMAL interpreter exit."""
    import subprocess
    import sys

    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "comm_absent_peer.py")], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert out.returncode == 0, (out.returncode, out.stderr[-3000:])
    r = _last_json(out.stdout)
    raw = np.random.default_rng(77).integers(0, 256, size=(1 << 12, 32), dtype=np.uint8)
    raw[:, 0] &= 0x3F
    want = oc.g1_mul_gen(oc.fr_eval(raw.tobytes(), (0xAB5E47).to_bytes(32, "big"))).hex()
    assert r["absent_peer"] is True and "did not all join" in r["message"], r
    assert 1.4 < r["gave_up_after_s"] < 10, r
    assert r["info_after"]["world"] == 0 and not r["info_after"]["broken"], r
    assert r["plain"] == want and r["plain_after"] == want and r["sharded_after"] == want and r["closed"], r


def test_a_timeout_on_one_lane_never_lets_another_lane_return_a_result(hip):
    """two sharded MSMs in flight on two lanes of one communicator.  The first overruns its 300-ms budget and
    aborts the communicator; the second (generous budget, its own collective still queued behind its stall) finds a complete
    record after its wait -- computed under an aborted communicator.  It must return KZG_E_COMM, never bytes."""
    import threading
    import time

    from zkp_subnet_amd import KzgError
    from zkp_subnet_amd._native import KZG_E_COMM

    lg = 12
    n = 1 << lg
    eng = hip()
    eng.gen_srs(0xFACADE, 1, lg, 0)
    eng.upload_fr(0, rand_scalars_bytes(n, 31), False)
    plain = eng.msm_resident(0, n, 0)
    eng.comm_init(eng.comm_unique_id(), 0, 1, init_timeout_ms=60000)
    assert eng.msm_sharded(0, n, 0) == plain
    res = {}

    def call(name):
        try:
            res[name] = eng.msm_sharded(0, n, 0)
        except KzgError as e:
            res[name] = e

    eng._chk(eng._lib.kzg_test_comm_stall_n(eng._h, 1000, 2))     # both calls meet a "peer" that is 1 s late
    eng.comm_set_timeout(300)
    a = threading.Thread(target=call, args=("a",))
    a.start()
    time.sleep(0.1)                                               # a has read its 300-ms budget and is queued
    eng.comm_set_timeout(20000)                                   # b would wait 20 s for ITS collective
    b = threading.Thread(target=call, args=("b",))
    b.start()
    a.join(30)
    b.join(30)
    assert not a.is_alive() and not b.is_alive()
    assert isinstance(res["a"], KzgError) and res["a"].code == KZG_E_COMM, res["a"]
    assert isinstance(res["b"], KzgError) and res["b"].code == KZG_E_COMM, res["b"]      # NOT bytes
    assert eng.comm_info()["broken"]
    assert eng.msm_resident(0, n, 0) == plain                     # the rest of the library is unharmed
    eng.comm_destroy()
    eng.comm_init(eng.comm_unique_id(), 0, 1, timeout_ms=30000, init_timeout_ms=60000)
    assert eng.msm_sharded(0, n, 0) == plain
    eng.comm_destroy()
    eng.close()


def _multi_handle(lib, devices):
    import ctypes

    ids = (ctypes.c_int * len(devices))(*devices)
    h = ctypes.c_void_p()
    rc = lib.kzg_multi_create(len(devices), ids, ctypes.byref(h))
    assert rc == 0, lib.kzg_multi_last_error(None)
    return h


def _check_multi_rows_from_file(devices, tmp_path):
    """kzg_multi_load_srs_file on G contexts: every context holds ONLY the slices of the worker indices it serves, every
    worker's commit+open == oracle; a failed reload leaves the handle refusing (never routing into a half-replaced set),
    a good reload serves again."""
    import ctypes

    from zkp_subnet_amd import _native

    lib = _native.load()
    scale, ms = 11, 3                   # 8 worker slices of 2^8 points
    T, M, G = 1 << (scale - ms), 1 << ms, len(devices)
    tx, ty = 0x7A11E5, 0x5EED5
    slices = [oc.srs_gen(tx.to_bytes(32, "big"), ty.to_bytes(32, "big"), scale, ms, i) for i in range(M)]
    good = tmp_path / "setup_11_3.uncompressed"
    good.write_bytes(b"".join(slices))
    bad = tmp_path / "setup_bad.uncompressed"
    blob = bytearray(b"".join(slices))
    blob[96 * (5 * T + 3) + 95] ^= 1    # one point of worker 5's slice leaves the curve: only the device that serves 5 sees it
    bad.write_bytes(bytes(blob))
    h = _multi_handle(lib, devices)
    try:
        assert lib.kzg_multi_load_srs_file(h, os.fsencode(str(good)), 0, scale, ms) == 0, lib.kzg_multi_last_error(h)
        for g in range(G):
            want = len(range(g, M, G)) * T
            assert lib.kzg_srs_points(ctypes.c_void_p(lib.kzg_multi_ctx(h, g))) == want, (g, want)
        alpha = (0x1234567 % o.R).to_bytes(32, "big")

        def serve_all():
            for i in range(M):
                row = rand_scalars_bytes(T, 900 + i)
                c, e, p = ctypes.create_string_buffer(48), ctypes.create_string_buffer(32), ctypes.create_string_buffer(48)
                rc = lib.kzg_multi_commit_open(h, i, row, T, 1, alpha, c, e, p)
                assert rc == 0, (i, lib.kzg_multi_last_error(h))
                assert c.raw == oc.commit(slices[i], row, True), i
                assert (e.raw, p.raw) == oc.open_(slices[i], row, alpha, True), i

        serve_all()
        rc = lib.kzg_multi_load_srs_file(h, os.fsencode(str(bad)), 0, scale, ms)
        assert rc == _native.KZG_E_POINT, rc
        c = ctypes.create_string_buffer(48)
        rc = lib.kzg_multi_commit(h, 0, rand_scalars_bytes(T, 1), T, 1, c)
        assert rc == _native.KZG_E_ARG and b"no SRS resident" in lib.kzg_multi_last_error(h)      # refuses; never a wrong slice
        assert lib.kzg_multi_load_srs_file(h, os.fsencode(str(good)), 0, scale, ms) == 0
        serve_all()
    finally:
        lib.kzg_multi_destroy(h)


def test_multi_handle_loads_per_device_slices_from_the_setup_file_three_contexts_one_gpu(tmp_path):
    _check_multi_rows_from_file([0, 0, 0], tmp_path)


def _check_segmented_msm(devices, tmp_path, lg_big=None):
    """ONE MSM over the G contexts of one handle (kzg_multi_msm, SEGMENTS layout): bit-identical to the single-device MSM over
    the same points and to the oracle's trapdoor value [f(tau)] G; ranges that straddle segments; the resident form; segments
    read from a setup file; sizes that do not divide by G."""
    from zkp_subnet_amd import HipEngine, KzgError, SegmentedMsm
    from zkp_subnet_amd._native import KZG_E_ARG

    tau = 0xBEEFCAFE1357
    G = len(devices)
    seg = SegmentedMsm(devices)
    one = HipEngine(devices[0])
    try:
        for n in (3 << 10, 10000):
            seg.gen_srs(tau, n)
            assert sum(seg.segment(g)[1] for g in range(G)) == n and seg.segment(0)[0] == 0
            lg = (n - 1).bit_length()
            one.gen_srs(tau, 1, lg, 0)
            scal = rand_scalars_bytes(n, 5150 + n)
            want = oc.g1_mul_gen(oc.fr_eval(scal, tau.to_bytes(32, "big")))
            assert one.msm(scal, 0) == want
            assert seg.msm(scal, 0) == want, n
            # a range that starts inside segment 0 and ends inside the last one; one that lies inside a single segment
            for off, cnt in ((n // 7, n - n // 7 - 5), (seg.segment(G - 1)[0] + 3, 17), (0, 1), (n - 1, 1)):
                assert seg.msm(scal[:32 * cnt], off) == one.msm(scal[:32 * cnt], off), (n, off, cnt)
            seg.upload(1, scal, 0)
            assert seg.msm_resident(1) == want
            seg.upload(2, scal[:32 * 100], n // 2)
            assert seg.msm_resident(2) == one.msm(scal[:32 * 100], n // 2)
            assert seg.msm(b"", 0) == bytes([0xC0]) + bytes(47)                      # empty sum: infinity
            with pytest.raises(KzgError) as ei:
                seg.msm(scal, 1)                                                     # runs past the last point
            assert ei.value.code == KZG_E_ARG
        # segments read from a FILE: device g preads only its byte range
        n = 3 << 10
        path = tmp_path / "flat.srs"
        one.gen_srs(tau, 1, 12, 0)
        path.write_bytes(one.srs_read(0, n))
        seg.load_srs_file(str(path), n)
        scal = rand_scalars_bytes(n, 99)
        assert seg.msm(scal, 0) == oc.g1_mul_gen(oc.fr_eval(scal, tau.to_bytes(32, "big")))
        if lg_big:          # BASELINE sizes through the trapdoor identity
            n = 1 << lg_big
            seg.gen_srs(tau, n)
            scal = rand_scalars_bytes(n, 2600 + lg_big)
            seg.upload(0, scal, 0)
            assert seg.msm_resident(0) == oc.g1_mul_gen(oc.fr_eval(scal, tau.to_bytes(32, "big")))
    finally:
        one.close()
        seg.close()


def test_one_msm_over_three_contexts_of_one_handle_on_one_gpu(tmp_path):
    _check_segmented_msm([0, 0, 0], tmp_path, lg_big=20)


def test_cfg4_shape_one_msm_over_eight_contexts_of_one_handle_2_24():
    """BASELINE.json configs[3]'s shape from behind the one-client seam: ONE MSM whose SRS is cut into EIGHT segments, one per
    context of one handle (here 2^24 points, eight contexts on this box's one GPU; the device-count-gated test below runs the
    same over distinct GPUs).  Scalars resident per segment, eight partial MSMs concurrently, one sum of 8 x 192 bytes: the
    result is the oracle's trapdoor value [f(tau)] G."""
    from zkp_subnet_amd import SegmentedMsm

    tau, n = 0xC0DEC0DE77, 1 << 24
    seg = SegmentedMsm([0] * 8)
    try:
        seg.gen_srs(tau, n)
        assert [seg.segment(g) for g in range(8)] == [(g << 21, 1 << 21) for g in range(8)]
        scal = rand_scalars_bytes(n, 2424)
        seg.upload(0, scal, 0)
        want = oc.g1_mul_gen(oc.fr_eval(scal, tau.to_bytes(32, "big")))
        assert seg.msm_resident(0) == want
        assert seg.msm_resident(0) == want                    # and again: the resident form is repeatable
        half = scal[32 * (n // 4):32 * (3 * n // 4)]          # a range that covers segments 2 .. 5 exactly
        seg.upload(1, half, n // 4)
        lo = oc.fr_eval(half, tau.to_bytes(32, "big"))
        shift = pow(tau, n // 4, o.R)
        assert seg.msm_resident(1) == oc.g1_mul_gen((int.from_bytes(lo, "big") * shift % o.R).to_bytes(32, "big"))
    finally:
        seg.close()


def test_cfg4_full_size_2_26_points_in_eight_segments_of_one_handle():
    """BASELINE.json configs[3] at FULL size from behind the one-client seam: 2^26 points cut into eight SRS segments of 2^23,
    one per context of ONE handle (eight contexts on this box's one GPU: 103 GB of window tables, c = 22 per segment), the
    scalars resident per segment, eight partial MSMs, one sum of 8 x 192 bytes == the oracle's [f(tau)] G (no MSM on the CPU
    side: f(tau) is a Horner evaluation of the 2^26 scalars, segment by segment)."""
    from zkp_subnet_amd import SegmentedMsm

    tau, n, G = 0x2626BEEF2626, 1 << 26, 8
    seg_n = n // G
    seg = SegmentedMsm([0] * G)
    try:
        seg.gen_srs(tau, n)
        assert [seg.segment(g) for g in range(G)] == [(g * seg_n, seg_n) for g in range(G)]
        y, tau_seg, txs = 0, pow(tau, seg_n, o.R), tau.to_bytes(32, "big")
        for g in range(G):                                      # segment by segment: 256 MB of scalars at a time on the host
            s_b = rand_scalars_bytes(seg_n, 2680 + g)
            seg.upload(1, s_b, g * seg_n)                       # slot 1: the LAST upload's range is what msm_resident(1) covers
            y = (y + pow(tau_seg, g, o.R) * int.from_bytes(oc.fr_eval(s_b, txs), "big")) % o.R
            if g == G - 1:
                last = oc.g1_mul_gen((pow(tau_seg, g, o.R) * int.from_bytes(oc.fr_eval(s_b, txs), "big") % o.R).to_bytes(32, "big"))
                assert seg.msm_resident(1) == last              # one segment alone: only device 7 has work
            del s_b
        whole = b"".join(rand_scalars_bytes(seg_n, 2680 + g) for g in range(G))
        seg.upload(0, whole, 0)
        del whole
        assert seg.msm_resident(0) == oc.g1_mul_gen(y.to_bytes(32, "big"))
    finally:
        seg.close()


# ------------------------------------------------------------------ device-count-gated: REAL N > 1 ranks / devices
# None of these can run on the pool's 1-GPU boxes; they size themselves from the visible device count, skip cleanly at 1 and
# run unmodified on any multi-GPU box (VERDICT r5 task 1): the first N-rank ncclCommInitRank + ncclAllGather of this library
# then happens inside a TEST, not inside a driver record.
def _visible_gpus():
    import torch

    return torch.cuda.device_count()      # counts through the SMI library: does not initialise HIP in this process


def _need_gpus(k=2):
    n = _visible_gpus()
    if n < k:
        pytest.skip(f"needs >= {k} visible GPUs, this box has {n}")
    return min(n, 8)


def _run_ranks(world, started, tmp_path, tau, init_ms, logs, absent=False):
    import subprocess
    import sys

    d = tmp_path / f"rdv_{world}_{len(started)}"
    d.mkdir()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "comm_ranks.py"), str(r), str(world), str(d), hex(tau),
                               str(init_ms), ",".join(str(x) for x in logs)] + (["absent"] if absent else []),
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT) for r in started]
    recs = []
    for p in procs:
        so, se = p.communicate(timeout=1200)
        assert p.returncode == 0, se[-3000:]
        recs.append(_last_json(so))
    return recs


def test_real_ranks_library_collective_one_process_per_gpu(tmp_path):
    """(a) one process per visible GPU, NO torch: unique id through a file -> kzg_comm_init_bounded -> kzg_comm_selftest ->
    kzg_msm_sharded at 2^16 and 2^20 points per rank; every rank's bytes == the oracle's [f(tau)] G over the whole SRS."""
    N = _need_gpus()
    tau = 0x5CA1AB1E0DD
    logs = [16, 20]
    recs = _run_ranks(N, list(range(N)), tmp_path, tau, 120000, logs)
    for lg in logs:
        whole = b"".join(np.random.default_rng(1000 * lg + r).integers(0, 256, size=(1 << lg, 32), dtype=np.uint8).tobytes()
                         for r in range(N))
        arr = np.frombuffer(whole, dtype=np.uint8).reshape(-1, 32).copy()
        arr[:, 0] &= 0x3F
        want = oc.g1_mul_gen(oc.fr_eval(arr.tobytes(), tau.to_bytes(32, "big"))).hex()
        for r in recs:
            assert r["init"] == "ok" and r["info"]["world"] == N and r["info"]["rccl_version_code"] > 20000, r
            assert r[f"msm_{lg}"] == want, (lg, r["rank"])


def test_real_ranks_an_absent_rank_costs_the_others_one_timeout(tmp_path):
    """(a') world = N but the last rank never starts: every rank that did start gets KZG_E_COMM inside the budget and its
    engine still serves."""
    N = _need_gpus()
    tau = 0xDEAD0BEEF
    recs = _run_ranks(N, list(range(N - 1)), tmp_path, tau, 5000, [12], absent=True)
    for r in recs:
        assert r["init"] == "E_COMM" and r["init_s"] < 30, r
        raw = np.random.default_rng(1000 * 12 + r["rank"]).integers(0, 256, size=(1 << 12, 32), dtype=np.uint8)
        raw[:, 0] &= 0x3F
        assert r["plain_after"] == oc.g1_mul_gen(oc.fr_eval(raw.tobytes(), tau.to_bytes(32, "big"))).hex(), r


def test_real_devices_one_handle_rows_and_one_msm_over_distinct_gpus(tmp_path):
    """(b) kzg_multi_* / MultiDeviceClient / SegmentedMsm over DISTINCT devices: per-device slices from a setup file, every
    Pianist row == oracle, one 2^22-point MSM cut into N segments == [f(tau)] G."""
    N = _need_gpus()
    devices = list(range(N))
    _check_multi_rows_from_file(devices, tmp_path)
    _check_segmented_msm(devices, tmp_path, lg_big=22)
    from zkp_subnet_amd import MultiDeviceClient, codec

    scale, ms, seed = 13, 3, 424242
    mc = MultiDeviceClient(devices, seed=seed)
    mc.start(scale, ms)
    try:
        from zkp_subnet_amd.client import derive_taus

        tx, ty = derive_taus(seed)
        T = 1 << (scale - ms)
        alpha = codec.be32_to_fr((0xA1FA % o.R).to_bytes(32, "big"))
        idx = list(range(1 << ms))
        rows = [rand_scalars_bytes(T, 70 + i) for i in idx]
        resp = mc.commit_and_open_rows(idx, [codec.be32_to_fr_list(r) for r in rows], alpha)
        for i, r in zip(idx, resp):
            assert r.status_code == 200, r.json()
            srs = oc.srs_gen(tx.to_bytes(32, "big"), ty.to_bytes(32, "big"), scale, ms, i)
            assert codec.g1_from_b64(r.json()["commitment"]) == oc.commit(srs, rows[i], True), i
            ev, pf = oc.open_(srs, rows[i], codec.fr_to_be32(alpha), True)
            assert codec.fr_to_be32(r.json()["eval"]) == ev and codec.g1_from_b64(r.json()["proof"]) == pf, i
    finally:
        mc.stop()


def test_real_ranks_bench_contract_with_every_visible_gpu():
    """(c) `python bench.py --gpus <visible>` as the driver launches a SCALE point: the line must come from the library's RCCL
    collective (no gloo fallback), name the RCCL version, and carry both other multi-GPU configurations."""
    import subprocess
    import sys

    N = _need_gpus()
    N = 1 << (N.bit_length() - 1)           # msm26 needs a power-of-two number of ranks
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", str(N), "--steps", "3", "--warmup", "1"],
                         capture_output=True, text=True, timeout=3000, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    line = _last_json(out.stdout)
    assert line["n_gpus"] == N and line["config"]["world_size"] == N, line["config"]
    assert not line["config"]["collective"].startswith("gloo fallback"), line["config"]["collective"]
    assert line["config"]["collective"].startswith("library"), line["config"]["collective"]
    assert line["config"].get("rccl_version") and not str(line["config"]["rccl_version"]).startswith("none"), line["config"]
    assert "error" not in line["msm26"] and "error" not in line["pianist_kzg22"], (line["msm26"], line["pianist_kzg22"])
