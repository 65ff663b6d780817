"""CPU-only tests of the batched opening's verifier (kzg_vk_verify_open_batch, csrc/pairing_host.cpp): proofs built entirely
with the C oracle -- commit for every C_j, open_ on h = sum_j gamma^j f_j -- over slices from oracle.cpu.srs_gen are
accepted, and every tampering is rejected (valid = 0, never an error), through the Verifier and through the Client."""
import random

import pytest

from oracle import bls12_381 as o
from oracle import cpu as oc
from tests.gpu_common import be
from zkp_subnet_amd import _native
from zkp_subnet_amd.build import build
from zkp_subnet_amd.client import Client
from zkp_subnet_amd.codec import be32_to_fr, g1_to_b64
from zkp_subnet_amd.engine import lagrange_factor
from zkp_subnet_amd.verifier import Verifier

R = o.R


def combine(rows, gamma):
    """h = sum_j gamma^j f_j element by element (either form: the INTT is linear)."""
    T = len(rows[0]) // 32
    out = []
    for t in range(T):
        acc = 0
        for j in reversed(range(len(rows))):
            acc = (acc * gamma + int.from_bytes(rows[j][32 * t:32 * t + 32], "big")) % R
        out.append(be(acc))
    return b"".join(out)


def batch_open(srs, rows, alpha, gamma, ef=True):
    comms = [oc.commit(srs, r, ef) for r in rows]
    evals = [oc.open_(srs, r, be(alpha), ef)[0] for r in rows]
    _, pi = oc.open_(srs, combine(rows, gamma), be(alpha), ef)
    return comms, evals, pi


@pytest.fixture(scope="module")
def setup():
    build()
    oc.build()
    rnd = random.Random(77)
    tx, ty = rnd.randrange(1, R), rnd.randrange(1, R)
    scale, ms = 6, 2
    vk = Verifier.synthetic(tx, [lagrange_factor(i, ms, ty) for i in range(1 << ms)])
    srs = {i: oc.srs_gen(be(tx), be(ty), scale, ms, i) for i in range(1 << ms)}
    yield rnd, vk, srs, 1 << (scale - ms)
    vk.close()


def rows_for(rnd, k, T):
    return [b"".join(be(rnd.randrange(R)) for _ in range(T)) for _ in range(k)]


@pytest.mark.parametrize("i,k,ef", [(0, 1, True), (1, 3, True), (3, 4, False), (2, 16, True)])
def test_oracle_batched_openings_verify(setup, i, k, ef):
    rnd, vk, srs, T = setup
    rows = rows_for(rnd, k, T)
    alpha, gamma = rnd.randrange(R), rnd.randrange(R)
    comms, evals, pi = batch_open(srs[i], rows, alpha, gamma, ef)
    assert vk.verify_open_batch(i, comms, evals, be(alpha), be(gamma), pi)
    if k == 1:   # one row: the ordinary single-row check agrees
        assert vk.verify(i, pi, be(alpha), evals[0], comms[0])


def test_tampered_batched_openings_are_rejected(setup):
    rnd, vk, srs, T = setup
    i, k = 1, 4
    rows = rows_for(rnd, k, T)
    alpha, gamma = rnd.randrange(R), rnd.randrange(R)
    comms, evals, pi = batch_open(srs[i], rows, alpha, gamma)
    a, g = be(alpha), be(gamma)
    assert vk.verify_open_batch(i, comms, evals, a, g, pi)
    bumped = list(evals)
    bumped[2] = be(int.from_bytes(evals[2], "big") + 1)
    assert not vk.verify_open_batch(i, comms, bumped, a, g, pi)
    swapped = list(comms)
    swapped[0], swapped[3] = swapped[3], swapped[0]
    assert not vk.verify_open_batch(i, swapped, evals, a, g, pi)
    assert not vk.verify_open_batch(i, comms, evals, a, be(gamma + 1), pi)           # wrong gamma
    assert not vk.verify_open_batch(i, comms, evals, be(alpha + 1), g, pi)           # wrong alpha
    other = rnd.randrange(R)
    _, _, pi_other = batch_open(srs[i], rows, alpha, other)                          # a proof made under another gamma
    assert not vk.verify_open_batch(i, comms, evals, a, g, pi_other)
    assert vk.verify_open_batch(i, comms, evals, a, be(other), pi_other)
    assert not vk.verify_open_batch(2, comms, evals, a, g, pi)                       # another worker's basis
    # malformed bytes: valid = 0, not an error
    assert not vk.verify_open_batch(i, comms, evals, a, g, b"\x00" * 48)
    assert not vk.verify_open_batch(i, [b"\xff" * 48] + comms[1:], evals, a, g, pi)
    assert not vk.verify_open_batch(i, comms, evals, a, g, pi[:47])
    # argument errors are errors
    for bad in (lambda: vk.verify_open_batch(i, comms, evals, R.to_bytes(32, "big"), g, pi),
                lambda: vk.verify_open_batch(i, comms, evals, a, R.to_bytes(32, "big"), pi),
                lambda: vk.verify_open_batch(9, comms, evals, a, g, pi)):
        with pytest.raises(_native.KzgError):
            bad()
    with pytest.raises(ValueError):
        vk.verify_open_batch(i, comms, evals[:3], a, g, pi)


def test_c_abi_k_limits(setup):
    import ctypes

    rnd, vk, srs, T = setup
    lib = _native.load()
    ok = ctypes.c_int(7)
    z = bytes(48 * 17)
    assert lib.kzg_vk_verify_open_batch(vk._h, 0, 0, z, bytes(32 * 17), bytes(32), bytes(32), z[:48], ctypes.byref(ok)) \
        == _native.KZG_E_ARG
    assert lib.kzg_vk_verify_open_batch(vk._h, 0, 17, z, bytes(32 * 17), bytes(32), bytes(32), z[:48], ctypes.byref(ok)) \
        == _native.KZG_E_ARG and ok.value == 0


class _VerifyOnly:
    def __init__(self, vk):
        self.verify_open_batch = vk.verify_open_batch


def test_client_verdicts_match(setup):
    rnd, vk, srs, T = setup
    i, k = 3, 3
    rows = rows_for(rnd, k, T)
    alpha, gamma = rnd.randrange(R), rnd.randrange(R)
    comms, evals, pi = batch_open(srs[i], rows, alpha, gamma)
    cl = Client(engine=_VerifyOnly(vk))
    cl.machines_scale, cl._slice_of = 2, None   # what start() leaves for a synthetic setup
    C = [g1_to_b64(c) for c in comms]
    E = [be32_to_fr(e) for e in evals]
    A, G, A1, G1 = (be32_to_fr(be(v)) for v in (alpha, gamma, alpha + 1, gamma + 1))   # Fr on the wire: base64 of 32 B
    r = cl.worker_verify_open_batch(i, g1_to_b64(pi), A, G, E, C)
    assert r.status_code == 200 and r.json() == {"valid": True}
    E2 = list(E)
    E2[1] = be32_to_fr(be(int.from_bytes(evals[1], "big") + 1))
    assert cl.worker_verify_open_batch(i, g1_to_b64(pi), A, G, E2, C).json() == {"valid": False}
    assert cl.worker_verify_open_batch(i, g1_to_b64(pi), A, G1, E, C).json() == {"valid": False}
    assert cl.worker_verify_open_batch(i, g1_to_b64(pi), A1, G, E, C).json() == {"valid": False}
    assert cl.worker_verify_open_batch(i, g1_to_b64(pi), A, G, E, C[::-1]).json() == {"valid": False}
    assert cl.worker_verify_open_batch(i, g1_to_b64(pi), A, G, E[:2], C).status_code == 400
    r = cl.worker_verify_open_batch(i, g1_to_b64(b"\x00" * 48), A, G, E, C)   # not a point
    assert r.status_code == 200 and r.json() == {"valid": False}
