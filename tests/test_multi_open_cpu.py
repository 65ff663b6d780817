"""CPU-only tests of the multi-point opening's verifier (kzg_vk_verify_open_multi, csrc/pairing_host.cpp): openings built
entirely with the C oracle -- commit for every C_j, fr_eval / open_ for every y_{j,p}, open_ on h_p = sum_t gamma_p^t f_{j_t}
for every pi_p -- over slices from oracle.cpu.srs_gen are accepted, every tampering is rejected (valid = 0, never an error),
through the Verifier and through the Client, and every argument limit is KZG_E_ARG at the C-ABI."""
import ctypes
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
    """h = sum_t gamma^t f_t element by element (either form: the INTT is linear)."""
    T = len(rows[0]) // 32
    out = []
    for t in range(T):
        acc = 0
        for j in reversed(range(len(rows))):
            acc = (acc * gamma + int.from_bytes(rows[j][32 * t:32 * t + 32], "big")) % R
        out.append(be(acc))
    return b"".join(out)


def multi_open(srs, rows, points, opened, gammas, ef=True):
    comms = [oc.commit(srs, r, ef) for r in rows]
    evals = [[oc.open_(srs, rows[j], be(a), ef)[0] for j in js] for a, js in zip(points, opened)]
    proofs = [oc.open_(srs, combine([rows[j] for j in js], g), be(a), ef)[1] for a, js, g in zip(points, opened, gammas)]
    return comms, evals, proofs


@pytest.fixture(scope="module")
def setup():
    build()
    oc.build()
    rnd = random.Random(78)
    tx, ty = rnd.randrange(1, R), rnd.randrange(1, R)
    scale, ms = 6, 2
    vk = Verifier.synthetic(tx, [lagrange_factor(i, ms, ty) for i in range(1 << ms)])
    srs = {i: oc.srs_gen(be(tx), be(ty), scale, ms, i) for i in range(1 << ms)}
    yield rnd, vk, srs, 1 << (scale - ms)
    vk.close()


def rows_for(rnd, k, T):
    return [b"".join(be(rnd.randrange(R)) for _ in range(T)) for _ in range(k)]


def args(points, gammas):
    return [be(a) for a in points], [be(g) for g in gammas]


@pytest.mark.parametrize("i,k,opened,ef", [
    (0, 1, [[0]], True),
    (1, 3, [[0, 1, 2], [1]], True),                      # PLONK shape: everything at zeta, one row at zeta * omega
    (3, 4, [[0, 2], [1, 3], [0, 1, 2, 3]], False),
    (2, 5, [[0, 1, 2, 3, 4]] * 4, True),                 # m = 4, full masks, equal row sets
    (0, 16, [list(range(16)), [3, 15]], True),
])
def test_oracle_multi_openings_verify(setup, i, k, opened, ef):
    rnd, vk, srs, T = setup
    rows = rows_for(rnd, k, T)
    m = len(opened)
    points, gammas = [rnd.randrange(R) for _ in range(m)], [rnd.randrange(R) for _ in range(m)]
    comms, evals, proofs = multi_open(srs[i], rows, points, opened, gammas, ef)
    P, G = args(points, gammas)
    assert vk.verify_open_multi(i, comms, P, opened, G, evals, proofs)


def test_equal_points_keep_their_own_proofs(setup):
    rnd, vk, srs, T = setup
    i, k = 1, 3
    rows = rows_for(rnd, k, T)
    a = rnd.randrange(R)
    points, opened, gammas = [a, a], [[0, 1], [2]], [rnd.randrange(R), rnd.randrange(R)]
    comms, evals, proofs = multi_open(srs[i], rows, points, opened, gammas)
    P, G = args(points, gammas)
    assert vk.verify_open_multi(i, comms, P, opened, G, evals, proofs)


def test_m1_full_mask_agrees_with_verify_open_batch(setup):
    rnd, vk, srs, T = setup
    i, k = 2, 4
    rows = rows_for(rnd, k, T)
    a, g = rnd.randrange(R), rnd.randrange(R)
    comms, evals, proofs = multi_open(srs[i], rows, [a], [list(range(k))], [g])
    assert vk.verify_open_multi(i, comms, [be(a)], [list(range(k))], [be(g)], evals, proofs)
    assert vk.verify_open_batch(i, comms, evals[0], be(a), be(g), proofs[0])
    bad = list(evals[0])
    bad[1] = be(int.from_bytes(bad[1], "big") + 1)
    assert not vk.verify_open_multi(i, comms, [be(a)], [list(range(k))], [be(g)], [bad], proofs)
    assert not vk.verify_open_batch(i, comms, bad, be(a), be(g), proofs[0])


def test_tampered_multi_openings_are_rejected(setup):
    rnd, vk, srs, T = setup
    i, k = 3, 4
    rows = rows_for(rnd, k, T)
    opened = [[0, 1, 2, 3], [1, 2], [3]]
    points, gammas = [rnd.randrange(R) for _ in range(3)], [rnd.randrange(R) for _ in range(3)]
    comms, evals, proofs = multi_open(srs[i], rows, points, opened, gammas)
    P, G = args(points, gammas)
    assert vk.verify_open_multi(i, comms, P, opened, G, evals, proofs)

    def rejected(c=comms, p=P, op=opened, g=G, e=evals, pf=proofs, idx=i):
        return not vk.verify_open_multi(idx, c, p, op, g, e, pf)

    c2 = list(comms)
    c2[2] = comms[1]
    assert rejected(c=c2)                                                   # one commitment
    e2 = [list(ev) for ev in evals]
    e2[1][0] = be(int.from_bytes(e2[1][0], "big") + 1)
    assert rejected(e=e2)                                                   # one evaluation at one point
    pf2 = list(proofs)
    pf2[2] = oc.open_(srs[i], rows[3], be(points[2] + 1))[1]
    assert rejected(pf=pf2)                                                 # one proof
    assert rejected(pf=[proofs[1], proofs[0], proofs[2]])                   # two proofs swapped
    assert rejected(p=[P[1], P[0], P[2]])                                   # two points swapped
    assert rejected(g=[G[0], be(gammas[1] + 1), G[2]])                      # one gamma
    assert rejected(op=[[0, 1, 2, 3], [1, 3], [3]])                         # a mask changed
    assert rejected(idx=0)                                                  # another worker's basis
    # malformed bytes: valid = 0, not an error
    assert rejected(pf=[proofs[0], b"\x00" * 48, proofs[2]])
    assert rejected(c=[b"\xff" * 48] + comms[1:])
    assert rejected(pf=[proofs[0], proofs[1], proofs[2][:47]])
    # argument errors are errors
    for bad in (lambda: vk.verify_open_multi(i, comms, [P[0], R.to_bytes(32, "big"), P[2]], opened, G, evals, proofs),
                lambda: vk.verify_open_multi(i, comms, P, opened, [G[0], G[1], R.to_bytes(32, "big")], evals, proofs),
                lambda: vk.verify_open_multi(9, comms, P, opened, G, evals, proofs),
                lambda: vk.verify_open_multi(i, comms, P, [[0, 1, 2, 3], [2, 1], [3]], G, evals, proofs),
                lambda: vk.verify_open_multi(i, comms, P, [[0, 1, 2, 3], [1, 4], [3]], G, evals, proofs)):
        with pytest.raises(_native.KzgError):
            bad()
    with pytest.raises(ValueError):
        vk.verify_open_multi(i, comms, P, opened, G, [evals[0], evals[1][:1], evals[2]], proofs)


def test_c_abi_argument_limits(setup):
    rnd, vk, srs, T = setup
    lib = _native.load()
    ok = ctypes.c_int(7)
    z48, z32 = bytes(48 * 17), bytes(32 * 80)

    def call(k, m, masks, i=0):
        arr = (ctypes.c_uint32 * max(len(masks), 1))(*masks)
        return lib.kzg_vk_verify_open_multi(vk._h, i, k, z48, m, z32, arr, z32, z32, z48, ctypes.byref(ok))

    assert call(0, 1, [1]) == _native.KZG_E_ARG                         # k = 0
    assert call(17, 1, [1]) == _native.KZG_E_ARG                        # k > 16
    assert call(2, 0, [1]) == _native.KZG_E_ARG                         # m = 0
    assert call(2, 5, [1] * 5) == _native.KZG_E_ARG                     # m > 4
    assert call(2, 2, [1, 0]) == _native.KZG_E_ARG                      # a zero mask
    assert call(2, 2, [1, 4]) == _native.KZG_E_ARG                      # a mask bit >= k
    assert call(2, 1, [3], i=4) == _native.KZG_E_ARG                    # worker outside the key
    assert ok.value == 0
    assert lib.kzg_vk_verify_open_multi(None, 0, 1, z48, 1, z32, (ctypes.c_uint32 * 1)(1), z32, z32, z48,
                                        ctypes.byref(ok)) == _native.KZG_E_ARG
    # the well-formed call on all-zero bytes: not a point, so valid = 0 and no error
    assert call(2, 1, [3]) == _native.KZG_OK and ok.value == 0


class _VerifyOnly:
    def __init__(self, vk):
        self.verify_open_multi = vk.verify_open_multi


def test_client_verdicts_match(setup):
    rnd, vk, srs, T = setup
    i, k = 1, 3
    rows = rows_for(rnd, k, T)
    opened = [[0, 1, 2], [2]]
    points, gammas = [rnd.randrange(R) for _ in range(2)], [rnd.randrange(R) for _ in range(2)]
    comms, evals, proofs = multi_open(srs[i], rows, points, opened, gammas)
    cl = Client(engine=_VerifyOnly(vk))
    cl.machines_scale, cl._slice_of = 2, None   # what start() leaves for a synthetic setup
    C = [g1_to_b64(c) for c in comms]
    E = [[be32_to_fr(e) for e in ev] for ev in evals]
    Pf = [g1_to_b64(p) for p in proofs]
    X = [be32_to_fr(be(v)) for v in points]
    G = [be32_to_fr(be(v)) for v in gammas]
    r = cl.worker_verify_open_multi(i, Pf, X, opened, G, E, C)
    assert r.status_code == 200 and r.json() == {"valid": True}
    E2 = [list(e) for e in E]
    E2[1][0] = be32_to_fr(be(int.from_bytes(evals[1][0], "big") + 1))
    assert cl.worker_verify_open_multi(i, Pf, X, opened, G, E2, C).json() == {"valid": False}
    assert cl.worker_verify_open_multi(i, Pf, X[::-1], opened, G, E, C).json() == {"valid": False}
    assert cl.worker_verify_open_multi(i, Pf, X, opened, [be32_to_fr(be(gammas[0] + 1)), G[1]], E, C).json() \
        == {"valid": False}
    # point 1 opens one row: its gamma multiplies nothing, any value verifies
    assert cl.worker_verify_open_multi(i, Pf, X, opened, [G[0], be32_to_fr(be(gammas[1] + 1))], E, C).json() \
        == {"valid": True}
    assert cl.worker_verify_open_multi(i, Pf[::-1], X, opened, G, E, C).json() == {"valid": False}
    assert cl.worker_verify_open_multi(i, Pf, X, opened, G, [E[0], E[1] + E[1]], C).status_code == 400
    assert cl.worker_verify_open_multi(i, Pf, X, [[0, 1, 2], [3]], G, E, C).status_code == 400   # row outside k
    r = cl.worker_verify_open_multi(i, [Pf[0], g1_to_b64(b"\x00" * 48)], X, opened, G, E, C)   # not a point
    assert r.status_code == 200 and r.json() == {"valid": False}
