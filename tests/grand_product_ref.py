"""The permutation grand product of kzg_rows_commit_grand_product from its definition, in Python integers -- the reference
of tests/test_grand_product_cpu.py (which pins it) and tests/test_gpu_grand_product.py (which compares the GPU with it) --
and a builder of real permutation instances (sigma rows of a random permutation of the k x T cells, wires constant on its
cycles)."""
import random

from tests.gpu_common import R, be, ints, row_bytes  # noqa: F401  (re-exported for the tests)


def omega(T):
    """the library's T-th root of unity: 7^((r-1)/T)"""
    assert T & (T - 1) == 0 and (R - 1) % T == 0
    return pow(7, (R - 1) // T, R)


def domain(T):
    w, out, x = omega(T), [], 1
    for _ in range(T):
        out.append(x)
        x = x * w % R
    return out


def batch_inverse(vals):
    """[1 / v] with one modular inversion; ZeroDivisionError when some v == 0"""
    pre, acc = [], 1
    for v in vals:
        pre.append(acc)
        acc = acc * v % R
    if acc == 0:
        raise ZeroDivisionError("zero denominator")
    inv, out = pow(acc, -1, R), [0] * len(vals)
    for t in range(len(vals) - 1, -1, -1):
        out[t] = inv * pre[t] % R
        inv = inv * vals[t] % R
    return out


def factors(wires, sigmas, shifts, beta, gamma):
    """(N_t, D_t) from the evaluations a_j(w^t), sigma_j(w^t) (lists of k lists of T integers)"""
    T = len(wires[0])
    dom = domain(T)
    N, D = [1] * T, [1] * T
    for a, sg, s in zip(wires, sigmas, shifts):
        for t in range(T):
            N[t] = N[t] * (a[t] + beta * s % R * dom[t] + gamma) % R
            D[t] = D[t] * (a[t] + beta * sg[t] + gamma) % R
    return N, D


def grand_product(wires, sigmas, shifts, beta, gamma):
    """z(w^t) for t in [0, T) and the closing value: z_0 = 1, z_{t+1} = z_t N_t / D_t, closing = prod N / prod D.
    ZeroDivisionError when some D_t == 0."""
    N, D = factors(wires, sigmas, shifts, beta, gamma)
    Dinv = batch_inverse(D)
    z, acc = [], 1
    for n, di in zip(N, Dinv):
        z.append(acc)
        acc = acc * n % R * di % R
    return z, acc


def permutation_instance(k, T, seed, shifts=None):
    """(wires, sigmas, shifts) as evaluation lists: a random permutation of the k*T cells, sigma_j(w^t) = the identity value
    s_j' w^t' of the cell that (j, t) maps to, wire values constant on the permutation's cycles.  shifts default to 1 and
    k - 1 non-residue cosets 7^j (7 generates the multiplicative group, so 7^j H are distinct cosets for j < (r-1)/T)."""
    rnd = random.Random(seed)
    shifts = shifts or [pow(7, j, R) for j in range(k)]
    dom = domain(T)
    cells = [(j, t) for j in range(k) for t in range(T)]
    image = cells[:]
    rnd.shuffle(image)
    perm = dict(zip(cells, image))
    wires = [[None] * T for _ in range(k)]
    for c in cells:
        if wires[c[0]][c[1]] is None:
            v, x = rnd.randrange(R), c
            while wires[x[0]][x[1]] is None:
                wires[x[0]][x[1]] = v
                x = perm[x]
    sigmas = [[shifts[perm[(j, t)][0]] * dom[perm[(j, t)][1]] % R for t in range(T)] for j in range(k)]
    return wires, sigmas, shifts
