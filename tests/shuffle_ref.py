"""The shuffle running product of kzg_rows_commit_shuffle from its definition, in Python integers -- the reference of
tests/test_shuffle_cpu.py (which pins it) and tests/test_gpu_shuffle.py (which compares the GPU with it) -- and a builder of
true shuffle instances (each group's shuffle tuples a seeded permutation of its input tuples over the enabled usable rows,
random garbage in the disabled and padding cells) with a one-cell broken variant."""
import random

from tests.gpu_common import R
from tests.grand_product_ref import batch_inverse, domain, omega  # noqa: F401  (re-exported for the tests)


def factors(inputs, shuffles, G, w, theta, gamma, input_sel=None, shuffle_sel=None):
    """(N_t, D_t) from the evaluations a_{g,c}(w^t), b_{g,c}(w^t) (lists of G * w lists of T integers, group-major).
    input_sel / shuffle_sel: None, or per group None or that side's selector row (T integers, any element of Fr)"""
    assert len(inputs) == len(shuffles) == G * w
    T = len(inputs[0])
    out = []
    for rows, sel in ((inputs, input_sel), (shuffles, shuffle_sel)):
        V = [1] * T
        for g in range(G):
            q = sel[g] if sel is not None else None
            for t in range(T):
                f = (gamma + sum(pow(theta, c, R) * rows[g * w + c][t] for c in range(w))) % R
                if q is not None:
                    f = (1 + q[t] * (f - 1)) % R
                V[t] = V[t] * f % R
        out.append(V)
    return out[0], out[1]


def shuffle_product(inputs, shuffles, G, w, theta, gamma, input_sel=None, shuffle_sel=None, usable=None, tail=()):
    """z(w^t) for t in [0, T) and the closing value: z_0 = 1, z_{t+1} = z_t N_t / D_t, closing = prod N / prod D.  usable = u:
    N_t = D_t = 1 on the rows t >= u, z_u = closing, z_t = tail[t - u - 1] behind it.  ZeroDivisionError when a D_t that counts
    is zero."""
    N, D = factors(inputs, shuffles, G, w, theta, gamma, input_sel, shuffle_sel)
    T = len(N)
    if usable is not None:
        assert 1 <= usable <= T - 1 and len(tail) == T - usable - 1
        N[usable:], D[usable:] = [1] * (T - usable), [1] * (T - usable)
    Dinv = batch_inverse(D)
    z, acc = [], 1
    for n, di in zip(N, Dinv):
        z.append(acc)
        acc = acc * n % R * di % R
    if usable is not None:
        z[usable + 1:] = list(tail)
    return z, acc


def shuffle_instance(G, w, T, seed, usable=None, sel=False):
    """(inputs, shuffles, input_sel, shuffle_sel) as evaluation lists, a TRUE instance: per group the shuffle tuples on the
    enabled usable rows are a seeded permutation of the input tuples on the enabled usable rows.  sel: each side of each group
    gets a 0/1 selector row of its own (the same number of enabled rows on both sides, at different places); otherwise the
    selector lists are None.  Every cell that does not count -- disabled, or at a row >= usable -- holds random garbage, and so
    do the selectors behind `usable`."""
    rnd = random.Random(seed)
    u = T if usable is None else usable
    inputs = [[rnd.randrange(R) for _ in range(T)] for _ in range(G * w)]
    shuffles = [[rnd.randrange(R) for _ in range(T)] for _ in range(G * w)]
    input_sel, shuffle_sel = ([], []) if sel else (None, None)
    for g in range(G):
        n_on = rnd.randrange(1, u + 1) if sel else u
        on_in, on_sh = (sorted(rnd.sample(range(u), n_on)) for _ in range(2))
        if sel:
            for on, lst in ((on_in, input_sel), (on_sh, shuffle_sel)):
                lst.append([int(t in on) if t < u else rnd.randrange(R) for t in range(T)])
        src = on_in[:]
        rnd.shuffle(src)
        for dst_t, src_t in zip(on_sh, src):
            for c in range(w):
                shuffles[g * w + c][dst_t] = inputs[g * w + c][src_t]
    return inputs, shuffles, input_sel, shuffle_sel


def broken(inputs, shuffles, input_sel, shuffle_sel, seed):
    """the instance with ONE cell of the shuffle side that counts (row 0 of an enabled row of group 0's first column) changed"""
    rnd = random.Random(seed)
    q = shuffle_sel[0] if shuffle_sel is not None else None
    t = next(t for t in range(len(shuffles[0])) if q is None or q[t] == 1)
    out = [r[:] for r in shuffles]
    out[0][t] = (out[0][t] + 1 + rnd.randrange(R - 1)) % R
    return inputs, out, input_sel, shuffle_sel
