"""The definitions of the product scan (csrc/fr_prod.hip), of the batched inversion behind it and of the additive scan
(csrc/fr_lookup.hip) in Python integers mod r, by the forms of kzg_test_scan_run, and the level plan both scans share as
include/kzg_mi355x_scan_test.h states it.  No project code is involved.  Every denominator must be invertible: what the kernels
leave when one is 0 is unspecified apart from the flag.  `inv` is the modular inverse; a caller with many vectors over the same
values may pass a memoised one."""
from tests.gpu_common import R


def inverse(x):
    return pow(x, -1, R)


def product(a, b, start=1, inv=inverse):
    """forms 0 and 1: ([start prod_{u<t} a[u] / b[u] for t < n], the closing value start prod_u a[u] / b[u])"""
    out, p = [], start % R
    for x, y in zip(a, b):
        out.append(p)
        p = p * x % R * inv(y) % R
    return out, p


def inverses(a, b=None, inv=inverse):
    """forms 2 (b None: 1 / a[t]) and 3 (b[t] / a[t]); the closing slot holds prod a / prod a = 1"""
    return [(1 if b is None else b[t]) * inv(x) % R for t, x in enumerate(a)], 1


def sums(a):
    """form 4: ([sum_{u<t} a[u] for t < n], the total)"""
    out, s = [], 0
    for x in a:
        out.append(s)
        s = (s + x) % R
    return out, s


def run(form, a, b=None, start=None, inv=inverse):
    """(out, closing) of form 0 .. 4"""
    if form in (0, 1):
        return product(a, b, 1 if form == 0 else start, inv)
    if form in (2, 3):
        return inverses(a, None if form == 2 else b, inv)
    assert form == 4
    return sums(a)


def plan(n, l0=None, top_max=2048):
    """the level plan as the header states it: {"K", "l", "n", "off"}; l0 = None: 2 below 2^17, 3 below 2^18, else 4.  Level 0 is
    always folded once (K >= 1); levels of 16 follow while more than top_max values are left"""
    if l0 is None:
        l0 = 2 if n < 1 << 17 else 3 if n < 1 << 18 else 4
    ls, ns, offs = [], [n], [0]
    while len(ns) == 1 or ns[-1] > top_max:
        l = l0 if len(ns) == 1 else 4
        ls.append(l)
        offs.append(offs[-1] + ns[-1] if len(ns) > 1 else 0)
        ns.append((ns[-1] + (1 << l) - 1) >> l)
    return {"K": len(ls), "l": ls + [0], "n": ns, "off": offs}
