"""The definition of kzg_rows_commit_sigma and kzg_rows_check_copies in Python integers: sort (label, flat index), link every
class cyclically in ascending flat index, let free cells and the rows behind `usable` map to themselves, and write
sigma_c(w^t) = shift[c'] w^t' of the image.  Columns are lists of canonical integers (evaluations at w_T^t)."""
from oracle.bls12_381 import R
from tests import grand_product_ref as gp


def images(labels, usable=None, free_label=None):
    """(image: flat index c * T + t -> flat index, classes, fixed).  labels: k columns of T canonical integers.  usable = None: all
    T rows take part; otherwise rows [0, usable) do and the rows behind map to themselves, their labels unread.  classes: the
    distinct non-free labels among the participating cells; fixed: the participating cells that map to themselves"""
    k, T = len(labels), len(labels[0])
    n = T if usable is None else usable
    assert 1 <= n <= T and all(len(col) == T for col in labels)
    img = list(range(k * T))
    cells = sorted((labels[c][t], c * T + t) for c in range(k) for t in range(n) if labels[c][t] != free_label)
    classes, p = 0, 0
    while p < len(cells):
        q = p
        while q + 1 < len(cells) and cells[q + 1][0] == cells[p][0]:
            q += 1
        for a in range(p, q + 1):
            img[cells[a][1]] = cells[a + 1][1] if a < q else cells[p][1]
        classes += 1
        p = q + 1
    fixed = sum(1 for c in range(k) for t in range(n) if img[c * T + t] == c * T + t)
    return img, classes, fixed


def sigma_columns(labels, shifts, usable=None, free_label=None):
    """(the k sigma columns as evaluations, {"classes", "fixed"})"""
    k, T = len(labels), len(labels[0])
    assert len(shifts) == k
    img, classes, fixed = images(labels, usable, free_label)
    dom = gp.domain(T)
    out = [[shifts[img[c * T + t] // T] * dom[img[c * T + t] % T] % R for t in range(T)] for c in range(k)]
    return out, {"classes": classes, "fixed": fixed}


def copy_violations(wires, labels, usable=None, free_label=None):
    """{"violations", "first": (column, row) | None}: the participating, non-free cells whose value differs from that of their
    class's smallest-flat-index cell"""
    k, T = len(labels), len(labels[0])
    n = T if usable is None else usable
    assert len(wires) == k and 1 <= n <= T
    head, bad = {}, []
    for c in range(k):
        for t in range(n):
            lab = labels[c][t]
            if lab == free_label:
                continue
            h = head.setdefault(lab, (c, t))
            if wires[c][t] != wires[h[0]][h[1]]:
                bad.append((c, t))
    return {"violations": len(bad), "first": bad[0] if bad else None}


def cycles(img):
    """the cycles of the permutation `img` as sorted tuples, sorted"""
    seen, out = set(), []
    for j in range(len(img)):
        if j in seen:
            continue
        cyc, x = [], j
        while x not in seen:
            seen.add(x)
            cyc.append(x)
            x = img[x]
        out.append(tuple(sorted(cyc)))
    return sorted(out)
