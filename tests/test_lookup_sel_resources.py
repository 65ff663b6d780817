"""Build-time check (no GPU): the compiler's per-kernel resource report (-Rpass-analysis=kernel-resource-usage, gfx950) of the
kernels the lookup selectors add.  A SEL quotient kernel must not spill where its sibling without selectors does not, and the
selector probe and the selector step of the running fraction must not spill at all.  The figures are printed for DESIGN."""
import os
import re
import subprocess
import tempfile

import pytest

from zkp_subnet_amd import build as kb


def report(src):
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run([kb._hipcc(), *kb.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(kb.CSRC, src), "-o",
                              os.path.join(tmp, "x.o")], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and name:
            out[name][m.group(1).split(" ")[0]] = int(m.group(2))
    return out


def test_the_sel_quotient_kernels_do_not_spill_where_their_siblings_do_not():
    rep = report("fr_quot.hip")
    sel = {k: v for k, v in rep.items() if "k_quot_points_sel" in k}
    assert len(sel) == 4, sorted(rep)
    for name, r in sorted(sel.items()):
        act, link = re.search(r"k_quot_points_selILb([01])ELb([01])E", name).groups()
        sib = [v for k, v in rep.items() if re.search(rf"13k_quot_pointsILb1ELb{act}ELb{link}E", k)]
        assert len(sib) == 1, name
        print(name, r, "sibling", sib[0])
        assert r["ScratchSize"] <= sib[0]["ScratchSize"], (name, r, sib[0])
        assert r["VGPRs"] <= sib[0]["VGPRs"] and r["Occupancy"] >= sib[0]["Occupancy"], (name, r, sib[0])


@pytest.mark.parametrize("src,kernel", [("fr_join.hip", "k_join_probe_sel"), ("fr_lookup.hip", "k_lk_step_sel")])
def test_the_builders_selector_kernels_do_not_spill(src, kernel):
    rep = {k: v for k, v in report(src).items() if kernel in k}
    assert rep
    for name, r in rep.items():
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)
