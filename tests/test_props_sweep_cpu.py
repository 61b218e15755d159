"""The host side of the lc/lp/pb sweep that needs no GPU: the canonical order of the 75 triples, the rule that picks
one from a table of costs, and the declaration in the C header."""
import os
import re

from megalania_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_triples_are_the_supported_ones_in_canonical_order():
    t = binding.PROPS_TRIPLES
    assert len(t) == 75 and len(set(t)) == 75
    assert all(lc + lp <= 4 and pb <= 4 and min(lc, lp, pb) >= 0 for lc, lp, pb in t)
    want = []
    for lc in range(5):
        for lp in range(5 - lc):
            for pb in range(5):
                want.append((lc, lp, pb))
    assert t == want
    assert t[0] == (0, 0, 0) and t[25] == (1, 0, 0) and t[-1] == (4, 0, 4)


def test_best_props_takes_the_first_of_equals():
    costs = [1000] * 75
    assert binding.best_props(costs) == (0, 0, 0)
    costs[binding.PROPS_TRIPLES.index((0, 2, 2))] = 999
    costs[binding.PROPS_TRIPLES.index((3, 0, 2))] = 999
    assert binding.best_props(costs) == (0, 2, 2)
    costs[0] = costs[25] = 5  # 0/0/0 and 1/0/0 tie on 7-bit text
    assert binding.best_props(costs) == (0, 0, 0)
    # u64 costs, as SA.props_sweep returns them
    import numpy as np
    big = np.full(75, (1 << 63) + 10, dtype=np.uint64)
    big[40] = (1 << 63) + 9
    assert binding.best_props(big) == binding.PROPS_TRIPLES[40]


def test_header_declares_the_sweep():
    hdr = open(os.path.join(ROOT, "include", "megalania_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bint\s+mgl_props_sweep\s*\(\s*mgl_sa\s*\*", code)
    assert re.search(r"#define\s+MGL_PROPS_TRIPLES\s+75\b", code)
    assert "mgl_props_cost" in code and "mgl_props_sweep" in binding.HIP_SYMBOLS
    assert "mgl_props_sweep" in hdr.split("#ifndef MEGALANIA_HIP_H")[0]  # the leading comment lists it
