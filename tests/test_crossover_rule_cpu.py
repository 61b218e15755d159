"""The crossover of parses (mgl_crossover) restated in Python, without a GPU.

Two valid parses of one input can be cut wherever both start a packet in the same walk state (ctx_state and the four rep
distances): on either side of such a cut the packets of either parse stay valid verbatim.  `crossover_rule` is the rule the
device must match integer for integer (tests/test_gpu_crossover.py compares against it); it is made of the oracle's running
totals (Oracle.cost_slab's `cum`) and test_gpu_optimal.advance only.  The tests here check what the rule promises -- the
child is a valid parse whose walk state equals every parent's at every boundary -- that the boundaries are the set the
definition names, and the reason to build it: the child of parents that one search evolved apart costs less than each."""
import bisect
import functools
import lzma
import os
import subprocess

import numpy as np
import pytest

from _libs import Oracle, literal_slab
from megalania_amd import binding, build, corpus
from test_adaptive_rule_cpu import greedy_in
from test_gpu_optimal import LIT, LONG_REP, MATCH, SMALL, advance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PK = literal_slab(1).dtype
DEFAULT_GRAIN = 64


def as_slab(slab):
    return np.ascontiguousarray(slab).astype(PK)


def walk_table(data, slab, lc=0, lp=0, pb=0):
    """Per packet start q of the slab's walk: S[q] = (ctx_state, rep0..rep3) before the packet, C[q] = the exact cost of the
    packets that start before q; C[n] = the total."""
    n = len(data)
    cum = Oracle(data, lc, lp, pb, dict_limit=0x400000).cost_slab(as_slab(slab))["cum"]
    S, Cq = {}, {}
    pos, ctx, reps, k = 0, 0, (0, 0, 0, 0), 0
    while pos < n:
        t, d, l = (int(x) for x in slab[pos])
        S[pos] = (ctx,) + reps
        Cq[pos] = int(cum[k - 1]) if k else 0
        ctx, reps = advance(ctx, reps, t, d)
        pos += l
        k += 1
    assert pos == n and k == len(cum)
    Cq[n] = int(cum[-1])
    return S, Cq


def boundaries_of(joints, n, grain):
    """The set definition: every joint (grain <= 1), else the first joint >= m * grain for every m >= 0, and n.  `joints` sorted."""
    if grain <= 1:
        return list(joints)
    out = {n}
    for m in range(n // grain + 1):
        out.add(joints[bisect.bisect_left(joints, m * grain)])  # n is a joint: there always is one
    return sorted(out)


def crossover_rule(data, parents, grain=0, lc=0, lp=0, pb=0, tabs=None):
    """The rule of mgl_crossover.  Returns the child and every figure of mgl_cross_stats (but gpu_ms), plus the joints, the
    boundary list and the winner of every region.  tabs: the parents' walk_table()s, where a caller has them already."""
    n, P = len(data), len(parents)
    assert 2 <= P <= 8 and all(len(p) == n for p in parents)
    grain = grain or DEFAULT_GRAIN
    tabs = tabs or [walk_table(data, p, lc, lp, pb) for p in parents]
    S0 = tabs[0][0]
    joints = sorted({0, n} | {q for q, s in S0.items() if all(S.get(q) == s for S, _ in tabs[1:])})
    bounds = boundaries_of(joints, n, grain)
    child = as_slab(parents[0]).copy()
    winners, predicted, regions_from = [], 0, [0] * P
    for b, b2 in zip(bounds, bounds[1:]):
        spans = [Cq[b2] - Cq[b] for _, Cq in tabs]
        w = spans.index(min(spans))  # ties to the lowest parent
        winners.append(w)
        predicted += spans[w]
        regions_from[w] += 1
        child[b:b2] = as_slab(parents[w])[b:b2]
    return dict(child=child, joints=joints, bounds=bounds, winners=winners, predicted=predicted, regions_from=regions_from,
                boundaries=len(bounds), parent_cost=[Cq[n] for _, Cq in tabs], grain=grain, parents=P,
                child_cost=Oracle(data, lc, lp, pb, dict_limit=0x400000).cost_slab(child)["total"])


def evolved(data, start, seed, steps=150, K=64, phase=2):
    """A parent: the best slab of Oracle.sa_batched run from `start`."""
    n = len(data)
    o = Oracle(data, dict_limit=0x400000)
    slab, best = as_slab(start).copy(), as_slab(start).copy()
    c0 = o.cost_slab(slab)["total"]
    o.sa_batched(slab, best, c0, c0, seed, K, phase, n, 0, steps)
    return best


@functools.lru_cache(maxsize=None)
def evolved_parents(name, count=4):
    data = {"prose": corpus.prose_like(6000, 0x51), "c2": corpus.config_input("c2")[0][:16384]}[name]
    start = greedy_in(data, 8)
    return data, start, [evolved(data, start, 1000 + i) for i in range(count)]


def check_valid(data, slab, lc=0, lp=0, pb=0):
    """the walk ends at n, every copy reproduces the input, and the stream decodes"""
    n = len(data)
    pos, ctx, reps = 0, 0, (0, 0, 0, 0)
    while pos < n:
        t, d, l = (int(x) for x in slab[pos])
        if t != LIT:
            D = (d if t == MATCH else reps[d if t == LONG_REP else 0]) + 1
            assert D <= pos and all(data[pos + k] == data[pos + k - D] for k in range(l)), pos
        ctx, reps = advance(ctx, reps, t, d)
        pos += l
    assert pos == n
    stream = binding.emit_stream(data, slab, lc, lp, pb)
    assert lzma.decompress(stream, format=lzma.FORMAT_ALONE) == data


def parents_for(name, data):
    """an all-literal parent, a greedy one and (long enough inputs) one the oracle's search moved away from the greedy one"""
    ps = [literal_slab(len(data)), greedy_in(data, 8)]
    if len(data) >= 1000:
        ps.append(evolved(data, ps[1], 7, steps=20, K=32))
    return ps


@pytest.mark.parametrize("grain", [1, 0, 1000])
@pytest.mark.parametrize("name,data", SMALL, ids=[s[0] for s in SMALL])
def test_child_is_a_valid_parse_and_meets_every_parent_at_the_boundaries(name, data, grain):
    n = len(data)
    ps = parents_for(name, data)
    r = crossover_rule(data, ps, grain)
    check_valid(data, r["child"])
    Sc, _ = walk_table(data, r["child"])
    tabs = [walk_table(data, p)[0] for p in ps]
    assert r["bounds"][0] == 0 and r["bounds"][-1] == n and set(r["bounds"]) <= set(r["joints"])
    for b in r["bounds"][:-1]:
        assert b in Sc and all(S[b] == Sc[b] for S in tabs), b
    assert sum(r["regions_from"]) == r["boundaries"] - 1 == len(r["winners"])
    # what the regions cost their winners along the winners' own walks; the child's model has another history
    assert r["predicted"] <= min(r["parent_cost"])


def test_other_properties():
    data = SMALL[1][1]
    ps = parents_for("prose", data)
    r = crossover_rule(data, ps, 64, lc=3, lp=0, pb=2)
    check_valid(data, r["child"], 3, 0, 2)
    assert r["parent_cost"] == [Oracle(data, 3, 0, 2, dict_limit=0x400000).cost_slab(as_slab(p))["total"] for p in ps]


def test_identical_parents_give_the_parent_back():
    data = SMALL[1][1]
    g = greedy_in(data, 8)
    for grain in (1, 0, 1000):
        r = crossover_rule(data, [g, g.copy(), g.copy()], grain)
        assert (r["child"] == as_slab(g)).all() and r["child_cost"] == r["parent_cost"][0] == r["predicted"]
        assert r["regions_from"] == [r["boundaries"] - 1, 0, 0]  # ties go to the lowest parent


def test_a_grain_beyond_the_input_gives_the_cheapest_parent():
    data = SMALL[0][1]
    n = len(data)
    ps = parents_for("c1", data)
    r = crossover_rule(data, ps, n + 1)
    w = r["parent_cost"].index(min(r["parent_cost"]))
    assert r["bounds"] == [0, n] and r["winners"] == [w]
    assert (r["child"] == as_slab(ps[w])).all() and r["child_cost"] == r["predicted"] == r["parent_cost"][w]


def brute_boundaries(joints, n, grain):
    """the definition read position by position"""
    js = set(joints)
    if grain <= 1:
        return sorted(js)
    out = {n}
    for m in range(n // grain + 1):
        q = m * grain
        while q not in js:
            q += 1
        out.add(q)
    return sorted(out)


@pytest.mark.parametrize("grain", [1, 64, 1000])
def test_boundaries_are_the_set_the_definition_names(grain):
    name, data = SMALL[3]
    assert name == "runs"
    n = len(data)
    ps = [literal_slab(n), greedy_in(data, 8)]
    r = crossover_rule(data, ps, grain)
    gaps = [b - a for a, b in zip(r["joints"], r["joints"][1:])]
    assert max(gaps) > 2 * 64  # a joint-free stretch that spans several multiples of 64: one boundary, not several
    assert r["bounds"] == brute_boundaries(r["joints"], n, grain)
    if grain == 1:
        assert r["bounds"] == r["joints"]
    if grain == 64:
        a = r["joints"][gaps.index(max(gaps))]
        inside = [b for b in r["bounds"] if a < b <= a + max(gaps)]
        assert inside == [a + max(gaps)]
    check_valid(data, r["child"])


@pytest.mark.parametrize("name", ["prose", "c2"])
def test_the_child_of_evolved_parents_costs_less_than_each(name):
    """The reason to build it.  Parents: the best slabs of four searches (seeds 1000..1003, K = 64, 150 steps, phase 2) from
    one greedy parse; two and four of them crossed at grain 64."""
    data, start, parents = evolved_parents(name)
    start_cost = Oracle(data, dict_limit=0x400000).cost_slab(start)["total"]
    for count in (2, 4):
        r = crossover_rule(data, parents[:count], 64)
        print(f"{name}: start {start_cost / 16384:.1f} B, parents {[round(c / 16384, 1) for c in r['parent_cost']]}, "
              f"child {r['child_cost'] / 16384:.1f} B, {r['boundaries'] - 1} regions {r['regions_from']}")
        assert r["child_cost"] < min(r["parent_cost"]) < start_cost
        check_valid(data, r["child"])


def test_the_interface_names_the_new_calls():
    header = open(os.path.join(ROOT, "include", "megalania_hip.h")).read()
    for sym in ("mgl_crossover", "mgl_sa_cross_best", "mgl_sa_exchange_cross"):
        assert sym + "(" in header and sym in binding.HIP_SYMBOLS
    assert "MGL_XO_MAX_PARENTS 8" in header and "mgl_cross_stats" in header
    assert binding.XO_MAX_PARENTS == 8
    # the struct the binding hands over has the header's layout: two u32, 8 + 3 + 8 u64, one u32 (padded), one double
    assert binding.CrossStats.parent_cost.offset == 8 and binding.CrossStats.child_cost.offset == 72
    assert binding.CrossStats.regions_from.offset == 96 and binding.CrossStats.adopted.offset == 160
    assert binding.CrossStats.gpu_ms.offset == 168 and __import__("ctypes").sizeof(binding.CrossStats) == 176
    r = subprocess.run([build.CLI], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--exchange best|cross" in r.stderr and b"--cross-grain" in r.stderr


@pytest.mark.parametrize("args", [
    ["--cross-grain", "64"],
    ["--exchange", "best", "--cross-grain", "64"],
    ["--exchange", "mix"],
    ["--chains", "2", "--rank", "0", "--comm-file", "some.comm", "--transport", "shm", "--cross-grain", "64"],
], ids=["grain-alone", "grain-with-best", "unknown-mode", "grain-with-chains"])
def test_cli_refuses_before_it_touches_a_device(args, tmp_path):
    f = tmp_path / "in.bin"
    f.write_bytes(b"some input that is never opened")
    r = subprocess.run([build.CLI] + args + [str(f)], capture_output=True, timeout=60)
    assert r.returncode != 0 and r.stdout == b""
    assert b"usage:" in r.stderr and b"no HIP device" not in r.stderr
    assert not os.path.exists("some.comm")
