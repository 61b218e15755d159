"""The planted-joint generator (tests/_planted_parse.py) against the Python restatement of the crossover rule, without a
GPU: what tests/test_gpu_crossover_edges.py relies on -- the parses are valid, their rep distances never move, the planted
joints are joints, a "rep" stretch against a "lit" one has none, rotating parents make the winners rotate and two equal
parents tie -- so that those tests cannot pass with the structure they are about missing."""
import numpy as np
import pytest

import _planted_parse as pp
from _libs import LITERAL, LONG_REP, MATCH, SHORT_REP
from test_crossover_rule_cpu import brute_boundaries, check_valid, crossover_rule, walk_table

SIZES = [63, 64, 65, 128, 129, 1000]
PERIODS = [3, 16, 251]


def planted_for(n, D):
    """joints on the word edges below n, one long gap, and n - 1"""
    js = [j for j in (63, 64, 65, 127, 128, 129, 500, 640, 641) if D + 5 <= j < n]
    if n - 1 >= D + 6:
        js.append(n - 1)
    return sorted(set(js))


def every_style(n, D, seed):
    """one parse per style behind D + 2, and one that changes style at every planted joint"""
    if n < D + 2:
        return [pp.planted_parse(n, D, [])]
    js = planted_for(n, D)
    out = [pp.planted_parse(n, D, pp.layout(n, D, js, [s] * (len(js) + 1)), seed + i) for i, s in enumerate(pp.STYLES)]
    out.append(pp.planted_parse(n, D, pp.layout(n, D, js, [pp.STYLES[r % 4] for r in range(len(js) + 1)]), seed + 9))
    out.append(pp.planted_parse(n, D, pp.layout(n, D, js, ["mix"] * (len(js) + 1)), seed + 10, poison=True))
    return out


@pytest.mark.parametrize("D", PERIODS)
@pytest.mark.parametrize("n", SIZES)
def test_every_generated_parse_is_valid_and_keeps_its_rep_distances(n, D):
    data = pp.periodic_input(n, D, 100 + D)
    assert len(data) == n and data[D:] == data[:max(0, n - D)] and data == pp.periodic_input(n, D, 100 + D)
    parses = every_style(n, D, 7) + (pp.rotating_parents(n, D, planted_for(n, D), 3, 5) if n >= D + 2 else [])
    for slab in parses:
        assert slab.dtype == np.dtype(pp.PACKET) and len(slab) == n
        check_valid(data, slab)
        S, _ = walk_table(data, slab)
        assert all(s[1:] == (D - 1, 0, 0, 0) for q, s in S.items() if q >= D + 2)
        on = pp.on_walk(slab)
        assert sorted(S) == list(np.nonzero(on)[0])
        if n >= D + 2:
            assert tuple(slab[D]) == (MATCH, D - 1, 2) and (slab["type"][:D] == LITERAL).all()
            assert set(slab["type"][on][D + 1:]) <= {LITERAL, SHORT_REP, LONG_REP} and (slab["dist"][on][D + 1:] == 0).all()


def test_the_styles_are_what_they_say():
    n, D = 1000, 16
    lit, rep, short, mix = (pp.planted_parse(n, D, [(n, s)], 3) for s in pp.STYLES)
    for slab, kinds in ((lit, {LITERAL}), (rep, {LONG_REP}), (short, {SHORT_REP}), (mix, {LITERAL, SHORT_REP, LONG_REP})):
        on = pp.on_walk(slab)
        on[:D + 2] = False
        assert set(slab["type"][on]) == kinds
    lens = rep["len"][pp.on_walk(rep)][D + 1:]
    assert {2, 273} <= set(lens) and lens.min() >= 2 and lens.max() <= 273
    assert set(pp.rep_lengths(3)) >= set(lens[:-1])  # all but the cut one come from the list
    # a "rep" stretch of one position is the leftover literal; longer ones end with a LONG_REP
    for width in range(1, 12):
        s = pp.planted_parse(600, D, [(300, "lit"), (300 + width, "rep"), (600, "lit")], 3)
        on = pp.on_walk(s)
        kinds = s["type"][300:300 + width][on[300:300 + width]]
        assert (kinds == (LITERAL if width == 1 else LONG_REP)).all() and on[300 + width]


def test_off_walk_entries_are_stale_and_well_formed_or_poison():
    n, D = 4097, 16
    data = pp.periodic_input(n, D, 1)
    segs = [(n, "rep")]
    clean = pp.planted_parse(n, D, segs, 3, stale=False)
    stale = pp.planted_parse(n, D, segs, 3)
    bad = pp.planted_parse(n, D, segs, 3, poison=True)
    on = pp.on_walk(stale)
    for slab in (clean, bad):
        assert (pp.on_walk(slab) == on).all() and (slab[on] == stale[on]).all()
    assert (clean["type"][~on] == LITERAL).all()
    off = np.nonzero(~on)[0]
    assert set(stale["type"][off]) == {LITERAL, MATCH, SHORT_REP, LONG_REP}
    for p in off:
        t, d, l = (int(x) for x in stale[p])
        assert 1 <= l <= min(273, n - p) and (l >= 2) == (t in (MATCH, LONG_REP))
        if t == MATCH:
            assert (d + 1) % D == 0 and d + 1 <= p and data[p:p + l] == data[p - d - 1:p - d - 1 + l]
        if t == LONG_REP:
            assert d < 4
    t, l = bad["type"][off].astype(int), bad["len"][off].astype(int)
    assert ((t == 0) | (t > LONG_REP) | (l == 0)).all()
    assert (t == 0).any() and (t > LONG_REP).any() and ((l == 0) & (t >= LITERAL) & (t <= LONG_REP)).any()
    # on the walk: one-byte packets only
    for cls in pp.POISON:
        m = pp.malformed(stale, 3, cls)
        assert (m != stale).sum() == 1 and (int(m[3]["type"]) in (0, LONG_REP + 1) or int(m[3]["len"]) == 0)
    with pytest.raises(AssertionError):
        pp.malformed(stale, D, "type0")


@pytest.mark.parametrize("D", [16, 251])
@pytest.mark.parametrize("P", [2, 3])
def test_planted_joints_are_joints_and_rotating_parents_rotate(P, D):
    n = 1000 if D == 16 else 2600
    data = pp.periodic_input(n, D, 2)
    js = sorted(planted_for(n, D) + ([1500, 2000, 2047, 2048, 2049] if n > 2049 else []))
    parents = pp.rotating_parents(n, D, js, P, 11)
    r = crossover_rule(data, parents, 1)
    assert set(js) <= set(r["joints"])
    # nothing else behind the opening that all parents share: a "rep" stretch meets a "lit" one nowhere inside
    assert [q for q in r["joints"] if q > D + 2] == js + [n]
    assert set(r["winners"]) == set(range(P))
    assert sum(r["regions_from"]) == r["boundaries"] - 1 and min(r["regions_from"]) > 0
    assert r["child_cost"] < min(r["parent_cost"])
    check_valid(data, r["child"])


@pytest.mark.parametrize("style", ["rep", "short"])
def test_a_rep_stretch_against_a_literal_one_has_no_joint_inside(style):
    n, D = 1000, 16
    data = pp.periodic_input(n, D, 3)
    js = [64, 500, 900]
    a = pp.planted_parse(n, D, pp.layout(n, D, js, [style] * 4), 1)
    b = pp.planted_parse(n, D, pp.layout(n, D, js, ["lit"] * 4), 2)
    r = crossover_rule(data, [a, b], 1)
    assert [q for q in r["joints"] if q > D + 2] == js + [n]
    # two parents of one style and one seed walk alike: every packet start is a joint
    same = crossover_rule(data, [a, a.copy()], 1)
    assert same["joints"] == sorted(walk_table(data, a)[0]) + [n]


@pytest.mark.parametrize("pair_first", [False, True], ids=["pair-last", "pair-first"])
def test_equal_parents_tie_to_the_lower_one(pair_first):
    n, D = 1000, 16
    data = pp.periodic_input(n, D, 4)
    js = [63, 128, 400, 705]
    parents = pp.tie_parents(n, D, js, 5, pair_first)
    a, b = (0, 1) if pair_first else (1, 2)
    on = pp.on_walk(parents[a])
    assert (parents[a][on] == parents[b][on]).all() and (pp.on_walk(parents[b]) == on).all()
    assert (parents[a] != parents[b]).any()  # the off-walk entries tell the two apart
    for grain in (1, 0, 65):
        r = crossover_rule(data, parents, grain)
        assert r["parent_cost"][a] == r["parent_cost"][b] < r["parent_cost"][3 - a - b]
        # regions inside the opening, which all three code alike, fall to parent 0; every region that reaches behind it is the pair's
        behind = [w for end, w in zip(r["bounds"][1:], r["winners"]) if end > D + 2]
        assert len(behind) >= 2 and set(behind) == {a}
        assert r["regions_from"][b] == 0
        assert [q for q in r["joints"] if q > D + 2] == js + [n]


@pytest.mark.parametrize("grain", [1, 2, 63, 64, 65])
def test_boundaries_at_word_edges_are_the_set_the_definition_names(grain):
    n, D = 1000, 16
    data = pp.periodic_input(n, D, 5)
    js = [127, 128, 129, 400, 639, 640, 641, 999]  # 64 k - 1, 64 k, 64 k + 1; (129, 400) spans 192, 256, 320 and 384
    r = crossover_rule(data, pp.rotating_parents(n, D, js, 2, 6), grain)
    assert [q for q in r["joints"] if q > D + 2] == js + [n]
    assert r["bounds"] == brute_boundaries(r["joints"], n, grain)
    if grain > 2:
        assert [b for b in r["bounds"] if 129 < b <= 400] == [400]  # one boundary for the whole stretch
