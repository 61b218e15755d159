"""mgl_crossover on planted joints (tests/_planted_parse.py): at the edges of the 64-bit bitmap words, across the
1 024-word passes of k_xo_lastnz (inputs beyond 65 536 bytes), with parents that tie, under other lc/lp/pb, through
mgl_sa_cross_best at length, and with malformed entries on and off the walk.  Everything is compared with the Python
restatement of the rule as tests/test_gpu_crossover.py compares it (its check_parity): the child entry for entry and every
figure of mgl_cross_stats, exact integers all.  Each test first asserts on the rule's own output that the structure it is
about is there (tests/test_crossover_planted_cpu.py guards the generator without a GPU).  `-m gpu`."""
import functools
import lzma

import pytest

import _planted_parse as pp
from _libs import LONG_REP, Oracle
from megalania_amd import binding
from test_crossover_rule_cpu import as_slab, boundaries_of, check_valid, crossover_rule, walk_table
from test_gpu_crossover import MGL_EINVAL, _raw, check_parity

pytestmark = pytest.mark.gpu

CHUNK = 65536  # positions that one pass of k_xo_lastnz covers: 1 024 bitmap words
LONG = 3 * CHUNK + 777  # 3 085 words: three passes and a part of a fourth
WORD_SIZES = [63, 64, 65, 127, 128, 129, 4097]
WORD_GRAINS = lambda n: (1, 0, 2, 63, 64, 65, n, n + 1, 2**32 - 1)
CHUNK_GRAINS = lambda n: (1, 0, 65536, 65537, 70000, n + 1)
OTHER_PROPS = [(3, 0, 2), (0, 2, 2)]


def word_joints(n, D=16):
    """bits 63, 0 and 1 of the first words, n - 1 and, where there is room, a stretch of 271 positions without a joint
    ((129, 400): it spans four multiples of 64) and the two edges of the last words"""
    js = {j for j in (63, 64, 65, 127, 128, 129) if j < n}
    if n > 4096:
        js |= set(range(400, 4001, 300)) | {4031, 4032, 4095}
    if n - 1 >= D + 6:
        js.add(n - 1)
    return sorted(js)


def chunk_joints(n):
    """one every 2 999 positions, the edges of a word in the first pass, 65 535 where the input is longer, and n - 1"""
    return sorted(set(range(3001, n - 10, 2999)) | {4095, 4096, 4097, n - 1} | {j for j in (CHUNK - 1, CHUNK) if j < n})


LAYOUT_A = [4096, 30000, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK - 1, 3 * CHUNK, LONG - 1]
LAYOUT_B = sorted(set(range(5000, LONG, 5000)) | {LONG - 1})
TIE_JOINTS = {4097: [63, 128, 400, 1025, 2048, 4032], CHUNK + 1: [320, 4095, 20000, 40000, 1023 * 64]}


@functools.lru_cache(maxsize=2)  # the walk tables of a long case weigh tens of MB a parent
def planted(kind, n, P, props=(0, 0, 0)):
    """(data, parents, their walk tables under props) of a named construction"""
    D = 16 if n <= 4097 else 251
    data = pp.periodic_input(n, D, 0xA000 + n)
    if kind == "tie":
        parents = pp.tie_parents(n, D, TIE_JOINTS[n], seed=n)
    else:
        joints = {"word": word_joints, "chunk": chunk_joints, "A": lambda n: LAYOUT_A, "B": lambda n: LAYOUT_B}[kind](n)
        parents = pp.rotating_parents(n, D, joints, P, seed=n + P)
    return data, parents, [walk_table(data, p, *props) for p in parents]


def planted_behind_the_opening(r, D):
    return [q for q in r["joints"] if q > D + 2]


def run_grains(data, parents, tabs, grains, props=(0, 0, 0)):
    lc, lp, pb = props
    sa = binding.SA(data, neighbours_per_step=64, lc=lc, lp=lp, pb=pb)
    try:
        return [check_parity(sa, data, parents, g, props, tabs=tabs)[0] for g in grains]
    finally:
        sa.close()


@pytest.mark.parametrize("n", WORD_SIZES)
def test_joints_at_the_edges_of_bitmap_words(n):
    D, grains = 16, WORD_GRAINS(n)
    js = word_joints(n)
    cases = []
    for P in (2, 3, 8):
        data, parents, tabs = planted("word", n, P)
        r = crossover_rule(data, parents, 1, tabs=tabs)
        assert planted_behind_the_opening(r, D) == js + [n] and n - 1 in r["joints"]
        assert len({tuple(boundaries_of(r["joints"], n, g or 64)) for g in grains}) > 1
        if n > 4096:
            assert 129 in js and 400 in js and not [q for q in r["joints"] if 129 < q < 400]
            assert set(r["winners"]) == set(range(P)) and r["child_cost"] < min(r["parent_cost"])
        cases.append((parents, tabs))
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        for parents, tabs in cases:
            for g in grains:
                check_parity(sa, data, parents, g, tabs=tabs)
    finally:
        sa.close()


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1])
def test_one_pass_of_the_word_scan_and_one_word_more(n):
    """nw = n / 64 + 1 = 1 024 (one pass, full), 1 025 and 1 025 (one word into the second pass; for 65 536 bit n alone)"""
    P, D = 8, 251
    data, parents, tabs = planted("chunk", n, P)
    assert n // 64 + 1 == (1024 if n < CHUNK else 1025)
    r = crossover_rule(data, parents, 1, tabs=tabs)
    assert planted_behind_the_opening(r, D) == chunk_joints(n) + [n]
    assert n - 1 in r["joints"] and (n < CHUNK or CHUNK - 1 in r["joints"])
    assert set(r["winners"]) == set(range(P)) and r["child_cost"] < min(r["parent_cost"])
    run_grains(data, parents, tabs, CHUNK_GRAINS(n))


@pytest.mark.parametrize("P", [2, 3])
def test_three_passes_with_an_empty_second_one(P):
    """Layout A: no joint in [65 538, 196 604), which holds all of bitmap words 1 025..3 070.  The last set bit before
    196 607 is found through last[3 070], which k_xo_lastnz's third pass has from the carry of the second, and that one
    from word 1 024."""
    D = 251
    data, parents, tabs = planted("A", LONG, P)
    assert LONG // 64 + 1 == 3085
    r = crossover_rule(data, parents, 1, tabs=tabs)
    assert planted_behind_the_opening(r, D) == LAYOUT_A + [LONG]
    assert not [q for q in r["joints"] if CHUNK + 2 <= q < 3 * CHUNK - 4]
    at = r["bounds"].index(3 * CHUNK - 1)
    assert r["bounds"][at - 1] == CHUNK + 1  # the region that closes at 196 607 begins at 65 537
    assert r["winners"][at - 1] == (LAYOUT_A.index(3 * CHUNK - 1)) % P  # and goes to the parent that codes it with LONG_REPs
    wants = run_grains(data, parents, tabs, CHUNK_GRAINS(LONG))
    assert wants[4]["bounds"] == [0, 3 * CHUNK - 1, LONG]  # grain 70 000: 0, then the first joint at or behind 70 000


def test_three_passes_with_joints_in_every_one():
    """Layout B: a joint every 5 000 positions."""
    P, D = 3, 251
    data, parents, tabs = planted("B", LONG, P)
    r = crossover_rule(data, parents, 1, tabs=tabs)
    assert planted_behind_the_opening(r, D) == LAYOUT_B + [LONG]
    assert all(any(k * CHUNK <= q < (k + 1) * CHUNK for q in LAYOUT_B) for k in range(4))
    assert set(r["winners"]) == set(range(P)) and r["child_cost"] < min(r["parent_cost"])
    run_grains(data, parents, tabs, CHUNK_GRAINS(LONG))


@pytest.mark.parametrize("pair_first", [False, True], ids=["pair-last", "pair-first"])
@pytest.mark.parametrize("n", sorted(TIE_JOINTS))
def test_equal_parents_tie_to_the_lower_one(n, pair_first):
    """Two parents that walk alike and cost less than the third, all literals: every region goes to the lower of the two."""
    D = 16 if n <= 4097 else 251
    data, parents, tabs = planted("tie", n, 3)
    if pair_first:
        parents, tabs = parents[1:] + parents[:1], tabs[1:] + tabs[:1]
    a, b = (0, 1) if pair_first else (1, 2)
    grains = (1, 0, 65, n + 1)
    for g in grains:
        r = crossover_rule(data, parents, g, tabs=tabs)
        assert planted_behind_the_opening(r, D) == TIE_JOINTS[n] + [n]
        assert r["parent_cost"][a] == r["parent_cost"][b] < r["parent_cost"][3 - a - b]
        # regions inside the opening, which all three code alike, fall to parent 0; every region that reaches behind it is the pair's
        behind = [w for end, w in zip(r["bounds"][1:], r["winners"]) if end > D + 2]
        assert behind and set(behind) == {a} and r["regions_from"][b] == 0
    assert (parents[a] != parents[b]).any()  # off the walk: a region taken from the wrong one of the two shows in the child
    run_grains(data, parents, tabs, grains)


@pytest.mark.parametrize("props", OTHER_PROPS)
@pytest.mark.parametrize("kind,n", [("word", 4097), ("chunk", CHUNK + 1)])
def test_planted_joints_at_other_properties(kind, n, props):
    D = 16 if kind == "word" else 251
    data, parents, tabs = planted(kind, n, 3, props)
    js = word_joints(n) if kind == "word" else chunk_joints(n)
    r = crossover_rule(data, parents, 1, *props, tabs=tabs)
    assert planted_behind_the_opening(r, D) == js + [n]  # the walk state does not depend on lc/lp/pb
    assert set(r["winners"]) == {0, 1, 2}
    wants = run_grains(data, parents, tabs, (1, 0, 65, CHUNK), props)
    check_valid(data, wants[0]["child"], *props)


def test_cross_best_adopts_the_child_beyond_the_first_pass():
    """mgl_sa_cross_best at 197 385 bytes: the own best slab and the other one are the two parents of layout A."""
    data, (a, b), tabs = planted("A", LONG, 2)
    want = crossover_rule(data, [a, b], 0, tabs=tabs)
    assert want["child_cost"] < min(want["parent_cost"])  # so the rule says: the child is adopted
    cost_a = tabs[0][1][LONG]
    assert cost_a == want["parent_cost"][0]
    sa = binding.SA(data, neighbours_per_step=64, accept="single")
    try:
        sa.set_best(a, cost_a)
        st = sa.cross_best(b)
        assert st["adopted"] == 2 and st["parents"] == 2 and st["grain"] == 64
        assert st["parent_cost"] == want["parent_cost"] and st["child_cost"] == want["child_cost"]
        assert st["predicted"] == want["predicted"] and st["boundaries"] == want["boundaries"]
        assert st["regions_from"] == want["regions_from"]
        best, c = sa.best()
        assert (best == want["child"].astype(best.dtype)).all()
        assert c == want["child_cost"] == Oracle(data, dict_limit=0x400000).cost_slab(as_slab(best))["total"]
        assert lzma.decompress(binding.emit_stream(data, best), format=lzma.FORMAT_ALONE) == data
    finally:
        sa.close()


# ---- malformed entries.  k_rebuild, the walk behind mgl_cost_slab, tests type < LITERAL, type > LONG_REP and len == 0 in
# one condition, before the entry reaches the model; it raises the flag that makes mgl_cost_slab refuse, costs a literal in
# the entry's place and walks on from the next position.  All three classes are built, on one-byte packets (see
# _planted_parse.malformed).  k_xo_walk stops at such an entry instead; the code returned is the same.

def _bad_sites(n):
    """the first packet, a packet on bit 0 of a word, the last packet: one-byte packets in every parent of `word_joints`"""
    return (0, 128, n - 1)


def test_a_malformed_entry_on_the_walk_is_refused_like_mgl_cost_slab_refuses_it():
    n = 4097
    assert {127, 128, 129, n - 1} <= set(word_joints(n))  # literals at 128 and n - 1, whoever codes the regions around them
    data, good, tabs = planted("word", n, 8)
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        for cls in pp.POISON:
            for site in _bad_sites(n):
                for P in (2, 3, 8):
                    for slot in sorted({0, P // 2, P - 1}):
                        assert pp.on_walk(good[slot])[site]
                        bad = pp.malformed(good[slot], site, cls)
                        try:
                            sa.cost_slab(bad, want_cum=False)
                            rc = 0
                        except binding.MglError as e:
                            rc = e.rc
                        assert rc == MGL_EINVAL, (cls, site)
                        parents = good[:slot] + [bad] + good[slot + 1:P]
                        assert _raw(sa, sa.h, parents, P) == rc, (cls, site, P, slot)
        check_parity(sa, data, good[:3], 0, tabs=tabs[:3])  # the handle is as usable as before
    finally:
        sa.close()


@pytest.mark.parametrize("P", [2, 3, 8])
def test_malformed_entries_off_the_walk_are_ignored_and_copied(P):
    n, D = 4097, 16
    data = pp.periodic_input(n, D, 0xB000 + P)
    parents = pp.rotating_parents(n, D, word_joints(n), P, seed=P, poison=True)
    tabs = [walk_table(data, p) for p in parents]
    for p in parents:
        off = ~pp.on_walk(p)
        t, l = p["type"][off].astype(int), p["len"][off].astype(int)
        assert off.sum() > 100 and ((t == 0) | (t > LONG_REP) | (l == 0)).all()
    wants = run_grains(data, parents, tabs, (1, 0, 65, n + 1))
    child = wants[0]["child"]
    assert ((child["type"] == 0) | (child["type"] > LONG_REP) | (child["len"] == 0)).sum() > 100  # the poison travels
    check_valid(data, child)
