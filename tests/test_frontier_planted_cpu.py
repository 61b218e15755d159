"""The planted inputs of tests/_planted_frontier.py reach what they are for, stated against `frontier_rule` and its budget
counter, and they discriminate: a rule that is wrong by one at the limit a case is about gives another list at the case's
position i.  tests/test_gpu_frontier_edges.py holds the device to `frontier_rule` on the same inputs.  No GPU, no handle."""
import bisect

import numpy as np
import pytest

import test_match_frontier_cpu as tmf
from _planted_frontier import (CAPPED, EXACT_15, SINGLE_COPIES, TWO_STEP, all_planted, ladder, single_step, stairs, zero_run,
                               zero_tail)
from test_adaptive_rule_cpu import _mlen
from test_match_frontier_cpu import UNLIMITED, exact_frontier, frontier_rule

WINDOW = 0x400000


def at(data, i, depth=tmf.DEFAULT_DEPTH, dict_limit=WINDOW):
    """(the list at i, the budget position i used)"""
    used = []
    lists = frontier_rule(data, depth, dict_limit, stats=used)
    return lists[i], used[i]


def rule_variant(data, depth, dict_limit=WINDOW, lookup16_cost=0):
    """`frontier_rule` with one knob: what the look-up at need == 16 costs (the rule: nothing).  A copy, so that the rule
    itself stays as it is; with the knob at 0 it has to give the rule's lists (asserted below on every planted input)."""
    data = bytes(data)
    n = len(data)
    d = np.frombuffer(data, dtype=np.uint8)
    maps = {D: {} for D in tmf.LEVELS}
    out = []
    for i in range(n):
        cap = min(273, n - i)
        lst, best, budget, q_last = [], 1, depth, None
        while best < cap and len(lst) < tmf.MAX_ENTRIES:
            need = best + 1
            level = need if need <= 8 else (16 if need >= 16 else 8)
            run = maps[level].get(data[i:i + level], [])
            if need == level:
                paid = lookup16_cost if need == 16 else 0
                if not run or i - run[-1] - 1 >= dict_limit or budget < paid:
                    break
                budget -= paid
                q = run[-1]
            else:
                q = None
                for j in range(bisect.bisect_left(run, q_last) - 1, -1, -1):
                    if budget == 0 or i - run[j] - 1 >= dict_limit:
                        break
                    budget -= 1
                    if _mlen(d, run[j], i, cap) > best:
                        q = run[j]
                        break
                if q is None:
                    break
            best = _mlen(d, q, i, cap)
            lst.append((q, best))
            q_last = q
        out.append(lst)
        for D in tmf.LEVELS:
            if i + D <= n:
                maps[D].setdefault(data[i:i + D], []).append(i)
    return out


PLANTED = all_planted()


@pytest.mark.parametrize("name", list(PLANTED), ids=list(PLANTED))
def test_unlimited_depth_is_the_brute_force_frontier_on_every_planted_input(name):
    data, _ = PLANTED[name]
    assert len(data) < 6000
    full = frontier_rule(data, UNLIMITED)
    assert full == exact_frontier(data)
    for depth in (1, 64):
        assert rule_variant(data, depth) == frontier_rule(data, depth), depth  # the copy is the rule
    n = len(data)
    for i, lst in enumerate(full):
        assert all(data[q:q + l] == data[i:i + l] and (l == min(273, n - i) or data[q + l] != data[i + l]) for q, l in lst)


# ---- the 60-entry cap

def test_the_ladder_fills_a_list_to_the_cap():
    data, i = ladder(1, 75)
    assert (len(data), i) == (3038, 2923)
    for depth in (52, 53, 64, 4096):
        lst, used = at(data, i, depth)
        assert len(lst) == tmf.MAX_ENTRIES == 60 and lst[-1][1] == 61 and used == 52, depth
        assert [l for _, l in lst] == list(range(2, 62))
    lst, used = at(data, i, 40)
    assert len(lst) == 48 and used == 40
    assert max(len(f) for f in frontier_rule(data, 64)) == 60  # and no list is longer


def test_the_ladder_offers_74_lengths_and_tells_a_cap_of_59_or_61(monkeypatch):
    data, i = ladder(1, 75)
    right = at(data, i, 4096)[0]
    assert right == at(data, i, 64)[0]
    for wrong, entries in ((59, 59), (61, 61), (1000, 74)):  # without a cap: every length 2..75
        monkeypatch.setattr(tmf, "MAX_ENTRIES", wrong)
        lst, _ = at(data, i, 4096)
        assert len(lst) == entries and lst != right and lst[:59] == right[:59]
    monkeypatch.undo()
    assert at(data, i, 4096)[0] == right
    # the last entry needs the whole budget of 52: one less and one entry is missing
    assert len(at(data, i, 51)[0]) == 59 and at(data, i, 51)[0] != at(data, i, 52)[0]


# ---- the budget, with the deciding entry on lanes 62, 63 and 0 of a trip of 64

@pytest.mark.parametrize("copies", SINGLE_COPIES)
@pytest.mark.parametrize("length", [12, 20], ids=["run8", "run16"])
def test_a_single_step_spends_its_copies_then_takes_the_far_source(length, copies):
    data, i = single_step(length, copies)
    near = i - (length + 1)
    for depth in (copies - 2, copies - 1, copies, copies + 1):
        lst, used = at(data, i, depth)
        assert lst == ([(near, length)] if depth < copies else [(near, length), (0, 40)]), depth
        assert used == min(depth, copies), depth
    # a budget off by one, either way, shows at i
    assert at(data, i, copies)[0] != at(data, i, copies - 1)[0]      # the right depth with depth - 1
    assert at(data, i, copies - 1)[0] != at(data, i, copies - 1 + 1)[0]  # one too few with depth + 1


def test_two_steps_carry_the_budget_from_the_8_byte_run_into_the_16_byte_run():
    data, i = stairs(11, TWO_STEP)
    want = {69: 1, 70: 2, 199: 2, 200: 3}
    for depth, entries in want.items():
        lst, used = at(data, i, depth)
        assert len(lst) == entries and used == depth, depth
    lst, _ = at(data, i, 200)
    assert [l for _, l in lst] == [10, 24, 50] and lst[-1][0] == 0
    assert at(data, i, 201)[1] == 200
    assert at(data, i, 70)[0] != at(data, i, 69)[0] and at(data, i, 200)[0] != at(data, i, 199)[0]


# ---- the change of level out of the 8-byte run

def test_the_look_up_at_need_16_is_free():
    data, i = stairs(*EXACT_15["direct"])
    assert at(data, i, 1) == ([(41, 15), (0, 40)], 0)
    data, i = stairs(*EXACT_15["scanned"])
    lst, used = at(data, i, 1)
    assert [l for _, l in lst] == [10, 15, 40] and used == 1
    data, i = stairs(*EXACT_15["scanned_16"])
    assert [l for _, l in at(data, i, 1)[0]] == [10, 15, 16]
    assert at(data, i, 2) == ([(74, 10), (58, 15), (41, 16), (0, 40)], 2)


@pytest.mark.parametrize("name,depth", [("scanned", 1), ("scanned_16", 2)])
def test_a_look_up_that_costs_budget_shows(name, depth):
    data, i = stairs(*EXACT_15[name])
    right = frontier_rule(data, depth)[i]
    assert rule_variant(data, depth)[i] == right
    wrong = rule_variant(data, depth, lookup16_cost=1)[i]
    assert wrong != right and wrong == right[:-1]


# ---- the window

def test_a_source_exactly_on_the_window_edge():
    data, i = single_step(12, 64)
    near = i - 13
    assert at(data, i, 64, dict_limit=i)[0] == [(near, 12), (0, 40)]  # distance - 1 == i - 1 < dict_limit
    assert at(data, i, 64, dict_limit=i - 1)[0] == [(near, 12)]
    assert at(data, i, 64, dict_limit=WINDOW)[0] == [(near, 12), (0, 40)]
    # dict_limit off by one, either way, shows at i
    assert at(data, i, 64, dict_limit=i - 1)[0] != at(data, i, 64, dict_limit=i)[0]
    assert at(data, i, 64, dict_limit=(i - 1) + 1)[0] != at(data, i, 64, dict_limit=i - 1)[0]


def test_a_window_edge_in_the_middle_of_a_trip():
    data, i = stairs(7, [(12, 100), (40, 1)])
    near = i - 13
    dict_limit = 13 * 40  # occurrence k (1 = nearest) is at distance 13 k: k <= 40 are inside
    assert sum(1 for k in range(1, 101) if 13 * k - 1 < dict_limit) == 40
    for depth in (39, 40, 64, 4096):
        lst, used = at(data, i, depth, dict_limit)
        assert lst == [(near, 12)] and used == min(depth, 39), depth  # the nearest is free, 39 more are examined
    assert at(data, i, 4096)[0] == [(near, 12), (0, 40)]  # without the window the long one is taken


# ---- caps and the padding

def test_capped_lengths():
    data, i = stairs(*CAPPED["273"])
    assert at(data, i)[0][-1] == (0, 273) and len(data) - i == 300
    data, i = stairs(*CAPPED["end"])
    assert at(data, i)[0][-1] == (0, 100) and len(data) - i == 100


def test_zero_tails_give_ordinary_capped_lists():
    data = zero_run()
    n = len(data)
    assert frontier_rule(data) == [[]] + [[(p - 1, min(273, n - p))] for p in range(1, n - 1)] + [[]]
    data = zero_tail()
    n = len(data)
    lists = frontier_rule(data)
    assert lists == exact_frontier(data)
    assert all(l <= n - p for p, lst in enumerate(lists) for _, l in lst)  # nothing matches into the padding
    assert lists[n - 20][-1][1] == 20 and lists[n - 20][-1][0] < 500  # the tail: found in the longer run, cut at the end
    assert lists[n - 1] == []
