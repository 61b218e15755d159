"""The rule of the parses' second match finder (`MGL_MF_FRONTIER`, mgl_matchfinder.hip) restated in plain Python, and
what can be said about it without a GPU.  tests/test_gpu_match_frontier.py holds the device against `frontier_rule`.

The frontier F(i) of position i: (q_1, l_1), (q_2, l_2), ... where q_k is the nearest earlier position whose match at i
is longer than l_(k-1) (l_0 = 1).  The device finds it through its exact-prefix orders (2..8 and 16 bytes), and bounds
the work per position by `depth`:

    cap = min(273, n - i); best = 1; budget = depth; list = []; q_last = none
    while best < cap and len(list) < 60:
        need  = best + 1
        level = need if need <= 8 else (16 if need >= 16 else 8)
        R = earlier positions q < i with data[q:q+level] == data[i:i+level], nearest first
        if need == level:   q = first of R; stop if none or i - q - 1 >= dict_limit            (costs no budget)
        else:               go through R from just beyond q_last; each entry examined costs 1 of budget; stop (the list
                            is final) at budget == 0, at the end of R, or at i - q - 1 >= dict_limit; q = the first
                            examined entry with matchlen(q, i, cap) > best
        list.append((q, matchlen(q, i, cap))); best = that length; q_last = q

With unlimited depth this is the brute-force frontier (`exact_frontier`).  `frontier_sources` swaps the lists in as the
MATCH sources of `adaptive_rule` and `dp_rule`, which is what the node loops do under MGL_MF_FRONTIER."""
import bisect
import contextlib
import functools
import lzma

import numpy as np
import pytest

import test_adaptive_rule_cpu as tar
import test_gpu_optimal as tgo
from _libs import Oracle
from megalania_amd import binding, corpus
from test_adaptive_rule_cpu import _mlen, adaptive_rule, greedy_in, resolve, slab_of
from test_gpu_optimal import SMALL, dp_rule, prices_rule

UNLIMITED = 1 << 30
LEVELS = (2, 3, 4, 5, 6, 7, 8, 16)
MAX_ENTRIES = 60  # 64 lanes of a node's wavefront minus the four rep lanes
DEFAULT_DEPTH = 64


def frontier_rule(data, depth=DEFAULT_DEPTH, dict_limit=0x400000, stats=None):
    """per position: [(q, match length)]; stats (a list) receives the budget each position used"""
    data = bytes(data)
    n = len(data)
    d = np.frombuffer(data, dtype=np.uint8)
    maps = {D: {} for D in LEVELS}  # prefix -> earlier positions, ascending
    out = []
    for i in range(n):
        cap = min(273, n - i)
        lst, best, budget, q_last = [], 1, depth, None
        while best < cap and len(lst) < MAX_ENTRIES:
            need = best + 1
            level = need if need <= 8 else (16 if need >= 16 else 8)
            run = maps[level].get(data[i:i + level], [])
            if need == level:
                if not run or i - run[-1] - 1 >= dict_limit:
                    break
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
        if stats is not None:
            stats.append(depth - budget)
        out.append(lst)
        for D in LEVELS:
            if i + D <= n:
                maps[D].setdefault(data[i:i + D], []).append(i)
    return out


def exact_frontier(data, dict_limit=0x400000):
    """brute force: every earlier position of the bigram bucket, nearest first; keep each one longer than all nearer ones"""
    data = bytes(data)
    n = len(data)
    d = np.frombuffer(data, dtype=np.uint8)
    buckets, out = {}, []
    for i in range(n):
        lst = []
        if i + 1 < n:
            b = buckets.setdefault(data[i:i + 2], [])
            cap, best = min(273, n - i), 1
            for q in reversed(b):
                if i - q - 1 >= dict_limit or best == cap or len(lst) == MAX_ENTRIES:
                    break
                ml = _mlen(d, q, i, cap)
                if ml > best:
                    lst.append((q, ml))
                    best = ml
            b.append(i)
        out.append(lst)
    return out


@functools.lru_cache(maxsize=16)
def cached_frontier(data, depth, dict_limit):
    return frontier_rule(data, depth, dict_limit)


@contextlib.contextmanager
def frontier_sources(depth=DEFAULT_DEPTH):
    """adaptive_rule and dp_rule read a node's MATCH sources from the module-level `_sources` / `candidates`: inside
    this block both hand out the frontier (their `cand` argument is then unused, as on the device).  The attributes are
    replaced, so `_sources`' lru_cache neither serves nor keeps a list of the other kind."""
    saved = tar._sources, tgo.candidates
    tar._sources = lambda data, cand, dict_limit: cached_frontier(bytes(data), depth, dict_limit)
    tgo.candidates = lambda data, cand, dict_limit: [[q for q, _ in lst] for lst in cached_frontier(bytes(data), depth, dict_limit)]
    try:
        yield
    finally:
        tar._sources, tgo.candidates = saved


EXACT_INPUTS = [(name, data, 0x400000) for name, data in SMALL[:4]] + [("run", b"a" * 3000, 0x400000), ("prose_w300", SMALL[1][1], 300),
                                                                       ("elf_w300", SMALL[2][1], 300)]


@pytest.mark.parametrize("name,data,dict_limit", EXACT_INPUTS, ids=[e[0] for e in EXACT_INPUTS])
def test_unlimited_depth_is_the_brute_force_frontier(name, data, dict_limit):
    got = frontier_rule(data, UNLIMITED, dict_limit)
    assert got == exact_frontier(data, dict_limit)
    n = len(data)
    for i, lst in enumerate(got):
        assert len(lst) <= MAX_ENTRIES
        assert all(q < i and i - q - 1 < dict_limit and 2 <= l <= min(273, n - i) for q, l in lst)
        assert all(a[0] > b[0] and a[1] < b[1] for a, b in zip(lst, lst[1:]))  # farther and longer along a list
        assert all(data[q:q + l] == data[i:i + l] and (l == min(273, n - i) or data[q + l] != data[i + l]) for q, l in lst)


@pytest.mark.parametrize("name,data,dict_limit", EXACT_INPUTS, ids=[e[0] for e in EXACT_INPUTS])
def test_a_budget_only_cuts_lists_short(name, data, dict_limit):
    full = frontier_rule(data, UNLIMITED, dict_limit)
    for depth in (1, 8):
        used = []
        cut = frontier_rule(data, depth, dict_limit, stats=used)
        assert max(used) <= depth
        assert all(c == f[:len(c)] for c, f in zip(cut, full)), depth
        # lengths 2..8 cost nothing: whatever the budget, a list reaches as far as the direct look-ups go
        assert all(len(c) >= sum(1 for _, l in f if l <= 8) for c, f in zip(cut, full)), depth


def test_the_small_inputs_reach_every_path_of_the_scan():
    """what tests/test_gpu_match_frontier.py relies on: `runs` has a list of 49 entries and a position that examines 692
    run entries (more than ten trips of a 64-lane wavefront), and the ELF slice has lists that a depth of 64 cuts short.
    What no natural input reaches (a list of 60, a budget that ends on a trip's edge, a source on the window's edge) is
    planted: tests/_planted_frontier.py, tests/test_frontier_planted_cpu.py"""
    used = []
    full = frontier_rule(SMALL[3][1], 4096, stats=used)
    assert max(len(f) for f in full) == 49 and max(used) == 692
    elf = SMALL[2][1]
    assert frontier_rule(elf, 64) != frontier_rule(elf, 4096)
    assert any(l > 16 for f in frontier_rule(elf, 64) for _, l in f)  # the 16-byte run is scanned too


def _valid(data, res, dict_limit=0x400000):
    n, pos, reps = len(data), 0, (0, 0, 0, 0)
    while pos < n:
        t, d, l = (int(x) for x in res[pos])
        if t != tgo.LIT:
            D = (d if t == tgo.MATCH else reps[d if t == tgo.LONG_REP else 0]) + 1
            assert D <= pos and data[pos:pos + l] == data[pos - D:pos - D + l], pos
            assert t != tgo.MATCH or d < dict_limit
        _, reps = tgo.advance(0, reps, t, d)
        pos += l
    assert pos == n


@pytest.mark.parametrize("lc,lp,pb", [(0, 0, 0), (3, 0, 2)])
@pytest.mark.parametrize("name,data", SMALL[:4], ids=[s[0] for s in SMALL[:4]])
def test_both_rules_parse_from_the_frontier(name, data, lc, lp, pb):
    g = greedy_in(data)
    with frontier_sources():
        a, a_obj, _ = adaptive_rule(data, g, 16, 1000, 64, 128, lc=lc, lp=lp, pb=pb)
        s, s_obj = dp_rule(data, prices_rule(data, g, lc, lp, pb), 16, 1000, lc=lc, lp=lp, pb=pb)
    assert tar._sources.__name__ == "_sources" and tgo.candidates.__name__ == "candidates"  # and both are back
    for got, obj in ((a, a_obj), (s, s_obj)):
        res = slab_of(resolve(got))
        _valid(data, res)
        assert obj > 0 and Oracle(data, lc=lc, lp=lp, pb=pb, dict_limit=0x400000).cost_slab(res)["total"] > 0
        assert lzma.decompress(binding.emit_stream(data, res, lc=lc, lp=lp, pb=pb), format=lzma.FORMAT_ALONE) == data


def test_the_frontier_parses_prose_cheaper_than_the_nearest_sixteen():
    """Two passes from the greedy parse at chunk 4 096 / segment 64 / ahead 128: the exact cost of the second pass's parse.
    Measured with this restatement, payload only: 8 467.4 B from the frontier against 8 503.8 B from the nearest 16."""
    data = corpus.prose_like(20000, 0x51)
    o = Oracle(data, dict_limit=0x400000)

    def two_passes():
        cur = greedy_in(data)
        for _ in range(2):
            cur = slab_of(resolve(adaptive_rule(data, cur, 16, 4096, 64, 128)[0]))
        return o.cost_slab(cur)["total"]

    nearest = two_passes()
    with frontier_sources():
        frontier = two_passes()
    print(f"prose 20 000 B, payload: frontier {frontier / 16384:.1f} B, nearest-16 {nearest / 16384:.1f} B")
    assert frontier < nearest
