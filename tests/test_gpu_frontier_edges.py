"""The frontier match finder and the parses' node loops at their stated limits (mgl_matchfinder.hip, `opt_node` in
mgl_optimal.hip, the segments and commits of mgl_adaptive.hip), on the inputs of tests/_planted_frontier.py, which reach
each limit on purpose; tests/test_frontier_planted_cpu.py shows on the CPU that they do and that a rule wrong by one gives
another list there.  The device is held to the same restatements as on the natural inputs: `frontier_rule` entry for entry,
`dp_rule` and `adaptive_rule` packet for packet plus the objective, the oracle's costing and liblzma for the seeds.  `-m gpu`.

  the 60-entry cap (`cnt >= MGL_MF_MAX_ENTRIES`; lanes 53..63 of a node)   the ladder: lists and node loops under "frontier"
  cand = 30, nsrc = 64                                                    the ladder and prose under "nearest", the sweep
  the budget around a trip of 64 run entries                              the single steps, N = 63, 64, 65, 128, 129
  8-byte run -> need == 16 -> 16-byte run, a budget spent in both         the exact-15 stairs, the two-step stairs
  a source on the window's edge, an edge inside a trip                    the window cases
  lengths capped at 273 and by the end; a tail like the padding           the cap cases, the zero tails
  ahead = 273, chunk = 512, commits of one packet, segment > the ring     SETTINGS and the segment-1 case"""
import contextlib
import lzma

import numpy as np
import pytest

import test_gpu_adaptive as tga
import test_gpu_match_frontier as tgmf
import test_gpu_optimal as tgo
import test_gpu_parse_sweep as tgps
from _libs import literal_slab
from _planted_frontier import CAPPED, EXACT_15, SINGLE_COPIES, TWO_STEP, ladder, single_step, stairs, zero_run, zero_tail
from megalania_amd import binding
from test_gpu_optimal import SMALL, as_list, dp_rule, greedy_slab, nprobs, prices_rule
from test_match_frontier_cpu import cached_frontier, frontier_sources

pytestmark = pytest.mark.gpu

WINDOW = 0x400000
LADDER, LADDER_I = ladder(1, 75)
PROSE = SMALL[1][1]


def _list_cases():
    """(id, data, dict_limit, depths): one handle each, a call of mgl_match_frontier per depth"""
    out = [("ladder", LADDER, WINDOW, (40, 52, 53, 64, 4096))]
    for length in (12, 20):
        for copies in SINGLE_COPIES:
            out.append((f"single_{length}x{copies}", single_step(length, copies)[0], WINDOW, (copies - 1, copies, copies + 1)))
    out.append(("two_step", stairs(11, TWO_STEP)[0], WINDOW, (69, 70, 199, 200)))
    for name, (seed, steps) in EXACT_15.items():
        out.append((f"exact15_{name}", stairs(seed, steps)[0], WINDOW, (1, 2)))
    data, i = single_step(12, 64)
    for which, dict_limit in (("outside", i - 1), ("inside", i), ("open", WINDOW)):  # the far source, at 0: inside iff i - 1 < dict_limit
        out.append((f"window_{which}", data, dict_limit, (63, 64, 65)))
    data, i = stairs(7, [(12, 100), (40, 1)])
    out.append(("window_mid_trip", data, 13 * 40, (39, 40, 64, 4096)))  # 40 of the 100 short occurrences are inside
    for name, (seed, steps) in CAPPED.items():
        out.append((f"capped_{name}", stairs(seed, steps)[0], WINDOW, (64, 4096)))
    out += [("zero_run", zero_run(), WINDOW, (64,)), ("zero_tail", zero_tail(), WINDOW, (64,))]
    return out


LIST_CASES = _list_cases()


@pytest.mark.parametrize("name,data,dict_limit,depths", LIST_CASES, ids=[c[0] for c in LIST_CASES])
def test_lists_match_the_rule_at_the_limit(name, data, dict_limit, depths):
    sa = tgmf._sa(data, dict_limit=dict_limit)
    before = sa.current()
    for depth in depths:
        off, src, ln, _ = sa.match_frontier(depth)
        want = cached_frontier(data, depth, dict_limit)
        assert len(off) == len(data) + 1 and off[0] == 0 and off[-1] == len(src) == len(ln) == sum(len(w) for w in want), depth
        got = tgmf._lists(off, src, ln)
        assert got == want, (depth, next(i for i, (g, w) in enumerate(zip(got, want)) if g != w))
    after = sa.current()
    assert after[1] == before[1] and as_list(after[0]) == as_list(before[0])  # SA state untouched
    sa.close()


# ---- the node loops with every lane busy

SOURCES = [  # id, input, finder, cand
    ("ladder_frontier", LADDER, "frontier", 16),  # lists of 60: lanes 4..63 carry a source; cand is ignored
    ("ladder_nearest30", LADDER, "nearest", 30),  # 74 bigram and 72 four-byte predecessors at LADDER_I: nsrc = 64
    ("prose_nearest30", PROSE, "nearest", 30),
]
TRIPLES = [(0, 0, 0), (3, 0, 2)]
SETTINGS = [(1 << 16, 64, 273), (512, 64, 273), (1 << 16, 1500, 273), (1 << 16, 1500, 0)]  # chunk, segment, ahead
node_loops = pytest.mark.parametrize("name,data,finder,cand", SOURCES, ids=[s[0] for s in SOURCES])
triples = pytest.mark.parametrize("lc,lp,pb", TRIPLES, ids=["".join(map(str, t)) for t in TRIPLES])


def _handle(data, finder, lc, lp, pb):
    sa = tgmf._sa(data, lc=lc, lp=lp, pb=pb)
    sa.set_match_finder(finder)
    return sa, (frontier_sources() if finder == "frontier" else contextlib.nullcontext())


@triples
@node_loops
def test_optimal_pass_with_every_lane_busy(name, data, finder, cand, lc, lp, pb):
    assert len(data) % 512  # the last chunk of 512 is short
    sa, sources = _handle(data, finder, lc, lp, pb)
    before = sa.current()
    greedy = prices_rule(data, greedy_slab(data, lc=lc, lp=lp, pb=pb)[0], lc, lp, pb)
    uniform = np.full(2 * nprobs(lc, lp), 2048, dtype=np.uint32)
    with sources:
        for which, prices in (("greedy", greedy), ("uniform", uniform)):
            for chunk in (1 << 16, 512):
                got, obj = sa.optimal_pass(prices, cand, chunk)
                want, want_obj = dp_rule(data, prices, cand, chunk, lc=lc, lp=lp, pb=pb)
                what = (which, chunk)
                assert as_list(got) == want, (what, next(i for i, (g, w) in enumerate(zip(as_list(got), want)) if g != w))
                assert obj == want_obj, what
    after = sa.current()
    assert after[1] == before[1] and as_list(after[0]) == as_list(before[0])  # SA state untouched
    sa.close()


@pytest.mark.parametrize("start", ["greedy", "literal"])
@triples
@node_loops
def test_adaptive_pass_with_every_lane_busy(name, data, finder, cand, lc, lp, pb, start):
    parse_in = greedy_slab(data, lc=lc, lp=lp, pb=pb)[0] if start == "greedy" else literal_slab(len(data))
    sa, sources = _handle(data, finder, lc, lp, pb)
    with sources:
        for chunk, segment, ahead in SETTINGS:
            tga._check_pass(sa, data, parse_in, cand, chunk, segment, ahead, lc=lc, lp=lp, pb=pb)
    sa.close()


# Commits of one packet: segment 1, so the rule runs one shortest path per committed packet.  The first 1 600 bytes of the
# ladder (three chunks of 512 bytes and one of 64); `adaptive_rule` took 1.9 s per call at ahead 273 under nearest-30, 1.0 s
# under the frontier, and 0.06 s at ahead 0, on one CPU core: 6 s for the two cases, well inside the 20 s allowed.
SEGMENT_ONE = LADDER[:1600]


@pytest.mark.parametrize("finder,cand", [("nearest", 30), ("frontier", 16)])
def test_adaptive_pass_commits_packet_by_packet(finder, cand):
    data = SEGMENT_ONE
    assert 512 < len(data) and len(data) % 512
    sa, sources = _handle(data, finder, 0, 0, 0)
    with sources:
        for parse_in in (greedy_slab(data)[0], literal_slab(len(data))):
            for ahead in (273, 0):
                tga._check_pass(sa, data, parse_in, cand, 512, 1, ahead)
    sa.close()


@pytest.mark.parametrize("kind", ["adaptive", "optimal"])
def test_seeds_on_the_ladder_cost_what_the_oracle_says(kind):
    """cost == the oracle's, liblzma decodes the stream: under the frontier at depth 64 and under nearest with cand = 30"""
    tgmf._check_seed(kind, LADDER, 0, 0, 0, WINDOW, cand=16)
    (tga if kind == "adaptive" else tgo)._check_seed(LADDER, 0, 0, 0, WINDOW, cand=30)
    cur, _, _ = (tga if kind == "adaptive" else tgo)._check_seed(LADDER, 3, 0, 2, WINDOW, cand=30, chunk=512)
    assert lzma.decompress(binding.emit_stream(LADDER, cur, lc=3, lp=0, pb=2), format=lzma.FORMAT_ALONE) == LADDER


def test_a_sweep_with_cand_30_equals_its_members():
    variants = [(tgps.N, 30, 64, 273), (tgps.F, 16, 64, 273)]
    sa = tgmf._sa(LADDER)
    sw = sa.seed_sweep(variants, passes=2, chunk=512)
    cur, cost = sa.current()
    sa.close()
    alone = [tgps._alone(LADDER, v, passes=2, chunk=512) for v in variants]
    for v, (st, _, _) in enumerate(alone):
        for k in tgps.FIELDS:
            assert sw["results"][v][k] == st[k], (variants[v], k)
    (bv, bp), bc = tgps._argmin([a[0] for a in alone])
    assert sw["best_variant"] == bv and sw["results"][bv]["best_pass"] == bp
    assert cost == bc == alone[bv][2] and as_list(cur) == alone[bv][1]
    assert cost == tgps._oracle_cost(LADDER, cur)
    assert lzma.decompress(binding.emit_stream(LADDER, cur), format=lzma.FORMAT_ALONE) == LADDER
