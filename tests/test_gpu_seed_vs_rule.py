"""`mgl_sa_seed_adaptive` over two passes against the rule iterated on the CPU.  The single-pass hook is pinned by
`adaptive_rule` (tests/test_gpu_adaptive.py), and a sweep by its members -- which run through the same batched kernels.
What neither pins is the hand-over from pass to pass: the resolve, the chunk starts and model snapshots taken from the
resolved parse, and the keeping of the best.  Here the CPU side is

    cur = slab_of(resolve(adaptive_rule(data, cur, ...)[0]))      starting from the greedy parse

and the device has to give, pass by pass, the rule's objective and the oracle's cost of `cur`, the oracle's cost of the
greedy parse, the argmin (ties to the earlier pass) and, as the current slab, the cheaper resolved parse entry for entry.

Inputs are the smallest that cross every seam: SMALL's "runs" (1 606 B) at chunk 512 has four chunks, chunk starts inside
a 273-byte rep packet and a last chunk shorter than the rest; c1 (4 096 B) at chunk 1000 under both ends of the settings.
`-m gpu`."""
import contextlib

import numpy as np
import pytest

from _libs import Oracle, literal_slab
from megalania_amd import binding
from test_adaptive_rule_cpu import adaptive_rule, resolve, slab_of
from test_gpu_optimal import SMALL, as_list, greedy_slab
from test_match_frontier_cpu import frontier_sources

pytestmark = pytest.mark.gpu

DATA = {name: bytes(data) for name, data in SMALL}
PASSES = 2

# name, input, seed settings, properties, from_current, frontier
CASES = [
    ("runs_chunk512", "runs", dict(cand=16, chunk=512, segment=64, ahead=128), {}, False, False),
    ("c1_cand16", "c1", dict(cand=16, chunk=1000, segment=64, ahead=128), {}, False, False),
    ("c1_cand1_seg300", "c1", dict(cand=1, chunk=1000, segment=300, ahead=0), {}, False, False),
    ("c1_lc3_pb2", "c1", dict(cand=16, chunk=1000, segment=64, ahead=128), dict(lc=3, lp=0, pb=2), False, False),
    ("c1_from_current", "c1", dict(cand=16, chunk=1000, segment=64, ahead=128), {}, True, False),
    ("c1_frontier", "c1", dict(cand=16, chunk=1000, segment=64, ahead=128), {}, False, True),
]


@pytest.mark.parametrize("name,which,kw,props,from_current,frontier", CASES, ids=[c[0] for c in CASES])
def test_two_passes_equal_the_rule_iterated(name, which, kw, props, from_current, frontier):
    data = DATA[which]
    oracle = Oracle(data, dict_limit=0x400000, **props)
    # pass 0's starts: the greedy parse of the seed's own `cand`; with from_current whatever slab the handle holds
    start, _ = greedy_slab(data, cand=8 if from_current else kw["cand"], **props)
    start_cost = oracle.cost_slab(np.ascontiguousarray(start).astype(literal_slab(1).dtype))["total"]

    sa = binding.SA(data, accept="single", neighbours_per_step=16, **props)
    if frontier:
        sa.set_match_finder(binding.MF_FRONTIER)
    if from_current:
        sa.set_slab(start)
    st = sa.seed_adaptive(passes=PASSES, from_current=from_current, **kw)
    got, got_cost = sa.current()
    sa.close()

    cur, parses, costs, objectives = start, [], [], []
    with frontier_sources() if frontier else contextlib.nullcontext():
        for _ in range(PASSES):
            want, obj, _ = adaptive_rule(data, cur, kw["cand"], kw["chunk"], kw["segment"], kw["ahead"], **props)
            cur = slab_of(resolve(want))
            parses.append(cur)
            costs.append(oracle.cost_slab(cur)["total"])
            objectives.append(obj)
    print(f"{name}: start {start_cost}, device cost {st['cost']} objective {st['objective']} best {st['best_pass']}; "
          f"rule cost {costs} objective {objectives}")

    assert st["passes"] == PASSES
    assert st["greedy_cost"] == start_cost
    assert st["objective"] == objectives
    assert st["cost"] == costs
    # the cheapest pass, ties to the earlier; a current slab that competes has to be beaten
    best_pass, best = None, start_cost if from_current else None
    for p, c in enumerate(costs):
        if best is None or c < best:
            best_pass, best = p, c
    assert st["best_pass"] == best_pass
    assert got_cost == best
    assert as_list(got) == as_list(start if best_pass is None else parses[best_pass])

