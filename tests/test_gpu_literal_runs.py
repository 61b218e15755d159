"""Runs of plain literals at the edges of the 64-position window (lit_run_take / lit_run_plan, csrc/mgl_device.h).

Five walks plan such a run seven literals at a time, nine lanes each: the neighbour kernel's removed packets, the model
replay, the parallel builder and both in-place accepts.  All of them cut a run at two literals, at seven and at the
window's edge, and under lc > 0 a literal at the window's first position has its previous byte in the input, not in the
window.  Random inputs reach those edges by chance; the parse planted here puts them at chosen positions.

The parse (tests/_planted_parse.py: a periodic input, literals and LONG_REPs of index 0 behind the opening MATCH): sixty
stretches of literals, each between two LONG_REPs.  The first literal behind a LONG_REP is coded with a match byte
(ctx_state 8 or 11), the ones behind it are plain (ctx_state < 7): a stretch of L + 1 literals is a plain run of L.  L takes
every value in 1..15, and for each L the plain run begins at a position = 62, 63, 0 and 1 (mod 64): runs of one (no run:
packet by packet), of two, of seven, of eight and nine (seven and a rest of one, of two), runs that end at a window's edge,
cross it, begin on it and one behind it.  Under lc/lp/pb = 3/0/2 and 0/0/0; every comparison is exact.  `-m gpu`."""
import functools

import numpy as np
import pytest

from _libs import LITERAL, LONG_REP, MATCH, SHORT_REP, Oracle, assert_same_base, canonical_base, literal_slab
from _planted_parse import periodic_input, planted_parse
from megalania_amd import binding

pytestmark = pytest.mark.gpu

D = 37                      # the input's period
LENGTHS = range(1, 16)
STARTS = (62, 63, 0, 1)     # mod 64
PROPS = [dict(lc=3, lp=0, pb=2), dict(lc=0, lp=0, pb=0)]
IDS = ["lc3lp0pb2", "lc0lp0pb0"]
WIN_DROPPED = 0xFFFFFFFE    # csrc/mgl_device.h: MGL_WIN_DROPPED


def P(slab):
    return np.ascontiguousarray(slab).astype(binding.PACKET)


def plain_runs(slab):
    """(first position, length) of every maximal run of plain literals on the walk: the ctx_state automaton of
    lzma_state.c, restated"""
    runs, pos, state, start = [], 0, 0, None
    while pos < len(slab):
        t = int(slab["type"][pos])
        plain = t == LITERAL and state < 7
        if plain and start is None:
            start = pos
        if not plain and start is not None:
            runs.append((start, pos - start))
            start = None
        if t == LITERAL:
            state = 0 if state < 4 else state - 3 if state < 10 else state - 6
        elif t == MATCH:
            state = 7 if state < 7 else 10
        elif t == LONG_REP:
            state = 8 if state < 7 else 11
        else:
            assert t == SHORT_REP
            state = 9 if state < 7 else 11
        pos += int(slab["len"][pos])
    if start is not None:
        runs.append((start, pos - start))
    return runs


@functools.lru_cache(maxsize=None)
def planted():
    """(input, slab): computed once, shared by every test, never written to"""
    segs, want, pos = [], [], D + 2
    for length in LENGTHS:
        for r in STARTS:
            first = pos + 3                      # room for a LONG_REP (two bytes at least) and the literal with a match byte
            start = first + (r - first) % 64     # the plain run's first position
            segs += [(start - 1, "rep"), (start + length, "lit")]
            want.append((start, length))
            pos = start + length
    n = pos + 40
    segs.append((n, "rep"))
    data = periodic_input(n, D, 0x117)
    slab = planted_parse(n, D, segs, seed=3)
    runs = plain_runs(slab)
    assert runs[0] == (0, D) and runs[1:] == want, (runs[:3], want[:2])   # (the D literals in front of the MATCH, then the planted runs)
    assert {(s % 64, length) for s, length in want} == {(r, length) for length in LENGTHS for r in STARTS}
    assert 3000 < n < 5000, n
    slab.setflags(write=False)
    return data, slab


def oracle_cost(o, slab) -> int:
    return o.cost_slab(np.array(slab).astype(literal_slab(1).dtype))["total"]


@pytest.mark.parametrize("props", PROPS, ids=IDS)
def test_planted_slab_costs_what_the_oracle_says(props):
    data, slab = planted()
    sa = binding.SA(data, accept="single", neighbours_per_step=8, seed=5, **props)
    sa.set_slab(P(slab))
    cur, cost = sa.current()
    sa.close()
    assert (cur == P(slab)).all()
    assert cost == oracle_cost(Oracle(data, dict_limit=0x400000, **props), slab)


@pytest.mark.parametrize("props", PROPS, ids=IDS)
def test_parallel_build_equals_serial_build(props):
    data, slab = planted()
    par = binding.SA(data, accept="single", neighbours_per_step=8, seed=5, **props)
    ser = binding.SA(data, accept="single", neighbours_per_step=8, seed=5, serial_build=True, snapshots=False, **props)
    par.set_slab(P(slab))
    ser.set_slab(P(slab))
    assert par.current()[1] == ser.current()[1]
    assert_same_base(canonical_base(par, P(slab)), canonical_base(ser, P(slab)), "planted literal runs")
    par.close()
    ser.close()


def lockstep(kind, steps, props, monkeypatch):
    """The pattern of Chains (tests/test_gpu_accept_giveups.py) from the planted slab: chain A patches its accepts in place,
    chain B has the in-place accept switched off and rebuilds after every accepted step, R only ever rebuilds from a slab.
    Step by step the same costs and counts; after every accepted step the same slab, the oracle's cost, and A's structures
    equal to R's rebuild.  Returns (accepted steps, of those patched in place)."""
    data, slab = planted()
    K, seed = 96, 5
    mk = lambda: binding.SA(data, accept=kind, neighbours_per_step=K, seed=seed, iters_per_epoch=10**7, **props)
    a = mk()
    off = "MGL_NO_INCREMENTAL_APPLY" if kind == "single" else "MGL_NO_BATCH"
    monkeypatch.setenv(off, "1")
    b = mk()
    monkeypatch.delenv(off)
    r = binding.SA(data, accept="single", neighbours_per_step=8, seed=seed, **props)
    o = Oracle(data, dict_limit=0x400000, **props)
    a.set_slab(P(slab))
    b.set_slab(P(slab))
    accepted = in_place = 0
    for s in range(steps):
        fb0 = a.batch_counters()[1] + a.batch_giveups() if kind == "bulk" else 0
        sa_, sb_ = a.run(1), b.run(1)   # (run raises on any MGL_ERR_* flag, MGL_ERR_REBUILD_MISMATCH included)
        for k in ("current_cost", "best_cost", "accepted", "evaluations"):
            assert sa_[k] == sb_[k], (kind, s, k, sa_[k], sb_[k])
        if not sa_["accepted"]:
            continue
        rebuilt = sa_["full_rebuilds"] if kind == "single" else a.batch_counters()[1] + a.batch_giveups() - fb0
        accepted += 1
        in_place += 0 if rebuilt else 1
        cur, cost = a.current()
        assert (cur == b.current()[0]).all(), (kind, s)
        assert cost == oracle_cost(o, cur), (kind, s)
        r.set_slab(cur)
        assert_same_base(canonical_base(a, cur), canonical_base(r, cur), (kind, s))
    for x in (a, b, r):
        x.close()
    return accepted, in_place


@pytest.mark.parametrize("props", PROPS, ids=IDS)
def test_single_steps_in_lockstep_with_the_rebuild(props, monkeypatch):
    accepted, in_place = lockstep("single", 12, props, monkeypatch)
    print(f"single: {accepted} of 12 steps accepted, {in_place} patched in place")
    assert in_place >= 1   # (else the accept walk was never run)


@pytest.mark.parametrize("props", PROPS, ids=IDS)
def test_bulk_steps_in_lockstep_with_the_rebuild(props, monkeypatch):
    accepted, in_place = lockstep("bulk", 6, props, monkeypatch)
    print(f"bulk: {accepted} of 6 steps accepted, {in_place} patched in place")
    assert in_place >= 1


@pytest.mark.parametrize("props", PROPS, ids=IDS)
def test_every_neighbour_of_a_step_costs_what_the_oracle_says(props):
    data, slab = planted()
    K, seed, step = 128, 5, 777
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=seed, **props)
    sa.set_slab(P(slab))
    costs = sa.neighbours(step, want_diffs=False)[0]
    win = sa.debug_dump(binding.DUMP.WINDOWS).reshape(-1, 2)
    sa.close()
    got = [(1 if int(c) != binding.INVALID_COST else -1 if int(w) == WIN_DROPPED else 0, int(c)) for c, w in zip(costs, win[:, 1])]
    o = Oracle(data, dict_limit=0x400000, **props)
    oslab = np.array(slab).astype(literal_slab(1).dtype)
    want = [o.neighbour_ex(oslab, seed, step, j, K=K)[:2] for j in range(K)]
    want = [(st, c if st == 1 else binding.INVALID_COST) for st, c in want]
    assert got == want, [(j, g, w) for j, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    print(f"{sum(st == 1 for st, _ in want)} of {K} neighbours costed, {sum(st == -1 for st, _ in want)} dropped")
    assert sum(st == 1 for st, _ in want) >= K // 2
