"""The serial stretch of a single step, between the last neighbour kernel and the next step's pick: the split form without a
late second pass (the last resort queued in front of the join with the re-simulations), and the accept's tail behind it (the
lazy copy of the best slab's structures, the accept, the step's end) on every way through it.  Every comparison is against the
full-walk engine and exact: costs are integer sums.  `-m gpu`."""
import lzma

import numpy as np
import pytest

from megalania_amd import binding, corpus

pytestmark = pytest.mark.gpu



def rows(slab):
    return [tuple(int(x) for x in r) for r in zip(slab["type"], slab["dist"], slab["len"])]


def liblzma_parse(data):
    stream = lzma.compress(data, format=lzma.FORMAT_ALONE,
                           filters=[dict(id=lzma.FILTER_LZMA1, preset=6, dict_size=1 << 22, lc=0, lp=0, pb=0)])
    return binding.stream_import(stream, data)[0]


def allocated_list_cap(sa):
    """the largest first-pass list capacity key 2 takes: the allocated one (capacities are multiples of 8)"""
    cap = 8
    while sa.L.mgl_debug_set(sa.h, binding.KEY.LIST_CAP, cap + 8) == 0:
        cap += 8
    sa.debug_set(binding.KEY.LIST_CAP, cap)
    return cap


# ---- the split form without the late pass
_walks = {}


def _steps(sa, steps, start):
    if start is not None:
        sa.set_slab(start)
    costs, second, last = [], 0, 0
    for _ in range(steps):
        st = sa.run(1)  # raises on any error flag of the control block
        costs.append(st["current_cost"])
        second += st["second_pass_neighbours"]
        last += st["fallback_neighbours"]
    cur, cost = sa.current()
    return costs, cost, rows(cur), second, last


def _split_vs_fullwalk(name, data, K, steps, start, cap):
    """`steps` single steps of the split form with first-pass lists of `cap` events (0: the allocated capacity) against the
    same steps on the full-walk engine (computed once per input)"""
    if name not in _walks:
        ref = binding.SA(data, accept="single", neighbours_per_step=K, fullwalk=True)
        _walks[name] = _steps(ref, steps, start)[:3]
        ref.close()
    sa = binding.SA(data, accept="single", neighbours_per_step=K)
    set_to = allocated_list_cap(sa)
    if cap:
        sa.debug_set(binding.KEY.LIST_CAP, cap)
    costs, cost, slab, second, last = _steps(sa, steps, start)
    sa.close()
    print(f"{name} K={K} list capacity {cap or set_to}: second-pass neighbours {second} of {steps * K}, last-resort neighbours {last}, final cost {cost}")
    assert costs == _walks[name][0]
    assert (cost, slab) == _walks[name][1:]
    return second, last


@pytest.fixture
def split_form(monkeypatch):
    monkeypatch.setenv("MGL_NO_ADAPT", "1")  # the split form in every step
    monkeypatch.setenv("MGL_HALVES", "2")    # in two slices from 1 024 neighbours per step on


@pytest.mark.parametrize("cap", [0, 8], ids=["allocated", "8"])
def test_two_slices_without_late_pass(split_form, cap):
    """20 000 B of the c2-shaped text, 1 024 neighbours per step (the fewest that run in two slices), 12 single steps.  With
    the lists at their allocated capacity k_sim gets the longest lists, hence the most distinct contexts, it can be handed: its
    context list (twice a change list) must hold them, or the run ends with an error.  With lists of 8 events nearly every
    neighbour overflows into the second pass.
    The last resort behind it is NOT reached, here or in any shape a test can set up, so `fallback_neighbours > 0` is not
    asserted.  Two ways lead a second-pass neighbour onto its list.  One is finding no scratch slot: there are as many slots
    as neighbours per step, 512 at the least (slots = max(K, 512)), and the pass's list index is below K, so no
    neighbours_per_step reaches past them.  The other is the hand-over at the end of nbr2_one (`ch.overflow || too_many`): in
    the second pass a full list means the neighbour is dropped, not handed on, `too_many` cannot be raised because the pass's
    context list holds every context there is (uctx_cap = ckpt_elems), and what is left is the walk guard of 2^20 rounds.
    The commit before this one reads fallback_neighbours 0 for both capacities here as well.  What the test covers of the
    last resort is therefore its launch over an empty list, queued in front of the join with the re-simulations, in every
    step; that it is right with work on its list while k_sim still runs rests on reasoning (it writes the outputs of its own
    neighbours only, and k_sim costs none of them: their headers stay 0xFFFFFFFF), not on a run."""
    data, _ = corpus.config_input("c2", 20000)
    second, _ = _split_vs_fullwalk("c2 20000", data, 1024, 12, None, cap)
    if cap:
        assert second > 12 * 1024 // 2, second


@pytest.mark.parametrize("cap", [0, 8], ids=["allocated", "8"])
def test_one_slice_without_late_pass(split_form, cap):
    """c1 (4 096 B), 256 neighbours per step in one slice, from the parse liblzma makes of it (repair picks from the first
    step on: tests/test_gpu_second_pass_workgroup.py)"""
    data, _ = corpus.config_input("c1")
    second, _ = _split_vs_fullwalk("c1 liblzma", data, 256, 12, liblzma_parse(data), cap)
    assert second > (12 * 256 // 2 if cap else 0), second


# ---- the accept's tail: all three ways through the snapshot condition, and the step's end behind them
def _epochs(data, K, steps, per_epoch, fullwalk, start):
    """`steps` single steps in epochs of `per_epoch` steps; every epoch but the first starts from the best slab (phase 1).
    Per step: (current cost, best cost, moves, new bests)."""
    sa = binding.SA(data, accept="single", neighbours_per_step=K, iters_per_epoch=per_epoch * K, fullwalk=fullwalk)
    if start is not None:
        sa.set_slab(start)
    out, restarts = [], 0
    for s in range(steps):
        if s and s % per_epoch == 0:
            sa.begin_epoch(1, from_best=True)
            restarts += 1
        st = sa.run(1)
        out.append((st["current_cost"], st["best_cost"], st["accepted"], st["improved"]))
        if not fullwalk:
            counts = sa.debug_dump(binding.DUMP.STEP_COUNTS)
            last, live = counts[0], counts[1:]
            # the dump: the finished step's counters (`unused4` has no user and stays zero), then the live ones of the device's
            # counter block, which the step's end must have cleared
            assert len(counts) == 2 and last["unused4"] == 0 and not live.view(np.uint32).any(), (s, counts)
    cur, cur_cost = sa.current()
    bst, best_cost = sa.best()
    sa.close()
    assert restarts >= 1
    return out, (cur_cost, rows(cur)), (best_cost, rows(bst))


def step_kinds(trace):
    """steps that took no move / set a new best / moved the base off the best slab it held (only then is a copy due): the three
    ways through the lazy snapshot's condition.  "Held the best slab" is inferred from the costs (current == best after the
    previous step), not read from the device: a move of equal cost would leave the best slab unnoticed and a later uphill move
    be counted here although no copy was due.  The counts say that the run was of the intended kind; what holds the device
    to the right behaviour on each branch is the comparison with the full-walk engine, step by step."""
    nothing = sum(1 for t in trace if t[2] == 0)
    new_best = sum(1 for t in trace if t[3])
    at_best = [True] + [t[0] == t[1] for t in trace[:-1]]  # (a restart from the best slab keeps it so)
    left_best = sum(1 for t, ab in zip(trace, at_best) if ab and t[2] and not t[3])
    return nothing, new_best, left_best


@pytest.mark.parametrize("K", [8, 256])
@pytest.mark.parametrize("name", ["lorem600", "c1"])
def test_folded_tail(name, K):
    """60 single steps in epochs of 12 (four restarts from the best slab), from the parse liblzma makes of the input: little is
    left to improve there, so steps take nothing, now and then a new best, and -- early in an epoch, where the transition draw
    is generous -- a move uphill, away from the best slab."""
    data = corpus.lorem(600) if name == "lorem600" else corpus.config_input("c1")[0]
    start = liblzma_parse(data)
    got = _epochs(data, K, 60, 12, False, start)
    want = _epochs(data, K, 60, 12, True, start)
    kinds = step_kinds(got[0])
    print(f"{name} K={K}: steps without a move {kinds[0]}, with a new best {kinds[1]}, off the best slab {kinds[2]}")
    assert got[0] == want[0]
    assert got[1] == want[1] and got[2] == want[2]
    assert all(kinds), kinds
