"""The split form's fused launch (k_neighbours2<false, MGL_NBR_PICKWALK>: a neighbour's pick and its window walk in one
wavefront) against the two launches it replaces (MGL_NO_FUSE=1): the same two code bodies on the same inputs, so every
figure is bit for bit the same -- per-step stats, current and best cost, the whole slab with its stale entries, and the
per-neighbour outputs of the last step.  Shapes are the smallest at which each path can go wrong.  `-m gpu`."""
import numpy as np
import pytest

from megalania_amd import binding, corpus

pytestmark = pytest.mark.gpu

STAT_KEYS = ("evaluations", "failed", "accepted", "improved", "current_cost", "best_cost", "packets", "packets_evaluated",
             "fallback_neighbours", "second_pass_neighbours", "bulk_steps", "dropped_neighbours", "improving_neighbours")


def _pair(monkeypatch, data, env=(), **kw):
    """(fused chain, two-launch chain) from the same seed.  The launch switches are read at create.  MGL_NO_ADAPT keeps both
    on the split form for every step, so that the launch under test is the one that runs."""
    for k in ("MGL_NO_SPLIT", "MGL_NO_FUSE", "MGL_NO_CONT", "MGL_HALVES", "MGL_PICK_WAVES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MGL_NO_ADAPT", "1")
    for k, v in env:
        monkeypatch.setenv(k, v)
    fused = binding.SA(data, **kw)
    monkeypatch.setenv("MGL_NO_FUSE", "1")
    split = binding.SA(data, **kw)
    monkeypatch.delenv("MGL_NO_FUSE")
    return fused, split


def _steps(fused, split, steps, what):
    """`steps` steps one at a time on both chains; returns the summed stats of the fused chain and of the other"""
    tot = [dict.fromkeys(STAT_KEYS, 0), dict.fromkeys(STAT_KEYS, 0)]
    for s in range(steps):
        a, b = fused.run(1), split.run(1)
        for k in STAT_KEYS:
            assert a[k] == b[k], (what, s, k, a[k], b[k])
        for t, st in zip(tot, (a, b)):
            for k in ("second_pass_neighbours", "fallback_neighbours", "evaluations"):
                t[k] += st[k]
    return tot


def _same_end(fused, split, what):
    (ca, cost_a), (cb, cost_b) = fused.current(), split.current()
    assert cost_a == cost_b, what
    assert (ca == cb).all(), what  # the whole slab: off-walk entries too
    (ba, bcost_a), (bb, bcost_b) = fused.best(), split.best()
    assert bcost_a == bcost_b and (ba == bb).all(), what
    # the last step's neighbours: cost, journal length, packets walked, window and soft window
    for sel in (binding.DUMP.COSTS, binding.DUMP.JOURNAL_LENS, binding.DUMP.WALKED, binding.DUMP.WINDOWS, binding.DUMP.SOFT_ENDS):
        x, y = fused.debug_dump(sel), split.debug_dump(sel)
        assert len(x) == len(y) and (x == y).all(), (what, sel, np.nonzero(x != y)[0][:8])


def _close(*chains):
    for c in chains:
        c.close()


def test_single_slice(monkeypatch):
    data = corpus.prose_like(64 << 10, 0xF5)
    fused, split = _pair(monkeypatch, data, neighbours_per_step=1024, seed=77, accept="single")
    fused.seed_greedy(); split.seed_greedy()
    _steps(fused, split, 40, "single")
    _same_end(fused, split, "single")
    fused.set_accept_mode("auto"); split.set_accept_mode("auto")
    _steps(fused, split, 8, "auto")
    _same_end(fused, split, "auto")
    _close(fused, split)


@pytest.mark.parametrize("halves,K", [(2, 2048), (3, 2050)], ids=["two_slices", "three_slices_K2050"])
def test_slices_above_1mib(monkeypatch, halves, K):
    """above 1 MiB: one wavefront per pick workgroup in the two-launch form, and j_base > 0 behind the first slice; K = 2 050
    is not divisible by three"""
    data = corpus.prose_like(1280 << 10, 0xF6)
    fused, split = _pair(monkeypatch, data, env=[("MGL_HALVES", str(halves))], neighbours_per_step=K, seed=78, accept="single")
    fused.seed_greedy(); split.seed_greedy()
    _steps(fused, split, 12, halves)
    _same_end(fused, split, halves)
    _close(fused, split)


@pytest.mark.parametrize("variant", ["small_lists", "no_continuations"])
def test_hand_over_to_second_pass(monkeypatch, variant):
    """c1's shape.  small_lists: the first-pass lists hold 32 events, so many walks overflow and the second pass restarts them
    from `pickrec`, which the fused launch still writes.  no_continuations: a repair pick restarts the neighbour instead of
    resuming its walk."""
    data = corpus.lorem(4096)
    env = [("MGL_NO_CONT", "1")] if variant == "no_continuations" else []
    fused, split = _pair(monkeypatch, data, env=env, neighbours_per_step=1024, seed=79, accept="single")
    if variant == "small_lists":
        fused.debug_set(binding.KEY.LIST_CAP, 32); split.debug_set(binding.KEY.LIST_CAP, 32)
    tot = _steps(fused, split, 12, variant)
    for t in tot:
        assert t["second_pass_neighbours"] > 0 and t["fallback_neighbours"] == 0, (variant, t)
    _same_end(fused, split, variant)
    _close(fused, split)


@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_edges_of_the_input(monkeypatch, n):
    """targets at byte 0 or n - 1: top-K returns before it looks, and `pos + 1 < n` fails"""
    data = corpus.lorem(4096)[:n]
    fused, split = _pair(monkeypatch, data, neighbours_per_step=64, seed=80, accept="single")
    _steps(fused, split, 5, n)
    _same_end(fused, split, n)
    _close(fused, split)


def test_larger_model(monkeypatch):
    """lc = 3: the model is 12 KiB larger, and the fused launch's LDS is sized from it"""
    data = corpus.prose_like(64 << 10, 0xF5)
    fused, split = _pair(monkeypatch, data, neighbours_per_step=1024, seed=81, accept="single", lc=3, lp=0, pb=2)
    fused.seed_greedy(); split.seed_greedy()
    _steps(fused, split, 10, "lc3")
    _same_end(fused, split, "lc3")
    _close(fused, split)
