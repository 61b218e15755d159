"""Live target weights (mgl_sa_set_live_weights, mgl_sa_live_weights; the refresh inside mgl_sa_run): the trajectory of a
handle with live weights is the trajectory of a handle whose caller sets the weights by hand (weight_targets_by_cost)
before every step the rule names -- every multiple of `every` on the handle's global step count, and the first step behind
a slab replaced from outside --, however the run is cut; MGL_LW_SINGLE_ONLY keeps bulk-route steps out of it; the focus
window, the refusals, what turns what off, the full-walk engine.  `-m gpu`."""
import ctypes as C

import numpy as np
import pytest

import _validity
from _focus_chain import K
from _libs import PACKET
from megalania_amd import binding, corpus

pytestmark = pytest.mark.gpu

MGL_EINVAL = -1
SEED = 20261
_BASE = corpus.enwik_like(6000, 0x71)
DATA = _BASE + _BASE[1000:3277]  # tests/test_gpu_focus.py's: 8 277 bytes, not a multiple of 64
N = len(DATA)
STEPS = 48


def P(slab):
    return np.ascontiguousarray(slab).astype(PACKET)


def same(a, b):
    return bool((P(a) == P(b)).all())


def handle(accept="single", greedy=True, **kw):
    sa = binding.SA(DATA, accept=accept, neighbours_per_step=K, seed=SEED, **kw)
    if greedy:
        sa.seed_greedy(8)
    return sa


def add(total, st):
    """the counters of several runs, summed; the costs are the last run's"""
    out = dict(total) if total else {k: 0 for k in st}
    for k, v in st.items():
        if k.startswith("gpu_ms") or k in ("neighbour_launches", "sim_launches"):
            out[k] = 0
        elif k in ("current_cost", "best_cost", "packets"):
            out[k] = v
        else:
            out[k] += v
    return out


def floor_of(sa, floor):
    return sa.cost_map()[1]["total"] // N if floor == "mean" else floor


def by_hand(sa, g0, steps, every, floor, stale=False):
    """`steps` steps from global step g0 with the weights set by hand wherever the rule refreshes; returns (stats, refreshes)"""
    g, end, total, refreshes = g0, g0 + steps, None, 0
    while g < end:
        if g % every == 0 or stale:
            sa.weight_targets_by_cost(floor_of(sa, floor))
            refreshes += 1
            stale = False
        nxt = min(end, (g // every + 1) * every)
        total = add(total, sa.run(nxt - g))
        g = nxt
    return total, refreshes


def assert_same_state(a, b, what):
    (ca, cca), (cb, ccb) = a.current(), b.current()
    (ba, bca), (bb, bcb) = a.best(), b.best()
    assert cca == ccb and bca == bcb, (what, cca, ccb, bca, bcb)
    assert same(ca, cb) and same(ba, bb), what


def assert_valid_best(sa, what):
    best, cost = sa.best()
    assert _validity.violations(DATA, best, 0x400000) == [], what
    assert sa.cost_slab(best, want_cum=False)["total"] == cost, what


def live_cfg(floor):
    return dict(floor=0, floor_mean=True) if floor == "mean" else dict(floor=floor)


@pytest.mark.parametrize("floor", [0, 7, "mean"])
@pytest.mark.parametrize("every", [1, 5, 16])
def test_live_equals_by_hand(every, floor):
    a, b = handle(), handle()
    try:
        a.set_live_weights(every, **live_cfg(floor))
        sa_stats = add(None, a.run(STEPS))
        sb_stats, refreshes = by_hand(b, 0, STEPS, every, floor)
        assert_same_state(a, b, (every, floor))
        assert sa_stats == sb_stats, (every, floor, sa_stats, sb_stats)
        wa, wb = a.target_weights(), b.target_weights()
        assert (wa[0] == wb[0]).all() and wa[1:] == wb[1:] and wa[1] > 0
        lw = a.live_weights()
        assert lw["refreshes"] == refreshes == -(-STEPS // every) and lw["skipped"] == 0 and lw["gpu_ms"] > 0
        assert lw["every"] == every and lw["floor_mean"] == (floor == "mean") and lw["floor"] == (0 if floor == "mean" else floor)
        assert lw["last_gstep"] == (STEPS - 1) // every * every
        assert_valid_best(a, (every, floor))
    finally:
        a.close()
        b.close()


def test_cuts():
    """48 steps as one run, as 16 + 32 and as 48 runs of one: the same slabs"""
    hs = [handle() for _ in range(3)]
    try:
        for h in hs:
            h.set_live_weights(5, floor=3)
        hs[0].run(48)
        hs[1].run(16), hs[1].run(32)
        for _ in range(48):
            hs[2].run(1)
        for h in hs[1:]:
            assert_same_state(hs[0], h, "cuts")
            assert h.live_weights()["refreshes"] == hs[0].live_weights()["refreshes"] == 10
            assert (h.target_weights()[0] == hs[0].target_weights()[0]).all()
    finally:
        for h in hs:
            h.close()


def test_a_slab_from_outside_refreshes_before_the_next_step():
    a, b = handle(), handle()
    try:
        a.set_live_weights(16)
        a.run(19)
        by_hand(b, 0, 19, 16, 0)
        assert_same_state(a, b, "before")
        other = handle()
        other.seed_greedy(64)
        other.run(5)
        slab = other.current()[0]
        other.close()
        a.set_slab(slab), b.set_slab(slab)
        assert a.live_weights()["refreshes"] == 2
        a.run(20)  # steps 19 .. 38: stale at 19, due at 32
        by_hand(b, 19, 20, 16, 0, stale=True)
        assert_same_state(a, b, "after")
        lw = a.live_weights()
        assert lw["refreshes"] == 4 and lw["last_gstep"] == 32
        # the stale refresh changed the trajectory: a handle that only refreshes when due goes another way
        c = handle()
        by_hand(c, 0, 19, 16, 0)
        c.set_slab(slab)
        by_hand(c, 19, 20, 16, 0, stale=False)
        assert not same(c.current()[0], a.current()[0])
        c.close()
        assert_valid_best(a, "stale")
    finally:
        a.close()
        b.close()


def run_plain(accept, steps, greedy, live=None):
    sa = handle(accept, greedy)
    if live:
        sa.set_live_weights(**live)
    st = sa.run(steps)
    return sa, st


def test_single_only_under_bulk_and_single():
    plain, _ = run_plain("bulk", 12, True)
    flagged, _ = run_plain("bulk", 12, True, dict(every=5, single_only=True))
    try:
        assert_same_state(plain, flagged, "bulk")
        lw = flagged.live_weights()
        assert lw["refreshes"] == 0 and lw["single_only"] and flagged.target_weights()[1] == 0
        assert_valid_best(flagged, "bulk")
    finally:
        plain.close()
        flagged.close()
    without, _ = run_plain("single", 24, True, dict(every=5))
    with_, _ = run_plain("single", 24, True, dict(every=5, single_only=True))
    bare, _ = run_plain("single", 24, True)
    try:
        assert_same_state(without, with_, "single")
        assert with_.live_weights()["refreshes"] == without.live_weights()["refreshes"] == 5
        assert not same(bare.current()[0], with_.current()[0]), "the weights changed nothing: the test shows nothing"
    finally:
        for h in (without, with_, bare):
            h.close()


def test_single_only_under_auto():
    """from the all-literal slab AUTO opens with a block of bulk steps: those pass as without weights, and the refreshes are
    the single steps that are due or the first single step behind a due bulk step (step 0, where live weights were enabled, is
    due).  A bulk threshold of K improving neighbours per step is never met on this input, so AUTO's counters send it to
    single steps behind the first block, inside the 64 steps."""
    every = 5
    auto = dict(accept="auto", bulk_threshold=K, neighbours_per_step=K, seed=SEED)
    a = binding.SA(DATA, **auto)
    plain = binding.SA(DATA, **auto)
    try:
        a.set_live_weights(every, single_only=True)
        a.run(64)
        modes = a.step_modes().tolist()
        assert len(modes) == 64 and modes[0] == 1 and 0 in modes, modes
        want, pending = 0, False
        for g, m in enumerate(modes):
            pending = pending or g % every == 0
            if m == 0 and pending:
                want, pending = want + 1, False
        assert a.live_weights()["refreshes"] == want >= 2, (want, modes)
        first_single = modes.index(0)
        b = binding.SA(DATA, **auto)
        b.set_live_weights(every, single_only=True)
        b.run(first_single)
        plain.run(first_single)
        assert plain.step_modes().tolist() == modes[:first_single]
        assert_same_state(b, plain, "the first bulk block")
        assert b.live_weights()["refreshes"] == 0
        b.run(64 - first_single)
        assert_same_state(a, b, "cut at the first single step")
        b.close()
        assert_valid_best(a, "auto")
    finally:
        a.close()
        plain.close()


def test_focus_window():
    lo, hi = 3000, 5500
    a, b = handle(), handle()
    try:
        before = a.current()[0]
        for h in (a, b):
            h.set_focus(lo, hi)
        a.set_live_weights(5, floor=2)
        a.run(30)
        by_hand(b, 0, 30, 5, 2)
        assert_same_state(a, b, "focus")
        cur, best = a.current()[0], a.best()[0]
        assert same(cur[:lo], before[:lo]) and same(best[:lo], before[:lo])
        assert not same(cur, before)
        wa, wb = a.target_weights(), b.target_weights()
        assert (wa[0] == wb[0]).all() and wa[1:] == wb[1:] and 0 < wa[2] < wa[1]
        assert_valid_best(a, "focus")
    finally:
        a.close()
        b.close()


def _raw_set(sa, every, floor=0, floor_mean=0, flags=0):
    cfg = binding.LiveWeightsConfig(every, floor, floor_mean, flags)
    return sa.L.mgl_sa_set_live_weights(sa.h, C.byref(cfg))


def test_refusals_and_what_turns_what_off():
    sa = handle()
    big = binding.SA(corpus.lorem(1 << 12) * 8, accept="single", neighbours_per_step=K, seed=SEED)  # 32 KiB: floor * n reaches 2^43 below 2^32
    pos = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, flags=binding.F_POSITION_TARGETS)
    try:
        sa.set_live_weights(5, floor=9)
        sa.run(7)
        state = sa.live_weights(), sa.target_weights()
        assert state[0]["refreshes"] == 2
        for args in [dict(every=0), dict(every=3, floor=(1 << 32) - (1 << 20)), dict(every=3, flags=2), dict(every=3, flags=0x80000001)]:
            assert _raw_set(sa, **args) == MGL_EINVAL, args
            now = sa.live_weights(), sa.target_weights()
            assert now[0] == state[0] and (now[1][0] == state[1][0]).all() and now[1][1:] == state[1][1:], args
        assert _raw_set(sa, 3, floor=(1 << 32) - 1 - (1 << 20)) == MGL_EINVAL  # fits an entry, but floor * n >= 2^43
        assert _raw_set(big, 3, floor=(1 << 43) // big.n + 1) == MGL_EINVAL and big.live_weights()["every"] == 0
        assert _raw_set(big, 3, floor=((1 << 43) - 1) // big.n) == 0 and big.live_weights()["every"] == 3
        assert _raw_set(pos, 3) == MGL_EINVAL and pos.live_weights()["every"] == 0
        assert sa.L.mgl_sa_set_live_weights(None, None) == MGL_EINVAL and sa.L.mgl_sa_live_weights(None, None, None) == MGL_EINVAL
        # explicit weights turn live weights off ...
        sa.set_target_weights(np.ones(N, dtype=np.uint32))
        assert sa.live_weights()["every"] == 0 and sa.live_weights()["refreshes"] == 0 and sa.target_weights()[1] == N
        sa.set_live_weights(4)
        assert sa.target_weights()[1] == 0, "enabling live weights replaces explicit ones; none in force until the first refresh"
        sa.weight_targets_by_cost(1)
        assert sa.live_weights()["every"] == 0 and sa.target_weights()[1] > N
        # ... and enabling them replaces explicit ones; None clears everything
        sa.set_live_weights(4, floor_mean=True, single_only=True)
        lw = sa.live_weights()
        assert lw["every"] == 4 and lw["floor_mean"] and lw["single_only"] and lw["refreshes"] == 0
        sa.run(3)  # steps 7, 8, 9: stale at 7, due at 8
        assert sa.live_weights()["refreshes"] == 2 and sa.target_weights()[1] > 0
        sa.set_live_weights(None)
        assert sa.live_weights()["every"] == 0 and sa.target_weights()[1] == 0 and not sa.target_weights()[0].any()
        sa.run(2)
        assert_valid_best(sa, "after clearing")
    finally:
        for h in (sa, big, pos):
            h.close()


def test_full_walk_engine_goes_the_same_way():
    inc = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, serial_build=True, snapshots=False)
    full = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, fullwalk=True)
    try:
        for h in (inc, full):
            h.seed_greedy(8)
            h.set_live_weights(5, floor=1)
            h.run(12)
        assert_same_state(inc, full, "engines")
        assert (inc.target_weights()[0] == full.target_weights()[0]).all()
        assert inc.live_weights()["refreshes"] == full.live_weights()["refreshes"] == 3
        assert_valid_best(full, "fullwalk")
    finally:
        inc.close()
        full.close()
