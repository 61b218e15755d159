"""Target weights on the device (mgl_sa_set_target_weights, mgl_sa_weight_targets_by_cost, mgl_sa_target_weights; csrc/mgl_weights.hip):
a step's targets against the Python restatement of the rule (tests/_weighted_targets.py) entry for entry, with and without a
focus window, on both engines; costs against the CPU oracle; runs; the weights made of the cost map on the device; refusals.
The data, the greedy slab and the window list are those of tests/test_gpu_focus.py.  `-m gpu`."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_focus as tf
from _libs import Oracle, walk
from _validity import violations
from _weighted_targets import ordinal_targets, targets
from megalania_amd import binding, corpus

pytestmark = pytest.mark.gpu

MGL_EINVAL, MGL_ENOMEM = -1, -2
DATA, N, K, SEED = tf.DATA, tf.N, tf.K, tf.SEED
P, same, journal, targets_of, greedy_slab = tf.P, tf.same, tf.journal, tf.targets_of, tf.greedy_slab
FULL = 0xFFFFFFFF


def u32(n, fill=0):
    return np.full(n, fill, dtype=np.uint32)


def rand_weights(n, seed, top=1 << 20):
    return np.random.default_rng(seed).integers(0, top, size=n, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def greedy_cost_map():
    """the cost map of the greedy slab, and its report's total"""
    sa = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED)
    try:
        sa.set_slab(greedy_slab()[0])
        m, rep = sa.cost_map()
        return m, rep["total"]
    finally:
        sa.close()


def long_match(slab, starts):
    """the start of a packet of 273 bytes"""
    at = [int(s) for s in starts if int(slab["len"][s]) == 273]
    assert at
    return at[0]


def check(sa, w, starts, window, step, K_, met=None, set_weights=True):
    if set_weights:
        sa.set_target_weights(w)
    sa.neighbours(step, want_diffs=False)
    want = targets(sa.L, w, starts, window, SEED, step, K_, info=met)
    got = targets_of(sa)
    assert got == want, (window, step, [(j, g, t) for j, (g, t) in enumerate(zip(got, want)) if g != t][:5])
    back, total, wsum = sa.target_weights()
    lo, hi = window if window else (0, len(w))
    assert (back == w).all() and total == int(w.astype(np.uint64).sum()) and wsum == int(w[lo:hi].astype(np.uint64).sum())
    return got


# ---- 1. the target rule
def weight_patterns(slab, starts):
    at = long_match(slab, starts)
    pats = [("ones", u32(N, 1))]
    for x in (0, 63, 64, 65, 4095, 4096, 4097, N - 1, at + 200, at + 272):
        w = u32(N)
        w[x] = 5
        pats.append(("byte%d" % x, w))
    w = u32(N, 1)
    w[128:192] = 0    # a whole cell
    w[4096:8192] = 0  # a whole block of the prefix sums
    pats.append(("zero cell and block", w))
    w = u32(N)
    w[[7, 100, 1000, 4000, 4096, 5000, 6000, 7000, 8191, N - 2]] = 1  # fewer weighted bytes than K: empty slices, shared targets
    pats.append(("ten bytes", w))
    pats.append(("random", rand_weights(N, 1)))
    w = u32(N)
    w[np.random.default_rng(2).permutation(N)[:4095]] = FULL  # the sum just below 2^44
    pats.append(("4095 full", w))
    pats.append(("cost map", greedy_cost_map()[0]))
    return pats


@pytest.mark.parametrize("K_", [K, 1], ids=["K64", "K1"])
def test_targets_equal_the_rule(K_):
    slab, _ = greedy_slab()
    starts = np.array(walk(slab))
    met = {}
    sa = binding.SA(DATA, accept="single", neighbours_per_step=K_, seed=SEED)
    try:
        sa.set_slab(slab)
        assert sa.target_weights()[1:] == (0, 0) and not sa.target_weights()[0].any()
        for i, (name, w) in enumerate(weight_patterns(slab, starts)):
            got = check(sa, w, starts, None, 3 + i, K_, met)
            assert all(t in set(starts.tolist()) for t in got), name
            if name.startswith("byte"):  # one weighted byte: every neighbour takes the packet that covers it
                x = int(name[4:])
                assert got == [int(starts[np.searchsorted(starts, x, side="right") - 1])] * K_, name
            if name == "ten bytes" and K_ > 1:
                assert len(set(got)) < len(got)
        assert met["earlier_word"] and (met["empty_slice"] or K_ == 1) and (met["wide_slice"] or K_ > 1)
        at = long_match(slab, starts)
        assert (at >> 6) + 3 <= (at + 200) >> 6  # the covering start lies at least three bitmap words back
        # cleared: the rule without weights
        sa.set_target_weights(None)
        sa.neighbours(99, want_diffs=False)
        assert targets_of(sa) == ordinal_targets(sa.L, starts, 0, N, SEED, 99, K_) and sa.target_weights()[1:] == (0, 0)
    finally:
        sa.close()


def test_a_wide_slice_was_met_at_k64():
    """K = 64 and the sum just below 2^44: every slice is about 2^38 wide, far above one 31-bit draw"""
    slab, _ = greedy_slab()
    starts = np.array(walk(slab))
    met = {}
    sa = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED)
    try:
        sa.set_slab(slab)
        w = u32(N)
        w[:4095] = FULL
        check(sa, w, starts, None, 1, K, met)
        assert met["wide_slice"]
    finally:
        sa.close()


# the scan's levels: 64 positions per cell, 64 cells per block, 64 blocks per turn of the last kernel.  131 149 = 2 * 65 536 + 77;
# 262 209 = 64 blocks + 65 positions: 65 blocks, the last of two cells, the second of one position
@pytest.mark.parametrize("n", [131149, 262209, 262144 - 1], ids=["131149", "262209", "262143"])
def test_larger_inputs(n):
    data = corpus.enwik_like(n, 0x72)
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=SEED)
    try:
        sa.seed_greedy(8)
        starts = np.array(walk(P(sa.current()[0])))
        check(sa, rand_weights(n, n), starts, None, 5, K)
        w = u32(n)
        w[[x for x in (n - 1, n - 64, n - 65, 4096 * 64 - 1, 4096 * 64, 4096 * 32 - 1, 4096 * 32) if x < n]] = 3  # the last position and cells, block edges
        check(sa, w, starts, None, 6, K)
        w = u32(n, FULL >> 14)  # 2^18 per byte: prefix sums above 2^32 from 16 384 positions on
        sa.set_target_weights(w)
        sa.set_focus(n // 3, n - 5)
        check(sa, w, starts, (n // 3, n - 5), 7, K, set_weights=False)
    finally:
        sa.close()


# ---- 2. with a focus window
@pytest.mark.parametrize("K_", [K, 1], ids=["K64", "K1"])
def test_windows_and_weights(K_):
    slab, _ = greedy_slab()
    starts, wins = tf.rule_windows(slab)
    met = {}
    sa = binding.SA(DATA, accept="single", neighbours_per_step=K_, seed=SEED)
    try:
        sa.set_slab(slab)
        for wi, w in enumerate((rand_weights(N, 3), greedy_cost_map()[0])):
            sa.set_target_weights(w)
            for i, (lo, hi) in enumerate(wins):
                sa.set_focus(lo, hi)
                got = check(sa, w, starts, (lo, hi), 10 * wi + i, K_, met, set_weights=False)
                inside = [int(s) for s in starts if lo <= s < hi]
                cover = int(starts[np.searchsorted(starts, lo, side="right") - 1])
                assert all(t in inside for t in got) if inside else got == [cover] * K_, (lo, hi)
                assert sa.focus()[:2] == (lo, hi)
        assert met["below_lo"]
    finally:
        sa.close()


def test_window_edges():
    slab, _ = greedy_slab()
    starts = np.array(walk(slab))
    at = long_match(slab, starts)
    nxt = int(starts[np.searchsorted(starts, at, side="right")])
    assert nxt == at + 273
    sa = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED)
    try:
        sa.set_slab(slab)
        # weight only in front of the window's first start: the covering packet starts below lo, the first start inside is taken
        lo, hi = at + 100, nxt + 40
        w = u32(N)
        w[lo:nxt] = 9
        sa.set_focus(lo, hi)
        assert check(sa, w, starts, (lo, hi), 1, K) == [nxt] * K
        # a window inside one long match: it holds no start, the packet that covers lo is the target
        lo, hi = at + 2, at + 5
        sa.set_focus(lo, hi)
        assert check(sa, u32(N, 1), starts, (lo, hi), 2, K) == [at] * K
        lo, hi = at + 70, at + 272  # ... across three bitmap words
        sa.set_focus(lo, hi)
        assert check(sa, rand_weights(N, 4), starts, (lo, hi), 3, K) == [at] * K
        # zero inside the window, weight outside: the plain focus rule
        lo, hi = tf.MIDDLE
        w = u32(N, 7)
        w[lo:hi] = 0
        sa.set_focus(lo, hi)
        got = check(sa, w, starts, (lo, hi), 4, K)
        assert got == tf.target_rule(sa, starts, lo, hi, SEED, 4, K)[0] and sa.target_weights()[2] == 0
        # the order of the two calls does not matter
        w = rand_weights(N, 5)
        sa.set_focus(0, 0)
        sa.set_target_weights(w)
        sa.set_focus(lo, hi)
        first = check(sa, w, starts, (lo, hi), 5, K, set_weights=False)
        sa.set_target_weights(None)
        sa.set_focus(0, 0)
        sa.set_focus(lo, hi)
        assert check(sa, w, starts, (lo, hi), 5, K) == first and sa.focus()[:2] == (lo, hi)
        # clearing the window under weights: the whole file weighs again
        sa.set_focus(0, 0)
        check(sa, w, starts, None, 6, K, set_weights=False)
    finally:
        sa.close()


# ---- 3. costing is untouched
def test_costs_equal_the_oracle_on_both_engines():
    slab, _ = greedy_slab()
    o = Oracle(DATA, dict_limit=0x400000)
    starts = np.array(walk(slab))
    w = greedy_cost_map()[0]
    got = {}
    for fullwalk in (False, True):
        sa = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, fullwalk=fullwalk)
        try:
            sa.set_slab(slab)
            sa.set_target_weights(w)
            for step in (5, 6):
                costs, nd, diffs = sa.neighbours(step)
                assert targets_of(sa) == targets(sa.L, w, starts, None, SEED, step, K), (fullwalk, step)
                got[fullwalk, step] = ([int(c) for c in costs], [journal(diffs, nd, j) for j in range(K)],
                                       sa.debug_dump(binding.DUMP.WINDOWS).tolist())
        finally:
            sa.close()
    for step in (5, 6):
        assert got[False, step] == got[True, step], step
        costs, journals, _ = got[False, step]
        ok = [j for j in range(K) if costs[j] != binding.INVALID_COST]
        assert len(ok) >= K // 2
        for j in ok:
            copy = slab.copy()
            for p, old, new in journals[j]:
                assert tf.as_list([copy[p]])[0] == old
                copy[p] = new
            assert o.cost_slab(copy)["total"] == costs[j], (step, j)


# ---- 4. runs
def test_runs_agree_on_both_engines():
    slab, _ = greedy_slab()
    o = Oracle(DATA, dict_limit=0x400000)
    out = []
    for fullwalk in (False, True):
        sa = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, iters_per_epoch=N, fullwalk=fullwalk)
        try:
            sa.set_slab(slab)
            sa.weight_targets_by_cost(floor=greedy_cost_map()[1] // N)
            st = sa.run(30)
            cur, cur_cost = sa.current()
            bst, best_cost = sa.best()
            assert st["steps"] == 30 and st["accepted"] > 0 and st["current_cost"] == cur_cost == o.cost_slab(P(cur))["total"]
            assert best_cost == o.cost_slab(P(bst))["total"]
            assert violations(DATA, P(cur), 0x400000) == [] and violations(DATA, P(bst), 0x400000) == []
            assert sa.target_weights()[1] == greedy_cost_map()[1] + (greedy_cost_map()[1] // N) * N  # still set behind the run
            out.append((cur_cost, best_cost, st["accepted"], st["evaluations"], st["failed"], P(cur), P(bst), targets_of(sa)))
        finally:
            sa.close()
    a, b = out
    assert a[:5] == b[:5] and same(a[5], b[5]) and same(a[6], b[6]) and a[7] == b[7]
    assert not same(a[5], slab)


@pytest.mark.parametrize("mode", ["single", "bulk", "auto"])
def test_runs_leave_everything_below_the_weighted_stretch(mode):
    begin, _ = greedy_slab()
    lo, hi = tf.MIDDLE
    starts = np.array(walk(begin))
    cover = int(starts[np.searchsorted(starts, lo, side="right") - 1])
    w = u32(N)
    w[lo:hi] = rand_weights(hi - lo, 6) + 1
    sa = binding.SA(DATA, accept=mode, neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    try:
        sa.set_slab(begin)
        sa.set_target_weights(w)
        st = sa.run(40)
        assert st["steps"] == 40 and st["accepted"] > 0
        cur, cur_cost = sa.current()
        bst, _ = sa.best()
        for what, slab in (("current", cur), ("best", bst)):
            assert same(slab[:cover], begin[:cover]), (what, np.nonzero(P(slab)[:cover] != begin[:cover])[0][:5])
            assert violations(DATA, P(slab), 0x400000) == [], what
        assert not same(cur, begin) and cur_cost == sa.cost_slab(P(cur), want_cum=False)["total"]
    finally:
        sa.close()


def test_set_then_clear_changes_nothing():
    slab, _ = greedy_slab()
    made = []
    try:
        for how in ("untouched", "set-then-cleared", "set-by-cost-then-cleared"):
            sa = binding.SA(DATA, accept="auto", neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
            made.append(sa)
            sa.set_slab(slab)
            before = sa.debug_dump(binding.DUMP.ALLOCATIONS).tolist()
            if how == "set-then-cleared":
                sa.set_target_weights(rand_weights(N, 8))
            if how == "set-by-cost-then-cleared":
                sa.weight_targets_by_cost(floor=3)
            if how != "untouched":
                held = sa.debug_dump(binding.DUMP.ALLOCATIONS).tolist()
                assert held[0] == before[0] + 3 and 4 * N + N // 8 <= held[1] - before[1] <= 4 * N + N // 8 + 256
                sa.set_target_weights(rand_weights(N, 9))  # replaced: the same buffers
                assert sa.debug_dump(binding.DUMP.ALLOCATIONS).tolist() == held
                sa.set_target_weights(None)
                assert sa.target_weights()[1:] == (0, 0)
            assert sa.debug_dump(binding.DUMP.ALLOCATIONS).tolist() == before
        runs = []
        for sa in made:
            st = sa.run(10)
            runs.append(((st["current_cost"], st["best_cost"], st["accepted"], st["evaluations"], st["failed"]), sa.step_modes().tolist(),
                         P(sa.current()[0]), P(sa.best()[0]), targets_of(sa)))
        for r in runs[1:]:
            assert r[0] == runs[0][0] and r[1] == runs[0][1] and same(r[2], runs[0][2]) and same(r[3], runs[0][3]) and r[4] == runs[0][4]
    finally:
        for sa in made:
            sa.close()


def test_weights_stay_across_epochs_slabs_and_seeds():
    w = rand_weights(N, 10)
    sa = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    try:
        sa.set_target_weights(w)
        sa.run(2)
        for change in (lambda: sa.begin_epoch(0), lambda: sa.seed_greedy(8), lambda: sa.set_slab(greedy_slab()[0]), lambda: sa.run(2),
                       lambda: sa.begin_epoch(1, from_best=True)):
            change()
            starts = np.array(walk(P(sa.current()[0])))
            check(sa, w, starts, None, 1000, K, set_weights=False)
    finally:
        sa.close()


def test_targets_follow_the_walk_inside_a_run():
    """several steps in one call: each step's targets, those made ahead beside the accept included, are the rule's on the slab
    that step began from"""
    slab, _ = greedy_slab()
    w = greedy_cost_map()[0]
    a = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    b = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    try:
        for h in (a, b):
            h.set_slab(slab)
            h.set_target_weights(w)
        a.run(6)
        for s in range(6):
            before = P(b.current()[0])
            b.run(1)
            assert targets_of(b) == targets(b.L, w, np.array(walk(before)), None, SEED, s, K), s
        assert targets_of(a) == targets_of(b) and same(a.current()[0], b.current()[0]) and a.current()[1] == b.current()[1]
    finally:
        a.close()
        b.close()


# ---- 5. weights of the cost map
@pytest.mark.parametrize("props", [(0, 0, 0), (3, 0, 2)], ids=["000", "302"])
def test_weight_targets_by_cost(props):
    slab, _ = greedy_slab()
    sa = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, lc=props[0], lp=props[1], pb=props[2])
    try:
        sa.set_slab(slab)
        m, rep = sa.cost_map()
        assert int(m.astype(np.uint64).sum()) == rep["total"]
        for floor in (0, 1, rep["total"] // N):
            total, ms = sa.weight_targets_by_cost(floor=floor)
            back, s_n, window = sa.target_weights()
            assert (back == m + np.uint32(floor)).all() and total == s_n == window == rep["total"] + floor * N and ms > 0, floor
        # an explicit slab, another one than the current
        lit = binding.literal_slab(N)
        m2, rep2 = sa.cost_map(lit)
        total, _ = sa.weight_targets_by_cost(floor=2, slab=lit)
        assert (sa.target_weights()[0] == m2 + np.uint32(2)).all() and total == rep2["total"] + 2 * N
        starts = np.array(walk(slab))
        check(sa, m2 + np.uint32(2), starts, None, 4, K, set_weights=False)
        held = sa.target_weights()
        # a slab that mgl_cost_slab refuses: the same code, the weights in force stay
        bad = slab.copy()
        bad[int(starts[5])] = (0, 0, 0)
        with pytest.raises(binding.MglError) as want:
            sa.cost_slab(bad, want_cum=False)
        with pytest.raises(binding.MglError) as e:
            sa.weight_targets_by_cost(floor=1, slab=bad)
        assert e.value.rc == want.value.rc != 0
        # a floor that could carry, and no room for the map's own buffers
        assert sa.L.mgl_sa_weight_targets_by_cost(sa.h, None, FULL - (1 << 20) + 1, None, None) == MGL_EINVAL
        sa.debug_set(binding.KEY.COSTMAP_NOMEM, 1)
        assert sa.L.mgl_sa_weight_targets_by_cost(sa.h, None, 1, None, None) == MGL_ENOMEM
        now = sa.target_weights()
        assert (now[0] == held[0]).all() and now[1:] == held[1:]
        check(sa, held[0], starts, None, 5, K, set_weights=False)
    finally:
        sa.close()


# ---- 6. refusals
def test_refusals():
    slab, _ = greedy_slab()
    starts = np.array(walk(slab))
    sa = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED)
    pos = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, flags=binding.F_POSITION_TARGETS)
    try:
        sa.set_slab(slab)
        w = rand_weights(N, 11)
        sa.set_target_weights(w)
        full = u32(N, FULL)  # the sum reaches 2^44
        assert sa.L.mgl_sa_set_target_weights(sa.h, full.ctypes.data_as(C.c_void_p)) == MGL_EINVAL
        with pytest.raises(binding.MglError) as e:
            sa.set_target_weights(full)
        assert e.value.rc == MGL_EINVAL
        edge = u32(N)
        edge[:4096] = FULL
        edge[4096] = 4096  # exactly 2^44
        assert sa.L.mgl_sa_set_target_weights(sa.h, edge.ctypes.data_as(C.c_void_p)) == MGL_EINVAL
        check(sa, w, starts, None, 1, K, set_weights=False)  # the previous weights are in force
        edge[4096] = 4095  # 2^44 - 1
        check(sa, edge, starts, None, 2, K)
        with pytest.raises(binding.MglError):
            sa.set_target_weights(w[:-1])
        # position draws have no targets kernel
        for call in (lambda: pos.L.mgl_sa_set_target_weights(pos.h, w.ctypes.data_as(C.c_void_p)), lambda: pos.L.mgl_sa_set_target_weights(pos.h, None),
                     lambda: pos.L.mgl_sa_weight_targets_by_cost(pos.h, None, 0, None, None)):
            assert call() == MGL_EINVAL
        assert pos.target_weights()[1:] == (0, 0) and pos.run(2)["steps"] == 2
        assert sa.L.mgl_sa_set_target_weights(None, w.ctypes.data_as(C.c_void_p)) == MGL_EINVAL
        assert sa.L.mgl_sa_weight_targets_by_cost(None, None, 0, None, None) == MGL_EINVAL
        assert sa.L.mgl_sa_target_weights(None, None, None, None) == MGL_EINVAL
    finally:
        sa.close()
        pos.close()
