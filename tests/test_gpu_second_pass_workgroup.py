"""The second pass as a workgroup: one wavefront evaluates a neighbour, the others share its re-simulations (the overlay at a
repair pick and the final one).  mgl_debug_set key 7 sets how many wavefronts cooperate -- 1, 2 or the compiled MGL_BIG_WAVES;
with 1 or 2 a neighbour's contexts take several trips, which otherwise only rare neighbours do.  Costs are integer sums, so
every comparison here is exact.  `-m gpu`."""
import lzma

import numpy as np
import pytest

from _libs import Oracle, literal_slab
from megalania_amd import binding, corpus

pytestmark = pytest.mark.gpu



def set_big_waves(sa, waves):
    """waves = 0 stands for the compiled MGL_BIG_WAVES (4 or 8: the one of the two the library takes); returns the number set"""
    if waves:
        sa.debug_set(binding.KEY.BIG_WAVES, waves)
        return waves
    took = [w for w in (4, 8) if sa.L.mgl_debug_set(sa.h, binding.KEY.BIG_WAVES, w) == 0]
    assert len(took) == 1, took
    return took[0]


def rows(slab):
    return [tuple(int(x) for x in r) for r in zip(slab["type"], slab["dist"], slab["len"])]


def test_knob_takes_1_2_and_the_compiled_size_only():
    sa = binding.SA(corpus.lorem(600), accept="single", neighbours_per_step=8)
    full = set_big_waves(sa, 0)
    for w in range(0, 10):
        assert (sa.L.mgl_debug_set(sa.h, binding.KEY.BIG_WAVES, w) == 0) == (w in (1, 2, full)), w
    sa.close()


# ---- one trajectory whatever the workgroup size
_runs = {}


def _four_engines(name, data, K, steps, start=None, **props):
    """`steps` single-accept steps with 1, 2 and MGL_BIG_WAVES cooperating wavefronts and on the full-walk engine (None), from
    the all-literal slab or from `start`: per engine (per-step current_cost, final cost, final slab, second-pass neighbours,
    most repair picks in a step)"""
    if name not in _runs:
        out = {}
        for waves in (1, 2, 0, None):
            sa = binding.SA(data, accept="single", neighbours_per_step=K, fullwalk=waves is None, **props)
            if waves is not None:
                set_big_waves(sa, waves)
            if start is not None:
                sa.set_slab(start)
            costs, second, picks = [], 0, 0
            for _ in range(steps):
                st = sa.run(1)
                costs.append(st["current_cost"])
                second += st["second_pass_neighbours"]
                if waves is not None:
                    picks = max(picks, int(sa.debug_dump(binding.DUMP.STEP_COUNTS)[0]["repair_picks"]))  # the last step's repair picks
            cur, cost = sa.current()
            print(f"{name} waves={waves}: second-pass neighbours {second}, most repair picks in a step {picks}, final cost {cost}")
            out[waves] = (costs, cost, rows(cur), second, picks)
            sa.close()
        _runs[name] = out
    return _runs[name]


def _same_everywhere(runs):
    for waves in (2, 0, None):
        assert runs[waves][0] == runs[1][0], waves
        assert runs[waves][1:3] == runs[1][1:3], waves


def test_repair_picks_same_trajectory_for_every_workgroup_size():
    """c1, the 4 096 B repeated paragraph, 256 neighbours per step, 60 single steps, from the parse liblzma makes of it
    (preset 6, imported from the .lzma stream): 1, 2 and MGL_BIG_WAVES cooperating wavefronts and the full-walk engine give
    one per-step cost list and one final slab, and the runs did take the second pass and repair picks, whose model is the
    overlay re-simulation.  The start matters: in that parse the first paragraph is matches, literals and rep matches side by
    side, and 13 of a step's 256 neighbours need a repair pick (counted with the CPU oracle at steps 0..2).  From the
    all-literal slab, and on slabs this search evolves from it, c1 takes none (measured: the counter stays 0 through 300
    steps, for 97 seeds): every long match there has the period as its distance, so a long rep the repair meets always
    validates under one of the four slots.  That start is the test below."""
    data, _ = corpus.config_input("c1")
    stream = lzma.compress(data, format=lzma.FORMAT_ALONE,
                           filters=[dict(id=lzma.FILTER_LZMA1, preset=6, dict_size=1 << 22, lc=0, lp=0, pb=0)])
    start, _ = binding.stream_import(stream, data)
    runs = _four_engines("c1 from liblzma's parse", data, 256, 60, start=start)
    _same_everywhere(runs)
    for waves in (1, 2, 0):
        assert runs[waves][3] > 0 and runs[waves][4] > 0, (waves, runs[waves][3:])


def test_long_windows_same_trajectory_for_every_workgroup_size():
    """The same from the all-literal slab: no repair picks, but 74 neighbours per step outgrow the first pass's lists (long
    windows in a repeated paragraph), so the final re-simulation runs over long lists."""
    runs = _four_engines("c1 from literals", corpus.config_input("c1")[0], 256, 60)
    _same_everywhere(runs)
    for waves in (1, 2, 0):
        assert runs[waves][3] > 0, waves


# ---- long lists against the oracle: the reference (the slab at a step and every neighbour's cost there) is computed once per
# (properties, step) and shared by the workgroup sizes; the runs must arrive at the same slab
_reference = {}


def _oracle_costs(props, step, data, cur, seed, K):
    key = (tuple(sorted(props.items())), step)
    if key not in _reference:
        o = Oracle(data, dict_limit=0x400000, **props)
        slab = cur.astype(literal_slab(1).dtype)
        want = np.zeros(K, dtype=np.uint64)
        for j in range(K):
            ok, cost, _ = o.neighbour(slab, seed, step, j, keep=False, K=K)
            want[j] = cost if ok else binding.INVALID_COST
        _reference[key] = (rows(cur), want)
    return _reference[key]


def _long_lists_vs_oracle(waves, props, at_steps):
    data = corpus.lorem(3000)
    K, seed = 96, 5
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=seed, iters_per_epoch=60, **props)
    sa.debug_set(binding.KEY.LIST_CAP, 16)  # first-pass lists of 16 events: most neighbours take the second pass
    set_big_waves(sa, waves)
    done = second = 0
    for step in at_steps:
        if step > done:
            second += sa.run(step - done)["second_pass_neighbours"]
            done = step
        cur, _ = sa.current()
        slab_rows, want = _oracle_costs(props, step, data, cur, seed, K)
        assert rows(cur) == slab_rows, step
        got = sa.neighbours(step, want_diffs=False)[0]
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (step, [(int(j), int(got[j]), int(want[j])) for j in bad[:5]])
    if done:
        print(f"waves={waves} {props}: {second} of {done * K} neighbours took the second pass")
        assert second > done * K // 2
    sa.close()


@pytest.mark.parametrize("waves", [2, 0], ids=["2", "MGL_BIG_WAVES"])
def test_long_lists_vs_oracle(waves):
    _long_lists_vs_oracle(waves, {}, (0, 5, 20))


@pytest.mark.parametrize("waves", [2, 0], ids=["2", "MGL_BIG_WAVES"])
def test_long_lists_vs_oracle_position_and_literal_bits(waves):
    """lc=3, lp=0, pb=2: more probability contexts, so more bitmap words and more distinct contexts per neighbour"""
    _long_lists_vs_oracle(waves, dict(lc=3, lp=0, pb=2), (5,))
