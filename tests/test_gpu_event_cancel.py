"""Event-level cancellation at the paired site of the window walk (changes_add_pair, csrc/mgl_kernels2.hip): where a neighbour
packet and a base packet start at the same position and do not cancel whole, the events both plans hold in the same slot --
same context, same bit -- stay off both change lists.  That is exact because a context occurs at most once in a packet's plan
(the CPU test), and every cost, trajectory and drop decision below is compared with the oracle or the full-walk engine, which
know nothing of it.  Costs are integer sums: every comparison is exact.  MGL_NO_EVCANCEL=1 restores the packet-level lists;
mgl_debug_dump selector 10 (DUMP.STEP_COUNTS), field `cancelled`, counts the cancelled pairs of the last step's (or mgl_neighbours call's) costed neighbours.
The GPU tests: `-m gpu`."""
import lzma
import os
import subprocess

import numpy as np
import pytest

from _libs import Oracle, literal_slab
from conftest import slab_from_rle
from megalania_amd import binding, corpus

WIN_DROPPED = 0xFFFFFFFE  # csrc/mgl_device.h: MGL_WIN_DROPPED
PROPS = [(0, 0, 0), (3, 0, 2), (0, 4, 4)]


def P(slab):
    return np.ascontiguousarray(slab).astype(binding.PACKET)


def rows(slab):
    return [tuple(int(x) for x in r) for r in zip(slab["type"], slab["dist"], slab["len"])]


def liblzma_parse(data):
    stream = lzma.compress(data, format=lzma.FORMAT_ALONE,
                           filters=[dict(id=lzma.FILTER_LZMA1, preset=6, dict_size=1 << 22, lc=0, lp=0, pb=0)])
    return binding.stream_import(stream, data)[0]


# ---- 1. CPU: a context occurs at most once in one packet
def _no_context_twice(name, data, slab, props):
    lc, lp, pb = props
    t = Oracle(data, lc=lc, lp=lp, pb=pb).trace_events(np.ascontiguousarray(slab).astype(literal_slab(1).dtype))
    assert len(t["ctx"]) > 0, name
    key = (t["pos"].astype(np.uint64) << np.uint64(32)) | t["ctx"].astype(np.uint64)
    uniq, counts = np.unique(key, return_counts=True)
    twice = uniq[counts > 1]
    assert len(twice) == 0, (name, props, [(int(k >> np.uint64(32)), int(k & np.uint64(0xFFFFFFFF))) for k in twice[:5]])


@pytest.mark.parametrize("props", PROPS, ids=lambda p: "%d%d%d" % p)
def test_no_context_twice_in_a_packet(props, golden, golden_input):
    """Oracle.trace_events lists every coded bit of a walk with its context and its packet's position: no (context, position)
    occurs twice, whatever the packet kinds (the evolved golden walks hold matches, short and long reps after literals and after
    matches; liblzma's parse of c1 and of lorem(3000) adds its own mix) and whatever lc / lp / pb.  The cancellation's
    exactness rests on this: one context at one position is at most one removed and one inserted event."""
    for name, packets in golden["evolved_walks"].items():
        data = golden_input(name)
        _no_context_twice(name, data, slab_from_rle(len(data), packets), props)
    for name, data in (("c1", corpus.config_input("c1")[0]), ("lorem3000", corpus.lorem(3000))):
        _no_context_twice(name + " liblzma", data, liblzma_parse(data), props)


def test_no_context_twice_in_a_plan_of_the_device_model(tmp_path):
    """The same on the slot-to-context map the kernels themselves run (csrc/mgl_model.h: mgl_plan_packet, mgl_plan_event, host
    and device code from one source), per packet kind: tests/plan_contexts_main.c plans literals (with and without a match
    byte), matches over every distance class and length class, short reps and long reps of every index under all 12 states,
    32 positions and six lc / lp / pb, and checks that no plan holds a context twice, that every key fits 16 bits, and that
    one packet at one position has the same slots under every state -- what the lane-wise comparison relies on."""
    exe = tmp_path / "plan_contexts"
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "plan_contexts_main.c")
    subprocess.check_call([os.environ.get("CC", "gcc"), "-std=gnu11", "-O1", "-Wall", "-Wextra", "-Werror", "-o", str(exe), src])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and r.stdout.strip().endswith(" 0 misses"), r.stdout[-2000:]


# ---- 2. / 3. costs against the oracle; the reference is computed once per (shape, step) and shared
_reference = {}


def _oracle_costs(shape, props, step, data, cur, seed, K):
    key = (shape, tuple(sorted(props.items())), step)
    if key not in _reference:
        o = Oracle(data, dict_limit=0x400000, **props)
        slab = np.ascontiguousarray(cur).astype(literal_slab(1).dtype)
        want = np.zeros(K, dtype=np.uint64)
        for j in range(K):
            ok, cost, _ = o.neighbour(slab, seed, step, j, keep=False, K=K)
            want[j] = cost if ok else binding.INVALID_COST
        _reference[key] = (rows(cur), want)
    return _reference[key]


def _set_big_waves(sa, waves):
    """waves = 0: the compiled MGL_BIG_WAVES (the one of 4 and 8 the library takes)"""
    if waves:
        sa.debug_set(binding.KEY.BIG_WAVES, waves)
        return
    took = [w for w in (4, 8) if sa.L.mgl_debug_set(sa.h, binding.KEY.BIG_WAVES, w) == 0]
    assert len(took) == 1, took


def _costs_vs_oracle(shape, data, K, seed, at_steps, start, cap, waves, props, switch_on, **kw):
    """every neighbour's cost at `at_steps` (running single steps in between: every variant must arrive at the same slabs)
    against the oracle's; returns (cancelled pairs over the mgl_neighbours calls, second-pass neighbours of the steps run)"""
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=seed, **props, **kw)
    if cap:
        sa.debug_set(binding.KEY.LIST_CAP, cap)
    _set_big_waves(sa, waves)
    if start is not None:
        sa.set_slab(start)
    done = second = pairs = 0
    for step in at_steps:
        if step > done:
            second += sa.run(step - done)["second_pass_neighbours"]
            done = step
        cur, _ = sa.current()
        slab_rows, want = _oracle_costs(shape, props, step, data, cur, seed, K)
        assert rows(cur) == slab_rows, step
        got = sa.neighbours(step, want_diffs=False)[0]
        n = int(sa.debug_dump(binding.DUMP.STEP_COUNTS)[0]["cancelled"])
        print(f"{shape} step {step} cap {cap or 'allocated'} waves {waves or 'MGL_BIG_WAVES'} switch {'on' if switch_on else 'off'}: {n} cancelled pairs")
        pairs += n
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (step, [(int(j), int(got[j]), int(want[j])) for j in bad[:5]])
    sa.close()
    return pairs, second, done


_C1_CASES = [(sw, cap, waves) for sw in ("on", "off") for cap in (0, 16) for waves in (1, 2, 0)] + [("on_no_split", 0, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("switch,cap,waves", _C1_CASES, ids=lambda v: {0: "default"}.get(v, str(v)))
def test_c1_liblzma_costs_vs_oracle(monkeypatch, switch, cap, waves):
    """c1 (4 096 B) from the parse liblzma makes of it, 256 neighbours per step, the split form in every step, at steps 0, 3
    and 8: every neighbour's cost equals the oracle's with the cancellation on and off, with first-pass lists at the allocated
    capacity (cap 0) and of 16 events (most neighbours take the second pass then, some of them resumed from a continuation
    record, which carries the cancelled count along), and with 1, 2 and MGL_BIG_WAVES (waves 0) wavefronts on a second-pass
    neighbour's re-simulations; once more in the one-kernel form (MGL_NO_SPLIT=1).  The counter of cancelled pairs is above 0
    with the switch on and 0 with it off."""
    monkeypatch.setenv("MGL_NO_ADAPT", "1")
    if switch == "off":
        monkeypatch.setenv("MGL_NO_EVCANCEL", "1")
    else:
        monkeypatch.delenv("MGL_NO_EVCANCEL", raising=False)
    if switch == "on_no_split":
        monkeypatch.setenv("MGL_NO_SPLIT", "1")
    data, _ = corpus.config_input("c1")
    pairs, second, done = _costs_vs_oracle("c1 liblzma", data, 256, 1673551, (0, 3, 8), liblzma_parse(data), cap, waves, {}, switch != "off")
    assert (pairs > 0) if switch != "off" else (pairs == 0), pairs
    if cap:
        assert second > done * 256 // 2, second


@pytest.mark.gpu
@pytest.mark.parametrize("props,at_steps", [((3, 0, 2), (0, 5, 20)), ((0, 4, 4), (0, 5, 20))], ids=["302", "044"])
def test_lorem_long_lists_vs_oracle(monkeypatch, props, at_steps):
    """lorem(3000), 96 neighbours per step, first-pass lists of 16 events as in test_long_lists_vs_oracle
    (tests/test_gpu_second_pass_workgroup.py), under lc=3 lp=0 pb=2 and lc=0 lp=4 pb=4: more probability contexts, and with
    position bits the same packet at the same position under another state shares its literal and length contexts."""
    monkeypatch.delenv("MGL_NO_EVCANCEL", raising=False)
    lc, lp, pb = props
    pairs, second, done = _costs_vs_oracle("lorem3000", corpus.lorem(3000), 96, 5, at_steps, None, 16, 0, dict(lc=lc, lp=lp, pb=pb), True, iters_per_epoch=60)
    assert pairs > 0
    assert second > done * 96 // 2


# ---- 4. trajectory against the full-walk engine
def _steps(sa, steps):
    costs = []
    for _ in range(steps):
        costs.append(sa.run(1)["current_cost"])  # raises on any error flag of the control block
    cur, cost = sa.current()
    return costs, cost, rows(cur)


@pytest.mark.gpu
def test_two_slices_trajectory_vs_fullwalk(monkeypatch):
    """20 000 B of the c2-shaped text, 1 024 neighbours per step in two slices, 12 single steps of the split form with the
    cancellation on: costs per step, final cost and final slab are the full-walk engine's."""
    monkeypatch.delenv("MGL_NO_EVCANCEL", raising=False)
    monkeypatch.setenv("MGL_NO_ADAPT", "1")
    monkeypatch.setenv("MGL_HALVES", "2")
    data, _ = corpus.config_input("c2", 20000)
    ref = binding.SA(data, accept="single", neighbours_per_step=1024, fullwalk=True)
    want = _steps(ref, 12)
    ref.close()
    sa = binding.SA(data, accept="single", neighbours_per_step=1024)
    got = _steps(sa, 12)
    pairs = int(sa.debug_dump(binding.DUMP.STEP_COUNTS)[0]["cancelled"])
    sa.close()
    print(f"c2 20000 K=1024: final cost {got[1]}, {pairs} cancelled pairs in the last step")
    assert got == want
    assert pairs > 0


# ---- 5. drop decisions
def _statuses(sa, step):
    costs = sa.neighbours(step, want_diffs=False)[0]
    win = sa.debug_dump(binding.DUMP.WINDOWS).reshape(-1, 2)
    pairs = int(sa.debug_dump(binding.DUMP.STEP_COUNTS)[0]["cancelled"])
    return [(1 if int(c) != binding.INVALID_COST else -1 if int(w) == WIN_DROPPED else 0, int(c)) for c, w in zip(costs, win[:, 1])], pairs


@pytest.mark.gpu
def test_drop_decisions_vs_oracle(monkeypatch):
    """Every neighbour's status -- costed, no candidate, dropped -- and cost equal neighbour_ex's with the cancellation on,
    on two shapes.
    (a) The shape of test_windows_and_drop_counter_vs_oracle (tests/test_gpu_parity.py): lorem(3000) after ten bulk steps of
    the oracle, 128 neighbours at step 777.  The oracle drops none of these 128 (counted on the CPU: 106 costed, 22 without a
    candidate, at steps 0..3 likewise), so this shape holds the device to dropping none either.
    (b) `one_period` of tests/_random_parse.py, steps 0 and 5 of 128 neighbours: the base on which the event-list rule fires
    (tests/test_random_parse_cpu.py::test_every_drop_rule_fires), beside the journal and the walk length; asserted here
    that it does.
    Capacity rule (2) counts events at packet level (stored + cancelled, Changes::n_cancel), as the oracle and the full-walk
    engine do.  No known shape puts a neighbour between the counted and the stored total at 4 096 -- the two differ by a few
    dozen events -- so a drop decision that only the counted total gets right is not observed here: that case rests on the
    separate count and on stored <= counted, not on a run."""
    import _random_parse as rp
    from _libs import DROP_EVENTS

    monkeypatch.delenv("MGL_NO_EVCANCEL", raising=False)
    data = corpus.lorem(3000)
    n, K, seed = len(data), 128, 5
    o = Oracle(data, dict_limit=0x400000)
    slab, best = literal_slab(n), literal_slab(n)
    o.sa_batched(slab, best, 0, 0, seed, K, 0, n, 0, 10, modes=np.ones(10, dtype=np.uint8))
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=seed)
    sa.set_slab(P(slab))
    got, pairs = _statuses(sa, 777)
    sa.close()
    want = [o.neighbour_ex(slab, seed, 777, j, K=K, reason=True) for j in range(K)]
    assert got == [(w[0], w[1]) for w in want], [(j, g, (w[0], w[1])) for j, (g, w) in enumerate(zip(got, want)) if g != (w[0], w[1])][:5]
    print(f"lorem(3000) after 10 bulk steps: {sum(w[0] == -1 for w in want)} of {K} neighbours dropped, {pairs} cancelled pairs")
    assert pairs > 0

    data, slab = rp.base("one_period")
    sa = binding.SA(data, dict_limit=rp.dict_limit_of("one_period"), accept="single", neighbours_per_step=rp.K, seed=rp.SEED)
    sa.set_slab(P(slab))
    by_events = 0
    for step in rp.STEPS:
        got, pairs = _statuses(sa, step)
        want = rp.oracle_neighbours("one_period", step)
        assert got == [(w[0], w[1]) for w in want], (step, [(j, g, (w[0], w[1])) for j, (g, w) in enumerate(zip(got, want)) if g != (w[0], w[1])][:5])
        by_events += sum(1 for w in want if w[0] == -1 and w[4] & DROP_EVENTS)
        print(f"one_period step {step}: {sum(w[0] == -1 for w in want)} of {rp.K} neighbours dropped, {pairs} cancelled pairs")
    sa.close()
    assert by_events > 0
