"""The cost map of the current slab read off the event chains (mgl_cost_map_live, SA.cost_map_live;
csrc/mgl_costmap_live.hip): integer for integer the serial walk's map and report (SA.cost_map of the current slab) and the
host's (binding.host_cost_map), with the total the current cost, in every state the base structures get into -- built by
either builder, patched by the single and the batch accept, rebuilt after a give-up, copied from a snapshot, with chains
that have moved in the pool -- at the sizes where a block of the chain index has its edges, under five triples, both block
shifts the tests can force, and on the full-walk engine, which has no chains and answers by the walk.  `-m gpu`."""
import ctypes as C
import functools
import lzma

import numpy as np
import pytest

from _libs import PACKET, block_shift, use_block_shift
from megalania_amd import binding, corpus

pytestmark = pytest.mark.gpu

MGL_ENOMEM = -2
K = 256
SEED = 0xC057
TRIPLES = [(0, 0, 0), (3, 0, 2), (0, 4, 2), (2, 2, 0), (4, 0, 4)]
_BASE = corpus.enwik_like(6000, 0x71)
DATA = _BASE + _BASE[1000:3277]  # tests/test_gpu_focus.py's: 8 277 bytes, not a multiple of 64, long matches in the greedy parse
LOREM = corpus.lorem(4096)
ELF = corpus._synthetic_elf(1 << 16, 0xEF)
C2 = corpus.config_input("c2")[0]
# what the file's cases saw, for test_zz_every_packet_type_and_direct_bits_were_seen (the file's last test)
SEEN = {"type_packets": [0, 0, 0, 0], "direct_bits": 0, "checks": 0}


def xz_parse(data, lc=0, lp=0, pb=0):
    stream = lzma.compress(data, format=lzma.FORMAT_ALONE,
                           filters=[dict(id=lzma.FILTER_LZMA1, preset=9 | lzma.PRESET_EXTREME, dict_size=1 << 22, lc=lc, lp=lp, pb=pb)])
    return binding.stream_import(stream, data)[0]


def check(sa, data, what):
    """live == walk == host on the current slab, total == current cost"""
    cur, cost = sa.current()
    live_map, live = sa.cost_map_live()
    walk_map, walk = sa.cost_map()
    host_map, host = binding.host_cost_map(data, cur, (sa.props.lc, sa.props.lp, sa.props.pb))
    live.pop("gpu_ms"), walk.pop("gpu_ms")
    assert live == walk == host, (what, live, walk, host)
    assert live["total"] == cost, (what, live["total"], cost)
    for other in (walk_map, host_map):
        bad = np.nonzero(live_map != other)[0]
        assert len(bad) == 0, (what, bad[:5], live_map[bad[:5]], other[bad[:5]])
    SEEN["type_packets"] = [a + b for a, b in zip(SEEN["type_packets"], live["type_packets"])]
    SEEN["direct_bits"] += live["class_bits"][5]
    SEEN["checks"] += 1
    return live


def states(data, what, lc=0, lp=0, pb=0, fullwalk=False, steps=40):
    """states 1-4 and 7 of one handle: all-literal, greedy, an imported xz parse, after single steps, the best slab's snapshot"""
    sa = binding.SA(data, neighbours_per_step=K, seed=SEED, accept="single", lc=lc, lp=lp, pb=pb, fullwalk=fullwalk)
    try:
        check(sa, data, what + " literal")
        if len(data) >= 2:
            sa.seed_greedy(8)
            check(sa, data, what + " greedy")
            sa.set_slab(xz_parse(data, lc, lp, pb))
            check(sa, data, what + " xz")
        if len(data) >= 63:
            sa.run(steps)
            check(sa, data, what + f" {steps} steps")
        if not fullwalk and len(data) >= 63:
            best_cost = sa.best_cost()
            sa.begin_epoch(0, from_best=False)
            check(sa, data, what + " literal again")
            sa.begin_epoch(1, from_best=True)
            assert check(sa, data, what + " from best")["total"] == best_cost
    finally:
        sa.close()


SMALL = [1, 63, 64, 65, 257]


@pytest.mark.parametrize("n", SMALL)
def test_small_sizes_and_the_first_block_edge(n):
    """n = 1 is the smallest mgl_sa_create accepts; 257 is one position into a second block of the chain index (shift 8)"""
    states(C2[:n], f"n {n}", steps=12)


@pytest.mark.parametrize("name", ["focus", "lorem", "elf"])
@pytest.mark.parametrize("fullwalk", [False, True], ids=["incremental", "fullwalk"])
def test_states_on_both_engines(name, fullwalk):
    data = {"focus": DATA, "lorem": LOREM, "elf": ELF}[name]
    if fullwalk and name == "elf":
        data = data[: 1 << 13]  # the full-walk engine walks the file per neighbour
    states(data, name, fullwalk=fullwalk, steps=12 if fullwalk else 40)


@pytest.mark.parametrize("triple", TRIPLES[1:], ids=lambda t: "lc%d-lp%d-pb%d" % t)
def test_triples(triple):
    lc, lp, pb = triple
    states(DATA, str(triple), lc, lp, pb)
    states(ELF[: 1 << 13], "fullwalk " + str(triple), lc, lp, pb, fullwalk=True, steps=4)


@pytest.mark.parametrize("shift", [9, 10])
def test_larger_blocks(shift, monkeypatch):
    use_block_shift(monkeypatch, shift)
    B = 1 << shift
    for n in (B - 1, B, B + 1):
        data = C2[:n]
        sa = binding.SA(data, neighbours_per_step=K, seed=SEED, accept="single")
        try:
            assert block_shift(sa) == shift
            check(sa, data, f"shift {shift} n {n} literal")
            sa.seed_greedy(8)
            sa.run(20)
            check(sa, data, f"shift {shift} n {n} steps")
        finally:
            sa.close()
    states(DATA, f"shift {shift} focus", 0, 4, 2)
    states(LOREM, f"shift {shift} lorem")


def test_bulk_steps_by_rebuild_and_by_batch_accept():
    data = DATA
    sa = binding.SA(data, neighbours_per_step=K, seed=SEED, accept="bulk")
    try:
        for s in range(8):  # from the all-literal slab: thousands of moves, the rebuild
            sa.run(1)
        check(sa, data, "8 bulk steps from literal")
        sa.seed_greedy(64)
        acc0 = sa.batch_counters()[0]
        for s in range(6):  # on the evolved slab: few moves, patched in by the batch accept
            sa.run(1)
            check(sa, data, f"bulk step {s} on greedy")
        assert sa.batch_counters()[0] - acc0 >= 3, sa.batch_counters()
        # a batch accept that gives up behind its commit: the rebuild takes the step
        fb0 = sa.batch_counters()[1]
        sa.debug_set(binding.KEY.BATCH_FAIL, 1 | (1 << 32))
        for s in range(6):
            sa.run(1)
            check(sa, data, f"bulk step {s} behind a forced give-up")
        assert sa.batch_counters()[1] - fb0 == 1, sa.batch_counters()
    finally:
        sa.close()


def test_builder_that_redoes_every_segment_serially():
    data = DATA
    sa = binding.SA(data, neighbours_per_step=K, seed=SEED, accept="bulk")
    try:
        sa.debug_set(binding.KEY.PBUILD_FIX, 1)
        sa.seed_greedy(8)
        check(sa, data, "pbuild fix, greedy")
        sa.run(3)
        check(sa, data, "pbuild fix, bulk steps")
    finally:
        sa.close()


def test_chains_that_moved_in_the_pool():
    data = LOREM
    sa = binding.SA(data, neighbours_per_step=K, seed=SEED, accept="single")
    try:
        top0 = int(sa.debug_dump(binding.DUMP.POOL_TOP)[0])
        sa.run(300)
        check(sa, data, "300 single steps on lorem")
        sa.run(300)
        check(sa, data, "600 single steps on lorem")
        assert int(sa.debug_dump(binding.DUMP.POOL_TOP)[0]) > top0, "no chain outgrew its slot: take more steps"
    finally:
        sa.close()


def _same_slab(a, b):
    return bool((np.ascontiguousarray(a).astype(PACKET) == np.ascontiguousarray(b).astype(PACKET)).all())


def test_the_call_leaves_the_search_untouched():
    """two handles, one asked for live maps between its runs: same slabs, costs, routes, focus, weights and neighbours"""
    data = C2[: 1 << 15]
    one, two = (binding.SA(data, neighbours_per_step=1024, seed=SEED) for _ in range(2))
    try:
        for sa in (one, two):
            sa.run(6)
            sa.set_focus(1000, 30000)
            sa.weight_targets_by_cost(5)
        before = two.current(), two.best(), two.focus(), two.target_weights()
        for _ in range(3):
            check(two, data, "between runs")
        after = two.current(), two.best(), two.focus(), two.target_weights()
        assert _same_slab(before[0][0], after[0][0]) and before[0][1] == after[0][1]
        assert _same_slab(before[1][0], after[1][0]) and before[1][1] == after[1][1]
        assert before[2] == after[2]
        assert (before[3][0] == after[3][0]).all() and before[3][1:] == after[3][1:]
        g = 6
        (c1, n1, _), (c2, n2, _) = one.neighbours(g, want_diffs=False), two.neighbours(g, want_diffs=False)
        assert (c1 == c2).all() and (n1 == n2).all()
        s1, s2 = one.run(8), two.run(8)
        assert one.step_modes().tolist() == two.step_modes().tolist()
        for k in ("current_cost", "best_cost", "accepted", "evaluations", "improved"):
            assert s1[k] == s2[k], k
        assert _same_slab(one.current()[0], two.current()[0]) and _same_slab(one.best()[0], two.best()[0])
        check(two, data, "after the second run")
    finally:
        one.close()
        two.close()


def test_no_room_for_the_buffers_leaves_the_handle_usable():
    data = DATA
    for fullwalk in (False, True):
        sa = binding.SA(data, neighbours_per_step=K, seed=SEED, accept="single", fullwalk=fullwalk)
        try:
            sa.seed_greedy(8)
            sa.debug_set(binding.KEY.COSTMAP_NOMEM, 1)
            out = np.full(sa.n, 0xA5A5A5A5, dtype=np.uint32)
            rep = binding.CostReport()
            rep.total = 77
            rc = sa.L.mgl_cost_map_live(sa.h, out.ctypes.data_as(C.c_void_p), C.byref(rep))
            assert rc == MGL_ENOMEM and (out == 0xA5A5A5A5).all() and rep.total == 77
            check(sa, data, "after ENOMEM")
            assert sa.run(3)["steps"] == 3
            check(sa, data, "and a run")
        finally:
            sa.close()
    assert binding.hip_lib().mgl_cost_map_live(None, None, None) == -1


@functools.lru_cache(maxsize=None)
def _elf_direct_bits():
    return binding.host_cost_map(ELF, xz_parse(ELF))[1]["class_bits"][5]


def test_zz_every_packet_type_and_direct_bits_were_seen():
    """the cases above must not all be parses without rep packets or far distances (runs last: pytest keeps file order)"""
    assert _elf_direct_bits() > 0, "the ELF slice's imported parse has no direct bits: lengthen the slice"
    if SEEN["checks"] < 40:  # only part of the file ran
        return
    assert all(v > 0 for v in SEEN["type_packets"]), SEEN
    assert SEEN["direct_bits"] > 0, SEEN
