"""The parallel builder, the chain index and the in-place accepts at blocks of 512 and 1 024 positions.

mgl_sa_create picks one block shift from the input size (8 up to 1 MiB, 9 up to 8 MiB, 10 above): the parallel builder's block
and the granularity of the chain index.  Inputs above 1 MiB are too large to compare structures on, so MGL_SB_SHIFT puts
the larger blocks on small inputs, and the shapes here put the edges where those blocks put them: block counts at one
block, a group of MGL_PB_GROUP blocks and a row group of MGL_PB_OFF_ROWS and one past each, a walk that enters blocks at
every offset the exit maps have, the parse of back-to-back length-2 matches, and one trajectory whatever the shift.
tests/test_gpu_incremental.py runs its own structure tests at the same shifts on the golden inputs.  `-m gpu`."""
import functools

import numpy as np
import pytest

from _libs import LITERAL, LONG_REP, MATCH, Oracle, assert_same_base, block_shift, canonical_base, literal_slab, use_block_shift
from _planted_parse import periodic_input
from megalania_amd import binding, corpus

pytestmark = pytest.mark.gpu

SHIFTS = (9, 10)
P = binding.PACKET


def oracle_cost(o, slab) -> int:
    return o.cost_slab(slab.astype(literal_slab(1).dtype))["total"]


def text(size: int) -> bytes:
    """enwik-shaped text up to the size BASELINE config c2 has, prose above it"""
    return corpus.config_input("c2", size)[0] if size <= 100_000 else corpus.prose_like(size, 0xB10C)


def edge_cases():
    """(shift, size, K, steps, accept): one block less a byte, one block, one position into a second block, a full group of
    MGL_PB_GROUP (64) blocks and one block past it, one block past a row group of MGL_PB_OFF_ROWS (128), and 300 001 B
    (586 / 293 blocks), there with bulk steps, so that the second round's slab is thousands of moves from the literal one"""
    out = []
    for s in SHIFTS:
        B = 1 << s
        for size, K, steps, accept in [(B - 1, 32, 20, "single"), (B, 32, 20, "single"), (B + 1, 32, 20, "single"),
                                       (64 * B, 64, 20, "single"), (64 * B + 1, 64, 20, "single"), (128 * B + 1, 256, 20, "single"),
                                       (300001, 2048, 6, "bulk")]:
            out.append(pytest.param(s, size, K, steps, accept, id=f"shift{s}-{size}"))
    return out


@pytest.mark.parametrize("shift,size,K,steps,accept", edge_cases())
def test_parallel_build_equals_serial_build_at_block_count_edges(shift, size, K, steps, accept, monkeypatch):
    """The loop of test_parallel_build_equals_serial_build with the sizes moved to where blocks of 512 and 1 024 positions
    have their edges: both builders derive identical structures (and each an index that agrees with its chains), the cost
    is the oracle's walk, on the all-literal slab and on the slab some SA steps later."""
    data = text(size)
    use_block_shift(monkeypatch, shift)
    par = binding.SA(data, accept=accept, neighbours_per_step=K, seed=3)
    ser = binding.SA(data, accept="single", neighbours_per_step=8, seed=3, serial_build=True, snapshots=False)
    assert block_shift(par) == block_shift(ser) == shift
    o = Oracle(data, dict_limit=0x400000)
    for round_ in range(2):
        cur, cost = par.current()
        ser.set_slab(cur)
        cur2, cost2 = ser.current()
        assert cost == cost2 and (cur == cur2).all()
        assert cost == oracle_cost(o, cur)
        par.set_slab(cur)  # rebuild `par` from scratch through the parallel builder
        assert par.current()[1] == cost
        assert_same_base(canonical_base(par, cur), canonical_base(ser, cur), (shift, size, round_))
        par.run(steps)
    par.close()
    ser.close()


def long_rep_slab(n: int, D: int) -> np.ndarray:
    """D literals, one MATCH of length D at the period's distance, LONG_REP index 0 of length D to the end, literals over
    what is left: one packet per D bytes"""
    s = np.zeros(n, dtype=P)
    s["type"], s["len"] = LITERAL, 1
    s[D] = (MATCH, D - 1, D)
    for pos in range(2 * D, n - D + 1, D):
        s[pos] = (LONG_REP, 0, D)
    return s


@pytest.mark.parametrize("shift", SHIFTS)
def test_walk_enters_blocks_at_every_offset(shift, monkeypatch):
    """Packets of 273 bytes back to back over 300 001 B: 273 is coprime to the block sizes, so over any 273 consecutive blocks
    (586 / 293 in all) the walk enters a block at each of the 273 offsets pb_exits maps, and leaves one at each.  Both
    builders agree, the cost is the oracle's walk, the index agrees with chains that hold one entry per 273 bytes; then
    ten single steps, each patched in place and equal to a rebuild from its slab."""
    n, D = 300001, 273
    data = periodic_input(n, D, 0x273)
    slab = long_rep_slab(n, D)
    entry = (-np.arange((n + (1 << shift) - 1) >> shift) << shift) % D  # offset of the first packet start at or behind each block's first position
    assert len(set(entry[1:274].tolist())) == D
    use_block_shift(monkeypatch, shift)
    par = binding.SA(data, accept="single", neighbours_per_step=256, seed=7, iters_per_epoch=10**7)
    ser = binding.SA(data, accept="single", neighbours_per_step=8, seed=7, serial_build=True, snapshots=False)
    ref = binding.SA(data, accept="single", neighbours_per_step=8, seed=7)
    assert block_shift(par) == block_shift(ser) == block_shift(ref) == shift
    o = Oracle(data, dict_limit=0x400000)
    par.set_slab(slab)
    ser.set_slab(slab)
    cur, cost = par.current()
    assert (cur == slab).all() and cost == ser.current()[1] == oracle_cost(o, slab)
    assert_same_base(canonical_base(par, slab), canonical_base(ser, slab), (shift, "built"))
    accepted = in_place = 0
    for s in range(10):
        st = par.run(1)
        accepted += st["accepted"]
        in_place += 1 if st["accepted"] and not st["full_rebuilds"] else 0
        if st["accepted"]:
            cur, cost = par.current()
            assert cost == oracle_cost(o, cur), s
            ref.set_slab(cur)
            assert_same_base(canonical_base(par, cur), canonical_base(ref, cur), (shift, s))
    print(f"shift {shift}: {accepted} of 10 steps accepted, {in_place} patched in place")
    assert accepted >= 5 and in_place >= 1  # (the oracle's replay of these ten steps accepts eight; a step that gave up was rebuilt, not patched)
    for x in (par, ser, ref):
        x.close()


@pytest.mark.parametrize("shift", SHIFTS)
def test_densest_parse_fits_the_staging_area(shift, monkeypatch):
    """The kind of parse MGL_PB_STAGE_PER_POS is sized for: length-2 matches at a far distance, back to back (a random
    65 536-byte block three times over; literals on the first copy): 16 staged events per match, 8 per position, where a
    literal run stages 9 and the area holds 16.  A block that outgrows its staging area sets pb.stage_over, which
    pb_finish turns into MGL_ERR_WALK_OVERRUN in the control block: mgl_sa_set_slab then refuses the slab (MglError here),
    and mgl_sa_run fails its consistency check.  Neither happens; parallel == serial build, cost == the oracle's walk."""
    D = 65536
    n = 3 * D
    data = periodic_input(n, D, 0xDE5E)
    slab = literal_slab(n).astype(P)
    slab["type"][D::2], slab["dist"][D::2], slab["len"][D::2] = MATCH, D - 1, 2
    use_block_shift(monkeypatch, shift)
    par = binding.SA(data, accept="single", neighbours_per_step=64, seed=7)
    ser = binding.SA(data, accept="single", neighbours_per_step=8, seed=7, serial_build=True, snapshots=False)
    assert block_shift(par) == block_shift(ser) == shift
    o = Oracle(data, dict_limit=0x400000)
    par.set_slab(slab)  # raises if the build left an error flag
    ser.set_slab(slab)
    cur, cost = par.current()
    assert (cur == slab).all() and cost == ser.current()[1] == oracle_cost(o, slab)
    assert_same_base(canonical_base(par, slab), canonical_base(ser, slab), (shift, "densest"))
    st = par.run(2)     # raises if the control block holds an error flag behind the steps
    assert st["steps"] == 2 and st["current_cost"] == oracle_cost(o, par.current()[0])
    par.close()
    ser.close()


def test_one_trajectory_whatever_the_shift(monkeypatch):
    """The index narrows searches and decides no result: three chains with blocks of 256, 512 and 1 024 positions walk in
    lockstep through 40 bulk and 40 single steps, with equal slabs on the way, and cost every neighbour of one more step
    alike -- and like the oracle (every eighth).  chain_block inside k_sim, the second pass and both accepts, on an evolved slab."""
    data, _ = corpus.config_input("c2", 60000)
    K, seed = 512, 1673551
    chains = []
    for shift in (8, 9, 10):
        use_block_shift(monkeypatch, shift)
        chains.append(binding.SA(data, accept="bulk", neighbours_per_step=K, seed=seed))
        assert block_shift(chains[-1]) == shift
    for s in range(80):
        if s == 40:
            for x in chains:
                x.set_accept_mode("single")
        sts = [x.run(1) for x in chains]
        for k in ("current_cost", "best_cost", "accepted", "evaluations", "dropped_neighbours"):
            assert sts[0][k] == sts[1][k] == sts[2][k], (s, k, [st[k] for st in sts])
        if s % 8 == 7:
            slabs = [x.current()[0] for x in chains]
            assert (slabs[0] == slabs[1]).all() and (slabs[0] == slabs[2]).all(), s
    cur = chains[0].current()[0]
    costs = [x.neighbours(80, want_diffs=False)[0] for x in chains]
    assert (costs[0] == costs[1]).all() and (costs[0] == costs[2]).all()
    o = Oracle(data, dict_limit=0x400000)
    curo = cur.astype(literal_slab(1).dtype)
    for j in range(0, K, 8):
        ok, c, _ = o.neighbour(curo, seed, 80, j, keep=False, K=K)
        assert int(costs[0][j]) == (c if ok else binding.INVALID_COST), j
    for x in chains:
        x.close()


@functools.lru_cache(maxsize=None)
def prose(size: int) -> bytes:
    return corpus.prose_like(size, 0x51E)


MIB = 1 << 20


@pytest.mark.parametrize("size,shift", [(MIB, 8), (MIB + 1, 9), (8 * MIB, 9), (8 * MIB + 1, 10)], ids=["1MiB", "1MiB+1", "8MiB", "8MiB+1"])
def test_size_rule_picks_the_shift(size, shift, monkeypatch):
    """With no override the input's size picks the shift: 8 up to 1 MiB, 9 up to 8 MiB, 10 from one byte above; blocks and
    index row stride follow from it.  All-literal slab, no steps.  (Measured on an MI355X: creating a handle on 8 MiB or on
    8 MiB + 1 B takes 0.07 s; the 8 MiB case 0.26 s in all, with the prose it makes, the 8 MiB + 1 B case 0.11 s.)"""
    use_block_shift(monkeypatch, None)
    data = prose(MIB + 1 if size <= MIB + 1 else 8 * MIB + 1)[:size]
    sa = binding.SA(data, accept="single", neighbours_per_step=8)
    nsb = (size + (1 << shift) - 1) >> shift
    assert [int(x) for x in sa.debug_dump(binding.DUMP.INDEX_GEOMETRY)] == [shift, nsb, (nsb + 2 + 3) & ~3]
    sa.close()
