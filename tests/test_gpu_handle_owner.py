"""The handle's owner of device memory (mgl_owner.h), seen through `mgl_debug_dump` selector 87: two u64 host counters, the
device allocations the handle holds and their bytes as requested.  Handles made the same way hold the same; what an API call
allocates for itself is gone when it returns, also when it fails; the match lists are replaced, not accumulated.  `-m gpu`."""
import numpy as np
import pytest

from _libs import literal_slab
from megalania_amd import binding, corpus

pytestmark = pytest.mark.gpu

N = 4096
DATA = corpus.enwik_like(N, 0x87)

CONFIGS = [
    ("default", {}),
    ("fullwalk", dict(fullwalk=True)),
    ("no_snapshots", dict(snapshots=False)),
    ("serial_build", dict(serial_build=True)),
    ("position_targets", dict(flags=binding.F_POSITION_TARGETS)),
    ("profile", dict(flags=binding.F_PROFILE)),
    ("lc3", dict(lc=3)),
]


def _sa(**kw):
    return binding.SA(DATA, neighbours_per_step=64, **kw)


def _held(sa):
    count, nbytes = sa.debug_dump(binding.DUMP.ALLOCATIONS).tolist()
    return count, nbytes


@pytest.mark.parametrize("name,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_handles_made_the_same_way_hold_the_same(name, kw):
    a, b = _sa(**kw), _sa(**kw)
    held_a, held_b = _held(a), _held(b)
    print(f"{name}: {held_a[0]} allocations, {held_a[1]} bytes")
    assert held_a == held_b
    assert held_a[0] > 0 and held_a[1] > 0
    a.close()
    b.close()
    assert a.h is None and b.h is None


def test_repeated_create_and_close():
    held = set()
    for _ in range(8):
        sa = _sa()
        held.add(_held(sa))
        assert sa.current()[1] > 0
        sa.close()
    assert len(held) == 1


@pytest.fixture()
def seeded():
    sa = _sa()
    sa.seed_greedy(16)
    assert (sa.current()[0]["type"] != 1).any()  # not the all-literal parse
    yield sa
    sa.close()


def test_match_lists_are_replaced_not_accumulated(seeded):
    sa = seeded
    count0, bytes0 = _held(sa)
    sa.seed_sweep([("frontier", 16, 0, 0)], passes=1, depth=8)
    off, src, ln, _ = sa.match_frontier(8)  # the lists of depth 8 the sweep left (held: not made again)
    lists8 = 4 * (N + 1) + (4 + 2) * (len(src) + 1)
    assert _held(sa) == (count0 + 3, bytes0 + lists8)  # offsets, sources, lengths -- and nothing of the sweep's own
    sa.seed_sweep([("frontier", 16, 0, 0)], passes=1, depth=16)
    off16, src16, ln16, _ = sa.match_frontier(16)
    lists16 = 4 * (N + 1) + (4 + 2) * (len(src16) + 1)
    assert _held(sa) == (count0 + 3, bytes0 + lists16)
    assert len(src16) >= len(src) and off16[-1] == len(src16)  # the lists held are depth 16's now
    off8, src8, ln8, _ = sa.match_frontier(8)  # and coming back gives depth 8's again, in the same room
    assert np.array_equal(off, off8) and np.array_equal(src, src8) and np.array_equal(ln, ln8)
    assert _held(sa) == (count0 + 3, bytes0 + lists8)


def test_calls_leave_nothing_behind(seeded):
    sa = seeded
    held = _held(sa)
    costs, _ = sa.props_sweep()
    assert len(costs) == len(binding.PROPS_TRIPLES) and _held(sa) == held
    st = sa.seed_optimal()
    assert st["passes"] > 0 and _held(sa) == held
    cur, cost = sa.current()
    child, xs = sa.crossover([literal_slab(N), cur])
    assert xs["parent_cost"][1] == cost and xs["child_cost"] > 0 and _held(sa) == held


def test_a_crossover_without_room_leaves_nothing_behind(seeded):
    sa = seeded
    held = _held(sa)
    cur, cost = sa.current()
    sa.debug_set(binding.KEY.CROSS_NOMEM, 1)
    with pytest.raises(binding.MglError) as e:
        sa.crossover([literal_slab(N), cur])
    assert "do not fit the device" in str(e.value) and e.value.rc == -2  # MGL_ENOMEM
    assert _held(sa) == held
    child, xs = sa.crossover([literal_slab(N), cur])
    assert xs["parent_cost"][1] == cost and _held(sa) == held
