"""What mgl_sa_run reports about the steps it timed (MGL_F_TIMING): which steps carry events, how many of their re-simulation
launches do, and that the times add up.  bench.py computes its headline from these numbers.  `-m gpu`.

The rule: a run of s steps times every step when s <= 16, else every fourth, and at most 512 of them; a timed step of the
split form brackets the k_sim launch of its first two slices.  MGL_NO_ADAPT=1 pins the split form: the adaptive choice goes by
wall clock.  No time is compared against a fixed number."""
import pytest

from megalania_amd import binding, corpus

pytestmark = pytest.mark.gpu


@pytest.fixture
def split_form(monkeypatch):
    monkeypatch.setenv("MGL_NO_ADAPT", "1")
    return monkeypatch


def make(data=None, K=96, accept="single", **kw):
    return binding.SA(corpus.lorem(3000) if data is None else data, neighbours_per_step=K, timing=True, accept=accept, **kw)


def test_short_run_times_every_step(split_form):
    sa = make()
    st = sa.run(16)
    sa.close()
    assert st["steps"] == 16 and st["neighbour_launches"] == 16 and st["sim_launches"] == 16
    assert st["gpu_ms_neighbours"] > 0 and st["gpu_ms_rebuild"] > 0 and st["gpu_ms_sim"] > 0
    # the intervals are disjoint stretches of one stream between the run's begin and end events; the factor covers
    # thirty-three float-rounded elapsed times
    assert st["gpu_ms_neighbours"] + st["gpu_ms_rebuild"] <= st["gpu_ms_total"] * (1 + 1e-4)


def test_longer_run_times_every_fourth_step(split_form):
    sa = make()
    st = sa.run(40)
    sa.close()
    assert st["steps"] == 40 and st["neighbour_launches"] == 10 and st["sim_launches"] == 10


def test_event_pools_are_reused_across_calls(split_form):
    sa = make()
    for _ in range(3):
        st = sa.run(3)
        assert st["steps"] == 3 and st["neighbour_launches"] == 3 and st["sim_launches"] == 3
    sa.close()


def test_two_slices_are_timed_per_step(split_form):
    split_form.setenv("MGL_HALVES", "2")
    sa = make(corpus.lorem(4096), K=1024)
    st = sa.run(8)
    sa.close()
    assert st["neighbour_launches"] == 8 and st["sim_launches"] == 16


def test_one_kernel_form_times_no_resimulation(split_form):
    split_form.setenv("MGL_NO_SPLIT", "1")
    sa = make()
    st = sa.run(8)
    sa.close()
    assert st["neighbour_launches"] == 8 and st["sim_launches"] == 0 and st["gpu_ms_sim"] == 0


def test_fullwalk_engine_times_no_resimulation(split_form):
    sa = make(fullwalk=True)
    st = sa.run(8)
    sa.close()
    assert st["neighbour_launches"] == 8 and st["sim_launches"] == 0


def test_bulk_steps_are_timed(split_form):
    sa = make(accept="bulk")
    st = sa.run(4)
    _, cost = sa.current()
    sa.close()
    assert st["neighbour_launches"] == 4 and st["bulk_steps"] == 4
    assert st["gpu_ms_rebuild"] > 0
    assert st["current_cost"] == cost


def test_at_most_512_steps_are_timed(split_form):
    sa = make(corpus.lorem(1000), K=32)
    st = sa.run(2052)  # 513 steps fall on the stride of four
    sa.close()
    assert st["steps"] == 2052 and st["neighbour_launches"] == 512
