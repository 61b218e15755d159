"""The order in which the fused launch (k_neighbours2<false, MGL_NBR_PICKWALK>) takes up the neighbours of its slice: the
picking ones first (k_targets' class hint, k_pick_order), against the parent's blockIdx order (MGL_NO_ORDER=1).

  results    the order moves no figure: per-step stats, current and best cost, the whole slab and the per-neighbour outputs
             of the last step are bit for bit the same with and without it
  order      every slice of `order` is a permutation of the slice, picking neighbours (hint != 0) in front, ascending in j
             inside each class -- for the hints of a step and for hint bytes written by the test (all 0, all 1, alternating,
             random)
  hint       where the slab is final when the targets are made (single steps), the hint is the kernels' own decision: the
             pick half of the two-launch form (MGL_NO_FUSE=1) leaves `mutated` per neighbour in word 7 of its pickstate
             record (dump 28), and hint == 1 - mutated for every neighbour.  Both ways a step's targets are made are
             covered: at the head of the step (steps run one at a time) and beside the previous step's accept (the last
             step of a run of two).  Behind a batch accept the hint is a guess: its share of wrong bytes is printed.

Shapes as in test_gpu_fused_pick_walk.py, the smallest at which each path can go wrong.  `-m gpu`."""
import numpy as np
import pytest

from megalania_amd import binding, corpus
from test_gpu_fused_pick_walk import _close, _same_end, _steps

pytestmark = pytest.mark.gpu

SWITCHES = ("MGL_NO_SPLIT", "MGL_NO_FUSE", "MGL_NO_CONT", "MGL_HALVES", "MGL_PICK_WAVES", "MGL_NO_ORDER")


def _env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MGL_NO_ADAPT", "1")  # the split form at every step: the launch under test is the one that runs
    for k, v in env:
        monkeypatch.setenv(k, v)


def _pair(monkeypatch, data, env=(), **kw):
    """(ordered chain, chain in blockIdx order) from the same seed; the switches are read at create"""
    _env(monkeypatch, env)
    ordered = binding.SA(data, **kw)
    monkeypatch.setenv("MGL_NO_ORDER", "1")
    plain = binding.SA(data, **kw)
    monkeypatch.delenv("MGL_NO_ORDER")
    assert len(ordered.debug_dump(binding.DUMP.PICK_ORDER)) == kw["neighbours_per_step"] and len(plain.debug_dump(binding.DUMP.PICK_ORDER)) == 0
    return ordered, plain


def _slices(K, halves):
    s = halves if halves >= 2 and K >= 1024 else 1
    return [(K * h // s, K * (h + 1) // s) for h in range(s)]


def _check_order(chain, K, halves, what):
    hint, order = chain.debug_dump(binding.DUMP.PICK_HINTS), chain.debug_dump(binding.DUMP.PICK_ORDER).astype(np.int64)
    assert len(hint) == K and len(order) == K
    for j0, j1 in _slices(K, halves):
        o = order[j0:j1]
        assert (np.sort(o) == np.arange(j0, j1)).all(), (what, j0, j1)
        cls = hint[o] != 0
        assert not (~cls[:-1] & cls[1:]).any(), (what, j0, "a picking neighbour behind a walk-only one")
        for c in (True, False):
            assert (np.diff(o[cls == c]) > 0).all(), (what, j0, c, "j does not ascend inside the class")
    return hint


def _check_adversarial(chain, K, halves, what):
    for pattern in (0, 1, 2, 0x9E3779B97F4A7C15, 12345):
        chain.debug_set(binding.KEY.PICK_HINTS, pattern)
        hint = _check_order(chain, K, halves, (what, pattern))
        if pattern == 0:
            assert not hint.any()
        elif pattern == 1:
            assert hint.all()
        elif pattern == 2:
            assert (hint == (np.arange(K) & 1)).all()
        else:
            assert 0 < np.count_nonzero(hint) < K or K < 8


def _decisions(chain, K):
    """what the two-launch form's pick half decided at the last step: 1 = grow/shrink"""
    return chain.debug_dump(binding.DUMP.PICKSTATE)["mutated"]


def _check_hint(monkeypatch, data, K, env=(), greedy=False, setup=None, auto_steps=0, **kw):
    _env(monkeypatch, list(env) + [("MGL_NO_FUSE", "1")])
    c = binding.SA(data, neighbours_per_step=K, accept="single", **kw)
    monkeypatch.delenv("MGL_NO_FUSE")
    if greedy:
        c.seed_greedy()
    if setup:
        setup(c)
    seen = 0
    for run in (1, 1, 1, 2, 2, 2):  # targets made at the head of the step, then beside the previous step's accept
        c.run(run)
        hint, dec = c.debug_dump(binding.DUMP.PICK_HINTS), _decisions(c, K)
        assert set(np.unique(dec)) <= {0, 1}
        wrong = np.nonzero(hint != 1 - dec)[0]
        assert len(wrong) == 0, (run, len(wrong), wrong[:8])
        seen += int(dec.sum())
    if auto_steps:
        c.set_accept_mode("auto")
        bad = tot = 0
        for _ in range(auto_steps // 2):
            c.run(2)
            hint, dec = c.debug_dump(binding.DUMP.PICK_HINTS), _decisions(c, K)
            bad += int(np.count_nonzero(hint != 1 - dec)); tot += K
        print(f"hint bytes that differ from the decision in auto steps: {bad} of {tot} ({100.0 * bad / tot:.2f} %)")
    c.close()
    return seen


def test_single_slice(monkeypatch):
    """one slice; the batch accept of the `auto` steps makes hints on a slab that is not final"""
    data, K = corpus.prose_like(64 << 10, 0xF5), 1024
    ordered, plain = _pair(monkeypatch, data, neighbours_per_step=K, seed=77, accept="single")
    ordered.seed_greedy(); plain.seed_greedy()
    _steps(ordered, plain, 40, "single")
    _same_end(ordered, plain, "single")
    _check_order(ordered, K, 1, "single")
    ordered.set_accept_mode("auto"); plain.set_accept_mode("auto")
    _steps(ordered, plain, 8, "auto")
    _same_end(ordered, plain, "auto")
    _check_order(ordered, K, 1, "auto")
    _check_adversarial(ordered, K, 1, "single")
    _close(ordered, plain)


def test_single_slice_hint(monkeypatch):
    grown = _check_hint(monkeypatch, corpus.prose_like(64 << 10, 0xF5), 1024, greedy=True, auto_steps=8, seed=77)
    assert grown > 0  # both classes were there to be told apart


@pytest.mark.parametrize("halves,K", [(2, 2048), (3, 2050)], ids=["two_slices", "three_slices_K2050"])
def test_slices_above_1mib(monkeypatch, halves, K):
    """j_base > 0 behind the first slice; K = 2 050 is not divisible by three"""
    data = corpus.prose_like(1280 << 10, 0xF6)
    ordered, plain = _pair(monkeypatch, data, env=[("MGL_HALVES", str(halves))], neighbours_per_step=K, seed=78, accept="single")
    ordered.seed_greedy(); plain.seed_greedy()
    _steps(ordered, plain, 12, halves)
    _same_end(ordered, plain, halves)
    hint = _check_order(ordered, K, halves, halves)
    assert 0 < np.count_nonzero(hint) < K
    _check_adversarial(ordered, K, halves, halves)
    _close(ordered, plain)


@pytest.mark.parametrize("halves,K", [(2, 2048), (3, 2050)], ids=["two_slices", "three_slices_K2050"])
def test_slices_above_1mib_hint(monkeypatch, halves, K):
    grown = _check_hint(monkeypatch, corpus.prose_like(1280 << 10, 0xF6), K, env=[("MGL_HALVES", str(halves))], greedy=True, seed=78)
    assert grown > 0


def test_hand_over_to_second_pass(monkeypatch):
    """c1's shape with first-pass lists of 32 events: hand-overs to the second pass and continuation records under the new mapping"""
    data, K = corpus.lorem(4096), 1024
    ordered, plain = _pair(monkeypatch, data, neighbours_per_step=K, seed=79, accept="single")
    ordered.debug_set(binding.KEY.LIST_CAP, 32); plain.debug_set(binding.KEY.LIST_CAP, 32)
    tot = _steps(ordered, plain, 12, "small_lists")
    for t in tot:
        assert t["second_pass_neighbours"] > 0 and t["fallback_neighbours"] == 0, t
    _same_end(ordered, plain, "small_lists")
    _check_order(ordered, K, 1, "small_lists")
    _close(ordered, plain)


def test_hand_over_to_second_pass_hint(monkeypatch):
    _check_hint(monkeypatch, corpus.lorem(4096), 1024, setup=lambda c: c.debug_set(binding.KEY.LIST_CAP, 32), seed=79)


@pytest.mark.parametrize("n", [1, 2, 3, 65])
def test_edges_of_the_input(monkeypatch, n):
    """`target + 1 == n`; slices shorter than a wavefront (K = 64, and fewer packets than neighbours)"""
    data, K = corpus.lorem(4096)[:n], 64
    ordered, plain = _pair(monkeypatch, data, neighbours_per_step=K, seed=80, accept="single")
    _steps(ordered, plain, 5, n)
    _same_end(ordered, plain, n)
    _check_order(ordered, K, 1, n)
    _check_adversarial(ordered, K, 1, n)
    _close(ordered, plain)
    _check_hint(monkeypatch, data, K, seed=80)


def test_position_targets(monkeypatch):
    """MGL_F_POSITION_TARGETS: no targets kernel, hence no hint and a null order -- the launch keeps blockIdx order and gives what the
    two-launch form gives"""
    data, K = corpus.prose_like(64 << 10, 0xF5), 1024
    kw = dict(neighbours_per_step=K, seed=82, accept="single", flags=binding.F_POSITION_TARGETS)
    _env(monkeypatch, [])
    fused = binding.SA(data, **kw)
    monkeypatch.setenv("MGL_NO_FUSE", "1")
    split = binding.SA(data, **kw)
    monkeypatch.delenv("MGL_NO_FUSE")
    assert len(fused.debug_dump(binding.DUMP.PICK_HINTS)) == 0 and len(fused.debug_dump(binding.DUMP.PICK_ORDER)) == 0
    with pytest.raises(binding.MglError):
        fused.debug_set(binding.KEY.PICK_HINTS, 0)
    fused.seed_greedy(); split.seed_greedy()
    _steps(fused, split, 8, "position")
    _same_end(fused, split, "position")
    _close(fused, split)
