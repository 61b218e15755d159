"""The handle's best-slab state under sequences of operations.

Where the best slab lives depends on Control::best_is_current, SnapMeta::valid of the two snapshots, mgl_sa::best_unverified
and the bulk_was_best / bulk_need_undo pair of a bulk step, and a dozen entry points read or flip
them.  Here one sequence of operations (tests/_handle_ops.py: runs, accept modes, temperatures, epochs, slabs set and
refused, best slabs set, refused and crossed, observers, focus, weights) goes, operation by operation, to

  S  the subject: a default handle (snapshots, lazy best, in-place accepts, batch accept),
  P  the plain witness: no snapshots, created under MGL_NO_BATCH and MGL_NO_INCREMENTAL_APPLY, so every accept is a rebuild and
     the best slab always has its own copy; never in MGL_ACCEPT_AUTO, it replays the modes S chose,
  F  the full-walk engine without snapshots, where the sequence holds single steps only,
  C  a second subject that cuts every run(n) into n run(1),

and after EVERY operation S must agree with each witness on the operation's result (return code; steps, evaluations,
failed, accepted, improved, current and best cost, packets, bulk steps), on current() and best() entry for entry and at
their costs, and on focus(), target_weights() and live_weights().  The base structures of S and P (canonical_base) are
compared after every operation that can change the base (run, begin_epoch, set_slab, seed_greedy) and after every
fifth other one.  Without any witness: the host's cost map of the best and of the current slab totals their costs and
both are valid parses by the rule of tests/_validity.py (a best slab the test knows to copy wrong bytes excepted, until
the epoch that starts from it refuses it with MGL_EINVAL and forgets it); the best cost moves only as the header says
(across a run: to the minimum of itself and the costs of the steps that took moves, from C's per-step results); an epoch
from a verified best slab starts at exactly that slab and cost; the live cost map of S equals the host's map.  Every
comparison is of integers and exact.

The scripted tour is also replayed by the CPU oracle from the slabs and costs the test tracks itself -- the reference
that shares no code with the handle.  The oracle has neither target weights nor a focus window, so the tour's runs
under those (the two searches under windows in front of its crossings, and its end) are held by P and C alone, and the
tracked slabs are taken from the handles there.

mgl_sa_create snapshots the all-literal base (first_build) and nothing clears that snapshot, so "begin_epoch(.., 0) with the
literal snapshot not yet made" cannot occur on a handle with snapshots: that half of the transition list is left out.

The last test asserts that every transition of _handle_ops.TRANSITIONS was met over the file.  `-m gpu`."""
import pytest

import _handle_ops as H
from _libs import Oracle, use_block_shift
from megalania_amd import corpus

pytestmark = pytest.mark.gpu

_BASE = corpus.enwik_like(6000, 0x71)
DATA = _BASE + _BASE[1000:3277]  # the 8 277 bytes of tests/test_gpu_focus.py: long matches, not a multiple of 64
SEEDS = [11, 12, 13, 14, 15, 16]
SINGLE = [(21, 8), (22, 8), (23, 8), (21, 256), (22, 256), (23, 256)]
EXPECTED_CASES = 1 + len(SEEDS) + len(SINGLE) + 2 + 2


def play(rig, ops, case):
    try:
        for op in ops:
            rig.step(op)
    finally:
        rig.close()
    H.CASES.add(case)


def test_scripted_tour(monkeypatch):
    """corpus.lorem(1800), K = 48, epochs of 12 steps: the trajectory test's size, where the oracle is fast"""
    data = corpus.lorem(1800)
    before = dict(H.MET)
    rig = H.Rig(monkeypatch, data, H.TOUR_K, H.TOUR_IPE, H.TOUR_SEED, oracle=Oracle(data, dict_limit=H.DICT))
    play(rig, H.tour(), "tour")
    missing = [t for t in H.TRANSITIONS if H.MET[t] == before.get(t, 0)]
    print("scripted tour:", {t: H.MET[t] - before.get(t, 0) for t in H.TRANSITIONS})
    assert not missing, missing


@pytest.mark.parametrize("seed", SEEDS)
def test_random_sequences(seed, monkeypatch):
    """40 operations on the 8 277-byte input, K = 64, epochs of 12 steps (the transition draw stays generous: steps go
    uphill and leave the best slab); even seeds start from the parse liblzma makes, odd ones from the all-literal slab"""
    K = 64
    rig = H.Rig(monkeypatch, DATA, K, 12 * K, 1000 + seed)
    ops = ([("set_slab", "xz")] if seed % 2 == 0 else []) + H.gen_sequence(seed, 40, len(DATA))
    play(rig, ops, ("random", seed))


@pytest.mark.parametrize("seed,K", SINGLE)
def test_random_sequences_single_only(seed, K, monkeypatch):
    """single steps only, so the full-walk engine is a witness too: corpus.lorem(600)"""
    data = corpus.lorem(600)
    rig = H.Rig(monkeypatch, data, K, 12 * K, 2000 + seed, witnesses=("F", "P", "C"), accept="single")
    play(rig, H.gen_sequence(seed, 40, len(data), single_only=True), ("single", seed, K))


@pytest.mark.parametrize("props,seed", [((3, 0, 2), 31), ((0, 4, 2), 32)], ids=["lc3-lp0-pb2", "lc0-lp4-pb2"])
def test_random_sequences_props(props, seed, monkeypatch):
    """the host cost map checks under the handle's own triple"""
    K = 64
    rig = H.Rig(monkeypatch, DATA[:3001], K, 12 * K, 3000 + seed, props=props)
    play(rig, H.gen_sequence(seed, 40, 3001), ("props", props))


@pytest.mark.parametrize("shift", [9, 10])
def test_block_shifts(shift, monkeypatch):
    """the scripted tour's operations at blocks of 512 and 1 024 positions, one position into the fifth (third) block"""
    use_block_shift(monkeypatch, shift)
    data = corpus.config_input("c2", 2049)[0]
    rig = H.Rig(monkeypatch, data, H.TOUR_K, H.TOUR_IPE, H.TOUR_SEED)
    play(rig, H.tour(), ("shift", shift))


def test_zz_every_transition_was_met():
    """the cases above must have taken every transition between them (runs last: pytest keeps file order)"""
    width = max(len(t) for t in H.TRANSITIONS)
    for t in H.TRANSITIONS:
        print(f"{t:<{width}}  {H.MET[t]}")
    if len(H.CASES) < EXPECTED_CASES:  # only part of the file ran
        return
    missing = [t for t in H.TRANSITIONS if H.MET[t] == 0]
    assert not missing, missing
