"""The device from random valid parses with stale entries (tests/_random_parse.py): walks, base structures, every
neighbour of a step on both engines, top-K in odd walk states, trajectories, in-place accepts and the consumers of the
current slab, each against the CPU oracle by exact integer equality.  Every other slab this suite hands the device was made
by a search or a parser of the project -- cheap parses over literals --; these hold LONG_REP 2 and 3, length-2 matches near
and far, chains of SHORT_REP, ctx_state 8 / 9 / 11 in front of every packet type, and matches and reps under the packets of
the walk, which a repair reads when a move uncovers them.  tests/test_oracle_vs_ref.py holds the oracle to the compiled
reference from such starts; tests/test_random_parse_cpu.py says what the bases contain.  `-m gpu`."""
import functools
import lzma

import numpy as np
import pytest

import _random_parse as rp
from _libs import LITERAL, LONG_REP, MATCH, SHORT_REP, Oracle, assert_same_base, canonical_base, literal_slab, walk
from megalania_amd import binding
from megalania_amd.binding import PROPS_TRIPLES
from test_gpu_incremental import check_base

pytestmark = pytest.mark.gpu

WIN_DROPPED = 0xFFFFFFFE  # csrc/mgl_device.h: MGL_WIN_DROPPED
BASES = pytest.mark.parametrize("name", rp.BASES)
# (base, lc/lp/pb): every base at 0/0/0, one under 2/1/2, one whose handle, oracle and generator share a 300-byte window
VARIANTS = [(b, False) for b in rp.BASES] + [("enwik4k", True), ("enwik4k_dict300", False)]
VARIANT_IDS = [b + ("-lc2lp1pb2" if alt else "") for b, alt in VARIANTS]


def P(slab):
    return np.ascontiguousarray(slab).astype(binding.PACKET)


def as_list(pk):
    return [(int(t), int(d), int(l)) for t, d, l in zip(pk["type"], pk["dist"], pk["len"])]


def tup(pk):
    return int(pk["type"]), int(pk["dist"]), int(pk["len"])


def _oracle(name, alt=False):
    return Oracle(rp.base(name)[0], dict_limit=rp.dict_limit_of(name), **(rp.ALT_PROPS if alt else {}))


def _sa(name, alt=False, **kw):
    return binding.SA(rp.base(name)[0], dict_limit=rp.dict_limit_of(name), **(rp.ALT_PROPS if alt else {}), **kw)


# ------------------------------------------------------------------------------------------------ 1. the walk
@pytest.mark.parametrize("alt", [False, True], ids=["lc0lp0pb0", "lc2lp1pb2"])
@pytest.mark.parametrize("name", list(rp._SPECS))
def test_walk_cost_and_final_state(name, alt):
    """mgl_cost_slab (total, packets, every running total) and mgl_final_state (probabilities, ctx_state, rep distances)"""
    data, slab = rp.base(name)
    want = _oracle(name, alt).cost_slab(slab, want_probs=True)
    sa = _sa(name, alt, neighbours_per_step=8)
    got = sa.cost_slab(P(slab))
    assert got["total"] == want["total"] and got["npackets"] == len(want["cum"]) == len(walk(slab))
    assert (got["cum"] == want["cum"]).all(), np.nonzero(got["cum"] != want["cum"])[0][:5]
    fs = sa.final_state(P(slab))
    assert fs["ctx_state"] == want["ctx_state"] and (fs["dists"] == want["dists"]).all()
    assert (fs["probs"] == want["probs"]).all(), np.nonzero(fs["probs"] != want["probs"])[0][:5]
    sa.close()


def test_props_sweep_equals_75_oracle_walks():
    data, slab = rp.base("two_periods")
    sa = _sa("two_periods", neighbours_per_step=8)
    got, _ = sa.props_sweep(P(slab))
    want = [Oracle(data, lc, lp, pb).cost_slab(slab)["total"] for lc, lp, pb in PROPS_TRIPLES]
    assert [int(c) for c in got] == want
    sa.close()


# ------------------------------------------------------------------------------------------------ 2. base structures
@pytest.mark.parametrize("serial_build", [False, True], ids=["parallel_build", "serial_build"])
@pytest.mark.parametrize("name,alt", [(b, False) for b in rp.BASES] + [("doubled", True)],
                         ids=rp.BASES + ["doubled-lc2lp1pb2"])
def test_base_structures_match_oracle_trace(name, alt, serial_build):
    """bitmaps, special-state records, dense checkpoints and per-context chains after mgl_sa_set_slab against the oracle's
    event trace -- under lc = 2, lp = 1 as well, where the literal coder is 8 times the size and the chains are laid out
    behind it"""
    data, slab = rp.base(name)
    sa = _sa(name, alt, accept="single", neighbours_per_step=8, serial_build=serial_build)
    sa.set_slab(P(slab))
    check_base(sa, _oracle(name, alt), slab, data)
    sa.close()


# ------------------------------------------------------------------------------------------------ 3. every neighbour
@pytest.mark.parametrize("fullwalk", [False, True], ids=["incremental", "fullwalk"])
@pytest.mark.parametrize("name,alt", VARIANTS, ids=VARIANT_IDS)
def test_every_neighbour_vs_oracle(name, alt, fullwalk):
    """Steps 0 and 5 of K = 128 neighbours: cost, journal, window (target, end, soft end, dep) and status of each equal the
    oracle's.  The device marks a dropped neighbour (MGL_WIN_DROPPED) without saying which capacity it ran over; the oracle
    says, so the counts per rule are the device's dropped neighbours under the oracle's reasons.  They are non-zero where
    tests/test_random_parse_cpu.py::test_every_drop_rule_fires says: repair picks on `doubled`, the journal on
    `two_periods`, journal, walk length and event lists on `one_period`."""
    data, slab = rp.base(name)
    sa = _sa(name, alt, accept="single", neighbours_per_step=rp.K, seed=rp.SEED, fullwalk=fullwalk)
    sa.set_slab(P(slab))
    bad, got_rows, want_rows = [], [], []
    for step in rp.STEPS:
        costs, nd, diffs = sa.neighbours(step)
        win = sa.debug_dump(binding.DUMP.WINDOWS).reshape(-1, 2)
        win2 = sa.debug_dump(binding.DUMP.SOFT_ENDS)
        for j, (st, cost, od, w, reason) in enumerate(rp.oracle_neighbours(name, step, alt)):
            got_st = 1 if int(costs[j]) != binding.INVALID_COST else -1 if int(win[j, 1]) == WIN_DROPPED else 0
            got_rows.append((got_st, 0, 0, 0, reason))
            want_rows.append((st, 0, 0, 0, reason))
            if got_st != st or int(costs[j]) != cost or int(win[j, 0]) != w[0]:
                bad.append((step, j, "status/cost/target", got_st, int(costs[j]), int(win[j, 0]), st, cost, w))
                continue
            if st != 1:
                continue
            got_w = (int(win[j, 0]), int(win[j, 1]), int(win2[j]) & 0x7FFFFFFF, int(win2[j]) >> 31)
            got_d = [(int(d["position"]), tup(d["old"]), tup(d["new"])) for d in diffs[j][: nd[j]]]
            want_d = [(int(d["position"]), tup(d["old"]), tup(d["new"])) for d in od]
            if got_w != w or got_d != want_d:
                bad.append((step, j, "window/journal", got_w, w, got_d, want_d))
    sa.close()
    assert not bad, (len(bad), bad[:3])
    got, want = rp.drop_counts(got_rows), rp.drop_counts(want_rows)
    print(f"{name}{' 2/1/2' if alt else ''} {'fullwalk' if fullwalk else 'incremental'}: dropped per rule {got}")
    assert got == want
    if not alt:
        assert got["repair_picks"] >= 1 or name != "doubled"
        assert got["journal"] >= 1 or name not in ("two_periods", "one_period")
        assert (got["walk"] >= 1 and got["events"] >= 1) or name != "one_period"


# ------------------------------------------------------------------------------------------------ 4. top-K in odd states
def _behind(slab, what, limit):
    w = walk(slab)
    n = len(slab)
    out = [p + int(slab[p]["len"]) for p in w if what(int(slab[p]["type"]), int(slab[p]["dist"]), int(slab[p]["len"]))]
    out = [p for p in out if p < n - 1]
    return out[:: max(1, len(out) // limit)][:limit]


@BASES
def test_top_k_in_odd_walk_states(name):
    """mgl_top_k == the oracle's canonical list at 16 positions of the walk: behind a LONG_REP 3 (the rep distances rotated
    all the way), behind a SHORT_REP, behind a length-2 match, behind a LONG_REP 2 where the walk has one, and spread over
    the rest"""
    data, slab = rp.base(name)
    pos = set()
    for what, needed in ((lambda t, d, l: t == LONG_REP and d == 3, True), (lambda t, d, l: t == SHORT_REP, True),
                         (lambda t, d, l: t == MATCH and l == 2, True), (lambda t, d, l: t == LONG_REP and d == 2, False)):
        found = _behind(slab, what, 3)
        assert found or not needed, name
        pos.update(found)
    w = walk(slab)
    for p in w[1:: max(1, len(w) // 16)]:
        if len(pos) < 16:
            pos.add(p)
    assert len(pos) == 16
    sa = _sa(name, neighbours_per_step=8)
    o = _oracle(name)
    for p in sorted(pos):
        pk, costs = sa.top_k(P(slab), p)
        opk, ocosts = o.top_k(slab.copy(), p, mode=1, k=20)
        assert as_list(pk) == as_list(opk) and [int(c) for c in costs] == [int(c) for c in ocosts], (name, p)
    sa.close()


# ------------------------------------------------------------------------------------------------ 5. trajectories
def _shape(name):
    """(K, steps): the oracle needs 6 ms for a neighbour of `one_period` (every one walks to the end of the input)"""
    return (48, 10) if name == "one_period" else (96, 40)


class OracleChain:
    """orc_sa_batched from a base with cur = 0 (= the base's own cost), one step per call"""

    def __init__(self, name):
        data, slab = rp.base(name)
        self.K, self.steps = _shape(name)
        self.o = _oracle(name)
        self.slab, self.best = slab.copy(), literal_slab(len(data))
        self.cur = self.best_cost = self.s = 0
        self.rows = []

    def step(self, mode):
        r = self.o.sa_batched(self.slab, self.best, self.cur, self.best_cost, rp.SEED, self.K, 0, self.steps * self.K, self.s,
                              self.s + 1, iter0=self.s * self.K, modes=[mode])
        self.cur, self.best_cost, self.s = r["cur"], r["best"], self.s + 1
        self.rows.append((r["cur"], int(r["trace"][0, 1]), r["valid"], r["dropped"]))
        return self.rows[-1]


@functools.lru_cache(maxsize=None)
def oracle_chain(name, mode):
    """the whole single (0) or bulk (1) trajectory of a base, shared by the tests that follow it"""
    before = Oracle.lib().orc_bulk_rollbacks(), Oracle.lib().orc_bulk_overlaps()
    ch = OracleChain(name)
    for _ in range(ch.steps):
        ch.step(mode)
    assert (Oracle.lib().orc_bulk_rollbacks(), Oracle.lib().orc_bulk_overlaps()) == before
    return ch


def _device_chain(name, accept):
    K, steps = _shape(name)
    sa = _sa(name, accept=accept, bulk_threshold=6, neighbours_per_step=K, seed=rp.SEED, iters_per_epoch=steps * K)
    sa.set_slab(P(rp.base(name)[1]))
    return sa, steps


@pytest.mark.parametrize("accept", ["single", "bulk", "auto"])
@BASES
def test_trajectory_vs_oracle(name, accept):
    """mgl_sa_run from the base against orc_sa_batched from the same slab: per step the current cost, the moves taken, the
    evaluations and the dropped neighbours; at the end the current and best slabs as whole arrays, stale entries and what the
    moves left behind included.  `auto` is replayed with the modes the library chose."""
    sa, steps = _device_chain(name, accept)
    ch = OracleChain(name) if accept == "auto" else oracle_chain(name, accept == "bulk")
    most = 0
    for s in range(steps):
        st = sa.run(1)
        want = ch.step(int(sa.step_modes()[0])) if accept == "auto" else ch.rows[s]
        assert (st["current_cost"], st["accepted"], st["evaluations"], st["dropped_neighbours"]) == want, (name, s)
        assert st["bulk_rollbacks"] == 0 and st["bulk_double_writes"] == 0, (name, s)
        most = max(most, st["accepted"])
    assert most > 1 or accept != "bulk"
    cur, cur_cost = sa.current()
    bst, best_cost = sa.best()
    assert cur_cost == ch.cur and best_cost == ch.best_cost
    assert as_list(cur) == as_list(ch.slab), np.nonzero(P(ch.slab) != cur)[0][:5]
    assert as_list(bst) == as_list(ch.best), np.nonzero(P(ch.best) != bst)[0][:5]
    assert lzma.decompress(binding.emit_stream(rp.base(name)[0], bst), format=lzma.FORMAT_ALONE) == rp.base(name)[0]
    sa.close()


# ------------------------------------------------------------------------------------------------ 6. accepts patch old structures
@pytest.mark.parametrize("accept", ["single", "bulk"])
@pytest.mark.parametrize("name", ["two_periods", "doubled"])
def test_accepts_patch_structures_built_from_the_base(name, accept, monkeypatch):
    """The in-place accepts (single; bulk through the batch path) patch chains, bitmaps, state records and checkpoints that
    were built from a parse full of reps, not grown from the literal slab: after every accepted step among the first 25 they
    equal a rebuild from the slab on a second handle, the cost is the oracle's walk, and a bulk chain with the batch path off
    (MGL_NO_BATCH: every bulk step a rebuild) walks the same trajectory."""
    data = rp.base(name)[0]
    inc, _ = _device_chain(name, accept)
    monkeypatch.setenv("MGL_NO_BATCH", "1")
    full, _ = _device_chain(name, accept)
    monkeypatch.delenv("MGL_NO_BATCH")
    ref = _sa(name, accept="single", neighbours_per_step=8)
    o, ch = _oracle(name), oracle_chain(name, accept == "bulk")
    accepted = 0
    for s in range(25):
        st, sf = inc.run(1), full.run(1)
        assert st["current_cost"] == sf["current_cost"] == ch.rows[s][0] and st["accepted"] == sf["accepted"] == ch.rows[s][1], (name, s)
        assert st["bulk_rollbacks"] == 0 and st["full_rebuilds"] == 0, (name, s)
        if st["accepted"]:
            accepted += 1
            cur, cost = inc.current()
            assert (cur == full.current()[0]).all(), (name, s)
            assert cost == o.cost_slab(cur.astype(literal_slab(1).dtype))["total"], (name, s)
            ref.set_slab(cur)
            assert_same_base(canonical_base(inc, cur), canonical_base(ref, cur), (name, accept, s))
    assert accepted >= 10
    if accept == "bulk":
        assert inc.batch_counters()[0] >= 3 and full.batch_counters() == (0, 0)
    inc.close(); full.close(); ref.close()


# ------------------------------------------------------------------------------------------------ 7. consumers of the current slab
def test_adaptive_pass_from_a_random_parse():
    """mgl_adaptive_pass prices its chunks from the model that parse_in leaves at their starts: here the model of a parse
    that is mostly reps, which no search of the project would produce"""
    from test_adaptive_rule_cpu import adaptive_rule
    data, slab = rp.base("doubled")
    sa = _sa("doubled", accept="single", neighbours_per_step=16)
    got, obj = sa.adaptive_pass(P(slab), 16, 1000, 64, 128)
    want, want_obj, _ = adaptive_rule(data, slab, 16, 1000, 64, 128)
    assert as_list(got) == want and obj == want_obj
    sa.close()


@BASES
def test_reparse_from_a_random_parse(name):
    """mgl_sa_seed_adaptive(from_current) after mgl_sa_set_slab(base): whatever it leaves costs what the oracle says, is no
    dearer than the base, and decodes"""
    data, slab = rp.base(name)
    sa = _sa(name, accept="single", neighbours_per_step=16)
    sa.set_slab(P(slab))
    base_cost = _oracle(name).cost_slab(slab)["total"]
    assert sa.current()[1] == base_cost
    st = sa.seed_adaptive(passes=1, from_current=True)
    cur, cost = sa.current()
    assert st["greedy_cost"] == base_cost and cost <= base_cost
    assert cost == _oracle(name).cost_slab(cur.astype(literal_slab(1).dtype))["total"]
    assert lzma.decompress(binding.emit_stream(data, cur), format=lzma.FORMAT_ALONE) == data
    sa.close()
