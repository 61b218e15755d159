"""Operations on an mgl_sa handle as data, the rig that applies one sequence of them to several handles at once, and the
bookkeeping of which transitions of the handle's best-slab state a sequence met.  Test infrastructure only: used by
tests/test_gpu_handle_states.py (on the device) and tests/test_handle_ops_cpu.py (generator, slabs and model, no device).

An operation is a tuple, ("run", 3), ("epoch", 1, True), ("set_slab", "xz") ...; `apply_op` turns one into calls on one handle
and returns what the caller can see of it, a refusal as ("refused", rc).  Slabs are named: the rig's pool holds the
all-literal slab, the parse liblzma makes, the device's greedy parse, the handle's own earlier current / best slabs
("saved_cur", "saved_best": replaced by every ("save",); "own_cur" / "own_best": what the handle holds at the time), and the
slabs made from them that must be refused.

`Rig` owns the handles: S the subject (default handle), and the witnesses P (no snapshots, every accept a rebuild, never in
MGL_ACCEPT_AUTO: it replays the modes S chose), F (the full-walk engine; single steps only) and C (a second subject that
cuts every run(n) into n run(1)).  `Rig.step` applies one operation to all of them and asserts everything the handles
must agree on, the invariants that need no witness (host cost map, the validity rule, how the best cost may move), and
-- with a `Model` -- the CPU oracle's replay of every run.

`Model` is the contract restated with the CPU oracle for the search: current and best slab, their costs, step and
iteration counters.  Next to them it follows the four pieces of state the handle keeps about where the best slab lives
(DESIGN.md section 7), from what the calls return (per-step accepted / improved of C, the modes, the batch counters,
`adopted`, return codes), only to name the transition an operation took: MET counts them."""
from __future__ import annotations

import collections
import hashlib
import lzma

import numpy as np

from _libs import LITERAL, MATCH, literal_slab, walk
from _validity import BYTES_DIFFER, violations
from megalania_amd import binding

EINVAL = -1
DICT = 0x400000
STAT_FIELDS = ("steps", "evaluations", "failed", "accepted", "improved", "current_cost", "best_cost", "packets", "bulk_steps")
SUMMED = ("steps", "evaluations", "failed", "accepted", "improved", "bulk_steps")
MODES = {"single": 0, "bulk": 1}

# every transition the file must have met (tests/test_gpu_handle_states.py::test_zz_every_transition_was_met)
TRANSITIONS = (
    "single step leaves the best slab", "single step sets a new best", "single step takes nothing",
    "bulk step leaves the best slab: batch accept", "bulk step leaves the best slab: rebuild behind a forced give-up",
    "bulk step sets a new best", "bulk step takes nothing",
    "epoch from best: the base is the best slab", "epoch from best: valid snapshot",
    "epoch from best: snapshot invalid after a bulk step", "epoch from best: snapshot invalid after set_best",
    "epoch from best: no snapshot made yet",
    "epoch from best: unverified good best", "epoch from best: unverified bad best refused", "epoch from best: no best yet",
    "epoch from literal: snapshot valid",
    "set_slab(valid) while the base holds the best slab", "set_slab(invalid) while the base holds the best slab",
    "seed_greedy while the base holds the best slab",
    "set_best while the base holds the best slab",
    "cross_best adopted 0", "cross_best adopted 1", "cross_best adopted 2", "cross_best while the base holds the best slab",
    "auto block cut by set_slab", "auto block cut by begin_epoch", "auto block cut by the end of a run",
    "live weights refreshed because set_slab left them stale",
)
MET = collections.Counter()
CASES = set()  # the cases of tests/test_gpu_handle_states.py that ran to their end


# ---- slabs
def P(slab):
    return np.ascontiguousarray(slab).astype(binding.PACKET)


def same(a, b):
    return all((a[f] == b[f]).all() for f in ("type", "dist", "len"))  # field by field: the records have padding


def key(slab):
    return hashlib.sha1(np.concatenate([slab["type"].astype(np.uint32), slab["dist"], slab["len"].astype(np.uint32)]).tobytes()).digest()


def xz_parse(data, props=(0, 0, 0)):
    stream = lzma.compress(data, format=lzma.FORMAT_ALONE,
                           filters=[dict(id=lzma.FILTER_LZMA1, preset=6, dict_size=1 << 22, lc=props[0], lp=props[1], pb=props[2])])
    return P(binding.stream_import(stream, data)[0])


def zeroed_entry(slab):
    """`slab` with one entry on its walk zeroed: no packet, every gate refuses it"""
    bad = slab.copy()
    bad[walk(slab)[5]] = (0, 0, 0)
    return bad


def wrong_bytes(data, slab):
    """`slab` with two literals of its walk replaced by a MATCH of length 2 whose source holds another byte: every entry is
    a packet and the walk has a cost, but the copy does not reproduce the input (the BYTES_DIFFER cases of tests/_validity.py)"""
    starts = walk(slab)
    on = np.zeros(len(slab) + 1, dtype=bool)
    on[starts] = True
    on[len(slab)] = True
    for p in starts:
        if p >= 8 and on[p + 1] and p + 2 <= len(slab) and on[p + 2] and slab[p]["type"] == LITERAL and slab[p + 1]["type"] == LITERAL \
                and data[p] != data[p - 1]:
            bad = slab.copy()
            bad[p] = (MATCH, 0, 2)
            return bad
    raise AssertionError("no pair of literals to plant a wrong copy on")


def host_total(data, slab, props):
    return binding.host_cost_map(data, slab, props)[1]["total"]


class Pool:
    """the named slabs of one rig; `greedy` needs a device, so the CPU checks leave it out"""

    def __init__(self, data, props=(0, 0, 0), greedy=None):
        self.data, self.props = data, props
        xz = xz_parse(data, props)
        self.slabs = {"literal": P(literal_slab(len(data))), "xz": xz, "saved_cur": xz, "saved_best": xz}
        if greedy is not None:
            self.slabs["greedy"] = P(greedy)
        self._cost, self._bad = {}, None

    def bad_bytes(self):
        if self._bad is None:
            self._bad = wrong_bytes(self.data, self.slabs["xz"])
        return self._bad

    def get(self, name):
        return self.slabs[name]

    def cost(self, name):
        s = self.slabs[name]
        k = key(s)
        if k not in self._cost:
            self._cost[k] = host_total(self.data, s, self.props)
        return self._cost[k]


# ---- the generator
def gen_sequence(seed, count, n, single_only=False, names=("literal", "xz", "greedy", "saved_cur", "saved_best")):
    """`count` operations drawn from np.random.default_rng(seed): a function of its arguments alone"""
    rng = np.random.default_rng(seed)
    kinds = ["run1", "runn", "temp", "epoch", "set_slab", "set_slab_bad", "seed_greedy", "set_best", "set_best_bad", "set_best_wrong_cost",
             "cross", "obs", "focus", "weights", "live", "save"] + ([] if single_only else ["mode"])
    weight = dict(run1=5, runn=6, temp=2, epoch=5, set_slab=3, set_slab_bad=1, seed_greedy=1, set_best=2, set_best_bad=1, set_best_wrong_cost=1,
                  cross=3, obs=3, focus=1, weights=1, live=1, save=2, mode=4)
    p = np.array([weight[k] for k in kinds], dtype=float)
    p /= p.sum()
    out = []
    pick = lambda seq: seq[int(rng.integers(len(seq)))]
    while len(out) < count:
        k = kinds[int(rng.choice(len(kinds), p=p))]
        if k == "run1":
            out.append(("run", 1))
        elif k == "runn":
            out.append(("run", int(rng.integers(2, 8))))
        elif k == "mode":
            out.append(("mode", pick(["single", "bulk", "auto", "auto"]), 6))
        elif k == "temp":
            out.append(("temp", pick([0, 0, 4 * 16384, 64 * 16384])))
        elif k == "epoch":
            out.append(("epoch", int(rng.integers(0, 3)), bool(rng.integers(0, 3))))  # two of three from the best slab
        elif k in ("set_slab", "set_slab_bad", "set_best", "set_best_wrong_cost"):
            out.append((k, pick(names)))
        elif k == "seed_greedy":
            out.append((k, pick([4, 8, 64])))
        elif k == "set_best_bad":
            out.append((k,))
        elif k == "cross":
            out.append((k, pick(list(names) + ["own_best"]), pick([0, 1, 16, 256])))
        elif k == "obs":
            out.append((k, pick(["cost_map_live", "cost_map", "best_packed", "slab_hash", "cost_slab", "neighbours"])))
        elif k == "focus":
            lo = int(rng.integers(0, n - 1))
            out.append(pick([("focus", lo, int(rng.integers(lo + 1, n + 1))), ("focus", 0, 0)]))
        elif k == "weights":
            out.append(("weights", pick([None, 0, 1, 40])))
        elif k == "live":
            out.append(pick([("live", None, 0, False), ("live", int(rng.integers(1, 6)), int(rng.integers(0, 3)), bool(rng.integers(0, 2)))]))
        elif k == "save":
            out.append(("save",))
    return out


# ---- one operation on one handle
def _arr(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def _cross(d):
    return tuple((k, tuple(v) if isinstance(v, list) else v) for k, v in sorted(d.items()) if k != "gpu_ms")


def _report(rep):
    return tuple((k, tuple(v) if isinstance(v, list) else v) for k, v in sorted(rep.items()) if k != "gpu_ms")


def apply_op(sa, pool, op, gstep=0):
    """what the caller sees of `op` on handle `sa` (everything but run and mode, which the rig treats per handle)"""
    kind = op[0]
    try:
        if kind == "temp":
            return sa.set_temperature(op[1])
        if kind == "epoch":
            return sa.begin_epoch(op[1], from_best=op[2])
        if kind == "set_slab":
            return sa.set_slab(pool.get(op[1]))
        if kind == "set_slab_bad":
            return sa.set_slab(zeroed_entry(pool.get(op[1])))
        if kind == "seed_greedy":
            return sa.seed_greedy(op[1])
        if kind == "set_best":
            return sa.set_best(pool.get(op[1]), pool.cost(op[1]))
        if kind == "set_best_wrong_cost":
            return sa.set_best(pool.get(op[1]), pool.cost(op[1]) + 1)
        if kind == "set_best_bad":
            bad = pool.bad_bytes()
            return sa.set_best(bad, sa.cost_slab(bad, want_cum=False)["total"])  # the device's own walk: the cost cannot refuse it
        if kind == "cross":
            other = sa.best()[0] if op[1] == "own_best" else sa.current()[0] if op[1] == "own_cur" else pool.get(op[1])
            return _cross(sa.cross_best(other, op[2]))
        if kind == "focus":
            return sa.set_focus(op[1], op[2])
        if kind == "weights":
            return sa.set_target_weights(None) if op[1] is None else sa.weight_targets_by_cost(op[1])[0]
        if kind == "live":
            return sa.set_live_weights(op[1], floor=op[2], single_only=op[3])
        if kind == "obs":
            what = op[1]
            if what == "cost_map_live":
                m, rep = sa.cost_map_live()
                return _arr(m), _report(rep)
            if what == "cost_map":
                m, rep = sa.cost_map()
                return _arr(m), _report(rep)
            if what == "best_packed":
                pk, cost = sa.best_packed()
                return _arr(pk), cost
            if what == "slab_hash":
                return sa.slab_hash(), sa.slab_hash(pool.get("xz"))
            if what == "cost_slab":
                r = sa.cost_slab(pool.get("xz"))
                return r["total"], r["npackets"], _arr(r["cum"])
            if what == "neighbours":
                return _arr(sa.neighbours(gstep, want_diffs=False)[0])
        raise AssertionError(op)
    except binding.MglError as e:
        return ("refused", e.rc)


OBSERVERS = ("obs",)
CHANGES_BASE = ("run", "epoch", "set_slab", "set_slab_bad", "seed_greedy")


def run_cut(sa, n):
    """run(1) n times: (summed stats, per-step stats, modes, per-step batch counters or None)"""
    steps, modes, batch = [], [], []
    for _ in range(n):
        b0 = sa.batch_counters()
        st = sa.run(1)
        b1 = sa.batch_counters()
        steps.append({f: st[f] for f in STAT_FIELDS})
        modes.append(int(sa.step_modes()[0]))
        batch.append((b1[0] - b0[0], b1[1] - b0[1]))
    return sum_stats(steps), steps, modes, batch


def sum_stats(steps):
    out = {f: sum(s[f] for s in steps) for f in SUMMED}
    out.update({f: steps[-1][f] for f in STAT_FIELDS if f not in SUMMED})
    return out


def run_modes(sa, modes):
    """the witness that is never in MGL_ACCEPT_AUTO: stretches of one mode, each under that mode"""
    parts, i = [], 0
    while i < len(modes):
        j = i
        while j < len(modes) and modes[j] == modes[i]:
            j += 1
        sa.set_accept_mode("bulk" if modes[i] else "single")
        st = sa.run(j - i)
        parts.append({f: st[f] for f in STAT_FIELDS})
        i = j
    return sum_stats(parts)


# ---- the model
class Model:
    """current / best slab and costs by the contract; the search by the CPU oracle (None: no replay, runs are adopted from
    the handles).  `bits`: where the implementation must be keeping the best slab, followed only to name transitions."""

    def __init__(self, data, K, ipe, seed, props=(0, 0, 0), oracle=None, counter=None):
        self.data, self.K, self.ipe, self.seed, self.props, self.oracle = data, K, ipe, seed, props, oracle
        self.counter = collections.Counter() if counter is None else counter  # (the device cases count in MET)
        n = len(data)
        self.cur, self.best = P(literal_slab(n)), P(literal_slab(n))
        self.cur_cost, self.best_cost = host_total(data, self.cur, props), 0
        self.gstep = self.iter = self.phase = self.temperature = 0
        self.mode, self.blk_done = "auto", 0
        self.weighted = self.live = False      # target weights / live weights in force: the oracle has neither
        self.focus = (0, 0)
        self.live_every = 0
        self.stale_by = None                   # who left the live weights stale
        # where the best slab lives
        self.base_is_best = False              # Control::best_is_current
        self.snap_valid = False                # SnapMeta::valid of snap_best
        self.unverified = False                # mgl_sa::best_unverified
        self.invalid_by = None                 # "bulk" / "set_best": who cleared a valid snap_best last (None: never made)
        self.best_is_bad = False               # the best slab came from set_best_bad (or is a child of it that kept the copy)

    def met(self, name):
        assert name in TRANSITIONS, name
        self.counter[name] += 1

    # -- set-up calls
    def _literal(self):
        self.cur = P(literal_slab(len(self.data)))
        self.cur_cost = host_total(self.data, self.cur, self.props)

    def _keep_best(self):
        if self.base_is_best:
            self.base_is_best, self.snap_valid = False, True

    def _cut_block(self, by):
        if self.mode == "auto" and self.blk_done:
            self.met(f"auto block cut by {by}")
        self.blk_done = 0

    def replace_current(self, slab, cost, how):
        if self.base_is_best:
            self.met(f"{how} while the base holds the best slab")
        self._keep_best()
        self._cut_block("set_slab")
        self.stale_by = "set_slab"
        if slab is None:
            self._literal()
        else:
            self.cur, self.cur_cost = P(slab), cost

    def begin_epoch(self, phase, from_best):
        """returns the rc the handle must give"""
        self._cut_block("begin_epoch")
        self.stale_by = "begin_epoch"
        self.iter, self.phase = 0, phase
        if from_best and self.best_cost == 0:
            self.met("epoch from best: no best yet")
            from_best = False
        if not from_best:
            self._keep_best()
            self.met("epoch from literal: snapshot valid")
            self._literal()
            return None
        if self.base_is_best:
            self.met("epoch from best: the base is the best slab")
            return None
        if self.snap_valid:
            self.met("epoch from best: valid snapshot")
        else:
            self.met("epoch from best: " + {"bulk": "snapshot invalid after a bulk step", "set_best": "snapshot invalid after set_best",
                                            None: "no snapshot made yet"}[self.invalid_by])
            if self.unverified and self.best_is_bad:
                self.met("epoch from best: unverified bad best refused")
                self.best, self.best_cost = P(literal_slab(len(self.data))), 0
                self.unverified = self.best_is_bad = self.snap_valid = False
                self.invalid_by = None
                self._literal()
                return EINVAL
            if self.unverified:
                self.met("epoch from best: unverified good best")
            self.unverified, self.snap_valid = False, True
        self.cur, self.cur_cost = self.best.copy(), self.best_cost
        return None

    def new_best(self, slab, cost, bad=False):
        if self.base_is_best:
            self.met("set_best while the base holds the best slab")
        self.best, self.best_cost = P(slab), cost
        self.base_is_best, self.snap_valid, self.unverified, self.invalid_by, self.best_is_bad = False, False, True, "set_best", bad

    def crossed(self, adopted, slab, cost):
        self.met(f"cross_best adopted {adopted}")
        if self.base_is_best:
            self.met("cross_best while the base holds the best slab")
        if adopted:
            self.best, self.best_cost = P(slab), cost
            self.base_is_best, self.snap_valid, self.unverified, self.invalid_by = False, False, True, "set_best"
            self.best_is_bad = violations(self.data, self.best, DICT) != []

    # -- a run
    def can_replay(self):
        return self.oracle is not None and not self.weighted and not self.live and self.focus == (0, 0)

    def replay(self, modes):
        """the oracle's replay of a run of len(modes) steps: per-step (accepted, improved, cost)"""
        o = self.oracle
        o.set_temperature(self.temperature)
        steps = []
        self.cur, self.best = self.cur.copy(), self.best.copy()  # the oracle writes in place
        for s, m in enumerate(modes):
            before = self.best_cost
            r = o.sa_batched(self.cur, self.best, self.cur_cost, self.best_cost, self.seed, self.K, self.phase, self.ipe,
                             self.gstep + s, self.gstep + s + 1, iter0=self.iter + s * self.K, modes=np.array([m], dtype=np.uint8))
            self.cur_cost, self.best_cost = r["cur"], r["best"]
            steps.append(dict(accepted=int(r["trace"][0, 1]), improved=int(self.best_cost != before), current_cost=r["cur"], evaluations=r["valid"]))
        return steps

    def ran(self, steps, modes, batch, live_rose_first):
        """per-step (accepted, improved) of a run that is over: the transitions, the counters, the block"""
        if self.mode == "auto" and self.blk_done:
            self.met("auto block cut by the end of a run")
        if self.live and self.stale_by == "set_slab" and live_rose_first and self.gstep % self.live_every:
            self.met("live weights refreshed because set_slab left them stale")
        if self.live:
            self.stale_by = None
        for st, m, b in zip(steps, modes, batch):
            route = "bulk" if m else "single"
            if st["accepted"] == 0:
                self.met(f"{route} step takes nothing")
            elif st["improved"]:
                self.met(f"{route} step sets a new best")
                self.base_is_best, self.best_is_bad, self.unverified = True, False, False
                if not self.snap_valid:
                    self.invalid_by = None  # (of this best slab no snapshot was made)
            elif self.base_is_best:
                self.base_is_best = False
                if not m:
                    self.met("single step leaves the best slab")
                    self.snap_valid = True
                else:
                    if self.snap_valid:  # (else there is nothing for k_bulk_finish to clear)
                        self.snap_valid, self.invalid_by = False, "bulk"
                    if b is not None and b[0]:
                        self.met("bulk step leaves the best slab: batch accept")
                    elif b is not None and b[1]:
                        self.met("bulk step leaves the best slab: rebuild behind a forced give-up")
            if self.mode == "auto":
                self.blk_done = (self.blk_done + 1) % (4 if m else 16)
        self.gstep += len(steps)
        self.iter += len(steps) * self.K


# ---- the rig
class Rig:
    """S and its witnesses over one input; step(op) applies one operation to all and asserts.  base_every: canonical_base of
    S against P after every operation that can change the base, and after every `base_every`-th other one."""

    def __init__(self, monkeypatch, data, K, ipe, seed, props=(0, 0, 0), witnesses=("P", "C"), oracle=None, accept=None, base_every=5):
        from _libs import assert_same_base, canonical_base
        self._canon, self._same_base = canonical_base, assert_same_base
        self.data, self.K, self.props, self.n = data, K, props, len(data)
        kw = dict(neighbours_per_step=K, seed=seed, iters_per_epoch=ipe, lc=props[0], lp=props[1], pb=props[2], accept=accept)
        assert "C" in witnesses  # its per-step results are what the best-cost rule and the transitions are read from
        self.h = {"S": binding.SA(data, **kw), "C": binding.SA(data, **kw)}
        if "P" in witnesses:
            monkeypatch.setenv("MGL_NO_BATCH", "1")
            monkeypatch.setenv("MGL_NO_INCREMENTAL_APPLY", "1")
            self.h["P"] = binding.SA(data, snapshots=False, **dict(kw, accept=accept or "single"))
            monkeypatch.delenv("MGL_NO_BATCH")
            monkeypatch.delenv("MGL_NO_INCREMENTAL_APPLY")
        if "F" in witnesses:
            assert accept == "single"
            self.h["F"] = binding.SA(data, fullwalk=True, snapshots=False, **kw)
        tmp = binding.SA(data, **kw)
        tmp.seed_greedy(8)
        self.pool = Pool(data, props, greedy=tmp.current()[0])
        tmp.close()
        self.model = Model(data, K, ipe, seed, props, oracle, counter=MET)
        self.model.mode = accept or "auto"
        self.base_every, self.others = base_every, 0
        self._checked = {}
        self.seen = self.observe("S")
        self.log = []

    def close(self):
        for sa in self.h.values():
            sa.close()

    # -- what a handle shows
    def observe(self, role):
        sa = self.h[role]
        cur, cur_cost = sa.current()
        bst, best_cost = sa.best()
        w, total, window = sa.target_weights()
        lw = sa.live_weights()
        return dict(cur=P(cur), cur_cost=cur_cost, best=P(bst), best_cost=best_cost, focus=sa.focus(), weights=(_arr(w), total, window),
                    live=tuple((k, v) for k, v in sorted(lw.items()) if k != "gpu_ms"))

    def _agree(self, a, b, what):
        assert a["cur_cost"] == b["cur_cost"] and a["best_cost"] == b["best_cost"], (what, "costs", a["cur_cost"], b["cur_cost"], a["best_cost"], b["best_cost"])
        for f in ("cur", "best"):
            if not same(a[f], b[f]):
                at = np.nonzero((a[f]["type"] != b[f]["type"]) | (a[f]["dist"] != b[f]["dist"]) | (a[f]["len"] != b[f]["len"]))[0]
                raise AssertionError((what, f, "entries differ at", at[:8].tolist()))
        for f in ("focus", "weights", "live"):
            assert a[f] == b[f], (what, f, a[f], b[f])

    def _valid_at(self, slab, cost, what):
        """host cost map total == cost and the validity rule, once per distinct slab"""
        k = key(slab)
        if k not in self._checked:
            v = violations(self.data, slab, DICT)
            self._checked[k] = (v, host_total(self.data, slab, self.props) if not v else None)
        v, total = self._checked[k]
        assert v == [], (what, v)
        assert total == cost, (what, total, cost)

    # -- one operation
    def step(self, op):
        m, S = self.model, self.h["S"]
        kind = op[0]
        tag = (len(self.log), op)
        self.log.append(op)
        prev = self.seen
        steps = modes = batch = None
        if kind == "save":
            if prev["best_cost"] and not m.best_is_bad:
                self.pool.slabs["saved_best"] = prev["best"]
            self.pool.slabs["saved_cur"] = prev["cur"]
            return None
        if kind == "force_batch_fail":  # the next batch accept gives up behind its commit (the subjects; P has no batch accept)
            for role in ("S", "C"):
                if role in self.h:
                    self.h[role].debug_set(binding.KEY.BATCH_FAIL, 1 | 1 << 32)
            return None
        if kind == "mode":
            for role, sa in self.h.items():
                if role == "P" and op[1] == "auto":
                    continue
                sa.set_accept_mode(op[1], op[2])
            m.mode, m.blk_done = op[1], 0
            res = {r: None for r in self.h}
        elif kind == "run":
            res = self._run(op[1])
            steps, modes, batch, live_first = self._last_run
        else:
            res = {role: apply_op(sa, self.pool, op, m.gstep) for role, sa in self.h.items()}
        for role in self.h:
            assert res[role] == res["S"], (tag, role, res[role], res["S"])
        r = res["S"]
        refused = isinstance(r, tuple) and len(r) == 2 and r[0] == "refused"
        now = self.seen = self.observe("S")
        for role in self.h:
            if role != "S":
                self._agree(now, self.observe(role), (tag, "S against", role))
        self._track(op, r, refused, prev, now, steps, modes, batch, tag)
        # the invariants that need no witness
        if now["best_cost"] and not m.best_is_bad:
            self._valid_at(now["best"], now["best_cost"], (tag, "best slab"))
        if not now["best_cost"]:
            assert same(now["best"], self.pool.get("literal")), (tag, "no best slab, but entries")
        self._valid_at(now["cur"], now["cur_cost"], (tag, "current slab"))
        if kind in OBSERVERS or refused and not (kind == "epoch" and op[2]) and kind != "set_slab_bad":
            self._agree(prev, now, (tag, "changed something"))
        if kind in CHANGES_BASE and not (refused and kind == "run"):
            live_map, rep = S.cost_map_live()
            host_map, host = binding.host_cost_map(self.data, now["cur"], self.props)
            assert rep["total"] == now["cur_cost"] == host["total"] and (live_map == host_map).all(), (tag, "live cost map")
        if "P" in self.h:
            self.others += kind not in CHANGES_BASE
            if kind in CHANGES_BASE or self.others % self.base_every == 0:
                self._same_base(self._canon(S, now["cur"]), self._canon(self.h["P"], now["cur"]), (tag, "base structures"))
        return r

    def _run(self, n):
        m, S = self.model, self.h["S"]
        st = S.run(n)
        s_modes = [int(x) for x in S.step_modes()]
        res = {"S": {f: st[f] for f in STAT_FIELDS}}
        assert len(s_modes) == n == st["steps"]
        if m.mode != "auto":
            assert s_modes == [MODES[m.mode]] * n, (m.mode, s_modes)
        C = self.h["C"]
        r0 = C.live_weights()["refreshes"]
        _, steps, c_modes, batch = run_cut(C, 1)
        live_first = C.live_weights()["refreshes"] > r0
        if n > 1:
            _, st2, md2, b2 = run_cut(C, n - 1)
            steps, c_modes, batch = steps + st2, c_modes + md2, batch + b2
        assert c_modes == s_modes, ("the modes depend on the cut", c_modes, s_modes)
        res["C"] = sum_stats(steps)
        if "P" in self.h:
            res["P"] = run_modes(self.h["P"], s_modes)
        if "F" in self.h:
            st = self.h["F"].run(n)
            res["F"] = {f: st[f] for f in STAT_FIELDS}
        self._last_run = (steps, s_modes, batch, live_first)
        return res

    # -- the contract on the best cost, the model and its transitions
    def _track(self, op, r, refused, prev, now, steps, modes, batch, tag):
        m, kind = self.model, op[0]
        unchanged_best = lambda: (now["best_cost"] == prev["best_cost"] and same(now["best"], prev["best"]))
        if kind == "run":
            assert not refused, (tag, r)
            assert not prev["best_cost"] or now["best_cost"] <= prev["best_cost"], (tag, "the best cost rose across a run")
            taken = [s["current_cost"] for s in steps if s["accepted"]]
            want = min(([prev["best_cost"]] if prev["best_cost"] else []) + taken, default=0)
            assert now["best_cost"] == want, (tag, "best cost", now["best_cost"], want)
            if m.can_replay():
                ref = m.replay(modes)
                for s, (a, b) in enumerate(zip(steps, ref)):
                    assert (a["accepted"], a["improved"], a["evaluations"]) == (b["accepted"], b["improved"], b["evaluations"]), (tag, "oracle, step", s, a, b)
                assert (now["cur_cost"], now["best_cost"]) == (m.cur_cost, m.best_cost), (tag, "oracle costs", m.cur_cost, m.best_cost)
                assert same(now["cur"], m.cur) and same(now["best"], m.best), (tag, "oracle slabs")
            else:  # not replayed: the run is adopted from the handles
                m.cur, m.cur_cost, m.best, m.best_cost = now["cur"], now["cur_cost"], now["best"], now["best_cost"]
            m.ran(steps, modes, batch, self._last_run[3])
            if now["best_cost"] != prev["best_cost"]:
                m.best_is_bad = m.unverified = False
            return
        if kind == "mode":
            return
        if kind == "temp":
            m.temperature = op[1]
        elif kind == "epoch":
            was_best, was_cost = prev["best"], prev["best_cost"]
            verified_from_best = op[2] and was_cost and not (m.unverified and m.best_is_bad)
            want = m.begin_epoch(op[1], op[2])
            assert (r == ("refused", want)) if want else r is None, (tag, r, want)
            if want:
                assert now["best_cost"] == 0, (tag, "the refused best slab was not forgotten")
            else:
                assert unchanged_best(), (tag, "begin_epoch changed the best slab")
            if verified_from_best:
                assert now["cur_cost"] == was_cost and same(now["cur"], was_best), (tag, "the epoch did not start from the best slab")
        elif kind in ("set_slab", "seed_greedy"):
            assert not refused, (tag, r)
            if kind == "set_slab":
                m.replace_current(self.pool.get(op[1]), self.pool.cost(op[1]), "set_slab(valid)")
            else:
                m.replace_current(now["cur"], now["cur_cost"], "seed_greedy")
            if kind == "set_slab":
                assert same(now["cur"], self.pool.get(op[1])) and now["cur_cost"] == self.pool.cost(op[1]), (tag, "set_slab")
            assert unchanged_best(), (tag, "the best slab changed")
        elif kind == "set_slab_bad":
            assert r == ("refused", EINVAL), (tag, r)
            m.replace_current(None, 0, "set_slab(invalid)")
            assert unchanged_best(), (tag, "the best slab changed")
        elif kind == "set_best":
            assert not refused, (tag, r)
            m.new_best(self.pool.get(op[1]), self.pool.cost(op[1]))
            assert now["best_cost"] == self.pool.cost(op[1]) and same(now["best"], self.pool.get(op[1])), (tag, "set_best")
        elif kind == "set_best_bad":
            assert not refused, (tag, r)
            m.new_best(now["best"], now["best_cost"], bad=True)
            assert violations(self.data, now["best"], DICT)[0][1] == BYTES_DIFFER and now["best_cost"] != prev["best_cost"], tag
        elif kind == "set_best_wrong_cost":
            assert r == ("refused", EINVAL), (tag, r)
        elif kind == "cross":
            assert not refused, (tag, r)
            st = dict(r)
            if st["parents"] == 0:
                assert prev["best_cost"] == 0 and st["adopted"] == 1, (tag, st)
                cost = st["parent_cost"][1]
            else:
                own, oth, child = st["parent_cost"][0], st["parent_cost"][1], st["child_cost"]
                assert own == prev["best_cost"], (tag, st)
                assert st["adopted"] == (2 if child < own and child < oth else 1 if oth < own else 0), (tag, st)
                cost = (own, oth, child)[st["adopted"]]
            assert now["best_cost"] == cost, (tag, st, now["best_cost"])
            if st["adopted"] == 0:
                assert unchanged_best(), (tag, "cross_best kept its best but changed it")
            elif st["adopted"] == 1 and op[1] != "own_best":
                assert same(now["best"], prev["cur"] if op[1] == "own_cur" else self.pool.get(op[1])), (tag, "cross_best adopted another slab than it was given")
            m.crossed(st["adopted"], now["best"], now["best_cost"])
        elif kind == "focus":
            if not refused:
                m.focus = (op[1], op[2])
        elif kind == "weights":
            if not refused:
                m.weighted, m.live = op[1] is not None, False
        elif kind == "live":
            if not refused:
                m.live, m.weighted, m.live_every = op[1] is not None, False, op[1] or 0
                m.stale_by = "enabled" if m.live else None
        if kind not in ("set_best", "set_best_bad", "cross", "epoch"):
            assert now["best_cost"] == prev["best_cost"], (tag, "the best cost moved")
        if kind not in ("epoch", "set_slab", "set_slab_bad", "seed_greedy"):
            assert now["cur_cost"] == prev["cur_cost"] and same(now["cur"], prev["cur"]), (tag, "the current slab moved")
        assert m.cur_cost == now["cur_cost"] and same(m.cur, now["cur"]), (tag, "model and handle disagree on the current slab")
        assert (m.best_cost == now["best_cost"]) and same(m.best, now["best"]), (tag, "model and handle disagree on the best slab")


# ---- the model alone (no device): what of a sequence the CPU can follow
def dry_run(model, pool, ops):
    """The model through `ops` without a handle, the runs by the oracle, as far as the CPU knows the outcome: it stops in
    front of the first operation whose result only the device has (seed_greedy's slab, a crossing of two different slabs,
    a run in MGL_ACCEPT_AUTO, under weights or a focus window) and returns how many operations it took."""
    m = model
    for i, op in enumerate(ops):
        kind = op[0]
        if kind == "run":
            if m.mode == "auto" or not m.can_replay():
                return i
            modes = [MODES[m.mode]] * op[1]
            steps = m.replay(modes)
            m.ran(steps, modes, [(1, 0) if md else None for md in modes], False)
        elif kind == "mode":
            m.mode, m.blk_done = op[1], 0
        elif kind == "temp":
            m.temperature = op[1]
        elif kind == "epoch":
            m.begin_epoch(op[1], op[2])
        elif kind == "set_slab":
            m.replace_current(pool.get(op[1]), pool.cost(op[1]), "set_slab(valid)")
        elif kind == "set_slab_bad":
            m.replace_current(None, 0, "set_slab(invalid)")
        elif kind == "set_best":
            m.new_best(pool.get(op[1]), pool.cost(op[1]))
        elif kind == "set_best_bad":
            bad = pool.bad_bytes()
            m.new_best(bad, m.oracle.cost_slab(bad)["total"], bad=True)
        elif kind == "cross":
            if m.best_cost == 0:
                m.crossed(1, pool.get(op[1]), pool.cost(op[1]))
            elif op[1] == "own_best":
                m.crossed(0, None, 0)
            else:
                return i
        elif kind == "save":
            if m.best_cost and not m.best_is_bad:
                pool.slabs["saved_best"] = m.best.copy()
            pool.slabs["saved_cur"] = m.cur.copy()
        elif kind == "seed_greedy":
            return i
        elif kind == "focus":
            m.focus = (op[1], op[2])
        elif kind == "weights":
            m.weighted, m.live = op[1] is not None, False
        elif kind == "live":
            m.live, m.weighted, m.live_every = op[1] is not None, False, op[1] or 0
    return len(ops)


# ---- the scripted tour
TOUR_K, TOUR_SEED = 48, 1673551
TOUR_IPE = 12 * TOUR_K
_T = 16384  # cost units per byte


def tour():
    """One hand-written sequence that takes every transition of TRANSITIONS once by construction, for corpus.lorem(1800),
    K = 48, epochs of 12 steps, seed 1673551.  The part up to seed_greedy runs in explicit modes, so the CPU model follows
    it (tests/test_handle_ops_cpu.py asserts which transitions that part takes); behind it come the operations whose outcome
    only the device has: the greedy seed, a crossing that adopts the child, MGL_ACCEPT_AUTO's blocks, weights and focus."""
    ops = [
        # single steps.  No best yet; a best adopted by cross_best and verified by the epoch that starts from it
        ("mode", "single", 6), ("epoch", 1, True), ("cross", "xz", 0), ("epoch", 1, True), ("run", 1), ("run", 3),
        # the base is the only holder of the best slab: observers, then everything that overwrites the base
        ("cross", "own_best", 64), ("obs", "best_packed"), ("obs", "slab_hash"), ("save",),
        ("set_slab", "literal"), ("obs", "cost_map_live"), ("epoch", 1, True), ("run", 2),
        ("set_slab_bad", "xz"), ("epoch", 2, True), ("run", 2), ("obs", "neighbours"),
        ("epoch", 0, True), ("set_best_wrong_cost", "xz"), ("set_best", "xz"), ("obs", "cost_map"), ("epoch", 1, True), ("run", 7),
        # bulk steps.  Step 0 of an epoch takes moves uphill: a new best, then -- the base still holding the best slab, and the
        # snapshot of an older best still valid -- off the best slab, and an epoch from the best slab right behind it
        ("mode", "bulk", 6), ("epoch", 1, True), ("run", 1), ("epoch", 1, True), ("run", 1), ("epoch", 1, True), ("run", 6), ("save",),
        # a single step off the best slab: after that descent the first step of an epoch finds nothing better
        ("mode", "single", 6), ("epoch", 0, True), ("run", 1),
        # a dearer best slab put under the current one, so that the next move is a new best; then step 0 of an epoch by the
        # bulk route, with the batch accept made to give up behind its commit: the rebuild applies the step that leaves the best slab
        ("set_best", "xz"), ("run", 3), ("mode", "bulk", 6), ("epoch", 0, True), ("force_batch_fail",), ("run", 1), ("epoch", 2, True),
        # a best slab that copies wrong bytes: refused by the epoch that starts from it, forgotten, and then there is none
        ("obs", "cost_slab"), ("set_best_bad",), ("epoch", 1, True), ("epoch", 0, True), ("run", 2),
        # -- from here on the device alone knows the outcome
        ("seed_greedy", 8), ("epoch", 1, True), ("run", 2),
        ("set_best", "greedy"), ("cross", "xz", 64), ("epoch", 0, True),
        # two searches from one parse, each under a window over one half: the child of the two is cheaper than both
        # (the text repeats from 600 on: behind it the parse is a few long matches that no search improves)
        ("set_slab", "xz"), ("focus", 0, 60), ("run", 6), ("save",), ("set_slab", "xz"), ("focus", 60, 600), ("run", 6), ("focus", 0, 0),
        ("set_best", "saved_cur"), ("cross", "own_cur", 16), ("epoch", 2, True),
        ("set_slab", "xz"), ("focus", 0, 100), ("run", 6), ("save",), ("set_slab", "xz"), ("focus", 100, 600), ("run", 6), ("focus", 0, 0),
        ("set_best", "saved_cur"), ("cross", "own_cur", 1), ("epoch", 2, True),
        # MGL_ACCEPT_AUTO: blocks of 4 bulk / 16 single steps, cut by the end of a run, by set_slab, by begin_epoch
        ("mode", "auto", 6), ("epoch", 0, False), ("run", 3), ("run", 2), ("set_slab", "xz"), ("run", 3), ("cross", "saved_cur", 16), ("run", 2),
        ("epoch", 1, True), ("run", 5),
        ("mode", "single", 6),
    ]
    g = sum(op[1] for op in ops if op[0] == "run") + 2
    every = 5 if g % 5 else 7  # the run behind set_slab must not start on a step that refreshes anyway
    ops += [("live", every, 1, False), ("run", 2), ("set_slab", "xz"), ("run", 2), ("live", None, 0, False),
            ("focus", 100, 900), ("run", 2), ("focus", 0, 0), ("weights", 3), ("run", 1), ("weights", None),
            ("epoch", 1, True), ("run", 3)]
    return ops


# the transitions the CPU model takes in the tour's first part (up to seed_greedy)
TOUR_CPU_PART = tuple(t for t in TRANSITIONS if t not in (
    "bulk step leaves the best slab: rebuild behind a forced give-up",  # (the model alone cannot tell who applied a bulk step)
    "seed_greedy while the base holds the best slab", "cross_best adopted 2", "auto block cut by set_slab", "auto block cut by begin_epoch",
    "auto block cut by the end of a run", "live weights refreshed because set_slab left them stale"))
