"""Every give-up path of the in-place accepts (mgl_kernels3.hip: a single accept; mgl_kernels5.hip: the moves of a bulk
step) against the rebuild.  Both accepts leave the step to a rebuild whenever something does not fit; mgl_debug_set's KEY.LIMIT
lowers what a site compares against, so the real comparison fires on an ordinary input, and the give-up word
(DUMP.GIVEUP_SITES) says which site fired.  Each case runs three chains with one seed: A with the limit lowered,
B that never patches in place, T with the default limits (it may not give up on the same steps), and a handle R that only
rebuilds from a slab.  DESIGN.md section 6 has the table of sites, limits and cases.  `-m gpu`."""
import numpy as np
import pytest

from _libs import Oracle, assert_same_base, canonical_base, literal_slab
from megalania_amd import binding, corpus
from megalania_amd.binding import GU, LIM

pytestmark = pytest.mark.gpu

EARLY = GU.CL_JOURNAL | GU.CL_ORDER | GU.WALK_OPS | GU.WALK_EVENTS | GU.WALK_GUARD | GU.WALK_INVALID | GU.WALK_OVERRUN
POOL_TOP = -1  # a case's value: the chain pool's top when the limit is set (nothing may take fresh pool space)
PB2 = dict(lc=2, lp=1, pb=2)


def site_names(word):
    return [g.name.lower() for g in GU if word & g]


class Chains:
    """A (limits lowered), B (never patches in place), T (default limits), R (rebuild only), one seed."""

    def __init__(self, kind, data, K, seed, props, monkeypatch, ipe=10**7):
        self.kind, self.data = kind, data
        mk = lambda: binding.SA(data, accept=kind, neighbours_per_step=K, seed=seed, iters_per_epoch=ipe, **props)
        self.a, self.t = mk(), mk()
        off = "MGL_NO_INCREMENTAL_APPLY" if kind == "single" else "MGL_NO_BATCH"
        monkeypatch.setenv(off, "1")
        self.b = mk()
        monkeypatch.delenv(off)
        self.r = binding.SA(data, accept="single", neighbours_per_step=8, seed=seed, **props)
        self.o = Oracle(data, dict_limit=0x400000, **props)
        self.step = 0
        self.gave_up = self.in_place = self.sites = 0
        self.multi = 0   # steps that took two or more moves and did not give up
        self.a.giveup_sites(); self.t.giveup_sites()

    def close(self):
        for x in (self.a, self.b, self.t, self.r):
            x.close()

    def counters(self, sa):
        if self.kind == "single":
            return None
        return sa.batch_counters() + (sa.batch_giveups(),)

    def check_structures(self, what):
        cur, cost = self.a.current()
        assert (cur == self.b.current()[0]).all(), what
        assert cost == self.o.cost_slab(cur.astype(literal_slab(1).dtype))["total"], what
        self.r.set_slab(cur)
        assert_same_base(canonical_base(self.a, cur), canonical_base(self.r, cur), what)

    def run(self, steps, expect=None, every=4):
        """`steps` steps in lockstep.  expect = None: A runs with the default limits and does exactly what T does (a bulk step
        from the all-literal slab can exceed a real capacity: the first steps at 30 KB stage more than MGL_BATCH_EVCAP events in one
        cluster); else A's limits are lowered: the sites A is allowed to take, and T may not give up at all on these steps.
        Returns the give-up words of A, step by step."""
        words = []
        for _ in range(steps):
            c0 = self.counters(self.a)
            sa_, sb_, st_ = self.a.run(1), self.b.run(1), self.t.run(1)   # (run raises on any MGL_ERR_* flag, MGL_ERR_REBUILD_MISMATCH included)
            what = (self.kind, "step", self.step)
            for k in ("current_cost", "best_cost", "accepted", "evaluations"):
                assert sa_[k] == sb_[k] == st_[k], (what, k, sa_[k], sb_[k], st_[k])
            assert sa_["bulk_rollbacks"] == 0 and st_["bulk_rollbacks"] == 0, what
            word = self.a.giveup_sites()
            if self.kind == "single":
                n_giveups = sa_["full_rebuilds"]
                assert st_["full_rebuilds"] == 0, what
            else:
                c1 = self.counters(self.a)
                late, early = c1[1] - c0[1], c1[2] - c0[2]
                n_giveups = late + early
                # a site behind the commit counts as a fallback, one in front of it as an early give-up
                assert (early == 1) == bool(word & EARLY) and (late == 1) == bool(word & ~EARLY), (what, site_names(word), late, early)
                assert sa_["full_rebuilds"] == 0, what
            assert n_giveups == (1 if word else 0), (what, site_names(word), n_giveups)
            tword = self.t.giveup_sites()
            if expect is None:
                assert word == tword, (what, "two chains with the default limits", site_names(word), site_names(tword))
                assert self.kind == "bulk" or word == 0, (what, "a single accept gave up with the default limits", site_names(word))
            else:
                assert tword == 0, (what, "the chain with the default limits gave up", site_names(tword))
                assert word & ~expect == 0, (what, "another site fired", site_names(word))
            self.gave_up += 1 if word else 0
            self.in_place += 1 if (sa_["accepted"] and not word) else 0
            self.multi += 1 if (sa_["accepted"] >= 2 and not word) else 0
            self.sites |= word
            if word or (sa_["accepted"] and self.step % every == 0):
                self.check_structures(what)
            words.append(word)
            self.step += 1
        return words


def arm(ch, limit, value):
    if value == POOL_TOP:
        value = int(ch.a.debug_dump(binding.DUMP.POOL_TOP)[0])
    ch.a.set_limit(limit, value)
    ch.gave_up = ch.in_place = ch.sites = 0   # (what the warm-up did on its own is not the case's)
    return value


def inputs(name):
    from test_oracle_golden import doubled_letters
    return {"enwik6k": lambda: corpus.enwik_like(6000, 0x5151), "enwik30k": lambda: corpus.enwik_like(30000, 0x5151),
            "lorem3k": lambda: corpus.lorem(3000), "doubled1": lambda: doubled_letters(1, 2600),
            "doubled5": lambda: doubled_letters(5, 2600)}[name]()


# one case per give-up site of mgl_kernels3.hip: (site, limit, value, input, props, K, warm-up steps, steps under the limit).
# The values: low enough that the site fires on these steps while the chain with the default limits patches every one of
# them in place; chosen from what that chain used per accepted step on the first run (enwik6k, steps 20-60: 42-58 inserted
# and 65-171 removed events, 50-62 touched contexts, 35-88 / 92-123 jobs, 359-4233 span and 326-4468 save entries).  The
# comments: steps under the limit that gave up / that patched in place, on the MI355X run the values were fixed on.
SINGLE = [
    ("apply_events", LIM.APPLY_EVENTS, 140, "enwik6k", {}, 96, 20, 40),          # 10 / 30, first at step 20
    ("apply_events", LIM.APPLY_EVENTS, 140, "enwik6k", PB2, 96, 20, 40),         # 8 / 32
    ("apply_guard", LIM.APPLY_GUARD, 3, "enwik6k", {}, 96, 20, 30),              # 30 / 0: every accepted move walks more than three packets
    ("apply_sub", LIM.APPLY_SUB, 8, "enwik6k", {}, 96, 20, 30),                  # 27 / 3
    ("apply_span", LIM.APPLY_SPAN, 128, "enwik6k", {}, 96, 20, 40),              # 37 / 3
    ("apply_pieces", LIM.APPLY_PIECES, 1, "enwik6k", {}, 96, 20, 40),            # 40 / 0: fires at the first re-join of any context (3 never fired in 40 steps: one move, one segment per context)
    ("apply_shift", LIM.APPLY_SHIFT, 3, "enwik6k", {}, 96, 20, 40),              # 38 / 2
    ("apply_pool", LIM.POOL, POOL_TOP, "enwik30k", {}, 256, 20, 900),            # 1 / 246: step 266, the first chain (an empty rep context, 264 entries of room) to outgrow its slot
    ("apply_jobs", LIM.JOBS, 105, "enwik6k", {}, 96, 20, 40),                    # 21 / 19
    ("apply_span_area", LIM.SPAN_AREA, 2800, "enwik6k", {}, 96, 20, 40),         # 12 / 28
    ("apply_scratch", LIM.SCRATCH, 2900, "enwik6k", PB2, 96, 20, 40),            # 27 / 13
    ("apply_scratch", LIM.SCRATCH, 2900, "enwik6k", {}, 96, 20, 40),
    ("apply_span", LIM.APPLY_SPAN, 128, "enwik6k", PB2, 96, 20, 40),
    ("apply_jobs", LIM.JOBS, 105, "enwik6k", PB2, 96, 20, 40),
]


@pytest.mark.parametrize("site,limit,value,name,props,K,warm,steps", SINGLE,
                         ids=[f"{c[0]}{'-lc2lp1pb2' if c[4] else ''}" for c in SINGLE])
def test_single_accept_that_gives_up_equals_the_rebuild(site, limit, value, name, props, K, warm, steps, monkeypatch):
    """The single accept's fallback (Control::apply_failed -> k_build inside the same step): taken at the named site, it leaves
    bitmaps, state records, chains, chain index, dense checkpoints and the cost exactly as a rebuild from the slab does (and
    k_build's own check of the patched cost against its walk raises no MGL_ERR_REBUILD_MISMATCH); with the limits restored the
    next steps patch in place again and still agree."""
    ch = Chains("single", inputs(name), K, 5, props, monkeypatch)
    ch.run(warm, expect=None, every=16)
    arm(ch, limit, value)
    first = None
    for _ in range(steps):   # (a long run under the limit -- the pool case waits for a chain to outgrow its slot -- ends four steps behind the first give-up)
        ch.run(1, expect=GU[site.upper()], every=4 if steps <= 100 else 64)
        if ch.gave_up and first is None:
            first = ch.step
        if steps > 100 and first is not None and ch.step - first >= 4:
            break
    assert ch.gave_up >= 1 and ch.sites == GU[site.upper()], (site, ch.gave_up, ch.in_place, site_names(ch.sites))
    ch.a.set_limit(0, 0)
    ch.in_place = 0
    ch.run(16, expect=None, every=2)
    assert ch.in_place >= 3
    ch.close()


# (site, limit, value, input, props, K, seed, warm-up steps, steps under the limit).  The warm-up has two give-ups of its own, with
# the default limits, which A, T, B and R agree on like on any other step: step 0 from the all-literal slab stages more than
# MGL_BATCH_EVCAP events in one cluster (status 2), and under lc2/lp1/pb2 step 3 fills the span area (status 1, behind a partial
# rewrite).  Not exercised, because no capacity reaches them: a merged journal that is not strictly ascending (cl_order) and a
# packet or rep packet of a merged walk that does not code the input (walk_invalid) -- both would be bugs of the selection.
BATCH = [
    ("cl_journal", LIM.BATCH_JOURNAL, 2, "enwik30k", {}, 256, 9, 12, 10),        # 10 / 0, from step 12 on (the first under the limit)
    ("walk_events", LIM.BATCH_EVENTS, 64, "enwik30k", {}, 256, 9, 12, 10),       # 10 / 0
    ("walk_ops", LIM.BATCH_OPS, 8, "enwik30k", {}, 256, 9, 12, 10),              # 10 / 0
    ("walk_guard", LIM.BATCH_GUARD, 4, "enwik30k", PB2, 256, 9, 12, 10),         # 10 / 0
    ("ch_sub", LIM.BATCH_SUB, 8, "enwik30k", {}, 256, 9, 12, 10),                # 10 / 0
    ("ch_shift", LIM.BATCH_SHIFT, 2, "enwik30k", {}, 256, 9, 12, 10),            # 10 / 0
    ("ch_pool", LIM.POOL, POOL_TOP, "enwik30k", {}, 256, 9, 12, 16),             # 1 / 15: step 12 (the rebuild it falls back to lays the pool out afresh, below the limit)
    ("ch_jobs", LIM.JOBS, 1750, "enwik30k", {}, 256, 9, 12, 10),                 # 9 / 1 (the default chain queues 1 580-1 900 jobs per list on these steps)
    ("ch_span_area", LIM.SPAN_AREA, 4096, "enwik30k", PB2, 256, 9, 12, 10),      # 10 / 0
    ("ch_span_area", LIM.SPAN_AREA, 4096, "enwik30k", {}, 256, 9, 12, 10),
    # step 5's own comparison (a run that outgrew its first place is written again, after the chain got its pool space): the default
    # chain uses 640-750 K span entries on these steps, about 285 K of them first places (1 080 runs x 264) -- a capacity between the
    # two lets most first places through; workgroups interleave, so either of the two sites may be the one that fires on a step
    ("ch_span_rerun", LIM.SPAN_AREA, 420000, "enwik30k", {}, 256, 9, 12, 10),
    ("walk_guard", LIM.BATCH_GUARD, 4, "enwik30k", {}, 256, 9, 12, 10),
    ("ch_scratch", LIM.SCRATCH, 64, "enwik30k", {}, 256, 9, 12, 10),             # 10 / 0
    ("ch_runs", LIM.BATCH_RUNS, 1080, "enwik30k", {}, 256, 9, 12, 10),           # 8 / 2 (1 020-1 200 runs per step)
]


@pytest.mark.parametrize("site,limit,value,name,props,K,seed,warm,steps", BATCH,
                         ids=[f"{c[0]}{'-lc2lp1pb2' if c[4] else ''}" for c in BATCH])
def test_batch_accept_that_gives_up_equals_the_rebuild(site, limit, value, name, props, K, seed, warm, steps, monkeypatch):
    """The batch accept's give-ups, each at its own site: in front of the commit (clusters, walks: status 2, nothing touched)
    and behind it (k_batch_chains: status 1, while other workgroups have rewritten chain descriptors, taken pool space, patched
    index rows and queued jobs).  The step ends exactly where the chain that always rebuilds ends, the structures equal a
    rebuild from the slab, and with the limits restored the next steps patch in place again."""
    ch = Chains("bulk", inputs(name), K, seed, props, monkeypatch)
    ch.run(warm, expect=None, every=6)
    arm(ch, limit, value)
    also = GU.CH_SPAN_AREA if site == "ch_span_rerun" else 0
    ch.run(steps, expect=GU[site.upper()] | also)
    assert ch.gave_up >= 1 and ch.sites & ~also == GU[site.upper()], (site, ch.gave_up, ch.in_place, site_names(ch.sites))
    ch.a.set_limit(0, 0)
    ch.in_place = 0
    acc0 = ch.a.batch_counters()[0]
    ch.run(8, expect=None, every=2)
    assert ch.in_place >= 3 and ch.a.batch_counters()[0] - acc0 >= 3
    ch.close()


@pytest.mark.parametrize("which,props", [("first", {}), ("half", {}), ("all", {}), ("early", {}), ("half", PB2), ("all", PB2)],
                         ids=["first", "half", "all", "early", "half-lc2lp1pb2", "all-lc2lp1pb2"])
def test_forced_give_up_behind_a_partial_rewrite(which, props, monkeypatch):
    """mgl_debug_set key 5.  High word n: k_batch_chains gives up once the n-th touched context has rewritten its chain's
    descriptors, taken its pool space and queued its jobs -- "some workgroups done, some not" cannot be made by a capacity.
    Which contexts are the first n depends on scheduling; the result may not.  n = 1, half of the step's touched contexts, all
    of them (sized from bt.hdr[10] of a probe chain that has just taken the step A is about to take).  Low word alone: the
    give-up at the top of the kernel, before any chain is touched.  Also under lc2/lp1/pb2: position-dependent contexts change
    which contexts a step touches."""
    ch = Chains("bulk", inputs("enwik30k"), 256, 9, props, monkeypatch)
    ch.run(12, expect=None, every=6)
    ch.gave_up = 0
    fb0 = ch.a.batch_counters()[1]
    for rnd in range(3):
        # a fresh chain with the same seed, run one step further than A stands: one trajectory, so A's next step touches as many
        # contexts.  (T cannot be sent ahead instead: Chains.run keeps A, B and T in lockstep and compares them step by step.)
        probe = binding.SA(ch.data, accept="bulk", neighbours_per_step=256, seed=9, iters_per_epoch=10**7, **props)
        probe.run(ch.step + 1)
        hdr = probe.debug_dump(binding.DUMP.BATCH_HDR)[0]
        probe.close()
        touched = int(hdr["touched"])
        assert hdr["status"] == binding.BATCH.DONE and touched >= 4, ("the probed step was no batch accept", hdr)
        n = {"first": 1, "half": touched // 2, "all": touched, "early": 0}[which]
        ch.a.debug_set(binding.KEY.BATCH_FAIL, 1 | (n << 32))
        want = GU.FORCED_EARLY if which == "early" else GU.FORCED_LATE
        words = ch.run(1, expect=want)
        assert words == [want], (which, rnd, n, touched, site_names(words[0]))
        ch.run(2, expect=None, every=1)
    assert ch.gave_up == 3 and ch.a.batch_counters()[1] - fb0 == 3
    ch.close()


@pytest.mark.parametrize("name,props,K,seed,warm,steps,ipe", [("doubled1", {}, 96, 1 * 7717, 0, 60, None), ("doubled5", {}, 96, 5 * 7717, 0, 60, None),
                                                              ("doubled5", PB2, 96, 5 * 7717, 0, 60, None), ("enwik30k", {}, 256, 9, 12, 24, 10**7)],
                         ids=["doubled1", "doubled5", "doubled5-lc2lp1pb2", "enwik30k"])
def test_cluster_boundary_guard(name, props, K, seed, warm, steps, ipe, monkeypatch):
    """k_batch_clusters separates clusters where the members' individual walks have re-joined the base (`reach` = their largest
    hard end); the selection lets a self-contained move start inside [soft end, hard end) of another, so the merged walk of a
    cluster is not proven to re-join by then.  k_batch_walk therefore stops at the next cluster's first journal entry: a walk
    that has not re-joined there gives the step to the rebuild instead of reading the next cluster's range with the old
    packets.  With limit 18 the clusters are split at the SOFT ends: every such pair then opens a cluster of its own, the
    first one's walk has provably not re-joined at the boundary, the guard must fire and the step must end exactly like the
    rebuild route's -- the structures compared with a rebuild after EVERY step (the steps that matter are those on which the
    guard did not fire and the moves were patched in with the wrong clusters), step by step against the chain that always
    rebuilds and, on the small inputs, the oracle: same costs, and the guard fires on exactly the steps on which the oracle's
    restatement of the knob (orc_bulk_soft_overruns) finds a cluster that has not re-joined -- no missed overrun, no false
    one.  With the knob off (chain T) the same steps show no overrun and no early give-up."""
    data = inputs(name)
    n = len(data)
    ch = Chains("bulk", data, K, seed, props, monkeypatch, ipe=ipe or n)
    small = n < 5000
    if small:
        slab, best = literal_slab(n), literal_slab(n)
        ocur = obest = 0
    ch.run(warm, expect=None, every=6)   # (30 KB: the all-literal slab's first steps exceed a real capacity, see Chains.run)
    arm(ch, LIM.SOFT_REACH, 1)
    t_early0, a_early0 = ch.t.batch_giveups(), ch.a.batch_giveups()
    for s in range(steps):
        word = ch.run(1, expect=GU.WALK_OVERRUN, every=1)[0]
        if small:
            soft0 = ch.o.bulk_soft_overruns()
            res = ch.o.sa_batched(slab, best, ocur, obest, seed, K, 0, n, s, s + 1, iter0=s * K, modes=[1])
            ocur, obest = res["cur"], res["best"]
            assert ch.a.current()[1] == ocur, (name, s)
            assert bool(word) == (ch.o.bulk_soft_overruns() != soft0), (name, s, "guard fired", bool(word))
    assert ch.gave_up >= 1 and ch.sites == GU.WALK_OVERRUN
    assert ch.a.batch_giveups() - a_early0 == ch.gave_up and ch.a.batch_counters()[1] == 0
    assert ch.t.batch_giveups() == t_early0 and ch.t.batch_counters()[1] == 0   # knob off: no overrun, no status-2 give-up on these steps
    if small:
        cur, cost = ch.a.current()
        assert cost == ocur and (cur["type"] == slab["type"]).all() and (cur["dist"] == slab["dist"]).all() and (cur["len"] == slab["len"]).all()
    ch.a.set_limit(0, 0)
    ch.run(6, expect=None, every=2)
    ch.close()


def test_key_6_refuses_what_it_cannot_honour():
    sa = binding.SA(corpus.lorem(2000), accept="single", neighbours_per_step=32, seed=3)
    for bad in (LIM.APPLY_EVENTS | (8193 << 8), LIM.BATCH_SHIFT | (2048 << 8), LIM.SOFT_REACH | (2 << 8), len(LIM) + 1, 0 | (1 << 8), 200 | (1 << 8)):
        assert sa.L.mgl_debug_set(sa.h, binding.KEY.LIMIT, bad) != 0, bad
    top = int(sa.debug_dump(binding.DUMP.POOL_TOP)[0])
    assert sa.L.mgl_debug_set(sa.h, binding.KEY.LIMIT, LIM.POOL | ((1 << 40) << 8)) != 0
    assert sa.L.mgl_debug_set(sa.h, binding.KEY.LIMIT, LIM.POOL | (top << 8)) == 0
    assert sa.L.mgl_debug_set(sa.h, binding.KEY.LIMIT, 0) == 0
    st = sa.run(20)
    assert st["accepted"] > 0 and st["full_rebuilds"] == 0 and sa.giveup_sites() == 0
    sa.close()
