"""The set-up of the top-K sources against the oracle, in both forms: batched (topk_plan_make: probe form 0,
topk_find<4, true>, and the split pick) and in place (source_range without a plan: probe form 1, topk_find<1>, and
the one-kernel form).  Aimed at what a search for the sources' bounds can get wrong: lower bounds that take two
and three 64-ary levels with the window floor inside a run of thousands of entries, orders whose runs differ in
length at one position, the scan cap (where the runs are searched for the first position the cap leaves, not for
the window floor), and the split pick itself, whose plan is made in front of the model load.  All comparisons are
exact.  `-m gpu`."""
import numpy as np
import pytest

from _libs import MATCH, Oracle, literal_slab, walk
from conftest import rand_bytes
from megalania_amd import binding, corpus
from test_gpu_parity import _check_neighbours
from test_oracle_search_config import as_list

pytestmark = pytest.mark.gpu

N = 24576
WINDOWS = [1000, 5000, 0]  # 0: the production window (4 MiB: none of these inputs reaches it)
CAPS = [1, 64, 65]
_CACHE = {}


def P(slab):
    return np.ascontiguousarray(slab).astype(binding.PACKET)


def make_input(name):
    if name == "abc":
        return b"abc" * 8192  # every order: runs of up to 8 192 entries, three 64-ary levels
    if name == "zeros":
        return bytes(N)  # one run in every order
    if name == "ab_lorem":
        return b"ab" * 6000 + corpus.lorem(N - 12000)
    raise KeyError(name)


def evolved_slab(data, steps=30, K=32, seed=11):
    """The slab test_oracle_search_config.evolve() makes -- 30 single-accept steps of 32 neighbours from the literal
    slab, seed 11 -- made by the device's search, which follows the oracle's step by step (test_gpu_search_config pins
    that): on these inputs the oracle needs minutes for it.  What is checked here is that it is a slab the oracle
    prices the same and that it carries matches."""
    n = len(data)
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=seed, iters_per_epoch=steps * K)
    sa.run(steps)
    cur, cost = sa.current()
    sa.close()
    slab = cur.astype(literal_slab(1).dtype)
    assert cost == Oracle(data).cost_slab(slab)["total"]
    assert len(walk(slab)) < n - 20
    return slab


def case(name):
    """data, [(kind, slab, walk positions)]: made once, shared by every test and left unchanged"""
    if name not in _CACHE:
        data = make_input(name)
        slabs = []
        for kind, slab in (("literal", literal_slab(len(data))), ("evolved", evolved_slab(data))):
            slab.setflags(write=False)
            slabs.append((kind, slab, walk(slab)))
        _CACHE[name] = (data, slabs)
    return _CACHE[name]


def probe_positions(w, n, D, count, seed):
    """about `count` on-walk positions: the two ends, the window's edge, and a seeded draw that is uniform in
    log(position).  On these inputs a position p has about p hits, each at up to 272 lengths, and the oracle prices
    every one: a draw uniform in p would cost it five times as much, while how many levels a search takes -- what
    these positions are for -- depends on log p.  About a fifth of the draw lies beyond 4 096 (three levels)."""
    on = set(w)
    rng = np.random.default_rng(seed)
    must = [1, 2, n - 2] + ([D - 1, D, D + 1] if D else [])
    pool = np.array([p for p in w if 0 < p < n - 1])
    want = np.exp(rng.uniform(0.0, np.log(n - 2), size=count))
    ps = {int(pool[min(len(pool) - 1, int(np.searchsorted(pool, x)))]) for x in want}
    return sorted(ps | {p for p in must if p in on})


def same_as_oracle(sa, o, slab, ps, k=20, what=()):
    """both probe forms against one oracle answer per position; the handle is left on the default form"""
    dslab = P(slab)
    for p in ps:
        opk, ocosts = o.top_k(slab, p, mode=1, k=k)
        want = (as_list(opk), [int(c) for c in ocosts])
        for form in (1, 0):
            pk, costs = sa.top_k(dslab, p, form=form)
            assert (as_list(pk), [int(c) for c in costs]) == want, (what, p, form)


@pytest.mark.parametrize("D", WINDOWS, ids=lambda D: f"D{D}")
@pytest.mark.parametrize("name", ["abc", "zeros", "ab_lorem"])
def test_probe_with_the_floor_inside_long_runs(name, D):
    """mgl_top_k == Oracle.top_k(mode=1) where the runs hold thousands of entries and the window floor falls inside
    them: searches of two and three levels in every order at once.  60 draws (fewer distinct positions near the
    start, where the draw is dense) and the ends and the window's edge, on the literal slab and again on the evolved
    one; the literal slab has every position on its walk, so the ends and the edge are always probed there."""
    data, slabs = case(name)
    n = len(data)
    sa = binding.SA(data, neighbours_per_step=8, dict_limit=D)
    o = Oracle(data, dict_limit=D)
    ob = Oracle(data)
    total, two, three = 0, 0, 0
    for kind, slab, w in slabs:
        ps = probe_positions(w, n, D, 60, seed=D + len(w))
        total += len(ps)
        if kind == "literal":
            assert {1, 2, n - 2} <= set(ps) and (not D or {D - 1, D, D + 1} <= set(ps))
        same_as_oracle(sa, o, slab, ps, what=(name, kind, D))
        for p in ps:
            offs = np.unique(ob.substrings(p, max_len=2)[0]).astype(np.int64)
            inside = int((p - offs - 1 < D).sum()) if D else len(offs)
            cut = D == 0 or len(offs) - inside > 0
            two += cut and inside > 64     # more than 64 entries on the near side of the floor: a second level
            three += cut and len(offs) > 4096  # a run of more than 64 * 64 entries: a third
    assert total >= 80, total
    assert two >= 3 and three >= 1, (two, three)
    sa.close()


def test_probe_form_key():
    """MGL_KEY_PROBE_FORM takes 0 and 1 and refuses 2 (the form stays what it was); a handle switched 1 -> 0 answers
    as one that never left 0."""
    data, slabs = case("ab_lorem")
    _, slab, w = slabs[1]
    dslab = P(slab)
    ps = probe_positions(w, len(data), 5000, 12, seed=5)
    sa = binding.SA(data, neighbours_per_step=8, dict_limit=5000)
    fresh = [sa.top_k(dslab, p) for p in ps]
    sa.debug_set(binding.KEY.PROBE_FORM, 1)
    with pytest.raises(binding.MglError) as e:
        sa.debug_set(binding.KEY.PROBE_FORM, 2)
    assert e.value.rc == -1  # MGL_EINVAL
    in_place = [sa.top_k(dslab, p) for p in ps]
    sa.debug_set(binding.KEY.PROBE_FORM, 0)
    again = [sa.top_k(dslab, p) for p in ps]
    for a, b, c in zip(fresh, in_place, again):
        assert as_list(a[0]) == as_list(c[0]) == as_list(b[0]) and a[1].tolist() == c[1].tolist() == b[1].tolist()
    assert any(len(a[0]) == 20 for a in fresh)
    sa.close()


def planted_orders_input():
    """Bytes below 0x80 at random, with two plants in bytes from 0x80 up (so that nothing else matches them):
    200 copies of a three-byte word, each followed by other low bytes -- at the last one, `short`, the three-byte run
    is long and no hit reaches four bytes beyond a handful, none sixteen; and 100 copies of a twenty-byte block -- at
    the last one, `long_`, every hit is twenty bytes long: the sixteen-byte run holds all of them and no shorter
    order has an entry of its own."""
    b = bytearray(x & 0x7F for x in rand_bytes(16384, 29))
    word, block = bytes([0x81, 0x92, 0xA3]), bytes(range(0xC0, 0xD4))
    at = 100
    for i in range(200):
        b[at:at + 3] = word
        b[at + 3], b[at + 4] = i % 128, i // 128  # what follows differs from copy to copy
        at += 37
    short = at - 37
    for i in range(100):
        b[at:at + 20] = block
        b[at + 20] = i  # and so does this
        at += 41
    long_ = at - 41
    assert at < len(b)
    return bytes(b), short, long_


@pytest.mark.parametrize("D", [1000, 0], ids=lambda D: f"D{D}")
def test_orders_whose_runs_differ(D):
    data, short, long_ = planted_orders_input()
    ob = Oracle(data)
    offs, lens = ob.substrings(short)
    per_q = {}
    for q, ln in zip(offs.tolist(), lens.tolist()):
        per_q[q] = max(per_q.get(q, 0), ln)
    assert sum(1 for v in per_q.values() if v == 3) >= 150 and max(per_q.values()) < 16, sorted(per_q.values())[-5:]
    offs, lens = ob.substrings(long_)
    per_q = {}
    for q, ln in zip(offs.tolist(), lens.tolist()):
        per_q[q] = max(per_q.get(q, 0), ln)
    assert len(per_q) == 99 and set(per_q.values()) == {20}, sorted(set(per_q.values()))
    if D:
        # the floor cuts both plants' runs
        assert 0 < sum(1 for q in per_q if long_ - q - 1 < D) < 99
    sa = binding.SA(data, neighbours_per_step=8, dict_limit=D)
    o = Oracle(data, dict_limit=D)
    slab = literal_slab(len(data))
    ps = sorted({p + d for p in (short, long_) for d in (-2, -1, 0, 1, 2)} | {short - 37, long_ - 41, long_ - 41 * 50})
    same_as_oracle(sa, o, slab, ps, what=("planted", D))
    # not vacuous: the long plant's list holds a twenty-byte MATCH, the short one's a three-byte MATCH and none longer than four
    assert any(t == MATCH and ln == 20 for t, _, ln in as_list(sa.top_k(P(slab), long_)[0]))
    short_list = [x for x in as_list(sa.top_k(P(slab), short)[0]) if x[0] == MATCH]
    assert short_list and max(ln for _, _, ln in short_list) <= 4 and any(ln == 3 for _, _, ln in short_list), short_list
    sa.close()


def far_plant_input():
    """Bytes below 0x80 at random; a forty-byte block of bytes from 0x80 up at 200, then its first two bytes a hundred
    times with low bytes behind them, then the block again at `t`: of the hits at t the hundred nearest match two
    bytes and the farthest forty, 3 100 bytes back."""
    b = bytearray(x & 0x7F for x in rand_bytes(4096, 31))
    block = bytes(range(0x90, 0xB8))
    b[200:240] = block
    at = 300
    for _ in range(100):
        b[at:at + 2] = block[:2]
        at += 30
    b[at:at + 40] = block
    return bytes(b), at


@pytest.mark.parametrize("M", CAPS, ids=lambda M: f"M{M}")
@pytest.mark.parametrize("name", ["abc", "zeros", "ab_lorem", "far_plant"])
def test_probe_under_a_scan_cap(name, M):
    """With max_bucket_scan the cap cuts inside the window: the runs' searches must use the first position the cap
    leaves (bucket_pos[lo]), not the window floor.  The case tells the two apart where the oracle's list without the
    cap holds a MATCH whose hit lies inside the window and beyond the cap.  A cap of 1 does that on every input.  Caps
    of 64 and 65 cannot on the periodic inputs, where the nearest hits are always the cheapest, nor on the text, where
    no bigram has 64 hits in the window: there the cases pin the second pass's searches for bucket_pos[lo] in runs of
    thousands of entries, and the oracle-only check is not worked out; far_plant is the input on which they do."""
    D = 5000
    if name == "far_plant":
        data, t = far_plant_input()
        slab = literal_slab(len(data))
        slabs = [("literal", slab, walk(slab))]
        extra = [t + d for d in (-2, -1, 0, 1, 2)]
    else:
        data, slabs = case(name)
        extra = []
    n = len(data)
    sa = binding.SA(data, neighbours_per_step=8, dict_limit=D, max_bucket_scan=M)
    o = Oracle(data, dict_limit=D, max_bucket_scan=M)
    o_floor = Oracle(data, dict_limit=D)  # what a search for the floor would admit
    ob = Oracle(data)
    excluded, tells_apart = 0, M == 1 or name == "far_plant"
    for kind, slab, w in slabs:
        ps = sorted(set(probe_positions(w, n, D, 30, seed=M + len(w))) | set(extra))
        same_as_oracle(sa, o, slab, ps, what=(name, kind, M))
        for p in ps if tells_apart else ():
            # from the oracle alone: a MATCH of the uncapped list whose hit lies inside the window and beyond the cap
            qs = np.unique(ob.substrings(p, max_len=2)[0]).astype(np.int64)
            qs = qs[p - qs - 1 < D]
            dropped = {int(q) for q in qs[:-M]}
            if not dropped:
                continue
            capped = set(as_list(o.top_k(slab, p, mode=1, k=20)[0]))
            for t_, d, ln in as_list(o_floor.top_k(slab, p, mode=1, k=20)[0]):
                excluded += t_ == MATCH and (p - d - 1) in dropped and (t_, d, ln) not in capped
    if tells_apart:
        assert excluded > 0
    sa.close()


class MemoOracle:
    """The oracle's neighbours of a (slab, step), worked out once: both engines are held against the same ones (on
    the 24 KiB input the oracle takes 60 ms for each)"""
    _store = {}

    def __init__(self, o, key):
        self._o, self._key = o, key

    def __getattr__(self, name):
        return getattr(self._o, name)

    def neighbour(self, slab, seed, step, j, keep=False, K=None):
        key = (self._key, hash(slab.tobytes()), seed, step, j, K)
        if key not in self._store:
            self._store[key] = self._o.neighbour(slab, seed, step, j, keep=keep, K=K)
        return self._store[key]


@pytest.mark.parametrize("engine", ["split", "one_kernel"])
@pytest.mark.parametrize("D", [256, 5000], ids=lambda D: f"D{D}")
@pytest.mark.parametrize("name", ["abc", "enwik6000"])
def test_split_pick_neighbours(name, D, engine, monkeypatch):
    """Every neighbour of a step == the oracle, cost and journal, at K = 64: the split pick (plan in front of the
    model load) and the one-kernel form (set-up in place) on the same steps, from the literal slab and from an
    evolved one."""
    if engine == "one_kernel":
        monkeypatch.setenv("MGL_NO_SPLIT", "1")
    else:
        monkeypatch.setenv("MGL_NO_ADAPT", "1")  # stay in the split form whatever the device's timing recommends after the run
    data = make_input("abc") if name == "abc" else corpus.enwik_like(6000, 0x5C)
    n, K, seed = len(data), 64, 41
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=seed, dict_limit=D)
    o = MemoOracle(Oracle(data, dict_limit=D), (name, D))
    base = literal_slab(n)
    sa.set_slab(P(base))
    for step in (0, 5):
        _check_neighbours(sa, o, base, seed, step, K)
    sa.run(30)
    cur, cost = sa.current()
    evolved = cur.astype(base.dtype)
    assert len(walk(evolved)) < n - 200  # the base carries matches
    assert cost == o.cost_slab(evolved)["total"]
    for step in (30, 31):
        _check_neighbours(sa, o, evolved, seed, step, K)
    sa.close()
