"""Random valid parses with stale entries (tests/_random_parse.py) as starting points of the incremental engine: that the
generator makes what it says -- valid parses that reach the expensive corners of the packet space --, that stale entries
really come onto the walks of the neighbours generated from them, and that every drop rule of the device fires among the
neighbours that tests/test_gpu_random_parse.py compares.  The oracle only: runs wherever the tests run."""
import lzma

import numpy as np
import pytest

import _random_parse as rp
from _libs import LITERAL, LONG_REP, MATCH, SHORT_REP, Oracle, walk
from conftest import sha_slab
from megalania_amd import binding

ALL = list(rp._SPECS)


def test_the_generator_is_pinned():
    """one (data, seed, settings) names one slab, whatever the Python: the draws are the project's counter RNG"""
    assert sha_slab(rp.base("enwik4k")[1]) == "290a17f498ccf35812c2142889df7c9a219426063d8a0958fdb1bc8973eff020"
    assert sha_slab(rp.base("one_period")[1]) == "6c7f9649baf0111b26b603905e721d48aa43d783d65016d98c7e916dc83941b1"
    data, slab = rp.base("lorem3k")
    again = rp.random_parse(data, 12, rp.TEXT, "any")
    assert (again == slab).all()
    bare = rp.random_parse(data, 12, rp.TEXT, "any", stale=False)
    on = rp.on_walk(bare)
    assert (bare["type"][~on] == LITERAL).all() and (bare["len"][~on] == 1).all()


@pytest.mark.parametrize("props", [{}, rp.ALT_PROPS], ids=["lc0lp0pb0", "lc2lp1pb2"])
@pytest.mark.parametrize("name", ALL)
def test_every_slab_is_a_valid_parse(name, props):
    data, slab = rp.base(name)
    o = Oracle(data, dict_limit=rp.dict_limit_of(name), **props)
    stream = o.emit(slab)
    assert lzma.decompress(stream, format=lzma.FORMAT_ALONE) == data
    assert binding.emit_stream(data, slab, **props) == stream
    far = [int(slab[p]["dist"]) for p in walk(slab) if slab[p]["type"] == MATCH]
    assert max(far) < rp.dict_limit_of(name)


def test_stale_entries_are_what_the_reference_could_hold():
    """off the walk: a MATCH that reproduces the input at its position inside the window, a LONG_REP of index 0..3 and a
    length that stays inside the input, a SHORT_REP or a literal -- and all four kinds occur on every base"""
    for name in ALL:
        data, slab = rp.base(name)
        n, lim = len(data), rp.dict_limit_of(name)
        off = np.nonzero(~rp.on_walk(slab))[0]
        kinds = set()
        for p in off:
            t, d, l = int(slab[p]["type"]), int(slab[p]["dist"]), int(slab[p]["len"])
            kinds.add(t)
            if t == MATCH:
                assert d < lim and d < p and 2 <= l <= min(273, n - p) and data[p:p + l] == bytes(data[p - d - 1 + k] for k in range(l)), (name, p)
            elif t == LONG_REP:
                assert d < 4 and 2 <= l <= min(273, n - p), (name, p)
            else:
                assert t in (LITERAL, SHORT_REP) and d == 0 and l == 1, (name, p)
        assert kinds == {LITERAL, MATCH, SHORT_REP, LONG_REP}, name


def test_the_walks_reach_the_expensive_corners():
    """all four LONG_REP indices, SHORT_REP, lengths 2 and 273, a MATCH with at least 8 direct bits (a distance of 8 192 or
    more: the 9 500-byte base is there for it), every ctx_state in front of some packet -- and, what no cheap parse has,
    every ctx_state in front of every packet type"""
    long_rep, lens, states = set(), set(), set()
    short_rep = direct8 = False
    for name in ALL:
        data, slab = rp.base(name)
        tr = Oracle(data).trace_events(slab)
        for p, st in zip(tr["pk_pos"], tr["pk_state"][:, 0]):
            t, d, l = int(slab[p]["type"]), int(slab[p]["dist"]), int(slab[p]["len"])
            states.add((int(st), t))
            lens.add(l)
            short_rep |= t == SHORT_REP
            if t == LONG_REP:
                long_rep.add(d)
            direct8 |= t == MATCH and d >= 8192
    assert long_rep == {0, 1, 2, 3} and short_rep and {2, 273} <= lens and direct8
    assert {s for s, _ in states} == set(range(12))
    assert states == {(s, t) for s in range(12) for t in (LITERAL, MATCH, SHORT_REP, LONG_REP)}


@pytest.mark.parametrize("name", [b for b in rp.BASES if len(rp._SPECS[b][0]()) >= 2600])
def test_stale_entries_go_live(name):
    """Over the neighbours the GPU tests compare (steps 0 and 5, K = 128): at least 60 % have status ok, and at least 10 %
    of those bring a stale non-literal entry onto their walk unchanged -- a position on the neighbour's walk, off the base's,
    not in the journal, holding a MATCH or a rep.  (Measured, as ok share / live share: enwik4k 86 / 11, lorem3k 62 / 22,
    doubled 96 / 18, two_periods 99 / 20, enwik4k_matches 84 / 13, one_period 68 / 15 per cent.)"""
    data, slab = rp.base(name)
    o = Oracle(data, dict_limit=rp.dict_limit_of(name))
    base_on = rp.on_walk(slab)
    ok = live = 0
    for step in rp.STEPS:
        for j, row in enumerate(rp.oracle_neighbours(name, step)):
            if row[0] != 1:
                continue
            ok += 1
            kept = slab.copy()
            st, _, diffs, _ = o.neighbour_ex(kept, rp.SEED, step, j, keep=True, K=rp.K)
            assert st == 1
            fresh = rp.on_walk(kept) & ~base_on
            fresh[diffs["position"]] = False
            live += bool((kept["type"][fresh] != LITERAL).any())
    print(f"{name}: ok {ok}/{2 * rp.K}, stale entries live in {live} ({100 * live // max(ok, 1)} %)")
    assert ok * 100 >= 60 * 2 * rp.K, (ok, live)
    assert live * 100 >= 10 * ok, (ok, live)


def test_every_drop_rule_fires():
    """The device gives a neighbour up when its journal needs more than 64 positions, its repair more than 8 top-K picks, its
    walk more than 2 048 packets or its change lists more than 4 096 events; the oracle says which (orc_last_drop_reason).
    Each rule fires among the neighbours of steps 0 and 5 that the GPU tests compare: the repair picks on `doubled`, the
    journal on `two_periods`, and journal, walk length and event lists on `one_period` (the event lists are within reach
    after all: a rep-dominated walk of a strictly periodic input).  Status values stay what they were."""
    total = {}
    for name in rp.BASES:
        rows = [r for step in rp.STEPS for r in rp.oracle_neighbours(name, step)]
        assert all((r[4] != 0) == (r[0] == -1) for r in rows), name
        assert all(r[1] == (1 << 64) - 1 and len(r[2]) == 0 for r in rows if r[0] != 1), name
        total[name] = rp.drop_counts(rows)
        print(name, total[name])
    assert total["doubled"]["repair_picks"] >= 1
    assert total["two_periods"]["journal"] >= 1
    assert total["one_period"]["journal"] >= 1 and total["one_period"]["walk"] >= 1 and total["one_period"]["events"] >= 1
