"""Every refusal of the device's slab validation, and the state of a handle after one.

A slab that does not come out of the search reaches the device through mgl_sa_set_slab, mgl_sa_set_best,
mgl_sa_adopt_best_packed (the exchanges' hand-over) and the parity hooks.  k_validate (csrc/mgl_kernels3.hip) is the only
device code that compares such a slab with the input; the walks in front of it decide what is a packet at all
(mgl_pk_wellformed, csrc/mgl_model.h).  The table of tests/_validity.py holds, for every clause of the rule, slabs that
violate that clause alone, each next to an accepted twin (tests/test_validity_rule_cpu.py checks the table itself and runs
it through the host's gate); here the device must refuse exactly the refused ones, by every way in, and be as the header
says afterwards (include/megalania_hip.h, "after a refusal").  n = 773, window 256; costs are integer sums and slabs are
compared entry for entry: every comparison is exact.

No test here searches (mgl_sa_run) from a slab of the table: the search's walks re-join the slab through entries that
were off its walk and take them as they are (as the reference's do: there a stale entry once was a packet of a valid
parse), so a slab to search from needs such entries off its walk too, and the table's are stale on purpose (wrong sources,
and in `poison` no packets at all).  The searches after a refusal start from the all-literal slab.  `-m gpu`."""
import functools
import lzma

import numpy as np
import pytest

import _validity as V
from _libs import Oracle, literal_slab
from megalania_amd import binding

pytestmark = pytest.mark.gpu

DATA, BASE, CASES = V.cases()
BY_ID = {c.id: c for c in CASES}
PROPS = [(0, 0, 0), (2, 1, 2)]
LIT = literal_slab(V.N)
EINVAL = -1


@functools.lru_cache(maxsize=None)
def oracle(props):
    return Oracle(DATA, *props, dict_limit=V.DICT_LIMIT)


@functools.lru_cache(maxsize=None)
def oracle_cost(props, cid):
    """the CPU oracle's walk of a valid slab: total, final ctx_state and rep distances.  Computed once per slab."""
    slab = LIT if cid == "literal" else BY_ID[cid].slab
    r = oracle(props).cost_slab(V.as_slab(slab))
    return r["total"], r["ctx_state"], tuple(int(x) for x in r["dists"])


def handle(props):
    return binding.SA(DATA, neighbours_per_step=64, seed=5, lc=props[0], lp=props[1], pb=props[2], dict_limit=V.DICT_LIMIT)


def same(a, b):
    return all((a[f] == b[f]).all() for f in ("type", "dist", "len"))


def alternating(cases):
    """accepted and refused cases in turn, so that every refusal is followed by work on the same handle"""
    ok = [c for c in cases if c.clause is None]
    bad = [c for c in cases if c.clause is not None]
    out = []
    for i in range(max(len(ok), len(bad))):
        out += ok[i:i + 1] + bad[i:i + 1]
    return out


def packed(slab):
    return slab["dist"].astype(np.uint64) | (slab["len"].astype(np.uint64) << np.uint64(32)) | (slab["type"].astype(np.uint64) << np.uint64(48))


def assert_current_is_literal(sa, props):
    cur, cost = sa.current()
    assert same(cur, LIT) and cost == oracle_cost(props, "literal")[0]


@pytest.mark.parametrize("props", PROPS, ids=lambda p: "lc%d-lp%d-pb%d" % p)
def test_set_slab_refuses_exactly_what_the_rule_refuses(props):
    """One handle for the whole table.  Accepted: the slab is the current one entry for entry (stale entries too) at the
    oracle's cost, and the emitter's stream of it decodes.  Refused: MGL_EINVAL, the current slab is the all-literal one
    at its exact cost, the best slab and its cost are untouched, and the search runs on."""
    sa = handle(props)
    assert sa.run(2)["best_cost"] > 0  # there is a best slab for the refusals to leave alone
    for c in alternating(CASES):
        if c.clause is None:
            sa.set_slab(c.slab)
            cur, cost = sa.current()
            assert same(cur, c.slab), c.id
            assert cost == oracle_cost(props, c.id)[0], c.id
            assert lzma.decompress(binding.emit_stream(DATA, cur, *props), format=lzma.FORMAT_ALONE) == DATA, c.id
            continue
        best, best_cost = sa.best()
        with pytest.raises(binding.MglError) as e:
            sa.set_slab(c.slab)
        assert e.value.rc == EINVAL, c.id
        assert_current_is_literal(sa, props)
        after, after_cost = sa.best()
        assert same(after, best) and after_cost == best_cost, c.id
        st = sa.run(2)
        assert st["steps"] == 2 and 0 < st["current_cost"] and 0 < st["best_cost"] <= best_cost, (c.id, st)
    sa.close()


@pytest.mark.parametrize("via", ["adopt_best_packed", "set_best"])
@pytest.mark.parametrize("props", PROPS, ids=lambda p: "lc%d-lp%d-pb%d" % p)
def test_an_adopted_best_slab_is_compared_with_the_input_when_an_epoch_starts_from_it(props, via):
    """The cost that comes with the slab is the device's own mgl_cost_slab of that very slab, which the walk gives for
    every case whose entries are packets (lines 6 to 13 of the table): the cost comparison cannot refuse it, only the
    comparison with the input bytes can.  Refused: MGL_EINVAL, no best slab any more, the current slab all-literal, and
    the search runs on.  Accepted: the epoch starts at that slab and that cost."""
    sa = handle(props)

    def adopt(slab, cost):
        if via == "set_best":
            sa.set_best(slab, cost)
        else:
            sa.adopt_best_packed(packed(slab), cost)

    for c in alternating([c for c in CASES if 6 <= c.line <= 13 or c.id in ("base", "poison")]):
        cost = sa.cost_slab(c.slab, want_cum=False)["total"]
        adopt(c.slab, cost)
        assert sa.best_cost() == cost
        if c.clause is None:
            sa.begin_epoch(1, from_best=True)
            cur, cur_cost = sa.current()
            assert same(cur, c.slab) and cur_cost == cost == oracle_cost(props, c.id)[0], c.id
            continue
        with pytest.raises(binding.MglError) as e:
            sa.begin_epoch(1, from_best=True)
        assert e.value.rc == EINVAL, c.id
        best, best_cost = sa.best()
        assert best_cost == 0 and same(best, LIT), c.id  # cost 0: "none", what the next exchange publishes
        assert_current_is_literal(sa, props)
        st = sa.run(2)
        assert st["steps"] == 2 and st["best_cost"] > 0, (c.id, st)
    # the cost comparison alone: the right slab with a cost one too high (mgl_sa_set_best compares at once)
    cost = oracle_cost(props, "base")[0]
    with pytest.raises(binding.MglError) as e:
        adopt(BASE, cost + 1)
        sa.begin_epoch(1, from_best=True)
    assert e.value.rc == EINVAL
    adopt(BASE, cost)
    sa.begin_epoch(1, from_best=True)
    assert sa.current()[1] == cost
    sa.close()


@pytest.mark.parametrize("props", PROPS, ids=lambda p: "lc%d-lp%d-pb%d" % p)
def test_the_walks_of_the_parity_hooks_refuse_what_is_no_packet(props):
    """mgl_cost_slab, mgl_props_sweep, mgl_final_state and mgl_crossover (the case as the first and as the last parent) on
    lines 1 to 5 of the table, their accepted twins and the slab with poison off its walk: an entry that is no packet, or
    does not fit, is refused by all of them with one code, and the handle costs the base parse as before.  Whether these
    hooks accept a slab whose packets have wrong sources is left open by the header and not pinned here."""
    sa = handle(props)
    triple = binding.PROPS_TRIPLES.index(props)
    other = BY_ID["long-rep-len273"].slab
    base_cost = oracle_cost(props, "base")[0]
    for c in alternating([c for c in CASES if c.line <= 5 or c.id == "poison"]):
        s = c.slab
        if c.clause is None:
            want, ctx_state, dists = oracle_cost(props, c.id)
            assert sa.cost_slab(s)["total"] == want, c.id
            assert int(sa.props_sweep(s)[0][triple]) == want, c.id
            fs = sa.final_state(s)
            assert (fs["ctx_state"], tuple(int(x) for x in fs["dists"])) == (ctx_state, dists), c.id
            assert sa.crossover([s, BASE])[1]["parent_cost"] == [want, base_cost], c.id
            assert sa.crossover([BASE, other, s])[1]["parent_cost"][2] == want, c.id
            continue
        codes = []
        for call in (lambda: sa.cost_slab(s), lambda: sa.props_sweep(s), lambda: sa.final_state(s),
                     lambda: sa.crossover([s, BASE]), lambda: sa.crossover([BASE, other, s])):
            with pytest.raises(binding.MglError) as e:
                call()
            codes.append(e.value.rc)
        assert len(set(codes)) == 1 and codes[0] is not None and codes[0] < 0, (c.id, codes)
        assert sa.cost_slab(BASE)["total"] == base_cost, c.id
    sa.close()
