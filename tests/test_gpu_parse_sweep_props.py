"""The parse sweep with a triple per variant (`mgl_parse_sweep_props`, SA.parse_sweep_props, CLI --props-joint): variant v
has to be, integer for integer, the parse that `seed_adaptive` makes on a fresh handle created with props[v] and set to
that variant's match finder, whatever the triple of the handle the sweep runs on; the winner is the cheapest of them with
ties to the lower variant and then the lower pass; the handle's search state stays as it was.  `-m gpu`."""
import functools
import lzma
import subprocess

import numpy as np
import pytest

from _libs import Oracle, literal_slab
from megalania_amd import binding, build, corpus
from test_gpu_optimal import MATCH, SMALL, as_list, greedy_slab
from test_gpu_parse_sweep import MEMBERS

pytestmark = pytest.mark.gpu

N, F = binding.MF_NEAREST, binding.MF_FRONTIER
FIELDS = ("cost", "objective", "best_pass", "greedy_cost", "passes")
TRIPLES = [(0, 0, 0), (3, 0, 2), (0, 2, 0), (4, 0, 4), (1, 3, 1), (2, 0, 1)]  # small and largest models in one launch
DEFAULT_SWEEP = binding.DEFAULT_SWEEP


def _sa(data, **kw):
    return binding.SA(data, accept="single", neighbours_per_step=16, **kw)


def _oracle_cost(data, slab, props, dict_limit=0x400000):
    lc, lp, pb = props
    o = Oracle(data, lc=lc, lp=lp, pb=pb, dict_limit=dict_limit)
    return o.cost_slab(np.ascontiguousarray(slab).astype(literal_slab(1).dtype))["total"]


def _argmin(results):
    """(variant, pass) of the cheapest cost: ties to the lower variant, then to the lower pass"""
    best, at = None, None
    for v, r in enumerate(results):
        for p, c in enumerate(r["cost"]):
            if best is None or c < best:
                best, at = c, (v, p)
    return at, best


@functools.lru_cache(maxsize=None)
def _alone(data, variant, props, dict_limit=0, passes=2, chunk=1000):
    """the variant on a fresh handle at its own triple: (stats, current slab as a list, its cost)"""
    finder, cand, segment, ahead = variant
    lc, lp, pb = props
    sa = _sa(data, lc=lc, lp=lp, pb=pb, dict_limit=dict_limit)
    sa.set_match_finder(finder, 0)
    st = sa.seed_adaptive(passes=passes, cand=cand, chunk=chunk, segment=segment, ahead=ahead)
    cur, cost = sa.current()
    sa.close()
    return st, as_list(cur), cost


def _check_winner(data, sw, props, dict_limit=0x400000):
    (bv, bp), bc = _argmin(sw["results"])
    assert sw["best_variant"] == bv and sw["results"][bv]["best_pass"] == bp
    assert bc == _oracle_cost(data, sw["slab"], props[bv], dict_limit)
    lc, lp, pb = props[bv]
    assert lzma.decompress(binding.emit_stream(data, sw["slab"], lc=lc, lp=lp, pb=pb), format=lzma.FORMAT_ALONE) == data
    return bv, bc


def _check_sweep_equals_members(data, handle_props, dict_limit=0):
    lc, lp, pb = handle_props
    sa = _sa(data, lc=lc, lp=lp, pb=pb, dict_limit=dict_limit)
    sw = sa.parse_sweep_props(MEMBERS, TRIPLES, passes=2, chunk=1000)
    sa.close()
    alone = [_alone(data, m, t, dict_limit) for m, t in zip(MEMBERS, TRIPLES)]
    assert len(sw["results"]) == len(MEMBERS)
    for v, (st, _, _) in enumerate(alone):
        for k in FIELDS:
            assert sw["results"][v][k] == st[k], (handle_props, MEMBERS[v], TRIPLES[v], k)
        assert len(sw["results"][v]["ms"]) == 2
    (bv, bp), bc = _argmin([a[0] for a in alone])
    assert sw["best_variant"] == bv and sw["results"][bv]["best_pass"] == bp
    assert bc == alone[bv][2] and as_list(sw["slab"]) == alone[bv][1]
    _check_winner(data, sw, TRIPLES, dict_limit or 0x400000)
    assert sw["gpu_ms"] > 0
    return as_list(sw["slab"])


@pytest.mark.parametrize("name,data", SMALL[1:3], ids=[s[0] for s in SMALL[1:3]])
@pytest.mark.parametrize("handle_props", [(0, 0, 0), (2, 0, 1)], ids=["at000", "at201"])
def test_a_sweep_equals_its_members_across_triples(name, data, handle_props):
    _check_sweep_equals_members(data, handle_props)


def test_a_sweep_equals_its_members_under_a_window():
    cur = _check_sweep_equals_members(SMALL[1][1], (0, 0, 0), dict_limit=300)
    assert all(t != MATCH or d < 300 for t, d, _ in cur)


@pytest.mark.parametrize("props", [(0, 0, 0), (3, 0, 2)], ids=["at000", "at302"])
def test_all_triples_equal_to_the_handles(props):
    data = corpus.enwik_like(3000, 0x33)
    lc, lp, pb = props
    twin = _sa(data, lc=lc, lp=lp, pb=pb)
    want = twin.seed_sweep(DEFAULT_SWEEP, passes=2, chunk=1000)
    cur, cost = twin.current()
    twin.close()
    sa = _sa(data, lc=lc, lp=lp, pb=pb)
    sw = sa.parse_sweep_props(DEFAULT_SWEEP, [props] * 16, passes=2, chunk=1000)
    sa.close()
    for v in range(16):
        assert all(sw["results"][v][k] == want["results"][v][k] for k in FIELDS), v
    assert sw["best_variant"] == want["best_variant"] and as_list(sw["slab"]) == as_list(cur)
    assert sw["results"][sw["best_variant"]]["cost"][sw["results"][sw["best_variant"]]["best_pass"]] == cost


def test_the_search_state_is_untouched():
    data = corpus.enwik_like(3000, 0x33)
    handles = [binding.SA(data, accept="single", neighbours_per_step=64, seed=7, iters_per_epoch=200) for _ in range(2)]
    sa, twin = handles
    for h in handles:
        h.seed_greedy(8)
        h.run(10)
    cur, cur_cost = sa.current()
    bst, bst_cost = sa.best()
    sw = sa.parse_sweep_props([(N, 16, 64, 128), (F, 16, 64, 128), (F, 8, 32, 273), (N, 1, 300, 0)],
                              [(3, 0, 2), (4, 0, 4), (0, 2, 0), (1, 3, 1)], passes=2, chunk=1000)
    assert sw["best_variant"] is not None
    after, after_cost = sa.current()
    assert after_cost == cur_cost and as_list(after) == as_list(cur)
    after, after_cost = sa.best()
    assert after_cost == bst_cost and as_list(after) == as_list(bst)
    for s in range(10):
        assert sa.run(1)["current_cost"] == twin.run(1)["current_cost"], s
    twin.close()
    parse_in = greedy_slab(data)[0]
    fresh = _sa(data)
    want, want_obj = fresh.adaptive_pass(parse_in, 16, 1000, 64, 128)
    fresh.close()
    got, obj = sa.adaptive_pass(parse_in, 16, 1000, 64, 128)  # the nearest rule's: the finder selection was left alone
    sa.close()
    assert obj == want_obj and as_list(got) == as_list(want)


@pytest.mark.parametrize("data", [b"x", b"ab", b"a" * 3000], ids=["n1", "n2", "run"])
def test_edge_inputs(data):
    props = [(0, 0, 0), (3, 0, 2), (0, 4, 4), (2, 2, 1)]
    sa = _sa(data)
    sw = sa.parse_sweep_props(DEFAULT_SWEEP[:4], props, passes=2, chunk=1000)
    sa.close()
    _check_winner(data, sw, props)
    for v in range(4):
        st, _, _ = _alone(data, DEFAULT_SWEEP[v], props[v])
        assert all(sw["results"][v][k] == st[k] for k in FIELDS), v


def test_sixty_four_variants():
    data = corpus.enwik_like(3000, 0x33)
    triples = [(1, 0, 1), (0, 0, 0), (4, 0, 0), (0, 1, 3)]
    lc, lp, pb = triples[0]
    twin = _sa(data, lc=lc, lp=lp, pb=pb)
    want = twin.seed_sweep(DEFAULT_SWEEP, passes=2, chunk=1000)
    twin.close()
    props = [t for t in triples for _ in range(16)]
    sa = _sa(data, lc=lc, lp=lp, pb=pb)
    sw = sa.parse_sweep_props(DEFAULT_SWEEP * 4, props, passes=2, chunk=1000)
    sa.close()
    assert len(sw["results"]) == 64
    for v in range(16):
        assert all(sw["results"][v][k] == want["results"][v][k] for k in FIELDS), v
    (bv, _), bc = _argmin(sw["results"])
    assert sw["best_variant"] == bv
    lc, lp, pb = props[bv]
    fresh = _sa(data, lc=lc, lp=lp, pb=pb)
    assert fresh.cost_slab(sw["slab"], want_cum=False)["total"] == bc
    fresh.close()


def test_ties_go_to_the_lower_variant():
    data = corpus.enwik_like(3000, 0x33)
    sa = _sa(data)
    sw = sa.parse_sweep_props([(N, 16, 64, 128), (F, 16, 64, 128), (F, 16, 64, 128)], [(0, 0, 0), (3, 0, 2), (3, 0, 2)],
                              passes=2, chunk=1000)
    sa.close()
    assert sw["results"][1]["cost"] == sw["results"][2]["cost"]
    (bv, _), _ = _argmin(sw["results"])
    assert sw["best_variant"] == bv != 2
    sa = _sa(data)
    sw = sa.parse_sweep_props([(F, 16, 64, 128)] * 2, [(3, 0, 2)] * 2, passes=2, chunk=1000)
    sa.close()
    assert sw["results"][0]["cost"] == sw["results"][1]["cost"] and sw["best_variant"] == 0


def test_bad_arguments_are_refused_and_the_handle_still_works():
    data = corpus.lorem(2048)
    sa = _sa(data)
    sa.seed_greedy(8)
    before, before_cost = sa.current()
    ok, p0 = [(N, 16, 64, 128)], [(0, 0, 0)]
    for variants, props, kw in ((ok, [(3, 2, 0)], {}), (ok, [(0, 0, 5)], {}), (ok, p0, dict(from_current=True)), ([], [], {}),
                                (ok * 65, p0 * 65, {}), (ok * 2, p0, {}), ([(2, 16, 64, 128)], p0, {}), ([(N, 31, 64, 128)], p0, {}),
                                ([(N, 16, 64, 274)], p0, {}), (ok, p0, dict(chunk=511)), (ok, p0, dict(passes=17)),
                                (ok, p0, dict(depth=4097))):
        with pytest.raises(binding.MglError) as e:
            sa.parse_sweep_props(variants, props, **kw)
        assert e.value.rc == -1, (variants[:1], props[:1], kw)
        after, after_cost = sa.current()
        assert after_cost == before_cost and as_list(after) == as_list(before)
        sa.adaptive_pass(literal_slab(len(data)), 8, 4096, 64, 128)  # and the handle still works
    sa.close()


def _joint_rule(data, passes, T):
    """section "--props-joint" of DESIGN.md 10, run through the binding: (triple, stage, grid index, pass, cost, stage A's cost, candidates)"""
    s = (0, 0, 0)
    sa = _sa(data)
    a = sa.parse_sweep_props(DEFAULT_SWEEP, [s] * 16, passes=passes)
    va = a["best_variant"]
    c_a = a["results"][va]["cost"][a["results"][va]["best_pass"]]
    table = [int(c) for c in sa.props_sweep(a["slab"])[0]]
    t_star = table.index(min(table))
    order = sorted((t for t in range(75) if binding.PROPS_TRIPLES[t] != s), key=lambda t: (table[t], t))
    cands = [binding.PROPS_TRIPLES[t] for t in order[:T]]
    b = sa.parse_sweep_props(DEFAULT_SWEEP * T, [c for c in cands for _ in range(16)], passes=passes)
    sa.close()
    vb = b["best_variant"]
    c_b = b["results"][vb]["cost"][b["results"][vb]["best_pass"]]
    pairs = [(c_a, s, "A", va, a["results"][va]["best_pass"]),
             (table[t_star], binding.PROPS_TRIPLES[t_star], "A-recosted", va, a["results"][va]["best_pass"]),
             (c_b, cands[vb // 16], "B", vb % 16, b["results"][vb]["best_pass"])]
    cost, triple, stage, variant, best_pass = min(pairs, key=lambda p: p[0])  # min keeps the first of equals
    return triple, stage, variant, best_pass, cost, c_a, cands


def test_cli_props_joint(tmp_path):
    data = corpus.enwik_like(5000, 0x35)
    f = tmp_path / "in.bin"
    f.write_bytes(data)
    out = tmp_path / "out.lzma"
    r = subprocess.run([build.CLI, "--props", "auto", "--adaptive-seed", "2", "--parse-sweep", "--props-joint", "3", "--parse-sweep-table",
                        "--epochs", "1", "--phases", "1", "--steps", "20", "-o", str(out), str(f)], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-400:]
    err = r.stderr.decode().splitlines()
    stream = out.read_bytes()
    assert lzma.decompress(stream, format=lzma.FORMAT_ALONE) == data
    line = next(l for l in err if l.startswith("props: "))
    lc, lp, pb = (int(line.split(k + "=")[1].split()[0].rstrip(",")) for k in ("lc", "lp", "pb"))
    assert stream[0] == (pb * 5 + lp) * 9 + lc, line
    triple, stage, variant, best_pass, cost, c_a, cands = _joint_rule(data, 2, 3)
    joint = next(l for l in err if l.startswith("props joint: "))
    want = (f"props joint: lc={triple[0]} lp={triple[1]} pb={triple[2]} stage {stage} variant {variant} pass {best_pass} cost {cost}; "
            f"stage A cost {c_a}; candidates " + " ".join("%d/%d/%d" % c for c in cands))
    assert joint == want
    assert (lc, lp, pb) == triple
    table = [l for l in err if l.startswith("parse-sweep-table:")]
    assert len(table) == 16 * (1 + 3)
    for k, c in enumerate([(0, 0, 0)] + cands):
        assert all(f"lc={c[0]} lp={c[1]} pb={c[2]} " in l for l in table[16 * k:16 * k + 16]), (k, c)
