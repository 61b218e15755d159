"""The adaptive parse under several settings at once (`mgl_sa_seed_sweep`, SA.seed_sweep, CLI --parse-sweep): every
variant has to be the parse that `seed_adaptive` makes on a fresh handle set to that variant's match finder, the winner
the cheapest of them with ties to the lower variant and then the lower pass, and what the call leaves in the handle is
pinned by the oracle's costing, by the oracle's batched SA continuing from it, and by liblzma.  `-m gpu`."""
import functools
import lzma
import statistics
import subprocess

import numpy as np
import pytest

from _libs import Oracle, literal_slab
from megalania_amd import binding, build, corpus
from test_gpu_optimal import MATCH, SMALL, as_list, greedy_slab

pytestmark = pytest.mark.gpu

N, F = binding.MF_NEAREST, binding.MF_FRONTIER
MEMBERS = [(N, 16, 64, 128), (F, 16, 64, 128), (N, 1, 300, 0), (F, 8, 32, 273), (N, 16, 1000, 128), (F, 1, 128, 0)]
FIELDS = ("cost", "objective", "best_pass", "greedy_cost", "passes")


def _sa(data, **kw):
    return binding.SA(data, accept="single", neighbours_per_step=16, **kw)


def _oracle_cost(data, slab, lc=0, lp=0, pb=0, dict_limit=0x400000):
    o = Oracle(data, lc=lc, lp=lp, pb=pb, dict_limit=dict_limit)
    return o.cost_slab(np.ascontiguousarray(slab).astype(literal_slab(1).dtype))["total"]


def _argmin(results, floor=None):
    """(variant, pass) of the cheapest cost: ties to the lower variant, then to the lower pass; `floor`: what has to be beaten"""
    best, at = floor, None
    for v, r in enumerate(results):
        for p, c in enumerate(r["cost"]):
            if best is None or c < best:
                best, at = c, (v, p)
    return at, best


def _alone(data, variant, depth=0, sa_kw=None, **kw):
    """the variant on a handle of its own: (stats, current slab as a list, its cost)"""
    finder, cand, segment, ahead = variant
    sa = _sa(data, **(sa_kw or {}))
    sa.set_match_finder(finder, depth)
    st = sa.seed_adaptive(cand=cand, segment=segment, ahead=ahead, **kw)
    cur, cost = sa.current()
    sa.close()
    return st, as_list(cur), cost


def _check_sweep_equals_members(data, lc=0, lp=0, pb=0, dict_limit=0x400000):
    sa_kw = dict(lc=lc, lp=lp, pb=pb, dict_limit=dict_limit)
    sa = _sa(data, **sa_kw)
    sw = sa.seed_sweep(MEMBERS, passes=2, chunk=1000)
    cur, cost = sa.current()
    sa.close()
    alone = [_alone(data, m, sa_kw=sa_kw, passes=2, chunk=1000) for m in MEMBERS]
    assert len(sw["results"]) == len(MEMBERS)
    for v, (st, _, _) in enumerate(alone):
        for k in FIELDS:
            assert sw["results"][v][k] == st[k], (MEMBERS[v], k)
        assert len(sw["results"][v]["ms"]) == 2
    (bv, bp), bc = _argmin([a[0] for a in alone])
    assert sw["best_variant"] == bv and sw["results"][bv]["best_pass"] == bp
    assert cost == bc == alone[bv][2] and as_list(cur) == alone[bv][1]
    assert cost == _oracle_cost(data, cur, lc, lp, pb, dict_limit)
    assert lzma.decompress(binding.emit_stream(data, cur, lc=lc, lp=lp, pb=pb), format=lzma.FORMAT_ALONE) == data
    assert sw["gpu_ms"] > 0
    return as_list(cur)


@pytest.mark.parametrize("name,data", SMALL[:4], ids=[s[0] for s in SMALL[:4]])
def test_a_sweep_equals_its_members(name, data):
    _check_sweep_equals_members(data)


def test_a_sweep_equals_its_members_at_other_properties_and_under_a_window():
    data = SMALL[1][1]
    _check_sweep_equals_members(data, lc=3, lp=0, pb=2)
    cur = _check_sweep_equals_members(data, dict_limit=300)
    assert all(t != MATCH or d < 300 for t, d, _ in cur)


def test_one_variant_equals_the_adaptive_seed_at_its_defaults():
    data = corpus.enwik_like(3000, 0x33)
    sa = _sa(data)
    sw = sa.seed_sweep([(N, 0, 0, 0)])
    cur, cost = sa.current()
    sa.close()
    st, want, want_cost = _alone(data, (N, 0, 0, 0))
    assert sw["best_variant"] == 0 and all(sw["results"][0][k] == st[k] for k in FIELDS)
    assert cost == want_cost and as_list(cur) == want


def test_sixty_four_variants():
    data = corpus.enwik_like(3000, 0x33)
    variants = [MEMBERS[v % 6] for v in range(64)]
    sa = _sa(data)
    sw = sa.seed_sweep(variants, passes=2, chunk=1000)
    _, cost = sa.current()
    sa.close()
    assert len(sw["results"]) == 64
    for v in range(6, 64):
        assert all(sw["results"][v][k] == sw["results"][v % 6][k] for k in FIELDS), v
    (bv, _), bc = _argmin(sw["results"])
    assert sw["best_variant"] == bv < 6 and cost == bc


@pytest.mark.parametrize("data", [b"x", b"ab", b"a" * 3000], ids=["n1", "n2", "run"])
def test_sweep_on_edge_inputs(data):
    sa = _sa(data)
    sw = sa.seed_sweep(binding.DEFAULT_SWEEP)
    cur, cost = sa.current()
    sa.close()
    (bv, _), bc = _argmin(sw["results"])
    assert sw["best_variant"] == bv and cost == bc == _oracle_cost(data, cur)
    assert lzma.decompress(binding.emit_stream(data, cur), format=lzma.FORMAT_ALONE) == data
    st, want, want_cost = _alone(data, binding.DEFAULT_SWEEP[0])
    assert all(sw["results"][0][k] == st[k] for k in FIELDS) and cost <= want_cost


def test_ties_go_to_the_lower_variant():
    data = corpus.enwik_like(3000, 0x33)
    sa = _sa(data)
    sw = sa.seed_sweep([(F, 16, 64, 128), (F, 16, 64, 128)], passes=2)
    sa.close()
    assert sw["results"][0]["cost"] == sw["results"][1]["cost"] and sw["best_variant"] == 0


def test_bad_arguments_are_refused_and_the_handle_still_works():
    data = corpus.lorem(2048)
    sa = _sa(data)
    sa.seed_greedy(8)
    before, before_cost = sa.current()
    ok = [(N, 16, 64, 128)]
    for variants, kw in (([], {}), (ok * 65, {}), ([(2, 16, 64, 128)], {}), ([(N, 31, 64, 128)], {}), ([(N, 16, 64, 274)], {}),
                         (ok, dict(chunk=511)), (ok, dict(passes=17)), (ok, dict(depth=4097))):
        with pytest.raises(binding.MglError) as e:
            sa.seed_sweep(variants, **kw)
        assert e.value.rc == -1, (variants[:1], kw)
        after, after_cost = sa.current()
        assert after_cost == before_cost and as_list(after) == as_list(before)
        sa.adaptive_pass(literal_slab(len(data)), 8, 4096, 64, 128)  # and the handle still works
    sa.close()


def test_from_current_never_costs_more():
    data = corpus.enwik_like(3000, 0x33)
    sa = binding.SA(data, accept="single", neighbours_per_step=64, seed=7, iters_per_epoch=200)
    sa.seed_greedy(8)
    sa.run(40)
    for k in range(2):  # the second sweep runs on the first one's output
        before, before_cost = sa.current()
        sw = sa.seed_sweep(binding.DEFAULT_SWEEP, passes=2, from_current=True)
        after, after_cost = sa.current()
        assert all(r["greedy_cost"] == before_cost for r in sw["results"])
        assert after_cost <= before_cost
        at, bc = _argmin(sw["results"], floor=before_cost)
        if sw["best_variant"] is None:
            assert at is None
            assert after_cost == before_cost and as_list(after) == as_list(before)
            assert all(c >= before_cost for r in sw["results"] for c in r["cost"])
        else:
            assert at is not None and sw["best_variant"] == at[0] and after_cost == bc < before_cost
        assert after_cost == _oracle_cost(data, after)
        print(f"sweep {k} from the current slab: {before_cost} -> {after_cost}, winner {sw['best_variant']}")
    sa.close()


def test_the_handles_finder_is_left_alone():
    """A sweep with frontier variants on a handle that never chose a finder: its next adaptive_pass is the nearest rule's.
    (That a sweep of nearest variants makes no lists is not checked here: mgl_match_frontier reports the build time of the
    lists the handle holds whether that call made them or reused them, so the binding does not show the difference.)"""
    data = corpus.enwik_like(3000, 0x33)
    parse_in = greedy_slab(data)[0]
    fresh = _sa(data)
    want, want_obj = fresh.adaptive_pass(parse_in, 16, 1000, 64, 128)
    fresh.close()
    sa = _sa(data)
    sa.seed_sweep(MEMBERS, passes=1, chunk=1000)
    got, obj = sa.adaptive_pass(parse_in, 16, 1000, 64, 128)
    sa.close()
    assert obj == want_obj and as_list(got) == as_list(want)


def test_search_continues_from_the_sweeps_seed_like_the_oracle():
    data = corpus.enwik_like(3000, 0x33)
    n, K, seed, steps = len(data), 64, 99, 40
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=seed, iters_per_epoch=steps)
    sa.seed_sweep(binding.DEFAULT_SWEEP, passes=2)
    cur, _ = sa.current()
    o = Oracle(data, dict_limit=0x400000)
    slab = np.ascontiguousarray(cur).astype(literal_slab(1).dtype)
    best = literal_slab(n)
    ref = o.sa_batched(slab, best, 0, 0, seed, K, 0, steps, 0, steps)
    for s in range(steps):
        st = sa.run(1)
        assert st["current_cost"] == int(ref["trace"][s, 3]), s
    got, got_cost = sa.current()
    assert got_cost == ref["cur"] and as_list(got) == as_list(slab)
    bst, best_cost = sa.best()
    assert best_cost == ref["best"] and as_list(bst) == as_list(best)
    sa.close()


GRID_NAMES = [f"{'frontier' if f == F else 'nearest'} cand {c} segment {s} ahead {a}" for f, c, s, a in binding.DEFAULT_SWEEP]


def _cli_sweep(tmp_path, data, extra):
    f = tmp_path / "in.bin"
    f.write_bytes(data)
    out = tmp_path / "out.lzma"
    r = subprocess.run([build.CLI, "--adaptive-seed", "2", "--parse-sweep", "--parse-sweep-table"] + extra +
                       ["--epochs", "1", "--phases", "1", "--steps", "20", "-o", str(out), str(f)], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-400:]
    err = r.stderr.decode().splitlines()
    stream = out.read_bytes()
    assert lzma.decompress(stream, format=lzma.FORMAT_ALONE) == data
    return err, stream


def test_cli_parse_sweep(tmp_path):
    data = corpus.enwik_like(5000, 0x35)
    err, _ = _cli_sweep(tmp_path, data, [])
    table = [l for l in err if l.startswith("parse-sweep-table:")]
    assert len(table) == 16 and sum(l.endswith("*") for l in table) == 1
    for l, name in zip(table, GRID_NAMES):
        assert l.split(": ", 1)[1].startswith(name + ":"), l
        assert len(l.split(":")[2].replace("*", "").split()) == 3  # two per-pass sizes and the unit
    line = next(l for l in err if l.startswith("parse sweep:"))
    v = int(line.split("variant ")[1].split()[0])
    f, c, s, a = binding.DEFAULT_SWEEP[v]
    assert f"({'frontier' if f == F else 'nearest'}, cand {c}, segment {s}, ahead {a})" in line, line
    assert table[v].endswith("*")
    # --props auto: every round's seed is a sweep, and the stream is coded under the printed triple
    err, stream = _cli_sweep(tmp_path, data, ["--props", "auto"])
    assert any(l.startswith("parse sweep:") for l in err)
    assert len([l for l in err if l.startswith("parse-sweep-table:")]) % 16 == 0
    line = next(l for l in err if l.startswith("props: "))
    lc, lp, pb = (int(line.split(k + "=")[1].split()[0].rstrip(",")) for k in ("lc", "lp", "pb"))
    assert stream[0] == (pb * 5 + lp) * 9 + lc, line
    f = tmp_path / "in.bin"
    for bad in (["--parse-sweep"], ["--parse-sweep", "--adaptive-seed", "2", "--match-finder", "frontier"],
                ["--parse-sweep-table", "--adaptive-seed", "2"]):
        r = subprocess.run([build.CLI] + bad + [str(f)], capture_output=True, timeout=60)
        assert r.returncode != 0 and r.stdout == b"", bad


@functools.lru_cache(maxsize=None)
def _c5_64k():
    return corpus.config_input("c5", 1 << 16)[0]


DEFAULTS_INPUTS = [("c2", lambda: corpus.config_input("c2")[0]), ("c5_64k", _c5_64k)]


@pytest.mark.parametrize("name,make", DEFAULTS_INPUTS, ids=[d[0] for d in DEFAULTS_INPUTS])
def test_never_worse_than_either_default(name, make):
    data = make()
    sa = _sa(data)
    sw = sa.seed_sweep(binding.DEFAULT_SWEEP)
    _, cost = sa.current()
    sa.close()
    _, _, nearest = _alone(data, (N, 0, 0, 0))
    _, _, frontier = _alone(data, (F, 0, 0, 0))
    v = sw["best_variant"]
    print(f"{name}: sweep {18 + cost / 16384:.1f} B (variant {v}: {GRID_NAMES[v]}, pass {sw['results'][v]['best_pass']}), "
          f"nearest default {18 + nearest / 16384:.1f} B, frontier default {18 + frontier / 16384:.1f} B, sweep {sw['gpu_ms']:.1f} ms")
    assert cost <= nearest and cost <= frontier


def test_batching_does_something():
    data = corpus.lorem(4096)  # c1: one chunk at the default chunk
    sa = _sa(data)
    sa.seed_sweep(binding.DEFAULT_SWEEP)  # warm-up: the frontier's lists, the kernels' first launches
    sweep_ms = statistics.median(sa.seed_sweep(binding.DEFAULT_SWEEP)["gpu_ms"] for _ in range(3))
    sa.close()
    alone_ms = []
    for f, c, s, a in binding.DEFAULT_SWEEP:
        one = _sa(data)
        one.set_match_finder(f)
        one.seed_adaptive(cand=c, segment=s, ahead=a)  # warm-up, as above
        alone_ms.append(statistics.median(sum(one.seed_adaptive(cand=c, segment=s, ahead=a)["ms"]) for _ in range(3)))
        one.close()
    print(f"c1, 16 variants x 3 passes: sweep {sweep_ms:.2f} ms, 16 calls {sum(alone_ms):.2f} ms, ratio {sum(alone_ms) / sweep_ms:.1f}")
    assert sweep_ms < sum(alone_ms)
