"""Adaptive-price optimal parse (`mgl_sa_seed_adaptive`, `mgl_adaptive_pass`, mgl_adaptive.hip): an opt-in seed and
re-parse that is not in the reference.  Pinned by the plain-Python restatement of the rule in
tests/test_adaptive_rule_cpu.py, by the oracle's costing of what it leaves in the handle, by the oracle's batched SA
continuing from it, and by liblzma decoding the stream.  `-m gpu`."""
import itertools
import lzma
import subprocess

import numpy as np
import pytest

from _libs import Oracle, literal_slab
from megalania_amd import binding, build, corpus
from test_adaptive_rule_cpu import adaptive_rule
from test_gpu_optimal import MATCH, SMALL, as_list, greedy_slab

pytestmark = pytest.mark.gpu


def _check_pass(sa, data, parse_in, cand, chunk, segment, ahead, **kw):
    before = sa.current()
    got, obj = sa.adaptive_pass(parse_in, cand, chunk, segment, ahead)
    want, want_obj, _ = adaptive_rule(data, parse_in, cand, chunk, segment, ahead, **kw)
    what = (cand, chunk, segment, ahead)
    assert as_list(got) == want, (what, next(i for i, (g, w) in enumerate(zip(as_list(got), want)) if g != w))
    assert obj == want_obj, what
    after = sa.current()
    assert after[1] == before[1] and as_list(after[0]) == as_list(before[0]), what  # SA state untouched
    return want


GRID = list(itertools.product((1, 16), (1000, 1 << 16), (64, 300), (0, 128)))  # cand, chunk, segment, ahead


@pytest.mark.parametrize("start", ["greedy", "literal"])
@pytest.mark.parametrize("name,data", SMALL, ids=[s[0] for s in SMALL])
def test_pass_matches_the_rule(name, data, start):
    parse_in = greedy_slab(data)[0] if start == "greedy" else literal_slab(len(data))
    sa = binding.SA(data, accept="single", neighbours_per_step=16)
    for cand, chunk, segment, ahead in GRID:
        _check_pass(sa, data, parse_in, cand, chunk, segment, ahead)
    sa.close()


@pytest.mark.parametrize("name,data", SMALL[:4], ids=[s[0] for s in SMALL[:4]])
def test_pass_matches_the_rule_under_a_window(name, data):
    g, _ = greedy_slab(data, dict_limit=300)
    sa = binding.SA(data, accept="single", neighbours_per_step=16, dict_limit=300)
    got = _check_pass(sa, data, g, 16, 1000, 64, 128, dict_limit=300)
    assert all(t != MATCH or d - 1 < 300 for t, d, _ in got)
    sa.close()


@pytest.mark.parametrize("name,data", SMALL[:4], ids=[s[0] for s in SMALL[:4]])
def test_pass_matches_the_rule_at_other_properties(name, data):
    g, _ = greedy_slab(data, lc=3, lp=0, pb=2)
    sa = binding.SA(data, accept="single", neighbours_per_step=16, lc=3, lp=0, pb=2)
    _check_pass(sa, data, g, 16, 1000, 64, 128, lc=3, lp=0, pb=2)
    _check_pass(sa, data, g, 16, 1 << 16, 300, 0, lc=3, lp=0, pb=2)
    sa.close()


def test_pass_rejects_bad_arguments():
    data = corpus.lorem(2048)
    sa = binding.SA(data, accept="single", neighbours_per_step=16)
    ok = literal_slab(len(data))
    not_a_parse = ok.copy()
    not_a_parse[0]["type"] = 0
    overrun = ok.copy()
    overrun[len(data) - 1] = (MATCH, 0, 3)
    for parse_in, cand, chunk, segment, ahead in ((ok, 0, 4096, 64, 128), (ok, 31, 4096, 64, 128), (ok, 8, 511, 64, 128),
                                                  (ok, 8, 4096, 64, 274), (not_a_parse, 8, 4096, 64, 128),
                                                  (overrun, 8, 4096, 64, 128)):
        with pytest.raises(binding.MglError):
            sa.adaptive_pass(parse_in, cand, chunk, segment, ahead)
    for kw in (dict(cand=31), dict(chunk=511), dict(ahead=274, segment=64), dict(passes=17)):
        with pytest.raises(binding.MglError):
            sa.seed_adaptive(**kw)
    sa.adaptive_pass(ok, 8, 4096, 64, 128)  # and the handle still works
    sa.close()


def _oracle_cost(data, slab, lc=0, lp=0, pb=0, dict_limit=0x400000):
    o = Oracle(data, lc=lc, lp=lp, pb=pb, dict_limit=dict_limit)
    return o.cost_slab(np.ascontiguousarray(slab).astype(literal_slab(1).dtype))["total"]


def _check_seed(data, lc, lp, pb, dict_limit, **kw):
    sa = binding.SA(data, accept="single", neighbours_per_step=16, lc=lc, lp=lp, pb=pb, dict_limit=dict_limit)
    st = sa.seed_adaptive(**kw)
    cur, cost = sa.current()
    assert cost == min(st["cost"]) == st["cost"][st["best_pass"]]
    assert cost == _oracle_cost(data, cur, lc, lp, pb, dict_limit)
    assert lzma.decompress(binding.emit_stream(data, cur, lc=lc, lp=lp, pb=pb), format=lzma.FORMAT_ALONE) == data
    assert all(t != MATCH or d < dict_limit for t, d, _ in as_list(cur))
    sa.close()
    return cur, cost, st


@pytest.mark.parametrize("dict_limit", [1000, 0x400000])
@pytest.mark.parametrize("lc,lp,pb", [(0, 0, 0), (3, 0, 2), (0, 2, 2)])
def test_seed_is_a_valid_exactly_costed_parse(lc, lp, pb, dict_limit):
    data = corpus.enwik_like(20000, 0x52)
    a, ca, st = _check_seed(data, lc, lp, pb, dict_limit, passes=3, chunk=4096)
    assert st["passes"] == 3 and len(st["ms"]) == 3
    b, cb, _ = _check_seed(data, lc, lp, pb, dict_limit, passes=3, chunk=4096)
    assert ca == cb and as_list(a) == as_list(b)


@pytest.mark.parametrize("data", [b"x", b"ab", b"a" * 3000], ids=["n1", "n2", "run"])
def test_seed_on_edge_inputs(data):
    _check_seed(data, 0, 0, 0, 0x400000)


def test_search_continues_from_the_adaptive_seed_like_the_oracle():
    data = corpus.enwik_like(3000, 0x33)
    n, K, seed, steps = len(data), 64, 99, 40
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=seed, iters_per_epoch=steps)
    sa.seed_adaptive(passes=2)
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


def test_reparse_from_the_current_slab_never_costs_more():
    data = corpus.enwik_like(3000, 0x33)
    sa = binding.SA(data, accept="single", neighbours_per_step=64, seed=7, iters_per_epoch=200)
    sa.seed_greedy(8)
    sa.run(40)
    for k in range(3):
        before, before_cost = sa.current()
        st = sa.seed_adaptive(passes=2, from_current=True)
        after, after_cost = sa.current()
        assert st["greedy_cost"] == before_cost
        assert after_cost <= before_cost
        if st["best_pass"] is None:
            assert after_cost == before_cost and as_list(after) == as_list(before)
            assert min(st["cost"]) >= before_cost
        else:
            assert after_cost == st["cost"][st["best_pass"]] == min(st["cost"]) < before_cost
        assert after_cost == _oracle_cost(data, after)
        print(f"re-parse {k}: {before_cost} -> {after_cost} (passes {st['cost']}, best {st['best_pass']})")
        if k < 2:
            sa.run(40)
            assert sa.current()[1] == _oracle_cost(data, sa.current()[0])
    # a parse that the re-parse cannot improve stays: its own output, handed back at once
    before, before_cost = sa.current()
    st = sa.seed_adaptive(passes=1, from_current=True)
    after, after_cost = sa.current()
    assert after_cost <= before_cost and (st["best_pass"] is not None or as_list(after) == as_list(before))
    sa.close()


def _lzma_9e(data, lc=0, lp=0, pb=0):
    return len(lzma.compress(data, format=lzma.FORMAT_ALONE,
                             filters=[dict(id=lzma.FILTER_LZMA1, preset=9 | lzma.PRESET_EXTREME, lc=lc, lp=lp, pb=pb,
                                           dict_size=1 << 22)]))


# The adaptive seed's estimate over stdlib lzma -9e at the library's defaults; each gate is the ratio rounded up to the next
# 0.5 %, and has to be below the static seed's 1.02.  c2: 38 371.8 B over 37 808 B = 1.0149, from the restatement in
# tests/test_adaptive_rule_cpu.py run on the CPU (greedy parse of 16 candidates, 3 passes, chunk 4 096, segment 64, ahead
# 128), which the device has to match integer for integer (test_pass_matches_the_rule); not yet measured on an MI355X.
# c5 at 256 KiB: not measured either way; 1.015 is the largest gate below 1.02 on that grid.
QUALITY = [
    ("c2", lambda: corpus.config_input("c2")[0], 1.015),
    ("c5_256k", lambda: corpus.config_input("c5", 1 << 18)[0], 1.015),
]


@pytest.mark.parametrize("name,make,gate", QUALITY, ids=[q[0] for q in QUALITY])
def test_seed_quality(name, make, gate):
    data = make()
    sa = binding.SA(data, accept="single", neighbours_per_step=16)
    so = sa.seed_optimal()
    _, static_cost = sa.current()
    sa.close()
    sa = binding.SA(data, accept="single", neighbours_per_step=16)
    st = sa.seed_adaptive()
    _, cost = sa.current()
    sa.close()
    xz = _lzma_9e(data)
    est = 18 + cost / 16384
    print(f"{name}: adaptive {est:.0f} B, static {18 + static_cost / 16384:.0f} B, lzma -9e {xz} B, ratio {est / xz:.4f} "
          f"(static {(18 + static_cost / 16384) / xz:.4f}), passes {st['cost']} ms {[round(m, 1) for m in st['ms']]} "
          f"(static ms {[round(m, 1) for m in so['ms']]})")
    assert gate < 1.02
    assert cost < static_cost
    assert est <= gate * xz


def test_seed_quality_c1_is_printed():
    data = corpus.lorem(4096)  # one repetitive 4 KiB chunk can go either way: no gate
    sa = binding.SA(data, accept="single", neighbours_per_step=16)
    sa.seed_optimal()
    _, static_cost = sa.current()
    st = sa.seed_adaptive()
    _, cost = sa.current()
    sa.close()
    assert cost == min(st["cost"])
    print(f"c1: adaptive {18 + cost / 16384:.0f} B, static {18 + static_cost / 16384:.0f} B, lzma -9e {_lzma_9e(data)} B")


def test_cli_adaptive_seed(tmp_path):
    data = corpus.enwik_like(5000, 0x35)
    f = tmp_path / "in.bin"
    f.write_bytes(data)
    out = tmp_path / "out.lzma"
    r = subprocess.run([build.CLI, "--adaptive-seed", "3", "--epochs", "1", "--phases", "1", "--steps", "50", "-o", str(out), str(f)],
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-400:]
    assert b"adaptive seed" in r.stderr
    assert lzma.decompress(out.read_bytes(), format=lzma.FORMAT_ALONE) == data
    r = subprocess.run([build.CLI, "--adaptive-seed", "3", "--props", "auto", "--epochs", "1", "--phases", "1", "--steps", "20",
                        "-o", str(out), str(f)], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-400:]
    stream = out.read_bytes()
    assert lzma.decompress(stream, format=lzma.FORMAT_ALONE) == data
    line = next(l for l in r.stderr.decode().splitlines() if l.startswith("props: "))
    lc, lp, pb = (int(line.split(k + "=")[1].split()[0].rstrip(",")) for k in ("lc", "lp", "pb"))
    assert stream[0] == (pb * 5 + lp) * 9 + lc, line
    r = subprocess.run([build.CLI, "--adaptive-seed", "3", "--optimal-seed", "3", str(f)], capture_output=True, timeout=600)
    assert r.returncode != 0
