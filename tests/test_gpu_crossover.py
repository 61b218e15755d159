"""Crossover of parses on the device (mgl_crossover, mgl_sa_cross_best, mgl_sa_exchange_cross, CLI --exchange cross) against
the Python restatement of the rule in test_crossover_rule_cpu.py: the child entry for entry and every figure of
mgl_cross_stats, exact integers all.  Costs are the CPU oracle's.  `-m gpu`."""
import ctypes as C
import functools
import hashlib
import lzma
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

import _random_parse as rp
from _libs import Oracle, literal_slab
from megalania_amd import binding, corpus
from test_adaptive_rule_cpu import greedy_in
from test_crossover_rule_cpu import as_slab, check_valid, crossover_rule, evolved, walk_table
from test_gpu_optimal import SMALL

pytestmark = pytest.mark.gpu

MGL_EINVAL = -1
INPUTS = SMALL + [("c2_4097", corpus.config_input("c2")[0][:4097])]  # n no multiple of 64, boundaries in the last bitmap word
IDS = [s[0] for s in INPUTS]
PROSE = SMALL[1][1]


@functools.lru_cache(maxsize=None)
def parents_of(name, kind):
    """eight parents of a named input.  random: valid parses with stale off-walk entries, few joints and long regions;
    evolved: the oracle's search run from one greedy parse under eight seeds, many joints"""
    data = dict(INPUTS)[name]
    if kind == "random":
        return [rp.random_parse(data, 100 + i, rp.TEXT, "any") for i in range(8)]
    start = greedy_in(data, 8)
    if len(data) < 1000:  # nothing to search on two bytes: the all-literal and the greedy parse take turns
        return [literal_slab(len(data)), start] * 4
    return [evolved(data, start, 21 + i, steps=12, K=32) for i in range(8)]


def check_parity(sa, data, parents, grain, props=(0, 0, 0), tabs=None):
    want = crossover_rule(data, parents, grain, *props, tabs=tabs)
    child, st = sa.crossover(parents, grain)
    P = len(parents)
    assert (child == want["child"].astype(child.dtype)).all(), (P, grain)
    assert st["parents"] == P and st["grain"] == (grain or 64) and st["adopted"] == 0
    assert st["parent_cost"] == want["parent_cost"] and st["child_cost"] == want["child_cost"], (P, grain)
    assert st["predicted"] == want["predicted"] and st["boundaries"] == want["boundaries"], (P, grain)
    assert st["regions_from"] == want["regions_from"], (P, grain)
    return want, st


@pytest.mark.parametrize("kind", ["random", "evolved"])
@pytest.mark.parametrize("name", IDS)
def test_crossover_equals_the_rule(name, kind):
    data = dict(INPUTS)[name]
    n = len(data)
    parents = parents_of(name, kind)
    tabs = [walk_table(data, p) for p in parents]
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        regions = 0
        for P in (2, 3, 8):
            for grain in (1, 0, 1000, n + 1, 37):
                want, st = check_parity(sa, data, parents[:P], grain, tabs=tabs[:P])
                regions = max(regions, want["boundaries"] - 1)
        # the same call twice on one handle: the buffers of a call are freed and made again
        first, again = (check_parity(sa, data, parents[:3], 37, tabs=tabs[:3])[1] for _ in range(2))
        assert {k: v for k, v in first.items() if k != "gpu_ms"} == {k: v for k, v in again.items() if k != "gpu_ms"}
        if n > 1000:
            assert regions >= 2  # the parents do meet somewhere inside (the random parses of `runs` at one joint only)
    finally:
        sa.close()


@pytest.mark.parametrize("props", [(3, 0, 2), (0, 2, 2)])
@pytest.mark.parametrize("kind", ["random", "evolved"])
def test_crossover_equals_the_rule_at_other_properties(kind, props):
    parents = parents_of("prose", kind)
    lc, lp, pb = props
    sa = binding.SA(PROSE, neighbours_per_step=64, lc=lc, lp=lp, pb=pb)
    try:
        tabs = [walk_table(PROSE, p, lc, lp, pb) for p in parents[:3]]
        for P, grain in ((2, 0), (3, 1), (3, 37)):
            want, _ = check_parity(sa, PROSE, parents[:P], grain, props, tabs=tabs[:P])
        check_valid(PROSE, want["child"], lc, lp, pb)
    finally:
        sa.close()


def test_crossover_leaves_the_search_untouched():
    parents = parents_of("prose", "evolved")
    one = binding.SA(PROSE, neighbours_per_step=64, seed=5)
    two = binding.SA(PROSE, neighbours_per_step=64, seed=5)
    try:
        for sa in (one, two):
            sa.run(3)
        before = two.neighbours(3)
        cur0, best0 = two.current(), two.best()
        two.crossover(parents[:2], 0)
        two.crossover(parents[:8], 1)
        after = two.neighbours(3)
        assert (before[0] == after[0]).all() and (before[1] == after[1]).all() and (before[2] == after[2]).all()
        cur1, best1 = two.current(), two.best()
        assert (cur0[0] == cur1[0]).all() and cur0[1] == cur1[1] and (best0[0] == best1[0]).all() and best0[1] == best1[1]
        s1, s2 = one.run(4), two.run(4)
        assert s1["current_cost"] == s2["current_cost"] and s1["best_cost"] == s2["best_cost"]
        assert (one.current()[0] == two.current()[0]).all()
    finally:
        one.close()
        two.close()


def _raw(sa, handle, parents, count, grain=0):
    keep = [np.ascontiguousarray(p, dtype=binding.PACKET) for p in parents if p is not None]
    it = iter(keep)
    arr = (C.c_void_p * max(1, len(parents)))(*[None if p is None else next(it).ctypes.data for p in parents])
    st = binding.CrossStats()
    return sa.L.mgl_crossover(handle, arr if parents else None, count, grain, None, C.byref(st))


def test_refusals():
    data = PROSE
    n = len(data)
    g = greedy_in(data, 8)
    lit = literal_slab(n)
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        assert _raw(sa, None, [g, lit], 2) == MGL_EINVAL
        assert sa.L.mgl_crossover(sa.h, None, 2, 0, None, None) == MGL_EINVAL
        assert _raw(sa, sa.h, [g], 1) == MGL_EINVAL
        assert _raw(sa, sa.h, [g] * 9, 9) == MGL_EINVAL
        assert _raw(sa, sa.h, [g, None, lit], 3) == MGL_EINVAL
        assert sa.L.mgl_sa_cross_best(sa.h, None, 0, None) == MGL_EINVAL and sa.L.mgl_sa_cross_best(None, None, 0, None) == MGL_EINVAL
        assert sa.L.mgl_sa_exchange_cross(sa.h, None, 0, None, None, None) == MGL_EINVAL
        # an invalid parse: the code mgl_cost_slab returns for it
        overrun = lit.copy()
        overrun[n - 1] = (binding.MATCH, 0, 5)
        wrong = as_slab(g).copy()
        on = rp.on_walk(wrong)
        at = next(p for p in range(n - 1, 0, -1) if on[p] and wrong[p]["type"] == binding.MATCH)
        d = int(wrong[at]["dist"])
        wrong[at]["dist"] = next(x for x in range(at) if data[at - x - 1] != data[at] and x != d)  # a source that differs from the input
        for bad in (overrun, wrong):
            try:
                sa.cost_slab(bad, want_cum=False)
                rc = 0
            except binding.MglError as e:
                rc = e.rc
            for parents in ([g, bad], [bad, g], [lit, g, bad]):
                assert _raw(sa, sa.h, parents, len(parents)) == rc, (rc, len(parents))
        assert _raw(sa, sa.h, [g, overrun], 2) == MGL_EINVAL
        check_parity(sa, data, [g, lit], 0)  # the handle is as usable as before
    finally:
        sa.close()


def test_cross_best_takes_the_child_the_other_slab_or_nothing():
    data = PROSE
    n = len(data)
    o = Oracle(data, dict_limit=0x400000)
    g = as_slab(greedy_in(data, 8))
    lit = literal_slab(n)
    a, b = (evolved(data, g, 21 + i, steps=40, K=32) for i in range(2))
    cost = lambda s: o.cost_slab(as_slab(s))["total"]
    sa = binding.SA(data, neighbours_per_step=64, accept="single")
    try:
        assert sa.best()[1] == 0
        st = sa.cross_best(lit)  # no best slab yet: the other one is adopted
        assert st["adopted"] == 1 and st["parents"] == 0 and st["parent_cost"][1] == cost(lit)
        best, c = sa.best()
        assert c == cost(lit) and (best == lit.astype(best.dtype)).all()
        st = sa.cross_best(g, n + 1)  # one region: the child is the greedy parse, no cheaper than it: the other slab
        assert st["adopted"] == 1 and st["parent_cost"] == [cost(lit), cost(g)] and st["child_cost"] == cost(g)
        best, c = sa.best()
        assert c == cost(g) and (best == g.astype(best.dtype)).all()
        st = sa.cross_best(lit)  # nothing beats the own best
        assert st["adopted"] == 0 and st["boundaries"] >= 2
        best, c = sa.best()
        assert c == cost(g) and (best == g.astype(best.dtype)).all()
        sa.set_best(a, cost(a))
        want = crossover_rule(data, [a, b], 0)
        assert want["child_cost"] < min(want["parent_cost"])  # what the restatement says of these two
        cur0 = sa.current()
        st = sa.cross_best(b)
        assert st["adopted"] == 2 and st["child_cost"] == want["child_cost"] and st["parent_cost"] == want["parent_cost"]
        assert st["predicted"] == want["predicted"] and st["regions_from"] == want["regions_from"]
        best, c = sa.best()
        assert c == want["child_cost"] == cost(best) and (best == want["child"].astype(best.dtype)).all()
        cur1 = sa.current()
        assert (cur0[0] == cur1[0]).all() and cur0[1] == cur1[1]  # the current slab stays
        sa.begin_epoch(1, from_best=True)
        stats = sa.run(4)
        cur, c = sa.current()
        assert c == stats["current_cost"] == cost(cur) and 0 < stats["best_cost"] <= want["child_cost"]
        best, c = sa.best()
        assert c == stats["best_cost"] == cost(best)
    finally:
        sa.close()


def _sha(slab):
    return hashlib.sha256(np.ascontiguousarray(slab).tobytes()).hexdigest()


def _chain_worker(rank, world, path, nonce, out):
    os.environ["MGL_NO_AUTOBUILD"] = "1"
    os.environ["MGL_COMM_TIMEOUT_S"] = "120"
    from megalania_amd import binding, corpus, multi_gpu

    data = corpus.enwik_like(4000, 0x52)
    comm = binding.Comm.shm(path, nonce, rank, world, 0)
    sa = binding.SA(data, accept="single", neighbours_per_step=256, seed=multi_gpu.chain_seed(1673551, rank), iters_per_epoch=len(data))
    sa.run(10 + 30 * (1 - rank))  # rank 0 searches longer: it should win
    before, before_cost = sa.best()
    winner, wcost, st = multi_gpu.exchange_cross_native(sa, comm, 64)
    after, after_cost = sa.best()
    sa.begin_epoch(1, from_best=True)  # what was adopted is checked against the input here
    final = sa.exchange_best(comm)
    words, fcost = sa.best_packed()
    slab, _ = sa.best()
    ok = lzma.decompress(binding.emit_stream(data, slab), format=lzma.FORMAT_ALONE) == data
    out.put((rank, winner, wcost, st, before.tobytes(), before_cost, after.tobytes(), after_cost, final, fcost,
             hashlib.sha256(np.ascontiguousarray(words).tobytes()).hexdigest(), ok))
    sa.close()
    comm.close()


def test_two_chains_cross_at_the_exchange(tmp_path):
    path = "/dev/shm/mgl_test_cross_%d" % os.getpid() if os.path.isdir("/dev/shm") else str(tmp_path / "comm.shm")
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_chain_worker, args=(r, 2, path, 0xC0DE, out)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(out.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    r0, r1 = res
    assert r0[1] == r1[1] and r0[2] == r1[2] == min(r0[5], r1[5])  # same winner, the cheaper best slab's cost
    win, lose = (r0, r1) if r0[1] == 0 else (r1, r0)
    assert (np.frombuffer(win[6], dtype=binding.PACKET) == np.frombuffer(win[4], dtype=binding.PACKET)).all()
    assert win[7] == win[5] and win[3]["parents"] == 0  # the winner's best is unchanged
    # the loser holds what the restatement makes of its own best slab and the winner's
    data = corpus.enwik_like(4000, 0x52)
    own = np.frombuffer(lose[4], dtype=binding.PACKET)
    other = np.frombuffer(win[4], dtype=binding.PACKET)
    want = crossover_rule(data, [own, other], 64)
    assert want["parent_cost"] == [lose[5], win[5]]
    st = lose[3]
    assert st["child_cost"] == want["child_cost"] and st["predicted"] == want["predicted"] and st["regions_from"] == want["regions_from"]
    if want["child_cost"] < min(want["parent_cost"]):
        kind, slab, cost = 2, want["child"], want["child_cost"]
    elif win[5] < lose[5]:
        kind, slab, cost = 1, other, win[5]
    else:
        kind, slab, cost = 0, own, lose[5]
    print(f"own {lose[5]}, winner's {win[5]}, child {want['child_cost']}: adopted {kind}")
    assert st["adopted"] == kind and lose[7] == cost
    got = np.frombuffer(lose[6], dtype=binding.PACKET)
    assert (got == np.ascontiguousarray(slab).astype(binding.PACKET)).all()  # field by field: the records have padding
    # one plain exchange: both hold the same slab, bit for bit, and it decodes
    assert r0[8] == r1[8] and r0[8][1] == min(win[7], lose[7]) == r0[9] == r1[9]
    assert r0[10] == r1[10] and r0[11] and r1[11]
    assert not os.path.exists(path)


def test_cli_two_chains_cross(tmp_path):
    import subprocess
    from megalania_amd import build

    data = corpus.enwik_like(3000, 0x64)
    f = tmp_path / "in.bin"
    f.write_bytes(data)
    comm = "/dev/shm/mgl_test_cli_cross_%d" % os.getpid() if os.path.isdir("/dev/shm") else str(tmp_path / "comm.shm")
    env = dict(os.environ, MGL_COMM_TIMEOUT_S="120")
    cmd = [build.CLI, "--epochs", "2", "--phases", "2", "--neighbours", "128", "--chains", "2", "--device", "0", "--transport", "shm",
           "--comm-file", comm, "--comm-nonce", "515151", "--exchange", "cross", "--cross-grain", "64"]
    ps = [subprocess.Popen(cmd + ["--rank", str(r), str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env) for r in (1, 0)]
    outs = [p.communicate(timeout=600) for p in ps]
    assert all(p.returncode == 0 for p in ps), [o[1].decode()[-400:] for o in outs]
    lines = [o[1].decode().splitlines() for o in outs]
    ex = [[ln for ln in ls if ln.startswith("exchange:")] for ls in lines]
    assert len(ex[0]) == 5 and ex[0] == ex[1]  # one crossing exchange per epoch and the plain one at the end
    cross = [[ln for ln in ls if ln.startswith("cross:")] for ls in lines]
    assert len(cross[0]) == len(cross[1]) == 4 and all("adopted" in ln for ln in cross[0] + cross[1])
    assert outs[0][0] == b""  # rank 1 writes no stream
    assert lzma.decompress(outs[1][0], format=lzma.FORMAT_ALONE) == data
    assert not os.path.exists(comm)
