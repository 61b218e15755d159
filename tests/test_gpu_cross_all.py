"""The exchange that crosses every chain's best slab on the device (mgl_slab_hash, mgl_sa_exchange_cross_all, CLI --exchange
cross-all) against the Python restatements: the selection and the hash of test_cross_all_cpu.py and the crossover rule of
test_crossover_rule_cpu.py, exact integers all.  Chains are processes that share GPU 0 over the host shared-memory transport,
nine at the most.  `-m gpu`."""
import functools
import lzma
import multiprocessing as mp
import os
import queue
import subprocess
import time

import numpy as np
import pytest

import _random_parse as rp
from _cross_all_chain import K, SEED, STEPS, chain
from _libs import Oracle, literal_slab
from megalania_amd import binding, build, corpus, multi_gpu
from test_adaptive_rule_cpu import greedy_in
from test_cross_all_cpu import select_parents, slab_hash_rule
from test_crossover_rule_cpu import as_slab, crossover_rule, evolved_parents

pytestmark = pytest.mark.gpu

MGL_EINVAL = -1
C2 = corpus.config_input("c2")[0][:4097]


def packed(slab):
    return np.ascontiguousarray(slab).astype(binding.PACKET)


def same(a, b):
    return bool((packed(a) == packed(b)).all())  # field by field: the records have padding


def oracle_cost(data, slab):
    return Oracle(data, dict_limit=0x400000).cost_slab(as_slab(slab))["total"]


# ---- the slab hash
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_slab_hash_equals_the_formula(n):
    data = C2[:n]
    sa = binding.SA(data, neighbours_per_step=K, accept="single", seed=5)
    try:
        with pytest.raises(binding.MglError) as e:
            sa.slab_hash()  # no best slab yet
        assert e.value.rc == MGL_EINVAL
        lit, greedy = literal_slab(n), greedy_in(data, 8)
        stale = rp.random_parse(data, 41, rp.TEXT, "any")
        for slab in (lit, greedy, stale):
            assert sa.slab_hash(slab) == slab_hash_rule(packed(slab)), n
        off = np.nonzero(~rp.on_walk(stale))[0]
        assert (len(off) > 0) == (n >= 63)  # n = 1: one literal, nothing lies under it
        if len(off):
            # one stale entry changed: the same walk, the same cost, another slab
            other = stale.copy()
            at = int(off[len(off) // 2])
            other[at] = (binding.LITERAL, 0, 1) if int(other[at]["type"]) != binding.LITERAL else (binding.SHORT_REP, 0, 1)
            assert sa.cost_slab(other, want_cum=False)["total"] == sa.cost_slab(stale, want_cum=False)["total"]
            assert sa.slab_hash(other) == slab_hash_rule(packed(other)) != sa.slab_hash(stale)
        # packets = NULL: the best slab, where set_best put it ...
        sa.set_best(stale, sa.cost_slab(stale, want_cum=False)["total"])
        assert sa.slab_hash() == slab_hash_rule(packed(stale))
        assert sa.L.mgl_slab_hash(sa.h, None, None) == MGL_EINVAL
        if n == 4097:
            # ... and where a search left it; a parity hook: the search goes on as if nothing had been asked
            one = binding.SA(data, neighbours_per_step=K, accept="single", seed=5)
            try:
                for s in (sa, one):
                    s.begin_epoch(0)
                    s.run(3)
                assert sa.slab_hash(greedy) == slab_hash_rule(packed(greedy))
                assert one.slab_hash() == slab_hash_rule(packed(one.best()[0]))
                assert sa.slab_hash() == slab_hash_rule(packed(sa.best()[0]))
            finally:
                one.close()
    finally:
        sa.close()


# ---- chains as processes (tests/_cross_all_chain.py: what a chain does)
def run_chains(world, jobs, tag):
    """jobs: dicts of data, slabs (per rank None or (slab, cost)), grains (one exchange each, the best slab set anew before each),
    nomem_rank, search.  Returns per rank, per job, the rows of _cross_all_chain.chain."""
    path = ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp") + "/mgl_test_cross_all_%d_%s" % (os.getpid(), tag)
    wire = [dict(j, slabs=[None if s is None else (packed(s[0]).tobytes(), int(s[1])) for s in j["slabs"]]) for j in jobs]
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=chain, args=(r, world, path, 0xA110 + world, wire, out)) for r in range(world)]
    for p in procs:
        p.start()
    res, deadline = {}, time.monotonic() + 300
    try:
        while len(res) < world:
            try:
                r, rows = out.get(timeout=0.5)
                res[r] = rows
            except queue.Empty:
                assert all(p.exitcode in (None, 0) for p in procs), [p.exitcode for p in procs]
                assert time.monotonic() < deadline
    finally:
        for p in procs:
            p.join(timeout=90)
        for p in procs:
            if p.is_alive():
                p.kill()
    assert [p.exitcode for p in procs] == [0] * world
    assert not os.path.exists(path)
    return [res[r] for r in range(world)]


def expected(data, slabs, grain, crossed=True):
    """What the restatements make of one exchange: the parents' ranks, the rule's result (None if nothing is crossed) and per
    rank (adopted, best slab, best cost)."""
    world = len(slabs)
    keys = [multi_gpu.pack_key(0 if s is None else s[1], r) for r, s in enumerate(slabs)]
    hashes = [0 if s is None else slab_hash_rule(packed(s[0])) for s in slabs]
    order = select_parents(keys, hashes)
    want = crossover_rule(data, [as_slab(slabs[r][0]) for r in order], grain) if len(order) >= 2 and crossed else None
    ends = []
    for r in range(world):
        own = slabs[r]
        if want is not None and want["child_cost"] < want["parent_cost"][0]:
            ends.append((2, want["child"], want["child_cost"]))
        elif order and (own is None or own[1] > slabs[order[0]][1]):
            ends.append((1,) + tuple(slabs[order[0]]))
        else:
            ends.append((0,) + (tuple(own) if own is not None else (None, 0)))
    return order, want, ends


def check_exchange(rows, data, slabs, grain, crossed=True):
    """rows: per rank the row of one exchange"""
    order, want, ends = expected(data, slabs, grain, crossed)
    for r, row in enumerate(rows):
        st, x = row["st"], row["st"]["cross"]
        assert st["chains_with_best"] == sum(s is not None for s in slabs) and st["distinct"] == len(order), (r, st)
        assert st["parent_rank"] == order and st["own_parent"] == (order.index(r) if r in order else None), (r, st)
        assert st["fell_back"] == (0 if crossed else 1)
        kind, slab, cost = ends[r]
        assert x["adopted"] == kind and row["cost"] == cost and row["cur_same"], (r, x, row["cost"], cost)
        if want is None:
            assert x["parents"] == 0 and x["child_cost"] == 0
        else:
            assert x["parents"] == len(order) and x["grain"] == (grain or 64)
            for k in ("parent_cost", "child_cost", "predicted", "boundaries", "regions_from"):
                assert x[k] == want[k], (r, k, x[k], want[k])
        if slab is None:
            assert row["cost"] == 0
        else:
            assert same(np.frombuffer(row["best"], dtype=binding.PACKET), slab), r  # entry for entry
            assert row["hash"] == slab_hash_rule(packed(slab))
    return order, want, ends


def with_costs(data, slabs):
    return [None if s is None else (as_slab(s), oracle_cost(data, s)) for s in slabs]


@functools.lru_cache(maxsize=None)
def world4():
    data, _, parents = evolved_parents("prose")
    slabs = with_costs(data, parents)
    return data, slabs, run_chains(4, [dict(data=data, slabs=slabs, grains=[64, 1], search=True)], "w4")


@pytest.mark.parametrize("grain", [64, 1])
def test_four_chains_take_the_child_of_all_four(grain):
    data, slabs, res = world4()
    rows = [res[r][0][[64, 1].index(grain)] for r in range(4)]
    # the CPU rule first: the child of all four is cheaper than the best parent (2 997.4 B against 3 011.2 B at grain 64)
    order, want, ends = expected(data, slabs, grain)
    assert len(order) == 4 and want["child_cost"] < min(want["parent_cost"]) == want["parent_cost"][0]
    if grain == 64:
        assert round(want["child_cost"] / 16384, 1) == 2997.4 and round(want["parent_cost"][0] / 16384, 1) == 3011.2
    assert sum(n > 0 for n in want["regions_from"]) >= 3  # regions of several parents: a crossing of more than two
    check_exchange(rows, data, slabs, grain)
    assert all(row["st"]["cross"]["adopted"] == 2 for row in rows)
    assert all(same(np.frombuffer(row["best"], dtype=binding.PACKET), want["child"]) for row in rows)


def test_the_search_goes_on_from_the_adopted_child():
    """mgl_sa_begin_epoch(.., from_best) verifies the child that came out of the last exchange (grain 1); twenty steps from it
    are the oracle's from the same slab."""
    data, slabs, res = world4()
    _, want, _ = expected(data, slabs, 1)
    o = Oracle(data, dict_limit=0x400000)
    for r in range(4):
        got = res[r][0][2]
        slab, best = as_slab(want["child"]).copy(), as_slab(want["child"]).copy()
        ref = o.sa_batched(slab, best, 0, want["child_cost"], multi_gpu.chain_seed(SEED, r), K, 1, STEPS, 0, STEPS)
        assert got["trace"] == [int(c) for c in ref["trace"][:, 3]], r
        assert got["cur_cost"] == ref["cur"] and got["best_cost"] == ref["best"] <= want["child_cost"]
        assert same(np.frombuffer(got["cur"], dtype=binding.PACKET), slab) and same(np.frombuffer(got["best"], dtype=binding.PACKET), best)


SMALL_PROSE = corpus.prose_like(1500, 0x52)


@functools.lru_cache(maxsize=None)
def world3():
    n = len(SMALL_PROSE)
    lit, greedy = literal_slab(n), greedy_in(SMALL_PROSE, 8)
    data, _, parents = evolved_parents("prose")
    jobs = dict(
        no_winner=dict(data=SMALL_PROSE, slabs=with_costs(SMALL_PROSE, [lit, greedy, greedy.copy()]), grains=[64]),
        none_child=dict(data=data, slabs=with_costs(data, [None, parents[1], parents[0]]), grains=[64]),
        none_parent=dict(data=SMALL_PROSE, slabs=with_costs(SMALL_PROSE, [greedy, None, lit]), grains=[1]),
        same=dict(data=SMALL_PROSE, slabs=with_costs(SMALL_PROSE, [greedy, greedy.copy(), greedy.copy()]), grains=[64]),
        nobody=dict(data=SMALL_PROSE, slabs=[None, None, None], grains=[64]),
        no_room=dict(data=SMALL_PROSE, slabs=with_costs(SMALL_PROSE, [lit, greedy, greedy.copy()]), grains=[64, 64], nomem_rank=1),
    )
    res = run_chains(3, list(jobs.values()), "w3")
    return {name: (job, [res[r][i][:] for r in range(3)]) for i, (name, job) in enumerate(jobs.items())}


def test_three_chains_the_child_does_not_win():
    job, rows = world3()["no_winner"]
    data, slabs = job["data"], job["slabs"]
    # the CPU rule first: the duplicate is dropped, and the child of (greedy, literal) is not cheaper than the greedy parse
    order, want, ends = expected(data, slabs, 64)
    assert order == [1, 0] and want["child_cost"] >= want["parent_cost"][0] == slabs[1][1]
    check_exchange([r[0] for r in rows], data, slabs, 64)
    assert [r[0]["st"]["cross"]["adopted"] for r in rows] == [1, 0, 0]  # the literal chain takes the greedy parse, the others stay


def test_three_chains_one_without_a_best_slab():
    job, rows = world3()["none_child"]
    order, want, ends = check_exchange([r[0] for r in rows], job["data"], job["slabs"], 64)
    assert order == [2, 1] and [e[0] for e in ends] == [2, 2, 2]  # left out of the parents, it takes the child like the others
    job, rows = world3()["none_parent"]
    order, want, ends = check_exchange([r[0] for r in rows], job["data"], job["slabs"], 1)
    assert order == [0, 2] and [e[0] for e in ends] == [0, 1, 1]  # no child worth taking: it adopts the cheapest parent


def test_three_chains_with_the_same_slab_cross_nothing():
    job, rows = world3()["same"]
    order, want, ends = check_exchange([r[0] for r in rows], job["data"], job["slabs"], 64)
    assert order == [0] and want is None and [e[0] for e in ends] == [0, 0, 0]
    job, rows = world3()["nobody"]
    order, want, ends = check_exchange([r[0] for r in rows], job["data"], job["slabs"], 64)
    assert order == [] and all(r[0]["cost"] == 0 for r in rows)


def test_a_chain_without_room_sends_everybody_to_the_plain_exchange():
    job, rows = world3()["no_room"]
    data, slabs = job["data"], job["slabs"]
    order, want, ends = check_exchange([r[0] for r in rows], data, slabs, 64, crossed=False)
    assert order == [1, 0] and [e[0] for e in ends] == [1, 0, 0]
    # the switch counted down to zero on chain 1, chains 0 and 2 never had one: the next exchange crosses
    check_exchange([r[1] for r in rows], data, slabs, 64)


def test_nine_chains_cross_the_eight_cheapest():
    data = rp.doubled_letters(1, 1500)
    parses = [rp.random_parse(data, 300 + i, rp.REPS, "any") for i in range(9)]
    slabs = with_costs(data, parses)
    order, want, ends = expected(data, slabs, 1)
    dearest = max(range(9), key=lambda r: slabs[r][1])
    assert len(order) == 8 and dearest not in order and dearest != 8
    assert sum(n > 0 for n in want["regions_from"]) >= 3  # what the CPU rule says of these parses: three parents give regions
    res = run_chains(9, [dict(data=data, slabs=slabs, grains=[1])], "w9")
    check_exchange([res[r][0][0] for r in range(9)], data, slabs, 1)
    assert res[dearest][0][0]["st"]["own_parent"] is None and res[dearest][0][0]["st"]["cross"]["adopted"] in (1, 2)


@pytest.mark.parametrize("transport", ["shm", "rccl"])
def test_a_world_of_one_changes_nothing(transport, tmp_path):
    """the RCCL form's only reachable case on one GPU (RCCL refuses two ranks per device): library, communicator, ncclAllGather"""
    data = SMALL_PROSE
    if transport == "shm":
        comm = binding.Comm.shm(("/dev/shm" if os.path.isdir("/dev/shm") else str(tmp_path)) + "/mgl_test_cross_all_one_%d" % os.getpid(), 0x111, 0, 1, 0)
    else:
        comm = binding.Comm(binding.Comm.unique_id(), 0, 1, 0)
    sa = binding.SA(data, neighbours_per_step=K, seed=3)
    try:
        st = sa.exchange_cross_all(comm, 64)
        assert (st["chains_with_best"], st["distinct"], st["parent_rank"], st["own_parent"], st["fell_back"]) == (0, 0, [], None, 0)
        run = sa.run(5)
        best0, cost0 = sa.best()
        cur0, cur_cost0 = sa.current()
        st = multi_gpu.exchange_cross_all_native(sa, comm)
        assert (st["chains_with_best"], st["distinct"], st["parent_rank"], st["own_parent"], st["fell_back"]) == (1, 1, [0], 0, 0)
        assert st["cross"]["parents"] == 0 and st["cross"]["adopted"] == 0 and st["cross"]["parent_cost"][0] == cost0 == run["best_cost"]
        best1, cost1 = sa.best()
        cur1, cur_cost1 = sa.current()
        assert same(best0, best1) and cost0 == cost1 and same(cur0, cur1) and cur_cost0 == cur_cost1
        assert sa.run(2)["steps"] == 2
    finally:
        sa.close()
        comm.close()


def test_refusals():
    sa = binding.SA(SMALL_PROSE, neighbours_per_step=K)
    try:
        assert sa.L.mgl_sa_exchange_cross_all(sa.h, None, 0, None) == MGL_EINVAL
        assert sa.L.mgl_sa_exchange_cross_all(None, None, 0, None) == MGL_EINVAL
        with pytest.raises(binding.MglError):
            sa.slab_hash(literal_slab(len(SMALL_PROSE) - 1))
    finally:
        sa.close()


def test_cli_three_chains_cross_all(tmp_path):
    data = corpus.enwik_like(3000, 0x64)
    f = tmp_path / "in.bin"
    f.write_bytes(data)
    comm = "/dev/shm/mgl_test_cli_cross_all_%d" % os.getpid() if os.path.isdir("/dev/shm") else str(tmp_path / "comm.shm")
    env = dict(os.environ, MGL_COMM_TIMEOUT_S="60")
    cmd = [build.CLI, "--epochs", "2", "--phases", "2", "--neighbours", "128", "--chains", "3", "--device", "0", "--transport", "shm",
           "--comm-file", comm, "--comm-nonce", "616161", "--exchange", "cross-all", "--cross-grain", "64", "--save-slab", str(tmp_path / "best.slab")]
    ps = [subprocess.Popen(cmd + ["--rank", str(r), str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env) for r in (2, 1, 0)]
    outs = [p.communicate(timeout=300) for p in ps][::-1]  # by rank
    assert all(p.returncode == 0 for p in ps), [o[1].decode()[-400:] for o in outs]
    ex = [[ln for ln in o[1].decode().splitlines() if ln.startswith("exchange:")] for o in outs]
    assert all(len(e) == 4 for e in ex)  # one per epoch, no plain exchange behind the last
    for lines in zip(*ex):
        assert all("cross-all" in ln and "distinct" in ln and "parents from chains [" in ln and "adopted" in ln for ln in lines), lines
        # D, the parents and the costs are the same everywhere; `adopted` is the chain's own
        assert len({ln.split(", adopted")[0] for ln in lines}) == 1, lines
        assert len({ln.split("best ")[-1].split(" bytes")[0] for ln in lines}) == 1, lines
    final = {e[-1].split("best ")[-1].split(" bytes")[0] for e in ex}
    assert len(final) == 1 and float(final.pop()) > 18  # every chain ends at the same cost
    assert outs[1][0] == outs[2][0] == b""  # rank 0 alone writes the stream
    assert lzma.decompress(outs[0][0], format=lzma.FORMAT_ALONE) == data
    costs = set()
    for name in ("best.slab", "best.slab.rank1", "best.slab.rank2"):  # every chain's own best slab decodes, at the common cost
        raw = (tmp_path / name).read_bytes()
        assert raw[:8] == b"MGLSLAB1" and int.from_bytes(raw[8:16], "little") == len(data)
        costs.add(int.from_bytes(raw[16:24], "little"))
        slab = np.frombuffer(raw[24:], dtype=binding.PACKET)
        assert lzma.decompress(binding.emit_stream(data, slab), format=lzma.FORMAT_ALONE) == data
    assert len(costs) == 1
    assert not os.path.exists(comm)
