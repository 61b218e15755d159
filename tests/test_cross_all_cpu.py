"""The exchange that crosses every chain's best slab (mgl_sa_exchange_cross_all, include/megalania_hip.h) without a GPU: the
selection of the parents and the slab hash restated in Python (tests/test_gpu_cross_all.py holds the device to both), the
all-gather of the host shared-memory transport across processes, the interface and the CLI's refusals."""
import ctypes as C
import multiprocessing as mp
import os
import subprocess
import tempfile

import numpy as np
import pytest

from megalania_amd import binding, build, corpus, multi_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_NONE = (1 << 54) - 1
M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15


def select_parents(keys, hashes):
    """keys[r] = (best cost or KEY_NONE) << 8 | r, hashes[r] = rank r's slab hash.  The ranks that hold a best slab in ascending
    key order, without those whose (cost, hash) an earlier one has, the first 8 of them: parent p's rank."""
    out, seen = [], set()
    for k in sorted(keys):
        r, cost = k & 0xFF, k >> 8
        if cost == KEY_NONE or (cost, hashes[r]) in seen:
            continue
        seen.add((cost, hashes[r]))
        out.append(r)
        if len(out) == binding.XO_MAX_PARENTS:
            break
    return out


def fin(z):
    """the splitmix64 finaliser"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def slab_hash_rule(slab):
    """h = sum over x < n of fin(packed[x] + (x + 1) * GOLD) mod 2^64, packed = dist | len << 32 | type << 48"""
    h = 0
    for x, (t, d, l) in enumerate(zip(slab["type"].tolist(), slab["dist"].tolist(), slab["len"].tolist())):
        h += fin(((d | l << 32 | t << 48) + (x + 1) * GOLD) & M64)
    return h & M64


def keys_of(costs):
    return [multi_gpu.pack_key(c, r) for r, c in enumerate(costs)]


def test_selection_properties_on_random_keys():
    rng = np.random.default_rng(7)
    for trial in range(300):
        world = int(rng.integers(1, 20))
        # few costs and few hashes, so that ties, duplicates and ranks without a slab all turn up
        costs = [int(c) for c in rng.choice([0, 0, 500, 600, 700, 800, 900, 1000, 1100, 1200, 1300], world)]
        hashes = [int(h) for h in rng.integers(0, 4, world)]
        keys = keys_of(costs)
        got = select_parents(keys, hashes)
        assert [keys[r] for r in got] == sorted(keys[r] for r in got)
        sigs = [(costs[r], hashes[r]) for r in got]
        assert len(set(sigs)) == len(sigs) and len(got) <= 8
        assert all(costs[r] != 0 for r in got)  # a rank without a best slab is never a parent
        live = {(costs[r], hashes[r]) for r in range(world) if costs[r]}
        assert len(got) == min(8, len(live))
        if got:  # the overall cheapest (lowest rank among equals) is parent 0, as in mgl_sa_exchange_best
            assert keys[got[0]] == min(keys)
        # the first rank of every (cost, hash) is the one that stays
        for r in got:
            assert r == min(k for k in range(world) if (costs[k], hashes[k]) == (costs[r], hashes[r]))


def test_selection_by_hand():
    # all ranks identical: one parent, the lowest rank
    assert select_parents(keys_of([700] * 5), [9] * 5) == [0]
    # nobody has a best slab
    assert select_parents(keys_of([0, 0, 0]), [0, 0, 0]) == []
    # nine distinct ranks: the dearest is left out, the others in cost order
    costs = [900, 100, 800, 200, 700, 300, 600, 400, 500]
    assert select_parents(keys_of(costs), list(range(9))) == [1, 3, 5, 7, 8, 6, 4, 2]
    # a cost tie between different hashes: both stay, the lower rank first; the same hash at another cost is another slab
    assert select_parents(keys_of([500, 400, 400, 400]), [1, 2, 3, 2]) == [1, 2, 0]
    assert select_parents(keys_of([500, 400]), [1, 1]) == [1, 0]
    # a rank without a best slab is skipped wherever it stands
    assert select_parents(keys_of([0, 300, 0, 200]), [0, 5, 0, 6]) == [3, 1]
    # duplicates do not use up the eight places
    assert select_parents(keys_of([100, 100] + [200 + i for i in range(8)]), [1, 1] + list(range(8))) == [0, 2, 3, 4, 5, 6, 7, 8]


def test_slab_hash_rule_sees_every_entry_and_its_position():
    lit = binding.literal_slab(3)
    assert slab_hash_rule(lit[:1]) == fin(((1 << 32 | 1 << 48) + GOLD) & M64)
    a = lit.copy()
    a[1] = (binding.MATCH, 0, 2)
    b = lit.copy()
    b[2] = (binding.MATCH, 0, 2)
    assert len({slab_hash_rule(lit), slab_hash_rule(a), slab_hash_rule(b)}) == 3  # the same entries at other positions
    assert slab_hash_rule(a) == slab_hash_rule(a.copy())


def _shm_dir():
    return "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()


def _word(rnd, rank):
    return (0xABCD000000000000 + rnd * 0x10001 + rank * 0x100000001) & M64 if rnd != 2 else M64 - rank


def _rank(path, nonce, rank, world, rounds, out):
    os.environ["MGL_COMM_TIMEOUT_S"] = "30"
    comm = binding.Comm.shm(path, nonce, rank, world)
    got = []
    for r in range(rounds):  # back to back: a fast rank's next word must not reach a slow rank's read of this one
        got.append(comm.allgather_u64(_word(r, rank)))
    low = comm.min_u64(1000 + rank)  # the min shares the staging area
    got.append(comm.allgather_u64(rank))
    comm.close()
    out.put((rank, got, low))


@pytest.mark.parametrize("world", [3, 5])
def test_allgather_across_processes(world):
    path = os.path.join(_shm_dir(), f"mgl_test_gather_{os.getpid()}_{world}")
    rounds = 6
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(path, 0xA11 + world, r, world, rounds, out)) for r in range(world)]
    for p in reversed(procs):
        p.start()
    res = dict((r, (got, low)) for r, got, low in (out.get(timeout=120) for _ in procs))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for k in range(world):
        got, low = res[k]
        for r in range(rounds):
            assert got[r] == [_word(r, q) for q in range(world)], (k, r)
        assert low == 1000 and got[rounds] == list(range(world))
    assert not os.path.exists(path)


def test_allgather_refuses_null_arguments():
    L = binding.hip_lib()
    word = C.c_uint64(0)
    assert L.mgl_comm_allgather_u64(None, 1, C.byref(word)) == -1
    assert L.mgl_slab_hash(None, None, C.byref(word)) == -1 and L.mgl_sa_exchange_cross_all(None, None, 0, None) == -1


def test_the_interface_names_the_new_calls():
    header = open(os.path.join(ROOT, "include", "megalania_hip.h")).read()
    for sym in ("mgl_comm_allgather_u64", "mgl_slab_hash", "mgl_sa_exchange_cross_all"):
        assert sym + "(" in header and sym in binding.HIP_SYMBOLS and hasattr(binding.hip_lib(), sym)
    assert "mgl_cross_all_stats" in header
    for field in ("chains_with_best", "distinct", "parent_rank[MGL_XO_MAX_PARENTS]", "own_parent", "fell_back", "mgl_cross_stats cross"):
        assert field in header, field
    # the header's layout: two u32, eight u32, two u32, then mgl_cross_stats (176 bytes, 8-aligned)
    S = binding.CrossAllStats
    assert (S.chains_with_best.offset, S.distinct.offset, S.parent_rank.offset, S.own_parent.offset, S.fell_back.offset) == (0, 4, 8, 40, 44)
    assert S.cross.offset == 48 and C.sizeof(S) == 48 + C.sizeof(binding.CrossStats) == 224
    assert callable(binding.SA.exchange_cross_all) and callable(binding.SA.slab_hash) and callable(binding.Comm.allgather_u64)
    assert callable(multi_gpu.exchange_cross_all_native)
    r = subprocess.run([build.CLI], capture_output=True, timeout=60)
    assert r.returncode != 0 and b"--exchange best|cross|cross-all" in r.stderr and b"mgl_sa_exchange_cross_all" in r.stderr
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "cross-all" in open(os.path.join(ROOT, doc)).read(), doc


@pytest.mark.parametrize("args", [
    ["--exchange", "cross-al"],
    ["--exchange", "cross-all", "--cross-grain"],
    ["--exchange", "cross-all", "--exchange", "best", "--cross-grain", "64"],
    ["--exchange", "cross-all", "--cross-grain", "64", "--chains", "2", "--rank", "0"],
    ["--exchange", "cross-all", "--chains", "3", "--rank", "3", "--comm-file", "some.comm", "--transport", "shm"],
    ["--exchange", "cross-all", "--chains", "2", "--rank", "0", "--comm-file", "some.comm", "--transport", "shm", "--props", "auto"],
], ids=["unknown-mode", "grain-without-value", "best-said-last", "chains-without-file", "rank-beyond-chains", "props-auto"])
def test_cli_refuses_before_it_touches_a_device(args, tmp_path):
    f = tmp_path / "in.bin"
    f.write_bytes(corpus.prose_like(64, 1))
    r = subprocess.run([build.CLI] + args + [str(f)], capture_output=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode != 0 and r.stdout == b""
    assert b"usage:" in r.stderr and b"no HIP device" not in r.stderr
    assert not os.path.exists(tmp_path / "some.comm")
