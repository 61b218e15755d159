"""The CPU oracle against the reference itself.  What the compiled reference (oracle/_ref/libmegalania_ref.so,
`make -C oracle`) gives for these cases -- walk costs, final states, streams, top-K lists, substrings, SA
trajectories under glibc rand() -- is recorded in tests/golden/oracle_vs_ref.json, and the oracle is checked
against that record everywhere.  Where the reference is built, it is checked against the same record too, so a
record that no longer matches the reference fails here.

The `random_starts` section does the same from seeded random parses with stale entries (tests/_random_parse.py): starts
that no search of the reference would reach, with matches, long reps and short reps under the packets of the walk, which the
reference's repair reads when a move uncovers them.

Re-record (where the reference is built): python tests/test_oracle_vs_ref.py REFERENCE_CHECKOUT"""
import json
import os
import re
import sys

import numpy as np
import pytest

from _libs import PACKET, Oracle, Ref, literal_slab, walk
from conftest import ROOT, rand_bytes, sha, sha_slab, slab_from_rle  # (puts the repository on sys.path when run as a script)
from megalania_amd import corpus
import _random_parse as rp

FIXTURE = os.path.join(ROOT, "tests", "golden", "oracle_vs_ref.json")


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _evolve(data, iters, seed):
    """A valid, SA-shaped slab made by the reference itself."""
    n = len(data)
    r = Ref(data)
    slab, best = literal_slab(n), literal_slab(n)
    Ref.lib().ref_srand(seed)
    r.sa_iters(slab, best, 0, 0, 0, n, 0, iters)
    return slab


def _on_walk(slab):
    return [(p, int(slab[p]["type"]), int(slab[p]["dist"]), int(slab[p]["len"])) for p in walk(slab)]


def _start(name, data, iters, seed):
    """The reference-evolved slab a case starts from, as recorded (packets on its walk, literals elsewhere); where the
    reference is built, it must evolve the same walk again."""
    slab = slab_from_rle(len(data), _fixture()["starts"][name]) if iters else literal_slab(len(data))
    if iters and Ref.available():
        assert _on_walk(_evolve(data, iters, seed)) == _on_walk(slab), name
    return slab


CASES = [
    ("lorem2k", corpus.lorem(2048), 500),
    ("enwik2k", corpus.enwik_like(2048, 0x51), 400),
    ("rand1k", rand_bytes(1024, 3), 200),
    ("zeros", b"\0" * 700, 150),
    ("two", b"ab", 0),  # SA on it would spin forever in the reference too (main.c:81-84: no neighbour exists)
    ("one", b"x", 0),
]
TRAJECTORY_DATA = corpus.enwik_like(1500, 0x99)


# name: (data, weights, len_mode); each under two generator seeds
RANDOM_STARTS = {
    "enwik2k": (lambda: corpus.enwik_like(2000, 0x42), rp.TEXT, "any"),
    "lorem2k": (lambda: corpus.lorem(2000), rp.TEXT, "any"),
    "doubled2k": (lambda: rp.doubled_letters(1, 2000), rp.REPS, "any"),
    "two_periods2k": (lambda: rp.two_periods(3), rp.REPS, "short"),
}
RANDOM_CASES = [(name, seed) for name in RANDOM_STARTS for seed in (1, 2)]


def _random_start(name, seed):
    make, weights, len_mode = RANDOM_STARTS[name]
    data = make()
    return data, rp.random_parse(data, seed, weights, len_mode)


def random_start_record(make_eng, seed_fn, data, start):
    return dict(walk=walk_record(make_eng(data), data, start),
                trajectories={str(step): trajectory_record(make_eng(data), seed_fn, start, step) for step in (0, 2)})


def _layout(L):
    return dict(sizeof_packet=L.ref_sizeof_packet(), num_probs=L.ref_num_probs(), sizeof_state=L.ref_sizeof_state())


def walk_record(eng, data, slab):
    """One case's figures from one engine (the oracle or the reference): the walk's cost, cumulative costs and final
    state, the stream, the top-K lists at positions on the walk and the substrings at positions of the input."""
    a = eng.cost_slab(slab, True)
    rec = dict(total=a["total"], cum=sha(a["cum"]), probs=sha(a["probs"]), ctx_state=int(a["ctx_state"]),
               dists=[int(x) for x in a["dists"]], stream=sha(np.frombuffer(eng.emit(slab), dtype=np.uint8)), top_k=[], substrings=[])
    w = walk(slab)
    rng = np.random.default_rng(5)
    for pos in sorted(set([w[0], w[-1]] + [w[i] for i in rng.integers(0, len(w), 12)])):
        pk, costs = eng.top_k(slab, pos, mode=0) if isinstance(eng, Oracle) else eng.top_k(slab, pos)
        rec["top_k"].append([pos, sha_slab(pk), [int(c) for c in costs]])
    for pos in sorted(set(int(x) for x in rng.integers(0, len(data), 16)) | {0, len(data) - 1}):
        for ml in (273, 3):
            offs, lens = eng.substrings(pos, ml)
            rec["substrings"].append([pos, ml, sha(offs), sha(lens)])
    return rec


def trajectory_record(eng, seed_fn, start, step):
    """Same glibc rand() stream, same costs, same accept decisions, same slabs: 500 SA iterations in two calls (successive
    calls must compose)."""
    n = len(start)
    slab, best = start.copy(), start.copy()
    seed_fn(1673551 + step)
    res = eng.sa_iters(slab, best, 0, 0, step, n, 0, 350)
    res2 = eng.sa_iters(slab, best, res["cur"], res["best"], step, n, 350, 500)
    return dict(slab=sha_slab(slab), best=sha_slab(best), trace=sha(res["trace"]), trace2=sha(res2["trace"]),
                cur=res2["cur"], best_cost=res2["best"], undo=res["undo"] + res2["undo"])


def test_layout_constants():
    rec = _fixture()["layout"]
    assert rec == dict(sizeof_packet=12, num_probs=2615, sizeof_state=5280)
    assert PACKET.itemsize == rec["sizeof_packet"] and Oracle(b"abc").nprobs == rec["num_probs"]
    if Ref.available():
        assert _layout(Ref.lib()) == rec


@pytest.mark.parametrize("name,data,iters", CASES, ids=[c[0] for c in CASES])
def test_walk_topk_emit(name, data, iters):
    slab = _start(name, data, iters, 1234)
    rec = _fixture()["walks"][name]
    assert walk_record(Oracle(data), data, slab) == rec
    if Ref.available():
        assert walk_record(Ref(data), data, slab) == rec


@pytest.mark.parametrize("step", [0, 1, 2])
def test_sa_trajectory(step):
    start = _start("trajectory", TRAJECTORY_DATA, 200 if step else 0, 42)
    rec = _fixture()["trajectories"][step]
    assert trajectory_record(Oracle(TRAJECTORY_DATA), Oracle.lib().orc_srand, start, step) == rec
    if Ref.available():
        assert trajectory_record(Ref(TRAJECTORY_DATA), Ref.lib().ref_srand, start, step) == rec


@pytest.mark.parametrize("name,seed", RANDOM_CASES, ids=[f"{n}-{s}" for n, s in RANDOM_CASES])
def test_random_starts(name, seed):
    """From a random parse with stale matches, long reps and short reps: the walk's figures, and 500 SA iterations in phase 0
    and in phase 2 (costs, accept decisions, undo-stack counts, final slabs with whatever the moves left off the walk)."""
    data, start = _random_start(name, seed)
    rec = _fixture()["random_starts"][f"{name}-{seed}"]
    assert sha_slab(start) == rec["start"]
    assert not rp.on_walk(start).all() and (start["type"][~rp.on_walk(start)] != 1).any()
    want = dict(walk=rec["walk"], trajectories=rec["trajectories"])
    assert random_start_record(Oracle, Oracle.lib().orc_srand, data, start) == want
    if Ref.available():
        assert random_start_record(Ref, Ref.lib().ref_srand, data, start) == want


def _record(reference_checkout):
    """Every expected value from the compiled reference; the reference's own perplexity_table.h for the bit-cost
    table that tests/test_host.py pins."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from make_golden import pk_list

    assert Ref.available(), "build oracle/_ref first: make -C oracle REF=" + reference_checkout
    body = open(os.path.join(reference_checkout, "src", "perplexity_table.h")).read().split("{", 1)[1]
    table = np.array([int(x) for x in re.findall(r"\d+", body)], dtype=np.uint16)
    assert len(table) == 2048
    starts = {name: pk_list(_evolve(data, iters, 1234)) for name, data, iters in CASES if iters}
    starts["trajectory"] = pk_list(_evolve(TRAJECTORY_DATA, 200, 42))
    out = dict(made_by="python tests/test_oracle_vs_ref.py: the compiled reference (oracle/_ref/libmegalania_ref.so)",
               layout=_layout(Ref.lib()), perplexity_table_sha256=sha(table), starts=starts, walks={}, trajectories=[],
               random_starts={})
    for name, data, iters in CASES:
        slab = slab_from_rle(len(data), starts[name]) if iters else literal_slab(len(data))
        out["walks"][name] = walk_record(Ref(data), data, slab)
    for step in (0, 1, 2):
        start = slab_from_rle(len(TRAJECTORY_DATA), starts["trajectory"]) if step else literal_slab(len(TRAJECTORY_DATA))
        out["trajectories"].append(trajectory_record(Ref(TRAJECTORY_DATA), Ref.lib().ref_srand, start, step))
    for name, seed in RANDOM_CASES:
        data, start = _random_start(name, seed)
        out["random_starts"][f"{name}-{seed}"] = dict(start=sha_slab(start), **random_start_record(Ref, Ref.lib().ref_srand, data, start))
    return out


if __name__ == "__main__":
    record = _record(sys.argv[1])
    with open(FIXTURE, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
