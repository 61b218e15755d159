"""The oracle's restatement of the batch accept's clusters (oracle/mgl_oracle.c:bulk_clusters) against a
brute-force one in Python, the seeds of the GPU cluster-boundary test, and the header's list of limit ids.  CPU only."""
import os
import re

import numpy as np
import pytest

from _libs import LITERAL, LONG_REP, MATCH, ROOT, SHORT_REP, Oracle, literal_slab
from test_oracle_golden import doubled_letters

MGL_BATCH_MAX = 192


def advance(st, pk):
    """the walk state without the probabilities (lzma_state.c:29-81): (pos, ctx_state, rep distances)"""
    pos, cs, d = st
    t, dist, ln = int(pk["type"]), int(pk["dist"]), int(pk["len"])
    if t == MATCH:
        d = (dist, d[0], d[1], d[2])
    elif t == LONG_REP:
        d = (d[dist],) + tuple(x for i, x in enumerate(d) if i != dist)
    cs = {LITERAL: 0 if cs < 4 else (cs - 3 if cs < 10 else cs - 6), MATCH: 7 if cs < 7 else 10,
          SHORT_REP: 9 if cs < 7 else 11, LONG_REP: 8 if cs < 7 else 11}[t]
    return pos + ln, cs, d


def brute_force_clusters(o, before, after, seed, step, K):
    """taken moves = the neighbours of `before` whose whole journal is in `after`; clusters by the device's rule; every
    cluster's re-join point by walking `before` against `before` + the cluster's journals"""
    n = len(before)
    taken = {}
    for j in range(K):
        st, _, diffs, win = o.neighbour_ex(before, seed, step, j, K=K)
        if st != 1 or len(diffs) == 0:
            continue
        if all(before[d["position"]] == d["old"] and after[d["position"]] == d["new"] for d in diffs):
            taken.setdefault(win[0], (j, win, diffs))   # (two neighbours with one target conflict: the smaller j is listed)
    clusters, reach = [], 0
    for target in sorted(taken):
        j, win, diffs = taken[target]
        if not clusters or target >= reach:
            clusters.append(dict(members=[], journal={}))
        clusters[-1]["members"].append((j,) + tuple(win))
        clusters[-1]["journal"].update({int(d["position"]): d["new"] for d in diffs})
        reach = max(reach, win[1])
    out = []
    for q, c in enumerate(clusters):
        first, last = min(c["journal"]), max(c["journal"])
        st = (0, 0, (0, 0, 0, 0))
        while st[0] < first:
            st = advance(st, before[st[0]])
        assert st[0] == first
        nb = bs = st
        new_at = lambda p: c["journal"].get(p, before[p])
        while nb[0] < n or bs[0] < n:
            if nb == bs and nb[0] > last:
                break
            if nb[0] <= bs[0] and nb[0] < n:
                if bs[0] == nb[0]:
                    bs = advance(bs, before[bs[0]])
                nb = advance(nb, new_at(nb[0]))
            else:
                bs = advance(bs, before[bs[0]])
        out.append(dict(first=first, last=last, rejoin=max(nb[0], bs[0]), next_first=None, members=c["members"]))
    for q in range(len(out) - 1):
        out[q]["next_first"] = out[q + 1]["first"]
    return out


@pytest.mark.parametrize("name,seed,K", [("doubled", 1, 96), ("runs", 5, 48)])
def test_oracle_cluster_table_equals_a_brute_force_restatement(name, seed, K):
    data = {"doubled": doubled_letters(seed, 1500),
            "runs": b"a" * 300 + b"ab" * 200 + bytes(range(64)) * 3 + b"a" * 120 + b"abcabcabd" * 40}[name]
    n = len(data)
    o = Oracle(data)
    slab, best = literal_slab(n), literal_slab(n)
    cur = best_cost = 0
    clusters = joined = 0
    over0 = o.bulk_cluster_overruns()
    for s in range(24):
        before = slab.copy()
        res = o.sa_batched(slab, best, cur, best_cost, seed=seed * 7717, K=K, phase=0, iters_per_epoch=n, step_begin=s, step_end=s + 1,
                           iter0=s * K, modes=[1])
        cur, best_cost = res["cur"], res["best"]
        if not int(res["trace"][0, 1]):
            continue
        got = o.bulk_cluster_table()
        want = brute_force_clusters(o, before, slab, seed * 7717, s, K)
        assert got == want, (name, s)
        assert 1 <= sum(len(c["members"]) for c in got) <= int(res["trace"][0, 1])   # (a taken move that changes nothing is in no cluster)
        for c in got:
            assert c["first"] <= c["last"] < c["rejoin"] and (c["next_first"] is None or c["rejoin"] <= c["next_first"]), (name, s, c)
        clusters += len(got)
        joined += sum(len(c["members"]) - 1 for c in got)
    assert o.bulk_cluster_overruns() == over0
    # not vacuous: at least ten clusters went through the comparison, and on the rep-heavy input some move joined a cluster
    # because it starts inside an earlier move's hard window
    assert clusters >= 10 and (joined >= 1 or name != "doubled")


@pytest.mark.parametrize("seed", [1, 5])
def test_seeds_of_the_gpu_cluster_boundary_test(seed):
    """tests/test_gpu_accept_giveups.py:test_cluster_boundary_guard switches on the knob that splits clusters at the soft ends
    and asserts that the device's boundary guard fires.  That needs steps that take a move starting inside [soft end, end)
    of an earlier taken one, while at most MGL_BATCH_MAX moves are taken (more: the step is a rebuild anyway): checked
    here, on the oracle, for the same inputs, seeds and K -- together with the real rule's count staying at zero."""
    data = doubled_letters(seed, 2600)
    n, K, steps = len(data), 96, 60
    o = Oracle(data, dict_limit=0x400000)
    slab, best = literal_slab(n), literal_slab(n)
    cur = best_cost = 0
    over0, soft0 = o.bulk_cluster_overruns(), o.bulk_soft_overruns()
    pairs = 0
    for s in range(steps):
        res = o.sa_batched(slab, best, cur, best_cost, seed * 7717, K, 0, n, s, s + 1, iter0=s * K, modes=[1])
        cur, best_cost = res["cur"], res["best"]
        taken = int(res["trace"][0, 1])
        assert taken <= MGL_BATCH_MAX
        if taken:
            for c in o.bulk_cluster_table():
                m = c["members"]
                pairs += sum(1 for i in range(len(m)) for k in range(i) if m[k][3] <= m[i][1] < m[k][2])
    assert pairs >= 10
    assert o.bulk_soft_overruns() - soft0 >= 5      # steps on which the knob makes a walk reach the next cluster un-joined
    assert o.bulk_cluster_overruns() == over0       # ... and none under the real rule


def _header_enum_comments(header, name, prefix):
    """{NAME: (value text, comment)} of `enum name` in the public header; a comment runs to the next enumerator"""
    body = re.search(r"enum %s \{(.*?)\n\};" % name, header, re.S).group(1)
    out = {}
    for n, v, rest in re.findall(r"\b%s([A-Z0-9_]+) = (\(1u << \d+\)|[^,\s]+),?(.*?)(?=\n\t%s|\Z)" % (prefix, prefix), body, re.S):
        out[n] = (v, " ".join(rest.replace("/*", " ").replace("*/", " ").replace(" * ", " ").split()))
    return out


def test_header_documents_the_limit_ids_of_key_6():
    """include/megalania_hip.h lists every limit id mgl_debug_set key 6 takes, with its number and what it limits, and the
    give-up sites; csrc/mgl_base2.h uses the header's and defines none of its own."""
    base2 = open(os.path.join(ROOT, "megalania_amd", "csrc", "mgl_base2.h")).read()
    header = open(os.path.join(ROOT, "include", "megalania_hip.h")).read()
    assert not re.search(r"#define MGL_(LIM|GU)_", base2) and "include/megalania_hip.h" in base2
    lims = _header_enum_comments(header, "mgl_accept_limit", "MGL_LIM_")
    ids = {name: int(v) for name, (v, _) in lims.items() if name != "COUNT"}
    assert len(ids) == 18 and sorted(ids.values()) == list(range(1, 19))
    phrase = {"APPLY_EVENTS": "inserted / removed events of the accepted neighbour", "APPLY_GUARD": "iterations of its walk",
              "APPLY_SUB": "events of one context", "APPLY_SPAN": "rewritten chain entries of one context",
              "APPLY_PIECES": "pieces / checkpoint segments of one context", "APPLY_SHIFT": "entries a chain's tail may shift by in place",
              "POOL": "chain pool entries", "JOBS": "copy jobs per list", "SPAN_AREA": "span area entries", "SCRATCH": "save area entries",
              "BATCH_JOURNAL": "journal entries of one cluster", "BATCH_EVENTS": "staged events of one cluster",
              "BATCH_OPS": "bitmap / state-record ops of one cluster", "BATCH_GUARD": "iterations of a cluster's walk",
              "BATCH_SUB": "events of one kind per context", "BATCH_SHIFT": "entries a stretch may shift by in place",
              "BATCH_RUNS": "runs on the checkpoint list", "SOFT_REACH": "1 / 0: clusters are split at the members' soft window ends"}
    assert set(phrase) == set(ids)
    for name, num in ids.items():
        assert lims[name][1].startswith(phrase[name]), (name, num)
    dumps = _header_enum_comments(header, "mgl_dump_selector", "MGL_DUMP_")
    assert dumps["GIVEUP_SITES"][0] == "84" and dumps["GIVEUP_SITES"][1].startswith("one u32: the give-up sites of the in-place accepts")
    sites = list(_header_enum_comments(header, "mgl_giveup_site", "MGL_GU_").values())
    assert [v for v, _ in sites] == [f"(1u << {b})" for b in range(len(sites))] and len(sites) == 27
