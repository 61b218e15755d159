"""The focus window on the device (mgl_sa_set_focus, mgl_sa_focus; k_targets of csrc/mgl_kernels2.hip): the target rule against a
numpy restatement entry for entry, prefix windows against the CPU oracle bit for bit (the oracle's whole-file rule with
orc_set_strata(Ko), P K = b Ko, draws from the same ordinals), any window on both engines, runs that leave everything below
the window untouched, setting and clearing, and two chains that take their slices round by round.  `-m gpu`."""
import functools
import lzma
import multiprocessing as mp
import os
import queue
import shutil
import subprocess
import time

import numpy as np
import pytest

from _focus_chain import K, ROUNDS, STEPS, chain
from _libs import Oracle, assert_same_base, canonical_base, literal_slab, walk
from _validity import violations
from megalania_amd import binding, build, corpus

pytestmark = pytest.mark.gpu

MGL_EINVAL = -1
SEED = 20260
WIN_NONE, WIN_DROPPED = 0xFFFFFFFF, 0xFFFFFFFE
_BASE = corpus.enwik_like(6000, 0x71)
DATA = _BASE + _BASE[1000:3277]  # 8 277 bytes (not a multiple of 64); the repeated stretch gives the greedy parse long matches
N = len(DATA)
MIDDLE = (3000, 5500)  # crosses 4 096, the edge of a block of the prefix sums


def P(slab):
    return np.ascontiguousarray(slab).astype(binding.PACKET)


def as_list(pk):
    return [(int(p["type"]), int(p["dist"]), int(p["len"])) for p in pk]


def same(a, b):
    return bool((P(a) == P(b)).all())  # field by field: the records have padding


def journal(diffs, nd, j):
    return [(int(d["position"]), as_list([d["old"]])[0], as_list([d["new"]])[0]) for d in diffs[j][: nd[j]]]


def ordinals(starts, lo, hi):
    """(a, b - a) of the rule: packet starts below lo and below hi; an empty window stands for the packet that covers lo"""
    a, b = int(np.searchsorted(starts, lo, side="left")), int(np.searchsorted(starts, hi, side="left"))
    if b == a:
        a -= 1
    return a, b - a


def target_rule(sa, starts, lo, hi, seed, step, K_):
    """the K targets of a step under window [lo, hi): neighbour j takes ordinal a + j (b - a) / K + u % width"""
    a, cnt = ordinals(starts, lo, hi)
    out = []
    for j in range(K_):
        o0, o1 = j * cnt // K_, (j + 1) * cnt // K_
        u = int(sa.L.mgl_rng_draw_at(seed, step, j, 0))
        out.append(int(starts[a + o0 + (u % (o1 - o0) if o1 > o0 else 0)]))
    return out, cnt


@functools.lru_cache(maxsize=None)
def greedy_slab():
    """the greedy parse of DATA as the device makes it (stale entries included), and its cost"""
    sa = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED)
    try:
        sa.seed_greedy(8)
        slab, cost = sa.current()
        return P(slab), cost
    finally:
        sa.close()


def targets_of(sa):
    return [int(t) for t in sa.debug_dump(binding.DUMP.WINDOWS).reshape(-1, 2)[:, 0]]


# ---- 1. the target rule
def rule_windows(slab):
    starts = np.array(walk(slab))
    lens = slab["len"][starts]
    long_at = int(starts[int(np.argmax(lens))])
    assert int(lens.max()) >= 8  # a long match: a window strictly inside it holds no packet start
    mid = len(starts) // 2
    wins = [(63, 4095), (64, 4096), (65, 4097), (0, 63), (0, 64), (0, 65), (63, 64), (64, 65), (4095, 4096), (4096, 4097), (4095, N), (4096, N),
            (4097, N), (100, N), (0, N),
            (int(starts[mid]), int(starts[mid]) + 1),            # one byte, on a packet start
            (long_at + 2, long_at + 5), (long_at + 1, long_at + 2),  # strictly inside one long match: empty
            (int(starts[mid]), int(starts[mid + 10])),           # ten packets, fewer than K
            (int(starts[-1]), N), (N - 1, N)]                    # the last packet; the last byte
    return starts, wins


@pytest.mark.parametrize("K_", [K, 1], ids=["K64", "K1"])
def test_targets_equal_the_rule(K_):
    slab, _ = greedy_slab()
    starts, wins = rule_windows(slab)
    on = set(int(s) for s in starts)
    sa = binding.SA(DATA, accept="single", neighbours_per_step=K_, seed=SEED)
    try:
        sa.set_slab(slab)
        seen_empty = seen_few = seen_shared = False
        for i, (lo, hi) in enumerate(wins):
            sa.set_focus(lo, hi)
            step = 3 + i
            sa.neighbours(step, want_diffs=False)
            want, cnt = target_rule(sa, starts, lo, hi, SEED, step, K_)
            got = targets_of(sa)
            assert got == want, ((lo, hi), [(j, g, w) for j, (g, w) in enumerate(zip(got, want)) if g != w][:5])
            assert sa.focus() == (lo, hi, cnt), (lo, hi)
            inside = [s for s in on if lo <= s < hi]
            if inside:
                assert cnt == len(inside) and all(lo <= t < hi and t in on for t in got), (lo, hi)
            else:  # the packet that covers lo
                cover = int(starts[np.searchsorted(starts, lo, side="right") - 1])
                assert cnt == 1 and cover < lo and got == [cover] * K_, (lo, hi)
                seen_empty = True
            seen_few |= 1 < cnt < K
            seen_shared |= len(set(got)) < len(got)
        assert seen_empty and seen_few and (seen_shared or K_ == 1)
        # no window: the whole walk, the rule of the default targets
        sa.set_focus(0, 0)
        sa.neighbours(99, want_diffs=False)
        want, cnt = target_rule(sa, starts, 0, N, SEED, 99, K_)
        assert targets_of(sa) == want and sa.focus() == (0, 0, len(starts)) and cnt == len(starts)
    finally:
        sa.close()


# ---- 2. prefix windows against the oracle
def prefix_cases():
    def lit(n):
        return DATA[:n], literal_slab(n)

    greedy, _ = greedy_slab()
    greedy = greedy.copy()
    starts = walk(greedy)
    if len(starts) % 2:
        # an even number of packets: one MATCH of even length becomes literals (behind the last rep packet, if the parse has any:
        # the rep distances of what follows a MATCH change with it)
        types = greedy["type"][starts]
        last_rep = max([s for s, t in zip(starts, types) if t in (binding.SHORT_REP, binding.LONG_REP)], default=-1)
        at = [s for s, t in zip(starts, types) if t == binding.MATCH and s > last_rep and int(greedy["len"][s]) % 2 == 0][-1]
        for q in range(at, at + int(greedy["len"][at])):
            greedy[q] = (binding.LITERAL, 0, 1)
        starts = walk(greedy)
    assert len(starts) % 2 == 0
    return [("literal8192", *lit(8192), 2048, 256), ("literal8200", *lit(8200), 4100, 128),
            ("greedy", DATA, greedy, int(starts[len(starts) // 2]), 2 * K)]


@pytest.mark.parametrize("case", [0, 1, 2], ids=["literal8192", "literal8200", "greedy"])
def test_prefix_window_equals_the_oracle(case):
    name, data, slab, hi, Ko = prefix_cases()[case]
    starts = np.array(walk(slab))
    b = int(np.searchsorted(starts, hi, side="left"))
    assert len(starts) * K == b * Ko, (name, len(starts), b)  # P K = b Ko: the oracle's slices of the walk are the device's of the window
    o = Oracle(data, dict_limit=0x400000)
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=SEED)
    try:
        sa.set_slab(P(slab))  # refuses a slab that is no valid parse
        sa.set_focus(0, hi)
        assert sa.focus() == (0, hi, b)
        outcomes = set()
        for step in (0, 11):
            costs, nd, diffs = sa.neighbours(step)
            win = sa.debug_dump(binding.DUMP.WINDOWS).reshape(-1, 2)
            win2 = sa.debug_dump(binding.DUMP.SOFT_ENDS)
            for j in range(K):
                st, cost, od, w = o.neighbour_ex(slab, SEED, step, j, K=Ko)
                outcomes.add(st)
                assert int(win[j, 0]) == w[0] < hi, (name, step, j, win[j], w)
                assert int(costs[j]) == cost and (st == 1) == (int(costs[j]) != binding.INVALID_COST), (name, step, j, int(costs[j]), cost, st)
                if st == 1:
                    assert journal(diffs, nd, j) == journal([od], [len(od)], 0), (name, step, j)
                    assert (int(win[j, 0]), int(win[j, 1]), int(win2[j]) & 0x7FFFFFFF, int(win2[j]) >> 31) == w, (name, step, j, win[j], win2[j], w)
                else:  # failed and dropped generates agree, too
                    assert int(nd[j]) == 0 and int(win[j, 1]) == (WIN_NONE if st == 0 else WIN_DROPPED), (name, step, j, st, win[j])
        assert 1 in outcomes
    finally:
        sa.close()


# ---- 3. any window, both engines
def test_middle_window_on_both_engines():
    slab, _ = greedy_slab()
    o = Oracle(DATA, dict_limit=0x400000)
    starts = np.array(walk(slab))
    lo, hi = MIDDLE
    got = {}
    for fullwalk in (False, True):
        sa = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, fullwalk=fullwalk)
        try:
            sa.set_slab(slab)
            sa.set_focus(lo, hi)
            for step in (5, 6):
                costs, nd, diffs = sa.neighbours(step)
                want, _ = target_rule(sa, starts, lo, hi, SEED, step, K)
                assert targets_of(sa) == want, (fullwalk, step)
                got[fullwalk, step] = ([int(c) for c in costs], [journal(diffs, nd, j) for j in range(K)])
        finally:
            sa.close()
    for step in (5, 6):
        assert got[False, step] == got[True, step], step  # MGL_F_FULLWALK: the same costs and journals
        costs, journals = got[False, step]
        ok = [j for j in range(K) if costs[j] != binding.INVALID_COST]
        assert len(ok) >= K // 2
        for j in ok:
            copy = slab.copy()
            assert journals[j] and min(p for p, _, _ in journals[j]) >= lo, (step, j)  # nothing below the window is written
            for p, old, new in journals[j]:
                assert as_list([copy[p]])[0] == old
                copy[p] = new
            assert o.cost_slab(copy)["total"] == costs[j], (step, j)
            assert violations(DATA, copy, 0x400000) == [], (step, j)


# ---- 4. runs
@pytest.mark.parametrize("start", ["greedy", "literal"])
@pytest.mark.parametrize("mode", ["single", "bulk", "auto"])
def test_runs_leave_everything_below_the_window(mode, start):
    lo, hi = MIDDLE
    begin = greedy_slab()[0] if start == "greedy" else P(literal_slab(N))
    o = Oracle(DATA, dict_limit=0x400000)
    sa = binding.SA(DATA, accept=mode, neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    ref = binding.SA(DATA, accept="single", neighbours_per_step=8)
    # the full-walk engine takes single steps only (mgl_sa_set_accept_mode refuses bulk on it): it follows the single-step runs
    full = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, iters_per_epoch=N, fullwalk=True) if mode == "single" else None
    try:
        for h in (sa, full):
            if h is not None:
                h.set_slab(begin)
                h.set_focus(lo, hi)
        st = sa.run(40)
        assert st["steps"] == 40 and st["accepted"] > 0 and sa.focus()[:2] == (lo, hi)
        if mode == "bulk":
            assert st["bulk_steps"] == 40
        cur, cur_cost = sa.current()
        bst, best_cost = sa.best()
        assert st["current_cost"] == cur_cost and st["best_cost"] == best_cost != 0
        for what, slab in (("current", cur), ("best", bst)):
            assert same(slab[:lo], begin[:lo]), (what, np.nonzero(P(slab)[:lo] != begin[:lo])[0][:5])
            assert violations(DATA, P(slab), 0x400000) == [], what
        assert not same(cur, begin)
        assert cur_cost == o.cost_slab(P(cur))["total"] and best_cost == o.cost_slab(P(bst))["total"]
        ref.set_slab(cur)
        assert ref.current()[1] == cur_cost
        assert_same_base(canonical_base(sa, cur), canonical_base(ref, cur), (mode, start))
        if full is not None:
            fs = full.run(40)
            fcur, fcur_cost = full.current()
            fbst, fbest_cost = full.best()
            assert (fcur_cost, fbest_cost, fs["accepted"], fs["evaluations"]) == (cur_cost, best_cost, st["accepted"], st["evaluations"])
            assert same(fcur, cur) and same(fbst, bst)
    finally:
        for h in (sa, ref, full):
            if h is not None:
                h.close()


# ---- 5. setting and clearing
@pytest.mark.parametrize("mode", ["single", "bulk"])
def test_a_new_window_holds_from_the_next_run_on(mode):
    """window A for the first step, window B for the next three, set between two mgl_sa_run calls: every target of the second call
    lies in B's packets -- also those of its later steps, which are made ahead, beside the accept of the step before.  Handle
    `b` takes the same steps one call each, so that every step's targets can be read."""
    slab, _ = greedy_slab()
    A, B = (200, 2100), (6000, 8000)
    a = binding.SA(DATA, accept=mode, neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    b = binding.SA(DATA, accept=mode, neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    try:
        for h in (a, b):
            h.set_slab(slab)
            h.set_focus(*A)
            h.run(1)
            assert all(A[0] <= x < A[1] for x in targets_of(h)), (mode, targets_of(h))
            h.set_focus(*B)
        a.run(3)
        for s in (1, 2, 3):
            before = P(b.current()[0])
            b.run(1)
            want, _ = target_rule(b, np.array(walk(before)), *B, SEED, s, K)
            assert targets_of(b) == want and all(B[0] <= x < B[1] for x in want), (mode, s)
        assert targets_of(a) == targets_of(b)
        assert same(a.current()[0], b.current()[0]) and a.current()[1] == b.current()[1]
        assert same(a.best()[0], b.best()[0]) and a.best()[1] == b.best()[1]
        assert same(a.current()[0][:A[0]], slab[:A[0]])
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("mode", ["single", "bulk"])
def test_targets_follow_the_walk_inside_a_run(mode):
    """several steps in one call under one window: each step's targets, the ones made ahead included, are the rule's on the slab
    that step began from"""
    slab, _ = greedy_slab()
    lo, hi = MIDDLE
    a = binding.SA(DATA, accept=mode, neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    b = binding.SA(DATA, accept=mode, neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    try:
        for h in (a, b):
            h.set_slab(slab)
            h.set_focus(lo, hi)
        a.run(6)  # one call: steps 1..5 use targets made ahead
        for s in range(6):  # one call per step: every step makes its targets itself
            before = P(b.current()[0])
            b.run(1)
            want, _ = target_rule(b, np.array(walk(before)), lo, hi, SEED, s, K)
            assert targets_of(b) == want, (mode, s)
        assert targets_of(a) == targets_of(b)
        assert same(a.current()[0], b.current()[0]) and a.current()[1] == b.current()[1]
    finally:
        a.close()
        b.close()


def trajectory(sa, steps=20):
    out = []
    for _ in range(steps):
        st = sa.run(1)
        out.append((st["current_cost"], st["best_cost"], st["accepted"], st["evaluations"], st["failed"], tuple(targets_of(sa))))
    return out, P(sa.current()[0]), P(sa.best()[0])


def test_clearing_and_the_whole_file_window_change_nothing():
    slab, _ = greedy_slab()
    made = []
    try:
        for how in ("untouched", "set-then-cleared", "whole-file"):
            sa = binding.SA(DATA, accept="auto", neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
            made.append(sa)
            sa.set_slab(slab)
            if how == "set-then-cleared":
                sa.set_focus(*MIDDLE)
                assert sa.focus()[:2] == MIDDLE
                sa.set_focus(0, 0)
            if how == "whole-file":
                sa.set_focus(0, N)
            assert sa.focus() == ((0, N) if how == "whole-file" else (0, 0)) + (len(walk(slab)),)
        runs = [trajectory(sa) for sa in made]
        for r in runs[1:]:
            assert r[0] == runs[0][0] and same(r[1], runs[0][1]) and same(r[2], runs[0][2])
    finally:
        for sa in made:
            sa.close()


def test_refusals_leave_the_handle_as_it_was():
    slab, _ = greedy_slab()
    plain = binding.SA(DATA, accept="auto", neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    sa = binding.SA(DATA, accept="auto", neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    held = binding.SA(DATA, accept="auto", neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    held_plain = binding.SA(DATA, accept="auto", neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    pos = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, flags=binding.F_POSITION_TARGETS)
    try:
        for h in (plain, sa, held, held_plain):
            h.set_slab(slab)
        held.set_focus(*MIDDLE)
        held_plain.set_focus(*MIDDLE)
        for h, before in ((sa, (0, 0)), (held, MIDDLE)):
            for lo, hi in ((5, 5), (6, 5), (N, N), (0, N + 1), (3, N + 1), (N, N + 1), (1, 0), (1 << 40, 1 << 41), (N - 1, 1 << 32)):
                assert h.L.mgl_sa_set_focus(h.h, lo, hi) == MGL_EINVAL, (lo, hi)
                with pytest.raises(binding.MglError) as e:
                    h.set_focus(lo, hi)
                assert e.value.rc == MGL_EINVAL
                assert h.focus()[:2] == before  # the window in force stays
        assert trajectory(sa, 8)[0] == trajectory(plain, 8)[0]
        assert trajectory(held, 8)[0] == trajectory(held_plain, 8)[0]
        # position draws have no targets kernel: no window, and the handle runs on
        for lo, hi in ((0, 0), MIDDLE, (0, N)):
            assert pos.L.mgl_sa_set_focus(pos.h, lo, hi) == MGL_EINVAL
        assert pos.run(2)["steps"] == 2
    finally:
        for h in (plain, sa, held, held_plain, pos):
            h.close()


def test_the_window_stays_across_epochs_slabs_and_seeds():
    sa = binding.SA(DATA, accept="single", neighbours_per_step=K, seed=SEED, iters_per_epoch=N)
    try:
        sa.set_focus(*MIDDLE)
        sa.run(2)
        for change in (lambda: sa.begin_epoch(0), lambda: sa.seed_greedy(8), lambda: sa.set_slab(greedy_slab()[0]), lambda: sa.run(2),
                       lambda: sa.begin_epoch(1, from_best=True), lambda: sa.seed_adaptive(passes=1)):
            change()
            assert sa.focus()[:2] == MIDDLE
            starts = np.array(walk(P(sa.current()[0])))
            sa.neighbours(1000, want_diffs=False)
            want, cnt = target_rule(sa, starts, *MIDDLE, SEED, 1000, K)
            assert targets_of(sa) == want and sa.focus()[2] == cnt
    finally:
        sa.close()


# ---- 6. two chains
@functools.lru_cache(maxsize=None)
def two_chains():
    path = ("/dev/shm" if os.path.isdir("/dev/shm") else "/tmp") + "/mgl_test_focus_%d" % os.getpid()
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=chain, args=(r, 2, path, 0xF0C5, DATA, out)) for r in range(2)]
    for p in procs:
        p.start()
    res, deadline = {}, time.monotonic() + 300
    try:
        while len(res) < 2:
            try:
                r, start, start_cost, rows = out.get(timeout=0.5)
                res[r] = (np.frombuffer(start, dtype=binding.PACKET), start_cost, rows)
            except queue.Empty:
                assert all(p.exitcode in (None, 0) for p in procs), [p.exitcode for p in procs]
                assert time.monotonic() < deadline
    finally:
        for p in procs:
            p.join(timeout=90)
        for p in procs:
            if p.is_alive():
                p.kill()
    assert [p.exitcode for p in procs] == [0, 0]
    assert not os.path.exists(path)
    return [res[0], res[1]]


def test_two_chains_take_their_slices():
    res = two_chains()
    start, start_cost = res[0][0], res[0][1]
    assert same(res[1][0], start) and res[1][1] == start_cost  # a common slab
    o = Oracle(DATA, dict_limit=0x400000)
    for rnd in range(ROUNDS):
        rows = [res[r][2][rnd] for r in range(2)]
        common = np.frombuffer(rows[0]["epoch_start"], dtype=binding.PACKET)
        for r, row in enumerate(rows):
            lo, hi = binding.focus_slice(N, 2, r, rnd)
            assert row["window"] == (lo, hi) and row["focus"][:2] == (lo, hi) and row["steps"] == STEPS
            # every epoch starts from the slab both chains hold ...
            assert same(np.frombuffer(row["epoch_start"], dtype=binding.PACKET), common) and row["epoch_cost"] == rows[0]["epoch_cost"]
            # ... and the search leaves it as it was below the chain's slice
            searched = np.frombuffer(row["searched"], dtype=binding.PACKET)
            assert same(searched[:lo], common[:lo]), (rnd, r)
            assert row["searched_cost"] <= row["epoch_cost"] and row["searched_cost"] == o.cost_slab(P(searched))["total"]
        if rnd == 0:
            assert same(common, start) and [row["window"] for row in rows] == [(0, N // 2), (N // 2, N)]
            assert all(row["searched_cost"] < start_cost for row in rows)  # both found something in their own half
        else:
            assert [row["window"] for row in rows] == [(0, N // 4), (N // 4, N)]
        # behind the exchange: one best slab, no dearer than the cheaper parent
        assert rows[0]["hash"] == rows[1]["hash"] and rows[0]["cost"] == rows[1]["cost"]
        assert same(np.frombuffer(rows[0]["best"], dtype=binding.PACKET), np.frombuffer(rows[1]["best"], dtype=binding.PACKET))
        assert rows[0]["cost"] <= min(row["searched_cost"] for row in rows)
        assert rows[0]["cost"] == o.cost_slab(P(np.frombuffer(rows[0]["best"], dtype=binding.PACKET)))["total"]
        assert violations(DATA, P(np.frombuffer(rows[0]["best"], dtype=binding.PACKET)), 0x400000) == []
    # begin_epoch(from_best) accepted what the last exchange left
    assert res[0][2][ROUNDS]["final_cost"] == res[1][2][ROUNDS]["final_cost"] == res[0][2][ROUNDS - 1]["cost"]


def test_two_chains_cross_pieces_of_both():
    """round 0: the chains improved different halves of a common slab, so the child takes regions of both and beats both"""
    rows = [two_chains()[r][2][0] for r in range(2)]
    x = rows[0]["xs"]["cross"]
    assert rows[0]["xs"]["distinct"] == 2 and x["parents"] == 2
    assert all(n > 0 for n in x["regions_from"][:2]), x
    assert x["adopted"] == 2 and x["child_cost"] < min(x["parent_cost"][:2])


def test_cli_two_chains_focus_rank(tmp_path):
    data = corpus.enwik_like(16384, 0x33)
    f = tmp_path / "in.bin"
    f.write_bytes(data)
    comm = "/dev/shm/mgl_test_cli_focus_%d" % os.getpid() if os.path.isdir("/dev/shm") else str(tmp_path / "comm.shm")
    env = dict(os.environ, MGL_COMM_TIMEOUT_S="60")
    cmd = [build.CLI, "--chains", "2", "--transport", "shm", "--exchange", "cross-all", "--focus", "rank", "--adaptive-seed", "1", "--epochs", "2",
           "--phases", "1", "--neighbours", "256", "--device", "0", "--comm-file", comm, "--comm-nonce", "717171"]
    ps = [subprocess.Popen(cmd + ["--rank", str(r), str(f)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env) for r in (1, 0)]
    outs = [p.communicate(timeout=300) for p in ps][::-1]  # by rank
    assert all(p.returncode == 0 for p in ps), [o[1].decode()[-400:] for o in outs]
    ex = [[ln for ln in o[1].decode().splitlines() if ln.startswith("exchange:")] for o in outs]
    assert all(len(e) == 2 for e in ex)
    final = {e[-1].split("best ")[-1].split(" bytes")[0] for e in ex}
    assert len(final) == 1  # both chains end at the same cost
    assert outs[1][0] == b""  # rank 0 alone writes the stream
    stream = outs[0][0]
    assert lzma.decompress(stream, format=lzma.FORMAT_ALONE) == data
    if shutil.which("xz"):
        x = subprocess.run(["xz", "-dc", "--format=lzma"], input=stream, capture_output=True, timeout=60)
        assert x.returncode == 0 and x.stdout == data
    assert not os.path.exists(comm)


def test_cli_focus_range(tmp_path):
    data = corpus.enwik_like(8192, 0x34)
    f = tmp_path / "in.bin"
    f.write_bytes(data)
    base = [build.CLI, "--greedy-seed", "8", "--epochs", "1", "--phases", "1", "--neighbours", "64", "--steps", "20", "--accept", "single"]
    slabs = {}
    for name, extra in (("plain", []), ("focus", ["--focus", "4096:6000"])):
        r = subprocess.run(base + extra + ["--save-slab", str(tmp_path / (name + ".slab")), str(f)], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-400:]
        assert lzma.decompress(r.stdout, format=lzma.FORMAT_ALONE) == data
        raw = (tmp_path / (name + ".slab")).read_bytes()
        slabs[name] = np.frombuffer(raw[24:], dtype=binding.PACKET)
    # the greedy parse is the same in both runs; under the window everything below 4 096 is still the greedy parse
    sa = binding.SA(data, accept="single", neighbours_per_step=64)
    try:
        sa.seed_greedy(8)
        greedy = P(sa.current()[0])
    finally:
        sa.close()
    assert same(slabs["focus"][:4096], greedy[:4096]) and not same(slabs["focus"], greedy)
    assert not same(slabs["plain"][:4096], greedy[:4096])  # without it the search writes there
    # a window beyond the input is refused when the size is known
    r = subprocess.run(base + ["--focus", "4096:9000", str(f)], capture_output=True, timeout=300)
    assert r.returncode != 0 and r.stdout == b"" and b"mgl_sa_set_focus" in r.stderr
