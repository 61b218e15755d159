"""The adaptive parse made again per segment, from its LZMA2 state reset and under its own lc/lp/pb (mgl_segment_reparse,
SA.segment_reparse, CLI --segment-reparse; DESIGN.md section 10, mgl_segparse.hip).  Every comparison is an exact integer or an
entry-for-entry slab: the starts against the host's segment cost, one whole-file segment against the existing parse kernels,
small inputs against the restatement of tests/_segment_parse.py, and the rule's promises -- a valid slab, costs the host
confirms, never a dearer total -- on inputs made to cross the cut, to lean on the reset's own rep and to fill all sixteen
segments.  chunk = 512 throughout, so that 8 KiB are many chunks.  `-m gpu`."""
import ctypes as C
import lzma
import re
import subprocess

import numpy as np
import pytest

import _segment_parse as R
import _segments as S
import _validity
from conftest import sha_slab
from megalania_amd import binding, build, corpus
from megalania_amd.binding import DUMP, MATCH, PACKET

pytestmark = pytest.mark.gpu

MGL_EINVAL, MGL_ERANGE = -1, -4
DICT = 0x400000
CHUNK = 512
GRAIN = 1024


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_all()


@pytest.fixture(scope="module")
def mixed():
    return S.mixed_input()


def seg(lo, hi, props):
    return dict(lo=lo, hi=hi, props=tuple(props))


def at_starts(slab, wanted, props):
    """segments whose inner cuts are `wanted`, each moved to the first packet start of `slab` at or above it"""
    starts = S.walk_starts(slab)
    cuts = [0] + [next(p for p in starts if p >= w) for w in wanted] + [len(slab)]
    assert cuts == sorted(set(cuts)), cuts
    return [seg(lo, hi, pr) for lo, hi, pr in zip(cuts, cuts[1:], props)]


def greedy_slab(data):
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        sa.seed_greedy(16)
        return sa.current()[0]
    finally:
        sa.close()


def reparse(data, slab, segs, **cfg):
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        return sa.segment_reparse(segs, slab, chunk=CHUNK, **cfg)
    finally:
        sa.close()


def check_promises(data, slab, segs, got, what):
    """what every call promises: a valid slab with the segments at packet starts, final_cost the host's figure for it, the same
    segments handed back, a strict gain or the input itself"""
    out, segs_out, stats, taken, ms = got
    total = lambda key: sum(st[key] for st in stats)
    print(f"{what}: n {len(data)}, {len(segs)} segments, taken {taken}, start {total('start_cost')} final {total('final_cost')}, {ms:.3f} ms; "
          f"best passes {[st['best_pass'] for st in stats]}")
    assert _validity.violations(data, out, DICT) == [], what
    starts = set(S.walk_starts(out))
    assert [(s["lo"], s["hi"], s["props"]) for s in segs_out] == [(s["lo"], s["hi"], tuple(s["props"])) for s in segs], what
    for s, so, st in zip(segs, segs_out, stats):
        assert s["lo"] in starts and (s["hi"] in starts or s["hi"] == len(data)), (what, s)
        assert st["start_cost"] == binding.host_segment_cost(data, slab, s["lo"], s["hi"], s["props"])[0], (what, s)
        assert st["final_cost"] == so["cost"] == binding.host_segment_cost(data, out, s["lo"], s["hi"], s["props"])[0], (what, s)
        assert st["best_pass"] is None or st["pass_cost"].index(min(st["pass_cost"])) == st["best_pass"], (what, st)  # ties to the lower pass
        assert st["best_pass"] is None or min(st["pass_cost"]) < st["start_cost"], (what, st)
    assert total("final_cost") <= total("start_cost"), what
    if taken:
        assert total("final_cost") < total("start_cost") and any(st["best_pass"] is not None for st in stats), what
    else:
        assert sha_slab(out) == sha_slab(slab) and all(st["final_cost"] == st["start_cost"] and st["best_pass"] is None for st in stats), what


def check_against_rule(data, slab, segs, got, what, **cfg):
    """the device's figures and its slab against segment_rule's, entry for entry"""
    out, _, stats, taken, _ = got
    want_out, want, want_taken = R.segment_rule(data, slab, [(s["lo"], s["hi"], tuple(s["props"])) for s in segs], chunk=CHUNK, **cfg)
    for k, (st, w) in enumerate(zip(stats, want)):
        for key in ("passes", "start_cost", "pass_cost", "objective", "best_pass", "final_cost"):
            assert st[key] == w[key], (what, k, key, st[key], w[key])
    assert taken == want_taken, what
    bad = np.nonzero(out != want_out)[0]
    assert not len(bad), (what, [(int(p), out[p], want_out[p]) for p in bad[:5]])
    return want


# ---- 1. the starts

def test_start_cost_is_the_host_s_segment_cost(mixed):
    sa = binding.SA(mixed, neighbours_per_step=64)
    try:
        sa.seed_greedy(16)
        cur = sa.current()[0]
        part = sa.segment_props(GRAIN)["segments"]
        assert len(part) >= 2
        _, segs_out, stats, _, _ = sa.segment_reparse(part, passes=1, chunk=CHUNK)  # the current slab, read where it lies
        assert [st["start_cost"] for st in stats] == [s["cost"] for s in part]
        for s, st in zip(part, stats):
            assert st["start_cost"] == binding.host_segment_cost(mixed, cur, s["lo"], s["hi"], s["props"])[0]
        assert [st["start_cost"] for st in sa.segment_reparse(part, cur, passes=1, chunk=CHUNK)[2]] == [st["start_cost"] for st in stats]
        xz = S.xz_parse(mixed)
        hand = at_starts(xz, [3000, 5500], [(0, 0, 0), (0, 2, 2), (4, 0, 0)])
        for s, st in zip(hand, sa.segment_reparse(hand, xz, passes=1, chunk=CHUNK)[2]):
            assert st["start_cost"] == binding.host_segment_cost(mixed, xz, s["lo"], s["hi"], s["props"])[0], s
    finally:
        sa.close()


# ---- 2. one segment over the whole input is the existing parse

@pytest.mark.parametrize("segment,ahead", [(64, 128), (1000, 0)])
@pytest.mark.parametrize("finder", ["nearest", "frontier"])
def test_one_segment_at_the_handle_s_triple_is_the_adaptive_reparse(mixed, finder, segment, ahead):
    """[0, n) under the handle's own triple: no re-expression, the grid starts at 0, the reset is the LZMA initial state -- every
    pass's exact cost and objective are those of seed_sweep's one variant from the current slab"""
    props = (3, 0, 2)
    sa = binding.SA(mixed, neighbours_per_step=64, lc=props[0], lp=props[1], pb=props[2])
    try:
        sa.seed_greedy(16)
        cur, cost = sa.current()
        sa.set_match_finder(finder)
        _, _, stats, _, _ = sa.segment_reparse([seg(0, len(mixed), props)], passes=3, chunk=CHUNK, segment=segment, ahead=ahead)
        assert sha_slab(sa.current()[0]) == sha_slab(cur)
        res = sa.seed_sweep([(finder, 16, segment, ahead)], passes=3, chunk=CHUNK, from_current=True)["results"][0]
        print(finder, segment, ahead, stats[0]["pass_cost"], res["cost"])
        assert stats[0]["start_cost"] == cost == res["greedy_cost"]
        assert stats[0]["pass_cost"] == res["cost"] and stats[0]["objective"] == res["objective"] and stats[0]["passes"] == res["passes"] == 3
    finally:
        sa.close()


# ---- 3. small inputs against the restatement

def small_input():
    """1 280 B of prose, 1 280 B of records, 512 B of prose again: what wants lc, what wants lp, and copies from far behind"""
    return corpus.prose_like(1280, 0x51) + S.records(1280, 0x51) + corpus.prose_like(1280, 0x51)[:512]


PARITY = {
    # a cut that is no multiple of 512; lc = 4 beside lp = 2, pb = 4
    "two segments": ([1300], [(4, 0, 0), (0, 2, 4)]),
    # a segment shorter than 512 (one chunk, shorter than the grid's step) and one shorter than segment + ahead = 192
    "three segments, short ones": ([1100, 1250], [(3, 0, 0), (0, 2, 2), (2, 1, 3)]),
    "three segments, a short first": ([400, 2600], [(0, 0, 0), (4, 0, 2), (1, 2, 4)]),
}


@pytest.mark.parametrize("source", ["greedy", "xz"])
@pytest.mark.parametrize("case", list(PARITY))
def test_restatement_parity(case, source):
    data = small_input()
    slab = greedy_slab(data) if source == "greedy" else S.xz_parse(data)
    segs = at_starts(slab, *PARITY[case])
    if case != "two segments":
        assert min(s["hi"] - s["lo"] for s in segs) < 192 or segs[0]["hi"] < 512
    got = reparse(data, slab, segs, passes=2)
    check_promises(data, slab, segs, got, f"{case}, {source}")
    check_against_rule(data, slab, segs, got, f"{case}, {source}", passes=2)


# ---- 4. copies cross the cut

def test_copies_reach_below_the_cut():
    half = corpus.prose_like(2048, 0x33)
    data = half + half
    slab = binding.literal_slab(len(data))
    segs = [seg(0, 2048, (0, 0, 0)), seg(2048, 4096, (0, 0, 0))]
    got = reparse(data, slab, segs, passes=1)
    out, _, stats, taken, _ = got
    check_promises(data, slab, segs, got, "doubled prose")
    assert taken and stats[1]["best_pass"] == 0
    crossing = [p for p in S.walk_starts(out)[:-1] if p >= 2048 and int(out[p]["type"]) == MATCH and p - int(out[p]["dist"]) - 1 < 2048]
    assert crossing, "no MATCH of the second segment has its source below the cut"
    # two bits a byte: out of reach for a parse of 2 KiB of prose from a fresh model that sees nothing below 2 048
    assert stats[1]["final_cost"] < 2048 * 16384 // 4, stats[1]
    check_against_rule(data, slab, segs, got, "doubled prose", passes=1)


# ---- 5. the reset's own rep

@pytest.mark.parametrize("source", ["greedy", "xz"])
def test_cuts_inside_zero_runs(source):
    """cuts inside runs coded at distance 1, which is also what a reset leaves in every rep slot: the packets behind a cut lean on
    the reset's own rep, and the joined slab names them against the whole file's stack"""
    data = bytes(4096) + corpus.prose_like(4096, 7) + bytes(4096)
    slab = greedy_slab(data) if source == "greedy" else S.xz_parse(data)
    segs = at_starts(slab, [1000, 10000], [(0, 0, 0), (3, 0, 0), (0, 0, 0)])
    got = reparse(data, slab, segs, passes=1)
    check_promises(data, slab, segs, got, f"zero runs, {source}")
    want = check_against_rule(data, slab, segs, got, f"zero runs, {source}", passes=1)
    for st, w in zip(got[2], want):  # where the join moved a segment's cost off its pass's, the restatement moved it by as much
        if st["best_pass"] is not None:
            assert st["final_cost"] - st["pass_cost"][st["best_pass"]] == w["final_cost"] - w["pass_cost"][w["best_pass"]]


# ---- 6. sixteen segments

def test_sixteen_segments():
    data = corpus.config_input("c5")[0][70_000:70_000 + 8200]
    slab = S.xz_parse(data)
    sa = binding.SA(data, neighbours_per_step=64)
    try:
        cuts = sa.segment_cuts(1, slab)  # leaves of ceil(8200 / 16) = 513 bytes: the most there can be
        assert len(cuts) == 17
        four = [(0, 0, 0), (3, 0, 2), (0, 2, 2), (4, 0, 4)]
        segs = [seg(lo, hi, four[k % 4]) for k, (lo, hi) in enumerate(zip(cuts, cuts[1:]))]
        got = sa.segment_reparse(segs, slab, passes=1, chunk=CHUNK)
    finally:
        sa.close()
    check_promises(data, slab, segs, got, "sixteen segments")
    want = check_against_rule(data, slab, segs, got, "sixteen segments", passes=1)
    for st, w in zip(got[2], want):
        if st["best_pass"] is not None:
            assert st["final_cost"] - st["pass_cost"][st["best_pass"]] == w["final_cost"] - w["pass_cost"][w["best_pass"]]


# ---- 7. gain, 8. guard

def test_gain_on_the_greedy_seed_and_nothing_more_on_its_own_output(mixed):
    sa = binding.SA(mixed, neighbours_per_step=64)
    try:
        sa.seed_greedy(16)
        cur = sa.current()[0]
        part = sa.segment_props(GRAIN)["segments"]
        got = sa.segment_reparse(part, passes=3, chunk=CHUNK)
        check_promises(mixed, cur, part, got, "greedy seed")
        out, segs_out, stats, taken, _ = got
        assert taken and any(st["best_pass"] is not None for st in stats)
        assert sum(st["final_cost"] for st in stats) < sum(st["start_cost"] for st in stats)
        assert lzma.decompress(binding.emit_xz_segments(mixed, mixed, out, segs_out)) == mixed
        # its own output as the input: the strict rule leaves little to gain; whatever comes back is no dearer and valid
        again = sa.segment_reparse(segs_out, out, passes=3, chunk=CHUNK)
        check_promises(mixed, out, segs_out, again, "its own output")
        assert [st["start_cost"] for st in again[2]] == [st["final_cost"] for st in stats]
        if not again[3]:
            assert (again[0] == out).all()
        else:
            assert sum(st["final_cost"] for st in again[2]) < sum(st["final_cost"] for st in stats)
    finally:
        sa.close()


# ---- 9. the search state

@pytest.mark.parametrize("fullwalk", [False, True], ids=["incremental", "fullwalk"])
def test_search_state_is_untouched(mixed, fullwalk):
    """as tests/test_gpu_segments.py has it: a handle that re-parses between two runs ends where one that does not ends"""
    foreign = S.xz_parse(mixed)
    one = binding.SA(mixed, neighbours_per_step=256, fullwalk=fullwalk)
    two = binding.SA(mixed, neighbours_per_step=256, fullwalk=fullwalk)
    try:
        for sa in (one, two):
            sa.seed_greedy(16)
        s1 = one.run(8)
        m1 = one.step_modes()
        two.run(4)
        m2a = two.step_modes()
        state = lambda: (sha_slab(two.current()[0]), two.current()[1], sha_slab(two.best()[0]), two.best()[1],
                         two.neighbours(4, want_diffs=False)[0].tolist(), two.debug_dump(DUMP.ALLOCATIONS).tolist())
        before = state()
        two.segment_reparse(two.segment_props(GRAIN)["segments"], passes=2, chunk=CHUNK)
        two.segment_reparse(two.segment_props(GRAIN, foreign)["segments"], foreign, passes=1, chunk=CHUNK)
        with pytest.raises(binding.MglError):
            two.segment_reparse([seg(0, 5, (0, 0, 0)), seg(6, len(mixed), (0, 0, 0))])
        assert before == state()
        s2 = two.run(4)
        m2 = np.concatenate([m2a, two.step_modes()])
        (c1, cc1), (c2, cc2) = one.current(), two.current()
        assert sha_slab(c1) == sha_slab(c2) and cc1 == cc2
        assert one.best()[1] == two.best()[1] and s1["best_cost"] == s2["best_cost"] and s1["current_cost"] == s2["current_cost"]
        assert m1.tolist() == m2.tolist()
    finally:
        one.close()
        two.close()


# ---- 10. refusals

def _raw(sa, slab, segs, cfg=None, out=True, segs_out=True):
    n = sa.n
    arr = binding._segments(segs)
    res = np.full(n, 0, dtype=PACKET)
    so = (binding.Segment * max(len(segs), 1))()
    return sa.L.mgl_segment_reparse(sa.h, None if slab is None else slab.ctypes.data_as(C.c_void_p), arr, len(segs),
                                    None if cfg is None else C.byref(binding.AdaptiveConfig(*cfg)),
                                    res.ctypes.data_as(C.c_void_p) if out else None, so if segs_out else None, None, None, None)


def test_refusals(mixed):
    n = len(mixed)
    slab = np.ascontiguousarray(S.xz_parse(mixed), dtype=PACKET)
    starts = S.walk_starts(slab)
    on = set(starts)
    a, b = starts[len(starts) // 3], starts[2 * len(starts) // 3]
    off = next(p for p in range(a + 1, n) if p not in on)
    P0 = (0, 0, 0)
    good = [seg(0, a, P0), seg(a, b, (0, 2, 2)), seg(b, n, (4, 0, 0))]
    sa = binding.SA(mixed, neighbours_per_step=64)
    try:
        alloc0 = sa.debug_dump(DUMP.ALLOCATIONS).tolist()
        assert _raw(sa, slab, good, (1, 0, CHUNK, 0, 0, 0)) == 0
        assert _raw(sa, slab, good, None) == 0  # the defaults
        # null arguments
        assert sa.L.mgl_segment_reparse(None, None, None, 0, None, None, None, None, None, None) == MGL_EINVAL
        assert _raw(sa, slab, good, out=False) == MGL_EINVAL and _raw(sa, slab, good, segs_out=False) == MGL_EINVAL
        res = np.zeros(n, dtype=PACKET)
        so = (binding.Segment * 3)()
        assert sa.L.mgl_segment_reparse(sa.h, None, None, 3, None, res.ctypes.data_as(C.c_void_p), so, None, None, None) == MGL_EINVAL
        # the number of segments
        seventeen = [0] + starts[1:17] + [n]
        assert _raw(sa, slab, []) == MGL_EINVAL
        assert _raw(sa, slab, [seg(lo, hi, P0) for lo, hi in zip(seventeen, seventeen[1:])]) == MGL_EINVAL
        # segments that do not tile [0, n) in ascending order
        for bad in ([seg(0, a, P0), seg(b, n, P0)], [seg(0, b, P0), seg(a, n, P0)], [seg(a, n, P0)], [seg(0, a, P0)], [seg(0, n + 1, P0)],
                    [seg(0, a, P0), seg(a, a, P0), seg(a, n, P0)], [seg(a, n, P0), seg(0, a, P0)], [seg(0, 0, P0), seg(0, n, P0)]):
            assert _raw(sa, slab, bad) == MGL_EINVAL, bad
        # an unsupported triple
        for pr in ((5, 0, 0), (3, 2, 0), (0, 5, 0), (0, 0, 5), (4, 1, 4)):
            assert _raw(sa, slab, [seg(0, a, P0), seg(a, n, pr)]) == MGL_EINVAL, pr
        # the settings mgl_sa_seed_adaptive refuses, and from_current
        for cfg in ((17, 0, 0, 0, 0, 0), (1, 31, 0, 0, 0, 0), (1, 0, 511, 0, 0, 0), (1, 0, 0, 64, 274, 0), (1, 0, 0, 0, 0, 1)):
            assert _raw(sa, slab, good, cfg) == MGL_EINVAL, cfg
            with pytest.raises(binding.MglError) as e:
                sa.seed_adaptive(*cfg[:5]) if not cfg[5] else sa.segment_reparse(good, slab, from_current=True)
            assert e.value.rc == MGL_EINVAL
        # a boundary that is no packet start
        assert _raw(sa, slab, [seg(0, off, P0), seg(off, n, P0)]) == MGL_ERANGE
        assert f"boundary {off} " in sa.L.mgl_last_error().decode()
        assert _raw(sa, slab, [seg(0, a, P0), seg(a, off, P0), seg(off, n, P0)]) == MGL_ERANGE
        # an invalid slab
        type0 = slab.copy()
        type0[starts[3]]["type"] = 0
        off_end = binding.literal_slab(n)
        off_end[n - 1] = (MATCH, 0, 5)
        for bad in (type0, off_end):
            assert _raw(sa, bad, good) == MGL_ERANGE
        # the call's buffers died with it; the handle works
        assert sa.debug_dump(DUMP.ALLOCATIONS).tolist() == alloc0
        sa.seed_greedy(16)
        assert sa.run(2)["steps"] == 2
        cur, cost = sa.current()
        assert sa.cost_slab(cur, want_cum=False)["total"] == cost
    finally:
        sa.close()


# ---- 11. the CLI

def test_cli_end_to_end(mixed, tmp_path):
    f = tmp_path / "in.bin"
    f.write_bytes(mixed)
    r = subprocess.run([build.CLI, "--format", "xz", "--adaptive-seed", "1", "--segment-props", str(GRAIN), "--segment-reparse", "2", "--epochs", "1",
                        "--phases", "1", str(f)], capture_output=True, timeout=600)
    err = r.stderr.decode()
    assert r.returncode == 0, err[-800:]
    assert lzma.decompress(r.stdout) == mixed
    props = re.findall(r"^segment-props: .* segmented ([\d.]+) B exact (\d+) segments (\d+) [\d.]+ ms$", err, re.M)
    head = re.findall(r"^segment-reparse: passes (\d+) segments (\d+) reparsed (\d+) taken ([01]) was ([\d.]+) B exact (\d+) now ([\d.]+) B exact (\d+) "
                      r"[\d.]+ ms$", err, re.M)
    rows = re.findall(r"^segment-parse: offset (\d+) bytes (\d+) lc=(\d) lp=(\d) pb=(\d) start ([\d.]+) B exact (\d+) best ([\d.]+) B exact (\d+) "
                      r"pass (\d+|-) final ([\d.]+) B exact (\d+)$", err, re.M)
    assert len(props) == 1 and len(head) == 1, err[-1200:]
    passes, nseg, reparsed, taken, was_b, was, now_b, now = head[0]
    print(head[0], rows)
    assert (int(passes), int(nseg)) == (2, int(props[0][2])) and len(rows) == int(nseg)
    assert int(was) == int(props[0][1]) and was_b == props[0][0]
    assert int(now) <= int(was) and now_b == f"{int(now) / 16384:.3f}"
    over = (len(rows) - 1) * binding.SEG_OVERHEAD
    assert sum(int(row[6]) for row in rows) + over == int(was) and sum(int(row[11]) for row in rows) + over == int(now)
    assert int(reparsed) == sum(row[9] != "-" for row in rows) and (int(taken) == 1) == (int(now) < int(was))
    assert all(int(row[8]) <= int(row[6]) and (row[9] == "-") == (int(row[8]) == int(row[6]) or not int(taken)) for row in rows)
    assert [int(row[0]) for row in rows] == [0] + [int(row[0]) + int(row[1]) for row in rows[:-1]] and int(rows[-1][0]) + int(rows[-1][1]) == len(mixed)
    # without the option: the same run and no such line
    r0 = subprocess.run([build.CLI, "--format", "xz", "--adaptive-seed", "1", "--segment-props", str(GRAIN), "--epochs", "1", "--phases", "1", str(f)],
                        capture_output=True, timeout=600)
    assert r0.returncode == 0 and lzma.decompress(r0.stdout) == mixed and b"segment-reparse:" not in r0.stderr and b"segment-parse:" not in r0.stderr
