"""Segment props without a device: the host's re-expression and segment cost against the Python
restatement in tests/_segments.py, on planted slabs whose rep stacks are known and on the standard library's -9e parses;
the partition DP and the grain rule of the C ABI against theirs."""
import numpy as np
import pytest

import _segments as S
from _libs import LITERAL, LONG_REP, MATCH, SHORT_REP
from _planted_parse import periodic_input
from megalania_amd import binding, build, corpus

MGL_EINVAL = -1


@pytest.fixture(scope="module", autouse=True)
def built():
    build.build_hip()
    build.build_host()


@pytest.fixture(scope="module")
def mixed():
    data = S.mixed_input()
    return data, S.xz_parse(data)


def tuples(packets):
    return [(int(p["type"]), int(p["dist"]), int(p["len"])) for p in packets]


def check_every_cut(data, slab, los=None):
    """host re-expression == restatement for the segments [lo, n) and [lo, next start .. ) of every given packet start"""
    n = len(data)
    starts = S.walk_starts(slab)
    for lo in starts[:-1] if los is None else los:
        want, changed = S.reexpress(slab, lo, n)
        assert tuples(binding.host_segment_packets(data, slab, lo, n)) == want, lo
        assert binding.host_segment_cost(data, slab, lo, n)[1] == changed, lo
    return starts


# ---- planted slabs: an input of period D, on which a copy at any whole number of periods is valid, so that the four rep slots
# can be given four different distances.  d(k) = k D - 1 is the distance field of a copy k periods back.

D = 7


def d(k):
    return k * D - 1


def planted(tail, n_extra=0):
    """5 D literals, MATCH 1, 2, 3 and 4 periods back (true stack (d4, d3, d2, d1)), then `tail`"""
    head = [(LITERAL, 0, 1)] * (5 * D) + [(MATCH, d(k), 3) for k in (1, 2, 3, 4)]
    packets = head + tail
    n = sum(p[2] for p in packets) + n_extra
    packets += [(LITERAL, 0, 1)] * n_extra
    data = periodic_input(n, D, 0x5E6)
    return data, S.slab_of(packets, n), 5 * D + 12  # the first packet of the tail


def test_cut_on_a_short_rep_makes_it_a_literal():
    data, slab, at = planted([(SHORT_REP, 0, 1), (LITERAL, 0, 1), (LONG_REP, 0, 4), (SHORT_REP, 0, 1), (LONG_REP, 0, 2)])
    got = tuples(binding.host_segment_packets(data, slab, at, len(data)))
    # r[0] = 0 is not d4: a literal; the LONG_REP 0 behind it finds d4 in no slot: a MATCH; from there r[0] = d4 as in the slab
    assert got == [(LITERAL, 0, 1), (LITERAL, 0, 1), (MATCH, d(4), 4), (SHORT_REP, 0, 1), (LONG_REP, 0, 2)]
    assert binding.host_segment_cost(data, slab, at, len(data))[1] == 2
    check_every_cut(data, slab)


@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_cut_on_a_long_rep_of_every_index(idx):
    other = (idx + 1) % 4
    data, slab, at = planted([(LONG_REP, idx, 5), (LONG_REP, 0, 2), (LONG_REP, other, 3), (LITERAL, 0, 1), (LONG_REP, 1, 2)], n_extra=3)
    true = [d(4), d(3), d(2), d(1)]
    got = tuples(binding.host_segment_packets(data, slab, at, len(data)))
    assert got[0] == (MATCH, true[idx], 5)           # in no slot of (0, 0, 0, 0)
    assert got[1] == (LONG_REP, 0, 2)                # the same distance again: kept
    assert got == S.reexpress(slab, at, len(data))[0]
    check_every_cut(data, slab)


def test_long_rep_moves_to_the_slot_that_holds_its_distance():
    # behind the cut: MATCH d5 (r = (d5, 0, 0, 0), t = (d5, d4, d3, d2)); LONG_REP 1 is d4, in no slot: MATCH (r = (d4, d5, 0, 0),
    # t = (d4, d5, d3, d2)); LONG_REP 1 is d5, r[1] too: kept; LONG_REP 2 is d3: MATCH; then t = (d3, d5, d4, d2), r = (d3, d5, d4, 0):
    # LONG_REP 3 is d2, in no slot: MATCH, and r == t
    data, slab, at = planted([(MATCH, d(5), 2), (LONG_REP, 1, 2), (LONG_REP, 1, 3), (LONG_REP, 2, 2), (LONG_REP, 3, 2), (LONG_REP, 3, 2),
                              (SHORT_REP, 0, 1)])
    got = tuples(binding.host_segment_packets(data, slab, at, len(data)))
    assert got == [(MATCH, d(5), 2), (MATCH, d(4), 2), (LONG_REP, 1, 3), (MATCH, d(3), 2), (MATCH, d(2), 2), (LONG_REP, 3, 2), (SHORT_REP, 0, 1)]
    assert got == S.reexpress(slab, at, len(data))[0]
    # a rep whose distance sits in another slot of r than of t: cut behind MATCH d5, LONG_REP 1 (t = (d4, d5, d3, d2)); MATCH d3 gives
    # r = (d3, 0, 0, 0), t = (d3, d4, d5, d2) -- LONG_REP 2 (d5): MATCH, r = (d5, d3, 0, 0), t = (d5, d3, d4, d2); LONG_REP 1 stays
    data, slab, at = planted([(MATCH, d(5), 2), (LONG_REP, 1, 2), (MATCH, d(3), 2), (LONG_REP, 2, 2), (LONG_REP, 2, 2), (LONG_REP, 1, 2)])
    cut = at + 4
    got = tuples(binding.host_segment_packets(data, slab, cut, len(data)))
    # t = (d5, d3, d4, d2), r = (d5, d3, 0, 0): LONG_REP 2 is d4: MATCH; then t = r in the first three slots, LONG_REP 1 is d5: kept
    assert got == [(MATCH, d(3), 2), (MATCH, d(5), 2), (MATCH, d(4), 2), (LONG_REP, 1, 2)]
    assert got == S.reexpress(slab, cut, len(data))[0]
    # and one that changes its index: t = (a, b, ..), r = (b, 0, 0, 0) -> LONG_REP 1 becomes LONG_REP 0
    data, slab, at = planted([(LONG_REP, 1, 2), (LONG_REP, 1, 2), (LONG_REP, 1, 2)])
    cut = at + 2  # t = (d3, d4, d2, d1) here; LONG_REP 1 is d4: MATCH, r = (d4, 0, 0, 0), t = (d4, d3, d2, d1); LONG_REP 1 is d3: MATCH
    got = tuples(binding.host_segment_packets(data, slab, cut, len(data)))
    assert got == [(MATCH, d(4), 2), (MATCH, d(3), 2)]
    data, slab, at = planted([(LONG_REP, 1, 2), (MATCH, d(4), 2), (LONG_REP, 2, 2), (LONG_REP, 1, 2)])
    cut = at + 2  # t = (d3, d4, d2, d1): MATCH d4 -> t = (d4, d3, d4, d2), r = (d4, 0, 0, 0); LONG_REP 2 is d4, r[2] is not: slot 0 holds it
    got = tuples(binding.host_segment_packets(data, slab, cut, len(data)))
    assert got[:2] == [(MATCH, d(4), 2), (LONG_REP, 0, 2)]
    assert got == S.reexpress(slab, cut, len(data))[0]
    check_every_cut(data, slab)


def test_zero_run_cut_on_a_long_rep_0_stays_a_rep():
    n, k = 40, 6
    packets = [(LITERAL, 0, 1), (MATCH, 0, 3)] + [(LONG_REP, 0, 6)] * k
    data = bytes(n)
    slab = S.slab_of(packets, n)
    for cut in range(4, n, 6):  # t[0] = 0 = r[0]: the state reset's distances are the run's
        got = tuples(binding.host_segment_packets(data, slab, cut, n))
        assert got == [(LONG_REP, 0, 6)] * ((n - cut) // 6)
        assert binding.host_segment_cost(data, slab, cut, n)[1] == 0
    check_every_cut(data, slab)


def test_unknown_distance_becomes_a_match_and_the_rep_behind_it_is_kept():
    data, slab, at = planted([(LITERAL, 0, 1), (LONG_REP, 2, 4), (LONG_REP, 0, 2), (LITERAL, 0, 1), (LONG_REP, 0, 3)])
    got = tuples(binding.host_segment_packets(data, slab, at, len(data)))
    assert got == [(LITERAL, 0, 1), (MATCH, d(2), 4), (LONG_REP, 0, 2), (LITERAL, 0, 1), (LONG_REP, 0, 3)]
    assert binding.host_segment_cost(data, slab, at, len(data))[1] == 1
    check_every_cut(data, slab)


def test_stacks_agree_after_four_distinct_matches():
    tail = [(MATCH, d(k), 2) for k in (5, 1, 3, 2)] + [(LONG_REP, 3, 2), (LONG_REP, 2, 3), (SHORT_REP, 0, 1), (LONG_REP, 1, 2), (LONG_REP, 3, 4)]
    data, slab, at = planted(tail)
    got = tuples(binding.host_segment_packets(data, slab, at, len(data)))
    assert got == tail and binding.host_segment_cost(data, slab, at, len(data))[1] == 0
    # one match short of four: slot 3 still differs
    cut = at + 2
    got = tuples(binding.host_segment_packets(data, slab, cut, len(data)))
    assert got[:4] == tail[1:4] + [(MATCH, d(5), 2)] and got[4:] == tail[5:]
    check_every_cut(data, slab)


def test_planted_segment_from_byte_0_is_the_plain_cost():
    data, slab, at = planted([(LONG_REP, 1, 5), (SHORT_REP, 0, 1), (LONG_REP, 3, 2)])
    n = len(data)
    for pr in [(0, 0, 0), (3, 0, 2), (0, 2, 2), (1, 3, 4)]:
        assert binding.host_segment_cost(data, slab, 0, n, pr) == (binding.host_cost_map(data, slab, pr)[1]["total"], 0)
        assert binding.host_segment_cost(data, slab, at, at, pr) == (0, 0)
    # a segment of literals only costs what the same literals cost at the head of a file that starts alike: 9 events each from
    # a fresh model, whatever came before the cut (lc = 0: no previous byte; pb = lp = 0: no position)
    head = binding.host_segment_cost(data, slab, 0, D, (0, 0, 0))[0]
    lits = S.slab_of([(LITERAL, 0, 1)] * n, n)
    assert binding.host_segment_cost(data, lits, 3 * D, 4 * D, (0, 0, 0))[0] == head


# ---- parses of the standard library's encoder


def test_whole_file_segment_is_the_cost_map_total_under_all_75_triples(mixed):
    data, slab = mixed
    for pr in binding.PROPS_TRIPLES:
        cost, changed = binding.host_segment_cost(data, slab, 0, len(data), pr)
        assert changed == 0 and cost == binding.host_cost_map(data, slab, pr)[1]["total"], pr


@pytest.mark.parametrize("name", ["mixed", "lorem", "zeros"])
def test_reexpression_on_encoder_parses(name, mixed):
    data, slab = mixed if name == "mixed" else (lambda x: (x, S.xz_parse(x)))(corpus.lorem(4096) if name == "lorem" else bytes(4096))
    starts = S.walk_starts(slab)
    step = max(1, len(starts) // 40)
    check_every_cut(data, slab, starts[:-1][::step])
    lo, hi = starts[len(starts) // 3], starts[2 * len(starts) // 3]
    assert tuples(binding.host_segment_packets(data, slab, lo, hi)) == S.reexpress(slab, lo, hi)[0]


def test_refusals(mixed):
    data, slab = mixed
    n = len(data)
    starts = S.walk_starts(slab)
    off = next(p for p in range(1, n) if p not in set(starts))
    for lo, hi, pr in [(off, n, (0, 0, 0)), (0, off, (0, 0, 0)), (0, n, (3, 2, 0)), (0, n, (0, 0, 5)), (starts[5], starts[4], (0, 0, 0)),
                       (0, n + 1, (0, 0, 0))]:
        with pytest.raises(binding.MglError) as e:
            binding.host_segment_cost(data, slab, lo, hi, pr)
        assert e.value.rc == MGL_EINVAL, (lo, hi, pr)
    bad = slab.copy()
    bad[starts[7]] = (MATCH, 0x300000, 5)
    with pytest.raises(binding.MglError) as e:
        binding.host_segment_cost(data, bad, 0, n)
    assert e.value.rc == MGL_EINVAL


# ---- partition and grain rule (C ABI, host arithmetic)


def random_table(m, seed, spread):
    u = corpus._stream(seed, 71, 0, m * (m + 1) // 2 * S.NTRIPLES) >> np.uint64(11)
    return (u % np.uint64(spread)).astype(np.uint64).reshape(-1, S.NTRIPLES) + np.uint64(1)


@pytest.mark.parametrize("m", [1, 2, 3, 7, 16])
@pytest.mark.parametrize("spread", [2, 5, 1 << 24])  # the small ones make ties among spans and among triples
def test_partition_matches_the_python_dp(m, spread):
    cuts = [0] + sorted(100 * (k + 1) + k * k for k in range(m))
    for seed in range(6):
        tab = random_table(m, 1000 * m + seed, spread)
        for overhead in (0, 1, binding.SEG_OVERHEAD, 1 << 60):
            want, total = S.partition(tab, cuts, overhead)
            segs, got = binding.segment_partition(tab, cuts, overhead)
            assert (S.as_tuples(segs), got) == (want, total), (m, seed, overhead)
            assert [s["lo"] for s in segs] == [0] + [s["hi"] for s in segs[:-1]] and segs[-1]["hi"] == cuts[-1]
            assert got == sum(s["cost"] for s in segs) + (len(segs) - 1) * overhead
            assert got <= int(tab[S.span_index(0, m, m)].min())  # never dearer than one triple
            if overhead == 1 << 60:
                assert len(segs) == 1
            if overhead == 0 and spread == 2:
                assert got <= m * 2


def test_partition_ties_go_to_the_lowest_cut_and_triple():
    m = 3
    tab = np.full((6, S.NTRIPLES), 10, dtype=np.uint64)
    segs, total = binding.segment_partition(tab, [0, 10, 20, 30], 0)
    assert S.as_tuples(segs) == [(0, 30, 0, 10)] and total == 10  # i = 0 comes first and nothing is strictly smaller
    tab[S.span_index(0, m, m)] = 40  # now three leaves at 10 each (30) tie with (0,1)+(1,3) and (0,2)+(2,3) at 20: lowest i wins
    segs, total = binding.segment_partition(tab, [0, 10, 20, 30], 0)
    assert total == 20 and S.as_tuples(segs) == S.partition(tab, [0, 10, 20, 30], 0)[0] == [(0, 10, 0, 10), (10, 30, 0, 10)]
    tab[S.span_index(1, 3, m), :7] = 11
    assert S.as_tuples(binding.segment_partition(tab, [0, 10, 20, 30], 0)[0])[1] == (10, 30, 7, 10)
    with pytest.raises(binding.MglError):
        binding.segment_partition(tab, [0], 0)


def test_span_index_is_dense_and_in_order():
    for m in range(1, 17):
        idx = [S.span_index(i, j, m) for i in range(m) for j in range(i + 1, m + 1)]
        assert idx == list(range(m * (m + 1) // 2)) and idx == [binding.span_index(i, j, m) for i in range(m) for j in range(i + 1, m + 1)]


def test_grain_rule_restated(mixed):
    """the rule itself (the C ABI's mgl_segment_cuts needs a handle and is compared with this on the device)"""
    data, slab = mixed
    n = len(data)
    starts = set(S.walk_starts(slab))
    for grain in (1, 100, 1024, 4096, 5000):
        cuts = S.grain_cuts(slab, grain)
        step = max(grain, n // 16)
        assert cuts[0] == 0 and cuts[-1] == n and cuts == sorted(set(cuts)) and set(cuts) <= starts
        assert len(cuts) - 1 <= 16 and len(cuts) - 1 <= -(-n // step)          # capped at 16 leaves
        assert all(0 <= c - k * step < 273 for k, c in enumerate(cuts[:-1]))  # each at the first start at or above its candidate
    assert S.grain_cuts(slab, n) == S.grain_cuts(slab, n + 1) == S.grain_cuts(slab, 0) == [0, n]  # n < grain: one leaf
    # candidates that meet at one packet start collapse: a parse with one packet of 273 bytes over several candidates
    z = bytes(600)
    zs = S.slab_of([(LITERAL, 0, 1), (MATCH, 0, 273), (LONG_REP, 0, 273), (LONG_REP, 0, 53)], 600)
    assert S.grain_cuts(zs, 60) == [0, 274, 547, 600] and len(z) == 600
    assert S.grain_cuts(zs, 580) == [0, 600]  # the only candidate snaps to n
