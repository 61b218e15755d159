"""Segment props restated in Python integers (include/megalania_hip.h, "Segment props"): the
re-expression of a segment's packets against the rep stack that starts at its cut, the span index, the grain rule and the
partition DP.  A segment's cost is left to the host function (mgl_host_segment_cost), which the device is compared with.
Test infrastructure only; shared by the CPU and the GPU tests, which also take their common inputs from here."""
from __future__ import annotations

import lzma

import numpy as np

from _libs import LITERAL, LONG_REP, MATCH, PACKET, SHORT_REP
from megalania_amd import binding, corpus

NTRIPLES = len(binding.PROPS_TRIPLES)
MAX_LEAVES = 16
EXTREME = 9 | lzma.PRESET_EXTREME


def advance_reps(reps, typ, dist):
    """mgl_advance's effect on the four rep distances"""
    if typ == MATCH:
        return [dist] + reps[:3]
    if typ == LONG_REP:
        return [reps[dist]] + reps[:dist] + reps[dist + 1:]
    return reps


def walk_starts(slab):
    """the packet starts of the walk, and n"""
    out, pos, lens = [], 0, slab["len"]
    while pos < len(slab):
        out.append(pos)
        pos += int(lens[pos])
    assert pos == len(slab)
    return out + [pos]


def reexpress(slab, lo, hi):
    """[(type, dist, len)] of the packets that start in [lo, hi), as a coder codes them that starts at lo with rep distances
    (0, 0, 0, 0); and how many of them differ from the slab's.  lo and hi must be packet starts."""
    t, pos = [0, 0, 0, 0], 0
    while pos < lo:
        e = slab[pos]
        t = advance_reps(t, int(e["type"]), int(e["dist"]))
        pos += int(e["len"])
    assert pos == lo, (pos, lo)
    r, out, changed = [0, 0, 0, 0], [], 0
    while pos < hi:
        typ, dist, ln = (int(slab[pos][k]) for k in ("type", "dist", "len"))
        q = (typ, dist, ln)
        if typ == SHORT_REP:
            if r[0] != t[0]:
                q = (LITERAL, dist, ln)
        elif typ == LONG_REP:
            d = t[dist]
            if r[dist] != d:
                q = (LONG_REP, r.index(d), ln) if d in r else (MATCH, d, ln)
        changed += q != (typ, dist, ln)
        out.append(q)
        t = advance_reps(t, typ, dist)
        r = advance_reps(r, q[0], q[1])
        pos += ln
    assert pos == hi, (pos, hi)
    return out, changed


def span_index(i, j, m):
    return i * m - i * (i - 1) // 2 + (j - i - 1)


def grain_cuts(slab, grain):
    """c_0 = 0 < .. < c_m = n: the multiples of max(grain, ceil(n / 16)) below n, each moved to the first packet start at or
    above it; those that meet there, or at n, count once.  grain 0 = 65536."""
    n = len(slab)
    step = max(grain or 65536, -(-n // MAX_LEAVES))
    starts = walk_starts(slab)
    cuts = [0]
    for cand in range(step, n, step):
        s = next(p for p in starts if p >= cand)
        if s < n and s != cuts[-1]:
            cuts.append(s)
    return cuts + [n]


def partition(cost, cuts, overhead):
    """(segments [(lo, hi, triple index, cost)], total) of the DP: best[j] = min over i < j of best[i] + min_T cost[s(i, j)][T]
    + (overhead if i > 0), ties to the lowest i and to the lowest triple."""
    m = len(cuts) - 1
    best, back = [0] + [None] * m, [None] * (m + 1)
    for j in range(1, m + 1):
        for i in range(j):
            row = [int(c) for c in cost[span_index(i, j, m)]]
            t = row.index(min(row))
            v = best[i] + row[t] + (overhead if i else 0)
            if best[j] is None or v < best[j]:
                best[j], back[j] = v, (i, t, row[t])
    segs, j = [], m
    while j:
        i, t, c = back[j]
        segs.append((cuts[i], cuts[j], t, c))
        j = i
    return segs[::-1], best[m]


def as_tuples(segments):
    """binding's segment dicts in partition()'s form"""
    return [(s["lo"], s["hi"], binding.PROPS_TRIPLES.index(tuple(s["props"])), s["cost"]) for s in segments]


def slab_of(packets, n):
    """lay walked packets [(type, dist, len)] down from byte 0; entries off the walk stay literals"""
    s = np.zeros(n, dtype=PACKET)
    s["type"], s["len"] = LITERAL, 1
    pos = 0
    for typ, dist, ln in packets:
        s[pos] = (typ, dist, ln)
        pos += ln
    assert pos == n, (pos, n)
    return s


def records(n_bytes, seed):
    """seeded 4-byte records: byte 0 uniform, byte 1 one of four values, byte 2 one of two (90/10), byte 3 0 or 0x80 (95/5):
    the kind of table that wants lp = 2 where prose wants lc = 3"""
    k = n_bytes // 4
    u = corpus._stream(seed, 61, 0, 4 * k).reshape(4, k) >> np.uint64(11)
    rec = np.zeros((k, 4), dtype=np.uint8)
    rec[:, 0] = (u[0] & np.uint64(0xFF)).astype(np.uint8)
    rec[:, 1] = np.array([0x10, 0x11, 0x40, 0x7F], dtype=np.uint8)[(u[1] % np.uint64(4)).astype(np.int64)]
    rec[:, 2] = np.where(u[2] % np.uint64(10) == 0, 0x3C, 0x02).astype(np.uint8)
    rec[:, 3] = np.where(u[3] % np.uint64(20) == 0, 0x80, 0x00).astype(np.uint8)
    return rec.tobytes()


def mixed_input(seed=0x51):
    """4 096 B of prose followed by 4 096 B of records: two halves that want different triples"""
    return corpus.prose_like(4096, seed) + records(4096, seed)


def xz_parse(data, lc=0, lp=0, pb=0):
    """the parse inside the standard library's -9e LZMA-alone stream of `data`, as a slab"""
    stream = lzma.compress(data, format=lzma.FORMAT_ALONE,
                           filters=[dict(id=lzma.FILTER_LZMA1, preset=EXTREME, dict_size=1 << 22, lc=lc, lp=lp, pb=pb)])
    return binding.stream_import(stream, data)[0]


def host_table(data, slab, cuts):
    """the table of SA.props_sweep_spans from the host function: every span, every triple"""
    m = len(cuts) - 1
    tab = np.zeros((m * (m + 1) // 2, NTRIPLES), dtype=np.uint64)
    for i in range(m):
        for j in range(i + 1, m + 1):
            for t, pr in enumerate(binding.PROPS_TRIPLES):
                tab[span_index(i, j, m), t] = binding.host_segment_cost(data, slab, cuts[i], cuts[j], pr)[0]
    return tab


def lzma2_chunks(stream):
    """[(control, props byte or None, usize, csize)] of the first block of an .xz stream"""
    at = 12
    at += (stream[at] + 1) * 4
    out = []
    while stream[at] != 0:
        c = stream[at]
        assert c >= 0x80, hex(c)
        usize = ((c & 0x1F) << 16 | stream[at + 1] << 8 | stream[at + 2]) + 1
        csize = (stream[at + 3] << 8 | stream[at + 4]) + 1
        at += 5
        props = None
        if c >= 0xC0:
            props = stream[at]
            at += 1
        out.append((c & 0xE0, props, usize, csize))
        at += csize
    return out


def props_byte(props):
    lc, lp, pb = props
    return (pb * 5 + lp) * 9 + lc
