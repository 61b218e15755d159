"""A seeded generator of valid parses that no search or parser of this project would make: every packet type at every
length the input allows, in whatever walk state they happen to meet, with stale (off-walk) entries of every type under
the packets.  Test infrastructure only.

Stale entries are program state: the repair of a neighbour reads whatever sits at a position that a shortened match
uncovers (packet_slab_neighbour.c:82-117), takes a stale MATCH as it is and re-validates a stale LONG_REP against the rep
distances of the moment.  What goes off the walk here is what the reference's own slab could hold there -- a MATCH that
reproduces the input at its position, a LONG_REP of any index with a length that stays inside the input, a SHORT_REP, a
literal -- never a corrupt entry.

Draws come from the project's counter RNG (corpus._stream), so a (data, seed, settings) names one slab on every Python."""
from __future__ import annotations

import bisect
import functools

import numpy as np

from _libs import LITERAL, LONG_REP, MATCH, PACKET, SHORT_REP, walk
from megalania_amd import corpus

MAX_LEN = 273
_LANE = 29


class _Draws:
    """u64 draws number 0, 1, 2, ... of corpus._stream(seed, _LANE)"""

    def __init__(self, seed: int):
        self.seed, self.start, self.buf, self.k = seed, 0, [], 0

    def next(self) -> int:
        if self.k == len(self.buf):
            self.buf = [int(x) for x in corpus._stream(self.seed, _LANE, self.start, 4096)]
            self.start += 4096
            self.k = 0
        self.k += 1
        return self.buf[self.k - 1]

    def below(self, n: int) -> int:
        return (self.next() >> 11) % n

    def weighted(self, weights) -> int:
        """index drawn in proportion to weights (some of them may be 0, not all)"""
        u = (self.next() >> 11) * (1.0 / (1 << 53)) * float(sum(weights))
        acc = 0.0
        for i, w in enumerate(weights):
            acc += w
            if w > 0 and u < acc:
                return i
        return max(i for i, w in enumerate(weights) if w > 0)


def _common(data: bytes, a: int, b: int, cap: int) -> int:
    """bytes that data[a:] and data[b:] share, at most cap (a < b; the ranges may overlap)"""
    k = 0
    while k < cap and data[a + k] == data[b + k]:
        k += 1
    return k


class _Bigrams:
    """earlier occurrences of a position's leading bigram inside the dictionary window"""

    def __init__(self, data: bytes, dict_limit: int):
        self.data, self.limit, self.at = data, dict_limit, {}
        for p in range(len(data) - 1):
            self.at.setdefault(data[p:p + 2], []).append(p)

    def source(self, rng: _Draws, pos: int):
        """one source for a MATCH at pos -- the nearest, the farthest or a uniform one -- or None"""
        if pos + 1 >= len(self.data):
            return None
        lst = self.at[self.data[pos:pos + 2]]
        hi = bisect.bisect_left(lst, pos)
        lo = bisect.bisect_left(lst, pos - self.limit)  # pos - q - 1 < limit
        if lo >= hi:
            return None
        how = rng.below(3)
        return lst[hi - 1] if how == 0 else lst[lo] if how == 1 else lst[lo + rng.below(hi - lo)]


def _length(rng: _Draws, longest: int, len_mode: str) -> int:
    if len_mode == "short":
        return 2 + rng.below(min(longest, 4) - 1)
    assert len_mode == "any", len_mode
    how = rng.below(3)
    return 2 if how == 0 else longest if how == 1 else 2 + rng.below(longest - 1)


def random_parse(data: bytes, seed: int, weights, len_mode: str, stale: bool = True, dict_limit: int = 0x400000) -> np.ndarray:
    """weights: literal / MATCH / SHORT_REP / LONG_REP, among the types that have a candidate at a position.
    len_mode: "any" draws a length from {2, the longest, uniform in between}, "short" uniform in 2..min(longest, 4)."""
    data = bytes(data)
    n = len(data)
    rng = _Draws(seed)
    big = _Bigrams(data, dict_limit)
    slab = np.zeros(n, dtype=PACKET)
    slab["type"], slab["len"] = LITERAL, 1
    wl, wm, ws, wr = weights
    reps = [0, 0, 0, 0]
    pos = 0
    while pos < n:
        room = min(MAX_LEN, n - pos)
        short = pos > 0 and data[pos] == data[pos - reps[0] - 1]
        longs = []
        if room >= 2:
            for k in range(4):
                if pos - reps[k] - 1 >= 0:
                    m = _common(data, pos - reps[k] - 1, pos, room)
                    if m >= 2:
                        longs.append((k, m))
        src = big.source(rng, pos) if pos > 0 else None
        kind = rng.weighted([wl, wm if src is not None else 0, ws if short else 0, wr if longs else 0])
        if kind == 0:
            pk = (LITERAL, 0, 1)
        elif kind == 1:
            pk = (MATCH, pos - src - 1, _length(rng, _common(data, src, pos, room), len_mode))
            reps = [pk[1]] + reps[:3]
        elif kind == 2:
            pk = (SHORT_REP, 0, 1)
        else:
            k, m = longs[rng.below(len(longs))]
            pk = (LONG_REP, k, _length(rng, m, len_mode))
            reps = [reps[k]] + reps[:k] + reps[k + 1:]
        slab[pos] = pk
        if stale:
            for p in range(pos + 1, pos + pk[2]):
                slab[p] = _stale_entry(rng, big, data, p, len_mode)
        pos += pk[2]
    return slab


def _stale_entry(rng: _Draws, big: _Bigrams, data: bytes, p: int, len_mode: str):
    """what may lie at the off-walk position p: valid there whatever the walk state turns out to be when it is uncovered"""
    room = min(MAX_LEN, len(data) - p)
    kind = rng.below(4)
    if kind == 0 and room >= 2:
        src = big.source(rng, p)
        if src is not None:
            return (MATCH, p - src - 1, _length(rng, _common(data, src, p, room), len_mode))
    if kind == 1 and room >= 2:
        return (LONG_REP, rng.below(4), 2 + rng.below(room - 1))
    if kind == 2:
        return (SHORT_REP, 0, 1)
    return (LITERAL, 0, 1)


def on_walk(slab) -> np.ndarray:
    on = np.zeros(len(slab), dtype=bool)
    on[walk(slab)] = True
    return on


def doubled_letters(seed: int, n: int) -> bytes:
    from test_oracle_golden import doubled_letters as f
    return f(seed, n)


def two_periods(times: int = 8) -> bytes:
    """a 7-byte and an 11-byte word over `abcd`, each repeated: two periods that take turns"""
    w7, w11 = b"abcdbcd", b"cbabdacbdcb"
    return (w7 * 40 + w11 * 30) * times


TEXT, REPS, MATCHES = (3, 3, 2, 3), (2, 0.2, 6, 6), (1, 3, 1, 1)
# name: (data, weights, len_mode, seed, dict_limit)
_SPECS = {
    "enwik4k": (lambda: corpus.enwik_like(4000, 0x42), TEXT, "any", 11, 0x400000),
    "lorem3k": (lambda: corpus.lorem(3000), TEXT, "any", 12, 0x400000),
    "doubled": (lambda: doubled_letters(1, 2600), REPS, "any", 13, 0x400000),
    "two_periods": (two_periods, REPS, "short", 14, 0x400000),
    "edge": (lambda: corpus.enwik_like(4000, 0x42)[:1025], MATCHES, "short", 15, 0x400000),
    "enwik4k_matches": (lambda: corpus.enwik_like(4000, 0x42), MATCHES, "any", 16, 0x400000),
    # every MATCH source within 300 bytes, on and off the walk: for handles and oracles made with dict_limit=300
    "enwik4k_dict300": (lambda: corpus.enwik_like(4000, 0x42), TEXT, "any", 17, 300),
    # one period only: every rep distance fits everywhere, so a move that reorders the rep distances changes no packet behind it
    # and its walk never meets the base's again -- the walk-length rule (and, through the matches, the event lists)
    "one_period": (lambda: b"abcdbcd" * 697, (2, 0.005, 10, 3), "short", 32, 0x400000),
    # sources more than 8 192 bytes back (8 direct bits and more) need a longer input than the others: walk tests only
    "far9k": (lambda: corpus.enwik_like(9500, 0x43), MATCHES, "any", 18, 0x400000),
}
BASES = ["enwik4k", "lorem3k", "doubled", "two_periods", "edge", "enwik4k_matches", "one_period"]
ALT_PROPS = dict(lc=2, lp=1, pb=2)
# the neighbours that the CPU and the GPU tests look at: steps 0 and 5 of K neighbours under this search seed
K, SEED, STEPS = 128, 99, (0, 5)


@functools.lru_cache(maxsize=None)
def _base(name: str):
    make, weights, len_mode, seed, dict_limit = _SPECS[name]
    data = make()
    slab = random_parse(data, seed, weights, len_mode, dict_limit=dict_limit)
    slab.setflags(write=False)
    return data, slab


def base(name: str):
    """(data, slab) of a named base; the slab is shared and read-only, so take a copy before handing it to anything that
    writes (the oracle's neighbour generator does, and undoes it)"""
    return _base(name)


def dict_limit_of(name: str) -> int:
    return _SPECS[name][4]


@functools.lru_cache(maxsize=None)
def oracle_neighbours(name: str, step: int, alt_props: bool = False):
    """per neighbour j of `step` from the named base: (status, cost, journal, window, drop reason) of the oracle"""
    from _libs import Oracle
    data, slab = base(name)
    o = Oracle(data, dict_limit=dict_limit_of(name), **(ALT_PROPS if alt_props else {}))
    work = slab.copy()
    out = [o.neighbour_ex(work, SEED, step, j, K=K, reason=True) for j in range(K)]
    assert (work == slab).all()
    return out


def drop_counts(rows) -> dict:
    """dropped neighbours per rule (a neighbour that ran over two capacities counts under both)"""
    from _libs import DROP_EVENTS, DROP_JOURNAL, DROP_REPAIR_PICKS, DROP_WALK
    return {what: sum(1 for r in rows if r[0] == -1 and r[4] & bit)
            for what, bit in (("journal", DROP_JOURNAL), ("repair_picks", DROP_REPAIR_PICKS), ("walk", DROP_WALK), ("events", DROP_EVENTS))}
