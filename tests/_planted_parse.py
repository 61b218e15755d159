"""Valid parses whose walk states are known in advance, so that the joints of a crossover can be
planted at chosen positions without a search.  Test infrastructure only.

The input has period D.  A parse opens with D literals and one MATCH of distance D at position D; from D + 2 on it uses
LITERAL, SHORT_REP and LONG_REP of index 0 only.  Any copy at distance D reproduces a periodic input, so every such parse
is valid, and none of those packets touches the rep distances: they stay (D - 1, 0, 0, 0) to the end.  Two such parses
therefore meet exactly where both start a packet with the same ctx_state, and ctx_state is easy to steer:

  * three literals bring it to 0 from any state, so "every parent codes [j - 3, j) as literals" (`sync_at(j)`) makes j a
    joint;
  * behind a LONG_REP it is 8 or 11, behind a SHORT_REP 9 or 11, and between literals that follow three literals it is 0:
    where one parent runs LONG_REPs (or SHORT_REPs) and another literals there is no joint, however long the stretch is.
    A "rep" stretch of two positions or more ends with a LONG_REP, never with a literal, so that the three literals of a
    `sync_at(j)` behind it reach state 0 at j and not before.

Off-walk entries are stale but well-formed, the classes tests/_random_parse.py lays down (a MATCH that reproduces the
input, a LONG_REP of any index that stays inside the input, a SHORT_REP, a literal); `poison=True` fills them with entries
no walk may ever take instead: type 0, a type above LONG_REP, length 0.

Draws come from the project's counter RNG (corpus._stream), so (n, D, segments, seed) names one slab on every Python."""
from __future__ import annotations

import numpy as np

from _libs import LITERAL, LONG_REP, MATCH, PACKET, SHORT_REP
from megalania_amd import corpus

MAX_LEN = 273
STYLES = ("lit", "rep", "short", "mix")
POISON = ("type0", "type_high", "len0")
_LANE_DATA, _LANE_LENS, _LANE_MIX, _LANE_STALE = 41, 42, 43, 44


def _draws(seed: int, lane: int, count: int) -> np.ndarray:
    return (corpus._stream(seed, lane, 0, max(1, count)) >> np.uint64(11)).astype(np.int64)


def periodic_input(n: int, D: int, seed: int) -> bytes:
    """a seeded random block of D bytes, repeated and cut to n"""
    block = (corpus._stream(seed, _LANE_DATA, 0, D) & np.uint64(0xFF)).astype(np.uint8).tobytes()
    return (block * (n // D + 1))[:n]


def rep_lengths(seed: int) -> list:
    """the lengths a "rep" stretch cycles through: both ends of 2..273 and three seeded ones in between"""
    return [MAX_LEN, 2] + [int(2 + x % (MAX_LEN - 1)) for x in _draws(seed, _LANE_LENS, 3)]


def sync_at(j: int):
    """the stretch that makes j a joint when every parent has it: literals up to j.  The stretch before it has to end at
    j - 3 or earlier in every parent (`layout` sees to that)."""
    return (j, "lit")


def layout(n: int, D: int, joints, styles) -> list:
    """The (end, style) stretches of a parse with `sync_at` before every planted joint.  joints: sorted, each in
    [D + 5, n); styles: one per region, len(joints) + 1 of them -- region r is [joints[r - 1], joints[r]) less its three
    closing literals, the first one begins at D + 2 and the last one runs to n with no literals behind it."""
    joints = list(joints)
    assert joints == sorted(set(joints)) and len(styles) == len(joints) + 1
    assert not joints or (joints[0] >= D + 5 and joints[-1] < n), (joints[:1], joints[-1:], n, D)
    segs, pos = [], D + 2
    for j, style in zip(joints, styles):
        if j - 3 > pos:
            segs.append((j - 3, style))
        segs.append(sync_at(j))
        pos = j
    if pos < n:
        segs.append((n, styles[-1]))
    return segs


def planted_parse(n: int, D: int, segments, seed: int = 0, stale: bool = True, poison: bool = False, stale_seed=None) -> np.ndarray:
    """Literals on 0..D-1, MATCH(dist = D - 1, len = 2) at D, then the stretches `segments` = [(end, style), ...], which
    must tile [D + 2, n).  An input too short for the MATCH (n < D + 2) gets the all-literal parse and takes no stretches.
    seed: the "rep" lengths and the "mix" draws; stale_seed (default: seed): the off-walk entries.  stale=False leaves
    literals off the walk; poison=True puts malformed entries there."""
    typ = np.full(n, LITERAL, dtype=np.uint8)
    dist = np.zeros(n, dtype=np.uint32)
    ln = np.ones(n, dtype=np.uint16)
    on = np.ones(n, dtype=bool)
    if n < D + 2:
        assert not list(segments)
        return _records(typ, dist, ln)

    def put(pos, t, length):
        typ[pos], ln[pos] = t, length
        on[pos + 1:pos + length] = False
        return pos + length

    typ[D], dist[D], ln[D] = MATCH, D - 1, 2
    on[D + 1] = False
    lens = rep_lengths(seed)
    mix = _draws(seed, _LANE_MIX, n)
    pos, k = D + 2, 0
    for end, style in segments:
        assert style in STYLES and pos <= end <= n, (pos, end, n, style)
        while pos < end:
            rem = end - pos
            kind = style if style != "mix" else ("lit", "short", "rep", "rep")[int(mix[pos]) & 3]
            if kind == "lit" or (kind == "rep" and rem == 1):  # a last leftover position becomes a literal
                pos += 1
            elif kind == "short":
                pos = put(pos, SHORT_REP, 1)
            else:
                length = min(lens[k % len(lens)], rem)
                k += 1
                if style == "rep" and rem - length == 1:  # leave room for a LONG_REP, not for a literal
                    length += 1 if length == 2 else -1
                pos = put(pos, LONG_REP, length)
    assert pos == n, (pos, n)
    off = np.nonzero(~on)[0]
    if (stale or poison) and len(off):
        r = _draws(seed if stale_seed is None else stale_seed, _LANE_STALE, 3 * len(off)).reshape(3, -1)
        room = np.minimum(MAX_LEN, n - off)
        # the classes of _random_parse._stale_entry: a MATCH a whole number of periods back, a LONG_REP of any index with a
        # length that stays inside the input, a SHORT_REP, a literal
        kind = np.where(room >= 2, r[0] % 4, 2 + r[0] % 2)
        t = np.choose(kind, [MATCH, LONG_REP, SHORT_REP, LITERAL])
        d = np.choose(kind, [(1 + r[1] % (off // D)) * D - 1, r[1] % 4, 0, 0])
        length = np.where(kind < 2, 2 + r[2] % np.maximum(room - 1, 1), 1)
        if poison:  # a third each: type 0, a type above LONG_REP, length 0 (under any type)
            cls = r[0] // 4 % 3
            t = np.choose(cls, [0, np.choose(r[1] // 4 % 3, [LONG_REP + 1, 128, 255]), t])
            length = np.where(cls == 2, 0, length)
        typ[off], dist[off], ln[off] = t, d, length
    return _records(typ, dist, ln)


def _records(typ, dist, ln) -> np.ndarray:
    slab = np.zeros(len(typ), dtype=PACKET)
    slab["type"], slab["dist"], slab["len"] = typ, dist, ln
    return slab


def rotating_parents(n: int, D: int, joints, P: int, seed: int = 0, poison: bool = False) -> list:
    """P parents over the planted joints j_1 < ... (0 and n are joints anyway): parent r mod P codes region r as "rep",
    every other parent codes it as "lit".  The winners rotate through the parents, none is the cheapest overall, and the
    child is much cheaper than each."""
    m = len(joints) + 1
    return [planted_parse(n, D, layout(n, D, joints, ["rep" if r % P == p else "lit" for r in range(m)]), seed + 16 * p, poison=poison)
            for p in range(P)]


def tie_parents(n: int, D: int, joints, seed: int = 0, pair_first: bool = False) -> list:
    """One parent all literals behind D + 2, and two that walk alike, "rep" in every region: they cost the same everywhere
    and less than the literals.  The off-walk entries of the two differ, so the child tells which of them a region came
    from.  The pair goes last, or first."""
    m = len(joints) + 1
    lit = planted_parse(n, D, layout(n, D, joints, ["lit"] * m), seed)
    pair = [planted_parse(n, D, layout(n, D, joints, ["rep"] * m), seed, stale_seed=seed + 1 + i) for i in range(2)]
    return pair + [lit] if pair_first else [lit] + pair


def on_walk(slab) -> np.ndarray:
    on = np.zeros(len(slab), dtype=bool)
    pos, lens = 0, slab["len"]
    while pos < len(slab):
        on[pos] = True
        pos += int(lens[pos])
    return on


def malformed(slab, pos: int, cls: str) -> np.ndarray:
    """A copy with the one-byte packet at the on-walk position pos made an entry no walk accepts.  One-byte packets only:
    the walk behind mgl_cost_slab flags such an entry, costs a literal in its place and goes on, and behind a one-byte
    packet it goes on along the parse's own, valid walk."""
    assert cls in POISON and int(slab[pos]["len"]) == 1, (pos, cls)
    out = slab.copy()
    if cls == "type0":
        out["type"][pos] = 0
    elif cls == "type_high":
        out["type"][pos] = LONG_REP + 1
    else:
        out["len"][pos] = 0
    return out
