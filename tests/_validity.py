"""When a slab is a valid parse of an input, restated in plain Python, and a table of slabs that are each one step
away from that line.  Test infrastructure only: nothing here calls into libmegalania_hip or the host library.

`violations` is the rule both gates must match -- k_validate behind the walks of the device (csrc/mgl_kernels3.hip) and
slab_is_valid in front of the host emitter (host/mgl_host.c).  It looks at the entries on the slab's walk only, takes the
source of a rep packet from its own rep stack, and names every clause the first offending packet violates; the clause
names are the host's reasons.

`cases` builds one small input, one valid base parse of it and a list of variants.  Every refused variant edits one
on-walk entry of an accepted one (`rep-stack-shift` edits a MATCH and leaves the rep packet that becomes invalid
untouched) and violates exactly one clause, and the rest of its walk is valid: a gate that lost that one clause accepts
it.  The input (n = 773: three blocks of 256 threads and 13 bitmap words, both with a ragged last one; window 256):

  [0, 291)    a run of one byte: every distance below the position is a valid source there
  [291, 773)  a block of 16 distinct bytes repeated: a copy is valid exactly at the multiples of 16 -- so the four rep slots
              hold four distinct valid distances -- except for the one planted byte at X = 448, which no source matches
              and which matches no destination

The base parse: literals, the overlapping copy MATCH(dist 0, len 273) inside the run, four MATCHes at 360..367 that load
the rep stack with (15, 31, 47, 63), a zone of literals around X where the byte-level variants are planted, the pair
M' = MATCH at 520 / R' = LONG_REP 0 at 528 of `rep-stack-shift`, and a tail with SHORT_REPs and LONG_REPs of every index
whose last packet ends at n.  Entries under the run's copy are stale but valid wherever a walk enters them (a variant that
makes that copy malformed walks into them); entries under the tail's packets are stale and mostly wrong if walked."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from _libs import LITERAL, LONG_REP, MATCH, PACKET, SHORT_REP, literal_slab
from test_gpu_optimal import advance

MIN_LEN, MAX_LEN = 2, 273

# the clauses, named after the reasons slab_is_valid prints
NOT_A_PACKET = "not a packet"                       # type 0 or above 4, length 0, runs past n
LITERAL_LONG = "literal longer than 1"
SHORT_REP_LONG = "short rep longer than 1"
LENGTH_RANGE = "length outside 2..273"              # MATCH, LONG_REP
REP_INDEX = "rep index above 3"
BEFORE_START = "source before the start"            # src >= p
OUTSIDE_WINDOW = "source outside the window"        # src >= dict_limit
BYTES_DIFFER = "bytes differ"
CLAUSES = (NOT_A_PACKET, LITERAL_LONG, SHORT_REP_LONG, LENGTH_RANGE, REP_INDEX, BEFORE_START, OUTSIDE_WINDOW, BYTES_DIFFER)
# the clauses of "this entry is no packet" (mgl_pk_wellformed of csrc/mgl_model.h, with `fits`)
MALFORMED = (NOT_A_PACKET, LITERAL_LONG, SHORT_REP_LONG, LENGTH_RANGE, REP_INDEX)


def wellformed(t: int, d: int, l: int) -> bool:
    """mgl_pk_wellformed restated"""
    if t in (LITERAL, SHORT_REP):
        return l == 1
    if t == MATCH:
        return MIN_LEN <= l <= MAX_LEN
    if t == LONG_REP:
        return MIN_LEN <= l <= MAX_LEN and d <= 3
    return False


def violations(data, slab, dict_limit, every=False):
    """[(position, clause), ...]: every clause that the first offending packet on the walk violates; [] for a valid parse.
    every=True: the same for every offending packet, along the walk the device takes -- an entry that is no packet is
    walked as a literal, any other by its length and with its effect on the rep stack."""
    n = len(data)
    pos, reps, out = 0, (0, 0, 0, 0), []
    while pos < n:
        t, d, l = (int(x) for x in slab[pos])
        v = []
        if not LITERAL <= t <= LONG_REP or l == 0 or pos + l > n:
            v.append(NOT_A_PACKET)
        if t == LITERAL and l > 1:
            v.append(LITERAL_LONG)
        if t == SHORT_REP and l > 1:
            v.append(SHORT_REP_LONG)
        if t in (MATCH, LONG_REP) and not MIN_LEN <= l <= MAX_LEN:
            v.append(LENGTH_RANGE)
        if t == LONG_REP and d > 3:
            v.append(REP_INDEX)
        src = d if t == MATCH else reps[0] if t == SHORT_REP else reps[d] if t == LONG_REP and d <= 3 else None
        if src is not None:
            if src >= pos:
                v.append(BEFORE_START)
            if src >= dict_limit:
                v.append(OUTSIDE_WINDOW)
            if src < pos and any(data[pos + k] != data[pos + k - src - 1] for k in range(min(l, n - pos))):
                v.append(BYTES_DIFFER)
        out += [(pos, c) for c in v]
        if v and not every:
            break
        if wellformed(t, d, l) and pos + l <= n:
            _, reps = advance(0, reps, t, d)
            pos += l
        else:
            pos += 1
    return out


def on_walk(slab) -> np.ndarray:
    """the positions the device's walk visits (an entry that is no packet counts as a literal)"""
    n = len(slab)
    on = np.zeros(n, dtype=bool)
    pos = 0
    while pos < n:
        on[pos] = True
        t, d, l = (int(x) for x in slab[pos])
        pos += l if wellformed(t, d, l) and pos + l <= n else 1
    return on


# ---- the table

N, DICT_LIMIT = 773, 256
RUN, PERIOD, X = 291, 16, 448
Case = namedtuple("Case", "id slab clause line edits twin")
"""clause: the one clause a refused case violates, None for an accepted one.  line: the line of the issue's list the case
stands for (0: the base parse).  edits: [(position, (type, dist, len))], the entries that differ from `twin` (the id of the
accepted case it was made from; None for the base)."""


def make_input(n: int = N) -> bytes:
    assert n == N
    block = bytes(0x80 + 5 * i for i in range(PERIOD))
    data = bytearray(b"a" * RUN + bytes(block[i % PERIOD] for i in range(RUN, n)))
    data[X] = 0
    assert len(set(block)) == PERIOD and 0 not in block and ord("a") not in block
    return bytes(data)


# the packets of the base parse that are not literals: position -> (type, dist, len)
BASE_PACKETS = {
    3: (MATCH, 0, 273),       # the overlapping copy, the first non-literal packet; [3, 276)
    360: (MATCH, 63, 2), 362: (MATCH, 47, 2), 364: (MATCH, 31, 2), 366: (MATCH, 15, 2),  # reps = (15, 31, 47, 63) from 368 on
    480: (LONG_REP, 0, 2),    # R
    520: (MATCH, 15, 2),      # M'
    528: (LONG_REP, 0, 2),    # R', source 512 under M', X under M' at distance 80
    580: (MATCH, 63, 2), 582: (MATCH, 47, 2), 584: (MATCH, 31, 2), 586: (MATCH, 15, 2),
    588: (SHORT_REP, 0, 1),
    589: (LONG_REP, 1, 17),   # [589, 606), reps (31, 15, 47, 63)
    607: (LONG_REP, 2, 9),    # [607, 616), reps (47, 31, 15, 63)
    616: (LONG_REP, 3, 40),   # [616, 656), reps (63, 47, 31, 15)
    657: (SHORT_REP, 0, 1),
    658: (LONG_REP, 0, 60),   # [658, 718)
    721: (LONG_REP, 1, 22),   # [721, 743), reps (47, 63, 31, 15)
    743: (LONG_REP, 0, 30),   # the last packet: ends at n
}
LAST = 743


def _stale(slab, on):
    """off-walk entries: under the run's copy whatever is valid wherever a walk enters it and is back on the base's walk at
    276; under the tail's packets the classes of tests/_random_parse.py, wrong sources and rep indices included.  The
    off-walk entries of the two-byte packets and of the last packet stay literals: the variants that break such a packet
    walk into them."""
    for q in np.nonzero(~on)[0]:
        q = int(q)
        if 3 < q < 276:
            room = 276 - q
            kind = q % 4 if room >= 2 else 2 + q % 2
            length = 2 + (q * 7) % min(room - 1, 40) if room >= 3 else 2
            slab[q] = [(MATCH, (q * 5) % min(q, DICT_LIMIT), length), (LONG_REP, (q // 4) % 4, length), (SHORT_REP, 0, 1),
                       (LITERAL, 0, 1)][kind]
        elif 588 < q < LAST:
            room = N - q
            kind = q % 5 if room >= 2 else 2
            length = 2 + (q * 3) % min(room - 1, MAX_LEN - 1) if room >= 2 else 1
            slab[q] = [(MATCH, PERIOD * (1 + q % 4) - 1, length), (LONG_REP, q % 4, length), (SHORT_REP, 0, 1),
                       (MATCH, q % 13, length), (LITERAL, 0, 1)][kind]


def base_parse(n: int = N) -> np.ndarray:
    assert n == N
    slab = literal_slab(n)
    on = np.ones(n, dtype=bool)
    for p, (t, d, l) in BASE_PACKETS.items():
        slab[p] = (t, d, l)
        on[p + 1:p + l] = False
    _stale(slab, on)
    return slab


def poisoned(slab) -> np.ndarray:
    """every off-walk entry replaced by one no walk may take: type 0, type 9, length 0, length 60000"""
    out = slab.copy()
    for k, q in enumerate(np.nonzero(~on_walk(slab))[0]):
        t, d, l = (int(x) for x in out[q])
        out[q] = [(0, d, l), (9, d, l), (t, d, 0), (t, d, 60000)][k % 4]
    return out


def cases(n: int = N, dict_limit: int = DICT_LIMIT):
    """(data, base, [Case, ...]); the list opens with the base parse itself"""
    assert (n, dict_limit) == (N, DICT_LIMIT)
    data, base = make_input(n), base_parse(n)
    made = {"base": base}
    out = [Case("base", base, None, 0, [], None)]

    def add(cid, twin, edits, clause, line):
        slab = made[twin].copy()
        for p, e in edits:
            slab[p] = e
        made[cid] = slab
        out.append(Case(cid, slab, clause, line, list(edits), twin))

    L, M, S, R = LITERAL, MATCH, SHORT_REP, LONG_REP
    # 1. no packet at all: on literals, at the edges of a 64-bit bitmap word and of a block of 256 threads
    add("type0@511", "base", [(511, (0, 0, 1))], NOT_A_PACKET, 1)        # p % 64 = 63, p % 256 = 255
    add("len0@512", "base", [(512, (L, 0, 0))], NOT_A_PACKET, 1)         # p % 64 = 0, p % 256 = 0
    add("type5@319", "base", [(319, (5, 0, 1))], NOT_A_PACKET, 1)        # p % 64 = 63
    add("type255@320", "base", [(320, (255, 0, 1))], NOT_A_PACKET, 1)    # p % 64 = 0
    # 2. the last packet of the walk: one byte past the input; the base's ends at n
    add("past-end@last", "base", [(LAST, (R, 0, n + 1 - LAST))], NOT_A_PACKET, 2)
    # 3.
    add("literal-len2", "base", [(300, (L, 0, 2))], LITERAL_LONG, 3)
    add("short-rep-len2", "base", [(588, (S, 0, 2))], SHORT_REP_LONG, 3)
    # 4. both ends of 2..273, for both kinds; the base has MATCH 2 at 360, MATCH 273 at 3 and LONG_REP 2 at 480
    add("match-len1", "base", [(360, (M, 63, 1))], LENGTH_RANGE, 4)
    add("match-len274@first", "base", [(3, (M, 0, 274))], LENGTH_RANGE, 4)  # the first non-literal packet
    add("long-rep-len273", "base", [(3, (R, 0, 273))], None, 4)
    add("long-rep-len274", "long-rep-len273", [(3, (R, 0, 274))], LENGTH_RANGE, 4)
    add("long-rep-len1", "base", [(480, (R, 0, 1))], LENGTH_RANGE, 4)
    # 5.
    add("rep-index3", "base", [(480, (R, 3, 2))], None, 5)
    add("rep-index4", "rep-index3", [(480, (R, 4, 2))], REP_INDEX, 5)
    add("rep-index-max", "rep-index3", [(480, (R, 0xFFFFFFFF, 2))], REP_INDEX, 5)
    # 6. a source one before the input, and the first byte of the input as a source
    add("match-dist-p-1", "base", [(1, (M, 0, 2))], None, 6)
    add("match-dist-p", "match-dist-p-1", [(1, (M, 1, 2))], BEFORE_START, 6)
    # 7. the rep distances start as 0, which is not below position 0
    add("short-rep@1", "base", [(1, (S, 0, 1))], None, 7)
    add("short-rep@0", "base", [(0, (S, 0, 1))], BEFORE_START, 7)
    # 8.
    add("long-rep@1", "base", [(1, (R, 2, 2))], None, 8)
    add("long-rep@0", "base", [(0, (R, 1, 2))], BEFORE_START, 8)
    # 9. the window's edge, where the start of the input is far enough away not to matter
    add("match-window-1", "base", [(280, (M, dict_limit - 1, 2))], None, 9)
    add("match-window", "match-window-1", [(280, (M, dict_limit, 2))], OUTSIDE_WINDOW, 9)
    # 10. one differing byte: the first, the last, and one inside the part of an overlapping copy that copies the copy
    add("match-first-byte-ok", "base", [(X + 16, (M, 47, 5))], None, 10)
    add("match-first-byte", "match-first-byte-ok", [(X + 16, (M, 15, 5))], BYTES_DIFFER, 10)
    add("match-last-byte-ok", "base", [(X + 12, (M, 15, 4))], None, 10)
    add("match-last-byte", "match-last-byte-ok", [(X + 12, (M, 15, 5))], BYTES_DIFFER, 10)
    add("match-overlap-ok", "base", [(X - 20, (M, 15, 20))], None, 10)
    add("match-overlap", "match-overlap-ok", [(X - 20, (M, 15, 40))], BYTES_DIFFER, 10)
    add("match-ok@511", "base", [(511, (M, 15, 2))], None, 10)
    add("match-bytes@511", "match-ok@511", [(511, (M, 14, 2))], BYTES_DIFFER, 10)   # p % 64 = 63, p % 256 = 255
    # 11.
    add("short-rep-ok", "base", [(X + 17, (S, 0, 1))], None, 11)
    add("short-rep-bytes", "base", [(X + 16, (S, 0, 1))], BYTES_DIFFER, 11)
    # 12. LONG_REP k at X + 16 (k + 1): rep k alone has X as its source.  The twin's index is one that keeps R valid behind it
    for k, ok in enumerate((2, 2, 3, 0)):
        p = X + 16 * (k + 1)                                                          # k = 3: p = 512, p % 256 = 0
        add(f"long-rep{k}-ok", "base", [(p, (R, ok, 2))], None, 12)
        add(f"long-rep{k}-bytes", f"long-rep{k}-ok", [(p, (R, k, 2))], BYTES_DIFFER, 12)
    # 13. M' moved to another valid source: R', untouched, now copies from X
    add("rep-stack-shift-ok", "base", [(520, (M, 31, 2))], None, 13)
    add("rep-stack-shift", "base", [(520, (M, 79, 2))], BYTES_DIFFER, 13)
    # 15. poison off the walk only
    made["poison"] = poisoned(base)
    out.append(Case("poison", made["poison"], None, 15, [], "base"))
    return data, base, out


# 14. where the offending entry of a refused case must also have been placed
PLACEMENTS = {"p % 64 == 0": lambda p: p % 64 == 0, "p % 64 == 63": lambda p: p % 64 == 63,
              "p % 256 == 0": lambda p: p % 256 == 0, "p % 256 == 255": lambda p: p % 256 == 255,
              "first non-literal packet": lambda p: p == 3, "last packet": lambda p: p == LAST}


def as_slab(slab) -> np.ndarray:
    return np.ascontiguousarray(slab).astype(PACKET)
