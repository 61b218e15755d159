"""The rule of the adaptive-price optimal parse (`mgl_adaptive_pass`, mgl_adaptive.hip) restated in plain Python,
and what can be said about it without a GPU: on small inputs its parse is valid, costed by the oracle, decoded by
liblzma, keeps inside the window, and every commit moves the anchor forward.  tests/test_gpu_adaptive.py holds
the device against `adaptive_rule`.

One pass takes a valid slab P_in.
  chunk starts   P_in is walked from the LZMA initial state with a live model (all slots 1024, updated per bit as
                 the range coder does).  A packet that starts at a multiple of `chunk` leaves its walk state and a
                 copy of the model there.  A multiple of `chunk` that a packet jumps over takes the LZMA initial
                 state (as k_opt_dp's chunks do without an entry) and the model as it stands before that packet.
  chunk [s, e)   anchor a = s with the chunk's state and model M.  Until a == e: end = min(a + segment + ahead, e);
                 k_opt_dp's forward shortest path over the nodes a..end with cap = min(273, end - i), the price of
                 (slot, bit) being T[M[slot]] or T[2048 - M[slot]] with M frozen; the path is read back from `end`;
                 its packets that start before a + segment are committed (all of them when end == e): written out
                 in k_opt_dp's unresolved form, their events applied to M under the path's exact states; the node
                 the last committed packet ends on is the next anchor, its total joins the objective."""
import functools
import lzma

import numpy as np
import pytest

from _libs import Oracle, literal_slab
from megalania_amd import binding
from test_gpu_greedy import greedy_rule
from test_gpu_optimal import (INF, LIT, LONG_REP, MATCH, OFF_LEN, OFF_REP_LEN, SHORT_REP, SMALL, advance, candidates,
                              dist_events, header_events, length_events, literal_events, nprobs, packet_events)


def model_update(M, events):
    for c, b in events:
        p = int(M[c])
        M[c] = p - (p >> 5) if b else p + ((2048 - p) >> 5)


def chunk_starts(data, slab, lc, lp, pb, chunk):
    """per chunk: (ctx_state, reps, model) as the walk of `slab` (a resolved, valid parse) leaves them"""
    n = len(data)
    M = np.full(nprobs(lc, lp), 1024, dtype=np.int64)
    out = [None] * ((n + chunk - 1) // chunk)
    pos, ctx, reps = 0, 0, (0, 0, 0, 0)
    while pos < n:
        t, d, l = int(slab["type"][pos]), int(slab["dist"][pos]), int(slab["len"][pos])
        for m in range((pos + chunk - 1) // chunk, (pos + l + chunk - 1) // chunk):
            out[m] = (ctx, reps, M.copy()) if m * chunk == pos else (0, (0, 0, 0, 0), M.copy())
        model_update(M, packet_events(data, lc, lp, pb, pos, ctx, reps, t, d, l)[0])
        ctx, reps = advance(ctx, reps, t, d)
        pos += l
    return out


@functools.lru_cache(maxsize=8)
def _sources(data, cand, dict_limit):
    """per position: the MATCH sources as (q, match length capped at 273 and at the end of the input)"""
    d = np.frombuffer(data, dtype=np.uint8)
    n = len(data)
    out = []
    for i, qs in enumerate(candidates(data, cand, dict_limit)):
        cap = min(273, n - i)
        out.append([(q, _mlen(d, q, i, cap)) for q in qs])
    return out


def _mlen(d, q, i, cap):
    ne = d[q:q + cap] != d[i:i + cap]
    k = int(ne.argmax()) if cap else 0
    return k if cap and ne[k] else cap


def adaptive_rule(data, slab_in, cand, chunk, segment, ahead, lc=0, lp=0, pb=0, dict_limit=0x400000):
    """(unresolved slab as a list of (type, absolute distance, len) per position, objective, anchors per chunk)"""
    data = bytes(data)
    n = len(data)
    d = np.frombuffer(data, dtype=np.uint8)
    T = Oracle.cost_table().astype(np.int64)
    srcs = _sources(data, cand, dict_limit)
    lc4 = np.minimum(np.arange(2, 274) - 2, 3)
    out = [(LIT, 0, 1)] * n
    objective = 0
    anchors = []
    for ci, (ctx0, reps0, M) in enumerate(chunk_starts(data, slab_in, lc, lp, pb, chunk)):
        s, e = ci * chunk, min(ci * chunk + chunk, n)
        a, st_a = s, (ctx0, reps0)
        anchors.append([a])
        while a < e:
            end = min(a + segment + ahead, e)
            P0, P1 = T[M], T[2048 - M]

            def price(ev, nd=0):
                return int(sum(P1[c] if b else P0[c] for c, b in ev)) + 2048 * nd

            lenp = functools.lru_cache(maxsize=None)(
                lambda base, ps: np.array([price(length_events(base, l, ps)) for l in range(2, 274)], dtype=np.int64))
            hdr = functools.lru_cache(maxsize=None)(lambda ctx, ps, typ, rep: price(header_events(ctx, ps, typ, rep)))
            distp = functools.lru_cache(maxsize=None)(
                lambda v: np.array([price(*dist_events(v, 2 + k)) for k in range(4)], dtype=np.int64))

            m = end - a
            tot = np.full(m + 1, INF, dtype=np.int64)
            tot[0] = 0
            edge = [None] * (m + 1)  # (type, x, len): x = rep index for LONG_REP, else absolute distance
            state = [None] * (m + 1)
            state[0] = st_a
            back = [None] * (m + 1)
            for k in range(m + 1):
                i = a + k
                if k:
                    t, x, l = edge[k]
                    ctx, reps = state[k - l]
                    back[k] = (t, reps[x] + 1 if t == LONG_REP else x, l)
                    state[k] = advance(ctx, reps, t, x - 1 if t == MATCH else x)
                if k == m:
                    break
                ctx, reps = state[k]
                cap = min(273, end - i)
                ps = i & ((1 << pb) - 1)
                rows = []  # (key, type, x, price per length 2..ml)
                if cap >= 2:
                    for r in range(4):
                        D = reps[r] + 1
                        if D <= i:
                            ml = _mlen(d, i - D, i, cap)
                            if ml >= 2:
                                rows.append((r, LONG_REP, r, hdr(ctx, ps, LONG_REP, r) + lenp(OFF_REP_LEN, ps)[:ml - 1]))
                    for q, full in srcs[i]:
                        ml = min(full, cap)
                        if ml >= 2:
                            D = i - q
                            pr = hdr(ctx, ps, MATCH, 0) + distp(D - 1)[lc4[:ml - 1]] + lenp(OFF_LEN, ps)[:ml - 1]
                            rows.append((5 + D, MATCH, D, pr))
                # length 1: SHORT_REP before LITERAL
                mb = data[i - reps[0] - 1] if ctx >= 7 and reps[0] < i else 0
                prev = data[i - 1] if lc > 0 and i > 0 else 0
                b1 = (price(header_events(ctx, ps, LIT) + literal_events(lc, lp, i, data[i], mb, prev, ctx >= 7)), LIT, 0)
                if reps[0] + 1 <= i and data[i] == data[i - reps[0] - 1]:
                    sr = hdr(ctx, ps, SHORT_REP, 0)
                    if sr <= b1[0]:
                        b1 = (sr, SHORT_REP, reps[0] + 1)
                if tot[k] + b1[0] < tot[k + 1]:
                    tot[k + 1] = tot[k] + b1[0]
                    edge[k + 1] = (b1[1], b1[2], 1)
                if rows:
                    rows.sort(key=lambda r: r[0])
                    W = max(len(r[3]) for r in rows)
                    Mx = np.full((len(rows), W), INF, dtype=np.int64)
                    for j, r in enumerate(rows):
                        Mx[j, :len(r[3])] = r[3]
                    w = np.argmin(Mx, axis=0)  # first minimum = smallest key
                    cand_tot = tot[k] + Mx[w, np.arange(W)]
                    for li in np.nonzero(cand_tot < tot[k + 2:k + 2 + W])[0]:
                        r = rows[w[li]]
                        tot[k + 2 + li] = cand_tot[li]
                        edge[k + 2 + li] = (r[1], r[2], int(li) + 2)
            # the path's packets as (first node, last node), read back from `end`
            path = []
            j = m
            while j > 0:
                path.append((j - back[j][2], j))
                j -= back[j][2]
            path.reverse()
            horizon = m if end == e else segment
            k = 0
            for k0, k1 in path:
                if k0 >= horizon:
                    break
                t, x, l = edge[k1]
                ctx, reps = state[k0]
                out[a + k0] = back[k1]
                model_update(M, packet_events(data, lc, lp, pb, a + k0, ctx, reps, t, x - 1 if t == MATCH else x, l)[0])
                k = k1
            objective += int(tot[k])
            a, st_a = a + k, state[k]
            anchors[-1].append(a)
    return out, objective, anchors


def slab_of(packets):
    s = literal_slab(len(packets))
    for i, (t, x, l) in enumerate(packets):
        s[i] = (t, x, l)
    return s


def resolve(packets):
    """k_opt_walk's resolution: the rule's copies (type, absolute distance, len) against the true rep stack"""
    out = [(LIT, 0, 1)] * len(packets)
    pos, ctx, reps = 0, 0, (0, 0, 0, 0)
    while pos < len(packets):
        t, D, l = packets[pos]
        if t == LIT:
            d = 0
        elif l == 1:
            t, d = (SHORT_REP, 0) if reps[0] == D - 1 else (LIT, 0)
        elif D - 1 in reps:
            t, d = LONG_REP, reps.index(D - 1)
        else:
            t, d = MATCH, D - 1
        out[pos] = (t, d, l)
        ctx, reps = advance(ctx, reps, t, d)
        pos += l
    return out


def greedy_in(data, cand=8, dict_limit=0x400000):
    return slab_of(greedy_rule(data, cand, dict_limit))


@pytest.mark.parametrize("segment,ahead", [(64, 0), (64, 128), (1000, 0), (1000, 128)])
@pytest.mark.parametrize("name,data", SMALL, ids=[s[0] for s in SMALL])
def test_rule_gives_a_valid_parse(name, data, segment, ahead):
    dict_limit = 300 if name == "prose" else 0x400000
    got, objective, anchors = adaptive_rule(data, greedy_in(data, 8, dict_limit), 16, 1000, segment, ahead, dict_limit=dict_limit)
    n = len(data)
    for c, an in enumerate(anchors):
        assert an[0] == c * 1000 and an[-1] == min(c * 1000 + 1000, n)
        assert all(x < y for x, y in zip(an, an[1:])), (c, an)  # every commit advances
    assert all(t != MATCH or D - 1 < dict_limit for t, D, _ in got)
    res = slab_of(resolve(got))
    # a valid parse: every copy reproduces the input, and the walk ends at n
    pos, reps = 0, (0, 0, 0, 0)
    while pos < n:
        t, d, l = (int(x) for x in res[pos])
        if t != LIT:
            D = (d if t == MATCH else reps[d if t == LONG_REP else 0]) + 1
            assert D <= pos and all(data[pos + k] == data[pos + k - D] for k in range(l)), pos
        _, reps = advance(0, reps, t, d)
        pos += l
    assert pos == n
    o = Oracle(data, dict_limit=dict_limit)
    cost = o.cost_slab(res)["total"]
    assert 0 < cost and objective > 0
    assert lzma.decompress(binding.emit_stream(data, res), format=lzma.FORMAT_ALONE) == data


def test_rule_at_other_properties_round_trips():
    data = SMALL[1][1]
    got, _, _ = adaptive_rule(data, greedy_in(data), 16, 1000, 64, 128, lc=3, lp=0, pb=2)
    res = slab_of(resolve(got))
    assert Oracle(data, lc=3, lp=0, pb=2, dict_limit=0x400000).cost_slab(res)["total"] > 0
    assert lzma.decompress(binding.emit_stream(data, res, lc=3, lp=0, pb=2), format=lzma.FORMAT_ALONE) == data
