"""Segment re-parse restated in Python integers (include/megalania_hip.h, "Segment re-parse"; DESIGN.md section 10;
mgl_segparse.hip): per segment the passes of the adaptive parse from the state reset at its start and under its own triple,
the choice among them, the join into one slab and the guard.  Built from the pieces the other restatements export: the event
model and the MATCH sources of tests/test_gpu_optimal.py, the model update and the sources' lengths of
tests/test_adaptive_rule_cpu.py (whose adaptive_rule `chunk_dp` below repeats for one chunk that may start anywhere), the
re-expression of tests/_segments.py.  The nearest match finder only.  Test infrastructure; shared by the CPU and GPU tests."""
from __future__ import annotations

import functools

import numpy as np

import _segments as S
from _libs import Oracle
from test_adaptive_rule_cpu import _mlen, _sources, model_update
from test_gpu_optimal import (INF, LIT, LONG_REP, MATCH, OFF_LEN, OFF_REP_LEN, SHORT_REP, advance, dist_events, header_events,
                              length_events, literal_events, nprobs, packet_events)

RESET = (0, (0, 0, 0, 0))  # ctx_state and rep distances behind an LZMA2 state reset -- and of the LZMA initial state
MIN_CHUNK, DEF = 512, dict(passes=3, cand=16, chunk=4096, segment=64, ahead=128)


def settings(n, passes=0, cand=0, chunk=0, segment=0, ahead=0):
    """the defaults and clamps of the library (adp_args): a chunk or a commit distance longer than the input acts like one of its length"""
    passes, cand, chunk = passes or DEF["passes"], cand or DEF["cand"], chunk or DEF["chunk"]
    if segment == 0:
        segment, ahead = DEF["segment"], DEF["ahead"]
    if chunk > n:
        chunk = max(n, MIN_CHUNK)
    return passes, cand, chunk, min(segment, chunk), ahead


def coder_walk(data, packets, lo, hi, props, chunk):
    """The segment's coder over `packets` [(type, dist, len)], which tile [lo, hi): fresh model under `props`, ctx_state 0, rep
    distances (0, 0, 0, 0) at lo.  Returns (exact cost, per chunk of the grid that starts at lo: (ctx_state, reps, model) as
    they stand before the packet that starts there; a chunk start inside a packet takes the reset state and the model before
    that packet)."""
    lc, lp, pb = props
    T = Oracle.cost_table().astype(np.int64)
    M = np.full(nprobs(lc, lp), 1024, dtype=np.int64)
    starts = [None] * (-(-(hi - lo) // chunk))
    pos, (ctx, reps), cost = lo, RESET, 0
    for t, d, l in packets:
        for m in range(-(-(pos - lo) // chunk), -(-(pos + l - lo) // chunk)):
            starts[m] = (ctx, reps, M.copy()) if lo + m * chunk == pos else RESET + (M.copy(),)
        ev, nd = packet_events(data, lc, lp, pb, pos, ctx, reps, t, d, l)
        cost += sum(int(T[2048 - M[c]] if b else T[M[c]]) for c, b in ev) + 2048 * nd
        model_update(M, ev)
        ctx, reps = advance(ctx, reps, t, d)
        pos += l
    assert pos == hi, (pos, hi)
    return cost, starts


def resolve_one(reps, t, D, l):
    """opt_resolve: the copy (type, absolute distance, len) against the rep stack `reps`"""
    if t == LIT:
        return LIT, 0, l
    if l == 1:
        return (SHORT_REP, 0, 1) if reps[0] == D - 1 else (LIT, 0, 1)
    return (LONG_REP, reps.index(D - 1), l) if D - 1 in reps else (MATCH, D - 1, l)


def resolved(copies, lo, hi, reps=RESET[1]):
    """the copies (position-indexed) that tile [lo, hi), resolved in walk order against a stack that starts as `reps`"""
    out, pos = [], lo
    while pos < hi:
        q = resolve_one(reps, *copies[pos])
        out.append(q)
        _, reps = advance(0, reps, q[0], q[1])
        pos += q[2]
    assert pos == hi, (pos, hi)
    return out


def chunk_dp(data, out, T, srcs, props, s, e, start, segment, ahead):
    """adaptive_rule's chunk [s, e) from `start` = (ctx_state, reps, model), its copies written to out[s:e]; returns the objective"""
    lc, lp, pb = props
    d = np.frombuffer(data, dtype=np.uint8)
    lc4 = np.minimum(np.arange(2, 274) - 2, 3)
    ctx0, reps0, M = start
    M = M.copy()
    objective, a, st_a = 0, s, (ctx0, reps0)
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
        edge, state, back = [None] * (m + 1), [None] * (m + 1), [None] * (m + 1)
        state[0] = st_a
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
                        rows.append((5 + D, MATCH, D, hdr(ctx, ps, MATCH, 0) + distp(D - 1)[lc4[:ml - 1]] + lenp(OFF_LEN, ps)[:ml - 1]))
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
        path, j = [], m
        while j > 0:
            path.append((j - back[j][2], j))
            j -= back[j][2]
        horizon, k = (m if end == e else segment), 0
        for k0, k1 in reversed(path):
            if k0 >= horizon:
                break
            t, x, l = edge[k1]
            ctx, reps = state[k0]
            out[a + k0] = back[k1]
            model_update(M, packet_events(data, lc, lp, pb, a + k0, ctx, reps, t, x - 1 if t == MATCH else x, l)[0])
            k = k1
        objective += int(tot[k])
        a, st_a = a + k, state[k]
    return objective


def segment_pass(data, out, starts, lo, hi, props, cand, chunk, segment, ahead, dict_limit):
    """one DP pass over the chunks of [lo, hi) from `starts`, the copies into out[lo:hi]; returns the objective"""
    T = Oracle.cost_table().astype(np.int64)
    srcs = _sources(bytes(data), cand, dict_limit)
    out[lo:hi] = [(LIT, 0, 1)] * (hi - lo)
    return sum(chunk_dp(data, out, T, srcs, props, s, min(s + chunk, hi), starts[m], segment, ahead)
               for m, s in enumerate(range(lo, hi, chunk)))


def true_stacks(slab, cuts):
    """the rep distances of the slab's own walk from byte 0 at every cut (all packet starts)"""
    out, t, pos = {}, [0, 0, 0, 0], 0
    for c in cuts:
        while pos < c:
            e = slab[pos]
            t = S.advance_reps(t, int(e["type"]), int(e["dist"]))
            pos += int(e["len"])
        assert pos == c, (pos, c)
        out[c] = list(t)
    return out


def join(slab, segs, kept):
    """One walk from byte 0: segment k takes kept[k] (position-indexed DP copies) or, where that is None, the input's packets with
    their distances made absolute through the input's own stack; every copy is resolved against the output's running stack."""
    n = len(slab)
    stacks = true_stacks(slab, [lo for lo, _, _ in segs])
    packets, reps = [], RESET[1]
    for (lo, hi, _), copies in zip(segs, kept):
        if copies is None:
            copies, t, pos = {}, stacks[lo], lo
            while pos < hi:
                typ, dist, ln = (int(slab[pos][k]) for k in ("type", "dist", "len"))
                D = {LIT: 0, MATCH: dist + 1, SHORT_REP: t[0] + 1}.get(typ) if typ != LONG_REP else t[dist] + 1
                copies[pos] = (typ, D, ln)
                t = S.advance_reps(t, typ, dist)
                pos += ln
        seg = resolved(copies, lo, hi, reps)
        for q in seg:
            _, reps = advance(0, reps, q[0], q[1])
        packets += seg
    return S.slab_of(packets, n)


def segment_cost(data, slab, lo, hi, props):
    """cost(lo, hi, T) of "Segment props": the re-expressed packets of [lo, hi) through the segment's coder"""
    return coder_walk(data, S.reexpress(slab, lo, hi)[0], lo, hi, props, hi - lo)[0]


def segment_rule(data, slab, segs, dict_limit=0x400000, **cfg):
    """mgl_segment_reparse: segs = [(lo, hi, (lc, lp, pb))] tiling the input at packet starts of `slab`.  Returns (slab out,
    stats per segment: dict(passes, best_pass, start_cost, final_cost, pass_cost, objective, kept = the taken pass's copies of
    [lo, hi) or None), taken)."""
    data = bytes(data)
    passes, cand, chunk, segment, ahead = settings(len(data), **cfg)
    stats = []
    for lo, hi, props in segs:
        start_cost, starts = coder_walk(data, S.reexpress(slab, lo, hi)[0], lo, hi, props, chunk)
        st = dict(passes=passes, best_pass=None, start_cost=start_cost, final_cost=start_cost, pass_cost=[], objective=[], kept=None)
        best, out = start_cost, [None] * len(data)
        for p in range(passes):
            st["objective"].append(segment_pass(data, out, starts, lo, hi, props, cand, chunk, segment, ahead, dict_limit))
            cost, starts = coder_walk(data, resolved(out, lo, hi), lo, hi, props, chunk)
            st["pass_cost"].append(cost)
            if cost < best:
                best, st["best_pass"], st["kept"] = cost, p, {q: out[q] for q in range(lo, hi)}
        stats.append(st)
    taken, result = False, slab
    if any(st["best_pass"] is not None for st in stats):
        joined = join(slab, segs, [st["kept"] for st in stats])
        final = [segment_cost(data, joined, lo, hi, props) for lo, hi, props in segs]
        taken = sum(final) < sum(st["start_cost"] for st in stats)
        if taken:
            result = joined
            for st, c in zip(stats, final):
                st["final_cost"] = c
    if not taken:
        for st in stats:
            st["best_pass"] = None
    return result, stats, taken
