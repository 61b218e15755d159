"""Optimal-parse seeding (`mgl_sa_seed_optimal`, mgl_optimal.hip): an opt-in starting slab that is not
in the reference.  Pinned here by a plain-Python restatement of the prices and of the DP rule, by the
oracle's costing of the seeded slab, by the oracle's batched SA continuing from it, and by liblzma
decoding the stream.  `-m gpu`."""
import functools
import lzma
import subprocess

import numpy as np
import pytest

from _libs import Oracle, literal_slab
from megalania_amd import binding, build, corpus

pytestmark = pytest.mark.gpu

LIT, MATCH, SHORT_REP, LONG_REP = 1, 2, 3, 4
INF = 1 << 62

# ---- the bit model of mgl_model.h, restated: (slot, bit) events of each part of a packet
IS_MATCH, IS_REP, G0, G1, G2, REP0_LONG = 0, 192, 204, 216, 228, 240
OFF_LEN, OFF_REP_LEN, OFF_DIST, OFF_LIT = 432, 946, 1460, 1847


def tree_events(base, val, nbits):
    out, m = [], 1
    for i in range(nbits - 1, -1, -1):
        b = (val >> i) & 1
        out.append((base + m, b))
        m = (m << 1) | b
    return out


def rev_tree_events(base, val, nbits):
    out, m = [], 1
    for i in range(nbits):
        b = (val >> i) & 1
        out.append((base + m, b))
        m = (m << 1) | b
    return out


def header_events(ctx, ps, typ, rep=0):
    sp = (ctx << 4) + ps
    if typ == LIT:
        return [(IS_MATCH + sp, 0)]
    if typ == MATCH:
        return [(IS_MATCH + sp, 1), (IS_REP + ctx, 0)]
    ev = [(IS_MATCH + sp, 1), (IS_REP + ctx, 1)]
    if typ == SHORT_REP:
        return ev + [(G0 + ctx, 0), (REP0_LONG + sp, 0)]
    if rep == 0:
        return ev + [(G0 + ctx, 0), (REP0_LONG + sp, 1)]
    ev += [(G0 + ctx, 1)]
    if rep == 1:
        return ev + [(G1 + ctx, 0)]
    return ev + [(G1 + ctx, 1), (G2 + ctx, int(rep != 2))]


def length_events(base, length, ps):
    l = length - 2
    if l < 8:
        return [(base, 0)] + tree_events(base + 2 + ps * 8, l, 3)
    if l < 16:
        return [(base, 1), (base + 1, 0)] + tree_events(base + 130 + ps * 8, l - 8, 3)
    return [(base, 1), (base + 1, 1)] + tree_events(base + 258, l - 16, 8)


def dist_events(v, length):
    """(events, direct bits) of distance value v (= distance - 1) at this length"""
    lc4 = min(length - 2, 3)
    if v < 4:
        return tree_events(OFF_DIST + lc4 * 64, v, 6), 0
    nlow = v.bit_length() - 2
    high = v >> nlow
    slot = nlow * 2 + high
    low = v & ((1 << nlow) - 1)
    ev = tree_events(OFF_DIST + lc4 * 64, slot, 6)
    if slot < 14:
        return ev + rev_tree_events(OFF_DIST + 272 + (high << nlow) - slot, low, nlow), 0
    return ev + rev_tree_events(OFF_DIST + 256, low & 15, 4), nlow - 4


def literal_events(lc, lp, pos, byte, match_byte, prev_byte, matched):
    base = OFF_LIT + 0x300 * (((pos & ((1 << lp) - 1)) << lc) + (prev_byte >> (8 - lc)))
    out, m = [], 1
    for i in range(7, -1, -1):
        b = (byte >> i) & 1
        c = m
        if matched and ((byte ^ match_byte) >> (i + 1)) == 0:
            c += (1 + ((match_byte >> i) & 1)) << 8
        out.append((base + c, b))
        m = (m << 1) | b
    return out


def next_ctx(s, typ):
    if typ == LIT:
        return 0 if s < 4 else (s - 3 if s < 10 else s - 6)
    if typ == MATCH:
        return 7 if s < 7 else 10
    if typ == SHORT_REP:
        return 9 if s < 7 else 11
    return 8 if s < 7 else 11


def advance(ctx, reps, typ, dist):
    if typ == MATCH:
        reps = (dist,) + reps[:3]
    elif typ == LONG_REP:
        reps = (reps[dist],) + reps[:dist] + reps[dist + 1:]
    return next_ctx(ctx, typ), reps


def packet_events(data, lc, lp, pb, pos, ctx, reps, typ, dist, length):
    ps = pos & ((1 << pb) - 1)
    if typ == LIT:
        mb = data[pos - reps[0] - 1] if ctx >= 7 and reps[0] < pos else 0
        prev = data[pos - 1] if lc > 0 and pos > 0 else 0
        return header_events(ctx, ps, LIT) + literal_events(lc, lp, pos, data[pos], mb, prev, ctx >= 7), 0
    if typ == MATCH:
        dev, nd = dist_events(dist, length)
        return header_events(ctx, ps, MATCH) + length_events(OFF_LEN, length, ps) + dev, nd
    if typ == SHORT_REP:
        return header_events(ctx, ps, SHORT_REP), 0
    return header_events(ctx, ps, LONG_REP, dist) + length_events(OFF_REP_LEN, length, ps), 0


def nprobs(lc, lp):
    return OFF_LIT + (0x300 << (lc + lp))


def prices_rule(data, slab, lc, lp, pb):
    """the prices k_opt_walk + k_opt_prices derive from the parse on `slab`"""
    T = Oracle.cost_table().astype(np.int64)
    counts = np.zeros(2 * nprobs(lc, lp), dtype=np.int64)
    pos, ctx, reps = 0, 0, (0, 0, 0, 0)
    while pos < len(data):
        t, d, l = int(slab["type"][pos]), int(slab["dist"][pos]), int(slab["len"][pos])
        ev, _ = packet_events(data, lc, lp, pb, pos, ctx, reps, t, d, l)
        for c, b in ev:
            counts[2 * c + b] += 1
        ctx, reps = advance(ctx, reps, t, d)
        pos += l
    n0, n1 = counts[0::2], counts[1::2]
    p0 = np.clip((2048 * (n0 + 1)) // (n0 + n1 + 2), 1, 2047)
    out = np.zeros_like(counts)
    out[0::2], out[1::2] = T[p0], T[2048 - p0]
    return out.astype(np.uint32)


def candidates(data, cand, dict_limit):
    """per position: the MATCH sources of gs_best (mgl_index.hip), as greedy_rule in test_gpu_greedy.py takes them"""
    n = len(data)
    out = [[] for _ in range(n)]
    by2, by4 = {}, {}
    for p in range(n):
        if p + 1 < n:
            cs = list(reversed(by2.get(data[p:p + 2], [])))[:cand]
            if min(273, n - p) >= 4:
                cs += list(reversed(by4.get(data[p:p + 4], [])))[:cand]
            out[p] = [q for q in cs if p - q - 1 < dict_limit]
            by2.setdefault(data[p:p + 2], []).append(p)
        if p + 3 < n:
            by4.setdefault(data[p:p + 4], []).append(p)
    return out


def dp_rule(data, prices, cand, chunk, lc=0, lp=0, pb=0, dict_limit=0x400000):
    """The rule of k_opt_dp, chunk by chunk from the LZMA initial state: (unresolved slab as a list of
    (type, absolute distance, len) per position, objective)."""
    n = len(data)
    P = np.asarray(prices, dtype=np.int64)

    def price(ev, nd=0):
        return int(sum(P[2 * c + b] for c, b in ev)) + 2048 * nd

    @functools.lru_cache(maxsize=None)
    def lenp(base, ps):
        return np.array([price(length_events(base, l, ps)) for l in range(2, 274)], dtype=np.int64)

    @functools.lru_cache(maxsize=None)
    def hdr(ctx, ps, typ, rep):
        return price(header_events(ctx, ps, typ, rep))

    @functools.lru_cache(maxsize=None)
    def distp(v):
        return np.array([price(*dist_events(v, 2 + k)) for k in range(4)], dtype=np.int64)

    lc4 = np.minimum(np.arange(2, 274) - 2, 3)
    cands = candidates(data, cand, dict_limit)
    out = [(LIT, 0, 1)] * n
    objective = 0
    for s in range(0, n, chunk):
        e = min(s + chunk, n)
        tot = np.full(e - s + 1, INF, dtype=np.int64)
        tot[0] = 0
        edge = [None] * (e - s + 1)  # (type, x, len): x = rep index for LONG_REP, else absolute distance
        state = [None] * (e - s + 1)
        state[0] = (0, (0, 0, 0, 0))
        back = [None] * (e - s + 1)
        for i in range(s, e):
            k = i - s
            if k:
                t, x, l = edge[k]
                ctx, reps = state[k - l]
                back[k] = (t, reps[x] + 1 if t == LONG_REP else x, l)
                state[k] = advance(ctx, reps, t, x - 1 if t == MATCH else x)
            ctx, reps = state[k]
            cap = min(273, e - i)
            ps = i & ((1 << pb) - 1)
            rows = []  # (key, type, x, price per length 2..ml)
            if cap >= 2:
                for r in range(4):
                    D = reps[r] + 1
                    if D <= i:
                        ml = 0
                        while ml < cap and data[i - D + ml] == data[i + ml]:
                            ml += 1
                        if ml >= 2:
                            rows.append((r, LONG_REP, r, hdr(ctx, ps, LONG_REP, r) + lenp(OFF_REP_LEN, ps)[:ml - 1]))
                for q in cands[i]:
                    D = i - q
                    ml = 0
                    while ml < cap and data[q + ml] == data[i + ml]:
                        ml += 1
                    if ml >= 2:
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
                L = max(len(r[3]) for r in rows)
                M = np.full((len(rows), L), INF, dtype=np.int64)
                for j, r in enumerate(rows):
                    M[j, :len(r[3])] = r[3]
                w = np.argmin(M, axis=0)  # first minimum = smallest key
                best = M[w, np.arange(L)]
                cand_tot = tot[k] + best
                better = np.nonzero(cand_tot < tot[k + 2:k + 2 + L])[0]
                for li in better:
                    r = rows[w[li]]
                    tot[k + 2 + li] = cand_tot[li]
                    edge[k + 2 + li] = (r[1], r[2], li + 2)
        k = e - s
        t, x, l = edge[k]
        ctx, reps = state[k - l]
        back[k] = (t, reps[x] + 1 if t == LONG_REP else x, l)
        objective += int(tot[k])
        j = k
        while j > 0:
            t, D, l = back[j]
            j -= l
            out[s + j] = (t, D, l)
    return out, objective


def as_list(slab):
    return [(int(t), int(d), int(l)) for t, d, l in zip(slab["type"], slab["dist"], slab["len"])]


def greedy_slab(data, cand=8, **kw):
    sa = binding.SA(data, accept="single", neighbours_per_step=16, **kw)
    sa.seed_greedy(cand)
    cur, cost = sa.current()
    sa.close()
    return cur, cost


def _elf(n):
    return corpus.elf1m(1 << 16)[0][8192:8192 + n]


SMALL = [
    ("c1", corpus.lorem(4096)),
    ("prose", corpus.prose_like(6000, 0x51)),
    ("elf", _elf(8192)),
    ("runs", b"a" * 700 + b"ab" * 300 + bytes(range(256)) + b"a" * 50),
    ("n2", b"ab"),
    ("n1", b"x"),
]


@pytest.mark.parametrize("name,data", SMALL, ids=[s[0] for s in SMALL])
def test_prices_of_a_slab_match_the_rule(name, data):
    sa = binding.SA(data, accept="single", neighbours_per_step=16)
    g, _ = greedy_slab(data)
    assert np.array_equal(sa.optimal_prices(g), prices_rule(data, g, 0, 0, 0))
    lit = literal_slab(len(data))
    assert np.array_equal(sa.optimal_prices(lit), prices_rule(data, lit, 0, 0, 0))
    sa.close()


def _check_pass(data, prices, cand, chunk, dict_limit=0x400000):
    sa = binding.SA(data, accept="single", neighbours_per_step=16, dict_limit=dict_limit)
    before = sa.current()
    got, obj = sa.optimal_pass(prices, cand, chunk)
    want, want_obj = dp_rule(data, prices, cand, chunk, dict_limit=dict_limit)
    assert as_list(got) == want
    assert obj == want_obj
    after = sa.current()
    assert after[1] == before[1] and as_list(after[0]) == as_list(before[0])  # SA state untouched
    sa.close()
    return want


@pytest.mark.parametrize("cand,chunk", [(16, 1 << 16), (1, 1 << 16), (16, 1000)])
@pytest.mark.parametrize("name,data", SMALL, ids=[s[0] for s in SMALL])
def test_dp_pass_matches_the_rule_under_greedy_prices(name, data, cand, chunk):
    g, _ = greedy_slab(data)
    _check_pass(data, prices_rule(data, g, 0, 0, 0), cand, chunk)


@pytest.mark.parametrize("chunk", [1 << 16, 1000])
@pytest.mark.parametrize("name,data", SMALL, ids=[s[0] for s in SMALL])
def test_dp_pass_matches_the_rule_under_uniform_prices(name, data, chunk):
    prices = np.full(2 * nprobs(0, 0), 2048, dtype=np.uint32)
    _check_pass(data, prices, 8, chunk)


@pytest.mark.parametrize("name,data", SMALL[:4], ids=[s[0] for s in SMALL[:4]])
def test_dp_pass_matches_the_rule_under_a_window(name, data):
    g, _ = greedy_slab(data, dict_limit=300)
    got = _check_pass(data, prices_rule(data, g, 0, 0, 0), 16, 1000, dict_limit=300)
    assert all(t != MATCH or d - 1 < 300 for t, d, _ in got)


def test_dp_pass_rejects_bad_arguments():
    data = corpus.lorem(2048)
    sa = binding.SA(data, accept="single", neighbours_per_step=16)
    ok = np.full(2 * nprobs(0, 0), 2048, dtype=np.uint32)
    for prices, cand, chunk in ((ok[:-1], 8, 4096), (ok, 0, 4096), (ok, 31, 4096), (ok, 8, 511)):
        with pytest.raises(binding.MglError):
            sa.optimal_pass(prices, cand, chunk)
    sa.close()


def _check_seed(data, lc, lp, pb, dict_limit, **kw):
    sa = binding.SA(data, accept="single", neighbours_per_step=16, lc=lc, lp=lp, pb=pb, dict_limit=dict_limit)
    st = sa.seed_optimal(**kw)
    cur, cost = sa.current()
    assert cost == min(st["cost"]) == st["cost"][st["best_pass"]]
    o = Oracle(data, lc=lc, lp=lp, pb=pb, dict_limit=dict_limit)
    slab = np.ascontiguousarray(cur).astype(literal_slab(1).dtype)
    assert cost == o.cost_slab(slab)["total"]
    assert lzma.decompress(binding.emit_stream(data, cur, lc=lc, lp=lp, pb=pb), format=lzma.FORMAT_ALONE) == data
    assert all(t != MATCH or d < dict_limit for t, d, _ in as_list(cur))
    sa.close()
    return cur, cost, st


@pytest.mark.parametrize("dict_limit", [1000, 0x400000])
@pytest.mark.parametrize("lc,lp,pb", [(0, 0, 0), (3, 0, 2), (0, 2, 2)])
def test_seed_is_a_valid_exactly_costed_parse(lc, lp, pb, dict_limit):
    data = corpus.enwik_like(20000, 0x52)
    a, ca, st = _check_seed(data, lc, lp, pb, dict_limit, passes=3, chunk=4096)
    assert st["passes"] == 3 and len(st["ms"]) == 3
    b, cb, _ = _check_seed(data, lc, lp, pb, dict_limit, passes=3, chunk=4096)
    assert ca == cb and as_list(a) == as_list(b)


@pytest.mark.parametrize("data", [b"x", b"ab", b"a" * 3000], ids=["n1", "n2", "run"])
def test_seed_on_edge_inputs(data):
    _check_seed(data, 0, 0, 0, 0x400000)


def test_search_continues_from_the_optimal_seed_like_the_oracle():
    data = corpus.enwik_like(3000, 0x33)
    n, K, seed, steps = len(data), 64, 99, 40
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=seed, iters_per_epoch=steps)
    sa.seed_optimal(passes=2)
    cur, _ = sa.current()
    o = Oracle(data, dict_limit=0x400000)
    slab = np.ascontiguousarray(cur).astype(literal_slab(1).dtype)
    best = literal_slab(n)
    ref = o.sa_batched(slab, best, 0, 0, seed, K, 0, steps, 0, steps)
    for s in range(steps):
        st = sa.run(1)
        assert st["current_cost"] == int(ref["trace"][s, 3]), s
    got, got_cost = sa.current()
    assert got_cost == ref["cur"] and as_list(got) == as_list(slab)
    bst, best_cost = sa.best()
    assert best_cost == ref["best"] and as_list(bst) == as_list(best)
    sa.close()


# the seed's estimate over stdlib lzma -9e at the library's defaults, measured on one MI355X:
# c1 1.0105, c2 1.0179, c5_256k 1.0171; each gate is its ratio rounded up to the next 0.5 %
QUALITY = [
    ("c1", lambda: corpus.lorem(4096), 1.015),
    ("c2", lambda: corpus.config_input("c2")[0], 1.02),
    ("c5_256k", lambda: corpus.config_input("c5", 1 << 18)[0], 1.02),
]


@pytest.mark.parametrize("name,make,gate", QUALITY, ids=[q[0] for q in QUALITY])
def test_seed_quality(name, make, gate):
    data = make()
    sa = binding.SA(data, accept="single", neighbours_per_step=16)
    sa.seed_greedy(8)
    _, greedy_cost = sa.current()
    st = sa.seed_optimal()
    _, cost = sa.current()
    sa.close()
    assert cost < greedy_cost
    xz = len(lzma.compress(data, format=lzma.FORMAT_ALONE,
                           filters=[dict(id=lzma.FILTER_LZMA1, preset=9 | lzma.PRESET_EXTREME, lc=0, lp=0, pb=0,
                                         dict_size=1 << 22)]))
    est = 18 + cost / 16384
    print(f"{name}: optimal {est:.0f} B, greedy {18 + greedy_cost / 16384:.0f} B, lzma -9e {xz} B, ratio {est / xz:.4f}, "
          f"passes {st['cost']} ms {[round(m, 1) for m in st['ms']]}")
    assert est <= gate * xz


def test_cli_optimal_seed(tmp_path):
    data = corpus.enwik_like(5000, 0x35)
    f = tmp_path / "in.bin"
    f.write_bytes(data)
    out = tmp_path / "out.lzma"
    r = subprocess.run([build.CLI, "--optimal-seed", "3", "--epochs", "1", "--phases", "1", "--steps", "50", "-o", str(out), str(f)],
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-400:]
    assert lzma.decompress(out.read_bytes(), format=lzma.FORMAT_ALONE) == data
    r = subprocess.run([build.CLI, "--optimal-seed", "3", "--greedy-seed", "64", str(f)], capture_output=True, timeout=600)
    assert r.returncode != 0
