"""The oracle's top-K search under the settings of mgl_sa_config that change what it returns -- the list size k,
the dictionary window (dict_limit) and the bucket scan cap (max_bucket_scan) -- against a brute force that
shares nothing with the oracle's search but its raw match-index query (orc_substrings of an unwindowed,
uncapped context) and its walk cost (orc_cost_slab).  The reference has no window and a fixed k = 20, so
nothing else pins these.  Also the argument checks of mgl_sa_create, which run before any device call.
No GPU needed."""
import ctypes as C

import numpy as np
import pytest

from _libs import LITERAL, LONG_REP, MATCH, SHORT_REP, Oracle, literal_slab, walk
from conftest import materialise, rand_bytes, slab_from_rle

BLOCK = 300  # planted block length: longer than the longest match (273)


def window_edge_input(D, n=None, seed=7):
    """Seeded random bytes with two planted 300-byte blocks: the copy at `near` repeats the bytes at distance
    exactly D - 1 (MATCH dist field D - 1: inside a window of D), the copy at `far` repeats other bytes at
    distance exactly D (outside).  Copies are made byte by byte, so a copy may overlap its source (D < 300)."""
    s1 = 64
    near = s1 + D
    s2 = s1 + BLOCK + 64 if D >= 2 * BLOCK + 128 else near + BLOCK + 64
    far = s2 + D + 1
    need = far + BLOCK + 64
    n = need if n is None else n
    assert n >= need
    b = bytearray(rand_bytes(n, seed + D))
    for src, dst in ((s1, near), (s2, far)):
        for i in range(BLOCK):
            b[dst + i] = b[src + i]
    return bytes(b), near, far


def evolve(data, steps=30, K=32, seed=11):
    """A slab the oracle's batched search evolved from the all-literal one (a base with matches and rep distances)."""
    o = Oracle(data)
    slab, best = literal_slab(len(data)), literal_slab(len(data))
    o.sa_batched(slab, best, 0, 0, seed, K, 0, steps * K, 0, steps)
    return slab


def seq_of(q, ln, kind):
    return ((q + 1) << 12) | (ln << 3) | kind


def brute_top_k(ob, data, slab, p, k, D, M):
    """The k best next packets at walk position p, pop order (worst first): every legal candidate priced by a
    full walk with the candidate at p, ordered canonically (cost ascending, then enumeration order descending).
    ob: an unwindowed, uncapped Oracle over data.  D: window (None = none).  M: scan cap (0 = none)."""
    n = len(data)
    offs, lens = ob.substrings(p)
    hits = {}
    for q, ln in zip(offs.tolist(), lens.tolist()):
        if D is None or p - q - 1 < D:
            hits[q] = max(hits.get(q, 0), ln)
    qs = sorted(hits)
    if M:
        qs = qs[-M:]  # the nearest M distinct hit positions
    pre = slab.copy()
    pre[p:] = literal_slab(n - p)  # literals do not touch the rep distances: the final state's are those at p
    dists = [int(x) for x in ob.cost_slab(pre)["dists"]]
    cands = [((LITERAL, 0, 1), 0)]
    if p > 0 and p - dists[0] - 1 >= 0 and data[p] == data[p - dists[0] - 1]:
        cands.append(((SHORT_REP, 0, 1), 1))
    for q in qs:
        dist = p - q - 1
        for ln in range(2, hits[q] + 1):
            cands.append(((MATCH, dist, ln), seq_of(q, ln, 0)))
            for i in range(4):
                if dist == dists[i]:
                    cands.append(((LONG_REP, i, ln), seq_of(q, ln, 1 + i)))
    inc = (int(slab[p]["type"]), int(slab[p]["dist"]), int(slab[p]["len"]))
    w = len([x for x in walk(slab) if x < p])  # walk index of the packet at p
    scored = []
    for pk, seq in cands:
        if pk == inc:
            continue  # top_k_packet_finder.c:99-101
        s = pre.copy()
        s[p] = pk
        cum = ob.cost_slab(s)["cum"]
        perp = int(cum[w]) - (int(cum[w - 1]) if w else 0)
        scored.append((perp // pk[2], -seq, pk))
    scored.sort()
    best = scored[:k]
    return [b[2] for b in reversed(best)], [b[0] for b in reversed(best)]


def as_list(pk):
    return [(int(p["type"]), int(p["dist"]), int(p["len"])) for p in pk]


def candidate_count(ob, p, D, M):
    offs, _ = ob.substrings(p)
    if D is not None:
        offs = offs[p - offs.astype(np.int64) - 1 < D]
    if M and len(offs):
        keep = np.unique(offs)[-M:]
        offs = offs[np.isin(offs, keep)]
    return len(offs)


def positions(ob, slab, D, M, count, extra=(), cap=2500, seed=3):
    """up to `count` walk positions whose candidate count under (D, M) stays at most `cap`, plus `extra` (kept
    when on the walk); the nearest positions to the end, the start and the window edge are always kept."""
    w = walk(slab)
    on = set(w)
    rng = np.random.default_rng(seed)
    pool = [p for p in w if p > 0]
    pick = [w[0], w[-1]] + [p for p in extra if p in on]
    if D is not None:
        pick += [p for p in pool if D - 2 <= p <= D + 2]
    for p in rng.permutation(pool)[: 4 * count].tolist():
        if len(pick) >= count + len(extra) + 7:
            break
        pick.append(p)
    return sorted({p for p in pick if candidate_count(ob, p, D, M) <= cap})


_INPUTS = {}


def inputs():
    """name -> (data, [(slab kind, slab)], planted positions)"""
    if not _INPUTS:
        import json
        import os

        with open(os.path.join(os.path.dirname(__file__), "golden", "reference_vectors.json")) as f:
            g = json.load(f)
        for name in ("lorem4k", "zeros600", "reps"):
            data = materialise(g["inputs"][name])
            ev = slab_from_rle(len(data), g["evolved_walks"][name]) if name in g["evolved_walks"] else evolve(data)
            _INPUTS[name] = (data, [("literal", literal_slab(len(data))), ("evolved", ev)], ())
        data = b"ab" * 700
        _INPUTS["ab1400"] = (data, [("literal", literal_slab(len(data))), ("evolved", evolve(data))], ())
        for D in (256, 4096):
            data, near, far = window_edge_input(D)
            planted = tuple(p + d for p in (near, far) for d in (-2, -1, 0, 1, 2))
            _INPUTS[f"edge{D}"] = (data, [("literal", literal_slab(len(data))), ("evolved", evolve(data, steps=12))], planted)
    return _INPUTS


# every value of each axis against the defaults of the others (k 20, no window, no cap), and the combinations
# the device tests use (tests/test_gpu_search_config.py)
DEFAULT = (20, None, 0)
GRID = sorted({(k, None, 0) for k in (1, 2, 20, 32)} | {(20, D, 0) for D in (1, 2, 3, 255, 256, 257, 4096, None)}
              | {(20, None, M) for M in (0, 1, 63, 64, 65)}
              | {(1, 256, 64), (2, 2, 1), (32, 4096, 65), (32, 1024, 64), (1, 255, 1), (32, 257, 63)},
              key=lambda s: (s[0], -1 if s[1] is None else s[1], s[2]))


def _sid(s):
    return f"k{s[0]}-D{'none' if s[1] is None else s[1]}-M{s[2]}"


@pytest.mark.parametrize("setting", GRID, ids=[_sid(s) for s in GRID])
def test_top_k_equals_brute_force(setting):
    k, D, M = setting
    checked = 0
    for name, (data, slabs, planted) in inputs().items():
        ob = Oracle(data)
        o = Oracle(data, dict_limit=D or 0, max_bucket_scan=M)
        for kind, slab in slabs:
            # inside zeros600 every earlier position is a hit of every length: only a small cap keeps it brute-forceable
            cnt = 4 if name == "zeros600" and not (M and M <= 65) else 6
            for p in positions(ob, slab, D, M, cnt, extra=planted):
                want_pk, want_c = brute_top_k(ob, data, slab, p, k, D, M)
                pk, costs = o.top_k(slab, p, mode=1, k=k)
                assert (as_list(pk), [int(c) for c in costs]) == (want_pk, want_c), (name, kind, p)
                checked += 1
    assert checked >= 40


@pytest.mark.parametrize("D", [256, 4096])
def test_window_edge_is_where_the_planted_copies_say(D):
    """The window-edge inputs do what the device tests rely on: at the near copy the top-K list (any k) holds
    the 273-byte MATCH at distance D - 1; at the far copy no MATCH reaches distance D, while without a window
    the 273-byte MATCH at distance D is there."""
    data, near, far = window_edge_input(D)
    slab = literal_slab(len(data))
    o = Oracle(data, dict_limit=D)
    for k in (1, 2, 20, 32):
        pk, _ = o.top_k(slab, near, mode=1, k=k)
        assert (MATCH, D - 1, 273) in as_list(pk), k
        pk, _ = o.top_k(slab, far, mode=1, k=k)
        assert all(t != MATCH or d < D for t, d, _ in as_list(pk)), k
    pk, _ = Oracle(data).top_k(slab, far, mode=1, k=1)
    assert as_list(pk) == [(MATCH, D, 273)]


def test_pick_draws_from_the_set_top_k():
    """orc_set_top_k reaches the neighbour generator: 20 is the default, and a list of 1 changes what the picks of
    a step produce."""
    data = materialise({"gen": "lorem", "n": 4096})
    base = literal_slab(len(data))
    seed, K = 99, 64
    o20, o1 = Oracle(data, top_k=20), Oracle(data, top_k=1)
    dflt = Oracle(data)
    differ = 0
    for j in range(K):
        r20 = o20.neighbour(base, seed, 3, j, K=K)
        assert r20[:2] == dflt.neighbour(base, seed, 3, j, K=K)[:2], j  # the default is 20
        r1 = o1.neighbour(base, seed, 3, j, K=K)
        differ += r1[1] != r20[1]
    assert differ > 0


def _create(props, top_k=20, data=b"abcabcabc"):
    from megalania_amd import binding

    L = binding.hip_lib()
    buf = np.frombuffer(data, dtype=np.uint8).copy()
    cfg = binding.Config(1, 8, top_k, 0, 0, 0, 0, 0)
    h = L.mgl_sa_create(buf.ctypes.data_as(C.c_void_p), len(buf), binding.Properties(*props), C.byref(cfg))
    return h, L.mgl_last_error().decode()


@pytest.mark.parametrize("props,top_k", [((0, 0, 0), 33), ((3, 2, 0), 20), ((0, 0, 5), 20), ((9, 0, 0), 20),
                                         ((0, 0, 0), 1 << 31)], ids=["top_k33", "lc_lp5", "pb5", "lc9", "top_k_huge"])
def test_sa_create_refuses_unsupported_settings(props, top_k):
    """mgl_sa_create checks these before it touches a device: NULL and an error text, with or without a GPU."""
    h, err = _create(props, top_k)
    assert not h and err, (h, err)
    assert "top_k" in err if top_k > 32 else "lc/lp/pb" in err
