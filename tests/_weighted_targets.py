"""The weighted target rule (include/megalania_hip.h: mgl_sa_set_target_weights; csrc/mgl_weights.hip) restated in Python integers
and numpy, shared by the CPU and GPU tests.  The two draws of a neighbour's stream come from mgl_rng_draw_at."""
import numpy as np

DRAW2 = 0xFFFFFFFF  # the stream index of the value's second draw
MAX_TOTAL = 1 << 44


def value(L, W, K, j, seed, step):
    """(v, a, b): the value neighbour j of K draws from W, and its slice [a, b)"""
    a, b = j * W // K, (j + 1) * W // K
    u = (int(L.mgl_rng_draw_at(seed, step, j, 0)) << 31) | int(L.mgl_rng_draw_at(seed, step, j, DRAW2))
    return a + (u % (b - a) if b > a else 0), a, b


def ordinal_targets(L, starts, lo, hi, seed, step, K):
    """the rule without weights, under window [lo, hi): what tests/test_gpu_focus.py restates"""
    a, b = int(np.searchsorted(starts, lo, side="left")), int(np.searchsorted(starts, hi, side="left"))
    if b == a:
        a -= 1
    cnt = b - a
    out = []
    for j in range(K):
        o0, o1 = j * cnt // K, (j + 1) * cnt // K
        u = int(L.mgl_rng_draw_at(seed, step, j, 0))
        out.append(int(starts[a + o0 + (u % (o1 - o0) if o1 > o0 else 0)]))
    return out


def target_of_byte(starts, x, lo, hi):
    """the start of the packet that covers x; below lo: the first start inside [lo, hi), if the window holds one"""
    t = int(starts[np.searchsorted(starts, x, side="right") - 1])
    if t < lo:
        i = int(np.searchsorted(starts, lo, side="left"))
        if i < len(starts) and int(starts[i]) < hi:
            t = int(starts[i])
    return t


def targets(L, w, starts, window, seed, step, K, info=None):
    """The K targets of a step.  w: n weights; starts: the walk's packet starts, ascending; window: (lo, hi) or None.
    info (a dict, optional) collects what the cases met: 'empty_slice', 'wide_slice', 'earlier_word', 'below_lo'."""
    n = len(w)
    lo, hi = window if window else (0, n)
    starts = np.asarray(starts)
    S = np.concatenate(([0], np.cumsum(np.asarray(w, dtype=np.uint64), dtype=np.uint64)))  # exact: the sum is below 2^44
    s_lo = int(S[lo])
    W = int(S[hi]) - s_lo
    if W == 0:
        return ordinal_targets(L, starts, lo, hi, seed, step, K)
    out = []
    for j in range(K):
        v, a, b = value(L, W, K, j, seed, step)
        x = int(np.searchsorted(S, np.uint64(s_lo + v), side="right")) - 1  # S[x] <= S[lo] + v < S[x + 1]
        assert lo <= x < hi and int(w[x]) != 0
        t = target_of_byte(starts, x, lo, hi)
        if info is not None:
            info["empty_slice"] = info.get("empty_slice", False) or b == a
            info["wide_slice"] = info.get("wide_slice", False) or b - a > 1 << 31
            cover = int(starts[np.searchsorted(starts, x, side="right") - 1])
            info["earlier_word"] = info.get("earlier_word", False) or (cover >> 6) < (x >> 6)
            info["below_lo"] = info.get("below_lo", False) or cover < lo
        out.append(t)
    return out


def brute_targets(L, w, starts, window, seed, step, K):
    """the same by the definition, position by position: for tiny cases"""
    n = len(w)
    lo, hi = window if window else (0, n)
    on = sorted(int(s) for s in starts)
    W = sum(int(w[x]) for x in range(lo, hi))
    if W == 0:
        inside = [s for s in on if lo <= s < hi] or [max(s for s in on if s <= lo)]
        out = []
        for j in range(K):
            o0, o1 = j * len(inside) // K, (j + 1) * len(inside) // K
            u = int(L.mgl_rng_draw_at(seed, step, j, 0))
            out.append(inside[o0 + (u % (o1 - o0) if o1 > o0 else 0)])
        return out
    out = []
    for j in range(K):
        v, _, _ = value(L, W, K, j, seed, step)
        acc, x = 0, None
        for p in range(lo, hi):
            if acc <= v < acc + int(w[p]):
                x = p
                break
            acc += int(w[p])
        t = max(s for s in on if s <= x)
        if t < lo:
            inside = [s for s in on if lo <= s < hi]
            if inside:
                t = inside[0]
        out.append(t)
    return out
