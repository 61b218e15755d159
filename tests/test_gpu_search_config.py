"""The device's top-K search against the oracle across the settings of mgl_sa_config that change what it returns:
top_k (1..32), the dictionary window (dict_limit) and the bucket scan cap (max_bucket_scan).  Every other GPU test
runs at top_k 20 with a window larger than its input; here the window cuts through the inputs, at its edge
(copies planted at distance D - 1 and D) and at the production size of 4 MiB.  Both forms of topk_find
(mgl_topk.hip) are reached, each directly and through an engine: the batched W = 4 form by probe form 0 and the
split pick, the in-place W = 1 form by probe form 1, the full-walk engine and the one-kernel form.
The oracle's own handling of these settings is pinned by a brute force in tests/test_oracle_search_config.py.
`-m gpu`."""
import lzma
import time

import numpy as np
import pytest

from _libs import MATCH, Oracle, literal_slab, walk
from megalania_amd import binding, corpus
from test_gpu_parity import _check_neighbours
from test_oracle_search_config import GRID, _sid, as_list, evolve, window_edge_input

pytestmark = pytest.mark.gpu

PROD_WINDOW = 0x400000


def P(slab):
    return np.ascontiguousarray(slab).astype(binding.PACKET)


def device_window(D):
    return PROD_WINDOW if D is None else D


_INPUTS = {}


def grid_inputs(D):
    """name -> (data, [(slab kind, slab)], planted positions): the brute force's inputs, plus a window-edge input
    for the setting's own window"""
    if "base" not in _INPUTS:
        from conftest import materialise, slab_from_rle
        import json
        import os

        with open(os.path.join(os.path.dirname(__file__), "golden", "reference_vectors.json")) as f:
            g = json.load(f)
        base = {}
        for name in ("lorem4k", "zeros600", "reps"):
            data = materialise(g["inputs"][name])
            ev = slab_from_rle(len(data), g["evolved_walks"][name]) if name in g["evolved_walks"] else evolve(data)
            base[name] = (data, [("literal", literal_slab(len(data))), ("evolved", ev)], ())
        data = b"ab" * 700
        base["ab1400"] = (data, [("literal", literal_slab(len(data))), ("evolved", evolve(data))], ())
        for E in (256, 4096):
            base[f"edge{E}"] = edge_case(E)
        _INPUTS["base"] = base
    out = dict(_INPUTS["base"])
    if D is not None and f"edge{D}" not in out:
        if D not in _INPUTS:
            _INPUTS[D] = edge_case(D)
        out[f"edge{D}"] = _INPUTS[D]
    return out


def edge_case(D):
    data, near, far = window_edge_input(D)
    planted = tuple(p + d for p in (near, far) for d in (-2, -1, 0, 1, 2))
    return data, [("literal", literal_slab(len(data))), ("evolved", evolve(data, steps=12))], planted, near, far


def check_window_edge(pk_near, pk_far, D, M, o_unwindowed, near):
    """non-vacuity at the planted copies: inside the window the 273-byte MATCH at distance D - 1 is in the list
    (when the scan cap leaves its hit in the scan); no MATCH at distance D or beyond ever is"""
    assert all(t != MATCH or d < D for t, d, _ in as_list(pk_far)), as_list(pk_far)
    if D >= 255:
        offs, _ = o_unwindowed.substrings(near)
        inside = {int(q) for q in offs if near - int(q) - 1 < D}
        if M == 0 or len(inside) <= M:
            assert (MATCH, D - 1, 273) in as_list(pk_near), as_list(pk_near)


@pytest.mark.parametrize("setting", GRID, ids=[_sid(s) for s in GRID])
def test_top_k_probe_vs_oracle_across_settings(setting):
    """(a) mgl_top_k in both probe forms (topk_find<4, true> with a plan, topk_find<1> in place) == one answer of
    Oracle.top_k(mode=1, k): packets and costs, at every position of the planted copies +-2 and about 200 walk
    positions per input."""
    k, D, M = setting
    rng = np.random.default_rng(k * 1000003 + (D or 0) * 101 + M)
    calls, t_dev = 0, 0.0
    for name, case in grid_inputs(D).items():
        data, slabs, planted = case[:3]
        sa = binding.SA(data, neighbours_per_step=8, top_k=k, dict_limit=device_window(D), max_bucket_scan=M)
        o = Oracle(data, dict_limit=D or 0, max_bucket_scan=M)
        for kind, slab in slabs:
            w = walk(slab)
            on = set(w)
            ps = sorted(set(rng.choice(w, size=min(100, len(w)), replace=False).tolist()) | {w[-1]}
                        | {p for p in planted if p in on})
            dslab = P(slab)
            for p in ps:
                opk, ocosts = o.top_k(slab, p, mode=1, k=k)
                assert len(opk) <= k
                for form in (1, 0):  # the handle is left on the default form
                    t0 = time.perf_counter()
                    pk, costs = sa.top_k(dslab, p, form=form)
                    t_dev += time.perf_counter() - t0
                    calls += 1
                    assert (as_list(pk), [int(c) for c in costs]) == (as_list(opk), [int(c) for c in ocosts]), (name, kind, p, form)
            if kind == "literal" and len(case) == 5 and name == f"edge{D}":
                near, far = case[3], case[4]
                check_window_edge(sa.top_k(dslab, near)[0], sa.top_k(dslab, far)[0], D, M, Oracle(data), near)
        sa.close()
    print(f"mgl_top_k: {calls} calls, {1e3 * t_dev / calls:.3f} ms per call")


def test_window_edge_cases_are_not_vacuous():
    """the near copy's MATCH at D - 1 shows up through the device at every k of the grid"""
    for D in (256, 4096):
        data, slabs, planted, near, far = edge_case(D)
        for k in (1, 2, 20, 32):
            sa = binding.SA(data, neighbours_per_step=8, top_k=k, dict_limit=D)
            slab = P(slabs[0][1])
            check_window_edge(sa.top_k(slab, near)[0], sa.top_k(slab, far)[0], D, 0, Oracle(data), near)
            sa.close()


NB_SETTINGS = [(1, None, 0), (2, None, 0), (32, None, 0), (20, 2, 0), (20, 256, 0), (20, 4096, 0),
               (20, None, 1), (20, None, 64), (20, None, 65), (32, 256, 65)]
NB_ENGINES = ["split", "one_kernel", "fullwalk"]


@pytest.mark.parametrize("engine", NB_ENGINES)
@pytest.mark.parametrize("setting", NB_SETTINGS, ids=[_sid(s) for s in NB_SETTINGS])
def test_neighbours_vs_oracle_across_settings(setting, engine, monkeypatch):
    """(b) every neighbour of a step == the oracle, cost and journal, from the literal slab and from a slab the
    device evolved under the same settings; split pick (topk_find<4, true>), one-kernel form and full walk (topk_find<1>)."""
    k, D, M = setting
    if engine == "one_kernel":
        monkeypatch.setenv("MGL_NO_SPLIT", "1")
    data = corpus.enwik_like(6000, 0x5C)
    n, K, seed = len(data), 64, 41
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=seed, top_k=k, dict_limit=device_window(D),
                    max_bucket_scan=M, fullwalk=engine == "fullwalk")
    o = Oracle(data, dict_limit=D or 0, max_bucket_scan=M, top_k=k)
    base = literal_slab(n)
    sa.set_slab(P(base))
    for step in (0, 5):
        _check_neighbours(sa, o, base, seed, step, K)
    sa.run(30)
    cur, cost = sa.current()
    evolved = cur.astype(base.dtype)
    if D is None or D >= 256:
        assert len(walk(evolved)) < n - 200  # the base carries matches (a window of 2 leaves next to none to take)
    assert cost == o.cost_slab(evolved)["total"]
    for step in (30, 31):
        _check_neighbours(sa, o, evolved, seed, step, K)
    sa.close()


def test_top_k_zero_means_twenty():
    data = corpus.enwik_like(6000, 0x5C)
    K, seed = 64, 41
    a = binding.SA(data, neighbours_per_step=K, seed=seed, top_k=0)
    b = binding.SA(data, neighbours_per_step=K, seed=seed, top_k=20)
    slab = P(literal_slab(len(data)))
    for step in (0, 9):
        assert (a.neighbours(step, want_diffs=False)[0] == b.neighbours(step, want_diffs=False)[0]).all(), step
    full = 0
    for p in (1, 100, 2999, 5000):
        pa, ca = a.top_k(slab, p)
        pb, cb = b.top_k(slab, p)
        assert as_list(pa) == as_list(pb) and list(ca) == list(cb) and len(pa) <= 20, p
        full += len(pa) == 20
    assert full >= 2  # lists of 20 where the position offers more candidates
    a.close()
    b.close()


TRAJ = [(1, None, 0), (32, 1024, 64)]


@pytest.mark.parametrize("accept", ["single", "bulk"])
@pytest.mark.parametrize("setting", TRAJ, ids=[_sid(s) for s in TRAJ])
def test_sa_run_trajectory_vs_oracle_across_settings(setting, accept):
    """(c) mgl_sa_run against orc_sa_batched step by step under the setting: current cost, accepted count, final
    slabs; the final slab is accepted by a second handle with the same settings and its stream decodes."""
    k, D, M = setting
    data = corpus.lorem(1800)
    n = len(data)
    K, seed, steps = 48, 1673551, 60
    ipe = steps * K
    kw = dict(neighbours_per_step=K, seed=seed, iters_per_epoch=ipe, top_k=k, dict_limit=device_window(D),
              max_bucket_scan=M)
    sa = binding.SA(data, accept=accept, **kw)
    o = Oracle(data, dict_limit=D or 0, max_bucket_scan=M, top_k=k)
    slab, best = literal_slab(n), literal_slab(n)
    modes = np.full(steps, 1 if accept == "bulk" else 0, dtype=np.uint8)
    ref = o.sa_batched(slab, best, 0, 0, seed, K, 0, ipe, 0, steps, modes=modes)
    evals = 0
    for s in range(steps):
        st = sa.run(1)
        evals += st["evaluations"]
        assert st["current_cost"] == int(ref["trace"][s, 3]), s
        assert st["accepted"] == int(ref["trace"][s, 1]), s
    assert evals == ref["valid"]
    assert int(ref["trace"][:, 1].sum()) > 10
    cur, cur_cost = sa.current()
    bst, best_cost = sa.best()
    assert cur_cost == ref["cur"] and best_cost == ref["best"]
    assert as_list(cur) == as_list(slab) and as_list(bst) == as_list(best)
    if D is not None:
        assert all(t != MATCH or d < D for t, d, _ in as_list(cur))
    sa2 = binding.SA(data, **kw)
    sa2.set_slab(cur)
    assert sa2.current()[1] == cur_cost
    sa2.close()
    assert lzma.decompress(binding.emit_stream(data, bst), format=lzma.FORMAT_ALONE) == data
    sa.close()


def test_production_window_at_full_scale():
    """(d) the default window of 4 MiB on an input just past it: copies planted at distance 0x3FFFFF (inside) and
    0x400000 (outside).  mgl_top_k == oracle at the copies; set_slab takes the MATCH at 0x3FFFFF with the oracle's
    cost and refuses the one at 0x400000; every neighbour of one step of that slab == the oracle."""
    D = PROD_WINDOW
    data, near, far = window_edge_input(D, D + 8192)
    n, K, seed = len(data), 64, 23
    sa = binding.SA(data, accept="single", neighbours_per_step=K, seed=seed)  # dict_limit 0: the production window
    o = Oracle(data, dict_limit=D)
    lit = literal_slab(n)
    dlit = P(lit)
    got = {}
    for p in [near + d for d in range(-2, 3)] + [far + d for d in range(-2, 3)]:
        pk, costs = sa.top_k(dlit, p)
        opk, ocosts = o.top_k(lit, p, mode=1, k=20)
        assert (as_list(pk), [int(c) for c in costs]) == (as_list(opk), [int(c) for c in ocosts]), p
        got[p] = pk
    check_window_edge(got[near], got[far], D, 0, Oracle(data), near)
    inside = lit.copy()
    inside[near] = (MATCH, D - 1, 273)
    sa.set_slab(P(inside))
    assert sa.current()[1] == o.cost_slab(inside)["total"]
    outside = lit.copy()
    outside[far] = (MATCH, D, 273)
    sa2 = binding.SA(data, accept="single", neighbours_per_step=K, seed=seed)
    with pytest.raises(binding.MglError):
        sa2.set_slab(P(outside))
    sa2.close()
    _check_neighbours(sa, o, inside, seed, 0, K)
    sa.close()
