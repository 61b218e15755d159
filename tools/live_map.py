#!/usr/bin/env python3
"""What the live cost map (mgl_cost_map_live) and live target weights (mgl_sa_set_live_weights) cost and gain
(DESIGN.md section 10).

  python tools/live_map.py time [cfg ...=c2 c5 c3]
      Device time of the live map against the serial walk (mgl_cost_map) on the same current slab -- the parse of stdlib lzma
      at 0/0/0, preset 9e for c2 and c5, preset 6 for c3, as in the cost map's own measurements --: 3 warm-up calls, then the
      median, min and max of 10.  Then, on the slab 60 AUTO steps later, the device time of one refresh of the live weights
      (map, weights, prefix sums) against the 25 steps between two refreshes: single steps with live weights every 25.

  python tools/live_map.py size [cfg=c2] [seeds=3]
      tools/weight_gain.py's table (same seeds, same step marks) with the weights refreshed inside the run:
      live 25:0, live 25:0,single, the smaller intervals live 5:0 and live 1:0, and live 5:0 switched on by the caller at
      the second and the third mark, beside none."""
import lzma
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from megalania_amd import binding, corpus  # noqa: E402

K_OF = {"c1": 1024, "c2": 4096, "c3": 16384, "c5": 4096}


def xz_parse(data, preset):
    stream = lzma.compress(data, format=lzma.FORMAT_ALONE, filters=[dict(id=lzma.FILTER_LZMA1, preset=preset, dict_size=1 << 22, lc=0, lp=0, pb=0)])
    return binding.stream_import(stream, data)[0]


def med(v):
    return f"median {statistics.median(v):9.3f} ms  min {min(v):9.3f}  max {max(v):9.3f}  ({len(v)} calls)"


def timing(cfg):
    data, what = corpus.config_input(cfg)
    n, K = len(data), K_OF[cfg]
    sa = binding.SA(data, neighbours_per_step=K, seed=1673551, iters_per_epoch=n, accept="auto")
    sa.set_slab(xz_parse(data, 6 if cfg == "c3" else 9 | lzma.PRESET_EXTREME))
    pool = int(sa.debug_dump(binding.DUMP.CHAIN_LEN).astype("u8").sum())
    print(f"{cfg} n={n} ({what}): chains hold {pool} events, {pool / n:.1f} per byte", flush=True)
    walk, live = [], []
    for i in range(13):
        rep = sa.cost_map_live()[1]
        if i >= 3:
            live.append(rep["gpu_ms"])
    for i in range(5 if cfg == "c3" else 13):
        rep_w = sa.cost_map()[1]
        if i >= (1 if cfg == "c3" else 3):
            walk.append(rep_w["gpu_ms"])
    assert {k: v for k, v in rep.items() if k != "gpu_ms"} == {k: v for k, v in rep_w.items() if k != "gpu_ms"}
    print(f"{cfg} mgl_cost_map      (serial walk): {med(walk)}")
    print(f"{cfg} mgl_cost_map_live (chains)     : {med(live)}  x{statistics.median(walk) / statistics.median(live):.1f}", flush=True)
    # the refresh against the steps between two refreshes
    sa.run(60)
    sa.set_accept_mode("single")
    sa.run(30)
    off, on, ms, refreshes = [], [], 0.0, 0
    for b in range(12):  # alternating blocks on one handle, as tools/weight_gain.py steptime
        live = b % 2 == 1
        sa.set_live_weights(25 if live else None)
        sa.run(5)  # settle: the first steps behind a change make their targets themselves
        t0 = time.perf_counter()
        sa.run(50)  # two refreshes fall into it when live
        (on if live else off).append((time.perf_counter() - t0) * 1e3 / 50)
        if live:
            lw = sa.live_weights()
            ms, refreshes = ms + lw["gpu_ms"], refreshes + lw["refreshes"]
    print(f"{cfg} K={K} single steps, wall clock, blocks of 50: {med(off)} per step without weights")
    print(f"{cfg} K={K} single steps, wall clock, blocks of 50: {med(on)} per step with live 25:0, refreshes included")
    print(f"{cfg} one refresh: {ms / refreshes:.3f} ms of device time (mean of {refreshes}) against {25 * statistics.median(off):.2f} ms for 25 steps", flush=True)
    sa.close()


def size(cfg, seeds):
    K = K_OF[cfg]
    marks = [8, 25, 74, 245] if cfg == "c2" else [62, 256]
    data, _ = corpus.config_input(cfg)
    n = len(data)
    # (setting, configuration, the step from which it is on)
    for setting, live, start in (("none", None, 0), ("live 25:0", dict(every=25), 0), ("live 25:0,single", dict(every=25, single_only=True), 0),
                                 ("live 5:0", dict(every=5), 0), ("live 1:0", dict(every=1), 0),
                                 ("live 5:0 from 25", dict(every=5), marks[1]), ("live 5:0 from 74", dict(every=5), marks[2])):
        rows = []
        for sd in range(seeds):
            sa = binding.SA(data, neighbours_per_step=K, seed=1673551 + 7919 * sd, iters_per_epoch=n, accept="auto")
            done, ev, row = 0, 0, []
            for m in marks:
                if live and done == start:
                    sa.set_live_weights(**live)
                st = sa.run(m - done)
                done = m
                ev += st["evaluations"]
                row.append((ev, 18 + st["best_cost"] / 16384))
            lw = sa.live_weights()
            rows.append(row)
            sa.close()
        for i, m in enumerate(marks):
            v = [r[i][1] for r in rows]
            print(f"{cfg} K={K} weights {setting:17s} steps {m:4d} evaluations {rows[0][i][0]:8d}: mean {sum(v) / len(v):9.1f}  min {min(v):9.1f} max {max(v):9.1f}", flush=True)
        if live:
            print(f"   last seed: {lw['refreshes']} refreshes, {lw['gpu_ms']:.2f} ms of device time in all")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "time":
        for cfg in sys.argv[2:] or ["c2", "c5", "c3"]:
            timing(cfg)
    elif mode == "size":
        size(sys.argv[2] if len(sys.argv) > 2 else "c2", int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    else:
        sys.exit(__doc__)
