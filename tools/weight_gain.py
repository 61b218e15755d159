#!/usr/bin/env python3
"""What cost-weighted targets (mgl_sa_set_target_weights) gain and what they cost.

  python tools/weight_gain.py size [cfg=c2] [seeds=3]
      Estimated stream size of a fresh chain at the step counts of tools/size_at.py (3e4, 1e5, 3e5, 1e6 successful evaluations on
      c2 at K = 4096), same seeds, under three settings: no weights (tools/size_at.py's own numbers), cost:mean and cost:0 --
      the weights made again from the current slab's cost map every 25 steps (mgl_sa_weight_targets_by_cost).  Prints the means
      beside those of the reference's five seeds (tests/golden/reference_spread_c2.json) for c2.

  python tools/weight_gain.py steptime [cfg=c3] [blocks=8] [steps=25]
      On one handle, on an evolved slab (greedy seed, then 200 steps), alternating blocks of single steps with weights off and
      weights on (cost map plus the mean floor): the median ms per step of each, and the time of one
      mgl_sa_weight_targets_by_cost."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from megalania_amd import binding, corpus  # noqa: E402

REFRESH = 25


def size(cfg, seeds):
    K = {"c1": 1024, "c2": 4096, "c3": 16384}[cfg]
    marks = [8, 25, 74, 245] if cfg == "c2" else [62, 256]
    data, _ = corpus.config_input(cfg)
    n = len(data)
    table = {}
    for setting in ("none", "cost:mean", "cost:0"):
        rows = []
        for sd in range(seeds):
            sa = binding.SA(data, neighbours_per_step=K, seed=1673551 + 7919 * sd, iters_per_epoch=n, accept="auto")
            done, ev, row = 0, 0, []
            for m in marks:
                while done < m:
                    if setting != "none" and done % REFRESH == 0:
                        sa.weight_targets_by_cost(floor=sa.current()[1] // n if setting == "cost:mean" else 0)
                    take = min(m, (done // REFRESH + 1) * REFRESH) - done
                    st = sa.run(take)
                    done += take
                    ev += st["evaluations"]
                row.append((ev, 18 + st["best_cost"] / 16384))
            rows.append(row)
            sa.close()
        table[setting] = rows
        for i, m in enumerate(marks):
            v = [r[i][1] for r in rows]
            print(f"{cfg} K={K} weights {setting:9s} steps {m:4d} evaluations {rows[0][i][0]:8d}: mean {sum(v) / len(v):9.1f}  min {min(v):9.1f} max {max(v):9.1f}",
                  flush=True)
    if cfg == "c2":
        ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_spread_c2.json")))
        for i, it in enumerate([30000, 100000, 300000, 1000000]):
            v = [p["est_bytes"] for r in ref["runs"] for p in r["points"] if p["iterations"] == it]
            print(f"{cfg} reference, {len(v)} seeds, iterations {it:8d}: mean {sum(v) / len(v):9.1f}  min {min(v):9.1f} max {max(v):9.1f}")


def steptime(cfg, blocks, steps):
    K = {"c1": 1024, "c2": 4096, "c3": 16384}[cfg]
    data, _ = corpus.config_input(cfg)
    n = len(data)
    sa = binding.SA(data, neighbours_per_step=K, seed=1673551, iters_per_epoch=n, accept="auto")
    sa.seed_greedy(8)
    sa.run(200)
    sa.set_accept_mode("single")
    sa.run(30)
    per = {"off": [], "on": []}
    for b in range(2 * blocks):
        on = b % 2 == 1
        if on:
            t0 = time.perf_counter()
            total, map_ms = sa.weight_targets_by_cost(floor=sa.current()[1] // n)
            set_ms = (time.perf_counter() - t0) * 1e3
            print(f"{cfg} n={n} weight_targets_by_cost: {set_ms:.2f} ms wall, {map_ms:.2f} ms of it the map's kernels", flush=True)
        else:
            sa.set_target_weights(None)
        sa.run(3)  # the first step behind a change makes its targets itself, not ahead
        t0 = time.perf_counter()
        sa.run(steps)  # one call: every step's targets are made ahead, beside the accept of the step before, as in a long run
        per["on" if on else "off"].append((time.perf_counter() - t0) * 1e3 / steps)
    for k in ("off", "on"):
        v = per[k]
        print(f"{cfg} K={K} single steps, weights {k:3s}: median {statistics.median(v):.4f} ms/step  min {min(v):.4f}  max {max(v):.4f}  ({len(v)} blocks of {steps} steps)")
        print(f"  blocks {k}:", " ".join(f"{x:.4f}" for x in v))
    sa.close()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "size"
    if mode == "size":
        size(sys.argv[2] if len(sys.argv) > 2 else "c2", int(sys.argv[3]) if len(sys.argv) > 3 else 3)
    elif mode == "steptime":
        steptime(sys.argv[2] if len(sys.argv) > 2 else "c3", int(sys.argv[3]) if len(sys.argv) > 3 else 8, int(sys.argv[4]) if len(sys.argv) > 4 else 25)
    else:
        sys.exit(__doc__)
