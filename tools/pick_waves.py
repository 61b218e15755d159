#!/usr/bin/env python3
"""Diagnostic: where a picking wavefront of the pick half (k_neighbours2<false, MGL_NBR_PICK>) spends its cycles on an
evolved slab (MGL_F_PROFILE): the lifetime percentiles of the wavefronts that pick, and each stage's share of the
summed lifetime.  The stages are enum PickStage (mgl_topk.hip).
   python tools/pick_waves.py c3 [single steps measured]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from megalania_amd import binding, corpus
cfg = sys.argv[1] if len(sys.argv) > 1 else "c3"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 8
K = {"c1": 1024, "c2": 4096, "c3": 16384, "c4": 16384, "c5": 4096}[cfg]
STAGES = ["target, state, mutate decision", "plan: batched set-up of all sources", "model load + replay",
          "price tables, literal, short rep", "set-up in place (bounds, ranks, runs, searches)", "rep pass",
          "scan 16-byte source", "scan 8-byte source", "scan D=7", "scan D=6", "scan D=5", "scan D=4", "scan D=3",
          "scan D=2 (bucket)", "draw + record", "-"]
data, desc = corpus.config_input(cfg)
props = dict(pb=2, max_bucket_scan=4096) if cfg == "c5" else {}
sa = binding.SA(data, neighbours_per_step=K, timing=True, iters_per_epoch=len(data), flags=binding.F_PROFILE, **props)
done = 0
while done < 6000:
    p = sa.run(128); done += p["steps"]
    if p["bulk_steps"] == 0: break
sa.set_accept_mode("single")
sa.run(8)


def dump():
    raw = sa.debug_dump(binding.DUMP.PHASE_CYCLES)
    return raw[32 + K:64 + K].astype(np.float64), raw[64 + K:64 + 2 * K].copy()


life, ms = [], []
acc0, last = dump()
for rep in range(reps):
    st = sa.run(1)
    acc, cur = dump()
    life.append(cur[cur != last].astype(np.float64))  # the wavefronts that picked in this step wrote theirs anew
    last = cur
    ms.append(st["gpu_ms_neighbours"])
life = np.concatenate(life)
cyc, cnt = (acc - acc0)[:16], (acc - acc0)[16:]
total = cyc.sum()
print(f"# {cfg}: after {done} steps, {reps} single steps, {len(life)} picking wavefronts of {reps * K} neighbours; neighbour kernels {np.mean(ms) * 1000:.0f} us per step")
print("lifetime of a picking wavefront, cycles: " + "  ".join(f"p{q}={np.percentile(life, q):.0f}" for q in (10, 50, 90, 99, 100)) + f"  mean={life.mean():.0f}")
print(f"{'stage':50s} {'share':>7s} {'cycles per picking wavefront':>30s} {'visits per wavefront':>22s}")
for i, name in enumerate(STAGES):
    if cnt[i] == 0: continue
    print(f"{name:50s} {100 * cyc[i] / total:6.1f}% {cyc[i] / len(life):30.0f} {cnt[i] / len(life):22.2f}")
setup = cyc[1] + cyc[4]
print(f"set-up of the sources (plan + in place): {100 * setup / total:.1f}% of a picking wavefront's lifetime, {setup / len(life):.0f} cycles")
sa.close()
