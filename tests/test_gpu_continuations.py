"""The continuation record: a walk half that meets a repair pick saves its walk (state, journal, change lists) and the second
pass takes it up at that pick; with MGL_NO_CONT=1 the second pass evaluates the neighbour again from its target.  Both, under
the fused launch and under the two launches it replaces (MGL_NO_FUSE=1), are the same rules on the same inputs, so the four
chains agree bit for bit -- per-step stats, current and best slab, the last step's per-neighbour outputs.  The start is the one
at which repair picks do happen: c1 (4 096 B), 256 neighbours per step, from the parse liblzma (preset 6) makes of it, where
13 of a step's 256 neighbours need one (test_gpu_second_pass_workgroup.py; from the all-literal slab c1 takes none).  `-m gpu`."""
import lzma

import numpy as np
import pytest

from megalania_amd import binding, corpus
from test_gpu_fused_pick_walk import STAT_KEYS

pytestmark = pytest.mark.gpu

K, STEPS, SEED = 256, 12, 83
DUMPS = ("COSTS", "JOURNAL_LENS", "WALKED", "WINDOWS", "SOFT_ENDS")
# (MGL_NO_FUSE, MGL_NO_CONT): the first chain is the one the others are held against
CHAINS = ((False, False), (False, True), (True, False), (True, True))


def _chains(monkeypatch, data, start, **props):
    """the four chains from one seed; the launch switches are read at create.  MGL_NO_ADAPT keeps every step on the split form."""
    for k in ("MGL_NO_SPLIT", "MGL_NO_FUSE", "MGL_NO_CONT", "MGL_HALVES", "MGL_PICK_WAVES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MGL_NO_ADAPT", "1")
    out = []
    for no_fuse, no_cont in CHAINS:
        for k, on in (("MGL_NO_FUSE", no_fuse), ("MGL_NO_CONT", no_cont)):
            if on:
                monkeypatch.setenv(k, "1")
            else:
                monkeypatch.delenv(k, raising=False)
        sa = binding.SA(data, neighbours_per_step=K, seed=SEED, accept="single", **props)
        sa.set_slab(start)
        out.append(sa)
    monkeypatch.delenv("MGL_NO_FUSE", raising=False)
    monkeypatch.delenv("MGL_NO_CONT", raising=False)
    return out


@pytest.mark.parametrize("props", [{}, dict(lc=3, lp=0, pb=2)], ids=["lc0_lp0_pb0", "lc3_lp0_pb2"])
def test_resume_and_restart_agree(monkeypatch, props):
    """lc=3, lp=0, pb=2: more bitmap words in front of it, so the journal's neighbours in the wave area sit elsewhere"""
    data, _ = corpus.config_input("c1")
    stream = lzma.compress(data, format=lzma.FORMAT_ALONE,
                           filters=[dict(id=lzma.FILTER_LZMA1, preset=6, dict_size=1 << 22, lc=0, lp=0, pb=0)])
    start, _ = binding.stream_import(stream, data)
    chains = _chains(monkeypatch, data, start, **props)
    picks = [0] * len(chains)     # most repair picks in a step
    fallback = [0] * len(chains)
    for s in range(STEPS):
        stats = [sa.run(1) for sa in chains]
        for i, (sa, st) in enumerate(zip(chains, stats)):
            for k in STAT_KEYS:
                assert st[k] == stats[0][k], (CHAINS[i], s, k, st[k], stats[0][k])
            picks[i] = max(picks[i], int(sa.debug_dump(binding.DUMP.STEP_COUNTS)[0]["repair_picks"]))
            fallback[i] += st["fallback_neighbours"]
    print(f"{props}: most repair picks in a step {picks}, fallback neighbours {fallback}")
    (c0, cost0), (b0, bcost0) = chains[0].current(), chains[0].best()
    dumps0 = [chains[0].debug_dump(getattr(binding.DUMP, d)) for d in DUMPS]
    for i, sa in enumerate(chains[1:], 1):
        (c, cost), (b, bcost) = sa.current(), sa.best()
        assert cost == cost0 and (c == c0).all(), CHAINS[i]  # the whole slab: off-walk entries too
        assert bcost == bcost0 and (b == b0).all(), CHAINS[i]
        for d, x in zip(DUMPS, dumps0):
            y = sa.debug_dump(getattr(binding.DUMP, d))
            assert len(x) == len(y) and (x == y).all(), (CHAINS[i], d, np.nonzero(x != y)[0][:8])
    for i in range(len(chains)):
        # the resume path (continuations on) and the restart path (off) were really taken, and nothing went on to the full walk
        assert picks[i] >= 1 and fallback[i] == 0, (CHAINS[i], picks[i], fallback[i])
    for sa in chains:
        sa.close()
