"""The in-place accepts (mgl_kernels3.hip: a single accept; mgl_kernels5.hip: the moves of a bulk step) on inputs of one to
three index blocks.  The sizes are chosen so that the helpers the two accepts share (mgl_base2.h) should take their edge
branches -- expected from the sizes, not observed by the test:

  * at shift 8 the chain index has one block at 255 and 256 B, two at 257 B, three at 600 B, so chain_index_patch mostly
    touches the last entry alone, blk == nsb, whose bound is MGL_POS_INF;
  * every change lies within MGL_MAX_MATCH of the start or close to it, so ckpt_rows clamps ck_lo to 0;
  * chains of a few entries: runs reach the sentinel un-coupled, hi = MGL_POS_INF, a new sentinel is written;
  * in the batch walk a cluster's next_first lies within one 64-position window of its own journal.

What the test does observe, by the lock-step method of test_gpu_accept_giveups.py (its Chains, with the `multi` counter this
file needs): chain A patches in place, chain B never does (MGL_NO_INCREMENTAL_APPLY / MGL_NO_BATCH), a handle R rebuilds from
A's slab; after every accepted step the slabs are equal, the cost is the oracle's and A's structures equal R's.  Every case
must see an accept that was patched in place with a give-up word of 0, a bulk case also a step that took two or more moves.
No size was refused at creation.  `-m gpu`."""
import pytest

from megalania_amd import corpus
from test_gpu_accept_giveups import PB2, Chains, site_names

pytestmark = pytest.mark.gpu

K, SEED, STEPS = 16, 9, 16
# (size, props, accept): what the sixteen steps did on the MI355X run the cases were fixed on --
# single: steps patched in place; bulk: steps patched in place / of those, steps that took two or more moves
CASES = [
    (255, {}, "single"),    # 13
    (255, {}, "bulk"),      # 16 / 12
    (255, PB2, "single"),   # 14
    (255, PB2, "bulk"),     # 16 / 13
    (256, {}, "single"),    # 14
    (256, {}, "bulk"),      # 14 / 13
    (256, PB2, "single"),   # 15
    (256, PB2, "bulk"),     # 14 / 12
    (257, {}, "single"),    # 14
    (257, {}, "bulk"),      # 16 / 14
    (257, PB2, "single"),   # 13
    (257, PB2, "bulk"),     # 14 / 12
    (600, {}, "single"),    # 15
    (600, {}, "bulk"),      # 16 / 15
    (600, PB2, "single"),   # 16
    (600, PB2, "bulk"),     # 16 / 16
]


@pytest.mark.parametrize("size,props,kind", CASES, ids=[f"{c[0]}-{c[2]}{'-lc2lp1pb2' if c[1] else ''}" for c in CASES])
def test_in_place_accept_equals_rebuild_on_tiny_inputs(size, props, kind, monkeypatch):
    ch = Chains(kind, corpus.enwik_like(size, 0x5151), K, SEED, props, monkeypatch)
    try:
        words = ch.run(STEPS, expect=None, every=1)   # structures, slab and oracle cost after every accepted step
        patched = ch.a.batch_counters()[0] if kind == "bulk" else ch.in_place
        print(f"{size} B {kind} {props}: {ch.in_place} of {STEPS} steps accepted with no give-up, {patched} patched in place, "
              f"{ch.multi} took two or more moves, give-ups {[site_names(w) for w in words if w]}")
        assert ch.in_place >= 1 and patched >= 1
        if kind == "bulk":
            assert ch.multi >= 1
    finally:
        ch.close()
