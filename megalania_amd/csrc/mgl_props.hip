/*
 * mgl_props.hip -- the exact cost of one parse under every supported lc/lp/pb.
 *
 * Not in the reference, whose properties are fixed at 0/0/0 (main.c:45).  A packet slab is a valid parse whatever
 * the properties are: the walk, the context automaton and the rep stack do not depend on them, only the probability
 * slot a bit lands in does (mgl_plan_packet takes the layout as an argument).  So one kernel costs the same slab
 * under all of them side by side:
 *
 *   k_props_sweep  grid of MGL_PROPS_NTRIPLES workgroups of one wavefront; workgroup t walks the slab from the LZMA
 *                  initial state under triple t (canonical order: for lc in 0..4, for lp in 0..4 - lc, for pb in 0..4),
 *                  the whole probability model (at most 1847 + (0x300 << 4) u16) and the bit-cost table in LDS.
 *                  Lane e takes event slot e of the packet (no slot occurs twice in one packet): reads its
 *                  probability, looks the bit's cost up, writes mgl_prob_update back; direct bits cost 2048 each;
 *                  per-lane u64 partial sums are reduced once at the end (u64 addition commutes: bit-exact).
 *
 * Validity does not depend on the triple and is decided once, by the host: mgl_props_sweep runs the existing walk
 * (scratch_walk, the one mgl_cost_slab uses) over a caller's slab first and refuses what that refuses, so the kernel
 * trusts its slab.  It still stops at an entry of no known type, of length 0 or running off the end, so that a slab that
 * slipped through could cost nonsense but never read out of bounds or loop.
 */
#include "mgl_device.h"

#define MGL_PROPS_NTRIPLES 75u

/* triple number t of the canonical order */
__host__ __device__ static inline mgl_layout mgl_props_triple(uint32_t t)
{
	const uint32_t pair = t / 5u; /* lc = 0: pairs 0..4, 1: 5..8, 2: 9..11, 3: 12..13, 4: 14 */
	const uint32_t lc = pair < 5u ? 0u : pair < 9u ? 1u : pair < 12u ? 2u : pair < 14u ? 3u : 4u;
	const uint32_t first = lc == 0u ? 0u : lc == 1u ? 5u : lc == 2u ? 9u : lc == 3u ? 12u : 14u;
	return mgl_make_layout(lc, pair - first, t % 5u);
}

__global__ void __launch_bounds__(64) k_props_sweep(DevCtx c, const mgl_pk* slab, uint64_t* cost_out)
{
	__shared__ uint16_t T[2048];
	__shared__ uint16_t probs[MGL_MAX_PROBS];
	const uint32_t lane = threadIdx.x;
	const mgl_layout L = mgl_props_triple(blockIdx.x);
	for (uint32_t i = lane; i < 2048u; i += 64u) T[i] = c.cost_tbl[i];
	for (uint32_t i = lane; i < L.total; i += 64u) probs[i] = MGL_PROB_INIT;
	Walk w;
	walk_reset(w);
	wave_sync();
	while (w.st.pos < c.n) {
		const uint32_t pos = w.st.pos;
		win_cover(w.win, c, slab, w.st.pos, lane);
		const mgl_pk pk = win_pk(w.win, pos);
		const uint32_t type = mgl_pk_type(pk), dist = mgl_pk_dist(pk), len = mgl_pk_len(pk);
		if (!mgl_pk_wellformed(type, dist, len) || len > c.n - pos) break; /* the walk of mgl_cost_slab refused such a slab: never taken */
		walk_packet<true>(w, L, c.data, probs, T, type, dist, len, lane);
	}
	const uint64_t total = wave_sum64(w.acc);
	if (lane == 0) cost_out[blockIdx.x] = total;
}
