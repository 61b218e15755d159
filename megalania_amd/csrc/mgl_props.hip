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
#define MGL_PROPS_MAX_PROBS (MGL_OFF_LIT + (0x300u << 4) + 1u) /* 14 135 rounded up to an even count */

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
	__shared__ uint16_t probs[MGL_PROPS_MAX_PROBS];
	const uint32_t lane = threadIdx.x;
	const mgl_layout L = mgl_props_triple(blockIdx.x);
	for (uint32_t i = lane; i < 2048u; i += 64u) T[i] = c.cost_tbl[i];
	for (uint32_t i = lane; i < L.total; i += 64u) probs[i] = MGL_PROB_INIT;
	Walk w;
	walk_reset(w);
	wave_sync();
	while (w.st.pos < c.n) {
		const uint32_t pos = w.st.pos;
		walk_window(w, c, slab, lane);
		const mgl_pk pk = walk_slab_at(w, pos);
		const uint32_t type = mgl_pk_type(pk), dist = mgl_pk_dist(pk), len = mgl_pk_len(pk);
		if (!mgl_pk_wellformed(type, dist, len) || len > c.n - pos) break; /* the walk of mgl_cost_slab refused such a slab: never taken */
		uint32_t match_byte = 0, prev_byte = 0;
		if (type == MGL_LITERAL) {
			if (w.st.ctx_state >= 7u && w.st.dists[0] < pos) match_byte = c.data[pos - w.st.dists[0] - 1u];
			if (L.lc > 0u && pos > 0u) prev_byte = pos > w.wbase ? walk_byte_at(w, pos - 1u) : c.data[pos - 1u];
		}
		mgl_plan pl;
		mgl_plan_packet(&L, &w.st, type, dist, len, walk_byte_at(w, pos), match_byte, prev_byte, &pl);
		if (lane < pl.nev) {
			uint32_t ctx, bit;
			mgl_plan_event(&pl, lane, &ctx, &bit);
			const uint32_t p = probs[ctx];
			w.acc += T[bit ? 2048u - p : p];
			probs[ctx] = (uint16_t)mgl_prob_update(p, bit);
		}
		if (lane == 0) w.acc += (uint64_t)pl.ndirect << 11;
		mgl_advance(&w.st, type, dist, len);
	}
	const uint64_t total = wave_sum64(w.acc);
	if (lane == 0) cost_out[blockIdx.x] = total;
}
