/*
 * mgl_costmap.hip -- where a parse spends its bits: the exact cost of every packet, per coder and per byte
 * (DESIGN.md section 10).
 *
 * Not in the reference, whose perplexity encoder keeps one running sum (perplexity_encoder.c:6-17).  The walk is the one
 * of k_props_sweep -- one wavefront, the whole model and the bit-cost table in LDS, lane e on event slot e -- and keeps
 * what that walk throws away:
 *
 *   k_costmap_walk    one workgroup of one wavefront walks the slab from the LZMA initial state under the layout it is
 *                     handed (the handle's or a foreign one, as in the sweep).  A lane's event belongs to the coder its
 *                     context index lies in (costmap_class: the ranges of mgl_model.h); the lane adds the event's cost
 *                     and one bit to its own pair of u64 accumulators for that coder, which are reduced once, at the
 *                     end.  Direct bits have no context: 2048 each, counted in a wave-uniform scalar.  The packet's
 *                     own total is the one reduction per packet (32 bits); lane 0 stores it with the packet's length,
 *                     packed into one word, at the packet's start position of `mark`, which the host zeroed.  Per-type
 *                     sums are wave-uniform scalars.  Packets are taken one per turn, as walk_packet takes them: the
 *                     literal-run planner hands out the events of up to seven literals at once, but those share
 *                     contexts (is_match, the top of the literal tree), so their costs would have to be taken one
 *                     packet at a time all the same.
 *   k_costmap_spread  a grid over positions: a position whose mark is set starts a packet of cost c and length len and
 *                     gives its byte k the value c / len + (k < c % len), clamped at n.  The bytes of a packet belong to
 *                     no other packet, so plain stores do, and every byte of a completed walk is written.
 *
 * Validity is the host's business, as in the sweep (mgl_cost_map runs the walk of mgl_cost_slab over a caller's slab
 * first).  The walk still stops at an entry that is no packet or runs off the end, and says where it stopped: a slab that
 * slipped through is reported, never read out of bounds or looped on.
 */
#include "mgl_costmap.h"

/* The sum of v over the wavefront (every lane active), wave-uniform.  This is the walk's one reduction per packet, so it
 * stays off the LDS crossbar that six __shfl_xor steps would cross: four row shifts inside the rows of 16 lanes (DPP
 * row_shr 1, 2, 4, 8; a lane without a source adds 0) leave each row's sum in its last lane, and four v_readlane add
 * the rows up. */
template <int ROW_SHR>
__device__ __forceinline__ uint32_t row_shr_or_zero(uint32_t v)
{
	return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + ROW_SHR, 0xF, 0xF, true);
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v)
{
	v += row_shr_or_zero<1>(v);
	v += row_shr_or_zero<2>(v);
	v += row_shr_or_zero<4>(v);
	v += row_shr_or_zero<8>(v);
	return rdlane(v, 15) + rdlane(v, 31) + rdlane(v, 47) + rdlane(v, 63);
}

__global__ void __launch_bounds__(64) k_costmap_walk(DevCtx c, mgl_layout L, const mgl_pk* slab, uint32_t* mark, CostMapSums* out)
{
	__shared__ uint16_t T[2048];
	__shared__ uint16_t probs[MGL_MAX_PROBS];
	const uint32_t lane = threadIdx.x;
	for (uint32_t i = lane; i < 2048u; i += 64u) T[i] = c.cost_tbl[i];
	for (uint32_t i = lane; i < L.total; i += 64u) probs[i] = MGL_PROB_INIT;
	mgl_wstate st = state_initial();
	Win win;
	win_reset(win);
	uint64_t cls_cost[MGL_CM_CLASSES - 1u] = {}, cls_bits[MGL_CM_CLASSES - 1u] = {}; /* per lane; constant indices only */
	uint64_t direct_bits = 0, total = 0, packets = 0;                                 /* wave-uniform from here on */
	uint64_t type_cost[4] = {}, type_packets[4] = {}, type_bytes[4] = {};
	wave_sync();
	while (st.pos < c.n) {
		const uint32_t pos = st.pos;
		win_cover(win, c, slab, pos, lane);
		const mgl_pk pk = win_pk(win, pos);
		const uint32_t type = mgl_pk_type(pk), dist = mgl_pk_dist(pk), len = mgl_pk_len(pk);
		if (!mgl_pk_wellformed(type, dist, len) || len > c.n - pos) break; /* the walk of mgl_cost_slab refused such a slab: never taken */
		mgl_plan pl;
		plan_at(L, c.data, st, type, dist, len, win_byte(win, pos), pl);
		uint32_t ev_cost = 0;
		if (lane < pl.nev) {
			uint32_t ctx, bit;
			mgl_plan_event(&pl, lane, &ctx, &bit);
			const uint32_t p = probs[ctx];
			ev_cost = T[bit ? 2048u - p : p];
			probs[ctx] = (uint16_t)mgl_prob_update(p, bit);
			const uint32_t k = costmap_class(ctx);
#pragma unroll
			for (uint32_t j = 0; j < MGL_CM_CLASSES - 1u; j++) {
				cls_cost[j] += k == j ? ev_cost : 0u;
				cls_bits[j] += k == j ? 1u : 0u;
			}
		}
		const uint32_t cost = uni(wave_sum32(ev_cost)) + (pl.ndirect << 11);
		if (lane == 0) mark[pos] = cost | len << MGL_CM_COST_BITS;
		direct_bits += pl.ndirect;
		total += cost;
		packets++;
#pragma unroll
		for (uint32_t t = 0; t < 4u; t++) {
			const bool mine = type == t + 1u;
			type_cost[t] += mine ? cost : 0u;
			type_packets[t] += mine ? 1u : 0u;
			type_bytes[t] += mine ? len : 0u;
		}
		mgl_advance(&st, type, dist, len);
	}
	uint64_t sum_cost[MGL_CM_CLASSES - 1u], sum_bits[MGL_CM_CLASSES - 1u];
#pragma unroll
	for (uint32_t j = 0; j < MGL_CM_CLASSES - 1u; j++) {
		sum_cost[j] = wave_sum64(cls_cost[j]);
		sum_bits[j] = wave_sum64(cls_bits[j]);
	}
	if (lane == 0) {
		out->total = total;
		out->packets = packets;
#pragma unroll
		for (uint32_t j = 0; j < MGL_CM_CLASSES - 1u; j++) {
			out->class_cost[j] = sum_cost[j];
			out->class_bits[j] = sum_bits[j];
		}
		out->class_cost[MGL_CM_CLASSES - 1u] = direct_bits << 11;
		out->class_bits[MGL_CM_CLASSES - 1u] = direct_bits;
#pragma unroll
		for (uint32_t t = 0; t < 4u; t++) {
			out->type_cost[t] = type_cost[t];
			out->type_packets[t] = type_packets[t];
			out->type_bytes[t] = type_bytes[t];
		}
		out->end_pos = st.pos;
		out->pad = 0;
	}
}

__global__ void __launch_bounds__(256) k_costmap_spread(uint32_t n, const uint32_t* mark, uint32_t* map)
{
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const uint32_t m = mark[p];
	if (m == 0) return; /* no packet starts here */
	const uint32_t cost = m & ((1u << MGL_CM_COST_BITS) - 1u), len = m >> MGL_CM_COST_BITS;
	const uint32_t share = cost / len, extra = cost % len;
	const uint32_t take = len < n - p ? len : n - p;
	for (uint32_t k = 0; k < take; k++) map[p + k] = share + (k < extra ? 1u : 0u);
}
