/*
 * mgl_costmap_live.hip -- the cost map of the current slab, read off the base structures.
 *
 * Not in the reference (see mgl_costmap.hip).  The serial walk of mgl_costmap.hip re-simulates the model to learn what every
 * coded bit cost.  For the current slab the incremental engine has that already: every coded event of the walk lies in its
 * context's chain (mgl_base2.h) with its packet's position, its bit and the probability before the update, so an event's
 * price is one look-up in the cost table and nothing is walked.  Every event of a packet carries the packet's start, a
 * packet starts in one block of 1 << sb_shift positions, and the chain index says where a context's entries of a block
 * lie: a block's packets get their whole cost from that block's stretch of every chain.
 *
 *   k_cml_blocks   a workgroup of four wavefronts per block of the chain index (the grid strides over the blocks), in
 *                  three stages around an LDS copy of the block's marks:
 *                    packets  a thread per position: a packet start (the on-walk bitmap) puts ndirect << 11 | len << 20
 *                             into its mark -- the direct bits' cost by costmap_ndirect, no context involved --, any
 *                             other position 0.
 *                    events   a wavefront per 64 contexts: lane l loads context c0 + l's two index entries of the block;
 *                             an inclusive scan of the counts numbers the group's entries, and the lanes stride over
 *                             those numbers, each finding its entry's context by a search of the 64 sums in LDS.  So
 *                             the one context that holds an entry per packet (is_match) and the thousands that hold
 *                             none cost what their entries cost, not a lane each.  The entry's price goes to its
 *                             packet's mark by an LDS add and to the lane's accumulators of its context's class.
 *                    marks    a thread per position again: the finished mark goes to global memory by a plain store
 *                             (every position of the block is written: no memset), and a packet start adds its cost to
 *                             the thread's sums per packet type.
 *                  At the end the workgroup reduces its sums (wave_sum64, then across the four wavefronts in LDS) and
 *                  issues one 64-bit atomic per sum that is not 0.  Integer adds commute: the result is exact whatever
 *                  the order.
 *   k_costmap_spread (mgl_costmap.hip) turns the marks into the map, as for the serial walk.
 *   k_cml_weights  its sibling for the live target weights: w[x] = map[x] + floor straight from the marks, no map in
 *                  between; floor is the caller's or, with floor_mean, the total the blocks kernel left / n.
 *   k_cml_check    one thread: the total against the control block's exact cost of the base; a difference raises
 *                  MGL_ERR_REBUILD_MISMATCH (inside a run, where the host does not read the sums before the next step).
 *
 * Nothing outside [ch_off[c] + row[b], ch_off[c] + row[b + 1]) of a context is read: the stale regions of the pool and the
 * sentinels are never looked at.  An index or a position that cannot be (a count above the block's positions, a position
 * outside the block, an entry outside the pool) is skipped, never followed: the total then differs from the control
 * block's cost and the call fails its consistency check.
 */
#include "mgl_base2.h"
#include "mgl_costmap.h"

#define MGL_CML_THREADS 256u
#define MGL_CML_WAVES (MGL_CML_THREADS / 64u)
#define MGL_CML_MAX_BLOCK (1u << 10) /* positions of the largest chain-index block (MGL_PB_MAX_SHIFT; mgl_api.hip asserts it) */
#define MGL_CML_GRID 1024u            /* workgroups at most: four per CU */
/* the sums a workgroup hands over, in CostMapSums' order of fields: total, packets, class_cost, class_bits, type_* */
#define MGL_CML_SUMS (2u + 2u * MGL_CM_CLASSES + 12u)
static_assert(offsetof(CostMapSums, end_pos) == MGL_CML_SUMS * sizeof(uint64_t), "the sums are CostMapSums' leading u64 fields");

__global__ void __launch_bounds__(MGL_CML_THREADS) k_cml_blocks(DevCtx c, Base2 b, uint32_t* mark, CostMapSums* out)
{
	__shared__ uint16_t T[2048];
	__shared__ uint32_t lmark[MGL_CML_MAX_BLOCK];
	__shared__ uint32_t grp_incl[MGL_CML_WAVES][64], grp_base[MGL_CML_WAVES][64];
	__shared__ uint64_t red[MGL_CML_WAVES][MGL_CML_SUMS];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const uint32_t bsize = 1u << b.sb_shift, total_ctx = c.L.total, pool = b.pool_cap + 256u;
	for (uint32_t i = tid; i < 2048u; i += MGL_CML_THREADS) T[i] = c.cost_tbl[i];
	uint64_t cls_cost[MGL_CM_CLASSES - 1u] = {}, cls_bits[MGL_CM_CLASSES - 1u] = {}; /* per lane; constant indices only */
	uint64_t type_cost[4] = {}, type_packets[4] = {}, type_bytes[4] = {}, direct_bits = 0;
	__syncthreads();
	for (uint32_t blk = blockIdx.x; blk < b.nsb; blk += gridDim.x) {
		const uint32_t p0 = blk << b.sb_shift;
		/* ---- packets: the direct bits and the length of every packet that starts in the block */
		for (uint32_t i = tid; i < bsize; i += MGL_CML_THREADS) {
			const uint32_t p = p0 + i;
			uint32_t m = 0;
			if (p < c.n && (b.onwalk[p >> 6] >> (p & 63u) & 1ull)) {
				const mgl_pk pk = b.slab[p];
				m = costmap_ndirect(mgl_pk_type(pk), mgl_pk_dist(pk)) << 11 | mgl_pk_len(pk) << MGL_CM_COST_BITS;
			}
			lmark[i] = m;
		}
		__syncthreads();
		/* ---- events: every context's entries of the block */
		for (uint32_t c0 = wave * 64u; c0 < total_ctx; c0 += MGL_CML_THREADS) {
			const uint32_t ctx = c0 + lane;
			uint32_t cnt = 0, first = 0;
			if (ctx < total_ctx) {
				const uint32_t* row = b.ch_sb + (size_t)ctx * b.sb_stride;
				const uint32_t lo = row[blk], hi = row[blk + 1u];
				cnt = hi - lo;
				if (cnt > bsize) cnt = 0; /* a context has at most one event per packet: cannot be */
				if (cnt) first = b.ch_off[ctx] + lo;
			}
			uint32_t incl = cnt;
			for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64); if ((int)lane >= o) incl += t; }
			const uint32_t entries = rdlane(incl, 63);
			if (entries == 0) continue; /* uniform */
			grp_incl[wave][lane] = incl;
			grp_base[wave][lane] = first - (incl - cnt); /* entry number e of the group lies at grp_base[its lane] + e */
			wave_sync();
			for (uint32_t e = lane; e < entries; e += 64u) {
				uint32_t l = 0; /* the first lane whose inclusive sum exceeds e: the one that holds entry e */
#pragma unroll
				for (uint32_t s = 32u; s; s >>= 1) if (grp_incl[wave][l + s - 1u] <= e) l += s;
				const uint32_t k = grp_base[wave][l] + e;
				if (k >= pool) continue;
				const uint32_t at = b.ch_pos[k] - p0, ev = b.ch_ev[k];
				if (at >= bsize || lmark[at] == 0) continue; /* (a mark that holds a packet's length is never 0, nor becomes it) */
				const uint32_t pr = ev & 0x7FFu, price = T[(ev >> 15) ? 2048u - pr : pr];
				atomicAdd(&lmark[at], price);
				const uint32_t cls = costmap_class(c0 + l);
#pragma unroll
				for (uint32_t j = 0; j < MGL_CM_CLASSES - 1u; j++) {
					cls_cost[j] += cls == j ? price : 0u;
					cls_bits[j] += cls == j ? 1u : 0u;
				}
			}
			wave_sync();
		}
		__syncthreads();
		/* ---- marks: out to global memory, and the sums per packet type */
		for (uint32_t i = tid; i < bsize; i += MGL_CML_THREADS) {
			const uint32_t p = p0 + i;
			if (p >= c.n) break;
			const uint32_t m = lmark[i];
			mark[p] = m;
			if (m == 0) continue;
			const uint32_t cost = m & ((1u << MGL_CM_COST_BITS) - 1u), len = m >> MGL_CM_COST_BITS;
			const mgl_pk pk = b.slab[p];
			const uint32_t type = mgl_pk_type(pk);
			direct_bits += costmap_ndirect(type, mgl_pk_dist(pk));
#pragma unroll
			for (uint32_t t = 0; t < 4u; t++) {
				const bool mine = type == t + 1u;
				type_cost[t] += mine ? cost : 0u;
				type_packets[t] += mine ? 1u : 0u;
				type_bytes[t] += mine ? len : 0u;
			}
		}
		__syncthreads();
	}
	/* ---- the workgroup's sums: across the wavefront, across the wavefronts, one atomic each */
	uint64_t v[MGL_CML_SUMS];
	v[0] = type_cost[0] + type_cost[1] + type_cost[2] + type_cost[3];
	v[1] = type_packets[0] + type_packets[1] + type_packets[2] + type_packets[3];
#pragma unroll
	for (uint32_t j = 0; j < MGL_CM_CLASSES - 1u; j++) { v[2u + j] = cls_cost[j]; v[2u + MGL_CM_CLASSES + j] = cls_bits[j]; }
	v[2u + MGL_CM_CLASSES - 1u] = direct_bits << 11;
	v[2u + 2u * MGL_CM_CLASSES - 1u] = direct_bits;
#pragma unroll
	for (uint32_t t = 0; t < 4u; t++) {
		v[2u + 2u * MGL_CM_CLASSES + t] = type_cost[t];
		v[6u + 2u * MGL_CM_CLASSES + t] = type_packets[t];
		v[10u + 2u * MGL_CM_CLASSES + t] = type_bytes[t];
	}
#pragma unroll
	for (uint32_t i = 0; i < MGL_CML_SUMS; i++) {
		const uint64_t s = wave_sum64(v[i]);
		if (lane == 0) red[wave][i] = s;
	}
	__syncthreads();
	if (tid < MGL_CML_SUMS) {
		uint64_t s = 0;
		for (uint32_t w = 0; w < MGL_CML_WAVES; w++) s += red[w][tid];
		if (s) atomicAdd((unsigned long long*)out + tid, (unsigned long long)s);
	}
}

/* the live target weights from the marks: k_costmap_spread and k_wt_from_map in one, w[p + k] = c / len + (k < c % len) + floor */
__global__ void __launch_bounds__(256) k_cml_weights(uint32_t n, const uint32_t* mark, uint32_t floor, uint32_t floor_mean, const CostMapSums* sums, uint32_t* w)
{
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const uint32_t m = mark[p];
	if (m == 0) return; /* no packet starts here */
	if (floor_mean) floor = (uint32_t)(sums->total / n); /* below 2^20: a byte's share of a packet's cost */
	const uint32_t cost = m & ((1u << MGL_CM_COST_BITS) - 1u), len = m >> MGL_CM_COST_BITS;
	const uint32_t share = cost / len, extra = cost % len;
	const uint32_t take = len < n - p ? len : n - p;
	for (uint32_t k = 0; k < take; k++) w[p + k] = share + (k < extra ? 1u : 0u) + floor;
}

/* the live map's total is the exact cost of the base, which the control block holds: anything else is the device's error */
__global__ void k_cml_check(const CostMapSums* sums, Control* ctl)
{
	if (sums->total != ctl->rebuild_cost) atomicOr(&ctl->error_flags, MGL_ERR_REBUILD_MISMATCH);
}
