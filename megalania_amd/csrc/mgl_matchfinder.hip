/*
 * mgl_matchfinder.hip -- per-position match lists for the optimal parses: the nearest source of every achievable
 * length ("match finder").
 *
 * Not in the reference.  The node loops of mgl_optimal.hip / mgl_adaptive.hip offer each node the `cand` nearest
 * earlier positions with the same two and the same four bytes; this file makes, once per handle, the list an LZ
 * optimiser wants instead: F(i) = (q_1, l_1), (q_2, l_2), ... with q_k the nearest earlier position whose match at i is
 * longer than l_{k-1}, so lengths rise and distances rise along a list.  The exact-prefix orders of mgl_index.hip
 * (D = 2..8 and 16: rank, run start, positions) make the nearest earlier position that shares D bytes with i one
 * look-up: the entry in front of i in its run.
 *
 * The rule, restated in plain Python in tests/test_match_frontier_cpu.py (frontier_rule):
 *
 *   cap = min(273, n - i); best = 1; budget = depth; list = []
 *   while best < cap and len(list) < 60:
 *       need  = best + 1
 *       level = need if need <= 8 else (16 if need >= 16 else 8)
 *       R = earlier positions that share `level` bytes with i, nearest first
 *       need == level:  q = first of R; stop if none or outside the window          (costs no budget)
 *       else:           go through R from just beyond the last source; every entry examined costs 1 of budget; stop
 *                       at budget == 0, at the end of R or outside the window; q = the first entry longer than best
 *       list += (q, matchlen(q, i, cap)); best = that length
 *
 * Three kernels, each run twice (count, then -- behind an exclusive scan of the counts -- fill):
 *
 *   k_mf_direct  a lane per position: the look-ups for need = 2..8.  A position that goes on (best >= 8) is queued
 *                with its state (count pass only; the fill pass reads the same queue)
 *   k_mf_scan    a wavefront per queued position: the look-up at need == 16 and the budgeted scans of the 8- and
 *                16-byte runs.  64 lanes take the next 64 entries of the run, nearest first, each computes its entry's
 *                match length, and a ballot picks the first that beats `best`; the later lanes of the same trip
 *                already hold their lengths for the next `need`.  The budget consumed is the ordinal of the last
 *                entry the serial rule would have examined: the one it took
 *
 * Output: off[n + 1] (exclusive scan of the list lengths), src[] (u32 source position), len[] (u16 match length).
 * No scratch memory, no LDS; the only atomic is the queue's counter (one add per wavefront of k_mf_direct).
 */
#include "mgl_device.h"

#define MGL_MF_MAX_ENTRIES 60u /* 64 lanes of a node's wavefront minus the four rep lanes */
#define MGL_MF_DEF_DEPTH 64u
#define MGL_MF_MAX_DEPTH 4096u

/* what the node loops read */
struct MfLists {
	const uint32_t* off; /* n + 1 */
	const uint32_t* src;
	const uint16_t* len;
};

/* match length of q against i, given that the first `from` bytes agree: 8 bytes per load, the trailing equal bytes of
 * the first word that differs.  Loads reach at most 7 bytes past i + cap <= n: the input is zero padded (128 bytes). */
__device__ __forceinline__ uint32_t mf_mlen(const uint8_t* d, uint32_t q, uint32_t i, uint32_t from, uint32_t cap)
{
	uint32_t k = from;
	while (k < cap) {
		uint64_t a, b;
		__builtin_memcpy(&a, d + q + k, 8);
		__builtin_memcpy(&b, d + i + k, 8);
		const uint64_t x = a ^ b;
		if (x) { k += ((uint32_t)__ffsll((long long)x) - 1u) >> 3; break; }
		k += 8u;
	}
	return k < cap ? k : cap;
}

/* the nearest earlier position that shares `D` bytes (2..8 or 16) with i, i + D <= n; false if there is none */
__device__ __forceinline__ bool mf_nearest(const DevCtx& c, uint32_t i, uint32_t D, uint32_t* q)
{
	if (D == 2u) {
		const uint32_t bigram = ((uint32_t)c.data[i] << 8) | c.data[i + 1];
		const uint32_t lo = c.bucket_off[bigram];
		const uint32_t hi = gs_lower_u32(c.bucket_pos, lo, c.bucket_off[bigram + 1], i);
		if (hi == lo) return false;
		*q = c.bucket_pos[hi - 1u];
		return true;
	}
	const uint32_t* rank = D == 16u ? c.hex_rank : D == 8u ? c.oct_rank : c.xrank[D - 2u];
	const uint32_t* run = D == 16u ? c.hex_run : D == 8u ? c.oct_run : c.xrun[D - 2u];
	const uint32_t* pos = D == 16u ? c.hex_pos : D == 8u ? c.oct_pos : c.xpos[D - 2u];
	const uint32_t r = rank[i];
	if (r == run[r]) return false;
	*q = pos[r - 1u];
	return true;
}

/* queue record of a position that goes on to k_mf_scan: x = position, y = last source, z = best | count << 16 */
template <bool FILL>
__global__ void __launch_bounds__(256) k_mf_direct(DevCtx c, uint32_t* off, uint32_t* src, uint16_t* len, uint4* queue, uint32_t* qcount)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t n = c.n;
	uint32_t best = 1u, cnt = 0u, q_last = 0u;
	const uint32_t cap = i < n ? ((n - i) < MGL_MAX_MATCH ? (n - i) : MGL_MAX_MATCH) : 0u;
	const uint32_t o = (FILL && i < n) ? off[i] : 0u;
	bool final = false;
	while (best < cap && best < 8u) {
		uint32_t q;
		if (!mf_nearest(c, i, best + 1u, &q) || i - q - 1u >= c.dict_limit) { final = true; break; }
		best = mf_mlen(c.data, q, i, best + 1u, cap);
		if (FILL) { src[o + cnt] = q; len[o + cnt] = (uint16_t)best; }
		cnt++;
		q_last = q;
	}
	if (FILL) return;
	if (i <= n) off[i] = cnt; /* off[n] = 0: the scan's total lands there */
	const bool more = !final && best < cap; /* best >= 8: at most 7 entries so far */
	const unsigned long long bal = __ballot(more);
	if (bal) {
		const uint32_t lane = threadIdx.x & 63u;
		uint32_t base = 0;
		if (lane == (uint32_t)__ffsll((long long)bal) - 1u) base = atomicAdd(qcount, (uint32_t)__popcll(bal));
		base = (uint32_t)__shfl((int)base, __ffsll((long long)bal) - 1, 64);
		if (more) queue[base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = make_uint4(i, q_last, best | (cnt << 16), 0u);
	}
}

/* One wavefront per queued position (4 per workgroup).  All of best, cnt, budget, the run bounds are wave-uniform. */
template <bool FILL>
__global__ void __launch_bounds__(256) k_mf_scan(DevCtx c, uint32_t depth, uint32_t* off, uint32_t* src, uint16_t* len, const uint4* queue,
                                                 const uint32_t* qcount)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t w = uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
	if (w >= *qcount) return;
	const uint4 rec = queue[w];
	const uint32_t i = uni(rec.x);
	uint32_t q_last = uni(rec.y), best = uni(rec.z & 0xFFFFu), cnt = uni(rec.z >> 16);
	const uint32_t n = c.n;
	const uint32_t cap = (n - i) < MGL_MAX_MATCH ? (n - i) : MGL_MAX_MATCH;
	const uint32_t o = FILL ? off[i] : 0u;
	uint32_t budget = depth;
	bool final = false;
	while (!final && best < cap && cnt < MGL_MF_MAX_ENTRIES) {
		if (best == 15u) {
			/* need == 16: one look-up, costs no budget */
			uint32_t q;
			if (!mf_nearest(c, i, 16u, &q) || i - q - 1u >= c.dict_limit) break;
			best = uni(mf_mlen(c.data, q, i, 16u, cap));
			if (FILL && lane == 0) { src[o + cnt] = q; len[o + cnt] = (uint16_t)best; }
			cnt++;
			q_last = q;
			continue;
		}
		/* need 9..15 in the 8-byte run, need >= 17 in the 16-byte run: the entries beyond q_last, nearest first; entry of
		 * ordinal t (0-based) sits at rq - 1 - t and is examined iff t < budget */
		const bool wide = best >= 16u;
		const uint32_t level = wide ? 16u : 8u;
		const uint32_t* pos = wide ? c.hex_pos : c.oct_pos;
		const uint32_t rq = wide ? c.hex_rank[q_last] : c.oct_rank[q_last];
		const uint32_t avail = rq - (wide ? c.hex_run[rq] : c.oct_run[rq]); /* entries of the run beyond q_last */
		const uint32_t lim = avail < budget ? avail : budget;
		uint32_t used = 0; /* ordinal + 1 of the last entry taken in this run */
		bool leave = false; /* the level changes: the next look-up is in another run */
		for (uint32_t t0 = 0; !final && !leave; t0 += 64u) {
			const uint32_t t = t0 + lane;
			uint32_t q = 0, ml = 0;
			if (t < lim) {
				q = pos[rq - 1u - t];
				if (i - q - 1u < c.dict_limit) ml = mf_mlen(c.data, q, i, level, cap);
			}
			/* lanes that hold no entry (end of the run, budget, window) have ml = 0: they form a suffix of the trip */
			unsigned long long after = ~0ull;
			for (;;) {
				const unsigned long long bal = __ballot(ml > best) & after;
				if (!bal) break;
				const uint32_t l = (uint32_t)__ffsll((long long)bal) - 1u;
				best = rdlane(ml, l);
				q_last = rdlane(q, l);
				if (FILL && lane == 0) { src[o + cnt] = q_last; len[o + cnt] = (uint16_t)best; }
				cnt++;
				used = t0 + l + 1u;
				after = l == 63u ? 0ull : ~((2ull << l) - 1ull);
				if (best >= cap || cnt >= MGL_MF_MAX_ENTRIES) { final = true; break; }
				if (!wide && best >= 15u) { leave = true; break; }
			}
			if (final || leave) break;
			/* nothing (more) in this trip beats best: the list is final unless all 64 lanes held an examined entry
			 * inside the window; an entry outside the window ends the scan like the end of the run */
			const unsigned long long held = __ballot(t < lim && i - q - 1u < c.dict_limit);
			if (held != ~0ull) final = true;
		}
		budget -= used;
	}
	if (!FILL && lane == 0) off[i] = cnt;
}
