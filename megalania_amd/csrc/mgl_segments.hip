/*
 * mgl_segments.hip -- the exact cost of every candidate segment of one parse under every supported lc/lp/pb (DESIGN.md
 * section 10, "Segment props"; include/megalania_hip.h has the definitions).
 *
 * Not in the reference, which writes one LZMA stream under 0/0/0.  An LZMA2 chunk may reset the coder's state and set new
 * properties without resetting the dictionary, so a parse can be coded in segments, each under the triple that suits its
 * bytes.  A segment's coder starts with a fresh model, ctx_state 0 and rep distances (0, 0, 0, 0), while the slab's rep
 * packets name slots of the rep stack of the slab's own walk from byte 0: each packet is named again against the
 * segment's stack (SHORT_REP -> LITERAL, LONG_REP i -> LONG_REP j or MATCH) before it is costed.  Two kernels:
 *
 *   k_seg_starts   one wavefront walks the slab once without a model -- rep stack and positions only -- and writes, per
 *                  cut, whether a packet starts there and the slab's own ("true") rep distances at that point.
 *   k_props_spans  grid of spans x MGL_PROPS_NTRIPLES workgroups of one wavefront.  Workgroup (q, T) takes the q-th span
 *                  of the launch order (longest first, so that the launch's tail is short) and walks [c_i, c_j) under
 *                  triple T exactly as k_props_sweep walks the whole slab: model and bit-cost table in LDS, lane e on
 *                  event slot e.  Beside the walk's own state it carries the true stack, advanced by the slab's packet
 *                  while the walk advances by the re-expressed one.  Both stacks and the re-expression are wave-uniform:
 *                  they are made of readlane'd slab words and uniform loads, and stay in scalar registers.
 *
 * Validity is decided once, by the host, as for k_props_sweep (mgl_props_sweep_spans runs scratch_walk over a caller's
 * slab and reads k_seg_starts' flags before it launches k_props_spans).  Both kernels still stop at an entry of no known
 * type, of length 0 or running past the end of their stretch: a slab that slipped through could cost nonsense but never
 * read out of bounds or loop.
 */
#include "mgl_device.h"

#define MGL_SEG_START_WORDS 5u /* per cut: on-walk flag, then the four true rep distances */

/* the four rep distances of mgl_advance, without the rest of the walk state */
struct RepStack { uint32_t d0, d1, d2, d3; };
__device__ __forceinline__ uint32_t rep_at(const RepStack& s, uint32_t i) { return i == 0 ? s.d0 : i == 1 ? s.d1 : i == 2 ? s.d2 : s.d3; }
__device__ __forceinline__ void rep_advance(RepStack& s, uint32_t type, uint32_t dist)
{
	if (type == MGL_MATCH) {
		s.d3 = s.d2; s.d2 = s.d1; s.d1 = s.d0; s.d0 = dist;
	} else if (type == MGL_LONG_REP) {
		const uint32_t d = rep_at(s, dist);
		if (dist > 2) s.d3 = s.d2;
		if (dist > 1) s.d2 = s.d1;
		if (dist > 0) s.d1 = s.d0;
		s.d0 = d;
	}
}

/* cuts: ncuts ascending positions, the last one n.  starts: ncuts x MGL_SEG_START_WORDS. */
__global__ void __launch_bounds__(64) k_seg_starts(DevCtx c, const mgl_pk* slab, const uint32_t* cuts, uint32_t ncuts, uint32_t* starts)
{
	const uint32_t lane = threadIdx.x;
	Win win;
	win_reset(win);
	RepStack t = { 0, 0, 0, 0 };
	uint32_t pos = 0, k = 0;
	for (;;) {
		/* cuts the walk has stepped over are no packet starts; the one it stands on is */
		while (k < ncuts && cuts[k] <= pos) {
			if (lane == 0) {
				uint32_t* o = starts + k * MGL_SEG_START_WORDS;
				o[0] = cuts[k] == pos ? 1u : 0u;
				o[1] = t.d0; o[2] = t.d1; o[3] = t.d2; o[4] = t.d3;
			}
			k++;
		}
		if (pos >= c.n || k >= ncuts) break;
		win_cover(win, c, slab, pos, lane);
		const mgl_pk pk = win_pk(win, pos);
		const uint32_t type = mgl_pk_type(pk), dist = mgl_pk_dist(pk), len = mgl_pk_len(pk);
		if (!mgl_pk_wellformed(type, dist, len) || len > c.n - pos) break; /* the walk of mgl_cost_slab refused such a slab: never taken */
		rep_advance(t, type, dist);
		pos += len;
	}
	for (; k < ncuts; k++) /* only behind a malformed entry */
		if (lane == 0) starts[k * MGL_SEG_START_WORDS] = 0u;
}

/* order[q] = i | j << 8: the span (i, j) that workgroups [q * 75, (q + 1) * 75) walk; m = ncuts - 1.
 * cost_out[s(i, j) * 75 + T], s(i, j) = i m - i (i - 1) / 2 + (j - i - 1). */
__global__ void __launch_bounds__(64) k_props_spans(DevCtx c, const mgl_pk* slab, const uint32_t* cuts, uint32_t m, const uint32_t* starts,
                                                    const uint32_t* order, uint64_t* cost_out)
{
	__shared__ uint16_t T[2048];
	__shared__ uint16_t probs[MGL_MAX_PROBS];
	const uint32_t lane = threadIdx.x;
	const uint32_t q = blockIdx.x / MGL_PROPS_NTRIPLES, triple = blockIdx.x % MGL_PROPS_NTRIPLES;
	const uint32_t ij = order[q], i = ij & 0xFFu, j = ij >> 8;
	const uint32_t lo = cuts[i];
	const uint32_t hi = cuts[j] < c.n ? cuts[j] : c.n;
	const mgl_layout L = mgl_props_triple(triple);
	for (uint32_t x = lane; x < 2048u; x += 64u) T[x] = c.cost_tbl[x];
	for (uint32_t x = lane; x < L.total; x += 64u) probs[x] = MGL_PROB_INIT;
	Walk w;
	walk_reset(w); /* ctx_state 0, rep distances 0: the state an LZMA2 state reset leaves */
	w.st.pos = lo;
	const uint32_t* s = starts + i * MGL_SEG_START_WORDS;
	RepStack t = { s[1], s[2], s[3], s[4] };
	wave_sync();
	while (w.st.pos < hi) {
		const uint32_t pos = w.st.pos;
		win_cover(w.win, c, slab, pos, lane);
		const mgl_pk pk = win_pk(w.win, pos);
		const uint32_t type = mgl_pk_type(pk), dist = mgl_pk_dist(pk), len = mgl_pk_len(pk);
		if (!mgl_pk_wellformed(type, dist, len) || len > hi - pos) break; /* refused by the host's walk: never taken */
		/* the packet in the terms of the segment's own rep stack */
		uint32_t rtype = type, rdist = dist;
		if (type == MGL_SHORT_REP) {
			if (w.st.dists[0] != t.d0) rtype = MGL_LITERAL;
		} else if (type == MGL_LONG_REP) {
			const uint32_t d = rep_at(t, dist);
			if (mgl_dist_at(&w.st, dist) != d) {
				if (w.st.dists[0] == d) rdist = 0;
				else if (w.st.dists[1] == d) rdist = 1;
				else if (w.st.dists[2] == d) rdist = 2;
				else if (w.st.dists[3] == d) rdist = 3;
				else { rtype = MGL_MATCH; rdist = d; }
			}
		}
		rep_advance(t, type, dist);
		walk_packet<true>(w, L, c.data, probs, T, rtype, rdist, len, lane);
	}
	const uint64_t total = wave_sum64(w.acc);
	if (lane == 0) cost_out[(i * m - i * (i - 1u) / 2u + (j - i - 1u)) * MGL_PROPS_NTRIPLES + triple] = total;
}
