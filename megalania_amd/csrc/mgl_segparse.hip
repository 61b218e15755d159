/*
 * mgl_segparse.hip -- the adaptive parse of mgl_adaptive.hip run per segment, each from the LZMA2 state reset at its cut and
 * under its own lc/lp/pb ("Segment re-parse"; include/megalania_hip.h has the rule).
 *
 * Segment props (mgl_segments.hip) only chooses how a finished parse is written: its packets were priced for one triple and
 * one running model, and are then coded behind resets under other triples.  Here a segment [lo, hi) is parsed again for the
 * coder that will run on it: a fresh model under the segment's triple, ctx_state 0, rep distances (0, 0, 0, 0) at lo, a
 * chunk grid that starts at lo, and no packet across hi -- while MATCH sources stay absolute positions of the whole
 * dictionary, so copies still reach below lo.  One variant is one segment (at most MGL_SEG_MAX_CUTS - 1); the segments tile
 * [0, n), so they share one position-indexed dp buffer and one back buffer.  Three kernels:
 *
 *   k_segp_walk  one wavefront per segment, model and cost table in LDS: walks the segment from the reset, costs it exactly
 *                and leaves walk state and model at every chunk start (k_adp_snap_sweep's convention for a chunk start inside
 *                a packet).  Its input is either a slab, whose rep packets are named again against the segment's stack as
 *                k_props_spans does (pass 0's starts; the cost of the joined slab), or a DP's copies, resolved against the
 *                segment coder's own state by opt_resolve (pass p's cost, pass p + 1's starts).
 *   k_segp_dp    workgroup (m, s): chunk m of segment s, adp_dp_chunk of mgl_adaptive.hip; a segment with fewer chunks than
 *                the grid is wide leaves at once.
 *   k_segp_join  one wavefront, no model: one walk from byte 0 that takes, per segment, the input's packets (made absolute
 *                through the input's own rep stack) or the kept DP copies, and resolves each against the output's running
 *                stack, so that the result is an ordinary slab whose rep packets name the stack of its walk from byte 0.
 *
 * The walks keep the guards of their neighbours: an entry of no known type, of length 0 or running past its stretch ends
 * the walk.  The rule is restated in plain Python in tests/_segment_parse.py.
 */
#include "mgl_device.h"

/* A segment: where it lies, its triple (adp_pack_props), the settings, its first chunk's index among all segments' chunks
 * (entry holds five words per chunk), how many chunks it has and where its snapshots start in `snaps` (in u16). */
struct SegVariant { uint32_t lo, hi, props, cand, segment, ahead, ch_off, nch; uint64_t snap_off; };
__device__ __forceinline__ mgl_layout segp_layout(const SegVariant& t)
{
	return mgl_make_layout(t.props & 0xFFu, (t.props >> 8) & 0xFFu, (t.props >> 16) & 0xFFu);
}

/* Segment v = blockIdx.x.  resolve == 0: `in` is a valid slab and starts[v x MGL_SEG_START_WORDS ..] holds its true rep stack
 * at lo (k_seg_starts over the segments' cuts); resolve != 0: `in` holds a DP's copies (type, absolute distance, len).
 * Chunk start m of the segment (position lo + m x chunk) gets entry[5 (ch_off + m) ..] and snaps[snap_off + m x stride ..]
 * as they stand before the packet that starts there; snaps == nullptr: neither is written.  cost[v] = the exact cost. */
__global__ void __launch_bounds__(64) k_segp_walk(DevCtx c, const SegVariant* tab, const mgl_pk* in, int resolve, uint32_t chunk,
                                                  const uint32_t* starts, uint32_t* entry, uint16_t* snaps, uint64_t* cost)
{
	__shared__ uint16_t T[2048];
	__shared__ __align__(4) uint16_t probs[MGL_MAX_PROBS];
	const uint32_t lane = threadIdx.x, v = blockIdx.x;
	const SegVariant t = tab[v];
	const mgl_layout L = segp_layout(t);
	const uint32_t lo = t.lo, hi = t.hi < c.n ? t.hi : c.n;
	const uint32_t stride = adp_stride(L);
	entry += (size_t)t.ch_off * 5u;
	if (snaps) snaps += t.snap_off;
	for (uint32_t i = lane; i < 2048u; i += 64u) T[i] = c.cost_tbl[i];
	for (uint32_t i = lane; i < stride; i += 64u) probs[i] = MGL_PROB_INIT;
	Walk w;
	walk_reset(w); /* ctx_state 0, rep distances 0: the state an LZMA2 state reset leaves */
	w.st.pos = lo;
	mgl_wstate& st = w.st;
	RepStack tr = { 0, 0, 0, 0 };
	if (!resolve) {
		const uint32_t* s = starts + v * MGL_SEG_START_WORDS;
		tr.d0 = s[1]; tr.d1 = s[2]; tr.d2 = s[3]; tr.d3 = s[4];
	}
	wave_sync();
	while (st.pos < hi) {
		const uint32_t pos = st.pos;
		win_cover(w.win, c, in, pos, lane);
		const mgl_pk pk = win_pk(w.win, pos);
		uint32_t type = mgl_pk_type(pk), dist = mgl_pk_dist(pk), len = mgl_pk_len(pk);
		if (len == 0 || len > hi - pos) break; /* leaves the segment: never taken */
		if (snaps) {
			for (uint32_t m = (pos - lo + chunk - 1u) / chunk; m < t.nch && (uint64_t)lo + (uint64_t)m * chunk < (uint64_t)pos + len; m++) {
				const bool here = lo + m * chunk == pos;
				if (lane < 5u) {
					const uint32_t word = lane == 0 ? st.ctx_state : mgl_dist_at(&st, lane - 1u);
					entry[5u * m + lane] = here ? word : 0u;
				}
				uint32_t* dst = (uint32_t*)(snaps + (size_t)m * stride);
				const uint32_t* src = (const uint32_t*)probs;
				for (uint32_t k = lane; k < stride / 2u; k += 64u) dst[k] = src[k];
			}
		}
		if (resolve) {
			opt_resolve(st, type, dist, len);
		} else {
			if (!mgl_pk_wellformed(type, dist, len)) break; /* refused by the host's walk: never taken */
			/* the packet in the terms of the segment's own rep stack (k_props_spans) */
			const uint32_t otype = type, odist = dist;
			if (type == MGL_SHORT_REP) {
				if (st.dists[0] != tr.d0) type = MGL_LITERAL;
			} else if (type == MGL_LONG_REP) {
				const uint32_t d = rep_at(tr, dist);
				if (mgl_dist_at(&st, dist) != d) {
					if (st.dists[0] == d) dist = 0;
					else if (st.dists[1] == d) dist = 1;
					else if (st.dists[2] == d) dist = 2;
					else if (st.dists[3] == d) dist = 3;
					else { type = MGL_MATCH; dist = d; }
				}
			}
			rep_advance(tr, otype, odist);
		}
		/* what is planned is a packet (mgl_model.h): a DP's copy is one once it is resolved.  Never taken. */
		if (!mgl_pk_wellformed(type, dist, len)) break;
		walk_packet<true>(w, L, c.data, probs, T, type, dist, len, lane);
		wave_sync();
	}
	const uint64_t total = wave_sum64(w.acc);
	if (lane == 0) cost[v] = total;
}

/* Workgroup (m, y): chunk m = [lo + m x chunk, min(lo + (m + 1) x chunk, hi)) of segment y, from the starts k_segp_walk left,
 * into the shared position-indexed back (n + 1) and out (n) and the segment's own objective. */
template <bool MF>
__global__ void __launch_bounds__(64) k_segp_dp(DevCtx c, const SegVariant* tab, const uint32_t* entry, const uint16_t* snaps, uint32_t chunk,
                                                mgl_pk* back, mgl_pk* out, unsigned long long* objective, MfLists mf)
{
	__shared__ OptLds S;
	__shared__ uint16_t T[2048];
	uint16_t* M = adp_model;

	const uint32_t m = blockIdx.x, v = blockIdx.y;
	const SegVariant t = tab[v];
	if (m >= t.nch) return; /* uniform: the whole workgroup leaves */
	const mgl_layout L = segp_layout(t);
	const uint32_t hi = t.hi < c.n ? t.hi : c.n;
	const uint32_t s = t.lo + m * chunk; /* below hi: m < nch = ceil((hi - lo) / chunk) */
	const uint32_t e = (hi - s) > chunk ? s + chunk : hi;
	adp_dp_chunk<MF>(S, T, M, c, L, t.cand, t.segment, t.ahead, s, e, entry + ((size_t)t.ch_off + m) * 5u,
	                 snaps + t.snap_off + (size_t)m * adp_stride(L), back, out, objective + v, mf);
}

/* One walk from byte 0 over the nseg segments of `tab`.  take[v] == 0: segment v keeps the packets of `in` (a valid slab whose
 * true rep stack at every cut is in `starts`), each made a copy of absolute distance through the input's stack; otherwise it
 * takes the DP copies in `keep`.  Every copy is resolved against the output's own running stack and written to out[], whose
 * entries off the walk the caller has filled with literals.  done[0] = the position the walk reached (n unless it met a
 * malformed entry). */
__global__ void __launch_bounds__(64) k_segp_join(DevCtx c, const SegVariant* tab, uint32_t nseg, const uint32_t* take, const mgl_pk* in,
                                                  const mgl_pk* keep, const uint32_t* starts, mgl_pk* out, uint32_t* done)
{
	const uint32_t lane = threadIdx.x;
	Win win;
	mgl_wstate o = state_initial(); /* the output's walk: its rep stack is what opt_resolve reads */
	for (uint32_t v = 0; v < nseg; v++) {
		const SegVariant t = tab[v];
		const uint32_t hi = t.hi < c.n ? t.hi : c.n;
		const bool dp = take[v] != 0u;
		const mgl_pk* src = dp ? keep : in;
		const uint32_t* s = starts + v * MGL_SEG_START_WORDS;
		RepStack tr = { s[1], s[2], s[3], s[4] };
		win_reset(win); /* the source changes at a cut */
		if (o.pos != t.lo) break; /* behind a malformed entry only */
		while (o.pos < hi) {
			const uint32_t pos = o.pos;
			win_cover(win, c, src, pos, lane);
			const mgl_pk pk = win_pk(win, pos);
			uint32_t type = mgl_pk_type(pk), dist = mgl_pk_dist(pk), len = mgl_pk_len(pk);
			if (len == 0 || len > hi - pos) break; /* never taken */
			if (!dp) {
				if (!mgl_pk_wellformed(type, dist, len)) break; /* refused by the host's walk: never taken */
				const uint32_t otype = type, odist = dist;
				if (type == MGL_MATCH) dist = dist + 1u;
				else if (type == MGL_SHORT_REP) dist = tr.d0 + 1u;
				else if (type == MGL_LONG_REP) dist = rep_at(tr, dist) + 1u;
				rep_advance(tr, otype, odist);
			}
			opt_resolve(o, type, dist, len);
			if (!mgl_pk_wellformed(type, dist, len)) break; /* a resolved copy is a packet: never taken */
			if (lane == 0) out[pos] = mgl_pack(type, dist, len);
			mgl_advance(&o, type, dist, len);
		}
		if (o.pos != hi) break;
	}
	if (lane == 0) done[0] = o.pos;
}
