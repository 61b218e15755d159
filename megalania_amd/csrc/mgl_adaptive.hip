/*
 * mgl_adaptive.hip -- the optimal parse of mgl_optimal.hip under adaptive prices.
 *
 * k_opt_dp prices every bit from whole-file counts, frozen for a pass.  LZMA's model adapts: here a chunk's DP runs
 * in segments, prices come from a live copy of the model, and the model is refreshed with the events of the packets
 * a segment commits.  Two kernels:
 *
 *   k_adp_snap  one wavefront, the model in LDS (as k_props_sweep holds it): walks a slab from the LZMA initial
 *               state, costs it exactly, and leaves the walk state and a copy of the model at every chunk start;
 *               when resolving it re-expresses the DP's copies against the true rep stack on the way (k_opt_walk)
 *   k_adp_dp    one workgroup (one wavefront) per chunk: k_opt_dp's forward shortest path, segment by segment (the
 *               instance <true> reads its MATCH sources from the lists of mgl_matchfinder.hip, as k_opt_dp<true>)
 *
 * k_adp_snap_sweep and k_adp_dp_sweep run the same two bodies for several variants of the settings at once (one wavefront
 * per variant, one workgroup per chunk and variant): mgl_sa_seed_sweep.  A variant carries its own lc/lp/pb there
 * (mgl_parse_sweep_props): the bodies take the probability layout as an argument, nothing else of a parse depends on it.
 *
 * The rule is restated in plain Python in tests/test_adaptive_rule_cpu.py.
 */
#include "mgl_device.h"

#define MGL_ADP_MAX_PROBS (MGL_OFF_LIT + (0x300u << 4) + 1u) /* 14 135 rounded up to an even count */
#define MGL_ADP_REP_SHIFT 56 /* back pointers and uncommitted entries keep a LONG_REP's rep index above the type byte */

/* u16 per snapshot: the model, padded to whole u32 words */
__host__ __device__ static inline uint32_t adp_stride(const mgl_layout& L) { return (L.total + 1u) & ~1u; }

/* One wavefront walks `in` with the live model laid out by L.  Chunk start m (position m x chunk) gets entry[5 m ..] = ctx_state and
 * the four rep distances, and snaps[m x stride ..] = the model, both as they stand before the packet that starts there.
 * A chunk start inside a packet takes the LZMA initial state and the model before that packet.  snaps == nullptr: none
 * are written.  *cost_out = the exact cost of the (resolved) parse. */
__device__ __forceinline__ void adp_snap_walk(const DevCtx& c, const mgl_layout L, const mgl_pk* in, mgl_pk* out, int resolve, uint32_t chunk,
                                              uint32_t* entry, uint16_t* snaps, uint64_t* cost_out)
{
	__shared__ uint16_t T[2048];
	__shared__ __align__(4) uint16_t probs[MGL_ADP_MAX_PROBS];
	const uint32_t lane = threadIdx.x;
	const uint32_t stride = adp_stride(L);
	for (uint32_t i = lane; i < 2048u; i += 64u) T[i] = c.cost_tbl[i];
	for (uint32_t i = lane; i < stride; i += 64u) probs[i] = MGL_PROB_INIT;
	Walk w;
	walk_reset(w);
	mgl_wstate& st = w.st;
	wave_sync();
	while (st.pos < c.n) {
		const uint32_t pos = st.pos;
		walk_window(w, c, in, lane);
		const mgl_pk pk = walk_slab_at(w, pos);
		uint32_t type = mgl_pk_type(pk), dist = mgl_pk_dist(pk), len = mgl_pk_len(pk);
		if (type < MGL_LITERAL || type > MGL_LONG_REP || len == 0 || len > c.n - pos) break; /* not a parse: the host validated it, never taken */
		if (snaps) {
			for (uint32_t m = (pos + chunk - 1u) / chunk; (uint64_t)m * chunk < (uint64_t)pos + len; m++) {
				const bool here = m * chunk == pos;
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
			/* the DP's copy (type, absolute distance D, len) against the true rep stack */
			if (type == MGL_LITERAL) {
				dist = 0;
			} else if (len == 1) {
				type = st.dists[0] == dist - 1u ? MGL_SHORT_REP : MGL_LITERAL;
				dist = 0;
			} else {
				const uint32_t v = dist - 1u;
				type = MGL_LONG_REP;
				if (st.dists[0] == v) dist = 0;
				else if (st.dists[1] == v) dist = 1;
				else if (st.dists[2] == v) dist = 2;
				else if (st.dists[3] == v) dist = 3;
				else { type = MGL_MATCH; dist = v; }
			}
			if (lane == 0) out[pos] = mgl_pack(type, dist, len);
		}
		uint32_t match_byte = 0, prev_byte = 0;
		if (type == MGL_LITERAL) {
			if (st.ctx_state >= 7 && st.dists[0] < pos) match_byte = c.data[pos - st.dists[0] - 1];
			if (L.lc > 0 && pos > 0) prev_byte = pos > w.wbase ? walk_byte_at(w, pos - 1u) : c.data[pos - 1];
		}
		mgl_plan pl;
		mgl_plan_packet(&L, &st, type, dist, len, walk_byte_at(w, pos), match_byte, prev_byte, &pl);
		if (lane < pl.nev) {
			uint32_t ctx, bit;
			mgl_plan_event(&pl, lane, &ctx, &bit); /* no slot occurs twice in one packet */
			const uint32_t p = probs[ctx];
			w.acc += T[bit ? 2048u - p : p];
			probs[ctx] = (uint16_t)mgl_prob_update(p, bit);
		}
		if (lane == 0) w.acc += (uint64_t)pl.ndirect << 11;
		mgl_advance(&st, type, dist, len);
		wave_sync();
	}
	const uint64_t total = wave_sum64(w.acc);
	if (lane == 0) *cost_out = total;
}

__global__ void __launch_bounds__(64) k_adp_snap(DevCtx c, const mgl_pk* in, mgl_pk* out, int resolve, uint32_t chunk,
                                                 uint32_t* entry, uint16_t* snaps, uint64_t* cost_out)
{
	adp_snap_walk(c, c.L, in, out, resolve, chunk, entry, snaps, cost_out);
}

__global__ void k_fill_literal_sweep(mgl_pk* slabs, size_t count)
{
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) slabs[i] = MGL_PK_LITERAL;
}

/* A variant of the sweeps: its settings, its lc/lp/pb and where its nch snapshots start in `snaps` (in u16; the strides
 * differ from variant to variant, so the offsets are a prefix sum made on the host). */
struct AdpVariant { uint32_t cand, segment, ahead, props; uint64_t snap_off; };
__host__ __device__ static inline uint32_t adp_pack_props(uint32_t lc, uint32_t lp, uint32_t pb) { return lc | (lp << 8) | (pb << 16); }
__device__ __forceinline__ mgl_layout adp_variant_layout(const AdpVariant& t)
{
	return mgl_make_layout(t.props & 0xFFu, (t.props >> 8) & 0xFFu, (t.props >> 16) & 0xFFu);
}

/* The sweep (mgl_sa_seed_sweep, mgl_parse_sweep_props): one wavefront per variant, each walking its own parse under its
 * own layout.  Variant v reads slab in_idx[v] of `in` (in_idx == nullptr: slab v; pass 0's starts are shared by the
 * variants of one `cand`) and writes slab v of `out`, its own nch chunk starts and cost[v]. */
__global__ void __launch_bounds__(64) k_adp_snap_sweep(DevCtx c, const AdpVariant* tab, const mgl_pk* in, const uint32_t* in_idx, mgl_pk* out,
                                                       int resolve, uint32_t chunk, uint32_t nch, uint32_t* entry, uint16_t* snaps, uint64_t* cost)
{
	const uint32_t v = blockIdx.x;
	const AdpVariant t = tab[v];
	const size_t n = c.n;
	adp_snap_walk(c, adp_variant_layout(t), in + (in_idx ? in_idx[v] : v) * n, out ? out + v * n : nullptr, resolve, chunk,
	              entry + (size_t)v * 5u * nch, snaps ? snaps + t.snap_off : nullptr, cost + v);
}

/* price of events [from, to) of a planned packet under the model M */
__device__ __forceinline__ uint32_t adp_events(const mgl_plan& pl, const uint16_t* M, const uint16_t* T, uint32_t from, uint32_t to)
{
	uint32_t s = 0;
	for (uint32_t e = from; e < to; e++) {
		uint32_t ctx, bit;
		mgl_plan_event(&pl, e, &ctx, &bit);
		const uint32_t p = M[ctx];
		s += T[bit ? 2048u - p : p];
	}
	return s;
}

extern __shared__ __align__(4) uint16_t adp_model[]; /* the chunk's model: adp_stride(L) u16, sized at launch (a sweep: its largest) */

/* One workgroup (one wavefront) per chunk [s, e).  The node loop is k_opt_dp's (same sources per lane, tie order,
 * SHORT_REP before LITERAL, states carried along winning edges, same LDS ring and the bounds stated there), run over the
 * nodes a..end of one segment at a time with cap = min(273, end - i) and prices read from the model M in LDS, which stays
 * frozen while a segment's DP runs.  Lane 0 then reads the path off the back pointers into out[] (entries that start
 * before the commit horizon only), and the wavefront walks those entries forward from the anchor: lane e applies event e
 * of each to M, under the exact state of the path.  Where that walk ends is the next anchor.
 *
 * back[] and out[] are read and written by lane 0 alone (what the other lanes need of an entry is broadcast). */
template <bool MF>
__device__ __forceinline__ void adp_dp_chunk(const DevCtx& c, const mgl_layout L, const uint32_t m, const uint32_t* entry, const uint16_t* snaps, uint32_t chunk,
                                             uint32_t cand, uint32_t segment, uint32_t ahead, mgl_pk* back, mgl_pk* out,
                                             unsigned long long* objective, const MfLists& mf)
{
	__shared__ uint64_t r_tot[MGL_OPT_RING];
	__shared__ uint64_t r_edge[MGL_OPT_RING];
	__shared__ uint32_t r_ctx[MGL_OPT_RING];
	__shared__ uint32_t r_rep[4][MGL_OPT_RING];
	__shared__ uint32_t lenp[2][16][MGL_MAX_MATCH - 1u]; /* [match, rep][pos_state][len - 2]: choice bits + tree */
	__shared__ uint32_t s_len[64];
	__shared__ uint32_t s_base[64][4];
	__shared__ uint64_t s_key[64];
	__shared__ uint16_t T[2048];
	uint16_t* M = adp_model;

	const uint32_t lane = threadIdx.x;
	const uint32_t s = m * chunk;
	const uint32_t e = (s + chunk) < c.n ? (s + chunk) : c.n;
	const uint32_t nps = 1u << L.pb;
	const uint8_t* d = c.data;
	const uint32_t stride = adp_stride(L);

	for (uint32_t k = lane; k < 2048u; k += 64u) T[k] = c.cost_tbl[k];
	{
		const uint32_t* src = (const uint32_t*)(snaps + (size_t)m * stride);
		uint32_t* dst = (uint32_t*)M;
		for (uint32_t k = lane; k < stride / 2u; k += 64u) dst[k] = src[k];
	}
	/* the anchor: position a, its exact walk state A (uniform) */
	mgl_wstate A;
	A.pos = s; A.ctx_state = entry[5u * m];
	A.dists[0] = entry[5u * m + 1u]; A.dists[1] = entry[5u * m + 2u];
	A.dists[2] = entry[5u * m + 3u]; A.dists[3] = entry[5u * m + 4u];
	uint64_t obj = 0;
	__syncthreads();

	for (uint32_t a = s; a < e;) {
		const uint32_t end = (e - a) > segment + ahead ? a + segment + ahead : e;
		/* this segment's length prices, from the model as it stands */
		for (uint32_t k = lane; k < 2u * nps * (MGL_MAX_MATCH - 1u); k += 64u) {
			const uint32_t kind = k / (nps * (MGL_MAX_MATCH - 1u)), r = k % (nps * (MGL_MAX_MATCH - 1u));
			const uint32_t ps = r / (MGL_MAX_MATCH - 1u), l = r % (MGL_MAX_MATCH - 1u) + 2u;
			mgl_plan pl;
			pl.type = MGL_MATCH; pl.nhdr = 0;
			mgl_plan_length(&pl, kind ? MGL_OFF_REP_LEN : MGL_OFF_LEN, l, ps);
			lenp[kind][ps][l - 2u] = adp_events(pl, M, T, 0, pl.len_nchoice + pl.len_tbits);
		}
		for (uint32_t k = lane; k < MGL_OPT_RING; k += 64u) r_tot[k] = ~0ull;
		__syncthreads();
		if (lane == 0) {
			const uint32_t k = a % MGL_OPT_RING;
			r_tot[k] = 0;
			r_ctx[k] = A.ctx_state;
			r_rep[0][k] = A.dists[0]; r_rep[1][k] = A.dists[1]; r_rep[2][k] = A.dists[2]; r_rep[3][k] = A.dists[3];
		}
		__syncthreads();

		for (uint32_t i = a; i < end; i++) {
			const uint32_t ki = i % MGL_OPT_RING;
			/* take node i: its state is its winning edge applied to its predecessor's */
			mgl_wstate W;
			if (i == a) {
				W = A;
			} else {
				const mgl_pk ed = r_edge[ki];
				const uint32_t et = mgl_pk_type(ed), ex = mgl_pk_dist(ed), el = mgl_pk_len(ed);
				const uint32_t kp = (i - el) % MGL_OPT_RING;
				W.ctx_state = r_ctx[kp];
				W.dists[0] = r_rep[0][kp]; W.dists[1] = r_rep[1][kp]; W.dists[2] = r_rep[2][kp]; W.dists[3] = r_rep[3][kp];
				const uint32_t absd = et == MGL_LONG_REP ? mgl_dist_at(&W, ex) + 1u : ex;
				W.pos = i - el;
				mgl_advance(&W, et, et == MGL_MATCH ? ex - 1u : ex, el);
				if (lane == 0) {
					back[i] = mgl_pack(et, absd, el) | (et == MGL_LONG_REP ? (uint64_t)ex << MGL_ADP_REP_SHIFT : 0ull);
					r_ctx[ki] = W.ctx_state;
					r_rep[0][ki] = W.dists[0]; r_rep[1][ki] = W.dists[1]; r_rep[2][ki] = W.dists[2]; r_rep[3][ki] = W.dists[3];
				}
			}
			W.pos = i;
			const uint64_t base_tot = r_tot[ki];
			const uint32_t cap = (end - i) < MGL_MAX_MATCH ? (end - i) : MGL_MAX_MATCH;
			const uint32_t ps = i & (nps - 1u);
			if (lane == 0 && i + MGL_MAX_MATCH <= end) r_tot[(i + MGL_MAX_MATCH) % MGL_OPT_RING] = ~0ull; /* slot of the node that enters the window */

			/* one source per lane: lanes 0..3 rep r, 4 .. 4 + cand - 1 the 2-byte order, then the 4-byte order; MF: lane
			 * 4 + k takes entry k of the node's match list, cut to this segment's cap */
			uint32_t slen = 0, sb0 = 0, sb1 = 0, sb2 = 0, sb3 = 0;
			uint64_t skey = 0;
			uint32_t f0 = 0, fcnt = 0;
			if (MF) { f0 = mf.off[i]; fcnt = mf.off[i + 1u] - f0; }
			if (lane < 4u) {
				const uint32_t D = mgl_dist_at(&W, lane) + 1u;
				if (D <= i && cap >= 2u) {
					while (slen < cap && d[i - D + slen] == d[i + slen]) slen++;
					if (slen >= 2u) {
						mgl_plan pl;
						mgl_plan_packet(&L, &W, MGL_LONG_REP, lane, 2u, 0u, 0u, 0u, &pl);
						sb0 = sb1 = sb2 = sb3 = adp_events(pl, M, T, 0, pl.nhdr);
					} else slen = 0;
				}
				skey = lane;
			} else if (MF) {
				if (lane - 4u < fcnt && cap >= 2u) {
					const uint32_t fl = mf.len[f0 + lane - 4u], D = i - mf.src[f0 + lane - 4u];
					slen = fl < cap ? fl : cap;
					mgl_plan pl;
					uint32_t b[4];
					for (uint32_t lc4 = 0; lc4 < 4u; lc4++) {
						mgl_plan_packet(&L, &W, MGL_MATCH, D - 1u, 2u + lc4, 0u, 0u, 0u, &pl);
						const uint32_t from = pl.nhdr + pl.len_nchoice + pl.len_tbits;
						b[lc4] = adp_events(pl, M, T, 0, pl.nhdr) + adp_events(pl, M, T, from, pl.nev) + (pl.ndirect << 11);
					}
					sb0 = b[0]; sb1 = b[1]; sb2 = b[2]; sb3 = b[3];
					skey = 5ull + D;
				}
			} else if (lane < 4u + 2u * cand && cap >= 2u && i + 1u < c.n) {
				const uint32_t src = lane < 4u + cand ? 0u : 1u, k = lane - 4u - src * cand;
				const uint32_t bigram = ((uint32_t)d[i] << 8) | d[i + 1];
				const uint32_t b_lo = c.bucket_off[bigram], b_end = c.bucket_off[bigram + 1];
				uint32_t q = 0;
				bool ok = false;
				if (src == 0) {
					const uint32_t hi = gs_lower_u32(c.bucket_pos, b_lo, b_end, i);
					if (hi - b_lo > k) { q = c.bucket_pos[hi - 1u - k]; ok = true; }
				} else if (((c.n - i) < MGL_MAX_MATCH ? (c.n - i) : MGL_MAX_MATCH) >= 4u) {
					const uint32_t x2 = ((uint32_t)d[i + 2] << 8) | d[i + 3];
					const uint32_t qa = gs_lower_u16(c.quad_nx, b_lo, b_end, x2);
					const uint32_t qb = gs_lower_u16(c.quad_nx, qa, b_end, x2 + 1u);
					const uint32_t hi = gs_lower_u32(c.quad_pos, qa, qb, i);
					if (hi - qa > k) { q = c.quad_pos[hi - 1u - k]; ok = true; }
				}
				if (ok && i - q - 1u < c.dict_limit) {
					while (slen < cap && d[q + slen] == d[i + slen]) slen++;
					if (slen >= 2u) {
						const uint32_t D = i - q;
						mgl_plan pl;
						uint32_t b[4];
						for (uint32_t lc4 = 0; lc4 < 4u; lc4++) {
							mgl_plan_packet(&L, &W, MGL_MATCH, D - 1u, 2u + lc4, 0u, 0u, 0u, &pl);
							const uint32_t from = pl.nhdr + pl.len_nchoice + pl.len_tbits;
							b[lc4] = adp_events(pl, M, T, 0, pl.nhdr) + adp_events(pl, M, T, from, pl.nev) + (pl.ndirect << 11);
						}
						sb0 = b[0]; sb1 = b[1]; sb2 = b[2]; sb3 = b[3];
						skey = 5ull + D;
					} else slen = 0;
				}
			}
			s_len[lane] = slen; s_key[lane] = skey;
			s_base[lane][0] = sb0; s_base[lane][1] = sb1; s_base[lane][2] = sb2; s_base[lane][3] = sb3;
			uint32_t maxl = slen;
			for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)maxl, o, 64); maxl = t > maxl ? t : maxl; }
			__syncthreads();

			const uint32_t nsrc = MF ? 4u + fcnt : 4u + 2u * cand;
			for (uint32_t l = 1u + lane; l <= (maxl > 1u ? maxl : 1u); l += 64u) {
				uint64_t best = ~0ull, bkey = ~0ull;
				uint32_t btype = 0, bx = 0;
				if (l == 1u) {
					/* SHORT_REP and LITERAL */
					const uint32_t r0 = W.dists[0];
					mgl_plan pl;
					if (r0 + 1u <= i && d[i] == d[i - r0 - 1u]) {
						mgl_plan_packet(&L, &W, MGL_SHORT_REP, 0u, 1u, d[i], 0u, 0u, &pl);
						best = adp_events(pl, M, T, 0, pl.nev); bkey = 4u; btype = MGL_SHORT_REP; bx = r0 + 1u;
					}
					const uint32_t mb = (W.ctx_state >= 7u && r0 < i) ? d[i - r0 - 1u] : 0u;
					const uint32_t pb = (L.lc > 0u && i > 0u) ? d[i - 1u] : 0u;
					mgl_plan_packet(&L, &W, MGL_LITERAL, 0u, 1u, d[i], mb, pb, &pl);
					const uint64_t lit = adp_events(pl, M, T, 0, pl.nev);
					if (lit < best) { best = lit; bkey = MGL_OPT_LIT_KEY; btype = MGL_LITERAL; bx = 0; }
				} else {
					const uint32_t lc4 = (l - 2u) < 3u ? (l - 2u) : 3u;
					for (uint32_t k = 0; k < nsrc; k++) {
						if (s_len[k] < l) continue;
						const uint64_t pr = (uint64_t)s_base[k][lc4] + lenp[k < 4u ? 1 : 0][ps][l - 2u];
						const uint64_t ky = s_key[k];
						if (pr < best || (pr == best && ky < bkey)) {
							best = pr; bkey = ky;
							btype = k < 4u ? MGL_LONG_REP : MGL_MATCH;
							bx = k < 4u ? k : (uint32_t)(ky - 5u);
						}
					}
				}
				if (best != ~0ull) {
					const uint64_t tot = base_tot + best;
					const uint32_t kj = (i + l) % MGL_OPT_RING;
					if (tot < r_tot[kj]) { r_tot[kj] = tot; r_edge[kj] = mgl_pack(btype, bx, l); }
				}
			}
			__syncthreads();
		}

		/* node `end`: take it, then read the path off the back pointers; only what starts before the horizon is kept */
		const uint32_t horizon = end == e ? e : a + segment;
		if (lane == 0) {
			const mgl_pk ed = r_edge[end % MGL_OPT_RING];
			const uint32_t et = mgl_pk_type(ed), ex = mgl_pk_dist(ed), el = mgl_pk_len(ed);
			const uint32_t kp = (end - el) % MGL_OPT_RING;
			mgl_wstate W;
			W.ctx_state = r_ctx[kp];
			W.dists[0] = r_rep[0][kp]; W.dists[1] = r_rep[1][kp]; W.dists[2] = r_rep[2][kp]; W.dists[3] = r_rep[3][kp];
			back[end] = et == MGL_LONG_REP ? mgl_pack(et, mgl_dist_at(&W, ex) + 1u, el) | ((uint64_t)ex << MGL_ADP_REP_SHIFT) : mgl_pack(et, ex, el);
			for (uint32_t j = end; j > a;) {
				const mgl_pk pk = back[j];
				if (mgl_pk_len(pk) == 0u || mgl_pk_len(pk) > j - a) break; /* every node has an edge: never taken */
				j -= mgl_pk_len(pk);
				if (j < horizon) out[j] = pk;
			}
		}
		/* commit: walk the kept entries from the anchor, refresh the model */
		uint32_t pos = a;
		while (pos < horizon) {
			const mgl_pk raw = uni64(lane == 0 ? out[pos] : 0ull);
			const uint32_t type = mgl_pk_type(raw), len = mgl_pk_len(raw);
			const uint32_t dist = type == MGL_MATCH ? mgl_pk_dist(raw) - 1u : type == MGL_LONG_REP ? (uint32_t)(raw >> MGL_ADP_REP_SHIFT) & 3u : 0u;
			if (len == 0u || len > e - pos) { pos = e; break; } /* the path is contiguous: never taken */
			if (type == MGL_LONG_REP && lane == 0) out[pos] = raw & ((1ull << MGL_ADP_REP_SHIFT) - 1ull);
			uint32_t match_byte = 0, prev_byte = 0;
			if (type == MGL_LITERAL) {
				if (A.ctx_state >= 7u && A.dists[0] < pos) match_byte = d[pos - A.dists[0] - 1u];
				if (L.lc > 0u && pos > 0u) prev_byte = d[pos - 1u];
			}
			mgl_plan pl;
			mgl_plan_packet(&L, &A, type, dist, len, d[pos], match_byte, prev_byte, &pl);
			if (lane < pl.nev) {
				uint32_t ctx, bit;
				mgl_plan_event(&pl, lane, &ctx, &bit); /* no slot occurs twice in one packet */
				M[ctx] = (uint16_t)mgl_prob_update(M[ctx], bit);
			}
			mgl_advance(&A, type, dist, len);
			pos = A.pos;
			wave_sync();
		}
		obj += r_tot[pos % MGL_OPT_RING]; /* still the slot of node `pos`: it lies within 273 nodes of `end` */
		a = pos;
		__syncthreads();
	}
	if (lane == 0) atomicAdd(objective, (unsigned long long)obj);
}

template <bool MF>
__global__ void __launch_bounds__(64) k_adp_dp(DevCtx c, const uint32_t* entry, const uint16_t* snaps, uint32_t chunk, uint32_t cand,
                                               uint32_t segment, uint32_t ahead, mgl_pk* back, mgl_pk* out, unsigned long long* objective,
                                               MfLists mf)
{
	adp_dp_chunk<MF>(c, c.L, blockIdx.x, entry, snaps, chunk, cand, segment, ahead, back, out, objective, mf);
}

/* The sweep: workgroup (m, y) runs chunk m of variant v = list[y], one of the variants of this instance's finder, with
 * that variant's settings and layout from `tab` and on its slice of entry, snaps, back, out and objective. */
template <bool MF>
__global__ void __launch_bounds__(64) k_adp_dp_sweep(DevCtx c, const AdpVariant* tab, const uint32_t* list, uint32_t nch, const uint32_t* entry,
                                                     const uint16_t* snaps, uint32_t chunk, mgl_pk* back, mgl_pk* out,
                                                     unsigned long long* objective, MfLists mf)
{
	const uint32_t v = list[blockIdx.y];
	const AdpVariant t = tab[v];
	const size_t n = c.n;
	adp_dp_chunk<MF>(c, adp_variant_layout(t), blockIdx.x, entry + (size_t)v * 5u * nch, snaps + t.snap_off, chunk, t.cand, t.segment, t.ahead,
	                 back + v * (n + 1u), out + v * n, objective + v, mf);
}
