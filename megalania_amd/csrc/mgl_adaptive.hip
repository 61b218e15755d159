/*
 * mgl_adaptive.hip -- the optimal parse of mgl_optimal.hip under adaptive prices.
 *
 * k_opt_dp prices every bit from whole-file counts, frozen for a pass.  LZMA's model adapts: here a chunk's DP runs
 * in segments, prices come from a live copy of the model, and the model is refreshed with the events of the packets
 * a segment commits.  The node step, its LDS and the resolve step are mgl_optimal.hip's (opt_node, OptLds, opt_resolve);
 * this file adds the pricer over the live model, the segments and the commits.  Two kernels, each over a batch of
 * variants of the settings (one wavefront per variant, one workgroup per chunk and variant); the single-variant entry
 * points (mgl_sa_seed_adaptive, mgl_adaptive_pass) run a batch of one:
 *
 *   k_adp_snap_sweep  per variant one wavefront, the model in LDS (as k_props_sweep holds it): walks a slab from the LZMA
 *                     initial state, costs it exactly, and leaves the walk state and a copy of the model at every chunk
 *                     start; when resolving it resolves the DP's copies on the way, as k_opt_walk does
 *   k_adp_dp_sweep    one workgroup (one wavefront) per chunk and variant: the forward shortest path, segment by segment
 *                     (the instance <true> reads its MATCH sources from the lists of mgl_matchfinder.hip, as k_opt_dp<true>);
 *                     its body, adp_dp_chunk, is shared with the per-segment parse of mgl_segparse.hip
 *
 * A variant carries its own lc/lp/pb (mgl_parse_sweep_props): the bodies take the probability layout as an argument,
 * nothing else of a parse depends on it.
 *
 * The rule is restated in plain Python in tests/test_adaptive_rule_cpu.py.
 */
#include "mgl_device.h"

/* u16 per snapshot: the model, padded to whole u32 words */
__host__ __device__ static inline uint32_t adp_stride(const mgl_layout& L) { return (L.total + 1u) & ~1u; }

/* A variant: its settings, its lc/lp/pb and where its nch snapshots start in `snaps` (in u16; the strides
 * differ from variant to variant, so the offsets are a prefix sum made on the host). */
struct AdpVariant { uint32_t cand, segment, ahead, props; uint64_t snap_off; };
__host__ __device__ static inline uint32_t adp_pack_props(uint32_t lc, uint32_t lp, uint32_t pb) { return lc | (lp << 8) | (pb << 16); }
__device__ __forceinline__ mgl_layout adp_variant_layout(const AdpVariant& t)
{
	return mgl_make_layout(t.props & 0xFFu, (t.props >> 8) & 0xFFu, (t.props >> 16) & 0xFFu);
}

/* One wavefront per variant, each walking its own parse with the live model laid out by its own triple.  Variant v reads
 * slab in_idx[v] of `in` (in_idx == nullptr: slab v; pass 0's starts are shared by the variants of one `cand`) and writes
 * slab v of `out`, its own nch chunk starts and cost[v] = the exact cost of the (resolved) parse.  Chunk start m (position
 * m x chunk) gets entry[5 m ..] = ctx_state and the four rep distances, and snaps[m x stride ..] = the model, both as they
 * stand before the packet that starts there.  A chunk start inside a packet takes the LZMA initial state and the model
 * before that packet.  snaps == nullptr: none are written. */
__global__ void __launch_bounds__(64) k_adp_snap_sweep(DevCtx c, const AdpVariant* tab, const mgl_pk* in, const uint32_t* in_idx, mgl_pk* out,
                                                       int resolve, uint32_t chunk, uint32_t nch, uint32_t* entry, uint16_t* snaps, uint64_t* cost)
{
	__shared__ uint16_t T[2048];
	__shared__ __align__(4) uint16_t probs[MGL_MAX_PROBS];
	const uint32_t lane = threadIdx.x, v = blockIdx.x;
	const AdpVariant t = tab[v];
	const mgl_layout L = adp_variant_layout(t);
	in += (size_t)(in_idx ? in_idx[v] : v) * c.n;
	if (out) out += (size_t)v * c.n;
	entry += (size_t)v * 5u * nch;
	if (snaps) snaps += t.snap_off;
	const uint32_t stride = adp_stride(L);
	for (uint32_t i = lane; i < 2048u; i += 64u) T[i] = c.cost_tbl[i];
	for (uint32_t i = lane; i < stride; i += 64u) probs[i] = MGL_PROB_INIT;
	Walk w;
	walk_reset(w);
	mgl_wstate& st = w.st;
	wave_sync();
	while (st.pos < c.n) {
		const uint32_t pos = st.pos;
		win_cover(w.win, c, in, w.st.pos, lane);
		const mgl_pk pk = win_pk(w.win, pos);
		uint32_t type = mgl_pk_type(pk), dist = mgl_pk_dist(pk), len = mgl_pk_len(pk);
		if (len == 0 || len > c.n - pos) break; /* leaves the input: never taken (see below) */
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
			opt_resolve(st, type, dist, len);
			if (lane == 0) out[pos] = mgl_pack(type, dist, len);
		}
		/* what is planned is a packet (mgl_model.h): a DP's copy is one once it is resolved (before that its distance is
		 * absolute, whatever its type), a slab from outside has been through the walk of mgl_cost_slab.  Never taken. */
		if (!mgl_pk_wellformed(type, dist, len)) break;
		walk_packet<true>(w, L, c.data, probs, T, type, dist, len, lane);
		wave_sync();
	}
	const uint64_t total = wave_sum64(w.acc);
	if (lane == 0) cost[v] = total;
}

/* the price of a bit under the live model M, through the cost table T (both in LDS) */
struct AdpLivePrices {
	const uint16_t *M, *T;
	__device__ __forceinline__ uint32_t operator()(uint32_t ctx, uint32_t bit) const
	{
		const uint32_t p = M[ctx];
		return T[bit ? 2048u - p : p];
	}
};

extern __shared__ __align__(4) uint16_t adp_model[]; /* the chunk's model: adp_stride(L) u16, sized at launch (a sweep: its largest) */

/* The shortest path of one chunk [s, e) under the live model, by one workgroup of one wavefront: settings and layout are the
 * caller's, `start` holds the five words of the chunk's walk state and `snap` its model (adp_stride(L) u16), S, T and M are
 * the workgroup's LDS.  The DP of mgl_optimal.hip runs over the nodes a..end of one segment at a time, an edge ending at `end`
 * at the latest, with prices read from the model M in LDS, which stays frozen while a segment's DP runs.  Lane 0 then reads
 * the path off the back pointers into out[] (entries that start before the commit horizon only), and the wavefront walks
 * those entries forward from the anchor: lane e applies event e of each to M, under the exact state of the path.  Where that
 * walk ends is the next anchor.  The sum of what the segments committed is added to *objective.
 *
 * back[] and out[] are indexed by absolute position (back: nodes s + 1 .. e, out: [s, e)) and are read and written by lane 0
 * alone (what the other lanes need of an entry is broadcast).  Until it is committed, an entry of out[] keeps a LONG_REP's rep
 * index above the type byte (MGL_OPT_REP_SHIFT).  k_adp_dp_sweep below and k_segp_dp (mgl_segparse.hip) are its callers. */
template <bool MF>
__device__ __forceinline__ void adp_dp_chunk(OptLds& S, uint16_t* T, uint16_t* M, const DevCtx& c, const mgl_layout& L, uint32_t cand,
                                             uint32_t segment, uint32_t ahead, uint32_t s, uint32_t e, const uint32_t* start,
                                             const uint16_t* snap, mgl_pk* back, mgl_pk* out, unsigned long long* objective, const MfLists& mf)
{
	const uint32_t lane = threadIdx.x;
	const uint8_t* d = c.data;
	const uint32_t stride = adp_stride(L);
	const AdpLivePrices price{ M, T };

	for (uint32_t k = lane; k < 2048u; k += 64u) T[k] = c.cost_tbl[k];
	{
		const uint32_t* src = (const uint32_t*)snap;
		uint32_t* dst = (uint32_t*)M;
		for (uint32_t k = lane; k < stride / 2u; k += 64u) dst[k] = src[k];
	}
	/* the anchor: position a, its exact walk state A (uniform) */
	mgl_wstate A = state_from_words(start, s);
	uint64_t obj = 0;
	__syncthreads();

	for (uint32_t a = s; a < e;) {
		const uint32_t end = (e - a) > segment + ahead ? a + segment + ahead : e;
		opt_begin(S, L, price, A); /* A.pos == a; this segment's length prices: from the model as it stands */
		for (uint32_t i = a; i < end; i++) opt_node<MF, true>(S, c, L, price, a, i, end, cand, back, mf);

		/* node `end`: take it, then read the path off the back pointers; only what starts before the horizon is kept */
		const uint32_t horizon = end == e ? e : a + segment;
		if (lane == 0) {
			mgl_wstate W;
			back[end] = opt_take<true>(S, end, W);
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
			const uint32_t dist = type == MGL_MATCH ? mgl_pk_dist(raw) - 1u : type == MGL_LONG_REP ? (uint32_t)(raw >> MGL_OPT_REP_SHIFT) & 3u : 0u;
			if (len == 0u || len > e - pos) { pos = e; break; } /* the path is contiguous: never taken */
			if (type == MGL_LONG_REP && lane == 0) out[pos] = raw & ((1ull << MGL_OPT_REP_SHIFT) - 1ull);
			mgl_plan pl;
			plan_at(L, d, A, type, dist, len, d[pos], pl); /* A.pos == pos */
			if (lane < pl.nev) {
				uint32_t ctx, bit;
				mgl_plan_event(&pl, lane, &ctx, &bit); /* no slot occurs twice in one packet */
				M[ctx] = (uint16_t)mgl_prob_update(M[ctx], bit);
			}
			mgl_advance(&A, type, dist, len);
			pos = A.pos;
			wave_sync();
		}
		obj += S.tot[pos % MGL_OPT_RING]; /* still the slot of node `pos`: it lies within 273 nodes of `end` */
		a = pos;
		__syncthreads();
	}
	if (lane == 0) atomicAdd(objective, (unsigned long long)obj);
}

/* Workgroup (m, y) runs chunk m = [s, e) of variant v = list[y], one of the variants of this instance's finder, with that
 * variant's settings and layout from `tab` and on its slice of entry, snaps, back, out and objective: adp_dp_chunk above. */
template <bool MF>
__global__ void __launch_bounds__(64) k_adp_dp_sweep(DevCtx c, const AdpVariant* tab, const uint32_t* list, uint32_t nch, const uint32_t* entry,
                                                     const uint16_t* snaps, uint32_t chunk, mgl_pk* back, mgl_pk* out,
                                                     unsigned long long* objective, MfLists mf)
{
	__shared__ OptLds S;
	__shared__ uint16_t T[2048];
	uint16_t* M = adp_model;

	const uint32_t m = blockIdx.x, v = list[blockIdx.y];
	const AdpVariant t = tab[v];
	const mgl_layout L = adp_variant_layout(t);
	const uint32_t s = m * chunk;
	const uint32_t e = (s + chunk) < c.n ? (s + chunk) : c.n;
	adp_dp_chunk<MF>(S, T, M, c, L, t.cand, t.segment, t.ahead, s, e, entry + ((size_t)v * nch + m) * 5u,
	                 snaps + t.snap_off + (size_t)m * adp_stride(L), back + (size_t)v * ((size_t)c.n + 1u), out + (size_t)v * c.n,
	                 objective + v, mf);
}
