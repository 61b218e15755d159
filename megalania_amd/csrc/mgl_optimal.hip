/*
 * mgl_optimal.hip -- a price-driven optimal parse as a starting slab.
 *
 * Not in the reference, whose search starts from the all-literal slab (main.c:71).  The same
 * shortest-path idea as the optimal parsers of LZMA encoders: bit prices, a forward dynamic
 * program over positions, rep distances carried along the best path.  The node step of that
 * program (opt_node) is written once, over a pricer: k_opt_dp below runs it under static prices,
 * mgl_adaptive.hip under the live model.  So are the resolve step (opt_resolve) that re-expresses
 * the DP's copies against the true rep stack, and the LDS the node step works in (OptLds).  Three kernels:
 *
 *   k_opt_walk    one wavefront walks a slab from the LZMA initial state: counts the zeros and
 *                 ones every probability slot sees and, when resolving, resolves the DP's copies
 *   k_opt_prices  counts -> one price per (slot, bit), in cost units (2048 per bit)
 *   k_opt_dp      one workgroup per chunk [s, e): forward shortest path over the nodes s..e; the instance <true>
 *                 takes a node's MATCH sources from the lists of mgl_matchfinder.hip instead of searching for them
 *
 * Prices: p0 = clamp(floor(2048 (n0 + 1) / (n0 + n1 + 2)), 1, 2047), price0 = T[p0], price1 =
 * T[2048 - p0]; direct bits cost 2048 as on the costing path.  The rule of k_opt_dp is restated
 * in plain Python in tests/test_gpu_optimal.py.
 */
#include "mgl_device.h"

#define MGL_OPT_RING 1024u   /* LDS ring of node records: > 273 nodes ahead + 273 behind the node being taken */
#define MGL_OPT_MAX_CAND 30u /* 4 rep lanes + 2 x cand match lanes fit one wavefront */
#define MGL_OPT_MIN_CHUNK 512u
#define MGL_OPT_LIT_KEY (1ull << 40)
#define MGL_OPT_REP_SHIFT 56 /* where a back pointer keeps a LONG_REP's rep index, above the type byte (opt_take<true>) */

/* the DP's copy (type, absolute distance D, len) against the true rep stack */
__device__ __forceinline__ void opt_resolve(const mgl_wstate& st, uint32_t& type, uint32_t& dist, uint32_t len)
{
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
}

/* ---- one wavefront: walk a slab, count the bits of every slot; resolve = re-express the DP's copies on the way */
__global__ void __launch_bounds__(64) k_opt_walk(DevCtx c, const mgl_pk* in, mgl_pk* out, uint32_t* counts, int resolve,
                                                 uint32_t chunk, uint32_t* entry)
{
	const uint32_t lane = threadIdx.x;
	mgl_wstate st = state_initial();
	while (st.pos < c.n) {
		const uint32_t pos = st.pos;
		const mgl_pk pk = in[pos];
		uint32_t type = mgl_pk_type(pk), dist = mgl_pk_dist(pk), len = mgl_pk_len(pk);
		if (len == 0 || len > c.n - pos) break; /* not a parse (mgl_optimal_prices validates its slab first) */
		if (resolve) {
			if (entry && pos % chunk == 0 && lane == 0) {
				uint32_t* w = entry + 5u * (pos / chunk);
				w[0] = st.ctx_state; w[1] = st.dists[0]; w[2] = st.dists[1]; w[3] = st.dists[2]; w[4] = st.dists[3];
			}
			opt_resolve(st, type, dist, len);
			if (lane == 0) out[pos] = mgl_pack(type, dist, len);
		}
		if (!mgl_pk_wellformed(type, dist, len)) break; /* only packets are planned (mgl_model.h): a resolved copy is one. Never taken */
		mgl_plan pl;
		plan_at(c.L, c.data, st, type, dist, len, c.data[pos], pl);
		if (lane < pl.nev) {
			uint32_t ctx, bit;
			mgl_plan_event(&pl, lane, &ctx, &bit);
			atomicAdd(&counts[2u * ctx + bit], 1u); /* no slot occurs twice in one packet */
		}
		mgl_advance(&st, type, dist, len);
	}
}

__global__ void __launch_bounds__(256) k_opt_prices(const uint32_t* counts, const uint16_t* T, uint32_t total, uint32_t* prices)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= total) return;
	const uint64_t n0 = counts[2u * k], n1 = counts[2u * k + 1u];
	uint64_t p0 = (2048u * (n0 + 1u)) / (n0 + n1 + 2u);
	p0 = p0 < 1u ? 1u : (p0 > 2047u ? 2047u : p0);
	prices[2u * k] = T[p0];
	prices[2u * k + 1u] = T[2048u - p0];
}

/* Where the price of a bit comes from: here the pass's table of static prices; mgl_adaptive.hip has the live model's */
struct OptStaticPrices {
	const uint32_t* prices;
	__device__ __forceinline__ uint32_t operator()(uint32_t ctx, uint32_t bit) const { return prices[2u * ctx + bit]; }
};

/* price of events [from, to) of a planned packet */
template <class P>
__device__ __forceinline__ uint32_t opt_events(const mgl_plan& pl, const P& price, uint32_t from, uint32_t to)
{
	uint32_t s = 0;
	for (uint32_t e = from; e < to; e++) {
		uint32_t ctx, bit;
		mgl_plan_event(&pl, e, &ctx, &bit);
		s += price(ctx, bit);
	}
	return s;
}

/* What one workgroup (one wavefront) of a DP holds in LDS.
 *
 * Node record, in a ring indexed by position mod MGL_OPT_RING: tot = the smallest total found so far for reaching the
 * node, edge = the edge that gave it (type, rep index or absolute distance, len), and -- once the node is taken -- its walk
 * state (ctx, rep).  Bound: a packet costs at most 26 events x T[1] (22 528) + 26 direct bits x 2 048 < 2^20, and the
 * cheapest path to any node is at most 9 x 22 528 < 2^18 per byte, so every total a node ever compares is below
 * 2^18 x chunk + 2^20: u64 cannot overflow for any input a handle accepts (n < 2^32).  Slots for i + 1 .. i + 273 are live
 * ahead of node i and the states of i - 273 .. i behind it, 547 < MGL_OPT_RING. */
struct OptLds {
	uint64_t tot[MGL_OPT_RING];
	uint64_t edge[MGL_OPT_RING];
	uint32_t ctx[MGL_OPT_RING];
	uint32_t rep[4][MGL_OPT_RING];
	uint32_t lenp[2][16][MGL_MAX_MATCH - 1u]; /* [match, rep][pos_state][len - 2]: choice bits + tree */
	uint32_t s_len[64];                       /* per lane: its source's length, base prices by min(len - 2, 3), tie key */
	uint32_t s_base[64][4];
	uint64_t s_key[64];
};

__device__ __forceinline__ void opt_ring_get(const OptLds& S, uint32_t k, mgl_wstate& W)
{
	W.ctx_state = S.ctx[k];
	W.dists[0] = S.rep[0][k]; W.dists[1] = S.rep[1][k]; W.dists[2] = S.rep[2][k]; W.dists[3] = S.rep[3][k];
}
__device__ __forceinline__ void opt_ring_put(OptLds& S, uint32_t k, const mgl_wstate& W)
{
	S.ctx[k] = W.ctx_state;
	S.rep[0][k] = W.dists[0]; S.rep[1][k] = W.dists[1]; S.rep[2][k] = W.dists[2]; S.rep[3][k] = W.dists[3];
}

/* A DP starts at node A.pos in the exact walk state A: the length prices as `price` stands, an empty ring, A in its slot */
template <class P>
__device__ __forceinline__ void opt_begin(OptLds& S, const mgl_layout& L, const P& price, const mgl_wstate& A)
{
	const uint32_t lane = threadIdx.x, nps = 1u << L.pb;
	for (uint32_t k = lane; k < 2u * nps * (MGL_MAX_MATCH - 1u); k += 64u) {
		const uint32_t kind = k / (nps * (MGL_MAX_MATCH - 1u)), r = k % (nps * (MGL_MAX_MATCH - 1u));
		const uint32_t ps = r / (MGL_MAX_MATCH - 1u), l = r % (MGL_MAX_MATCH - 1u) + 2u;
		mgl_plan pl;
		pl.type = MGL_MATCH; pl.nhdr = 0;
		mgl_plan_length(&pl, kind ? MGL_OFF_REP_LEN : MGL_OFF_LEN, l, ps);
		S.lenp[kind][ps][l - 2u] = opt_events(pl, price, 0, pl.len_nchoice + pl.len_tbits);
	}
	for (uint32_t k = lane; k < MGL_OPT_RING; k += 64u) S.tot[k] = ~0ull;
	__syncthreads();
	if (lane == 0) {
		S.tot[A.pos % MGL_OPT_RING] = 0;
		opt_ring_put(S, A.pos % MGL_OPT_RING, A);
	}
	__syncthreads();
}

/* Take node j (not a DP's first): W = its state, which is its winning edge applied to its predecessor's.  Returns the back
 * pointer (type, absolute distance, len); REP_IDX: a LONG_REP's rep index rides above the type byte, for a caller that
 * walks the path forward again without a rep stack to look the distance up in. */
template <bool REP_IDX>
__device__ __forceinline__ mgl_pk opt_take(const OptLds& S, uint32_t j, mgl_wstate& W)
{
	const mgl_pk ed = S.edge[j % MGL_OPT_RING];
	const uint32_t et = mgl_pk_type(ed), ex = mgl_pk_dist(ed), el = mgl_pk_len(ed);
	opt_ring_get(S, (j - el) % MGL_OPT_RING, W);
	const uint32_t absd = et == MGL_LONG_REP ? mgl_dist_at(&W, ex) + 1u : ex;
	W.pos = j - el;
	mgl_advance(&W, et, et == MGL_MATCH ? ex - 1u : ex, el);
	return mgl_pack(et, absd, el) | (REP_IDX && et == MGL_LONG_REP ? (uint64_t)ex << MGL_OPT_REP_SHIFT : 0ull);
}

/* b[min(len - 2, 3)] = what a MATCH at distance D costs in state W beside its length's choice bits and tree */
template <class P>
__device__ __forceinline__ void opt_match_base(const mgl_layout& L, const mgl_wstate& W, const P& price, uint32_t D, uint32_t b[4])
{
	for (uint32_t lc4 = 0; lc4 < 4u; lc4++) {
		mgl_plan pl;
		mgl_plan_packet(&L, &W, MGL_MATCH, D - 1u, 2u + lc4, 0u, 0u, 0u, &pl);
		const uint32_t from = pl.nhdr + pl.len_nchoice + pl.len_tbits;
		b[lc4] = opt_events(pl, price, 0, pl.nhdr) + opt_events(pl, price, from, pl.nev) + (pl.ndirect << 11);
	}
}

/* The node step of a DP over the nodes a..end that opt_begin started at a: take node i, find one source per lane, relax
 * every edge out of i (an edge ends at `end` at the latest).  back[j] (global) = the winning edge into node j, written as
 * j is taken. */
template <bool MF, bool REP_IDX, class P>
__device__ __forceinline__ void opt_node(OptLds& S, const DevCtx& c, const mgl_layout& L, const P& price, uint32_t a, uint32_t i, uint32_t end,
                                         uint32_t cand, mgl_pk* back, const MfLists& mf)
{
	const uint32_t lane = threadIdx.x, nps = 1u << L.pb, ki = i % MGL_OPT_RING;
	const uint8_t* d = c.data;
	mgl_wstate W;
	if (i == a) {
		opt_ring_get(S, ki, W);
	} else {
		const mgl_pk bk = opt_take<REP_IDX>(S, i, W);
		if (lane == 0) {
			back[i] = bk;
			opt_ring_put(S, ki, W);
		}
	}
	W.pos = i;
	const uint64_t base_tot = S.tot[ki];
	const uint32_t cap = (end - i) < MGL_MAX_MATCH ? (end - i) : MGL_MAX_MATCH;
	const uint32_t ps = i & (nps - 1u);
	if (lane == 0 && i + MGL_MAX_MATCH <= end) S.tot[(i + MGL_MAX_MATCH) % MGL_OPT_RING] = ~0ull; /* slot of the node that enters the window */

	/* one source per lane: lanes 0..3 rep r, 4 .. 4 + cand - 1 the 2-byte order, then the 4-byte order; MF: lane 4 + k
	 * takes entry k of the node's match list, whose length is known (no bytes are compared), cut to cap */
	uint32_t slen = 0, sb[4] = { 0, 0, 0, 0 };
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
				sb[0] = sb[1] = sb[2] = sb[3] = opt_events(pl, price, 0, pl.nhdr);
			} else slen = 0;
		}
		skey = lane;
	} else if (MF) {
		if (lane - 4u < fcnt && cap >= 2u) {
			const uint32_t fl = mf.len[f0 + lane - 4u], D = i - mf.src[f0 + lane - 4u];
			slen = fl < cap ? fl : cap;
			opt_match_base(L, W, price, D, sb);
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
				opt_match_base(L, W, price, D, sb);
				skey = 5ull + D;
			} else slen = 0;
		}
	}
	S.s_len[lane] = slen; S.s_key[lane] = skey;
	for (uint32_t k = 0; k < 4u; k++) S.s_base[lane][k] = sb[k];
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
				best = opt_events(pl, price, 0, pl.nev); bkey = 4u; btype = MGL_SHORT_REP; bx = r0 + 1u;
			}
			const uint32_t mb = (W.ctx_state >= 7u && r0 < i) ? d[i - r0 - 1u] : 0u;
			const uint32_t pb = (L.lc > 0u && i > 0u) ? d[i - 1u] : 0u;
			mgl_plan_packet(&L, &W, MGL_LITERAL, 0u, 1u, d[i], mb, pb, &pl);
			const uint64_t lit = opt_events(pl, price, 0, pl.nev);
			if (lit < best) { best = lit; bkey = MGL_OPT_LIT_KEY; btype = MGL_LITERAL; bx = 0; }
		} else {
			const uint32_t lc4 = (l - 2u) < 3u ? (l - 2u) : 3u;
			for (uint32_t k = 0; k < nsrc; k++) {
				if (S.s_len[k] < l) continue;
				const uint64_t pr = (uint64_t)S.s_base[k][lc4] + S.lenp[k < 4u ? 1 : 0][ps][l - 2u];
				const uint64_t ky = S.s_key[k];
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
			if (tot < S.tot[kj]) { S.tot[kj] = tot; S.edge[kj] = mgl_pack(btype, bx, l); }
		}
	}
	__syncthreads();
}

/* One workgroup (one wavefront) per chunk [s, e) of `chunk` bytes, under static prices, from the state in entry[5 x chunk ..]
 * (entry == nullptr: the LZMA initial state).  back[] has n + 1 entries; the chunk's parse is read off it from e backwards
 * into out[] (position-indexed; positions off the path keep their literal). */
template <bool MF>
__global__ void __launch_bounds__(64) k_opt_dp(DevCtx c, const uint32_t* prices, const uint32_t* entry, uint32_t chunk,
                                               uint32_t cand, mgl_pk* back, mgl_pk* out, unsigned long long* objective, MfLists mf)
{
	__shared__ OptLds S;
	const uint32_t s = blockIdx.x * chunk;
	const uint32_t e = (s + chunk) < c.n ? (s + chunk) : c.n;
	const OptStaticPrices price{ prices };
	mgl_wstate A;
	A.pos = s; A.ctx_state = entry ? entry[5u * blockIdx.x] : 0u;
	for (uint32_t r = 0; r < 4; r++) A.dists[r] = entry ? entry[5u * blockIdx.x + 1u + r] : 0u;
	opt_begin(S, c.L, price, A);
	for (uint32_t i = s; i < e; i++) opt_node<MF, false>(S, c, c.L, price, s, i, e, cand, back, mf);

	/* node e: take it, then read the path off the back pointers */
	if (threadIdx.x == 0) {
		mgl_wstate W;
		if (e > s) back[e] = opt_take<false>(S, e, W);
		atomicAdd(objective, (unsigned long long)S.tot[e % MGL_OPT_RING]);
		for (uint32_t j = e; j > s;) {
			const mgl_pk pk = back[j];
			j -= mgl_pk_len(pk);
			out[j] = pk;
		}
	}
}
