/*
 * mgl_crossover.hip -- recombine several valid parses of the input region by region.
 *
 * Not in the reference, which runs one chain.  Two valid parses can be cut at any position where both start a packet in
 * the same walk state (ctx_state and the four rep distances): on either side of such a cut the packets of either parse
 * stay valid verbatim.  Between consecutive cuts the child takes the entries of the parent that codes the stretch more
 * cheaply under its own model; one exact costing of the child then says what it is worth.
 *
 *   k_xo_walk     grid of P workgroups of one wavefront: workgroup p walks parent p from the LZMA initial state, the model
 *                 and the bit-cost table in LDS (k_props_sweep's walk under the handle's own triple).  Per packet start q
 *                 it writes the exact cost of the packets before q (u64), the five-word walk state before q and q's bit
 *                 of the parent's on-walk bitmap; cost[n] is the total.  An entry of no known type, of length 0 or
 *                 running past the end -- what k_rebuild, the walk behind mgl_cost_slab, flags -- stops the walk and
 *                 raises err[p]; total[p] is the parent's exact cost.  The child is costed by the same kernel as a batch of one.
 *   k_xo_joints   a lane per position q in 0..n: q is a joint if every parent starts a packet there in one and the same
 *                 state (q = 0 and q = n always are); a wavefront's ballot is the bitmap word.
 *   k_xo_lastnz   per bitmap word the last non-empty word at or before it (one workgroup, a running maximum), so that
 *                 "the last set bit at or before q" is two loads and a leading-zero count however long the gap is.
 *   k_xo_bounds   a lane per position: with grain g > 1 a joint q is a boundary iff a multiple of g lies in (previous
 *                 joint, q] -- q is then the first joint at or after it -- or q = n; with g <= 1 every joint is one.
 *   k_xo_winner   a lane per position: a boundary b' > 0 closes the region [b, b') behind the boundary before it; the
 *                 parent with the smallest cost[b'] - cost[b] wins it, ties to the lowest index.  winner[b] is its index.
 *   k_xo_scatter  a lane per position x < n: child[x] = the entry at x of the winner of the region x lies in.
 *   k_slab_hash   a lane per position x < n: the sum mod 2^64 of the mixed (entry, position) words of a packed slab, the word
 *                 by which the exchange of all chains' best slabs (mgl_sa_exchange_cross_all) tells equal slabs from
 *                 different ones without sending them.
 *
 * Atomics: the count of boundaries, regions_from[], the sum of the minima and the slab hash (one per wavefront each; u64
 * addition commutes, so the sums are exact).  Every index is bounded by n (or the word count) before it is used.
 */
#include "mgl_device.h"

#define MGL_XO_PARENTS 8u

/* device counters of one call */
struct XoCounters {
	unsigned long long boundaries, predicted;
	unsigned long long regions_from[MGL_XO_PARENTS];
	unsigned long long total[MGL_XO_PARENTS]; /* k_xo_walk: parent p's exact cost */
	uint32_t err[MGL_XO_PARENTS];             /* k_xo_walk: parent p is not a parse the walk accepts */
};

/* per-parent arrays side by side: parent p's begin at p * stride */
struct XoView {
	const mgl_pk* slab; /* P x n */
	uint64_t* cost;     /* P x (n + 1): cost of the packets that start before q; [n] the total */
	uint32_t* state;    /* P x 5 n: ctx_state, rep0..rep3 before the packet at q */
	uint64_t* onwalk;   /* P x nw, nw = n / 64 + 1 words (positions 0..n) */
	uint32_t nw;
};

__global__ void __launch_bounds__(64) k_xo_walk(DevCtx c, XoView v, XoCounters* cnt)
{
	__shared__ uint16_t T[2048];
	__shared__ uint16_t probs[MGL_MAX_PROBS];
	const uint32_t lane = threadIdx.x, p = blockIdx.x;
	const mgl_pk* slab = v.slab + (size_t)p * c.n;
	uint64_t* cost = v.cost + (size_t)p * ((size_t)c.n + 1u);
	uint32_t* state = v.state + (size_t)p * 5u * c.n;
	uint64_t* onwalk = v.onwalk + (size_t)p * v.nw;
	for (uint32_t i = lane; i < 2048u; i += 64u) T[i] = c.cost_tbl[i];
	for (uint32_t i = lane; i < c.L.total; i += 64u) probs[i] = MGL_PROB_INIT;
	Walk w;
	walk_reset(w);
	wave_sync();
	uint32_t word = 0;
	uint64_t bits = 0;
	bool bad = false;
	while (w.st.pos < c.n) {
		const uint32_t pos = w.st.pos;
		win_cover(w.win, c, slab, w.st.pos, lane);
		const mgl_pk pk = win_pk(w.win, pos);
		const uint32_t type = mgl_pk_type(pk), dist = mgl_pk_dist(pk), len = mgl_pk_len(pk);
		if (!mgl_pk_wellformed(type, dist, len) || len > c.n - pos) { bad = true; break; }
		const uint64_t before = wave_sum64(w.acc);
		const uint32_t pw = pos >> 6;
		if (pw != word) {
			if (lane == 0) onwalk[word] = bits;
			word = pw; bits = 0;
		}
		bits |= 1ull << (pos & 63u);
		if (lane == 0) cost[pos] = before;
		if (lane < 5u) state[(size_t)pos * 5u + lane] = lane == 0 ? w.st.ctx_state : mgl_dist_at(&w.st, lane - 1u);
		walk_packet<true>(w, c.L, c.data, probs, T, type, dist, len, lane);
	}
	const uint64_t total = wave_sum64(w.acc);
	if (lane == 0) {
		onwalk[word] = bits; /* the words the walk jumped over were cleared before the launch */
		cost[c.n] = total;
		cnt->total[p] = total;
		cnt->err[p] = bad ? 1u : 0u;
	}
}

/* q in 0..n is a joint: a wavefront covers one bitmap word */
__global__ void __launch_bounds__(256) k_xo_joints(uint32_t n, uint32_t nparents, XoView v, uint64_t* joint)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	bool is = false;
	if (q == 0u || q == n) is = true;
	else if (q < n) {
		is = true;
		for (uint32_t p = 0; p < nparents && is; p++) is = (v.onwalk[(size_t)p * v.nw + (q >> 6)] >> (q & 63u)) & 1ull;
		if (is) {
			const uint32_t* s0 = v.state + (size_t)q * 5u;
			for (uint32_t p = 1; p < nparents && is; p++) {
				const uint32_t* s = v.state + ((size_t)p * n + q) * 5u;
				is = s[0] == s0[0] && s[1] == s0[1] && s[2] == s0[2] && s[3] == s0[3] && s[4] == s0[4];
			}
		}
	}
	const unsigned long long m = __ballot(is);
	if ((threadIdx.x & 63u) == 0u && (q >> 6) < v.nw) joint[q >> 6] = m;
}

/* last[w] = 1 + the index of the last non-empty word at or before w (0: none).  One workgroup of 1024. */
__global__ void __launch_bounds__(1024) k_xo_lastnz(const uint64_t* bm, uint32_t nw, uint32_t* last)
{
	__shared__ uint32_t wave_max[16];
	__shared__ uint32_t carry_s;
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
	if (tid == 0) carry_s = 0;
	__syncthreads();
	for (uint32_t base = 0; base < nw; base += 1024u) {
		const uint32_t i = base + tid;
		uint32_t x = (i < nw && bm[i]) ? i + 1u : 0u;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64); if ((int)lane >= o && y > x) x = y; }
		if (lane == 63u) wave_max[wv] = x;
		__syncthreads();
		uint32_t pre = carry_s;
		for (uint32_t k = 0; k < wv; k++) pre = wave_max[k] > pre ? wave_max[k] : pre;
		if (pre > x) x = pre;
		if (i < nw) last[i] = x;
		__syncthreads();
		if (tid == 1023u) carry_s = x;
		__syncthreads();
	}
}

/* the last set bit at or before x; bit 0 of the bitmap is always set */
__device__ __forceinline__ uint32_t xo_last_le(const uint64_t* bm, const uint32_t* last, uint32_t x)
{
	uint32_t w = x >> 6;
	uint64_t m = bm[w] & (~0ull >> (63u - (x & 63u)));
	if (!m) {
		const uint32_t l = w ? last[w - 1u] : 0u;
		if (!l) return 0u; /* never: bit 0 is set */
		w = l - 1u;
		m = bm[w];
	}
	return (w << 6) + 63u - (uint32_t)__clzll((long long)m);
}

__global__ void __launch_bounds__(256) k_xo_bounds(uint32_t n, uint32_t nw, uint32_t grain, const uint64_t* joint, const uint32_t* jlast,
                                                   uint64_t* bound, XoCounters* cnt)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	bool is = false;
	if (q <= n && ((joint[q >> 6] >> (q & 63u)) & 1ull)) {
		if (grain <= 1u || q == 0u || q == n) is = true;
		else {
			const uint32_t prev = xo_last_le(joint, jlast, q - 1u);
			is = (q / grain) * grain > prev;
		}
	}
	const unsigned long long m = __ballot(is);
	if ((threadIdx.x & 63u) == 0u && (q >> 6) < nw) {
		bound[q >> 6] = m;
		if (m) atomicAdd(&cnt->boundaries, (unsigned long long)__popcll(m));
	}
}

__global__ void __launch_bounds__(256) k_xo_winner(uint32_t n, uint32_t nparents, const uint64_t* cost, const uint64_t* bound,
                                                   const uint32_t* blast, uint8_t* winner, XoCounters* cnt)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	const bool closes = q >= 1u && q <= n && ((bound[q >> 6] >> (q & 63u)) & 1ull);
	uint32_t win = MGL_XO_PARENTS;
	uint64_t least = 0;
	if (closes) {
		const uint32_t b = xo_last_le(bound, blast, q - 1u);
		for (uint32_t p = 0; p < nparents; p++) {
			const uint64_t* cp = cost + (size_t)p * ((size_t)n + 1u);
			const uint64_t d = cp[q] - cp[b];
			if (p == 0u || d < least) { least = d; win = p; }
		}
		winner[b] = (uint8_t)win;
	}
	const uint64_t sum = wave_sum64(least);
	if (sum && (threadIdx.x & 63u) == 0u) atomicAdd(&cnt->predicted, (unsigned long long)sum);
	for (uint32_t p = 0; p < nparents; p++) {
		const unsigned long long m = __ballot(win == p);
		if (m && (threadIdx.x & 63u) == 0u) atomicAdd(&cnt->regions_from[p], (unsigned long long)__popcll(m));
	}
}

__global__ void __launch_bounds__(256) k_xo_scatter(uint32_t n, uint32_t nparents, const mgl_pk* slabs, const uint64_t* bound,
                                                    const uint32_t* blast, const uint8_t* winner, mgl_pk* child)
{
	const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
	if (x >= n) return;
	uint32_t w = winner[xo_last_le(bound, blast, x)];
	if (w >= nparents) w = 0u; /* never: every region below n has a winner */
	child[x] = slabs[(size_t)w * n + x];
}

/* *out += the sum over x < n of fin(slab[x] + (x + 1) * 0x9E3779B97F4A7C15) mod 2^64, fin = the splitmix64 finaliser: mgl_mix64
 * adds the constant once more before it finalises, hence the x where the formula has x + 1.  Every entry counts, the stale
 * ones off the walk too: the crossover copies entries verbatim, so two slabs are the same parent only if all of them agree. */
__global__ void __launch_bounds__(256) k_slab_hash(uint32_t n, const mgl_pk* slab, unsigned long long* out)
{
	const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t h = x < n ? mgl_mix64((uint64_t)slab[x] + (uint64_t)x * 0x9E3779B97F4A7C15ull) : 0ull;
	const uint64_t sum = wave_sum64(h);
	if ((threadIdx.x & 63u) == 0u) atomicAdd(out, (unsigned long long)sum);
}
