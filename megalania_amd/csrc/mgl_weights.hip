/*
 * mgl_weights.hip -- cost-weighted targets: a step's K targets drawn by per-byte weights.
 *
 * Not in the reference, which draws its target over the whole slab (packet_slab_neighbour.c:162-163).  The soft form of the
 * focus window: w[x], one uint32 per input byte, S[x] = the sum of the weights below x (uint64), W = S[hi] - S[lo] over
 * the focus window in force ([0, n) without one).  Neighbour j of K draws a value v in the j-th of K equal slices of W,
 * the byte x of the window with S[x] - S[lo] <= v < S[x + 1] - S[lo] is found, and the target is the start of the packet
 * that covers x on the current walk (k_targets_weighted below has the whole rule).  All of it exact integer arithmetic.
 *
 * The prefix structure is made once per mgl_sa_set_target_weights / mgl_sa_weight_targets_by_cost, never per step:
 *
 *   k_wt_cells   a wavefront per cell of 64 positions (one word of the on-walk bitmap): the sum of its weights.
 *   k_wt_blocks  a wavefront per block of 64 cells (4 096 positions): the cell sums become exclusive prefix sums inside
 *                the block, the block's total goes to `blk`.
 *   k_wt_scan    one wavefront: the block totals become exclusive prefix sums, 64 blocks per turn; the grand total is the
 *                entry behind the last cell, pre[ncell] = S[n].
 *   k_wt_add     a thread per cell: the block's prefix is added back.  pre[c] = S[64 c].
 *
 * Plain launches behind one another on one stream, like k_rank_blocks / k_rank_scan: no workgroup waits for another.
 * Sums cannot overflow: the host refuses weights whose total reaches 2^44 before anything is launched.
 */
#include "mgl_device.h"

#define MGL_WT_CELL_SHIFT 6u  /* positions per cell: a bitmap word */
#define MGL_WT_BLOCK_CELLS 64u /* cells per block: a lane each */
#define MGL_WT_MAX_TOTAL (1ull << 44) /* S[n] below this: j W fits 64 bits at K <= 2^20 */
#define MGL_WT_MAX_K (1u << 20)
#define MGL_WT_DRAW2 0xFFFFFFFFu /* the stream index of the value's second draw, see weight_value */

__host__ __device__ __forceinline__ uint32_t wt_cells(uint32_t n) { return (n + 63u) >> MGL_WT_CELL_SHIFT; }
__host__ __device__ __forceinline__ uint32_t wt_blocks(uint32_t n) { return (wt_cells(n) + MGL_WT_BLOCK_CELLS - 1u) / MGL_WT_BLOCK_CELLS; }

/* inclusive prefix sums over the wavefront's lanes */
__device__ __forceinline__ uint64_t wave_scan64(uint64_t v, uint32_t lane)
{
	for (int o = 1; o < 64; o <<= 1) { const uint64_t t = shfl_up64(v, o); if ((int)lane >= o) v += t; }
	return v;
}

/* w[x] = map[x] + floor: the weights of mgl_sa_weight_targets_by_cost from the cost map as k_costmap_spread left it on the
 * device (an entry is below 2^20 and the host refuses a floor that could carry) */
__global__ void __launch_bounds__(256) k_wt_from_map(uint32_t n, const uint32_t* map, uint32_t floor, uint32_t* w)
{
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p < n) w[p] = map[p] + floor;
}

__global__ void __launch_bounds__(256) k_wt_cells(const uint32_t* w, uint32_t n, uint64_t* pre, uint32_t ncell)
{
	const uint32_t cell = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (cell >= ncell) return;
	const uint32_t p = (cell << MGL_WT_CELL_SHIFT) + lane;
	const uint64_t s = wave_sum64(p < n ? (uint64_t)w[p] : 0ull);
	if (lane == 0) pre[cell] = s;
}
__global__ void __launch_bounds__(64) k_wt_blocks(uint64_t* pre, uint32_t ncell, uint64_t* blk)
{
	const uint32_t lane = threadIdx.x, cell = blockIdx.x * MGL_WT_BLOCK_CELLS + lane;
	const uint64_t v = cell < ncell ? pre[cell] : 0ull;
	const uint64_t incl = wave_scan64(v, lane);
	if (cell < ncell) pre[cell] = incl - v;
	if (lane == 63u) blk[blockIdx.x] = incl;
}
__global__ void __launch_bounds__(64) k_wt_scan(uint64_t* blk, uint32_t nblk, uint64_t* pre, uint32_t ncell)
{
	const uint32_t lane = threadIdx.x;
	uint64_t base = 0; /* uniform */
	for (uint32_t b0 = 0; b0 < nblk; b0 += 64u) {
		const uint32_t i = b0 + lane;
		const uint64_t v = i < nblk ? blk[i] : 0ull;
		const uint64_t incl = wave_scan64(v, lane);
		if (i < nblk) blk[i] = base + incl - v;
		base += rdlane64(incl, 63);
	}
	if (lane == 0) pre[ncell] = base;
}
__global__ void __launch_bounds__(256) k_wt_add(uint64_t* pre, uint32_t ncell, const uint64_t* blk)
{
	const uint32_t cell = blockIdx.x * 256u + threadIdx.x;
	if (cell < ncell) pre[cell] += blk[cell / MGL_WT_BLOCK_CELLS];
}

/* S[x], x <= n: the prefix of x's cell plus the cell's weights below x.  One wavefront; uniform. */
__device__ __forceinline__ uint64_t wt_sum_below(const uint32_t* w, const uint64_t* pre, uint32_t n, uint32_t x, uint32_t lane)
{
	const uint32_t cell = x >> MGL_WT_CELL_SHIFT, p = (cell << MGL_WT_CELL_SHIFT) + lane; /* x = n, a multiple of 64: cell = ncell, no lane counts */
	const uint64_t v = (p < x && p < n) ? (uint64_t)w[p] : 0ull;
	return pre[cell] + uni64(wave_sum64(v));
}
/* what the window [lo, hi) weighs (mgl_sa_set_target_weights, mgl_sa_set_focus): out[0] = S[lo], out[1] = W = S[hi] - S[lo] */
__global__ void __launch_bounds__(64) k_wt_window(const uint32_t* w, const uint64_t* pre, uint32_t n, uint32_t lo, uint32_t hi, uint64_t* out)
{
	const uint64_t a = wt_sum_below(w, pre, n, lo, threadIdx.x), b = wt_sum_below(w, pre, n, hi, threadIdx.x);
	if (threadIdx.x == 0) { out[0] = a; out[1] = b - a; }
}

/* The value v neighbour j of K draws from W (0 < W < 2^44, K <= 2^20, so (j + 1) W fits 64 bits): uniform inside slice j of K
 * equal slices of W.  A slice can be wider than one 31-bit draw (K = 1 and a 10 MB cost map: W is about 2^38), so two draws
 * of the neighbour's stream make 62 bits: draw 0, the neighbour's target draw of the ordinal rule, and draw 0xFFFFFFFF.
 * No neighbour stream reaches that index: the streams count up from 0 one draw at a time (nbr_draw, mgl_topk.hip; rng.n
 * starts at 1 or at most 32 behind the target, mgl_kernels.hip:nbr_fullwalk_one and mgl_kernels2.hip:nbr2_one) through the mutation's
 * one draw and the picks' ten draws a turn (nine in pick_from_top_k, one for pick_best), and a neighbour's repair loop ends at
 * its guard: 4 096 or 2^20 turns in nbr2_one, n <= MGL_MAX_INPUT turns in nbr_fullwalk_one -- below 1.8e9 < 2^31 draws in all.  (The
 * accept's judge(), mgl_kernels4.hip, draws from index 2 up under the key of j = 0xFFFFFFFF, no neighbour's key: K <= 2^20.) */
__host__ __device__ __forceinline__ uint64_t weight_value(uint64_t W, uint32_t K, uint32_t j, uint64_t key)
{
	const uint64_t a = (uint64_t)j * W / K, b = ((uint64_t)j + 1ull) * W / K;
	const uint64_t u = (uint64_t)mgl_rng_draw(key, 0) << 31 | (uint64_t)mgl_rng_draw(key, MGL_WT_DRAW2);
	return a + (b > a ? u % (b - a) : 0ull);
}

/* The step's targets under weights: k_targets' sibling, one wavefront per neighbour, launched in its place when weights are
 * set and the window weighs something (W != 0; with W == 0 the ordinal rule holds and k_targets runs).  The weights, their
 * cell prefixes, S[lo] and W are arguments of this kernel only: DevCtx stays as the neighbour kernels know it.
 *   value   v = weight_value(W, K, j, key), g = S[lo] + v
 *   cell    the greatest cell c with pre[c] <= g, by a wave-uniform binary search (pre[ncell] = S[n] > g); its sum is not 0
 *   byte    x = 64 c + the first lane whose inclusive sum of the cell's weights exceeds g - pre[c]: S[x] <= g < S[x + 1],
 *           so w[x] != 0 and lo <= x < hi
 *   start   the greatest on-walk position <= x: the highest bit of x's bitmap word at or below x, going back whole words while
 *           they are empty (a packet is at most 273 bytes, so at most five words; position 0 starts a packet)
 *   window  a start below lo (the packet that covers lo reaches x): the first start in [lo, hi) takes its place, which lies
 *           no further than that packet's end; if the window holds none the start stays -- the focus rule's empty window
 * tgt[j] and the pick hint are written as k_targets writes them. */
__global__ void __launch_bounds__(256) k_targets_weighted(DevCtx c, Base2 b, const uint64_t* onwalk, uint32_t nw0, const Control* ctl, uint64_t seed, uint64_t step_override,
                                                          uint32_t K, uint32_t* tgt, unsigned char* hint, uint32_t lo, uint32_t hi, const uint32_t* w,
                                                          const uint64_t* pre, uint64_t s_lo, uint64_t W)
{
	const uint32_t j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (j >= K) return;
	const uint64_t gstep = step_override != ~0ull ? step_override : ctl->gstep;
	const uint64_t key = mgl_rng_key(seed, gstep, j);
	const uint64_t g = s_lo + weight_value(W, K, j, key);
	uint32_t cl = 0, ch = wt_cells(c.n); /* pre[cl] <= g < pre[ch] */
	while (ch - cl > 1u) { const uint32_t mid = (cl + ch) >> 1; if (pre[mid] <= g) cl = mid; else ch = mid; }
	const uint64_t rem = g - pre[cl];
	const uint32_t p = (cl << MGL_WT_CELL_SHIFT) + lane;
	const uint64_t incl = wave_scan64(p < c.n ? (uint64_t)w[p] : 0ull, lane);
	const unsigned long long has = __ballot(incl > rem);
	uint32_t x = has ? (cl << MGL_WT_CELL_SHIFT) + (uint32_t)__ffsll((long long)has) - 1u : lo; /* `has` is never 0 on a prefix structure of these weights */
	if (x >= c.n) x = c.n - 1u;
	uint32_t wi = x >> 6;
	uint64_t word = (wi < nw0 ? onwalk[wi] : 0ull) & ((2ull << (x & 63u)) - 1ull);
	while (word == 0 && wi > 0) { wi--; word = wi < nw0 ? onwalk[wi] : 0ull; }
	uint32_t t = word ? (wi << 6) + 63u - (uint32_t)__clzll((long long)word) : 0u;
	if (t < lo) {
		const uint32_t last = (hi - 1u) >> 6;
		wi = lo >> 6;
		word = (wi < nw0 ? onwalk[wi] : 0ull) & ~((1ull << (lo & 63u)) - 1ull);
		while (word == 0 && wi < last) { wi++; word = wi < nw0 ? onwalk[wi] : 0ull; }
		const uint32_t s = word ? (wi << 6) + (uint32_t)__ffsll((long long)word) - 1u : hi;
		if (s < hi) t = s;
	}
	t = uni(t);
	if (lane == 0) tgt[j] = t;
	if (hint != nullptr) {
		const bool picks = nbr_will_pick(c, b, t, key); /* uniform: t is */
		if (lane == 0) hint[j] = picks ? 1 : 0;
	}
}
