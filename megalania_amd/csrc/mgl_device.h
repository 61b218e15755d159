/*
 * mgl_device.h -- device-side building blocks shared by every kernel file of the library (mgl_api.hip includes them all as one translation unit).
 * gfx950 only: 64-lane wavefronts, probabilities and the bit-cost table in LDS.
 *
 * Conventions
 *   - one wavefront works on one slab walk.  Control flow is wave-uniform; walk state
 *     (position, ctx_state, rep distances) is kept in scalar registers via readfirstlane.
 *   - lane e of the wave evaluates event slot e of the current packet (mgl_model.h), so a
 *     packet costs one LDS read-modify-write round trip; per-lane u64 partial sums are
 *     reduced once at the end (u64 addition commutes, so the total is bit-exact).
 *   - the walk reads the slab and the input through a 64-position register window
 *     (one coalesced load per 64 bytes of input) and fetches entries with v_readlane.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mgl_model.h"
#include "mgl_words.h"

#define MGL_WAVE 64
#define MGL_CKPT_SHIFT 10u          /* one prefix checkpoint per 1024 input bytes */
#define MGL_MAX_DIFFS 64u           /* journal capacity per neighbour */
#define MGL_MAX_REPAIR_PICKS 8u /* top-K picks one neighbour's repair may need before it is given up and dropped (every one is a model
                                * reconstruction + a top-K query in the middle of the walk); the oracle counts the same picks */
#define MGL_MAX_WALK 2048u   /* neighbour packets the two-pointer walk visits (skipped literal runs do not count) before the neighbour is
                            * given up and dropped: rep distances that no match ever flushes (long runs coded as rep matches) keep two
                            * walks apart for kilobytes; the oracle counts the same packets */
#define MGL_MAX_TOPK 32u
#define MGL_PRICE_WORDS 1072u         /* top-K price tables per wavefront (u32): the layout below */
/* The price tables of one top-K query (mgl_topk.hip), the way LZMA encoders price candidates (lzma_packet_encoder.c:42-104), in
 * u32 words from the wavefront's table base.  Lengths 2..17 are priced when a query starts, 18.. (the 8-bit high tree) only
 * when a match that long shows up. */
enum PriceOff : uint32_t {
	PT_LEN_MATCH = 0,                      /* match coder: price of length l at [l - 2], l = 2..273 */
	PT_LEN_REP = PT_LEN_MATCH + 272u,      /* rep coder: the same */
	PT_SLOT = PT_LEN_REP + 272u,           /* distance slot s in length context k (lengths 2, 3, 4, 5+) at [64 k + s] */
	PT_TAIL = PT_SLOT + 4u * 64u,          /* reverse-tree tail of every distance below 128 */
	PT_ALIGN = PT_TAIL + 128u,             /* the four align bits */
	PT_LBSLOT = PT_ALIGN + 16u,            /* per slot: the least a distance of that slot costs in any length context (pruning bound) */
	PT_SUFMIN = PT_LBSLOT + 64u,           /* [s] = the least of lbslot[s..63] */
	PT_END = PT_SUFMIN + 64u
};
static_assert(PT_END == MGL_PRICE_WORDS, "the price tables' parts add up to MGL_PRICE_WORDS");
struct PriceTab { uint32_t *len_m, *len_r, *slot, *tail, *align, *lbslot, *sufmin; };
__device__ __forceinline__ PriceTab price_tab(uint32_t* base)
{
	PriceTab p;
	p.len_m = base + PT_LEN_MATCH; p.len_r = base + PT_LEN_REP; p.slot = base + PT_SLOT; p.tail = base + PT_TAIL;
	p.align = base + PT_ALIGN; p.lbslot = base + PT_LBSLOT; p.sufmin = base + PT_SUFMIN;
	return p;
}
#define MGL_SEQ_MASK ((1ull << 44) - 1ull)
#define MGL_INVALID_COST (~0ull)

struct DevCtx {
	const uint8_t* data;        /* n bytes (+64 bytes of zero padding) */
	uint32_t n;
	const uint32_t* bucket_off; /* 65537 */
	const uint32_t* bucket_pos; /* n-1 positions, ascending inside each bigram bucket */
	const uint16_t* bucket_nx;  /* per entry of bucket_pos: data[p + 2] | data[p + 3] << 8 */
	const uint32_t* quad_pos;   /* the same positions ordered by (data[p..p+3], p): inside a bigram bucket, runs of equal next-two-bytes */
	const uint16_t* quad_nx;    /* per entry of quad_pos: data[p + 2] << 8 | data[p + 3] (ascending inside a bucket) */
	/* deeper orders of the same positions (mgl_index.hip): sorted by the first 4 / 8 / 16 bytes, then by position.
	 * Per order: rank[p] = where position p sits; run[i] = first entry of the run of equal prefixes entry i belongs
	 * to (so the earlier positions that share p's prefix are exactly entries [run[rank[p]], rank[p])); and the
	 * bytes that follow the prefix, so that a hit's match length is known up to the next order's prefix without
	 * touching the input */
	/* the exact-length sources, D = 2..7 (index D - 2): positions ordered by their first D bytes then by position
	 * (D = 2: the bigram bucket itself, D = 4: quad_pos), rank / run as above (unused for D = 2: the bucket bounds
	 * play that part), and byte D of every entry: an entry whose byte D equals the target's belongs to the next
	 * source, all others match exactly D bytes */
	const uint32_t* xpos[6]; const uint32_t* xrank[6]; const uint32_t* xrun[6]; const uint8_t* xnxb[6];
	const uint32_t* oct_pos; const uint32_t* oct_rank; const uint32_t* oct_run; const uint64_t* oct_nx8;    /* bytes 8..15 */
	const uint32_t* hex_pos; const uint32_t* hex_rank; const uint32_t* hex_run; const uint64_t* hex_nx8;    /* bytes 16..23 */
	const uint16_t* cost_tbl;   /* 2048 x u16 */
	mgl_layout L;
	uint32_t dict_limit;
	uint32_t max_scan;
	uint32_t top_k;
	uint32_t diag_stop;         /* diagnostic: neighbour kernel returns after phase N (0 = run normally) */
	/* stratified targets (nullptr: MGL_F_POSITION_TARGETS, position draws): packets on the walk before every block of 4 096 positions
	 * (k_rank_blocks / k_rank_scan, once per step), so that neighbour j can take the packet of a given ordinal */
	const uint32_t* strat_pre;
	uint32_t strat_nblk;
	const uint32_t* strat_tgt;  /* K: the step's targets, made from strat_pre by k_targets before the neighbour kernels run */
};

struct CkptHdr {
	uint32_t pos, ctx_state;
	uint32_t dists[4];
	uint32_t ordinal, pad;
	uint64_t cum;
};

struct BaseView {
	mgl_pk* slab;          /* n packed entries, position-indexed */
	uint64_t* onwalk;      /* bitmap: bit (p&63) of word p>>6 set iff a packet starts at p */
	uint16_t* ckpt_probs;  /* nckpt x ckpt_elems */
	CkptHdr* ckpt_hdr;
	uint32_t nckpt;
	uint32_t ckpt_elems;   /* probabilities per checkpoint, rounded up to a multiple of 8 */
};

struct Control {
	uint64_t cur_cost, best_cost;
	uint64_t gstep, iter;
	uint64_t evals, failed, accepted, improved, packets_eval;
	uint64_t packets, rebuild_cost;
	uint32_t phase;
	uint32_t accepted_flag, copy_best_flag, dirty_pos, winner;
	uint32_t apply_failed; /* the incremental accept did not fit: rebuild from the slab */
	uint32_t best_is_current; /* the base structures are the best slab's: no device copy of them exists yet */
	uint32_t nbr_single;    /* the next step evaluates neighbours with the one-kernel form (repairs are frequent) */
	uint32_t mode_steps;    /* steps since the form last changed */
	uint32_t probing;       /* steps left of a short trial of the other form (keeps its timing fresh) */
	uint32_t ema_clean;     /* smoothed step duration, 10 ns ticks: split form, second pass empty ... */
	uint32_t ema_dirty;     /* ... split form, second pass taken ... */
	uint32_t ema_single;    /* ... one-kernel form */
	uint32_t p_dirty;       /* smoothed probability (x 65536) that a step needs a repair pick / second pass */
	unsigned long long t_last; /* wall clock at the end of the previous step */
	uint32_t full_rebuilds;  /* accepts that went through k_build */
	uint64_t fallback_nbrs;  /* neighbours costed by the full-walk kernel (did not fit the LDS lists) */
	uint64_t big_nbrs;       /* neighbours redone by the second (global-scratch) pass */
	uint32_t final_ctx_state;
	uint32_t final_dists[4];
	uint32_t error_flags;
	/* batched decision (mgl_kernels4.hip) */
	uint64_t imp_cands;      /* neighbours that cost less than the current slab, summed over steps */
	uint64_t dropped;        /* neighbours dropped because their journal outgrew MGL_MAX_DIFFS */
	uint64_t bulk_steps;     /* steps that took every window-best acceptable neighbour */
	uint32_t taken;          /* neighbours the last step took */
	uint32_t bulk_was_best;  /* bulk step: the base held the best slab's structures when the step began */
	uint32_t bulk_need_undo; /* bulk step: the best slab has to be restored from the new one + the undo log */
	uint64_t bulk_overlaps;  /* slab entries two taken journals of one bulk step both wanted to change (k_bulk_round; such a step is taken back) */
};
#define MGL_ERR_REBUILD_MISMATCH 1u
#define MGL_ERR_WALK_OVERRUN 2u
#define MGL_ERR_BAD_PACKET 4u /* a packet that does not reproduce the input (k_validate) */
#define MGL_ERR_SIM_LIST 8u /* k_sim was handed more distinct contexts than its list holds: cannot happen (mgl_kernels2.hip:sim_one) */

#define MGL_WIN_NONE 0xFFFFFFFFu    /* no cost: no candidate at the target / handed to a later pass */
#define MGL_WIN_DROPPED 0xFFFFFFFEu /* no cost: the journal outgrew MGL_MAX_DIFFS */
struct NbrOut {
	uint64_t* cost;    /* K */
	uint32_t* ndiffs;  /* K */
	uint32_t* walked;  /* K: packets costed by the neighbour (from its checkpoint on) */
	uint32_t* win;     /* 2 K: target position; first position from which neighbour and base are coded
	                    * identically again (n if never), or MGL_WIN_NONE / MGL_WIN_DROPPED with an invalid cost */
	uint32_t* win2;    /* K: soft end of the window (first meeting point inside the base's rep-free tail, else the end)
	                    * | bit 31: a rep packet inside the window reads a rep distance from before it */
	uint32_t* dpos;    /* K x MGL_MAX_DIFFS */
	mgl_pk* dold;
	mgl_pk* dnew;
};

__device__ __forceinline__ uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
__device__ __forceinline__ uint32_t rdlane(uint32_t x, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)x, (int)l); }
__device__ __forceinline__ uint64_t rdlane64(uint64_t x, uint32_t l)
{
	return (uint64_t)rdlane((uint32_t)x, l) | ((uint64_t)rdlane((uint32_t)(x >> 32), l) << 32);
}
__device__ __forceinline__ uint64_t uni64(uint64_t x)
{
	return (uint64_t)uni((uint32_t)x) | ((uint64_t)uni((uint32_t)(x >> 32)) << 32);
}
__device__ __forceinline__ uint64_t shfl64(uint64_t x, int src)
{
	uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, src, 64);
	uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), src, 64);
	return (uint64_t)lo | ((uint64_t)hi << 32);
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t x, int delta)
{
	uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, delta, 64);
	uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), delta, 64);
	return (uint64_t)lo | ((uint64_t)hi << 32);
}
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
	for (int o = 32; o > 0; o >>= 1) {
		uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
		uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
		v += (uint64_t)lo | ((uint64_t)hi << 32);
	}
	return v;
}
/* Stratified target: neighbour j of a step of K takes a packet of the j-th of K equal slices of the
 * walk's P packets (by ordinal), uniformly inside the slice (draw 0 of its stream).  Every packet is as likely a target as
 * under independent uniform draws (packet_slab_neighbour.c:162-163 draws an ordinal too), but the K targets of a step are
 * distinct and spread over the file, so that far fewer improving neighbours of one step overlap.  `pre[b]` = packets that
 * start before block b of 4 096 positions (k_rank_blocks / k_rank_scan, once per step).  Returns the target position. */
/* `first` (0 without a focus window): the slices are cut from the P packets of ordinals [first, first + P), see focus_ordinals. */
__device__ __forceinline__ uint32_t stratified_target(const uint64_t* onwalk, uint32_t nw0, const uint32_t* pre, uint32_t nblk,
                                                      uint32_t first, uint32_t P, uint32_t K, uint32_t j, uint32_t u, uint32_t lane)
{
	const uint32_t lo_o = (uint32_t)((uint64_t)j * P / K), hi_o = (uint32_t)((uint64_t)(j + 1u) * P / K);
	uint32_t ord = lo_o + (hi_o > lo_o ? u % (hi_o - lo_o) : 0u);
	if (ord >= P) ord = P ? P - 1u : 0u;
	ord += first;
	uint32_t lo = 0, hi = nblk; /* pre[lo] <= ord < pre[hi] */
	while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (pre[mid] <= ord) lo = mid; else hi = mid; }
	const uint32_t rem = ord - pre[lo];
	const uint32_t w = lo * 64u + lane;
	const uint64_t word = w < nw0 ? onwalk[w] : 0ull;
	const uint32_t cnt = (uint32_t)__popcll(word);
	uint32_t incl = cnt;
	for (int o = 1; o < 64; o <<= 1) { const uint32_t t2 = (uint32_t)__shfl_up((int)incl, o, 64); if ((int)lane >= o) incl += t2; }
	const unsigned long long has = __ballot(incl > rem);
	uint32_t tpos = 0;
	if (has) {
		const uint32_t l = (uint32_t)__ffsll((long long)has) - 1u;
		const uint32_t before = rdlane(incl - cnt, l);
		uint64_t wv = rdlane64(word, l);
		for (uint32_t q = rem - before; q > 0; q--) wv &= wv - 1ull;
		tpos = ((lo * 64u + l) << 6) + (uint32_t)__ffsll((long long)wv) - 1u;
	}
	return uni(tpos);
}
/* packets of the walk that start below position x (x <= n): the prefix sum of x's block of 4 096 positions plus the popcounts of
 * the block's bitmap words up to x's, that one masked below x.  One wavefront, one word per lane. */
__device__ __forceinline__ uint32_t starts_below(const uint64_t* onwalk, uint32_t nw0, const uint32_t* pre, uint32_t x, uint32_t lane)
{
	const uint32_t blk = x >> 12, wx = x >> 6; /* x = n, a multiple of 4 096: blk = nblk, whose prefix sum is the walk's total, and no word counts */
	const uint32_t w = blk * 64u + lane;
	uint64_t word = (w < nw0 && w <= wx) ? onwalk[w] : 0ull;
	if (w == wx) word &= (1ull << (x & 63u)) - 1ull;
	return pre[blk] + (uint32_t)uni64(wave_sum64((uint64_t)__popcll(word)));
}
/* Focus window (mgl_sa_set_focus): the packets that start in [lo, hi), as ordinals [*first, *first + count) of the walk; a step's
 * K slices are cut from these instead of from the whole walk.  A window inside one packet holds no start: it stands for the
 * packet that covers lo (position 0 starts a packet, so one exists).  0 < hi <= n, lo < hi. */
__device__ __forceinline__ uint32_t focus_ordinals(const uint64_t* onwalk, uint32_t nw0, const uint32_t* pre, uint32_t lo, uint32_t hi,
                                                   uint32_t lane, uint32_t* first)
{
	uint32_t a = starts_below(onwalk, nw0, pre, lo, lane);
	const uint32_t b = starts_below(onwalk, nw0, pre, hi, lane);
	if (b == a) a -= 1u;
	*first = a;
	return b - a;
}

/* LDS written by some lanes of this wave is read by others: keep the compiler from moving
 * accesses across (the hardware executes a wave's LDS operations in order). */
__device__ __forceinline__ void wave_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
}

/* ------------------------------------------------------------------ the slab walk */

/* the 64-position register window every walk reads the slab and the input through */
struct Win { /* no padding in this order: a Walk handed to top-K by reference lives in scratch, and its size shows there */
	uint32_t base; /* positions [base, base + 64) */
	uint32_t byte;
	mgl_pk pk;
};
__device__ __forceinline__ void win_reset(Win& w) { w.base = 0xFFFFFFFFu; w.pk = 0; w.byte = 0; }
/* make the window cover pos */
__device__ __forceinline__ void win_cover(Win& w, const DevCtx& c, const mgl_pk* slab, uint32_t pos, uint32_t lane)
{
	const uint32_t base = pos & ~63u;
	if (base != w.base) {
		const uint32_t p = base + lane;
		w.pk = p < c.n ? slab[p] : 0;
		w.byte = c.data[p < c.n ? p : c.n]; /* data has >= 64 bytes of zero padding */
		w.base = base;
	}
}
__device__ __forceinline__ mgl_pk win_pk(const Win& w, uint32_t pos) { return rdlane64(w.pk, pos - w.base); }
__device__ __forceinline__ uint32_t win_byte(const Win& w, uint32_t pos) { return rdlane(w.byte, pos - w.base); }

/* the LZMA initial state, at position 0 */
__device__ __forceinline__ mgl_wstate state_initial()
{
	mgl_wstate st;
	st.pos = 0; st.ctx_state = 0;
	st.dists[0] = st.dists[1] = st.dists[2] = st.dists[3] = 0;
	return st;
}
/* the state at pos from five stored words: ctx_state and the four rep distances */
__device__ __forceinline__ mgl_wstate state_from_words(const uint32_t* s, uint32_t pos)
{
	mgl_wstate st;
	st.pos = pos; st.ctx_state = s[0];
	st.dists[0] = s[1]; st.dists[1] = s[2]; st.dists[2] = s[3]; st.dists[3] = s[4];
	return st;
}

struct Walk {
	mgl_wstate st;   /* uniform */
	uint64_t acc;    /* per-lane partial perplexity */
	Win win;
	uint32_t packets;
};

__device__ __forceinline__ void walk_reset(Walk& w)
{
	w.st = state_initial();
	w.acc = 0; win_reset(w.win); w.packets = 0;
}

/* n literal transitions of the ctx_state automaton (lzma_state.c:33-41); 3 reach 0 from anywhere */
__device__ __forceinline__ uint32_t lit_steps(uint32_t s, uint32_t n)
{
	if (n > 3) n = 3;
	for (uint32_t i = 0; i < n; i++) s = mgl_next_ctx_state(s, MGL_LITERAL);
	return s;
}

/* the whole probability model under the largest layout (lc + lp = 4): 14 135 rounded up to an even count */
#define MGL_MAX_PROBS (MGL_OFF_LIT + (0x300u << 4) + 1u)

/* Plan the packet (type, dist, len) that starts at st.pos, whose first input byte is `byte`, under layout L: the one place
 * that fetches a literal's match byte and previous byte. */
__device__ __forceinline__ void plan_at(const mgl_layout& L, const uint8_t* data, const mgl_wstate& st, uint32_t type, uint32_t dist,
                                        uint32_t len, uint32_t byte, mgl_plan& pl)
{
	uint32_t match_byte = 0, prev_byte = 0;
	if (type == MGL_LITERAL) {
		if (st.ctx_state >= 7 && st.dists[0] < st.pos) match_byte = data[st.pos - st.dists[0] - 1];
		if (L.lc > 0 && st.pos > 0) prev_byte = data[st.pos - 1];
	}
	mgl_plan_packet(&L, &st, type, dist, len, byte, match_byte, prev_byte, &pl);
}

/* Cost one packet at the walk's position against the adaptive model in LDS (laid out by L) and advance.
 * Lane e takes event slot e; no slot occurs twice in one packet, so the lanes' read-modify-writes do not meet.
 * UPDATE=false leaves probabilities untouched (candidate costing) and does not advance. */
template <bool UPDATE>
__device__ __forceinline__ void walk_packet(Walk& w, const mgl_layout& L, const uint8_t* data, uint16_t* probs, const uint16_t* T,
                                            uint32_t type, uint32_t dist, uint32_t len, uint32_t lane)
{
	mgl_plan pl;
	plan_at(L, data, w.st, type, dist, len, win_byte(w.win, w.st.pos), pl);
	if (lane < pl.nev) {
		uint32_t ctx, bit;
		mgl_plan_event(&pl, lane, &ctx, &bit);
		uint32_t p = probs[ctx];
		w.acc += T[bit ? 2048u - p : p];
		if (UPDATE) probs[ctx] = (uint16_t)mgl_prob_update(p, bit);
	}
	if (lane == 0) w.acc += (uint64_t)pl.ndirect << 11;
	if (UPDATE) {
		mgl_advance(&w.st, type, dist, len);
		w.packets++;
	}
}

/* ------------------------------------------------------------------ runs of plain literals
 * Where a walk meets a run of plain literals (ctx_state < 7, so no match byte), up to seven of them are planned at once,
 * nine lanes each (is_match + the eight bits of the literal tree: 7 x 9 = 63 lanes), instead of one per turn of the walk
 * loop.  Uses only the slab / input window in registers.  What a caller does with its lane's event differs: the neighbour
 * kernel and the two accept walks append it to a change list, the model replay and the parallel builder go through the
 * run's packets one by one (the packets share contexts -- is_match and the top of the literal tree -- and probability
 * updates and chain ranks have to stay in position order). */
struct LitLane {
	bool active;      /* this lane holds an event of the run ... */
	uint32_t i, p;    /* ... of its literal i, at position p; the event's place in the run is `lane` itself (9 i + slot) */
	uint32_t ctx, bit;
};
/* How many literals of the run that begins at offset o of the window to plan at once: the consecutive literals from there
 * on (each one's successor is on the walk), cut at the window's edge, at `limit` and at seven.  0: fewer than two -- take
 * the packet-at-a-time path.  The caller has checked that ctx_state < 7. */
__device__ __forceinline__ uint32_t lit_run_take(bool lane_is_literal, uint32_t o, uint32_t limit)
{
	const unsigned long long lit = __ballot(lane_is_literal) >> o; /* window entries from the walk's position on */
	uint32_t run = ~lit == 0ull ? 64u : (uint32_t)__ffsll((long long)~lit) - 1u;
	run = run < 64u - o ? run : 64u - o;
	run = run < limit ? run : limit;
	return run < 2u ? 0u : run < 7u ? run : 7u;
}
/* Plan literals st.pos .. st.pos + take - 1 and hand each lane its event.  false: a literal's plan is not the 1 + 8 events
 * assumed above (the caller takes the run one packet at a time).  Does not advance st. */
__device__ __forceinline__ bool lit_run_plan(const DevCtx& c, const Win& win, const mgl_wstate& st, uint32_t take, uint32_t lane, LitLane& out)
{
	const uint32_t i = lane / 9u, p = st.pos + i;
	out.active = i < take; out.i = i; out.p = p;
	const uint32_t byte = (uint32_t)__shfl((int)win.byte, (int)((p - win.base) & 63u), 64);
	uint32_t prev_byte = 0;
	if (c.L.lc > 0) { /* the window's first position has its previous byte in the input only */
		const uint32_t wprev = (uint32_t)__shfl((int)win.byte, (int)((p - 1u - win.base) & 63u), 64);
		prev_byte = p == 0 ? 0u : (p - 1u >= win.base ? wprev : (uint32_t)c.data[p - 1u]);
	}
	mgl_wstate sv = st;
	sv.pos = p; sv.ctx_state = lit_steps(st.ctx_state, i);
	mgl_plan pl;
	mgl_plan_packet(&c.L, &sv, MGL_LITERAL, 0, 1, byte, 0, prev_byte, &pl);
	if (__ballot(out.active && pl.nev != 9u)) return false;
	out.ctx = 0; out.bit = 0;
	if (out.active) mgl_plan_event(&pl, lane - i * 9u, &out.ctx, &out.bit);
	return true;
}
/* model and walk state of prefix checkpoint ci into `probs` and `w`; returns the cost up to there (mgl_kernels.hip; the
 * top-K probe of mgl_topk.hip, which stands in front of it, starts from one too) */
__device__ __forceinline__ uint64_t ckpt_load(const BaseView& b, const DevCtx& c, uint32_t ci, uint16_t* probs, Walk& w, uint32_t lane);
