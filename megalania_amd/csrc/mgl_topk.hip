/*
 * mgl_topk.hip -- the top-K search at one position, one wavefront per query: every legal next packet at a walk's state, priced
 * from the adapted model, the K best kept (top_k_packet_finder.c:95-125 over packet_enumerator.c:57-74 and
 * substring_enumerator.c:85-105).  The wave-wide list (TopK), the cost helpers, the 64-ary lower bound, the
 * numbered stages and stops (PickStage, TopkStop), the two forms of a query's set-up (TopkPlan; source_range and its kin), the
 * query (topk_find: stages over TopkPrices and TopkLimits), the draw (pick_from_top_k) and the parity hook (k_topk_probe).
 * Included by mgl_api.hip in front of mgl_kernels.hip, whose full-walk engine picks.
 */
#include "mgl_device.h"

/* ================================================================== top-K (wave-wide) */
struct TopK {
	uint64_t key;   /* lane i (< count) holds the i-th best key; others ~0 */
	uint32_t count; /* uniform */
	uint32_t k;
};

__device__ __forceinline__ uint64_t topk_make_key(uint32_t cost, uint64_t seq)
{
	return ((uint64_t)cost << 44) | (MGL_SEQ_MASK - seq);
}
__device__ __forceinline__ uint64_t topk_threshold(const TopK& t)
{
	return t.count < t.k ? MGL_INVALID_COST : rdlane64(t.key, t.k - 1u); /* count and k are uniform */
}
/* K-th best cost + 1, or MGL_NO_LIMIT while the list is not full: a candidate of `len` bytes can only qualify if
 * perp / len <= K-th best cost, i.e. perp < limit * len.  Costs are < 2^20 and lengths <= 273: the products fit 32 bits */
#define MGL_NO_LIMIT 0xFFFFFFFFu
__device__ __forceinline__ uint32_t topk_limit(const TopK& t)
{
	const uint64_t thr = topk_threshold(t);
	return thr == MGL_INVALID_COST ? MGL_NO_LIMIT : (uint32_t)(thr >> 44) + 1u;
}
/* every lane may offer one candidate key (or ~0); all offers better than the current
 * K-th best are merged into the sorted list */
__device__ __forceinline__ void topk_offer(TopK& t, uint64_t cand, uint32_t lane, bool allow_batch = true)
{
	const uint64_t thr0 = topk_threshold(t);
	unsigned long long m = __ballot(cand < thr0);
	if (!m) return;
	if (allow_batch && __popcll(m) >= 4) {
		/* many at once: rank every element of (list + qualifying offers) among all of them -- keys
		 * are distinct -- and send each to the lane of its rank */
		uint32_t less_e = 0, less_c = 0, e_less = 0;
		for (unsigned long long mm = m; mm; mm &= mm - 1ull) {
			const uint32_t j = (uint32_t)__ffsll((long long)mm) - 1u;
			const uint64_t x = rdlane64(cand, j);
			less_e += x < t.key ? 1u : 0u;
			less_c += x < cand ? 1u : 0u;
			const uint32_t below = (uint32_t)__popcll(__ballot(t.key < x)); /* list keys below offer j */
			if (lane == j) e_less = below;
		}
		const bool mine = (m >> lane) & 1ull;
		uint32_t dest_e = lane < t.count ? lane + less_e : 63u;
		uint32_t dest_c = mine ? e_less + less_c : 63u;
		dest_e = dest_e < 63u ? dest_e : 63u; dest_c = dest_c < 63u ? dest_c : 63u;
		const uint64_t ve = lane < t.count ? t.key : 0ull, vc = mine ? cand : 0ull;
		const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_permute((int)(dest_e << 2), (int)(uint32_t)ve) |
		                    (uint32_t)__builtin_amdgcn_ds_permute((int)(dest_c << 2), (int)(uint32_t)vc);
		const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_permute((int)(dest_e << 2), (int)(uint32_t)(ve >> 32)) |
		                    (uint32_t)__builtin_amdgcn_ds_permute((int)(dest_c << 2), (int)(uint32_t)(vc >> 32));
		uint32_t nc = t.count + (uint32_t)__popcll(m);
		nc = nc < t.k ? nc : t.k;
		t.count = nc;
		t.key = lane < nc ? ((uint64_t)lo | ((uint64_t)hi << 32)) : MGL_INVALID_COST;
		return;
	}
	for (;;) {
		uint64_t thr = topk_threshold(t);
		m = __ballot(cand < thr);
		if (!m) break;
		int src = __ffsll((long long)m) - 1;
		uint64_t x = rdlane64(cand, (uint32_t)src);
		uint32_t r = (uint32_t)__popcll(__ballot(t.key < x));
		uint64_t up = shfl_up64(t.key, 1);
		if (lane == r) t.key = x;
		else if (lane > r) t.key = up;
		if (lane >= t.k) t.key = MGL_INVALID_COST;
		if (t.count < t.k) t.count++;
		if ((int)lane == src) cand = MGL_INVALID_COST;
	}
}

/* decode a top-K key back into a packet */
__device__ __forceinline__ mgl_pk topk_packet(uint64_t key, uint32_t pos)
{
	uint64_t seq = MGL_SEQ_MASK - (key & MGL_SEQ_MASK);
	if (seq == 0) return MGL_PK_LITERAL;
	if (seq == 1) return MGL_PK_SHORT_REP;
	uint32_t q1 = (uint32_t)(seq >> 12), len = (uint32_t)(seq >> 3) & 0x1FFu, kind = (uint32_t)seq & 7u;
	if (kind == 0) return mgl_pack(MGL_MATCH, pos - q1, len);
	return mgl_pack(MGL_LONG_REP, kind - 1, len);
}

/* ================================================================== small helpers */
__device__ __forceinline__ uint32_t bit_cost(const uint16_t* probs, const uint16_t* T, uint32_t ctx, uint32_t bit)
{
	uint32_t p = probs[ctx];
	return T[bit ? 2048u - p : p];
}
__device__ __forceinline__ uint32_t tree_cost(const uint16_t* probs, const uint16_t* T, uint32_t base, uint32_t val, uint32_t nbits)
{
	uint32_t m = 1, c = 0;
	for (uint32_t i = nbits; i-- > 0;) {
		uint32_t b = (val >> i) & 1u;
		c += bit_cost(probs, T, base + m, b);
		m = (m << 1) | b;
	}
	return c;
}
__device__ __forceinline__ uint32_t rev_tree_cost(const uint16_t* probs, const uint16_t* T, uint32_t base, uint32_t val, uint32_t nbits)
{
	uint32_t m = 1, c = 0;
	for (uint32_t i = 0; i < nbits; i++) {
		uint32_t b = val & 1u;
		val >>= 1;
		c += bit_cost(probs, T, base + m, b);
		m = (m << 1) | b;
	}
	return c;
}
/* lzma_packet_encoder.c:42-63 as a read-only cost */
__device__ __forceinline__ uint32_t length_cost(const uint16_t* probs, const uint16_t* T, uint32_t base, uint32_t len, uint32_t pos_state)
{
	uint32_t l = len - 2;
	if (l < 8) return bit_cost(probs, T, base, 0) + tree_cost(probs, T, base + MGL_LEN_LOW + pos_state * 8, l, 3);
	uint32_t c = bit_cost(probs, T, base, 1);
	if (l < 16) return c + bit_cost(probs, T, base + 1, 0) + tree_cost(probs, T, base + MGL_LEN_MID + pos_state * 8, l - 8, 3);
	return c + bit_cost(probs, T, base + 1, 1) + tree_cost(probs, T, base + MGL_LEN_HIGH, l - 16, 8);
}
/* distance slot of distance d (lzma_packet_encoder.c:70-74) */
__device__ __forceinline__ uint32_t dist_slot(uint32_t d)
{
	if (d < 4) return d;
	const uint32_t nlow = mgl_msb32(d) - 2;
	return nlow * 2 + (d >> nlow);
}
/* the least v of every aligned group of WIDTH lanes (a power of two), in all lanes of the group */
template <int WIDTH>
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
	for (int o = WIDTH / 2; o > 0; o >>= 1) { const uint32_t u = (uint32_t)__shfl_xor((int)v, o, 64); v = u < v ? u : v; }
	return v;
}

/* One step of a 64-ary lower bound over [a, b): lane i probed entry a + i * step, step = ceil((b - a) / 64), and m is the
 * ballot of "my probe is >= x" (a probe past b holds).  The predicate is monotone in the lane; f = first lane that holds
 * (64 if none).  Lane 0 probes a itself, so f == 0 means the answer is a; else it lies in (probe[f-1], probe[f]]. */
__device__ __forceinline__ void lower_bound_narrow(uint32_t& a, uint32_t& b, unsigned long long m)
{
	const uint32_t step = (b - a + 63u) / 64u;
	const int f = m ? __ffsll((long long)m) - 1 : 64;
	if (f == 0) { b = a; return; }
	const uint32_t na = a + (uint32_t)(f - 1) * step + 1u;
	uint32_t nb = a + (uint32_t)f * step;
	if (nb > b) nb = b;
	a = na; b = nb;
}
/* first index in [a, b) whose bucket position is >= x: 64-ary search, one probe per lane */
__device__ __forceinline__ uint32_t bucket_lower_bound(const uint32_t* bp, uint32_t a, uint32_t b, uint32_t x, uint32_t lane)
{
	while (b > a) {
		const uint32_t idx = a + lane * ((b - a + 63u) / 64u);
		const bool ge = idx >= b ? true : (bp[idx] >= x);
		lower_bound_narrow(a, b, __ballot(ge));
	}
	return a;
}

/* ================================================================== the numbered stages and stops */
/* Stage clock of the pick half's profile (MGL_F_PROFILE; acc == nullptr in normal runs): cycles and visits per stage, summed
 * over the picking wavefronts of a launch (tools/pick_waves.py prints them under these numbers). */
enum PickStage : uint32_t {
	PS_TARGET = 0,   /* target, state, mutate decision */
	PS_PLAN = 1,     /* the plan (batched set-up) */
	PS_MODEL = 2,    /* model load and replay */
	PS_PRICES = 3,   /* price tables, literal, short rep */
	PS_SETUP = 4,    /* set-up done in place (bounds, ranks, runs, searches, up to each source's first trip) */
	PS_REP = 5,      /* rep pass */
	PS_LONG = 6,     /* 6, 7: scans of the sixteen- and the eight-byte source */
	PS_EXACT = 8,    /* 8..13: scans of D = 7..2 */
	PS_DRAW = 14     /* draw and record */
};
#define MGL_PICK_STAGES 16u
struct PickProf { unsigned long long* acc; unsigned long long t; };
__device__ __forceinline__ void pick_prof_mark(PickProf* p, uint32_t stage, uint32_t lane)
{
	if (!p || !p->acc) return;
	const unsigned long long now = __builtin_readcyclecounter();
	if (lane == 0) { atomicAdd(&p->acc[stage], now - p->t); atomicAdd(&p->acc[MGL_PICK_STAGES + stage], 1ull); }
	p->t = __builtin_readcyclecounter();
}
/* Diagnostic stops inside a query (DevCtx::diag_stop, MGL_KEY_DIAG_STOP): the query returns behind the named stage, so the
 * difference of two stops is a stage's cost (tools/phase_cost2.py).  With a plan the window and the runs' bounds are known
 * before the query starts: stops 33 and 34 then both mean "set-up done". */
enum TopkStop : uint32_t {
	TS_TABLES = 31,      /* price tables and bounds */
	TS_LITERAL = 32,     /* + literal, short rep */
	TS_WINDOW = 33,      /* + the window: bucket bounds */
	TS_BEFORE_REP = 34,  /* + the window's first position */
	TS_REP = 35,         /* + rep pass, the long sources' bounds */
	TS_LONG16 = 36,      /* + sixteen-byte source */
	TS_LONG8 = 37,       /* + eight-byte source */
	TS_EXACT_TO_4 = 38,  /* + D = 7..4 */
	TS_FILTER_ONLY = 39, /* every source, the exact-length ones filter without pricing */
	TS_FIRST = TS_TABLES, TS_LAST = TS_FILTER_ONLY
};

/* ================================================================== the batched set-up */
/* ---- the batched set-up of topk_find's sources.
 * Where a source's entries start and end is a chain of reads of the immutable index: rank[pos] -> run[rank] -> a 64-ary
 * lower bound over the run, nine such chains per query, and none reads what another found.  Done in place, one behind the
 * other, they are about forty dependent round trips to memory.  The plan does them level by level -- every chain's loads
 * of one level are issued together and waited for once -- from the position and the rep distances alone: no model, no price.
 * So the pick half makes it before it loads the model, and its handful of round trips stand in front of the checkpoint
 * copy, not behind it.  All fields are wave-uniform (they live in SGPRs). */
struct TopkPlan {
	uint32_t lo, hi;          /* the bigram bucket's entries inside the scan window */
	uint32_t wmin;            /* a hit lies at a position >= wmin (below) */
	uint32_t r16, l16, r8, l8; /* own rank and first entry inside the window: sixteen- and eight-byte orders */
	uint32_t top[5], low[5];  /* the same for the exact-length orders D = 3..7 (index D - 3) */
	uint32_t rep;             /* byte k: bytes (of the first 64, capped by the longest match) the source of rep distance k shares with the target */
	uint64_t x0, x8, x16;     /* the target's bytes 0..23 */
};
/* Window floor.  The scan window is the bucket's entries [lo, hi): those at positions in [pos - dict_limit, pos), of which a
 * scan cap (max_scan) keeps the nearest.  An entry q < pos of a D-byte run (or a rep source that carries the bigram) is a
 * bucket entry, and the bucket ascends, so q >= bucket_pos[lo] <=> q >= pos - dict_limit as long as no cap cuts: the runs'
 * searches then need no bucket_pos[lo] and go in lock step with the bucket's.  With a cap they wait for it (second pass). */
__device__ __forceinline__ void topk_plan_make(TopkPlan& p, const DevCtx& c, const mgl_wstate& st, uint32_t lane)
{
	const uint32_t pos = st.pos;
	p.lo = p.hi = p.wmin = p.r16 = p.l16 = p.r8 = p.l8 = p.rep = 0;
#pragma unroll
	for (uint32_t i = 0; i < 5; i++) p.top[i] = p.low[i] = 0;
	p.x0 = p.x8 = p.x16 = 0;
	if (pos == 0 || pos >= c.n - 1) return; /* no match starts here: topk_find returns before it looks */
	const uint32_t maxlen = (c.n - pos) < MGL_MAX_MATCH ? (c.n - pos) : MGL_MAX_MATCH;
	/* level 0: the target's bytes, the first 64 bytes of the four rep sources, and the seven ranks (a lane per table) */
	const uint32_t* rt = lane == 0 ? c.oct_rank : lane == 1 ? c.hex_rank : lane == 2 ? c.xrank[1] : lane == 3 ? c.xrank[2] :
	                     lane == 4 ? c.xrank[3] : lane == 5 ? c.xrank[4] : c.xrank[5];
	uint32_t rk = 0;
	if (lane < 7) rk = rt[pos];
	uint64_t xw = 0;
	if (lane < 3) __builtin_memcpy(&xw, c.data + pos + 8u * lane, 8); /* the input has 64 bytes of zero padding */
	const uint32_t pv = c.data[pos + lane];
	uint32_t qv[4];
#pragma unroll
	for (uint32_t k = 0; k < 4; k++) {
		const uint32_t dk = mgl_dist_at(&st, k);
		qv[k] = dk < pos ? (uint32_t)c.data[pos - dk - 1u + lane] : 0x100u;
	}
#pragma unroll
	for (uint32_t k = 0; k < 4; k++) {
		if (mgl_dist_at(&st, k) >= pos) continue;
		const unsigned long long m = __ballot(lane >= maxlen || qv[k] != pv);
		p.rep |= (m ? (uint32_t)__ffsll((long long)m) - 1u : 64u) << (8u * k);
	}
	p.x0 = rdlane64(xw, 0); p.x8 = rdlane64(xw, 1); p.x16 = rdlane64(xw, 2);
	p.r8 = rdlane(rk, 0); p.r16 = rdlane(rk, 1);
#pragma unroll
	for (uint32_t i = 0; i < 5; i++) p.top[i] = rdlane(rk, 2u + i);
	/* level 1: the bucket's bounds and the seven run starts */
	const uint32_t bigram = (((uint32_t)p.x0 & 0xFFu) << 8) | (((uint32_t)p.x0 >> 8) & 0xFFu);
	const uint32_t* st1 = lane < 2 ? c.bucket_off : lane == 2 ? c.oct_run : lane == 3 ? c.hex_run : lane == 4 ? c.xrun[1] :
	                      lane == 5 ? c.xrun[2] : lane == 6 ? c.xrun[3] : lane == 7 ? c.xrun[4] : c.xrun[5];
	const uint32_t i1 = lane < 2 ? bigram + lane : lane == 2 ? p.r8 : lane == 3 ? p.r16 : lane == 4 ? p.top[0] :
	                    lane == 5 ? p.top[1] : lane == 6 ? p.top[2] : lane == 7 ? p.top[3] : p.top[4];
	uint32_t s1 = 0;
	if (lane < 9) s1 = st1[i1];
	const uint32_t off0 = rdlane(s1, 0), off1 = rdlane(s1, 1);
	/* levels 2..: nine lower bounds in lock step.  0: the bucket's end (entries < pos); 1: its start (entries >= the floor; the
	 * same index over [off0, off1) as over [off0, end), the floor being below pos); 2, 3: eight- and sixteen-byte runs; 4..8: D = 3..7 */
	const uint32_t floor = pos > c.dict_limit ? pos - c.dict_limit : 0u;
	const uint32_t* const tab[9] = { c.bucket_pos, c.bucket_pos, c.oct_pos, c.hex_pos, c.xpos[1], c.xpos[2], c.xpos[3], c.xpos[4], c.xpos[5] };
	uint32_t a[9], b[9];
	a[0] = a[1] = off0; b[0] = b[1] = off1;
	a[2] = rdlane(s1, 2); b[2] = p.r8;
	a[3] = rdlane(s1, 3); b[3] = p.r16;
#pragma unroll
	for (uint32_t i = 0; i < 5; i++) { a[4u + i] = rdlane(s1, 4u + i); b[4u + i] = p.top[i]; }
	const bool capped = c.max_scan != 0;
	uint32_t xlow = floor;
	/* a floor of 0 admits every entry: those searches have their answer */
	uint32_t on = capped ? 0x003u : (floor != 0 ? 0x1FFu : 0x001u);
	if (floor == 0) on &= ~2u;
#pragma nounroll
	for (uint32_t pass = 0; pass < 2; pass++) {
		if (pass == 1) {
			if (!capped) break;
			/* the cap cuts inside the window: the runs are searched for the first position the cap leaves */
			p.hi = a[0]; p.lo = floor != 0 ? a[1] : off0;
			if (p.hi - p.lo > c.max_scan) p.lo = p.hi - c.max_scan;
			if (p.hi == p.lo) return; /* no hit: topk_find returns before it looks at the rest */
			xlow = uni(c.bucket_pos[p.lo]);
			on = 0x1FCu;
		}
		for (;;) {
			uint32_t v[9];
			bool any = false;
#pragma unroll
			for (uint32_t s = 0; s < 9; s++) {
				v[s] = 0xFFFFFFFFu;
				if (!((on >> s) & 1u) || b[s] <= a[s]) continue;
				any = true;
				const uint32_t idx = a[s] + lane * ((b[s] - a[s] + 63u) / 64u);
				if (idx < b[s]) v[s] = tab[s][idx];
			}
			if (!any) break;
#pragma unroll
			for (uint32_t s = 0; s < 9; s++) {
				if (!((on >> s) & 1u) || b[s] <= a[s]) continue;
				lower_bound_narrow(a[s], b[s], __ballot(v[s] >= (s == 0 ? pos : xlow))); /* a probe past the end holds ~0 */
			}
		}
	}
	if (!capped) { p.hi = a[0]; p.lo = floor != 0 ? a[1] : off0; }
	p.wmin = xlow;
	p.l8 = a[2]; p.l16 = a[3];
#pragma unroll
	for (uint32_t i = 0; i < 5; i++) p.low[i] = a[4u + i];
}

/* ---- the two forms of a query's set-up behind one face.  BATCH: the answers come from `plan` (topk_plan_make at this
 * position and these rep distances).  Otherwise they are looked up in place when a stage asks: the kernels that run at
 * 256 VGPRs keep that form, a plan held across their model load would only add to their spills, and a source that the
 * earlier sources' pruning never reaches costs them nothing. */
/* the target's first two bytes, as the bucket index (the in-place form's; the plan has used its own) */
template <bool BATCH>
__device__ __forceinline__ uint32_t target_bigram(const DevCtx& c, const Walk& w)
{
	return BATCH ? 0u : ((uint32_t)win_byte(w.win, w.st.pos) << 8) | c.data[w.st.pos + 1];
}
/* Own rank of pos in the order of source S (3..7, 8, 16): what the in-place form of source_range starts from (the plan holds
 * the ranges whole).  Apart from it, so that the two long sources have both ranks in flight before the first search waits. */
template <bool BATCH>
__device__ __forceinline__ uint32_t source_rank(const DevCtx& c, uint32_t S, uint32_t pos)
{
	if (BATCH) return 0;
	return uni((S == 16 ? c.hex_rank : S == 8 ? c.oct_rank : c.xrank[S - 2u])[pos]); /* pos is uniform */
}
/* Entries [low, top) of source S, nearest last.  S is the length of the prefix the source's order sorts by: 2 the bigram
 * bucket (its scan window: positions in [pos - dict_limit, pos), of which a scan cap keeps the nearest), 3..7 the
 * exact-length orders, 8 and 16 the two long ones -- for those the entries of pos's run at positions >= wpos (rank: source_rank). */
template <bool BATCH>
__device__ __forceinline__ void source_range(const DevCtx& c, const Walk& w, const TopkPlan* plan, uint32_t S, uint32_t rank, uint32_t wpos, uint32_t lane, uint32_t& low, uint32_t& top)
{
	const uint32_t pos = w.st.pos;
	if (BATCH) {
		/* no indexing of the plan by a variable: it lives in registers */
		switch (S) {
		case 2: low = plan->lo; top = plan->hi; break;
		case 3: low = plan->low[0]; top = plan->top[0]; break;
		case 4: low = plan->low[1]; top = plan->top[1]; break;
		case 5: low = plan->low[2]; top = plan->top[2]; break;
		case 6: low = plan->low[3]; top = plan->top[3]; break;
		case 7: low = plan->low[4]; top = plan->top[4]; break;
		case 8: low = plan->l8; top = plan->r8; break;
		default: low = plan->l16; top = plan->r16; break;
		}
	} else if (S == 2) {
		const uint32_t bigram = target_bigram<BATCH>(c, w);
		low = c.bucket_off[bigram];
		const uint32_t end = c.bucket_off[bigram + 1];
		top = bucket_lower_bound(c.bucket_pos, low, end, pos, lane); /* hits are < pos */
		if (pos > c.dict_limit) low = bucket_lower_bound(c.bucket_pos, low, top, pos - c.dict_limit, lane);
		if (c.max_scan && top - low > c.max_scan) low = top - c.max_scan;
	} else {
		const uint32_t* run = S == 16 ? c.hex_run : S == 8 ? c.oct_run : c.xrun[S - 2u];
		const uint32_t* at = S == 16 ? c.hex_pos : S == 8 ? c.oct_pos : c.xpos[S - 2u];
		top = rank;
		low = bucket_lower_bound(at, run[top], top, wpos, lane);
	}
}
/* the first position of the scan window [lo, hi) (not empty): hits lie at [wpos, pos).  With a plan: its floor, which admits the same entries */
template <bool BATCH>
__device__ __forceinline__ uint32_t window_first(const DevCtx& c, const TopkPlan* plan, uint32_t lo)
{
	return BATCH ? plan->wmin : c.bucket_pos[lo];
}
/* the target's bytes 0..23: byte D of x0 is what separates source D from source D + 1 */
template <bool BATCH>
__device__ __forceinline__ void target_bytes(const DevCtx& c, const TopkPlan* plan, uint32_t pos, uint64_t& x0, uint64_t& x8, uint64_t& x16)
{
	if (BATCH) { x0 = plan->x0; x8 = plan->x8; x16 = plan->x16; return; }
	__builtin_memcpy(&x0, c.data + pos, 8); /* the input has 64 bytes of zero padding */
	__builtin_memcpy(&x8, c.data + pos + 8, 8);
	__builtin_memcpy(&x16, c.data + pos + 16, 8);
}
/* The rep pass's shortcut.  Does the source at q (a rep distance's) carry the target's bigram, and which bytes are left to
 * compare: the match length is L if `from` >= maxlen, else the compare goes on at byte `from`.  With a plan the first 64
 * bytes of all four sources are compared already (they carry the bigram when two or more agree). */
template <bool BATCH>
__device__ __forceinline__ bool rep_first_bytes(const DevCtx& c, const TopkPlan* plan, uint32_t bigram, uint32_t k, uint32_t q, uint32_t maxlen, uint32_t& L, uint32_t& from)
{
	L = maxlen; from = 0;
	if (!BATCH) return c.data[q] == (bigram >> 8) && c.data[q + 1] == (bigram & 0xFFu);
	const uint32_t L0 = (plan->rep >> (8u * k)) & 0xFFu;
	if (L0 < 64u) { L = L0; from = maxlen; } else from = 64u;
	return L0 >= 2u;
}

/* ================================================================== the query's state */
/* a query's prices: all wave-uniform but the tables */
struct TopkPrices {
	uint32_t pos_state;
	uint32_t hdr_match, hdr_short, hdr_lr0, hdr_lr1, hdr_lr2, hdr_lr3; /* packet headers, lzma_packet_encoder.c:13-40 */
	PriceTab tab;                 /* the wavefront's price tables (mgl_device.h) */
	uint32_t minlen_m, minlen_r;  /* cheapest length price of either coder over the lengths priced so far: lower bounds for pruning */
	uint32_t min15;               /* cheapest match-length price up to the eight-byte source's cap */
	bool high_ready;              /* lengths >= 18 are priced */
};
/* ... and its limits */
struct TopkLimits {
	uint32_t pos, maxlen;
	uint32_t inc_type, inc_len, inc_dist; /* the incumbent: never offered (top_k_packet_finder.c:99-101) */
	uint32_t lim32;               /* topk_limit(), kept across the batches of a scan and refreshed after offers */
};

/* ================================================================== the stages of a query */
/* ---- price tables and their bounds: the tables, per slot the least a distance in it can cost, the cheapest lengths */
__device__ __forceinline__ void prices_build(TopkPrices& pr, const DevCtx& c, const mgl_wstate& st, const uint16_t* probs, const uint16_t* T, uint32_t* table, uint32_t lane)
{
	const uint32_t state = st.ctx_state;
	const uint32_t pos_state = st.pos & ((1u << c.L.pb) - 1u);
	const uint32_t sp = (state << 4) + pos_state;
	const uint32_t c_m1 = bit_cost(probs, T, MGL_CS_IS_MATCH + sp, 1);
	const uint32_t c_r0 = bit_cost(probs, T, MGL_CS_IS_REP + state, 0);
	const uint32_t c_r1 = bit_cost(probs, T, MGL_CS_IS_REP + state, 1);
	const uint32_t g0_0 = bit_cost(probs, T, MGL_CS_G0 + state, 0), g0_1 = bit_cost(probs, T, MGL_CS_G0 + state, 1);
	const uint32_t g1_0 = bit_cost(probs, T, MGL_CS_G1 + state, 0), g1_1 = bit_cost(probs, T, MGL_CS_G1 + state, 1);
	const uint32_t g2_0 = bit_cost(probs, T, MGL_CS_G2 + state, 0), g2_1 = bit_cost(probs, T, MGL_CS_G2 + state, 1);
	const uint32_t l_0 = bit_cost(probs, T, MGL_CS_REP0_LONG + sp, 0), l_1 = bit_cost(probs, T, MGL_CS_REP0_LONG + sp, 1);
	const uint32_t hdr_rep = c_m1 + c_r1;
	pr.pos_state = pos_state;
	pr.hdr_match = c_m1 + c_r0;
	pr.hdr_short = hdr_rep + g0_0 + l_0;
	pr.hdr_lr0 = hdr_rep + g0_0 + l_1; pr.hdr_lr1 = hdr_rep + g0_1 + g1_0;
	pr.hdr_lr2 = hdr_rep + g0_1 + g1_1 + g2_0; pr.hdr_lr3 = hdr_rep + g0_1 + g1_1 + g2_1;
	const PriceTab tab = pr.tab = price_tab(table);
	if (lane < 32) {
		const uint32_t l = 2 + (lane & 15u);
		(lane < 16 ? tab.len_m : tab.len_r)[l - 2] = length_cost(probs, T, lane < 16 ? MGL_OFF_LEN : MGL_OFF_REP_LEN, l, pos_state);
	}
	for (uint32_t e = lane; e < 256; e += 64) tab.slot[e] = tree_cost(probs, T, MGL_OFF_DIST + (e & ~63u), e & 63u, 6);
	for (uint32_t d = 4 + lane; d < 128; d += 64) {
		const uint32_t nlow = mgl_msb32(d) - 2, low = d & ((1u << nlow) - 1u), high = d >> nlow;
		tab.tail[d] = rev_tree_cost(probs, T, MGL_OFF_DIST + MGL_DIST_POS + (high << nlow) - (nlow * 2 + high), low, nlow);
	}
	if (lane < 16) tab.align[lane] = rev_tree_cost(probs, T, MGL_OFF_DIST + MGL_DIST_ALIGN, lane, 4);
	pr.high_ready = false;
	wave_sync();
	{
		const uint32_t slot = lane;
		uint32_t m = tab.slot[slot];
		for (uint32_t k = 1; k < 4; k++) { const uint32_t v = tab.slot[64u * k + slot]; m = v < m ? v : m; }
		const uint32_t amin = uni(wave_min<16>(lane < 16 ? tab.align[lane] : 0xFFFFFFFFu));
		/* direct bits + at least the cheapest align nibble; the reverse-tree tails of nearer slots count as 0 */
		if (slot >= 14) m += (((slot >> 1) - 5u) << 11) + amin;
		tab.lbslot[slot] = m;
		uint32_t sm = m;
		for (int o = 1; o < 64; o <<= 1) {
			const uint32_t tdn = (uint32_t)__shfl_down((int)sm, o, 64);
			if ((int)lane + o < 64) sm = tdn < sm ? tdn : sm;
		}
		tab.sufmin[slot] = sm;
	}
	wave_sync();
	/* the cheapest of the lengths priced so far, 2..17 */
	pr.minlen_m = uni(wave_min<16>(lane < 16 ? pr.tab.len_m[lane] : 0xFFFFFFFFu));
	pr.minlen_r = uni(wave_min<16>(lane < 16 ? pr.tab.len_r[lane] : 0xFFFFFFFFu));
}
/* lengths >= 18 (the 8-bit high tree) are priced only when a match that long shows up */
__device__ __forceinline__ void price_high_lengths(TopkPrices& pr, const uint16_t* probs, const uint16_t* T, uint32_t lane)
{
	const PriceTab& tab = pr.tab;
#pragma nounroll /* seven copies of this function are inlined, and a query runs at most one, once */
	for (uint32_t l = 18 + lane; l <= MGL_MAX_MATCH; l += 64) {
		tab.len_m[l - 2] = length_cost(probs, T, MGL_OFF_LEN, l, pr.pos_state);
		tab.len_r[l - 2] = length_cost(probs, T, MGL_OFF_REP_LEN, l, pr.pos_state);
	}
	pr.high_ready = true;
	wave_sync();
	uint32_t a = 0xFFFFFFFFu, b = 0xFFFFFFFFu;
	for (uint32_t l = 16 + lane; l < 272; l += 64) { a = tab.len_m[l] < a ? tab.len_m[l] : a; b = tab.len_r[l] < b ? tab.len_r[l] : b; }
	a = wave_min<64>(a); b = wave_min<64>(b);
	pr.minlen_m = a < pr.minlen_m ? uni(a) : pr.minlen_m; pr.minlen_r = b < pr.minlen_r ? uni(b) : pr.minlen_r;
}

/* ---- LITERAL and SHORT_REP, packet_enumerator.c:60-66 */
__device__ __forceinline__ void offer_literal_short_rep(TopK& t, const DevCtx& c, const Walk& w, const uint16_t* probs, const uint16_t* T, const TopkPrices& pr, mgl_pk incumbent, uint32_t lane)
{
	const uint32_t pos = w.st.pos;
	uint64_t cand = MGL_INVALID_COST;
	uint32_t byte = win_byte(w.win, pos);
	uint32_t rep_byte = (pos > 0 && w.st.dists[0] < pos) ? c.data[pos - w.st.dists[0] - 1] : 0x100u;
	uint32_t prev_byte = (c.L.lc > 0 && pos > 0) ? c.data[pos - 1] : 0;
	mgl_plan pl;
	mgl_plan_packet(&c.L, &w.st, MGL_LITERAL, 0, 1, byte, rep_byte, prev_byte, &pl);
	uint32_t ec = 0;
	if (lane < pl.nev) {
		uint32_t ctx, bit;
		mgl_plan_event(&pl, lane, &ctx, &bit);
		ec = bit_cost(probs, T, ctx, bit);
	}
	uint32_t lit = (uint32_t)wave_sum64(ec);
	if (lane == 0 && incumbent != MGL_PK_LITERAL) cand = topk_make_key(lit, 0);
	if (lane == 1 && pos > 0 && byte == rep_byte && incumbent != MGL_PK_SHORT_REP) cand = topk_make_key(pr.hdr_short, 1);
	topk_offer(t, cand, lane);
}

/* ---- LONG_REP candidates (packet_enumerator.c:48-54: a hit whose distance is rep distance i also offers LONG_REP i at
 * every length).  At most four hits can: the positions the four rep distances point at, when they carry this bigram and lie
 * inside the scan window.  They are priced here, on their own (a LONG_REP's price does not depend on the distance), so the
 * distance-ordered scans of the sources deal with MATCH candidates only and can stop on a distance bound even when a rep
 * distance points into the bucket. */
template <bool BATCH>
__device__ __forceinline__ void rep_pass(TopK& t, const DevCtx& c, const Walk& w, const uint16_t* probs, const uint16_t* T, TopkPrices& pr, const TopkLimits& lm, const TopkPlan* plan, uint32_t wpos, uint32_t lane)
{
	const uint32_t pos = lm.pos, maxlen = lm.maxlen;
	const uint32_t bigram = target_bigram<BATCH>(c, w);
#pragma unroll
	for (uint32_t k = 0; k < 4; k++) {
		const uint32_t dk = mgl_dist_at(&w.st, k);
		if (dk >= pos) continue;
		const uint32_t q = pos - dk - 1u;
		uint32_t L, from;
		if (q < wpos || !rep_first_bytes<BATCH>(c, plan, bigram, k, q, maxlen, L, from)) continue;
		/* match length, substring_enumerator.c:99-103: 64 bytes per trip */
		for (uint32_t base = from; base < maxlen; base += 64) {
			const uint32_t i = base + lane;
			const bool stop = i >= maxlen || c.data[q + i] != c.data[pos + i];
			const unsigned long long m = __ballot(stop);
			if (m) { const uint32_t f = base + (uint32_t)__ffsll((long long)m) - 1u; L = f < maxlen ? f : maxlen; break; }
		}
		if (L >= 18 && !pr.high_ready) price_high_lengths(pr, probs, T, lane);
		const uint32_t hdr = k == 0 ? pr.hdr_lr0 : k == 1 ? pr.hdr_lr1 : k == 2 ? pr.hdr_lr2 : pr.hdr_lr3;
		for (uint32_t top = L; top >= 2;) {
			const uint64_t thr = topk_threshold(t);
			const uint32_t lim = topk_limit(t);
			if (lim != MGL_NO_LIMIT && hdr + pr.minlen_r >= lim * top) break; /* nothing at this or any shorter length */
			uint64_t cand = MGL_INVALID_COST;
			if (lane + 2u <= top) {
				const uint32_t len = top - lane;
				const uint32_t perp = hdr + pr.tab.len_r[len - 2];
				if ((lim == MGL_NO_LIMIT || perp < lim * len) && !(lm.inc_type == MGL_LONG_REP && len == lm.inc_len && lm.inc_dist == k)) {
					const uint64_t key = topk_make_key(perp / len, ((uint64_t)(q + 1) << 12) | ((uint64_t)len << 3) | (1u + k));
					if (key < thr) cand = key;
				}
			}
			topk_offer(t, cand, lane);
			top = top > 64u + 1u ? top - 64u : 0u;
		}
	}
}

/* ---- MATCH candidates: eight sources, longest matches first, nearest entries first inside each.
 *   16+ bytes  the run of the sixteen-byte order that holds this position: entries [run start, own rank) are the earlier
 *              positions sharing 16 bytes; eight more bytes sit beside each entry, the rest is compared in the input;
 *   8..15      the run of the eight-byte order, entries of the deeper run skipped (their next eight bytes equal ours); the
 *              length comes from those eight bytes alone;
 *   D = 7..2   the run of the D-byte order (D = 2: the bigram bucket), entries whose byte D equals ours skipped (they
 *              belong to the next source up): all others match exactly D bytes.
 * Inside a source the price only grows with the distance slot, and the lengths are capped by the next source's prefix: a
 * scan stops at the first batch whose nearest entry cannot reach the K-th best any more even at the cheapest length up to
 * that cap and the cheapest slot from there on (a true lower bound: the selection stays exact). */

/* what the scans start from: behind the rep pass (lengths 2..17 are priced by now) */
__device__ __forceinline__ void scans_begin(const TopK& t, TopkPrices& pr, TopkLimits& lm, uint32_t lane)
{
	pr.min15 = uni(wave_min<16>(lane < 14 ? pr.tab.len_m[lane] : 0xFFFFFFFFu));
	lm.lim32 = topk_limit(t);
}

/* price the survivors of a batch: per lane one hit at position hq with match length hL (have = lane holds one) */
__device__ __forceinline__ void price_hits(TopK& t, const uint16_t* probs, const uint16_t* T, TopkPrices& pr, TopkLimits& lm, uint32_t hq, uint32_t hL, bool have, uint32_t lane)
{
	if (!pr.high_ready && __ballot(have && hL >= 18)) price_high_lengths(pr, probs, T, lane);
	/* one table read decides for most hits: even the cheapest conceivable price at the longest
	 * length this hit offers does not reach the current K-th best */
	const PriceTab& tab = pr.tab;
	const uint32_t d = lm.pos - hq - 1u;
	uint32_t slot = d, lb = 0;
	if (have) {
		slot = dist_slot(d);
		lb = pr.hdr_match + pr.minlen_m + tab.lbslot[slot];
		if (lm.lim32 != MGL_NO_LIMIT && lb >= lm.lim32 * hL) have = false;
	}
	if (!__ballot(have)) return;
	uint32_t s0 = 0, s1 = 0, s2 = 0, s3 = 0, tail = 0;
	if (have) {
		/* distance price per length context from the tables */
		if (d >= 4) {
			const uint32_t nlow = mgl_msb32(d) - 2;
			tail = d < 128 ? tab.tail[d] : ((nlow - 4) << 11) + tab.align[d & 15u];
		}
		s0 = tab.slot[slot]; s1 = tab.slot[64 + slot]; s2 = tab.slot[128 + slot]; s3 = tab.slot[192 + slot];
	}
	/* Candidates of a hit: the MATCH at every length 2..L (packet_enumerator.c:48-49).  The selection is
	 * order-independent, so each lane walks its hit from the longest length down (the cheapest per byte
	 * first, which tightens the threshold at once) and stops as soon as even a lower bound of the price
	 * cannot beat the current K-th best any more.  The exact perp/len division is only done for candidates
	 * that pass the multiply test. */
	uint32_t len = hL;
	while (__ballot(have)) {
		const uint64_t thr = topk_threshold(t);
		const uint32_t lim = topk_limit(t);
		uint64_t cand = MGL_INVALID_COST;
		while (have) {
			if (lim != MGL_NO_LIMIT && lb >= lim * len) { have = false; break; } /* nothing at this or any shorter length */
			const uint32_t sc = len == 2 ? s0 : len == 3 ? s1 : len == 4 ? s2 : s3;
			const uint32_t perp = pr.hdr_match + tab.len_m[len - 2] + sc + tail;
			const uint32_t clen = len;
			len--;
			if (len < 2) have = false;
			if (lim != MGL_NO_LIMIT && perp >= lim * clen) continue;
			if (lm.inc_type == MGL_MATCH && clen == lm.inc_len && d == lm.inc_dist) continue; /* top_k_packet_finder.c:99-101 */
			const uint64_t key = topk_make_key(perp / clen, ((uint64_t)(hq + 1) << 12) | ((uint64_t)clen << 3));
			if (key < thr) { cand = key; break; }
		}
		topk_offer(t, cand, lane);
	}
	lm.lim32 = topk_limit(t);
}

/* ---- a long source, entries [low, top): 64 entries per trip, the next trip's entries in flight.  SIXTEEN: the
 * sixteen-byte order (lengths 16..maxlen), else the eight-byte order (8..15); x = the target's eight bytes behind the prefix */
__device__ __forceinline__ void scan_long(TopK& t, const DevCtx& c, const uint16_t* probs, const uint16_t* T, TopkPrices& pr, TopkLimits& lm, bool sixteen, uint32_t low, uint32_t top, uint64_t x, uint32_t lane)
{
	const uint32_t pos = lm.pos, maxlen = lm.maxlen;
	const uint32_t* spos = sixteen ? c.hex_pos : c.oct_pos;
	const uint64_t* snx = sixteen ? c.hex_nx8 : c.oct_nx8;
	const uint32_t cnt = top - low;
	const uint32_t lcap = sixteen ? maxlen : 15u;
	uint32_t q = 0, q1 = 0;
	uint64_t y = 0, y1 = 0;
	if (lane < cnt) { q = spos[top - 1u - lane]; y = snx[top - 1u - lane]; }
	for (uint32_t hb = 0; hb < cnt; hb += 64) {
		bool have = hb + lane < cnt;
		if (hb + 64u + lane < cnt) { q1 = spos[top - 65u - hb - lane]; y1 = snx[top - 65u - hb - lane]; }
		const uint32_t cq = q;
		const uint64_t cy = y;
		q = q1; y = y1;
		{
			/* lane 0 holds the nearest entry of this batch */
			const uint32_t sn = dist_slot(pos - rdlane(cq, 0) - 1u);
			const uint32_t ml = sixteen ? pr.minlen_m : pr.min15;
			if (lm.lim32 != MGL_NO_LIMIT && pr.hdr_match + ml + pr.tab.sufmin[sn] >= lm.lim32 * lcap) break;
		}
		uint32_t L = 0;
		if (have) {
			const uint64_t df = x ^ cy;
			if (sixteen) {
				if (df) L = 16u + (((uint32_t)__ffsll((long long)df) - 1u) >> 3);
				else {
					/* 24 bytes match: eight bytes per step from the input (zero padded past its end) */
					L = 24;
					while (L < maxlen) {
						uint64_t xx, yy;
						__builtin_memcpy(&xx, c.data + pos + L, 8);
						__builtin_memcpy(&yy, c.data + cq + L, 8);
						const uint64_t df2 = xx ^ yy;
						if (df2) { L += ((uint32_t)__ffsll((long long)df2) - 1u) >> 3; break; }
						L += 8;
					}
				}
			} else {
				if (!df) have = false; /* 16+ bytes: priced from the deeper run */
				else L = 8u + (((uint32_t)__ffsll((long long)df) - 1u) >> 3);
			}
			if (L > maxlen) L = maxlen;
		}
		price_hits(t, probs, T, pr, lm, cq, L, have, lane);
	}
}

/* ---- an exact-length source, D = 7 down to 2, entries [low, top): an entry of the D-byte order's run whose byte D differs
 * from ours matches exactly D bytes (the others belong to the next source up).  These runs hold the bulk of the entries
 * (10^4 .. 10^5 per query in a 4 MiB window of text) and almost all of them are turned away; with one length per source the
 * pruning bound is one distance threshold, recomputed only when the K-th best moves: an entry at distance >= dthr cannot
 * qualify at length D or shorter (hdr + cheapest length price up to D + sufmin[slot] >= lim * D, a true lower bound), and
 * the scan of the source ends at the first such entry.  The scan is memory latency bound, so a lane takes W consecutive
 * entries per trip (W = 4: 256 per wavefront, one 16-byte and one 4-byte load) and filters them with a subtraction and two
 * compares each. */
__device__ __forceinline__ uint32_t exact_dist_threshold(const TopkPrices& pr, uint32_t lim32, uint32_t minup, uint32_t D, uint32_t lane)
{
	if (lim32 == MGL_NO_LIMIT) return 0xFFFFFFFFu;
	const uint32_t fixed = pr.hdr_match + minup, need = lim32 * D;
	const unsigned long long m = __ballot(need <= fixed || pr.tab.sufmin[lane] >= need - fixed);
	if (!m) return 0xFFFFFFFFu;
	const uint32_t sl = (uint32_t)__ffsll((long long)m) - 1u;
	return sl < 4u ? sl : ((2u | (sl & 1u)) << ((sl >> 1) - 1u)); /* first distance of that slot */
}
/* entries hb + W lane + r, r = 0..W-1 (r = 0 nearest): array indices top - 1 - e, i.e. the W words at
 * top - W - hb - W lane, the nearest last */
template <int W>
__device__ __forceinline__ void exact_load(const uint32_t* spos, const uint8_t* snxb, uint32_t pos, uint32_t top, uint32_t cnt, uint32_t hb, uint32_t lane, uint32_t qv[W], uint32_t& yv)
{
	const uint32_t e0 = hb + (uint32_t)W * lane;
	if (W == 4 && e0 + 3u < cnt) {
		const uint32_t base = top - 4u - e0;
		uint4 qq;
		__builtin_memcpy(&qq, spos + base, 16);
		qv[0] = qq.w; qv[1 % W] = qq.z; qv[2 % W] = qq.y; qv[3 % W] = qq.x;
		uint32_t yy;
		__builtin_memcpy(&yy, snxb + base, 4);
		yv = __builtin_bswap32(yy); /* byte r of yv = entry r */
	} else {
		yv = 0;
#pragma unroll
		for (uint32_t r = 0; r < (uint32_t)W; r++) {
			const bool in = e0 + r < cnt;
			const uint32_t idx = in ? top - 1u - (e0 + r) : top - 1u;
			qv[r] = in ? spos[idx] : pos; /* distance "-1": never passes the filter */
			yv |= (uint32_t)snxb[idx] << (8u * r);
		}
	}
}
template <int W, bool PROF>
__device__ __forceinline__ void scan_exact(TopK& t, const DevCtx& c, const uint16_t* probs, const uint16_t* T, TopkPrices& pr, TopkLimits& lm, PickProf* pp, uint32_t D, uint32_t low, uint32_t top, uint64_t x0, uint32_t lane)
{
	const uint32_t pos = lm.pos;
	const uint32_t* spos = c.xpos[D - 2u];
	const uint8_t* snxb = c.xnxb[D - 2u];
	const uint32_t cnt = top - low;
	if (PROF && cnt == 0) pick_prof_mark(pp, PS_SETUP, lane);
	if (cnt == 0) return;
	const uint32_t xb = (uint32_t)(x0 >> (8u * D)) & 0xFFu; /* our byte D (D = 7: byte 7 is the top byte of x0) */
	const uint32_t hitlen = D < lm.maxlen ? D : lm.maxlen;
	/* cheapest match-length price over lengths 2..D */
	const uint32_t minup = uni(wave_min<8>(lane < D - 1u ? pr.tab.len_m[lane] : 0xFFFFFFFFu));
	uint32_t lim_seen = lm.lim32;
	uint32_t dthr = exact_dist_threshold(pr, lm.lim32, minup, D, lane);
	uint32_t qa[W], qb[W], ya, yb = 0;
#pragma unroll
	for (uint32_t r = 0; r < (uint32_t)W; r++) qb[r] = 0;
	if (PROF) pick_prof_mark(pp, PS_SETUP, lane); /* set-up: up to this source's first trip */
	exact_load<W>(spos, snxb, pos, top, cnt, 0, lane, qa, ya);
	for (uint32_t hb = 0; hb < cnt; hb += 64u * W) {
		if (hb + 64u * W < cnt) exact_load<W>(spos, snxb, pos, top, cnt, hb + 64u * W, lane, qb, yb); /* the next trip, in flight */
		if (lim_seen != lm.lim32) { lim_seen = lm.lim32; dthr = exact_dist_threshold(pr, lm.lim32, minup, D, lane); }
		/* lane 0's first entry is the nearest of this trip */
		if (pos - rdlane(qa[0], 0) - 1u >= dthr) break;
		uint32_t prmask = 0; /* bit r: entry r of this lane passes the filter */
#pragma unroll
		for (uint32_t r = 0; r < (uint32_t)W; r++) {
			const uint32_t d = pos - qa[r] - 1u; /* out-of-range slots hold q = pos: d = 0xFFFFFFFF */
			/* byte D equal: the match goes on: priced from the next source up */
			const bool p = ((ya >> (8u * r)) & 0xFFu) != xb && d < dthr && d != 0xFFFFFFFFu;
			prmask |= (p ? 1u : 0u) << r;
		}
		if (c.diag_stop == TS_FILTER_ONLY) prmask = 0;
		/* one copy of the pricing code: the (rare) survivors of the W entries take turns */
		for (uint32_t r = 0; r < (uint32_t)W && __ballot(prmask != 0); r++) {
			const bool p = (prmask >> r) & 1u;
			if (!__ballot(p)) continue;
			uint32_t q_r = qa[0];
#pragma unroll
			for (uint32_t k = 1; k < (uint32_t)W; k++) q_r = r == k ? qa[k] : q_r;
			price_hits(t, probs, T, pr, lm, q_r, hitlen, p, lane);
			prmask &= ~(1u << r);
		}
#pragma unroll
		for (uint32_t r = 0; r < (uint32_t)W; r++) qa[r] = qb[r];
		ya = yb;
	}
	if (PROF) pick_prof_mark(pp, PS_EXACT + (7u - D), lane);
}

/* ================================================================== the query */
/* top_k_packet_finder_find (top_k_packet_finder.c:120-125): enumerate every legal next
 * packet at the walk's state, cost each from the adapted model (cost = perplexity/length,
 * :115-116), keep the k best.  Order-independent ("canonical") selection: better = lower
 * cost, then later in the reference's enumeration order (the reference's `<=`, :89).
 * table: the wavefront's price tables in LDS, MGL_PRICE_WORDS u32.
 * W: entries a lane takes per trip through the exact-length sources (4 where registers allow: the pick kernel; 1 in the
 * one-kernel form, which has none to spare).
 * BATCH: the sources' bounds come from `plan` (source_range and its kin, above).
 * PROF: the stage marks of the pick half's profile are compiled in (`pp`: its clock); the kernels of normal runs hold none. */
template <int W, bool BATCH = false, bool PROF = false>
__device__ void topk_find(TopK& t, const DevCtx& c, const Walk& w, const uint16_t* probs, const uint16_t* T, uint32_t* table, mgl_pk incumbent, uint32_t lane, const TopkPlan* plan = nullptr, PickProf* pp = nullptr)
{
	const uint32_t pos = w.st.pos;
	TopkPrices pr;
	TopkLimits lm;
	t.key = MGL_INVALID_COST;
	t.count = 0;
	t.k = c.top_k;
	prices_build(pr, c, w.st, probs, T, table, lane);
	if (c.diag_stop == TS_TABLES) return;
	offer_literal_short_rep(t, c, w, probs, T, pr, incumbent, lane);
	if (c.diag_stop == TS_LITERAL) return;
	/* substring_enumerator.c:85-105: nothing at the first and the last byte */
	if (pos == 0 || pos >= c.n - 1) return;
	if (PROF) pick_prof_mark(pp, PS_PRICES, lane);
	/* the scan window: the bucket's entries [lo, hi), hits at positions [wpos, pos) */
	uint32_t lo, hi;
	source_range<BATCH>(c, w, plan, 2, 0, 0, lane, lo, hi); /* the bucket has no rank and defines wpos */
	if (c.diag_stop == TS_WINDOW) { t.count += (hi - lo) & 1u; return; }
	if (hi == lo) return;
	const uint32_t wpos = window_first<BATCH>(c, plan, lo);
	if (PROF) pick_prof_mark(pp, PS_SETUP, lane);
	lm.pos = pos;
	lm.maxlen = (c.n - pos) < MGL_MAX_MATCH ? (c.n - pos) : MGL_MAX_MATCH;
	lm.inc_type = mgl_pk_type(incumbent); lm.inc_len = mgl_pk_len(incumbent); lm.inc_dist = mgl_pk_dist(incumbent);
	if (c.diag_stop == TS_BEFORE_REP) return;
	rep_pass<BATCH>(t, c, w, probs, T, pr, lm, plan, wpos, lane);
	if (PROF) pick_prof_mark(pp, PS_REP, lane);
	uint64_t x0, x8, x16;
	uint32_t l8, r8, l16, r16;
	target_bytes<BATCH>(c, plan, pos, x0, x8, x16);
	const uint32_t k8 = source_rank<BATCH>(c, 8, pos), k16 = source_rank<BATCH>(c, 16, pos);
	source_range<BATCH>(c, w, plan, 8, k8, wpos, lane, l8, r8);
	source_range<BATCH>(c, w, plan, 16, k16, wpos, lane, l16, r16);
	if (PROF) pick_prof_mark(pp, PS_SETUP, lane);
	if (c.diag_stop == TS_REP) return;
	scans_begin(t, pr, lm, lane);
	for (uint32_t ph = 0; ph < 2; ph++) {
		if (c.diag_stop >= TS_LONG16 && c.diag_stop <= TS_EXACT_TO_4 && ph > c.diag_stop - TS_LONG16) break;
		scan_long(t, c, probs, T, pr, lm, ph == 0, ph == 0 ? l16 : l8, ph == 0 ? r16 : r8, ph == 0 ? x16 : x8, lane);
		if (PROF) pick_prof_mark(pp, PS_LONG + ph, lane);
	}
	if (c.diag_stop == TS_LONG16 || c.diag_stop == TS_LONG8) return;
	for (uint32_t D = 7; D >= 2; D--) {
		if (c.diag_stop == TS_EXACT_TO_4 && D < 4) break;
		uint32_t low = lo, top = hi;
		if (D > 2) source_range<BATCH>(c, w, plan, D, source_rank<BATCH>(c, D, pos), wpos, lane, low, top);
		scan_exact<W, PROF>(t, c, probs, T, pr, lm, pp, D, low, top, x0, lane);
	}
}

/* ================================================================== the draw */
struct NbrRng { uint64_t key; uint32_t n; };
__device__ __forceinline__ uint32_t nbr_draw(NbrRng& r) { return mgl_rng_draw(r.key, r.n++); }

/* packet_slab_neighbour.c:56-72 with the canonical top-K order */
template <int W, bool BATCH = false, bool PROF = false>
__device__ bool pick_from_top_k(const DevCtx& c, const Walk& w, const uint16_t* probs, const uint16_t* T, uint32_t* lencost, mgl_pk incumbent, bool best, NbrRng& rng, uint32_t lane, mgl_pk* picked, const TopkPlan* plan = nullptr, PickProf* pp = nullptr)
{
	TopK t;
	topk_find<W, BATCH, PROF>(t, c, w, probs, T, lencost, incumbent, lane, plan, pp);
	const uint32_t count = t.count;
	if (count == 0) return false;
	uint32_t choice = nbr_draw(rng) % count; /* :48-54 max of 8 draws */
	for (int i = 0; i < 7; i++) { uint32_t x = nbr_draw(rng) % count; choice = x > choice ? x : choice; }
	if (nbr_draw(rng) % 8u == 0 || best) choice = count - 1;
	/* pop order is worst first: the (choice+1)-th pop is rank count-1-choice from the best */
	uint64_t key = shfl64(t.key, (int)(count - 1 - choice));
	*picked = topk_packet(key, w.st.pos);
	return true;
}

/* ================================================================== the probe */

/* top-K at an arbitrary on-walk position of a (scratch) base; list written worst first.  FORM (MGL_KEY_PROBE_FORM): 0 the
 * batched form of the pick half (W = 4, a plan), 1 the in-place form of the repair picks, the one-kernel form and the
 * full-walk engine (W = 1, no plan). */
template <int FORM>
__global__ void __launch_bounds__(64) k_topk_probe(DevCtx c, BaseView b, uint32_t position, mgl_pk* out_pk, uint64_t* out_cost, uint32_t* out_count)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	uint16_t* T = (uint16_t*)smem;
	uint16_t* probs = (uint16_t*)(smem + 4096);
	uint32_t* lencost = (uint32_t*)(smem + 4096 + (size_t)b.ckpt_elems * 2);
	const uint32_t lane = threadIdx.x;
	for (uint32_t i = lane; i < 2048; i += 64) T[i] = c.cost_tbl[i];
	wave_sync();
	if (position >= c.n || !((b.onwalk[position >> 6] >> (position & 63u)) & 1ull)) {
		if (lane == 0) *out_count = ~0u;
		return;
	}
	Walk w;
	ckpt_load(b, c, position >> MGL_CKPT_SHIFT, probs, w, lane);
	while (w.st.pos < position) {
		win_cover(w.win, c, b.slab, w.st.pos, lane);
		const mgl_pk pk = win_pk(w.win, w.st.pos);
		walk_packet<true>(w, c.L, c.data, probs, T, mgl_pk_type(pk), mgl_pk_dist(pk), mgl_pk_len(pk), lane);
	}
	win_cover(w.win, c, b.slab, w.st.pos, lane);
	TopK t;
	if (FORM == 0) {
		TopkPlan plan;
		topk_plan_make(plan, c, w.st, lane);
		topk_find<4, true>(t, c, w, probs, T, lencost, win_pk(w.win, position), lane, &plan);
	} else {
		topk_find<1>(t, c, w, probs, T, lencost, win_pk(w.win, position), lane);
	}
	if (lane < t.count) {
		const uint32_t o = t.count - 1 - lane; /* worst first */
		out_pk[o] = topk_packet(t.key, position);
		out_cost[o] = t.key >> 44;
	}
	if (lane == 0) *out_count = t.count;
}
