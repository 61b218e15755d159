/*
 * mgl_kernels2.hip -- the incremental neighbour path.
 *
 *   k_build        one wavefront walks the base slab twice: (1) bitmaps, per-special state
 *                  records, per-context event counts -> chain offsets; (2) fills the chains
 *                  (position, bit, probability before) and the dense checkpoints, totals the cost
 *   k_neighbours2  one wavefront per neighbour.  Work is proportional to the *changed window*,
 *                  not to the file: walk state at the target from the special records, mutate
 *                  (top-K needs the model at the target: dense checkpoint + <= 64 bytes of replay),
 *                  then a two-pointer walk over the neighbour's and the base's packets that stops
 *                  when position, ctx_state and rep distances agree again; identical packets
 *                  cancel, runs of plain literals are skipped through the special bitmap.  The
 *                  inserted / removed events are then priced per probability context against
 *                  the base chains until each perturbed probability re-joins its base trajectory.
 *                  The result is the neighbour's exact total (u64) -- the same number
 *                  packet_slab_neighbour_generate (packet_slab_neighbour.c:154-173) would return.
 */
#include "mgl_base2.h"

/* ================================================================== k_build */

struct BitAcc {
	uint32_t word;
	uint64_t bits;
};
__device__ __forceinline__ void bitacc_move(BitAcc& a, uint64_t* arr, uint32_t new_word, uint32_t lane)
{
	if (new_word == a.word) return;
	if (lane == 0) arr[a.word] = a.bits;
	for (uint32_t z = a.word + 1 + lane; z < new_word; z += 64) arr[z] = 0;
	a.word = new_word; a.bits = 0;
}

__device__ void build_body(const DevCtx& c, const Base2& b, Control* ctl, int check_cost)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	uint16_t* T = (uint16_t*)smem;
	uint16_t* probs = (uint16_t*)(smem + 4096);
	uint32_t* cnt = (uint32_t*)(smem + 4096 + (size_t)b.ck_elems * 2);
	uint32_t* off = cnt + b.ck_elems;
	const uint32_t lane = threadIdx.x;
	const uint32_t total = c.L.total;
	/* check_cost: 0 = unconditional build; 1 = per-step rebuild after an accept;
	 * 2 = only when the incremental accept (k_apply_*) gave up */
	if (check_cost && !ctl->accepted_flag) return;
	if (check_cost == 2 && !ctl->apply_failed) return;
	for (uint32_t i = lane; i < 2048; i += 64) T[i] = c.cost_tbl[i];
	for (uint32_t i = lane; i < b.ck_elems; i += 64) { cnt[i] = 0; off[i] = 0; }
	wave_sync();

	/* ---- pass 1: bitmaps, special-state records, event counts */
	Walk w;
	walk_reset(w);
	BitAcc on = { 0, 0 }, sp = { 0, 0 };
	uint32_t guard = 0;
	while (w.st.pos < c.n) {
		const uint32_t pos = w.st.pos;
		if (++guard > c.n) { if (lane == 0) atomicOr(&ctl->error_flags, MGL_ERR_WALK_OVERRUN); break; }
		bitacc_move(on, b.onwalk, pos >> 6, lane);
		bitacc_move(sp, b.sp0, pos >> 6, lane);
		on.bits |= 1ull << (pos & 63u);
		win_cover(w.win, c, b.slab, w.st.pos, lane);
		const mgl_pk pk = win_pk(w.win, pos);
		uint32_t type = mgl_pk_type(pk), len = mgl_pk_len(pk), dist = mgl_pk_dist(pk);
		if (!mgl_pk_wellformed(type, dist, len) || len > c.n - pos) {
			type = MGL_LITERAL; len = 1; dist = 0;
			if (lane == 0) atomicOr(&ctl->error_flags, MGL_ERR_WALK_OVERRUN);
		}
		if (type != MGL_LITERAL) {
			sp.bits |= 1ull << (pos & 63u);
			if (lane < 8) state_record_write(b, pos, w.st, lane);
		}
		mgl_plan pl;
		plan_at(c.L, c.data, w.st, type, dist, len, win_byte(w.win, pos), pl);
		if (lane < pl.nev) {
			uint32_t ctx, bit;
			mgl_plan_event(&pl, lane, &ctx, &bit);
			cnt[ctx]++; /* contexts of one packet are distinct: no conflict */
		}
		mgl_advance(&w.st, type, dist, len);
		w.packets++;
	}
	{
		const uint32_t nw0 = b.nw0;
		bitacc_move(on, b.onwalk, nw0, lane);
		bitacc_move(sp, b.sp0, nw0, lane);
	}
	const uint32_t npackets = w.packets;
	__threadfence();
	wave_sync();
	/* summary levels of the special bitmap */
	for (uint32_t u = 0; u < b.nw1; u++) {
		const uint32_t wd = u * 64 + lane;
		const bool nz = wd < b.nw0 && b.sp0[wd] != 0;
		const unsigned long long m = __ballot(nz);
		if (lane == 0) b.sp1[u] = m;
	}
	__threadfence();
	wave_sync();
	for (uint32_t v = 0; v < b.nw2; v++) {
		const uint32_t u = v * 64 + lane;
		const bool nz = u < b.nw1 && b.sp1[u] != 0;
		const unsigned long long m = __ballot(nz);
		if (lane == 0) b.sp2[v] = m;
	}
	/* chain offsets: capacity = 2 len + 257 rounded up to 8 (incl. the sentinel): room to grow before a
	 * chain has to move (k_apply_chains); lanes own contiguous context ranges */
	{
		const uint32_t per = (total + 63u) / 64u;
		const uint32_t lo = lane * per, hi = (lo + per) < total ? (lo + per) : total;
		uint32_t sum = 0;
		for (uint32_t i = lo; i < hi; i++) sum += (2u * cnt[i] + 257u + 7u) & ~7u;
		uint32_t incl = sum;
		for (int o = 1; o < 64; o <<= 1) {
			const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
			if ((int)lane >= o) incl += t;
		}
		uint32_t run = incl - sum;
		for (uint32_t i = lo; i < hi; i++) {
			const uint32_t cap = (2u * cnt[i] + 257u + 7u) & ~7u; /* multiple of 8: 16-byte aligned chains */
			off[i] = run;
			b.ch_off[i] = run; b.ch_len[i] = cnt[i]; b.ch_cap[i] = cap;
			run += cap;
		}
		const uint32_t all = (uint32_t)__shfl((int)incl, 63, 64);
		if (lane == 0) {
			*b.pool_top = all;
			if (all > b.pool_cap) atomicOr(&ctl->error_flags, MGL_ERR_WALK_OVERRUN);
		}
		if (all > b.pool_cap) return;
	}
	wave_sync();
	for (uint32_t i = lane; i < b.ck_elems; i += 64) { cnt[i] = 0; probs[i] = MGL_PROB_INIT; }
	wave_sync();

	/* ---- pass 2: chains + dense checkpoints + chain index + cost */
	walk_reset(w);
	uint32_t next_ck = 0, next_sb = 0;
	guard = 0;
	while (w.st.pos < c.n) {
		const uint32_t pos = w.st.pos;
		if (++guard > c.n) break;
		while (next_sb <= (pos >> b.sb_shift)) { /* entries per context before this block */
			for (uint32_t i = lane; i < total; i += 64) b.ch_sb[(size_t)i * b.sb_stride + next_sb] = cnt[i];
			next_sb++;
		}
		while (next_ck < b.nck && (next_ck << MGL_CK2_SHIFT) <= pos) {
			uint32_t* dst = (uint32_t*)(b.ck_probs + (size_t)next_ck * b.ck_elems);
			const uint32_t* src = (const uint32_t*)probs;
			for (uint32_t i = lane; i < b.ck_elems / 2; i += 64) dst[i] = src[i];
			next_ck++;
		}
		win_cover(w.win, c, b.slab, w.st.pos, lane);
		const mgl_pk pk = win_pk(w.win, pos);
		uint32_t type = mgl_pk_type(pk), len = mgl_pk_len(pk), dist = mgl_pk_dist(pk);
		if (!mgl_pk_wellformed(type, dist, len) || len > c.n - pos) { type = MGL_LITERAL; len = 1; dist = 0; }
		mgl_plan pl;
		plan_at(c.L, c.data, w.st, type, dist, len, win_byte(w.win, pos), pl);
		if (lane < pl.nev) {
			uint32_t ctx, bit;
			mgl_plan_event(&pl, lane, &ctx, &bit);
			const uint32_t p = probs[ctx];
			const uint32_t k = off[ctx] + cnt[ctx]++;
			b.ch_pos[k] = pos;
			b.ch_ev[k] = (uint16_t)((bit << 15) | p);
			w.acc += T[bit ? 2048u - p : p];
			probs[ctx] = (uint16_t)mgl_prob_update(p, bit);
		}
		if (lane == 0) w.acc += (uint64_t)pl.ndirect << 11;
		mgl_advance(&w.st, type, dist, len);
		w.packets++;
	}
	wave_sync();
	/* checkpoints whose boundary lies behind the last packet start hold the final model, so
	 * that every checkpoint is defined (k_apply_chains relies on that) */
	while (next_ck < b.nck) {
		uint32_t* dst = (uint32_t*)(b.ck_probs + (size_t)next_ck * b.ck_elems);
		const uint32_t* src = (const uint32_t*)probs;
		for (uint32_t i = lane; i < b.ck_elems / 2; i += 64) dst[i] = src[i];
		next_ck++;
	}
	for (; next_sb <= b.nsb; next_sb++)
		for (uint32_t i = lane; i < total; i += 64) b.ch_sb[(size_t)i * b.sb_stride + next_sb] = cnt[i];
	/* sentinels: position = infinity, probability = the context's final value */
	for (uint32_t i = lane; i < total; i += 64) {
		const uint32_t k = off[i] + cnt[i];
		b.ch_pos[k] = MGL_POS_INF;
		b.ch_ev[k] = probs[i];
	}
	const uint64_t cost = wave_sum64(w.acc);
	if (lane == 0) {
		ctl->packets = npackets;
		ctl->rebuild_cost = cost;
		ctl->final_ctx_state = w.st.ctx_state;
		ctl->final_dists[0] = w.st.dists[0]; ctl->final_dists[1] = w.st.dists[1];
		ctl->final_dists[2] = w.st.dists[2]; ctl->final_dists[3] = w.st.dists[3];
		if (check_cost) {
			if (ctl->cur_cost != cost) atomicOr(&ctl->error_flags, MGL_ERR_REBUILD_MISMATCH);
			ctl->accepted_flag = 0;
			ctl->full_rebuilds++;
		}
	}
}

__global__ void __launch_bounds__(64) k_build(DevCtx c, Base2 b, Control* ctl, int check_cost)
{
	build_body(c, b, ctl, check_cost);
}
/* the tail of an incremental step in one launch: the fallback rebuild (only when k_apply_* gave
 * up) and then the step's bookkeeping (mgl_kernels3.hip) */
__device__ void step_end_body(Control* ctl, int lazy_best, StepCounts* counts, int adaptive, int form_single);
__global__ void __launch_bounds__(64) k_build_end(DevCtx c, Base2 b, Control* ctl, int lazy_best, StepCounts* counts, int adaptive, int form_single)
{
	build_body(c, b, ctl, 2);
	__threadfence();
	wave_sync();
	step_end_body(ctl, lazy_best, counts, adaptive, form_single);
}

/* ================================================================== change lists */

struct Changes {
	uint16_t* ins_key; /* ctx | bit << 15 */
	uint32_t* ins_pos;
	uint16_t* rem_key; /* ctx */
	uint32_t* rem_pos;
	uint16_t* uctx;     /* distinct touched contexts (scratch of chain_sim) */
	uint32_t* ctxbits;  /* LDS bitmap over the probability contexts (scratch of chain_sim) */
	uint32_t cap;       /* capacity of each list */
	uint32_t uctx_cap;
	uint32_t nbitwords;
	uint32_t n_ins, n_rem; /* uniform: the stored lengths */
	uint32_t n_cancel;     /* uniform: event pairs the paired site of the walk left out of both lists (changes_add_pair).  A pair is one
	                        * inserted and one removed event, so the totals capacity rule (2) of DESIGN.md section 4 counts -- every event
	                        * of every packet that does not cancel whole -- are n_ins + n_cancel and n_rem + n_cancel */
	int64_t direct;        /* (inserted - removed) direct-bit cost, uniform */
	unsigned long long* dbg; /* diagnostic counters (MGL_F_PROFILE), else nullptr */
	uint32_t diag;
	bool overflow;
	bool list_full;        /* overflow because a list reached its capacity (as opposed to any other reason) */
};

/* append the events of one planned packet to the inserted (INS) or removed list */
template <bool INS>
__device__ __forceinline__ void changes_add(Changes& ch, const mgl_plan& pl, uint32_t pos, uint32_t lane)
{
	uint32_t& n = INS ? ch.n_ins : ch.n_rem;
	if (n + pl.nev > ch.cap || n + ch.n_cancel + pl.nev > MGL_BIG_CAP) { ch.overflow = true; ch.list_full = true; return; } /* room by the stored length, the rule by the counted one */
	if (lane < pl.nev) {
		uint32_t ctx, bit;
		mgl_plan_event(&pl, lane, &ctx, &bit);
		if (INS) { ch.ins_key[n + lane] = (uint16_t)(ctx | (bit << 15)); ch.ins_pos[n + lane] = pos; }
		else { ch.rem_key[n + lane] = (uint16_t)ctx; ch.rem_pos[n + lane] = pos; }
	}
	n += pl.nev;
	const int64_t d = (int64_t)((uint64_t)pl.ndirect << 11);
	ch.direct += INS ? d : -d;
}

/* The paired site of the window walk: a neighbour packet (planned, `npl`) and, where bnev != 0, the base packet that starts at
 * the same position and does not cancel whole (its keys ctx | bit << 15 one per lane in `bkey`, its direct bits in `bndirect`).
 * An event both plans hold in the same slot -- same context, same bit, same position -- is left out of both lists: a context
 * occurs at most once in a packet's plan, so at that context and position the merged chain is the base chain, and the
 * re-simulation computes the same probabilities and the same delta with the pair or without it.  Two plans of the same packet
 * have the same slot structure, and so have the headers and length trees of different packets where they agree, so a lane
 * compares the two keys of its own slot.  The survivors keep their order (the lists stay sorted by position). */
__device__ __forceinline__ void changes_add_pair(Changes& ch, uint32_t bkey, uint32_t bnev, uint32_t bndirect, const mgl_plan& npl, uint32_t pos,
                                                 uint32_t lane, bool evcancel)
{
	uint32_t nkey = 0;
	if (lane < npl.nev) {
		uint32_t ctx, bit;
		mgl_plan_event(&npl, lane, &ctx, &bit);
		nkey = ctx | (bit << 15);
	}
	const bool common = evcancel && lane < bnev && lane < npl.nev && bkey == nkey;
	const unsigned long long cm = __ballot(common);
	const uint32_t nc = (uint32_t)__popcll(cm);
	/* the rule counts the packets' events, the room is the survivors' */
	if (ch.n_rem + ch.n_cancel + bnev > MGL_BIG_CAP || ch.n_ins + ch.n_cancel + npl.nev > MGL_BIG_CAP ||
	    ch.n_rem + bnev - nc > ch.cap || ch.n_ins + npl.nev - nc > ch.cap) { ch.overflow = true; ch.list_full = true; return; }
	if (!common) {
		const uint32_t at = lane - __builtin_amdgcn_mbcnt_hi((uint32_t)(cm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)cm, 0u)); /* cancelled slots below this one */
		if (lane < bnev) { ch.rem_key[ch.n_rem + at] = (uint16_t)(bkey & 0x7FFFu); ch.rem_pos[ch.n_rem + at] = pos; }
		if (lane < npl.nev) { ch.ins_key[ch.n_ins + at] = (uint16_t)nkey; ch.ins_pos[ch.n_ins + at] = pos; }
	}
	ch.n_rem += bnev - nc; ch.n_ins += npl.nev - nc; ch.n_cancel += nc;
	ch.direct += (int64_t)((uint64_t)npl.ndirect << 11) - (int64_t)((uint64_t)bndirect << 11);
}

/* first index >= start (and < n) whose key, masked, equals cx; n if none.  Sixteen 16-bit keys
 * per trip: two independent 16-byte reads (the lists are 16-byte aligned), so a scan waits for
 * half as many LDS round trips. */
__device__ __forceinline__ uint32_t next_with_ctx(const uint16_t* keys, uint32_t start, uint32_t n, uint32_t cx, uint32_t mask)
{
	uint32_t base = start & ~7u;
	while (base < n) {
		const uint4 q = *reinterpret_cast<const uint4*>(keys + base);
		uint4 r = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu); /* no context has this key */
		if (base + 8u < n) r = *reinterpret_cast<const uint4*>(keys + base + 8u);
		const uint32_t w[8] = { q.x, q.y, q.z, q.w, r.x, r.y, r.z, r.w };
		uint32_t hit = 0;
#pragma unroll
		for (uint32_t e = 0; e < 16; e++) {
			const uint32_t key = (w[e >> 1] >> ((e & 1u) * 16u)) & mask;
			hit |= (key == cx ? 1u : 0u) << e;
		}
		if (base < start) hit &= ~0u << (start - base);
		if (hit) {
			const uint32_t idx = base + (uint32_t)__ffs((int)hit) - 1u;
			return idx < n ? idx : n;
		}
		base += 16;
	}
	return n;
}

/* Price the change lists against the base chains.  Every distinct touched context is
 * re-simulated by one lane from its first change, merging the base chain (minus removed
 * events) with the inserted events by position, until no change is pending and the running
 * probability equals the base's (re-coupled), the chain ends, or `limit` is reached.
 * Returns sum(new cost - base cost) over the simulated spans (all lanes get the value).
 * If overlay != nullptr the probability each touched context has at `limit` is written into
 * it (contexts that re-coupled before `limit` keep the base value already there). */
/* part A (one wavefront): the distinct touched contexts, ascending, into ch.uctx; returns how many */
__device__ __forceinline__ uint32_t chain_list(Changes& ch, uint32_t lane, bool* too_many)
{
	const uint32_t m = ch.n_ins + ch.n_rem;
	wave_sync();
	/* distinct contexts through a bitmap in LDS, then listed in ascending order */
	for (uint32_t i = lane; i < ch.nbitwords; i += 64) ch.ctxbits[i] = 0;
	wave_sync();
	for (uint32_t e = lane; e < m; e += 64) {
		const uint32_t key = e < ch.n_ins ? (ch.ins_key[e] & 0x7FFFu) : ch.rem_key[e - ch.n_ins];
		atomicOr(&ch.ctxbits[key >> 5], 1u << (key & 31u));
	}
	wave_sync();
	uint32_t nu = 0;
	for (uint32_t w0 = 0; w0 < ch.nbitwords; w0 += 64) {
		const uint32_t word = w0 + lane < ch.nbitwords ? ch.ctxbits[w0 + lane] : 0u;
		const uint32_t cntl = (uint32_t)__popc(word);
		uint32_t incl = cntl;
		for (int o = 1; o < 64; o <<= 1) {
			const uint32_t tmp = (uint32_t)__shfl_up((int)incl, o, 64);
			if ((int)lane >= o) incl += tmp;
		}
		const uint32_t chunk = (uint32_t)__shfl((int)incl, 63, 64);
		if (nu + chunk > ch.uctx_cap) { *too_many = true; return 0; }
		uint32_t at = nu + incl - cntl;
		uint32_t wv = word;
		while (wv) {
			ch.uctx[at++] = (uint16_t)(((w0 + lane) << 5) + ((uint32_t)__ffs((int)wv) - 1u));
			wv &= wv - 1u;
		}
		nu += chunk;
	}
	wave_sync();
	return nu;
}
/* part B: this lane's share of the contexts -- uctx[first + lane], then every `stride` further on
 * (64 for a wavefront on its own; k_sim puts several wavefronts on one neighbour).  Returns the
 * lane's own sum. */
/* traffic (nullable): the bytes of chain data this lane asked the memory system for are added to it -- 4 per position
 * probed by a search, 48 per eight-entry chunk (positions + events), 32 per sixteen events of the re-coupling stretch:
 * the re-simulation's algorithmic bytes, counted where they are read (bench.py's roofline block) */
__device__ __forceinline__ int64_t chain_sim_contexts(const Base2& b, Changes& ch, const uint16_t* T, uint32_t limit, uint16_t* overlay,
                                                      uint32_t lane, uint32_t first, uint32_t stride, uint32_t nu, uint32_t* traffic = nullptr)
{
	int64_t delta = 0;
	for (uint32_t base = first; base < nu; base += stride) {
		if (base + lane >= nu) continue;
		const uint32_t cx = ch.uctx[base + lane];
		uint32_t ii = next_with_ctx(ch.ins_key, 0, ch.n_ins, cx, 0x7FFFu);
		uint32_t ri = next_with_ctx(ch.rem_key, 0, ch.n_rem, cx, 0xFFFFu);
		const uint32_t ipos0 = ii < ch.n_ins ? ch.ins_pos[ii] : MGL_POS_INF;
		const uint32_t rpos0 = ri < ch.n_rem ? ch.rem_pos[ri] : MGL_POS_INF;
		const uint32_t x0 = ipos0 < rpos0 ? ipos0 : rpos0;
		const uint32_t* cpos = b.ch_pos + b.ch_off[cx];
		const uint16_t* cev = b.ch_ev + b.ch_off[cx];
		const uint32_t clen = b.ch_len[cx];
		uint32_t probes = 0;
		uint32_t blo, bhi; /* the chain index narrows the search to the entries of x0's block */
		chain_block(b, cx, x0, &blo, &bhi);
		uint32_t k = chain_lower_bound(cpos, bhi, x0, traffic ? &probes : nullptr, blo);
		if (traffic) *traffic += 20u; /* chain offset and length of this context, two index entries */
		/* eight chain entries (positions + events) per round trip, kept in registers */
		uint4 c_pa = make_uint4(0, 0, 0, 0), c_pb = c_pa, c_ev = c_pa;
		uint32_t c_base = 0xFFFFFFFFu;
		auto chunk = [&](uint32_t kk) {
			if ((kk & ~7u) != c_base) {
				c_base = kk & ~7u; /* chains start 32-byte aligned; the pool is over-allocated past its end */
				c_pa = *reinterpret_cast<const uint4*>(cpos + c_base);
				c_pb = *reinterpret_cast<const uint4*>(cpos + c_base + 4);
				c_ev = *reinterpret_cast<const uint4*>(cev + c_base);
				if (traffic) *traffic += 48u;
			}
		};
		auto pos_at = [&](uint32_t kk) -> uint32_t {
			const uint32_t e = kk & 7u;
			return e == 0 ? c_pa.x : e == 1 ? c_pa.y : e == 2 ? c_pa.z : e == 3 ? c_pa.w : e == 4 ? c_pb.x : e == 5 ? c_pb.y : e == 6 ? c_pb.z : c_pb.w;
		};
		auto ev_at = [&](uint32_t kk) -> uint32_t {
			const uint32_t e = kk & 7u;
			const uint32_t wd = e < 2 ? c_ev.x : e < 4 ? c_ev.y : e < 6 ? c_ev.z : c_ev.w;
			return (wd >> ((e & 1u) * 16u)) & 0xFFFFu;
		};
		chunk(k);
		uint32_t p = ev_at(k) & 0x7FFu;
		bool at_limit = false, ended = false;
		if (ch.diag == 42) { delta += p; continue; }
		uint32_t iters = 0;
		/* ---- part 1: while this context still has changes ahead (or a limit applies):
		 * merge base entries and inserted events by position; the position of the next change of
		 * either list is kept in a register */
		uint32_t ipos = ipos0, rpos = rpos0;
		for (;;) {
			const bool pending = ipos != MGL_POS_INF || rpos != MGL_POS_INF;
			if (!pending && limit == MGL_POS_INF) break; /* -> part 2 */
			iters++;
			chunk(k);
			const uint32_t bpos = pos_at(k);
			if (ipos < bpos) {
				if (ipos >= limit) { at_limit = true; ended = true; break; }
				const uint32_t bit = ch.ins_key[ii] >> 15;
				delta += T[bit ? 2048u - p : p];
				p = mgl_prob_update(p, bit);
				ii = next_with_ctx(ch.ins_key, ii + 1, ch.n_ins, cx, 0x7FFFu);
				ipos = ii < ch.n_ins ? ch.ins_pos[ii] : MGL_POS_INF;
				continue;
			}
			if (bpos == MGL_POS_INF) { ended = true; break; }          /* chain exhausted */
			if (bpos >= limit) { at_limit = true; ended = true; break; }
			const uint32_t ev = ev_at(k);
			const uint32_t bp = ev & 0x7FFu, bb = ev >> 15;
			if (p == bp) {
				if (!pending) { ended = true; break; }   /* re-coupled, nothing ahead (limit mode) */
				/* re-coupled, but this context changes again further on: everything up to
				 * that position is coded exactly as in the base, so jump there */
				const uint32_t nxt = ipos < rpos ? ipos : rpos;
				if (nxt > bpos) {
					if (nxt >= limit) { ended = true; break; } /* the base value holds at the limit */
					chain_block(b, cx, nxt, &blo, &bhi);
					k = chain_lower_bound(cpos, bhi, nxt, traffic ? &probes : nullptr, blo > k ? blo : k);
					if (traffic) *traffic += 8u;
					chunk(k);
					p = ev_at(k) & 0x7FFu;
					continue;
				}
			}
			delta -= T[bb ? 2048u - bp : bp];
			if (rpos == bpos) {
				ri = next_with_ctx(ch.rem_key, ri + 1, ch.n_rem, cx, 0xFFFFu);
				rpos = ri < ch.n_rem ? ch.rem_pos[ri] : MGL_POS_INF;
			} else {
				delta += T[bb ? 2048u - p : p];
				p = mgl_prob_update(p, bb);
			}
			k++;
		}
		if (ch.diag == 43) { delta += p; continue; }
		/* ---- part 2: no change ahead: follow the base chain until the probability re-joins
		 * the base trajectory.  Only (bit, base probability) is needed: 16 entries per round
		 * trip (two 16-byte loads), the next 16 already in flight while these are processed. */
		if (!ended) {
			uint32_t kb = k & ~15u;
			uint4 a0 = *reinterpret_cast<const uint4*>(cev + kb);
			uint4 a1 = *reinterpret_cast<const uint4*>(cev + kb + 8);
			int32_t d32 = 0; /* 16 events x 22 528 at most per round: widened once per round */
			while (!ended) {
				/* may read up to 64 bytes past the sentinel: the pool is over-allocated for that */
				const uint4 n0 = *reinterpret_cast<const uint4*>(cev + kb + 16);
				const uint4 n1 = *reinterpret_cast<const uint4*>(cev + kb + 24);
				if (traffic) *traffic += 32u;
#pragma unroll
				for (uint32_t e = 0; e < 16; e++) {
					const uint32_t idx = kb + e;
					if (ended || idx < k) continue;
					if (idx >= clen) { ended = true; continue; }               /* chain exhausted */
					const uint4 q = e < 8 ? a0 : a1;
					const uint32_t h = e & 7u;
					const uint32_t wd = h < 2 ? q.x : h < 4 ? q.y : h < 6 ? q.z : q.w;
					const uint32_t ev = (wd >> ((h & 1u) * 16u)) & 0xFFFFu;
					const uint32_t bp = ev & 0x7FFu, bb = ev >> 15;
					if (p == bp) { ended = true; continue; }                   /* re-coupled */
					d32 += (int32_t)T[bb ? 2048u - p : p] - (int32_t)T[bb ? 2048u - bp : bp];
					p = mgl_prob_update(p, bb);
				}
				delta += d32; d32 = 0;
				a0 = n0; a1 = n1; kb += 16;
			}
			k = kb;
		}
		if (ch.dbg) atomicMax(&ch.dbg[21], (unsigned long long)iters);
		if (traffic) *traffic += 4u * probes;
		if (overlay && (at_limit || (limit != MGL_POS_INF && cpos[k] == MGL_POS_INF))) overlay[cx] = (uint16_t)p;
		(void)c_base;
	}
	return delta;
}
/* forced: left to the inliner it stays a call in the second pass (k_neighbours2<true, FULL>: 704 -> 796 B/lane of scratch) */
__device__ __forceinline__ int64_t chain_sim(const Base2& b, Changes& ch, const uint16_t* T, uint32_t limit, uint16_t* overlay,
                                             uint32_t lane, bool* too_many)
{
	const uint32_t nu = chain_list(ch, lane, too_many);
	if (*too_many) return 0;
	if (ch.diag == 41) return (int64_t)nu;
	const int64_t delta = chain_sim_contexts(b, ch, T, limit, overlay, lane, 0u, 64u, nu);
	/* signed wave sum */
	uint64_t u = (uint64_t)delta;
	u = wave_sum64(u);
	wave_sync();
	return (int64_t)u;
}

/* ================================================================== k_neighbours2 */

/* optional per-phase cycle accounting (diagnostic: prof == nullptr in normal runs) */
struct Prof {
	unsigned long long* acc;
	unsigned long long t;
};
__device__ __forceinline__ void prof_start(Prof& p, unsigned long long* acc) { p.acc = acc; if (acc) p.t = __builtin_readcyclecounter(); }
__device__ __forceinline__ void prof_mark(Prof& p, int phase, uint32_t lane)
{
	if (!p.acc) return;
	const unsigned long long now = __builtin_readcyclecounter();
	if (lane == 0) { atomicAdd(&p.acc[phase], now - p.t); atomicAdd(&p.acc[8 + phase], 1ull); atomicMax(&p.acc[16 + phase], now - p.t); }
	p.t = __builtin_readcyclecounter();
}

/* Base packets the neighbour's walk has passed over disappear, and under a freshly picked match
 * they are mostly a run of plain literals: their events go to the inserted (INS) or removed list
 * seven packets at a time (lit_run_take / lit_run_plan, mgl_device.h).  Returns the number of
 * packets taken (0: not a plain-literal run of at least two -- take the packet-at-a-time path). */
template <bool INS>
__device__ __forceinline__ uint32_t literal_run_events(const DevCtx& c, Changes& ch, const Win& win, mgl_wstate& st, uint32_t limit, uint32_t lane)
{
	if (st.ctx_state >= 7u) return 0;
	const uint32_t take = lit_run_take(mgl_pk_type(win.pk) == MGL_LITERAL, st.pos - win.base, limit);
	if (!take) return 0;
	uint32_t& n = INS ? ch.n_ins : ch.n_rem;
	if (n + 9u * take > ch.cap || n + ch.n_cancel + 9u * take > MGL_BIG_CAP) { ch.overflow = true; ch.list_full = true; return take; }
	LitLane ll;
	if (!lit_run_plan(c, win, st, take, lane, ll)) return 0;
	if (ll.active) {
		const uint32_t at = n + lane;
		if (INS) { ch.ins_key[at] = (uint16_t)(ll.ctx | (ll.bit << 15)); ch.ins_pos[at] = ll.p; }
		else { ch.rem_key[at] = (uint16_t)ll.ctx; ch.rem_pos[at] = ll.p; }
	}
	n += 9u * take;
	st.pos += take;
	st.ctx_state = lit_steps(st.ctx_state, take);
	return take;
}

/* The base's adaptive model before the first base packet at or after y, into LDS: dense
 * checkpoint + replay of < 2^MGL_CK2_SHIFT bytes of base packets.
 * model_load_inl is the body, always inlined: the fused instance calls it directly -- left to the inliner it is a call there,
 * and a call takes the kernel's DevCtx and Base2 arguments by reference, i.e. a copy of both in scratch (640 B/lane). */
__device__ __forceinline__ void model_load_inl(const DevCtx& c, const Base2& b, uint16_t* probs, const uint16_t* T, uint32_t y, uint32_t lane)
{
	const uint32_t ck = y >> MGL_CK2_SHIFT;
	/* 16 bytes per lane and four loads in flight per trip (rows are 16-byte multiples, 16-byte aligned on both sides):
	 * a 5 KiB model is two round trips instead of twenty-one */
	const uint4* src = (const uint4*)(b.ck_probs + (size_t)ck * b.ck_elems);
	uint4* dst = (uint4*)probs;
	const uint32_t n16 = b.ck_elems / 8u;
	for (uint32_t base = 0; base < n16; base += 256u) {
		uint4 r[4];
#pragma unroll
		for (uint32_t u = 0; u < 4; u++) { const uint32_t i = base + u * 64u + lane; if (i < n16) r[u] = src[i]; }
#pragma unroll
		for (uint32_t u = 0; u < 4; u++) { const uint32_t i = base + u * 64u + lane; if (i < n16) dst[i] = r[u]; }
	}
	/* first base packet start in [ck << shift, y): one bitmap word holds the whole checkpoint block */
	const uint32_t first = ck << MGL_CK2_SHIFT;
	const uint64_t bits = b.onwalk[first >> 6] & ((y & 63u) ? ((1ull << (y & 63u)) - 1ull) : 0ull) & (~0ull << (first & 63u));
	wave_sync();
	if (bits) {
		const uint32_t start = uni(((first >> 6) << 6) + ctz64(bits));
		Walk w;
		walk_reset(w);
		w.st = uni_state(base_state_at(b, start));
		while (w.st.pos < y) {
			win_cover(w.win, c, b.slab, w.st.pos, lane);
			if (w.st.ctx_state < 7u) {
				/* a run of plain literals (lit_run_plan): their probability updates are applied packet by packet
				 * (the packets share contexts: is_match and the top of the literal tree), which is all that has
				 * to stay in order */
				const uint32_t take = lit_run_take(mgl_pk_type(w.win.pk) == MGL_LITERAL, w.st.pos - w.win.base, y - w.st.pos);
				LitLane ll;
				if (take && lit_run_plan(c, w.win, w.st, take, lane, ll)) {
					for (uint32_t r = 0; r < take; r++) {
						if (ll.active && ll.i == r) probs[ll.ctx] = (uint16_t)mgl_prob_update(probs[ll.ctx], ll.bit);
						wave_sync();
					}
					w.st.pos += take; w.st.ctx_state = lit_steps(w.st.ctx_state, take);
					w.packets += take;
					continue;
				}
			}
			const mgl_pk pk = win_pk(w.win, w.st.pos);
			walk_packet<true>(w, c.L, c.data, probs, T, mgl_pk_type(pk), mgl_pk_dist(pk), mgl_pk_len(pk), lane);
		}
		wave_sync();
	}
}
__device__ void model_load(const DevCtx& c, const Base2& b, uint16_t* probs, const uint16_t* T, uint32_t y, uint32_t lane)
{
	model_load_inl(c, b, probs, T, y, lane);
}

/* the Walk-based helpers of the full-walk path read the input through Walk's window */
__device__ __forceinline__ void walk_from_state(Walk& w, const mgl_wstate& st)
{
	walk_reset(w);
	w.st = st;
}

#include "mgl_nbr2.h" /* scratch slots and change-list helpers, NbrArgs / Nbr / NbrWalk, the continuation record, the fused hand, the outputs */
/* MODE: the regular launch is split in two so that each half needs fewer registers and more
 * wavefronts fit a SIMD (top-K is the register hog):
 *   MGL_NBR_PICK  everything up to the mutated packet: target, walk state, and -- unless the
 *                 mutation is a grow/shrink -- the model at the target and the top-K pick; the
 *                 picked packet and the RNG position go to `pickrec`;
 *   MGL_NBR_REST  recomputes the cheap part, takes the pick from `pickrec`, then window walk and
 *                 chain re-simulation.  A repair that needs another top-K pick (rare) hands the
 *                 neighbour to the next pass;
 *   MGL_NBR_FULL  the whole thing in one kernel (the BIG second pass, which starts from scratch);
 *   MGL_NBR_PICKWALK  the two halves' bodies one behind the other in one wavefront (the split form's default launch): the
 *                 same code on the same inputs, but no launch boundary -- and so no wait for the slice's slowest top-K
 *                 query -- between a neighbour's pick and its walk.  Not the phase machine as one kernel (246 VGPRs):
 *                 nothing but a handful of wave-uniform scalars (PickHand) lives across the top-K. */
#ifndef MGL_REST_WAVES_PER_SIMD
#define MGL_REST_WAVES_PER_SIMD 4
#endif
#define MGL_NBR_FULL 0
#define MGL_NBR_PICK 1
#define MGL_NBR_REST 2
#define MGL_NBR_PICKWALK 3
/* ---- the second pass's re-simulations, by the whole workgroup
 *
 * A second-pass workgroup is MGL_BIG_WAVES wavefronts on one neighbour.  Wavefront 0 evaluates the neighbour (nbr2_one);
 * the others wait in coop_helpers and take part in its re-simulations only -- the overlay at a repair pick and the final
 * one -- the way k_sim's wavefronts share a regular neighbour's contexts.  Wavefront 0 lists the distinct contexts, posts a
 * command in LDS and then runs the same three barriers as the helpers (coop_share):
 *     A   the command is posted              -> everyone copies its share of the two lists into LDS
 *     B   the lists are in LDS               -> everyone re-simulates contexts wid * 64 + lane, + blockDim.x, ...
 *     C   sums (and overlay values) are in   -> wavefront 0 adds the sums up and walks on
 * Wavefront 0 reaches barrier A only in coop_sim and once more, with EXIT, behind its loop over the units (every return
 * of nbr2_one leads there); a helper leaves at A on EXIT or when the generation has not advanced.  No barrier sits in
 * divergent code, nothing spins. */
#ifndef MGL_BIG_WAVES
#define MGL_BIG_WAVES 4u /* one per SIMD: the instance keeps its 256 VGPRs + AGPRs at one wavefront per SIMD */
#endif
#define MGL_COOP_SIM 1u
#define MGL_COOP_EXIT 2u
#define MGL_COOP_BYTES 128u /* LDS the command takes, behind the copy of the lists */
struct CoopCmd {
	uint32_t gen;     /* advanced by wavefront 0 with every command */
	uint32_t op;
	uint32_t slot;    /* the neighbour's scratch slot: lists and context list */
	uint32_t n_ins, n_rem, nu, limit;
	uint32_t overlay; /* byte offset of wavefront 0's model in the workgroup's LDS; 0: no overlay */
	unsigned long long sum[MGL_BIG_WAVES];
};
static_assert(sizeof(CoopCmd) <= MGL_COOP_BYTES, "CoopCmd outgrew its LDS");
__device__ __forceinline__ CoopCmd* coop_cmd(unsigned char* smem, uint32_t per_wave_bytes)
{
	return (CoopCmd*)(smem + 4096u + per_wave_bytes + 12u * MGL_BIG_CAP);
}
/* every wavefront of the workgroup, behind barrier A: barriers B and C are in here */
__device__ __forceinline__ void coop_share(const DevCtx& c, const Base2& b, const BigScratch& big, unsigned long long* dbg, unsigned char* smem,
                                           uint32_t per_wave_bytes, const uint16_t* T, CoopCmd* cmd, uint32_t lane, uint32_t wid)
{
	const uint32_t slot = uni(cmd->slot), overlay = uni(cmd->overlay);
	Changes cl;
	changes_reset(cl);
	cl.n_ins = uni(cmd->n_ins); cl.n_rem = uni(cmd->n_rem);
	cl.ctxbits = nullptr; cl.nbitwords = 0; cl.dbg = dbg; cl.diag = c.diag_stop;
	/* the lists sit in the slot's global scratch; a re-simulation scans them once per touched context, so it works on a copy
	 * in LDS (behind wavefront 0's area: the second pass's launch reserves it) */
	changes_use_slot(cl, big, slot);
	const uint16_t* gik = cl.ins_key; const uint32_t* gip = cl.ins_pos;
	const uint16_t* grk = cl.rem_key; const uint32_t* grp = cl.rem_pos;
	uint32_t* cp = (uint32_t*)(smem + 4096u + per_wave_bytes);
	cl.ins_pos = cp; cl.rem_pos = cp + MGL_BIG_CAP;
	cl.ins_key = (uint16_t*)(cp + 2u * MGL_BIG_CAP); cl.rem_key = cl.ins_key + MGL_BIG_CAP;
	cl.cap = MGL_BIG_CAP;
	for (uint32_t e = threadIdx.x; e < cl.n_ins; e += blockDim.x) { cl.ins_pos[e] = gip[e]; cl.ins_key[e] = gik[e]; }
	for (uint32_t e = threadIdx.x; e < cl.n_rem; e += blockDim.x) { cl.rem_pos[e] = grp[e]; cl.rem_key[e] = grk[e]; }
	__syncthreads(); /* B */
	const int64_t mine = chain_sim_contexts(b, cl, T, uni(cmd->limit), overlay ? (uint16_t*)(smem + overlay) : nullptr, lane, wid * 64u, blockDim.x, uni(cmd->nu));
	const uint64_t u = wave_sum64((uint64_t)mine);
	if (lane == 0) cmd->sum[wid] = u;
	__syncthreads(); /* C */
}
/* wavefront 0, at either re-simulation site of the second pass: chain_sim with the workgroup's help */
__device__ __forceinline__ int64_t coop_sim(const DevCtx& c, const Base2& b, const BigScratch& big, unsigned long long* dbg, unsigned char* smem,
                                            uint32_t per_wave_bytes, const uint16_t* T, Changes& ch, uint32_t slot, uint32_t limit, uint16_t* overlay,
                                            uint32_t lane, bool* too_many)
{
	const uint32_t nu = chain_list(ch, lane, too_many); /* from the lists in global memory: one pass over the keys */
	if (*too_many) return 0;
	if (ch.diag == 41) return (int64_t)nu;
	CoopCmd* cmd = coop_cmd(smem, per_wave_bytes);
	if (lane == 0) {
		cmd->op = MGL_COOP_SIM; cmd->slot = slot; cmd->n_ins = ch.n_ins; cmd->n_rem = ch.n_rem; cmd->nu = nu; cmd->limit = limit;
		cmd->overlay = overlay ? (uint32_t)((unsigned char*)overlay - smem) : 0u;
		cmd->gen = cmd->gen + 1u;
	}
	__syncthreads(); /* A */
	coop_share(c, b, big, dbg, smem, per_wave_bytes, T, cmd, lane, 0u);
	uint64_t d = 0;
	for (uint32_t w = 0; w < (blockDim.x >> 6); w++) d += cmd->sum[w];
	wave_sync();
	return (int64_t)d;
}
/* wavefronts 1 .. of a second-pass workgroup */
__device__ __forceinline__ void coop_helpers(const DevCtx& c, const Base2& b, const BigScratch& big, unsigned long long* dbg, unsigned char* smem,
                                             uint32_t per_wave_bytes, const uint16_t* T, uint32_t lane, uint32_t wid)
{
	CoopCmd* cmd = coop_cmd(smem, per_wave_bytes);
	uint32_t seen = 0;
	for (;;) {
		__syncthreads(); /* A */
		const uint32_t gen = uni(cmd->gen);
		if (uni(cmd->op) == MGL_COOP_EXIT || gen == seen) return;
		seen = gen;
		coop_share(c, b, big, dbg, smem, per_wave_bytes, T, cmd, lane, wid);
	}
}

/* ================================================================== one neighbour: nbr2_one and its stages */

/* ---- the stages of nbr2_one, in its order */

/* Reads the launch's LDS geometry.  Leaves the journal (empty), the bitmap, the model's and the price tables' place, and the lists'.
 * LDS per wavefront: [journal | context bitmap | union].  The union holds EITHER the model + top-K price tables (while the
 * mutation is chosen) OR the change lists (afterwards): the lists only start to fill once the mutated packet is known.  A
 * repair that needs another top-K pick while the lists are live is handed to the BIG pass, whose lists are in global memory.
 * This keeps 11 instead of 8 wavefronts per CU. */
template <int MODE>
__device__ __forceinline__ unsigned char* nbr_wave_area(const DevCtx& c, const NbrArgs& a, Nbr& n)
{
	unsigned char* mine = a.smem + ((MODE == MGL_NBR_REST || MODE == MGL_NBR_PICK) ? 0u : 4096u) + (size_t)a.wid * a.per_wave_bytes;
	Journal& jn = n.jn; Changes& ch = n.ch;
	jn.old = (mgl_pk*)mine;
	jn.neu = jn.old + MGL_MAX_DIFFS;
	jn.pos = (uint32_t*)(jn.neu + MGL_MAX_DIFFS);
	jn.count = 0; jn.overflow = false;
	ch.nbitwords = (c.L.total + 31u) >> 5;
	ch.ctxbits = jn.pos + MGL_MAX_DIFFS;
	/* the pick half never reads the journal or the bitmap: its wave area is the model + price tables alone */
	unsigned char* uni_base = MODE == MGL_NBR_PICK ? mine : (unsigned char*)(ch.ctxbits + ((ch.nbitwords + 3u) & ~3u));
	const uint32_t cap = a.big.chg_cap;
	ch.ins_pos = (uint32_t*)uni_base;
	ch.rem_pos = ch.ins_pos + cap;
	ch.ins_key = (uint16_t*)(ch.rem_pos + cap);
	ch.rem_key = ch.ins_key + cap;
	ch.uctx = ch.rem_key + cap;
	ch.cap = cap; ch.uctx_cap = 2 * cap;
	return uni_base;
}

/* Reads the step's targets or draws one; n.crec / n.resumed.  Leaves n.pos, the neighbour's walk state there (w.nb) and the RNG
 * position.  Five sources: the pick body's hand (fused; with it comes n.first), the pick half's state record, a continuation
 * record, the step's stratified targets, the neighbour's own draws (same rule as the full-walk path).  The pick half puts what it
 * found on record for the walk half */
template <bool BIG, int MODE, bool FUSED>
__device__ __forceinline__ void nbr_target(const DevCtx& c, const Base2& b, const NbrArgs& a, uint32_t lane, Nbr& n, NbrWalk& w, NbrRng& rng, const PickHand* hand)
{
	const uint32_t j = n.j;
	uint32_t target;
	mgl_wstate& nb = w.nb;
	if (MODE == MGL_NBR_REST && FUSED) {
		hand_take_target(hand, n, rng, nb);
		return;
	} else if (MODE == MGL_NBR_REST) {
		const uint4 s0 = a.pickstate[2u * j], s1 = a.pickstate[2u * j + 1u];
		target = s0.x; rng.n = s0.y;
		nb.pos = target; nb.ctx_state = s0.z;
		nb.dists[0] = s0.w; nb.dists[1] = s1.x; nb.dists[2] = s1.y; nb.dists[3] = s1.z;
	} else if (BIG && n.resumed) {
		cont_resume_target(n.crec, &target, nb);
	} else if (c.strat_pre != nullptr) {
		target = uni(c.strat_tgt[j]); /* stratified_target(), worked out for the whole step by k_targets */
		rng.n = 1;
		nb = uni_state(base_state_at(b, target));
	} else {
		uint32_t mydraw = lane < 32 ? mgl_rng_draw(rng.key, lane) % c.n : 0;
		bool on = lane < 32 && ((b.onwalk[mydraw >> 6] >> (mydraw & 63u)) & 1ull);
		unsigned long long m = __ballot(on);
		if (m) {
			int f = __ffsll((long long)m) - 1;
			target = rdlane(mydraw, (uint32_t)f);
			rng.n = (uint32_t)f + 1;
		} else {
			rng.n = 32;
			uint32_t p = rdlane(mydraw, 31);
			uint32_t wd = p >> 6;
			uint64_t bits = b.onwalk[wd] & (~0ull << (p & 63u));
			while (!bits && ++wd < b.nw0) bits = b.onwalk[wd];
			target = uni(bits ? (wd << 6) + ctz64(bits) : 0u);
		}
		nb = uni_state(base_state_at(b, target));
	}
	if (MODE == MGL_NBR_PICK && !FUSED && lane == 0) { /* one of the last two sources */
		a.pickstate[2u * j] = make_uint4(target, rng.n, nb.ctx_state, nb.dists[0]);
		a.pickstate[2u * j + 1u] = make_uint4(nb.dists[1], nb.dists[2], nb.dists[3], 0u);
	}
	n.pos = target;
}

/* Reads the packets at the target and behind it, the state there, one draw.  Leaves n.mutated and, if set, n.m_first (and
 * w.second_set, w.m_second), journalled except in the pick half; *second: the base's packet behind the target where the rule read
 * and rewrote it.  mutate, packet_slab_neighbour.c:119-152.  nbr_will_pick, below, is the rule once more */
template <int MODE>
__device__ __forceinline__ void nbr_grow_shrink(const DevCtx& c, const Base2& b, uint32_t lane, Nbr& n, NbrWalk& w, NbrRng& rng, mgl_pk* second_out)
{
	const uint32_t pos = n.pos;
	const mgl_pk first = n.first;
	if (pos + 1 < c.n && (nbr_draw(rng) % 2u) == 0) {
		const mgl_pk second = uni64(b.slab[pos + 1]);
		const uint32_t ft = mgl_pk_type(first), flen = mgl_pk_len(first);
		const uint32_t st = mgl_pk_type(second), slen = mgl_pk_len(second), sdist = mgl_pk_dist(second);
		if ((ft == MGL_LONG_REP || ft == MGL_MATCH) && flen > 2) {
			w.m_second = mgl_pack(ft, mgl_pk_dist(first), flen - 1);
			n.m_first = MGL_PK_LITERAL;
			*second_out = second;
			if (MODE != MGL_NBR_PICK) { journal_set(n.jn, pos, first, n.m_first, lane); journal_set(n.jn, pos + 1, second, w.m_second, lane); }
			w.second_set = true; n.mutated = true;
		} else if ((ft == MGL_LITERAL || ft == MGL_SHORT_REP) && (st == MGL_MATCH || st == MGL_LONG_REP)) {
			const mgl_wstate nb = w.nb; /* a copy, here and in rep_taint_step: mgl_dist_at then chooses among four values, not among pointers into w, which would keep all of w in memory */
			uint32_t rep_start = pos - (st == MGL_LONG_REP ? mgl_dist_at(&nb, sdist) : sdist);
			if (slen < MGL_MAX_MATCH && rep_start > 0 && rep_start <= pos && win_byte(n.win, pos) == c.data[rep_start - 1]) {
				n.m_first = mgl_pack(st, sdist, slen + 1);
				if (MODE != MGL_NBR_PICK) journal_set(n.jn, pos, first, n.m_first, lane);
				n.mutated = true;
			}
		}
	}
}
/* Will neighbour j pick, or does it take a grow/shrink mutation and go straight into its walk?  nbr_grow_shrink's rule a second
 * time (draw 1 of the neighbour's stream, the packets at the target and behind it, the rep distances there, two input bytes), for
 * k_targets.  There are two because one rule for both, with the distance look-up handed in, moved a neighbour kernel's row for the
 * worse (the one-kernel form: 604 -> 620 B/lane of scratch): this one reads the slab and the state itself and only answers, the
 * other works on what its wavefront holds and journals as it decides.
 * It only orders a launch (k_pick_order): a wrong answer costs time, never a result.  tests/test_gpu_pick_order.py holds the two
 * together.  Every load is inside its buffer whatever the slab holds: pos < n, and base_state_at looks at positions below pos. */
__device__ __forceinline__ bool nbr_will_pick(const DevCtx& c, const Base2& b, uint32_t pos, uint64_t key)
{
	if (pos >= c.n || pos + 1 >= c.n || (mgl_rng_draw(key, 1) % 2u) != 0) return true;
	const mgl_pk first = b.slab[pos], second = b.slab[pos + 1];
	const uint32_t ft = mgl_pk_type(first), flen = mgl_pk_len(first);
	const uint32_t st = mgl_pk_type(second), slen = mgl_pk_len(second), sdist = mgl_pk_dist(second);
	if ((ft == MGL_LONG_REP || ft == MGL_MATCH) && flen > 2) return false;
	if ((ft == MGL_LITERAL || ft == MGL_SHORT_REP) && (st == MGL_MATCH || st == MGL_LONG_REP)) {
		uint32_t d = sdist;
		if (st == MGL_LONG_REP) { const mgl_wstate nb = base_state_at(b, pos); d = mgl_dist_at(&nb, sdist); }
		const uint32_t rep_start = pos - d;
		if (slen < MGL_MAX_MATCH && rep_start > 0 && rep_start <= pos && c.data[pos] == c.data[rep_start - 1]) return false;
	}
	return true;
}

/* Reads the pick record (the pick half's, or the pick body's hand) of a neighbour without a grow/shrink.  Leaves the mutated packet
 * journalled, the RNG position behind the pick, and the walk as the next phase -- or no candidate, and the end.  The second pass,
 * too, takes the mutation's pick from the first half when there was one */
template <int MODE, bool FUSED>
__device__ __forceinline__ void nbr_take_pick(const NbrArgs& a, uint32_t lane, Nbr& n, NbrRng& rng, const PickHand* hand)
{
	const uint4 rec = (MODE == MGL_NBR_REST && FUSED) ? hand_take_pick(hand) : a.pickrec[n.j];
	if (!(rec.w & 1u)) { n.generate_failed = true; n.phase = P_OUT; }
	else {
		n.m_first = (mgl_pk)rec.x | ((mgl_pk)rec.y << 32);
		journal_set(n.jn, n.pos, n.first, n.m_first, lane);
		rng.n = rec.z;
		n.pick_is_mutation = false;
		n.phase = P_WALK;
	}
}

/* P_MODEL.  Reads w.pick_pos and the lists.  Leaves the base's adaptive model before the first base packet at or after pick_pos in
 * probs (dense checkpoint + replay of < 64 bytes of base packets); live lists, which share the model's LDS, are moved to a global
 * scratch slot first.  Next: P_SIM (overlay: the touched contexts' re-simulated values) when there are lists, else P_TOPK.
 * Returns true where a diagnostic stop ends the neighbour */
template <bool PROF, bool FUSED>
__device__ __forceinline__ bool phase_model(const DevCtx& c, const Base2& b, const NbrArgs& a, uint32_t lane, const uint16_t* T, Nbr& n, const NbrWalk& w, uint16_t* probs, PickProf& pp)
{
	const BigScratch& big = a.big; Changes& ch = n.ch;
	if ((ch.n_ins + ch.n_rem) != 0 && !n.spilled) {
		uint32_t sl = 0;
		if (lane == 0) sl = atomicAdd(big.spill_ctr, 1u);
		sl = uni(sl);
		if (sl >= big.slots) { ch.overflow = true; n.phase = P_OUT; return false; }
		lists_copy_to_slot(ch, big, sl, lane);
		__threadfence_block();
		wave_sync();
		changes_use_slot(ch, big, sl);
		n.spilled = true;
	}
	if constexpr (FUSED) model_load_inl(c, b, probs, T, w.pick_pos, lane);
	else model_load(c, b, probs, T, w.pick_pos, lane);
	if (PROF) pick_prof_mark(&pp, PS_MODEL, lane);
	if (!n.pick_is_mutation) prof_mark(n.prof, 5, lane); /* repair: base model at the pick position */
	if (n.pick_is_mutation) {
		prof_mark(n.prof, 1, lane); /* model at target */
		if (c.diag_stop == 2) { if (lane == 0) nbr_out_diag(a.out, n.j, probs[lane]); return true; }
	}
	/* ... with the touched contexts overridden by their re-simulated values */
	if ((ch.n_ins + ch.n_rem) != 0) { n.sim_limit = w.pick_pos; n.sim_overlay = true; n.phase = P_SIM; }
	else n.phase = P_TOPK;
	return false;
}

/* P_SIM.  Reads the lists and the request (n.sim_limit, n.sim_overlay).  Three forms.  The walk half holds no re-simulation code: its
 * lists go to k_sim, which puts several wavefronts on one neighbour's contexts and writes the cost, and it ends (P_OUT; journal and
 * counters are written there).  The second pass re-simulates with its workgroup (coop_sim), the one-kernel form alone (chain_sim):
 * an overlay leaves the model at a repair pick overridden (next: P_TOPK), the final one leaves n.delta (next: P_OUT) */
template <bool BIG, int MODE>
__device__ __forceinline__ void phase_sim(const DevCtx& c, const Base2& b, const NbrArgs& a, uint32_t lane, const uint16_t* T, Nbr& n, uint16_t* probs)
{
	const BigScratch& big = a.big; Changes& ch = n.ch;
	const uint32_t j = n.j;
	if (MODE == MGL_NBR_REST) {
		uint16_t* gk = big.sim_keys + (size_t)j * (2u * big.chg_cap);
		uint32_t* gp = big.sim_pos + (size_t)j * (2u * big.chg_cap);
		lists_copy_out(ch, gk, gp, gk + big.chg_cap, gp + big.chg_cap, lane);
		/* no fence: the consumer is a later launch on a stream that waits for this one */
		if (lane == 0) big.sim_hdr[j] = make_uint4(ch.n_ins, ch.n_rem, (uint32_t)(uint64_t)ch.direct, (uint32_t)((uint64_t)ch.direct >> 32));
		n.sim_deferred = true;
		n.phase = P_OUT;
		return;
	}
	int64_t r;
	if (BIG) r = coop_sim(c, b, big, a.prof_acc, a.smem, a.per_wave_bytes, T, ch, n.slot, n.sim_limit, n.sim_overlay ? probs : nullptr, lane, &n.too_many);
	else r = chain_sim(b, ch, T, n.sim_limit, n.sim_overlay ? probs : nullptr, lane, &n.too_many);
	wave_sync();
	if (n.too_many) { n.phase = P_OUT; return; }
	if (n.sim_overlay) { prof_mark(n.prof, 6, lane); n.phase = P_TOPK; } /* repair: model overridden by the re-simulated values */
	else { n.delta = r; prof_mark(n.prof, 4, lane); n.phase = P_OUT; }
}

/* P_TOPK.  Reads the model in probs and the request (n.pick_is_mutation: at the target against n.first; else w.pick_*).  The pick
 * half records the pick and ends (returns true, as a diagnostic stop does).  Otherwise leaves the mutated packet journalled, or the
 * repair's pick in w.picked_pk / w.have_pick; next: P_WALK -- or no candidate at the target, and P_OUT */
template <int MODE, bool PROF, bool FUSED>
__device__ __forceinline__ bool phase_topk(const DevCtx& c, const Base2& b, const NbrArgs& a, uint32_t lane, const uint16_t* T, Nbr& n, NbrWalk& w, NbrRng& rng, Walk& tw, uint16_t* probs, uint32_t* lencost, const TopkPlan& plan, PickProf& pp, PickHand* hand)
{
	const uint32_t j = n.j;
	walk_from_state(tw, w.nb);
	win_cover(tw.win, c, b.slab, tw.st.pos, lane);
	mgl_pk picked;
	bool ok;
	if constexpr (MODE == MGL_NBR_PICK) ok = pick_from_top_k<4, true, PROF>(c, tw, probs, T, lencost, w.pick_inc, w.pick_best, rng, lane, &picked, &plan, &pp);
	else {
		/* a call, which is what the inliner made of it while the phases were one function: said here, so that the one-kernel form and
		 * the second pass keep the registers, the scratch and the wavefronts per SIMD they had */
		[[clang::noinline]] ok = pick_from_top_k<1>(c, tw, probs, T, lencost, w.pick_inc, w.pick_best, rng, lane, &picked);
	}
	if (MODE == MGL_NBR_PICK) {
		if (lane == 0) a.pickrec[j] = make_uint4((uint32_t)picked, (uint32_t)(picked >> 32), rng.n, ok ? 1u : 0u); /* fused, too: the second pass restarts from it */
		if (FUSED) hand_put_pick(hand, picked, rng, ok);
		if (PROF) pick_prof_mark(&pp, PS_DRAW, lane);
		if (PROF && pp.acc && lane == 0) pp.acc[2u * MGL_PICK_STAGES + j] = __builtin_readcyclecounter() - n.t_begin; /* a picking wavefront's lifetime */
		return true;
	}
	if (n.pick_is_mutation) {
		if (!ok) { n.generate_failed = true; n.phase = P_OUT; return false; }
		n.m_first = picked;
		journal_set(n.jn, n.pos, n.first, n.m_first, lane);
		n.pick_is_mutation = false;
		prof_mark(n.prof, 2, lane); /* top-K */
		if (c.diag_stop == 3 || (c.diag_stop >= TS_FIRST && c.diag_stop <= TS_LAST)) { if (lane == 0) nbr_out_diag(a.out, j, (uint32_t)n.m_first); return true; }
	} else {
		w.picked_pk = ok ? picked : w.pick_inc;
		w.have_pick = true;
		prof_mark(n.prof, 7, lane); /* repair: top-K */
	}
	n.win.base = 0xFFFFFFFFu;
	n.phase = P_WALK;
	return false;
}

/* ---- P_WALK's pieces */

/* mgl_advance for a state inside NbrWalk, on a copy: mgl_advance chooses among the rep distances by pointer, and a pointer chosen
 * among w's fields keeps all of w in memory (144 B/lane of scratch in every walking instance) */
__device__ __forceinline__ void walk_advance(mgl_wstate& st, uint32_t type, uint32_t dist, uint32_t len)
{
	mgl_wstate s = st;
	mgl_advance(&s, type, dist, len);
	st = s;
}

/* the base packet at w.bs.pos goes away: its events to the removed list, the base's walk a packet on */
__device__ __forceinline__ void base_packet_out(const DevCtx& c, const Base2& b, uint32_t lane, Nbr& n, NbrWalk& w)
{
	win_cover(n.win, c, b.slab, w.bs.pos, lane);
	const mgl_pk bpk = win_pk(n.win, w.bs.pos);
	mgl_plan bpl;
	plan_at(c.L, c.data, w.bs, mgl_pk_type(bpk), mgl_pk_dist(bpk), mgl_pk_len(bpk), win_byte(n.win, w.bs.pos), bpl);
	changes_add<false>(n.ch, bpl, w.bs.pos, lane);
	walk_advance(w.bs, mgl_pk_type(bpk), mgl_pk_dist(bpk), mgl_pk_len(bpk));
}

enum { REPAIR_PACKET, REPAIR_STOP, REPAIR_SAVED };
/* The repair rules of packet_slab_neighbour.c:82-117 for the neighbour's packet at p (not its first, not one back from a pick).
 * Leaves the packet the base codes there for this neighbour (*old) and the packet it gets (*pk): REPAIR_PACKET.  A long rep that
 * validates under no slot needs a top-K pick: the base's walk is caught up to p (the model at p needs every base packet that starts
 * before p priced in) and the request left in w.pick_*; REPAIR_STOP, with *request_pick -- or with n.walk_long (too many picks)
 * or an overflow.  The walk half holds no top-K code: with continuation records it saves the walk as it stands -- here, where
 * everything is live anyway, so that the walk loop carries no value for it -- hands the neighbour to the second pass and ends,
 * REPAIR_SAVED */
template <bool BIG, int MODE>
__device__ __forceinline__ uint32_t repair_packet(const DevCtx& c, const Base2& b, const NbrArgs& a, uint32_t lane, Nbr& n, NbrWalk& w, NbrRng& rng, Walk& tw, uint32_t p, mgl_pk* pk_out, mgl_pk* old_out, bool* request_pick)
{
	const BigScratch& big = a.big; Changes& ch = n.ch;
	if (w.count < 8) w.count++;
	const mgl_pk old = (w.second_set && p == n.pos + 1) ? w.m_second : win_pk(n.win, p);
	mgl_pk pk = old;
	*old_out = old;
	uint32_t type = mgl_pk_type(pk);
	if (type == MGL_SHORT_REP || (type == MGL_LITERAL && w.count < 4)) {
		const bool same = w.nb.dists[0] < p && win_byte(n.win, p) == c.data[p - w.nb.dists[0] - 1];
		if (same) { if (w.count < 4) pk = MGL_PK_SHORT_REP; }
		else pk = MGL_PK_LITERAL;
	}
	type = mgl_pk_type(pk);
	if (type == MGL_LONG_REP) {
		const uint32_t len = mgl_pk_len(pk);
		uint32_t idx = mgl_pk_dist(pk);
		walk_from_state(tw, w.nb);
		bool ok = long_rep_ok(c, tw, idx, len, lane);
		for (uint32_t i = 0; i < 4 && !ok; i++) { idx = i; ok = long_rep_ok(c, tw, idx, len, lane); }
		pk = mgl_pack(MGL_LONG_REP, idx, len);
		if (!ok) {
			if (++w.npicks > MGL_MAX_REPAIR_PICKS) { n.walk_long = true; return REPAIR_STOP; }
			w.pick_best = (nbr_draw(rng) % 4u) == 0;
			while (w.bs.pos < p && !ch.overflow) base_packet_out(c, b, lane, n, w);
			if (ch.overflow) return REPAIR_STOP;
			w.resume_old = old; w.pick_pos = p; w.pick_inc = pk;
			if (MODE == MGL_NBR_REST && big.cont != nullptr) {
				uint32_t slot2 = 0;
				if (lane == 0) {
					atomicAdd(big.spill_ctr + 1, 1u); /* repair picks this step */
					slot2 = atomicAdd(a.todo_count, 1u);
					a.todo[slot2] = n.j;
					nbr_out_none(a.out, n.j, n.pos, 0, MGL_WIN_NONE);
				}
				slot2 = uni(slot2);
				if (slot2 < big.slots) { /* else: no scratch slot, the second pass sends it on to the full walk */
					lists_copy_to_slot(ch, big, slot2, lane);
					cont_save(big.cont + (size_t)slot2 * MGL_CONT_WORDS, n.j, n.pos, w, rng, n.jn, ch, lane);
				}
				return REPAIR_SAVED;
			}
			*request_pick = true;
			if (!BIG && lane == 0) atomicAdd(big.spill_ctr + 1, 1u); /* repair picks this step */
			return REPAIR_STOP; /* -> P_MODEL, then back to the walk with w.have_pick */
		}
	}
	*pk_out = pk;
	return REPAIR_PACKET;
}

/* which rep distances the neighbour's packet pk at p reads and pushes: bit k of w.taint = distance k comes from before the window.
 * A rep packet: the soft window reaches at least to behind it -- unless it is the base's own packet at this position reading a slot
 * that holds the same distance in both walks (the move has no part in what it codes) */
__device__ __forceinline__ void rep_taint_step(const Nbr& n, NbrWalk& w, uint32_t p, mgl_pk pk)
{
	const uint32_t ntype = mgl_pk_type(pk), ndist = mgl_pk_dist(pk);
	if (ntype == MGL_SHORT_REP || ntype == MGL_LONG_REP) {
		const uint32_t slot = ntype == MGL_SHORT_REP ? 0u : ndist;
		const mgl_wstate nb = w.nb, bs = w.bs;
		const bool same_read = bs.pos == p && win_pk(n.win, p) == pk && mgl_dist_at(&nb, slot) == mgl_dist_at(&bs, slot);
		if (!same_read) w.wsoft = 0xFFFFFFFFu;
		w.dep |= ntype == MGL_SHORT_REP ? (w.taint & 1u) : ((w.taint >> ndist) & 1u);
	}
	if (ntype == MGL_MATCH) w.taint = (w.taint << 1) & 0xFu;
	else if (ntype == MGL_LONG_REP) w.taint = (w.taint & ~((2u << ndist) - 1u)) | ((w.taint & ((1u << ndist) - 1u)) << 1) | ((w.taint >> ndist) & 1u);
}

/* is pk at p the base's packet at the same position, coded identically (its events cancel whole)?  Which events a packet produces
 * depends on the packet, ctx_state, the position and -- for a literal after a match -- the byte at rep distance 0; decided before
 * anything is planned */
__device__ __forceinline__ bool codes_identically(const DevCtx& c, const Nbr& n, const NbrWalk& w, uint32_t p, mgl_pk pk)
{
	bool cancelled = false;
	if (w.bs.pos == p && win_pk(n.win, p) == pk && w.nb.ctx_state == w.bs.ctx_state) {
		cancelled = true;
		if (mgl_pk_type(pk) == MGL_LITERAL && w.nb.ctx_state >= 7) {
			const uint32_t mn = w.nb.dists[0] < p ? c.data[p - w.nb.dists[0] - 1] : 0u;
			const uint32_t mb = w.bs.dists[0] < p ? c.data[p - w.bs.dists[0] - 1] : 0u;
			cancelled = mn == mb;
		}
	}
	return cancelled;
}

/* P_WALK: the two-pointer walk over neighbour packets (w.nb) and base packets (w.bs) from where w stands, until both code
 * identically again.  Leaves the lists, the journal and n.wend; next: P_SIM (the final re-simulation), P_MODEL (a repair's pick:
 * back here with w.have_pick) or P_OUT (n.walk_long, an overflow).  Returns true where the neighbour has ended: its walk saved
 * in a continuation record, or a diagnostic stop */
template <bool BIG, int MODE>
__device__ __forceinline__ bool phase_walk(const DevCtx& c, const Base2& b, const NbrArgs& a, uint32_t lane, Nbr& n, NbrWalk& w, NbrRng& rng, Walk& tw)
{
	Changes& ch = n.ch; Journal& jn = n.jn; Win& win = n.win;
	bool request_pick = false;
	while (w.nb.pos < c.n || w.bs.pos < c.n) {
		if (ch.overflow || jn.overflow || n.too_many || ++w.guard > (BIG ? (1u << 20) : 4096u)) { ch.overflow = true; break; }
		if (!w.first_packet && !w.have_pick && w.nb.pos == w.bs.pos && w.count >= 3) {
			const bool same_ctx = w.nb.ctx_state == w.bs.ctx_state;
			const bool same_d = w.nb.dists[0] == w.bs.dists[0] && w.nb.dists[1] == w.bs.dists[1] && w.nb.dists[2] == w.bs.dists[2] &&
			                    w.nb.dists[3] == w.bs.dists[3];
			if (same_ctx && w.wsoft == 0xFFFFFFFFu) w.wsoft = w.nb.pos;
			if (same_ctx && same_d) break; /* the rest of the file is coded identically */
			if (same_ctx && w.nb.ctx_state < 7) {
				/* plain literals up to the next special packet code identically: skip them */
				uint32_t sx = uni(sp_find_next(b, w.nb.pos));
				if (sx == MGL_POS_INF || sx > c.n) sx = c.n;
				if (sx > w.nb.pos) {
					const uint32_t cs = lit_steps(w.nb.ctx_state, sx - w.nb.pos);
					w.nb.pos = w.bs.pos = sx; w.nb.ctx_state = w.bs.ctx_state = cs;
					w.count = 8;
					continue;
				}
			}
		}
		if (w.walked > MGL_MAX_WALK && !w.have_pick) { n.walk_long = true; break; }
		if ((w.have_pick || w.nb.pos <= w.bs.pos) && w.nb.pos < c.n) {
			/* ---- next neighbour packet */
			const uint32_t p = w.nb.pos;
			win_cover(win, c, b.slab, p, lane);
			mgl_pk pk, old = 0;
			if (w.have_pick) {
				pk = w.picked_pk; old = w.resume_old; w.have_pick = false; /* back from the top-K pick for this packet */
			} else if (w.first_packet) {
				pk = n.m_first; /* :169 the mutated packet is coded as is */
			} else {
				const uint32_t r = repair_packet<BIG, MODE>(c, b, a, lane, n, w, rng, tw, p, &pk, &old, &request_pick);
				if (r == REPAIR_SAVED) return true;
				if (r == REPAIR_STOP) break;
			}
			if (!w.first_packet && pk != old) {
				const mgl_pk base_old = (w.second_set && p == n.pos + 1) ? uni64(b.slab[p]) : old;
				journal_set(jn, p, base_old, pk, lane);
				w.wsoft = 0xFFFFFFFFu; /* a changed packet (a SHORT_REP the repair turned into a literal, say): the soft window reaches behind it */
			}
			w.first_packet = false;
			w.walked++;
			const uint32_t ntype = mgl_pk_type(pk), ndist = mgl_pk_dist(pk), nlen = mgl_pk_len(pk);
			rep_taint_step(n, w, p, pk);
			if (codes_identically(c, n, w, p, pk)) {
				walk_advance(w.bs, ntype, ndist, nlen);
			} else {
				/* of the base packet only a key per lane and two counts stay live while the neighbour's is planned */
				uint32_t bkey = 0, bnev = 0, bndirect = 0;
				if (w.bs.pos == p) {
					const mgl_pk bpk = win_pk(win, p);
					const uint32_t btype = mgl_pk_type(bpk), bdist = mgl_pk_dist(bpk), blen = mgl_pk_len(bpk);
					mgl_plan bpl;
					plan_at(c.L, c.data, w.bs, btype, bdist, blen, win_byte(win, p), bpl);
					bnev = bpl.nev; bndirect = bpl.ndirect;
					if (lane < bnev) {
						uint32_t cx, bt;
						mgl_plan_event(&bpl, lane, &cx, &bt);
						bkey = cx | (bt << 15);
					}
					walk_advance(w.bs, btype, bdist, blen);
				}
				mgl_plan npl;
				plan_at(c.L, c.data, w.nb, ntype, ndist, nlen, win_byte(win, p), npl);
				changes_add_pair(ch, bkey, bnev, bndirect, npl, p, lane, a.big.evcancel != 0);
			}
			walk_advance(w.nb, ntype, ndist, nlen);
		} else {
			/* ---- a base packet the neighbour has already passed over: its events go away, a run of plain literals at a time */
			win_cover(win, c, b.slab, w.bs.pos, lane);
			if (literal_run_events<false>(c, ch, win, w.bs, (w.nb.pos < c.n ? w.nb.pos : c.n) - w.bs.pos, lane)) continue;
			base_packet_out(c, b, lane, n, w);
		}
	}
	if (n.walk_long) { n.phase = P_OUT; return false; }
	if (request_pick) { prof_mark(n.prof, 3, lane); n.phase = P_MODEL; return false; }
	prof_mark(n.prof, 3, lane); /* window walk */
	if (c.diag_stop == 4) { if (lane == 0) nbr_out_diag(a.out, n.j, ch.n_ins + ch.n_rem); return true; }
	if (ch.overflow || jn.overflow || n.too_many) { n.phase = P_OUT; return false; }
	n.wend = w.nb.pos;
	n.sim_limit = MGL_POS_INF; n.sim_overlay = false; n.phase = P_SIM;
	return false;
}

/* The end of a neighbour that left the phases without a result.  Reads how they ended; returns false for the one that has a result */
template <bool BIG>
__device__ __forceinline__ bool nbr_out_unfinished(const NbrArgs& a, uint32_t lane, const Nbr& n, const NbrWalk& w)
{
	const uint32_t j = n.j;
	if (n.generate_failed) { /* no candidate at the target (main.c:81-84 retries those) */
		if (lane == 0) nbr_out_none(a.out, j, n.pos, 0, MGL_WIN_NONE);
		return true;
	}
	if (n.jn.overflow) { /* same rule as the full-walk path and the oracle: dropped */
		if (lane == 0) nbr_out_none(a.out, j, n.pos, w.walked, MGL_WIN_DROPPED);
		return true;
	}
	if (n.walk_long || (n.ch.list_full && n.ch.cap == a.big.cap && !n.jn.overflow)) {
		/* more inserted or removed events than the second pass's lists hold (MGL_BIG_CAP), or more than MGL_MAX_WALK packets
		 * visited before the walks met again: dropped, like a neighbour with too long a journal; the oracle counts the same */
		if (lane == 0) nbr_out_none(a.out, j, n.pos, w.walked, MGL_WIN_DROPPED);
		return true;
	}
	if (n.ch.overflow || n.too_many) {
		/* does not fit the change lists: hand it to the next pass (BIG, then the full-walk kernel) */
		if (lane == 0) {
			const uint32_t slot2 = atomicAdd(a.todo_count, 1u);
			a.todo[slot2] = j;
			if (BIG) atomicAdd((unsigned long long*)&a.ctl->fallback_nbrs, 1ull);
			nbr_out_none(a.out, j, n.pos, 0, MGL_WIN_NONE);
		}
		return true;
	}
	return false;
}

/* one neighbour, by the wavefront a.wid of its workgroup; `unit` = the neighbour's index in this launch's slice
 * (regular launch) or its slot in the second pass's list (BIG).  `hand`: the fused instance, whose two bodies are this function
 * as the pick half and as the walk half */
template <bool BIG, int MODE, bool PROF = false, bool FUSED = false>
__device__ __forceinline__ void nbr2_one(const DevCtx& c, const Base2& b, const NbrArgs& a, uint32_t lane, const uint16_t* T, uint32_t unit, PickHand* hand = nullptr)
{
	static_assert(!FUSED || (!BIG && !PROF && (MODE == MGL_NBR_PICK || MODE == MGL_NBR_REST)), "the fused instance is the two halves of the regular launch");
	const BigScratch& big = a.big;
	Nbr n; NbrWalk w; NbrRng rng;
	/* ---- which neighbour: [j_base, j_end) is the slice of the step this launch covers */
	n.j = a.j_base + unit; n.slot = 0;
	n.t_begin = a.prof_acc ? __builtin_readcyclecounter() : 0ull;
	if (BIG) {
		n.slot = unit;
		const uint32_t nflag = *big.todo_in_count;
		if (n.slot >= nflag) return;
		n.j = uni(big.todo_in[n.slot]);
		if (lane == 0) atomicAdd((unsigned long long*)&a.ctl->big_nbrs, 1ull); /* counted where the second pass takes it up */
	}
	if (n.j >= a.K || (!BIG && n.j >= a.j_end)) return;
	unsigned char* const uni_base = nbr_wave_area<MODE>(c, a, n);
	uint16_t* const probs = (uint16_t*)uni_base;                                   /* the model */
	uint32_t* const lencost = (uint32_t*)(uni_base + (size_t)b.ck_elems * 2); /* top-K's price tables */
	if (BIG) {
		if (n.slot >= big.slots) { /* more flagged neighbours than scratch slots: full walk */
			if (lane == 0) { const uint32_t s2 = atomicAdd(a.todo_count, 1u); a.todo[s2] = n.j; }
			return;
		}
		changes_use_slot(n.ch, big, n.slot);
	}
	changes_reset(n.ch);
	n.too_many = false; n.spilled = BIG;
	const uint64_t gstep = a.step_override != ~0ull ? a.step_override : a.ctl->gstep;
	rng.key = mgl_rng_key(a.seed, gstep, n.j); rng.n = 0;
	/* second pass: a walk the second half saved at its repair pick (same neighbour, same slot) is taken up there */
	n.crec = (BIG && big.cont != nullptr) ? big.cont + (size_t)n.slot * MGL_CONT_WORDS : nullptr;
	n.resumed = BIG && n.crec != nullptr && cont_holds(n.crec, n.j);

	/* ---- the target, the state there and the base's packet */
	if (MODE == MGL_NBR_REST && lane == 0) big.sim_hdr[n.j] = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
	nbr_target<BIG, MODE, FUSED>(c, b, a, lane, n, w, rng, hand);
	/* the pick half keeps its own stage clock (PickProf: stages behind the second half's lifetimes in the profile buffer) */
	prof_start(n.prof, MODE == MGL_NBR_PICK ? nullptr : a.prof_acc);
	n.ch.dbg = MODE == MGL_NBR_PICK ? nullptr : a.prof_acc;
	PickProf pp; /* PROF: the pick half's profiled instance, launched only under MGL_F_PROFILE */
	pp.acc = PROF ? a.prof_acc + 32u + a.K : nullptr;
	pp.t = n.t_begin;
	n.ch.diag = c.diag_stop;
	w.bs = w.nb;
	win_reset(n.win);
	Walk tw; /* scratch Walk for top-K (its window is the input window at the query position) */
	if (!(MODE == MGL_NBR_REST && FUSED)) { win_cover(n.win, c, b.slab, n.pos, lane); n.first = win_pk(n.win, n.pos); } /* from the hand: the walk covers its window itself */
	if (MODE == MGL_NBR_PICK && FUSED) hand_put_target(hand, n, w.nb);
	prof_mark(n.prof, 0, lane); /* state at target */
	if (c.diag_stop == 1) { if (lane == 0) nbr_out_diag(a.out, n.j, (uint32_t)n.first); return; }

	/* ---- the mutation: a grow/shrink, decided here, or a top-K pick (the phases) */
	n.m_first = n.first; w.m_second = 0;
	w.second_set = false; n.mutated = false;
	mgl_pk second = 0; /* the base's packet behind the target, where a grow/shrink rewrote it */
	if (MODE == MGL_NBR_REST && FUSED) {
		/* the pick body's grow/shrink decision: journalled here, not made again */
		hand_take_mutation(hand, n, w, &second);
		if (n.mutated) {
			journal_set(n.jn, n.pos, n.first, n.m_first, lane);
			if (w.second_set) journal_set(n.jn, n.pos + 1, second, w.m_second, lane);
		}
	} else if (!(BIG && n.resumed)) nbr_grow_shrink<MODE>(c, b, lane, n, w, rng, &second);
	n.phase = n.mutated ? P_WALK : P_MODEL;
	if (MODE == MGL_NBR_PICK && FUSED) hand_put_mutation(hand, n, w, rng, second);
	if (MODE == MGL_NBR_PICK && n.mutated) { /* nothing to pick: the second half redoes the grow/shrink itself */
		if (!FUSED && lane == 0) reinterpret_cast<uint32_t*>(a.pickstate)[8u * n.j + 7u] = 1u; /* the decision, on record for the tests of the class hint (mgl_debug_dump 28) */
		return;
	}
	/* where the pick's sources start and end depends on the target and the rep distances alone: searched for here, all
	 * sources level by level, in front of the model load instead of source by source behind it */
	TopkPlan plan;
	if (MODE == MGL_NBR_PICK) {
		if (PROF) pick_prof_mark(&pp, PS_TARGET, lane);
		topk_plan_make(plan, c, w.nb, lane);
		if (PROF) pick_prof_mark(&pp, PS_PLAN, lane);
	}
	if (MODE == MGL_NBR_REST && c.diag_stop != 0 && c.diag_stop != 4 && c.diag_stop < 40) return; /* diagnostic stops of the first half */

	/* ---- the walk at its start: the pending pick is the mutation's; or the walk a continuation record holds, at its repair pick */
	n.pick_is_mutation = !n.mutated;
	w.pick_pos = n.pos; w.pick_inc = n.first; w.pick_best = false;
	w.have_pick = false; w.picked_pk = 0; w.resume_old = 0;
	w.count = 0; w.walked = 0; w.npicks = 0; w.guard = 0;
	w.wsoft = 0xFFFFFFFFu; w.taint = 0xFu; w.dep = 0u;
	w.first_packet = true;
	n.sim_limit = MGL_POS_INF; n.sim_overlay = false; n.delta = 0;
	n.generate_failed = false; n.sim_deferred = false; n.walk_long = false;
	n.wend = 0;
	if (BIG && n.resumed) {
		cont_resume(n.crec, w, rng, n.jn, n.ch, lane);
		n.mutated = true; n.pick_is_mutation = false;
		n.phase = P_MODEL;
	}
	/* the host passes the pick records only when the split form ran */
	if ((MODE == MGL_NBR_REST || (BIG && a.pickrec != nullptr)) && !n.mutated) nbr_take_pick<MODE, FUSED>(a, lane, n, rng, hand);

	/* ---- the rest runs as a small phase machine so that each big piece of code (model load, chain re-simulation, top-K) exists
	 * exactly once in the kernel: the mutation's top-K pick and a repair's top-K pick share one site, and so do the overlay
	 * re-simulation (model at a repair position) and the final one.  Halves the code size and the register pressure. */
	for (;;) {
		if (MODE == MGL_NBR_REST && (n.phase == P_MODEL || n.phase == P_TOPK)) { n.ch.overflow = true; n.phase = P_OUT; continue; } /* repair pick without a continuation record: the next pass evaluates the neighbour again */
		if (MODE != MGL_NBR_REST && n.phase == P_MODEL) { if (phase_model<PROF, FUSED>(c, b, a, lane, T, n, w, probs, pp)) return; }
		if (MODE != MGL_NBR_PICK && n.phase == P_SIM) { phase_sim<BIG, MODE>(c, b, a, lane, T, n, probs); }
		if (MODE != MGL_NBR_REST && n.phase == P_TOPK) { if (phase_topk<MODE, PROF, FUSED>(c, b, a, lane, T, n, w, rng, tw, probs, lencost, plan, pp, hand)) return; }
		if (MODE != MGL_NBR_PICK && n.phase == P_WALK) { if (phase_walk<BIG, MODE>(c, b, a, lane, n, w, rng, tw)) return; }
		if (n.phase == P_OUT) break;
	}

	if (nbr_out_unfinished<BIG>(a, lane, n, w)) return;
	nbr_out_result(a, lane, n, w);
}

template <bool BIG, int MODE, bool PROF = false>
__global__ void __launch_bounds__((MODE == MGL_NBR_PICK ? 512 : (BIG ? 64 * MGL_BIG_WAVES : 64)), (MODE == MGL_NBR_FULL ? (BIG ? 1 : MGL_NBR_WAVES_PER_SIMD) : (MODE == MGL_NBR_REST ? MGL_REST_WAVES_PER_SIMD : 4))) /* MGL_NBR_PICKWALK: (64, 4) */ k_neighbours2(DevCtx c, Base2 b, Control* ctl, uint64_t seed,
                                                     uint64_t step_override, uint32_t K, NbrOut out, uint32_t per_wave_bytes,
                                                     uint32_t* todo, uint32_t* todo_count, unsigned long long* prof_acc,
                                                     BigScratch big, uint4* pickrec, uint32_t j_base, uint32_t j_end, uint4* pickstate)
{
	/* Which form of the regular launch runs (split: pick + rest + k_sim, or the one-kernel form) is the host's
	 * choice per block of steps (mgl_sa_run reads the device's recommendation, Control::nbr_single): only the
	 * chosen form is launched.  The second pass is launched with a small grid whatever its list holds -- the
	 * host does not know the count -- and strides over it, a workgroup per neighbour; with an empty list a
	 * workgroup costs one load. */
	const uint32_t waves = blockDim.x >> 6;
	if (BIG && blockIdx.x >= *big.todo_in_count) return; /* uniform over the workgroup */
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	uint16_t* T = (uint16_t*)smem;
	if (BIG && threadIdx.x == 0) { CoopCmd* cmd = coop_cmd(smem, per_wave_bytes); cmd->gen = 0; cmd->op = MGL_COOP_SIM; }
	/* 4 KiB as 256 16-byte units (the table is hipMalloc-aligned, T sits at the start of the LDS block); the second
	 * half of the split form prices nothing (its re-simulation is k_sim's) and has no table: 4 KiB less per workgroup */
	if (MODE == MGL_NBR_PICK || MODE == MGL_NBR_PICKWALK) {
		/* the pick half reads the 4 KiB cost table through the vector cache instead of keeping a copy in LDS: 16 instead of 11
		 * wavefronts per CU at 10 MB (c3 neighbour kernels - 5 %), no change at 100 KB */
		T = const_cast<uint16_t*>(c.cost_tbl);
	} else if (MODE != MGL_NBR_REST) {
		for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) reinterpret_cast<uint4*>(T)[i] = reinterpret_cast<const uint4*>(c.cost_tbl)[i];
		__syncthreads();
	}
	const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
	/* the fused instance has no stage marks, and its `pickstate` is the launch's order (below); the fused launch's wavefront and the
	 * second pass's evaluating one are their workgroups' wavefront 0 */
	constexpr bool FUSED = MODE == MGL_NBR_PICKWALK;
	const NbrArgs a{ctl, seed, step_override, K, out, per_wave_bytes, todo, todo_count, FUSED ? nullptr : prof_acc, big, pickrec, j_base, j_end,
	                FUSED ? nullptr : pickstate, smem, (FUSED || BIG) ? 0u : wid};
	if constexpr (MODE == MGL_NBR_PICKWALK) {
		/* one wavefront per workgroup: the pick body, then the walk body on the same LDS area (the pick's model and price
		 * tables are dead by then).  Each body's returns end that body alone: a neighbour whose pick body returned early
		 * (grow/shrink, a diagnostic stop) still gets its walk body, which takes the same decision from the same values. */
		static_assert(!BIG && !PROF, "the fused instance is a regular launch without stage marks");
		/* which neighbour of the slice: the launch's order (k_pick_order: the picking neighbours first) travels in the `pickstate`
		 * slot, which this instance has no other use for; null = blockIdx order */
		const uint32_t* const order = reinterpret_cast<const uint32_t*>(pickstate);
		const uint32_t unit = order != nullptr ? order[j_base + blockIdx.x] - j_base : blockIdx.x;
		PickHand hand;
		hand.target = 0; hand.rng_n = 0; hand.ctx_state = 0; hand.dists[0] = hand.dists[1] = hand.dists[2] = hand.dists[3] = 0;
		hand.first = hand.second = hand.m_first = hand.m_second = 0; hand.flags = 0;
		nbr2_one<false, MGL_NBR_PICK, false, true>(c, b, a, lane, T, unit, &hand);
		wave_sync(); /* the walk body's journal and lists overwrite what the pick body's lanes read */
		nbr2_one<false, MGL_NBR_REST, false, true>(c, b, a, lane, T, unit, &hand);
	} else if (BIG) {
		/* wavefront 0 takes the workgroup's neighbours one at a time; the others help with their re-simulations */
		if (wid != 0) { coop_helpers(c, b, big, prof_acc, smem, per_wave_bytes, T, lane, wid); return; }
		const uint32_t n = *big.todo_in_count;
		for (uint32_t unit = blockIdx.x; unit < n; unit += gridDim.x)
			nbr2_one<BIG, MODE, PROF>(c, b, a, lane, T, unit);
		if (lane == 0) { CoopCmd* cmd = coop_cmd(smem, per_wave_bytes); cmd->op = MGL_COOP_EXIT; cmd->gen = cmd->gen + 1u; }
		__syncthreads(); /* A, for the last time: the helpers leave */
	} else {
		nbr2_one<BIG, MODE, PROF>(c, b, a, lane, T, blockIdx.x * waves + wid);
	}
}


/* ================================================================== k_sim
 *
 * The re-simulation of the split launch's second half, as its own launch: MGL_SIM_WAVES wavefronts
 * per neighbour share its touched contexts (one context per lane, as in chain_sim), so a neighbour
 * with 150 contexts is one trip instead of three.  The second half's duration is its slowest
 * wavefront (the mean one lives a third of that), and the slowest are the ones with many contexts.
 * Small kernel: no walk state, no journal -- 64 VGPRs less than the second half. */
#ifndef MGL_SIM_WAVES
#define MGL_SIM_WAVES 2u   /* the regular launch: thousands of neighbours, a hundred contexts each */
#endif
#define MGL_SIM_WAVES_MAX 8u
struct SimShared {
	uint16_t* T;
	uint32_t* dyn;
	unsigned long long* sum;
	uint32_t* nu_many; /* [0] distinct contexts, [1] too many */
};
template <bool COUNT>
__device__ __forceinline__ void sim_one(const DevCtx& c, const Base2& b, Control* ctl, const NbrOut& out, const BigScratch& big, const uint4* hdrs,
                                        uint32_t j, const SimShared& sh, unsigned long long* traffic_ctr)
{
	const uint4 hdr = hdrs[j];
	if (hdr.x == 0xFFFFFFFFu) return; /* failed, dropped or handed on: its cost is written (uniform over the workgroup) */
	const uint32_t cap = big.chg_cap;
	uint32_t* s_bits = sh.dyn;
	uint32_t* s_pos = sh.dyn + ((((c.L.total + 31u) >> 5) + 3u) & ~3u);
	uint16_t* s_key = (uint16_t*)(s_pos + 2u * cap);
	uint16_t* s_uctx = s_key + 2u * cap;
	const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
	Changes ch;
	ch.n_ins = hdr.x; ch.n_rem = hdr.y;
	ch.ins_pos = s_pos; ch.rem_pos = s_pos + cap;
	ch.ins_key = s_key; ch.rem_key = s_key + cap;
	ch.uctx = s_uctx; ch.ctxbits = s_bits;
	ch.cap = cap; ch.uctx_cap = 2 * cap;
	ch.nbitwords = (c.L.total + 31u) >> 5;
	ch.direct = 0; ch.n_cancel = 0; ch.dbg = nullptr; ch.diag = c.diag_stop; ch.overflow = false; ch.list_full = false;
	const uint16_t* gk = big.sim_keys + (size_t)j * (2u * cap);
	const uint32_t* gp = big.sim_pos + (size_t)j * (2u * cap);
	for (uint32_t e = threadIdx.x; e < ch.n_ins; e += blockDim.x) { s_key[e] = gk[e]; s_pos[e] = gp[e]; }
	for (uint32_t e = threadIdx.x; e < ch.n_rem; e += blockDim.x) { s_key[cap + e] = gk[cap + e]; s_pos[cap + e] = gp[cap + e]; }
	__syncthreads();
	if (wid == 0) {
		/* The list cannot run out of room here.  Both change lists were filled by the walk half, where changes_add and the
		 * literal-run path refuse an event beyond `cap` per list and raise list_full; such a neighbour goes to the second pass
		 * and its header stays 0xFFFFFFFF, so it never gets here.  What does get here has n_ins <= cap and n_rem <= cap, hence
		 * at most n_ins + n_rem <= 2 cap = uctx_cap distinct contexts, whatever chg_cap is set to (mgl_debug_set key 2). */
		bool too_many = false;
		const uint32_t nu = chain_list(ch, lane, &too_many);
		if (lane == 0) { sh.nu_many[0] = nu; sh.nu_many[1] = too_many ? 1u : 0u; }
	}
	__syncthreads();
	if (sh.nu_many[1]) { /* the invariant above is broken: no cost, and the run ends with an error instead of dropping the neighbour quietly */
		if (threadIdx.x == 0) {
			atomicOr(&ctl->error_flags, MGL_ERR_SIM_LIST);
			out.cost[j] = MGL_INVALID_COST; out.ndiffs[j] = 0; out.walked[j] = 0; out.win[2u * j + 1u] = MGL_WIN_NONE;
		}
		return;
	}
	if (c.diag_stop == 41) { if (threadIdx.x == 0) out.cost[j] = sh.nu_many[0]; return; } /* diagnostic: listing only */
	uint32_t traffic = 0;
	const int64_t mine = chain_sim_contexts(b, ch, sh.T, MGL_POS_INF, nullptr, lane, wid * 64u, blockDim.x, sh.nu_many[0], COUNT ? &traffic : nullptr);
	const uint64_t u = wave_sum64((uint64_t)mine);
	if (lane == 0) sh.sum[wid] = u;
	if (COUNT) {
		/* + the change lists this workgroup brought into LDS (6 bytes per event), once per neighbour */
		const uint64_t tb = wave_sum64((uint64_t)traffic) + (wid == 0 ? 6ull * (ch.n_ins + ch.n_rem) + 16ull : 0ull);
		if (lane == 0) atomicAdd(traffic_ctr, (unsigned long long)tb);
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint64_t d = 0;
		for (uint32_t w = 0; w < (blockDim.x >> 6); w++) d += sh.sum[w];
		const int64_t direct = (int64_t)((uint64_t)hdr.z | ((uint64_t)hdr.w << 32));
		out.cost[j] = (uint64_t)((int64_t)ctl->rebuild_cost + (int64_t)d + direct);
	}
}
/* workgroup x = neighbour j_base + x with header sim_hdr */
/* COUNT: the same kernel adding up the bytes of chain data and change lists it reads (traffic_ctr[0]) and its launches that had
 * work (traffic_ctr[1]); bench.py runs a few steps with it after its timed region */
template <bool COUNT>
__global__ void __launch_bounds__(64 * MGL_SIM_WAVES_MAX, 8) k_sim(DevCtx c, Base2 b, Control* ctl, NbrOut out, BigScratch big, uint32_t j_base, uint32_t j_end,
                                                           unsigned long long* traffic_ctr)
{
	if (j_base + blockIdx.x >= j_end) return;
	__shared__ __attribute__((aligned(16))) uint16_t T[2048];
	/* sized by the launch: one bit per context, then the two lists (positions, keys) and the context list */
	extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];
	__shared__ unsigned long long s_sum[MGL_SIM_WAVES_MAX];
	__shared__ uint32_t s_nm[2];
	if (big.sim_hdr[j_base + blockIdx.x].x == 0xFFFFFFFFu) return; /* before the table load: most launches of a bulk-free step's tail */
	for (uint32_t i = threadIdx.x; i < 256; i += blockDim.x) reinterpret_cast<uint4*>(T)[i] = reinterpret_cast<const uint4*>(c.cost_tbl)[i];
	SimShared sh;
	sh.T = T; sh.dyn = s_dyn; sh.sum = s_sum; sh.nu_many = s_nm;
	sim_one<COUNT>(c, b, ctl, out, big, big.sim_hdr, j_base + blockIdx.x, sh, traffic_ctr);
}


/* ================================================================== packets before every block of 4 096 positions (stratified targets) */
__global__ void __launch_bounds__(64) k_rank_blocks(const uint64_t* onwalk, uint32_t nw0, uint32_t* pre, uint32_t nblk)
{
	const uint32_t blk = blockIdx.x, lane = threadIdx.x;
	if (blk >= nblk) return;
	const uint32_t w = blk * 64u + lane;
	unsigned long long v = w < nw0 ? (unsigned long long)__popcll(onwalk[w]) : 0ull;
	v = wave_sum64(v);
	if (lane == 0) pre[blk + 1u] = (uint32_t)v;
}
__global__ void __launch_bounds__(1024) k_rank_scan(uint32_t* pre, uint32_t nblk)
{
	__shared__ uint32_t s_w[16], s_base;
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
	if (tid == 0) { s_base = 0; pre[0] = 0; }
	__syncthreads();
	for (uint32_t base = 0; base < nblk; base += blockDim.x) {
		const uint32_t i = base + tid;
		const uint32_t v = i < nblk ? pre[i + 1u] : 0u;
		uint32_t incl = v;
		for (int o = 1; o < 64; o <<= 1) { const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64); if ((int)lane >= o) incl += t; }
		if (lane == 63) s_w[wid] = incl;
		__syncthreads();
		uint32_t bsum = s_base;
		for (uint32_t q = 0; q < wid; q++) bsum += s_w[q];
		if (i < nblk) pre[i + 1u] = bsum + incl;
		__syncthreads();
		if (tid == blockDim.x - 1u) s_base = bsum + incl;
		__syncthreads();
	}
}

/* the step's targets: one wavefront per neighbour (mgl_device.h:stratified_target; draw 0 of the neighbour's stream picks the
 * packet inside its slice).  A kernel of its own: in the pick kernel, sixteen wavefronts per CU, the same search was a
 * dozen dependent loads at the head of every wavefront's critical path.  With `hint` (incremental engine) it also says which
 * neighbours will pick: 1 = picks, 0 = grow/shrink.  Exact where the slab is final when this runs (behind k_apply_walk of a
 * single step), a guess behind a batch accept.  FOCUS: the launch passes a focus window; without one the instantiation is the
 * kernel as it was before there were windows (two unused arguments), so that a search without a window pays nothing. */
template <bool FOCUS>
__global__ void __launch_bounds__(256) k_targets(DevCtx c, Base2 b, const uint64_t* onwalk, uint32_t nw0, const Control* ctl, uint64_t seed, uint64_t step_override,
                                                 uint32_t K, uint32_t* tgt, unsigned char* hint, uint32_t focus_lo, uint32_t focus_hi)
{
	const uint32_t j = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (j >= K) return;
	const uint64_t gstep = step_override != ~0ull ? step_override : ctl->gstep;
	const uint64_t key = mgl_rng_key(seed, gstep, j);
	/* packets on the walk: the last prefix sum (Control::packets says the same once the accept is through; this kernel may run beside it);
	 * under a focus window (FOCUS: focus_hi != 0; kernel arguments: DevCtx stays as the neighbour kernels know it) the packets that start inside it */
	uint32_t first = 0, P = c.strat_pre[c.strat_nblk];
	if (FOCUS) P = focus_ordinals(onwalk, nw0, c.strat_pre, focus_lo, focus_hi, lane, &first);
	const uint32_t t = stratified_target(onwalk, nw0, c.strat_pre, c.strat_nblk, first, P, K, j, mgl_rng_draw(key, 0), lane);
	if (lane == 0) tgt[j] = t;
	if (hint != nullptr) {
		const bool picks = nbr_will_pick(c, b, t, key); /* uniform: t is */
		if (lane == 0) hint[j] = picks ? 1 : 0;
	}
}
/* what k_targets makes of a focus window on the current walk (mgl_sa_focus): out[0] = the first ordinal, out[1] = the packets.
 * One wavefront, behind k_rank_blocks / k_rank_scan. */
__global__ void __launch_bounds__(64) k_focus_count(const uint64_t* onwalk, uint32_t nw0, const uint32_t* pre, uint32_t focus_lo, uint32_t focus_hi, uint32_t* out)
{
	uint32_t first = 0;
	const uint32_t count = focus_ordinals(onwalk, nw0, pre, focus_lo, focus_hi, threadIdx.x, &first);
	if (threadIdx.x == 0) { out[0] = first; out[1] = count; }
}

/* slice h of `slices` of a step's K neighbours is [mgl_slice_bound(K, h, slices), mgl_slice_bound(K, h + 1, slices)): the
 * launches of launch_neighbours and the order below cut the step at the same places */
__host__ __device__ __forceinline__ uint32_t mgl_slice_bound(uint32_t K, uint32_t h, uint32_t slices) { return (uint32_t)((uint64_t)K * h / slices); }

/* of a flag per thread of a 1 024-thread workgroup: how many threads below this one have it set, and (*total) how many in all */
__device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t* s_w, uint32_t* total)
{
	const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
	const unsigned long long m = __ballot(flag);
	__syncthreads(); /* the previous use of s_w is read */
	if (lane == 0) s_w[wid] = (uint32_t)__popcll(m);
	__syncthreads();
	uint32_t below = 0, all = 0;
	for (uint32_t q = 0; q < 16u; q++) { const uint32_t v = s_w[q]; if (q < wid) below += v; all += v; }
	*total = all;
	return below + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}
/* The order in which a fused launch takes up the neighbours of its slice: workgroup x evaluates order[j0 + x].  Workgroups
 * start in blockIdx order; with the picking neighbours (hint != 0) in front, ascending in j, and the grow/shrink ones behind
 * them, ascending too, the last slot round of a launch holds short walk-only wavefronts instead of picking ones seven times
 * in ten.  (Measured on c3: all walk-only neighbours at the end beats half of them, evenly spread, which beats none: DESIGN.md
 * section 5.)  One workgroup per slice; a permutation of [j0, j1) whatever the hint bytes hold. */
__global__ void __launch_bounds__(1024) k_pick_order(const unsigned char* hint, uint32_t* order, uint32_t K, uint32_t slices)
{
	__shared__ uint32_t s_w[16];
	const uint32_t j0 = mgl_slice_bound(K, blockIdx.x, slices), j1 = mgl_slice_bound(K, blockIdx.x + 1u, slices);
	uint32_t picking = 0; /* of the slice: where its walk-only neighbours start */
	for (uint32_t s = j0; s < j1; s += 1024u) {
		const uint32_t j = s + threadIdx.x;
		uint32_t t;
		(void)block_rank(j < j1 && hint[j] != 0, s_w, &t);
		picking += t;
	}
	uint32_t front_seen = 0, back_seen = 0;
	for (uint32_t s = j0; s < j1; s += 1024u) {
		const uint32_t j = s + threadIdx.x;
		const bool in = j < j1, front = in && hint[j] != 0;
		uint32_t tf;
		const uint32_t rf = block_rank(front, s_w, &tf);
		if (front) order[j0 + front_seen + rf] = j;
		else if (in) order[j0 + picking + back_seen + (threadIdx.x - rf)] = j; /* the threads below an in-range thread are in range */
		const uint32_t n_in = j1 - s < 1024u ? j1 - s : 1024u;
		front_seen += tf; back_seen += n_in - tf;
	}
}
