/*
 * mgl_kernels.hip -- CDNA4 (gfx950) kernels around the base slab.
 *
 *   ckpt_store / ckpt_load   prefix checkpoints of the model
 *   k_rebuild      walk the base slab: on-walk bitmap, prefix checkpoints, total cost
 *                  (== the loop of main.c:116-118 under perplexity_encoder.c:6-17)
 *   k_neighbours   the full-walk engine, the last resort behind the incremental kernels (mgl_kernels2.hip): one wavefront per
 *                  neighbour walks to the end of the file: mutate (packet_slab_neighbour.c:119-152), top-K pick
 *                  (mgl_topk.hip), repair + cost (:82-117)
 *   k_copy_best    main.c:91
 *   k_substrings / k_import / k_export / k_fill_literal   parity hook and layout conversion
 *
 * Integer table-lookup work: no MFMA.  Probabilities (u16) and the bit-cost table live in
 * LDS; the input, the slab and the match index stay in HBM/L2 and are read coalesced.
 */
#include "mgl_device.h"

/* ================================================================== checkpoints */

__device__ __forceinline__ void ckpt_store(const BaseView& b, const DevCtx& c, uint32_t ci, const uint16_t* probs,
                                           const Walk& w, uint64_t cum, uint32_t lane)
{
	uint32_t* dst = (uint32_t*)(b.ckpt_probs + (size_t)ci * b.ckpt_elems);
	const uint32_t* src = (const uint32_t*)probs;
	for (uint32_t i = lane; i < b.ckpt_elems / 2; i += 64) dst[i] = src[i];
	if (lane == 0) {
		CkptHdr h;
		h.pos = w.st.pos; h.ctx_state = w.st.ctx_state;
		h.dists[0] = w.st.dists[0]; h.dists[1] = w.st.dists[1]; h.dists[2] = w.st.dists[2]; h.dists[3] = w.st.dists[3];
		h.ordinal = w.packets; h.pad = 0; h.cum = cum;
		b.ckpt_hdr[ci] = h;
	}
}
__device__ __forceinline__ uint64_t ckpt_load(const BaseView& b, const DevCtx& c, uint32_t ci, uint16_t* probs,
                                              Walk& w, uint32_t lane)
{
	const uint32_t* src = (const uint32_t*)(b.ckpt_probs + (size_t)ci * b.ckpt_elems);
	uint32_t* dst = (uint32_t*)probs;
	for (uint32_t i = lane; i < b.ckpt_elems / 2; i += 64) dst[i] = src[i];
	const CkptHdr* h = &b.ckpt_hdr[ci];
	walk_reset(w);
	w.st.pos = uni(h->pos); w.st.ctx_state = uni(h->ctx_state);
	w.st.dists[0] = uni(h->dists[0]); w.st.dists[1] = uni(h->dists[1]);
	w.st.dists[2] = uni(h->dists[2]); w.st.dists[3] = uni(h->dists[3]);
	w.packets = uni(h->ordinal);
	uint64_t cum = uni64(h->cum);
	wave_sync();
	return cum;
}

/* ================================================================== k_rebuild */
/* One wavefront walks the base slab from the checkpoint that precedes the first changed
 * position (or from byte 0) to the end: rewrites the on-walk bitmap and the prefix
 * checkpoints, counts packets and produces the slab's exact total cost.
 * cum_out (nullable): running total after every packet (parity hook). */
__global__ void __launch_bounds__(64) k_rebuild(DevCtx c, BaseView b, Control* ctl, int from_dirty, uint64_t* cum_out,
                                                uint16_t* final_probs)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	uint16_t* T = (uint16_t*)smem;
	uint16_t* probs = (uint16_t*)(smem + 4096);
	const uint32_t lane = threadIdx.x;
	for (uint32_t i = lane; i < 2048; i += 64) T[i] = c.cost_tbl[i];

	Walk w;
	uint64_t base_cum = 0;
	uint32_t ci = 0;
	if (from_dirty) {
		if (!ctl->accepted_flag) return;
		ci = uni(ctl->dirty_pos) >> MGL_CKPT_SHIFT;
	}
	if (ci == 0) {
		for (uint32_t i = lane; i < b.ckpt_elems; i += 64) probs[i] = MGL_PROB_INIT;
		walk_reset(w);
		wave_sync();
	} else {
		base_cum = ckpt_load(b, c, ci, probs, w, lane);
	}
	uint32_t next_ck = ci; /* next checkpoint index to (re)write: covers positions >= next_ck << SHIFT */
	/* on-walk bitmap: keep the bits below the restart position in its word */
	uint32_t word = w.st.pos >> 6;
	uint64_t bits = 0;
	if (w.st.pos & 63u) bits = b.onwalk[word] & ((1ull << (w.st.pos & 63u)) - 1ull);

	uint32_t guard = 0;
	while (w.st.pos < c.n) {
		const uint32_t pos = w.st.pos;
		if (++guard > c.n) { if (lane == 0) atomicOr(&ctl->error_flags, MGL_ERR_WALK_OVERRUN); break; }
		while (next_ck < b.nckpt && (next_ck << MGL_CKPT_SHIFT) <= pos) {
			uint64_t cum = base_cum + wave_sum64(w.acc);
			ckpt_store(b, c, next_ck, probs, w, cum, lane);
			next_ck++;
		}
		/* flush finished bitmap words */
		const uint32_t pw = pos >> 6;
		if (pw != word) {
			if (lane == 0) b.onwalk[word] = bits;
			for (uint32_t z = word + 1 + lane; z < pw; z += 64) b.onwalk[z] = 0;
			word = pw; bits = 0;
		}
		bits |= 1ull << (pos & 63u);
		win_cover(w.win, c, b.slab, w.st.pos, lane);
		const mgl_pk pk = win_pk(w.win, pos);
		uint32_t type = mgl_pk_type(pk), len = mgl_pk_len(pk), dist = mgl_pk_dist(pk);
		if (!mgl_pk_wellformed(type, dist, len) || len > c.n - pos) { /* not a packet (mgl_model.h): cost as literal */
			type = MGL_LITERAL; len = 1; dist = 0;
			if (lane == 0) atomicOr(&ctl->error_flags, MGL_ERR_WALK_OVERRUN);
		}
		walk_packet<true>(w, c.L, c.data, probs, T, type, dist, len, lane);
		if (cum_out) {
			uint64_t cum = base_cum + wave_sum64(w.acc);
			if (lane == 0) cum_out[w.packets - 1] = cum;
		}
	}
	if (lane == 0) b.onwalk[word] = bits;
	{
		const uint32_t nwords = (c.n + 63u) >> 6;
		for (uint32_t z = word + 1 + lane; z < nwords; z += 64) b.onwalk[z] = 0;
	}
	const uint64_t total = base_cum + wave_sum64(w.acc);
	wave_sync();
	if (final_probs) for (uint32_t i = lane; i < c.L.total; i += 64) final_probs[i] = probs[i];
	if (lane == 0) {
		ctl->packets = w.packets;
		ctl->rebuild_cost = total;
		ctl->final_ctx_state = w.st.ctx_state;
		ctl->final_dists[0] = w.st.dists[0]; ctl->final_dists[1] = w.st.dists[1];
		ctl->final_dists[2] = w.st.dists[2]; ctl->final_dists[3] = w.st.dists[3];
		if (from_dirty) {
			if (ctl->cur_cost != total) atomicOr(&ctl->error_flags, MGL_ERR_REBUILD_MISMATCH);
			ctl->accepted_flag = 0;
		}
	}
}

/* ================================================================== k_neighbours */

struct Journal {
	uint32_t* pos; /* LDS, MGL_MAX_DIFFS */
	mgl_pk* old;
	mgl_pk* neu;
	uint32_t count; /* uniform */
	bool overflow;
};
__device__ __forceinline__ void journal_set(Journal& jn, uint32_t pos, mgl_pk old, mgl_pk neu, uint32_t lane)
{
	/* the mutated pair (first two entries) may be touched again by the repair */
	for (uint32_t i = 0; i < jn.count && i < 2; i++) {
		if (jn.pos[i] == pos) { if (lane == 0) jn.neu[i] = neu; wave_sync(); return; }
	}
	if (jn.count >= MGL_MAX_DIFFS) { jn.overflow = true; return; }
	if (lane == 0) { jn.pos[jn.count] = pos; jn.old[jn.count] = old; jn.neu[jn.count] = neu; }
	jn.count++;
	wave_sync();
}

/* packet_slab_neighbour.c:74-80: memcmp over the rep source, all lanes compare */
__device__ __forceinline__ bool long_rep_ok(const DevCtx& c, const Walk& w, uint32_t idx, uint32_t len, uint32_t lane)
{
	const uint32_t rd = mgl_dist_at(&w.st, idx);
	if (rd >= w.st.pos || w.st.pos + len > c.n) return false;
	const uint32_t src = w.st.pos - rd - 1u;
	bool bad = false;
	for (uint32_t i = lane; i < len; i += 64) bad |= c.data[src + i] != c.data[w.st.pos + i];
	return __ballot(bad) == 0;
}

/* The neighbour's packet at p: its journal entry if it has one, else the base slab's. */
__device__ __forceinline__ mgl_pk journal_or_base(const Journal& jn, const mgl_pk* slab, uint32_t p, uint32_t lane)
{
	const bool hit = lane < jn.count && jn.pos[lane] == p; /* MGL_MAX_DIFFS == 64: one entry per lane */
	const unsigned long long m = __ballot(hit);
	if (m) return jn.neu[(uint32_t)__ffsll((long long)m) - 1u];
	return slab[p];
}
/* End of the neighbour's window: the first position at which its walk and the base's stand on the
 * same byte with the same ctx_state and rep distances, at least three repair packets after the
 * mutated one (the incremental kernel stops its two-pointer walk there).  The
 * full-walk engine has walked to the end of the file, so it finds the point afterwards from the
 * journal.  `st` = walk state at the target (uniform). */
struct WinInfo { uint32_t end, soft, n_ins, n_rem, walked; };
/* events of one packet (mgl_plan_packet's nev: independent of the bytes) */
__device__ __forceinline__ uint32_t packet_events(const DevCtx& c, const mgl_wstate& st, mgl_pk pk)
{
	mgl_plan pl;
	mgl_plan_packet(&c.L, &st, mgl_pk_type(pk), mgl_pk_dist(pk), mgl_pk_len(pk), 0u, 0u, 0u, &pl);
	return pl.nev;
}
__device__ WinInfo window_end_from_journal(const DevCtx& c, const mgl_pk* slab, const Journal& jn, mgl_wstate st, uint32_t lane)
{
	mgl_wstate nb = st, bs = st;
	uint32_t count = 0, wsoft = 0xFFFFFFFFu, taint = 0xFu, dep = 0u, wend = c.n, n_ins = 0, n_rem = 0, walked = 0;
	bool first = true;
	for (;;) {
		if (!first && nb.pos == bs.pos && count >= 3 && nb.ctx_state == bs.ctx_state) {
			if (wsoft == 0xFFFFFFFFu) wsoft = nb.pos;
			if (nb.dists[0] == bs.dists[0] && nb.dists[1] == bs.dists[1] && nb.dists[2] == bs.dists[2] && nb.dists[3] == bs.dists[3]) { wend = nb.pos; break; }
			if (nb.ctx_state < 7u && nb.pos < c.n) {
				/* plain literals up to the base's next non-literal packet: skipped, not visited (the incremental kernel's jump) */
				uint32_t sx = nb.pos;
				while (sx < c.n && mgl_pk_type(uni64(slab[sx])) == MGL_LITERAL) sx++;
				if (sx > nb.pos) {
					const uint32_t cs = lit_steps(nb.ctx_state, sx - nb.pos);
					nb.pos = bs.pos = sx; nb.ctx_state = bs.ctx_state = cs;
					count = 8;
					continue;
				}
			}
		}
		if (nb.pos >= c.n && bs.pos >= c.n) { wend = c.n; break; }
		if (walked > MGL_MAX_WALK) break;
		if (nb.pos <= bs.pos && nb.pos < c.n) {
			if (!first && count < 8) count++;
			first = false;
			walked++;
			const uint32_t p = nb.pos;
			const mgl_pk pk = uni64(journal_or_base(jn, slab, p, lane));
			const uint32_t ntype = mgl_pk_type(pk), ndist = mgl_pk_dist(pk);
			if (count > 0 && pk != uni64(slab[p])) wsoft = 0xFFFFFFFFu; /* a changed packet: the soft window reaches behind it */
			if (ntype == MGL_SHORT_REP || ntype == MGL_LONG_REP) {
				/* not when it is the base's own packet reading a slot that holds the same distance in both walks */
				const uint32_t slot = ntype == MGL_SHORT_REP ? 0u : ndist;
				const bool same_read = bs.pos == p && uni64(slab[p]) == pk && mgl_dist_at(&nb, slot) == mgl_dist_at(&bs, slot);
				if (!same_read) wsoft = 0xFFFFFFFFu;
				dep |= ntype == MGL_SHORT_REP ? (taint & 1u) : ((taint >> ndist) & 1u);
			}
			if (ntype == MGL_MATCH) taint = (taint << 1) & 0xFu;
			else if (ntype == MGL_LONG_REP) taint = (taint & ~((2u << ndist) - 1u)) | ((taint & ((1u << ndist) - 1u)) << 1) | ((taint >> ndist) & 1u);
			/* identical coding of the base packet at the same position cancels (the rule of the incremental kernel) */
			const bool paired = bs.pos == p;
			mgl_pk bpk = pk;
			bool cancelled = false;
			if (paired) {
				bpk = uni64(slab[p]);
				cancelled = bpk == pk && nb.ctx_state == bs.ctx_state;
				if (cancelled && ntype == MGL_LITERAL && nb.ctx_state >= 7) {
					const uint32_t mn = nb.dists[0] < p ? c.data[p - nb.dists[0] - 1] : 0u;
					const uint32_t mb = bs.dists[0] < p ? c.data[p - bs.dists[0] - 1] : 0u;
					cancelled = mn == mb;
				}
			}
			if (!cancelled) {
				n_ins += packet_events(c, nb, pk);
				if (paired) n_rem += packet_events(c, bs, bpk);
			}
			if (paired) mgl_advance(&bs, mgl_pk_type(bpk), mgl_pk_dist(bpk), mgl_pk_len(bpk));
			mgl_advance(&nb, ntype, ndist, mgl_pk_len(pk));
		} else {
			const mgl_pk pk = uni64(slab[bs.pos]);
			n_rem += packet_events(c, bs, pk);
			mgl_advance(&bs, mgl_pk_type(pk), mgl_pk_dist(pk), mgl_pk_len(pk));
		}
	}
	WinInfo wi;
	wi.n_ins = n_ins; wi.n_rem = n_rem; wi.walked = walked;
	wi.end = wend;
	wi.soft = (wsoft < wend ? wsoft : wend) | (dep << 31);
	return wi;
}

/* One wavefront = one neighbour of the base slab (packet_slab_neighbour.c:154-173). */
/* todo != nullptr: only the neighbours listed there are evaluated (the ones the incremental
 * kernel could not fit), walking from byte 0 instead of from a prefix checkpoint. */
__device__ void nbr_fullwalk_one(const DevCtx& c, const BaseView& b, const Control* ctl, uint64_t seed, uint64_t step_override, uint32_t K,
                                 const NbrOut& out, uint32_t per_wave_bytes, bool from_zero, unsigned char* smem, const uint16_t* T, uint32_t j,
                                 uint32_t lane, uint32_t wid)
{
	if (j >= K) return;
	unsigned char* mine = smem + 4096 + (size_t)wid * per_wave_bytes;
	uint16_t* probs = (uint16_t*)mine;
	uint32_t* lencost = (uint32_t*)(mine + (size_t)b.ckpt_elems * 2);
	Journal jn;
	jn.old = (mgl_pk*)(lencost + MGL_PRICE_WORDS);
	jn.neu = jn.old + MGL_MAX_DIFFS;
	jn.pos = (uint32_t*)(jn.neu + MGL_MAX_DIFFS);
	jn.count = 0; jn.overflow = false;

	const uint64_t gstep = step_override != ~0ull ? step_override : ctl->gstep;
	NbrRng rng; rng.key = mgl_rng_key(seed, gstep, j); rng.n = 0;

	/* target: uniform over the packets of the walk by rejection sampling on positions
	 * (the reference draws a packet ordinal, packet_slab_neighbour.c:162-163) */
	uint32_t target;
	if (c.strat_pre != nullptr) {
		target = uni(c.strat_tgt[j]); /* stratified_target(), worked out for the whole step by k_targets */
		rng.n = 1;
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
			/* next on-walk position at or after p, else 0 */
			const uint32_t nwords = (c.n + 63u) >> 6;
			uint32_t wd = p >> 6;
			uint64_t bits = b.onwalk[wd] & (~0ull << (p & 63u));
			while (!bits && ++wd < nwords) bits = b.onwalk[wd];
			target = bits ? (wd << 6) + (uint32_t)__ffsll((long long)bits) - 1u : 0u;
			target = uni(target);
		}
	}

	/* prefix: nearest checkpoint, then the unchanged packets up to the target (:165) */
	Walk w;
	uint64_t base_cum = 0;
	if (from_zero) {
		for (uint32_t i = lane; i < b.ckpt_elems; i += 64) probs[i] = MGL_PROB_INIT;
		walk_reset(w);
		wave_sync();
	} else {
		base_cum = ckpt_load(b, c, target >> MGL_CKPT_SHIFT, probs, w, lane);
	}
	const uint32_t first_packet = w.packets;
	while (w.st.pos < target) {
		win_cover(w.win, c, b.slab, w.st.pos, lane);
		const mgl_pk pk = win_pk(w.win, w.st.pos);
		walk_packet<true>(w, c.L, c.data, probs, T, mgl_pk_type(pk), mgl_pk_dist(pk), mgl_pk_len(pk), lane);
	}
	if (w.st.pos != target) { /* cannot happen for an on-walk target; fail safe */
		if (lane == 0) { out.cost[j] = MGL_INVALID_COST; out.ndiffs[j] = 0; out.walked[j] = 0; out.win[2u * j] = target; out.win[2u * j + 1u] = MGL_WIN_NONE; }
		return;
	}
	const mgl_wstate st_target = w.st;

	/* mutate, packet_slab_neighbour.c:119-152 */
	const uint32_t pos = target;
	win_cover(w.win, c, b.slab, w.st.pos, lane);
	const mgl_pk first = win_pk(w.win, pos);
	mgl_pk m_first = first, m_second = 0;
	bool second_set = false, mutated = false;
	if (pos + 1 < c.n && (nbr_draw(rng) % 2u) == 0) {
		const mgl_pk second = uni64(b.slab[pos + 1]);
		const uint32_t ft = mgl_pk_type(first), flen = mgl_pk_len(first);
		const uint32_t st = mgl_pk_type(second), slen = mgl_pk_len(second), sdist = mgl_pk_dist(second);
		if ((ft == MGL_LONG_REP || ft == MGL_MATCH) && flen > 2) {
			m_second = mgl_pack(ft, mgl_pk_dist(first), flen - 1);
			m_first = MGL_PK_LITERAL;
			journal_set(jn, pos, first, m_first, lane);
			journal_set(jn, pos + 1, second, m_second, lane);
			second_set = true; mutated = true;
		} else if ((ft == MGL_LITERAL || ft == MGL_SHORT_REP) && (st == MGL_MATCH || st == MGL_LONG_REP)) {
			uint32_t rep_start = pos - (st == MGL_LONG_REP ? mgl_dist_at(&w.st, sdist) : sdist);
			if (slen < MGL_MAX_MATCH && rep_start > 0 && rep_start <= pos &&
			    win_byte(w.win, pos) == c.data[rep_start - 1]) {
				m_first = mgl_pack(st, sdist, slen + 1);
				journal_set(jn, pos, first, m_first, lane);
				mutated = true;
			}
		}
	}
	if (!mutated) {
		mgl_pk picked;
		if (!pick_from_top_k<1>(c, w, probs, T, lencost, first, false, rng, lane, &picked)) {
			if (lane == 0) { out.cost[j] = MGL_INVALID_COST; out.ndiffs[j] = 0; out.walked[j] = 0; out.win[2u * j] = target; out.win[2u * j + 1u] = MGL_WIN_NONE; }
			return;
		}
		m_first = picked;
		journal_set(jn, pos, first, m_first, lane);
	}
	walk_packet<true>(w, c.L, c.data, probs, T, mgl_pk_type(m_first), mgl_pk_dist(m_first), mgl_pk_len(m_first), lane); /* :169 */

	/* repair_remaining_packets, packet_slab_neighbour.c:82-117 */
	uint32_t count = 0, guard = 0, npicks = 0;
	while (w.st.pos < c.n && !jn.overflow) {
		if (++guard > c.n) break;
		count++;
		const uint32_t p = w.st.pos;
		win_cover(w.win, c, b.slab, w.st.pos, lane);
		const mgl_pk old = (second_set && p == pos + 1) ? m_second : win_pk(w.win, p);
		mgl_pk pk = old;
		uint32_t type = mgl_pk_type(pk);
		if (type == MGL_SHORT_REP || (type == MGL_LITERAL && count < 4)) {
			/* for a LITERAL past the third packet the byte test cannot change anything (:91-97) */
			const bool same = w.st.dists[0] < p && win_byte(w.win, p) == c.data[p - w.st.dists[0] - 1];
			if (same) { if (count < 4) pk = MGL_PK_SHORT_REP; }
			else pk = MGL_PK_LITERAL;
		}
		type = mgl_pk_type(pk);
		if (type == MGL_LONG_REP) {
			const uint32_t len = mgl_pk_len(pk);
			uint32_t idx = mgl_pk_dist(pk);
			bool ok = long_rep_ok(c, w, idx, len, lane);
			for (uint32_t i = 0; i < 4 && !ok; i++) { idx = i; ok = long_rep_ok(c, w, idx, len, lane); }
			pk = mgl_pack(MGL_LONG_REP, idx, len);
			if (!ok) {
				npicks++;
				const bool best = (nbr_draw(rng) % 4u) == 0;
				mgl_pk picked;
				if (pick_from_top_k<1>(c, w, probs, T, lencost, pk, best, rng, lane, &picked)) pk = picked;
			}
		}
		if (pk != old) {
			const mgl_pk base_old = (second_set && p == pos + 1) ? uni64(b.slab[p]) : old;
			journal_set(jn, p, base_old, pk, lane);
		}
		walk_packet<true>(w, c.L, c.data, probs, T, mgl_pk_type(pk), mgl_pk_dist(pk), mgl_pk_len(pk), lane);
	}

	const uint64_t total = base_cum + wave_sum64(w.acc);
	wave_sync();
	if (jn.overflow) {
		if (lane == 0) { out.cost[j] = MGL_INVALID_COST; out.ndiffs[j] = 0; out.walked[j] = w.packets - first_packet; out.win[2u * j] = target; out.win[2u * j + 1u] = MGL_WIN_DROPPED; }
		return;
	}
	const WinInfo wi = window_end_from_journal(c, b.slab, jn, st_target, lane);
	const uint32_t wend = wi.end;
	if (wi.n_ins > 4096u || wi.n_rem > 4096u || wi.walked > MGL_MAX_WALK || npicks > MGL_MAX_REPAIR_PICKS) { /* MGL_BIG_CAP / MGL_MAX_WALK / MGL_MAX_REPAIR_PICKS: what the incremental engine's lists hold, its walk visits, its repair picks */
		if (lane == 0) { out.cost[j] = MGL_INVALID_COST; out.ndiffs[j] = 0; out.walked[j] = w.packets - first_packet; out.win[2u * j] = target; out.win[2u * j + 1u] = MGL_WIN_DROPPED; }
		return;
	}
	/* journal out: entries whose final value equals the base value are dropped */
	uint32_t nd = 0;
	for (uint32_t i = 0; i < jn.count; i++) {
		if (jn.old[i] == jn.neu[i]) continue;
		if (lane == 0) {
			out.dpos[(size_t)j * MGL_MAX_DIFFS + nd] = jn.pos[i];
			out.dold[(size_t)j * MGL_MAX_DIFFS + nd] = jn.old[i];
			out.dnew[(size_t)j * MGL_MAX_DIFFS + nd] = jn.neu[i];
		}
		nd++;
	}
	if (lane == 0) { out.cost[j] = total; out.ndiffs[j] = nd; out.walked[j] = w.packets - first_packet; out.win[2u * j] = target; out.win[2u * j + 1u] = wend; out.win2[j] = wi.soft; }
}

/* todo != nullptr: only the neighbours listed there are evaluated (the ones the incremental kernels could not
 * fit), walking from byte 0 instead of from a prefix checkpoint; the launch is a small grid that strides over
 * the list (the host does not know its length: empty in practice, and then a workgroup costs one load). */
__global__ void __launch_bounds__(256) k_neighbours(DevCtx c, BaseView b, const Control* ctl, uint64_t seed,
                                                    uint64_t step_override, uint32_t K, NbrOut out, uint32_t per_wave_bytes,
                                                    const uint32_t* todo, const uint32_t* todo_count)
{
	const uint32_t waves = blockDim.x >> 6;
	if (todo && blockIdx.x * waves >= *todo_count) return; /* nothing listed for this workgroup: before any load */
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	uint16_t* T = (uint16_t*)smem;
	for (uint32_t i = threadIdx.x; i < 2048; i += blockDim.x) T[i] = c.cost_tbl[i];
	__syncthreads();
	const uint32_t lane = threadIdx.x & 63u, wid = threadIdx.x >> 6;
	if (todo) {
		const uint32_t n = *todo_count;
		for (uint32_t slot = blockIdx.x * waves + wid; slot < n; slot += gridDim.x * waves)
			nbr_fullwalk_one(c, b, ctl, seed, step_override, K, out, per_wave_bytes, true, smem, T, uni(todo[slot]), lane, wid);
	} else {
		nbr_fullwalk_one(c, b, ctl, seed, step_override, K, out, per_wave_bytes, false, smem, T, blockIdx.x * waves + wid, lane, wid);
	}
}

/* main.c:91 -- the new best slab (after the journal has been applied) */
__global__ void k_copy_best(const Control* ctl, const mgl_pk* slab, mgl_pk* best, uint32_t n)
{
	if (!ctl->copy_best_flag) return;
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) best[i] = slab[i];
}

/* ================================================================== hooks & layout */

/* 12-byte reference records (lzma_packet.h:13-17) <-> packed 8-byte entries */
__global__ void k_import(const uint32_t* aos /* 3 dwords per record */, mgl_pk* slab, uint32_t n)
{
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const uint32_t t = aos[3 * i] & 0xFFu, d = aos[3 * i + 1], l = aos[3 * i + 2] & 0xFFFFu;
		slab[i] = mgl_pack(t, d, l);
	}
}
__global__ void k_export(const mgl_pk* slab, uint32_t* aos, uint32_t n)
{
	for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
		const mgl_pk p = slab[i];
		aos[3 * i] = mgl_pk_type(p); aos[3 * i + 1] = mgl_pk_dist(p); aos[3 * i + 2] = mgl_pk_len(p);
	}
}
/* count: one slab, or the parses' several side by side (above 2^32 entries then) */
__global__ void k_fill_literal(mgl_pk* slab, size_t count)
{
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) slab[i] = MGL_PK_LITERAL;
}

/* substring_enumerator_for_each, one thread, reference callback order (parity hook) */
__global__ void k_substrings(DevCtx c, uint32_t pos, uint32_t max_len, uint32_t* offs, uint32_t* lens, uint32_t cap,
                             uint32_t* count)
{
	uint32_t k = 0;
	if (pos != 0 && pos != c.n - 1 && pos < c.n) {
		const uint32_t bg = ((uint32_t)c.data[pos] << 8) | c.data[pos + 1];
		for (uint32_t i = c.bucket_off[bg]; i < c.bucket_off[bg + 1]; i++) {
			const uint32_t q = c.bucket_pos[i];
			if (q >= pos) break;
			if (pos - q - 1 >= c.dict_limit) continue;
			if (k < cap) { offs[k] = q; lens[k] = 2; }
			k++;
			for (uint32_t j = 2; j < max_len && j + pos < c.n; j++) {
				if (c.data[pos + j] != c.data[q + j]) break;
				if (k < cap) { offs[k] = q; lens[k] = j + 1; }
				k++;
			}
		}
	}
	*count = k;
}
