/*
 * mgl_nbr2.h -- what the evaluation of one neighbour (nbr2_one, mgl_kernels2.hip) keeps between its stages, and what it
 * leaves in memory for another launch or another body: the second pass's scratch slots and the change-list helpers that
 * go with them, the launch's arguments (NbrArgs), the neighbour (Nbr) and its window walk (NbrWalk), the continuation
 * record, the fused instance's hand-over (PickHand) and a neighbour's outputs.  Included by mgl_kernels2.hip behind the
 * change lists (Changes) and the journal, which it builds on.
 */
/* BIG = false: the regular launch, change lists in LDS (MGL_CHG_CAP events each).
 * BIG = true: second chance for the few neighbours whose lists overflowed LDS: same code, lists
 * in a per-neighbour global scratch area (big.cap events each); what overflows even that goes
 * to the full-walk kernel. */
struct BigScratch {
	uint16_t* ins_key; uint32_t* ins_pos; uint16_t* rem_key; uint32_t* rem_pos; uint16_t* uctx;
	uint32_t cap, uctx_cap, slots;
	const uint32_t* todo_in; const uint32_t* todo_in_count;
	uint32_t* spill_ctr; /* slots handed out to first-pass wavefronts that had to spill their lists */
	/* re-simulation handed to k_sim (several wavefronts per neighbour): per neighbour a header
	 * {n_ins, n_rem, direct lo, direct hi} (n_ins = ~0: nothing to do) and the two change lists */
	uint32_t chg_cap; /* events per first-pass list (MGL_CHG_CAP, more when a step has few neighbours and LDS to spare) */
	uint4* sim_hdr;
	uint16_t* sim_keys; /* per neighbour: ins_key[chg_cap] | rem_key[chg_cap] */
	uint32_t* sim_pos;  /* per neighbour: ins_pos[chg_cap] | rem_pos[chg_cap] */
	/* continuation records, one per scratch slot (MGL_CONT_WORDS u32 each): a second-half wavefront whose repair needs a top-K pick
	 * saves its walk here (state, journal; its change lists go to the slot's list area) and the second pass resumes it at the
	 * pick instead of evaluating the neighbour again from its target.  nullptr: no continuations (restart, as before) */
	uint32_t* cont;
	uint32_t evcancel; /* the paired site of the window walk leaves events common to both packets out of the lists; 0 (MGL_NO_EVCANCEL=1): packet-level lists */
};
#define MGL_CONT_WORDS 368u       /* the layout: ContWord, below */
#define MGL_CONT_MAGIC 0x434F4E54u
/* empty lists, nothing counted */
__device__ __forceinline__ void changes_reset(Changes& ch)
{
	ch.n_ins = ch.n_rem = 0; ch.n_cancel = 0; ch.direct = 0; ch.overflow = false; ch.list_full = false;
}
/* from here on the lists and the context list are scratch slot `slot`'s, in global memory (what the lists hold does not move:
 * lists_copy_out) */
__device__ __forceinline__ void changes_use_slot(Changes& ch, const BigScratch& big, uint32_t slot)
{
	ch.ins_key = big.ins_key + (size_t)slot * big.cap; ch.ins_pos = big.ins_pos + (size_t)slot * big.cap;
	ch.rem_key = big.rem_key + (size_t)slot * big.cap; ch.rem_pos = big.rem_pos + (size_t)slot * big.cap;
	ch.uctx = big.uctx + (size_t)slot * big.uctx_cap;
	ch.cap = big.cap; ch.uctx_cap = big.uctx_cap;
}
/* one wavefront copies both lists to a global list area: a scratch slot's, or a neighbour's k_sim lists */
__device__ __forceinline__ void lists_copy_out(const Changes& ch, uint16_t* ins_key, uint32_t* ins_pos, uint16_t* rem_key, uint32_t* rem_pos, uint32_t lane)
{
	for (uint32_t i = lane; i < ch.n_ins; i += 64) { ins_key[i] = ch.ins_key[i]; ins_pos[i] = ch.ins_pos[i]; }
	for (uint32_t i = lane; i < ch.n_rem; i += 64) { rem_key[i] = ch.rem_key[i]; rem_pos[i] = ch.rem_pos[i]; }
}
/* ... to scratch slot `slot`'s */
__device__ __forceinline__ void lists_copy_to_slot(const Changes& ch, const BigScratch& big, uint32_t slot, uint32_t lane)
{
	Changes to;
	changes_use_slot(to, big, slot);
	lists_copy_out(ch, to.ins_key, to.ins_pos, to.rem_key, to.rem_pos, lane);
}
/* what the pick body of the fused instance hands to its walk body, in place of `pickstate` and the read of `pickrec`: all
 * wave-uniform, so scalar registers */
struct PickHand {
	uint32_t target, rng_n;      /* rng_n: the RNG position behind the grow/shrink draw, or behind the pick */
	uint32_t ctx_state, dists[4]; /* walk state at the target */
	mgl_pk first, second;        /* the base's packets at the target and behind it (second: only with HAND_SECOND) */
	mgl_pk m_first, m_second;    /* the mutated packet(s): grow/shrink, or the top-K pick */
	uint32_t flags;
};
#define MGL_HAND_MUTATED 1u /* grow/shrink: no pick */
#define MGL_HAND_SECOND 2u  /* ... that rewrote the packet behind the target too */
#define MGL_HAND_OK 4u      /* the top-K pick found a candidate */
/* what is constant for a launch, and the wavefront's place in it: the kernel fills it once.  Four things travel beside it as
 * plain arguments (c, b, lane, T), because the compiler's inter-procedural passes run before the stages are inlined and see
 * through arguments, not through a struct: T reaches pick_from_top_k<1> as a known LDS address, lane with its range, and the two
 * kernel arguments reach model_load as themselves, not as a scratch copy */
struct NbrArgs {
	Control* ctl; uint64_t seed, step_override; uint32_t K; const NbrOut& out; uint32_t per_wave_bytes;
	uint32_t* todo; uint32_t* todo_count; unsigned long long* prof_acc; const BigScratch& big; uint4* pickrec; uint32_t j_base, j_end; uint4* pickstate;
	unsigned char* smem; uint32_t wid;
};
/* what the window walk carries from one packet to the next -- which is what a continuation record stores (cont_save, cont_resume) */
struct NbrWalk {
	mgl_wstate nb, bs;      /* the neighbour's walk state and the base's */
	uint32_t count;         /* repair packet counter of packet_slab_neighbour.c:84-86, saturating */
	uint32_t walked;        /* neighbour packets visited */
	uint32_t npicks;        /* repair picks of this neighbour */
	/* for the bulk step's selection: the first meeting point -- same byte, same ctx_state -- behind the last rep
	 * packet the walk meets, and whether a rep packet of the neighbour reads a distance from before the window */
	uint32_t wsoft, taint, dep;
	uint32_t guard;
	bool first_packet;      /* the next neighbour packet is the mutated one, coded as is */
	bool second_set;        /* the mutation rewrote the packet behind the target too: to m_second */
	mgl_pk m_second;
	/* a repair's top-K pick: the request ... */
	uint32_t pick_pos;
	mgl_pk pick_inc;        /* the incumbent */
	bool pick_best;
	mgl_pk resume_old;      /* the packet the repair found there */
	/* ... and its result, handed back to the walk */
	bool have_pick;
	mgl_pk picked_pk;
};
enum { P_MODEL, P_SIM, P_TOPK, P_WALK, P_OUT };
/* the neighbour a wavefront evaluates, between the stages of nbr2_one */
struct Nbr {
	uint32_t j, slot;        /* its index in the step; its scratch slot (second pass) */
	unsigned long long t_begin;
	uint32_t pos;            /* the target */
	mgl_pk first, m_first;   /* the base's packet there, and the neighbour's */
	bool mutated;            /* m_first is known (grow/shrink, or a resumed walk) */
	bool pick_is_mutation;   /* the pending pick is the mutation's, not a repair's */
	uint32_t* crec; bool resumed;       /* second pass: the slot's continuation record, and whether it holds this neighbour's walk */
	Journal jn; Changes ch; Win win; Prof prof;
	bool spilled;            /* the lists are in a global scratch slot */
	bool too_many;
	uint32_t phase;
	uint32_t sim_limit; bool sim_overlay; /* re-simulation request */
	int64_t delta;
	bool generate_failed, sim_deferred, walk_long;
	uint32_t wend;           /* where the two walks meet again: the end of this neighbour's window */
};

/* ---- continuation record: a second-half wavefront whose repair needs a top-K pick saves its walk in its scratch slot's record,
 * and the second pass takes it up at that pick (BigScratch::cont).  The layout, in u32 words: */
enum ContWord : uint32_t {
	CW_MAGIC = 0,     /* MGL_CONT_MAGIC: the record is live.  Written last; cleared by the wavefront that takes the walk up */
	CW_J = 1,         /* the neighbour */
	CW_TARGET = 2,
	CW_NB = 3, CW_BS = 9, /* mgl_wstate, six words each: pos, ctx_state, dists[4] */
	CW_COUNT = 15, CW_WALKED = 16, CW_NPICKS = 17, CW_WSOFT = 18, CW_TAINT = 19, CW_DEP = 20,
	CW_RNG_N = 21, CW_GUARD = 22, CW_JN_COUNT = 23, CW_N_INS = 24, CW_N_REM = 25,
	CW_FLAGS = 26,    /* CW_F_*; word 27 is free */
	CW_PICK_INC = 28, CW_RESUME_OLD = 30, CW_M_SECOND = 32, CW_DIRECT = 34, /* 64 bits each, low word first */
	CW_N_CANCEL = 36,
	CW_HDR_END = 37,
	CW_JN_POS = 48,   /* the journal, an entry per lane: positions, */
	CW_JN_OLD = 112,  /* old packets (mgl_pk: two words each) */
	CW_JN_NEU = 240,  /* and new packets */
	CW_END = 368
};
#define CW_F_PICK_BEST 1u
#define CW_F_SECOND_SET 2u
static_assert(CW_HDR_END <= CW_JN_POS, "the continuation record's header outgrew its 48 words");
static_assert(MGL_MAX_DIFFS <= 64u, "a continuation record holds a journal entry per lane");
static_assert(CW_JN_OLD == CW_JN_POS + 64u && CW_JN_NEU == CW_JN_OLD + 2u * 64u && CW_END == CW_JN_NEU + 2u * 64u && CW_END == MGL_CONT_WORDS,
              "the continuation record is a header and three journal areas, MGL_CONT_WORDS in all");
__device__ __forceinline__ void cont_put64(uint32_t* rec, uint32_t w, uint64_t v) { rec[w] = (uint32_t)v; rec[w + 1u] = (uint32_t)(v >> 32); }
__device__ __forceinline__ uint64_t cont_get64(const uint32_t* rec, uint32_t w) { return (uint64_t)uni(rec[w]) | ((uint64_t)uni(rec[w + 1u]) << 32); }
__device__ __forceinline__ void cont_put_state(uint32_t* rec, uint32_t w, const mgl_wstate& st)
{
	rec[w] = st.pos; rec[w + 1u] = st.ctx_state; rec[w + 2u] = st.dists[0]; rec[w + 3u] = st.dists[1]; rec[w + 4u] = st.dists[2]; rec[w + 5u] = st.dists[3];
}
__device__ __forceinline__ void cont_get_state(const uint32_t* rec, uint32_t w, mgl_wstate& st)
{
	st.pos = uni(rec[w]); st.ctx_state = uni(rec[w + 1u]);
	st.dists[0] = uni(rec[w + 2u]); st.dists[1] = uni(rec[w + 3u]); st.dists[2] = uni(rec[w + 4u]); st.dists[3] = uni(rec[w + 5u]);
}
/* the walk as it stands at a repair pick (w.pick_* and w.resume_old set), by the whole wavefront; the change lists go to the
 * slot's list area (lists_copy_to_slot) */
__device__ __forceinline__ void cont_save(uint32_t* rec, uint32_t j, uint32_t target, const NbrWalk& w, const NbrRng& rng, const Journal& jn, const Changes& ch, uint32_t lane)
{
	if (lane < jn.count) {
		rec[CW_JN_POS + lane] = jn.pos[lane];
		reinterpret_cast<mgl_pk*>(rec + CW_JN_OLD)[lane] = jn.old[lane];
		reinterpret_cast<mgl_pk*>(rec + CW_JN_NEU)[lane] = jn.neu[lane];
	}
	if (lane == 0) {
		rec[CW_J] = j; rec[CW_TARGET] = target;
		cont_put_state(rec, CW_NB, w.nb);
		cont_put_state(rec, CW_BS, w.bs);
		rec[CW_COUNT] = w.count; rec[CW_WALKED] = w.walked; rec[CW_NPICKS] = w.npicks; rec[CW_WSOFT] = w.wsoft; rec[CW_TAINT] = w.taint; rec[CW_DEP] = w.dep;
		rec[CW_RNG_N] = rng.n; rec[CW_GUARD] = w.guard; rec[CW_JN_COUNT] = jn.count; rec[CW_N_INS] = ch.n_ins; rec[CW_N_REM] = ch.n_rem;
		rec[CW_FLAGS] = (w.pick_best ? CW_F_PICK_BEST : 0u) | (w.second_set ? CW_F_SECOND_SET : 0u);
		cont_put64(rec, CW_PICK_INC, w.pick_inc);
		cont_put64(rec, CW_RESUME_OLD, w.resume_old);
		cont_put64(rec, CW_M_SECOND, w.m_second);
		cont_put64(rec, CW_DIRECT, (uint64_t)ch.direct);
		rec[CW_N_CANCEL] = ch.n_cancel;
		rec[CW_MAGIC] = MGL_CONT_MAGIC; /* the reader is a later launch */
	}
}
/* does the record hold neighbour j's walk? */
__device__ __forceinline__ bool cont_holds(const uint32_t* rec, uint32_t j) { return uni(rec[CW_MAGIC]) == MGL_CONT_MAGIC && uni(rec[CW_J]) == j; }
/* taking it up, first part: the target and the neighbour's state at the pick (what nbr_target leaves) ... */
__device__ __forceinline__ void cont_resume_target(const uint32_t* rec, uint32_t* target, mgl_wstate& nb)
{
	*target = uni(rec[CW_TARGET]);
	cont_get_state(rec, CW_NB, nb);
}
/* ... second part, behind the mutation stage: the rest, in cont_save's order; the journal and the record's release.  The walk goes on
 * at the pick: not at its first packet, and counting events at packet level as it did */
__device__ __forceinline__ void cont_resume(uint32_t* rec, NbrWalk& w, NbrRng& rng, Journal& jn, Changes& ch, uint32_t lane)
{
	cont_get_state(rec, CW_BS, w.bs);
	w.count = uni(rec[CW_COUNT]); w.walked = uni(rec[CW_WALKED]); w.npicks = uni(rec[CW_NPICKS]); w.wsoft = uni(rec[CW_WSOFT]); w.taint = uni(rec[CW_TAINT]); w.dep = uni(rec[CW_DEP]);
	rng.n = uni(rec[CW_RNG_N]); w.guard = uni(rec[CW_GUARD]); jn.count = uni(rec[CW_JN_COUNT]); ch.n_ins = uni(rec[CW_N_INS]); ch.n_rem = uni(rec[CW_N_REM]);
	const uint32_t fl = uni(rec[CW_FLAGS]);
	w.pick_best = (fl & CW_F_PICK_BEST) != 0; w.second_set = (fl & CW_F_SECOND_SET) != 0;
	w.pick_inc = cont_get64(rec, CW_PICK_INC);
	w.resume_old = cont_get64(rec, CW_RESUME_OLD);
	w.m_second = cont_get64(rec, CW_M_SECOND);
	ch.direct = (int64_t)cont_get64(rec, CW_DIRECT);
	ch.n_cancel = uni(rec[CW_N_CANCEL]);
	if (lane < jn.count) {
		jn.pos[lane] = rec[CW_JN_POS + lane];
		jn.old[lane] = reinterpret_cast<const mgl_pk*>(rec + CW_JN_OLD)[lane];
		jn.neu[lane] = reinterpret_cast<const mgl_pk*>(rec + CW_JN_NEU)[lane];
	}
	wave_sync();
	if (lane == 0) rec[CW_MAGIC] = 0u; /* taken */
	w.pick_pos = w.nb.pos;
	w.first_packet = false;
}

/* ---- what the fused instance's pick body hands to its walk body (PickHand), a put/take pair per stage */
/* the target, the state there and the base's packet */
__device__ __forceinline__ void hand_put_target(PickHand* hand, const Nbr& n, const mgl_wstate& nb)
{
	hand->target = n.pos; hand->ctx_state = nb.ctx_state;
	hand->dists[0] = nb.dists[0]; hand->dists[1] = nb.dists[1]; hand->dists[2] = nb.dists[2]; hand->dists[3] = nb.dists[3];
	hand->first = uni64(n.first);
}
__device__ __forceinline__ void hand_take_target(const PickHand* hand, Nbr& n, NbrRng& rng, mgl_wstate& nb)
{
	n.pos = hand->target; rng.n = hand->rng_n; /* the RNG position is the one behind the pick body's last draw */
	nb.pos = n.pos; nb.ctx_state = hand->ctx_state;
	nb.dists[0] = hand->dists[0]; nb.dists[1] = hand->dists[1]; nb.dists[2] = hand->dists[2]; nb.dists[3] = hand->dists[3];
	n.first = hand->first;
}
/* the grow/shrink decision and the packets it read (`second`: behind the target, where it rewrote that one) and made */
__device__ __forceinline__ void hand_put_mutation(PickHand* hand, const Nbr& n, const NbrWalk& w, const NbrRng& rng, mgl_pk second)
{
	hand->second = uni64(second);
	hand->m_first = uni64(n.m_first); hand->m_second = uni64(w.m_second); hand->rng_n = uni(rng.n);
	hand->flags = (n.mutated ? MGL_HAND_MUTATED : 0u) | (w.second_set ? MGL_HAND_SECOND : 0u);
}
__device__ __forceinline__ void hand_take_mutation(const PickHand* hand, Nbr& n, NbrWalk& w, mgl_pk* second)
{
	*second = hand->second;
	n.mutated = (hand->flags & MGL_HAND_MUTATED) != 0; w.second_set = (hand->flags & MGL_HAND_SECOND) != 0;
	n.m_first = n.mutated ? hand->m_first : n.first; w.m_second = n.mutated ? hand->m_second : 0; /* without a grow/shrink, m_first is the pick's: hand_take_pick */
}
/* the top-K pick, as a pick record */
__device__ __forceinline__ void hand_put_pick(PickHand* hand, mgl_pk picked, const NbrRng& rng, bool ok)
{
	hand->m_first = uni64(picked); hand->rng_n = uni(rng.n); if (ok) hand->flags |= MGL_HAND_OK;
}
__device__ __forceinline__ uint4 hand_take_pick(const PickHand* hand)
{
	return make_uint4((uint32_t)hand->m_first, (uint32_t)(hand->m_first >> 32), hand->rng_n, (hand->flags & MGL_HAND_OK) ? 1u : 0u);
}

/* ---- a neighbour's outputs; lane 0 writes */
/* no result: an invalid cost and no journal.  `code`: MGL_WIN_NONE (no candidate, or handed to the next pass) or MGL_WIN_DROPPED */
__device__ __forceinline__ void nbr_out_none(const NbrOut& out, uint32_t j, uint32_t pos, uint32_t walked, uint32_t code)
{
	out.cost[j] = MGL_INVALID_COST; out.ndiffs[j] = 0; out.walked[j] = walked; out.win[2u * j] = pos; out.win[2u * j + 1u] = code;
}
/* a diagnostic stop: no result either, and the stop's value where the packets walked go */
__device__ __forceinline__ void nbr_out_diag(const NbrOut& out, uint32_t j, uint32_t value)
{
	out.cost[j] = MGL_INVALID_COST; out.ndiffs[j] = 0; out.walked[j] = value;
}
/* the result, by the whole wavefront: the journal without the entries the repair set back, cost (unless k_sim writes it), windows
 * and the profile word */
__device__ __forceinline__ void nbr_out_result(const NbrArgs& a, uint32_t lane, const Nbr& n, const NbrWalk& w)
{
	const NbrOut& out = a.out; const Journal& jn = n.jn; const Changes& ch = n.ch;
	const uint32_t j = n.j;
	if (lane == 0 && ch.n_cancel) atomicAdd(a.big.spill_ctr + 3, ch.n_cancel); /* event pairs cancelled in the neighbours this step finished */
	const uint64_t total = (uint64_t)((int64_t)a.ctl->rebuild_cost + n.delta + ch.direct); /* rebuild_cost: exact cost of the base */
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
	if (lane == 0) { if (!n.sim_deferred) out.cost[j] = total; out.ndiffs[j] = nd; out.walked[j] = w.walked; out.win[2u * j] = n.pos; out.win[2u * j + 1u] = n.wend; out.win2[j] = (w.wsoft < n.wend ? w.wsoft : n.wend) | (w.dep << 31); }
	if (a.prof_acc && lane == 0) /* diagnostic: wave lifetime (40 bits) | change events (12 bits) | packets walked (12 bits) */
		a.prof_acc[32 + j] = ((__builtin_readcyclecounter() - n.t_begin) & 0xFFFFFFFFFFull) |
		                     ((unsigned long long)((ch.n_ins + ch.n_rem) & 0xFFFu) << 40) | ((unsigned long long)(w.walked & 0xFFFu) << 52);
}

