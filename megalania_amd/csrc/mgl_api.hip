/*
 * mgl_api.hip -- the C ABI of include/megalania_hip.h over the kernels in mgl_kernels*.hip and their neighbours.
 * A handle's DevOwner (mgl_owner.h) owns its device memory, pinned buffers, events and its three HIP streams (StepQueues);
 * no host thread is created.
 */
#include "mgl_topk.hip"
#include "mgl_kernels.hip"
#include "mgl_kernels2.hip"
#include "mgl_kernels3.hip"
#include "mgl_kernels4.hip"
#include "mgl_kernels5.hip"
#include "mgl_pbuild.hip"
#include "mgl_index.hip"
#include "mgl_matchfinder.hip"
#include "mgl_optimal.hip"
#include "mgl_adaptive.hip"
#include "mgl_props.hip"
#include "mgl_segments.hip"
#include "mgl_segparse.hip"
#include "mgl_costmap.hip"
#include "mgl_costmap_live.hip"
#include "mgl_crossover.hip"
#include "mgl_weights.hip"
#include "../../include/megalania_hip.h"
#include "mgl_owner.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

static const uint16_t k_cost_table[2048] = {
#include "mgl_cost_table.inc"
};

#define MGL_MAX_INPUT 176000000ull
static thread_local std::string g_err;
static int fail(int code, const std::string& msg)
{
	g_err = msg;
	return code;
}
#define HIPCHK(expr)                                                                         \
	do {                                                                                     \
		hipError_t e_ = (expr);                                                              \
		if (e_ != hipSuccess)                                                                \
			return fail(MGL_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));     \
	} while (0)

#define TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0) /* an MGL_* code other than MGL_OK goes up */
/* `bytes` of device memory from `own` at *ptr, every byte `fill` (-1: as it comes).  An allocation that does not fit is an
 * MGL_EDEVICE error like any other failed runtime call -- or, for a caller that names `nomem`, MGL_ENOMEM with that message,
 * and no error is left behind for the next launch check */
static int dalloc(DevOwner& own, void** ptr, size_t bytes, int fill = -1, const char* nomem = nullptr)
{
	const hipError_t e = own.device(ptr, bytes);
	if (e != hipSuccess && nomem) {
		(void)hipGetLastError();
		return fail(MGL_ENOMEM, nomem);
	}
	if (e != hipSuccess) return fail(MGL_EDEVICE, std::string("hipMalloc: ") + hipGetErrorString(e));
	if (fill >= 0) HIPCHK(hipMemset(*ptr, fill, bytes));
	return MGL_OK;
}
/* the same for `count` elements of the pointer's type */
template <class T>
static int dnew(DevOwner& own, T*& ptr, size_t count, int fill = -1, const char* nomem = nullptr)
{
	return dalloc(own, (void**)&ptr, sizeof(T) * count, fill, nomem);
}

extern "C" const char* mgl_version(void) { return "megalania-hip 0.1 (gfx950)"; }
extern "C" const char* mgl_last_error(void) { return g_err.c_str(); }
extern "C" int mgl_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}
extern "C" uint32_t mgl_rng_draw_at(uint64_t seed, uint64_t step, uint32_t j, uint32_t n)
{
	return mgl_rng_draw(mgl_rng_key(seed, step, j), n);
}

struct BaseMem {
	BaseView v;
	Control* ctl;
};

/* the match index (mgl_index.hip) as the host builds it; DevCtx holds const views of the same arrays (fill_ctx_index) */
struct MatchIndex {
	uint32_t *bucket_off = nullptr, *bucket_pos = nullptr, *quad_pos = nullptr;
	uint16_t *bucket_nx = nullptr, *quad_nx = nullptr;
	/* exact-length orders D = 2..7; xpos[0] and xpos[2] alias bucket_pos / quad_pos, D = 2 has no rank / run */
	uint32_t *xpos[6] = {}, *xrank[6] = {}, *xrun[6] = {};
	uint8_t* xnxb[6] = {};
	uint32_t *oct_pos = nullptr, *oct_rank = nullptr, *oct_run = nullptr;
	uint32_t *hex_pos = nullptr, *hex_rank = nullptr, *hex_run = nullptr;
	uint64_t *oct_nx8 = nullptr, *hex_nx8 = nullptr;
};

/* The MGL_* environment variables a handle honours, read once per handle at the top of create_impl (read_env) and nowhere
 * else: the creation stages read this.  (MGL_TRACE and MGL_PROF_BIG are the process's, MGL_COMM_TIMEOUT_S is the exchange's.) */
struct EnvSwitches {
	uint32_t halves;          /* MGL_HALVES: slices of a step's neighbours, 1..8 (any other value: 1); unset: 2 above 1 MiB of input, else 1 */
	uint32_t sb_shift;        /* MGL_SB_SHIFT: log2 of the builder's block, 8..10 (any other value is ignored); 0 = the size rule of create_engine */
	bool no_incremental_apply; /* MGL_NO_INCREMENTAL_APPLY: single steps rebuild the base instead of patching it (and no batch accept) */
	bool no_batch;            /* MGL_NO_BATCH: bulk steps always rebuild */
	bool no_evcancel;         /* MGL_NO_EVCANCEL: the window walk lists all events of a re-coded packet, not the changed ones only */
	bool no_split;            /* MGL_NO_SPLIT: the one-kernel form only */
	bool no_cont;             /* MGL_NO_CONT: no continuation records between the second half and the second pass */
	bool no_fuse;             /* MGL_NO_FUSE: pick and walk of a slice as two launches */
	uint32_t simw;            /* MGL_SIMW: wavefronts per neighbour of k_sim, 1, 2, 4 or 8 (any other value is ignored); 0 = MGL_SIM_WAVES */
	bool no_adapt;            /* MGL_NO_ADAPT: the split form stays, whatever the device recommends */
	uint32_t pick_waves;      /* MGL_PICK_WAVES: wavefronts per workgroup of the pick half, 1, 2, 4 or 8; 0 (unset, any other value) = the rule of set_launch_geometry */
	bool no_order;            /* MGL_NO_ORDER: the fused launch takes its neighbours in blockIdx order */
	uint32_t bulk_threshold;  /* MGL_BULK_THRESHOLD: improving neighbours per step above which a bulk step pays, at least 1 (0 is read as 1); 0 = unset: the rule of create_targets */
};
/* the three streams of a handle and the events that order a step's kernels across them */
struct StepQueues {
	hipStream_t stream = nullptr;  /* the main stream: everything that is not named below */
	hipStream_t stream2 = nullptr; /* second half of a step's neighbours: its kernels fill the other half's tails */
	hipStream_t stream3 = nullptr; /* the re-simulation kernels of the split form: beside the second pass, which only needs the walks */
	hipEvent_t ev_fork = nullptr, ev_join = nullptr;
	hipEvent_t ev_tgt = nullptr, ev_tgt_go = nullptr; /* the next step's targets worked out beside the rest of this step's accept (launch_targets_ahead) */
	hipEvent_t ev_rest[8] = {}, ev_sim = nullptr;
	hipEvent_t ev_val = nullptr;   /* a bulk step's validation beside its build */
	hipEvent_t ev_bstat = nullptr; /* behind the read-back copy of the batch accept's status words */
};
/* the next step's targets, made ahead on the second stream: none queued / queued and good for the next launch_neighbours /
 * queued but the base went another way: to be made again */
enum TgtAhead { TGT_NONE, TGT_READY, TGT_STALE };
/* MGL_ACCEPT_AUTO's state: it switches between single and bulk steps block by block */
struct AutoAccept {
	bool bulk_now = true;          /* what the next block of steps runs as */
	uint64_t bulk_hold = 0;        /* single steps left before bulk steps are tried again (their windows were too long) */
	uint64_t blk_done = 0;         /* steps of the current block already run (a block carries over from one mgl_sa_run call to the next) */
	uint64_t blk_imp0 = 0, blk_acc0 = 0; /* the device's improving / accepted counters when the current block began */
	bool select_small = false;    /* the previous bulk step had few acceptable neighbours: this one's selection runs as one launch */
	/* MGL_ACCEPT_AUTO starts over: a fresh block, bulk steps first (a new slab says nothing about the old one's windows) */
	void reset() { bulk_now = true; bulk_hold = 0; blk_done = 0; select_small = false; }
	void decide(bool was_bulk, uint64_t block, uint64_t improving, uint64_t taken, uint32_t bulk_threshold, bool batch_ok);
};
/* the form the regular neighbour launch runs as */
struct LaunchForm {
	bool split_nbr, adaptive; /* adaptive: the device recommends the split or the one-kernel form, the host adopts it block by block */
	bool fuse;                /* the two halves as one launch (k_neighbours2<false, MGL_NBR_PICKWALK>); MGL_NO_FUSE=1: two launches */
	bool form_single = false; /* the form the regular launch runs as right now */
	uint32_t short_looks = 0; /* blocks of at most four steps still to come after a switch of the launch form */
};
/* mgl_sa_set_live_weights: the target weights made again from the live cost map (mgl_costmap_live.hip) inside mgl_sa_run.
 * cfg.every == 0: off.  d_mark, d_sums: the refresh's own buffers beside the weights' three, the handle's while live weights are on */
struct LiveWeights {
	mgl_live_weights_config cfg = {};
	mgl_live_weights_stats stats = {};
	bool stale = false;            /* enabled, or the current slab replaced from outside a run, since the last refresh */
	bool skip = false;             /* the last refresh's weights sum to 2^44 or more: launch_targets ignores them until the next one */
	uint32_t* d_mark = nullptr;
	CostMapSums* d_sums = nullptr;
	hipEvent_t t0 = nullptr, t1 = nullptr;
};
/* diagnostic hooks of the tests (mgl_debug_set) */
struct TestHooks {
	uint32_t xo_nomem = 0;   /* key 8: the next so many crossovers find no room for their buffers */
	uint32_t cm_nomem = 0;   /* key 10: the next so many cost maps find no room for theirs */
	uint32_t batch_fail = 0; /* key 5: the next so many batch accepts give up behind their commit */
	uint32_t batch_late = 0; /* ... 0: before any chain is touched; n: once the n-th touched context has rewritten its chain's descriptors */
	uint32_t rollbacks = 0;  /* key 3: treat the next so many bulk steps that took moves as failed validations */
};
/* MGL_F_TIMING brackets steps with events: every step of a short run, every fourth of a longer one (the ten event records of a
 * timed step cost it 30 us at 10 MB), at most 512 of them.  A timed step has four slots on the main stream and, in the split
 * form, two per slice for the k_sim launches of its first two slices on the stream they run on (the re-simulation kernel
 * measured on its own: it is the path's dominant kernel).  The events are the handle's, made on demand (pool_event). */
enum TimedSlot { T_NBR_BEGIN, T_NBR_END, T_ACCEPT_BEGIN, T_ACCEPT_END, T_SIM_BEGIN, T_SIM_END };
struct StepTimer {
	hipEvent_t ev_begin = nullptr, ev_end = nullptr; /* around the whole run */
	std::vector<hipEvent_t> ev_pool, ev_sim_pool;    /* four per timed step each: the slots above / begin and end of slices 0 and 1 */
	uint64_t stride = 1, timed = 0;  /* of the current run: every stride-th step is timed, `timed` of them in all */
	int64_t step = -1;               /* >= 0: the current step's place among the timed ones */
	bool sim = false;                /* ... and its k_sim launches are bracketed too (the split form runs) */
	std::vector<uint8_t> sim_timed;  /* per timed step: how many of the regular k_sim launches carry events (0: none, the one-kernel form ran) */
};

struct mgl_sa {
	DevOwner own;            /* every device buffer, pinned buffer, event and stream of the handle: released when the handle is deleted */
	int device;
	EnvSwitches env;
	StepQueues q;
	TgtAhead tgt_ahead = TGT_NONE;
	uint32_t halves;
	uint32_t n;
	mgl_properties props;
	mgl_sa_config cfg;
	uint64_t temperature = 0; /* mgl_sa_set_temperature: 0 = the reference's accept rule */
	DevCtx ctx;
	uint8_t* d_data;
	MatchIndex ix;
	uint16_t* d_cost_tbl;
	BaseMem base, scratch;
	mgl_pk* d_best;
	NbrOut nbr;
	uint32_t* d_aos;
	uint64_t* d_cum;
	uint16_t* d_final_probs;
	mgl_pk* d_topk_pk;
	uint64_t* d_topk_cost;
	uint32_t* d_small; /* [0] count */
	uint32_t* d_sub_offs;
	uint32_t* d_sub_lens;
	uint32_t sub_cap;
	uint64_t sqrt_thresh;
	uint32_t per_wave_bytes, waves_per_block, nbr_lds, walk_lds;
	/* incremental path (mgl_kernels2.hip) */
	bool incremental;
	Base2 b2;
	unsigned long long* d_prof; /* only with MGL_F_PROFILE: 32 u64 per-phase cycles + counts | K second-half lifetimes | 32 pick stages | K pick lifetimes */
	uint32_t* d_todo;       /* [0] = count, [1..K] = neighbour indices for the full-walk fallback */
	uint32_t per_wave2, waves_per_block2, nbr2_lds, build_lds;
	uint32_t big_waves = MGL_BIG_WAVES; /* wavefronts of a second-pass workgroup (mgl_debug_set key 7 lowers it for tests) */
	uint32_t probe_form = 0;            /* the form of the top-K search mgl_top_k probes (MGL_KEY_PROBE_FORM) */
	uint32_t chg_cap = MGL_CHG_CAP; /* events per first-pass list */
	uint32_t per_wave_pick, per_wave_rest, pick_waves; /* LDS per wavefront of the two halves of the split launch */
	uint32_t fused_lds;     /* its dynamic LDS: one wavefront, the larger of the two halves' areas */
	size_t b2_bytes;
	BigScratch big;
	uint32_t* d_todo2;
	uint4* d_pickstate;     /* 2 K: target, RNG position and walk state at the target (first half -> second half) */
	uint4* d_pickrec;       /* K: picked packet, RNG position, ok flag (first half -> second half of the neighbour evaluation) */
	LaunchForm form;
	StepCounts* d_counts;   /* [0] live, [1] the last finished step's */
	ApplyBuf ab;
	uint32_t apply_blocks;
	bool incremental_apply;
	/* copies of the base structures of the all-literal slab and of the best slab (main.c:71-77) */
	bool snapshots;
	Base2 snap_lit, snap_best;
	SnapMeta* d_snap_meta; /* [0] literal, [1] best */
	bool parallel_build;
	PBuild pb;
	StepTimer timer;
	/* the step's decision: single (one winner, incremental accept) or bulk (every window-best acceptable
	 * neighbour, parallel rebuild); MGL_ACCEPT_AUTO switches between them block by block */
	int accept_mode = MGL_ACCEPT_AUTO;
	uint32_t bulk_threshold = 0;   /* improving neighbours per step above which a bulk step pays */
	AutoAccept autoacc;
	BulkBuf bulk;
	BatchBuf batch;               /* a bulk step that took few moves patches the base instead of rebuilding it (mgl_kernels5.hip) */
	bool batch_ok = false;
	uint32_t* d_strat_tgt = nullptr;
	uint32_t* d_strat_pre = nullptr; /* stratified targets: packets before every block of 4 096 positions */
	uint32_t focus_lo = 0, focus_hi = 0; /* mgl_sa_set_focus: the targets' byte window, hi = 0: none; handed to k_targets by every launch */
	uint32_t* d_focus_cnt = nullptr; /* two words for mgl_sa_focus: first ordinal, packets */
	/* mgl_sa_set_target_weights / mgl_sa_weight_targets_by_cost (mgl_weights.hip): n weights, their cell prefixes (cells + 1), and the
	 * block totals of the scan with two words behind them for S[lo] and W.  All null: no weights.  wt_slo, wt_window: S[lo] and W of
	 * the focus window in force, read back whenever weights or window change; handed to k_targets_weighted by every launch */
	uint32_t* d_wt = nullptr;
	uint64_t* d_wt_pre = nullptr;
	uint64_t* d_wt_blk = nullptr;
	uint64_t wt_total = 0, wt_slo = 0, wt_window = 0;
	bool wt_apply = true;          /* false only while a run's bulk-route steps pass under MGL_LW_SINGLE_ONLY: launch_targets then ignores the weights */
	LiveWeights live;
	/* made with the targets (launch_targets), for the fused launch: K bytes, 1 = the neighbour will pick, 0 = grow/shrink; and
	 * K neighbour indices, every slice's picking neighbours in front of its others (k_pick_order).  Null: MGL_NO_ORDER=1,
	 * position targets, no split form */
	unsigned char* d_pick_hint = nullptr;
	uint32_t* d_pick_order = nullptr;
	BatchHdr* h_bstat = nullptr;   /* pinned: the batch accept's status words, read back once per bulk step */
	TestHooks force;
	AcceptLimits lim, lim_max;     /* what the in-place accepts compare against (mgl_debug_set key 6 lowers them) and the compiled / allocated values */
	uint64_t batch_early_giveups = 0; /* bulk steps that began a batch accept and left it before anything was touched (clusters or a walk gave up) */
	uint64_t batch_accepts = 0, batch_fallbacks = 0; /* bulk steps whose moves were patched in / that went to the rebuild although a batch accept began */
	std::vector<uint8_t> mode_log; /* per step of the last mgl_sa_run: 0 single, 1 bulk */
	uint64_t bulk_rollbacks = 0;   /* bulk steps whose combined parse failed validation and was taken back (never seen) */
	bool best_unverified = false;  /* packets_best came from another chain: checked when an epoch starts from it */
	uint32_t sim_waves = MGL_SIM_WAVES; /* wavefronts per neighbour in the regular re-simulation launch (MGL_SIMW: 1, 2, 4, 8) */
	bool count_traffic = false;     /* mgl_debug_set key 4: count the bytes of chain data the re-simulation kernel reads */
	unsigned long long* d_traffic = nullptr; /* [0] bytes [1] spare */
	/* the parses' match finder (mgl_sa_set_match_finder) and the lists of mgl_matchfinder.hip: made on first use, kept with
	 * the depth they were made at, made again when another depth is asked for */
	int mf_finder = MGL_MF_NEAREST;
	uint32_t mf_depth = MGL_MF_DEF_DEPTH;
	uint32_t mf_built = 0;         /* depth of the lists held, 0 = none */
	uint32_t* d_mf_off = nullptr;
	uint32_t* d_mf_src = nullptr;
	uint16_t* d_mf_len = nullptr;
	size_t mf_total = 0;
	double mf_ms = 0;              /* device time of the build that made them */
};

static uint64_t ceil_sqrt_u64(uint64_t x)
{
	uint64_t r = (uint64_t)sqrt((double)x);
	while (r * r > x) r--;
	while ((r + 1) * (r + 1) <= x) r++;
	return r * r == x ? r : r + 1;
}

static int alloc_base(DevOwner& own, BaseMem& b, uint32_t n, uint32_t ckpt_elems)
{
	memset(&b, 0, sizeof b);
	b.v.nckpt = (n + (1u << MGL_CKPT_SHIFT) - 1u) >> MGL_CKPT_SHIFT;
	b.v.ckpt_elems = ckpt_elems;
	TRY(dnew(own, b.v.slab, n));
	TRY(dnew(own, b.v.onwalk, ((size_t)n + 63) / 64 + 1, 0));
	TRY(dnew(own, b.v.ckpt_probs, (size_t)b.v.nckpt * ckpt_elems));
	TRY(dnew(own, b.v.ckpt_hdr, b.v.nckpt));
	return dnew(own, b.ctl, 1, 0);
}

/* One device array of a Base2: where its pointer lives, its bytes, the element size if it is one of the two chain pool arrays
 * (4 ch_pos, 2 ch_ev, else 0: a snapshot copies a pool array up to the pool's top only), the byte a fresh base fills it with
 * (-1: none), and what it adds to the total alloc_b2 reports (the pool arrays without their 256 entries of slack, the small
 * arrays nothing). */
struct B2Array {
	void** ptr;
	size_t bytes;
	uint32_t pool_elem;
	int fill;
	size_t counted;
};
#define MGL_B2_ARRAYS 14u
static_assert(MGL_B2_ARRAYS <= MGL_SNAP_SEGS, "a snapshot's plan holds a segment per array");
/* the arrays of `b` for an input of n bytes, in the order of a snapshot's segments */
static void b2_arrays(Base2& b, size_t n, B2Array a[MGL_B2_ARRAYS])
{
	const size_t pool = (size_t)b.pool_cap + 256, ck = sizeof(uint32_t) * b.ck_elems, sb = sizeof(uint32_t) * (size_t)b.ck_elems * b.sb_stride;
	uint32_t k = 0;
	a[k++] = { (void**)&b.slab, sizeof(mgl_pk) * n, 0, -1, sizeof(mgl_pk) * n };
	a[k++] = { (void**)&b.onwalk, sizeof(uint64_t) * ((n + 63) / 64 + 1), 0, -1, 0 };
	a[k++] = { (void**)&b.sp0, sizeof(uint64_t) * (b.nw0 + 64), 0, 0, sizeof(uint64_t) * (b.nw0 + 64) };
	a[k++] = { (void**)&b.sp1, sizeof(uint64_t) * (b.nw1 + 64), 0, 0, 0 };
	a[k++] = { (void**)&b.sp2, sizeof(uint64_t) * (b.nw2 + 64), 0, 0, 0 };
	a[k++] = { (void**)&b.sp_state, sizeof(uint32_t) * 8 * n, 0, -1, sizeof(uint32_t) * 8 * n };
	a[k++] = { (void**)&b.ck_probs, sizeof(uint16_t) * (size_t)b.nck * b.ck_elems, 0, -1, sizeof(uint16_t) * (size_t)b.nck * b.ck_elems };
	a[k++] = { (void**)&b.ch_off, ck, 0, -1, 0 };
	a[k++] = { (void**)&b.ch_len, ck, 0, -1, 0 };
	a[k++] = { (void**)&b.ch_cap, ck, 0, -1, 0 };
	a[k++] = { (void**)&b.ch_pos, sizeof(uint32_t) * pool, 4, 0xFF, sizeof(uint32_t) * (size_t)b.pool_cap };
	a[k++] = { (void**)&b.ch_ev, sizeof(uint16_t) * pool, 2, 0, sizeof(uint16_t) * (size_t)b.pool_cap };
	a[k++] = { (void**)&b.pool_top, sizeof(uint32_t), 0, -1, 0 };
	a[k++] = { (void**)&b.ch_sb, sb, 0, 0, sb };
}
/* device arrays of the incremental base, its geometry set; `own_slab`: also the slab and the on-walk bitmap (else they are the
 * caller's); `init`: filled as a fresh base's */
static int alloc_b2(DevOwner& own, Base2& b, size_t n, bool own_slab, bool init, size_t* bytes_out)
{
	B2Array a[MGL_B2_ARRAYS];
	b2_arrays(b, n, a);
	size_t bytes = 0;
	for (uint32_t k = own_slab ? 0u : 2u; k < MGL_B2_ARRAYS; k++) {
		TRY(dalloc(own, a[k].ptr, a[k].bytes, init ? a[k].fill : -1));
		bytes += a[k].counted;
	}
	if (bytes_out) *bytes_out = bytes;
	return MGL_OK;
}
/* dir 0: base -> snapshot, dir 1: snapshot -> base; cond: only if this step found a new best */
static int launch_snapshot(mgl_sa* sa, Base2& snap, uint32_t which, int dir, int cond)
{
	Base2 from = dir == 0 ? sa->b2 : snap, to = dir == 0 ? snap : sa->b2;
	B2Array src[MGL_B2_ARRAYS], dst[MGL_B2_ARRAYS];
	b2_arrays(from, sa->n, src);
	b2_arrays(to, sa->n, dst);
	SnapPlan p;
	memset(&p, 0, sizeof p);
	for (uint32_t k = 0; k < MGL_B2_ARRAYS; k++) {
		p.seg[k].src = *src[k].ptr; p.seg[k].dst = *dst[k].ptr; p.seg[k].bytes = src[k].bytes; p.seg[k].pool_elem = src[k].pool_elem;
	}
	p.nseg = MGL_B2_ARRAYS;
	p.src_pool_top = from.pool_top;
	hipLaunchKernelGGL(k_snapshot, dim3(2048), dim3(256), 0, sa->q.stream, p, sa->base.ctl, sa->d_snap_meta + which, dir, cond);
	HIPCHK(hipGetLastError());
	return MGL_OK;
}

static int launch_rebuild(mgl_sa* sa, BaseMem& b, int from_dirty, uint64_t* cum, uint16_t* final_probs)
{
	hipLaunchKernelGGL(k_rebuild, dim3(1), dim3(64), sa->walk_lds, sa->q.stream, sa->ctx, b.v, b.ctl, from_dirty, cum, final_probs);
	HIPCHK(hipGetLastError());
	return MGL_OK;
}
/* the base structures of the slab from scratch, block-parallel (mgl_pbuild.hip) */
static int launch_pbuild(mgl_sa* sa, bool validate_beside = false)
{
	const DevCtx& c = sa->ctx;
	Base2& b = sa->b2;
	PBuild& pb = sa->pb;
	Control* ctl = sa->base.ctl;
	hipStream_t st = sa->q.stream;
	const uint32_t total = c.L.total;
	hipLaunchKernelGGL(pb_exits, dim3(pb.nblk), dim3(320), 0, st, c, b, pb);
	hipLaunchKernelGGL(pb_entries_group, dim3(pb.ngrp), dim3(320), MGL_PB_GROUP * MGL_PB_ENTRIES * 2u, st, pb);
	hipLaunchKernelGGL(pb_entries, dim3(1), dim3(64), 0, st, c, pb);
	hipLaunchKernelGGL(pb_entries_fill, dim3(pb.ngrp), dim3(64), 0, st, pb);
	hipLaunchKernelGGL(pb_mark, dim3(pb.nblk), dim3(64), 0, st, c, b, pb, ctl);
	{
		const uint32_t nch = (pb.nblk + MGL_PB_SCAN_CHUNK - 1u) / MGL_PB_SCAN_CHUNK;
		hipLaunchKernelGGL(pb_scan_chunks, dim3((nch + 255u) / 256u), dim3(256), 0, st, pb);
		hipLaunchKernelGGL(pb_scan, dim3(1), dim3(64), 0, st, pb);
		hipLaunchKernelGGL(pb_scan_fill, dim3((nch + 255u) / 256u), dim3(256), 0, st, pb);
	}
	hipLaunchKernelGGL(pb_levels, dim3((b.nw0 + 255) / 256), dim3(256), 0, st, (const uint64_t*)b.sp0, b.sp1, b.nw0, b.nw1);
	hipLaunchKernelGGL(pb_levels, dim3((b.nw1 + 255) / 256), dim3(256), 0, st, (const uint64_t*)b.sp1, b.sp2, b.nw1, b.nw2);
	hipLaunchKernelGGL(pb_walk, dim3(pb.nblk), dim3(64), b.ck_elems * 4u, st, c, b, pb);
	if (validate_beside) {
		/* a bulk step's check of the new parse (every packet against the input) needs the bitmaps and the special-state
		 * records, which exist from here on: it runs on the second stream beside the rest of the build */
		HIPCHK(hipEventRecord(sa->q.ev_fork, st));
		HIPCHK(hipStreamWaitEvent(sa->q.stream2, sa->q.ev_fork, 0));
		hipLaunchKernelGGL(k_validate, dim3((sa->ctx.n + 255u) / 256u), dim3(256), 0, sa->q.stream2, sa->ctx, sa->b2, sa->base.ctl);
		HIPCHK(hipEventRecord(sa->q.ev_val, sa->q.stream2));
	}
	{
		const uint32_t og = (pb.nblk + MGL_PB_OFF_ROWS - 1u) / MGL_PB_OFF_ROWS;
		hipLaunchKernelGGL(pb_offsets_sum, dim3((b.ck_elems + 255) / 256, og), dim3(256), 0, st, b, pb);
		hipLaunchKernelGGL(pb_offsets_top, dim3((b.ck_elems + 255) / 256), dim3(256), 0, st, b, pb, total, og);
		hipLaunchKernelGGL(pb_offsets, dim3((b.ck_elems + 255) / 256, og), dim3(256), 0, st, b, pb, total);
		hipLaunchKernelGGL(pb_index, dim3((total + 31u) / 32u, (pb.nblk + 1u + 31u) / 32u), dim3(256), 0, st, b, pb, total);
	}
	hipLaunchKernelGGL(pb_layout, dim3(1), dim3(64), 0, st, b, pb, ctl, total);
	hipLaunchKernelGGL(pb_scatter, dim3(pb.nblk), dim3(256), b.ck_elems * 4u, st, b, pb, total);
	hipLaunchKernelGGL(pb_sim, dim3((pb.seg_cap + 63) / 64), dim3(64), 0, st, c, b, pb);
	hipLaunchKernelGGL(pb_sim_fix, dim3((total + 63) / 64), dim3(64), 0, st, c, b, pb);
	hipLaunchKernelGGL(pb_ckpt, dim3((b.ck_elems + 63) / 64, (b.nck + MGL_PB_CK_ROWS - 1) / MGL_PB_CK_ROWS), dim3(64), 0, st, c, b);
	hipLaunchKernelGGL(pb_finish, dim3(1), dim3(64), 0, st, pb, ctl);
	if (validate_beside) HIPCHK(hipStreamWaitEvent(st, sa->q.ev_val, 0));
	HIPCHK(hipGetLastError());
	return MGL_OK;
}
static int rebuild_base(mgl_sa* sa, int after_accept)
{
	if (!sa->incremental) return launch_rebuild(sa, sa->base, after_accept, nullptr, nullptr);
	if (sa->parallel_build && !after_accept) return launch_pbuild(sa);
	hipLaunchKernelGGL(k_build, dim3(1), dim3(64), sa->build_lds, sa->q.stream, sa->ctx, sa->b2, sa->base.ctl, after_accept);
	HIPCHK(hipGetLastError());
	return MGL_OK;
}
/* every packet on the current base's walk reproduces the input (incremental engine: needs the special-state records) */
static int launch_validate(mgl_sa* sa)
{
	if (!sa->incremental) return MGL_OK;
	hipLaunchKernelGGL(k_validate, dim3((sa->ctx.n + 255u) / 256u), dim3(256), 0, sa->q.stream, sa->ctx, sa->b2, sa->base.ctl);
	HIPCHK(hipGetLastError());
	return MGL_OK;
}
/* the structs the accept kernels get: the handle's, with the capacities a test may have lowered (mgl_debug_set key 6) */
static Base2 accept_b2(const mgl_sa* sa) { Base2 b = sa->b2; b.pool_cap = sa->lim.v[MGL_LIM_POOL]; return b; }
static ApplyBuf accept_ab(const mgl_sa* sa)
{
	ApplyBuf ab = sa->ab;
	ab.job_cap = sa->lim.v[MGL_LIM_JOBS]; ab.span_cap = sa->lim.v[MGL_LIM_SPAN_AREA]; ab.scratch_cap = sa->lim.v[MGL_LIM_SCRATCH];
	return ab;
}
static BatchBuf accept_bt(const mgl_sa* sa) { BatchBuf bt = sa->batch; bt.runs_cap = sa->lim.v[MGL_LIM_BATCH_RUNS]; return bt; }
static void accept_limits_init(mgl_sa* sa, uint32_t* why)
{
	AcceptLimits& m = sa->lim_max;
	memset(&m, 0, sizeof m);
	m.v[MGL_LIM_APPLY_EVENTS] = MGL_APPLY_CAP; m.v[MGL_LIM_APPLY_GUARD] = 1u << 20; m.v[MGL_LIM_APPLY_SUB] = MGL_SUB_CAP;
	m.v[MGL_LIM_APPLY_SPAN] = MGL_SPAN_CAP; m.v[MGL_LIM_APPLY_PIECES] = MGL_PIECE_CAP; m.v[MGL_LIM_APPLY_SHIFT] = MGL_SUB_CAP;
	m.v[MGL_LIM_POOL] = sa->b2.pool_cap; m.v[MGL_LIM_JOBS] = sa->ab.job_cap; m.v[MGL_LIM_SPAN_AREA] = sa->ab.span_cap;
	m.v[MGL_LIM_SCRATCH] = sa->ab.scratch_cap;
	m.v[MGL_LIM_BATCH_JOURNAL] = MGL_BATCH_JCAP; m.v[MGL_LIM_BATCH_EVENTS] = MGL_BATCH_EVCAP; m.v[MGL_LIM_BATCH_OPS] = MGL_BATCH_OPCAP;
	m.v[MGL_LIM_BATCH_GUARD] = 1u << 18; m.v[MGL_LIM_BATCH_SUB] = MGL_BATCH_SUB; m.v[MGL_LIM_BATCH_SHIFT] = 2047u;
	m.v[MGL_LIM_BATCH_RUNS] = sa->batch.runs_cap; m.v[MGL_LIM_SOFT_REACH] = 1u;
	m.why = why;
	sa->lim = m;
	sa->lim.v[MGL_LIM_SOFT_REACH] = 0u;
}
/* incremental engine, after k_decide: fold the winner into the base structures */
static int launch_targets_ahead(mgl_sa* sa, uint64_t next_gstep);
static int launch_apply(mgl_sa* sa, uint64_t next_gstep = ~0ull)
{
	/* the base is about to leave the best slab it still holds: keep a copy first (lazy: while every
	 * accepted step is a new best no copy is ever taken) */
	if (sa->snapshots) TRY(launch_snapshot(sa, sa->snap_best, 1, 0, 2));
	hipLaunchKernelGGL(k_apply_walk, dim3(1), dim3(64), 0, sa->q.stream, sa->ctx, sa->b2, sa->base.ctl, sa->nbr, sa->ab, sa->lim);
	if (next_gstep != ~0ull) TRY(launch_targets_ahead(sa, next_gstep)); /* the bitmap is final from here on */
	if (!sa->snapshots)
		hipLaunchKernelGGL(k_copy_best, dim3(256), dim3(256), 0, sa->q.stream, (const Control*)sa->base.ctl,
		                   (const mgl_pk*)sa->base.v.slab, sa->d_best, sa->ctx.n);
	hipLaunchKernelGGL(k_apply_chains, dim3(sa->apply_blocks), dim3(MGL_APPLY_THREADS), 0, sa->q.stream, sa->ctx, accept_b2(sa), sa->base.ctl, accept_ab(sa), sa->lim);
	hipLaunchKernelGGL(k_apply_jobs, dim3(1024), dim3(256), 0, sa->q.stream, sa->b2, (const Control*)sa->base.ctl, sa->ab, 0, (const BatchHdr*)nullptr);
	hipLaunchKernelGGL(k_apply_jobs, dim3(1024), dim3(256), 0, sa->q.stream, sa->b2, (const Control*)sa->base.ctl, sa->ab, 1, (const BatchHdr*)nullptr);
	hipLaunchKernelGGL(k_build_end, dim3(1), dim3(64), sa->build_lds, sa->q.stream, sa->ctx, sa->b2, sa->base.ctl, sa->snapshots ? 1 : 0, sa->d_counts, sa->form.adaptive ? 1 : 0, sa->form.form_single ? 1 : 0);
	HIPCHK(hipGetLastError());
	return MGL_OK;
}
/* diagnostic switches of the launch path, read once.  MGL_TRACE=1: name every launch of the neighbour evaluation on stderr and wait
 * for the device after it, so that a faulting kernel is the last one named */
static const bool g_trace = getenv("MGL_TRACE") != nullptr, g_prof_big = getenv("MGL_PROF_BIG") != nullptr;
#define NBR_TRACE(name) do { if (g_trace) { fprintf(stderr, "[mgl] %s\n", name); hipError_t e_ = hipDeviceSynchronize(); if (e_ != hipSuccess) fprintf(stderr, "[mgl] %s -> %s\n", name, hipGetErrorString(e_)); } } while (0)
/* event i of a pool that grows on demand; the events are the handle's */
static hipEvent_t pool_event(mgl_sa* sa, std::vector<hipEvent_t>& pool, size_t i)
{
	while (pool.size() <= i) {
		hipEvent_t e = nullptr;
		if (sa->own.event(&e) != hipSuccess) return nullptr;
		pool.push_back(e);
	}
	return pool[i];
}
/* slot `slot` of the current step (slice h's, for the two k_sim slots) on stream st, if the step is a timed one */
static int mark(mgl_sa* sa, TimedSlot slot, hipStream_t st, uint32_t h = 0)
{
	StepTimer& t = sa->timer;
	const bool sim = slot >= T_SIM_BEGIN;
	if (t.step < 0 || (sim && (!t.sim || h >= 2))) return MGL_OK;
	const size_t i = 4 * (size_t)t.step + (sim ? 2 * h + (slot - T_SIM_BEGIN) : slot);
	HIPCHK(hipEventRecord(pool_event(sa, sim ? t.ev_sim_pool : t.ev_pool, i), st));
	return MGL_OK;
}
static uint32_t nbr_slices(const mgl_sa* sa) { return (sa->halves >= 2 && sa->cfg.neighbours_per_step >= 1024) ? sa->halves : 1u; }
/* stratified targets of a step: packets before every block of 4 096 positions of the current walk, their
 * prefix sums, then one wavefront per neighbour turns its ordinal into a position */
static void launch_targets(mgl_sa* sa, hipStream_t st, uint64_t step_override)
{
	const uint32_t K = sa->cfg.neighbours_per_step;
	const uint64_t* onwalk = sa->incremental ? sa->b2.onwalk : sa->base.v.onwalk;
	const uint32_t nw0 = sa->incremental ? sa->b2.nw0 : (sa->ctx.n + 63u) >> 6;
	if (sa->d_wt && sa->wt_window && sa->wt_apply && !sa->live.skip) { /* weights in force and the window weighs something: the weighted rule (mgl_weights.hip), which counts no packets */
		hipLaunchKernelGGL(k_targets_weighted, dim3((K + 3u) / 4u), dim3(256), 0, st, sa->ctx, sa->b2, onwalk, nw0, (const Control*)sa->base.ctl, sa->cfg.seed, step_override, K,
		                   sa->d_strat_tgt, sa->d_pick_hint, sa->focus_lo, sa->focus_hi ? sa->focus_hi : sa->n, (const uint32_t*)sa->d_wt, (const uint64_t*)sa->d_wt_pre,
		                   sa->wt_slo, sa->wt_window);
	} else {
		hipLaunchKernelGGL(k_rank_blocks, dim3(sa->ctx.strat_nblk), dim3(64), 0, st, onwalk, nw0, sa->d_strat_pre, sa->ctx.strat_nblk);
		hipLaunchKernelGGL(k_rank_scan, dim3(1), dim3(1024), 0, st, sa->d_strat_pre, sa->ctx.strat_nblk);
		hipLaunchKernelGGL(sa->focus_hi ? k_targets<true> : k_targets<false>, dim3((K + 3u) / 4u), dim3(256), 0, st, sa->ctx, sa->b2, onwalk, nw0, (const Control*)sa->base.ctl, sa->cfg.seed, step_override, K, sa->d_strat_tgt,
		                   sa->d_pick_hint, sa->focus_lo, sa->focus_hi);
	}
	if (sa->d_pick_order) {
		const uint32_t slices = nbr_slices(sa);
		hipLaunchKernelGGL(k_pick_order, dim3(slices), dim3(1024), 0, st, (const unsigned char*)sa->d_pick_hint, sa->d_pick_order, K, slices);
	}
}
/* The next step's targets need the on-walk bitmap of the new base and nothing else: an accept has written it long before it is
 * through with chains and checkpoints, so they are worked out on the second stream beside the rest of the accept (30 us off
 * every step).  Called right behind the launch that completes the bitmap; `next_gstep` is the step they are for.
 * Records ev_tgt_go on the main stream, queues on the second stream behind it, records ev_tgt there. */
static int launch_targets_ahead(mgl_sa* sa, uint64_t next_gstep)
{
	if (!sa->d_strat_pre || !sa->incremental) return MGL_OK;
	HIPCHK(hipEventRecord(sa->q.ev_tgt_go, sa->q.stream));
	HIPCHK(hipStreamWaitEvent(sa->q.stream2, sa->q.ev_tgt_go, 0));
	launch_targets(sa, sa->q.stream2, next_gstep);
	HIPCHK(hipEventRecord(sa->q.ev_tgt, sa->q.stream2));
	HIPCHK(hipGetLastError());
	sa->tgt_ahead = TGT_READY;
	return MGL_OK;
}

/* ---- a step's neighbour evaluation in stages: launch_neighbours calls them in the order they stand in. */
/* the eight arguments every k_neighbours2 launch shares, written once */
template <class Kern>
static void launch_nbr2(mgl_sa* sa, Kern kern, uint32_t grid, uint32_t threads, uint32_t lds, hipStream_t st, uint64_t step_override, uint32_t per_wave,
                        uint32_t* todo, uint32_t* todo_count, unsigned long long* prof, uint4* pickrec, uint32_t j0, uint32_t j1, uint4* pickstate)
{
	hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, st, sa->ctx, sa->b2, sa->base.ctl, sa->cfg.seed, step_override, sa->cfg.neighbours_per_step,
	                   sa->nbr, per_wave, todo, todo_count, prof, sa->big, pickrec, j0, j1, pickstate);
}
/* The step's targets, on the main stream.  Waits for ev_tgt if targets were queued ahead; makes them here unless those are good. */
static int nbr_targets(mgl_sa* sa, uint64_t step_override)
{
	if (!sa->d_strat_pre) return MGL_OK;
	if (sa->tgt_ahead != TGT_NONE) HIPCHK(hipStreamWaitEvent(sa->q.stream, sa->q.ev_tgt, 0)); /* made beside the previous step's accept (or at least out of the buffers' way) */
	if (sa->tgt_ahead != TGT_READY) launch_targets(sa, sa->q.stream, step_override);
	sa->tgt_ahead = TGT_NONE;
	return MGL_OK;
}
/* The full-walk kernel on the main stream; no waits, no records.  With `todo` it is the last resort of the incremental engine
 * (a small grid strides over the list), without it the full-walk engine's whole evaluation. */
static void nbr_fullwalk(mgl_sa* sa, uint64_t step_override, const uint32_t* todo, const uint32_t* todo_count)
{
	const uint32_t K = sa->cfg.neighbours_per_step, blocks = (K + sa->waves_per_block - 1) / sa->waves_per_block;
	hipLaunchKernelGGL(k_neighbours, dim3(todo && blocks > 256u ? 256u : blocks), dim3(64 * sa->waves_per_block), sa->nbr_lds, sa->q.stream, sa->ctx, sa->base.v,
	                   (const Control*)sa->base.ctl, sa->cfg.seed, step_override, K, sa->nbr, sa->per_wave_bytes, todo, todo_count); NBR_TRACE("k_neighbours");
}
/* The first two thirds of the split form -- pick, then window walk -- of every slice, as one fused launch per slice (or as
 * two: MGL_NO_FUSE, MGL_F_PROFILE).  Slices alternate between the main and the second stream.  Records ev_fork on the main
 * stream, which the second stream waits for if there are two slices or more; records ev_rest[h] behind slice h's walk on
 * its stream.  (The third stream needs no wait of its own for the fork: its first wait, ev_rest[0], is recorded on the main
 * stream behind the fork, for any number of slices.) */
static int nbr_pick_walk(mgl_sa* sa, uint64_t step_override, uint32_t slices)
{
	const uint32_t K = sa->cfg.neighbours_per_step;
	HIPCHK(hipEventRecord(sa->q.ev_fork, sa->q.stream));
	if (slices >= 2) HIPCHK(hipStreamWaitEvent(sa->q.stream2, sa->q.ev_fork, 0));
	for (uint32_t h = 0; h < slices; h++) {
		const uint32_t j0 = mgl_slice_bound(K, h, slices), j1 = mgl_slice_bound(K, h + 1, slices);
		hipStream_t st = (h & 1u) ? sa->q.stream2 : sa->q.stream;
		if (sa->form.fuse && !sa->d_prof) {
			/* pick and walk of a neighbour in one wavefront: no barrier on the slice's slowest pick in front of its walks.  Under
			 * MGL_F_PROFILE the two halves run as two launches (below): the stage marks are the pick half's */
			launch_nbr2(sa, k_neighbours2<false, MGL_NBR_PICKWALK>, j1 - j0, 64, sa->fused_lds, st, step_override, sa->fused_lds, sa->d_todo, &sa->d_counts[0].second_pass,
			            nullptr, sa->d_pickrec, j0, j1, (uint4*)sa->d_pick_order); NBR_TRACE("k_neighbours2<false, MGL_NBR_PICKWALK>"); /* the order in the unused `pickstate` slot */
		} else {
			/* under MGL_F_PROFILE the instance that carries the stage marks (tools/pick_waves.py); normal runs hold none of them */
			launch_nbr2(sa, sa->d_prof ? k_neighbours2<false, MGL_NBR_PICK, true> : k_neighbours2<false, MGL_NBR_PICK>, (j1 - j0 + sa->pick_waves - 1) / sa->pick_waves,
			            64 * sa->pick_waves, sa->pick_waves * sa->per_wave_pick, st, step_override, sa->per_wave_pick, sa->d_todo, &sa->d_counts[0].second_pass, sa->d_prof,
			            sa->d_pickrec, j0, j1, sa->d_pickstate); NBR_TRACE("k_neighbours2<false, MGL_NBR_PICK>");
			launch_nbr2(sa, k_neighbours2<false, MGL_NBR_REST>, j1 - j0, 64, sa->per_wave_rest, st, step_override, sa->per_wave_rest, sa->d_todo, &sa->d_counts[0].second_pass,
			            g_prof_big ? nullptr : sa->d_prof, sa->d_pickrec, j0, j1, sa->d_pickstate); NBR_TRACE("k_neighbours2<false, MGL_NBR_REST>");
		}
		HIPCHK(hipEventRecord(sa->q.ev_rest[h], st));
	}
	HIPCHK(hipGetLastError());
	return MGL_OK;
}
/* The second half's re-simulation, several wavefronts per neighbour: slice h's k_sim on the third stream behind a wait for
 * ev_rest[h], between its two timing slots (MGL_F_TIMING).  Records ev_sim behind the last one; then the main stream waits
 * for the ev_rest of the odd slices (the walks of the other stream's slices). */
static int nbr_sim(mgl_sa* sa, uint32_t slices)
{
	const uint32_t K = sa->cfg.neighbours_per_step;
	const uint32_t sim_lds_regular = ((((sa->ctx.L.total + 31u) >> 5) + 3u) & ~3u) * 4u + sa->chg_cap * 16u;
	hipStream_t st = sa->q.stream3;
	for (uint32_t h = 0; h < slices; h++) {
		const uint32_t j0 = mgl_slice_bound(K, h, slices), j1 = mgl_slice_bound(K, h + 1, slices);
		HIPCHK(hipStreamWaitEvent(st, sa->q.ev_rest[h], 0));
		TRY(mark(sa, T_SIM_BEGIN, st, h));
		hipLaunchKernelGGL(sa->count_traffic ? k_sim<true> : k_sim<false>, dim3(j1 - j0), dim3(64 * sa->sim_waves), sim_lds_regular, st, sa->ctx, sa->b2, sa->base.ctl, sa->nbr,
		                   sa->big, j0, j1, sa->count_traffic ? sa->d_traffic : (unsigned long long*)nullptr); NBR_TRACE("k_sim");
		TRY(mark(sa, T_SIM_END, st, h));
	}
	HIPCHK(hipEventRecord(sa->q.ev_sim, st));
	for (uint32_t h = 1; h < slices; h += 2) HIPCHK(hipStreamWaitEvent(sa->q.stream, sa->q.ev_rest[h], 0));
	return MGL_OK;
}
/* the one-kernel form, on the main stream; no waits, no records */
static void nbr_one_kernel(mgl_sa* sa, uint64_t step_override)
{
	const uint32_t K = sa->cfg.neighbours_per_step, blocks2 = (K + sa->waves_per_block2 - 1) / sa->waves_per_block2;
	launch_nbr2(sa, k_neighbours2<false, MGL_NBR_FULL>, blocks2, 64 * sa->waves_per_block2, sa->nbr2_lds, sa->q.stream, step_override, sa->per_wave2, sa->d_todo, &sa->d_counts[0].second_pass,
	            sa->d_prof, sa->d_pickrec, 0u, K, sa->d_pickstate); NBR_TRACE("k_neighbours2<false, MGL_NBR_FULL>");
}
/* The second pass, on the main stream behind whatever the regular form queued there; no records.  The few whose change lists
 * overflowed LDS (or that need a second top-K pick): the whole evaluation in one kernel, lists in global scratch, a workgroup
 * per neighbour -- one wavefront evaluates it, the others share its re-simulations */
static void nbr_second_pass(mgl_sa* sa, uint64_t step_override, bool split_now)
{
	const uint32_t bigblocks = sa->big.slots < 1024u ? sa->big.slots : 1024u; /* the kernel strides over its list: none is dropped */
	const uint32_t big_lds = 4096u + sa->per_wave2 + 12u * MGL_BIG_CAP + MGL_COOP_BYTES; /* + a copy of both lists for the re-simulations, + the workgroup's command */
	launch_nbr2(sa, k_neighbours2<true, MGL_NBR_FULL>, bigblocks, 64 * sa->big_waves, big_lds, sa->q.stream, step_override, sa->per_wave2, sa->d_todo2, &sa->d_counts[0].last_resort,
	            g_prof_big ? sa->d_prof : nullptr, split_now ? sa->d_pickrec : nullptr, 0u, sa->cfg.neighbours_per_step, sa->d_pickstate); NBR_TRACE("k_neighbours2<true, MGL_NBR_FULL>");
}
/* Whatever overflowed even the second pass: exact full walk from byte 0.  It reads the second pass's list and writes the outputs
 * of its own neighbours only, which k_sim never costs (their headers stay 0xFFFFFFFF): it is queued right behind the second
 * pass, and the re-simulations join behind it -- the main stream waits for ev_sim. */
static int nbr_last_resort(mgl_sa* sa, uint64_t step_override, bool split_now)
{
	nbr_fullwalk(sa, step_override, sa->d_todo2, &sa->d_counts[0].last_resort);
	if (split_now) HIPCHK(hipStreamWaitEvent(sa->q.stream, sa->q.ev_sim, 0));
	HIPCHK(hipGetLastError());
	return MGL_OK;
}
/* a step's neighbour evaluation: its targets, then on the incremental engine pick / walk slices on two streams, re-simulations
 * on a third, second pass, last resort */
static int launch_neighbours(mgl_sa* sa, uint64_t step_override, bool zero_counts = true)
{
	TRY(nbr_targets(sa, step_override));
	if (!sa->incremental) {
		nbr_fullwalk(sa, step_override, nullptr, nullptr);
		HIPCHK(hipGetLastError());
		return MGL_OK;
	}
	if (zero_counts) HIPCHK(hipMemsetAsync(sa->d_counts, 0, sizeof(StepCounts), sa->q.stream)); /* todo counts + spill slots; k_step_end clears them between steps */
	const bool split_now = sa->form.split_nbr && !sa->form.form_single;
	if (split_now) {
		/* the step's neighbours in slices on two streams: while the slowest wavefronts of one slice's kernel finish,
		 * the other slice's kernels keep the CUs busy.  The re-simulation kernels run on a third stream: the second
		 * pass below needs the walks, not the re-simulations, and its few long-running wavefronts overlap with them. */
		const uint32_t slices = nbr_slices(sa);
		TRY(nbr_pick_walk(sa, step_override, slices));
		TRY(nbr_sim(sa, slices));
	} else {
		nbr_one_kernel(sa, step_override);
	}
	nbr_second_pass(sa, step_override, split_now);
	return nbr_last_resort(sa, step_override, split_now);
}

static int import_slab(mgl_sa* sa, const mgl_packet* packets, mgl_pk* d_slab)
{
	HIPCHK(hipMemcpyAsync(sa->d_aos, packets, sizeof(mgl_packet) * (size_t)sa->n, hipMemcpyHostToDevice, sa->q.stream));
	hipLaunchKernelGGL(k_import, dim3(1024), dim3(256), 0, sa->q.stream, (const uint32_t*)sa->d_aos, d_slab, sa->n);
	HIPCHK(hipGetLastError());
	return MGL_OK;
}
static int export_slab(mgl_sa* sa, const mgl_pk* d_slab, mgl_packet* packets)
{
	hipLaunchKernelGGL(k_export, dim3(1024), dim3(256), 0, sa->q.stream, d_slab, sa->d_aos, sa->n);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(packets, sa->d_aos, sizeof(mgl_packet) * (size_t)sa->n, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	return MGL_OK;
}

extern "C" void mgl_sa_destroy(mgl_sa* sa)
{
	if (!sa) return;
	(void)hipSetDevice(sa->device);
	if (sa->q.stream) (void)hipStreamSynchronize(sa->q.stream);
	delete sa; /* sa->own releases everything the handle made */
}

/* ---- mgl_sa_create in stages: create_impl calls them in the order they stand in.  Everything is made through sa->own, so a
 * stage that fails leaves nothing to undo: mgl_sa_create destroys the handle. */
/* every environment switch of a handle, for an input of n bytes (EnvSwitches says what each one is) */
static void read_env(EnvSwitches& e, size_t n)
{
	const auto set = [](const char* name) { return getenv(name) != nullptr; };
	const auto num = [](const char* name) { return getenv(name) ? atoi(getenv(name)) : 0; };
	/* measured: + 8 % on the 10 MB input, nothing on the 100 KB one (its kernels are too short to overlap) */
	e.halves = set("MGL_HALVES") ? (uint32_t)num("MGL_HALVES") : (n > (1u << 20) ? 2u : 1u);
	if (e.halves < 1 || e.halves > 8) e.halves = 1;
	/* (tests): 512- and 1 024-position blocks on small inputs.  Nothing outside 8..10 is taken: the builder's LDS arrays hold
	 * MGL_PB_MAX_BLOCK positions, and a block is whole bitmap words (shift - 6) */
	const int s = num("MGL_SB_SHIFT"), w = num("MGL_SIMW"), pw = num("MGL_PICK_WAVES");
	e.sb_shift = s >= 8 && s <= (int)MGL_PB_MAX_SHIFT ? (uint32_t)s : 0u;
	e.no_incremental_apply = set("MGL_NO_INCREMENTAL_APPLY"); e.no_batch = set("MGL_NO_BATCH"); e.no_evcancel = set("MGL_NO_EVCANCEL");
	e.no_split = set("MGL_NO_SPLIT"); e.no_cont = set("MGL_NO_CONT"); e.no_fuse = set("MGL_NO_FUSE");
	e.no_adapt = set("MGL_NO_ADAPT"); e.no_order = set("MGL_NO_ORDER");
	e.simw = w == 1 || w == 2 || w == 4 || w == 8 ? (uint32_t)w : 0u;
	e.pick_waves = pw == 1 || pw == 2 || pw == 4 || pw == 8 ? (uint32_t)pw : 0u;
	e.bulk_threshold = set("MGL_BULK_THRESHOLD") ? (uint32_t)num("MGL_BULK_THRESHOLD") : 0u;
	if (set("MGL_BULK_THRESHOLD") && e.bulk_threshold == 0) e.bulk_threshold = 1;
}
static int create_streams(mgl_sa* sa)
{
	DevOwner& own = sa->own;
	HIPCHK(own.stream(&sa->q.stream));
	HIPCHK(own.stream(&sa->q.stream2));
	for (hipEvent_t* e : { &sa->q.ev_fork, &sa->q.ev_join, &sa->q.ev_tgt, &sa->q.ev_tgt_go }) HIPCHK(own.event(e, hipEventDisableTiming));
	HIPCHK(own.stream(&sa->q.stream3));
	for (auto& e : sa->q.ev_rest) HIPCHK(own.event(&e, hipEventDisableTiming));
	HIPCHK(own.event(&sa->q.ev_sim, hipEventDisableTiming));
	HIPCHK(own.event(&sa->q.ev_val, hipEventDisableTiming));
	sa->halves = sa->env.halves;
	HIPCHK(own.event(&sa->timer.ev_begin));
	HIPCHK(own.event(&sa->timer.ev_end));
	return MGL_OK;
}

static int alloc_match_index(mgl_sa* sa, size_t n)
{
	DevOwner& own = sa->own;
	MatchIndex& ix = sa->ix;
	TRY(dnew(own, ix.bucket_off, 65537));
	TRY(dnew(own, ix.bucket_pos, n));
	TRY(dnew(own, ix.bucket_nx, n));
	TRY(dnew(own, ix.quad_pos, n));
	TRY(dnew(own, ix.quad_nx, n));
	ix.xpos[0] = ix.bucket_pos; ix.xpos[2] = ix.quad_pos; /* D = 2 and D = 4 are the bigram and the four-byte order */
	for (int i = 0; i < 6; i++) {
		TRY(dnew(own, ix.xnxb[i], n + 1, 0));
		if (!ix.xpos[i]) TRY(dnew(own, ix.xpos[i], n + 1, 0));
		if (i == 0) continue; /* the bucket bounds play the part of rank and run */
		TRY(dnew(own, ix.xrank[i], n + 1, 0));
		TRY(dnew(own, ix.xrun[i], n + 1, 0));
	}
	for (uint32_t** a : { &ix.oct_pos, &ix.oct_rank, &ix.oct_run, &ix.hex_pos, &ix.hex_rank, &ix.hex_run }) TRY(dnew(own, *a, n + 1, 0));
	TRY(dnew(own, ix.oct_nx8, n + 1));
	return dnew(own, ix.hex_nx8, n + 1);
}
/* match index (substring_enumerator.c:26-47): positions bucketed by leading bigram, ascending inside a bucket, and the
 * deeper orders of the same positions -- stable counting sorts on the device (mgl_index.hip) */
static int build_match_index(mgl_sa* sa, size_t n)
{
	TRY(alloc_match_index(sa, n));
	const MatchIndex& ix = sa->ix;
	const uint32_t m = (uint32_t)(n - 1); /* positions that start a bigram */
	if (m == 0) {
		HIPCHK(hipMemset(ix.bucket_off, 0, sizeof(uint32_t) * 65537));
		return MGL_OK;
	}
	const uint8_t* data = sa->d_data;
	hipStream_t st = sa->q.stream;
	const uint32_t nblk = (m + MGL_IX_ITEMS - 1) / MGL_IX_ITEMS;
	const dim3 per_pos(m / 256 + 1);
	DevOwner scratch; /* gone when the index stands, and when a step fails */
	uint32_t *tmp = nullptr, *matrix = nullptr;
	TRY(dnew(scratch, tmp, m));
	TRY(dnew(scratch, matrix, 256 * (size_t)nblk));
	/* the positions ordered by their first D bytes, then by position, into dst: one count / scan / scatter pass per byte, the
	 * last byte first.  The first pass reads no input (the positions in order); odd passes write tmp and even ones dst, so
	 * that the last pass (byte 0) lands in dst */
	auto radix_order = [&](uint32_t D, uint32_t* dst) {
		for (int pass = (int)D - 1; pass >= 0; pass--) {
			const uint32_t* in = pass == (int)D - 1 ? nullptr : ((pass & 1) ? (const uint32_t*)dst : (const uint32_t*)tmp);
			uint32_t* out = (pass & 1) ? tmp : dst;
			hipLaunchKernelGGL(ix_count, dim3(nblk), dim3(64), 0, st, data, in, m, pass, matrix, nblk);
			hipLaunchKernelGGL(ix_scan, dim3(1), dim3(1024), 0, st, matrix, 256u * nblk);
			hipLaunchKernelGGL(ix_scatter, dim3(nblk), dim3(64), 0, st, data, in, out, m, pass, (const uint32_t*)matrix, nblk);
		}
	};
	/* of an order deeper than the bigram's: rank, the bytes that follow the prefix, run starts */
	auto level = [&](const uint32_t* pos, uint32_t* rank, uint32_t* run, void* nx, uint32_t D, uint32_t nxbytes) {
		hipLaunchKernelGGL(ix_rank, per_pos, dim3(256), 0, st, pos, m, rank);
		if (nxbytes == 1) hipLaunchKernelGGL(ix_next_byte, per_pos, dim3(256), 0, st, data, pos, m, (uint8_t*)nx, D);
		else hipLaunchKernelGGL(ix_next_bytes, per_pos, dim3(256), 0, st, data, pos, m, nx, D, nxbytes);
		hipLaunchKernelGGL(ix_heads, per_pos, dim3(256), 0, st, data, pos, m, D, run);
		hipLaunchKernelGGL(ix_maxscan, dim3(1), dim3(1024), 0, st, run, m);
	};
	radix_order(2, ix.bucket_pos); /* by data[p + 1], then data[p] */
	hipLaunchKernelGGL(ix_offsets, per_pos, dim3(256), 0, st, data, (const uint32_t*)ix.bucket_pos, m, ix.bucket_off);
	hipLaunchKernelGGL(ix_next2, per_pos, dim3(256), 0, st, data, (const uint32_t*)ix.bucket_pos, m, ix.bucket_nx, 0);
	radix_order(4, ix.quad_pos);
	hipLaunchKernelGGL(ix_next2, per_pos, dim3(256), 0, st, data, (const uint32_t*)ix.quad_pos, m, ix.quad_nx, 1);
	for (uint32_t D : { 3u, 5u, 6u, 7u }) radix_order(D, ix.xpos[D - 2]);
	radix_order(8, ix.oct_pos);
	radix_order(16, ix.hex_pos);
	hipLaunchKernelGGL(ix_next_byte, per_pos, dim3(256), 0, st, data, (const uint32_t*)ix.bucket_pos, m, ix.xnxb[0], 2u);
	for (uint32_t i = 1; i < 6; i++) level(ix.xpos[i], ix.xrank[i], ix.xrun[i], ix.xnxb[i], i + 2u, 1u);
	level(ix.oct_pos, ix.oct_rank, ix.oct_run, ix.oct_nx8, 8u, 8u);
	level(ix.hex_pos, ix.hex_rank, ix.hex_run, ix.hex_nx8, 16u, 8u);
	const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(st); /* before the scratch goes */
	HIPCHK(e1);
	HIPCHK(e2);
	return MGL_OK;
}
/* DevCtx's views of the index */
static void fill_ctx_index(DevCtx& c, const MatchIndex& ix)
{
	c.bucket_off = ix.bucket_off; c.bucket_pos = ix.bucket_pos; c.bucket_nx = ix.bucket_nx; c.quad_pos = ix.quad_pos; c.quad_nx = ix.quad_nx;
	for (int i = 0; i < 6; i++) { c.xpos[i] = ix.xpos[i]; c.xrank[i] = ix.xrank[i]; c.xrun[i] = ix.xrun[i]; c.xnxb[i] = ix.xnxb[i]; }
	c.oct_pos = ix.oct_pos; c.oct_rank = ix.oct_rank; c.oct_run = ix.oct_run; c.oct_nx8 = ix.oct_nx8;
	c.hex_pos = ix.hex_pos; c.hex_rank = ix.hex_rank; c.hex_run = ix.hex_run; c.hex_nx8 = ix.hex_nx8;
}

/* the two bases, the neighbours' outputs, the bulk selection's buffers and the staging areas of the API calls */
static int alloc_search_buffers(mgl_sa* sa, size_t n, uint32_t ckpt_elems)
{
	DevOwner& own = sa->own;
	TRY(alloc_base(own, sa->base, (uint32_t)n, ckpt_elems));
	TRY(alloc_base(own, sa->scratch, (uint32_t)n, ckpt_elems));
	const size_t K = sa->cfg.neighbours_per_step;
	TRY(dnew(own, sa->nbr.cost, K));
	TRY(dnew(own, sa->nbr.ndiffs, K));
	TRY(dnew(own, sa->nbr.walked, K));
	TRY(dnew(own, sa->nbr.win, 2 * K, 0xFF));
	TRY(dnew(own, sa->nbr.win2, K, 0xFF));
	memset(&sa->bulk, 0, sizeof sa->bulk);
	TRY(dnew(own, sa->bulk.ckey, K));
	TRY(dnew(own, sa->bulk.cwin, K));
	TRY(dnew(own, sa->bulk.taken, K));
	TRY(dnew(own, sa->bulk.cstate, 2 * K));
	TRY(dnew(own, sa->bulk.cflags, K, 0));
	TRY(dnew(own, sa->bulk.hdr, 1));
	BulkHdr h0 = {};
	h0.min_key = ~0ull;
	HIPCHK(hipMemcpy(sa->bulk.hdr, &h0, sizeof h0, hipMemcpyHostToDevice));
	TRY(dnew(own, sa->nbr.dpos, K * MGL_MAX_DIFFS));
	TRY(dnew(own, sa->nbr.dold, K * MGL_MAX_DIFFS));
	TRY(dnew(own, sa->nbr.dnew, K * MGL_MAX_DIFFS));
	TRY(dalloc(own, (void**)&sa->d_aos, sizeof(mgl_packet) * n));
	TRY(dnew(own, sa->d_cum, n));
	TRY(dnew(own, sa->d_final_probs, ckpt_elems));
	TRY(dnew(own, sa->d_topk_pk, 64));
	TRY(dnew(own, sa->d_topk_cost, 64));
	TRY(dnew(own, sa->d_small, 16));
	sa->sub_cap = 1u << 20;
	TRY(dnew(own, sa->d_sub_offs, sa->sub_cap));
	return dnew(own, sa->d_sub_lens, sa->sub_cap);
}

/* the parallel builder's buffers (mgl_pbuild.hip), on the blocks of the chain index */
static int alloc_pbuild(mgl_sa* sa, size_t n, uint32_t ckpt_elems)
{
	DevOwner& own = sa->own;
	PBuild& pb = sa->pb;
	memset(&pb, 0, sizeof pb);
	pb.shift = sa->b2.sb_shift; /* 256 / 512 / 1 024 positions per block up to 1 MiB / 8 MiB / above */
	pb.nblk = (uint32_t)((n + (1u << pb.shift) - 1) >> pb.shift);
	pb.ngrp = (pb.nblk + MGL_PB_GROUP - 1u) / MGL_PB_GROUP;
	const size_t nblk = pb.nblk, nch = (nblk + MGL_PB_SCAN_CHUNK - 1u) / MGL_PB_SCAN_CHUNK;
	TRY(dnew(own, pb.exits, nblk * MGL_PB_ENTRIES));
	TRY(dnew(own, pb.entry, nblk + 1));
	TRY(dnew(own, pb.gexits, (size_t)pb.ngrp * MGL_PB_ENTRIES));
	TRY(dnew(own, pb.gentry, pb.ngrp));
	TRY(dnew(own, pb.ch_map, nch));
	TRY(dnew(own, pb.ch_vs, 8 * nch));
	TRY(dnew(own, pb.ch_pk, nch));
	TRY(dnew(own, pb.ch_state, 8 * nch));
	TRY(dnew(own, pb.gsum, (size_t)((pb.nblk + MGL_PB_OFF_ROWS - 1u) / MGL_PB_OFF_ROWS) * ckpt_elems));
	TRY(dnew(own, pb.tf_ctx, nblk));
	TRY(dnew(own, pb.tf_dist, 8 * nblk));
	TRY(dnew(own, pb.tf_pk, nblk));
	TRY(dnew(own, pb.st_in, 8 * nblk));
	TRY(dnew(own, pb.hist, nblk * ckpt_elems));
	TRY(dnew(own, pb.stage, nblk * ((MGL_PB_STAGE_PER_POS << pb.shift) + 32u)));
	TRY(dnew(own, pb.stage_n, nblk));
	TRY(dnew(own, pb.stage_over, 1, 0));
	TRY(dnew(own, pb.acc, 1, 0));
	pb.seg_cap = sa->b2.pool_cap / MGL_PB_SEG + ckpt_elems + 64u;
	TRY(dnew(own, pb.seg_off, ckpt_elems + 1));
	return dnew(own, pb.unres, pb.seg_cap);
}
/* incremental engine: the geometry of its base (bitmaps, special-state records, dense checkpoints, event chains, chain index),
 * the base, the parallel builder, the snapshots of the all-literal and the best slab */
static int create_engine(mgl_sa* sa, size_t n, uint32_t ckpt_elems)
{
	DevOwner& own = sa->own;
	const size_t K = sa->cfg.neighbours_per_step;
	Base2& b = sa->b2;
	memset(&b, 0, sizeof b);
	b.slab = sa->base.v.slab;
	b.onwalk = sa->base.v.onwalk;
	b.nw0 = (uint32_t)((n + 63) / 64);
	b.nw1 = (b.nw0 + 63) / 64;
	b.nw2 = (b.nw1 + 63) / 64;
	b.nck = (uint32_t)((n + (1u << MGL_CK2_SHIFT) - 1) >> MGL_CK2_SHIFT);
	b.ck_elems = ckpt_elems;
	b.pool_cap = (uint32_t)(24 * n + (size_t)sa->ctx.L.total * 272 + 4096);
	/* chain index: one entry per context and block of the parallel builder (the builder's per-block counts are its source) */
	b.sb_shift = n <= (1u << 20) ? 8u : n <= (1u << 23) ? 9u : MGL_PB_MAX_SHIFT;
	if (sa->env.sb_shift) b.sb_shift = sa->env.sb_shift;
	b.nsb = (uint32_t)((n + (1u << b.sb_shift) - 1) >> b.sb_shift);
	b.sb_stride = (b.nsb + 2u + 3u) & ~3u;
	TRY(alloc_b2(own, b, n, false, true, &sa->b2_bytes));
	sa->parallel_build = !(sa->cfg.flags & MGL_F_SERIAL_BUILD);
	if (sa->parallel_build) TRY(alloc_pbuild(sa, n, ckpt_elems));
	sa->snapshots = !(sa->cfg.flags & MGL_F_NO_SNAPSHOTS);
	if (sa->snapshots) {
		for (Base2* s : { &sa->snap_lit, &sa->snap_best }) {
			*s = b; /* the geometry; every array becomes the snapshot's own */
			TRY(alloc_b2(own, *s, n, true, false, nullptr));
		}
		TRY(dnew(own, sa->d_snap_meta, 2, 0));
		sa->d_best = sa->snap_best.slab; /* packets_best lives in the best snapshot */
	}
	if (sa->cfg.flags & MGL_F_PROFILE) TRY(dnew(own, sa->d_prof, 64 + 2 * K, 0));
	return dnew(own, sa->d_todo, K + 1, 0);
}

/* the in-place accepts' buffers: single (ApplyBuf, mgl_kernels3.hip) and batch (BatchBuf, mgl_kernels5.hip), and their limits */
static int alloc_accept_buffers(mgl_sa* sa)
{
	DevOwner& own = sa->own;
	sa->incremental_apply = !sa->env.no_incremental_apply;
	ApplyBuf& ab = sa->ab;
	memset(&ab, 0, sizeof ab);
	/* one workgroup per touched context plans the rewrite; the copies run as job lists */
	sa->apply_blocks = 256;
	ab.scratch_cap = sa->b2.pool_cap + 256u;
	ab.span_cap = 1u << 22;
	ab.job_cap = 1u << 20;
	TRY(dnew(own, ab.hdr, 1, 0));
	TRY(dnew(own, ab.ins_key, MGL_BATCH_ALLOC)); /* a single accept uses MGL_APPLY_CAP of each of these four */
	TRY(dnew(own, ab.rem_key, MGL_BATCH_ALLOC));
	TRY(dnew(own, ab.ins_pos, MGL_BATCH_ALLOC));
	TRY(dnew(own, ab.rem_pos, MGL_BATCH_ALLOC));
	TRY(dnew(own, ab.tctx, 16384));
	TRY(dnew(own, ab.scratch_pos, ab.scratch_cap));
	TRY(dnew(own, ab.scratch_ev, ab.scratch_cap));
	TRY(dnew(own, ab.span_pos, ab.span_cap));
	TRY(dnew(own, ab.span_ev, ab.span_cap));
	TRY(dnew(own, ab.jobs_b, ab.job_cap));
	TRY(dnew(own, ab.jobs_c, ab.job_cap));
	BatchBuf& bt = sa->batch;
	memset(&bt, 0, sizeof bt);
	TRY(dnew(own, bt.hdr, 1, 0));
	TRY(dnew(own, bt.cl, MGL_CL_WORDS * MGL_BATCH_MAX));
	TRY(dnew(own, bt.jpos, MGL_BATCH_MAX * MGL_MAX_DIFFS));
	TRY(dnew(own, bt.jnew, MGL_BATCH_MAX * MGL_MAX_DIFFS));
	TRY(dnew(own, bt.jold, MGL_BATCH_MAX * MGL_MAX_DIFFS));
	TRY(dnew(own, bt.st_ikey, MGL_BATCH_ALLOC));
	TRY(dnew(own, bt.st_rkey, MGL_BATCH_ALLOC));
	TRY(dnew(own, bt.st_ipos, MGL_BATCH_ALLOC));
	TRY(dnew(own, bt.st_rpos, MGL_BATCH_ALLOC));
	TRY(dnew(own, bt.ops, 2 * (size_t)MGL_BATCH_MAX * MGL_BATCH_OPCAP));
	TRY(dnew(own, bt.ins_cl, MGL_BATCH_ALLOC));
	TRY(dnew(own, bt.rem_cl, MGL_BATCH_ALLOC));
	bt.nctx = sa->ctx.L.total;
	bt.runs_cap = 1u << 17;
	TRY(dnew(own, bt.runs, 2 * (size_t)bt.runs_cap));
	for (uint32_t** p : { &bt.cnt_i, &bt.cnt_r, &bt.off_i, &bt.off_r, &bt.cur_i, &bt.cur_r, &bt.touched }) TRY(dnew(own, *p, bt.nctx + 64u, 0));
	TRY(dnew(own, bt.bk_ipos, MGL_BATCH_ALLOC));
	TRY(dnew(own, bt.bk_rpos, MGL_BATCH_ALLOC));
	TRY(dnew(own, bt.bk_ibit, MGL_BATCH_ALLOC));
	TRY(dnew(own, bt.bk_icl, MGL_BATCH_ALLOC));
	TRY(dnew(own, bt.bk_rcl, MGL_BATCH_ALLOC));
	TRY(dnew(own, bt.acc, 1, 0));
	HIPCHK(own.pinned((void**)&sa->h_bstat, sizeof(BatchHdr)));
	HIPCHK(own.event(&sa->q.ev_bstat, hipEventDisableTiming));
	sa->batch_ok = sa->incremental_apply && !sa->env.no_batch;
	uint32_t* why = nullptr;
	TRY(dnew(own, why, 1, 0));
	accept_limits_init(sa, why);
	return MGL_OK;
}

/* what the neighbour evaluation keeps in global memory: the second pass's list areas, the hand-over between the halves of the
 * split form, the re-simulation's lists and headers, the continuation records, the per-step counters */
static int alloc_nbr_scratch(mgl_sa* sa, uint32_t ckpt_elems)
{
	DevOwner& own = sa->own;
	const size_t K = sa->cfg.neighbours_per_step;
	/* first-pass list size: a step of few neighbours leaves most of the LDS idle, and on repetitive inputs
	 * (long matches everywhere) windows are long: give the lists the room */
	sa->chg_cap = K <= 1024u ? 4u * MGL_CHG_CAP : (K <= 2048u ? 2u * MGL_CHG_CAP : MGL_CHG_CAP);
	BigScratch& g = sa->big;
	memset(&g, 0, sizeof g);
	g.chg_cap = sa->chg_cap;
	g.cap = MGL_BIG_CAP; g.uctx_cap = ckpt_elems; g.slots = (uint32_t)(K > 512 ? K : 512); /* every neighbour of a step may need one */
	const size_t slots = g.slots;
	TRY(dnew(own, g.ins_key, g.cap * slots));
	TRY(dnew(own, g.rem_key, g.cap * slots));
	TRY(dnew(own, g.ins_pos, g.cap * slots));
	TRY(dnew(own, g.rem_pos, g.cap * slots));
	TRY(dnew(own, g.uctx, g.uctx_cap * slots));
	TRY(dnew(own, sa->d_todo2, K + 1, 0));
	TRY(dnew(own, sa->d_counts, 2, 0));
	g.todo_in = sa->d_todo; g.todo_in_count = &sa->d_counts[0].second_pass; g.spill_ctr = &sa->d_counts[0].spill_slots;
	g.evcancel = sa->env.no_evcancel ? 0u : 1u; /* the window walk lists a re-coded packet's changed events only; MGL_NO_EVCANCEL=1: all of them */
	TRY(dnew(own, sa->d_pickrec, K));
	TRY(dnew(own, sa->d_pickstate, 2 * K));
	sa->form.split_nbr = !sa->env.no_split;
	if (sa->form.split_nbr) {
		/* the second half's re-simulation as its own launch (k_sim): lists and headers per neighbour */
		TRY(dnew(own, g.sim_hdr, K, 0xFF));
		TRY(dnew(own, g.sim_keys, 2u * sa->chg_cap * K));
		TRY(dnew(own, g.sim_pos, 2u * sa->chg_cap * K));
		/* continuation records: the second half saves a walk that stops at a repair pick, the second pass resumes it */
		if (!sa->env.no_cont) TRY(dnew(own, g.cont, MGL_CONT_WORDS * slots, 0));
	}
	return dnew(own, sa->d_traffic, 2, 0);
}

/* every dynamic LDS size, the wavefronts per workgroup of every neighbour launch, the kernels' LDS attributes, and the switches
 * of the launch path.  LDS budget of the full-walk kernels: 4 KiB cost table + per wave {probabilities, 2x272 length prices,
 * journal} */
static int set_launch_geometry(mgl_sa* sa, size_t n, uint32_t ckpt_elems)
{
	const uint32_t cu_lds = 160u * 1024u;
	sa->per_wave_bytes = ckpt_elems * 2u + MGL_PRICE_WORDS * 4u + MGL_MAX_DIFFS * (8u + 8u + 4u);
	sa->waves_per_block = 4;
	while (sa->waves_per_block > 1 && 4096u + sa->waves_per_block * sa->per_wave_bytes > cu_lds) sa->waves_per_block--;
	sa->nbr_lds = 4096u + sa->waves_per_block * sa->per_wave_bytes;
	sa->walk_lds = 4096u + ckpt_elems * 2u + MGL_PRICE_WORDS * 4u;
	HIPCHK(hipFuncSetAttribute((const void*)k_neighbours, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sa->nbr_lds));
	HIPCHK(hipFuncSetAttribute((const void*)k_rebuild, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sa->walk_lds));
	HIPCHK(hipFuncSetAttribute((const void*)k_topk_probe<0>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sa->walk_lds));
	HIPCHK(hipFuncSetAttribute((const void*)k_topk_probe<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sa->walk_lds));
	if (!sa->incremental) return MGL_OK;

	/* journal + context bitmap + max(model + price tables, change lists + context list) */
	const uint32_t fixed = MGL_MAX_DIFFS * (8u + 8u + 4u) + (((((sa->ctx.L.total + 31u) >> 5) + 3u) & ~3u) * 4u);
	const uint32_t model = ckpt_elems * 2u + MGL_PRICE_WORDS * 4u;
	const uint32_t lists = sa->chg_cap * (4u + 4u + 2u + 2u) + 2u * sa->chg_cap * 2u;
	sa->per_wave2 = (fixed + (model > lists ? model : lists) + 15u) & ~15u;
	sa->per_wave_pick = (model + 15u) & ~15u; /* no journal / bitmap in the pick half */
	sa->per_wave_rest = (fixed + lists + 15u) & ~15u;
	/* measured: one wavefront per workgroup wins although more would pack more waves into a CU's 160 KiB of LDS (LDS is
	 * released per workgroup, and neighbour run times have a long tail) */
	sa->waves_per_block2 = 1;
	sa->nbr2_lds = 4096u + sa->waves_per_block2 * sa->per_wave2;
	sa->build_lds = 4096u + ckpt_elems * 2u + ckpt_elems * 8u;
	sa->fused_lds = (sa->per_wave_pick > sa->per_wave_rest ? sa->per_wave_pick : sa->per_wave_rest);
	HIPCHK(hipFuncSetAttribute((const void*)k_neighbours2<false, MGL_NBR_FULL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sa->nbr2_lds));
	HIPCHK(hipFuncSetAttribute((const void*)k_neighbours2<false, MGL_NBR_PICK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cu_lds));
	HIPCHK(hipFuncSetAttribute((const void*)k_neighbours2<false, MGL_NBR_PICK, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cu_lds));
	HIPCHK(hipFuncSetAttribute((const void*)k_neighbours2<false, MGL_NBR_REST>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sa->nbr2_lds));
	HIPCHK(hipFuncSetAttribute((const void*)k_neighbours2<true, MGL_NBR_FULL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4096u + sa->per_wave2 + 12u * MGL_BIG_CAP + MGL_COOP_BYTES)));
	HIPCHK(hipFuncSetAttribute((const void*)k_neighbours2<false, MGL_NBR_PICKWALK>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sa->fused_lds));
	HIPCHK(hipFuncSetAttribute((const void*)k_sim<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
	HIPCHK(hipFuncSetAttribute((const void*)k_sim<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
	HIPCHK(hipFuncSetAttribute((const void*)k_build, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sa->build_lds));
	HIPCHK(hipFuncSetAttribute((const void*)k_build_end, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sa->build_lds));

	sa->form.fuse = !sa->env.no_fuse;
	if (sa->env.simw) sa->sim_waves = sa->env.simw;
	sa->form.adaptive = sa->form.split_nbr && !sa->env.no_adapt;
	sa->form.form_single = !sa->form.split_nbr; /* one-kernel form only, or the split form until the device recommends otherwise */
	/* eight pick wavefronts share a cost table per workgroup: 4 KiB + 8 x 9.3 KiB = 78 KiB, two
	 * workgroups = 16 wavefronts per CU, so the 4 096 neighbours of a c2 step are all resident at
	 * once (with two per workgroup 14 fit and the last 512 waited for a slot: 127 -> 108 us).
	 * Above 1 MiB top-K run times vary too much for wavefronts to hold each other's LDS: one per
	 * workgroup there (c3, first 200 steps: 3.04 ms per step against 3.26 with eight) */
	sa->pick_waves = sa->env.pick_waves;
	/* the workgroup size that puts most wavefronts on a CU's 160 KiB (larger models -- lc > 0 -- fit fewer) */
	uint32_t best_w = 1, best_resident = 0;
	for (uint32_t w = 1; w <= 8; w *= 2) {
		const uint32_t bytes = w * sa->per_wave_pick;
		if (bytes > cu_lds) break;
		const uint32_t resident = (cu_lds / ((bytes + 1279u) / 1280u * 1280u)) * w;
		if (resident > best_resident) { best_resident = resident; best_w = w; }
	}
	if (n > (1u << 20)) best_w = 1;
	if (sa->pick_waves == 0 || sa->pick_waves * sa->per_wave_pick > cu_lds) sa->pick_waves = best_w;
	return MGL_OK;
}

/* targets: stratified by packet ordinal (default), or position draws (MGL_F_POSITION_TARGETS); and the decision's thresholds */
static int create_targets(mgl_sa* sa, size_t n)
{
	DevOwner& own = sa->own;
	const size_t K = sa->cfg.neighbours_per_step;
	if (!(sa->cfg.flags & MGL_F_POSITION_TARGETS)) {
		sa->ctx.strat_nblk = (uint32_t)((n + 4095u) / 4096u);
		TRY(dnew(own, sa->d_strat_pre, sa->ctx.strat_nblk + 2u, 0));
		sa->ctx.strat_pre = sa->d_strat_pre;
		TRY(dnew(own, sa->d_strat_tgt, K));
		sa->ctx.strat_tgt = sa->d_strat_tgt;
		TRY(dnew(own, sa->d_focus_cnt, 2, 0));
		/* the fused launch takes up its picking neighbours first; MGL_NO_ORDER=1: in blockIdx order */
		if (sa->incremental && sa->form.split_nbr && !sa->env.no_order) {
			TRY(dnew(own, sa->d_pick_hint, K, 1));
			TRY(dnew(own, sa->d_pick_order, K));
		}
	}
	sa->sqrt_thresh = ceil_sqrt_u64(sa->cfg.iters_per_epoch);
	/* a bulk step costs a parallel rebuild (about 3 single steps at 100 KB, 6 at 10 MB, 20 at 100 MB) */
	/* ... unless the step takes few moves: those are patched in at once (mgl_kernels5.hip) for about half a single step's time, so a bulk
	 * step pays as soon as it can be expected to take two moves */
	sa->bulk_threshold = sa->env.bulk_threshold ? sa->env.bulk_threshold : sa->batch_ok ? 2u : (n <= (1u << 20) ? 16u : n <= (1u << 24) ? 32u : 128u);
	return MGL_OK;
}

/* packet_slab_new: all-literal current and best slabs, the base built on them and checked */
static int first_build(mgl_sa* sa, size_t n)
{
	hipLaunchKernelGGL(k_fill_literal, dim3(1024), dim3(256), 0, sa->q.stream, sa->base.v.slab, sa->ctx.n);
	if (!sa->d_best) TRY(dnew(sa->own, sa->d_best, n)); /* (with snapshots it is the best snapshot's slab) */
	hipLaunchKernelGGL(k_fill_literal, dim3(1024), dim3(256), 0, sa->q.stream, sa->d_best, sa->ctx.n);
	HIPCHK(hipGetLastError());
	TRY(rebuild_base(sa, 0));
	if (sa->incremental && sa->snapshots) TRY(launch_snapshot(sa, sa->snap_lit, 0, 0, 0));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	/* an input the structures were not sized for shows here, not steps later inside mgl_sa_run */
	Control c0;
	HIPCHK(hipMemcpy(&c0, sa->base.ctl, sizeof c0, hipMemcpyDeviceToHost));
	if (c0.error_flags) return fail(MGL_EDEVICE, "mgl_sa_create: building the base structures of the all-literal slab failed");
	return MGL_OK;
}

static int create_impl(mgl_sa* sa, const uint8_t* data, size_t n)
{
	HIPCHK(hipSetDevice(sa->device));
	read_env(sa->env, n);
	TRY(create_streams(sa));
	const mgl_layout L = mgl_make_layout(sa->props.lc, sa->props.lp, sa->props.pb);
	const uint32_t ckpt_elems = (L.total + 7u) & ~7u;
	/* input, zero padded so that window loads past the end stay in bounds */
	TRY(dnew(sa->own, sa->d_data, n + 128, 0));
	HIPCHK(hipMemcpy(sa->d_data, data, n, hipMemcpyHostToDevice));
	TRY(build_match_index(sa, n));
	TRY(dnew(sa->own, sa->d_cost_tbl, 2048));
	HIPCHK(hipMemcpy(sa->d_cost_tbl, k_cost_table, sizeof(k_cost_table), hipMemcpyHostToDevice));
	sa->ctx.data = sa->d_data; sa->ctx.n = (uint32_t)n;
	fill_ctx_index(sa->ctx, sa->ix);
	sa->ctx.cost_tbl = sa->d_cost_tbl; sa->ctx.L = L;
	sa->ctx.dict_limit = sa->cfg.dict_limit; sa->ctx.max_scan = sa->cfg.max_bucket_scan; sa->ctx.top_k = sa->cfg.top_k;
	TRY(alloc_search_buffers(sa, n, ckpt_elems));
	sa->incremental = !(sa->cfg.flags & MGL_F_FULLWALK);
	if (sa->incremental) {
		TRY(create_engine(sa, n, ckpt_elems));
		TRY(alloc_accept_buffers(sa));
		TRY(alloc_nbr_scratch(sa, ckpt_elems));
	}
	TRY(set_launch_geometry(sa, n, ckpt_elems));
	TRY(create_targets(sa, n));
	return first_build(sa, n);
}

extern "C" mgl_sa* mgl_sa_create(const uint8_t* data, size_t n, mgl_properties props, const mgl_sa_config* cfg)
{
	if (!data || n == 0 || !cfg) { fail(MGL_EINVAL, "mgl_sa_create: bad data/size/config"); return nullptr; }
	/* 32-bit chain pool: 24 n + 272 contexts + slack must fit (and costs stay below 2^44: k_decide packs cost << 20 | j) */
	if (n > MGL_MAX_INPUT) { fail(MGL_EINVAL, "mgl_sa_create: input larger than 176 000 000 bytes is not supported"); return nullptr; }
	if (props.lc + props.lp > 4 || props.pb > 4 || props.lc > 8) { fail(MGL_EINVAL, "mgl_sa_create: unsupported lc/lp/pb"); return nullptr; }
	mgl_sa* sa = new (std::nothrow) mgl_sa();
	if (!sa) { fail(MGL_ENOMEM, "mgl_sa_create: out of host memory"); return nullptr; }
	sa->cfg = *cfg;
	sa->props = props;
	sa->n = (uint32_t)n;
	sa->device = cfg->device;
	if (sa->cfg.neighbours_per_step == 0) sa->cfg.neighbours_per_step = 1;
	if (sa->cfg.neighbours_per_step > (1u << 20)) { delete sa; fail(MGL_EINVAL, "neighbours_per_step > 2^20"); return nullptr; }
	if (sa->cfg.top_k == 0) sa->cfg.top_k = 20;
	if (sa->cfg.top_k > MGL_MAX_TOPK) { delete sa; fail(MGL_EINVAL, "top_k > 32"); return nullptr; }
	if (sa->cfg.dict_limit == 0) sa->cfg.dict_limit = 0x400000u;
	if (sa->cfg.iters_per_epoch == 0) sa->cfg.iters_per_epoch = n;
	int rc = create_impl(sa, data, n);
	if (rc != MGL_OK) {
		std::string keep = g_err;
		mgl_sa_destroy(sa);
		g_err = keep;
		return nullptr;
	}
	return sa;
}

static int read_ctl(mgl_sa* sa, BaseMem& b, Control* out)
{
	HIPCHK(hipMemcpyAsync(out, b.ctl, sizeof(Control), hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	return MGL_OK;
}
static int write_ctl(mgl_sa* sa, BaseMem& b, const Control* in)
{
	HIPCHK(hipMemcpyAsync(b.ctl, in, sizeof(Control), hipMemcpyHostToDevice, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	return MGL_OK;
}

/* the base still is the only holder of the best slab's structures and is about to be replaced */
static int keep_best_before_overwrite(mgl_sa* sa, Control& c)
{
	if (!(sa->incremental && sa->snapshots) || !c.best_is_current) return MGL_OK;
	int rc = launch_snapshot(sa, sa->snap_best, 1, 0, 0);
	if (rc) return rc;
	c.best_is_current = 0;
	return MGL_OK;
}


/* The base has just been rebuilt on a new current slab: the walk's verdict on it, after checking every packet against the
 * input too if `validate`.  A slab that fails is `bad` in the name of `who`; *cost (nullable) = its exact cost. */
static int check_current(mgl_sa* sa, bool validate, int bad, const char* who, uint64_t* cost)
{
	int rc;
	Control c;
	if (validate && (rc = launch_validate(sa))) return rc;
	if ((rc = read_ctl(sa, sa->base, &c))) return rc;
	if (c.error_flags) return fail(bad, std::string(who) + ": the new current slab is not a valid parse of the input");
	if (cost) *cost = c.rebuild_cost;
	return MGL_OK;
}

/* The current slab becomes the all-literal one, with its base structures and its exact cost: from the kept copy where
 * there is one, else filled, rebuilt and kept.  The control block's flags and counters are the caller's business. */
static int current_to_literal(mgl_sa* sa)
{
	int rc;
	const bool snaps = sa->incremental && sa->snapshots;
	if (snaps) {
		SnapMeta meta;
		HIPCHK(hipMemcpyAsync(&meta, sa->d_snap_meta, sizeof meta, hipMemcpyDeviceToHost, sa->q.stream));
		HIPCHK(hipStreamSynchronize(sa->q.stream));
		if (meta.valid) {
			if ((rc = launch_snapshot(sa, sa->snap_lit, 0u, 1, 0))) return rc;
			HIPCHK(hipStreamSynchronize(sa->q.stream));
			return MGL_OK;
		}
	}
	hipLaunchKernelGGL(k_fill_literal, dim3(1024), dim3(256), 0, sa->q.stream, sa->base.v.slab, sa->ctx.n);
	HIPCHK(hipGetLastError());
	if ((rc = rebuild_base(sa, 0))) return rc;
	if (snaps && (rc = launch_snapshot(sa, sa->snap_lit, 0u, 0, 0))) return rc;
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	return MGL_OK;
}

/* A slab from outside has just been refused as the current one (megalania_hip.h, "after a refusal"): the handle goes on
 * from the all-literal slab with clear flags, as after mgl_sa_begin_epoch(phase, 0) -- not from a slab that is no parse.
 * forget_best: the refused slab was the best one, which is then none (cost 0, all-literal entries).  The refusal's text
 * stays the last error. */
static int recover_from_refusal(mgl_sa* sa, bool forget_best)
{
	const std::string keep = g_err;
	Control c;
	int rc = read_ctl(sa, sa->base, &c);
	if (rc) return rc;
	c.cur_cost = 0; c.accepted_flag = 0; c.copy_best_flag = 0; c.error_flags = 0;
	if (forget_best) {
		c.best_cost = 0; c.best_is_current = 0;
		sa->best_unverified = false;
		hipLaunchKernelGGL(k_fill_literal, dim3(1024), dim3(256), 0, sa->q.stream, sa->d_best, sa->ctx.n);
		HIPCHK(hipGetLastError());
		if (sa->d_snap_meta) HIPCHK(hipMemsetAsync(sa->d_snap_meta + 1, 0, sizeof(SnapMeta), sa->q.stream));
	}
	if ((rc = write_ctl(sa, sa->base, &c))) return rc;
	sa->autoacc.reset();
	if ((rc = current_to_literal(sa))) return rc;
	g_err = keep;
	return MGL_OK;
}

/* The current slab is replaced by what `put` leaves in base.v.slab (an import, a kernel launch, a device copy): the best
 * slab's structures are saved if the base is their only holder, MGL_ACCEPT_AUTO starts over, the current cost and the
 * flags are cleared and the base is rebuilt; then check_current.  A slab from outside (`validate`) that is refused does
 * not stay: recover_from_refusal, and the best slab is as it was. */
template <class Put>
static int replace_current(mgl_sa* sa, Put put, bool validate, int bad, const char* who, uint64_t* cost = nullptr)
{
	Control c;
	int rc = read_ctl(sa, sa->base, &c);
	if (rc) return rc;
	if ((rc = keep_best_before_overwrite(sa, c))) return rc;
	sa->autoacc.reset();
	sa->live.stale = true; /* live weights: the next step refreshes them */
	if ((rc = put())) return rc;
	c.cur_cost = 0; c.accepted_flag = 0; c.copy_best_flag = 0; c.error_flags = 0;
	if ((rc = write_ctl(sa, sa->base, &c))) return rc;
	if ((rc = rebuild_base(sa, 0))) return rc;
	rc = check_current(sa, validate, bad, who, cost);
	if (rc == bad && validate) {
		const int rc2 = recover_from_refusal(sa, false);
		if (rc2) return rc2;
	}
	return rc;
}
/* put: a copy of a slab on the device */
static auto put_slab(mgl_sa* sa, const mgl_pk* slab)
{
	return [=]() -> int {
		HIPCHK(hipMemcpyAsync(sa->base.v.slab, slab, sizeof(mgl_pk) * sa->n, hipMemcpyDeviceToDevice, sa->q.stream));
		return MGL_OK;
	};
}

extern "C" int mgl_sa_begin_epoch(mgl_sa* sa, unsigned phase, int from_best)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	HIPCHK(hipSetDevice(sa->device));
	Control c;
	int rc = read_ctl(sa, sa->base, &c);
	if (rc) return rc;
	if (from_best && c.best_cost == 0) from_best = 0; /* no best yet: packets_best is still the all-literal slab */
	sa->live.stale = true; /* live weights: the next step refreshes them */
	const bool snaps = sa->incremental && sa->snapshots;
	const bool base_is_best = snaps && c.best_is_current;
	if (!from_best && (rc = keep_best_before_overwrite(sa, c))) return rc;
	c.iter = 0; c.cur_cost = 0; c.phase = phase; c.accepted_flag = 0; c.copy_best_flag = 0;
	if ((rc = write_ctl(sa, sa->base, &c))) return rc;
	/* MGL_ACCEPT_AUTO starts every epoch the same way, whatever the previous one left behind: a fresh block, bulk steps
	 * first from the all-literal slab (thousands of improving neighbours), single steps first from the best slab */
	sa->autoacc.reset();
	sa->autoacc.bulk_now = !from_best;
	if (from_best && base_is_best) return MGL_OK; /* main.c:73-76 would copy packets_best over itself */
	if (!from_best) return current_to_literal(sa);
	if (snaps) {
		SnapMeta meta;
		HIPCHK(hipMemcpyAsync(&meta, sa->d_snap_meta + 1, sizeof meta, hipMemcpyDeviceToHost, sa->q.stream));
		HIPCHK(hipStreamSynchronize(sa->q.stream));
		if (meta.valid) {
			if ((rc = launch_snapshot(sa, sa->snap_best, 1u, 1, 0))) return rc;
			HIPCHK(hipStreamSynchronize(sa->q.stream));
			return MGL_OK;
		}
	}
	HIPCHK(hipMemcpyAsync(sa->base.v.slab, sa->d_best, sizeof(mgl_pk) * (size_t)sa->n, hipMemcpyDeviceToDevice, sa->q.stream));
	if ((rc = rebuild_base(sa, 0))) return rc;
	if (sa->best_unverified) {
		/* a best slab that came from outside (another chain, mgl_sa_set_best) is checked here, where it first matters:
		 * every packet against the input, and the total against the cost it came with */
		if ((rc = launch_validate(sa))) return rc;
		Control v;
		if ((rc = read_ctl(sa, sa->base, &v))) return rc;
		if (v.error_flags || v.rebuild_cost != v.best_cost) {
			(void)fail(MGL_EINVAL, "mgl_sa_begin_epoch: the adopted best slab is not a valid parse of the input at the cost it came with");
			if ((rc = recover_from_refusal(sa, true))) return rc;
			sa->autoacc.bulk_now = true; /* the epoch starts from the all-literal slab after all */
			return MGL_EINVAL;
		}
		sa->best_unverified = false;
	}
	/* the base now is the best slab's: keep it for the next epoch */
	if (snaps && (rc = launch_snapshot(sa, sa->snap_best, 1u, 0, 0))) return rc;
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	return MGL_OK;
}

extern "C" int mgl_sa_set_slab(mgl_sa* sa, const mgl_packet* packets)
{
	if (!sa || !packets) return fail(MGL_EINVAL, "null argument");
	HIPCHK(hipSetDevice(sa->device));
	return replace_current(sa, [=] { return import_slab(sa, packets, sa->base.v.slab); }, true, MGL_EINVAL, "mgl_sa_set_slab");
}

extern "C" int mgl_sa_set_temperature(mgl_sa* sa, uint64_t temperature)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	if (temperature >> 40) return fail(MGL_EINVAL, "mgl_sa_set_temperature: temperature must be below 2^40 cost units");
	sa->temperature = temperature;
	return MGL_OK;
}

extern "C" int mgl_sa_seed_greedy(mgl_sa* sa, uint32_t candidates)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	if (candidates == 0) return fail(MGL_EINVAL, "mgl_sa_seed_greedy: candidates must be > 0");
	HIPCHK(hipSetDevice(sa->device));
	const auto put = [=]() -> int {
		hipLaunchKernelGGL(k_greedy_seed, dim3((sa->ctx.n + 255u) / 256u), dim3(256), 0, sa->q.stream, sa->ctx, sa->base.v.slab, candidates);
		HIPCHK(hipGetLastError());
		return MGL_OK;
	};
	return replace_current(sa, put, false, MGL_EDEVICE, "mgl_sa_seed_greedy");
}

/* ---- optimal-parse seed (mgl_optimal.hip) */
static int scratch_walk(mgl_sa* sa, const mgl_packet* packets, bool want_cum, bool want_probs, Control* out);
#define MGL_OPT_DEF_PASSES 3u
#define MGL_OPT_DEF_CAND 16u
#define MGL_OPT_DEF_CHUNK 4096u
struct OptBufs {
	DevOwner own; /* the call's temporaries: gone with it */
	uint32_t *counts = nullptr, *prices = nullptr, *entry = nullptr;
	mgl_pk *back = nullptr, *dp = nullptr, *res = nullptr, *keep = nullptr;
	unsigned long long* obj = nullptr;
};
static int opt_alloc(mgl_sa* sa, OptBufs& o, uint32_t chunk, bool seed)
{
	const size_t n = sa->n, total = sa->ctx.L.total, nch = (n + chunk - 1) / chunk;
	TRY(dnew(o.own, o.counts, 2 * total));
	TRY(dnew(o.own, o.prices, 2 * total));
	TRY(dnew(o.own, o.back, n + 1));
	TRY(dnew(o.own, o.dp, n));
	TRY(dnew(o.own, o.obj, 1));
	if (seed) {
		TRY(dnew(o.own, o.entry, 5 * nch));
		TRY(dnew(o.own, o.res, n));
		TRY(dnew(o.own, o.keep, n));
	}
	return MGL_OK;
}
/* prices of the parse on `slab` (a valid parse) */
static int opt_prices(mgl_sa* sa, OptBufs& o, const mgl_pk* slab)
{
	const uint32_t total = sa->ctx.L.total;
	HIPCHK(hipMemsetAsync(o.counts, 0, sizeof(uint32_t) * 2 * total, sa->q.stream));
	hipLaunchKernelGGL(k_opt_walk, dim3(1), dim3(64), 0, sa->q.stream, sa->ctx, slab, (mgl_pk*)nullptr, o.counts, 0, 1u, (uint32_t*)nullptr);
	hipLaunchKernelGGL(k_opt_prices, dim3((total + 255) / 256), dim3(256), 0, sa->q.stream, (const uint32_t*)o.counts, sa->ctx.cost_tbl, total, o.prices);
	HIPCHK(hipGetLastError());
	return MGL_OK;
}
/* ---- the parses' match lists (mgl_matchfinder.hip) */
struct MfTmp {
	DevOwner own;
	uint4* queue = nullptr;
	uint32_t* qcount = nullptr;
	hipEvent_t t0 = nullptr, t1 = nullptr;
};
/* the handle holds the lists of depth `depth` afterwards */
static int mf_ensure(mgl_sa* sa, uint32_t depth)
{
	if (sa->mf_built == depth) return MGL_OK;
	const uint32_t n = (uint32_t)sa->n;
	sa->own.release(sa->d_mf_off); sa->own.release(sa->d_mf_src); sa->own.release(sa->d_mf_len); /* another depth's */
	sa->d_mf_off = nullptr; sa->d_mf_src = nullptr; sa->d_mf_len = nullptr;
	sa->mf_built = 0; sa->mf_total = 0;
	MfTmp t;
	TRY(dnew(sa->own, sa->d_mf_off, (size_t)n + 1));
	TRY(dnew(t.own, t.queue, n));
	TRY(dnew(t.own, t.qcount, 1));
	HIPCHK(t.own.event(&t.t0));
	HIPCHK(t.own.event(&t.t1));
	const dim3 g_direct(n / 256u + 1u); /* n + 1 lanes: off[n] */
	HIPCHK(hipEventRecord(t.t0, sa->q.stream));
	HIPCHK(hipMemsetAsync(t.qcount, 0, sizeof(uint32_t), sa->q.stream));
	hipLaunchKernelGGL(k_mf_direct<false>, g_direct, dim3(256), 0, sa->q.stream, sa->ctx, sa->d_mf_off, (uint32_t*)nullptr, (uint16_t*)nullptr, t.queue, t.qcount);
	uint32_t queued = 0;
	HIPCHK(hipMemcpyAsync(&queued, t.qcount, sizeof queued, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	if (queued > n) return fail(MGL_EDEVICE, "match finder: the scan queue overran");
	const dim3 g_scan((queued + 3u) / 4u);
	if (queued) hipLaunchKernelGGL(k_mf_scan<false>, g_scan, dim3(256), 0, sa->q.stream, sa->ctx, depth, sa->d_mf_off, (uint32_t*)nullptr, (uint16_t*)nullptr,
	                               (const uint4*)t.queue, (const uint32_t*)t.qcount);
	hipLaunchKernelGGL(ix_scan, dim3(1), dim3(1024), 0, sa->q.stream, sa->d_mf_off, n + 1u);
	uint32_t total = 0;
	HIPCHK(hipMemcpyAsync(&total, sa->d_mf_off + n, sizeof total, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	if ((uint64_t)total > (uint64_t)MGL_MF_MAX_ENTRIES * n) return fail(MGL_EDEVICE, "match finder: the list lengths do not add up");
	TRY(dnew(sa->own, sa->d_mf_src, (size_t)total + 1));
	TRY(dnew(sa->own, sa->d_mf_len, (size_t)total + 1));
	hipLaunchKernelGGL(k_mf_direct<true>, g_direct, dim3(256), 0, sa->q.stream, sa->ctx, sa->d_mf_off, sa->d_mf_src, sa->d_mf_len, t.queue, t.qcount);
	if (queued) hipLaunchKernelGGL(k_mf_scan<true>, g_scan, dim3(256), 0, sa->q.stream, sa->ctx, depth, sa->d_mf_off, sa->d_mf_src, sa->d_mf_len,
	                               (const uint4*)t.queue, (const uint32_t*)t.qcount);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(t.t1, sa->q.stream));
	HIPCHK(hipEventSynchronize(t.t1));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, t.t0, t.t1));
	sa->mf_ms = ms; sa->mf_total = total; sa->mf_built = depth;
	return MGL_OK;
}
static MfLists mf_lists(const mgl_sa* sa) { return MfLists{ sa->d_mf_off, sa->d_mf_src, sa->d_mf_len }; }

extern "C" int mgl_sa_set_match_finder(mgl_sa* sa, int finder, uint32_t depth)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	if (finder != MGL_MF_NEAREST && finder != MGL_MF_FRONTIER) return fail(MGL_EINVAL, "mgl_sa_set_match_finder: unknown finder");
	if (depth > MGL_MF_MAX_DEPTH) return fail(MGL_EINVAL, "mgl_sa_set_match_finder: depth must be at most 4096");
	sa->mf_finder = finder;
	sa->mf_depth = depth ? depth : MGL_MF_DEF_DEPTH;
	return MGL_OK;
}

extern "C" int mgl_match_frontier(mgl_sa* sa, uint32_t depth, uint32_t* off_out, uint32_t* src_out, uint16_t* len_out, size_t cap,
                                  size_t* count, double* gpu_ms)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	if (depth > MGL_MF_MAX_DEPTH) return fail(MGL_EINVAL, "mgl_match_frontier: depth must be at most 4096");
	HIPCHK(hipSetDevice(sa->device));
	int rc = mf_ensure(sa, depth ? depth : MGL_MF_DEF_DEPTH);
	if (rc) return rc;
	if (count) *count = sa->mf_total;
	if (gpu_ms) *gpu_ms = sa->mf_ms;
	if (cap < sa->mf_total) return fail(MGL_ERANGE, "mgl_match_frontier: cap is below the number of entries");
	if (off_out) HIPCHK(hipMemcpyAsync(off_out, sa->d_mf_off, sizeof(uint32_t) * ((size_t)sa->n + 1), hipMemcpyDeviceToHost, sa->q.stream));
	if (src_out && sa->mf_total) HIPCHK(hipMemcpyAsync(src_out, sa->d_mf_src, sizeof(uint32_t) * sa->mf_total, hipMemcpyDeviceToHost, sa->q.stream));
	if (len_out && sa->mf_total) HIPCHK(hipMemcpyAsync(len_out, sa->d_mf_len, sizeof(uint16_t) * sa->mf_total, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	return MGL_OK;
}

/* one DP pass into o.dp (entry == nullptr: the LZMA initial state at every chunk start) */
static int opt_dp(mgl_sa* sa, OptBufs& o, const uint32_t* entry, uint32_t cand, uint32_t chunk)
{
	const uint32_t nch = (uint32_t)((sa->n + chunk - 1) / chunk);
	const bool mf = sa->mf_finder == MGL_MF_FRONTIER;
	if (mf) { int rc = mf_ensure(sa, sa->mf_depth); if (rc) return rc; }
	hipLaunchKernelGGL(k_fill_literal, dim3(1024), dim3(256), 0, sa->q.stream, o.dp, (uint32_t)sa->n);
	HIPCHK(hipMemsetAsync(o.obj, 0, sizeof(unsigned long long), sa->q.stream));
	if (mf) hipLaunchKernelGGL(k_opt_dp<true>, dim3(nch), dim3(64), 0, sa->q.stream, sa->ctx, (const uint32_t*)o.prices, entry, chunk, cand, o.back, o.dp, o.obj, mf_lists(sa));
	else hipLaunchKernelGGL(k_opt_dp<false>, dim3(nch), dim3(64), 0, sa->q.stream, sa->ctx, (const uint32_t*)o.prices, entry, chunk, cand, o.back, o.dp, o.obj, MfLists{});
	HIPCHK(hipGetLastError());
	return MGL_OK;
}
static int opt_args(uint32_t cand, uint32_t chunk)
{
	if (cand == 0 || cand > MGL_OPT_MAX_CAND) return fail(MGL_EINVAL, "optimal parse: cand must be 1..30");
	if (chunk < MGL_OPT_MIN_CHUNK) return fail(MGL_EINVAL, "optimal parse: chunk must be at least 512 bytes");
	return MGL_OK;
}

extern "C" int mgl_optimal_pass(mgl_sa* sa, const uint32_t* prices, size_t nprices, uint32_t cand, uint32_t chunk,
                                mgl_packet* packets_out, uint64_t* objective)
{
	if (!sa || !prices || !packets_out) return fail(MGL_EINVAL, "null argument");
	int rc = opt_args(cand, chunk);
	if (rc) return rc;
	if (nprices != 2 * (size_t)sa->ctx.L.total) return fail(MGL_EINVAL, "mgl_optimal_pass: nprices must be 2 x the number of probabilities");
	for (size_t k = 0; k < nprices; k++)
		if (prices[k] > 0xFFFFu) return fail(MGL_EINVAL, "mgl_optimal_pass: a price is above 65535 cost units");
	HIPCHK(hipSetDevice(sa->device));
	OptBufs o;
	if ((rc = opt_alloc(sa, o, chunk, false))) return rc;
	HIPCHK(hipMemcpyAsync(o.prices, prices, sizeof(uint32_t) * nprices, hipMemcpyHostToDevice, sa->q.stream));
	if ((rc = opt_dp(sa, o, nullptr, cand, chunk))) return rc;
	unsigned long long obj = 0;
	HIPCHK(hipMemcpyAsync(&obj, o.obj, sizeof obj, hipMemcpyDeviceToHost, sa->q.stream));
	if ((rc = export_slab(sa, o.dp, packets_out))) return rc;
	if (objective) *objective = obj;
	return MGL_OK;
}

extern "C" int mgl_optimal_prices(mgl_sa* sa, const mgl_packet* packets, uint32_t* prices_out, size_t nprices)
{
	if (!sa || !packets || !prices_out) return fail(MGL_EINVAL, "null argument");
	if (nprices < 2 * (size_t)sa->ctx.L.total) return fail(MGL_ERANGE, "prices_out too small");
	HIPCHK(hipSetDevice(sa->device));
	Control c;
	int rc = scratch_walk(sa, packets, false, false, &c); /* validates the slab */
	if (rc) return rc;
	OptBufs o;
	if ((rc = opt_alloc(sa, o, MGL_OPT_DEF_CHUNK, false))) return rc;
	if ((rc = opt_prices(sa, o, sa->scratch.v.slab))) return rc;
	HIPCHK(hipMemcpyAsync(prices_out, o.prices, sizeof(uint32_t) * 2 * sa->ctx.L.total, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	return MGL_OK;
}

extern "C" int mgl_sa_seed_optimal(mgl_sa* sa, const mgl_optimal_config* cfg, mgl_optimal_stats* stats)
{
	static const char* who = "mgl_sa_seed_optimal";
	if (!sa) return fail(MGL_EINVAL, "null handle");
	const uint32_t passes = cfg && cfg->passes ? cfg->passes : MGL_OPT_DEF_PASSES;
	const uint32_t cand = cfg && cfg->cand ? cfg->cand : MGL_OPT_DEF_CAND;
	const uint32_t chunk = cfg && cfg->chunk ? cfg->chunk : MGL_OPT_DEF_CHUNK;
	int rc = opt_args(cand, chunk);
	if (rc) return rc;
	if (passes > MGL_OPT_MAX_PASSES) return fail(MGL_EINVAL, "mgl_sa_seed_optimal: at most 16 passes");
	HIPCHK(hipSetDevice(sa->device));
	mgl_optimal_stats st;
	memset(&st, 0, sizeof st);
	OptBufs o;
	if ((rc = opt_alloc(sa, o, chunk, true))) return rc;
	const uint32_t n = (uint32_t)sa->n;
	/* pass 0's prices: the greedy parse.  It and every pass's parse become the current slab in turn: the base's rebuild is
	 * what costs them */
	hipLaunchKernelGGL(k_greedy_seed, dim3((n + 255u) / 256u), dim3(256), 0, sa->q.stream, sa->ctx, o.res, cand);
	HIPCHK(hipGetLastError());
	if ((rc = replace_current(sa, put_slab(sa, o.res), false, MGL_EDEVICE, who, &st.greedy_cost))) return rc;
	if ((rc = opt_prices(sa, o, o.res))) return rc;
	hipEvent_t t0, t1;
	HIPCHK(o.own.event(&t0));
	HIPCHK(o.own.event(&t1));
	uint64_t best = ~0ull;
	for (uint32_t p = 0; p < passes && rc == MGL_OK; p++) {
		if (hipEventRecord(t0, sa->q.stream) != hipSuccess) { rc = fail(MGL_EDEVICE, "hipEventRecord"); break; }
		if ((rc = opt_dp(sa, o, p ? o.entry : nullptr, cand, chunk))) break;
		hipLaunchKernelGGL(k_fill_literal, dim3(1024), dim3(256), 0, sa->q.stream, o.res, n);
		HIPCHK(hipMemsetAsync(o.counts, 0, sizeof(uint32_t) * 2 * sa->ctx.L.total, sa->q.stream));
		hipLaunchKernelGGL(k_opt_walk, dim3(1), dim3(64), 0, sa->q.stream, sa->ctx, (const mgl_pk*)o.dp, o.res, o.counts, 1, chunk, o.entry);
		hipLaunchKernelGGL(k_opt_prices, dim3((sa->ctx.L.total + 255) / 256), dim3(256), 0, sa->q.stream, (const uint32_t*)o.counts, sa->ctx.cost_tbl,
		                   sa->ctx.L.total, o.prices);
		if ((rc = replace_current(sa, put_slab(sa, o.res), false, MGL_EDEVICE, who, &st.cost[p]))) break;
		unsigned long long obj = 0;
		HIPCHK(hipMemcpyAsync(&obj, o.obj, sizeof obj, hipMemcpyDeviceToHost, sa->q.stream));
		float ms = 0;
		HIPCHK(hipEventRecord(t1, sa->q.stream));
		HIPCHK(hipEventSynchronize(t1));
		st.objective[p] = obj;
		HIPCHK(hipEventElapsedTime(&ms, t0, t1));
		st.ms[p] = ms;
		st.passes = p + 1;
		if (st.cost[p] < best) {
			best = st.cost[p]; st.best_pass = p;
			HIPCHK(hipMemcpyAsync(o.keep, o.res, sizeof(mgl_pk) * n, hipMemcpyDeviceToDevice, sa->q.stream));
		}
	}
	if (rc) return rc;
	/* the cheapest pass stays current (the last one already is), validated */
	if (st.best_pass + 1 != st.passes) rc = replace_current(sa, put_slab(sa, o.keep), true, MGL_EDEVICE, who, &best);
	else rc = check_current(sa, true, MGL_EDEVICE, who, nullptr);
	if (rc) return rc;
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	if (stats) *stats = st;
	return MGL_OK;
}

/* ---- adaptive-price optimal parse (mgl_adaptive.hip): a batch of variants of the settings through one launch per stage.
 * mgl_sa_seed_sweep keeps the cheapest parse as the current slab; mgl_parse_sweep_props gives every variant a triple of its
 * own and hands the cheapest parse out; mgl_sa_seed_adaptive and mgl_adaptive_pass are a batch of one.  The stages below work
 * on one Parse each, in the order they stand in. */
#define MGL_ADP_DEF_SEGMENT 64u
#define MGL_ADP_DEF_AHEAD 128u
struct Parse {
	/* settings (parse_args) */
	uint32_t nv = 0, passes = 0, chunk = 0, depth = 0, nch = 0, ncand = 0, nnear = 0, nfront = 0, lds_near = 0, lds_front = 0;
	bool from_current = false;
	size_t snap_total = 0;
	AdpVariant h_tab[MGL_SWEEP_MAX];
	uint32_t h_lists[MGL_SWEEP_MAX], cand_idx[MGL_SWEEP_MAX], cands[MGL_SWEEP_MAX]; /* variants by finder; a variant's cand among the distinct ones */
	/* device buffers and events (parse_alloc) */
	uint16_t* snaps = nullptr;
	uint32_t *entry = nullptr, *lists = nullptr, *start_idx = nullptr;
	mgl_pk *back = nullptr, *dp = nullptr, *res = nullptr, *keep = nullptr;
	unsigned long long* obj = nullptr;
	uint64_t* cost = nullptr;
	AdpVariant* tab = nullptr;
	hipEvent_t t0 = nullptr, t1 = nullptr, call0 = nullptr, fork = nullptr, join = nullptr;
	/* results: the last walk's costs and the last DP's objectives, per variant; the stats; the best parse so far */
	uint64_t h_cost[MGL_SWEEP_MAX], vbest[MGL_SWEEP_MAX], best = ~0ull;
	unsigned long long h_obj[MGL_SWEEP_MAX];
	float ms = 0;
	uint32_t best_v = UINT32_MAX;
	std::vector<mgl_optimal_stats> st;
	DevOwner own; /* of the device buffers and events */
};

/* checks and defaults; a chunk or a segment longer than the input acts like one of its length */
static int adp_args(const mgl_sa* sa, uint32_t cand, uint32_t& chunk, uint32_t& segment, uint32_t& ahead, bool ahead_given)
{
	int rc = opt_args(cand, chunk);
	if (rc) return rc;
	if (ahead > MGL_MAX_MATCH) return fail(MGL_EINVAL, "adaptive parse: ahead must be at most 273");
	if (segment == 0) { segment = MGL_ADP_DEF_SEGMENT; if (!ahead_given) ahead = MGL_ADP_DEF_AHEAD; }
	const uint32_t n = (uint32_t)sa->n;
	if (chunk > n) chunk = n > MGL_OPT_MIN_CHUNK ? n : MGL_OPT_MIN_CHUNK;
	if (segment > chunk) segment = chunk;
	return MGL_OK;
}

/* Argument checks and the variant table: per variant its settings after the defaults and clamps, its triple (props[v], or the
 * handle's) and where its snapshots lie; the variants listed by finder; the distinct cands. */
static int parse_args(const mgl_sa* sa, Parse& P, uint32_t passes, uint32_t chunk, uint32_t depth, bool from_current, bool ahead_given,
                      const mgl_parse_variant* variants, const mgl_properties* props, size_t nvariants)
{
	if (nvariants == 0 || nvariants > MGL_SWEEP_MAX) return fail(MGL_EINVAL, "parse sweep: 1 to 64 variants");
	if (props && from_current) return fail(MGL_EINVAL, "mgl_parse_sweep_props: a current slab has a cost under one triple only; from_current must be 0");
	if (passes > MGL_OPT_MAX_PASSES) return fail(MGL_EINVAL, "adaptive parse: at most 16 passes");
	if (depth > MGL_MF_MAX_DEPTH) return fail(MGL_EINVAL, "parse sweep: depth must be at most 4096");
	P.nv = (uint32_t)nvariants; P.passes = passes; P.depth = depth; P.from_current = from_current;
	for (uint32_t v = 0; v < P.nv; v++) {
		if (variants[v].finder != MGL_MF_NEAREST && variants[v].finder != MGL_MF_FRONTIER) return fail(MGL_EINVAL, "parse sweep: unknown finder");
		if (props && ((uint32_t)props[v].lc + props[v].lp > 4u || props[v].pb > 4u))
			return fail(MGL_EINVAL, "mgl_parse_sweep_props: supported properties are lc + lp <= 4, pb <= 4");
		AdpVariant& t = P.h_tab[v];
		t.cand = variants[v].cand ? variants[v].cand : MGL_OPT_DEF_CAND;
		t.segment = variants[v].segment; t.ahead = variants[v].ahead;
		t.props = props ? adp_pack_props(props[v].lc, props[v].lp, props[v].pb) : adp_pack_props(sa->ctx.L.lc, sa->ctx.L.lp, sa->ctx.L.pb);
		P.chunk = chunk; /* clamped the same way for every variant */
		int rc = adp_args(sa, t.cand, P.chunk, t.segment, t.ahead, ahead_given);
		if (rc) return rc;
		uint32_t k = 0;
		while (k < P.ncand && P.cands[k] != t.cand) k++;
		if (k == P.ncand) P.cands[P.ncand++] = t.cand;
		P.cand_idx[v] = k;
		if (variants[v].finder == MGL_MF_NEAREST) P.h_lists[P.nnear++] = v;
	}
	P.nfront = P.nv - P.nnear;
	for (uint32_t v = 0, k = P.nnear; v < P.nv; v++)
		if (variants[v].finder == MGL_MF_FRONTIER) P.h_lists[k++] = v;
	/* a variant's snapshots: nch models of its own layout; a launch's dynamic LDS: the largest model among its variants */
	P.nch = (uint32_t)(((size_t)sa->n + P.chunk - 1) / P.chunk);
	for (uint32_t v = 0; v < P.nv; v++) {
		AdpVariant& t = P.h_tab[v];
		const uint32_t stride = adp_stride(mgl_make_layout(t.props & 0xFFu, (t.props >> 8) & 0xFFu, (t.props >> 16) & 0xFFu));
		t.snap_off = P.snap_total;
		P.snap_total += (size_t)P.nch * stride;
		uint32_t& lds = variants[v].finder == MGL_MF_FRONTIER ? P.lds_front : P.lds_near;
		if (stride * (uint32_t)sizeof(uint16_t) > lds) lds = stride * (uint32_t)sizeof(uint16_t);
	}
	return MGL_OK;
}

/* The buffers, the frontier's lists if a variant asks for them, the tables on the device.  resolved: the passes' parses are
 * resolved (res; pass 0's greedy parses lie there first) and the best is kept (keep).  A buffer that does not fit is
 * MGL_ENOMEM. */
static int parse_alloc(mgl_sa* sa, Parse& P, bool resolved)
{
	static const char* nomem = "adaptive parse: the per-variant buffers do not fit the device";
	const size_t n = sa->n, nv = P.nv;
	if (P.nfront) TRY(mf_ensure(sa, P.depth));
	auto room = [&](auto*& ptr, size_t count) { return dnew(P.own, ptr, count, -1, nomem); };
	TRY(room(P.snaps, P.snap_total));
	TRY(room(P.entry, 5 * P.nch * nv));
	TRY(room(P.back, (n + 1) * nv));
	TRY(room(P.dp, n * nv));
	if (resolved) {
		TRY(room(P.res, n * nv));
		TRY(room(P.keep, n));
	}
	TRY(room(P.obj, nv));
	TRY(room(P.cost, nv));
	TRY(room(P.tab, nv));
	TRY(room(P.lists, nv));
	TRY(room(P.start_idx, nv));
	for (hipEvent_t* e : { &P.t0, &P.t1, &P.call0, &P.fork, &P.join }) HIPCHK(P.own.event(e));
	if (P.nnear) HIPCHK(hipFuncSetAttribute((const void*)k_adp_dp_sweep<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds_near));
	if (P.nfront) HIPCHK(hipFuncSetAttribute((const void*)k_adp_dp_sweep<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds_front));
	HIPCHK(hipEventRecord(P.call0, sa->q.stream));
	HIPCHK(hipMemcpyAsync(P.tab, P.h_tab, sizeof(AdpVariant) * nv, hipMemcpyHostToDevice, sa->q.stream));
	HIPCHK(hipMemcpyAsync(P.lists, P.h_lists, sizeof(uint32_t) * nv, hipMemcpyHostToDevice, sa->q.stream));
	return MGL_OK;
}

/* Pass 0's chunk starts and model snapshots, from the walk of `given` (a valid parse on the device) for every variant, or
 * (nullptr) of one greedy parse per distinct cand.  The walk's cost is the variant's greedy_cost; with from_current it is
 * what the variant, and the batch, have to beat. */
static int parse_starts(mgl_sa* sa, Parse& P, const mgl_pk* given)
{
	const uint32_t n = (uint32_t)sa->n, nv = P.nv;
	uint32_t idx[MGL_SWEEP_MAX];
	for (uint32_t v = 0; v < nv; v++) idx[v] = given ? 0u : P.cand_idx[v];
	HIPCHK(hipMemcpyAsync(P.start_idx, idx, sizeof(uint32_t) * nv, hipMemcpyHostToDevice, sa->q.stream));
	if (!given) {
		for (uint32_t k = 0; k < P.ncand; k++) /* ncand <= nv slabs of res, which no pass has written yet */
			hipLaunchKernelGGL(k_greedy_seed, dim3((n + 255u) / 256u), dim3(256), 0, sa->q.stream, sa->ctx, P.res + (size_t)k * n, P.cands[k]);
		given = P.res;
	}
	hipLaunchKernelGGL(k_adp_snap_sweep, dim3(nv), dim3(64), 0, sa->q.stream, sa->ctx, (const AdpVariant*)P.tab, given, (const uint32_t*)P.start_idx,
	                   (mgl_pk*)nullptr, 0, P.chunk, P.nch, P.entry, P.snaps, P.cost);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(P.h_cost, P.cost, sizeof(uint64_t) * nv, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	P.st.assign(nv, mgl_optimal_stats{});
	for (uint32_t v = 0; v < nv; v++) {
		P.st[v].greedy_cost = P.h_cost[v];
		P.st[v].best_pass = UINT32_MAX;
		P.vbest[v] = P.from_current ? P.h_cost[v] : ~0ull;
	}
	P.best = P.from_current ? P.h_cost[0] : ~0ull;
	return MGL_OK;
}

/* One DP pass from the chunk starts in entry / snaps into dp: one launch, or with both finders present two side by side,
 * the frontier's on the handle's second stream */
static int parse_dp(mgl_sa* sa, Parse& P)
{
	const size_t n = sa->n;
	const bool both = P.nnear && P.nfront;
	HIPCHK(hipEventRecord(P.t0, sa->q.stream));
	hipLaunchKernelGGL(k_fill_literal, dim3(1024), dim3(256), 0, sa->q.stream, P.dp, n * P.nv);
	HIPCHK(hipMemsetAsync(P.obj, 0, sizeof(unsigned long long) * P.nv, sa->q.stream));
	if (both) {
		HIPCHK(hipEventRecord(P.fork, sa->q.stream));
		HIPCHK(hipStreamWaitEvent(sa->q.stream2, P.fork, 0));
	}
	if (P.nfront)
		hipLaunchKernelGGL(k_adp_dp_sweep<true>, dim3(P.nch, P.nfront), dim3(64), P.lds_front, both ? sa->q.stream2 : sa->q.stream, sa->ctx,
		                   (const AdpVariant*)P.tab, (const uint32_t*)P.lists + P.nnear, P.nch, (const uint32_t*)P.entry, (const uint16_t*)P.snaps, P.chunk,
		                   P.back, P.dp, P.obj, mf_lists(sa));
	if (both) HIPCHK(hipEventRecord(P.join, sa->q.stream2));
	if (P.nnear)
		hipLaunchKernelGGL(k_adp_dp_sweep<false>, dim3(P.nch, P.nnear), dim3(64), P.lds_near, sa->q.stream, sa->ctx, (const AdpVariant*)P.tab,
		                   (const uint32_t*)P.lists, P.nch, (const uint32_t*)P.entry, (const uint16_t*)P.snaps, P.chunk, P.back, P.dp, P.obj, MfLists{});
	if (both) HIPCHK(hipStreamWaitEvent(sa->q.stream, P.join, 0));
	HIPCHK(hipGetLastError());
	return MGL_OK;
}

/* Resolve and cost: the serial walk of every variant's dp into res, exactly costed, leaving the next pass's chunk starts
 * (`snaps`: and its model snapshots).  h_cost, h_obj and ms hold the pass afterwards. */
static int parse_resolve(mgl_sa* sa, Parse& P, bool snaps)
{
	const size_t n = sa->n;
	hipLaunchKernelGGL(k_fill_literal, dim3(1024), dim3(256), 0, sa->q.stream, P.res, n * P.nv);
	hipLaunchKernelGGL(k_adp_snap_sweep, dim3(P.nv), dim3(64), 0, sa->q.stream, sa->ctx, (const AdpVariant*)P.tab, (const mgl_pk*)P.dp,
	                   (const uint32_t*)nullptr, P.res, 1, P.chunk, P.nch, P.entry, snaps ? P.snaps : (uint16_t*)nullptr, P.cost);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(P.h_obj, P.obj, sizeof(unsigned long long) * P.nv, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipMemcpyAsync(P.h_cost, P.cost, sizeof(uint64_t) * P.nv, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipEventRecord(P.t1, sa->q.stream));
	HIPCHK(hipEventSynchronize(P.t1));
	HIPCHK(hipEventElapsedTime(&P.ms, P.t0, P.t1));
	return MGL_OK;
}

/* Pass p's figures into the stats, and the cheapest (variant, pass) so far into keep: ties to the lower variant, then to
 * the lower pass; with from_current the current slab holds every tie */
static int parse_keep(mgl_sa* sa, Parse& P, uint32_t p)
{
	uint32_t keep_v = UINT32_MAX;
	for (uint32_t v = 0; v < P.nv; v++) {
		mgl_optimal_stats& s = P.st[v];
		const uint64_t cost = P.h_cost[v];
		s.cost[p] = cost; s.objective[p] = P.h_obj[v]; s.ms[p] = P.ms; s.passes = p + 1;
		if (cost < P.vbest[v]) { P.vbest[v] = cost; s.best_pass = p; }
		if (cost < P.best || (cost == P.best && P.best_v != UINT32_MAX && v < P.best_v)) { P.best = cost; P.best_v = keep_v = v; }
	}
	if (keep_v != UINT32_MAX)
		HIPCHK(hipMemcpyAsync(P.keep, P.res + (size_t)keep_v * sa->n, sizeof(mgl_pk) * sa->n, hipMemcpyDeviceToDevice, sa->q.stream));
	return MGL_OK;
}

/* props == nullptr: every variant under the handle's triple, and the winner becomes the current slab (unless, with
 * from_current, nothing beat it: the handle is left as it is).  Otherwise variant v under props[v]; nothing of the search
 * state is touched and the winner goes to packets_out. */
static int sweep_run(mgl_sa* sa, const char* who, const mgl_parse_sweep_config* cfg, const mgl_parse_variant* variants, const mgl_properties* props,
                     size_t nvariants, mgl_optimal_stats* results, uint32_t* best_variant, mgl_packet* packets_out, double* gpu_ms)
{
	Parse P;
	int rc = parse_args(sa, P, cfg && cfg->passes ? cfg->passes : MGL_OPT_DEF_PASSES, cfg && cfg->chunk ? cfg->chunk : MGL_OPT_DEF_CHUNK,
	                    cfg && cfg->depth ? cfg->depth : sa->mf_depth, cfg && cfg->from_current, false, variants, props, nvariants);
	if (rc) return rc;
	HIPCHK(hipSetDevice(sa->device));
	if ((rc = parse_alloc(sa, P, true))) return rc;
	if ((rc = parse_starts(sa, P, P.from_current ? sa->base.v.slab : nullptr))) return rc;
	for (uint32_t p = 0; p < P.passes; p++) {
		if ((rc = parse_dp(sa, P))) return rc;
		if ((rc = parse_resolve(sa, P, p + 1 < P.passes))) return rc;
		if ((rc = parse_keep(sa, P, p))) return rc;
	}
	if (props) {
		/* the handle cannot cost a slab under a foreign triple: the winner is handed out, not made current */
		if (packets_out && (rc = export_slab(sa, P.keep, packets_out))) return rc;
	} else if (P.best_v != UINT32_MAX) {
		uint64_t built = 0;
		if ((rc = replace_current(sa, put_slab(sa, P.keep), true, MGL_EDEVICE, who, &built))) return rc;
		if (built != P.best) return fail(MGL_EDEVICE, std::string(who) + ": the walk's cost of the seeded slab differs from the rebuild's");
	}
	HIPCHK(hipEventRecord(P.t1, sa->q.stream));
	HIPCHK(hipEventSynchronize(P.t1));
	float call_ms = 0;
	HIPCHK(hipEventElapsedTime(&call_ms, P.call0, P.t1));
	if (results) memcpy(results, P.st.data(), sizeof(mgl_optimal_stats) * P.nv);
	if (best_variant) *best_variant = P.best_v;
	if (gpu_ms) *gpu_ms = call_ms;
	return MGL_OK;
}

extern "C" int mgl_sa_seed_sweep(mgl_sa* sa, const mgl_parse_sweep_config* cfg, const mgl_parse_variant* variants, size_t nvariants,
                                 mgl_optimal_stats* results, uint32_t* best_variant, double* gpu_ms)
{
	if (!sa || !variants) return fail(MGL_EINVAL, "null argument");
	return sweep_run(sa, "mgl_sa_seed_sweep", cfg, variants, nullptr, nvariants, results, best_variant, nullptr, gpu_ms);
}

extern "C" int mgl_parse_sweep_props(mgl_sa* sa, const mgl_parse_sweep_config* cfg, const mgl_parse_variant* variants, const mgl_properties* props,
                                     size_t nvariants, mgl_optimal_stats* results, uint32_t* best_variant, mgl_packet* packets_out, double* gpu_ms)
{
	if (!sa || !variants || !props) return fail(MGL_EINVAL, "null argument");
	return sweep_run(sa, "mgl_parse_sweep_props", cfg, variants, props, nvariants, results, best_variant, packets_out, gpu_ms);
}

/* one variant, with the handle's finder and depth */
extern "C" int mgl_sa_seed_adaptive(mgl_sa* sa, const mgl_adaptive_config* cfg, mgl_optimal_stats* stats)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	const mgl_parse_sweep_config sc = { cfg ? cfg->passes : 0u, cfg ? cfg->chunk : 0u, sa->mf_depth, cfg ? cfg->from_current : 0u };
	const mgl_parse_variant var = { (uint32_t)sa->mf_finder, cfg ? cfg->cand : 0u, cfg ? cfg->segment : 0u, cfg ? cfg->ahead : 0u };
	return sweep_run(sa, "mgl_sa_seed_adaptive", &sc, &var, nullptr, 1, stats, nullptr, nullptr, nullptr);
}

/* one variant and one DP from the starts of the validated scratch slab: neither resolved nor kept */
extern "C" int mgl_adaptive_pass(mgl_sa* sa, const mgl_packet* parse_in, uint32_t cand, uint32_t chunk, uint32_t segment, uint32_t ahead,
                                 mgl_packet* packets_out, uint64_t* objective)
{
	if (!sa || !parse_in || !packets_out) return fail(MGL_EINVAL, "null argument");
	if (cand == 0) return fail(MGL_EINVAL, "optimal parse: cand must be 1..30");
	const mgl_parse_variant var = { (uint32_t)sa->mf_finder, cand, segment, ahead };
	Parse P;
	int rc = parse_args(sa, P, 1, chunk, sa->mf_depth, false, true, &var, nullptr, 1);
	if (rc) return rc;
	HIPCHK(hipSetDevice(sa->device));
	Control c;
	if (scratch_walk(sa, parse_in, false, false, &c)) return fail(MGL_ERANGE, "mgl_adaptive_pass: parse_in is not a valid parse of the input");
	if ((rc = parse_alloc(sa, P, false))) return rc;
	if ((rc = parse_starts(sa, P, sa->scratch.v.slab))) return rc;
	if ((rc = parse_dp(sa, P))) return rc;
	HIPCHK(hipMemcpyAsync(P.h_obj, P.obj, sizeof(unsigned long long), hipMemcpyDeviceToHost, sa->q.stream));
	if ((rc = export_slab(sa, P.dp, packets_out))) return rc;
	if (objective) *objective = P.h_obj[0];
	return MGL_OK;
}

extern "C" int mgl_sa_set_accept_mode(mgl_sa* sa, int mode, uint32_t bulk_threshold)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	if (mode != MGL_ACCEPT_AUTO && mode != MGL_ACCEPT_SINGLE && mode != MGL_ACCEPT_BULK) return fail(MGL_EINVAL, "mgl_sa_set_accept_mode: unknown mode");
	if (mode == MGL_ACCEPT_BULK && !(sa->incremental && sa->parallel_build)) return fail(MGL_EINVAL, "mgl_sa_set_accept_mode: bulk steps need the incremental engine and its parallel builder");
	sa->accept_mode = mode;
	if (bulk_threshold) sa->bulk_threshold = bulk_threshold;
	sa->autoacc.reset();
	return MGL_OK;
}
static int weights_window(mgl_sa* sa);
static int live_refresh(mgl_sa* sa, uint64_t gstep);
/* The focus window: host state only (with target weights in force, also what the window weighs).  Targets that were queued ahead
 * under the old window are made again. */
extern "C" int mgl_sa_set_focus(mgl_sa* sa, uint64_t lo, uint64_t hi)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	if (!sa->d_strat_pre) return fail(MGL_EINVAL, "mgl_sa_set_focus: position targets (MGL_F_POSITION_TARGETS) have no focus window");
	if (hi > sa->n || (lo >= hi && (lo | hi) != 0)) return fail(MGL_EINVAL, "mgl_sa_set_focus: the window must be 0, 0 or lo < hi <= n");
	sa->focus_lo = (uint32_t)lo; sa->focus_hi = (uint32_t)hi;
	if (sa->tgt_ahead != TGT_NONE) sa->tgt_ahead = TGT_STALE;
	if (sa->d_wt) { /* target weights in force: what the new window weighs (weights_window, below) */
		HIPCHK(hipSetDevice(sa->device));
		return weights_window(sa);
	}
	return MGL_OK;
}
extern "C" int mgl_sa_focus(mgl_sa* sa, uint64_t* lo, uint64_t* hi, uint64_t* packets)
{
	if (!sa || !lo || !hi) return fail(MGL_EINVAL, "null argument");
	*lo = sa->focus_lo; *hi = sa->focus_hi;
	if (!packets) return MGL_OK;
	if (!sa->d_strat_pre) return fail(MGL_EINVAL, "mgl_sa_focus: position targets (MGL_F_POSITION_TARGETS) count no packets");
	HIPCHK(hipSetDevice(sa->device));
	const uint64_t* onwalk = sa->incremental ? sa->b2.onwalk : sa->base.v.onwalk;
	const uint32_t nw0 = sa->incremental ? sa->b2.nw0 : (sa->ctx.n + 63u) >> 6;
	hipStream_t st = sa->q.stream;
	HIPCHK(hipStreamSynchronize(sa->q.stream2)); /* targets queued ahead use the same prefix sums */
	hipLaunchKernelGGL(k_rank_blocks, dim3(sa->ctx.strat_nblk), dim3(64), 0, st, onwalk, nw0, sa->d_strat_pre, sa->ctx.strat_nblk);
	hipLaunchKernelGGL(k_rank_scan, dim3(1), dim3(1024), 0, st, sa->d_strat_pre, sa->ctx.strat_nblk);
	hipLaunchKernelGGL(k_focus_count, dim3(1), dim3(64), 0, st, onwalk, nw0, (const uint32_t*)sa->d_strat_pre, sa->focus_lo, sa->focus_hi ? sa->focus_hi : sa->n, sa->d_focus_cnt);
	HIPCHK(hipGetLastError());
	uint32_t v[2] = { 0, 0 };
	HIPCHK(hipMemcpyAsync(v, sa->d_focus_cnt, sizeof v, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	*packets = v[1];
	return MGL_OK;
}
/* pure host arithmetic: chain `rank` of `world` gets slice [B_rank, B_rank+1) of [0, n); even rounds cut at i n / world, odd rounds
 * half a slice further down, so that no boundary stays where it was */
extern "C" int mgl_focus_slice(uint64_t n, uint32_t world, uint32_t rank, uint64_t round, uint64_t* lo, uint64_t* hi)
{
	if (!lo || !hi) return fail(MGL_EINVAL, "null argument");
	if (world == 0 || rank >= world || n < 2ull * world) return fail(MGL_EINVAL, "mgl_focus_slice: needs rank < world and n >= 2 world");
	auto bound = [&](uint64_t i) -> uint64_t {
		if (i == 0) return 0;
		if (i == world) return n;
		return (round & 1u) ? (uint64_t)((unsigned __int128)(2 * i - 1) * n / (2ull * world)) : (uint64_t)((unsigned __int128)i * n / world);
	};
	*lo = bound(rank); *hi = bound(rank + 1ull);
	return MGL_OK;
}
extern "C" int mgl_sa_step_modes(mgl_sa* sa, uint8_t* modes_out, size_t cap, size_t* count)
{
	if (!sa || !count) return fail(MGL_EINVAL, "null argument");
	*count = sa->mode_log.size();
	if (modes_out) memcpy(modes_out, sa->mode_log.data(), cap < sa->mode_log.size() ? cap : sa->mode_log.size());
	return MGL_OK;
}

/* MGL_ACCEPT_AUTO, after a block of steps, from device counters only (reproducible): bulk steps pay while a
 * step offers many improving neighbours AND their windows are short enough for several to be taken at once.
 * From the all-literal slab nothing resets the rep distances, so every window runs to the end of the file
 * and a bulk step takes one move like a single step, at three times the price: then single steps for a while. */
void AutoAccept::decide(bool was_bulk, uint64_t block, uint64_t improving, uint64_t taken, uint32_t bulk_threshold, bool batch_ok)
{
	const bool many = improving >= (uint64_t)bulk_threshold * block;
	if (was_bulk) {
		/* (a bulk step that takes one move is a single step at a higher price: from the all-literal slab, where no window
		 * closes, or once improving neighbours have become rare) */
		if (batch_ok ? 2u * taken < 3u * block : taken < 4u * block) { bulk_now = false; bulk_hold = 48; }
		else bulk_now = many;
		return;
	}
	bulk_hold = bulk_hold > block ? bulk_hold - block : 0;
	bulk_now = many && bulk_hold == 0;
}

static DecideArgs decide_args(const mgl_sa* sa)
{
	DecideArgs a;
	a.K = sa->cfg.neighbours_per_step; a.seed = sa->cfg.seed; a.iters_per_epoch = sa->cfg.iters_per_epoch;
	a.sqrt_thresh = sa->sqrt_thresh; a.temperature = sa->temperature;
	return a;
}
/* what closes a bulk step: best-slab tracking, the step's counters.  `gate` = the batch accept's status word when these
 * are queued before the host has read it (they then run beside the read-back), nullptr when the host knows the step is in */
static void launch_bulk_close(mgl_sa* sa, const BatchHdr* gate)
{
	hipLaunchKernelGGL(k_bulk_finish, dim3(1), dim3(64), 0, sa->q.stream, sa->base.ctl, sa->bulk, sa->snapshots ? 1 : 0,
	                   sa->snapshots ? &sa->d_snap_meta[1].valid : (uint32_t*)nullptr, gate);
	if (sa->snapshots) {
		hipLaunchKernelGGL(k_bulk_keep_copy, dim3(1024), dim3(256), 0, sa->q.stream, (const Control*)sa->base.ctl, (const mgl_pk*)sa->base.v.slab, sa->d_best, sa->ctx.n, gate);
		hipLaunchKernelGGL(k_bulk_keep_undo, dim3(64), dim3(256), 0, sa->q.stream, (const Control*)sa->base.ctl, sa->nbr, sa->bulk, sa->d_best, gate);
	} else {
		hipLaunchKernelGGL(k_bulk_copy_best, dim3(256), dim3(256), 0, sa->q.stream, (const Control*)sa->base.ctl, (const mgl_pk*)sa->base.v.slab, sa->d_best, sa->ctx.n, gate);
	}
	hipLaunchKernelGGL(k_bulk_reset, dim3(1), dim3(64), 0, sa->q.stream, sa->bulk, gate);
	hipLaunchKernelGGL(k_bulk_step_end, dim3(1), dim3(64), 0, sa->q.stream, sa->base.ctl, sa->d_counts, sa->form.form_single ? 1 : 0, gate);
}
/* ---- the tail of a bulk step in stages: launch_bulk_tail calls them in the order they stand in.  All on the main stream. */
/* the selection: which of the step's acceptable neighbours are taken; no waits, no records */
static int bulk_select(mgl_sa* sa)
{
	const uint32_t K = sa->cfg.neighbours_per_step;
	const DecideArgs a = decide_args(sa);
	const uint32_t blocks = (K + 255u) / 256u;
	hipLaunchKernelGGL(k_bulk_prep, dim3(blocks), dim3(256), 0, sa->q.stream, sa->ctx, sa->base.ctl, sa->nbr, a, sa->bulk);
	if (sa->autoacc.select_small) {
		hipLaunchKernelGGL(k_bulk_select_small, dim3(1), dim3(1024), 0, sa->q.stream, sa->base.ctl, sa->nbr, sa->bulk, K);
	} else for (uint32_t r = 0; r < MGL_BULK_ROUNDS; r++) {
		hipLaunchKernelGGL(k_bulk_pairs, dim3(blocks, blocks), dim3(256), 0, sa->q.stream, sa->bulk, K, r);
		hipLaunchKernelGGL(k_bulk_round, dim3(blocks), dim3(256), 0, sa->q.stream, sa->base.ctl, sa->nbr, sa->bulk, sa->base.v.slab, K, r);
	}
	hipLaunchKernelGGL(k_bulk_end, dim3(1), dim3(64), 0, sa->q.stream, sa->base.ctl, sa->bulk, a);
	HIPCHK(hipGetLastError());
	return MGL_OK;
}
/* A step that took few moves patches the base structures for all of them at once (mgl_kernels5.hip); every kernel of
 * that looks at the status word first, so a step that took none, or too many, passes through in a few microseconds.
 * Queues the batch accept (the next step's targets ahead behind its second pb_levels: launch_targets_ahead), the copy of
 * the status words to pinned memory, ev_bstat behind it and the closing kernels behind the gate; waits for ev_bstat on the
 * host.  bstat = the status words; *closed = the closing kernels are queued and the gate is open. */
static int bulk_batch_accept(mgl_sa* sa, uint64_t next_gstep, BatchHdr* bstat, bool* closed)
{
	Base2& b = sa->b2;
	hipStream_t st = sa->q.stream;
	if (sa->force.batch_fail) { /* give up at the top of k_batch_chains, or behind the n-th context's rewrite */
		const uint32_t early = sa->force.batch_late ? 0u : 1u, late = sa->force.batch_late;
		HIPCHK(hipMemcpyAsync(&sa->batch.hdr->force_early, &early, sizeof early, hipMemcpyHostToDevice, st));
		HIPCHK(hipMemcpyAsync(&sa->batch.hdr->force_late, &late, sizeof late, hipMemcpyHostToDevice, st));
	}
	const BatchBuf bt = accept_bt(sa);
	const ApplyBuf ab = accept_ab(sa);
	hipLaunchKernelGGL(k_batch_clusters, dim3(1), dim3(1024), 0, st, sa->ctx, (const Control*)sa->base.ctl, sa->nbr, sa->bulk, sa->batch, sa->lim);
	hipLaunchKernelGGL(k_batch_walk, dim3(MGL_BATCH_MAX), dim3(64), 0, st, sa->ctx, b, sa->batch, sa->lim);
	hipLaunchKernelGGL(k_batch_commit, dim3(MGL_BATCH_MAX), dim3(256), 0, st, sa->ctx, b, sa->base.ctl, sa->batch, sa->ab);
	hipLaunchKernelGGL(pb_levels, dim3((b.nw0 + 255) / 256), dim3(256), 0, st, (const uint64_t*)b.sp0, b.sp1, b.nw0, b.nw1);
	hipLaunchKernelGGL(pb_levels, dim3((b.nw1 + 255) / 256), dim3(256), 0, st, (const uint64_t*)b.sp1, b.sp2, b.nw1, b.nw2);
	/* the bitmaps are the new base's from here on -- if the batch accept goes through, which the status read below says */
	if (next_gstep != ~0ull) TRY(launch_targets_ahead(sa, next_gstep));
	hipLaunchKernelGGL(k_batch_scan, dim3(1), dim3(1024), 0, st, sa->batch, sa->ab);
	hipLaunchKernelGGL(k_batch_fill, dim3(256), dim3(256), 0, st, sa->batch, sa->ab);
	hipLaunchKernelGGL(k_batch_chains, dim3(MGL_BATCH_GRID), dim3(MGL_BATCH_THREADS), 0, st, sa->ctx, accept_b2(sa), sa->base.ctl, bt, ab, sa->lim);
	hipLaunchKernelGGL(k_batch_ckpt, dim3(1024, 8), dim3(256), 0, st, b, (const Control*)sa->base.ctl, bt, ab);
	hipLaunchKernelGGL(k_apply_jobs, dim3(1024), dim3(256), 0, st, b, (const Control*)sa->base.ctl, sa->ab, 0, (const BatchHdr*)sa->batch.hdr);
	hipLaunchKernelGGL(k_apply_jobs, dim3(1024), dim3(256), 0, st, b, (const Control*)sa->base.ctl, sa->ab, 1, (const BatchHdr*)sa->batch.hdr);
	hipLaunchKernelGGL(k_batch_end, dim3(1), dim3(64), 0, st, sa->base.ctl, sa->batch);
	HIPCHK(hipGetLastError());
	const size_t read_back = offsetof(BatchHdr, acceptable) + sizeof sa->h_bstat->acceptable; /* status .. acceptable */
	HIPCHK(hipMemcpyAsync(sa->h_bstat, sa->batch.hdr, read_back, hipMemcpyDeviceToHost, st)); /* pinned: no staging copy */
	HIPCHK(hipEventRecord(sa->q.ev_bstat, st));
	launch_bulk_close(sa, (const BatchHdr*)sa->batch.hdr); /* behind the gate: they run while the host reads the status */
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventSynchronize(sa->q.ev_bstat));
	memcpy(bstat, sa->h_bstat, read_back);
	*closed = bstat->status == MGL_BATCH_DONE || bstat->status == MGL_BATCH_NONE;
	if (!*closed && sa->tgt_ahead != TGT_NONE) sa->tgt_ahead = TGT_STALE; /* the step goes to the rebuild (or was never committed): the targets are made again */
	if (sa->force.batch_fail) {
		const uint32_t zero = 0u;
		HIPCHK(hipMemcpy(&sa->batch.hdr->force_early, &zero, sizeof zero, hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(&sa->batch.hdr->force_late, &zero, sizeof zero, hipMemcpyHostToDevice));
		/* a step that took nothing, or went to the rebuild anyway, does not count; a batch accept the hook was applied to does,
		 * whether it gave up or (late form with n above the contexts that got that far) went through: the hook never stays
		 * armed with a stale n */
		if ((bstat->status == MGL_BATCH_BEGAN || bstat->status == MGL_BATCH_DONE) && --sa->force.batch_fail == 0) sa->force.batch_late = 0;
	}
	return MGL_OK;
}
/* The rebuild's: the journals into the slab (unless the batch accept got as far as writing them: MGL_BATCH_BEGAN = it gave
 * up behind its commit), everything that hangs off the slab re-derived, the parse checked after the fact (soft window
 * ends rest on an argument about rep distances, not on a proof for every coincidence of values): every packet of
 * the new parse against the input; a parse that fails is taken back as a whole.  One small read-back per bulk
 * step (a bulk step of this kind is a rebuild: milliseconds).  The validation runs on the second stream between ev_fork
 * and ev_val (launch_pbuild); the host waits for the main stream at every read-back. */
static int bulk_rebuild_checked(mgl_sa* sa, const BatchHdr& bstat)
{
	const bool gave_up_late = sa->batch_ok && bstat.status == MGL_BATCH_BEGAN;
	if (gave_up_late) sa->batch_fallbacks++;
	if (sa->batch_ok && bstat.status == MGL_BATCH_REBUILD && bstat.failed) sa->batch_early_giveups++; /* (MGL_BATCH_REBUILD without it: more moves than a batch accept handles) */
	if (bstat.status != MGL_BATCH_BEGAN)
		hipLaunchKernelGGL(k_bulk_write, dim3(64), dim3(256), 0, sa->q.stream, sa->base.ctl, sa->nbr, sa->bulk, sa->base.v.slab);
	HIPCHK(hipGetLastError());
	Control now;
	if (gave_up_late) { /* apply_failed was raised: not the rebuild's concern */
		TRY(read_ctl(sa, sa->base, &now));
		now.apply_failed = 0;
		TRY(write_ctl(sa, sa->base, &now));
	}
	TRY(launch_pbuild(sa, sa->incremental));
	TRY(read_ctl(sa, sa->base, &now));
	if (sa->force.rollbacks && now.taken) { sa->force.rollbacks--; now.error_flags |= MGL_ERR_BAD_PACKET; } /* diagnostic (mgl_debug_set key 3): exercise the net */
	if (!(now.error_flags & MGL_ERR_BAD_PACKET)) return MGL_OK;
	hipLaunchKernelGGL(k_bulk_rollback, dim3(64), dim3(256), 0, sa->q.stream, sa->nbr, sa->bulk, sa->base.v.slab);
	HIPCHK(hipGetLastError());
	now.error_flags &= ~MGL_ERR_BAD_PACKET;
	now.accepted -= now.taken;
	now.taken = 0;
	sa->bulk_rollbacks++;
	TRY(write_ctl(sa, sa->base, &now));
	return launch_pbuild(sa);
}
/* the tail of a bulk step: selection, journals into the slab, parallel rebuild, best-slab tracking */
static int launch_bulk_tail(mgl_sa* sa, uint64_t next_gstep)
{
	TRY(bulk_select(sa));
	BatchHdr bstat = {};
	bstat.status = MGL_BATCH_REBUILD; /* without the batch path: everything is the rebuild's */
	bool closed = false;
	/* (the rollback net hangs under the rebuild: while a test forces it, steps go that way) */
	if (sa->batch_ok && !sa->force.rollbacks) TRY(bulk_batch_accept(sa, next_gstep, &bstat, &closed));
	if (sa->batch_ok) sa->autoacc.select_small = bstat.acceptable <= 512u; /* this step's acceptable neighbours size the next step's selection */
	if (bstat.status == MGL_BATCH_DONE) sa->batch_accepts++; /* the moves are in: structures patched, exact cost in Control::rebuild_cost, every rep packet of the new walk checked */
	else if (bstat.status != MGL_BATCH_NONE) TRY(bulk_rebuild_checked(sa, bstat));
	if (!closed) launch_bulk_close(sa, nullptr);
	HIPCHK(hipGetLastError());
	return MGL_OK;
}

/* ---- mgl_sa_run in stages */
#define MGL_TIMED_STEPS_MAX 512u
/* a run of `steps` steps begins: which of them carry events (StepTimer) */
static void timer_begin_run(StepTimer& t, bool timing, uint64_t steps)
{
	t.stride = steps > 16 ? 4u : 1u;
	const uint64_t n = (steps + t.stride - 1) / t.stride;
	t.timed = timing ? (n < MGL_TIMED_STEPS_MAX ? n : MGL_TIMED_STEPS_MAX) : 0;
	t.step = -1;
	t.sim_timed.clear();
}
/* step s of the run begins; `slices` k_sim launches if its regular launch is the split form's, else 0 */
static void timer_begin_step(StepTimer& t, uint64_t s, uint32_t slices)
{
	const bool timed = s % t.stride == 0 && s / t.stride < t.timed;
	t.step = timed ? (int64_t)(s / t.stride) : -1;
	t.sim = timed && slices != 0;
	if (timed) t.sim_timed.push_back((uint8_t)(slices < 2u ? slices : 2u));
}
/* the run has been waited for: the elapsed times between its marks into stats */
static int timer_add(const StepTimer& t, mgl_sa_stats* stats)
{
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, t.ev_begin, t.ev_end));
	stats->gpu_ms_total = ms;
	for (size_t s = 0; s < t.timed && 4 * s + 3 < t.ev_pool.size(); s++) {
		HIPCHK(hipEventElapsedTime(&ms, t.ev_pool[4 * s + T_NBR_BEGIN], t.ev_pool[4 * s + T_NBR_END]));
		stats->gpu_ms_neighbours += ms;
		HIPCHK(hipEventElapsedTime(&ms, t.ev_pool[4 * s + T_ACCEPT_BEGIN], t.ev_pool[4 * s + T_ACCEPT_END]));
		stats->gpu_ms_rebuild += ms;
	}
	stats->neighbour_launches = t.timed;
	for (size_t s = 0; s < t.timed && s < t.sim_timed.size(); s++)
		for (uint32_t h = 0; h < t.sim_timed[s]; h++) { /* the regular launches: one per slice, at most two timed */
			HIPCHK(hipEventElapsedTime(&ms, t.ev_sim_pool[4 * s + 2 * h], t.ev_sim_pool[4 * s + 2 * h + 1]));
			stats->gpu_ms_sim += ms;
			stats->sim_launches++;
		}
	return MGL_OK;
}
/* a step's neighbours between their two timing slots */
static int run_neighbours(mgl_sa* sa, bool zero_counts)
{
	TRY(mark(sa, T_NBR_BEGIN, sa->q.stream));
	TRY(launch_neighbours(sa, ~0ull, zero_counts));
	return mark(sa, T_NBR_END, sa->q.stream);
}
/* Live target weights, before step `gstep` of a run takes its targets (megalania_hip.h has the rule): under
 * MGL_LW_SINGLE_ONLY a bulk-route step passes without weights and without a refresh; any other step refreshes if one is due
 * or the handle is stale.  Targets queued ahead under the other setting are made again. */
static int live_step(mgl_sa* sa, uint64_t gstep, bool bulk)
{
	LiveWeights& lw = sa->live;
	const bool apply = !(bulk && (lw.cfg.flags & MGL_LW_SINGLE_ONLY));
	if (apply != sa->wt_apply) {
		sa->wt_apply = apply;
		if (sa->tgt_ahead != TGT_NONE) sa->tgt_ahead = TGT_STALE;
	}
	if (!apply) {
		if (gstep % lw.cfg.every == 0) lw.stale = true; /* due during bulk steps: before the first single step after them */
		return MGL_OK;
	}
	if (lw.stale || gstep % lw.cfg.every == 0) return live_refresh(sa, gstep);
	return MGL_OK;
}
/* One step by the single route: neighbours, the decision, then the in-place accept (launch_apply, which queues the targets of
 * step next_gstep ahead) or -- MGL_NO_INCREMENTAL_APPLY, the full-walk engine -- best-slab copy, rebuild and lazy snapshot */
static int step_single(mgl_sa* sa, bool first, uint64_t next_gstep)
{
	const bool inc_apply = sa->incremental && sa->incremental_apply;
	TRY(run_neighbours(sa, first || !inc_apply));
	hipLaunchKernelGGL(k_decide, dim3(1), dim3(1024), 0, sa->q.stream, sa->ctx, sa->base.v, sa->base.ctl, sa->nbr, decide_args(sa), inc_apply ? 0 : 1);
	HIPCHK(hipGetLastError());
	TRY(mark(sa, T_ACCEPT_BEGIN, sa->q.stream));
	if (inc_apply) {
		TRY(launch_apply(sa, next_gstep));
	} else {
		hipLaunchKernelGGL(k_copy_best, dim3(256), dim3(256), 0, sa->q.stream, (const Control*)sa->base.ctl,
		                   (const mgl_pk*)sa->base.v.slab, sa->d_best, sa->ctx.n);
		HIPCHK(hipGetLastError());
		TRY(rebuild_base(sa, 1));
		if (sa->incremental && sa->snapshots) TRY(launch_snapshot(sa, sa->snap_best, 1, 0, 1));
	}
	return mark(sa, T_ACCEPT_END, sa->q.stream);
}
/* one step by the bulk route: neighbours, then launch_bulk_tail */
static int step_bulk(mgl_sa* sa, bool first, uint64_t next_gstep)
{
	TRY(run_neighbours(sa, first || !(sa->incremental && sa->incremental_apply)));
	TRY(mark(sa, T_ACCEPT_BEGIN, sa->q.stream));
	TRY(launch_bulk_tail(sa, next_gstep));
	return mark(sa, T_ACCEPT_END, sa->q.stream);
}
/* How many steps run before the host looks at the device again.  Every block ends with one small read-back: AUTO needs the
 * counters, and the form of the regular launch (split / one kernel) follows the device's recommendation from block to block.
 * AUTO: a block is `full` = 16 single / 4 bulk steps wherever the calls' boundaries fall (blk_done steps of it are done). */
static uint64_t block_length(const mgl_sa* sa, int mode, uint64_t full, uint64_t left)
{
	uint64_t block = mode == MGL_ACCEPT_AUTO ? full - sa->autoacc.blk_done : full;
	if (sa->form.short_looks && block > 4u) block = 4u; /* a form was just switched (a trial, usually): look again soon, a trial of a form twice as slow should not last a whole block */
	return block > left ? left : block;
}
/* the form the device recommends becomes the regular launch's */
static void adopt_form(mgl_sa* sa, const Control& c)
{
	if (sa->form.adaptive && sa->form.form_single != (c.nbr_single != 0)) { sa->form.form_single = c.nbr_single != 0; sa->form.short_looks = 3; }
}
/* between two blocks, with the counters just read: the launch form, and AUTO's route for the next block if this one is over */
static void end_block(mgl_sa* sa, const Control& now, bool bulk, uint64_t full, bool block_over)
{
	AutoAccept& au = sa->autoacc;
	if (sa->form.short_looks) sa->form.short_looks--;
	adopt_form(sa, now);
	if (!block_over) return;
	au.decide(bulk, full, now.imp_cands - au.blk_imp0, now.accepted - au.blk_acc0, sa->bulk_threshold, sa->batch_ok);
	au.blk_done = 0; au.blk_imp0 = now.imp_cands; au.blk_acc0 = now.accepted;
}
/* what a run did, from the control block before and after it, the timed steps and the handle's own counters */
static int fill_stats(mgl_sa* sa, const Control& before, const Control& after, uint64_t rollbacks_before, unsigned long long traffic_before, mgl_sa_stats* stats)
{
	memset(stats, 0, sizeof *stats);
	stats->steps = after.gstep - before.gstep; stats->evaluations = after.evals - before.evals; stats->failed = after.failed - before.failed;
	stats->accepted = after.accepted - before.accepted; stats->improved = after.improved - before.improved;
	stats->packets_evaluated = after.packets_eval - before.packets_eval;
	stats->current_cost = after.cur_cost; stats->best_cost = after.best_cost; stats->packets = after.packets;
	TRY(timer_add(sa->timer, stats));
	if (sa->count_traffic) {
		unsigned long long now[2] = { 0, 0 };
		HIPCHK(hipMemcpy(now, sa->d_traffic, sizeof now, hipMemcpyDeviceToHost));
		stats->sim_bytes_counted = now[0] - traffic_before;
	}
	stats->full_rebuilds = after.full_rebuilds - before.full_rebuilds; stats->fallback_neighbours = after.fallback_nbrs - before.fallback_nbrs;
	stats->second_pass_neighbours = after.big_nbrs - before.big_nbrs; stats->bulk_steps = after.bulk_steps - before.bulk_steps;
	stats->dropped_neighbours = after.dropped - before.dropped; stats->improving_neighbours = after.imp_cands - before.imp_cands;
	stats->bulk_rollbacks = sa->bulk_rollbacks - rollbacks_before; stats->bulk_double_writes = after.bulk_overlaps - before.bulk_overlaps;
	return MGL_OK;
}

extern "C" int mgl_sa_run(mgl_sa* sa, uint64_t steps, mgl_sa_stats* stats)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	HIPCHK(hipSetDevice(sa->device));
	Control before, after;
	TRY(read_ctl(sa, sa->base, &before));
	timer_begin_run(sa->timer, (sa->cfg.flags & MGL_F_TIMING) != 0, steps);
	const int mode = (sa->incremental && sa->parallel_build) ? sa->accept_mode : MGL_ACCEPT_SINGLE; /* bulk steps rebuild with the parallel builder */
	sa->mode_log.clear();
	if (sa->tgt_ahead != TGT_NONE) sa->tgt_ahead = TGT_STALE; /* (only behind a run that ended early: whatever was queued is not trusted) */
	const uint64_t rollbacks_before = sa->bulk_rollbacks;
	unsigned long long traffic_before[2] = { 0, 0 };
	if (sa->count_traffic) HIPCHK(hipMemcpy(traffic_before, sa->d_traffic, sizeof traffic_before, hipMemcpyDeviceToHost));
	AutoAccept& au = sa->autoacc;
	if (au.blk_done == 0) { au.blk_imp0 = before.imp_cands; au.blk_acc0 = before.accepted; }
	HIPCHK(hipEventRecord(sa->timer.ev_begin, sa->q.stream));
	for (uint64_t s = 0; s < steps;) {
		const bool bulk = mode == MGL_ACCEPT_BULK || (mode == MGL_ACCEPT_AUTO && au.bulk_now);
		const uint64_t full = mode == MGL_ACCEPT_AUTO ? (bulk ? 4u : 16u) : 64u;
		const uint64_t block = block_length(sa, mode, full, steps - s);
		for (uint64_t e = s + block; s < e; s++) {
			if (sa->mode_log.size() < (1u << 20)) sa->mode_log.push_back(bulk ? 1 : 0);
			if (sa->live.cfg.every) TRY(live_step(sa, before.gstep + s, bulk));
			timer_begin_step(sa->timer, s, sa->form.split_nbr && !sa->form.form_single ? nbr_slices(sa) : 0u);
			const uint64_t next_gstep = s + 1 < steps ? before.gstep + s + 1 : ~0ull;
			const int rc = bulk ? step_bulk(sa, s == 0, next_gstep) : step_single(sa, s == 0, next_gstep);
			sa->timer.step = -1; /* a launch_neighbours outside a run (mgl_neighbours) marks nothing */
			if (rc) return rc;
		}
		if (mode == MGL_ACCEPT_AUTO) au.blk_done += block;
		const bool block_over = mode == MGL_ACCEPT_AUTO && au.blk_done == full;
		if (block_over || (s < steps && sa->form.adaptive)) {
			Control now;
			TRY(read_ctl(sa, sa->base, &now));
			if (now.error_flags) break;
			end_block(sa, now, bulk, full, block_over);
		}
	}
	HIPCHK(hipEventRecord(sa->timer.ev_end, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	sa->wt_apply = true; /* outside a run the weights in force hold (mgl_neighbours) */
	TRY(read_ctl(sa, sa->base, &after));
	adopt_form(sa, after);
	if (stats) TRY(fill_stats(sa, before, after, rollbacks_before, traffic_before[0], stats));
	if (after.error_flags) {
		char buf[96];
		snprintf(buf, sizeof buf, "mgl_sa_run: device consistency check failed (flags 0x%x)", after.error_flags);
		return fail(MGL_EDEVICE, buf);
	}
	return MGL_OK;
}

extern "C" int mgl_sa_current(mgl_sa* sa, mgl_packet* packets_out, uint64_t* perplexity_out)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	HIPCHK(hipSetDevice(sa->device));
	Control c;
	int rc = read_ctl(sa, sa->base, &c);
	if (rc) return rc;
	if (perplexity_out) *perplexity_out = c.rebuild_cost;
	if (packets_out) return export_slab(sa, sa->base.v.slab, packets_out);
	return MGL_OK;
}
extern "C" int mgl_sa_best(mgl_sa* sa, mgl_packet* packets_out, uint64_t* perplexity_out)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	HIPCHK(hipSetDevice(sa->device));
	Control c;
	int rc = read_ctl(sa, sa->base, &c);
	if (rc) return rc;
	if (perplexity_out) *perplexity_out = c.best_cost;
	if (packets_out) return export_slab(sa, (sa->incremental && sa->snapshots && c.best_is_current) ? sa->base.v.slab : sa->d_best, packets_out);
	return MGL_OK;
}

/* run the walk kernel over `packets` in the scratch base */
static int scratch_walk(mgl_sa* sa, const mgl_packet* packets, bool want_cum, bool want_probs, Control* out)
{
	int rc = import_slab(sa, packets, sa->scratch.v.slab);
	if (rc) return rc;
	HIPCHK(hipMemsetAsync(sa->scratch.ctl, 0, sizeof(Control), sa->q.stream));
	if ((rc = launch_rebuild(sa, sa->scratch, 0, want_cum ? sa->d_cum : nullptr, want_probs ? sa->d_final_probs : nullptr))) return rc;
	if ((rc = read_ctl(sa, sa->scratch, out))) return rc;
	if (out->error_flags) return fail(MGL_EINVAL, "slab is not a valid parse of the input");
	return MGL_OK;
}

extern "C" int mgl_sa_set_best(mgl_sa* sa, const mgl_packet* packets, uint64_t perplexity)
{
	if (!sa || !packets) return fail(MGL_EINVAL, "null argument");
	HIPCHK(hipSetDevice(sa->device));
	Control c;
	int rc = scratch_walk(sa, packets, false, false, &c);
	if (rc) return rc;
	if (c.rebuild_cost != perplexity) return fail(MGL_EINVAL, "mgl_sa_set_best: perplexity does not match the slab");
	HIPCHK(hipMemcpyAsync(sa->d_best, sa->scratch.v.slab, sizeof(mgl_pk) * (size_t)sa->n, hipMemcpyDeviceToDevice, sa->q.stream));
	if (sa->d_snap_meta) HIPCHK(hipMemsetAsync(sa->d_snap_meta + 1, 0, sizeof(SnapMeta), sa->q.stream));
	if ((rc = read_ctl(sa, sa->base, &c))) return rc;
	c.best_cost = perplexity;
	c.best_is_current = 0;
	sa->best_unverified = true; /* the walk has no eye for the copied bytes: mgl_sa_begin_epoch(.., from_best) looks at them */
	return write_ctl(sa, sa->base, &c);
}

extern "C" int mgl_cost_slab(mgl_sa* sa, const mgl_packet* packets, uint64_t* total, uint64_t* per_packet_cumulative,
                             size_t* npackets)
{
	if (!sa || !packets) return fail(MGL_EINVAL, "null argument");
	HIPCHK(hipSetDevice(sa->device));
	Control c;
	int rc = scratch_walk(sa, packets, per_packet_cumulative != nullptr, false, &c);
	if (rc) return rc;
	if (total) *total = c.rebuild_cost;
	if (npackets) *npackets = (size_t)c.packets;
	if (per_packet_cumulative)
		HIPCHK(hipMemcpy(per_packet_cumulative, sa->d_cum, sizeof(uint64_t) * (size_t)c.packets, hipMemcpyDeviceToHost));
	return MGL_OK;
}

/* The exact cost of one parse under every supported lc/lp/pb (mgl_props.hip).  Validity is decided here, once, by the walk
 * mgl_cost_slab uses; the current slab (packets == NULL) is a valid parse by construction and is read where it lies. */
extern "C" int mgl_props_sweep(mgl_sa* sa, const mgl_packet* packets, mgl_props_cost* out, size_t cap, size_t* count, double* gpu_ms)
{
	static_assert(MGL_PROPS_TRIPLES == MGL_PROPS_NTRIPLES, "header and kernel disagree on the number of triples");
	if (!sa || !out) return fail(MGL_EINVAL, "null argument");
	if (count) *count = MGL_PROPS_TRIPLES;
	if (cap < MGL_PROPS_TRIPLES) return fail(MGL_ERANGE, "mgl_props_sweep: out holds fewer than 75 entries");
	HIPCHK(hipSetDevice(sa->device));
	const mgl_pk* slab = sa->base.v.slab;
	if (packets) {
		Control c;
		int rc = scratch_walk(sa, packets, false, false, &c);
		if (rc) return rc;
		slab = sa->scratch.v.slab;
	}
	struct Tmp {
		DevOwner own;
		uint64_t* d = nullptr;
		hipEvent_t t0 = nullptr, t1 = nullptr;
	} tmp;
	TRY(dnew(tmp.own, tmp.d, MGL_PROPS_TRIPLES));
	HIPCHK(tmp.own.event(&tmp.t0));
	HIPCHK(tmp.own.event(&tmp.t1));
	HIPCHK(hipEventRecord(tmp.t0, sa->q.stream));
	hipLaunchKernelGGL(k_props_sweep, dim3(MGL_PROPS_TRIPLES), dim3(64), 0, sa->q.stream, sa->ctx, slab, tmp.d);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(tmp.t1, sa->q.stream));
	uint64_t costs[MGL_PROPS_TRIPLES];
	HIPCHK(hipMemcpyAsync(costs, tmp.d, sizeof costs, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, tmp.t0, tmp.t1));
	if (gpu_ms) *gpu_ms = ms;
	for (uint32_t t = 0; t < MGL_PROPS_TRIPLES; t++) {
		const mgl_layout L = mgl_props_triple(t);
		out[t].props.lc = (uint8_t)L.lc; out[t].props.lp = (uint8_t)L.lp; out[t].props.pb = (uint8_t)L.pb;
		out[t].cost = costs[t];
	}
	return MGL_OK;
}

/* ---- segment props (mgl_segments.hip; include/megalania_hip.h, "Segment props", has the definitions) ---- */

static size_t seg_span_index(size_t i, size_t j, size_t m) { return i * m - i * (i - 1) / 2 + (j - i - 1); }

/* the grain rule over a host copy of a valid slab; cuts holds MGL_SEG_MAX_CUTS entries.  0: an entry of length 0 on the walk */
static size_t seg_cuts_host(const mgl_packet* p, uint64_t n, uint64_t grain, uint64_t* cuts)
{
	const uint64_t leaf = (n + 15) / 16, g = grain ? grain : 65536, step = g > leaf ? g : leaf;
	size_t k = 0;
	uint64_t pos = 0;
	cuts[k++] = 0;
	for (uint64_t cand = step; cand < n; cand += step) { /* at most 15 candidates: 16 step >= n */
		while (pos < cand) {
			if (!p[pos].len) return 0;
			pos += p[pos].len;
		}
		if (pos >= n) break;
		if (pos != cuts[k - 1]) cuts[k++] = pos;
	}
	cuts[k++] = n;
	return k;
}

/* the slab a call works on, validated if it is the caller's: on the device (*d_slab) and, if asked for, on the host */
static int seg_take_slab(mgl_sa* sa, const mgl_packet* packets, const mgl_pk** d_slab, std::vector<mgl_packet>* host)
{
	*d_slab = sa->base.v.slab;
	if (packets) {
		Control c;
		TRY(scratch_walk(sa, packets, false, false, &c));
		*d_slab = sa->scratch.v.slab;
	}
	if (host) {
		host->resize(sa->n);
		if (packets) memcpy(host->data(), packets, sizeof(mgl_packet) * (size_t)sa->n);
		else TRY(export_slab(sa, sa->base.v.slab, host->data()));
	}
	return MGL_OK;
}

extern "C" int mgl_segment_cuts(mgl_sa* sa, const mgl_packet* packets, uint64_t grain, uint64_t* cuts_out, size_t cap, size_t* ncuts)
{
	if (!sa || !cuts_out || !ncuts) return fail(MGL_EINVAL, "null argument");
	HIPCHK(hipSetDevice(sa->device));
	const mgl_pk* d_slab;
	std::vector<mgl_packet> host;
	TRY(seg_take_slab(sa, packets, &d_slab, &host));
	uint64_t cuts[MGL_SEG_MAX_CUTS];
	const size_t k = seg_cuts_host(host.data(), sa->n, grain, cuts);
	if (!k) return fail(MGL_EINVAL, "slab is not a valid parse of the input");
	*ncuts = k;
	if (cap < k) return fail(MGL_ERANGE, "mgl_segment_cuts: cuts_out is too small");
	memcpy(cuts_out, cuts, sizeof(uint64_t) * k);
	return MGL_OK;
}

/* the two kernels over a valid slab that lies on the device */
static int seg_sweep_device(mgl_sa* sa, const mgl_pk* slab, const uint64_t* cuts, size_t ncuts, uint64_t* cost_out, float* ms)
{
	static const char* nomem = "mgl_props_sweep_spans: the call's buffers do not fit the device";
	const uint32_t m = (uint32_t)ncuts - 1u, spans = m * (m + 1u) / 2u;
	/* launch order: longest span first, ties in index order */
	uint32_t h_cuts[MGL_SEG_MAX_CUTS], h_order[MGL_SEG_MAX_SPANS];
	for (size_t k = 0; k < ncuts; k++) h_cuts[k] = (uint32_t)cuts[k];
	uint32_t q = 0;
	for (uint32_t i = 0; i < m; i++)
		for (uint32_t j = i + 1; j <= m; j++) h_order[q++] = i | j << 8;
	std::stable_sort(h_order, h_order + spans, [&](uint32_t a, uint32_t b) {
		return h_cuts[a >> 8] - h_cuts[a & 0xFFu] > h_cuts[b >> 8] - h_cuts[b & 0xFFu];
	});
	struct Tmp {
		DevOwner own;
		uint32_t *cuts = nullptr, *order = nullptr, *starts = nullptr;
		uint64_t* cost = nullptr;
		hipEvent_t t0 = nullptr, t1 = nullptr;
	} tmp;
	TRY(dnew(tmp.own, tmp.cuts, MGL_SEG_MAX_CUTS, -1, nomem));
	TRY(dnew(tmp.own, tmp.order, MGL_SEG_MAX_SPANS, -1, nomem));
	TRY(dnew(tmp.own, tmp.starts, MGL_SEG_MAX_CUTS * MGL_SEG_START_WORDS, -1, nomem));
	TRY(dnew(tmp.own, tmp.cost, (size_t)spans * MGL_PROPS_TRIPLES, -1, nomem));
	HIPCHK(tmp.own.event(&tmp.t0));
	HIPCHK(tmp.own.event(&tmp.t1));
	hipStream_t s = sa->q.stream;
	HIPCHK(hipMemcpyAsync(tmp.cuts, h_cuts, sizeof(uint32_t) * ncuts, hipMemcpyHostToDevice, s));
	HIPCHK(hipMemcpyAsync(tmp.order, h_order, sizeof(uint32_t) * spans, hipMemcpyHostToDevice, s));
	HIPCHK(hipEventRecord(tmp.t0, s));
	hipLaunchKernelGGL(k_seg_starts, dim3(1), dim3(64), 0, s, sa->ctx, slab, (const uint32_t*)tmp.cuts, (uint32_t)ncuts, tmp.starts);
	HIPCHK(hipGetLastError());
	/* the sweep follows at once: from a cut that is no packet start its walks are bounded nonsense, thrown away below */
	hipLaunchKernelGGL(k_props_spans, dim3(spans * MGL_PROPS_TRIPLES), dim3(64), 0, s, sa->ctx, slab, (const uint32_t*)tmp.cuts, m,
	                   (const uint32_t*)tmp.starts, (const uint32_t*)tmp.order, tmp.cost);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(tmp.t1, s));
	uint32_t h_starts[MGL_SEG_MAX_CUTS * MGL_SEG_START_WORDS];
	std::vector<uint64_t> h_cost((size_t)spans * MGL_PROPS_TRIPLES);
	HIPCHK(hipMemcpyAsync(h_starts, tmp.starts, sizeof(uint32_t) * ncuts * MGL_SEG_START_WORDS, hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(h_cost.data(), tmp.cost, sizeof(uint64_t) * h_cost.size(), hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	for (size_t k = 0; k < ncuts; k++)
		if (!h_starts[k * MGL_SEG_START_WORDS]) return fail(MGL_ERANGE, "mgl_props_sweep_spans: cut " + std::to_string(cuts[k]) + " is not a packet start of the walk");
	HIPCHK(hipEventElapsedTime(ms, tmp.t0, tmp.t1));
	memcpy(cost_out, h_cost.data(), sizeof(uint64_t) * h_cost.size());
	return MGL_OK;
}

static int seg_check_cuts(const mgl_sa* sa, const uint64_t* cuts, size_t ncuts)
{
	bool ok = ncuts >= 2 && ncuts <= MGL_SEG_MAX_CUTS && cuts[0] == 0 && cuts[ncuts - 1] == sa->n;
	for (size_t k = 1; ok && k < ncuts; k++) ok = cuts[k] > cuts[k - 1];
	return ok ? MGL_OK : fail(MGL_EINVAL, "mgl_props_sweep_spans: between 2 and 17 cuts, strictly ascending from 0 to n");
}

extern "C" int mgl_props_sweep_spans(mgl_sa* sa, const mgl_packet* packets, const uint64_t* cuts, size_t ncuts, uint64_t* cost_out, size_t cap,
                                     size_t* count, double* gpu_ms)
{
	static_assert(MGL_SEG_MAX_SPANS == (MGL_SEG_MAX_CUTS - 1) * MGL_SEG_MAX_CUTS / 2, "spans of the most cuts");
	if (!sa || !cuts || !cost_out) return fail(MGL_EINVAL, "null argument");
	TRY(seg_check_cuts(sa, cuts, ncuts));
	const size_t m = ncuts - 1, need = m * (m + 1) / 2 * MGL_PROPS_TRIPLES;
	if (count) *count = need;
	if (cap < need) return fail(MGL_ERANGE, "mgl_props_sweep_spans: cost_out holds fewer than 75 entries per span");
	HIPCHK(hipSetDevice(sa->device));
	const mgl_pk* slab;
	TRY(seg_take_slab(sa, packets, &slab, nullptr));
	float ms = 0;
	TRY(seg_sweep_device(sa, slab, cuts, ncuts, cost_out, &ms));
	if (gpu_ms) *gpu_ms = ms;
	return MGL_OK;
}

extern "C" int mgl_segment_partition(const uint64_t* cost, size_t ncuts, const uint64_t* cuts, uint64_t overhead, mgl_segment* segs_out, size_t* nseg,
                                     uint64_t* total)
{
	if (!cost || !cuts || !segs_out || !nseg) return fail(MGL_EINVAL, "null argument");
	if (ncuts < 2 || ncuts > MGL_SEG_MAX_CUTS) return fail(MGL_EINVAL, "mgl_segment_partition: between 2 and 17 cuts");
	const size_t m = ncuts - 1;
	uint64_t best[MGL_SEG_MAX_CUTS];
	size_t from[MGL_SEG_MAX_CUTS], triple[MGL_SEG_MAX_CUTS];
	best[0] = 0;
	for (size_t j = 1; j <= m; j++) {
		bool have = false;
		for (size_t i = 0; i < j; i++) {
			const uint64_t* row = cost + seg_span_index(i, j, m) * MGL_PROPS_TRIPLES;
			size_t arg = 0;
			for (size_t t = 1; t < MGL_PROPS_TRIPLES; t++)
				if (row[t] < row[arg]) arg = t;
			const uint64_t v = best[i] + row[arg] + (i ? overhead : 0);
			if (!have || v < best[j]) { best[j] = v; from[j] = i; triple[j] = arg; have = true; }
		}
	}
	size_t k = 0;
	for (size_t j = m; j; j = from[j]) k++;
	*nseg = k;
	for (size_t j = m; j; j = from[j]) {
		const mgl_layout L = mgl_props_triple((uint32_t)triple[j]);
		mgl_segment& sg = segs_out[--k];
		sg.lo = cuts[from[j]]; sg.hi = cuts[j];
		sg.props.lc = (uint8_t)L.lc; sg.props.lp = (uint8_t)L.lp; sg.props.pb = (uint8_t)L.pb;
		sg.cost = cost[seg_span_index(from[j], j, m) * MGL_PROPS_TRIPLES + triple[j]];
	}
	if (total) *total = best[m];
	return MGL_OK;
}

extern "C" int mgl_sa_segment_props(mgl_sa* sa, const mgl_packet* packets, uint64_t grain, mgl_segment* segs_out, size_t cap, size_t* nseg,
                                    uint64_t* total, uint64_t* single_best, double* gpu_ms)
{
	if (!sa || !segs_out || !nseg) return fail(MGL_EINVAL, "null argument");
	HIPCHK(hipSetDevice(sa->device));
	const mgl_pk* slab;
	std::vector<mgl_packet> host;
	TRY(seg_take_slab(sa, packets, &slab, &host));
	uint64_t cuts[MGL_SEG_MAX_CUTS];
	const size_t ncuts = seg_cuts_host(host.data(), sa->n, grain, cuts);
	if (!ncuts) return fail(MGL_EINVAL, "slab is not a valid parse of the input");
	const size_t m = ncuts - 1;
	std::vector<uint64_t> cost(m * (m + 1) / 2 * MGL_PROPS_TRIPLES);
	float ms = 0;
	TRY(seg_sweep_device(sa, slab, cuts, ncuts, cost.data(), &ms));
	if (gpu_ms) *gpu_ms = ms;
	mgl_segment segs[MGL_SEG_MAX_CUTS];
	size_t k = 0;
	TRY(mgl_segment_partition(cost.data(), ncuts, cuts, MGL_SEG_OVERHEAD, segs, &k, total));
	if (single_best) *single_best = *std::min_element(cost.begin() + seg_span_index(0, m, m) * MGL_PROPS_TRIPLES, cost.begin() + (seg_span_index(0, m, m) + 1) * MGL_PROPS_TRIPLES);
	*nseg = k;
	if (cap < k) return fail(MGL_ERANGE, "mgl_sa_segment_props: segs_out is too small");
	memcpy(segs_out, segs, sizeof(mgl_segment) * k);
	return MGL_OK;
}

/* ---- segment re-parse (mgl_segparse.hip; include/megalania_hip.h, "Segment re-parse", has the rule): the stages of
 * mgl_segment_reparse, in the order they stand in.  One SegParse is one call: its buffers die with it. */
#define MGL_SEGP_MAX (MGL_SEG_MAX_CUTS - 1)
struct SegParse {
	/* settings (segp_args) */
	uint32_t nseg = 0, passes = 0, chunk = 0, maxch = 0, totch = 0, lds = 0;
	size_t snap_total = 0;
	SegVariant h_tab[MGL_SEGP_MAX];
	uint32_t h_cuts[MGL_SEG_MAX_CUTS];
	/* device buffers and events (segp_alloc) */
	SegVariant* tab = nullptr;
	uint32_t *cuts = nullptr, *starts = nullptr, *entry = nullptr, *take = nullptr, *done = nullptr;
	uint16_t* snaps = nullptr;
	mgl_pk *back = nullptr, *dp = nullptr, *keep = nullptr, *out = nullptr;
	unsigned long long* obj = nullptr;
	uint64_t* cost = nullptr;
	hipEvent_t t0 = nullptr, t1 = nullptr;
	/* the last walk's costs and the last DP's objectives, per segment */
	uint64_t h_cost[MGL_SEGP_MAX];
	unsigned long long h_obj[MGL_SEGP_MAX];
	DevOwner own;
};

/* argument checks; per segment its place, triple, settings after the defaults and clamps, its chunks and its snapshots */
static int segp_args(const mgl_sa* sa, SegParse& P, const mgl_segment* segs, size_t nseg, const mgl_adaptive_config* cfg)
{
	if (nseg < 1 || nseg > MGL_SEGP_MAX) return fail(MGL_EINVAL, "mgl_segment_reparse: between 1 and 16 segments");
	for (size_t k = 0; k < nseg; k++) {
		if (segs[k].lo != (k ? segs[k - 1].hi : 0) || segs[k].hi <= segs[k].lo || segs[k].hi > sa->n)
			return fail(MGL_EINVAL, "mgl_segment_reparse: the segments must tile [0, n) in ascending order");
		if ((uint32_t)segs[k].props.lc + segs[k].props.lp > 4u || segs[k].props.pb > 4u)
			return fail(MGL_EINVAL, "mgl_segment_reparse: supported properties are lc + lp <= 4, pb <= 4");
	}
	if (segs[nseg - 1].hi != sa->n) return fail(MGL_EINVAL, "mgl_segment_reparse: the segments must tile [0, n) in ascending order");
	if (cfg && cfg->from_current) return fail(MGL_EINVAL, "mgl_segment_reparse: from_current must be 0 (the slab is the packets argument)");
	P.nseg = (uint32_t)nseg;
	P.passes = cfg && cfg->passes ? cfg->passes : MGL_OPT_DEF_PASSES;
	if (P.passes > MGL_OPT_MAX_PASSES) return fail(MGL_EINVAL, "adaptive parse: at most 16 passes");
	uint32_t cand = cfg && cfg->cand ? cfg->cand : MGL_OPT_DEF_CAND, segment = cfg ? cfg->segment : 0u, ahead = cfg ? cfg->ahead : 0u;
	P.chunk = cfg && cfg->chunk ? cfg->chunk : MGL_OPT_DEF_CHUNK;
	TRY(adp_args(sa, cand, P.chunk, segment, ahead, false));
	for (uint32_t v = 0; v < P.nseg; v++) {
		SegVariant& t = P.h_tab[v];
		t.lo = (uint32_t)segs[v].lo; t.hi = (uint32_t)segs[v].hi;
		t.props = adp_pack_props(segs[v].props.lc, segs[v].props.lp, segs[v].props.pb);
		t.cand = cand; t.segment = segment; t.ahead = ahead;
		t.nch = (t.hi - t.lo + P.chunk - 1u) / P.chunk;
		t.ch_off = P.totch; t.snap_off = P.snap_total;
		const uint32_t stride = adp_stride(mgl_make_layout(segs[v].props.lc, segs[v].props.lp, segs[v].props.pb));
		P.totch += t.nch;
		P.snap_total += (size_t)t.nch * stride;
		if (t.nch > P.maxch) P.maxch = t.nch;
		if (stride * (uint32_t)sizeof(uint16_t) > P.lds) P.lds = stride * (uint32_t)sizeof(uint16_t);
		P.h_cuts[v] = t.lo;
	}
	P.h_cuts[P.nseg] = (uint32_t)sa->n;
	return MGL_OK;
}

static int segp_alloc(mgl_sa* sa, SegParse& P)
{
	static const char* nomem = "mgl_segment_reparse: the call's buffers do not fit the device";
	const size_t n = sa->n;
	auto room = [&](auto*& ptr, size_t count) { return dnew(P.own, ptr, count, -1, nomem); };
	TRY(room(P.tab, MGL_SEGP_MAX));
	TRY(room(P.cuts, MGL_SEG_MAX_CUTS));
	TRY(room(P.starts, MGL_SEG_MAX_CUTS * MGL_SEG_START_WORDS));
	TRY(room(P.take, MGL_SEGP_MAX));
	TRY(room(P.done, 1));
	TRY(room(P.obj, MGL_SEGP_MAX));
	TRY(room(P.cost, MGL_SEGP_MAX));
	TRY(dnew(P.own, P.entry, 5 * (size_t)P.totch, 0, nomem)); /* a walk that stops early leaves the LZMA initial state behind it */
	TRY(room(P.snaps, P.snap_total));
	TRY(room(P.back, n + 1));
	TRY(room(P.dp, n));
	TRY(room(P.keep, n));
	TRY(room(P.out, n));
	HIPCHK(P.own.event(&P.t0));
	HIPCHK(P.own.event(&P.t1));
	if (sa->mf_finder == MGL_MF_FRONTIER) HIPCHK(hipFuncSetAttribute((const void*)k_segp_dp<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds));
	else HIPCHK(hipFuncSetAttribute((const void*)k_segp_dp<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)P.lds));
	HIPCHK(hipMemcpyAsync(P.tab, P.h_tab, sizeof(SegVariant) * P.nseg, hipMemcpyHostToDevice, sa->q.stream));
	HIPCHK(hipMemcpyAsync(P.cuts, P.h_cuts, sizeof(uint32_t) * (P.nseg + 1u), hipMemcpyHostToDevice, sa->q.stream));
	return MGL_OK;
}

/* The walk of `slab` (a valid parse on the device) segment by segment from the resets: h_cost holds cost(lo, hi, T_s) of
 * every segment afterwards; `snaps`: the walk leaves the chunk starts and the model snapshots as well.  MGL_ERANGE (or
 * `bad`) where a segment boundary is no packet start of the slab. */
static int segp_slab_walk(mgl_sa* sa, SegParse& P, const mgl_pk* slab, bool snaps, int bad)
{
	hipStream_t s = sa->q.stream;
	const uint32_t ncuts = P.nseg + 1u;
	hipLaunchKernelGGL(k_seg_starts, dim3(1), dim3(64), 0, s, sa->ctx, slab, (const uint32_t*)P.cuts, ncuts, P.starts);
	hipLaunchKernelGGL(k_segp_walk, dim3(P.nseg), dim3(64), 0, s, sa->ctx, (const SegVariant*)P.tab, slab, 0, P.chunk, (const uint32_t*)P.starts,
	                   P.entry, snaps ? P.snaps : (uint16_t*)nullptr, P.cost);
	HIPCHK(hipGetLastError());
	uint32_t h_starts[MGL_SEG_MAX_CUTS * MGL_SEG_START_WORDS];
	HIPCHK(hipMemcpyAsync(h_starts, P.starts, sizeof(uint32_t) * ncuts * MGL_SEG_START_WORDS, hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(P.h_cost, P.cost, sizeof(uint64_t) * P.nseg, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	for (uint32_t k = 0; k < ncuts; k++)
		if (!h_starts[k * MGL_SEG_START_WORDS])
			return fail(bad, "mgl_segment_reparse: segment boundary " + std::to_string(P.h_cuts[k]) + " is not a packet start of the walk");
	return MGL_OK;
}

/* One pass: the DP of every chunk of every segment from the starts in entry / snaps into dp, then the walk that resolves
 * the copies against each segment coder's own state, costs them exactly and leaves the next pass's starts */
static int segp_pass(mgl_sa* sa, SegParse& P, bool snaps)
{
	hipStream_t s = sa->q.stream;
	hipLaunchKernelGGL(k_fill_literal, dim3(1024), dim3(256), 0, s, P.dp, (size_t)sa->n);
	HIPCHK(hipMemsetAsync(P.obj, 0, sizeof(unsigned long long) * P.nseg, s));
	if (sa->mf_finder == MGL_MF_FRONTIER)
		hipLaunchKernelGGL(k_segp_dp<true>, dim3(P.maxch, P.nseg), dim3(64), P.lds, s, sa->ctx, (const SegVariant*)P.tab, (const uint32_t*)P.entry,
		                   (const uint16_t*)P.snaps, P.chunk, P.back, P.dp, P.obj, mf_lists(sa));
	else
		hipLaunchKernelGGL(k_segp_dp<false>, dim3(P.maxch, P.nseg), dim3(64), P.lds, s, sa->ctx, (const SegVariant*)P.tab, (const uint32_t*)P.entry,
		                   (const uint16_t*)P.snaps, P.chunk, P.back, P.dp, P.obj, MfLists{});
	hipLaunchKernelGGL(k_segp_walk, dim3(P.nseg), dim3(64), 0, s, sa->ctx, (const SegVariant*)P.tab, (const mgl_pk*)P.dp, 1, P.chunk,
	                   (const uint32_t*)nullptr, P.entry, snaps ? P.snaps : (uint16_t*)nullptr, P.cost);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(P.h_obj, P.obj, sizeof(unsigned long long) * P.nseg, hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(P.h_cost, P.cost, sizeof(uint64_t) * P.nseg, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	return MGL_OK;
}

/* The join: out = per segment the input's packets or the kept DP copies, resolved in one walk from byte 0; then the cost of
 * every segment of it, as pass 0's starts were made */
static int segp_join(mgl_sa* sa, SegParse& P, const mgl_pk* slab, const uint32_t* h_take)
{
	hipStream_t s = sa->q.stream;
	HIPCHK(hipMemcpyAsync(P.take, h_take, sizeof(uint32_t) * P.nseg, hipMemcpyHostToDevice, s));
	hipLaunchKernelGGL(k_fill_literal, dim3(1024), dim3(256), 0, s, P.out, (size_t)sa->n);
	/* starts still holds the input's true stacks at the cuts (segp_slab_walk) */
	hipLaunchKernelGGL(k_segp_join, dim3(1), dim3(64), 0, s, sa->ctx, (const SegVariant*)P.tab, P.nseg, (const uint32_t*)P.take, slab,
	                   (const mgl_pk*)P.keep, (const uint32_t*)P.starts, P.out, P.done);
	HIPCHK(hipGetLastError());
	uint32_t done = 0;
	HIPCHK(hipMemcpyAsync(&done, P.done, sizeof done, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	if (done != sa->n) return fail(MGL_EDEVICE, "mgl_segment_reparse: the join's walk stopped at " + std::to_string(done));
	return segp_slab_walk(sa, P, P.out, false, MGL_EDEVICE);
}

extern "C" int mgl_segment_reparse(mgl_sa* sa, const mgl_packet* packets, const mgl_segment* segs, size_t nseg, const mgl_adaptive_config* cfg,
                                   mgl_packet* packets_out, mgl_segment* segs_out, mgl_segment_parse_stats* stats, int* taken, double* gpu_ms)
{
	if (!sa || !segs || !packets_out || !segs_out) return fail(MGL_EINVAL, "null argument");
	SegParse P;
	TRY(segp_args(sa, P, segs, nseg, cfg));
	HIPCHK(hipSetDevice(sa->device));
	const mgl_pk* slab = sa->base.v.slab;
	std::vector<mgl_packet> host(sa->n);
	if (packets) {
		Control c;
		if (scratch_walk(sa, packets, false, false, &c)) return fail(MGL_ERANGE, "mgl_segment_reparse: packets is not a valid parse of the input");
		slab = sa->scratch.v.slab;
		memcpy(host.data(), packets, sizeof(mgl_packet) * (size_t)sa->n);
	} else TRY(export_slab(sa, slab, host.data()));
	if (sa->mf_finder == MGL_MF_FRONTIER) TRY(mf_ensure(sa, sa->mf_depth));
	TRY(segp_alloc(sa, P));
	HIPCHK(hipEventRecord(P.t0, sa->q.stream));

	mgl_segment_parse_stats st[MGL_SEGP_MAX];
	memset(st, 0, sizeof st);
	uint64_t best[MGL_SEGP_MAX], sum_start = 0, sum_final = 0;
	uint32_t take[MGL_SEGP_MAX], any = 0;
	TRY(segp_slab_walk(sa, P, slab, true, MGL_ERANGE));
	for (uint32_t v = 0; v < P.nseg; v++) {
		st[v].passes = P.passes; st[v].best_pass = UINT32_MAX;
		st[v].start_cost = st[v].final_cost = best[v] = P.h_cost[v];
		sum_start += P.h_cost[v];
	}
	for (uint32_t p = 0; p < P.passes; p++) {
		TRY(segp_pass(sa, P, p + 1 < P.passes));
		for (uint32_t v = 0; v < P.nseg; v++) {
			st[v].pass_cost[p] = P.h_cost[v]; st[v].objective[p] = P.h_obj[v];
			if (P.h_cost[v] >= best[v]) continue;
			best[v] = P.h_cost[v]; st[v].best_pass = p;
			const SegVariant& t = P.h_tab[v];
			HIPCHK(hipMemcpyAsync(P.keep + t.lo, P.dp + t.lo, sizeof(mgl_pk) * (t.hi - t.lo), hipMemcpyDeviceToDevice, sa->q.stream));
		}
	}
	for (uint32_t v = 0; v < P.nseg; v++) any |= take[v] = st[v].best_pass != UINT32_MAX;

	/* the guard: the joined slab is handed out only where its segments cost less than the input's, in total */
	int took = 0;
	if (any) {
		TRY(segp_join(sa, P, slab, take));
		for (uint32_t v = 0; v < P.nseg; v++) sum_final += P.h_cost[v];
		took = sum_final < sum_start;
	}
	if (took) {
		for (uint32_t v = 0; v < P.nseg; v++) st[v].final_cost = P.h_cost[v];
		TRY(export_slab(sa, P.out, packets_out));
	} else {
		for (uint32_t v = 0; v < P.nseg; v++) st[v].best_pass = UINT32_MAX;
		memcpy(packets_out, host.data(), sizeof(mgl_packet) * (size_t)sa->n);
	}
	HIPCHK(hipEventRecord(P.t1, sa->q.stream));
	HIPCHK(hipEventSynchronize(P.t1));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, P.t0, P.t1));
	if (took) {
		/* device consistency check: what is handed out is a valid parse of the input */
		Control c;
		if (scratch_walk(sa, packets_out, false, false, &c)) return fail(MGL_EDEVICE, "mgl_segment_reparse: the joined slab is not a valid parse of the input");
	}
	for (uint32_t v = 0; v < P.nseg; v++) {
		segs_out[v] = segs[v];
		segs_out[v].cost = st[v].final_cost;
	}
	if (stats) memcpy(stats, st, sizeof(mgl_segment_parse_stats) * P.nseg);
	if (taken) *taken = took;
	if (gpu_ms) *gpu_ms = ms;
	return MGL_OK;
}

/* the two kernels of the cost map over a valid slab that lies on the device; the map stays in tmp.map, on the device, for as
 * long as the caller keeps `tmp` (mgl_cost_map copies it out, mgl_sa_weight_targets_by_cost makes weights of it there) */
struct CostMapBufs {
	DevOwner own;
	uint32_t *mark = nullptr, *map = nullptr;
	CostMapSums* sums = nullptr;
	hipEvent_t t0 = nullptr, t1 = nullptr;
};
static int cost_map_device(mgl_sa* sa, const mgl_pk* slab, const mgl_properties& pr, CostMapBufs& tmp, CostMapSums* sums, float* ms)
{
	static const char* nomem = "mgl_cost_map: the per-position buffers do not fit the device";
	CostMapSums& h = *sums;
	const size_t n = sa->n;
	if (sa->force.cm_nomem) { sa->force.cm_nomem--; return fail(MGL_ENOMEM, nomem); }
	TRY(dnew(tmp.own, tmp.mark, n, -1, nomem));
	TRY(dnew(tmp.own, tmp.map, n, -1, nomem));
	TRY(dnew(tmp.own, tmp.sums, 1, -1, nomem));
	HIPCHK(tmp.own.event(&tmp.t0));
	HIPCHK(tmp.own.event(&tmp.t1));
	hipStream_t s = sa->q.stream;
	HIPCHK(hipEventRecord(tmp.t0, s));
	HIPCHK(hipMemsetAsync(tmp.mark, 0, sizeof(uint32_t) * n, s));
	hipLaunchKernelGGL(k_costmap_walk, dim3(1), dim3(64), 0, s, sa->ctx, mgl_make_layout(pr.lc, pr.lp, pr.pb), slab, tmp.mark, tmp.sums);
	HIPCHK(hipGetLastError());
	hipLaunchKernelGGL(k_costmap_spread, dim3((sa->n + 255u) / 256u), dim3(256), 0, s, sa->n, (const uint32_t*)tmp.mark, tmp.map);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(tmp.t1, s));
	HIPCHK(hipMemcpyAsync(&h, tmp.sums, sizeof h, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	if (h.end_pos != sa->n) return fail(MGL_EDEVICE, "mgl_cost_map: the walk stopped inside the slab (device consistency check)");
	HIPCHK(hipEventElapsedTime(ms, tmp.t0, tmp.t1));
	return MGL_OK;
}
static void cost_report_fill(mgl_cost_report* report, const CostMapSums& h, float ms)
{
	report->total = h.total; report->packets = h.packets;
	for (uint32_t k = 0; k < MGL_CC_CLASSES; k++) { report->class_cost[k] = h.class_cost[k]; report->class_bits[k] = h.class_bits[k]; }
	for (uint32_t t = 0; t < 4; t++) { report->type_cost[t] = h.type_cost[t]; report->type_packets[t] = h.type_packets[t]; report->type_bytes[t] = h.type_bytes[t]; }
	report->gpu_ms = ms;
}
/* Where a parse spends its bits (mgl_costmap.hip).  Validity as in mgl_props_sweep: the walk of mgl_cost_slab decides it for a
 * caller's slab, and the current slab is read where it lies.  The call's two buffers -- a mark and a map entry per position,
 * 8 bytes per input byte -- are its own and die with it. */
extern "C" int mgl_cost_map(mgl_sa* sa, const mgl_packet* packets, const mgl_properties* props, uint32_t* map_out, mgl_cost_report* report)
{
	static_assert(MGL_CC_CLASSES == MGL_CM_CLASSES, "header and kernel disagree on the number of classes");
	if (!sa) return fail(MGL_EINVAL, "null handle");
	const mgl_properties pr = props ? *props : sa->props;
	if ((uint32_t)pr.lc + pr.lp > 4u || pr.pb > 4u) return fail(MGL_EINVAL, "mgl_cost_map: supported properties are lc + lp <= 4, pb <= 4");
	HIPCHK(hipSetDevice(sa->device));
	const mgl_pk* slab = sa->base.v.slab;
	if (packets) {
		Control c;
		int rc = scratch_walk(sa, packets, false, false, &c);
		if (rc) return rc;
		slab = sa->scratch.v.slab;
	}
	CostMapBufs tmp;
	CostMapSums h;
	float ms = 0;
	TRY(cost_map_device(sa, slab, pr, tmp, &h, &ms));
	const size_t n = sa->n;
	if (map_out) HIPCHK(hipMemcpy(map_out, tmp.map, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
	if (report) cost_report_fill(report, h, ms);
	return MGL_OK;
}
/* the live map's kernel over the current base (incremental engine): zeroes the sums, leaves marks and sums on the device */
static int launch_cost_map_live(mgl_sa* sa, uint32_t* mark, CostMapSums* sums)
{
	static_assert(MGL_CML_MAX_BLOCK == (1u << MGL_PB_MAX_SHIFT), "the live map's LDS marks hold the chain index's largest block");
	hipStream_t s = sa->q.stream;
	HIPCHK(hipMemsetAsync(sums, 0, sizeof *sums, s));
	hipLaunchKernelGGL(k_cml_blocks, dim3(sa->b2.nsb < MGL_CML_GRID ? sa->b2.nsb : MGL_CML_GRID), dim3(MGL_CML_THREADS), 0, s, sa->ctx, sa->b2, mark, sums);
	HIPCHK(hipGetLastError());
	return MGL_OK;
}
/* The cost map of the current slab from the event chains (mgl_costmap_live.hip): mgl_cost_map(sa, NULL, NULL, ..)'s integers
 * without its walk.  The full-walk engine keeps no chains and is served by the walk. */
extern "C" int mgl_cost_map_live(mgl_sa* sa, uint32_t* map_out, mgl_cost_report* report)
{
	static const char* nomem = "mgl_cost_map_live: the per-position buffers do not fit the device";
	if (!sa) return fail(MGL_EINVAL, "null handle");
	if (!sa->incremental) return mgl_cost_map(sa, nullptr, nullptr, map_out, report);
	HIPCHK(hipSetDevice(sa->device));
	if (sa->force.cm_nomem) { sa->force.cm_nomem--; return fail(MGL_ENOMEM, nomem); }
	CostMapBufs tmp;
	const size_t n = sa->n;
	TRY(dnew(tmp.own, tmp.mark, n, -1, nomem));
	TRY(dnew(tmp.own, tmp.map, n, -1, nomem));
	TRY(dnew(tmp.own, tmp.sums, 1, -1, nomem));
	HIPCHK(tmp.own.event(&tmp.t0));
	HIPCHK(tmp.own.event(&tmp.t1));
	hipStream_t s = sa->q.stream;
	HIPCHK(hipEventRecord(tmp.t0, s));
	TRY(launch_cost_map_live(sa, tmp.mark, tmp.sums));
	hipLaunchKernelGGL(k_costmap_spread, dim3((sa->n + 255u) / 256u), dim3(256), 0, s, sa->n, (const uint32_t*)tmp.mark, tmp.map);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(tmp.t1, s));
	CostMapSums h;
	HIPCHK(hipMemcpyAsync(&h, tmp.sums, sizeof h, hipMemcpyDeviceToHost, s));
	Control c;
	TRY(read_ctl(sa, sa->base, &c));
	if (h.total != c.rebuild_cost) return fail(MGL_EDEVICE, "mgl_cost_map_live: the chains' total is not the current cost (device consistency check)");
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, tmp.t0, tmp.t1));
	if (map_out) HIPCHK(hipMemcpy(map_out, tmp.map, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
	if (report) cost_report_fill(report, h, ms);
	return MGL_OK;
}

/* ---- cost-weighted targets (mgl_weights.hip) */
static void weights_release(mgl_sa* sa)
{
	sa->own.release(sa->d_wt); sa->own.release(sa->d_wt_pre); sa->own.release(sa->d_wt_blk);
	sa->d_wt = nullptr; sa->d_wt_pre = nullptr; sa->d_wt_blk = nullptr;
	sa->wt_total = sa->wt_slo = sa->wt_window = 0;
	if (sa->tgt_ahead != TGT_NONE) sa->tgt_ahead = TGT_STALE;
}
/* the handle's three buffers, kept from one set to the next; one that does not fit leaves the handle without weights */
static int weights_alloc(mgl_sa* sa)
{
	static const char* nomem = "target weights: the buffers (4 n + n / 8 bytes) do not fit the device";
	if (sa->d_wt) return MGL_OK;
	int rc = dnew(sa->own, sa->d_wt, sa->n, -1, nomem);
	if (!rc) rc = dnew(sa->own, sa->d_wt_pre, (size_t)wt_cells(sa->n) + 1u, -1, nomem);
	if (!rc) rc = dnew(sa->own, sa->d_wt_blk, (size_t)wt_blocks(sa->n) + 2u, -1, nomem);
	if (rc) weights_release(sa);
	return rc;
}
/* S[lo] and W of the focus window in force, read back: one wavefront and one synchronisation per change of weights or window,
 * none per step */
static int weights_window(mgl_sa* sa)
{
	if (!sa->d_wt) return MGL_OK;
	hipStream_t st = sa->q.stream;
	uint64_t* out = sa->d_wt_blk + wt_blocks(sa->n);
	hipLaunchKernelGGL(k_wt_window, dim3(1), dim3(64), 0, st, (const uint32_t*)sa->d_wt, (const uint64_t*)sa->d_wt_pre, sa->n, sa->focus_lo, sa->focus_hi ? sa->focus_hi : sa->n, out);
	HIPCHK(hipGetLastError());
	uint64_t v[2] = { 0, 0 };
	HIPCHK(hipMemcpyAsync(v, out, sizeof v, hipMemcpyDeviceToHost, st));
	HIPCHK(hipStreamSynchronize(st));
	sa->wt_slo = v[0]; sa->wt_window = v[1];
	return MGL_OK;
}
/* the prefix structure over the weights in d_wt: the four launches of mgl_weights.hip, on the main stream */
static int weights_prefix(mgl_sa* sa)
{
	hipStream_t st = sa->q.stream;
	const uint32_t n = sa->n, ncell = wt_cells(n), nblk = wt_blocks(n);
	hipLaunchKernelGGL(k_wt_cells, dim3((ncell + 3u) / 4u), dim3(256), 0, st, (const uint32_t*)sa->d_wt, n, sa->d_wt_pre, ncell);
	hipLaunchKernelGGL(k_wt_blocks, dim3(nblk), dim3(64), 0, st, sa->d_wt_pre, ncell, sa->d_wt_blk);
	hipLaunchKernelGGL(k_wt_scan, dim3(1), dim3(64), 0, st, sa->d_wt_blk, nblk, sa->d_wt_pre, ncell);
	hipLaunchKernelGGL(k_wt_add, dim3((ncell + 255u) / 256u), dim3(256), 0, st, sa->d_wt_pre, ncell, (const uint64_t*)sa->d_wt_blk);
	HIPCHK(hipGetLastError());
	return MGL_OK;
}
/* the prefix structure, then the window.  Targets queued ahead were made under the old weights, and may still be reading them:
 * the second stream is waited for before this is called. */
static int weights_commit(mgl_sa* sa, uint64_t total)
{
	TRY(weights_prefix(sa));
	sa->wt_total = total;
	if (sa->tgt_ahead != TGT_NONE) sa->tgt_ahead = TGT_STALE;
	return weights_window(sa);
}
static int weights_refuse(const mgl_sa* sa, const char* who)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	if (!sa->d_strat_pre) return fail(MGL_EINVAL, std::string(who) + ": position targets (MGL_F_POSITION_TARGETS) take no weights");
	return MGL_OK;
}
/* ---- live target weights (megalania_hip.h has the rule; mgl_costmap_live.hip the map) */
/* live weights off: the refresh's buffers go, the weights' own stay for whoever set others */
static void live_off(mgl_sa* sa)
{
	LiveWeights& lw = sa->live;
	sa->own.release(lw.d_mark); sa->own.release(lw.d_sums); sa->own.release(lw.t0); sa->own.release(lw.t1);
	lw = LiveWeights();
}
/* One refresh, before step `gstep` takes its targets and behind the previous step's accept on the main stream: the live map's
 * marks (the serial walk's on the full-walk engine), w = map + floor straight into the weights, the prefix structure, the
 * window.  One synchronisation: the window's words and the map's sums come back together. */
static int live_refresh(mgl_sa* sa, uint64_t gstep)
{
	LiveWeights& lw = sa->live;
	hipStream_t st = sa->q.stream;
	const uint32_t n = sa->n;
	/* targets queued ahead were made under the old weights and may still be reading them: the main stream waits for the second */
	if (sa->tgt_ahead != TGT_NONE) { HIPCHK(hipStreamWaitEvent(st, sa->q.ev_tgt, 0)); sa->tgt_ahead = TGT_STALE; }
	HIPCHK(hipEventRecord(lw.t0, st));
	if (sa->incremental) {
		TRY(launch_cost_map_live(sa, lw.d_mark, lw.d_sums));
		hipLaunchKernelGGL(k_cml_check, dim3(1), dim3(1), 0, st, (const CostMapSums*)lw.d_sums, sa->base.ctl);
	} else {
		HIPCHK(hipMemsetAsync(lw.d_mark, 0, sizeof(uint32_t) * (size_t)n, st));
		hipLaunchKernelGGL(k_costmap_walk, dim3(1), dim3(64), 0, st, sa->ctx, sa->ctx.L, (const mgl_pk*)sa->base.v.slab, lw.d_mark, lw.d_sums);
	}
	hipLaunchKernelGGL(k_cml_weights, dim3((n + 255u) / 256u), dim3(256), 0, st, n, (const uint32_t*)lw.d_mark, lw.cfg.floor, lw.cfg.floor_mean, (const CostMapSums*)lw.d_sums, sa->d_wt);
	HIPCHK(hipGetLastError());
	TRY(weights_prefix(sa));
	HIPCHK(hipEventRecord(lw.t1, st));
	CostMapSums h;
	HIPCHK(hipMemcpyAsync(&h, lw.d_sums, sizeof h, hipMemcpyDeviceToHost, st));
	TRY(weights_window(sa)); /* synchronises */
	if (!sa->incremental && h.end_pos != n) return fail(MGL_EDEVICE, "live weights: the walk stopped inside the slab (device consistency check)");
	const uint64_t floor = lw.cfg.floor_mean ? h.total / n : lw.cfg.floor;
	sa->wt_total = h.total + floor * n;
	lw.skip = sa->wt_total >= MGL_WT_MAX_TOTAL; /* this interval runs by the rule without weights */
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, lw.t0, lw.t1));
	lw.stats.refreshes++; lw.stats.skipped += lw.skip ? 1u : 0u;
	lw.stats.last_gstep = gstep; lw.stats.last_total = h.total; lw.stats.gpu_ms += ms;
	lw.stale = false;
	return MGL_OK;
}
extern "C" int mgl_sa_set_live_weights(mgl_sa* sa, const mgl_live_weights_config* cfg)
{
	static const char* nomem = "mgl_sa_set_live_weights: the buffers (8 n + n / 8 bytes) do not fit the device";
	TRY(weights_refuse(sa, "mgl_sa_set_live_weights"));
	if (cfg) {
		if (cfg->every == 0) return fail(MGL_EINVAL, "mgl_sa_set_live_weights: every must be at least 1");
		if (cfg->flags & ~MGL_LW_SINGLE_ONLY) return fail(MGL_EINVAL, "mgl_sa_set_live_weights: unknown flags");
		if (!cfg->floor_mean && cfg->floor > 0xFFFFFFFFu - (1u << MGL_CM_COST_BITS)) return fail(MGL_EINVAL, "mgl_sa_set_live_weights: floor + a map entry must fit 32 bits");
		if (!cfg->floor_mean && (uint64_t)cfg->floor * sa->n >= (MGL_WT_MAX_TOTAL >> 1)) return fail(MGL_EINVAL, "mgl_sa_set_live_weights: floor * n must stay below 2^43");
	}
	HIPCHK(hipSetDevice(sa->device));
	HIPCHK(hipStreamSynchronize(sa->q.stream2));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	live_off(sa);
	weights_release(sa); /* explicit weights are replaced; none are in force until the first refresh */
	if (!cfg) return MGL_OK;
	LiveWeights& lw = sa->live;
	int rc = weights_alloc(sa);
	if (!rc) rc = dnew(sa->own, lw.d_mark, sa->n, -1, nomem);
	if (!rc) rc = dnew(sa->own, lw.d_sums, 1, -1, nomem);
	if (!rc && (sa->own.event(&lw.t0) != hipSuccess || sa->own.event(&lw.t1) != hipSuccess)) rc = fail(MGL_EDEVICE, "mgl_sa_set_live_weights: no event");
	if (rc) { live_off(sa); weights_release(sa); return rc; }
	/* until the first refresh the weights are all 0: the window weighs nothing, whoever asks (mgl_sa_set_focus, mgl_sa_target_weights) */
	HIPCHK(hipMemsetAsync(sa->d_wt, 0, sizeof(uint32_t) * (size_t)sa->n, sa->q.stream));
	HIPCHK(hipMemsetAsync(sa->d_wt_pre, 0, sizeof(uint64_t) * ((size_t)wt_cells(sa->n) + 1u), sa->q.stream));
	lw.cfg = *cfg;
	lw.cfg.floor_mean = cfg->floor_mean ? 1u : 0u;
	if (lw.cfg.floor_mean) lw.cfg.floor = 0;
	lw.stale = true;
	return MGL_OK;
}
extern "C" int mgl_sa_live_weights(mgl_sa* sa, mgl_live_weights_config* cfg_out, mgl_live_weights_stats* stats_out)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	if (cfg_out) *cfg_out = sa->live.cfg;
	if (stats_out) *stats_out = sa->live.stats;
	return MGL_OK;
}

extern "C" int mgl_sa_set_target_weights(mgl_sa* sa, const uint32_t* weights)
{
	TRY(weights_refuse(sa, "mgl_sa_set_target_weights"));
	uint64_t total = 0;
	if (weights) {
		for (size_t x = 0; x < sa->n; x++) total += weights[x]; /* n < 2^28 entries below 2^32: no carry */
		if (total >= MGL_WT_MAX_TOTAL) return fail(MGL_EINVAL, "mgl_sa_set_target_weights: the weights must sum to less than 2^44");
	}
	HIPCHK(hipSetDevice(sa->device));
	HIPCHK(hipStreamSynchronize(sa->q.stream2));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	live_off(sa); /* explicit weights replace live ones */
	if (!weights) { weights_release(sa); return MGL_OK; }
	TRY(weights_alloc(sa));
	HIPCHK(hipMemcpyAsync(sa->d_wt, weights, sizeof(uint32_t) * (size_t)sa->n, hipMemcpyHostToDevice, sa->q.stream));
	return weights_commit(sa, total);
}
extern "C" int mgl_sa_weight_targets_by_cost(mgl_sa* sa, const mgl_packet* packets, uint32_t floor, uint64_t* total, double* gpu_ms)
{
	TRY(weights_refuse(sa, "mgl_sa_weight_targets_by_cost"));
	if (floor > 0xFFFFFFFFu - (1u << MGL_CM_COST_BITS)) return fail(MGL_EINVAL, "mgl_sa_weight_targets_by_cost: floor + a map entry must fit 32 bits");
	HIPCHK(hipSetDevice(sa->device));
	const mgl_pk* slab = sa->base.v.slab;
	if (packets) {
		Control c;
		TRY(scratch_walk(sa, packets, false, false, &c));
		slab = sa->scratch.v.slab;
	}
	CostMapBufs tmp;
	CostMapSums h;
	float ms = 0;
	TRY(cost_map_device(sa, slab, sa->props, tmp, &h, &ms)); /* MGL_ENOMEM here: the weights in force stay */
	const uint64_t sum = h.total + (uint64_t)floor * sa->n; /* below 2^20 n + 2^32 n < 2^61 */
	if (sum >= MGL_WT_MAX_TOTAL) return fail(MGL_EINVAL, "mgl_sa_weight_targets_by_cost: the weights must sum to less than 2^44");
	HIPCHK(hipStreamSynchronize(sa->q.stream2));
	live_off(sa); /* explicit weights replace live ones */
	TRY(weights_alloc(sa));
	hipLaunchKernelGGL(k_wt_from_map, dim3((sa->n + 255u) / 256u), dim3(256), 0, sa->q.stream, sa->n, (const uint32_t*)tmp.map, floor, sa->d_wt);
	HIPCHK(hipGetLastError());
	TRY(weights_commit(sa, sum)); /* synchronises: the map is read before `tmp` dies */
	if (total) *total = sum;
	if (gpu_ms) *gpu_ms = ms;
	return MGL_OK;
}
extern "C" int mgl_sa_target_weights(mgl_sa* sa, uint32_t* weights_out, uint64_t* total, uint64_t* window)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	if (total) *total = sa->wt_total;
	if (window) *window = sa->wt_window;
	if (!weights_out) return MGL_OK;
	if (!sa->d_wt) { memset(weights_out, 0, sizeof(uint32_t) * (size_t)sa->n); return MGL_OK; }
	HIPCHK(hipSetDevice(sa->device));
	HIPCHK(hipMemcpyAsync(weights_out, sa->d_wt, sizeof(uint32_t) * (size_t)sa->n, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	return MGL_OK;
}
extern "C" int mgl_weight_value(uint64_t W, uint32_t K, uint32_t j, uint64_t seed, uint64_t step, uint64_t* v)
{
	if (!v) return fail(MGL_EINVAL, "null argument");
	if (W == 0 || W >= MGL_WT_MAX_TOTAL || K == 0 || K > MGL_WT_MAX_K || j >= K) return fail(MGL_EINVAL, "mgl_weight_value: needs 0 < W < 2^44 and j < K <= 2^20");
	*v = weight_value(W, K, j, mgl_rng_key(seed, step, j));
	return MGL_OK;
}

/* ---- crossover of parses (mgl_crossover.hip) */
#define MGL_XO_DEF_GRAIN 64u
struct XoBufs {
	mgl_pk *slabs = nullptr, *child = nullptr;
	uint64_t *cost = nullptr, *onwalk = nullptr, *joint = nullptr, *bound = nullptr;
	uint32_t *state = nullptr, *last = nullptr;
	uint8_t* winner = nullptr;
	XoCounters* cnt = nullptr;
	hipEvent_t t0 = nullptr, t1 = nullptr;
	DevOwner own;
};
/* a buffer that does not fit is MGL_ENOMEM (the crossing exchange of all chains falls back on it) */
static int xo_alloc(mgl_sa* sa, XoBufs& x, uint32_t P)
{
	static const char* nomem = "crossover: the per-parent buffers do not fit the device";
	const size_t n = sa->n, nw = n / 64 + 1;
	if (sa->force.xo_nomem) { sa->force.xo_nomem--; return fail(MGL_ENOMEM, nomem); }
	auto room = [&](auto*& ptr, size_t count) { return dnew(x.own, ptr, count, -1, nomem); };
	TRY(room(x.slabs, n * P));
	TRY(room(x.cost, (n + 1) * P));
	TRY(room(x.state, 5 * n * P));
	TRY(room(x.onwalk, nw * P));
	TRY(room(x.child, n));
	TRY(room(x.joint, nw));
	TRY(room(x.bound, nw));
	TRY(room(x.last, nw));
	TRY(room(x.winner, n + 1));
	TRY(room(x.cnt, 1));
	HIPCHK(x.own.event(&x.t0));
	HIPCHK(x.own.event(&x.t1));
	return MGL_OK;
}
/* The P parents lie packed in x.slabs: walk them, cut, pick, scatter into x.child and cost the child.  A parent the walk
 * refuses is MGL_EINVAL, as from scratch_walk.  *st is filled except `adopted`. */
static int xo_run(mgl_sa* sa, XoBufs& x, uint32_t P, uint32_t grain, mgl_cross_stats* st)
{
	const uint32_t n = sa->n, nw = n / 64u + 1u, nblk = (n + 1u + 255u) / 256u;
	if (grain == 0) grain = MGL_XO_DEF_GRAIN;
	hipStream_t s = sa->q.stream;
	XoView v;
	v.slab = x.slabs; v.cost = x.cost; v.state = x.state; v.onwalk = x.onwalk; v.nw = nw;
	HIPCHK(hipEventRecord(x.t0, s));
	HIPCHK(hipMemsetAsync(x.onwalk, 0, sizeof(uint64_t) * (size_t)nw * P, s));
	HIPCHK(hipMemsetAsync(x.cnt, 0, sizeof(XoCounters), s));
	HIPCHK(hipMemsetAsync(x.winner, 0xFF, (size_t)n + 1, s));
	hipLaunchKernelGGL(k_xo_walk, dim3(P), dim3(64), 0, s, sa->ctx, v, x.cnt);
	HIPCHK(hipGetLastError());
	XoCounters h;
	HIPCHK(hipMemcpyAsync(&h, x.cnt, sizeof h, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	memset(st, 0, sizeof *st);
	st->parents = P; st->grain = grain;
	for (uint32_t p = 0; p < P; p++) {
		if (h.err[p]) return fail(MGL_EINVAL, "slab is not a valid parse of the input");
		st->parent_cost[p] = h.total[p];
	}
	hipLaunchKernelGGL(k_xo_joints, dim3(nblk), dim3(256), 0, s, n, P, v, x.joint);
	hipLaunchKernelGGL(k_xo_lastnz, dim3(1), dim3(1024), 0, s, (const uint64_t*)x.joint, nw, x.last);
	hipLaunchKernelGGL(k_xo_bounds, dim3(nblk), dim3(256), 0, s, n, nw, grain, (const uint64_t*)x.joint, (const uint32_t*)x.last, x.bound, x.cnt);
	hipLaunchKernelGGL(k_xo_lastnz, dim3(1), dim3(1024), 0, s, (const uint64_t*)x.bound, nw, x.last);
	hipLaunchKernelGGL(k_xo_winner, dim3(nblk), dim3(256), 0, s, n, P, (const uint64_t*)x.cost, (const uint64_t*)x.bound, (const uint32_t*)x.last,
	                   x.winner, x.cnt);
	hipLaunchKernelGGL(k_xo_scatter, dim3((n + 255u) / 256u), dim3(256), 0, s, n, P, (const mgl_pk*)x.slabs, (const uint64_t*)x.bound,
	                   (const uint32_t*)x.last, (const uint8_t*)x.winner, x.child);
	HIPCHK(hipGetLastError());
	/* the child: a batch of one, over parent 0's arrays (the winners are chosen) */
	v.slab = x.child;
	hipLaunchKernelGGL(k_xo_walk, dim3(1), dim3(64), 0, s, sa->ctx, v, x.cnt);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(x.t1, s));
	HIPCHK(hipMemcpyAsync(&h, x.cnt, sizeof h, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	if (h.err[0]) return fail(MGL_EDEVICE, "crossover: the child is not a valid parse (device consistency check)");
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, x.t0, x.t1));
	st->gpu_ms = ms;
	st->child_cost = h.total[0];
	st->predicted = h.predicted;
	st->boundaries = h.boundaries;
	for (uint32_t p = 0; p < P; p++) st->regions_from[p] = h.regions_from[p];
	return MGL_OK;
}

extern "C" int mgl_crossover(mgl_sa* sa, const mgl_packet* const* parents, size_t nparents, uint32_t grain, mgl_packet* child_out,
                             mgl_cross_stats* stats)
{
	static_assert(MGL_XO_MAX_PARENTS == MGL_XO_PARENTS, "header and kernels disagree on the number of parents");
	if (!sa || !parents) return fail(MGL_EINVAL, "null argument");
	if (nparents < 2 || nparents > MGL_XO_MAX_PARENTS) return fail(MGL_EINVAL, "mgl_crossover: 2 to 8 parents");
	for (size_t p = 0; p < nparents; p++) if (!parents[p]) return fail(MGL_EINVAL, "mgl_crossover: null parent");
	HIPCHK(hipSetDevice(sa->device));
	XoBufs x;
	int rc = xo_alloc(sa, x, (uint32_t)nparents);
	if (rc) return rc;
	for (size_t p = 0; p < nparents; p++) {
		if ((rc = import_slab(sa, parents[p], x.slabs + p * (size_t)sa->n))) return rc;
		HIPCHK(hipStreamSynchronize(sa->q.stream)); /* the staging area is reused */
	}
	mgl_cross_stats st;
	if ((rc = xo_run(sa, x, (uint32_t)nparents, grain, &st))) return rc;
	if (stats) *stats = st;
	if (child_out) return export_slab(sa, x.child, child_out);
	return MGL_OK;
}

/* the hash of the n packed entries at `slab` (device); the first of the 64 words of top-K scratch takes the sum */
static int slab_hash_device(mgl_sa* sa, const mgl_pk* slab, uint64_t* hash)
{
	unsigned long long* d_sum = (unsigned long long*)sa->d_topk_cost;
	HIPCHK(hipMemsetAsync(d_sum, 0, sizeof *d_sum, sa->q.stream));
	hipLaunchKernelGGL(k_slab_hash, dim3((sa->n + 255u) / 256u), dim3(256), 0, sa->q.stream, sa->n, slab, d_sum);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(hash, d_sum, sizeof *hash, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	return MGL_OK;
}

extern "C" int mgl_final_state(mgl_sa* sa, const mgl_packet* packets, uint16_t* probs_out, size_t probs_cap,
                               uint8_t* ctx_state_out, uint32_t dists_out[4])
{
	if (!sa || !packets) return fail(MGL_EINVAL, "null argument");
	HIPCHK(hipSetDevice(sa->device));
	Control c;
	int rc = scratch_walk(sa, packets, false, true, &c);
	if (rc) return rc;
	if (ctx_state_out) *ctx_state_out = (uint8_t)c.final_ctx_state;
	if (dists_out) memcpy(dists_out, c.final_dists, sizeof c.final_dists);
	if (probs_out) {
		const uint32_t total = sa->ctx.L.total, lit = total - MGL_OFF_LIT;
		if (probs_cap < total) return fail(MGL_ERANGE, "probs_out too small");
		std::vector<uint16_t> mine(total);
		HIPCHK(hipMemcpy(mine.data(), sa->d_final_probs, sizeof(uint16_t) * total, hipMemcpyDeviceToHost));
		/* reference struct order (lzma_state.h:47-53): lit | len | rep_len | dist | ctx_state */
		uint16_t* o = probs_out;
		memcpy(o, &mine[MGL_OFF_LIT], 2 * lit); o += lit;
		memcpy(o, &mine[MGL_OFF_LEN], 2 * 514); o += 514;
		memcpy(o, &mine[MGL_OFF_REP_LEN], 2 * 514); o += 514;
		memcpy(o, &mine[MGL_OFF_DIST], 2 * 387); o += 387;
		memcpy(o, &mine[0], 2 * 432);
	}
	return MGL_OK;
}

extern "C" int mgl_top_k(mgl_sa* sa, const mgl_packet* packets, size_t position, mgl_packet* out, uint64_t* costs, size_t* count)
{
	if (!sa || !packets || !out || !costs || !count) return fail(MGL_EINVAL, "null argument");
	if (position >= sa->n) return fail(MGL_ERANGE, "position outside the input");
	HIPCHK(hipSetDevice(sa->device));
	Control c;
	int rc = scratch_walk(sa, packets, false, false, &c);
	if (rc) return rc;
	const auto probe = sa->probe_form ? k_topk_probe<1> : k_topk_probe<0>;
	hipLaunchKernelGGL(probe, dim3(1), dim3(64), sa->walk_lds, sa->q.stream, sa->ctx, sa->scratch.v, (uint32_t)position,
	                   sa->d_topk_pk, sa->d_topk_cost, sa->d_small);
	HIPCHK(hipGetLastError());
	uint32_t cnt = 0;
	mgl_pk pk[64];
	uint64_t cs[64];
	HIPCHK(hipMemcpyAsync(&cnt, sa->d_small, sizeof cnt, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipMemcpyAsync(pk, sa->d_topk_pk, sizeof pk, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipMemcpyAsync(cs, sa->d_topk_cost, sizeof cs, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	if (cnt == ~0u) return fail(MGL_ERANGE, "position is not on the slab's walk");
	for (uint32_t i = 0; i < cnt; i++) {
		out[i].type = (uint8_t)mgl_pk_type(pk[i]); out[i].dist = mgl_pk_dist(pk[i]); out[i].len = (uint16_t)mgl_pk_len(pk[i]);
		costs[i] = cs[i];
	}
	*count = cnt;
	return MGL_OK;
}

extern "C" int mgl_substrings(mgl_sa* sa, size_t pos, size_t max_len, uint32_t* offsets, uint32_t* lengths, size_t cap, size_t* count)
{
	if (!sa || !count) return fail(MGL_EINVAL, "null argument");
	if (pos >= sa->n) return fail(MGL_ERANGE, "position outside the input");
	HIPCHK(hipSetDevice(sa->device));
	const uint32_t dcap = cap < sa->sub_cap ? (uint32_t)cap : sa->sub_cap;
	DevCtx c = sa->ctx;
	c.dict_limit = 0xFFFFFFFFu; /* the index query itself has no window (substring_enumerator.c:97 is a todo) */
	hipLaunchKernelGGL(k_substrings, dim3(1), dim3(1), 0, sa->q.stream, c, (uint32_t)pos, (uint32_t)max_len, sa->d_sub_offs,
	                   sa->d_sub_lens, dcap, sa->d_small);
	HIPCHK(hipGetLastError());
	uint32_t cnt = 0;
	HIPCHK(hipMemcpyAsync(&cnt, sa->d_small, sizeof cnt, hipMemcpyDeviceToHost, sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	const uint32_t take = cnt < dcap ? cnt : dcap;
	if (offsets && take) HIPCHK(hipMemcpy(offsets, sa->d_sub_offs, sizeof(uint32_t) * take, hipMemcpyDeviceToHost));
	if (lengths && take) HIPCHK(hipMemcpy(lengths, sa->d_sub_lens, sizeof(uint32_t) * take, hipMemcpyDeviceToHost));
	*count = cnt;
	return MGL_OK;
}

extern "C" int mgl_neighbours(mgl_sa* sa, uint64_t global_step, uint64_t* costs, mgl_diff* diffs, uint32_t* ndiffs, size_t diff_cap)
{
	if (!sa || !costs) return fail(MGL_EINVAL, "null argument");
	HIPCHK(hipSetDevice(sa->device));
	int rc = launch_neighbours(sa, global_step);
	if (rc == MGL_OK && sa->d_counts) HIPCHK(hipMemcpyAsync(&sa->d_counts[1], &sa->d_counts[0], sizeof(StepCounts), hipMemcpyDeviceToDevice, sa->q.stream));
	if (rc) return rc;
	const size_t K = sa->cfg.neighbours_per_step;
	HIPCHK(hipMemcpyAsync(costs, sa->nbr.cost, sizeof(uint64_t) * K, hipMemcpyDeviceToHost, sa->q.stream));
	std::vector<uint32_t> nd(K), dpos;
	std::vector<mgl_pk> dold, dnew;
	HIPCHK(hipMemcpyAsync(nd.data(), sa->nbr.ndiffs, sizeof(uint32_t) * K, hipMemcpyDeviceToHost, sa->q.stream));
	if (diffs) {
		dpos.resize(K * MGL_MAX_DIFFS); dold.resize(K * MGL_MAX_DIFFS); dnew.resize(K * MGL_MAX_DIFFS);
		HIPCHK(hipMemcpyAsync(dpos.data(), sa->nbr.dpos, sizeof(uint32_t) * dpos.size(), hipMemcpyDeviceToHost, sa->q.stream));
		HIPCHK(hipMemcpyAsync(dold.data(), sa->nbr.dold, sizeof(mgl_pk) * dold.size(), hipMemcpyDeviceToHost, sa->q.stream));
		HIPCHK(hipMemcpyAsync(dnew.data(), sa->nbr.dnew, sizeof(mgl_pk) * dnew.size(), hipMemcpyDeviceToHost, sa->q.stream));
	}
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	for (size_t j = 0; j < K; j++) {
		if (ndiffs) ndiffs[j] = nd[j];
		if (!diffs) continue;
		for (size_t e = 0; e < nd[j] && e < diff_cap; e++) {
			mgl_diff* d = &diffs[j * diff_cap + e];
			const mgl_pk o = dold[j * MGL_MAX_DIFFS + e], w = dnew[j * MGL_MAX_DIFFS + e];
			d->position = dpos[j * MGL_MAX_DIFFS + e];
			d->old_packet.type = (uint8_t)mgl_pk_type(o); d->old_packet.dist = mgl_pk_dist(o); d->old_packet.len = (uint16_t)mgl_pk_len(o);
			d->new_packet.type = (uint8_t)mgl_pk_type(w); d->new_packet.dist = mgl_pk_dist(w); d->new_packet.len = (uint16_t)mgl_pk_len(w);
		}
	}
	return MGL_OK;
}

/* mgl_debug_dump's answers that are host values, not device memory: a buffer too small gets the size and nothing else */
static int dump_host(const void* v, size_t sz, void* out, size_t cap_bytes, size_t* bytes)
{
	*bytes = sz;
	if (cap_bytes >= sz) memcpy(out, v, sz);
	return MGL_OK;
}
/* test hook: raw copies of the incremental path's base structures (enum mgl_dump_selector) */
extern "C" int mgl_debug_dump(mgl_sa* sa, uint32_t what, void* out, size_t cap_bytes, size_t* bytes)
{
	if (!sa || !out || !bytes) return fail(MGL_EINVAL, "null argument");
	if (what == MGL_DUMP_ALLOCATIONS) { /* on every handle */
		const uint64_t v[2] = { sa->own.live, sa->own.live_bytes };
		return dump_host(v, sizeof v, out, cap_bytes, bytes);
	}
	if (!sa->incremental && what != MGL_DUMP_WINDOWS && what != MGL_DUMP_SOFT_ENDS) return fail(MGL_EINVAL, "mgl_debug_dump: handle runs the full-walk engine");
	HIPCHK(hipSetDevice(sa->device));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	const Base2& b = sa->b2;
	const MatchIndex& ix = sa->ix;
	const size_t K = sa->cfg.neighbours_per_step, n1 = sa->n - 1;
	const void* src = nullptr;
	size_t sz = 0;
	uint32_t top = 0;
	if (sa->incremental) HIPCHK(hipMemcpy(&top, b.pool_top, sizeof top, hipMemcpyDeviceToHost));
	switch (what) {
	case MGL_DUMP_CHAIN_OFF: src = b.ch_off; sz = sizeof(uint32_t) * sa->ctx.L.total; break;
	case MGL_DUMP_CHAIN_LEN: src = b.ch_len; sz = sizeof(uint32_t) * sa->ctx.L.total; break;
	case MGL_DUMP_CHAIN_POS: src = b.ch_pos; sz = sizeof(uint32_t) * (size_t)top; break;
	case MGL_DUMP_CHAIN_EV: src = b.ch_ev; sz = sizeof(uint16_t) * (size_t)top; break;
	case MGL_DUMP_ONWALK: src = b.onwalk; sz = sizeof(uint64_t) * b.nw0; break;
	case MGL_DUMP_SPECIAL: src = b.sp0; sz = sizeof(uint64_t) * b.nw0; break;
	case MGL_DUMP_SPECIAL_STATE: src = b.sp_state; sz = sizeof(uint32_t) * 8 * (size_t)sa->n; break;
	case MGL_DUMP_CHECKPOINTS: src = b.ck_probs; sz = sizeof(uint16_t) * (size_t)b.nck * b.ck_elems; break;
	case MGL_DUMP_CHAIN_CAP: src = b.ch_cap; sz = sizeof(uint32_t) * sa->ctx.L.total; break;
	case MGL_DUMP_PHASE_CYCLES: src = sa->d_prof; sz = src ? sizeof(unsigned long long) * (64 + 2 * K) : 0; break;
	case MGL_DUMP_STEP_COUNTS: { /* last, then live */
		StepCounts v[2];
		*bytes = sizeof v;
		if (cap_bytes < sizeof v) return fail(MGL_ERANGE, "mgl_debug_dump: buffer too small");
		HIPCHK(hipMemcpy(&v[0], &sa->d_counts[1], sizeof(StepCounts), hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(&v[1], &sa->d_counts[0], sizeof(StepCounts), hipMemcpyDeviceToHost));
		return dump_host(v, sizeof v, out, cap_bytes, bytes);
	}
	case MGL_DUMP_PBUILD_TOTALS: src = sa->pb.acc; sz = src ? offsetof(PbAcc, left) : 0; break;
	case MGL_DUMP_BUCKET_OFF: src = ix.bucket_off; sz = sizeof(uint32_t) * 65537; break;
	case MGL_DUMP_BUCKET_POS: src = ix.bucket_pos; sz = sizeof(uint32_t) * n1; break;
	case MGL_DUMP_APPLY_HDR: src = sa->ab.hdr; sz = src ? sizeof(ApplyHdr) : 0; break;
	case MGL_DUMP_PICK_RECORDS: src = sa->d_pickrec; sz = src ? sizeof(uint4) * K : 0; break;
	case MGL_DUMP_CONTROL: src = sa->base.ctl; sz = sizeof(Control); break;
	case MGL_DUMP_QUAD_POS: src = ix.quad_pos; sz = sizeof(uint32_t) * n1; break;
	case MGL_DUMP_QUAD_NEXT: src = ix.quad_nx; sz = sizeof(uint16_t) * n1; break;
	case MGL_DUMP_WINDOWS: src = sa->nbr.win; sz = sizeof(uint32_t) * 2 * K; break;
	case MGL_DUMP_SOFT_ENDS: src = sa->nbr.win2; sz = sizeof(uint32_t) * K; break;
	case MGL_DUMP_COSTS: src = sa->nbr.cost; sz = sizeof(uint64_t) * K; break;
	case MGL_DUMP_JOURNAL_LENS: src = sa->nbr.ndiffs; sz = sizeof(uint32_t) * K; break;
	case MGL_DUMP_WALKED: src = sa->nbr.walked; sz = sizeof(uint32_t) * K; break;
	case MGL_DUMP_PICK_HINTS: src = sa->d_pick_hint; sz = src ? K : 0; break;
	case MGL_DUMP_PICK_ORDER: src = sa->d_pick_order; sz = src ? sizeof(uint32_t) * K : 0; break;
	case MGL_DUMP_PICKSTATE: src = sa->d_pickstate; sz = src ? sizeof(uint4) * 2 * K : 0; break;
	case 30: case 31: case 32: case 33: case 34: case 35: src = ix.xpos[what - MGL_DUMP_XPOS_BASE]; sz = sizeof(uint32_t) * n1; break;
	case 40: case 41: case 42: case 43: case 44: case 45: src = ix.xrank[what - MGL_DUMP_XRANK_BASE]; sz = src ? sizeof(uint32_t) * n1 : 0; break;
	case 50: case 51: case 52: case 53: case 54: case 55: src = ix.xrun[what - MGL_DUMP_XRUN_BASE]; sz = src ? sizeof(uint32_t) * n1 : 0; break;
	case 60: case 61: case 62: case 63: case 64: case 65: src = ix.xnxb[what - MGL_DUMP_XNEXT_BASE]; sz = n1; break;
	case MGL_DUMP_OCT_POS: src = ix.oct_pos; sz = sizeof(uint32_t) * n1; break;
	case MGL_DUMP_OCT_RANK: src = ix.oct_rank; sz = sizeof(uint32_t) * n1; break;
	case MGL_DUMP_OCT_RUN: src = ix.oct_run; sz = sizeof(uint32_t) * n1; break;
	case MGL_DUMP_OCT_NEXT8: src = ix.oct_nx8; sz = sizeof(uint64_t) * n1; break;
	case MGL_DUMP_HEX_POS: src = ix.hex_pos; sz = sizeof(uint32_t) * n1; break;
	case MGL_DUMP_HEX_RANK: src = ix.hex_rank; sz = sizeof(uint32_t) * n1; break;
	case MGL_DUMP_HEX_RUN: src = ix.hex_run; sz = sizeof(uint32_t) * n1; break;
	case MGL_DUMP_HEX_NEXT8: src = ix.hex_nx8; sz = sizeof(uint64_t) * n1; break;
	case MGL_DUMP_BATCH_COUNTS: {
		const uint64_t v[3] = { sa->batch_accepts, sa->batch_fallbacks, sa->batch_early_giveups };
		return dump_host(v, sizeof v, out, cap_bytes, bytes);
	}
	case MGL_DUMP_BATCH_HDR: src = sa->batch.hdr; sz = sizeof(BatchHdr); break;
	case MGL_DUMP_BATCH_ACC: src = sa->batch.acc; sz = sizeof(BatchAcc); break;
	case MGL_DUMP_CHAIN_INDEX: src = b.ch_sb; sz = sizeof(uint32_t) * (size_t)b.ck_elems * b.sb_stride; break;
	case MGL_DUMP_GIVEUP_SITES: src = sa->lim.why; sz = sizeof(uint32_t); break; /* cleared below */
	case MGL_DUMP_POOL_TOP: src = b.pool_top; sz = sizeof(uint32_t); break;
	case MGL_DUMP_INDEX_GEOMETRY: {
		const uint32_t v[3] = { b.sb_shift, b.nsb, b.sb_stride };
		return dump_host(v, sizeof v, out, cap_bytes, bytes);
	}
	default: return fail(MGL_EINVAL, "mgl_debug_dump: unknown selector");
	}
	*bytes = sz;
	if (sz > cap_bytes) return fail(MGL_ERANGE, "mgl_debug_dump: buffer too small");
	if (sz) HIPCHK(hipMemcpy(out, src, sz, hipMemcpyDeviceToHost));
	if (what == MGL_DUMP_GIVEUP_SITES) HIPCHK(hipMemset(sa->lim.why, 0, sizeof(uint32_t)));
	return MGL_OK;
}

/* MGL_KEY_LIMIT: limit `id` of the in-place accepts := v (at most the compiled / allocated one); id 0: all back to their defaults */
static int set_limit(mgl_sa* sa, uint32_t id, uint64_t v)
{
	if (!sa->incremental || !sa->lim.why) return fail(MGL_EINVAL, "mgl_debug_set: no in-place accept on this handle");
	HIPCHK(hipSetDevice(sa->device));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	if (id == 0) {
		if (v) return fail(MGL_EINVAL, "mgl_debug_set: limit id 0 takes value 0 (restore the defaults)");
		for (uint32_t i = 1; i < MGL_LIM_COUNT; i++) sa->lim.v[i] = i == MGL_LIM_SOFT_REACH ? 0u : sa->lim_max.v[i];
	} else {
		if (id >= MGL_LIM_COUNT || v > sa->lim_max.v[id]) return fail(MGL_EINVAL, "mgl_debug_set: unknown limit, or a value above the compiled / allocated one");
		sa->lim.v[id] = (uint32_t)v;
	}
	HIPCHK(hipMemset(sa->lim.why, 0, sizeof(uint32_t)));
	return MGL_OK;
}
/* MGL_KEY_PICK_HINTS, the test of k_pick_order: overwrite the hint bytes (0: all 0, 1: all 1, 2: alternating, else: random from `value`) and make the order again */
static int set_pick_hints(mgl_sa* sa, uint64_t value)
{
	if (!sa->d_pick_order) return fail(MGL_EINVAL, "mgl_debug_set: no launch order on this handle");
	const uint32_t K = sa->cfg.neighbours_per_step, slices = nbr_slices(sa);
	std::vector<unsigned char> h(K);
	uint64_t x = value;
	for (uint32_t j = 0; j < K; j++) {
		x = x * 6364136223846793005ull + 1442695040888963407ull;
		h[j] = value == 0 ? 0 : value == 1 ? 1 : value == 2 ? (unsigned char)(j & 1u) : (unsigned char)((x >> 40) % 3u); /* any non-zero byte is a picking neighbour */
	}
	HIPCHK(hipSetDevice(sa->device));
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	HIPCHK(hipStreamSynchronize(sa->q.stream2));
	HIPCHK(hipMemcpy(sa->d_pick_hint, h.data(), K, hipMemcpyHostToDevice));
	hipLaunchKernelGGL(k_pick_order, dim3(slices), dim3(1024), 0, sa->q.stream, (const unsigned char*)sa->d_pick_hint, sa->d_pick_order, K, slices);
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(sa->q.stream));
	return MGL_OK;
}
/* diagnostic knobs (tools/, tests/): enum mgl_debug_key */
extern "C" int mgl_debug_set(mgl_sa* sa, uint32_t key, uint64_t value)
{
	if (!sa) return fail(MGL_EINVAL, "null handle");
	switch (key) {
	case MGL_KEY_DIAG_STOP: sa->ctx.diag_stop = (uint32_t)value; return MGL_OK;
	case MGL_KEY_PBUILD_FIX: sa->pb.force_fix = (uint32_t)value; return MGL_OK;
	case MGL_KEY_LIST_CAP: /* below what was allocated: pushes neighbours into the second pass */
		if (value < 8 || value > sa->chg_cap || (value & 7u)) return fail(MGL_EINVAL, "mgl_debug_set: list capacity must be a multiple of 8 within the allocated one");
		sa->big.chg_cap = (uint32_t)value;
		return MGL_OK;
	case MGL_KEY_ROLLBACKS: sa->force.rollbacks = (uint32_t)value; return MGL_OK;
	case MGL_KEY_COUNT_TRAFFIC:
		if (!sa->d_traffic) return fail(MGL_EINVAL, "mgl_debug_set: no split neighbour evaluation on this handle");
		sa->count_traffic = value != 0;
		return MGL_OK;
	case MGL_KEY_BATCH_FAIL: /* low word: how many batch accepts; high word 0: before a chain is touched, n: behind the n-th context's rewrite */
		sa->force.batch_late = (uint32_t)(value >> 32);
		sa->force.batch_fail = (uint32_t)value;
		if (sa->force.batch_late && !sa->force.batch_fail) sa->force.batch_fail = 1;
		return MGL_OK;
	case MGL_KEY_LIMIT: return set_limit(sa, (uint32_t)(value & 0xFFu), value >> 8);
	case MGL_KEY_BIG_WAVES: /* the block size of the second-pass launch and nothing else */
		if (value != 1 && value != 2 && value != MGL_BIG_WAVES) return fail(MGL_EINVAL, "mgl_debug_set: 1, 2 or MGL_BIG_WAVES wavefronts");
		sa->big_waves = (uint32_t)value;
		return MGL_OK;
	case MGL_KEY_CROSS_NOMEM: sa->force.xo_nomem = (uint32_t)value; return MGL_OK;
	case MGL_KEY_PICK_HINTS: return set_pick_hints(sa, value);
	case MGL_KEY_COSTMAP_NOMEM: sa->force.cm_nomem = (uint32_t)value; return MGL_OK;
	case MGL_KEY_PROBE_FORM:
		if (value > 1) return fail(MGL_EINVAL, "mgl_debug_set: probe form 0 (batched) or 1 (in place)");
		sa->probe_form = (uint32_t)value;
		return MGL_OK;
	default: return fail(MGL_EINVAL, "mgl_debug_set: unknown key");
	}
}

#include "mgl_exchange.inc"
