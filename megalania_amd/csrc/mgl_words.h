/* The small control blocks that the kernels and the host share, one struct per block.  Plain C: the .hip files use it and a
 * host C compiler can read it (tests/test_debug_words_cpu.py prints the layouts from it and holds megalania_amd/binding.py's
 * dtypes against them).  Every block is one element of its struct, allocated zeroed; mgl_debug_dump hands them out raw. */
#ifndef MGL_WORDS_H
#define MGL_WORDS_H
#include <stdint.h>

#ifdef __cplusplus
#define MGL_WORDS_SIZE(T_, n_) static_assert(sizeof(T_) == (n_), #T_ ": layout")
#else
#define MGL_WORDS_SIZE(T_, n_) _Static_assert(sizeof(T_) == (n_), #T_ ": layout")
#endif

/* BulkBuf::hdr: a bulk step's totals (mgl_kernels4.hip), summed by its kernels and folded into Control when the step closes */
typedef struct BulkHdr {
	unsigned long long acceptable; /* neighbours the accept rule lets through: entries of the candidate list */
	unsigned long long taken;      /* of those, the ones the selection took */
	unsigned long long valid;      /* neighbours that were generated and costed */
	unsigned long long walked;     /* packets their window walks went over */
	unsigned long long improving;  /* candidates cheaper than the base */
	unsigned long long dropped;    /* neighbours dropped (journal too long, walks that did not meet) */
	unsigned long long min_key;    /* smallest taken key; ~0 between steps */
	unsigned long long pad;
} BulkHdr;
MGL_WORDS_SIZE(BulkHdr, 64);

/* BatchHdr::status: every kernel of the batch accept looks here first, the host reads it back once per bulk step */
#define MGL_BATCH_NONE 0u    /* the step took no move: nothing to do */
#define MGL_BATCH_BEGAN 1u   /* a batch accept is under way; read back by the host: it gave up behind its commit, the rebuild finishes the step */
#define MGL_BATCH_REBUILD 2u /* left to the rebuild: more moves than a batch accept handles, or it gave up before anything was touched */
#define MGL_BATCH_DONE 3u    /* the moves are in */
/* BatchHdr::failed */
#define MGL_BATCH_FAIL_WALK 1u     /* a walk gave up */
#define MGL_BATCH_FAIL_INVALID 2u  /* a walk met an invalid packet */
#define MGL_BATCH_FAIL_CLUSTERS 4u /* the clusters gave up */

/* BatchBuf::hdr (mgl_kernels5.hip).  The host reads back status .. acceptable. */
typedef struct BatchHdr {
	uint32_t status;        /* MGL_BATCH_NONE / BEGAN / REBUILD / DONE */
	uint32_t clusters;      /* clusters of taken neighbours */
	uint32_t n_ins;         /* inserted events of the combined lists */
	uint32_t n_rem;         /* removed events of the combined lists */
	uint32_t failed;        /* MGL_BATCH_FAIL_* seen by a kernel before anything was touched */
	uint32_t journal;       /* journal entries of all clusters */
	uint32_t unused6;       /* cleared with the rest, never written */
	uint32_t acceptable;    /* acceptable neighbours of this step: the host sizes the next step's selection by it */
	uint32_t runs;          /* runs on BatchBuf::runs (k_batch_ckpt patches the dense checkpoints along them) */
	uint32_t force_early;   /* test hook (MGL_KEY_BATCH_FAIL): give up at the top of k_batch_chains */
	uint32_t touched;       /* contexts that have events: entries of BatchBuf::touched */
	uint32_t unused11;
	uint32_t force_reached; /* test hook: contexts that got as far as force_late asks */
	uint32_t force_late;    /* test hook: give up behind the force_late-th context's rewrite */
	uint32_t unused14, unused15;
} BatchHdr;
MGL_WORDS_SIZE(BatchHdr, 64);

/* BatchBuf::cl: MGL_CL_WORDS u32 per cluster.  Index constants, not a struct: the kernels index the words in 32-bit
 * arithmetic, and a struct's 64-bit element index would change their instructions. */
#define MGL_CL_WORDS 8u
#define MGL_CL_FIRST 0u   /* first entry of the merged journal */
#define MGL_CL_ENTRIES 1u /* journal entries */
#define MGL_CL_N_INS 2u   /* staged inserted events */
#define MGL_CL_N_REM 3u   /* staged removed events */
#define MGL_CL_OPS 4u     /* bitmap / state-record ops */

/* BatchBuf::acc: the step's changes, summed by atomics */
typedef struct BatchAcc {
	long long cost;    /* cost change summed by k_batch_chains */
	long long direct;  /* direct-bit cost change */
	long long packets; /* packets on the walk, change */
	long long pad;
} BatchAcc;
MGL_WORDS_SIZE(BatchAcc, 32);

/* ApplyHdr::walk_cycles2: the low bits are cycles, the rest the walk's iteration count */
#define MGL_APPLY_GUARD_SHIFT 20
#define MGL_APPLY_CYCLES_MASK 0xFFFFFu

/* ApplyBuf::hdr (mgl_kernels3.hip; the batch accept uses the cursors too).  The cycle words are written with
 * MGL_KEY_DIAG_STOP = 50 only. */
typedef struct ApplyHdr {
	uint32_t n_ins;           /* inserted events of the accepted neighbour */
	uint32_t n_rem;           /* removed events */
	uint32_t n_tctx;          /* touched contexts; 0 when the walk gave up */
	uint32_t first_pos;       /* first journal position */
	uint32_t jobs_b;          /* copy jobs of pass B (save the old entries) */
	uint32_t jobs_c;          /* copy jobs of pass C (write the new ones) */
	uint32_t span_used;       /* span area entries used */
	uint32_t scratch_used;    /* scratch entries used */
	uint32_t stage_cycles[5]; /* k_apply_chains: the slowest workgroup's cycles per stage */
	uint32_t walk_cycles0;    /* k_apply_walk: cycles of its three stretches */
	uint32_t walk_cycles1;
	uint32_t walk_cycles2;    /* cycles & MGL_APPLY_CYCLES_MASK | iterations << MGL_APPLY_GUARD_SHIFT */
} ApplyHdr;
MGL_WORDS_SIZE(ApplyHdr, 64);

/* PBuild::acc: the parallel builder's totals (mgl_pbuild.hip) */
typedef struct PbAcc {
	unsigned long long cost;       /* the slab's exact cost */
	unsigned long long packets;    /* packets on the walk */
	unsigned long long ctx_state;  /* final LZMA state */
	unsigned long long dists[4];   /* final rep distances */
	unsigned long long redone;     /* chain segments pb_sim_fix redid */
	unsigned long long left;       /* chain segments pb_sim left to it */
} PbAcc;
MGL_WORDS_SIZE(PbAcc, 72);

/* The step counters: [0] live (zero between steps), [1] the last finished step's or mgl_neighbours call's */
typedef struct StepCounts {
	uint32_t second_pass;  /* neighbours on the second-pass list (first-pass overflow) */
	uint32_t last_resort;  /* neighbours on the last-resort list (second-pass overflow) */
	uint32_t spill_slots;  /* spill slots handed out */
	uint32_t repair_picks; /* repair picks */
	uint32_t unused4;      /* always zero */
	uint32_t cancelled;    /* event pairs the window walks of the costed neighbours left out of their change lists (0 under MGL_NO_EVCANCEL=1) */
	uint32_t unused6, unused7;
} StepCounts;
MGL_WORDS_SIZE(StepCounts, 32);

#endif /* MGL_WORDS_H */
