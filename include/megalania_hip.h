/*
 * megalania_hip.h -- C ABI of the MI355X SA hot path (libmegalania_hip.so).
 *
 * Drop-in boundary for blackle/Megalania's simulated-annealing loop.  Everything here is
 * plain C: pointers, sizes, integer status codes.  The library owns all device memory; the
 * caller owns every host buffer it passes in.  One host thread per mgl_sa handle (the
 * reference is single-threaded: global rand(), stateful TopKPacketFinder).
 *
 * What each entry point replaces in the reference (paths relative to its src/):
 *
 *   mgl_sa_create     main.c:44-51   lzma_state_init + packet_enumerator_new (match index,
 *                                    substring_enumerator.c:26-47) + top_k_packet_finder_new(20)
 *                                    + packet_slab_new (all-literal, packet_slab.c:15-35)
 *   mgl_sa_begin_epoch main.c:69-77  fresh slab per epoch (all-literal, or a copy of best)
 *   mgl_sa_run        main.c:78-102  the hot loop: packet_slab_neighbour_generate
 *                                    (packet_slab_neighbour.c:154-173: prefix cost, mutate,
 *                                    top-K pick, repair, total perplexity), accept / undo
 *   mgl_sa_best       main.c:91      packets_best, handed back in the reference's own
 *                                    12-byte LZMAPacket layout (lzma_packet.h:13-17) so that
 *                                    main.c:110-119 (header + range coder) emits it unchanged
 *   mgl_cost_slab     the loop of main.c:116-118 run with perplexity_encoder
 *                                    (perplexity_encoder.c:6-17) instead of range_encoder
 *   mgl_top_k         top_k_packet_finder_find/pop (top_k_packet_finder.c:120-138)
 *   mgl_substrings    substring_enumerator_for_each (substring_enumerator.c:85-105)
 *   mgl_sa_destroy    main.c:107-108,121 the matching frees
 *   mgl_props_sweep   no reference counterpart (lc = lp = pb = 0 are fixed there, main.c:45): one parse costed
 *                                    under every supported lc/lp/pb at once
 *   mgl_cost_map      no reference counterpart (perplexity_encoder.c:6-17 keeps one sum): the cost of a parse per byte,
 *                                    per coder and per packet type
 *   mgl_crossover, mgl_sa_cross_best, mgl_sa_exchange_cross, mgl_sa_exchange_cross_all
 *                     no reference counterpart (the reference runs one chain): several valid parses recombined region
 *                                    by region between the positions where their walks agree; the last one crosses the
 *                                    distinct best slabs of all chains (mgl_slab_hash, mgl_comm_allgather_u64 serve it)
 *   mgl_sa_set_focus, mgl_sa_focus, mgl_focus_slice
 *                     no reference counterpart (packet_slab_neighbour.c:162-163 draws its target over the whole slab): a
 *                                    step's targets confined to a byte window, and the rule that hands every chain its slice
 *   mgl_sa_set_target_weights, mgl_sa_weight_targets_by_cost, mgl_sa_target_weights, mgl_weight_value
 *                     no reference counterpart: a step's targets drawn in proportion to a weight per input byte, the
 *                                    weights the caller's or the cost map of a slab
 *   mgl_cost_map_live, mgl_sa_set_live_weights, mgl_sa_live_weights
 *                     no reference counterpart: the cost map of the current slab read off the engine's event chains instead
 *                                    of walked, and target weights made again from it inside mgl_sa_run
 *   mgl_segment_cuts, mgl_props_sweep_spans, mgl_segment_partition, mgl_sa_segment_props
 *                     no reference counterpart: a parse cut into segments that each start from an LZMA2 state reset under
 *                                    their own lc/lp/pb, every candidate segment costed under every triple at once
 *   mgl_segment_reparse
 *                     no reference counterpart: the adaptive parse made again inside every segment, from its reset and
 *                                    under its own triple
 *
 * Error convention: the reference returns NULL / -1 / false and prints to stderr
 * (packet_slab.c:18-27, memory_mapper.c:12-31); here constructors return NULL and
 * operations return 0 or a negative MGL_E* code; mgl_last_error() has the text.
 * Nothing aborts; HIP errors are translated.
 */
#ifndef MEGALANIA_HIP_H
#define MEGALANIA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGL_OK 0
#define MGL_EINVAL (-1)   /* bad argument */
#define MGL_ENOMEM (-2)   /* host or device allocation failed */
#define MGL_EDEVICE (-3)  /* HIP runtime error (no GPU, launch failure, ...) */
#define MGL_ERANGE (-4)   /* position not on the slab's walk / buffer too small */

/* lzma_packet.h:5-17 -- identical layout (type @0, dist @4, len @8, sizeof == 12). */
#ifndef MGL_NO_PACKET_TYPES
typedef struct {
	uint8_t type;   /* 1 LITERAL, 2 MATCH, 3 SHORT_REP, 4 LONG_REP */
	uint32_t dist;  /* MATCH: distance-1; LONG_REP: rep index 0..3 */
	uint16_t len;   /* LITERAL/SHORT_REP: 1; else 2..273 */
} mgl_packet;
/* lzma_state.h:53-57 */
typedef struct {
	uint8_t lc, lp, pb;
} mgl_properties;
#endif

typedef struct {
	uint64_t seed;                /* main.c:68 uses 1673551 */
	uint32_t neighbours_per_step; /* K: candidate neighbours costed per SA step */
	uint32_t top_k;               /* main.c:49 uses 20; at most 32 */
	uint32_t dict_limit;          /* candidates need dist < dict_limit; 0 = 0x400000, the
	                                 dictionary size lzma_header_encoder.c:16 writes */
	uint32_t max_bucket_scan;     /* cap on match-index hits scanned per top-K query, nearest
	                                 first; 0 = unlimited (the reference's behaviour) */
	uint64_t iters_per_epoch;     /* main.c:67 num_iters (defaults to the input size) */
	int32_t device;               /* HIP device ordinal */
	uint32_t flags;               /* MGL_F_* */
} mgl_sa_config;

#define MGL_F_TIMING 1u   /* record HIP events around every kernel launch of mgl_sa_run */
#define MGL_F_FULLWALK 2u /* cost every neighbour by walking the slab to the end (the simple,
                             slow engine) instead of incrementally against the base chains;
                             both engines return identical numbers */

#define MGL_F_PROFILE 4u  /* diagnostic: per-phase cycle counters in the neighbour kernels */
#define MGL_F_SERIAL_BUILD 16u /* derive the base structures with the one-wavefront builder only (diagnostic) */
#define MGL_F_POSITION_TARGETS 32u /* neighbour j's target from up to 32 uniform position draws (the first that is a packet start)
                              * instead of the default: a packet of the j-th of K equal slices of the walk's packets, by ordinal.
                              * Both make every packet equally likely (packet_slab_neighbour.c:162-163 draws a packet ordinal);
                              * the default keeps the K targets of one step apart, so that fewer improving neighbours of a step
                              * overlap and a bulk step takes 95 % of them instead of 80 % */
#define MGL_F_NO_SNAPSHOTS 8u /* do not keep device copies of the all-literal / best base structures:
                              * mgl_sa_begin_epoch then re-derives them from the slab (less memory, slower) */

typedef struct {
	uint64_t steps;          /* SA steps executed by this call */
	uint64_t evaluations;    /* neighbour evaluations that produced a cost (successful generates) */
	uint64_t failed;         /* generates that found no candidate (main.c:81-84 retries those) */
	uint64_t accepted;       /* steps that moved to a neighbour */
	uint64_t improved;       /* steps that set a new best */
	uint64_t current_cost;   /* perplexity of the current slab, 1/2048-bit units; 0 = none yet */
	uint64_t best_cost;
	uint64_t packets;        /* packets on the current slab's walk */
	uint64_t packets_evaluated; /* sum over evaluations of the packets costed (for B_eval) */
	double gpu_ms_total;     /* first launch -> last launch, HIP events on the library's stream */
	double gpu_ms_neighbours;/* sum over the timed steps of the neighbour kernels' span (MGL_F_TIMING: every step of a run of at most 16 steps,
	                          * every fourth step of a longer one, at most 512; `neighbour_launches` says how many were timed) */
	double gpu_ms_rebuild;   /* the same steps: decision / selection and accept (or rebuild) */
	uint64_t neighbour_launches;
	uint64_t full_rebuilds;       /* accepted steps whose base update fell back to a full rebuild */
	uint64_t fallback_neighbours; /* neighbours costed by the full-walk kernel instead of incrementally */
	uint64_t second_pass_neighbours; /* neighbours redone incrementally with their lists in global memory */
	uint64_t bulk_steps;          /* steps that took every window-best acceptable neighbour (mgl_sa_set_accept_mode) */
	uint64_t dropped_neighbours;  /* generates dropped because their journal outgrew 64 slab entries (counted in `failed`;
	                               * the reference's undo stack grows without bound, packet_slab_undo_stack.c:70-77) */
	uint64_t improving_neighbours;/* evaluations that cost less than the slab they were made from */
	uint64_t bulk_rollbacks;      /* bulk steps whose combined parse failed the after-the-fact validation and were taken back
	                               * as a whole (the safety net of the soft window ends; never seen) */
	uint64_t bulk_double_writes;  /* slab entries that two journals taken by one bulk step both wanted to change (detected entry
	                               * by entry with a compare-and-swap; such a step is taken back, so it also counts above) */
	double gpu_ms_sim;            /* sum over launches of the chain re-simulation kernel k_sim, the path's dominant kernel, each
	                               * bracketed by HIP events on the stream it runs on (MGL_F_TIMING; split launch form only) */
	uint64_t sim_launches;        /* the launches summed in gpu_ms_sim: one per slice of a step (the second pass re-simulates in place) */
	uint64_t sim_bytes_counted;   /* bytes of chain data (positions, events) and change lists k_sim's loads asked for, counted by
	                               * the kernel itself while mgl_debug_set key 4 is on (its algorithmic bytes; 0 otherwise) */
} mgl_sa_stats;

/* How a step of K costed neighbours moves the chain (the reference decides after every single
 * evaluation, main.c:86-96; see DESIGN.md section 4 for the batched rule both modes share):
 *   MGL_ACCEPT_SINGLE  the best acceptable neighbour of the step (base structures updated in place);
 *   MGL_ACCEPT_BULK    every acceptable neighbour that is the best of its own window -- hundreds to
 *                      thousands of moves per step while the slab is young -- followed by a parallel
 *                      rebuild of the base structures, which also yields the new slab's exact cost;
 *   MGL_ACCEPT_AUTO    (default) bulk steps while a step offers at least `bulk_threshold` improving
 *                      neighbours on average, single steps otherwise; decided per block of steps from
 *                      device counters only, so a run is reproducible.  bulk_threshold 0 = default. */
#define MGL_ACCEPT_AUTO 0
#define MGL_ACCEPT_SINGLE 1
#define MGL_ACCEPT_BULK 2

typedef struct {
	uint32_t position;
	mgl_packet old_packet;
	mgl_packet new_packet;
} mgl_diff;

typedef struct mgl_sa mgl_sa;

/* library / device */
const char* mgl_version(void);
const char* mgl_last_error(void);
int mgl_device_count(void);

/* lifecycle.  `data` is copied to the device; it is not retained. */
mgl_sa* mgl_sa_create(const uint8_t* data, size_t n, mgl_properties props, const mgl_sa_config* cfg);
void mgl_sa_destroy(mgl_sa* sa);

/* Slabs from outside, and the state after a refusal.  A slab the search did not make itself is checked on the device
 * before the search goes on from it: every entry on its walk is a packet (type 1..4; length 1 for LITERAL and SHORT_REP,
 * 2..273 for MATCH and LONG_REP; a LONG_REP index of at most 3) that ends inside the input, and every copy has its source
 * inside the input and the handle's dictionary window and reproduces the input byte for byte (rep packets by the rep
 * distances of the slab's own walk).  Entries off the walk are not looked at and come back entry for entry
 * (mgl_sa_current, mgl_sa_best, the crossover's child).  mgl_sa_run, however, re-joins the slab through entries that were
 * off its walk and takes them as they are, like the reference (packet_slab_neighbour.c:82-117, where a stale entry once
 * was a packet of a valid parse): a slab that a search is to start from must hold off its walk only what a search leaves
 * there -- a MATCH that reproduces the input, a LONG_REP of any index or a SHORT_REP that stays inside the input, a
 * literal.  mgl_sa_set_slab checks at once.  A best slab
 * from outside (mgl_sa_set_best, mgl_sa_adopt_best_packed, mgl_sa_cross_best, the exchanges) is accepted on its walk and
 * its cost -- which refuses what is no packet or does not fit -- and compared with the input bytes by the first
 * mgl_sa_begin_epoch(.., from_best) that starts from it, together with its cost.  The parity hooks (mgl_cost_slab,
 * mgl_props_sweep, mgl_final_state, mgl_crossover, ...) refuse an entry that is no packet or does not fit; whether they
 * look at the sources of the copies is left open.
 * After a refused mgl_sa_set_slab or a refused mgl_sa_begin_epoch(.., from_best) -- both MGL_EINVAL -- the handle is as
 * after mgl_sa_begin_epoch(phase, 0): the current slab is the all-literal one at its exact cost, no error is pending and
 * mgl_sa_run works.  mgl_sa_set_slab leaves the best slab and its cost untouched; mgl_sa_begin_epoch forgets the best slab
 * it refused: mgl_sa_best reports cost 0 ("none", which is what the next exchange publishes) and all-literal entries. */
/* Start an epoch (main.c:71-77): phase = the reference's `step` (0..2); from_best != 0 copies
 * the best slab into the current one, else the current slab becomes all-literal.  Resets the
 * within-epoch iteration counter and the current cost.  MGL_EINVAL: the best slab came from outside and is not a valid
 * parse of the input at the cost it came with (see above for the state this leaves). */
int mgl_sa_begin_epoch(mgl_sa* sa, unsigned phase, int from_best);
/* Replace the current slab (n entries, position-indexed).  Must be a valid parse: MGL_EINVAL otherwise (see above). */
int mgl_sa_set_slab(mgl_sa* sa, const mgl_packet* packets);
/* Replace the current slab by a greedy LZ parse made on the device (not in the reference, whose
 * search always starts from the all-literal slab, main.c:71; SURVEY 8f-3 "greedy seeding"): every
 * position independently receives the longest match among the `candidates` nearest earlier
 * occurrences of its two and of its four leading bytes inside the dictionary window (nearest
 * among equals; len 2 only up to distance 128, len 3 up to 2^14; dropped when the next position
 * would take a longer one), or a literal; the slab walk picks the parse out of them.  Same effect on the handle as mgl_sa_set_slab. */
int mgl_sa_seed_greedy(mgl_sa* sa, uint32_t candidates);
/* Optimal-parse seed (not in the reference; DESIGN.md section 10, megalania_amd/csrc/mgl_optimal.hip).  Pass p runs
 * a forward shortest path over every chunk of `chunk` bytes under static bit prices, then resolves the concatenated
 * parse against the true rep stack; pass 0 takes its prices from the greedy seed's parse (`cand` candidates), pass
 * p > 0 from pass p - 1's resolved parse, whose walk states also start pass p's chunks.  Every resolved parse is
 * costed exactly; the cheapest becomes the current slab, with the same effect on the handle as mgl_sa_seed_greedy.
 * Fields left 0 take the defaults; cand is at most 30 (MATCH candidates per order, as in mgl_sa_seed_greedy). */
#define MGL_OPT_MAX_PASSES 16
typedef struct {
	uint32_t passes; /* default 3, at most MGL_OPT_MAX_PASSES */
	uint32_t cand;   /* default 16 */
	uint32_t chunk;  /* bytes per DP chunk, default 4096, at least 512 */
} mgl_optimal_config;
typedef struct {
	uint32_t passes;     /* passes run */
	uint32_t best_pass;  /* the one whose parse became the current slab */
	uint64_t greedy_cost; /* exact cost of the greedy parse the first prices came from */
	uint64_t cost[MGL_OPT_MAX_PASSES];      /* exact cost of each resolved parse */
	uint64_t objective[MGL_OPT_MAX_PASSES]; /* sum of the DP's static prices over the chunks */
	double ms[MGL_OPT_MAX_PASSES];          /* device time of each pass: DP, resolution, costing, next prices */
} mgl_optimal_stats;
int mgl_sa_seed_optimal(mgl_sa* sa, const mgl_optimal_config* cfg, mgl_optimal_stats* stats);
/* Parity hook: one DP pass under explicit `prices` (nprices = 2 x number of probabilities, price of (slot, bit) at
 * 2 * slot + bit, cost units) with the LZMA initial state at every chunk start.  packets_out (n entries) is the
 * concatenated, unresolved parse: copies carry their type in the DP (LONG_REP, SHORT_REP, MATCH) and their absolute
 * distance (>= 1), positions off the parse hold literals; *objective = sum of its prices.  The SA state is untouched. */
int mgl_optimal_pass(mgl_sa* sa, const uint32_t* prices, size_t nprices, uint32_t cand, uint32_t chunk,
                     mgl_packet* packets_out, uint64_t* objective);
/* The prices mgl_sa_seed_optimal derives from a (valid) slab: 2 x number of probabilities u32. */
int mgl_optimal_prices(mgl_sa* sa, const mgl_packet* packets, uint32_t* prices_out, size_t nprices);
/* Adaptive-price optimal parse (not in the reference; DESIGN.md section 10, megalania_amd/csrc/mgl_adaptive.hip).  As
 * mgl_sa_seed_optimal, but a chunk's shortest path runs in segments under the live probability model: a chunk starts from
 * the walk state and the model that the previous parse's walk leaves there, each segment's DP looks `ahead` bytes past its
 * commit horizon of `segment` bytes, and the model is refreshed with the events of the packets a segment commits.  Pass 0
 * takes its chunk starts from the greedy parse (`cand` candidates), or with from_current from the current slab; pass p > 0
 * from pass p - 1's resolved parse.  Every resolved parse is costed exactly; the cheapest becomes the current slab, with
 * mgl_sa_seed_optimal's effect on the handle.  With from_current the current slab competes too (the re-parse: a caller may
 * alternate it with mgl_sa_run): if no pass beats it the handle is left untouched, stats->best_pass is UINT32_MAX, and
 * stats->greedy_cost holds the current slab's cost.  Fields left 0 take the defaults (segment 0: both segment and ahead).
 * The call is mgl_sa_seed_sweep with one variant, under the handle's finder and depth: MGL_ENOMEM, with the handle left
 * usable, where its buffers (about 34 bytes per input byte) do not fit the device. */
typedef struct {
	uint32_t passes;   /* default 3, at most MGL_OPT_MAX_PASSES */
	uint32_t cand;     /* default 16, at most 30 */
	uint32_t chunk;    /* default 4096, at least 512 */
	uint32_t segment;  /* commit distance, 0 = default (64, with ahead 128) */
	uint32_t ahead;    /* look-ahead past the commit horizon, at most 273 */
	uint32_t from_current; /* 0: pass 0 starts from the greedy parse; 1: from the current slab */
} mgl_adaptive_config;
int mgl_sa_seed_adaptive(mgl_sa* sa, const mgl_adaptive_config* cfg, mgl_optimal_stats* stats);
/* Parity hook: one pass from the chunk starts of `parse_in` (n entries; MGL_ERANGE unless a valid parse).  packets_out
 * (n entries) is the concatenated, unresolved parse in mgl_optimal_pass's form; *objective = the sum over the segments of
 * the prices of what each committed.  segment 0 takes the default commit distance.  The SA state is untouched.
 * MGL_ENOMEM as for mgl_sa_seed_adaptive (about 18 bytes per input byte here). */
int mgl_adaptive_pass(mgl_sa* sa, const mgl_packet* parse_in, uint32_t cand, uint32_t chunk, uint32_t segment, uint32_t ahead,
                      mgl_packet* packets_out, uint64_t* objective);
/* The adaptive parse under several settings at once.  Variant v is the parse that
 * mgl_sa_seed_adaptive({passes, cand, chunk, segment, ahead, from_current}) makes on a handle set to
 * mgl_sa_set_match_finder(finder, depth); all variants run through one launch of each stage, and results[v] (nvariants
 * entries, nullable) holds that call's passes, best_pass, greedy_cost, cost[] and objective[].  results[v].ms[p] is the
 * device time of pass p of the whole batch, *gpu_ms (nullable) that of the whole call.  The cheapest cost[p] over all
 * (variant, pass) -- ties to the lower variant, then to the lower pass -- becomes the current slab, with
 * mgl_sa_seed_adaptive's effect on the handle, and *best_variant (nullable) names its variant.  With from_current the
 * current slab competes: if nothing beats it the handle is left untouched and *best_variant is UINT32_MAX.  The handle's
 * own match-finder selection stays; the frontier's lists are made (or reused) at `depth` only if a variant asks for them.
 * MGL_EINVAL: no or more than MGL_SWEEP_MAX variants, an unknown finder, cand above 30, ahead above 273, chunk below 512,
 * more than 16 passes, depth above 4096.  MGL_ENOMEM: the buffers (about 26 bytes per input byte and variant, pass 0's
 * greedy parses included, and 8 per input byte for the kept parse) do not fit; the handle stays usable. */
#define MGL_SWEEP_MAX 64
typedef struct {
	uint32_t finder;   /* MGL_MF_NEAREST | MGL_MF_FRONTIER */
	uint32_t cand;     /* 0 = default 16, at most 30 */
	uint32_t segment;  /* 0 = default (64, with ahead 128), as in mgl_adaptive_config */
	uint32_t ahead;    /* at most 273 */
} mgl_parse_variant;
typedef struct {
	uint32_t passes;       /* default 3, at most MGL_OPT_MAX_PASSES */
	uint32_t chunk;        /* default 4096, at least 512; common to all variants */
	uint32_t depth;        /* frontier scan budget; 0 = the handle's (default 64), at most 4096 */
	uint32_t from_current; /* as in mgl_adaptive_config */
} mgl_parse_sweep_config;
int mgl_sa_seed_sweep(mgl_sa* sa, const mgl_parse_sweep_config* cfg, const mgl_parse_variant* variants, size_t nvariants,
                      mgl_optimal_stats* results /* nvariants entries */, uint32_t* best_variant, double* gpu_ms);
/* The same batch with a triple per variant: variant v is, integer for integer, the parse that
 * mgl_sa_seed_adaptive({passes, cand, chunk, segment, ahead, from_current = 0}) makes on a fresh handle created with
 * props[v] (same data, dict_limit and max_bucket_scan) and set to mgl_sa_set_match_finder(variants[v].finder, depth);
 * results[v] (nvariants entries, nullable) holds that call's passes, best_pass, greedy_cost, cost[] and objective[], every
 * cost exact under props[v], and ms[p] the batch's pass p.  The handle's own triple plays no part in any number.  The
 * cheapest cost[p] over all (variant, pass) wins -- costs under different triples compared as they are, ties to the lower
 * variant, then to the lower pass: *best_variant (nullable) names its variant and packets_out (n entries, nullable)
 * receives its resolved parse, entry for entry what mgl_sa_current returns on that fresh handle after its
 * mgl_sa_seed_adaptive.  The search state is untouched, as by the parity hooks (only the frontier's lists are made or
 * reused at `depth` if a variant asks for them): the handle cannot cost a slab under a foreign triple, so the winner is
 * not made current -- create a handle at the winning triple and give it the parse through mgl_sa_set_slab.
 * MGL_EINVAL: whatever mgl_sa_seed_sweep refuses, props == NULL, a triple mgl_sa_create refuses (lc + lp > 4 or pb > 4),
 * cfg->from_current != 0 (a current slab has a cost under one triple only).  MGL_ENOMEM as in mgl_sa_seed_sweep; a
 * variant's snapshots take ceil(n / chunk) models of its own triple's size. */
int mgl_parse_sweep_props(mgl_sa* sa, const mgl_parse_sweep_config* cfg, const mgl_parse_variant* variants,
                          const mgl_properties* props /* nvariants entries */, size_t nvariants,
                          mgl_optimal_stats* results /* nvariants entries */, uint32_t* best_variant, mgl_packet* packets_out,
                          double* gpu_ms);
/* The match finder of the parses above (not in the reference; DESIGN.md section 10, megalania_amd/csrc/mgl_matchfinder.hip):
 * where a node of the shortest path takes its MATCH sources from.  MGL_MF_NEAREST (default): the `cand` nearest earlier
 * positions with the same two bytes and the `cand` nearest with the same four.  MGL_MF_FRONTIER: for every achievable
 * length the nearest earlier position that reaches it -- the list an LZ optimiser gets from a binary-tree match finder
 * -- at most 60 entries per position, inside the handle's dictionary window.  Lengths 2..8 and 16 are one index look-up
 * each; a longer match is looked for among the positions that share 8 (16) bytes, nearest first, and `depth` bounds how
 * many of those are examined per position over all lengths (0 = default 64, at most 4096; with enough depth the list is
 * exact).  Applies to every later mgl_sa_seed_optimal, mgl_optimal_pass, mgl_sa_seed_adaptive and mgl_adaptive_pass on the
 * handle; `cand` then only shapes the greedy parse that pass 0 starts from.  The lists are made on the first such call
 * and kept (made again when the depth changes).  MGL_EINVAL: unknown finder, depth above 4096. */
#define MGL_MF_NEAREST 0
#define MGL_MF_FRONTIER 1
int mgl_sa_set_match_finder(mgl_sa* sa, int finder, uint32_t depth);
/* Parity hook: the MGL_MF_FRONTIER lists at `depth` (0 = default).  off_out (n + 1 entries, nullable): position i's
 * entries are [off[i], off[i + 1]); src_out / len_out (cap entries each, nullable): source position and match length
 * (capped at 273 and at the end of the input), lengths and distances rising along a list.  *count = off[n];
 * cap < *count: MGL_ERANGE with *count set.  gpu_ms (nullable): device time of the build that made the lists the handle
 * holds.  The SA state is untouched. */
int mgl_match_frontier(mgl_sa* sa, uint32_t depth, uint32_t* off_out, uint32_t* src_out, uint16_t* len_out, size_t cap,
                       size_t* count, double* gpu_ms);
/* Opt-in Metropolis accept rule (not in the reference, whose rule ignores the cost difference,
 * main.c:86).  temperature = 0 (default): the reference's rule.  temperature > 0, in
 * cost units (16384 per output byte, main.c:97): when the step's best neighbour does not improve,
 * the randomly drawn neighbour is accepted iff u < exp(-delta / t_eff) with u uniform, evaluated in
 * integers through the reference's log table (perplexity_table.h:4): delta * 2048 <=
 * t_eff * T[u], u in 1..2047, t_eff = temperature * (iters_per_epoch - i) / iters_per_epoch
 * (linear cooling inside the epoch).  Must be below 2^40. */
int mgl_sa_set_temperature(mgl_sa* sa, uint64_t temperature);
int mgl_sa_set_accept_mode(mgl_sa* sa, int mode, uint32_t bulk_threshold);
/* The modes of the steps of the last mgl_sa_run (0 single, 1 bulk), for replaying a run elsewhere; of a call of more
 * than 2^20 steps only the first 2^20 are kept.  In MGL_ACCEPT_AUTO the mode is chosen per block of 16 single (4 bulk)
 * steps; a block carries over from one mgl_sa_run call to the next, so the sequence of modes -- and with it the
 * trajectory -- does not depend on how a run is cut into calls; mgl_sa_begin_epoch, mgl_sa_set_slab, mgl_sa_seed_greedy
 * and mgl_sa_set_accept_mode start a fresh block whatever came before (bulk steps first, except single steps first
 * in an epoch that starts from the best slab). */
int mgl_sa_step_modes(mgl_sa* sa, uint8_t* modes_out, size_t cap, size_t* count);
/* Focus window (no reference counterpart: the reference draws its target over the whole slab, packet_slab_neighbour.c:162-163;
 * DESIGN.md sections 4 and 9).  While a window [lo, hi) is set, in byte positions, the K neighbours of a step take their targets
 * among the packets that start in [lo, hi) of the current walk: with a packet starts below lo and b below hi, neighbour j takes
 * a packet of the j-th of K equal slices of the ordinals [a, b), by the rule of the default targets applied to b - a (with fewer
 * than K packets in the window several neighbours share a target and differ by their streams).  Empty window -- no packet starts
 * in [lo, hi), the window lies inside one packet: the packet that covers lo is the only target (a := a - 1).  A neighbour never
 * writes below its target (packet_slab_neighbour.c:82-152 only move forward from it), so a search under a window leaves every
 * slab entry below lo untouched, current and best; entries at and above hi may change (a repair runs until it re-joins).
 * (0, 0) clears the window; (0, n) is a window and gives the trajectory of none.  Being byte positions, the window keeps its
 * meaning while the walk changes; it stays set across mgl_sa_run, mgl_sa_begin_epoch, mgl_sa_set_slab, the seeds and the
 * exchanges until it is changed, and mgl_neighbours honours it like mgl_sa_run, on both engines.  Slab, costs, RNG streams,
 * MGL_ACCEPT_AUTO's block and mgl_sa_stats are untouched.  MGL_EINVAL, handle unchanged: lo >= hi other than (0, 0), hi > n, a
 * handle created with MGL_F_POSITION_TARGETS (position draws have no ordinals to cut). */
int mgl_sa_set_focus(mgl_sa* sa, uint64_t lo, uint64_t hi);
/* The window in force (0, 0: none); packets (nullable) receives the b - a above on the current walk -- the walk's packets when
 * no window is set, 1 for an empty window. */
int mgl_sa_focus(mgl_sa* sa, uint64_t* lo, uint64_t* hi, uint64_t* packets);
/* host arithmetic only, no device involved: the window of chain `rank` of `world` in exchange round `round`, [B_rank, B_rank+1)
 * with, in even rounds, B_i = i n / world, and in odd rounds B_0 = 0, B_world = n, B_i = (2 i - 1) n / (2 world) between -- half
 * a slice further down, so that no boundary stays where it was.  In every round the slices tile [0, n) without overlap and
 * none is empty.  MGL_EINVAL: world == 0, rank >= world, n < 2 world. */
int mgl_focus_slice(uint64_t n, uint32_t world, uint32_t rank, uint64_t round, uint64_t* lo, uint64_t* hi);
/* Target weights, the soft form of the focus window (no reference counterpart; DESIGN.md sections 4 and 10,
 * megalania_amd/csrc/mgl_weights.hip).  While weights are set, the K neighbours of a step take their targets in proportion to a
 * weight per input byte.  All of it is exact integer arithmetic:
 *   - w[x], one uint32 per byte, S[x] = the sum of w below x (uint64); [lo, hi) = the focus window in force, [0, n) without one;
 *     W = S[hi] - S[lo].  W == 0: the step's targets are those of the rule without weights (under the window, if one is set).
 *   - Neighbour j draws v = a + (b > a ? u % (b - a) : 0) from slice [a, b) = [j W / K, (j + 1) W / K) of W, with
 *     u = draw 0 << 31 | draw 0xFFFFFFFF of its stream (62 bits: a slice can be wider than one draw; mgl_weight_value).
 *   - x is the byte of [lo, hi) with S[x] - S[lo] <= v < S[x + 1] - S[lo]; a byte of weight 0 is never drawn.
 *   - The target is the start of the packet that covers x on the current walk.  Under a window that start may lie below lo:
 *     then the first packet start inside [lo, hi) is the target, or, if the window holds none, the packet that covers lo (the
 *     focus window's own empty case).  So a search under a window still leaves every slab entry below lo untouched.
 * Being byte positions, the weights keep their meaning while the walk changes: they stay set across mgl_sa_run,
 * mgl_sa_begin_epoch, mgl_sa_set_slab, the seeds and the exchanges until they are replaced or cleared, and mgl_neighbours
 * honours them like mgl_sa_run, on both engines.  Slab, costs, RNG streams, MGL_ACCEPT_AUTO's block, the focus window and
 * mgl_sa_stats are untouched by setting or clearing them.  Device memory: 4 n + n / 8 bytes, the handle's while weights are set
 * (a prefix sum per 64 bytes, made once per call, never per step).
 * NULL clears.  MGL_EINVAL, handle and weights in force unchanged: sum >= 2^44, a handle created with MGL_F_POSITION_TARGETS.
 * MGL_ENOMEM, handle usable, no weights in force afterwards: the buffers (4 n + n / 8 bytes) do not fit. */
int mgl_sa_set_target_weights(mgl_sa* sa, const uint32_t* weights /* n entries */);
/* weights := cost map of `packets` (NULL: the current slab) under the handle's lc/lp/pb, + floor per byte; a slab that
 * mgl_cost_map refuses is refused with its code and the weights in force stay.  total (nullable) = map total + floor * n.
 * The map never leaves the device.  MGL_EINVAL also for floor > 2^32 - 1 - 2^20 (an entry would not fit) and a total >= 2^44;
 * MGL_ENOMEM from the map's own buffers (8 n bytes for the length of the call) leaves the weights in force as they were.
 * gpu_ms (nullable): device time of the map's two kernels. */
int mgl_sa_weight_targets_by_cost(mgl_sa* sa, const mgl_packet* packets, uint32_t floor, uint64_t* total, double* gpu_ms);
/* parity hook: weights_out (n entries, nullable), *total = S[n], *window = W under the focus in force; all 0 when none are set */
int mgl_sa_target_weights(mgl_sa* sa, uint32_t* weights_out, uint64_t* total, uint64_t* window);
/* host arithmetic only, no device: the value v neighbour j draws.  MGL_EINVAL: W == 0, W >= 2^44, K == 0, K > 2^20, j >= K, v NULL */
int mgl_weight_value(uint64_t W, uint32_t K, uint32_t j, uint64_t seed, uint64_t step, uint64_t* v);
/* Live target weights (no reference counterpart; DESIGN.md sections 4 and 10): the weights of
 * mgl_sa_weight_targets_by_cost(sa, NULL, floor, ..) made again inside mgl_sa_run, from the live cost map (mgl_cost_map_live;
 * the walk's map on the full-walk engine, the same integers).  The rule, with g = the handle's global step number (the steps
 * run since the handle was made):
 *   - When.  Before step g takes its targets the weights are refreshed if g % every == 0, or if the handle is stale: live
 *     weights were just enabled, or the current slab was replaced from outside a run since the last refresh
 *     (mgl_sa_begin_epoch, mgl_sa_set_slab, the seeds, an adopted re-parse).  Nothing else refreshes.  A refresh sets
 *     w[x] = live map[x] + floor of the slab as it stands before step g -- floor the configured one, or with floor_mean
 *     total / n of that very map, what mgl_sa_weight_targets_by_cost adds when handed total / n -- and makes the prefix sums
 *     and the window's weight as every setting of weights does.  So a trajectory does not depend on how it is cut into
 *     mgl_sa_run calls, and it is the trajectory of a caller who calls mgl_sa_weight_targets_by_cost before every such step.
 *   - MGL_LW_SINGLE_ONLY.  A step takes its targets by the weights only if it goes the single route; a bulk-route step uses
 *     the rule without weights and makes no refresh, and a refresh that falls due during bulk steps (the stale case
 *     included) happens before the first single step after them.  Under MGL_ACCEPT_SINGLE the flag changes nothing, under
 *     MGL_ACCEPT_BULK weights never apply, and under MGL_ACCEPT_AUTO they come on exactly when the device's own counters say
 *     the slab has stopped offering bulk_threshold improving neighbours per step -- reproducible for the reason AUTO is.
 *   - Sum.  A refresh whose weights sum to 2^44 or more leaves the steps up to the next refresh to the rule without weights
 *     and counts in `skipped`; the run does not fail.
 * mgl_neighbours honours the weights in force and never refreshes; mgl_sa_target_weights returns the last refresh's weights
 * (all 0 before the first).  The focus window composes as with any weights (W == 0: the rule without weights; nothing below
 * lo is written).  mgl_sa_set_target_weights and mgl_sa_weight_targets_by_cost turn live weights off (explicit weights
 * replace them); enabling live weights replaces explicit ones.  Slab, costs, RNG streams, MGL_ACCEPT_AUTO's block, the focus
 * window and mgl_sa_stats are untouched by enabling or disabling.  Device memory: the weights' 4 n + n / 8 bytes and 4 n for
 * the map's marks, the handle's while live weights are on.  A refresh costs one read-back (the window's 16 bytes with the
 * map's sums), as a block end costs one.
 * cfg == NULL: off, weights cleared.  MGL_EINVAL, handle unchanged: every == 0, unknown flags, and without floor_mean a
 * floor > 2^32 - 1 - 2^20 or floor * n >= 2^43; a handle created with MGL_F_POSITION_TARGETS.  MGL_ENOMEM: the buffers do not
 * fit; the handle stays usable with no weights in force. */
#define MGL_LW_SINGLE_ONLY 1u
typedef struct {
	uint32_t every;      /* steps between refreshes, >= 1 */
	uint32_t floor;      /* added per byte; ignored with floor_mean */
	uint32_t floor_mean; /* 1: floor = total / n of each refresh's map (what `cost:mean` adds) */
	uint32_t flags;      /* MGL_LW_* */
} mgl_live_weights_config;
typedef struct {
	uint64_t refreshes;  /* since enabled */
	uint64_t skipped;    /* refreshes whose sum reached 2^44: that interval ran by the rule without weights */
	uint64_t last_gstep, last_total; /* the last refresh: its step and its map's total */
	double gpu_ms;       /* device time of all refreshes: map, weights, prefix sums */
} mgl_live_weights_stats;
int mgl_sa_set_live_weights(mgl_sa* sa, const mgl_live_weights_config* cfg /* NULL: off, weights cleared */);
int mgl_sa_live_weights(mgl_sa* sa, mgl_live_weights_config* cfg_out, mgl_live_weights_stats* stats_out); /* every == 0: off */
/* Adopt a best slab found elsewhere (another chain / GPU): replaces best slab and best cost.
 * `perplexity` must be the slab's exact cost: the slab is walked on the device at once, which refuses (MGL_EINVAL, nothing
 * adopted) an entry that is no packet or does not fit, and a cost other than `perplexity`.  That walk does not look at the
 * bytes a copy copies: like a slab adopted from a peer, this one is compared with the input by the first
 * mgl_sa_begin_epoch(.., from_best) that starts from it, which refuses it then. */
int mgl_sa_set_best(mgl_sa* sa, const mgl_packet* packets, uint64_t perplexity);
/* ---- chains on several GPUs (no reference counterpart: the reference is one process; main.c:75-77 is what
 * an exchange feeds).  One chain per GPU / process; mgl_comm wraps one RCCL communicator (librccl is loaded on
 * first use).  Rank 0 calls mgl_comm_unique_id and hands the 128 bytes to the others by any means (a file, a
 * launcher's store); every rank then calls mgl_comm_init on its device. */
typedef struct mgl_comm mgl_comm;
int mgl_comm_unique_id(uint8_t id_out[128]);
int mgl_comm_init(mgl_comm** comm_out, const uint8_t id[128], int rank, int world, int device);
/* The same handle over a host shared-memory file instead of RCCL (no reference counterpart either): keys and the packed
 * slab are staged through `path` (a file on a memory-backed file system, e.g. under /dev/shm).  For chains that share one
 * GPU -- RCCL refuses two ranks per device -- and for boxes without RCCL; mgl_sa_exchange_best runs the same protocol over
 * it.  Rank 0 creates the file (replacing any left by an earlier run) and removes it in mgl_comm_destroy; the others wait
 * for a file that carries this run's `nonce` and `world` (any value all ranks of one run agree on, different from run to
 * run).  Waits -- here and in every exchange -- give up with MGL_EDEVICE after MGL_COMM_TIMEOUT_S seconds (default 600). */
int mgl_comm_init_shm(mgl_comm** comm_out, const char* path, uint64_t nonce, int rank, int world, int device);
/* host transport only, no device involved: the minimum over the ranks of one word each (the first half of an exchange) */
int mgl_comm_min_u64(mgl_comm* comm, uint64_t mine, uint64_t* min_out);
/* host transport only, no device involved: every rank's word in rank order (all_out: mgl_comm_world entries).  The collective
 * by which mgl_sa_exchange_cross_all publishes keys and slab hashes; its RCCL form (ncclAllGather) runs inside that call. */
int mgl_comm_allgather_u64(mgl_comm* comm, uint64_t mine, uint64_t* all_out);
void mgl_comm_destroy(mgl_comm* comm);
int mgl_comm_rank(const mgl_comm* comm);
int mgl_comm_world(const mgl_comm* comm);
/* One exchange: a single 8-byte ncclAllReduce(min) of (best_cost << 8 | rank), then ncclBroadcast of the
 * winner's best slab in its packed 8-byte device form, HBM to HBM over xGMI (the host transport stages both
 * through its file); chains whose own best is worse
 * adopt it as packets_best (mgl_sa_begin_epoch(.., from_best) continues from it and verifies it first).
 * winner_rank / winner_cost (nullable) receive the outcome; cost 0 = no chain has a best slab yet.
 * Collective: every rank of the communicator must call it. */
int mgl_sa_exchange_best(mgl_sa* sa, mgl_comm* comm, int* winner_rank, uint64_t* winner_cost);
/* Crossover of parses (no reference counterpart; DESIGN.md section 10, megalania_amd/csrc/mgl_crossover.hip).  Every parent
 * (n entries, position-indexed, a valid parse) is walked from position 0 with the LZMA initial state and a fresh model under
 * the handle's lc/lp/pb.  A position q is a joint if q = 0, q = n, or every parent starts a packet at q in the same walk state
 * (ctx_state and the four rep distances).  Boundaries: with grain <= 1 every joint; with grain g > 1 the joints that are the
 * first joint >= m g for some m >= 0, and n (a set: no boundary depends on an earlier one).  Between consecutive boundaries
 * b < b' the child takes, entry for entry (stale off-walk entries included), the parent whose packets starting in [b, b')
 * cost least along its own walk, ties to the lowest parent.  The child is a valid parse by construction; it can cost more
 * than its best parent, so it is costed exactly.  grain 0 = 64.
 * MGL_EINVAL: a null handle, parents or parent, fewer than 2 or more than MGL_XO_MAX_PARENTS parents; a parent that
 * mgl_cost_slab refuses is refused with mgl_cost_slab's code.  MGL_ENOMEM, with the handle left usable: the call's buffers
 * (about 36 bytes per input byte and parent, allocated per call and freed) do not fit the device. */
#define MGL_XO_MAX_PARENTS 8
typedef struct {
	uint32_t parents, grain;            /* as used (grain 0 -> 64) */
	uint64_t parent_cost[MGL_XO_MAX_PARENTS]; /* exact cost of each parent */
	uint64_t child_cost;                /* exact cost of the child */
	uint64_t predicted;                 /* sum over the regions of the winner's cost there (diagnostic: the child's model adapts
	                                     * along a mixed history, so its real cost differs) */
	uint64_t boundaries;                /* boundaries, 0 and n included: one more than there are regions */
	uint64_t regions_from[MGL_XO_MAX_PARENTS]; /* regions taken from each parent */
	uint32_t adopted;                   /* mgl_sa_cross_best / exchange: 0 own best kept, 1 the other slab adopted, 2 the child adopted */
	double gpu_ms;                      /* device time: walks, joints, boundaries, winners, scatter, the child's walk */
} mgl_cross_stats;
/* parity hook: SA state untouched; child_out (n entries) nullable */
int mgl_crossover(mgl_sa* sa, const mgl_packet* const* parents, size_t nparents, uint32_t grain, mgl_packet* child_out,
                  mgl_cross_stats* stats);
/* parents = (the handle's best slab, other).  Child strictly cheaper than both: it becomes the best slab at its exact cost (the
 * cost is verified; `other`'s copies, and so the child's, are compared with the input when an epoch first starts from it, as for
 * mgl_sa_set_best);  else other strictly cheaper than the best: adopted as mgl_sa_set_best does;  else nothing changes.  No best slab
 * yet: other is adopted (stats: parents 0, nothing was crossed; parent_cost[1] its cost).  The current slab and the run state are untouched
 * (mgl_sa_begin_epoch(.., from_best) continues from the new best slab). */
int mgl_sa_cross_best(mgl_sa* sa, const mgl_packet* other, uint32_t grain, mgl_cross_stats* stats);
/* mgl_sa_exchange_best's two collectives (min of cost << 8 | rank, broadcast of the winner's packed slab), then on every rank but the
 * winner mgl_sa_cross_best against the received slab, device to device.  Ranks may hold different best slabs afterwards, each no
 * dearer than the winner's.  What a rank adopts here came from a peer and is checked against the input when an epoch first starts
 * from it, as after mgl_sa_exchange_best.  stats (nullable): this rank's crossing; all zero on the winner.  Collective. */
int mgl_sa_exchange_cross(mgl_sa* sa, mgl_comm* comm, uint32_t grain, int* winner_rank, uint64_t* winner_cost, mgl_cross_stats* stats);
/* Parity hook (SA state untouched): the hash by which chains tell equal slabs from different ones without sending them.
 * h = sum over x < n of fin(packed[x] + (x + 1) * 0x9E3779B97F4A7C15) mod 2^64, packed = dist | len << 32 | type << 48 (the 8-byte
 * device form) and fin the splitmix64 finaliser, z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB,
 * z ^= z >> 31.  Every entry counts, stale off-walk ones too (the crossover copies entries verbatim).  packets NULL = the best
 * slab; MGL_EINVAL if there is none yet. */
int mgl_slab_hash(mgl_sa* sa, const mgl_packet* packets, uint64_t* hash);
/* The exchange that crosses the best slabs of all chains (collective; opt-in next to mgl_sa_exchange_best and
 * mgl_sa_exchange_cross).
 * (1) Every rank publishes key = (best_cost, or "none") << 8 | rank and mgl_slab_hash of its best slab: two all-gathers.
 * (2) Every rank makes the same selection: the ranks that hold a best slab in ascending key order, skipping a rank whose
 *     (cost, hash) an already selected rank has, at most MGL_XO_MAX_PARENTS of them.  D remain; parent p is the p-th, so the
 *     crossover's ties go to the cheaper chain.  A hash collision between different slabs of one cost can only drop a parent.
 * (3) D = 0: nothing happens.  D = 1: mgl_sa_exchange_best -- one broadcast, ranks with a dearer best slab or none adopt it
 *     (cross.parents = 0, cross.adopted = 1 on those ranks, cross.parent_cost[0] its cost).  D >= 2: every rank allocates mgl_crossover's buffers and one min
 *     of an ok flag follows; if any rank had no room all of them take the D = 1 path instead (fell_back = 1, still MGL_OK).
 *     Otherwise parent p's owner broadcasts its best slab into slot p of the crossover's slab buffer, device to device (the
 *     host transport stages through its file), and every rank runs mgl_crossover's kernels on the D parents.  A parent whose
 *     walked cost is not the cost its rank published: MGL_EINVAL, nothing adopted.
 * (4) The same on every rank: child_cost < parent_cost[0]: the child becomes the best slab (cross.adopted = 2);  else ranks
 *     whose best is dearer than parent 0, or that have none, adopt parent 0 (1);  else nothing changes (0).
 * What a rank adopts came from peers and is checked against the input when an epoch first starts from it, as after
 * mgl_sa_exchange_best.  The current slab and the run state are untouched.  grain as in mgl_crossover.  stats nullable. */
typedef struct {
	uint32_t chains_with_best;               /* ranks that published a best slab */
	uint32_t distinct;                       /* D: the parents */
	uint32_t parent_rank[MGL_XO_MAX_PARENTS]; /* the rank that owns each parent */
	uint32_t own_parent;                     /* this rank's parent index, UINT32_MAX if it is none */
	uint32_t fell_back;                      /* 1: a rank could not allocate, everybody took the D = 1 path */
	mgl_cross_stats cross;                   /* the crossing, the same on every rank but gpu_ms (nothing crossed: zero but `adopted` and parent_cost[0]) */
} mgl_cross_all_stats;
int mgl_sa_exchange_cross_all(mgl_sa* sa, mgl_comm* comm, uint32_t grain, mgl_cross_all_stats* stats);
/* The same hand-over through host memory in the packed device form (dist | len << 32 | type << 48, 8 bytes
 * per position), for transports other than RCCL.  Adopting does not verify; see mgl_sa_exchange_best. */
int mgl_sa_best_packed(mgl_sa* sa, uint64_t* packed_out, uint64_t* perplexity_out);
int mgl_sa_adopt_best_packed(mgl_sa* sa, const uint64_t* packed, uint64_t perplexity);

/* Run `steps` SA steps, each costing cfg.neighbours_per_step neighbours.  Entirely
 * device-resident; the call returns after the last kernel has completed. */
int mgl_sa_run(mgl_sa* sa, uint64_t steps, mgl_sa_stats* stats);
/* Current / best slab, n entries each, reference layout. */
int mgl_sa_current(mgl_sa* sa, mgl_packet* packets_out, uint64_t* perplexity_out);
int mgl_sa_best(mgl_sa* sa, mgl_packet* packets_out, uint64_t* perplexity_out);

/* Parity hooks (each leaves the SA state untouched). */
/* Cost a whole slab from byte 0.  per_packet_cumulative (nullable) receives one running
 * total per walked packet; npackets (nullable) their number. */
int mgl_cost_slab(mgl_sa* sa, const mgl_packet* packets, uint64_t* total,
                  uint64_t* per_packet_cumulative, size_t* npackets);
/* Exact cost of one parse under every supported lc/lp/pb (no reference counterpart; DESIGN.md section 10,
 * megalania_amd/csrc/mgl_props.hip): the triples mgl_sa_create accepts, lc + lp <= 4 and pb <= 4, in the canonical
 * order `for lc in 0..4: for lp in 0..4-lc: for pb in 0..4`.  out[t].cost is what mgl_cost_slab returns for the same
 * slab on a handle created with out[t].props, and the call refuses exactly the slabs mgl_cost_slab refuses.
 * packets == NULL: the current slab.  cap < 75: MGL_ERANGE, *count = 75.  gpu_ms (nullable): device time of the sweep. */
#define MGL_PROPS_TRIPLES 75
typedef struct { mgl_properties props; uint64_t cost; } mgl_props_cost;
int mgl_props_sweep(mgl_sa* sa, const mgl_packet* packets, mgl_props_cost* out, size_t cap, size_t* count, double* gpu_ms);
/* Where a parse spends its bits (no reference counterpart; DESIGN.md section 10, megalania_amd/csrc/mgl_costmap.hip): the
 * exact cost of the slab per byte, per coder and per packet type, in the cost units of mgl_cost_slab (2048 per bit).
 *   - A parity hook like its neighbours: slab, costs, RNG streams, the block state of MGL_ACCEPT_AUTO, the focus window and
 *     mgl_sa_stats stay as they were.  Both engines (MGL_F_FULLWALK too).
 *   - The slab is walked from byte 0 with the LZMA initial state and a fresh model under `props` (NULL: the handle's).  A
 *     triple other than the handle's is allowed, exactly as in mgl_props_sweep; lc + lp > 4 or pb > 4 is MGL_EINVAL.
 *     packets == NULL: the current slab.  Off-walk entries are never looked at.
 *   - A slab that mgl_cost_slab refuses is refused with the same code, and nothing is written.
 *   - map_out (nullable): n entries.  A packet of exact cost c and length L that starts at p gives byte p + k the value
 *     c / L + (k < c % L ? 1 : 0): the entries of a packet sum to its cost, the whole map to report->total.  c < 2^20.
 *   - report (nullable): see below.  A coded bit belongs to the class its probability context lies in (the ranges are those
 *     of megalania_amd/csrc/mgl_model.h, L.total = MGL_OFF_LIT + (0x300 << (lc + lp))).
 *   - Device memory: 8 bytes per input byte for the length of the call (a mark per position and the map), allocated and
 *     freed by the call; MGL_ENOMEM, with the handle left usable, when they do not fit. */
#define MGL_CC_KIND       0  /* is_match, is_rep, is_rep_g0/g1/g2, is_rep0_long: contexts [0, MGL_OFF_LEN) */
#define MGL_CC_LITERAL    1  /* literal coder: contexts [MGL_OFF_LIT, L.total) */
#define MGL_CC_LENGTH     2  /* match length coder: [MGL_OFF_LEN, MGL_OFF_REP_LEN) */
#define MGL_CC_REP_LENGTH 3  /* rep length coder: [MGL_OFF_REP_LEN, MGL_OFF_DIST) */
#define MGL_CC_DISTANCE   4  /* pos_slot, pos_coder, align: [MGL_OFF_DIST, MGL_OFF_LIT) */
#define MGL_CC_DIRECT     5  /* direct bits: 2048 each, no context */
#define MGL_CC_CLASSES    6
typedef struct {
	uint64_t total, packets;                 /* what mgl_cost_slab returns for the same slab (under `props`) */
	uint64_t class_cost[MGL_CC_CLASSES];     /* sums to total */
	uint64_t class_bits[MGL_CC_CLASSES];     /* coded bits (events; direct bits for MGL_CC_DIRECT) */
	uint64_t type_cost[4], type_packets[4], type_bytes[4]; /* index = packet type - 1; costs sum to total, bytes to n */
	double gpu_ms;                           /* device time of the call's kernels; 0 from the host form */
} mgl_cost_report;
int mgl_cost_map(mgl_sa* sa, const mgl_packet* packets, const mgl_properties* props, uint32_t* map_out, mgl_cost_report* report);
/* The cost map of the current slab without the walk (no reference counterpart; DESIGN.md section 10,
 * megalania_amd/csrc/mgl_costmap_live.hip).  map_out (n entries, nullable) and every field of report (nullable) except gpu_ms
 * equal, integer for integer, what mgl_cost_map(sa, NULL, NULL, map_out, report) returns at that moment: the current slab
 * under the handle's own lc/lp/pb.  The incremental engine keeps every coded event of the current walk, with the
 * probability before its update, in its event chains: an event's price is one table look-up and nothing is re-simulated,
 * so the map is a data-parallel pass over the chains (milliseconds where the walk takes a second).  The chains exist under
 * the handle's triple only: no foreign triple, no caller's slab.  A handle of the full-walk engine (MGL_F_FULLWALK) keeps
 * no chains and is served by mgl_cost_map's walk, with the same integers.
 *   - A parity hook: slab, costs, RNG streams, MGL_ACCEPT_AUTO's block, the focus window, the weights in force and
 *     mgl_sa_stats stay as they were.
 *   - Device memory as for mgl_cost_map, 8 bytes per input byte for the length of the call; MGL_ENOMEM, with the handle left
 *     usable, when they do not fit (MGL_KEY_COSTMAP_NOMEM forces it here too).
 *   - MGL_EDEVICE (device consistency check): the map's total is not the exact cost the control block holds. */
int mgl_cost_map_live(mgl_sa* sa, uint32_t* map_out /* n, nullable */, mgl_cost_report* report /* nullable */);
/* Segment props (no reference counterpart; DESIGN.md section 10, megalania_amd/csrc/mgl_segments.hip): a parse cut into
 * segments, each coded from an LZMA2 state reset under its own lc/lp/pb, the dictionary running through.  All of it is exact
 * integer arithmetic, in the cost units of mgl_cost_slab.
 *   - Segment [lo, hi), lo and hi packet starts of the slab's walk (hi may be n): its coder starts at lo with a fresh model
 *     under its triple, ctx_state 0 and rep distances (0, 0, 0, 0).  Copies may reach below lo; literal contexts use the
 *     absolute position and the real previous byte.
 *   - Re-expression.  The slab's rep packets name slots of the rep stack t of the slab's own walk from byte 0; the segment
 *     has its own stack r.  In walk order: LITERAL and MATCH stay.  SHORT_REP, D = t[0]: stays if r[0] == D, else LITERAL.
 *     LONG_REP i of length L, D = t[i]: stays if r[i] == D, else LONG_REP j for the least j with r[j] == D, else
 *     MATCH(D, L).  Then t advances by the original packet, r and the segment's ctx_state by the re-expressed one.
 *   - cost(lo, hi, T) = the sum of the exact bit costs of the re-expressed packets that start in [lo, hi).  With lo = 0
 *     nothing is re-expressed, and cost(0, n, T) is mgl_props_sweep's entry for T.
 *   - Cuts c_0 = 0 < c_1 < .. < c_m = n, all packet starts, m <= 16 (ncuts = m + 1 <= MGL_SEG_MAX_CUTS).  Span (i, j), i < j,
 *     is [c_i, c_j) and has index s(i, j) = i m - i (i - 1) / 2 + (j - i - 1); there are m (m + 1) / 2 spans.
 *   - The grain rule (mgl_segment_cuts): g' = max(grain, ceil(n / 16)); the candidates k g', k >= 1, below n, each moved to
 *     the first packet start at or above it; candidates that meet there, or at n, count once.  grain 0 = 65536.
 *   - The partition (mgl_segment_partition): best[0] = 0, best[j] = min over i < j of best[i] + min_T cost[s(i, j)][T] +
 *     (i > 0 ? overhead : 0), i ascending and only a strictly smaller value replacing the current one, triple ties to the
 *     first in mgl_props_sweep's order.  MGL_SEG_OVERHEAD is the .xz writer's bound for one further chunk: 6 header bytes
 *     with the props byte and at most 5 flush bytes. */
#define MGL_SEG_MAX_CUTS 17
#define MGL_SEG_MAX_SPANS 136
#define MGL_SEG_OVERHEAD (11ull * 16384ull)
typedef struct { uint64_t lo, hi; mgl_properties props; uint64_t cost; } mgl_segment;
/* The cuts of the grain rule on the walk of `packets` (NULL: the current slab; a caller's slab is validated like
 * mgl_props_sweep's).  cuts_out: cap entries, c_0 .. c_m; *ncuts = m + 1.  cap < *ncuts: MGL_ERANGE with *ncuts set. */
int mgl_segment_cuts(mgl_sa* sa, const mgl_packet* packets, uint64_t grain, uint64_t* cuts_out, size_t cap, size_t* ncuts);
/* Parity hook (the search state is untouched): cost_out[s * 75 + T] = cost(span s, triple T of mgl_props_sweep's order),
 * every span walked by its own wavefront.  *count = 75 m (m + 1) / 2; cap < *count: MGL_ERANGE with *count set.
 * The slab is validated by the walk mgl_props_sweep uses and refused as there.  MGL_EINVAL: cuts not strictly ascending
 * from 0 to n, fewer than 2 or more than MGL_SEG_MAX_CUTS.  MGL_ERANGE: a cut that is no packet start.  The call's buffers
 * are its own and die with it; MGL_ENOMEM leaves the handle usable.  gpu_ms (nullable): device time of the two kernels. */
int mgl_props_sweep_spans(mgl_sa* sa, const mgl_packet* packets, const uint64_t* cuts, size_t ncuts, uint64_t* cost_out, size_t cap,
                          size_t* count, double* gpu_ms);
/* Host arithmetic only, no device involved: the partition above over a table of mgl_props_sweep_spans.  segs_out: room for
 * ncuts - 1 segments; *nseg of them are written, in ascending order, tiling [0, n); *total (nullable) = best[m], the sum of
 * the segments' costs plus (*nseg - 1) overhead.  MGL_EINVAL: a null argument, ncuts outside 2..MGL_SEG_MAX_CUTS. */
int mgl_segment_partition(const uint64_t* cost, size_t ncuts, const uint64_t* cuts, uint64_t overhead, mgl_segment* segs_out, size_t* nseg,
                          uint64_t* total);
/* The three above in a row, with MGL_SEG_OVERHEAD: the cheapest segmentation of `packets` (NULL: the current slab) over the
 * grain's cuts.  segs_out: cap entries (MGL_SEG_MAX_CUTS - 1 always suffice; fewer than needed: MGL_ERANGE with *nseg set).
 * *single_best (nullable) = min_T cost[s(0, m)][T], the best one triple does; *total <= *single_best. */
int mgl_sa_segment_props(mgl_sa* sa, const mgl_packet* packets, uint64_t grain, mgl_segment* segs_out, size_t cap, size_t* nseg,
                         uint64_t* total, uint64_t* single_best, double* gpu_ms);
/* Segment re-parse (no reference counterpart; DESIGN.md section 10, megalania_amd/csrc/mgl_segparse.hip): the adaptive parse
 * of mgl_sa_seed_adaptive run again inside every segment, for the coder that will code it -- from the state reset at the
 * segment's start and under the segment's own triple -- instead of for the one triple and the one running model the slab
 * was made under.  Exact integers in mgl_cost_slab's units throughout.
 *   - Input: a valid slab (`packets`, NULL: the current slab), nseg segments that tile [0, n) at packet starts (what
 *     mgl_emit_xz_segments accepts), and mgl_adaptive_config's settings with their defaults; from_current must be 0.  The
 *     handle's match finder and depth apply as for mgl_sa_seed_adaptive.
 *   - Per segment s = [lo, hi) under its triple T_s, independently of the others.  Chunk m is [lo + m chunk,
 *     min(lo + (m + 1) chunk, hi)): the grid starts at lo.  Pass 0's chunk starts and model snapshots come from the walk of
 *     the segment's own packets from the reset, re-expressed as under "Segment props" above (a chunk start inside a packet
 *     takes the LZMA initial state and the model before that packet, as in mgl_sa_seed_adaptive); that walk's cost is
 *     start_cost = cost(lo, hi, T_s).  Pass p runs mgl_sa_seed_adaptive's shortest path over every chunk with prices under
 *     T_s's layout; an edge ends at its chunk's end at the latest, so no packet crosses hi, while MATCH sources are absolute
 *     positions bounded by the dictionary only: copies reach below lo.  The pass's copies are then walked from the reset,
 *     resolved against the segment coder's own rep stack and costed exactly (pass_cost[p]); that walk leaves pass p + 1's
 *     starts.  objective[p] as in mgl_optimal_stats.  The cheapest pass is taken if it costs strictly less than start_cost,
 *     ties to the lower pass; otherwise the segment keeps its packets and best_pass is UINT32_MAX.
 *   - Join.  A slab's rep packets name the rep stack of the walk from byte 0, so the result is assembled as copies and
 *     resolved once: one walk from 0 takes per segment the input's packets, their distances made absolute through the
 *     input's own stack, or the taken pass's copies, and names each against the output's running stack (distance found in
 *     the stack: SHORT_REP for length 1, else LONG_REP of the least such slot; otherwise LITERAL for length 1, else MATCH).
 *     The output is an ordinary valid slab with the same segments at packet starts; final_cost = cost(lo, hi, T_s) of it.
 *     A packet that uses the distance-1 rep a reset leaves in the coder's stack can come out of the join as a MATCH or a
 *     LITERAL where the whole-file stack lacks that distance; final_cost then differs from pass_cost[best_pass] by that
 *     packet, and by nothing else.
 *   - Guard.  Unless the sum of final_cost is strictly below the sum of start_cost the call hands back the input slab:
 *     *taken = 0, final_cost = start_cost and best_pass = UINT32_MAX for every segment.  The result never costs more. */
typedef struct {
	uint32_t passes, best_pass;             /* best_pass UINT32_MAX: the input's packets were kept */
	uint64_t start_cost, final_cost;
	uint64_t pass_cost[MGL_OPT_MAX_PASSES], objective[MGL_OPT_MAX_PASSES];
} mgl_segment_parse_stats;
/* packets_out: n entries.  segs_out: nseg entries, the same lo, hi and props with cost = final_cost.  stats: nseg entries,
 * nullable; taken and gpu_ms (device time of the call) nullable.  The search state is untouched; the call's buffers (about
 * 40 bytes per input byte) are its own and die with it, MGL_ENOMEM leaves the handle usable.  MGL_EINVAL: a null argument,
 * nseg outside 1..16, segments that do not tile [0, n) in ascending order, a triple outside lc + lp <= 4, pb <= 4, whatever
 * mgl_sa_seed_adaptive refuses of the settings, from_current != 0.  MGL_ERANGE: an invalid slab, or a segment boundary that
 * is no packet start.  mgl_emit_xz_segments(packets_out, segs_out) codes the result. */
int mgl_segment_reparse(mgl_sa* sa, const mgl_packet* packets, const mgl_segment* segs, size_t nseg, const mgl_adaptive_config* cfg,
                        mgl_packet* packets_out, mgl_segment* segs_out, mgl_segment_parse_stats* stats, int* taken, double* gpu_ms);
/* Final model state after costing `packets`: probabilities in the reference's struct order
 * (lzma_state.h:47-53: lit | len | rep_len | dist | ctx_state), ctx_state, rep distances. */
int mgl_final_state(mgl_sa* sa, const mgl_packet* packets, uint16_t* probs_out, size_t probs_cap,
                    uint8_t* ctx_state_out, uint32_t dists_out[4]);
/* Best cfg.top_k next packets at `position` (must be on the walk of `packets`), in the
 * reference's pop order: worst first, best last.  costs[i] = perplexity/length (integer). */
int mgl_top_k(mgl_sa* sa, const mgl_packet* packets, size_t position, mgl_packet* out,
              uint64_t* costs, size_t* count);
/* Match-index query at `pos`: (offset, length) pairs in the reference's callback order. */
int mgl_substrings(mgl_sa* sa, size_t pos, size_t max_len, uint32_t* offsets, uint32_t* lengths,
                   size_t cap, size_t* count);
/* Generate and cost the K neighbours the *next* mgl_sa_run step would look at (or those of
 * an explicit global step number), without deciding.  costs[j] = UINT64_MAX for a failed
 * generate.  diffs (nullable): diff_cap entries per neighbour, ndiffs[j] valid ones. */
int mgl_neighbours(mgl_sa* sa, uint64_t global_step, uint64_t* costs, mgl_diff* diffs,
                   uint32_t* ndiffs, size_t diff_cap);
/* Test / diagnostic hooks (no reference counterpart).  mgl_debug_dump: raw copy of one of the incremental engine's device
 * structures; *bytes receives the size even when the buffer is too small (MGL_ERANGE).  A handle of the full-walk engine
 * answers MGL_DUMP_WINDOWS, MGL_DUMP_SOFT_ENDS and MGL_DUMP_ALLOCATIONS only.  K = cfg.neighbours_per_step, n = the input's
 * bytes.  The structs named are those of megalania_amd/csrc/mgl_words.h.  The numbers are the ABI: they never change. */
enum mgl_dump_selector {
	MGL_DUMP_CHAIN_OFF = 0,      /* u32 per context: chain offsets */
	MGL_DUMP_CHAIN_LEN = 1,      /* u32 per context: chain lengths */
	MGL_DUMP_CHAIN_POS = 2,      /* u32 per pool entry: chain positions */
	MGL_DUMP_CHAIN_EV = 3,       /* u16 per pool entry: chain events */
	MGL_DUMP_ONWALK = 4,         /* u64 words: on-walk bitmap */
	MGL_DUMP_SPECIAL = 5,        /* u64 words: special bitmap */
	MGL_DUMP_SPECIAL_STATE = 6,  /* 8 u32 per position: special-state records */
	MGL_DUMP_CHECKPOINTS = 7,    /* u16: dense checkpoints */
	MGL_DUMP_CHAIN_CAP = 8,      /* u32 per context: chain capacities */
	MGL_DUMP_PHASE_CYCLES = 9,   /* u64, 64 + 2 K: phase-cycle counters (MGL_F_PROFILE; empty without) */
	MGL_DUMP_STEP_COUNTS = 10,   /* StepCounts[2], per-step overflow / repair counters: those of the last finished step or mgl_neighbours
	                              * call, then the live ones, which the end of a step leaves at zero */
	MGL_DUMP_PBUILD_TOTALS = 11, /* PbAcc up to and including `redone` (8 u64): parallel-builder totals */
	MGL_DUMP_BUCKET_OFF = 12,    /* u32, 65537: match index, bucket offsets */
	MGL_DUMP_BUCKET_POS = 13,    /* u32, n - 1: match index, positions */
	MGL_DUMP_APPLY_HDR = 14,     /* ApplyHdr: accept-path counters */
	MGL_DUMP_PICK_RECORDS = 15,  /* 4 u32 per neighbour: pick records */
	MGL_DUMP_CONTROL = 16,       /* bytes: the control block */
	MGL_DUMP_QUAD_POS = 18,      /* u32, n - 1: positions of the 4-byte order */
	MGL_DUMP_QUAD_NEXT = 19,     /* u16, n - 1: its next bytes */
	MGL_DUMP_WINDOWS = 21,       /* 2 u32 per neighbour: the windows (target, end) of the last costed neighbours */
	MGL_DUMP_SOFT_ENDS = 22,     /* u32 per neighbour: their soft ends | dep << 31 */
	MGL_DUMP_COSTS = 23,         /* u64 per neighbour: their costs */
	MGL_DUMP_JOURNAL_LENS = 24,  /* u32 per neighbour: journal lengths */
	MGL_DUMP_WALKED = 25,        /* u32 per neighbour: packets walked */
	MGL_DUMP_PICK_HINTS = 26,    /* K bytes (empty with MGL_NO_ORDER=1 or position targets): what the last targets launch left for the fused
	                              * pick + walk launch: 1 = the neighbour will pick, 0 = it takes a grow/shrink mutation */
	MGL_DUMP_PICK_ORDER = 27,    /* K u32 (empty likewise): every slice's neighbours in the order the launch takes them up (the picking ones
	                              * first, ascending in j inside each class) */
	MGL_DUMP_PICKSTATE = 28,     /* 8 u32 per neighbour: the two-launch form's pickstate records; word 7 = 1 where the pick half took the
	                              * grow/shrink mutation (MGL_NO_FUSE=1 / MGL_F_PROFILE) */
	/* the exact-length orders D = 2..7: selector = base + D - 2 */
	MGL_DUMP_XPOS_BASE = 30,     /* u32, n - 1: positions */
	MGL_DUMP_XRANK_BASE = 40,    /* u32, n - 1: ranks */
	MGL_DUMP_XRUN_BASE = 50,     /* u32, n - 1: run starts */
	MGL_DUMP_XNEXT_BASE = 60,    /* u8, n - 1: next byte */
	MGL_DUMP_OCT_POS = 70,       /* u32, n - 1: the 8-byte order's positions, */
	MGL_DUMP_OCT_RANK = 71,      /* u32: ranks, */
	MGL_DUMP_OCT_RUN = 72,       /* u32: run starts */
	MGL_DUMP_OCT_NEXT8 = 73,     /* u64: and next eight bytes */
	MGL_DUMP_HEX_POS = 74,       /* the same four of the 16-byte order */
	MGL_DUMP_HEX_RANK = 75,
	MGL_DUMP_HEX_RUN = 76,
	MGL_DUMP_HEX_NEXT8 = 77,
	MGL_DUMP_BATCH_COUNTS = 80,  /* three u64 host counters: bulk steps whose moves were patched into the base structures at once (batch
	                              * accept), those that began so and fell back to the rebuild behind their commit (status 1), and those that
	                              * left the step to the rebuild before anything was touched because the clusters or a walk gave up (status 2
	                              * with a failure seen) */
	MGL_DUMP_BATCH_HDR = 81,     /* BatchHdr: the batch accept's header */
	MGL_DUMP_BATCH_ACC = 82,     /* BatchAcc: and totals */
	MGL_DUMP_CHAIN_INDEX = 83,   /* u32: the chain index, a row per context */
	MGL_DUMP_GIVEUP_SITES = 84,  /* one u32: the give-up sites of the in-place accepts seen since the last dump (enum mgl_giveup_site;
	                              * cleared by the dump and by MGL_KEY_LIMIT) */
	MGL_DUMP_POOL_TOP = 85,      /* one u32: the chain pool's top */
	MGL_DUMP_INDEX_GEOMETRY = 86, /* three u32: the chain index's block shift (the size rule's or MGL_SB_SHIFT's; the parallel builder's block is
	                              * the same), its blocks and the words of an index row */
	MGL_DUMP_ALLOCATIONS = 87    /* two u64 host counters, answered by every handle: the device allocations the handle holds right now and
	                              * their total bytes as requested */
};
enum mgl_debug_key {
	MGL_KEY_DIAG_STOP = 0,     /* stop the neighbour kernels after a phase (tools/phase_cost.py); 50 = stage timing in the accept path */
	MGL_KEY_PBUILD_FIX = 1,    /* make the parallel builder redo every chain segment serially (exercises its fallback) */
	MGL_KEY_LIST_CAP = 2,      /* shrink the first-pass change lists (a multiple of 8, at most the allocated size) so that neighbours
	                            * overflow into the second pass (exercises it) */
	MGL_KEY_ROLLBACKS = 3,     /* treat the next so many bulk steps that took moves as failed validations (exercises the rollback) */
	MGL_KEY_COUNT_TRAFFIC = 4, /* 1 / 0: the re-simulation kernel adds up the bytes it reads (mgl_sa_stats.sim_bytes_counted; a few percent slower) */
	MGL_KEY_BATCH_FAIL = 5,    /* n: the next n batch accepts (bulk steps that patch few moves into the base structures) give up after they
	                            * have written their journals and bitmaps (exercises the fallback to the rebuild from there): at the top of
	                            * the chain kernel, before any chain is touched.  Second form, value >> 32 = m > 0: the give-up comes once
	                            * the m-th touched context has rewritten its chain's descriptors, taken its pool space and queued its copy
	                            * jobs -- behind a partial rewrite by other workgroups (a low word of 0 then counts as 1).  Every batch
	                            * accept the hook is applied to counts against the low word, also one that goes through because fewer
	                            * than m contexts got that far (nothing gives up then); steps that take nothing or too many moves do not count */
	MGL_KEY_LIMIT = 6,         /* id | value << 8: limit `id` (enum mgl_accept_limit) of the in-place accepts := value, so that a give-up's
	                            * real comparison fires on an ordinary input; a value above the compiled / allocated one is refused
	                            * (MGL_EINVAL); id 0 with value 0 restores every default */
	MGL_KEY_BIG_WAVES = 7,     /* 1, 2 or the compiled MGL_BIG_WAVES (anything else: MGL_EINVAL): the wavefronts of a second-pass workgroup,
	                            * which share a neighbour's re-simulations; with 1 or 2 a neighbour's contexts take several trips */
	MGL_KEY_CROSS_NOMEM = 8,   /* n: the next n crossovers (mgl_crossover, mgl_sa_cross_best and the crossing exchanges) find no room for
	                            * their buffers (MGL_ENOMEM; exercises mgl_sa_exchange_cross_all's fall-back) */
	MGL_KEY_PICK_HINTS = 9,    /* pattern: overwrite the class hints (MGL_DUMP_PICK_HINTS) with 0: all 0, 1: all 1, 2: alternating, anything
	                            * else: random bytes from `pattern`, and make the order (MGL_DUMP_PICK_ORDER) from them again -- the test
	                            * of k_pick_order */
	MGL_KEY_COSTMAP_NOMEM = 10, /* n: the next n calls of mgl_cost_map / mgl_cost_map_live find no room for their buffers (MGL_ENOMEM; the handle stays usable) */
	MGL_KEY_PROBE_FORM = 11    /* which form of the top-K search mgl_top_k probes: 0 (the default) the pick half's, batched set-up and four entries
	                            * a lane; 1 the in-place form of the repair picks, the one-kernel form and the full-walk engine (anything else: MGL_EINVAL) */
};
/* What the in-place accepts compare against before they give up (MGL_KEY_LIMIT).  1-6: the single accept (mgl_kernels3.hip);
 * 7-10: both; 11-18: the batch accept (mgl_kernels5.hip). */
enum mgl_accept_limit {
	MGL_LIM_APPLY_EVENTS = 1,   /* inserted / removed events of the accepted neighbour */
	MGL_LIM_APPLY_GUARD = 2,    /* iterations of its walk */
	MGL_LIM_APPLY_SUB = 3,      /* events of one context */
	MGL_LIM_APPLY_SPAN = 4,     /* rewritten chain entries of one context */
	MGL_LIM_APPLY_PIECES = 5,   /* pieces / checkpoint segments of one context */
	MGL_LIM_APPLY_SHIFT = 6,    /* entries a chain's tail may shift by in place */
	MGL_LIM_POOL = 7,           /* chain pool entries (a chain that outgrows its slot finds the pool exhausted) */
	MGL_LIM_JOBS = 8,           /* copy jobs per list */
	MGL_LIM_SPAN_AREA = 9,      /* span area entries */
	MGL_LIM_SCRATCH = 10,       /* save area entries */
	MGL_LIM_BATCH_JOURNAL = 11, /* journal entries of one cluster */
	MGL_LIM_BATCH_EVENTS = 12,  /* staged events of one cluster */
	MGL_LIM_BATCH_OPS = 13,     /* bitmap / state-record ops of one cluster */
	MGL_LIM_BATCH_GUARD = 14,   /* iterations of a cluster's walk */
	MGL_LIM_BATCH_SUB = 15,     /* events of one kind per context */
	MGL_LIM_BATCH_SHIFT = 16,   /* entries a stretch may shift by in place */
	MGL_LIM_BATCH_RUNS = 17,    /* runs on the checkpoint list */
	MGL_LIM_SOFT_REACH = 18,    /* 1 / 0: clusters are split at the members' soft window ends instead of their hard ends (a wrong rule on
	                             * purpose: the boundary guard of the cluster walks must then send the step to the rebuild) */
	MGL_LIM_COUNT = 19
};
/* Where an in-place accept gave up: the bits of MGL_DUMP_GIVEUP_SITES */
enum mgl_giveup_site {
	MGL_GU_APPLY_EVENTS = (1u << 0),    /* k_apply_walk: event lists */
	MGL_GU_APPLY_GUARD = (1u << 1),     /* k_apply_walk: iteration guard */
	MGL_GU_APPLY_SUB = (1u << 2),       /* k_apply_chains: events of one context */
	MGL_GU_APPLY_SPAN = (1u << 3),      /* k_apply_chains: rewritten entries of one context */
	MGL_GU_APPLY_PIECES = (1u << 4),    /* k_apply_chains: pieces / checkpoint segments */
	MGL_GU_APPLY_POOL = (1u << 5),      /* k_apply_chains: chain pool exhausted */
	MGL_GU_APPLY_JOBS = (1u << 6),      /* k_apply_chains: job lists */
	MGL_GU_APPLY_SPAN_AREA = (1u << 7),
	MGL_GU_APPLY_SCRATCH = (1u << 8),
	MGL_GU_APPLY_SHIFT = (1u << 9),
	MGL_GU_CL_JOURNAL = (1u << 10),     /* k_batch_clusters: a cluster's merged journal */
	MGL_GU_CL_ORDER = (1u << 11),       /* k_batch_clusters: merged journal not strictly ascending */
	MGL_GU_WALK_OPS = (1u << 12),       /* k_batch_walk */
	MGL_GU_WALK_EVENTS = (1u << 13),
	MGL_GU_WALK_GUARD = (1u << 14),
	MGL_GU_WALK_INVALID = (1u << 15),   /* a packet or rep packet of the merged walk that does not code the input */
	MGL_GU_WALK_OVERRUN = (1u << 16),   /* the merged walk had not re-joined the base at the next cluster's first entry */
	MGL_GU_CH_SUB = (1u << 17),         /* k_batch_chains */
	MGL_GU_CH_SPAN_AREA = (1u << 18),   /* step 3: the place every run gets to begin with */
	MGL_GU_CH_SHIFT = (1u << 19),
	MGL_GU_CH_POOL = (1u << 20),
	MGL_GU_CH_JOBS = (1u << 21),
	MGL_GU_CH_SCRATCH = (1u << 22),
	MGL_GU_CH_RUNS = (1u << 23),
	MGL_GU_FORCED_EARLY = (1u << 24),   /* MGL_KEY_BATCH_FAIL, low word */
	MGL_GU_FORCED_LATE = (1u << 25),    /* MGL_KEY_BATCH_FAIL, high word */
	MGL_GU_CH_SPAN_RERUN = (1u << 26)   /* k_batch_chains step 5: the span area, for a run that did not fit its first place (the chain has
	                                     * its pool space by then) */
};
int mgl_debug_dump(mgl_sa* sa, uint32_t what, void* out, size_t cap_bytes, size_t* bytes);
int mgl_debug_set(mgl_sa* sa, uint32_t key, uint64_t value);
/* draw n of neighbour j at global step `step` (31-bit, like rand()); j = 0xFFFFFFFF is the
 * step's own stream (accept decision). */
uint32_t mgl_rng_draw_at(uint64_t seed, uint64_t step, uint32_t j, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif /* MEGALANIA_HIP_H */
