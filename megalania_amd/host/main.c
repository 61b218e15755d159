/*
 * megalania-hip -- command-line driver in C, the GPU-path counterpart of the reference's
 * main.c:28-128: `megalania-hip [options] <file>` writes an LZMA-alone stream (or, with
 * --format xz, an .xz stream) to stdout and progress to stderr.  Host code only calls the C ABI (include/megalania_hip.h) and emits
 * the best slab through EncoderInterface / OutputInterface like main.c:110-119.
 *
 * Schedule (main.c:64-77): `phases` x `epochs` epochs; phase 0 epochs start from an
 * all-literal slab, later phases from the best slab so far.  The reference runs N (= file
 * size) single-neighbour iterations per epoch; here an epoch is ceil(N / K) steps of K
 * neighbours, i.e. the same number of neighbour evaluations.  Defaults are the reference's
 * (3 x 200) and, like the reference, take a very long time on anything but tiny inputs:
 * use --epochs / --steps to bound the run.
 */
#include <fcntl.h>
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "mgl_host.h"

static void usage(const char* argv0)
{
	fprintf(stderr,
	        "usage: %s [--neighbours K] [--epochs E] [--phases P] [--steps S] [--seed N]\n"
	        "          [--lc N --lp N --pb N | --props auto [--props-rounds R] [--props-table] [--props-joint T]] [--device D] [--max-scan M]\n"
	        "          [--format lzma|xz] [--filter none|x86|auto] [--dict-size BYTES]\n"
	        "          [-o out.lzma] [--save-slab file] [--load-slab file] [--greedy-seed C] [--optimal-seed P | --adaptive-seed P]\n"
	        "          [--match-finder nearest|frontier [--mf-depth N]] [--parse-sweep [--parse-sweep-table]] [--temperature B]\n"
	        "          [--seed-stream file.lzma|file.xz [--clip-window]]\n"
	        "          [--accept auto|single|bulk] [--chains N --rank R --comm-file PATH [--comm-nonce X] [--transport rccl|shm]\n"
	        "          [--exchange best|cross|cross-all [--cross-grain N]]] [--focus LO:HI|rank]\n"
	        "          [--cost-map FILE] [--cost-report] [--cost-bucket B] filename\n"
	        "  -o           write the stream to a file instead of stdout\n"
	        "  --save-slab  after every epoch, write the best packet slab (resumable checkpoint)\n"
	        "  --load-slab  start from a slab written by --save-slab (same input, same lc/lp/pb, same filter)\n"
	        "  --format F   the container written: lzma (LZMA-alone, default) or xz (one stream, one block, CRC32 check)\n"
	        "  --filter F   with --format xz: none (default), x86 (the input goes through the .xz x86 branch/call/jump filter before\n"
	        "               anything else sees it, and the block declares it) or auto: the parse of the seed option (without one, an\n"
	        "               optimal parse made for this only) is made over the plain and over the filtered bytes and the cheaper\n"
	        "               exact cost wins, a tie goes to none.  auto: not with --seed-stream, --load-slab or --chains above 1\n"
	        "  --dict-size BYTES  the dictionary: no copy reaches farther back, and the stream declares it (.xz: the next size\n"
	        "               the format can name).  At least 4096; 0 or absent = 4 MiB\n"
	        "  --greedy-seed C  epochs that the reference starts from the all-literal slab start from a greedy\n"
	        "               parse instead (longest of the C nearest candidates per position; e.g. 256)\n"
	        "  --optimal-seed P  epochs that the reference starts from the all-literal slab start from the best of P\n"
	        "               price-driven optimal parses made on the device (e.g. 3); not with --greedy-seed,\n"
	        "               --seed-stream or --load-slab\n"
	        "  --adaptive-seed P  as --optimal-seed, but the parses are priced from the live probability model, refreshed as\n"
	        "               each segment of a chunk is committed (e.g. 3); not with --optimal-seed, --greedy-seed,\n"
	        "               --seed-stream or --load-slab\n"
	        "  --match-finder F  where --optimal-seed / --adaptive-seed / --props auto take a node's match sources from: the\n"
        "               nearest candidates of the two- and four-byte orders (nearest, default) or the nearest source of every\n"
        "               achievable length (frontier); --mf-depth N bounds the run entries the frontier examines per position\n"
        "               (default 64, at most 4096)\n"
	        "  --parse-sweep    with --adaptive-seed P: the seed is made under 16 settings at once (both match finders, commit\n"
	        "               distances 64, 32, 128, 256, look-ahead 128 and 273) and the cheapest parse is kept; --mf-depth N\n"
	        "               applies to the frontier's variants; not with --match-finder.  --parse-sweep-table prints every\n"
	        "               variant's per-pass sizes\n"
        "  --seed-stream F  start from the parse inside an existing .lzma / .xz stream of this input (e.g. xz -9e's):\n"
	        "               it becomes the best slab and every epoch starts from it; lc/lp/pb default to the stream's;\n"
	        "               with --format xz, an .xz stream that declares the x86 filter selects --filter x86\n"
	        "  --clip-window    with --seed-stream: copies from beyond the dictionary window become literals instead\n"
	        "               of an error\n"
	        "  --props auto     choose lc/lp/pb before the search: the parse of the seed option (without one, an optimal parse made\n"
	        "               for this only) is costed under all 75 supported triples at once and the search runs under the\n"
	        "               cheapest; a seed that depends on the triple is made again under it, up to R sweeps (default 3).\n"
	        "               Not with --lc/--lp/--pb or --chains above 1.  --props-table prints the last sweep's 75 costs\n"
	        "  --props-joint T  with --props auto --adaptive-seed P --parse-sweep: instead of the rounds, the parse sweep is made at\n"
	        "               0/0/0, its winner is costed under all 75 triples, and one more batch makes the 16 settings under each of\n"
	        "               the T cheapest other triples (1..4) on the same handle; the cheapest (triple, parse) of both stages wins.\n"
	        "               At most two handles are created.  Not with --seed-stream, --load-slab, --greedy-seed, --lc/--lp/--pb or\n"
	        "               --chains above 1\n"
	        "  --temperature B  Metropolis accept rule instead of the reference's: B = e-folding slack in output\n"
	        "               bytes at the start of an epoch, cooled linearly to 0 (e.g. 2; 0 = reference rule)\n"
	        "  --chains N --rank R --comm-file PATH  one of N independent chains, one process per GPU (device = R unless\n"
	        "               --device says otherwise): after every epoch the chains exchange their best slab over RCCL\n"
	        "               (8-byte all-reduce + one broadcast); rank 0 creates PATH (the communicator id) and writes the\n"
	        "               stream, the others wait for a PATH that carries the same --comm-nonce (give every run its own,\n"
	        "               e.g. the launcher's pid: a file left by an earlier run is then never mistaken for this one's);\n"
	        "               --transport shm stages the exchange through PATH itself (host shared memory) instead of RCCL:\n"
	        "               for chains that share one GPU.  --save-slab: chain R > 0 writes to <file>.rankR\n"
	        "  --exchange best|cross|cross-all  what the chains do with the cheapest best slab after an epoch: every other chain adopts it\n"
	        "               (best, default), or recombines it with its own best slab region by region between the positions where\n"
	        "               the two walks agree and keeps the child if it is cheaper than both (cross; mgl_sa_exchange_cross);\n"
	        "               one plain exchange follows the last epoch, so that rank 0 writes the overall best.  --cross-grain N:\n"
	        "               about one cut per N input bytes (default 64; 1 = every joint); only with --exchange cross or cross-all.\n"
	        "               cross-all (mgl_sa_exchange_cross_all): the chains publish cost and hash of their best slabs, the distinct\n"
	        "               ones (the 8 cheapest at most) travel to every chain and all chains make the same child of them; it\n"
	        "               becomes every chain's best slab if it is cheaper than the cheapest parent, which the dearer chains adopt\n"
	        "               otherwise.  Every chain then holds a best slab of the same cost: no plain exchange follows\n"
	        "  --focus LO:HI  the search takes its targets among the packets that start in bytes [LO, HI) of the input (LO < HI, HI at\n"
	        "               most the file's size) and writes nothing below LO: refines one stretch, e.g. behind --seed-stream from a\n"
	        "               stream whose input changed only there.  --focus rank (needs --chains N, N >= 2): before every epoch chain\n"
	        "               R takes slice R of N of the input (mgl_focus_slice), shifted by half a slice every other epoch, so that\n"
	        "               chains that leave an exchange with a common slab work on different stretches of it\n"
	        "  --cost-map FILE  where the emitted parse spends its bits (mgl_cost_map, under the run's final lc/lp/pb): FILE gets one\n"
	        "               little-endian u32 per input byte, the byte's share of its packet's exact cost (2048 per bit); the values\n"
	        "               sum to the parse's cost.  With --filter x86 the positions are those of the filtered bytes.  The emitted\n"
	        "               stream is the same with and without this option and the next two; each may be given alone\n"
	        "  --cost-report    print to stderr one line per coder and per packet type of the emitted parse:\n"
	        "               `cost-class: NAME bits N cost X B share P %% exact C` (kind, literal, length, rep_length, distance, direct)\n"
	        "               `cost-type: NAME packets N bytes M cost X B share P %% exact C` (literal, match, short_rep, long_rep)\n"
	        "               behind `cost-report: total X B exact C packets N lc=.. lp=.. pb=.. T ms`; X = C / 16384\n"
	        "  --cost-bucket B  print one line per B input bytes: `cost-bucket: offset O bytes N cost X B bpb R exact C`\n"
	        "  --accept     what a step of K neighbours takes: the best acceptable one (single), every one that is\n"
	        "               the best of its own window (bulk), or whichever pays (auto, default)\n", argv0);
}

/* the seed made on the device: the best of `passes` optimal parses, under static prices or (adaptive) the live model's */
typedef struct { uint32_t passes; bool adaptive; int finder; uint32_t mf_depth; bool sweep, sweep_table; } seed_spec;

/* --parse-sweep's grid (mirrored by binding.DEFAULT_SWEEP): index 0 is the library's default, which therefore holds a tie */
#define SWEEP_GRID 16
static const mgl_parse_variant sweep_grid[SWEEP_GRID] = {
	{ MGL_MF_NEAREST, 16, 64, 128 },   { MGL_MF_NEAREST, 16, 64, 273 },   { MGL_MF_NEAREST, 16, 32, 128 },   { MGL_MF_NEAREST, 16, 32, 273 },
	{ MGL_MF_NEAREST, 16, 128, 128 },  { MGL_MF_NEAREST, 16, 128, 273 },  { MGL_MF_NEAREST, 16, 256, 128 },  { MGL_MF_NEAREST, 16, 256, 273 },
	{ MGL_MF_FRONTIER, 16, 64, 128 },  { MGL_MF_FRONTIER, 16, 64, 273 },  { MGL_MF_FRONTIER, 16, 32, 128 },  { MGL_MF_FRONTIER, 16, 32, 273 },
	{ MGL_MF_FRONTIER, 16, 128, 128 }, { MGL_MF_FRONTIER, 16, 128, 273 }, { MGL_MF_FRONTIER, 16, 256, 128 }, { MGL_MF_FRONTIER, 16, 256, 273 },
};

/* the adaptive seed under every variant of the grid at once; *os = the winner's stats */
static int make_sweep_seed(mgl_sa* sa, seed_spec seed, mgl_optimal_stats* os)
{
	mgl_optimal_stats res[SWEEP_GRID];
	const mgl_parse_sweep_config sc = { seed.passes, 0, seed.mf_depth, 0 };
	uint32_t best = 0;
	double ms = 0;
	int rc = mgl_sa_seed_sweep(sa, &sc, sweep_grid, SWEEP_GRID, res, &best, &ms);
	if (rc != MGL_OK) return rc;
	if (best >= SWEEP_GRID) return MGL_EDEVICE; /* without from_current some variant always wins */
	if (seed.sweep_table)
		for (uint32_t v = 0; v < SWEEP_GRID; v++) {
			fprintf(stderr, "parse-sweep-table: %s cand %u segment %u ahead %u:", sweep_grid[v].finder == MGL_MF_FRONTIER ? "frontier" : "nearest",
			        sweep_grid[v].cand, sweep_grid[v].segment, sweep_grid[v].ahead);
			for (uint32_t p = 0; p < res[v].passes; p++) fprintf(stderr, " %.1f", 18 + res[v].cost[p] / 16384.0);
			fprintf(stderr, " B%s\n", v == best ? " *" : "");
		}
	fprintf(stderr, "parse sweep: variant %u (%s, cand %u, segment %u, ahead %u), pass %u, %.1f B; %u variants in %.1f ms\n", best,
	        sweep_grid[best].finder == MGL_MF_FRONTIER ? "frontier" : "nearest", sweep_grid[best].cand, sweep_grid[best].segment,
	        sweep_grid[best].ahead, res[best].best_pass, 18 + res[best].cost[res[best].best_pass] / 16384.0, SWEEP_GRID, ms);
	*os = res[best];
	return MGL_OK;
}

static int make_seed(mgl_sa* sa, seed_spec seed, mgl_optimal_stats* os)
{
	if (seed.sweep) return make_sweep_seed(sa, seed, os);
	/* set on every handle a seed is made on: --props auto makes fresh ones */
	int rc = mgl_sa_set_match_finder(sa, seed.finder, seed.mf_depth);
	if (rc != MGL_OK) return rc;
	if (seed.adaptive) {
		mgl_adaptive_config ac = { seed.passes, 0, 0, 0, 0, 0 };
		return mgl_sa_seed_adaptive(sa, &ac, os);
	}
	mgl_optimal_config oc = { seed.passes, 0, 0 };
	return mgl_sa_seed_optimal(sa, &oc, os);
}

static bool same_props(mgl_properties a, mgl_properties b) { return a.lc == b.lc && a.lp == b.lp && a.pb == b.pb; }

/* slab file: "MGLSLAB1", u64 size, u64 perplexity, size x 12-byte packets (lzma_packet.h:13-17) */
static bool read_slab_file(const char* path, size_t file_size, mgl_packet* packets, uint64_t* perplexity)
{
	FILE* f = fopen(path, "rb");
	char magic[8];
	uint64_t hdr[2] = { 0, 0 };
	const bool ok = f && fread(magic, 8, 1, f) == 1 && memcmp(magic, "MGLSLAB1", 8) == 0 && fread(hdr, 8, 2, f) == 2 &&
	                hdr[0] == file_size && fread(packets, sizeof(mgl_packet), file_size, f) == file_size;
	if (f) fclose(f);
	*perplexity = hdr[1];
	return ok;
}

/* --props auto.  `sa` is a handle at *props that nothing has been done to yet.  Each round costs
 * one parse under all 75 triples (mgl_props_sweep) and moves to a fresh handle at the cheapest, until that is the
 * handle's own or `rounds` sweeps are done.  parse_fixed: `parse` holds a parse that does not depend on the triple (a
 * stream's, a loaded slab's, the greedy one); otherwise every round makes the seed `seed` under the handle's triple
 * into it.  Of all (triple, parse) pairs seen the cheapest wins: *props becomes its triple, `kept` its parse (only
 * when the parse is not fixed), and the handle returned is an untouched one at that triple.  NULL after an error
 * (already reported). */
static mgl_sa* choose_props(mgl_sa* sa, const uint8_t* data, size_t n, const mgl_sa_config* cfg, mgl_properties* props,
                            mgl_packet* parse, bool parse_fixed, seed_spec seed, unsigned rounds, bool print_table,
                            mgl_packet* kept)
{
	mgl_props_cost tab[MGL_PROPS_TRIPLES];
	uint64_t best_cost = UINT64_MAX, best_at0 = 0;
	mgl_properties best = *props;
	unsigned done = 0;
	bool touched = false;
	for (;;) {
		if (!parse_fixed) {
			mgl_optimal_stats os;
			uint64_t cost = 0;
			if (make_seed(sa, seed, &os) != MGL_OK || mgl_sa_current(sa, parse, &cost) != MGL_OK) goto fail;
			touched = true;
		}
		size_t count = 0;
		if (mgl_props_sweep(sa, parse, tab, MGL_PROPS_TRIPLES, &count, NULL) != MGL_OK) goto fail;
		done++;
		size_t arg = 0; /* the cheapest, ties to the first in canonical order */
		for (size_t t = 1; t < MGL_PROPS_TRIPLES; t++)
			if (tab[t].cost < tab[arg].cost) arg = t;
		if (tab[arg].cost < best_cost) {
			best_cost = tab[arg].cost; best = tab[arg].props; best_at0 = tab[0].cost;
			if (!parse_fixed) memcpy(kept, parse, sizeof(mgl_packet) * n);
		}
		if (same_props(tab[arg].props, *props) || done >= rounds) break;
		mgl_sa_destroy(sa);
		*props = tab[arg].props;
		touched = false;
		if ((sa = mgl_sa_create(data, n, *props, cfg)) == NULL) goto fail;
	}
	if (touched || !same_props(best, *props)) {
		mgl_sa_destroy(sa);
		*props = best;
		if ((sa = mgl_sa_create(data, n, *props, cfg)) == NULL) goto fail;
	}
	fprintf(stderr, "props: lc=%u lp=%u pb=%u, sweep %llu B, at 0/0/0 %llu B, %u rounds\n", best.lc, best.lp, best.pb,
	        (unsigned long long)((best_cost + 16383) / 16384), (unsigned long long)((best_at0 + 16383) / 16384), done);
	if (print_table)
		for (size_t t = 0; t < MGL_PROPS_TRIPLES; t++)
			fprintf(stderr, "props-table: lc=%u lp=%u pb=%u cost %llu (%llu B)\n", tab[t].props.lc, tab[t].props.lp, tab[t].props.pb,
			        (unsigned long long)tab[t].cost, (unsigned long long)((tab[t].cost + 16383) / 16384));
	return sa;
fail:
	fprintf(stderr, "Error: %s\n", mgl_last_error());
	return NULL;
}

/* --props-joint T.  `sa` is an untouched handle at *props = 0/0/0.  Stage A: the grid at 0/0/0
 * (parse W_A, cost c_A).  W_A is costed under all 75 triples; t* is the cheapest, the candidates C the T cheapest other than
 * 0/0/0.  Stage B: one batch of 16 x T variants, grid entry g under C[k] at 16 k + g (parse W_B at cost c_B under C[k_B]).
 * The cheapest of (0/0/0, W_A, c_A), (t*, W_A, table[t*]), (C[k_B], W_B, c_B) wins, ties in this order; `kept` receives
 * its parse and *props its triple.  Returns a handle at that triple on which the parse costs what the pair said. */
#define JOINT_MAX 4
static void print_sweep_rows(mgl_properties pr, const mgl_optimal_stats* res, uint32_t star)
{
	for (uint32_t g = 0; g < SWEEP_GRID; g++) {
		fprintf(stderr, "parse-sweep-table: lc=%u lp=%u pb=%u %s cand %u segment %u ahead %u:", pr.lc, pr.lp, pr.pb,
		        sweep_grid[g].finder == MGL_MF_FRONTIER ? "frontier" : "nearest", sweep_grid[g].cand, sweep_grid[g].segment, sweep_grid[g].ahead);
		for (uint32_t p = 0; p < res[g].passes; p++) fprintf(stderr, " %.1f", 18 + res[g].cost[p] / 16384.0);
		fprintf(stderr, " B%s\n", g == star ? " *" : "");
	}
}
static mgl_sa* choose_props_joint(mgl_sa* sa, const uint8_t* data, size_t n, const mgl_sa_config* cfg, mgl_properties* props, seed_spec seed,
                                  unsigned T, bool print_table, mgl_packet* kept)
{
	static mgl_optimal_stats res_a[SWEEP_GRID], res_b[SWEEP_GRID * JOINT_MAX];
	mgl_parse_variant var_b[SWEEP_GRID * JOINT_MAX];
	mgl_properties pr_a[SWEEP_GRID], pr_b[SWEEP_GRID * JOINT_MAX], cand[JOINT_MAX];
	mgl_props_cost tab[MGL_PROPS_TRIPLES];
	const mgl_parse_sweep_config sc = { seed.passes, 0, seed.mf_depth, 0 };
	const mgl_properties s0 = *props;
	mgl_packet* w_b = (mgl_packet*)malloc(sizeof(mgl_packet) * n);
	uint32_t best_a = 0, best_b = 0;
	double ms_a = 0, ms_b = 0;
	size_t count = 0;
	if (!w_b) { fprintf(stderr, "Error: out of memory\n"); return NULL; }
	for (uint32_t g = 0; g < SWEEP_GRID; g++) pr_a[g] = s0;
	if (mgl_parse_sweep_props(sa, &sc, sweep_grid, pr_a, SWEEP_GRID, res_a, &best_a, kept, &ms_a) != MGL_OK) goto fail;
	if (best_a >= SWEEP_GRID) { mgl_sa_destroy(sa); free(w_b); fprintf(stderr, "Error: the parse sweep named no variant\n"); return NULL; }
	const uint64_t c_a = res_a[best_a].cost[res_a[best_a].best_pass];
	if (mgl_props_sweep(sa, kept, tab, MGL_PROPS_TRIPLES, &count, NULL) != MGL_OK) goto fail;
	size_t t_star = 0; /* the cheapest, ties to the first in canonical order */
	for (size_t t = 1; t < MGL_PROPS_TRIPLES; t++)
		if (tab[t].cost < tab[t_star].cost) t_star = t;
	/* the T cheapest triples other than the start, by cost, ties in canonical order */
	bool taken[MGL_PROPS_TRIPLES] = { false };
	for (unsigned k = 0; k < T; k++) {
		size_t arg = MGL_PROPS_TRIPLES;
		for (size_t t = 0; t < MGL_PROPS_TRIPLES; t++)
			if (!taken[t] && !same_props(tab[t].props, s0) && (arg == MGL_PROPS_TRIPLES || tab[t].cost < tab[arg].cost)) arg = t;
		taken[arg] = true;
		cand[k] = tab[arg].props;
		for (uint32_t g = 0; g < SWEEP_GRID; g++) { var_b[SWEEP_GRID * k + g] = sweep_grid[g]; pr_b[SWEEP_GRID * k + g] = cand[k]; }
	}
	if (mgl_parse_sweep_props(sa, &sc, var_b, pr_b, (size_t)SWEEP_GRID * T, res_b, &best_b, w_b, &ms_b) != MGL_OK) goto fail;
	if (best_b >= SWEEP_GRID * T) { mgl_sa_destroy(sa); free(w_b); fprintf(stderr, "Error: the parse sweep named no variant\n"); return NULL; }
	const uint64_t c_b = res_b[best_b].cost[res_b[best_b].best_pass];
	/* the decision */
	const char* stage = "A";
	mgl_properties win = s0;
	uint64_t cost = c_a;
	uint32_t variant = best_a, pass = res_a[best_a].best_pass;
	if (tab[t_star].cost < cost) { stage = "A-recosted"; win = tab[t_star].props; cost = tab[t_star].cost; }
	if (c_b < cost) {
		stage = "B"; win = pr_b[best_b]; cost = c_b; variant = best_b % SWEEP_GRID; pass = res_b[best_b].best_pass;
		memcpy(kept, w_b, sizeof(mgl_packet) * n);
	}
	free(w_b);
	w_b = NULL;
	if (!same_props(win, s0)) {
		mgl_sa_destroy(sa);
		*props = win;
		if ((sa = mgl_sa_create(data, n, *props, cfg)) == NULL) goto fail;
	}
	uint64_t check = 0;
	if (mgl_sa_set_slab(sa, kept) != MGL_OK || mgl_sa_current(sa, NULL, &check) != MGL_OK) goto fail;
	if (check != cost) {
		fprintf(stderr, "Error: the joint choice's parse costs %llu on a handle at its triple, not %llu\n", (unsigned long long)check, (unsigned long long)cost);
		mgl_sa_destroy(sa);
		return NULL;
	}
	fprintf(stderr, "props: lc=%u lp=%u pb=%u, sweep %llu B, at 0/0/0 %llu B, joint with %u candidates in %.1f + %.1f ms\n", win.lc, win.lp, win.pb,
	        (unsigned long long)((cost + 16383) / 16384), (unsigned long long)((c_a + 16383) / 16384), T, ms_a, ms_b);
	fprintf(stderr, "props joint: lc=%u lp=%u pb=%u stage %s variant %u pass %u cost %llu; stage A cost %llu; candidates", win.lc, win.lp, win.pb, stage,
	        variant, pass, (unsigned long long)cost, (unsigned long long)c_a);
	for (unsigned k = 0; k < T; k++) fprintf(stderr, " %u/%u/%u", cand[k].lc, cand[k].lp, cand[k].pb);
	fprintf(stderr, "\n");
	if (seed.sweep_table) {
		print_sweep_rows(s0, res_a, !strcmp(stage, "B") ? SWEEP_GRID : best_a);
		for (unsigned k = 0; k < T; k++) print_sweep_rows(cand[k], res_b + SWEEP_GRID * k, !strcmp(stage, "B") && best_b / SWEEP_GRID == k ? variant : SWEEP_GRID);
	}
	if (print_table)
		for (size_t t = 0; t < MGL_PROPS_TRIPLES; t++)
			fprintf(stderr, "props-table: lc=%u lp=%u pb=%u cost %llu (%llu B)\n", tab[t].props.lc, tab[t].props.lp, tab[t].props.pb,
			        (unsigned long long)tab[t].cost, (unsigned long long)((tab[t].cost + 16383) / 16384));
	return sa;
fail:
	free(w_b);
	fprintf(stderr, "Error: %s\n", mgl_last_error());
	return NULL;
}

/* --filter auto: the seed whose exact cost decides.  Greedy parse, the optimal / adaptive seed of the run, or an optimal
 * parse at the library's defaults where the run has no seed option. */
static int make_filter_seed(mgl_sa* sa, uint32_t greedy, seed_spec seed, mgl_packet* parse, uint64_t* cost)
{
	mgl_optimal_stats os;
	int rc;
	if (greedy) rc = mgl_sa_seed_greedy(sa, greedy);
	else if (seed.passes) rc = make_seed(sa, seed, &os);
	else {
		mgl_optimal_config oc = { 0, 0, 0 };
		rc = mgl_sa_seed_optimal(sa, &oc, &os);
	}
	return rc != MGL_OK ? rc : mgl_sa_current(sa, parse, cost);
}

/* --cost-map / --cost-report / --cost-bucket: the slab the run emits, handed to mgl_cost_map explicitly under the run's
 * final triple.  The line formats are fixed (README.md, "Cost map"); costs in bytes are cost / 16384, `exact` is the
 * integer itself. */
static bool report_costs(mgl_sa* sa, const mgl_packet* slab, size_t n, mgl_properties props, const char* map_path, bool tables,
                         unsigned long long bucket)
{
	static const char* const class_name[MGL_CC_CLASSES] = { "kind", "literal", "length", "rep_length", "distance", "direct" };
	static const char* const type_name[4] = { "literal", "match", "short_rep", "long_rep" };
	const bool want_map = map_path || bucket;
	uint32_t* map = want_map ? (uint32_t*)malloc(sizeof(uint32_t) * n) : NULL;
	mgl_cost_report r;
	if (want_map && !map) { fprintf(stderr, "Error: out of memory\n"); return false; }
	if (mgl_cost_map(sa, slab, &props, map, &r) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); free(map); return false; }
	if (map_path) {
		/* n little-endian u32, one per byte the LZMA layer sees */
		FILE* f = fopen(map_path, "wb");
		bool ok = f != NULL;
		for (size_t p = 0; ok && p < n; p++) {
			const uint8_t le[4] = { (uint8_t)map[p], (uint8_t)(map[p] >> 8), (uint8_t)(map[p] >> 16), (uint8_t)(map[p] >> 24) };
			ok = fwrite(le, 4, 1, f) == 1;
		}
		if (f && fclose(f) != 0) ok = false;
		if (!ok) { fprintf(stderr, "Error: could not write %s\n", map_path); free(map); return false; }
	}
	const double total = r.total ? (double)r.total : 1.0;
	if (tables) {
		fprintf(stderr, "cost-report: total %.3f B exact %llu packets %llu lc=%u lp=%u pb=%u %.3f ms\n", r.total / 16384.0, (unsigned long long)r.total,
		        (unsigned long long)r.packets, props.lc, props.lp, props.pb, r.gpu_ms);
		for (unsigned k = 0; k < MGL_CC_CLASSES; k++)
			fprintf(stderr, "cost-class: %s bits %llu cost %.3f B share %.2f %% exact %llu\n", class_name[k], (unsigned long long)r.class_bits[k],
			        r.class_cost[k] / 16384.0, 100.0 * r.class_cost[k] / total, (unsigned long long)r.class_cost[k]);
		for (unsigned t = 0; t < 4; t++)
			fprintf(stderr, "cost-type: %s packets %llu bytes %llu cost %.3f B share %.2f %% exact %llu\n", type_name[t], (unsigned long long)r.type_packets[t],
			        (unsigned long long)r.type_bytes[t], r.type_cost[t] / 16384.0, 100.0 * r.type_cost[t] / total, (unsigned long long)r.type_cost[t]);
	}
	for (size_t lo = 0, hi = 0; bucket && lo < n; lo = hi) {
		hi = n - lo < bucket ? n : lo + (size_t)bucket;
		uint64_t c = 0;
		for (size_t p = lo; p < hi; p++) c += map[p];
		fprintf(stderr, "cost-bucket: offset %zu bytes %zu cost %.3f B bpb %.4f exact %llu\n", lo, hi - lo, c / 16384.0, c / 2048.0 / (double)(hi - lo),
		        (unsigned long long)c);
	}
	free(map);
	return true;
}

int main(int argc, char** argv)
{
	mgl_sa_config cfg;
	memset(&cfg, 0, sizeof cfg);
	cfg.seed = 1673551; /* main.c:68 */
	cfg.neighbours_per_step = 4096;
	cfg.top_k = 20;     /* main.c:49 */
	mgl_properties props = { 0, 0, 0 }; /* main.c:45 */
	unsigned epochs = 200, phases = 3;  /* main.c:66,69 */
	unsigned long long steps_override = 0;
	const char* filename = NULL;
	const char *out_path = NULL, *save_path = NULL, *load_path = NULL, *seed_stream_path = NULL;
	int clip_window = 0, props_given = 0;
	bool props_auto = false, props_table = false;
	unsigned props_rounds = 3, props_joint = 0;
	uint32_t greedy = 0, optimal = 0, adaptive = 0, mf_depth = 0;
	int finder = MGL_MF_NEAREST;
	bool finder_given = false, parse_sweep = false, parse_sweep_table = false;
	mgl_packet* optimal_slab = NULL;
	double temperature_bytes = 0;
	int accept_mode = MGL_ACCEPT_AUTO;
	int chains = 1, rank = 0, device_given = 0;
	const char* comm_path = NULL;
	unsigned long long comm_nonce = 0;
	int transport_shm = 0;
	int exchange_cross = 0, exchange_all = 0, cross_grain_given = 0;
	uint32_t cross_grain = 0;
	bool format_xz = false, filter_given = false;
	enum { FILTER_NONE, FILTER_X86, FILTER_AUTO } filter = FILTER_NONE;
	uint32_t dict_size = 0;
	bool focus_given = false, focus_rank = false;
	unsigned long long focus_lo = 0, focus_hi = 0;
	const char* cost_map_path = NULL;
	bool cost_report = false;
	unsigned long long cost_bucket = 0;
	for (int i = 1; i < argc; i++) {
		const char* a = argv[i];
		const char* v = i + 1 < argc ? argv[i + 1] : NULL;
		if (a[0] != '-') { filename = a; continue; }
		if (!strcmp(a, "--clip-window")) { clip_window = 1; continue; }
		if (!strcmp(a, "--props-table")) { props_table = true; continue; }
		if (!strcmp(a, "--parse-sweep")) { parse_sweep = true; continue; }
		if (!strcmp(a, "--parse-sweep-table")) { parse_sweep_table = true; continue; }
		if (!strcmp(a, "--cost-report")) { cost_report = true; continue; }
		if (!v) { usage(argv[0]); return -1; }
		if (!strcmp(a, "--neighbours")) cfg.neighbours_per_step = (uint32_t)strtoul(v, NULL, 0);
		else if (!strcmp(a, "--epochs")) epochs = (unsigned)strtoul(v, NULL, 0);
		else if (!strcmp(a, "--phases")) phases = (unsigned)strtoul(v, NULL, 0);
		else if (!strcmp(a, "--steps")) steps_override = strtoull(v, NULL, 0);
		else if (!strcmp(a, "--seed")) cfg.seed = strtoull(v, NULL, 0);
		else if (!strcmp(a, "--lc")) { props.lc = (uint8_t)strtoul(v, NULL, 0); props_given = 1; }
		else if (!strcmp(a, "--lp")) { props.lp = (uint8_t)strtoul(v, NULL, 0); props_given = 1; }
		else if (!strcmp(a, "--pb")) { props.pb = (uint8_t)strtoul(v, NULL, 0); props_given = 1; }
		else if (!strcmp(a, "--props")) {
			if (strcmp(v, "auto") != 0) { usage(argv[0]); return -1; }
			props_auto = true;
		}
		else if (!strcmp(a, "--props-rounds")) { props_rounds = (unsigned)strtoul(v, NULL, 0); if (!props_rounds) { usage(argv[0]); return -1; } }
		else if (!strcmp(a, "--props-joint")) { props_joint = (unsigned)strtoul(v, NULL, 0); if (!props_joint || props_joint > JOINT_MAX) { usage(argv[0]); return -1; } }
		else if (!strcmp(a, "--device")) { cfg.device = (int32_t)strtol(v, NULL, 0); device_given = 1; }
		else if (!strcmp(a, "--chains")) chains = (int)strtol(v, NULL, 0);
		else if (!strcmp(a, "--rank")) rank = (int)strtol(v, NULL, 0);
		else if (!strcmp(a, "--comm-file")) comm_path = v;
		else if (!strcmp(a, "--comm-nonce")) comm_nonce = strtoull(v, NULL, 0);
		else if (!strcmp(a, "--transport")) {
			if (!strcmp(v, "shm")) transport_shm = 1;
			else if (strcmp(v, "rccl") != 0) { usage(argv[0]); return -1; }
		}
		else if (!strcmp(a, "--exchange")) {
			exchange_cross = exchange_all = 0;
			if (!strcmp(v, "cross")) exchange_cross = 1;
			else if (!strcmp(v, "cross-all")) exchange_all = 1;
			else if (strcmp(v, "best") != 0) { usage(argv[0]); return -1; }
		}
		else if (!strcmp(a, "--cross-grain")) { cross_grain = (uint32_t)strtoul(v, NULL, 0); cross_grain_given = 1; }
		else if (!strcmp(a, "--max-scan")) cfg.max_bucket_scan = (uint32_t)strtoul(v, NULL, 0);
		else if (!strcmp(a, "--format")) {
			if (!strcmp(v, "xz")) format_xz = true;
			else if (!strcmp(v, "lzma")) format_xz = false;
			else { usage(argv[0]); return -1; }
		}
		else if (!strcmp(a, "--filter")) {
			if (!strcmp(v, "none")) filter = FILTER_NONE;
			else if (!strcmp(v, "x86")) filter = FILTER_X86;
			else if (!strcmp(v, "auto")) filter = FILTER_AUTO;
			else { usage(argv[0]); return -1; }
			filter_given = true;
		}
		else if (!strcmp(a, "--dict-size")) {
			char* end = NULL;
			const unsigned long long d = strtoull(v, &end, 0);
			if (end == v || *end || (d && d < 4096) || d > 0xFFFFFFFFull) {
				fprintf(stderr, "Error: --dict-size takes a number of bytes from 4096 to 4294967295 (0 = 4 MiB)\n");
				usage(argv[0]);
				return -1;
			}
			dict_size = (uint32_t)d;
		}
		else if (!strcmp(a, "--focus")) {
			if (focus_given) { fprintf(stderr, "Error: --focus given twice\n"); usage(argv[0]); return -1; }
			focus_given = true;
			if (!strcmp(v, "rank")) focus_rank = true;
			else {
				char *e1 = NULL, *e2 = NULL;
				const bool digits = v[0] >= '0' && v[0] <= '9';
				focus_lo = strtoull(v, &e1, 0);
				if (digits && e1 != v && *e1 == ':' && e1[1] >= '0' && e1[1] <= '9') focus_hi = strtoull(e1 + 1, &e2, 0);
				if (!e2 || e2 == e1 + 1 || *e2 || focus_lo >= focus_hi) {
					fprintf(stderr, "Error: --focus takes LO:HI, byte positions with LO < HI, or `rank`\n");
					usage(argv[0]);
					return -1;
				}
			}
		}
		else if (!strcmp(a, "--cost-map")) cost_map_path = v;
		else if (!strcmp(a, "--cost-bucket")) {
			char* end = NULL;
			cost_bucket = strtoull(v, &end, 0);
			if (end == v || *end || !cost_bucket) { fprintf(stderr, "Error: --cost-bucket takes a number of bytes, at least 1\n"); usage(argv[0]); return -1; }
		}
		else if (!strcmp(a, "-o")) out_path = v;
		else if (!strcmp(a, "--save-slab")) save_path = v;
		else if (!strcmp(a, "--load-slab")) load_path = v;
		else if (!strcmp(a, "--greedy-seed")) greedy = (uint32_t)strtoul(v, NULL, 0);
		else if (!strcmp(a, "--optimal-seed")) { optimal = (uint32_t)strtoul(v, NULL, 0); if (!optimal) { usage(argv[0]); return -1; } }
		else if (!strcmp(a, "--adaptive-seed")) { adaptive = (uint32_t)strtoul(v, NULL, 0); if (!adaptive) { usage(argv[0]); return -1; } }
		else if (!strcmp(a, "--match-finder")) {
			if (!strcmp(v, "nearest")) finder = MGL_MF_NEAREST;
			else if (!strcmp(v, "frontier")) finder = MGL_MF_FRONTIER;
			else { usage(argv[0]); return -1; }
			finder_given = true;
		}
		else if (!strcmp(a, "--mf-depth")) { mf_depth = (uint32_t)strtoul(v, NULL, 0); if (!mf_depth || mf_depth > 4096) { usage(argv[0]); return -1; } }
		else if (!strcmp(a, "--seed-stream")) seed_stream_path = v;
		else if (!strcmp(a, "--temperature")) temperature_bytes = strtod(v, NULL);
		else if (!strcmp(a, "--accept")) {
			if (!strcmp(v, "auto")) accept_mode = MGL_ACCEPT_AUTO;
			else if (!strcmp(v, "single")) accept_mode = MGL_ACCEPT_SINGLE;
			else if (!strcmp(v, "bulk")) accept_mode = MGL_ACCEPT_BULK;
			else { usage(argv[0]); return -1; }
		}
		else { usage(argv[0]); return -1; }
		i++;
	}
	if (!filename) { usage(argv[0]); return -1; }
	if (seed_stream_path && (load_path || greedy)) {
		fprintf(stderr, "Error: --seed-stream cannot be combined with --load-slab or --greedy-seed\n");
		usage(argv[0]);
		return -1;
	}
	if (optimal && (greedy || seed_stream_path || load_path)) {
		fprintf(stderr, "Error: --optimal-seed cannot be combined with --greedy-seed, --seed-stream or --load-slab\n");
		usage(argv[0]);
		return -1;
	}
	if (adaptive && (optimal || greedy || seed_stream_path || load_path)) {
		fprintf(stderr, "Error: --adaptive-seed cannot be combined with --optimal-seed, --greedy-seed, --seed-stream or --load-slab\n");
		usage(argv[0]);
		return -1;
	}
	if ((finder_given || mf_depth) && !(optimal || adaptive || props_auto)) {
		fprintf(stderr, "Error: --match-finder / --mf-depth need --optimal-seed, --adaptive-seed or --props auto\n");
		usage(argv[0]);
		return -1;
	}
	if ((parse_sweep && !adaptive) || (parse_sweep_table && !parse_sweep)) { usage(argv[0]); return -1; }
	if (parse_sweep && finder_given) {
		fprintf(stderr, "Error: --parse-sweep runs both match finders; --match-finder cannot be combined with it\n");
		usage(argv[0]);
		return -1;
	}
	if (mf_depth && finder != MGL_MF_FRONTIER && !parse_sweep) { usage(argv[0]); return -1; }
	const seed_spec seed = { adaptive ? adaptive : optimal, adaptive != 0, finder, mf_depth, parse_sweep, parse_sweep_table }; /* passes 0: no seed of this kind */
	if (clip_window && !seed_stream_path) { usage(argv[0]); return -1; }
	if (props_auto && (props_given || chains > 1)) {
		fprintf(stderr, "Error: --props auto cannot be combined with --lc/--lp/--pb or with --chains above 1\n");
		usage(argv[0]);
		return -1;
	}
	if (props_table && !props_auto) { usage(argv[0]); return -1; }
	if (props_joint && !(props_auto && adaptive && parse_sweep)) {
		fprintf(stderr, "Error: --props-joint needs --props auto --adaptive-seed P --parse-sweep\n");
		usage(argv[0]);
		return -1;
	}
	if (cross_grain_given && !exchange_cross && !exchange_all) {
		fprintf(stderr, "Error: --cross-grain needs --exchange cross or --exchange cross-all\n");
		usage(argv[0]);
		return -1;
	}
	if (filter != FILTER_NONE && !format_xz) {
		fprintf(stderr, "Error: --filter x86 / auto need --format xz: an .lzma stream has no place to declare a filter\n");
		usage(argv[0]);
		return -1;
	}
	if (filter == FILTER_AUTO && (seed_stream_path || load_path || chains > 1)) {
		fprintf(stderr, "Error: --filter auto cannot be combined with --seed-stream, --load-slab or --chains above 1\n");
		usage(argv[0]);
		return -1;
	}
	if (focus_rank && chains < 2) {
		fprintf(stderr, "Error: --focus rank needs --chains N with N at least 2\n");
		usage(argv[0]);
		return -1;
	}
	cfg.dict_limit = dict_size; /* 0: the library's 4 MiB */
	if (chains < 1 || rank < 0 || rank >= chains || (chains > 1 && !comm_path)) { usage(argv[0]); return -1; }
	if (chains > 1) {
		if (!device_given) cfg.device = rank;
		/* distinct, reproducible RNG stream per chain (the same rule as megalania_amd/multi_gpu.py:chain_seed) */
		if (rank) cfg.seed ^= 0x9E3779B97F4A7C15ull * (uint64_t)(rank + 1);
	}

	int fd = open(filename, O_RDONLY);
	if (fd < 0) { fprintf(stderr, "Error: could not open %s\n", filename); return -1; }
	struct stat sb;
	if (fstat(fd, &sb) < 0) { fprintf(stderr, "Error: could not stat %s\n", filename); close(fd); return -1; }
	const size_t file_size = (size_t)sb.st_size;
	if (file_size == 0) { close(fd); return 0; } /* main.c:40-42 */
	/* orig_data: the file.  file_data: what the LZMA layer sees, the file itself or (--filter x86) its filtered copy; the
	 * handle, the seeds, the slabs and the chains all work on file_data, and only the .xz writer looks at both */
	const uint8_t* const orig_data = (const uint8_t*)mmap(NULL, file_size, PROT_READ, MAP_PRIVATE, fd, 0);
	const uint8_t* file_data = orig_data;
	uint8_t* filtered = NULL;
	if (orig_data == MAP_FAILED) { fprintf(stderr, "Error: could not map %s\n", filename); close(fd); return -1; }

	if (mgl_device_count() < 1) {
		fprintf(stderr, "Error: no HIP device found; this program has no CPU search path\n");
		return -1;
	}
	/* --seed-stream: the stream's properties unless --lc/--lp/--pb say otherwise (a parse is valid under any) */
	uint8_t* seed_stream = NULL;
	size_t seed_stream_len = 0;
	if (seed_stream_path) {
		FILE* f = fopen(seed_stream_path, "rb");
		long sz = -1;
		if (f && fseek(f, 0, SEEK_END) == 0) sz = ftell(f);
		if (sz > 0 && fseek(f, 0, SEEK_SET) == 0 && (seed_stream = (uint8_t*)malloc((size_t)sz)) != NULL &&
		    fread(seed_stream, 1, (size_t)sz, f) == (size_t)sz)
			seed_stream_len = (size_t)sz;
		if (f) fclose(f);
		mgl_stream_info info;
		uint32_t stream_filter = 0;
		if (!seed_stream_len || mgl_stream_info_read_x(seed_stream, seed_stream_len, &info, &stream_filter) != MGL_OK) {
			fprintf(stderr, "Error: %s is not an LZMA-alone or .xz stream\n", seed_stream_path);
			return -1;
		}
		if (stream_filter == 4) {
			if (!format_xz) {
				fprintf(stderr, "Error: %s declares the x86 BCJ filter, which an .lzma stream cannot declare: use --format xz\n", seed_stream_path);
				return -1;
			}
			if (filter_given && filter == FILTER_NONE) {
				fprintf(stderr, "Error: %s declares the x86 BCJ filter, so its parse is one of the filtered input: not with --filter none\n", seed_stream_path);
				return -1;
			}
			filter = FILTER_X86;
		}
		if (!props_given) props = info.props;
		else if (props.lc != info.props.lc || props.lp != info.props.lp || props.pb != info.props.pb)
			fprintf(stderr, "note: %s was coded with lc/lp/pb %u/%u/%u; searching with the given %u/%u/%u\n", seed_stream_path,
			        info.props.lc, info.props.lp, info.props.pb, props.lc, props.lp, props.pb);
	}
	cfg.iters_per_epoch = file_size;
	if (filter != FILTER_NONE) {
		if ((filtered = (uint8_t*)malloc(file_size)) == NULL) { fprintf(stderr, "Error: out of memory\n"); return -1; }
		memcpy(filtered, orig_data, file_size);
		mgl_bcj_x86(filtered, file_size, 1);
	}
	if (filter == FILTER_X86) file_data = filtered;
	mgl_sa* sa = mgl_sa_create(file_data, file_size, props, &cfg);
	if (sa == NULL) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
	bool filter_seed_kept = false;
	if (filter == FILTER_AUTO) {
		/* The same seed over the plain bytes (on `sa`) and over the filtered ones, one handle after the other; the cheaper
		 * exact cost wins and a tie goes to none.  Where the filter changes no byte the two parses are the same one. */
		mgl_packet* parse[2] = { (mgl_packet*)malloc(sizeof(mgl_packet) * file_size), (mgl_packet*)malloc(sizeof(mgl_packet) * file_size) };
		uint64_t cost[2] = { 0, 0 };
		if (!parse[0] || !parse[1]) { fprintf(stderr, "Error: out of memory\n"); return -1; }
		if (make_filter_seed(sa, greedy, seed, parse[0], &cost[0]) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
		const bool changed = memcmp(filtered, orig_data, file_size) != 0;
		cost[1] = cost[0];
		if (changed) {
			mgl_sa_destroy(sa);
			if ((sa = mgl_sa_create(filtered, file_size, props, &cfg)) == NULL || make_filter_seed(sa, greedy, seed, parse[1], &cost[1]) != MGL_OK) {
				fprintf(stderr, "Error: %s\n", mgl_last_error());
				return -1;
			}
		}
		const int win = cost[1] < cost[0];
		fprintf(stderr, "filter auto: none %llu x86 %llu -> %s (exact costs %llu %llu)\n", (unsigned long long)((cost[0] + 16383) / 16384),
		        (unsigned long long)((cost[1] + 16383) / 16384), win ? "x86" : "none", (unsigned long long)cost[0], (unsigned long long)cost[1]);
		filter = win ? FILTER_X86 : FILTER_NONE;
		file_data = win ? filtered : orig_data;
		/* the handle alive is the filtered bytes' when they were looked at; --props auto wants an untouched one */
		if (changed ? (!win || props_auto) : props_auto) {
			mgl_sa_destroy(sa);
			if ((sa = mgl_sa_create(file_data, file_size, props, &cfg)) == NULL) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
		}
		if (seed.passes && !props_auto) { optimal_slab = parse[win]; filter_seed_kept = true; }
		else free(parse[win]);
		free(parse[!win]);
	}
	if (props_auto) {
		/* the parse to look at: the seed the user asked for; without one an optimal seed at its defaults, for the sweep only */
		mgl_packet* parse = (mgl_packet*)malloc(sizeof(mgl_packet) * file_size);
		bool fixed = true;
		uint64_t unused = 0;
		if (!parse) { fprintf(stderr, "Error: out of memory\n"); return -1; }
		if (seed_stream) {
			mgl_import_stats ist;
			if (mgl_stream_import(seed_stream, seed_stream_len, file_data, file_size, cfg.dict_limit, (clip_window ? MGL_IMPORT_CLIP_WINDOW : 0) | (filter == FILTER_X86 ? MGL_IMPORT_X86 : 0),
			                      parse, &ist) != MGL_OK) {
				fprintf(stderr, "Error: %s: %s at input position %llu\n", seed_stream_path, ist.error ? ist.error : "import failed",
				        (unsigned long long)ist.error_pos);
				return -1;
			}
		} else if (load_path) {
			if (!read_slab_file(load_path, file_size, parse, &unused)) { fprintf(stderr, "Error: %s is not a slab for this input\n", load_path); return -1; }
		} else if (greedy) {
			/* the greedy parse does not look at the properties: made once, on a handle that is then replaced */
			if (mgl_sa_seed_greedy(sa, greedy) != MGL_OK || mgl_sa_current(sa, parse, &unused) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
			mgl_sa_destroy(sa);
			if ((sa = mgl_sa_create(file_data, file_size, props, &cfg)) == NULL) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
		} else {
			fixed = false;
			if ((optimal_slab = (mgl_packet*)malloc(sizeof(mgl_packet) * file_size)) == NULL) { fprintf(stderr, "Error: out of memory\n"); return -1; }
		}
		if (props_joint) sa = choose_props_joint(sa, file_data, file_size, &cfg, &props, seed, props_joint, props_table, optimal_slab);
		else sa = choose_props(sa, file_data, file_size, &cfg, &props, parse, fixed, seed, props_rounds, props_table, optimal_slab);
		if (sa == NULL) return -1;
		free(parse);
		if (!seed.passes) { free(optimal_slab); optimal_slab = NULL; } /* no seed option: the search starts from the all-literal slab */
	}

	if (temperature_bytes > 0 && mgl_sa_set_temperature(sa, (uint64_t)(temperature_bytes * 16384.0)) != MGL_OK) {
		fprintf(stderr, "Error: %s\n", mgl_last_error());
		return -1;
	}
	mgl_comm* comm = NULL;
	if (comm_path && transport_shm) {
		if (mgl_comm_init_shm(&comm, comm_path, comm_nonce, rank, chains, cfg.device) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
	} else if (comm_path) { /* also with --chains 1: the same code path on a one-GPU box */
		/* rendezvous file: "MGLCOMM1", u64 nonce, the 128-byte RCCL id.  Rank 0 replaces whatever an earlier run left
		 * under the name and removes it again once every chain has joined; the others only take a file of this run */
		uint8_t uid[128];
		if (rank == 0) {
			char tmp[4096];
			snprintf(tmp, sizeof tmp, "%s.tmp", comm_path);
			(void)unlink(comm_path);
			FILE* f = fopen(tmp, "wb");
			const uint64_t nonce = comm_nonce;
			if (mgl_comm_unique_id(uid) != MGL_OK || !f || fwrite("MGLCOMM1", 8, 1, f) != 1 || fwrite(&nonce, 8, 1, f) != 1 ||
			    fwrite(uid, 128, 1, f) != 1 || fclose(f) != 0 || rename(tmp, comm_path) != 0) {
				fprintf(stderr, "Error: could not publish the communicator id in %s: %s\n", comm_path, mgl_last_error());
				return -1;
			}
		} else {
			const char* te = getenv("MGL_COMM_TIMEOUT_S");
			const double limit = te && atof(te) > 0 ? atof(te) : 600.0;
			bool got = false;
			for (double waited = 0; !got && waited < limit; waited += 0.1) {
				FILE* f = fopen(comm_path, "rb");
				char magic[8];
				uint64_t nonce = 0;
				if (f && fread(magic, 8, 1, f) == 1 && !memcmp(magic, "MGLCOMM1", 8) && fread(&nonce, 8, 1, f) == 1 && nonce == comm_nonce &&
				    fread(uid, 128, 1, f) == 1) got = true;
				if (f) fclose(f);
				if (!got) usleep(100000);
			}
			if (!got) { fprintf(stderr, "Error: no communicator id of this run (--comm-nonce %llu) appeared in %s\n", comm_nonce, comm_path); return -1; }
		}
		if (mgl_comm_init(&comm, uid, rank, chains, cfg.device) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
		if (rank == 0) (void)unlink(comm_path); /* ncclCommInitRank returns once every rank has joined: nobody reads the file any more */
	}
	if (mgl_sa_set_accept_mode(sa, accept_mode, 0) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
	mgl_packet* packets_best = (mgl_packet*)malloc(sizeof(mgl_packet) * file_size);
	if (packets_best == NULL) { fprintf(stderr, "Error: out of memory\n"); return -1; }
	bool resumed = false;
	if (load_path) {
		uint64_t perplexity = 0;
		if (!read_slab_file(load_path, file_size, packets_best, &perplexity)) {
			fprintf(stderr, "Error: %s is not a slab for this input\n", load_path);
			return -1;
		}
		/* --props auto: the file's perplexity belongs to the triple it was saved under; the slab is costed under the chosen one */
		if (props_auto && mgl_cost_slab(sa, packets_best, &perplexity, NULL, NULL) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
		/* the library re-costs the slab and refuses it unless the perplexity matches */
		if (mgl_sa_set_best(sa, packets_best, perplexity) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
		resumed = true;
	}
	if (seed_stream) {
		/* the stream's parse, re-expressed for one LZMA1 stream, becomes the best slab (re-costed and checked by
		 * the library like a --load-slab one); every epoch then starts from the best slab */
		mgl_import_stats ist;
		const int irc = mgl_stream_import(seed_stream, seed_stream_len, file_data, file_size, cfg.dict_limit,
		                                  (clip_window ? MGL_IMPORT_CLIP_WINDOW : 0) | (filter == FILTER_X86 ? MGL_IMPORT_X86 : 0), packets_best, &ist);
		if (irc != MGL_OK) {
			fprintf(stderr, "Error: %s: %s at input position %llu%s\n", seed_stream_path, ist.error ? ist.error : "import failed",
			        (unsigned long long)ist.error_pos, irc == MGL_ERANGE ? " (--clip-window turns such copies into literals)" : "");
			return -1;
		}
		uint64_t cost = 0;
		size_t npk = 0;
		if (mgl_cost_slab(sa, packets_best, &cost, NULL, &npk) != MGL_OK || mgl_sa_set_best(sa, packets_best, cost) != MGL_OK) {
			fprintf(stderr, "Error: %s\n", mgl_last_error());
			return -1;
		}
		fprintf(stderr, "seed stream: %zu packets, estimate %f bytes, stream %zu bytes, %llu re-expressed, %llu clipped\n", npk,
		        18 + cost / 16384.f, seed_stream_len, (unsigned long long)ist.reexpressed, (unsigned long long)ist.clipped);
		free(seed_stream);
		resumed = true;
	}

	if (seed.passes && !props_auto && !filter_seed_kept) { /* --props auto kept the parse of its cheapest (triple, parse) pair in optimal_slab */
		/* made once; every epoch that would start from the all-literal slab starts from it */
		mgl_optimal_stats os;
		uint64_t cost = 0;
		optimal_slab = (mgl_packet*)malloc(sizeof(mgl_packet) * (file_size ? file_size : 1));
		if (!optimal_slab || make_seed(sa, seed, &os) != MGL_OK || mgl_sa_current(sa, optimal_slab, &cost) != MGL_OK) {
			fprintf(stderr, "Error: %s\n", optimal_slab ? mgl_last_error() : "out of memory");
			return -1;
		}
		double ms = 0;
		for (uint32_t p = 0; p < os.passes; p++) ms += os.ms[p];
		char mf[96] = "nearest";
		if (seed.sweep) snprintf(mf, sizeof mf, "chosen by the parse sweep");
		else if (seed.finder == MGL_MF_FRONTIER) {
			/* the lists the seed used are still in the handle: only their count and build time are asked for */
			size_t entries = 0;
			double build_ms = 0;
			if (mgl_match_frontier(sa, seed.mf_depth, NULL, NULL, NULL, (size_t)-1, &entries, &build_ms) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
			snprintf(mf, sizeof mf, "frontier, %zu entries built in %.2f ms", entries, build_ms);
		}
		fprintf(stderr, "%s seed: %u passes in %.1f ms, estimate %f bytes (greedy parse %f), match finder %s\n", seed.adaptive ? "adaptive" : "optimal", os.passes, ms,
		        18 + cost / 16384.f, 18 + os.greedy_cost / 16384.f, mf);
	}

	if (focus_given && !focus_rank && mgl_sa_set_focus(sa, focus_lo, focus_hi) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
	unsigned long long steps_per_epoch = (file_size + cfg.neighbours_per_step - 1) / cfg.neighbours_per_step;
	if (steps_override) steps_per_epoch = steps_override;
	for (unsigned phase = 0; phase < phases; phase++) {
		for (unsigned epoch = 0; epoch < epochs; epoch++) {
			if (focus_rank) {
				/* chain `rank`'s slice for this round; the rounds count the epochs of the whole run, which the chains share */
				uint64_t lo = 0, hi = 0;
				if (mgl_focus_slice(file_size, (uint32_t)chains, (uint32_t)rank, (uint64_t)phase * epochs + epoch, &lo, &hi) != MGL_OK ||
				    mgl_sa_set_focus(sa, lo, hi) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
			}
			if (mgl_sa_begin_epoch(sa, phase, phase != 0 || resumed) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
			if (greedy && phase == 0 && !resumed && mgl_sa_seed_greedy(sa, greedy) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
			if (seed.passes && phase == 0 && mgl_sa_set_slab(sa, optimal_slab) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
			mgl_sa_stats st;
			if (mgl_sa_run(sa, steps_per_epoch, &st) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
			/* main.c:97-99: 18 = 13 header bytes + 5 flush bytes, 16384 = 2048 * 8 */
			fprintf(stderr, "current file size: %f\tbest: %f\tstep: %u\tepoch: %04u\t%.0f evals/s\n",
			        18 + st.current_cost / 16384.f, 18 + st.best_cost / 16384.f, phase + 1, epoch,
			        st.gpu_ms_total > 0 ? st.evaluations / (st.gpu_ms_total * 1e-3) : 0.0);
			if (comm && exchange_all) {
				mgl_cross_all_stats as;
				if (mgl_sa_exchange_cross_all(sa, comm, cross_grain, &as) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
				char owners[8 * MGL_XO_MAX_PARENTS + 1] = "";
				for (uint32_t p = 0; p < as.distinct; p++) snprintf(owners + strlen(owners), sizeof owners - strlen(owners), p ? " %u" : "%u", as.parent_rank[p]);
				const uint64_t now = as.cross.adopted == 2 ? as.cross.child_cost : as.cross.parent_cost[0];
				if (as.cross.parents)
					fprintf(stderr, "exchange: cross-all: %u distinct of %u best slabs, parents from chains [%s], cheapest %f bytes, child %f bytes of %llu regions, "
					        "adopted %u, best %f bytes, %.2f ms\n", as.distinct, as.chains_with_best, owners, 18 + as.cross.parent_cost[0] / 16384.f,
					        18 + as.cross.child_cost / 16384.f, (unsigned long long)(as.cross.boundaries - 1), as.cross.adopted, 18 + now / 16384.f, as.cross.gpu_ms);
				else if (as.distinct)
					fprintf(stderr, "exchange: cross-all: %u distinct of %u best slabs, parents from chains [%s], nothing crossed%s, adopted %u, best %f bytes\n",
					        as.distinct, as.chains_with_best, owners, as.fell_back ? " (a chain had no room for the buffers)" : "", as.cross.adopted, 18 + now / 16384.f);
				else
					fprintf(stderr, "exchange: cross-all: no chain has a best slab yet, adopted 0\n");
			} else if (comm) {
				int winner = -1;
				uint64_t wcost = 0;
				mgl_cross_stats xs;
				if ((exchange_cross ? mgl_sa_exchange_cross(sa, comm, cross_grain, &winner, &wcost, &xs) : mgl_sa_exchange_best(sa, comm, &winner, &wcost)) != MGL_OK) {
					fprintf(stderr, "Error: %s\n", mgl_last_error());
					return -1;
				}
				fprintf(stderr, "exchange: chain %d holds the best slab, %f bytes\n", winner, 18 + wcost / 16384.f);
				if (exchange_cross && xs.parents)
					fprintf(stderr, "cross: chain %d: own %f, child %f of %llu regions (%llu own), %s (adopted %u), %.2f ms\n", rank, 18 + xs.parent_cost[0] / 16384.f,
					        18 + xs.child_cost / 16384.f, (unsigned long long)(xs.boundaries - 1), (unsigned long long)xs.regions_from[0],
					        xs.adopted == 2 ? "the child is the new best" : xs.adopted == 1 ? "the winner's slab adopted" : "own best kept", xs.adopted, xs.gpu_ms);
				else if (exchange_cross)
					fprintf(stderr, "cross: chain %d: nothing crossed (adopted %u)\n", rank, xs.adopted);
			}
			if (save_path && st.best_cost != 0) {
				uint64_t hdr[2] = { file_size, 0 };
				if (mgl_sa_best(sa, packets_best, &hdr[1]) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
				/* one checkpoint per chain: chain R > 0 writes <file>.rankR (the chains run the same command line) */
				char dst[4096], tmp[4200];
				if (rank) snprintf(dst, sizeof dst, "%s.rank%d", save_path, rank);
				else snprintf(dst, sizeof dst, "%s", save_path);
				snprintf(tmp, sizeof tmp, "%s.tmp", dst);
				FILE* f = fopen(tmp, "wb");
				if (!f || fwrite("MGLSLAB1", 8, 1, f) != 1 || fwrite(hdr, 8, 2, f) != 2 ||
				    fwrite(packets_best, sizeof(mgl_packet), file_size, f) != file_size || fclose(f) != 0 || rename(tmp, dst) != 0)
					fprintf(stderr, "warning: could not write %s\n", dst);
			}
		}
	}

	if (comm && exchange_cross) {
		/* the crossing exchanges leave every chain its own best slab: one plain exchange, so that rank 0 writes the overall best */
		int winner = -1;
		uint64_t wcost = 0;
		if (mgl_sa_exchange_best(sa, comm, &winner, &wcost) != MGL_OK) { fprintf(stderr, "Error: %s\n", mgl_last_error()); return -1; }
		fprintf(stderr, "exchange: chain %d holds the best slab, %f bytes\n", winner, 18 + wcost / 16384.f);
	}
	uint64_t best = 0;
	if (mgl_sa_best(sa, packets_best, &best) != MGL_OK) {
		fprintf(stderr, "Error: could not fetch the best slab: %s\n", mgl_last_error());
		return -1;
	}
	if (rank == 0 && (cost_map_path || cost_report || cost_bucket) &&
	    !report_costs(sa, packets_best, file_size, props, cost_map_path, cost_report, cost_bucket)) return -1;
	mgl_comm_destroy(comm);
	mgl_sa_destroy(sa);
	if (rank != 0) return 0; /* every chain holds the common best slab after the last exchange; rank 0 writes it */

	FILE* out = stdout;
	if (out_path && (out = fopen(out_path, "wb")) == NULL) { fprintf(stderr, "Error: could not open %s\n", out_path); return -1; }
	OutputInterface output;
	mgl_file_output_new(&output, out);
	if (format_xz) {
		const mgl_xz_options xo = { filter == FILTER_X86 ? 4u : 0u, dict_size, 1 };
		if (!mgl_emit_xz(orig_data, file_data, file_size, props, packets_best, &xo, &output)) return -1;
	} else if (dict_size) {
		if (!mgl_emit_stream_dict(file_data, file_size, props, packets_best, dict_size, &output)) return -1;
	} else if (!mgl_emit_stream(file_data, file_size, props, packets_best, &output)) return -1;
	if (out_path ? fclose(out) != 0 : fflush(stdout) != 0) { fprintf(stderr, "Error: could not write the stream\n"); return -1; }
	free(optimal_slab);
	free(packets_best);
	free(filtered);
	munmap((void*)orig_data, file_size);
	close(fd);
	return 0;
}
