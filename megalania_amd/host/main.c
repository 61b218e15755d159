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
 *
 * The file reads top to bottom: the options (cli_opts: parse_args fills it, check_args refuses what cannot be combined,
 * before the input is opened and before a device is looked for), the run's context (cli_run) with its helpers, the
 * stages over that context, each returning 0 or the exit status, and main(), which is the list of the stages.
 */
#include <fcntl.h>
#include <stdarg.h>
#include <stdbool.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "mgl_host.h"

static const char usage_options[] =
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
	"  --target-weights cost[:mean|:N] | file:PATH  the search draws a step's targets in proportion to a weight per input byte\n"
	"               (mgl_sa_set_target_weights) instead of uniformly by packet; with --focus, inside the window.  cost: before\n"
	"               every epoch's run the weights become the cost map of the slab the epoch starts from plus a floor per byte,\n"
	"               made on the device: cost:mean (= cost) adds the mean cost of a byte, so that half the weight is uniform by\n"
	"               byte and no stretch starves, cost:N adds N, cost:0 is the pure map.  file:PATH: one little-endian u32 per\n"
	"               input byte, the format --cost-map writes (with --filter x86 per filtered byte), set once for the whole run;\n"
	"               a file of another size is an error and nothing is written.  With --chains every chain has its own weights\n"
	"  --live-weights R[:N|:mean][,single]  target weights that follow the search (mgl_sa_set_live_weights): before every R-th step\n"
	"               of the handle, and before the first step of an epoch, the weights become the cost map of the slab as it\n"
	"               stands plus a floor per byte -- N (default 0, the pure map) or, with mean, the map's mean --, read off the\n"
	"               engine's event chains on the device.  ,single: only single-route steps use and refresh them, so that under\n"
	"               --accept auto the weights come on once the slab has stopped offering improving neighbours in bulk.  One\n"
	"               line per epoch on stderr: `live-weights: every R steps, floor F, refreshes M, skipped S, X ms` (the counts\n"
	"               since the start).  Not together with --target-weights.  With --chains every chain has its own weights\n"
	"  --cost-map FILE  where the emitted parse spends its bits (mgl_cost_map, under the run's final lc/lp/pb): FILE gets one\n"
	"               little-endian u32 per input byte, the byte's share of its packet's exact cost (2048 per bit); the values\n"
	"               sum to the parse's cost.  With --filter x86 the positions are those of the filtered bytes.  The emitted\n"
	"               stream is the same with and without this option and the next two; each may be given alone\n"
	"  --cost-report    print to stderr one line per coder and per packet type of the emitted parse:\n"
	"               `cost-class: NAME bits N cost X B share P % exact C` (kind, literal, length, rep_length, distance, direct)\n"
	"               `cost-type: NAME packets N bytes M cost X B share P % exact C` (literal, match, short_rep, long_rep)\n"
	"               behind `cost-report: total X B exact C packets N lc=.. lp=.. pb=.. T ms`; X = C / 16384\n"
	"  --cost-bucket B  print one line per B input bytes: `cost-bucket: offset O bytes N cost X B bpb R exact C`\n"
	"  --segment-props GRAIN|auto  with --format xz: after the search the best parse is cut at about every GRAIN bytes (auto =\n"
	"               65536; at most 16 leaves, so at least a sixteenth of the input each), every run of leaves is costed from an\n"
	"               LZMA2 state reset under all 75 lc/lp/pb at once (mgl_props_sweep_spans) and the stream is written in the\n"
	"               cheapest segments (mgl_segment_partition, 11 bytes charged per further segment), each behind a chunk that\n"
	"               resets the state and sets its triple; the dictionary runs through.  Never larger in exact cost than the\n"
	"               stream under the best single triple.  Two kinds of lines on stderr:\n"
	"               `segment-props: grain G cuts C spans S single lc=.. lp=.. pb=.. X B exact C segmented X B exact C segments M T ms`\n"
	"               `segment: offset O bytes N lc=.. lp=.. pb=.. cost X B exact C reexpressed R` (X = C / 16384; R = rep packets\n"
	"               named again against the segment's own rep stack).  Not with --cost-map, --cost-report or --cost-bucket,\n"
	"               which describe a stream under one triple\n"
	"  --segment-reparse P  with --segment-props: the chosen segments are parsed again, each for the coder that codes it -- P\n"
	"               (1..16) passes of the adaptive parse from the state reset at the segment's start, under the segment's own\n"
	"               triple, copies still reaching below the cut (mgl_segment_reparse; --match-finder / --mf-depth apply).  A\n"
	"               segment keeps its packets unless a pass costs less, and the whole result is dropped unless it costs less in\n"
	"               total, so the stream never grows.  One round; lines on stderr:\n"
	"               `segment-reparse: passes P segments M reparsed R taken 0|1 was X B exact C now X B exact C T ms`\n"
	"               `segment-parse: offset O bytes N lc=.. lp=.. pb=.. start X B exact C best X B exact C pass p|- final X B exact C`\n"
	"  --accept     what a step of K neighbours takes: the best acceptable one (single), every one that is\n"
	"               the best of its own window (bulk), or whichever pays (auto, default)\n";

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
	        "          [--target-weights cost[:mean|:N]|file:PATH]\n"
	        "          [--live-weights R[:N|:mean][,single]]\n"
	        "          [--cost-map FILE] [--cost-report] [--cost-bucket B] [--segment-reparse P] [--segment-props GRAIN|auto] filename\n", argv0);
	fputs(usage_options, stderr);
}

/* ---- options ---- */

/* the seed made on the device: the best of `passes` optimal parses, under static prices or (adaptive) the live model's */
typedef struct { uint32_t passes; bool adaptive; int finder; uint32_t mf_depth; bool sweep, sweep_table; } seed_spec;

enum { FILTER_NONE, FILTER_X86, FILTER_AUTO };          /* in the order of --filter's words */
enum { EXCHANGE_BEST, EXCHANGE_CROSS, EXCHANGE_ALL };   /* in the order of --exchange's words */
enum { WEIGHTS_NONE, WEIGHTS_COST_MEAN, WEIGHTS_COST_FLOOR, WEIGHTS_FILE }; /* --target-weights */
#define JOINT_MAX 4 /* --props-joint's candidates */

/* everything the command line says, grouped as the usage text groups it */
typedef struct {
	const char* argv0;
	/* search: cfg holds --neighbours, --seed, --device, --max-scan and, from check_args, the dictionary and the chain's device and seed */
	mgl_sa_config cfg;
	unsigned epochs, phases, accept_mode;
	unsigned long long steps;
	double temperature_bytes;
	bool device_given;
	/* props */
	mgl_properties props;
	uint32_t props_rounds, props_joint;
	bool props_given, props_auto, props_table;
	/* seed: `seed` is what check_args makes of --optimal-seed / --adaptive-seed and what goes with them */
	uint32_t greedy, optimal, adaptive, mf_depth, finder;
	bool finder_given, parse_sweep, parse_sweep_table, clip_window;
	seed_spec seed;
	/* format, filter */
	uint32_t filter, dict_size;
	bool format_xz, filter_given;
	/* --segment-props: the grain, 0 for auto */
	bool segment_props;
	unsigned long long segment_grain;
	uint32_t segment_reparse; /* --segment-reparse: the passes, 0 for none */
	bool segment_reparse_given;
	/* chains, exchange */
	int chains, rank;
	uint32_t exchange, cross_grain;
	unsigned long long comm_nonce;
	bool transport_shm, cross_grain_given;
	/* focus, target weights, cost map */
	unsigned long long focus_lo, focus_hi, cost_bucket;
	bool focus_given, focus_rank, cost_report;
	unsigned weights; /* WEIGHTS_* */
	uint32_t weights_floor;
	const char* weights_path;
	bool live_given;
	mgl_live_weights_config live; /* --live-weights */
	/* files */
	const char *filename, *out_path, *save_path, *load_path, *seed_stream_path, *comm_path, *cost_map_path;
} cli_opts;

/* a refused command line: the reason, where the rule has one, and the usage text */
static int refuse(const cli_opts* o, const char* why)
{
	if (why) fprintf(stderr, "Error: %s\n", why);
	usage(o->argv0);
	return -1;
}

/* v as a count of lo..hi, after the cast to 32 bits */
static bool count_in(const char* v, uint32_t lo, uint32_t hi, uint32_t* out)
{
	*out = (uint32_t)strtoul(v, NULL, 0);
	return *out >= lo && *out <= hi;
}

/* the index of v among the words (w2 nullable), -1 for none of them */
static int word(const char* v, const char* w0, const char* w1, const char* w2)
{
	return !strcmp(v, w0) ? 0 : !strcmp(v, w1) ? 1 : w2 && !strcmp(v, w2) ? 2 : -1;
}

/* v as a number and nothing else */
static bool number(const char* v, unsigned long long* out)
{
	char* end = NULL;
	*out = strtoull(v, &end, 0);
	return end != v && !*end;
}

/* --focus LO:HI|rank: the reason for a refusal, NULL for none */
static const char* parse_focus(const char* v, cli_opts* o)
{
	if (o->focus_given) return "--focus given twice";
	o->focus_given = true;
	if (!strcmp(v, "rank")) { o->focus_rank = true; return NULL; }
	char *e1 = NULL, *e2 = NULL;
	const bool digits = v[0] >= '0' && v[0] <= '9';
	o->focus_lo = strtoull(v, &e1, 0);
	if (digits && e1 != v && *e1 == ':' && e1[1] >= '0' && e1[1] <= '9') o->focus_hi = strtoull(e1 + 1, &e2, 0);
	if (!e2 || e2 == e1 + 1 || *e2 || o->focus_lo >= o->focus_hi) return "--focus takes LO:HI, byte positions with LO < HI, or `rank`";
	return NULL;
}

/* --target-weights cost[:mean|:N] | file:PATH: the reason for a refusal, NULL for none */
static const char* parse_target_weights(const char* v, cli_opts* o)
{
	static const char* const malformed = "--target-weights takes cost, cost:mean, cost:N (N from 0 to 4293918719) or file:PATH";
	unsigned long long n = 0;
	if (o->weights != WEIGHTS_NONE) return "--target-weights given twice";
	if (!strcmp(v, "cost") || !strcmp(v, "cost:mean")) o->weights = WEIGHTS_COST_MEAN;
	else if (!strncmp(v, "cost:", 5) && v[5] >= '0' && v[5] <= '9' && number(v + 5, &n) && n <= 0xFFFFFFFFull - (1u << 20)) {
		o->weights = WEIGHTS_COST_FLOOR; /* a map entry is below 2^20: entry + N fits 32 bits */
		o->weights_floor = (uint32_t)n;
	} else if (!strncmp(v, "file:", 5) && v[5]) {
		o->weights = WEIGHTS_FILE;
		o->weights_path = v + 5;
	} else return malformed;
	return NULL;
}

/* --live-weights R[:N|:mean][,single]: the reason for a refusal, NULL for none */
static const char* parse_live_weights(const char* v, cli_opts* o)
{
	static const char* const malformed = "--live-weights takes R, R:N, R:mean (R from 1, N from 0 to 4293918719), optionally followed by ,single";
	char* end = NULL;
	if (o->live_given) return "--live-weights given twice";
	o->live_given = true;
	if (v[0] < '0' || v[0] > '9') return malformed;
	const unsigned long long every = strtoull(v, &end, 10);
	if (every < 1 || every > 0xFFFFFFFFull) return malformed;
	o->live = (mgl_live_weights_config){ .every = (uint32_t)every };
	if (!strncmp(end, ":mean", 5)) { o->live.floor_mean = 1; end += 5; }
	else if (*end == ':') {
		if (end[1] < '0' || end[1] > '9') return malformed;
		const unsigned long long n = strtoull(end + 1, &end, 10);
		if (n > 0xFFFFFFFFull - (1u << 20)) return malformed; /* a map entry is below 2^20: entry + N fits 32 bits */
		o->live.floor = (uint32_t)n;
	}
	if (!strcmp(end, ",single")) o->live.flags = MGL_LW_SINGLE_ONLY;
	else if (*end) return malformed;
	return NULL;
}

/* The last of a repeated option wins (--focus, --target-weights and --live-weights refuse a repeat), the last non-option argument is the file name. */
static int parse_args(int argc, char** argv, cli_opts* o)
{
	/* the reference's seed (main.c:68), top K (:49), props 0/0/0 (:45) and schedule (:66,69) */
	*o = (cli_opts){ .argv0 = argv[0], .cfg = { .seed = 1673551, .neighbours_per_step = 4096, .top_k = 20 }, .epochs = 200, .phases = 3,
	                 .props_rounds = 3, .chains = 1 };
	for (int i = 1; i < argc; i++) {
		const char* a = argv[i];
		const char* v = i + 1 < argc ? argv[i + 1] : NULL;
		const char* why = NULL;
		unsigned long long n = 0;
		bool bad = false;
		int w = 0;
		if (a[0] != '-') { o->filename = a; continue; }
		if (!strcmp(a, "--clip-window")) { o->clip_window = true; continue; }
		if (!strcmp(a, "--props-table")) { o->props_table = true; continue; }
		if (!strcmp(a, "--parse-sweep")) { o->parse_sweep = true; continue; }
		if (!strcmp(a, "--parse-sweep-table")) { o->parse_sweep_table = true; continue; }
		if (!strcmp(a, "--cost-report")) { o->cost_report = true; continue; }
		if (!v) return refuse(o, NULL);
		if (!strcmp(a, "--neighbours")) o->cfg.neighbours_per_step = (uint32_t)strtoul(v, NULL, 0);
		else if (!strcmp(a, "--epochs")) o->epochs = (unsigned)strtoul(v, NULL, 0);
		else if (!strcmp(a, "--phases")) o->phases = (unsigned)strtoul(v, NULL, 0);
		else if (!strcmp(a, "--steps")) o->steps = strtoull(v, NULL, 0);
		else if (!strcmp(a, "--seed")) o->cfg.seed = strtoull(v, NULL, 0);
		else if (!strcmp(a, "--lc")) { o->props.lc = (uint8_t)strtoul(v, NULL, 0); o->props_given = true; }
		else if (!strcmp(a, "--lp")) { o->props.lp = (uint8_t)strtoul(v, NULL, 0); o->props_given = true; }
		else if (!strcmp(a, "--pb")) { o->props.pb = (uint8_t)strtoul(v, NULL, 0); o->props_given = true; }
		else if (!strcmp(a, "--props")) { bad = strcmp(v, "auto") != 0; o->props_auto = true; }
		else if (!strcmp(a, "--props-rounds")) bad = !count_in(v, 1, UINT32_MAX, &o->props_rounds);
		else if (!strcmp(a, "--props-joint")) bad = !count_in(v, 1, JOINT_MAX, &o->props_joint);
		else if (!strcmp(a, "--device")) { o->cfg.device = (int32_t)strtol(v, NULL, 0); o->device_given = true; }
		else if (!strcmp(a, "--max-scan")) o->cfg.max_bucket_scan = (uint32_t)strtoul(v, NULL, 0);
		else if (!strcmp(a, "--format")) { bad = (w = word(v, "lzma", "xz", NULL)) < 0; o->format_xz = w == 1; }
		else if (!strcmp(a, "--filter")) { bad = (w = word(v, "none", "x86", "auto")) < 0; o->filter = w; o->filter_given = true; }
		else if (!strcmp(a, "--dict-size")) {
			if (!number(v, &n) || (n && n < 4096) || n > 0xFFFFFFFFull) why = "--dict-size takes a number of bytes from 4096 to 4294967295 (0 = 4 MiB)";
			o->dict_size = (uint32_t)n;
		}
		else if (!strcmp(a, "-o")) o->out_path = v;
		else if (!strcmp(a, "--save-slab")) o->save_path = v;
		else if (!strcmp(a, "--load-slab")) o->load_path = v;
		else if (!strcmp(a, "--greedy-seed")) o->greedy = (uint32_t)strtoul(v, NULL, 0);
		else if (!strcmp(a, "--optimal-seed")) bad = !count_in(v, 1, UINT32_MAX, &o->optimal);
		else if (!strcmp(a, "--adaptive-seed")) bad = !count_in(v, 1, UINT32_MAX, &o->adaptive);
		else if (!strcmp(a, "--match-finder")) { bad = (w = word(v, "nearest", "frontier", NULL)) < 0; o->finder = w == 1 ? MGL_MF_FRONTIER : MGL_MF_NEAREST; o->finder_given = true; }
		else if (!strcmp(a, "--mf-depth")) bad = !count_in(v, 1, 4096, &o->mf_depth);
		else if (!strcmp(a, "--seed-stream")) o->seed_stream_path = v;
		else if (!strcmp(a, "--temperature")) o->temperature_bytes = strtod(v, NULL);
		else if (!strcmp(a, "--accept")) { bad = (w = word(v, "auto", "single", "bulk")) < 0; o->accept_mode = w == 1 ? MGL_ACCEPT_SINGLE : w == 2 ? MGL_ACCEPT_BULK : MGL_ACCEPT_AUTO; }
		else if (!strcmp(a, "--chains")) o->chains = (int)strtol(v, NULL, 0);
		else if (!strcmp(a, "--rank")) o->rank = (int)strtol(v, NULL, 0);
		else if (!strcmp(a, "--comm-file")) o->comm_path = v;
		else if (!strcmp(a, "--comm-nonce")) o->comm_nonce = strtoull(v, NULL, 0);
		else if (!strcmp(a, "--transport")) { bad = (w = word(v, "rccl", "shm", NULL)) < 0; if (w == 1) o->transport_shm = true; } /* rccl, the default, does not undo an earlier shm */
		else if (!strcmp(a, "--exchange")) { bad = (w = word(v, "best", "cross", "cross-all")) < 0; o->exchange = w; }
		else if (!strcmp(a, "--cross-grain")) { o->cross_grain = (uint32_t)strtoul(v, NULL, 0); o->cross_grain_given = true; }
		else if (!strcmp(a, "--focus")) why = parse_focus(v, o);
		else if (!strcmp(a, "--target-weights")) why = parse_target_weights(v, o);
		else if (!strcmp(a, "--live-weights")) why = parse_live_weights(v, o);
		else if (!strcmp(a, "--cost-map")) o->cost_map_path = v;
		else if (!strcmp(a, "--segment-props")) {
			o->segment_props = true;
			o->segment_grain = 0;
			if (strcmp(v, "auto") != 0 && (v[0] < '0' || v[0] > '9' || !number(v, &o->segment_grain) || !o->segment_grain))
				why = "--segment-props takes a number of bytes, at least 1, or auto";
		}
		else if (!strcmp(a, "--segment-reparse")) {
			o->segment_reparse_given = true;
			if (v[0] < '0' || v[0] > '9' || !count_in(v, 1, MGL_OPT_MAX_PASSES, &o->segment_reparse)) why = "--segment-reparse takes a number of passes from 1 to 16";
		}
		else if (!strcmp(a, "--cost-bucket")) { if (!number(v, &o->cost_bucket) || !o->cost_bucket) why = "--cost-bucket takes a number of bytes, at least 1"; }
		else bad = true;
		if (bad || why) return refuse(o, why);
		i++;
	}
	return 0;
}

/* What cannot be combined, in this order: a command line that breaks two rules gets the first one's answer.  Nothing has
 * been opened and no device looked for yet.  Then the values derived from more than one option. */
static int check_args(cli_opts* o)
{
	const bool from_file = o->seed_stream_path || o->load_path; /* the starting parse is read, not made */
	if (!o->filename) return refuse(o, NULL);
	if (o->seed_stream_path && (o->load_path || o->greedy)) return refuse(o, "--seed-stream cannot be combined with --load-slab or --greedy-seed");
	if (o->optimal && (o->greedy || from_file)) return refuse(o, "--optimal-seed cannot be combined with --greedy-seed, --seed-stream or --load-slab");
	if (o->adaptive && (o->optimal || o->greedy || from_file))
		return refuse(o, "--adaptive-seed cannot be combined with --optimal-seed, --greedy-seed, --seed-stream or --load-slab");
	if ((o->finder_given || o->mf_depth) && !(o->optimal || o->adaptive || o->props_auto || o->segment_reparse_given))
		return refuse(o, "--match-finder / --mf-depth need --optimal-seed, --adaptive-seed or --props auto");
	if ((o->parse_sweep && !o->adaptive) || (o->parse_sweep_table && !o->parse_sweep)) return refuse(o, NULL);
	if (o->parse_sweep && o->finder_given) return refuse(o, "--parse-sweep runs both match finders; --match-finder cannot be combined with it");
	if (o->mf_depth && o->finder != MGL_MF_FRONTIER && !o->parse_sweep) return refuse(o, NULL);
	if (o->clip_window && !o->seed_stream_path) return refuse(o, NULL);
	if (o->props_auto && (o->props_given || o->chains > 1)) return refuse(o, "--props auto cannot be combined with --lc/--lp/--pb or with --chains above 1");
	if (o->props_table && !o->props_auto) return refuse(o, NULL);
	if (o->props_joint && !(o->props_auto && o->adaptive && o->parse_sweep)) return refuse(o, "--props-joint needs --props auto --adaptive-seed P --parse-sweep");
	if (o->cross_grain_given && o->exchange == EXCHANGE_BEST) return refuse(o, "--cross-grain needs --exchange cross or --exchange cross-all");
	if (o->filter != FILTER_NONE && !o->format_xz) return refuse(o, "--filter x86 / auto need --format xz: an .lzma stream has no place to declare a filter");
	if (o->filter == FILTER_AUTO && (from_file || o->chains > 1)) return refuse(o, "--filter auto cannot be combined with --seed-stream, --load-slab or --chains above 1");
	if (o->segment_props && !o->format_xz) return refuse(o, "--segment-props needs --format xz: an .lzma stream cannot reset its state or change lc/lp/pb");
	if (o->segment_props && (o->cost_map_path || o->cost_report || o->cost_bucket))
		return refuse(o, "--segment-props cannot be combined with --cost-map, --cost-report or --cost-bucket: they describe a stream under one triple");
	if (o->segment_reparse_given && !o->segment_props) return refuse(o, "--segment-reparse needs --segment-props: it parses the segments that option chooses");
	if (o->focus_rank && o->chains < 2) return refuse(o, "--focus rank needs --chains N with N at least 2");
	if (o->live_given && o->weights != WEIGHTS_NONE) return refuse(o, "--live-weights and --target-weights exclude each other");
	if (o->chains < 1 || o->rank < 0 || o->rank >= o->chains || (o->chains > 1 && !o->comm_path)) return refuse(o, NULL);

	o->seed = (seed_spec){ o->adaptive ? o->adaptive : o->optimal, o->adaptive != 0, o->finder, o->mf_depth, o->parse_sweep, o->parse_sweep_table };
	o->cfg.dict_limit = o->dict_size; /* 0: the library's 4 MiB */
	if (o->chains > 1) {
		if (!o->device_given) o->cfg.device = o->rank;
		/* distinct, reproducible RNG stream per chain (the same rule as megalania_amd/multi_gpu.py:chain_seed) */
		if (o->rank) o->cfg.seed ^= 0x9E3779B97F4A7C15ull * (uint64_t)(o->rank + 1);
	}
	return 0;
}

/* ---- the run's context and its helpers ---- */

typedef struct {
	const cli_opts* o;
	mgl_sa_config cfg;
	mgl_properties props; /* the given ones, then the seed stream's, then --props auto's */
	int filter;           /* the given one, then the seed stream's, then --filter auto's */
	/* orig_data: the file.  file_data: what the LZMA layer sees, the file itself or (--filter x86) its filtered copy; the
	 * handle, the seeds, the slabs and the chains all work on file_data, and only the .xz writer looks at both */
	int fd;
	const uint8_t *orig_data, *file_data;
	uint8_t* filtered;
	size_t file_size;
	mgl_sa* sa;
	mgl_comm* comm;
	/* the parse that the phase 0 epochs start from under --optimal-seed / --adaptive-seed; filled by whichever stage made
	 * it first: --filter auto, --props auto or the run's seed */
	mgl_packet* seed_slab;
	bool seed_filled;
	mgl_packet* packets_best;
	bool resumed; /* a best slab was loaded: every epoch starts from it */
	uint8_t* seed_stream;
	size_t seed_stream_len;
	/* --segment-props: the segments the stream is written in */
	mgl_segment segs[MGL_SEG_MAX_CUTS];
	size_t nseg;
} cli_run;

/* every error of the run: one `Error:` line on stderr, exit status 255; nothing is freed on the way out */
__attribute__((format(printf, 1, 2))) static int fail(const char* fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	fprintf(stderr, "Error: ");
	vfprintf(stderr, fmt, ap);
	fprintf(stderr, "\n");
	va_end(ap);
	return -1;
}

static int lib_error(void) { return fail("%s", mgl_last_error()); }

static mgl_packet* alloc_slab(const cli_run* r)
{
	mgl_packet* p = (mgl_packet*)malloc(sizeof(mgl_packet) * r->file_size);
	if (!p) fail("out of memory");
	return p;
}

/* Estimated bytes of a cost.  The three arithmetic types are those of the lines they are printed in: the digits depend
 * on them.  main.c:97-99: 18 = 13 header bytes + 5 flush bytes, 16384 = 2048 * 8 */
static float bytes_f(uint64_t cost) { return 18 + cost / 16384.f; }
static double bytes_d(uint64_t cost) { return 18 + cost / 16384.0; }
static unsigned long long bytes_up(uint64_t cost) { return (cost + 16383) / 16384; }

/* an untouched handle over file_data at the context's props, in place of the one alive (if any) */
static int fresh_handle(cli_run* r)
{
	mgl_sa_destroy(r->sa);
	r->sa = mgl_sa_create(r->file_data, r->file_size, r->props, &r->cfg);
	return r->sa ? 0 : lib_error();
}

static bool same_props(mgl_properties a, mgl_properties b) { return a.lc == b.lc && a.lp == b.lp && a.pb == b.pb; }

/* the cheapest of the 75 triples, ties to the first in canonical order */
static size_t cheapest_triple(const mgl_props_cost* tab)
{
	size_t arg = 0;
	for (size_t t = 1; t < MGL_PROPS_TRIPLES; t++)
		if (tab[t].cost < tab[arg].cost) arg = t;
	return arg;
}

static void print_props_table(const mgl_props_cost* tab)
{
	for (size_t t = 0; t < MGL_PROPS_TRIPLES; t++)
		fprintf(stderr, "props-table: lc=%u lp=%u pb=%u cost %llu (%llu B)\n", tab[t].props.lc, tab[t].props.lp, tab[t].props.pb,
		        (unsigned long long)tab[t].cost, bytes_up(tab[t].cost));
}

static const char* finder_name(uint32_t finder) { return finder == MGL_MF_FRONTIER ? "frontier" : "nearest"; }

/* --parse-sweep's grid (mirrored by binding.DEFAULT_SWEEP): index 0 is the library's default, which therefore holds a tie */
#define SWEEP_GRID 16
static const mgl_parse_variant sweep_grid[SWEEP_GRID] = {
	{ MGL_MF_NEAREST, 16, 64, 128 },   { MGL_MF_NEAREST, 16, 64, 273 },   { MGL_MF_NEAREST, 16, 32, 128 },   { MGL_MF_NEAREST, 16, 32, 273 },
	{ MGL_MF_NEAREST, 16, 128, 128 },  { MGL_MF_NEAREST, 16, 128, 273 },  { MGL_MF_NEAREST, 16, 256, 128 },  { MGL_MF_NEAREST, 16, 256, 273 },
	{ MGL_MF_FRONTIER, 16, 64, 128 },  { MGL_MF_FRONTIER, 16, 64, 273 },  { MGL_MF_FRONTIER, 16, 32, 128 },  { MGL_MF_FRONTIER, 16, 32, 273 },
	{ MGL_MF_FRONTIER, 16, 128, 128 }, { MGL_MF_FRONTIER, 16, 128, 273 }, { MGL_MF_FRONTIER, 16, 256, 128 }, { MGL_MF_FRONTIER, 16, 256, 273 },
};

/* --parse-sweep-table: the grid's per-pass sizes; pr (nullable): the triple the rows were made under; star: the winner */
static void print_sweep_rows(const mgl_properties* pr, const mgl_optimal_stats* res, uint32_t star)
{
	for (uint32_t g = 0; g < SWEEP_GRID; g++) {
		fprintf(stderr, "parse-sweep-table:");
		if (pr) fprintf(stderr, " lc=%u lp=%u pb=%u", pr->lc, pr->lp, pr->pb);
		fprintf(stderr, " %s cand %u segment %u ahead %u:", finder_name(sweep_grid[g].finder), sweep_grid[g].cand, sweep_grid[g].segment, sweep_grid[g].ahead);
		for (uint32_t p = 0; p < res[g].passes; p++) fprintf(stderr, " %.1f", bytes_d(res[g].cost[p]));
		fprintf(stderr, " B%s\n", g == star ? " *" : "");
	}
}

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
	if (!ok) fail("%s is not a slab for this input", path);
	return ok;
}

/* through <path>.tmp and a rename: a reader never sees half a file */
static bool write_slab_file(const char* path, size_t file_size, const mgl_packet* packets, uint64_t perplexity)
{
	const uint64_t hdr[2] = { file_size, perplexity };
	char tmp[4200];
	snprintf(tmp, sizeof tmp, "%s.tmp", path);
	FILE* f = fopen(tmp, "wb");
	return f && fwrite("MGLSLAB1", 8, 1, f) == 1 && fwrite(hdr, 8, 2, f) == 2 && fwrite(packets, sizeof(mgl_packet), file_size, f) == file_size &&
	       fclose(f) == 0 && rename(tmp, path) == 0;
}

/* the seed stream's parse, re-expressed for one LZMA1 stream, into `out`; hint: the error line names --clip-window where it would help */
static int import_seed_stream(const cli_run* r, mgl_packet* out, bool hint, mgl_import_stats* ist)
{
	const uint32_t flags = (r->o->clip_window ? MGL_IMPORT_CLIP_WINDOW : 0) | (r->filter == FILTER_X86 ? MGL_IMPORT_X86 : 0);
	const int rc = mgl_stream_import(r->seed_stream, r->seed_stream_len, r->file_data, r->file_size, r->cfg.dict_limit, flags, out, ist);
	if (rc == MGL_OK) return 0;
	return fail("%s: %s at input position %llu%s", r->o->seed_stream_path, ist->error ? ist->error : "import failed", (unsigned long long)ist->error_pos,
	            hint && rc == MGL_ERANGE ? " (--clip-window turns such copies into literals)" : "");
}

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
	if (seed.sweep_table) print_sweep_rows(NULL, res, best);
	fprintf(stderr, "parse sweep: variant %u (%s, cand %u, segment %u, ahead %u), pass %u, %.1f B; %u variants in %.1f ms\n", best,
	        finder_name(sweep_grid[best].finder), sweep_grid[best].cand, sweep_grid[best].segment, sweep_grid[best].ahead, res[best].best_pass,
	        bytes_d(res[best].cost[res[best].best_pass]), SWEEP_GRID, ms);
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

/* --filter auto: the seed whose exact cost decides.  Greedy parse, the optimal / adaptive seed of the run, or an optimal
 * parse at the library's defaults where the run has no seed option. */
static int make_filter_seed(cli_run* r, mgl_packet* parse, uint64_t* cost)
{
	mgl_optimal_stats os;
	int rc;
	if (r->o->greedy) rc = mgl_sa_seed_greedy(r->sa, r->o->greedy);
	else if (r->o->seed.passes) rc = make_seed(r->sa, r->o->seed, &os);
	else {
		mgl_optimal_config oc = { 0, 0, 0 };
		rc = mgl_sa_seed_optimal(r->sa, &oc, &os);
	}
	return rc != MGL_OK ? rc : mgl_sa_current(r->sa, parse, cost);
}

/* ---- the stages: 0, or the exit status after the error has been reported ---- */

/* an empty input leaves file_size 0 and nothing mapped */
static int map_input(cli_run* r)
{
	const char* name = r->o->filename;
	struct stat sb;
	if ((r->fd = open(name, O_RDONLY)) < 0) return fail("could not open %s", name);
	if (fstat(r->fd, &sb) < 0) return fail("could not stat %s", name);
	r->cfg.iters_per_epoch = r->file_size = (size_t)sb.st_size;
	if (r->file_size == 0) { close(r->fd); return 0; }
	r->orig_data = r->file_data = (const uint8_t*)mmap(NULL, r->file_size, PROT_READ, MAP_PRIVATE, r->fd, 0);
	return r->orig_data == MAP_FAILED ? fail("could not map %s", name) : 0;
}

static int find_device(void) { return mgl_device_count() < 1 ? fail("no HIP device found; this program has no CPU search path") : 0; }

/* --seed-stream: the stream's properties unless --lc/--lp/--pb say otherwise (a parse is valid under any), and its filter */
static int read_seed_stream_header(cli_run* r)
{
	const cli_opts* o = r->o;
	const char* path = o->seed_stream_path;
	if (!path) return 0;
	FILE* f = fopen(path, "rb");
	long sz = -1;
	if (f && fseek(f, 0, SEEK_END) == 0) sz = ftell(f);
	if (sz > 0 && fseek(f, 0, SEEK_SET) == 0 && (r->seed_stream = (uint8_t*)malloc((size_t)sz)) != NULL && fread(r->seed_stream, 1, (size_t)sz, f) == (size_t)sz)
		r->seed_stream_len = (size_t)sz;
	if (f) fclose(f);
	mgl_stream_info info;
	uint32_t stream_filter = 0;
	if (!r->seed_stream_len || mgl_stream_info_read_x(r->seed_stream, r->seed_stream_len, &info, &stream_filter) != MGL_OK)
		return fail("%s is not an LZMA-alone or .xz stream", path);
	if (stream_filter == 4) {
		if (!o->format_xz) return fail("%s declares the x86 BCJ filter, which an .lzma stream cannot declare: use --format xz", path);
		if (o->filter_given && o->filter == FILTER_NONE)
			return fail("%s declares the x86 BCJ filter, so its parse is one of the filtered input: not with --filter none", path);
		r->filter = FILTER_X86;
	}
	if (!o->props_given) r->props = info.props;
	else if (!same_props(r->props, info.props))
		fprintf(stderr, "note: %s was coded with lc/lp/pb %u/%u/%u; searching with the given %u/%u/%u\n", path, info.props.lc, info.props.lp,
		        info.props.pb, r->props.lc, r->props.lp, r->props.pb);
	return 0;
}

static int make_filtered_copy(cli_run* r)
{
	if (r->filter == FILTER_NONE) return 0;
	if ((r->filtered = (uint8_t*)malloc(r->file_size)) == NULL) return fail("out of memory");
	memcpy(r->filtered, r->orig_data, r->file_size);
	mgl_bcj_x86(r->filtered, r->file_size, 1);
	if (r->filter == FILTER_X86) r->file_data = r->filtered;
	return 0;
}

/* --filter auto: the same seed over the plain bytes (on the handle alive) and over the filtered ones, one handle after the
 * other; the cheaper exact cost wins and a tie goes to none.  Where the filter changes no byte the two parses are the same one. */
static int choose_filter(cli_run* r)
{
	const cli_opts* o = r->o;
	if (r->filter != FILTER_AUTO) return 0;
	mgl_packet* parse[2] = { alloc_slab(r), alloc_slab(r) };
	uint64_t cost[2] = { 0, 0 };
	if (!parse[0] || !parse[1]) return -1;
	if (make_filter_seed(r, parse[0], &cost[0]) != MGL_OK) return lib_error();
	const bool changed = memcmp(r->filtered, r->orig_data, r->file_size) != 0;
	cost[1] = cost[0];
	if (changed) {
		r->file_data = r->filtered;
		if (fresh_handle(r)) return -1;
		if (make_filter_seed(r, parse[1], &cost[1]) != MGL_OK) return lib_error();
	}
	const int win = cost[1] < cost[0];
	fprintf(stderr, "filter auto: none %llu x86 %llu -> %s (exact costs %llu %llu)\n", bytes_up(cost[0]), bytes_up(cost[1]), win ? "x86" : "none",
	        (unsigned long long)cost[0], (unsigned long long)cost[1]);
	r->filter = win ? FILTER_X86 : FILTER_NONE;
	r->file_data = win ? r->filtered : r->orig_data;
	/* the handle alive is the filtered bytes' when they were looked at; --props auto wants an untouched one */
	if ((changed ? (!win || o->props_auto) : o->props_auto) && fresh_handle(r)) return -1;
	if (o->seed.passes && !o->props_auto) { r->seed_slab = parse[win]; r->seed_filled = true; }
	else free(parse[win]);
	free(parse[!win]);
	return 0;
}

/* --props auto.  The handle is one at r->props that nothing has been done to yet.  Each round costs
 * one parse under all 75 triples (mgl_props_sweep) and moves to a fresh handle at the cheapest, until that is the
 * handle's own or --props-rounds sweeps are done.  parse_fixed: `parse` holds a parse that does not depend on the triple (a
 * stream's, a loaded slab's, the greedy one); otherwise every round makes the run's seed under the handle's triple
 * into it.  Of all (triple, parse) pairs seen the cheapest wins: r->props becomes its triple, the seed slab its parse (only
 * when the parse is not fixed), and the handle left is an untouched one at that triple. */
static int choose_props(cli_run* r, mgl_packet* parse, bool parse_fixed)
{
	mgl_props_cost tab[MGL_PROPS_TRIPLES];
	uint64_t best_cost = UINT64_MAX, best_at0 = 0;
	mgl_properties best = r->props;
	unsigned done = 0;
	bool touched = false;
	for (;;) {
		if (!parse_fixed) {
			mgl_optimal_stats os;
			uint64_t cost = 0;
			if (make_seed(r->sa, r->o->seed, &os) != MGL_OK || mgl_sa_current(r->sa, parse, &cost) != MGL_OK) return lib_error();
			touched = true;
		}
		size_t count = 0;
		if (mgl_props_sweep(r->sa, parse, tab, MGL_PROPS_TRIPLES, &count, NULL) != MGL_OK) return lib_error();
		done++;
		const size_t arg = cheapest_triple(tab);
		if (tab[arg].cost < best_cost) {
			best_cost = tab[arg].cost; best = tab[arg].props; best_at0 = tab[0].cost;
			if (!parse_fixed) memcpy(r->seed_slab, parse, sizeof(mgl_packet) * r->file_size);
		}
		if (same_props(tab[arg].props, r->props) || done >= r->o->props_rounds) break;
		r->props = tab[arg].props;
		touched = false;
		if (fresh_handle(r)) return -1;
	}
	if (touched || !same_props(best, r->props)) {
		r->props = best;
		if (fresh_handle(r)) return -1;
	}
	fprintf(stderr, "props: lc=%u lp=%u pb=%u, sweep %llu B, at 0/0/0 %llu B, %u rounds\n", best.lc, best.lp, best.pb, bytes_up(best_cost),
	        bytes_up(best_at0), done);
	if (r->o->props_table) print_props_table(tab);
	return 0;
}

/* --props-joint T.  The handle is an untouched one at r->props = 0/0/0.  Stage A: the grid at 0/0/0
 * (parse W_A, cost c_A).  W_A is costed under all 75 triples; t* is the cheapest, the candidates C the T cheapest other than
 * 0/0/0.  Stage B: one batch of 16 x T variants, grid entry g under C[k] at 16 k + g (parse W_B at cost c_B under C[k_B]).
 * The cheapest of (0/0/0, W_A, c_A), (t*, W_A, table[t*]), (C[k_B], W_B, c_B) wins, ties in this order; the seed slab receives
 * its parse and r->props its triple.  Leaves a handle at that triple on which the parse costs what the pair said. */
static int choose_props_joint(cli_run* r)
{
	static mgl_optimal_stats res_a[SWEEP_GRID], res_b[SWEEP_GRID * JOINT_MAX];
	mgl_parse_variant var_b[SWEEP_GRID * JOINT_MAX];
	mgl_properties pr_a[SWEEP_GRID], pr_b[SWEEP_GRID * JOINT_MAX], cand[JOINT_MAX];
	mgl_props_cost tab[MGL_PROPS_TRIPLES];
	const seed_spec seed = r->o->seed;
	const unsigned T = r->o->props_joint;
	const mgl_parse_sweep_config sc = { seed.passes, 0, seed.mf_depth, 0 };
	const mgl_properties s0 = r->props;
	mgl_packet* const kept = r->seed_slab;
	mgl_packet* w_b = alloc_slab(r);
	uint32_t best_a = 0, best_b = 0;
	double ms_a = 0, ms_b = 0;
	size_t count = 0;
	if (!w_b) return -1;
	for (uint32_t g = 0; g < SWEEP_GRID; g++) pr_a[g] = s0;
	if (mgl_parse_sweep_props(r->sa, &sc, sweep_grid, pr_a, SWEEP_GRID, res_a, &best_a, kept, &ms_a) != MGL_OK) return lib_error();
	if (best_a >= SWEEP_GRID) return fail("the parse sweep named no variant");
	const uint64_t c_a = res_a[best_a].cost[res_a[best_a].best_pass];
	if (mgl_props_sweep(r->sa, kept, tab, MGL_PROPS_TRIPLES, &count, NULL) != MGL_OK) return lib_error();
	const size_t t_star = cheapest_triple(tab);
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
	if (mgl_parse_sweep_props(r->sa, &sc, var_b, pr_b, (size_t)SWEEP_GRID * T, res_b, &best_b, w_b, &ms_b) != MGL_OK) return lib_error();
	if (best_b >= SWEEP_GRID * T) return fail("the parse sweep named no variant");
	const uint64_t c_b = res_b[best_b].cost[res_b[best_b].best_pass];
	/* the decision */
	const char* stage = "A";
	mgl_properties win = s0;
	uint64_t cost = c_a;
	uint32_t variant = best_a, pass = res_a[best_a].best_pass;
	if (tab[t_star].cost < cost) { stage = "A-recosted"; win = tab[t_star].props; cost = tab[t_star].cost; }
	const bool from_b = c_b < cost;
	if (from_b) {
		stage = "B"; win = pr_b[best_b]; cost = c_b; variant = best_b % SWEEP_GRID; pass = res_b[best_b].best_pass;
		memcpy(kept, w_b, sizeof(mgl_packet) * r->file_size);
	}
	free(w_b);
	if (!same_props(win, s0)) {
		r->props = win;
		if (fresh_handle(r)) return -1;
	}
	uint64_t check = 0;
	if (mgl_sa_set_slab(r->sa, kept) != MGL_OK || mgl_sa_current(r->sa, NULL, &check) != MGL_OK) return lib_error();
	if (check != cost) return fail("the joint choice's parse costs %llu on a handle at its triple, not %llu", (unsigned long long)check, (unsigned long long)cost);
	fprintf(stderr, "props: lc=%u lp=%u pb=%u, sweep %llu B, at 0/0/0 %llu B, joint with %u candidates in %.1f + %.1f ms\n", win.lc, win.lp, win.pb,
	        bytes_up(cost), bytes_up(c_a), T, ms_a, ms_b);
	fprintf(stderr, "props joint: lc=%u lp=%u pb=%u stage %s variant %u pass %u cost %llu; stage A cost %llu; candidates", win.lc, win.lp, win.pb, stage,
	        variant, pass, (unsigned long long)cost, (unsigned long long)c_a);
	for (unsigned k = 0; k < T; k++) fprintf(stderr, " %u/%u/%u", cand[k].lc, cand[k].lp, cand[k].pb);
	fprintf(stderr, "\n");
	if (seed.sweep_table) {
		print_sweep_rows(&s0, res_a, from_b ? SWEEP_GRID : best_a);
		for (unsigned k = 0; k < T; k++) print_sweep_rows(&cand[k], res_b + SWEEP_GRID * k, from_b && best_b / SWEEP_GRID == k ? variant : SWEEP_GRID);
	}
	if (r->o->props_table) print_props_table(tab);
	return 0;
}

/* --props auto: the parse to look at is the seed the user asked for; without one an optimal seed at its defaults, for the
 * sweep only, and the search starts from the all-literal slab */
static int auto_props(cli_run* r)
{
	const cli_opts* o = r->o;
	if (!o->props_auto) return 0;
	mgl_packet* parse = alloc_slab(r);
	mgl_import_stats ist;
	bool fixed = true;
	uint64_t unused = 0;
	if (!parse) return -1;
	if (r->seed_stream) {
		if (import_seed_stream(r, parse, false, &ist)) return -1;
	} else if (o->load_path) {
		if (!read_slab_file(o->load_path, r->file_size, parse, &unused)) return -1;
	} else if (o->greedy) {
		/* the greedy parse does not look at the properties: made once, on a handle that is then replaced */
		if (mgl_sa_seed_greedy(r->sa, o->greedy) != MGL_OK || mgl_sa_current(r->sa, parse, &unused) != MGL_OK) return lib_error();
		if (fresh_handle(r)) return -1;
	} else {
		fixed = false;
		if ((r->seed_slab = alloc_slab(r)) == NULL) return -1;
	}
	if (o->props_joint ? choose_props_joint(r) : choose_props(r, parse, fixed)) return -1;
	free(parse);
	r->seed_filled = o->seed.passes != 0;
	if (!r->seed_filled) { free(r->seed_slab); r->seed_slab = NULL; }
	return 0;
}

/* --temperature B, in the cost's units */
static int set_temperature(cli_run* r)
{
	const double b = r->o->temperature_bytes;
	return b > 0 && mgl_sa_set_temperature(r->sa, (uint64_t)(b * 16384.0)) != MGL_OK ? lib_error() : 0;
}

/* The RCCL id through the rendezvous file: "MGLCOMM1", u64 nonce, the 128-byte id.  Rank 0 replaces whatever an earlier
 * run left under the name; the others only take a file of this run. */
static int rendezvous(const cli_opts* o, uint8_t uid[128])
{
	if (o->rank == 0) {
		char tmp[4096];
		snprintf(tmp, sizeof tmp, "%s.tmp", o->comm_path);
		(void)unlink(o->comm_path);
		FILE* f = fopen(tmp, "wb");
		const uint64_t nonce = o->comm_nonce;
		if (mgl_comm_unique_id(uid) == MGL_OK && f && fwrite("MGLCOMM1", 8, 1, f) == 1 && fwrite(&nonce, 8, 1, f) == 1 && fwrite(uid, 128, 1, f) == 1 &&
		    fclose(f) == 0 && rename(tmp, o->comm_path) == 0) return 0;
		return fail("could not publish the communicator id in %s: %s", o->comm_path, mgl_last_error());
	}
	const char* te = getenv("MGL_COMM_TIMEOUT_S");
	const double limit = te && atof(te) > 0 ? atof(te) : 600.0;
	for (double waited = 0; waited < limit; waited += 0.1) {
		FILE* f = fopen(o->comm_path, "rb");
		char magic[8];
		uint64_t nonce = 0;
		const bool got = f && fread(magic, 8, 1, f) == 1 && !memcmp(magic, "MGLCOMM1", 8) && fread(&nonce, 8, 1, f) == 1 && nonce == o->comm_nonce &&
		                 fread(uid, 128, 1, f) == 1;
		if (f) fclose(f);
		if (got) return 0;
		usleep(100000);
	}
	return fail("no communicator id of this run (--comm-nonce %llu) appeared in %s", o->comm_nonce, o->comm_path);
}

/* --comm-file, also with --chains 1: the same code path on a one-GPU box */
static int open_comm(cli_run* r)
{
	const cli_opts* o = r->o;
	uint8_t uid[128];
	if (!o->comm_path) return 0;
	if (o->transport_shm) return mgl_comm_init_shm(&r->comm, o->comm_path, o->comm_nonce, o->rank, o->chains, r->cfg.device) != MGL_OK ? lib_error() : 0;
	if (rendezvous(o, uid)) return -1;
	if (mgl_comm_init(&r->comm, uid, o->rank, o->chains, r->cfg.device) != MGL_OK) return lib_error();
	if (o->rank == 0) (void)unlink(o->comm_path); /* ncclCommInitRank returns once every rank has joined: nobody reads the file any more */
	return 0;
}

static int set_accept_mode(cli_run* r) { return mgl_sa_set_accept_mode(r->sa, (int)r->o->accept_mode, 0) != MGL_OK ? lib_error() : 0; }

static int load_slab(cli_run* r)
{
	uint64_t perplexity = 0;
	if (!r->o->load_path) return 0;
	if (!read_slab_file(r->o->load_path, r->file_size, r->packets_best, &perplexity)) return -1;
	/* --props auto: the file's perplexity belongs to the triple it was saved under; the slab is costed under the chosen one */
	if (r->o->props_auto && mgl_cost_slab(r->sa, r->packets_best, &perplexity, NULL, NULL) != MGL_OK) return lib_error();
	/* the library re-costs the slab and refuses it unless the perplexity matches */
	if (mgl_sa_set_best(r->sa, r->packets_best, perplexity) != MGL_OK) return lib_error();
	r->resumed = true;
	return 0;
}

/* the stream's parse becomes the best slab (re-costed and checked by the library like a --load-slab one); every epoch then
 * starts from the best slab */
static int seed_stream_as_best(cli_run* r)
{
	mgl_import_stats ist;
	uint64_t cost = 0;
	size_t npk = 0;
	if (!r->seed_stream) return 0;
	if (import_seed_stream(r, r->packets_best, true, &ist)) return -1;
	if (mgl_cost_slab(r->sa, r->packets_best, &cost, NULL, &npk) != MGL_OK || mgl_sa_set_best(r->sa, r->packets_best, cost) != MGL_OK) return lib_error();
	fprintf(stderr, "seed stream: %zu packets, estimate %f bytes, stream %zu bytes, %llu re-expressed, %llu clipped\n", npk, bytes_f(cost),
	        r->seed_stream_len, (unsigned long long)ist.reexpressed, (unsigned long long)ist.clipped);
	free(r->seed_stream);
	r->resumed = true;
	return 0;
}

/* --optimal-seed / --adaptive-seed, unless an earlier stage kept its parse already: made once; every epoch that would start
 * from the all-literal slab starts from it */
static int make_run_seed(cli_run* r)
{
	const seed_spec seed = r->o->seed;
	mgl_optimal_stats os;
	uint64_t cost = 0;
	double ms = 0;
	char mf[96] = "nearest";
	if (!seed.passes || r->seed_filled) return 0;
	if ((r->seed_slab = alloc_slab(r)) == NULL) return -1;
	if (make_seed(r->sa, seed, &os) != MGL_OK || mgl_sa_current(r->sa, r->seed_slab, &cost) != MGL_OK) return lib_error();
	r->seed_filled = true;
	for (uint32_t p = 0; p < os.passes; p++) ms += os.ms[p];
	if (seed.sweep) snprintf(mf, sizeof mf, "chosen by the parse sweep");
	else if (seed.finder == MGL_MF_FRONTIER) {
		/* the lists the seed used are still in the handle: only their count and build time are asked for */
		size_t entries = 0;
		double build_ms = 0;
		if (mgl_match_frontier(r->sa, seed.mf_depth, NULL, NULL, NULL, (size_t)-1, &entries, &build_ms) != MGL_OK) return lib_error();
		snprintf(mf, sizeof mf, "frontier, %zu entries built in %.2f ms", entries, build_ms);
	}
	fprintf(stderr, "%s seed: %u passes in %.1f ms, estimate %f bytes (greedy parse %f), match finder %s\n", seed.adaptive ? "adaptive" : "optimal", os.passes, ms,
	        bytes_f(cost), bytes_f(os.greedy_cost), mf);
	return 0;
}

/* --focus LO:HI holds for the whole run */
static int set_focus(cli_run* r)
{
	const cli_opts* o = r->o;
	return o->focus_given && !o->focus_rank && mgl_sa_set_focus(r->sa, o->focus_lo, o->focus_hi) != MGL_OK ? lib_error() : 0;
}

/* --focus rank: the chain's slice for this round; the rounds count the epochs of the whole run, which the chains share */
static int focus_slice(cli_run* r, uint64_t round)
{
	uint64_t lo = 0, hi = 0;
	if (!r->o->focus_rank) return 0;
	if (mgl_focus_slice(r->file_size, (uint32_t)r->o->chains, (uint32_t)r->o->rank, round, &lo, &hi) != MGL_OK || mgl_sa_set_focus(r->sa, lo, hi) != MGL_OK)
		return lib_error();
	return 0;
}

/* --target-weights file:PATH holds for the whole run: n little-endian u32, what --cost-map writes */
static int load_target_weights(cli_run* r)
{
	const cli_opts* o = r->o;
	const size_t n = r->file_size;
	if (o->weights != WEIGHTS_FILE) return 0;
	FILE* f = fopen(o->weights_path, "rb");
	if (!f) return fail("could not open %s", o->weights_path);
	uint32_t* w = (uint32_t*)malloc(sizeof(uint32_t) * n);
	uint8_t le[4], extra;
	bool ok = w != NULL;
	size_t p = 0;
	for (; ok && p < n && fread(le, 4, 1, f) == 1; p++) w[p] = (uint32_t)le[0] | (uint32_t)le[1] << 8 | (uint32_t)le[2] << 16 | (uint32_t)le[3] << 24;
	const bool fits = ok && p == n && fread(&extra, 1, 1, f) == 0;
	fclose(f);
	if (!w) return fail("out of memory");
	if (!fits) { free(w); return fail("%s does not hold %zu weights of 4 bytes, one per input byte", o->weights_path, n); }
	const int rc = mgl_sa_set_target_weights(r->sa, w);
	free(w);
	return rc != MGL_OK ? lib_error() : 0;
}

/* --target-weights cost: the weights of the epoch that is about to run, from the slab it starts from */
static int weigh_by_cost(cli_run* r)
{
	const cli_opts* o = r->o;
	uint64_t cost = 0, total = 0;
	double ms = 0;
	if (o->weights != WEIGHTS_COST_MEAN && o->weights != WEIGHTS_COST_FLOOR) return 0;
	/* the map's total is the slab's cost, so the mean cost of a byte is known before the map is made */
	if (o->weights == WEIGHTS_COST_MEAN && mgl_sa_current(r->sa, NULL, &cost) != MGL_OK) return lib_error();
	const uint32_t floor = o->weights == WEIGHTS_COST_MEAN ? (uint32_t)(cost / r->file_size) : o->weights_floor;
	if (mgl_sa_weight_targets_by_cost(r->sa, NULL, floor, &total, &ms) != MGL_OK) return lib_error();
	fprintf(stderr, "target-weights: cost map + %u per byte, total %llu, %.2f ms\n", floor, (unsigned long long)total, ms);
	return 0;
}

/* --live-weights: on before the first epoch, for the whole run */
static int enable_live_weights(cli_run* r)
{
	if (!r->o->live_given) return 0;
	return mgl_sa_set_live_weights(r->sa, &r->o->live) != MGL_OK ? lib_error() : 0;
}

/* --live-weights: what the refreshes did up to the end of this epoch's run */
static int report_live_weights(cli_run* r)
{
	mgl_live_weights_stats st;
	char floor[16] = "mean";
	if (!r->o->live_given) return 0;
	if (mgl_sa_live_weights(r->sa, NULL, &st) != MGL_OK) return lib_error();
	if (!r->o->live.floor_mean) snprintf(floor, sizeof floor, "%u", r->o->live.floor);
	fprintf(stderr, "live-weights: every %u steps, floor %s, refreshes %llu, skipped %llu, %.2f ms\n", r->o->live.every, floor,
	        (unsigned long long)st.refreshes, (unsigned long long)st.skipped, st.gpu_ms);
	return 0;
}

/* the plain exchange: every chain adopts the cheapest best slab */
static int exchange_best(cli_run* r)
{
	int winner = -1;
	uint64_t wcost = 0;
	if (mgl_sa_exchange_best(r->sa, r->comm, &winner, &wcost) != MGL_OK) return lib_error();
	fprintf(stderr, "exchange: chain %d holds the best slab, %f bytes\n", winner, bytes_f(wcost));
	return 0;
}

/* what the chains do after an epoch (--exchange), and what came of it */
static int exchange_and_report(cli_run* r)
{
	const cli_opts* o = r->o;
	if (!r->comm || o->exchange == EXCHANGE_BEST) return r->comm ? exchange_best(r) : 0;
	if (o->exchange == EXCHANGE_CROSS) {
		int winner = -1;
		uint64_t wcost = 0;
		mgl_cross_stats xs;
		if (mgl_sa_exchange_cross(r->sa, r->comm, o->cross_grain, &winner, &wcost, &xs) != MGL_OK) return lib_error();
		fprintf(stderr, "exchange: chain %d holds the best slab, %f bytes\n", winner, bytes_f(wcost));
		if (xs.parents)
			fprintf(stderr, "cross: chain %d: own %f, child %f of %llu regions (%llu own), %s (adopted %u), %.2f ms\n", o->rank, bytes_f(xs.parent_cost[0]),
			        bytes_f(xs.child_cost), (unsigned long long)(xs.boundaries - 1), (unsigned long long)xs.regions_from[0],
			        xs.adopted == 2 ? "the child is the new best" : xs.adopted == 1 ? "the winner's slab adopted" : "own best kept", xs.adopted, xs.gpu_ms);
		else
			fprintf(stderr, "cross: chain %d: nothing crossed (adopted %u)\n", o->rank, xs.adopted);
		return 0;
	}
	mgl_cross_all_stats as;
	if (mgl_sa_exchange_cross_all(r->sa, r->comm, o->cross_grain, &as) != MGL_OK) return lib_error();
	char owners[8 * MGL_XO_MAX_PARENTS + 1] = "";
	for (uint32_t p = 0; p < as.distinct; p++) snprintf(owners + strlen(owners), sizeof owners - strlen(owners), p ? " %u" : "%u", as.parent_rank[p]);
	const uint64_t now = as.cross.adopted == 2 ? as.cross.child_cost : as.cross.parent_cost[0];
	if (as.cross.parents)
		fprintf(stderr, "exchange: cross-all: %u distinct of %u best slabs, parents from chains [%s], cheapest %f bytes, child %f bytes of %llu regions, "
		        "adopted %u, best %f bytes, %.2f ms\n", as.distinct, as.chains_with_best, owners, bytes_f(as.cross.parent_cost[0]),
		        bytes_f(as.cross.child_cost), (unsigned long long)(as.cross.boundaries - 1), as.cross.adopted, bytes_f(now), as.cross.gpu_ms);
	else if (as.distinct)
		fprintf(stderr, "exchange: cross-all: %u distinct of %u best slabs, parents from chains [%s], nothing crossed%s, adopted %u, best %f bytes\n",
		        as.distinct, as.chains_with_best, owners, as.fell_back ? " (a chain had no room for the buffers)" : "", as.cross.adopted, bytes_f(now));
	else
		fprintf(stderr, "exchange: cross-all: no chain has a best slab yet, adopted 0\n");
	return 0;
}

/* the crossing exchange leaves every chain its own best slab: one plain exchange, so that rank 0 writes the overall best */
static int final_exchange(cli_run* r) { return r->comm && r->o->exchange == EXCHANGE_CROSS ? exchange_best(r) : 0; }

/* --save-slab, one checkpoint per chain: chain R > 0 writes <file>.rankR (the chains run the same command line) */
static int save_checkpoint(cli_run* r, const mgl_sa_stats* st)
{
	uint64_t perplexity = 0;
	char dst[4096];
	if (!r->o->save_path || st->best_cost == 0) return 0;
	if (mgl_sa_best(r->sa, r->packets_best, &perplexity) != MGL_OK) return lib_error();
	if (r->o->rank) snprintf(dst, sizeof dst, "%s.rank%d", r->o->save_path, r->o->rank);
	else snprintf(dst, sizeof dst, "%s", r->o->save_path);
	if (!write_slab_file(dst, r->file_size, r->packets_best, perplexity)) fprintf(stderr, "warning: could not write %s\n", dst);
	return 0;
}

static int run_epochs(cli_run* r)
{
	const cli_opts* o = r->o;
	const unsigned long long steps = o->steps ? o->steps : (r->file_size + r->cfg.neighbours_per_step - 1) / r->cfg.neighbours_per_step;
	for (unsigned phase = 0; phase < o->phases; phase++) {
		for (unsigned epoch = 0; epoch < o->epochs; epoch++) {
			mgl_sa_stats st;
			if (focus_slice(r, (uint64_t)phase * o->epochs + epoch)) return -1;
			if (mgl_sa_begin_epoch(r->sa, phase, phase != 0 || r->resumed) != MGL_OK) return lib_error();
			if (o->greedy && phase == 0 && !r->resumed && mgl_sa_seed_greedy(r->sa, o->greedy) != MGL_OK) return lib_error();
			if (r->seed_filled && phase == 0 && mgl_sa_set_slab(r->sa, r->seed_slab) != MGL_OK) return lib_error();
			if (weigh_by_cost(r)) return -1;
			if (mgl_sa_run(r->sa, steps, &st) != MGL_OK) return lib_error();
			fprintf(stderr, "current file size: %f\tbest: %f\tstep: %u\tepoch: %04u\t%.0f evals/s\n", bytes_f(st.current_cost), bytes_f(st.best_cost),
			        phase + 1, epoch, st.gpu_ms_total > 0 ? st.evaluations / (st.gpu_ms_total * 1e-3) : 0.0);
			if (report_live_weights(r) || exchange_and_report(r) || save_checkpoint(r, &st)) return -1;
		}
	}
	return 0;
}

static int fetch_best(cli_run* r)
{
	uint64_t best = 0;
	return mgl_sa_best(r->sa, r->packets_best, &best) != MGL_OK ? fail("could not fetch the best slab: %s", mgl_last_error()) : 0;
}

/* --cost-map / --cost-report / --cost-bucket, on rank 0: the slab the run emits, handed to mgl_cost_map explicitly under the
 * run's final triple.  The line formats are fixed (README.md, "Cost map"); costs in bytes are cost / 16384, `exact` is the
 * integer itself. */
static int report_costs(cli_run* r)
{
	static const char* const class_name[MGL_CC_CLASSES] = { "kind", "literal", "length", "rep_length", "distance", "direct" };
	static const char* const type_name[4] = { "literal", "match", "short_rep", "long_rep" };
	const char* map_path = r->o->cost_map_path;
	const unsigned long long bucket = r->o->cost_bucket;
	const size_t n = r->file_size;
	if (r->o->rank != 0 || !(map_path || r->o->cost_report || bucket)) return 0;
	const bool want_map = map_path || bucket;
	uint32_t* map = want_map ? (uint32_t*)malloc(sizeof(uint32_t) * n) : NULL;
	mgl_cost_report c;
	if (want_map && !map) return fail("out of memory");
	if (mgl_cost_map(r->sa, r->packets_best, &r->props, map, &c) != MGL_OK) return lib_error();
	if (map_path) {
		/* n little-endian u32, one per byte the LZMA layer sees */
		FILE* f = fopen(map_path, "wb");
		bool ok = f != NULL;
		for (size_t p = 0; ok && p < n; p++) {
			const uint8_t le[4] = { (uint8_t)map[p], (uint8_t)(map[p] >> 8), (uint8_t)(map[p] >> 16), (uint8_t)(map[p] >> 24) };
			ok = fwrite(le, 4, 1, f) == 1;
		}
		if (f && fclose(f) != 0) ok = false;
		if (!ok) return fail("could not write %s", map_path);
	}
	const double total = c.total ? (double)c.total : 1.0;
	if (r->o->cost_report) {
		fprintf(stderr, "cost-report: total %.3f B exact %llu packets %llu lc=%u lp=%u pb=%u %.3f ms\n", c.total / 16384.0, (unsigned long long)c.total,
		        (unsigned long long)c.packets, r->props.lc, r->props.lp, r->props.pb, c.gpu_ms);
		for (unsigned k = 0; k < MGL_CC_CLASSES; k++)
			fprintf(stderr, "cost-class: %s bits %llu cost %.3f B share %.2f %% exact %llu\n", class_name[k], (unsigned long long)c.class_bits[k],
			        c.class_cost[k] / 16384.0, 100.0 * c.class_cost[k] / total, (unsigned long long)c.class_cost[k]);
		for (unsigned t = 0; t < 4; t++)
			fprintf(stderr, "cost-type: %s packets %llu bytes %llu cost %.3f B share %.2f %% exact %llu\n", type_name[t], (unsigned long long)c.type_packets[t],
			        (unsigned long long)c.type_bytes[t], c.type_cost[t] / 16384.0, 100.0 * c.type_cost[t] / total, (unsigned long long)c.type_cost[t]);
	}
	for (size_t lo = 0, hi = 0; bucket && lo < n; lo = hi) {
		hi = n - lo < bucket ? n : lo + (size_t)bucket;
		uint64_t sum = 0;
		for (size_t p = lo; p < hi; p++) sum += map[p];
		fprintf(stderr, "cost-bucket: offset %zu bytes %zu cost %.3f B bpb %.4f exact %llu\n", lo, hi - lo, sum / 16384.0, sum / 2048.0 / (double)(hi - lo),
		        (unsigned long long)sum);
	}
	free(map);
	return 0;
}

/* --segment-props, on rank 0: the slab the run emits is cut by the grain rule, every span costed under every triple from a
 * state reset, and the cheapest tiling kept for write_stream -- the three calls mgl_sa_segment_props makes, made here one by one
 * because the `single` figure wants the triple of the table's whole-file row, not only its cost.  The handle's own triple plays
 * no part.  Each segment is walked once more on the host, for the count of re-expressed packets and as a check of the device's
 * figure.  The line formats are fixed (README.md, "Segment props"). */
static int choose_segments(cli_run* r)
{
	const cli_opts* o = r->o;
	if (!o->segment_props || o->rank != 0) return 0;
	uint64_t cuts[MGL_SEG_MAX_CUTS], total = 0;
	size_t ncuts = 0, count = 0;
	double ms = 0;
	if (mgl_segment_cuts(r->sa, r->packets_best, o->segment_grain, cuts, MGL_SEG_MAX_CUTS, &ncuts) != MGL_OK) return lib_error();
	const size_t m = ncuts - 1, spans = m * (m + 1) / 2;
	uint64_t* tab = (uint64_t*)malloc(sizeof(uint64_t) * spans * MGL_PROPS_TRIPLES);
	if (!tab) return fail("out of memory");
	if (mgl_props_sweep_spans(r->sa, r->packets_best, cuts, ncuts, tab, spans * MGL_PROPS_TRIPLES, &count, &ms) != MGL_OK ||
	    mgl_segment_partition(tab, ncuts, cuts, MGL_SEG_OVERHEAD, r->segs, &r->nseg, &total) != MGL_OK) return lib_error();
	/* span (0, m) is row m - 1; the triples come in the order lc, lp, pb */
	const uint64_t* whole = tab + (m - 1) * MGL_PROPS_TRIPLES;
	mgl_properties single = { 0, 0, 0 };
	size_t arg = 0, t = 0;
	for (unsigned lc = 0; lc <= 4; lc++)
		for (unsigned lp = 0; lp + lc <= 4; lp++)
			for (unsigned pb = 0; pb <= 4; pb++, t++)
				if (whole[t] < whole[arg] || t == 0) { arg = t; single = (mgl_properties){ (uint8_t)lc, (uint8_t)lp, (uint8_t)pb }; }
	fprintf(stderr, "segment-props: grain %llu cuts %zu spans %zu single lc=%u lp=%u pb=%u %.3f B exact %llu segmented %.3f B exact %llu segments %zu %.3f ms\n",
	        o->segment_grain ? o->segment_grain : 65536ull, ncuts, spans, single.lc, single.lp, single.pb, whole[arg] / 16384.0,
	        (unsigned long long)whole[arg], total / 16384.0, (unsigned long long)total, r->nseg, ms);
	free(tab);
	for (size_t k = 0; k < r->nseg; k++) {
		const mgl_segment* sg = &r->segs[k];
		uint64_t cost = 0, changed = 0;
		if (mgl_host_segment_cost(r->file_data, r->file_size, r->packets_best, sg->lo, sg->hi, sg->props, &cost, &changed) != MGL_OK || cost != sg->cost)
			return fail("segment at %llu: the host walk does not confirm the device's cost %llu", (unsigned long long)sg->lo, (unsigned long long)sg->cost);
		fprintf(stderr, "segment: offset %llu bytes %llu lc=%u lp=%u pb=%u cost %.3f B exact %llu reexpressed %llu\n", (unsigned long long)sg->lo,
		        (unsigned long long)(sg->hi - sg->lo), sg->props.lc, sg->props.lp, sg->props.pb, sg->cost / 16384.0, (unsigned long long)sg->cost,
		        (unsigned long long)changed);
	}
	return 0;
}

/* --segment-reparse, behind choose_segments: the best slab and the chosen segments go through mgl_segment_reparse once, under
 * the run's match finder; what comes back is what write_stream codes.  Every segment of the returned slab is walked once more
 * on the host, as choose_segments does.  The line formats are fixed (README.md, "Segment re-parse"). */
static int reparse_segments(cli_run* r)
{
	const cli_opts* o = r->o;
	if (!o->segment_reparse || o->rank != 0) return 0;
	const size_t n = r->file_size, nseg = r->nseg;
	mgl_packet* out = (mgl_packet*)malloc(sizeof(mgl_packet) * n);
	mgl_segment segs[MGL_SEG_MAX_CUTS];
	mgl_segment_parse_stats st[MGL_SEG_MAX_CUTS];
	const mgl_adaptive_config ac = { o->segment_reparse, 0, 0, 0, 0, 0 };
	int taken = 0;
	double ms = 0;
	if (!out) return fail("out of memory");
	if (mgl_sa_set_match_finder(r->sa, (int)o->finder, o->mf_depth) != MGL_OK ||
	    mgl_segment_reparse(r->sa, r->packets_best, r->segs, nseg, &ac, out, segs, st, &taken, &ms) != MGL_OK) return lib_error();
	uint64_t was = 0, now = 0;
	size_t reparsed = 0;
	for (size_t k = 0; k < nseg; k++) {
		uint64_t cost = 0, changed = 0;
		if (mgl_host_segment_cost(r->file_data, n, out, segs[k].lo, segs[k].hi, segs[k].props, &cost, &changed) != MGL_OK || cost != segs[k].cost)
			return fail("segment at %llu: the host walk does not confirm the device's cost %llu of the re-parse", (unsigned long long)segs[k].lo,
			            (unsigned long long)segs[k].cost);
		was += st[k].start_cost + (k ? MGL_SEG_OVERHEAD : 0);
		now += st[k].final_cost + (k ? MGL_SEG_OVERHEAD : 0);
		reparsed += st[k].best_pass != UINT32_MAX;
	}
	fprintf(stderr, "segment-reparse: passes %u segments %zu reparsed %zu taken %d was %.3f B exact %llu now %.3f B exact %llu %.3f ms\n", o->segment_reparse,
	        nseg, reparsed, taken, was / 16384.0, (unsigned long long)was, now / 16384.0, (unsigned long long)now, ms);
	for (size_t k = 0; k < nseg; k++) {
		const mgl_segment_parse_stats* s = &st[k];
		uint64_t best = s->start_cost;
		char pass[16] = "-";
		for (uint32_t p = 0; p < s->passes; p++)
			if (s->pass_cost[p] < best) best = s->pass_cost[p];
		if (s->best_pass != UINT32_MAX) snprintf(pass, sizeof pass, "%u", s->best_pass);
		fprintf(stderr, "segment-parse: offset %llu bytes %llu lc=%u lp=%u pb=%u start %.3f B exact %llu best %.3f B exact %llu pass %s final %.3f B exact %llu\n",
		        (unsigned long long)segs[k].lo, (unsigned long long)(segs[k].hi - segs[k].lo), segs[k].props.lc, segs[k].props.lp, segs[k].props.pb,
		        s->start_cost / 16384.0, (unsigned long long)s->start_cost, best / 16384.0, (unsigned long long)best, pass, s->final_cost / 16384.0,
		        (unsigned long long)s->final_cost);
	}
	memcpy(r->packets_best, out, sizeof(mgl_packet) * n);
	memcpy(r->segs, segs, sizeof(mgl_segment) * nseg);
	free(out);
	return 0;
}

static int write_stream(cli_run* r)
{
	const cli_opts* o = r->o;
	FILE* out = stdout;
	OutputInterface output;
	if (o->out_path && (out = fopen(o->out_path, "wb")) == NULL) return fail("could not open %s", o->out_path);
	mgl_file_output_new(&output, out);
	if (o->format_xz) {
		const mgl_xz_options xo = { r->filter == FILTER_X86 ? 4u : 0u, o->dict_size, 1 };
		if (o->segment_props ? !mgl_emit_xz_segments(r->orig_data, r->file_data, r->file_size, r->packets_best, r->segs, r->nseg, &xo, &output)
		                     : !mgl_emit_xz(r->orig_data, r->file_data, r->file_size, r->props, r->packets_best, &xo, &output)) return -1;
	} else if (o->dict_size) {
		if (!mgl_emit_stream_dict(r->file_data, r->file_size, r->props, r->packets_best, o->dict_size, &output)) return -1;
	} else if (!mgl_emit_stream(r->file_data, r->file_size, r->props, r->packets_best, &output)) return -1;
	return (o->out_path ? fclose(out) != 0 : fflush(stdout) != 0) ? fail("could not write the stream") : 0;
}

int main(int argc, char** argv)
{
	cli_opts o;
	if (parse_args(argc, argv, &o) || check_args(&o)) return -1;
	cli_run r = { .o = &o, .cfg = o.cfg, .props = o.props, .filter = o.filter };
	if (map_input(&r)) return -1;
	if (r.file_size == 0) return 0; /* main.c:40-42 */
	if (find_device() ||
	    read_seed_stream_header(&r) ||
	    make_filtered_copy(&r) ||
	    fresh_handle(&r) ||
	    choose_filter(&r) ||
	    auto_props(&r) ||
	    set_temperature(&r) ||
	    open_comm(&r) ||
	    set_accept_mode(&r) ||
	    (r.packets_best = alloc_slab(&r)) == NULL ||
	    load_slab(&r) ||
	    seed_stream_as_best(&r) ||
	    make_run_seed(&r) ||
	    set_focus(&r) ||
	    load_target_weights(&r) ||
	    enable_live_weights(&r) ||
	    run_epochs(&r) ||
	    final_exchange(&r) ||
	    fetch_best(&r) ||
	    report_costs(&r) ||
	    choose_segments(&r) ||
	    reparse_segments(&r)) return -1;
	mgl_comm_destroy(r.comm);
	mgl_sa_destroy(r.sa);
	if (o.rank != 0) return 0; /* every chain holds the common best slab after the last exchange; rank 0 writes it */
	if (write_stream(&r)) return -1;
	free(r.seed_slab);
	free(r.packets_best);
	free(r.filtered);
	munmap((void*)r.orig_data, r.file_size);
	close(r.fd);
	return 0;
}
