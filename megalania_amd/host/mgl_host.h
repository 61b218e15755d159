/*
 * mgl_host.h -- host-side (C) mirror of the reference's emission path, over the kept
 * EncoderInterface / OutputInterface vtables (include/megalania_interfaces.h).
 *
 * Name map to the reference (same argument order and meaning, `mgl_` prefixed so that the
 * library can be linked next to the reference's own objects without symbol clashes):
 *
 *   mgl_range_encoder_new / _free     range_encoder.c:83-101   (_free flushes 5 bytes, then frees)
 *   mgl_perplexity_encoder_new        perplexity_encoder.c:19-24 (borrows the caller's uint64_t)
 *   mgl_lzma_state_init               lzma_state.c:16-27
 *   mgl_lzma_encode_packet            lzma_packet_encoder.c:169-194
 *   mgl_lzma_encode_header            lzma_header_encoder.c:11-21
 *   mgl_file_output_new               file_output.c:9-13
 *   mgl_memory_output_new             (no reference equivalent: OutputInterface over a buffer)
 *   mgl_emit_stream                   main.c:110-119 as one call
 *   mgl_stream_info_read / _import    (no reference equivalent: the reference has no decoder)
 *   mgl_emit_stream_dict              mgl_emit_stream with the dictionary size as a parameter
 *   mgl_bcj_x86 / mgl_emit_xz         (no reference equivalent: the .xz container and its x86 filter)
 *   mgl_host_cost_map                 (no reference equivalent: perplexity_encoder.c's sum split per byte and per coder)
 *   mgl_host_segment_cost / _packets, mgl_emit_xz_segments  (no reference equivalent: a parse coded in segments, each behind
 *                                     an LZMA2 state reset under its own lc/lp/pb)
 *
 * Stream import reads the parse out of an existing LZMA-alone (.lzma) or .xz stream of the same
 * input, as a starting slab for the search (the best known parse of a file is usually the one
 * xz already wrote).  Range decoder + LZMA packet decoder over the encoder's own contexts
 * (csrc/mgl_model.h); no output is materialised: each decoded byte is compared with `data`,
 * which also serves as the dictionary, whatever size the header declares.  .xz: streams
 * (concatenated ones too), blocks with any check, index, padding, and LZMA2 chunks of every
 * kind; a filter chain other than a single LZMA2 filter is refused, except that MGL_IMPORT_X86 admits [x86, LZMA2], for
 * which `data` is the filtered input.  Checks are not verified
 * (the byte comparison covers the content).  The slab is position-indexed like every slab here
 * (walked packets at their start, all-literal elsewhere); every packet is resolved to its
 * concrete distance under the stream's own rep stack and re-expressed against the output
 * walk's (LZMA2 state resets and clipped copies make them differ): MATCH stays MATCH; a rep
 * becomes LONG_REP(j) / SHORT_REP (j = 0, length 1) where that distance sits at index j of the
 * output stack, else MATCH, or a literal when its length is 1.  For an LZMA-alone stream with
 * nothing clipped this is the identity.  A copy whose 0-based distance is >= `window` (0 = 4 MiB,
 * the dictionary mgl_emit_stream declares) is MGL_ERANGE, or `len` literals under
 * MGL_IMPORT_CLIP_WINDOW.  Truncated / corrupt streams, a byte that differs from the input, a
 * declared size other than n and a stream that ends early are MGL_EINVAL; bytes after the end
 * marker or the declared size are ignored.
 *
 * Error conventions follow the reference: constructors that allocate return false/NULL and
 * print to stderr; a failed OutputInterface.write is only logged (range_encoder.c:29-31).
 */
#ifndef MGL_HOST_H
#define MGL_HOST_H

#include <stdio.h>
#include "../../include/megalania_interfaces.h"
#include "../../include/megalania_hip.h"
#include "../csrc/mgl_model.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lzma_state.h:60-74.  Probabilities are heap-allocated because lc/lp change their number. */
typedef struct {
	const uint8_t* data;
	size_t data_size;
	mgl_properties properties;
	mgl_layout layout;
	mgl_wstate walk; /* ctx_state, rep distances, position */
	Prob* probs;
} mgl_lzma_state;

bool mgl_lzma_state_init(mgl_lzma_state* st, const uint8_t* data, size_t data_size, mgl_properties props);
void mgl_lzma_state_free(mgl_lzma_state* st);
void mgl_lzma_encode_packet(mgl_lzma_state* st, EncoderInterface* enc, mgl_packet packet);
void mgl_lzma_encode_header(const mgl_lzma_state* st, OutputInterface* output);

bool mgl_range_encoder_new(EncoderInterface* enc, OutputInterface* output);
void mgl_range_encoder_free(EncoderInterface* enc);
void mgl_perplexity_encoder_new(EncoderInterface* enc, uint64_t* perplexity);

void mgl_file_output_new(OutputInterface* output, FILE* file);
typedef struct { uint8_t* buf; size_t cap; size_t len; } mgl_memory_sink;
void mgl_memory_output_new(OutputInterface* output, mgl_memory_sink* sink);

/* header + every packet on the slab's walk through a fresh range coder; false on bad input */
bool mgl_emit_stream(const uint8_t* data, size_t n, mgl_properties props, const mgl_packet* slab, OutputInterface* output);
/* the same stream with `dict_size` (0 = 0x400000) as the header's dictionary and as the window the slab is checked against */
bool mgl_emit_stream_dict(const uint8_t* data, size_t n, mgl_properties props, const mgl_packet* slab, uint32_t dict_size,
                          OutputInterface* output);

/* mgl_cost_map (include/megalania_hip.h) without a device: the same integers -- per-byte map (nullable, n entries), class
 * and type tables (nullable; gpu_ms = 0) -- from the slab's walk under `props`, through an EncoderInterface that prices
 * every bit from csrc/mgl_cost_table.inc and files it under the coder its probability belongs to.  MGL_EINVAL, with
 * nothing written, for lc + lp > 4, pb > 4, n = 0 and for a slab that is not a valid parse of the input (the check of
 * mgl_emit_stream with no dictionary limit: a message on stderr names the entry); MGL_ENOMEM when the model cannot be
 * allocated. */
int mgl_host_cost_map(const uint8_t* data, size_t n, mgl_properties props, const mgl_packet* slab, uint32_t* map_out,
                      mgl_cost_report* report);

/* The .xz x86 branch/call/jump filter (filter id 0x04, start offset 0) over the whole buffer, in place: the relative
 * targets of E8 / E9 become absolute ones (encode != 0) or relative ones again (encode == 0). */
void mgl_bcj_x86(uint8_t* buf, size_t n, int encode);

typedef struct {
	uint32_t filter;    /* 0 none, 4 x86 */
	uint32_t dict_size; /* 0 = 0x400000 */
	uint32_t check;     /* 0 none, 1 CRC32 */
} mgl_xz_options;
/* One .xz stream of one block: [x86,] LZMA2 over the slab's walk.  `coded` is what the LZMA layer sees (the filtered
 * input when filter = 4, else `original` itself), `slab` a parse of `coded`; the block check is over `original`.  The
 * declared dictionary is the smallest one the format can name that holds max(dict_size, 4096), and the slab is checked
 * against it.  One model and one rep stack run through all LZMA2 chunks: the first resets dictionary, state and
 * properties, the later ones nothing.  n = 0 writes the empty stream (no block).  opt NULL = all defaults (check none).
 * false (with a message on stderr) on a bad slab or option. */
bool mgl_emit_xz(const uint8_t* original, const uint8_t* coded, size_t n, mgl_properties props, const mgl_packet* slab,
                 const mgl_xz_options* opt, OutputInterface* output);

/* Segment props on the host (include/megalania_hip.h, "Segment props", has the definitions; one re-expression routine
 * serves all three).
 * mgl_host_segment_cost: *cost (nullable) = cost(lo, hi, props), the segment's re-expressed packets through the perplexity
 * encoder from a fresh model; *reexpressed (nullable) = how many of them differ from the slab's.  lo == hi costs 0.
 * MGL_EINVAL: lc + lp > 4 or pb > 4, n = 0, a slab that is not a valid parse (mgl_host_cost_map's check), lo > hi, hi > n,
 * lo or hi not a packet start of the walk.  MGL_ENOMEM when the model cannot be allocated.
 * mgl_host_segment_packets: the same walk without a model; out (nullable, cap entries) receives the re-expressed packets
 * in walk order, *count their number; MGL_ERANGE, with *count set, when out is too small. */
int mgl_host_segment_cost(const uint8_t* data, size_t n, const mgl_packet* slab, uint64_t lo, uint64_t hi, mgl_properties props,
                          uint64_t* cost, uint64_t* reexpressed);
int mgl_host_segment_packets(const uint8_t* data, size_t n, const mgl_packet* slab, uint64_t lo, uint64_t hi, mgl_packet* out,
                             size_t cap, size_t* count);
/* mgl_emit_xz with a triple per segment: still one stream of one block and one dictionary.  segs[0 .. nseg) tile [0, n) in
 * ascending order, every lo a packet start of the slab's walk (`cost` is not looked at).  The first chunk is 0xE0 as in
 * mgl_emit_xz; the first chunk of every later segment is 0xC0 -- state reset and that segment's props byte, also where the
 * triple repeats --; all others are 0x80.  A chunk never crosses a segment's end and a packet is never split; the
 * chunk-size rules are mgl_emit_xz's.  One segment writes mgl_emit_xz's bytes.  n = 0 (with nseg = 0) writes the empty
 * stream.  false (with a message on stderr) as mgl_emit_xz, and when the segments do not tile [0, n) at packet starts. */
bool mgl_emit_xz_segments(const uint8_t* original, const uint8_t* coded, size_t n, const mgl_packet* slab, const mgl_segment* segs,
                          size_t nseg, const mgl_xz_options* opt, OutputInterface* output);

typedef struct {
	int container;            /* 1 LZMA-alone (.lzma), 2 .xz */
	mgl_properties props;     /* .lzma: the header byte; .xz: the first LZMA2 chunk that carries props */
	uint32_t dict_size;       /* as declared (.xz: the first block's LZMA2 filter) */
	uint64_t declared_size;   /* UINT64_MAX = unknown (end marker expected); .xz: the sum of its chunks */
} mgl_stream_info;
/* MGL_OK, or MGL_EINVAL when `stream` is neither container (or a malformed .xz) */
int mgl_stream_info_read(const uint8_t* stream, size_t len, mgl_stream_info* out);
/* the same, except that an .xz whose blocks all use the chain [x86 (no properties, or start offset 0), LZMA2] is read too:
 * *filter_out = 4 for it, 0 for a plain LZMA2 chain and for .lzma */
int mgl_stream_info_read_x(const uint8_t* stream, size_t len, mgl_stream_info* out, uint32_t* filter_out);

#define MGL_IMPORT_CLIP_WINDOW 1u /* copies from beyond the window become literals instead of an error */
#define MGL_IMPORT_X86 2u         /* an .xz chain [x86 (no properties, or start offset 0), LZMA2] is accepted: `data` is then the
                                     filtered input (mgl_bcj_x86), which the caller filters; every other chain is refused */
typedef struct {
	uint64_t packets, literals, matches, short_reps, long_reps[4]; /* as the stream coded them */
	uint64_t reexpressed;     /* packets whose type or rep index had to change */
	uint64_t clipped;         /* copies turned into literals under MGL_IMPORT_CLIP_WINDOW */
	uint64_t props_changes;   /* LZMA2 chunks that set props other than the first ones */
	uint64_t error_pos;       /* input position of the first problem (valid when the call fails) */
	const char* error;        /* static text of the first problem, NULL on success */
} mgl_import_stats;
/* slab_out (nullable: validate only): n entries.  st (nullable).  0 or a negative MGL_E* code. */
int mgl_stream_import(const uint8_t* stream, size_t len, const uint8_t* data, size_t n,
                      uint32_t window, uint32_t flags, mgl_packet* slab_out, mgl_import_stats* st);

#ifdef __cplusplus
}
#endif
#endif
