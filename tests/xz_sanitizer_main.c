/*
 * Stand-alone driver for tests/test_xz_emit_cpu.py::test_host_paths_under_sanitizers: built together with
 * megalania_amd/host/mgl_host.c under -fsanitize=address,undefined and run as a child process.
 *
 * For n = 0..6 and n = 300 it writes a small filtered .xz with mgl_emit_xz, then hands every prefix of that stream and
 * every single-byte change of its first 64 bytes to mgl_stream_import (MGL_IMPORT_X86) and mgl_stream_info_read_x.
 * Every buffer is a heap block of exactly the size in use, so a read or write one byte outside any of them is a
 * report.  Exit status 0 and "ok" on stdout when every call returned.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../megalania_amd/host/mgl_host.h"

static void* exact(const void* src, size_t len)
{
	void* p = malloc(len); /* a zero-sized block, or none: touching it at all is a report */
	if (len && !p) { fprintf(stderr, "out of memory\n"); exit(2); }
	if (len) memcpy(p, src, len);
	return p;
}

/* one import and one info read of `stream`, whatever they answer */
static void probe(const uint8_t* stream, size_t len, const uint8_t* coded, size_t n, unsigned long* accepted)
{
	uint8_t* s = (uint8_t*)exact(stream, len);
	mgl_packet* out = (mgl_packet*)malloc(sizeof(mgl_packet) * n);
	mgl_import_stats st;
	mgl_stream_info info;
	uint32_t filter = 99;
	if (n && !out) { fprintf(stderr, "out of memory\n"); exit(2); }
	if (mgl_stream_import(s, len, coded, n, 0, MGL_IMPORT_X86, out, &st) == MGL_OK) ++*accepted;
	(void)mgl_stream_info_read_x(s, len, &info, &filter);
	if (filter != 0 && filter != 4) { fprintf(stderr, "filter_out left at %u\n", filter); exit(3); }
	free(out);
	free(s);
}

static int one_size(size_t n)
{
	uint8_t* original = (uint8_t*)malloc(n ? n : 1);
	mgl_packet* slab = (mgl_packet*)malloc(sizeof(mgl_packet) * (n ? n : 1));
	if (!original || !slab) return 2;
	/* period 100, a call every 20 bytes: the filter changes the operands, the period leaves matches */
	for (size_t i = 0; i < n; i++) original[i] = (uint8_t)((i % 100) * 7 + 1);
	for (size_t i = 0; i + 5 <= n; i += 20) { original[i] = 0xE8; original[i + 1] = (uint8_t)i; original[i + 2] = 1; original[i + 3] = 0; original[i + 4] = 0; }
	uint8_t* coded = (uint8_t*)exact(original, n);
	mgl_bcj_x86(coded, n, 1);
	memset(slab, 0, sizeof(mgl_packet) * (n ? n : 1));
	for (size_t i = 0; i < n; i++) { slab[i].type = MGL_LITERAL; slab[i].len = 1; }
	if (n > 150) { /* one copy from a period back, as long as the filtered bytes allow */
		uint32_t len = 0;
		while (150 + len < n && len < MGL_MAX_MATCH && coded[150 + len] == coded[50 + len]) len++;
		if (len >= MGL_MIN_MATCH) { slab[150].type = MGL_MATCH; slab[150].dist = 99; slab[150].len = (uint16_t)len; }
	}
	static uint8_t xz[4096];
	mgl_memory_sink sink = { xz, sizeof xz, 0 };
	OutputInterface output;
	mgl_memory_output_new(&output, &sink);
	const mgl_xz_options opt = { 4, 4096, 1 };
	const mgl_properties props = { 0, 0, 0 };
	if (!mgl_emit_xz(original, coded, n, props, slab, &opt, &output) || sink.len > sizeof xz) return 4;
	/* the inverse filter gives the original back */
	uint8_t* back = (uint8_t*)exact(coded, n);
	mgl_bcj_x86(back, n, 0);
	if (n && memcmp(back, original, n) != 0) return 5;
	free(back);

	unsigned long accepted = 0;
	probe(xz, sink.len, coded, n, &accepted);
	if (accepted != (n ? 1u : 0u)) return 6; /* the whole stream imports; the empty one holds no LZMA chunk, which the importer says */
	for (size_t cut = 0; cut < sink.len; cut++) probe(xz, cut, coded, n, &accepted);
	uint8_t* bad = (uint8_t*)exact(xz, sink.len);
	for (size_t at = 0; at < 64 && at < sink.len; at++) {
		for (unsigned v = 0; v < 256; v++) {
			if (v == xz[at]) continue;
			bad[at] = (uint8_t)v;
			probe(bad, sink.len, coded, n, &accepted);
		}
		bad[at] = xz[at];
	}
	free(bad);
	free(coded);
	free(slab);
	free(original);
	return 0;
}

int main(void)
{
	static const size_t sizes[] = { 0, 1, 2, 3, 4, 5, 6, 300 };
	for (size_t k = 0; k < sizeof sizes / sizeof sizes[0]; k++) {
		const int rc = one_size(sizes[k]);
		if (rc) { fprintf(stderr, "n = %zu: step %d failed\n", sizes[k], rc); return rc; }
	}
	puts("ok");
	return 0;
}
