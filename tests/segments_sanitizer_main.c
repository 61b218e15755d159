/*
 * Stand-alone driver for tests/test_xz_segments_cpu.py::test_segment_paths_under_sanitizers: built together with
 * megalania_amd/host/mgl_host.c under -fsanitize=address,undefined and run as a child process.
 *
 * A planted slab over an input of period 7 -- literals, four matches at four different distances, then rep packets of every
 * kind -- goes through mgl_host_segment_cost and mgl_host_segment_packets for every pair of packet starts and through
 * mgl_emit_xz_segments for every way to cut it in two and for the cut at every packet start at once (as far as 16 segments
 * go); every stream is read back by mgl_stream_import.  Positions off the walk and segments that do not tile are handed in
 * too.  Every buffer is a heap block of exactly the size in use, so a read or write one byte outside any of them is a
 * report.  Exit status 0 and "ok" on stdout when every call answered as expected.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../megalania_amd/host/mgl_host.h"

#define PERIOD 7u
#define FAIL(step) do { fprintf(stderr, "step %d failed at line %d\n", (step), __LINE__); exit(step); } while (0)

static void* exact(size_t len)
{
	void* p = malloc(len);
	if (len && !p) { fprintf(stderr, "out of memory\n"); exit(2); }
	return p;
}

static size_t put(mgl_packet* slab, size_t pos, unsigned type, uint32_t dist, unsigned len)
{
	slab[pos].type = (uint8_t)type;
	slab[pos].dist = dist;
	slab[pos].len = (uint16_t)len;
	return pos + len;
}

static int import_ok(const uint8_t* xz, size_t len, const uint8_t* data, size_t n, uint64_t* props_changes)
{
	uint8_t* s = (uint8_t*)exact(len);
	mgl_packet* out = (mgl_packet*)exact(sizeof(mgl_packet) * n);
	mgl_import_stats st;
	memcpy(s, xz, len);
	const int rc = mgl_stream_import(s, len, data, n, 0, 0, out, &st);
	if (props_changes) *props_changes = st.props_changes;
	free(out);
	free(s);
	return rc == MGL_OK;
}

int main(void)
{
	/* the walk: 35 literals, MATCH 1..4 periods back, then reps; n is fixed by the packets */
	static const struct { unsigned type; uint32_t dist; unsigned len; } tail[] = {
		{ MGL_SHORT_REP, 0, 1 }, { MGL_LONG_REP, 1, 5 }, { MGL_LONG_REP, 0, 2 }, { MGL_LONG_REP, 3, 273 }, { MGL_LITERAL, 0, 1 },
		{ MGL_LONG_REP, 2, 9 }, { MGL_SHORT_REP, 0, 1 }, { MGL_MATCH, 5 * PERIOD - 1, 18 }, { MGL_LONG_REP, 3, 4 }, { MGL_LITERAL, 0, 1 },
		{ MGL_LITERAL, 0, 1 }, { MGL_LONG_REP, 1, 2 }, { MGL_SHORT_REP, 0, 1 }, { MGL_LONG_REP, 2, 30 }, { MGL_LITERAL, 0, 1 },
	};
	size_t n = 5 * PERIOD + 4 * 3;
	for (size_t k = 0; k < sizeof tail / sizeof tail[0]; k++) n += tail[k].len;
	uint8_t* data = (uint8_t*)exact(n);
	mgl_packet* slab = (mgl_packet*)exact(sizeof(mgl_packet) * n);
	for (size_t i = 0; i < n; i++) data[i] = (uint8_t)(0x41 + 29 * (i % PERIOD));
	memset(slab, 0, sizeof(mgl_packet) * n);
	for (size_t i = 0; i < n; i++) { slab[i].type = MGL_LITERAL; slab[i].len = 1; }
	size_t pos = 5 * PERIOD;
	for (uint32_t k = 1; k <= 4; k++) pos = put(slab, pos, MGL_MATCH, k * PERIOD - 1, 3);
	for (size_t k = 0; k < sizeof tail / sizeof tail[0]; k++) pos = put(slab, pos, tail[k].type, tail[k].dist, tail[k].len);
	if (pos != n) FAIL(3);

	size_t* starts = (size_t*)exact(sizeof(size_t) * (n + 1));
	size_t ns = 0;
	for (pos = 0; pos < n; pos += slab[pos].len) starts[ns++] = pos;
	starts[ns] = n;

	const mgl_properties triples[3] = { { 0, 0, 0 }, { 3, 0, 2 }, { 0, 4, 4 } };
	/* every pair of packet starts: cost, count, packets into a block of exactly that many */
	for (size_t a = 0; a <= ns; a++)
		for (size_t b = a; b <= ns; b++) {
			uint64_t cost = 0, changed = 0;
			size_t count = 0;
			if (mgl_host_segment_cost(data, n, slab, starts[a], starts[b], triples[(a + b) % 3], &cost, &changed) != MGL_OK) FAIL(4);
			if ((cost == 0) != (a == b) || changed > b - a) FAIL(5);
			if (mgl_host_segment_packets(data, n, slab, starts[a], starts[b], NULL, 0, &count) != MGL_OK || count != b - a) FAIL(6);
			mgl_packet* out = (mgl_packet*)exact(sizeof(mgl_packet) * count);
			if (mgl_host_segment_packets(data, n, slab, starts[a], starts[b], out, count, &count) != MGL_OK) FAIL(7);
			size_t bytes = 0;
			for (size_t k = 0; k < count; k++) bytes += out[k].len;
			if (bytes != starts[b] - starts[a]) FAIL(8);
			if (count && mgl_host_segment_packets(data, n, slab, starts[a], starts[b], out, count - 1, &count) != MGL_ERANGE) FAIL(9);
			free(out);
		}
	/* from byte 0 a segment is the plain cost */
	for (unsigned t = 0; t < 3; t++) {
		uint64_t cost = 0;
		mgl_cost_report rep;
		if (mgl_host_segment_cost(data, n, slab, 0, n, triples[t], &cost, NULL) != MGL_OK) FAIL(10);
		if (mgl_host_cost_map(data, n, triples[t], slab, NULL, &rep) != MGL_OK || rep.total != cost) FAIL(11);
	}
	/* off the walk, out of range, a bad triple */
	const mgl_properties bad_triple = { 3, 2, 0 };
	for (pos = 1; pos < n; pos++) {
		size_t k = 0;
		while (k < ns && starts[k] != pos) k++;
		if (k < ns) continue;
		if (mgl_host_segment_cost(data, n, slab, pos, n, triples[0], NULL, NULL) != MGL_EINVAL) FAIL(12);
		if (mgl_host_segment_cost(data, n, slab, 0, pos, triples[0], NULL, NULL) != MGL_EINVAL) FAIL(13);
	}
	if (mgl_host_segment_cost(data, n, slab, 0, n + 1, triples[0], NULL, NULL) != MGL_EINVAL) FAIL(14);
	if (mgl_host_segment_cost(data, n, slab, 0, n, bad_triple, NULL, NULL) != MGL_EINVAL) FAIL(15);

	/* the writer: one segment is mgl_emit_xz; every cut in two; 16 segments at once */
	static uint8_t xz[8192], one[8192];
	const mgl_xz_options opt = { 0, 4096, 1 };
	OutputInterface output;
	mgl_memory_sink sink = { one, sizeof one, 0 };
	mgl_memory_output_new(&output, &sink);
	if (!mgl_emit_xz(data, data, n, triples[1], slab, &opt, &output) || sink.len > sizeof one) FAIL(16);
	const size_t one_len = sink.len;
	mgl_segment* segs = (mgl_segment*)exact(sizeof(mgl_segment) * 1);
	segs[0] = (mgl_segment){ 0, n, triples[1], 0 };
	sink = (mgl_memory_sink){ xz, sizeof xz, 0 };
	if (!mgl_emit_xz_segments(data, data, n, slab, segs, 1, &opt, &output)) FAIL(17);
	if (sink.len != one_len || memcmp(xz, one, one_len) != 0) FAIL(18);
	free(segs);
	for (size_t a = 1; a < ns; a++) {
		segs = (mgl_segment*)exact(sizeof(mgl_segment) * 2);
		segs[0] = (mgl_segment){ 0, starts[a], triples[a % 3], 0 };
		segs[1] = (mgl_segment){ starts[a], n, triples[(a + 1) % 3], 0 };
		sink = (mgl_memory_sink){ xz, sizeof xz, 0 };
		uint64_t changes = 0;
		if (!mgl_emit_xz_segments(data, data, n, slab, segs, 2, &opt, &output) || sink.len > sizeof xz) FAIL(19);
		if (!import_ok(xz, sink.len, data, n, &changes) || changes != 1) FAIL(20);
		/* the same two segments with a gap, an overlap, a short end, the second one first: refused, nothing read outside */
		segs[1].lo = starts[a] + 1;
		if (mgl_emit_xz_segments(data, data, n, slab, segs, 2, &opt, &output)) FAIL(21);
		segs[1].lo = starts[a - 1];
		if (mgl_emit_xz_segments(data, data, n, slab, segs, 2, &opt, &output)) FAIL(22);
		segs[1].lo = starts[a]; segs[1].hi = n - 1;
		if (mgl_emit_xz_segments(data, data, n, slab, segs, 2, &opt, &output)) FAIL(23);
		segs[1].hi = n;
		if (mgl_emit_xz_segments(data, data, n, slab, segs, 1, &opt, &output)) FAIL(24);
		free(segs);
	}
	/* a cut inside a packet */
	segs = (mgl_segment*)exact(sizeof(mgl_segment) * 2);
	segs[0] = (mgl_segment){ 0, 5 * PERIOD + 1, triples[0], 0 };
	segs[1] = (mgl_segment){ 5 * PERIOD + 1, n, triples[0], 0 };
	if (mgl_emit_xz_segments(data, data, n, slab, segs, 2, &opt, &output)) FAIL(25);
	free(segs);
	if (mgl_emit_xz_segments(data, data, n, slab, NULL, 0, &opt, &output)) FAIL(26);
	/* 16 segments, cut at the last 15 packet starts */
	const size_t many = 16;
	if (ns < many) FAIL(27);
	segs = (mgl_segment*)exact(sizeof(mgl_segment) * many);
	for (size_t k = 0; k < many; k++) {
		const size_t lo = k ? starts[ns - many + k] : 0, hi = k + 1 < many ? starts[ns - many + k + 1] : n;
		segs[k] = (mgl_segment){ lo, hi, triples[k % 3], 0 };
	}
	sink = (mgl_memory_sink){ xz, sizeof xz, 0 };
	if (!mgl_emit_xz_segments(data, data, n, slab, segs, many, &opt, &output) || sink.len > sizeof xz) FAIL(28);
	if (!import_ok(xz, sink.len, data, n, NULL)) FAIL(29);
	free(segs);
	/* the empty input */
	sink = (mgl_memory_sink){ xz, sizeof xz, 0 };
	if (!mgl_emit_xz_segments(NULL, NULL, 0, NULL, NULL, 0, &opt, &output)) FAIL(30);
	free(starts);
	free(slab);
	free(data);
	puts("ok");
	return 0;
}
