/*
 * mgl_host.c -- host emission path in C (see mgl_host.h for the map to the reference).
 * The bit model is shared with the GPU kernels through csrc/mgl_model.h: a packet is
 * planned once and its events are visited in slot order, which is coding order.
 */
#include "mgl_host.h"

#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------ LZMA state / packets */

bool mgl_lzma_state_init(mgl_lzma_state* st, const uint8_t* data, size_t data_size, mgl_properties props)
{
	st->data = data;
	st->data_size = data_size;
	st->properties = props;
	st->layout = mgl_make_layout(props.lc, props.lp, props.pb);
	memset(&st->walk, 0, sizeof st->walk);
	st->probs = (Prob*)malloc(sizeof(Prob) * st->layout.total);
	if (st->probs == NULL) {
		fprintf(stderr, "Error: could not allocate the probability model in mgl_lzma_state_init\n");
		return false;
	}
	for (uint32_t i = 0; i < st->layout.total; i++) st->probs[i] = MGL_PROB_INIT_VAL;
	return true;
}

void mgl_lzma_state_free(mgl_lzma_state* st)
{
	free(st->probs);
	st->probs = NULL;
}

/* plan `packet` at the state's position: the one place that fetches a literal's match byte and previous byte */
static void plan_packet_here(const mgl_lzma_state* st, mgl_packet packet, mgl_plan* plan)
{
	const uint32_t pos = st->walk.pos;
	const uint32_t byte = st->data[pos];
	uint32_t match_byte = 0, prev_byte = 0;
	if (packet.type == MGL_LITERAL) {
		if (st->walk.ctx_state >= 7) match_byte = st->data[pos - st->walk.dists[0] - 1];
		if (pos > 0) prev_byte = st->data[pos - 1];
	}
	mgl_plan_packet(&st->layout, &st->walk, packet.type, packet.dist, packet.len, byte, match_byte, prev_byte, plan);
}

void mgl_lzma_encode_packet(mgl_lzma_state* st, EncoderInterface* enc, mgl_packet packet)
{
	mgl_plan plan;
	plan_packet_here(st, packet, &plan);
	for (uint32_t slot = 0; slot < plan.nev; slot++) {
		if (plan.ndirect && slot == plan.direct_after) {
			(*enc->encode_direct_bits)(enc, plan.direct_val, plan.ndirect);
		}
		uint32_t ctx, bit;
		mgl_plan_event(&plan, slot, &ctx, &bit);
		Prob* prob = &st->probs[ctx];
		(*enc->encode_bit)(enc, bit != 0, *prob); /* sink sees the pre-update value, probability_model.c:7 */
		*prob = (Prob)mgl_prob_update(*prob, bit);
	}
	mgl_advance(&st->walk, packet.type, packet.dist, packet.len);
}

static void encode_header_dict(const mgl_lzma_state* st, uint32_t dict, OutputInterface* output)
{
	uint8_t hdr[13];
	const mgl_properties* p = &st->properties;
	hdr[0] = (uint8_t)((p->pb * 5 + p->lp) * 9 + p->lc);
	for (int i = 0; i < 4; i++) hdr[1 + i] = (uint8_t)(dict >> (8 * i));
	const uint64_t size = (uint32_t)st->data_size; /* :19 goes through htole32 */
	for (int i = 0; i < 8; i++) hdr[5 + i] = (uint8_t)(size >> (8 * i));
	(*output->write)(output, &hdr[0], 1);
	(*output->write)(output, &hdr[1], 4);
	(*output->write)(output, &hdr[5], 8);
}

void mgl_lzma_encode_header(const mgl_lzma_state* st, OutputInterface* output)
{
	encode_header_dict(st, 0x400000, output); /* lzma_header_encoder.c:16 */
}

/* ------------------------------------------------------------------ range coder */

typedef struct {
	OutputInterface* output;
	uint64_t low;
	uint32_t range;
	uint8_t cache;
	uint64_t pending; /* cache byte + the 0xFF run behind it */
	/* range_encoder.c:18-38 hands every byte to OutputInterface.write on its own; here they are
	 * collected and handed over 64 KiB at a time through the same vtable (same bytes, same order) */
	size_t fill;
	bool write_failed;
	uint8_t buf[65536];
} mgl_rc;

#define MGL_RC_TOP 0x01000000u

static void rc_flush(mgl_rc* rc)
{
	if (rc->fill && !(*rc->output->write)(rc->output, rc->buf, rc->fill) && !rc->write_failed) {
		fprintf(stderr, "could not write %zu bytes\n", rc->fill); /* logged only, like range_encoder.c:29-31 */
		rc->write_failed = true;
	}
	rc->fill = 0;
}
static void rc_emit(mgl_rc* rc, uint8_t byte)
{
	rc->buf[rc->fill++] = byte;
	if (rc->fill == sizeof rc->buf) rc_flush(rc);
}

/* move the top byte of `low` out, resolving a possible carry into the bytes held back */
static void rc_shift_low(mgl_rc* rc)
{
	const uint32_t carry = (uint32_t)(rc->low >> 32);
	const uint32_t low32 = (uint32_t)rc->low;
	if (low32 < 0xFF000000u || carry) {
		uint8_t head = rc->cache;
		do {
			rc_emit(rc, (uint8_t)(head + carry));
			head = 0xFF;
		} while (--rc->pending);
		rc->cache = (uint8_t)(low32 >> 24);
	}
	rc->pending++;
	rc->low = (uint64_t)(low32 & 0x00FFFFFFu) << 8;
}

static void rc_encode_bit(EncoderInterface* enc, bool bit, Prob prob)
{
	mgl_rc* rc = (mgl_rc*)enc->private_data;
	const uint32_t bound = (rc->range >> MGL_NUM_BIT_MODEL_TOTAL_BITS) * prob;
	if (bit) {
		rc->low += bound;
		rc->range -= bound;
	} else {
		rc->range = bound;
	}
	while (rc->range < MGL_RC_TOP) {
		rc->range <<= 8;
		rc_shift_low(rc);
	}
}

static void rc_encode_direct_bits(EncoderInterface* enc, unsigned bits, unsigned num_bits)
{
	mgl_rc* rc = (mgl_rc*)enc->private_data;
	while (num_bits--) {
		rc->range >>= 1;
		if ((bits >> num_bits) & 1u) rc->low += rc->range;
		if (rc->range < MGL_RC_TOP) {
			rc->range <<= 8;
			rc_shift_low(rc);
		}
	}
}

bool mgl_range_encoder_new(EncoderInterface* enc, OutputInterface* output)
{
	mgl_rc* rc = (mgl_rc*)malloc(sizeof *rc);
	if (rc == NULL) {
		fprintf(stderr, "Error: could not allocate memory in mgl_range_encoder_new\n");
		return false;
	}
	rc->output = output;
	rc->low = 0;
	rc->range = 0xFFFFFFFFu;
	rc->cache = 0;
	rc->pending = 1;
	rc->fill = 0;
	rc->write_failed = false;
	enc->encode_bit = rc_encode_bit;
	enc->encode_direct_bits = rc_encode_direct_bits;
	enc->private_data = rc;
	return true;
}

void mgl_range_encoder_free(EncoderInterface* enc)
{
	mgl_rc* rc = (mgl_rc*)enc->private_data;
	for (int i = 0; i < 5; i++) rc_shift_low(rc);
	rc_flush(rc);
	free(rc);
	enc->private_data = NULL;
}

/* ------------------------------------------------------------------ perplexity backend */

static const uint16_t k_bit_cost[2048] = {
#include "../csrc/mgl_cost_table.inc"
};

static void perp_encode_bit(EncoderInterface* enc, bool bit, Prob prob)
{
	*(uint64_t*)enc->private_data += k_bit_cost[bit ? 2048 - prob : prob];
}
static void perp_encode_direct_bits(EncoderInterface* enc, unsigned bits, unsigned num_bits)
{
	(void)bits;
	*(uint64_t*)enc->private_data += (uint64_t)num_bits << MGL_NUM_BIT_MODEL_TOTAL_BITS;
}
void mgl_perplexity_encoder_new(EncoderInterface* enc, uint64_t* perplexity)
{
	enc->encode_bit = perp_encode_bit;
	enc->encode_direct_bits = perp_encode_direct_bits;
	enc->private_data = perplexity;
}

/* ------------------------------------------------------------------ outputs */

static bool file_sink_write(OutputInterface* output, const void* data, size_t data_size)
{
	return fwrite(data, data_size, 1, (FILE*)output->private_data) == 1;
}
void mgl_file_output_new(OutputInterface* output, FILE* file)
{
	output->write = file_sink_write;
	output->private_data = file;
}
static bool memory_sink_write(OutputInterface* output, const void* data, size_t data_size)
{
	mgl_memory_sink* s = (mgl_memory_sink*)output->private_data;
	const bool fits = s->len + data_size <= s->cap;
	if (fits) memcpy(s->buf + s->len, data, data_size);
	s->len += data_size; /* keeps counting so the caller learns the needed size */
	return fits;
}
void mgl_memory_output_new(OutputInterface* output, mgl_memory_sink* sink)
{
	output->write = memory_sink_write;
	output->private_data = sink;
}

/* ------------------------------------------------------------------ main.c:110-119 */

#define MGL_DEFAULT_DICT 0x400000u
static const uint8_t k_xz_magic[6] = { 0xFD, '7', 'z', 'X', 'Z', 0x00 };

/* The reference's emitter codes whatever it is given (main.c:116-118) and reads data[pos - dists[0] - 1] unguarded; here
 * a slab is refused unless its walk is a valid parse of the input that a dictionary of `window` bytes can decode: packet
 * types and lengths, MATCH distances inside the window and the prefix, LONG_REP indices, and the copied bytes
 * themselves.  false with a message on stderr. */
static bool slab_is_valid(const uint8_t* data, size_t n, const mgl_packet* slab, uint32_t window)
{
	mgl_wstate w;
	memset(&w, 0, sizeof w);
	const char* why = NULL;
	while (w.pos < n && !why) {
		const mgl_packet* p = &slab[w.pos];
		const size_t pos = w.pos;
		uint32_t src_dist = 0;
		if (p->type < MGL_LITERAL || p->type > MGL_LONG_REP || p->len == 0 || pos + p->len > n) why = "not a packet";
		else if (p->type == MGL_LITERAL) { if (p->len != 1) why = "literal longer than one byte"; }
		else if (p->type == MGL_SHORT_REP) {
			if (p->len != 1) why = "short rep longer than one byte";
			else if (w.dists[0] >= pos) why = "distance reaches before the start of the input";
			else if (data[pos] != data[pos - w.dists[0] - 1]) why = "short rep does not reproduce the input";
		} else {
			if (p->len < MGL_MIN_MATCH || p->len > MGL_MAX_MATCH) why = "match length outside 2..273";
			else if (p->type == MGL_LONG_REP && p->dist > 3) why = "rep index above 3";
			else {
				src_dist = p->type == MGL_MATCH ? p->dist : mgl_dist_at(&w, p->dist);
				if (src_dist >= pos) why = "distance reaches before the start of the input";
				else if (src_dist >= window)
					why = window == MGL_DEFAULT_DICT ? "distance outside the 4 MiB dictionary of the header" : "distance outside the declared dictionary";
				else {
					/* overlapping copies are legal: compare byte by byte */
					const uint8_t* a = data + pos - src_dist - 1;
					const uint8_t* b = data + pos;
					for (uint32_t i = 0; i < p->len; i++) if (a[i] != b[i]) { why = "match does not reproduce the input"; break; }
				}
			}
		}
		if (why) {
			fprintf(stderr, "Error: slab entry at %zu: %s\n", pos, why);
			return false;
		}
		mgl_advance(&w, p->type, p->dist, p->len);
	}
	return true;
}

bool mgl_emit_stream_dict(const uint8_t* data, size_t n, mgl_properties props, const mgl_packet* slab, uint32_t dict_size,
                          OutputInterface* output)
{
	const uint32_t dict = dict_size ? dict_size : MGL_DEFAULT_DICT;
	mgl_lzma_state st;
	if (!mgl_lzma_state_init(&st, data, n, props)) return false;
	if (!slab_is_valid(data, n, slab, dict)) { mgl_lzma_state_free(&st); return false; }
	encode_header_dict(&st, dict, output);
	EncoderInterface enc;
	if (!mgl_range_encoder_new(&enc, output)) { mgl_lzma_state_free(&st); return false; }
	while (st.walk.pos < n) mgl_lzma_encode_packet(&st, &enc, slab[st.walk.pos]);
	mgl_range_encoder_free(&enc);
	mgl_lzma_state_free(&st);
	return true;
}

bool mgl_emit_stream(const uint8_t* data, size_t n, mgl_properties props, const mgl_packet* slab, OutputInterface* output)
{
	return mgl_emit_stream_dict(data, n, props, slab, MGL_DEFAULT_DICT, output);
}

/* ------------------------------------------------------------------ cost map (no reference equivalent)
 *
 * The perplexity backend with a memory: an EncoderInterface that knows which probability each bit it is handed belongs
 * to.  The interface carries the probability's value, not its place, so the sink follows the packet's plan itself: the
 * driver plans the packet it is about to hand to mgl_lzma_encode_packet (the same plan that call makes), and the k-th
 * encode_bit of the packet is event slot k of that plan -- slot order is coding order -- whose context index is the
 * probability's offset in mgl_lzma_state.probs.  The offset names the coder (the ranges of csrc/mgl_model.h). */
typedef struct {
	mgl_plan plan;
	uint32_t slot;
	uint64_t packet_cost;
	uint64_t class_cost[MGL_CC_CLASSES], class_bits[MGL_CC_CLASSES];
} mgl_costmap_sink;

static unsigned costmap_class(uint32_t offset)
{
	return offset < MGL_OFF_LEN ? MGL_CC_KIND : offset < MGL_OFF_REP_LEN ? MGL_CC_LENGTH : offset < MGL_OFF_DIST ? MGL_CC_REP_LENGTH
	     : offset < MGL_OFF_LIT ? MGL_CC_DISTANCE : MGL_CC_LITERAL;
}
static void costmap_encode_bit(EncoderInterface* enc, bool bit, Prob prob)
{
	mgl_costmap_sink* s = (mgl_costmap_sink*)enc->private_data;
	uint32_t offset, planned_bit;
	mgl_plan_event(&s->plan, s->slot++, &offset, &planned_bit);
	const unsigned k = costmap_class(offset);
	const uint64_t cost = k_bit_cost[bit ? 2048 - prob : prob];
	s->class_cost[k] += cost;
	s->class_bits[k] += 1;
	s->packet_cost += cost;
}
static void costmap_encode_direct_bits(EncoderInterface* enc, unsigned bits, unsigned num_bits)
{
	mgl_costmap_sink* s = (mgl_costmap_sink*)enc->private_data;
	(void)bits;
	const uint64_t cost = (uint64_t)num_bits << MGL_NUM_BIT_MODEL_TOTAL_BITS;
	s->class_cost[MGL_CC_DIRECT] += cost;
	s->class_bits[MGL_CC_DIRECT] += num_bits;
	s->packet_cost += cost;
}

int mgl_host_cost_map(const uint8_t* data, size_t n, mgl_properties props, const mgl_packet* slab, uint32_t* map_out,
                      mgl_cost_report* report)
{
	if (!data || !slab || n == 0 || n > 0xFFFFFFFFu) return MGL_EINVAL;
	if (props.lc + props.lp > 4 || props.pb > 4) return MGL_EINVAL;
	if (!slab_is_valid(data, n, slab, 0xFFFFFFFFu)) return MGL_EINVAL; /* a cost has no dictionary: any source inside the input */
	mgl_lzma_state st;
	if (!mgl_lzma_state_init(&st, data, n, props)) return MGL_ENOMEM;
	mgl_costmap_sink sink;
	memset(&sink, 0, sizeof sink);
	EncoderInterface enc = { costmap_encode_bit, costmap_encode_direct_bits, &sink };
	mgl_cost_report r;
	memset(&r, 0, sizeof r);
	while (st.walk.pos < n) {
		const size_t pos = st.walk.pos;
		const mgl_packet pk = slab[pos];
		plan_packet_here(&st, pk, &sink.plan);
		sink.slot = 0;
		sink.packet_cost = 0;
		mgl_lzma_encode_packet(&st, &enc, pk);
		const uint64_t c = sink.packet_cost;
		if (map_out)
			for (uint32_t k = 0; k < pk.len; k++) map_out[pos + k] = (uint32_t)(c / pk.len + (k < c % pk.len ? 1u : 0u));
		r.total += c;
		r.packets++;
		r.type_cost[pk.type - 1] += c;
		r.type_packets[pk.type - 1]++;
		r.type_bytes[pk.type - 1] += pk.len;
	}
	mgl_lzma_state_free(&st);
	for (unsigned k = 0; k < MGL_CC_CLASSES; k++) { r.class_cost[k] = sink.class_cost[k]; r.class_bits[k] = sink.class_bits[k]; }
	if (report) *report = r;
	return MGL_OK;
}

/* ------------------------------------------------------------------ segments (no reference equivalent)
 *
 * A segment's coder starts from an LZMA2 state reset in the middle of the slab's walk: fresh model, ctx_state 0, rep
 * distances (0, 0, 0, 0), the dictionary untouched.  The slab's rep packets name slots of the rep stack of the slab's own
 * walk from byte 0 (`t`); the segment has its own (`r`), so each packet is named again in r's terms
 * (include/megalania_hip.h, "Segment props", has the rule).  The copy itself never changes, so what was valid stays valid. */

static bool props_ok(mgl_properties p) { return p.lc + p.lp <= 4 && p.pb <= 4; }

/* the packet at t's position as the walk with rep stack r codes it */
static mgl_packet seg_reexpress(const mgl_wstate* t, const mgl_wstate* r, mgl_packet pk)
{
	if (pk.type == MGL_SHORT_REP) {
		if (r->dists[0] != t->dists[0]) pk.type = MGL_LITERAL;
	} else if (pk.type == MGL_LONG_REP) {
		const uint32_t d = mgl_dist_at(t, pk.dist);
		if (mgl_dist_at(r, pk.dist) != d) {
			uint32_t j = 0;
			while (j < 4 && r->dists[j] != d) j++;
			if (j < 4) pk.dist = j;
			else { pk.type = MGL_MATCH; pk.dist = d; }
		}
	}
	return pk;
}

static bool same_packet(mgl_packet a, mgl_packet b) { return a.type == b.type && a.dist == b.dist && a.len == b.len; }

/* the slab's own walk from byte 0 up to `to`; false when `to` is no packet start (the slab is a valid parse) */
static bool seg_true_walk(const mgl_packet* slab, uint64_t to, mgl_wstate* t)
{
	memset(t, 0, sizeof *t);
	while (t->pos < to) mgl_advance(t, slab[t->pos].type, slab[t->pos].dist, slab[t->pos].len);
	return t->pos == to;
}

/* The segment [lo, hi) through `enc` under `props`, or, with out != NULL, its re-expressed packets into out[0 .. cap). */
static int seg_walk(const uint8_t* data, size_t n, const mgl_packet* slab, uint64_t lo, uint64_t hi, mgl_properties props,
                    EncoderInterface* enc, mgl_packet* out, size_t cap, size_t* count, uint64_t* reexpressed)
{
	if (!data || !slab || n == 0 || n > 0xFFFFFFFFu || lo > hi || hi > n || !props_ok(props)) return MGL_EINVAL;
	if (!slab_is_valid(data, n, slab, 0xFFFFFFFFu)) return MGL_EINVAL;
	mgl_wstate t;
	if (!seg_true_walk(slab, lo, &t)) return MGL_EINVAL;
	mgl_lzma_state st;
	if (!mgl_lzma_state_init(&st, data, n, props)) return MGL_ENOMEM;
	st.walk.pos = (uint32_t)lo;
	size_t k = 0;
	uint64_t changed = 0;
	while (t.pos < hi) {
		const mgl_packet pk = slab[t.pos], q = seg_reexpress(&t, &st.walk, pk);
		if (!same_packet(pk, q)) changed++;
		if (out && k < cap) out[k] = q;
		k++;
		if (enc) mgl_lzma_encode_packet(&st, enc, q);
		else mgl_advance(&st.walk, q.type, q.dist, q.len);
		mgl_advance(&t, pk.type, pk.dist, pk.len);
	}
	mgl_lzma_state_free(&st);
	if (t.pos != hi) return MGL_EINVAL;
	if (count) *count = k;
	if (reexpressed) *reexpressed = changed;
	return out && k > cap ? MGL_ERANGE : MGL_OK;
}

int mgl_host_segment_cost(const uint8_t* data, size_t n, const mgl_packet* slab, uint64_t lo, uint64_t hi, mgl_properties props,
                          uint64_t* cost, uint64_t* reexpressed)
{
	uint64_t sum = 0;
	EncoderInterface enc;
	mgl_perplexity_encoder_new(&enc, &sum);
	const int rc = seg_walk(data, n, slab, lo, hi, props, &enc, NULL, 0, NULL, reexpressed);
	if (rc == MGL_OK && cost) *cost = sum;
	return rc;
}

int mgl_host_segment_packets(const uint8_t* data, size_t n, const mgl_packet* slab, uint64_t lo, uint64_t hi, mgl_packet* out,
                             size_t cap, size_t* count)
{
	const mgl_properties none = { 0, 0, 0 };
	if (!out && cap) return MGL_EINVAL;
	return seg_walk(data, n, slab, lo, hi, none, NULL, out, cap, count, NULL);
}

/* ------------------------------------------------------------------ x86 BCJ filter (.xz filter id 0x04)
 *
 * The relative 32-bit target behind an E8 (call) or E9 (jmp) opcode becomes an absolute one, so that calls of one
 * function from many places repeat byte for byte.  Only targets whose top byte is 00 or FF (a plausible displacement)
 * are converted; prev_mask remembers which of the last bytes looked like such a top byte or an opcode, so that an opcode
 * byte inside another instruction's operand is not taken for one.  The decoder runs the same scan and subtracts. */

static bool bcj_ms(uint8_t b) { return b == 0x00 || b == 0xFF; }

void mgl_bcj_x86(uint8_t* buf, size_t n, int encode)
{
	static const uint8_t allowed[8] = { 1, 1, 1, 0, 1, 0, 0, 0 };
	static const uint8_t bitno[8] = { 0, 1, 2, 2, 3, 3, 3, 3 };
	if (n < 5) return;
	uint32_t prev_mask = 0;
	size_t prev_pos = (size_t)0 - 5; /* only its distance to p is used, modulo 2^32 */
	size_t p = 0;
	while (p <= n - 5) {
		if (buf[p] != 0xE8 && buf[p] != 0xE9) { p++; continue; }
		const uint32_t off = (uint32_t)(p - prev_pos);
		prev_pos = p;
		if (off > 5) prev_mask = 0;
		else for (uint32_t i = 0; i < off; i++) { prev_mask &= 0x77; prev_mask <<= 1; }
		uint8_t b = buf[p + 4];
		if (bcj_ms(b) && allowed[(prev_mask >> 1) & 7] && (prev_mask >> 1) < 0x10) {
			uint32_t src = (uint32_t)b << 24 | (uint32_t)buf[p + 3] << 16 | (uint32_t)buf[p + 2] << 8 | buf[p + 1];
			uint32_t dest;
			for (;;) {
				dest = encode ? src + (uint32_t)(p + 5) : src - (uint32_t)(p + 5);
				if (prev_mask == 0) break;
				const uint32_t i = bitno[prev_mask >> 1];
				b = (uint8_t)(dest >> (24 - 8 * i));
				if (!bcj_ms(b)) break;
				src = dest ^ ((1u << (32 - 8 * i)) - 1u);
			}
			buf[p + 4] = (uint8_t)~(((dest >> 24) & 1u) - 1u);
			buf[p + 3] = (uint8_t)(dest >> 16);
			buf[p + 2] = (uint8_t)(dest >> 8);
			buf[p + 1] = (uint8_t)dest;
			p += 5;
			prev_mask = 0;
		} else {
			p++;
			prev_mask |= 1;
			if (bcj_ms(b)) prev_mask |= 0x10;
		}
	}
}

/* ------------------------------------------------------------------ .xz writer */

static uint32_t crc32_ieee(uint32_t crc, const uint8_t* p, size_t n)
{
	static uint32_t table[256];
	if (!table[1]) /* filled with the same values by whoever gets here first */
		for (uint32_t i = 0; i < 256; i++) {
			uint32_t c = i;
			for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
			table[i] = c;
		}
	crc = ~crc;
	for (size_t i = 0; i < n; i++) crc = table[(crc ^ p[i]) & 0xFF] ^ (crc >> 8);
	return ~crc;
}

static void le32_put(uint8_t* p, uint32_t v)
{
	for (int i = 0; i < 4; i++) p[i] = (uint8_t)(v >> (8 * i));
}

static size_t xz_varint_put(uint8_t* p, uint64_t v)
{
	size_t k = 0;
	while (v >= 0x80) { p[k++] = (uint8_t)(v | 0x80); v >>= 7; }
	p[k++] = (uint8_t)v;
	return k;
}

/* size that LZMA2 dictionary byte b declares: 2^n or 2^n + 2^(n-1), b = 40 the 4 GiB - 1 maximum */
static uint64_t xz_dict_of_byte(uint32_t b) { return (uint64_t)(2u | (b & 1u)) << (b / 2 + 11); }

/* A chunk is closed before a packet that could take its compressed size past 64 KiB.  The bytes a chunk has cost so far
 * are exact: its encoder has shifted `emitted + pending - 1` bytes out of `low` and the flush shifts five more, each
 * shift being one byte of output.  What one more packet can add is bounded by its events: a modelled bit leaves
 * range >= 2^24 >> 11 = 2^13, so its normalisation shifts at most twice; a direct bit halves the range and shifts at most
 * once.  The longest packet is a MATCH with is_match, is_rep, 10 length bits (two choices and the 8-bit tree), 6 slot
 * bits and 4 align bits (22 modelled bits) and 26 direct bits: 2 * 22 + 26 = 70 bytes. */
#define XZ_PACKET_MAX_BYTES 70u
#define XZ_CHUNK_USIZE_MAX (1u << 21)
#define XZ_CHUNK_CSIZE_MAX (1u << 16)

static size_t rc_bytes_if_flushed(const EncoderInterface* enc, const mgl_memory_sink* sink)
{
	const mgl_rc* rc = (const mgl_rc*)enc->private_data;
	return sink->len + rc->fill + (size_t)rc->pending - 1 + 5;
}

static bool xz_write(OutputInterface* output, const void* p, size_t n, bool* failed)
{
	if (n && !(*output->write)(output, p, n) && !*failed) {
		fprintf(stderr, "could not write %zu bytes\n", n); /* logged only, like the range coder's sink */
		*failed = true;
	}
	return true;
}

/* The writer behind mgl_emit_xz (one segment, [0, n)) and mgl_emit_xz_segments; `who` names the caller in the messages.
 * Segment k > 0 opens with a chunk that resets the state and sets its properties; its packets are re-expressed against the
 * rep stack that starts there (seg_reexpress; the identity in segment 0). */
static bool emit_xz_core(const char* who, const uint8_t* original, const uint8_t* coded, size_t n, const mgl_packet* slab,
                         const mgl_segment* segs, size_t nseg, const mgl_xz_options* opt, OutputInterface* output)
{
	static const mgl_xz_options k_defaults = { 0, 0, 0 };
	if (!opt) opt = &k_defaults;
	if ((opt->filter != 0 && opt->filter != 4) || opt->check > 1) {
		fprintf(stderr, "Error: %s: filter must be 0 or 4 and check 0 or 1\n", who);
		return false;
	}
	for (size_t k = 0; k < nseg; k++)
		if (segs[k].props.lc > 4 || segs[k].props.lp > 4 || segs[k].props.pb > 4 || segs[k].props.lc + segs[k].props.lp > 4) {
			fprintf(stderr, "Error: %s: LZMA2 needs lc + lp <= 4 and pb <= 4\n", who);
			return false;
		}
	if (n && (!original || !coded || !slab)) {
		fprintf(stderr, "Error: %s: null argument\n", who);
		return false;
	}
	if (opt->filter == 0 && coded != original && n && memcmp(coded, original, n) != 0) {
		fprintf(stderr, "Error: %s: without a filter the coded bytes are the original ones\n", who);
		return false;
	}
	const uint32_t want = opt->dict_size ? opt->dict_size : MGL_DEFAULT_DICT;
	uint32_t dict_byte = 0;
	while (dict_byte < 40 && xz_dict_of_byte(dict_byte) < (want < 4096 ? 4096 : want)) dict_byte++;
	const uint32_t window = dict_byte == 40 ? 0xFFFFFFFFu : (uint32_t)xz_dict_of_byte(dict_byte);
	if (!slab_is_valid(coded, n, slab, window)) return false;
	/* the segments tile [0, n) and every one starts at a packet start of the walk */
	for (size_t k = 0; n && k < nseg; k++) {
		mgl_wstate at;
		if (segs[k].lo != (k ? segs[k - 1].hi : 0) || segs[k].hi <= segs[k].lo || segs[k].hi > n || (k + 1 == nseg && segs[k].hi != n) ||
		    !seg_true_walk(slab, segs[k].lo, &at)) {
			fprintf(stderr, "Error: %s: segment %zu does not continue the tiling of the input at a packet start\n", who, k);
			return false;
		}
	}

	bool failed = false;
	uint8_t hdr[32];
	/* stream header: magic, flags (00, check id), CRC32 of the flags */
	const uint8_t flags[2] = { 0, (uint8_t)opt->check };
	memcpy(hdr, k_xz_magic, 6);
	memcpy(hdr + 6, flags, 2);
	le32_put(hdr + 8, crc32_ieee(0, flags, 2));
	xz_write(output, hdr, 12, &failed);

	uint64_t unpadded = 0;
	if (n) {
		/* block header: size byte, flags (number of filters - 1, no size fields), filter flags, zero padding, CRC32 */
		size_t h = 2;
		memset(hdr, 0, sizeof hdr);
		if (opt->filter == 4) { hdr[h++] = 0x04; hdr[h++] = 0x00; }
		hdr[h++] = 0x21; hdr[h++] = 0x01; hdr[h++] = (uint8_t)dict_byte;
		const size_t hsize = (h + 3) / 4 * 4 + 4;
		hdr[0] = (uint8_t)(hsize / 4 - 1);
		hdr[1] = opt->filter == 4 ? 1 : 0;
		le32_put(hdr + hsize - 4, crc32_ieee(0, hdr, hsize - 4));
		xz_write(output, hdr, hsize, &failed);
		unpadded = hsize;

		mgl_lzma_state st;
		mgl_properties props = segs[0].props;
		if (!mgl_lzma_state_init(&st, coded, n, props)) return false;
		uint8_t* cbuf = (uint8_t*)malloc(XZ_CHUNK_CSIZE_MAX);
		if (!cbuf) { fprintf(stderr, "Error: could not allocate memory in %s\n", who); mgl_lzma_state_free(&st); return false; }
		bool first = true, reset = false;
		size_t seg = 0;
		mgl_wstate tw; /* the slab's own walk, whose rep stack the slab's rep packets name */
		memset(&tw, 0, sizeof tw);
		while (st.walk.pos < n) {
			if (st.walk.pos == segs[seg].hi) {
				/* the next segment: a fresh model under its triple, ctx_state 0, reps 0; the position runs on */
				props = segs[++seg].props;
				mgl_lzma_state_free(&st);
				if (!mgl_lzma_state_init(&st, coded, n, props)) { free(cbuf); return false; }
				st.walk.pos = tw.pos;
				reset = true;
			}
			const size_t seg_end = (size_t)segs[seg].hi;
			/* one chunk: a fresh range coder over a memory sink; model and rep stack carry on */
			mgl_memory_sink sink = { cbuf, XZ_CHUNK_CSIZE_MAX, 0 };
			OutputInterface mem;
			mgl_memory_output_new(&mem, &sink);
			EncoderInterface enc;
			if (!mgl_range_encoder_new(&enc, &mem)) { free(cbuf); mgl_lzma_state_free(&st); return false; }
			const size_t start = st.walk.pos;
			do {
				/* the first packet of a chunk always fits: 5 + 70 bytes, at most 273 bytes of input */
				const mgl_packet pk = slab[st.walk.pos];
				mgl_lzma_encode_packet(&st, &enc, seg_reexpress(&tw, &st.walk, pk));
				mgl_advance(&tw, pk.type, pk.dist, pk.len);
			} while (st.walk.pos < seg_end && st.walk.pos - start + slab[st.walk.pos].len <= XZ_CHUNK_USIZE_MAX &&
			         rc_bytes_if_flushed(&enc, &sink) + XZ_PACKET_MAX_BYTES <= XZ_CHUNK_CSIZE_MAX);
			mgl_range_encoder_free(&enc);
			const size_t usize = st.walk.pos - start, csize = sink.len;
			if (csize > XZ_CHUNK_CSIZE_MAX || usize > XZ_CHUNK_USIZE_MAX) { /* the bound above rules this out */
				fprintf(stderr, "Error: %s: an LZMA2 chunk came out at %zu bytes for %zu\n", who, csize, usize);
				free(cbuf);
				mgl_lzma_state_free(&st);
				return false;
			}
			size_t c = 0;
			hdr[c++] = (uint8_t)((first ? 0xE0 : reset ? 0xC0 : 0x80) | ((usize - 1) >> 16));
			hdr[c++] = (uint8_t)((usize - 1) >> 8);
			hdr[c++] = (uint8_t)(usize - 1);
			hdr[c++] = (uint8_t)((csize - 1) >> 8);
			hdr[c++] = (uint8_t)(csize - 1);
			if (first || reset) hdr[c++] = (uint8_t)((props.pb * 5 + props.lp) * 9 + props.lc);
			xz_write(output, hdr, c, &failed);
			xz_write(output, cbuf, csize, &failed);
			unpadded += c + csize;
			first = reset = false;
		}
		free(cbuf);
		mgl_lzma_state_free(&st);
		/* end of the LZMA2 data, block padding, check */
		memset(hdr, 0, 8);
		size_t t = 1;
		unpadded += 1;
		while ((unpadded + (t - 1)) % 4) t++;
		if (opt->check == 1) { le32_put(hdr + t, crc32_ieee(0, original, n)); t += 4; unpadded += 4; }
		xz_write(output, hdr, t, &failed);
	}

	/* index: indicator, number of records, (unpadded size, uncompressed size), padding, CRC32 */
	uint8_t idx[32];
	size_t k = 0;
	memset(idx, 0, sizeof idx);
	idx[k++] = 0x00;
	idx[k++] = n ? 1 : 0;
	if (n) {
		k += xz_varint_put(idx + k, unpadded);
		k += xz_varint_put(idx + k, n);
	}
	k = (k + 3) / 4 * 4;
	le32_put(idx + k, crc32_ieee(0, idx, k));
	k += 4;
	xz_write(output, idx, k, &failed);
	/* footer: CRC32 of the next six bytes, backward size, flags, magic */
	le32_put(hdr + 4, (uint32_t)(k / 4 - 1));
	memcpy(hdr + 8, flags, 2);
	le32_put(hdr, crc32_ieee(0, hdr + 4, 6));
	hdr[10] = 'Y';
	hdr[11] = 'Z';
	xz_write(output, hdr, 12, &failed);
	return true;
}

bool mgl_emit_xz(const uint8_t* original, const uint8_t* coded, size_t n, mgl_properties props, const mgl_packet* slab,
                 const mgl_xz_options* opt, OutputInterface* output)
{
	const mgl_segment whole = { 0, n, props, 0 };
	return emit_xz_core("mgl_emit_xz", original, coded, n, slab, &whole, 1, opt, output);
}

bool mgl_emit_xz_segments(const uint8_t* original, const uint8_t* coded, size_t n, const mgl_packet* slab, const mgl_segment* segs,
                          size_t nseg, const mgl_xz_options* opt, OutputInterface* output)
{
	if (n ? (!segs || nseg == 0) : nseg != 0) {
		fprintf(stderr, "Error: mgl_emit_xz_segments: the segments do not tile the input\n");
		return false;
	}
	return emit_xz_core("mgl_emit_xz_segments", original, coded, n, slab, segs, nseg, opt, output);
}

/* ------------------------------------------------------------------ stream import
 *
 * Reads the parse out of an existing LZMA-alone or .xz stream of `data`.  Nothing is
 * materialised: every decoded byte is compared with the input, which therefore also serves as
 * the dictionary.  The contexts are the encoder's (mgl_model.h), so the decoder below is the
 * exact mirror of mgl_plan_packet / mgl_plan_event.  Every read is bounded; a short or corrupt
 * stream is an error, never an out-of-bounds access. */

typedef struct {
	/* what is being checked and written */
	const uint8_t* data;
	size_t n;
	uint32_t window;
	uint32_t flags;
	mgl_packet* slab;
	mgl_import_stats* st;
	/* the stream's model: layout, probabilities, walk state (ctx_state, reps) */
	mgl_properties props;
	bool have_props;
	mgl_layout L;
	Prob* probs;
	uint32_t probs_cap;
	mgl_wstate sw;
	size_t dict_start; /* input position of the last dictionary reset */
	/* .xz filter chain: [x86, LZMA2] is read only when asked for; `filter` is what the blocks so far declared (0 none, 4 x86) */
	bool accept_x86, have_chain;
	uint32_t filter;
	/* the output walk, whose rep stack the packets are re-expressed against */
	mgl_wstate ow;
	size_t pos;
	/* range decoder over [in, in_end) */
	const uint8_t* in;
	const uint8_t* in_end;
	uint32_t range, code;
	bool overrun;
	/* first problem */
	const char* error;
	size_t error_pos;
	int rc;
} mgl_imp;

static int imp_fail(mgl_imp* im, int rc, const char* why)
{
	if (!im->error) {
		im->error = why;
		im->error_pos = im->pos;
		im->rc = rc;
	}
	return rc;
}

static uint8_t rd_byte(mgl_imp* im)
{
	if (im->in < im->in_end) return *im->in++;
	im->overrun = true;
	return 0;
}

/* normalisation right after every bit, like the encoder's: a well-formed stream is then
 * consumed exactly (5 initial bytes + one per shift) */
static void rd_normalize(mgl_imp* im)
{
	while (im->range < MGL_RC_TOP) {
		im->range <<= 8;
		im->code = (im->code << 8) | rd_byte(im);
	}
}

static bool rd_init(mgl_imp* im, const uint8_t* p, const uint8_t* end)
{
	im->in = p;
	im->in_end = end;
	im->overrun = false;
	im->range = 0xFFFFFFFFu;
	im->code = 0;
	if (rd_byte(im) != 0) return false; /* the encoder's first byte is its initial cache, always 0 */
	for (int i = 0; i < 4; i++) im->code = (im->code << 8) | rd_byte(im);
	return !im->overrun && im->code != 0xFFFFFFFFu;
}

static uint32_t rd_bit(mgl_imp* im, uint32_t ctx)
{
	Prob* p = &im->probs[ctx];
	const uint32_t bound = (im->range >> MGL_NUM_BIT_MODEL_TOTAL_BITS) * *p;
	uint32_t bit;
	if (im->code < bound) {
		im->range = bound;
		bit = 0;
	} else {
		im->code -= bound;
		im->range -= bound;
		bit = 1;
	}
	*p = (Prob)mgl_prob_update(*p, bit);
	rd_normalize(im);
	return bit;
}

static uint32_t rd_direct(mgl_imp* im, uint32_t nbits)
{
	uint32_t v = 0;
	while (nbits--) {
		im->range >>= 1;
		uint32_t bit = im->code >= im->range;
		if (bit) im->code -= im->range;
		v = (v << 1) | bit;
		rd_normalize(im);
	}
	return v;
}

/* bit tree, most significant bit first: contexts 1, 1b, 1bb, ... */
static uint32_t rd_tree(mgl_imp* im, uint32_t base, uint32_t nbits)
{
	uint32_t m = 1;
	for (uint32_t i = 0; i < nbits; i++) m = (m << 1) | rd_bit(im, base + m);
	return m - (1u << nbits);
}

/* reverse bit tree (probability_model.c:34-44), least significant bit first */
static uint32_t rd_tree_rev(mgl_imp* im, uint32_t base, uint32_t nbits)
{
	uint32_t m = 1, v = 0;
	for (uint32_t e = 0; e < nbits; e++) {
		const uint32_t bit = rd_bit(im, base + m);
		m = (m << 1) | bit;
		v |= bit << e;
	}
	return v;
}

/* mgl_plan_length in reverse */
static uint32_t rd_length(mgl_imp* im, uint32_t base, uint32_t pos_state)
{
	if (!rd_bit(im, base)) return MGL_MIN_MATCH + rd_tree(im, base + MGL_LEN_LOW + pos_state * 8, 3);
	if (!rd_bit(im, base + 1)) return MGL_MIN_MATCH + 8 + rd_tree(im, base + MGL_LEN_MID + pos_state * 8, 3);
	return MGL_MIN_MATCH + 16 + rd_tree(im, base + MGL_LEN_HIGH, 8);
}

static bool imp_set_props(mgl_imp* im, uint8_t b)
{
	if (b >= 9 * 5 * 5) return false;
	mgl_properties p = { (uint8_t)(b % 9), (uint8_t)((b / 9) % 5), (uint8_t)(b / 45) };
	im->L = mgl_make_layout(p.lc, p.lp, p.pb);
	if (im->L.total > im->probs_cap) {
		Prob* np = (Prob*)realloc(im->probs, sizeof(Prob) * im->L.total);
		if (!np) return false;
		im->probs = np;
		im->probs_cap = im->L.total;
	}
	if (im->have_props && (p.lc != im->props.lc || p.lp != im->props.lp || p.pb != im->props.pb) && im->st) im->st->props_changes++;
	if (!im->have_props) im->props = p;
	im->have_props = true;
	return true;
}

/* LZMA state reset: fresh probabilities, ctx_state 0, reps 0 (the output walk keeps its own) */
static void imp_reset_state(mgl_imp* im)
{
	for (uint32_t i = 0; i < im->L.total; i++) im->probs[i] = MGL_PROB_INIT_VAL;
	const uint32_t pos = im->sw.pos;
	memset(&im->sw, 0, sizeof im->sw);
	im->sw.pos = pos;
}

/* one literal of the output walk (the slab entry keeps its all-literal default) */
static void imp_put_literal(mgl_imp* im)
{
	mgl_advance(&im->ow, MGL_LITERAL, 0, 1);
	im->pos++;
}

static void imp_put(mgl_imp* im, uint32_t type, uint32_t dist, uint32_t len)
{
	if (im->slab) {
		mgl_packet* e = &im->slab[im->pos];
		e->type = (uint8_t)type;
		e->dist = dist;
		e->len = (uint16_t)len;
	}
	mgl_advance(&im->ow, type, dist, len);
	im->pos += len;
}

/* A copy of `len` bytes from 0-based distance `d` that the stream coded as `type` / `idx`
 * (MATCH: idx unused; LONG_REP: rep index; SHORT_REP).  Checks it against the input and
 * emits it in the output walk's terms. */
static int imp_copy(mgl_imp* im, uint32_t type, uint32_t idx, uint32_t d, uint32_t len)
{
	const size_t pos = im->pos;
	if (len > im->n - pos) return imp_fail(im, MGL_EINVAL, "stream continues past the end of the input");
	if ((size_t)d >= pos - im->dict_start) return imp_fail(im, MGL_EINVAL, "copy reaches before the start of the dictionary");
	const uint8_t* a = im->data + pos - d - 1;
	const uint8_t* b = im->data + pos;
	for (uint32_t i = 0; i < len; i++)
		if (a[i] != b[i]) {
			im->pos = pos + i;
			return imp_fail(im, MGL_EINVAL, "decoded byte differs from the input");
		}
	if (d >= im->window) {
		if (!(im->flags & MGL_IMPORT_CLIP_WINDOW)) return imp_fail(im, MGL_ERANGE, "copy distance outside the window");
		for (uint32_t i = 0; i < len; i++) imp_put_literal(im);
		if (im->st) im->st->clipped++;
		return MGL_OK;
	}
	uint32_t otype = MGL_MATCH, odist = d;
	if (type != MGL_MATCH) {
		/* the stream's own index first: that keeps an unchanged rep stack the identity */
		int j = mgl_dist_at(&im->ow, idx) == d ? (int)idx : -1;
		for (uint32_t k = 0; k < 4 && j < 0; k++) if (im->ow.dists[k] == d) j = (int)k;
		if (len == 1) {
			if (j == 0) { otype = MGL_SHORT_REP; odist = 0; }
			else otype = MGL_LITERAL;
		} else if (j >= 0) { otype = MGL_LONG_REP; odist = (uint32_t)j; }
		if (im->st && (otype != type || (otype == MGL_LONG_REP && odist != idx))) im->st->reexpressed++;
	}
	if (otype == MGL_LITERAL) imp_put_literal(im);
	else imp_put(im, otype, odist, len);
	if (im->st) {
		if (type == MGL_MATCH) im->st->matches++;
		else if (type == MGL_SHORT_REP) im->st->short_reps++;
		else im->st->long_reps[idx]++;
	}
	return MGL_OK;
}

/* Decode packets until the input position reaches `limit`, or an end marker when `limit` is
 * unknown (SIZE_MAX).  *ended = an end marker was met. */
static int imp_decode(mgl_imp* im, size_t limit, bool* ended)
{
	*ended = false;
	const uint32_t pb_mask = (1u << im->L.pb) - 1u, lp_mask = (1u << im->L.lp) - 1u;
	while (im->pos < limit || limit == SIZE_MAX) {
		if (im->overrun) return imp_fail(im, MGL_EINVAL, "stream is truncated");
		const size_t rel = im->pos - im->dict_start;
		const uint32_t state = im->sw.ctx_state;
		const uint32_t pos_state = (uint32_t)rel & pb_mask;
		const uint32_t sp = (state << 4) + pos_state;
		if (!rd_bit(im, MGL_CS_IS_MATCH + sp)) {
			/* literal, mgl_plan_packet / mgl_plan_event */
			if (im->pos >= im->n) return imp_fail(im, MGL_EINVAL, "stream continues past the end of the input");
			const uint32_t prev = rel ? im->data[im->pos - 1] : 0;
			const uint32_t lit_ctx = (((uint32_t)rel & lp_mask) << im->L.lc) + (prev >> (8u - im->L.lc));
			const uint32_t base = MGL_OFF_LIT + 0x300u * lit_ctx;
			uint32_t match_byte = 0, matched = state >= 7;
			if (matched) {
				if ((size_t)im->sw.dists[0] >= rel) return imp_fail(im, MGL_EINVAL, "copy reaches before the start of the dictionary");
				match_byte = im->data[im->pos - im->sw.dists[0] - 1];
			}
			uint32_t sym = 1;
			for (int i = 7; i >= 0; i--) {
				const uint32_t mbit = (match_byte >> i) & 1u;
				const uint32_t bit = rd_bit(im, base + sym + (matched ? (1u + mbit) << 8 : 0));
				sym = (sym << 1) | bit;
				if (matched && bit != mbit) matched = 0;
			}
			if ((sym & 0xFFu) != im->data[im->pos]) return imp_fail(im, MGL_EINVAL, "decoded byte differs from the input");
			mgl_advance(&im->sw, MGL_LITERAL, 0, 1);
			imp_put_literal(im);
			if (im->st) im->st->literals++;
		} else if (!rd_bit(im, MGL_CS_IS_REP + state)) {
			/* match: length, distance slot, then the reverse tree or direct bits + align */
			const uint32_t len = rd_length(im, MGL_OFF_LEN, pos_state);
			const uint32_t len_ctx = len - 2 < 3 ? len - 2 : 3;
			const uint32_t slot = rd_tree(im, MGL_OFF_DIST + len_ctx * 64, 6);
			uint32_t d = slot;
			if (slot >= 4) {
				const uint32_t nlow = (slot >> 1) - 1;
				d = (2u | (slot & 1u)) << nlow;
				if (slot < 14) d += rd_tree_rev(im, MGL_OFF_DIST + MGL_DIST_POS + d - slot, nlow);
				else {
					d += rd_direct(im, nlow - 4) << 4;
					d += rd_tree_rev(im, MGL_OFF_DIST + MGL_DIST_ALIGN, 4);
				}
			}
			if (d == 0xFFFFFFFFu) {
				if (im->overrun) return imp_fail(im, MGL_EINVAL, "stream is truncated");
				*ended = true;
				return MGL_OK;
			}
			if (len > limit - im->pos && limit != SIZE_MAX) return imp_fail(im, MGL_EINVAL, "copy crosses the end of the chunk");
			int rc = imp_copy(im, MGL_MATCH, 0, d, len);
			if (rc) return rc;
			mgl_advance(&im->sw, MGL_MATCH, d, len);
		} else {
			uint32_t type = MGL_LONG_REP, idx = 0, len;
			if (!rd_bit(im, MGL_CS_G0 + state)) {
				if (!rd_bit(im, MGL_CS_REP0_LONG + sp)) type = MGL_SHORT_REP;
			} else if (!rd_bit(im, MGL_CS_G1 + state)) idx = 1;
			else idx = rd_bit(im, MGL_CS_G2 + state) ? 3 : 2;
			len = type == MGL_SHORT_REP ? 1 : rd_length(im, MGL_OFF_REP_LEN, pos_state);
			if (len > limit - im->pos && limit != SIZE_MAX) return imp_fail(im, MGL_EINVAL, "copy crosses the end of the chunk");
			int rc = imp_copy(im, type, idx, mgl_dist_at(&im->sw, idx), len);
			if (rc) return rc;
			mgl_advance(&im->sw, type, idx, len);
		}
		if (im->st) im->st->packets++;
	}
	return MGL_OK;
}

/* the range decoder has consumed its input exactly and ends at zero (as liblzma requires) */
static int imp_finish_rc(mgl_imp* im, bool exact)
{
	if (im->overrun) return imp_fail(im, MGL_EINVAL, "stream is truncated");
	if (im->code != 0) return imp_fail(im, MGL_EINVAL, "range decoder does not end at zero");
	if (exact && im->in != im->in_end) return imp_fail(im, MGL_EINVAL, "LZMA2 chunk has bytes left over");
	return MGL_OK;
}

static uint64_t le_read(const uint8_t* p, int nbytes)
{
	uint64_t v = 0;
	for (int i = nbytes - 1; i >= 0; i--) v = (v << 8) | p[i];
	return v;
}

/* .xz multibyte integer (at most 9 bytes); false on a truncated or overlong one */
static bool xz_varint(const uint8_t* s, size_t len, size_t* at, uint64_t* out)
{
	uint64_t v = 0;
	for (int i = 0; i < 9; i++) {
		if (*at >= len) return false;
		const uint8_t b = s[(*at)++];
		v |= (uint64_t)(b & 0x7F) << (7 * i);
		if (!(b & 0x80)) { *out = v; return b != 0 || i == 0; }
	}
	return false;
}

static const char* xz_filter_name(uint64_t id)
{
	switch (id) {
	case 0x03: return "filter chain holds the delta filter; only a single LZMA2 filter is supported";
	case 0x04: return "filter chain holds the x86 BCJ filter; only a single LZMA2 filter is supported";
	case 0x05: return "filter chain holds the PowerPC BCJ filter; only a single LZMA2 filter is supported";
	case 0x06: return "filter chain holds the IA-64 BCJ filter; only a single LZMA2 filter is supported";
	case 0x07: return "filter chain holds the ARM BCJ filter; only a single LZMA2 filter is supported";
	case 0x08: return "filter chain holds the ARM-Thumb BCJ filter; only a single LZMA2 filter is supported";
	case 0x09: return "filter chain holds the SPARC BCJ filter; only a single LZMA2 filter is supported";
	case 0x0A: return "filter chain holds the ARM64 BCJ filter; only a single LZMA2 filter is supported";
	case 0x21: return "filter chain holds LZMA2 together with other filters; only a single LZMA2 filter is supported";
	default: return "filter chain holds an unknown filter; only a single LZMA2 filter is supported";
	}
}

/* Walk a .xz file: streams, blocks, LZMA2 chunks, index, footers, padding.  With im->data set
 * the LZMA chunks are decoded against it; otherwise only their headers are read (for
 * mgl_stream_info_read: props, dictionary, total size). */
static int xz_walk(mgl_imp* im, const uint8_t* s, size_t len, uint32_t* dict_size, uint64_t* total)
{
	const bool decode = im->data != NULL;
	size_t at = 0;
	uint64_t upos = 0; /* uncompressed bytes so far */
	int nstreams = 0;
	*dict_size = 0;
	for (;;) {
		/* stream padding between streams: zero bytes, a multiple of four */
		if (nstreams) {
			size_t z = at;
			while (z < len && s[z] == 0) z++;
			if (z + 6 > len || memcmp(s + z, k_xz_magic, 6) != 0) break; /* trailing bytes are ignored */
			if ((z - at) % 4) return imp_fail(im, MGL_EINVAL, ".xz stream padding is not a multiple of four bytes");
			at = z;
		}
		if (len - at < 12 || memcmp(s + at, k_xz_magic, 6) != 0) return imp_fail(im, MGL_EINVAL, "not an .xz stream header");
		if (s[at + 6] != 0 || s[at + 7] > 0x0F) return imp_fail(im, MGL_EINVAL, "unsupported .xz stream flags");
		static const uint8_t k_check_size[16] = { 0, 4, 4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64 };
		const uint8_t check_id = s[at + 7];
		const size_t check_size = k_check_size[check_id];
		at += 12;
		nstreams++;
		/* blocks */
		while (at < len && s[at] != 0) {
			const size_t bstart = at;
			const size_t hsize = ((size_t)s[at] + 1) * 4;
			if (hsize > len - at) return imp_fail(im, MGL_EINVAL, ".xz block header is truncated");
			const uint8_t* h = s + at;
			const uint8_t bflags = h[1];
			if (bflags & 0x3C) return imp_fail(im, MGL_EINVAL, "unsupported .xz block flags");
			const unsigned nfilters = (bflags & 3u) + 1;
			size_t hp = 2;
			uint64_t v;
			const size_t hend = hsize - 4; /* CRC32 at the end (not verified) */
			if ((bflags & 0x40) && !xz_varint(h, hend, &hp, &v)) return imp_fail(im, MGL_EINVAL, "bad .xz block header");
			if ((bflags & 0x80) && !xz_varint(h, hend, &hp, &v)) return imp_fail(im, MGL_EINVAL, "bad .xz block header");
			uint64_t ids[4], psize = 0;
			uint8_t dict_byte = 0;
			bool x86_plain = false; /* the first filter is x86 without properties or with start offset 0 */
			for (unsigned f = 0; f < nfilters; f++) {
				if (!xz_varint(h, hend, &hp, &ids[f]) || !xz_varint(h, hend, &hp, &psize) || psize > hend - hp)
					return imp_fail(im, MGL_EINVAL, "bad .xz block header");
				if (ids[f] == 0x21 && psize == 1) dict_byte = h[hp];
				if (f == 0 && ids[f] == 0x04) x86_plain = psize == 0 || (psize == 4 && le_read(h + hp, 4) == 0);
				hp += (size_t)psize;
			}
			uint32_t chain = 0;
			if (im->accept_x86 && nfilters == 2 && ids[0] == 0x04 && ids[1] == 0x21) {
				if (!x86_plain) return imp_fail(im, MGL_EINVAL, "x86 BCJ filter with a start offset other than 0");
				chain = 4;
			} else if (nfilters != 1 || ids[0] != 0x21) {
				for (unsigned f = 0; f < nfilters; f++)
					if (ids[f] != 0x21) return imp_fail(im, MGL_EINVAL, xz_filter_name(ids[f]));
				return imp_fail(im, MGL_EINVAL, xz_filter_name(0x21));
			}
			/* one filtered input serves the whole file: every block has to use the first one's chain */
			if (im->have_chain && chain != im->filter) return imp_fail(im, MGL_EINVAL, "blocks with different filter chains");
			im->have_chain = true;
			im->filter = chain;
			if (psize != 1 || dict_byte > 40) return imp_fail(im, MGL_EINVAL, "bad LZMA2 filter properties");
			if (!*dict_size)
				*dict_size = dict_byte == 40 ? 0xFFFFFFFFu : (2u | (dict_byte & 1u)) << (dict_byte / 2 + 11);
			at += hsize;
			/* LZMA2 chunks; every block starts a fresh decoder, which needs a dictionary reset first */
			bool need_dict_reset = true, need_props = true;
			for (;;) {
				if (at >= len) return imp_fail(im, MGL_EINVAL, "LZMA2 data is truncated");
				const uint8_t c = s[at];
				if (c == 0x00) { at++; break; }
				if (c == 0x01 || c >= 0xE0) {
					need_dict_reset = false;
					if (decode) im->dict_start = im->pos;
				} else if (need_dict_reset) return imp_fail(im, MGL_EINVAL, "LZMA2 chunk without the dictionary reset a block starts with");
				if (c < 0x80) {
					/* uncompressed chunk: its bytes are literals; the LZMA state carries over */
					if (c > 0x02) return imp_fail(im, MGL_EINVAL, "bad LZMA2 control byte");
					if (len - at < 3) return imp_fail(im, MGL_EINVAL, "LZMA2 data is truncated");
					const size_t usize = ((size_t)s[at + 1] << 8 | s[at + 2]) + 1;
					at += 3;
					if (usize > len - at) return imp_fail(im, MGL_EINVAL, "LZMA2 data is truncated");
					if (c == 0x01) need_props = true;
					if (decode) {
						if (usize > im->n - im->pos) return imp_fail(im, MGL_EINVAL, "stream continues past the end of the input");
						for (size_t i = 0; i < usize; i++) {
							if (s[at + i] != im->data[im->pos]) return imp_fail(im, MGL_EINVAL, "decoded byte differs from the input");
							imp_put_literal(im);
						}
						im->sw.pos += (uint32_t)usize;
						if (im->st) { im->st->packets += usize; im->st->literals += usize; }
					}
					upos += usize;
					at += usize;
					continue;
				}
				const int reset = (c >> 5) & 3; /* 0 none, 1 state, 2 state + props, 3 + dictionary */
				if (len - at < 5 + (reset >= 2)) return imp_fail(im, MGL_EINVAL, "LZMA2 data is truncated");
				const size_t usize = ((size_t)(c & 0x1F) << 16 | (size_t)s[at + 1] << 8 | s[at + 2]) + 1;
				const size_t csize = ((size_t)s[at + 3] << 8 | s[at + 4]) + 1;
				at += 5;
				if (reset >= 2) {
					const uint8_t pbyte = s[at++];
					if (pbyte >= 225 || pbyte % 9 + (pbyte / 9) % 5 > 4) return imp_fail(im, MGL_EINVAL, "bad LZMA2 properties");
					if (!imp_set_props(im, pbyte)) return imp_fail(im, MGL_ENOMEM, "out of memory");
					need_props = false;
				} else if (need_props) return imp_fail(im, MGL_EINVAL, "LZMA2 chunk without the properties it needs");
				if (csize > len - at) return imp_fail(im, MGL_EINVAL, "LZMA2 data is truncated");
				if (decode) {
					if (reset >= 1) imp_reset_state(im);
					if (!rd_init(im, s + at, s + at + csize)) return imp_fail(im, MGL_EINVAL, "bad range coder start");
					if (usize > im->n - im->pos) return imp_fail(im, MGL_EINVAL, "stream continues past the end of the input");
					bool ended;
					int rc = imp_decode(im, im->pos + usize, &ended);
					if (!rc && ended) rc = imp_fail(im, MGL_EINVAL, "end marker inside an LZMA2 chunk");
					if (!rc) rc = imp_finish_rc(im, true);
					if (rc) return rc;
				}
				upos += usize;
				at += csize;
			}
			/* block padding to a multiple of four, then the check (not verified: the bytes were) */
			while ((at - bstart) % 4) {
				if (at >= len || s[at] != 0) return imp_fail(im, MGL_EINVAL, "bad .xz block padding");
				at++;
			}
			if (check_size > len - at) return imp_fail(im, MGL_EINVAL, ".xz block check is truncated");
			at += check_size;
		}
		/* index: indicator, record count, (unpadded, uncompressed) pairs, padding, CRC32 */
		if (at >= len) return imp_fail(im, MGL_EINVAL, ".xz index is missing");
		const size_t istart = at++;
		uint64_t nrec, v;
		if (!xz_varint(s, len, &at, &nrec)) return imp_fail(im, MGL_EINVAL, "bad .xz index");
		for (uint64_t r = 0; r < nrec; r++)
			if (!xz_varint(s, len, &at, &v) || !xz_varint(s, len, &at, &v)) return imp_fail(im, MGL_EINVAL, "bad .xz index");
		while ((at - istart) % 4) {
			if (at >= len || s[at] != 0) return imp_fail(im, MGL_EINVAL, "bad .xz index padding");
			at++;
		}
		if (len - at < 4 + 12) return imp_fail(im, MGL_EINVAL, ".xz stream footer is truncated");
		at += 4;
		const uint8_t* f = s + at;
		if (f[10] != 'Y' || f[11] != 'Z' || f[8] != 0 || f[9] != check_id) return imp_fail(im, MGL_EINVAL, "bad .xz stream footer");
		if (le_read(f + 4, 4) * 4 + 4 != at - istart) return imp_fail(im, MGL_EINVAL, ".xz stream footer does not match the index");
		at += 12;
	}
	if (!im->have_props) return imp_fail(im, MGL_EINVAL, ".xz stream holds no LZMA chunk");
	*total = upos;
	return MGL_OK;
}

static bool is_xz(const uint8_t* s, size_t len)
{
	return len >= 6 && memcmp(s, k_xz_magic, 6) == 0;
}

static int stream_info_read(const uint8_t* stream, size_t len, mgl_stream_info* out, bool accept_x86, uint32_t* filter_out)
{
	if (filter_out) *filter_out = 0;
	if (!stream || !out) return MGL_EINVAL;
	memset(out, 0, sizeof *out);
	if (is_xz(stream, len)) {
		mgl_imp im;
		memset(&im, 0, sizeof im);
		im.accept_x86 = accept_x86;
		uint32_t dict = 0;
		uint64_t total = 0;
		const int rc = xz_walk(&im, stream, len, &dict, &total);
		free(im.probs);
		if (rc) return rc;
		out->container = 2;
		out->props = im.props;
		out->dict_size = dict;
		out->declared_size = total;
		if (filter_out) *filter_out = im.filter;
		return MGL_OK;
	}
	if (len < 13 || stream[0] >= 225) return MGL_EINVAL;
	out->container = 1;
	out->props.lc = (uint8_t)(stream[0] % 9);
	out->props.lp = (uint8_t)((stream[0] / 9) % 5);
	out->props.pb = (uint8_t)(stream[0] / 45);
	out->dict_size = (uint32_t)le_read(stream + 1, 4);
	out->declared_size = le_read(stream + 5, 8);
	return MGL_OK;
}

int mgl_stream_info_read(const uint8_t* stream, size_t len, mgl_stream_info* out)
{
	return stream_info_read(stream, len, out, false, NULL);
}

int mgl_stream_info_read_x(const uint8_t* stream, size_t len, mgl_stream_info* out, uint32_t* filter_out)
{
	return stream_info_read(stream, len, out, true, filter_out);
}

int mgl_stream_import(const uint8_t* stream, size_t len, const uint8_t* data, size_t n, uint32_t window, uint32_t flags,
                      mgl_packet* slab_out, mgl_import_stats* st)
{
	if (st) memset(st, 0, sizeof *st);
	if (!stream || (!data && n)) {
		if (st) st->error = "null argument";
		return MGL_EINVAL;
	}
	static const uint8_t k_empty = 0;
	mgl_imp im;
	memset(&im, 0, sizeof im);
	im.data = data ? data : &k_empty; /* non-NULL: xz_walk decodes */
	im.n = n;
	im.window = window ? window : 0x400000u; /* 0 = the dictionary mgl_emit_stream declares */
	im.flags = flags;
	im.accept_x86 = (flags & MGL_IMPORT_X86) != 0;
	im.slab = slab_out;
	im.st = st;
	if (slab_out) {
		/* the all-literal slab (padding bytes zero, like binding.literal_slab) */
		memset(slab_out, 0, sizeof(mgl_packet) * n);
		for (size_t i = 0; i < n; i++) { slab_out[i].type = MGL_LITERAL; slab_out[i].len = 1; }
	}
	int rc = MGL_OK;
	if (is_xz(stream, len)) {
		uint32_t dict;
		uint64_t total;
		rc = xz_walk(&im, stream, len, &dict, &total);
		if (!rc && im.pos != n) rc = imp_fail(&im, MGL_EINVAL, "stream ends before the end of the input");
	} else if (len < 13) {
		rc = imp_fail(&im, MGL_EINVAL, "stream is shorter than an LZMA header");
	} else {
		const uint64_t declared = le_read(stream + 5, 8);
		if (stream[0] >= 225) rc = imp_fail(&im, MGL_EINVAL, "bad LZMA properties byte");
		else if (!imp_set_props(&im, stream[0])) rc = imp_fail(&im, MGL_ENOMEM, "out of memory");
		else if (declared != UINT64_MAX && declared != n) rc = imp_fail(&im, MGL_EINVAL, "declared size differs from the input");
		if (!rc) {
			imp_reset_state(&im);
			if (!rd_init(&im, stream + 13, stream + len)) rc = imp_fail(&im, MGL_EINVAL, "bad range coder start");
		}
		if (!rc) {
			bool ended = false;
			rc = imp_decode(&im, declared == UINT64_MAX ? SIZE_MAX : n, &ended);
			if (!rc && im.pos != n) rc = imp_fail(&im, MGL_EINVAL, "stream ends before the end of the input");
			if (!rc) rc = imp_finish_rc(&im, false);
		}
	}
	free(im.probs);
	if (rc && st) {
		st->error = im.error;
		st->error_pos = im.error_pos;
	}
	return rc;
}
