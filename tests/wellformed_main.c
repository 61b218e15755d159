/* mgl_pk_wellformed (csrc/mgl_model.h: "this slab entry is a packet", host and device code from one source) over every type
 * 0..5 and 255, every length 0..300 and 65535, and every rep index or distance 0..5 and 0xFFFFFFFF.  One line
 * "type dist len verdict" per entry.  Every entry the predicate passes is planned with the product's own mgl_plan_packet /
 * mgl_plan_event under lc/lp/pb 0/0/0 and 3/0/2, all 12 states and several positions: every context lies below L.total and
 * none occurs twice, which is what the walks that index probs[ctx] and count cnt[ctx]++ rely on.  Triples "type dist len"
 * read from stdin are answered as "? type dist len verdict".  Last line: plans checked and misses; exit status 1 on a miss. */
#include <stdio.h>
#include <string.h>
#include "../megalania_amd/csrc/mgl_model.h"

static unsigned long plans, misses;
static unsigned short seen_at[32768]; /* plan number + 1 in which a context was last seen */

static void plan_is_safe(const mgl_layout* L, const mgl_wstate* st, uint32_t type, uint32_t dist, uint32_t len, uint32_t byte, uint32_t match_byte)
{
	mgl_plan pl;
	static unsigned short stamp;
	mgl_plan_packet(L, st, type, dist, len, byte, match_byte, byte ^ 0x5Au, &pl);
	if (++stamp == 0) { memset(seen_at, 0, sizeof seen_at); stamp = 1; }
	plans++;
	if (pl.nev == 0 || pl.nev > MGL_MAX_EVENTS) { misses++; printf("nev %u: type %u dist %u len %u\n", pl.nev, type, dist, len); return; }
	for (uint32_t slot = 0; slot < pl.nev; slot++) {
		uint32_t ctx = 0xFFFFFFFFu, bit = 2;
		mgl_plan_event(&pl, slot, &ctx, &bit);
		if (ctx >= L->total || ctx >= 32768u || bit > 1u) {
			misses++;
			printf("slot %u ctx %u bit %u out of range (total %u): type %u dist %u len %u state %u pos %u\n", slot, ctx, bit, L->total, type, dist, len, st->ctx_state, st->pos);
			continue;
		}
		if (seen_at[ctx] == stamp) { misses++; printf("ctx %u twice: type %u dist %u len %u state %u pos %u\n", ctx, type, dist, len, st->ctx_state, st->pos); }
		seen_at[ctx] = stamp;
	}
}

int main(void)
{
	static const uint32_t types[] = { 0, 1, 2, 3, 4, 5, 255 };
	static const uint32_t dists[] = { 0, 1, 2, 3, 4, 5, 0xFFFFFFFFu };
	static const uint32_t props[][3] = { { 0, 0, 0 }, { 3, 0, 2 } };
	static const uint32_t positions[] = { 0, 1, 2, 3, 255, 256, 4096 + 7 };
	for (size_t ti = 0; ti < sizeof types / sizeof types[0]; ti++)
		for (uint32_t li = 0; li <= 301; li++)
			for (size_t di = 0; di < sizeof dists / sizeof dists[0]; di++) {
				const uint32_t type = types[ti], len = li <= 300 ? li : 65535u, dist = dists[di];
				const int ok = mgl_pk_wellformed(type, dist, len);
				printf("%u %u %u %d\n", type, dist, len, ok);
				if (!ok) continue;
				for (size_t pi = 0; pi < sizeof props / sizeof props[0]; pi++) {
					const mgl_layout L = mgl_make_layout(props[pi][0], props[pi][1], props[pi][2]);
					for (uint32_t state = 0; state < 12; state++)
						for (size_t qi = 0; qi < sizeof positions / sizeof positions[0]; qi++) {
							mgl_wstate st;
							st.pos = positions[qi]; st.ctx_state = state; st.dists[0] = 3; st.dists[1] = 70; st.dists[2] = 500; st.dists[3] = 9000;
							plan_is_safe(&L, &st, type, dist, len, 0xA5u, 0xA4u);
							plan_is_safe(&L, &st, type, dist, len, 0x00u, 0xFFu);
						}
				}
			}
	unsigned type, dist, len;
	while (scanf("%u %u %u", &type, &dist, &len) == 3) printf("? %u %u %u %d\n", type, dist, len, mgl_pk_wellformed(type, dist, len));
	printf("%lu plans, %lu misses\n", plans, misses);
	return misses ? 1 : 0;
}
