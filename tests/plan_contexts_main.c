/* Every packet kind planned with the product's own mgl_plan_packet / mgl_plan_event (csrc/mgl_model.h, the code the kernels
 * run) under every ctx_state and position state and several lc / lp / pb: a context occurs at most once in a plan, every
 * key ctx | bit << 15 fits 16 bits, a plan has at most MGL_MAX_EVENTS slots, and the same packet at the same position has
 * the same number of slots whatever the state.  The window walk's event-level cancellation (changes_add_pair) compares the
 * two plans of a position slot by slot and rests on all four.  Prints the number of plans checked; exit status 1 on a miss. */
#include <stdio.h>
#include <string.h>
#include "../megalania_amd/csrc/mgl_model.h"

static unsigned long plans, misses;
static unsigned short seen_at[32768]; /* plan number + 1 in which a context was last seen */

static uint32_t check(const mgl_layout* L, const mgl_wstate* st, uint32_t type, uint32_t dist, uint32_t len, uint32_t byte,
                      uint32_t match_byte, uint32_t prev_byte)
{
	mgl_plan pl;
	static unsigned short stamp;
	mgl_plan_packet(L, st, type, dist, len, byte, match_byte, prev_byte, &pl);
	if (++stamp == 0) { memset(seen_at, 0, sizeof seen_at); stamp = 1; }
	plans++;
	if (pl.nev == 0 || pl.nev > MGL_MAX_EVENTS) { misses++; printf("nev %u: type %u dist %u len %u state %u\n", pl.nev, type, dist, len, st->ctx_state); }
	for (uint32_t slot = 0; slot < pl.nev && slot < 64; slot++) {
		uint32_t ctx = 0xFFFFFFFFu, bit = 2;
		mgl_plan_event(&pl, slot, &ctx, &bit);
		if (ctx >= L->total || ctx >= 32768u || bit > 1u) {
			misses++;
			printf("slot %u ctx %u bit %u out of range (total %u): type %u dist %u len %u state %u pos %u\n", slot, ctx, bit, L->total, type, dist, len, st->ctx_state, st->pos);
			continue;
		}
		if (seen_at[ctx] == stamp) {
			misses++;
			printf("ctx %u twice: type %u dist %u len %u state %u pos %u byte %u match_byte %u lc %u lp %u pb %u\n", ctx, type, dist, len, st->ctx_state, st->pos, byte, match_byte, L->lc, L->lp, L->pb);
		}
		seen_at[ctx] = stamp;
	}
	return pl.nev;
}

int main(void)
{
	static const uint32_t props[][3] = { { 0, 0, 0 }, { 3, 0, 2 }, { 0, 4, 4 }, { 4, 0, 0 }, { 2, 1, 2 }, { 1, 3, 1 } };
	static const uint32_t dists[] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12, 15, 16, 23, 24, 31, 32, 47, 48, 63, 64, 95, 96, 126, 127, 128, 191, 192, 255, 256,
	                                  1000, 4095, 4096, 65535, 65536, 1u << 20, (1u << 22) - 1u, 1u << 22, (1u << 30) + 12345u, 0xFFFFFFFEu };
	static const uint32_t lens[] = { 2, 3, 4, 5, 9, 10, 11, 17, 18, 19, 100, 272, 273 };
	static const uint32_t bytes[] = { 0x00, 0x01, 0x5A, 0x7F, 0x80, 0xA5, 0xFE, 0xFF };
	for (size_t pi = 0; pi < sizeof props / sizeof props[0]; pi++) {
		const mgl_layout L = mgl_make_layout(props[pi][0], props[pi][1], props[pi][2]);
		for (uint32_t pos = 0; pos < 32; pos++) {
			uint32_t nev0[4][64]; /* slots of [kind][variant] under state 0 */
			for (uint32_t state = 0; state < 12; state++) {
				mgl_wstate st;
				st.pos = pos + 4096u; st.ctx_state = state; st.dists[0] = 3; st.dists[1] = 70; st.dists[2] = 500; st.dists[3] = 9000;
				for (size_t b = 0; b < 8; b++)
					for (size_t m = 0; m < 8; m++) {
						const uint32_t n = check(&L, &st, MGL_LITERAL, 0, 1, bytes[b], bytes[m], bytes[(b + m) & 7]);
						if (n != 9u) { misses++; printf("literal with %u slots\n", n); }
					}
				uint32_t v = 0;
				for (size_t d = 0; d < sizeof dists / sizeof dists[0]; d++) {
					const uint32_t len = lens[d % (sizeof lens / sizeof lens[0])];
					const uint32_t n = check(&L, &st, MGL_MATCH, dists[d], len, 0, 0, 0);
					if (state == 0) nev0[0][v] = n; else if (nev0[0][v] != n) { misses++; printf("match dist %u len %u: %u slots under state %u, %u under 0\n", dists[d], len, n, state, nev0[0][v]); }
					v++;
				}
				for (size_t l = 0; l < sizeof lens / sizeof lens[0]; l++) {
					const uint32_t n = check(&L, &st, MGL_MATCH, 5, lens[l], 0, 0, 0);
					if (state == 0) nev0[1][l] = n; else if (nev0[1][l] != n) { misses++; printf("match len %u: slots differ by state\n", lens[l]); }
					for (uint32_t idx = 0; idx < 4; idx++) {
						const uint32_t r = check(&L, &st, MGL_LONG_REP, idx, lens[l], 0, 0, 0);
						if (state == 0) nev0[2][l * 4 + idx] = r; else if (nev0[2][l * 4 + idx] != r) { misses++; printf("long rep %u len %u: slots differ by state\n", idx, lens[l]); }
					}
				}
				if (check(&L, &st, MGL_SHORT_REP, 0, 1, bytes[pos & 7], 0, 0) != 4u) { misses++; printf("short rep: not 4 slots\n"); }
			}
		}
	}
	printf("%lu plans, %lu misses\n", plans, misses);
	return misses ? 1 : 0;
}
