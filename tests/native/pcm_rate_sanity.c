/* The plain-C host side of the rate matcher (csrc/pcm_rate.c) over its edges, on exactly-sized heap rows: a program of its own, built with ASan
 * and UBSan by tests/test_pcm_rate_cpu.py and run as a program.  Prints "ok" at the end. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/sdrfm.h"

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd(void) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

/* a legal table of random taps: |coef| <= 65535 / (nt / 2) keeps every half row at the bound or below */
static int16_t* make_table(uint32_t nt, uint32_t logph) {
  const uint32_t rows = (1u << logph) + 1u;
  const int32_t lim = (int32_t)(65535u / (nt / 2u)) > 32767 ? 32767 : (int32_t)(65535u / (nt / 2u));
  int16_t* c = (int16_t*)malloc(sizeof(int16_t) * rows * nt);
  CHECK(c);
  for (uint32_t k = 0; k < rows * nt; ++k) c[k] = (int16_t)((int32_t)(rnd() % (2u * (uint32_t)lim + 1u)) - lim);
  return c;
}

static int16_t* make_row(uint32_t n) {
  int16_t* x = (int16_t*)malloc(sizeof(int16_t) * 2 * (n ? n : 1u));   /* (malloc(0) may be NULL) */
  CHECK(x);
  for (uint32_t k = 0; k < 2 * n; ++k) x[k] = (int16_t)(rnd() & 0xFFFFu);
  if (n >= 2) { x[0] = x[1] = -32768; x[2] = x[3] = 32767; }
  return x;
}

static uint32_t cap_of(uint64_t step, uint32_t n) { return (uint32_t)((((uint64_t)n << 32) / step) + 1u); }

/* the whole row in one call against the row cut at `cut`: outputs, pos and hist */
static void cut_case(const int16_t* coef, uint32_t nt, uint32_t logph, uint64_t step, const int16_t* x, uint32_t n, const int16_t* whole, uint32_t n_whole,
                     uint64_t pos_whole, const int16_t* hist_whole, uint32_t cut) {
  const uint32_t hn = 2 * (nt - 1);
  int16_t* hist = (int16_t*)calloc(hn, sizeof(int16_t));
  CHECK(hist);
  uint64_t pos = 0;
  uint32_t got = 0, total = 0;
  const uint32_t len[2] = {cut, n - cut};
  for (int k = 0; k < 2; ++k) {
    /* exactly-sized copies of the piece and of its outputs: a read or a write one element out of place is a report */
    int16_t* piece = (int16_t*)malloc(sizeof(int16_t) * 2 * (len[k] ? len[k] : 1u));
    CHECK(piece);
    memcpy(piece, x + 2 * (size_t)(k ? cut : 0), sizeof(int16_t) * 2 * len[k]);
    uint32_t want = 0;
    {
      uint64_t p2 = pos;
      int16_t* h2 = (int16_t*)malloc(sizeof(int16_t) * hn);
      int16_t* big = (int16_t*)malloc(sizeof(int16_t) * 2 * cap_of(step, len[k]));
      CHECK(h2 && big);
      memcpy(h2, hist, sizeof(int16_t) * hn);
      CHECK(sdrfm_pcm_rate_s16(len[k] ? piece : NULL, len[k], coef, nt, logph, step, &p2, h2, big, cap_of(step, len[k]), &want) == SDRFM_OK);
      free(h2);
      free(big);
    }
    int16_t* out = (int16_t*)malloc(sizeof(int16_t) * 2 * (want ? want : 1u));
    CHECK(out);
    if (want) {                                                   /* one pair short: refused, nothing written, the state as it was */
      const uint64_t p0 = pos;
      int16_t* h0 = (int16_t*)malloc(sizeof(int16_t) * hn);
      CHECK(h0);
      memcpy(h0, hist, sizeof(int16_t) * hn);
      memset(out, 0x5A, sizeof(int16_t) * 2 * want);
      got = 77;
      CHECK(sdrfm_pcm_rate_s16(piece, len[k], coef, nt, logph, step, &pos, hist, out, want - 1u, &got) == SDRFM_ECAPACITY);
      CHECK(pos == p0 && got == 77 && memcmp(h0, hist, sizeof(int16_t) * hn) == 0);
      for (uint32_t q = 0; q < 2 * want; ++q) CHECK(out[q] == 0x5A5A);
      free(h0);
    }
    CHECK(sdrfm_pcm_rate_s16(len[k] ? piece : NULL, len[k], coef, nt, logph, step, &pos, hist, want ? out : NULL, want, &got) == SDRFM_OK);
    CHECK(got == want && total + got <= n_whole);
    CHECK(memcmp(out, whole + 2 * (size_t)total, sizeof(int16_t) * 2 * got) == 0);
    total += got;
    free(out);
    free(piece);
  }
  CHECK(total == n_whole && pos == pos_whole && memcmp(hist, hist_whole, sizeof(int16_t) * hn) == 0);
  free(hist);
}

static void every_cut(uint32_t nt, uint32_t logph, uint64_t step, uint32_t n) {
  int16_t* coef = make_table(nt, logph);
  CHECK(sdrfm_pcm_rate_check_coef(coef, nt, logph) == SDRFM_OK);
  int16_t* x = make_row(n);
  const uint32_t hn = 2 * (nt - 1), cap = cap_of(step, n);
  int16_t* hist = (int16_t*)calloc(hn, sizeof(int16_t));
  int16_t* whole = (int16_t*)malloc(sizeof(int16_t) * 2 * cap);
  CHECK(hist && whole);
  uint64_t pos = 0;
  uint32_t n_whole = 0;
  CHECK(sdrfm_pcm_rate_s16(x, n, coef, nt, logph, step, &pos, hist, whole, cap, &n_whole) == SDRFM_OK);
  CHECK(n_whole == (uint32_t)((((uint64_t)n << 32) + step - 1u) / step));
  for (uint32_t cut = 0; cut <= n; ++cut) cut_case(coef, nt, logph, step, x, n, whole, n_whole, pos, hist, cut);
  free(whole);
  free(hist);
  free(x);
  free(coef);
}

static void refusals(void) {
  const uint32_t nt = 8, logph = 4;
  int16_t* coef = make_table(nt, logph);
  int16_t* x = make_row(16);
  int16_t hist[14] = {0}, out[2 * 65];
  uint64_t pos = 0;
  uint32_t got = 0;
  const uint64_t one = (uint64_t)1 << 32;
  CHECK(sdrfm_pcm_rate_s16(x, 16, NULL, nt, logph, one, &pos, hist, out, 65, &got) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_rate_s16(x, 16, coef, nt, logph, one, NULL, hist, out, 65, &got) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_rate_s16(x, 16, coef, nt, logph, one, &pos, NULL, out, 65, &got) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_rate_s16(x, 16, coef, nt, logph, one, &pos, hist, out, 65, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_rate_s16(NULL, 16, coef, nt, logph, one, &pos, hist, out, 65, &got) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_rate_s16(x, 16, coef, nt, logph, one, &pos, hist, NULL, 65, &got) == SDRFM_EINVAL);
  const uint32_t bad_nt[] = {0, 2, 6, 10, 68, 128};
  for (size_t k = 0; k < sizeof(bad_nt) / sizeof(bad_nt[0]); ++k) {
    CHECK(sdrfm_pcm_rate_s16(x, 16, coef, bad_nt[k], logph, one, &pos, hist, out, 65, &got) == SDRFM_EINVAL);
    CHECK(sdrfm_pcm_rate_check_coef(coef, bad_nt[k], logph) == SDRFM_EINVAL);
  }
  const uint32_t bad_ph[] = {0, 3, 9, 32};
  for (size_t k = 0; k < sizeof(bad_ph) / sizeof(bad_ph[0]); ++k) {
    CHECK(sdrfm_pcm_rate_s16(x, 16, coef, nt, bad_ph[k], one, &pos, hist, out, 65, &got) == SDRFM_EINVAL);
    CHECK(sdrfm_pcm_rate_check_coef(coef, nt, bad_ph[k]) == SDRFM_EINVAL);
  }
  const uint64_t bad_step[] = {0, 1, (one >> 2) - 1, (one << 2) + 1, ~(uint64_t)0};
  for (size_t k = 0; k < sizeof(bad_step) / sizeof(bad_step[0]); ++k)
    CHECK(sdrfm_pcm_rate_s16(x, 16, coef, nt, logph, bad_step[k], &pos, hist, out, 65, &got) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_rate_s16(x, (1u << 20) + 1u, coef, nt, logph, one, &pos, hist, out, 65, &got) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_rate_check_coef(NULL, nt, logph) == SDRFM_EINVAL);
  CHECK(pos == 0 && got == 0);
  for (int k = 0; k < 14; ++k) CHECK(hist[k] == 0);
  /* n = 0: nothing out, nothing moves, and no pointer but the state's is looked at */
  CHECK(sdrfm_pcm_rate_s16(NULL, 0, coef, nt, logph, one, &pos, hist, NULL, 0, &got) == SDRFM_OK && got == 0 && pos == 0);
  /* pos ahead of the call: no output, pos comes back by n pairs, the history still moves */
  pos = 5 * one + 3;
  CHECK(sdrfm_pcm_rate_s16(x, 2, coef, nt, logph, one << 2, &pos, hist, NULL, 0, &got) == SDRFM_OK && got == 0 && pos == 3 * one + 3);
  CHECK(memcmp(hist + 10, x, sizeof(int16_t) * 4) == 0 && hist[9] == 0);
  /* the bound, per half row: 65535 passes, 65536 does not, in either half of any row */
  memset(coef, 0, sizeof(int16_t) * 17 * nt);
  coef[0] = 32767; coef[1] = -32767; coef[2] = 1;                /* 65535 in the first half of row 0 */
  coef[16 * nt + 4] = -32768; coef[16 * nt + 5] = 32767;         /* 65535 in the second half of the last row */
  CHECK(sdrfm_pcm_rate_check_coef(coef, nt, logph) == SDRFM_OK);
  coef[3] = -1;
  CHECK(sdrfm_pcm_rate_check_coef(coef, nt, logph) == SDRFM_EINVAL);
  coef[3] = 0; coef[4] = 32767; coef[5] = 32767; coef[6] = 1;     /* the other half of row 0 holds its own 65535 */
  CHECK(sdrfm_pcm_rate_check_coef(coef, nt, logph) == SDRFM_OK);
  coef[16 * nt + 7] = 1;
  CHECK(sdrfm_pcm_rate_check_coef(coef, nt, logph) == SDRFM_EINVAL);
  free(x);
  free(coef);
}

int main(void) {
  const uint64_t one = (uint64_t)1 << 32;
  every_cut(4, 4, one, 9);
  every_cut(8, 4, one >> 2, 21);
  every_cut(8, 5, one << 2, 40);
  every_cut(8, 5, (one << 2) - 1u, 40);
  every_cut(32, 8, one + 429497u, 70);
  every_cut(32, 8, 4674794336ull, 70);
  every_cut(64, 8, one - 429497u, 130);
  refusals();
  printf("ok\n");
  return 0;
}
