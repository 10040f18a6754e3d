/* The plain-C host side of the look-ahead limiter (csrc/limit.c) over its edges and its refusals, on exactly-sized heap rows: a program of its
 * own, built with ASan and UBSan by tests/test_limit_cpu.py and run as a program.  Prints "ok" at the end. */
#include <math.h>
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

static int16_t* make_row(uint32_t n) {
  int16_t* x = (int16_t*)malloc(sizeof(int16_t) * 2 * (n ? n : 1u));   /* (malloc(0) may be NULL) */
  CHECK(x);
  for (uint32_t k = 0; k < 2 * n; ++k) x[k] = (int16_t)(rnd() & 0xFFFFu);
  if (n >= 2) { x[0] = x[1] = -32768; x[2] = x[3] = 32767; }
  return x;
}

static int32_t* make_state(uint32_t lw) {
  const uint32_t words = sdrfm_pcm_limit_state_words(lw);
  int32_t* st = (int32_t*)malloc(sizeof(int32_t) * words);
  CHECK(st && sdrfm_pcm_limit_state_init(lw, st) == SDRFM_OK);
  return st;
}

static const sdrfm_pcm_limit_rec IDENT = {0, 0, 32768, 0};

/* one row whole and in ragged pieces: the same PCM, state and record; every output under the ceiling */
static void walk(uint32_t lw, uint32_t slew, sdrfm_pcm_limit_params p, uint32_t n) {
  const uint32_t words = sdrfm_pcm_limit_state_words(lw);
  int16_t* x = make_row(n);
  int16_t* whole = make_row(n);
  int16_t* parts = make_row(n);
  int32_t* s1 = make_state(lw);
  int32_t* s2 = make_state(lw);
  sdrfm_pcm_limit_rec r1 = IDENT, r2 = IDENT;
  CHECK(sdrfm_pcm_limit_s16(n ? x : NULL, n, lw, slew, 0, &p, s1, n ? whole : NULL, &r1) == SDRFM_OK);
  const uint32_t cuts[] = {1, 0, 2, (1u << lw) - 2u, (1u << lw) - 1u, 1u << lw, 1, 1023, 1024, 1025, 7};
  uint32_t at = 0, J = 0;
  for (uint32_t k = 0; at < n; ++k) {
    uint32_t c = cuts[k % (sizeof(cuts) / sizeof(cuts[0]))];
    if (c > n - at) c = n - at;
    /* an exactly-sized copy of the piece: a read or a write one pair too far is caught */
    int16_t* in = make_row(c);
    int16_t* out = make_row(c);
    memcpy(in, x + 2 * (size_t)at, sizeof(int16_t) * 2 * c);
    CHECK(sdrfm_pcm_limit_s16(c ? in : NULL, c, lw, slew, J, &p, s2, c ? out : NULL, &r2) == SDRFM_OK);
    memcpy(parts + 2 * (size_t)at, out, sizeof(int16_t) * 2 * c);
    free(in);
    free(out);
    at += c;
    J = J + c < 65536u ? J + c : 65536u;
  }
  CHECK(memcmp(whole, parts, sizeof(int16_t) * 2 * n) == 0 && memcmp(s1, s2, sizeof(int32_t) * words) == 0 && memcmp(&r1, &r2, sizeof(r1)) == 0);
  CHECK(r1.n == n && r1.limited <= n && r1.min_gain <= 32768u && (r1.limited ? r1.min_gain < 32768u && r1.at < n : r1.min_gain == 32768u && r1.at == 0));
  for (uint32_t k = 0; k < 2 * n; ++k) CHECK((uint32_t)abs(whole[k]) <= p.ceiling);
  /* in place */
  int32_t* s3 = make_state(lw);
  sdrfm_pcm_limit_rec r3 = IDENT;
  CHECK(sdrfm_pcm_limit_s16(n ? x : NULL, n, lw, slew, 0, &p, s3, n ? x : NULL, &r3) == SDRFM_OK);
  CHECK(memcmp(whole, x, sizeof(int16_t) * 2 * n) == 0 && memcmp(s1, s3, sizeof(int32_t) * words) == 0 && memcmp(&r1, &r3, sizeof(r1)) == 0);
  free(x); free(whole); free(parts); free(s1); free(s2); free(s3);
}

static void refusals(void) {
  const sdrfm_pcm_limit_params good = {29204, 874, 4096, 4096};
  int16_t* x = make_row(8);
  int16_t* y = make_row(8);
  int16_t y0[16];
  memcpy(y0, y, sizeof(y0));
  int32_t* st = make_state(2);
  int32_t st0[12];
  memcpy(st0, st, sizeof(st0));
  sdrfm_pcm_limit_rec acc = {5, 1, 30000, 2}, acc0 = acc;
  sdrfm_pcm_limit_params p = good;
#define REFUSED(call)                                                                                                          \
  do {                                                                                                                         \
    CHECK((call) == SDRFM_EINVAL);                                                                                             \
    CHECK(memcmp(y, y0, sizeof(y0)) == 0 && memcmp(st, st0, sizeof(st0)) == 0 && memcmp(&acc, &acc0, sizeof(acc)) == 0);      \
  } while (0)
  REFUSED(sdrfm_pcm_limit_s16(NULL, 8, 2, 1, 0, &good, st, y, &acc));
  REFUSED(sdrfm_pcm_limit_s16(x, 8, 2, 1, 0, &good, st, NULL, &acc));
  REFUSED(sdrfm_pcm_limit_s16(x, 8, 2, 1, 0, NULL, st, y, &acc));
  REFUSED(sdrfm_pcm_limit_s16(x, 8, 2, 1, 0, &good, NULL, y, &acc));
  REFUSED(sdrfm_pcm_limit_s16(x, 8, 2, 1, 0, &good, st, y, NULL));
  REFUSED(sdrfm_pcm_limit_s16(x, 8, 1, 1, 0, &good, st, y, &acc));
  REFUSED(sdrfm_pcm_limit_s16(x, 8, 9, 1, 0, &good, st, y, &acc));
  REFUSED(sdrfm_pcm_limit_s16(x, 8, 2, 0, 0, &good, st, y, &acc));
  REFUSED(sdrfm_pcm_limit_s16(x, 8, 2, 32769, 0, &good, st, y, &acc));
  REFUSED(sdrfm_pcm_limit_s16(x, 8, 2, 1, 65537, &good, st, y, &acc));
  REFUSED(sdrfm_pcm_limit_s16(x, (1u << 20) + 1u, 2, 1, 0, &good, st, y, &acc));
  p = good; p.ceiling = 0; REFUSED(sdrfm_pcm_limit_s16(x, 8, 2, 1, 0, &p, st, y, &acc));
  p = good; p.ceiling = 32768; REFUSED(sdrfm_pcm_limit_s16(x, 8, 2, 1, 0, &p, st, y, &acc));
  p = good; p.release = 0; REFUSED(sdrfm_pcm_limit_s16(x, 8, 2, 1, 0, &p, st, y, &acc));
  p = good; p.release = (1u << 23) + 1u; REFUSED(sdrfm_pcm_limit_s16(x, 8, 2, 1, 0, &p, st, y, &acc));
  p = good; p.gain0 = 65537; REFUSED(sdrfm_pcm_limit_s16(x, 8, 2, 1, 0, &p, st, y, &acc));
  p = good; p.gain_t = 65537; REFUSED(sdrfm_pcm_limit_s16(x, 8, 2, 1, 0, &p, st, y, &acc));
#undef REFUSED
  /* n = 0 takes NULL rows and leaves everything but the record's n (+ 0) as it was */
  CHECK(sdrfm_pcm_limit_s16(NULL, 0, 2, 1, 65536, &good, st, NULL, &acc) == SDRFM_OK);
  CHECK(memcmp(st, st0, sizeof(st0)) == 0 && memcmp(&acc, &acc0, sizeof(acc)) == 0);
  /* the corners of the ranges are taken */
  p.ceiling = 1; p.release = 1u << 23; p.gain0 = 65536; p.gain_t = 0;
  CHECK(sdrfm_pcm_limit_check_params(&p, 8, 32768) == SDRFM_OK && sdrfm_pcm_limit_check_params(&p, 2, 1) == SDRFM_OK);
  CHECK(sdrfm_pcm_limit_check_params(NULL, 6, 1) == SDRFM_EINVAL && sdrfm_pcm_limit_check_params(&p, 6, 0) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_limit_state_words(1) == 0 && sdrfm_pcm_limit_state_words(9) == 0 && sdrfm_pcm_limit_state_words(2) == 12 &&
        sdrfm_pcm_limit_state_words(8) == 1020);
  CHECK(sdrfm_pcm_limit_state_init(2, NULL) == SDRFM_EINVAL && sdrfm_pcm_limit_state_init(9, st) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_limit_add(NULL, &acc) == SDRFM_EINVAL && sdrfm_pcm_limit_add(&acc, NULL) == SDRFM_EINVAL);
  free(x); free(y); free(st);
}

static void report_and_ceiling(void) {
  sdrfm_pcm_limit_report_t r;
  sdrfm_pcm_limit_rec m = {48000, 12000, 16384, 24000};
  CHECK(sdrfm_pcm_limit_report(&m, 48000.0, &r) == SDRFM_OK);
  CHECK(fabs(r.reduction_db - 20.0 * log10(2.0)) < 1e-12 && r.limited_frac == 0.25 && r.at_seconds == 0.5);
  m.min_gain = 32768; m.limited = 0; m.at = 0;
  CHECK(sdrfm_pcm_limit_report(&m, 48000.0, &r) == SDRFM_OK && r.reduction_db == 0.0 && r.limited_frac == 0.0);
  m.min_gain = 0;
  CHECK(sdrfm_pcm_limit_report(&m, 48000.0, &r) == SDRFM_OK && isinf(r.reduction_db) && r.reduction_db > 0);
  m.n = 0;
  CHECK(sdrfm_pcm_limit_report(&m, 48000.0, &r) == SDRFM_OK && isnan(r.reduction_db) && isnan(r.limited_frac) && isnan(r.at_seconds));
  CHECK(sdrfm_pcm_limit_report(NULL, 48000.0, &r) == SDRFM_EINVAL && sdrfm_pcm_limit_report(&m, 48000.0, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_limit_report(&m, 0.0, &r) == SDRFM_EINVAL && sdrfm_pcm_limit_report(&m, NAN, &r) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_limit_ceiling(-1.0) == 29204u && sdrfm_pcm_limit_ceiling(-2.0) == 26028u && sdrfm_pcm_limit_ceiling(-6.0) == 16422u);
  CHECK(sdrfm_pcm_limit_ceiling(0.0) == 32767u && sdrfm_pcm_limit_ceiling(20.0) == 32767u && sdrfm_pcm_limit_ceiling(-200.0) == 1u);
  CHECK(sdrfm_pcm_limit_ceiling(NAN) == 1u && sdrfm_pcm_limit_ceiling(-INFINITY) == 1u && sdrfm_pcm_limit_ceiling(INFINITY) == 32767u);
}

int main(void) {
  const sdrfm_pcm_limit_params corners[] = {{29204, 874, 4096, 4096}, {1, 1, 65536, 65536}, {32767, 1u << 23, 65536, 65536},
                                            {12000, 5000, 20000, 20000}, {29204, 874, 0, 0}, {20000, 300, 0, 65536}, {20000, 300, 65536, 100}};
  const uint32_t ns[] = {0, 1, 2, 3, 254, 255, 256, 1023, 1024, 1025, 2600};
  for (uint32_t lw = 2; lw <= 8; ++lw)
    for (size_t c = 0; c < sizeof(corners) / sizeof(corners[0]); ++c)
      for (size_t k = 0; k < sizeof(ns) / sizeof(ns[0]); ++k) walk(lw, c & 1 ? 32768u : 3u, corners[c], ns[k]);
  refusals();
  report_and_ceiling();
  printf("ok\n");
  return 0;
}
