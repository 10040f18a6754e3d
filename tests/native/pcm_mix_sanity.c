/* The plain-C host side of the PCM mix bus (csrc/pcm_mix.c) over exactly-sized heap rows and every refusal: a program of its own, built with
 * ASan and UBSan by tests/test_pcm_mix_cpu.py and run as a program.  Prints "ok" at the end. */
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

static int16_t* make_rows(size_t count) {
  int16_t* x = (int16_t*)malloc(sizeof(int16_t) * (count ? count : 1u));   /* (malloc(0) may be NULL) */
  CHECK(x);
  for (size_t k = 0; k < count; ++k) x[k] = (int16_t)(rnd() >> 13);
  return x;
}

static const sdrfm_pcm_mix_rec ZERO = {0, 0, 0, 0};

/* n_in rows of exactly 2n int16 each (stride 2n: the last row ends where the heap block does), one bus whole and in ragged pieces */
static void walk(uint32_t n_in, uint32_t n, uint32_t n_slots, uint32_t slew, const uint16_t* curve) {
  int16_t* x = make_rows((size_t)n_in * 2 * n);
  int16_t* whole = make_rows(2 * (size_t)n);
  int16_t* parts = make_rows(2 * (size_t)n);
  sdrfm_pcm_mix_slot slots[8];
  for (uint32_t k = 0; k < n_slots; ++k) {
    slots[k].src = k % 4 == 2 ? SDRFM_PCM_MIX_NONE : (uint32_t)(rnd() % n_in);
    slots[k].mode = (uint32_t)(rnd() % 5);
    slots[k].g0 = k % 4 == 3 ? 0u : (uint32_t)(rnd() % 32769);
    slots[k].gt = k % 4 == 3 ? 0u : (uint32_t)(rnd() % 32769);
  }
  CHECK(sdrfm_pcm_mix_check_slots(slots, n_slots, n_in) == SDRFM_OK);
  sdrfm_pcm_mix_rec rw = ZERO, rp = ZERO;
  CHECK(sdrfm_pcm_mix_s16(x, 2 * (size_t)n, n_in, n, slots, n_slots, slew, 5, curve, whole, &rw) == SDRFM_OK);
  CHECK(rw.n == n && rw.clipped_l <= n && rw.clipped_r <= n && rw.peak <= 262144);
  static const uint32_t cut[] = {1, 0, 2047, 2050, 3, 700};
  uint32_t at = 0, c = 0;
  while (at < n) {
    uint32_t len = cut[c++ % (sizeof cut / sizeof cut[0])];
    if (len > n - at) len = n - at;
    /* exactly-sized copies of the piece's input and output: a read or a write past the piece is a heap overflow */
    int16_t* px = make_rows((size_t)n_in * 2 * len);
    int16_t* py = make_rows(2 * (size_t)len);
    for (uint32_t r = 0; r < n_in; ++r) memcpy(px + (size_t)r * 2 * len, x + (size_t)r * 2 * n + 2 * (size_t)at, sizeof(int16_t) * 2 * len);
    const uint32_t J = 5u + at > 65536u ? 65536u : 5u + at;
    CHECK(sdrfm_pcm_mix_s16(px, 2 * (size_t)len, n_in, len, slots, n_slots, slew, J, curve, py, &rp) == SDRFM_OK);
    memcpy(parts + 2 * (size_t)at, py, sizeof(int16_t) * 2 * len);
    free(px); free(py);
    at += len;
  }
  CHECK(memcmp(whole, parts, sizeof(int16_t) * 2 * n) == 0 && memcmp(&rw, &rp, sizeof rw) == 0);
  free(x); free(whole); free(parts);
}

/* a dead slot's row is never read: n_in says two rows, the heap block holds one */
static void dead_rows_are_not_read(void) {
  const uint32_t n = 300;
  int16_t* x = make_rows(2 * (size_t)n);
  int16_t* y = make_rows(2 * (size_t)n);
  const sdrfm_pcm_mix_slot slots[3] = {{0, SDRFM_PCM_MIX_STEREO, 32768, 32768}, {1, SDRFM_PCM_MIX_MONO, 0, 0}, {SDRFM_PCM_MIX_NONE, SDRFM_PCM_MIX_SWAP, 32768, 1}};
  sdrfm_pcm_mix_rec r = ZERO;
  CHECK(sdrfm_pcm_mix_s16(x, 2 * (size_t)n, 2, n, slots, 3, 9, 0, NULL, y, &r) == SDRFM_OK);
  CHECK(memcmp(x, y, sizeof(int16_t) * 2 * n) == 0 && r.n == n && r.clipped_l == 0 && r.clipped_r == 0);   /* and unity is the identity */
  free(x); free(y);
}

static void refusals(void) {
  int16_t x[16], y[8], y0[8];
  memset(x, 1, sizeof x); memset(y, 2, sizeof y); memcpy(y0, y, sizeof y);
  uint16_t lin[SDRFM_PCM_MIX_CURVE_LEN], bad[SDRFM_PCM_MIX_CURVE_LEN];
  for (uint32_t j = 0; j < SDRFM_PCM_MIX_CURVE_LEN; ++j) lin[j] = bad[j] = (uint16_t)(256u * j);
  bad[5] = 0;
  sdrfm_pcm_mix_slot s[8];
  for (int k = 0; k < 8; ++k) { s[k].src = 1; s[k].mode = 0; s[k].g0 = 32768; s[k].gt = 0; }
  const sdrfm_pcm_mix_rec r0 = {7, 1, 2, 3};
  sdrfm_pcm_mix_rec r = r0;
#define REFUSED(code, call) do { CHECK((call) == (code)); CHECK(memcmp(&r, &r0, sizeof r) == 0 && memcmp(y, y0, sizeof y) == 0); } while (0)
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, 4, NULL, 2, 1, 0, NULL, y, &r));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, 4, s, 2, 1, 0, NULL, y, NULL));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(NULL, 8, 2, 4, s, 2, 1, 0, NULL, y, &r));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, 4, s, 2, 1, 0, NULL, NULL, &r));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 0, 4, s, 2, 1, 0, NULL, y, &r));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 65537, 4, s, 2, 1, 0, NULL, y, &r));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, 4, s, 0, 1, 0, NULL, y, &r));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, 4, s, 9, 1, 0, NULL, y, &r));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, 4, s, 2, 0, 0, NULL, y, &r));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, 4, s, 2, 32769, 0, NULL, y, &r));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, 4, s, 2, 1, 65537, NULL, y, &r));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, (1u << 20) + 1u, s, 2, 1, 0, NULL, y, &r));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 9, 2, 4, s, 2, 1, 0, NULL, y, &r));
  REFUSED(SDRFM_ECAPACITY, sdrfm_pcm_mix_s16(x, 6, 2, 4, s, 2, 1, 0, NULL, y, &r));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, 4, s, 2, 1, 0, bad, y, &r));
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 1, 4, s, 2, 1, 0, NULL, y, &r));                /* src 1 of one row */
  s[1].mode = 5;
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, 4, s, 2, 1, 0, NULL, y, &r));
  s[1].mode = 0; s[1].g0 = 32769;
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, 4, s, 2, 1, 0, NULL, y, &r));
  s[1].g0 = 0; s[1].gt = 32769;
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, 4, s, 2, 1, 0, NULL, y, &r));
  s[1].gt = 0; s[1].src = 0xFFFFFFFEu;
  REFUSED(SDRFM_EINVAL, sdrfm_pcm_mix_s16(x, 8, 2, 4, s, 2, 1, 0, NULL, y, &r));
  s[1].src = 1;
#undef REFUSED
  /* the edges that are taken: n == 0 with NULL rows, J at its ceiling, the largest slew, a stride that is not looked at for one row */
  CHECK(sdrfm_pcm_mix_s16(NULL, 0, 2, 0, s, 2, 1, 65536, lin, NULL, &r) == SDRFM_OK && memcmp(&r, &r0, sizeof r) == 0);
  for (int k = 0; k < 8; ++k) s[k].src = 0;
  CHECK(sdrfm_pcm_mix_s16(x, 2, 1, 4, s, 8, 32768, 65536, lin, y, &r) == SDRFM_OK && r.n == 11);
  for (int k = 0; k < 8; ++k) CHECK(y[k] == 0);                                                   /* every ramp has reached 0 */
  CHECK(sdrfm_pcm_mix_check_slots(NULL, 1, 1) == SDRFM_EINVAL && sdrfm_pcm_mix_check_slots(s, 0, 1) == SDRFM_OK);
  CHECK(sdrfm_pcm_mix_check_curve(NULL) == SDRFM_EINVAL && sdrfm_pcm_mix_check_curve(bad) == SDRFM_EINVAL && sdrfm_pcm_mix_check_curve(lin) == SDRFM_OK);
  CHECK(sdrfm_pcm_mix_add(NULL, &r) == SDRFM_EINVAL && sdrfm_pcm_mix_add(&r, NULL) == SDRFM_EINVAL);
  sdrfm_pcm_mix_report_t rep;
  CHECK(sdrfm_pcm_mix_report(NULL, &rep) == SDRFM_EINVAL && sdrfm_pcm_mix_report(&r, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_mix_report(&ZERO, &rep) == SDRFM_OK && isnan(rep.peak_dbfs) && isnan(rep.clipped_frac));
  const sdrfm_pcm_mix_rec quiet = {10, 0, 0, 0}, full = {10, 10, 10, 262144};
  CHECK(sdrfm_pcm_mix_report(&quiet, &rep) == SDRFM_OK && isinf(rep.peak_dbfs) && rep.peak_dbfs < 0 && rep.clipped_frac == 0.0);
  CHECK(sdrfm_pcm_mix_report(&full, &rep) == SDRFM_OK && fabs(rep.peak_dbfs - 20.0 * log10(8.0)) < 1e-12 && rep.clipped_frac == 1.0);
}

int main(void) {
  uint16_t eqp[SDRFM_PCM_MIX_CURVE_LEN];
  for (uint32_t j = 0; j < SDRFM_PCM_MIX_CURVE_LEN; ++j) eqp[j] = (uint16_t)lround(32768.0 * sin(3.14159265358979323846 * j / 256.0));
  static const uint32_t ns[] = {0, 1, 2, 3, 2047, 2048, 2049, 4099, 4800};
  for (size_t k = 0; k < sizeof ns / sizeof ns[0]; ++k) {
    walk(1, ns[k], 1, 1, NULL);
    walk(3, ns[k], 2, 7, eqp);
    walk(2, ns[k], 8, 32768, NULL);
    walk(7, ns[k], 3, 3, eqp);
  }
  walk(1, 70000, 2, 1, NULL);                                      /* J past its ceiling inside the run */
  dead_rows_are_not_read();
  refusals();
  printf("ok\n");
  return 0;
}
