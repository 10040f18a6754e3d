/* The plain-C host side of the raw-capture IQ meter (csrc/iq_meter.c) over exactly-sized heap rows and every refusal: a program of its own, built
 * with ASan and UBSan by tests/test_iq_meter_cpu.py and run as a program.  Prints "ok" at the end. */
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

static uint8_t* make_row(size_t nbytes, int fill) {
  uint8_t* x = (uint8_t*)malloc(nbytes ? nbytes : 1u);            /* (malloc(0) may be NULL) */
  CHECK(x);
  for (size_t k = 0; k < nbytes; ++k) x[k] = fill >= 0 ? (uint8_t)fill : (uint8_t)(rnd() >> 11);
  return x;
}

static int same(const sdrfm_iq_meter* a, const sdrfm_iq_meter* b) { return memcmp(a, b, sizeof *a) == 0; }

/* the four ties between a record and its row */
static void ties(const sdrfm_iq_meter* m, const uint64_t* h) {
  uint64_t n[2] = {0, 0}, s[2] = {0, 0}, s2[2] = {0, 0};
  for (int c = 0; c < 2; ++c)
    for (uint64_t b = 0; b < 256; ++b) { n[c] += h[256 * c + b]; s[c] += b * h[256 * c + b]; s2[c] += b * b * h[256 * c + b]; }
  CHECK(n[0] == m->n && n[1] == m->n && s[0] == m->sum_i && s[1] == m->sum_q && s2[0] == m->sum_ii && s2[1] == m->sum_qq);
  CHECK(h[0] + h[255] == m->rail_i && h[256] + h[511] == m->rail_q);
}

/* one row whole and in ragged even pieces, 0 and 2 bytes among them: the same record and row */
static void walk(size_t nbytes, int fill) {
  uint8_t* x = make_row(nbytes, fill);
  sdrfm_iq_meter whole, parts, piece;
  uint64_t hw[SDRFM_IQ_HIST_BINS], hp[SDRFM_IQ_HIST_BINS];
  memset(&whole, 0, sizeof whole); memset(&parts, 0, sizeof parts);
  memset(hw, 0, sizeof hw); memset(hp, 0, sizeof hp);
  CHECK(sdrfm_iq_meter_u8(x, nbytes, &whole, hw) == SDRFM_OK);
  CHECK(whole.n == nbytes / 2);
  ties(&whole, hw);
  static const size_t cut[] = {2, 0, 16, 4098, 6, 0, 1022};
  size_t at = 0, k = 0;
  while (at < nbytes) {
    size_t c = cut[k++ % (sizeof cut / sizeof cut[0])];
    if (c > nbytes - at) c = nbytes - at;
    uint8_t* p = make_row(c, 0);                                   /* an exactly-sized copy: a read past the piece is a heap overflow */
    memcpy(p, x + at, c);
    memset(&piece, 0, sizeof piece);
    CHECK(sdrfm_iq_meter_u8(c ? p : NULL, c, &piece, NULL) == SDRFM_OK);
    CHECK(sdrfm_iq_meter_u8(c ? p : NULL, c, &piece, hp) == SDRFM_OK);   /* twice onto piece: n doubles */
    CHECK(piece.n == c);
    piece.n /= 2; piece.sum_i /= 2; piece.sum_q /= 2; piece.sum_ii /= 2; piece.sum_qq /= 2; piece.sum_iq /= 2; piece.rail_i /= 2; piece.rail_q /= 2;
    CHECK(sdrfm_iq_meter_add(&parts, &piece) == SDRFM_OK);
    free(p);
    at += c;
  }
  CHECK(same(&whole, &parts) && memcmp(hw, hp, sizeof hw) == 0);
  if (fill >= 0 && nbytes) {
    const uint64_t n = nbytes / 2, f = (uint64_t)fill;
    CHECK(whole.sum_i == n * f && whole.sum_q == n * f && whole.sum_ii == n * f * f && whole.sum_iq == n * f * f);
    CHECK(whole.rail_i == ((fill == 0 || fill == 255) ? n : 0));
    sdrfm_iq_report_t r;
    CHECK(sdrfm_iq_meter_report(&whole, &r) == SDRFM_OK);
    CHECK(r.dc_i == (double)fill - 127.5 && r.rms_dbfs == -INFINITY && isnan(r.gain_db) && isnan(r.skew_rad) && isnan(r.image_rejection_db));
    CHECK(isfinite(r.total_dbfs));
  }
  uint32_t row[SDRFM_IQ_HIST_BINS];
  uint64_t acc[SDRFM_IQ_HIST_BINS];
  for (uint32_t b = 0; b < SDRFM_IQ_HIST_BINS; ++b) { row[b] = (uint32_t)hw[b]; acc[b] = hw[b]; }
  CHECK(sdrfm_iq_hist_add(acc, row) == SDRFM_OK);
  for (uint32_t b = 0; b < SDRFM_IQ_HIST_BINS; ++b) CHECK(acc[b] == 2 * hw[b]);
  sdrfm_iq_hist_report_t hr;
  CHECK(sdrfm_iq_hist_report(hw, &hr) == SDRFM_OK && hr.n == nbytes / 2);
  if (nbytes) CHECK(hr.peak_i >= hr.level999_i && hr.level999_i >= 1.0 / 255.0 && hr.codes_i >= 1.0 && hr.headroom_db_q >= 0.0);
  else CHECK(isnan(hr.peak_i) && isnan(hr.headroom_db_q) && isnan(hr.codes_i));
  free(x);
}

static void refusals(void) {
  uint8_t* x = make_row(4, -1);
  sdrfm_iq_meter m, z;
  uint64_t h[SDRFM_IQ_HIST_BINS];
  uint32_t row[SDRFM_IQ_HIST_BINS];
  memset(&m, 0, sizeof m); memset(&z, 0, sizeof z); memset(h, 0, sizeof h); memset(row, 0, sizeof row);
  CHECK(sdrfm_iq_meter_u8(x, 4, NULL, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_iq_meter_u8(NULL, 4, &m, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_iq_meter_u8(x, 3, &m, h) == SDRFM_EODD);
  CHECK(same(&m, &z) && h[x[0]] == 0);                             /* nothing touched */
  CHECK(sdrfm_iq_meter_u8(NULL, 0, &m, NULL) == SDRFM_OK && same(&m, &z));
  CHECK(sdrfm_iq_meter_add(NULL, &m) == SDRFM_EINVAL && sdrfm_iq_meter_add(&m, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_iq_hist_add(NULL, row) == SDRFM_EINVAL && sdrfm_iq_hist_add(h, NULL) == SDRFM_EINVAL);
  sdrfm_iq_report_t r;
  sdrfm_iq_hist_report_t hr;
  CHECK(sdrfm_iq_meter_report(NULL, &r) == SDRFM_EINVAL && sdrfm_iq_meter_report(&m, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_iq_hist_report(NULL, &hr) == SDRFM_EINVAL && sdrfm_iq_hist_report(h, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_iq_meter_report(&z, &r) == SDRFM_OK && isnan(r.dc_i) && isnan(r.rms_dbfs) && isnan(r.rail_share_q) && isnan(r.image_rejection_db));
  m.n = 2; m.sum_i = 400; m.sum_ii = 10;                           /* a record no capture gives: the variance would be negative */
  CHECK(sdrfm_iq_meter_report(&m, &r) == SDRFM_EINVAL);
  h[3] = 1;                                                        /* the halves differ */
  CHECK(sdrfm_iq_hist_report(h, &hr) == SDRFM_EINVAL);
  /* the largest record sums that a caller can accumulate still give finite moments: n = 2^40 pairs of alternating rails */
  memset(&m, 0, sizeof m);
  m.n = 1ull << 40; m.sum_i = m.sum_q = (1ull << 39) * 255u; m.sum_ii = m.sum_qq = (1ull << 39) * 65025u; m.sum_iq = (1ull << 39) * 65025u;
  m.rail_i = m.rail_q = m.n;
  CHECK(sdrfm_iq_meter_report(&m, &r) == SDRFM_OK);
  CHECK(r.dc_i == 0.0 && fabs(r.rms_dbfs - 10.0 * log10(2.0)) < 1e-12 && r.rail_share_i == 1.0 && fabs(r.gain_db) < 1e-12);
  CHECK(fabs(r.skew_rad - asin(1.0)) < 1e-12);
  free(x);
}

int main(void) {
  static const size_t sizes[] = {0, 2, 4, 14, 16, 18, 4094, 4096, 4098, 131072, 100002};
  for (size_t k = 0; k < sizeof sizes / sizeof sizes[0]; ++k) {
    walk(sizes[k], -1);
    walk(sizes[k], 0);
    walk(sizes[k], 255);
    walk(sizes[k], 128);
  }
  refusals();
  printf("ok\n");
  return 0;
}
