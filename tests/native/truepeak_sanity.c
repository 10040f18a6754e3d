/* The plain-C host side of the true-peak meter (csrc/truepeak.c) walked over its edges as a program of its own, built with ASan and UBSan
 * (tests/test_truepeak_cpu.py): the default table and its symmetries, the bound's edges, every refusal with nothing written, calls shorter than
 * the history, a cut into calls against one call, the limit's rounding and clamping, and the report. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/sdrfm.h"

static int fails = 0;
#define CHECK(c)                                                                  \
  do {                                                                            \
    if (!(c)) {                                                                   \
      if (++fails < 20) printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);     \
    }                                                                             \
  } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rng(void) {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

int main(void) {
  /* the default table */
  int16_t def[48];
  uint32_t P = 0, NT = 0;
  CHECK(sdrfm_truepeak_default_coef(NULL, &P, &NT) == SDRFM_EINVAL && P == 0 && NT == 0);
  CHECK(sdrfm_truepeak_default_coef(def, &P, &NT) == SDRFM_OK && P == 4 && NT == 12);
  CHECK(sdrfm_truepeak_default_coef(def, NULL, NULL) == SDRFM_OK);
  for (int k = 0; k < 12; ++k) CHECK(def[k] == def[36 + 11 - k] && def[12 + k] == def[24 + 11 - k] && def[k] % 4 == 0 && def[12 + k] % 4 == 0);
  CHECK(def[6] == 4 * 7964 && def[12] == 4 * -239 && def[47] == 4 * 14);
  CHECK(sdrfm_truepeak_check_coef(def, 4, 12) == SDRFM_OK);

  /* the bound's edges, in either half; shapes */
  int16_t* tab = (int16_t*)calloc(8 * 64, sizeof(int16_t));      /* the heap: ASan sees a read beyond P * NT */
  if (!tab) return 2;
  CHECK(sdrfm_truepeak_check_coef(NULL, 4, 12) == SDRFM_EINVAL);
  for (uint32_t p = 0; p <= 9; ++p)
    for (uint32_t nt = 0; nt <= 70; ++nt) {
      const int ok = (p == 2 || p == 4 || p == 8) && nt >= 4 && nt <= 64 && nt % 4 == 0;
      if (p * nt <= 8 * 64) CHECK(sdrfm_truepeak_check_coef(tab, p, nt) == (ok ? SDRFM_OK : SDRFM_EINVAL));
    }
  for (int h = 0; h < 2; ++h) {
    memset(tab, 0, 8 * 64 * sizeof(int16_t));
    int16_t* row = tab + 3 * 8 + h * 4;                           /* row 3 of [4][8] */
    row[0] = -32768; row[1] = 32767;
    CHECK(sdrfm_truepeak_check_coef(tab, 4, 8) == SDRFM_OK);     /* 65535 */
    row[2] = -1;
    CHECK(sdrfm_truepeak_check_coef(tab, 4, 8) == SDRFM_EINVAL); /* 65536 */
    row[2] = 0; row[3] = 1;
    CHECK(sdrfm_truepeak_check_coef(tab, 4, 8) == SDRFM_EINVAL);
  }
  free(tab);

  /* the limit */
  CHECK(sdrfm_truepeak_limit(0.0) == (uint64_t)1 << 30 && sdrfm_truepeak_limit(NAN) == 0 && sdrfm_truepeak_limit(-INFINITY) == 0);
  CHECK(sdrfm_truepeak_limit(INFINITY) == 0xFFFFFFFFull && sdrfm_truepeak_limit(100.0) == 0xFFFFFFFFull && sdrfm_truepeak_limit(-1000.0) == 0);
  CHECK(sdrfm_truepeak_limit(-1.0) == (uint64_t)floor(1073741824.0 * pow(10.0, -0.05)) && sdrfm_truepeak_limit(-1.0) == 956973407ull);
  CHECK(sdrfm_truepeak_limit(20.0 * log10(4.0)) >= 0xFFFFFFFEull);

  /* refusals write nothing */
  int16_t pcm[2 * 40], hist[2 * 11], hist0[2 * 11];
  for (int k = 0; k < 80; ++k) pcm[k] = (int16_t)(rng() & 0xFFFFu);
  for (int k = 0; k < 22; ++k) hist0[k] = hist[k] = (int16_t)(k - 7);
  sdrfm_truepeak acc, acc0;
  memset(&acc, 0, sizeof(acc));
  acc.n = 5; acc.peak_l = 9; acc.at_l = 2;
  acc0 = acc;
  CHECK(sdrfm_pcm_truepeak_s16(pcm, 40, def, 4, 12, 0, hist, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_truepeak_s16(NULL, 40, def, 4, 12, 0, hist, &acc) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_truepeak_s16(pcm, 40, NULL, 4, 12, 0, hist, &acc) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_truepeak_s16(pcm, 40, def, 4, 12, 0, NULL, &acc) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_truepeak_s16(pcm, 40, def, 3, 12, 0, hist, &acc) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_truepeak_s16(pcm, 40, def, 4, 10, 0, hist, &acc) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_truepeak_s16(pcm, 40, def, 4, 68, 0, hist, &acc) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_truepeak_s16(pcm, 40, def, 4, 12, 0x100000000ull, hist, &acc) == SDRFM_EINVAL);
  CHECK(memcmp(&acc, &acc0, sizeof(acc)) == 0 && memcmp(hist, hist0, sizeof(hist)) == 0);
  CHECK(sdrfm_pcm_truepeak_s16(NULL, 0, def, 4, 12, 0xFFFFFFFFull, hist, &acc) == SDRFM_OK);   /* no pairs: nothing moves */
  CHECK(memcmp(&acc, &acc0, sizeof(acc)) == 0 && memcmp(hist, hist0, sizeof(hist)) == 0);
  CHECK(sdrfm_truepeak_add(NULL, &acc) == SDRFM_EINVAL && sdrfm_truepeak_add(&acc, NULL) == SDRFM_EINVAL);

  /* a cut into calls, some shorter than the history, against one call; exactly sized buffers on the heap */
  const uint32_t cuts[9] = {1, 0, 11, 3, 12, 2, 10, 1, 0};
  uint32_t total = 0;
  for (int k = 0; k < 9; ++k) total += cuts[k];
  sdrfm_truepeak whole, parts;
  memset(&whole, 0, sizeof(whole));
  parts = whole;
  int16_t* hw = (int16_t*)calloc(22, sizeof(int16_t));
  int16_t* hp = (int16_t*)calloc(22, sizeof(int16_t));
  if (!hw || !hp) return 2;
  CHECK(total == 40 && sdrfm_pcm_truepeak_s16(pcm, 40, def, 4, 12, 1u << 29, hw, &whole) == SDRFM_OK);
  uint32_t at = 0;
  for (int k = 0; k < 9; ++k) {
    int16_t* piece = (int16_t*)malloc(2 * cuts[k] * sizeof(int16_t) + 1);
    if (!piece) return 2;
    memcpy(piece, pcm + 2 * at, 2 * cuts[k] * sizeof(int16_t));
    CHECK(sdrfm_pcm_truepeak_s16(cuts[k] ? piece : NULL, cuts[k], def, 4, 12, 1u << 29, hp, &parts) == SDRFM_OK);
    free(piece);
    at += cuts[k];
  }
  CHECK(memcmp(&whole, &parts, sizeof(whole)) == 0 && memcmp(hw, hp, 22 * sizeof(int16_t)) == 0);
  CHECK(memcmp(hw, pcm + 80 - 22, 22 * sizeof(int16_t)) == 0 && whole.n == 40 && whole.peak_l > 0 && whole.reserved == 0);
  free(hw);
  free(hp);

  /* the 32-bit trap: phase 1's whole row lined up with matching signs at the rails passes 2^31 (and one value of another phase beside it) */
  int16_t trap[2 * 16], ht[22];
  memset(trap, 0, sizeof(trap));
  memset(ht, 0, sizeof(ht));
  for (int i = 0; i < 12; ++i) trap[2 * i] = def[12 + 11 - i] >= 0 ? 32767 : -32768;
  sdrfm_truepeak t;
  memset(&t, 0, sizeof(t));
  CHECK(sdrfm_pcm_truepeak_s16(trap, 16, def, 4, 12, 0x7FFFFFFFull, ht, &t) == SDRFM_OK);
  CHECK(t.peak_l == 2171945028ull && t.at_l == 11 && t.peak_r == 0 && t.at_r == 0 && t.over_l == 2 && t.over_r == 0);

  /* the report */
  sdrfm_truepeak_report_t rep;
  CHECK(sdrfm_truepeak_report(NULL, 4, 48000.0, &rep) == SDRFM_EINVAL && sdrfm_truepeak_report(&t, 4, 48000.0, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_truepeak_report(&t, 3, 48000.0, &rep) == SDRFM_EINVAL && sdrfm_truepeak_report(&t, 4, 0.0, &rep) == SDRFM_EINVAL);
  CHECK(sdrfm_truepeak_report(&t, 4, NAN, &rep) == SDRFM_EINVAL);
  CHECK(sdrfm_truepeak_report(&t, 4, 48000.0, &rep) == SDRFM_OK);
  CHECK(fabs(rep.dbtp_l - 20.0 * log10(2171945028.0 / 1073741824.0)) < 1e-12 && rep.dbtp_r == -INFINITY && rep.dbtp == rep.dbtp_l);
  CHECK(rep.over_frac_l == 2.0 / 64.0 && rep.over_frac_r == 0.0 && rep.at_seconds_l == 11.0 / 48000.0 && rep.at_seconds_r == 0.0);
  memset(&t, 0, sizeof(t));
  CHECK(sdrfm_truepeak_report(&t, 8, 48000.0, &rep) == SDRFM_OK && isnan(rep.dbtp) && isnan(rep.over_frac_l) && isnan(rep.at_seconds_r));
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("ok\n");
  return 0;
}
