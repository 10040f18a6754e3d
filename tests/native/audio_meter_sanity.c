/* The plain-C host side of the audio meter (csrc/audio_meter.c) under ASan and UBSan, a program of its own: the routine on edge
 * rows (none, one pair, the rails, exactly-sized heap rows so that a read past 2n is caught), additivity over every cut of a row, the join on
 * records with sums near 2^62 and beyond (wrap-around is defined), the report's NaN and -inf cases, and every refusal. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/sdrfm.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { ++fails; printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

int main(void) {
  sdrfm_audio_meter zero, a, b;
  sdrfm_audio_report_t rep;
  memset(&zero, 0, sizeof(zero));
  CHECK(sizeof(sdrfm_audio_meter) == 192 && sizeof(sdrfm_audio_runs) == 32);

  /* refusals */
  a = zero;
  int16_t one[2] = {5, -5};
  CHECK(sdrfm_pcm_audio_meter_s16(one, 1, 0, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_audio_meter_s16(NULL, 1, 0, &a) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_audio_meter_s16(one, 1, 32768, &a) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_audio_meter_s16(one, 1, 0xFFFFFFFFu, &a) == SDRFM_EINVAL);
  CHECK(!memcmp(&a, &zero, sizeof(a)));
  CHECK(sdrfm_pcm_audio_meter_s16(NULL, 0, 0, &a) == SDRFM_OK && !memcmp(&a, &zero, sizeof(a)));
  CHECK(sdrfm_audio_meter_add(NULL, &a) == SDRFM_EINVAL && sdrfm_audio_meter_add(&a, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_audio_meter_report(NULL, 48000.0, &rep) == SDRFM_EINVAL && sdrfm_audio_meter_report(&a, 48000.0, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_audio_meter_report(&a, 0.0, &rep) == SDRFM_EINVAL && sdrfm_audio_meter_report(&a, -1.0, &rep) == SDRFM_EINVAL);
  CHECK(sdrfm_audio_meter_report(&a, NAN, &rep) == SDRFM_EINVAL && sdrfm_audio_meter_report(&a, INFINITY, &rep) == SDRFM_EINVAL);

  /* n = 0: every field NaN */
  CHECK(sdrfm_audio_meter_report(&zero, 48000.0, &rep) == SDRFM_OK);
  for (size_t k = 0; k < sizeof(rep) / sizeof(double); ++k) CHECK(isnan(((double*)&rep)[k]));

  /* the rails on an exactly-sized heap row */
  for (uint32_t n = 1; n <= 70; n += 23) {
    int16_t* p = (int16_t*)malloc(sizeof(int16_t) * 2 * n);
    for (uint32_t i = 0; i < n; ++i) { p[2 * i] = -32768; p[2 * i + 1] = 32767; }
    a = zero;
    CHECK(sdrfm_pcm_audio_meter_s16(p, n, 32767, &a) == SDRFM_OK);
    CHECK(a.n == n && a.sum_l == -32768 * (int64_t)n && a.sum_r == 32767 * (int64_t)n && a.sq_l == ((uint64_t)n << 30));
    CHECK(a.cross == -(int64_t)32768 * 32767 * n && a.peak_l == 32768 && a.peak_r == 32767 && a.clip_l == n && a.clip_r == n);
    CHECK(a.quiet_l.count == 0 && a.quiet_l.longest == 0 && a.quiet_r.count == n && a.quiet_r.lead == n && a.quiet_r.trail == n && a.quiet_both.count == 0);
    CHECK(sdrfm_audio_meter_report(&a, 48000.0, &rep) == SDRFM_OK);
    CHECK(rep.peak_l_dbfs == 0.0 && rep.rms_l_dbfs == 0.0 && rep.rail_l == 1.0 && rep.rail_r == 1.0 && rep.correlation < -0.999999);
    CHECK(rep.longest_r_s == (double)n / 48000.0 && rep.quiet_r == 1.0 && rep.quiet_l == 0.0);
    free(p);
  }

  /* additivity: every cut of a row with a run across the cut */
  {
    enum { N = 41 };
    int16_t* p = (int16_t*)malloc(sizeof(int16_t) * 2 * N);
    for (int i = 0; i < N; ++i) { p[2 * i] = (i >= 9 && i < 30) ? (int16_t)(i % 3 - 1) : (int16_t)(1000 + i); p[2 * i + 1] = (i % 7 < 5) ? 0 : -2000; }
    sdrfm_audio_meter whole = zero;
    CHECK(sdrfm_pcm_audio_meter_s16(p, N, 1, &whole) == SDRFM_OK);
    CHECK(whole.quiet_l.longest == 21 && whole.quiet_l.lead == 0 && whole.quiet_l.trail == 0 && whole.quiet_l.count == 21);
    for (int c1 = 0; c1 <= N; ++c1)
      for (int c2 = c1; c2 <= N; c2 += 5) {
        a = zero;
        CHECK(sdrfm_pcm_audio_meter_s16(p, (uint32_t)c1, 1, &a) == SDRFM_OK);
        CHECK(sdrfm_pcm_audio_meter_s16(p + 2 * c1, (uint32_t)(c2 - c1), 1, &a) == SDRFM_OK);
        b = zero;
        CHECK(sdrfm_pcm_audio_meter_s16(p + 2 * c2, (uint32_t)(N - c2), 1, &b) == SDRFM_OK);
        CHECK(sdrfm_audio_meter_add(&a, &b) == SDRFM_OK);
        CHECK(!memcmp(&a, &whole, sizeof(a)));
      }
    free(p);
  }

  /* sums near 2^62 add exactly; beyond 2^63 they wrap and nothing is undefined */
  a = zero; b = zero;
  a.n = b.n = (uint64_t)1 << 31;
  a.sum_l = b.sum_l = -((int64_t)1 << 46); a.sq_l = b.sq_l = (uint64_t)1 << 61; a.cross = b.cross = -((int64_t)1 << 61);
  a.quiet_l.count = a.quiet_l.lead = a.quiet_l.trail = a.quiet_l.longest = a.n;
  b.quiet_l.count = b.quiet_l.lead = b.quiet_l.trail = b.quiet_l.longest = b.n;
  CHECK(sdrfm_audio_meter_add(&a, &b) == SDRFM_OK);
  CHECK(a.n == ((uint64_t)1 << 32) && a.sum_l == -((int64_t)1 << 47) && a.sq_l == ((uint64_t)1 << 62) && a.cross == -((int64_t)1 << 62));
  CHECK(a.quiet_l.lead == a.n && a.quiet_l.trail == a.n && a.quiet_l.longest == a.n && a.quiet_l.count == a.n);
  b = a;
  CHECK(sdrfm_audio_meter_add(&a, &b) == SDRFM_OK && sdrfm_audio_meter_add(&a, &b) == SDRFM_OK);   /* -3 x 2^62 wraps */
  CHECK(a.cross == (int64_t)((uint64_t)3 * (uint64_t)(-((int64_t)1 << 62))));

  /* the report: zero power is -inf dB and has no correlation */
  a = zero;
  int16_t quiet[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  CHECK(sdrfm_pcm_audio_meter_s16(quiet, 4, 0, &a) == SDRFM_OK && sdrfm_audio_meter_report(&a, 8000.0, &rep) == SDRFM_OK);
  CHECK(isinf(rep.rms_l_dbfs) && rep.rms_l_dbfs < 0 && isinf(rep.peak_r_dbfs) && isnan(rep.correlation) && isinf(rep.mid_dbfs) && isnan(rep.side_mid_db));
  CHECK(rep.trail_both_s == 4.0 / 8000.0 && rep.longest_both_s == 4.0 / 8000.0 && rep.quiet_both == 1.0 && rep.dc_l == 0.0);
  int16_t lonly[4] = {100, 0, -100, 0};
  a = zero;
  CHECK(sdrfm_pcm_audio_meter_s16(lonly, 2, 0, &a) == SDRFM_OK && sdrfm_audio_meter_report(&a, 8000.0, &rep) == SDRFM_OK);
  CHECK(isnan(rep.correlation) && rep.side_mid_db == 0.0 && isinf(rep.rms_r_dbfs) && fabs(rep.rms_l_dbfs - 20.0 * log10(100.0 / 32768.0)) < 1e-12);
  int16_t anti[4] = {100, -100, -300, 300};
  a = zero;
  CHECK(sdrfm_pcm_audio_meter_s16(anti, 2, 0, &a) == SDRFM_OK && sdrfm_audio_meter_report(&a, 8000.0, &rep) == SDRFM_OK);
  CHECK(rep.correlation == -1.0 && isinf(rep.mid_dbfs) && isinf(rep.side_mid_db) && rep.side_mid_db > 0);

  if (fails) { printf("%d failures\n", fails); return 1; }
  printf("ok\n");
  return 0;
}
