/* Drives csrc/scan.c under ASan + UBSan on the CPU: sdrfm_scan_report and sdrfm_scan_meter_add on edge records — no d at all, zero sums,
 * the worst-case sums of the header, negative sums, sums that wrap in the addition — and on refused arguments.  Prints "ok". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/sdrfm.h"

static int all_nan(const sdrfm_scan_report_t* r) {
  return isnan(r->level_dbfs) && isnan(r->freq_err_hz) && isnan(r->dev_rms_hz) && isnan(r->pilot_rms_rad) && isnan(r->pilot_dev_hz) &&
         isnan(r->pilot_frac) && isnan(r->pilot_steadiness);
}

int main(void) {
  sdrfm_scan_meter* m = (sdrfm_scan_meter*)calloc(3, sizeof *m);   /* on the heap: an access past a record is ASan's to see */
  sdrfm_scan_report_t* r = (sdrfm_scan_report_t*)malloc(sizeof *r);
  if (!m || !r) return 1;
  if (sizeof(sdrfm_scan_meter) != 64) return 2;
  /* n = 0: NaNs */
  if (sdrfm_scan_report(&m[0], 2.4e6, 10, 0.98982, r) != SDRFM_OK || !all_nan(r)) return 3;
  /* n > 0, every sum 0: silence */
  m[0].n = 1u << 21;
  if (sdrfm_scan_report(&m[0], 2.4e6, 10, 0.98982, r) != SDRFM_OK) return 4;
  if (!(isinf(r->level_dbfs) && r->level_dbfs < 0) || r->freq_err_hz != 0.0 || r->dev_rms_hz != 0.0 || r->pilot_rms_rad != 0.0 || r->pilot_frac != 0.0 ||
      !isnan(r->pilot_steadiness))
    return 5;
  /* the header's worst case: 2^21 d's of |y| = 2040 sqrt 2, d = -pi, pw = 1270 */
  const uint64_t n = 1u << 21;
  m[1].n = n; m[1].n_pilot = n;
  m[1].rf_q = (int64_t)(n * 2130739200ull);                      /* 8 323 200 * 2^8 */
  m[1].freq_q = -(int64_t)(n * 52707179ull);                     /* pi 2^24 */
  m[1].dev_q = (int64_t)(n * 165584485ull);                      /* pi^2 2^24 */
  m[1].pilot_q = (int64_t)(n * 21307064320ull);                  /* 1270 * 2^24 */
  m[1].pilot2_q = (int64_t)(n * (1612900ull << 20));               /* 1270^2 * 2^20 */
  if (m[1].pilot2_q <= 0 || (uint64_t)m[1].pilot2_q >= (1ull << 62)) return 6;
  if (sdrfm_scan_report(&m[1], 2.4e6, 10, 0.98982, r) != SDRFM_OK) return 7;
  if (fabs(r->freq_err_hz + 120000.0) > 1.0 || r->dev_rms_hz > 100.0 || fabs(r->pilot_steadiness - 1.0) > 1e-6 || r->pilot_frac != 1.0 ||
      fabs(r->pilot_rms_rad - sqrt(1270.0)) > 1e-6 || fabs(r->level_dbfs - 10.0 * log10(8323200.0 / (127.5 * 127.5))) > 1e-9)
    return 8;
  /* the extremes of every field: the report stays finite or NaN, never traps */
  m[2].n = UINT64_MAX; m[2].n_pilot = UINT64_MAX;
  m[2].rf_q = INT64_MIN; m[2].freq_q = INT64_MIN; m[2].dev_q = INT64_MIN; m[2].pilot_q = INT64_MIN; m[2].pilot2_q = INT64_MAX;
  if (sdrfm_scan_report(&m[2], 1.0, UINT32_MAX, 1e-300, r) != SDRFM_OK) return 9;
  /* sums: plain, to zero, and wrapping (defined: two's complement) */
  sdrfm_scan_meter acc;
  memset(&acc, 0, sizeof acc);
  if (sdrfm_scan_meter_add(&acc, &m[1]) != SDRFM_OK || sdrfm_scan_meter_add(&acc, &m[1]) != SDRFM_OK) return 10;
  if (acc.n != 2 * n || acc.freq_q != 2 * m[1].freq_q || acc.pilot2_q != (int64_t)(2 * (uint64_t)m[1].pilot2_q) || acc.reserved != 0) return 11;
  if (sdrfm_scan_meter_add(&acc, &m[2]) != SDRFM_OK || sdrfm_scan_meter_add(&acc, &m[2]) != SDRFM_OK) return 12;
  if (sdrfm_scan_meter_add(&m[2], &m[2]) != SDRFM_OK || m[2].rf_q != 0) return 13;   /* INT64_MIN + INT64_MIN wraps to 0; acc and m may alias */
  /* refusals */
  if (sdrfm_scan_report(NULL, 2.4e6, 10, 1.0, r) != SDRFM_EINVAL || sdrfm_scan_report(&m[0], 2.4e6, 10, 1.0, NULL) != SDRFM_EINVAL) return 14;
  if (sdrfm_scan_report(&m[0], 2.4e6, 0, 1.0, r) != SDRFM_EINVAL || sdrfm_scan_report(&m[0], NAN, 10, 1.0, r) != SDRFM_EINVAL ||
      sdrfm_scan_report(&m[0], -1.0, 10, 1.0, r) != SDRFM_EINVAL || sdrfm_scan_report(&m[0], 2.4e6, 10, 0.0, r) != SDRFM_EINVAL ||
      sdrfm_scan_report(&m[0], INFINITY, 10, 1.0, r) != SDRFM_EINVAL)
    return 15;
  if (sdrfm_scan_meter_add(NULL, &m[0]) != SDRFM_EINVAL || sdrfm_scan_meter_add(&acc, NULL) != SDRFM_EINVAL) return 16;
  free(r);
  free(m);
  printf("ok\n");
  return 0;
}
