/* Drives the histogram side of csrc/scan.c under ASan + UBSan on the CPU: sdrfm_scan_hist_add and sdrfm_scan_hist_report on edge rows — no
 * count at all, one bin, the two extreme bins 54 and 457, the first and the last word of a row, counts at the top of uint32 and of
 * uint64, a record beside the row and one that is not the row's — and on refused arguments.  Prints "ok". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/sdrfm.h"

#define B SDRFM_SCAN_HIST_BINS

static int all_nan(const sdrfm_scan_hist_report_t* r) {
  return isnan(r->centre_hz) && isnan(r->peak_pos_hz) && isnan(r->peak_neg_hz) && isnan(r->peak_hz) && isnan(r->over_min) && isnan(r->over_max) &&
         isnan(r->mpx_power_dbr);
}

int main(void) {
  /* on the heap and exactly a row long: an access past a row is ASan's to see */
  uint64_t* acc = (uint64_t*)calloc(B, sizeof *acc);
  uint32_t* row = (uint32_t*)calloc(B, sizeof *row);
  sdrfm_scan_meter* m = (sdrfm_scan_meter*)calloc(1, sizeof *m);
  sdrfm_scan_hist_report_t* r = (sdrfm_scan_hist_report_t*)malloc(sizeof *r);
  if (!acc || !row || !m || !r) return 1;
  if (sizeof(sdrfm_scan_hist_report_t) != 64 || B != 512) return 2;
  const double hz = 2.4e6 / (2.0 * 3.14159265358979323846 * 10.0);
  /* no count: NaNs, with and without a record */
  if (sdrfm_scan_hist_report(acc, NULL, 2.4e6, 10, 75e3, r) != SDRFM_OK || r->n != 0 || !all_nan(r)) return 3;
  if (sdrfm_scan_hist_report(acc, m, 2.4e6, 10, 75e3, r) != SDRFM_OK || r->n != 0 || !all_nan(r)) return 4;
  /* one bin */
  row[256] = 1u << 21;
  if (sdrfm_scan_hist_add(acc, row) != SDRFM_OK || acc[256] != (1u << 21)) return 5;
  if (sdrfm_scan_hist_report(acc, NULL, 2.4e6, 10, 75e3, r) != SDRFM_OK || r->n != (1u << 21)) return 6;
  if (fabs(r->centre_hz - hz / 128.0) > 1e-9 || fabs(r->peak_hz - hz / 128.0) > 1e-6 || r->over_max != 0.0 || !isnan(r->mpx_power_dbr)) return 7;
  m->n = 1u << 21;                                                /* d = 0 throughout: centre 0, no deviation */
  if (sdrfm_scan_hist_report(acc, m, 2.4e6, 10, 0.0, r) != SDRFM_OK) return 8;
  if (r->centre_hz != 0.0 || r->peak_neg_hz != 0.0 || r->over_min != 0.0 || r->over_max != 1.0 || !(isinf(r->mpx_power_dbr) && r->mpx_power_dbr < 0)) return 9;
  /* the two extreme bins, and the first and the last word of a row, at the top of uint32 */
  memset(row, 0, B * sizeof *row);
  row[54] = row[457] = row[0] = row[B - 1] = UINT32_MAX;
  for (int k = 0; k < 3; ++k)
    if (sdrfm_scan_hist_add(acc, row) != SDRFM_OK) return 10;
  if (acc[0] != 3ull * UINT32_MAX || acc[B - 1] != 3ull * UINT32_MAX || acc[54] != acc[457]) return 11;
  if (sdrfm_scan_hist_report(acc, NULL, 2.4e6, 10, 75e3, r) != SDRFM_OK || r->n != 12ull * UINT32_MAX + (1u << 21)) return 12;
  if (fabs(r->peak_pos_hz + r->centre_hz - 4.0 * hz) > 1e-6 || fabs(r->peak_neg_hz + r->centre_hz + 4.0 * hz) > 1e-6 || !(r->over_min > 0.99)) return 13;
  m->n = r->n; m->freq_q = INT64_MIN; m->dev_q = INT64_MAX;
  if (sdrfm_scan_hist_report(acc, m, 2.4e6, 10, 75e3, r) != SDRFM_OK) return 14;
  m->freq_q = INT64_MAX; m->dev_q = INT64_MIN;
  if (sdrfm_scan_hist_report(acc, m, 1.0, UINT32_MAX, 1e300, r) != SDRFM_OK || r->over_max != 0.0) return 15;
  /* counts at the top of uint64: the sum wraps (defined: unsigned), the report stays finite or NaN, never traps */
  for (uint32_t b = 0; b < B; ++b) acc[b] = UINT64_MAX;
  if (sdrfm_scan_hist_add(acc, row) != SDRFM_OK || acc[54] != (uint64_t)UINT32_MAX - 1u) return 16;
  if (sdrfm_scan_hist_report(acc, NULL, 2.4e6, 10, 75e3, r) != SDRFM_OK) return 17;
  /* refusals */
  if (sdrfm_scan_hist_add(NULL, row) != SDRFM_EINVAL || sdrfm_scan_hist_add(acc, NULL) != SDRFM_EINVAL) return 18;
  if (sdrfm_scan_hist_report(NULL, NULL, 2.4e6, 10, 75e3, r) != SDRFM_EINVAL || sdrfm_scan_hist_report(acc, NULL, 2.4e6, 10, 75e3, NULL) != SDRFM_EINVAL) return 19;
  if (sdrfm_scan_hist_report(acc, NULL, 2.4e6, 0, 75e3, r) != SDRFM_EINVAL || sdrfm_scan_hist_report(acc, NULL, NAN, 10, 75e3, r) != SDRFM_EINVAL ||
      sdrfm_scan_hist_report(acc, NULL, -1.0, 10, 75e3, r) != SDRFM_EINVAL || sdrfm_scan_hist_report(acc, NULL, INFINITY, 10, 75e3, r) != SDRFM_EINVAL ||
      sdrfm_scan_hist_report(acc, NULL, 2.4e6, 10, -1.0, r) != SDRFM_EINVAL || sdrfm_scan_hist_report(acc, NULL, 2.4e6, 10, NAN, r) != SDRFM_EINVAL)
    return 20;
  m->n = 7;                                                       /* not the row's */
  if (sdrfm_scan_hist_report(acc, m, 2.4e6, 10, 75e3, r) != SDRFM_EINVAL) return 21;
  free(r);
  free(m);
  free(row);
  free(acc);
  printf("ok\n");
  return 0;
}
