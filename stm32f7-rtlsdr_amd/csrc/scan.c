/*
 * scan.c — the host side of the scan handle's records (include/sdrfm.h), plain C99 with no GPU behind it: what a
 * sdrfm_scan_meter says in physical units (sdrfm_scan_report) and the exact sum of records (sdrfm_scan_meter_add); and of its deviation
 * histograms: the exact sum of rows (sdrfm_scan_hist_add) and what a histogram says about peak deviation and the share of
 * the time beyond a limit (sdrfm_scan_hist_report).
 */
#include <math.h>
#include <stddef.h>

#include "../../include/sdrfm.h"

static int positive(double v) { return isfinite(v) && v > 0.0; }

int sdrfm_scan_report(const sdrfm_scan_meter* m, double fs, uint32_t D, double pilot_gain, sdrfm_scan_report_t* out) {
  if (!m || !out || !D || !positive(fs) || !positive(pilot_gain)) return SDRFM_EINVAL;
  if (m->n == 0) {
    out->level_dbfs = out->freq_err_hz = out->dev_rms_hz = out->pilot_rms_rad = out->pilot_dev_hz = out->pilot_frac = out->pilot_steadiness = NAN;
    return SDRFM_OK;
  }
  const double n = (double)m->n, hz = fs / (2.0 * 3.14159265358979323846 * (double)D);
  const double sp = ldexp((double)m->rf_q, -8), sd = ldexp((double)m->freq_q, -24), se = ldexp((double)m->dev_q, -24);
  const double spw = ldexp((double)m->pilot_q, -24), sg = ldexp((double)m->pilot2_q, -20);
  const double md = sd / n, var = se / n - md * md;
  out->level_dbfs = sp > 0.0 ? 10.0 * log10(sp / n / (127.5 * 127.5)) : -INFINITY;
  out->freq_err_hz = md * hz;
  out->dev_rms_hz = sqrt(var > 0.0 ? var : 0.0) * hz;
  out->pilot_rms_rad = sqrt(spw > 0.0 ? spw / n : 0.0);
  out->pilot_dev_hz = out->pilot_rms_rad * hz / pilot_gain;
  out->pilot_frac = (double)m->n_pilot / n;
  out->pilot_steadiness = spw != 0.0 ? n * sg / (spw * spw) : NAN;
  return SDRFM_OK;
}

int sdrfm_scan_meter_add(sdrfm_scan_meter* acc, const sdrfm_scan_meter* m) {
  if (!acc || !m) return SDRFM_EINVAL;
  acc->n += m->n;
  acc->n_pilot += m->n_pilot;
  acc->rf_q = (int64_t)((uint64_t)acc->rf_q + (uint64_t)m->rf_q);          /* (unsigned: wrap-around is defined) */
  acc->freq_q = (int64_t)((uint64_t)acc->freq_q + (uint64_t)m->freq_q);
  acc->dev_q = (int64_t)((uint64_t)acc->dev_q + (uint64_t)m->dev_q);
  acc->pilot_q = (int64_t)((uint64_t)acc->pilot_q + (uint64_t)m->pilot_q);
  acc->pilot2_q = (int64_t)((uint64_t)acc->pilot2_q + (uint64_t)m->pilot2_q);
  acc->reserved += m->reserved;
  return SDRFM_OK;
}

int sdrfm_scan_hist_add(uint64_t* acc512, const uint32_t* row512) {
  if (!acc512 || !row512) return SDRFM_EINVAL;
  for (uint32_t b = 0; b < SDRFM_SCAN_HIST_BINS; ++b) acc512[b] += row512[b];
  return SDRFM_OK;
}

int sdrfm_scan_hist_report(const uint64_t* hist512, const sdrfm_scan_meter* m, double fs, uint32_t D, double limit_hz, sdrfm_scan_hist_report_t* out) {
  if (!hist512 || !out || !D || !positive(fs) || !isfinite(limit_hz) || limit_hz < 0.0) return SDRFM_EINVAL;
  const int B = (int)SDRFM_SCAN_HIST_BINS;
  uint64_t total = 0;
  double moment = 0.0;                                           /* sum hist[b] (b - 255.5) */
  int lowest = -1, highest = -1;
  for (int b = 0; b < B; ++b) {
    if (!hist512[b]) continue;
    total += hist512[b];
    moment += (double)hist512[b] * ((double)b - 255.5);
    if (lowest < 0) lowest = b;
    highest = b;
  }
  if (m && m->n != total) return SDRFM_EINVAL;
  out->n = total;
  if (total == 0) {
    out->centre_hz = out->peak_pos_hz = out->peak_neg_hz = out->peak_hz = out->over_min = out->over_max = out->mpx_power_dbr = NAN;
    return SDRFM_OK;
  }
  const double n = (double)total, hz = fs / (2.0 * 3.14159265358979323846 * (double)D);
  double centre;
  if (m) centre = ldexp((double)m->freq_q, -24) / n * hz;        /* sdrfm_scan_report's freq_err_hz, operation for operation */
  else centre = hz * (moment / 64.0 / n);
  uint64_t wholly = 0, partly = 0;
  for (int b = lowest; b <= highest; ++b) {
    if (!hist512[b]) continue;
    const double lo = hz * ((double)(b - 256) / 64.0) - centre, hi = hz * ((double)(b - 255) / 64.0) - centre;
    if (lo > limit_hz || hi <= -limit_hz) wholly += hist512[b];
    if (hi > limit_hz || lo < -limit_hz) partly += hist512[b];
  }
  out->centre_hz = centre;
  out->peak_pos_hz = hz * ((double)(highest - 255) / 64.0) - centre;
  out->peak_neg_hz = hz * ((double)(lowest - 256) / 64.0) - centre;
  out->peak_hz = out->peak_pos_hz > -out->peak_neg_hz ? out->peak_pos_hz : -out->peak_neg_hz;
  out->over_min = (double)wholly / n;
  out->over_max = (double)partly / n;
  if (m) {
    const double md = ldexp((double)m->freq_q, -24) / n, var = ldexp((double)m->dev_q, -24) / n - md * md;
    const double dev = sqrt(var > 0.0 ? var : 0.0) * hz;         /* sdrfm_scan_report's dev_rms_hz */
    out->mpx_power_dbr = dev > 0.0 ? 10.0 * log10(2.0 * dev * dev / (19000.0 * 19000.0)) : -INFINITY;
  } else {
    out->mpx_power_dbr = NAN;
  }
  return SDRFM_OK;
}
