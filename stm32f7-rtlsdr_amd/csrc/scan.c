/*
 * scan.c — the host side of the scan handle's records (include/sdrfm.h), plain C99 with no GPU behind it: what a
 * sdrfm_scan_meter says in physical units (sdrfm_scan_report) and the exact sum of records (sdrfm_scan_meter_add).
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
