/*
 * iq_meter.c — the host side of the raw-capture IQ meter (include/sdrfm.h), plain C99, no GPU behind it:
 * sdrfm_iq_meter_u8 is the definition as code (the device kernel equals it integer for integer), the joins of records and rows, and what a
 * record and a row say in double.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sdrfm.h"

__extension__ typedef unsigned __int128 u128;

int sdrfm_iq_meter_u8(const uint8_t* iq, size_t nbytes, sdrfm_iq_meter* acc, uint64_t* hist512) {
  if (!acc || (!iq && nbytes)) return SDRFM_EINVAL;
  if (nbytes & 1u) return SDRFM_EODD;
  uint64_t si = 0, sq = 0, sii = 0, sqq = 0, siq = 0, ri = 0, rq = 0;
  for (size_t k = 0; k < nbytes; k += 2) {
    const uint32_t bi = iq[k], bq = iq[k + 1];
    si += bi; sq += bq;
    sii += bi * bi; sqq += bq * bq; siq += bi * bq;
    ri += (bi == 0u) | (bi == 255u);
    rq += (bq == 0u) | (bq == 255u);
    if (hist512) { hist512[bi] += 1; hist512[256u + bq] += 1; }
  }
  acc->n += nbytes / 2;
  acc->sum_i += si; acc->sum_q += sq;
  acc->sum_ii += sii; acc->sum_qq += sqq; acc->sum_iq += siq;
  acc->rail_i += ri; acc->rail_q += rq;
  return SDRFM_OK;
}

int sdrfm_iq_meter_add(sdrfm_iq_meter* acc, const sdrfm_iq_meter* m) {
  if (!acc || !m) return SDRFM_EINVAL;
  acc->n += m->n;
  acc->sum_i += m->sum_i; acc->sum_q += m->sum_q;
  acc->sum_ii += m->sum_ii; acc->sum_qq += m->sum_qq; acc->sum_iq += m->sum_iq;
  acc->rail_i += m->rail_i; acc->rail_q += m->rail_q;
  return SDRFM_OK;
}

int sdrfm_iq_hist_add(uint64_t* acc512, const uint32_t* row512) {
  if (!acc512 || !row512) return SDRFM_EINVAL;
  for (uint32_t b = 0; b < SDRFM_IQ_HIST_BINS; ++b) acc512[b] += row512[b];
  return SDRFM_OK;
}

/* (a - b) as a double, from the integers */
static double diff128(u128 a, u128 b) { return a >= b ? (double)(a - b) : -(double)(b - a); }

int sdrfm_iq_meter_report(const sdrfm_iq_meter* m, sdrfm_iq_report_t* out) {
  if (!m || !out) return SDRFM_EINVAL;
  if (m->n == 0) {
    double* f = (double*)out;
    for (size_t k = 0; k < sizeof(*out) / sizeof(double); ++k) f[k] = NAN;
    return SDRFM_OK;
  }
  const u128 n = m->n, si = m->sum_i, sq = m->sum_q;
  if (n * m->sum_ii < si * si || n * m->sum_qq < sq * sq) return SDRFM_EINVAL;
  const double nn = (double)n * (double)n;
  const double var_i = (double)(n * m->sum_ii - si * si) / nn, var_q = (double)(n * m->sum_qq - sq * sq) / nn;
  const double cov = diff128(n * m->sum_iq, si * sq) / nn;
  out->dc_i = diff128(2 * si, 255 * n) / (2.0 * (double)n);
  out->dc_q = diff128(2 * sq, 255 * n) / (2.0 * (double)n);
  const double fs2 = 127.5 * 127.5, var = var_i + var_q;
  out->rms_dbfs = var > 0.0 ? 10.0 * log10(var / fs2) : -INFINITY;
  const double total = var + out->dc_i * out->dc_i + out->dc_q * out->dc_q;
  out->total_dbfs = total > 0.0 ? 10.0 * log10(total / fs2) : -INFINITY;
  out->rail_share_i = (double)m->rail_i / (double)n;
  out->rail_share_q = (double)m->rail_q / (double)n;
  if (!(var_i > 0.0) || !(var_q > 0.0)) {
    out->gain_db = out->skew_rad = out->image_rejection_db = NAN;
    return SDRFM_OK;
  }
  double rho = cov / sqrt(var_i * var_q);
  rho = rho > 1.0 ? 1.0 : rho < -1.0 ? -1.0 : rho;
  const double g = sqrt(var_q / var_i);
  out->gain_db = 10.0 * log10(var_q / var_i);
  out->skew_rad = asin(rho);
  const double c = 2.0 * g * cos(out->skew_rad), num = 1.0 + c + g * g, den = 1.0 - c + g * g;
  out->image_rejection_db = den > 0.0 ? 10.0 * log10(num / den) : INFINITY;
  return SDRFM_OK;
}

int sdrfm_iq_hist_report(const uint64_t* hist512, sdrfm_iq_hist_report_t* out) {
  if (!hist512 || !out) return SDRFM_EINVAL;
  u128 tot[2] = {0, 0};
  for (int c = 0; c < 2; ++c)
    for (int b = 0; b < 256; ++b) tot[c] += hist512[256 * c + b];
  if (tot[0] != tot[1] || tot[0] >> 64) return SDRFM_EINVAL;
  out->n = (uint64_t)tot[0];
  double* res[2][4] = {{&out->peak_i, &out->level999_i, &out->codes_i, &out->headroom_db_i}, {&out->peak_q, &out->level999_q, &out->codes_q, &out->headroom_db_q}};
  for (int c = 0; c < 2; ++c) {
    if (out->n == 0) { *res[c][0] = *res[c][1] = *res[c][2] = *res[c][3] = NAN; continue; }
    const uint64_t* h = hist512 + 256 * c;
    int codes = 0, peak = -1, k999 = -1;
    u128 cum = 0;
    for (int b = 0; b < 256; ++b) codes += h[b] != 0;
    for (int k = 0; k < 128; ++k) {                              /* level (2k + 1) / 255: the codes 127 - k and 128 + k */
      const u128 at = (u128)h[127 - k] + h[128 + k];
      if (at) peak = k;
      cum += at;
      if (k999 < 0 && cum * 1000 >= tot[c] * 999) k999 = k;
    }
    *res[c][0] = (2.0 * peak + 1.0) / 255.0;
    *res[c][1] = (2.0 * k999 + 1.0) / 255.0;
    *res[c][2] = (double)codes;
    *res[c][3] = -20.0 * log10(*res[c][1]);
  }
  return SDRFM_OK;
}
