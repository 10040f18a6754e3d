/*
 * truepeak.c — the host side of the stereo PCM sink's true-peak meter (include/sdrfm.h), plain C99 with no GPU behind it: the
 * default table of ITU-R BS.1770-4 Annex 2, the bound a table has to keep for the device to take it (sdrfm_truepeak_check_coef), a limit in
 * the record's units (sdrfm_truepeak_limit), the record of int16 stereo PCM one pair at a time (sdrfm_pcm_truepeak_s16: the definition as
 * code, and what a board-side host runs), the ordered join of two records (sdrfm_truepeak_add) and what a record says in dBTP
 * (sdrfm_truepeak_report).
 */
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "../../include/sdrfm.h"
#include "sdrfm_truepeak.h"

/* BS.1770-4 Annex 2, phases 0 and 1 in units of 2^-13; phase 2 is phase 1 reversed, phase 3 phase 0 reversed */
static const int16_t TP_BS1770[2][12] = {
  {14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68},
  {-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155},
};

int sdrfm_truepeak_default_coef(int16_t* out, uint32_t* n_phases, uint32_t* n_taps) {
  if (!out) return SDRFM_EINVAL;
  for (uint32_t k = 0; k < 12u; ++k) {
    out[k] = (int16_t)(4 * TP_BS1770[0][k]);                     /* 2^-13 -> Q15; the largest is 31856 */
    out[12u + k] = (int16_t)(4 * TP_BS1770[1][k]);
    out[24u + k] = (int16_t)(4 * TP_BS1770[1][11u - k]);
    out[36u + k] = (int16_t)(4 * TP_BS1770[0][11u - k]);
  }
  if (n_phases) *n_phases = 4u;
  if (n_taps) *n_taps = 12u;
  return SDRFM_OK;
}

int sdrfm_truepeak_check_coef(const int16_t* coef, uint32_t n_phases, uint32_t n_taps) {
  if (!coef || !tp_shape_ok(n_phases, n_taps)) return SDRFM_EINVAL;
  const uint32_t half = n_taps / 2u;
  for (uint32_t p = 0; p < n_phases; ++p)
    for (uint32_t h = 0; h < 2u; ++h) {
      uint32_t sum = 0;
      for (uint32_t k = 0; k < half; ++k) {
        const int32_t c = coef[(size_t)p * n_taps + h * half + k];
        sum += (uint32_t)(c < 0 ? -c : c);
      }
      if (sum > SDRFM_TP_HALF_MAX) return SDRFM_EINVAL;
    }
  return SDRFM_OK;
}

uint64_t sdrfm_truepeak_limit(double dbtp) {
  if (isnan(dbtp)) return 0u;
  const double v = floor(1073741824.0 * pow(10.0, dbtp / 20.0));
  if (!(v > 0.0)) return 0u;
  return v >= 4294967295.0 ? SDRFM_TP_LIMIT_MAX : (uint64_t)v;
}

int sdrfm_pcm_truepeak_s16(const int16_t* pcm_interleaved, uint32_t n, const int16_t* coef, uint32_t n_phases, uint32_t n_taps, uint64_t limit,
                           int16_t* hist, sdrfm_truepeak* acc) {
  if (!acc || !coef || !hist || (!pcm_interleaved && n) || !tp_shape_ok(n_phases, n_taps) || limit > SDRFM_TP_LIMIT_MAX) return SDRFM_EINVAL;
  const uint32_t keep = n_taps - 1u;
  sdrfm_truepeak m;
  memset(&m, 0, sizeof(m));
  m.n = n;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t p = 0; p < n_phases; ++p) {
      const int16_t* c = coef + (size_t)p * n_taps;
      int64_t a[2] = {0, 0};
      for (uint32_t k = 0; k < n_taps; ++k) {
        const int64_t idx = (int64_t)i - (int64_t)k;             /* the history below 0 */
        const int16_t* x = idx >= 0 ? pcm_interleaved + 2 * (size_t)idx : hist + 2 * (size_t)((int64_t)keep + idx);
        a[0] += (int32_t)c[k] * x[0];
        a[1] += (int32_t)c[k] * x[1];
      }
      const uint64_t ml = tp_abs(a[0]), mr = tp_abs(a[1]);
      if (ml > m.peak_l) { m.peak_l = ml; m.at_l = i; }          /* strict: the earliest pair stays */
      if (mr > m.peak_r) { m.peak_r = mr; m.at_r = i; }
      m.over_l += ml > limit;
      m.over_r += mr > limit;
    }
  tp_join(acc, &m);
  /* the last n_taps - 1 pairs of (history, new pairs): for n < n_taps - 1 the history's tail moves down first */
  if (n >= keep) memcpy(hist, pcm_interleaved + 2 * (size_t)(n - keep), sizeof(int16_t) * 2 * keep);
  else if (n) {
    memmove(hist, hist + 2 * (size_t)n, sizeof(int16_t) * 2 * (keep - n));
    memcpy(hist + 2 * (size_t)(keep - n), pcm_interleaved, sizeof(int16_t) * 2 * n);
  }
  return SDRFM_OK;
}

int sdrfm_truepeak_add(sdrfm_truepeak* acc, const sdrfm_truepeak* m) {
  if (!acc || !m) return SDRFM_EINVAL;
  tp_join(acc, m);
  return SDRFM_OK;
}

static double tp_dbtp(uint64_t peak) { return peak ? 20.0 * log10((double)peak / 1073741824.0) : -INFINITY; }

int sdrfm_truepeak_report(const sdrfm_truepeak* m, uint32_t n_phases, double fs_audio, sdrfm_truepeak_report_t* out) {
  if (!m || !out || !(n_phases == 2u || n_phases == 4u || n_phases == 8u) || !(isfinite(fs_audio) && fs_audio > 0.0)) return SDRFM_EINVAL;
  if (m->n == 0) {
    double* f = (double*)out;
    for (size_t k = 0; k < sizeof(*out) / sizeof(double); ++k) f[k] = NAN;
    return SDRFM_OK;
  }
  const double values = (double)m->n * (double)n_phases;
  out->dbtp_l = tp_dbtp(m->peak_l);
  out->dbtp_r = tp_dbtp(m->peak_r);
  out->dbtp = out->dbtp_l > out->dbtp_r ? out->dbtp_l : out->dbtp_r;
  out->over_frac_l = (double)m->over_l / values;
  out->over_frac_r = (double)m->over_r / values;
  out->at_seconds_l = (double)m->at_l / fs_audio;
  out->at_seconds_r = (double)m->at_r / fs_audio;
  return SDRFM_OK;
}
