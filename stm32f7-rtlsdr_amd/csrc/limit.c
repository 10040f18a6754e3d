/*
 * limit.c — the host side of the look-ahead PCM limiter (include/sdrfm.h), plain C99 with no GPU behind it: one stream's call
 * one pair at a time (sdrfm_pcm_limit_s16: the definition as code, and what a board-side host runs), the ranges the device takes
 * (sdrfm_pcm_limit_check_params), the ordered join of two records (sdrfm_pcm_limit_add), what a record says in dB (sdrfm_pcm_limit_report) and
 * a ceiling in LSB from dBFS (sdrfm_pcm_limit_ceiling).
 */
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "../../include/sdrfm.h"
#include "sdrfm_limit.h"

#define LIMIT_BLOCK 1024u                          /* pairs taken at a time: the work arrays stay on the stack */

uint32_t sdrfm_pcm_limit_state_words(uint32_t log2_window) {
  return log2_window >= SDRFM_LIMIT_LW_MIN && log2_window <= SDRFM_LIMIT_LW_MAX ? limit_state_words(log2_window) : 0u;
}

int sdrfm_pcm_limit_check_params(const sdrfm_pcm_limit_params* p, uint32_t log2_window, uint32_t gain_slew) {
  if (!p || !limit_shape_ok(log2_window, gain_slew) || !limit_params_ok(p)) return SDRFM_EINVAL;
  return SDRFM_OK;
}

uint32_t sdrfm_pcm_limit_ceiling(double dbfs) {
  if (isnan(dbfs)) return 1u;
  const double v = floor(32768.0 * pow(10.0, dbfs / 20.0));
  if (!(v > 1.0)) return 1u;
  return v >= 32767.0 ? SDRFM_LIMIT_CEILING_MAX : (uint32_t)v;
}

int sdrfm_pcm_limit_s16(const int16_t* in, uint32_t n, uint32_t log2_window, uint32_t gain_slew, uint32_t J, const sdrfm_pcm_limit_params* p,
                        int32_t* state, int16_t* out, sdrfm_pcm_limit_rec* acc) {
  if (!state || !acc || sdrfm_pcm_limit_check_params(p, log2_window, gain_slew) != SDRFM_OK) return SDRFM_EINVAL;
  if (n > SDRFM_LIMIT_N_MAX || J > SDRFM_ACTL_J_MAX || (n && (!in || !out))) return SDRFM_EINVAL;
  const uint32_t lw = log2_window, D = (1u << lw) - 1u;
  /* entry D + i of each array belongs to pair i of the block; the D entries before it are the pairs before the block */
  int32_t xl[SDRFM_LIMIT_D_MAX + LIMIT_BLOCK], xr[SDRFM_LIMIT_D_MAX + LIMIT_BLOCK];
  uint32_t g[SDRFM_LIMIT_D_MAX + LIMIT_BLOCK], r[SDRFM_LIMIT_D_MAX + LIMIT_BLOCK];
  for (uint32_t k = 0; k < D; ++k) {
    xl[k] = state[2u * k];
    xr[k] = state[2u * k + 1u];
    g[k] = (uint32_t)state[2u * D + k];
    r[k] = (uint32_t)state[3u * D + k];
  }
  sdrfm_pcm_limit_rec m;
  m.n = n; m.limited = 0; m.min_gain = SDRFM_LIMIT_ONE; m.at = 0;
  for (uint32_t base = 0; base < n; base += LIMIT_BLOCK) {
    const uint32_t cnt = n - base < LIMIT_BLOCK ? n - base : LIMIT_BLOCK;
    for (uint32_t i = 0; i < cnt; ++i) {                         /* the block's input is read before any of its outputs is written: out may be in */
      const uint32_t G = audio_ctl_ramp(p->gain0, p->gain_t, gain_slew, J + base + i + 1u);
      xl[D + i] = limit_gain(in[2 * (size_t)(base + i)], G);
      xr[D + i] = limit_gain(in[2 * (size_t)(base + i) + 1], G);
      g[D + i] = limit_detect(xl[D + i], xr[D + i], p->ceiling);
    }
    for (uint32_t i = 0; i < cnt; ++i) {
      uint32_t mn = SDRFM_LIMIT_ONE, S = 0;
      for (uint32_t k = 0; k <= D; ++k) mn = g[D + i - k] < mn ? g[D + i - k] : mn;
      r[D + i] = limit_apply(limit_map_of(mn, p->release), r[D + i - 1u]);
      for (uint32_t k = 0; k <= D; ++k) S += r[D + i - k];
      const uint32_t s = limit_smooth(S, lw);
      out[2 * (size_t)(base + i)] = limit_out(xl[i], s);
      out[2 * (size_t)(base + i) + 1] = limit_out(xr[i], s);
      if (s < m.min_gain) { m.min_gain = s; m.at = base + i; }   /* strict: the earliest pair stays */
      m.limited += s < SDRFM_LIMIT_ONE;
    }
    /* the last D entries of (lead-in, block) lead the next block in */
    memmove(xl, xl + cnt, sizeof(int32_t) * D);
    memmove(xr, xr + cnt, sizeof(int32_t) * D);
    memmove(g, g + cnt, sizeof(uint32_t) * D);
    memmove(r, r + cnt, sizeof(uint32_t) * D);
  }
  for (uint32_t k = 0; k < D; ++k) {
    state[2u * k] = xl[k];
    state[2u * k + 1u] = xr[k];
    state[2u * D + k] = (int32_t)g[k];
    state[3u * D + k] = (int32_t)r[k];
  }
  limit_join(acc, &m);
  return SDRFM_OK;
}

int sdrfm_pcm_limit_state_init(uint32_t log2_window, int32_t* state) {
  if (!state || log2_window < SDRFM_LIMIT_LW_MIN || log2_window > SDRFM_LIMIT_LW_MAX) return SDRFM_EINVAL;
  const uint32_t D = (1u << log2_window) - 1u;
  for (uint32_t k = 0; k < D; ++k) {
    state[2u * k] = state[2u * k + 1u] = 0;
    state[2u * D + k] = (int32_t)SDRFM_LIMIT_ONE;
    state[3u * D + k] = (int32_t)SDRFM_LIMIT_R_ONE;
  }
  return SDRFM_OK;
}

int sdrfm_pcm_limit_add(sdrfm_pcm_limit_rec* acc, const sdrfm_pcm_limit_rec* m) {
  if (!acc || !m) return SDRFM_EINVAL;
  limit_join(acc, m);
  return SDRFM_OK;
}

int sdrfm_pcm_limit_report(const sdrfm_pcm_limit_rec* m, double fs_audio, sdrfm_pcm_limit_report_t* out) {
  if (!m || !out || !(isfinite(fs_audio) && fs_audio > 0.0)) return SDRFM_EINVAL;
  if (m->n == 0) {
    out->reduction_db = out->limited_frac = out->at_seconds = NAN;
    return SDRFM_OK;
  }
  out->reduction_db = m->min_gain ? -20.0 * log10((double)m->min_gain / 32768.0) : INFINITY;
  if (m->min_gain >= SDRFM_LIMIT_ONE) out->reduction_db = 0.0;
  out->limited_frac = (double)m->limited / (double)m->n;
  out->at_seconds = (double)m->at / fs_audio;
  return SDRFM_OK;
}
