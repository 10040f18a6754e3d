/*
 * limit_tp.c — the host side of the look-ahead PCM limiter's true-peak form (include/sdrfm.h), plain C99 with no GPU behind it:
 * one stream's call one pair at a time (sdrfm_pcm_tplimit_s16: the definition as code, with 64-bit accumulation, and what a board-side host runs)
 * and the state's length, its value before the start and the latency.  The ranges, the join, the report and the ceiling are csrc/limit.c's.
 */
#include <stddef.h>
#include <string.h>

#include "../../include/sdrfm.h"
#include "sdrfm_limit.h"

#define LIMIT_BLOCK 1024u                          /* pairs taken at a time: the work arrays stay on the stack */
#define LIMIT_LX_MAX (SDRFM_LIMIT_D_MAX + SDRFM_LIMIT_H_MAX)

static int tplimit_shape_ok(uint32_t lw, uint32_t n_taps) {
  return lw >= SDRFM_LIMIT_LW_MIN && lw <= SDRFM_LIMIT_LW_MAX && tp_shape_ok(2u, n_taps) && limit_tp_window_ok(lw, n_taps);
}

uint32_t sdrfm_pcm_tplimit_state_words(uint32_t log2_window, uint32_t n_taps) {
  return tplimit_shape_ok(log2_window, n_taps) ? limit_tp_state_words(log2_window, n_taps) : 0u;
}

uint32_t sdrfm_pcm_tplimit_latency(uint32_t log2_window, uint32_t n_taps) {
  return tplimit_shape_ok(log2_window, n_taps) ? limit_tp_latency(log2_window, n_taps) : 0u;
}

int sdrfm_pcm_tplimit_state_init(uint32_t log2_window, uint32_t n_taps, int32_t* state) {
  if (!state || !tplimit_shape_ok(log2_window, n_taps)) return SDRFM_EINVAL;
  const uint32_t D = (1u << log2_window) - 1u, LX = D + n_taps / 2u;
  for (uint32_t k = 0; k < 2u * LX; ++k) state[k] = 0;
  for (uint32_t k = 0; k < D; ++k) {
    state[2u * LX + k] = (int32_t)SDRFM_LIMIT_ONE;
    state[2u * LX + D + k] = (int32_t)SDRFM_LIMIT_R_ONE;
  }
  return SDRFM_OK;
}

int sdrfm_pcm_tplimit_s16(const int16_t* in, uint32_t n, uint32_t log2_window, uint32_t gain_slew, uint32_t J, const sdrfm_pcm_limit_params* p,
                          const int16_t* coef, uint32_t n_phases, uint32_t n_taps, int32_t* state, int16_t* out, sdrfm_pcm_limit_rec* acc) {
  int16_t def[48];
  if (!state || !acc || sdrfm_pcm_limit_check_params(p, log2_window, gain_slew) != SDRFM_OK) return SDRFM_EINVAL;
  if (n > SDRFM_LIMIT_N_MAX || J > SDRFM_ACTL_J_MAX || (n && (!in || !out))) return SDRFM_EINVAL;
  if (!coef) { (void)sdrfm_truepeak_default_coef(def, &n_phases, &n_taps); coef = def; }
  if (sdrfm_truepeak_check_coef(coef, n_phases, n_taps) != SDRFM_OK || !limit_tp_window_ok(log2_window, n_taps)) return SDRFM_EINVAL;
  const uint32_t lw = log2_window, D = (1u << lw) - 1u, H = n_taps / 2u, LX = D + H;
  /* entry LX + i of the x' arrays is pair i of the block, and its detector pair, H pairs back, is entry D + i of x', g and r */
  int32_t xl[LIMIT_LX_MAX + LIMIT_BLOCK], xr[LIMIT_LX_MAX + LIMIT_BLOCK];
  uint32_t g[SDRFM_LIMIT_D_MAX + LIMIT_BLOCK], r[SDRFM_LIMIT_D_MAX + LIMIT_BLOCK];
  for (uint32_t k = 0; k < LX; ++k) {
    xl[k] = state[2u * k];
    xr[k] = state[2u * k + 1u];
  }
  for (uint32_t k = 0; k < D; ++k) {
    g[k] = (uint32_t)state[2u * LX + k];
    r[k] = (uint32_t)state[2u * LX + D + k];
  }
  sdrfm_pcm_limit_rec m;
  m.n = n; m.limited = 0; m.min_gain = SDRFM_LIMIT_ONE; m.at = 0;
  for (uint32_t base = 0; base < n; base += LIMIT_BLOCK) {
    const uint32_t cnt = n - base < LIMIT_BLOCK ? n - base : LIMIT_BLOCK;
    for (uint32_t i = 0; i < cnt; ++i) {                         /* the block's input is read before any of its outputs is written: out may be in */
      const uint32_t G = audio_ctl_ramp(p->gain0, p->gain_t, gain_slew, J + base + i + 1u);
      xl[LX + i] = limit_gain(in[2 * (size_t)(base + i)], G);
      xr[LX + i] = limit_gain(in[2 * (size_t)(base + i) + 1], G);
    }
    for (uint32_t i = 0; i < cnt; ++i) {
      uint64_t T = 0;                                            /* step 1b: LX >= NT - 1, so every x'[u - k] is in the arrays */
      for (uint32_t ph = 0; ph < n_phases; ++ph) {
        const int16_t* c = coef + (size_t)ph * n_taps;
        int64_t al = 0, ar = 0;
        for (uint32_t k = 0; k < n_taps; ++k) {
          al += (int64_t)c[k] * xl[LX + i - k];
          ar += (int64_t)c[k] * xr[LX + i - k];
        }
        const uint64_t ml = tp_abs(al), mr = tp_abs(ar);
        T = ml > T ? ml : T;
        T = mr > T ? mr : T;
      }
      g[D + i] = limit_detect_tp(xl[D + i], xr[D + i], T, p->ceiling);
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
    /* the last entries of (lead-in, block) lead the next block in */
    memmove(xl, xl + cnt, sizeof(int32_t) * LX);
    memmove(xr, xr + cnt, sizeof(int32_t) * LX);
    memmove(g, g + cnt, sizeof(uint32_t) * D);
    memmove(r, r + cnt, sizeof(uint32_t) * D);
  }
  for (uint32_t k = 0; k < LX; ++k) {
    state[2u * k] = xl[k];
    state[2u * k + 1u] = xr[k];
  }
  for (uint32_t k = 0; k < D; ++k) {
    state[2u * LX + k] = (int32_t)g[k];
    state[2u * LX + D + k] = (int32_t)r[k];
  }
  limit_join(acc, &m);
  return SDRFM_OK;
}
