/*
 * pcm_rate.c — the host side of the PCM rate matcher (include/sdrfm.h), plain C99 with no GPU behind it: one stream's call
 * one output pair at a time (sdrfm_pcm_rate_s16: the definition as code, and what a board-side host runs) and the bound a coefficient
 * table has to keep for the device to take it (sdrfm_pcm_rate_check_coef).
 */
#include <stddef.h>
#include <string.h>

#include "../../include/sdrfm.h"
#include "sdrfm_pcm_rate.h"

static int rate_shape_ok(uint32_t n_taps, uint32_t log2_phases) {
  return n_taps >= SDRFM_RATE_TAPS_MIN && n_taps <= SDRFM_RATE_TAPS_MAX && n_taps % 4u == 0 && log2_phases >= SDRFM_RATE_LOGPH_MIN &&
         log2_phases <= SDRFM_RATE_LOGPH_MAX;
}

int sdrfm_pcm_rate_check_coef(const int16_t* coef, uint32_t n_taps, uint32_t log2_phases) {
  if (!coef || !rate_shape_ok(n_taps, log2_phases)) return SDRFM_EINVAL;
  const uint32_t rows = (1u << log2_phases) + 1u, half = n_taps / 2u;
  for (uint32_t p = 0; p < rows; ++p)
    for (uint32_t h = 0; h < 2; ++h) {
      uint32_t sum = 0;
      for (uint32_t k = 0; k < half; ++k) {
        const int32_t c = coef[(size_t)p * n_taps + h * half + k];
        sum += (uint32_t)(c < 0 ? -c : c);
      }
      if (sum > SDRFM_RATE_HALF_MAX) return SDRFM_EINVAL;
    }
  return SDRFM_OK;
}

/* pair idx of the call's input: the history below 0 */
static const int16_t* rate_pair(const int16_t* in, const int16_t* hist, int64_t idx, uint32_t n_taps) {
  return idx >= 0 ? in + 2 * (size_t)idx : hist + 2 * (size_t)((int64_t)(n_taps - 1u) + idx);
}

int sdrfm_pcm_rate_s16(const int16_t* in, uint32_t n, const int16_t* coef, uint32_t n_taps, uint32_t log2_phases, uint64_t step, uint64_t* pos,
                       int16_t* hist, int16_t* out, uint32_t out_cap_pairs, uint32_t* n_out) {
  if (!coef || !pos || !hist || !n_out || !rate_shape_ok(n_taps, log2_phases)) return SDRFM_EINVAL;
  if (step < SDRFM_RATE_STEP_MIN || step > SDRFM_RATE_STEP_MAX || n > SDRFM_RATE_N_MAX || (!in && n)) return SDRFM_EINVAL;
  const uint32_t cnt = rate_count(*pos, step, n);
  if (cnt > out_cap_pairs) return SDRFM_ECAPACITY;               /* before anything is written */
  if (cnt && !out) return SDRFM_EINVAL;
  for (uint32_t j = 0; j < cnt; ++j) {
    const uint64_t P = *pos + (uint64_t)j * step;
    const int64_t i = (int64_t)(P >> 32);
    const uint32_t f = (uint32_t)P;
    const uint32_t p = f >> (32u - log2_phases), mu = (f >> (24u - log2_phases)) & 255u;
    const int16_t* c0 = coef + (size_t)p * n_taps;
    const int16_t* c1 = c0 + n_taps;
    int64_t a[2][2] = {{0, 0}, {0, 0}};                          /* [channel][row] */
    for (uint32_t k = 0; k < n_taps; ++k) {
      const int16_t* x = rate_pair(in, hist, i - (int64_t)n_taps + 1 + (int64_t)k, n_taps);
      a[0][0] += (int32_t)c0[k] * x[0];
      a[0][1] += (int32_t)c1[k] * x[0];
      a[1][0] += (int32_t)c0[k] * x[1];
      a[1][1] += (int32_t)c1[k] * x[1];
    }
    out[2 * (size_t)j] = rate_mix(a[0][0], a[0][1], mu);
    out[2 * (size_t)j + 1] = rate_mix(a[1][0], a[1][1], mu);
  }
  *pos = rate_advance(*pos, step, n, cnt);
  /* the last n_taps - 1 pairs of (history, new pairs): for n < n_taps - 1 the history's tail moves down first */
  const uint32_t keep = n_taps - 1u;
  if (n >= keep) memcpy(hist, in + 2 * (size_t)(n - keep), sizeof(int16_t) * 2 * keep);
  else if (n) {
    memmove(hist, hist + 2 * (size_t)n, sizeof(int16_t) * 2 * (keep - n));
    memcpy(hist + 2 * (size_t)(keep - n), in, sizeof(int16_t) * 2 * n);
  }
  *n_out = cnt;
  return SDRFM_OK;
}
