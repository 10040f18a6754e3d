/*
 * tuned_ref.c — the scalar-C definition of a tuned stream's discriminator output d (include/sdrfm.h), from the start of a
 * stream (history 0), and beside it the frozen real-tap K1-K3 in the same style, which the tuned one must reproduce bit for bit at
 * offset 0.  Compiled with -ffp-contract=off: every fmaf below is one fused operation, every other operation is rounded on its own.
 *
 *   K1  x[n] = (I - 127.5, Q - 127.5); x[n < 0] = 0
 *   K2  y[m], newest input n = (m + 1) D - 1: chains over the T inputs n - (T - 1) .. n, oldest first, tap t[T - 1 - j] on the j-th
 *       real:   y = (sum h xr, sum h xi)
 *       tuned:  A = chain with hr, B = chain with hi (each a pair); y = (Ar - Bi, Ai + Br)
 *   K3  d[m] of y[m] and y[m - 1] (y[-1] = 0): sdrfm_discriminate / sdrfm_discriminate_tuned of csrc/sdrfm_math.h (the host's IEEE divide)
 */
#include <stddef.h>
#include <stdint.h>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_math.h"

static void chain(const uint8_t* iq, int64_t newest, const float* t, uint32_t stride, uint32_t T, float* re, float* im) {
  float ar = 0.0f, ai = 0.0f;
  for (uint32_t j = 0; j < T; ++j) {
    const int64_t n = newest - (int64_t)(T - 1) + j;
    const float xr = n >= 0 ? (float)iq[2 * n] - 127.5f : 0.0f, xi = n >= 0 ? (float)iq[2 * n + 1] - 127.5f : 0.0f;
    const float c = t[(size_t)stride * (T - 1 - j)];
    ar = __builtin_fmaf(c, xr, ar);
    ai = __builtin_fmaf(c, xi, ai);
  }
  *re = ar;
  *im = ai;
}

/* d[0 .. nsamp / D) of the frozen definition, taps h[0 .. T); returns the count */
uint32_t tuned_ref_d_real(const uint8_t* iq, uint32_t nsamp, const float* h, uint32_t T, uint32_t D, float* d) {
  const uint32_t M = nsamp / D;
  float pr = 0.0f, pi = 0.0f;
  for (uint32_t m = 0; m < M; ++m) {
    float yr, yi;
    chain(iq, (int64_t)(m + 1) * D - 1, h, 1, T, &yr, &yi);
    d[m] = sdrfm_discriminate(yr, yi, pr, pi);
    pr = yr;
    pi = yi;
  }
  return M;
}

/* d[0 .. nsamp / D) of a tuned stream, taps hz[0 .. 2T) as (hr[k], hi[k]) pairs; returns the count */
uint32_t tuned_ref_d(const uint8_t* iq, uint32_t nsamp, const float* hz, uint32_t T, uint32_t D, float rot, float* d) {
  const uint32_t M = nsamp / D;
  float pr = 0.0f, pi = 0.0f;
  for (uint32_t m = 0; m < M; ++m) {
    float ar, ai, br, bi;
    chain(iq, (int64_t)(m + 1) * D - 1, hz, 2, T, &ar, &ai);
    chain(iq, (int64_t)(m + 1) * D - 1, hz + 1, 2, T, &br, &bi);
    const float yr = ar - bi, yi = ai + br;
    d[m] = sdrfm_discriminate_tuned(yr, yi, pr, pi, rot);
    pr = yr;
    pi = yi;
  }
  return M;
}
