/*
 * scan_ref.c — the scalar-C definition of a scan stream's record (include/sdrfm.h) from the bytes of a stream's start
 * (history 0), in the style of tuned_ref.c.  Compiled with -ffp-contract=off: every fmaf below is one fused operation, every other
 * operation is rounded on its own.
 *
 *   K1  x[n] = (I - 127.5, Q - 127.5); x[n < 0] = 0
 *   K2  y[m], newest input n = (m + 1) D - 1: A = chain with hr, B = chain with hi over the T inputs n - (T - 1) .. n, oldest first, tap
 *       t[T - 1 - j] on the j-th; y = (Ar - Bi, Ai + Br)
 *   K3  d[m] of y[m] and y[m - 1] (y[-1] = 0): sdrfm_discriminate_tuned of csrc/sdrfm_math.h (the host's IEEE divide)
 *   q   q[m] = sum_k b[k] d[m - k], two fmaf chains, oldest d first (k = P - 1 first), d[m < 0] = 0
 *   the five terms of m and their integers: p = fmaf(yr, yr, yi yi) at 2^8; d and e = d d at 2^24; pw = fmaf(qr, qr, qi qi) at 2^24;
 *   g = pw pw at 2^20; each (int64) rintf(term 2^k), ties to even
 * The record of the d's [m0, m1) is the sum of their integers: a call that follows earlier calls has m0 > 0.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_math.h"

static void chain(const uint8_t* iq, int64_t newest, const float* t, uint32_t T, float* re, float* im) {
  float ar = 0.0f, ai = 0.0f;
  for (uint32_t j = 0; j < T; ++j) {
    const int64_t n = newest - (int64_t)(T - 1) + j;
    const float xr = n >= 0 ? (float)iq[2 * n] - 127.5f : 0.0f, xi = n >= 0 ? (float)iq[2 * n + 1] - 127.5f : 0.0f;
    const float c = t[2 * (size_t)(T - 1 - j)];
    ar = __builtin_fmaf(c, xr, ar);
    ai = __builtin_fmaf(c, xi, ai);
  }
  *re = ar;
  *im = ai;
}

static int64_t fix(float term, float scale) { return (int64_t)rintf(term * scale); }

/* d[0 .. M), p[0 .. M) and pw[0 .. M) of the stream, M = nsamp / D (taps hz[0 .. 2T) as (hr, hi) pairs, b[0 .. 2P) as (re, im) pairs), and
 * rec[0 .. 8) = the record of the d's [m0, m1) in sdrfm_scan_meter's order; returns M */
uint32_t scan_ref(const uint8_t* iq, uint32_t nsamp, const float* hz, uint32_t T, uint32_t D, float rot, const float* b, uint32_t P, float pmin2,
                  uint32_t m0, uint32_t m1, float* d, float* p, float* pw, int64_t* rec) {
  const uint32_t M = nsamp / D;
  float pr = 0.0f, pi = 0.0f;
  for (uint32_t m = 0; m < M; ++m) {
    float ar, ai, br, bi;
    chain(iq, (int64_t)(m + 1) * D - 1, hz, T, &ar, &ai);
    chain(iq, (int64_t)(m + 1) * D - 1, hz + 1, T, &br, &bi);
    const float yr = ar - bi, yi = ai + br;
    d[m] = sdrfm_discriminate_tuned(yr, yi, pr, pi, rot);
    p[m] = __builtin_fmaf(yr, yr, yi * yi);
    pr = yr;
    pi = yi;
  }
  for (uint32_t m = 0; m < M; ++m) {
    float qr = 0.0f, qi = 0.0f;
    for (uint32_t j = 0; j < P; ++j) {                           /* oldest first: k = P - 1 - j */
      const uint32_t k = P - 1 - j;
      const float dv = m >= k ? d[m - k] : 0.0f;
      qr = __builtin_fmaf(b[2 * k], dv, qr);
      qi = __builtin_fmaf(b[2 * k + 1], dv, qi);
    }
    pw[m] = __builtin_fmaf(qr, qr, qi * qi);
  }
  for (int k = 0; k < 8; ++k) rec[k] = 0;
  for (uint32_t m = m0; m < m1 && m < M; ++m) {
    rec[0] += 1;
    rec[1] += pw[m] >= pmin2 ? 1 : 0;
    rec[2] += fix(p[m], 0x1p+8f);
    rec[3] += fix(d[m], 0x1p+24f);
    rec[4] += fix(d[m] * d[m], 0x1p+24f);
    rec[5] += fix(pw[m], 0x1p+24f);
    rec[6] += fix(pw[m] * pw[m], 0x1p+20f);
  }
  return M;
}
