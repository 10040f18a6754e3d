/*
 * retune_ref.c — the scalar-C definition of a re-tuned stream's discriminator output d (include/sdrfm.h) in the style of
 * tuned_ref.c: one stream from its first byte (history 0) under a list of events, each of which acts between two d's.  Compiled with
 * -ffp-contract=off: every fmaf below is one fused operation, every other operation is rounded on its own.
 *
 * K1-K3 are tuned_ref.c's (the real-tap form until the first event where the stream starts untuned).  An event at input n0 acts when the
 * inputs [0, n0) have been taken: before d[m0], m0 = n0 / D.  It replaces the taps and the rotation and transforms the carried state:
 *   restart   x[n < n0] = 0 from here on, y[m0 - 1] = 0 and every earlier d is 0 for what follows
 *   kept      y[m0 - 1] is turned by the carry unless that is bitwise (1.0f, +0.0f):  t = yi*ci; yr' = fmaf(yr, cr, -t); u = yi*cr;
 *             yi' = fmaf(yr, ci, u);  the last H d's gain sh = rot_old - rot_new, wrapped once, unless sh == 0.0f
 * What the stages behind d see of the earlier d's after event e — the last H of them matter — is written to view + e * M: d[0 .. m0) as
 * transformed by this and every earlier event (the d's before the stream's start are not part of it: an event with sh != 0 needs
 * m0 >= H to be composed with those stages).
 */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_math.h"

static void chain(const uint8_t* iq, int64_t newest, int64_t xmin, const float* t, uint32_t stride, uint32_t T, float* re, float* im) {
  float ar = 0.0f, ai = 0.0f;
  for (uint32_t j = 0; j < T; ++j) {
    const int64_t n = newest - (int64_t)(T - 1) + j;
    const float xr = n >= xmin ? (float)iq[2 * n] - 127.5f : 0.0f, xi = n >= xmin ? (float)iq[2 * n + 1] - 127.5f : 0.0f;
    const float c = t[(size_t)stride * (T - 1 - j)];
    ar = __builtin_fmaf(c, xr, ar);
    ai = __builtin_fmaf(c, xi, ai);
  }
  *re = ar;
  *im = ai;
}

/* d[0 .. nsamp / D) of a stream that starts with the real taps h0[0 .. T) (real0 != 0) or the tuned taps h0[0 .. 2T) and rot0, under n_ev
 * events in the order given, their n0 not decreasing: ev_n0[e], ev_hz + e * 2T, ev_rot[e], ev_carry + 2 e, ev_restart[e].
 * view: n_ev x M floats (see above).  Returns the count M. */
uint32_t retune_ref_d(const uint8_t* iq, uint32_t nsamp, uint32_t T, uint32_t D, uint32_t H, const float* h0, int real0, float rot0, uint32_t n_ev,
                      const uint32_t* ev_n0, const float* ev_hz, const float* ev_rot, const float* ev_carry, const uint8_t* ev_restart, float* d,
                      float* view) {
  const uint32_t M = nsamp / D;
  const float* hz = h0;
  int real = real0;
  float rot = real0 ? 0.0f : rot0, pr = 0.0f, pi = 0.0f;
  int64_t xmin = 0;
  uint32_t e = 0;
  for (uint32_t m = 0; m <= M; ++m) {
    for (; e < n_ev && ev_n0[e] / D == m; ++e) {                  /* the events before d[m] */
      const float cr = ev_carry[2 * e], ci = ev_carry[2 * e + 1];
      float* v = view + (size_t)e * M;                            /* the view after the event before this one, then the d's since */
      const uint32_t mp = e ? ev_n0[e - 1] / D : 0;
      if (e) memcpy(v, view + (size_t)(e - 1) * M, sizeof(float) * mp);
      memcpy(v + mp, d + mp, sizeof(float) * (m - mp));
      memset(v + m, 0, sizeof(float) * (M - m));
      if (ev_restart[e]) {
        xmin = ev_n0[e];
        pr = pi = 0.0f;
        memset(v, 0, sizeof(float) * m);
      } else {
        uint32_t one_bits, zero_bits;
        memcpy(&one_bits, &cr, 4);
        memcpy(&zero_bits, &ci, 4);
        if (!(one_bits == 0x3f800000u && zero_bits == 0u)) {
          const float t = pi * ci, u = pi * cr;
          const float nr = __builtin_fmaf(pr, cr, -t), ni = __builtin_fmaf(pr, ci, u);
          pr = nr;
          pi = ni;
        }
        float sh = rot - ev_rot[e];
        if (sh > 0x1.921fb6p+1f) sh -= 0x1.921fb6p+2f;
        else if (sh < -0x1.921fb6p+1f) sh += 0x1.921fb6p+2f;
        if (sh != 0.0f)
          for (uint32_t i = m > H ? m - H : 0; i < m; ++i) v[i] = v[i] + sh;
      }
      hz = ev_hz + (size_t)e * 2 * T;
      rot = ev_rot[e];
      real = 0;
    }
    if (m == M) break;
    float yr, yi;
    const int64_t newest = (int64_t)(m + 1) * D - 1;
    if (real) {
      chain(iq, newest, xmin, hz, 1, T, &yr, &yi);
      d[m] = sdrfm_discriminate(yr, yi, pr, pi);
    } else {
      float ar, ai, br, bi;
      chain(iq, newest, xmin, hz, 2, T, &ar, &ai);
      chain(iq, newest, xmin, hz + 1, 2, T, &br, &bi);
      yr = ar - bi;
      yi = ai + br;
      d[m] = sdrfm_discriminate_tuned(yr, yi, pr, pi, rot);
    }
    pr = yr;
    pi = yi;
  }
  return M;
}
