/*
 * pcm_sink.c — the step right after the path on the reference board: demodulated audio (radians per
 * 240 kS/s sample, at 48 kHz) -> FM de-emphasis -> int16 stereo-interleaved PCM in the layout BSP_AUDIO_OUT_Play consumes
 * (uint16_t* pBuffer, Size in bytes; Utilities/STM32746G-Discovery/stm32746g_discovery_audio.c:224; L and R carry the same
 * mono programme).  Host-side plain C on purpose: the de-emphasis is a one-pole recursion (serial per stream) over
 * 4.9 MB per batch, i.e. microseconds of CPU time next to the D2H copy; it is not part of the GPU hot path.
 *
 *   y[n]   = y[n-1] + alpha * (x[n] - y[n-1])          alpha = 1 - exp(-1 / (fs * tau)),  tau = 75e-6 (US) or 50e-6 (EU)
 *   pcm[n] = sat16(lrintf(y[n] * gain))                 gain: radians -> full scale, e.g. 32767 / (2*pi*75e3/240e3)
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sdrfm.h"
#include "sdrfm_audio_ctl.h"

int sdrfm_pcm_deemph_s16(const float* audio, uint32_t n, float alpha, float gain, float* state, int16_t* pcm_stereo) {
  if ((n && (!audio || !pcm_stereo)) || !state || !(alpha > 0.0f) || alpha > 1.0f) return SDRFM_EINVAL;
  float y = *state;
  for (uint32_t i = 0; i < n; ++i) {
    y = fmaf(alpha, audio[i] - y, y);
    float v = y * gain;
    if (v > 32767.0f) v = 32767.0f;
    if (v < -32768.0f) v = -32768.0f;
    const int16_t s = (int16_t)lrintf(v);
    pcm_stereo[2 * i] = s;
    pcm_stereo[2 * i + 1] = s;
  }
  *state = y;
  return SDRFM_OK;
}

/* one channel of the stereo form: the operations of sdrfm_pcm_deemph_s16, every second PCM slot */
static void deemph_channel(const float* x, uint32_t n, float alpha, float gain, float* state, int16_t* pcm) {
  float y = *state;
  for (uint32_t i = 0; i < n; ++i) {
    y = fmaf(alpha, x[i] - y, y);
    float v = y * gain;
    if (v > 32767.0f) v = 32767.0f;
    if (v < -32768.0f) v = -32768.0f;
    pcm[2 * i] = (int16_t)lrintf(v);
  }
  *state = y;
}

int sdrfm_pcm_deemph_stereo_s16(const float* left, const float* right, uint32_t n, float alpha, float gain, float* state,
                                int16_t* pcm_stereo) {
  if ((n && (!left || !right || !pcm_stereo)) || !state || !(alpha > 0.0f) || alpha > 1.0f) return SDRFM_EINVAL;
  deemph_channel(left, n, alpha, gain, &state[0], pcm_stereo);
  deemph_channel(right, n, alpha, gain, &state[1], pcm_stereo + 1);
  return SDRFM_OK;
}

/* The stereo form with a ramped high-cut (include/sdrfm.h): the coefficient of sample i is alpha scaled by the ramp's Q15 value
 * after J + i + 1 samples; L and R share it and carry their own y.  The definition, in its order: the reference of the device sink's conditioned forms. */
int sdrfm_pcm_deemph_stereo_hicut_s16(const float* left, const float* right, uint32_t n, float alpha, float gain, uint16_t h0, uint16_t ht,
                                      uint32_t slew, uint32_t J, float* state, int16_t* pcm_stereo) {
  if ((n && (!left || !right || !pcm_stereo)) || !state || !(alpha > 0.0f) || alpha > 1.0f) return SDRFM_EINVAL;
  if (h0 < SDRFM_HICUT_MIN || h0 > SDRFM_ACTL_ONE || ht < SDRFM_HICUT_MIN || ht > SDRFM_ACTL_ONE) return SDRFM_EINVAL;
  if (slew < 1u || slew > SDRFM_ACTL_ONE) return SDRFM_EINVAL;
  float yl = state[0], yr = state[1];
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t h = audio_ctl_ramp(h0, ht, slew, audio_ctl_advance(J, i + 1u));
    const float a = alpha * ((float)h * 0x1p-15f);
    yl = fmaf(a, left[i] - yl, yl);
    yr = fmaf(a, right[i] - yr, yr);
    float vl = yl * gain, vr = yr * gain;
    if (vl > 32767.0f) vl = 32767.0f;
    if (vl < -32768.0f) vl = -32768.0f;
    if (vr > 32767.0f) vr = 32767.0f;
    if (vr < -32768.0f) vr = -32768.0f;
    pcm_stereo[2 * (size_t)i] = (int16_t)lrintf(vl);
    pcm_stereo[2 * (size_t)i + 1] = (int16_t)lrintf(vr);
  }
  state[0] = yl;
  state[1] = yr;
  return SDRFM_OK;
}

float sdrfm_pcm_alpha(float fs_hz, float tau_s) { return 1.0f - expf(-1.0f / (fs_hz * tau_s)); }
