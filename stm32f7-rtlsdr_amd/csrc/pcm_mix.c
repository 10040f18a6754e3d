/*
 * pcm_mix.c — the host side of the PCM mix bus (include/sdrfm.h), plain C99 with no GPU behind it: one bus's call one pair at
 * a time (sdrfm_pcm_mix_s16: the definition as code, and what a board-side host runs), the ranges the device takes (sdrfm_pcm_mix_check_slots,
 * sdrfm_pcm_mix_check_curve), the join of two records (sdrfm_pcm_mix_add) and what a record says (sdrfm_pcm_mix_report).
 */
#include <math.h>
#include <stddef.h>

#include "../../include/sdrfm.h"
#include "sdrfm_pcm_mix.h"

int sdrfm_pcm_mix_check_slots(const sdrfm_pcm_mix_slot* slots, uint32_t count, uint32_t n_in) {
  if (!slots) return SDRFM_EINVAL;
  for (uint32_t k = 0; k < count; ++k) {
    if (slots[k].src != PMIX_NONE && slots[k].src >= n_in) return SDRFM_EINVAL;
    if (slots[k].mode >= PMIX_MODES || slots[k].g0 > PMIX_ONE || slots[k].gt > PMIX_ONE) return SDRFM_EINVAL;
  }
  return SDRFM_OK;
}

int sdrfm_pcm_mix_check_curve(const uint16_t* curve) { return curve && pmix_curve_ok(curve) ? SDRFM_OK : SDRFM_EINVAL; }

int sdrfm_pcm_mix_s16(const int16_t* in, size_t in_stride, uint32_t n_in, uint32_t n, const sdrfm_pcm_mix_slot* slots, uint32_t n_slots, uint32_t slew,
                      uint32_t J, const uint16_t* curve, int16_t* out, sdrfm_pcm_mix_rec* acc) {
  if (!slots || !acc || n_in < 1u || n_in > PMIX_ROWS_MAX || n_slots < 1u || n_slots > PMIX_SLOTS_MAX || slew < 1u || slew > PMIX_ONE) return SDRFM_EINVAL;
  if (n > PMIX_N_MAX || J > SDRFM_ACTL_J_MAX || (in_stride & 1u) || (n && (!in || !out))) return SDRFM_EINVAL;
  if (sdrfm_pcm_mix_check_slots(slots, n_slots, n_in) != SDRFM_OK || (curve && !pmix_curve_ok(curve))) return SDRFM_EINVAL;
  if (n_in > 1u && in_stride < 2 * (size_t)n) return SDRFM_ECAPACITY;
  sdrfm_pcm_mix_rec m;
  m.n = n; m.clipped_l = 0; m.clipped_r = 0; m.peak = 0;
  for (uint32_t i = 0; i < n; ++i) {
    int64_t al = 0, ar = 0;
    for (uint32_t k = 0; k < n_slots; ++k) {
      if (!pmix_live(slots[k].src, slots[k].g0, slots[k].gt)) continue;            /* contributes 0: its row is not read */
      const int16_t* row = in + (size_t)slots[k].src * in_stride;
      const int32_t L = row[2 * (size_t)i], R = row[2 * (size_t)i + 1];
      const PmixWeights w = pmix_weights(slots[k].mode);
      const uint32_t g = audio_ctl_ramp(slots[k].g0, slots[k].gt, slew, J + i + 1u);
      const int32_t c = (int32_t)(curve ? pmix_curve(curve, g) : g);
      al += (int64_t)c * (w.ll * L + w.lr * R);
      ar += (int64_t)c * (w.rl * L + w.rr * R);
    }
    const int32_t vl = pmix_round(al), vr = pmix_round(ar), yl = pmix_clamp(vl), yr = pmix_clamp(vr);
    out[2 * (size_t)i] = (int16_t)yl;
    out[2 * (size_t)i + 1] = (int16_t)yr;
    m.clipped_l += vl != yl;
    m.clipped_r += vr != yr;
    const uint64_t ml = (uint64_t)(vl < 0 ? -vl : vl), mr = (uint64_t)(vr < 0 ? -vr : vr);
    if (ml > m.peak) m.peak = ml;
    if (mr > m.peak) m.peak = mr;
  }
  return sdrfm_pcm_mix_add(acc, &m);
}

int sdrfm_pcm_mix_add(sdrfm_pcm_mix_rec* acc, const sdrfm_pcm_mix_rec* m) {
  if (!acc || !m) return SDRFM_EINVAL;
  acc->n += m->n;
  acc->clipped_l += m->clipped_l;
  acc->clipped_r += m->clipped_r;
  if (m->peak > acc->peak) acc->peak = m->peak;
  return SDRFM_OK;
}

int sdrfm_pcm_mix_report(const sdrfm_pcm_mix_rec* m, sdrfm_pcm_mix_report_t* out) {
  if (!m || !out) return SDRFM_EINVAL;
  if (m->n == 0) {
    out->peak_dbfs = out->clipped_frac = NAN;
    return SDRFM_OK;
  }
  out->peak_dbfs = m->peak ? 20.0 * log10((double)m->peak / 32768.0) : -INFINITY;
  out->clipped_frac = (double)(m->clipped_l + m->clipped_r) / (2.0 * (double)m->n);
  return SDRFM_OK;
}
