/*
 * audio_meter.c — the host side of the stereo PCM sink's audio meter (include/sdrfm.h), plain C99 with no GPU behind it:
 * the record of int16 stereo PCM one pair at a time (sdrfm_pcm_audio_meter_s16: the definition as code, and what a board-side host runs),
 * the ordered join of two records (sdrfm_audio_meter_add) and what a record says in physical units (sdrfm_audio_meter_report).
 */
#include <math.h>
#include <stddef.h>
#include <string.h>

#include "../../include/sdrfm.h"
#include "sdrfm_audio_meter.h"

/* one more pair onto a predicate's runs; run = the length of the run that ends at the pair before, all = every pair so far satisfied it */
static void runs_step(sdrfm_audio_runs* r, int q, uint64_t* run, int* all) {
  if (q) {
    ++r->count;
    ++*run;
    if (*all) r->lead = *run;
    if (*run > r->longest) r->longest = *run;
  } else {
    *run = 0;
    *all = 0;
  }
  r->trail = *run;
}

int sdrfm_pcm_audio_meter_s16(const int16_t* pcm_interleaved, uint32_t n, uint32_t quiet_lsb, sdrfm_audio_meter* acc) {
  if (!acc || quiet_lsb > SDRFM_AM_QUIET_MAX || (!pcm_interleaved && n)) return SDRFM_EINVAL;
  sdrfm_audio_meter m;
  memset(&m, 0, sizeof(m));
  const int32_t q = (int32_t)quiet_lsb;
  uint64_t run[3] = {0, 0, 0};
  int all[3] = {1, 1, 1};
  uint64_t sum_l = 0, sum_r = 0, cross = 0;                       /* signed sums in unsigned arithmetic: wrap-around is defined */
  for (uint32_t i = 0; i < n; ++i) {
    const int32_t L = pcm_interleaved[2 * (size_t)i], R = pcm_interleaved[2 * (size_t)i + 1];
    const uint32_t al = (uint32_t)(L < 0 ? -L : L), ar = (uint32_t)(R < 0 ? -R : R);
    sum_l += (uint64_t)(int64_t)L;
    sum_r += (uint64_t)(int64_t)R;
    m.sq_l += (uint64_t)(L * L);
    m.sq_r += (uint64_t)(R * R);
    cross += (uint64_t)(int64_t)(L * R);
    if (al > m.peak_l) m.peak_l = al;
    if (ar > m.peak_r) m.peak_r = ar;
    m.clip_l += (L == -32768 || L == 32767);
    m.clip_r += (R == -32768 || R == 32767);
    const int ql = (int32_t)al <= q, qr = (int32_t)ar <= q;
    runs_step(&m.quiet_l, ql, &run[0], &all[0]);
    runs_step(&m.quiet_r, qr, &run[1], &all[1]);
    runs_step(&m.quiet_both, ql && qr, &run[2], &all[2]);
  }
  m.n = n;
  m.sum_l = (int64_t)sum_l;
  m.sum_r = (int64_t)sum_r;
  m.cross = (int64_t)cross;
  am_meter_join(acc, &m);
  return SDRFM_OK;
}

int sdrfm_audio_meter_add(sdrfm_audio_meter* acc, const sdrfm_audio_meter* m) {
  if (!acc || !m) return SDRFM_EINVAL;
  am_meter_join(acc, m);
  return SDRFM_OK;
}

static double db_of_power(double p) { return p > 0.0 ? 10.0 * log10(p) : -INFINITY; }

int sdrfm_audio_meter_report(const sdrfm_audio_meter* m, double fs_audio, sdrfm_audio_report_t* out) {
  if (!m || !out || !(isfinite(fs_audio) && fs_audio > 0.0)) return SDRFM_EINVAL;
  if (m->n == 0) {
    double* f = (double*)out;
    for (size_t k = 0; k < sizeof(*out) / sizeof(double); ++k) f[k] = NAN;
    return SDRFM_OK;
  }
  const double n = (double)m->n, fsq = 32768.0 * 32768.0;
  const double sl = (double)m->sq_l, sr = (double)m->sq_r, cr = (double)m->cross;
  const double mid = (sl + sr + 2.0 * cr) / 4.0, side = (sl + sr - 2.0 * cr) / 4.0;
  out->rms_l_dbfs = db_of_power(sl / n / fsq);
  out->rms_r_dbfs = db_of_power(sr / n / fsq);
  out->peak_l_dbfs = m->peak_l ? 20.0 * log10((double)m->peak_l / 32768.0) : -INFINITY;
  out->peak_r_dbfs = m->peak_r ? 20.0 * log10((double)m->peak_r / 32768.0) : -INFINITY;
  out->dc_l = (double)m->sum_l / n;
  out->dc_r = (double)m->sum_r / n;
  out->rail_l = (double)m->clip_l / n;
  out->rail_r = (double)m->clip_r / n;
  out->quiet_l = (double)m->quiet_l.count / n;
  out->quiet_r = (double)m->quiet_r.count / n;
  out->quiet_both = (double)m->quiet_both.count / n;
  out->longest_l_s = (double)m->quiet_l.longest / fs_audio;
  out->longest_r_s = (double)m->quiet_r.longest / fs_audio;
  out->longest_both_s = (double)m->quiet_both.longest / fs_audio;
  out->trail_l_s = (double)m->quiet_l.trail / fs_audio;
  out->trail_r_s = (double)m->quiet_r.trail / fs_audio;
  out->trail_both_s = (double)m->quiet_both.trail / fs_audio;
  out->correlation = (m->sq_l && m->sq_r) ? cr / sqrt(sl * sr) : NAN;
  out->mid_dbfs = db_of_power(mid / n / fsq);
  out->side_dbfs = db_of_power(side / n / fsq);
  out->side_mid_db = (mid > 0.0 || side > 0.0) ? db_of_power(side) - db_of_power(mid) : NAN;
  return SDRFM_OK;
}
