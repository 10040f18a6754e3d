/*
 * loudness.c — the host side of the stereo PCM sink's K-weighted loudness meter (include/sdrfm.h), plain C99 with no GPU
 * behind it: the BS.1770-4 coefficients and their check, the sub-block energies of int16 stereo PCM one pair at a time
 * (sdrfm_pcm_loudness_s16: the definition as code, and what a board-side host runs), and the gate that turns consecutive sub-block energies
 * into momentary, short-term and integrated loudness and loudness range (sdrfm_loudness_gate_*).  Built with -ffp-contract=off: every
 * product and sum of the filter is rounded on its own.
 */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/sdrfm.h"
#include "sdrfm_loudness.h"

int sdrfm_loudness_default_coef(sdrfm_loudness_coef* out) {
  static const double K48[10] = {1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                                 1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621};
  if (!out) return SDRFM_EINVAL;
  memcpy(out->c, K48, sizeof(K48));
  return SDRFM_OK;
}

int sdrfm_loudness_check_coef(const sdrfm_loudness_coef* coef) {
  if (!coef) return SDRFM_EINVAL;
  for (int k = 0; k < 10; ++k)
    if (!isfinite(coef->c[k])) return SDRFM_EINVAL;
  for (int q = 0; q < 2; ++q) {
    const double a1 = coef->c[5 * q + 3], a2 = coef->c[5 * q + 4];
    if (!(fabs(a2) < 1.0) || !(fabs(a1) < 1.0 + a2)) return SDRFM_EINVAL;
  }
  return SDRFM_OK;
}

/* the sets the DEVICE may be enabled with (sdrfm_loudness.h: ld_probe).  This object, built with -ffp-contract=off, holds the one compiled copy of
 * the probe: the sink's enable calls it */
int sdrfm_loudness_check_domain(const sdrfm_loudness_coef* coef, double* rel, double* abs_per_sample) {
  if (sdrfm_loudness_check_coef(coef) != SDRFM_OK) return SDRFM_EINVAL;
  double pw[SDRFM_LD_TABLE];
  ld_matrix_powers(coef->c, pw);
  return ld_in_domain(coef->c, pw, rel, abs_per_sample) ? SDRFM_OK : SDRFM_EINVAL;
}

int sdrfm_pcm_loudness_s16(const int16_t* pcm_interleaved, uint32_t n, const sdrfm_loudness_coef* coef, uint32_t block_len,
                           sdrfm_loudness_state* state, sdrfm_loudness_block* out_blocks, uint32_t out_cap, uint32_t* n_blocks) {
  if (!state || !coef || !n_blocks || (!pcm_interleaved && n)) return SDRFM_EINVAL;
  if (sdrfm_loudness_check_coef(coef) != SDRFM_OK) return SDRFM_EINVAL;
  if (block_len < SDRFM_LD_BLOCK_MIN || block_len > SDRFM_LD_BLOCK_MAX) return SDRFM_EINVAL;
  const uint64_t done = ld_blocks_done(state->pos, n, block_len);
  if (done > out_cap) return SDRFM_ECAPACITY;
  if (done && !out_blocks) return SDRFM_EINVAL;
  sdrfm_loudness_state s = *state;
  uint32_t left = block_len - (uint32_t)(s.pos % block_len), k = 0;   /* pairs until the open sub-block is complete */
  for (uint32_t i = 0; i < n; ++i) {
    const double yl = ld_kw_step(coef->c, s.z[0], (double)pcm_interleaved[2 * (size_t)i]);
    const double yr = ld_kw_step(coef->c, s.z[1], (double)pcm_interleaved[2 * (size_t)i + 1]);
    s.e[0] = s.e[0] + yl * yl;
    s.e[1] = s.e[1] + yr * yr;
    if (--left == 0) {
      out_blocks[k].e_l = s.e[0];
      out_blocks[k].e_r = s.e[1];
      ++k;
      s.e[0] = s.e[1] = 0.0;
      left = block_len;
    }
  }
  s.pos += n;
  *state = s;
  *n_blocks = k;
  return SDRFM_OK;
}

/* ---- the gate ---------------------------------------------------------------------------------------------------------------------------- */
#define LG_BINS 800            /* 0.1 LU over -70 .. +10 LUFS */
#define LG_LO (-70.0)
#define LG_M 4                 /* sub-blocks of a momentary window and of a gating block */
#define LG_S 30                /* sub-blocks of a short-term window */

typedef struct lg_hist { uint64_t cnt[LG_BINS]; double sum[LG_BINS]; } lg_hist;

struct sdrfm_loudness_gate {
  uint32_t block_len;
  double scale;                /* 1 / (block_len 32768^2) */
  double z[LG_S];              /* the last 30 z, z[k % 30] */
  uint64_t n, n_gating, n_short;
  double m_pow, s_pow, max_m_pow, max_s_pow;   /* mean z of the last windows and the largest so far */
  lg_hist gating, shortterm;
};

static double lg_lufs(double pow_) { return pow_ > 0.0 ? -0.691 + 10.0 * log10(pow_) : -INFINITY; }

static int lg_bin(double lufs) {   /* lufs > -70 */
  const double b = floor((lufs - LG_LO) * 10.0);
  return b < 0.0 ? 0 : (b > LG_BINS - 1 ? LG_BINS - 1 : (int)b);
}

static void lg_add(lg_hist* h, double pow_) {
  const double l = lg_lufs(pow_);
  if (!(l > LG_LO)) return;                                       /* the absolute gate */
  const int b = lg_bin(l);
  ++h->cnt[b];
  h->sum[b] = h->sum[b] + pow_;
}

/* the oldest-to-newest mean of the last w z */
static double lg_window(const sdrfm_loudness_gate_t* g, int w) {
  double t = 0.0;
  for (uint64_t k = g->n - (uint64_t)w; k < g->n; ++k) t = t + g->z[k % LG_S];
  return t / w;
}

/* the bins a relative gate `drop` LU below the histogram's power mean keeps: from *first on.  Returns the entries past the absolute gate */
static uint64_t lg_relative(const lg_hist* h, double drop, int* first) {
  uint64_t cnt = 0;
  double sum = 0.0;
  for (int b = 0; b < LG_BINS; ++b) { cnt += h->cnt[b]; sum = sum + h->sum[b]; }
  *first = 0;
  if (cnt) {
    const double gate = lg_lufs(sum / (double)cnt) - drop;
    *first = gate > LG_LO ? lg_bin(gate) : 0;                     /* at a bin edge: the bin that holds the gate is kept whole */
  }
  return cnt;
}

/* the mean loudness of the bin that holds the element of 0-based rank r among the bins from `first` on */
static double lg_rank(const lg_hist* h, int first, uint64_t r) {
  uint64_t cum = 0;
  for (int b = first; b < LG_BINS; ++b) {
    cum += h->cnt[b];
    if (cum > r) return lg_lufs(h->sum[b] / (double)h->cnt[b]);
  }
  return NAN;
}

int sdrfm_loudness_gate_create(uint32_t block_len, sdrfm_loudness_gate_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = NULL;
  if (block_len < SDRFM_LD_BLOCK_MIN || block_len > SDRFM_LD_BLOCK_MAX) return SDRFM_EINVAL;
  sdrfm_loudness_gate_t* g = (sdrfm_loudness_gate_t*)calloc(1, sizeof(*g));
  if (!g) return SDRFM_ENOMEM;
  g->block_len = block_len;
  g->scale = 1.0 / ((double)block_len * 32768.0 * 32768.0);
  *out = g;
  return SDRFM_OK;
}

void sdrfm_loudness_gate_free(sdrfm_loudness_gate_t* g) { free(g); }

int sdrfm_loudness_gate_reset(sdrfm_loudness_gate_t* g) {
  if (!g) return SDRFM_EINVAL;
  const uint32_t block_len = g->block_len;
  const double scale = g->scale;
  memset(g, 0, sizeof(*g));
  g->block_len = block_len;
  g->scale = scale;
  return SDRFM_OK;
}

int sdrfm_loudness_gate_push(sdrfm_loudness_gate_t* g, const sdrfm_loudness_block* blocks, uint32_t n) {
  if (!g || (!blocks && n)) return SDRFM_EINVAL;
  for (uint32_t k = 0; k < n; ++k)
    if (!isfinite(blocks[k].e_l) || !isfinite(blocks[k].e_r) || blocks[k].e_l < 0.0 || blocks[k].e_r < 0.0) return SDRFM_EINVAL;
  for (uint32_t k = 0; k < n; ++k) {
    g->z[g->n % LG_S] = (blocks[k].e_l + blocks[k].e_r) * g->scale;
    ++g->n;
    if (g->n >= LG_M) {
      g->m_pow = lg_window(g, LG_M);
      if (g->n_gating == 0 || g->m_pow > g->max_m_pow) g->max_m_pow = g->m_pow;
      ++g->n_gating;
      lg_add(&g->gating, g->m_pow);
    }
    if (g->n >= LG_S) {
      g->s_pow = lg_window(g, LG_S);
      if (g->n_short == 0 || g->s_pow > g->max_s_pow) g->max_s_pow = g->s_pow;
      ++g->n_short;
      lg_add(&g->shortterm, g->s_pow);
    }
  }
  return SDRFM_OK;
}

int sdrfm_loudness_gate_report(const sdrfm_loudness_gate_t* g, sdrfm_loudness_report_t* out) {
  if (!g || !out) return SDRFM_EINVAL;
  memset(out, 0, sizeof(*out));
  out->n_blocks = g->n;
  out->n_gating = g->n_gating;
  out->n_short = g->n_short;
  out->m = g->n_gating ? lg_lufs(g->m_pow) : NAN;
  out->max_m = g->n_gating ? lg_lufs(g->max_m_pow) : NAN;
  out->s = g->n_short ? lg_lufs(g->s_pow) : NAN;
  out->max_s = g->n_short ? lg_lufs(g->max_s_pow) : NAN;
  int first;
  out->n_abs = lg_relative(&g->gating, 10.0, &first);
  double sum = 0.0;
  for (int b = first; b < LG_BINS; ++b) { out->n_rel += g->gating.cnt[b]; sum = sum + g->gating.sum[b]; }
  out->i = !g->n_gating ? NAN : (out->n_rel ? lg_lufs(sum / (double)out->n_rel) : -INFINITY);
  out->n_short_abs = lg_relative(&g->shortterm, 20.0, &first);
  for (int b = first; b < LG_BINS; ++b) out->n_short_rel += g->shortterm.cnt[b];
  if (!out->n_short_rel) out->lra = NAN;
  else {
    const double span = (double)(out->n_short_rel - 1u);
    out->lra = lg_rank(&g->shortterm, first, (uint64_t)floor(span * 0.95 + 0.5)) - lg_rank(&g->shortterm, first, (uint64_t)floor(span * 0.10 + 0.5));
  }
  return SDRFM_OK;
}
