/*
 * sdrfm_limit.h — the per-stream look-ahead PCM limiter (include/sdrfm.h): the one copy of the per-pair arithmetic, the
 * (min, +) maps of the release, the window steps, the record join and the launch geometry that the kernel, csrc/limit.c and the CPU checks all
 * use, and the kernel's body.  The true-peak form (csrc/limit_tp.c) shares all of it and adds the interpolator's stage: the
 * kernel's body is one template with two instances.
 *
 * The release r[u] = min(256 m[u], r[u - 1] + delta) is the map f(r) = min(a, r + b) with a = 256 m[u], b = delta.  Two such maps compose to
 * one of the same form, (a2, b2) o (a1, b1) = (min(a2, a1 + b2), b1 + b2), and composition of maps is associative, so a run of pairs is one
 * map and the recurrence scans exactly in any grouping.  Every r lies in [0, 2^23] and every a in [0, 2^23], so a map whose b has reached
 * 2^23 answers a whatever r is: b is CLAMPED to 2^23, which changes no value and keeps every composed b inside 32 bits.  (2^23, 0) is the
 * identity on that range.
 *
 * The window minimum and the window sum over W = 2^LW entries are LW doubling steps each: after step k entry i covers [i - 2^(k+1) + 1, i].
 *
 * The first part is plain C99 integers, no HIP types: csrc/limit.c and tests/native/limit_check.cpp compile it with a host compiler alone.
 * The kernel's body follows under __HIPCC__.  Internal to the library; the drop-in boundary is include/sdrfm.h.
 */
#ifndef SDRFM_LIMIT_H
#define SDRFM_LIMIT_H

#include <stdint.h>

#include "../../include/sdrfm.h"
#include "sdrfm_audio_ctl.h"
#include "sdrfm_truepeak.h"

#if defined(__HIPCC__)
#define SDRFM_LIMIT_FN __host__ __device__ __forceinline__
#else
#define SDRFM_LIMIT_FN static inline
#endif

#define SDRFM_LIMIT_NT 1024u                       /* lanes of a stream's workgroup: sixteen waves, four per SIMD */
#define SDRFM_LIMIT_CHUNK 5u                       /* consecutive pairs a lane composes in the release: odd, so that the lanes' chunks start on different LDS banks */
#define SDRFM_LIMIT_TILE SDRFM_PCM_LIMIT_TILE      /* pairs of a tile: a call of a tenth of a second at 48 kHz is one tile */
#define SDRFM_LIMIT_LW_MIN 2u
#define SDRFM_LIMIT_LW_MAX 8u
#define SDRFM_LIMIT_D_MAX ((1u << SDRFM_LIMIT_LW_MAX) - 1u)
#define SDRFM_LIMIT_N_MAX (1u << 20)               /* pairs per call */
#define SDRFM_LIMIT_ONE 32768u                     /* Q15 1.0: no reduction */
#define SDRFM_LIMIT_R_ONE (1u << 23)               /* the same in the release's Q23 */
#define SDRFM_LIMIT_GAIN_UNITY 4096u               /* Q12 1.0 */
#define SDRFM_LIMIT_GAIN_MAX 65536u                /* Q12 16.0 */
#define SDRFM_LIMIT_SLEW_MAX 32768u
#define SDRFM_LIMIT_CEILING_MAX 32767u
#define SDRFM_LIMIT_CEILING_DEFAULT 29204u         /* floor(32768 10^(-1/20)) */
#define SDRFM_LIMIT_RELEASE_DEFAULT 874u           /* 2^23 / 874 = 9598 pairs: 0.2 s at 48 kHz */
/* an LDS array of the kernel: a tile behind its lead-in, rounded up */
#define SDRFM_LIMIT_ARRAY (SDRFM_LIMIT_TILE + SDRFM_LIMIT_D_MAX + 1u)

/* the true-peak form: H = NT / 2 more pairs of lead-in in front of the x' planes, and the packed table */
#define SDRFM_LIMIT_H_MAX (SDRFM_TP_TAPS_MAX / 2u)
#define SDRFM_LIMIT_ARRAY_TP (SDRFM_LIMIT_ARRAY + SDRFM_LIMIT_H_MAX)

#if SDRFM_LIMIT_TILE != SDRFM_LIMIT_NT * SDRFM_LIMIT_CHUNK
#error "a tile is one chunk per lane"
#endif

SDRFM_LIMIT_FN uint32_t limit_state_words(uint32_t lw) { return 4u * ((1u << lw) - 1u); }

SDRFM_LIMIT_FN int limit_shape_ok(uint32_t lw, uint32_t slew) {
  return lw >= SDRFM_LIMIT_LW_MIN && lw <= SDRFM_LIMIT_LW_MAX && slew >= 1u && slew <= SDRFM_LIMIT_SLEW_MAX;
}

SDRFM_LIMIT_FN int limit_params_ok(const sdrfm_pcm_limit_params* p) {
  return p->ceiling >= 1u && p->ceiling <= SDRFM_LIMIT_CEILING_MAX && p->release >= 1u && p->release <= SDRFM_LIMIT_R_ONE &&
         p->gain0 <= SDRFM_LIMIT_GAIN_MAX && p->gain_t <= SDRFM_LIMIT_GAIN_MAX;
}

/* step 1: one sample under the make-up gain G <= 65536 in Q12.  |x G| <= 2^31 and only -32768 x 65536 reaches it: inside an int32 with the
 * rounding constant added.  |result| <= 2^19 */
SDRFM_LIMIT_FN int32_t limit_gain(int16_t x, uint32_t G) { return ((int32_t)x * (int32_t)G + 2048) >> 12; }

/* step 2: the gain in Q15 that brings the pair under the ceiling C: C 32768 < 2^30 */
SDRFM_LIMIT_FN uint32_t limit_detect(int32_t xl, int32_t xr, uint32_t C) {
  const uint32_t al = (uint32_t)(xl < 0 ? -xl : xl), ar = (uint32_t)(xr < 0 ? -xr : xr), a = al > ar ? al : ar;
  return a <= C ? SDRFM_LIMIT_ONE : (C << 15) / a;
}

/* The true-peak form.  The window has to hold half a row, 2^LW >= NT / 2: then D + H >= NT - 1 and the x' delay line is the interpolator's
 * history as well.  State: x' of the last D + H pairs, then g and r of the last D detector pairs: 4 D + 2 H = 4 D + NT words. */
SDRFM_LIMIT_FN int limit_tp_window_ok(uint32_t lw, uint32_t n_taps) { return (1u << lw) >= n_taps / 2u; }
SDRFM_LIMIT_FN uint32_t limit_tp_state_words(uint32_t lw, uint32_t n_taps) { return 4u * ((1u << lw) - 1u) + n_taps; }
SDRFM_LIMIT_FN uint32_t limit_tp_latency(uint32_t lw, uint32_t n_taps) { return (1u << lw) - 1u + n_taps / 2u; }

/* step 1b: one pair's P phases of both channels.  xl, xr: the x' planes at the window's first (oldest) sample, n_taps entries of either are
 * read; tab: tp_pack_table's table, tap-reversed, two taps per dword.  |x'| <= 2^19 does not fit the true-peak meter's packed 16-bit dot
 * products; the products are taken as plain 64-bit multiply-adds (v_mad_i64_i32 on the device), which measured faster here than two packed
 * passes over the digits of x' (DESIGN.md §4.25).  |a| <= 2 * 65535 * 2^19 < 2^36.  P is a constant where the kernel calls this, so the phase
 * loops unroll and the accumulators stay in registers. */
SDRFM_LIMIT_FN void limit_tp_values(const int32_t* xl, const int32_t* xr, const uint32_t* tab, uint32_t P, uint32_t n_taps,
                                    int64_t a[2][SDRFM_TP_PHASES_MAX]) {
  const uint32_t rowdw = n_taps / 2u;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t p = 0; p < SDRFM_TP_PHASES_MAX; ++p) a[0][p] = a[1][p] = 0;
  for (uint32_t d = 0; d < rowdw; ++d) {
    const int32_t l0 = xl[2u * d], l1 = xl[2u * d + 1u], r0 = xr[2u * d], r1 = xr[2u * d + 1u];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t p = 0; p < SDRFM_TP_PHASES_MAX; ++p)
      if (p < P) {
        const uint32_t k = tab[p * rowdw + d];
        const int32_t c0 = (int16_t)(k & 0xFFFFu), c1 = (int16_t)(k >> 16);
        a[0][p] += (int64_t)c0 * l0 + (int64_t)c1 * l1;
        a[1][p] += (int64_t)c0 * r0 + (int64_t)c1 * r1;
      }
  }
}

/* T: the largest |A| of the pair, < 2^36 */
SDRFM_LIMIT_FN uint64_t limit_tp_peak(const int32_t* xl, const int32_t* xr, const uint32_t* tab, uint32_t P, uint32_t n_taps) {
  int64_t a[2][SDRFM_TP_PHASES_MAX];
  limit_tp_values(xl, xr, tab, P, n_taps, a);
  uint64_t T = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t p = 0; p < SDRFM_TP_PHASES_MAX; ++p)
    if (p < P) {
      const uint64_t l = tp_abs(a[0][p]), r = tp_abs(a[1][p]);
      T = l > T ? l : T;
      T = r > T ? r : T;
    }
  return T;
}

/* step 2': the detector pair's samples and the oversampled peak T (units of 2^-15 LSB) rounded UP to an LSB; a < 2^22 */
SDRFM_LIMIT_FN uint32_t limit_detect_tp(int32_t xl, int32_t xr, uint64_t T, uint32_t C) {
  const uint32_t al = (uint32_t)(xl < 0 ? -xl : xl), ar = (uint32_t)(xr < 0 ? -xr : xr), at = (uint32_t)((T + 32767u) >> 15);
  uint32_t a = al > ar ? al : ar;
  a = at > a ? at : a;
  return a <= C ? SDRFM_LIMIT_ONE : (C << 15) / a;
}

/* step 5's shift and step 6: the delayed sample under the smoothed gain s <= 32768.  |x s| <= 2^34 */
SDRFM_LIMIT_FN uint32_t limit_smooth(uint32_t S, uint32_t lw) { return S >> (lw + 8u); }
SDRFM_LIMIT_FN int16_t limit_out(int32_t x, uint32_t s) { return (int16_t)(((int64_t)x * (int64_t)s + 16384) >> 15); }

/* the release's maps */
typedef struct limit_map { uint32_t a, b; } limit_map;

SDRFM_LIMIT_FN limit_map limit_map_identity(void) { limit_map f; f.a = SDRFM_LIMIT_R_ONE; f.b = 0u; return f; }
/* the map of one pair whose window minimum is m (Q15) */
SDRFM_LIMIT_FN limit_map limit_map_of(uint32_t m, uint32_t delta) { limit_map f; f.a = 256u * m; f.b = delta; return f; }
SDRFM_LIMIT_FN uint32_t limit_apply(limit_map f, uint32_t r) { const uint32_t v = r + f.b; return f.a < v ? f.a : v; }
/* second after first */
SDRFM_LIMIT_FN limit_map limit_compose(limit_map second, limit_map first) {
  limit_map f;
  const uint32_t a = first.a + second.b, b = first.b + second.b;   /* each term <= 2^23 */
  f.a = second.a < a ? second.a : a;
  f.b = b < SDRFM_LIMIT_R_ONE ? b : SDRFM_LIMIT_R_ONE;
  return f;
}

/* one doubling step at entry i of an array whose entries each cover the span entries that end there */
SDRFM_LIMIT_FN uint32_t limit_win_min(const uint32_t* src, uint32_t i, uint32_t span) {
  const uint32_t v = src[i];
  if (i < span) return v;
  const uint32_t w = src[i - span];
  return w < v ? w : v;
}
SDRFM_LIMIT_FN uint32_t limit_win_sum(const uint32_t* src, uint32_t i, uint32_t span) { return i < span ? src[i] : src[i] + src[i - span]; }

/* the smallest gain and, among equals, the earliest pair: the smaller key */
SDRFM_LIMIT_FN uint64_t limit_key(uint32_t s, uint32_t i) { return ((uint64_t)s << 32) | i; }
SDRFM_LIMIT_FN uint64_t limit_key_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
SDRFM_LIMIT_FN uint64_t limit_key_none(void) { return limit_key(SDRFM_LIMIT_ONE, 0xFFFFFFFFu); }
SDRFM_LIMIT_FN void limit_rec_of(uint64_t key, uint64_t n, uint64_t limited, sdrfm_pcm_limit_rec* m) {
  m->n = n;
  m->limited = limited;
  m->min_gain = key >> 32;
  m->at = (key >> 32) < SDRFM_LIMIT_ONE ? (uint64_t)(uint32_t)key : 0u;
}

/* the ordered join of include/sdrfm.h: *acc then *m, into *acc */
SDRFM_LIMIT_FN void limit_join(sdrfm_pcm_limit_rec* acc, const sdrfm_pcm_limit_rec* m) {
  if (m->min_gain < acc->min_gain) { acc->min_gain = m->min_gain; acc->at = acc->n + m->at; }
  acc->n += m->n;
  acc->limited += m->limited;
}

/* the launch geometry: the tiles of a call and the kernel's dynamic LDS — x' in two planes, two work arrays, the waves' maps, keys and counts */
SDRFM_LIMIT_FN uint32_t limit_tiles(uint32_t n) { return (n + SDRFM_LIMIT_TILE - 1u) / SDRFM_LIMIT_TILE; }
SDRFM_LIMIT_FN uint32_t limit_lds_bytes(void) { return 4u * 4u * SDRFM_LIMIT_ARRAY + (SDRFM_LIMIT_NT / 64u) * (8u + 8u + 8u); }
/* the true-peak form: the x' planes are longer, and the packed table lies behind the counts */
SDRFM_LIMIT_FN uint32_t limit_tp_lds_bytes(void) {
  return 4u * 2u * (SDRFM_LIMIT_ARRAY_TP + SDRFM_LIMIT_ARRAY) + (SDRFM_LIMIT_NT / 64u) * (8u + 8u + 8u) + 4u * SDRFM_TP_TABLE_DWORDS;
}

#if defined(__HIPCC__)

struct LimitParams {
  const int16_t* in;
  size_t in_stride;                /* int16 elements per stream, even; rows are 4-byte aligned */
  int16_t* out;                    /* may be in */
  size_t out_stride;
  const sdrfm_pcm_limit_params* par;   /* [n_streams] */
  int32_t* state;                  /* [n_streams][4 D] */
  sdrfm_pcm_limit_rec* rec;        /* [n_streams] */
  uint32_t n, lw, slew, J;
};

/* the true-peak form's launch: the state is [n_streams][4 D + NT] */
struct LimitTpParams : LimitParams {
  const unsigned* table;           /* [P][nt / 2] dwords, tp_pack_table's */
  uint32_t nt, P;
};

__device__ __forceinline__ limit_map limit_shfl_up(limit_map f, int d) {
  limit_map g;
  g.a = (uint32_t)__shfl_up((int)f.a, d);
  g.b = (uint32_t)__shfl_up((int)f.b, d);
  return g;
}

/* One workgroup of SDRFM_LIMIT_NT lanes per stream, the row in tiles of SDRFM_LIMIT_TILE pairs.  lds: xl, xr (x' behind D pairs of lead-in), two
 * work arrays of the same length, then per wave a map, a key and a count.  Lanes t < D carry the lead-in of the next tile — the last D entries
 * of x', g and r — in registers: they are read from the state before the first barrier and written back behind the last, so nothing reads
 * state this launch has overwritten, and a tile's input is staged whole before any of its outputs is stored, so out may be in.
 *
 * TP is the true-peak form (Params = LimitTpParams): the x' planes lie behind LX = D + H pairs of lead-in (the lanes t < LX carry it), the packed
 * table lies in LDS behind the counts, and between steps 1 and 3 stage 1b / 2' takes each detector pair's gain from its own samples, at plane
 * entry D + j, and from the P phases over the NT entries that end at entry LX + j.  g, r and the windows are indexed by the detector pair, which
 * entry D + j of the work arrays is in both forms, and the output pair is plane entry j in both.  Where the two forms differ the sample form's
 * statements stand as they were, under if constexpr: k_pcm_limit compiles to the instructions it had before the template. */
template <uint32_t P, typename Params>
__device__ __forceinline__ void limit_tp_stage(const int32_t* xl, const int32_t* xr, uint32_t* wa, const uint32_t* tab, const Params& p, uint32_t D,
                                               uint32_t cnt, uint32_t C) {
  const uint32_t first = D + p.nt / 2u + 1u - p.nt;               /* the window of pair j starts at entry LX + j - (NT - 1) >= 0 */
  for (uint32_t j = threadIdx.x; j < cnt; j += SDRFM_LIMIT_NT) {  /* neighbouring lanes read neighbouring plane entries, every lane the same table dword */
    const uint64_t T = limit_tp_peak(xl + first + j, xr + first + j, tab, P, p.nt);
    wa[D + j] = limit_detect_tp(xl[D + j], xr[D + j], T, C);
  }
}

template <bool TP, typename Params>
__device__ __forceinline__ void limit_stream(unsigned* lds, const Params& p) {
  constexpr uint32_t AX = TP ? SDRFM_LIMIT_ARRAY_TP : SDRFM_LIMIT_ARRAY;
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6, n = p.n, lw = p.lw, D = (1u << lw) - 1u;
  if (n == 0) return;                                            /* uniform: the state and the record stay */
  uint32_t LX = D, H2 = 0;                                       /* the x' planes' lead-in, and 2 H: the state is 4 D + 2 H words */
  if constexpr (TP) { LX = D + p.nt / 2u; H2 = p.nt; }
  int32_t* const xl = reinterpret_cast<int32_t*>(lds);
  int32_t* const xr = xl + AX;
  uint32_t* const wa = lds + 2u * AX;
  uint32_t* const wb = wa + SDRFM_LIMIT_ARRAY;
  limit_map* const wmap = reinterpret_cast<limit_map*>(wb + SDRFM_LIMIT_ARRAY);
  uint64_t* const wkey = reinterpret_cast<uint64_t*>(wmap + SDRFM_LIMIT_NT / 64u);
  uint64_t* const wcnt = wkey + SDRFM_LIMIT_NT / 64u;
  [[maybe_unused]] uint32_t* const tab = reinterpret_cast<uint32_t*>(wcnt + SDRFM_LIMIT_NT / 64u);
  const sdrfm_pcm_limit_params par = p.par[blockIdx.x];
  const unsigned* row = reinterpret_cast<const unsigned*>(p.in + (size_t)blockIdx.x * p.in_stride);
  unsigned* orow = reinterpret_cast<unsigned*>(p.out + (size_t)blockIdx.x * p.out_stride);
  int32_t* st = p.state + (size_t)blockIdx.x * 4u * D;
  if constexpr (TP) st += (size_t)blockIdx.x * H2;
  int32_t tx_l = 0, tx_r = 0;
  uint32_t tg = 0, tr = 0;
  if constexpr (TP) {
    if (t < LX) { tx_l = st[2u * t]; tx_r = st[2u * t + 1u]; }
    if (t < D) { tg = (uint32_t)st[2u * LX + t]; tr = (uint32_t)st[2u * LX + D + t]; }
  } else {
    if (t < D) { tx_l = st[2u * t]; tx_r = st[2u * t + 1u]; tg = (uint32_t)st[2u * D + t]; tr = (uint32_t)st[3u * D + t]; }
  }
  uint32_t carry = (uint32_t)st[4u * D - 1u + H2];               /* r[-1] */
  if constexpr (TP)
    for (uint32_t k = t; k < p.P * (p.nt / 2u); k += SDRFM_LIMIT_NT) tab[k] = p.table[k];   /* read behind the first tile's barrier */
  uint64_t key = limit_key_none();
  uint32_t limited = 0;
  for (uint32_t base = 0; base < n; base += SDRFM_LIMIT_TILE) {
    const uint32_t cnt = n - base < SDRFM_LIMIT_TILE ? n - base : SDRFM_LIMIT_TILE, len = D + cnt;
    if (base) __syncthreads();                                   /* the arrays are free again */
    if constexpr (TP) {
      if (t < LX) { xl[t] = tx_l; xr[t] = tx_r; }
      if (t < D) wa[t] = tg;
    } else {
      if (t < D) { xl[t] = tx_l; xr[t] = tx_r; wa[t] = tg; }
    }
    for (uint32_t j = t; j < cnt; j += SDRFM_LIMIT_NT) {         /* steps 1 and 2 */
      const unsigned d = row[base + j];
      const uint32_t G = audio_ctl_ramp(par.gain0, par.gain_t, p.slew, p.J + base + j + 1u);
      const int32_t l = limit_gain((int16_t)(d & 0xFFFFu), G), r = limit_gain((int16_t)(d >> 16), G);
      xl[LX + j] = l;
      xr[LX + j] = r;
      if constexpr (!TP) wa[D + j] = limit_detect(l, r, par.ceiling);
    }
    __syncthreads();
    if constexpr (!TP) {
      if (t < D) { tx_l = xl[cnt + t]; tx_r = xr[cnt + t]; tg = wa[cnt + t]; }
    } else {                                                     /* steps 1b and 2' */
      if (t < LX) { tx_l = xl[cnt + t]; tx_r = xr[cnt + t]; }
      switch (p.P) {
        case 2: limit_tp_stage<2>(xl, xr, wa, tab, p, D, cnt, par.ceiling); break;
        case 4: limit_tp_stage<4>(xl, xr, wa, tab, p, D, cnt, par.ceiling); break;
        default: limit_tp_stage<8>(xl, xr, wa, tab, p, D, cnt, par.ceiling); break;
      }
      __syncthreads();
      if (t < D) tg = wa[cnt + t];
    }
    uint32_t* src = wa;
    uint32_t* dst = wb;
    for (uint32_t k = 0; k < lw; ++k) {                          /* step 3: entry D + j ends as m[j] */
      for (uint32_t i = t; i < len; i += SDRFM_LIMIT_NT) dst[i] = limit_win_min(src, i, 1u << k);
      __syncthreads();
      uint32_t* const x = src; src = dst; dst = x;
    }
    /* step 4: the lane's chunk as one map, the maps scanned over the wave and the waves joined through LDS; r replaces m in place */
    uint32_t mv[SDRFM_LIMIT_CHUNK];
    limit_map f = limit_map_identity();
#pragma unroll
    for (uint32_t q = 0; q < SDRFM_LIMIT_CHUNK; ++q) {
      const uint32_t j = t * SDRFM_LIMIT_CHUNK + q;
      mv[q] = j < cnt ? src[D + j] : SDRFM_LIMIT_ONE;
      if (j < cnt) f = limit_compose(limit_map_of(mv[q], par.release), f);
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const limit_map below = limit_shfl_up(f, d);
      if (lane >= (uint32_t)d) f = limit_compose(f, below);
    }
    if (lane == 63u) wmap[w] = f;
    limit_map before = limit_shfl_up(f, 1);                      /* the lanes of this wave below this one */
    if (lane == 0) before = limit_map_identity();
    __syncthreads();
    limit_map pre = limit_map_identity(), tot = limit_map_identity();
    for (uint32_t v = 0; v < SDRFM_LIMIT_NT / 64u; ++v) {
      const limit_map m = wmap[v];
      if (v < w) pre = limit_compose(m, pre);
      tot = limit_compose(m, tot);
    }
    uint32_t r = limit_apply(before, limit_apply(pre, carry));
#pragma unroll
    for (uint32_t q = 0; q < SDRFM_LIMIT_CHUNK; ++q) {
      const uint32_t j = t * SDRFM_LIMIT_CHUNK + q;
      if (j < cnt) {
        r = limit_apply(limit_map_of(mv[q], par.release), r);
        src[D + j] = r;
      }
    }
    if (t < D) src[t] = tr;
    carry = limit_apply(tot, carry);
    __syncthreads();
    if (t < D) tr = src[cnt + t];
    for (uint32_t k = 0; k < lw; ++k) {                          /* step 5: entry D + j ends as S[j] */
      for (uint32_t i = t; i < len; i += SDRFM_LIMIT_NT) dst[i] = limit_win_sum(src, i, 1u << k);
      __syncthreads();
      uint32_t* const x = src; src = dst; dst = x;
    }
    for (uint32_t j = t; j < cnt; j += SDRFM_LIMIT_NT) {         /* step 6: x'[u - D] is entry j */
      const uint32_t s = limit_smooth(src[D + j], lw);
      const unsigned L = (uint16_t)limit_out(xl[j], s), R = (uint16_t)limit_out(xr[j], s);
      orow[base + j] = L | (R << 16);
      key = limit_key_min(key, limit_key(s, base + j));
      limited += s < SDRFM_LIMIT_ONE ? 1u : 0u;
    }
  }
  if constexpr (TP) {
    if (t < LX) { st[2u * t] = tx_l; st[2u * t + 1u] = tx_r; }
    if (t < D) { st[2u * LX + t] = (int32_t)tg; st[2u * LX + D + t] = (int32_t)tr; }
  } else {
    if (t < D) { st[2u * t] = tx_l; st[2u * t + 1u] = tx_r; st[2u * D + t] = (int32_t)tg; st[3u * D + t] = (int32_t)tr; }
  }
  uint64_t c = limited;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    key = limit_key_min(key, (uint64_t)__shfl_xor((long long)key, d));
    c += (uint64_t)__shfl_xor((long long)c, d);
  }
  if (lane == 0) { wkey[w] = key; wcnt[w] = c; }
  __syncthreads();
  if (t == 0) {                                                  /* the waves' keys and counts, then the call behind the stream's record */
    uint64_t kk = limit_key_none(), cc = 0;
    for (uint32_t v = 0; v < SDRFM_LIMIT_NT / 64u; ++v) { kk = limit_key_min(kk, wkey[v]); cc += wcnt[v]; }
    sdrfm_pcm_limit_rec call, acc = p.rec[blockIdx.x];
    limit_rec_of(kk, n, cc, &call);
    limit_join(&acc, &call);
    p.rec[blockIdx.x] = acc;
  }
}

#endif /* __HIPCC__ */
#endif
