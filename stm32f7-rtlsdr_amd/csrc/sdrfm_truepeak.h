/*
 * sdrfm_truepeak.h — the stereo PCM sink's per-stream true-peak meter (include/sdrfm.h): the one copy of the table packing,
 * the lane's dot-product order, the key reduction and the join that the kernel, csrc/truepeak.c and the CPU checks all use, and the kernel's
 * body.
 *
 * A[i][p] = sum over k of coef[p][k] x[i - k] is taken over the NT samples x[i - NT + 1 .. i] in ascending order, so the table is held
 * TAP-REVERSED and packed two taps per dword: dword d of row p is coef[p][NT - 1 - 2d] | coef[p][NT - 2 - 2d] << 16.  The samples of one
 * channel lie packed two per dword in a plane that starts at an even sample; a window that starts at an odd sample forms each operand from two
 * neighbouring dwords by a 64-bit shift.  The first NT / 4 dwords of a row are the taps [NT/2, NT), the others the taps [0, NT/2): each half's
 * dot product fits an int32 by the half-row bound, and the two halves are added in 64 bits.
 *
 * A lane's peaks are kept as one 64-bit key per channel, peak << 32 | (0xFFFFFFFF - pair index): the larger key is the larger peak and, among
 * equal peaks, the earlier pair, so max over keys is commutative and the order of lanes, waves and tiles does not matter.
 *
 * The first part is plain C99 integers, no HIP types: csrc/truepeak.c and tests/native/truepeak_check.cpp compile it with a host compiler
 * alone.  The kernel's body follows under __HIPCC__.  Internal to the library; the drop-in boundary is include/sdrfm.h.
 */
#ifndef SDRFM_TRUEPEAK_H
#define SDRFM_TRUEPEAK_H

#include <stdint.h>

#include "../../include/sdrfm.h"

#if defined(__HIPCC__)
#define SDRFM_TP_FN __host__ __device__ __forceinline__
#else
#define SDRFM_TP_FN static inline
#endif

#define SDRFM_TP_NT 1024u                          /* lanes of a stream's workgroup: sixteen waves, four per SIMD (measured against 256 and 512) */
#define SDRFM_TP_TILE 4864u                        /* pairs of a tile, even: a call of a tenth of a second at 48 kHz is one tile */
#define SDRFM_TP_TAPS_MIN 4u
#define SDRFM_TP_TAPS_MAX 64u
#define SDRFM_TP_PHASES_MAX 8u
#define SDRFM_TP_HALF_MAX 65535u                   /* the sum of |coef| over half a row: 65535 * 32768 < 2^31 */
#define SDRFM_TP_LIMIT_MAX 0xFFFFFFFFull
#define SDRFM_TP_TABLE_DWORDS (SDRFM_TP_PHASES_MAX * SDRFM_TP_TAPS_MAX / 2u)
/* a plane: the tile's pairs and the NT before them, two per dword, and the dword a lane fetches beyond its taps */
#define SDRFM_TP_PLANE_DWORDS (SDRFM_TP_TILE / 2u + SDRFM_TP_TAPS_MAX / 2u + 1u)

SDRFM_TP_FN int tp_shape_ok(uint32_t n_phases, uint32_t n_taps) {
  return (n_phases == 2u || n_phases == 4u || n_phases == 8u) && n_taps >= SDRFM_TP_TAPS_MIN && n_taps <= SDRFM_TP_TAPS_MAX && n_taps % 4u == 0;
}

/* the table as the device holds it: n_phases rows of n_taps / 2 dwords, tap-reversed */
SDRFM_TP_FN void tp_pack_table(const int16_t* coef, uint32_t n_phases, uint32_t n_taps, uint32_t* out) {
  for (uint32_t p = 0; p < n_phases; ++p)
    for (uint32_t d = 0; d < n_taps / 2u; ++d) {
      const uint32_t lo = (uint16_t)coef[p * n_taps + (n_taps - 1u - 2u * d)], hi = (uint16_t)coef[p * n_taps + (n_taps - 2u - 2u * d)];
      out[p * (n_taps / 2u) + d] = lo | (hi << 16);
    }
}

/* two consecutive samples of one channel in a dword, the earlier one low */
SDRFM_TP_FN uint32_t tp_pack2(int16_t first, int16_t second) { return (uint32_t)(uint16_t)first | ((uint32_t)(uint16_t)second << 16); }

/* c + a.lo b.lo + a.hi b.hi on int16 halves, wrapping: exact whenever the true sum fits an int32, which the half-row bound guarantees */
SDRFM_TP_FN int32_t tp_dot2(uint32_t a, uint32_t b, int32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef short tp_v2s __attribute__((ext_vector_type(2)));
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(tp_v2s, a), __builtin_bit_cast(tp_v2s, b), c, false);
#else
  const int32_t lo = (int32_t)(int16_t)(a & 0xFFFFu) * (int32_t)(int16_t)(b & 0xFFFFu);
  const int32_t hi = (int32_t)(int16_t)(a >> 16) * (int32_t)(int16_t)(b >> 16);
  return (int32_t)((uint32_t)c + (uint32_t)lo + (uint32_t)hi);
#endif
}

/* the operand that starts sh / 16 samples into lo: sh is 0 or 16 */
SDRFM_TP_FN uint32_t tp_operand(uint32_t lo, uint32_t hi, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> sh); }

/* One pair's P phases of both channels.  xl, xr: the planes at the dword that holds the window's first sample, q0 >> 1 for a window that starts
 * at plane sample q0; sh = 16 (q0 & 1); n_taps / 2 + 1 dwords of either are read.  tab: the packed table.  a[channel][phase] = A, exact under
 * the half-row bound.  P is a constant where the kernel calls this, so the phase loops unroll and acc stays in registers. */
SDRFM_TP_FN void tp_lane_pair(const uint32_t* xl, const uint32_t* xr, uint32_t sh, const uint32_t* tab, uint32_t P, uint32_t n_taps,
                              int64_t a[2][SDRFM_TP_PHASES_MAX]) {
  const uint32_t half = n_taps / 4u, rowdw = n_taps / 2u;
  uint32_t dl = xl[0], dr = xr[0], m = 0;
  for (uint32_t h = 0; h < 2u; ++h) {
    int32_t acc[2][SDRFM_TP_PHASES_MAX];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t p = 0; p < SDRFM_TP_PHASES_MAX; ++p) acc[0][p] = acc[1][p] = 0;
    const uint32_t end = m + half;
    for (; m < end; ++m) {
      const uint32_t nl = xl[m + 1u], nr = xr[m + 1u];
      const uint32_t vl = tp_operand(dl, nl, sh), vr = tp_operand(dr, nr, sh);
#if defined(__HIPCC__)
#pragma unroll
#endif
      for (uint32_t p = 0; p < SDRFM_TP_PHASES_MAX; ++p)
        if (p < P) {
          const uint32_t k = tab[p * rowdw + m];
          acc[0][p] = tp_dot2(vl, k, acc[0][p]);
          acc[1][p] = tp_dot2(vr, k, acc[1][p]);
        }
      dl = nl;
      dr = nr;
    }
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t p = 0; p < SDRFM_TP_PHASES_MAX; ++p)
      if (p < P) {
        a[0][p] = h ? a[0][p] + acc[0][p] : (int64_t)acc[0][p];
        a[1][p] = h ? a[1][p] + acc[1][p] : (int64_t)acc[1][p];
      }
  }
}

SDRFM_TP_FN uint64_t tp_abs(int64_t v) { return (uint64_t)(v < 0 ? -v : v); }

/* the key of a value |A| < 2^32 at call-local pair i < 2^32, the larger of two keys, and a key's two halves back */
SDRFM_TP_FN uint64_t tp_key(uint64_t mag, uint32_t i) { return (mag << 32) | (uint64_t)(0xFFFFFFFFu - i); }
SDRFM_TP_FN uint64_t tp_key_max(uint64_t a, uint64_t b) { return a > b ? a : b; }
SDRFM_TP_FN uint64_t tp_key_peak(uint64_t key) { return key >> 32; }
SDRFM_TP_FN uint64_t tp_key_at(uint64_t key) { return (key >> 32) ? (uint64_t)(0xFFFFFFFFu - (uint32_t)key) : 0u; }

/* one pair's P values of one channel into a lane's key and count */
SDRFM_TP_FN void tp_take(const int64_t* a, uint32_t P, uint32_t i, uint64_t limit, uint64_t* key, uint32_t* over) {
  uint64_t mag = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (uint32_t p = 0; p < SDRFM_TP_PHASES_MAX; ++p)
    if (p < P) {
      const uint64_t v = tp_abs(a[p]);
      mag = v > mag ? v : mag;
      *over += v > limit ? 1u : 0u;
    }
  *key = tp_key_max(*key, tp_key(mag, i));
}

/* the ordered join of include/sdrfm.h: *acc then *m, into *acc */
SDRFM_TP_FN void tp_join(sdrfm_truepeak* acc, const sdrfm_truepeak* m) {
  if (m->peak_l > acc->peak_l) { acc->peak_l = m->peak_l; acc->at_l = acc->n + m->at_l; }
  if (m->peak_r > acc->peak_r) { acc->peak_r = m->peak_r; acc->at_r = acc->n + m->at_r; }
  acc->n += m->n;
  acc->over_l += m->over_l;
  acc->over_r += m->over_r;
  acc->reserved += m->reserved;
}

#if defined(__HIPCC__)

struct TruePeakParams {
  const int16_t* pcm;
  size_t pcm_stride;               /* int16 elements per stream, even; rows are 4-byte aligned */
  sdrfm_truepeak* rec;             /* [n_streams] */
  unsigned* hist;                  /* [n_streams][nt - 1] pairs, L | R << 16, oldest first */
  const unsigned* table;           /* [P][nt / 2] dwords, tp_pack_table's */
  uint64_t limit;
  uint32_t n, nt, P;
};

struct TruePeakShared {
  unsigned tab[SDRFM_TP_TABLE_DWORDS];
  unsigned pl[SDRFM_TP_PLANE_DWORDS], pr[SDRFM_TP_PLANE_DWORDS];
  uint64_t key[2][SDRFM_TP_NT / 64u], over[2][SDRFM_TP_NT / 64u];
};

/* pair idx of a stream's input as the call sees it: the history below 0, zero outside [-(nt - 1), n) */
__device__ __forceinline__ unsigned tp_fetch(const unsigned* row, const unsigned* hist, int64_t idx, uint32_t n, uint32_t nt) {
  if (idx >= 0) return idx < (int64_t)n ? row[idx] : 0u;
  return idx >= -(int64_t)(nt - 1u) ? hist[(int64_t)(nt - 1u) + idx] : 0u;
}

__device__ __forceinline__ uint64_t tp_wave_max(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = tp_key_max(v, (uint64_t)__shfl_xor((long long)v, d));
  return v;
}

__device__ __forceinline__ uint64_t tp_wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((long long)v, d);
  return v;
}

/* a tile's pairs, lane t taking t, t + SDRFM_TP_NT, ...: neighbouring lanes read neighbouring plane dwords (two lanes share one), every lane the same
 * table dword */
template <uint32_t P>
__device__ __forceinline__ void tp_tile(const TruePeakShared& sh, uint32_t nt, uint32_t base, uint32_t cnt, uint64_t limit, uint64_t key[2], uint32_t over[2]) {
  for (uint32_t r = threadIdx.x; r < cnt; r += SDRFM_TP_NT) {
    const uint32_t q0 = r + 1u;                                  /* the plane starts nt pairs before the tile: the window starts at r + 1 */
    int64_t a[2][SDRFM_TP_PHASES_MAX];
    tp_lane_pair(sh.pl + (q0 >> 1), sh.pr + (q0 >> 1), (q0 & 1u) * 16u, sh.tab, P, nt, a);
    tp_take(a[0], P, base + r, limit, &key[0], &over[0]);
    tp_take(a[1], P, base + r, limit, &key[1], &over[1]);
  }
}

/* One workgroup of SDRFM_TP_NT lanes per stream.  The stream's new history is read before the first barrier and written behind it, when the
 * first tile's lead-in has been staged from the old one: nothing reads history this launch has overwritten. */
__device__ __forceinline__ void truepeak_stream(TruePeakShared& sh, const TruePeakParams& p) {
  const uint32_t t = threadIdx.x, nt = p.nt, n = p.n;
  if (n == 0) return;                                            /* uniform: the record and the history stay */
  const unsigned* row = reinterpret_cast<const unsigned*>(p.pcm + (size_t)blockIdx.x * p.pcm_stride);
  unsigned* hist = p.hist + (size_t)blockIdx.x * (nt - 1u);
  for (uint32_t k = t; k < p.P * (nt / 2u); k += SDRFM_TP_NT) sh.tab[k] = p.table[k];
  unsigned newh = 0;
  if (t < nt - 1u) {
    const uint64_t c = (uint64_t)n + t;                          /* index into (history, new pairs) of the last nt - 1 of them */
    newh = c < nt - 1u ? hist[c] : row[c - (nt - 1u)];
  }
  uint64_t key[2] = {0, 0};
  uint32_t over[2] = {0, 0};
  for (uint64_t base = 0; base < n; base += SDRFM_TP_TILE) {
    if (base) __syncthreads();                                   /* the planes are free again */
    const uint32_t cnt = n - base < SDRFM_TP_TILE ? (uint32_t)(n - base) : SDRFM_TP_TILE;
    const int64_t a0 = (int64_t)base - (int64_t)nt;              /* even */
    const uint32_t need = (cnt >> 1) + nt / 2u + 1u;             /* <= SDRFM_TP_PLANE_DWORDS: a lane's last fetch is dword (cnt >> 1) + nt / 2 */
    for (uint32_t q = t; q < need; q += SDRFM_TP_NT) {
      const unsigned d0 = tp_fetch(row, hist, a0 + 2 * (int64_t)q, n, nt), d1 = tp_fetch(row, hist, a0 + 2 * (int64_t)q + 1, n, nt);
      sh.pl[q] = (d0 & 0xFFFFu) | (d1 << 16);
      sh.pr[q] = (d0 >> 16) | (d1 & 0xFFFF0000u);
    }
    __syncthreads();
    if (base == 0 && t < nt - 1u) hist[t] = newh;
    switch (p.P) {
      case 2: tp_tile<2>(sh, nt, (uint32_t)base, cnt, p.limit, key, over); break;
      case 4: tp_tile<4>(sh, nt, (uint32_t)base, cnt, p.limit, key, over); break;
      default: tp_tile<8>(sh, nt, (uint32_t)base, cnt, p.limit, key, over); break;
    }
  }
  const uint32_t w = t >> 6;
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    const uint64_t k = tp_wave_max(key[ch]), o = tp_wave_sum(over[ch]);
    if ((t & 63u) == 0) { sh.key[ch][w] = k; sh.over[ch][w] = o; }
  }
  __syncthreads();
  if (t == 0) {                                                  /* the waves' keys and counts, then the call behind the stream's record */
    uint64_t k[2] = {0, 0}, o[2] = {0, 0};
    for (uint32_t v = 0; v < SDRFM_TP_NT / 64u; ++v)
      for (int ch = 0; ch < 2; ++ch) { k[ch] = tp_key_max(k[ch], sh.key[ch][v]); o[ch] += sh.over[ch][v]; }
    sdrfm_truepeak call;
    call.n = n;
    call.peak_l = tp_key_peak(k[0]); call.at_l = tp_key_at(k[0]); call.over_l = o[0];
    call.peak_r = tp_key_peak(k[1]); call.at_r = tp_key_at(k[1]); call.over_r = o[1];
    call.reserved = 0;
    sdrfm_truepeak acc = p.rec[blockIdx.x];
    tp_join(&acc, &call);
    p.rec[blockIdx.x] = acc;
  }
}

#endif /* __HIPCC__ */
#endif
