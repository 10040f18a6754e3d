/*
 * sdrfm_pcm_rate.h — the per-stream PCM rate matcher (include/sdrfm.h): the one copy of the count, advance and span arithmetic
 * that the host code, the kernel, csrc/pcm_rate.c and the CPU checks all use, and the kernel's body.
 *
 * A stream resamples int16 stereo pairs by a 32.32 fixed-point step through a polyphase table with linear interpolation between neighbouring
 * rows.  Everything is integers: how many outputs a call of n pairs yields (rate_count), where the phase accumulator stands afterwards
 * (rate_advance) and which outputs and which input window a workgroup takes (rate_span) are closed forms of (pos, step, n).
 *
 * The first part is plain C99 integers, no HIP types: csrc/pcm_rate.c and tests/native/pcm_rate_check.cpp compile it with a host compiler
 * alone.  The kernel's body follows under __HIPCC__.  Internal to the library; the drop-in boundary is include/sdrfm.h.
 */
#ifndef SDRFM_PCM_RATE_H
#define SDRFM_PCM_RATE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SDRFM_RATE_FN __host__ __device__ __forceinline__
#else
#define SDRFM_RATE_FN static inline
#endif

#define SDRFM_RATE_NT 256u                         /* lanes of a workgroup: four waves */
#define SDRFM_RATE_STEP_MIN ((uint64_t)1 << 30)    /* 1/4 input pair per output pair */
#define SDRFM_RATE_STEP_MAX ((uint64_t)1 << 34)    /* 4 input pairs per output pair */
#define SDRFM_RATE_N_MAX (1u << 20)                /* pairs per call */
#define SDRFM_RATE_TAPS_MIN 4u
#define SDRFM_RATE_TAPS_MAX 64u
#define SDRFM_RATE_LOGPH_MIN 4u
#define SDRFM_RATE_LOGPH_MAX 8u
#define SDRFM_RATE_HALF_MAX 65535u                 /* the sum of |coef| over half a row: 65535 * 32768 < 2^31 */
#define SDRFM_RATE_SPAN_MAX 1024u                  /* outputs of a workgroup at most: four per lane (measured against 256 .. 2048) */
#define SDRFM_RATE_LDS_BYTES 65536u                /* the table and a span's window together */

/* the outputs of a call of n <= 2^20 new pairs: the j >= 0 with pos + j step < n 2^32.  step >= 2^30 */
SDRFM_RATE_FN uint32_t rate_count(uint64_t pos, uint64_t step, uint32_t n) {
  const uint64_t N = (uint64_t)n << 32;
  return pos >= N ? 0u : (uint32_t)((N - pos + step - 1u) / step);   /* < 2^52 + 2^34: no wrap; the quotient is <= 2^22 */
}

/* pos of the next call, measured against ITS first new pair; cnt = rate_count(pos, step, n) */
SDRFM_RATE_FN uint64_t rate_advance(uint64_t pos, uint64_t step, uint32_t n, uint32_t cnt) {
  return pos + (uint64_t)cnt * step - ((uint64_t)n << 32);
}

/* the dwords of a table row as the device holds it: NT / 2 tap pairs and one of padding, which makes the stride odd */
SDRFM_RATE_FN uint32_t rate_row_dwords(uint32_t nt) { return nt / 2u + 1u; }
/* ... and of the table, rounded up to whole 16-byte words: it is staged four dwords at a time */
SDRFM_RATE_FN uint32_t rate_table_dwords(uint32_t nt, uint32_t logph) { return (((1u << logph) + 1u) * rate_row_dwords(nt) + 3u) & ~3u; }

/* the dwords of one channel's plane that hold any window of span outputs at step: the window is i_last - i_first + NT pairs,
 * i_last - i_first <= ((span - 1) step >> 32) + 1; one pair more when the window starts at an odd index, and one dword more because a lane
 * always fetches NT / 2 + 1 dwords */
SDRFM_RATE_FN uint32_t rate_plane_dwords(uint32_t span, uint64_t step, uint32_t nt) {
  const uint64_t w = (((uint64_t)(span - 1u) * step) >> 32) + 1u + nt;
  return (uint32_t)((w + 2u) / 2u + 1u);
}

SDRFM_RATE_FN uint32_t rate_lds_bytes(uint32_t span, uint64_t step, uint32_t nt, uint32_t logph) {
  return 4u * (rate_table_dwords(nt, logph) + 2u * rate_plane_dwords(span, step, nt));
}

/* the span length of a launch whose largest step is step: the largest of 1024, 512, 256 whose table and window fit SDRFM_RATE_LDS_BYTES.
 * 256 always fits: NT = 64, 256 phases and step 2^34 take 38296 bytes */
SDRFM_RATE_FN uint32_t rate_span_len(uint64_t step, uint32_t nt, uint32_t logph) {
  uint32_t span = SDRFM_RATE_SPAN_MAX;
  while (span > SDRFM_RATE_NT && rate_lds_bytes(span, step, nt, logph) > SDRFM_RATE_LDS_BYTES) span /= 2u;
  return span;
}

/* span b of a stream's cnt outputs: its first output, how many it takes (0 behind the end) and, for count > 0, its window of input pairs
 * [*w0, *w0 + *w): *w0 >= -(NT - 1) (negative indices are the history), *w0 + *w <= n */
SDRFM_RATE_FN void rate_span(uint64_t pos, uint64_t step, uint32_t cnt, uint32_t span, uint32_t b, uint32_t nt, uint32_t* first, uint32_t* count,
                             int64_t* w0, uint32_t* w) {
  const uint64_t f = (uint64_t)span * b;
  *first = f < cnt ? (uint32_t)f : cnt;
  *count = f < cnt ? (cnt - (uint32_t)f < span ? cnt - (uint32_t)f : span) : 0u;
  *w0 = 0;
  *w = 0;
  if (*count) {
    const uint64_t i_first = (pos + (uint64_t)*first * step) >> 32, i_last = (pos + (uint64_t)(*first + *count - 1u) * step) >> 32;
    *w0 = (int64_t)i_first - (int64_t)nt + 1;
    *w = (uint32_t)(i_last - i_first) + nt;
  }
}

SDRFM_RATE_FN int16_t rate_sat16(int64_t v) { return (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v)); }

/* one output sample of one channel from its two row sums */
SDRFM_RATE_FN int16_t rate_mix(int64_t a0, int64_t a1, uint32_t mu) {
  const int64_t acc = a0 * (int64_t)(256u - mu) + a1 * (int64_t)mu;   /* |a| <= 2^32: below 2^41 */
  return rate_sat16((acc + ((int64_t)1 << 22)) >> 23);
}

#if defined(__HIPCC__)

struct RateParams {
  const int16_t* in;
  size_t in_stride;                /* int16 elements per stream, even; rows are 4-byte aligned */
  int16_t* out;
  size_t out_stride;               /* likewise */
  const uint4* table;              /* [(NPH + 1)][nt / 2 + 1] dwords: taps 2m | 2m + 1 << 16; rate_table_dwords of them, 16-byte aligned */
  const uint64_t* step;            /* [n_streams] */
  const uint64_t* pos_in;          /* [n_streams]: the set this call reads */
  uint64_t* pos_out;               /* ... and the one it writes */
  const unsigned* hist_in;         /* [n_streams][nt - 1] pairs, L | R << 16, oldest first */
  unsigned* hist_out;
  uint32_t n, nt, logph, span, plane_dw;
};

typedef short rate_v2s __attribute__((ext_vector_type(2)));

/* c + a.lo b.lo + a.hi b.hi on int16 halves, wrapping: exact whenever the true sum fits an int32, which the half-row bound guarantees */
__device__ __forceinline__ int rate_dot2(unsigned a, unsigned b, int c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(rate_v2s, a), __builtin_bit_cast(rate_v2s, b), c, false);
#else
  return c + (int)(int16_t)(a & 0xFFFFu) * (int)(int16_t)(b & 0xFFFFu) + ((int)a >> 16) * ((int)b >> 16);
#endif
}

/* pair idx of a stream's input as the call sees it: the history below 0, zero outside [-(nt - 1), n) */
__device__ __forceinline__ unsigned rate_fetch(const unsigned* row, const unsigned* hist, int64_t idx, uint32_t n, uint32_t nt) {
  if (idx >= 0) return idx < (int64_t)n ? row[idx] : 0u;
  return idx >= -(int64_t)(nt - 1u) ? hist[(int64_t)(nt - 1u) + idx] : 0u;
}

/* One workgroup of SDRFM_RATE_NT lanes per (span, stream).  lds: the table, then the window's L plane and its R plane, plane_dw dwords each;
 * plane dword q holds pairs a0 + 2q and a0 + 2q + 1 of one channel, a0 = the window's start rounded down to even.  A lane's NT taps start at
 * plane index i - NT + 1 - a0: when that is odd every tap pair is formed from two neighbouring dwords.  Span 0 of a stream also writes the
 * stream's next pos and history into the other set. */
__device__ __forceinline__ void rate_stream_span(unsigned* lds, const RateParams& p) {
  const uint32_t s = blockIdx.y, b = blockIdx.x, t = threadIdx.x;
  const uint32_t nt = p.nt, rowdw = rate_row_dwords(nt), tabdw = rate_table_dwords(nt, p.logph);
  const uint64_t step = p.step[s], pos = p.pos_in[s];
  const unsigned* row = reinterpret_cast<const unsigned*>(p.in + (size_t)s * p.in_stride);
  const unsigned* hist = p.hist_in + (size_t)s * (nt - 1u);
  const uint32_t cnt = rate_count(pos, step, p.n);
  if (b == 0) {                                                  /* the stream's state for the next call */
    if (t < nt - 1u) {
      const uint64_t c = (uint64_t)p.n + t;                      /* index into (history, new pairs) of the last nt - 1 of them */
      p.hist_out[(size_t)s * (nt - 1u) + t] = c < nt - 1u ? hist[c] : row[c - (nt - 1u)];
    }
    if (t == 0) p.pos_out[s] = rate_advance(pos, step, p.n, cnt);
  }
  uint32_t first, count, w;
  int64_t w0;
  rate_span(pos, step, cnt, p.span, b, nt, &first, &count, &w0, &w);
  if (count == 0) return;                                        /* uniform over the workgroup */
  unsigned* const tab = lds;
  unsigned* const pl = lds + tabdw;
  unsigned* const pr = pl + p.plane_dw;
#pragma unroll 2
  for (uint32_t k = t; k < tabdw / 4u; k += SDRFM_RATE_NT) reinterpret_cast<uint4*>(tab)[k] = p.table[k];   /* wide, independent loads: they overlap */
  const int64_t a0 = w0 & ~(int64_t)1;
  uint32_t need = (uint32_t)((w0 + (int64_t)w - a0 + 1) / 2) + 1u;   /* the window's dwords and the one a lane fetches beyond its taps */
  if (need > p.plane_dw) need = p.plane_dw;                      /* (never: rate_plane_dwords bounds it) */
  for (uint32_t q = t; q < need; q += SDRFM_RATE_NT) {
    const unsigned d0 = rate_fetch(row, hist, a0 + 2 * (int64_t)q, p.n, nt), d1 = rate_fetch(row, hist, a0 + 2 * (int64_t)q + 1, p.n, nt);
    pl[q] = (d0 & 0xFFFFu) | (d1 << 16);
    pr[q] = (d0 >> 16) | (d1 & 0xFFFF0000u);
  }
  __syncthreads();
  unsigned* const orow = reinterpret_cast<unsigned*>(p.out + (size_t)s * p.out_stride);
  const uint32_t half = nt / 4u;                                 /* dwords of half a row */
  for (uint32_t r = t; r < count; r += SDRFM_RATE_NT) {
    const uint32_t j = first + r;
    const uint64_t P = pos + (uint64_t)j * step;
    const uint32_t f = (uint32_t)P;
    const uint32_t ph = f >> (32u - p.logph), mu = (f >> (24u - p.logph)) & 255u;
    const uint32_t q0 = (uint32_t)((int64_t)(P >> 32) - (int64_t)nt + 1 - a0);
    const uint32_t sh = (q0 & 1u) * 16u;
    const unsigned* xl = pl + (q0 >> 1);
    const unsigned* xr = pr + (q0 >> 1);
    const unsigned* c0 = tab + ph * rowdw;
    const unsigned* c1 = c0 + rowdw;
    int64_t a[2][2];                                             /* [channel][row] */
    unsigned dl = xl[0], dr = xr[0];
    uint32_t m = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      int l0 = 0, l1 = 0, r0 = 0, r1 = 0;
      const uint32_t end = m + half;
#pragma unroll 4
      for (; m < end; ++m) {
        const unsigned nl = xl[m + 1], nr = xr[m + 1];
        const unsigned vl = (unsigned)((((uint64_t)nl << 32) | dl) >> sh), vr = (unsigned)((((uint64_t)nr << 32) | dr) >> sh);
        const unsigned k0 = c0[m], k1 = c1[m];
        l0 = rate_dot2(vl, k0, l0);
        l1 = rate_dot2(vl, k1, l1);
        r0 = rate_dot2(vr, k0, r0);
        r1 = rate_dot2(vr, k1, r1);
        dl = nl;
        dr = nr;
      }
      if (h == 0) { a[0][0] = l0; a[0][1] = l1; a[1][0] = r0; a[1][1] = r1; }
      else { a[0][0] += l0; a[0][1] += l1; a[1][0] += r0; a[1][1] += r1; }
    }
    const unsigned L = (uint16_t)rate_mix(a[0][0], a[0][1], mu), R = (uint16_t)rate_mix(a[1][0], a[1][1], mu);
    orow[j] = L | (R << 16);
  }
}

#endif /* __HIPCC__ */
#endif
