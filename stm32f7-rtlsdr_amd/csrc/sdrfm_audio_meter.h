/*
 * sdrfm_audio_meter.h — the stereo PCM sink's per-stream audio meter (include/sdrfm.h): the one copy of the run arithmetic
 * that the meter kernel, sdrfm_audio_meter_add and the CPU checks all use, and the kernel's body.
 *
 * A record describes sample pairs in their order.  Its sums add; its three sdrfm_audio_runs (a predicate's count, leading run, trailing run and
 * longest run) form an associative, non-commutative monoid under am_runs_join, whose identity is the zero record of zero pairs.  So any cut of a
 * row into pieces, joined in order, gives the row's record: a wave walks its stretch 64 pairs at a time (one __ballot is 64 pairs' predicate
 * as a scalar mask, am_mask_runs turns a mask into a runs record with bit operations), the four waves' records are joined in wave order, and
 * the call's record is joined onto the stream's.
 *
 * The first part is plain C99 integers, no HIP types: csrc/audio_meter.c and tests/native/audio_meter_check.cpp compile it with a host
 * compiler alone.  The kernel's body follows under __HIPCC__.  Internal to the library; the drop-in boundary is include/sdrfm.h.
 */
#ifndef SDRFM_AUDIO_METER_H
#define SDRFM_AUDIO_METER_H

#include <stdint.h>

#include "../../include/sdrfm.h"

#if defined(__HIPCC__)
#define SDRFM_AM_FN __host__ __device__ __forceinline__
#else
#define SDRFM_AM_FN static inline
#endif

#define SDRFM_AM_NT 256u             /* lanes of a stream's workgroup: four waves, the default sink's geometry */
#define SDRFM_AM_QUIET_MAX 32767u    /* the largest threshold: |x| <= 32767 leaves only -32768 loud */

SDRFM_AM_FN uint32_t am_ctz64(uint64_t v) { return (uint32_t)__builtin_ctzll(v); }   /* v != 0 */
SDRFM_AM_FN uint32_t am_clz64(uint64_t v) { return (uint32_t)__builtin_clzll(v); }   /* v != 0 */

/* the runs of a block of len pairs, 1 <= len <= 64, whose predicate is bit i of mask for pair i; bits at and above len are ignored */
SDRFM_AM_FN sdrfm_audio_runs am_mask_runs(uint64_t mask, uint32_t len) {
  const uint64_t valid = len >= 64u ? ~(uint64_t)0 : (((uint64_t)1 << len) - 1u);   /* no shift by 64 */
  sdrfm_audio_runs r;
  uint64_t m = mask & valid;
  if (m == valid) { r.count = r.lead = r.trail = r.longest = len; return r; }
  if (m == 0) { r.count = r.lead = r.trail = r.longest = 0; return r; }
  r.count = (uint64_t)__builtin_popcountll(m);
  r.lead = am_ctz64(~m);                                         /* m != valid: ~m has a bit below len */
  r.trail = am_clz64(~(m << (64u - len)));                       /* pair len - 1 moved to bit 63; the complement is not 0 for the same reason */
  uint32_t longest = 0;
  while (m) { m &= m << 1; ++longest; }                          /* every pass shortens each run by one */
  r.longest = longest;
  return r;
}

/* a (an pairs) followed by b (bn pairs) */
SDRFM_AM_FN sdrfm_audio_runs am_runs_join(sdrfm_audio_runs a, uint64_t an, sdrfm_audio_runs b, uint64_t bn) {
  sdrfm_audio_runs r;
  const uint64_t across = a.trail + b.lead;
  uint64_t longest = a.longest > b.longest ? a.longest : b.longest;
  if (across > longest) longest = across;
  r.count = a.count + b.count;
  r.lead = a.lead + (a.lead == an ? b.lead : 0u);
  r.trail = b.trail + (b.trail == bn ? a.trail : 0u);
  r.longest = longest;
  return r;
}

/* the ordered join of include/sdrfm.h: *acc then *m, into *acc.  Signed sums in unsigned arithmetic: wrap-around is defined */
SDRFM_AM_FN void am_meter_join(sdrfm_audio_meter* acc, const sdrfm_audio_meter* m) {
  acc->quiet_l = am_runs_join(acc->quiet_l, acc->n, m->quiet_l, m->n);
  acc->quiet_r = am_runs_join(acc->quiet_r, acc->n, m->quiet_r, m->n);
  acc->quiet_both = am_runs_join(acc->quiet_both, acc->n, m->quiet_both, m->n);
  acc->n += m->n;
  acc->sum_l = (int64_t)((uint64_t)acc->sum_l + (uint64_t)m->sum_l);
  acc->sum_r = (int64_t)((uint64_t)acc->sum_r + (uint64_t)m->sum_r);
  acc->sq_l += m->sq_l;
  acc->sq_r += m->sq_r;
  acc->cross = (int64_t)((uint64_t)acc->cross + (uint64_t)m->cross);
  if (m->peak_l > acc->peak_l) acc->peak_l = m->peak_l;
  if (m->peak_r > acc->peak_r) acc->peak_r = m->peak_r;
  acc->clip_l += m->clip_l;
  acc->clip_r += m->clip_r;
  for (int k = 0; k < 3; ++k) acc->reserved[k] += m->reserved[k];
}

/* the stretch of a row of n pairs that wave w of SDRFM_AM_NT / 64 takes: contiguous, in wave order, every boundary but the last a multiple of 64 */
SDRFM_AM_FN void am_wave_stretch(uint32_t n, uint32_t w, uint64_t* begin, uint64_t* end) {
  const uint64_t per = ((((uint64_t)n + 3u) / 4u) + 63u) & ~(uint64_t)63;
  const uint64_t b = per * w, e = b + per;
  *begin = b < n ? b : n;
  *end = e < n ? e : n;
}

#if defined(__HIPCC__)

struct AudioMeterParams {
  const int16_t* pcm;
  size_t pcm_stride;               /* int16 elements per stream, even; rows are 4-byte aligned */
  sdrfm_audio_meter* rec;          /* [n_streams] */
  uint32_t n, quiet_lsb;
};

__device__ __forceinline__ int64_t am_wave_sum(int64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

__device__ __forceinline__ uint32_t am_wave_max(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d);
    v = o > v ? o : v;
  }
  return v;
}

/* One workgroup of SDRFM_AM_NT lanes per stream.  part: one record per wave, in LDS.  Loads are coalesced dwords of (L | R << 16), four blocks
 * of 64 in flight per wave; a lane at or behind its wave's end loads nothing and holds a zero word, which adds nothing to the sums, the peaks
 * or the rail counts — and am_mask_runs ignores its predicate bit. */
__device__ __forceinline__ void audio_meter_stream(sdrfm_audio_meter* part, const AudioMeterParams& p) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned* row = reinterpret_cast<const unsigned*>(p.pcm + (size_t)blockIdx.x * p.pcm_stride);
  const int q = (int)p.quiet_lsb;
  uint64_t begin, end;
  am_wave_stretch(p.n, w, &begin, &end);
  int64_t sum_l = 0, sum_r = 0, cross = 0;
  uint64_t sq_l = 0, sq_r = 0, clip_l = 0, clip_r = 0;
  uint32_t peak_l = 0, peak_r = 0;
  sdrfm_audio_runs run[3] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};   /* wave-uniform: the pairs begin .. base */
  for (uint64_t base = begin; base < end; base += 256u) {
    unsigned word[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint64_t i = base + 64u * u + lane;
      word[u] = i < end ? row[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint64_t b = base + 64u * u;
      if (b >= end) break;
      const uint32_t len = end - b < 64u ? (uint32_t)(end - b) : 64u;
      const int L = (int)(int16_t)(word[u] & 0xFFFFu), R = (int)word[u] >> 16;
      const int al = L < 0 ? -L : L, ar = R < 0 ? -R : R;
      sum_l += L;
      sum_r += R;
      sq_l += (uint32_t)(L * L);
      sq_r += (uint32_t)(R * R);
      cross += L * R;                                            /* |L R| <= 2^30 */
      peak_l = (uint32_t)al > peak_l ? (uint32_t)al : peak_l;
      peak_r = (uint32_t)ar > peak_r ? (uint32_t)ar : peak_r;
      clip_l += (L == -32768 || L == 32767) ? 1u : 0u;
      clip_r += (R == -32768 || R == 32767) ? 1u : 0u;
      const uint64_t ml = __ballot(al <= q), mr = __ballot(ar <= q);
      const uint64_t done = b - begin;
      run[0] = am_runs_join(run[0], done, am_mask_runs(ml, len), len);
      run[1] = am_runs_join(run[1], done, am_mask_runs(mr, len), len);
      run[2] = am_runs_join(run[2], done, am_mask_runs(ml & mr, len), len);
    }
  }
  sum_l = am_wave_sum(sum_l);
  sum_r = am_wave_sum(sum_r);
  cross = am_wave_sum(cross);
  sq_l = (uint64_t)am_wave_sum((int64_t)sq_l);
  sq_r = (uint64_t)am_wave_sum((int64_t)sq_r);
  clip_l = (uint64_t)am_wave_sum((int64_t)clip_l);
  clip_r = (uint64_t)am_wave_sum((int64_t)clip_r);
  peak_l = am_wave_max(peak_l);
  peak_r = am_wave_max(peak_r);
  if (lane == 0) {
    sdrfm_audio_meter m;
    m.n = end - begin;
    m.sum_l = sum_l; m.sum_r = sum_r; m.sq_l = sq_l; m.sq_r = sq_r; m.cross = cross;
    m.peak_l = peak_l; m.peak_r = peak_r; m.clip_l = clip_l; m.clip_r = clip_r;
    m.quiet_l = run[0]; m.quiet_r = run[1]; m.quiet_both = run[2];
    m.reserved[0] = m.reserved[1] = m.reserved[2] = 0;
    part[w] = m;
  }
  __syncthreads();
  if (threadIdx.x == 0) {                                        /* the waves in their order, then the call behind the stream's record */
    sdrfm_audio_meter call = part[0];
    for (uint32_t k = 1; k < SDRFM_AM_NT / 64u; ++k) am_meter_join(&call, &part[k]);
    sdrfm_audio_meter acc = p.rec[blockIdx.x];
    am_meter_join(&acc, &call);
    p.rec[blockIdx.x] = acc;
  }
}

#endif /* __HIPCC__ */
#endif
