/*
 * sdrfm_pcm_mix.h — the PCM mix bus's launch geometry, its per-pair arithmetic and the kernel body (include/sdrfm.h).
 * The geometry and the arithmetic are plain functions a CPU program can include (tests/native/pcm_mix_check.cpp walks them; csrc/pcm_mix.c is
 * built from them); the body is compiled by hipcc only.
 *
 * A call of n pairs on n_bus buses runs n_bus x spans workgroups of PMIX_NT lanes, spans = cdiv(n, PMIX_SPAN).  Workgroup (bus, span) takes the
 * pairs [span PMIX_SPAN, min(n, (span + 1) PMIX_SPAN)) of that bus; lane t takes the pairs first + t + j PMIX_NT, j < PMIX_PER_LANE, that lie
 * below the span's end.  A pair is one dword (L in the low half, R in the high half), rows are 4-byte aligned, and every access of the body is
 * one dword: legal at every address a row may have, and a wave's 64 dwords are contiguous.
 *
 * Arithmetic.  A slot's contribution to a channel is c (w_L L + w_R R) with c <= 2^15 and the weights of pmix_weights, |w_L L + w_R R| <= 2^16:
 * one product is at most 2^31 in magnitude and the sum over eight slots at most 2^34, so the sum is kept in 64 bits (pmix_acc_bound).
 */
#ifndef SDRFM_PCM_MIX_H
#define SDRFM_PCM_MIX_H

#include <stddef.h>
#include <stdint.h>

#include "sdrfm_audio_ctl.h"

#ifdef __HIPCC__
#define PMIX_HD __host__ __device__ inline
#else
#define PMIX_HD static inline
#endif

#define PMIX_NT 256u                 /* lanes of a workgroup */
#define PMIX_PER_LANE 8u             /* pairs of a lane */
#define PMIX_SPAN (PMIX_NT * PMIX_PER_LANE)   /* pairs of a workgroup: SDRFM_PCM_MIX_SPAN */
#define PMIX_N_MAX (1u << 20)        /* pairs per call */
#define PMIX_ROWS_MAX 65536u         /* n_in and n_bus */
#define PMIX_SLOTS_MAX 8u
#define PMIX_ONE 32768u              /* Q15 1.0 */
#define PMIX_NONE 0xFFFFFFFFu        /* SDRFM_PCM_MIX_NONE */
#define PMIX_MODES 5u
#define PMIX_CURVE_LEN 129u

/* the workgroups of a row of n pairs */
PMIX_HD uint32_t pmix_spans(uint32_t n) { return (n + PMIX_SPAN - 1u) / PMIX_SPAN; }

typedef struct PmixSpan { uint32_t first, end; } PmixSpan;          /* the pairs [first, end) of a workgroup */

PMIX_HD PmixSpan pmix_span(uint32_t n, uint32_t span) {
  PmixSpan s;
  s.first = span * PMIX_SPAN;                                       /* (span < 512: no wrap) */
  s.end = n - s.first < PMIX_SPAN ? n : s.first + PMIX_SPAN;
  return s;
}

/* lane t's pair number j of a span that starts at first */
PMIX_HD uint32_t pmix_lane_pair(uint32_t first, uint32_t t, uint32_t j) { return first + t + j * PMIX_NT; }

/* what a mode takes of (L, R): l = w.ll L + w.lr R, r = w.rl L + w.rr R */
typedef struct PmixWeights { int32_t ll, lr, rl, rr; } PmixWeights;

PMIX_HD PmixWeights pmix_weights(uint32_t mode) {
  PmixWeights w;
  w.ll = mode == 0u || mode == 2u ? 2 : mode == 1u ? 1 : 0;         /* STEREO, LEFT: 2 L;  MONO: L + R */
  w.lr = mode == 3u || mode == 4u ? 2 : mode == 1u ? 1 : 0;         /* RIGHT, SWAP: 2 R */
  w.rl = mode == 2u || mode == 4u ? 2 : mode == 1u ? 1 : 0;         /* LEFT, SWAP: 2 L */
  w.rr = mode == 0u || mode == 3u ? 2 : mode == 1u ? 1 : 0;         /* STEREO, RIGHT: 2 R */
  return w;
}

/* a slot that contributes nothing whatever its row holds: c(0) = 0 */
PMIX_HD int pmix_live(uint32_t src, uint32_t g0, uint32_t gt) { return src != PMIX_NONE && (g0 | gt) != 0u; }

/* the curve at gain g in [0, 32768]: linear between the 129 knots, rounded to nearest */
PMIX_HD uint32_t pmix_curve(const uint16_t* t, uint32_t g) {
  if (g >= PMIX_ONE) return t[128];
  const uint32_t j = g >> 8, f = g & 255u, a = t[j], b = t[j + 1u];
  return a + (((b - a) * f + 128u) >> 8);                           /* b >= a: the table does not decrease */
}

PMIX_HD int pmix_curve_ok(const uint16_t* t) {
  if (t[0] != 0u || t[128] != PMIX_ONE) return 0;
  for (uint32_t j = 0; j < 128u; ++j)
    if (t[j + 1u] < t[j]) return 0;
  return 1;
}

/* the largest |acc| of n_slots slots: every c at 2^15 and every |w_L L + w_R R| at 2^16 */
PMIX_HD int64_t pmix_acc_bound(uint32_t n_slots) { return (int64_t)n_slots * 32768 * 65536; }

/* the sum to the value before the clamp, and the clamp */
PMIX_HD int32_t pmix_round(int64_t acc) { return (int32_t)((acc + 32768) >> 16); }
PMIX_HD int32_t pmix_clamp(int32_t v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

#ifdef __HIPCC__

struct PmixSlot { uint32_t src, mode, g0, gt; };                    // sdrfm_pcm_mix_slot

struct PmixParams {
  const int16_t* in;
  size_t in_stride;                  // int16 elements; 0 where n_in == 1
  int16_t* out;
  size_t out_stride;                 // likewise for n_bus == 1
  const PmixSlot* slots;             // [n_bus][n_slots]
  const uint16_t* curve;             // 129 values on the device, or nullptr
  unsigned long long* rec;           // [n_bus][4]: n, clipped_l, clipped_r, peak
  uint32_t n, n_slots, slew, J;
};

// the body of k_pcm_mix: table is the curve's copy in LDS (not read without one), red the workgroup's three joined values
__device__ inline void pcm_mix_block(const PmixParams& p, uint16_t* table, uint32_t* red) {
  const uint32_t tid = threadIdx.x, bus = blockIdx.x, span = blockIdx.y;
  const PmixSpan sp = pmix_span(p.n, span);
  const bool curved = p.curve != nullptr;                            // (uniform over the launch)
  if (curved) {
    if (tid < PMIX_CURVE_LEN) table[tid] = p.curve[tid];
  }
  if (tid < 3u) red[tid] = 0u;
  __syncthreads();

  int64_t al[PMIX_PER_LANE], ar[PMIX_PER_LANE];
#pragma unroll
  for (uint32_t j = 0; j < PMIX_PER_LANE; ++j) { al[j] = 0; ar[j] = 0; }
  const PmixSlot* slots = p.slots + (size_t)bus * p.n_slots;
  for (uint32_t k = 0; k < p.n_slots; ++k) {
    // the slot once per workgroup, in scalar registers: a dead slot is a uniform branch and its row is never addressed
    const uint32_t src = __builtin_amdgcn_readfirstlane(slots[k].src), mode = __builtin_amdgcn_readfirstlane(slots[k].mode);
    const uint32_t g0 = __builtin_amdgcn_readfirstlane(slots[k].g0), gt = __builtin_amdgcn_readfirstlane(slots[k].gt);
    if (!pmix_live(src, g0, gt)) continue;
    const PmixWeights w = pmix_weights(mode);
    const uint32_t* row = reinterpret_cast<const uint32_t*>(p.in + (size_t)src * p.in_stride);
#pragma unroll
    for (uint32_t j = 0; j < PMIX_PER_LANE; ++j) {
      const uint32_t i = pmix_lane_pair(sp.first, tid, j);
      if (i < sp.end) {
        const uint32_t d = row[i];
        const int32_t L = (int16_t)(d & 0xffffu), R = (int16_t)(d >> 16);
        const uint32_t g = audio_ctl_ramp(g0, gt, p.slew, p.J + i + 1u);
        const int32_t c = (int32_t)(curved ? pmix_curve(table, g) : g);
        al[j] += (int64_t)c * (w.ll * L + w.lr * R);
        ar[j] += (int64_t)c * (w.rl * L + w.rr * R);
      }
    }
  }

  uint32_t cl = 0u, cr = 0u, peak = 0u;
  uint32_t* orow = reinterpret_cast<uint32_t*>(p.out + (size_t)bus * p.out_stride);
#pragma unroll
  for (uint32_t j = 0; j < PMIX_PER_LANE; ++j) {
    const uint32_t i = pmix_lane_pair(sp.first, tid, j);
    if (i < sp.end) {
      const int32_t vl = pmix_round(al[j]), vr = pmix_round(ar[j]), yl = pmix_clamp(vl), yr = pmix_clamp(vr);
      orow[i] = ((uint32_t)yl & 0xffffu) | ((uint32_t)yr << 16);
      cl += vl != yl; cr += vr != yr;
      const uint32_t ml = (uint32_t)(vl < 0 ? -vl : vl), mr = (uint32_t)(vr < 0 ? -vr : vr);
      peak = peak > ml ? peak : ml;
      peak = peak > mr ? peak : mr;
    }
  }

  // the lanes' values joined over the wave in registers, over the workgroup in LDS and onto the bus's record by 64-bit integer atomics
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cl += __shfl_down(cl, o, 64);
    cr += __shfl_down(cr, o, 64);
    const uint32_t q = __shfl_down(peak, o, 64);
    peak = peak > q ? peak : q;
  }
  if ((tid & 63u) == 0u) {
    if (cl) atomicAdd(&red[0], cl);
    if (cr) atomicAdd(&red[1], cr);
    atomicMax(&red[2], peak);
  }
  __syncthreads();
  if (tid == 0u) {
    unsigned long long* m = p.rec + 4 * (size_t)bus;
    atomicAdd(&m[0], (unsigned long long)(sp.end - sp.first));
    if (red[0]) atomicAdd(&m[1], (unsigned long long)red[0]);
    if (red[1]) atomicAdd(&m[2], (unsigned long long)red[1]);
    if (red[2]) atomicMax(&m[3], (unsigned long long)red[2]);
  }
}

#endif  /* __HIPCC__ */
#endif  /* SDRFM_PCM_MIX_H */
