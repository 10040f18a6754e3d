/*
 * sdrfm_sink_hicut.h — the device code of the stereo PCM sink's CONDITIONED forms (sdrfm_sink_stereo.hip; include/sdrfm.h): the sink's
 * recursion with a coefficient that differs per stream and moves per sample,
 *
 *   h[i]     = audio_ctl_ramp(h0, ht, slew, audio_ctl_advance(J, i + 1))      (sdrfm_audio_ctl.h: the one copy of the ramp)
 *   alpha[i] = alpha * ((float)h[i] * 2^-15)                                  the inner product exact, the outer one rounded once
 *   y[i]     = fmaf(alpha[i], x[i] - y[i-1], y[i-1])                          L and R share alpha[i], each carries its own y
 *   pcm[i]   = (int16) rint(clamp(y[i] * gain, -32768, 32767))
 *
 * — the host routine sdrfm_pcm_deemph_stereo_hicut_s16 (csrc/pcm_sink.c), operation for operation.  Two forms, beside the plain sink's two
 * (sdrfm_sink_kernels.h, which this header includes for sink_step, sink_pack and the scan's geometry and leaves as it is):
 *   hicut_exact_tiles    sink_exact_tiles<2>'s tile walk; the lane (= the stream) holds its record and evaluates the ramp at every step.
 *   hicut_scan_segments  sink_scan_segments' geometry — 256 lanes per stream, 19-sample chunks, four waves, three phases per segment of 4864 samples —
 *                        over AFFINE MAPS.  The plain scan carries a chunk's state with one constant, (1 - alpha)^19; here a chunk's decay is the
 *                        product of its own nineteen (1 - alpha[q]), so every lane walks that product beside its chunk's contribution and the scan
 *                        combines the pairs (A, s): "after this chunk the state is A times the state before it, plus s".
 * Internal to sdrfm_sink_stereo.hip: no part of the C-ABI.  tools/pcm_hicut_scan_emulate.py restates the scan on the CPU.
 */
#ifndef SDRFM_SINK_HICUT_H
#define SDRFM_SINK_HICUT_H

#include "sdrfm_audio_ctl.h"
#include "sdrfm_sink_kernels.h"

namespace {

// one stream's record, as the kernels read it: where the ramp started and where it goes, Q15 in [SDRFM_HICUT_MIN, 32768]
struct HicutRec {
  uint16_t h0, ht;
};

// what every conditioned launch gets beside the plain launch's arguments
struct HicutParams {
  const HicutRec* rec;   // [n_streams]
  uint32_t slew, J;      // the ramps' units per sample; the samples the sink has taken between the set and this call (saturated)
};

// the coefficient of sample i (0-based) of the call: the definition's first two lines
__device__ __forceinline__ float hicut_alpha(float alpha, HicutRec r, uint32_t slew, uint32_t J, uint32_t i) {
  const uint32_t h = audio_ctl_ramp(r.h0, r.ht, slew, audio_ctl_advance(J, i + 1u));
  return alpha * ((float)h * 0x1p-15f);
}

// ---- the exact chain: sink_exact_tiles<2> with the coefficient taken per sample; r: the lane's (= the stream's) record ----------------------------------
__device__ __forceinline__ void hicut_exact_tiles(unsigned (&tile)[2][64 * 65], const float* const (&in)[2], size_t audio_stride, int16_t* pcm, size_t pcm_stride,
                                                  uint32_t s0, uint32_t rows, uint32_t n, float alpha, float gain, HicutRec r, uint32_t slew, uint32_t J,
                                                  float (&y)[2]) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t t0 = 0; t0 < n; t0 += 64) {
    const uint32_t cols = (n - t0 < 64u) ? n - t0 : 64u;
    if (lane < cols)
      for (uint32_t row = 0; row < rows; ++row)
#pragma unroll
        for (int c = 0; c < 2; ++c) tile[c][row * 65 + lane] = __float_as_uint(in[c][(size_t)(s0 + row) * audio_stride + t0 + lane]);
    __syncthreads();
    if (lane < rows) {
      for (uint32_t i = 0; i < cols; ++i) {
        const float a = hicut_alpha(alpha, r, slew, J, t0 + i);
        unsigned w[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) w[c] = sink_step(a, gain, __uint_as_float(tile[c][lane * 65 + i]), y[c]);
        tile[0][lane * 65 + i] = sink_pack(w);
      }
    }
    __syncthreads();
    if (lane < cols)
      for (uint32_t row = 0; row < rows; ++row)
        reinterpret_cast<unsigned*>(pcm + (size_t)(s0 + row) * pcm_stride)[t0 + lane] = tile[0][row * 65 + lane];
    __syncthreads();
  }
}

// ---- the blocked scan over affine maps: the workgroup (SINK_NT lanes) serves one stream with record r; y0: the states before the call, and behind it.
// Per segment of SINK_NT chunks of SINK_C samples, one lane per chunk:
//   1. lane t walks its chunk from state 0 (lane 0: from the carried state) -> e[t], and beside it the chunk's own decay through the same operations,
//      a = fmaf(alpha[q], -a, a) from a = 1 -> A[t]: what the chunk leaves of a state handed to it (an empty chunk: A = 1, e = 0, the identity);
//   2. the inclusive prefix over the pairs, (A, s) after (Ao, so) = (A Ao, A so + s): six shuffle steps on both words within each wave, the four waves'
//      totals (A_w, s_w) through LDS and combined in order, cw = fmaf(A_w, cw, s_w); a lane's carry-in is fmaf(A_prev, cw, s_prev) with the pair of the
//      lane before it, the first lane of a wave takes cw, the first lane of the segment the carried state;
//   3. lane t walks its chunk AGAIN from that carry-in with exactly the exact form's operations, and packs the PCM.
// The nineteen alpha[q] of a lane are computed once per segment from the record, slew and J and serve both channels and both walks.
// x: the segment's samples per channel, x[0] then (in place) the packed PCM words; sc: the waves' totals — s per channel, then A —, sc[c][0] then the
// segment's last state.
__device__ __forceinline__ void hicut_scan_segments(float (&x)[2][SINK_SEG], float (&sc)[3][4], const float* const (&row)[2], unsigned* out, uint32_t n,
                                                    float alpha, float gain, HicutRec r, uint32_t slew, uint32_t J, float (&y0)[2]) {
  unsigned* const xw = reinterpret_cast<unsigned*>(x[0]);
  const uint32_t t = threadIdx.x;
  for (uint32_t base = 0; base < n; base += SINK_SEG) {
    const uint32_t m = (n - base < SINK_SEG) ? n - base : SINK_SEG;   // samples of this segment
#pragma unroll
    for (uint32_t q = 0; q < SINK_C; ++q) {                     // coalesced, as in the plain scan
      const uint32_t i = t + SINK_NT * q;
      if (i < m) {
#pragma unroll
        for (int c = 0; c < 2; ++c) x[c][i] = row[c][base + i];
      }
    }
    __syncthreads();
    const uint32_t i0 = t * SINK_C < m ? t * SINK_C : m, cnt = (m - i0 < SINK_C) ? m - i0 : SINK_C;
    unsigned* const wq = xw + i0;
    float xr[2][SINK_C], al[SINK_C];
#pragma unroll
    for (uint32_t q = 0; q < SINK_C; ++q) {
      if (q < cnt) {
#pragma unroll
        for (int c = 0; c < 2; ++c) xr[c][q] = (x[c] + i0)[q];
        al[q] = hicut_alpha(alpha, r, slew, J, base + i0 + q);
      } else {
#pragma unroll
        for (int c = 0; c < 2; ++c) xr[c][q] = 0.0f;
        al[q] = 0.0f;
      }
    }
    // 1. the chunk's own contribution to its last sample and the chunk's decay (lane 0 starts from the real state: its chain is the exact one already)
    float y[2], A = 1.0f;
#pragma unroll
    for (int c = 0; c < 2; ++c) y[c] = t == 0 ? y0[c] : 0.0f;
#pragma unroll
    for (uint32_t q = 0; q < SINK_C; ++q)
      if (q < cnt) {
#pragma unroll
        for (int c = 0; c < 2; ++c) y[c] = __builtin_fmaf(al[q], xr[c][q] - y[c], y[c]);
        A = __builtin_fmaf(al[q], -A, A);
      }
    // 2. the prefix over the pairs: within a wave by six shuffle steps on both words, between the four waves through twelve words of LDS
    const uint32_t wl = t & 63u, wv = t >> 6;
    float sv[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) sv[c] = y[c];
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
      const float Ao = __shfl_up(A, d, 64);
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const float so = __shfl_up(sv[c], d, 64);
        const float sn = __builtin_fmaf(A, so, sv[c]);
        sv[c] = wl >= d ? sn : sv[c];
      }
      const float An = A * Ao;
      A = wl >= d ? An : A;
    }
    if (wl == 63u) {
#pragma unroll
      for (int c = 0; c < 2; ++c) sc[c][wv] = sv[c];
      sc[2][wv] = A;
    }
    float prev[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) prev[c] = __shfl_up(sv[c], 1u, 64);
    const float Aprev = __shfl_up(A, 1u, 64);                   // the pair of the lanes of this wave before this one
    __syncthreads();
    // 3. the exact form's chain from the true carry-in
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      float cw = 0.0f;                                          // the state at the end of the previous wave's chunks
      if (wv >= 1u) cw = sc[c][0];
      if (wv >= 2u) cw = __builtin_fmaf(sc[2][1], cw, sc[c][1]);
      if (wv >= 3u) cw = __builtin_fmaf(sc[2][2], cw, sc[c][2]);
      y[c] = wl == 0u ? (wv == 0u ? y0[c] : cw) : __builtin_fmaf(Aprev, cw, prev[c]);
    }
    __syncthreads();                                            // (every carry-in is in a register before sc[c][0] takes the segment's last state below)
#pragma unroll
    for (uint32_t q = 0; q < SINK_C; ++q)
      if (q < cnt) {
        unsigned w[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) w[c] = sink_step(al[q], gain, xr[c][q], y[c]);
        wq[q] = sink_pack(w);
      }
    if (cnt > 0 && i0 + cnt == m) {                             // the lane that holds the segment's last sample: the states behind it
#pragma unroll
      for (int c = 0; c < 2; ++c) sc[c][0] = y[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; ++c) y0[c] = sc[c][0];
#pragma unroll
    for (uint32_t q = 0; q < SINK_C; ++q) {
      const uint32_t i = t + SINK_NT * q;
      if (i < m) out[base + i] = xw[i];
    }
    __syncthreads();
  }
}

}  // namespace

#endif
