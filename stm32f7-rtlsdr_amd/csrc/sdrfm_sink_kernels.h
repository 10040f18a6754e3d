/*
 * sdrfm_sink_kernels.h — the device code the mono and the stereo PCM sink share (sdrfm_sink.hip, sdrfm_sink_stereo.hip).  Internal to those two files: no part
 * of the C-ABI.  A sink walks NCH independent de-emphasis chains per stream (mono 1, stereo 2: L and R) and packs them into one dword per sample,
 *
 *   y[n]   = fmaf(alpha, x[n] - y[n-1], y[n-1])                    one rounded difference, one fused multiply-add (sdrfm_pcm_deemph_s16, csrc/pcm_sink.c)
 *   pcm[n] = (int16) rint(clamp(y[n] * gain, -32768, 32767))       low half: channel 0, high half: channel NCH - 1 (mono: L = R)
 *
 * in two forms, each written ONCE here as a template over NCH and instantiated by both files' kernels, so that per channel the stereo sink's operations and
 * their order are the mono sink's by construction (the build has -ffp-contract=off and no fast-math: source order fixes the bits):
 *   sink_exact_tiles   the exact chain: one lane per stream, 64 streams per wave, the data transposed through 64 x 65-word LDS tiles;
 *   sink_scan_segments the blocked scan (the default): one workgroup of SINK_NT lanes per stream, three phases per segment (below).
 * What the kernels keep to themselves is how a stream's state is taken and how it is left: the tagged words of sdrfm_sink_chain.h (mono), a plain
 * float[n_streams][2] (stereo).  tools/pcm_stereo_scan_emulate.py restates the scan on the CPU the same way: scan_segment takes the chains as leading axes.
 * (The chain inside a demodulator launch, sdrfm_q.hip, has another geometry — 8-sample chunks, one wave — and is no instance of this.)
 */
#ifndef SDRFM_SINK_KERNELS_H
#define SDRFM_SINK_KERNELS_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sdrfm_host.h"

namespace {

// the blocked scan's geometry: segments of SINK_NT chunks of SINK_C samples, one lane per chunk
constexpr uint32_t SINK_NT = 256, SINK_C = 19, SINK_SEG = SINK_NT * SINK_C;
static_assert(SINK_NT == 256, "four waves: the carries between them are combined by hand");   // 4864 samples per segment (BASELINE's 4800 per call: one segment), 19 KiB of LDS per channel;
                                                                             // lanes SINK_C = 19 words apart (odd): conflict-free LDS accesses

// the blocked scan's carry factor: (1 - alpha)^(samples per chunk), in double, rounded once
inline float sink_carry_factor(float alpha) { return (float)pow(1.0 - (double)alpha, (double)SINK_C); }

// one step of the chain and its PCM word: the operations of sdrfm_pcm_deemph_s16, in its order
__device__ __forceinline__ unsigned sink_step(float alpha, float gain, float x, float& y) {
  y = __builtin_fmaf(alpha, x - y, y);
  float v = y * gain;
  if (v > 32767.0f) v = 32767.0f;
  if (v < -32768.0f) v = -32768.0f;
  return (unsigned)(int)__builtin_rintf(v) & 0xffffu;
}

// the PCM dword of one sample: low half channel 0, high half channel NCH - 1 (one channel: L = R).  The halves are disjoint, so + is |; as a sum the
// one-channel word compiles to a single multiply by 0x10001, as `w | w << 16` written out did
template <int NCH>
__device__ __forceinline__ unsigned sink_pack(const unsigned (&w)[NCH]) { return w[0] + (w[NCH - 1] << 16); }

// ---- the exact chain: the workgroup (one wave) serves streams [s0, s0 + rows), lane = stream; y: the lane's states, in and out ------------------------------
//   HBM --row r: 64 lanes x 4 B, 256 B coalesced--> LDS tile[c][r][t] (row stride 65 words: conflict-free by rows and by columns)
//   lane = stream: 64 dependent steps per channel from LDS, the packed PCM back into tile[0] in place
//   LDS --row r--> HBM 256 B coalesced stores of the interleaved int16 pairs
template <int NCH>
__device__ __forceinline__ void sink_exact_tiles(unsigned (&tile)[NCH][64 * 65], const float* const (&in)[NCH], size_t audio_stride, int16_t* pcm, size_t pcm_stride,
                                                 uint32_t s0, uint32_t rows, uint32_t n, float alpha, float gain, float (&y)[NCH]) {
  const uint32_t lane = threadIdx.x;
  for (uint32_t t0 = 0; t0 < n; t0 += 64) {
    const uint32_t cols = (n - t0 < 64u) ? n - t0 : 64u;
    if (lane < cols)
      for (uint32_t r = 0; r < rows; ++r)
#pragma unroll
        for (int c = 0; c < NCH; ++c) tile[c][r * 65 + lane] = __float_as_uint(in[c][(size_t)(s0 + r) * audio_stride + t0 + lane]);
    __syncthreads();
    if (lane < rows) {
      for (uint32_t i = 0; i < cols; ++i) {
        unsigned w[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) w[c] = sink_step(alpha, gain, __uint_as_float(tile[c][lane * 65 + i]), y[c]);
        tile[0][lane * 65 + i] = sink_pack(w);
      }
    }
    __syncthreads();
    if (lane < cols)
      for (uint32_t r = 0; r < rows; ++r)
        reinterpret_cast<unsigned*>(pcm + (size_t)(s0 + r) * pcm_stride)[t0 + lane] = tile[0][r * 65 + lane];
    __syncthreads();
  }
}

// ---- the blocked scan: the workgroup (SINK_NT lanes) serves one stream, rows row[c] -> PCM row out; y0: the states before the call, and behind it (every lane
// holds them).  The recursion is linear — y[n] = (1 - alpha) y[n-1] + alpha x[n] —, so per segment of SINK_NT chunks of SINK_C samples, one lane per chunk:
//   1. lane t walks its chunk from state 0 (lane 0: from the carried state) -> e[t], the chunk's own contribution to its last sample;
//   2. the carries s[t] = pc s[t-1] + e[t], pc = (1 - alpha)^SINK_C: six shuffle steps within each wave, the four waves' totals combined through LDS;
//   3. lane t walks its chunk AGAIN, now from its true carry-in s[t-1], with exactly the exact form's operations, and packs the PCM.
// x: the segment's samples per channel, x[0] then (in place) the packed PCM words; sc: per channel the waves' totals, then the segment's last state.
template <int NCH>
__device__ __forceinline__ void sink_scan_segments(float (&x)[NCH][SINK_SEG], float (&sc)[NCH][4], const float* const (&row)[NCH], unsigned* out, uint32_t n,
                                                   float alpha, float gain, float pc, float (&y0)[NCH]) {
  unsigned* const xw = reinterpret_cast<unsigned*>(x[0]);
  const uint32_t t = threadIdx.x;
  for (uint32_t base = 0; base < n; base += SINK_SEG) {
    const uint32_t m = (n - base < SINK_SEG) ? n - base : SINK_SEG;   // samples of this segment
#pragma unroll
    for (uint32_t q = 0; q < SINK_C; ++q) {                     // coalesced: NCH SINK_C independent loads per lane in flight
      const uint32_t i = t + SINK_NT * q;
      if (i < m) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) x[c][i] = row[c][base + i];
      }
    }
    __syncthreads();
    // the lane's chunk [i0, i0 + cnt) of every channel in registers: both walks below then run at the chain's own latency (sub -> fma), no LDS round trip inside
    const uint32_t i0 = t * SINK_C < m ? t * SINK_C : m, cnt = (m - i0 < SINK_C) ? m - i0 : SINK_C;
    unsigned* const wq = xw + i0;                               // the chunk's PCM words (its base taken once: every q is then a constant offset from one address)
    float xr[NCH][SINK_C];
#pragma unroll
    for (uint32_t q = 0; q < SINK_C; ++q) {
      if (q < cnt) {                                            // (one branch for all channels: their reads of one q pair up in one LDS instruction)
#pragma unroll
        for (int c = 0; c < NCH; ++c) xr[c][q] = (x[c] + i0)[q];
      } else {
#pragma unroll
        for (int c = 0; c < NCH; ++c) xr[c][q] = 0.0f;
      }
    }
    // 1. the chunk's own contribution to its last sample (lane 0 starts from the real state: its chain is the exact one already)
    float y[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) y[c] = t == 0 ? y0[c] : 0.0f;
#pragma unroll
    for (uint32_t q = 0; q < SINK_C; ++q)
      if (q < cnt) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) y[c] = __builtin_fmaf(alpha, xr[c][q] - y[c], y[c]);
      }
    // 2. s[t] = pc s[t-1] + e[t] (only the last non-empty chunk may be short, and nothing follows it): within a wave by six shuffle steps (the powers squared
    // on the way), between the four waves through four words of LDS — one barrier where a Hillis-Steele scan over 256 lanes in LDS took sixteen
    const uint32_t wl = t & 63u, wv = t >> 6;
    float sv[NCH], pw = pc;
#pragma unroll
    for (int c = 0; c < NCH; ++c) sv[c] = y[c];
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const float o = __shfl_up(sv[c], d, 64);
        const float sn = __builtin_fmaf(pw, o, sv[c]);
        sv[c] = wl >= d ? sn : sv[c];
      }
      pw *= pw;
    }                                                           // (pw = pc^64 now: what a whole wave's chunks leave of a state)
    if (wl == 63u) {
#pragma unroll
      for (int c = 0; c < NCH; ++c) sc[c][wv] = sv[c];
    }
    float pl = 1.0f, pb = pc;                                   // pc^wl: what the chunks of this wave before the lane's leave of the wave's carry-in
#pragma unroll
    for (uint32_t bit = 0; bit < 6u; ++bit) {
      pl = ((wl >> bit) & 1u) ? pl * pb : pl;
      pb *= pb;
    }
    float prev[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) prev[c] = __shfl_up(sv[c], 1u, 64);
    __syncthreads();
    // 3. the exact form's chain from the true carry-in
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      float cw = 0.0f;                                          // the state at the end of the previous wave's chunks
      if (wv >= 1u) cw = sc[c][0];
      if (wv >= 2u) cw = __builtin_fmaf(pw, cw, sc[c][1]);
      if (wv >= 3u) cw = __builtin_fmaf(pw, cw, sc[c][2]);
      y[c] = wl == 0u ? (wv == 0u ? y0[c] : cw) : __builtin_fmaf(pl, cw, prev[c]);
    }
    __syncthreads();                                            // (every carry-in is in a register before sc[c][0] takes the segment's last state below)
#pragma unroll
    for (uint32_t q = 0; q < SINK_C; ++q)
      if (q < cnt) {
        unsigned w[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) w[c] = sink_step(alpha, gain, xr[c][q], y[c]);
        wq[q] = sink_pack(w);
      }
    if (cnt > 0 && i0 + cnt == m) {                             // the lane that holds the segment's last sample: the states behind it
#pragma unroll
      for (int c = 0; c < NCH; ++c) sc[c][0] = y[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NCH; ++c) y0[c] = sc[c][0];
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
