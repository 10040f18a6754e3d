/*
 * sdrfm_hist.h — the deviation histogram of a scan stream (include/sdrfm.h): which of SDRFM_SCAN_HIST_BINS bins a new d of
 * a call counts in, and how a workgroup's counts reach the stream's row.
 *
 * The bin of d is floor(dq / 2^18) + 256 of dq = (int32) rintf(d * 2^24) — the integer sdrfm_meter.h's meter_take adds to freq_q, formed
 * here by the same expression.  A workgroup counts in 512 words of its own LDS, one atomic add of 1 per new d, and adds its non-zero bins
 * to the row once, after its walk, by 32-bit global atomics.  Counts are sums of ones: the row depends on nothing but the bytes.
 */
#ifndef SDRFM_HIST_H
#define SDRFM_HIST_H

#include "sdrfm_meter.h"

namespace {

constexpr uint32_t HIST_BINS = SDRFM_SCAN_HIST_BINS, HIST_LDS_BYTES = 4 * HIST_BINS;
constexpr int HIST_SHIFT = 18, HIST_ZERO_BIN = 256;            // a bin is 2^18 steps of 2^-24 rad = 1/64 rad; d = 0 opens bin 256
static_assert(HIST_BINS == 512 && HIST_BINS == 2 * PF_THREADS, "two bins per lane in hist_zero and hist_flush");

// where the bins start in a workgroup's LDS: the next multiple of 16 at or behind the `end` of the scan kernel's arrays
__host__ __device__ constexpr size_t hist_bins_offset(size_t end) { return (end + 15) & ~(size_t)15; }

// |d| <= pi and one ulp more at the most, so dq lies in +-52 707 179 and the bin in [54, 457]; the mask keeps any other bit pattern of d
// (none is reachable from bytes) inside the array as well
__device__ __forceinline__ uint32_t hist_bin(float d) {
  const int dq = (int)__builtin_rintf(d * SCAN_Q_D);
  return (uint32_t)((dq >> HIST_SHIFT) + HIST_ZERO_BIN) & (HIST_BINS - 1);
}

__device__ __forceinline__ void hist_zero(uint32_t* bins, int tid) {
  bins[tid] = 0u;
  bins[tid + (int)PF_THREADS] = 0u;
}

// one new d
__device__ __forceinline__ void hist_take(uint32_t* bins, float d) { atomicAdd(bins + hist_bin(d), 1u); }

// the workgroup's bins -> the stream's row (zeroed before the launch), two bins per lane; an empty bin is skipped
__device__ __forceinline__ void hist_flush(const uint32_t* bins, uint32_t* row, int tid) {
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int b = tid + k * (int)PF_THREADS;
    const uint32_t v = bins[b];
    if (v) atomicAdd(row + b, v);
  }
}

}  // namespace

#endif
