/*
 * sdrfm_meter.h — the meter stage behind the pilot filter's q (include/sdrfm.h): what one new d of a call adds to
 * its stream's sdrfm_scan_meter, and how a workgroup's sums reach the record.  One copy, for sdrfm_scan.hip (whose walk ends at q) and
 * for sdrfm_bcast.hip's metered kernels (which take the same y, d and q on their way to the carriers): the records of the two are the
 * same integers because these are the same functions on the same values.
 *
 * Every new d gives five fp32 terms, each rounded once where written and turned into an integer by rintf(term * 2^k); a lane sums its
 * integers in registers over its whole span (MeterAcc), a wave reduces them once and adds them to the record with one 64-bit atomic per
 * field.  Integer sums are associative, so the record depends on nothing but the bytes.
 */
#ifndef SDRFM_METER_H
#define SDRFM_METER_H

#include "sdrfm_pilot_front.h"

namespace {

static_assert(sizeof(sdrfm_scan_meter) == 64, "the kernels address a record as eight 64-bit words");

constexpr float SCAN_Q_RF = 0x1p+8f, SCAN_Q_D = 0x1p+24f, SCAN_Q_G = 0x1p+20f;   // the scalings of the header (powers of two: exact)
constexpr uint32_t METER_MAX_BYTES = 4u << 20;                                   // of a call, per stream: n <= 2^21 (the header's int64 bounds)
constexpr double METER_MAX_CTAP_SUM = 16.0, METER_MAX_PTAP_SUM = 8.0;            // sum(|hr| + |hi|) per stream, sum(|br| + |bi|)

__device__ __forceinline__ long long scan_fix(float term, float scale) { return (long long)__builtin_rintf(term * scale); }

__device__ __forceinline__ unsigned long long scan_wave_sum(unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// a lane's sums over its span
struct MeterAcc {
  long long rf = 0, fq = 0, dv = 0, pq = 0, p2 = 0;
  uint32_t cnt = 0, on = 0;
};

// one new d: its y, the d itself, the q of the pilot window that ends at it
__device__ __forceinline__ void meter_take(MeterAcc& m, f2_t y, float d, f2_t q, float pmin2) {
  const float pw = __builtin_fmaf(q.x, q.x, q.y * q.y);
  m.rf += scan_fix(__builtin_fmaf(y.x, y.x, y.y * y.y), SCAN_Q_RF);
  m.fq += (long long)(int)__builtin_rintf(d * SCAN_Q_D);       // |d| <= pi and d^2 <= pi^2 (one ulp more at the most): both fit 32 bits
  m.dv += (long long)(int)__builtin_rintf((d * d) * SCAN_Q_D);
  m.pq += scan_fix(pw, SCAN_Q_D);
  m.p2 += scan_fix(pw * pw, SCAN_Q_G);
  m.on += pw >= pmin2 ? 1u : 0u;
  m.cnt += 1u;
}

// the lanes' sums -> the stream's record (eight 64-bit words, zeroed before the launch): one wave reduction and one atomic per field and
// wave (a field no lane added to is skipped)
__device__ __forceinline__ void meter_flush(const MeterAcc& m, unsigned long long* rec, int tid) {
  const unsigned long long v[7] = {m.cnt, m.on, (unsigned long long)m.rf, (unsigned long long)m.fq, (unsigned long long)m.dv,
                                   (unsigned long long)m.pq, (unsigned long long)m.p2};
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    const unsigned long long t = scan_wave_sum(v[k]);
    if ((tid & 63) == 0 && t) atomicAdd(rec + k, t);
  }
}

// ---- host side: the bounds that keep every sum of a call inside int64
// sum of |v[k]| over n floats, in double; NaN where a value is not finite
double meter_abs_sum(const float* v, uint32_t n) {
  double sum = 0.0;
  for (uint32_t k = 0; k < n; ++k) {
    if (!std::isfinite(v[k])) return NAN;
    sum += std::fabs((double)v[k]);
  }
  return sum;
}

// every one of ns rows of `row` floats is finite and within `bound`
bool meter_taps_ok(const float* taps, uint32_t ns, uint32_t row, double bound) {
  for (uint32_t s = 0; s < ns; ++s)
    if (!(meter_abs_sum(taps + (size_t)s * row, row) <= bound)) return false;
  return true;
}

}  // namespace

#endif
