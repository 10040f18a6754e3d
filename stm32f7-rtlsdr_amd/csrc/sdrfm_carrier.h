/*
 * sdrfm_carrier.h — what the kernels behind the pilot filter make of one q = b * d (include/sdrfm.h): the 38 kHz
 * carrier and the difference signal s of the stereo definition, the 57 kHz carrier and the mixed-down z of the RDS definition.  One
 * copy of each expression, for sdrfm_stereo.hip, sdrfm_rds.hip and sdrfm_bcast.hip (which evaluates both on the same q): every
 * product and quotient is rounded once, the only contractions are the fmafs written (the files are built with -ffp-contract=off).
 */
#ifndef SDRFM_CARRIER_H
#define SDRFM_CARRIER_H

#include "sdrfm_pilot_front.h"

namespace {

// q -> (carrier, s) of one discriminator sample; returns whether the pilot is on
__device__ __forceinline__ bool carrier_stereo(float pmin2, float diff_gain, f2_t q, float dd, float& s_out) {
  const float pw = __builtin_fmaf(q.x, q.x, q.y * q.y);
  const bool on = pw >= pmin2;
  const float c = on ? (-2.0f * (q.x * q.y)) / pw : 0.0f;
  s_out = (c * diff_gain) * dd;
  return on;
}

// q -> z of one discriminator sample (the 57 kHz carrier of size |q| times rds_gain times the delayed d); returns whether the pilot is on
__device__ __forceinline__ bool carrier_rds(float pmin2, float rds_gain, f2_t q, float dd, float& zr, float& zi) {
  const float qq = q.y * q.y;
  const float pw = __builtin_fmaf(q.x, q.x, qq);
  const bool on = pw >= pmin2;
  const float u2r = __builtin_fmaf(q.x, q.x, -qq) / pw;
  const float u2i = (2.0f * (q.x * q.y)) / pw;
  float kr = __builtin_fmaf(u2r, q.x, -(u2i * q.y));
  float ki = __builtin_fmaf(u2r, q.y, u2i * q.x);
  kr = on ? kr : 0.0f;
  ki = on ? ki : 0.0f;
  zr = (kr * rds_gain) * dd;
  zi = (ki * rds_gain) * dd;
  return on;
}

}  // namespace

#endif
