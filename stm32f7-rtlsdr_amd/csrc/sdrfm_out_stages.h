/*
 * sdrfm_out_stages.h — the output stages behind the carriers of sdrfm_carrier.h, one copy of each: which outputs
 * of a decimator belong to a step, the audio chains of sdrfm_stereo.hip and sdrfm_bcast.hip, the RDS chains and the carry of their z's
 * of sdrfm_rds.hip and sdrfm_bcast.hip.  The broadcast kernel's outputs are bit for bit the other two kernels' because these are the
 * same functions.  Where the arrays lie in LDS, which lanes take which outputs and what else is carried is the calling kernel's.
 * audio_outputs<true> is the broadcast kernel's blended form: the same chains, and L and R formed under the stream's
 * ramped blend and gain (sdrfm_audio_ctl.h); audio_outputs<> is the code it was.
 */
#ifndef SDRFM_OUT_STAGES_H
#define SDRFM_OUT_STAGES_H

#include "sdrfm_audio_ctl.h"
#include "sdrfm_pilot_front.h"

namespace {

__device__ __forceinline__ int cdiv(int a, int b) { return (a + b - 1) / b; }

// the outputs [x, y) of a decimator by D whose newest d lies in [a, b), of the call's A; output j's newest d is f0 + j D
__device__ __forceinline__ int2 step_outputs(int a, int b, int f0, int D, int A) {
  const int jl = a - f0 > 0 ? (a - f0 + D - 1) / D : 0;
  int jh = b - f0 > 0 ? (b - f0 + D - 1) / D : 0;
  if (jh > A) jh = A;
  return make_int2(jl, jh);
}

// ---- audio: outputs j0, j0 + stride, ... < jh of the step that starts at d[a]; am on the delayed d, as on s, the taps newest first.
//      ds = [the H carried d's | the step's], ss[k] = s of d[a - (Ta - 1) + k];
//      left, right: the stream's rows

// the blended stage's stream: its ramps' record, the handle's slew and the audio outputs between the set and this call's output 0
struct AudioBlend {
  AudioCtlRec rec;
  uint32_t slew, J;
};

// L and R of one output from its two chains' ends under the ramps' values b and v (Q15): beta = b 2^-15 and mu = v 2^-15 are exact,
// t = beta as, L = mu (am + t), R = mu (am - t), every product and every sum rounded on its own whatever the translation unit is built with
__device__ __forceinline__ void audio_blend(float am, float as, uint32_t b, uint32_t v, float& l, float& r) {
#pragma clang fp contract(off)
  const float beta = (float)b * 0x1p-15f, mu = (float)v * 0x1p-15f;
  const float t = beta * as;
  const float sum = am + t, dif = am - t;
  l = mu * sum;
  r = mu * dif;
}

// BL: the broadcast handle's blended form — the same two chains in the same order, audio_blend behind them
template <bool BL = false>
__device__ __forceinline__ void audio_outputs(const float* ds, const float* ss, const float* gas, uint32_t Ta, uint32_t Da, int f0, int a, uint32_t H,
                                              uint32_t Dl, int j0, int stride, int jh, float* left, float* right, const AudioBlend* bl = nullptr) {
  for (int j = j0; j < jh; j += stride) {
    const int nj = f0 + j * (int)Da - a;                         // step-relative index of the newest d of output j
    const float* wd = ds + (int)H + nj - (int)Dl - (int)(Ta - 1);
    const float* wsv = ss + nj;
    float am = 0.0f, as = 0.0f;
    for (uint32_t k = 0; k < Ta; ++k) {
      const float c = gas[Ta - 1 - k];
      am = __builtin_fmaf(c, wd[k], am);
      as = __builtin_fmaf(c, wsv[k], as);
    }
    if constexpr (BL) {
      const uint32_t n = bl->J + (uint32_t)j + 1u;                // outputs since the set, this one included
      audio_blend(am, as, audio_ctl_ramp(bl->rec.b0, bl->rec.bt, bl->slew, n), audio_ctl_ramp(bl->rec.v0, bl->rec.vt, bl->slew, n), left[j], right[j]);
    } else {
      left[j] = am + as;
      right[j] = am - as;
    }
  }
}

// ---- RDS: zr and zi of the step's d's lie in planes of their own, zs[pl ZP + k] = z of d[a - (Tr - 1) + k], so that the lanes' windows,
//      Dr apart, spread over the banks; gs holds the taps oldest first, on 16 bytes: the chains read them four at a time

// words of one z plane: Tr - 1 + NDT, made odd
__host__ __device__ __forceinline__ uint32_t rds_zplane(uint32_t Tr, uint32_t NDT) { return (Tr - 1 + NDT) | 1u; }

__device__ __forceinline__ void rds_taps_to_lds(float* gs, const float* g, uint32_t Tr, int tid, int nthr) {
  for (int k = tid; k < (int)Tr; k += nthr) gs[k] = g[Tr - 1 - k];
}

// the Tr - 1 z's before the step, kept in zb (plane by plane) by the step before -> the planes
__device__ __forceinline__ void rds_tail_restore(float* zs, const float* zb, uint32_t Tr, uint32_t ZP, int tid, int nthr) {
  for (int k = tid; k < 2 * ((int)Tr - 1); k += nthr) {
    const int pl = k >= (int)Tr - 1 ? 1 : 0;
    zs[pl * (int)ZP + (k - pl * ((int)Tr - 1))] = zb[k];
  }
}

// the last Tr - 1 z's of a step of n d's -> zb, for the next step
__device__ __forceinline__ void rds_tail_save(float* zb, const float* zs, int n, uint32_t Tr, uint32_t ZP, int tid, int nthr) {
  for (int k = tid; k < 2 * ((int)Tr - 1); k += nthr) {
    const int pl = k >= (int)Tr - 1 ? 1 : 0;
    zb[k] = zs[pl * (int)ZP + n + (k - pl * ((int)Tr - 1))];
  }
}

// the chains of outputs [jl, jl + nj): chain i < nj is wr of output jl + i, chain nj + i its wi; one lane per chain, a contiguous share
// of the chains for each of the nw waves that take them (this lane: ln of wave wv < nw); bb: the stream's row
__device__ __forceinline__ void rds_chains(const float* zs, const float* gs, uint32_t Tr, uint32_t Dr, uint32_t ZP, int f0, int a, int jl, int nj, int nw,
                                           int wv, int ln, float* bb) {
  const int per_wave = cdiv(2 * nj, nw);
  const int i_end = (wv + 1) * per_wave < 2 * nj ? (wv + 1) * per_wave : 2 * nj;
  for (int i = wv * per_wave + ln; i < i_end; i += 64) {
    const int pl = i >= nj ? 1 : 0, j = jl + i - pl * nj;
    const float* wz = zs + pl * (int)ZP + (f0 + j * (int)Dr - a);   // the window's oldest z
    float acc = 0.0f;
    uint32_t k = 0;
    for (; k + 16 <= Tr; k += 16) {                             // 16 z's and taps in flight, then their fmaf's in order: the chain waits for
      float zv[16];                                             // LDS once per 16 links, not once per link
      float4 gv[4];
#pragma unroll
      for (int u = 0; u < 16; ++u) zv[u] = wz[k + u];
#pragma unroll
      for (int u = 0; u < 4; ++u) gv[u] = *reinterpret_cast<const float4*>(gs + k + 4 * u);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc = __builtin_fmaf(gv[u].x, zv[4 * u], acc);
        acc = __builtin_fmaf(gv[u].y, zv[4 * u + 1], acc);
        acc = __builtin_fmaf(gv[u].z, zv[4 * u + 2], acc);
        acc = __builtin_fmaf(gv[u].w, zv[4 * u + 3], acc);
      }
    }
    for (; k < Tr; ++k) acc = __builtin_fmaf(gs[k], wz[k], acc);
    bb[2 * (size_t)j + pl] = acc;
  }
}

}  // namespace

#endif
