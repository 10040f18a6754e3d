/*
 * sdrfm_pilot_front.h — what the stereo, the RDS and the broadcast kernels (sdrfm_stereo.hip, sdrfm_rds.hip, sdrfm_bcast.hip)
 * have in common: the walk from the input bytes to the pilot filter's q, on the device; on the host, the state that walk carries from call
 * to call, the decimators behind d, the split of a call over workgroups and the steps of a call on host buffers.
 *
 * K1-K3 (x, y, d) are the bit-exact kernels' own: the same fmaf chain order and sdrfm_discriminate from sdrfm_math.h, so d is the
 * definition's d.  Behind it, at the discriminator rate, the complex pilot filter q = b * d; what is made of q is the including kernel's.
 *
 * One workgroup (256 lanes) walks a contiguous span of one stream's new d's in steps of NDT d's (front_walk):
 *   stage   the inputs of the step's y's -> LDS as f16 pairs (x = byte - 127.5 is exact in f16)      \
 *   y       K2 fmaf chains -> LDS                                                                      > front_d_stage
 *   d       K3 -> LDS, behind the H d's carried from the previous step                                /
 *   pilot   q of the step's outputs [O0, C), each handed to the kernel's own callable                   front_pilot
 * and the kernel's output chains behind that.  The span starts with a prologue that computes only the H d's before it (halo), so
 * workgroups are independent.  The workgroup that ends the stream's chunk hands the state over (front_hand_over): hist_x (T - 1 inputs),
 * y[M - 1], the last H d's.
 *
 * Two forms of every stage, chosen by the kernel's template arguments: <0, 0, 0> takes every shape with runtime loops, one output per
 * lane; <64, 10, 101> keeps the taps in registers and gives each lane 4 consecutive y's (one pass over their inputs) and 4 consecutive
 * pilot outputs (one pass over their d's).  Every chain is evaluated in the same order, so both are bit-identical.
 *
 * A fourth template argument gives the tuned form of the walk (the broadcast kernel's only): the stream's own complex
 * channel taps (hr, hi) and rotation.  K2 is then two of the real chains above over the same staged x — A with hr, B with hi,
 * y = (Ar - Bi, Ai + Br) — and K3 is sdrfm_discriminate_tuned.  The fast form reloads its 64 tap registers between the two passes.
 */
#ifndef SDRFM_PILOT_FRONT_H
#define SDRFM_PILOT_FRONT_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/sdrfm.h"
#include "sdrfm_math.h"

namespace {

typedef float f2_t __attribute__((ext_vector_type(2)));
typedef __fp16 h2_t __attribute__((ext_vector_type(2)));

constexpr uint32_t PF_THREADS = 256;
constexpr uint32_t PF_FAST_NY = 4 * PF_THREADS;   // y's per step of the fast kernels (4 per lane)
constexpr uint32_t PF_LDS_BUDGET = 64u << 10;

// the kernel parameters of the walk; StereoParams, RdsParams and BcastParams derive from it
struct FrontParams {
  const uint8_t* iq;
  size_t iq_stride;
  uint32_t* pilot_count;       // per stream, zeroed before the launch; nullptr: not counted
  const float2* hist_x_in;     // [ns][T-1]
  float2* hist_x_out;
  const float2* yprev_in;      // [ns]
  float2* yprev_out;
  const float* hist_d_in;      // [ns][H]: d[-H .. -1]
  float* hist_d_out;
  const float* h;              // T
  const float2* tp;            // P: tp[j] = (br, bi)[P - 1 - j] (oldest first)
  uint32_t T, D, P, H, Dl;
  float pmin2;
  uint32_t N, M;
  int32_t e0;
  uint32_t NY, NDT;            // y's / new d's per step (NDT <= NY - 1)
  uint32_t span;               // new d's per workgroup
  uint32_t blocks_per_stream;
  uint32_t region_words;       // LDS words of the region x shares with the d's and what the kernel puts behind them
  uint32_t vec;                // 16-byte input loads allowed (iq and iq_stride multiples of 16)
};

// a workgroup's view of the walk: the kernel lays out its LDS and sets the six pointers, front_begin fills in the rest
template <int FT, int FD, int FP, bool TU = false>
struct FrontWg {
  h2_t* xs;                    // region: x as f16 pairs ...
  float* ds;                   // ... or [H + NDT]: the carried d's, then the step's new ones (the kernel's own arrays follow)
  f2_t* ys;                    // [NY]
  float* hb;                   // [H]: the last H d's, for the next step / the hand-over
  f2_t* tps;                   // [P]
  float* hs;                   // [T]; tuned: [2T], hr then hi
  uint32_t T, D, P, s, blk;
  int tid, nthr;
  f2_t yprev;
  const uint8_t* row;
  const float* ctaps;          // tuned: the stream's 2T floats, (hr[k], hi[k]) pairs; set by the kernel
  float rot;                   // tuned: the stream's rotation; set by the kernel
  float hv[(FT > 0 && !TU) ? FT : 1];
};

__device__ __forceinline__ h2_t pack_x(float a, float b) { return __builtin_amdgcn_cvt_pkrtz(a, b); }   // exact: a, b in {k - 127.5, 0}

__device__ __forceinline__ f2_t unpack_x(h2_t v) { return f2_t{(float)v.x, (float)v.y}; }

// x[n] of the call: n in [-(T-1), N) is the definition's (history for n < 0); outside that range the value is never used
__device__ __forceinline__ h2_t x_at(const FrontParams& p, uint32_t s, int n) {
  if (n >= 0) {
    if (n >= (int)p.N) return pack_x(0.f, 0.f);
    const uchar2 v = *reinterpret_cast<const uchar2*>(p.iq + (size_t)s * p.iq_stride + 2 * (size_t)n);
    return pack_x((float)v.x - 127.5f, (float)v.y - 127.5f);
  }
  if (n < -(int)(p.T - 1)) return pack_x(0.f, 0.f);
  const float2 v = p.hist_x_in[(size_t)s * (p.T - 1) + (p.T - 1 + n)];
  return pack_x(v.x, v.y);
}

__device__ __forceinline__ float2 x_at_f(const FrontParams& p, uint32_t s, int n) {
  if (n < 0) return p.hist_x_in[(size_t)s * (p.T - 1) + (p.T - 1 + n)];
  const uchar2 v = *reinterpret_cast<const uchar2*>(p.iq + (size_t)s * p.iq_stride + 2 * (size_t)n);
  return make_float2((float)v.x - 127.5f, (float)v.y - 127.5f);
}

__device__ __forceinline__ f2_t fma2(f2_t a, f2_t b, f2_t c) { return __builtin_elementwise_fma(a, b, c); }

// the workgroup's stream and place in it, the channel and pilot taps -> LDS (fast: the channel taps -> registers too), the carried y
template <int FT, int FD, int FP, bool TU>
__device__ __forceinline__ void front_begin(const FrontParams& p, FrontWg<FT, FD, FP, TU>& w) {
  constexpr bool FAST = FT > 0;
  w.T = FAST ? FT : p.T; w.D = FAST ? FD : p.D; w.P = FAST ? FP : p.P;
  w.tid = (int)threadIdx.x; w.nthr = (int)blockDim.x;
  w.s = blockIdx.x / p.blocks_per_stream; w.blk = blockIdx.x % p.blocks_per_stream;
  for (int k = w.tid; k < (int)w.P; k += w.nthr) { const float2 t = p.tp[k]; w.tps[k] = f2_t{t.x, t.y}; }
  if constexpr (TU) {
    for (int k = w.tid; k < (int)w.T; k += w.nthr) { w.hs[k] = w.ctaps[2 * k]; w.hs[w.T + k] = w.ctaps[2 * k + 1]; }
  } else {
    for (int k = w.tid; k < (int)w.T; k += w.nthr) w.hs[k] = p.h[k];
  }
  if constexpr (FAST && !TU) {
#pragma unroll
    for (int k = 0; k < FT; ++k) {
      w.hv[k] = p.h[k];
      asm volatile("" : "+v"(w.hv[k]));                         // wave-uniform taps in VGPRs: 64 of them do not fit the SGPR file
    }
  }
  w.yprev = f2_t{p.yprev_in[w.s].x, p.yprev_in[w.s].y};
  w.row = p.iq + (size_t)w.s * p.iq_stride;
}

// the fast K2 pass: 4 consecutive y's of one lane from one read of their inputs at w4, each chain oldest first with the taps in hv
template <int FT, int FD>
__device__ __forceinline__ void front_k2_pass(const uint4* w4, const float (&hv)[FT], f2_t (&acc)[4]) {
  constexpr int R = 4, NW = (R - 1) * FD + FT, NW4 = (NW + 3) / 4;
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r] = f2_t{0.f, 0.f};
#pragma unroll
  for (int j4 = 0; j4 < NW4; ++j4) {
    const uint4 v = w4[j4];
    const uint32_t ww[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = 4 * j4 + q;
      const f2_t x = unpack_x(__builtin_bit_cast(h2_t, ww[q]));
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int jj = j - r * FD;                            // position in y[u0 + r]'s window, oldest first
        if (jj >= 0 && jj < FT) acc[r] = fma2(f2_t{hv[FT - 1 - jj], hv[FT - 1 - jj]}, x, acc[r]);
      }
    }
  }
}

// the fast tuned K2's tap registers: one of the two tap sets from LDS (wave-uniform reads), held in VGPRs as front_begin holds the untuned ones
template <int FT>
__device__ __forceinline__ void front_taps_to_regs(const float* hs, float (&hv)[FT]) {
#pragma unroll
  for (int k = 0; k < FT; ++k) hv[k] = hs[k];                 // (hs is aligned to 4 bytes only: the kernel's arrays before it have any length)
#pragma unroll
  for (int k = 0; k < FT; ++k) asm volatile("" : "+v"(hv[k]));
}

// a step's d's: stage x, K2, K3.  Leaves ds = [the H carried d's | d[a .. b)] and hb = the last H of them; stores yprev_out at the chunk's end
template <int FT, int FD, int FP, bool TU>
__device__ __forceinline__ void front_d_stage(const FrontParams& p, const FrontWg<FT, FD, FP, TU>& w, int a, int b) {
  constexpr bool FAST = FT > 0;
  const uint32_t T = w.T, D = w.D, H = p.H, s = w.s;
  const int tid = w.tid, nthr = w.nthr;
  h2_t* xs = w.xs;
  float* ds = w.ds;
  f2_t* ys = w.ys;
  float* hb = w.hb;
  const int n = b - a;
  const int yA = a - 1 > 0 ? a - 1 : 0;                       // y's [yA, b - 1] are computed (y[-1] is the carried one)
  const int ny = b - yA > 0 ? b - yA : 0;
  // ---- stage x[xlo .. xlo + NX) as f16 pairs
  if (ny > 0) {
    const int xlo = p.e0 + yA * (int)D - (int)(T - 1), nx = (ny - 1) * (int)D + (int)T, x1 = xlo + nx;
    int v0 = x1, v1 = x1;                                     // [v0, v1): whole aligned 8-sample groups inside the chunk
    if (p.vec) {
      const int lo0 = ((xlo > 0 ? xlo : 0) + 7) & ~7, hi0 = (x1 < (int)p.N ? x1 : (int)p.N) & ~7;
      if (lo0 < hi0) { v0 = lo0; v1 = hi0; }
    }
    for (int i = tid; i < v0 - xlo; i += nthr) xs[i] = x_at(p, s, xlo + i);
    for (int i = tid; i < x1 - v1; i += nthr) xs[v1 - xlo + i] = x_at(p, s, v1 + i);
    for (int gi = v0 / 8 + tid; gi < v1 / 8; gi += nthr) {
      const uint4 v = *reinterpret_cast<const uint4*>(w.row + 16 * (size_t)gi);
      h2_t* o = xs + (8 * gi - xlo);
      const uint32_t ww[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o[2 * k] = pack_x((float)(ww[k] & 0xffu) - 127.5f, (float)((ww[k] >> 8) & 0xffu) - 127.5f);
        o[2 * k + 1] = pack_x((float)((ww[k] >> 16) & 0xffu) - 127.5f, (float)(ww[k] >> 24) - 127.5f);
      }
    }
  }
  __syncthreads();
  // ---- K2: ys[u] = y[yA + u]
  if constexpr (FAST) {
    constexpr int R = 4;
    const int u0 = R * tid;
    if (u0 < ny) {
      const uint4* w4 = reinterpret_cast<const uint4*>(xs + u0 * FD);   // 16 * FD * tid bytes: aligned
      f2_t acc[R];
      if constexpr (TU) {                                     // the pass with hr, the registers reloaded with hi, the pass again
        float hv[FT];
        f2_t accb[R];
        front_taps_to_regs<FT>(w.hs, hv);
        front_k2_pass<FT, FD>(w4, hv, acc);
        front_taps_to_regs<FT>(w.hs + FT, hv);
        front_k2_pass<FT, FD>(w4, hv, accb);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = f2_t{acc[r].x - accb[r].y, acc[r].y + accb[r].x};
      } else {
        front_k2_pass<FT, FD>(w4, w.hv, acc);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) ys[u0 + r] = acc[r];
    }
  } else if constexpr (TU) {
    for (int u = tid; u < ny; u += nthr) {
      const h2_t* win = xs + u * (int)D;
      f2_t acc = f2_t{0.f, 0.f}, accb = f2_t{0.f, 0.f};
      for (uint32_t j = 0; j < T; ++j) {
        const float cr = w.hs[T - 1 - j], ci = w.hs[2 * T - 1 - j];
        const f2_t x = unpack_x(win[j]);
        acc = fma2(f2_t{cr, cr}, x, acc);
        accb = fma2(f2_t{ci, ci}, x, accb);
      }
      ys[u] = f2_t{acc.x - accb.y, acc.y + accb.x};
    }
  } else {
    for (int u = tid; u < ny; u += nthr) {
      const h2_t* win = xs + u * (int)D;
      f2_t acc = f2_t{0.f, 0.f};
      for (uint32_t j = 0; j < T; ++j) { const float c = w.hs[T - 1 - j]; acc = fma2(f2_t{c, c}, unpack_x(win[j]), acc); }
      ys[u] = acc;
    }
  }
  __syncthreads();
  // ---- K3: ds = [hb | d[a .. b)]
  for (int k = tid; k < n; k += nthr) {
    const int i = a + k;
    float d;
    if (i < 0) {
      d = p.hist_d_in[(size_t)s * H + (H + i)];
    } else {
      const f2_t y = ys[i - yA];
      const f2_t pr = (i == 0) ? w.yprev : ys[i - 1 - yA];
      if constexpr (TU) d = sdrfm_discriminate_tuned(y.x, y.y, pr.x, pr.y, w.rot);
      else d = sdrfm_discriminate(y.x, y.y, pr.x, pr.y);
    }
    ds[H + k] = d;
  }
  for (int k = tid; k < (int)H; k += nthr) ds[k] = hb[k];
  if (tid == 0 && b == (int)p.M && b > 0) { const f2_t y = ys[b - 1 - yA]; p.yprev_out[s] = make_float2(y.x, y.y); }
  __syncthreads();
  for (int k = tid; k < (int)H; k += nthr) hb[k] = ds[n + k];   // the last H d's, for the next step / the hand-over
}

// the pilot filter over a step's ds: use(o, q) for every output o in [O0, C) this lane serves, o's window being ds[o .. o + P)
template <int FT, int FD, int FP, bool TU, typename Use>
__device__ __forceinline__ void front_pilot(const FrontWg<FT, FD, FP, TU>& w, int O0, int C, Use use) {
  const float* ds = w.ds;
  const f2_t* tps = w.tps;
  if constexpr (FT > 0) {
    constexpr int R = 4;
    for (int o0 = O0 + R * w.tid; o0 < C; o0 += R * w.nthr) {
      f2_t acc[R];
#pragma unroll
      for (int r = 0; r < R; ++r) acc[r] = f2_t{0.f, 0.f};
      const float* wd = ds + o0;
      float win[R];
#pragma unroll
      for (int r = 0; r < R - 1; ++r) win[r + 1] = wd[r];
#pragma unroll R
      for (int j = 0; j < FP; ++j) {                        // (unrolled by R: the window's shift becomes a renaming)
#pragma unroll
        for (int r = 0; r < R - 1; ++r) win[r] = win[r + 1];
        win[R - 1] = wd[j + R - 1];
        const f2_t t = tps[j];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fma2(t, f2_t{win[r], win[r]}, acc[r]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (o0 + r < C) use(o0 + r, acc[r]);
    }
  } else {
    for (int o = O0 + w.tid; o < C; o += w.nthr) {
      f2_t q = f2_t{0.f, 0.f};
      for (uint32_t j = 0; j < w.P; ++j) { const float dv = ds[o + j]; q = fma2(tps[j], f2_t{dv, dv}, q); }
      use(o, q);
    }
  }
}

// the workgroup's span: the prologue's steps (the H d's before it), then its own; step(a, b, full) takes d[a .. b), b - a <= NDT
template <int FT, int FD, int FP, bool TU, typename Step>
__device__ __forceinline__ void front_walk(const FrontParams& p, const FrontWg<FT, FD, FP, TU>& w, Step step) {
  const int NDT = (int)p.NDT, lo = (int)(w.blk * p.span);
  int hi = lo + (int)p.span;
  if (hi > (int)p.M) hi = (int)p.M;
  for (int a = lo - (int)p.H; a < lo;) { const int b = a + NDT < lo ? a + NDT : lo; step(a, b, false); a = b; }
  for (int a = lo; a < hi;) { const int b = a + NDT < hi ? a + NDT : hi; step(a, b, true); a = b; }
}

// the lanes' pilot counts -> pilot_count[s]: one wave reduction and one atomic per wave
__device__ __forceinline__ void front_count(const FrontParams& p, uint32_t s, int tid, uint32_t cnt) {
  if (p.pilot_count) {
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((tid & 63) == 0 && cnt) atomicAdd(p.pilot_count + s, cnt);
  }
}

// state hand-over by the workgroup that ends the chunk
template <int FT, int FD, int FP, bool TU>
__device__ __forceinline__ void front_hand_over(const FrontParams& p, const FrontWg<FT, FD, FP, TU>& w) {
  const uint32_t T = w.T, H = p.H, s = w.s;
  if (w.blk + 1 == p.blocks_per_stream) {
    for (int k = w.tid; k < (int)H; k += w.nthr) p.hist_d_out[(size_t)s * H + k] = w.hb[k];
    if (w.tid == 0 && p.M == 0) p.yprev_out[s] = p.yprev_in[s];   // (otherwise the step that ends the chunk wrote y[M - 1])
    for (int k = w.tid; k + 1 < (int)T; k += w.nthr) p.hist_x_out[(size_t)s * (T - 1) + k] = x_at_f(p, s, (int)p.N - (int)(T - 1) + k);
  }
}

// =================================================================================================================
//  Host side: the part of a handle that serves the walk — taps, carried state in ping-pong sets, input staging, stream — and what the
//  three handles do alike around it: a decimator behind d (Decim), the workgroup split, the protocol of a call.
// =================================================================================================================
struct PilotFront {
  float* hc = nullptr;                         // T
  float* bc = nullptr;                         // 2P (re, im)
  int device = 0;
  uint32_t ns = 0, T = 0, D = 0, P = 0, H = 0, max_bytes = 0;
  float pmin2 = 0.0f;
  hipStream_t own_stream = nullptr, stream = nullptr;
  float* d_h = nullptr;
  float2* d_tp = nullptr;
  float2* d_hist_x[2] = {nullptr, nullptr};
  float2* d_yprev[2] = {nullptr, nullptr};
  float* d_hist_d[2] = {nullptr, nullptr};
  uint8_t* d_iq = nullptr;                     // host-buffer calls: staging
  size_t d_iq_stride = 0;
  uint32_t* d_pc = nullptr;                    // host-buffer calls: the pilot counts [ns]
  int cur = 0;
  uint32_t phase_x = 0;
};

bool finite_all(const float* v, uint32_t n) {
  for (uint32_t k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

// the config fields all three handles have
bool front_config_ok(uint32_t ns, uint32_t T, uint32_t D, const float* h, uint32_t P, const float* b, float pilot_min) {
  if (!ns || !h || !b) return false;
  if (!T || T > SDRFM_MAX_TAPS || !D || D > SDRFM_MAX_DECIM) return false;
  if (!P || P > SDRFM_STEREO_MAX_PILOT_TAPS || !(P & 1u)) return false;
  if (!std::isfinite(pilot_min) || !(pilot_min > 0.0f)) return false;
  // pmin2 rounding to 0 (pilot_min below ~2.6e-23) would open the gate for pw = 0: the carrier is 0/0 = NaN on silent input
  if (!(pilot_min * pilot_min > 0.0f)) return false;
  return finite_all(h, T) && finite_all(b, 2 * P);
}

// makes `device` current if it is a gfx950; SDRFM_OK or SDRFM_NO_DEVICE
int front_open_device(int device, hipDeviceProp_t* prop) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SDRFM_NO_DEVICE;
  if (device < 0 || device >= ndev) return SDRFM_NO_DEVICE;
  if (hipGetDeviceProperties(prop, device) != hipSuccess) return SDRFM_NO_DEVICE;
  if (strncmp(prop->gcnArchName, "gfx950", 6) != 0) {
    fprintf(stderr, "[sdrfm] device %d is %s; this library carries gfx950 code only\n", device, prop->gcnArchName);
    return SDRFM_NO_DEVICE;
  }
  if (hipSetDevice(device) != hipSuccess) return SDRFM_NO_DEVICE;
  return SDRFM_OK;
}

void front_free(PilotFront& f) {
  (void)hipFree(f.d_h); (void)hipFree(f.d_tp);
  for (int i = 0; i < 2; ++i) { (void)hipFree(f.d_hist_x[i]); (void)hipFree(f.d_yprev[i]); (void)hipFree(f.d_hist_d[i]); }
  (void)hipFree(f.d_iq); (void)hipFree(f.d_pc);
  if (f.own_stream) (void)hipStreamDestroy(f.own_stream);
  free(f.hc); free(f.bc);
}

// copies the taps, creates the stream, allocates the device side; SDRFM_OK or SDRFM_ENOMEM (the caller frees what there is with front_free)
int front_alloc(PilotFront& f, uint32_t ns, uint32_t T, uint32_t D, const float* h, uint32_t P, const float* b, float pilot_min, uint32_t H,
                uint32_t max_bytes_per_call, int device) {
  f.device = device;
  f.ns = ns; f.T = T; f.D = D; f.P = P; f.H = H;
  f.pmin2 = pilot_min * pilot_min;
  f.max_bytes = (max_bytes_per_call ? max_bytes_per_call : (1u << 20)) & ~1u;
  f.hc = (float*)malloc(sizeof(float) * T);
  f.bc = (float*)malloc(sizeof(float) * 2 * P);
  float2* tp = (float2*)malloc(sizeof(float2) * P);
  if (!f.hc || !f.bc || !tp) { free(tp); return SDRFM_ENOMEM; }
  memcpy(f.hc, h, sizeof(float) * T);
  memcpy(f.bc, b, sizeof(float) * 2 * P);
  for (uint32_t j = 0; j < P; ++j) tp[j] = make_float2(f.bc[2 * (P - 1 - j)], f.bc[2 * (P - 1 - j) + 1]);
  const size_t hx = T > 1 ? T - 1 : 1, hd = H ? H : 1;
  f.d_iq_stride = ((size_t)f.max_bytes + 255) & ~(size_t)255;
  bool ok = hipStreamCreateWithFlags(&f.own_stream, hipStreamNonBlocking) == hipSuccess;
  f.stream = f.own_stream;
  ok = ok && hipMalloc(&f.d_h, sizeof(float) * T) == hipSuccess && hipMalloc(&f.d_tp, sizeof(float2) * P) == hipSuccess;
  for (int i = 0; i < 2; ++i)
    ok = ok && hipMalloc(&f.d_hist_x[i], sizeof(float2) * ns * hx) == hipSuccess && hipMalloc(&f.d_yprev[i], sizeof(float2) * ns) == hipSuccess &&
         hipMalloc(&f.d_hist_d[i], sizeof(float) * ns * hd) == hipSuccess;
  ok = ok && hipMalloc(&f.d_iq, f.d_iq_stride * ns) == hipSuccess && hipMalloc(&f.d_pc, sizeof(uint32_t) * ns) == hipSuccess &&
       hipMemcpy(f.d_h, f.hc, sizeof(float) * T, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(f.d_tp, tp, sizeof(float2) * P, hipMemcpyHostToDevice) == hipSuccess;
  free(tp);
  return ok ? SDRFM_OK : SDRFM_ENOMEM;
}

// zeroes the carried state; SDRFM_OK or SDRFM_FAIL
int front_reset(PilotFront& f) {
  if (hipSetDevice(f.device) != hipSuccess) return SDRFM_FAIL;
  const size_t ns = f.ns, hx = f.T > 1 ? f.T - 1 : 1, hd = f.H ? f.H : 1;
  for (int i = 0; i < 2; ++i) {
    if (hipMemsetAsync(f.d_hist_x[i], 0, sizeof(float2) * ns * hx, f.stream) != hipSuccess) return SDRFM_FAIL;
    if (hipMemsetAsync(f.d_yprev[i], 0, sizeof(float2) * ns, f.stream) != hipSuccess) return SDRFM_FAIL;
    if (hipMemsetAsync(f.d_hist_d[i], 0, sizeof(float) * ns * hd, f.stream) != hipSuccess) return SDRFM_FAIL;
  }
  if (hipStreamSynchronize(f.stream) != hipSuccess) return SDRFM_FAIL;
  f.cur = 0;
  f.phase_x = 0;
  return SDRFM_OK;
}

// waits for the stream in use, then switches: hip_stream, or NULL for the handle's own (as host_stream_use does for the PCM-side handles).  A
// launch on the old stream may still read the taps and write the state that a tune, a reset or a call behind the switch replaces
int front_use_stream(PilotFront& f, void* hip_stream) {
  if (hipSetDevice(f.device) != hipSuccess || hipStreamSynchronize(f.stream) != hipSuccess) return SDRFM_FAIL;
  f.stream = hip_stream ? (hipStream_t)hip_stream : f.own_stream;
  return SDRFM_OK;
}

// a step geometry and its LDS bytes
struct FrontStep {
  uint32_t NY, NDT, region_words;
  size_t lds;
};
typedef size_t (*front_lds_fn)(uint32_t T, uint32_t D, uint32_t P, uint32_t Tg, uint32_t H, uint32_t NY, uint32_t NDT, uint32_t* region_words);

FrontStep front_step(front_lds_fn lds_fn, uint32_t T, uint32_t D, uint32_t P, uint32_t Tg, uint32_t H, uint32_t NY, uint32_t NDT) {
  FrontStep g = {NY, NDT, 0, 0};
  g.lds = lds_fn(T, D, P, Tg, H, NY, NDT, &g.region_words);
  return g;
}

// the generic kernels' step: the largest even NY, NDT = NY - 1, whose LDS fits the budget (NY = 2 if none does)
FrontStep front_step_generic(front_lds_fn lds_fn, uint32_t T, uint32_t D, uint32_t P, uint32_t Tg, uint32_t H) {
  uint32_t ny = 1024;
  while (ny > 2 && lds_fn(T, D, P, Tg, H, ny, ny - 1, nullptr) > PF_LDS_BUDGET) ny -= 2;
  return front_step(lds_fn, T, D, P, Tg, H, ny, ny - 1);
}

// the new d's of a call of nbytes per stream
uint64_t front_new_d(const PilotFront& f, uint32_t nbytes) { return (f.phase_x + (uint64_t)(nbytes / 2)) / f.D; }

// the walk's part of a call's parameters: a call of nbytes per stream at d_iq, with the step geometry g
void front_fill(const PilotFront& f, FrontParams& p, const uint8_t* d_iq, size_t iq_stride, uint32_t nbytes, uint32_t* d_pc, const FrontStep& g) {
  p.iq = d_iq; p.iq_stride = iq_stride;
  p.pilot_count = d_pc;
  const int c = f.cur;
  p.hist_x_in = f.d_hist_x[c]; p.hist_x_out = f.d_hist_x[c ^ 1];
  p.yprev_in = f.d_yprev[c]; p.yprev_out = f.d_yprev[c ^ 1];
  p.hist_d_in = f.d_hist_d[c]; p.hist_d_out = f.d_hist_d[c ^ 1];
  p.h = f.d_h; p.tp = f.d_tp;
  p.T = f.T; p.D = f.D; p.P = f.P; p.H = f.H; p.Dl = (f.P - 1) / 2;
  p.pmin2 = f.pmin2;
  p.N = nbytes / 2; p.M = (uint32_t)front_new_d(f, nbytes);
  p.e0 = (int32_t)(f.D - 1 - f.phase_x);
  p.vec = ((uintptr_t)d_iq % 16 == 0 && (f.ns == 1 || iq_stride % 16 == 0)) ? 1u : 0u;
  p.NY = g.NY; p.NDT = g.NDT; p.region_words = g.region_words;
}

// after a launch: the other state set is current, the input phase moves on
void front_advance(PilotFront& f, uint32_t N) {
  f.cur ^= 1;
  f.phase_x = (f.phase_x + N) % f.D;
}

// ---- one decimator behind d: the audio chains, the RDS chains
struct Decim {
  uint32_t T = 0, D = 0;                       // taps, decimation
  uint32_t phase = 0;                          // d's since its last output's newest one
  uint32_t max_out = 0;                        // the most outputs a call of max_bytes can give
  float* gc = nullptr;                         // T: the host's copy
  float* d_g = nullptr;                        // T: the device's
};

bool decim_config_ok(uint32_t T, uint32_t D, const float* g, float gain) {
  return g && T && T <= SDRFM_MAX_TAPS && D && D <= SDRFM_MAX_DECIM && std::isfinite(gain) && finite_all(g, T);
}

// copies the taps to the host's and the device's side of a handle whose front is allocated; SDRFM_OK or SDRFM_ENOMEM (decim_free frees what there is)
int decim_alloc(Decim& c, const PilotFront& f, uint32_t T, uint32_t D, const float* g) {
  c.T = T; c.D = D;
  const uint64_t m = (uint64_t)(f.max_bytes / 2 + f.D - 1) / f.D + 1;
  c.max_out = (uint32_t)((m + D - 1) / D + 1);
  c.gc = (float*)malloc(sizeof(float) * T);
  if (!c.gc) return SDRFM_ENOMEM;
  memcpy(c.gc, g, sizeof(float) * T);
  const bool ok = hipMalloc(&c.d_g, sizeof(float) * T) == hipSuccess && hipMemcpy(c.d_g, c.gc, sizeof(float) * T, hipMemcpyHostToDevice) == hipSuccess;
  return ok ? SDRFM_OK : SDRFM_ENOMEM;
}

void decim_free(Decim& c) { (void)hipFree(c.d_g); free(c.gc); }

void decim_reset(Decim& c) { c.phase = 0; }

// the outputs of a call of M new d's, the newest d of its output 0 (output j's: f0 + j D), and the phase after it
uint32_t decim_outputs(const Decim& c, uint64_t M) { return (uint32_t)((c.phase + M) / c.D); }
int32_t decim_f0(const Decim& c) { return (int32_t)(c.D - 1 - c.phase); }
void decim_advance(Decim& c, uint32_t M) { c.phase = (c.phase + M) % c.D; }

// ---- the workgroup split of the RDS and the broadcast handles
// workgroups the device runs at a time of the kernel a handle launches: what one unit holds of it, by its LDS and its registers, x the units
template <typename K>
uint32_t front_slots(K kernel, size_t lds, const hipDeviceProp_t& prop) {
  int per_cu = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, PF_THREADS, lds);
  if (e != hipSuccess || per_cu < 1) per_cu = 1;
  return (uint32_t)per_cu * (uint32_t)(prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1);
}

// workgroups per stream: the machine takes `slots` workgroups at a time, so the call lasts (rounds of workgroups) x (a workgroup's span plus
// its prologue, which costs about half as much per d); the split with the shortest such time, the fewest workgroups among equals, no span
// below one step.  A stream gets at least one workgroup (the one that hands the state over).  The results do not depend on the split.
uint32_t front_split(uint32_t M, uint32_t NDT, uint32_t H, uint32_t ns, uint32_t slots) {
  uint32_t blocks_per_stream = 1;
  if (M) {
    const uint32_t most = (M + NDT - 1) / NDT;
    uint64_t best = ~(uint64_t)0;
    for (uint32_t bps = 1; bps <= most && bps <= 64; ++bps) {
      const uint64_t rounds = ((uint64_t)ns * bps + slots - 1) / slots, span = (M + bps - 1) / bps;
      const uint64_t cost = rounds * (span + H / 2 + 64);
      if (cost < best) { best = cost; blocks_per_stream = bps; }
    }
  }
  return blocks_per_stream;
}

// ---- the protocol of a call; each returns SDRFM_OK or SDRFM_FAIL
// a call's pilot counts start at 0: on the stream where pc is device memory (the launch adds to it), at once where it is the caller's host
// array; pc may be nullptr (not counted)
int front_zero_count(const PilotFront& f, uint32_t* pc, bool on_device) {
  if (pc && !on_device) memset(pc, 0, sizeof(uint32_t) * f.ns);
  if (pc && on_device && hipMemsetAsync(pc, 0, sizeof(uint32_t) * f.ns, f.stream) != hipSuccess) return SDRFM_FAIL;
  return SDRFM_OK;
}

// a call of no bytes: no launch, no outputs, the counts are 0
int front_empty_call(const PilotFront& f, uint32_t* pilot_count, uint32_t flags) {
  const bool on_device = (flags & SDRFM_F_DEVICE_PTRS) != 0;
  if (pilot_count && on_device && hipSetDevice(f.device) != hipSuccess) return SDRFM_FAIL;
  return front_zero_count(f, pilot_count, on_device);
}

// a call on host buffers, in stream order: the input -> d_iq, the launch on the handle's own buffers, every output array back, front_finish
int front_stage_in(const PilotFront& f, const uint8_t* iq, size_t iq_stride, uint32_t nbytes) {
  const hipError_t e = hipMemcpy2DAsync(f.d_iq, f.d_iq_stride, iq, f.ns > 1 ? iq_stride : nbytes, nbytes, f.ns, hipMemcpyHostToDevice, f.stream);
  return e == hipSuccess ? SDRFM_OK : SDRFM_FAIL;
}

// `width` floats per stream from the handle's array (rows of src_stride floats) to the caller's (rows of dst_stride, which one stream need not give)
int front_copy_back(const PilotFront& f, float* dst, size_t dst_stride, const float* d_src, size_t src_stride, size_t width) {
  if (!width) return SDRFM_OK;
  const hipError_t e = hipMemcpy2DAsync(dst, (f.ns > 1 ? dst_stride : width) * sizeof(float), d_src, src_stride * sizeof(float), width * sizeof(float), f.ns,
                                        hipMemcpyDeviceToHost, f.stream);
  return e == hipSuccess ? SDRFM_OK : SDRFM_FAIL;
}

int front_finish(const PilotFront& f, uint32_t* pilot_count) {
  if (pilot_count && hipMemcpyAsync(pilot_count, f.d_pc, sizeof(uint32_t) * f.ns, hipMemcpyDeviceToHost, f.stream) != hipSuccess) return SDRFM_FAIL;
  return hipStreamSynchronize(f.stream) == hipSuccess ? SDRFM_OK : SDRFM_FAIL;
}

}  // namespace

#endif
