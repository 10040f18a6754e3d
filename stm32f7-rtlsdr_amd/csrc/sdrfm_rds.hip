/*
 * sdrfm_rds.hip — the Radio Data System's complex baseband behind the sdrfm_rds_* C-ABI (include/sdrfm.h).
 *
 * K1-K3 (x, y, d) and the pilot filter q = b * d are the stereo kernel's (csrc/sdrfm_stereo.hip): the same fmaf chain order and
 * sdrfm_discriminate from sdrfm_math.h.  Behind q, at the discriminator rate: the 57 kHz carrier k = u2 q, u2 = q^2 / |q|^2 (gated by
 * |q|^2 >= pilot_min^2), the mixed-down z = (k * rds_gain) d[m - Δ], and the decimating low-pass w = g * z, two real chains.
 *
 * One workgroup (256 lanes) walks a contiguous span of one stream's new d's in steps of NDT d's:
 *   stage   the inputs of the step's y's -> LDS as f16 pairs (x = byte - 127.5 is exact in f16)
 *   y       K2 fmaf chains -> LDS
 *   d       K3 -> LDS, behind the H = P - 1 + Tr - 1 d's carried from the previous step
 *   pilot   q, carrier, z of the step's new d's -> LDS behind the Tr - 1 z's carried from the previous step (the span's first step
 *           computes those Tr - 1 too: that is what the halo's d's are for); the pilot count of the new d's
 *   output  wr, wi -> HBM; one lane per chain (the re lanes first, then the im lanes), zr and zi in planes of their own so that the
 *           lanes' windows, Dr apart, spread over the banks
 * The halo is 2.7 times the stereo kernel's at the default shape (354 d's), and the pilot pass is the dearest one: carrying z from step
 * to step keeps it at one evaluation per d, so a step takes NY - 1 new d's whatever Tr is, and the prologue costs K1-K3 only.
 * The span starts with that prologue, so workgroups are independent.  The workgroup that ends the stream's chunk hands the state
 * over: hist_x (T - 1 inputs), y[M - 1], the last H d's.
 *
 * Two instantiations of the same walk: k_rds<0, 0, 0> takes every shape with runtime loops, one output per lane;
 * k_rds<64, 10, 101> keeps the taps in registers and gives each lane 4 consecutive y's (one pass over their inputs) and 4
 * consecutive pilot outputs (one pass over their d's).  Every chain is evaluated in the same order, so both are bit-identical.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/sdrfm.h"
#include "sdrfm_math.h"

namespace {

typedef float f2_t __attribute__((ext_vector_type(2)));
typedef __fp16 h2_t __attribute__((ext_vector_type(2)));

constexpr uint32_t RD_THREADS = 256;
constexpr uint32_t RD_FAST_NY = 4 * RD_THREADS;   // y's per step of the fast kernel (4 per lane)
constexpr uint32_t RD_LDS_BUDGET = 64u << 10;

struct RdsParams {
  const uint8_t* iq;
  size_t iq_stride;
  float* bb;                   // [ns][bb_stride]: (wr, wi) pairs
  size_t bb_stride;
  uint32_t* pilot_count;       // per stream, zeroed before the launch; nullptr: not counted
  const float2* hist_x_in;     // [ns][T-1]
  float2* hist_x_out;
  const float2* yprev_in;      // [ns]
  float2* yprev_out;
  const float* hist_d_in;      // [ns][H]: d[-H .. -1]
  float* hist_d_out;
  const float* h;              // T
  const float* g;              // Tr
  const float2* tp;            // P: tp[j] = (br, bi)[P - 1 - j] (oldest first)
  uint32_t T, D, P, Tr, Dr, H, Dl;
  float pmin2, rds_gain;
  uint32_t N, M, A;
  int32_t e0, f0;
  uint32_t NY, NDT;            // y's / new d's per step (NDT <= NY - 1)
  uint32_t span;               // new d's per workgroup
  uint32_t blocks_per_stream;
  uint32_t region_words;       // LDS words of the x / (d, zr, zi) region
  uint32_t zplane;             // words of one z plane: Tr - 1 + NDT, made odd
  uint32_t vec;                // 16-byte input loads allowed (iq and iq_stride multiples of 16)
};

__device__ __forceinline__ h2_t pack_x(float a, float b) { return __builtin_amdgcn_cvt_pkrtz(a, b); }   // exact: a, b in {k - 127.5, 0}

__device__ __forceinline__ f2_t unpack_x(h2_t v) { return f2_t{(float)v.x, (float)v.y}; }

// x[n] of the call: n in [-(T-1), N) is the definition's (history for n < 0); outside that range the value is never used
__device__ __forceinline__ h2_t x_at(const RdsParams& p, uint32_t s, int n) {
  if (n >= 0) {
    if (n >= (int)p.N) return pack_x(0.f, 0.f);
    const uchar2 v = *reinterpret_cast<const uchar2*>(p.iq + (size_t)s * p.iq_stride + 2 * (size_t)n);
    return pack_x((float)v.x - 127.5f, (float)v.y - 127.5f);
  }
  if (n < -(int)(p.T - 1)) return pack_x(0.f, 0.f);
  const float2 v = p.hist_x_in[(size_t)s * (p.T - 1) + (p.T - 1 + n)];
  return pack_x(v.x, v.y);
}

__device__ __forceinline__ float2 x_at_f(const RdsParams& p, uint32_t s, int n) {
  if (n < 0) return p.hist_x_in[(size_t)s * (p.T - 1) + (p.T - 1 + n)];
  const uchar2 v = *reinterpret_cast<const uchar2*>(p.iq + (size_t)s * p.iq_stride + 2 * (size_t)n);
  return make_float2((float)v.x - 127.5f, (float)v.y - 127.5f);
}

__device__ __forceinline__ f2_t fma2(f2_t a, f2_t b, f2_t c) { return __builtin_elementwise_fma(a, b, c); }

// q -> z of one discriminator sample (the 57 kHz carrier of size |q| times rds_gain times the delayed d); returns whether the pilot is on
__device__ __forceinline__ bool carrier(const RdsParams& p, f2_t q, float dd, float& zr, float& zi) {
  const float qq = q.y * q.y;
  const float pw = __builtin_fmaf(q.x, q.x, qq);
  const bool on = pw >= p.pmin2;
  const float u2r = __builtin_fmaf(q.x, q.x, -qq) / pw;
  const float u2i = (2.0f * (q.x * q.y)) / pw;
  float kr = __builtin_fmaf(u2r, q.x, -(u2i * q.y));
  float ki = __builtin_fmaf(u2r, q.y, u2i * q.x);
  kr = on ? kr : 0.0f;
  ki = on ? ki : 0.0f;
  zr = (kr * p.rds_gain) * dd;
  zi = (ki * p.rds_gain) * dd;
  return on;
}

template <int FT, int FD, int FP>
__global__ void __launch_bounds__(RD_THREADS) k_rds(RdsParams p) {
  constexpr bool FAST = FT > 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t T = FAST ? FT : p.T, D = FAST ? FD : p.D, P = FAST ? FP : p.P;
  const uint32_t Tr = p.Tr, Dr = p.Dr, H = p.H, Dl = p.Dl, NY = p.NY, NDT = p.NDT, ZP = p.zplane;
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  // LDS: region (x as f16 pairs | d's, zr's, zi's) | ys[NY] | hb[H] | tps[P] | gs[Tr] | hs[T] | zb[2 (Tr - 1)]; hb and tps padded so that gs
  // starts on 16 bytes.  gs holds the taps oldest first (gs[k] = g[Tr - 1 - k]): the output chains read them four at a time
  h2_t* xs = reinterpret_cast<h2_t*>(smem);
  float* ds = reinterpret_cast<float*>(smem);                   // [H + NDT]: the carried d's, then the step's new ones
  float* zs = ds + H + NDT;                                     // two planes [ZP >= Tr - 1 + NDT]: zr, zi of the carried and the new d's
  f2_t* ys = reinterpret_cast<f2_t*>(smem + 4 * (size_t)p.region_words);
  float* hb = reinterpret_cast<float*>(ys + NY);
  f2_t* tps = reinterpret_cast<f2_t*>(hb + ((H + 3) & ~3u));
  float* gs = reinterpret_cast<float*>(tps + ((P + 1) & ~1u));
  float* hs = gs + ((Tr + 3) & ~3u);
  float* zb = hs + T;                                           // the last Tr - 1 (zr, zi), plane by plane, for the next step

  const uint32_t s = blockIdx.x / p.blocks_per_stream, blk = blockIdx.x % p.blocks_per_stream;
  for (int k = tid; k < (int)P; k += nthr) { const float2 t = p.tp[k]; tps[k] = f2_t{t.x, t.y}; }
  for (int k = tid; k < (int)Tr; k += nthr) gs[k] = p.g[Tr - 1 - k];
  for (int k = tid; k < (int)T; k += nthr) hs[k] = p.h[k];
  float hv[FAST ? FT : 1];
  if constexpr (FAST) {
#pragma unroll
    for (int k = 0; k < FT; ++k) {
      hv[k] = p.h[k];
      asm volatile("" : "+v"(hv[k]));                           // wave-uniform taps in VGPRs: 64 of them do not fit the SGPR file
    }
  }
  const f2_t yprev = f2_t{p.yprev_in[s].x, p.yprev_in[s].y};
  const uint8_t* row = p.iq + (size_t)s * p.iq_stride;
  uint32_t cnt = 0;

  auto step = [&](int a, int b, bool full, bool first) {
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
        const uint4 w = *reinterpret_cast<const uint4*>(row + 16 * (size_t)gi);
        h2_t* o = xs + (8 * gi - xlo);
        const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
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
      constexpr int R = 4, NW = (R - 1) * FD + FT, NW4 = (NW + 3) / 4;
      const int u0 = R * tid;
      if (u0 < ny) {
        const uint4* w4 = reinterpret_cast<const uint4*>(xs + u0 * FD);   // 16 * FD * tid bytes: aligned
        f2_t acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = f2_t{0.f, 0.f};
#pragma unroll
        for (int j4 = 0; j4 < NW4; ++j4) {
          const uint4 w = w4[j4];
          const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int j = 4 * j4 + q;
            const f2_t x = unpack_x(__builtin_bit_cast(h2_t, ww[q]));
#pragma unroll
            for (int r = 0; r < R; ++r) {
              const int jj = j - r * FD;                        // position in y[u0 + r]'s window, oldest first
              if (jj >= 0 && jj < FT) acc[r] = fma2(f2_t{hv[FT - 1 - jj], hv[FT - 1 - jj]}, x, acc[r]);
            }
          }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) ys[u0 + r] = acc[r];
      }
    } else {
      for (int u = tid; u < ny; u += nthr) {
        const h2_t* w = xs + u * (int)D;
        f2_t acc = f2_t{0.f, 0.f};
        for (uint32_t j = 0; j < T; ++j) { const float c = hs[T - 1 - j]; acc = fma2(f2_t{c, c}, unpack_x(w[j]), acc); }
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
        const f2_t pr = (i == 0) ? yprev : ys[i - 1 - yA];
        d = sdrfm_discriminate(y.x, y.y, pr.x, pr.y);
      }
      ds[H + k] = d;
    }
    for (int k = tid; k < (int)H; k += nthr) ds[k] = hb[k];
    if (tid == 0 && b == (int)p.M && b > 0) { const f2_t y = ys[b - 1 - yA]; p.yprev_out[s] = make_float2(y.x, y.y); }
    __syncthreads();
    for (int k = tid; k < (int)H; k += nthr) hb[k] = ds[n + k];   // the last H d's, for the next step / the hand-over
    if (full) {
      // ---- pilot filter, carrier, z: plane index o stands for m = a - (Tr - 1) + o, its pilot window is ds[o .. o + P).  The span's first
      //      step computes all of [0, C); a later one takes the first Tr - 1 from the step before and computes the new d's only
      const int C = n + (int)Tr - 1, O0 = first ? 0 : (int)Tr - 1;
      if (!first)
        for (int k = tid; k < 2 * ((int)Tr - 1); k += nthr) {
          const int pl = k >= (int)Tr - 1 ? 1 : 0;
          zs[pl * (int)ZP + (k - pl * ((int)Tr - 1))] = zb[k];
        }
      if constexpr (FAST) {
        constexpr int R = 4;
        for (int o0 = O0 + R * tid; o0 < C; o0 += R * nthr) {
          f2_t acc[R];
#pragma unroll
          for (int r = 0; r < R; ++r) acc[r] = f2_t{0.f, 0.f};
          const float* w = ds + o0;
          float win[R];
#pragma unroll
          for (int r = 0; r < R - 1; ++r) win[r + 1] = w[r];
#pragma unroll R
          for (int j = 0; j < FP; ++j) {                        // (unrolled by R: the window's shift becomes a renaming)
#pragma unroll
            for (int r = 0; r < R - 1; ++r) win[r] = win[r + 1];
            win[R - 1] = w[j + R - 1];
            const f2_t t = tps[j];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = fma2(t, f2_t{win[r], win[r]}, acc[r]);
          }
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int o = o0 + r;
            if (o < C) {
              float zr, zi;
              const bool on = carrier(p, acc[r], ds[o + Dl], zr, zi);
              zs[o] = zr;
              zs[ZP + o] = zi;
              cnt += (on && o >= (int)Tr - 1) ? 1u : 0u;
            }
          }
        }
      } else {
        for (int o = O0 + tid; o < C; o += nthr) {
          f2_t q = f2_t{0.f, 0.f};
          for (uint32_t j = 0; j < P; ++j) { const float dv = ds[o + j]; q = fma2(tps[j], f2_t{dv, dv}, q); }
          float zr, zi;
          const bool on = carrier(p, q, ds[o + Dl], zr, zi);
          zs[o] = zr;
          zs[ZP + o] = zi;
          cnt += (on && o >= (int)Tr - 1) ? 1u : 0u;
        }
      }
      __syncthreads();
      // ---- output: the j's whose newest d lies in [a, b); lane i < nj serves wr of output jl + i, lane nj + i its wi
      int jl = a - p.f0 > 0 ? (a - p.f0 + (int)Dr - 1) / (int)Dr : 0;
      int jh = b - p.f0 > 0 ? (b - p.f0 + (int)Dr - 1) / (int)Dr : 0;
      if (jh > (int)p.A) jh = (int)p.A;
      const int nj = jh > jl ? jh - jl : 0;
      const int per_wave = (2 * nj + nthr / 64 - 1) / (nthr / 64), wv = tid >> 6;   // a contiguous share of the chains for every wave
      const int i_end = (wv + 1) * per_wave < 2 * nj ? (wv + 1) * per_wave : 2 * nj;
      for (int i = wv * per_wave + (tid & 63); i < i_end; i += 64) {
        const int pl = i >= nj ? 1 : 0, j = jl + i - pl * nj;
        const float* wz = zs + pl * (int)ZP + (p.f0 + j * (int)Dr - a);   // the window's oldest z
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
        p.bb[(size_t)s * p.bb_stride + 2 * (size_t)j + pl] = acc;
      }
      for (int k = tid; k < 2 * ((int)Tr - 1); k += nthr) {       // the last Tr - 1 z's, for the next step
        const int pl = k >= (int)Tr - 1 ? 1 : 0;
        zb[k] = zs[pl * (int)ZP + n + (k - pl * ((int)Tr - 1))];
      }
    }
    __syncthreads();
  };

  const int lo = (int)(blk * p.span);
  int hi = lo + (int)p.span;
  if (hi > (int)p.M) hi = (int)p.M;
  for (int a = lo - (int)H; a < lo;) { const int b = a + (int)NDT < lo ? a + (int)NDT : lo; step(a, b, false, false); a = b; }
  for (int a = lo; a < hi;) { const int b = a + (int)NDT < hi ? a + (int)NDT : hi; step(a, b, true, a == lo); a = b; }

  if (p.pilot_count) {
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if ((tid & 63) == 0 && cnt) atomicAdd(p.pilot_count + s, cnt);
  }
  // ---- state hand-over by the workgroup that ends the chunk
  if (blk + 1 == p.blocks_per_stream) {
    for (int k = tid; k < (int)H; k += nthr) p.hist_d_out[(size_t)s * H + k] = hb[k];
    if (tid == 0 && p.M == 0) p.yprev_out[s] = p.yprev_in[s];   // (otherwise the step that ends the chunk wrote y[M - 1])
    for (int k = tid; k + 1 < (int)T; k += nthr) p.hist_x_out[(size_t)s * (T - 1) + k] = x_at_f(p, s, (int)p.N - (int)(T - 1) + k);
  }
}

}  // namespace

// =================================================================================================================
//  Host side: handle, argument checks (all before any device work), launch geometry, state ping-pong.
// =================================================================================================================
struct sdrfm_rds {
  sdrfm_rds_config cfg;                     // taps pointers point at the copies below
  float* hc = nullptr;
  float* gc = nullptr;                         // Tr
  float* bc = nullptr;                         // 2P (re, im)
  int device = 0;
  uint32_t max_bytes = 0, max_out = 0, H = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  float* d_h = nullptr;
  float* d_g = nullptr;
  float2* d_tp = nullptr;
  float2* d_hist_x[2] = {nullptr, nullptr};
  float2* d_yprev[2] = {nullptr, nullptr};
  float* d_hist_d[2] = {nullptr, nullptr};
  uint8_t* d_iq = nullptr;                     // host-buffer calls: staging
  size_t d_iq_stride = 0;
  float* d_bb = nullptr;
  size_t d_bb_stride = 0;
  uint32_t* d_pc = nullptr;
  int cur = 0;
  uint32_t phase_x = 0, phase_d = 0;
  bool fast = false;
  uint32_t fast_lds = 0;
  uint32_t slots = 1;                          // workgroups the device runs at a time (compute units x workgroups per unit)
  char kernel_name[96];
};

namespace {

// LDS bytes of a step geometry (see the layout in k_rds)
uint32_t rds_zplane(uint32_t Tr, uint32_t NDT) { return (Tr - 1 + NDT) | 1u; }

size_t rds_lds(uint32_t T, uint32_t D, uint32_t P, uint32_t Tr, uint32_t H, uint32_t NY, uint32_t NDT, uint32_t* region_words) {
  const size_t nx = (size_t)(NY - 1) * D + T + 4, nds = (size_t)H + NDT + 2 * (size_t)rds_zplane(Tr, NDT);
  size_t rw = nx > nds ? nx : nds;
  rw = (rw + 3) & ~(size_t)3;
  if (region_words) *region_words = (uint32_t)rw;
  return 4 * rw + 8 * (size_t)NY + 4 * (size_t)((H + 3) & ~3u) + 8 * (size_t)((P + 1) & ~1u) + 4 * (size_t)((Tr + 3) & ~3u) + 4 * (size_t)T +
         8 * (size_t)(Tr - 1);
}

void rds_free(sdrfm_rds* h) {
  if (!h) return;
  (void)hipFree(h->d_h); (void)hipFree(h->d_g); (void)hipFree(h->d_tp);
  for (int i = 0; i < 2; ++i) { (void)hipFree(h->d_hist_x[i]); (void)hipFree(h->d_yprev[i]); (void)hipFree(h->d_hist_d[i]); }
  (void)hipFree(h->d_iq); (void)hipFree(h->d_bb); (void)hipFree(h->d_pc);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  free(h->hc); free(h->gc); free(h->bc);
  delete h;
}

bool finite_all(const float* v, uint32_t n) {
  for (uint32_t k = 0; k < n; ++k)
    if (!std::isfinite(v[k])) return false;
  return true;
}

}  // namespace

extern "C" {

int sdrfm_rds_create(const sdrfm_rds_config* cfg, sdrfm_rds_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!cfg || cfg->struct_size != sizeof(sdrfm_rds_config)) return SDRFM_EINVAL;
  if (!cfg->n_streams || !cfg->fir_coeffs || !cfg->rds_coeffs || !cfg->pilot_coeffs) return SDRFM_EINVAL;
  if (cfg->flags & ~SDRFM_RDS_CFG_FORCE_GENERIC) return SDRFM_EINVAL;
  if (!cfg->fir_taps || cfg->fir_taps > SDRFM_MAX_TAPS || !cfg->rds_taps || cfg->rds_taps > SDRFM_MAX_TAPS) return SDRFM_EINVAL;
  if (!cfg->fir_decim || cfg->fir_decim > SDRFM_MAX_DECIM || !cfg->rds_decim || cfg->rds_decim > SDRFM_MAX_DECIM) return SDRFM_EINVAL;
  if (!cfg->pilot_taps || cfg->pilot_taps > SDRFM_STEREO_MAX_PILOT_TAPS || !(cfg->pilot_taps & 1u)) return SDRFM_EINVAL;
  if (!std::isfinite(cfg->pilot_min) || !(cfg->pilot_min > 0.0f) || !std::isfinite(cfg->rds_gain)) return SDRFM_EINVAL;
  // pmin2 rounding to 0 (pilot_min below ~2.6e-23) would open the gate for pw = 0: u2 = 0/0 = NaN on silent input
  if (!(cfg->pilot_min * cfg->pilot_min > 0.0f)) return SDRFM_EINVAL;
  if (!finite_all(cfg->fir_coeffs, cfg->fir_taps) || !finite_all(cfg->rds_coeffs, cfg->rds_taps) ||
      !finite_all(cfg->pilot_coeffs, 2 * cfg->pilot_taps))
    return SDRFM_EINVAL;

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SDRFM_NO_DEVICE;
  if (cfg->device < 0 || cfg->device >= ndev) return SDRFM_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess) return SDRFM_NO_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    fprintf(stderr, "[sdrfm] device %d is %s; this library carries gfx950 code only\n", cfg->device, prop.gcnArchName);
    return SDRFM_NO_DEVICE;
  }
  if (hipSetDevice(cfg->device) != hipSuccess) return SDRFM_NO_DEVICE;

  sdrfm_rds* h = new (std::nothrow) sdrfm_rds();
  if (!h) return SDRFM_ENOMEM;
  h->cfg = *cfg;
  h->device = cfg->device;
  const uint32_t T = cfg->fir_taps, D = cfg->fir_decim, P = cfg->pilot_taps, Tr = cfg->rds_taps, Dr = cfg->rds_decim;
  const size_t ns = cfg->n_streams;
  h->H = P - 1 + Tr - 1;
  h->max_bytes = (cfg->max_bytes_per_call ? cfg->max_bytes_per_call : (1u << 20)) & ~1u;
  {
    const uint64_t m = (uint64_t)(h->max_bytes / 2 + D - 1) / D + 1;
    h->max_out = (uint32_t)((m + Dr - 1) / Dr + 1);
  }
  h->hc = (float*)malloc(sizeof(float) * T);
  h->gc = (float*)malloc(sizeof(float) * Tr);
  h->bc = (float*)malloc(sizeof(float) * 2 * P);
  if (!h->hc || !h->gc || !h->bc) { rds_free(h); return SDRFM_ENOMEM; }
  memcpy(h->hc, cfg->fir_coeffs, sizeof(float) * T);
  memcpy(h->gc, cfg->rds_coeffs, sizeof(float) * Tr);
  memcpy(h->bc, cfg->pilot_coeffs, sizeof(float) * 2 * P);
  h->cfg.fir_coeffs = h->hc;
  h->cfg.rds_coeffs = h->gc;
  h->cfg.pilot_coeffs = h->bc;

  float2* tp = (float2*)malloc(sizeof(float2) * P);
  if (!tp) { rds_free(h); return SDRFM_ENOMEM; }
  for (uint32_t j = 0; j < P; ++j) tp[j] = make_float2(h->bc[2 * (P - 1 - j)], h->bc[2 * (P - 1 - j) + 1]);
  const size_t hx = T > 1 ? T - 1 : 1, hd = h->H ? h->H : 1;
  h->d_iq_stride = ((size_t)h->max_bytes + 255) & ~(size_t)255;
  h->d_bb_stride = (2 * (size_t)h->max_out + 63) & ~(size_t)63;
#define CR(expr) do { if ((expr) != hipSuccess) { free(tp); rds_free(h); return SDRFM_ENOMEM; } } while (0)
  CR(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
  h->stream = h->own_stream;
  CR(hipMalloc(&h->d_h, sizeof(float) * T));
  CR(hipMalloc(&h->d_g, sizeof(float) * Tr));
  CR(hipMalloc(&h->d_tp, sizeof(float2) * P));
  for (int i = 0; i < 2; ++i) {
    CR(hipMalloc(&h->d_hist_x[i], sizeof(float2) * ns * hx));
    CR(hipMalloc(&h->d_yprev[i], sizeof(float2) * ns));
    CR(hipMalloc(&h->d_hist_d[i], sizeof(float) * ns * hd));
  }
  CR(hipMalloc(&h->d_iq, h->d_iq_stride * ns));
  CR(hipMalloc(&h->d_bb, sizeof(float) * h->d_bb_stride * ns));
  CR(hipMalloc(&h->d_pc, sizeof(uint32_t) * ns));
  CR(hipMemcpy(h->d_h, h->hc, sizeof(float) * T, hipMemcpyHostToDevice));
  CR(hipMemcpy(h->d_g, h->gc, sizeof(float) * Tr, hipMemcpyHostToDevice));
  CR(hipMemcpy(h->d_tp, tp, sizeof(float2) * P, hipMemcpyHostToDevice));
#undef CR
  free(tp);
  h->fast_lds = (uint32_t)rds_lds(64, 10, 101, Tr, h->H, RD_FAST_NY, RD_FAST_NY - 1, nullptr);
  h->fast = !(cfg->flags & SDRFM_RDS_CFG_FORCE_GENERIC) && T == 64 && D == 10 && P == 101 && h->fast_lds <= RD_LDS_BUDGET;
  if (h->fast) snprintf(h->kernel_name, sizeof h->kernel_name, "rds-fast T64 D10 P101 Tr%u Dr%u", Tr, Dr);
  else snprintf(h->kernel_name, sizeof h->kernel_name, "rds-generic T%u D%u P%u Tr%u Dr%u", T, D, P, Tr, Dr);
  {
    // what one unit holds of this handle's kernel: by its LDS (the step geometry of rds_enqueue) and its registers
    size_t lds = h->fast_lds;
    if (!h->fast) {
      uint32_t ny = 1024;
      while (ny > 2 && rds_lds(T, D, P, Tr, h->H, ny, ny - 1, nullptr) > RD_LDS_BUDGET) ny -= 2;
      lds = rds_lds(T, D, P, Tr, h->H, ny, ny - 1, nullptr);
    }
    int per_cu = 0;
    const hipError_t e = h->fast ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_rds<64, 10, 101>, RD_THREADS, lds)
                                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_rds<0, 0, 0>, RD_THREADS, lds);
    if (e != hipSuccess || per_cu < 1) per_cu = 1;
    h->slots = (uint32_t)per_cu * (uint32_t)(prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1);
  }
  const int rc = sdrfm_rds_reset(h);
  if (rc != SDRFM_OK) { rds_free(h); return rc; }
  *out = h;
  return SDRFM_OK;
}

void sdrfm_rds_destroy(sdrfm_rds_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  rds_free(h);
}

int sdrfm_rds_reset(sdrfm_rds_t* h) {
  if (!h) return SDRFM_EINVAL;
  if (hipSetDevice(h->device) != hipSuccess) return SDRFM_FAIL;
  const size_t ns = h->cfg.n_streams, T = h->cfg.fir_taps;
  const size_t hx = T > 1 ? T - 1 : 1, hd = h->H ? h->H : 1;
  for (int i = 0; i < 2; ++i) {
    if (hipMemsetAsync(h->d_hist_x[i], 0, sizeof(float2) * ns * hx, h->stream) != hipSuccess) return SDRFM_FAIL;
    if (hipMemsetAsync(h->d_yprev[i], 0, sizeof(float2) * ns, h->stream) != hipSuccess) return SDRFM_FAIL;
    if (hipMemsetAsync(h->d_hist_d[i], 0, sizeof(float) * ns * hd, h->stream) != hipSuccess) return SDRFM_FAIL;
  }
  if (hipStreamSynchronize(h->stream) != hipSuccess) return SDRFM_FAIL;
  h->cur = 0;
  h->phase_x = h->phase_d = 0;
  return SDRFM_OK;
}

int sdrfm_rds_count(const sdrfm_rds_t* h, uint32_t nbytes, uint32_t* n_out) {
  if (!h || !n_out) return SDRFM_EINVAL;
  if (nbytes & 1u) return SDRFM_EODD;
  const uint64_t M = (h->phase_x + (uint64_t)(nbytes / 2)) / h->cfg.fir_decim;
  *n_out = (uint32_t)((h->phase_d + M) / h->cfg.rds_decim);
  return SDRFM_OK;
}

// one call on device buffers, enqueued on the handle's stream
static int rds_enqueue(sdrfm_rds* h, const uint8_t* d_iq, size_t iq_stride, uint32_t nbytes, float* d_bb, size_t bb_stride, uint32_t* d_pc,
                       uint32_t* n_out) {
  const uint32_t T = h->cfg.fir_taps, D = h->cfg.fir_decim, P = h->cfg.pilot_taps, Tr = h->cfg.rds_taps, Dr = h->cfg.rds_decim;
  const uint32_t ns = h->cfg.n_streams, N = nbytes / 2;
  const uint32_t M = (h->phase_x + N) / D, A = (h->phase_d + M) / Dr;
  RdsParams p;
  memset(&p, 0, sizeof p);
  p.iq = d_iq; p.iq_stride = iq_stride;
  p.bb = d_bb; p.bb_stride = bb_stride;
  p.pilot_count = d_pc;
  const int c = h->cur;
  p.hist_x_in = h->d_hist_x[c]; p.hist_x_out = h->d_hist_x[c ^ 1];
  p.yprev_in = h->d_yprev[c]; p.yprev_out = h->d_yprev[c ^ 1];
  p.hist_d_in = h->d_hist_d[c]; p.hist_d_out = h->d_hist_d[c ^ 1];
  p.h = h->d_h; p.g = h->d_g; p.tp = h->d_tp;
  p.T = T; p.D = D; p.P = P; p.Tr = Tr; p.Dr = Dr; p.H = h->H; p.Dl = (P - 1) / 2;
  p.pmin2 = h->cfg.pilot_min * h->cfg.pilot_min;
  p.rds_gain = h->cfg.rds_gain;
  p.N = N; p.M = M; p.A = A;
  p.e0 = (int32_t)(D - 1 - h->phase_x);
  p.f0 = (int32_t)(Dr - 1 - h->phase_d);
  p.vec = ((uintptr_t)d_iq % 16 == 0 && (ns == 1 || iq_stride % 16 == 0)) ? 1u : 0u;
  size_t lds;
  if (h->fast) {
    p.NY = RD_FAST_NY;
    p.NDT = RD_FAST_NY - 1;
    lds = rds_lds(64, 10, 101, Tr, h->H, p.NY, p.NDT, &p.region_words);
  } else {
    uint32_t ny = 1024;
    while (ny > 2 && rds_lds(T, D, P, Tr, h->H, ny, ny - 1, nullptr) > RD_LDS_BUDGET) ny -= 2;
    p.NY = ny;
    p.NDT = ny - 1;
    lds = rds_lds(T, D, P, Tr, h->H, p.NY, p.NDT, &p.region_words);
  }
  if (lds > RD_LDS_BUDGET) return SDRFM_FAIL;                    // (no shape within the header's limits gets here: NY = 2 fits them all)
  p.zplane = rds_zplane(Tr, p.NDT);
  // workgroups per stream: the machine takes h->slots workgroups at a time, so the call lasts (rounds of workgroups) x (a workgroup's span plus
  // its prologue, which costs about half as much per d); the split with the shortest such time, the fewest workgroups among equals, no span
  // below one step.  A stream gets at least one workgroup (the one that hands the state over).  The results do not depend on the split.
  p.blocks_per_stream = 1;
  if (M) {
    const uint32_t most = (M + p.NDT - 1) / p.NDT;
    uint64_t best = ~(uint64_t)0;
    for (uint32_t bps = 1; bps <= most && bps <= 64; ++bps) {
      const uint64_t rounds = ((uint64_t)ns * bps + h->slots - 1) / h->slots, span = (M + bps - 1) / bps;
      const uint64_t cost = rounds * (span + h->H / 2 + 64);
      if (cost < best) { best = cost; p.blocks_per_stream = bps; }
    }
  }
  p.span = M ? (M + p.blocks_per_stream - 1) / p.blocks_per_stream : 0;
  if (d_pc && hipMemsetAsync(d_pc, 0, sizeof(uint32_t) * ns, h->stream) != hipSuccess) return SDRFM_FAIL;
  const dim3 grid(ns * p.blocks_per_stream), block(RD_THREADS);
  if (h->fast) k_rds<64, 10, 101><<<grid, block, lds, h->stream>>>(p);
  else k_rds<0, 0, 0><<<grid, block, lds, h->stream>>>(p);
  if (hipGetLastError() != hipSuccess) return SDRFM_FAIL;
  h->cur ^= 1;
  h->phase_x = (h->phase_x + N) % D;
  h->phase_d = (h->phase_d + M) % Dr;
  *n_out = A;
  return SDRFM_OK;
}

int sdrfm_rds_process_batch(sdrfm_rds_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, float* bb, size_t bb_stride,
                            uint32_t* pilot_count, uint32_t* n_out, uint32_t flags) {
  if (!h || !n_out) return SDRFM_EINVAL;
  if (flags & ~SDRFM_F_DEVICE_PTRS) return SDRFM_EINVAL;       // SDRFM_F_OVERLAP: not for this handle
  if (nbytes & 1u) return SDRFM_EODD;
  if (nbytes > h->max_bytes) return SDRFM_ECAPACITY;
  const uint32_t ns = h->cfg.n_streams;
  if (nbytes == 0) {
    *n_out = 0;
    if (pilot_count) {
      if (flags & SDRFM_F_DEVICE_PTRS) {
        if (hipSetDevice(h->device) != hipSuccess || hipMemsetAsync(pilot_count, 0, sizeof(uint32_t) * ns, h->stream) != hipSuccess) return SDRFM_FAIL;
      } else {
        memset(pilot_count, 0, sizeof(uint32_t) * ns);
      }
    }
    return SDRFM_OK;
  }
  if (!iq) return SDRFM_EINVAL;
  if (ns > 1 && iq_stride < nbytes) return SDRFM_ECAPACITY;
  uint32_t A = 0;
  (void)sdrfm_rds_count(h, nbytes, &A);
  if (A && !bb) return SDRFM_EINVAL;
  if (ns > 1 && bb_stride < 2 * (size_t)A) return SDRFM_ECAPACITY;
  if (hipSetDevice(h->device) != hipSuccess) return SDRFM_FAIL;
  if (flags & SDRFM_F_DEVICE_PTRS) return rds_enqueue(h, iq, iq_stride, nbytes, bb, bb_stride, pilot_count, n_out);

  if (hipMemcpy2DAsync(h->d_iq, h->d_iq_stride, iq, ns > 1 ? iq_stride : nbytes, nbytes, ns, hipMemcpyHostToDevice, h->stream) != hipSuccess)
    return SDRFM_FAIL;
  const int rc = rds_enqueue(h, h->d_iq, h->d_iq_stride, nbytes, h->d_bb, h->d_bb_stride, h->d_pc, n_out);
  if (rc != SDRFM_OK) return rc;
  const size_t dst = (ns > 1 ? bb_stride : 2 * (size_t)A) * sizeof(float), src = h->d_bb_stride * sizeof(float);
  if (A && hipMemcpy2DAsync(bb, dst, h->d_bb, src, 2 * (size_t)A * sizeof(float), ns, hipMemcpyDeviceToHost, h->stream) != hipSuccess)
    return SDRFM_FAIL;
  if (pilot_count && hipMemcpyAsync(pilot_count, h->d_pc, sizeof(uint32_t) * ns, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return SDRFM_FAIL;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return SDRFM_FAIL;
  return SDRFM_OK;
}

int sdrfm_rds_set_stream(sdrfm_rds_t* h, void* hip_stream) {
  if (!h) return SDRFM_EINVAL;
  h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
  return SDRFM_OK;
}

int sdrfm_rds_synchronize(sdrfm_rds_t* h) {
  if (!h) return SDRFM_EINVAL;
  if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return SDRFM_FAIL;
  return SDRFM_OK;
}

const char* sdrfm_rds_kernel_name(const sdrfm_rds_t* h) { return h ? h->kernel_name : ""; }

}  // extern "C"
