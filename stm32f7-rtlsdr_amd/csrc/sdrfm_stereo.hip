/*
 * sdrfm_stereo.hip — broadcast FM stereo decoding behind the sdrfm_stereo_* C-ABI (include/sdrfm.h).
 *
 * K1-K3 (x, y, d) are the bit-exact kernels' own: the same fmaf chain order and sdrfm_discriminate from sdrfm_math.h, so d is
 * the definition's d.  Behind it, at the discriminator rate: the complex pilot filter q = b * d, the 38 kHz carrier
 * c = -2 qr qi / |q|^2 (gated by |q|^2 >= pilot_min^2), the difference signal s = (c * diff_gain) d[m - Δ], and the two audio
 * chains am (on d delayed by Δ) and as (on s), L = am + as, R = am - as.
 *
 * One workgroup (256 lanes) walks a contiguous span of one stream's new d's in steps of NDT d's:
 *   stage   the inputs of the step's y's -> LDS as f16 pairs (x = byte - 127.5 is exact in f16)
 *   y       K2 fmaf chains -> LDS
 *   d       K3 -> LDS, behind the H = P - 1 + Ta - 1 d's carried from the previous step
 *   pilot   q, carrier, s for the step's audio windows -> LDS; the pilot count of the new d's
 *   audio   am, as -> L, R in HBM
 * The span starts with a prologue that computes only the H d's before it (halo), so workgroups are independent.  The
 * workgroup that ends the stream's chunk hands the state over: hist_x (T - 1 inputs), y[M - 1], the last H d's.
 *
 * Two instantiations of the same walk: k_stereo<0, 0, 0> takes every shape with runtime loops, one output per lane;
 * k_stereo<64, 10, 101> keeps the taps in registers and gives each lane 4 consecutive y's (one pass over their inputs) and 4
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

constexpr uint32_t ST_THREADS = 256;
constexpr uint32_t ST_FAST_NY = 4 * ST_THREADS;   // y's per step of the fast kernel (4 per lane)
constexpr uint32_t ST_LDS_BUDGET = 64u << 10;

struct StereoParams {
  const uint8_t* iq;
  size_t iq_stride;
  float* left;
  float* right;
  size_t audio_stride;
  uint32_t* pilot_count;       // per stream, zeroed before the launch; nullptr: not counted
  const float2* hist_x_in;     // [ns][T-1]
  float2* hist_x_out;
  const float2* yprev_in;      // [ns]
  float2* yprev_out;
  const float* hist_d_in;      // [ns][H]: d[-H .. -1]
  float* hist_d_out;
  const float* h;              // T
  const float* g;              // Ta
  const float2* tp;            // P: tp[j] = (br, bi)[P - 1 - j] (oldest first)
  uint32_t T, D, P, Ta, Da, H, Dl;
  float pmin2, diff_gain;
  uint32_t N, M, A;
  int32_t e0, f0;
  uint32_t NY, NDT;            // y's / new d's per step (NDT <= NY - 1)
  uint32_t span;               // new d's per workgroup
  uint32_t blocks_per_stream;
  uint32_t region_words;       // LDS words of the x / (d, s) region
  uint32_t vec;                // 16-byte input loads allowed (iq and iq_stride multiples of 16)
};

__device__ __forceinline__ h2_t pack_x(float a, float b) { return __builtin_amdgcn_cvt_pkrtz(a, b); }   // exact: a, b in {k - 127.5, 0}

__device__ __forceinline__ f2_t unpack_x(h2_t v) { return f2_t{(float)v.x, (float)v.y}; }

// x[n] of the call: n in [-(T-1), N) is the definition's (history for n < 0); outside that range the value is never used
__device__ __forceinline__ h2_t x_at(const StereoParams& p, uint32_t s, int n) {
  if (n >= 0) {
    if (n >= (int)p.N) return pack_x(0.f, 0.f);
    const uchar2 v = *reinterpret_cast<const uchar2*>(p.iq + (size_t)s * p.iq_stride + 2 * (size_t)n);
    return pack_x((float)v.x - 127.5f, (float)v.y - 127.5f);
  }
  if (n < -(int)(p.T - 1)) return pack_x(0.f, 0.f);
  const float2 v = p.hist_x_in[(size_t)s * (p.T - 1) + (p.T - 1 + n)];
  return pack_x(v.x, v.y);
}

__device__ __forceinline__ float2 x_at_f(const StereoParams& p, uint32_t s, int n) {
  if (n < 0) return p.hist_x_in[(size_t)s * (p.T - 1) + (p.T - 1 + n)];
  const uchar2 v = *reinterpret_cast<const uchar2*>(p.iq + (size_t)s * p.iq_stride + 2 * (size_t)n);
  return make_float2((float)v.x - 127.5f, (float)v.y - 127.5f);
}

__device__ __forceinline__ f2_t fma2(f2_t a, f2_t b, f2_t c) { return __builtin_elementwise_fma(a, b, c); }

// q -> (carrier, s) of one discriminator sample; returns whether the pilot is on
__device__ __forceinline__ bool carrier(const StereoParams& p, f2_t q, float dd, float& s_out) {
  const float pw = __builtin_fmaf(q.x, q.x, q.y * q.y);
  const bool on = pw >= p.pmin2;
  const float c = on ? (-2.0f * (q.x * q.y)) / pw : 0.0f;
  s_out = (c * p.diff_gain) * dd;
  return on;
}

template <int FT, int FD, int FP>
__global__ void __launch_bounds__(ST_THREADS) k_stereo(StereoParams p) {
  constexpr bool FAST = FT > 0;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t T = FAST ? FT : p.T, D = FAST ? FD : p.D, P = FAST ? FP : p.P;
  const uint32_t Ta = p.Ta, Da = p.Da, H = p.H, Dl = p.Dl, NY = p.NY, NDT = p.NDT;
  const int tid = (int)threadIdx.x, nthr = (int)blockDim.x;
  // LDS: region (x as f16 pairs | d's and s's) | ys[NY] | hb[H] | tps[P] | gs[Ta] | hs[T]
  h2_t* xs = reinterpret_cast<h2_t*>(smem);
  float* ds = reinterpret_cast<float*>(smem);                   // [H + NDT]: the carried d's, then the step's new ones
  float* ss = ds + H + NDT;                                     // [Ta - 1 + NDT]: s of the step's audio windows
  f2_t* ys = reinterpret_cast<f2_t*>(smem + 4 * (size_t)p.region_words);
  float* hb = reinterpret_cast<float*>(ys + NY);
  f2_t* tps = reinterpret_cast<f2_t*>(hb + ((H + 1) & ~1u));
  float* gs = reinterpret_cast<float*>(tps + P);
  float* hs = gs + Ta;

  const uint32_t s = blockIdx.x / p.blocks_per_stream, blk = blockIdx.x % p.blocks_per_stream;
  for (int k = tid; k < (int)P; k += nthr) { const float2 t = p.tp[k]; tps[k] = f2_t{t.x, t.y}; }
  for (int k = tid; k < (int)Ta; k += nthr) gs[k] = p.g[k];
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

  auto step = [&](int a, int b, bool full) {
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
      // ---- pilot filter, carrier, s for m in [a - (Ta - 1), b): output o's window is ds[o .. o + P)
      const int C = n + (int)Ta - 1;
      if constexpr (FAST) {
        constexpr int R = 4;
        for (int o0 = R * tid; o0 < C; o0 += R * nthr) {
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
              float sv;
              const bool on = carrier(p, acc[r], ds[o + Dl], sv);
              ss[o] = sv;
              cnt += (on && o >= (int)Ta - 1) ? 1u : 0u;
            }
          }
        }
      } else {
        for (int o = tid; o < C; o += nthr) {
          f2_t q = f2_t{0.f, 0.f};
          for (uint32_t j = 0; j < P; ++j) { const float dv = ds[o + j]; q = fma2(tps[j], f2_t{dv, dv}, q); }
          float sv;
          const bool on = carrier(p, q, ds[o + Dl], sv);
          ss[o] = sv;
          cnt += (on && o >= (int)Ta - 1) ? 1u : 0u;
        }
      }
      __syncthreads();
      // ---- audio: outputs j whose newest d lies in [a, b)
      int jl = a - p.f0 > 0 ? (a - p.f0 + (int)Da - 1) / (int)Da : 0;
      int jh = b - p.f0 > 0 ? (b - p.f0 + (int)Da - 1) / (int)Da : 0;
      if (jh > (int)p.A) jh = (int)p.A;
      for (int j = jl + tid; j < jh; j += nthr) {
        const int nj = p.f0 + j * (int)Da - a;                   // step-relative index of the newest d of output j
        const float* wd = ds + (int)H + nj - (int)Dl - (int)(Ta - 1);
        const float* wsv = ss + nj;
        float am = 0.0f, as = 0.0f;
        for (uint32_t k = 0; k < Ta; ++k) {
          const float c = gs[Ta - 1 - k];
          am = __builtin_fmaf(c, wd[k], am);
          as = __builtin_fmaf(c, wsv[k], as);
        }
        p.left[(size_t)s * p.audio_stride + j] = am + as;
        p.right[(size_t)s * p.audio_stride + j] = am - as;
      }
    }
    __syncthreads();
  };

  const int lo = (int)(blk * p.span);
  int hi = lo + (int)p.span;
  if (hi > (int)p.M) hi = (int)p.M;
  for (int a = lo - (int)H; a < lo;) { const int b = a + (int)NDT < lo ? a + (int)NDT : lo; step(a, b, false); a = b; }
  for (int a = lo; a < hi;) { const int b = a + (int)NDT < hi ? a + (int)NDT : hi; step(a, b, true); a = b; }

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
struct sdrfm_stereo {
  sdrfm_stereo_config cfg;                     // taps pointers point at the copies below
  float* hc = nullptr;
  float* gc = nullptr;
  float* bc = nullptr;                         // 2P (re, im)
  int device = 0;
  uint32_t max_bytes = 0, max_audio = 0, H = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  float* d_h = nullptr;
  float* d_g = nullptr;
  float2* d_tp = nullptr;
  float2* d_hist_x[2] = {nullptr, nullptr};
  float2* d_yprev[2] = {nullptr, nullptr};
  float* d_hist_d[2] = {nullptr, nullptr};
  uint8_t* d_iq = nullptr;                     // host-buffer calls: staging
  size_t d_iq_stride = 0;
  float* d_left = nullptr;
  float* d_right = nullptr;
  size_t d_audio_stride = 0;
  uint32_t* d_pc = nullptr;
  int cur = 0;
  uint32_t phase_x = 0, phase_d = 0;
  bool fast = false;
  uint32_t fast_lds = 0;
  char kernel_name[96];
};

namespace {

// LDS bytes of a step geometry (see the layout in k_stereo)
size_t stereo_lds(uint32_t T, uint32_t D, uint32_t P, uint32_t Ta, uint32_t H, uint32_t NY, uint32_t NDT, uint32_t* region_words) {
  const size_t nx = (size_t)(NY - 1) * D + T + 4, nds = (size_t)H + NDT + Ta - 1 + NDT;
  size_t rw = nx > nds ? nx : nds;
  rw = (rw + 3) & ~(size_t)3;
  if (region_words) *region_words = (uint32_t)rw;
  return 4 * rw + 8 * (size_t)NY + 4 * (size_t)((H + 1) & ~1u) + 8 * (size_t)P + 4 * (size_t)Ta + 4 * (size_t)T;
}

void stereo_free(sdrfm_stereo* h) {
  if (!h) return;
  (void)hipFree(h->d_h); (void)hipFree(h->d_g); (void)hipFree(h->d_tp);
  for (int i = 0; i < 2; ++i) { (void)hipFree(h->d_hist_x[i]); (void)hipFree(h->d_yprev[i]); (void)hipFree(h->d_hist_d[i]); }
  (void)hipFree(h->d_iq); (void)hipFree(h->d_left); (void)hipFree(h->d_right); (void)hipFree(h->d_pc);
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

int sdrfm_stereo_create(const sdrfm_stereo_config* cfg, sdrfm_stereo_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!cfg || cfg->struct_size != sizeof(sdrfm_stereo_config)) return SDRFM_EINVAL;
  if (!cfg->n_streams || !cfg->fir_coeffs || !cfg->audio_coeffs || !cfg->pilot_coeffs) return SDRFM_EINVAL;
  if (cfg->flags & ~SDRFM_STEREO_CFG_FORCE_GENERIC) return SDRFM_EINVAL;
  if (!cfg->fir_taps || cfg->fir_taps > SDRFM_MAX_TAPS || !cfg->audio_taps || cfg->audio_taps > SDRFM_MAX_TAPS) return SDRFM_EINVAL;
  if (!cfg->fir_decim || cfg->fir_decim > SDRFM_MAX_DECIM || !cfg->audio_decim || cfg->audio_decim > SDRFM_MAX_DECIM) return SDRFM_EINVAL;
  if (!cfg->pilot_taps || cfg->pilot_taps > SDRFM_STEREO_MAX_PILOT_TAPS || !(cfg->pilot_taps & 1u)) return SDRFM_EINVAL;
  if (!std::isfinite(cfg->pilot_min) || !(cfg->pilot_min > 0.0f) || !std::isfinite(cfg->diff_gain)) return SDRFM_EINVAL;
  // pmin2 rounding to 0 (pilot_min below ~2.6e-23) would open the gate for pw = 0: c = 0/0 = NaN on silent input
  if (!(cfg->pilot_min * cfg->pilot_min > 0.0f)) return SDRFM_EINVAL;
  if (!finite_all(cfg->fir_coeffs, cfg->fir_taps) || !finite_all(cfg->audio_coeffs, cfg->audio_taps) ||
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

  sdrfm_stereo* h = new (std::nothrow) sdrfm_stereo();
  if (!h) return SDRFM_ENOMEM;
  h->cfg = *cfg;
  h->device = cfg->device;
  const uint32_t T = cfg->fir_taps, D = cfg->fir_decim, P = cfg->pilot_taps, Ta = cfg->audio_taps, Da = cfg->audio_decim;
  const size_t ns = cfg->n_streams;
  h->H = P - 1 + Ta - 1;
  h->max_bytes = (cfg->max_bytes_per_call ? cfg->max_bytes_per_call : (1u << 20)) & ~1u;
  {
    const uint64_t m = (uint64_t)(h->max_bytes / 2 + D - 1) / D + 1;
    h->max_audio = (uint32_t)((m + Da - 1) / Da + 1);
  }
  h->hc = (float*)malloc(sizeof(float) * T);
  h->gc = (float*)malloc(sizeof(float) * Ta);
  h->bc = (float*)malloc(sizeof(float) * 2 * P);
  if (!h->hc || !h->gc || !h->bc) { stereo_free(h); return SDRFM_ENOMEM; }
  memcpy(h->hc, cfg->fir_coeffs, sizeof(float) * T);
  memcpy(h->gc, cfg->audio_coeffs, sizeof(float) * Ta);
  memcpy(h->bc, cfg->pilot_coeffs, sizeof(float) * 2 * P);
  h->cfg.fir_coeffs = h->hc;
  h->cfg.audio_coeffs = h->gc;
  h->cfg.pilot_coeffs = h->bc;

  float2* tp = (float2*)malloc(sizeof(float2) * P);
  if (!tp) { stereo_free(h); return SDRFM_ENOMEM; }
  for (uint32_t j = 0; j < P; ++j) tp[j] = make_float2(h->bc[2 * (P - 1 - j)], h->bc[2 * (P - 1 - j) + 1]);
  const size_t hx = T > 1 ? T - 1 : 1, hd = h->H ? h->H : 1;
  h->d_iq_stride = ((size_t)h->max_bytes + 255) & ~(size_t)255;
  h->d_audio_stride = ((size_t)h->max_audio + 63) & ~(size_t)63;
#define CR(expr) do { if ((expr) != hipSuccess) { free(tp); stereo_free(h); return SDRFM_ENOMEM; } } while (0)
  CR(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
  h->stream = h->own_stream;
  CR(hipMalloc(&h->d_h, sizeof(float) * T));
  CR(hipMalloc(&h->d_g, sizeof(float) * Ta));
  CR(hipMalloc(&h->d_tp, sizeof(float2) * P));
  for (int i = 0; i < 2; ++i) {
    CR(hipMalloc(&h->d_hist_x[i], sizeof(float2) * ns * hx));
    CR(hipMalloc(&h->d_yprev[i], sizeof(float2) * ns));
    CR(hipMalloc(&h->d_hist_d[i], sizeof(float) * ns * hd));
  }
  CR(hipMalloc(&h->d_iq, h->d_iq_stride * ns));
  CR(hipMalloc(&h->d_left, sizeof(float) * h->d_audio_stride * ns));
  CR(hipMalloc(&h->d_right, sizeof(float) * h->d_audio_stride * ns));
  CR(hipMalloc(&h->d_pc, sizeof(uint32_t) * ns));
  CR(hipMemcpy(h->d_h, h->hc, sizeof(float) * T, hipMemcpyHostToDevice));
  CR(hipMemcpy(h->d_g, h->gc, sizeof(float) * Ta, hipMemcpyHostToDevice));
  CR(hipMemcpy(h->d_tp, tp, sizeof(float2) * P, hipMemcpyHostToDevice));
#undef CR
  free(tp);
  const uint32_t ndt_fast = ST_FAST_NY - (Ta > 1 ? Ta - 1 : 1);
  h->fast_lds = (uint32_t)stereo_lds(64, 10, 101, Ta, h->H, ST_FAST_NY, ndt_fast, nullptr);
  h->fast = !(cfg->flags & SDRFM_STEREO_CFG_FORCE_GENERIC) && T == 64 && D == 10 && P == 101 && ndt_fast >= 1 &&
            h->fast_lds <= ST_LDS_BUDGET;
  if (h->fast) snprintf(h->kernel_name, sizeof h->kernel_name, "stereo-fast T64 D10 P101 Ta%u Da%u", Ta, Da);
  else snprintf(h->kernel_name, sizeof h->kernel_name, "stereo-generic T%u D%u P%u Ta%u Da%u", T, D, P, Ta, Da);
  const int rc = sdrfm_stereo_reset(h);
  if (rc != SDRFM_OK) { stereo_free(h); return rc; }
  *out = h;
  return SDRFM_OK;
}

void sdrfm_stereo_destroy(sdrfm_stereo_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  stereo_free(h);
}

int sdrfm_stereo_reset(sdrfm_stereo_t* h) {
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

int sdrfm_stereo_audio_count(const sdrfm_stereo_t* h, uint32_t nbytes, uint32_t* n_audio) {
  if (!h || !n_audio) return SDRFM_EINVAL;
  if (nbytes & 1u) return SDRFM_EODD;
  const uint64_t M = (h->phase_x + (uint64_t)(nbytes / 2)) / h->cfg.fir_decim;
  *n_audio = (uint32_t)((h->phase_d + M) / h->cfg.audio_decim);
  return SDRFM_OK;
}

// one call on device buffers, enqueued on the handle's stream
static int stereo_enqueue(sdrfm_stereo* h, const uint8_t* d_iq, size_t iq_stride, uint32_t nbytes, float* d_left, float* d_right,
                          size_t audio_stride, uint32_t* d_pc, uint32_t* n_audio) {
  const uint32_t T = h->cfg.fir_taps, D = h->cfg.fir_decim, P = h->cfg.pilot_taps, Ta = h->cfg.audio_taps, Da = h->cfg.audio_decim;
  const uint32_t ns = h->cfg.n_streams, N = nbytes / 2;
  const uint32_t M = (h->phase_x + N) / D, A = (h->phase_d + M) / Da;
  StereoParams p;
  memset(&p, 0, sizeof p);
  p.iq = d_iq; p.iq_stride = iq_stride;
  p.left = d_left; p.right = d_right; p.audio_stride = audio_stride;
  p.pilot_count = d_pc;
  const int c = h->cur;
  p.hist_x_in = h->d_hist_x[c]; p.hist_x_out = h->d_hist_x[c ^ 1];
  p.yprev_in = h->d_yprev[c]; p.yprev_out = h->d_yprev[c ^ 1];
  p.hist_d_in = h->d_hist_d[c]; p.hist_d_out = h->d_hist_d[c ^ 1];
  p.h = h->d_h; p.g = h->d_g; p.tp = h->d_tp;
  p.T = T; p.D = D; p.P = P; p.Ta = Ta; p.Da = Da; p.H = h->H; p.Dl = (P - 1) / 2;
  p.pmin2 = h->cfg.pilot_min * h->cfg.pilot_min;
  p.diff_gain = h->cfg.diff_gain;
  p.N = N; p.M = M; p.A = A;
  p.e0 = (int32_t)(D - 1 - h->phase_x);
  p.f0 = (int32_t)(Da - 1 - h->phase_d);
  p.vec = ((uintptr_t)d_iq % 16 == 0 && (ns == 1 || iq_stride % 16 == 0)) ? 1u : 0u;
  size_t lds;
  if (h->fast) {
    p.NY = ST_FAST_NY;
    p.NDT = ST_FAST_NY - (Ta > 1 ? Ta - 1 : 1);
    lds = stereo_lds(64, 10, 101, Ta, h->H, p.NY, p.NDT, &p.region_words);
  } else {
    uint32_t ny = 1024;
    while (ny > 2 && stereo_lds(T, D, P, Ta, h->H, ny, ny - 1, nullptr) > ST_LDS_BUDGET) ny -= 2;
    p.NY = ny;
    p.NDT = ny - 1;
    lds = stereo_lds(T, D, P, Ta, h->H, p.NY, p.NDT, &p.region_words);
  }
  // every workgroup walks ~8 steps after its prologue; a stream gets at least one workgroup (the one that hands the state over)
  const uint32_t per = 8 * p.NDT;
  p.blocks_per_stream = M ? (M + per - 1) / per : 1;
  p.span = M ? (M + p.blocks_per_stream - 1) / p.blocks_per_stream : 0;
  if (d_pc && hipMemsetAsync(d_pc, 0, sizeof(uint32_t) * ns, h->stream) != hipSuccess) return SDRFM_FAIL;
  const dim3 grid(ns * p.blocks_per_stream), block(ST_THREADS);
  if (h->fast) k_stereo<64, 10, 101><<<grid, block, lds, h->stream>>>(p);
  else k_stereo<0, 0, 0><<<grid, block, lds, h->stream>>>(p);
  if (hipGetLastError() != hipSuccess) return SDRFM_FAIL;
  h->cur ^= 1;
  h->phase_x = (h->phase_x + N) % D;
  h->phase_d = (h->phase_d + M) % Da;
  *n_audio = A;
  return SDRFM_OK;
}

int sdrfm_stereo_process_batch(sdrfm_stereo_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, float* left, float* right,
                               size_t audio_stride, uint32_t* pilot_count, uint32_t* n_audio, uint32_t flags) {
  if (!h || !n_audio) return SDRFM_EINVAL;
  if (flags & ~SDRFM_F_DEVICE_PTRS) return SDRFM_EINVAL;       // SDRFM_F_OVERLAP: not for this handle
  if (nbytes & 1u) return SDRFM_EODD;
  if (nbytes > h->max_bytes) return SDRFM_ECAPACITY;
  const uint32_t ns = h->cfg.n_streams;
  if (nbytes == 0) {
    *n_audio = 0;
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
  (void)sdrfm_stereo_audio_count(h, nbytes, &A);
  if (A && (!left || !right)) return SDRFM_EINVAL;
  if (ns > 1 && audio_stride < A) return SDRFM_ECAPACITY;
  if (hipSetDevice(h->device) != hipSuccess) return SDRFM_FAIL;
  if (flags & SDRFM_F_DEVICE_PTRS) return stereo_enqueue(h, iq, iq_stride, nbytes, left, right, audio_stride, pilot_count, n_audio);

  if (hipMemcpy2DAsync(h->d_iq, h->d_iq_stride, iq, ns > 1 ? iq_stride : nbytes, nbytes, ns, hipMemcpyHostToDevice, h->stream) != hipSuccess)
    return SDRFM_FAIL;
  const int rc = stereo_enqueue(h, h->d_iq, h->d_iq_stride, nbytes, h->d_left, h->d_right, h->d_audio_stride, h->d_pc, n_audio);
  if (rc != SDRFM_OK) return rc;
  const size_t dst = (ns > 1 ? audio_stride : A) * sizeof(float), src = h->d_audio_stride * sizeof(float);
  if (A && (hipMemcpy2DAsync(left, dst, h->d_left, src, A * sizeof(float), ns, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
            hipMemcpy2DAsync(right, dst, h->d_right, src, A * sizeof(float), ns, hipMemcpyDeviceToHost, h->stream) != hipSuccess))
    return SDRFM_FAIL;
  if (pilot_count && hipMemcpyAsync(pilot_count, h->d_pc, sizeof(uint32_t) * ns, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return SDRFM_FAIL;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return SDRFM_FAIL;
  return SDRFM_OK;
}

int sdrfm_stereo_set_stream(sdrfm_stereo_t* h, void* hip_stream) {
  if (!h) return SDRFM_EINVAL;
  h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
  return SDRFM_OK;
}

int sdrfm_stereo_synchronize(sdrfm_stereo_t* h) {
  if (!h) return SDRFM_EINVAL;
  if (hipSetDevice(h->device) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return SDRFM_FAIL;
  return SDRFM_OK;
}

const char* sdrfm_stereo_kernel_name(const sdrfm_stereo_t* h) { return h ? h->kernel_name : ""; }

}  // extern "C"
