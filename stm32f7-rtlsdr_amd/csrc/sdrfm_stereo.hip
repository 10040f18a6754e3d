/*
 * sdrfm_stereo.hip — broadcast FM stereo decoding behind the sdrfm_stereo_* C-ABI (include/sdrfm.h).
 *
 * The walk from the input bytes to the pilot filter's q = b * d is sdrfm_pilot_front.h's, shared with the RDS kernel.  What this file
 * adds behind q, at the discriminator rate: the 38 kHz carrier c = -2 qr qi / |q|^2 (gated by |q|^2 >= pilot_min^2; sdrfm_carrier.h), the difference
 * signal s = (c * diff_gain) d[m - Δ] over the step's audio windows -> LDS, and the two audio chains am (on d delayed by Δ) and as
 * (on s), L = am + as, R = am - as -> HBM (sdrfm_out_stages.h, shared with the broadcast kernel).  H = P - 1 + Ta - 1.
 *
 * k_stereo<0, 0, 0> and k_stereo<64, 10, 101> are the header's two forms of the walk; the carrier and the audio chains are the same code in both.
 */
#include <new>

#include "sdrfm_carrier.h"
#include "sdrfm_out_stages.h"
#include "sdrfm_pilot_front.h"
#include "sdrfm_sink_stereo.h"

namespace {

struct StereoParams : FrontParams {
  float* left;
  float* right;
  size_t audio_stride;
  const float* g;              // Ta
  uint32_t Ta, Da;
  float diff_gain;
  uint32_t A;
  int32_t f0;
};

template <int FT, int FD, int FP>
__global__ void __launch_bounds__(PF_THREADS) k_stereo(StereoParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t P = FT > 0 ? FP : p.P;
  const uint32_t Ta = p.Ta, Da = p.Da, H = p.H, Dl = p.Dl, NY = p.NY, NDT = p.NDT;
  // LDS: region (x as f16 pairs | d's and s's) | ys[NY] | hb[H] | tps[P] | gs[Ta] | hs[T]
  FrontWg<FT, FD, FP> w;
  w.xs = reinterpret_cast<h2_t*>(smem);
  w.ds = reinterpret_cast<float*>(smem);
  float* ss = w.ds + H + NDT;                                   // [Ta - 1 + NDT]: s of the step's audio windows
  w.ys = reinterpret_cast<f2_t*>(smem + 4 * (size_t)p.region_words);
  w.hb = reinterpret_cast<float*>(w.ys + NY);
  w.tps = reinterpret_cast<f2_t*>(w.hb + ((H + 1) & ~1u));
  float* gs = reinterpret_cast<float*>(w.tps + P);
  w.hs = gs + Ta;
  front_begin(p, w);
  const int tid = w.tid, nthr = w.nthr;
  const uint32_t s = w.s;
  const float* ds = w.ds;
  for (int k = tid; k < (int)Ta; k += nthr) gs[k] = p.g[k];
  uint32_t cnt = 0;

  front_walk(p, w, [&](int a, int b, bool full) {
    front_d_stage(p, w, a, b);
    if (full) {
      // ---- pilot filter, carrier, s for m in [a - (Ta - 1), b)
      front_pilot(w, 0, b - a + (int)Ta - 1, [&](int o, f2_t q) __attribute__((always_inline)) {
        float sv;
        const bool on = carrier_stereo(p.pmin2, p.diff_gain, q, ds[o + Dl], sv);
        ss[o] = sv;
        cnt += (on && o >= (int)Ta - 1) ? 1u : 0u;
      });
      __syncthreads();
      // ---- audio: outputs j whose newest d lies in [a, b), one per lane
      const int2 jr = step_outputs(a, b, p.f0, (int)Da, (int)p.A);
      audio_outputs(ds, ss, gs, Ta, Da, p.f0, a, H, Dl, jr.x + tid, nthr, jr.y, p.left + (size_t)s * p.audio_stride, p.right + (size_t)s * p.audio_stride);
    }
    __syncthreads();
  });

  front_count(p, s, tid, cnt);
  front_hand_over(p, w);
}

}  // namespace

// =================================================================================================================
//  Host side: handle, argument checks (all before any device work), launch geometry.  The walk's state is the header's PilotFront.
// =================================================================================================================
struct sdrfm_stereo {
  sdrfm_stereo_config cfg;                     // taps pointers point at the copies in f and below
  PilotFront f;
  Decim au;                                    // the audio decimator
  float* d_left = nullptr;
  float* d_right = nullptr;
  size_t d_audio_stride = 0;
  bool fast = false;
  FrontStep step;                              // of the kernel this handle launches
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
  front_free(h->f);
  decim_free(h->au);
  (void)hipFree(h->d_left); (void)hipFree(h->d_right);
  delete h;
}

}  // namespace

extern "C" {

int sdrfm_stereo_create(const sdrfm_stereo_config* cfg, sdrfm_stereo_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!cfg || cfg->struct_size != sizeof(sdrfm_stereo_config)) return SDRFM_EINVAL;
  if (!front_config_ok(cfg->n_streams, cfg->fir_taps, cfg->fir_decim, cfg->fir_coeffs, cfg->pilot_taps, cfg->pilot_coeffs, cfg->pilot_min))
    return SDRFM_EINVAL;
  if (cfg->flags & ~SDRFM_STEREO_CFG_FORCE_GENERIC) return SDRFM_EINVAL;
  if (!decim_config_ok(cfg->audio_taps, cfg->audio_decim, cfg->audio_coeffs, cfg->diff_gain)) return SDRFM_EINVAL;
  hipDeviceProp_t prop;
  int rc = front_open_device(cfg->device, &prop);
  if (rc != SDRFM_OK) return rc;

  sdrfm_stereo* h = new (std::nothrow) sdrfm_stereo();
  if (!h) return SDRFM_ENOMEM;
  h->cfg = *cfg;
  const uint32_t T = cfg->fir_taps, D = cfg->fir_decim, P = cfg->pilot_taps, Ta = cfg->audio_taps, Da = cfg->audio_decim, H = P - 1 + Ta - 1;
  const size_t ns = cfg->n_streams;
  rc = front_alloc(h->f, cfg->n_streams, T, D, cfg->fir_coeffs, P, cfg->pilot_coeffs, cfg->pilot_min, H, cfg->max_bytes_per_call, cfg->device);
  if (rc != SDRFM_OK) { stereo_free(h); return rc; }
  rc = decim_alloc(h->au, h->f, Ta, Da, cfg->audio_coeffs);
  if (rc != SDRFM_OK) { stereo_free(h); return rc; }
  h->cfg.fir_coeffs = h->f.hc;
  h->cfg.audio_coeffs = h->au.gc;
  h->cfg.pilot_coeffs = h->f.bc;
  h->d_audio_stride = ((size_t)h->au.max_out + 63) & ~(size_t)63;
  const size_t audio_bytes = sizeof(float) * h->d_audio_stride * ns;
  if (hipMalloc(&h->d_left, audio_bytes) != hipSuccess || hipMalloc(&h->d_right, audio_bytes) != hipSuccess) { stereo_free(h); return SDRFM_ENOMEM; }
  const uint32_t ndt_fast = PF_FAST_NY - (Ta > 1 ? Ta - 1 : 1);
  h->step = front_step(stereo_lds, 64, 10, 101, Ta, H, PF_FAST_NY, ndt_fast);
  h->fast = !(cfg->flags & SDRFM_STEREO_CFG_FORCE_GENERIC) && T == 64 && D == 10 && P == 101 && ndt_fast >= 1 && h->step.lds <= PF_LDS_BUDGET;
  if (!h->fast) h->step = front_step_generic(stereo_lds, T, D, P, Ta, H);
  if (h->fast) snprintf(h->kernel_name, sizeof h->kernel_name, "stereo-fast T64 D10 P101 Ta%u Da%u", Ta, Da);
  else snprintf(h->kernel_name, sizeof h->kernel_name, "stereo-generic T%u D%u P%u Ta%u Da%u", T, D, P, Ta, Da);
  rc = sdrfm_stereo_reset(h);
  if (rc != SDRFM_OK) { stereo_free(h); return rc; }
  *out = h;
  return SDRFM_OK;
}

void sdrfm_stereo_destroy(sdrfm_stereo_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->f.device);
  (void)hipStreamSynchronize(h->f.stream);
  stereo_free(h);
}

int sdrfm_stereo_reset(sdrfm_stereo_t* h) {
  if (!h) return SDRFM_EINVAL;
  const int rc = front_reset(h->f);
  if (rc != SDRFM_OK) return rc;
  decim_reset(h->au);
  return SDRFM_OK;
}

int sdrfm_stereo_audio_count(const sdrfm_stereo_t* h, uint32_t nbytes, uint32_t* n_audio) {
  if (!h || !n_audio) return SDRFM_EINVAL;
  if (nbytes & 1u) return SDRFM_EODD;
  *n_audio = decim_outputs(h->au, front_new_d(h->f, nbytes));
  return SDRFM_OK;
}

// one call on device buffers, enqueued on the handle's stream
static int stereo_enqueue(sdrfm_stereo* h, const uint8_t* d_iq, size_t iq_stride, uint32_t nbytes, float* d_left, float* d_right,
                          size_t audio_stride, uint32_t* d_pc, uint32_t* n_audio) {
  const uint32_t ns = h->cfg.n_streams;
  StereoParams p;
  memset(&p, 0, sizeof p);
  front_fill(h->f, p, d_iq, iq_stride, nbytes, d_pc, h->step);
  const uint32_t M = p.M, A = decim_outputs(h->au, M);
  p.left = d_left; p.right = d_right; p.audio_stride = audio_stride;
  p.g = h->au.d_g;
  p.Ta = h->au.T; p.Da = h->au.D;
  p.diff_gain = h->cfg.diff_gain;
  p.A = A;
  p.f0 = decim_f0(h->au);
  // every workgroup walks ~8 steps after its prologue; a stream gets at least one workgroup (the one that hands the state over)
  const uint32_t per = 8 * p.NDT;
  p.blocks_per_stream = M ? (M + per - 1) / per : 1;
  p.span = M ? (M + p.blocks_per_stream - 1) / p.blocks_per_stream : 0;
  if (front_zero_count(h->f, d_pc, true) != SDRFM_OK) return SDRFM_FAIL;
  const dim3 grid(ns * p.blocks_per_stream), block(PF_THREADS);
  if (h->fast) k_stereo<64, 10, 101><<<grid, block, h->step.lds, h->f.stream>>>(p);
  else k_stereo<0, 0, 0><<<grid, block, h->step.lds, h->f.stream>>>(p);
  if (hipGetLastError() != hipSuccess) return SDRFM_FAIL;
  front_advance(h->f, p.N);
  decim_advance(h->au, M);
  *n_audio = A;
  return SDRFM_OK;
}

int sdrfm_stereo_process_batch(sdrfm_stereo_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, float* left, float* right,
                               size_t audio_stride, uint32_t* pilot_count, uint32_t* n_audio, uint32_t flags) {
  if (!h || !n_audio) return SDRFM_EINVAL;
  if (flags & ~SDRFM_F_DEVICE_PTRS) return SDRFM_EINVAL;       // SDRFM_F_OVERLAP: not for this handle
  if (nbytes & 1u) return SDRFM_EODD;
  if (nbytes > h->f.max_bytes) return SDRFM_ECAPACITY;
  const uint32_t ns = h->cfg.n_streams;
  if (nbytes == 0) {
    *n_audio = 0;
    return front_empty_call(h->f, pilot_count, flags);
  }
  if (!iq) return SDRFM_EINVAL;
  if (ns > 1 && iq_stride < nbytes) return SDRFM_ECAPACITY;
  uint32_t A = 0;
  (void)sdrfm_stereo_audio_count(h, nbytes, &A);
  if (A && (!left || !right)) return SDRFM_EINVAL;
  if (ns > 1 && audio_stride < A) return SDRFM_ECAPACITY;
  if (hipSetDevice(h->f.device) != hipSuccess) return SDRFM_FAIL;
  if (flags & SDRFM_F_DEVICE_PTRS) return stereo_enqueue(h, iq, iq_stride, nbytes, left, right, audio_stride, pilot_count, n_audio);

  if (front_stage_in(h->f, iq, iq_stride, nbytes) != SDRFM_OK) return SDRFM_FAIL;
  const int rc = stereo_enqueue(h, h->f.d_iq, h->f.d_iq_stride, nbytes, h->d_left, h->d_right, h->d_audio_stride, h->f.d_pc, n_audio);
  if (rc != SDRFM_OK) return rc;
  if (front_copy_back(h->f, left, audio_stride, h->d_left, h->d_audio_stride, A) != SDRFM_OK) return SDRFM_FAIL;
  if (front_copy_back(h->f, right, audio_stride, h->d_right, h->d_audio_stride, A) != SDRFM_OK) return SDRFM_FAIL;
  return front_finish(h->f, pilot_count);
}

// the call above and, behind it on the handle's stream, the stereo sink's default kernel over this call's L and R rows
int sdrfm_stereo_process_batch_pcm(sdrfm_stereo_t* h, sdrfm_pcm_stereo_sink_t* sink, const uint8_t* iq, size_t iq_stride, uint32_t nbytes,
                                   float* left, float* right, size_t audio_stride, int16_t* pcm, size_t pcm_stride, uint32_t* pilot_count,
                                   uint32_t* n_audio, uint32_t flags) {
  if (!h || !sink || !n_audio) return SDRFM_EINVAL;
  if (flags & ~SDRFM_F_DEVICE_PTRS) return SDRFM_EINVAL;
  if (!left != !right) return SDRFM_EINVAL;                    // both, or neither: the sink then reads the handle's own rows
  if (nbytes & 1u) return SDRFM_EODD;
  if (nbytes > h->f.max_bytes) return SDRFM_ECAPACITY;
  const uint32_t ns = h->cfg.n_streams;
  const bool dev = (flags & SDRFM_F_DEVICE_PTRS) != 0;
  uint32_t A = 0;
  (void)sdrfm_stereo_audio_count(h, nbytes, &A);
  int rc = sdrfm_stereo_sink_check(sink, h->f.device, ns, A, pcm, pcm_stride, dev);
  if (rc != SDRFM_OK) return rc;
  if (nbytes == 0) {
    *n_audio = 0;
    return front_empty_call(h->f, pilot_count, flags);
  }
  if (!iq) return SDRFM_EINVAL;
  if (ns > 1 && iq_stride < nbytes) return SDRFM_ECAPACITY;
  if (left && ns > 1 && audio_stride < A) return SDRFM_ECAPACITY;
  if (hipSetDevice(h->f.device) != hipSuccess) return SDRFM_FAIL;
  if (dev) {
    float* const l = left ? left : h->d_left;
    float* const r = left ? right : h->d_right;
    const size_t as = left ? audio_stride : h->d_audio_stride;
    rc = stereo_enqueue(h, iq, iq_stride, nbytes, l, r, as, pilot_count, n_audio);
    if (rc != SDRFM_OK) return rc;
    return sdrfm_stereo_sink_launch_on(sink, l, r, as, A, pcm, pcm_stride, h->f.stream);
  }

  int16_t* d_pcm = nullptr;
  size_t d_pcm_stride = 0;
  rc = sdrfm_stereo_sink_reserve(sink, A, &d_pcm, &d_pcm_stride);   // (before anything is enqueued: a refusal leaves both handles alone)
  if (rc != SDRFM_OK) return rc;
  if (front_stage_in(h->f, iq, iq_stride, nbytes) != SDRFM_OK) return SDRFM_FAIL;
  rc = stereo_enqueue(h, h->f.d_iq, h->f.d_iq_stride, nbytes, h->d_left, h->d_right, h->d_audio_stride, h->f.d_pc, n_audio);
  if (rc != SDRFM_OK) return rc;
  rc = sdrfm_stereo_sink_launch_on(sink, h->d_left, h->d_right, h->d_audio_stride, A, d_pcm, d_pcm_stride, h->f.stream);
  if (rc != SDRFM_OK) return rc;
  if (left && front_copy_back(h->f, left, audio_stride, h->d_left, h->d_audio_stride, A) != SDRFM_OK) return SDRFM_FAIL;
  if (left && front_copy_back(h->f, right, audio_stride, h->d_right, h->d_audio_stride, A) != SDRFM_OK) return SDRFM_FAIL;
  if (sdrfm_stereo_sink_copy_back(sink, pcm, pcm_stride, A, h->f.stream) != SDRFM_OK) return SDRFM_FAIL;
  return front_finish(h->f, pilot_count);
}

int sdrfm_stereo_set_stream(sdrfm_stereo_t* h, void* hip_stream) {
  if (!h) return SDRFM_EINVAL;
  return front_use_stream(h->f, hip_stream);
}

int sdrfm_stereo_synchronize(sdrfm_stereo_t* h) {
  if (!h) return SDRFM_EINVAL;
  if (hipSetDevice(h->f.device) != hipSuccess || hipStreamSynchronize(h->f.stream) != hipSuccess) return SDRFM_FAIL;
  return SDRFM_OK;
}

const char* sdrfm_stereo_kernel_name(const sdrfm_stereo_t* h) { return h ? h->kernel_name : ""; }

}  // extern "C"
