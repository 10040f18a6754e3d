/*
 * sdrfm_sink_stereo.hip — the device-side STEREO audio sink behind the sdrfm_pcm_stereo_sink_* C-ABI (include/sdrfm.h): the L and R
 * rows the stereo and the broadcast handles leave (f32, 48 kHz) -> FM de-emphasis of either channel on its own -> int16 stereo-interleaved PCM in the
 * layout BSP_AUDIO_OUT_Play consumes, pcm[2i] = L, pcm[2i+1] = R.  Per channel the arithmetic is the host routine sdrfm_pcm_deemph_stereo_s16's
 * (csrc/pcm_sink.c), operation for operation:
 *
 *   y[n]   = fmaf(alpha, x[n] - y[n-1], y[n-1])
 *   pcm[n] = (int16) rint(clamp(y[n] * gain, -32768, 32767))      one dword per sample: L | R << 16
 *
 * The two forms of the mono sink (sdrfm_sink.hip), each walking TWO chains in a lane.  Both sinks instantiate the same two bodies of sdrfm_sink_kernels.h,
 * the mono sink for one channel and this one for two, so PER CHANNEL the operations and their order are the mono sink's by construction:
 *   k_pcm_stereo_sink       SDRFM_PCM_F_EXACT, sink_exact_tiles<2>: one lane per stream, 64 streams per wave, the data moved coalesced through two
 *                           64 x 65-word LDS tiles (L and R), the packed PCM written back into the L tile in place.  Bit-identical to the host routine,
 *                           PCM and state.
 *   k_pcm_stereo_sink_scan  the default, sink_scan_segments<2>: one workgroup of 256 lanes per stream, the lane's 19-sample chunk of L and the same chunk
 *                           of R in registers, both chains through the scan's three phases side by side.  The chain is latency-bound (sub -> fma), so
 *                           the second, independent chain fills slots the first leaves empty.  The even PCM slots are bit for bit what the mono default
 *                           sink leaves for the L rows and the odd slots what it leaves for the R rows (tests/test_pcm_stereo_sink_gpu.py confirms it).
 *                           LDS: two segments + eight carry words, 38 KiB.
 * A CONDITIONED sink (sdrfm_pcm_stereo_sink_set_hicut) launches the two kernels of sdrfm_sink_hicut.h's bodies in their place: the same
 * two geometries with a coefficient that differs per stream and moves per sample.  A sink that never asks for a high-cut launches the two above.
 *   k_pcm_stereo_sink_hicut       SDRFM_PCM_F_EXACT: bit-identical to sdrfm_pcm_deemph_stereo_hicut_s16, PCM and both states.
 *   k_pcm_stereo_sink_hicut_scan  the default: the blocked scan over affine maps, a chunk's decay walked beside its contribution.
 * What this sink leaves out on purpose: it takes no part in the in-launch chain protocol (sdrfm_sink_chain.h) — no tagged state slots, no waits on the
 * device, no atomics.  The state is a plain float[n_streams][2]; a stream's workgroup (its lane, in the exact form) reads it at the start and writes
 * it at the end, and calls on one HIP stream are ordered.
 * A METERED sink (sdrfm_pcm_stereo_sink_meter_enable) follows every launch of any of the four with one launch of
 *   k_pcm_audio_meter       one workgroup of 256 lanes per stream over the PCM row just written (sdrfm_audio_meter.h): the call's integer record
 *                           joined onto the stream's.  A kernel of its own for the reason the sink is one: the four above keep their bits.
 * A sink with LOUDNESS enabled (sdrfm_pcm_stereo_sink_loudness_enable) follows every launch, and the meter's if there is one, with
 *   k_pcm_loudness          one workgroup of 256 lanes per stream over the same PCM row (sdrfm_loudness.h): K-weighting in double by a two-pass
 *                           blocked scan, the sub-block energies into the stream's ring.
 * A sink with TRUE PEAK enabled (sdrfm_pcm_stereo_sink_truepeak_enable) follows every launch, and those two if there are any, with
 *   k_pcm_truepeak          one workgroup of 1024 lanes per stream over the same PCM row (sdrfm_truepeak.h): a polyphase FIR in packed 16-bit dot
 *                           products over LDS-staged planes, the peak and its place by a max over 64-bit keys.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/sdrfm.h"
#include "sdrfm_audio_ctl.h"
#include "sdrfm_audio_meter.h"
#include "sdrfm_loudness.h"
#include "sdrfm_sink_hicut.h"
#include "sdrfm_sink_kernels.h"
#include "sdrfm_sink_stereo.h"
#include "sdrfm_truepeak.h"

namespace {

struct StereoSinkParams {
  const float* left;
  const float* right;
  size_t audio_stride;   // floats
  int16_t* pcm;
  size_t pcm_stride;     // int16 elements per stream (>= 2 * n)
  float* state;          // [n_streams][2]: y[n-1] of L, of R
  uint32_t n_streams, n;
  float alpha, gain;
};

__global__ void __launch_bounds__(64) k_pcm_stereo_sink(StereoSinkParams p) {
  __shared__ unsigned tile[2][64 * 65];                         // L and R
  const uint32_t lane = threadIdx.x;
  const uint32_t s0 = blockIdx.x * 64;
  const uint32_t rows = (p.n_streams - s0 < 64u) ? p.n_streams - s0 : 64u;
  const uint32_t mine = s0 + lane;
  float y[2] = {(lane < rows) ? p.state[2 * (size_t)mine] : 0.0f, (lane < rows) ? p.state[2 * (size_t)mine + 1] : 0.0f};
  const float* const in[2] = {p.left, p.right};
  sink_exact_tiles<2>(tile, in, p.audio_stride, p.pcm, p.pcm_stride, s0, rows, p.n, p.alpha, p.gain, y);
  if (lane < rows) {
    p.state[2 * (size_t)mine] = y[0];
    p.state[2 * (size_t)mine + 1] = y[1];
  }
}

__global__ void __launch_bounds__(256) k_pcm_stereo_sink_scan(StereoSinkParams p, float pc) {
  __shared__ float x[2][SINK_SEG];
  __shared__ float sc[2][4];
  const uint32_t s = blockIdx.x;
  const float* const row[2] = {p.left + (size_t)s * p.audio_stride, p.right + (size_t)s * p.audio_stride};
  float y0[2] = {p.state[2 * (size_t)s], p.state[2 * (size_t)s + 1]};
  sink_scan_segments<2>(x, sc, row, reinterpret_cast<unsigned*>(p.pcm + (size_t)s * p.pcm_stride), p.n, p.alpha, p.gain, pc, y0);
  if (threadIdx.x == 0) {
    p.state[2 * (size_t)s] = y0[0];
    p.state[2 * (size_t)s + 1] = y0[1];
  }
}

// ---- the conditioned forms: the same geometries, the lane's (the workgroup's) record beside the state ------------------------------------------------------
__global__ void __launch_bounds__(64) k_pcm_stereo_sink_hicut(StereoSinkParams p, HicutParams hp) {
  __shared__ unsigned tile[2][64 * 65];                         // L and R
  const uint32_t lane = threadIdx.x;
  const uint32_t s0 = blockIdx.x * 64;
  const uint32_t rows = (p.n_streams - s0 < 64u) ? p.n_streams - s0 : 64u;
  const uint32_t mine = s0 + lane;
  float y[2] = {(lane < rows) ? p.state[2 * (size_t)mine] : 0.0f, (lane < rows) ? p.state[2 * (size_t)mine + 1] : 0.0f};
  const HicutRec r = (lane < rows) ? hp.rec[mine] : HicutRec{(uint16_t)SDRFM_ACTL_ONE, (uint16_t)SDRFM_ACTL_ONE};
  const float* const in[2] = {p.left, p.right};
  hicut_exact_tiles(tile, in, p.audio_stride, p.pcm, p.pcm_stride, s0, rows, p.n, p.alpha, p.gain, r, hp.slew, hp.J, y);
  if (lane < rows) {
    p.state[2 * (size_t)mine] = y[0];
    p.state[2 * (size_t)mine + 1] = y[1];
  }
}

__global__ void __launch_bounds__(256) k_pcm_stereo_sink_hicut_scan(StereoSinkParams p, HicutParams hp) {
  __shared__ float x[2][SINK_SEG];
  __shared__ float sc[3][4];                                    // the waves' totals: s of L, s of R, A
  const uint32_t s = blockIdx.x;
  const float* const row[2] = {p.left + (size_t)s * p.audio_stride, p.right + (size_t)s * p.audio_stride};
  float y0[2] = {p.state[2 * (size_t)s], p.state[2 * (size_t)s + 1]};
  hicut_scan_segments(x, sc, row, reinterpret_cast<unsigned*>(p.pcm + (size_t)s * p.pcm_stride), p.n, p.alpha, p.gain, hp.rec[s], hp.slew, hp.J, y0);
  if (threadIdx.x == 0) {
    p.state[2 * (size_t)s] = y0[0];
    p.state[2 * (size_t)s + 1] = y0[1];
  }
}

// ---- the audio meter: reads what any of the four wrote ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SDRFM_AM_NT) k_pcm_audio_meter(AudioMeterParams p) {
  __shared__ sdrfm_audio_meter part[SDRFM_AM_NT / 64];
  audio_meter_stream(part, p);
}

// ---- the loudness meter: reads the same rows ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SDRFM_LD_NT) k_pcm_loudness(LoudnessParams p) {
  __shared__ LoudnessShared sh;
  loudness_stream(sh, p);
}

// ---- the true-peak meter: reads the same rows ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SDRFM_TP_NT) k_pcm_truepeak(TruePeakParams p) {
  __shared__ TruePeakShared sh;
  truepeak_stream(sh, p);
}

}  // namespace

struct sdrfm_pcm_stereo_sink {
  uint32_t n_streams;
  float alpha, gain;
  HostStream hs;
  float* d_state;      // [n_streams][2]
  RowStage stage;      // staging for host-pointer calls: floats in, the streams' left rows then their right rows; (L, R) pairs out
  // the high-cut (sdrfm_pcm_stereo_sink_set_hicut): the streams' ramps on the host and, from the first set on, on the device; the sink's slew and the
  // samples taken since the last set (saturated).  hicut: the sink is conditioned and launches the conditioned kernels
  HicutRec* hc_host;   // [n_streams]
  HicutRec* d_hc;
  uint32_t slew, J;
  bool hicut;
  // the audio meter (sdrfm_pcm_stereo_sink_meter_enable): the streams' records on the device, from the first enable on; meter: the sink is
  // metered and every launch is followed by the meter kernel
  sdrfm_audio_meter* d_meter;   // [n_streams]
  uint32_t quiet_lsb;
  bool meter;
  // the loudness meter (sdrfm_pcm_stereo_sink_loudness_enable): states, ring and matrix powers on the device while enabled; lpos mirrors the
  // streams' pos (every stream receives the same n), lread = the sub-blocks already handed out
  sdrfm_loudness_state* d_lstate;   // [n_streams]
  sdrfm_loudness_block* d_lring;    // [n_streams][lcap]
  double* d_lpw;                    // [SDRFM_LD_TABLE]
  sdrfm_loudness_coef lcoef;
  uint32_t lblock, lcap;
  uint64_t lpos, lread;
  bool loud;
  // the true-peak meter (sdrfm_pcm_stereo_sink_truepeak_enable): records, histories and the packed table on the device while enabled
  sdrfm_truepeak* d_tprec;          // [n_streams]
  unsigned* d_tphist;               // [n_streams][tp_nt - 1] pairs
  unsigned* d_tptab;                // [tp_P][tp_nt / 2]
  uint64_t tp_limit;
  uint32_t tp_P, tp_nt;
  bool tpeak;
};

static const HicutRec HICUT_FLAT = {(uint16_t)SDRFM_ACTL_ONE, (uint16_t)SDRFM_ACTL_ONE};

static void stereo_sink_free(sdrfm_pcm_stereo_sink* k) {
  if (!k) return;
  (void)hipSetDevice(k->hs.device);
  if (k->d_state) (void)hipFree(k->d_state);
  row_stage_free(k->stage);
  if (k->d_hc) (void)hipFree(k->d_hc);
  if (k->d_meter) (void)hipFree(k->d_meter);
  if (k->d_lstate) (void)hipFree(k->d_lstate);
  if (k->d_lring) (void)hipFree(k->d_lring);
  if (k->d_lpw) (void)hipFree(k->d_lpw);
  if (k->d_tprec) (void)hipFree(k->d_tprec);
  if (k->d_tphist) (void)hipFree(k->d_tphist);
  if (k->d_tptab) (void)hipFree(k->d_tptab);
  free(k->hc_host);
  host_stream_close(k->hs);
  delete k;
}

static StereoSinkParams stereo_sink_params(const sdrfm_pcm_stereo_sink* k, const float* left, const float* right, size_t audio_stride, uint32_t n,
                                           int16_t* pcm, size_t pcm_stride) {
  StereoSinkParams p;
  p.left = left; p.right = right; p.audio_stride = audio_stride; p.pcm = pcm; p.pcm_stride = pcm_stride;
  p.state = k->d_state; p.n_streams = k->n_streams; p.n = n; p.alpha = k->alpha; p.gain = k->gain;
  return p;
}

// the checks every call makes of its PCM rows against n > 0 outputs
static int stereo_sink_pcm_ok(uint32_t n_streams, uint32_t n, const int16_t* pcm, size_t pcm_stride, bool device_ptrs) {
  if (!pcm) return SDRFM_EINVAL;
  if (!pcm_rows_capacity(n_streams, pcm_stride, 2 * (size_t)n)) return SDRFM_ECAPACITY;   // unlike the three newer handles: before the odd stride
  if (pcm_stride & 1u) return SDRFM_EINVAL;                        // rows are written as (L, R) dwords
  if (device_ptrs && (uintptr_t)pcm % 4 != 0) return SDRFM_EINVAL;
  return SDRFM_OK;
}

// ---- the sink behind a stereo or a broadcast launch (sdrfm_sink_stereo.h) ----------------------------------------------------------------------------
int sdrfm_stereo_sink_check(const sdrfm_pcm_stereo_sink* k, int device, uint32_t n_streams, uint32_t n, const int16_t* pcm, size_t pcm_stride,
                            bool device_ptrs) {
  if (!k || k->hs.device != device || k->n_streams != n_streams) return SDRFM_EINVAL;
  return n ? stereo_sink_pcm_ok(n_streams, n, pcm, pcm_stride, device_ptrs) : SDRFM_OK;
}

int sdrfm_stereo_sink_reserve(sdrfm_pcm_stereo_sink* k, uint32_t n, int16_t** d_pcm, size_t* d_pcm_stride) {
  if (!k) return SDRFM_EINVAL;
  const int rc = row_stage_reserve(k->stage, RowShape{1024u, sizeof(float), 2 * (size_t)k->n_streams, PCM_PAIR_BYTES, k->n_streams, false}, n, n);
  if (rc != SDRFM_OK) return rc;
  if (d_pcm) *d_pcm = static_cast<int16_t*>(k->stage.d_out);
  if (d_pcm_stride) *d_pcm_stride = 2 * (size_t)k->stage.cap_out;
  return SDRFM_OK;
}

// one call of the sink over device buffers, in either form, on `stream`
static int stereo_sink_launch(sdrfm_pcm_stereo_sink* k, const float* left, const float* right, size_t audio_stride, uint32_t n, int16_t* pcm, size_t pcm_stride,
                              hipStream_t stream, bool exact) {
  const StereoSinkParams p = stereo_sink_params(k, left, right, audio_stride, n, pcm, pcm_stride);
  if (k->hicut) {
    const HicutParams hp = {k->d_hc, k->slew, k->J};
    if (exact) hipLaunchKernelGGL(k_pcm_stereo_sink_hicut, dim3((k->n_streams + 63) / 64), dim3(64), 0, stream, p, hp);
    else hipLaunchKernelGGL(k_pcm_stereo_sink_hicut_scan, dim3(k->n_streams), dim3(SINK_NT), 0, stream, p, hp);
  } else if (exact) hipLaunchKernelGGL(k_pcm_stereo_sink, dim3((k->n_streams + 63) / 64), dim3(64), 0, stream, p);
  else hipLaunchKernelGGL(k_pcm_stereo_sink_scan, dim3(k->n_streams), dim3(SINK_NT), 0, stream, p, sink_carry_factor(k->alpha));
  STRY(hipGetLastError(), SDRFM_FAIL);
  k->J = audio_ctl_advance(k->J, n);                            // the samples since the last set: the next call's ramps go on from here
  if (k->meter) {                                               // behind the rows just written, on the same stream
    const AudioMeterParams mp = {pcm, pcm_stride, k->d_meter, n, k->quiet_lsb};
    hipLaunchKernelGGL(k_pcm_audio_meter, dim3(k->n_streams), dim3(SDRFM_AM_NT), 0, stream, mp);
    STRY(hipGetLastError(), SDRFM_FAIL);
  }
  if (k->loud) {                                                // behind the meter, over the same rows
    LoudnessParams lp;
    lp.pcm = pcm; lp.pcm_stride = pcm_stride; lp.state = k->d_lstate; lp.ring = k->d_lring; lp.pw = k->d_lpw; lp.coef = k->lcoef;
    lp.blk0 = k->lpos / k->lblock;
    lp.keep_from = ld_keep_from((k->lpos + n) / k->lblock, k->lcap);
    lp.n = n; lp.block_len = k->lblock; lp.cap_blocks = k->lcap; lp.off0 = (uint32_t)(k->lpos % k->lblock);
    hipLaunchKernelGGL(k_pcm_loudness, dim3(k->n_streams), dim3(SDRFM_LD_NT), 0, stream, lp);
    STRY(hipGetLastError(), SDRFM_FAIL);
    k->lpos += n;                                               // the host's mirror of every stream's pos
  }
  if (k->tpeak) {                                               // behind both, over the same rows
    const TruePeakParams tp = {pcm, pcm_stride, k->d_tprec, k->d_tphist, k->d_tptab, k->tp_limit, n, k->tp_nt, k->tp_P};
    hipLaunchKernelGGL(k_pcm_truepeak, dim3(k->n_streams), dim3(SDRFM_TP_NT), 0, stream, tp);
    STRY(hipGetLastError(), SDRFM_FAIL);
  }
  return SDRFM_OK;
}

int sdrfm_stereo_sink_launch_on(sdrfm_pcm_stereo_sink* k, const float* left, const float* right, size_t audio_stride, uint32_t n, int16_t* pcm,
                                size_t pcm_stride, hipStream_t stream) {
  if (!k) return SDRFM_EINVAL;
  if (n == 0) return SDRFM_OK;
  return stereo_sink_launch(k, left, right, audio_stride, n, pcm, pcm_stride, stream, false);
}

int sdrfm_stereo_sink_copy_back(const sdrfm_pcm_stereo_sink* k, int16_t* pcm, size_t pcm_stride, uint32_t n, hipStream_t stream) {
  if (!k) return SDRFM_EINVAL;
  if (n == 0) return SDRFM_OK;
  const size_t ps = pcm_rows_pitch(k->n_streams, pcm_stride, 2 * (size_t)n);
  STRY(hipMemcpy2DAsync(pcm, sizeof(int16_t) * ps, k->stage.d_out, PCM_PAIR_BYTES * k->stage.cap_out, PCM_PAIR_BYTES * n, k->n_streams,
                        hipMemcpyDeviceToHost, stream), SDRFM_FAIL);
  return SDRFM_OK;
}

extern "C" {

int sdrfm_pcm_stereo_sink_create(uint32_t n_streams, float alpha, float gain, int32_t device, sdrfm_pcm_stereo_sink_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!n_streams || !(alpha > 0.0f) || alpha > 1.0f || !(gain == gain)) return SDRFM_EINVAL;
  if (const int rc = host_open_device(device); rc != SDRFM_OK) return rc;
  sdrfm_pcm_stereo_sink* k = new (std::nothrow) sdrfm_pcm_stereo_sink();
  if (!k) return SDRFM_ENOMEM;
  memset(static_cast<void*>(k), 0, sizeof(*k));
  k->n_streams = n_streams; k->alpha = alpha; k->gain = gain; k->hs.device = device;
  k->slew = SDRFM_ACTL_ONE; k->J = SDRFM_ACTL_J_MAX;
  k->hc_host = (HicutRec*)malloc(sizeof(HicutRec) * (size_t)n_streams);
  if (!k->hc_host) { stereo_sink_free(k); return SDRFM_ENOMEM; }
  for (size_t s = 0; s < n_streams; ++s) k->hc_host[s] = HICUT_FLAT;
  if (host_stream_open(k->hs, device) != SDRFM_OK ||
      hipMalloc(&k->d_state, sizeof(float) * 2 * (size_t)n_streams) != hipSuccess) { stereo_sink_free(k); return SDRFM_ENOMEM; }
  const int rc = sdrfm_pcm_stereo_sink_reset(k);
  if (rc != SDRFM_OK) { stereo_sink_free(k); return rc; }
  *out = k;
  return SDRFM_OK;
}

void sdrfm_pcm_stereo_sink_destroy(sdrfm_pcm_stereo_sink_t* k) {
  if (!k) return;
  (void)host_stream_wait(k->hs);
  stereo_sink_free(k);
}

int sdrfm_pcm_stereo_sink_reset(sdrfm_pcm_stereo_sink_t* k) {
  if (!k) return SDRFM_EINVAL;
  STRY(hipSetDevice(k->hs.device), SDRFM_FAIL);                      // unlike the limiter and the mix bus: no wait for the stream before the state is cleared
  STRY(hipMemsetAsync(k->d_state, 0, sizeof(float) * 2 * (size_t)k->n_streams, k->hs.cur), SDRFM_FAIL);
  if (k->meter) STRY(hipMemsetAsync(k->d_meter, 0, sizeof(sdrfm_audio_meter) * (size_t)k->n_streams, k->hs.cur), SDRFM_FAIL);
  if (k->loud) {
    STRY(hipMemsetAsync(k->d_lstate, 0, sizeof(sdrfm_loudness_state) * (size_t)k->n_streams, k->hs.cur), SDRFM_FAIL);
    STRY(hipMemsetAsync(k->d_lring, 0, sizeof(sdrfm_loudness_block) * (size_t)k->n_streams * k->lcap, k->hs.cur), SDRFM_FAIL);
    k->lpos = k->lread = 0;
  }
  if (k->tpeak) {
    STRY(hipMemsetAsync(k->d_tprec, 0, sizeof(sdrfm_truepeak) * (size_t)k->n_streams, k->hs.cur), SDRFM_FAIL);
    STRY(hipMemsetAsync(k->d_tphist, 0, sizeof(unsigned) * (size_t)k->n_streams * (k->tp_nt - 1u), k->hs.cur), SDRFM_FAIL);
  }
  STRY(hipStreamSynchronize(k->hs.cur), SDRFM_FAIL);
  k->J = SDRFM_ACTL_J_MAX;                                      // the high-cut's settings stay, its ramps are complete
  return SDRFM_OK;
}

int sdrfm_pcm_stereo_sink_set_stream(sdrfm_pcm_stereo_sink_t* k, void* hip_stream) {
  return k ? host_stream_use(k->hs, hip_stream) : SDRFM_EINVAL;
}

int sdrfm_pcm_stereo_sink_synchronize(sdrfm_pcm_stereo_sink_t* k) { return k ? host_stream_wait(k->hs) : SDRFM_EINVAL; }

int sdrfm_pcm_stereo_sink_process_batch(sdrfm_pcm_stereo_sink_t* k, const float* left, const float* right, size_t audio_stride, uint32_t n,
                                        int16_t* pcm, size_t pcm_stride, uint32_t flags) {
  if (!k) return SDRFM_EINVAL;
  if (flags & ~(SDRFM_F_DEVICE_PTRS | SDRFM_PCM_F_EXACT)) return SDRFM_EINVAL;
  if (n == 0) return SDRFM_OK;
  if (!left || !right) return SDRFM_EINVAL;
  if (!pcm) return SDRFM_EINVAL;
  if (!pcm_rows_capacity(k->n_streams, audio_stride, n)) return SDRFM_ECAPACITY;
  const bool device_ptrs = (flags & SDRFM_F_DEVICE_PTRS) != 0;
  const int ok = stereo_sink_pcm_ok(k->n_streams, n, pcm, pcm_stride, device_ptrs);
  if (ok != SDRFM_OK) return ok;
  STRY(hipSetDevice(k->hs.device), SDRFM_FAIL);
  const bool exact = (flags & SDRFM_PCM_F_EXACT) != 0;
  if (device_ptrs) return stereo_sink_launch(k, left, right, audio_stride, n, pcm, pcm_stride, k->hs.cur, exact);
  // host buffers: stage, run, copy back, synchronous
  int rc = sdrfm_stereo_sink_reserve(k, n, nullptr, nullptr);
  if (rc != SDRFM_OK) return rc;
  const RowStage& st = k->stage;
  const size_t ns = k->n_streams, as = sizeof(float) * pcm_rows_pitch(ns, audio_stride, n);
  rc = rows_to_device(st, sizeof(float), 0, left, as, sizeof(float) * n, ns, k->hs.cur);
  if (rc != SDRFM_OK) return rc;
  rc = rows_to_device(st, sizeof(float), ns, right, as, sizeof(float) * n, ns, k->hs.cur);
  if (rc != SDRFM_OK) return rc;
  float* const d_left = static_cast<float*>(st.d_in);
  rc = stereo_sink_launch(k, d_left, d_left + ns * st.cap_in, st.cap_in, n, static_cast<int16_t*>(st.d_out), 2 * (size_t)st.cap_out, k->hs.cur, exact);
  if (rc != SDRFM_OK) return rc;
  const int cb = sdrfm_stereo_sink_copy_back(k, pcm, pcm_stride, n, k->hs.cur);
  if (cb != SDRFM_OK) return cb;
  STRY(hipStreamSynchronize(k->hs.cur), SDRFM_FAIL);
  return SDRFM_OK;
}

/* Host copy of the carried de-emphasis states of every stream: state_out[2s] = L, state_out[2s + 1] = R. */
int sdrfm_pcm_stereo_sink_get_state(sdrfm_pcm_stereo_sink_t* k, float* state_out) {
  if (!k || !state_out) return SDRFM_EINVAL;
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
  STRY(hipMemcpy(state_out, k->d_state, sizeof(float) * 2 * (size_t)k->n_streams, hipMemcpyDeviceToHost), SDRFM_FAIL);
  return SDRFM_OK;
}

// the streams' high-cut.  Every check comes before any device work; the call waits for the sink's stream before it replaces the
// records a launch may still read
int sdrfm_pcm_stereo_sink_set_hicut(sdrfm_pcm_stereo_sink_t* k, const uint16_t* hicut_q15, uint32_t slew_q15) {
  if (!k) return SDRFM_EINVAL;
  if (slew_q15 > SDRFM_ACTL_ONE) return SDRFM_EINVAL;
  if (!slew_q15 && hicut_q15) return SDRFM_EINVAL;
  const uint32_t ns = k->n_streams;
  for (uint32_t s = 0; hicut_q15 && s < ns; ++s)
    if (hicut_q15[s] < SDRFM_HICUT_MIN || hicut_q15[s] > SDRFM_ACTL_ONE) return SDRFM_EINVAL;
  if (slew_q15 && k->alpha * 0.03125f < 0.001f) return SDRFM_EINVAL;   // the smallest effective coefficient, alpha SDRFM_HICUT_MIN / 32768, stays >= 0.001
  if (hipSetDevice(k->hs.device) != hipSuccess) return SDRFM_FAIL;
  if (!slew_q15) {                                               // back to the plain kernels: h = 1, nothing to ramp
    if (hipStreamSynchronize(k->hs.cur) != hipSuccess) return SDRFM_FAIL;
    for (uint32_t s = 0; s < ns; ++s) k->hc_host[s] = HICUT_FLAT;
    k->hicut = false;
    k->slew = SDRFM_ACTL_ONE;
    k->J = SDRFM_ACTL_J_MAX;
    return SDRFM_OK;
  }
  if (!k->d_hc && hipMalloc(&k->d_hc, sizeof(HicutRec) * ns) != hipSuccess) return SDRFM_ENOMEM;
  if (hipStreamSynchronize(k->hs.cur) != hipSuccess) return SDRFM_FAIL;   // no launch still reads the records about to be replaced
  for (uint32_t s = 0; s < ns; ++s) {
    HicutRec& r = k->hc_host[s];
    r.h0 = (uint16_t)audio_ctl_ramp(r.h0, r.ht, k->slew, k->J);
    if (hicut_q15) r.ht = hicut_q15[s];
  }
  k->slew = slew_q15;
  k->J = 0;
  k->hicut = true;
  if (hipMemcpy(k->d_hc, k->hc_host, sizeof(HicutRec) * ns, hipMemcpyHostToDevice) != hipSuccess) return SDRFM_FAIL;
  return SDRFM_OK;
}

// the value the next sample starts from, and the target; any pointer may be NULL
int sdrfm_pcm_stereo_sink_get_hicut(const sdrfm_pcm_stereo_sink_t* k, uint16_t* hicut_q15, uint16_t* target_q15, uint32_t* slew_q15) {
  if (!k) return SDRFM_EINVAL;
  for (uint32_t s = 0; s < k->n_streams; ++s) {
    const HicutRec& r = k->hc_host[s];
    if (hicut_q15) hicut_q15[s] = (uint16_t)audio_ctl_ramp(r.h0, r.ht, k->slew, k->J);
    if (target_q15) target_q15[s] = r.ht;
  }
  if (slew_q15) *slew_q15 = k->hicut ? k->slew : 0u;
  return SDRFM_OK;
}

// the audio meter.  Every check comes before any device work; enable and disable wait for the sink's stream before they change
// what a launch may still use
int sdrfm_pcm_stereo_sink_meter_enable(sdrfm_pcm_stereo_sink_t* k, uint32_t quiet_lsb) {
  if (!k || quiet_lsb > SDRFM_AM_QUIET_MAX) return SDRFM_EINVAL;
  if (hipSetDevice(k->hs.device) != hipSuccess) return SDRFM_FAIL;
  const size_t bytes = sizeof(sdrfm_audio_meter) * (size_t)k->n_streams;
  if (!k->d_meter && hipMalloc(&k->d_meter, bytes) != hipSuccess) { k->d_meter = nullptr; return SDRFM_ENOMEM; }
  STRY(hipStreamSynchronize(k->hs.cur), SDRFM_FAIL);
  STRY(hipMemsetAsync(k->d_meter, 0, bytes, k->hs.cur), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->hs.cur), SDRFM_FAIL);
  k->quiet_lsb = quiet_lsb;
  k->meter = true;
  return SDRFM_OK;
}

int sdrfm_pcm_stereo_sink_meter_disable(sdrfm_pcm_stereo_sink_t* k) {
  if (!k) return SDRFM_EINVAL;
  if (!k->meter) return SDRFM_OK;
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
  k->meter = false;
  return SDRFM_OK;
}

int sdrfm_pcm_stereo_sink_meter_read(sdrfm_pcm_stereo_sink_t* k, sdrfm_audio_meter* out, uint32_t flags) {
  if (!k || !out || (flags & ~(SDRFM_F_DEVICE_PTRS | SDRFM_AMETER_F_RESET)) || (uintptr_t)out % 8 != 0 || !k->meter) return SDRFM_EINVAL;
  return records_read(k->hs, out, k->d_meter, sizeof(sdrfm_audio_meter) * (size_t)k->n_streams, nullptr, flags);
}

// the loudness meter.  Every check comes before any device work; enable and disable wait for the sink's stream before they
// change or free what a launch may still use
static void loudness_release(sdrfm_pcm_stereo_sink* k) {
  if (k->d_lstate) (void)hipFree(k->d_lstate);
  if (k->d_lring) (void)hipFree(k->d_lring);
  if (k->d_lpw) (void)hipFree(k->d_lpw);
  k->d_lstate = nullptr; k->d_lring = nullptr; k->d_lpw = nullptr;
  k->loud = false;
  k->lpos = k->lread = 0;
}

int sdrfm_pcm_stereo_sink_loudness_enable(sdrfm_pcm_stereo_sink_t* k, const sdrfm_loudness_coef* coef, uint32_t block_len, uint32_t cap_blocks) {
  if (!k) return SDRFM_EINVAL;
  sdrfm_loudness_coef c;
  if (coef) c = *coef;
  else (void)sdrfm_loudness_default_coef(&c);
  if (sdrfm_loudness_check_coef(&c) != SDRFM_OK) return SDRFM_EINVAL;
  if (block_len < SDRFM_LD_BLOCK_MIN || block_len > SDRFM_LD_BLOCK_MAX || cap_blocks < 1u || cap_blocks > SDRFM_LD_CAP_MAX) return SDRFM_EINVAL;
  // a stable set the scan is not good for is refused: the host routine serves it.  The library's own default is in the domain (the CPU tests hold
  // that) and is not probed again at every enable
  if (coef && sdrfm_loudness_check_domain(&c, nullptr, nullptr) != SDRFM_OK) return SDRFM_EINVAL;
  double pw[SDRFM_LD_TABLE];
  ld_matrix_powers(c.c, pw);                                    // on the host, here: the scan's A^(L 2^i) in its balanced coordinates
  if (hipSetDevice(k->hs.device) != hipSuccess) return SDRFM_FAIL;
  STRY(hipStreamSynchronize(k->hs.cur), SDRFM_FAIL);
  loudness_release(k);                                          // an enabled sink starts over
  const size_t sb = sizeof(sdrfm_loudness_state) * (size_t)k->n_streams, rb = sizeof(sdrfm_loudness_block) * (size_t)k->n_streams * cap_blocks;
  if (hipMalloc(&k->d_lstate, sb) != hipSuccess || hipMalloc(&k->d_lring, rb) != hipSuccess || hipMalloc(&k->d_lpw, sizeof(pw)) != hipSuccess) {
    loudness_release(k);
    return SDRFM_ENOMEM;
  }
  if (hipMemsetAsync(k->d_lstate, 0, sb, k->hs.cur) != hipSuccess || hipMemsetAsync(k->d_lring, 0, rb, k->hs.cur) != hipSuccess ||
      hipMemcpyAsync(k->d_lpw, pw, sizeof(pw), hipMemcpyHostToDevice, k->hs.cur) != hipSuccess || hipStreamSynchronize(k->hs.cur) != hipSuccess) {
    loudness_release(k);
    return SDRFM_FAIL;
  }
  k->lcoef = c; k->lblock = block_len; k->lcap = cap_blocks;
  k->loud = true;
  return SDRFM_OK;
}

int sdrfm_pcm_stereo_sink_loudness_disable(sdrfm_pcm_stereo_sink_t* k) {
  if (!k) return SDRFM_EINVAL;
  if (!k->loud) return SDRFM_OK;
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
  loudness_release(k);
  return SDRFM_OK;
}

int sdrfm_pcm_stereo_sink_loudness_read(sdrfm_pcm_stereo_sink_t* k, sdrfm_loudness_block* out, uint32_t out_cap_blocks, uint64_t* first_block,
                                        uint32_t* n_blocks, uint32_t flags) {
  if (!k || !first_block || !n_blocks || flags || !k->loud) return SDRFM_EINVAL;
  const uint64_t done = k->lpos / k->lblock, kept = ld_keep_from(done, k->lcap);
  const uint64_t first = k->lread > kept ? k->lread : kept;
  const uint32_t nb = (uint32_t)(done - first);                 // <= lcap
  if (nb > out_cap_blocks) return SDRFM_ECAPACITY;
  if (nb && !out) return SDRFM_EINVAL;
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
  if (nb) {                                                     // the ring wraps at most once inside [first, done)
    const uint32_t s0 = ld_ring_slot(first, k->lcap);
    const uint32_t a = nb < k->lcap - s0 ? nb : k->lcap - s0, b = nb - a;
    const size_t rec = sizeof(sdrfm_loudness_block);
    STRY(hipMemcpy2D(out, rec * nb, k->d_lring + s0, rec * k->lcap, rec * a, k->n_streams, hipMemcpyDeviceToHost), SDRFM_FAIL);
    if (b) STRY(hipMemcpy2D(out + a, rec * nb, k->d_lring, rec * k->lcap, rec * b, k->n_streams, hipMemcpyDeviceToHost), SDRFM_FAIL);
  }
  k->lread = done;
  *first_block = first;
  *n_blocks = nb;
  return SDRFM_OK;
}

int sdrfm_pcm_stereo_sink_loudness_get_state(sdrfm_pcm_stereo_sink_t* k, sdrfm_loudness_state* out) {
  if (!k || !out || !k->loud) return SDRFM_EINVAL;
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
  STRY(hipMemcpy(out, k->d_lstate, sizeof(sdrfm_loudness_state) * (size_t)k->n_streams, hipMemcpyDeviceToHost), SDRFM_FAIL);
  return SDRFM_OK;
}

// the true-peak meter.  Every check comes before any device work; enable and disable wait for the sink's stream before they
// change or free what a launch may still use
static void truepeak_release(sdrfm_pcm_stereo_sink* k) {
  if (k->d_tprec) (void)hipFree(k->d_tprec);
  if (k->d_tphist) (void)hipFree(k->d_tphist);
  if (k->d_tptab) (void)hipFree(k->d_tptab);
  k->d_tprec = nullptr; k->d_tphist = nullptr; k->d_tptab = nullptr;
  k->tpeak = false;
}

int sdrfm_pcm_stereo_sink_truepeak_enable(sdrfm_pcm_stereo_sink_t* k, const int16_t* coef, uint32_t n_phases, uint32_t n_taps, uint64_t limit) {
  if (!k || limit > SDRFM_TP_LIMIT_MAX) return SDRFM_EINVAL;
  int16_t dflt[48];
  if (!coef) {
    (void)sdrfm_truepeak_default_coef(dflt, &n_phases, &n_taps);
    coef = dflt;
  }
  if (sdrfm_truepeak_check_coef(coef, n_phases, n_taps) != SDRFM_OK) return SDRFM_EINVAL;
  uint32_t tab[SDRFM_TP_TABLE_DWORDS];
  tp_pack_table(coef, n_phases, n_taps, tab);
  if (hipSetDevice(k->hs.device) != hipSuccess) return SDRFM_FAIL;
  STRY(hipStreamSynchronize(k->hs.cur), SDRFM_FAIL);
  truepeak_release(k);                                          // an enabled sink starts over
  const size_t rb = sizeof(sdrfm_truepeak) * (size_t)k->n_streams, hb = sizeof(unsigned) * (size_t)k->n_streams * (n_taps - 1u);
  const size_t tb = sizeof(uint32_t) * n_phases * (n_taps / 2u);
  if (hipMalloc(&k->d_tprec, rb) != hipSuccess || hipMalloc(&k->d_tphist, hb) != hipSuccess || hipMalloc(&k->d_tptab, tb) != hipSuccess) {
    truepeak_release(k);
    return SDRFM_ENOMEM;
  }
  if (hipMemsetAsync(k->d_tprec, 0, rb, k->hs.cur) != hipSuccess || hipMemsetAsync(k->d_tphist, 0, hb, k->hs.cur) != hipSuccess ||
      hipMemcpyAsync(k->d_tptab, tab, tb, hipMemcpyHostToDevice, k->hs.cur) != hipSuccess || hipStreamSynchronize(k->hs.cur) != hipSuccess) {
    truepeak_release(k);
    return SDRFM_FAIL;
  }
  k->tp_limit = limit; k->tp_P = n_phases; k->tp_nt = n_taps;
  k->tpeak = true;
  return SDRFM_OK;
}

int sdrfm_pcm_stereo_sink_truepeak_disable(sdrfm_pcm_stereo_sink_t* k) {
  if (!k) return SDRFM_EINVAL;
  if (!k->tpeak) return SDRFM_OK;
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
  truepeak_release(k);
  return SDRFM_OK;
}

int sdrfm_pcm_stereo_sink_truepeak_read(sdrfm_pcm_stereo_sink_t* k, sdrfm_truepeak* out, uint32_t flags) {
  if (!k || !out || (flags & ~(SDRFM_F_DEVICE_PTRS | SDRFM_AMETER_F_RESET)) || (uintptr_t)out % 8 != 0 || !k->tpeak) return SDRFM_EINVAL;
  // a reset takes the records only: the history stays and the stream continues
  return records_read(k->hs, out, k->d_tprec, sizeof(sdrfm_truepeak) * (size_t)k->n_streams, nullptr, flags);
}

}  // extern "C"
