/*
 * sdrfm_sink.hip — device-side audio sink for the batched path: demodulated audio (f32, 48 kHz) ->
 * FM de-emphasis -> int16 stereo-interleaved PCM in the layout the reference board's sink consumes,
 * BSP_AUDIO_OUT_Play(uint16_t* pBuffer, uint32_t Size) (Utilities/STM32746G-Discovery/stm32746g_discovery_audio.c:224;
 * L and R carry the same mono programme).  Same arithmetic, operation for operation, as the host routine
 * sdrfm_pcm_deemph_s16 (csrc/pcm_sink.c), so the two are interchangeable bit for bit:
 *
 *   y[n]   = fmaf(alpha, x[n] - y[n-1], y[n-1])        one rounded difference, one fused multiply-add
 *   pcm[n] = (int16) rint(clamp(y[n] * gain, -32768, 32767))      round-half-even, L = R
 *
 * Both forms of the recursion are written once, for any number of channels, in sdrfm_sink_kernels.h; the kernels here instantiate them for ONE chain per
 * stream around the way this sink keeps its state (the tagged words of sdrfm_sink_chain.h), and the stereo sink's (sdrfm_sink_stereo.hip) for two.
 *
 * Parallelisation: the recursion rounds at every step, so a scan (which re-associates) cannot reproduce it bit for bit;
 * the chain of one stream is therefore walked by ONE lane, 64 streams per wave, and what IS parallel — moving the data —
 * is kept coalesced by transposing 64 x 64 tiles through LDS (sink_exact_tiles).
 * The chain is latency-bound (one lane per stream, and every 64 samples a tile of 64 dependent row loads): measured 1.35 ms per 256 x 4800
 * launch (profiles/r06_sink.txt; rounds 2 - 5 quoted an estimate of 25 us that had never been timed) — sixty demodulator calls.  It is kept
 * as the EXACT form (SDRFM_PCM_F_EXACT): bit-identical to the host routine.
 *
 * The default since round 6 is a BLOCKED SCAN (k_pcm_sink_scan): the recursion is linear — y[n] = (1 - alpha) y[n-1] + alpha x[n] —,
 * so a stream's call is cut into segments of 256 chunks of 19 samples, one lane per chunk, one workgroup of 256 lanes per stream, and walked in the three
 * phases of sink_scan_segments: every chunk's own contribution from state 0, the carries between the chunks, every chunk again from its true carry-in with
 * exactly the exact form's operations.  (The carries between the four waves go through four words of LDS and one barrier; the first version's Hillis-Steele
 * scan over 256 lanes in LDS took sixteen: 7.4 -> 7.0 us per launch.)
 * What differs from the exact chain is therefore only the carry-in of a chunk (re-associated: ~1e-7 relative), and that difference decays with
 * (1 - alpha)^k inside the chunk: the PCM is within 1 LSB of the exact form's (equal but where y * gain sits within 1e-3 of a rounding boundary),
 * the carried state within 1e-6 relative (2.5e-7 at 75 us, tests/test_pcm_sink_gpu.py; 8e-7 at alpha = 0.001, where a carry-in hardly decays inside its chunk:
 * tests/test_pcm_sink_params_gpu.py).  The audio row goes through LDS once (coalesced loads, chunk stride odd: conflict-free),
 * the PCM row back the same way; the chunk sits in registers for both walks.  7.0 us per 256 x 4800 launch against the exact form's 1.35 ms
 * (profiles/r06_sink.txt).
 */
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/sdrfm.h"
#include "sdrfm_sink_chain.h"
#include "sdrfm_sink_kernels.h"

namespace {

struct SinkParams {
  const float* audio;
  size_t audio_stride;   // floats
  int16_t* pcm;
  size_t pcm_stride;     // int16 elements per stream (>= 2 * n)
  const unsigned long long* sg_in;   // [n_streams] {tag << 32 | bits of y[n-1]}: the slot of the tag before this call (sdrfm_sink_chain.h) ...
  unsigned long long* sg_out;        // ... and of the tag behind it
  uint32_t gen_next;     // the tag behind this call
  uint32_t n_streams, n;
  float alpha, gain;
};

__global__ void __launch_bounds__(64) k_pcm_sink(SinkParams p) {
  __shared__ unsigned tile[1][64 * 65];
  const uint32_t lane = threadIdx.x;
  const uint32_t s0 = blockIdx.x * 64;
  const uint32_t rows = (p.n_streams - s0 < 64u) ? p.n_streams - s0 : 64u;
  const uint32_t mine = s0 + lane;
  float y[1] = {(lane < rows) ? __uint_as_float((unsigned)p.sg_in[mine]) : 0.0f};
  const float* const in[1] = {p.audio};
  sink_exact_tiles<1>(tile, in, p.audio_stride, p.pcm, p.pcm_stride, s0, rows, p.n, p.alpha, p.gain, y);
  if (lane < rows) p.sg_out[mine] = ((unsigned long long)p.gen_next << 32) | __float_as_uint(y[0]);
}

// ---- the blocked scan (the default): one workgroup of 256 lanes per stream around sink_scan_segments<1> (sdrfm_sink_kernels.h) -----------------------------
// (A variant with ONE WAVE per stream, 75-sample chunks in registers and no LDS at all was built to slip in beside the demodulator's waves, which hold all but
// 0.9 KiB of a CU's LDS: 10.5 us alone against 7.4 us for this one, and no faster in the consumer loop — profiles/r06_sink.txt.  Not kept.)
// LIST: the workgroup's stream is list[blockIdx.x], and the call is PART of a sink call whose other streams the chain inside a demodulator launch serves
// (sdrfm_sink_chain.h): the state is taken by that protocol — the tagged word of slot sg_in, waited for on the device (bounded) — and published the same way.
template <bool LIST>
__global__ void __launch_bounds__(256) k_pcm_sink_scan(SinkParams p, float pc, const uint32_t* list, uint32_t* err) {
  __shared__ float x[1][SINK_SEG];
  __shared__ float sc[1][4];
  const uint32_t s = LIST ? list[blockIdx.x] : blockIdx.x, t = threadIdx.x;
  const float* const row[1] = {p.audio + (size_t)s * p.audio_stride};
  float y0[1];
  if constexpr (LIST) {
    if (t == 0) {
      unsigned long long pv = 0ull, zero = 0ull;
      asm volatile("" : "+v"(zero));                             // (an opaque 0: a read-modify-write the compiler cannot turn back into a load, which may hit a stale line)
      int it = 0;
      for (;; ++it) {
        pv = __hip_atomic_fetch_add(const_cast<unsigned long long*>(p.sg_in) + s, zero, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((uint32_t)(pv >> 32) == p.gen_next - 1u || it == (1 << 19)) break;
        __builtin_amdgcn_s_sleep(16);
      }
      if (it == (1 << 19)) { pv = 0ull; __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
      sc[0][0] = __uint_as_float((unsigned)pv);
    }
    __syncthreads();
    y0[0] = sc[0][0];
    __syncthreads();
  } else {
    y0[0] = __uint_as_float((unsigned)p.sg_in[s]);
  }
  sink_scan_segments<1>(x, sc, row, reinterpret_cast<unsigned*>(p.pcm + (size_t)s * p.pcm_stride), p.n, p.alpha, p.gain, pc, y0);
  if (t == 0) {
    const unsigned long long w = ((unsigned long long)p.gen_next << 32) | __float_as_uint(y0[0]);
    if constexpr (LIST) __hip_atomic_store(p.sg_out + s, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else p.sg_out[s] = w;
  }
}

}  // namespace

struct sdrfm_pcm_sink {
  uint32_t n_streams;
  float alpha, gain;
  HostStream hs;
  unsigned long long* d_sg;   // [SDRFM_CHAIN_SG_SLOTS][n_streams] {tag << 32 | bits of y[n-1]}, tag t in slot t % 8 (sdrfm_sink_chain.h)
  float* d_dpow;       // [SDRFM_CHAIN_FIX] (1 - alpha)^(k + 1)
  uint32_t calls;      // calls issued so far (mod 2^32): the tag d_sg holds when every one of them is through
  RowStage stage;      // staging for host-pointer calls: floats in, (L, R) pairs out, straight into the caller's rows
};

static void sink_free(sdrfm_pcm_sink* k) {
  if (!k) return;
  (void)hipSetDevice(k->hs.device);
  if (k->d_sg) (void)hipFree(k->d_sg);
  if (k->d_dpow) (void)hipFree(k->d_dpow);
  row_stage_free(k->stage);
  host_stream_close(k->hs);
  delete k;
}

// ---- the sink inside a demodulator launch (sdrfm_sink_chain.h) ---------------------------------------------------------------------------------------
extern "C" int sdrfm_sink_chain_tables(float alpha, float* pc, float* w, float* dinv) {
  const double d = 1.0 - (double)alpha;
  *pc = (float)pow(d, (double)SDRFM_CHAIN_CH);
  for (uint32_t q = 0; q < SDRFM_CHAIN_CH; ++q) w[q] = (float)((double)alpha * pow(d, (double)(SDRFM_CHAIN_CH - 1u - q)));
  for (uint32_t q = 0; q < SDRFM_CHAIN_CH; ++q) dinv[q] = (float)pow(d, -(double)q);
  // (pc a normal float: w[0] = alpha pc / d is normal and dinv[7] = d / pc finite with it, and a product that underflows in the scan is off by 2^-149 dinv[7] < 1e-11)
  return (alpha >= SDRFM_CHAIN_MIN_ALPHA && *pc >= FLT_MIN) ? 2 : 1;
}

int sdrfm_sink_chain_params(sdrfm_pcm_sink* k, int device, uint32_t n_streams, SdrfmSinkChain* out) {
  if (!k || !out || k->hs.device != device || k->n_streams != n_streams) return 0;
  out->pcm = nullptr; out->pcm_stride = 0; out->runstate = nullptr; out->run_call = 0;
  out->sg = k->d_sg; out->n_streams = n_streams; out->dpow = k->d_dpow; out->err = reinterpret_cast<uint32_t*>(k->d_dpow + SDRFM_CHAIN_FIX);
  out->call = k->calls;
  out->alpha = k->alpha; out->gain = k->gain;
  return sdrfm_sink_chain_tables(k->alpha, &out->pc, out->w, out->dinv);
}

void sdrfm_sink_chain_issued(sdrfm_pcm_sink* k) { ++k->calls; }

// the parameters of the sink's call number `call`: it takes the states of tag `call` and leaves those of tag `call + 1` (sdrfm_sink_chain.h)
static SinkParams sink_params(const sdrfm_pcm_sink* k, uint32_t call, const float* audio, size_t audio_stride, uint32_t n, int16_t* pcm, size_t pcm_stride) {
  SinkParams p;
  p.sg_in = k->d_sg + (size_t)(call % SDRFM_CHAIN_SG_SLOTS) * k->n_streams; p.sg_out = k->d_sg + (size_t)((call + 1u) % SDRFM_CHAIN_SG_SLOTS) * k->n_streams;
  p.n_streams = k->n_streams; p.n = n; p.alpha = k->alpha; p.gain = k->gain;
  p.gen_next = call + 1u;
  p.audio = audio; p.audio_stride = audio_stride; p.pcm = pcm; p.pcm_stride = pcm_stride;
  return p;
}

// one whole call of the sink over device buffers, in either form, on `stream`
static int sink_launch(sdrfm_pcm_sink* k, const float* audio, size_t audio_stride, uint32_t n, int16_t* pcm, size_t pcm_stride, hipStream_t stream, bool exact) {
  const SinkParams p = sink_params(k, k->calls, audio, audio_stride, n, pcm, pcm_stride);
  if (exact) hipLaunchKernelGGL(k_pcm_sink, dim3((k->n_streams + 63) / 64), dim3(64), 0, stream, p);
  else hipLaunchKernelGGL(k_pcm_sink_scan<false>, dim3(k->n_streams), dim3(SINK_NT), 0, stream, p, sink_carry_factor(k->alpha), nullptr, nullptr);
  STRY(hipGetLastError(), SDRFM_FAIL);
  ++k->calls;
  return SDRFM_OK;
}

int sdrfm_sink_launch_on(sdrfm_pcm_sink* k, const float* audio, size_t audio_stride, uint32_t n, int16_t* pcm, size_t pcm_stride, hipStream_t stream) {
  if (!k) return SDRFM_EINVAL;
  if (n == 0) return SDRFM_OK;
  return sink_launch(k, audio, audio_stride, n, pcm, pcm_stride, stream, false);
}

int sdrfm_sink_launch_list_on(sdrfm_pcm_sink* k, const SdrfmSinkChain& c, const uint32_t* list_dev, uint32_t n_list, const float* audio, size_t audio_stride, uint32_t n,
                              int16_t* pcm, size_t pcm_stride, hipStream_t stream, hipEvent_t done) {
  if (!k || !list_dev) return SDRFM_EINVAL;
  if (n == 0 || n_list == 0) return SDRFM_OK;
  const SinkParams p = sink_params(k, c.call, audio, audio_stride, n, pcm, pcm_stride);
  hipExtLaunchKernelGGL(k_pcm_sink_scan<true>, dim3(n_list), dim3(SINK_NT), 0, stream, nullptr, done, 0, p, sink_carry_factor(k->alpha), list_dev, c.err);
  STRY(hipGetLastError(), SDRFM_FAIL);
  return SDRFM_OK;
}

extern "C" {

int sdrfm_pcm_sink_create(uint32_t n_streams, float alpha, float gain, int32_t device, sdrfm_pcm_sink_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!n_streams || !(alpha > 0.0f) || alpha > 1.0f || !(gain == gain)) return SDRFM_EINVAL;
  if (const int rc = host_open_device(device); rc != SDRFM_OK) return rc;
  sdrfm_pcm_sink* k = new (std::nothrow) sdrfm_pcm_sink();
  if (!k) return SDRFM_ENOMEM;
  memset(static_cast<void*>(k), 0, sizeof(*k));
  k->n_streams = n_streams; k->alpha = alpha; k->gain = gain; k->hs.device = device;
  if (host_stream_open(k->hs, device) != SDRFM_OK ||
      hipMalloc(&k->d_sg, sizeof(unsigned long long) * SDRFM_CHAIN_SG_SLOTS * n_streams) != hipSuccess ||
      hipMalloc(&k->d_dpow, sizeof(float) * (SDRFM_CHAIN_FIX + 1)) != hipSuccess) { sink_free(k); return SDRFM_ENOMEM; }   // (+ the error word)
  {
    float dp[SDRFM_CHAIN_FIX + 1];
    for (uint32_t i = 0; i < SDRFM_CHAIN_FIX; ++i) dp[i] = (float)pow(1.0 - (double)alpha, (double)(i + 1));
    dp[SDRFM_CHAIN_FIX] = 0.0f;
    if (hipMemcpy(k->d_dpow, dp, sizeof(dp), hipMemcpyHostToDevice) != hipSuccess) { sink_free(k); return SDRFM_FAIL; }
  }
  const int rc = sdrfm_pcm_sink_reset(k);
  if (rc != SDRFM_OK) { sink_free(k); return rc; }
  *out = k;
  return SDRFM_OK;
}

void sdrfm_pcm_sink_destroy(sdrfm_pcm_sink_t* k) {
  if (!k) return;
  (void)host_stream_wait(k->hs);
  sink_free(k);
}

int sdrfm_pcm_sink_reset(sdrfm_pcm_sink_t* k) {
  if (!k) return SDRFM_EINVAL;
  STRY(hipSetDevice(k->hs.device), SDRFM_FAIL);                   // unlike the limiter and the mix bus: no wait for the stream before the state is cleared
  STRY(hipMemsetAsync(k->d_sg, 0, sizeof(unsigned long long) * SDRFM_CHAIN_SG_SLOTS * k->n_streams, k->hs.cur), SDRFM_FAIL);
  STRY(hipMemsetAsync(k->d_dpow + SDRFM_CHAIN_FIX, 0, sizeof(uint32_t), k->hs.cur), SDRFM_FAIL);   // (the chain's error word)
  STRY(hipStreamSynchronize(k->hs.cur), SDRFM_FAIL);
  k->calls = 0;
  return SDRFM_OK;
}

int sdrfm_pcm_sink_set_stream(sdrfm_pcm_sink_t* k, void* hip_stream) {
  return k ? host_stream_use(k->hs, hip_stream) : SDRFM_EINVAL;
}

// a run of a demodulator launch gave up waiting for its predecessor's word (sdrfm_sink_chain.h): the PCM since then is not to be trusted
static int sink_chain_error(sdrfm_pcm_sink* k) {
  uint32_t e = 0;
  if (hipMemcpy(&e, k->d_dpow + SDRFM_CHAIN_FIX, sizeof(e), hipMemcpyDeviceToHost) != hipSuccess) return SDRFM_FAIL;
  if (e) fprintf(stderr, "[sdrfm] PCM sink: a run of a demodulator launch waited in vain for its predecessor's state (csrc/sdrfm_sink_chain.h)\n");
  return e ? SDRFM_FAIL : SDRFM_OK;
}

int sdrfm_pcm_sink_synchronize(sdrfm_pcm_sink_t* k) {
  if (!k) return SDRFM_EINVAL;
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
  return sink_chain_error(k);
}

int sdrfm_pcm_sink_process_batch(sdrfm_pcm_sink_t* k, const float* audio, size_t audio_stride, uint32_t n, int16_t* pcm,
                                 size_t pcm_stride, uint32_t flags) {
  if (!k) return SDRFM_EINVAL;
  if (flags & ~(SDRFM_F_DEVICE_PTRS | SDRFM_PCM_F_EXACT)) return SDRFM_EINVAL;
  if (n == 0) return SDRFM_OK;
  if (!audio || !pcm) return SDRFM_EINVAL;
  const uint32_t ns = k->n_streams;
  // unlike the three newer handles: the capacity before the odd stride
  if (!pcm_rows_capacity(ns, audio_stride, n) || !pcm_rows_capacity(ns, pcm_stride, 2 * (size_t)n)) return SDRFM_ECAPACITY;
  if (pcm_stride & 1u) return SDRFM_EINVAL;                          // rows are written as (L,R) dwords
  STRY(hipSetDevice(k->hs.device), SDRFM_FAIL);
  const bool exact = (flags & SDRFM_PCM_F_EXACT) != 0;
  if (flags & SDRFM_F_DEVICE_PTRS) {
    if ((uintptr_t)pcm % 4 != 0) return SDRFM_EINVAL;
    return sink_launch(k, audio, audio_stride, n, pcm, pcm_stride, k->hs.cur, exact);
  }
  // host buffers: stage, run, copy back, synchronous
  RowStage& st = k->stage;
  int rc = row_stage_reserve(st, RowShape{1024u, sizeof(float), ns, PCM_PAIR_BYTES, ns, false}, n, n);
  if (rc != SDRFM_OK) return rc;
  rc = rows_to_device(st, sizeof(float), 0, audio, sizeof(float) * pcm_rows_pitch(ns, audio_stride, n), sizeof(float) * n, ns, k->hs.cur);
  if (rc != SDRFM_OK) return rc;
  rc = sink_launch(k, static_cast<float*>(st.d_in), st.cap_in, n, static_cast<int16_t*>(st.d_out), 2 * (size_t)st.cap_out, k->hs.cur, exact);
  if (rc != SDRFM_OK) return rc;
  return rows_to_host(st, PCM_PAIR_BYTES, pcm, sizeof(int16_t) * pcm_rows_pitch(ns, pcm_stride, 2 * (size_t)n), n, nullptr, ns, k->hs.cur);
}

/* Host copy of the carried de-emphasis state y[n-1] of every stream (tests, and switching between this sink and the host one). */
int sdrfm_pcm_sink_get_state(sdrfm_pcm_sink_t* k, float* state_out) {
  if (!k || !state_out) return SDRFM_EINVAL;
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
  unsigned long long* tmp = new (std::nothrow) unsigned long long[k->n_streams];
  if (!tmp) return SDRFM_ENOMEM;
  const hipError_t e = hipMemcpy(tmp, k->d_sg + (size_t)(k->calls % SDRFM_CHAIN_SG_SLOTS) * k->n_streams, sizeof(unsigned long long) * k->n_streams, hipMemcpyDeviceToHost);
  for (uint32_t i = 0; e == hipSuccess && i < k->n_streams; ++i) { const unsigned b = (unsigned)tmp[i]; memcpy(state_out + i, &b, sizeof(float)); }
  delete[] tmp;
  return e == hipSuccess ? sink_chain_error(k) : SDRFM_FAIL;
}

}  // extern "C"
