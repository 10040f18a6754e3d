/*
 * sdrfm_pcm_limit.hip — the per-stream look-ahead PCM limiter behind the sdrfm_pcm_limit_* C-ABI (include/sdrfm.h): the int16
 * stereo rows the PCM sinks leave, under a ramped make-up gain and a look-ahead peak limiter, on the device.  The arithmetic is the host
 * routine sdrfm_pcm_limit_s16's (csrc/limit.c) and all-integer, so the outputs, the state and the records are that routine's bit for bit.
 *
 *   k_pcm_limit      one workgroup of 1024 lanes per stream, grid (streams); the row in tiles of SDRFM_PCM_LIMIT_TILE pairs staged in LDS behind
 *                    their lead-in.  The body, the arithmetic and the geometry are in csrc/sdrfm_limit.h.
 *   k_pcm_limit_tp   the same body's true-peak form for a handle made by sdrfm_pcm_tplimit_create: the detector sees the P
 *                    phases of the oversampled waveform, as 64-bit multiply-adds over the x' planes.
 *
 * State: 4 D int32 per stream (4 D + NT in the true-peak form) on the device, one set.  The kernel reads a stream's state into registers before its first barrier and writes it
 * behind its last, and calls are ordered by the HIP stream they are enqueued on.  The gain ramp is a closed form of (gain0, gain_t, slew, J):
 * the handle keeps J on the host and passes it by value.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/sdrfm.h"
#include "sdrfm_host.h"
#include "sdrfm_limit.h"

namespace {

__global__ void __launch_bounds__(SDRFM_LIMIT_NT) k_pcm_limit(LimitParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned limit_lds[];
  limit_stream<false>(limit_lds, p);
}

__global__ void __launch_bounds__(SDRFM_LIMIT_NT) k_pcm_limit_tp(LimitTpParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned limit_lds[];
  limit_stream<true>(limit_lds, p);
}

}  // namespace

struct sdrfm_pcm_limit {
  uint32_t n_streams, lw, slew, J;
  uint32_t P, nt, words;           // the detector's table (0, 0 for the sample form) and the state's words per stream
  unsigned* d_table;               // the packed table, true-peak form only
  HostStream hs;
  sdrfm_pcm_limit_params* d_par;   // [n_streams]
  int32_t* d_state;                // [n_streams][4 D]
  sdrfm_pcm_limit_rec* d_rec;      // [n_streams]
  sdrfm_pcm_limit_params* par;     // host: the parameters as the device holds them
  int32_t* state0;                 // host: the state after reset, and the records' identity
  sdrfm_pcm_limit_rec* rec0;
  RowStage stage;                  // staging for host-pointer calls: pairs, limited in place
};

static void limit_free(sdrfm_pcm_limit* k) {
  if (!k) return;
  (void)hipSetDevice(k->hs.device);
  if (k->d_par) (void)hipFree(k->d_par);
  if (k->d_state) (void)hipFree(k->d_state);
  if (k->d_rec) (void)hipFree(k->d_rec);
  if (k->d_table) (void)hipFree(k->d_table);
  row_stage_free(k->stage);
  free(k->par);
  free(k->state0);
  free(k->rec0);
  host_stream_close(k->hs);
  delete k;
}

// one call over device buffers on the handle's stream; J moves with it
static int limit_launch(sdrfm_pcm_limit* k, const int16_t* in, size_t in_stride, uint32_t n, int16_t* out, size_t out_stride) {
  LimitTpParams p;
  p.in = in; p.in_stride = in_stride; p.out = out; p.out_stride = out_stride;
  p.par = k->d_par; p.state = k->d_state; p.rec = k->d_rec;
  p.n = n; p.lw = k->lw; p.slew = k->slew; p.J = k->J;
  p.table = k->d_table; p.nt = k->nt; p.P = k->P;
  if (k->nt) hipLaunchKernelGGL(k_pcm_limit_tp, dim3(k->n_streams), dim3(SDRFM_LIMIT_NT), limit_tp_lds_bytes(), k->hs.cur, p);
  else hipLaunchKernelGGL(k_pcm_limit, dim3(k->n_streams), dim3(SDRFM_LIMIT_NT), limit_lds_bytes(), k->hs.cur, static_cast<const LimitParams&>(p));
  STRY(hipGetLastError(), SDRFM_FAIL);
  k->J = audio_ctl_advance(k->J, n);
  return SDRFM_OK;
}

// the parameters to the device, behind whatever launch may still read them
static int limit_upload(sdrfm_pcm_limit* k) {
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
  STRY(hipMemcpy(k->d_par, k->par, sizeof(sdrfm_pcm_limit_params) * (size_t)k->n_streams, hipMemcpyHostToDevice), SDRFM_FAIL);
  return SDRFM_OK;
}

// the two constructors behind their refusals: coef NULL is the sample form, else a table sdrfm_truepeak_check_coef has taken
static int limit_create(const sdrfm_pcm_limit_config* cfg, const int16_t* coef, uint32_t n_phases, uint32_t n_taps, sdrfm_pcm_limit_t** out) {
  if (const int rc = host_open_device(cfg->device); rc != SDRFM_OK) return rc;
  sdrfm_pcm_limit* k = new (std::nothrow) sdrfm_pcm_limit();
  if (!k) return SDRFM_ENOMEM;
  memset(static_cast<void*>(k), 0, sizeof(*k));
  const uint32_t ns = cfg->n_streams, words = coef ? limit_tp_state_words(cfg->log2_window, n_taps) : limit_state_words(cfg->log2_window);
  if (coef) { k->P = n_phases; k->nt = n_taps; }
  k->words = words;
  k->n_streams = ns; k->lw = cfg->log2_window; k->slew = cfg->gain_slew; k->hs.device = cfg->device;
  k->par = (sdrfm_pcm_limit_params*)malloc(sizeof(sdrfm_pcm_limit_params) * ns);
  k->state0 = (int32_t*)malloc(sizeof(int32_t) * (size_t)words * ns);
  k->rec0 = (sdrfm_pcm_limit_rec*)malloc(sizeof(sdrfm_pcm_limit_rec) * ns);
  if (!k->par || !k->state0 || !k->rec0) { limit_free(k); return SDRFM_ENOMEM; }
  for (uint32_t s = 0; s < ns; ++s) {
    k->par[s].ceiling = SDRFM_LIMIT_CEILING_DEFAULT; k->par[s].release = SDRFM_LIMIT_RELEASE_DEFAULT;
    k->par[s].gain0 = k->par[s].gain_t = SDRFM_LIMIT_GAIN_UNITY;
    if (coef) (void)sdrfm_pcm_tplimit_state_init(k->lw, n_taps, k->state0 + (size_t)s * words);
    else (void)sdrfm_pcm_limit_state_init(k->lw, k->state0 + (size_t)s * words);
    k->rec0[s].n = 0; k->rec0[s].limited = 0; k->rec0[s].min_gain = SDRFM_LIMIT_ONE; k->rec0[s].at = 0;
  }
  const bool ok = host_stream_open(k->hs, cfg->device) == SDRFM_OK &&
                  hipMalloc(&k->d_par, sizeof(sdrfm_pcm_limit_params) * ns) == hipSuccess &&
                  hipMalloc(&k->d_state, sizeof(int32_t) * (size_t)words * ns) == hipSuccess &&
                  hipMalloc(&k->d_rec, sizeof(sdrfm_pcm_limit_rec) * ns) == hipSuccess;
  if (!ok) { limit_free(k); return SDRFM_ENOMEM; }
  if (coef) {
    unsigned packed[SDRFM_TP_TABLE_DWORDS];
    tp_pack_table(coef, n_phases, n_taps, packed);
    const size_t bytes = sizeof(unsigned) * n_phases * (n_taps / 2u);
    if (hipMalloc(&k->d_table, bytes) != hipSuccess) { limit_free(k); return SDRFM_ENOMEM; }
    if (hipMemcpy(k->d_table, packed, bytes, hipMemcpyHostToDevice) != hipSuccess) { limit_free(k); return SDRFM_FAIL; }
  }
  const void* const kernel = coef ? reinterpret_cast<const void*>(k_pcm_limit_tp) : reinterpret_cast<const void*>(k_pcm_limit);
  if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(coef ? limit_tp_lds_bytes() : limit_lds_bytes())) != hipSuccess ||
      hipMemcpy(k->d_par, k->par, sizeof(sdrfm_pcm_limit_params) * ns, hipMemcpyHostToDevice) != hipSuccess) {
    limit_free(k);
    return SDRFM_FAIL;
  }
  const int rc = sdrfm_pcm_limit_reset(k);
  if (rc != SDRFM_OK) { limit_free(k); return rc; }
  *out = k;
  return SDRFM_OK;
}

extern "C" {

int sdrfm_pcm_limit_create(const sdrfm_pcm_limit_config* cfg, sdrfm_pcm_limit_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!cfg || !cfg->n_streams || cfg->flags || !limit_shape_ok(cfg->log2_window, cfg->gain_slew)) return SDRFM_EINVAL;
  return limit_create(cfg, nullptr, 0, 0, out);
}

int sdrfm_pcm_tplimit_create(const sdrfm_pcm_limit_config* cfg, const int16_t* coef, uint32_t n_phases, uint32_t n_taps, sdrfm_pcm_limit_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!cfg || !cfg->n_streams || cfg->flags || !limit_shape_ok(cfg->log2_window, cfg->gain_slew)) return SDRFM_EINVAL;
  int16_t def[48];
  if (!coef) { (void)sdrfm_truepeak_default_coef(def, &n_phases, &n_taps); coef = def; }
  if (sdrfm_truepeak_check_coef(coef, n_phases, n_taps) != SDRFM_OK || !limit_tp_window_ok(cfg->log2_window, n_taps)) return SDRFM_EINVAL;
  return limit_create(cfg, coef, n_phases, n_taps, out);
}

int sdrfm_pcm_tplimit_get_detector(const sdrfm_pcm_limit_t* k, uint32_t* n_phases, uint32_t* n_taps, uint32_t* latency) {
  if (!k) return SDRFM_EINVAL;
  if (n_phases) *n_phases = k->P;
  if (n_taps) *n_taps = k->nt;
  if (latency) *latency = (1u << k->lw) - 1u + k->nt / 2u;
  return SDRFM_OK;
}

void sdrfm_pcm_limit_destroy(sdrfm_pcm_limit_t* k) {
  if (!k) return;
  (void)host_stream_wait(k->hs);
  limit_free(k);
}

int sdrfm_pcm_limit_reset(sdrfm_pcm_limit_t* k) {
  if (!k) return SDRFM_EINVAL;
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
  STRY(hipMemcpy(k->d_state, k->state0, sizeof(int32_t) * (size_t)k->words * k->n_streams, hipMemcpyHostToDevice), SDRFM_FAIL);
  STRY(hipMemcpy(k->d_rec, k->rec0, sizeof(sdrfm_pcm_limit_rec) * (size_t)k->n_streams, hipMemcpyHostToDevice), SDRFM_FAIL);
  return SDRFM_OK;
}

// every check comes before any device work; the calls wait for the handle's stream before they replace what a launch may still read
int sdrfm_pcm_limit_set_params(sdrfm_pcm_limit_t* k, const uint32_t* ceiling, const uint32_t* release) {
  if (!k || (!ceiling && !release)) return SDRFM_EINVAL;
  for (uint32_t s = 0; s < k->n_streams; ++s) {
    if (ceiling && (ceiling[s] < 1u || ceiling[s] > SDRFM_LIMIT_CEILING_MAX)) return SDRFM_EINVAL;
    if (release && (release[s] < 1u || release[s] > SDRFM_LIMIT_R_ONE)) return SDRFM_EINVAL;
  }
  for (uint32_t s = 0; s < k->n_streams; ++s) {
    if (ceiling) k->par[s].ceiling = ceiling[s];
    if (release) k->par[s].release = release[s];
  }
  return limit_upload(k);
}

int sdrfm_pcm_limit_set_gain(sdrfm_pcm_limit_t* k, const uint32_t* gain_q12, uint32_t jump) {
  if (!k || !gain_q12 || jump > 1u) return SDRFM_EINVAL;
  for (uint32_t s = 0; s < k->n_streams; ++s)
    if (gain_q12[s] > SDRFM_LIMIT_GAIN_MAX) return SDRFM_EINVAL;
  for (uint32_t s = 0; s < k->n_streams; ++s) {                   // the ramps restart where they have got to
    k->par[s].gain0 = jump ? gain_q12[s] : audio_ctl_ramp(k->par[s].gain0, k->par[s].gain_t, k->slew, k->J);
    k->par[s].gain_t = gain_q12[s];
  }
  k->J = 0;
  return limit_upload(k);
}

int sdrfm_pcm_limit_get_params(const sdrfm_pcm_limit_t* k, sdrfm_pcm_limit_params* out, uint32_t* J) {
  if (!k) return SDRFM_EINVAL;
  if (out) memcpy(out, k->par, sizeof(sdrfm_pcm_limit_params) * (size_t)k->n_streams);
  if (J) *J = k->J;
  return SDRFM_OK;
}

int sdrfm_pcm_limit_process_batch(sdrfm_pcm_limit_t* k, const int16_t* in, size_t in_stride, uint32_t n, int16_t* out, size_t out_stride, uint32_t flags) {
  if (!k) return SDRFM_EINVAL;
  int rc = pcm_rows_refusal(flags, SDRFM_F_DEVICE_PTRS, n, SDRFM_LIMIT_N_MAX, in, in_stride, out, out_stride);
  if (rc != SDRFM_OK) return rc == PCM_ROWS_EMPTY ? SDRFM_OK : rc;
  const uint32_t ns = k->n_streams;
  const size_t need = 2 * (size_t)n;
  if (!pcm_rows_capacity(ns, in_stride, need) || !pcm_rows_capacity(ns, out_stride, need)) return SDRFM_ECAPACITY;
  STRY(hipSetDevice(k->hs.device), SDRFM_FAIL);
  if (flags & SDRFM_F_DEVICE_PTRS) return limit_launch(k, in, in_stride, n, out, out_stride);
  // host buffers: stage, limit in place, copy back, synchronous
  RowStage& st = k->stage;
  rc = row_stage_reserve(st, RowShape{1024u, PCM_PAIR_BYTES, ns, 0, 0, true}, n, 0);
  if (rc != SDRFM_OK) return rc;
  rc = rows_to_device(st, PCM_PAIR_BYTES, 0, in, sizeof(int16_t) * pcm_rows_pitch(ns, in_stride, need), PCM_PAIR_BYTES * n, ns, k->hs.cur);
  if (rc != SDRFM_OK) return rc;
  int16_t* const d_buf = static_cast<int16_t*>(st.d_in);
  rc = limit_launch(k, d_buf, 2 * (size_t)st.cap_in, n, d_buf, 2 * (size_t)st.cap_in);
  if (rc != SDRFM_OK) return rc;
  return rows_to_host(st, PCM_PAIR_BYTES, out, sizeof(int16_t) * pcm_rows_pitch(ns, out_stride, need), n, nullptr, ns, k->hs.cur);
}

int sdrfm_pcm_limit_read(sdrfm_pcm_limit_t* k, sdrfm_pcm_limit_rec* out, uint32_t flags) {
  if (!k || !out || (flags & ~(SDRFM_F_DEVICE_PTRS | SDRFM_AMETER_F_RESET)) || (uintptr_t)out % 8 != 0) return SDRFM_EINVAL;
  // a reset takes the records only, back to rec0: the state stays and the stream continues
  return records_read(k->hs, out, k->d_rec, sizeof(sdrfm_pcm_limit_rec) * (size_t)k->n_streams, k->rec0, flags);
}

int sdrfm_pcm_limit_get_state(sdrfm_pcm_limit_t* k, int32_t* state) {
  if (!k || !state) return SDRFM_EINVAL;
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
  STRY(hipMemcpy(state, k->d_state, sizeof(int32_t) * (size_t)k->words * k->n_streams, hipMemcpyDeviceToHost), SDRFM_FAIL);
  return SDRFM_OK;
}

int sdrfm_pcm_limit_set_stream(sdrfm_pcm_limit_t* k, void* hip_stream) {
  return k ? host_stream_use(k->hs, hip_stream) : SDRFM_EINVAL;
}

int sdrfm_pcm_limit_synchronize(sdrfm_pcm_limit_t* k) { return k ? host_stream_wait(k->hs) : SDRFM_EINVAL; }

const char* sdrfm_pcm_limit_kernel_name(const sdrfm_pcm_limit_t* k) { return k ? (k->nt ? "pcm-limit-tp" : "pcm-limit") : nullptr; }

}  // extern "C"
