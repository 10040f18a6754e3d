/*
 * sdrfm_pcm_rate.hip — the per-stream PCM rate matcher behind the sdrfm_pcm_rate_* C-ABI (include/sdrfm.h): the int16 stereo
 * rows the PCM sinks leave, resampled per stream by a 32.32 fixed-point step through a polyphase table, on the device.  The arithmetic is the host
 * routine sdrfm_pcm_rate_s16's (csrc/pcm_rate.c) and all-integer, so the outputs, pos and hist are that routine's bit for bit.
 *
 *   k_pcm_rate   one workgroup of 256 lanes per (span of consecutive outputs, stream), grid (spans, streams).  The table and the span's input window
 *                are staged in LDS, L and R in planes of their own so that two neighbouring taps of a channel are one dword; a lane takes every
 *                256th output of the span: P is one 64-bit multiply-add, the two half-row sums per row and channel are packed 16-bit dot products
 *                into int32 accumulators (exact by the table's half-row bound), the interpolation and the rounding are 64-bit, the pair is one
 *                dword store.  The span length is a pure function of the launch's largest step (rate_span_len, sdrfm_pcm_rate.h).
 *
 * State: pos and hist in two sets on the device.  Call c reads set c & 1 and writes the other — span 0 of a stream does — so the spans of a stream
 * never race.  cnt and pos are closed forms of (pos, step, n): the handle keeps a host mirror of pos, which is how n_out is known when a call only
 * enqueues; sdrfm_pcm_rate_get_state holds the device's pos to the mirror.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/sdrfm.h"
#include "sdrfm_pcm_rate.h"

#define STRY(expr, code)                                                                                       \
  do {                                                                                                         \
    hipError_t e__ = (expr);                                                                                   \
    if (e__ != hipSuccess) {                                                                                   \
      fprintf(stderr, "[sdrfm] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e__), __FILE__, __LINE__);  \
      return (code);                                                                                           \
    }                                                                                                          \
  } while (0)

namespace {

__global__ void __launch_bounds__(SDRFM_RATE_NT) k_pcm_rate(RateParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned rate_lds[];
  rate_stream_span(rate_lds, p);
}

}  // namespace

struct sdrfm_pcm_rate {
  uint32_t n_streams, nt, logph;
  int device;
  hipStream_t own_stream, stream;
  unsigned* d_table;    // [(NPH + 1)][nt / 2 + 1]
  uint64_t* d_step;     // [n_streams]
  uint64_t* d_pos;      // [2][n_streams]
  unsigned* d_hist;     // [2][n_streams][nt - 1]
  uint32_t cur;         // the set the next call reads
  uint64_t* step;       // host: the steps, and the mirror of the device's pos
  uint64_t* pos;
  uint32_t* cnt;        // scratch: the counts of the call being made
  int16_t* d_in;        // staging for host-pointer calls
  int16_t* d_out;
  int16_t* h_out;
  uint32_t cap_in, cap_out;   // pairs per stream the staging holds
};

static void rate_free(sdrfm_pcm_rate* k) {
  if (!k) return;
  (void)hipSetDevice(k->device);
  if (k->d_table) (void)hipFree(k->d_table);
  if (k->d_step) (void)hipFree(k->d_step);
  if (k->d_pos) (void)hipFree(k->d_pos);
  if (k->d_hist) (void)hipFree(k->d_hist);
  if (k->d_in) (void)hipFree(k->d_in);
  if (k->d_out) (void)hipFree(k->d_out);
  free(k->h_out);
  free(k->step);
  free(k->pos);
  free(k->cnt);
  if (k->own_stream) (void)hipStreamDestroy(k->own_stream);
  delete k;
}

// the counts of a call of n pairs from the mirror; returns their maximum and, with it, the largest step
static uint32_t rate_counts(const sdrfm_pcm_rate* k, uint32_t n, uint32_t* cnt, uint64_t* max_step) {
  uint32_t mx = 0;
  uint64_t ms = 0;
  for (uint32_t s = 0; s < k->n_streams; ++s) {
    const uint32_t c = rate_count(k->pos[s], k->step[s], n);
    if (cnt) cnt[s] = c;
    if (c > mx) mx = c;
    if (k->step[s] > ms) ms = k->step[s];
  }
  if (max_step) *max_step = ms;
  return mx;
}

// one call over device buffers on the handle's stream; the mirror moves with it
static int rate_launch(sdrfm_pcm_rate* k, const int16_t* in, size_t in_stride, uint32_t n, int16_t* out, size_t out_stride, uint32_t max_cnt,
                       uint64_t max_step) {
  RateParams p;
  p.in = in; p.in_stride = in_stride; p.out = out; p.out_stride = out_stride; p.table = reinterpret_cast<const uint4*>(k->d_table); p.step = k->d_step;
  p.pos_in = k->d_pos + (size_t)k->cur * k->n_streams;
  p.pos_out = k->d_pos + (size_t)(k->cur ^ 1u) * k->n_streams;
  p.hist_in = k->d_hist + (size_t)k->cur * k->n_streams * (k->nt - 1u);
  p.hist_out = k->d_hist + (size_t)(k->cur ^ 1u) * k->n_streams * (k->nt - 1u);
  p.n = n; p.nt = k->nt; p.logph = k->logph;
  p.span = rate_span_len(max_step, k->nt, k->logph);
  p.plane_dw = rate_plane_dwords(p.span, max_step, k->nt);
  const uint32_t spans = max_cnt ? (max_cnt + p.span - 1u) / p.span : 1u;   // span 0 carries the state even when nothing comes out
  hipLaunchKernelGGL(k_pcm_rate, dim3(spans, k->n_streams), dim3(SDRFM_RATE_NT), rate_lds_bytes(p.span, max_step, k->nt, k->logph), k->stream, p);
  STRY(hipGetLastError(), SDRFM_FAIL);
  for (uint32_t s = 0; s < k->n_streams; ++s) k->pos[s] = rate_advance(k->pos[s], k->step[s], n, k->cnt[s]);
  k->cur ^= 1u;
  return SDRFM_OK;
}

static int rate_reserve(sdrfm_pcm_rate* k, uint32_t n, uint32_t max_cnt) {
  if (n > k->cap_in) {
    if (k->d_in) (void)hipFree(k->d_in);
    k->d_in = nullptr; k->cap_in = 0;
    const uint32_t cap = (n + 1023u) & ~1023u;
    if (hipMalloc(&k->d_in, sizeof(int16_t) * 2 * (size_t)cap * k->n_streams) != hipSuccess) return SDRFM_ENOMEM;
    k->cap_in = cap;
  }
  if (max_cnt > k->cap_out) {
    if (k->d_out) (void)hipFree(k->d_out);
    free(k->h_out);
    k->d_out = nullptr; k->h_out = nullptr; k->cap_out = 0;
    const uint32_t cap = (max_cnt + 1023u) & ~1023u;
    k->h_out = (int16_t*)malloc(sizeof(int16_t) * 2 * (size_t)cap * k->n_streams);
    if (!k->h_out || hipMalloc(&k->d_out, sizeof(int16_t) * 2 * (size_t)cap * k->n_streams) != hipSuccess) return SDRFM_ENOMEM;
    k->cap_out = cap;
  }
  return SDRFM_OK;
}

extern "C" {

int sdrfm_pcm_rate_create(const sdrfm_pcm_rate_config* cfg, sdrfm_pcm_rate_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!cfg || !cfg->n_streams || cfg->flags || !cfg->coef) return SDRFM_EINVAL;
  if (sdrfm_pcm_rate_check_coef(cfg->coef, cfg->n_taps, cfg->log2_phases) != SDRFM_OK) return SDRFM_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) return SDRFM_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SDRFM_NO_DEVICE;
  STRY(hipSetDevice(cfg->device), SDRFM_NO_DEVICE);
  sdrfm_pcm_rate* k = new (std::nothrow) sdrfm_pcm_rate();
  if (!k) return SDRFM_ENOMEM;
  memset(static_cast<void*>(k), 0, sizeof(*k));
  const uint32_t ns = cfg->n_streams, nt = cfg->n_taps;
  k->n_streams = ns; k->nt = nt; k->logph = cfg->log2_phases; k->device = cfg->device;
  k->step = (uint64_t*)malloc(sizeof(uint64_t) * ns);
  k->pos = (uint64_t*)malloc(sizeof(uint64_t) * ns);
  k->cnt = (uint32_t*)malloc(sizeof(uint32_t) * ns);
  const uint32_t rows = (1u << k->logph) + 1u, rowdw = rate_row_dwords(nt), tabdw = rate_table_dwords(nt, k->logph);
  unsigned* tab = (unsigned*)calloc(tabdw, sizeof(unsigned));
  if (!k->step || !k->pos || !k->cnt || !tab) { free(tab); rate_free(k); return SDRFM_ENOMEM; }
  for (uint32_t p = 0; p < rows; ++p)
    for (uint32_t m = 0; m < nt / 2u; ++m)
      tab[(size_t)p * rowdw + m] = (uint16_t)cfg->coef[(size_t)p * nt + 2 * m] | ((unsigned)(uint16_t)cfg->coef[(size_t)p * nt + 2 * m + 1] << 16);
  for (uint32_t s = 0; s < ns; ++s) { k->step[s] = (uint64_t)1 << 32; k->pos[s] = 0; }
  const bool ok = hipStreamCreateWithFlags(&k->own_stream, hipStreamNonBlocking) == hipSuccess &&
                  hipMalloc(&k->d_table, sizeof(unsigned) * tabdw) == hipSuccess && hipMalloc(&k->d_step, sizeof(uint64_t) * ns) == hipSuccess &&
                  hipMalloc(&k->d_pos, sizeof(uint64_t) * 2 * ns) == hipSuccess &&
                  hipMalloc(&k->d_hist, sizeof(unsigned) * 2 * (size_t)ns * (nt - 1u)) == hipSuccess;
  if (!ok) { free(tab); rate_free(k); return SDRFM_ENOMEM; }
  k->stream = k->own_stream;
  const bool up = hipMemcpy(k->d_table, tab, sizeof(unsigned) * tabdw, hipMemcpyHostToDevice) == hipSuccess &&
                  hipMemcpy(k->d_step, k->step, sizeof(uint64_t) * ns, hipMemcpyHostToDevice) == hipSuccess;
  free(tab);
  if (!up) { rate_free(k); return SDRFM_FAIL; }
  const int rc = sdrfm_pcm_rate_reset(k);
  if (rc != SDRFM_OK) { rate_free(k); return rc; }
  *out = k;
  return SDRFM_OK;
}

void sdrfm_pcm_rate_destroy(sdrfm_pcm_rate_t* k) {
  if (!k) return;
  (void)hipSetDevice(k->device);
  (void)hipStreamSynchronize(k->stream);
  rate_free(k);
}

int sdrfm_pcm_rate_reset(sdrfm_pcm_rate_t* k) {
  if (!k) return SDRFM_EINVAL;
  STRY(hipSetDevice(k->device), SDRFM_FAIL);
  STRY(hipMemsetAsync(k->d_pos, 0, sizeof(uint64_t) * 2 * (size_t)k->n_streams, k->stream), SDRFM_FAIL);
  STRY(hipMemsetAsync(k->d_hist, 0, sizeof(unsigned) * 2 * (size_t)k->n_streams * (k->nt - 1u), k->stream), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  for (uint32_t s = 0; s < k->n_streams; ++s) k->pos[s] = 0;
  k->cur = 0;
  return SDRFM_OK;
}

// every check comes before any device work; the call waits for the handle's stream before it replaces the steps a launch may still read
int sdrfm_pcm_rate_set_step(sdrfm_pcm_rate_t* k, const uint64_t* step) {
  if (!k || !step) return SDRFM_EINVAL;
  for (uint32_t s = 0; s < k->n_streams; ++s)
    if (step[s] < SDRFM_RATE_STEP_MIN || step[s] > SDRFM_RATE_STEP_MAX) return SDRFM_EINVAL;
  STRY(hipSetDevice(k->device), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  STRY(hipMemcpy(k->d_step, step, sizeof(uint64_t) * (size_t)k->n_streams, hipMemcpyHostToDevice), SDRFM_FAIL);
  memcpy(k->step, step, sizeof(uint64_t) * (size_t)k->n_streams);
  return SDRFM_OK;
}

int sdrfm_pcm_rate_count(const sdrfm_pcm_rate_t* k, uint32_t n, uint32_t* n_out, uint32_t* max_out) {
  if (!k || n > SDRFM_RATE_N_MAX) return SDRFM_EINVAL;
  const uint32_t mx = rate_counts(k, n, n_out, nullptr);
  if (max_out) *max_out = mx;
  return SDRFM_OK;
}

int sdrfm_pcm_rate_process_batch(sdrfm_pcm_rate_t* k, const int16_t* in, size_t in_stride, uint32_t n, int16_t* out, size_t out_stride,
                                 uint32_t* n_out, uint32_t flags) {
  if (!k) return SDRFM_EINVAL;
  if (flags & ~SDRFM_F_DEVICE_PTRS) return SDRFM_EINVAL;
  if (n > SDRFM_RATE_N_MAX) return SDRFM_EINVAL;
  if ((in_stride | out_stride) & 1u) return SDRFM_EINVAL;           // rows are read and written as (L, R) dwords
  if (n == 0) {
    for (uint32_t s = 0; n_out && s < k->n_streams; ++s) n_out[s] = 0;
    return SDRFM_OK;
  }
  if (!in || !out) return SDRFM_EINVAL;
  const bool device_ptrs = (flags & SDRFM_F_DEVICE_PTRS) != 0;
  if (device_ptrs && ((uintptr_t)in % 4 != 0 || (uintptr_t)out % 4 != 0)) return SDRFM_EINVAL;
  uint64_t max_step = 0;
  const uint32_t max_cnt = rate_counts(k, n, k->cnt, &max_step);
  if (k->n_streams > 1 && (in_stride < 2 * (size_t)n || out_stride < 2 * (size_t)max_cnt)) return SDRFM_ECAPACITY;
  STRY(hipSetDevice(k->device), SDRFM_FAIL);
  if (device_ptrs) {
    const int rc = rate_launch(k, in, in_stride, n, out, out_stride, max_cnt, max_step);
    for (uint32_t s = 0; rc == SDRFM_OK && n_out && s < k->n_streams; ++s) n_out[s] = k->cnt[s];
    return rc;
  }
  // host buffers: stage, run, copy back, synchronous
  int rc = rate_reserve(k, n, max_cnt);
  if (rc != SDRFM_OK) return rc;
  const size_t is = (k->n_streams > 1) ? in_stride : 2 * (size_t)n, os = (k->n_streams > 1) ? out_stride : 2 * (size_t)max_cnt;
  STRY(hipMemcpy2DAsync(k->d_in, sizeof(int16_t) * 2 * k->cap_in, in, sizeof(int16_t) * is, sizeof(int16_t) * 2 * n, k->n_streams, hipMemcpyHostToDevice,
                        k->stream), SDRFM_FAIL);
  rc = rate_launch(k, k->d_in, 2 * (size_t)k->cap_in, n, k->d_out, 2 * (size_t)k->cap_out, max_cnt, max_step);
  if (rc != SDRFM_OK) return rc;
  if (max_cnt)
    STRY(hipMemcpy2DAsync(k->h_out, sizeof(int16_t) * 2 * k->cap_out, k->d_out, sizeof(int16_t) * 2 * k->cap_out, sizeof(int16_t) * 2 * max_cnt, k->n_streams,
                          hipMemcpyDeviceToHost, k->stream), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  for (uint32_t s = 0; s < k->n_streams; ++s) {                   // exactly 2 cnt[s] int16 per row
    if (k->cnt[s]) memcpy(out + s * os, k->h_out + (size_t)s * 2 * k->cap_out, sizeof(int16_t) * 2 * k->cnt[s]);
    if (n_out) n_out[s] = k->cnt[s];
  }
  return SDRFM_OK;
}

int sdrfm_pcm_rate_get_state(sdrfm_pcm_rate_t* k, uint64_t* step, uint64_t* pos) {
  if (!k) return SDRFM_EINVAL;
  STRY(hipSetDevice(k->device), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  uint64_t* dev = (uint64_t*)malloc(sizeof(uint64_t) * (size_t)k->n_streams);
  if (!dev) return SDRFM_ENOMEM;
  if (hipMemcpy(dev, k->d_pos + (size_t)k->cur * k->n_streams, sizeof(uint64_t) * (size_t)k->n_streams, hipMemcpyDeviceToHost) != hipSuccess) {
    free(dev);
    return SDRFM_FAIL;
  }
  const bool same = memcmp(dev, k->pos, sizeof(uint64_t) * (size_t)k->n_streams) == 0;
  if (pos) memcpy(pos, dev, sizeof(uint64_t) * (size_t)k->n_streams);
  if (step) memcpy(step, k->step, sizeof(uint64_t) * (size_t)k->n_streams);
  free(dev);
  return same ? SDRFM_OK : SDRFM_FAIL;
}

int sdrfm_pcm_rate_set_stream(sdrfm_pcm_rate_t* k, void* hip_stream) {
  if (!k) return SDRFM_EINVAL;
  STRY(hipSetDevice(k->device), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  k->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : k->own_stream;
  return SDRFM_OK;
}

int sdrfm_pcm_rate_synchronize(sdrfm_pcm_rate_t* k) {
  if (!k) return SDRFM_EINVAL;
  STRY(hipSetDevice(k->device), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  return SDRFM_OK;
}

const char* sdrfm_pcm_rate_kernel_name(const sdrfm_pcm_rate_t* k) { return k ? "pcm-rate" : nullptr; }

}  // extern "C"
