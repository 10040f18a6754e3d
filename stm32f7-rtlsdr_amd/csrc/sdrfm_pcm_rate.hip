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
#include "sdrfm_host.h"
#include "sdrfm_pcm_rate.h"

namespace {

__global__ void __launch_bounds__(SDRFM_RATE_NT) k_pcm_rate(RateParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned rate_lds[];
  rate_stream_span(rate_lds, p);
}

}  // namespace

struct sdrfm_pcm_rate {
  uint32_t n_streams, nt, logph;
  HostStream hs;
  unsigned* d_table;    // [(NPH + 1)][nt / 2 + 1]
  uint64_t* d_step;     // [n_streams]
  uint64_t* d_pos;      // [2][n_streams]
  unsigned* d_hist;     // [2][n_streams][nt - 1]
  uint32_t cur;         // the set the next call reads
  uint64_t* step;       // host: the steps, and the mirror of the device's pos
  uint64_t* pos;
  uint32_t* cnt;        // scratch: the counts of the call being made
  RowStage stage;       // staging for host-pointer calls: pairs, the two sides grown apart (n in, the largest count out)
};

static void rate_free(sdrfm_pcm_rate* k) {
  if (!k) return;
  (void)hipSetDevice(k->hs.device);
  if (k->d_table) (void)hipFree(k->d_table);
  if (k->d_step) (void)hipFree(k->d_step);
  if (k->d_pos) (void)hipFree(k->d_pos);
  if (k->d_hist) (void)hipFree(k->d_hist);
  row_stage_free(k->stage);
  free(k->step);
  free(k->pos);
  free(k->cnt);
  host_stream_close(k->hs);
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
  hipLaunchKernelGGL(k_pcm_rate, dim3(spans, k->n_streams), dim3(SDRFM_RATE_NT), rate_lds_bytes(p.span, max_step, k->nt, k->logph), k->hs.cur, p);
  STRY(hipGetLastError(), SDRFM_FAIL);
  for (uint32_t s = 0; s < k->n_streams; ++s) k->pos[s] = rate_advance(k->pos[s], k->step[s], n, k->cnt[s]);
  k->cur ^= 1u;
  return SDRFM_OK;
}

extern "C" {

int sdrfm_pcm_rate_create(const sdrfm_pcm_rate_config* cfg, sdrfm_pcm_rate_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!cfg || !cfg->n_streams || cfg->flags || !cfg->coef) return SDRFM_EINVAL;
  if (sdrfm_pcm_rate_check_coef(cfg->coef, cfg->n_taps, cfg->log2_phases) != SDRFM_OK) return SDRFM_EINVAL;
  if (const int rc = host_open_device(cfg->device); rc != SDRFM_OK) return rc;
  sdrfm_pcm_rate* k = new (std::nothrow) sdrfm_pcm_rate();
  if (!k) return SDRFM_ENOMEM;
  memset(static_cast<void*>(k), 0, sizeof(*k));
  const uint32_t ns = cfg->n_streams, nt = cfg->n_taps;
  k->n_streams = ns; k->nt = nt; k->logph = cfg->log2_phases; k->hs.device = cfg->device;
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
  const bool ok = host_stream_open(k->hs, cfg->device) == SDRFM_OK &&
                  hipMalloc(&k->d_table, sizeof(unsigned) * tabdw) == hipSuccess && hipMalloc(&k->d_step, sizeof(uint64_t) * ns) == hipSuccess &&
                  hipMalloc(&k->d_pos, sizeof(uint64_t) * 2 * ns) == hipSuccess &&
                  hipMalloc(&k->d_hist, sizeof(unsigned) * 2 * (size_t)ns * (nt - 1u)) == hipSuccess;
  if (!ok) { free(tab); rate_free(k); return SDRFM_ENOMEM; }
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
  (void)host_stream_wait(k->hs);
  rate_free(k);
}

int sdrfm_pcm_rate_reset(sdrfm_pcm_rate_t* k) {
  if (!k) return SDRFM_EINVAL;
  STRY(hipSetDevice(k->hs.device), SDRFM_FAIL);                   // unlike the limiter and the mix bus: no wait for the stream before the state is cleared
  STRY(hipMemsetAsync(k->d_pos, 0, sizeof(uint64_t) * 2 * (size_t)k->n_streams, k->hs.cur), SDRFM_FAIL);
  STRY(hipMemsetAsync(k->d_hist, 0, sizeof(unsigned) * 2 * (size_t)k->n_streams * (k->nt - 1u), k->hs.cur), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->hs.cur), SDRFM_FAIL);
  for (uint32_t s = 0; s < k->n_streams; ++s) k->pos[s] = 0;
  k->cur = 0;
  return SDRFM_OK;
}

// every check comes before any device work; the call waits for the handle's stream before it replaces the steps a launch may still read
int sdrfm_pcm_rate_set_step(sdrfm_pcm_rate_t* k, const uint64_t* step) {
  if (!k || !step) return SDRFM_EINVAL;
  for (uint32_t s = 0; s < k->n_streams; ++s)
    if (step[s] < SDRFM_RATE_STEP_MIN || step[s] > SDRFM_RATE_STEP_MAX) return SDRFM_EINVAL;
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
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
  const uint32_t ns = k->n_streams;
  int rc = pcm_rows_refusal(flags, SDRFM_F_DEVICE_PTRS, n, SDRFM_RATE_N_MAX, in, in_stride, out, out_stride);
  if (rc == PCM_ROWS_EMPTY) {
    for (uint32_t s = 0; n_out && s < ns; ++s) n_out[s] = 0;
    return SDRFM_OK;
  }
  if (rc != SDRFM_OK) return rc;
  uint64_t max_step = 0;
  const uint32_t max_cnt = rate_counts(k, n, k->cnt, &max_step);
  const size_t need_in = 2 * (size_t)n, need_out = 2 * (size_t)max_cnt;
  if (!pcm_rows_capacity(ns, in_stride, need_in) || !pcm_rows_capacity(ns, out_stride, need_out)) return SDRFM_ECAPACITY;
  STRY(hipSetDevice(k->hs.device), SDRFM_FAIL);
  if (flags & SDRFM_F_DEVICE_PTRS) {
    rc = rate_launch(k, in, in_stride, n, out, out_stride, max_cnt, max_step);
    for (uint32_t s = 0; rc == SDRFM_OK && n_out && s < ns; ++s) n_out[s] = k->cnt[s];
    return rc;
  }
  // host buffers: stage, run, copy back exactly 2 cnt[s] int16 per row, synchronous
  RowStage& st = k->stage;
  rc = row_stage_reserve(st, RowShape{1024u, PCM_PAIR_BYTES, ns, PCM_PAIR_BYTES, ns, true}, n, max_cnt);
  if (rc != SDRFM_OK) return rc;
  rc = rows_to_device(st, PCM_PAIR_BYTES, 0, in, sizeof(int16_t) * pcm_rows_pitch(ns, in_stride, need_in), PCM_PAIR_BYTES * n, ns, k->hs.cur);
  if (rc != SDRFM_OK) return rc;
  rc = rate_launch(k, static_cast<int16_t*>(st.d_in), 2 * (size_t)st.cap_in, n, static_cast<int16_t*>(st.d_out), 2 * (size_t)st.cap_out, max_cnt, max_step);
  if (rc != SDRFM_OK) return rc;
  rc = rows_to_host(st, PCM_PAIR_BYTES, out, sizeof(int16_t) * pcm_rows_pitch(ns, out_stride, need_out), max_cnt, k->cnt, ns, k->hs.cur);
  for (uint32_t s = 0; rc == SDRFM_OK && n_out && s < ns; ++s) n_out[s] = k->cnt[s];
  return rc;
}

int sdrfm_pcm_rate_get_state(sdrfm_pcm_rate_t* k, uint64_t* step, uint64_t* pos) {
  if (!k) return SDRFM_EINVAL;
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
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
  return k ? host_stream_use(k->hs, hip_stream) : SDRFM_EINVAL;
}

int sdrfm_pcm_rate_synchronize(sdrfm_pcm_rate_t* k) { return k ? host_stream_wait(k->hs) : SDRFM_EINVAL; }

const char* sdrfm_pcm_rate_kernel_name(const sdrfm_pcm_rate_t* k) { return k ? "pcm-rate" : nullptr; }

}  // extern "C"
