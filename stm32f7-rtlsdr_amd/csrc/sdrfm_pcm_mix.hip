/*
 * sdrfm_pcm_mix.hip — the PCM mix bus behind the sdrfm_pcm_mix_* C-ABI (include/sdrfm.h): n_bus stereo rows formed from n_in
 * stereo rows under per-slot ramped gains, on the device.  The arithmetic is the host routine sdrfm_pcm_mix_s16's (csrc/pcm_mix.c) and
 * all-integer, so the outputs and the records are that routine's bit for bit.
 *
 *   k_pcm_mix   grid (n_bus, spans) of 256 lanes, a workgroup per SDRFM_PCM_MIX_SPAN pairs of one bus.  The body, the arithmetic and the geometry
 *               are in csrc/sdrfm_pcm_mix.h.
 *
 * The handle keeps the slots and J on the host and the slots' copy on the device; a ramp is a closed form of (g0, gt, slew, J), so the kernel
 * carries no state.  The records are added to by 64-bit integer atomics and zeroed by reset and by a read that asks for it.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/sdrfm.h"
#include "sdrfm_pcm_mix.h"

#define STRY(expr, code)                                                                                       \
  do {                                                                                                         \
    hipError_t e__ = (expr);                                                                                   \
    if (e__ != hipSuccess) {                                                                                   \
      fprintf(stderr, "[sdrfm] %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e__), __FILE__, __LINE__);  \
      return (code);                                                                                           \
    }                                                                                                          \
  } while (0)

static_assert(sizeof(sdrfm_pcm_mix_slot) == 16 && sizeof(PmixSlot) == 16, "a slot is four uint32");
static_assert(sizeof(sdrfm_pcm_mix_rec) == 32, "the record is four uint64");
static_assert(PMIX_SPAN == SDRFM_PCM_MIX_SPAN && PMIX_NONE == SDRFM_PCM_MIX_NONE && PMIX_CURVE_LEN == SDRFM_PCM_MIX_CURVE_LEN, "the header's constants");
static_assert(PMIX_MODES == SDRFM_PCM_MIX_SWAP + 1u, "the header's modes");

namespace {

__global__ void __launch_bounds__(PMIX_NT) k_pcm_mix(PmixParams p) {
  __shared__ uint16_t table[PMIX_CURVE_LEN + 3u];
  __shared__ uint32_t red[4];
  pcm_mix_block(p, table, red);
}

}  // namespace

struct sdrfm_pcm_mix {
  uint32_t n_in, n_bus, n_slots, slew, J;
  int device;
  hipStream_t own_stream, stream;
  sdrfm_pcm_mix_slot* slots;       // host: [n_bus][n_slots], as the device holds them
  sdrfm_pcm_mix_slot* d_slots;
  uint16_t* d_curve;               // 129 values, or nullptr
  sdrfm_pcm_mix_rec* d_rec;        // [n_bus]
  int16_t* d_in;                   // staging for host-pointer calls: [n_in][2 cap] and [n_bus][2 cap]
  int16_t* d_out;
  int16_t* h_out;
  uint32_t cap;                    // pairs per row the staging holds
};

static void mix_free(sdrfm_pcm_mix* k) {
  if (!k) return;
  (void)hipSetDevice(k->device);
  if (k->d_slots) (void)hipFree(k->d_slots);
  if (k->d_curve) (void)hipFree(k->d_curve);
  if (k->d_rec) (void)hipFree(k->d_rec);
  if (k->d_in) (void)hipFree(k->d_in);
  if (k->d_out) (void)hipFree(k->d_out);
  free(k->h_out);
  free(k->slots);
  if (k->own_stream) (void)hipStreamDestroy(k->own_stream);
  delete k;
}

static size_t mix_slot_count(const sdrfm_pcm_mix* k) { return (size_t)k->n_bus * k->n_slots; }

// one call over device buffers on the handle's stream; J moves with it
static int mix_launch(sdrfm_pcm_mix* k, const int16_t* in, size_t in_stride, uint32_t n, int16_t* out, size_t out_stride) {
  PmixParams p;
  p.in = in; p.in_stride = k->n_in > 1 ? in_stride : 0; p.out = out; p.out_stride = k->n_bus > 1 ? out_stride : 0;
  p.slots = reinterpret_cast<const PmixSlot*>(k->d_slots); p.curve = k->d_curve;
  p.rec = reinterpret_cast<unsigned long long*>(k->d_rec);
  p.n = n; p.n_slots = k->n_slots; p.slew = k->slew; p.J = k->J;
  hipLaunchKernelGGL(k_pcm_mix, dim3(k->n_bus, pmix_spans(n)), dim3(PMIX_NT), 0, k->stream, p);
  STRY(hipGetLastError(), SDRFM_FAIL);
  k->J = audio_ctl_advance(k->J, n);
  return SDRFM_OK;
}

static int mix_reserve(sdrfm_pcm_mix* k, uint32_t n) {
  if (n <= k->cap) return SDRFM_OK;
  if (k->d_in) (void)hipFree(k->d_in);
  if (k->d_out) (void)hipFree(k->d_out);
  free(k->h_out);
  k->d_in = nullptr; k->d_out = nullptr; k->h_out = nullptr; k->cap = 0;
  const uint32_t cap = (n + 1023u) & ~1023u;
  k->h_out = (int16_t*)malloc(sizeof(int16_t) * 2 * (size_t)cap * k->n_bus);
  if (!k->h_out || hipMalloc(&k->d_in, sizeof(int16_t) * 2 * (size_t)cap * k->n_in) != hipSuccess ||
      hipMalloc(&k->d_out, sizeof(int16_t) * 2 * (size_t)cap * k->n_bus) != hipSuccess)
    return SDRFM_ENOMEM;
  k->cap = cap;
  return SDRFM_OK;
}

// the slots to the device, behind whatever launch may still read them
static int mix_upload(sdrfm_pcm_mix* k) {
  STRY(hipSetDevice(k->device), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  STRY(hipMemcpy(k->d_slots, k->slots, sizeof(sdrfm_pcm_mix_slot) * mix_slot_count(k), hipMemcpyHostToDevice), SDRFM_FAIL);
  return SDRFM_OK;
}

extern "C" {

int sdrfm_pcm_mix_create(const sdrfm_pcm_mix_config* cfg, const uint16_t* curve, sdrfm_pcm_mix_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!cfg || cfg->flags || cfg->n_in < 1u || cfg->n_in > PMIX_ROWS_MAX || cfg->n_bus < 1u || cfg->n_bus > PMIX_ROWS_MAX || cfg->n_slots < 1u ||
      cfg->n_slots > PMIX_SLOTS_MAX || cfg->slew < 1u || cfg->slew > PMIX_ONE)
    return SDRFM_EINVAL;
  if (curve && !pmix_curve_ok(curve)) return SDRFM_EINVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) return SDRFM_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SDRFM_NO_DEVICE;
  STRY(hipSetDevice(cfg->device), SDRFM_NO_DEVICE);
  sdrfm_pcm_mix* k = new (std::nothrow) sdrfm_pcm_mix();
  if (!k) return SDRFM_ENOMEM;
  memset(static_cast<void*>(k), 0, sizeof(*k));
  k->n_in = cfg->n_in; k->n_bus = cfg->n_bus; k->n_slots = cfg->n_slots; k->slew = cfg->slew; k->device = cfg->device;
  const size_t ns = mix_slot_count(k);
  k->slots = (sdrfm_pcm_mix_slot*)malloc(sizeof(sdrfm_pcm_mix_slot) * ns);
  if (!k->slots) { mix_free(k); return SDRFM_ENOMEM; }
  for (size_t s = 0; s < ns; ++s) { k->slots[s].src = SDRFM_PCM_MIX_NONE; k->slots[s].mode = SDRFM_PCM_MIX_STEREO; k->slots[s].g0 = k->slots[s].gt = 0; }
  const bool ok = hipStreamCreateWithFlags(&k->own_stream, hipStreamNonBlocking) == hipSuccess &&
                  hipMalloc(&k->d_slots, sizeof(sdrfm_pcm_mix_slot) * ns) == hipSuccess &&
                  hipMalloc(&k->d_rec, sizeof(sdrfm_pcm_mix_rec) * k->n_bus) == hipSuccess &&
                  (!curve || hipMalloc(&k->d_curve, sizeof(uint16_t) * PMIX_CURVE_LEN) == hipSuccess);
  if (!ok) { mix_free(k); return SDRFM_ENOMEM; }
  k->stream = k->own_stream;
  if (hipMemcpy(k->d_slots, k->slots, sizeof(sdrfm_pcm_mix_slot) * ns, hipMemcpyHostToDevice) != hipSuccess ||
      (curve && hipMemcpy(k->d_curve, curve, sizeof(uint16_t) * PMIX_CURVE_LEN, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemsetAsync(k->d_rec, 0, sizeof(sdrfm_pcm_mix_rec) * k->n_bus, k->stream) != hipSuccess || hipStreamSynchronize(k->stream) != hipSuccess) {
    mix_free(k);
    return SDRFM_FAIL;
  }
  *out = k;
  return SDRFM_OK;
}

void sdrfm_pcm_mix_destroy(sdrfm_pcm_mix_t* k) {
  if (!k) return;
  (void)hipSetDevice(k->device);
  (void)hipStreamSynchronize(k->stream);
  mix_free(k);
}

int sdrfm_pcm_mix_reset(sdrfm_pcm_mix_t* k) {
  if (!k) return SDRFM_EINVAL;
  STRY(hipSetDevice(k->device), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  STRY(hipMemsetAsync(k->d_rec, 0, sizeof(sdrfm_pcm_mix_rec) * (size_t)k->n_bus, k->stream), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  return SDRFM_OK;
}

// every check comes before any device work; the calls wait for the handle's stream before they replace what a launch may still read
int sdrfm_pcm_mix_set_routes(sdrfm_pcm_mix_t* k, const uint32_t* src, const uint32_t* mode) {
  if (!k || (!src && !mode)) return SDRFM_EINVAL;
  const size_t ns = mix_slot_count(k);
  for (size_t s = 0; s < ns; ++s) {
    if (src && src[s] != SDRFM_PCM_MIX_NONE && src[s] >= k->n_in) return SDRFM_EINVAL;
    if (mode && mode[s] >= PMIX_MODES) return SDRFM_EINVAL;
  }
  for (size_t s = 0; s < ns; ++s) {
    if (src) k->slots[s].src = src[s];
    if (mode) k->slots[s].mode = mode[s];
  }
  return mix_upload(k);
}

int sdrfm_pcm_mix_set_gains(sdrfm_pcm_mix_t* k, const uint32_t* target, uint32_t jump) {
  if (!k || !target || jump > 1u) return SDRFM_EINVAL;
  const size_t ns = mix_slot_count(k);
  for (size_t s = 0; s < ns; ++s)
    if (target[s] > PMIX_ONE) return SDRFM_EINVAL;
  for (size_t s = 0; s < ns; ++s) {                               // the ramps restart where they have got to
    k->slots[s].g0 = jump ? target[s] : audio_ctl_ramp(k->slots[s].g0, k->slots[s].gt, k->slew, k->J);
    k->slots[s].gt = target[s];
  }
  k->J = 0;
  return mix_upload(k);
}

int sdrfm_pcm_mix_get_slots(const sdrfm_pcm_mix_t* k, sdrfm_pcm_mix_slot* out, uint32_t* J) {
  if (!k) return SDRFM_EINVAL;
  if (out) memcpy(out, k->slots, sizeof(sdrfm_pcm_mix_slot) * mix_slot_count(k));
  if (J) *J = k->J;
  return SDRFM_OK;
}

int sdrfm_pcm_mix_process_batch(sdrfm_pcm_mix_t* k, const int16_t* in, size_t in_stride, uint32_t n, int16_t* out, size_t out_stride, uint32_t flags) {
  if (!k) return SDRFM_EINVAL;
  if (flags & ~SDRFM_F_DEVICE_PTRS) return SDRFM_EINVAL;
  if (n > PMIX_N_MAX) return SDRFM_EINVAL;
  if ((in_stride | out_stride) & 1u) return SDRFM_EINVAL;           // rows are read and written as (L, R) dwords
  if (n == 0) return SDRFM_OK;
  if (!in || !out) return SDRFM_EINVAL;
  const bool device_ptrs = (flags & SDRFM_F_DEVICE_PTRS) != 0;
  if (device_ptrs && ((uintptr_t)in % 4 != 0 || (uintptr_t)out % 4 != 0)) return SDRFM_EINVAL;
  if ((k->n_in > 1 && in_stride < 2 * (size_t)n) || (k->n_bus > 1 && out_stride < 2 * (size_t)n)) return SDRFM_ECAPACITY;
  // bus b writes while bus c reads: the rows' byte ranges must be apart
  const size_t is = k->n_in > 1 ? in_stride : 2 * (size_t)n, os = k->n_bus > 1 ? out_stride : 2 * (size_t)n;
  const uintptr_t in0 = (uintptr_t)in, in1 = in0 + sizeof(int16_t) * ((k->n_in - 1u) * is + 2 * (size_t)n);
  const uintptr_t out0 = (uintptr_t)out, out1 = out0 + sizeof(int16_t) * ((k->n_bus - 1u) * os + 2 * (size_t)n);
  if (in0 < out1 && out0 < in1) return SDRFM_EINVAL;
  STRY(hipSetDevice(k->device), SDRFM_FAIL);
  if (device_ptrs) return mix_launch(k, in, in_stride, n, out, out_stride);
  // host buffers: stage, mix, copy back, synchronous
  int rc = mix_reserve(k, n);
  if (rc != SDRFM_OK) return rc;
  STRY(hipMemcpy2DAsync(k->d_in, sizeof(int16_t) * 2 * k->cap, in, sizeof(int16_t) * is, sizeof(int16_t) * 2 * n, k->n_in, hipMemcpyHostToDevice,
                        k->stream), SDRFM_FAIL);
  rc = mix_launch(k, k->d_in, 2 * (size_t)k->cap, n, k->d_out, 2 * (size_t)k->cap);
  if (rc != SDRFM_OK) return rc;
  STRY(hipMemcpy2DAsync(k->h_out, sizeof(int16_t) * 2 * k->cap, k->d_out, sizeof(int16_t) * 2 * k->cap, sizeof(int16_t) * 2 * n, k->n_bus,
                        hipMemcpyDeviceToHost, k->stream), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  for (uint32_t b = 0; b < k->n_bus; ++b) memcpy(out + b * os, k->h_out + (size_t)b * 2 * k->cap, sizeof(int16_t) * 2 * n);   // exactly 2n int16 per row
  return SDRFM_OK;
}

int sdrfm_pcm_mix_read(sdrfm_pcm_mix_t* k, sdrfm_pcm_mix_rec* out, uint32_t flags) {
  if (!k || !out || (flags & ~(SDRFM_F_DEVICE_PTRS | SDRFM_AMETER_F_RESET)) || (uintptr_t)out % 8 != 0) return SDRFM_EINVAL;
  STRY(hipSetDevice(k->device), SDRFM_FAIL);
  const size_t bytes = sizeof(sdrfm_pcm_mix_rec) * (size_t)k->n_bus;
  if (flags & SDRFM_F_DEVICE_PTRS) {                              // enqueued on the handle's stream, and nowhere else
    STRY(hipMemcpyAsync(out, k->d_rec, bytes, hipMemcpyDeviceToDevice, k->stream), SDRFM_FAIL);
    if (flags & SDRFM_AMETER_F_RESET) STRY(hipMemsetAsync(k->d_rec, 0, bytes, k->stream), SDRFM_FAIL);
    return SDRFM_OK;
  }
  STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  STRY(hipMemcpy(out, k->d_rec, bytes, hipMemcpyDeviceToHost), SDRFM_FAIL);
  if (flags & SDRFM_AMETER_F_RESET) {
    STRY(hipMemsetAsync(k->d_rec, 0, bytes, k->stream), SDRFM_FAIL);
    STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  }
  return SDRFM_OK;
}

int sdrfm_pcm_mix_set_stream(sdrfm_pcm_mix_t* k, void* hip_stream) {
  if (!k) return SDRFM_EINVAL;
  STRY(hipSetDevice(k->device), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  k->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : k->own_stream;
  return SDRFM_OK;
}

int sdrfm_pcm_mix_synchronize(sdrfm_pcm_mix_t* k) {
  if (!k) return SDRFM_EINVAL;
  STRY(hipSetDevice(k->device), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->stream), SDRFM_FAIL);
  return SDRFM_OK;
}

const char* sdrfm_pcm_mix_kernel_name(const sdrfm_pcm_mix_t* k) { return k ? "pcm-mix" : nullptr; }

}  // extern "C"
