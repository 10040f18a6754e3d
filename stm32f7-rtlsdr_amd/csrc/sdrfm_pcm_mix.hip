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
#include "sdrfm_host.h"
#include "sdrfm_pcm_mix.h"

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
  HostStream hs;
  sdrfm_pcm_mix_slot* slots;       // host: [n_bus][n_slots], as the device holds them
  sdrfm_pcm_mix_slot* d_slots;
  uint16_t* d_curve;               // 129 values, or nullptr
  sdrfm_pcm_mix_rec* d_rec;        // [n_bus]
  RowStage stage;                  // staging for host-pointer calls: pairs, [n_in] rows in and [n_bus] rows out
};

static void mix_free(sdrfm_pcm_mix* k) {
  if (!k) return;
  (void)hipSetDevice(k->hs.device);
  if (k->d_slots) (void)hipFree(k->d_slots);
  if (k->d_curve) (void)hipFree(k->d_curve);
  if (k->d_rec) (void)hipFree(k->d_rec);
  row_stage_free(k->stage);
  free(k->slots);
  host_stream_close(k->hs);
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
  hipLaunchKernelGGL(k_pcm_mix, dim3(k->n_bus, pmix_spans(n)), dim3(PMIX_NT), 0, k->hs.cur, p);
  STRY(hipGetLastError(), SDRFM_FAIL);
  k->J = audio_ctl_advance(k->J, n);
  return SDRFM_OK;
}

// the slots to the device, behind whatever launch may still read them
static int mix_upload(sdrfm_pcm_mix* k) {
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
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
  if (const int rc = host_open_device(cfg->device); rc != SDRFM_OK) return rc;
  sdrfm_pcm_mix* k = new (std::nothrow) sdrfm_pcm_mix();
  if (!k) return SDRFM_ENOMEM;
  memset(static_cast<void*>(k), 0, sizeof(*k));
  k->n_in = cfg->n_in; k->n_bus = cfg->n_bus; k->n_slots = cfg->n_slots; k->slew = cfg->slew; k->hs.device = cfg->device;
  const size_t ns = mix_slot_count(k);
  k->slots = (sdrfm_pcm_mix_slot*)malloc(sizeof(sdrfm_pcm_mix_slot) * ns);
  if (!k->slots) { mix_free(k); return SDRFM_ENOMEM; }
  for (size_t s = 0; s < ns; ++s) { k->slots[s].src = SDRFM_PCM_MIX_NONE; k->slots[s].mode = SDRFM_PCM_MIX_STEREO; k->slots[s].g0 = k->slots[s].gt = 0; }
  const bool ok = host_stream_open(k->hs, cfg->device) == SDRFM_OK &&
                  hipMalloc(&k->d_slots, sizeof(sdrfm_pcm_mix_slot) * ns) == hipSuccess &&
                  hipMalloc(&k->d_rec, sizeof(sdrfm_pcm_mix_rec) * k->n_bus) == hipSuccess &&
                  (!curve || hipMalloc(&k->d_curve, sizeof(uint16_t) * PMIX_CURVE_LEN) == hipSuccess);
  if (!ok) { mix_free(k); return SDRFM_ENOMEM; }
  if (hipMemcpy(k->d_slots, k->slots, sizeof(sdrfm_pcm_mix_slot) * ns, hipMemcpyHostToDevice) != hipSuccess ||
      (curve && hipMemcpy(k->d_curve, curve, sizeof(uint16_t) * PMIX_CURVE_LEN, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemsetAsync(k->d_rec, 0, sizeof(sdrfm_pcm_mix_rec) * k->n_bus, k->hs.cur) != hipSuccess || hipStreamSynchronize(k->hs.cur) != hipSuccess) {
    mix_free(k);
    return SDRFM_FAIL;
  }
  *out = k;
  return SDRFM_OK;
}

void sdrfm_pcm_mix_destroy(sdrfm_pcm_mix_t* k) {
  if (!k) return;
  (void)host_stream_wait(k->hs);
  mix_free(k);
}

int sdrfm_pcm_mix_reset(sdrfm_pcm_mix_t* k) {
  if (!k) return SDRFM_EINVAL;
  if (const int rc = host_stream_wait(k->hs); rc != SDRFM_OK) return rc;
  STRY(hipMemsetAsync(k->d_rec, 0, sizeof(sdrfm_pcm_mix_rec) * (size_t)k->n_bus, k->hs.cur), SDRFM_FAIL);
  STRY(hipStreamSynchronize(k->hs.cur), SDRFM_FAIL);
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
  int rc = pcm_rows_refusal(flags, SDRFM_F_DEVICE_PTRS, n, PMIX_N_MAX, in, in_stride, out, out_stride);
  if (rc != SDRFM_OK) return rc == PCM_ROWS_EMPTY ? SDRFM_OK : rc;
  const size_t need = 2 * (size_t)n;
  if (!pcm_rows_capacity(k->n_in, in_stride, need) || !pcm_rows_capacity(k->n_bus, out_stride, need)) return SDRFM_ECAPACITY;
  const size_t is = pcm_rows_pitch(k->n_in, in_stride, need), os = pcm_rows_pitch(k->n_bus, out_stride, need);
  if (!pcm_rows_apart(in, k->n_in, is, out, k->n_bus, os, n)) return SDRFM_EINVAL;   // bus b writes while bus c reads
  STRY(hipSetDevice(k->hs.device), SDRFM_FAIL);
  if (flags & SDRFM_F_DEVICE_PTRS) return mix_launch(k, in, in_stride, n, out, out_stride);
  // host buffers: stage, mix, copy back, synchronous
  RowStage& st = k->stage;
  rc = row_stage_reserve(st, RowShape{1024u, PCM_PAIR_BYTES, k->n_in, PCM_PAIR_BYTES, k->n_bus, true}, n, n);
  if (rc != SDRFM_OK) return rc;
  rc = rows_to_device(st, PCM_PAIR_BYTES, 0, in, sizeof(int16_t) * is, PCM_PAIR_BYTES * n, k->n_in, k->hs.cur);
  if (rc != SDRFM_OK) return rc;
  rc = mix_launch(k, static_cast<int16_t*>(st.d_in), 2 * (size_t)st.cap_in, n, static_cast<int16_t*>(st.d_out), 2 * (size_t)st.cap_out);
  if (rc != SDRFM_OK) return rc;
  return rows_to_host(st, PCM_PAIR_BYTES, out, sizeof(int16_t) * os, n, nullptr, k->n_bus, k->hs.cur);
}

int sdrfm_pcm_mix_read(sdrfm_pcm_mix_t* k, sdrfm_pcm_mix_rec* out, uint32_t flags) {
  if (!k || !out || (flags & ~(SDRFM_F_DEVICE_PTRS | SDRFM_AMETER_F_RESET)) || (uintptr_t)out % 8 != 0) return SDRFM_EINVAL;
  return records_read(k->hs, out, k->d_rec, sizeof(sdrfm_pcm_mix_rec) * (size_t)k->n_bus, nullptr, flags);
}

int sdrfm_pcm_mix_set_stream(sdrfm_pcm_mix_t* k, void* hip_stream) {
  return k ? host_stream_use(k->hs, hip_stream) : SDRFM_EINVAL;
}

int sdrfm_pcm_mix_synchronize(sdrfm_pcm_mix_t* k) { return k ? host_stream_wait(k->hs) : SDRFM_EINVAL; }

const char* sdrfm_pcm_mix_kernel_name(const sdrfm_pcm_mix_t* k) { return k ? "pcm-mix" : nullptr; }

}  // extern "C"
