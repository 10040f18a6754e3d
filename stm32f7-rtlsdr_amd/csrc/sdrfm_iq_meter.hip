/*
 * sdrfm_iq_meter.hip — the raw-capture IQ meter behind the sdrfm_iq_meter_* C-ABI (include/sdrfm.h): per stream the sums of
 * the raw bytes — level, rails, DC and the I/Q cross term — and, where asked for, the 2 x 256 counts of the byte values, on the device.
 * Everything is a sum of small integers, so records and rows are the host routine sdrfm_iq_meter_u8's (csrc/iq_meter.c) integer for integer.
 *
 *   k_iq_meter<false>   grid (streams x workgroups per stream) of 256 lanes: 16-byte loads behind a peeled head and tail, packed byte dot
 *                       products into 32-bit lane sums, joined per workgroup and added to the zeroed record by 64-bit integer atomics.
 *   k_iq_meter<true>    the same with IQM_HIST_REPL copies of the 512 bins in LDS, flushed once per workgroup.
 * The body, the arithmetic and the geometry are in csrc/sdrfm_iq_meter.h.  The handle carries no stream state.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/sdrfm.h"
#include "sdrfm_host.h"
#include "sdrfm_iq_meter.h"

static_assert(sizeof(sdrfm_iq_meter) == 64, "the record is 8 uint64");
static_assert(IQM_MAX_BYTES == SDRFM_IQ_MAX_BYTES && 512u == SDRFM_IQ_HIST_BINS, "the header's limits");

namespace {

template <bool HIST>
__global__ void __launch_bounds__(IQM_NT) k_iq_meter(IqMeterParams p) {
  __shared__ __attribute__((aligned(16))) uint32_t bins[HIST ? 512u * IQM_HIST_REPL : 4u];
  __shared__ unsigned long long red[8];
  iq_meter_block<HIST>(p, bins, red);
}

}  // namespace

struct sdrfm_iq_meter_handle {
  uint32_t n_streams, max_bytes;
  HostStream hs;
  sdrfm_iq_meter* d_meters;        // host-buffer calls: the records [n_streams]
  uint32_t* d_hist;                // host-buffer hist calls: the rows [n_streams][512], allocated at the first such call
  RowStage stage;                  // host-buffer calls: the rows staged, bytes; nothing comes back through it
  bool last_hist;
};

static void iqm_free(sdrfm_iq_meter_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->hs.device);
  if (h->d_meters) (void)hipFree(h->d_meters);
  if (h->d_hist) (void)hipFree(h->d_hist);
  row_stage_free(h->stage);
  host_stream_close(h->hs);
  delete h;
}

// one call on device buffers, enqueued on the handle's stream: both outputs zeroed, then added to
static int iqm_enqueue(sdrfm_iq_meter_handle* h, const uint8_t* d_iq, size_t iq_stride, uint32_t nbytes, sdrfm_iq_meter* d_meters, uint32_t* d_hist) {
  const uint32_t ns = h->n_streams;
  STRY(hipMemsetAsync(d_meters, 0, sizeof(sdrfm_iq_meter) * (size_t)ns, h->hs.cur), SDRFM_FAIL);
  if (d_hist) STRY(hipMemsetAsync(d_hist, 0, sizeof(uint32_t) * 512u * (size_t)ns, h->hs.cur), SDRFM_FAIL);
  h->last_hist = d_hist != nullptr;
  if (nbytes == 0) return SDRFM_OK;
  const IqmGrid g = iqm_grid(ns, nbytes);
  IqMeterParams p;
  p.iq = d_iq; p.iq_stride = ns > 1 ? iq_stride : 0; p.nbytes = nbytes; p.bps = g.bps; p.share = g.share;
  p.meters = reinterpret_cast<unsigned long long*>(d_meters); p.hist = d_hist;
  const dim3 grid(ns * g.bps), block(IQM_NT);
  if (d_hist) hipLaunchKernelGGL(k_iq_meter<true>, grid, block, 0, h->hs.cur, p);
  else hipLaunchKernelGGL(k_iq_meter<false>, grid, block, 0, h->hs.cur, p);
  STRY(hipGetLastError(), SDRFM_FAIL);
  return SDRFM_OK;
}

extern "C" {

int sdrfm_iq_meter_create(const sdrfm_iq_meter_config* cfg, sdrfm_iq_meter_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!cfg || cfg->struct_size != sizeof(sdrfm_iq_meter_config)) return SDRFM_EINVAL;
  if (!cfg->n_streams || cfg->n_streams > IQM_MAX_STREAMS || cfg->max_bytes_per_call > IQM_MAX_BYTES || cfg->flags) return SDRFM_EINVAL;
  if (const int rc = host_open_device(cfg->device); rc != SDRFM_OK) return rc;
  sdrfm_iq_meter_handle* h = new (std::nothrow) sdrfm_iq_meter_handle();
  if (!h) return SDRFM_ENOMEM;
  memset(static_cast<void*>(h), 0, sizeof(*h));
  h->n_streams = cfg->n_streams; h->max_bytes = cfg->max_bytes_per_call ? cfg->max_bytes_per_call : (1u << 20); h->hs.device = cfg->device;
  if (host_stream_open(h->hs, cfg->device) != SDRFM_OK ||
      hipMalloc(&h->d_meters, sizeof(sdrfm_iq_meter) * (size_t)h->n_streams) != hipSuccess) {
    iqm_free(h);
    return SDRFM_ENOMEM;
  }
  *out = h;
  return SDRFM_OK;
}

void sdrfm_iq_meter_destroy(sdrfm_iq_meter_t* h) {
  if (!h) return;
  (void)host_stream_wait(h->hs);
  iqm_free(h);
}

// the checks in sdrfm_scan_process_batch's order, all before any device work
int sdrfm_iq_meter_process_batch(sdrfm_iq_meter_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, sdrfm_iq_meter* meters, uint32_t* hist,
                                 uint32_t flags) {
  if (!h || !meters) return SDRFM_EINVAL;
  if (flags & ~SDRFM_F_DEVICE_PTRS) return SDRFM_EINVAL;         // SDRFM_F_OVERLAP: not for this handle
  if ((uintptr_t)meters % 8 != 0 || (uintptr_t)hist % 4 != 0) return SDRFM_EINVAL;
  if (nbytes & 1u) return SDRFM_EODD;
  if (nbytes > h->max_bytes) return SDRFM_ECAPACITY;
  const uint32_t ns = h->n_streams;
  const bool dev = (flags & SDRFM_F_DEVICE_PTRS) != 0;
  if (nbytes == 0) {                                             // no launch: zero records, zero rows
    if (!dev) {
      memset(meters, 0, sizeof(sdrfm_iq_meter) * (size_t)ns);
      if (hist) memset(hist, 0, sizeof(uint32_t) * 512u * (size_t)ns);
      h->last_hist = hist != nullptr;
      return SDRFM_OK;
    }
    STRY(hipSetDevice(h->hs.device), SDRFM_FAIL);
    return iqm_enqueue(h, nullptr, 0, 0, meters, hist);
  }
  if (!iq) return SDRFM_EINVAL;
  if (!pcm_rows_capacity(ns, iq_stride, nbytes)) return SDRFM_ECAPACITY;
  STRY(hipSetDevice(h->hs.device), SDRFM_FAIL);
  if (dev) return iqm_enqueue(h, iq, iq_stride, nbytes, meters, hist);
  // host buffers: stage, meter, copy back, synchronous
  RowStage& st = h->stage;
  int rc = row_stage_reserve(st, RowShape{IQM_CHUNK, 1, ns, 0, 0, false}, nbytes, 0);
  if (rc != SDRFM_OK) return rc;
  if (hist && !h->d_hist && hipMalloc(&h->d_hist, sizeof(uint32_t) * 512u * (size_t)ns) != hipSuccess) { h->d_hist = nullptr; return SDRFM_ENOMEM; }
  rc = rows_to_device(st, 1, 0, iq, pcm_rows_pitch(ns, iq_stride, nbytes), nbytes, ns, h->hs.cur);
  if (rc != SDRFM_OK) return rc;
  rc = iqm_enqueue(h, static_cast<const uint8_t*>(st.d_in), st.cap_in, nbytes, h->d_meters, hist ? h->d_hist : nullptr);
  if (rc != SDRFM_OK) return rc;
  STRY(hipMemcpyAsync(meters, h->d_meters, sizeof(sdrfm_iq_meter) * (size_t)ns, hipMemcpyDeviceToHost, h->hs.cur), SDRFM_FAIL);
  if (hist) STRY(hipMemcpyAsync(hist, h->d_hist, sizeof(uint32_t) * 512u * (size_t)ns, hipMemcpyDeviceToHost, h->hs.cur), SDRFM_FAIL);
  STRY(hipStreamSynchronize(h->hs.cur), SDRFM_FAIL);
  return SDRFM_OK;
}

int sdrfm_iq_meter_set_stream(sdrfm_iq_meter_t* h, void* hip_stream) {
  if (!h) return SDRFM_EINVAL;
  h->hs.cur = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->hs.own;   // unlike the other handles: no hipSetDevice and no wait for the stream in use
  return SDRFM_OK;
}

int sdrfm_iq_meter_synchronize(sdrfm_iq_meter_t* h) { return h ? host_stream_wait(h->hs) : SDRFM_EINVAL; }

// unlike the other handles: "" for NULL, not NULL
const char* sdrfm_iq_meter_kernel_name(const sdrfm_iq_meter_t* h) { return !h ? "" : h->last_hist ? "iq-meter-hist" : "iq-meter"; }

}  // extern "C"
