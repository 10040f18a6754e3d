/*
 * sdrfm_scan.hip — the scan handle behind the sdrfm_scan_* C-ABI (include/sdrfm.h): for every stream — a candidate offset
 * of a capture — one small integer record of what the tuned walk of sdrfm_pilot_front.h sees on the way to the pilot filter's q: the
 * channel power |y|^2, d and d^2, the pilot power |q|^2 and its square, and how many d's passed the pilot gate.
 *
 * The walk is the tuned broadcast kernel's up to q (K2 with the stream's complex taps, sdrfm_discriminate_tuned, the pilot filter), with
 * nothing behind q: H = P - 1, no carriers, no output chains, no tails.  What a new d adds to the record and how the lanes' sums reach it
 * is sdrfm_meter.h's, which the broadcast handle's metered kernels call as well.
 *
 * k_scan<0, 0, 0, true> and k_scan<64, 10, 101, true> are the header's two forms of the tuned walk; the meters are the same code in both.
 *
 * k_scan_hist (sdrfm_scan_process_batch_hist) is the same walk and the same record with sdrfm_hist.h's bins beside it:
 * one count per new d by the size of d, 512 bins a stream.  It carries the plain call's state, so the two calls alternate on a handle.
 */
#include <new>

#include "sdrfm_hist.h"
#include "sdrfm_meter.h"
#include "sdrfm_pilot_front.h"

namespace {

struct ScanParams : FrontParams {
  unsigned long long* meters;  // [ns][8]: sdrfm_scan_meter as eight 64-bit words, zeroed before the launch
  const float* ctaps;          // [ns][2T], (hr[k], hi[k]) pairs
  const float* rot;            // [ns]
};

template <int FT, int FD, int FP, bool TU>
__global__ void __launch_bounds__(PF_THREADS) k_scan(ScanParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t T = FT > 0 ? FT : p.T, P = FT > 0 ? FP : p.P, H = p.H, NY = p.NY;
  // LDS: region (x as f16 pairs | the H carried and the step's new d's) | ys[NY] | hb[H] | tps[P] | hs[2T]; hb and tps padded so that
  // every array starts on 16 bytes
  FrontWg<FT, FD, FP, TU> w;
  w.xs = reinterpret_cast<h2_t*>(smem);
  w.ds = reinterpret_cast<float*>(smem);
  w.ys = reinterpret_cast<f2_t*>(smem + 4 * (size_t)p.region_words);
  w.hb = reinterpret_cast<float*>(w.ys + NY);
  w.tps = reinterpret_cast<f2_t*>(w.hb + ((H + 3) & ~3u));
  w.hs = reinterpret_cast<float*>(w.tps + ((P + 1) & ~1u));
  const uint32_t st = blockIdx.x / p.blocks_per_stream;
  w.ctaps = p.ctaps + (size_t)st * 2 * T;
  w.rot = p.rot[st];
  front_begin(p, w);
  const int tid = w.tid;
  const float* ds = w.ds;
  const f2_t* ys = w.ys;
  MeterAcc acc;

  front_walk(p, w, [&](int a, int b, bool full) {
    front_d_stage(p, w, a, b);
    if (full) {
      // ---- output o stands for the new d a + o: its y lies at ys[a + o - yA], its d at ds[H + o], its pilot window ds[o .. o + P) ends at it
      const int yo = a - (a - 1 > 0 ? a - 1 : 0);
      front_pilot(w, 0, b - a, [&](int o, f2_t q) __attribute__((always_inline)) {
        meter_take(acc, ys[o + yo], ds[H + o], q, p.pmin2);
      });
    }
    __syncthreads();
  });

  meter_flush(acc, p.meters + 8 * (size_t)w.s, tid);
  front_hand_over(p, w);
}

// ---- the hist call: k_scan's walk and record, and beside meter_take one count per new d in the workgroup's LDS bins
struct ScanHistParams : ScanParams {
  uint32_t* hist;              // [ns][hist_stride]: a row's first SDRFM_SCAN_HIST_BINS words, zeroed before the launch
  size_t hist_stride;          // words
};

template <int FT, int FD, int FP, bool TU>
__global__ void __launch_bounds__(PF_THREADS) k_scan_hist(ScanHistParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t T = FT > 0 ? FT : p.T, P = FT > 0 ? FP : p.P, H = p.H, NY = p.NY;
  // LDS: k_scan's layout, then bins[SDRFM_SCAN_HIST_BINS] on the next 16 bytes behind hs
  FrontWg<FT, FD, FP, TU> w;
  w.xs = reinterpret_cast<h2_t*>(smem);
  w.ds = reinterpret_cast<float*>(smem);
  w.ys = reinterpret_cast<f2_t*>(smem + 4 * (size_t)p.region_words);
  w.hb = reinterpret_cast<float*>(w.ys + NY);
  w.tps = reinterpret_cast<f2_t*>(w.hb + ((H + 3) & ~3u));
  w.hs = reinterpret_cast<float*>(w.tps + ((P + 1) & ~1u));
  uint32_t* bins = reinterpret_cast<uint32_t*>(smem + hist_bins_offset((size_t)(reinterpret_cast<unsigned char*>(w.hs + 2 * T) - smem)));
  const uint32_t st = blockIdx.x / p.blocks_per_stream;
  w.ctaps = p.ctaps + (size_t)st * 2 * T;
  w.rot = p.rot[st];
  front_begin(p, w);
  const int tid = w.tid;
  const float* ds = w.ds;
  const f2_t* ys = w.ys;
  MeterAcc acc;
  hist_zero(bins, tid);
  __syncthreads();

  front_walk(p, w, [&](int a, int b, bool full) {
    front_d_stage(p, w, a, b);
    if (full) {
      const int yo = a - (a - 1 > 0 ? a - 1 : 0);
      front_pilot(w, 0, b - a, [&](int o, f2_t q) __attribute__((always_inline)) {
        const float d = ds[H + o];
        meter_take(acc, ys[o + yo], d, q, p.pmin2);
        hist_take(bins, d);
      });
    }
    __syncthreads();
  });

  meter_flush(acc, p.meters + 8 * (size_t)w.s, tid);
  __syncthreads();
  hist_flush(bins, p.hist + (size_t)w.s * p.hist_stride, tid);
  front_hand_over(p, w);
}

}  // namespace

// =================================================================================================================
//  Host side: handle, argument checks (all before any device work), launch geometry.  The walk's state is the header's PilotFront.
// =================================================================================================================
struct sdrfm_scan {
  sdrfm_scan_config cfg;                       // pilot_coeffs points at the copy in f; ctaps and rot are not kept on the host
  PilotFront f;
  bool fast = false, shared_input = false;
  FrontStep step;
  uint32_t slots = 1;
  char kernel_name[64];
  bool hist_fast = false, last_hist = false;   // the hist call's kernel form; whether the last call was a hist call
  FrontStep hist_step;                         // the hist call's step: the bins take LDS from it at the LDS-limited shapes
  uint32_t hist_slots = 1;
  char hist_kernel_name[72];
  uint32_t* d_hist = nullptr;                  // host-buffer hist calls: the rows [ns][512], allocated at the first such call
  float* d_ctaps = nullptr;                    // [ns][2T]
  float* d_rot = nullptr;                      // [ns]
  sdrfm_scan_meter* d_meters = nullptr;        // host-buffer calls: the records [ns]
};

namespace {

constexpr uint32_t SCAN_MAX_BYTES = METER_MAX_BYTES;

// LDS bytes of a step geometry (see the layout in k_scan); Tg is not used
size_t scan_lds(uint32_t T, uint32_t D, uint32_t P, uint32_t Tg, uint32_t H, uint32_t NY, uint32_t NDT, uint32_t* region_words) {
  (void)Tg;
  const size_t nx = (size_t)(NY - 1) * D + T + 4, nds = (size_t)H + NDT + 4;
  size_t rw = nx > nds ? nx : nds;
  rw = (rw + 3) & ~(size_t)3;
  if (region_words) *region_words = (uint32_t)rw;
  return 4 * rw + 8 * (size_t)NY + 4 * (size_t)((H + 3) & ~3u) + 8 * (size_t)((P + 1) & ~1u) + 8 * (size_t)T;
}

// LDS bytes of the hist kernel's step: scan_lds (rounded up to 16 where T is odd) and the bins
size_t scan_hist_lds(uint32_t T, uint32_t D, uint32_t P, uint32_t Tg, uint32_t H, uint32_t NY, uint32_t NDT, uint32_t* region_words) {
  return hist_bins_offset(scan_lds(T, D, P, Tg, H, NY, NDT, region_words)) + HIST_LDS_BYTES;
}

// the tuning a handle takes: finite, |rot| <= pi, and per stream sum(|hr| + |hi|) <= 16 (the header's int64 bounds)
bool scan_tuning_ok(const float* ctaps, const float* rot, uint32_t ns, uint32_t T) {
  if (!ctaps || !rot || !meter_taps_ok(ctaps, ns, 2 * T, METER_MAX_CTAP_SUM)) return false;
  for (uint32_t s = 0; s < ns; ++s) {
    if (!std::isfinite(rot[s]) || std::fabs(rot[s]) > 0x1.921fb6p+1f) return false;
  }
  return true;
}

void scan_free(sdrfm_scan* h) {
  if (!h) return;
  front_free(h->f);
  (void)hipFree(h->d_ctaps); (void)hipFree(h->d_rot); (void)hipFree(h->d_meters); (void)hipFree(h->d_hist);
  delete h;
}

int scan_upload_tuning(sdrfm_scan* h, const float* ctaps, const float* rot) {
  const size_t ns = h->f.ns, T = h->f.T;
  if (hipMemcpy(h->d_ctaps, ctaps, sizeof(float) * ns * 2 * T, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->d_rot, rot, sizeof(float) * ns, hipMemcpyHostToDevice) != hipSuccess)
    return SDRFM_FAIL;
  return SDRFM_OK;
}

}  // namespace

extern "C" {

int sdrfm_scan_create(const sdrfm_scan_config* cfg, sdrfm_scan_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!cfg || cfg->struct_size != sizeof(sdrfm_scan_config)) return SDRFM_EINVAL;
  // (the front's real channel taps are not used by a tuned walk: the first stream's row stands in for them in its checks and its copy)
  if (!front_config_ok(cfg->n_streams, cfg->fir_taps, cfg->fir_decim, cfg->ctaps, cfg->pilot_taps, cfg->pilot_coeffs, cfg->pilot_min))
    return SDRFM_EINVAL;
  if (cfg->flags & ~(SDRFM_SCAN_CFG_FORCE_GENERIC | SDRFM_SCAN_CFG_SHARED_INPUT)) return SDRFM_EINVAL;
  if (cfg->max_bytes_per_call > SCAN_MAX_BYTES) return SDRFM_EINVAL;
  if (!scan_tuning_ok(cfg->ctaps, cfg->rot, cfg->n_streams, cfg->fir_taps)) return SDRFM_EINVAL;
  if (!meter_taps_ok(cfg->pilot_coeffs, 1, 2 * cfg->pilot_taps, METER_MAX_PTAP_SUM)) return SDRFM_EINVAL;
  hipDeviceProp_t prop;
  int rc = front_open_device(cfg->device, &prop);
  if (rc != SDRFM_OK) return rc;

  sdrfm_scan* h = new (std::nothrow) sdrfm_scan();
  if (!h) return SDRFM_ENOMEM;
  h->cfg = *cfg;
  const uint32_t T = cfg->fir_taps, D = cfg->fir_decim, P = cfg->pilot_taps, H = P - 1;
  const size_t ns = cfg->n_streams;
  rc = front_alloc(h->f, cfg->n_streams, T, D, cfg->ctaps, P, cfg->pilot_coeffs, cfg->pilot_min, H, cfg->max_bytes_per_call, cfg->device);
  if (rc != SDRFM_OK) { scan_free(h); return rc; }
  h->cfg.pilot_coeffs = h->f.bc;
  h->cfg.ctaps = nullptr;
  h->cfg.rot = nullptr;
  h->shared_input = (cfg->flags & SDRFM_SCAN_CFG_SHARED_INPUT) != 0;
  if (hipMalloc(&h->d_ctaps, sizeof(float) * ns * 2 * T) != hipSuccess || hipMalloc(&h->d_rot, sizeof(float) * ns) != hipSuccess ||
      hipMalloc(&h->d_meters, sizeof(sdrfm_scan_meter) * ns) != hipSuccess) {
    scan_free(h);
    return SDRFM_ENOMEM;
  }
  if (scan_upload_tuning(h, cfg->ctaps, cfg->rot) != SDRFM_OK) { scan_free(h); return SDRFM_FAIL; }
  h->step = front_step(scan_lds, 64, 10, 101, 0, H, PF_FAST_NY, PF_FAST_NY - 1);
  h->fast = !(cfg->flags & SDRFM_SCAN_CFG_FORCE_GENERIC) && T == 64 && D == 10 && P == 101 && h->step.lds <= PF_LDS_BUDGET;
  if (!h->fast) h->step = front_step_generic(scan_lds, T, D, P, 0, H);
  if (h->fast) snprintf(h->kernel_name, sizeof h->kernel_name, "scan-fast T64 D10 P101");
  else snprintf(h->kernel_name, sizeof h->kernel_name, "scan-generic T%u D%u P%u", T, D, P);
  h->slots = front_slots(h->fast ? k_scan<64, 10, 101, true> : k_scan<0, 0, 0, true>, h->step.lds, prop);
  h->hist_step = front_step(scan_hist_lds, 64, 10, 101, 0, H, PF_FAST_NY, PF_FAST_NY - 1);
  h->hist_fast = h->fast && h->hist_step.lds <= PF_LDS_BUDGET;
  if (!h->hist_fast) h->hist_step = front_step_generic(scan_hist_lds, T, D, P, 0, H);
  if (h->hist_fast) snprintf(h->hist_kernel_name, sizeof h->hist_kernel_name, "scan-fast T64 D10 P101 + hist");
  else snprintf(h->hist_kernel_name, sizeof h->hist_kernel_name, "scan-generic T%u D%u P%u + hist", T, D, P);
  h->hist_slots = front_slots(h->hist_fast ? k_scan_hist<64, 10, 101, true> : k_scan_hist<0, 0, 0, true>, h->hist_step.lds, prop);
  rc = sdrfm_scan_reset(h);
  if (rc != SDRFM_OK) { scan_free(h); return rc; }
  *out = h;
  return SDRFM_OK;
}

void sdrfm_scan_destroy(sdrfm_scan_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->f.device);
  (void)hipStreamSynchronize(h->f.stream);
  scan_free(h);
}

int sdrfm_scan_reset(sdrfm_scan_t* h) {
  if (!h) return SDRFM_EINVAL;
  return front_reset(h->f);
}

int sdrfm_scan_tune(sdrfm_scan_t* h, const float* ctaps, const float* rot) {
  if (!h) return SDRFM_EINVAL;
  if (!scan_tuning_ok(ctaps, rot, h->f.ns, h->f.T)) return SDRFM_EINVAL;
  if (hipSetDevice(h->f.device) != hipSuccess) return SDRFM_FAIL;
  if (hipStreamSynchronize(h->f.stream) != hipSuccess) return SDRFM_FAIL;   // no launch still reads the taps about to be replaced
  if (scan_upload_tuning(h, ctaps, rot) != SDRFM_OK) return SDRFM_FAIL;
  return sdrfm_scan_reset(h);
}

// one call on device buffers, enqueued on the handle's stream; d_hist: the hist call's rows, nullptr for the plain call
static int scan_enqueue(sdrfm_scan* h, const uint8_t* d_iq, size_t iq_stride, uint32_t nbytes, sdrfm_scan_meter* d_meters, uint32_t* d_hist,
                        size_t hist_stride) {
  const uint32_t ns = h->cfg.n_streams;
  const FrontStep& step = d_hist ? h->hist_step : h->step;
  if (step.lds > PF_LDS_BUDGET) return SDRFM_FAIL;               // (no shape within the header's limits gets here: NY = 2 fits them all)
  ScanHistParams p;
  memset(&p, 0, sizeof p);
  if (h->shared_input) iq_stride = 0;                            // every stream reads row 0
  front_fill(h->f, p, d_iq, iq_stride, nbytes, nullptr, step);
  p.meters = reinterpret_cast<unsigned long long*>(d_meters);
  p.ctaps = h->d_ctaps; p.rot = h->d_rot;
  p.hist = d_hist; p.hist_stride = hist_stride;
  p.blocks_per_stream = front_split(p.M, p.NDT, p.H, ns, d_hist ? h->hist_slots : h->slots);
  p.span = p.M ? (p.M + p.blocks_per_stream - 1) / p.blocks_per_stream : 0;
  if (hipMemsetAsync(d_meters, 0, sizeof(sdrfm_scan_meter) * ns, h->f.stream) != hipSuccess) return SDRFM_FAIL;
  const dim3 grid(ns * p.blocks_per_stream), block(PF_THREADS);
  if (d_hist) {
    if (hipMemset2DAsync(d_hist, sizeof(uint32_t) * hist_stride, 0, HIST_LDS_BYTES, ns, h->f.stream) != hipSuccess) return SDRFM_FAIL;
    if (h->hist_fast) k_scan_hist<64, 10, 101, true><<<grid, block, step.lds, h->f.stream>>>(p);
    else k_scan_hist<0, 0, 0, true><<<grid, block, step.lds, h->f.stream>>>(p);
  } else {
    const ScanParams& ps = p;
    if (h->fast) k_scan<64, 10, 101, true><<<grid, block, step.lds, h->f.stream>>>(ps);
    else k_scan<0, 0, 0, true><<<grid, block, step.lds, h->f.stream>>>(ps);
  }
  if (hipGetLastError() != hipSuccess) return SDRFM_FAIL;
  front_advance(h->f, p.N);
  h->last_hist = d_hist != nullptr;
  return SDRFM_OK;
}

// the plain call (hist == nullptr) and the hist call: the checks in one order, all before any device work
static int scan_call(sdrfm_scan* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, sdrfm_scan_meter* meters, uint32_t* hist, size_t hist_stride,
                     uint32_t flags) {
  if (flags & ~SDRFM_F_DEVICE_PTRS) return SDRFM_EINVAL;         // SDRFM_F_OVERLAP: not for this handle
  if (nbytes & 1u) return SDRFM_EODD;
  if (nbytes > h->f.max_bytes) return SDRFM_ECAPACITY;
  const uint32_t ns = h->cfg.n_streams;
  const bool dev = (flags & SDRFM_F_DEVICE_PTRS) != 0;
  if (nbytes == 0) {                                             // no launch: zero records, zero rows
    if (!dev) {
      memset(meters, 0, sizeof(sdrfm_scan_meter) * ns);
      for (uint32_t s = 0; hist && s < ns; ++s) memset(hist + (size_t)s * hist_stride, 0, HIST_LDS_BYTES);
      return SDRFM_OK;
    }
    if (hipSetDevice(h->f.device) != hipSuccess) return SDRFM_FAIL;
    if (hist && hipMemset2DAsync(hist, sizeof(uint32_t) * hist_stride, 0, HIST_LDS_BYTES, ns, h->f.stream) != hipSuccess) return SDRFM_FAIL;
    return hipMemsetAsync(meters, 0, sizeof(sdrfm_scan_meter) * ns, h->f.stream) == hipSuccess ? SDRFM_OK : SDRFM_FAIL;
  }
  if (!iq) return SDRFM_EINVAL;
  if (ns > 1 && !h->shared_input && iq_stride < nbytes) return SDRFM_ECAPACITY;
  if (hipSetDevice(h->f.device) != hipSuccess) return SDRFM_FAIL;
  if (dev) return scan_enqueue(h, iq, iq_stride, nbytes, meters, hist, hist_stride);

  if (hist && !h->d_hist && hipMalloc(&h->d_hist, (size_t)HIST_LDS_BYTES * ns) != hipSuccess) { h->d_hist = nullptr; return SDRFM_ENOMEM; }
  if (h->shared_input) {
    if (hipMemcpyAsync(h->f.d_iq, iq, nbytes, hipMemcpyHostToDevice, h->f.stream) != hipSuccess) return SDRFM_FAIL;
  } else if (front_stage_in(h->f, iq, iq_stride, nbytes) != SDRFM_OK) {
    return SDRFM_FAIL;
  }
  const int rc = scan_enqueue(h, h->f.d_iq, h->f.d_iq_stride, nbytes, h->d_meters, hist ? h->d_hist : nullptr, HIST_BINS);
  if (rc != SDRFM_OK) return rc;
  if (hipMemcpyAsync(meters, h->d_meters, sizeof(sdrfm_scan_meter) * ns, hipMemcpyDeviceToHost, h->f.stream) != hipSuccess) return SDRFM_FAIL;
  if (hist && hipMemcpy2DAsync(hist, sizeof(uint32_t) * hist_stride, h->d_hist, HIST_LDS_BYTES, HIST_LDS_BYTES, ns, hipMemcpyDeviceToHost,
                               h->f.stream) != hipSuccess)
    return SDRFM_FAIL;
  return hipStreamSynchronize(h->f.stream) == hipSuccess ? SDRFM_OK : SDRFM_FAIL;
}

int sdrfm_scan_process_batch(sdrfm_scan_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, sdrfm_scan_meter* meters, uint32_t flags) {
  if (!h || !meters) return SDRFM_EINVAL;
  return scan_call(h, iq, iq_stride, nbytes, meters, nullptr, 0, flags);
}

int sdrfm_scan_process_batch_hist(sdrfm_scan_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, sdrfm_scan_meter* meters, uint32_t* hist,
                                  size_t hist_stride, uint32_t flags) {
  if (!h || !meters || !hist || hist_stride < HIST_BINS) return SDRFM_EINVAL;   // (before the handle is read)
  return scan_call(h, iq, iq_stride, nbytes, meters, hist, hist_stride, flags);
}

int sdrfm_scan_set_stream(sdrfm_scan_t* h, void* hip_stream) {
  if (!h) return SDRFM_EINVAL;
  return front_use_stream(h->f, hip_stream);
}

int sdrfm_scan_synchronize(sdrfm_scan_t* h) {
  if (!h) return SDRFM_EINVAL;
  if (hipSetDevice(h->f.device) != hipSuccess || hipStreamSynchronize(h->f.stream) != hipSuccess) return SDRFM_FAIL;
  return SDRFM_OK;
}

// the kernel of the handle's last call: the plain call's until a hist call has been made, then whichever call came last
const char* sdrfm_scan_kernel_name(const sdrfm_scan_t* h) { return !h ? "" : h->last_hist ? h->hist_kernel_name : h->kernel_name; }

}  // extern "C"
