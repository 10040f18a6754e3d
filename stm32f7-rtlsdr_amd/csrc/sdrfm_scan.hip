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
 */
#include <new>

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
  (void)hipFree(h->d_ctaps); (void)hipFree(h->d_rot); (void)hipFree(h->d_meters);
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

// one call on device buffers, enqueued on the handle's stream
static int scan_enqueue(sdrfm_scan* h, const uint8_t* d_iq, size_t iq_stride, uint32_t nbytes, sdrfm_scan_meter* d_meters) {
  const uint32_t ns = h->cfg.n_streams;
  if (h->step.lds > PF_LDS_BUDGET) return SDRFM_FAIL;            // (no shape within the header's limits gets here: NY = 2 fits them all)
  ScanParams p;
  memset(&p, 0, sizeof p);
  if (h->shared_input) iq_stride = 0;                            // every stream reads row 0
  front_fill(h->f, p, d_iq, iq_stride, nbytes, nullptr, h->step);
  p.meters = reinterpret_cast<unsigned long long*>(d_meters);
  p.ctaps = h->d_ctaps; p.rot = h->d_rot;
  p.blocks_per_stream = front_split(p.M, p.NDT, p.H, ns, h->slots);
  p.span = p.M ? (p.M + p.blocks_per_stream - 1) / p.blocks_per_stream : 0;
  if (hipMemsetAsync(d_meters, 0, sizeof(sdrfm_scan_meter) * ns, h->f.stream) != hipSuccess) return SDRFM_FAIL;
  const dim3 grid(ns * p.blocks_per_stream), block(PF_THREADS);
  if (h->fast) k_scan<64, 10, 101, true><<<grid, block, h->step.lds, h->f.stream>>>(p);
  else k_scan<0, 0, 0, true><<<grid, block, h->step.lds, h->f.stream>>>(p);
  if (hipGetLastError() != hipSuccess) return SDRFM_FAIL;
  front_advance(h->f, p.N);
  return SDRFM_OK;
}

int sdrfm_scan_process_batch(sdrfm_scan_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, sdrfm_scan_meter* meters, uint32_t flags) {
  if (!h || !meters) return SDRFM_EINVAL;
  if (flags & ~SDRFM_F_DEVICE_PTRS) return SDRFM_EINVAL;         // SDRFM_F_OVERLAP: not for this handle
  if (nbytes & 1u) return SDRFM_EODD;
  if (nbytes > h->f.max_bytes) return SDRFM_ECAPACITY;
  const uint32_t ns = h->cfg.n_streams;
  const bool dev = (flags & SDRFM_F_DEVICE_PTRS) != 0;
  if (nbytes == 0) {                                             // no launch: zero records
    if (!dev) { memset(meters, 0, sizeof(sdrfm_scan_meter) * ns); return SDRFM_OK; }
    if (hipSetDevice(h->f.device) != hipSuccess) return SDRFM_FAIL;
    return hipMemsetAsync(meters, 0, sizeof(sdrfm_scan_meter) * ns, h->f.stream) == hipSuccess ? SDRFM_OK : SDRFM_FAIL;
  }
  if (!iq) return SDRFM_EINVAL;
  if (ns > 1 && !h->shared_input && iq_stride < nbytes) return SDRFM_ECAPACITY;
  if (hipSetDevice(h->f.device) != hipSuccess) return SDRFM_FAIL;
  if (dev) return scan_enqueue(h, iq, iq_stride, nbytes, meters);

  if (h->shared_input) {
    if (hipMemcpyAsync(h->f.d_iq, iq, nbytes, hipMemcpyHostToDevice, h->f.stream) != hipSuccess) return SDRFM_FAIL;
  } else if (front_stage_in(h->f, iq, iq_stride, nbytes) != SDRFM_OK) {
    return SDRFM_FAIL;
  }
  const int rc = scan_enqueue(h, h->f.d_iq, h->f.d_iq_stride, nbytes, h->d_meters);
  if (rc != SDRFM_OK) return rc;
  if (hipMemcpyAsync(meters, h->d_meters, sizeof(sdrfm_scan_meter) * ns, hipMemcpyDeviceToHost, h->f.stream) != hipSuccess) return SDRFM_FAIL;
  return hipStreamSynchronize(h->f.stream) == hipSuccess ? SDRFM_OK : SDRFM_FAIL;
}

int sdrfm_scan_set_stream(sdrfm_scan_t* h, void* hip_stream) {
  if (!h) return SDRFM_EINVAL;
  h->f.stream = hip_stream ? (hipStream_t)hip_stream : h->f.own_stream;
  return SDRFM_OK;
}

int sdrfm_scan_synchronize(sdrfm_scan_t* h) {
  if (!h) return SDRFM_EINVAL;
  if (hipSetDevice(h->f.device) != hipSuccess || hipStreamSynchronize(h->f.stream) != hipSuccess) return SDRFM_FAIL;
  return SDRFM_OK;
}

const char* sdrfm_scan_kernel_name(const sdrfm_scan_t* h) { return h ? h->kernel_name : ""; }

}  // extern "C"
