/*
 * sdrfm_rds.hip — the Radio Data System's complex baseband behind the sdrfm_rds_* C-ABI (include/sdrfm.h).
 *
 * The walk from the input bytes to the pilot filter's q = b * d is sdrfm_pilot_front.h's, shared with the stereo kernel.  What this file
 * adds behind q, at the discriminator rate: the 57 kHz carrier k = u2 q, u2 = q^2 / |q|^2 (gated by |q|^2 >= pilot_min^2; sdrfm_carrier.h), the mixed-down
 * z = (k * rds_gain) d[m - Δ], and the decimating low-pass w = g * z, two real chains.  H = P - 1 + Tr - 1.  A step's last two stages here:
 *   pilot   q, carrier, z of the step's new d's -> LDS behind the Tr - 1 z's carried from the previous step (the span's first step
 *           computes those Tr - 1 too: that is what the halo's d's are for); the pilot count of the new d's
 *   output  wr, wi -> HBM; one lane per chain (the re lanes first, then the im lanes), zr and zi in planes of their own so that the
 *           lanes' windows, Dr apart, spread over the banks (sdrfm_out_stages.h, shared with the broadcast kernel)
 * The halo is 2.7 times the stereo kernel's at the default shape (354 d's), and the pilot pass is the dearest one: carrying z from step
 * to step keeps it at one evaluation per d, so a step takes NY - 1 new d's whatever Tr is, and the prologue costs K1-K3 only.
 *
 * k_rds<0, 0, 0> and k_rds<64, 10, 101> are the header's two forms of the walk; the carrier and the output chains are the same code in both.
 */
#include <new>

#include "sdrfm_carrier.h"
#include "sdrfm_out_stages.h"
#include "sdrfm_pilot_front.h"

namespace {

struct RdsParams : FrontParams {
  float* bb;                   // [ns][bb_stride]: (wr, wi) pairs
  size_t bb_stride;
  const float* g;              // Tr
  uint32_t Tr, Dr;
  float rds_gain;
  uint32_t A;
  int32_t f0;
  uint32_t zplane;             // words of one z plane: Tr - 1 + NDT, made odd
};

template <int FT, int FD, int FP>
__global__ void __launch_bounds__(PF_THREADS) k_rds(RdsParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t P = FT > 0 ? FP : p.P;
  const uint32_t Tr = p.Tr, Dr = p.Dr, H = p.H, Dl = p.Dl, NY = p.NY, NDT = p.NDT, ZP = p.zplane;
  // LDS: region (x as f16 pairs | d's, zr's, zi's) | ys[NY] | hb[H] | tps[P] | gs[Tr] | hs[T] | zb[2 (Tr - 1)]; hb and tps padded so that gs
  // starts on 16 bytes.  gs holds the taps oldest first (gs[k] = g[Tr - 1 - k]): the output chains read them four at a time
  FrontWg<FT, FD, FP> w;
  w.xs = reinterpret_cast<h2_t*>(smem);
  w.ds = reinterpret_cast<float*>(smem);
  float* zs = w.ds + H + NDT;                                   // two planes [ZP >= Tr - 1 + NDT]: zr, zi of the carried and the new d's
  w.ys = reinterpret_cast<f2_t*>(smem + 4 * (size_t)p.region_words);
  w.hb = reinterpret_cast<float*>(w.ys + NY);
  w.tps = reinterpret_cast<f2_t*>(w.hb + ((H + 3) & ~3u));
  float* gs = reinterpret_cast<float*>(w.tps + ((P + 1) & ~1u));
  w.hs = gs + ((Tr + 3) & ~3u);
  front_begin(p, w);
  float* zb = w.hs + w.T;                                       // the last Tr - 1 (zr, zi), plane by plane, for the next step
  const int tid = w.tid, nthr = w.nthr, lo = (int)(w.blk * p.span);
  const uint32_t s = w.s;
  const float* ds = w.ds;
  rds_taps_to_lds(gs, p.g, Tr, tid, nthr);
  uint32_t cnt = 0;

  front_walk(p, w, [&](int a, int b, bool full) {
    front_d_stage(p, w, a, b);
    if (full) {
      const int n = b - a;
      const bool first = a == lo;
      // ---- pilot filter, carrier, z: plane index o stands for m = a - (Tr - 1) + o, its pilot window is ds[o .. o + P).  The span's first
      //      step computes all of [0, C); a later one takes the first Tr - 1 from the step before and computes the new d's only
      const int C = n + (int)Tr - 1, O0 = first ? 0 : (int)Tr - 1;
      if (!first) rds_tail_restore(zs, zb, Tr, ZP, tid, nthr);
      front_pilot(w, O0, C, [&](int o, f2_t q) __attribute__((always_inline)) {
        float zr, zi;
        const bool on = carrier_rds(p.pmin2, p.rds_gain, q, ds[o + Dl], zr, zi);
        zs[o] = zr;
        zs[ZP + o] = zi;
        cnt += (on && o >= (int)Tr - 1) ? 1u : 0u;
      });
      __syncthreads();
      // ---- output: the j's whose newest d lies in [a, b), their chains shared among all the waves
      const int2 jr = step_outputs(a, b, p.f0, (int)Dr, (int)p.A);
      rds_chains(zs, gs, Tr, Dr, ZP, p.f0, a, jr.x, jr.y > jr.x ? jr.y - jr.x : 0, nthr / 64, tid >> 6, tid & 63, p.bb + (size_t)s * p.bb_stride);
      rds_tail_save(zb, zs, n, Tr, ZP, tid, nthr);
    }
    __syncthreads();
  });

  front_count(p, s, tid, cnt);
  front_hand_over(p, w);
}

}  // namespace

// =================================================================================================================
//  Host side: handle, argument checks (all before any device work), launch geometry.  The walk's state is the header's PilotFront.
// =================================================================================================================
struct sdrfm_rds {
  sdrfm_rds_config cfg;                        // taps pointers point at the copies in f and below
  PilotFront f;
  Decim rd;                                    // the RDS decimator
  float* d_bb = nullptr;
  size_t d_bb_stride = 0;
  bool fast = false;
  FrontStep step;                              // of the kernel this handle launches
  uint32_t slots = 1;                          // workgroups the device runs at a time (compute units x workgroups per unit)
  char kernel_name[96];
};

namespace {

// LDS bytes of a step geometry (see the layout in k_rds)
size_t rds_lds(uint32_t T, uint32_t D, uint32_t P, uint32_t Tr, uint32_t H, uint32_t NY, uint32_t NDT, uint32_t* region_words) {
  const size_t nx = (size_t)(NY - 1) * D + T + 4, nds = (size_t)H + NDT + 2 * (size_t)rds_zplane(Tr, NDT);
  size_t rw = nx > nds ? nx : nds;
  rw = (rw + 3) & ~(size_t)3;
  if (region_words) *region_words = (uint32_t)rw;
  return 4 * rw + 8 * (size_t)NY + 4 * (size_t)((H + 3) & ~3u) + 8 * (size_t)((P + 1) & ~1u) + 4 * (size_t)((Tr + 3) & ~3u) + 4 * (size_t)T +
         8 * (size_t)(Tr - 1);
}

void rds_free(sdrfm_rds* h) {
  if (!h) return;
  front_free(h->f);
  decim_free(h->rd);
  (void)hipFree(h->d_bb);
  delete h;
}

}  // namespace

extern "C" {

int sdrfm_rds_create(const sdrfm_rds_config* cfg, sdrfm_rds_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!cfg || cfg->struct_size != sizeof(sdrfm_rds_config)) return SDRFM_EINVAL;
  if (!front_config_ok(cfg->n_streams, cfg->fir_taps, cfg->fir_decim, cfg->fir_coeffs, cfg->pilot_taps, cfg->pilot_coeffs, cfg->pilot_min))
    return SDRFM_EINVAL;
  if (cfg->flags & ~SDRFM_RDS_CFG_FORCE_GENERIC) return SDRFM_EINVAL;
  if (!decim_config_ok(cfg->rds_taps, cfg->rds_decim, cfg->rds_coeffs, cfg->rds_gain)) return SDRFM_EINVAL;
  hipDeviceProp_t prop;
  int rc = front_open_device(cfg->device, &prop);
  if (rc != SDRFM_OK) return rc;

  sdrfm_rds* h = new (std::nothrow) sdrfm_rds();
  if (!h) return SDRFM_ENOMEM;
  h->cfg = *cfg;
  const uint32_t T = cfg->fir_taps, D = cfg->fir_decim, P = cfg->pilot_taps, Tr = cfg->rds_taps, Dr = cfg->rds_decim, H = P - 1 + Tr - 1;
  const size_t ns = cfg->n_streams;
  rc = front_alloc(h->f, cfg->n_streams, T, D, cfg->fir_coeffs, P, cfg->pilot_coeffs, cfg->pilot_min, H, cfg->max_bytes_per_call, cfg->device);
  if (rc != SDRFM_OK) { rds_free(h); return rc; }
  rc = decim_alloc(h->rd, h->f, Tr, Dr, cfg->rds_coeffs);
  if (rc != SDRFM_OK) { rds_free(h); return rc; }
  h->cfg.fir_coeffs = h->f.hc;
  h->cfg.rds_coeffs = h->rd.gc;
  h->cfg.pilot_coeffs = h->f.bc;
  h->d_bb_stride = (2 * (size_t)h->rd.max_out + 63) & ~(size_t)63;
  if (hipMalloc(&h->d_bb, sizeof(float) * h->d_bb_stride * ns) != hipSuccess) { rds_free(h); return SDRFM_ENOMEM; }
  h->step = front_step(rds_lds, 64, 10, 101, Tr, H, PF_FAST_NY, PF_FAST_NY - 1);
  h->fast = !(cfg->flags & SDRFM_RDS_CFG_FORCE_GENERIC) && T == 64 && D == 10 && P == 101 && h->step.lds <= PF_LDS_BUDGET;
  if (!h->fast) h->step = front_step_generic(rds_lds, T, D, P, Tr, H);
  if (h->fast) snprintf(h->kernel_name, sizeof h->kernel_name, "rds-fast T64 D10 P101 Tr%u Dr%u", Tr, Dr);
  else snprintf(h->kernel_name, sizeof h->kernel_name, "rds-generic T%u D%u P%u Tr%u Dr%u", T, D, P, Tr, Dr);
  h->slots = front_slots(h->fast ? k_rds<64, 10, 101> : k_rds<0, 0, 0>, h->step.lds, prop);
  rc = sdrfm_rds_reset(h);
  if (rc != SDRFM_OK) { rds_free(h); return rc; }
  *out = h;
  return SDRFM_OK;
}

void sdrfm_rds_destroy(sdrfm_rds_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->f.device);
  (void)hipStreamSynchronize(h->f.stream);
  rds_free(h);
}

int sdrfm_rds_reset(sdrfm_rds_t* h) {
  if (!h) return SDRFM_EINVAL;
  const int rc = front_reset(h->f);
  if (rc != SDRFM_OK) return rc;
  decim_reset(h->rd);
  return SDRFM_OK;
}

int sdrfm_rds_count(const sdrfm_rds_t* h, uint32_t nbytes, uint32_t* n_out) {
  if (!h || !n_out) return SDRFM_EINVAL;
  if (nbytes & 1u) return SDRFM_EODD;
  *n_out = decim_outputs(h->rd, front_new_d(h->f, nbytes));
  return SDRFM_OK;
}

// one call on device buffers, enqueued on the handle's stream
static int rds_enqueue(sdrfm_rds* h, const uint8_t* d_iq, size_t iq_stride, uint32_t nbytes, float* d_bb, size_t bb_stride, uint32_t* d_pc,
                       uint32_t* n_out) {
  const uint32_t ns = h->cfg.n_streams;
  if (h->step.lds > PF_LDS_BUDGET) return SDRFM_FAIL;            // (no shape within the header's limits gets here: NY = 2 fits them all)
  RdsParams p;
  memset(&p, 0, sizeof p);
  front_fill(h->f, p, d_iq, iq_stride, nbytes, d_pc, h->step);
  const uint32_t M = p.M, A = decim_outputs(h->rd, M);
  p.bb = d_bb; p.bb_stride = bb_stride;
  p.g = h->rd.d_g;
  p.Tr = h->rd.T; p.Dr = h->rd.D;
  p.rds_gain = h->cfg.rds_gain;
  p.A = A;
  p.f0 = decim_f0(h->rd);
  p.zplane = rds_zplane(p.Tr, p.NDT);
  p.blocks_per_stream = front_split(M, p.NDT, p.H, ns, h->slots);
  p.span = M ? (M + p.blocks_per_stream - 1) / p.blocks_per_stream : 0;
  if (front_zero_count(h->f, d_pc, true) != SDRFM_OK) return SDRFM_FAIL;
  const dim3 grid(ns * p.blocks_per_stream), block(PF_THREADS);
  if (h->fast) k_rds<64, 10, 101><<<grid, block, h->step.lds, h->f.stream>>>(p);
  else k_rds<0, 0, 0><<<grid, block, h->step.lds, h->f.stream>>>(p);
  if (hipGetLastError() != hipSuccess) return SDRFM_FAIL;
  front_advance(h->f, p.N);
  decim_advance(h->rd, M);
  *n_out = A;
  return SDRFM_OK;
}

int sdrfm_rds_process_batch(sdrfm_rds_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, float* bb, size_t bb_stride,
                            uint32_t* pilot_count, uint32_t* n_out, uint32_t flags) {
  if (!h || !n_out) return SDRFM_EINVAL;
  if (flags & ~SDRFM_F_DEVICE_PTRS) return SDRFM_EINVAL;       // SDRFM_F_OVERLAP: not for this handle
  if (nbytes & 1u) return SDRFM_EODD;
  if (nbytes > h->f.max_bytes) return SDRFM_ECAPACITY;
  const uint32_t ns = h->cfg.n_streams;
  if (nbytes == 0) {
    *n_out = 0;
    return front_empty_call(h->f, pilot_count, flags);
  }
  if (!iq) return SDRFM_EINVAL;
  if (ns > 1 && iq_stride < nbytes) return SDRFM_ECAPACITY;
  uint32_t A = 0;
  (void)sdrfm_rds_count(h, nbytes, &A);
  if (A && !bb) return SDRFM_EINVAL;
  if (ns > 1 && bb_stride < 2 * (size_t)A) return SDRFM_ECAPACITY;
  if (hipSetDevice(h->f.device) != hipSuccess) return SDRFM_FAIL;
  if (flags & SDRFM_F_DEVICE_PTRS) return rds_enqueue(h, iq, iq_stride, nbytes, bb, bb_stride, pilot_count, n_out);

  if (front_stage_in(h->f, iq, iq_stride, nbytes) != SDRFM_OK) return SDRFM_FAIL;
  const int rc = rds_enqueue(h, h->f.d_iq, h->f.d_iq_stride, nbytes, h->d_bb, h->d_bb_stride, h->f.d_pc, n_out);
  if (rc != SDRFM_OK) return rc;
  if (front_copy_back(h->f, bb, bb_stride, h->d_bb, h->d_bb_stride, 2 * (size_t)A) != SDRFM_OK) return SDRFM_FAIL;
  return front_finish(h->f, pilot_count);
}

int sdrfm_rds_set_stream(sdrfm_rds_t* h, void* hip_stream) {
  if (!h) return SDRFM_EINVAL;
  return front_use_stream(h->f, hip_stream);
}

int sdrfm_rds_synchronize(sdrfm_rds_t* h) {
  if (!h) return SDRFM_EINVAL;
  if (hipSetDevice(h->f.device) != hipSuccess || hipStreamSynchronize(h->f.stream) != hipSuccess) return SDRFM_FAIL;
  return SDRFM_OK;
}

const char* sdrfm_rds_kernel_name(const sdrfm_rds_t* h) { return h ? h->kernel_name : ""; }

}  // extern "C"
