/*
 * sdrfm_bcast.hip — the broadcast receiver behind the sdrfm_bcast_* C-ABI (include/sdrfm.h): the stereo handle's L and R
 * and the RDS handle's baseband of the same streams from one launch, bit for bit what sdrfm_stereo.hip and sdrfm_rds.hip give.
 *
 * The walk from the input bytes to the pilot filter's q = b * d is sdrfm_pilot_front.h's and runs once per d.  Behind q both carriers of
 * sdrfm_carrier.h are taken from the same q: s (the stereo difference signal) and zr, zi (the RDS subcarrier mixed down) -> LDS, the gate
 * counted once.  Behind one barrier the audio chains of k_stereo (am on d delayed by Δ, as on s; L = am + as, R = am - as) and the
 * output chains of k_rds (wr, wi: z in two odd-length planes, taps oldest first, 16 z's and taps read ahead of their 16 fmaf's): the
 * functions of sdrfm_out_stages.h, which those two kernels call as well.
 * H = P - 1 + max(Ta, Tr) - 1.  Both tails are carried from step to step in LDS — the last Ta - 1 s's and the last Tr - 1 z's of both
 * planes — so the pilot filter runs once per d and a step takes NY - 1 new d's whatever Ta and Tr are; the span's first step computes
 * the tails before it (that is what the halo's d's are for).  s and z are pure functions of d and q, so carrying them changes no bit.
 * The waves of a workgroup run in lockstep over their lanes, so a chain hides another only from wave to wave: every step gives the RDS
 * chains to some of the waves and the audio outputs to the others where that is the shorter way (bcast_rds_waves).
 *
 * k_bcast<0, 0, 0> and k_bcast<64, 10, 101> are the header's two forms of the walk; the carriers and the chains are the same code in both.
 *
 * A tuned handle (sdrfm_bcast_tune) launches the same two with the header's tuned walk: every stream has complex channel
 * taps and a rotation of its own and receives the station at that offset of its input — or of row 0 of the input, which all streams
 * then share.  Only K2 and K3 differ; everything behind d is the code above.
 *
 * A metered call (sdrfm_bcast_process_batch_metered) launches the fifth template argument's form of either: the same walk
 * and the same outputs, and every new d besides handed to sdrfm_meter.h's meter stage where its y, the d itself and the q of the pilot
 * window that ends at it are in LDS and registers anyway — the scan handle's record of the stream, from the launch that receives it.
 *
 * A re-tune (sdrfm_bcast_retune) replaces the taps and rotations between two calls and keeps the streams running:
 * k_bcast_retune rewrites the current set of the carried state in place — the carried y turned by the caller's carry, the carried d's
 * re-referenced to the new rotation, or all three kinds zeroed for a stream that restarts — and k_bcast is not touched.
 *
 * A conditioned handle (sdrfm_bcast_set_audio) launches the sixth template argument's form of any of those: the same walk,
 * carriers and chains, and where L and R are formed the stream's stereo blend and output gain, both ramped per audio output by
 * sdrfm_audio_ctl.h's closed form from one small record per stream — values, not carried state, so nothing new is handed over.
 *
 * A hist call (sdrfm_bcast_process_batch_metered_hist) launches the seventh template argument's form of a metered kernel:
 * beside meter_take every new d counted in sdrfm_hist.h's 512 bins, which lie in LDS behind the plain layout — the scan handle's histogram
 * row of the stream, from the launch that receives it.  The bins shorten the step at the LDS-limited shapes; no result depends on the step.
 */
#include <new>

#include "sdrfm_carrier.h"
#include "sdrfm_hist.h"
#include "sdrfm_meter.h"
#include "sdrfm_out_stages.h"
#include "sdrfm_pilot_front.h"
#include "sdrfm_sink_stereo.h"

namespace {

struct BcastParams : FrontParams {
  float* left;
  float* right;
  size_t audio_stride;
  float* bb;                   // [ns][bb_stride]: (wr, wi) pairs
  size_t bb_stride;
  const float* ga;             // Ta
  const float* gr;             // Tr
  uint32_t Ta, Da, Tr, Dr;
  float diff_gain, rds_gain;
  uint32_t Aa, Ar;             // outputs of the call
  int32_t f0a, f0r;            // the newest d of output 0 of either decimator
  uint32_t zplane;             // words of one z plane: Tr - 1 + NDT, made odd
  const float* ctaps;          // tuned: [ns][2T], (hr[k], hi[k]) pairs
  const float* rot;            // tuned: [ns]
  unsigned long long* meters;  // metered: [ns][8], sdrfm_scan_meter as eight 64-bit words, zeroed before the launch
  const AudioCtlRec* actl;     // blended: [ns], the streams' ramps
  uint32_t slew, J;            // blended: the ramps' units per audio output, the audio outputs between the set and this call
  uint32_t* hist;              // hist: [ns][hist_stride], a row's first SDRFM_SCAN_HIST_BINS words, zeroed before the launch
  size_t hist_stride;          // words
};

// how many of a workgroup's nw waves take a step's nc RDS chains (of Tr links), the others taking its na audio outputs (of 2 Ta links):
// the count with the shortest longer side; nw = every wave takes its share of both, one after the other, where no split beats that
__device__ __forceinline__ int bcast_rds_waves(int nw, int nc, int Tr, int na, int Ta) {
  int wr = nw, best = cdiv(nc, 64 * nw) * Tr + cdiv(na, 64 * nw) * 2 * Ta;
  for (int r = 1; r < nw; ++r) {
    const int tr = cdiv(nc, 64 * r) * Tr, ta = cdiv(na, 64 * (nw - r)) * 2 * Ta, t = tr > ta ? tr : ta;
    if (t < best) { best = t; wr = r; }
  }
  return wr;
}

template <int FT, int FD, int FP, bool TU, bool ME = false, bool BL = false, bool HI = false>
__global__ void __launch_bounds__(PF_THREADS) k_bcast(BcastParams p) {
  static_assert(ME || !HI, "the histogram counts the d's the meter stage takes");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t T = FT > 0 ? FT : p.T, P = FT > 0 ? FP : p.P;
  const uint32_t Ta = p.Ta, Da = p.Da, Tr = p.Tr, Dr = p.Dr, H = p.H, Dl = p.Dl, NY = p.NY, NDT = p.NDT, ZP = p.zplane;
  const int Tm = (int)(Ta > Tr ? Ta : Tr), oa = Tm - (int)Ta, oz = Tm - (int)Tr;
  // LDS: region (x as f16 pairs | d's, s's, zr's, zi's) | ys[NY] | hb[H] | tps[P] | grs[Tr] | gas[Ta] | hs[T; tuned: 2T] | zb[2 (Tr - 1)] | sb[Ta - 1];
  // hb and tps padded so that grs starts on 16 bytes.  grs holds the RDS taps oldest first (grs[k] = gr[Tr - 1 - k]): the output chains
  // read them four at a time
  // (a metered kernel adds nothing to it: y, d and q of a new d are there already; a hist kernel adds bins[SDRFM_SCAN_HIST_BINS] on the next
  // 16 bytes behind sb)
  FrontWg<FT, FD, FP, TU> w;
  w.xs = reinterpret_cast<h2_t*>(smem);
  w.ds = reinterpret_cast<float*>(smem);
  float* ss = w.ds + H + NDT;                                   // [Ta - 1 + NDT]: s of the carried and the new d's
  float* zs = ss + (Ta - 1 + NDT);                              // two planes [ZP >= Tr - 1 + NDT]: zr, zi likewise
  w.ys = reinterpret_cast<f2_t*>(smem + 4 * (size_t)p.region_words);
  w.hb = reinterpret_cast<float*>(w.ys + NY);
  w.tps = reinterpret_cast<f2_t*>(w.hb + ((H + 3) & ~3u));
  float* grs = reinterpret_cast<float*>(w.tps + ((P + 1) & ~1u));
  float* gas = grs + ((Tr + 3) & ~3u);
  w.hs = gas + Ta;
  float* zb = w.hs + (TU ? 2 * T : T);                                        // the last Tr - 1 (zr, zi), plane by plane, for the next step
  float* sb = zb + 2 * (Tr - 1);                                // the last Ta - 1 s's
  uint32_t* bins = nullptr;                                     // hist: the workgroup's counts
  if constexpr (HI) bins = reinterpret_cast<uint32_t*>(smem + hist_bins_offset((size_t)(reinterpret_cast<unsigned char*>(sb + (Ta - 1)) - smem)));
  if constexpr (TU) {
    const uint32_t st = blockIdx.x / p.blocks_per_stream;
    w.ctaps = p.ctaps + (size_t)st * 2 * T;
    w.rot = p.rot[st];
  }
  front_begin(p, w);
  const int tid = w.tid, nthr = w.nthr, lo = (int)(w.blk * p.span);
  const uint32_t s = w.s;
  const float* ds = w.ds;
  rds_taps_to_lds(grs, p.gr, Tr, tid, nthr);
  for (int k = tid; k < (int)Ta; k += nthr) gas[k] = p.ga[k];
  AudioBlend bl;                                                // blended: the stream's ramps
  if constexpr (BL) {
    bl.rec = p.actl[s];
    bl.slew = p.slew;
    bl.J = p.J;
  }
  uint32_t cnt = 0;
  MeterAcc acc;                                                 // metered: the lane's sums, and the gate's count in place of cnt
  if constexpr (HI) {
    hist_zero(bins, tid);
    __syncthreads();
  }

  front_walk(p, w, [&](int a, int b, bool full) {
    front_d_stage(p, w, a, b);
    if (full) {
      const int n = b - a;
      const bool first = a == lo;
      // ---- pilot filter, both carriers: index o stands for m = a - (Tm - 1) + o, its pilot window is ds[o .. o + P); s of m lies at
      //      ss[o - oa], z at zs[o - oz].  The span's first step computes all of [0, C); a later one takes the tails from the step before
      //      and computes the new d's only
      const int C = n + Tm - 1, O0 = first ? 0 : Tm - 1;
      const int yo = a - (a - 1 > 0 ? a - 1 : 0);                 // metered: y of the new d a + j lies at ys[j + yo]
      if (!first) {
        rds_tail_restore(zs, zb, Tr, ZP, tid, nthr);
        for (int k = tid; k < (int)Ta - 1; k += nthr) ss[k] = sb[k];
      }
      front_pilot(w, O0, C, [&](int o, f2_t q) __attribute__((always_inline)) {
        const float dd = ds[o + Dl];
        float sv, zr, zi;
        const bool on = carrier_stereo(p.pmin2, p.diff_gain, q, dd, sv);
        carrier_rds(p.pmin2, p.rds_gain, q, dd, zr, zi);
        if (o >= oa) ss[o - oa] = sv;
        if (o >= oz) {
          zs[o - oz] = zr;
          zs[(int)ZP + o - oz] = zi;
        }
        if constexpr (ME) {
          // the new d m = a + j, j = o - (Tm - 1): the UNDELAYED d ds[H + j], at which o's pilot window ends (H = P - 1 + Tm - 1).  The
          // tails a span's first step recomputes (o < Tm - 1) belong to d's before the span: another workgroup's, or an earlier call's
          if (o >= Tm - 1) {
            const int j = o - (Tm - 1);
            meter_take(acc, w.ys[j + yo], ds[H + j], q, p.pmin2);
            if constexpr (HI) hist_take(bins, ds[H + j]);
          }
        } else {
          cnt += (on && o >= Tm - 1) ? 1u : 0u;
        }
      });
      __syncthreads();
      // ---- the outputs whose newest d lies in [a, b): nja audio outputs from ja.x, njr RDS outputs from jr.x as 2 njr chains (the re ones first)
      const int2 ja = step_outputs(a, b, p.f0a, (int)Da, (int)p.Aa), jr = step_outputs(a, b, p.f0r, (int)Dr, (int)p.Ar);
      const int nja = ja.y > ja.x ? ja.y - ja.x : 0, njr = jr.y > jr.x ? jr.y - jr.x : 0;
      const int nw = nthr / 64, wv = tid >> 6, ln = tid & 63;
      const int wr = bcast_rds_waves(nw, 2 * njr, (int)Tr, nja, (int)Ta);
      const int wa0 = wr < nw ? wr : 0, wa = nw - wa0;            // the audio waves: [wa0, nw)
      if (wv < wr) rds_chains(zs, grs, Tr, Dr, ZP, p.f0r, a, jr.x, njr, wr, wv, ln, p.bb + (size_t)s * p.bb_stride);
      if (wv >= wa0)                                              // one output per lane of the waves that take them
        audio_outputs<BL>(ds, ss, gas, Ta, Da, p.f0a, a, H, Dl, ja.x + (wv - wa0) * 64 + ln, 64 * wa, ja.y, p.left + (size_t)s * p.audio_stride,
                          p.right + (size_t)s * p.audio_stride, &bl);
      rds_tail_save(zb, zs, n, Tr, ZP, tid, nthr);                // the tails, for the next step
      for (int k = tid; k < (int)Ta - 1; k += nthr) sb[k] = ss[n + k];
    }
    __syncthreads();
  });

  if constexpr (ME) {
    front_count(p, s, tid, acc.on);                             // the same comparison on the same pw as the carriers' gate
    meter_flush(acc, p.meters + 8 * (size_t)s, tid);
    if constexpr (HI) {
      __syncthreads();
      hist_flush(bins, p.hist + (size_t)s * p.hist_stride, tid);
    }
  } else {
    front_count(p, s, tid, cnt);
  }
  front_hand_over(p, w);
}

// ---- the re-tune's transform of the carried state.  One record per stream, made by the host: what to do and with what
struct RetuneOp {
  float cr, ci;                // the carry: yprev' = yprev (cr + j ci)
  float sh;                    // the shift: hist_d' = hist_d + sh (rot_old - rot_new, wrapped once)
  uint32_t mode;               // RT_*
};
constexpr uint32_t RT_RESTART = 1, RT_CARRY = 2, RT_SHIFT = 4;
constexpr uint32_t RT_STREAMS = PF_THREADS / 64;               // streams per workgroup: a wave each

// in place on the current state set: per stream one float2, H floats and, for a restart, T - 1 float2's
__global__ void __launch_bounds__(PF_THREADS) k_bcast_retune(const RetuneOp* ops, float2* hist_x, float2* yprev, float* hist_d, uint32_t ns, uint32_t T,
                                                             uint32_t H) {
  const uint32_t s = blockIdx.x * RT_STREAMS + threadIdx.x / 64, ln = threadIdx.x & 63;
  if (s >= ns) return;
  const RetuneOp op = ops[s];
  float2* hx = hist_x + (size_t)s * (T - 1);
  float* hd = hist_d + (size_t)s * H;
  if (op.mode & RT_RESTART) {                                   // the stream whose earlier x were all 0
    for (uint32_t k = ln; k + 1 < T; k += 64) hx[k] = make_float2(0.0f, 0.0f);
    for (uint32_t k = ln; k < H; k += 64) hd[k] = 0.0f;
    if (ln == 0) yprev[s] = make_float2(0.0f, 0.0f);
    return;
  }
  if ((op.mode & RT_CARRY) && ln == 0) {
    const float2 y = yprev[s];
    const float t = y.y * op.ci, u = y.y * op.cr;                // (the TU is built with -ffp-contract=off: two rounded products)
    yprev[s] = make_float2(__builtin_fmaf(y.x, op.cr, -t), __builtin_fmaf(y.x, op.ci, u));
  }
  if (op.mode & RT_SHIFT)
    for (uint32_t k = ln; k < H; k += 64) hd[k] = hd[k] + op.sh;
}

}  // namespace

// =================================================================================================================
//  Host side: handle, argument checks (all before any device work), launch geometry.  The walk's state is the header's PilotFront.
//  bcast_kernel names the twenty-four instantiations, once; a BcastForm for the untuned and one for the tuned kernels holds what a launch
//  looks up (step, slots, name); the four process_batch entries are one call path (bcast_batch), tune and retune one installation.
// =================================================================================================================
typedef void (*bcast_kernel_fn)(BcastParams);

// what the untuned and the tuned kernels each have of their own
struct BcastForm {
  FrontStep step;                              // of the kernels of this form
  bool fast = false;
  uint32_t slots[2][2] = {{1, 1}, {1, 1}};     // [metered][blend]: workgroups the device runs at a time (compute units x workgroups per unit)
  char name[2][120];                           // [blend]
  // the hist kernels' own: the bins take LDS from the step at the LDS-limited shapes
  FrontStep hist_step;
  bool hist_fast = false;
  uint32_t hist_slots[2] = {1, 1};             // [blend]
  char hist_name[2][128];                      // [blend]
};

struct sdrfm_bcast {
  sdrfm_bcast_config cfg;                      // taps pointers point at the copies in f and below
  PilotFront f;
  Decim au, rd;                                // the audio and the RDS decimator, their phases carried separately
  float* d_left = nullptr;
  float* d_right = nullptr;
  size_t d_audio_stride = 0;
  float* d_bb = nullptr;
  size_t d_bb_stride = 0;
  BcastForm form[2];                           // [tuned]
  // the tuned form (sdrfm_bcast_tune): the taps and rotations the handle was last tuned with
  bool tuned = false, shared_input = false;
  float* d_ctaps = nullptr;                    // [ns][2T]
  float* d_rot = nullptr;                      // [ns]
  float* rot_host = nullptr;                   // [ns]: the rotations the device holds, 0 on an untuned handle (a re-tune's rot_old)
  // the re-tune (sdrfm_bcast_retune): its per-stream records, the host's and the device's
  RetuneOp* ops_host = nullptr;
  RetuneOp* d_ops = nullptr;
  // the metered form (sdrfm_bcast_process_batch_metered): whether the taps keep a record inside int64 — the pilot taps and the untuned
  // channel taps looked at at create, the tuned ones at tune
  bool meter_ok = false, meter_ok_tuned = false;
  sdrfm_scan_meter* d_meters = nullptr;        // host-buffer calls: the records [ns]
  uint32_t* d_hist = nullptr;                  // host-buffer hist calls: the rows [ns][512], allocated at the first such call
  // the conditioned form (sdrfm_bcast_set_audio): the streams' ramps on the host and, from the first set on, on the device; the handle's
  // slew and the audio outputs since the last set (saturated)
  bool blend = false;
  AudioCtlRec* actl_host = nullptr;
  AudioCtlRec* d_actl = nullptr;
  uint32_t slew = SDRFM_ACTL_ONE, J = SDRFM_ACTL_J_MAX;
};

namespace {

// LDS bytes of a step geometry (see the layout in k_bcast); the header's Tg carries both lengths: Ta in the upper half, Tr in the lower
uint32_t bcast_tg(uint32_t Ta, uint32_t Tr) { return (Ta << 16) | Tr; }

size_t bcast_lds(uint32_t T, uint32_t D, uint32_t P, uint32_t Tg, uint32_t H, uint32_t NY, uint32_t NDT, uint32_t* region_words) {
  const uint32_t Ta = Tg >> 16, Tr = Tg & 0xffffu;
  const size_t nx = (size_t)(NY - 1) * D + T + 4, nds = (size_t)H + NDT + (Ta - 1 + NDT) + 2 * (size_t)rds_zplane(Tr, NDT);
  size_t rw = nx > nds ? nx : nds;
  rw = (rw + 3) & ~(size_t)3;
  if (region_words) *region_words = (uint32_t)rw;
  return 4 * rw + 8 * (size_t)NY + 4 * (size_t)((H + 3) & ~3u) + 8 * (size_t)((P + 1) & ~1u) + 4 * (size_t)((Tr + 3) & ~3u) + 4 * (size_t)Ta +
         4 * (size_t)T + 8 * (size_t)(Tr - 1) + 4 * (size_t)(Ta - 1);
}

// the tuned kernels keep both tap sets in LDS: T more words
size_t bcast_lds_tuned(uint32_t T, uint32_t D, uint32_t P, uint32_t Tg, uint32_t H, uint32_t NY, uint32_t NDT, uint32_t* region_words) {
  return bcast_lds(T, D, P, Tg, H, NY, NDT, region_words) + 4 * (size_t)T;
}

// the hist kernels' LDS: the plain layout (rounded up to 16) and the bins
size_t bcast_hist_lds(uint32_t T, uint32_t D, uint32_t P, uint32_t Tg, uint32_t H, uint32_t NY, uint32_t NDT, uint32_t* region_words) {
  return hist_bins_offset(bcast_lds(T, D, P, Tg, H, NY, NDT, region_words)) + HIST_LDS_BYTES;
}

size_t bcast_hist_lds_tuned(uint32_t T, uint32_t D, uint32_t P, uint32_t Tg, uint32_t H, uint32_t NY, uint32_t NDT, uint32_t* region_words) {
  return hist_bins_offset(bcast_lds_tuned(T, D, P, Tg, H, NY, NDT, region_words)) + HIST_LDS_BYTES;
}

// the twenty-four kernels: the sixteen of the plain and the metered calls, the eight of the hist call (all metered)
bcast_kernel_fn bcast_kernel(bool fast, bool tuned, bool metered, bool blend, bool hist = false) {
  static const bcast_kernel_fn kh[2][2][2] = {                   // [tuned][blend][fast]
      {{k_bcast<0, 0, 0, false, true, false, true>, k_bcast<64, 10, 101, false, true, false, true>},
       {k_bcast<0, 0, 0, false, true, true, true>, k_bcast<64, 10, 101, false, true, true, true>}},
      {{k_bcast<0, 0, 0, true, true, false, true>, k_bcast<64, 10, 101, true, true, false, true>},
       {k_bcast<0, 0, 0, true, true, true, true>, k_bcast<64, 10, 101, true, true, true, true>}}};
  if (hist) return kh[tuned][blend][fast];
  static const bcast_kernel_fn k[2][2][2][2] = {                 // [tuned][metered][blend][fast]
      {{{k_bcast<0, 0, 0, false, false, false>, k_bcast<64, 10, 101, false, false, false>},
        {k_bcast<0, 0, 0, false, false, true>, k_bcast<64, 10, 101, false, false, true>}},
       {{k_bcast<0, 0, 0, false, true, false>, k_bcast<64, 10, 101, false, true, false>},
        {k_bcast<0, 0, 0, false, true, true>, k_bcast<64, 10, 101, false, true, true>}}},
      {{{k_bcast<0, 0, 0, true, false, false>, k_bcast<64, 10, 101, true, false, false>},
        {k_bcast<0, 0, 0, true, false, true>, k_bcast<64, 10, 101, true, false, true>}},
       {{k_bcast<0, 0, 0, true, true, false>, k_bcast<64, 10, 101, true, true, false>},
        {k_bcast<0, 0, 0, true, true, true>, k_bcast<64, 10, 101, true, true, true>}}}};
  return k[tuned][metered][blend][fast];
}

// every ramp at its target: what a restart of the streams leaves of the conditioning (the settings stay)
void bcast_ramps_complete(sdrfm_bcast* h) { h->J = SDRFM_ACTL_J_MAX; }

void bcast_free(sdrfm_bcast* h) {
  if (!h) return;
  front_free(h->f);
  decim_free(h->au); decim_free(h->rd);
  (void)hipFree(h->d_left); (void)hipFree(h->d_right); (void)hipFree(h->d_bb);
  (void)hipFree(h->d_ctaps); (void)hipFree(h->d_rot); (void)hipFree(h->d_meters); (void)hipFree(h->d_ops); (void)hipFree(h->d_actl);
  (void)hipFree(h->d_hist);
  free(h->rot_host); free(h->ops_host); free(h->actl_host);
  delete h;
}

}  // namespace

extern "C" {

int sdrfm_bcast_create(const sdrfm_bcast_config* cfg, sdrfm_bcast_t** out) {
  if (!out) return SDRFM_EINVAL;
  *out = nullptr;
  if (!cfg || cfg->struct_size != sizeof(sdrfm_bcast_config)) return SDRFM_EINVAL;
  if (!front_config_ok(cfg->n_streams, cfg->fir_taps, cfg->fir_decim, cfg->fir_coeffs, cfg->pilot_taps, cfg->pilot_coeffs, cfg->pilot_min))
    return SDRFM_EINVAL;
  if (cfg->flags & ~SDRFM_BCAST_CFG_FORCE_GENERIC) return SDRFM_EINVAL;
  if (!decim_config_ok(cfg->audio_taps, cfg->audio_decim, cfg->audio_coeffs, cfg->diff_gain)) return SDRFM_EINVAL;
  if (!decim_config_ok(cfg->rds_taps, cfg->rds_decim, cfg->rds_coeffs, cfg->rds_gain)) return SDRFM_EINVAL;
  hipDeviceProp_t prop;
  int rc = front_open_device(cfg->device, &prop);
  if (rc != SDRFM_OK) return rc;

  sdrfm_bcast* h = new (std::nothrow) sdrfm_bcast();
  if (!h) return SDRFM_ENOMEM;
  h->cfg = *cfg;
  const uint32_t T = cfg->fir_taps, D = cfg->fir_decim, P = cfg->pilot_taps, Ta = cfg->audio_taps, Da = cfg->audio_decim;
  const uint32_t Tr = cfg->rds_taps, Dr = cfg->rds_decim, H = P - 1 + (Ta > Tr ? Ta : Tr) - 1;
  const size_t ns = cfg->n_streams;
  rc = front_alloc(h->f, cfg->n_streams, T, D, cfg->fir_coeffs, P, cfg->pilot_coeffs, cfg->pilot_min, H, cfg->max_bytes_per_call, cfg->device);
  if (rc != SDRFM_OK) { bcast_free(h); return rc; }
  rc = decim_alloc(h->au, h->f, Ta, Da, cfg->audio_coeffs);
  if (rc == SDRFM_OK) rc = decim_alloc(h->rd, h->f, Tr, Dr, cfg->rds_coeffs);
  if (rc != SDRFM_OK) { bcast_free(h); return rc; }
  h->cfg.fir_coeffs = h->f.hc;
  h->cfg.pilot_coeffs = h->f.bc;
  h->cfg.audio_coeffs = h->au.gc;
  h->cfg.rds_coeffs = h->rd.gc;
  h->d_audio_stride = ((size_t)h->au.max_out + 63) & ~(size_t)63;
  h->d_bb_stride = (2 * (size_t)h->rd.max_out + 63) & ~(size_t)63;
  const size_t audio_bytes = sizeof(float) * h->d_audio_stride * ns;
  if (hipMalloc(&h->d_left, audio_bytes) != hipSuccess || hipMalloc(&h->d_right, audio_bytes) != hipSuccess ||
      hipMalloc(&h->d_bb, sizeof(float) * h->d_bb_stride * ns) != hipSuccess ||
      hipMalloc(&h->d_meters, sizeof(sdrfm_scan_meter) * ns) != hipSuccess || hipMalloc(&h->d_ops, sizeof(RetuneOp) * ns) != hipSuccess) {
    bcast_free(h);
    return SDRFM_ENOMEM;
  }
  h->rot_host = (float*)calloc(ns, sizeof(float));
  h->ops_host = (RetuneOp*)malloc(sizeof(RetuneOp) * ns);
  h->actl_host = (AudioCtlRec*)malloc(sizeof(AudioCtlRec) * ns);
  if (!h->rot_host || !h->ops_host || !h->actl_host) { bcast_free(h); return SDRFM_ENOMEM; }
  for (size_t s = 0; s < ns; ++s) h->actl_host[s] = AudioCtlRec{SDRFM_ACTL_ONE, SDRFM_ACTL_ONE, SDRFM_ACTL_ONE, SDRFM_ACTL_ONE};
  for (int tu = 0; tu < 2; ++tu) {
    BcastForm& f = h->form[tu];
    const front_lds_fn lds = tu ? bcast_lds_tuned : bcast_lds;
    f.step = front_step(lds, 64, 10, 101, bcast_tg(Ta, Tr), H, PF_FAST_NY, PF_FAST_NY - 1);
    f.fast = !(cfg->flags & SDRFM_BCAST_CFG_FORCE_GENERIC) && T == 64 && D == 10 && P == 101 && f.step.lds <= PF_LDS_BUDGET;
    if (!f.fast) f.step = front_step_generic(lds, T, D, P, bcast_tg(Ta, Tr), H);
    snprintf(f.name[0], sizeof f.name[0], "bcast-%s%s T%u D%u P%u Ta%u Da%u Tr%u Dr%u", f.fast ? "fast" : "generic", tu ? "-tuned" : "", T, D, P, Ta,
             Da, Tr, Dr);
    snprintf(f.name[1], sizeof f.name[1], "%s blend", f.name[0]);
    for (int me = 0; me < 2; ++me)
      for (int bl = 0; bl < 2; ++bl) f.slots[me][bl] = front_slots(bcast_kernel(f.fast, tu, me, bl), f.step.lds, prop);
    const front_lds_fn hlds = tu ? bcast_hist_lds_tuned : bcast_hist_lds;
    f.hist_step = front_step(hlds, 64, 10, 101, bcast_tg(Ta, Tr), H, PF_FAST_NY, PF_FAST_NY - 1);
    f.hist_fast = f.fast && f.hist_step.lds <= PF_LDS_BUDGET;
    if (!f.hist_fast) f.hist_step = front_step_generic(hlds, T, D, P, bcast_tg(Ta, Tr), H);
    snprintf(f.hist_name[0], sizeof f.hist_name[0], "bcast-%s%s T%u D%u P%u Ta%u Da%u Tr%u Dr%u + hist", f.hist_fast ? "fast" : "generic",
             tu ? "-tuned" : "", T, D, P, Ta, Da, Tr, Dr);
    snprintf(f.hist_name[1], sizeof f.hist_name[1], "bcast-%s%s T%u D%u P%u Ta%u Da%u Tr%u Dr%u blend + hist", f.hist_fast ? "fast" : "generic",
             tu ? "-tuned" : "", T, D, P, Ta, Da, Tr, Dr);
    for (int bl = 0; bl < 2; ++bl) f.hist_slots[bl] = front_slots(bcast_kernel(f.hist_fast, tu, true, bl, true), f.hist_step.lds, prop);
  }
  h->meter_ok = meter_taps_ok(h->f.hc, 1, T, METER_MAX_CTAP_SUM) && meter_taps_ok(h->f.bc, 1, 2 * P, METER_MAX_PTAP_SUM);
  rc = sdrfm_bcast_reset(h);
  if (rc != SDRFM_OK) { bcast_free(h); return rc; }
  *out = h;
  return SDRFM_OK;
}

void sdrfm_bcast_destroy(sdrfm_bcast_t* h) {
  if (!h) return;
  (void)hipSetDevice(h->f.device);
  (void)hipStreamSynchronize(h->f.stream);
  bcast_free(h);
}

int sdrfm_bcast_reset(sdrfm_bcast_t* h) {
  if (!h) return SDRFM_EINVAL;
  const int rc = front_reset(h->f);
  if (rc != SDRFM_OK) return rc;
  decim_reset(h->au);
  decim_reset(h->rd);
  bcast_ramps_complete(h);
  return SDRFM_OK;
}

int sdrfm_bcast_counts(const sdrfm_bcast_t* h, uint32_t nbytes, uint32_t* n_audio, uint32_t* n_rds) {
  if (!h || !n_audio || !n_rds) return SDRFM_EINVAL;
  if (nbytes & 1u) return SDRFM_EODD;
  const uint64_t M = front_new_d(h->f, nbytes);
  *n_audio = decim_outputs(h->au, M);
  *n_rds = decim_outputs(h->rd, M);
  return SDRFM_OK;
}

static bool bcast_shared(const sdrfm_bcast* h) { return h->tuned && h->shared_input; }

// a host-buffer call's input -> the handle's staging rows; one row where the streams share it
static int bcast_stage_in(const sdrfm_bcast* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes) {
  if (!bcast_shared(h)) return front_stage_in(h->f, iq, iq_stride, nbytes);
  return hipMemcpyAsync(h->f.d_iq, iq, nbytes, hipMemcpyHostToDevice, h->f.stream) == hipSuccess ? SDRFM_OK : SDRFM_FAIL;
}

// one call on device buffers, enqueued on the handle's stream; d_meters: a metered call's records, nullptr for a plain call; d_hist: a hist
// call's rows, nullptr for any other
static int bcast_enqueue(sdrfm_bcast* h, const uint8_t* d_iq, size_t iq_stride, uint32_t nbytes, float* d_left, float* d_right, size_t audio_stride,
                         float* d_bb, size_t bb_stride, uint32_t* d_pc, sdrfm_scan_meter* d_meters, uint32_t* d_hist, size_t hist_stride,
                         uint32_t* n_audio, uint32_t* n_rds) {
  const uint32_t ns = h->cfg.n_streams;
  const BcastForm& form = h->form[h->tuned];
  const bool hist = d_hist != nullptr;
  const FrontStep& step = hist ? form.hist_step : form.step;
  if (step.lds > PF_LDS_BUDGET) return SDRFM_FAIL;               // (no shape within the header's limits gets here: NY = 2 fits them all)
  BcastParams p;
  memset(&p, 0, sizeof p);
  if (h->tuned && h->shared_input) iq_stride = 0;                // every stream reads row 0
  front_fill(h->f, p, d_iq, iq_stride, nbytes, d_pc, step);
  p.ctaps = h->d_ctaps; p.rot = h->d_rot;
  const uint32_t M = p.M, Aa = decim_outputs(h->au, M), Ar = decim_outputs(h->rd, M);
  p.left = d_left; p.right = d_right; p.audio_stride = audio_stride;
  p.bb = d_bb; p.bb_stride = bb_stride;
  p.ga = h->au.d_g; p.gr = h->rd.d_g;
  p.Ta = h->au.T; p.Da = h->au.D; p.Tr = h->rd.T; p.Dr = h->rd.D;
  p.diff_gain = h->cfg.diff_gain;
  p.rds_gain = h->cfg.rds_gain;
  p.Aa = Aa; p.Ar = Ar;
  p.f0a = decim_f0(h->au);
  p.f0r = decim_f0(h->rd);
  p.zplane = rds_zplane(p.Tr, p.NDT);
  p.meters = reinterpret_cast<unsigned long long*>(d_meters);
  p.actl = h->d_actl; p.slew = h->slew; p.J = h->J;
  p.hist = d_hist; p.hist_stride = hist_stride;
  const bool metered = d_meters != nullptr;
  p.blocks_per_stream = front_split(M, p.NDT, p.H, ns, hist ? form.hist_slots[h->blend] : form.slots[metered][h->blend]);   // as the RDS handle chooses them
  p.span = M ? (M + p.blocks_per_stream - 1) / p.blocks_per_stream : 0;
  if (front_zero_count(h->f, d_pc, true) != SDRFM_OK) return SDRFM_FAIL;
  if (d_meters && hipMemsetAsync(d_meters, 0, sizeof(sdrfm_scan_meter) * ns, h->f.stream) != hipSuccess) return SDRFM_FAIL;
  if (hist && hipMemset2DAsync(d_hist, sizeof(uint32_t) * hist_stride, 0, HIST_LDS_BYTES, ns, h->f.stream) != hipSuccess) return SDRFM_FAIL;
  const dim3 grid(ns * p.blocks_per_stream), block(PF_THREADS);
  const bcast_kernel_fn kernel = bcast_kernel(hist ? form.hist_fast : form.fast, h->tuned, metered, h->blend, hist);
  kernel<<<grid, block, step.lds, h->f.stream>>>(p);
  if (hipGetLastError() != hipSuccess) return SDRFM_FAIL;
  front_advance(h->f, p.N);
  decim_advance(h->au, M);
  decim_advance(h->rd, M);
  h->J = audio_ctl_advance(h->J, Aa);
  *n_audio = Aa;
  *n_rds = Ar;
  return SDRFM_OK;
}

// the most bytes per stream a call takes: a metered one at most what keeps its records inside int64
static uint32_t bcast_max_bytes(const sdrfm_bcast* h, bool metered) {
  return metered && h->f.max_bytes > METER_MAX_BYTES ? METER_MAX_BYTES : h->f.max_bytes;
}

// a call of no bytes: no launch, no outputs, the counts, a metered call's records and a hist call's rows are 0
static int bcast_empty_call(const sdrfm_bcast* h, uint32_t* pilot_count, sdrfm_scan_meter* meters, uint32_t* hist, size_t hist_stride, uint32_t flags) {
  const uint32_t ns = h->cfg.n_streams;
  const size_t bytes = sizeof(sdrfm_scan_meter) * ns;
  if (meters && !(flags & SDRFM_F_DEVICE_PTRS)) memset(meters, 0, bytes);
  if (meters && (flags & SDRFM_F_DEVICE_PTRS) &&
      (hipSetDevice(h->f.device) != hipSuccess || hipMemsetAsync(meters, 0, bytes, h->f.stream) != hipSuccess))
    return SDRFM_FAIL;
  for (uint32_t s = 0; hist && !(flags & SDRFM_F_DEVICE_PTRS) && s < ns; ++s) memset(hist + (size_t)s * hist_stride, 0, HIST_LDS_BYTES);
  if (hist && (flags & SDRFM_F_DEVICE_PTRS) &&
      hipMemset2DAsync(hist, sizeof(uint32_t) * hist_stride, 0, HIST_LDS_BYTES, ns, h->f.stream) != hipSuccess)
    return SDRFM_FAIL;
  return front_empty_call(h->f, pilot_count, flags);
}

// a host-buffer call's records back, in stream order before front_finish
static int bcast_meters_back(const sdrfm_bcast* h, sdrfm_scan_meter* meters) {
  if (!meters) return SDRFM_OK;
  const hipError_t e = hipMemcpyAsync(meters, h->d_meters, sizeof(sdrfm_scan_meter) * h->cfg.n_streams, hipMemcpyDeviceToHost, h->f.stream);
  return e == hipSuccess ? SDRFM_OK : SDRFM_FAIL;
}

// a host-buffer hist call's rows back, likewise
static int bcast_hist_back(const sdrfm_bcast* h, uint32_t* hist, size_t hist_stride) {
  if (!hist) return SDRFM_OK;
  const hipError_t e = hipMemcpy2DAsync(hist, sizeof(uint32_t) * hist_stride, h->d_hist, HIST_LDS_BYTES, HIST_LDS_BYTES, h->cfg.n_streams,
                                        hipMemcpyDeviceToHost, h->f.stream);
  return e == hipSuccess ? SDRFM_OK : SDRFM_FAIL;
}

// the four process_batch entries.  sink == nullptr: the plain call.  With a sink, behind the launch on the handle's stream the stereo sink's
// default kernel over this call's L and R rows, which are the handle's own where the caller gives none.  With `meters` the
// metered call of either form: the same checks in the same order, the same launch geometry.  With `hist` besides the hist call of either:
// the same checks again, the hist kernels' step
static int bcast_batch(sdrfm_bcast_t* h, sdrfm_pcm_stereo_sink_t* sink, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, float* left,
                       float* right, size_t audio_stride, int16_t* pcm, size_t pcm_stride, float* bb, size_t bb_stride, uint32_t* pilot_count,
                       sdrfm_scan_meter* meters, uint32_t* hist, size_t hist_stride, uint32_t* n_audio, uint32_t* n_rds, uint32_t flags) {
  if (!h || !n_audio || !n_rds) return SDRFM_EINVAL;
  if (flags & ~SDRFM_F_DEVICE_PTRS) return SDRFM_EINVAL;       // SDRFM_F_OVERLAP: not for this handle
  if (sink && !left != !right) return SDRFM_EINVAL;            // both, or neither: the sink then reads the handle's own rows
  if (nbytes & 1u) return SDRFM_EODD;
  if (nbytes > bcast_max_bytes(h, meters != nullptr)) return SDRFM_ECAPACITY;
  const uint32_t ns = h->cfg.n_streams;
  const bool dev = (flags & SDRFM_F_DEVICE_PTRS) != 0;
  uint32_t Aa = 0, Ar = 0;
  (void)sdrfm_bcast_counts(h, nbytes, &Aa, &Ar);
  int rc = sink ? sdrfm_stereo_sink_check(sink, h->f.device, ns, Aa, pcm, pcm_stride, dev) : SDRFM_OK;
  if (rc != SDRFM_OK) return rc;
  if (nbytes == 0) {
    *n_audio = 0;
    *n_rds = 0;
    return bcast_empty_call(h, pilot_count, meters, hist, hist_stride, flags);
  }
  if (!iq) return SDRFM_EINVAL;
  if (ns > 1 && !bcast_shared(h) && iq_stride < nbytes) return SDRFM_ECAPACITY;
  if (!sink && Aa && (!left || !right)) return SDRFM_EINVAL;
  if (Ar && !bb) return SDRFM_EINVAL;
  if (ns > 1 && ((left && audio_stride < Aa) || bb_stride < 2 * (size_t)Ar)) return SDRFM_ECAPACITY;
  if (hipSetDevice(h->f.device) != hipSuccess) return SDRFM_FAIL;
  if (dev) {
    const bool own = sink && !left;
    float* const l = own ? h->d_left : left;
    float* const r = own ? h->d_right : right;
    const size_t as = own ? h->d_audio_stride : audio_stride;
    rc = bcast_enqueue(h, iq, iq_stride, nbytes, l, r, as, bb, bb_stride, pilot_count, meters, hist, hist_stride, n_audio, n_rds);
    if (rc != SDRFM_OK || !sink) return rc;
    return sdrfm_stereo_sink_launch_on(sink, l, r, as, Aa, pcm, pcm_stride, h->f.stream);
  }

  if (hist && !h->d_hist && hipMalloc(&h->d_hist, (size_t)HIST_LDS_BYTES * ns) != hipSuccess) { h->d_hist = nullptr; return SDRFM_ENOMEM; }
  int16_t* d_pcm = nullptr;
  size_t d_pcm_stride = 0;
  if (sink) rc = sdrfm_stereo_sink_reserve(sink, Aa, &d_pcm, &d_pcm_stride);   // (before anything is enqueued: a refusal leaves both handles alone)
  if (rc != SDRFM_OK) return rc;
  if (bcast_stage_in(h, iq, iq_stride, nbytes) != SDRFM_OK) return SDRFM_FAIL;
  rc = bcast_enqueue(h, h->f.d_iq, h->f.d_iq_stride, nbytes, h->d_left, h->d_right, h->d_audio_stride, h->d_bb, h->d_bb_stride, h->f.d_pc,
                     meters ? h->d_meters : nullptr, hist ? h->d_hist : nullptr, HIST_BINS, n_audio, n_rds);
  if (rc != SDRFM_OK) return rc;
  if (sink) rc = sdrfm_stereo_sink_launch_on(sink, h->d_left, h->d_right, h->d_audio_stride, Aa, d_pcm, d_pcm_stride, h->f.stream);
  if (rc != SDRFM_OK) return rc;
  if (left && front_copy_back(h->f, left, audio_stride, h->d_left, h->d_audio_stride, Aa) != SDRFM_OK) return SDRFM_FAIL;
  if (left && front_copy_back(h->f, right, audio_stride, h->d_right, h->d_audio_stride, Aa) != SDRFM_OK) return SDRFM_FAIL;
  if (front_copy_back(h->f, bb, bb_stride, h->d_bb, h->d_bb_stride, 2 * (size_t)Ar) != SDRFM_OK) return SDRFM_FAIL;
  if (sink && sdrfm_stereo_sink_copy_back(sink, pcm, pcm_stride, Aa, h->f.stream) != SDRFM_OK) return SDRFM_FAIL;
  if (bcast_meters_back(h, meters) != SDRFM_OK) return SDRFM_FAIL;
  if (bcast_hist_back(h, hist, hist_stride) != SDRFM_OK) return SDRFM_FAIL;
  return front_finish(h->f, pilot_count);
}

int sdrfm_bcast_process_batch(sdrfm_bcast_t* h, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, float* left, float* right,
                              size_t audio_stride, float* bb, size_t bb_stride, uint32_t* pilot_count, uint32_t* n_audio, uint32_t* n_rds,
                              uint32_t flags) {
  return bcast_batch(h, nullptr, iq, iq_stride, nbytes, left, right, audio_stride, nullptr, 0, bb, bb_stride, pilot_count, nullptr, nullptr, 0, n_audio,
                     n_rds, flags);
}

int sdrfm_bcast_process_batch_pcm(sdrfm_bcast_t* h, sdrfm_pcm_stereo_sink_t* sink, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, float* left,
                                  float* right, size_t audio_stride, int16_t* pcm, size_t pcm_stride, float* bb, size_t bb_stride,
                                  uint32_t* pilot_count, uint32_t* n_audio, uint32_t* n_rds, uint32_t flags) {
  if (!sink) return SDRFM_EINVAL;                                // (this entry has no plain form)
  return bcast_batch(h, sink, iq, iq_stride, nbytes, left, right, audio_stride, pcm, pcm_stride, bb, bb_stride, pilot_count, nullptr, nullptr, 0, n_audio,
                     n_rds, flags);
}

// either call above with the streams' records from the same launch.  What is the metered call's own is refused first:
// no records to write, PCM without a sink, taps whose sums could leave int64; the form's own checks follow in its own order.  hist: the
// hist call's rows (checked by its entry), nullptr for the metered call
static int bcast_metered(sdrfm_bcast_t* h, sdrfm_pcm_stereo_sink_t* sink, const uint8_t* iq, size_t iq_stride, uint32_t nbytes, float* left,
                         float* right, size_t audio_stride, int16_t* pcm, size_t pcm_stride, float* bb, size_t bb_stride, uint32_t* pilot_count,
                         sdrfm_scan_meter* meters, uint32_t* hist, size_t hist_stride, uint32_t* n_audio, uint32_t* n_rds, uint32_t flags) {
  if (!h || !meters || !n_audio || !n_rds) return SDRFM_EINVAL;
  if (!sink && pcm) return SDRFM_EINVAL;
  if ((uintptr_t)meters % 8 || (uintptr_t)hist % 4) return SDRFM_EINVAL;
  if (!(h->tuned ? h->meter_ok_tuned : h->meter_ok)) return SDRFM_EINVAL;
  return bcast_batch(h, sink, iq, iq_stride, nbytes, left, right, audio_stride, pcm, pcm_stride, bb, bb_stride, pilot_count, meters, hist, hist_stride,
                     n_audio, n_rds, flags);
}

int sdrfm_bcast_process_batch_metered(sdrfm_bcast_t* h, sdrfm_pcm_stereo_sink_t* sink, const uint8_t* iq, size_t iq_stride, uint32_t nbytes,
                                      float* left, float* right, size_t audio_stride, int16_t* pcm, size_t pcm_stride, float* bb, size_t bb_stride,
                                      uint32_t* pilot_count, sdrfm_scan_meter* meters, uint32_t* n_audio, uint32_t* n_rds, uint32_t flags) {
  return bcast_metered(h, sink, iq, iq_stride, nbytes, left, right, audio_stride, pcm, pcm_stride, bb, bb_stride, pilot_count, meters, nullptr, 0,
                       n_audio, n_rds, flags);
}

// the metered call with the streams' deviation histograms from the same launch.  What is the hist call's own is refused
// first, before the handle is read; everything else is the metered call's code
int sdrfm_bcast_process_batch_metered_hist(sdrfm_bcast_t* h, sdrfm_pcm_stereo_sink_t* sink, const uint8_t* iq, size_t iq_stride, uint32_t nbytes,
                                           float* left, float* right, size_t audio_stride, int16_t* pcm, size_t pcm_stride, float* bb,
                                           size_t bb_stride, uint32_t* pilot_count, sdrfm_scan_meter* meters, uint32_t* hist, size_t hist_stride,
                                           uint32_t* n_audio, uint32_t* n_rds, uint32_t flags) {
  if (!h || !meters || !hist || hist_stride < HIST_BINS) return SDRFM_EINVAL;
  return bcast_metered(h, sink, iq, iq_stride, nbytes, left, right, audio_stride, pcm, pcm_stride, bb, bb_stride, pilot_count, meters, hist, hist_stride,
                       n_audio, n_rds, flags);
}

int sdrfm_bcast_set_stream(sdrfm_bcast_t* h, void* hip_stream) {
  if (!h) return SDRFM_EINVAL;
  return front_use_stream(h->f, hip_stream);
}

int sdrfm_bcast_synchronize(sdrfm_bcast_t* h) {
  if (!h) return SDRFM_EINVAL;
  if (hipSetDevice(h->f.device) != hipSuccess || hipStreamSynchronize(h->f.stream) != hipSuccess) return SDRFM_FAIL;
  return SDRFM_OK;
}

const char* sdrfm_bcast_kernel_name(const sdrfm_bcast_t* h) {
  return h ? h->form[h->tuned].name[h->blend] : "";
}

// the kernel a hist call launches now
const char* sdrfm_bcast_hist_kernel_name(const sdrfm_bcast_t* h) {
  return h ? h->form[h->tuned].hist_name[h->blend] : "";
}

// sdrfm_bcast_tune's and sdrfm_bcast_retune's taps and rotations: all finite, every rotation within [-pi, pi]
static bool bcast_tuning_ok(const sdrfm_bcast* h, const float* ctaps, const float* rot) {
  const uint32_t ns = h->cfg.n_streams;
  if (!finite_all(ctaps, ns * 2 * h->f.T) || !finite_all(rot, ns)) return false;
  for (uint32_t s = 0; s < ns; ++s)
    if (std::fabs(rot[s]) > 0x1.921fb6p+1f) return false;
  return true;
}

// checked taps and rotations -> the device (allocated at the first tuning) and the handle's record of its tuning.  Waits for the handle's
// stream: no launch still reads the taps about to be replaced.  The carried state is the caller's to reset or to transform
static int bcast_install_tuning(sdrfm_bcast* h, const float* ctaps, const float* rot, uint32_t flags) {
  const uint32_t ns = h->cfg.n_streams, T = h->f.T;
  if (hipSetDevice(h->f.device) != hipSuccess) return SDRFM_FAIL;
  if (!h->d_ctaps) {
    float *dc = nullptr, *dr = nullptr;
    if (hipMalloc(&dc, sizeof(float) * ns * 2 * T) != hipSuccess || hipMalloc(&dr, sizeof(float) * ns) != hipSuccess) {
      (void)hipFree(dc);
      return SDRFM_ENOMEM;
    }
    h->d_ctaps = dc; h->d_rot = dr;
  }
  if (hipStreamSynchronize(h->f.stream) != hipSuccess) return SDRFM_FAIL;
  if (hipMemcpy(h->d_ctaps, ctaps, sizeof(float) * ns * 2 * T, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->d_rot, rot, sizeof(float) * ns, hipMemcpyHostToDevice) != hipSuccess)
    return SDRFM_FAIL;
  h->tuned = true;
  h->shared_input = (flags & SDRFM_TUNE_SHARED_INPUT) != 0;
  h->meter_ok_tuned = meter_taps_ok(ctaps, ns, 2 * T, METER_MAX_CTAP_SUM) && meter_taps_ok(h->f.bc, 1, 2 * h->f.P, METER_MAX_PTAP_SUM);
  memcpy(h->rot_host, rot, sizeof(float) * ns);
  return SDRFM_OK;
}

int sdrfm_bcast_tune(sdrfm_bcast_t* h, const float* ctaps, const float* rot, uint32_t flags) {
  if (!h) return SDRFM_EINVAL;
  if (!ctaps != !rot) return SDRFM_EINVAL;
  if (flags & ~SDRFM_TUNE_SHARED_INPUT) return SDRFM_EINVAL;
  if (!ctaps) {                                                  // back to the untuned kernels
    if (flags) return SDRFM_EINVAL;
    const int rc = sdrfm_bcast_reset(h);                         // (waits for the handle's stream: no launch reads the taps any more)
    if (rc != SDRFM_OK) return rc;
    h->tuned = h->shared_input = h->meter_ok_tuned = false;
    memset(h->rot_host, 0, sizeof(float) * h->cfg.n_streams);
    return SDRFM_OK;
  }
  if (!bcast_tuning_ok(h, ctaps, rot)) return SDRFM_EINVAL;
  const int rc = bcast_install_tuning(h, ctaps, rot, flags);
  return rc == SDRFM_OK ? sdrfm_bcast_reset(h) : rc;
}

// the taps and rotations replaced between two calls, the streams kept running.  Every check comes before any device work;
// like sdrfm_bcast_tune the call waits for the handle's stream before it replaces the taps a launch may still read, then enqueues the
// transform of the carried state and returns
int sdrfm_bcast_retune(sdrfm_bcast_t* h, const float* ctaps, const float* rot, const float* carry, const uint8_t* restart, uint32_t flags) {
  if (!h || !ctaps || !rot) return SDRFM_EINVAL;
  if (flags & ~SDRFM_TUNE_SHARED_INPUT) return SDRFM_EINVAL;
  const uint32_t ns = h->cfg.n_streams, T = h->f.T, H = h->f.H;
  if (!bcast_tuning_ok(h, ctaps, rot) || (carry && !finite_all(carry, 2 * ns))) return SDRFM_EINVAL;
  for (uint32_t s = 0; s < ns; ++s)
    if (restart && restart[s] > 1) return SDRFM_EINVAL;
  uint32_t any = 0;                                              // the streams' records, from the rotations the device still holds
  for (uint32_t s = 0; s < ns; ++s) {
    RetuneOp& op = h->ops_host[s];
    op.cr = carry ? carry[2 * s] : 1.0f;
    op.ci = carry ? carry[2 * s + 1] : 0.0f;
    float sh = h->rot_host[s] - rot[s];
    if (sh > 0x1.921fb6p+1f) sh -= 0x1.921fb6p+2f;
    else if (sh < -0x1.921fb6p+1f) sh += 0x1.921fb6p+2f;
    op.sh = sh;
    const bool identity = op.cr == 1.0f && op.ci == 0.0f && !std::signbit(op.ci);   // bitwise (1.0f, +0.0f)
    op.mode = (restart && restart[s]) ? RT_RESTART : ((identity ? 0u : RT_CARRY) | (sh == 0.0f ? 0u : RT_SHIFT));
    any |= op.mode;
  }
  const int rc = bcast_install_tuning(h, ctaps, rot, flags);
  if (rc != SDRFM_OK) return rc;
  if (any) {                                                     // (the identity re-tune launches nothing)
    if (hipMemcpy(h->d_ops, h->ops_host, sizeof(RetuneOp) * ns, hipMemcpyHostToDevice) != hipSuccess) return SDRFM_FAIL;
    const int c = h->f.cur;
    k_bcast_retune<<<dim3((ns + RT_STREAMS - 1) / RT_STREAMS), dim3(PF_THREADS), 0, h->f.stream>>>(h->d_ops, h->f.d_hist_x[c], h->f.d_yprev[c],
                                                                                                 h->f.d_hist_d[c], ns, T, H);
    if (hipGetLastError() != hipSuccess) return SDRFM_FAIL;
  }
  return SDRFM_OK;
}

// the streams' stereo blend and output gain.  Every check comes before any device work; like sdrfm_bcast_tune the call
// waits for the handle's stream before it replaces the records a launch may still read
int sdrfm_bcast_set_audio(sdrfm_bcast_t* h, const uint16_t* blend_q15, const uint16_t* gain_q15, uint32_t slew_q15) {
  if (!h) return SDRFM_EINVAL;
  if (slew_q15 > SDRFM_ACTL_ONE) return SDRFM_EINVAL;
  if (!slew_q15 && (blend_q15 || gain_q15)) return SDRFM_EINVAL;
  const uint32_t ns = h->cfg.n_streams;
  for (uint32_t s = 0; s < ns; ++s)
    if ((blend_q15 && blend_q15[s] > SDRFM_ACTL_ONE) || (gain_q15 && gain_q15[s] > SDRFM_ACTL_ONE)) return SDRFM_EINVAL;
  if (hipSetDevice(h->f.device) != hipSuccess) return SDRFM_FAIL;
  if (!slew_q15) {                                               // back to the plain kernels: b = v = 1, nothing to ramp
    if (hipStreamSynchronize(h->f.stream) != hipSuccess) return SDRFM_FAIL;
    for (uint32_t s = 0; s < ns; ++s) h->actl_host[s] = AudioCtlRec{SDRFM_ACTL_ONE, SDRFM_ACTL_ONE, SDRFM_ACTL_ONE, SDRFM_ACTL_ONE};
    h->blend = false;
    h->slew = SDRFM_ACTL_ONE;
    bcast_ramps_complete(h);
    return SDRFM_OK;
  }
  if (!h->d_actl && hipMalloc(&h->d_actl, sizeof(AudioCtlRec) * ns) != hipSuccess) return SDRFM_ENOMEM;
  if (hipStreamSynchronize(h->f.stream) != hipSuccess) return SDRFM_FAIL;   // no launch still reads the records about to be replaced
  for (uint32_t s = 0; s < ns; ++s)
    audio_ctl_rebase(&h->actl_host[s], h->slew, h->J, blend_q15 ? blend_q15 + s : nullptr, gain_q15 ? gain_q15 + s : nullptr);
  h->slew = slew_q15;
  h->J = 0;
  h->blend = true;
  if (hipMemcpy(h->d_actl, h->actl_host, sizeof(AudioCtlRec) * ns, hipMemcpyHostToDevice) != hipSuccess) return SDRFM_FAIL;
  return SDRFM_OK;
}

// the values the next output starts from, and the targets; any pointer may be NULL
int sdrfm_bcast_get_audio(const sdrfm_bcast_t* h, uint16_t* blend_q15, uint16_t* gain_q15, uint16_t* blend_target_q15, uint16_t* gain_target_q15) {
  if (!h) return SDRFM_EINVAL;
  for (uint32_t s = 0; s < h->cfg.n_streams; ++s) {
    const AudioCtlRec& r = h->actl_host[s];
    if (blend_q15) blend_q15[s] = (uint16_t)audio_ctl_ramp(r.b0, r.bt, h->slew, h->J);
    if (gain_q15) gain_q15[s] = (uint16_t)audio_ctl_ramp(r.v0, r.vt, h->slew, h->J);
    if (blend_target_q15) blend_target_q15[s] = (uint16_t)r.bt;
    if (gain_target_q15) gain_target_q15[s] = (uint16_t)r.vt;
  }
  return SDRFM_OK;
}

}  // extern "C"
