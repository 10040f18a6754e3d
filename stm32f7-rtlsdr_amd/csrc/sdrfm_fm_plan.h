/*
 * sdrfm_fm_plan.h — which designs an FM handle owns: the create-time half of the FM path's host arithmetic (sdrfm_fm_call.h has the per-call
 * half).  fm_plan() takes the config's shape and flags, the verdicts on the taps, the few facts only the runtime or design Q's translation unit
 * can give, and the development library's knobs; it returns the complete FmGeom, the chosen instances (indices into kFmInstances:
 * sdrfm_fm_tiles.h), the sizes and the names.  Plain C++17 without HIP: tests/native/fm_plan_case.cpp holds it to plans recorded on an MI355X
 * (tests/test_fm_plan_cpu.py), and the CPU checks of the call path get their FmGeom here.  sdrfm_create (sdrfm.hip) gathers the inputs, plans,
 * allocates what the plan asks for, and plans again with a design refused where the runtime would not have it.
 * Internal to the library; the drop-in boundary is include/sdrfm.h.
 */
#ifndef SDRFM_FM_PLAN_H
#define SDRFM_FM_PLAN_H

#include <math.h>
#include <stdio.h>
#include <string.h>

#include "sdrfm_fm_call.h"
#include "sdrfm_fm_tiles.h"
#include "sdrfm_q_host.h"

#define SDRFM_FM_MIX_R 4u           /* design B's tile for the noisy streams of a mixed batch (sdrfm_q.hip: kMixVariants carry it inside design Q's launch) */

// The development library's environment knobs (libsdrfm_dev.so reads them once per create: sdrfm.hip, fm_read_knobs); the defaults are the product.
struct FmKnobs {
  char fast_kind = 'b';              // SDRFM_FAST_KIND: 'a' = design A
  uint32_t fast_r = 12;              // SDRFM_FAST_R (default by kind: 12 for design B, 3 for design A)
  uint32_t audio_batch = 0;          // SDRFM_AUDIO_BATCH: design A's sub-tiles per audio flush (0: Da)
  uint32_t prio_balance = 1;         // SDRFM_NO_PRIO clears it
  uint32_t end_prio = (1u | (1u << 2)) << 6;   // SDRFM_END_PRIO
  uint32_t fold_state_ok = 1;        // SDRFM_NO_FOLD clears it
  bool no_stream = false;            // SDRFM_NO_STREAM: no design S
  bool stream_profile = false;       // SDRFM_STREAM_PROFILE: per-wave time stamps of design S
  uint32_t q_nslot = 0;              // SDRFM_Q_NSLOT: design Q's ring in KiB (0: the rate's default)
  uint32_t q_waves_per_cu = 0;       // SDRFM_Q_WAVES_PER_CU (0: by LDS, 12 at most)
  float q_guard_r = -1.0f, q_guard_a = -1.0f;   // SDRFM_Q_GUARD_R / _A (< 0: the taps' own; 0 and 4: the guard never fires)
  bool no_q = false;                 // SDRFM_NO_Q: no design Q
  bool q_no_adapt = false;           // SDRFM_Q_NO_ADAPT: design Q whatever the streams hold
  uint32_t warm_ahead = 0;           // SDRFM_WARM_AHEAD
  int ablate = 0;                    // SDRFM_ABLATE: kernel mode 2 .. 7 where the tile has it
  bool phase_profile = false;        // SDRFM_PHASE_PROFILE: kernel mode 1 where the tile has it
  uint32_t waves_per_cu = 0;         // SDRFM_WAVES_PER_CU (0: by LDS, 16 at most)
  uint32_t min_subtiles = 4;         // SDRFM_MIN_SUBTILES
  double mix_cost = 2.7, mix_rho = 12.7;   // SDRFM_MIX_COST, SDRFM_MIX_RHO
  bool mix_split_off = false;        // SDRFM_MIX_SPLIT_OFF
  bool mix_off = false;              // SDRFM_MIX_OFF: two launches for a mixed batch
  uint32_t mix_waves_per_cu = 0;     // SDRFM_MIX_WAVES_PER_CU
};

// What the taps say about design Q.
struct FmTapVerdict {
  bool lowpass;                      // sum|h| <= 2 |sum h|
  bool guard_ok;                     // the conditioning guard's thresholds exist and a carrier clears the radius
  float guard_r, guard_a;
};
// PERFORMANCE heuristic, not a correctness condition: design Q is offered LOW-PASS channel filters only, sum|h| <= 2 |sum h| (a windowed sinc
// has 1.2 - 1.5) — with heavy cancellation (no pass band around DC) |y| is small against the chain's partial sums for every input,
// the guard sends most outputs to the repair path and the bit-exact kernels are the faster way to the same numbers.
// The conditioning guard's thresholds (qtaps.c: sdrfm_q_guard).  A guard that would send a carrier at an eighth of full scale to the
// repair path makes design Q pointless for these taps: the bit-exact kernels serve them.
// (worst_case, SDRFM_CFG_GUARD_WORST_CASE: the radius from the proven worst-case bound — 6.9 x at 64 taps; a carrier at a third of full scale must still clear it)
static inline FmTapVerdict fm_tap_verdict(const float* h, uint32_t T, const float* g, uint32_t Ta, bool worst_case) {
  double q_abs = 0.0, q_sum = 0.0;
  for (uint32_t k = 0; k < T; ++k) { q_abs += fabs((double)h[k]); q_sum += (double)h[k]; }
  FmTapVerdict v = {q_abs <= 2.0 * fabs(q_sum), false, 0.0f, 4.0f};
  v.guard_ok = sdrfm_q_guard2(h, T, g, Ta, worst_case ? 1 : 0, &v.guard_r, &v.guard_a) == 0 &&
               (double)v.guard_r <= (worst_case ? 0.33 : 0.125) * 127.5 * fabs(q_sum) && v.guard_a > 3.0f;
  return v;
}

struct FmPlanIn {
  uint32_t T, D, Ta, Da, n_streams;
  bool force_generic, bit_exact;     // SDRFM_CFG_FORCE_GENERIC, SDRFM_CFG_BIT_EXACT
  uint32_t n_cu;
  FmTapVerdict taps;
  bool q_built;                      // sdrfm_q_build held the taps (asked only where fm_plan_offers_q says so) ...
  uint32_t q_c0;                     // ... and the first K-chunk that holds one
  // design Q's translation unit (sdrfm_q.hip) and the runtime
  uint32_t q_default_nslot;          // the rate's ring in KiB, and a wave's LDS bytes with it (0: no instance at this D, Da)
  uint32_t q_default_lds;
  uint32_t q_lds;                    // a wave's LDS bytes at the ring fm_plan_q_nslot names
  const char* q_symbol;              // the kernel's name at (q_c0, that ring)
  uint32_t mix_lds;                  // the one-launch kernel with design B's R = 4 tile at (q_c0, that ring, T): LDS bytes of a workgroup (0: no instance) ...
  int mix_blocks_per_cu;             // ... and how many of them the runtime says a CU holds (0: unknown)
};
// What the runtime refused (sdrfm_create plans again without it).
struct FmRefused {
  bool q;                            // design Q's tables or routing state could not be allocated
  uint32_t instances;                // bit i: hipFuncSetAttribute refused kFmInstances[i] its LDS
};

struct FmPlan {
  bool supported;                    // false: not even the generic kernel fits the shape (SDRFM_NOT_SUPPORTED)
  FmGeom geo;
  int fast, fast_s, fast_mix;        // kFmInstances indices; -1: none
  uint32_t AB, warm_ahead;           // the fast tile: sub-tiles of d buffered per audio flush, L2 warm-up distance
  int fast_mode;                     // ... its kernel mode
  bool stream_profile;               // development library: d_dbg holds design S's time stamps / (fast_mode == 1) the fast tile's phase profile
  size_t lds_bytes;                  // the generic kernel's block
  uint32_t q_nslot, q_c0;
  float q_guard_r, q_guard_a;
  char generic_name[64], fast_name[64], fast_s_name[64], fast_q_name[64], kernel_name[64];
};

// design Q: K2 on the i8 matrix pipe (sdrfm_q.hip).  Not bit-identical to the fmaf-chain kernels (within 1e-6 of the oracle where the phase is
// well conditioned, repaired to the definition's own d where it is not), so a handle created with SDRFM_CFG_BIT_EXACT never selects it.
// Instances: (D, Da) = (10, 5) — the 2.4 MS/s front end of BASELINE —, (8, 8) and (16, 5): the 2.048 and 3.2 MS/s rates RTLSDR_set_sample_rate
// accepts (usbh_rtlsdr.c:676-678); 32 audio taps each.
static inline bool fm_plan_offers_q(const FmPlanIn& in, const FmKnobs& k) {
  return !in.force_generic && !in.bit_exact && !k.no_q && in.q_default_lds != 0 && in.Ta == SDRFM_Q_TA && in.T <= SDRFM_Q_TP && in.T <= 9 * in.D &&
         in.taps.lowpass && in.taps.guard_ok;
}
static inline uint32_t fm_plan_q_nslot(const FmPlanIn& in, const FmKnobs& k) { return k.q_nslot ? k.q_nslot : in.q_default_nslot; }

static inline bool fm_instance_serves(const FmInstance& v, const FmPlanIn& in) {
  return v.T == in.T && v.D == in.D && (!v.Ta || (v.Ta == in.Ta && v.Da == in.Da));
}

static inline FmPlan fm_plan(const FmPlanIn& in, const FmKnobs& k, const FmRefused& refused) {
  FmPlan p;
  memset(&p, 0, sizeof(p));
  p.fast = p.fast_s = p.fast_mix = -1;
  FmGeom& geo = p.geo;
  geo.T = in.T; geo.D = in.D; geo.Ta = in.Ta; geo.Da = in.Da; geo.n_streams = in.n_streams;
  geo.fold_state_ok = k.fold_state_ok;
  const FmGenericTile gt = fm_generic_tile(in.T, in.D, in.Ta, in.Da);
  p.lds_bytes = gt.lds;
  p.supported = gt.lds <= 160 * 1024;
  if (!p.supported) return p;
  geo.NA = gt.NA;
  snprintf(p.generic_name, sizeof(p.generic_name), "generic T%u D%u Ta%u Da%u NA%u", in.T, in.D, in.Ta, in.Da, gt.NA);
  snprintf(p.kernel_name, sizeof(p.kernel_name), "%s", p.generic_name);
  if (in.force_generic) return p;
  auto usable = [&](int i) { return !((refused.instances >> i) & 1u) && fm_instance_serves(kFmInstances[i], in); };

  // design S
  for (int i = 0; i < kFmInstanceCount && p.fast_s < 0; ++i) {
    const FmInstance& v = kFmInstances[i];
    if (v.kind != 's' || !usable(i) || k.no_stream) continue;
    p.fast_s = i;
    p.stream_profile = k.stream_profile;
    geo.has_s = true; geo.seg = v.seg; geo.n_cu = in.n_cu;
    snprintf(p.fast_s_name, sizeof(p.fast_s_name), "fast-s T%u D%u S%u L%u Ta%u Da%u", v.T, v.D, v.R, v.seg, v.Ta, v.Da);
  }

  // design Q
  if (fm_plan_offers_q(in, k) && in.q_built && !refused.q) {
    geo.has_q = true; geo.n_cu = in.n_cu;
    p.q_c0 = in.q_c0 > 1 ? 1 : in.q_c0;
    p.q_guard_r = k.q_guard_r < 0.0f ? in.taps.guard_r : k.q_guard_r;
    p.q_guard_a = k.q_guard_a < 0.0f ? in.taps.guard_a : k.q_guard_a;
    p.q_nslot = fm_plan_q_nslot(in, k);
    geo.q_waves_per_cu = 12;
    if (SDRFM_FM_LDS_PER_CU / in.q_default_lds < geo.q_waves_per_cu) geo.q_waves_per_cu = SDRFM_FM_LDS_PER_CU / in.q_default_lds;   // (D = 16: 11 one-wave workgroups fit a CU's LDS)
    if (k.q_waves_per_cu) geo.q_waves_per_cu = k.q_waves_per_cu;
    geo.q_lds = in.q_lds;
    geo.q_lds_waves_per_cu = in.q_lds ? (uint32_t)(SDRFM_FM_LDS_PER_CU / in.q_lds) : 0u;
    snprintf(p.fast_q_name, sizeof(p.fast_q_name), "fast-q T%u D%u Ta%u Da%u %s", in.T, in.D, in.Ta, in.Da, in.q_symbol ? in.q_symbol : "");
  }

  // the fast bit-exact tile: the wanted kind at the wanted R, else the first of that kind, else the first there is
  for (int pass = 0; pass < 3 && p.fast < 0; ++pass)
    for (int i = 0; i < kFmInstanceCount; ++i) {
      const FmInstance& v = kFmInstances[i];
      if (v.kind == 's' || !usable(i)) continue;
      if (pass == 0 && (v.R != k.fast_r || v.kind != k.fast_kind)) continue;
      if (pass == 1 && v.kind != k.fast_kind) continue;
      const uint32_t NYT = 64 * v.R, DOFF = (in.Ta - 1 + 3u) & ~3u;
      // audio flush every AB sub-tiles: AB = Da makes every flush exactly 64*R outputs (all lanes busy)
      uint32_t AB = v.kind == 'b' ? (uint32_t)fastb_ab((int)v.R) : (k.audio_batch ? k.audio_batch : in.Da);   // (design B: a compile-time property of the tile)
      if (AB > 8) AB = 8;
      while (AB > 1 && fast_tile_lds(v.xbytes, AB, v.R, v.T, in.Ta) > 40 * 1024) --AB;
      if (in.Ta - 1 > AB * NYT || DOFF + AB * NYT < 2 * (in.Ta + 1)) continue;
      const size_t lds = fast_tile_lds(v.xbytes, AB, v.R, v.T, in.Ta);
      if (lds > 160 * 1024) continue;
      p.fast = i;
      p.AB = AB;
      p.warm_ahead = k.warm_ahead;
      if (k.ablate >= 2 && k.ablate <= 7 && ((v.modes >> k.ablate) & 1u)) p.fast_mode = k.ablate;
      if (k.phase_profile && ((v.modes >> 1) & 1u) && !p.stream_profile) p.fast_mode = 1;
      geo.has_fast = true; geo.fast_is_b = v.kind == 'b'; geo.fast_R = v.R; geo.fast_lds = lds;
      uint32_t per_cu = (uint32_t)((160 * 1024) / lds);
      if (per_cu > 16) per_cu = 16;
      if (k.waves_per_cu) per_cu = k.waves_per_cu;
      geo.waves_target = in.n_cu * per_cu;
      geo.min_subtiles = k.min_subtiles ? k.min_subtiles : 4;
      snprintf(p.fast_name, sizeof(p.fast_name), "fast-%c T%u D%u R%u Ta%u Da%u AB%u", v.kind, v.T, v.D, v.R, in.Ta, in.Da, AB);
      snprintf(p.kernel_name, sizeof(p.kernel_name), "%s", p.fast_name);
      break;
    }

  // design B's smallest tile for the noisy streams of a mixed batch: beside design Q's launch, or inside it where the one-launch kernel has an instance
  if (geo.has_fast && geo.fast_is_b && geo.has_q)
    for (int i = 0; i < kFmInstanceCount && p.fast_mix < 0; ++i) {
      const FmInstance& v = kFmInstances[i];
      if (v.kind != 'b' || v.R != SDRFM_FM_MIX_R || !usable(i)) continue;
      const uint32_t NYT = 64 * v.R, DOFF = (in.Ta - 1 + 3u) & ~3u;
      if (in.Ta - 1 > NYT || DOFF + NYT < 2 * (in.Ta + 1)) continue;
      p.fast_mix = i;
      geo.has_mix_tile = true;
      geo.fast_mix_lds = fastb_lds((int)v.T, (int)v.D, (int)v.R, (int)in.Ta);
      // a stream costs the design-B workgroups about mix_cost times what it costs design Q's: the shares of the wave slots (measured: 2.0 / 2.7 / 3.2 ->
      // 41.2 / 38.9 / 40.3 us serial, 31.5 / 30.8 / 33.0 us overlapped with a quarter of the streams noisy: profiles/r05_mixed_batches.txt)
      geo.mix_R = v.R; geo.mix_cost = k.mix_cost; geo.mix_rho = k.mix_rho; geo.mix_split_off = k.mix_split_off;
      geo.mix_lds = in.mix_lds;
      if (geo.mix_lds) {
        geo.mix_waves_per_cu = in.mix_blocks_per_cu > 0 ? (uint32_t)in.mix_blocks_per_cu : SDRFM_FM_LDS_PER_CU / geo.mix_lds;
        if (geo.mix_waves_per_cu > geo.q_waves_per_cu) geo.mix_waves_per_cu = geo.q_waves_per_cu;   // (15 fit; design Q's own 12 are faster: sdrfm_q.hip)
        if (k.mix_off) geo.mix_lds = 0;
        if (k.mix_waves_per_cu) geo.mix_waves_per_cu = k.mix_waves_per_cu;
      }
    }
  return p;
}

#endif
