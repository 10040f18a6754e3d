/*
 * sdrfm_fm_call.h — the FM call path's host arithmetic (sdrfm.hip: enqueue): which design may serve a call, how the machine's wave slots are
 * dealt out, how a stream is cut into segments, waves or runs.  Plain C++17 without HIP: values and two small PODs in, values out, so that
 * tests/native/fm_call_check.cpp (tests/test_fm_call_cpu.py) runs all of it on a CPU — the bit-exact designs give the same bits however a stream
 * is segmented and design Q however it is cut into runs, so no parity test sees a wrong share or an empty run; the GPU only sees it as time or
 * as a fault.  enqueue() keeps the HIP sequencing and calls in here for every number it launches with.
 * Internal to the library; the drop-in boundary is include/sdrfm.h.
 */
#ifndef SDRFM_FM_CALL_H
#define SDRFM_FM_CALL_H

#include <stddef.h>
#include <stdint.h>

#define SDRFM_FM_Q_STEP_OUT 128u   /* design Q: decimated outputs per wave step (sdrfm_q.h: SDRFM_Q_STEP_OUT; sdrfm.hip asserts they agree) */
#define SDRFM_FM_LDS_PER_CU 163840u
#define SDRFM_FM_CHAIN_FIX 64u     /* the PCM sink's chain: audio outputs of a run its predecessor's state still reaches (sdrfm_sink_chain.h: SDRFM_CHAIN_FIX; sdrfm.hip asserts they agree) */

// What sdrfm_create fixes and a call never changes.
struct FmGeom {
  uint32_t T, D, Ta, Da;             // channel taps / decimation, audio taps / decimation
  uint32_t n_streams;
  uint32_t n_cu;                     // compute units of the device
  // which designs exist for the handle
  bool has_q;                        // design Q (operand tables on the device)
  bool has_fast, fast_is_b;          // a fast bit-exact tile (design B; development library: or design A)
  bool has_s;                        // design S
  bool has_mix_tile;                 // design B's smallest tile (R = 4): the noisy streams' workgroups beside design Q's
  uint32_t mix_lds;                  // ... INSIDE design Q's launch (k_mix): LDS bytes of a workgroup, 0 = no instance
  // design Q
  uint32_t q_waves_per_cu;
  size_t q_lds;                      // LDS bytes of one of its waves
  uint32_t q_lds_waves_per_cu;       // ... and how many of them a CU's LDS holds (15 at D = 10; q_waves_per_cu is what a launch is cut for)
  // design B
  uint32_t fast_R;                   // outputs per lane and sub-tile of the handle's tile
  size_t fast_lds;
  uint32_t waves_target;             // resident waves the fast kernel aims for (CUs x waves that fit by LDS)
  uint32_t min_subtiles;             // minimum sub-tiles per segment (bounds the per-segment halo recompute)
  uint32_t fold_state_ok;            // design B knob, fixed at create
  size_t fast_mix_lds;               // the R = 4 tile: LDS bytes of a wave in a launch of its own
  uint32_t mix_R, mix_waves_per_cu;  // ... its R; workgroups of the one launch a CU holds
  double mix_cost, mix_rho;          // what a stream costs design B against design Q; a design-B sub-tile in design-Q quads
  bool mix_split_off;                // (development library: SDRFM_MIX_SPLIT_OFF keeps the share-only split of the wave slots)
  // design S: samples per lane segment; generic kernel: audio outputs per tile
  uint32_t seg, NA;
};

// One call.
struct FmCall {
  uint32_t N, M, A;                  // per stream: IQ samples, decimated outputs, audio outputs
  uint32_t phase_x, phase_d;         // the two decimators' phases before the call
  uint64_t n_seen;                   // IQ samples consumed since reset (history is all-real once >= T-1)
  bool iq_al4, iq_al16;              // iq and iq_stride are both multiples of 4 / of 16 bytes
};

// ---- counts ------------------------------------------------------------------------------------------------------------------------------
// a decimator by `decim` at phase `phase` (inputs since its last output) given n more inputs: outputs, phase afterwards
struct FmStage { uint32_t out, phase; };
static inline FmStage fm_stage(uint32_t phase, uint64_t n, uint32_t decim) {
  return FmStage{(uint32_t)(((uint64_t)phase + n) / decim), (uint32_t)(((uint64_t)phase + n) % decim)};
}
struct FmCounts { uint32_t N, M, A, phase_x, phase_d; };   // the call's counts, and the phases AFTER it
static inline FmCounts fm_counts(uint32_t phase_x, uint32_t phase_d, uint32_t nbytes, uint32_t D, uint32_t Da) {
  const uint32_t N = nbytes / 2;
  const FmStage x = fm_stage(phase_x, N, D), d = fm_stage(phase_d, x.out, Da);
  return FmCounts{N, x.out, d.out, x.phase, d.phase};
}
// the most audio outputs a call of nbytes can give at any phases, and one to spare at either stage (buffer sizes)
static inline uint32_t fm_max_audio(uint32_t D, uint32_t Da, uint32_t nbytes) {
  const uint64_t m = (uint64_t)fm_stage(D - 1, nbytes / 2, D).out + 1;
  return fm_stage(Da - 1, m, Da).out + 1;
}

// ---- eligibility -------------------------------------------------------------------------------------------------------------------------
// decimated outputs touching never-seen samples at the start of a stream
static inline uint32_t fm_y_aff(const FmGeom& g) { return (g.T + g.D - 1) / g.D + 1; }
// Design B cannot express the zero history at the start of a stream in bytes: until T-1 real samples have been seen its
// first y_aff outputs are wrong and the generic kernel recomputes the audio that depends on them (fm_fixup).  The STATE it
// hands over (last Ta-1 discriminator outputs, y[M-1]) must not contain any of those outputs either, so a first call that
// short runs on the generic kernel entirely.
static inline bool fm_short_first(const FmGeom& g, const FmCall& c) {
  return g.has_fast && g.fast_is_b && c.n_seen + 1 < g.T && c.M < fm_y_aff(g) + g.Ta;
}
static inline bool fm_fast_ok(const FmGeom& g, const FmCall& c) {
  return g.has_fast && c.A > 0 && (c.phase_x % 2 == 0) && c.iq_al4 && c.N < (1u << 30) && !fm_short_first(g, c);
}
static inline uint32_t fm_q_steps(uint32_t M) { return (M + SDRFM_FM_Q_STEP_OUT - 1) / SDRFM_FM_Q_STEP_OUT; }
static inline uint32_t fm_q_quads(uint32_t M) { return ((M + 7u) / 8u + 3u) / 4u; }
// Design Q serves whole numbers of audio periods at decimator phase 0 on 16-byte aligned rows, when the call holds enough steps
// (128 outputs each) to put at least two waves on every CU; the first call after a reset must be long enough that the state it
// hands over holds no output computed from the (inexpressible in bytes) zero history.  It also serves one dongle's second of IQ
// (BASELINE configs[1]: 1875 steps cut into two-step runs, 5.7 us against 9.6 - 13 us for design B).
static inline bool fm_q_fit(const FmGeom& g, const FmCall& c) {
  return g.has_q && c.A > 0 && c.phase_x == 0 && c.phase_d == 0 && (c.N % (g.D * g.Da * 8u)) == 0 &&
         c.iq_al16 && c.N < (1u << 30) && c.M >= g.Ta &&
         (c.n_seen + 1 >= g.T || c.M >= fm_y_aff(g) + g.Ta) &&
         (uint64_t)g.n_streams * fm_q_steps(c.M) >= 2ull * g.n_cu;
}
// design Q serves n_clean streams (all of them when no stream is noisy); with half of the streams
// noisy the bit-exact kernels take the whole batch (design S fills the machine then)
static inline bool fm_q_ok(bool q_fit, uint32_t n_noisy, uint32_t n_streams) {
  return q_fit && n_streams - n_noisy > 0 && 2 * n_noisy < n_streams;
}
// a mixed call whose two kinds of workgroup go out in ONE launch (k_mix)
static inline bool fm_fuse(const FmGeom& g, const FmCall& c, bool mixed) {
  return mixed && g.mix_lds && fm_fast_ok(g, c) && g.has_mix_tile && c.M >= g.Ta && g.fold_state_ok;
}
// Who serves the call, given the n_noisy streams the routing has sent to the bit-exact kernels (sdrfm_fm_route.h; 0 for a call design Q cannot take): design Q
// some of the streams (q_ok), the bit-exact kernels every stream on the handle's stream (bx_all) or the noisy ones beside design Q (mixed): in its launch
// (fuse) or ahead of it.
struct FmServe { bool q_ok, bx_all, mixed, fuse; };
static inline FmServe fm_serve(const FmGeom& g, const FmCall& c, uint32_t n_noisy) {
  FmServe s;
  s.q_ok = fm_q_ok(fm_q_fit(g, c), n_noisy, g.n_streams);
  s.bx_all = !s.q_ok; s.mixed = s.q_ok && n_noisy > 0; s.fuse = fm_fuse(g, c, s.mixed);
  return s;
}
// Design S.  A lane-segment wave is long (its 64 lanes walk 480 samples each, ~25 us alone on a SIMD): design S pays when
// the launch fills the machine (>= one wave per SIMD); a single dongle's call is served faster by design B,
// which cuts its segments as short as the call needs.  Not beside design Q's launch (mixed): design B's small tile serves
// there — a wave of design S needs 16 KB of LDS and lasts 25 us.
static inline uint32_t fm_s_waves(const FmGeom& g, const FmCall& c) { return (c.N / g.seg + 62) / 63; }   // waves per stream: 63 useful lane segments each
static inline bool fm_stream_ok(const FmGeom& g, const FmCall& c, uint32_t nsub, bool mixed) {
  return fm_fast_ok(g, c) && g.has_s && c.phase_x == 0 && c.phase_d == 0 && (c.N % g.seg) == 0 &&
         (c.M % g.Da) == 0 && c.M >= g.Ta && c.iq_al16 &&
         g.fold_state_ok &&
         (uint64_t)nsub * fm_s_waves(g, c) >= 4ull * g.n_cu &&
         !mixed;
}
// SDRFM_F_OVERLAP, the part that is geometry: the stream has T-1 real samples, and the previous call's buffer can warm design Q's runs up
// (two steps of it at least, rows of whole 16-byte pieces)
static inline bool fm_ovl_geometry_ok(const FmGeom& g, const FmCall& c, uint32_t prev_nbytes, bool prev_al16) {
  return c.n_seen + 1 >= g.T &&
         prev_nbytes >= 2u * g.D * SDRFM_FM_Q_STEP_OUT && (prev_nbytes % 16 == 0) && prev_al16;
}
// Quads (32 decimated outputs = 32 / Da audio outputs each) a run spans at least when the sink's chain rides in the launch.  A run publishes its end state from
// its own outputs alone, as if nothing before them mattered, and its first SDRFM_FM_CHAIN_FIX audio outputs are finished with its predecessor's state: both
// stand only for a run that OWNS more than SDRFM_FM_CHAIN_FIX audio outputs ((1 - alpha)^64 is below rounding for every alpha the chain serves; a run of
// 48 would publish a state that lacks (1 - alpha)^48 = 1.6e-6 of what came before it at the 75 us alpha).  One warm-up quad and the owned quads that hold
// SDRFM_FM_CHAIN_FIX + 2 audio periods (a run's first and last audio output are cut by floor(32 q / Da): one period may be lost): 18 at Da = 8 (17 owned:
// 68 audio outputs); never fewer than the 13 of Da = 5 (12 owned: 76 audio outputs).
static inline uint32_t fm_chain_run_quads(uint32_t Da) {
  const uint32_t own = ((SDRFM_FM_CHAIN_FIX + 2u) * Da + 31u) / 32u;
  return 1u + (own > 12u ? own : 12u);
}
// The sink's chain inside design Q's launch, the part that needs no sink: every stream's whole audio row from this launch (no routed stream unless
// the one launch serves it, no outputs the generic kernel recomputes behind it at the start of a stream), enough quads for runs longer than their
// predecessor's reach.
static inline bool fm_chain_fits(const FmGeom& g, const FmCall& c, bool q_ok, bool mixed, bool fuse) {
  return q_ok && (!mixed || fuse) && !(c.n_seen + 1 < g.T) && fm_q_quads(c.M) >= fm_chain_run_quads(g.Da);
}

// ---- the machine's wave slots ------------------------------------------------------------------------------------------------------------
struct FmSplit { uint32_t bx_waves, q_total; };   // the bit-exact kernels' waves, design Q's workgroups
// Mixed calls share the machine between the two launches: a stream costs the bit-exact kernels about twice what it costs design Q, so design Q's
// grid is cut for its share of the CUs' wave slots (fewer runs per stream) and design B's for the LDS that leaves (its launch goes out first: its
// waves are the longer ones).
// Where the shape has a one-launch kernel (k_mix) both kinds of workgroup go out in ONE grid that fills the machine once: the wave slots are dealt out by
// the same shares, a design-B segment is about as long as a design-Q run, and neither launch waits for the other.
static inline FmSplit fm_split(const FmGeom& g, const FmCall& c, bool mixed, bool fuse, uint32_t n_noisy) {
  FmSplit s = {g.waves_target, g.q_waves_per_cu * g.n_cu};
  if (!mixed) return s;
  const uint32_t n_clean = g.n_streams - n_noisy;
  const double cost = fuse ? g.mix_cost : 2.0;
  const double share = (cost * n_noisy) / ((double)n_clean + cost * n_noisy);
  if (fuse) {
    const uint32_t total = g.mix_waves_per_cu * g.n_cu;
    const uint32_t q_steps = fm_q_steps(c.M);
    s.bx_waves = (uint32_t)((double)total * share + 0.5);
    if (s.bx_waves < n_noisy) s.bx_waves = n_noisy;
    // The whole grid is resident at once, so the launch lasts as long as its LONGEST wave, and both kinds of wave come in whole units: a design-B segment walks
    // ceil(NA Da / 256) sub-tiles (a partly filled one costs a whole one), a design-Q run ceil((quads + runs) / runs) quads.  Around the share above, the number of
    // segments per routed stream is therefore chosen for the smaller of the two maxima — a sub-tile of design B weighs 12.7 quads of design Q in a wave's time at
    // this shape (64 taps, / 10: calibrated at 25 % routed streams, where 16 segments of six sub-tiles beside runs of 76 quads balance) —, ties for the fuller
    // sub-tiles: 28.4 -> 27.1 us per call with a quarter of the streams routed (profiles/r06_mixed_split.txt).  Other shapes keep the share as it is.
    if (g.T == 64 && g.D == 10 && g.mix_R == 4 && c.A >= 64 && !g.mix_split_off) {
      const uint32_t nyt = 64u * g.mix_R, qt = fm_q_quads(c.M), s0 = s.bx_waves / n_noisy;
      double best_cost = 1e30, best_eff = 0.0;
      uint32_t best_s = 0;
      for (uint32_t sg = s0 > 6u ? s0 - 6u : 1u; sg <= s0 + 4u; ++sg) {
        const uint32_t na = (c.A + sg - 1u) / sg, tiles = (c.A + na - 1u) / na;
        if ((uint64_t)tiles * n_noisy + n_clean > total) break;
        const uint32_t sub = (na * g.Da + nyt - 1u) / nyt;
        uint32_t rr = (total - tiles * n_noisy) / n_clean;
        if (rr > q_steps / 2u) rr = q_steps / 2u;
        if (rr < 1u) continue;
        const uint32_t quads = (qt + rr + rr - 1u) / rr;
        const double cost = (double)sub * g.mix_rho > (double)quads ? (double)sub * g.mix_rho : (double)quads;
        const double eff = (double)(na * g.Da) / (double)(sub * nyt);
        if (cost < best_cost - 1e-9 || (cost < best_cost + 1e-9 && eff > best_eff)) { best_cost = cost; best_eff = eff; best_s = tiles; }
      }
      if (best_s) s.bx_waves = best_s * n_noisy;
    }
    s.q_total = total > s.bx_waves + n_clean ? total - s.bx_waves : n_clean;
  } else {
    uint32_t q_slots = (uint32_t)((double)g.q_waves_per_cu * (1.0 - share) + 0.5);
    if (q_slots + 1 > g.q_waves_per_cu) q_slots = g.q_waves_per_cu - 1;
    if (q_slots < 2) q_slots = 2;
    const size_t left = SDRFM_FM_LDS_PER_CU > q_slots * g.q_lds ? SDRFM_FM_LDS_PER_CU - q_slots * g.q_lds : 0u;
    const size_t b_lds = g.has_mix_tile ? g.fast_mix_lds : g.fast_lds;
    uint32_t per_cu = b_lds ? (uint32_t)(left / b_lds) : 1u;
    if (per_cu < 1) per_cu = 1;
    s.bx_waves = g.n_cu * per_cu;
    s.q_total = q_slots * g.n_cu;
  }
  return s;
}

// ---- a stream's cut into workgroups ------------------------------------------------------------------------------------------------------
struct FmTiles { uint32_t NA, tiles_per_stream, grid, fold_state; };   // audio outputs per tile, tiles per stream, workgroups of the launch, hand-over folded
// Design B: every stream is split into segments so that ~bx_waves waves are resident; each segment >= min_subtiles sub-tiles.
// `small_tile`: the R = 4 tile serves (the noisy streams of a mixed call where it exists), else the handle's own.
static inline FmTiles fm_b_tiles(const FmGeom& g, const FmCall& c, uint32_t nsub, uint32_t bx_waves, bool small_tile) {
  const uint32_t NYT = 64 * (small_tile ? g.mix_R : g.fast_R);
  const uint32_t sub_total = (c.M + NYT - 1) / NYT;
  uint32_t segs = bx_waves / nsub;
  // a segment pays a fixed prologue, so it normally covers >= min_subtiles sub-tiles; when that would leave most of the
  // GPU without a wave (few streams: the reference's one dongle), shorter segments win: one stream x 1 s runs in 9.6 us
  // with single-sub-tile segments against 18.8 us with four
  uint32_t ms = g.min_subtiles;
  while (ms > 1 && (uint64_t)nsub * (sub_total / ms) < bx_waves / 2) ms >>= 1;
  const uint32_t seg_cap = sub_total / ms;
  if (segs > seg_cap) segs = seg_cap;
  if (segs < 1) segs = 1;
  FmTiles t;
  t.NA = (c.A + segs - 1) / segs;
  t.tiles_per_stream = (c.A + t.NA - 1) / t.NA;
  t.grid = nsub * t.tiles_per_stream + nsub;
  // design B: state hand-over folded into the last segment's wave (needs M >= Ta so that the d ring alone holds the
  // new history, and the last sub-tile must contain y[M-1], which the kernel arranges)
  t.fold_state = ((small_tile || g.fast_is_b) && c.M >= g.Ta && g.fold_state_ok) ? 1u : 0u;
  if (t.fold_state) t.grid -= nsub;
  return t;
}
// the generic kernel: tiles of NA audio outputs, one hand-over block per stream
static inline FmTiles fm_generic_tiles(const FmGeom& g, const FmCall& c, uint32_t nsub) {
  FmTiles t;
  t.NA = g.NA;
  t.tiles_per_stream = (c.A + g.NA - 1) / g.NA;
  t.grid = nsub * t.tiles_per_stream + nsub;
  t.fold_state = 0;
  return t;
}
// The bit-exact launch over nsub streams: design S where it pays ('s': tiles_per_stream waves per stream), else design B cut for bx_waves resident waves ('b':
// on its small tile for the noisy streams of a mixed call where that exists, else on the handle's own), else the generic kernel ('g').
struct FmBx { char kind; bool small_tile; FmTiles tiles; bool halo_bytes; };   // halo_bytes: the kernel reads its halo as bytes
static inline FmBx fm_bx(const FmGeom& g, const FmCall& c, uint32_t nsub, uint32_t bx_waves, bool mixed) {
  if (fm_stream_ok(g, c, nsub, mixed)) { const uint32_t w = fm_s_waves(g, c); return FmBx{'s', false, FmTiles{0u, w, nsub * w, 1u}, true}; }
  if (fm_fast_ok(g, c)) { const bool small = mixed && g.has_mix_tile; return FmBx{'b', small, fm_b_tiles(g, c, nsub, bx_waves, small), small || g.fast_is_b}; }
  return FmBx{'g', false, fm_generic_tiles(g, c, nsub), false};
}
// Designs Q, B and S read their halo as bytes, which cannot express the zero history at the start of a stream: the few audio
// outputs that depend on inputs before the first real sample are recomputed by the generic kernel (tile 0..k only), for every stream.
struct FmFixup { uint32_t y_aff, a_aff, tiles_per_stream; };
static inline FmFixup fm_fixup(const FmGeom& g, const FmCall& c) {
  FmFixup f;
  f.y_aff = fm_y_aff(g);
  f.a_aff = (f.y_aff + g.Ta + g.Da - 1) / g.Da;  // audio outputs touching them
  f.tiles_per_stream = (f.a_aff + g.NA - 1) / g.NA;
  const uint32_t full = (c.A + g.NA - 1) / g.NA;
  if (f.tiles_per_stream > full) f.tiles_per_stream = full;
  return f;
}

// ---- design Q's runs ---------------------------------------------------------------------------------------------------------------------
struct FmRuns { uint32_t runs; bool with_chain; };
// runs (waves) per stream: fill the machine once; every run at least four owned steps (a run warms up over a quarter of a step), two
// when the call is too small to fill the machine otherwise
static inline uint32_t fm_q_min_steps(uint32_t n_clean, uint32_t q_steps, uint32_t q_total) {
  return ((uint64_t)n_clean * (q_steps / 4) >= (uint64_t)q_total / 2) ? 4u : 2u;
}
// What a run costs, in vector instructions per lane, counted once in the gfx950 assembly of k_mfir<0,5,10,5> as the library's Makefile builds it (static counts
// along the path of a warmed-up run that meets no repair; not fitted to any timing — they only rank run counts):
//   a run, whatever its length: 140 before the first matrix issue + 29 the peeled last step has over a loop step + 21 for the two flush set-ups behind it
//                               + 10 on the way out = 200
//   an audio stage:             76 for its 128 outputs + 10 for the flush's trip that stores them = 86
//   a step, whole or partly filled: 105 vector instructions and 9 matrix issues = 114 (the audio stage apart)
#define SDRFM_FM_Q_RUN_VALU 200u
#define SDRFM_FM_Q_STAGE_VALU 86u
#define SDRFM_FM_Q_STEP_VALU 114u
// a stream's Gq = Qt + (warm-up quads) grid quads dealt out to `runs` runs as the kernel does it (sdrfm_q.hip: e0, e1): the longest run's quads, the steps it walks
// and the audio stages it executes
struct FmRunShape { uint32_t quads, steps, stages; };
static inline FmRunShape fm_q_run_shape(uint32_t M, uint32_t runs, bool overlapped, uint32_t Da) {
  const uint32_t Gq = fm_q_quads(M) + runs - 1u + (overlapped ? 1u : 0u);
  FmRunShape s;
  s.quads = (Gq + runs - 1u) / runs; s.steps = (s.quads + 3u) / 4u; s.stages = (s.steps + Da - 1u) / Da;
  return s;
}
static inline uint64_t fm_q_runs_cost(uint32_t runs, const FmRunShape& s) {
  return (uint64_t)runs * (SDRFM_FM_Q_RUN_VALU + (uint64_t)SDRFM_FM_Q_STAGE_VALU * s.stages + (uint64_t)SDRFM_FM_Q_STEP_VALU * s.steps);
}
// chain_run_quads: fm_chain_run_quads(Da) of the handle (the default is the BASELINE front end's, Da = 5: the least any rate needs)
// staged (an overlapped plain call; Da, park_stages = SDRFM_Q_PARK_STAGES, lds_waves = the waves the device holds by LDS: FmGeom::q_lds_waves_per_cu x n_cu): the
// count is chosen for whole audio stages.  Filling the machine once (`fill`, the rule below) leaves a run of the headline call 16 steps: four audio stages, the last
// of them computed for one step's d's, and every run pays its fixed cost.  Two overlapped calls are resident together, so fewer, longer runs still occupy every
// wave slot.  Among the counts from `fill` down to the least that does (2 n_clean runs >= lds_waves), those whose runs execute NO MORE STAGES than fill's (the longer
// run only fills the last stage up: nothing this rule picks adds a stage to a run, let alone a flush inside the step loop) are ranked by
// runs x (SDRFM_FM_Q_RUN_VALU + SDRFM_FM_Q_STAGE_VALU x stages + SDRFM_FM_Q_STEP_VALU x steps); ties go to the larger count.  The step term keeps counts out
// that leave every run's last step mostly empty: 11 runs of the headline call walk 11 x 18 = 198 steps against 192 and 190, and measure slower than 12
// (profiles/q_runs_ab.txt).  Every constraint of the rule below is an upper bound on the count, so it holds for the choice as well.  Calls that do not
// fill the machine (min_steps = 2, a single stream) keep `fill`.
static inline FmRuns fm_q_runs(const FmCall& c, uint32_t q_total, uint32_t n_clean, bool with_chain, uint32_t runstate_cap,
                               uint32_t chain_run_quads = fm_chain_run_quads(5u), bool staged = false, uint32_t Da = 0u, uint32_t park_stages = 0u,
                               uint64_t lds_waves = 0u) {
  const uint32_t q_steps = fm_q_steps(c.M), q_quads = fm_q_quads(c.M);
  uint32_t runs = q_total / n_clean;
  const uint32_t min_steps = fm_q_min_steps(n_clean, q_steps, q_total);
  if (runs > q_steps / min_steps) runs = q_steps / min_steps;
  // (the sink's chain inside the launch: every run must own more outputs than its predecessor's state reaches — fm_chain_run_quads —: a small call is cut
  // into fewer runs for it)
  if (with_chain && runs > q_quads / chain_run_quads) runs = q_quads / chain_run_quads;
  if (runs < 1) runs = 1;
  if (staged && Da && min_steps == 4u && n_clean > 1u && runs > 1u) {
    uint32_t least = (uint32_t)((lds_waves + 2ull * n_clean - 1u) / (2ull * n_clean));
    if (least < 1u) least = 1u;
    const uint32_t fill_stages = fm_q_run_shape(c.M, runs, true, Da).stages;
    uint32_t best = runs;
    uint64_t best_cost = ~0ull;
    for (uint32_t r = runs; r >= least; --r) {
      const FmRunShape s = fm_q_run_shape(c.M, r, true, Da);
      if (s.stages > fill_stages || s.stages > park_stages) break;   // (fewer runs are longer still)
      const uint64_t cost = fm_q_runs_cost(r, s);
      if (cost < best_cost) { best_cost = cost; best = r; }
    }
    runs = best;
  }
  // (the runs' hand-off words were allocated for the largest grid: a launch they cannot hold goes without the chain)
  if (with_chain && (uint64_t)n_clean * runs > runstate_cap) with_chain = false;
  return FmRuns{runs, with_chain};
}
// audio stages of ONE stream's waves in this call: what the call adds to its routing window
static inline uint64_t fm_win_stages(uint32_t runs, uint32_t q_steps, uint32_t Da) {
  return (uint64_t)runs * ((q_steps / runs + Da - 1) / Da);
}

// ---- buffers -----------------------------------------------------------------------------------------------------------------------------
// Do rows [a + i sa, a + i sa + la) and [b + j sb, b + j sb + lb), i, j < n, share a byte?  Exact for equal strides (two views of one
// buffer at different offsets do not); otherwise the two whole ranges are compared.
static inline bool fm_rows_overlap(const uint8_t* a, size_t sa, size_t la, const uint8_t* b, size_t sb, size_t lb, uint32_t n) {
  if (!a || !b || n == 0 || la == 0 || lb == 0) return false;
  const uintptr_t ua = (uintptr_t)a, ub = (uintptr_t)b;
  if (n == 1 || sa != sb || sa == 0) {
    const uintptr_t ea = ua + (uintptr_t)(n - 1) * sa + la, eb = ub + (uintptr_t)(n - 1) * sb + lb;
    return ua < eb && ub < ea;
  }
  // row i of a and row j of b start d - (i - j) s apart (d = b - a): they share a byte iff that distance lies in (-lb, la) for some
  // i - j in (-n, n), that is iff an integer of (-n, n) lies in ((d - la) / s, (d + lb) / s).  (Rows no longer than the stride: floor(d / s) or
  // a neighbour, the three candidates this function used to try; rows LONGER than the stride — a buffer whose own rows overlap — reach further.)
  const long long s = (long long)sa, d = (long long)(ub - ua);
  const long long x = d - (long long)la, y = d + (long long)lb;
  long long lo = (x >= 0 ? x / s : -((-x + s - 1) / s)) + 1;    // floor(x / s) + 1
  long long hi = (y > 0 ? (y + s - 1) / s : -(-y / s)) - 1;     // ceil(y / s) - 1
  if (lo < 1 - (long long)n) lo = 1 - (long long)n;
  if (hi > (long long)n - 1) hi = (long long)n - 1;
  return lo <= hi;
}

#endif
