/* Design Q's stage-aligned run count for overlapped calls (csrc/sdrfm_fm_call.h: fm_q_runs with its trailing inputs, fm_q_run_shape, fm_q_runs_cost) on a CPU,
 * under UBSan (tests/test_fm_runs_cpu.py builds and runs this).
 *
 * Design Q gives the same bits however a stream is cut into runs, so no parity test sees a wrong count: the GPU sees it as time only.
 *   known answers   the headline call, worked by hand from the kernel's dealing rule (Gq = Qt + runs - 1 + vs quads dealt evenly, four quads a step, Da steps a stage)
 *   properties      over a seeded sweep of (M, n_clean, Da, overlapped, with_chain)
 * Every FmGeom is the one the library plans for the shape (csrc/sdrfm_fm_plan.h) from what an MI355X answers (fm_geom.h).
 * Prints "ok" and exits 0, or says what failed and exits 1. */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_fm_call.h"
#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_q_host.h"
#include "fm_geom.h"

static int g_failed = 0;
#define CHECK(cond, ...)                                                         \
  do {                                                                           \
    if (!(cond)) {                                                               \
      if (g_failed < 20) { printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
      ++g_failed;                                                                \
    }                                                                            \
  } while (0)

static uint64_t g_rng = 0x71c3a5e90badd00dull;                   // the sweep's seed
static uint64_t rnd() {                                          // splitmix64
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static uint32_t rnd_in(uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rnd() % ((uint64_t)hi - lo + 1)); }

struct Shape { uint32_t T, D, Ta, Da; };
static FmGeom geom(const Shape& sh, uint32_t ns) { return fm_test_geom(sh.T, sh.D, sh.Ta, sh.Da, ns, false, fm_test_facts_mi355x(sh.T, sh.D, sh.Da)); }
static FmCall call_of(uint32_t nbytes, const FmGeom& g) {
  const FmCounts n = fm_counts(0, 0, nbytes, g.D, g.Da);
  return FmCall{n.N, n.M, n.A, 0, 0, 1u << 20, true, true};
}
static const uint32_t PARK = SDRFM_Q_PARK_STAGES;                // (csrc/sdrfm_q_host.h: the constant the kernel's LDS layout is built from)
static uint32_t lds_waves(const FmGeom& g) { return g.q_lds_waves_per_cu; }
// the call as sdrfm.hip makes it for an overlapped plain call, and as it made it before (the six-argument form)
static FmRuns staged(const FmGeom& g, const FmCall& c, uint32_t q_total, uint32_t n_clean, bool chain, bool ovl) {
  return fm_q_runs(c, q_total, n_clean, chain, g.q_waves_per_cu * g.n_cu, fm_chain_run_quads(g.Da), ovl, g.Da, PARK, (uint64_t)lds_waves(g) * g.n_cu);
}
static FmRuns today(const FmGeom& g, const FmCall& c, uint32_t q_total, uint32_t n_clean, bool chain) {
  return fm_q_runs(c, q_total, n_clean, chain, g.q_waves_per_cu * g.n_cu, fm_chain_run_quads(g.Da));
}
// the kernel's own dealing (sdrfm_q.hip: e0, e1): least and most quads of a run, and their sum
static void deal(uint32_t M, uint32_t runs, bool ovl, uint32_t* lo, uint32_t* hi, uint64_t* sum) {
  const uint32_t Gq = fm_q_quads(M) + runs - 1u + (ovl ? 1u : 0u);
  *lo = ~0u; *hi = 0; *sum = 0;
  for (uint32_t r = 0; r < runs; ++r) {
    const uint32_t e0 = (uint32_t)(((uint64_t)r * Gq) / runs), e1 = (uint32_t)(((uint64_t)(r + 1) * Gq) / runs), n = e1 - e0;
    if (n < *lo) *lo = n;
    if (n > *hi) *hi = n;
    *sum += n;
  }
}

static uint64_t cost_of(uint32_t M, uint32_t runs, uint32_t Da) { return fm_q_runs_cost(runs, fm_q_run_shape(M, runs, true, Da)); }
#define SHAPE_IS(M_, runs_, Da_, q_, s_, st_)                                                                                   \
  do { const FmRunShape z_ = fm_q_run_shape(M_, runs_, true, Da_);                                                                \
       CHECK(z_.quads == (q_) && z_.steps == (s_) && z_.stages == (st_), "%u runs: %u quads %u steps %u stages", (unsigned)(runs_), z_.quads, z_.steps, z_.stages); } while (0)

static void known_answers() {
  const Shape sh = {64, 10, 32, 5};
  // the constants as counted (a change to them is a change to every figure below)
  CHECK(SDRFM_FM_Q_RUN_VALU == 200u && SDRFM_FM_Q_STAGE_VALU == 86u && SDRFM_FM_Q_STEP_VALU == 114u && PARK == 4u, "constants");
  {  // the headline call, overlapped: Qt = 750.  12 runs: Gq = 762 -> 64 quads = 16 steps = 4 stages; 11: 761 -> 70 = 18 steps = 4; 10: 760 -> 76 = 19 steps = 4;
     // 9: 759 -> 85 = 22 steps = 5 stages, more than twelve's four: out.  12 x (200 + 344 + 1824) = 28416, 11 x (200 + 344 + 2052) = 28556, 10 x (200 + 344 + 2166)
     // = 27100: ten, and eleven behind twelve, as measured (profiles/q_runs_ab.txt)
    const FmGeom g = geom(sh, 256);
    const FmCall c = call_of(480000, g);
    const uint32_t q_total = fm_split(g, c, false, false, 0).q_total;
    CHECK(lds_waves(g) == 15 && q_total == 3072 && fm_q_quads(c.M) == 750, "%u %u", lds_waves(g), q_total);
    SHAPE_IS(c.M, 12, 5, 64, 16, 4); SHAPE_IS(c.M, 11, 5, 70, 18, 4); SHAPE_IS(c.M, 10, 5, 76, 19, 4); SHAPE_IS(c.M, 9, 5, 85, 22, 5);
    CHECK(cost_of(c.M, 12, 5) == 28416 && cost_of(c.M, 11, 5) == 28556 && cost_of(c.M, 10, 5) == 27100, "costs");
    CHECK(staged(g, c, q_total, 256, false, true).runs == 10, "%u", staged(g, c, q_total, 256, false, true).runs);
    // the same call through the old argument forms, and as a serial call: 12
    CHECK(fm_q_runs(c, q_total, 256, false, 0).runs == 12 && today(g, c, q_total, 256, false).runs == 12, "old forms");
    CHECK(staged(g, c, q_total, 256, false, false).runs == 12, "a serial call keeps the count");
    // the window's stages follow the count: 36 -> 40 per call
    CHECK(fm_win_stages(12, fm_q_steps(c.M), 5) == 36 && fm_win_stages(10, fm_q_steps(c.M), 5) == 40, "window stages");
  }
  {  // 512 streams: six runs of 126 quads = 32 steps = seven stages fill the machine (they flush in their loop today); nothing below them is considered: six stay
    const FmGeom g = geom(sh, 512);
    const FmCall c = call_of(480000, g);
    const uint32_t q_total = fm_split(g, c, false, false, 0).q_total;
    SHAPE_IS(c.M, 6, 5, 126, 32, 7);
    CHECK(today(g, c, q_total, 512, false).runs == 6 && staged(g, c, q_total, 512, false, true).runs == 6, "%u", staged(g, c, q_total, 512, false, true).runs);
  }
  {  // a 0.05 s call (Qt = 375): 12 runs x 33 quads = 9 steps = 2 stages: 12 x (200 + 172 + 1026) = 16776; 11 x 36 quads = 9 steps: 15378; 10 x 39 quads = 10 steps = 2
     // full stages: 10 x (200 + 172 + 1140) = 15120; 9 x 43 quads = 11 steps = 3 stages: out.  Ten.
    const FmGeom g = geom(sh, 256);
    const FmCall c = call_of(240000, g);
    const uint32_t q_total = fm_split(g, c, false, false, 0).q_total;
    SHAPE_IS(c.M, 12, 5, 33, 9, 2); SHAPE_IS(c.M, 11, 5, 36, 9, 2); SHAPE_IS(c.M, 10, 5, 39, 10, 2); SHAPE_IS(c.M, 9, 5, 43, 11, 3);
    CHECK(cost_of(c.M, 12, 5) == 16776 && cost_of(c.M, 11, 5) == 15378 && cost_of(c.M, 10, 5) == 15120, "costs");
    CHECK(today(g, c, q_total, 256, false).runs == 12 && staged(g, c, q_total, 256, false, true).runs == 10, "%u", staged(g, c, q_total, 256, false, true).runs);
  }
  {  // a single stream x 1 s keeps its 937 two-step runs
    const FmGeom g = geom(sh, 1);
    const FmCall c = call_of(4800000, g);
    CHECK(staged(g, c, fm_split(g, c, false, false, 0).q_total, 1, false, true).runs == 937, "one stream");
  }
  {  // (8, 8), 256 streams x 0.1 s: M = 25600, Qt = 800, stages of eight steps.  12 runs x 68 quads = 17 steps = 3 stages: 12 x (200 + 258 + 1938) = 28752;
     // 11 x 74 = 19 steps: 28864; 10 x 81 = 21 steps: 28520; 9 x 90 = 23 steps = 3 stages: 9 x (200 + 258 + 2622) = 27720; 8 x 101 = 26 steps = 4 stages: out.
     // 14 waves fit a CU by LDS: two calls hold them from 7 runs on.  Nine.
    const Shape s88 = {64, 8, 32, 8};
    const FmGeom g = geom(s88, 256);
    const FmCall c = call_of(2 * 204800, g);
    const uint32_t q_total = fm_split(g, c, false, false, 0).q_total;
    CHECK(c.M == 25600 && fm_q_quads(c.M) == 800, "%u", c.M);
    SHAPE_IS(c.M, 12, 8, 68, 17, 3); SHAPE_IS(c.M, 11, 8, 74, 19, 3); SHAPE_IS(c.M, 10, 8, 81, 21, 3); SHAPE_IS(c.M, 9, 8, 90, 23, 3); SHAPE_IS(c.M, 8, 8, 101, 26, 4);
    CHECK(cost_of(c.M, 12, 8) == 28752 && cost_of(c.M, 11, 8) == 28864 && cost_of(c.M, 10, 8) == 28520 && cost_of(c.M, 9, 8) == 27720, "costs");
    CHECK(lds_waves(g) == 14 && today(g, c, q_total, 256, false).runs == 12 && staged(g, c, q_total, 256, false, true).runs == 9, "%u %u", lds_waves(g),
          staged(g, c, q_total, 256, false, true).runs);
  }
  {  // (16, 5), 256 streams x 0.1 s: M = 20000, Qt = 625; 11 waves fit a CU by LDS and fill it.  11 runs x 58 quads = 15 steps = 3 full stages; 10 x 64 = 16 steps = 4
     // stages: out.  Eleven stay: the runs are stage-aligned as they are
    const Shape s165 = {64, 16, 32, 5};
    const FmGeom g = geom(s165, 256);
    const FmCall c = call_of(2 * 320000, g);
    const uint32_t q_total = fm_split(g, c, false, false, 0).q_total;
    CHECK(c.M == 20000 && fm_q_quads(c.M) == 625 && lds_waves(g) == 11, "%u %u", c.M, lds_waves(g));
    SHAPE_IS(c.M, 11, 5, 58, 15, 3); SHAPE_IS(c.M, 10, 5, 64, 16, 4);
    CHECK(today(g, c, q_total, 256, false).runs == 11 && staged(g, c, q_total, 256, false, true).runs == 11, "%u", staged(g, c, q_total, 256, false, true).runs);
    // ... and x 0.05 s (Qt = 313): 11 x 30 quads = 8 steps = 2 stages: 11 x (200 + 172 + 912) = 14124; 10 x 33 = 9 steps: 10 x 1398 = 13980; 9 x 36 = 9 steps: 12582;
    // 8 x 41 = 11 steps = 3 stages: out; two calls hold 11 x 256 slots from 6 runs on.  Nine.
    const FmCall h = call_of(2 * 160000, g);
    CHECK(fm_q_quads(h.M) == 313, "%u", fm_q_quads(h.M));
    SHAPE_IS(h.M, 11, 5, 30, 8, 2); SHAPE_IS(h.M, 10, 5, 33, 9, 2); SHAPE_IS(h.M, 9, 5, 36, 9, 2); SHAPE_IS(h.M, 8, 5, 41, 11, 3);
    CHECK(cost_of(h.M, 11, 5) == 14124 && cost_of(h.M, 10, 5) == 13980 && cost_of(h.M, 9, 5) == 12582, "costs");
    CHECK(today(g, h, q_total, 256, false).runs == 11 && staged(g, h, q_total, 256, false, true).runs == 9, "%u", staged(g, h, q_total, 256, false, true).runs);
  }
}

static void sweep() {
  const Shape shapes[3] = {{64, 10, 32, 5}, {64, 8, 32, 8}, {64, 16, 32, 5}};
  uint32_t changed = 0;
  for (int it = 0; it < 20000; ++it) {
    const Shape& sh = shapes[rnd() % 3];
    const uint32_t ns = (rnd() & 3) ? rnd_in(2, 700) : rnd_in(1, 4);
    const FmGeom g = geom(sh, ns);
    const uint32_t unit = sh.D * sh.Da * 8u;
    const FmCall c = call_of(2 * unit * rnd_in(1, (rnd() & 1) ? 120 : 1500), g);
    if (c.M < g.Ta) continue;
    const uint32_t n_clean = rnd_in(ns / 2 + 1, ns);
    const bool ovl = rnd() & 1, chain = rnd() & 1;
    // (the wave slots a launch is cut for: the whole machine's, or a mixed launch's share of it)
    const uint32_t full = g.q_waves_per_cu * g.n_cu, q_total = (rnd() & 1) ? full : rnd_in(n_clean, full > n_clean ? full : n_clean);
    const FmRuns was = today(g, c, q_total, n_clean, chain), now = staged(g, c, q_total, n_clean, chain, ovl);
    const uint32_t steps = fm_q_steps(c.M), quads = fm_q_quads(c.M), min_steps = fm_q_min_steps(n_clean, steps, q_total);
    CHECK(now.runs >= 1 && now.runs <= was.runs, "%u runs, today %u", now.runs, was.runs);
    if (!ovl) CHECK(now.runs == was.runs && now.with_chain == was.with_chain, "a serial call: %u, today %u", now.runs, was.runs);
    if (min_steps == 2 || n_clean == 1) CHECK(now.runs == was.runs, "a call that does not fill the machine: %u, today %u", now.runs, was.runs);
    const FmRunShape s_was = fm_q_run_shape(c.M, was.runs, ovl, sh.Da), s_now = fm_q_run_shape(c.M, now.runs, ovl, sh.Da);
    if (s_was.stages <= PARK) CHECK(s_now.stages <= PARK, "%u runs flush in their loop (%u stages), today's %u do not", now.runs, s_now.stages, was.runs);
    CHECK(s_now.stages <= s_was.stages, "%u runs execute %u stages, today's %u runs %u", now.runs, s_now.stages, was.runs, s_was.stages);
    CHECK(fm_q_runs_cost(now.runs, s_now) <= fm_q_runs_cost(was.runs, s_was), "cost %" PRIu64 " > %" PRIu64, fm_q_runs_cost(now.runs, s_now), fm_q_runs_cost(was.runs, s_was));
    // the old rule's constraints (tests/native/fm_call_check.cpp)
    CHECK(now.runs == 1 || (uint64_t)now.runs * min_steps <= steps, "runs %u x %u of %u steps", now.runs, min_steps, steps);
    if (now.with_chain) CHECK((now.runs == 1 || now.runs <= quads / fm_chain_run_quads(sh.Da)) && (uint64_t)n_clean * now.runs <= full, "chain: %u runs", now.runs);
    if (chain && !now.with_chain) CHECK((uint64_t)n_clean * now.runs > full, "the chain was dropped with room for its words");
    // two calls in flight still hold every wave slot
    if (now.runs != was.runs) { ++changed; CHECK(2ull * now.runs * n_clean >= (uint64_t)lds_waves(g) * g.n_cu, "%u runs x %u streams", now.runs, n_clean); }
    // the kernel's dealing: the runs' quads add up to Gq and differ by one at most; the longest is what the plan reckoned with
    uint32_t lo, hi; uint64_t sum;
    deal(c.M, now.runs, ovl, &lo, &hi, &sum);
    CHECK(sum == (uint64_t)quads + now.runs - 1u + (ovl ? 1u : 0u) && hi - lo <= 1u && hi == s_now.quads, "dealt %u .. %u, sum %" PRIu64 ", planned %u", lo, hi, sum, s_now.quads);
  }
  CHECK(changed > 200, "the sweep met only %u calls whose count changes", changed);
}

int main() {
  known_answers();
  sweep();
  if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
  printf("ok\n");
  return 0;
}
