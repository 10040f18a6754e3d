/* The FM call path's host arithmetic (csrc/sdrfm_fm_call.h) on a CPU, under UBSan (tests/test_fm_call_cpu.py builds and runs this).
 *
 * No parity test sees this arithmetic: the bit-exact designs give the same bits however a stream is segmented, design Q however it is cut into runs.
 * Three kinds of check:
 *   known answers   figures DESIGN.md and the code's comments state for the headline shape (not taken from the functions under test)
 *   properties      over a seeded sweep of shapes, stream counts, call sizes and routed fractions; who serves a call and which bit-exact kernel is launched
 *                   are asked of the functions enqueue() and launch_bx() themselves call (fm_serve, fm_bx)
 *   fm_rows_overlap against a brute-force byte-set intersection
 * Every FmGeom is the one the library plans for the shape (csrc/sdrfm_fm_plan.h) from what an MI355X answers (fm_geom.h), not a hand-written one.
 * Prints "ok" and exits 0, or says what failed and exits 1. */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_fm_call.h"
#include "fm_geom.h"

static int g_failed = 0;
#define CHECK(cond, ...)                                                         \
  do {                                                                           \
    if (!(cond)) {                                                               \
      if (g_failed < 20) { printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
      ++g_failed;                                                                \
    }                                                                            \
  } while (0)

static uint64_t g_rng = 0x5d2f3a11c0ffee01ull;                   // the sweep's seed
static uint64_t rnd() {                                          // splitmix64
  uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static uint32_t rnd_in(uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rnd() % ((uint64_t)hi - lo + 1)); }

// a default handle of shape (T, D, Ta, Da) as the library plans it (tests/native/fm_geom.h)
struct Shape { uint32_t T, D, Ta, Da; };
static FmGeom geom(const Shape& sh, uint32_t ns, bool bit_exact = false) { return fm_test_geom(sh.T, sh.D, sh.Ta, sh.Da, ns, bit_exact, fm_test_facts_mi355x(sh.T, sh.D, sh.Da)); }

static FmCall call_of(uint32_t phase_x, uint32_t phase_d, uint32_t nbytes, const FmGeom& g, uint64_t n_seen, bool al4, bool al16) {
  const FmCounts n = fm_counts(phase_x, phase_d, nbytes, g.D, g.Da);
  return FmCall{n.N, n.M, n.A, phase_x, phase_d, n_seen, al4, al16};
}

// ---- known answers (T 64, D 10, Ta 32, Da 5; 256 CUs, 12 design-Q waves and 12 mixed workgroups per CU) -------------------------------------------
static void known_answers() {
  const Shape sh = {64, 10, 32, 5};
  CHECK(fm_chain_run_quads(5) == 13u && fm_chain_run_quads(8) == 18u && fm_chain_run_quads(1) == 13u, "quads per run under the sink's chain: %u, %u", fm_chain_run_quads(5), fm_chain_run_quads(8));
  const uint64_t seen = 1u << 20;                                // (a stream well past its first T-1 samples)
  {  // 256 streams x 480 000 B: design Q fits, 12 runs per stream, 3072 workgroups
    const FmGeom g = geom(sh, 256);
    const FmCall c = call_of(0, 0, 480000, g, seen, true, true);
    CHECK(c.N == 240000 && c.M == 24000 && c.A == 4800, "%u %u %u", c.N, c.M, c.A);
    CHECK(fm_q_fit(g, c), "headline batch");
    const FmSplit s = fm_split(g, c, false, false, 0);
    const FmRuns r = fm_q_runs(c, s.q_total, 256, false, 0);
    CHECK(s.q_total == 3072 && r.runs == 12 && 256 * r.runs == 3072, "%u %u", s.q_total, r.runs);
    // design Q refuses: an odd decimator phase, N no multiple of D Da 8, a row not 16-byte aligned, M < Ta
    CHECK(!fm_q_fit(g, call_of(1, 0, 480000, g, seen, true, true)), "odd phase");
    CHECK(!fm_q_fit(g, call_of(0, 0, 480000 + 2 * 200, g, seen, true, true)), "N %% 400");
    CHECK(!fm_q_fit(g, call_of(0, 0, 480000, g, seen, true, false)), "alignment");
    FmGeom g1030 = geom(sh, 1030);                    // (1030 streams x 1 step fill the machine: only M < Ta is left to refuse 40 outputs)
    CHECK(fm_q_fit(g1030, call_of(0, 0, 800, g1030, seen, true, true)), "40 outputs, 32 audio taps");
    g1030.Ta = 48;
    CHECK(!fm_q_fit(g1030, call_of(0, 0, 800, g1030, seen, true, true)), "M < Ta");
  }
  {  // 1 stream x 4 800 000 B: fits, 1875 steps, 937 two-step runs; 1 stream x 480 000 B: 188 steps < 2 per CU
    const FmGeom g = geom(sh, 1);
    const FmCall c = call_of(0, 0, 4800000, g, seen, true, true);
    CHECK(fm_q_fit(g, c) && fm_q_steps(c.M) == 1875, "%u", fm_q_steps(c.M));
    const FmRuns r = fm_q_runs(c, fm_split(g, c, false, false, 0).q_total, 1, false, 0);
    CHECK(r.runs == 937 && fm_q_min_steps(1, 1875, 3072) == 2, "%u", r.runs);
    const FmCall c1 = call_of(0, 0, 480000, g, seen, true, true);
    CHECK(fm_q_steps(c1.M) == 188 && !fm_q_fit(g, c1), "%u", fm_q_steps(c1.M));
  }
  {  // 256 streams x 480 000 B on a bit-exact handle: design S, 8 waves per stream
    const FmGeom g = geom(sh, 256, true);
    const FmCall c = call_of(0, 0, 480000, g, seen, true, true);
    CHECK(!fm_q_fit(g, c) && fm_stream_ok(g, c, 256, false) && fm_s_waves(g, c) == 8, "%u", fm_s_waves(g, c));
    const FmBx b = fm_bx(g, c, 256, g.waves_target, false);
    CHECK(fm_serve(g, c, 0).bx_all && b.kind == 's' && b.tiles.grid == 2048 && b.halo_bytes, "%c %u", b.kind, b.tiles.grid);
  }
  {  // 64 of 256 streams routed, one launch: 16 segments of 6 sub-tiles (1024 design-B workgroups), 2048 design-Q workgroups, 10 runs of 76 quads
     // (profiles/r06_mixed_split.txt)
    const FmGeom g = geom(sh, 256);
    const FmCall c = call_of(0, 0, 480000, g, seen, true, true);
    const FmServe sv = fm_serve(g, c, 64);
    CHECK(sv.q_ok && !sv.bx_all && sv.mixed && sv.fuse, "fused");
    CHECK(fm_serve(g, c, 128).bx_all && fm_serve(g, c, 127).mixed, "half of the streams routed: the bit-exact kernels take the batch");
    const FmSplit s = fm_split(g, c, true, true, 64);
    const FmTiles t = fm_b_tiles(g, c, 64, s.bx_waves, true);
    const FmRuns r = fm_q_runs(c, s.q_total, 192, false, 0);
    CHECK(s.bx_waves == 1024 && s.q_total == 2048, "%u %u", s.bx_waves, s.q_total);
    CHECK(t.tiles_per_stream == 16 && t.grid == 1024 && t.fold_state == 1 && (t.NA * 5 + 255) / 256 == 6, "%u %u %u", t.tiles_per_stream, t.grid, t.NA);
    CHECK(r.runs == 10 && (fm_q_quads(c.M) + r.runs + r.runs - 1) / r.runs == 76, "%u", r.runs);
  }
  // the buffer-size bound: ceil(n / D) + 1 decimated outputs, ceil of that / Da, + 1 audio outputs
  CHECK(fm_max_audio(10, 5, 480000) == 4802 && fm_max_audio(10, 5, 0) == 2 && fm_max_audio(8, 8, 2 * 2049) == 34 && fm_max_audio(16, 5, 0xfffffffeu) == 26843547,
        "%u %u %u %u", fm_max_audio(10, 5, 480000), fm_max_audio(10, 5, 0), fm_max_audio(8, 8, 2 * 2049), fm_max_audio(16, 5, 0xfffffffeu));
  {  // the first-call fix-up: 8 outputs touch never-seen samples, 8 audio outputs (<= 64: one tile)
    const FmGeom g = geom(sh, 256);
    const FmFixup f = fm_fixup(g, call_of(0, 0, 480000, g, 0, true, true));
    CHECK(f.y_aff == 8 && f.a_aff == 8 && f.tiles_per_stream == 1, "%u %u %u", f.y_aff, f.a_aff, f.tiles_per_stream);
  }
}

// ---- properties ----------------------------------------------------------------------------------------------------------------------------
static void check_tiles(const FmTiles& t, const FmCall& c, uint32_t nsub, const char* what) {
  CHECK(nsub == 0 || c.A == 0 || t.tiles_per_stream >= 1, "%s: a stream without a workgroup", what);
  CHECK((int64_t)t.tiles_per_stream * t.NA >= (int64_t)c.A && (int64_t)c.A > ((int64_t)t.tiles_per_stream - 1) * t.NA,
        "%s: tiles %u NA %u A %u", what, t.tiles_per_stream, t.NA, c.A);
  const uint64_t grid = (uint64_t)nsub * t.tiles_per_stream + (t.fold_state ? 0u : nsub);
  CHECK(grid == t.grid && grid <= 0xffffffffull, "%s: grid %" PRIu64 " / %u", what, grid, t.grid);
}

// top: 0 = a drawn call size; 1 = the largest call, 2^30 - 1 samples; 2 = the largest one design Q may take (a multiple of 8 D Da below 2^30)
static void one_case(const Shape& sh, int top = 0) {
  const uint32_t T = sh.T, D = sh.D, Da = sh.Da;
  const uint32_t ns = (rnd() & 3) ? rnd_in(1, 1030) : rnd_in(1, 8);
  FmGeom g = geom(sh, ns);
  if ((rnd() & 15) == 0) g.mix_lds = 0;                          // (no one-launch instance: the two-launch split)
  if ((rnd() & 15) == 0) g.has_s = false;
  if ((rnd() & 31) == 0) g.has_mix_tile = false, g.mix_lds = 0;
  g.waves_target = g.n_cu * rnd_in(4, 16);
  if ((rnd() & 3) == 0) g.fast_R = 4u * rnd_in(1, 3);
  // a call: from one audio period to 2^30 - 1 samples; half of them as design Q wants them (phase 0, whole groups of 8 audio periods, aligned rows)
  const uint32_t period = D * Da, n_max = (1u << 30) - 1u;
  const bool tidy = top ? top == 2 : (rnd() & 1);
  const uint32_t scale = 1u << rnd_in(0, 30);
  uint32_t N = top ? n_max : rnd_in(period, period + scale);
  if (N > n_max) N = n_max;
  if (tidy) { N -= N % (period * 8u); if (N == 0) N = period * 8u; }
  const uint32_t phase_x = tidy ? 0u : rnd_in(0, D - 1), phase_d = tidy ? 0u : rnd_in(0, Da - 1);
  const uint64_t n_seen = (rnd() & 7) ? (1u << 20) : rnd_in(0, T);
  const FmCall c = call_of(phase_x, phase_d, 2u * N, g, n_seen, tidy || (rnd() & 1), tidy);
  // who serves the call (fm_serve), with a drawn share of the streams routed when design Q can take it
  const uint32_t routed_pct = (rnd() & 1) ? 0u : rnd_in(0, 100);
  const uint32_t n_noisy = fm_q_fit(g, c) ? (uint32_t)((uint64_t)ns * routed_pct / 100u) : 0u, n_clean = ns - n_noisy;
  const FmServe sv = fm_serve(g, c, n_noisy);
  const bool q_ok = sv.q_ok, mixed = sv.mixed, fuse = sv.fuse;
  CHECK(sv.bx_all != q_ok && (!mixed || q_ok) && (!fuse || mixed) && (!q_ok || (n_clean > 0 && 2 * n_noisy < ns)), "served by neither or both: %d %d %d %d", q_ok, sv.bx_all, mixed, fuse);
  const FmSplit s = fm_split(g, c, mixed, fuse, n_noisy);
  if (fuse) {
    const uint32_t total = g.mix_waves_per_cu * g.n_cu;
    CHECK((uint64_t)s.bx_waves + s.q_total <= total || s.q_total == n_clean, "fused split: %u + %u of %u, %u clean", s.bx_waves, s.q_total, total, n_clean);
    CHECK(s.bx_waves >= n_noisy && s.q_total >= n_clean, "fused split: %u for %u routed, %u for %u clean", s.bx_waves, n_noisy, s.q_total, n_clean);
    const double share = (g.mix_cost * n_noisy) / ((double)n_clean + g.mix_cost * n_noisy);
    uint32_t by_share = (uint32_t)((double)total * share + 0.5);
    if (by_share < n_noisy) by_share = n_noisy;
    CHECK(s.bx_waves == by_share || s.bx_waves % n_noisy == 0, "the search's choice: %u waves for %u routed streams", s.bx_waves, n_noisy);
  }
  if (mixed || !q_ok) {
    const uint32_t nsub = mixed ? n_noisy : ns;
    const FmBx b = fm_bx(g, c, nsub, s.bx_waves, mixed);          // the kernel launch_bx() launches, and its cut
    if (b.kind == 's') {
      const uint32_t w = b.tiles.tiles_per_stream;
      CHECK(w >= 1 && (uint64_t)w * 63 * g.seg >= c.N && (uint64_t)nsub * w <= 0xffffffffull && b.tiles.grid == nsub * w, "design S: %u waves", w);
      CHECK(g.has_s && !mixed && b.halo_bytes, "design S without an instance, or beside design Q");
    } else {
      check_tiles(b.tiles, c, nsub, b.kind == 'b' ? "design B" : "generic");
      CHECK(b.kind == 'g' || (b.kind == 'b' && g.has_fast && (!b.small_tile || (mixed && g.has_mix_tile))), "a tile the handle does not have: %c %d", b.kind, b.small_tile);
    }
  }
  if (q_ok) {
    const uint32_t steps = fm_q_steps(c.M), cap = g.q_waves_per_cu * g.n_cu;
    const bool want_chain = fm_chain_fits(g, c, q_ok, mixed, fuse) && (rnd() & 1);
    const FmRuns r = fm_q_runs(c, s.q_total, n_clean, want_chain, cap, fm_chain_run_quads(Da));
    const uint32_t min_steps = fm_q_min_steps(n_clean, steps, s.q_total);
    CHECK(r.runs >= 1 && (r.runs == 1 || (uint64_t)r.runs * min_steps <= steps), "runs %u x %u of %u steps", r.runs, min_steps, steps);
    CHECK((uint64_t)n_clean * r.runs <= 0xffffffffull, "design Q's grid");
    const uint32_t rq = fm_chain_run_quads(Da);                   // 13 at Da = 5, 18 at Da = 8: the owned quads hold more than SDRFM_FM_CHAIN_FIX audio outputs wherever the run is cut
    CHECK(rq >= 13u && (uint64_t)(rq - 1u) * 32u >= (uint64_t)(SDRFM_FM_CHAIN_FIX + 2u) * Da, "%u quads per run at Da %u", rq, Da);
    CHECK(!r.with_chain || (want_chain && fm_q_quads(c.M) / r.runs >= rq && (uint64_t)n_clean * r.runs <= cap), "chain: %u runs over %u quads", r.runs,
          fm_q_quads(c.M));
    CHECK(!want_chain || fm_q_quads(c.M) / r.runs >= rq, "a run of fewer than %u quads: %u runs over %u quads", rq, r.runs, fm_q_quads(c.M));
    CHECK(fm_win_stages(r.runs, steps, Da) >= 1, "window stages");
  }
  if (c.n_seen + 1 < T) {
    const FmFixup f = fm_fixup(g, c);
    CHECK((uint64_t)f.tiles_per_stream * g.NA < (uint64_t)c.A + g.NA && (f.tiles_per_stream >= 1 || c.A == 0), "fix-up: %u tiles, A %u", f.tiles_per_stream, c.A);
    CHECK((uint64_t)f.tiles_per_stream * g.NA >= (f.a_aff < c.A ? f.a_aff : c.A), "fix-up covers %u of %u", f.tiles_per_stream * g.NA, f.a_aff);
  }
}

// the counts of any cut of a capture sum to the one-shot counts; the phases after the cuts are the phases after the one-shot call
static void one_cut(uint32_t D, uint32_t Da) {
  const uint32_t px = rnd_in(0, D - 1), pd = rnd_in(0, Da - 1);
  uint32_t total_n = rnd_in(0, 1u << rnd_in(1, 30));               // up to 2^30 - 1 samples, the most a call may hold
  if (total_n > (1u << 30) - 1u || (rnd() & 63) == 0) total_n = (1u << 30) - 1u;
  const uint32_t total = 2u * total_n;
  const FmCounts whole = fm_counts(px, pd, total, D, Da);
  uint32_t x = px, d = pd, left = total;
  uint64_t sn = 0, sm = 0, sa = 0;
  uint32_t most = 0;
  for (int cut = 0; left; ++cut) {
    uint32_t nb = (cut == 12) ? left : 2u * rnd_in(0, left / 2);
    const FmCounts n = fm_counts(x, d, nb, D, Da);
    sn += n.N; sm += n.M; sa += n.A; x = n.phase_x; d = n.phase_d; left -= nb;
    if (fm_max_audio(D, Da, nb) > most) most = fm_max_audio(D, Da, nb);
    CHECK(n.A <= fm_max_audio(D, Da, nb), "fm_max_audio(%u) = %u < %u", nb, fm_max_audio(D, Da, nb), n.A);
  }
  CHECK(sn == whole.N && sm == whole.M && sa == whole.A && x == whole.phase_x && d == whole.phase_d,
        "cuts of %u B at phases %u, %u: %" PRIu64 " %" PRIu64 " %" PRIu64 " -> %u %u; one shot %u %u %u -> %u %u", total, px, pd, sn, sm, sa, x, d, whole.N,
        whole.M, whole.A, whole.phase_x, whole.phase_d);
}

// ---- fm_rows_overlap against the byte sets ---------------------------------------------------------------------------------------------------
static uint8_t g_arena[1024];
static void rows_overlap_brute() {
  uint8_t* const a = g_arena + 512;
  uint8_t mark[1024];
  unsigned long cases = 0;
  for (uint32_t n = 1; n <= 6; ++n)
    for (size_t sa = 0; sa <= 14; ++sa)
      for (size_t la = 0; la <= 12; ++la)
        for (size_t lb = 0; lb <= 12; ++lb)
          for (int sbi = 0; sbi < 3; ++sbi) {
            // equal strides (where the function is exact) in full; unequal ones (the whole ranges are compared) for a few lengths
            const size_t sb = sbi == 0 ? sa : (sbi == 1 ? sa + 1 + la % 3 : sa / 2);
            if (sbi && (sb == sa || (la % 4 != 1) || (lb % 5 != 2))) continue;
            memset(mark, 0, sizeof(mark));
            for (uint32_t i = 0; i < n; ++i) for (size_t k = 0; k < la; ++k) mark[512 + i * sa + k] = 1;
            for (int off = -100; off <= 100; ++off) {
              const uint8_t* b = a + off;
              bool brute = false;
              for (uint32_t j = 0; j < n && !brute; ++j) for (size_t k = 0; k < lb; ++k) if (mark[512 + off + (long)(j * sb + k)]) { brute = true; break; }
              const bool got = fm_rows_overlap(a, sa, la, b, sb, lb, n), rev = fm_rows_overlap(b, sb, lb, a, sa, la, n);
              ++cases;
              CHECK(got == rev, "order: n %u sa %zu la %zu sb %zu lb %zu off %d: %d / %d", n, sa, la, sb, lb, off, got, rev);
              if (n == 1 || sa == sb) {
                // (stride 0: every row is the first row — the whole ranges ARE the byte sets; stride < length and identical buffers included)
                CHECK(got == brute, "n %u stride %zu la %zu lb %zu off %d: %d, byte sets %d", n, sa, la, lb, off, got, brute);
              } else {
                const bool hull = la && lb && (long)0 < off + (long)((n - 1) * sb + lb) && off < (long)((n - 1) * sa + la);
                CHECK(got == hull && (!brute || got), "n %u sa %zu la %zu sb %zu lb %zu off %d: %d, ranges %d, byte sets %d", n, sa, la, sb, lb, off, got, hull, brute);
              }
            }
          }
  CHECK(!fm_rows_overlap(nullptr, 4, 4, a, 4, 4, 2) && !fm_rows_overlap(a, 4, 4, nullptr, 4, 4, 2) && !fm_rows_overlap(a, 4, 4, a, 4, 4, 0), "null / empty");
  // interleaved disjoint rows: two views of one buffer, 8 bytes each of every 16
  CHECK(!fm_rows_overlap(a, 16, 8, a + 8, 16, 8, 6) && fm_rows_overlap(a, 16, 8, a + 7, 16, 8, 6) && fm_rows_overlap(a, 16, 8, a, 16, 8, 6), "interleaved rows");
  printf("rows_overlap: %lu cases\n", cases);
}

int main() {
  known_answers();
  // every shape the library has fast kernels for: (T, D, Ta, Da); design Q's instances are (D, Da) = (10, 5), (8, 8), (16, 5) at 32 audio taps
  static const Shape shapes[] = {{64, 10, 32, 5}, {32, 10, 32, 5}, {16, 10, 32, 5}, {64, 8, 32, 8}, {16, 8, 32, 8}, {64, 4, 32, 8}, {64, 16, 32, 5}};
  unsigned long cases = 0;
  for (const Shape& sh : shapes)
    for (int i = 0; i < 40000; ++i, ++cases) one_case(sh, i < 400 ? 1 + (i & 1) : 0);
  for (const Shape& sh : shapes)
    for (int i = 0; i < 3000; ++i) one_cut(sh.D, sh.Da);
  printf("sweep: seed 0x5d2f3a11c0ffee01, %lu cases\n", cases);
  rows_overlap_brute();
  if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
  printf("ok\n");
  return 0;
}
