// The PCM mix bus's launch geometry and per-pair arithmetic (csrc/sdrfm_pcm_mix.h) walked on the CPU: a program of its own, built with ASan and
// UBSan by tests/test_pcm_mix_cpu.py and run as a program.  It plays the kernel's walk — every workgroup, every lane, every one of a lane's
// pairs — so a pair taken twice, a pair missed or a pair outside the row shows; holds the curve's interpolation to its definition over every gain,
// the self-crossfade to 32768 over every pair count, the modes to their table and the sum to its 2^34 bound.  Prints the geometry of a few
// shapes (the test holds the Python mirror to them) and "ok" at the end.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_pcm_mix.h"

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);           \
      exit(1);                                                             \
    }                                                                      \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

// every pair of a row of n exactly once, none at or beyond n
static void walk(uint32_t n) {
  std::vector<uint8_t> times(n, 0);                                  // exactly n: an index at or beyond n is a heap overflow
  const uint32_t spans = pmix_spans(n);
  CHECK(spans <= 512u && (uint64_t)spans * PMIX_SPAN >= n && (spans == 0u || (uint64_t)(spans - 1u) * PMIX_SPAN < n));
  for (uint32_t s = 0; s < spans; ++s) {
    const PmixSpan sp = pmix_span(n, s);
    CHECK(sp.first < sp.end && sp.end <= n && sp.end - sp.first <= PMIX_SPAN && sp.first == s * PMIX_SPAN);
    CHECK(sp.end == n || sp.end - sp.first == PMIX_SPAN);
    for (uint32_t t = 0; t < PMIX_NT; ++t)
      for (uint32_t j = 0; j < PMIX_PER_LANE; ++j) {
        const uint32_t i = pmix_lane_pair(sp.first, t, j);
        if (i < sp.end) times[i] += 1;
      }
  }
  for (uint32_t i = 0; i < n; ++i) CHECK(times[i] == 1);
}

// the definition of step 2, on 64-bit integers
static int64_t curve_def(const uint16_t* t, int64_t g) {
  if (g == 32768) return t[128];
  const int64_t j = g >> 8, f = g & 255;
  return t[j] + ((((int64_t)t[j + 1] - t[j]) * f + 128) >> 8);
}

static void curves() {
  uint16_t lin[PMIX_CURVE_LEN], eqp[PMIX_CURVE_LEN];
  const double pi = 3.14159265358979323846;
  for (uint32_t j = 0; j < PMIX_CURVE_LEN; ++j) {
    lin[j] = (uint16_t)(256u * j);
    eqp[j] = (uint16_t)lround(32768.0 * sin(pi * j / 256.0));
  }
  CHECK(pmix_curve_ok(lin) && pmix_curve_ok(eqp) && eqp[64] == 23170);
  uint32_t last = 0;
  for (uint32_t g = 0; g <= PMIX_ONE; ++g) {
    CHECK(pmix_curve(lin, g) == g);                                  // the linear table changes nothing
    const uint32_t c = pmix_curve(eqp, g);
    CHECK((int64_t)c == curve_def(eqp, g) && (int64_t)pmix_curve(lin, g) == curve_def(lin, g));
    CHECK(c >= last && c <= PMIX_ONE);                               // no decrease between or across knots
    last = c;
  }
  CHECK(pmix_curve(eqp, 0) == 0 && pmix_curve(eqp, PMIX_ONE) == PMIX_ONE);
  // the steepest table the rules take: one step of 32768, whose product with f stays inside 32 bits
  uint16_t step[PMIX_CURVE_LEN];
  for (uint32_t j = 0; j < PMIX_CURVE_LEN; ++j) step[j] = j < 77u ? 0 : 32768;
  CHECK(pmix_curve_ok(step));
  for (uint32_t g = 0; g <= PMIX_ONE; ++g) CHECK((int64_t)pmix_curve(step, g) == curve_def(step, g));
  // what the rules refuse
  uint16_t bad[PMIX_CURVE_LEN];
  for (uint32_t j = 0; j < PMIX_CURVE_LEN; ++j) bad[j] = lin[j];
  bad[0] = 1; CHECK(!pmix_curve_ok(bad)); bad[0] = 0;
  bad[128] = 32767; CHECK(!pmix_curve_ok(bad)); bad[128] = 32768;
  bad[60] = (uint16_t)(bad[59] - 1u); CHECK(!pmix_curve_ok(bad)); bad[60] = lin[60];
  bad[127] = 32769; CHECK(!pmix_curve_ok(bad)); bad[127] = lin[127];
  CHECK(pmix_curve_ok(bad));
}

static void crossfade() {
  static const uint32_t slews[] = {1, 2, 3, 7, 255, 256, 32767, 32768};
  for (uint32_t slew : slews)
    for (uint32_t n = 0; n <= 65537u; ++n) {
      const uint32_t down = audio_ctl_ramp(PMIX_ONE, 0, slew, n), up = audio_ctl_ramp(0, PMIX_ONE, slew, n);
      CHECK(down + up == PMIX_ONE);
      const uint64_t move = (uint64_t)n * slew < PMIX_ONE ? (uint64_t)n * slew : PMIX_ONE;
      CHECK(up == move);
    }
}

static void modes_and_bound() {
  for (uint32_t k = 0; k < 200000u; ++k) {
    const int32_t L = (int16_t)rnd(), R = (int16_t)rnd();
    const int32_t want[PMIX_MODES][2] = {{2 * L, 2 * R}, {L + R, L + R}, {2 * L, 2 * L}, {2 * R, 2 * R}, {2 * R, 2 * L}};
    for (uint32_t m = 0; m < PMIX_MODES; ++m) {
      const PmixWeights w = pmix_weights(m);
      CHECK(w.ll * L + w.lr * R == want[m][0] && w.rl * L + w.rr * R == want[m][1]);
    }
  }
  for (uint32_t m = 0; m < PMIX_MODES; ++m) {                         // |l|, |r| <= 2^16 at the corners
    const PmixWeights w = pmix_weights(m);
    CHECK(w.ll >= 0 && w.lr >= 0 && w.rl >= 0 && w.rr >= 0 && w.ll + w.lr == 2 && w.rl + w.rr == 2);
  }
  CHECK(pmix_acc_bound(PMIX_SLOTS_MAX) == (int64_t)1 << 34);
  // both rails through eight STEREO slots at unity: the sum AT the bound, the value before the clamp at 2^18
  int64_t lo = 0, hi = 0;
  for (uint32_t k = 0; k < PMIX_SLOTS_MAX; ++k) { lo += (int64_t)32768 * (2 * -32768); hi += (int64_t)32768 * (2 * 32767); }
  CHECK(lo == -pmix_acc_bound(PMIX_SLOTS_MAX) && hi < pmix_acc_bound(PMIX_SLOTS_MAX));
  CHECK(pmix_round(lo) == -262144 && pmix_round(hi) == 262136 && pmix_clamp(pmix_round(lo)) == -32768 && pmix_clamp(pmix_round(hi)) == 32767);
  // unity, and MONO never clips
  for (int32_t x = -32768; x <= 32767; ++x) CHECK(pmix_round((int64_t)32768 * 2 * x) == x);
  CHECK(pmix_round((int64_t)32768 * (32767 + 32767)) == 32767 && pmix_round((int64_t)32768 * (-32768 - 32768)) == -32768);
  CHECK(pmix_round((int64_t)32768 * (32767 + 32766)) == 32767 && pmix_round((int64_t)32768 * (-3)) == -1 && pmix_round((int64_t)32768 * (-1)) == 0);
  CHECK(pmix_live(0, 0, 1) && pmix_live(0, 1, 0) && !pmix_live(0, 0, 0) && !pmix_live(PMIX_NONE, PMIX_ONE, PMIX_ONE));
}

int main() {
  for (uint32_t n = 0; n <= 3u * PMIX_SPAN + 3u; ++n) walk(n);
  walk(PMIX_N_MAX);
  curves();
  crossfade();
  modes_and_bound();
  static const uint32_t shapes[][2] = {{1, 0}, {1, 1}, {1, 2047}, {2, 2048}, {5, 2049}, {3, 4099}, {256, 4800}, {1, 70000}, {1, 1u << 20}, {65536, 1u << 20}};
  for (const auto& s : shapes) printf("grid %u %u %u %u\n", s[0], s[1], s[0], pmix_spans(s[1]));
  printf("ok\n");
  return 0;
}
