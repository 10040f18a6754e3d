// The rate matcher's count, advance and span arithmetic (csrc/sdrfm_pcm_rate.h) held to naive 128-bit arithmetic: a program of its own, built with
// ASan and UBSan by tests/test_pcm_rate_cpu.py and run as a program.  Prints "ok" at the end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_pcm_rate.h"

typedef unsigned __int128 u128;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    if (!(cond)) {                                                        \
      fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);          \
      fprintf(stderr, __VA_ARGS__);                                       \
      fprintf(stderr, "\n");                                              \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

// the j >= 0 with pos + j step < n 2^32, counted without a division
static uint32_t naive_count(uint64_t pos, uint64_t step, uint32_t n) {
  const u128 N = (u128)n << 32;
  if ((u128)pos >= N) return 0;
  u128 lo = 0, hi = ((u128)1 << 23);                                      // the first j at or beyond the end lies in (lo, hi]
  while (hi - lo > 1) {
    const u128 mid = (lo + hi) / 2;
    if ((u128)pos + mid * step < N) lo = mid; else hi = mid;
  }
  return (uint32_t)hi;
}

static void check_case(uint64_t pos, uint64_t step, uint32_t n) {
  const uint32_t cnt = rate_count(pos, step, n), want = naive_count(pos, step, n);
  CHECK(cnt == want, "pos %llu step %llu n %u: %u != %u", (unsigned long long)pos, (unsigned long long)step, n, cnt, want);
  const u128 N = (u128)n << 32;
  if (cnt) {
    CHECK((u128)pos + (u128)(cnt - 1) * step < N, "the last output lies beyond the input");
    CHECK((u128)pos + (u128)cnt * step >= N, "one more output would fit");
  }
  const u128 next = (u128)pos + (u128)cnt * step - N;                     // >= 0 either way
  CHECK((u128)rate_advance(pos, step, n, cnt) == next, "advance: pos %llu step %llu n %u", (unsigned long long)pos, (unsigned long long)step, n);
}

// the spans of one call tile [0, cnt) exactly once, in order, and every window lies inside [-(nt - 1), n) and inside the plane the launch reserves
static void check_spans(uint64_t pos, uint64_t step, uint32_t n, uint32_t nt, uint32_t logph, uint64_t max_step) {
  const uint32_t cnt = rate_count(pos, step, n);
  const uint32_t span = rate_span_len(max_step, nt, logph), plane = rate_plane_dwords(span, max_step, nt);
  CHECK(span >= SDRFM_RATE_NT && span <= SDRFM_RATE_SPAN_MAX && span % SDRFM_RATE_NT == 0, "span %u", span);
  CHECK(rate_lds_bytes(span, max_step, nt, logph) <= SDRFM_RATE_LDS_BYTES, "LDS %u", rate_lds_bytes(span, max_step, nt, logph));
  const uint32_t spans = cnt ? (cnt + span - 1) / span : 1;
  uint32_t at = 0;
  for (uint32_t b = 0; b < spans + 2; ++b) {                              // two beyond the grid: they take nothing
    uint32_t first, count, w;
    int64_t w0;
    rate_span(pos, step, cnt, span, b, nt, &first, &count, &w0, &w);
    if (b >= spans || !cnt) { CHECK(count == 0, "span %u behind the end takes %u", b, count); continue; }
    CHECK(first == at && count >= 1 && count <= span, "span %u: first %u count %u at %u", b, first, count, at);
    at += count;
    const int64_t i_first = (int64_t)(((u128)pos + (u128)first * step) >> 32), i_last = (int64_t)(((u128)pos + (u128)(first + count - 1) * step) >> 32);
    CHECK(w0 == i_first - (int64_t)nt + 1 && w0 + (int64_t)w == i_last + 1, "span %u: window [%lld, +%u)", b, (long long)w0, w);
    CHECK(w0 >= -(int64_t)(nt - 1) && w0 + (int64_t)w <= (int64_t)n, "span %u: window [%lld, +%u) outside [-%u, %u)", b, (long long)w0, w, nt - 1, n);
    const int64_t a0 = w0 & ~(int64_t)1;                                  // as the kernel stages it
    CHECK(a0 <= w0 && w0 - a0 <= 1, "even start");
    const uint64_t need = (uint64_t)((w0 + (int64_t)w - a0 + 1) / 2) + 1;
    CHECK(need <= plane, "span %u: %llu dwords in a plane of %u", b, (unsigned long long)need, plane);
    // the last lane's fetch: dword (q0 >> 1) + nt / 2 of the plane
    const uint64_t q0 = (uint64_t)(i_last - (int64_t)nt + 1 - a0);
    CHECK((q0 >> 1) + nt / 2 < need, "span %u: a lane fetches behind the staged dwords", b);
  }
  CHECK(at == cnt, "the spans cover %u of %u", at, cnt);
}

int main() {
  const uint64_t steps[] = {SDRFM_RATE_STEP_MIN, SDRFM_RATE_STEP_MIN + 1, ((uint64_t)1 << 32) - 429497, (uint64_t)1 << 32, ((uint64_t)1 << 32) + 429497,
                            4674794336ull /* 48 / 44.1 */, SDRFM_RATE_STEP_MAX - 1, SDRFM_RATE_STEP_MAX};
  const uint32_t ns[] = {0, 1, 2, 3, 63, 64, 4800, SDRFM_RATE_N_MAX - 1, SDRFM_RATE_N_MAX};
  for (uint64_t step : steps)
    for (uint32_t n : ns) {
      const uint64_t N = (uint64_t)n << 32;
      const uint64_t poss[] = {0, 1, step - 1, step, N ? N - 1 : 0, N, N + 1, N + step, 0xFFFFFFFFull, (uint64_t)1 << 32, ((uint64_t)1 << 34) - 1};
      for (uint64_t pos : poss) check_case(pos, step, n);
    }
  for (int t = 0; t < 200000; ++t) {
    const uint64_t step = SDRFM_RATE_STEP_MIN + rnd() % (SDRFM_RATE_STEP_MAX - SDRFM_RATE_STEP_MIN + 1);
    const uint32_t n = (t & 1) ? (uint32_t)(rnd() % (SDRFM_RATE_N_MAX + 1)) : (uint32_t)(rnd() % 70);
    const uint64_t pos = (t & 2) ? rnd() % (step + 1) : rnd() % ((((uint64_t)n + 2) << 32) + 1);   // below a step, as between calls; or anywhere round the end
    check_case(pos, step, n);
  }
  // spans: every table shape's extremes, steps mixed in one launch (the span length follows the largest)
  const uint32_t nts[] = {4, 32, 64}, logphs[] = {4, 8};
  const uint32_t span_ns[] = {1, 2, 3, 31, 32, 63, 64, 65, 1023, 1024, 1025, 4800, 16384};
  for (uint32_t nt : nts)
    for (uint32_t logph : logphs)
      for (uint64_t step : steps)
        for (uint64_t max_step : {step, (uint64_t)SDRFM_RATE_STEP_MAX})
          for (uint32_t n : span_ns) {
            const uint64_t poss[] = {0, 1, step - 1, step / 2, 0xFFFFFFFFull, ((uint64_t)n << 32) - 1, (uint64_t)n << 32, rnd() % step};
            for (uint64_t pos : poss) check_spans(pos, step, n, nt, logph, max_step);
          }
  check_spans(0, SDRFM_RATE_STEP_MIN, SDRFM_RATE_N_MAX, 64, 8, SDRFM_RATE_STEP_MAX);         // 2^22 outputs
  check_spans(12345, SDRFM_RATE_STEP_MAX, SDRFM_RATE_N_MAX, 64, 8, SDRFM_RATE_STEP_MAX);
  for (int t = 0; t < 3000; ++t) {
    const uint64_t step = SDRFM_RATE_STEP_MIN + rnd() % (SDRFM_RATE_STEP_MAX - SDRFM_RATE_STEP_MIN + 1);
    const uint32_t nt = 4 * (1 + (uint32_t)(rnd() % 16)), logph = 4 + (uint32_t)(rnd() % 5);
    check_spans(rnd() % step, step, (uint32_t)(rnd() % 20000), nt, logph, (t & 1) ? step : step + rnd() % (SDRFM_RATE_STEP_MAX - step + 1));
  }
  // the mixing step's rounding and rails
  if (rate_mix(0, 0, 0) != 0 || rate_mix((int64_t)1 << 15, 0, 0) != 1 || rate_mix(((int64_t)1 << 14) - 1, 0, 0) != 0 || rate_mix((int64_t)1 << 14, 0, 0) != 1 ||
      rate_mix(-((int64_t)1 << 14), 0, 0) != 0 || rate_mix(-((int64_t)1 << 14) - 1, 0, 0) != -1 || rate_mix((int64_t)1 << 31, (int64_t)1 << 31, 128) != 32767 ||
      rate_mix(-((int64_t)1 << 31), -((int64_t)1 << 31), 255) != -32768 || rate_mix(32767 * 32768ll, 32767 * 32768ll, 77) != 32767 ||
      rate_mix(0, (int64_t)1 << 15, 128) != 1 || rate_mix(0, (int64_t)1 << 15, 127) != 0) {
    fprintf(stderr, "rate_mix\n");
    return 1;
  }
  printf("ok\n");
  return 0;
}
