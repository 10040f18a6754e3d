// The arithmetic of the limiter's true-peak form in csrc/sdrfm_limit.h, compiled for the host alone and run under ASan and UBSan
// by tests/test_limit_tp_cpu.py: the lane's sums over the packed, tap-reversed table against the 64-bit sum of the definition — at x' = +-2^19
// on every tap, with tables AT the half-row bound of sdrfm_truepeak_check_coef, and on random rows over the full 20-bit range — the detector's
// rounding up, and the window geometry the kernel uses (every window inside the plane for every shape the constructor takes).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_limit.h"

static int fails = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

// the 64-bit sums, straight from the definition: a[c][p] = sum_k coef[p][k] x_c[last - k]
static void direct(const int32_t* xl, const int32_t* xr, const int16_t* coef, uint32_t P, uint32_t nt, int64_t a[2][SDRFM_TP_PHASES_MAX]) {
  for (uint32_t p = 0; p < P; ++p) {
    a[0][p] = a[1][p] = 0;
    for (uint32_t k = 0; k < nt; ++k) {
      a[0][p] += (int64_t)coef[p * nt + k] * xl[nt - 1 - k];
      a[1][p] += (int64_t)coef[p * nt + k] * xr[nt - 1 - k];
    }
  }
}

static void one_case(const int32_t* xl, const int32_t* xr, const int16_t* coef, uint32_t P, uint32_t nt) {
  uint32_t tab[SDRFM_TP_TABLE_DWORDS];
  tp_pack_table(coef, P, nt, tab);
  int64_t want[2][SDRFM_TP_PHASES_MAX], got[2][SDRFM_TP_PHASES_MAX];
  direct(xl, xr, coef, P, nt, want);
  limit_tp_values(xl, xr, tab, P, nt, got);
  uint64_t T = 0;
  for (uint32_t p = 0; p < P; ++p)
    for (int c = 0; c < 2; ++c) {
      CHECK(got[c][p] == want[c][p]);
      CHECK(tp_abs(want[c][p]) < (1ull << 36));
      T = tp_abs(want[c][p]) > T ? tp_abs(want[c][p]) : T;
    }
  CHECK(limit_tp_peak(xl, xr, tab, P, nt) == T);
}

// a table whose every half-row has sum |coef| == 65535 exactly, with the signs from `pattern`
static void bound_table(std::vector<int16_t>& coef, uint32_t P, uint32_t nt, uint32_t pattern) {
  coef.assign((size_t)P * nt, 0);
  const uint32_t half = nt / 2;
  for (uint32_t p = 0; p < P; ++p)
    for (uint32_t h = 0; h < 2; ++h) {
      int16_t* row = coef.data() + (size_t)p * nt + h * half;
      uint32_t left = 65535u;
      for (uint32_t k = 0; k < half; ++k) {
        const uint32_t most = left < 32767u ? left : 32767u;
        uint32_t v = (k + 1 == half || half == 2) ? most : (pattern & 8u ? most : rnd() % (most + 1u));
        if (half == 2 && k == 0) v = 32767u;
        if (half == 2 && k == 1) v = 32768u;                      // only -32768 reaches it
        left -= v;
        const bool neg = ((pattern >> ((k + p + h) % 3u)) & 1u) != 0 || v == 32768u;
        row[k] = (int16_t)(neg ? -(int32_t)v : (int32_t)v);
      }
    }
}

int main() {
  // every shape, tables at the bound, rows on the rails and random
  const uint32_t shapes[][2] = {{4, 12}, {8, 4}, {2, 64}, {8, 64}, {2, 4}, {4, 32}};
  for (const auto& sh : shapes) {
    const uint32_t P = sh[0], nt = sh[1];
    CHECK(tp_shape_ok(P, nt));
    std::vector<int16_t> coef;
    std::vector<int32_t> xl(nt), xr(nt);
    for (uint32_t pattern = 0; pattern < 16; ++pattern) {
      bound_table(coef, P, nt, pattern);
      for (uint32_t p = 0; p < P; ++p)                                // the table is AT the bound, and the library takes it
        for (uint32_t h = 0; h < 2; ++h) {
          uint32_t sum = 0;
          for (uint32_t k = 0; k < nt / 2; ++k) sum += (uint32_t)std::abs((int)coef[p * nt + h * (nt / 2) + k]);
          CHECK(sum <= 65535u && (pattern & 8u ? sum == 65535u : true));
        }
      // the rails, with the signs of row 0 (the largest possible |A|) and against them
      for (uint32_t k = 0; k < nt; ++k) {
        xl[nt - 1 - k] = coef[k] < 0 ? -(1 << 19) : (1 << 19);
        xr[nt - 1 - k] = coef[k] < 0 ? (1 << 19) : -(1 << 19);
      }
      one_case(xl.data(), xr.data(), coef.data(), P, nt);
      for (uint32_t k = 0; k < nt; ++k) { xl[k] = 1 << 19; xr[k] = -(1 << 19); }
      one_case(xl.data(), xr.data(), coef.data(), P, nt);
      for (int rep = 0; rep < 50; ++rep) {
        for (uint32_t k = 0; k < nt; ++k) {
          xl[k] = (int32_t)(rnd() % ((1u << 20) + 1u)) - (1 << 19);
          xr[k] = (rnd() & 3u) ? (int32_t)(rnd() % ((1u << 20) + 1u)) - (1 << 19) : ((rnd() & 1u) ? (1 << 19) : -(1 << 19));
        }
        one_case(xl.data(), xr.data(), coef.data(), P, nt);
      }
    }
  }
  // the detector: the oversampled peak is rounded UP to an LSB, the samples count as they are
  CHECK(limit_detect_tp(0, 0, 0, 1) == 32768u);
  CHECK(limit_detect_tp(0, 0, 32768, 1) == 32768u);                  // exactly 1 LSB
  CHECK(limit_detect_tp(0, 0, 32769, 1) == 16384u);                  // a hair over: 2 LSB
  CHECK(limit_detect_tp(100, -100, 100ull << 15, 100) == 32768u);
  CHECK(limit_detect_tp(100, -100, (100ull << 15) + 1, 100) == (100u << 15) / 101u);
  CHECK(limit_detect_tp(-(1 << 19), 0, 0, 32767) == limit_detect(-(1 << 19), 0, 32767));
  CHECK(limit_detect_tp(0, 0, 2ull * 65535 * (1ull << 19), 32767) == (32767u << 15) / (uint32_t)((2ull * 65535 * (1ull << 19) + 32767) >> 15));
  // the geometry: for every shape the constructor takes, every window of every pair of a full tile lies inside the x' plane
  for (uint32_t lw = SDRFM_LIMIT_LW_MIN; lw <= SDRFM_LIMIT_LW_MAX; ++lw)
    for (uint32_t nt = SDRFM_TP_TAPS_MIN; nt <= SDRFM_TP_TAPS_MAX; nt += 4) {
      if (!limit_tp_window_ok(lw, nt)) continue;
      const uint32_t D = (1u << lw) - 1u, LX = D + nt / 2u;
      CHECK(LX + 1u >= nt);                                            // the first pair's window starts at entry LX - (NT - 1) >= 0
      CHECK(LX + SDRFM_LIMIT_TILE <= SDRFM_LIMIT_ARRAY_TP);
      CHECK(limit_tp_state_words(lw, nt) == 2u * LX + 2u * D && limit_tp_latency(lw, nt) == LX);
    }
  CHECK(limit_tp_lds_bytes() <= 160u * 1024u && limit_tp_lds_bytes() == 87680u);
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
