// The lane arithmetic of csrc/sdrfm_truepeak.h on the host: the table packing, the planes, the odd and even alignment of a window, the two
// half-rows, the key reduction and the join, held to the definition (a 64-bit sum per value, a first-maximum search) over every alignment and
// every table shape the library accepts.  emulate() walks a call the way the kernel does — tiles, planes staged behind their nt predecessors,
// lanes in any order — with a tile length of its own, so that short rows cross tile borders.  Built with ASan and UBSan and run as a program
// (tests/test_truepeak_cpu.py): an index outside a plane or the table, a shift by 64 or a signed overflow stops it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_truepeak.h"

static int fails = 0;
#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) {                                                                  \
      if (++fails < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                                            \
  } while (0)

static bool same(const sdrfm_truepeak& a, const sdrfm_truepeak& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

// the definition: one call of n pairs, joined onto acc; hist advanced
static void define(const std::vector<int16_t>& pcm, uint32_t n, const std::vector<int16_t>& coef, uint32_t P, uint32_t nt, uint64_t limit,
                   std::vector<int16_t>& hist, sdrfm_truepeak* acc) {
  sdrfm_truepeak m;
  std::memset(&m, 0, sizeof(m));
  m.n = n;
  auto x = [&](int64_t idx, int ch) -> int64_t { return idx >= 0 ? pcm[2 * (size_t)idx + ch] : hist[2 * (size_t)((int64_t)nt - 1 + idx) + ch]; };
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t p = 0; p < P; ++p) {
      int64_t a[2] = {0, 0};
      for (uint32_t k = 0; k < nt; ++k)
        for (int ch = 0; ch < 2; ++ch) a[ch] += (int64_t)coef[p * nt + k] * x((int64_t)i - k, ch);
      const uint64_t ml = (uint64_t)(a[0] < 0 ? -a[0] : a[0]), mr = (uint64_t)(a[1] < 0 ? -a[1] : a[1]);
      if (ml > m.peak_l) { m.peak_l = ml; m.at_l = i; }
      if (mr > m.peak_r) { m.peak_r = mr; m.at_r = i; }
      m.over_l += ml > limit;
      m.over_r += mr > limit;
    }
  if (m.peak_l > acc->peak_l) { acc->peak_l = m.peak_l; acc->at_l = acc->n + m.at_l; }
  if (m.peak_r > acc->peak_r) { acc->peak_r = m.peak_r; acc->at_r = acc->n + m.at_r; }
  acc->n += n;
  acc->over_l += m.over_l;
  acc->over_r += m.over_r;
  std::vector<int16_t> all(hist);
  all.insert(all.end(), pcm.begin(), pcm.begin() + 2 * (size_t)n);
  hist.assign(all.end() - 2 * (size_t)(nt - 1), all.end());
}

// the kernel's walk with the header's functions: tile pairs per tile (even), lanes visited backwards to show that their order does not matter
static void emulate(const std::vector<int16_t>& pcm, uint32_t n, const std::vector<int16_t>& coef, uint32_t P, uint32_t nt, uint64_t limit, uint32_t tile,
                    std::vector<int16_t>& hist, sdrfm_truepeak* acc) {
  if (n == 0) return;
  std::vector<uint32_t> tab(P * (nt / 2));
  tp_pack_table(coef.data(), P, nt, tab.data());
  auto fetch = [&](int64_t idx, int ch) -> int16_t {
    if (idx >= 0) return idx < (int64_t)n ? pcm[2 * (size_t)idx + ch] : (int16_t)0;
    return idx >= -(int64_t)(nt - 1) ? hist[2 * (size_t)((int64_t)nt - 1 + idx) + ch] : (int16_t)0;
  };
  uint64_t key[2] = {0, 0}, over[2] = {0, 0};
  for (uint64_t base = 0; base < n; base += tile) {
    const uint32_t cnt = n - base < tile ? (uint32_t)(n - base) : tile;
    const int64_t a0 = (int64_t)base - nt;
    const uint32_t need = (cnt >> 1) + nt / 2 + 1;
    std::vector<uint32_t> pl(need), pr(need);                    // exactly what the kernel stages: ASan sees a fetch beyond it
    for (uint32_t q = 0; q < need; ++q) {
      pl[q] = tp_pack2(fetch(a0 + 2 * (int64_t)q, 0), fetch(a0 + 2 * (int64_t)q + 1, 0));
      pr[q] = tp_pack2(fetch(a0 + 2 * (int64_t)q, 1), fetch(a0 + 2 * (int64_t)q + 1, 1));
    }
    for (uint32_t r = cnt; r-- > 0;) {
      const uint32_t q0 = r + 1;
      int64_t a[2][SDRFM_TP_PHASES_MAX];
      tp_lane_pair(pl.data() + (q0 >> 1), pr.data() + (q0 >> 1), (q0 & 1u) * 16u, tab.data(), P, nt, a);
      for (int ch = 0; ch < 2; ++ch) {
        uint32_t o = 0;
        tp_take(a[ch], P, (uint32_t)base + r, limit, &key[ch], &o);
        over[ch] += o;
      }
    }
  }
  sdrfm_truepeak call;
  call.n = n;
  call.peak_l = tp_key_peak(key[0]); call.at_l = tp_key_at(key[0]); call.over_l = over[0];
  call.peak_r = tp_key_peak(key[1]); call.at_r = tp_key_at(key[1]); call.over_r = over[1];
  call.reserved = 0;
  tp_join(acc, &call);
  std::vector<int16_t> all(hist);
  all.insert(all.end(), pcm.begin(), pcm.begin() + 2 * (size_t)n);
  hist.assign(all.end() - 2 * (size_t)(nt - 1), all.end());
}

// a random table inside the bound: every half-row scaled to a chosen sum of |coef|
static std::vector<int16_t> random_table(std::mt19937& g, uint32_t P, uint32_t nt, bool at_bound) {
  std::vector<int16_t> c(P * nt);
  const uint32_t half = nt / 2;
  for (uint32_t p = 0; p < P; ++p)
    for (uint32_t h = 0; h < 2; ++h) {
      uint32_t left = at_bound ? SDRFM_TP_HALF_MAX : g() % (SDRFM_TP_HALF_MAX + 1u);
      for (uint32_t k = 0; k < half; ++k) {
        uint32_t mag = k + 1 == half ? (left > 32767u ? 32767u : left) : (left ? g() % ((left > 32767u ? 32767u : left) + 1u) : 0u);
        left -= mag;
        c[p * nt + h * half + k] = (int16_t)((g() & 1u) ? -(int32_t)mag : (int32_t)mag);
      }
      if (at_bound && left) {                                    // spend the rest on taps of -32768: nt = 4 has two taps per half
        for (uint32_t k = 0; k < half && left; ++k) {
          int16_t& t = c[p * nt + h * half + k];
          const uint32_t mag = (uint32_t)(t < 0 ? -t : t), room = 32768u - mag, add = left < room ? left : room;
          t = (int16_t)(-(int32_t)(mag + add));
          left -= add;
        }
      }
    }
  return c;
}

static uint32_t half_sum(const std::vector<int16_t>& c, uint32_t nt, uint32_t p, uint32_t h) {
  uint32_t s = 0;
  for (uint32_t k = 0; k < nt / 2; ++k) { const int32_t v = c[p * nt + h * (nt / 2) + k]; s += (uint32_t)(v < 0 ? -v : v); }
  return s;
}

static std::vector<int16_t> random_pcm(std::mt19937& g, uint32_t n, int kind) {
  std::vector<int16_t> x(2 * (size_t)n);
  for (auto& v : x) {
    const uint32_t r = g();
    v = kind == 0 ? (int16_t)(r & 0xFFFFu) : ((r & 1u) ? (int16_t)32767 : (int16_t)-32768);
  }
  return x;
}

int main() {
  std::mt19937 g(20261020u);
  // the packing and the operand
  CHECK(tp_pack2(-1, 2) == 0x0002FFFFu && tp_pack2(-32768, 32767) == 0x7FFF8000u);
  CHECK(tp_operand(0x22221111u, 0x44443333u, 0) == 0x22221111u && tp_operand(0x22221111u, 0x44443333u, 16) == 0x33332222u);
  CHECK(tp_dot2(tp_pack2(-32768, -32768), tp_pack2(-32768, 32767), 5) == 5 + (1 << 30) - 32768 * 32767);
  CHECK(tp_key_at(tp_key(0, 7)) == 0 && tp_key_peak(tp_key(0, 7)) == 0 && tp_key_at(tp_key(9, 7)) == 7 && tp_key_peak(tp_key(0xFFFF0000ull, 0xFFFFFFFFu)) == 0xFFFF0000ull);
  CHECK(tp_key_max(tp_key(5, 3), tp_key(5, 2)) == tp_key(5, 2) && tp_key_max(tp_key(5, 3), tp_key(6, 9)) == tp_key(6, 9));
  for (uint32_t P = 0; P <= 9; ++P)
    for (uint32_t nt = 0; nt <= 70; ++nt) CHECK(tp_shape_ok(P, nt) == ((P == 2 || P == 4 || P == 8) && nt >= 4 && nt <= 64 && nt % 4 == 0));

  // every accepted shape; rows of every length around the history and across tiles of 8 and 14 pairs (either parity of every window start);
  // a cut into calls against one call; full-range and rail input; limits from 0 to the top
  const uint32_t Ps[3] = {2, 4, 8};
  for (uint32_t P : Ps)
    for (uint32_t nt = 4; nt <= 64; nt += 4)
      for (int bound = 0; bound < 2; ++bound) {
        const std::vector<int16_t> coef = random_table(g, P, nt, bound != 0);
        for (uint32_t p = 0; p < P; ++p)
          for (uint32_t h = 0; h < 2; ++h) CHECK(bound ? half_sum(coef, nt, p, h) == SDRFM_TP_HALF_MAX : half_sum(coef, nt, p, h) <= SDRFM_TP_HALF_MAX);
        const uint64_t limits[4] = {0, (uint64_t)1 << 30, (uint64_t)g(), SDRFM_TP_LIMIT_MAX};
        const uint64_t limit = limits[g() % 4];
        const uint32_t lens[8] = {1, 2, nt - 2, nt - 1, nt, 29, 3 * nt + 1, 70};
        for (uint32_t tile : {8u, 14u}) {
          sdrfm_truepeak want, got, whole;
          std::memset(&want, 0, sizeof(want));
          got = whole = want;
          std::vector<int16_t> hw(2 * (nt - 1), 0), hg(hw), hwhole(hw), all;
          for (uint32_t n : lens) {
            const std::vector<int16_t> pcm = random_pcm(g, n, bound);
            define(pcm, n, coef, P, nt, limit, hw, &want);
            emulate(pcm, n, coef, P, nt, limit, tile, hg, &got);
            CHECK(same(want, got));
            CHECK(hw == hg);
            all.insert(all.end(), pcm.begin(), pcm.end());
          }
          define(all, (uint32_t)(all.size() / 2), coef, P, nt, limit, hwhole, &whole);
          CHECK(same(whole, got));                               // any cut, joined in order, is the stream's record
          CHECK(hwhole == hg);
        }
      }

  // a table at the bound, every tap negative, against a constant -32768: every product positive, 2 * 65535 * 32768, the top of the key
  for (uint32_t P : Ps)
    for (uint32_t nt : {4u, 12u, 64u}) {
      std::vector<int16_t> coef(P * nt, 0);
      for (uint32_t p = 0; p < P; ++p)
        for (uint32_t h = 0; h < 2; ++h) {
          coef[p * nt + h * (nt / 2) + p % (nt / 2)] = -32768;
          coef[p * nt + h * (nt / 2) + (p + 1) % (nt / 2)] = -32767;
        }
      const uint32_t n = 2 * nt + 3;
      std::vector<int16_t> pcm(2 * (size_t)n, -32768), hw(2 * (nt - 1), 0), hg(hw);
      sdrfm_truepeak want, got;
      std::memset(&want, 0, sizeof(want));
      got = want;
      define(pcm, n, coef, P, nt, 4294901759ull, hw, &want);
      emulate(pcm, n, coef, P, nt, 4294901759ull, 14, hg, &got);
      CHECK(same(want, got));
      CHECK(got.peak_l == 4294901760ull && got.peak_r == 4294901760ull && got.over_l > 0);
      sdrfm_truepeak at_limit;
      std::memset(&at_limit, 0, sizeof(at_limit));
      std::vector<int16_t> h2(2 * (nt - 1), 0);
      emulate(pcm, n, coef, P, nt, 4294901760ull, 14, h2, &at_limit);
      CHECK(at_limit.over_l == 0 && at_limit.over_r == 0);       // strict
    }

  // the join: associative on random triples, the zero record its identity, ties to the earlier pair
  for (int it = 0; it < 2000; ++it) {
    sdrfm_truepeak r[3];
    for (auto& x : r) {
      x.n = g() % 100;
      x.peak_l = x.n ? g() % 4 : 0; x.peak_r = x.n ? g() % 4 : 0;
      x.at_l = x.peak_l ? g() % x.n : 0; x.at_r = x.peak_r ? g() % x.n : 0;
      x.over_l = g() % 50; x.over_r = g() % 50; x.reserved = 0;
    }
    sdrfm_truepeak ab = r[0], bc = r[1], left, right, zero;
    tp_join(&ab, &r[1]);
    left = ab;
    tp_join(&left, &r[2]);
    tp_join(&bc, &r[2]);
    right = r[0];
    tp_join(&right, &bc);
    CHECK(same(left, right));
    std::memset(&zero, 0, sizeof(zero));
    sdrfm_truepeak z = zero, y = r[0];
    tp_join(&z, &r[0]);
    tp_join(&y, &zero);
    CHECK(same(z, r[0]) && same(y, r[0]));
    if (r[0].peak_l == r[1].peak_l && r[0].peak_l) CHECK(ab.at_l == r[0].at_l);
  }
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}
