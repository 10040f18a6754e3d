// The arithmetic of csrc/sdrfm_limit.h on the host, held to one-pair-at-a-time iteration: the (min, +) maps and their composition with the
// clamp, the release scanned in the kernel's order — a lane's chunk, the wave by doubling steps, the waves in order, the carry from tile to
// tile — against sequential evaluation, the doubling minimum and the doubling sum against the naive window for every LW, the per-pair
// arithmetic at its extremes, and the record join with its associativity and its ties.  Built with ASan and UBSan and run as a program
// (tests/test_limit_cpu.py): an index outside an array, a shift too far or a signed overflow stops it.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <random>
#include <vector>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_limit.h"

static int fails = 0;
#define CHECK(c)                                                                 \
  do {                                                                           \
    if (!(c)) {                                                                  \
      if (++fails < 20) std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
    }                                                                            \
  } while (0)

static std::mt19937_64 rng(20240611);
static uint32_t below(uint32_t n) { return (uint32_t)(rng() % n); }

// a window minimum m in Q15: mostly 32768, sometimes deep, sometimes 0
static uint32_t some_m() {
  const uint32_t k = below(8);
  return k < 4 ? 32768u : (k == 4 ? 0u : (k == 5 ? below(32769u) : 30000u + below(2769u)));
}

static void check_maps() {
  const uint32_t deltas[] = {1u, 874u, 5000u, (1u << 23) - 1u, 1u << 23};
  const uint32_t rs[] = {0u, 1u, 255u, 256000u, (1u << 23) - 1u, 1u << 23};
  const limit_map id = limit_map_identity();
  for (uint32_t d1 : deltas)
    for (uint32_t d2 : deltas)
      for (int rep = 0; rep < 40; ++rep) {
        const limit_map f1 = limit_map_of(some_m(), d1), f2 = limit_map_of(some_m(), d2), f3 = limit_map_of(some_m(), d1);
        const limit_map f21 = limit_compose(f2, f1), f32 = limit_compose(f3, f2);
        const limit_map l = limit_compose(f3, f21), r = limit_compose(f32, f1);
        CHECK(l.a == r.a && l.b == r.b);                          // associative, with the clamp
        CHECK(f21.b <= SDRFM_LIMIT_R_ONE && f21.a <= SDRFM_LIMIT_R_ONE);
        const limit_map i1 = limit_compose(id, f1), i2 = limit_compose(f1, id);
        CHECK(i1.a == f1.a && i1.b == f1.b && i2.a == f1.a && i2.b == f1.b);
        for (uint32_t r0 : rs) {
          CHECK(limit_apply(f21, r0) == limit_apply(f2, limit_apply(f1, r0)));
          CHECK(limit_apply(l, r0) == limit_apply(f3, limit_apply(f2, limit_apply(f1, r0))));
          CHECK(limit_apply(id, r0) == r0);
          // against the unclamped definition in 64 bits
          const uint64_t a = std::min<uint64_t>(f2.a, (uint64_t)f1.a + f2.b), b = (uint64_t)f1.b + f2.b;
          CHECK(limit_apply(f21, r0) == std::min<uint64_t>(a, (uint64_t)r0 + b));
        }
      }
  // a tile-long run of the largest delta: b stays clamped
  limit_map f = id;
  for (uint32_t k = 0; k < SDRFM_LIMIT_TILE; ++k) f = limit_compose(limit_map_of(32768u, 1u << 23), f);
  CHECK(f.b == SDRFM_LIMIT_R_ONE && f.a == SDRFM_LIMIT_R_ONE);
}

// the release over a row of n window minima the way the kernel takes it, with `lanes` lanes of `chunk` pairs per tile and waves of `wave` lanes
static void scan_kernel_order(const std::vector<uint32_t>& m, uint32_t delta, uint32_t r0, uint32_t lanes, uint32_t chunk, uint32_t wave,
                              std::vector<uint32_t>& r) {
  const uint32_t tile = lanes * chunk, n = (uint32_t)m.size();
  r.assign(n, 0u);
  uint32_t carry = r0;
  for (uint32_t base = 0; base < n; base += tile) {
    const uint32_t cnt = n - base < tile ? n - base : tile;
    std::vector<limit_map> f(lanes, limit_map_identity());
    for (uint32_t t = 0; t < lanes; ++t)
      for (uint32_t q = 0; q < chunk; ++q) {
        const uint32_t j = t * chunk + q;
        if (j < cnt) f[t] = limit_compose(limit_map_of(m[base + j], delta), f[t]);
      }
    for (uint32_t d = 1; d < wave; d <<= 1) {                    // the inclusive scan of every wave, all lanes at once
      std::vector<limit_map> g(f);
      for (uint32_t t = 0; t < lanes; ++t)
        if ((t % wave) >= d) f[t] = limit_compose(g[t], g[t - d]);
    }
    const uint32_t waves = lanes / wave;
    std::vector<limit_map> wtot(waves);
    for (uint32_t w = 0; w < waves; ++w) wtot[w] = f[w * wave + wave - 1u];
    limit_map tot = limit_map_identity();
    for (uint32_t w = 0; w < waves; ++w) tot = limit_compose(wtot[w], tot);
    for (uint32_t t = 0; t < lanes; ++t) {
      const uint32_t w = t / wave;
      limit_map pre = limit_map_identity();
      for (uint32_t v = 0; v < w; ++v) pre = limit_compose(wtot[v], pre);
      const limit_map before = (t % wave) ? f[t - 1u] : limit_map_identity();
      uint32_t x = limit_apply(before, limit_apply(pre, carry));
      for (uint32_t q = 0; q < chunk; ++q) {
        const uint32_t j = t * chunk + q;
        if (j < cnt) { x = limit_apply(limit_map_of(m[base + j], delta), x); r[base + j] = x; }
      }
    }
    carry = limit_apply(tot, carry);
    CHECK(carry == r[base + cnt - 1u]);
  }
}

static void check_scan() {
  const uint32_t deltas[] = {1u, 874u, 1u << 23};
  for (uint32_t delta : deltas)
    for (int shape = 0; shape < 4; ++shape) {
      const uint32_t lanes = shape == 0 ? SDRFM_LIMIT_NT : 16u << shape, chunk = shape == 0 ? SDRFM_LIMIT_CHUNK : (uint32_t)(2 * shape + 1),
                     wave = shape == 0 ? 64u : 8u;
      const uint32_t tile = lanes * chunk;
      const uint32_t ns[] = {1u, chunk, chunk + 1u, wave * chunk, wave * chunk + 1u, tile - 1u, tile, tile + 1u, 2u * tile + 3u};
      for (uint32_t n : ns)
        for (int kind = 0; kind < 3; ++kind) {
          std::vector<uint32_t> m(n);
          for (uint32_t i = 0; i < n; ++i) m[i] = kind == 0 ? some_m() : (kind == 1 ? (i == n / 3 ? 0u : 32768u) : 32768u);
          const uint32_t r0 = kind == 2 ? 0u : (kind == 1 ? SDRFM_LIMIT_R_ONE : below(SDRFM_LIMIT_R_ONE + 1u));
          std::vector<uint32_t> want(n), got;
          uint64_t x = r0;
          for (uint32_t i = 0; i < n; ++i) { x = std::min<uint64_t>(256ull * m[i], x + delta); want[i] = (uint32_t)x; }
          scan_kernel_order(m, delta, r0, lanes, chunk, wave, got);
          CHECK(got == want);
        }
    }
}

static void check_windows() {
  for (uint32_t lw = SDRFM_LIMIT_LW_MIN; lw <= SDRFM_LIMIT_LW_MAX; ++lw) {
    const uint32_t W = 1u << lw, D = W - 1u;
    const uint32_t lens[] = {D + 1u, D + 2u, 2u * D + 1u, D + 700u};
    for (uint32_t len : lens)
      for (int kind = 0; kind < 2; ++kind) {
        std::vector<uint32_t> a(len);
        for (uint32_t i = 0; i < len; ++i) a[i] = kind ? SDRFM_LIMIT_R_ONE - below(2u) * below(SDRFM_LIMIT_R_ONE + 1u) : some_m();
        const std::vector<uint32_t> src(a);
        std::vector<uint32_t> mn(src), sm(src), tmp(len);
        for (uint32_t k = 0; k < lw; ++k) {
          for (uint32_t i = 0; i < len; ++i) tmp[i] = limit_win_min(mn.data(), i, 1u << k);
          mn.swap(tmp);
          for (uint32_t i = 0; i < len; ++i) tmp[i] = limit_win_sum(sm.data(), i, 1u << k);
          sm.swap(tmp);
        }
        for (uint32_t i = D; i < len; ++i) {                     // entries behind the lead-in are whole windows
          uint32_t m = 0xFFFFFFFFu;
          uint64_t s = 0;
          for (uint32_t k = 0; k <= D; ++k) { m = std::min(m, src[i - k]); s += src[i - k]; }
          CHECK(mn[i] == m);
          CHECK(s <= (1ull << 31) && sm[i] == s);
          CHECK(limit_smooth(sm[i], lw) <= SDRFM_LIMIT_ONE && limit_smooth(sm[i], lw) == (uint32_t)((s / W) >> 8));
        }
      }
  }
}

static void check_pair_arithmetic() {
  const int16_t xs[] = {-32768, -32767, -1, 0, 1, 2, 12345, 32767};
  const uint32_t Gs[] = {0u, 1u, 4095u, 4096u, 4097u, 20000u, 65535u, 65536u};
  const uint32_t Cs[] = {1u, 2u, 12000u, 29204u, 32767u};
  for (int16_t x : xs)
    for (uint32_t G : Gs) {
      const int64_t p = (int64_t)x * (int64_t)G + 2048;
      const int64_t want = p >= 0 ? p / 4096 : -((-p + 4095) / 4096);   // floor
      CHECK(limit_gain(x, G) == want);
      CHECK(limit_gain(x, 4096u) == x);
      for (int16_t y : xs)
        for (uint32_t C : Cs) {
          const int32_t l = limit_gain(x, G), r = limit_gain(y, G);
          const uint32_t g = limit_detect(l, r, C);
          const uint64_t a = std::max<uint64_t>((uint64_t)std::llabs((long long)l), (uint64_t)std::llabs((long long)r));
          CHECK(g == (a <= C ? 32768u : (uint32_t)(((uint64_t)C * 32768u) / a)));
          for (uint32_t s : {0u, g ? 1u : 0u, g / 2u, g}) {               // any s <= g keeps the pair under the ceiling, rounding included
            CHECK(std::abs((int)limit_out(l, s)) <= (int)C && std::abs((int)limit_out(r, s)) <= (int)C);
            const int64_t q = (int64_t)l * s + 16384;
            CHECK(limit_out(l, s) == (q >= 0 ? q / 32768 : -((-q + 32767) / 32768)));
          }
        }
      CHECK(limit_out(x, 32768u) == x);
    }
}

static sdrfm_pcm_limit_rec rec_of_run(const std::vector<uint32_t>& s, size_t lo, size_t hi) {
  sdrfm_pcm_limit_rec m = {hi - lo, 0, SDRFM_LIMIT_ONE, 0};
  for (size_t i = lo; i < hi; ++i) {
    if (s[i] < m.min_gain) { m.min_gain = s[i]; m.at = i - lo; }
    m.limited += s[i] < SDRFM_LIMIT_ONE;
  }
  return m;
}
static bool same(const sdrfm_pcm_limit_rec& a, const sdrfm_pcm_limit_rec& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

static void check_records() {
  const sdrfm_pcm_limit_rec id = {0, 0, SDRFM_LIMIT_ONE, 0};
  for (int rep = 0; rep < 300; ++rep) {
    const size_t n = 1 + below(60);
    std::vector<uint32_t> s(n);
    for (auto& v : s) v = below(4) ? 32768u : 32760u + below(8u);   // few values: ties are common
    const size_t c1 = below((uint32_t)n + 1u), c2 = c1 + below((uint32_t)(n - c1) + 1u);
    const sdrfm_pcm_limit_rec a = rec_of_run(s, 0, c1), b = rec_of_run(s, c1, c2), c = rec_of_run(s, c2, n), whole = rec_of_run(s, 0, n);
    sdrfm_pcm_limit_rec l = a, bc = b, r = a, e = id, f = a;
    limit_join(&l, &b); limit_join(&l, &c);                       // (a b) c
    limit_join(&bc, &c); limit_join(&r, &bc);                     // a (b c)
    limit_join(&e, &a);                                           // the identity on either side
    limit_join(&f, &id);
    CHECK(same(l, whole) && same(r, whole) && same(e, a) && same(f, a));
    // the key reduction in any order gives the run's record
    uint64_t key = limit_key_none(), cnt = 0;
    for (size_t i = n; i-- > 0;) { key = limit_key_min(key, limit_key(s[i], (uint32_t)i)); cnt += s[i] < SDRFM_LIMIT_ONE; }
    sdrfm_pcm_limit_rec k;
    limit_rec_of(key, n, cnt, &k);
    CHECK(same(k, whole));
  }
  sdrfm_pcm_limit_rec none;
  limit_rec_of(limit_key_none(), 0, 0, &none);
  CHECK(same(none, id));
}

int main() {
  CHECK(limit_state_words(2) == 12u && limit_state_words(8) == 1020u);
  CHECK(limit_tiles(0) == 0u && limit_tiles(1) == 1u && limit_tiles(SDRFM_LIMIT_TILE) == 1u && limit_tiles(SDRFM_LIMIT_TILE + 1u) == 2u);
  CHECK(SDRFM_LIMIT_ARRAY >= SDRFM_LIMIT_TILE + SDRFM_LIMIT_D_MAX && limit_lds_bytes() <= 160u * 1024u && SDRFM_LIMIT_CHUNK % 2u == 1u);
  check_maps();
  check_scan();
  check_windows();
  check_pair_arithmetic();
  check_records();
  if (fails) { std::printf("%d checks failed\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}
