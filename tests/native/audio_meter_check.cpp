// The run arithmetic of csrc/sdrfm_audio_meter.h on the CPU, a program of its own built with ASan and UBSan:
//   am_mask_runs against a naive loop — every 16-bit mask at every length 1 .. 16, random 64-bit masks at lengths 1 .. 64, all-ones and
//   all-zeros at 64, and junk above the length ignored;
//   am_runs_join and am_meter_join — identity on either side, associativity on random triples, a witness that the join is not commutative;
//   a row cut the way the kernel cuts it (am_wave_stretch, 64 pairs at a time, four waves joined in order) against the whole row.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_audio_meter.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static sdrfm_audio_runs naive(const std::vector<int>& q) {
  sdrfm_audio_runs r = {0, 0, 0, 0};
  uint64_t run = 0;
  bool all = true;
  for (size_t i = 0; i < q.size(); ++i) {
    if (q[i]) { ++r.count; ++run; if (all) r.lead = run; if (run > r.longest) r.longest = run; }
    else { run = 0; all = false; }
  }
  r.trail = run;
  return r;
}

static bool same(const sdrfm_audio_runs& a, const sdrfm_audio_runs& b) {
  return a.count == b.count && a.lead == b.lead && a.trail == b.trail && a.longest == b.longest;
}

static void check_mask(uint64_t mask, uint32_t len) {
  std::vector<int> q(len);
  for (uint32_t i = 0; i < len; ++i) q[i] = (int)((mask >> i) & 1u);
  const sdrfm_audio_runs got = am_mask_runs(mask, len), want = naive(q);
  CHECK(same(got, want), "mask %016llx len %u: got %llu %llu %llu %llu want %llu %llu %llu %llu", (unsigned long long)mask, len,
        (unsigned long long)got.count, (unsigned long long)got.lead, (unsigned long long)got.trail, (unsigned long long)got.longest,
        (unsigned long long)want.count, (unsigned long long)want.lead, (unsigned long long)want.trail, (unsigned long long)want.longest);
}

static sdrfm_audio_meter random_record(std::mt19937_64& g, uint64_t n) {
  // a record some sequence of n pairs has: built from a random predicate sequence so that the runs are consistent with n
  sdrfm_audio_meter m;
  std::memset(&m, 0, sizeof(m));
  m.n = n;
  m.sum_l = (int64_t)(g() >> 3) - (int64_t)(g() >> 3);
  m.sum_r = (int64_t)(g() >> 3) - (int64_t)(g() >> 3);
  m.cross = (int64_t)(g() >> 3) - (int64_t)(g() >> 3);
  m.sq_l = g() >> 2; m.sq_r = g() >> 2;
  m.peak_l = (uint32_t)(g() % 32769u); m.peak_r = (uint32_t)(g() % 32769u);
  m.clip_l = g() % (n + 1); m.clip_r = g() % (n + 1);
  sdrfm_audio_runs* r[3] = {&m.quiet_l, &m.quiet_r, &m.quiet_both};
  for (int k = 0; k < 3; ++k) {
    std::vector<int> q(n);
    const unsigned density = (unsigned)(g() % 5u);               // 0: none, 4: all
    for (auto& v : q) v = (g() % 4u) < density;
    *r[k] = naive(q);
  }
  return m;
}

int main() {
  // every 16-bit mask at every valid length
  for (uint32_t len = 1; len <= 16; ++len)
    for (uint32_t m = 0; m < 65536u; ++m) check_mask(m, len);
  // bits above the length are ignored
  for (uint32_t len = 1; len <= 16; ++len)
    for (uint32_t m = 0; m < 65536u; m += 97) {
      const sdrfm_audio_runs a = am_mask_runs(m, len), b = am_mask_runs((uint64_t)m | 0xFFFFFFFFFFFF0000ull, len);
      CHECK(same(a, b), "junk above len %u changes mask %x", len, m);
    }
  std::mt19937_64 g(20);
  for (uint32_t len = 1; len <= 64; ++len) {
    check_mask(~0ull, len);
    check_mask(0ull, len);
    for (int t = 0; t < 4000; ++t) {
      uint64_t m = g();
      switch (t & 3) {                                             // dense, sparse, plain, long runs
        case 0: m |= g(); break;
        case 1: m &= g(); break;
        case 2: break;
        default: m = (~0ull << (g() % 64u)) ^ (~0ull << (g() % 64u)) ^ (t & 4 ? ~0ull : 0ull); break;
      }
      check_mask(m, len);
    }
  }
  check_mask(~0ull, 64);
  check_mask(0ull, 64);
  check_mask(~0ull >> 1, 64);
  check_mask(~0ull << 1, 64);
  check_mask(1ull << 63, 64);

  // the joins: identity, associativity, and no commutativity
  sdrfm_audio_meter zero;
  std::memset(&zero, 0, sizeof(zero));
  for (int t = 0; t < 20000; ++t) {
    const sdrfm_audio_meter a = random_record(g, g() % 40u), b = random_record(g, g() % 40u), c = random_record(g, g() % 40u);
    sdrfm_audio_meter l = a, r = zero, ab = a, bc = b, ab_c, a_bc = a;
    am_meter_join(&l, &zero);
    am_meter_join(&r, &a);
    CHECK(!std::memcmp(&l, &a, sizeof(a)) && !std::memcmp(&r, &a, sizeof(a)), "identity, trial %d", t);
    am_meter_join(&ab, &b);
    ab_c = ab;
    am_meter_join(&ab_c, &c);
    am_meter_join(&bc, &c);
    am_meter_join(&a_bc, &bc);
    CHECK(!std::memcmp(&ab_c, &a_bc, sizeof(a)), "associativity, trial %d", t);
  }
  {  // quiet then loud is not loud then quiet
    const std::vector<int> q1 = {1, 1, 1}, q2 = {0, 1};
    const sdrfm_audio_runs a = naive(q1), b = naive(q2);
    const sdrfm_audio_runs ab = am_runs_join(a, 3, b, 2), ba = am_runs_join(b, 2, a, 3);
    CHECK(same(ab, naive({1, 1, 1, 0, 1})) && same(ba, naive({0, 1, 1, 1, 1})) && !same(ab, ba), "commutativity witness");
  }
  // the join is the concatenation: random sequences cut at random places
  for (int t = 0; t < 20000; ++t) {
    const size_t n = g() % 300u, cut = n ? g() % (n + 1) : 0;
    std::vector<int> q(n);
    const unsigned density = (unsigned)(g() % 5u);
    for (auto& v : q) v = (g() % 4u) < density;
    const std::vector<int> qa(q.begin(), q.begin() + (long)cut), qb(q.begin() + (long)cut, q.end());
    CHECK(same(am_runs_join(naive(qa), cut, naive(qb), n - cut), naive(q)), "join != concatenation, n %zu cut %zu", n, cut);
  }
  // a row cut the way the kernel cuts it
  for (uint32_t n : {0u, 1u, 2u, 63u, 64u, 65u, 255u, 256u, 257u, 1023u, 1024u, 1025u, 4800u, 4801u, 4865u}) {
    for (int t = 0; t < 30; ++t) {
      std::vector<int> q(n);
      const unsigned density = (unsigned)(g() % 5u);
      for (auto& v : q) v = (g() % 4u) < density;
      sdrfm_audio_runs row = {0, 0, 0, 0};
      uint64_t row_n = 0, covered = 0;
      for (uint32_t w = 0; w < 4; ++w) {
        uint64_t begin, end;
        am_wave_stretch(n, w, &begin, &end);
        CHECK(begin == covered && end >= begin && end <= n && (w == 3 || end == n || end % 64 == 0), "stretch n %u wave %u: %llu .. %llu", n, w,
              (unsigned long long)begin, (unsigned long long)end);
        covered = end;
        sdrfm_audio_runs wave = {0, 0, 0, 0};
        for (uint64_t b = begin; b < end; b += 64) {
          const uint32_t len = end - b < 64 ? (uint32_t)(end - b) : 64u;
          uint64_t mask = len == 64 ? 0 : (g() >> len) << len;         // junk above the block, as the lanes behind the end would give
          for (uint32_t i = 0; i < len; ++i) mask |= (uint64_t)q[b + i] << i;
          wave = am_runs_join(wave, b - begin, am_mask_runs(mask, len), len);
        }
        row = am_runs_join(row, row_n, wave, end - begin);
        row_n += end - begin;
      }
      CHECK(covered == n && row_n == n, "stretches cover %llu of %u", (unsigned long long)covered, n);
      CHECK(same(row, naive(q)), "kernel cut, n %u trial %d", n, t);
    }
  }
  {  // am_wave_stretch at the top of the range: no overflow
    uint64_t begin, end;
    am_wave_stretch(0xFFFFFFFFu, 3, &begin, &end);
    CHECK(end == 0xFFFFFFFFull && begin == 3ull * 0x40000000ull, "stretch at 2^32 - 1: %llu .. %llu", (unsigned long long)begin, (unsigned long long)end);
  }
  if (fails) { std::printf("%d failures\n", fails); return 1; }
  std::printf("ok\n");
  return 0;
}
