// tests/native/loudness_check.cpp — the shared arithmetic of csrc/sdrfm_loudness.h held to naive loops, as a program of its own under ASan and
// UBSan.  Built twice: with LOUDNESS_CHECK_REDUCED the tile shrinks to 4 lanes of 3 pairs and the index functions are walked exhaustively
// (block_len 64 .. 70 x every pos mod block_len x n = 0 .. 3 tiles + 1); without it the library's own geometry is used for the ring rule and
// the matrix-power table.  Prints "ok".
#ifdef LOUDNESS_CHECK_REDUCED
#define SDRFM_LD_L_CHECK 3u
#define SDRFM_LD_NT_CHECK 4u
#endif
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_loudness.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);                \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

// one call of n pairs on a stream at pos: walk the tiles as the kernel does and mark, per pair, the sub-block the kernel's sums put it into
static void walk_call(uint64_t pos, uint32_t n, uint32_t B) {
  std::vector<int64_t> owner(n, -1);
  std::vector<int> times(n, 0);
  uint32_t off = (uint32_t)(pos % B);
  uint64_t blk = pos / B;
  CHECK(ld_tiles(n) == (n + SDRFM_LD_TILE - 1) / SDRFM_LD_TILE);
  uint64_t done = 0;
  for (uint32_t t = 0; t < ld_tiles(n); ++t) {
    const uint32_t base = t * SDRFM_LD_TILE, m = ld_tile_len(n, t);
    CHECK(m >= 1 && m <= SDRFM_LD_TILE && base + m <= n && (t + 1 < ld_tiles(n) ? m == SDRFM_LD_TILE : base + m == n));
    const uint32_t nact = ld_active_lanes(m);
    // the lanes' chunks tile [0, m) in lane order
    uint32_t at = 0;
    std::vector<uint32_t> split(SDRFM_LD_NT), begin(SDRFM_LD_NT), len(SDRFM_LD_NT);
    for (uint32_t j = 0; j < SDRFM_LD_NT; ++j) {
      ld_chunk(m, j, &begin[j], &len[j]);
      CHECK(len[j] <= SDRFM_LD_L && (len[j] == 0) == (j >= nact));
      if (len[j]) CHECK(begin[j] == at);
      at += len[j];
      const uint32_t o = (off + begin[j]) % B;
      split[j] = ld_split(o, B, len[j]);
      uint32_t naive = 0;                                                        // pairs of the chunk before the first sub-block boundary
      for (uint32_t i = 0; i < len[j]; ++i) {
        if (i > 0 && (pos + base + begin[j] + i) % B == 0) break;
        ++naive;
      }
      CHECK(split[j] == naive);
    }
    CHECK(at == m);
    const uint32_t nb = ld_tile_blocks(off, m, B);
    CHECK(nb == (pos + base + m) / B - (pos + base) / B);
    for (uint32_t k = 0; k <= nb; ++k) {
      int64_t start;
      uint32_t lo, hi;
      ld_block_span(off, m, B, k, &start, &lo, &hi);
      CHECK(lo <= m && hi <= m);
      if (hi > lo) {
        for (uint32_t j = lo / SDRFM_LD_L; j <= (hi - 1) / SDRFM_LD_L; ++j) {
          CHECK(j < nact);
          const uint32_t part = ld_piece(j, start);
          const uint32_t a = part ? split[j] : 0u, b = part ? len[j] : split[j];  // the pairs of the chunk that piece holds
          CHECK(b > a);                                                          // never an empty piece: the chunk meets the sub-block
          for (uint32_t i = a; i < b; ++i) {
            owner[base + begin[j] + i] = (int64_t)(blk + k);
            ++times[base + begin[j] + i];
          }
        }
      }
    }
    blk += nb;
    done += nb;
    off = ld_tile_next_off(off, m, B);
    CHECK(off == (pos + base + m) % B);
  }
  for (uint32_t i = 0; i < n; ++i) CHECK(times[i] == 1 && owner[i] == (int64_t)((pos + i) / B));
  uint64_t naive_done = 0;
  for (uint32_t i = 0; i < n; ++i) naive_done += (pos + i + 1) % B == 0;
  CHECK(done == naive_done && ld_blocks_done(pos, n, B) == naive_done);
}

// the ring: of the sub-blocks a stream has completed after a call only the newest cap are stored, each in a slot of its own
static void ring_rule() {
  for (uint32_t cap = 1; cap <= 7; ++cap)
    for (uint64_t before = 0; before <= 9; ++before)
      for (uint64_t add = 0; add <= 20; ++add) {
        const uint64_t total = before + add, keep = ld_keep_from(total, cap);
        std::vector<int> writers(cap, 0);
        uint64_t stored = 0;
        for (uint64_t b = before; b < total; ++b)
          if (b >= keep) { ++writers[ld_ring_slot(b, cap)]; ++stored; }
        for (uint32_t s = 0; s < cap; ++s) CHECK(writers[s] <= 1);
        CHECK(stored == (add < cap ? add : cap));                               // exactly the newest min(add, cap) of this call
        for (uint64_t b = keep; b < total; ++b)                                  // and what a read finds in a slot is the newest with that slot
          for (uint64_t o = keep; o < total; ++o) CHECK(b == o || ld_ring_slot(b, cap) != ld_ring_slot(o, cap));
      }
  CHECK(ld_keep_from(75, 4) == 71 && ld_ring_slot(71, 4) == 3 && ld_ring_slot(74, 4) == 2);
}

static void matmul_l(const long double* X, const long double* Y, long double* out) {
  for (int r = 0; r < 4; ++r)
    for (int q = 0; q < 4; ++q) {
      long double t = 0;
      for (int k = 0; k < 4; ++k) t += X[4 * r + k] * Y[4 * k + q];
      out[4 * r + q] = t;
    }
}

// the table against repeated multiplication in long double, and the transition against the step itself
static void table() {
  sdrfm_loudness_coef c;
  const double k48[10] = {1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                          1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621};
  for (int k = 0; k < 10; ++k) c.c[k] = k48[k];
  double A[16], pw[SDRFM_LD_TABLE];
  ld_transition(c.c, A);
  const double z0[4] = {1234.5, -987.25, 40000.0, -39990.5};
  double z[4] = {z0[0], z0[1], z0[2], z0[3]};
  (void)ld_kw_step(c.c, z, 0.0);                                                 // a step with no input is the transition
  for (int r = 0; r < 4; ++r) {
    double want = 0;
    for (int k = 0; k < 4; ++k) want += A[4 * r + k] * z0[k];
    CHECK(std::fabs(z[r] - want) <= 1e-9);
  }
  const double kappa = ld_balance(c.c);
  CHECK(kappa == 256.0);                                                         // 1 / sqrt(1 + a1 + a2) = 200.8
  ld_matrix_powers(c.c, pw);
  CHECK(pw[16 * SDRFM_LD_STEPS] == kappa && pw[16 * SDRFM_LD_STEPS + 1] == 1.0 / kappa);
  // the transition in the scan's coordinates, T A T^-1 with T z = (z0, z1, z2, kappa (z2 + z3)), entry by entry
  long double Al[16], P[16], t[16];
  for (int r = 0; r < 4; ++r) {
    long double row[4];
    for (int k = 0; k < 4; ++k) row[k] = r < 3 ? (long double)A[4 * r + k] : (long double)kappa * ((long double)A[8 + k] + (long double)A[12 + k]);
    Al[4 * r] = row[0];
    Al[4 * r + 1] = row[1];
    Al[4 * r + 2] = row[2] - row[3];
    Al[4 * r + 3] = row[3] / (long double)kappa;
  }
  for (int k = 0; k < 16; ++k) P[k] = Al[k];
  uint32_t have = 1;
  double zs[4] = {z0[0], z0[1], z0[2], z0[3]};                                   // the same steps through the filter itself
  uint32_t stepped = 0;
  for (uint32_t i = 0; i < SDRFM_LD_STEPS; ++i) {
    const uint32_t want = SDRFM_LD_L << i;
    for (; have < want; ++have) {                                                // one factor at a time
      matmul_l(Al, P, t);
      for (int k = 0; k < 16; ++k) P[k] = t[k];
    }
    double worst = 0, largest = 0;
    for (int k = 0; k < 16; ++k) {
      const double d = std::fabs((double)(P[k] - (long double)pw[16 * i + k]));
      worst = d > worst ? d : worst;
      largest = std::fabs((double)P[k]) > largest ? std::fabs((double)P[k]) : largest;
    }
#ifndef LOUDNESS_CHECK_REDUCED
    CHECK(largest <= 1.0);                                                       // the balanced coordinates at L = 19: no entry above 1
#endif
    CHECK(worst <= 2.3e-16 * (largest > 1.0 ? largest : 1.0));                   // rounded to double once: half an ulp of the largest entry
    for (; stepped < want; ++stepped) (void)ld_kw_step(c.c, zs, 0.0);
    const double w0[4] = {z0[0], z0[1], z0[2], kappa * (z0[2] + z0[3])};         // T z0, through the table, and back
    double w[4] = {0, 0, 0, 0};
    ld_matvec_add(pw + 16 * i, w0, w);
    w[3] = w[3] / kappa - w[2];
    for (int r = 0; r < 4; ++r) CHECK(std::fabs(w[r] - zs[r]) <= 1e-6);          // the table is the filter's own zero-input response
  }
}

// the plain-C restatement of the kernel (ld_emulate_channel) against the definition over ragged calls, and the predicate built on it
static void domain() {
  const double k48[10] = {1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                          1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621};
  double pw[SDRFM_LD_TABLE], rel = -1, ab = -1;
  ld_matrix_powers(k48, pw);
  const uint32_t cuts[] = {1, 0, 2, SDRFM_LD_L, SDRFM_LD_TILE - 1, SDRFM_LD_TILE + 1, 257, 64, 2 * SDRFM_LD_TILE + 17};
  for (uint32_t B : {64u, 100u}) {
    double zg[4] = {0, 0, 0, 0}, zw[4] = {0, 0, 0, 0}, eg = 0, ew = 0;
    uint64_t pg = 0, pw_ = 0, seed = 12345;
    for (uint32_t n : cuts) {
      std::vector<int16_t> x(n);
      for (auto& v : x) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        v = (int16_t)(uint16_t)(seed >> 48);
      }
      std::vector<double> got(n / B + 2, -1.0), want(n / B + 2, -2.0);
      const uint32_t k = ld_emulate_channel(k48, pw, x.data(), n, B, zg, &eg, &pg, got.data());
      CHECK(k == ld_reference_channel(k48, x.data(), n, B, zw, &ew, &pw_, want.data()) && k == ld_blocks_done(pg - n, n, B));
      CHECK(pg == pw_ && got[k] == -1.0 && want[k] == -2.0);                      // nothing behind the sub-blocks the call completes
      for (uint32_t i = 0; i < k; ++i) CHECK(std::fabs(got[i] - want[i]) <= 1e-9 * want[i] + 1e-3 * B);
      CHECK(std::fabs(eg - ew) <= 1e-9 * ew + 1e-3 * B);
      for (int r = 0; r < 4; ++r) CHECK(std::fabs(zg[r] - zw[r]) <= 1e-6);
    }
  }
  const int in = ld_in_domain(k48, pw, &rel, &ab);
  CHECK(rel >= 0 && ab >= 0 && in == (rel <= SDRFM_LD_ACCEPT_REL && ab <= SDRFM_LD_ACCEPT_ABS));
#ifndef LOUDNESS_CHECK_REDUCED
  CHECK(in && rel > 1e-11 && ab > 1e-5);                                         // the default set: 3.17e-11 and 3.41e-5 (tests/loudness_cases.py)
  double near_minus_one[10];
  for (int k = 0; k < 10; ++k) near_minus_one[k] = k48[k];
  near_minus_one[8] = 2.0 * 0.999 * std::cos(1e-3);                              // high-pass poles at 0.999 e^(+-i (pi - 1e-3))
  near_minus_one[9] = 0.999 * 0.999;
  ld_matrix_powers(near_minus_one, pw);
  CHECK(!ld_in_domain(near_minus_one, pw, &rel, &ab) && rel > 1e-7);
  CHECK(!ld_in_domain(near_minus_one, pw, nullptr, nullptr));
#endif
}

int main() {
  domain();
#ifdef LOUDNESS_CHECK_REDUCED
  static_assert(SDRFM_LD_TILE == 12, "the reduced tile");
  for (uint32_t B = 64; B <= 70; ++B)
    for (uint32_t off = 0; off < B; ++off)
      for (uint32_t n = 0; n <= 3 * SDRFM_LD_TILE + 1; ++n) {
        walk_call(off, n, B);
        walk_call((uint64_t)B * 1000003u + off, n, B);
      }
#else
  static_assert(SDRFM_LD_L == 19 && SDRFM_LD_NT == 256 && SDRFM_LD_TILE == 4864 && SDRFM_LD_L <= SDRFM_LD_BLOCK_MIN, "the library's geometry");
  const uint32_t ns[] = {1, 18, 19, 20, 4800, 4863, 4864, 4865, 9745};
  for (uint32_t B : {64u, 100u, 4800u})
    for (uint32_t n : ns)
      for (uint64_t pos : {(uint64_t)0, (uint64_t)1, (uint64_t)B - 1, (uint64_t)3 * B + 17, ((uint64_t)1 << 33) + 5}) walk_call(pos, n, B);
#endif
  ring_rule();
  table();
  std::printf("ok\n");
  return 0;
}
