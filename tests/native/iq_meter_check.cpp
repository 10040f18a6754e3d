// The raw-capture IQ meter's launch geometry and per-dword arithmetic (csrc/sdrfm_iq_meter.h) walked on the CPU: a program of its own, built with
// ASan and UBSan by tests/test_iq_meter_cpu.py and run as a program.  It plays the kernel's walk — every workgroup, every lane, the head and the
// tail — over exactly-sized heap rows with plain loads, so a byte taken twice, a byte missed or a byte outside the row shows.  Prints the
// geometry of a few shapes (the test holds the Python mirror to them) and "ok" at the end.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_iq_meter.h"

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

struct Sums { uint64_t v[7]; };

static Sums naive(const uint8_t* row, uint32_t nbytes) {
  Sums s;
  memset(&s, 0, sizeof s);
  for (uint32_t k = 0; k < nbytes; k += 2) {
    const uint64_t bi = row[k], bq = row[k + 1];
    s.v[0] += bi; s.v[1] += bq; s.v[2] += bi * bi; s.v[3] += bq * bq; s.v[4] += bi * bq;
    s.v[5] += bi == 0 || bi == 255; s.v[6] += bq == 0 || bq == 255;
  }
  return s;
}

static uint32_t load32(const uint8_t* p) { uint32_t w; memcpy(&w, p, 4); return w; }

// the kernel's walk over one row at byte offset `off` of a 16-byte aligned arena: times[k] counts how often byte k of the row is taken (the byte an
// odd row's shift borrows from the next aligned vector is taken THERE and not where it was loaded first), the sums come out of iqm_take
static Sums walk(const uint8_t* row, uintptr_t addr, uint32_t nbytes, uint32_t n_streams, std::vector<uint8_t>& times, uint64_t* lane_max) {
  const IqmRow g = iqm_row(addr, nbytes);
  const IqmGrid grid = iqm_grid(n_streams, nbytes);
  CHECK(g.head % 2 == 0 && g.tail % 2 == 0 && g.head <= 16 && g.tail <= 14 && g.head + g.nvec * IQM_VEC + g.tail == nbytes);
  CHECK(g.nvec == 0 || (addr + g.head - g.odd) % 16 == 0);
  CHECK(grid.bps >= 1 && grid.share % IQM_NT == 0 && grid.share / IQM_NT <= IQM_MAX_ITERS);
  CHECK((uint64_t)grid.bps * grid.share >= g.nvec);                           // every vector has a workgroup
  CHECK((uint64_t)n_streams * grid.bps < (1ull << 31));
  CHECK(iqm_lane_bound(grid.share / IQM_NT) + 255u * 255u <= 0xFFFFFFFFull);  // a lane's vectors and the one edge pair it may take besides
  times.assign(nbytes, 0);
  Sums s;
  memset(&s, 0, sizeof s);
  const uint8_t* body = row + g.head - g.odd;
  for (uint32_t b = 0; b < grid.bps; ++b) {
    const uint32_t v0 = b * grid.share, v1 = v0 + grid.share < g.nvec ? v0 + grid.share : g.nvec;
    for (uint32_t tid = 0; tid < IQM_NT; ++tid) {
      IqmAcc a = {0, 0, 0, 0, 0, 0, 0};
      for (uint32_t v = v0 + tid; v < v1; v += IQM_NT) {
        const uint8_t* at = body + (size_t)v * IQM_VEC;
        CHECK(at >= row && at + IQM_VEC + g.odd <= row + nbytes);             // every load inside the row
        uint32_t w[4] = {load32(at), load32(at + 4), load32(at + 8), load32(at + 12)};
        if (g.odd) {
          const uint32_t nx = at[IQM_VEC];
          w[0] = iqm_shift(w[0], w[1]); w[1] = iqm_shift(w[1], w[2]); w[2] = iqm_shift(w[2], w[3]); w[3] = iqm_shift(w[3], nx);
        }
        for (int k = 0; k < 4; ++k) iqm_take(&a, w[k]);
        for (uint32_t k = 0; k < IQM_VEC; ++k) times[(size_t)(at - row) + g.odd + k] += 1;
      }
      if (b == 0 && tid < 15) {
        const uint32_t k = tid < 8 ? tid : tid - 8;
        if (tid < 8 ? 2 * k < g.head : 2 * k < g.tail) {
          const uint32_t o = (tid < 8 ? 0 : g.head + g.nvec * IQM_VEC) + 2 * k;
          CHECK(o + 1 < nbytes);
          iqm_take_pair(&a, row[o], row[o + 1]);
          times[o] += 1; times[o + 1] += 1;
        }
      }
      const uint32_t lane[7] = {a.si, a.sq, a.sii, a.sqq, a.siq, a.ri, a.rq};
      for (int k = 0; k < 7; ++k) { s.v[k] += lane[k]; if (lane_max && lane[k] > *lane_max) *lane_max = lane[k]; }
    }
  }
  return s;
}

// the same cover as intervals, for rows too long to count byte by byte: the workgroups' vector ranges tile [0, nvec) in order, and with the head
// and the tail that is the row
static void cover_intervals(uint32_t nbytes, uint32_t off, uint32_t n_streams) {
  const IqmRow g = iqm_row((uintptr_t)off, nbytes);
  const IqmGrid grid = iqm_grid(n_streams, nbytes);
  CHECK(g.head % 2 == 0 && g.tail % 2 == 0 && g.head <= 16 && g.tail <= 14 && g.head + g.nvec * IQM_VEC + g.tail == nbytes);
  CHECK(g.nvec == 0 || (off + g.head - g.odd) % 16 == 0);
  CHECK(grid.share % IQM_NT == 0 && grid.share / IQM_NT <= IQM_MAX_ITERS && (uint64_t)n_streams * grid.bps < (1ull << 31));
  uint32_t next = 0;
  for (uint32_t b = 0; b < grid.bps; ++b) {
    const uint32_t v0 = b * grid.share, v1 = v0 + grid.share < g.nvec ? v0 + grid.share : g.nvec;
    if (v0 < v1) { CHECK(v0 == next); next = v1; }
  }
  CHECK(next == g.nvec);
  CHECK(g.nvec == 0 || (size_t)g.head - g.odd + (size_t)g.nvec * IQM_VEC + g.odd <= nbytes);   // the last load and the byte behind it
}

static void cover(uint32_t nbytes, uint32_t off, uint32_t n_streams, int fill) {
  // an exactly-sized heap block: the row starts `off` bytes into a 16-byte aligned address, which malloc gives
  void* mem = nullptr;
  CHECK(posix_memalign(&mem, 16, (size_t)off + nbytes + (off + nbytes == 0)) == 0);
  uint8_t* block = (uint8_t*)mem;
  uint8_t* row = block + off;
  for (uint32_t k = 0; k < nbytes; ++k) row[k] = fill >= 0 ? (uint8_t)fill : (uint8_t)rnd();
  std::vector<uint8_t> times;
  uint64_t lane_max = 0;
  const Sums got = walk(row, (uintptr_t)row, nbytes, n_streams, times, &lane_max), want = naive(row, nbytes);
  for (uint32_t k = 0; k < nbytes; ++k) CHECK(times[k] == 1);
  CHECK(memcmp(&got, &want, sizeof got) == 0);
  free(block);
}

int main() {
  // every byte exactly once and the sums the naive ones: every nbytes in 0 .. 4096 at the row offsets 0 .. 17
  for (uint32_t off = 0; off < 18; ++off)
    for (uint32_t nbytes = 0; nbytes <= 4096; nbytes += 2) cover(nbytes, off, 1 + (nbytes % 5), -1);
  // more than one workgroup per row, shares of several steps, and rows that end inside a share
  for (uint32_t off = 0; off < 18; ++off) {
    cover(3 * 4096 * 7 + 2 * off, off, 300, -1);
    cover(1 << 20, off, 1, off & 1 ? 255 : -1);
  }
  // the maximum: the cover as intervals at every offset, and all 255 from one stream walked whole — the lanes' 32-bit sums hold (the walk's check
  // against iqm_lane_bound) and come out as the naive 64-bit ones
  for (uint32_t off = 0; off < 18; ++off) {
    cover_intervals(IQM_MAX_BYTES, off, 1);
    cover_intervals(IQM_MAX_BYTES, off, IQM_MAX_STREAMS);
    cover_intervals(IQM_MAX_BYTES - 2, off, 7);
  }
  for (uint32_t off = 0; off < 2; ++off) cover(IQM_MAX_BYTES, off, 1, 255);
  {
    const IqmGrid g = iqm_grid(IQM_MAX_STREAMS, IQM_MAX_BYTES);                // the longest share there is
    CHECK(g.share / IQM_NT == IQM_MAX_ITERS && iqm_lane_bound(IQM_MAX_ITERS) + 65025u <= 0xFFFFFFFFull);
    CHECK(iqm_lane_bound(2 * IQM_MAX_ITERS + 65) > 0xFFFFFFFFull);            // and the bound is not idle: little over twice the share would not fit
  }
  // the SWAR rail test against the naive one over all 2^16 halfwords, in both halves of a dword and beside rails in the other half
  for (uint32_t h = 0; h < 65536; ++h) {
    const uint32_t other[3] = {0x00000000u, 0xFFFF0000u, 0x5A010000u};
    for (int k = 0; k < 3; ++k) {
      const uint32_t w = h | other[k], x = (h << 16) | (other[k] >> 16);
      for (int which = 0; which < 2; ++which) {
        const uint32_t v = which ? x : w, r = iqm_rails(v);
        uint32_t want = 0;
        for (int b = 0; b < 4; ++b) { const uint32_t c = (v >> (8 * b)) & 255u; if (c == 0 || c == 255) want |= 0x80u << (8 * b); }
        CHECK(r == want);
      }
    }
  }
  // the dot-product masks at both parities: a dword I Q I Q as it stands, and Q I Q I put back by the shift
  for (int t = 0; t < 200000; ++t) {
    uint8_t b[9];
    for (int k = 0; k < 9; ++k) b[k] = t < 512 ? (uint8_t)((t >> k) & 1 ? 255 : 0) : (uint8_t)rnd();   // (first every pattern of rails)
    for (uint32_t odd = 0; odd < 2; ++odd) {
      // the pairs start at b[odd]; the aligned dwords are b[0..3] and b[4..7]
      uint32_t w = load32(b), w1 = load32(b + 4);
      if (odd) w = iqm_shift(w, w1);
      IqmAcc a = {0, 0, 0, 0, 0, 0, 0};
      iqm_take(&a, w);
      const Sums want = naive(b + odd, 4);
      CHECK(a.si == want.v[0] && a.sq == want.v[1] && a.sii == want.v[2] && a.sqq == want.v[3] && a.siq == want.v[4] && a.ri == want.v[5] && a.rq == want.v[6]);
    }
  }
  CHECK(iqm_dot4(0xFFFFFFFFu, 0xFFFFFFFFu, 7u) == 4u * 65025u + 7u);
  // the geometry of a few shapes, for the Python mirror
  const uint32_t shapes[][2] = {{1, 0}, {1, 2}, {1, 4096}, {1, 4098}, {3, 8192}, {65, 393216}, {65, 393218}, {1, 1u << 20}, {16, 1u << 20}, {256, 480000},
                                {1, IQM_MAX_BYTES}, {65536, IQM_MAX_BYTES}, {2049, 1u << 16}};
  for (size_t k = 0; k < sizeof shapes / sizeof shapes[0]; ++k) {
    const IqmGrid g = iqm_grid(shapes[k][0], shapes[k][1]);
    printf("grid %u %u %u %u\n", shapes[k][0], shapes[k][1], g.bps, g.share);
  }
  printf("ok\n");
  return 0;
}
