// tests/native/pcm_rows_check.cpp — the (L, R) row checks of csrc/sdrfm_pcm_rows.h as pure functions, a program of its own under ASan and UBSan
// (tests/test_pcm_rows_cpu.py): every refusal of pcm_rows_refusal and its precedence over the next one, the single-row stride exemption, the mix
// bus's overlap test at touching, abutting and nested ranges against a walk over the bytes, and stage_cap at the sizes around a capacity step, at
// every handle's maximum and where the uint32 sum wraps.  Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_pcm_rows.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);     \
      exit(1);                                                    \
    }                                                             \
  } while (0)

static const uint32_t N_MAX = 1u << 20;   // SDRFM_LIMIT_N_MAX = SDRFM_RATE_N_MAX = PMIX_N_MAX
static const uint32_t DEV = SDRFM_F_DEVICE_PTRS, BAD = 0x80u;

// the refusals in their order; defect d present where bit d of `mask` is set.  The answer is that of the first one present
enum { D_FLAG, D_NMAX, D_ODD_IN, D_ODD_OUT, D_EMPTY, D_NULL_IN, D_NULL_OUT, D_ALIGN_IN, D_ALIGN_OUT, D_COUNT };

static int expected(unsigned mask, bool device) {
  if (mask & (1u << D_FLAG)) return SDRFM_EINVAL;
  if (mask & (1u << D_NMAX)) return SDRFM_EINVAL;
  if (mask & ((1u << D_ODD_IN) | (1u << D_ODD_OUT))) return SDRFM_EINVAL;
  if (mask & (1u << D_EMPTY)) return PCM_ROWS_EMPTY;
  if (mask & ((1u << D_NULL_IN) | (1u << D_NULL_OUT))) return SDRFM_EINVAL;
  if (device && (mask & ((1u << D_ALIGN_IN) | (1u << D_ALIGN_OUT)))) return SDRFM_EINVAL;   // host rows may lie anywhere
  return SDRFM_OK;
}

static void refusals() {
  alignas(8) static int16_t in[64], out[64];
  unsigned seen_ok = 0, seen_empty = 0;
  for (int device = 0; device < 2; ++device)
    for (unsigned mask = 0; mask < (1u << D_COUNT); ++mask) {
      if ((mask & (1u << D_NMAX)) && (mask & (1u << D_EMPTY))) continue;          // one n
      if ((mask & (1u << D_NULL_IN)) && (mask & (1u << D_ALIGN_IN))) continue;    // one pointer
      if ((mask & (1u << D_NULL_OUT)) && (mask & (1u << D_ALIGN_OUT))) continue;
      const uint32_t flags = (device ? DEV : 0u) | ((mask & (1u << D_FLAG)) ? BAD : 0u);
      const uint32_t n = (mask & (1u << D_NMAX)) ? N_MAX + 1u : (mask & (1u << D_EMPTY)) ? 0u : 8u;
      const size_t is = 16 + ((mask >> D_ODD_IN) & 1u), os = 16 + ((mask >> D_ODD_OUT) & 1u);
      const void* pi = (mask & (1u << D_NULL_IN)) ? nullptr : (const void*)((const char*)in + ((mask & (1u << D_ALIGN_IN)) ? 2 : 0));
      const void* po = (mask & (1u << D_NULL_OUT)) ? nullptr : (const void*)((const char*)out + ((mask & (1u << D_ALIGN_OUT)) ? 2 : 0));
      const int got = pcm_rows_refusal(flags, DEV, n, N_MAX, pi, is, po, os), want = expected(mask, device != 0);
      if (got != want) fprintf(stderr, "device %d mask %#x: %d, expected %d\n", device, mask, got, want);
      CHECK(got == want);
      seen_ok += got == SDRFM_OK;
      seen_empty += got == PCM_ROWS_EMPTY;
    }
  CHECK(seen_ok == 1 + 4 && seen_empty > 0);                     // no defect; and on the host the three misalignments beside it
  CHECK(PCM_ROWS_EMPTY != SDRFM_OK && PCM_ROWS_EMPTY != SDRFM_EINVAL && PCM_ROWS_EMPTY < 0);
  // n at the maximum is taken, one more is not; a flag that is allowed is no defect; 1 and 3 mod 4 are off the boundary too
  CHECK(pcm_rows_refusal(0, DEV, N_MAX, N_MAX, in, 16, out, 16) == SDRFM_OK);
  CHECK(pcm_rows_refusal(0, DEV, N_MAX + 1u, N_MAX, in, 16, out, 16) == SDRFM_EINVAL);
  CHECK(pcm_rows_refusal(4u, DEV | 4u, 8, N_MAX, in, 16, out, 16) == SDRFM_OK && pcm_rows_refusal(4u, DEV, 8, N_MAX, in, 16, out, 16) == SDRFM_EINVAL);
  for (int off = 1; off < 4; ++off) CHECK(pcm_rows_refusal(DEV, DEV, 8, N_MAX, (const char*)in + off, 16, out, 16) == SDRFM_EINVAL);
  CHECK(pcm_rows_refusal(DEV, DEV, 8, N_MAX, (const char*)in + 4, 16, (const char*)out + 4, 16) == SDRFM_OK);
}

static void capacity() {
  for (size_t rows = 0; rows < 4; ++rows)
    for (size_t need = 0; need < 6; ++need)
      for (size_t stride = 0; stride < 8; ++stride) {
        CHECK((pcm_rows_capacity(rows, stride, need) != 0) == (rows <= 1 || stride >= need));   // a single row ignores its stride
        CHECK(pcm_rows_pitch(rows, stride, need) == (rows > 1 ? stride : need));
      }
  CHECK(pcm_rows_capacity(2, 15, 16) == 0 && pcm_rows_capacity(2, 16, 16) != 0 && pcm_rows_capacity(1, 0, 16) != 0);
}

// the definition: some byte belongs to both ranges
static bool share_a_byte(size_t in0, size_t in_rows, size_t is, size_t out0, size_t out_rows, size_t os, uint32_t n) {
  const size_t in1 = in0 + 2 * ((in_rows - 1) * is + 2 * (size_t)n), out1 = out0 + 2 * ((out_rows - 1) * os + 2 * (size_t)n);
  for (size_t b = in0; b < in1; ++b)
    if (b >= out0 && b < out1) return true;
  return false;
}

static void apart() {
  static int16_t mem[4096];
  const size_t base = 1024;                                      // in rows start here, in int16
  for (size_t in_rows = 1; in_rows <= 3; ++in_rows)
    for (size_t out_rows = 1; out_rows <= 3; ++out_rows)
      for (uint32_t n = 1; n <= 3; ++n)
        for (size_t pad = 0; pad <= 2; pad += 2) {
          const size_t is = 2 * n + pad, os = 2 * n + pad;
          const size_t in_len = (in_rows - 1) * is + 2 * n, out_len = (out_rows - 1) * os + 2 * n;
          for (size_t o = base - out_len - 2; o <= base + in_len + 2; ++o) {   // from clear below, through touching, nested and abutting, to clear above
            const bool want = !share_a_byte(2 * base, in_rows, is, 2 * o, out_rows, os, n);
            CHECK((pcm_rows_apart(mem + base, in_rows, is, mem + o, out_rows, os, n) != 0) == want);
          }
          CHECK(pcm_rows_apart(mem + base, in_rows, is, mem + base - out_len, out_rows, os, n));        // abutting below: the ranges only touch
          CHECK(pcm_rows_apart(mem + base, in_rows, is, mem + base + in_len, out_rows, os, n));         // abutting above
          CHECK(!pcm_rows_apart(mem + base, in_rows, is, mem + base - out_len + 1, out_rows, os, n));   // one int16 in
          CHECK(!pcm_rows_apart(mem + base, in_rows, is, mem + base + in_len - 1, out_rows, os, n));
          CHECK(!pcm_rows_apart(mem + base, in_rows, is, mem + base, out_rows, os, n));                 // in place
        }
  CHECK(!pcm_rows_apart(mem + base, 3, 8, mem + base + 10, 1, 2, 1));   // nested: one pair inside the input rows' span, between two rows' data
}

static void caps() {
  const uint32_t sizes[] = {0u, 1u, 1023u, 1024u, 1025u};
  const uint32_t want[] = {0u, 1024u, 1024u, 1024u, 2048u};
  for (int i = 0; i < 5; ++i) CHECK(stage_cap(sizes[i], 1024u) == want[i]);
  // every handle's maximum: the limiter's, the matcher's and the mix bus's 2^20 pairs, the matcher's largest count 4 * 2^20 + 1, the IQ meter's 2^26 bytes
  CHECK(stage_cap(1u << 20, 1024u) == 1u << 20 && stage_cap((1u << 22) + 1u, 1024u) == (1u << 22) + 1024u);
  CHECK(stage_cap(64u << 20, 4096u) == 64u << 20 && stage_cap(1000u, 4096u) == 4096u && stage_cap(4097u, 4096u) == 8192u && stage_cap(0u, 4096u) == 0u);
  for (uint32_t n = 0; n < 5000u; ++n) {
    const uint32_t c = stage_cap(n, 1024u);
    CHECK(c >= n && c % 1024u == 0 && c - n < 1024u);
  }
  // the uint32 sum: exact up to UINT32_MAX - 1023 rounded down, 0 beyond — the n_max checks keep every caller far below
  CHECK(stage_cap(0xFFFFFC00u, 1024u) == 0xFFFFFC00u && stage_cap(0xFFFFFC01u, 1024u) == 0u && stage_cap(0xFFFFFFFFu, 1024u) == 0u);
  CHECK((uint64_t)(1u << 22) + 1u < 0xFFFFFC00u && (uint64_t)(64u << 20) < 0xFFFFF000u);
}

int main() {
  refusals();
  capacity();
  apart();
  caps();
  printf("ok\n");
  return 0;
}
