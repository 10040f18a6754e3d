/* sdrfm_pcm_deemph_stereo_hicut_s16 (csrc/pcm_sink.c; include/sdrfm.h) as a program of its own, built with ASan and UBSan by
 * tests/test_hicut_cpu.py: every buffer is allocated at exactly the size the contract names, so a read or a write past it is an error.  Edge sizes
 * (0, 1, 2, 19, 4865), both ramp directions, the four slews; h0 = ht = 32768 against sdrfm_pcm_deemph_stereo_s16, cuts into calls against the one
 * call, the saturated count, every refusal.  Prints "ok". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/sdrfm.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);           \
      return 1;                                                         \
    }                                                                   \
  } while (0)

static uint32_t lcg = 12345u;
static float draw(void) {
  lcg = lcg * 1664525u + 1013904223u;
  return ((float)(lcg >> 8) / 8388608.0f - 1.0f) * 3.0f;
}

static uint32_t advance(uint32_t J, uint32_t n) {
  const uint64_t s = (uint64_t)J + n;
  return s < 65536u ? (uint32_t)s : 65536u;
}

int main(void) {
  const float alpha = 0.2425f, gain = 16689.0f;
  const uint32_t sizes[] = {0, 1, 2, 19, 4865}, slews[] = {1, 7, 40, 32768};
  const uint16_t pairs[][2] = {{1024, 32768}, {32768, 1024}, {1025, 32767}, {8192, 8192}, {32768, 32768}};
  for (unsigned a = 0; a < sizeof sizes / sizeof *sizes; ++a) {
    const uint32_t n = sizes[a];
    float* l = (float*)malloc(sizeof(float) * (n ? n : 1));
    float* r = (float*)malloc(sizeof(float) * (n ? n : 1));
    int16_t* one = (int16_t*)malloc(sizeof(int16_t) * (n ? 2 * n : 1));
    int16_t* cut = (int16_t*)malloc(sizeof(int16_t) * (n ? 2 * n : 1));
    CHECK(l && r && one && cut);
    for (uint32_t i = 0; i < n; ++i) { l[i] = draw(); r[i] = draw(); }
    for (unsigned b = 0; b < sizeof slews / sizeof *slews; ++b)
      for (unsigned c = 0; c < sizeof pairs / sizeof *pairs; ++c) {
        const uint16_t h0 = pairs[c][0], ht = pairs[c][1];
        float s1[2] = {0.25f, -0.5f}, s2[2] = {0.25f, -0.5f};
        CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(n ? l : NULL, n ? r : NULL, n, alpha, gain, h0, ht, slews[b], 3, s1, n ? one : NULL) == SDRFM_OK);
        /* the same samples in three calls (the middle one of 0 or 1 samples), J carried */
        const uint32_t n1 = n / 3, n2 = n > n1 ? 1 : 0, n3 = n - n1 - n2;
        uint32_t J = 3;
        CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(l, r, n1, alpha, gain, h0, ht, slews[b], J, s2, cut) == SDRFM_OK);
        J = advance(J, n1);
        CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(l + n1, r + n1, n2, alpha, gain, h0, ht, slews[b], J, s2, cut + 2 * n1) == SDRFM_OK);
        J = advance(J, n2);
        CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(l + n1 + n2, r + n1 + n2, n3, alpha, gain, h0, ht, slews[b], J, s2, cut + 2 * (n1 + n2)) == SDRFM_OK);
        CHECK(memcmp(one, cut, sizeof(int16_t) * 2 * n) == 0 && memcmp(s1, s2, sizeof s1) == 0);
        if (h0 == 32768 && ht == 32768) {                       /* the plain recursion bit for bit */
          float s3[2] = {0.25f, -0.5f};
          CHECK(sdrfm_pcm_deemph_stereo_s16(l, r, n, alpha, gain, s3, cut) == SDRFM_OK);
          CHECK(memcmp(one, cut, sizeof(int16_t) * 2 * n) == 0 && memcmp(s1, s3, sizeof s1) == 0);
        }
        /* a completed ramp: J = 65536 and UINT32_MAX are a flat ht */
        float s4[2] = {0.0f, 0.0f}, s5[2] = {0.0f, 0.0f}, s6[2] = {0.0f, 0.0f};
        CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(l, r, n, alpha, gain, h0, ht, slews[b], 65536u, s4, one) == SDRFM_OK);
        CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(l, r, n, alpha, gain, h0, ht, slews[b], UINT32_MAX, s5, cut) == SDRFM_OK);
        CHECK(memcmp(one, cut, sizeof(int16_t) * 2 * n) == 0 && memcmp(s4, s5, sizeof s4) == 0);
        CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(l, r, n, alpha, gain, ht, ht, 1, 0, s6, cut) == SDRFM_OK);
        CHECK(memcmp(one, cut, sizeof(int16_t) * 2 * n) == 0 && memcmp(s4, s6, sizeof s4) == 0);
      }
    free(l); free(r); free(one); free(cut);
  }
  /* the refusals: nothing is written */
  float x[4] = {1.0f, 2.0f, 3.0f, 4.0f}, st[2] = {0.5f, 0.5f};
  int16_t pcm[8];
  memset(pcm, 0x55, sizeof pcm);
  const int E = SDRFM_EINVAL;
  CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(NULL, x, 4, alpha, gain, 32768, 32768, 1, 0, st, pcm) == E);
  CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(x, NULL, 4, alpha, gain, 32768, 32768, 1, 0, st, pcm) == E);
  CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(x, x, 4, alpha, gain, 32768, 32768, 1, 0, st, NULL) == E);
  CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(x, x, 4, alpha, gain, 32768, 32768, 1, 0, NULL, pcm) == E);
  CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(x, x, 4, 0.0f, gain, 32768, 32768, 1, 0, st, pcm) == E);
  CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(x, x, 4, 1.5f, gain, 32768, 32768, 1, 0, st, pcm) == E);
  CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(x, x, 4, alpha, gain, 1023, 32768, 1, 0, st, pcm) == E);
  CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(x, x, 4, alpha, gain, 32769, 32768, 1, 0, st, pcm) == E);
  CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(x, x, 4, alpha, gain, 32768, 1023, 1, 0, st, pcm) == E);
  CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(x, x, 4, alpha, gain, 32768, 65535, 1, 0, st, pcm) == E);
  CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(x, x, 4, alpha, gain, 32768, 32768, 0, 0, st, pcm) == E);
  CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(x, x, 4, alpha, gain, 32768, 32768, 32769, 0, st, pcm) == E);
  for (unsigned i = 0; i < 8; ++i) CHECK(pcm[i] == 0x5555);
  CHECK(st[0] == 0.5f && st[1] == 0.5f);
  CHECK(sdrfm_pcm_deemph_stereo_hicut_s16(NULL, NULL, 0, alpha, gain, 1024, 32768, 32768, 0, st, NULL) == SDRFM_OK);
  printf("ok\n");
  return 0;
}
