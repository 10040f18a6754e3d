/* Drives csrc/rds.c under UBSan (bounds included) on the CPU: every sample rate the decoder accepts at its edges, noise, a square
 * biphase signal with a drifting clock, one-sample pushes, a tiny group buffer.  Prints "ok". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/sdrfm.h"

static uint32_t lcg(uint32_t* s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }

int main(void) {
  const double rates[] = {4750.0, 5000.0, 9600.0, 19000.0, 47500.0, 76000.0};
  uint32_t seed = 1;
  for (unsigned r = 0; r < sizeof rates / sizeof rates[0]; ++r) {
    sdrfm_rds_sync_t* s = NULL;
    if (sdrfm_rds_sync_create(rates[r], &s) != SDRFM_OK || !s) return 1;
    const uint32_t n = (uint32_t)(rates[r] * 1.5);
    float* bb = (float*)malloc(sizeof(float) * 2 * n);
    if (!bb) return 2;
    /* differentially coded blocks with valid check words, rectangular biphase symbols, clock 300 ppm fast, axis at 1 rad */
    const double spb = rates[r] / 1187.5 / 1.0003;
    int e = 0;
    uint32_t word = 0, nbit = 26, blk = 0;
    double t_next = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
      while ((double)i >= t_next) {
        if (nbit == 26) {
          const uint16_t info = (uint16_t)lcg(&seed);
          const int off = (int)(blk & 3) == 2 ? 2 : ((blk & 3) == 3 ? 4 : (int)(blk & 3));
          word = ((uint32_t)info << 10) | sdrfm_rds_checkword(info, off);
          nbit = 0; blk++;
        }
        e ^= (int)((word >> (25 - nbit)) & 1u);
        nbit++;
        t_next += spb;
      }
      const double frac = ((double)i - (t_next - spb)) / spb;
      const double v = (e ? 1.0 : -1.0) * (frac < 0.5 ? 1.0 : -1.0) * 0.01 + ((double)(lcg(&seed) & 1023) - 512.0) * 2e-6;
      bb[2 * i] = (float)(v * cos(1.0));
      bb[2 * i + 1] = (float)(v * sin(1.0));
    }
    bb[7] = NAN; bb[8] = INFINITY;                           /* non-finite samples count as silence */
    sdrfm_rds_group g[2];
    uint32_t got = 0, total = 0;
    for (uint32_t i = 0; i < 500 && i < n; ++i) {            /* one sample per push */
      if (sdrfm_rds_sync_push(s, bb + 2 * i, 1, g, 2, &got) != SDRFM_OK) return 3;
      total += got;
    }
    if (sdrfm_rds_sync_push(s, bb + 1000, n - 500, g, 2, &got) != SDRFM_OK || got > 2) return 4;   /* cap 2: the rest is dropped */
    sdrfm_rds_sync_info st;
    if (sdrfm_rds_sync_stats(s, &st) != SDRFM_OK) return 5;
    if (st.groups < 10 || st.blocks_ok < 40) { fprintf(stderr, "rate %g: %u groups, %llu blocks ok\n", rates[r], st.groups, (unsigned long long)st.blocks_ok); return 6; }
    if (sdrfm_rds_sync_reset(s) != SDRFM_OK) return 7;
    for (uint32_t i = 0; i < 2 * n; ++i) bb[i] = ((float)(lcg(&seed) & 4095) - 2048.0f) * 1e-5f;   /* noise */
    if (sdrfm_rds_sync_push(s, bb, n, g, 2, &got) != SDRFM_OK) return 8;
    if (sdrfm_rds_sync_push(s, bb, 0, NULL, 0, &got) != SDRFM_OK || got != 0) return 9;
    sdrfm_rds_sync_destroy(s);
    free(bb);
  }
  printf("ok\n");
  return 0;
}
