/* tests/native/loudness_sanity.c — the plain-C host side of the loudness meter (csrc/loudness.c) walked over its edges under ASan and UBSan:
 * exactly sized heap rows, every cut of a 300-pair row into two calls at block_len 64, every refusal, the gate's NaN and -inf cases.
 * Prints "ok". */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/sdrfm.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      printf("FAILED line %d: %s\n", __LINE__, #c);                     \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

static uint32_t lcg(uint32_t* s) { *s = *s * 1664525u + 1013904223u; return *s >> 8; }

int main(void) {
  sdrfm_loudness_coef c;
  CHECK(sdrfm_loudness_default_coef(&c) == SDRFM_OK && sdrfm_loudness_check_coef(&c) == SDRFM_OK);
  CHECK(sdrfm_loudness_default_coef(NULL) == SDRFM_EINVAL && sdrfm_loudness_check_coef(NULL) == SDRFM_EINVAL);
  enum { N = 300, B = 64 };
  uint32_t seed = 7;
  int16_t* row = (int16_t*)malloc(sizeof(int16_t) * 2 * N);                      /* exactly sized: a read past 2n is caught */
  for (int i = 0; i < 2 * N; ++i) row[i] = (int16_t)((int)(lcg(&seed) & 0xFFFF) - 32768);
  sdrfm_loudness_block* whole = (sdrfm_loudness_block*)malloc(sizeof(*whole) * (N / B));
  sdrfm_loudness_state s0, s;
  uint32_t nb = 0;
  memset(&s0, 0, sizeof(s0));
  CHECK(sdrfm_pcm_loudness_s16(row, N, &c, B, &s0, whole, N / B, &nb) == SDRFM_OK && nb == N / B && s0.pos == N);
  for (uint32_t k = 0; k < nb; ++k) CHECK(whole[k].e_l > 0.0 && whole[k].e_r > 0.0);
  CHECK(s0.e[0] > 0.0);                                                          /* 300 = 4 x 64 + 44: a sub-block is open */
  for (uint32_t cut = 0; cut <= N; ++cut) {                                      /* every cut: the same sequence of operations, so the same bits */
    const uint32_t n1 = cut / B, n2 = N / B - n1;
    int16_t* a = (int16_t*)malloc(sizeof(int16_t) * 2 * cut + 1);
    int16_t* b = (int16_t*)malloc(sizeof(int16_t) * 2 * (N - cut) + 1);
    sdrfm_loudness_block* oa = (sdrfm_loudness_block*)malloc(sizeof(*oa) * n1 + 1);   /* exactly what each call completes */
    sdrfm_loudness_block* ob = (sdrfm_loudness_block*)malloc(sizeof(*ob) * n2 + 1);
    memcpy(a, row, sizeof(int16_t) * 2 * cut);
    memcpy(b, row + 2 * cut, sizeof(int16_t) * 2 * (N - cut));
    memset(&s, 0, sizeof(s));
    uint32_t ka = 99, kb = 99;
    CHECK(sdrfm_pcm_loudness_s16(a, cut, &c, B, &s, oa, n1, &ka) == SDRFM_OK && ka == n1 && s.pos == cut);
    CHECK(sdrfm_pcm_loudness_s16(b, N - cut, &c, B, &s, ob, n2, &kb) == SDRFM_OK && kb == n2 && s.pos == N);
    for (uint32_t k = 0; k < N / B; ++k) {
      const sdrfm_loudness_block* g = k < n1 ? &oa[k] : &ob[k - n1];
      CHECK(g->e_l == whole[k].e_l && g->e_r == whole[k].e_r);
    }
    CHECK(memcmp(&s, &s0, sizeof(s)) == 0);
    free(a); free(b); free(oa); free(ob);
  }
  /* every refusal, with nothing changed */
  sdrfm_loudness_state before = s0;
  sdrfm_loudness_block out[8];
  sdrfm_loudness_coef bad = c;
  nb = 77;
  CHECK(sdrfm_pcm_loudness_s16(NULL, 5, &c, B, &s0, out, 8, &nb) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_loudness_s16(row, 5, NULL, B, &s0, out, 8, &nb) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_loudness_s16(row, 5, &c, B, NULL, out, 8, &nb) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_loudness_s16(row, 5, &c, B, &s0, out, 8, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_loudness_s16(row, 5, &c, 63, &s0, out, 8, &nb) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_loudness_s16(row, 5, &c, (1u << 20) + 1u, &s0, out, 8, &nb) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_loudness_s16(row, 100, &c, B, &s0, out, 0, &nb) == SDRFM_ECAPACITY);   /* 44 + 100 pairs complete two sub-blocks */
  CHECK(sdrfm_pcm_loudness_s16(row, 100, &c, B, &s0, out, 1, &nb) == SDRFM_ECAPACITY);
  CHECK(sdrfm_pcm_loudness_s16(row, 100, &c, B, &s0, NULL, 8, &nb) == SDRFM_EINVAL);
  bad.c[4] = 1.0;                                                                /* a pole on the circle */
  CHECK(sdrfm_loudness_check_coef(&bad) == SDRFM_EINVAL && sdrfm_pcm_loudness_s16(row, 5, &bad, B, &s0, out, 8, &nb) == SDRFM_EINVAL);
  bad = c; bad.c[8] = -(1.0 + c.c[9]);
  CHECK(sdrfm_loudness_check_coef(&bad) == SDRFM_EINVAL);
  bad = c; bad.c[1] = NAN;
  CHECK(sdrfm_loudness_check_coef(&bad) == SDRFM_EINVAL);
  bad = c; bad.c[6] = INFINITY;
  CHECK(sdrfm_loudness_check_coef(&bad) == SDRFM_EINVAL);
  CHECK(nb == 77 && memcmp(&before, &s0, sizeof(s0)) == 0);
  CHECK(sdrfm_pcm_loudness_s16(NULL, 0, &c, B, &s0, NULL, 0, &nb) == SDRFM_OK && nb == 0 && memcmp(&before, &s0, sizeof(s0)) == 0);
  CHECK(sdrfm_pcm_loudness_s16(row, 100, &c, B, &s0, out, 2, &nb) == SDRFM_OK && nb == 2 && s0.pos == 400);
  /* the gate */
  sdrfm_loudness_gate_t* g = (sdrfm_loudness_gate_t*)row;
  sdrfm_loudness_report_t r;
  CHECK(sdrfm_loudness_gate_create(4800, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_loudness_gate_create(63, &g) == SDRFM_EINVAL && g == NULL);
  CHECK(sdrfm_loudness_gate_create((1u << 20) + 1u, &g) == SDRFM_EINVAL);
  CHECK(sdrfm_loudness_gate_create(4800, &g) == SDRFM_OK && g);
  CHECK(sdrfm_loudness_gate_report(g, &r) == SDRFM_OK);                          /* nothing pushed: NaN throughout */
  CHECK(isnan(r.m) && isnan(r.s) && isnan(r.i) && isnan(r.lra) && isnan(r.max_m) && isnan(r.max_s) && r.n_blocks == 0 && r.n_gating == 0);
  sdrfm_loudness_block zero[40], loud[40];
  for (int k = 0; k < 40; ++k) {
    zero[k].e_l = zero[k].e_r = 0.0;
    loud[k].e_l = loud[k].e_r = 4800.0 * 32768.0 * 32768.0 * 0.005;             /* z = 0.01: -20.691 LUFS */
  }
  CHECK(sdrfm_loudness_gate_push(g, zero, 3) == SDRFM_OK && sdrfm_loudness_gate_report(g, &r) == SDRFM_OK);
  CHECK(isnan(r.m) && isnan(r.i) && r.n_blocks == 3);                            /* too few for a gating block */
  CHECK(sdrfm_loudness_gate_push(g, zero, 30) == SDRFM_OK && sdrfm_loudness_gate_report(g, &r) == SDRFM_OK);
  CHECK(isinf(r.m) && r.m < 0 && isinf(r.s) && r.s < 0 && isinf(r.i) && r.i < 0 && isinf(r.max_m) && isnan(r.lra));   /* zero power */
  CHECK(r.n_blocks == 33 && r.n_gating == 30 && r.n_abs == 0 && r.n_rel == 0 && r.n_short == 4 && r.n_short_abs == 0);
  CHECK(sdrfm_loudness_gate_reset(g) == SDRFM_OK && sdrfm_loudness_gate_report(g, &r) == SDRFM_OK && isnan(r.m) && r.n_blocks == 0);
  CHECK(sdrfm_loudness_gate_push(g, loud, 29) == SDRFM_OK && sdrfm_loudness_gate_report(g, &r) == SDRFM_OK);
  CHECK(fabs(r.m + 20.691) < 1e-9 && fabs(r.i + 20.691) < 1e-9 && isnan(r.s) && isnan(r.lra) && r.n_gating == 26 && r.n_rel == 26);
  CHECK(sdrfm_loudness_gate_push(g, loud, 1) == SDRFM_OK && sdrfm_loudness_gate_report(g, &r) == SDRFM_OK);
  CHECK(fabs(r.s + 20.691) < 1e-9 && r.lra == 0.0 && r.n_short == 1 && r.n_short_rel == 1 && fabs(r.max_s + 20.691) < 1e-9);
  loud[0].e_l = -1.0;
  CHECK(sdrfm_loudness_gate_push(g, loud, 2) == SDRFM_EINVAL);
  loud[0].e_l = NAN;
  CHECK(sdrfm_loudness_gate_push(g, loud, 2) == SDRFM_EINVAL);
  CHECK(sdrfm_loudness_gate_push(NULL, loud, 1) == SDRFM_EINVAL && sdrfm_loudness_gate_push(g, NULL, 1) == SDRFM_EINVAL);
  CHECK(sdrfm_loudness_gate_push(g, NULL, 0) == SDRFM_OK);
  CHECK(sdrfm_loudness_gate_report(NULL, &r) == SDRFM_EINVAL && sdrfm_loudness_gate_report(g, NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_loudness_gate_reset(NULL) == SDRFM_EINVAL);
  CHECK(sdrfm_loudness_gate_report(g, &r) == SDRFM_OK && r.n_blocks == 30);     /* the refused pushes took nothing */
  sdrfm_loudness_gate_free(g);
  sdrfm_loudness_gate_free(NULL);
  free(whole);
  free(row);
  printf("ok\n");
  return 0;
}
