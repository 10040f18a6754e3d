/* The plain-C host side of the limiter's true-peak form (csrc/limit_tp.c over csrc/limit.c and csrc/truepeak.c) walked over its
 * edges under ASan and UBSan by tests/test_limit_tp_cpu.py: every refusal with nothing touched, the extremes of every range with buffers of
 * exactly the documented sizes, in-place calls, and a cut at every length from 0 to D + H + 1 against one call. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sdrfm.h"

static int fails = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++fails; } \
  } while (0)

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd(void) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 16);
}

static sdrfm_pcm_limit_rec identity(void) {
  sdrfm_pcm_limit_rec r;
  r.n = 0; r.limited = 0; r.min_gain = 32768u; r.at = 0;
  return r;
}

/* one call with heap buffers of exactly the documented sizes, so that a byte too far is a finding */
static int call(const int16_t* x, uint32_t n, uint32_t lw, const sdrfm_pcm_limit_params* par, const int16_t* coef, uint32_t P, uint32_t nt,
                int32_t* state, int16_t* y, sdrfm_pcm_limit_rec* rec, int in_place) {
  int16_t* in = (int16_t*)malloc(sizeof(int16_t) * 2 * (size_t)n + 1);
  int16_t* out = in_place ? in : (int16_t*)malloc(sizeof(int16_t) * 2 * (size_t)n + 1);
  int16_t* tab = coef ? (int16_t*)malloc(sizeof(int16_t) * P * nt) : NULL;
  const uint32_t words = sdrfm_pcm_tplimit_state_words(lw, coef ? nt : 12u);
  int32_t* st = (int32_t*)malloc(sizeof(int32_t) * words);
  memcpy(in, x, sizeof(int16_t) * 2 * (size_t)n);
  if (tab) memcpy(tab, coef, sizeof(int16_t) * P * nt);
  memcpy(st, state, sizeof(int32_t) * words);
  const int rc = sdrfm_pcm_tplimit_s16(n ? in : NULL, n, lw, 3, 5, par, tab, P, nt, st, n ? out : NULL, rec);
  memcpy(y, out, sizeof(int16_t) * 2 * (size_t)n);
  memcpy(state, st, sizeof(int32_t) * words);
  if (!in_place) free(out);
  free(in); free(tab); free(st);
  return rc;
}

int main(void) {
  int16_t def[48];
  uint32_t P = 0, NT = 0;
  CHECK(sdrfm_truepeak_default_coef(def, &P, &NT) == SDRFM_OK && P == 4 && NT == 12);
  /* the sizes */
  CHECK(sdrfm_pcm_tplimit_state_words(2, 12) == 0 && sdrfm_pcm_tplimit_latency(2, 12) == 0);      /* 2^2 < 6 */
  CHECK(sdrfm_pcm_tplimit_state_words(3, 12) == 40 && sdrfm_pcm_tplimit_latency(3, 12) == 13);
  CHECK(sdrfm_pcm_tplimit_state_words(2, 4) == 16 && sdrfm_pcm_tplimit_state_words(2, 8) == 20 && sdrfm_pcm_tplimit_state_words(5, 64) == 188);
  CHECK(sdrfm_pcm_tplimit_state_words(4, 64) == 0 && sdrfm_pcm_tplimit_state_words(1, 4) == 0 && sdrfm_pcm_tplimit_state_words(9, 4) == 0);
  CHECK(sdrfm_pcm_tplimit_state_words(8, 6) == 0 && sdrfm_pcm_tplimit_state_words(8, 68) == 0 && sdrfm_pcm_tplimit_state_words(8, 0) == 0);
  CHECK(sdrfm_pcm_tplimit_state_words(8, 64) == 4 * 255 + 64 && sdrfm_pcm_tplimit_latency(8, 64) == 287);
  int32_t st[4 * 255 + 64], st0[4 * 255 + 64];
  CHECK(sdrfm_pcm_tplimit_state_init(3, 12, NULL) == SDRFM_EINVAL && sdrfm_pcm_tplimit_state_init(2, 12, st) == SDRFM_EINVAL);
  CHECK(sdrfm_pcm_tplimit_state_init(3, 12, st) == SDRFM_OK);
  for (int k = 0; k < 40; ++k) CHECK(st[k] == (k < 26 ? 0 : k < 33 ? 32768 : 1 << 23));
  /* every refusal, with nothing touched */
  const sdrfm_pcm_limit_params good = {29204u, 874u, 4096u, 4096u};
  sdrfm_pcm_limit_params bad = good;
  bad.gain_t = 65537u;
  int16_t x[64], y[64], over[48];
  for (int k = 0; k < 64; ++k) { x[k] = (int16_t)(1000 * k); y[k] = 77; }
  memcpy(over, def, sizeof(over));
  over[0] = 32767; over[1] = 32767; over[2] = 2;                                                 /* half a row over the bound */
  sdrfm_pcm_limit_rec rec = {5, 1, 30000, 2}, rec0 = rec;
  memcpy(st0, st, sizeof(st));
#define REFUSED(expr)                                                                                  \
  do {                                                                                                 \
    CHECK((expr) == SDRFM_EINVAL);                                                                     \
    CHECK(!memcmp(st, st0, sizeof(st)) && !memcmp(&rec, &rec0, sizeof(rec)));                          \
    for (int k_ = 0; k_ < 64; ++k_) CHECK(y[k_] == 77);                                                \
  } while (0)
  REFUSED(sdrfm_pcm_tplimit_s16(NULL, 8, 3, 1, 0, &good, def, 4, 12, st, y, &rec));
  REFUSED(sdrfm_pcm_tplimit_s16(x, 8, 3, 1, 0, &good, def, 4, 12, st, NULL, &rec));
  REFUSED(sdrfm_pcm_tplimit_s16(x, 8, 3, 1, 0, NULL, def, 4, 12, st, y, &rec));
  REFUSED(sdrfm_pcm_tplimit_s16(x, 8, 3, 1, 0, &good, def, 4, 12, NULL, y, &rec));
  REFUSED(sdrfm_pcm_tplimit_s16(x, 8, 3, 1, 0, &good, def, 4, 12, st, y, NULL));
  REFUSED(sdrfm_pcm_tplimit_s16(x, 8, 3, 1, 0, &bad, def, 4, 12, st, y, &rec));
  REFUSED(sdrfm_pcm_tplimit_s16(x, (1u << 20) + 1u, 3, 1, 0, &good, def, 4, 12, st, y, &rec));
  REFUSED(sdrfm_pcm_tplimit_s16(x, 8, 3, 1, 65537, &good, def, 4, 12, st, y, &rec));
  REFUSED(sdrfm_pcm_tplimit_s16(x, 8, 3, 0, 0, &good, def, 4, 12, st, y, &rec));
  REFUSED(sdrfm_pcm_tplimit_s16(x, 8, 9, 1, 0, &good, def, 4, 12, st, y, &rec));
  REFUSED(sdrfm_pcm_tplimit_s16(x, 8, 2, 1, 0, &good, def, 4, 12, st, y, &rec));                 /* 2^LW < NT / 2 */
  REFUSED(sdrfm_pcm_tplimit_s16(x, 8, 2, 1, 0, &good, NULL, 0, 0, st, y, &rec));                 /* likewise with the default table */
  REFUSED(sdrfm_pcm_tplimit_s16(x, 8, 3, 1, 0, &good, def, 3, 12, st, y, &rec));                 /* the table's shape ... */
  REFUSED(sdrfm_pcm_tplimit_s16(x, 8, 3, 1, 0, &good, def, 4, 10, st, y, &rec));
  REFUSED(sdrfm_pcm_tplimit_s16(x, 8, 3, 1, 0, &good, over, 4, 12, st, y, &rec));                /* ... and its bound */
  /* every shape at the extremes of the ranges: one call against a cut at every length from 0 to D + H + 1, out of place and in place */
  const uint32_t shapes[][3] = {{3, 4, 12}, {6, 4, 12}, {8, 4, 12}, {2, 8, 4}, {5, 2, 64}, {8, 8, 64}};
  const sdrfm_pcm_limit_params pars[] = {{29204u, 874u, 4096u, 4096u}, {1u, 1u, 65536u, 65536u}, {32767u, 1u << 23, 65536u, 0u}, {12000u, 5000u, 0u, 65536u}};
  int16_t tab[8 * 64];
  for (size_t sh = 0; sh < sizeof(shapes) / sizeof(shapes[0]); ++sh) {
    const uint32_t lw = shapes[sh][0], p_ = shapes[sh][1], nt = shapes[sh][2], lat = sdrfm_pcm_tplimit_latency(lw, nt);
    const uint32_t words = sdrfm_pcm_tplimit_state_words(lw, nt);
    const int use_def = p_ == 4 && nt == 12;
    for (uint32_t p = 0; p < p_; ++p)                                                             /* each half-row at the bound */
      for (uint32_t k = 0; k < nt; ++k) {
        const uint32_t j = k % (nt / 2u);
        tab[p * nt + k] = (int16_t)(j == 0 ? 32767 : j == 1 ? -32768 : 0);
      }
    CHECK(sdrfm_truepeak_check_coef(tab, p_, nt) == SDRFM_OK);
    CHECK(words == 4 * ((1u << lw) - 1u) + nt && lat == (1u << lw) - 1u + nt / 2u);
    for (size_t q = 0; q < sizeof(pars) / sizeof(pars[0]); ++q) {
      const uint32_t total = (lat + 2) * (lat + 3) / 2 + 700;                                     /* every length 0 .. D + H + 1, then the rest */
      int16_t* row = (int16_t*)malloc(sizeof(int16_t) * 2 * total);
      int16_t* whole = (int16_t*)malloc(sizeof(int16_t) * 2 * total);
      int16_t* parts = (int16_t*)malloc(sizeof(int16_t) * 2 * total);
      for (uint32_t k = 0; k < 2 * total; ++k) row[k] = (rnd() & 7u) ? (int16_t)(rnd() & 0xFFFFu) : ((rnd() & 1u) ? 32767 : -32768);
      int32_t a[4 * 255 + 64], b[4 * 255 + 64];
      CHECK(sdrfm_pcm_tplimit_state_init(lw, nt, a) == SDRFM_OK && sdrfm_pcm_tplimit_state_init(lw, nt, b) == SDRFM_OK);
      sdrfm_pcm_limit_rec ra = identity(), rb = identity();
      const int16_t* c = use_def ? NULL : tab;
      CHECK(call(row, total, lw, &pars[q], c, p_, nt, a, whole, &ra, 0) == SDRFM_OK);
      for (uint32_t k = 0; k < 2 * total; ++k) CHECK((uint32_t)abs((int)whole[k]) <= pars[q].ceiling);
      /* a cut at every length: the call's J is fixed in `call`, so the pieces use the sample form's closed-form ramp at a fixed J too — the cuts
       * are compared under gain0 == gain_t only, where J does not matter */
      if (pars[q].gain0 == pars[q].gain_t) {
        uint32_t at = 0, len = 0;
        while (at < total) {
          const uint32_t m = len <= lat + 1 ? len : total - at;
          const uint32_t take = m < total - at ? m : total - at;
          CHECK(call(row + 2 * at, take, lw, &pars[q], c, p_, nt, b, parts + 2 * at, &rb, (int)(len & 1u)) == SDRFM_OK);
          at += take;
          ++len;
        }
        CHECK(!memcmp(whole, parts, sizeof(int16_t) * 2 * total) && !memcmp(a, b, sizeof(int32_t) * words) && !memcmp(&ra, &rb, sizeof(ra)));
      }
      free(row); free(whole); free(parts);
    }
  }
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
