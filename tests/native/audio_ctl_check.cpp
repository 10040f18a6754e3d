/* CPU check of csrc/sdrfm_audio_ctl.h, the one copy of the blend and gain ramps the broadcast kernel and the host share.
 * Over slew in {1, 2, 3, 7, 40, 32767, 32768} and x0, xt in {0, 1, 2, 6, 7, 8, 16383, 32767, 32768}:
 *   - audio_ctl_ramp equals the one-output-at-a-time iteration "move towards the target by at most slew" for every n up to past the
 *     ramp's end, and include/sdrfm.h's closed form with its cdiv;
 *   - it is monotone, stays between x0 and xt, and is xt from the ramp's end on, up to n = 2^32 - 1;
 *   - ramp(x0, J1 + J2) == ramp(ramp(x0, J1), J2): a rebase in mid-ramp continues it;
 *   - saturating the count at 65536 changes nothing, and audio_ctl_advance saturates there;
 *   - audio_ctl_rebase moves both starts, keeps a target whose pointer is NULL and takes one that is given.
 * Built with -fsanitize=address,undefined by tests/test_audio_ctl_cpu.py; prints "ok" at the end. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_audio_ctl.h"

static const uint32_t SLEWS[] = {1, 2, 3, 7, 40, 32767, 32768};
static const uint32_t VALUES[] = {0, 1, 2, 6, 7, 8, 16383, 32767, 32768};
#define COUNT(a) (sizeof(a) / sizeof((a)[0]))

static long checks = 0;

static void fail(const char* what, uint32_t slew, uint32_t x0, uint32_t xt, uint32_t n, uint32_t got, uint32_t want) {
  fprintf(stderr, "%s: slew %u, x0 %u, xt %u, n %u: got %u, want %u\n", what, slew, x0, xt, n, got, want);
  exit(1);
}

static uint32_t step_once(uint32_t x, uint32_t xt, uint32_t slew) {
  if (x < xt) return xt - x > slew ? x + slew : xt;
  return x - xt > slew ? x - slew : xt;
}

/* include/sdrfm.h's form, with its division */
static uint32_t closed_form(uint32_t x0, uint32_t xt, uint32_t slew, uint32_t n) {
  const uint32_t dist = xt >= x0 ? xt - x0 : x0 - xt, steps = (dist + slew - 1) / slew, k = n < steps ? n : steps;
  const uint32_t move = k * slew < dist ? k * slew : dist;
  return xt >= x0 ? x0 + move : x0 - move;
}

int main(void) {
  for (size_t a = 0; a < COUNT(SLEWS); ++a)
    for (size_t b = 0; b < COUNT(VALUES); ++b)
      for (size_t c = 0; c < COUNT(VALUES); ++c) {
        const uint32_t slew = SLEWS[a], x0 = VALUES[b], xt = VALUES[c];
        const uint32_t dist = xt >= x0 ? xt - x0 : x0 - xt, end = (dist + slew - 1) / slew, past = end + 5;
        uint32_t x = x0;
        for (uint32_t n = 0; n <= past; ++n) {                   /* n = 0 is x0 itself */
          const uint32_t got = audio_ctl_ramp(x0, xt, slew, n);
          if (got != x) fail("iteration", slew, x0, xt, n, got, x);
          if (got != closed_form(x0, xt, slew, n)) fail("closed form", slew, x0, xt, n, got, closed_form(x0, xt, slew, n));
          if (n >= end && got != xt) fail("end", slew, x0, xt, n, got, xt);
          if (n + 1 == end && end && got == xt) fail("ends early", slew, x0, xt, n, got, xt);
          x = step_once(x, xt, slew);
          ++checks;
        }
        const uint32_t far[] = {65535u, 65536u, 65537u, 1u << 20, 0x7fffffffu, 0xffffffffu};
        for (size_t f = 0; f < COUNT(far); ++f) {
          const uint32_t got = audio_ctl_ramp(x0, xt, slew, far[f]);
          const uint32_t want = closed_form(x0, xt, slew, far[f] < 65536u ? far[f] : 65536u);
          if (got != want) fail("far", slew, x0, xt, far[f], got, want);
          const uint32_t sat = far[f] < SDRFM_ACTL_J_MAX ? far[f] : SDRFM_ACTL_J_MAX;
          if (got != audio_ctl_ramp(x0, xt, slew, sat)) fail("saturated count", slew, x0, xt, far[f], got, audio_ctl_ramp(x0, xt, slew, sat));
          ++checks;
        }
        /* composition: every J1 up to past the end at a stride that keeps the run short, J2 likewise */
        const uint32_t stride1 = past / 37 + 1, stride2 = past / 29 + 1;
        for (uint32_t j1 = 0; j1 <= past; j1 += stride1) {
          const uint32_t mid = audio_ctl_ramp(x0, xt, slew, j1);
          for (uint32_t j2 = 0; j2 <= past; j2 += stride2) {
            const uint32_t got = audio_ctl_ramp(mid, xt, slew, j2), want = audio_ctl_ramp(x0, xt, slew, j1 + j2);
            if (got != want) fail("composition", slew, x0, xt, j1 * 100000u + j2, got, want);
            ++checks;
          }
          /* the same through the host's rebase, towards a new target and towards the kept one */
          struct AudioCtlRec r = {x0, xt, xt, x0};
          const uint16_t nb = (uint16_t)VALUES[(b + c) % COUNT(VALUES)];
          audio_ctl_rebase(&r, slew, j1, &nb, NULL);
          if (r.b0 != mid || r.bt != nb) fail("rebase blend", slew, x0, xt, j1, r.b0, mid);
          if (r.v0 != audio_ctl_ramp(xt, x0, slew, j1) || r.vt != x0) fail("rebase gain", slew, x0, xt, j1, r.v0, r.vt);
          ++checks;
        }
      }
  /* the count */
  if (audio_ctl_advance(0, 0) != 0 || audio_ctl_advance(5, 7) != 12 || audio_ctl_advance(65535, 1) != 65536 || audio_ctl_advance(65536, 1) != 65536 ||
      audio_ctl_advance(1, 0xffffffffu) != 65536 || audio_ctl_advance(65536, 0xffffffffu) != 65536 || audio_ctl_advance(0, 65535) != 65535) {
    fprintf(stderr, "audio_ctl_advance\n");
    return 1;
  }
  if (sizeof(struct AudioCtlRec) != 16) {
    fprintf(stderr, "the record is %zu bytes\n", sizeof(struct AudioCtlRec));
    return 1;
  }
  printf("%ld checks\nok\n", checks);
  return 0;
}
