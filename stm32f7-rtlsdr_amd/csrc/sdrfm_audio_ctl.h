/*
 * sdrfm_audio_ctl.h — the ramps of the broadcast receiver's per-stream stereo blend and output gain (include/sdrfm.h): the
 * one copy of the arithmetic that k_bcast's blended output stage, sdrfm_bcast_set_audio and sdrfm_bcast_get_audio all use.
 *
 * A ramp is four plain integers: where it started (x0), where it goes (xt), both Q15 in [0, 32768], the handle's slew in 1 .. 32768 units
 * per audio output, and n, the audio outputs since the ramp was set.  "Move towards the target by at most slew per output" has the closed
 * form
 *     k = min(n, cdiv(|xt - x0|, slew)),   x(n) = x0 + sgn(xt - x0) min(k slew, |xt - x0|)
 * and min(k slew, |xt - x0|) = min(min(n, 65536) slew, |xt - x0|): below the ramp's end both are n slew, from it on both are the whole
 * distance (cdiv(..) <= 32768).  The second form needs no division and stays inside 32 bits (65536 x 32768 = 2^31), so that is what is
 * evaluated; tests/native/audio_ctl_check.cpp holds it to the first form and to the one-output-at-a-time iteration.
 * Evaluated from values, never from carried device state: any cut of a capture into calls gives the same integers.
 *
 * Plain integers, no HIP types in the arithmetic: the CPU check compiles this header with a host compiler alone.
 * Internal to the library; the drop-in boundary is include/sdrfm.h.
 */
#ifndef SDRFM_AUDIO_CTL_H
#define SDRFM_AUDIO_CTL_H

#include <stdint.h>

#if defined(__HIPCC__)
#define SDRFM_ACTL_FN __host__ __device__ __forceinline__
#else
#define SDRFM_ACTL_FN static inline
#endif

#define SDRFM_ACTL_ONE 32768u        /* Q15 1.0: the largest blend, gain and slew */
#define SDRFM_ACTL_J_MAX 65536u      /* the outputs-since-set count saturates here: every ramp has ended by then */

/* one stream's record, as the kernel reads it: 16 bytes */
struct AudioCtlRec {
  uint32_t b0, bt;                   /* blend: the ramp's start and its target */
  uint32_t v0, vt;                   /* gain likewise */
};

/* the ramp's value after n outputs (n = 0: x0 itself); output j of a call that starts J outputs after the set uses n = J + j + 1 */
SDRFM_ACTL_FN uint32_t audio_ctl_ramp(uint32_t x0, uint32_t xt, uint32_t slew, uint32_t n) {
  const uint32_t up = xt >= x0 ? 1u : 0u, dist = up ? xt - x0 : x0 - xt;
  const uint32_t run = (n < SDRFM_ACTL_J_MAX ? n : SDRFM_ACTL_J_MAX) * slew, move = run < dist ? run : dist;
  return up ? x0 + move : x0 - move;
}

/* the count after `outputs` more, saturated */
SDRFM_ACTL_FN uint32_t audio_ctl_advance(uint32_t J, uint32_t outputs) {
  const uint64_t n = (uint64_t)J + outputs;
  return n < SDRFM_ACTL_J_MAX ? (uint32_t)n : SDRFM_ACTL_J_MAX;
}

/* the host's rebase at a set: the ramps restart (J = 0 from here on) at the values they have reached after J outputs, towards new targets —
 * bt / vt, or the old target where the pointer is NULL */
SDRFM_ACTL_FN void audio_ctl_rebase(struct AudioCtlRec* r, uint32_t slew, uint32_t J, const uint16_t* bt, const uint16_t* vt) {
  r->b0 = audio_ctl_ramp(r->b0, r->bt, slew, J);
  r->v0 = audio_ctl_ramp(r->v0, r->vt, slew, J);
  if (bt) r->bt = *bt;
  if (vt) r->vt = *vt;
}

#endif
