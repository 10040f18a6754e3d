/*
 * sdrfm_pcm_rows.h — the argument checks the PCM-side handles make of their (L, R) rows before any device work: pure
 * functions, no HIP, so that a program of its own holds them on the CPU (tests/native/pcm_rows_check.cpp).  Internal: no part of the C-ABI.
 * Rows are int16, interleaved L, R; strides count int16; n counts pairs.
 */
#ifndef SDRFM_PCM_ROWS_H
#define SDRFM_PCM_ROWS_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/sdrfm.h"

#define PCM_PAIR_BYTES (2 * sizeof(int16_t))   /* one (L, R) pair */
#define PCM_ROWS_EMPTY (-1)   /* pcm_rows_refusal: n == 0, nothing to do; the entry answers SDRFM_OK (no status is negative) */

/* the opening of sdrfm_pcm_limit_process_batch, sdrfm_pcm_mix_process_batch and sdrfm_pcm_rate_process_batch, in their order: unknown flags, n over
 * the handle's maximum, an odd stride (rows are read and written as (L, R) dwords), n == 0, null rows, device rows off a 4-byte boundary.
 * SDRFM_OK: go on; SDRFM_EINVAL; or PCM_ROWS_EMPTY. */
static inline int pcm_rows_refusal(uint32_t flags, uint32_t allowed_flags, uint32_t n, uint32_t n_max, const void* in, size_t in_stride, const void* out,
                                   size_t out_stride) {
  if (flags & ~allowed_flags) return SDRFM_EINVAL;
  if (n > n_max) return SDRFM_EINVAL;
  if ((in_stride | out_stride) & 1u) return SDRFM_EINVAL;
  if (n == 0) return PCM_ROWS_EMPTY;
  if (!in || !out) return SDRFM_EINVAL;
  if ((flags & SDRFM_F_DEVICE_PTRS) && ((uintptr_t)in % 4 != 0 || (uintptr_t)out % 4 != 0)) return SDRFM_EINVAL;
  return SDRFM_OK;
}

/* the SDRFM_ECAPACITY rule: `rows` rows `stride` elements apart hold `need` elements each; a single row ignores its stride */
static inline int pcm_rows_capacity(size_t rows, size_t stride, size_t need) { return rows <= 1 || stride >= need; }

/* the distance a call walks from row to row: the stride, or for a single row, whose stride is ignored, the row itself */
static inline size_t pcm_rows_pitch(size_t rows, size_t stride, size_t need) { return rows > 1 ? stride : need; }

/* the mix bus's rule (bus b writes while bus c reads): the bytes from the first input row's first pair to the last one's n-th, and the same of the
 * output rows, share no byte.  Ranges that only touch are apart.  Pitches as pcm_rows_pitch gives them; rows >= 1, n >= 1. */
static inline int pcm_rows_apart(const int16_t* in, size_t in_rows, size_t in_pitch, const int16_t* out, size_t out_rows, size_t out_pitch, uint32_t n) {
  const uintptr_t in0 = (uintptr_t)in, in1 = in0 + sizeof(int16_t) * ((in_rows - 1u) * in_pitch + 2 * (size_t)n);
  const uintptr_t out0 = (uintptr_t)out, out1 = out0 + sizeof(int16_t) * ((out_rows - 1u) * out_pitch + 2 * (size_t)n);
  return !(in0 < out1 && out0 < in1);
}

/* the capacity a staging buffer grows to for n elements per row: n rounded up to a multiple of `round`, a power of two (1024 pairs; the IQ
 * meter: a workgroup's 4096 bytes).  In uint32 the sum wraps for n > UINT32_MAX - (round - 1) and the answer is then 0: every caller has held n
 * to its handle's maximum before (2^20 pairs, 2^26 bytes), far below that. */
static inline uint32_t stage_cap(uint32_t n, uint32_t round) { return (n + (round - 1u)) & ~(round - 1u); }

#endif
