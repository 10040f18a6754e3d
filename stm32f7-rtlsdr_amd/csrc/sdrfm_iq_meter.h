/*
 * sdrfm_iq_meter.h — the raw-capture IQ meter's launch geometry, its per-dword arithmetic and the kernel body (include/sdrfm.h).
 * The geometry and the arithmetic are plain functions a CPU program can include (tests/native/iq_meter_check.cpp walks them); the body is
 * compiled by hipcc only.
 *
 * A row of nbytes at any byte address is cut into
 *     head    pairs in front of the first LOGICAL vector, at most 8
 *     nvec    logical vectors of 16 bytes = 8 pairs, each starting with an I
 *     tail    pairs behind the last vector, at most 7
 * An even address: the vectors are the 16-byte aligned ones.  An ODD address puts every aligned dword at Q I Q I, and every pair across two
 * dwords; there the logical vector k is the aligned vector k shifted by ONE byte — bytes 1 .. 15 of the aligned load and the byte behind it,
 * which is always a byte of the row — so that its dwords read I Q I Q again and the one arithmetic serves both.  `odd` is the parity of the
 * row's address and with it of every aligned address in the row: the shift is decided once per row.
 * The grid is streams x bps workgroups; workgroup b of a row takes the vectors [b share, (b + 1) share) below nvec, lane t the vectors
 * t, t + 256, ... of that share, and workgroup 0 takes the head and tail pairs with its lanes 0 .. 14.  share is a multiple of IQM_NT and
 * at most IQM_NT * IQM_MAX_ITERS, which is what keeps a lane's sums in 32 bits (iqm_lane_bound).
 */
#ifndef SDRFM_IQ_METER_H
#define SDRFM_IQ_METER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define IQM_HD __host__ __device__ inline
#else
#define IQM_HD static inline
#endif

#define IQM_NT 256u            /* lanes of a workgroup */
#define IQM_VEC 16u            /* bytes of a vector */
#define IQM_CHUNK (IQM_NT * IQM_VEC)   /* bytes a workgroup takes per step: 4096 */
#define IQM_MAX_ITERS 4096u    /* vectors per lane at the most */
#define IQM_GRID_TARGET 2048u  /* workgroups that fill the machine: 256 CUs x 8 */
#define IQM_MAX_BYTES (64u << 20)
#define IQM_MAX_STREAMS 65536u
#define IQM_HIST_REPL 16u      /* copies of the 512 bins in LDS, one per lane & 15 */

typedef struct IqmRow { uint32_t odd, head, nvec, tail; } IqmRow;   /* head and tail in BYTES, both even */

/* the cut of a row at byte address addr */
IQM_HD IqmRow iqm_row(uintptr_t addr, uint32_t nbytes) {
  IqmRow g;
  g.odd = (uint32_t)(addr & 1u);
  const uint32_t lead = ((0u - (uint32_t)(addr & 15u)) & 15u) + g.odd;   /* to the aligned address, and one byte on where that one holds a Q */
  g.head = lead < nbytes ? lead : nbytes;
  g.nvec = (nbytes - g.head) / IQM_VEC;
  g.tail = nbytes - g.head - g.nvec * IQM_VEC;
  return g;
}

typedef struct IqmGrid { uint32_t bps, share; } IqmGrid;            /* workgroups per stream; vectors per workgroup */

/* the split of n_streams rows of nbytes: enough workgroups to fill the machine from ONE stream, none without a whole step of work unless the row is
 * that short, and no lane beyond IQM_MAX_ITERS vectors */
IQM_HD IqmGrid iqm_grid(uint32_t n_streams, uint32_t nbytes) {
  IqmGrid g;
  const uint32_t nv = nbytes / IQM_VEC, steps = (nv + IQM_NT - 1u) / IQM_NT;
  uint32_t want = (IQM_GRID_TARGET + n_streams - 1u) / n_streams;
  if (want > steps) want = steps;
  const uint32_t least = (steps + IQM_MAX_ITERS - 1u) / IQM_MAX_ITERS;
  if (want < least) want = least;
  if (want < 1u) want = 1u;
  g.bps = want;
  g.share = ((steps + want - 1u) / want) * IQM_NT;
  return g;
}

/* a lane's partial sums over its vectors: 32 bits hold them while iqm_lane_bound says so */
typedef struct IqmAcc { uint32_t si, sq, sii, sqq, siq, ri, rq; } IqmAcc;

/* the largest value a lane's 32-bit sum can reach over `iters` vectors: 8 bytes of 255 per component and vector, squared */
IQM_HD uint64_t iqm_lane_bound(uint32_t iters) { return (uint64_t)iters * 8u * 255u * 255u; }

/* sum over the four bytes of a[k] b[k]: v_dot4_u32_u8 on the device */
IQM_HD uint32_t iqm_dot4(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4(a, b, c, false);
#else
  for (int k = 0; k < 4; ++k) c += ((a >> (8 * k)) & 255u) * ((b >> (8 * k)) & 255u);
  return c;
#endif
}

/* 0x80 in every byte of w that is 0 or 255, nothing elsewhere (exact: no carry leaves a byte) */
IQM_HD uint32_t iqm_rails(uint32_t w) {
  const uint32_t m = 0x7f7f7f7fu, x = ~w;
  const uint32_t z = ~(((w & m) + m) | w | m);        /* bytes equal to 0 */
  const uint32_t f = ~(((x & m) + m) | x | m);        /* bytes equal to 255 */
  return z | f;
}

/* the dword of a row at odd parity put back at I Q I Q: bytes 1 .. 3 of w and byte 0 of what follows it */
IQM_HD uint32_t iqm_shift(uint32_t w, uint32_t next) { return (w >> 8) | (next << 24); }

/* one dword I Q I Q onto a lane's sums */
IQM_HD void iqm_take(IqmAcc* a, uint32_t w) {
  const uint32_t e = w & 0x00ff00ffu, o = (w >> 8) & 0x00ff00ffu, r = iqm_rails(w);
  a->si = iqm_dot4(w, 0x00010001u, a->si);
  a->sq = iqm_dot4(w, 0x01000100u, a->sq);
  a->sii = iqm_dot4(e, e, a->sii);
  a->sqq = iqm_dot4(o, o, a->sqq);
  a->siq = iqm_dot4(e, o, a->siq);
  a->ri += (uint32_t)__builtin_popcount(r & 0x00800080u);
  a->rq += (uint32_t)__builtin_popcount(r & 0x80008000u);
}

/* one pair onto a lane's sums: the head and the tail */
IQM_HD void iqm_take_pair(IqmAcc* a, uint32_t bi, uint32_t bq) {
  a->si += bi; a->sq += bq;
  a->sii += bi * bi; a->sqq += bq * bq; a->siq += bi * bq;
  a->ri += (uint32_t)((bi == 0u) | (bi == 255u));
  a->rq += (uint32_t)((bq == 0u) | (bq == 255u));
}

#ifdef __HIPCC__

struct IqMeterParams {
  const uint8_t* iq;
  size_t iq_stride;
  uint32_t nbytes, bps, share;
  unsigned long long* meters;      // [n_streams][8], zeroed before the launch
  uint32_t* hist;                  // [n_streams][512], zeroed before the launch; the hist instance only
};

// one dword's four counts into the lane's copy of the bins: bins[bin * IQM_HIST_REPL + copy]
__device__ inline void iqm_count(uint32_t* bins, uint32_t copy, uint32_t w) {
  atomicAdd(&bins[(w & 255u) * IQM_HIST_REPL + copy], 1u);
  atomicAdd(&bins[(256u + ((w >> 8) & 255u)) * IQM_HIST_REPL + copy], 1u);
  atomicAdd(&bins[((w >> 16) & 255u) * IQM_HIST_REPL + copy], 1u);
  atomicAdd(&bins[(256u + (w >> 24)) * IQM_HIST_REPL + copy], 1u);
}

// the body of k_iq_meter<HIST>: bins is the workgroup's 512 x IQM_HIST_REPL counts in LDS (not read where !HIST), red its 8 joined sums
template <bool HIST>
__device__ inline void iq_meter_block(const IqMeterParams& p, uint32_t* bins, unsigned long long* red) {
  const uint32_t tid = threadIdx.x, s = blockIdx.x / p.bps, b = blockIdx.x - s * p.bps;
  const uint8_t* row = p.iq + (size_t)s * p.iq_stride;
  const IqmRow g = iqm_row(reinterpret_cast<uintptr_t>(row), p.nbytes);
  const uint32_t copy = tid & (IQM_HIST_REPL - 1u);
  if (HIST) {
    for (uint32_t k = tid; k < 512u * IQM_HIST_REPL; k += IQM_NT) bins[k] = 0u;
  }
  if (tid < 8u) red[tid] = 0ull;
  __syncthreads();

  IqmAcc a = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
  const uint8_t* body = row + g.head - g.odd;                    // 16-byte aligned; the logical vector k starts g.odd bytes into the aligned vector k
  const uint32_t v0 = b * p.share, v1 = v0 + p.share < g.nvec ? v0 + p.share : g.nvec;   // (bps * share <= 2^22 + 2^19: no wrap)
#pragma unroll 4
  for (uint32_t v = v0 + tid; v < v1; v += IQM_NT) {
    const uint8_t* at = body + (size_t)v * IQM_VEC;
    const uint4 d = *reinterpret_cast<const uint4*>(at);
    uint32_t w0 = d.x, w1 = d.y, w2 = d.z, w3 = d.w;
    if (g.odd) {                                                 // (uniform over the workgroup)
      const uint32_t nx = at[IQM_VEC];
      w0 = iqm_shift(w0, w1); w1 = iqm_shift(w1, w2); w2 = iqm_shift(w2, w3); w3 = iqm_shift(w3, nx);
    }
    iqm_take(&a, w0); iqm_take(&a, w1); iqm_take(&a, w2); iqm_take(&a, w3);
    if (HIST) { iqm_count(bins, copy, w0); iqm_count(bins, copy, w1); iqm_count(bins, copy, w2); iqm_count(bins, copy, w3); }
  }
  if (b == 0u && tid < 15u) {                                    // the head's pairs on lanes 0 .. 7, the tail's on lanes 8 .. 14
    const uint32_t k = tid < 8u ? tid : tid - 8u;
    const bool live = tid < 8u ? 2u * k < g.head : 2u * k < g.tail;
    if (live) {
      const uint8_t* at = row + (tid < 8u ? 0u : g.head + g.nvec * IQM_VEC) + 2u * k;
      const uint32_t bi = at[0], bq = at[1];
      iqm_take_pair(&a, bi, bq);
      if (HIST) { atomicAdd(&bins[bi * IQM_HIST_REPL + copy], 1u); atomicAdd(&bins[(256u + bq) * IQM_HIST_REPL + copy], 1u); }
    }
  }

  // the lanes' sums, widened, joined over the wave in registers, over the workgroup in LDS and over the row by 64-bit integer atomics
  unsigned long long t[7] = {a.si, a.sq, a.sii, a.sqq, a.siq, a.ri, a.rq};
#pragma unroll
  for (int k = 0; k < 7; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t[k] += __shfl_down(t[k], o, 64);
  }
  if ((tid & 63u) == 0u) {
#pragma unroll
    for (int k = 0; k < 7; ++k) atomicAdd(&red[1 + k], t[k]);
  }
  __syncthreads();
  unsigned long long* m = p.meters + 8 * (size_t)s;
  if (tid == 0u && b == 0u) atomicAdd(&m[0], (unsigned long long)(p.nbytes / 2u));
  if (tid >= 1u && tid < 8u && red[tid]) atomicAdd(&m[tid], red[tid]);
  if (HIST) {                                                    // the copies of a bin summed, one global atomic per bin that counted anything
    uint32_t* out = p.hist + (size_t)s * 512u;
    for (uint32_t bin = tid; bin < 512u; bin += IQM_NT) {
      const uint4* c = reinterpret_cast<const uint4*>(bins + bin * IQM_HIST_REPL);
      uint32_t n = 0u;
#pragma unroll
      for (uint32_t q = 0; q < IQM_HIST_REPL / 4u; ++q) { const uint4 x = c[q]; n += x.x + x.y + x.z + x.w; }
      if (n) atomicAdd(&out[bin], n);
    }
  }
}

#endif  /* __HIPCC__ */
#endif  /* SDRFM_IQ_METER_H */
