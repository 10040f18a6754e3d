/*
 * sdrfm_fm_tiles.h — the FM handle's tiles as data and arithmetic: which instances of designs S, B and A the library carries, and the LDS
 * sizes that follow from a tile's shape.  Plain C++17 without HIP: the kernels (sdrfm_b.h, sdrfm.hip, sdrfm_q.hip) size their tiles with
 * these functions, sdrfm.hip expands the list into its table of kernel pointers, and sdrfm_fm_plan.h chooses from the same list on a CPU.
 * Internal to the library; the drop-in boundary is include/sdrfm.h.
 */
#ifndef SDRFM_FM_TILES_H
#define SDRFM_FM_TILES_H

#include <stddef.h>
#include <stdint.h>

// ---- design A (float tile): bytes of the x tile: positions [0, HP + NST) in rows of R*D samples, last row trimmed, rounded up to 16 B
constexpr int fast_xbytes(int T, int D, int R) {
  const int RD = R * D, HP = T - D, NST = 64 * RD, RS = (RD + (((RD / 2) % 2 == 0) ? 2 : 0)) * 8;
  const int last = HP + NST - 1;
  return (((last / RD) * RS + (last % RD + 1) * 8) + 15) & ~15;
}

// ---- design B (raw-byte tile)
constexpr int fastb_hp(int T, int D) { return ((T - D) + 7) & ~7; }                      // halo samples (16-B granular)
constexpr int fastb_rs(int D, int R) { return R * D * 2 + ((((R * D * 2) / 16) % 2 == 0) ? 16 : 0); }  // row stride, B
// sub-tiles of d's buffered per audio flush: the small tile (R = 4: 256 d's = 51 audio outputs per sub-tile, which leaves the flush's three chains per lane
// two thirds idle) flushes every third sub-tile
#ifndef SDRFM_B_AB_SMALL
#define SDRFM_B_AB_SMALL 3
#endif
constexpr int fastb_ab(int R) { return R <= 4 ? SDRFM_B_AB_SMALL : 1; }
constexpr int fastb_xbytes(int T, int D, int R) {
  const int RD = R * D, last = fastb_hp(T, D) + 64 * RD - 1;
  return (((last / RD) * fastb_rs(D, R) + (last % RD + 1) * 2) + 15) & ~15;
}

// ---- a workgroup of design A or B: the sample tile, then the d ring (Ta - 1 history words rounded up to 4, AB sub-tiles of 64 R d's), the taps
constexpr size_t fast_tile_lds(size_t xbytes, uint32_t AB, uint32_t R, uint32_t T, uint32_t Ta) {
  return xbytes + (size_t)(((Ta - 1 + 3u) & ~3u) + AB * 64u * R + T + Ta) * 4;
}
constexpr size_t fastb_lds(int T, int D, int R, int Ta) {
  return fast_tile_lds((size_t)fastb_xbytes(T, D, R), (uint32_t)fastb_ab(R), (uint32_t)R, (uint32_t)T, (uint32_t)Ta);
}

// ---- the generic kernel's tile: as many audio outputs per block as fit ~48 KiB of LDS, capped at 64
struct FmGenericTile { uint32_t NA; size_t lds; };
constexpr FmGenericTile fm_generic_tile(uint32_t T, uint32_t D, uint32_t Ta, uint32_t Da) {
  uint32_t NA = 64;
  for (;;) {
    const size_t ND = (size_t)(NA - 1) * Da + Ta, NY = ND + 1, NX = (NY - 1) * D + T;
    const size_t lds = NX * 8 + NY * 8 + ND * 4 + T * 4 + Ta * 4;
    if (lds <= 48 * 1024 || NA == 1) return FmGenericTile{NA, lds};
    NA /= 2;
  }
}

// ---- the instances: X(kind, T, D, R, NB, Ta, Da, modes) ------------------------------------------------------------------------------------
// kind   s = streaming lanes (design S), b = raw-byte tile (design B), a = float tile (design A)
// R      outputs per lane and sub-tile (A, B) / accumulator slots (S);  NB: design S's blocks per lane segment (0 otherwise)
// Ta, Da compile-time audio geometry (0 = any: design A)
// modes  bit m: kernel mode m is instantiated in the development library — 0 the product's, 1 the phase profile, 2 .. 7 timing ablations with wrong
//        results (SDRFM_ABLATE; design B, headline shape only: [2] halo samples not converted, [3] no sample converted, [4] no discriminator, [5] no
//        conversion, no FIR, no discriminator: staging, LDS window reads and audio stage remain).  The product library instantiates mode 0 alone.
#ifdef SDRFM_DEV
#define SDRFM_FM_MODES(m) (m)
// design A: kept as the measured alternative; ablation modes only on the documented shape
#define SDRFM_FM_INSTANCES_DEV(X) X(a, 64, 10, 3, 0, 0, 0, 0xffu) X(a, 16, 10, 2, 0, 0, 0, 0x03u) X(a, 32, 10, 2, 0, 0, 0, 0x03u)
#else
#define SDRFM_FM_MODES(m) 0x01u
#define SDRFM_FM_INSTANCES_DEV(X)
#endif
#define SDRFM_FM_INSTANCES(X)                                                                                                              \
  /* design S: the BASELINE configs[2]/[3] shape; serves calls that are whole numbers of lane segments                                     \
     (a 16-tap instance is correct too but no faster than design B on cold inputs: 35.2 vs 34.1 us; it is not instantiated) */             \
  X(s, 64, 10, 8, 6, 32, 5, 0x01u) X(s, 32, 10, 8, 6, 32, 5, 0x01u)                                                                        \
  /* 2.4 MS/s -> 240 kS/s -> 48 kHz: the rate the firmware programs (usbh_rtlsdr.c:898) and the BASELINE configs */                        \
  X(b, 64, 10, 12, 0, 32, 5, 0x3fu) X(b, 64, 10, 8, 0, 32, 5, 0x01u) X(b, 16, 10, 12, 0, 32, 5, 0x03u) X(b, 32, 10, 12, 0, 32, 5, 0x01u)   \
  /* R = 4: the noisy streams' workgroups beside design Q's (per-stream routing; inside design Q's launch: k_mix): 8.8 KB of LDS per wave  \
     — a slot one of design Q's waves (10.9 KB) leaves takes one, which the 19 KB of the R = 12 instance cannot count on while design Q's  \
     waves keep coming */                                                                                                                   \
  X(b, 64, 10, 4, 0, 32, 5, 0x01u) X(b, 32, 10, 4, 0, 32, 5, 0x01u) X(b, 16, 10, 4, 0, 32, 5, 0x01u)                                       \
  /* the other rates RTLSDR_set_sample_rate accepts and a dongle is commonly run at:                                                        \
     2.048 MS/s -> 256 kS/s -> 32 kHz, 1.024 MS/s -> 256 kS/s -> 32 kHz, 3.2 MS/s -> 200 kS/s -> 40 kHz */                                 \
  X(b, 64, 8, 12, 0, 32, 8, 0x01u) X(b, 16, 8, 12, 0, 32, 8, 0x01u) X(b, 64, 4, 12, 0, 32, 8, 0x01u) X(b, 64, 16, 8, 0, 32, 5, 0x01u)      \
  X(b, 64, 8, 4, 0, 32, 8, 0x01u) X(b, 16, 8, 4, 0, 32, 8, 0x01u) X(b, 64, 16, 4, 0, 32, 5, 0x01u)                                         \
  SDRFM_FM_INSTANCES_DEV(X)

struct FmInstance {
  char kind;                         // 's', 'b' or 'a'
  uint32_t T, D, R;
  uint32_t Ta, Da;
  uint32_t modes;                    // kernel modes this library instantiates (bit 0 always)
  uint32_t xbytes;                   // LDS bytes of the sample tile (A, B) / of the whole ring (S)
  uint32_t seg;                      // design S: samples per lane segment (0 otherwise)
};
constexpr FmInstance fm_instance(char kind, int T, int D, int R, int NB, int Ta, int Da, uint32_t modes) {
  return FmInstance{kind, (uint32_t)T, (uint32_t)D, (uint32_t)R, (uint32_t)Ta, (uint32_t)Da, modes,
                    kind == 's' ? 2u * 64u * 128u : (uint32_t)(kind == 'b' ? fastb_xbytes(T, D, R) : fast_xbytes(T, D, R)),
                    kind == 's' ? (uint32_t)(NB * R * D) : 0u};
}
#define SDRFM_FM_SHAPE(kind, T_, D_, R_, NB_, TA_, DA_, M_) fm_instance(#kind[0], T_, D_, R_, NB_, TA_, DA_, SDRFM_FM_MODES(M_)),
constexpr FmInstance kFmInstances[] = {SDRFM_FM_INSTANCES(SDRFM_FM_SHAPE)};
constexpr int kFmInstanceCount = (int)(sizeof(kFmInstances) / sizeof(kFmInstances[0]));

#endif
