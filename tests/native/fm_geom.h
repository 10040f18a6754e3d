/* The FmGeom sdrfm_create arrives at on a 256-CU device (MI355X) for 32 audio taps, shared by the CPU checks of the FM call path
 * (fm_call_check.cpp, fm_shape_cases.cpp), and which shapes the library has an instance of (csrc/sdrfm.hip: kFastVariants and the design-Q rules of
 * sdrfm_create; a comment there points here: keep the two in step). */
#ifndef SDRFM_TESTS_FM_GEOM_H
#define SDRFM_TESTS_FM_GEOM_H

#include <string.h>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_fm_call.h"

// a handle of shape (T, D, Ta, Da) on a 256-CU device, every design instantiated: the values sdrfm_create arrives at for the headline shape
// (tile R = 12 at two waves per SIMD, the R = 4 tile of 6.8 KB beside design Q's waves of 10.9 KB, 12 workgroups of either kind per CU)
static inline FmGeom fm_test_geom(uint32_t T, uint32_t D, uint32_t Ta, uint32_t Da, uint32_t ns) {
  FmGeom g;
  memset(&g, 0, sizeof(g));
  g.T = T; g.D = D; g.Ta = Ta; g.Da = Da; g.n_streams = ns; g.n_cu = 256;
  g.has_q = true; g.has_fast = true; g.fast_is_b = true; g.has_s = (D == 10 && Da == 5 && Ta == 32 && (T == 64 || T == 32)); g.has_mix_tile = true;
  g.mix_lds = 17000; g.q_waves_per_cu = (D == 16) ? 11 : 12; g.q_lds = 11164;
  g.fast_R = (D == 16) ? 8 : 12; g.fast_lds = 19968; g.waves_target = 256 * 8; g.min_subtiles = 4; g.fold_state_ok = 1;
  g.fast_mix_lds = 6960; g.mix_R = 4; g.mix_waves_per_cu = g.q_waves_per_cu; g.mix_cost = 2.7; g.mix_rho = 12.7; g.mix_split_off = false;
  g.seg = 6 * 8 * D; g.NA = 64;
  return g;
}

// design B's instances at 32 audio taps (kFastVariants, kind 'b'), and its R = 4 tile
static inline bool fm_test_has_b(uint32_t T, uint32_t D, uint32_t Da) {
  if (Da == 5) return (D == 10 && (T == 64 || T == 16 || T == 32)) || (D == 16 && T == 64);
  if (Da == 8) return (D == 8 && (T == 64 || T == 16)) || (D == 4 && T == 64);
  return false;
}
static inline bool fm_test_has_b4(uint32_t T, uint32_t D, uint32_t Da) { return fm_test_has_b(T, D, Da) && D != 4; }

// ... with only the designs the library has an instance of for the shape (low-pass taps the guard accepts; bit_exact: SDRFM_CFG_BIT_EXACT)
static inline FmGeom fm_test_geom_instances(uint32_t T, uint32_t D, uint32_t Da, uint32_t ns, bool bit_exact) {
  FmGeom g = fm_test_geom(T, D, 32, Da, ns);
  const bool q_shape = (D == 10 && Da == 5) || (D == 8 && Da == 8) || (D == 16 && Da == 5);   // sdrfm_q_geometry_ok
  g.has_q = !bit_exact && q_shape && T <= 64 && T <= 9 * D;
  g.has_fast = g.fast_is_b = fm_test_has_b(T, D, Da);
  g.has_mix_tile = g.has_q && fm_test_has_b4(T, D, Da);
  if (!g.has_mix_tile) g.mix_lds = 0;
  return g;
}

#endif
