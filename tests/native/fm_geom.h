/* The FmGeom of a handle as the library plans it (csrc/sdrfm_fm_plan.h: fm_plan), for the CPU checks of the FM call path (fm_call_check.cpp,
 * fm_shape_cases.cpp, fm_plan_case.cpp).  What only a device and design Q's translation unit can say — compute units, design Q's ring and LDS bytes,
 * the one-launch kernel's LDS bytes and occupancy — is what an MI355X answered (fm_test_facts_mi355x), or comes in on a command line as
 * "n_cu:q_nslot:q_lds:mix_lds:mix_blocks_per_cu". */
#ifndef SDRFM_TESTS_FM_GEOM_H
#define SDRFM_TESTS_FM_GEOM_H

#include <stdio.h>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_fm_plan.h"

struct FmTestFacts { unsigned n_cu, q_default_nslot, q_default_lds, mix_lds; int mix_blocks_per_cu; };
static inline bool fm_test_parse_facts(const char* s, FmTestFacts* f) {
  return sscanf(s, "%u:%u:%u:%u:%d", &f->n_cu, &f->q_default_nslot, &f->q_default_lds, &f->mix_lds, &f->mix_blocks_per_cu) == 5;
}

// The answers tests/golden/fm_plan_mi355x.json records under "runtime" (tests/test_fm_plan_cpu.py plans every recorded default handle with these and
// must arrive at the record): 256 CUs; design Q's ring and a wave's LDS bytes by rate; the one-launch kernel, which exists where design B has an
// R = 4 tile, takes the larger of the two workgroups' LDS (design Q's everywhere) and the occupancy the runtime reports for it.
static inline FmTestFacts fm_test_facts_mi355x(uint32_t T, uint32_t D, uint32_t Da) {
  FmTestFacts f = {256u, 0u, 0u, 0u, 0};
  if (D == 10 && Da == 5) { f.q_default_nslot = 5; f.q_default_lds = 10864; if (T == 64 || T == 32 || T == 16) f.mix_blocks_per_cu = 15; }
  if (D == 8 && Da == 8) { f.q_default_nslot = 4; f.q_default_lds = 11344; if (T == 64 || T == 16) f.mix_blocks_per_cu = T == 64 ? 12 : 14; }
  if (D == 16 && Da == 5) { f.q_default_nslot = 8; f.q_default_lds = 14032; if (T == 64) f.mix_blocks_per_cu = 11; }
  if (f.mix_blocks_per_cu) f.mix_lds = f.q_default_lds;
  return f;
}

// a handle of shape (T, D, Ta, Da): low-pass taps the guard accepts, whose tables build with a tap in the first chunk
static inline FmPlanIn fm_test_plan_in(uint32_t T, uint32_t D, uint32_t Ta, uint32_t Da, uint32_t ns, bool bit_exact, const FmTestFacts& f) {
  FmPlanIn in;
  memset(&in, 0, sizeof(in));
  in.T = T; in.D = D; in.Ta = Ta; in.Da = Da; in.n_streams = ns; in.bit_exact = bit_exact; in.n_cu = f.n_cu;
  in.taps = FmTapVerdict{true, true, 4.7f, 3.14f};
  in.q_built = true; in.q_c0 = 0;
  in.q_default_nslot = f.q_default_nslot; in.q_default_lds = in.q_lds = f.q_default_lds; in.q_symbol = "";
  in.mix_lds = f.mix_lds; in.mix_blocks_per_cu = f.mix_blocks_per_cu;
  return in;
}
static inline FmGeom fm_test_geom(uint32_t T, uint32_t D, uint32_t Ta, uint32_t Da, uint32_t ns, bool bit_exact, const FmTestFacts& f) {
  return fm_plan(fm_test_plan_in(T, D, Ta, Da, ns, bit_exact, f), FmKnobs(), FmRefused{false, 0u}).geo;
}

#endif
