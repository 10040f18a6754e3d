/* One create-time plan of the FM handle (csrc/sdrfm_fm_plan.h: fm_plan) on a CPU, for tests/test_fm_plan_cpu.py, which compares it field for field with
 * what the library printed on an MI355X before this function existed (tests/golden/fm_plan_mi355x.json).
 *
 *   fm_plan_case T D Ta Da n_streams flags refuse_q n_cu:q_nslot:q_lds:mix_lds:mix_blocks taps.f32
 * flags as sdrfm_config has them; refuse_q = 1 plans as sdrfm_create does after design Q's allocations failed; the facts are the recorded answers of
 * the runtime and of design Q's translation unit, or "mi355x" for fm_geom.h's own table of them (which this holds to the record); taps.f32 holds the
 * T channel taps and the Ta audio taps as raw floats.  The verdicts on the taps are computed here, from the same taps and by the library's own routines (fm_tap_verdict, qtaps.c: sdrfm_q_build).  Prints the plan as one
 * JSON object in the record's layout.  Built with qtaps.c.
 * Before anything else the knobs' defaults are held to the values the product library is built with, written out here. */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "fm_geom.h"

static void print_instance(const char* name, int i) {
  if (i < 0) { printf(", \"%s\": null", name); return; }
  const FmInstance& v = kFmInstances[i];
  printf(", \"%s\": {\"kind\": \"%c\", \"T\": %u, \"D\": %u, \"R\": %u, \"Ta\": %u, \"Da\": %u}", name, v.kind, v.T, v.D, v.R, v.Ta, v.Da);
}

int main(int argc, char** argv) {
  const FmKnobs k;
  if (!(k.fast_kind == 'b' && k.fast_r == 12 && k.audio_batch == 0 && k.prio_balance == 1 && k.end_prio == 320 && k.fold_state_ok == 1 && !k.no_stream &&
        !k.stream_profile && k.q_nslot == 0 && k.q_waves_per_cu == 0 && k.q_guard_r < 0 && k.q_guard_a < 0 && !k.no_q && !k.q_no_adapt && k.warm_ahead == 0 &&
        k.ablate == 0 && !k.phase_profile && k.waves_per_cu == 0 && k.min_subtiles == 4 && k.mix_cost == 2.7 && k.mix_rho == 12.7 && !k.mix_split_off &&
        !k.mix_off && k.mix_waves_per_cu == 0)) { fprintf(stderr, "FmKnobs' defaults are not the product's\n"); return 1; }
  FmTestFacts f;
  const bool table = argc == 10 && !strcmp(argv[8], "mi355x");
  if (argc != 10 || (!table && !fm_test_parse_facts(argv[8], &f))) { fprintf(stderr, "usage: %s T D Ta Da n_streams flags refuse_q facts taps.f32\n", argv[0]); return 2; }
  const uint32_t T = (uint32_t)atol(argv[1]), D = (uint32_t)atol(argv[2]), Ta = (uint32_t)atol(argv[3]), Da = (uint32_t)atol(argv[4]);
  const uint32_t flags = (uint32_t)atol(argv[6]);
  if (table) f = fm_test_facts_mi355x(T, D, Da);
  std::vector<float> taps(T + Ta);
  FILE* tf = fopen(argv[9], "rb");
  if (!tf || fread(taps.data(), sizeof(float), T + Ta, tf) != T + Ta) { fprintf(stderr, "cannot read %u + %u taps from %s\n", T, Ta, argv[9]); return 2; }
  fclose(tf);
  const float *h = taps.data(), *g = h + T;

  // sdrfm_create's order: the verdicts (flags: SDRFM_CFG_FORCE_GENERIC 1, SDRFM_CFG_BIT_EXACT 4, SDRFM_CFG_GUARD_WORST_CASE 8), the tables where design Q is offered
  FmPlanIn in = fm_test_plan_in(T, D, Ta, Da, (uint32_t)atol(argv[5]), (flags & 4u) != 0, f);
  in.force_generic = (flags & 1u) != 0;
  in.taps = FmTapVerdict{false, false, 0.0f, 0.0f};
  if (!in.force_generic) in.taps = fm_tap_verdict(h, T, g, Ta, (flags & 8u) != 0);
  in.q_built = false; in.q_c0 = 0;
  char symbol[48] = "";
  if (fm_plan_offers_q(in, k)) {
    std::vector<int8_t> tab((size_t)SDRFM_Q_SPARSE_CHUNKS(D) * SDRFM_Q_DIGITS * 64 * 16);
    float qs = 0.f, qc = 0.f;
    in.q_built = sdrfm_q_build(h, T, D, tab.data(), &qs, &qc, &in.q_c0) == 0;
    // (the kernel's name as sdrfm_q.hip's table spells it: the rate's parameters are left out at the BASELINE rate)
    const unsigned c0 = in.q_c0 > 1 ? 1 : in.q_c0, ns = fm_plan_q_nslot(in, k);
    if (D == 10 && Da == 5) snprintf(symbol, sizeof(symbol), "k_mfir<%u,%u>", c0, ns);
    else snprintf(symbol, sizeof(symbol), "k_mfir<%u,%u,%u,%u>", c0, ns, D, Da);
    in.q_symbol = symbol;
  }
  const FmPlan p = fm_plan(in, k, FmRefused{atol(argv[7]) != 0, 0u});
  if (!p.supported) { printf("{\"supported\": false}\n"); return 0; }
  const FmGeom& G = p.geo;
  printf("{\"geo\": {\"T\": %u, \"D\": %u, \"Ta\": %u, \"Da\": %u, \"n_streams\": %u, \"n_cu\": %u, \"has_q\": %d, \"has_fast\": %d, \"fast_is_b\": %d, \"has_s\": %d, "
         "\"has_mix_tile\": %d, \"mix_lds\": %u, \"q_waves_per_cu\": %u, \"q_lds\": %zu, \"fast_R\": %u, \"fast_lds\": %zu, \"waves_target\": %u, \"min_subtiles\": %u, "
         "\"fold_state_ok\": %u, \"fast_mix_lds\": %zu, \"mix_R\": %u, \"mix_waves_per_cu\": %u, \"mix_cost\": %.17g, \"mix_rho\": %.17g, \"mix_split_off\": %d, "
         "\"seg\": %u, \"NA\": %u}",
         G.T, G.D, G.Ta, G.Da, G.n_streams, G.n_cu, (int)G.has_q, (int)G.has_fast, (int)G.fast_is_b, (int)G.has_s, (int)G.has_mix_tile, G.mix_lds, G.q_waves_per_cu,
         G.q_lds, G.fast_R, G.fast_lds, G.waves_target, G.min_subtiles, G.fold_state_ok, G.fast_mix_lds, G.mix_R, G.mix_waves_per_cu, G.mix_cost, G.mix_rho,
         (int)G.mix_split_off, G.seg, G.NA);
  print_instance("fast", p.fast);
  print_instance("fast_s", p.fast_s);
  print_instance("fast_mix", p.fast_mix);
  printf(", \"AB\": %u, \"warm_ahead\": %u, \"fast_mode\": %d, \"lds_bytes\": %zu, \"q_nslot\": %u, \"q_c0\": %u, \"q_guard_r\": %.9g, \"q_guard_a\": %.9g", p.AB, p.warm_ahead,
         p.fast_mode, p.lds_bytes, p.q_nslot, p.q_c0, (double)p.q_guard_r, (double)p.q_guard_a);
  printf(", \"names\": {\"generic\": \"%s\", \"fast\": \"%s\", \"fast_s\": \"%s\", \"fast_q\": \"%s\", \"kernel\": \"%s\"}}\n", p.generic_name, p.fast_name, p.fast_s_name,
         p.fast_q_name, p.kernel_name);
  return 0;
}
