/* What the FM call path's host arithmetic (csrc/sdrfm_fm_call.h) answers for the calls of tests/fm_exact_cases.py on a bit-exact handle, for
 * tests/test_fm_exact_cases_cpu.py: which bit-exact kernel serves each call and how it cuts a stream, so that the class
 * tests/test_fm_exact_shapes_gpu.py names for a call — generic tile size, design B's segments, the short last one, the folded hand-over, the
 * first call's fix-up — is the one the rules reach on a 256-CU device, checked on a machine without one.
 *
 *   fm_exact_cases T D Ta Da n_streams  call...
 * with one call per argument, "nsamp:cls": samples per stream and the alignment class of iq and iq_stride (16, 4 or 1).  The handle is planned as
 * the library plans a SDRFM_CFG_BIT_EXACT handle of that shape on an MI355X (fm_geom.h); samples seen and both decimators' phases are carried from
 * call to call as enqueue() carries them.  First line, once per handle:
 *   "NA lds supported"                      g.NA, fm_generic_tile(...).lds, lds <= 160 KiB
 * then one line per call:
 *   "N M A phase_x phase_d kind NA tiles fold subtiles short_first fixup_tiles min_subtiles"
 * phase_x / phase_d before the call; kind, NA, tiles (per stream) and fold from fm_bx(g, c, n_streams, g.waves_target, false); subtiles =
 * ceil(M / (64 R)) (0 without a design-B tile); fixup_tiles = fm_fixup(g, c).tiles_per_stream where the fix-up runs (a kernel that reads its halo
 * as bytes, before T - 1 samples were seen), else 0; min_subtiles = where fm_b_tiles' back-off 4 -> 2 -> 1 ends for the call (the same loop, repeated
 * here because fm_b_tiles does not report it; 0 where design B does not serve). */
#include <cstdio>
#include <cstdlib>

#include "fm_geom.h"

int main(int argc, char** argv) {
  if (argc < 6) { fprintf(stderr, "usage: %s T D Ta Da n_streams nsamp:cls...\n", argv[0]); return 2; }
  const uint32_t T = (uint32_t)atol(argv[1]), D = (uint32_t)atol(argv[2]), Ta = (uint32_t)atol(argv[3]), Da = (uint32_t)atol(argv[4]);
  const uint32_t ns = (uint32_t)atol(argv[5]);
  const FmGeom g = fm_test_geom(T, D, Ta, Da, ns, true, fm_test_facts_mi355x(T, D, Da));
  const FmGenericTile gt = fm_generic_tile(T, D, Ta, Da);
  printf("%u %zu %d\n", g.NA, gt.lds, (int)(gt.lds <= 160u * 1024u));

  uint32_t phase_x = 0, phase_d = 0;
  uint64_t n_seen = 0;
  for (int i = 6; i < argc; ++i) {
    unsigned nsamp = 0, cls = 0;
    if (sscanf(argv[i], "%u:%u", &nsamp, &cls) != 2 || (cls != 16 && cls != 4 && cls != 1)) { fprintf(stderr, "bad call %s\n", argv[i]); return 2; }
    const FmCounts n = fm_counts(phase_x, phase_d, 2 * nsamp, g.D, g.Da);
    const FmCall c = {n.N, n.M, n.A, phase_x, phase_d, n_seen, cls >= 4, cls == 16};
    FmBx b = {'-', false, FmTiles{0u, 0u, 0u, 0u}, false};
    if (n.N) b = fm_bx(g, c, ns, g.waves_target, false);         // (enqueue() returns before any launch when a call holds no sample)
    const uint32_t nyt = 64u * g.fast_R;
    const uint32_t sub_total = g.has_fast ? (n.M + nyt - 1) / nyt : 0u;
    uint32_t ms = 0;
    if (b.kind == 'b') { ms = g.min_subtiles; while (ms > 1 && (uint64_t)ns * (sub_total / ms) < g.waves_target / 2) ms >>= 1; }
    const bool fix = n.N && b.halo_bytes && n_seen + 1 < g.T;
    printf("%u %u %u %u %u %c %u %u %u %u %d %u %u\n", n.N, n.M, n.A, phase_x, phase_d, b.kind, b.tiles.NA, b.tiles.tiles_per_stream, b.tiles.fold_state,
           sub_total, (int)fm_short_first(g, c), fix ? fm_fixup(g, c).tiles_per_stream : 0u, ms);
    n_seen += n.N; phase_x = n.phase_x; phase_d = n.phase_d;
  }
  return 0;
}
