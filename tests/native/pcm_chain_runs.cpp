/* The number of runs design Q cuts a stream's call into when the PCM sink's chain rides in its launch, by the host arithmetic enqueue() uses
 * (csrc/sdrfm_fm_call.h), for tests/test_pcm_chain_cpu.py: the test hands the answer to tools/pcm_chain_emulate.py's run_cuts(), which restates the
 * kernel's cut of a stream into those runs.
 *
 *   pcm_chain_runs T D Ta Da n_streams n_cu q_waves_per_cu  nbytes...
 * prints one line per call size: "nbytes M A q_fit chain_fits runs with_chain" (a stream past its first T - 1 samples, phases 0, aligned rows, nothing routed). */
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_fm_call.h"

int main(int argc, char** argv) {
  if (argc < 9) { fprintf(stderr, "usage: %s T D Ta Da n_streams n_cu q_waves_per_cu nbytes...\n", argv[0]); return 2; }
  FmGeom g;
  memset(&g, 0, sizeof(g));
  g.T = (uint32_t)atol(argv[1]); g.D = (uint32_t)atol(argv[2]); g.Ta = (uint32_t)atol(argv[3]); g.Da = (uint32_t)atol(argv[4]);
  g.n_streams = (uint32_t)atol(argv[5]); g.n_cu = (uint32_t)atol(argv[6]); g.q_waves_per_cu = (uint32_t)atol(argv[7]);
  g.has_q = true;
  for (int i = 8; i < argc; ++i) {
    const uint32_t nbytes = (uint32_t)atol(argv[i]);
    const FmCounts n = fm_counts(0, 0, nbytes, g.D, g.Da);
    const FmCall c = {n.N, n.M, n.A, 0, 0, 1u << 20, true, true};
    const bool q_fit = fm_q_fit(g, c), q_ok = fm_q_ok(q_fit, 0, g.n_streams), fits = fm_chain_fits(g, c, q_ok, false, false);
    const FmSplit s = fm_split(g, c, false, false, 0);
    const FmRuns r = fm_q_runs(c, s.q_total, g.n_streams, fits, g.q_waves_per_cu * g.n_cu, fm_chain_run_quads(g.Da));
    printf("%u %u %u %d %d %u %d\n", nbytes, c.M, c.A, (int)q_fit, (int)fits, r.runs, (int)r.with_chain);
  }
  return 0;
}
