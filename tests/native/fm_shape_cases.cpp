/* What the FM call path's host arithmetic (csrc/sdrfm_fm_call.h) answers for a sequence of calls on one handle, for tests/test_fm_shapes_cpu.py:
 * every case of tests/fm_shape_cases.py goes through here, so that the design tests/test_fm_shapes_gpu.py names for a call is the one the
 * eligibility rules reach on a 256-CU device — checked on a machine without one.
 *
 *   fm_shape_cases T D Da n_streams bit_exact n_routed route_at  call...
 * with one call per argument, "nsamp:cls:overlap:device": samples per stream, the alignment class of iq and iq_stride (16, 4 or 1), SDRFM_F_OVERLAP
 * set or not, device pointers or host buffers (the staging rows: 256-byte aligned).  n_routed streams are routed to the bit-exact kernels from call
 * route_at on.  The handle's state (samples seen, the decimators' phases, the previous call's buffer, whether design Q served the previous call:
 * enqueue()'s prev_by_q) is carried from call to call as enqueue() carries it.  One line per call:
 *   "nsamp M A q_fit q_ok stream_ok fast_ok prev_dev prev_q ovl_geometry_ok overlapped fuse"
 * stream_ok as launch_bx asks it (every stream, not beside design Q); ovl_geometry_ok is fm_ovl_geometry_ok on the previous call's bytes and alignment
 * whatever served it; overlapped = q_ok && the flag && prev_dev && prev_q && ovl_geometry_ok (buffers that share no rows).  The FmGeom is the one the library
 * plans for the shape at 32 audio taps on an MI355X (fm_geom.h: fm_plan with low-pass taps the guard accepts). */
#include <cstdio>
#include <cstdlib>

#include "fm_geom.h"

int main(int argc, char** argv) {
  if (argc < 9) { fprintf(stderr, "usage: %s T D Da n_streams bit_exact n_routed route_at nsamp:cls:overlap:device...\n", argv[0]); return 2; }
  const uint32_t T = (uint32_t)atol(argv[1]), D = (uint32_t)atol(argv[2]), Da = (uint32_t)atol(argv[3]);
  const FmGeom g = fm_test_geom(T, D, 32u, Da, (uint32_t)atol(argv[4]), atol(argv[5]) != 0, fm_test_facts_mi355x(T, D, Da));
  const uint32_t n_routed = (uint32_t)atol(argv[6]);
  const int route_at = (int)atol(argv[7]);

  uint32_t phase_x = 0, phase_d = 0, prev_nbytes = 0;
  uint64_t n_seen = 0;
  bool prev_dev = false, prev_al16 = false, prev_q = false;
  for (int i = 8; i < argc; ++i) {
    unsigned nsamp = 0, cls = 0, overlap = 0, device = 0;
    if (sscanf(argv[i], "%u:%u:%u:%u", &nsamp, &cls, &overlap, &device) != 4 || (cls != 16 && cls != 4 && cls != 1)) { fprintf(stderr, "bad call %s\n", argv[i]); return 2; }
    if (!device) cls = 16;
    const uint32_t nbytes = 2 * nsamp;
    const FmCounts n = fm_counts(phase_x, phase_d, nbytes, g.D, g.Da);
    const FmCall c = {n.N, n.M, n.A, phase_x, phase_d, n_seen, cls >= 4, cls == 16};
    const bool q_fit = fm_q_fit(g, c);
    const uint32_t n_noisy = (q_fit && i - 8 >= route_at) ? n_routed : 0u;
    const bool q_ok = fm_q_ok(q_fit, n_noisy, g.n_streams), mixed = q_ok && n_noisy > 0;
    const bool geo_ok = fm_ovl_geometry_ok(g, c, prev_nbytes, prev_al16);
    const bool ovl = q_ok && overlap && device && prev_dev && prev_q && geo_ok;
    printf("%u %u %u %d %d %d %d %d %d %d %d %d\n", nsamp, c.M, c.A, (int)q_fit, (int)q_ok, (int)fm_stream_ok(g, c, g.n_streams, false), (int)fm_fast_ok(g, c),
           (int)prev_dev, (int)prev_q, (int)geo_ok, (int)ovl, (int)fm_fuse(g, c, mixed));
    n_seen += n.N; phase_x = n.phase_x; phase_d = n.phase_d;
    prev_dev = device != 0; prev_nbytes = nbytes; prev_al16 = cls == 16; prev_q = q_ok;
  }
  return 0;
}
