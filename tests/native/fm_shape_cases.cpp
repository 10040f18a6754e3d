/* What the FM call path's host arithmetic (csrc/sdrfm_fm_call.h, csrc/sdrfm_fm_carry.h) answers for a sequence of calls on one handle, for
 * tests/test_fm_shapes_cpu.py: every case of tests/fm_shape_cases.py goes through here, so that the design tests/test_fm_shapes_gpu.py names for a call is the
 * one the eligibility rules reach on a 256-CU device — checked on a machine without one.
 *
 *   fm_shape_cases T D Da n_streams bit_exact n_routed route_at  call...
 * with one call per argument, "nsamp:cls:overlap:device": samples per stream, the alignment class of iq and iq_stride (16, 4 or 1), SDRFM_F_OVERLAP
 * set or not, device pointers or host buffers (the staging rows: 256-byte aligned).  n_routed streams are routed to the bit-exact kernels from call
 * route_at on.  The handle's state is an FmCarry taken through the header's functions in enqueue()'s order (three input buffers and two audio buffers in
 * turn: rows that share no bytes).  One line per call:
 *   "nsamp M A q_fit q_ok stream_ok fast_ok prev_dev prev_q ovl_geometry_ok overlapped fuse"
 * stream_ok as launch_bx asks it (every stream, not beside design Q); ovl_geometry_ok is fm_ovl_geometry_ok on the previous call's bytes and alignment
 * whatever served it; overlapped = fm_carry_overlap says yes.  The FmGeom is the one the library
 * plans for the shape at 32 audio taps on an MI355X (fm_geom.h: fm_plan with low-pass taps the guard accepts). */
#include <cstdio>
#include <cstdlib>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_fm_carry.h"
#include "fm_geom.h"

int main(int argc, char** argv) {
  if (argc < 9) { fprintf(stderr, "usage: %s T D Da n_streams bit_exact n_routed route_at nsamp:cls:overlap:device...\n", argv[0]); return 2; }
  const uint32_t T = (uint32_t)atol(argv[1]), D = (uint32_t)atol(argv[2]), Da = (uint32_t)atol(argv[3]);
  const FmGeom g = fm_test_geom(T, D, 32u, Da, (uint32_t)atol(argv[4]), atol(argv[5]) != 0, fm_test_facts_mi355x(T, D, Da));
  const uint32_t n_routed = (uint32_t)atol(argv[6]);
  const int route_at = (int)atol(argv[7]);

  FmCarry cy = {};
  fm_carry_reset(cy);
  uint32_t last_nbytes = 0;                                      // the previous call's rows, whatever served it and wherever they lay
  bool last_al16 = false;
  for (int i = 8; i < argc; ++i) {
    unsigned nsamp = 0, cls = 0, overlap = 0, device = 0;
    if (sscanf(argv[i], "%u:%u:%u:%u", &nsamp, &cls, &overlap, &device) != 4 || (cls != 16 && cls != 4 && cls != 1)) { fprintf(stderr, "bad call %s\n", argv[i]); return 2; }
    if (!device) cls = 16;
    const uint32_t nbytes = 2 * nsamp;
    const size_t stride = (nbytes + 255u) / 256u * 256u + (cls == 16 ? 0u : cls);
    const FmRows rows = {reinterpret_cast<const uint8_t*>(((uintptr_t)(i % 3) + 1) << 28) + (cls == 16 ? 0u : cls), stride, nbytes,
                         reinterpret_cast<const float*>(((uintptr_t)(i % 2) + 5) << 28), stride, nullptr, 0};
    const FmCounts n = fm_carry_counts(cy, nbytes, g.D, g.Da);
    const FmCall c = fm_carry_call(cy, n, rows.iq, rows.iq_stride);
    const bool q_fit = fm_q_fit(g, c);
    if (n_routed && i - 8 == route_at && g.has_q) fm_carry_assigned(cy);   // the test hook right before the call: route_apply
    const uint32_t n_noisy = (q_fit && i - 8 >= route_at) ? n_routed : 0u;
    const FmServe sv = fm_serve(g, c, n_noisy);
    const bool geo_ok = fm_ovl_geometry_ok(g, c, last_nbytes, last_al16);
    const bool prev_dev = cy.prev_iq != nullptr, prev_q = cy.prev_by_q;
    const bool ovl = fm_carry_overlap(cy, g, c, rows, sv.q_ok, overlap && device, false, false, g.n_streams) == FM_OVL_YES;
    printf("%u %u %u %d %d %d %d %d %d %d %d %d\n", nsamp, c.M, c.A, (int)q_fit, (int)sv.q_ok, (int)fm_stream_ok(g, c, g.n_streams, false), (int)fm_fast_ok(g, c),
           (int)prev_dev, (int)prev_q, (int)geo_ok, (int)ovl, (int)sv.fuse);
    if (!ovl) { const FmJoin j = fm_carry_join(cy, FM_JOIN_ALL); for (uint32_t k = 0; k < 2; ++k) if (j.wait[k]) fm_carry_joined(cy, FM_JOIN_ALL, k); }
    if (sv.bx_all) fm_carry_to_bx(cy);
    const FmSlot slot = fm_carry_slot(cy, ovl, false);
    if (sv.q_ok) fm_carry_q_launched(cy, ovl, slot.k, fm_carry_q_pre(cy, ovl, g.T).carry, rows, c.A, false, false);
    fm_carry_advance(cy, n, rows, device != 0);
    last_nbytes = nbytes; last_al16 = cls == 16;
  }
  return 0;
}
