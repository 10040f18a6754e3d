/*
 * sdrfm_fm_carry.h — what the FM handle carries from one call to the next, and its overlap joins: the host's bookkeeping, without HIP.
 *
 * Whether a call may overlap the previous one, which state the next kernel is handed and what a join records and waits for are decided by some twenty
 * values that every call reads and rewrites: where the streams stand, what the current state set holds, the previous call's device rows, the rows the
 * latest overlapped call may still be writing, and which of the two internal streams hold calls no join has covered.  They live here as one POD in the
 * manner of sdrfm_fm_route.h: plain C++17, values and small PODs in and out.  A function says what the caller has to do — run sdrfm_q_fix_yprev, refill
 * hist_q, record an event, wait for it — and never does it: sdrfm.hip keeps the buffers, events and streams and the order of its HIP calls, and calls each
 * function at the point its HIP calls have reached, so that a call that fails half-way leaves the carry at that point.  tests/native/fm_carry_check.cpp
 * (tests/test_fm_carry_cpu.py) drives the same functions on a CPU; so do fm_shape_cases.cpp and fm_route_check.cpp.
 * Internal to the library; the drop-in boundary is include/sdrfm.h.
 *
 * The three validity flags ("What a call leaves for the next", has the table of who sets and who reads them):
 *   yprev_exact   y[-1] of the current state set is the definition's (a reset, a bit-exact kernel or sdrfm_q_fix_yprev wrote it), not design Q's own value
 *   hist_q_valid  hist_q of the current state set holds the last raw samples: design Q left them, or an assignment refilled them from hist_b
 *   prev_by_q     design Q served (some streams of) the previous call: the state it left is what an overlapped call's warm-up reproduces.  NOT hist_q_valid:
 *                 an assignment sets that one behind a bit-exact call too, and leaves this one alone
 */
#ifndef SDRFM_FM_CARRY_H
#define SDRFM_FM_CARRY_H

#include "sdrfm_fm_call.h"

struct FmCarry {
  // where the streams stand
  uint64_t n_seen;                   // IQ samples consumed since reset (history is all-real once >= T-1)
  int cur;                           // index of the state set holding the current state
  uint32_t phase_x, phase_d;
  // what the current state set holds (above)
  bool yprev_exact, hist_q_valid, prev_by_q;
  // the previous call's device buffer (valid after a SDRFM_F_DEVICE_PTRS call): what an overlapped call warms its streams up from
  const uint8_t* prev_iq; size_t prev_stride; uint32_t prev_nbytes;
  // the audio and PCM rows the most recent overlapped call writes (it may still be running when the next call is made)
  const float* prev_ovl_audio; size_t prev_ovl_audio_stride; uint32_t prev_ovl_audio_n;
  const int16_t* prev_ovl_pcm; size_t prev_ovl_pcm_stride;
  // the two internal streams: pending: stream k holds overlapped calls no join has covered; bound: its latest kernel carries ovl_done[k] as its stop event
  // (or sdrfm_wait_previous recorded it behind that kernel); join_style: the caller joins after every call; next: the stream the next overlapped call takes
  bool ovl_pending[2], ovl_bound[2], ovl_join_style;
  uint32_t ovl_next;
};

// The rows of one call; audio null: none given, pcm null: no sink's chain to ride.
struct FmRows {
  const uint8_t* iq; size_t iq_stride; uint32_t nbytes;
  const float* audio; size_t audio_stride;
  const int16_t* pcm; size_t pcm_stride;
};

// sdrfm_reset, behind its join of everything: the streams start again.  KEPT AS IT IS: ovl_next, ovl_join_style, ovl_bound and the prev_ovl_* rows survive a
// reset (the internal streams, their events and the caller's way of joining are the handle's, not the streams'; the rows are only read behind a design-Q call).
static inline void fm_carry_reset(FmCarry& c) {
  c.prev_iq = nullptr;
  c.yprev_exact = true;                                           // y[-1] = 0, as the definition has it
  c.hist_q_valid = false; c.prev_by_q = false;
  c.cur = 0; c.phase_x = c.phase_d = 0; c.n_seen = 0;
}

// ---- the call ----------------------------------------------------------------------------------------------------------------------------------------
static inline FmCounts fm_carry_counts(const FmCarry& c, uint32_t nbytes, uint32_t D, uint32_t Da) { return fm_counts(c.phase_x, c.phase_d, nbytes, D, Da); }
static inline bool fm_al(const uint8_t* p, size_t stride, unsigned a) { return ((uintptr_t)p % a == 0) && (stride % a == 0); }
static inline FmCall fm_carry_call(const FmCarry& c, const FmCounts& n, const uint8_t* iq, size_t iq_stride) {
  return FmCall{n.N, n.M, n.A, c.phase_x, c.phase_d, c.n_seen, fm_al(iq, iq_stride, 4), fm_al(iq, iq_stride, 16)};
}
static inline int fm_carry_set(const FmCarry& c) { return c.cur; }   // the state set the call reads; it writes the other one

// SDRFM_F_OVERLAP: may the call run beside the previous one?  FM_OVL_YES, or the first term that refuses it.  q_ok, flag: design Q serves (some of) the call,
// and the caller asked; with_chain: the sink's chain rides in the launch; pcm_no_audio: such a call stores no audio.
// What the flag asks of the caller is checked where that is cheap: a call whose rows overlap the previous call's rows or whose audio buffer is the one the
// previous overlapped call may still be writing runs as if the flag were absent.  So does a call right behind one design Q did not serve (prev_by_q; NOT
// hist_q_valid, which an assignment also sets when it refills hist_q from the bit-exact kernels' samples): the warm-up would recompute y[-1] and the last
// Ta - 1 discriminator outputs with design Q's arithmetic where the same call without the flag takes over the definition's from the bit-exact kernels' state —
// the first audio outputs then differ in their last bits, and the flag promises the same audio bit for bit (tests/test_fm_shapes_gpu.py: "prev-served-by-b",
// "prev-served-by-b-then-routed").
enum FmOvl : uint8_t {
  FM_OVL_YES,
  FM_OVL_NOT_ASKED,      // not design Q's call, or no flag
  FM_OVL_NO_PREV_BUFFER, // the previous call came through host buffers (or there was none since the reset)
  FM_OVL_PREV_NOT_Q,     // the bit-exact kernels served the previous call: the warm-up would recompute their hand-over with design Q's arithmetic (last-bit differences)
  FM_OVL_GEOMETRY,       // fm_ovl_geometry_ok
  FM_OVL_IQ_ROWS,        // the call's rows share bytes with the previous call's (one buffer used for every call)
  FM_OVL_AUDIO_ROWS,     // its audio rows are the ones the previous overlapped call may still be writing — unless the call writes no audio
  FM_OVL_PCM_ROWS        // the same for the PCM rows, when the chain rides
};
static inline FmOvl fm_carry_overlap(const FmCarry& c, const FmGeom& g, const FmCall& cl, const FmRows& r, bool q_ok, bool flag, bool with_chain,
                                     bool pcm_no_audio, uint32_t n_streams) {
  const uint8_t* const audio = reinterpret_cast<const uint8_t*>(r.audio);
  const uint8_t* const pcm = reinterpret_cast<const uint8_t*>(r.pcm);
  if (!q_ok || !flag) return FM_OVL_NOT_ASKED;
  if (!c.prev_iq) return FM_OVL_NO_PREV_BUFFER;
  if (!c.prev_by_q) return FM_OVL_PREV_NOT_Q;
  if (!fm_ovl_geometry_ok(g, cl, c.prev_nbytes, fm_al(c.prev_iq, c.prev_stride, 16))) return FM_OVL_GEOMETRY;
  if (fm_rows_overlap(c.prev_iq, c.prev_stride, c.prev_nbytes, r.iq, r.iq_stride, r.nbytes, n_streams)) return FM_OVL_IQ_ROWS;
  if (!(with_chain && pcm_no_audio) && c.prev_ovl_audio &&
      fm_rows_overlap(reinterpret_cast<const uint8_t*>(c.prev_ovl_audio), c.prev_ovl_audio_stride * sizeof(float), c.prev_ovl_audio_n * sizeof(float), audio,
                      r.audio_stride * sizeof(float), (size_t)cl.A * sizeof(float), n_streams))
    return FM_OVL_AUDIO_ROWS;
  if (with_chain && c.prev_ovl_pcm &&
      fm_rows_overlap(reinterpret_cast<const uint8_t*>(c.prev_ovl_pcm), c.prev_ovl_pcm_stride * sizeof(int16_t), c.prev_ovl_audio_n * 2 * sizeof(int16_t), pcm,
                      r.pcm_stride * sizeof(int16_t), (size_t)cl.A * 2 * sizeof(int16_t), n_streams))
    return FM_OVL_PCM_ROWS;
  return FM_OVL_YES;
}
// what an overlapped call's kernels warm up from (nothing otherwise)
struct FmPrev { const uint8_t* iq; size_t stride; uint32_t N; };
static inline FmPrev fm_carry_prev(const FmCarry& c, bool ovl) { return ovl ? FmPrev{c.prev_iq, c.prev_stride, c.prev_nbytes / 2} : FmPrev{nullptr, 0, 0}; }

// ---- handing the state to the bit-exact kernels -----------------------------------------------------------------------------------------------------------
// Design Q's own y[-1] is within 1e-4 of the definition's, which a small |y| would turn into a wrong d[0]: before a bit-exact kernel reads it, or an
// assignment moves streams between the kernels, sdrfm_q_fix_yprev recomputes it from the raw samples design Q left — exactly behind a design-Q call.
static inline bool fm_carry_fix_yprev(const FmCarry& c) { return !c.yprev_exact && c.hist_q_valid; }
// the bit-exact kernels serve the whole call (bx_all), behind the fix: they leave the definition's y[-1] and no raw samples, and write no rows beside the next call
static inline void fm_carry_to_bx(FmCarry& c) { c.yprev_exact = true; c.hist_q_valid = false; c.prev_by_q = false; c.prev_ovl_audio = nullptr; }
// a new assignment of streams to kernels (route_apply), behind the fix and its refill of hist_q from hist_b; who served the previous call is as it was
static inline void fm_carry_assigned(FmCarry& c) { c.yprev_exact = true; c.hist_q_valid = true; }

// ---- design Q's launch ------------------------------------------------------------------------------------------------------------------------------------
// The slot the call's launches go to: internal stream 0 or 1 in turn for an overlapped call, else 2 = the handle's stream.  busy: the handle's stream holds work
// (what hipStreamQuery answered, asked for an overlapped call only); wait_in: the internal stream has to wait for ovl_in, recorded behind that work.
struct FmSlot { uint32_t k; bool wait_in; };
static inline FmSlot fm_carry_slot(FmCarry& c, bool ovl, bool busy) {
  if (!ovl) return FmSlot{2u, false};
  const uint32_t k = c.ovl_next;
  c.ovl_next ^= 1u;
  return FmSlot{k, busy};
}
// Before the launch.  refill_hist_q: the repair path's raw samples have to be taken from hist_b first (the first design-Q call behind a reset or a bit-exact
// call; an overlapped call reads the previous call's buffer instead); yprev_exact: for the kernel's parameters; carry: the kernel carries ovl_done[slot] as its
// stop event (a caller that joins after every call: fm_route_stop).
struct FmQPre { bool refill_hist_q, yprev_exact, carry; };
static inline FmQPre fm_carry_q_pre(const FmCarry& c, bool ovl, uint32_t T) {
  return FmQPre{!c.hist_q_valid && !ovl && T > 1, c.yprev_exact, ovl && c.ovl_join_style};
}
// After it.  k, carry: as above; A: audio outputs per stream; with_chain, pcm_no_audio: as the launch went out.
static inline void fm_carry_q_launched(FmCarry& c, bool ovl, uint32_t k, bool carry, const FmRows& r, uint32_t A, bool with_chain, bool pcm_no_audio) {
  if (ovl) { c.ovl_pending[k] = true; c.ovl_bound[k] = carry; }
  c.prev_ovl_audio = (ovl && !(with_chain && pcm_no_audio)) ? r.audio : nullptr; c.prev_ovl_audio_stride = r.audio_stride; c.prev_ovl_audio_n = A;
  c.prev_ovl_pcm = (ovl && with_chain) ? r.pcm : nullptr; c.prev_ovl_pcm_stride = r.pcm_stride;
  c.yprev_exact = false; c.hist_q_valid = true; c.prev_by_q = true;
}

// ---- the end of the call: the other state set is the current one, the streams have moved on; a host-buffer call leaves nothing to warm up from ----------------
static inline void fm_carry_advance(FmCarry& c, const FmCounts& n, const FmRows& r, bool device_ptrs) {
  c.cur ^= 1;
  c.n_seen += n.N;
  if (device_ptrs) { c.prev_iq = r.iq; c.prev_stride = r.iq_stride; c.prev_nbytes = r.nbytes; }
  else c.prev_iq = nullptr;
  c.phase_x = n.phase_x; c.phase_d = n.phase_d;
}

// ---- the joins ------------------------------------------------------------------------------------------------------------------------------------------------
// Per internal stream k: record ovl_done[k] on it first (its latest kernel does not carry the event), then make the joining stream wait for ovl_done[k].
//   FM_JOIN_ALL        everything overlapped so far, onto the handle's stream (join_overlap: sdrfm_flush, and every call or entry that needs the stream in order)
//   FM_JOIN_PREVIOUS   all but the latest overlapped call, onto the handle's stream (sdrfm_flush_previous): the stream the NEXT call takes = the one the call
//                      before the latest took
//   FM_JOIN_PREVIOUS_ON_CALLER   the same onto a stream of the caller's (sdrfm_wait_previous)
// The two previous-joins say that the caller joins after every call: from then on the kernels carry their stream's completion event (fm_carry_q_pre).
enum FmJoinKind : uint8_t { FM_JOIN_ALL, FM_JOIN_PREVIOUS, FM_JOIN_PREVIOUS_ON_CALLER };
struct FmJoin { bool record[2], wait[2]; };
static inline FmJoin fm_carry_join(FmCarry& c, FmJoinKind kind) {
  FmJoin j = {{false, false}, {false, false}};
  if (kind != FM_JOIN_ALL) c.ovl_join_style = true;
  for (uint32_t k = 0; k < 2; ++k) {
    if (kind != FM_JOIN_ALL && k != c.ovl_next) continue;
    j.wait[k] = c.ovl_pending[k];
    j.record[k] = c.ovl_pending[k] && !c.ovl_bound[k];
  }
  return j;
}
// Slot k's record and wait are issued.  KEPT AS IT IS, the difference between the two previous-joins: the handle's stream now stands behind stream k, which
// is pending no more (ovl_bound is not touched: a later kernel rewrites it); a caller's stream says nothing about the handle's, so stream k stays pending
// for the handle's next join and the event just recorded is marked bound — recorded once, it covers the stream's latest call for every later waiter.
static inline void fm_carry_joined(FmCarry& c, FmJoinKind kind, uint32_t k) {
  if (kind == FM_JOIN_PREVIOUS_ON_CALLER) c.ovl_bound[k] = true;
  else c.ovl_pending[k] = false;
}

#endif
