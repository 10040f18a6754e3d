/*
 * sdrfm_fm_route.h — the FM handle's per-stream routing between design Q and the bit-exact kernels: the host's bookkeeping, without HIP.
 *
 * Which kernel serves a stream is also a matter of what the stream holds: noise-only input sends design Q to its repair path at
 * almost every audio stage (3 x the time of a carrier's call; the bit-exact kernels: 1.4 x), and a kernel lasts as long as its slowest
 * wave — so the choice is made PER STREAM (round 5; rounds 3 - 4: per handle).  Design Q's waves add their repair passes into a word per
 * stream (device memory); a window of SDRFM_Q_ADAPT_WINDOW design-Q calls is read back on a side stream behind the completion events of
 * the window's last kernels (hipExtLaunchKernelGGL stop events: no marker packets in the compute queues).  A stream more than a quarter of whose audio stages needed a repair
 * pass is served by the bit-exact kernels for SDRFM_Q_ADAPT_BACKOFF calls (design-B workgroups over the list of such streams INSIDE design
 * Q's launch over the others — sdrfm_q.hip: k_mix — or, where design B has no instance, a launch ahead of it), then tried on design Q again.
 * DETERMINISTIC since round 6: a window's statistics take effect at a FIXED call — the first design-Q call of the window
 * SDRFM_Q_ADAPT_SETS windows later, when the window's counter set comes round again — whenever the read-back arrived; should it not have arrived by then
 * (a host more than SETS - 1 windows of calls ahead of its device) that call waits for it.  Which kernel serves a stream at which call is therefore a
 * function of the bytes and the call sequence alone: two runs of one capture give the same bits (tests/test_route_gpu.py).  Every choice is within the
 * tolerance, a stream's audio is bit-identical to what its kernel gives alone, and SDRFM_CFG_BIT_EXACT pins the kernels.
 *
 * That promise is a property of the integers below alone, so they live here in the manner of sdrfm_fm_call.h: plain C++17, values and small PODs in and out.
 * A function says what the caller has to do — wait for a read-back, record an event, which event a kernel carries — and never does it: sdrfm.hip keeps the
 * buffers, events and streams and the order of the HIP calls, and tests/native/fm_route_check.cpp (tests/test_fm_route_cpu.py) drives the same functions
 * against an emulated device on a CPU.  Internal to the library; the drop-in boundary is include/sdrfm.h.
 */
#ifndef SDRFM_FM_ROUTE_H
#define SDRFM_FM_ROUTE_H

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define SDRFM_Q_ADAPT_WINDOW 16u     /* design-Q calls per window of per-stream repair statistics */
#define SDRFM_Q_ADAPT_SETS 4u        /* counter sets taken in turn: a window's statistics take effect when its set comes round again — at the first design-Q call of the
                                        window SETS windows later, a FIXED call: the host waits there if the device has not delivered them (a host > (SETS - 1) windows ahead) */
#define SDRFM_Q_ADAPT_BACKOFF 1024u  /* eligible calls served by the bit-exact kernels after a window of noise-like input */

// A design-Q kernel goes to one of three slots: internal stream 0, internal stream 1, the handle's stream (2).
struct FmRoute {
  uint32_t ns;
  // the assignment FLAGGED: what the statistics, the retries and the test hook have decided ...
  uint8_t* noisy; uint64_t* retry_at;   // per stream: served by the bit-exact kernels until call retry_at (~0: pinned by the test hook)
  uint64_t calls, next_retry;           // calls made since reset, design Q's or not; the earliest retry_at among the flagged streams
  bool dirty;                           // ... differs from the assignment IN FORCE, which the kernels run by until the caller has applied the new one:
  uint32_t n_noisy; int list_cur;       // the list version in use, [ns - n_noisy clean streams | n_noisy noisy streams]
  bool applied_pending[2];              // list version v: its copy to the device is enqueued, its host buffer must not be rewritten before it is over
  // the open window
  uint32_t win_calls, set; uint64_t win_stages;   // design-Q calls so far, the counter set they add into, audio stages per stream they cover
  bool win_used[3], win_need[3];        // per slot: holds kernels of the window at all / holds kernels no event covers
  // the closed windows: read-back of set i under way; audio stages per stream its window covered
  bool rb_pending[SDRFM_Q_ADAPT_SETS]; uint64_t rb_stages[SDRFM_Q_ADAPT_SETS];
  uint32_t bx_slot;                     // the bit-exact sub-launches of mixed calls take two completion events in turn
};

static inline bool fm_route_alloc(FmRoute& r, uint32_t ns) {
  r.ns = ns; r.next_retry = ~0ull;
  r.noisy = static_cast<uint8_t*>(calloc(ns, 1)); r.retry_at = static_cast<uint64_t*>(calloc(ns, sizeof(uint64_t)));
  return r.noisy && r.retry_at;
}
static inline void fm_route_free(FmRoute& r) { free(r.noisy); free(r.retry_at); r.noisy = nullptr; r.retry_at = nullptr; }
// Every stream back on design Q, no window open, no read-back expected (the caller has synchronised the device and cleared its counters).
static inline void fm_route_reset(FmRoute& r) {
  memset(r.noisy, 0, r.ns);
  r.n_noisy = 0; r.next_retry = ~0ull; r.dirty = false; r.applied_pending[0] = r.applied_pending[1] = false; r.calls = 0;
  r.win_calls = 0; r.win_stages = 0; r.set = 0;
  for (int k = 0; k < 3; ++k) r.win_need[k] = r.win_used[k] = false;
  for (uint32_t i = 0; i < SDRFM_Q_ADAPT_SETS; ++i) r.rb_pending[i] = false;
}

// ---- intake, at a call design Q can take: read-back, retries, then (dirty) the caller applies the flagged assignment -------------------------------
// The counter set whose read-back must be taken in at this call (the caller waits for it first), or -1: the first design-Q call of a window takes in what
// the window that last counted into its set left — SETS windows ago, (SETS - 1) windows of calls after the read-back was enqueued.
static inline int fm_route_due(const FmRoute& r) { return (r.win_calls == 0 && r.rb_pending[r.set]) ? (int)r.set : -1; }
// pass[s]: repair passes of stream s in that window.  More than a quarter of its audio stages: the stream leaves design Q for a while.
// (rb_stages adds fm_win_stages of every call with the run count that call was launched with.  fm_win_stages leaves the warm-up quads out — runs x ceil(floor(q_steps
// / runs) / Da) —, so at configs[2] it counts 3 stages for each of a serial call's 12 runs, which execute 4 (and take a pass at each), and 4 for each of an overlapped
// call's 10 runs, which execute 4: the threshold is more than 9 passes out of 48 executed stages in a window of serial calls and more than 10 out of 40 in a window of
// overlapped ones — 19 % against 25 %.  A noise-only stream repairs at almost every stage and a carrier at none, so both sit far from either figure.)
static inline void fm_route_take(FmRoute& r, uint32_t set, const uint32_t* pass) {
  r.rb_pending[set] = false;
  for (uint32_t s = 0; s < r.ns; ++s)
    if (!r.noisy[s] && (uint64_t)pass[s] * 4u > r.rb_stages[set]) {   // (a stream already flagged keeps its retry_at: the hook's pin, or an earlier window's)
      r.noisy[s] = 1; r.dirty = true;
      r.retry_at[s] = r.calls + SDRFM_Q_ADAPT_BACKOFF;
      if (r.retry_at[s] < r.next_retry) r.next_retry = r.retry_at[s];
    }
}
// streams whose time on the bit-exact kernels is over (counted in calls): design Q is tried again
static inline void fm_route_retry(FmRoute& r) {
  if (r.calls < r.next_retry) return;
  r.next_retry = ~0ull;
  for (uint32_t s = 0; s < r.ns; ++s) {
    if (!r.noisy[s]) continue;
    if (r.retry_at[s] <= r.calls) { r.noisy[s] = 0; r.dirty = true; }
    else if (r.retry_at[s] < r.next_retry) r.next_retry = r.retry_at[s];
  }
}
// Every call counts towards the back-off, also one design Q cannot take — AFTER its intake: a read-back taken in at call c is retried at call c + BACKOFF.
static inline void fm_route_count_call(FmRoute& r) { ++r.calls; }

// ---- applying the flagged assignment: begin (v: the list version to fill; wait: for its previous copy first), fill, [the caller's copies, still by the
// assignment in force], commit -----------------------------------------------------------------------------------------------------------------------
struct FmRouteList { int v; bool wait; };
static inline FmRouteList fm_route_list_begin(FmRoute& r) {
  const FmRouteList l = {r.list_cur ^ 1, r.applied_pending[r.list_cur ^ 1]};   // (a copy enqueued two assignments ago: over, but for a host that far ahead)
  r.applied_pending[l.v] = false;
  return l;
}
struct FmRouteCounts { uint32_t n_clean, n_noisy; };
static inline FmRouteCounts fm_route_list_fill(const FmRoute& r, uint32_t* list) {   // [clean streams ascending | noisy streams ascending]
  FmRouteCounts n = {0, 0};
  for (uint32_t s = 0; s < r.ns; ++s) if (!r.noisy[s]) list[n.n_clean++] = s;
  for (uint32_t s = 0; s < r.ns; ++s) if (r.noisy[s]) list[n.n_clean + n.n_noisy++] = s;
  return n;
}
static inline void fm_route_list_commit(FmRoute& r, int v, uint32_t n_noisy) { r.applied_pending[v] = true; r.list_cur = v; r.n_noisy = n_noisy; r.dirty = false; }

// The test hook: mask[s] != 0 flags stream s, 0 clears it; either way the stream is pinned (no retry moves it; the statistics may still flag a cleared one).
static inline bool fm_route_set_mask(FmRoute& r, const uint8_t* mask) {
  r.next_retry = ~0ull;
  for (uint32_t s = 0; s < r.ns; ++s) {
    const uint8_t want = mask[s] ? 1 : 0;
    if (r.noisy[s] != want) r.dirty = true;
    r.noisy[s] = want; r.retry_at[s] = ~0ull;
  }
  return r.dirty;
}

// ---- the window ---------------------------------------------------------------------------------------------------------------------------------
enum FmRouteEvent : uint8_t { FM_ROUTE_NO_EVENT, FM_ROUTE_WINDOW_EVENT, FM_ROUTE_OVL_DONE };   // the window's event [set][slot]; the overlap's ovl_done[slot]
// What a design-Q kernel on slot k carries as its stop event, and the counter set it adds into.  counting: the handle keeps statistics (every window counts:
// its set was taken in at the window's first call).  The window's last two calls carry the window's event — both internal streams are covered when calls
// take them in turn; carry: a caller that joins after every call has the kernel carry its internal stream's ovl_done instead, which stands for everything
// the stream holds, the window's kernels included.
struct FmRouteStop { FmRouteEvent evt; uint32_t set; };
static inline FmRouteStop fm_route_stop(FmRoute& r, bool counting, uint32_t k, bool carry) {
  FmRouteStop s = {FM_ROUTE_NO_EVENT, r.set};
  if (counting) {
    r.win_used[k] = true;
    if (r.win_calls + 2 >= SDRFM_Q_ADAPT_WINDOW) { s.evt = FM_ROUTE_WINDOW_EVENT; r.win_need[k] = false; }
    else r.win_need[k] = true;
  }
  if (carry) { s.evt = FM_ROUTE_OVL_DONE; if (r.win_used[k]) r.win_need[k] = false; }
  return s;
}
// The call is counted into the window (stages: fm_win_stages of the call); true: the window closes behind it.
static inline bool fm_route_count(FmRoute& r, uint64_t stages) { r.win_stages += stages; return ++r.win_calls >= SDRFM_Q_ADAPT_WINDOW; }
// The close: per slot, whether the window's event has to be recorded on it first (it holds kernels of the window that no attached event covers) and which
// event the side stream waits for before it collects counter set `set` (bound[k]: the latest kernel of internal stream k carries ovl_done[k], at or behind
// the window's last kernel there).  The next window counts into the next set; this one's read-back is expected when the set comes round.
struct FmRouteClose { uint32_t set; bool record[3]; FmRouteEvent wait[3]; };
static inline FmRouteClose fm_route_close(FmRoute& r, bool bound0, bool bound1) {
  FmRouteClose c = {r.set, {false, false, false}, {FM_ROUTE_NO_EVENT, FM_ROUTE_NO_EVENT, FM_ROUTE_NO_EVENT}};
  const bool bound[3] = {bound0, bound1, false};
  for (int k = 0; k < 3; ++k) {
    if (!r.win_used[k]) continue;
    c.record[k] = r.win_need[k];
    c.wait[k] = bound[k] ? FM_ROUTE_OVL_DONE : FM_ROUTE_WINDOW_EVENT;
    r.win_used[k] = r.win_need[k] = false;
  }
  r.rb_pending[r.set] = true; r.rb_stages[r.set] = r.win_stages;
  r.set = (r.set + 1u) % SDRFM_Q_ADAPT_SETS; r.win_calls = 0; r.win_stages = 0;
  return c;
}
// a mixed call's bit-exact launch of its own: the completion event it takes; the previous such launch's is the other one
static inline uint32_t fm_route_bx_take(FmRoute& r) { const uint32_t mine = r.bx_slot; r.bx_slot ^= 1u; return mine; }

#endif
