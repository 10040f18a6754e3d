/* The FM handle's carried state and overlap joins (csrc/sdrfm_fm_carry.h) on a CPU, under UBSan (tests/test_fm_carry_cpu.py builds and runs this).
 *
 * Handle drives the header in enqueue()'s order — counts, who serves (fm_serve on the geometry the library plans: fm_geom.h), the overlap decision, the
 * join or the slot, the hand-over, design Q's launch, the end of the call — against two internal streams kept as kernel counts and their ovl_done events
 * as positions in them, and keeps an account of its own beside the carry.
 *   known answers   every sequence of tests/fm_shape_cases.py: overlap_cases() with the term that refuses the flag, each row collision alone, when
 *                   sdrfm_q_fix_yprev and the hist_q refill are asked for, the slots, and the three joins' record and wait lists on a six-call script
 *   properties      over a seeded sweep of call sequences (fit or not, flagged or not, device or host rows, routed or not) with the three joins, assignments
 *                   and resets in between: (a) - (f) below
 * Prints "ok" and exits 0, or says what failed and exits 1. */
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_fm_carry.h"
#include "fm_geom.h"

static int g_failed = 0;
#define CHECK(cond, ...)                                                         \
  do {                                                                           \
    if (!(cond)) {                                                               \
      if (g_failed < 20) { printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
      ++g_failed;                                                                \
    }                                                                            \
  } while (0)

static uint64_t mix64(uint64_t z) {                              // splitmix64's finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
struct Rng {
  uint64_t s;
  uint64_t next() { return mix64(s += 0x9e3779b97f4a7c15ull); }
  uint32_t in(uint32_t lo, uint32_t hi) { return lo + (uint32_t)(next() % ((uint64_t)hi - lo + 1)); }
  bool one_in(uint32_t n) { return next() % n == 0; }
};

template <class P> static P* at(unsigned buffer, unsigned offset = 0) { return reinterpret_cast<P*>((((uintptr_t)buffer + 1) << 28) + offset); }   // rows 256 MB apart
static unsigned long g_verdicts[8];                              // how often the sweep met each answer of fm_carry_overlap
static const char* const kOvl[] = {"yes", "not-asked", "no-prev-buffer", "prev-not-q", "geometry", "iq-rows", "audio-rows", "pcm-rows"};

struct Call {
  uint32_t nsamp; unsigned cls; bool flag, device;                // samples per stream, alignment class of the rows (16, 4, 1), SDRFM_F_OVERLAP, device pointers
  int iq, audio, pcm;                                            // buffers (-1: the next in turn: three inputs, two outputs; audio -2: none given); pcm >= 0: the chain rides
};
static Call call(uint32_t nsamp, unsigned cls = 16, bool flag = false, bool device = true) { return Call{nsamp, cls, flag, device, -1, -1, -1}; }
static Call q(uint32_t nsamp) { return call(nsamp, 16, true); }
struct Did { FmOvl ovl; uint32_t slot; bool q_ok, fix_yprev, refill, carry; };

struct Handle {
  FmGeom g;
  FmCarry cy;
  uint32_t n_noisy;                                              // streams the assignment in force routes to the bit-exact kernels
  unsigned calls;
  // the emulated device: kernels on internal stream 0 / 1, where ovl_done[k] stands in its stream, how far the handle's stream is ordered behind stream k
  uint64_t pos[2], done[2], joined[2];
  std::string log;                                               // the joins' records and waits: "r0w0r1w1"
  // the test's own account
  bool last_dev, last_q, q_yprev;                                // the latest call since the reset: device rows / design Q served; y[-1] is design Q's own
  int last_ovl_slot;

  explicit Handle(uint32_t ns, uint32_t T = 64) : n_noisy(0), calls(0), last_dev(false), last_q(false), q_yprev(false), last_ovl_slot(-1) {
    g = fm_test_geom(T, 10, 32, 5, ns, false, fm_test_facts_mi355x(T, 10, 5));
    memset(&cy, 0, sizeof(cy)); memset(pos, 0, sizeof(pos)); memset(done, 0, sizeof(done)); memset(joined, 0, sizeof(joined));
    fm_carry_reset(cy);                                           // sdrfm_create: a zeroed handle, then sdrfm_reset
    invariants();
  }

  void join(FmJoinKind kind) {                                   // sdrfm.hip: join()
    const FmJoin j = fm_carry_join(cy, kind);
    // (e) the two previous-joins never touch the stream of the latest overlapped call
    if (kind != FM_JOIN_ALL && last_ovl_slot >= 0) CHECK(!j.record[last_ovl_slot] && !j.wait[last_ovl_slot], "join %d touches slot %d", (int)kind, last_ovl_slot);
    for (uint32_t k = 0; k < 2; ++k) {
      CHECK(!j.record[k] || j.wait[k], "slot %u: a record nobody waits for", k);
      if (j.record[k]) { done[k] = pos[k]; log += k ? "r1" : "r0"; }
      if (!j.wait[k]) continue;
      log += k ? "w1" : "w0";
      // (c) an event that is waited for stands behind the latest kernel of its stream
      CHECK(done[k] == pos[k], "slot %u: the event stands at %" PRIu64 ", the latest kernel at %" PRIu64, k, done[k], pos[k]);
      if (kind != FM_JOIN_PREVIOUS_ON_CALLER) joined[k] = done[k];
      fm_carry_joined(cy, kind, k);
    }
    if (kind == FM_JOIN_ALL) {
      // (d) after join-all nothing is pending, and the handle's stream stands behind everything
      for (int k = 0; k < 2; ++k) CHECK(!cy.ovl_pending[k] && joined[k] == pos[k], "slot %d after join-all: pending %d, joined %" PRIu64 " of %" PRIu64, k, (int)cy.ovl_pending[k], joined[k], pos[k]);
    }
    invariants();
  }
  void reset() { join(FM_JOIN_ALL); fm_carry_reset(cy); last_dev = last_q = q_yprev = false; invariants(); }   // sdrfm_reset
  bool assign(uint32_t nn) {                                     // route_apply: true = sdrfm_q_fix_yprev ran
    join(FM_JOIN_ALL);
    const bool fix = fm_carry_fix_yprev(cy);
    CHECK(fix == q_yprev, "assignment: fix %d, design Q's y[-1] %d", (int)fix, (int)q_yprev);
    fm_carry_assigned(cy); q_yprev = false; n_noisy = nn;
    invariants();
    return fix;
  }
  void invariants() {
    // (b) bound: a design-Q kernel or sdrfm_wait_previous put the event behind the stream's latest kernel
    for (int k = 0; k < 2; ++k) CHECK(!cy.ovl_bound[k] || done[k] == pos[k], "slot %d bound, event at %" PRIu64 " of %" PRIu64, k, done[k], pos[k]);
    // (f) y[-1] is not the definition's exactly when design Q served last and neither an assignment, a hand-over nor a reset came since
    CHECK(cy.yprev_exact == !q_yprev, "yprev_exact %d, design Q's y[-1] %d", (int)cy.yprev_exact, (int)q_yprev);
    CHECK(!cy.prev_by_q || cy.hist_q_valid, "design Q served the previous call and left no raw samples");
    CHECK(cy.prev_by_q == last_q && (cy.prev_iq != nullptr) == last_dev, "prev_by_q %d (%d), prev buffer %d (%d)", (int)cy.prev_by_q, (int)last_q, cy.prev_iq != nullptr, (int)last_dev);
    for (int k = 0; k < 2; ++k) CHECK(!cy.ovl_pending[k] || joined[k] < pos[k] || pos[k] == 0, "slot %d pending with nothing to join", k);
  }

  Did process(const Call& c, bool chain = false, bool pcm_no_audio = false) {   // enqueue()
    const unsigned off = c.cls == 16 ? 0 : c.cls;
    const uint32_t nbytes = 2 * c.nsamp;
    const size_t stride = (nbytes + 255u) / 256u * 256u + off;
    const FmRows rows = {at<const uint8_t>(c.iq >= 0 ? c.iq : calls % 3, c.device ? off : 0), c.device ? stride : stride - off, nbytes,
                         c.audio == -2 ? nullptr : at<const float>(8 + (c.audio >= 0 ? c.audio : calls % 2)), 512,
                         c.pcm >= 0 ? at<const int16_t>(12 + c.pcm) : nullptr, 1024};
    const FmCounts n = fm_carry_counts(cy, nbytes, g.D, g.Da);
    const FmCall cl = fm_carry_call(cy, n, rows.iq, rows.iq_stride);
    const FmServe sv = fm_serve(g, cl, fm_q_fit(g, cl) ? n_noisy : 0u);
    Did d = {FM_OVL_NOT_ASKED, 2u, sv.q_ok, false, false, false};
    const bool with_chain = chain && c.pcm >= 0 && sv.q_ok;
    d.ovl = fm_carry_overlap(cy, g, cl, rows, sv.q_ok, c.flag, with_chain, pcm_no_audio, g.n_streams);
    const bool ovl = d.ovl == FM_OVL_YES;
    ++g_verdicts[d.ovl];
    // (a) a call is overlapped only right behind a device-pointer call that design Q served
    CHECK(!ovl || (c.flag && sv.q_ok && last_dev && last_q), "call %u overlapped: flag %d, q_ok %d, behind device rows %d, design Q %d", calls, (int)c.flag, (int)sv.q_ok, (int)last_dev, (int)last_q);
    if (!ovl) join(FM_JOIN_ALL);
    if (sv.bx_all) {
      d.fix_yprev = fm_carry_fix_yprev(cy);
      CHECK(d.fix_yprev == q_yprev, "call %u: fix %d, design Q's y[-1] %d", calls, (int)d.fix_yprev, (int)q_yprev);
      fm_carry_to_bx(cy); q_yprev = false;
    }
    const FmSlot slot = fm_carry_slot(cy, ovl, false);
    d.slot = slot.k;
    CHECK(ovl ? slot.k < 2 && slot.k != (uint32_t)last_ovl_slot : slot.k == 2, "call %u takes slot %u behind slot %d", calls, slot.k, last_ovl_slot);
    const FmPrev pv = fm_carry_prev(cy, ovl);
    CHECK(ovl ? pv.iq == cy.prev_iq && pv.N == cy.prev_nbytes / 2 : !pv.iq && !pv.N, "call %u: warm-up rows", calls);
    if (sv.q_ok) {
      const FmQPre pre = fm_carry_q_pre(cy, ovl, g.T);
      d.refill = pre.refill_hist_q; d.carry = pre.carry;
      CHECK(pre.yprev_exact == !q_yprev, "call %u: the kernel is told yprev_exact %d", calls, (int)pre.yprev_exact);
      if (ovl) { ++pos[slot.k]; if (pre.carry) done[slot.k] = pos[slot.k]; last_ovl_slot = (int)slot.k; }
      fm_carry_q_launched(cy, ovl, slot.k, pre.carry, rows, cl.A, with_chain, pcm_no_audio);
      q_yprev = true;
    }
    fm_carry_advance(cy, n, rows, c.device);
    last_dev = c.device; last_q = sv.q_ok;
    ++calls;
    invariants();
    return d;
  }
};

// ---- known answers ---------------------------------------------------------------------------------------------------------------------------------------
struct Step { Call c; FmOvl want; };
static void sequence(const char* name, uint32_t ns, const std::vector<Step>& steps, uint32_t n_routed = 0, unsigned route_at = 0) {
  Handle h(ns);
  for (size_t i = 0; i < steps.size(); ++i) {
    if (n_routed && i == route_at) {
      h.assign(n_routed);                                        // the hook right before the call: hist_q refilled from design B's samples ...
      CHECK(h.cy.hist_q_valid && !h.cy.prev_by_q, "%s: the assignment sets hist_q_valid and leaves prev_by_q", name);   // ... and the flagged call still refused
    }
    const Did d = h.process(steps[i].c);
    CHECK(d.ovl == steps[i].want, "%s call %zu: %s, expected %s", name, i, kOvl[d.ovl], kOvl[steps[i].want]);
  }
}

static void known_answers() {
  const Step tail = {call(777), FM_OVL_NOT_ASKED};                // tests/fm_shape_cases.py: TAIL
  const Step first = {call(1600), FM_OVL_NOT_ASKED};
  sequence("other-size-and-stride", 264, {{call(3200), FM_OVL_NOT_ASKED}, {q(1600), FM_OVL_YES}, {q(2000), FM_OVL_YES}, tail});
  sequence("prev-4-aligned", 264, {first, {call(1600, 4), FM_OVL_NOT_ASKED}, {q(1600), FM_OVL_PREV_NOT_Q}, tail});
  sequence("prev-short", 512, {first, {q(1200), FM_OVL_YES}, {q(1600), FM_OVL_GEOMETRY}, {q(1600), FM_OVL_YES}, tail});
  sequence("prev-not-whole-pieces", 264, {first, {call(1650), FM_OVL_NOT_ASKED}, {q(1600), FM_OVL_PREV_NOT_Q}, tail});
  sequence("prev-served-by-b", 200, {{q(1600), FM_OVL_NOT_ASKED}, {q(3200), FM_OVL_PREV_NOT_Q}, {q(3200), FM_OVL_YES}, tail});
  sequence("prev-host", 264, {first, {call(1600, 16, false, false), FM_OVL_NOT_ASKED}, {q(1600), FM_OVL_NO_PREV_BUFFER}, {q(1600), FM_OVL_YES}, tail});
  sequence("flag-on-unaligned", 264, {first, {call(1600, 4, true), FM_OVL_NOT_ASKED}, {q(1600), FM_OVL_PREV_NOT_Q}, {q(1600), FM_OVL_YES}, tail});
  sequence("prev-served-by-b-then-routed", 264, {first, {call(1600, 4), FM_OVL_NOT_ASKED}, {q(1600), FM_OVL_PREV_NOT_Q}, {q(1600), FM_OVL_YES}, tail}, 66, 2);

  {  // each row collision alone, behind an overlapped call (input 1, audio 1, PCM 1 with the chain in its launch); 4400 samples: 14 quads, the fewest a chain's run needs
    for (int what = 0; what < 5; ++what) {
      Handle h(264);
      Call c0 = q(4400), c1 = q(4400), c2 = q(4400);
      c0.iq = 0; c0.audio = 0; c0.pcm = 0; c1.iq = 1; c1.audio = 1; c1.pcm = 1; c2.iq = 2; c2.audio = 0; c2.pcm = 0;
      FmOvl want = FM_OVL_YES;
      bool no_audio = false;
      if (what == 1) { c2.iq = 1; want = FM_OVL_IQ_ROWS; }                        // the same iq buffer as the previous call
      if (what == 2) { c2.audio = 1; want = FM_OVL_AUDIO_ROWS; }                  // the audio buffer the previous overlapped call writes
      if (what == 3) { c2.audio = 1; no_audio = true; }                           // ... by a call that writes no audio: the chain rides and stores none
      if (what == 4) { c2.pcm = 1; want = FM_OVL_PCM_ROWS; }                      // the PCM rows
      CHECK(h.process(c0, true).ovl == FM_OVL_NO_PREV_BUFFER, "the first call has nothing to warm up from");
      CHECK(h.process(c1, true).ovl == FM_OVL_YES, "an overlapped call with the chain");
      CHECK(h.cy.prev_ovl_audio == at<const float>(9) && h.cy.prev_ovl_pcm == at<const int16_t>(13), "the rows the overlapped call writes");
      const Did d = h.process(c2, true, no_audio);
      CHECK(d.ovl == want, "collision %d: %s, expected %s", what, kOvl[d.ovl], kOvl[want]);
      // the PCM rows of a call without the chain collide with nothing
      if (what == 4) { Handle p(264); p.process(c0, true); p.process(c1, true); CHECK(p.process(c2, false).ovl == FM_OVL_YES, "no chain, no PCM rows"); }
    }
  }
  {  // sdrfm_q_fix_yprev: exactly behind a design-Q call, never twice; the hist_q refill: the first design-Q call behind a reset or a bit-exact call
    Handle h(264);
    const Call b = call(1600, 4);                                 // design B's
    Did d = h.process(b);
    CHECK(!d.q_ok && !d.fix_yprev, "behind a reset: no fix");
    d = h.process(b);
    CHECK(!d.fix_yprev, "behind a bit-exact call: no fix");
    d = h.process(call(1600));
    CHECK(d.q_ok && d.refill, "the first design-Q call behind a bit-exact call refills hist_q");
    d = h.process(call(1600));
    CHECK(d.q_ok && !d.refill, "design Q left the raw samples");
    d = h.process(q(1600));
    CHECK(d.ovl == FM_OVL_YES && !d.refill, "an overlapped call asks for no refill");
    d = h.process(b);
    CHECK(d.fix_yprev, "a bit-exact call behind design Q: the fix");
    CHECK(!h.assign(0), "fixed once: the assignment behind it asks for none");
    d = h.process(call(1600));
    CHECK(d.q_ok && !d.refill, "the assignment behind the bit-exact call refilled hist_q");
    CHECK(h.assign(0), "an assignment behind design Q: the fix");
    CHECK(!h.assign(0), "never twice");
    d = h.process(b);
    CHECK(!d.fix_yprev, "the assignment fixed it");
    h.process(call(1600));
    CHECK(h.process(b).fix_yprev && !h.process(b).fix_yprev, "two bit-exact calls behind design Q: the first one's fix, never twice");
    h.process(call(1600));
    h.reset();
    CHECK(!fm_carry_fix_yprev(h.cy) && h.cy.cur == 0 && h.cy.n_seen == 0 && !h.cy.prev_iq, "behind a reset: no fix, the streams at their start");
    d = h.process(call(1600));
    CHECK(d.q_ok && d.refill, "the first design-Q call behind a reset refills hist_q");
    Handle one(512, 16);                                          // (T = 1 has no history to refill: the term is there, no handle of the library reaches it)
    CHECK(!fm_carry_q_pre(one.cy, false, 1).refill_hist_q && fm_carry_q_pre(one.cy, false, 2).refill_hist_q, "T > 1");
  }
  {  // a host-buffer call clears the previous buffer; the slots alternate, and a call on the handle's stream takes none
    Handle h(264);
    h.process(call(1600));
    CHECK(h.cy.prev_iq == at<const uint8_t>(0) && h.cy.prev_nbytes == 3200 && h.cy.cur == 1 && h.cy.n_seen == 1600, "a device call leaves its rows");
    h.process(call(1600, 16, false, false));
    CHECK(!h.cy.prev_iq && h.cy.prev_by_q && h.cy.cur == 0 && h.cy.n_seen == 3200, "a host-buffer call leaves none");
    h.process(call(1600));
    const uint32_t want[6] = {0, 1, 0, 2, 1, 0};
    for (int i = 0; i < 6; ++i) { const Did d = h.process(i == 3 ? call(1600) : q(1600)); CHECK(d.slot == want[i], "call %d on slot %u", i, d.slot); }
  }
  {  // the three joins on six flagged calls (the first on the handle's stream, then slots 0 1 0 1 0): what is recorded and waited for
    Handle a(264);
    for (int i = 0; i < 6; ++i) CHECK(!a.process(q(1600)).carry, "no join so far: no kernel carries an event");
    a.join(FM_JOIN_ALL); a.join(FM_JOIN_ALL);
    CHECK(a.log == "r0w0r1w1", "sdrfm_flush behind the burst: %s", a.log.c_str());
    Handle b(264), c(264);
    const char* const want_b[6] = {"", "", "w0", "w1", "w0", "w1"};
    for (int i = 0; i < 6; ++i) {
      CHECK(b.process(q(1600)).carry == (i > 0) && c.process(q(1600)).carry == (i > 0), "call %d: the kernels of a joining caller carry the event", i);
      b.log.clear(); c.log.clear();
      b.join(FM_JOIN_PREVIOUS); c.join(FM_JOIN_PREVIOUS_ON_CALLER);
      CHECK(b.log == want_b[i] && c.log == want_b[i], "join behind call %d: %s / %s, expected %s", i, b.log.c_str(), c.log.c_str(), want_b[i]);
    }
    b.log.clear(); c.log.clear();
    b.join(FM_JOIN_ALL); c.join(FM_JOIN_ALL);
    CHECK(b.log == "w0" && c.log == "w0w1", "sdrfm_flush at the end: %s (sdrfm_flush_previous joined stream 1), %s (sdrfm_wait_previous left both pending)", b.log.c_str(), c.log.c_str());
    // sdrfm_wait_previous behind kernels that carry nothing: recorded once, bound from then on; the handle's stream still has to join
    Handle w(264);
    for (int i = 0; i < 3; ++i) w.process(q(1600));               // slots 2 0 1
    w.join(FM_JOIN_PREVIOUS_ON_CALLER); w.join(FM_JOIN_PREVIOUS_ON_CALLER);
    CHECK(w.log == "r0w0w0" && w.cy.ovl_bound[0] && w.cy.ovl_pending[0], "%s", w.log.c_str());
    w.join(FM_JOIN_PREVIOUS);
    CHECK(w.log == "r0w0w0w0" && w.cy.ovl_bound[0] && !w.cy.ovl_pending[0], "%s", w.log.c_str());
    w.join(FM_JOIN_ALL);
    CHECK(w.log == "r0w0w0w0r1w1", "%s", w.log.c_str());
    // what a reset keeps
    w.process(q(1600)); w.process(q(1600));
    const FmCarry before = w.cy;
    w.reset();
    CHECK(w.cy.ovl_next == before.ovl_next && w.cy.ovl_join_style && w.cy.ovl_bound[0] == before.ovl_bound[0] && w.cy.ovl_bound[1] == before.ovl_bound[1] &&
          w.cy.prev_ovl_audio == before.prev_ovl_audio && w.cy.prev_ovl_audio_n == before.prev_ovl_audio_n && w.cy.prev_ovl_pcm == before.prev_ovl_pcm, "a reset keeps the overlap's own state");
  }
}

// ---- the sweep ---------------------------------------------------------------------------------------------------------------------------------------------
static void one_case(uint64_t seed) {
  Rng rng{seed};
  const uint32_t ns = rng.one_in(3) ? 200 : rng.one_in(2) ? 264 : 512;   // 200: design Q needs three steps
  Handle h(ns);
  const uint32_t p_unfit = rng.in(0, 40), p_flag = rng.in(20, 100), p_host = rng.one_in(2) ? 0 : rng.in(1, 30), p_join = rng.one_in(3) ? 0 : rng.in(1, 100);
  const uint32_t sizes[5] = {1600, 3200, 1200, 2000, 4400};
  const uint32_t n_acts = rng.in(20, 200);
  for (uint32_t i = 0; i < n_acts; ++i) {
    Call c = call(sizes[rng.in(0, 4)], 16, rng.in(0, 99) < p_flag, rng.in(0, 99) >= p_host);
    if (rng.in(0, 99) < p_unfit) { if (rng.one_in(2)) c.cls = rng.one_in(2) ? 4 : 1; else c.nsamp = rng.one_in(2) ? 777 : 1650; }
    if (!c.device) c.flag = false;                                // (include/sdrfm.h: the flag without device pointers is refused before enqueue())
    if (rng.one_in(10)) c.iq = (int)rng.in(0, 2);                 // sometimes any buffer: row collisions
    if (rng.one_in(10)) c.audio = (int)rng.in(0, 1);
    c.pcm = (int)rng.in(0, 1);
    h.process(c, rng.one_in(3), rng.one_in(4));
    if (rng.in(0, 99) < p_join) h.join(rng.one_in(5) ? FM_JOIN_ALL : rng.one_in(3) ? FM_JOIN_PREVIOUS_ON_CALLER : FM_JOIN_PREVIOUS);
    if (rng.one_in(25)) h.assign(rng.one_in(2) ? 0u : rng.one_in(4) ? ns / 2 : ns / 4);   // (half of the streams routed: the bit-exact kernels take every call)
    if (rng.one_in(40)) h.reset();
  }
  h.join(FM_JOIN_ALL);
}

int main() {
  known_answers();
  unsigned long cases = 0;
  for (uint64_t seed = 1; seed <= 3000; ++seed, ++cases) one_case(0x7c15a9e3779b9f4bull + seed);
  printf("sweep: seed 0x7c15a9e3779b9f4b, %lu sequences; calls", cases);
  for (int v = 0; v < 8; ++v) { printf(" %s %lu", kOvl[v], g_verdicts[v]); CHECK(g_verdicts[v] >= 100, "the sweep hardly meets \"%s\"", kOvl[v]); }
  printf("\n");
  if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
  printf("ok\n");
  return 0;
}
