/* The FM handle's per-stream routing (csrc/sdrfm_fm_route.h) on a CPU, under UBSan (tests/test_fm_route_cpu.py builds and runs this).
 *
 * "Which kernel serves a stream at which call is a function of the bytes and the call sequence alone" is a property of the header's integers; the GPU tests
 * need 1 200 calls to see one back-off expire and cannot place a reset, a mask or a late read-back where they hurt.  Here the header is driven the way
 * csrc/sdrfm.hip drives it (Sim: intake, who serves, the kernel's stop event, the count, the close — with fm_serve of csrc/sdrfm_fm_call.h deciding who
 * serves, on the geometry the library plans: fm_geom.h; csrc/sdrfm_fm_carry.h deciding which calls overlap, their slots and the joins) against an emulated device: streams as kernel counts, events as positions in them, counter sets,
 * and a queue of read-backs of which the TEST decides when each one arrives.
 *   known answers   from the constants and from what tests/test_route_gpu.py holds on hardware (calls 64, 1088, 1152; window 68 closes at call 1103), the
 *                   list's order, the strict threshold, the call patterns that need no event record — literals here, not the header's macros
 *   properties      over a seeded sweep of call sequences (design Q's or not, overlapped or not, a joining caller or not), noise per stream and window,
 *                   read-back arrival, and a reset or a mask at any point: (a) - (f) below
 * Prints "ok" and exits 0, or says what failed and exits 1. */
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_fm_carry.h"
#include "../../stm32f7-rtlsdr_amd/csrc/sdrfm_fm_route.h"
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

// What the scheme is stated with (DESIGN.md 4.Q "Routing"): the checks count in these, the header in its macros.
static const uint32_t kWindow = 16, kSets = 4, kBackoff = 1024;

// ---- the emulated device and sdrfm.hip's sequencing around the header ----------------------------------------------------------------------------
struct Event { int slot; uint64_t pos; bool attached; uint64_t window; };   // where it stands in its stream; attached: a kernel's stop event, not a record
struct Readback { uint32_t set; uint64_t window; std::vector<uint32_t> pass; bool arrived; };
enum Arrival { AT_ONCE, NEVER_UNASKED, AT_RANDOM };              // when the device delivers a read-back (NEVER_UNASKED: the host is always SETS - 1 windows ahead)
// how much of a stream's audio stages need a repair pass in a window
enum Noise : uint8_t { CLEAN, A_QUARTER, ALL };

struct Sim {
  FmGeom g;
  FmCall c_fit, c_unfit;                                         // a call design Q can take, and one it cannot (an odd decimator phase)
  uint32_t ns;
  FmRoute r;
  std::vector<uint32_t> pass_dev[4], pass_host[4], list[2];
  uint32_t list_clean[2];
  std::deque<Readback> queue;
  Arrival arrival; Rng arrive_rng;
  uint64_t pos[3];                                               // kernels on internal stream 0, 1, the handle's stream
  Event win_evt[4][3], ovl_done[2];
  FmCarry cy;                                                    // the handle's carried state: the header's functions keep it, as in sdrfm.hip
  // the test's own account
  uint64_t epoch, window, call, taken;                           // resets so far; windows closed / calls made / read-backs taken in since the last one
  uint32_t my_win_calls;
  uint64_t win_last[3];                                          // position of the open window's last kernel per slot (0: none)
  std::vector<uint8_t> pinned; bool have_mask;
  std::vector<uint64_t> close_call, trace;
  unsigned records, forced;
  uint64_t noise_seed; uint32_t noisy_every;

  Sim(uint32_t n_streams, Arrival a, uint64_t seed, uint32_t every) : ns(n_streams), arrival(a), arrive_rng{seed ^ 0xa5a5}, noise_seed(seed), noisy_every(every) {
    g = fm_test_geom(64, 10, 32, 5, ns, false, fm_test_facts_mi355x(64, 10, 5));
    const FmCounts n = fm_counts(0, 0, 48000, g.D, g.Da);
    c_fit = FmCall{n.N, n.M, n.A, 0, 0, 1u << 20, true, true};
    c_unfit = c_fit; c_unfit.phase_x = 1;
    CHECK(fm_q_fit(g, c_fit) && !fm_q_fit(g, c_unfit), "%u streams", ns);
    memset(&r, 0, sizeof(r));
    CHECK(fm_route_alloc(r, ns), "alloc");
    for (int i = 0; i < 4; ++i) { pass_dev[i].assign(ns, 0); pass_host[i].assign(ns, 0xdeadbeef); }
    for (int v = 0; v < 2; ++v) { list[v].assign(ns, ~0u); list_clean[v] = 0; }
    memset(pos, 0, sizeof(pos)); memset(win_evt, 0, sizeof(win_evt)); memset(ovl_done, 0, sizeof(ovl_done)); memset(win_last, 0, sizeof(win_last));
    memset(&cy, 0, sizeof(cy));
    epoch = window = call = taken = 0; my_win_calls = 0; have_mask = false; records = forced = 0;
    reset();
  }
  ~Sim() { fm_route_free(r); }
  Sim(const Sim&) = delete;

  // noise-only streams (every noisy_every-th, as tests/test_route_gpu.py lays them out) and, in the sweep, anything per window
  Noise noise(uint32_t s) const {
    if (noisy_every) return s % noisy_every == 1 ? ALL : CLEAN;
    const uint64_t h = mix64(noise_seed ^ (epoch << 48) ^ (window << 24) ^ s);
    if (mix64(noise_seed ^ s) % 4 == 0) return (h & 1) ? A_QUARTER : CLEAN;   // a quarter of the streams never pass the threshold
    return h % 8 < 5 ? CLEAN : (h % 8 == 5 ? A_QUARTER : ALL);
  }
  bool never_over(uint32_t s) const { return noisy_every ? s % noisy_every != 1 : mix64(noise_seed ^ s) % 4 == 0; }

  void deliver(Readback& rb) { pass_host[rb.set] = rb.pass; rb.arrived = true; }
  void deliveries() {                                            // the side stream is in order: the oldest first
    for (Readback& rb : queue)
      if (!rb.arrived) { if (arrival == AT_ONCE || (arrival == AT_RANDOM && arrive_rng.one_in(24))) deliver(rb); else break; }
  }
  void record(Event& e, int slot) { e = Event{slot, pos[slot], false, window}; }
  void join(FmJoinKind kind) {                                   // sdrfm.hip's join(): the waits move no event
    const FmJoin j = fm_carry_join(cy, kind);
    for (uint32_t k = 0; k < 2; ++k) { if (j.record[k]) record(ovl_done[k], (int)k); if (j.wait[k]) fm_carry_joined(cy, kind, k); }
  }
  void join_overlap() { join(FM_JOIN_ALL); }
  void flush_previous() { join(FM_JOIN_PREVIOUS); }
  void wait_previous() { join(FM_JOIN_PREVIOUS_ON_CALLER); }

  void reset() {                                                 // sdrfm_reset: joins and synchronises, then route_reset
    join_overlap(); fm_carry_reset(cy);
    fm_route_reset(r);
    for (int i = 0; i < 4; ++i) pass_dev[i].assign(ns, 0);
    queue.clear();
    ++epoch; window = call = taken = 0; my_win_calls = 0; memset(win_last, 0, sizeof(win_last)); have_mask = false;
    close_call.clear();
  }
  void apply() {                                                 // route_apply
    join_overlap(); fm_carry_assigned(cy);
    const int cur = r.list_cur; const uint32_t nn = r.n_noisy;
    const FmRouteList l = fm_route_list_begin(r);
    CHECK(l.v == (cur ^ 1), "the list in use is rewritten");
    const FmRouteCounts n = fm_route_list_fill(r, list[l.v].data());
    CHECK(r.list_cur == cur && r.n_noisy == nn && r.dirty, "the assignment in force changed before the commit");   // (the caller's copies run by it)
    CHECK(n.n_clean + n.n_noisy == ns, "%u + %u of %u", n.n_clean, n.n_noisy, ns);
    for (uint32_t i = 0; i < ns; ++i) {                          // [clean ascending | noisy ascending]
      const uint32_t s = list[l.v][i];
      CHECK(s < ns && (r.noisy[s] != 0) == (i >= n.n_clean) && (i == 0 || i == n.n_clean || list[l.v][i - 1] < s), "list[%u] = %u", i, s);
    }
    list_clean[l.v] = n.n_clean;
    fm_route_list_commit(r, l.v, n.n_noisy);
    CHECK(r.list_cur == l.v && r.n_noisy == n.n_noisy && !r.dirty, "commit");
  }
  void set_mask(const std::vector<uint8_t>& m) {                  // sdrfm_debug_route
    if (fm_route_set_mask(r, m.data())) apply();
    pinned = m; have_mask = true;
    for (uint32_t s = 0; s < ns; ++s) CHECK(r.retry_at[s] == ~0ull && (r.noisy[s] != 0) == (m[s] != 0), "stream %u", s);
    CHECK(r.n_noisy == flagged(), "in force %u, flagged %u", r.n_noisy, flagged());
  }
  uint32_t flagged() const { uint32_t n = 0; for (uint32_t s = 0; s < ns; ++s) n += r.noisy[s]; return n; }

  void intake() {                                                // route_intake
    // (b) a window's read-back is taken in once, at the first call design Q can take of the window SETS windows later
    const bool expect = my_win_calls == 0 && !queue.empty() && queue.front().window + kSets == window;
    const int due = fm_route_due(r);
    CHECK((due >= 0) == expect, "call %" PRIu64 ": due %d, window %" PRIu64 ", %zu read-backs under way", call, due, window, queue.size());
    if (due >= 0 && !queue.empty()) {
      Readback& rb = queue.front();
      CHECK((uint32_t)due == rb.set && rb.window == taken, "set %d for window %" PRIu64 ", %" PRIu64 " taken so far", due, rb.window, taken);
      if (!rb.arrived) { deliver(rb); ++forced; }                // (the host waits for it: hipEventSynchronize)
      fm_route_take(r, (uint32_t)due, pass_host[due].data());
      queue.pop_front(); ++taken;
    }
    fm_route_retry(r);
    if (r.dirty) apply();
  }

  void close() {                                                 // route_window_close
    const FmRouteClose cw = fm_route_close(r, cy.ovl_bound[0], cy.ovl_bound[1]);
    CHECK(cw.set == window % kSets, "window %" PRIu64 " closes set %u", window, cw.set);
    uint64_t what = cw.set;
    for (int k = 0; k < 3; ++k) {
      what = what * 16 + cw.record[k] * 4 + cw.wait[k];
      if (!win_last[k]) { CHECK(cw.wait[k] == FM_ROUTE_NO_EVENT && !cw.record[k], "slot %d held no kernel of the window", k); continue; }
      // (c) covered by an event at or behind the window's last kernel there; no record where an attached event covers it already
      Event& we = win_evt[cw.set][k];
      const bool covered = (we.attached && we.window == window && we.pos >= win_last[k]) || (k < 2 && ovl_done[k].attached && ovl_done[k].pos >= win_last[k]);
      CHECK(!(cw.record[k] && covered), "window %" PRIu64 " slot %d: a record behind a stop event", window, k);
      if (cw.record[k]) { record(we, k); ++records; }
      CHECK(cw.wait[k] == FM_ROUTE_WINDOW_EVENT || (cw.wait[k] == FM_ROUTE_OVL_DONE && k < 2), "slot %d waits for %d", k, cw.wait[k]);
      const Event& e = cw.wait[k] == FM_ROUTE_OVL_DONE ? ovl_done[k < 2 ? k : 0] : we;
      CHECK(e.slot == k && e.pos >= win_last[k], "window %" PRIu64 " slot %d: event at %" PRIu64 ", last kernel at %" PRIu64, window, k, e.pos, win_last[k]);
      win_last[k] = 0;
    }
    trace.push_back(what);
    for (const Readback& rb : queue) CHECK(rb.set != cw.set, "set %u collected twice", cw.set);
    queue.push_back(Readback{cw.set, window, pass_dev[cw.set], false});   // k_route_collect: copies, and clears for the window after the next
    pass_dev[cw.set].assign(ns, 0);
    close_call.push_back(call);
    ++window; my_win_calls = 0;
  }

  // one sdrfm_process_batch_device call; returns true when design Q served (some of) it
  bool process(bool fit, bool want_ovl) {                        // enqueue()
    deliveries();
    const FmCall& c = fit ? c_fit : c_unfit;
    const bool q_fit = fm_q_fit(g, c);
    if (q_fit) intake();
    const uint32_t n_noisy = q_fit ? r.n_noisy : 0u, n_clean = ns - n_noisy;
    const FmServe sv = fm_serve(g, c, n_noisy);
    // (f) design Q serves n_clean > 0 streams only while 2 n_noisy < ns
    CHECK(sv.q_ok == (q_fit && 2 * n_noisy < ns && n_clean > 0) && sv.bx_all == !sv.q_ok, "call %" PRIu64 ": %u of %u routed", call, n_noisy, ns);
    CHECK(!n_noisy || list_clean[r.list_cur] == n_clean, "the list in use holds %u clean streams, design Q serves %u", list_clean[r.list_cur], n_clean);
    CHECK(r.n_noisy == flagged() && !r.dirty, "call %" PRIu64 ": in force %u, flagged %u", call, r.n_noisy, flagged());
    // (e) no retry sweep moves a stream the hook has flagged
    if (have_mask) for (uint32_t s = 0; s < ns; ++s) CHECK(!pinned[s] || r.noisy[s], "call %" PRIu64 ": pinned stream %u is back on design Q", call, s);
    for (uint32_t s = 0; s < ns; ++s) CHECK(!r.noisy[s] || !never_over(s) || (have_mask && pinned[s]), "call %" PRIu64 ": stream %u never passed the threshold", call, s);
    fm_route_count_call(r);
    uint64_t what = mix64(sv.q_ok * 8 + sv.mixed * 4 + sv.fuse * 2 + 1);
    for (uint32_t s = 0; s < ns; ++s) what = mix64(what ^ r.noisy[s]);
    // (three input buffers in turn, no audio rows: only who served the previous call can refuse the flag; c carries the position, the carry only the rest)
    const FmRows rows = {reinterpret_cast<const uint8_t*>((uintptr_t)(call % 3 + 1) << 28), 2 * (size_t)c.N, 2 * c.N, nullptr, 0, nullptr, 0};
    const bool ovl = fm_carry_overlap(cy, g, c, rows, sv.q_ok, want_ovl, false, false, ns) == FM_OVL_YES;
    if (!ovl) join_overlap();
    if (sv.bx_all) fm_carry_to_bx(cy);
    const uint32_t k = fm_carry_slot(cy, ovl, false).k;
    if (sv.mixed && !sv.fuse) (void)fm_route_bx_take(r);
    if (sv.q_ok) {
      const uint64_t at = ++pos[k];                              // the design-Q kernel
      const bool carry = fm_carry_q_pre(cy, ovl, g.T).carry;
      const FmRouteStop stop = fm_route_stop(r, true, k, carry);
      what = mix64(what ^ (stop.evt * 4 + stop.set));
      // (b) no set is counted into while its read-back is under way
      CHECK(stop.set == window % kSets, "call %" PRIu64 " counts into set %u in window %" PRIu64, call, stop.set, window);
      for (const Readback& rb : queue) CHECK(rb.set != stop.set, "call %" PRIu64 " counts into set %u, whose read-back is under way", call, stop.set);
      const FmSplit sp = fm_split(g, c, sv.mixed, sv.fuse, n_noisy);
      const uint32_t steps = fm_q_steps(c.M), runs = fm_q_runs(c, sp.q_total, n_clean, false, 0).runs;
      const uint64_t stages = fm_win_stages(runs, steps, g.Da);
      for (uint32_t i = 0; i < n_clean; ++i) {                    // design Q's waves add their repair passes, for the streams it serves
        const uint32_t s = n_noisy ? list[r.list_cur][i] : i;
        const Noise nz = noise(s);
        pass_dev[stop.set][s] += nz == ALL ? (uint32_t)stages : nz == A_QUARTER ? (uint32_t)(stages / 4) : 0u;
      }
      // (c) the window's event rides on one of the window's last two calls
      if (stop.evt == FM_ROUTE_WINDOW_EVENT) { CHECK(my_win_calls + 2 >= kWindow, "call %u of its window carries the window's event", my_win_calls); win_evt[stop.set][k] = Event{(int)k, at, true, window}; }
      if (stop.evt == FM_ROUTE_OVL_DONE) { CHECK(carry && k < 2, "slot %u", k); ovl_done[k < 2 ? k : 0] = Event{(int)k, at, true, window}; }
      CHECK(stop.evt != FM_ROUTE_NO_EVENT || (!carry && my_win_calls + 2 < kWindow), "call %u of its window carries no event", my_win_calls);
      win_last[k] = at;
      fm_carry_q_launched(cy, ovl, k, carry, rows, c.A, false, false);
      const bool closes = fm_route_count(r, stages);
      ++my_win_calls;
      CHECK(closes == (my_win_calls == kWindow), "call %u of its window %s", my_win_calls, closes ? "closes it" : "does not close it");
      if (closes) close();
    }
    fm_carry_advance(cy, FmCounts{c.N, c.M, c.A, 0, 0}, rows, true);
    trace.push_back(what);
    ++call;
    return sv.q_ok;
  }
};

// ---- known answers -------------------------------------------------------------------------------------------------------------------------------
static void known_answers() {
  {  // the threshold is strict, an already flagged stream keeps its retry, the list is [clean ascending | noisy ascending]
    FmRoute r;
    memset(&r, 0, sizeof(r));
    CHECK(fm_route_alloc(r, 6), "alloc");
    fm_route_reset(r);
    r.win_used[2] = true; r.win_stages = 64; r.win_calls = 16;
    const FmRouteClose cw = fm_route_close(r, false, false);
    CHECK(cw.set == 0 && r.set == 1 && r.rb_pending[0] && r.rb_stages[0] == 64 && cw.wait[2] == FM_ROUTE_WINDOW_EVENT && !cw.record[2] && cw.wait[0] == FM_ROUTE_NO_EVENT, "close");
    CHECK(fm_route_due(r) < 0, "set 1 has nothing under way");
    r.set = 0; r.calls = 100;
    CHECK(fm_route_due(r) == 0, "set 0 is due");
    r.noisy[5] = 1; r.retry_at[5] = 7777; r.next_retry = 7777;
    const uint32_t pass[6] = {16, 17, 0, 64, 15, 64};             // of 64 stages: exactly a quarter stays, one more goes
    fm_route_take(r, 0, pass);
    CHECK(!r.noisy[0] && r.noisy[1] && !r.noisy[2] && r.noisy[3] && !r.noisy[4] && r.noisy[5] && r.dirty && !r.rb_pending[0], "a quarter of the stages is not MORE than a quarter");
    CHECK(r.retry_at[1] == 100 + 1024 && r.retry_at[3] == 1124 && r.retry_at[5] == 7777 && r.next_retry == 1124, "%" PRIu64 " %" PRIu64, r.retry_at[1], r.next_retry);
    uint32_t list[6];
    const FmRouteCounts n = fm_route_list_fill(r, list);
    const uint32_t want[6] = {0, 2, 4, 1, 3, 5};
    CHECK(n.n_clean == 3 && n.n_noisy == 3 && !memcmp(list, want, sizeof(want)) && r.n_noisy == 0, "list");
    r.calls = 1123; fm_route_retry(r);
    CHECK(r.noisy[1] && r.noisy[3], "one call early");
    r.calls = 1124; fm_route_retry(r);
    CHECK(!r.noisy[1] && !r.noisy[3] && r.noisy[5] && r.next_retry == 7777, "the back-off is over at call retry_at");
    fm_route_free(r);
  }
  // 256 streams, 32 of them noise-only from call 0, every call design Q's (tests/test_route_gpu.py: up == 64, down within up + 1000 .. up + 1100, noisy again)
  for (int pattern = 0; pattern < 3; ++pattern)                  // all on the handle's stream; the two internal streams in turn; ... with a join after every call
    for (int a = 0; a < 3; ++a) {
      Sim sim(256, (Arrival)a, 7 + a, 8);
      std::vector<uint32_t> hist;
      for (int k = 0; k < 1200; ++k) {
        CHECK(sim.process(true, pattern > 0), "call %d is design Q's", k);
        if (pattern == 2) sim.flush_previous();
        hist.push_back(sim.flagged());
      }
      uint32_t up = 0, down = 0, again = 0;
      while (up < 1200 && hist[up] == 0) ++up;
      for (down = up; down < 1200 && hist[down] != 0; ++down) {}
      for (again = down; again < 1200 && hist[again] == 0; ++again) {}
      CHECK(up == 64 && hist[64] == 32 && down == 1088 && again == 1152 && hist[1199] == 32, "pattern %d arrival %d: up %u down %u again %u", pattern, a, up, down, again);
      for (uint32_t s = 0; s < 256; ++s) CHECK((sim.r.noisy[s] != 0) == (s % 8 == 1), "stream %u", s);
      CHECK(sim.close_call.size() == 75 && sim.close_call[0] == 15 && sim.close_call[68] == 1103 && sim.taken == 71, "window 68 closes at call %" PRIu64, sim.close_call[68]);
      // a host SETS - 1 windows ahead waits at every intake, one the device keeps up with never; no event record on either pattern but for the burst's
      // first call, which shares the handle's stream with no later one
      CHECK(sim.forced == (a == NEVER_UNASKED ? 71u : a == AT_ONCE ? 0u : sim.forced), "%u waits", sim.forced);
      CHECK(sim.records == (pattern ? 1u : 0u), "pattern %d: %u event records", pattern, sim.records);
    }
}

// ---- the sweep ---------------------------------------------------------------------------------------------------------------------------------------
struct Action { uint8_t kind; bool fit, ovl; uint64_t seed; };   // kind 0: a call; 1: sdrfm_flush_previous; 2: sdrfm_wait_previous; 3: sdrfm_reset; 4: the hook's mask
struct OvlState { bool bound[2], join_style; uint32_t next; };

static void play(Sim& sim, const std::vector<Action>& acts, size_t from, size_t* reset_at, OvlState* at_reset, size_t* trace_at_reset) {
  for (size_t i = from; i < acts.size(); ++i) {
    const Action& a = acts[i];
    if (a.kind == 0) sim.process(a.fit, a.ovl);
    else if (a.kind == 1) sim.flush_previous();
    else if (a.kind == 2) sim.wait_previous();
    else if (a.kind == 3) {
      sim.reset();
      if (reset_at) { *reset_at = i; *at_reset = OvlState{{sim.cy.ovl_bound[0], sim.cy.ovl_bound[1]}, sim.cy.ovl_join_style, sim.cy.ovl_next}; *trace_at_reset = sim.trace.size(); }
    } else {
      Rng m{a.seed};
      std::vector<uint8_t> mask(sim.ns);
      const uint32_t pct = m.in(0, 70);
      for (uint32_t s = 0; s < sim.ns; ++s) mask[s] = m.in(0, 99) < pct;
      sim.set_mask(mask);
    }
  }
}

static void one_case(uint64_t seed, bool long_run) {
  Rng rng{seed};
  const uint32_t ns = rng.one_in(4) ? rng.in(27, 40) : rng.in(41, 300);
  const uint32_t n_acts = long_run ? 1400 : rng.in(40, 420);
  const uint32_t p_unfit = rng.one_in(3) ? 0 : rng.in(1, 30), p_ovl = rng.in(0, 100), p_join = rng.one_in(2) ? 0 : rng.in(1, 100);
  std::vector<Action> acts;
  // one reset or mask anywhere, mid-window included (a long run: a mask over streams the statistics have flagged, with their back-off still to expire)
  const uint32_t special_at = long_run ? rng.in(80, 300) : rng.in(0, n_acts - 1), special = long_run ? (rng.one_in(2) ? 2 : 0) : rng.in(0, 3);
  for (uint32_t i = 0; i < n_acts; ++i) {
    if (i == special_at && special) acts.push_back(Action{(uint8_t)(special == 1 ? 3 : 4), false, false, rng.next()});
    acts.push_back(Action{0, rng.in(0, 99) >= p_unfit, rng.in(0, 99) < p_ovl, 0});
    if (rng.in(0, 99) < p_join) acts.push_back(Action{(uint8_t)(rng.one_in(5) ? 2 : 1), false, false, 0});
    if (!long_run && rng.one_in(300)) acts.push_back(Action{(uint8_t)(rng.one_in(2) ? 3 : 4), false, false, rng.next()});
  }
  // (a) the same bytes and calls give the same assignment, kernels and events at every call, whenever the read-backs arrive
  std::vector<uint64_t> first;
  size_t reset_at = 0, trace_at_reset = 0;
  OvlState ovl_at_reset = {{false, false}, false, 0};
  bool had_reset = false;
  for (int a = 0; a < 3; ++a) {
    Sim sim(ns, (Arrival)a, seed, 0);
    size_t ra = ~(size_t)0;
    play(sim, acts, 0, &ra, &ovl_at_reset, &trace_at_reset);
    if (a == 0) { first = sim.trace; reset_at = ra; had_reset = ra != ~(size_t)0; }
    else CHECK(sim.trace == first, "seed %" PRIu64 ": arrival %d gives another sequence", seed, a);
  }
  // (d) after a reset, nothing of the earlier windows reaches a later one: a handle that never saw them does the same from there on (the overlap's own
  // state, which a reset keeps, given to it)
  if (had_reset) {
    Sim sim(ns, AT_RANDOM, seed, 0);
    sim.cy.ovl_bound[0] = ovl_at_reset.bound[0]; sim.cy.ovl_bound[1] = ovl_at_reset.bound[1]; sim.cy.ovl_join_style = ovl_at_reset.join_style; sim.cy.ovl_next = ovl_at_reset.next;
    for (size_t i = 0; i <= reset_at; ++i) sim.epoch += acts[i].kind == 3;   // (the noise of the windows after THAT reset)
    play(sim, acts, reset_at + 1, nullptr, nullptr, nullptr);
    CHECK(sim.trace.size() + trace_at_reset == first.size() && std::equal(sim.trace.begin(), sim.trace.end(), first.begin() + (long)trace_at_reset),
          "seed %" PRIu64 ": the calls behind the reset at action %zu differ from a fresh handle's", seed, reset_at);
  }
}

int main() {
  known_answers();
  unsigned long cases = 0;
  for (uint64_t seed = 1; seed <= 400; ++seed, ++cases) one_case(0x5d2f3a11c0ffee01ull + seed, seed % 40 == 0);
  printf("sweep: seed 0x5d2f3a11c0ffee01, %lu sequences\n", cases);
  if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
  printf("ok\n");
  return 0;
}
