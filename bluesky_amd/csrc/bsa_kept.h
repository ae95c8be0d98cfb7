// What a detect keeps from earlier calls, and every event that drops it
// (DESIGN.md 3.24).  Host only: nothing of HIP in here.
//
// Each kept state is a `valid` flag and the key it was made for.  A detect asks
// matches(key), re-arms with keep(key) and consumes with drop(); everything
// outside a detect goes through invalidate(c, Change) (bsa_internal.h), which
// reads kDrops below.  Configuration (reuse_on, the budgets, hk_on ...), the
// statistics and the device buffers stay in Ctx beside these.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace bsa {

// K0a's spatial order (Ctx::perm_r / perm_c) of a detect in aircraft-index
// order.  Any permutation gives identical results; `age` (detects since the
// sort) is the caller's re-sort rule, not part of the match.  Fields: ==
struct KeptOrder {
  struct Key {
    int64_t n, rb, re;
    bool shared, distinct;
    double f;  // midpoint factor the order was computed with (k_keys)
  };
  bool valid = false;
  Key key{};
  int64_t age = 0;
  bool matches(const Key &k) const {
    return valid && key.n == k.n && key.rb == k.rb && key.re == k.re && key.shared == k.shared &&
           key.distinct == k.distinct && key.f == k.f;
  }
  void keep(const Key &k) {
    valid = true;
    key = k;
    age = 0;
  }
  void drop() { valid = false; }
};

// The reusable candidate list and its snapshot (shared own == intruder, all
// rows).  The four parameters are compared as bytes (a NaN equals itself, +0
// differs from -0); the list's capacity and device buffer are part of the key
struct KeptCands {
  struct Key {
    double rpz, hpz, tla, flags;
    int64_t n;
    unsigned long long cap;
    const void *list;
  };
  bool valid = false;
  Key key{0, 0, 0, 0, -1, 0, nullptr};
  bool matches(const Key &k) const {
    return valid && key.n == k.n && key.cap == k.cap && key.list == k.list &&
           memcmp(&key, &k, offsetof(Key, n)) == 0;
  }
  void keep(const Key &k) {
    valid = true;
    key = k;
  }
  void drop() { valid = false; }
};

// K0d's tile-pair list with its record snapshot and, in halo mode, the halo
// plan kept with it.  The seven parameters are compared as
// bytes.  sym: the list holds each unordered tile pair once, its off-diagonal
// items flagged mirrored (DetectPlan::sym) -- a list is only
// ever swept by a detect whose plan took the same choice
struct KeptTilePairs {
  struct Key {
    double rpz, hpz, tla, mid, rb, re, sym;
    int64_t n;
  };
  bool valid = false;
  Key key{0, 0, 0, 0, 0, 0, 0, -1};
  bool matches(const Key &k) const { return valid && key.n == k.n && memcmp(&key, &k, offsetof(Key, n)) == 0; }
  bool kept_for(int64_t n) const { return valid && key.n == n; }  // K4' checks its records against this list's budgets
  void keep(const Key &k) {
    valid = true;
    key = k;
  }
  void drop() { valid = false; }
};

// The column records and boxes the last K4' wrote for the next detect (one
// rank).  Any detect consumes them: it rewrites the same buffers.  Fields: ==
struct KeptPrep {
  struct Key {
    double rpz, hpz, tla, mid;
    int64_t n;
  };
  bool valid = false;
  Key key{};
  bool matches(const Key &k) const {
    return valid && key.rpz == k.rpz && key.hpz == k.hpz && key.tla == k.tla && key.mid == k.mid && key.n == k.n;
  }
  void keep(const Key &k) {
    valid = true;
    key = k;
  }
  void drop() { valid = false; }
};

// The last detect's K2 zeroed the next detect's counters, dequeue words
// (counters2 / workq2) and row counts, for a detect of as many rows
struct KeptZero {
  struct Key {
    int64_t rows;
  };
  bool valid = false;
  Key key{};
  bool matches(const Key &k) const { return valid && key.rows == k.rows; }
  void keep(const Key &k) {
    valid = true;
    key = k;
  }
  void drop() { valid = false; }
};

// HK: the build decisions of the last host-decided detects.
// No key: the history is this sim's while nothing dropped it.  `m` numbers the
// host-decided detects of the context and only grows; `cool` counts the
// device-decided detects left after a stale abort (set beside invalidate)
struct HkHistory {
  bool valid = false;
  bool built[4] = {false, false, false, false};  // decisions of detects m & 3
  int64_t m = 0;
  int64_t cool = 0;
  bool matches() const { return valid; }
  bool built_lately(int64_t hm) const { return built[(hm + 3) & 3] || built[(hm + 2) & 3]; }
  void keep(int64_t hm, bool build) {
    valid = true;
    built[hm & 3] = build;
  }
  void drop() { valid = false; }
};

// ---- what happens outside a detect (and at its end), and what each drops
enum class Change {
  NewState,           // bsa_set_state
  NewSim,             // bsa_sim_init (after its bsa_set_state)
  EditedArrays,       // bsa_sim_update, no CD input among the arrays
  EditedCdInput,      // bsa_sim_update with lat lon alt tas hdg vs gs trk gseast gsnorth
  SimParams,          // bsa_sim_set_params
  OtherRows,          // bsa_sim_probe_rank
  Traffic,            // bsa_sim_create / bsa_sim_delete (set_n)
  BatchAborted,       // batch_rollback
  BatchStopped,       // batch_stopped: a stage ended the batch after a completed step
  StepNotEnqueued,    // step_enqueue: its CD call failed
  DetectNotEnqueued,  // detect_enqueue: its first event record failed
  DetectDone,         // detect_finish
  DetectOverflow,     // detect_finish: the candidate list overflowed
  SetCandReuse,       // bsa_set_candidate_reuse
  SetTileReuse,       // bsa_set_tile_reuse
  SetHk,              // bsa_set_hk
  SetSymSweep,        // bsa_set_symmetric_sweep
  WindField,          // bsa_set_windfield3d
  Turbulence,         // bsa_sim_set_turbulence: on / off, sd, seed
  Adsb,               // bsa_sim_set_adsb: on / off and every setting
  RouteEdit,          // bsa_sim_route_edit
  Count
};
struct Drops {
  bool order, cands, tiles, prep, zero, hk;
};
constexpr bool drop = true, stays = false;
// Why a cell may stay while its row drops others (the full text: DESIGN.md 3.24):
//  (p) any permutation is correct; the key holds n and the rows; home-order detects use none
//  (d) K0b checks every aircraft against the list's snapshot on the device; a detect that cannot
//      reuse (rows, halo, flags) drops the list itself
//  (k) the key holds what changed
//  (i) the list does not depend on it
//  (z) only a detect with prepared records or a kept list skips K0z, and the row drops both
//  (b) a detect without a matching list builds whatever the history says
//  (c) the detect consumed or re-armed it before it was enqueued
//  (s) only the dropped state reads that setting
//  (w) the wind moves aircraft only through K4'; every kept state bounds drift by the records K4' or the
//      next detect actually writes, against its snapshot, whatever wind produced them -- no state reads the field
//  (t) turbulence moves aircraft after K4', so K4' prepares no records while it is on (StepPlan::prep) and every
//      detect makes its own from the perturbed state with K0b: on one rank no list is kept then (a kept list needs
//      prepared records), on several the own-tile K0b checks every record against the list's snapshot.  Switching
//      it on, off or to other sd / seed drops what was made under the other setting's drift: the prepared
//      records' budget check and HK's predictions assumed it
//  (a) the ADS-B stage reads the traffic state and writes only its own picture and lastupdate arrays, which no detect
//      reads (the step's detect takes the true state as intruder): nothing kept depends on it or on its settings
//  (r) a route edit writes the route table and the FMS arrays (actwp.*, iactwp, swlnav, selspd, ap.alt): guidance
//      targets only, no position or velocity, and no detect reads any of them; the aircraft move under the new
//      targets only through K4', whose records (or the next detect's) every kept state checks against its snapshot
//  (n) the steps enqueued behind the stop became no-ops, but their detects ran -- on the state the stop left, with
//      the host's later decisions: they re-armed the candidate list, the tile-pair list and its snapshot, the zeroed
//      counters and the HK history for steps that never happened, and K4' prepared no records for them.  All of it
//      is over the right state, but the host-side keys (HK's m, the prepared flag, which K2 zeroed what) describe
//      steps the clocks are rolled back over, so everything BatchAborted drops goes; a firing is rare, the next
//      detect rebuilds
//  (?) unexplained
constexpr Drops kDrops[(int)Change::Count] = {
    //                      order  cands  tiles  prep   zero   hk
    /* NewState          */ {stays, stays, drop, drop, stays, stays},   // p d . . z b
    /* NewSim            */ {stays, stays, drop, drop, stays, drop},    // p d . . z .
    /* EditedArrays      */ {stays, stays, drop, drop, stays, stays},   // p i . . z b
    /* EditedCdInput     */ {stays, drop, drop, drop, stays, stays},    // p . . . z b
    /* SimParams         */ {stays, stays, drop, drop, stays, stays},   // p k . . z b
    /* OtherRows         */ {stays, stays, drop, drop, stays, stays},   // p d . . z b
    /* Traffic           */ {drop, drop, drop, drop, stays, stays},     // . . . . z b
    /* BatchAborted      */ {stays, drop, drop, drop, drop, drop},      // p . . . . .
    /* BatchStopped      */ {stays, drop, drop, drop, drop, drop},      // p n n n n n
    /* StepNotEnqueued   */ {stays, stays, stays, stays, stays, drop},  // p ? ? ? ? .
    /* DetectNotEnqueued */ {stays, drop, stays, stays, stays, stays},  // p . ? c c ?
    /* DetectDone        */ {stays, stays, stays, stays, drop, stays},  // c c c c . c
    /* DetectOverflow    */ {stays, drop, stays, stays, drop, stays},   // c . i c . c
    /* SetCandReuse      */ {stays, drop, stays, stays, stays, stays},  // p . s s s s
    /* SetTileReuse      */ {stays, stays, drop, stays, stays, stays},  // p s . s s b
    /* SetHk             */ {stays, stays, stays, stays, stays, drop},  // p s s s s .
    /* SetSymSweep       */ {stays, stays, drop, stays, stays, stays},  // p i . i i b
    /* WindField         */ {stays, stays, stays, stays, stays, stays}, // w w w w w w
    /* Turbulence        */ {stays, drop, drop, drop, stays, drop},     // p t t t z t
    /* Adsb              */ {stays, stays, stays, stays, stays, stays}, // a a a a a a
    /* RouteEdit         */ {stays, stays, stays, stays, stays, stays}, // r r r r r r
};

}  // namespace bsa
