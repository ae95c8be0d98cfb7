// One detect on the host (bsa_cd.hip): its plan, its run state, and the
// launchers of the kernel units (bsa_k0.hip, bsa_prefilter.hip, bsa_rank.hip).
#pragma once
#include <algorithm>

#include "bsa_cd_args.h"
#include "bsa_sim_row.h"  // K24Args

namespace bsa {

static inline unsigned blocks_for(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

static inline SoA6 soa(const DevBuf *a) {
  return SoA6{(const double *)a[0].p, (const double *)a[1].p, (const double *)a[2].p,
              (const double *)a[3].p, (const double *)a[4].p, (const double *)a[5].p};
}

// ---- one detect: DetectPlan (every decision, taken by detect_decide from the
// DetectRequest and the context's state before the first stream operation),
// DetectRun (the request, the result and the device pointers the stages
// share), one function per stage, detect_enqueue runs them in order
struct DetectPlan {
  double rpz, hpz, tla;
  int flags;
  // -- detect shape
  int64_t n, rb, re, nrows;
  bool empty;  // n == 0 || nrows == 0: nothing below `timed` is decided
  bool distinct;
  // home mode (the resident sim, bsa_sim.hip): own[] is already in spatial
  // (home) order, h2id names the aircraft; the rows are the 512-aligned home
  // slice [rb, re) of the columns (no re-sort, no gather)
  bool home;
  // halo mode (home mode of the row-sharded step, or its one-GPU probe): K0
  // prepares the rank's own column tiles [a0, a1) (na of them), halo_mid plans
  // / exchanges the tiles its rows can reach, K0 prepares those from the list
  bool halo;
  int a0, a1, na;
  // home mode: K1b builds its fp64 records from the state arrays instead of
  // reading 128-B records K0b wrote for EVERY column: cheaper when K0b's
  // record writes dominate -- at 1M (0.165 -> 0.084 ms of K0) or for one rank's
  // slice of several; with one rank below 2^18 aircraft the stored records
  // win (each aircraft is in ~5 candidates there: K1b 27 -> 18 us at 100k).
  // BSA_HOME_REC=0/1 overrides.
  bool recs;
  // KWIK: stage 1 is exact-safe only with the pair's own mean latitude in
  // cavelat (own == intruder), and the CPA refine's geometry
  // is the great circle's: a distinct intruder set disables the prefilter,
  // and the refine keeps every stage-1 survivor.
  int kwik, noprune;
  // rows share the column order and records when own == intruder and the
  // whole range is detected; only then can the candidate list be reused
  bool shared;
  int64_t roff;  // the rows' offset in the shared records
  // -- reuse and rebuild decisions
  bool reuse;  // candidate-list reuse
  // stage 1 at the look-ahead midpoints: its bound is derived
  // for the great-circle geometry and fixed reaches, so not with KWIK nor with
  // the reuse budgets (whose drift checks assume t = 0 points); the
  // BSA_STAGE1_T0 environment variable selects t = 0 for A/B measurements
  int mid;
  // symmetric sweep: rows and columns are the same records
  // and every row is detected, so K0d lists each unordered tile pair once
  // (row tile <= column tile) and the sweep refines the stage-1 survivors of
  // an off-diagonal item in both orientations.  One rank, midpoint stage 1,
  // no KWIK / NOPRUNE / candidate reuse.  The level: 0 both orders, 1 as
  // above, 2 also the triangular sweep inside a diagonal tile pair (3.2d: a
  // slice skips the column sub-groups below its own and refines the ones above
  // both ways); the lower of bsa_set_symmetric_sweep's and BSA_PF_SYM's (A/B).
  // Part of the kept tile-pair list's key.
  int sym;
  // the resident step's K4' already wrote this detect's column records and
  // boxes from the state it computed (Ctx::prep; any detect consumes or
  // invalidates them: it rewrites the same buffers)
  bool prepped;
  // tile-pair list reuse: the resident step's detects of a
  // rank's rows -- one rank: records prepared (and checked) by K4'; several
  // ranks or the probe: the halo plan is kept with the list.  Any other detect
  // of this context invalidates the kept list.  Halo mode: K0d sweeps the
  // present column tiles only (tp_list: own + received, the flat halo list;
  // BSA_TP_HALO_ALL=1 sweeps all tiles for A/B).  tvalid: the kept list is
  // this shape's.
  bool tp_list, tpr, tvalid;
  // Who decides a rebuild.  HK (the resident step, Ctx::hk_*): the host, before
  // enqueuing -- a kept list (hkeep) then launches no K0d and, several ranks,
  // no box all-gather, no halo plan and one K0b for own + halo tiles.  Every
  // rank takes the same decision from the same inputs (the host-side
  // invalidations are collective events, the prediction is all-reduced with
  // the gate).  Otherwise the device: the records' preparers raise a flag, K0d
  // / the plan read it (round-5 behaviour).  hm: the HK detect's number.
  bool hk, hkeep;
  int64_t hm;
  // K0z skipped: the last detect's K2 (k_rank_rows) zeroed this detect's
  // counter block (double-buffered), dequeue words and per-row counts, and
  // writes inconf / tcpamax of every row itself; the prepped tile boxes are
  // derived from the group boxes by K0d (direct form only).  (HK keep, halo
  // mode: K2 zeroed this detect's counters too, or K0z runs as its own launch
  // -- not inside the merged K0b, whose halo workgroups write Counters)
  bool nozero;
  // stage events of this detect: only one detect in ev_every is timed (each
  // record costs a ~5 us bubble before the next kernel, bsa_set_timing_sample)
  bool timed;
  hipEvent_t *ev;
  unsigned long long nf_epoch;  // non-finite tcpa inputs: this detect's epoch (the prepped records carry K4''s)
  double kf;                    // k_keys midpoint factor
  // K0a spatial order.  Any permutation gives identical results (the output is
  // re-sorted canonically), so the order is reused for up to kResortEvery
  // calls on the same shape: aircraft move ~km between calls, tiles span ~100
  // km (with a reusable list: 64 calls, and every re-sort rebuilds the list).
  bool resort;
  // -- launch shape
  unsigned long long cap;  // candidate capacity
  // candidate-list reuse: the list of the last build stays valid for this
  // perm / parameters / buffers unless an aircraft overran its budget
  // (decided on the device by K0b; ctl[0] = build this detect)
  bool rvalid;
  // halo overlap (Ctx::ov_mode): a kept plan of several ranks (mode 2: also the
  // probe) sweeps the own column tiles on the stream while the exchange, the
  // received tiles' K0b and their sweep run on xstream
  bool ovl;
  // K1b fused into the prefilter (ExactFuse): stored records, row buckets, no
  // KWIK / candidate reuse, not one rank's share of a sharded step (there the
  // sweep is short and the workgroups' end-of-sweep evaluation lengthened it
  // more than K1b's launch cost: global1m rank 2 of 8, prefilter 46 + K1b 11
  // -> 63 us; box100k one rank: 0.1387-0.1396 -> 0.1336-0.1367 ms per step).
  // BSA_FUSE_EXACT=0/1 overrides (A/B).
  bool fuse;
  int B;  // K2 row buckets (B pairs per row per list; a fuller row retries wider, then without)
  int nrt, nct;
  long long ntp;
  int ngr, ngc, nsc;
  unsigned long long icap;  // items: 8 slices per tile pair
  // K1a prefilter: persistent grid, PF_BLOCKS_PER_CU workgroups per CU
  // (LDS-limited residency), at least one workgroup per dequeue shard
  unsigned pf_grid;
  PfKnobs kn;  // (ph, ca0, ca1: per launch)
  int diag;    // rows sharing the column records: row i is column roff + i (its diagonal), else -1
};

struct DetectRun {
  Ctx *c;
  const DetectPlan &p;
  const DetectRequest &q;
  DetectResult &res;
  SoA6 own, intr;
  Counters *dcnt;
  NfArgs nfa;
  ReuseParams rz{};
  const unsigned *build = nullptr;  // candidate reuse: its control words
  const unsigned *perm_c = nullptr, *perm_r = nullptr;
  const RowRec *rowrec = nullptr;
  const PFRec *pfrow = nullptr;
  const PFVel *pfvrow = nullptr;
  const float4 *pfprow = nullptr;
  const TileBox *gbox_r = nullptr, *tbox_r = nullptr;
  HaloTpr ht{};  // tile-pair list reuse: the halo plan's share (halo_mid may raise ht.force),
  TprArgs tp{};  // K0d's and the prefilter's
  // HK: the prediction word of this detect's records (raised by their
  // preparer -- K4' one step ago, or the own tiles' K0b here)
  unsigned long long *hk_word = nullptr;
  HeavyNext hn{};

  int mark(int e) const {
    if (p.timed) BSA_HIP(c, hipEventRecord(p.ev[e], c->stream));
    return 0;
  }
  // K0z: zero the per-detect state (launched once the reuse decision is known)
  // (k_zero, bsa_k0.hip)
  int zero(bool keep, unsigned *rctl, int rforce, bool tiles = false) const;
  // K0b's arguments that every launch of this detect shares
  PrepColsLaunch prep_cols() const {
    PrepColsLaunch a;
    a.n = (int)p.n;
    a.perm = perm_c;
    a.presorted = p.home ? 1 : 0;
    a.rec = p.recs ? 1 : 0;
    a.own = own;
    a.intr = intr;
    a.distinct = p.distinct ? 1 : 0;
    a.shared = p.shared ? 1 : 0;
    a.rpz = p.rpz;
    a.hpz = p.hpz;
    a.tla = p.tla;
    a.mid = p.mid;
    a.rz = rz;
    a.nf = nfa;
    a.zs.nrows = (int)p.nrows;
    return a;
  }
};

// ---- the launchers (each next to its kernel): the arguments come from the
// DetectRun, a stage function states what it decides.  They were file-local
// before the units were split: hidden, so the library exports what it did.
#pragma GCC visibility push(hidden)
// K0 (bsa_k0.hip)
int spatial_order(Ctx *c, int cnt, int base, const double *lat, const double *lon, const double *trk,
                  const double *gs, double f, DevBuf &key, DevBuf &idx, DevBuf &key2, DevBuf &perm);
int launch_prep_cols(Ctx *c, hipStream_t stream, unsigned grid, const PrepColsLaunch &a);
int launch_prep_rows(const DetectRun &R);
int launch_boxes(const DetectRun &R, bool cols);  // the rows' boxes, or the columns' (a reused candidate list)
int launch_tilepairs_direct(const DetectRun &R);
int launch_tilepairs(const DetectRun &R);
// K1a (bsa_prefilter.hip); pf_trace_arm: a no-op unless built with -DBSA_PF_TRACE
int launch_prefilter(const DetectRun &R, hipStream_t stream, unsigned grid, const PrefilterLaunch &a);
int pf_trace_arm(Ctx *c);
// K1b / K2 (bsa_rank.hip)
int launch_exact(const DetectRun &R, unsigned grid);
int launch_scatter(const DetectRun &R);
int launch_rowblk(const DetectRun &R, bool heavy);  // heavy: with the next detect's item listing (R.hn)
int launch_rank(const DetectRun &R, const MvpFuse &mf);
int rank_launch(Ctx *c, const RankLaunch &a, bool k24, const K24Args &ka);
#pragma GCC visibility pop

}  // namespace bsa
