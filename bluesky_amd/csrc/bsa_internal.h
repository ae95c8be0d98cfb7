// Internal runtime of libbsaccel: context, device buffers, error plumbing.
// gfx950 (MI355X) only; compiled with -ffp-contract=off so every fp64
// expression rounds exactly like numpy's (one rounding per operation).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bsaccel.h"
#include "bsa_kept.h"

namespace bsa {

// ---------------------------------------------------------------- constants
// bluesky/tools/aero.py:11-28, bluesky/tools/geo.py:7,38-39
constexpr double kNM = 1852.0;
constexpr double kFT = 0.3048;
constexpr double kKTS = 0.514444;
constexpr double kWGS84_A = 6378137.0;
constexpr double kWGS84_B = 6356752.314245;
constexpr double kPI = 3.14159265358979323846;  // NPY_PI
constexpr double kD2R = kPI / 180.0;            // numpy deg2rad / radians factor
constexpr double kR2D = 180.0 / kPI;            // numpy rad2deg / degrees factor

// ---------------------------------------------------------------- records
// Per-index fp64 records gathered by the exact pair kernel (128 B = one
// cache line each).  Orientation follows StateBasedCD.py: for pair (i, j)
// the geometry row is ownship i and the column is intruder j, while the
// velocity / altitude differences are own[j] - intruder[i]
// (StateBasedCD.py:39-40,65-69).  So the ROW record i carries own[i]'s
// position and intruder[i]'s velocity; the COLUMN record j carries
// intruder[j]'s position and own[j]'s velocity.
struct alignas(16) RowRec {
  double lat, lon;        // own[i] [deg]
  double sinlat, coslat;  // sin/cos(radians(own.lat[i]))          geo.py:137-140
  double hemA;            // |lat| * (rwgs84(lat) + a)              geo.py:127
  double u, v;            // int.gs[i] * sin/cos(radians(int.trk[i]))  StateBasedCD.py:35-37
  double alt, vs;         // int.alt[i], int.vs[i]
  double pad0;
  double ilat;            // int.lat[i]  (KWIK cavelat, geo.py:355; same offset as ColRec::olat)
  double pad[5];
};
struct alignas(16) ColRec {
  double lat, lon;        // int[j]
  double sinlat, coslat;
  double hemA;
  double u, v;            // own.gs[j] * sin/cos(radians(own.trk[j]))  StateBasedCD.py:30-32
  double alt, vs;         // own.alt[j], own.vs[j]
  double eps;             // (own.lat[j] == 0.) * 1e-6                geo.py:128
  double olat;            // own.lat[j]  (KWIK cavelat, geo.py:355)
  double pad[5];
};
static_assert(sizeof(RowRec) == 128, "RowRec must be one cache line");
static_assert(sizeof(ColRec) == 128, "ColRec must be one cache line");

// fp32 prefilter record (32 B), one per sorted row / column.
// Stage 1 keeps a pair iff |x_i - x_j| < s_i + s_j (tested in a plane, see
// k_prefilter) and lo_j < hi_i and hi_j > lo_i (<=> |a_j - a_i| < h_i + h_j).
// x / a are the position / altitude at t = 0, or (midpoint mode, DESIGN.md
// 3.2b) at t = tla/2 along the velocity, with the reaches to match.
struct alignas(16) PFRec {
  float x, y, z;   // stage-1 point (unit-sphere units)
  float s;         // horizontal reach, chord units (half of the pair bound); INF = always
  float lo, hi;    // a -/+ h, h = vertical reach [m] (half of the pair bound)
  float alt;       // altitude [m] at t = 0 (refine)
  float pad;
};
// The refine's position (PFPos, float4 x y z 0): the unit vector at t = 0.
static_assert(sizeof(PFRec) == 32, "PFRec must be 32 B");

// velocity part, read only by the CPA refine (rows and columns)
struct alignas(16) PFVel {
  float u, v;      // east / north velocity [m/s] (orientation as RowRec / ColRec)
  float vs;        // vertical speed [m/s]
  unsigned flags;  // bit 0: never refine this index (unbounded radius quirk / non-finite
                   //        / tangent basis ill-conditioned near a pole)
};
static_assert(sizeof(PFVel) == 16, "PFVel must be 16 B");

// Candidate-list reuse (BSA reuse mode): state of one
// aircraft (sorted position) when the candidate list was last built, and its
// vertical budget [m].  The unit vector and velocity are fp64.
struct alignas(16) Snap {
  double x, y, z;   // unit position vector
  double u, v;      // gs * sin / cos(trk)
  double alt, vs;
  float sv;         // vertical budget of this build [m]
  float pad;
};
static_assert(sizeof(Snap) == 64, "Snap must be 64 B");

// axis-aligned bounds of a group / tile of sorted PFRecs (culling)
struct alignas(16) TileBox {
  float lo[3], hi[3];   // unit-vector bounds
  float vlo, vhi;       // min lo, max hi (vertical reach intervals)
  float smax, pad0;
  int count, pad1;
};
static_assert(sizeof(TileBox) == 48, "TileBox must be 48 B");

constexpr int kTile = 512;  // rows per row block == columns per column tile
constexpr int kResortEvery = 8;  // detect calls between spatial re-sorts
constexpr int kResortEveryReuse = 64;  // ... with a reusable candidate list (a re-sort rebuilds it)
constexpr int kEvSets = 4096;    // detect timing event sets kept between resets

#ifndef BSA_CAND_SHARDS
#define BSA_CAND_SHARDS 8
#endif
constexpr int kCandShards = BSA_CAND_SHARDS;  // candidate list shards (one counter each, 128 B apart)
constexpr unsigned kDangling = 0xffffffffu;  // resopairs column of a deleted intruder (sorts last in a row)
// gate[0] of the resident step (all-reduced max over ranks): 0 nothing, 1 a
// non-finite tcpa input in some rank's columns (every row's tcpamax is NaN),
// >= 2 abort the step (2 candidate / row-bucket overflow, 3 resopairs overflow)
constexpr unsigned long long kGateNonfinite = 1, kGateOverflow = 2, kGateBkOverflow = 3;
// gate[2]: the HK prediction of this CD call (some rank's records left kHkPredict of their budgets)
constexpr int kGateWords = 3;
constexpr int kSimCtlSticky = 24, kSimCtlSteps = 32, kSimCtlDemand = 40, kSimCtlKdemand = 48, kSimCtlStale = 56;
constexpr int kSimCtlPend = 64;  // one u64 per StopStage; [24, kSimCtlEnd) are zeroed per batch and read back after it
// The sticky word's values: 0 the batch runs; kStickyAborted the step that raised it did not happen (the state is
// its start: grow, re-run); kStickyStopped the step that raised it is complete and the host has to act before the
// next one (nothing to re-run).  A stop is raised only while the word is 0, by a stage behind the step's steps_done
// increment, together with [28, 32): stop_word(stage, tag) -- which stage raised it first and the raising step's
// tag (its number in the batch + 1, < 2^24).  That word, not the sticky value, tells the host the batch stopped: a
// detect of a later, no-op step may still overflow and store kStickyAborted over the stop.  Every stopping stage
// with something for the host stores its step's tag into its pending word (kSimCtlPend + 8 stage), raiser or not:
// batch_stopped hands the stop to each stage whose word holds the stop's tag (bsa_stop.h)
constexpr unsigned kStickyAborted = 1u, kStickyStopped = 2u;
enum StopStage : unsigned { kStopNone = 0, kStopCond = 1, kStopArea = 2, kStopCount };  // (conditions; the experiment area)
constexpr unsigned kStopTagMax = (1u << 24) - 1;
constexpr unsigned stop_word(unsigned stage, unsigned tag) { return (stage << 24) | tag; }
constexpr unsigned stop_stage(unsigned w) { return w >> 24; }
constexpr unsigned stop_tag(unsigned w) { return w & kStopTagMax; }
constexpr int kSimCtlEnd = kSimCtlPend + 8 * (int)kStopCount;
// behind the per-batch words, never zeroed by a batch: the trail stage's running total of undrained segments and
// its demand word (u32 each; bsa_trails.hip), read back with the batch's words
constexpr int kSimCtlTrail = kSimCtlEnd, kSimCtlAll = kSimCtlTrail + 8;
// sim_ctl's per-batch words as batch_end hands them back
struct BatchCtl {
  unsigned sticky, stop;  // kSticky*; stop_word(stage, tag) of the first raiser, 0: no stop
  unsigned long long steps_done, bk_demand, key_demand, stale, pend[kStopCount];
};
static_assert(offsetof(BatchCtl, stop) == 4 && offsetof(BatchCtl, steps_done) == kSimCtlSteps - kSimCtlSticky &&
                  offsetof(BatchCtl, bk_demand) == kSimCtlDemand - kSimCtlSticky &&
                  offsetof(BatchCtl, key_demand) == kSimCtlKdemand - kSimCtlSticky &&
                  offsetof(BatchCtl, stale) == kSimCtlStale - kSimCtlSticky &&
                  offsetof(BatchCtl, pend) == kSimCtlPend - kSimCtlSticky && sizeof(BatchCtl) == kSimCtlEnd - kSimCtlSticky,
              "BatchCtl mirrors sim_ctl from kSimCtlSticky on");
// a stopping stage's host side: a stop nobody polled yet, and its step count
struct StopSide {
  bool pending = false;
  int64_t step = 0;
};
constexpr int kHkRing = 16;  // HK: published predictions (pinned host words), slot m % kHkRing
constexpr unsigned long long kNanBits = 0x7ff8000000000000ull;  // (a quiet NaN)

// HK publication (Ctx::hk_*): lane 0 of block 0 of a CD step's K4' (or of the
// fused K2 + K4') stores base | prediction (bit 0) | aborted (bit 1) into the
// ring slot of the detect, in pinned host memory the host polls (a vector
// store, system scope; written before any early return of the kernel)
struct HkPub {
  unsigned long long *slot;  // device view of hk_host[m % kHkRing], or NULL (no publication)
  unsigned long long base;   // (m + 1) << 2
  unsigned long long *src;   // the prediction word (gate[2] after the all-reduce, or the rank's own word)
  int zero;                  // zero *src once read (the rank's own word: its next user is two detects on)
};
// (relaxed: the host reads this one word; a release at system scope would
// write back the whole L2 first -- buffer_wbl2 -- under the other waves' feet)
template <typename Aborted>
__device__ __forceinline__ void hk_publish(const HkPub &p, Aborted aborted) {
  if (!p.slot) return;
  const unsigned long long v = p.base | (p.src && *p.src ? 1ull : 0ull) | (aborted() ? 2ull : 0ull);
  if (p.zero && p.src) *p.src = 0ull;
  __hip_atomic_store(p.slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// counters block on the device
constexpr int kFuseRecsMax = 64;  // fused K1b: mid-sweep flush records per prefilter wave (LDS)

struct Counters {
  unsigned long long cand;    // host-side total (sum of the shard counts)
  unsigned long long conf;
  unsigned long long los;
  unsigned long long tiles;
  unsigned long long groups;  // (64-row x 8-column) blocks swept by the prefilter
  unsigned long long tiles_near;  // of `tiles`: pairs whose boxes overlap (listed first, swept first)
  unsigned long long tpr_stale;   // a host-kept tile-pair list (HK) whose records left their budgets: re-run
  unsigned long long k2_demand;   // K2 row buckets: the largest row count beyond Ctx::k2_bucket (0: fit)
  unsigned long long halo_ovf;    // halo exchange: more tiles to send / receive than the capacities
  unsigned long long halo_miss;   // halo exchange inconsistent (a kept tile pair without its data): bug
  unsigned long long fuse_ovf;    // fused K1b: a wave flushed more blocks than it can record (retry unfused)
  // diagnostic builds only (-DBSA_PF_STAMPS): prefilter s_memtime cycles per phase
  unsigned long long stamp[8];
  unsigned long long cshard[kCandShards][16];  // candidates per shard (word 0 of each line)
  unsigned long long gpart[32][16];  // sub-groups swept, per prefilter workgroup shard (summed into groups by K2)
  // the exact evaluation counted a conflict (plain stores of 1, one per wave): the lean K2 + K4' gates MVP with it
  // (asas.py:486-487) where the full form has P, the sum.  Last, so that no other word moves
  unsigned long long any_conf;
};

// ---------------------------------------------------------------- buffers
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
};

struct Ctx;
bool ensure(Ctx *c, DevBuf &b, size_t bytes, const char *what);
// Pinned host staging (bsa_ctx.hip): host_copy copies its jobs with a small
// thread pool (chunks of 256 KiB; small totals on the calling thread);
// pin_stage returns the context's pinned buffer of >= bytes once no DMA from
// it is pending; pin_issued marks a DMA from it just enqueued on c->stream.
struct HostCopy {
  void *dst;
  const void *src;
  size_t bytes;
};
void host_copy(const HostCopy *jobs, int n);
constexpr int kGatherMax = 12;
struct GatherParts {
  const unsigned *src[kGatherMax];
  unsigned long long woff[kGatherMax + 1];
  unsigned long long wlen[kGatherMax];
  int n;
};
__global__ void k_gather_words(GatherParts g, unsigned *__restrict__ dst);
unsigned char *pin_stage(Ctx *c, size_t bytes);
int pin_issued(Ctx *c);
bool ensure_keep(Ctx *c, DevBuf &b, size_t bytes, const char *what);  // grows, keeps contents
void release(DevBuf &b);

// The host clocks of the resident step: everything the host counts per enqueued step, as one
// value.  step_advance (bsa_sim.hip) is the one function that moves them over a step, after the step is
// enqueued; a batch saves them with one assignment and replays them with the same function.  Each stage reads
// its own clock, its _off resets it
struct StepClocks {
  int64_t steps = 0, cd_calls = 0;         // completed steps; CD calls (bsa_sim_cd's among them)
  double fms_simt = 0.0, fms_t0 = -999.0;  // FMS: the simt of the next step, Autopilot.t0,
  int64_t fms_ticks = 0;                   // ... the ticks of completed steps
  int64_t turb_call = 0;                   // turbulence (3.25): the call number of the next step's draws
  int64_t sect_ctr = 0;                    // sectors (3.27): steps since bsa_sim_set_sectors
  int64_t gv_ctr = 0;                      // geovectors (3.28): steps completed since bsa_sim_set_geovectors
  int64_t area_ctr = 0;                    // experiment area (3.30): steps since bsa_sim_set_exparea
  double trail_simt = 0.0, trail_last = 0.0;  // trails (3.31): the simt the next step's traf.update is called with,
                                              // ... and the one the last step's was
  double adsb_simt = 0.0;                  // ADS-B (3.32): the simt the next step's adsb.update is called with,
  int64_t adsb_call = 0;                   // ... the call number of its draws (+ 1 per step with noise on),
  int adsb_cur = 0;                        // ... and which lastupdate buffer it reads (it writes the other)
  int64_t lean_cd = 0, full_cd = 0;        // CD steps whose K2 ran lean (StepPlan::lean) / placed its pair lists
};

struct Ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  // state
  int64_t n = 0;
  bool has_intruder = false;
  DevBuf own[6];   // lat lon trk gs alt vs
  DevBuf intr[6];
  DevBuf rowrec, colrec, pfrow, pfcol, pfvrow, pfvcol, pfprow, pfpcol;
  // spatial order: Morton keys and the sorted-position -> original-index maps
  DevBuf key_r, idx_r, key_r2, perm_r, key_c, idx_c, key_c2, perm_c;
  DevBuf tbox_r, tbox_c, gbox_r, gbox_c, sbox_c, tilepairs, workq;
  DevBuf rowcnt, rowoff;         // K2 counting sort
  DevBuf kbuck;                  // K2 row buckets (column indices)
  int k2_bucket = 8;             // bucket width (pairs per row); 0 = scatter into row segments
  DevBuf scan_ws;                // single-pass scan: [0] ticket counter, then tile status words
  bool scan_ready = false;
  unsigned long long scan_tickets = 0;
  unsigned scan_epoch = 0;
  DevBuf scan_stage;             // bsa_scan_excl / bsa_flagged_list's arrays (the tests' entries)
  // what a detect keeps from earlier calls (bsa_kept.h); dropped through invalidate() below
  KeptOrder order;
  KeptCands cands;
  KeptTilePairs tiles;
  KeptPrep prep;
  KeptZero zero;
  HkHistory hk;

  // detect buffers
  DevBuf counters;           // Counters
  DevBuf counters2, workq2;  // the next detect's counters / dequeue words (double-buffered, zeroed by K2: Ctx::zero)
  DevBuf cand;               // uint2 (i, j)
  DevBuf cflag;              // per candidate: bit0 conflict, bit1 LoS
  unsigned long long cand_cap = 0;
  DevBuf ckey, cval, ckey2, cval2;  // conflict keys / slot ids (+ sorted)
  DevBuf cpay;               // 5 x cap doubles: qdr dist tcpa tin dcpa (slot order)
  unsigned long long conf_cap = 0;
  DevBuf lkey, lkey2;        // LoS keys (+ sorted)
  unsigned long long los_cap = 0;
  DevBuf out_ci, out_cj, out_li, out_lj;  // int32 sorted
  DevBuf out_pay;            // 5 x n_conf doubles, sorted
  DevBuf inconf, tcpamax;    // per row of the last detect
  DevBuf sort_tmp;

  // last detect
  int64_t last_rb = 0, last_re = 0;
  int64_t last_conf = 0, last_los = 0, last_cand = 0, last_tiles = 0, last_tiles_total = 0,
          last_groups = 0;
  int last_flags = 0;
  bool have_pairs = false;

  // candidate-list reuse across detects (shared own == intruder only)
  bool reuse_on = false;
  double reuse_sh = 800.0, reuse_sv = 60.0;   // horizontal budget, default / max vertical budget [m]
  DevBuf snap_build, snap_cur, reuse_ctl, reuse_use;  // ctl: [0] build flag, [1] detects since build

  // tile-pair list reuse: K0d's item list, built on boxes
  // inflated by (tpr_dx chord, tpr_ds reach, tpr_dv m), is kept while every
  // aircraft's prefilter record stays within those distances of its record at
  // the build (checked by whoever prepares the records: K4' / K0b); a record
  // outside raises tpr_ctl[0] and the next detect rebuilds on the device
  bool tpr_on = true;                  // resident home-order detects of all rows (BSA_TPR=0: off)
  float tpr_dx = 3.2e-4f, tpr_ds = 1.6e-5f, tpr_dv = 300.f;  // ~2 km, ~100 m of reach, 300 m
  DevBuf tpr_snap;                     // PFRec per aircraft at the last build
  DevBuf tpr_ctl;                      // u64: [0] build flag, [1] near items, [2] far items, [3] builds, [4] detects,
                                       // [5] the probe's rebuild flag, [6 + (m & 1)] HK prediction of detect m
  // Host-known list decisions (HK, round 6): in the resident
  // step the host decides build / keep BEFORE it enqueues a detect, so a kept
  // list launches no K0d (and, several ranks, no box all-gather, no halo plan
  // and one K0b for own + halo tiles).  Detect m keeps when neither m-1 nor
  // m-2 built and the device's prediction for m -- the records of detect m-2
  // within kHkPredict of every budget, over all ranks -- says so; the step's
  // K4' publishes that prediction into a pinned host ring (hk_host), so the
  // host waits at most for the work of the step before.  The kept detect still
  // checks every record against the full budgets: one outside aborts the step
  // (Counters::tpr_stale) and it re-runs with a build.
  bool hk_on = true;                   // BSA_HK=0: the device decides (round-5 behaviour)
  int64_t hk_cool_len = 32;            // device-decided detects after the next stale abort (doubles per
                                       // abort, <= 4096): a workload whose lists go stale often ends up device-decided
  int64_t hk_keeps = 0, hk_builds = 0, hk_stale = 0, hk_waits = 0;  // statistics
  float hk_f = 0.75f;                  // prediction fraction of the budgets (BSA_HK_F)
  unsigned long long *hk_host = nullptr, *hk_hdev = nullptr;  // pinned ring (host / device view)
  // longest items first (bsa_cd_args.h HeavyArgs): per list slot cost / flag, two item lists and counts
  DevBuf hv_cost, hv_flag, hv_list[4], hv_cnt;  // lists: [parity][tier]
  unsigned long long hv_icap = 0;
  unsigned hv_epoch = 0;
  double hv_us = 16.0;                 // listing threshold [us] per item (BSA_PF_HEAVY_US at bsa_create; < 0: off)
  bool hv_us_env = false;              // ... set by BSA_PF_HEAVY_US (else halved for a rank's share, bsa_cd.hip)
  double hv_x = 3.0;                   // ... x this: the top tier, twice the pieces (BSA_PF_HEAVY_X; <= 0: one tier)
  // halo overlap (round 6): on a kept-plan detect of several
  // ranks the halo send / recv, the halo K0b and the sweep of the halo column
  // tiles run on xstream while the own tiles' K0b and sweep run on `stream`;
  // joined by ov_ev[2] before K1b.  ov_mode: 1 exchange mode only (default),
  // 2 also the one-GPU probe (its cost without an exchange to hide), 0 off
  // (BSA_HALO_OVERLAP at bsa_create).  Off by default: on one GPU the split
  // costs ~17 us per step (probe, no exchange to hide: two sweeps' ramps and
  // tails + cross-stream event waits of ~5-10 us each), more than the ~30 us
  // exchange it could hide would repay only on the 8-GPU node
  int ov_mode = 0;
  hipStream_t xstream = nullptr;
  hipEvent_t ov_ev[3] = {nullptr, nullptr, nullptr};  // packed / own tiles prepared / halo sweep done
  int64_t ov_count = 0;                // overlapped detects (statistics)
  // (device-scope events: the join's wait 13 -> 10 us, the step 0.136 -> 0.134 ms; BSA_OV_EVFLAGS, A/B)
  unsigned ov_evflags = hipEventDisableTiming | hipEventDisableSystemFence;

  // detect timing: one set of 5 events per detect since the last reset
  std::vector<hipEvent_t> evpool;
  int ev_sets = 0, ev_last = 0;
  int ev_every = 1;       // time one detect in ev_every (0 = none), bsa_set_timing_sample
  int64_t ev_count = 0;   // detects since the last bsa_timing_reset
  bool ev_valid = false;
  bool empty_detect = false;
  DevBuf stats;  // accumulated per-detect statistics {groups, candidates, tiles, detects, list builds}
  void *trace_buf = nullptr;  // diagnostic builds (-DBSA_PF_TRACE): prefilter item timeline
  size_t trace_bytes = 0;

  // MVP / kinematics staging (host-buffer entry points)
  DevBuf seg, mvp_stage, kin_stage, mvp_pdv, mvp_pfl, mvp_rowdv;
  DevBuf xfer_stage;  // batched home-order transfers (bsa_xfer.hip: HomeBatch), index-order staging
  // pinned host staging of the drop-ins' transfers (pin_stage, bsa_ctx.hip):
  // one DMA per batch; pin_ev guards the buffer while a DMA from it may run
  void *pin = nullptr;
  size_t pin_bytes = 0;
  hipEvent_t pin_ev = nullptr;
  bool pin_busy = false;

  // multi-GPU: comm is an ncclComm_t (one process per GPU) or group an
  // in-process group of contexts (bsa_comm.hip); at most one is set
  void *comm = nullptr;
  struct Group *group = nullptr;
  int nranks = 1, rank = 0;
  DevBuf red;  // small reduction scratch
  // stream-ordered collectives this rank issued since the last bsa_timing_reset
  // (bsa_sim_comm_stats): calls and the bytes it sends / receives (payload,
  // as RCCL would move them; the in-process group's staging copies aside)
  int64_t comm_calls = 0, comm_tx = 0, comm_rx = 0;
  DevBuf pg_send, pg_recv;  // C2 pair gather staging (bsa_gather_pairs)

  // GPU-resident sim (bsa_sim.hip).  Its state lives in HOME order: home
  // position h holds aircraft h2id[h] (id2h is the inverse), fixed at init as
  // the spatial order of the initial traffic, so a rank's rows are a
  // contiguous, spatially compact home range [sim_rb, sim_re) (512-aligned)
  // and the detect reads its columns without a gather or a re-sort.  lpos[r]:
  // position of home sim_rb + r among the rank's rows sorted by aircraft index.
  bool home = false;                  // own[] and the sim arrays are in home order
  bool last_home = false;             // the last detect's ci / li are home rows (fetch translates)
  DevBuf h2id, id2h;                  // u32, device
  DevBuf lbyidx;                      // u32, device: this rank's home rows (relative) in ascending index order
  DevBuf fetch_stage;                 // fetch_pairs of a home-order detect: the lists re-ordered on the device
  std::vector<unsigned> h2id_h, id2h_h, lpos_h;  // host copies
  bool sim_ready = false;
  DevBuf nx_alt, nx_vs, nx_gse, nx_gsn;  // K2 fused with K4' (one rank): alt / vs / gseast / gsnorth double buffers
  bsa_sim_params simp{};
  StepClocks clk;
  int64_t sim_rb = 0, sim_re = 0, sim_rpr = 0;
  int64_t sim_last_conf = 0, sim_last_los = 0;
  bool sim_gathered = true;  // replicas consistent with every rank's rows
  bool sim_gs_derivable = false;  // gseast / gsnorth of every row follow from gs / trk (K4' without wind ran)
  DevBuf s_tas, s_hdg, s_gse, s_gsn;                        // traffic state besides own[]
  DevBuf s_aptrk, s_aptas, s_apalt, s_apvs, s_selalt, s_bank, s_eps, s_accel;  // frozen
  DevBuf s_atrk, s_atas, s_avs, s_aalt, s_ase, s_asn, s_active;  // ASAS (full n)
  DevBuf g_send, g_recv;  // all-gather staging (bsa_xfer.hip: gather_rows; g_send also comm_allgather_inplace's)
  // Non-finite tcpa inputs (StateBasedCD.py:90: tcpamax = np.max(tcpa *
  // swconfl) is NaN on every row once one tcpa is NaN): nonfin[0] = the epoch
  // of the last column records holding a non-finite lat / lon / u / v (its
  // producers store the epoch, K2 compares; no zeroing, no atomics)
  DevBuf nonfin;
  DevBuf rownf;  // rows of their own (not columns): per row (index order), its position / velocity is not finite
  unsigned long long nf_counter = 0, nf_prep_epoch = 0;  // epochs (K0b: a new one; K4' prep: the next detect's)
  DevBuf sim_ctl;  // [0,24) gate {abort / non-finite, P, HK prediction}; [24,28) sticky abort / stop; [28,32) the
                   // stopping stage and step's tag; [32,40) steps
                   // done; [40,48) resopairs demand on a bookkeeping overflow; [48,56) pair-key
                   // block demand (several ranks); [56,64) an HK-kept list went stale in the batch;
                   // [64, kSimCtlEnd) the stopping stages' pending words (BatchCtl)
  StopSide stops[kStopCount];  // the stopping stages' unpolled stops (stage_stopped; the polls consume them)
  // ASAS bookkeeping (bsa_asas.hip, resume_nav = 1): resopairs CSR over own
  // rows (+ next), per-row kept counts, LoS row pointers of the last call,
  // previous call's conflict / LoS CSR (one rank), stats
  DevBuf bk_rptr, bk_rcol, bk_nptr, bk_ncol, bk_cnt, bk_lptr, bk_pcptr, bk_plptr, bk_pccol, bk_plcol;
  DevBuf bk_stats, bk_tmp;
  unsigned long long bk_cap = 0;  // resopairs capacity (pairs)
  // several ranks: this rank's pair-key block and all ranks' blocks (this / the
  // previous call), bk_kw words per rank (grown on demand, the step retried)
  DevBuf bk_ksend, bk_kcur, bk_kprev;
  unsigned long long bk_kw = 0, bk_kw_alloc = 0;
  bool bk_ready = false;

  // halo exchange of the row-sharded resident step (bsa_halo.hip): each rank
  // receives only the column tiles its rows' boxes can reach (plus the tiles
  // of its resopairs' intruders) and prepares only those and its own tiles
  int halo_mode = 0;               // detect_enqueue (home mode): 0 off, 1 exchange (several ranks),
                                   // 2 one-GPU probe of one rank's share (bsa_sim_detect_rows)
  std::vector<int64_t> halo_cap;   // R x R tile capacities [sender * R + receiver], equal on all ranks
  DevBuf h_blk, h_gblk, h_plan, h_lists, h_send, h_recv, h_hl, h_dem;
  DevBuf h_present;                // plan reuse: the kept plan's present mask (k_halo_lists at a rebuild)
  int64_t halo_hl = 0;             // slots of the flat halo tile list (this rank's receive capacities)
  int64_t halo_grows = 0;          // capacity regrowths (aborted steps)
  int64_t halo_rx = 0, halo_tx = 0;  // bytes received / sent per CD step (the capacities' transfers)
  int halo_fields = 8;             // fp64 arrays per halo row of the last exchange (6 when derivable)
  bool last_fused = false;  // the last detect ran K1b fused into the prefilter (ExactFuse, bsa_cd_args.h)
  bool fuse_skip = false;   // a fused detect ran out of flush records: its retry runs K1b as its own launch
  bool fuse_on = true;      // bsa_set_exact_fusion
  int fuse_recs = kFuseRecsMax;  // ... per-wave mid-sweep flush records (testing knob)
  int64_t fuse_count = 0, fuse_retries = 0;  // bsa_exact_fusion_stats
  int sym_on = 2;           // bsa_set_symmetric_sweep: the level allowed (DetectPlan::sym)
  int last_sym = 0;         // the last detect's level (> 0: it swept each unordered tile pair once)
  int64_t sym_count = 0;    // ... and how many did (bsa_symmetric_sweep_stats)
  int lean_on = 1;          // bsa_set_lean_pairs: a batch's detects before its last skip the pair lists (StepPlan::lean;
                            // 2: its last one too, a testing aid)
  int64_t batch_target = 0; // clk.steps at the end of the bsa_sim_step call being enqueued (StepPlan::lean)
  // region layout agreement (comm_halo): every rank's send lengths / offsets
  // are compared with every receiver's expectation whenever the layout may have
  // changed -- a new capacity generation (init, regrowth: collective events) or
  // field count -- before any grouped send / recv is enqueued
  int64_t halo_cap_gen = 0, halo_chk_gen = -1;
  int halo_chk_nf = -1;
  int halo_tot_word = 0;           // h_dem word holding the last plan's received-tile total

  // 2-D wind field (bsa_set_windfield): lat lon vnorth veast of wf_nvec points
  DevBuf wfield;
  int64_t wf_nvec = 0;
  // 3-D wind field (bsa_set_windfield3d, bsa_wind.hip): lat lon of wf3_nvec points, then
  // {vnorth, veast}[level * nvec + point] on wf3_nalt levels wf3_altstep [m] apart.
  // wind_pa: the wind per aircraft k_wind3d wrote last (vnorth, then veast at + wind_pa_n);
  // wind_stage: bsa_wind_getdata's positions
  DevBuf wfield3, wind_pa, wind_stage;
  int64_t wf3_nvec = 0, wf3_nalt = 0, wind_pa_n = 0;
  double wf3_altstep = 0.0;

  // Turbulence.Woosh in the resident step (bsa_sim_set_turbulence, bsa_turb.hip): sd as given
  // (clamped where the scale is made) and the seed; the call number of the next step's draws is clk.turb_call.
  // turb_stage: bsa_turb_draws / _apply's arrays
  DevBuf turb_stage;
  bool sim_turb = false;
  double turb_sd[3] = {0.0, 0.0, 0.0};
  unsigned long long turb_seed = 0;

  // The area filter (bsa_area.hip).  area_stage: bsa_area_inside's points, masks, counts and table
  DevBuf area_stage;
  // Sector occupancy in the resident step (bsa_sim_set_areas / _set_sectors): the packed area
  // table (host) and its vertices (device); the sectors' shapes in sector order (sect_tab), their counts
  // (sect_cnt, kSect* words), the mask word of every aircraft at the last update (s_scur) and at the one before
  // (s_sprev), both per-aircraft arrays (kSimArrays).  sect_every: the cadence, in steps of clk.sect_ctr;
  // sect_gone: deleted aircraft's words until the next bsa_sim_sectors_deleted
  std::vector<bsa_area_shape> area_tab;
  DevBuf area_verts, sect_tab, sect_cnt, s_scur, s_sprev;
  bool sim_sect = false;
  std::vector<int32_t> sect_idx;
  int64_t sect_every = 1;
  struct SectGone {
    int64_t pos;
    unsigned long long word;
  };
  std::vector<SectGone> sect_gone;

  // Geovectoring (bsa_geovec.hip).  gv_stage: bsa_geovec_apply's arrays and tables.  In the
  // resident step (bsa_sim_set_geovectors): the rows (gv_tab, shape = row number) and their shapes in list order
  // (gv_shapes), the undo set an applying launch fills first (gv_undo, 4 x n fp64: selspd ap_trk selvs selalt at
  // the step's start), the counters (gv_cnt, kGvCntWords u64).  gv_every: the cadence, in steps of clk.gv_ctr
  DevBuf gv_stage, gv_tab, gv_shapes, gv_undo, gv_cnt;
  bool sim_gv = false;
  int gv_n = 0;
  int64_t gv_every = 1;

  // Conditional commands (bsa_cond.hip).  cond_stage: bsa_cond_update's arrays.  In the resident
  // step (bsa_sim_set_conditions): the table by aircraft index -- idx / type / target (host mirrors cond_*_h of
  // every device row), lastdif and a flag byte per row (live / fired at the last stop / dead) on the device only,
  // cond_ws the ordered compaction's words (flagged_list).  steps_last / steps_total: what bsa_sim_steps_run reports
  DevBuf cond_stage, cond_idx, cond_type, cond_tgt, cond_last, cond_flag, cond_ws;
  std::vector<int32_t> cond_idx_h, cond_type_h;
  std::vector<double> cond_tgt_h;
  bool sim_cond = false;
  int64_t sim_aborts = 0;  // batches aborted and re-run since bsa_sim_init (batch_rollback; bsa_sim_aborts)
  int64_t steps_last = 0, batch_steps0 = 0;  // (the step count at the running batch's begin: StepPlan::cond_tag)

  // The experiment area (bsa_exparea.hip).  xa_stage: bsa_exparea_update's arrays.  In the resident
  // step (bsa_sim_set_exparea): per aircraft (kSimArrays) the accumulators distance2D / distance3D / work, oldalt,
  // create_time and a flag byte (inside / exit pending / taxi delete pending); xa_shape: the area (a copy of its
  // row of area_tab) or none (name None: everything is outside); xa_every: the cadence, in steps of clk.area_ctr;
  // xa_dt: the plugin's nominal dt; xa_ws / xa_rec: the ordered compaction's words (flagged_list) and the poll's
  // records; xa_now: the simt new aircraft are created at (bsa_sim_exparea_simt)
  DevBuf xa_stage, s_xd2, s_xd3, s_xwork, s_xoldalt, s_xctime, s_xflag, xa_ws, xa_rec;
  bool sim_exparea = false, xa_has_shape = false, xa_active = false, xa_swtaxi = true;
  bsa_area_shape xa_shape{};
  int64_t xa_every = 1;
  double xa_dt = 0.5, xa_swtaxialt = 0.0, xa_now = 0.0;

  // Trails (bsa_trails.hip).  tr_stage: bsa_trails_update's arrays.  In the resident step
  // (bsa_sim_set_trails): per aircraft (kSimArrays) lastlat / lastlon / lasttim; the segment buffers tr_seg (5 fp64
  // arrays of tr_cap, then int32 idx) the pass appends to at the running total (sim_ctl, kSimCtlTrail); tr_ws the
  // compaction's words; tr_max the most tr_cap may grow to; tr_undrained / tr_demand: the total and the demand
  // word as the last batch's read-back (or drain) left them.  Its clock: clk.trail_simt
  DevBuf tr_stage, s_tlat, s_tlon, s_ttim, tr_seg, tr_ws;
  bool sim_trails = false, tr_active = false;
  double tr_dt = 10.0;
  int64_t tr_cap = 0, tr_max = 0, tr_undrained = 0, tr_demand = 0;

  // The ADS-B model (bsa_adsb.hip).  adsb_stage: bsa_adsb_update's / bsa_adsb_draws' arrays.  In the
  // resident step (bsa_sim_set_adsb): per aircraft (kSimArrays) the picture lat lon alt trk tas gs vs and two
  // lastupdate buffers -- a step reads s_adlast<clk.adsb_cur> and writes the other for all its rows, so an aborted
  // step leaves the one it read as it was.  Its clocks: clk.adsb_*
  DevBuf ad_shared;  // the step's shared draw: three unit normals, written by a one-lane launch in front of k_adsb
  DevBuf adsb_stage, s_adlast0, s_adlast1, s_adlat, s_adlon, s_adalt, s_adtrk, s_adtas, s_adgs, s_advs;
  bool sim_adsb = false, ad_noise = false, ad_per_ac = false;
  double ad_sigma[2] = {1e-4, 30.48}, ad_trunc = 0.0;
  unsigned long long ad_seed = 0;

  // standalone geo matrices (bsa_geo.hip)
  DevBuf geo_in, geo_pts, geo_out;
  hipEvent_t geo_ev[2] = {nullptr, nullptr};
  double geo_ms = 0.0;

  // ACDATA feed of the resident sim (bsa_feed.hip): pre-step altitude of the
  // last step (for traf.cas), device staging, pinned host mirror, completion event
  DevBuf s_altprev, feed_dev;
  // OpenAP flight envelope of the resident sim (bsa_sim_set_limits) + traf.ax
  DevBuf s_env, s_ax;
  bool sim_limits = false;
  // OpenAP flight-phase envelope (bsa_sim_set_perf): type table, per-aircraft
  // type index (int32) and the phase of the last step (u8)
  DevBuf s_ptab, s_ptype, s_phase;
  bool sim_perf = false;
  // OpenAP drag / thrust / fuel flow (bsa_sim_set_forces, bsa_perf.hip): the
  // force table (16 doubles per type of s_ptab), per-aircraft mass, the six
  // outputs of the last step (6 x n: cd0 drag thrustratio thrust fuelflow
  // bank), the fuel burnt by the committed steps and the last step's share
  // (fuelflow x simdt, committed by the next step's launch)
  DevBuf s_ftab, s_fmass, s_fout, s_fused, s_fpend;
  DevBuf f_const;  // perf::ForceConst, computed once per context
  bool sim_forces = false;
  // Autopilot guidance in the step (bsa_sim_set_fms, bsa_fms.hip),
  // home order: the 15 fp64 arrays of bsa_fms_state (15 x n), its 4 flags
  // (4 x n u8), iactwp / rt_off / rt_n (3 x n int32), the route table, and the
  // undo set a ticking launch fills first (17 x n fp64: the 13 mutable reals,
  // ap_trk / ap_alt / ap_vs / selalt; 2 x n u8; n int32).  Its clock: clk.fms_*
  DevBuf s_fmsr, s_fmsf, s_fmsi, s_fmsrows, s_fmsur, s_fmsuf, s_fmsui;
  bool sim_fms = false;
  int64_t fms_nrows = 0;  // rows of the route table (bsa_sim_set_fms's, plus what bsa_sim_create_with appended)
  // Route edits (bsa_route.hip): the waypoint type per table row (u8; the first fms_ntypes rows
  // hold one, rows behind them are type 0 until an edit reaches them), the second table a compaction writes,
  // staging, and the counts of bsa_sim_route_stats
  DevBuf s_fmstype, s_fmsrows2, s_fmstype2, rt_stage, rt_ws;
  int64_t fms_ntypes = 0, rt_written = 0, rt_compactions = 0;
  // NORESO / RESOOFF membership (bsa_sim_set_reso_lists, u8 in home order) and
  // the rows whose ResumeNav dropped a pair in the last CD call (u8, home order)
  // and how many pairs it dropped per row (int32: waypoint recovery runs once per pair)
  DevBuf s_noreso, s_resooff, s_dropped, s_dropcnt;
  bool sim_recovery = false;  // bsa_sim_set_recovery: k_sim_recover after k_bk_write
  DevBuf s_atm;          // traf.p / rho / Temp = vatmos(traf.alt) of the last step (3 x n), when on
  bool sim_atmos = false;
  bool sim_noreso = false, sim_resooff = false;
  int64_t sim_ntypes = 0;
  void *feed_host = nullptr;
  size_t feed_host_bytes = 0;
  hipEvent_t feed_ev = nullptr;
  bool feed_pending = false;
  int64_t feed_steps = 0, feed_rb = 0, feed_re = 0;
};

// the one place outside a detect that drops kept detect state (kDrops, bsa_kept.h)
inline void invalidate(Ctx *c, Change what) {
  const Drops &d = kDrops[(int)what];
  if (d.order) c->order.drop();
  if (d.cands) c->cands.drop();
  if (d.tiles) c->tiles.drop();
  if (d.prep) c->prep.drop();
  if (d.zero) c->zero.drop();
  if (d.hk) c->hk.drop();
}

// ---- the resident sim's per-aircraft arrays, described once
struct BufRef {  // a DevBuf of the context: c->*m, or c->own[own] when m is NULL
  DevBuf Ctx::*m;
  int own;
};
inline DevBuf &buf_at(Ctx *c, BufRef r) { return r.m ? c->*r.m : c->own[r.own]; }
// pointer k of an ABI struct that holds array pointers only
inline void *ptr_at(const void *strct, int k) { return ((void *const *)strct)[k]; }

// kSimArrays: every persistent per-aircraft array (home order).  sim_release,
// bsa_sim_delete / bsa_sim_create and the re-partition on several ranks walk
// it (bsa_traffic.hip: per_aircraft), bsa_sim_init allocates its kSimAlways rows
// guard: kSimAlways allocated by bsa_sim_init; kSimDetect the last detect's per-row outputs (the detect's to
// allocate); kSimOnUse once allocated (the reso lists); the others while Ctx::sim_<switch> is on
enum SimGuard { kSimAlways, kSimDetect, kSimOnUse, kSimLimits, kSimPerf, kSimForces, kSimFms, kSimAtmos, kSimSectors, kSimExparea, kSimTrails, kSimAdsb };
struct SimArray {
  BufRef buf;
  int esz, count;  // element size; sub-arrays of length n in the buffer
  bool gathered;   // bsa_sim_init allocates the all-gather length (nranks x rpr)
  SimGuard guard;
};
// bsa_fms_state: its fp64 arrays (the first kFmsMutable are written by a tick;
// selvs, apvsdef are read only), its flags, iactwp / rt_off / rt_n, and the
// reals of the undo set (the mutable ones + ap_trk, ap_alt, ap_vs, selalt)
constexpr int kFmsReals = 15, kFmsMutable = 13, kFmsFlags = 4, kFmsInts = 3, kFmsUndoReals = kFmsMutable + 4;
inline const SimArray kSimArrays[] = {
    {{nullptr, 0}, 8, 1, true, kSimAlways},         {{nullptr, 1}, 8, 1, true, kSimAlways},
    {{nullptr, 2}, 8, 1, true, kSimAlways},         {{nullptr, 3}, 8, 1, true, kSimAlways},
    {{nullptr, 4}, 8, 1, true, kSimAlways},         {{nullptr, 5}, 8, 1, true, kSimAlways},
    {{&Ctx::s_tas}, 8, 1, true, kSimAlways},        {{&Ctx::s_hdg}, 8, 1, true, kSimAlways},
    {{&Ctx::s_gse}, 8, 1, true, kSimAlways},        {{&Ctx::s_gsn}, 8, 1, true, kSimAlways},
    {{&Ctx::s_aptrk}, 8, 1, false, kSimAlways},     {{&Ctx::s_aptas}, 8, 1, false, kSimAlways},
    {{&Ctx::s_apalt}, 8, 1, false, kSimAlways},     {{&Ctx::s_apvs}, 8, 1, false, kSimAlways},
    {{&Ctx::s_selalt}, 8, 1, false, kSimAlways},    {{&Ctx::s_bank}, 8, 1, false, kSimAlways},
    {{&Ctx::s_eps}, 8, 1, false, kSimAlways},       {{&Ctx::s_accel}, 8, 1, false, kSimAlways},
    {{&Ctx::s_atrk}, 8, 1, false, kSimAlways},      {{&Ctx::s_atas}, 8, 1, false, kSimAlways},
    {{&Ctx::s_avs}, 8, 1, false, kSimAlways},       {{&Ctx::s_aalt}, 8, 1, false, kSimAlways},
    {{&Ctx::s_altprev}, 8, 1, false, kSimAlways},   {{&Ctx::s_ax}, 8, 1, false, kSimAlways},
    {{&Ctx::tcpamax}, 8, 1, false, kSimDetect},     {{&Ctx::s_ase}, 4, 1, false, kSimAlways},
    {{&Ctx::s_asn}, 4, 1, false, kSimAlways},       {{&Ctx::s_active}, 1, 1, false, kSimAlways},
    {{&Ctx::inconf}, 1, 1, false, kSimDetect},      {{&Ctx::s_noreso}, 1, 1, false, kSimOnUse},
    {{&Ctx::s_resooff}, 1, 1, false, kSimOnUse},    {{&Ctx::s_dropped}, 1, 1, false, kSimAlways},
    {{&Ctx::s_env}, 8, 6, false, kSimLimits},       {{&Ctx::s_atm}, 8, 3, false, kSimAtmos},
    {{&Ctx::s_ptype}, 4, 1, false, kSimPerf},       {{&Ctx::s_phase}, 1, 1, false, kSimPerf},
    {{&Ctx::s_fmass}, 8, 1, false, kSimForces},     {{&Ctx::s_fout}, 8, 6, false, kSimForces},
    {{&Ctx::s_fused}, 8, 1, false, kSimForces},     {{&Ctx::s_fpend}, 8, 1, false, kSimForces},
    {{&Ctx::s_fmsr}, 8, kFmsReals, false, kSimFms}, {{&Ctx::s_fmsf}, 1, kFmsFlags, false, kSimFms},
    {{&Ctx::s_fmsi}, 4, kFmsInts, false, kSimFms},   {{&Ctx::s_dropcnt}, 4, 1, false, kSimAlways},
    {{&Ctx::s_scur}, 8, 1, false, kSimSectors},      {{&Ctx::s_sprev}, 8, 1, false, kSimSectors},
    {{&Ctx::s_xd2}, 8, 1, false, kSimExparea},       {{&Ctx::s_xd3}, 8, 1, false, kSimExparea},
    {{&Ctx::s_xwork}, 8, 1, false, kSimExparea},     {{&Ctx::s_xoldalt}, 8, 1, false, kSimExparea},
    {{&Ctx::s_xctime}, 8, 1, false, kSimExparea},    {{&Ctx::s_xflag}, 1, 1, false, kSimExparea},
    {{&Ctx::s_tlat}, 8, 1, false, kSimTrails},       {{&Ctx::s_tlon}, 8, 1, false, kSimTrails},
    {{&Ctx::s_ttim}, 8, 1, false, kSimTrails},
    {{&Ctx::s_adlast0}, 8, 1, false, kSimAdsb},      {{&Ctx::s_adlast1}, 8, 1, false, kSimAdsb},
    {{&Ctx::s_adlat}, 8, 1, false, kSimAdsb},        {{&Ctx::s_adlon}, 8, 1, false, kSimAdsb},
    {{&Ctx::s_adalt}, 8, 1, false, kSimAdsb},        {{&Ctx::s_adtrk}, 8, 1, false, kSimAdsb},
    {{&Ctx::s_adtas}, 8, 1, false, kSimAdsb},        {{&Ctx::s_adgs}, 8, 1, false, kSimAdsb},
    {{&Ctx::s_advs}, 8, 1, false, kSimAdsb},
};
// is the array part of the sim now (to be carried through a delete / create)?
inline bool sim_array_on(Ctx *c, const SimArray &a) {
  switch (a.guard) {
    case kSimOnUse: return buf_at(c, a.buf).p != nullptr;
    case kSimLimits: return c->sim_limits;
    case kSimPerf: return c->sim_perf;
    case kSimForces: return c->sim_forces;
    case kSimFms: return c->sim_fms;
    case kSimAtmos: return c->sim_atmos;
    case kSimSectors: return c->sim_sect;
    case kSimExparea: return c->sim_exparea;
    case kSimTrails: return c->sim_trails;
    case kSimAdsb: return c->sim_adsb;
    default: return true;
  }
}

// kSimFields: the arrays of bsa_sim_state in its declaration order, row k for
// the pointer at byte 8 k (bsa_sim_init, bsa_sim_create, bsa_sim_update; the
// first kSimOutFields are bsa_sim_out's, at the same offsets).  An array of
// kSimArrays that no row names, as `buf` or as `also`, starts at zero
struct SimField {
  BufRef buf;         // its array
  bool replicated;    // the all-gather completes it on every rank
  bool cd_input;      // CD reads it: an update invalidates what was derived from it
  DevBuf Ctx::*also;  // a second array new aircraft start from this field (asas.py:402-407; the feed's
};                    // pre-step altitude), or NULL
inline const SimField kSimFields[] = {
    {{nullptr, 0}, true, true, nullptr},           {{nullptr, 1}, true, true, nullptr},            // lat lon
    {{nullptr, 4}, true, true, &Ctx::s_altprev},   {{&Ctx::s_tas}, false, true, &Ctx::s_atas},     // alt tas
    {{&Ctx::s_hdg}, false, true, nullptr},         {{nullptr, 5}, true, true, nullptr},            // hdg vs
    {{nullptr, 3}, true, true, nullptr},           {{nullptr, 2}, true, true, &Ctx::s_atrk},       // gs trk
    {{&Ctx::s_gse}, true, true, nullptr},          {{&Ctx::s_gsn}, true, true, nullptr},           // gseast gsnorth
    {{&Ctx::s_aptrk}, false, false, nullptr},      {{&Ctx::s_aptas}, false, false, nullptr},       // ap_trk ap_tas
    {{&Ctx::s_apalt}, false, false, nullptr},      {{&Ctx::s_apvs}, false, false, nullptr},        // ap_alt ap_vs
    {{&Ctx::s_selalt}, false, false, nullptr},     {{&Ctx::s_bank}, false, false, nullptr},        // selalt bank
    {{&Ctx::s_eps}, false, false, nullptr},        {{&Ctx::s_accel}, false, false, nullptr},       // eps accel
    {{&Ctx::s_aalt}, false, false, nullptr},                                                       // asas_alt
};
constexpr int kSimStateFields = sizeof(kSimFields) / sizeof(kSimFields[0]), kSimOutFields = 10;
static_assert(kSimStateFields * sizeof(double *) == sizeof(bsa_sim_state) &&
                  offsetof(bsa_sim_state, asas_alt) == (kSimStateFields - 1) * sizeof(double *),
              "one kSimFields row per bsa_sim_state array");
static_assert(offsetof(bsa_sim_out, gsnorth) == offsetof(bsa_sim_state, gsnorth), "bsa_sim_out starts as bsa_sim_state");
inline bool sim_field_names(Ctx *c, const DevBuf *b) {
  for (const SimField &f : kSimFields)
    if (&buf_at(c, f.buf) == b || (f.also && &(c->*f.also) == b)) return true;
  return false;
}

// the ASAS outputs in bsa_asas_out's field order (bsa_sim_read: the first four and active)
struct AsasArray {
  DevBuf Ctx::*buf;
  int esz;
};
inline const AsasArray kAsasArrays[8] = {{&Ctx::s_atrk, 8}, {&Ctx::s_atas, 8}, {&Ctx::s_avs, 8},    {&Ctx::s_aalt, 8},
                                         {&Ctx::s_ase, 4},  {&Ctx::s_asn, 4},  {&Ctx::s_active, 1}, {&Ctx::s_dropped, 1}};
static_assert(8 * sizeof(void *) == sizeof(bsa_asas_out), "one kAsasArrays row per bsa_asas_out array");

// bsa_fms_state's arrays in declaration order
struct FmsFields {
  double *reals[kFmsReals];
  uint8_t *flags[kFmsFlags];
};
inline FmsFields fms_fields(const bsa_fms_state &st) {
  return {{st.actwp_lat, st.actwp_lon, st.actwp_nextaltco, st.actwp_xtoalt, st.actwp_spd, st.actwp_vs,
           st.actwp_turndist, st.actwp_flyby, st.actwp_next_qdr, st.dist2vs, st.vnavvs, st.swvnavvs, st.selspd,
           st.selvs, st.apvsdef},
          {st.swlnav, st.swvnav, st.abco, st.belco}};
}

// device pointers for the MVP kernel (full-N traffic arrays, per-row outputs)
struct MvpDev {
  const double *gseast, *gsnorth, *vs, *alt, *trk, *gs, *selalt, *apvs;
  const double *aptrk, *aptas, *apalt;  // resident step, CR OFF (DoNothing.py) only; else NULL
  const uint8_t *noreso, *resooff;
  double *asas_alt, *o_trk, *o_tas, *o_vs;
  float *o_asase, *o_asasn;
  double *o_tsolv;
};
struct MvpIn;
// pairs_done / rows_folded: K2 of the same detect wrote the per-pair vectors /
// folded them per row (DetectResult).  defer != NULL (resident step): the
// per-row kernel is not launched; its arguments go to *defer for the fused
// MVP + pilot + kinematics kernel
int mvp_device(Ctx *c, const bsa_mvp_params &p, const MvpDev &d, const unsigned *seg,
               const unsigned long long *gate, unsigned *sticky, const uint8_t *inconf, uint8_t *active,
               bool resolve, bool pairs_done = false, bool rows_folded = false, MvpIn *defer = nullptr);

// device pointers for the fused kinematics kernel
struct KinDev {
  const double *ptas, *phdg, *palt, *pvs, *bank, *eps, *accel;
  double *tas, *hdg, *alt, *vs, *lat, *lon;
  double *ax, *delspd, *cas, *mach, *gsnorth, *gseast, *gs, *trk, *coslat, *az;
  uint8_t *swhdgsel, *swaltsel;
};
int kin_device(Ctx *c, int64_t n, double simdt, int winddim, double vn, double ve, const KinDev &d);
struct WindField;
WindField wind_field(const Ctx *c);  // device view of the context's 2-D field (bsa_kin.hip)
// winddim 3 (bsa_wind.hip): k_wind3d on rows [rb, re) of n, enqueued in front of the kernel that reads
// wind_field_pa(c), the per-aircraft wind it writes
int wind3d_launch(Ctx *c, int64_t rb, int64_t re, int64_t n, const double *lat, const double *lon, const double *alt);
WindField wind_field_pa(const Ctx *c);
// Turbulence.Woosh of the step (bsa_turb.hip): k_sim_turb on home rows [rb, re), call number clk.turb_call,
// enqueued after the step's K4' on the arrays it wrote.  turb_off: off, the call number back at 0
int turb_sim_launch(Ctx *c, int64_t rb, int64_t re, const unsigned *sticky, const double *trk, double *lat,
                    double *lon, double *alt);
void turb_off(Ctx *c);

// The stopping stages (StopStage; the device side: bsa_stop.h).  stage_stopped: batch_stopped found the stage's
// pending word at the stop's tag (the clocks are already those of the stop); the stage's poll consumes it
void stage_stopped(Ctx *c, StopStage s);
// Conditional commands of the step (bsa_cond.hip): k_sim_cond, the step's first stopping launch; tag: the step's
// number in its batch + 1 (what a stop it raises carries).  cond_note_deleted: Condition.delac for the (sorted)
// aircraft of a bsa_sim_delete, before anything moves.  cond_off forgets the table
int cond_sim_launch(Ctx *c, unsigned tag);
int cond_note_deleted(Ctx *c, const std::vector<int64_t> &d);
void cond_off(Ctx *c);

// The experiment area of the step (bsa_exparea.hip): k_sim_exparea, the step's last launch (after
// k_sim_cond) in the steps whose StepPlan::area_pass is set; tag as for cond_sim_launch.  exparea_passes_at: does
// the step at clk.area_ctr run the pass?  exparea_created: Area.create for the m aircraft bsa_sim_create appended
// after the first n (alt: theirs, host)
bool exparea_passes_at(const Ctx *c);
int exparea_sim_launch(Ctx *c, unsigned tag);
int exparea_created(Ctx *c, int64_t n, int64_t m, const double *alt);
void exparea_off(Ctx *c);

// Trails of the step (bsa_trails.hip): Trails.update(simt) on what the step left, after k_sim_cond
// and before the experiment area's pass; t: clk.trail_simt before the step's advance; tag as for cond_sim_launch.
// trails_reserve: the segment buffers sized for nsteps more steps, before a batch is enqueued (refuses a batch
// whose bound exceeds tr_max).  trails_created: Trails.create for the m aircraft bsa_sim_create appended after the
// first n (lat / lon: theirs, host)
int trails_sim_launch(Ctx *c, double t, unsigned tag);
int trails_reserve(Ctx *c, int64_t nsteps);
int trails_created(Ctx *c, int64_t n, int64_t m, const double *lat, const double *lon);
void trails_off(Ctx *c);

// The ADS-B model of the step (bsa_adsb.hip): ADSB.update(simt) on the state the previous step left,
// this rank's rows, after a geovector application and before the FMS stage (traffic.py:392); t: clk.adsb_simt before
// the step's advance.  adsb_created: ADSB.create for the m aircraft bsa_sim_create appended after the first n (s:
// their state, host).  adsb_off: off, the arrays released, the clocks back at 0
int adsb_sim_launch(Ctx *c, double t);
int adsb_created(Ctx *c, int64_t n, int64_t m, const bsa_sim_state *s);
void adsb_off(Ctx *c);

// Sector occupancy (bsa_area.hip): sect_sim_launch after the last stage of a step whose StepPlan::sect_pass is
// set (clk.sect_ctr + 1 a multiple of the cadence); sect_note_deleted by bsa_sim_delete before anything moves;
// sect_off forgets the sectors
int sect_sim_launch(Ctx *c);
int sect_note_deleted(Ctx *c, int64_t k, const int64_t *idx);
void sect_off(Ctx *c);
// the area table as the kernels read it (bsa_area.hip): every argument checked, corners and levels sorted, the
// cull bounds filled in; BSA_AREA_CULL=0 in the environment
int area_pack(Ctx *c, const char *who, int64_t nshapes, const bsa_area_shape *shapes, int64_t nvert,
              const double *verts, std::vector<bsa_area_shape> *out);
bool area_env_nocull();

// Geovectoring in the resident step (bsa_geovec.hip).  geovec_applies_at: does the step at
// clk.gv_ctr apply -- are the steps completed since bsa_sim_set_geovectors a positive multiple of the cadence
// (StepPlan::gv_apply)?  geovec_sim_launch: the launch of such a step, first on its stream.
// geovec_sim_restore: the undo set back into the state, stream-ordered (after an aborted applying step).
// geovec_off forgets the geovectors
bool geovec_applies_at(const Ctx *c);
int geovec_sim_launch(Ctx *c);
int geovec_sim_restore(Ctx *c);
void geovec_off(Ctx *c);

// OpenAP drag / thrust / fuel flow (bsa_perf.hip).  forces_consts: Ctx::f_const
// filled (once).  forces_sim_launch: k_sim_forces of the step about to be
// enqueued, on this rank's rows; commit = the pending fuel of the step before
// is added to fuel_used first (false for the first step of a re-run attempt).
int forces_consts(Ctx *c);
int forces_sim_launch(Ctx *c, bool commit);
void forces_off(Ctx *c);
// The <stage>_created hooks of bsa_sim_create_with, for the m aircraft appended after the first n:
// the stage's arrays are already grown to n + m, moved to that stride and zero in the new rows (so the flight phase,
// the force outputs, perf.bank and the fuel burnt start as after set_perf / set_forces); each copies its checked
// part of x into the new rows, stream-ordered, and does nothing while its stage is off.  limits_created /
// perf_created: bsa_sim.hip; forces_created: bsa_perf.hip; fms_created (bsa_fms.hip) also appends x.route_rows to the
// route table, rebases rt_off by the rows it held and sizes the undo set for n + m; it synchronises
int limits_created(Ctx *c, int64_t n, int64_t m, const bsa_sim_create_extra &x);
int perf_created(Ctx *c, int64_t n, int64_t m, const bsa_sim_create_extra &x);
int forces_created(Ctx *c, int64_t n, int64_t m, const bsa_sim_create_extra &x);
int fms_created(Ctx *c, int64_t n, int64_t m, const bsa_sim_create_extra &x);

// Autopilot guidance (bsa_fms.hip).  fms_check_routes: every index the kernels
// use unguarded, on host arrays.  fms_sim_launch: k_sim_fms of the step about
// to be enqueued, on this rank's rows (tick: the whole FMS part, after saving
// the undo set; else ap.tas only).  fms_sim_restore: the undo set back into
// the state, stream-ordered (after an aborted tick step).  fms_off: guidance
// off, and with it what lives in its arrays: waypoint recovery, the geovectors
int fms_check_routes(Ctx *c, const char *who, int64_t n, int64_t nrows, const int32_t *rt_off, const int32_t *rt_n,
                     const int32_t *iactwp, const uint8_t *swlnav);
int fms_sim_launch(Ctx *c, bool tick);
int fms_sim_restore(Ctx *c);
// the device view of the FMS arrays (the resident sim's: fms_sim_arrays; the standalone calls stage their own)
struct FmsArrays {
  const double *tr[8];     // lat lon alt tas gs trk ax bank (read only)
  double *st[kFmsReals];   // bsa_fms_state's doubles (selvs, apvsdef read only)
  uint8_t *fl[4];          // swlnav swvnav abco belco (abco, belco read only)
  double *tg[5];           // ap_trk ap_tas ap_alt ap_vs selalt
  int *iactwp;
  const int *rt_off, *rt_n;
  const double *rows;
};
FmsArrays fms_sim_arrays(Ctx *c);
void fms_off(Ctx *c);
// waypoint recovery of the CD step just enqueued (after bk_apply, before K4'): k_sim_recover on this rank's rows
int fms_sim_recover(Ctx *c);
inline bool fms_ticks_at(double simt, double t0) { return t0 + 1.01 < simt || simt < t0 || simt < 1.01; }

// ASAS bookkeeping of one CD call (bsa_asas.hip): bk_count before the gate
// all-reduce and MVP (may raise the gate's bit 1 on resopairs overflow),
// bk_apply after MVP.  State arrays are full-N device arrays.
struct BkDev {
  const double *lat, *lon, *gse, *gsn, *trk;  // home order
  const unsigned *h2id, *id2h;                // home <-> aircraft index
  uint8_t *active;
  uint8_t *dropped;             // per row: ResumeNav dropped one of its pairs (waypoint recovery)
  int *dropcnt;                 // ... and how many (one findact + direct each)
  unsigned long long *gate;
  unsigned *sticky;
  unsigned long long *demand;   // resopairs overflow: pairs needed
  unsigned long long *kdemand;  // several ranks, key block overflow: words needed
};
#if defined(__HIPCC__)
// the abort test of every kernel enqueued after the gate all-reduce of a CD step (the bookkeeping, k_sim_recover)
__device__ __forceinline__ bool bk_aborted(const unsigned long long *gate, const unsigned *sticky) {
  return sticky[0] != 0 || gate[0] >= kGateOverflow;
}
#endif
int bk_count(Ctx *c, const BkDev &d);
int bk_apply(Ctx *c, const BkDev &d);
void bk_release(Ctx *c);

// halo exchange (bsa_halo.hip; halo_pre / halo_mid and the device pieces in
// bsa_halo.h).  halo_mid: after K0 prepared the rank's own column tiles (and
// their boxes), plan which tiles every rank needs, exchange them (mode 1) and
// leave the flat list of this rank's halo tiles in h_hl (halo_hl slots, -1 =
// unused) and its present mask in h_plan
bool home_records(const Ctx *c, int64_t nrows);   // home-mode detect (of nrows rows) stores fp64 column records
int stage1_mid(int flags, bool reuse, int kwik);  // midpoint stage 1 for this detect?
int halo_init_caps(Ctx *c);      // bsa_sim_init, several ranks: exact initial capacities (no exchange)
int halo_grow(Ctx *c);           // after an aborted step, several ranks (collective)
void halo_release(Ctx *c);
const uint8_t *halo_present(const Ctx *c);  // the received-tile mask of the last halo_mid
const unsigned *halo_list_count(const Ctx *c);  // the probe's halo list length (device), else NULL
// K0b over every column tile (fused boxes, no per-detect zeroing): the halo
// plan's view of all tile boxes when every rank's state is on this GPU (bsa_k0.hip)
// every column tile's records and boxes (one K0b); nf_epoch != 0: non-finite
// columns store it into Ctx::nonfin (the detect that takes that epoch sees them)
int prep_all_tiles(Ctx *c, double rpz, double hpz, double tla, unsigned long long nf_epoch = 0);
// the buffers a preparer of n columns writes (K0b, or K4' for the next detect):
// colrec (rec only), pfcol, pfvcol, pfpcol and the tile / group / sub-group boxes
bool ensure_col_prep(Ctx *c, int64_t n, bool rec);

// exclusive prefix sum of n words, one launch (bsa_scan.hip)
int scan_excl(Ctx *c, const unsigned *in, unsigned *out, int n);
// The i in [0, n) with (flag[id2h ? id2h[i] : i] & mask) != 0 in ascending order (np.where's): wave ballots, one
// scan_excl, ranks within the wave, no atomic cursor.  ws: flagged_ws_words(n) words of device scratch; the list
// also stays in it, at *dev_list (or NULL).  Synchronises the stream
size_t flagged_ws_words(int64_t n);
int flagged_list(Ctx *c, int64_t n, const uint8_t *flag, const unsigned *id2h, unsigned mask, unsigned *ws,
                 std::vector<int32_t> *out, const int **dev_list);
// spatial (home) order of the n aircraft in own[] (bsa_k0.hip): home -> aircraft index
int home_order(Ctx *c, double tla, std::vector<unsigned> &h2id);
// the last detect's pair lists and per-row outputs in aircraft-index terms
// (bsa_ctx.hip): home rows -> indices, rows in ascending index order
struct HostPairs {
  std::vector<int32_t> ci, cj, li, lj;
  std::vector<double> pay;  // 5 x P (qdr dist tcpa tinconf dcpa)
  std::vector<uint8_t> inconf;
  std::vector<double> tcpamax;
};
int download_pairs(Ctx *c, HostPairs &h);
void home_pairs_to_ids(const Ctx *c, int64_t rb, HostPairs &h);
// resident sim (bsa_sim.hip): the maps of Ctx::h2id_h (host + device, lpos of this rank's rows)
int set_home_maps(Ctx *c);
// this rank's 512-aligned home range [sim_rb, sim_re) and rows per rank for c->n (bsa_sim.hip)
void set_rank_rows(Ctx *c);

// error helpers
int fail(Ctx *c, const char *fmt, ...);
#define BSA_HIP(c, call)                                                              \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess)                                                             \
      return ::bsa::fail((c), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                         __FILE__, __LINE__);                                         \
  } while (0)

// collectives (bsa_comm.hip): RCCL or the in-process group, stream-ordered;
// no-ops (plain copies) with one rank
bool comm_multi(const Ctx *c);
int comm_allgather(Ctx *c, const void *send, void *recv, size_t bytes);  // recv: nranks x bytes
int comm_allreduce_max_u64(Ctx *c, unsigned long long *buf, int count); // device words, in place
int comm_allgather_inplace(Ctx *c, double *const *f, int nf, size_t rpr); // rank blocks of nf arrays
int comm_allreduce_host(Ctx *c, double *v, int count, bool max);         // host values (synchronises)
int comm_gatherv(Ctx *c, int root, const void *send, size_t bytes, void *recv, const size_t *off,
                 const size_t *len);                                     // rank-order blocks to root
int comm_halo(Ctx *c, const void *send, const size_t *soff, const size_t *slen, size_t stot, void *recv,
              const size_t *roff, const size_t *rlen, const size_t *peer);  // halo regions (bsa_halo.hip)
void comm_release(Ctx *c);

// sim / comm teardown (bsa_sim.hip); ACDATA feed teardown (bsa_feed.hip)
void sim_release(Ctx *c);
void feed_release(Ctx *c);
int sim_adopt_pairs(Ctx *c);  // after resident steps: the last CD call's pairs become fetchable

// ---- one detect (bsa_cd.hip): what the caller asks for and what it gets back.
// Everything a detect honours is in its DetectRequest; nothing of one call is
// left on the context for the next.
// Non-finite tcpa inputs (Ctx::nonfin): producers (the column records'
// makers) store `epoch` into *word when a column's position or velocity is
// non-finite; K2 makes every row's tcpamax NaN when *word == epoch, and a
// row's own when rowbad[row] is set (rows of their own, written by
// k_prep_rows in index order; NULL when the rows are columns)
struct NfArgs {
  unsigned long long *word;
  unsigned long long epoch;
  const uint8_t *rowbad;
};
// full-N traffic arrays MVP's per-pair vector reads (bsa_mvp_math.h)
struct MvpPairIn {
  const double *gseast, *gsnorth, *vs, *alt;
  const uint8_t *noreso;  // NULL = empty NORESO list
  const unsigned *id2h;   // resident step (home order): the intruder's home position; NULL = identity
};
// MVP's per-pair vectors written by k_rank in the resident step (pdv == NULL: off)
struct MvpFuse {
  bsa_mvp_params p;
  MvpPairIn in;
  double4 *pdv;
  uint8_t *pfl;
  double4 *rowdv;  // k_rank_rows: each row's folded dv (mvp_fold), or NULL
};
// the next detect's listed items (HeavyArgs, bsa_cd_args.h): what heavy_next (bsa_rank.hip) reads and appends to
struct HeavyNext {
  unsigned *cost;           // read and zeroed
  unsigned *list[2], *count, *flag;
  unsigned epoch;           // the next detect's
  unsigned thresh[2];       // ticks (100 MHz)
  const unsigned long long *work;  // [1] near, [2] far items of this detect's list
  unsigned long long icap;
};
constexpr unsigned kHeavyBlocks = 64;  // extra workgroups for the listing (k_rowblk's; the lean k_rank_rows')
// k_rank_rows' arguments (a value, so that the step can launch K2 fused with its K4': k24_launch)
struct RankLaunch {
  unsigned grid;
  int nrows;
  Counters *cnt;
  unsigned long long cap;
  unsigned *rowoff, *rowcnt;
  const uint2 *kb;
  int B;
  const double *cpay;
  int rb;
  int *ci, *cj;
  double *out;
  int *li, *lj;
  unsigned long long *stats, *gate;
  const unsigned *build;
  MvpFuse mf;
  unsigned char *inconf;
  unsigned long long *tcpamax;
  Counters *cnext;
  unsigned long long *wnext;
  NfArgs nf;
  unsigned long long *hkp;  // HK: the prediction word K2 moves into gate[2] (NULL: none / fused K4' publishes it)
  // the lean form (DetectRequest::lean_k2, fused with K4' only): no block sums, no pair lists; grid = the row blocks
  // + heavy extra workgroups that list the next detect's items (hn), k_rowblk's part on a full detect
  bool lean = false;
  unsigned heavy = 0;
  HeavyNext hn{};
};
struct DetectRequest {
  double rpz = 0.0, hpz = 0.0, tla = 0.0;
  int flags = 0;
  int64_t rb = 0, re = 0;              // rows (re <= 0: all)
  unsigned long long *gate = nullptr;  // (device, nullable): receives {overflow, P, HK prediction} for the resident step
  bool home = false;                   // own[] is in home order (the resident sim's state), rows a 512-aligned home slice
  bool host_decides = false;           // HK: the tile-pair list's build / keep decision may be the host's
  unsigned long long nf_epoch = 0;     // != 0: the non-finite epoch this detect takes (records prepared by the caller carry it)
  // != NULL: K2 evaluates MVP's per-pair vectors as it places each pair (full-N device arrays)
  const bsa_mvp_params *mvp = nullptr;
  const double *gse = nullptr, *gsn = nullptr, *vs = nullptr, *alt = nullptr;
  const uint8_t *noreso = nullptr;     // NORESO list or NULL
  bool keep_k2 = false;                // K2 (k_rank_rows) is not launched but returned, for a launch fused with K4'
  bool lean_k2 = false;                // ... in its lean form (StepPlan::lean): nothing reads this detect's pair lists
};
struct DetectResult {
  bool pairs_done = false;   // K2 produced MVP's per-pair vectors
  bool rows_folded = false;  // ... and folded them per row (Ctx::mvp_rowdv)
  bool hk = false, hk_keep = false;  // the detect was host-decided / kept its list
  int64_t hk_m = 0;          // its number (the step's K4' publishes ring slot hk_m % kHkRing)
  bool k2_kept = false;      // K2 was kept (DetectRequest::keep_k2; not with bucket width 0):
  RankLaunch k2;             // its launch, and the timed detect's last stage event
  hipEvent_t k2_ev = nullptr;  // (or NULL) to record behind it
};
// detect = enqueue + finish, retried with the same request while a buffer overflowed
int detect(Ctx *c, const DetectRequest &q, int64_t *n_conf, int64_t *n_los);
bool nonfin_word(Ctx *c);  // Ctx::nonfin allocated (zeroed when new)
int detect_enqueue(Ctx *c, const DetectRequest &q, DetectResult *res);
int detect_finish(Ctx *c, bool *retry);
// the detect's and the resident step's A/B and diagnostic environment knobs
// (DESIGN.md 3.19), all read once at the first use of any of them.  None is a
// product setting.
struct DetectEnv {
  int home_rec;        // BSA_HOME_REC=0/1: home mode stores fp64 column records (-1: home_records' rule)
  bool stage1_t0;      // BSA_STAGE1_T0!=0: stage 1 at the t = 0 points, not the look-ahead midpoints
  bool tp_super;       // BSA_TP_SUPER=1: K0d as k_tilepairs (super-tiles) at every size
  bool k0z;            // BSA_K0Z=1: K0z always launched, never left to the last detect's K2
  bool tp_halo_all;    // BSA_TP_HALO_ALL=1: halo mode's K0d sweeps all column tiles, not the present ones
  bool tpr;            // BSA_TPR=0: no tile-pair list reuse
  bool hk_trace;       // BSA_HK_TRACE=1: one stderr line per host-known rebuild decision and step abort (diagnostics)
  double tpr_sh;       // BSA_TPR_SH>0: the kept list's horizontal budget [m]
  int pf_pieces;       // BSA_PF_PIECES=1/2/4/8: units per prefilter item
  int pf_heavy_t0;     // BSA_PF_HEAVY_T0=0..3: PfKnobs::t0
  int pf_pieces_near;  // BSA_PF_PIECES_NEAR=1/2/4/8: units per near item
  int fuse_exact;      // BSA_FUSE_EXACT=0/1: K1b fused into the prefilter (-1: detect_decide's rule)
  int ov_grid_a;       // BSA_OV_GRID_A: workgroups per CU of the overlap's own-tile sweep (<= 0: the whole grid)
  int k1b_grid;        // BSA_K1B_GRID>0: K1b's grid
  int pf_sym;          // BSA_PF_SYM=0/1/2: the highest sweep level a plan takes (DetectPlan::sym; unset: 2)
  // the resident step (bsa_sim.hip: step_decide)
  bool k24;            // BSA_K24=0: K2 and K4' as two launches
  int k4_block;        // BSA_K4_BLOCK=64/128/256: K4' workgroup size (anything else: 64)
  bool sim_prep;       // BSA_SIM_PREP=0: K4' does not prepare the next detect's records
  bool lean_k2;        // BSA_LEAN_K2=0: every detect of a batch places its pair lists (StepPlan::lean off)
};
const DetectEnv &detect_env();
#ifdef BSA_PF_TRACE
int pf_trace_dump(Ctx *c, unsigned long long groups, unsigned long long tiles);  // (diagnostic builds)
#endif
void grow_k2_bucket(Ctx *c, unsigned long long demand);

}  // namespace bsa
