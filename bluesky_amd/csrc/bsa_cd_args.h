// Conflict detection: the by-value argument structs and the constants that
// the host side (bsa_cd.hip) and the kernel units (bsa_k0.hip,
// bsa_prefilter.hip, bsa_rank.hip) share.
#pragma once
#include "bsa_halo.h"
#include "bsa_internal.h"
#include "bsa_prep.h"

namespace bsa {

// Candidate-list reuse.  A list built with every aircraft's
// reach inflated by its budgets (horizontal sh, vertical sv) stays a superset
// of the exact list while every aircraft's drift since the build stays inside
// them: drift_h = |dchord| * kRS * L + |dvel| * T, drift_v = |dalt| + |dvs| * T
// (L bounds the rotation of the refine's local basis, chord <= kRefineChord).
struct ReuseParams {
  const Snap *build;  // snapshot of the last build (nullptr: reuse off)
  Snap *cur;          // this detect's state (becomes the snapshot on a build)
  unsigned *ctl;      // [0] build flag (set here on a budget overrun), [1] detects since build
  float *use;         // per wave: largest horizontal / vertical budget fraction used
  float sh_chord;     // horizontal budget in chord units (added to the stage-1 reach)
  double sh;          // horizontal budget [m, refine units]
  double sv_default, sv_min, sv_max, ktarget;
  int valid;          // the snapshot belongs to this perm / parameters
};
constexpr double kRefineChord = 0.03;  // the refine keeps (without refining) pairs with a longer chord

constexpr int kWorkShards = 32;  // dequeue counters (4 per XCD group): a returning atomic on one
                                 // word saturates at ~88 dequeues/us (MI355X_MICROARCH 'dequeue')
constexpr int kWorkStride = 16;  // u64 words between counters (128 B apart)

// K2 with row buckets (k_rank_rows): one workgroup per kRankRows rows; the
// pair counts of every block (k_rowblk) follow the 2 (nrows + 1) per-row
// counts, so the row offsets need no scan with a look-back chain.  (K1b
// counting them with atomics, one per wave and block, cost 12 us at the 100k
// box: the per-block words were hit by every wave of a block's rows at once.)
#ifndef BSA_RANK_ROWS
#define BSA_RANK_ROWS 512
#endif
constexpr int kRankRows = BSA_RANK_ROWS;
static_assert(kRankRows % 64 == 0 && kRankRows <= 1024, "whole waves per K2 block");
constexpr int kRankLds = 3 * kRankRows;  // pairs per block folded from LDS (512 rows: 67 KB, 2 blocks per CU)
// lanes per workgroup of k_rank_rows: its rows take one lane each, its pairs
// (~1.7 per row at the 100k box) one lane each.  Two lanes per row place a
// block's pairs in one pass instead of two, but the 1024-lane workgroup caps
// the kernel at 128 VGPRs (7 spilled): K2 27.7 -> 29.0 us at the 100k box
// (A/B on one box, round 4), so one
#ifndef BSA_RANK_LANES_PER_ROW
#define BSA_RANK_LANES_PER_ROW 1
#endif
constexpr int kRankThreads = BSA_RANK_LANES_PER_ROW * kRankRows;
static_assert(kRankThreads <= 1024, "K2 workgroup size");
__host__ __device__ __forceinline__ int rank_blocks(int nrows) { return (nrows + kRankRows - 1) / kRankRows; }
__host__ __device__ __forceinline__ int rowcnt_words(int nrows) { return 2 * (nrows + 1) + 2 * rank_blocks(nrows); }

// Per-detect state to zero (k_zero, or fused into k_prep_cols: cnt != nullptr)
struct ZeroArgs {
  int nrows, full, keep;
  Counters *cnt;
  unsigned long long *work;
  unsigned char *inconf;
  unsigned long long *tcpamax;
  unsigned *rowcnt;
  unsigned *x[3];  // more word regions to zero (the halo plan's buffers: HaloPre), or NULL
  int xn[3];
};
// (NfArgs, the non-finite tcpa inputs' word and epoch: bsa_internal.h)


// K0c fused into K0b (no candidate-list reuse): the workgroup's kTile records
// are one tile, so the boxes are reduced right after the records are written.
struct FusedBoxes {
  TileBox *sbox, *gbox, *tbox;  // gbox == nullptr: not fused (k_boxes runs)
  TileBox *blk;                 // halo exchange: tile boxes also into the block sent (blk[tile - blk_base])
  int blk_base;
};

// Plan reuse (several ranks / the probe): the own-tile K0b
// compares each record it writes with the last build's and raises the rank's
// rebuild flag on the first one outside the budgets (snap == NULL: off)
struct TprCheck {
  const PFRec *snap;
  unsigned *flag;
  float dx, ds, dv;
  // HK (Ctx::hk_*): the prediction word of this detect, raised when a record
  // left f x every budget (the list is rebuilt two detects on), or NULL
  unsigned long long *pred;
  float f;
};

// ---- K0d tile pairs (bsa_k0.hip)
constexpr int kSlicesPerTile = kTile / kGroup;  // 64-row slices (work items) per row tile
static_assert(kSlicesPerTile == 8, "8 slices per tile (item bit layout, slice boxes = group boxes)");
constexpr unsigned kItemMirror = 1u << 31;  // item word 0: row tile (22 bits) | slice << 22 | triangular | mirrored
constexpr unsigned kItemTri = 1u << 30;     // (bits 25-29 are free)
constexpr int kTPDirectMax = 1024;  // column tiles up to which K0d runs direct (k_tilepairs_direct)
// Tile-pair list reuse: ctl == NULL -> off (the list is this
// detect's own); else K0d builds (grown boxes, snapshot of the records) only
// when forced by the host or flagged by the records' preparer (ctl[0]), and
// the prefilter publishes the built list's item counts (ctl[1], ctl[2])
struct TprArgs {
  unsigned long long *ctl;
  int force;
  float dx, ds, dv;
  const PFRec *pc;  // this detect's column records (rows = columns)
  PFRec *snap;
  unsigned *myflag;  // several ranks / the probe: the rank's rebuild flag, cleared here (the plan read it)
  // HK keep (the host kept the list; K0d is not launched): the prefilter takes
  // the kept item counts from ctl[1], ctl[2] and aborts the step
  // (Counters::tpr_stale) when the records' violation word vflag is set
  int keep;
  const unsigned *vflag;
  unsigned long long *stale;  // ... and records it for the batch (sim_ctl, kSimCtlStale)
};

// ---- K1b pair math (bsa_pair_math.h)
constexpr int kPayStride = 6;  // doubles per candidate record (cpay): key, qdr, dist, tcpa, tin, dcpa

// K1b fused into the prefilter (stored fp64 records, row
// buckets, not KWIK / candidate reuse): each prefilter workgroup evaluates the
// candidates it appended at the end of its sweep (they sit in its LDS stages),
// and the blocks its waves flushed mid-sweep (a full stage; recorded in LDS).
// A candidate's id (its cpay record, its
// bucket entries) is its slot in the candidate array, shard * ccap + position,
// not K1b's flat index -- K2 reads only what the buckets name.  The candidate
// list, every record and every bucket come out exactly as with K1b's launch
// (the list's order differs, which nothing downstream depends on: K2 ranks
// each row's bucket by column).  R == NULL: K1b runs as its own launch.
struct ExactFuse {
  const RowRec *R;                 // row records (the column records + roff when shared)
  const ColRec *C;                 // column records (sorted / home order)
  const unsigned *perm_r, *perm_c;  // sorted position -> index (perm_r NULL: home rows rb + x)
  double rpz, hpz, tla;
  int rb, nrows, B;
  double *cpay;
  unsigned *rowcnt;
  uint2 *kb;
  unsigned nrec;                   // flush records per wave (<= kFuseRecs; bsa_set_exact_fusion)
};

// ---- K1a prefilter (bsa_prefilter.hip)
constexpr int PF_BLOCK = 256;
constexpr int PF_WAVES = PF_BLOCK / 64;

struct RefineParams {
  float R;      // rpz [m]
  float H;      // hpz [m]
  float T;      // max(tla, 0) [s]
  float lim2;   // ((R + EABS) / (1 - E1) / R_S)^2 (unit-sphere units, as the refine's positions)
  float zero;   // 0 (diagnostic builds: -DBSA_PF_REFINE_X2 evaluates the refine twice)
};
constexpr float kRS = 6371000.f;   // scale of the unit-sphere chord to metres
constexpr float kE1 = 0.012f;      // bound on |log(reference dist / estimated dist)|
constexpr float kEABS = 50.f;      // absolute position error budget [m]
constexpr int PF_WROWS = 64;   // rows per wave (one per lane)
// fused K1b: mid-sweep flushes a wave can record for the end of its
// workgroup's sweep (each holds >= 65 candidates: >= 4 160 per wave; more sets
// Counters::fuse_ovf and the detect is retried with K1b's own launch)
constexpr int kFuseRecs = kFuseRecsMax;
constexpr int PF_ITEMS_PER_TILE = kTile / PF_WROWS;  // work items per tile pair
// Work distribution knob of the sweep (BSA_PF_SHARDS overrides it for
// measurements; results never depend on it)
struct PfKnobs {
  int pieces;  // units per item (tile pair, 64-row slice): 1, 2, 4 (or 8, BSA_PF_PIECES)
  int pnear;   // ... per near item (the pair's boxes overlap: the densest items)
  int t0;      // log2 of the listed top tier's pieces per near item's (HeavyArgs; BSA_PF_HEAVY_T0)
  // halo overlap (Ctx::ov_mode): 0 every item; 1 the items of the own column
  // tiles [ca0, ca1); 2 the others (the received tiles), with the dequeue
  // counters at word 8 of each shard's stride
  int ph, ca0, ca1;
};
// Longest items first (a kept tile-pair list): the sweep's
// span is set by its longest items (a dense item's refine runs up to ~60 us;
// one that starts late ends long after the median wave).  Every unit adds its
// duration to its list slot's cost; K1b lists the slots above a threshold for
// the next detect (consecutive detects sweep nearly the same pairs), whose
// prefilter dequeues those items first -- split as near items are -- and skips
// them among the regular units (flag == epoch).  Every slot is swept exactly
// once either way: results never depend on which items are listed.
// Two tiers: list 0 (the longest, cost >= thresh[0]) in twice a near item's
// pieces, list 1 (cost >= thresh[1]) split as near items are.
struct HeavyArgs {
  const unsigned *list[2];  // this detect's listed slots, or list[0] NULL (off)
  const unsigned *count;    // ... their numbers [2]
  unsigned *count_next;     // the next detect's [2], zeroed here (K1b appends)
  const unsigned *flag;     // per slot: == epoch -> listed this detect
  unsigned *cost;           // per slot: s_memrealtime ticks of its units (summed)
  unsigned epoch;
};
// (HeavyNext, the next detect's listing: bsa_internal.h, with RankLaunch)
#ifndef BSA_PF_WAVES_PER_EU
#define BSA_PF_WAVES_PER_EU 4
#endif
constexpr int PF_BLOCKS_PER_CU = BSA_PF_WAVES_PER_EU;  // resident workgroups per CU (4 waves each): LDS and VGPR limits

// One K0b launch (k_prep_cols; the records go to Ctx::colrec / pfcol / pfvcol
// / pfpcol).  The first block is the same at every launch of one detect
// (DetectRun::prep_cols); a launch site states what differs from the neutral
// values of the second.
struct PrepColsLaunch {
  int n = 0;
  const unsigned *perm = nullptr;
  int presorted = 1, rec = 0;
  SoA6 own{}, intr{};
  int distinct = 0, shared = 1;
  double rpz = 0.0, hpz = 0.0, tla = 0.0;
  int mid = 0;
  ReuseParams rz{};
  NfArgs nf{};

  FusedBoxes fb{};  // no fused K0c
  ZeroArgs zs{0, 1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, {}, {}};  // no fused K0z (only nrows set)
  int tile_base = 0;               // workgroup b < nown prepares tile tile_base + b,
  const int *tile_list = nullptr;  // the others slot b - nown of this list,
  HaloUnpack hu{};                 // unpacked from the exchange first,
  Counters *hcnt = nullptr;        // with a mismatch reported here
  TprCheck tck{};                  // no budget checks
  int nown = -1;                   // the whole grid
};

// One K1a launch (k_prefilter): rp and xf are the same at every launch of one
// detect; a launch site states the knobs and what differs from no list reuse
// and no listing
struct PrefilterLaunch {
  RefineParams rp;
  ExactFuse xf;
  PfKnobs kn;
  TprArgs tp{};
  HeavyArgs hv{};
};

}  // namespace bsa
