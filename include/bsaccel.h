/*
 * bsaccel.h -- C ABI of the MI355X-native BlueSky CD / MVP / kinematics path.
 *
 * One shared library (bluesky_amd/libbsaccel.so, HIP for gfx950) that the
 * Python drop-ins in bluesky_amd/ bind through ctypes.  Plain pointers and
 * sizes only; no exceptions cross the ABI.  Every entry point returns an int
 * status: 0 = OK, < 0 = error (message via bsa_last_error(ctx)).
 *
 * Reference interfaces replaced (paths relative to the BlueSky checkout):
 *   bsa_detect / bsa_fetch_pairs
 *       bluesky/traffic/asas/StateBasedCD.py:7-103   detect(ownship, intruder, RPZ, HPZ, tlookahead)
 *       bluesky/tools/geo.py:110-162                 qdrdist_matrix (fused, never materialised)
 *       bluesky/traffic/asas/src_cpp/casas.cpp:12-106 casas.detect (native variant it supersedes)
 *   bsa_mvp
 *       bluesky/traffic/asas/MVP.py:14-300           resolve / MVP / prioRules
 *   bsa_kinematics
 *       bluesky/traffic/traffic.py:425-483           UpdateAirSpeed / UpdateGroundSpeed / UpdatePosition
 *       bluesky/tools/aero.py:62-147                 vatmos / vtas2cas / vtas2mach (inlined)
 *   bsa_set_windfield (winddim 2)
 *       bluesky/traffic/windfield.py:158-179         Windfield.getdata, 2-D field
 *   bsa_set_windfield3d (winddim 3), bsa_wind_getdata
 *       bluesky/traffic/windfield.py:158-202         Windfield.getdata, 3-D field (per position)
 *   bsa_turb_draws, bsa_turb_apply, bsa_sim_set_turbulence
 *       bluesky/traffic/turbulence.py:24-46          Turbulence.Woosh (build-defined draws)
 *   bsa_area_inside, bsa_sim_set_areas
 *       bluesky/tools/areafilter.py:29-35,61-104     checkInside of Box / Circle / Poly / Line
 *   bsa_sim_set_sectors, bsa_sim_sectors_poll, bsa_sim_sectors_deleted
 *       plugins/sectorcount.py:53-96                 per-sector occupancy, arrived / left
 *   bsa_geovec_apply, bsa_sim_set_geovectors, bsa_sim_geovec_stats
 *       plugins/geovector.py:76-128                  applygeovec: speed, track and V/S limits per area
 *   bsa_qdrdist
 *       bluesky/tools/geo.py:110-162,347-363         qdrdist_matrix / kwikqdrdist_matrix, materialised
 *   bsa_sim_set_limits
 *       bluesky/traffic/pilot.py:65-68 + performance/openap/perfoap.py:185-209  applylimits (OpenAP)
 *   bsa_sim_acdata_*
 *       bluesky/simulation/qtgl/screenio.py:194-239  send_aircraft_data (ACDATA stream fields)
 *   bsa_sim_*     GPU-resident chain of the above, no reference equivalent
 *   bsa_comm_*    RCCL row-sharded multi-GPU mode, no reference equivalent
 *   bsa_scan_excl, bsa_flagged_list
 *       test seams of the device's exclusive scan and ordered index list, no reference equivalent
 *
 * Threading: a context is bound to one HIP device and one stream and is not
 * thread-safe; use one context per host thread (the BlueSky sim loop is
 * single-threaded, bluesky/network/detached.py:34-41).
 */
#ifndef BSACCEL_H
#define BSACCEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSA_ABI_VERSION 2

typedef struct bsa_ctx bsa_ctx;

/* detect flags */
#define BSA_FLAG_WITH_DCPA 1 /* also produce dcpa = sqrt(max(dcpa2,0)) per conflict */
#define BSA_FLAG_NOPRUNE   2 /* test aid: treat every pair as a candidate (disables the exact-safe prefilter) */
#define BSA_FLAG_RESORT    4 /* recompute the spatial order now (it is otherwise reused for up to
                                8 calls; results never depend on it, only the speed does) */
#define BSA_FLAG_KWIK      8 /* opt-in flat-earth variant: geo.kwikqdrdist_matrix
                                (geo.py:347-363) replaces qdrdist_matrix in StateBasedCD.detect, its
                                metre distance passed on in nm; qdr in [0, 360) */
#define BSA_FLAG_STAGE1_T0 16 /* test aid: prefilter stage 1 at the t = 0 positions with the full
                                look-ahead reach instead of the look-ahead midpoints (DESIGN.md
                                3.2b); results are identical, only the culling differs */

/* ---------------------------------------------------------------- lifecycle */

/* ABI version of the loaded library (== BSA_ABI_VERSION it was built with). */
int bsa_abi_version(void);

/* Number of visible HIP devices (>= 0), or < 0 on runtime error. */
int bsa_device_count(void);

/* Create a context on HIP device `device`.  Returns NULL on failure; the
 * reason is then available from bsa_last_error(NULL). */
bsa_ctx *bsa_create(int device);
void bsa_destroy(bsa_ctx *ctx);

/* Last error message of `ctx` (or of the failed bsa_create when ctx==NULL).
 * The string is owned by the library and valid until the next call. */
const char *bsa_last_error(const bsa_ctx *ctx);

/* Block until all work queued on the context's stream has finished. */
int bsa_sync(bsa_ctx *ctx);

/* ---------------------------------------------------------------- state
 * Replaces reading bs.traf.{lat,lon,trk,gs,alt,vs} inside StateBasedCD.detect
 * (StateBasedCD.py:16-17,30-37,65-69).  Host arrays are C-contiguous float64
 * of length n, borrowed for the duration of the call (copied to HBM).
 * Units as in bluesky Traffic: lat/lon/trk [deg], gs [m/s], alt [m], vs [m/s]. */
int bsa_set_state(bsa_ctx *ctx, int64_t n,
                  const double *lat, const double *lon, const double *trk,
                  const double *gs, const double *alt, const double *vs);

/* Optional distinct intruder set (detect(ownship, intruder, ...) with
 * intruder is not ownship).  n must equal the ownship n; n == 0 clears it
 * (intruder = ownship again).  Must be called after bsa_set_state. */
int bsa_set_intruder(bsa_ctx *ctx, int64_t n,
                     const double *lat, const double *lon, const double *trk,
                     const double *gs, const double *alt, const double *vs);

/* ---------------------------------------------------------------- detect
 * StateBasedCD.detect for ownship rows [row_begin, row_end) against all n
 * intruder columns (row_end <= 0 means n).  rpz/hpz in metres, tla in
 * seconds.  On success *n_conf / *n_los hold the number of conflict and
 * loss-of-separation pairs of these rows; the pairs stay on the device until
 * the next bsa_detect (bsa_mvp consumes them). */
int bsa_detect(bsa_ctx *ctx, double rpz, double hpz, double tla, int flags,
               int64_t row_begin, int64_t row_end,
               int64_t *n_conf, int64_t *n_los);

/* Copy the last detect's results to caller-allocated host arrays, in the
 * reference's row-major (i, j) order (StateBasedCD.py:93-101):
 *   ci, cj, qdr[deg], dist[m], tcpa[s], tinconf[s]       n_conf entries each
 *   dcpa[m] (n_conf, may be NULL; needs BSA_FLAG_WITH_DCPA)
 *   li, lj                                                n_los entries each
 *   inconf (uint8 0/1), tcpamax[s]                        row_end-row_begin entries
 * Any pointer may be NULL to skip that output.  Non-finite inputs follow the
 * reference (StateBasedCD.py:90): tcpamax is NaN on every row when some
 * column's position / velocity is not finite, and on one row when only that
 * row's is; the pairs are the finite aircraft's. */
int bsa_fetch_pairs(bsa_ctx *ctx,
                    int32_t *ci, int32_t *cj, double *qdr, double *dist,
                    double *tcpa, double *tinconf, double *dcpa,
                    int32_t *li, int32_t *lj,
                    uint8_t *inconf, double *tcpamax);

/* Candidate-pair count of the last detect (pairs that passed the
 * conservative prefilter and were evaluated exactly in fp64). */
int bsa_last_candidates(bsa_ctx *ctx, int64_t *n_candidates);

/* Candidate-list capacity (pairs surviving the prefilter) for the next
 * detects; rounded up to a multiple of the shard count.  Detects grow it on
 * overflow (with a retry), so this is a tuning / testing knob only.  Once the
 * resident sim's ASAS bookkeeping has started it also sets the resopairs
 * capacity (grown the same way). */
int bsa_set_candidate_capacity(bsa_ctx *ctx, int64_t capacity);

/* K2 (canonical order) row buckets: width w (1..64) pairs per row are
 * placed by K1b directly, K2 ranks each pair inside its row's bucket; a row
 * with more pairs makes the detect retry with a wider bucket (beyond 64: the
 * scatter into row segments, width 0).  Default 8.  Results never depend on
 * it (tests set it to exercise every path). */
int bsa_set_row_bucket(bsa_ctx *ctx, int width);
/* K1b (the exact fp64 evaluation of the prefilter's candidates) fused into
 * the prefilter's launch (on by default; stored records, row buckets, not
 * KWIK / candidate reuse): each prefilter workgroup evaluates the candidates
 * it produced at the end of its sweep.  max_records (0..64, default 64): the
 * mid-sweep flushes a wave records for that; a wave that flushes more makes
 * the detect retry with K1b as its own launch (0 forces that retry whenever
 * a wave flushes mid-sweep: a testing knob).  Results never depend on it. */
int bsa_set_exact_fusion(bsa_ctx *ctx, int on, int max_records);
/* [0] detects enqueued with K1b fused, [1] of them retried unfused (a wave ran
 * out of flush records), [2] whether the last detect fused (0 / 1). */
int bsa_exact_fusion_stats(bsa_ctx *ctx, int64_t *out3);
/* Symmetric prefilter sweep (on by default): when the rows
 * and the columns of a detect are the same aircraft (own == intruder, every
 * row, one rank; midpoint stage 1, not KWIK / NOPRUNE / candidate reuse) each
 * unordered pair of 512-aircraft tiles is listed and stage-1-tested once, and
 * its survivors are refined in both orientations.  `on` is a level: 0 sweeps
 * both orders, 1 is the above, 2 (a fresh context's) adds the triangular
 * sweep inside a diagonal tile pair (a 64-row slice skips the
 * column sub-groups below its own columns and refines the ones above them in
 * both orientations); any other value is refused.  Results never depend on
 * it (A/B; the BSA_PF_SYM=0 / 1 / 2 environment variable caps the level of
 * every context). */
int bsa_set_symmetric_sweep(bsa_ctx *ctx, int on);
/* [0] detects enqueued with the symmetric sweep, [1] the last detect's level
 * (0: both orders, 1 / 2 as above). */
int bsa_symmetric_sweep_stats(bsa_ctx *ctx, int64_t *out2);
/* Lean pair placement in the resident step (on by default):
 * in one bsa_sim_step call, every CD step that a later CD step of the same
 * call follows skips the global placement of its conflict / LoS pair lists
 * (and the launch that sums the blocks' pair counts for it) -- the later step
 * overwrites them before the host could read any.  Only where nothing on the
 * device reads them either: one rank, K2 fused with K4', no ASAS bookkeeping,
 * no stage that can stop a batch early.  The call's last CD step always places
 * them, so every result, count and statistic after the call is the same
 * (A/B; the BSA_LEAN_K2=0 environment variable turns it off in every context).
 * on = 2 is a testing aid: the call's last CD step runs lean too, after which
 * the pair lists, their counts and bsa_sim_stats' n_conf / n_los are NOT valid
 * (the state arrays are); any other value is refused. */
int bsa_set_lean_pairs(bsa_ctx *ctx, int on);
/* [0] CD steps since bsa_sim_init that ran lean, [1] that placed their lists. */
int bsa_lean_pairs_stats(bsa_ctx *ctx, int64_t *out2);
/* The prefilter items listed for the NEXT detect (longest items first,
 * DESIGN.md 3.2), tier 0 or 1: *count receives their number, slots[] (if
 * *count <= cap) their list slots in no particular order.  A testing aid. */
int bsa_listed_items(bsa_ctx *ctx, int tier, uint32_t *slots, int64_t cap, int64_t *count);
/* Candidate-list reuse across detects (own == intruder, whole row range, not
 * KWIK / NOPRUNE).  A detect that builds the list inflates
 * every aircraft's reach by a horizontal budget sigma_h [m] and a vertical
 * budget (sigma_v [m] at first, then adapted per aircraft to its own drift
 * rate, up to 4 sigma_v); later detects skip the sweep (K0c/K0d/K1a) and
 * re-evaluate that list exactly, until some aircraft's drift since the build
 * (position, velocity, altitude, vertical speed) exceeds its budget, a
 * re-sort, a parameter change or an overflow -- checked on the device, so the
 * results are identical to a full detect.  Off by default. */
int bsa_set_candidate_reuse(bsa_ctx *ctx, int on, double sigma_h, double sigma_v);
/* List builds and detects since the last bsa_timing_reset. */
int bsa_reuse_stats(bsa_ctx *ctx, int64_t *builds, int64_t *detects);
/* Largest fraction of its horizontal [0] / vertical [1] budget any aircraft
 * had used at the last detect (> 1 triggered a build; 0 after a forced one). */
int bsa_reuse_budget_use(bsa_ctx *ctx, double *use2);
/* Tile-pair list reuse in the resident sim step (on by
 * default): the detect's coarse cull -- which (512-row tile, 512-column tile,
 * 64-row slice) items the prefilter sweeps (K0d) -- is built on boxes grown by
 * sigma_h [m] horizontally (and proportionally in reach) and sigma_v [m]
 * vertically, and kept while every aircraft's prefilter record stays within
 * those distances of its record at the build (K4' checks each record it
 * prepares; the first one outside makes the next detect rebuild on the
 * device).  Every pair is still tested and evaluated at every detect, so the
 * results are identical with it on or off.  off: every detect builds. */
int bsa_set_tile_reuse(bsa_ctx *ctx, int on, double sigma_h, double sigma_v);
/* [0] tile-pair list builds, [1] detects that used the kept or a fresh list,
 * since the sim's first such detect (device counters). */
int bsa_tile_reuse_stats(bsa_ctx *ctx, int64_t *out2);
/* Host-known list decisions in the resident step (HK): on =
 * 0 lets the device decide every rebuild (the round-5 behaviour, one K0d /
 * halo plan launch per detect); f in (0, 4] is the fraction of the drift
 * budgets past which the device predicts a rebuild two detects ahead (f > 1:
 * predictions come late, kept lists go stale and their steps re-run -- a
 * testing knob).  Results never depend on either. */
int bsa_set_hk(bsa_ctx *ctx, int on, double f);
/* out6 = {host-kept detects, host-built detects, waits for a prediction,
 * stale aborts (re-run steps), device-decided detects after them, on} */
int bsa_hk_stats(bsa_ctx *ctx, int64_t *out6);
/* Halo overlap of the row-sharded resident step: on a detect
 * that keeps its halo plan, the halo send / recv, the received tiles' K0b and
 * the sweep of the halo column tiles run on a second stream while the own
 * tiles' K0b and sweep run; joined before K1b.  mode 0 off (default), 1
 * several ranks, 2 also the one-GPU probe (bsa_sim_probe_rank: its cost with
 * no exchange to hide).  Results never depend on it.  out: overlapped detects. */
int bsa_set_halo_overlap(bsa_ctx *ctx, int mode);
int bsa_halo_overlap_count(bsa_ctx *ctx, int64_t *out1);

/* Tile pairs (512 rows x 512 columns) of the last detect that survived the
 * bounding-box cull, the total number of tile pairs, and the number of
 * (64-row x 8-column) blocks the prefilter actually swept (each block is
 * BSA_PF_BLOCK_PAIRS stage-1 pair tests). */
#define BSA_PF_BLOCK_PAIRS 512
int bsa_last_tiles(bsa_ctx *ctx, int64_t *kept, int64_t *total, int64_t *groups);

/* Device time of the last detect's stages in milliseconds, measured with
 * HIP events on the context stream: [0] spatial order + records + tile cull,
 * [1] prefilter, [2] exact, [3] sort+gather, [4] whole detect. */
int bsa_last_timings(bsa_ctx *ctx, double *ms5);

/* Timing / statistics accumulation over many detects (benchmarking): reset
 * forgets every recorded detect; summary waits for the stream and returns the
 * MEAN stage durations over the detects since the reset (same layout as
 * bsa_last_timings) and the SUMS stats4 = {(64-row x 16-column) prefilter
 * blocks swept, candidates, surviving tile pairs, detects}. */
int bsa_timing_reset(bsa_ctx *ctx);
int bsa_timing_summary(bsa_ctx *ctx, double *ms5, int64_t *stats4);
/* Record the stage events of one detect in `every` (default 1 = all; 0 =
 * none; counted from the last bsa_timing_reset, whose first detect is timed).
 * Each event record costs a ~5 us gap before the next kernel, so the bench
 * samples; bsa_last_timings then reports the last timed detect and
 * bsa_timing_summary averages the timed ones. */
int bsa_set_timing_sample(bsa_ctx *ctx, int every);

/* ---------------------------------------------------------------- MVP
 * MVP.resolve (bluesky/traffic/asas/MVP.py:14-143) on the device-resident
 * conflict pairs of the last bsa_detect (rows [row_begin,row_end) of it).
 * Scalars as held by ASAS (asas.py:81-112): Rm = R*mar, dhm = dh*mar, vmin/
 * vmax/vsmin/vsmax in m/s; switches 0/1; priocode one of BSA_PRIO_* (any
 * other value = a code prioRules does not know: no change). */
#define BSA_PRIO_NONE 0
#define BSA_PRIO_FF1  1
#define BSA_PRIO_FF2  2
#define BSA_PRIO_FF3  3
#define BSA_PRIO_LAY1 4
#define BSA_PRIO_LAY2 5
typedef struct bsa_mvp_params {
  double Rm, dhm, dtlookahead, vmin, vmax, vsmin, vsmax;
  int32_t swresohoriz, swresospd, swresohdg, swresovert;
  int32_t swprio, priocode;
  int32_t swnoreso, swresooff;
} bsa_mvp_params;

/* Load externally detected conflict pairs (e.g. from the numpy StateBasedCD)
 * as if they were the last detect's, for all n rows: P pairs in confpair
 * order with ci non-decreasing (row-major, as detect returns them), and their
 * qdr [deg], dist [m], tcpa [s], tLOS [s] (MVP.py:33). */
int bsa_set_pairs(bsa_ctx *ctx, int64_t P, const int32_t *ci, const int32_t *cj,
                  const double *qdr, const double *dist, const double *tcpa,
                  const double *tlos);

/* Inputs (host, length n = state n): gseast, gsnorth, selalt, apvs (= traf.ap.vs),
 * noreso / resooff: uint8 per aircraft (membership of asas.noresolst /
 * asas.resoofflst; NULL = empty list).  vs/alt/trk/gs come from bsa_set_state.
 * asas_alt: persistent asas.alt of the detect rows, read-modify-write.
 * Outputs (detect rows): asas.trk, asas.tas, asas.vs, asas.asase/asasn (float32). */
int bsa_mvp(bsa_ctx *ctx, const bsa_mvp_params *p,
            const double *gseast, const double *gsnorth, const double *selalt,
            const double *apvs, const uint8_t *noreso, const uint8_t *resooff,
            double *asas_alt, double *trk, double *tas, double *vs,
            float *asase, float *asasn);

/* ---------------------------------------------------------------- kinematics
 * Traffic.UpdateAirSpeed + UpdateGroundSpeed + UpdatePosition
 * (bluesky/traffic/traffic.py:425-483) for n aircraft, one fused kernel.
 * winddim 0 = no wind, 1 = constant wind (windnorth/windeast m/s,
 * windfield.py:150-152), 2 = the context's 2-D wind field (bsa_set_windfield;
 * windnorth/windeast ignored), 3 = the context's 3-D wind field
 * (bsa_set_windfield3d; windnorth/windeast ignored).  Host arrays of length n; state arrays are updated
 * in place; output pointers may be NULL. */
typedef struct bsa_kin_io {
  /* inputs */
  const double *ptas, *phdg, *palt, *pvs; /* pilot.tas/hdg/alt/vs */
  const double *bank, *eps, *accel;       /* traf.bank, traf.eps, perf.acceleration() */
  /* state, in/out */
  double *tas, *hdg, *alt, *vs, *lat, *lon;
  /* outputs */
  double *ax, *delspd, *cas, *mach, *gsnorth, *gseast, *gs, *trk, *coslat, *az;
  uint8_t *swhdgsel, *swaltsel;
} bsa_kin_io;

int bsa_kinematics(bsa_ctx *ctx, int64_t n, double simdt, int winddim,
                   double windnorth, double windeast, bsa_kin_io *io);

/* 2-D wind field for winddim 2 (bsa_kinematics and the resident sim):
 * Windfield.getdata's inverse-distance-squared interpolation
 * (bluesky/traffic/windfield.py:158-179) over nvec definition points at
 * lat/lon [deg] with wind vnorth/veast [m/s] (Windfield.vnorth[0, :] /
 * veast[0, :], as WindSim.addpoint stores them).  Evaluated per aircraft at
 * its pre-step position, for both Pilot.APorASAS (pilot.py:31-35) and
 * UpdateGroundSpeed (traffic.py:463).  Altitude profiles are the 3-D field
 * below.  nvec = 0 clears the field.  Host arrays are copied. */
int bsa_set_windfield(bsa_ctx *ctx, int64_t nvec, const double *lat, const double *lon,
                      const double *vnorth, const double *veast);

/* 3-D wind field for winddim 3 (bsa_kinematics, the resident sim,
 * bsa_wind_getdata): Windfield.getdata with altitude profiles
 * (bluesky/traffic/windfield.py:158-202).  The reference's getdata raises for
 * array arguments longer than one (windfield.py:177 takes the truth value of
 * an array comparison) but evaluates one position at a time; the pin is that
 * per-aircraft result.  The 2-D field's horizontal weights, then
 *   idxalt = max(0, min((nalt-1)*altstep - 1e-20, alt) / altstep),
 *   ialt = floor(idxalt), falt = idxalt - ialt,
 *   vn = (1-falt) * sum_k vnorth[ialt,k] horfact_k + falt * sum_k vnorth[ialt+1,k] horfact_k
 * (veast alike), at each aircraft's pre-step position and altitude.
 * vnorth / veast: Windfield.vnorth / veast as WindSim.addpoint leaves them,
 * nalt x nvec doubles, row-major (Windfield: nalt = 451, altstep = 100 ft).
 * Build-defined: ialt is clamped into [0, nalt-2] before any table read, so
 * alt >= (nalt-1)*altstep (where the reference raises IndexError) gives the
 * top level's wind and a NaN altitude a NaN wind; nothing outside the table is
 * ever read.  nvec >= 1, nalt >= 2, altstep > 0; nvec = 0 clears the field.
 * Stored apart from the 2-D field; winddim selects which one is read.  Host
 * arrays are copied.  May be called between steps of a resident sim (a
 * weather reload); no kept detect state depends on the field. */
int bsa_set_windfield3d(bsa_ctx *ctx, int64_t nvec, int64_t nalt, double altstep,
                        const double *lat, const double *lon,
                        const double *vnorth, const double *veast);

/* Windfield.getdata at n host-given positions -- the array form the reference
 * lacks for 3-D fields (its callers: traffic.py:280,355, autopilot.py:336).
 * winddim 1: the 2-D field's first point everywhere (windfield.py:150-152),
 * 2: the 2-D field, 3: the 3-D field (alt [m]; ignored and may be NULL
 * otherwise).  vn_out / ve_out: n doubles [m/s]. */
int bsa_wind_getdata(bsa_ctx *ctx, int winddim, int64_t n, const double *lat, const double *lon,
                     const double *alt, double *vn_out, double *ve_out);

/* ---------------------------------------------------------------- geo matrices
 * Standalone materialised producers of
 *   geo.qdrdist_matrix(lat1, lon1, lat2, lon2)      bluesky/tools/geo.py:110-162
 *   geo.kwikqdrdist_matrix(lata, lona, latb, lonb)  bluesky/tools/geo.py:347-363 (BSA_GEO_KWIK)
 * as called outside the CD (traffic/metric.py:596,711,1188 with 1 x m / 1 x n
 * np.matrix operands; traffic/asas/SSD.py:169 with 1-D arrays, i.e.
 * element-wise pairs).  qdr [deg] (KWIK: [0, 360)), dist [nm] (KWIK: metres,
 * as the reference returns them).
 *   outer  (default): out[i*n + j] for i < m, j < n.  qdrdist needs m == n or
 *          m == 1 (its `(lat1 == 0.)*1e-6` term is added to the n-vector
 *          lat2, geo.py:128); KWIK needs m == n (its cavelat is indexed
 *          [j, i], geo.py:355).  Other shapes make the reference broadcast to
 *          a different result shape and are rejected (BSA_EINVAL).
 *   BSA_GEO_PAIRWISE: out[k] for k < m, m == n (1-D operands: every product
 *          of the reference is element-wise).
 * Host arrays are borrowed (float64); qdr / dist are caller-allocated
 * (m*n or m doubles); either may be NULL.  The outputs go through HBM and back
 * over PCIe; bsa_geo_last_ms reports the device time of the producing kernel
 * alone (HIP events on the context stream). */
#define BSA_GEO_KWIK     1
#define BSA_GEO_PAIRWISE 2
int bsa_qdrdist(bsa_ctx *ctx, int64_t m, const double *lat1, const double *lon1,
                int64_t n, const double *lat2, const double *lon2, int flags,
                double *qdr, double *dist);
int bsa_geo_last_ms(bsa_ctx *ctx, double *ms);

/* ---------------------------------------------------------------- multi-GPU
 * One process per GPU, one context per process.  Rank r owns the home rows
 * [r*rpr, min(n, (r+1)*rpr)) of the resident sim, rpr = ceil(n/R) rounded up
 * to a multiple of 512 (a spatially compact chunk of the traffic, SURVEY.md
 * 8e).  Before each CD step every rank receives only the column tiles its rows
 * can reach (a halo exchange: box all-gather, then grouped RCCL send / recv of
 * those tiles' state over xGMI), not the whole state.  No
 * reference equivalent (the reference's only distributed backend,
 * bluesky/network/ ZMQ, is out of scope). */
#define BSA_UNIQUE_ID_BYTES 128
/* Create a communicator id on one rank (ncclGetUniqueId); ship its 128 bytes
 * to the other ranks out of band. */
int bsa_comm_unique_id(char *id128);
int bsa_comm_init(bsa_ctx *ctx, int nranks, int rank, const char *id128);
/* In-process group: several contexts in ONE process form the ranks of a
 * row-sharded sim, each driven by its own host thread, exchanging with
 * device-to-device copies ordered by HIP events (RCCL refuses two ranks on one
 * GPU; this runs the nranks > 1 paths on one GPU and lets one process drive
 * several).  Create the group, then every rank joins it from its thread; the
 * group is freed by bsa_group_destroy once no context is joined any more
 * (destroying it earlier defers the free to its last member's leaving). */
typedef struct bsa_group bsa_group;
bsa_group *bsa_group_create(int nranks);  /* NULL if nranks is not in [1, 16] */
void bsa_group_destroy(bsa_group *g);
int bsa_comm_init_group(bsa_ctx *ctx, bsa_group *g, int rank);
/* Collective: element-wise max of `count` host doubles over all ranks, in
 * place (also a barrier).  Without a communicator it is a no-op. */
int bsa_comm_allreduce_max(bsa_ctx *ctx, double *values, int count);
/* Collective: element-wise sum of `count` host doubles over all ranks. */
int bsa_comm_allreduce_sum(bsa_ctx *ctx, double *values, int count);
/* The communicator as its transport sees it (not collective): info4 =
 * {transport (0 none, 1 RCCL, 2 in-process group), ranks, this rank, device}.
 * With RCCL the ranks / rank / device come from RCCL itself (ncclCommCount,
 * ncclCommUserRank, ncclCommCuDevice), so a report of N ranks is RCCL's. */
int bsa_comm_info(bsa_ctx *ctx, int *info4);

/* C2 pair gather ("pair lists are gathered to the host").
 * Collective over the ranks' last detect (bsa_detect on each rank's row
 * slice, or the resident sim's last CD call): totals3 = {conflict pairs, LoS
 * pairs, rows} summed over all ranks (the root sizes its arrays from them);
 * then bsa_gather_pairs moves every rank's results to `root` and concatenates
 * them in rank order, which is the reference's global row-major order
 * (StateBasedCD.py:93-101) since ranks own contiguous row blocks.  Arrays as
 * in bsa_fetch_pairs (inconf / tcpamax: one entry per row of all ranks); any
 * pointer may be NULL; `out` is read on the root only (dcpa is meaningful
 * only when the detects used BSA_FLAG_WITH_DCPA). */
typedef struct bsa_pairs_out {
  int32_t *ci, *cj;
  double *qdr, *dist, *tcpa, *tinconf, *dcpa;
  int32_t *li, *lj;
  uint8_t *inconf;
  double *tcpamax;
} bsa_pairs_out;
int bsa_gather_counts(bsa_ctx *ctx, int64_t *totals3);
int bsa_gather_pairs(bsa_ctx *ctx, int root, const bsa_pairs_out *out);

/* ---------------------------------------------------------------- GPU-resident sim
 * The synthetic sim step of SURVEY.md 8d with all state resident in HBM:
 *   every cd_every steps: [halo exchange] -> detect (own rows) -> MVP (own rows,
 *                         only if any rank has a conflict, asas.py:486-487)
 *                         -> asas.active = inconf, or (resume_nav = 1) the ASAS
 *                         bookkeeping + ResumeNav (asas.py:409-504) on the device
 *   every step:           Pilot.APorASAS (pilot.py:28-63, winddim 0/1) fused with
 *                         UpdateAirSpeed/GroundSpeed/Position (traffic.py:425-483)
 * AP targets, selalt, bank, eps and perf.acceleration() are frozen inputs.
 * Every array crosses this ABI in aircraft-index order.  On the device the
 * sim keeps them in HOME order (the spatial order of the state at
 * bsa_sim_init): rank r owns the home range [row_begin, row_end) of
 * bsa_sim_stats (512-aligned, spatially compact), whose aircraft indices
 * bsa_sim_row_ids lists; "this rank's rows" below are those aircraft, in
 * ascending index (all of 0..n-1 with one rank). */
typedef struct bsa_sim_params {
  double simdt, rpz, hpz, tla;
  int32_t cd_every; /* >= 1: CD + MVP every k steps (1 = DTNOLOOK=simdt, 20 = asas_dt/simdt) */
  int32_t reso;     /* 1: RESO MVP (MVP.py:14-143); 0: RESO OFF, the reference's default CR
                       (asas.py:41,76-77): DoNothing.resolve (DoNothing.py:11-20) copies the
                       autopilot targets into asas.trk/tas/vs/alt when there are confpairs.
                       Either way asas.active = inconf, or ResumeNav's with resume_nav = 1 */
  bsa_mvp_params mvp;
  int32_t winddim;  /* 0 = no wind, 1 = constant wind (windfield.py:150-152), 2 = 2-D field
                       (bsa_set_windfield), 3 = 3-D field (bsa_set_windfield3d): the wind branches of Pilot.APorASAS
                       (pilot.py:31-36,51-61) and UpdateGroundSpeed */
  int32_t resume_nav; /* 1: ASAS.update bookkeeping on the device: resopairs, ResumeNav's
                         asas.active (asas.py:409-471) and the unique / cumulative pair
                         counts (asas.py:490-502); 0: asas.active = inconf */
  double windnorth, windeast; /* [m/s] */
} bsa_sim_params;

typedef struct bsa_sim_state {
  const double *lat, *lon, *alt, *tas, *hdg, *vs, *gs, *trk, *gseast, *gsnorth;
  const double *ap_trk, *ap_tas, *ap_alt, *ap_vs, *selalt, *bank, *eps, *accel;
  const double *asas_alt; /* initial asas.alt (asas.py:405-409 sets it to traf.alt) */
} bsa_sim_state;

typedef struct bsa_sim_out {
  double *lat, *lon, *alt, *tas, *hdg, *vs, *gs, *trk, *gseast, *gsnorth;
  double *asas_trk, *asas_tas, *asas_vs, *asas_alt;
  uint8_t *active;
} bsa_sim_out;

/* Upload the full state (length n, all ranks pass the same) and parameters. */
int bsa_sim_init(bsa_ctx *ctx, int64_t n, const bsa_sim_state *s, const bsa_sim_params *p);
/* Advance nsteps; collective when a communicator is set.  With conditional
 * commands on (bsa_sim_set_conditions) the call returns 0 after fewer steps
 * when a condition fired: bsa_sim_steps_run says how many ran.  After such a
 * stopped batch the "last detect" of bsa_sim_stats / bsa_fetch_pairs is one
 * made on the state the stop left by the steps enqueued behind it (which
 * changed nothing else) -- with cd_every > 1 possibly at a step count at which
 * single steps would not have detected. */
int bsa_sim_step(bsa_ctx *ctx, int nsteps);
/* Pilot.applylimits with the OpenAP model (pilot.py:65-68 ->
 * performance/openap/perfoap.py:185-209) inside the step, between
 * Pilot.APorASAS and UpdateAirSpeed (traffic.py:397-407): the pilot's tas /
 * vs / alt are clipped to a per-aircraft envelope (full-n host arrays, copied:
 * hmax [m], vmin / vmax [m/s CAS], vsmin / vsmax [m/s], axmax [m/s^2]), the
 * vertical-speed cap scaled by (1 - ax/axmax) with ax = traf.ax of the
 * previous step (0 after bsa_sim_init).  The envelope is a frozen input here;
 * OpenAP's per-phase envelope update (perfoap.py:115-183) is bsa_sim_set_perf,
 * which takes precedence.  hmax == NULL switches the limits off (the default
 * after bsa_sim_init). */
int bsa_sim_set_limits(bsa_ctx *ctx, const double *hmax, const double *vmin, const double *vmax,
                       const double *vsmin, const double *vsmax, const double *axmax);
/* OpenAP.update (performance/openap/perfoap.py:115-131) inside the step:
 * each aircraft's flight phase is inferred from its pre-step vs / alt
 * (phase.py:14-62), its envelope looked up in its type's row at that phase
 * (__construct_limit_matrix, perfoap.py:211-262) and applied as
 * bsa_sim_set_limits does, and UpdateAirSpeed's acceleration is
 * OpenAP.acceleration() (2 m/s^2 in phase GD, else 0.5; perfoap.py:271-280)
 * instead of the frozen accel.  table: ntypes rows of 24 doubles -- vmin by
 * phase NA..GD (9), vmax by phase (9), vsmin, vsmax, hmax, axmax, lifttype
 * (1 fixed wing, 2 rotor, 0 other), 0 (bluesky_amd/perf.py builds it from the
 * reference's Coefficient tables); type_idx: full-n row per aircraft
 * (validated).  Takes precedence over bsa_sim_set_limits; table == NULL
 * switches it off (the default after bsa_sim_init).  bsa_sim_create stays
 * refused while it is on (bsa_sim_create_with takes the new aircraft's type_idx). */
int bsa_sim_set_perf(bsa_ctx *ctx, int64_t ntypes, const double *table, const int32_t *type_idx);
/* This rank's rows of the flight phase of the last step
 * (0..8, phase.py:4-12; needs bsa_sim_set_perf) and of traf.ax, written into
 * full-n host arrays; either pointer may be NULL. */
int bsa_sim_read_perf(bsa_ctx *ctx, uint8_t *phase, double *ax);
/* The second half of OpenAP.update (perfoap.py:133-173): zero-lift drag
 * coefficient by flight phase, drag (fixed wing: rhovs (cd0 + k cl^2); tas == 0
 * gives NaN as numpy does), thrust ratio (thrust.py:5-129: take-off, in-flight
 * by altitude segment, 15 % of it in descent, else 0), thrust, fuel flow
 * engnum (a tr^2 + b tr + c) [kg/s] and the model's own bank limit (15 deg in
 * TO / LD, 35 in IC / CR / AP, else unchanged; it does not feed traf.bank).
 * Rotors and lift type 0 keep the reference's zeros (cd0 = cd0_clean).
 * table: the ntypes x 24 type table of bsa_sim_set_perf; ftable: ntypes rows
 * of 16 doubles -- Sref, engnum, engthrust, engbpr, ff_a, ff_b, ff_c,
 * cd0_clean, cd0_gd, cd0_to, cd0_ic, cd0_ap, cd0_ld, k, default mass, 0
 * (bluesky_amd/perf.py force_table builds it; ntypes <= 384); type_idx: row
 * per aircraft; phase: 0..8 per aircraft (phase.py:4-12), or NULL to derive
 * it from vs / alt as the step does; mass [kg], tas, vs, alt: length n.
 * Outputs: length n; bank holds the previous perf.bank on entry. */
int bsa_openap_forces(bsa_ctx *ctx, int64_t n, int64_t ntypes, const double *table, const double *ftable,
                      const int32_t *type_idx, const uint8_t *phase, const double *mass, const double *tas,
                      const double *vs, const double *alt, double *cd0, double *drag, double *thrustratio,
                      double *thrust, double *fuelflow, double *bank);
/* The same inside the resident step, on the pre-step state (OpenAP.update runs
 * before the pilot and the kinematics, traffic.py:397-404), in a launch of its
 * own at the start of every step; nothing in the step reads its outputs.
 * Needs bsa_sim_set_perf (its type index and lift types; ntypes must be its
 * row count, engnum x engthrust finite for fixed wings); mass: full-n host
 * array [kg], constant as in the reference.  Switching on zeroes the outputs,
 * perf.bank and the fuel burnt.  ftable == NULL switches it off (the default),
 * and so does every bsa_sim_set_perf call.  bsa_sim_delete carries the arrays
 * along; bsa_sim_create stays refused while bsa_sim_set_perf is on
 * (bsa_sim_create_with takes the new aircraft's mass and keeps the others' fuel).
 * Fuel burnt (an extension, not in the reference): per aircraft, the sum over
 * the completed steps, in step order, of that step's fuelflow x simdt [kg] --
 * exact through aborted and re-run steps (each step counted once). */
int bsa_sim_set_forces(bsa_ctx *ctx, int64_t ntypes, const double *ftable, const double *mass);
/* This rank's rows of the last step's outputs and of the fuel burnt, into
 * full-n host arrays (rows as bsa_sim_row_ids); any pointer may be NULL. */
int bsa_sim_read_forces(bsa_ctx *ctx, double *cd0, double *drag, double *thrustratio, double *thrust,
                        double *fuelflow, double *bank, double *fuel_used);
/* Autopilot LNAV / VNAV guidance and waypoint switching on the device: one
 * full Autopilot.update call with a forced FMS tick (autopilot.py:59-203, with
 * ActiveWaypoint.Reached / calcturn, Route.getnextwp on a route table,
 * ComputeVNAV and geo.qdrdist) for n aircraft in host arrays.
 *
 * The FMS state of the aircraft, arrays of length n.  Doubles: traf.actwp's
 * nine arrays, ap.dist2vs / vnavvs / swvnavvs (0 or 1), traf.selspd / selvs /
 * apvsdef; uint8 flags: traf.swlnav / swvnav / abco / belco.  selvs, apvsdef,
 * abco and belco are only read. */
typedef struct bsa_fms_state {
  double *actwp_lat, *actwp_lon, *actwp_nextaltco, *actwp_xtoalt, *actwp_spd, *actwp_vs, *actwp_turndist,
      *actwp_flyby, *actwp_next_qdr;
  double *dist2vs, *vnavvs, *swvnavvs, *selspd, *selvs, *apvsdef;
  uint8_t *swlnav, *swvnav, *abco, *belco;
} bsa_fms_state;
/* route_rows: nrows x 8 doubles, one waypoint per row: lat, lon [deg], alt [m]
 * (< 0: none), spd [CAS m/s or Mach] (-999: none), xtoalt, toalt [m] (the
 * route's wpxtoalt / wptoalt after Route.calcfp), flyby (1 / 0), nextqdr (the
 * bearing to the following waypoint, -999 for the last).  Aircraft k owns rows
 * [rt_off[k], rt_off[k] + rt_n[k]) and flies to its row iactwp[k]; rt_n 0 (no
 * route) needs swlnav 0 and iactwp -1 or 0.  Every index is range-checked here, before anything
 * is launched.  lat .. bank: the traffic state the call reads (bank [rad]).
 * In and out: iactwp, *st, and the autopilot's targets ap_trk / ap_alt / ap_vs
 * and traf.selalt; out: ap_tas. */
int bsa_fms_update(bsa_ctx *ctx, int64_t n, int64_t nrows, const double *route_rows, const int32_t *rt_off,
                   const int32_t *rt_n, int32_t *iactwp, const double *lat, const double *lon, const double *alt,
                   const double *tas, const double *gs, const double *trk, const double *ax, const double *bank,
                   const bsa_fms_state *st, double *ap_trk, double *ap_tas, double *ap_alt, double *ap_vs,
                   double *selalt);
/* Waypoint recovery (asas.py:459-465): Route.findact (route.py:1043-1079) and
 * Route.direct (route.py:635-688, with the whole of ComputeVNAV) applied
 * count[k] >= 0 times in sequence to aircraft k -- once per resopair that
 * ResumeNav dropped for it in one call.  Arrays and range checks as
 * bsa_fms_update (traf.ax is not read).  In and out: iactwp, ap_alt and of *st
 * actwp_lat / lon / nextaltco / xtoalt / spd / vs / turndist / flyby, dist2vs,
 * selspd, swlnav; everything else is read only, and an aircraft with count 0
 * or no route keeps every value.  direct goes to the waypoint's index, which
 * is the reference's lookup by name for a route with unique names. */
int bsa_fms_recover(bsa_ctx *ctx, int64_t n, int64_t nrows, const double *route_rows, const int32_t *rt_off,
                    const int32_t *rt_n, int32_t *iactwp, const double *lat, const double *lon, const double *alt,
                    const double *tas, const double *gs, const double *trk, const double *bank,
                    const bsa_fms_state *st, double *ap_alt, const int32_t *count);
/* The same inside the resident step, on the pre-step state (ap.update is the
 * first call of Traffic.update, traffic.py:395), in a launch of its own at the
 * start of every step, so that resident aircraft follow their routes with no
 * host work inside a batch.  Arrays as bsa_fms_update, full-n host arrays in
 * aircraft-index order; the traffic state and ap_trk / ap_tas / ap_alt / ap_vs /
 * selalt are the sim's own.  simt: the time of the next step; t0: Autopilot.t0
 * (-999. at start).  The context advances simt by simdt per step and ticks by
 * the reference's rule (autopilot.py:61-62); a step that does not tick only
 * evaluates ap.tas.  Exact through aborted and re-run batches.  route_rows ==
 * NULL switches it off (the default); a second call replaces everything.
 * bsa_sim_delete carries the arrays along on one rank and is refused on
 * several; bsa_sim_create is refused while it is on (bsa_sim_create_with
 * takes the new aircraft's routes and state, on one rank). */
int bsa_sim_set_fms(bsa_ctx *ctx, int64_t nrows, const double *route_rows, const int32_t *rt_off, const int32_t *rt_n,
                    const int32_t *iactwp, const bsa_fms_state *st, double simt, double t0);
/* Waypoint recovery inside the resident step (off by default): every CD step
 * with resume_nav = 1 applies bsa_fms_recover's findact + direct to this rank's
 * rows right after ResumeNav, once per resopair it dropped, on the pre-step
 * state and before the step's Pilot.APorASAS reads ap.alt.  Refused while
 * bsa_sim_set_fms is off; bsa_sim_set_fms(NULL) switches it off; inert with
 * resume_nav = 0.  Exact through aborted and re-run batches. */
int bsa_sim_set_recovery(bsa_ctx *ctx, int on);
/* Resopairs ResumeNav dropped per ownship in the last CD call (resume_nav = 1),
 * this rank's rows into a full-n host array: bsa_asas_out.dropped as a count. */
int bsa_sim_read_dropcount(bsa_ctx *ctx, int32_t *count);
/* ---------------------------------------------------------------- turbulence
 * Turbulence.Woosh (bluesky/traffic/turbulence.py:24-46): position noise along
 * the flight direction, the wing direction and the vertical.  The reference
 * draws from numpy's global Mersenne state; here the draws are build-defined:
 * aircraft `index` of call number `call` owns one Philox4x64-10 block,
 *   counter = {index, call, 0, 0}, key = {seed, 0}      -> words w0..w3
 *   u_i = ((w_i >> 11) + 0.5) * 2^-53                    (never 0)
 *   z0 = sqrt(-2 log u0) cos(2 pi u1), z1 = sqrt(-2 log u0) sin(2 pi u1),
 *   z2 = sqrt(-2 log u2) cos(2 pi u3)
 * and turbhf, turbhw, turbalt = (sd[k] * sqrt(dt)) * z_k.  A pure function of
 * (seed, call, index): no state, any order, any partition.  sd: three finite
 * values >= 0, clamped like Turbulence.SetStandards (sd > 1e-6 ? sd : 1e-6).
 *
 * bsa_turb_draws: indices first_index .. first_index + n - 1 of one call.
 * raw4n (4 n words, index-major; may be NULL) and z3n (3 n unit normals,
 * index-major: z0 z1 z2 per index). */
int bsa_turb_draws(bsa_ctx *ctx, int64_t n, uint64_t seed, uint64_t call, uint64_t first_index,
                   uint64_t *raw4n, double *z3n);
/* One Woosh over host arrays of length n: alt += turbalt, lat +=
 * degrees(turblat / Rearth), lon += degrees(turblon / Rearth / coslat) with
 * turblat / turblon the draws rotated by trk [deg]; coslat as traf.coslat
 * (traffic.py:482).  hf / hw / valt: the unit normals to apply (all three), or
 * all NULL: aircraft i takes the draw of (seed, call, i).  lat / lon / alt are
 * updated in place. */
int bsa_turb_apply(bsa_ctx *ctx, int64_t n, double dt, const double *sd3, const double *hf, const double *hw,
                   const double *valt, uint64_t seed, uint64_t call, const double *trk, const double *coslat,
                   double *lat, double *lon, double *alt);
/* Woosh as the last stage of every resident step (off by default;
 * traffic.py:416): after the step's position update, on this rank's rows, with
 * dt = simdt, the post-step trk and the coslat UpdatePosition left; an
 * aircraft's index is its current one (bsa_sim_row_ids; after bsa_sim_delete the
 * compacted one).  The host keeps the call number: 0 at bsa_sim_init, + 1 per
 * step while on.  While on, the step prepares no records for the next detect
 * and keeps no tile-pair list on one rank; each detect makes its records from
 * the perturbed state.  Exact through aborted and re-run
 * batches.  Several ranks: every rank calls it alike.  sd3 is checked also
 * when on = 0. */
int bsa_sim_set_turbulence(bsa_ctx *ctx, int on, const double *sd3, uint64_t seed);
/* The call number of the next step's draws: set from *set_to when not NULL
 * (>= 0; continuing another sim's stream), then stored to *call when not NULL. */
int bsa_sim_turb_call(bsa_ctx *ctx, int64_t *call, const int64_t *set_to);
/* ---------------------------------------------------------------- conditional commands
 * Condition.update (bluesky/traffic/conditional.py:25-49; ATALT / ATSPD).  A
 * condition is (idx, type, target, lastdif): the aircraft's index, type 0 =
 * altitude / 1 = speed, the target [m or m/s CAS] and the difference at the
 * last update.  Per condition, in numpy's order:
 *   actual  = (type == 0) * alt[idx] + (type == 1) * cas[idx]
 *   actdif  = target - actual;  fired = actdif * lastdif <= 0;  lastdif = actdif
 * A condition with lastdif == 0 fires at the next update whatever the state; a
 * non-finite product never fires.
 *
 * bsa_cond_update: one update over host arrays (idx / type / target / lastdif
 * of ncond conditions, alt / cas of n aircraft).  lastdif is rewritten; fired
 * (room for ncond) receives the fired conditions' numbers in ascending order
 * (np.where's), *count how many.  Every idx and type is checked first;
 * ncond = 0 launches nothing. */
int bsa_cond_update(bsa_ctx *ctx, int64_t ncond, const int32_t *idx, const int32_t *type, const double *target,
                    double *lastdif, int64_t n, const double *alt, const double *cas, int32_t *fired,
                    int64_t *count);
/* cond.update() as the last stage of every resident step (traffic.py:419; off
 * by default, ncond = 0 switches it off).  idx is the aircraft index
 * (bsa_sim_row_ids); speed conditions compare vtas2cas(tas, the altitude before
 * the step's position update), altitude conditions the altitude the step left
 * (turbulence included).  A step in which a condition fires is completed, the
 * fired conditions are dead from then on (delcondition) and the batch STOPS
 * after it: bsa_sim_step returns 0 having run fewer steps (bsa_sim_steps_run),
 * and the host executes the commands before it steps on.  One rank only:
 * refused when a communicator of several ranks is set. */
int bsa_sim_set_conditions(bsa_ctx *ctx, int64_t ncond, const int32_t *idx, const int32_t *type, const double *target,
                           const double *lastdif);
/* Steps the last bsa_sim_step call ran (fewer than asked when a stage stopped
 * the batch) and the sim's step count; either pointer may be NULL.  After a
 * stopped batch the last detect's counts and pair lists describe the state
 * the stop left (see bsa_sim_step), not the last completed step's own detect. */
int bsa_sim_steps_run(bsa_ctx *ctx, int64_t *last_batch, int64_t *total);
/* The conditions that fired at the last stop, ascending, as numbers of the table
 * before this call (as uploaded, or as the last poll / delete left it); *step:
 * the step count at which they fired.  Then the dead conditions leave the
 * table, the rest keep their order (delcondition).  *count > cap: nothing is
 * written or consumed.  Without a stop since the last poll *count = 0. */
int bsa_sim_cond_poll(bsa_ctx *ctx, int64_t cap, int32_t *fired, int64_t *count, int64_t *step);
/* The live table, lastdif included (any array may be NULL; *count > cap:
 * nothing written).  bsa_sim_delete applies Condition.delac to it
 * (conditional.py:108-128): one deleted aircraft after another in ascending
 * order, each removing its conditions and shifting the indices above it down;
 * bsa_sim_create leaves it alone. */
int bsa_sim_read_conditions(bsa_ctx *ctx, int64_t cap, int32_t *idx, int32_t *type, double *target, double *lastdif,
                            int64_t *count);
/* ---------------------------------------------------------------- area filter
 * areafilter.checkInside (bluesky/tools/areafilter.py:29-35) for a table of
 * shapes in one launch.  A shape (areafilter.py:52-104):
 *   BSA_AREA_LINE    never inside
 *   BSA_AREA_BOX     c = lat, lon, lat, lon of two opposite corners (any order):
 *                    lat0 <= lat <= lat1 & lon0 <= lon <= lon1, inclusive
 *   BSA_AREA_CIRCLE  c = clat, clon, r [NM]: geo.kwikdist(clat, clon, lat, lon) <= r
 *                    (geo.py:288-305, its operation order)
 *   BSA_AREA_POLY    nvert ring vertices from vertex voff of `verts` ((lat, lon)
 *                    pairs, fp64): matplotlib's Path.contains_points with x = lat,
 *                    y = lon -- an even-odd crossing count over the ring closed from
 *                    its last vertex to its first; for each edge (x0,y0)->(x1,y1):
 *                      f0 = (y0 >= y); f1 = (y1 >= y)
 *                      if f0 != f1 and (((y1 - y)*(x0 - x1) >= (x1 - x)*(y0 - y1)) == f1): inside ^= 1
 *                    A ring of fewer than 3 vertices holds nothing, and a point
 *                    with a non-finite lat or lon is in no polygon.
 * and bottom <= alt <= top for all but LINE (top / bottom in either order:
 * areafilter.py:64-65).  fp64, no contraction.  blat / blon are the library's
 * (cull bounds); what the caller writes there is ignored. */
#define BSA_AREA_LINE   0
#define BSA_AREA_BOX    1
#define BSA_AREA_CIRCLE 2
#define BSA_AREA_POLY   3
typedef struct bsa_area_shape {
  int32_t type;
  int32_t nvert; /* POLY: >= 1 */
  int64_t voff;  /* POLY: first vertex */
  double top, bottom;
  double c[4];
  double blat[2], blon[2];
} bsa_area_shape;
#define BSA_AREA_NOCULL 1 /* test aid: every shape for every point (no wave-level cull; also env BSA_AREA_CULL=0);
                             results are identical, only the speed differs */
/* n points (host arrays) against nshapes shapes (<= 1024) over nvert vertices
 * (verts: 2 nvert doubles, <= 65536 vertices).  out_words: W = ceil(nshapes /
 * 64) arrays of n 64-bit words, word-major: bit s % 64 of out_words[(s / 64) * n
 * + i] = point i is inside shape s.  counts (nshapes words, may be NULL): points
 * inside each shape.  Errors (bsa_last_error): NULL arrays, n < 0, a table
 * beyond the limits, an unknown type, a polygon of fewer than 1 vertex, of a
 * vertex range outside the array or of a non-finite vertex, an unknown flag. */
int bsa_area_inside(bsa_ctx *ctx, int64_t n, const double *lat, const double *lon, const double *alt,
                    int64_t nshapes, const bsa_area_shape *shapes, int64_t nvert, const double *verts, int flags,
                    uint64_t *out_words, uint64_t *counts);
/* ---------------------------------------------------------------- sector occupancy
 * plugins/sectorcount.py:53-96 inside the resident step (off by default; nothing
 * is launched while off).  bsa_sim_set_areas uploads the sim's area table
 * (shapes / verts as for bsa_area_inside, same checks and limits; nshapes = 0
 * clears it) and forgets the sectors, which name its shapes. */
int bsa_sim_set_areas(bsa_ctx *ctx, int64_t nshapes, const bsa_area_shape *shapes, int64_t nvert,
                      const double *verts);
/* nsect sectors (<= 64: one mask word per aircraft; 0 = off), sector k the
 * shape shape_idx[k] of the table.  SECTORCOUNT ADD (sectorcount.py:91-96): the
 * previous masks are seeded with one inside pass at the current state, whose
 * occupancy the next poll reports with nothing arrived or left.  A step counter
 * starts at 0 here; after the last stage of each step that brings it to a
 * multiple of `every` (>= 1; the caller's max(update_interval, simdt) / simdt,
 * tools/plugin.py:127) the pass runs on this rank's rows: the current masks,
 * per sector n_tot, arrived = now & ~before, left = before & ~now for this
 * update and summed (64-bit) since this call; the current masks then become the
 * previous ones.  The pass only reads simulation state, and it is exact through
 * aborted and re-run batches (each update counted once).  The mask words are
 * per-aircraft arrays: bsa_sim_create (new aircraft: 0, outside), bsa_sim_delete
 * and the re-partition on several ranks carry them.  Several ranks: every rank
 * calls it alike and counts its own rows; the caller sums. */
int bsa_sim_set_sectors(bsa_ctx *ctx, int64_t nsect, const int32_t *shape_idx, int64_t every);
/* The LAST update, this rank's rows.  Per sector (nsect words each, any may be
 * NULL): n_tot, arrived, left, and arrived_total / left_total since
 * bsa_sim_set_sectors (every update, also those inside a batch).  *step: the
 * step count (since bsa_sim_set_sectors) of that update, 0 = the seeding pass;
 * *updates: how many there were.  cur_words / prev_words (may be NULL): bit k =
 * inside sector k at the last update / at the one before, this rank's rows of
 * full-n host arrays in aircraft-index order (bsa_sim_row_ids names the rows;
 * other entries are left alone). */
int bsa_sim_sectors_poll(bsa_ctx *ctx, uint64_t *n_tot, uint64_t *arrived, uint64_t *left, uint64_t *arrived_total,
                         uint64_t *left_total, int64_t *step, int64_t *updates, uint64_t *cur_words,
                         uint64_t *prev_words);
/* Aircraft of this rank's rows that bsa_sim_delete removed while sectors were
 * on ("left by deletion", sectorcount.py's set difference): pos[k] = position in
 * that call's index list, words[k] = the masks it had.  *count = how many are
 * pending; they are copied and forgotten when cap >= *count, else left for a
 * call with room.  Read it after each bsa_sim_delete: positions of two calls
 * are not told apart. */
int bsa_sim_sectors_deleted(bsa_ctx *ctx, int64_t cap, int64_t *pos, uint64_t *words, int64_t *count);
/* ---------------------------------------------------------------- experiment area
 * The AREA plugin (plugins/area.py:85-220): flight statistics per aircraft and
 * the deletes at the boundary.  One Area.update over host arrays of n aircraft
 * (area.py:112-142), in the reference's order, fp64:
 *   returns at once when swtaxi and not active;
 *   resultantspd = sqrt(gs*gs + vs*vs);  distance2D += dt*gs;
 *   distance3D += dt*resultantspd;  work += (thrust*dt)*resultantspd
 *   (thrust NULL: work stays);
 *   !swtaxi: delidxalt = where((oldalt >= swtaxialt) * (alt < swtaxialt)), then
 *   oldalt = alt;
 *   delidx = where(inside * !inside_now), inside = inside_now, with inside_now
 *   the area filter's test of `shape` (its polygon ring in verts[nvert][2]);
 *   shape NULL is Area.name None: everything is outside.
 * inside: one byte per aircraft (0 / 1), updated like the fp64 arrays.  Both
 * lists are ascending (np.where's order) and hold at most n entries.  n == 0
 * launches nothing. */
int bsa_exparea_update(bsa_ctx *ctx, int64_t n, const double *gs, const double *vs, const double *alt,
                       const double *lat, const double *lon, const double *thrust, double *distance2D,
                       double *distance3D, double *work, double *oldalt, uint8_t *inside, double dt,
                       const bsa_area_shape *shape, int64_t nvert, const double *verts, int active, int swtaxi,
                       double swtaxialt, int32_t *delidx, int64_t *ndel, int32_t *delidxalt, int64_t *ndelalt);
/* The same update as the resident step's last stage (after the conditions), in
 * the steps that bring the count of steps since the first enabling call to a
 * multiple of `every` (every = max(dt, simdt) / simdt; dt itself is the
 * plugin's nominal interval, which the accumulators use).  shape_idx: a shape
 * of bsa_sim_set_areas, or -1 for none.  It reads the state the step left and
 * the thrust of that step's bsa_sim_set_forces launch (forces off: work stays
 * 0).  The first call with on != 0 starts the arrays as Area.create does for
 * every aircraft: accumulators 0, oldalt = alt, create_time = simt, inside all
 * false -- an aircraft must be seen inside once before it can exit; later calls
 * change the parameters only; on == 0 switches the stage off.  bsa_sim_delete
 * and bsa_sim_create carry the arrays (new aircraft: oldalt = their alt,
 * create_time = the last bsa_sim_exparea_simt); bsa_sim_set_areas forgets the
 * shape (set it again).  A step in which an aircraft exits or sinks through
 * swtaxialt completes, then the batch stops as for a fired condition (see
 * bsa_sim_step / bsa_sim_steps_run); the deletes themselves are the caller's.
 * While on, bsa_sim_step takes at most 2^24 - 1 steps per call.  One rank only. */
int bsa_sim_set_exparea(bsa_ctx *ctx, int on, int32_t shape_idx, double dt, int64_t every, double simt, int active,
                        int swtaxi, double swtaxialt);
int bsa_sim_exparea_simt(bsa_ctx *ctx, double simt);
/* The deletes of the last stop: delidx (exits) and delidxalt (taxi deletes),
 * aircraft indices ascending; *step: the step count of that stop.  records:
 * 19 doubles per exited aircraft, in delidx's order -- create_time distance2D
 * distance3D work lat lon alt tas vs hdg asas.active, then ap alt tas vs trk
 * and asas alt tas vs trk (the pilot's select is the caller's).  A count above
 * cap: nothing is written or consumed.  Without a stop with deletes since the
 * last poll both counts are 0. */
int bsa_sim_exparea_poll(bsa_ctx *ctx, int64_t cap, int32_t *delidx, int64_t *ndel, int32_t *delidxalt,
                         int64_t *ndelalt, double *records, int64_t *step);
/* The arrays by aircraft index, n long each (any may be NULL). */
int bsa_sim_read_exparea(bsa_ctx *ctx, double *distance2D, double *distance3D, double *work, double *oldalt,
                         double *create_time, uint8_t *inside);
/* ---------------------------------------------------------------- trails
 * traffic/trails.py: Trails.update(t).  While active, every aircraft i (in
 * ascending index order, np.where's) with t - lasttim[i] > dt -- strict; a NaN
 * delta selects nothing -- emits the segment (lastlat[i], lastlon[i], lat[i],
 * lon[i], t) and then takes lat[i], lon[i], t as lastlat / lastlon / lasttim.
 * While inactive lastlat / lastlon take the positions and lasttim takes t;
 * nothing is emitted.  Every number of a segment is a copy.
 * bsa_trails_update: one update over host arrays; lastlat, lastlon and lasttim
 * are updated in place.  The segments go to lat0 .. time and idx (the emitting
 * aircraft), cap entries each, *count of them.  n == 0 launches nothing; a
 * count above cap is an error that names both numbers (the arrays are then
 * left as they were). */
int bsa_trails_update(bsa_ctx *ctx, int64_t n, const double *lat, const double *lon, double *lastlat,
                      double *lastlon, double *lasttim, double t, double dt, int active, int64_t cap, double *lat0,
                      double *lon0, double *lat1, double *lon1, double *time, int32_t *idx, int64_t *count);
/* The same update as a stage of every resident step, after the conditions and
 * before the experiment area: trails.update(simt) is the last statement of
 * Traffic.update.  t is the simt the step started at (the stage's own clock:
 * `simt` here, + simdt per step, accumulated in fp64 as simulation.py does);
 * the positions are those the step leaves.  The segments collect on the device
 * in emission order until bsa_sim_trails_drain; a batch neither synchronises
 * nor copies for them.  The first call with on != 0 starts lastlat / lastlon at
 * the current positions and lasttim at lasttim[] (n values by aircraft index:
 * the time of the update that preceded a TRAIL ON is simt - simdt); later calls
 * change active / dt / max_segments only, and active = 0 after active = 1 drops
 * the undrained segments as setTrails(False) does.  on == 0 switches the stage
 * off.  bsa_sim_delete and bsa_sim_create carry the arrays; of m new aircraft
 * only the LAST starts at its position, the others at (0, 0), all at lasttim 0
 * (Trails.create).  bsa_sim_step sizes the segment buffers before it enqueues:
 * undrained + n * min(k, floor(k * simdt / dt) + 1) for k steps, and refuses
 * the call, running nothing, when that exceeds max_segments (drain, or step
 * less).  One rank only. */
int bsa_sim_set_trails(bsa_ctx *ctx, int on, int active, double dt, double simt, const double *lasttim,
                       int64_t max_segments);
/* The segments since the last drain, in emission order (idx: the aircraft's
 * index when it emitted), and optionally lastlat / lastlon by aircraft index (n
 * long; may be NULL).  *count above cap: nothing is written or consumed.
 * Resets the device's total (clearnew()).  Synchronises. */
int bsa_sim_trails_drain(bsa_ctx *ctx, int64_t cap, double *lat0, double *lon0, double *lat1, double *lon1,
                         double *time, int32_t *idx, int64_t *count, double *lastlat, double *lastlon);
/* The arrays by aircraft index (n long each; any may be NULL), the stage's
 * clock (*simt: the t of the next step's update, *last_t: that of the last
 * step's) and the undrained segment count as of the last batch or drain. */
int bsa_sim_read_trails(bsa_ctx *ctx, double *lastlat, double *lastlon, double *lasttim, double *simt,
                        double *last_t, int64_t *undrained);
/* ---------------------------------------------------------------- ADS-B model
 * traffic/adsbmodel.py: ADSB.update(time).  An aircraft is due when
 * lastupdate + trunctime < time -- strict, false for a NaN.  For a due aircraft
 * the picture's trk, tas, gs, vs are copies of the traffic's; lat, lon, alt are
 * copies too, or with noise x + (0 + sigma z): sigma = transerror[0] [deg] for
 * lat and lon, transerror[1] [m] for alt, z a unit normal; two roundings, as
 * numpy's.  Then lastupdate += trunctime (not = time).  Nothing of an aircraft
 * that is not due is written.
 * The normals are build-defined: Philox4x64-10, counter {index, call, stream,
 * 0}, key {seed, 0}; stream 1 gives the update's three normals (lat, lon, alt;
 * the Box-Muller pairs of bsa_turb_draws), stream 2 create's uniform (word 0);
 * stream 0 is turbulence's.  per_aircraft == 0 (the reference: it draws ONE
 * normal per quantity per call, shared by every due aircraft): index 0.
 * per_aircraft == 1: the aircraft's index, first_index + its position here.
 * bsa_adsb_draws: the words (4 n), normals (3 n) and uniforms (n) of indices
 * first_index .. of `call` in stream 1 or 2; any output may be NULL.
 * bsa_adsb_update: one update over host arrays; lastupdate and the seven
 * picture arrays are updated in place.  draws: the unit normals to apply
 * instead -- 3 values (shared) or lat | lon | alt, n each (per aircraft) -- or
 * NULL.  transerror and trunctime must be finite and >= 0. */
int bsa_adsb_draws(bsa_ctx *ctx, int64_t n, uint64_t seed, uint64_t call, uint64_t first_index, int stream,
                   uint64_t *raw4n, double *z3n, double *un);
int bsa_adsb_update(bsa_ctx *ctx, int64_t n, double time, double trunctime, int noise, const double *transerror,
                    int per_aircraft, const double *draws, uint64_t seed, uint64_t call, uint64_t first_index,
                    const double *lat, const double *lon, const double *alt, const double *trk, const double *tas,
                    const double *gs, const double *vs, double *lastupdate, double *alat, double *alon, double *aalt,
                    double *atrk, double *atas, double *ags, double *avs);
/* The same update as a stage of every resident step, where Traffic.update runs
 * it (traffic.py:392): on the state the previous step left, after a geovector
 * application and before the FMS stage, on this rank's rows.  time is the
 * stage's clock: `simt` here, + simdt per step, accumulated in fp64.  The call
 * number of the draws starts at 0 and grows by one per step with noise on.
 * The first call with on != 0 starts the picture at the current state -- vs
 * too, where ADSB.create leaves 0 -- and lastupdate at lastupdate[] (n values
 * by aircraft index); later calls change noise, transerror, trunctime, seed and
 * per_aircraft only (lastupdate may be NULL).  on == 0 switches the stage off
 * and frees its arrays; off, a step launches nothing for it.  bsa_sim_delete
 * and bsa_sim_create carry the arrays; a new aircraft starts with lastupdate =
 * -trunctime u (u: stream 2 at its index and the current call number), the
 * picture at its state and vs 0.  An aborted batch repeats nothing: the stage
 * keeps two lastupdate buffers, reads one and writes the other.  Sharded: every
 * rank calls it alike; per-aircraft draws depend on the aircraft index only. */
int bsa_sim_set_adsb(bsa_ctx *ctx, int on, int noise, const double *transerror, double trunctime, uint64_t seed,
                     int per_aircraft, double simt, const double *lastupdate);
/* This rank's rows of the arrays, by aircraft index in n-long arrays (other
 * entries untouched; any may be NULL), the stage's clock (*simt: the time of the
 * next step's update) and the call number of its draws. */
int bsa_sim_read_adsb(bsa_ctx *ctx, double *lastupdate, double *lat, double *lon, double *alt, double *trk, double *tas,
                      double *gs, double *vs, double *simt, int64_t *call);
/* The call number of the next noisy update (*call, after setting it from
 * *set_to if given; either may be NULL). */
int bsa_sim_adsb_call(bsa_ctx *ctx, int64_t *call, const int64_t *set_to);
/* ---------------------------------------------------------------- geovectoring
 * plugins/geovector.py:76-128: per area an allowed interval for ground speed,
 * track and vertical speed.  The geovectors are an ordered list; each is
 * applied to every aircraft before the next, so a later one reads what an
 * earlier one wrote (per aircraft a sequential fold: one lane per aircraft).
 * For an aircraft inside the geovector's shape (the area filter's test), in
 * this order:
 *   GSMIN  casmin = vtas2cas(gsmin, alt); selspd < casmin: selspd = casmin
 *   GSMAX  casmax = vtas2cas(gsmax, alt); selspd > casmax: selspd = casmax
 *   TRK    degto180(trk - trkmin) < 0: ap_trk = trkmin; then
 *          degto180(trk - trkmax) > 0: ap_trk = trkmax   (the max wins)
 *          degto180(a) = (a + 180) % 360 - 180, numpy's %
 *   VSMIN  vs < vsmin: selvs = vsmin, selalt = alt + sign(vsmin) * 200 ft
 *   VSMAX  vs > vsmax: selvs = vsmax, selalt = alt + sign(vsmax) * 200 ft
 * trk, vs and alt are the traffic's and are never written; no comparison with a
 * NaN is true.  The reference switches a limit on by Python truth, so a bound of
 * exactly 0 is "off" there: `given` says which limits are on, and a given bound
 * (for TRK either of the two) that is exactly 0 is refused here.  An aircraft
 * that no limit changes keeps its four values bit for bit. */
#define BSA_GEOVEC_GSMIN 1
#define BSA_GEOVEC_GSMAX 2
#define BSA_GEOVEC_TRK   4 /* both track bounds */
#define BSA_GEOVEC_VSMIN 8
#define BSA_GEOVEC_VSMAX 16
#define BSA_GEOVEC_MAX   256 /* geovectors per call / per sim */
typedef struct bsa_geovec {
  int32_t shape; /* index into the shape table */
  int32_t given; /* BSA_GEOVEC_* bits */
  double gsmin, gsmax, trkmin, trkmax, vsmin, vsmax; /* m/s, deg, m/s */
} bsa_geovec;
/* n aircraft (host arrays) under ngv geovectors (<= BSA_GEOVEC_MAX) over the
 * shape table (as for bsa_area_inside, same checks and limits).  selspd, ap_trk,
 * selvs and selalt are read and written in place.  flags: BSA_AREA_NOCULL (test
 * aid; results identical).  changed (4 words, may be NULL): aircraft whose
 * selspd / ap_trk / selvs / selalt differs bitwise from what came in.  Errors,
 * all before any launch: NULL arrays, n < 0, ngv beyond the limit, a shape index
 * outside the table, unknown `given` bits, a given bound that is exactly 0, an
 * unknown flag, and the table's own errors. */
int bsa_geovec_apply(bsa_ctx *ctx, int64_t n, const double *lat, const double *lon, const double *alt,
                     const double *trk, const double *vs, int64_t nshapes, const bsa_area_shape *shapes,
                     int64_t nvert, const double *verts, int64_t ngv, const bsa_geovec *gv, int flags,
                     double *selspd, double *ap_trk, double *selvs, double *selalt, uint64_t *changed);
/* Geovectoring inside the resident step (off by default; nothing is launched
 * while off; ngv = 0: off).  gv[k].shape names a shape of bsa_sim_set_areas'
 * table; selspd / selvs are the FMS state's (bsa_sim_set_fms), ap_trk / selalt
 * the sim's: refused while the sim has no area table or no guidance.
 * bsa_sim_set_areas forgets the geovectors, bsa_sim_set_fms(NULL) switches them
 * off.  The stage is the plugin's preupdate (tools/plugin.py:127-132,161-169):
 * the first launch of a step, on this rank's rows of the pre-step state, at the
 * start of every step before which a positive multiple of `every` (>= 1; an
 * integer count of steps, the caller's max(update_interval, simdt) / simdt) steps
 * have completed since this call -- the first application comes one interval
 * after loading.  Exact through aborted and re-run batches: an applying launch
 * first saves the four arrays' rows, and an aborted applying step gets them back
 * (after the FMS undo set).  None of the four arrays is a detect input.  Several
 * ranks: every rank calls it alike and applies to its own rows. */
int bsa_sim_set_geovectors(bsa_ctx *ctx, int64_t ngv, const bsa_geovec *gv, int64_t every);
/* *applies: applications in completed steps since bsa_sim_set_geovectors;
 * changed4_total (4 words): this rank's aircraft whose selspd / ap_trk / selvs /
 * selalt an application changed, summed over them.  Either may be NULL.  An
 * error while geovectoring is off. */
int bsa_sim_geovec_stats(bsa_ctx *ctx, int64_t *applies, uint64_t *changed4_total);
/* This rank's rows (bsa_sim_row_ids) of the FMS state, iactwp and the
 * autopilot's targets into full-n host arrays, the clock and the number of
 * ticks since bsa_sim_set_fms; any pointer may be NULL. */
int bsa_sim_read_fms(bsa_ctx *ctx, const bsa_fms_state *st, int32_t *iactwp, double *ap_trk, double *ap_tas,
                     double *ap_alt, double *ap_vs, double *selalt, double *simt, double *t0, int64_t *ticks);
/* Traffic.update's atmosphere, traf.p / rho / Temp = vatmos(traf.alt) on the
 * pre-step altitude (traffic.py:389, aero.py:62-74), computed inside the step
 * when on (off after bsa_sim_init: nothing in the step reads them; a host
 * performance model in hybrid mode does).  _read: this rank's rows of the last
 * step into full-n host arrays [Pa, kg/m3, K]; any pointer may be NULL. */
int bsa_sim_set_atmos(bsa_ctx *ctx, int on);
int bsa_sim_read_atmos(bsa_ctx *ctx, double *p, double *rho, double *temp);
/* Overwrite per-aircraft arrays of the resident sim (full-n host arrays, all
 * ranks pass the same) while keeping the ASAS bookkeeping (resopairs, the
 * previous call's pair sets, asas.active / trk / tas / vs) and traf.ax: the
 * hybrid mode where the host simulator (autopilot, performance model, stack
 * commands) changes traffic between steps (traffic.py:383-404 runs them
 * before Traffic.update's kinematics).  NULL pointers leave that array as it
 * is; asas_alt overwrites the persistent asas.alt. */
int bsa_sim_update(bsa_ctx *ctx, const bsa_sim_state *s);
/* Traffic.create for the resident sim (traffic.py:192-312 + ASAS.create,
 * asas.py:402-407): append m aircraft whose state is s (m-long host arrays,
 * every field required); asas.trk / tas start at trk / tas, asas.alt at
 * s->asas_alt, asas.vs / active / traf.ax at 0.  They take indices n..n+m-1.
 * Fails while OpenAP limits are on (set them again after).  Collective with
 * several ranks (all pass the same arrays): every rank's replicas are completed
 * first, the rows re-partitioned over the new n afterwards (each rank keeps
 * the bookkeeping of its new range). */
int bsa_sim_create(bsa_ctx *ctx, int64_t m, const bsa_sim_state *s);
/* bsa_sim_create while the envelope, OpenAP and the autopilot guidance run
 * (DESIGN.md 3.15): the same append, plus the new aircraft's rows of every such
 * stage that is on.  x holds one part per stage, m-long host arrays each: the
 * six envelope arrays (bsa_sim_set_limits on), type_idx (bsa_sim_set_perf on:
 * rows of its table), mass (bsa_sim_set_forces on), and for bsa_sim_set_fms
 * the new aircraft's waypoints (nrows x 8, may be none), rt_off relative to
 * them, rt_n, iactwp and st, as bsa_sim_set_fms takes them for all aircraft.
 * A stage that is on needs its part; a part (any of its pointers, or nrows)
 * given for a stage that is off is an error; x == NULL is no part at all, so
 * with none of the four on this is bsa_sim_create.  Everything is validated on
 * the host before anything is enqueued -- type_idx inside the table (whose
 * every row bsa_sim_set_forces has checked), each route inside route_rows,
 * iactwp inside its route (without a route: -1 or 0, and LNAV off), flags 0 or
 * 1, no NULL -- and a refused call leaves the sim as it was.  New aircraft
 * start with phase 0 as after bsa_sim_set_perf, and with the six force
 * outputs, perf.bank and the fuel burnt at 0 as after bsa_sim_set_forces; the
 * others keep everything, fuel burnt included.  route_rows is appended to the
 * device's route table (which only grows: deleted aircraft leave holes) and
 * rt_off rebased; simt, t0, the tick count and bsa_sim_set_recovery stay.
 * Several ranks: collective as bsa_sim_create with the envelope, perf and
 * forces parts (the re-partition carries their arrays); refused with guidance
 * on, as bsa_sim_delete is. */
typedef struct bsa_sim_create_extra {
  const double *hmax, *vmin, *vmax, *vsmin, *vsmax, *axmax; /* limits on (set_limits form): m each */
  const int32_t *type_idx;                                  /* perf on: m rows of the type table */
  const double *mass;                                       /* forces on: m */
  int64_t nrows;
  const double *route_rows;                                 /* fms on: the new aircraft's waypoints, nrows x 8 */
  const int32_t *rt_off, *rt_n, *iactwp;                    /* m each; rt_off relative to route_rows */
  const bsa_fms_state *st;                                  /* m-long arrays */
} bsa_sim_create_extra;
int bsa_sim_create_with(bsa_ctx *ctx, int64_t m, const bsa_sim_state *s, const bsa_sim_create_extra *x);
/* Traffic.delete for the resident sim (traffic.py:364-378 ->
 * trafficarrays.py:99-117): remove the k aircraft idx[0..k) (any order,
 * duplicates ignored); the rest keep their order and shift down, as np.delete
 * does.  The ASAS bookkeeping follows the reference's callsign-keyed sets:
 * resopairs of a deleted ownship go; a resopair whose intruder was deleted
 * stays (bsa_sim_resopairs reports idx2 = -1) until the next CD call's
 * ResumeNav switches the ownship's ASAS off and drops it (asas.py:419-468).
 * Removing every aircraft is an error (re-init instead).  Collective with
 * several ranks (all pass the same list), re-partitioned as bsa_sim_create. */
int bsa_sim_delete(bsa_ctx *ctx, int64_t k, const int64_t *idx);
/* Full-n host copies of the state (collective: gathers all ranks' rows).
 * Any pointer may be NULL. */
int bsa_sim_read(bsa_ctx *ctx, bsa_sim_out *o);
/* [0] steps done, [1] CD calls, [2] conflicts and [3] LoS pairs of the last
 * CD call (this rank's rows), [4] this rank's row_begin, [5] row_end (its home
 * range: row_end - row_begin rows; (0, n) with one rank). */
int bsa_sim_stats(bsa_ctx *ctx, int64_t *out6);
/* Batches of bsa_sim_step / bsa_sim_cd that aborted (a buffer overflowed, a kept
 * list went stale) and were re-run from the aborted step, since bsa_sim_init. */
int bsa_sim_aborts(bsa_ctx *ctx, int64_t *aborts);
/* The aircraft indices of this rank's rows, ascending (row_end - row_begin
 * entries): the rows of bsa_sim_acdata_poll's arrays, of bsa_fetch_pairs'
 * inconf / tcpamax after resident steps, and of bsa_sim_read_perf. */
int bsa_sim_row_ids(bsa_ctx *ctx, int32_t *ids);
/* Measurement aid: the sim's detect (home order, its rpz / hpz / tla) of the
 * home rows [row_begin, row_end) (row_begin a multiple of 512) against all
 * columns -- one rank's share of a CD step, on one GPU, as that rank computes
 * it: its own column tiles, the halo plan, the halo tiles (bsa_sim_halo_stats
 * [2] counts them; the boxes of all tiles, which the other ranks would send,
 * are prepared before the timed stages).  Its pairs REPLACE the
 * last CD call's as the fetchable / gatherable pairs (bsa_fetch_pairs); the
 * sim's state and ASAS bookkeeping are not changed, and the next CD step
 * detects the sim's own rows again. */
int bsa_sim_detect_rows(bsa_ctx *ctx, int64_t row_begin, int64_t row_end, int64_t *n_conf, int64_t *n_los);
/* Halo exchange of the sharded step (several ranks): [0] bytes
 * this rank receives and [1] sends per CD call (the agreed capacities' regions),
 * [2] column tiles (512 aircraft) it received at the last CD call -- or, after
 * bsa_sim_detect_rows, the tiles that rank share needs from other ranks --
 * and [3] capacity regrowths (aborted and re-run steps) since bsa_sim_init. */
int bsa_sim_halo_stats(bsa_ctx *ctx, int64_t *out4);
/* Stream-ordered collectives (RCCL or the in-process group) this rank issued
 * since the last bsa_timing_reset: [0] calls, [1] payload bytes it sent,
 * [2] payload bytes it received (as RCCL moves them).  Per CD step of the
 * sharded sim: the box all-gather, the halo send / recv, the 16-B gate
 * all-reduce (+ the pair-key all-gather with resume_nav). */
int bsa_sim_comm_stats(bsa_ctx *ctx, int64_t *out3);
/* Testing aid: override this rank's copy of the tile capacity sender ->
 * receiver (the capacities must agree on all ranks, and RCCL's grouped send /
 * recv needs every send length to match its receive; the in-process group
 * checks that agreement at every exchange and fails loudly, so a disagreement
 * is caught on one GPU).  tiles >= 0; the next bsa_sim_init or regrowth
 * recomputes the capacities. */
int bsa_sim_set_halo_cap(bsa_ctx *ctx, int sender, int receiver, int64_t tiles);
/* Measurement aid (tools/probe_step.py): a ONE-rank sim plays rank `rank` of
 * `nranks` on this GPU -- bsa_sim_step then runs that rank's share of the
 * sharded step (its home rows: own tiles, halo plan and halo tiles as
 * bsa_sim_detect_rows does, K3 / K4' on its rows) with no collective; the
 * other rows do not move.  The results are not the sim's (timing only);
 * nranks = 1 returns to the whole sim (re-init it for results). */
int bsa_sim_probe_rank(bsa_ctx *ctx, int rank, int nranks);
/* Collective (every rank, before the same step): the next halo exchange
 * re-checks the region layout on all ranks -- every send length / offset
 * against its receiver's expectation, one host all-reduce -- as it does after
 * bsa_sim_init and every capacity regrowth, before any RCCL send / recv is
 * enqueued; a disagreement fails the step on every rank ("halo lengths
 * disagree").  Testing aid with bsa_sim_set_halo_cap. */
int bsa_sim_halo_recheck(bsa_ctx *ctx);
/* ASAS bookkeeping after the last CD call (resume_nav = 1; replaces
 * ASAS.update's Python sets, asas.py:490-502):
 * [0] |resopairs| of this rank's rows, [1] |confpairs_unique|,
 * [2] |lospairs_unique|, [3] len(confpairs_all), [4] len(lospairs_all),
 * [5] number of active aircraft of this rank's rows.  [1]-[4] are counts of
 * the global pair sets (every rank gathers all ranks' pair keys; the same
 * values on every rank). */
int bsa_sim_asas_stats(bsa_ctx *ctx, int64_t *out6);
/* This rank's resopairs (aircraft indices; idx1 ascending, then idx2; idx2 = -1, last in its
 * row, for an intruder deleted since the last CD call), at most cap pairs;
 * *count = total (call again with a larger buffer when *count > cap). */
int bsa_sim_resopairs(bsa_ctx *ctx, int32_t *idx1, int32_t *idx2, int64_t cap, int64_t *count);

/* One CD call of the resident sim WITHOUT the kinematics: [halo exchange] ->
 * detect -> resolver -> asas.active or the bookkeeping + ResumeNav, i.e. the
 * body of ASAS.update (asas.py:478-504), exactly the CD part of a
 * bsa_sim_step; the state does not move and the step count does not advance.
 * The ASAS.update drop-in (bluesky_amd/asas.py) runs it after writing the host
 * simulator's traffic with bsa_sim_update.  Overflows are grown and re-run
 * inside the call.  Collective with several ranks. */
int bsa_sim_cd(bsa_ctx *ctx);
/* Replace the parameters of a running sim (stack commands such as ZONER,
 * ZONEDH, DTLOOK, RMETHH change asas.R / dh / dtlookahead / the MVP switches
 * between calls, asas.py:190-395).  Turning resume_nav on starts with empty
 * bookkeeping. */
int bsa_sim_set_params(bsa_ctx *ctx, const bsa_sim_params *p);
/* NORESO / RESOOFF lists (asas.noresolst / asas.resoofflst, MVP.py:44-61) as
 * full-n uint8 host arrays of membership in aircraft-index order (NULL = empty
 * list); the step's MVP applies them when mvp.swnoreso / swresooff are set.
 * They follow bsa_sim_delete / bsa_sim_create (new aircraft are in neither). */
int bsa_sim_set_reso_lists(bsa_ctx *ctx, const uint8_t *noreso, const uint8_t *resooff);
/* ASAS outputs of this rank's rows after the last CD call, written into
 * full-n host arrays (other rows untouched; any pointer may be NULL):
 * asas.trk / tas / vs / alt, asase / asasn (float32), asas.active, and
 * dropped = 1 for an ownship of which ResumeNav dropped a resopair in that call
 * (asas.py:454-468: the reference then starts waypoint recovery with
 * route.findact + route.direct -- the ASAS drop-in applies it on the host from
 * this flag, the resident step on the device with bsa_sim_set_recovery, once
 * per dropped pair, bsa_sim_read_dropcount; resume_nav = 1). */
typedef struct bsa_asas_out {
  double *trk, *tas, *vs, *alt;
  float *asase, *asasn;
  uint8_t *active, *dropped;
} bsa_asas_out;
int bsa_sim_read_asas(bsa_ctx *ctx, bsa_asas_out *o);

/* ACDATA feed: the per-aircraft fields
 * ScreenIO.send_aircraft_data streams at 5 Hz
 * (bluesky/simulation/qtgl/screenio.py:194-239) for this rank's rows, served
 * from HBM without stalling the sim.  _request enqueues a snapshot behind the
 * steps already queued (one pack kernel + one copy into a pinned host mirror;
 * no host synchronisation); _poll returns 1 while it is still in flight (wait
 * = 0) or waits for it (wait = 1), then copies it into the caller's arrays
 * (row_end - row_begin entries each; any pointer may be NULL) and returns 0.
 * inconf / tcpamax are asas.inconf / asas.tcpamax of the last CD call (0
 * before the first), cas is traf.cas after the last step (0 before the first),
 * asasn / asase as asas holds them.  nconf_cur / nlos_cur = len(confpairs_unique) /
 * len(lospairs_unique), nconf_tot / nlos_tot = len(confpairs_all) /
 * len(lospairs_all) (screenio.py:207-210), global over all ranks; -1 unless
 * resume_nav = 1.  A new request first waits for the previous snapshot. */
typedef struct bsa_acdata {
  int64_t steps, row_begin, row_end;  /* set by _poll */
  int64_t nconf_cur, nconf_tot, nlos_cur, nlos_tot;
  double *lat, *lon, *alt, *tas, *cas, *gs, *trk, *vs, *tcpamax;
  uint8_t *inconf;
  float *asasn, *asase;
} bsa_acdata;
int bsa_sim_acdata_request(bsa_ctx *ctx);
int bsa_sim_acdata_poll(bsa_ctx *ctx, int wait, bsa_acdata *out);

/* ---------------------------------------------------------------- route edits
 * ADDWPT / DELWPT / DIRECT on the route table.  A batch is m
 * records; the records of one aircraft apply in batch order, each to the route
 * the one before left, records of different aircraft are independent.  Names
 * are the host's: pos is an index into the route.
 *   INSERT     a new waypoint before row pos (pos == n appends); bump_active:
 *              AFTER was given and found (iactwp >= pos moves up by one)
 *   OVERWRITE  row pos gets the record's waypoint
 *   DELETE     row pos goes, iactwp by Route.delwpt's rule; the active-waypoint
 *              data stay (the reference's delwpt does not touch them); a route
 *              emptied this way ends with iactwp -1 and LNAV off
 *   DIRECT     Route.direct to row pos
 * After an INSERT / OVERWRITE the route's flight plan (Route.calcfp) is
 * recomputed, actwp.next_qdr = getnextqdr(), and with 0 <= iactwp < n
 * Route.direct runs to iactwp; after a DELETE the flight plan is recomputed.
 * A refused batch changes nothing; the call returns the refusal (> 0) and
 * bsa_last_error names the record.  -1: any other failure. */
enum { BSA_ROUTE_INSERT = 0, BSA_ROUTE_OVERWRITE = 1, BSA_ROUTE_DELETE = 2, BSA_ROUTE_DIRECT = 3 };
enum {
  BSA_ROUTE_OK = 0,
  BSA_ROUTE_ERR_AIRCRAFT = 1,  /* aircraft index outside [0, n) */
  BSA_ROUTE_ERR_OP = 2,        /* no such op */
  BSA_ROUTE_ERR_POS = 3,       /* pos outside the route as the earlier records of the batch left it */
  BSA_ROUTE_ERR_WPTYPE = 4,    /* runway (5) or calculated (4) waypoint, or no waypoint type */
  BSA_ROUTE_ERR_NONFINITE = 5, /* lat / lon not finite */
  BSA_ROUTE_ERR_RANKS = 6      /* guidance on several ranks */
};
typedef struct bsa_route_edit_rec {
  int32_t aircraft, op, pos, flyby, wptype, bump_active;
  double lat, lon, alt, spd;
} bsa_route_edit_rec;
/* bsa_route_edit: the batch on host arrays (the parity form).  The table and
 * the state as bsa_fms_recover takes them; wptype: the waypoint type per table
 * row, NULL = all 0 (only Route.dest, 3, matters: calcfp gives it toalt 0).
 * iactwp, the mutable arrays of st and ap_alt are updated in place.  The new
 * table comes back compacted in aircraft order: out_rows (room for cap_rows
 * rows, cap_rows >= nrows + m), out_wptype (cap_rows, may be NULL), out_off /
 * out_n (n each), *out_nrows. */
int bsa_route_edit(bsa_ctx *ctx, int64_t n, int64_t nrows, const double *route_rows, const uint8_t *wptype,
                   const int32_t *rt_off, const int32_t *rt_n, int32_t *iactwp, const double *lat, const double *lon,
                   const double *alt, const double *tas, const double *gs, const double *trk, const double *bank,
                   const bsa_fms_state *st, double *ap_alt, int64_t m, const bsa_route_edit_rec *rec, int64_t cap_rows,
                   double *out_rows, uint8_t *out_wptype, int32_t *out_off, int32_t *out_n, int64_t *out_nrows);
/* bsa_sim_route_edit: the batch on the resident sim's table, between batches of
 * steps (guidance on, one rank).  Each edited route is rewritten behind the
 * table's live tail and the aircraft repointed to it; the rows it held are dead.
 * Once dead rows outnumber live ones the same call compacts the table in
 * aircraft order.  The FMS clock and every kept detect state stay. */
int bsa_sim_route_edit(bsa_ctx *ctx, int64_t m, const bsa_route_edit_rec *rec);
/* bsa_sim_route_rows: live rows of the table (what bsa_sim_read_routes returns).
 * bsa_sim_read_routes: the table compacted in aircraft order, as bsa_sim_set_fms
 * takes it: rows (cap_rows >= live rows), wptype (may be NULL), off / n (n each).
 * The sim's own table stays as it is. */
int bsa_sim_route_rows(bsa_ctx *ctx, int64_t *live);
int bsa_sim_read_routes(bsa_ctx *ctx, int64_t cap_rows, double *rows, uint8_t *wptype, int32_t *rt_off, int32_t *rt_n,
                        int64_t *nrows);
/* bsa_sim_route_stats: live rows, dead rows (the table's tail minus the live
 * ones), the rows the last bsa_sim_route_edit wrote (the sum of the edited
 * routes' new lengths) and the compactions since bsa_sim_set_fms. */
int bsa_sim_route_stats(bsa_ctx *ctx, int64_t *live, int64_t *dead, int64_t *written, int64_t *compactions);

/* ---------------------------------------------------------------- test seams
 * The two device primitives under the detect's row offsets, the bookkeeping's
 * CSR, the halo plan and the stopping stages' lists, over host arrays.  The
 * arrays are staged into device scratch and the library's own functions run on
 * the context's stream, with the context's scan state (tile status words,
 * ticket counter, epoch) -- the state every other caller's scans use.  Their
 * callers are the tests.
 *
 * bsa_scan_excl: out[i] = (in[0] + ... + in[i-1]) mod 2^32, out[0] = 0.
 * n == 0 writes nothing; n > INT32_MAX is refused. */
int bsa_scan_excl(bsa_ctx *ctx, int64_t n, const uint32_t *in, uint32_t *out);
/* bsa_flagged_list: the i in [0, n) with flag[id2h ? id2h[i] : i] & mask != 0,
 * ascending (np.flatnonzero's), into out (room for cap); *count = how many,
 * written also when count > cap, which is an error.  Every id2h[i] must be
 * below n.  n == 0 launches nothing. */
int bsa_flagged_list(bsa_ctx *ctx, int64_t n, const uint8_t *flag, const uint32_t *id2h, uint32_t mask, int64_t cap,
                     int32_t *out, int64_t *count);

#ifdef __cplusplus
}
#endif
#endif /* BSACCEL_H */
