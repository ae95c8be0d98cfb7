// StateBased conflict detection, K1a (pipeline: bsa_cd.hip):
// the prefilter sweep of the kept tile pairs (with K1b when fused), its
// launcher and the STAMPS / TRACE diagnostics.
#include "bsa_box.h"
#include "bsa_detect.h"
#include "bsa_internal.h"
#include "bsa_pair_math.h"
#include "bsa_prep.h"
#include "bsa_wave.h"

#pragma clang fp contract(off)

namespace bsa {

// ------------------------------------------------------------------ K1a prefilter
// Stage 1 rounding budget (planar test).  Rows lie within
// ~0.02 of the plane origin and a kept pair has s < 0.5, so every term of
// acc is < 0.6 in magnitude and its fp32 roundings (k, K, 1 add, 2 fma; the
// projection errors are inside s's 1e-6 chord margin) total < 2e-7.
constexpr float kPlaneMargin = 4e-7f;

typedef float f2 __attribute__((ext_vector_type(2)));

// stage 2: conservative closest-approach refine of one (row, column) pair.
// rp = (x, y, z, -) and rv = (u, v, vs, alt) of the row, rb = (x, y, rho, -)
// / rho of its fp32 unit vector (its local east / north basis, staged once per
// item); cp = (x, y, z, -) and cv = (u, v, vs, alt) of the column.  Positions
// are unit-sphere chords, u / v are pre-scaled by 1 / R_S (kInvRS) to the
// same units (times and the vertical terms are unchanged).  u is NaN for an
// index that must never be refined (quirk column, non-finite position, row
// within ~0.6 deg of a pole), which keeps the pair through the `vv` test.
// Returns false only when no t in [0, max(tla,0)] can lie in both the
// vertical and the horizontal window of the reference's geometry (DESIGN.md
// "CPA refine"); any NaN keeps the pair.
constexpr float kInvRS = 1.f / kRS;
// far: keep without refining when the chord may exceed kRefineChord.  With
// fp32 unit vectors (|c|^2, |r|^2 within 2e-7 of 1) and the dot product's
// rounding (< 2e-7), chord^2 = |c|^2 + |r|^2 - 2 c.r <= 2 - 2 c.r + 1e-6, so
// c.r >= 1 - (kRefineChord^2 - 2e-6) / 2 refines chords <= kRefineChord only.
constexpr float kFarCos = (float)(1.0 - (kRefineChord * kRefineChord - 2e-6) / 2.0);
__device__ __forceinline__ bool pf_refine(const float4 &rp, const float4 &rv, const float4 &rb, const float4 &cp,
                                          const float4 &cv, const RefineParams &prm) {
  // Branch-free: every lane evaluates every test and the decision is one
  // select at the end -- the same values and the same keep / reject outcome as
  // testing them in order with early returns (far or clamped pairs are kept
  // whatever the rest says), without the exec-mask bookkeeping and the
  // per-branch LDS waits of the early-exit form.
  const bool far = cp.x * rp.x + cp.y * rp.y + cp.z * rp.z < kFarCos;  // > ~190 km: keep
  // the chord projected on the row's local east / north basis
  //   e = (-y, x, 0) / rho,  n = (-z x / rho, -z y / rho, rho),  rho = cos(lat):
  // e.r = n.r = 0, so (c - r).e = c.e and (c - r).n = c.n -- no difference
  // vector, and the per-row basis comes from LDS (|c.e|, |c.n| rounding < 5e-7,
  // ~3 m, inside kEABS)
  const float pe = cp.y * rb.x - cp.x * rb.y;
  const float pn = cp.z * rb.z - rp.z * (cp.x * rb.x + cp.y * rb.y);
  const float ve = cv.x - rv.x, vn = cv.y - rv.y;          // (own.u[j] - int.u[i]) / R_S
  const float vv = ve * ve + vn * vn;
  const bool clamp = !(vv >= 4e-6f * kInvRS * kInvRS);     // reference may clamp dv2; NaN
  const float dalt = cv.w - rv.w;                          // own.alt[j] - int.alt[i]
  const float H = prm.H + (rp.w + cp.w);                   // + vertical budgets (reuse; else 0)
  const float dvs = cv.z - rv.z;
  const float adv = __builtin_fabsf(dvs);
  // reciprocals by v_rcp_f32 (1 ulp): every division here only places a
  // window edge or the closest-approach time, and the margins below are
  // many orders of magnitude wider than 1 ulp
  const bool level = adv < 1e-3f;
  const bool level_out = __builtin_fabsf(dalt) >= H + 1e-3f * prm.T + 2.f + 1e-5f * __builtin_fabsf(dalt);
  const float inv = __builtin_amdgcn_rcpf(dvs);
  const float ta = (-H - dalt) * inv, tb = (H - dalt) * inv;
  const float lo = fminf(ta, tb), hi = fmaxf(ta, tb);
  const float d = (2.f + 1e-5f * (__builtin_fabsf(dalt) + H)) * __builtin_fabsf(inv) +
                  1e-4f * fmaxf(__builtin_fabsf(lo), __builtin_fabsf(hi));
  const float w0 = fmaxf(lo - d, 0.f), w1 = fminf(hi + d, prm.T);
  const bool vout = level ? level_out : (w0 > w1);
  const float t0 = level ? 0.f : w0, t1 = level ? prm.T : w1;
  const float tl = t0 * (1.f - kE1), th = t1 * (1.f + 2.f * kE1);
  float ts = -(pe * ve + pn * vn) * __builtin_amdgcn_rcpf(vv);
  ts = fminf(fmaxf(ts, tl), th);
  const float qe = pe + ve * ts, qn = pn + vn * ts;
  const bool hout = qe * qe + qn * qn > prm.lim2;
  return far | clamp | !(vout | hout);
}

#ifndef PF_Q1
#define PF_Q1 512  // per-wave stage-1 queue: u16 (row_local << 6 | column slot)
#endif
// Refine survivors are staged in the wave's LDS slot of PF_RES candidates; a
// full slot is flushed to the candidate list (one returning atomic on the
// shard counter per PF_RES candidates), and at the end of the sweep the four
// waves of a workgroup flush what is left with ONE atomic together -- the list
// is dense (no unused slots), so K1b runs every wave with all 64 lanes busy
#ifndef PF_RES
#define PF_RES 128
#endif
constexpr int kSubsPerTile = kTile / kSub;
static_assert(kSubsPerTile == 64, "one sub-group box per lane");
constexpr int kSubsPerBatch = 64 / kSub;  // sub-groups per 64-column batch
static_assert(PF_Q1 >= 64 * 8, "one 8-column chunk of survivors fits the stage-1 queue");

// Diagnostic item timeline (build with -DBSA_PF_TRACE; `make trace`,
// tools/pf_trace.py): per work item {item, wave << 8 | sub-groups, start,
// end} (s_memrealtime, 100 MHz) into a per-wave region of pf_trace (no
// atomics), dumped by detect_finish to $BSA_PF_TRACE_FILE.
#ifdef BSA_PF_TRACE
__device__ unsigned long long *pf_trace;
constexpr unsigned long long kTraceRecs = 1ull << 21;
constexpr unsigned kTraceWave = 256;
#endif
// Diagnostic phase timers (build with -DBSA_PF_STAMPS; `make stamps`):
// cycles per wave spent in 0 dequeue/setup, 1 stage 1, 2 refine drains,
// 3 flushes, summed over waves into Counters::stamp.
#ifdef BSA_PF_STAMPS
#define PF_STAMP(k)                                               \
  do {                                                            \
    const unsigned long long now_ = __builtin_amdgcn_s_memtime(); \
    st_acc[k] += now_ - st_last;                                  \
    st_last = now_;                                               \
  } while (0)
#else
#define PF_STAMP(k) \
  do {              \
  } while (0)
#endif

// K1a: each wave sweeps its 64 rows (one per lane, in registers) against the
// columns of a tile pair that survive culling at 8-column sub-group
// granularity (each lane tests one of the 64 sub-group boxes of the
// 512-column tile against the wave's row box).  The surviving columns are
// gathered in batches of 64 (eight sub-groups; one coalesced record load per lane, issued
// one batch ahead), projected and staged in the wave's LDS slot as column
// PAIRS, from which every lane reads them as broadcasts: each packed fp32
// instruction tests the lane's row against two columns.
//
// Stage 1 works in a plane: rows and columns are projected orthogonally onto
// the plane spanned by an (fp32-)orthonormal pair E, N (the tangent plane at
// the item's first row).  A projection never lengthens a vector, so the planar
// distance is <= the chord and "planar < s_i + s_j" keeps every pair with
// chord < s_i + s_j, wherever E, N point.  With P = ((p - o).E, (p - o).N) and
// k = s^2/2 - |P|^2/2 the test is linear in the column's values:
//   acc = (K_i + k_j) + s_i s_j + E_i e_j + N_i n_j = ((s_i + s_j)^2 - |P_i - P_j|^2) / 2
// (K_i = k_i + kPlaneMargin), plus the vertical interval test
// lo_j < hi_i and hi_j > lo_i.  The three signs are combined with one
// v_bitop3 (keep iff sign(acc) = 0, sign(lo_j - hi_i) = 1, sign(hi_j - lo_i) = 0;
// the +-0 and NaN cases can only keep a pair, never drop one) and shifted
// into a per-lane column bit mask with v_alignbit.
//
// Survivors of each 8-column chunk go to an LDS queue (DPP prefix sum of the
// per-lane counts).  The queue is drained after every batch (or when full)
// with all 64 lanes busy through stage 2 (refine) on LDS-resident inputs (the
// batch's staged columns, the item's staged rows, row unit vectors by
// ds_bpermute).  Stage-2 survivors are staged in the wave's LDS slot and
// appended densely to the candidate list (one atomic per PF_RES candidates,
// and one per workgroup at the end of the sweep).
template <bool NOPRUNE>
// 4 waves per SIMD = PF_BLOCKS_PER_CU resident workgroups: up to 128 VGPRs,
// no spills (at 5 waves the 96-VGPR cap spilled to scratch, and every scratch
// reload in the batch loop waited for the in-flight prefetch: 8 us slower)
#define PF_OCC __attribute__((amdgpu_waves_per_eu(BSA_PF_WAVES_PER_EU, 8)))
__global__ __launch_bounds__(PF_BLOCK) PF_OCC void k_prefilter(
    const PFRec *__restrict__ prow, const PFVel *__restrict__ vrow, const float4 *__restrict__ pprow, int nrows,
    const PFRec *__restrict__ pcol, const PFVel *__restrict__ vcol, const float4 *__restrict__ ppcol, int ncols,
    const TileBox *__restrict__ gbox_r, const TileBox *__restrict__ sbox_c, int noprune,
    const uint2 *__restrict__ items, unsigned long long icap,
    Counters *__restrict__ cnt,
    unsigned long long *__restrict__ work, RefineParams prm,
    uint2 *__restrict__ cand, unsigned long long cap, const unsigned *__restrict__ build, PfKnobs kn, int diag,
    TprArgs tp, HeavyArgs hv, ExactFuse xf) {
  __shared__ unsigned short q1s[PF_WAVES][PF_Q1];
  __shared__ float4 cka[PF_WAVES][32];      // staged column pairs: k k' s s'     (stage 1)
  __shared__ float4 cen[PF_WAVES][32];      //                      e e' n n'     (stage 1)
  __shared__ float4 clh[PF_WAVES][32];      //                      lo lo' hi hi' (stage 1)
  __shared__ float4 csx[PF_WAVES][64];      // staged columns:      x y z -       (refine)
  __shared__ float4 csv[PF_WAVES][64];      //                      u v vs alt    (refine)
  __shared__ float2 cbs[PF_WAVES][64];      //                      1/rho rho     (mirrored refine basis)
  __shared__ unsigned cix[PF_WAVES][64];    //                      sorted column index
  __shared__ float4 rsv[PF_WAVES][PF_WROWS];  // staged rows:       u v vs alt    (refine)
  __shared__ float4 rsp[PF_WAVES][PF_WROWS];  //                    x y z sigma   (refine)
  __shared__ float4 rbs[PF_WAVES][PF_WROWS];  //                    x/rho y/rho rho - (refine basis)
  __shared__ unsigned char sgs[PF_WAVES][kSubsPerBatch];  // the next batch's sub-groups (tile-local)
  __shared__ uint2 cst[PF_WAVES][PF_RES];   // staged candidates (row, column) of the wave
  if (build && !build[0]) return;  // reused candidate list
  if (tp.keep && *tp.vflag != 0u) {  // HK: a record left the kept list's budgets -- the step re-runs
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      cnt->tpr_stale = 1ull;
      if (tp.stale) *tp.stale = 1ull;  // (the batch's own record: later detects' counters may not show it)
    }
    // (the next detect's listed-item counts start at zero as in a sweep:
    // this detect's K2 still lists items for it, and a stale count would
    // sweep old slots twice)
    if (hv.list[0] && blockIdx.x == 0 && threadIdx.x < 2) hv.count_next[threadIdx.x] = 0u;
    return;
  }
  if (tp.ctl && kn.ph != 2 && blockIdx.x == 0 && threadIdx.x == 0) {  // tile-pair list reuse: K0d is complete here
    if (!tp.keep && (tp.force || tp.ctl[0] != 0ull)) {  // it built: keep the list's counts, clear the flag
      tp.ctl[1] = work[1];
      tp.ctl[2] = work[2];
      tp.ctl[0] = 0ull;
      tp.ctl[3] += 1ull;
    }
    tp.ctl[4] += 1ull;
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned short *q1 = q1s[w];
  float *ska = (float *)cka[w];
  float *sen = (float *)cen[w];
  float *slh = (float *)clh[w];
  float4 *sx = csx[w];
  float4 *sv = csv[w];
  unsigned *sci = cix[w];
  float4 *rv = rsv[w];
  unsigned subs = 0;      // 8-column sub-groups swept by this wave (for the roofline)
  const float qnan = __builtin_nanf("");
  // Dynamic work distribution: an item is one (tile pair, 64-row slice) that
  // K0d listed (the slice's box may reach the column tile's: at the 100k box
  // 44 % of the 8 x 3 642 slices do not, and each cost its wave a dequeue ->
  // tile -> box-load chain when all were numbered implicitly), split into
  // `pieces` units; each wave dequeues units from the counter of its shard
  // (blockIdx % 32, 128 B apart; a returning atomic on one word saturates at
  // ~88 per us).  Near tile pairs (the costly ones) come first in the list.  A
  // unit's sub-group mask is formed as it starts (below).  (Measured slower:
  // claiming the next item ahead (+20 us, also without spills: a returning
  // atomic in flight joins every later in-order vmcnt wait, so its latency is
  // moved, not hidden); several items per dequeue, or PF_GROUP consecutive tile
  // pairs of one slice per item sharing the row setup, with the next pair's
  // first batch prefetched (+10 / +30 / +90 us at 2 / 4 / 8: fewer, longer
  // items balance worse); stealing items from other shards once a wave's shard
  // is dry (+130 us: the drained shards' counters are hammered by failing
  // returning atomics); a separate K0e launch listing only the items with a
  // non-empty sub-group mask, dense ones split further (-8 us of sweep, but the
  // launch's cold dependent loads took 13 us).)
  // pieces > 1: a unit takes the set bits of rank p mod pieces of its item's
  // column mask (an equal share of the sub-groups; contiguous quarters of the
  // mask were uneven where the dense columns bunch) -- the densest items, 60-85
  // us each, set the sweep's span otherwise (tools/pf_trace.py); empty pieces
  // are skipped
  // K0d's items (complete before this launch): near ones from the front of
  // the list, the others from its back; each is `pieces` units
  // near items take kn.pnear units each, the others kn.pieces
  // (32-bit unit arithmetic, powers of two: the 64-bit forms with a run-time
  // divisor expanded into ~50 scalar instructions per unit)
  const unsigned lnear = (unsigned)__builtin_ctz((unsigned)kn.pnear), lpc = (unsigned)__builtin_ctz((unsigned)kn.pieces);
  // (HK keep: no K0d copied the kept list's counts into the dequeue words)
  const unsigned inear = (unsigned)(tp.keep ? tp.ctl[1] : work[1]), unear = inear << lnear;
  const unsigned nfar = (unsigned)(tp.keep ? tp.ctl[2] : work[2]);
  const unsigned nreg = unear + (nfar << lpc);
  unsigned nh0 = 0, nh1 = 0;
  if (hv.list[0]) {
    nh0 = __builtin_amdgcn_readfirstlane(hv.count[0]);
    nh1 = __builtin_amdgcn_readfirstlane(hv.count[1]);
    if (blockIdx.x == 0 && threadIdx.x < 2) hv.count_next[threadIdx.x] = 0u;
  }
  const unsigned lh0 = lnear + (unsigned)kn.t0;
  const unsigned hu0 = nh0 << lh0, hunits = hu0 + (nh1 << lnear);
  const unsigned nunits = hunits + nreg;
  const unsigned shard = blockIdx.x & (kWorkShards - 1);
  unsigned long long *wq = work + shard * kWorkStride + (kn.ph == 2 ? 8 : 0);
  // candidates: shard `shard` owns cand[shard * ccap, (shard + 1) * ccap) and
  // its own counter (spreads the flush atomics over kCandShards addresses)
  const unsigned long long ccap = cap / kCandShards;
  uint2 *ccand = cand + (unsigned long long)(shard % kCandShards) * ccap;
  unsigned long long *cshard = &cnt->cshard[shard % kCandShards][0];
  // the wave's staged candidates cst[w][0, nst) (wave-uniform count): a refine
  // round's survivors (mask mk) take the next entries in lane order; a round
  // that does not fit flushes the slot first (one returning atomic on the
  // shard counter reserves exactly nst list slots).  Most waves never flush
  // before the end of the sweep (the 100k box: ~37 candidates per wave), where
  // the workgroup flushes its four slots with one atomic.  (Reserving blocks of
  // PF_RES list slots directly left each wave's last block ~70 % unused: K1b
  // ran ~524 k slots for ~153 k candidates.)
  // (32-bit slot arithmetic: a shard's slots, and its counter until an
  // overflowing detect is retried, stay far below 2^32)
  const unsigned ccap32 = (unsigned)ccap;
  uint2 *stg = cst[w];
  unsigned nst = 0;
  unsigned nemit = 0;  // candidates this wave wrote (statistics)
  // fused K1b: the blocks this wave flushed mid-sweep, {position, count} (wave-uniform count)
  __shared__ uint2 xrc[PF_WAVES][kFuseRecs];
  unsigned nxr = 0;
  auto flush_stage = [&]() {
    __builtin_amdgcn_wave_barrier();
    unsigned long long r = 0;
    if (lane == 0) r = atomicAdd(cshard, (unsigned long long)nst);
    const unsigned nb = __builtin_amdgcn_readfirstlane((unsigned)r);
    for (unsigned k = lane; k < nst; k += 64)
      if (nb + k < ccap32) ccand[nb + k] = stg[k];
    if (xf.R) {  // fused K1b: the block is evaluated at the end of the workgroup's sweep
      if (lane == 0) {
        if (nxr < xf.nrec) xrc[w][nxr] = make_uint2(nb, nst);
        else cnt->fuse_ovf = 1ull;  // (the detect is retried with K1b as its own launch)
      }
      ++nxr;
    }
    nst = 0;
    __builtin_amdgcn_wave_barrier();
  };
  auto emit = [&](unsigned long long mk, bool keep, uint2 v) {
    const unsigned c = (unsigned)__popcll(mk), pre = lane_prefix(mk);
    if (nst + c > (unsigned)PF_RES) flush_stage();
    if (keep) stg[nst + pre] = v;
    nst += c;
    nemit += c;
  };
#ifdef BSA_PF_STAMPS
  // [4] stage-1 survivors, [5] refine rounds, [6] batches, [7] enqueue loop trips
  unsigned long long st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long st_last = __builtin_amdgcn_s_memtime();
#endif
#ifdef BSA_PF_TRACE
  unsigned tr_n = 0;
#endif
  for (;;) {
    unsigned item;
    {
      unsigned long long m0 = 0;
      if (lane == 0) m0 = atomicAdd(wq, 1ull);
      item = __builtin_amdgcn_readfirstlane((unsigned)m0);
    }
    // the unit of the shard's item-th dequeue: blocks of 8 consecutive units, 4
    // consecutive blocks to the 4 shards of one XCD (shard & 7 = the XCD of its
    // workgroups), so the items of a tile pair -- consecutive in the list -- are
    // swept on one XCD, close together in time: the column tile enters one L2
    item = (((item >> 3) * kWorkShards + 4 * (shard & 7) + (shard >> 3)) << 3) | (item & 7u);
    if (item >= nunits) break;
#ifdef BSA_PF_TRACE
    const unsigned long long tr0 = __builtin_amdgcn_s_memrealtime();
    unsigned tr_subs = 0;
#endif
    // the unit's list slot and piece: a listed item's piece (the first hunits
    // units), or a regular unit -- skipped when its item is listed
    unsigned long long slot;
    unsigned ls, piece;
    bool skip = false;
    const unsigned long long hq0 = hv.cost ? __builtin_amdgcn_s_memrealtime() : 0ull;
    if (item < hunits) {
      const bool t0 = item < hu0;
      ls = t0 ? lh0 : lnear;
      const unsigned ui = t0 ? item : item - hu0;
      piece = ui & ((1u << ls) - 1u);
      slot = hv.list[t0 ? 0 : 1][ui >> ls];
      skip = !(slot < inear || (slot >= icap - nfar && slot < icap));  // (a slot of a list since rebuilt)
      if (skip) slot = 0;
    } else {
      const unsigned uj = item - hunits;
      const bool inr = uj < unear;
      ls = inr ? lnear : lpc;
      const unsigned ui = inr ? uj : uj - unear;
      piece = ui & ((1u << ls) - 1u);
      const unsigned e = inr ? (ui >> ls) : inear + (ui >> ls);
      slot = e < inear ? (unsigned long long)e : icap - 1 - (unsigned long long)(e - inear);
      if (hv.list[0]) skip = hv.flag[slot] == hv.epoch;
    }
    const unsigned npc = 1u << ls;
    const uint2 it = items[slot];  // (issued with the flag's load: the skip needs both)
    if (kn.ph && !skip)  // halo overlap: the other launch sweeps it
      skip = ((it.y - (unsigned)kn.ca0) < (unsigned)(kn.ca1 - kn.ca0)) != (kn.ph == 1);
    do {  // one item; `break` ends it
    if (skip) break;
    // the item: (row tile | slice << 22, column tile)
    const uint2 rc = make_uint2(it.x & 0x3fffffu, it.y);
    const unsigned slice = (it.x >> 22) & (unsigned)(kSlicesPerTile - 1);
    // a mirrored item (K0d, a symmetric list: rows = columns, row tile < column
    // tile): the tile pair (column tile, row tile) is not listed -- the drain
    // refines every stage-1 survivor in both orientations (wave-uniform)
    const bool mir = !NOPRUNE && __builtin_amdgcn_readfirstlane(it.x & kItemMirror) != 0u;
    // a triangular item (K0d, level 2: slice q of tile t against column tile t,
    // DESIGN.md 3.2d): the sub-groups below the slice's own columns are skipped
    // (the items of the slices below cover those pairs), the ones above them
    // are mirrored, the slice's own 64 x 64 block is swept as ever (wave-uniform)
    const bool tri = !NOPRUNE && __builtin_amdgcn_readfirstlane(it.x & kItemTri) != 0u;
    // column sub-groups of this tile that may interact with the wave's row box:
    // the stage-1 test on box gaps (one sub-group box per lane), evaluated as
    // the item starts
    unsigned long long gm;
    {
      const int cb = (int)rc.y * kTile;
      const int nsub = min(kSubsPerTile, (ncols - cb + kSub - 1) / kSub);
      const int sg = min(lane, nsub - 1);
      const TileBox sb = sbox_c[cb / kSub + sg];
      const TileBox rg = gbox_r[((int)rc.x * kTile) / kGroup + (int)slice];
      gm = __ballot(lane < nsub && (noprune || boxes_may_interact(rg, sb)));
    }
    if (tri) gm &= ~0ull << (8u * slice);  // (sub-group lane k: columns cbase + 8 k ..; the slice's own: 8 q .. 8 q + 7)
    if (npc > 1)  // piece p: the set bits of rank p, p + npc, ... (equal shares of a dense mask)
      gm = __ballot(((gm >> lane) & 1ull) && (lane_prefix(gm) & (npc - 1u)) == piece);
    const int rbase = (int)rc.x * kTile + (int)slice * PF_WROWS;
    const int cbase = (int)rc.y * kTile;
    if (!gm) break;
    // the drain refines a survivor the other way round too when its column is
    // mlo or above: every column of a mirrored item, the columns above the
    // slice's own 64 of a triangular one, none otherwise (wave-uniform)
    const unsigned mlo = mir ? 0u : (tri ? (unsigned)(rbase + PF_WROWS) : ~0u);
    const bool mt = mir || tri;
    subs += (unsigned)__popcll(gm);
#ifdef BSA_PF_TRACE
    tr_subs = (unsigned)__popcll(gm);
#endif

    // the next batch = the first kSubsPerBatch remaining sub-groups (ascending):
    // lane b holding the r-th set bit of m (r < 8, r = set bits below b) posts
    // b to slot r; this lane takes column lane % kSub of the sub-group in slot
    // lane / kSub.  `taken` = the batch's bits, removed from the mask after it.
    unsigned long long taken = 0;
    auto batch_col = [&](unsigned long long m) -> int {
      const bool mine = ((m >> lane) & 1ull) && lane_prefix(m) < (unsigned)kSubsPerBatch;
      if (mine) sgs[w][lane_prefix(m)] = (unsigned char)lane;
      taken = __ballot(mine);
      const unsigned q = (unsigned)lane / kSub;
      if (q >= (unsigned)__popcll(taken)) return -1;
      const int j = cbase + (int)sgs[w][q] * kSub + (lane & (kSub - 1));
      return j < ncols ? j : -1;
    };
    auto drop_batch = [&](unsigned long long m) { return m & ~taken; };
    // unconditional loads (an empty slot reads column 0; its survivor bits are
    // masked by colmask and it is never queued): a load under a branch makes
    // the compiler wait for it right there, which would expose the prefetch
    auto load_col = [&](int j, PFRec &r, PFVel &v, float4 &q) {
      const int jj = j >= 0 ? j : 0;
      r = pcol[jj];
      v = vcol[jj];
      q = ppcol[jj];
    };
    int jn = batch_col(gm);
    PFRec nx;
    PFVel nv;
    float4 np;
    load_col(jn, nx, nv, np);

    const int krow = rbase + lane;
    const bool va = krow < nrows;
    // (unconditional, as load_col: a lane past the last row reads row rbase and
    // its survivor bits are masked)
    const int krw = va ? krow : rbase;
    const PFRec A = prow[krw];
    const PFVel AV = vrow[krw];
    const float4 AP = pprow[krw];
    // the item's plane: o = first row of the slice, E / N an orthonormal
    // tangent pair at o (any orthonormal pair is exact-safe; near a pole, or
    // for a non-finite o, the x / y axes)
    // (wave-uniform: kept in SGPRs)
    PFRec O = prow[rbase];
    O.x = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(O.x)));
    O.y = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(O.y)));
    O.z = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(O.z)));
    float ex = 1.f, ey = 0.f, nxx = 0.f, nyy = 1.f, nzz = 0.f;
    {
      const float rho2 = O.x * O.x + O.y * O.y;
      if (rho2 > 1e-6f && rho2 <= 1.f) {
        const float ir = __builtin_amdgcn_rsqf(rho2);
        const float rho = rho2 * ir;
        ex = -O.y * ir;
        ey = O.x * ir;
        nxx = -O.z * O.x * ir;
        nyy = -O.z * O.y * ir;
        nzz = rho;
      }
    }
    const float ox = isfinite(O.x) ? O.x : 0.f, oy = isfinite(O.y) ? O.y : 0.f,
                oz = isfinite(O.z) ? O.z : 0.f;
    auto project = [&](float x, float y, float z, float &e, float &n) {
      const float dx = x - ox, dy = y - oy, dz = z - oz;
      e = dx * ex + dy * ey;
      n = dx * nxx + dy * nyy + dz * nzz;
    };
    float re_, rn_;
    project(A.x, A.y, A.z, re_, rn_);
    const f2 E = {re_, re_}, N = {rn_, rn_}, S = {A.s, A.s};
    const float kr = 0.5f * A.s * A.s - 0.5f * (re_ * re_ + rn_ * rn_) + kPlaneMargin;
    const f2 K = {kr, kr};
    const f2 HI = {A.hi, A.hi}, LO = {A.lo, A.lo};
    // the row of this lane for the refine (u = NaN: never refine), position at
    // t = 0 and vertical budget; read from LDS by the drain (a register
    // broadcast would make it wait for the in-flight batch prefetch)
    rv[lane] = make_float4(AV.flags ? qnan : AV.u * kInvRS, AV.v * kInvRS, AV.vs, A.alt);
    rsp[w][lane] = make_float4(AP.x, AP.y, AP.z, A.pad);
    {  // the row's refine basis (rows within ~0.6 deg of a pole are flagged: u = NaN)
      const float rho2 = AP.x * AP.x + AP.y * AP.y;
      const float irho = __builtin_amdgcn_rsqf(rho2);
      rbs[w][lane] = make_float4(AP.x * irho, AP.y * irho, rho2 * irho, 0.f);
    }
    unsigned n1 = 0;                 // wave-uniform
    unsigned long long colmask = 0;  // valid slots of the swept batch

    auto drain = [&]() {
      __builtin_amdgcn_wave_barrier();
      PF_STAMP(1);
#ifdef BSA_PF_STAMPS
      st_acc[4] += n1;
      st_acc[5] += (n1 + 63) / 64;
#endif
      for (unsigned b0 = 0; b0 < n1; b0 += 64) {
        const unsigned k = b0 + lane;
        const unsigned e = q1[k < n1 ? k : b0];
        const unsigned rl = e >> 6, cl = e & 63u;
        bool keep = false, keepm = false;
        unsigned gi = 0, gj = 0;
        if (k < n1) {
          gi = (unsigned)rbase + rl;
          gj = sci[cl];
          keep = NOPRUNE ? true : pf_refine(rsp[w][rl], rv[rl], rbs[w][rl], sx[cl], sv[cl], prm);
          // mirrored item, or a column above a triangular item's own 64: the
          // same routine with the roles swapped -- the column as the row (its
          // basis staged with the batch), the row as the column; the staged
          // row and column values have one layout
          if (mt && gj >= mlo) {
            const float4 cp = sx[cl];
            const float2 cb = cbs[w][cl];
            keepm = pf_refine(cp, sv[cl], make_float4(cp.x * cb.x, cp.y * cb.x, cb.y, 0.f), rsp[w][rl], rv[rl], prm);
          }
          // an aircraft against itself (rows = the columns [diag, diag + nrows)):
          // never a pair (StateBasedCD.py's +1e9 I sentinel), ~40 % of the
          // refine survivors at the 100k box otherwise
          keep = keep && (diag < 0 || gj != (unsigned)diag + gi);
#ifdef BSA_PF_REFINE_X2
          {  // the same test on inputs the compiler cannot prove equal: the refine's cost, measured
            float4 c2 = sx[cl];
            c2.x += prm.zero;
            keep = keep & (NOPRUNE ? true : pf_refine(rsp[w][rl], rv[rl], rbs[w][rl], c2, sv[cl], prm));
          }
#endif
        }
        const unsigned long long mk = __ballot(keep);
        if (mk) {
          emit(mk, keep, make_uint2(gi, gj));
        }
        if (mt) {  // candidate (row gj, column gi): rows are the columns from 0 on (diag == 0)
          const unsigned long long mm = __ballot(keepm);
          if (mm) emit(mm, keepm, make_uint2(gj, gi));
        }
      }
      n1 = 0;
      __builtin_amdgcn_wave_barrier();
      PF_STAMP(2);
    };

    // survivors of 8-column chunk(s) arrive as a per-lane bit mask (bit u =
    // slot col0 + u); `enqueue` queues one chunk (the rare path when a whole
    // batch overflows the queue)
    auto enqueue = [&](unsigned bm, unsigned col0) {
      const unsigned c = (unsigned)__popc(bm);
      const unsigned x = wave_incl_scan(c);
      const unsigned total = __builtin_amdgcn_readlane(x, 63);
      if (total == 0) return;
      if (n1 + total > (unsigned)PF_Q1) drain();
      unsigned pos = n1 + x - c;
#ifdef BSA_PF_STAMPS
      {
        unsigned mx = c;
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
        st_acc[7] += mx;
      }
#endif
      while (bm) {
        q1[pos++] = (unsigned short)(((unsigned)lane << 6) | (col0 + (unsigned)__builtin_ctz(bm)));
        bm &= bm - 1u;
      }
      n1 = __builtin_amdgcn_readfirstlane(n1 + total);
    };
    // the whole batch's survivors (bit = slot) with ONE wave scan; the queue is
    // empty here (drained after every batch)
    auto enqueue_batch = [&](unsigned long long M) {
      const unsigned c = (unsigned)__popcll(M);
      const unsigned x = wave_incl_scan(c);
      const unsigned total = __builtin_amdgcn_readlane(x, 63);
      if (total == 0) return;
      if (total > (unsigned)PF_Q1) {
#pragma unroll 1
        for (unsigned ch = 0; ch < 8; ++ch) enqueue((unsigned)(M >> (8 * ch)) & 0xffu, 8 * ch);
        return;
      }
      unsigned pos = x - c;
      while (M) {
        q1[pos++] = (unsigned short)(((unsigned)lane << 6) | (unsigned)__builtin_ctzll(M));
        M &= M - 1ull;
      }
      n1 = total;
    };

    PF_STAMP(0);
    for (;;) {
      // project and stage the current batch (in-order LDS within the wave:
      // these writes land after the previous batch's reads, incl. its drain)
      {
        float ce, cn;
        project(nx.x, nx.y, nx.z, ce, cn);
        const float ck = 0.5f * nx.s * nx.s - 0.5f * (ce * ce + cn * cn);
        const int pb = (lane >> 1) * 4 + (lane & 1);  // pair lane>>1, half lane&1
        ska[pb] = ck;
        ska[pb + 2] = nx.s;
        sen[pb] = ce;
        sen[pb + 2] = cn;
        slh[pb] = nx.lo;
        slh[pb + 2] = nx.hi;
        sx[lane] = make_float4(np.x, np.y, np.z, nx.pad);
        sv[lane] = make_float4(nv.flags ? qnan : nv.u * kInvRS, nv.v * kInvRS, nv.vs, nx.alt);
        sci[lane] = (unsigned)jn;
        if (mt) {  // the column's refine basis as a row's (rbs above: x/rho, y/rho, rho), once per
                    // staged column; 1/rho and rho only -- 8 B per column keep the workgroup within 40 KB
          const float rho2 = np.x * np.x + np.y * np.y;
          const float irho = __builtin_amdgcn_rsqf(rho2);
          cbs[w][lane] = make_float2(irho, rho2 * irho);
        }
        colmask = __ballot(jn >= 0);
      }
#ifdef BSA_PF_STAMPS
      st_acc[6] += 1;
#endif
      gm = drop_batch(gm);
      const bool more = gm != 0;
      // prefetch the next batch while this one is swept (unconditionally: see load_col)
      jn = more ? batch_col(gm) : -1;
      load_col(jn, nx, nv, np);
      // sweep only the chunks holding valid slots
      const int nchunk = colmask ? (64 - __builtin_clzll(colmask) + 7) >> 3 : 0;
      // the survivor bits of chunks 0-3 / 4-7 shift into one word each (four
      // chunks unrolled: static LDS offsets, and the bit reversal / 64-bit
      // placement once per four chunks instead of per chunk)
      unsigned long long M = 0;  // this lane's stage-1 survivors of the batch, bit = slot
#pragma unroll 1
      for (int hf = 0; hf < 2; ++hf) {
      const int kc = min(max(nchunk - 4 * hf, 0), 4);
      if (!kc) break;
      unsigned bm = 0;
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        if (c4 >= kc) break;
        const int j0 = (hf * 4 + c4) * 8;
#pragma unroll
        for (int h = 0; h < 4; h += 2) {
        // two column pairs per load group (register pressure: occupancy)
        float4 pa[2], pe[2], pl[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          pa[u] = cka[w][(j0 >> 1) + h + u];
          pe[u] = cen[w][(j0 >> 1) + h + u];
          pl[u] = clh[w][(j0 >> 1) + h + u];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          if (NOPRUNE) {
            bm = (bm << 2) | 3u;
          } else {
            f2 acc = K + (f2){pa[u].x, pa[u].y};
            acc = __builtin_elementwise_fma(S, (f2){pa[u].z, pa[u].w}, acc);
            acc = __builtin_elementwise_fma(E, (f2){pe[u].x, pe[u].y}, acc);
            acc = __builtin_elementwise_fma(N, (f2){pe[u].z, pe[u].w}, acc);
            const f2 dlo = (f2){pl[u].x, pl[u].y} - HI;   // < 0 to keep
            const f2 dhi = (f2){pl[u].z, pl[u].w} - LO;   // > 0 to keep
            const unsigned t0 = (unsigned)__float_as_int(dlo.x) &
                                ~((unsigned)__float_as_int(acc.x) | (unsigned)__float_as_int(dhi.x));
            const unsigned t1 = (unsigned)__float_as_int(dlo.y) &
                                ~((unsigned)__float_as_int(acc.y) | (unsigned)__float_as_int(dhi.y));
            bm = __builtin_amdgcn_alignbit(bm, t0, 31);   // (bm << 1) | (t0 >> 31)
            bm = __builtin_amdgcn_alignbit(bm, t1, 31);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
        }
      }
      // bit 8 kc - 1 - u <-> slot 32 hf + u: reverse into bit u
      M |= (unsigned long long)(__builtin_bitreverse32(bm) >> (32 - 8 * kc)) << (32 * hf);
      }
      enqueue_batch(M & colmask & (va ? ~0ull : 0ull));
      // refine this batch's survivors while its columns are staged
      if (n1) drain();
      PF_STAMP(1);
      if (!more) break;
    }
    } while (0);
    if (hv.cost && lane == 0 && !skip)  // (non-returning)
      atomicAdd(&hv.cost[slot], (unsigned)(__builtin_amdgcn_s_memrealtime() - hq0));
#ifdef BSA_PF_TRACE
    if (lane == 0 && pf_trace) {  // per-wave record region (no atomics)
      const unsigned long long slot = ((unsigned long long)blockIdx.x * PF_WAVES + w) * kTraceWave + tr_n++;
      if (tr_n <= kTraceWave && slot < kTraceRecs) {
        unsigned long long *t = pf_trace + 4 * slot;
        t[0] = item | (item < hunits ? (1ull << 63) : 0ull) | ((unsigned long long)npc << 48);  // listed, pieces
        t[1] = ((unsigned long long)blockIdx.x << 2 | w) << 8 | tr_subs;
        t[2] = tr0;
        t[3] = __builtin_amdgcn_s_memrealtime();
      }
    }
#endif
  }
  PF_STAMP(0);
  // the workgroup's staged candidates with one atomic on its shard counter,
  // and the roofline's sub-group count: one atomic per workgroup, spread over
  // 32 lines (4096 waves adding to one word serialised at ~12 ns each, ~50 us
  // of the sweep's tail when the waves finish together)
  __shared__ unsigned wsubs[PF_WAVES], wcand[PF_WAVES], wst[PF_WAVES], wxr[PF_WAVES];
  __shared__ unsigned wbase;
  if (lane == 0) {
    wsubs[w] = subs;
    wcand[w] = nemit;
    wst[w] = nst;
    wxr[w] = min(nxr, xf.nrec);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned t = 0, tc = 0, ts = 0;
    for (int q = 0; q < PF_WAVES; ++q) t += wsubs[q];
    if (t) atomicAdd(&cnt->gpart[blockIdx.x & 31][0], (unsigned long long)t);
    for (int q = 0; q < PF_WAVES; ++q) tc += wcand[q];
    if (tc) atomicAdd(&cnt->gpart[blockIdx.x & 31][1], (unsigned long long)tc);  // candidates
    for (int q = 0; q < PF_WAVES; ++q) ts += wst[q];
    wbase = ts ? (unsigned)atomicAdd(cshard, (unsigned long long)ts) : 0u;
  }
  __syncthreads();
  if (!xf.R) {  // (fused K1b: nothing reads the final candidates back from the list)
    unsigned o = wbase;
    for (int q = 0; q < w; ++q) o += wst[q];
    for (unsigned k = lane; k < nst; k += 64)
      if (o + k < ccap32) ccand[o + k] = stg[k];
  } else {  // fused K1b (ExactFuse)
    // the workgroup's own final candidates [wbase, wbase + ts) of its shard,
    // from its waves' LDS stages (all 256 lanes: ~150 candidates at the 100k box)
    const unsigned o1 = wst[0], o2 = o1 + wst[1], o3 = o2 + wst[2], ts = o3 + wst[3];
    const unsigned long long sbase = (unsigned long long)(shard % kCandShards) * ccap;
    for (unsigned k = threadIdx.x; k < ts; k += PF_BLOCK) {
      const int q = (k >= o1) + (k >= o2) + (k >= o3);
      const unsigned kq = k - (q == 0 ? 0u : (q == 1 ? o1 : (q == 2 ? o2 : o3)));
      if (wbase + k < ccap32) fuse_exact_one(xf, cst[q][kq], sbase + wbase + k, cnt);
    }
    // ... and the blocks its waves flushed mid-sweep (written to the list by
    // this workgroup, visible to it after the barrier above)
    for (int q = 0; q < PF_WAVES; ++q)
      for (unsigned r = 0; r < wxr[q]; ++r) {
        const uint2 bk = xrc[q][r];
        for (unsigned k = threadIdx.x; k < bk.y; k += PF_BLOCK)
          if (bk.x + k < ccap32) fuse_exact_one(xf, ccand[bk.x + k], sbase + bk.x + k, cnt);
      }
  }
#ifdef BSA_PF_STAMPS
  PF_STAMP(3);
  if (lane == 0)
    for (int k = 0; k < 8; ++k) atomicAdd(&cnt->stamp[k], st_acc[k]);
#endif
}

// ---- the launcher (bsa_detect.h; PrefilterLaunch: bsa_cd_args.h)
int launch_prefilter(const DetectRun &R, hipStream_t stream, unsigned grid, const PrefilterLaunch &a) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  const auto K = p.noprune ? k_prefilter<true> : k_prefilter<false>;
  hipLaunchKernelGGL(K, dim3(grid), dim3(PF_BLOCK), 0, stream, R.pfrow, R.pfvrow, R.pfprow, (int)p.nrows,
                     (const PFRec *)c->pfcol.p, (const PFVel *)c->pfvcol.p, (const float4 *)c->pfpcol.p, (int)p.n,
                     R.gbox_r, (const TileBox *)c->sbox_c.p, p.noprune, (const uint2 *)c->tilepairs.p, p.icap, R.dcnt,
                     (unsigned long long *)c->workq.p, a.rp, (uint2 *)c->cand.p, p.cap, R.build, a.kn, p.diag, a.tp,
                     a.hv, a.xf);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

// diagnostic builds: a zeroed timeline buffer behind pf_trace before a
// detect's prefilter (detect_prefilter)
int pf_trace_arm(Ctx *c) {
#ifdef BSA_PF_TRACE
  static DevBuf tb;
  const size_t need = (size_t)kTraceRecs * 32;
  if (!ensure(c, tb, need, "prefilter trace")) return -1;
  BSA_HIP(c, hipMemsetAsync(tb.p, 0, need, c->stream));
  void *pt = tb.p;
  BSA_HIP(c, hipMemcpyToSymbolAsync(HIP_SYMBOL(pf_trace), &pt, sizeof pt, 0, hipMemcpyHostToDevice, c->stream));
  c->trace_buf = tb.p;
  c->trace_bytes = need;
#endif
  return 0;
}

#ifdef BSA_PF_TRACE
// diagnostic builds: the last prefilter's item timeline to $BSA_PF_TRACE_FILE
// (tools/pf_trace.py; detect_finish, and bsa_sim_step after each batch)
int pf_trace_dump(Ctx *c, unsigned long long groups, unsigned long long tiles) {
  const char *fn = getenv("BSA_PF_TRACE_FILE");
  if (!fn || !c->trace_buf) return 0;
  std::vector<unsigned long long> t(kTraceRecs * 4);
  BSA_HIP(c, hipMemcpy(t.data(), c->trace_buf, t.size() * 8, hipMemcpyDeviceToHost));
  if (FILE *f = fopen(fn, "ab")) {
    const unsigned long long hdr[4] = {0xfeedull, (unsigned long long)(t.size() / 4), groups, tiles};
    fwrite(hdr, 8, 4, f);
    fwrite(t.data(), 8, t.size(), f);
    fclose(f);
  }
  return 0;
}
#endif

}  // namespace bsa
