// StateBased conflict detection, K1b and K2 (pipeline: bsa_cd.hip, DESIGN.md
// 3.3 / 3.4): the exact evaluation of the candidates and the pairs in the
// reference's row-major order, with their launchers.
#include "bsa_detect.h"
#include "bsa_geo_math.h"
#include "bsa_internal.h"
#include "bsa_mvp_math.h"
#include "bsa_mvp_row.h"
#include "bsa_pair_math.h"
#include "bsa_prep.h"
#include "bsa_sim_row.h"
#include "bsa_wave.h"

#pragma clang fp contract(off)

namespace bsa {

// ------------------------------------------------------------------ K1b exact
// flat candidate index space: shard s holds min(count_s, cap / kCandShards)
// candidates; pre[s] = candidates of the shards before s, returns the total
__device__ __forceinline__ unsigned long long cand_prefix(const Counters *cnt, unsigned long long cap,
                                                          unsigned long long *pre) {
  const unsigned long long ccap = cap / kCandShards;
  pre[0] = 0;
#pragma unroll
  for (int q = 0; q < kCandShards; ++q) pre[q + 1] = pre[q] + min(cnt->cshard[q][0], ccap);
  return pre[kCandShards];
}
__device__ __forceinline__ bool cand_overflow(const Counters *cnt, unsigned long long cap) {
  const unsigned long long ccap = cap / kCandShards;
  bool o = cnt->k2_demand != 0;  // a K2 row bucket was full: retried with wider buckets
  o |= cnt->halo_ovf != 0 || cnt->halo_miss != 0;  // halo tiles missing: the step is re-run
  o |= cnt->fuse_ovf != 0;  // fused K1b out of flush records: re-run with K1b's own launch
  o |= cnt->tpr_stale != 0;  // a host-kept tile-pair list that no longer covers the records: re-run, rebuilt
#pragma unroll
  for (int q = 0; q < kCandShards; ++q) o |= cnt->cshard[q][0] > ccap;
  return o;
}


// The next detect's listed items (HeavyArgs): every item whose units took at
// least a threshold is listed (two tiers), its cost word zeroed.  Runs on the
// grid's last lanes (K1b: the lanes past the candidate count; k_rowblk's extra
// blocks when K1b is fused into the prefilter -- in K2's launch, whose lanes
// would have had the time, its code cost K2 +5 us even when skipped; the lean
// K2 + K4', which has no k_rowblk in front of it, appends workgroups that do
// nothing else).  Called by every thread of workgroup blk of the nblk that
// take part (block-uniform trips: it synchronises the block).  One returning atomic per tier per BLOCK and trip, the block's
// waves placed by an LDS prefix (one per wave contended on two words: ~350
// at the 100k box, serialised at ~88 per us, were most of k_rowblk's 5.7 us).
constexpr int kHeavyMaxWaves = 16;
__device__ __forceinline__ void heavy_next(const HeavyNext &hn, unsigned nblk, unsigned blk) {
  __shared__ unsigned hcnt[2][kHeavyMaxWaves];
  __shared__ unsigned hbase[2];
  const unsigned long long inear = hn.work[1], m = inear + hn.work[2];
  const unsigned long long nt = (unsigned long long)nblk * blockDim.x;
  const unsigned long long g0 = (unsigned long long)blk * blockDim.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, W = (int)(blockDim.x >> 6);
  // trip j: lane k = nt - 1 - (g0 + t) + j nt; the block's smallest is nt - g0 - blockDim.x + j nt
  for (unsigned long long kb = nt - g0 - blockDim.x; kb < m; kb += nt) {
    const unsigned long long k = kb + (blockDim.x - 1 - threadIdx.x);
    unsigned long long slot = 0;
    int tier = 2;
    if (k < m) {
      slot = k < inear ? k : hn.icap - 1 - (k - inear);
      const unsigned cst = hn.cost[slot];
      hn.cost[slot] = 0u;
      tier = cst >= hn.thresh[0] ? 0 : (cst >= hn.thresh[1] ? 1 : 2);
    }
    const unsigned long long mk0 = __ballot(tier == 0), mk1 = __ballot(tier == 1);
    if (lane == 0) {
      hcnt[0][w] = (unsigned)__popcll(mk0);
      hcnt[1][w] = (unsigned)__popcll(mk1);
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      unsigned tot = 0;
      for (int v = 0; v < W; ++v) tot += hcnt[threadIdx.x][v];
      hbase[threadIdx.x] = tot ? atomicAdd(&hn.count[threadIdx.x], tot) : 0u;
    }
    __syncthreads();
    if (tier < 2) {
      unsigned off = hbase[tier];
      for (int v = 0; v < w; ++v) off += hcnt[tier][v];
      hn.list[tier][off + lane_prefix(tier == 0 ? mk0 : mk1)] = (unsigned)slot;
      hn.flag[slot] = hn.epoch;
    }
    __syncthreads();  // (hcnt / hbase of the next trip)
  }
}

// Results are stored per candidate (flag, key, payload) rather than appended
// to a shared list: appending needs an atomic with return on ONE counter per
// wave, which serialises at ~88/us (MI355X_MICROARCH 'dequeue') and cost
// ~70 us at 100k.  The per-row counts feed K2's counting sort.
// MODE: kExactRec (stored records), kExactKwik (stored records, KWIK),
// kExactHome (records built from the home-ordered state) -- one kernel per
// mode: with all three paths in one body the register allocation covered the
// union (205 VGPRs, 2 waves per SIMD)
constexpr int kExactRec = 0, kExactKwik = 1, kExactHome = 2;
// Stored-record modes at 3 waves per SIMD (139 VGPRs): at 4 the 128-VGPR cap
// spilled 12 B per lane to scratch inside the fp64 chain, and the dense list's
// ~2 400 working waves fit 3 per SIMD in one round anyway (box100k: 0.1394 ->
// 0.1377 ms per step, A/B 4 x 60 steps)
#ifndef BSA_EXACT_WAVES
#define BSA_EXACT_WAVES 3
#endif
#ifndef BSA_EXACT_HOME_WAVES
#define BSA_EXACT_HOME_WAVES 2
#endif
template <int MODE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MODE == kExactHome ? BSA_EXACT_HOME_WAVES : BSA_EXACT_WAVES, 8))) void k_exact(
    const RowRec *__restrict__ R, const ColRec *__restrict__ C,
    const unsigned *__restrict__ perm_r, const unsigned *__restrict__ perm_c,
    const uint2 *__restrict__ cand, Counters *__restrict__ cnt, SoA6 hs,
    unsigned long long cap, double rpz, double hpz, double tla, int rb, int nrows,
    unsigned char *__restrict__ cflag, double *__restrict__ cpay, unsigned char *__restrict__ inconf,
    unsigned long long *__restrict__ tcpamax_bits, unsigned *__restrict__ rowcnt, uint2 *__restrict__ kb,
    int B,
    unsigned *__restrict__ rctl, const Snap *__restrict__ snap_cur, Snap *__restrict__ snap_build, int nsnap,
    HeavyNext hn) {
  if (hn.cost) heavy_next(hn, gridDim.x, blockIdx.x);  // the next detect's listed items, on the grid's last lanes (idle: past the candidates)
  if (cand_overflow(cnt, cap)) return;  // the caller retries with more room
  if (rctl) {  // reuse: after a build this detect's state becomes the snapshot
    const bool built = rctl[0] != 0;
    const int k0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (built)
      for (int k = k0; k < nsnap; k += gridDim.x * blockDim.x) snap_build[k] = snap_cur[k];
    if (k0 == 0) rctl[1] = built ? 0u : rctl[1] + 1u;
  }
  unsigned long long pre[kCandShards + 1];
  const unsigned long long ncand = cand_prefix(cnt, cap, pre);
  const unsigned long long ccap = cap / kCandShards;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long idx = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
       idx < ncand; idx += stride) {
    int sh = 0;
#pragma unroll
    for (int q = 1; q < kCandShards; ++q) sh += (idx >= pre[q]) ? 1 : 0;
    const uint2 p = cand[(unsigned long long)sh * ccap + (idx - pre[sh])];
    unsigned char flag = 0;
    int row = 0;
    {
      // home mode (perm_r == NULL, the resident sim): rows are the home slice
      // [rb, rb + nrows) of the columns; the key's row is the home row, its
      // column the aircraft index (so K2 orders each row's pairs by index)
      const unsigned oi = perm_r ? perm_r[p.x] : (unsigned)rb + p.x, oj = perm_c[p.y];
      if (perm_r ? oi != oj : oi != p.y) {
        PairResult o;
#ifdef BSA_K1B_NOMATH  // diagnostic build (timing of K1b's memory chain alone; results are wrong)
        {
          const RowRec rr = R[p.x];
          const ColRec cc = C[p.y];
          o = PairResult{false, false, rr.lat, cc.lat, rr.lon, cc.lon, 0.0};
        }
#else
        if (MODE == kExactHome) {  // the records from the state arrays (rows = columns' slice)
          const ColRec ri = col_record(hs, hs, (int)oi), cj = col_record(hs, hs, (int)p.y);
          o = eval_pair<false>(reinterpret_cast<const RowRec &>(ri), cj, rpz, hpz, tla);
        } else {
          o = eval_pair<MODE == kExactKwik>(R[p.x], C[p.y], rpz, hpz, tla);
        }
#endif
#ifdef BSA_K1B_NOATOM  // diagnostic build (K1b without its per-row count atomics; results are wrong)
        {
          double *rq = cpay + idx * kPayStride;
          rq[1] = o.qdr;
          rq[2] = o.dist;
          rq[3] = o.tcpa;
          rq[4] = o.tin;
          rq[5] = o.dcpa + (o.conf ? 1.0 : 0.0) + (o.los ? 2.0 : 0.0);
        }
        o.conf = o.los = false;
#endif
        flag = (o.conf ? 1 : 0) | (o.los ? 2 : 0);
        row = (int)oi - rb;
        if (B) {  // row buckets (k_rank_rows writes inconf / tcpamax per row)
          exact_bucket(o, row, oj, p.y, idx, nrows, B, cpay, rowcnt, kb, cnt);
        } else {
          // one 48-B record per candidate: key | qdr dist tcpa tin dcpa (conflicts)
          double *rec = cpay + idx * kPayStride;
          if (flag) rec[0] = __longlong_as_double((long long)(((unsigned long long)oi << 32) | oj));
          if (o.conf) {
            rec[1] = o.qdr;
            rec[2] = o.dist;
            rec[3] = o.tcpa;
            rec[4] = o.tin;
            rec[5] = o.dcpa;
            inconf[row] = 1;
            // tcpamax = max_j(tcpa * swconfl) >= +-0 (StateBasedCD.py:90): only
            // positive tcpa can raise it, and positive doubles order as integers.
            if (o.tcpa > 0.0)
              atomicMax(&tcpamax_bits[row], (unsigned long long)__double_as_longlong(o.tcpa));
            atomicAdd(&rowcnt[row], 1u);
          }
          if (o.los) atomicAdd(&rowcnt[nrows + 1 + row], 1u);
        }
      }
    }
    if (!B) cflag[idx] = flag;
  }
}

// ------------------------------------------------------------------ K2 canonical order
// Per-row counting sort.  rowcnt holds [conflicts per row | 0 | LoS per row | 0]
// (2 (nrows + 1) words); its exclusive scan rowoff gives each row's segment
// in the conflict list and (minus P) in the LoS list.  k_scatter drops every
// pair's key into its row segment (in any order); k_rank ranks every entry
// among its row segment's columns, so the lists come out exactly in
// np.where's row-major order (StateBasedCD.py:93-95).  All counts are read on
// the device (no host round trip inside a detect), and nothing is written
// when the candidate list overflowed: the caller retries with more room.
__global__ __launch_bounds__(256) void k_scatter(const Counters *__restrict__ cnt, unsigned long long cap,
                                                 int rb, int nrows, const unsigned char *__restrict__ cflag,
                                                 const double *__restrict__ cpay,
                                                 const unsigned *__restrict__ rowoff,
                                                 unsigned *__restrict__ rowcnt,
                                                 unsigned long long *__restrict__ skey,
                                                 unsigned *__restrict__ sslot,
                                                 unsigned long long *__restrict__ lkey) {
  if (cand_overflow(cnt, cap)) return;
  unsigned long long pre[kCandShards + 1];
  const unsigned long long ncand = cand_prefix(cnt, cap, pre);
  const unsigned P = rowoff[nrows];
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long k = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; k < ncand;
       k += stride) {
    const unsigned char f = cflag[k];
    if (!f) continue;
    const unsigned long long key = (unsigned long long)__double_as_longlong(cpay[k * kPayStride]);
    const int row = (int)(key >> 32) - rb;
    if (f & 1) {
      const unsigned pos = rowoff[row] + atomicSub(&rowcnt[row], 1u) - 1u;
      skey[pos] = key;
      sslot[pos] = (unsigned)k;
    }
    if (f & 2) {
      const int r = nrows + 1 + row;
      lkey[rowoff[r] - P + atomicSub(&rowcnt[r], 1u) - 1u] = key;
    }
  }
}

// One lane per pair slot of the scattered lists (grid-stride over P + L, the
// device-side counts): the slot's rank among its row segment's columns (the
// segment is short: ~1.5 pairs per row at the 100k box; any length works)
// is its final index, so ci / cj / payload (conflicts) and li / lj (LoS)
// come out exactly in np.where's row-major order.  Every lane issues its
// segment loads independently: ~4 dependent memory round trips per detect
// instead of a per-row chain.  Block 0 / lane 0 also publishes the detect's
// totals: cnt->conf / los, the accumulated statistics and the gate words
// (gate[0] = overflow, gate[1] = P) the resident sim step reads.
__global__ __launch_bounds__(256) void k_rank(int nrows, Counters *__restrict__ cnt, unsigned long long cap,
                                              const unsigned *__restrict__ rowoff,
                                              const unsigned long long *__restrict__ skey,
                                              const unsigned *__restrict__ sslot,
                                              const double *__restrict__ cpay,
                                              const unsigned long long *__restrict__ lkey, int rb,
                                              int *__restrict__ ci, int *__restrict__ cj, double *__restrict__ out,
                                              int *__restrict__ li, int *__restrict__ lj,
                                              unsigned long long *__restrict__ stats,
                                              unsigned long long *__restrict__ gate,
                                              const unsigned *__restrict__ build, MvpFuse mf, NfArgs nf,
                                              unsigned long long *__restrict__ tcpamax_bits) {
  const bool ovf = cand_overflow(cnt, cap);
  const bool nfcol = nf.word && *nf.word == nf.epoch;
  const unsigned P = rowoff[nrows], L = rowoff[2 * nrows + 1] - P;
  const unsigned t0 = blockIdx.x * blockDim.x + threadIdx.x;
  if (t0 == 0) {
    unsigned long long pre[kCandShards + 1];
    (void)cand_prefix(cnt, cap, pre);
    unsigned long long ncand = 0;  // candidates written (the prefilter's per-workgroup counts; the list is dense)
    for (int q = 0; q < 32; ++q) ncand += cnt->gpart[q][1];
    cnt->conf = ovf ? 0 : P;
    cnt->los = ovf ? 0 : L;
    cnt->cand = ncand;
    unsigned long long g = 0;
    for (int q = 0; q < 32; ++q) g += cnt->gpart[q][0];
    cnt->groups = g;
    const bool built = !build || build[0];  // a reused list swept nothing this detect
    // an overflowed detect is retried and counted once, when it completes; a
    // list built by a detect whose K2 row buckets overflowed is complete and
    // reused by the retry, so that build counts
    bool list_ovf = false;
    for (int q = 0; q < kCandShards; ++q) list_ovf |= cnt->cshard[q][0] > cap / kCandShards;
    if (built && !list_ovf) {
      stats[0] += cnt->groups;
      stats[2] += cnt->tiles;
      stats[4] += 1;
    }
    if (!ovf) {
      stats[1] += ncand;
      stats[3] += 1;
    }
    if (gate) {
      gate[0] = ovf ? kGateOverflow : (nfcol ? kGateNonfinite : 0);
      gate[1] = ovf ? 0 : P;
      gate[2] = 1ull;  // (HK: no prediction from this K2 form -- rebuild, the safe side)
    }
  }
  if (ovf) return;
  const unsigned stride = gridDim.x * blockDim.x;
  if (nfcol || nf.rowbad)  // non-finite tcpa inputs: tcpamax NaN (K1b's atomics left the others)
    for (int r = (int)t0; r < nrows; r += (int)stride)
      if (nfcol || nf.rowbad[r]) tcpamax_bits[r] = kNanBits;
  for (unsigned x = t0; x < P + L; x += stride) {
    const bool conf = x < P;
    const unsigned long long *keys = conf ? skey : lkey;
    const unsigned xl = conf ? x : x - P;
    const unsigned long long kk = keys[xl];
    const int row = (int)(kk >> 32) - rb;
    const unsigned col = (unsigned)kk;
    const unsigned base = conf ? 0u : P;
    const unsigned b = rowoff[(conf ? 0 : nrows + 1) + row] - base;
    const unsigned e = rowoff[(conf ? 1 : nrows + 2) + row] - base;
    unsigned rank = 0;
    for (unsigned y = b; y < e; ++y) rank += ((unsigned)keys[y] < col) ? 1u : 0u;
    const unsigned pos = b + rank;
    if (conf) {
      const unsigned v = sslot[xl];
      ci[pos] = (int)(kk >> 32);
      cj[pos] = (int)col;
      double pay[5];
#pragma unroll
      for (int f = 0; f < 5; ++f) {
        pay[f] = cpay[(size_t)v * kPayStride + 1 + f];
        out[(size_t)f * P + pos] = pay[f];
      }
      if (mf.pdv) {  // resident step: MVP's per-pair vector (MVP.py:33-56) for k_mvp_row
        double4 dv;
        uint8_t fl;
        mvp_pair(mf.p, mf.in, (int)(kk >> 32), (int)col, pay[0], pay[1], pay[2], pay[3], dv, fl);
        mf.pdv[pos] = dv;
        mf.pfl[pos] = fl;
      }
    } else {
      li[pos] = (int)(kk >> 32);
      lj[pos] = (int)col;
    }
  }
}

// K2 with row buckets (K1b wrote each row's (column, candidate) entries in
// any order and the pair counts of every kRankRows-row block): workgroup b
// takes rows [b kRankRows, (b + 1) kRankRows), one per lane.  Its conflict /
// LoS bases are the block counts before b (and P, the total, for the LoS
// list), its rows' offsets an LDS scan of their counts -- rowoff comes out
// exactly as the scan of the scatter path made it, without a scan launch and
// its look-back chain.  Then the block's pairs, flattened (one lane each):
// the row by binary search over the offsets, the pair's rank among its row's
// bucket (the row's columns) its place in np.where's row-major order
// (StateBasedCD.py:93-95), its payload gathered from its candidate record.
// Block 0 / lane 0 publishes the totals as k_rank does.
// the conflict / LoS pair counts of every kRankRows-row block (behind the
// per-row counts: bcnt[b], bcnt[nb + b]); one wave per block, kRankRows / 64
// rows per lane (one load round trip; an overflowed detect's sums are never
// read: k_rank_rows checks the overflow itself)
// k_rowblk: 16 waves per block, wave w of block b sums row block 16 b + w
constexpr int kRowblkWaves = 16;
__global__ __launch_bounds__(64 * kRowblkWaves) void k_rowblk(int nrows, unsigned *__restrict__ rowcnt, HeavyNext hn) {
  // (K1b fused into the prefilter: the next detect's listed items here, on
  // every lane of the grid -- the host adds kHeavyBlocks blocks past the
  // row-block sums for them, ~1 slot per lane at the 100k box)
  if (hn.cost) heavy_next(hn, gridDim.x, blockIdx.x);
  const int nb = rank_blocks(nrows), b = blockIdx.x * kRowblkWaves + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (b >= nb) return;
  unsigned c = 0, l = 0;
#pragma unroll
  for (int q = 0; q < kRankRows / 64; ++q) {
    const int r = b * kRankRows + q * 64 + lane;
    c += r < nrows ? rowcnt[r] : 0u;
    l += r < nrows ? rowcnt[nrows + 1 + r] : 0u;
  }
  for (int o = 32; o > 0; o >>= 1) {
    c += (unsigned)__shfl_xor((int)c, o);
    l += (unsigned)__shfl_xor((int)l, o);
  }
  if (lane == 0) {
    rowcnt[2 * (nrows + 1) + b] = c;
    rowcnt[2 * (nrows + 1) + nb + b] = l;
  }
}

// LEAN (with K24 only; DESIGN.md 3.4, StepPlan::lean): a detect whose pair lists nobody can read before the next
// detect overwrites them.  No block sums (no k_rowblk in front), so no cb / lb / P / L: none of ci, cj, out, li,
// lj, rowoff, cnt->conf / los is written and the LoS pairs are not visited.  Everything per row and per block is
// as in the full form, bit for bit: the block-local offsets, each conflict pair's rank and MVP vector at
// so[lo] + rank, the folds in the same order, K4'.  MVP's gate (P != 0 in the full form) is Counters::any_conf; a
// block beyond its LDS arrays folds through its own slice of pdv / pfl (kRankRows x B entries from b kRankRows B:
// every row's pairs fit its bucket) and takes tcpamax, a maximum, from its rows' buckets.  The workgroups past the
// row blocks (hvn > 0 of them) list the next detect's items (heavy_next), k_rowblk's part on a full detect
template <bool K24, bool LEAN>
__global__ __launch_bounds__(kRankThreads) void k_rank_rows(int nrows, Counters *__restrict__ cnt, unsigned long long cap,
                                                         unsigned *__restrict__ rowoff,
                                                         unsigned *__restrict__ rowcnt,
                                                         const uint2 *__restrict__ kb, int B,
                                                         const double *__restrict__ cpay, int rb,
                                                         int *__restrict__ ci, int *__restrict__ cj,
                                                         double *__restrict__ out, int *__restrict__ li,
                                                         int *__restrict__ lj, unsigned long long *__restrict__ stats,
                                                         unsigned long long *__restrict__ gate,
                                                         const unsigned *__restrict__ build, MvpFuse mf,
                                                         unsigned char *__restrict__ inconf,
                                                         unsigned long long *__restrict__ tcpamax_bits,
                                                         Counters *__restrict__ cnext,
                                                         unsigned long long *__restrict__ wnext, K24Args ka,
                                                         NfArgs nf, unsigned long long *__restrict__ hkp, HeavyNext hn,
                                                         unsigned hvn) {
  static_assert(K24 || !LEAN, "the lean form is the fused K2 + K4' only");
  constexpr int W = kRankThreads / 64;
  __shared__ unsigned red[4][W];
  __shared__ unsigned soff[2][kRankRows + 1];  // the block's rows' exclusive offsets (conf, LoS), + total
  // the block's MVP pair vectors for the fold (when they fit; else through pdv / pfl)
  __shared__ double4 sdv[kRankLds];
  __shared__ uint8_t sfl[kRankLds];
  __shared__ double stc[kRankLds];  // ... and their tcpa (tcpamax)
  const int nb = rank_blocks(nrows), b = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (LEAN && b >= nb) {  // (block-uniform, before any barrier: these workgroups hold no rows)
    heavy_next(hn, hvn, (unsigned)(b - nb));
    return;
  }
  const unsigned *bcnt = rowcnt + 2 * (nrows + 1);
  const bool rowlane = t < kRankRows;  // lanes past the block's rows only place pairs
  const int r = rowlane ? b * kRankRows + t : nrows;
  const unsigned c = r < nrows ? rowcnt[r] : 0u, l = r < nrows ? rowcnt[nrows + 1 + r] : 0u;
  // non-finite tcpa inputs (NfArgs; loaded with the counts)
  const bool nfcol = nf.word && *nf.word == nf.epoch;
  const unsigned nfrow = nf.rowbad && r < nrows ? nf.rowbad[r] : 0u;
  const unsigned long long anyc = LEAN ? cnt->any_conf : 0ull;  // (the exact evaluation's launch is complete)
  // the next detect's per-row counts and counters start at zero (its K0z
  // launch is skipped, detect_enqueue): this block's counts are read, the
  // next detect's counter block (cnext / wnext, double-buffered) is idle
  if (r < nrows) {
    rowcnt[r] = 0u;
    rowcnt[nrows + 1 + r] = 0u;
  }
  if (b == 0) {
    constexpr int kWords = (int)(sizeof(Counters) / 8);
    for (int k = t; k < kWords; k += kRankThreads) reinterpret_cast<unsigned long long *>(cnext)[k] = 0ull;
    for (int k = t; k < kWorkShards * kWorkStride; k += kRankThreads) wnext[k] = 0ull;
  }
  const bool ovf = cand_overflow(cnt, cap);
  // P / L = all conflict / LoS pairs, cb / lb = those of the blocks before b
  unsigned P = 0, L = 0, cb = 0, lb = 0;
  if (!LEAN) {
    for (int q = t; q < nb; q += kRankThreads) {
      const unsigned x = bcnt[q], y = bcnt[nb + q];
      P += x;
      L += y;
      cb += q < b ? x : 0u;
      lb += q < b ? y : 0u;
    }
    unsigned v[4] = {P, L, cb, lb};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      for (int o = 32; o > 0; o >>= 1) v[k] += (unsigned)__shfl_xor((int)v[k], o);
      if (lane == 0) red[k][w] = v[k];
    }
  }
  const unsigned xc = wave_incl_scan(c), xl = wave_incl_scan(l);
  __shared__ unsigned wsum[2][W];
  if (lane == 63) {
    wsum[0][w] = xc;
    wsum[1][w] = xl;
  }
  __syncthreads();
  P = L = cb = lb = 0;
  unsigned wc = 0, wl = 0, tc = 0, tl = 0;
#pragma unroll
  for (int q = 0; q < W; ++q) {
    if (!LEAN) {
      P += red[0][q];
      L += red[1][q];
      cb += red[2][q];
      lb += red[3][q];
    }
    wc += q < w ? wsum[0][q] : 0u;
    wl += q < w ? wsum[1][q] : 0u;
    tc += wsum[0][q];
    tl += wsum[1][q];
  }
  if (b == 0 && t == 0) {
    unsigned long long ncand = 0;  // candidates written (the prefilter's per-workgroup counts; the list is dense)
    for (int q = 0; q < 32; ++q) ncand += cnt->gpart[q][1];
    if (!LEAN) {
      cnt->conf = ovf ? 0 : P;
      cnt->los = ovf ? 0 : L;
    }
    cnt->cand = ncand;
    unsigned long long g = 0;
    for (int q = 0; q < 32; ++q) g += cnt->gpart[q][0];
    cnt->groups = g;
    const bool built = !build || build[0];  // a reused list swept nothing this detect
    bool list_ovf = false;  // (see k_rank)
    for (int q = 0; q < kCandShards; ++q) list_ovf |= cnt->cshard[q][0] > cap / kCandShards;
    if (built && !list_ovf) {
      stats[0] += cnt->groups;
      stats[2] += cnt->tiles;
      stats[4] += 1;
    }
    if (!ovf) {
      stats[1] += ncand;
      stats[3] += 1;
    }
    if (gate) {
      gate[0] = ovf ? kGateOverflow : (nfcol ? kGateNonfinite : 0);
      gate[1] = ovf ? 0 : (LEAN ? anyc : (unsigned long long)P);  // (read as "any conflict": mvp_row)
      gate[2] = hkp && *hkp ? 1ull : 0ull;  // HK: this detect's prediction, all-reduced with the gate
    }
    if (hkp) *hkp = 0ull;  // (the word's next writer is two detects on)
    // HK, fused K4' (one rank): this detect's prediction to the host, before
    // any return (the host may be waiting for it); here rather than at the
    // kernel's start, where its loads cost every workgroup ~5 us
    if (K24) hk_publish(ka.pub, [&] { return ovf || *ka.d.sticky != 0u; });
  }
  // fused K4' (K24): an aborted step (this detect overflowed, or an earlier
  // step of the batch did) keeps every row's state -- including the double
  // buffer's other half, which the host swaps in after the step
  const bool k24_stop = K24 && (ovf || *ka.d.sticky != 0u);
  if (K24 && k24_stop) {
    if (ovf && b == 0 && t == 0) ka.mv.sticky[0] = 1u;
    if (rowlane && r < nrows) {
      const int k = rb + r;
      ka.d.alt_w[k] = ka.d.alt[k];
      ka.d.vs_w[k] = ka.d.vs[k];
      ka.d.gse_w[k] = ka.d.gse[k];
      ka.d.gsn_w[k] = ka.d.gsn[k];
    }
    return;
  }
  if (ovf) return;
  const unsigned ec = wc + xc - c, el = wl + xl - l;  // exclusive, within the block
  if (rowlane) {
    soff[0][t] = ec;
    soff[1][t] = el;
  }
  if (t == 0) {
    soff[0][kRankRows] = tc;
    soff[1][kRankRows] = tl;
  }
  if (!LEAN && r < nrows) {
    rowoff[r] = cb + ec;
    rowoff[nrows + 1 + r] = P + lb + el;
  }
  if (!LEAN && b == nb - 1 && t == 0) {
    rowoff[nrows] = P;
    rowoff[2 * nrows + 1] = P + L;
  }
  __syncthreads();
  const bool lds = tc <= (unsigned)kRankLds;  // the block's conflict pairs fit the LDS arrays
  const bool lds_fold = mf.rowdv && lds;
  // where the block's pairs start in pdv / pfl: their global position, or (lean) the block's own slice
  const size_t fb = LEAN ? (size_t)b * kRankRows * (size_t)B : (size_t)cb;
  for (unsigned x = t; x < (LEAN ? tc : tc + tl); x += kRankThreads) {
    const bool conf = x < tc;
    const unsigned q = conf ? x : x - tc;
    const unsigned *so = soff[conf ? 0 : 1];
    int lo = 0, hi = kRankRows;  // the last row i with so[i] <= q (rows without pairs share their successor's offset)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (so[mid] <= q) lo = mid;
      else hi = mid;
    }
    const unsigned k = q - so[lo], m = so[lo + 1] - so[lo];
    const int row = b * kRankRows + lo;
    const uint2 *bk = kb + ((size_t)(conf ? 0 : nrows) + row) * B;
    uint2 e;
    unsigned rank = 0;
    if (B == 8) {  // the whole bucket (one 64-B line, always allocated) in 4 loads issued together,
                   // not one dependent round trip per entry of the row
      uint4 q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = reinterpret_cast<const uint4 *>(bk)[u];
      const unsigned col[8] = {q[0].x, q[0].z, q[1].x, q[1].z, q[2].x, q[2].z, q[3].x, q[3].z};
      const unsigned cid[8] = {q[0].y, q[0].w, q[1].y, q[1].w, q[2].y, q[2].w, q[3].y, q[3].w};
      e = make_uint2(0u, 0u);
#pragma unroll
      for (unsigned y = 0; y < 8; ++y)
        if (y == k) e = make_uint2(col[y], cid[y]);
#pragma unroll
      for (unsigned y = 0; y < 8; ++y) rank += (y < m && col[y] < e.x) ? 1u : 0u;
    } else {
      e = bk[k];
      for (unsigned y = 0; y < m; ++y) rank += (bk[y].x < e.x) ? 1u : 0u;
    }
    if (conf) {
      const unsigned pos = cb + so[lo] + rank;
      if (!LEAN) {
        ci[pos] = rb + row;
        cj[pos] = (int)e.x;
      }
      double pay[5];
#pragma unroll
      for (int f = 0; f < 5; ++f) {
        pay[f] = cpay[(size_t)e.y * kPayStride + 1 + f];
        if (!LEAN) out[(size_t)f * P + pos] = pay[f];
      }
      const unsigned jh = (unsigned)__double_as_longlong(cpay[(size_t)e.y * kPayStride]);  // (K1b: home column)
      if (lds) stc[so[lo] + rank] = pay[2];
      if (mf.pdv) {  // resident step: MVP's per-pair vector (MVP.py:33-56), folded below
        double4 dv;
        uint8_t fl;
        MvpPairIn in = mf.in;
        int j = (int)e.x;
        if (in.id2h) {  // home order: the intruder's home position as K1b stored it
          j = (int)jh;
          in.id2h = nullptr;
        }
        mvp_pair(mf.p, in, rb + row, j, pay[0], pay[1], pay[2], pay[3], dv, fl);
        if (lds_fold) {
          sdv[so[lo] + rank] = dv;
          sfl[so[lo] + rank] = fl;
        } else {
          mf.pdv[fb + so[lo] + rank] = dv;
          mf.pfl[fb + so[lo] + rank] = fl;
        }
      }
    } else if (!LEAN) {
      const unsigned pos = lb + so[lo] + rank;
      li[pos] = rb + row;
      lj[pos] = (int)e.x;
    }
  }
  // per row (this workgroup's stores are visible to its lanes after the
  // barrier): inconf = any conflict (StateBasedCD.py:89), tcpamax =
  // max_j(tcpa * swconfl) (:90) -- +0 or the largest positive tcpa, as K1b's
  // atomics on the bit patterns made it -- and K3's fold of the row's pairs,
  // in order (MVP.py:44-61), from LDS or from pdv / pfl
  __syncthreads();
  const bool live = rowlane && r < nrows;
  if (!K24 && !live) return;
  if (live) {
    inconf[r] = c ? 1 : 0;
    unsigned long long tm = 0ull;
    for (unsigned k = 0; k < c; ++k) {
      // (lean, beyond LDS: from the row's bucket, in the bucket's order -- a maximum)
      const double tq = lds    ? stc[ec + k]
                        : LEAN ? cpay[(size_t)kb[(size_t)r * B + k].y * kPayStride + 3]
                               : out[(size_t)2 * P + cb + ec + k];
      const unsigned long long bits = (unsigned long long)__double_as_longlong(tq);
      if (tq > 0.0 && bits > tm) tm = bits;
    }
    // non-finite tcpa inputs in some column (every row) or in this row: NaN,
    // as np.max propagates it
    tcpamax_bits[r] = nfcol || nfrow ? kNanBits : tm;
    if (mf.rowdv)
      mf.rowdv[r] = lds_fold ? mvp_fold(sdv, sfl, ec, ec + c) : mvp_fold(mf.pdv + fb, mf.pfl + fb, ec, ec + c);
  }
  if (K24) {  // K4' of this workgroup's rows (k_sim_pilot_kin<true, PREP>'s body), every lane
    __shared__ unsigned long long sgate[2];
    if (t == 0) {
      sgate[0] = 0ull;
      sgate[1] = LEAN ? anyc : (unsigned long long)P;
    }
    __syncthreads();
    if (b == 0 && t == 0) *ka.d.steps_done += 1;
    MvpIn mv = ka.mv;
    mv.gate = sgate;
    const int k = rb + r;  // (rows = all aircraft: rb = 0)
    // the wave's group boxes from its lanes' records (lanes past nrows too, whose zeroed
    // records reduce to nothing); waves past the block's rows (BSA_RANK_LANES_PER_ROW > 1)
    // hold no rows and must not write a box (wave-uniform: kRankRows % 64 == 0)
    if (ka.prep && rowlane) {
      PFRec pr{}, pb{};
      if (ka.pa.snap && live) pb = ka.pa.snap[k];
      if (live)
        pr = pilot_kin_row<true, true>(rb, k, ka.simdt, ka.winddim, ka.vwn, ka.vwe, ka.wf, ka.d, mv, ka.mp, ka.pa);
      group_boxes_v(ka.pa.n, k / kGroup, pr, ka.pa.sbox, ka.pa.gbox);
      if (ka.pa.snap) {
        const bool outb = live && !pf_within(pr, pb, ka.pa.dx, ka.pa.ds, ka.pa.dv);
        if (__ballot(outb) && lane == 0) ka.pa.tpr_ctl[0] = 1ull;
        if (ka.pa.pred) {  // HK: ... or f x the budgets (a rebuild two detects on)
          const float f = ka.pa.pf;
          const bool nearb = live && !pf_within(pr, pb, f * ka.pa.dx, f * ka.pa.ds, f * ka.pa.dv);
          if (__ballot(nearb) && lane == 0) *ka.pa.pred = 1ull;
        }
      }
    } else if (live) {
      pilot_kin_row<true, false>(rb, k, ka.simdt, ka.winddim, ka.vwn, ka.vwe, ka.wf, ka.d, mv, ka.mp, ka.pa);
    }
  }
}

// ---- the launchers (bsa_detect.h)
// K1b: one kernel per mode (stored records, KWIK, records from the home-ordered state)
int launch_exact(const DetectRun &R, unsigned grid) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  const auto KEX = !p.recs ? k_exact<kExactHome> : (p.kwik ? k_exact<kExactKwik> : k_exact<kExactRec>);
  hipLaunchKernelGGL(KEX, dim3(grid), dim3(256), 0, c->stream, R.rowrec,
                     (const ColRec *)c->colrec.p, R.perm_r, R.perm_c, (const uint2 *)c->cand.p, R.dcnt, R.own, p.cap,
                     p.rpz, p.hpz, p.tla, (int)p.rb, (int)p.nrows, (unsigned char *)c->cflag.p, (double *)c->cpay.p,
                     (unsigned char *)c->inconf.p, (unsigned long long *)c->tcpamax.p, (unsigned *)c->rowcnt.p,
                     (uint2 *)c->kbuck.p, p.B, p.reuse ? (unsigned *)c->reuse_ctl.p : nullptr,
                     (const Snap *)c->snap_cur.p, (Snap *)c->snap_build.p, (int)p.n, R.hn);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

// K2 at bucket width 0: the evaluated candidates into their rows' segments (after the row counts' scan) ...
int launch_scatter(const DetectRun &R) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  hipLaunchKernelGGL(k_scatter, dim3(256 * 4), dim3(256), 0, c->stream, (const Counters *)R.dcnt, p.cap, (int)p.rb,
                     (int)p.nrows, (const unsigned char *)c->cflag.p, (const double *)c->cpay.p,
                     (const unsigned *)c->rowoff.p, (unsigned *)c->rowcnt.p, (unsigned long long *)c->ckey2.p,
                     (unsigned *)c->cval2.p, (unsigned long long *)c->lkey2.p);
  BSA_HIP(c, hipGetLastError());
  return 0;
}
// ... and each segment ranked by column into the outputs
int launch_rank(const DetectRun &R, const MvpFuse &mf) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  hipLaunchKernelGGL(k_rank, dim3(256 * 4), dim3(256), 0, c->stream, (int)p.nrows, R.dcnt, p.cap,
                     (const unsigned *)c->rowoff.p, (const unsigned long long *)c->ckey2.p,
                     (const unsigned *)c->cval2.p, (const double *)c->cpay.p,
                     (const unsigned long long *)c->lkey2.p, (int)p.rb, (int *)c->out_ci.p, (int *)c->out_cj.p,
                     (double *)c->out_pay.p, (int *)c->out_li.p, (int *)c->out_lj.p,
                     (unsigned long long *)c->stats.p, R.q.gate, R.build, mf, R.nfa, (unsigned long long *)c->tcpamax.p);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

// K2 with row buckets: the blocks' pair counts (and, heavy, the next detect's item listing) ...
int launch_rowblk(const DetectRun &R, bool heavy) {
  Ctx *c = R.c;
  const int nrows = (int)R.p.nrows;
  hipLaunchKernelGGL(k_rowblk, dim3((unsigned)((rank_blocks(nrows) + kRowblkWaves - 1) / kRowblkWaves) +
                                        (heavy ? kHeavyBlocks : 0u)),
                     dim3(64 * kRowblkWaves), 0, c->stream, nrows, (unsigned *)c->rowcnt.p, heavy ? R.hn : HeavyNext{});
  BSA_HIP(c, hipGetLastError());
  return 0;
}
// ... and one K2 launch (k_rank_rows; RankLaunch: bsa_internal.h), alone or fused with the step's K4'
int rank_launch(Ctx *c, const RankLaunch &a, bool k24, const K24Args &ka) {
  if (a.lean && !k24) return fail(c, "internal: the lean K2 is the fused K2 + K4' only");
  const auto K = a.lean ? k_rank_rows<true, true> : (k24 ? k_rank_rows<true, false> : k_rank_rows<false, false>);
  hipLaunchKernelGGL(K, dim3(a.grid + (a.lean ? a.heavy : 0u)), dim3(kRankThreads), 0, c->stream, a.nrows, a.cnt, a.cap,
                     a.rowoff, a.rowcnt, a.kb, a.B, a.cpay, a.rb, a.ci, a.cj, a.out, a.li, a.lj, a.stats, a.gate, a.build,
                     a.mf, a.inconf, a.tcpamax, a.cnext, a.wnext, ka, a.nf, k24 ? nullptr : a.hkp, a.hn, a.heavy);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

// the K2 launch a detect kept (DetectResult::k2), fused with the step's K4'
int k24_launch(Ctx *c, const RankLaunch &k2, hipEvent_t k2_ev, const K24Args &ka) {
  if (rank_launch(c, k2, true, ka)) return -1;
  if (k2_ev) BSA_HIP(c, hipEventRecord(k2_ev, c->stream));
  return 0;
}

// K2 row buckets too narrow for a row with `demand` pairs: the next power of
// two, or (beyond 64) the scatter into row segments
void grow_k2_bucket(Ctx *c, unsigned long long demand) {
  int b = std::max(c->k2_bucket, 1);
  while ((unsigned long long)b < demand && b <= 64) b *= 2;
  c->k2_bucket = b > 64 ? 0 : b;
}

}  // namespace bsa
