// StateBased conflict detection for gfx950:
//   StateBasedCD.detect (bluesky/traffic/asas/StateBasedCD.py:7-103) with
//   geo.qdrdist_matrix (bluesky/tools/geo.py:110-162) fused in.
//
// Pipeline, all on one stream, one host sync:
//   K0a keys       Morton code of each position's unit vector (rows = own,
//                  columns = intruder), then hipcub radix sort -> spatial order.
//   K0b prep       per sorted index: fp64 records (the per-aircraft factors of
//                  the reference's N x N broadcasts) + fp32 prefilter records.
//   K0c tilebox    bounds of every 512-row block / 512-column tile.
//   K0d tilepairs  (row block, column tile) pairs whose bounds can contain a
//                  kept pair; all others are skipped without touching a pair.
//   K1a prefilter  N-body sweep of the surviving tile pairs: lane = ownship
//                  row (2 per lane), column tile in LDS (broadcast reads);
//                  stage 1 conservative reach test, stage 2 conservative
//                  fp32 closest-approach refine (exact-safe proofs);
//                  survivors compacted per wave (ballot/mbcnt, 1 atomic/flush).
//   K1b exact      one lane per candidate: the reference's fp64 expression
//                  sequence op for op (-ffp-contract=off), outputs appended
//                  with one atomic per wave.
//   K2  rank       the reference's row-major np.where order: K1b drops each
//                  pair into its row's bucket, k_rowblk sums the row counts
//                  and k_rank_rows ranks each row's pairs by column and
//                  writes the outputs.  Bucket width 0 (a row overflowed the
//                  widest bucket): scan of the row counts, scatter into row
//                  segments, k_rank per segment.
// Neither the spatial order nor the culling changes any result: every stage
// before K1b only removes pairs that provably cannot be a conflict or a loss
// of separation, and K1b evaluates the survivors exactly.
//
// This file is the host side of one detect: the decisions (DetectPlan), one
// function per stage, enqueue and finish.  The kernels stand with their
// launchers (bsa_detect.h) in bsa_k0.hip (K0), bsa_prefilter.hip (K1a),
// bsa_rank.hip (K1b, K2) and bsa_scan.hip.
#include <chrono>
#include <thread>

#include "bsa_detect.h"
#include "bsa_halo.h"
#include "bsa_internal.h"

namespace bsa {

// event set of this detect (the pool keeps one set per detect since the last
// bsa_timing_reset, up to kEvSets; later detects reuse the last set)
static int next_events(Ctx *c, hipEvent_t **ev) {
  const int k = std::min(c->ev_sets, kEvSets - 1);
  if ((int)c->evpool.size() < 5 * (k + 1)) {
    const size_t old = c->evpool.size();
    c->evpool.resize(5 * (size_t)(k + 1), nullptr);
    // timing-only events: no system-scope fence at record (a fenced record left a
    // ~6 us bubble before the next kernel, 5 per detect; only elapsed times are read)
    for (size_t q = old; q < c->evpool.size(); ++q)
      BSA_HIP(c, hipEventCreateWithFlags(&c->evpool[q], hipEventDisableSystemFence));
  }
  *ev = &c->evpool[5 * (size_t)k];
  c->ev_last = k;
  if (c->ev_sets < kEvSets) c->ev_sets++;
  return 0;
}

// the environment knobs (DetectEnv, bsa_internal.h)
const DetectEnv &detect_env() {
  static const DetectEnv env = [] {
    const auto num = [](const char *name, int unset) {
      const char *s = getenv(name);
      return s ? atoi(s) : unset;
    };
    const char *sh = getenv("BSA_TPR_SH");
    const int k4b = num("BSA_K4_BLOCK", 64);
    return DetectEnv{num("BSA_HOME_REC", -1),
                     num("BSA_STAGE1_T0", 0) != 0,
                     num("BSA_TP_SUPER", 0) == 1,
                     num("BSA_K0Z", 0) == 1,
                     num("BSA_TP_HALO_ALL", 0) == 1,
                     num("BSA_TPR", 1) != 0,
                     num("BSA_HK_TRACE", 0) == 1,
                     sh ? atof(sh) : 0.0,
                     num("BSA_PF_PIECES", 0),
                     num("BSA_PF_HEAVY_T0", -1),
                     num("BSA_PF_PIECES_NEAR", 0),
                     num("BSA_FUSE_EXACT", -1),
                     num("BSA_OV_GRID_A", 2),
                     num("BSA_K1B_GRID", 0),
                     std::min(std::max(num("BSA_PF_SYM", 2), 0), 2),
                     num("BSA_K24", 1) != 0,
                     (k4b == 64 || k4b == 128 || k4b == 256) ? k4b : 64,
                     num("BSA_SIM_PREP", 1) != 0,
                     num("BSA_LEAN_K2", 1) != 0};
  }();
  return env;
}

// stage 1 at the look-ahead midpoints unless KWIK, candidate
// reuse, BSA_FLAG_STAGE1_T0 or the BSA_STAGE1_T0 environment variable
// home mode: K1b reads stored fp64 column records (else builds them from the
// state arrays); BSA_HOME_REC=0/1 overrides (see detect_decide)
// One rank below 163 840 rows stores them (K1b then runs fused into the
// prefilter, on stored records; 500k and 1M rows are slower with them).  A
// rank of a row-sharded step (halo mode) does not: its two K0b launches (own
// and halo tiles) would write 128 B per column, and its K1b runs unfused
// anyway.  Measured with the whole rank step (tools/probe_step.py, 200 settle
// steps, slowest rank, BSA_HOME_REC=1 -> 0, A/B x 2): global1m R = 8 0.1175 /
// 0.1175 -> 0.1115 / 0.1127 ms, box100k R = 8 0.0822 / 0.0827 -> 0.0806 /
// 0.0800, R = 4 0.0966 / 0.0974 -> 0.0945 / 0.0939, R = 2 0.1092 / 0.1088 ->
// 0.1109 / 0.1082 (an older detect-only probe with per-stage events had
// favoured the records by ~4 us).
bool home_records(const Ctx *c, int64_t nrows) {
  const int env = detect_env().home_rec;
  return env >= 0 ? env == 1 : c->halo_mode == 0 && nrows <= 163840;
}

int stage1_mid(int flags, bool reuse, int kwik) {
  return (!reuse && !kwik && !(flags & BSA_FLAG_STAGE1_T0) && !detect_env().stage1_t0) ? 1 : 0;
}

bool nonfin_word(Ctx *c) {
  const bool fresh = !c->nonfin.p;
  if (!ensure(c, c->nonfin, 16, "non-finite input word")) return false;
  if (fresh && hipMemsetAsync(c->nonfin.p, 0, 16, c->stream) != hipSuccess) {
    fail(c, "zeroing the non-finite input word failed");
    return false;
  }
  return true;
}

// HK: wait until the step of detect m published its prediction (ring slot m
// % kHkRing holds (m + 1) << 2 | flags); the device runs the step before the
// one being enqueued, so this normally returns at once or after part of a step
static int hk_wait(Ctx *c, int64_t m, unsigned long long *v) {
  volatile unsigned long long *p = c->hk_host + (m % kHkRing);
  const unsigned long long want = (unsigned long long)(m + 1);
  if ((*p >> 2) == want) {
    *v = *p;
    return 0;
  }
  c->hk_waits++;
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spin = 0;; ++spin) {
    const unsigned long long x = __atomic_load_n(p, __ATOMIC_ACQUIRE);
    if ((x >> 2) == want) {
      *v = x;
      return 0;
    }
    if ((spin & 1023u) == 1023u) {
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60))
        return fail(c, "HK: the device did not publish detect %lld's prediction within 60 s", (long long)m);
      std::this_thread::yield();
    }
  }
}

// the halo overlap's second stream and events (Ctx::ov_*), created once
static int ov_init(Ctx *c) {
  if (!c->xstream) BSA_HIP(c, hipStreamCreateWithFlags(&c->xstream, hipStreamNonBlocking));
  for (hipEvent_t &e : c->ov_ev)
    if (!e) BSA_HIP(c, hipEventCreateWithFlags(&e, c->ov_evflags));
  return 0;
}

// HK (see DetectPlan::hk): the host's rebuild decision for this detect
static int decide_hk(Ctx *c, DetectPlan &p, bool host_decides) {
  if (p.tpr && host_decides && c->hk_on && !c->simp.resume_nav && c->hk_hdev) {
    if (c->hk.cool > 0) {  // after a stale abort: device-decided for a while
      c->hk.cool--;
      c->hk.drop();
    } else {
      p.hk = true;
      p.hm = c->hk.m++;
      const int64_t hm = p.hm;
      const int nf = (c->simp.winddim == 0 && c->sim_gs_derivable) ? 6 : 8;  // (halo_mid's field count)
      bool build = !p.tvalid || !c->hk.matches() || (c->halo_mode == 1 && nf != c->halo_fields);
      // a build one or two detects ago: its snapshot is fresh enough (the
      // prediction covers two steps of drift); else the prediction made from
      // the records of detect hm - 2, published by that step's K4'
      if (!build && !c->hk.built_lately(hm)) {
        unsigned long long v = 0;
        if (hk_wait(c, hm - 2, &v)) return -1;
        build = (v & 3ull) != 0;  // predicted, or that step aborted (its retry rebuilds anyway)
      }
      c->hk.keep(hm, build);
      p.hkeep = !build;
      (build ? c->hk_builds : c->hk_keeps)++;
      if (detect_env().hk_trace)
        fprintf(stderr, "[bsa hk] rank %d detect %lld: %s (tvalid %d, step %lld)\n", c->rank, (long long)hm,
                build ? "build" : "keep", p.tvalid ? 1 : 0, (long long)c->clk.steps);
    }
  } else if (p.tpr) {
    c->hk.drop();  // a device-decided detect: the build history is no longer the host's
  }
  return 0;
}

// the launch shape of a detect with rows (and the candidate list's reuse state)
static int decide_launch(Ctx *c, DetectPlan &p) {
  const DetectEnv &env = detect_env();
  const int64_t n = p.n, nrows = p.nrows;
  p.kf = p.mid ? 0.5 * (p.tla > 0.0 ? p.tla : 0.0) / 6371000.0 : 0.0;
  p.resort = !p.home && (!c->order.matches({n, p.rb, p.re, p.shared, p.distinct, p.kf}) || (p.flags & BSA_FLAG_RESORT) ||
                         c->order.age >= (p.reuse ? kResortEveryReuse : kResortEvery));
  if (c->cand_cap == 0)
    // 8 x max(128 k, 4 rows) candidates in all (at 100k rows ~12x the demand), whole shards
    c->cand_cap = (unsigned long long)kCandShards *
                  (((unsigned long long)8 * std::max<int64_t>(1 << 17, 4 * nrows) + kCandShards - 1) / kCandShards);
  p.cap = c->cand_cap;
  if (!ensure(c, c->cand, p.cap * sizeof(uint2), "candidate pairs")) return -1;
  if (p.reuse) {
    if (!ensure(c, c->snap_build, (size_t)n * sizeof(Snap), "reuse snapshot") ||
        !ensure(c, c->snap_cur, (size_t)n * sizeof(Snap), "reuse state") ||
        !ensure(c, c->reuse_use, (size_t)((n + 63) / 64) * 8, "reuse budget use") ||
        !ensure(c, c->reuse_ctl, 16, "reuse control"))
      return -1;
    const KeptCands::Key key{p.rpz, p.hpz, p.tla, (double)p.flags, n, p.cap, c->cand.p};
    p.rvalid = !p.resort && c->cands.matches(key);
    c->cands.keep(key);  // optimistic: an overflow invalidates it (detect_finish / sim retry)
  }
  p.na = p.halo ? p.a1 - p.a0 : 0;
  p.ovl = p.halo && p.hkeep && !p.noprune && p.na > 0 && (c->ov_mode == 2 || (c->ov_mode == 1 && c->halo_mode == 1));
  p.nrt = (int)((nrows + kTile - 1) / kTile);
  p.nct = (int)((n + kTile - 1) / kTile);
  p.ntp = (long long)p.nrt * p.nct;
  p.ngr = (int)((nrows + kGroup - 1) / kGroup);
  p.ngc = (int)((n + kGroup - 1) / kGroup);
  p.nsc = (int)((n + kSub - 1) / kSub);
  p.icap = (unsigned long long)p.ntp * kSlicesPerTile;
  // pieces: ~8 items per row tile, a few hundred row tiles fill the waves;
  // fewer rows split the items (BSA_PF_PIECES overrides)
  p.kn = PfKnobs{1, 1, 1, 0, 0, 0};
  if (env.pf_heavy_t0 >= 0 && env.pf_heavy_t0 <= 3) p.kn.t0 = env.pf_heavy_t0;
  // (measured, tools/gpu_pieces.sh: 2 pieces at the 100k box, 102 -> 97 us; 4 for
  // one rank of 8 there, 36 -> 29 us; 2 at 125k rows of 1M, 65 -> 53 us; 1
  // from 250k rows up, where 2 cost +15 us.  Round 5, with the longest-items
  // listing and the fused K1b: 1 piece from 64k rows up -- the 100k box
  // 0.1204 / 0.1212 -> 0.1185 / 0.1181 ms per step, one rank of 8 at 1M
  // 0.1130 / 0.1117 -> 0.1118 / 0.1112; tools/gpu_ab.sh, BSA_PF_PIECES=1),
  // 2 from 16k rows: one rank of 4 at the 100k box (25k rows) 0.0942 / 0.0938
  // -> 0.0925 / 0.0912 (tools/probe_step.py), of 8 (12.8k rows) stays at 4
  p.kn.pieces = nrows >= (1 << 16) ? 1 : (nrows >= (1 << 14) ? 2 : 4);
  const auto pieces_ok = [](int v) { return v == 1 || v == 2 || v == 4 || v == 8; };
  if (pieces_ok(env.pf_pieces)) p.kn.pieces = env.pf_pieces;
  p.kn.pnear = p.kn.pieces;
  if (pieces_ok(env.pf_pieces_near)) p.kn.pnear = env.pf_pieces_near;
  p.B = c->k2_bucket;
  p.fuse = env.fuse_exact != 0 && (env.fuse_exact == 1 || !p.halo) && c->fuse_on && !c->fuse_skip && p.B > 0 &&
           p.recs && !p.kwik && !p.reuse && !p.ovl;
  c->fuse_skip = false;  // (one retry unfused; the next detect fuses again)
  c->last_fused = p.fuse;
  if (p.fuse) c->fuse_count++;
  p.diag = p.shared ? (int)p.roff : -1;
  p.pf_grid = (unsigned)std::max<long long>(
      kWorkShards, std::min<long long>(p.ntp * PF_ITEMS_PER_TILE / PF_WAVES + 1, 256 * PF_BLOCKS_PER_CU));
  return 0;
}

// Every decision of one detect and the host bookkeeping that goes with them,
// before anything of it is enqueued (the field comments of DetectPlan say why)
static int detect_decide(Ctx *c, const DetectRequest &q, DetectPlan *plan) {
  const DetectEnv &env = detect_env();
  DetectPlan &p = *plan;
  p = DetectPlan{};
  const double rpz = q.rpz, hpz = q.hpz, tla = q.tla;
  const int flags = q.flags;
  int64_t rb = q.rb, re = q.re;
  const int64_t n = c->n;
  if (re <= 0) re = n;
  if (rb < 0 || rb > re || re > n)
    return fail(c, "bad row range [%lld, %lld) for n=%lld", (long long)rb, (long long)re, (long long)n);
  if (n > (int64_t)0x7fffffff) return fail(c, "n=%lld exceeds 2^31-1", (long long)n);
  const int64_t nrows = re - rb;
  c->have_pairs = false;
  c->last_rb = rb;
  c->last_re = re;
  c->last_flags = flags;
  c->last_conf = c->last_los = c->last_cand = 0;
  if (!ensure(c, c->counters, sizeof(Counters), "counters") ||
      !ensure(c, c->counters2, sizeof(Counters), "next counters") ||
      !ensure(c, c->workq2, kWorkShards * kWorkStride * 8, "next work counters") ||
      !ensure(c, c->stats, 8 * 8, "detect statistics") ||
      !ensure(c, c->inconf, (size_t)(nrows > 0 ? nrows : 1), "inconf") ||
      !ensure(c, c->tcpamax, (size_t)(nrows > 0 ? nrows : 1) * 8, "tcpamax") ||
      !ensure(c, c->workq, kWorkShards * kWorkStride * 8, "work counters") ||
      !ensure(c, c->rowcnt, (size_t)rowcnt_words((int)nrows) * 4, "row counts") ||
      !ensure(c, c->rowoff, (size_t)(2 * (nrows + 1)) * 4, "row offsets"))
    return -1;
  p.rpz = rpz;
  p.hpz = hpz;
  p.tla = tla;
  p.flags = flags;
  p.n = n;
  p.rb = rb;
  p.re = re;
  p.nrows = nrows;
  p.distinct = c->has_intruder;
  p.home = q.home;
  c->last_home = p.home;
  p.halo = p.home && c->halo_mode != 0;
  p.a0 = (int)(rb / kTile);
  p.a1 = (int)((re + kTile - 1) / kTile);
  p.recs = !p.home || home_records(c, nrows);
  if (p.home && (p.distinct || (rb % kTile != 0 && re > rb) || (flags & BSA_FLAG_KWIK)))  // (a rank without rows: rb = n)
    return fail(c, "home-order detect needs own == intruder, a %d-aligned row slice, no KWIK", kTile);
  p.kwik = (flags & BSA_FLAG_KWIK) ? 1 : 0;
  p.noprune = ((flags & BSA_FLAG_NOPRUNE) || (p.kwik && p.distinct)) ? 1 : 0;
  p.shared = p.home || (!p.distinct && rb == 0 && re == n);
  p.roff = p.home ? rb : 0;
  p.reuse = c->reuse_on && p.shared && rb == 0 && re == n && !p.noprune && !p.kwik && n > 0 && !p.halo;
  if (!p.reuse) c->cands.drop();
  p.mid = stage1_mid(flags, p.reuse, p.kwik);
  p.prepped = p.home && !p.halo && !p.reuse && rb == 0 && re == n && flags == 0 &&
              c->prep.matches({rpz, hpz, tla, (double)p.mid, n});
  c->prep.drop();
  if (!nonfin_word(c)) return -1;
  p.nf_epoch = p.prepped ? c->nf_prep_epoch : (q.nf_epoch ? q.nf_epoch : ++c->nf_counter);
  p.tp_list = p.halo && !env.tp_halo_all && !env.tp_super;
  p.tpr = env.tpr && c->tpr_on && p.home && !p.reuse && flags == 0 && !env.tp_super &&
          ((!p.halo && p.prepped && (n + kTile - 1) / kTile <= kTPDirectMax) || p.tp_list);
  p.sym = p.shared && rb == 0 && re == n && !p.halo && c->nranks == 1 && p.mid && !p.noprune && !p.kwik && !p.reuse
              ? std::min(env.pf_sym, c->sym_on)
              : 0;
  c->last_sym = p.sym;
  if (p.sym) c->sym_count++;
  const KeptTilePairs::Key tkey{rpz, hpz, tla, (double)p.mid, (double)rb, (double)re, (double)p.sym, n};
  p.tvalid = p.tpr && c->tiles.matches(tkey);
  if (decide_hk(c, p, q.host_decides)) return -1;
  if (p.tpr)  // (every rank, also one without rows: the kept state stays collective)
    c->tiles.keep(tkey);
  else
    c->tiles.drop();
  p.nozero = ((p.prepped && (n + kTile - 1) / kTile <= kTPDirectMax) || (p.hkeep && p.halo)) && !env.k0z &&
             !env.tp_super && c->k2_bucket > 0 && c->zero.matches({nrows});
  c->zero.drop();
  if (p.nozero) {
    std::swap(c->counters, c->counters2);
    std::swap(c->workq, c->workq2);
  }
  p.timed = c->ev_every > 0 && (c->ev_count++ % c->ev_every) == 0;
  if (p.timed && next_events(c, &p.ev)) return -1;
  p.empty = n == 0 || nrows == 0;
  if (p.empty) return 0;
  c->empty_detect = false;
  return decide_launch(c, p);
}

// a detect without aircraft or rows: zeroed outputs; a rank without rows still
// takes part in the exchange (HK keep: no box all-gather)
static int detect_empty(const DetectRun &R) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  if (R.zero(false, nullptr, 0)) return -1;
  if (p.halo) {
    HaloPre hp;
    HaloUnpack hu;
    if (halo_pre(c, p.rb, p.re, &hp)) return -1;
    if (!p.hkeep) {
      for (int r = 0; r < 3; ++r)
        if (hp.zn[r]) BSA_HIP(c, hipMemsetAsync(hp.z[r], 0, (size_t)hp.zn[r] * 4, c->stream));
      // (its plan-reuse flag stays clear: it holds no records that could drift)
      if (unsigned *f = halo_flag_word(c)) BSA_HIP(c, hipMemsetAsync(f, 0, 4, c->stream));
    }
    if (halo_mid(c, p.rb, p.re, &hu, nullptr, p.hkeep)) return -1;
  }
  if (R.q.gate) BSA_HIP(c, hipMemsetAsync(R.q.gate, 0, kGateWords * 8, c->stream));
  for (int e = 1; e < 5; ++e)
    if (R.mark(e)) return -1;
  c->ev_valid = c->ev_valid || p.timed;
  c->empty_detect = true;
  return 0;
}

// ---- K0a spatial order (DetectPlan::resort), after the reusable candidate
// list's K0z
static int detect_order(DetectRun &R) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  if (p.reuse) {
    R.rz.build = (const Snap *)c->snap_build.p;
    R.rz.cur = (Snap *)c->snap_cur.p;
    R.rz.ctl = (unsigned *)c->reuse_ctl.p;
    R.rz.use = (float *)c->reuse_use.p;
    R.rz.sh = c->reuse_sh;
    R.rz.sh_chord = (float)(c->reuse_sh / 6.3e6) * 1.000001f;
    R.rz.sv_default = c->reuse_sv;
    R.rz.sv_min = 1.0;
    R.rz.sv_max = 4.0 * c->reuse_sv;
    R.rz.ktarget = 16.0;
    R.rz.valid = p.rvalid ? 1 : 0;
    R.build = (const unsigned *)c->reuse_ctl.p;
    // K0z runs inside K0b (k_prep_cols) unless the list is reused (its build flag is set here)
    if (R.zero(true, (unsigned *)c->reuse_ctl.p, p.rvalid ? 0 : 1)) return -1;
  }
  if (p.resort) {
    // columns: intruder position, own velocity; rows: own position, intruder velocity
    if (spatial_order(c, (int)p.n, 0, R.intr.lat, R.intr.lon, R.own.trk, R.own.gs, p.kf, c->key_c, c->idx_c,
                      c->key_c2, c->perm_c))
      return -1;
    if (!p.shared && spatial_order(c, (int)p.nrows, (int)p.rb, R.own.lat, R.own.lon, R.intr.trk, R.intr.gs, p.kf,
                                   c->key_r, c->idx_r, c->key_r2, c->perm_r))
      return -1;
    c->order.keep({p.n, p.rb, p.re, p.shared, p.distinct, p.kf});
  }
  if (!p.home) c->order.age++;
  R.perm_c = (const unsigned *)(p.home ? c->h2id.p : c->perm_c.p);
  R.perm_r = p.home ? nullptr : (const unsigned *)(p.shared ? c->perm_c.p : c->perm_r.p);
  return 0;
}

// the buffers of K0b / K0c and those sized by the candidate capacity (every
// pair list <= candidates); shared: the column records serve as row records
// too (RowRec and ColRec agree field for field up to `vs`)
static int detect_buffers(DetectRun &R) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  const unsigned long long cap = p.cap;
  const int64_t n = p.n, nrows = p.nrows, roff = p.roff;
  if (!ensure(c, c->cflag, cap, "candidate flags") ||
      !ensure(c, c->cpay, cap * kPayStride * 8, "candidate records") ||
      !ensure(c, c->ckey2, cap * 8, "conflict keys") || !ensure(c, c->cval2, cap * 4, "conflict slots") ||
      !ensure(c, c->lkey2, cap * 8, "los keys") || !ensure(c, c->out_ci, cap * 4, "ci") ||
      !ensure(c, c->out_cj, cap * 4, "cj") || !ensure(c, c->out_pay, cap * 5 * 8, "conflict outputs") ||
      !ensure(c, c->out_li, cap * 4, "li") || !ensure(c, c->out_lj, cap * 4, "lj"))
    return -1;
  if (!ensure_col_prep(c, n, true)) return -1;
  if (!p.shared && (!ensure(c, c->rowrec, nrows * sizeof(RowRec), "row records") ||
                    !ensure(c, c->pfrow, nrows * sizeof(PFRec), "prefilter rows") ||
                    !ensure(c, c->pfvrow, nrows * sizeof(PFVel), "prefilter row velocities") ||
                    !ensure(c, c->pfprow, nrows * sizeof(float4), "prefilter row positions") ||
                    !ensure(c, c->rownf, (size_t)nrows, "row non-finite flags")))
    return -1;
  R.rowrec = p.shared ? (const RowRec *)c->colrec.p + roff : (const RowRec *)c->rowrec.p;
  R.pfrow = p.shared ? (const PFRec *)c->pfcol.p + roff : (const PFRec *)c->pfrow.p;
  R.pfvrow = p.shared ? (const PFVel *)c->pfvcol.p + roff : (const PFVel *)c->pfvrow.p;
  R.pfprow = p.shared ? (const float4 *)c->pfpcol.p + roff : (const float4 *)c->pfprow.p;
  if (!ensure(c, c->tilepairs, (size_t)p.ntp * kSlicesPerTile * sizeof(uint2), "prefilter items")) return -1;
  return 0;
}

// halo mode, after K0b of the own tiles (or none: HK keep): the plan / the
// exchange (halo_mid), then K0b of the received tiles
static int detect_halo_records(DetectRun &R, const PrepColsLaunch &own_tiles) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  HaloUnpack hu{};
  // (halo overlap: K0z before the pack -- xstream's K0b writes Counters)
  if (p.ovl && !p.nozero && R.zero(false, nullptr, 0)) return -1;
  if (halo_mid(c, p.rb, p.re, &hu, p.tpr ? &R.ht : nullptr, p.hkeep, p.ovl && c->halo_mode == 1 ? c->xstream : nullptr))
    return -1;
  hu.count = halo_list_count(c);
  // the received tiles: unpacked (exchange), records and boxes (no zeroing,
  // no budget checks, no boxes into the sent block)
  PrepColsLaunch recv = own_tiles;
  recv.tile_base = 0;
  recv.tile_list = (const int *)c->h_hl.p;
  recv.hu = hu;
  recv.hcnt = R.dcnt;
  recv.tck = TprCheck{};
  recv.nown = 0;
  if (p.ovl) {
    // the own tiles (budget checks included) on the stream; the received
    // ones on xstream once the exchange is in (the probe: no exchange, after
    // K0z), which then waits for the own tiles (its sweep's rows)
    if (c->halo_mode != 1) {
      BSA_HIP(c, hipEventRecord(c->ov_ev[0], c->stream));
      BSA_HIP(c, hipStreamWaitEvent(c->xstream, c->ov_ev[0], 0));
    }
    if (launch_prep_cols(c, c->stream, (unsigned)p.na, own_tiles)) return -1;
    BSA_HIP(c, hipEventRecord(c->ov_ev[1], c->stream));
    if (c->halo_hl > 0 && launch_prep_cols(c, c->xstream, (unsigned)c->halo_hl, recv)) return -1;
    BSA_HIP(c, hipStreamWaitEvent(c->xstream, c->ov_ev[1], 0));
  } else if (p.hkeep) {
    // HK keep: no plan, so the own tiles wait for nothing before the
    // exchange -- ONE K0b for them and the received tiles (workgroups [0, na)
    // the own tiles with their budget checks, the rest the halo list's
    // slots); K0z is K2's (double-buffered counters) or its own launch,
    // never inside it (its halo workgroups write Counters)
    if (!p.nozero && R.zero(false, nullptr, 0)) return -1;
    PrepColsLaunch both = recv;
    both.tile_base = p.a0;
    both.tck = own_tiles.tck;
    both.nown = p.na;
    if (launch_prep_cols(c, c->stream, (unsigned)(p.na + c->halo_hl), both)) return -1;
  } else if (c->halo_hl > 0) {
    if (launch_prep_cols(c, c->stream, (unsigned)c->halo_hl, recv)) return -1;
  }
  return 0;
}

// ---- K0b records in sorted order, K0c for the columns fused into it unless
// the candidate list is reused (then the boxes wait for the build decision
// every K0b lane contributes to); halo mode: the exchange between the own and
// the received tiles' K0b
static int detect_records(DetectRun &R) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  if (detect_buffers(R)) return -1;
  if (!p.shared) {  // (rows that are columns: the column word covers them)
    R.nfa.rowbad = (const uint8_t *)c->rownf.p;
    if (launch_prep_rows(R)) return -1;
  }
  // tile-pair list reuse (DetectPlan::tpr): the list's buffers and budgets
  if (p.tpr) {
    if (!ensure(c, c->tpr_snap, (size_t)p.n * sizeof(PFRec), "tile-pair list snapshot")) return -1;
    const bool fresh = !c->tpr_ctl.p;
    if (!ensure(c, c->tpr_ctl, 64, "tile-pair list control")) return -1;
    if (fresh) BSA_HIP(c, hipMemsetAsync(c->tpr_ctl.p, 0, 64, c->stream));
    const double sh_env = detect_env().tpr_sh;
    if (sh_env > 0.0) {
      c->tpr_dx = (float)(sh_env / 6.3e6);
      c->tpr_ds = (float)(sh_env / 6.3e6 / 20);
    }
    const bool force = p.hk ? !p.hkeep : !p.tvalid;  // (HK: the host's decision; a kept list launches no plan)
    R.ht = HaloTpr{p.halo ? 1 : 0, force ? 1 : 0, c->tpr_dx, c->tpr_ds, c->tpr_dv,
                   (unsigned long long *)c->tpr_ctl.p, nullptr};
  }
  R.hk_word = p.hk ? (unsigned long long *)c->tpr_ctl.p + 6 + (p.hm & 1) : nullptr;
  // halo mode: the plan's buffers are zeroed and the own tile boxes written
  // into the exchanged block by this K0b (no memset / copy launches)
  HaloPre hp{};
  if (p.halo && halo_pre(c, p.rb, p.re, &hp, p.tpr ? &R.ht : nullptr)) return -1;
  PrepColsLaunch a = R.prep_cols();
  const ZeroArgs no_zero = a.zs;
  // plan reuse: the own K0b checks its records against the last build's and
  // raises this rank's flag (not at a forced rebuild: it rebuilds anyway)
  if (p.tpr && p.halo) {
    R.ht.myflag = halo_flag_word(c);
    if (!R.ht.force)
      a.tck = TprCheck{(const PFRec *)c->tpr_snap.p, R.ht.myflag, c->tpr_dx, c->tpr_ds, c->tpr_dv, R.hk_word, c->hk_f};
  }
  if (!p.reuse) {  // fused K0c and K0z
    a.fb = FusedBoxes{(TileBox *)c->sbox_c.p, (TileBox *)c->gbox_c.p, (TileBox *)c->tbox_c.p, hp.blk, hp.blk_base};
    a.zs = ZeroArgs{(int)p.nrows, 1, 0, R.dcnt, (unsigned long long *)c->workq.p, (unsigned char *)c->inconf.p,
                    (unsigned long long *)c->tcpamax.p, (unsigned *)c->rowcnt.p, {hp.z[0], hp.z[1], hp.z[2]},
                    {hp.zn[0], hp.zn[1], hp.zn[2]}};
  }
  a.tile_base = p.halo ? p.a0 : 0;  // (halo mode: the own tiles only)
  if (p.ovl && ov_init(c)) return -1;
  if (p.prepped) {  // K0b + K0c ran in the previous step's K4': K0z + the tile boxes here
    if (!p.nozero && R.zero(false, nullptr, 0, true)) return -1;
  } else if (!(p.halo && p.hkeep)) {  // (HK keep, several ranks: the own tiles go with the halo tiles below)
    if (launch_prep_cols(c, c->stream, p.halo ? (unsigned)p.na : blocks_for(p.n, kTile), a)) return -1;
  }
  if (!p.halo) return 0;
  // the later launches of the own tiles: K0z and the sent block are done
  a.zs = no_zero;
  a.fb.blk = nullptr;
  return detect_halo_records(R, a);
}

// ---- K0c/K0d group / tile boxes (rows; columns when reused) and the tile-pair work list
static int detect_tilepairs(DetectRun &R) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  const int64_t roff = p.roff;
  const bool tp_super = detect_env().tp_super;
  if (!p.shared && (!ensure(c, c->tbox_r, p.nrt * sizeof(TileBox), "row tile boxes") ||
                    !ensure(c, c->gbox_r, p.ngr * sizeof(TileBox), "row group boxes")))
    return -1;
  R.gbox_r = p.shared ? (const TileBox *)c->gbox_c.p + roff / kGroup : (const TileBox *)c->gbox_r.p;
  R.tbox_r = p.shared ? (const TileBox *)c->tbox_c.p + roff / kTile : (const TileBox *)c->tbox_r.p;
  if (!p.shared && launch_boxes(R, false)) return -1;
  if (p.reuse && launch_boxes(R, true)) return -1;
  if (p.tpr)  // (after halo_mid, which may have forced the rebuild)
    R.tp = TprArgs{(unsigned long long *)c->tpr_ctl.p, R.ht.force, c->tpr_dx, c->tpr_ds, c->tpr_dv,
                   (const PFRec *)c->pfcol.p + roff, (PFRec *)c->tpr_snap.p + roff, p.halo ? R.ht.myflag : nullptr,
                   p.hkeep ? 1 : 0, p.hkeep ? (p.halo ? R.ht.myflag : (const unsigned *)c->tpr_ctl.p) : nullptr,
                   p.hkeep && c->sim_ctl.p ? (unsigned long long *)((char *)c->sim_ctl.p + kSimCtlStale) : nullptr};
  // HK keep: no K0d -- the prefilter takes the kept list's counts from the control words
  if (p.hkeep) return 0;
  return (p.nct <= kTPDirectMax || p.tp_list) && !tp_super ? launch_tilepairs_direct(R) : launch_tilepairs(R);
}

// longest items first (HeavyArgs): detects of a kept tile-pair list only
// (Ctx::hv_us: the listing threshold, < 0 off); leaves the next detect's
// listing (R.hn) to K1b / K2
static int heavy_setup(DetectRun &R, HeavyArgs *hv) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  const unsigned long long icap = p.icap;
  if (!(p.tpr && c->hv_us >= 0.0)) return 0;
  const bool fresh = c->hv_icap != icap || !c->hv_cnt.p;
  if (!ensure(c, c->hv_cost, icap * 4, "item costs") || !ensure(c, c->hv_flag, icap * 4, "listed item flags") ||
      !ensure(c, c->hv_list[0], icap * 4, "listed items") || !ensure(c, c->hv_list[1], icap * 4, "listed items") ||
      !ensure(c, c->hv_list[2], icap * 4, "listed items") || !ensure(c, c->hv_list[3], icap * 4, "listed items") ||
      !ensure(c, c->hv_cnt, 64, "listed item counts"))
    return -1;
  if (fresh) {
    BSA_HIP(c, hipMemsetAsync(c->hv_cost.p, 0, icap * 4, c->stream));
    BSA_HIP(c, hipMemsetAsync(c->hv_flag.p, 0, icap * 4, c->stream));
    BSA_HIP(c, hipMemsetAsync(c->hv_cnt.p, 0, 64, c->stream));
    c->hv_icap = icap;
  }
  const unsigned E = ++c->hv_epoch;  // (flags hold epochs >= 1; 0 = never)
  unsigned *cn = (unsigned *)c->hv_cnt.p;
  const unsigned a = E & 1, b = (E + 1) & 1;  // this detect's / the next one's lists and counts
  const double x = c->hv_x > 0.0 ? c->hv_x : 1e30;  // (tier 0 off: no slot reaches it)
  // a rank's share (halo mode) sweeps in ~40 us, not ~70: half the threshold
  // (one rank of 8 at global1m, probe A/B x 3: 0.1010-0.1029 -> 0.1007-0.1009
  // ms per step at 8 us, 0.0995-0.1010 at 5; box100k unchanged at 16)
  const double us = p.halo && !c->hv_us_env ? 0.5 * c->hv_us : c->hv_us;
  *hv = HeavyArgs{{(const unsigned *)c->hv_list[2 * a].p, (const unsigned *)c->hv_list[2 * a + 1].p}, cn + 2 * a,
                  cn + 2 * b, (const unsigned *)c->hv_flag.p, (unsigned *)c->hv_cost.p, E};
  R.hn = HeavyNext{(unsigned *)c->hv_cost.p, {(unsigned *)c->hv_list[2 * b].p, (unsigned *)c->hv_list[2 * b + 1].p},
                   cn + 2 * b, (unsigned *)c->hv_flag.p, E + 1,
                   {(unsigned)std::min(us * x * 100.0, 4e9), (unsigned)std::min(us * 100.0, 4e9)},
                   // the list's item counts: ctl[1], ctl[2] (the prefilter publishes a built list's there;
                   // an HK-kept detect fills no dequeue words)
                   (const unsigned long long *)c->tpr_ctl.p, icap};
  return 0;
}

// ---- K1a prefilter (with K1b when fused), the overlap's two sweeps and their join
static int detect_prefilter(DetectRun &R) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  const float T = (float)(p.tla > 0.0 ? p.tla : 0.0);
  const float lim = (float)((p.rpz + kEABS + (p.reuse ? 2.0 * c->reuse_sh : 0.0)) / (1.0 - kE1));
  const float liml = lim / kRS;  // unit-sphere units (pf_refine)
  PrefilterLaunch a{RefineParams{(float)p.rpz, (float)p.hpz, T, p.kwik ? INFINITY : liml * liml, 0.f}, ExactFuse{}, p.kn};
  if (pf_trace_arm(c)) return -1;
  HeavyArgs hv{};
  if (heavy_setup(R, &hv)) return -1;
  if (p.B && !ensure(c, c->kbuck, (size_t)2 * p.nrows * p.B * sizeof(uint2), "K2 row buckets")) return -1;
  if (p.fuse)
    a.xf = ExactFuse{R.rowrec, (const ColRec *)c->colrec.p, R.perm_r, R.perm_c, p.rpz, p.hpz, p.tla, (int)p.rb,
                     (int)p.nrows, p.B, (double *)c->cpay.p, (unsigned *)c->rowcnt.p, (uint2 *)c->kbuck.p,
                     (unsigned)c->fuse_recs};
  if (p.noprune) {  // every tile pair, every pair: no list reuse, no listing
    if (launch_prefilter(R, c->stream, p.pf_grid, a)) return -1;
  } else {
    a.tp = R.tp;
    a.hv = hv;
    for (int ph = p.ovl ? 1 : 0; ph <= (p.ovl ? 2 : 0); ++ph) {  // (halo overlap: own tiles here, the others on xstream)
      a.kn.ph = ph;
      a.kn.ca0 = p.a0;
      a.kn.ca1 = p.a1;
      // (the own tiles' sweep leaves half the workgroup slots to the received
      // tiles' K0b and sweep: 2 of 4 per CU, BSA_OV_GRID_A; probe with the
      // overlap 0.134 ms per step at 4, 0.121 at 2, 0.104 without it)
      const int ga = detect_env().ov_grid_a;
      const unsigned g = ph == 1 && ga > 0
                             ? std::min<unsigned>(p.pf_grid, std::max(256u * (unsigned)ga, (unsigned)kWorkShards))
                             : p.pf_grid;
      if (launch_prefilter(R, ph == 2 ? c->xstream : c->stream, g, a)) return -1;
    }
  }
  if (p.ovl) {  // join: K1b on waits for the halo tiles' sweep
    BSA_HIP(c, hipEventRecord(c->ov_ev[2], c->xstream));
    BSA_HIP(c, hipStreamWaitEvent(c->stream, c->ov_ev[2], 0));
    c->ov_count++;
  }
  return 0;
}

// ---- K1b exact evaluation (unless fused into K1a): grid-stride over the
// device-side count of the dense candidate list; 2048 workgroups (524 k lanes:
// the 100k box's ~153 k candidates in one stride, the workgroups past the
// count exit at once; BSA_K1B_GRID overrides for A/B)
static int detect_exact(DetectRun &R) {
  if (R.p.fuse) return 0;
  const int k1b_grid = detect_env().k1b_grid;
  return launch_exact(R, k1b_grid > 0 ? (unsigned)k1b_grid : 256u * 8u);
}

// ---- K2: row offsets and the pairs in row-major order: from K1b's row
// buckets (k_rank_rows, one launch), or scan + scatter into row segments +
// per-segment rank (bucket width 0); MVP's per-pair vectors when asked for
static int detect_rank(DetectRun &R) {
  Ctx *c = R.c;
  const DetectPlan &p = R.p;
  const unsigned long long cap = p.cap;
  const int nrows = (int)p.nrows, rb = (int)p.rb, B = p.B;
  if (!B) {
    const int nscan = 2 * (nrows + 1);
    if (scan_excl(c, (const unsigned *)c->rowcnt.p, (unsigned *)c->rowoff.p, nscan)) return -1;
    if (launch_scatter(R)) return -1;
  }
  const DetectRequest &q = R.q;
  MvpFuse mf{};
  if (q.mvp) {
    // (the lean K2 folds a block beyond its LDS arrays through the block's own slice, kRankRows x B entries)
    const unsigned long long npair = std::max<unsigned long long>(
        {cap, 1ull, q.lean_k2 ? (unsigned long long)rank_blocks(nrows) * kRankRows * (unsigned long long)B : 0ull});
    if (!ensure(c, c->mvp_pdv, npair * sizeof(double4), "mvp pair dv") || !ensure(c, c->mvp_pfl, npair, "mvp pair flags"))
      return -1;
    mf.p = *q.mvp;
    mf.in = MvpPairIn{q.gse, q.gsn, q.vs, q.alt, q.noreso, p.home ? (const unsigned *)c->id2h.p : nullptr};
    mf.pdv = (double4 *)c->mvp_pdv.p;
    mf.pfl = (uint8_t *)c->mvp_pfl.p;
    R.res.pairs_done = true;
    if (B) {  // K2 also folds each row's vectors (MvpIn::rowdv)
      if (!ensure(c, c->mvp_rowdv, (size_t)std::max(nrows, 1) * sizeof(double4), "mvp row dv")) return -1;
      mf.rowdv = (double4 *)c->mvp_rowdv.p;
      R.res.rows_folded = true;
    }
  }
  if (B) {
    const bool hl = p.fuse && R.hn.cost;  // the heavy-item listing moves here from K1b
    // lean: no block sums -- the listing rides on extra workgroups of the K2 + K4' launch
    const bool lean = q.lean_k2 && q.keep_k2;
    if (!lean && launch_rowblk(R, hl)) return -1;
    RankLaunch rl{(unsigned)rank_blocks(nrows), nrows, R.dcnt, cap, (unsigned *)c->rowoff.p,
                        (unsigned *)c->rowcnt.p, (const uint2 *)c->kbuck.p, B, (const double *)c->cpay.p, rb,
                        (int *)c->out_ci.p, (int *)c->out_cj.p, (double *)c->out_pay.p, (int *)c->out_li.p,
                        (int *)c->out_lj.p, (unsigned long long *)c->stats.p, q.gate, R.build, mf,
                        (unsigned char *)c->inconf.p, (unsigned long long *)c->tcpamax.p,
                        (Counters *)c->counters2.p, (unsigned long long *)c->workq2.p, R.nfa, R.hk_word};
    if (lean) {
      rl.lean = true;
      rl.heavy = hl ? kHeavyBlocks : 0u;
      if (hl) rl.hn = R.hn;
    }
    if (q.keep_k2) {  // the step launches it fused with K4' (k24_launch)
      R.res.k2 = rl;
      R.res.k2_kept = true;
      R.res.k2_ev = p.timed ? p.ev[4] : nullptr;
    } else if (rank_launch(c, rl, false, K24Args{})) {
      return -1;
    }
    c->zero.keep({p.nrows});
    return 0;
  }
  return launch_rank(R, mf);
}

// Enqueue one complete detect on the stream (K0-K2), no host synchronisation.
// *res says what the detect did for its caller (DetectResult, bsa_internal.h).
int detect_enqueue(Ctx *c, const DetectRequest &q, DetectResult *res) {
  *res = DetectResult{};
  DetectPlan p;
  if (detect_decide(c, q, &p)) return -1;
  res->hk = p.hk;
  res->hk_keep = p.hkeep;
  res->hk_m = p.hm;
  DetectRun R{c, p, q, *res, soa(c->own), soa(p.distinct ? c->intr : c->own), (Counters *)c->counters.p,
              NfArgs{(unsigned long long *)c->nonfin.p, p.nf_epoch, nullptr}};
  if (R.mark(0)) {
    invalidate(c, Change::DetectNotEnqueued);  // (detect_decide's optimistic mark: nothing of this detect is enqueued)
    return -1;
  }
  if (p.empty) return detect_empty(R);
  if (detect_order(R) || detect_records(R) || detect_tilepairs(R) || R.mark(1)) return -1;
  if (detect_prefilter(R) || R.mark(2)) return -1;
  if (detect_exact(R) || R.mark(3)) return -1;
  if (detect_rank(R)) return -1;
  if (!res->k2_kept && R.mark(4)) return -1;
  c->ev_valid = c->ev_valid || p.timed;
  return 0;
}

// Wait for the enqueued detect and read its totals.  *retry is set (and the
// candidate capacity grown) when the candidate list overflowed.
int detect_finish(Ctx *c, bool *retry) {
  *retry = false;
  Counters h;
  BSA_HIP(c, hipMemcpyAsync(&h, c->counters.p, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  if (c->empty_detect) {
    c->last_conf = c->last_los = c->last_cand = c->last_tiles = c->last_groups = 0;
    c->have_pairs = true;
    return 0;
  }
  invalidate(c, Change::DetectDone);  // (a retry zeroes everything again; so does any host-side recovery)
  // every cause of a retry is fixed before the one retry (not one per retry)
  if (h.fuse_ovf) {  // a wave flushed more blocks than the fused K1b records: K1b as its own launch
    c->fuse_skip = true;
    c->fuse_retries++;
    *retry = true;
  }
  if (h.k2_demand) {  // a K2 row bucket was full: nothing was written (the
    grow_k2_bucket(c, h.k2_demand);  // candidate list itself is complete: a reusable one stays valid)
    *retry = true;
  }
  unsigned long long worst = 0;
  for (int q = 0; q < kCandShards; ++q) worst = std::max(worst, h.cshard[q][0]);
  const unsigned long long total = h.cand;  // (the list is dense: K2 summed the shard counts)
  if (worst > c->cand_cap / kCandShards) {
    c->cand_cap = (unsigned long long)kCandShards * (worst + worst / 4 + 1024);
    invalidate(c, Change::DetectOverflow);
    *retry = true;
  }
  if (*retry) return 0;
  const int64_t nrows = c->last_re - c->last_rb;
  c->last_cand = (int64_t)total;
  c->last_tiles = (int64_t)h.tiles;
  c->last_tiles_total = (int64_t)(((nrows + kTile - 1) / kTile) * ((c->n + kTile - 1) / kTile));
  c->last_groups = (int64_t)h.groups;
  c->last_conf = (int64_t)h.conf;
  c->last_los = (int64_t)h.los;
  c->have_pairs = true;
#ifdef BSA_PF_TRACE
  if (pf_trace_dump(c, h.groups, h.tiles)) return -1;
#endif
#ifdef BSA_PF_STAMPS
  fprintf(stderr, "[bsa stamps] prefilter wave-cycles: setup %.4g stage1 %.4g drain %.4g flush %.4g | "
          "stage-1 survivors %.4g refine rounds %.4g batches %.4g enqueue trips %.4g\n",
          (double)h.stamp[0], (double)h.stamp[1], (double)h.stamp[2], (double)h.stamp[3], (double)h.stamp[4],
          (double)h.stamp[5], (double)h.stamp[6], (double)h.stamp[7]);
#endif
  return 0;
}

int detect(Ctx *c, const DetectRequest &q, int64_t *n_conf, int64_t *n_los) {
  DetectResult res;  // (nothing of it is the standalone caller's)
  for (int attempt = 0;; ++attempt) {
    if (detect_enqueue(c, q, &res)) return -1;
    bool retry = false;
    if (detect_finish(c, &retry)) return -1;
    if (!retry) break;
    if (attempt >= 4) return fail(c, "candidate buffer overflow after %d retries", attempt + 1);
  }
  *n_conf = c->last_conf;
  *n_los = c->last_los;
  return 0;
}

}  // namespace bsa
