// GPU-resident sim step and the RCCL row-sharded multi-GPU mode.
//
// One step, rows [rb, re) owned by this rank:
//   every cd_every steps:
//     C1  all-gather of the 8 state arrays CD/MVP read for other rows
//         (lat lon trk gs alt vs gseast gsnorth) over xGMI, one RCCL call
//     K0-K2 detect(own rows x all columns)          asas.py:481-483
//     C2  all-reduce(max) of the 2-word gate {candidate overflow, P} (RCCL,
//         device buffer; skipped on one rank)
//     K3  MVP on the own rows' pairs, only when some rank has a conflict
//         (asas.py:486-487 `if self.confpairs`), and asas.active = inconf
//   every step:
//     K4' Pilot.APorASAS (no wind, pilot.py:41-63) fused with the kinematic
//         update (traffic.py:425-483) of the own rows
//
// A batch of steps is enqueued without any host synchronisation; the gate is
// read on the device.  A candidate-list overflow sets a sticky abort flag:
// every later kernel that writes persistent state (K3, K4') becomes a no-op,
// so the state stays exactly as before the failed step; the host then grows
// the buffers and re-runs the batch from that step.
#include <algorithm>
#include <type_traits>

#include "bsa_kin_math.h"
#include "bsa_mvp_row.h"
#include "bsa_prep.h"
#include "bsa_sim_row.h"
#include "bsa_xfer.h"

#pragma clang fp contract(off)

namespace bsa {

// Pilot.APorASAS (pilot.py:28-63; no wind, constant wind or a 2-D field) +
// UpdateAirSpeed/GroundSpeed/Position, rows [rb, re).  FUSE (a CD step without
// the ASAS bookkeeping): K3's per-row part (bsa_mvp_row.h: the dv fold, the
// finalize, asas.active = inconf, or DoNothing) runs first in the same lane --
// the row's new ASAS targets are what its pilot reads next (traffic.py:397),
// one launch and one pass over the row state fewer.  The gate check of
// k_mvp_row is made by every lane, so the whole grid agrees on an abort.
// PREP (one rank, the next step is a CD step): the lane also writes the next
// detect's column record of its row from the state it has just computed
// (bsa_prep.h: k_prep_cols' expressions, bitwise its records), and each wave
// reduces its group's sub-group and group boxes; that detect then skips its
// K0b launch, its K0z unites the group boxes into tile boxes
// (detect_enqueue, Ctx::prep).
template <bool FUSE, bool PREP>
__global__ __launch_bounds__(256) void k_sim_pilot_kin(int rb, int re, double simdt, int winddim, double vwn,
                                                         double vwe, WindField wf, SimDev d, MvpIn mv,
                                                         bsa_mvp_params mp, PrepArgs pa, HkPub pub) {
  const bool stop = *d.sticky != 0u || (FUSE && mv.gate[0] >= kGateOverflow);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (FUSE && mv.gate[0] >= kGateOverflow) mv.sticky[0] = 1u;
    hk_publish(pub, [&] { return stop; });  // HK: the CD step's prediction to the host (also when it aborts)
  }
  if (stop) return;
  const int k = rb + blockIdx.x * blockDim.x + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0) *d.steps_done += 1;
  if (PREP) {  // every lane reaches the wave's group reduction (its record from registers)
    PFRec p{}, b{};
    if (pa.snap && k < re) b = pa.snap[k];  // (issued with the row's other loads)
    if (k < re) p = pilot_kin_row<FUSE, PREP>(rb, k, simdt, winddim, vwn, vwe, wf, d, mv, mp, pa);
    group_boxes_v(pa.n, k / kGroup, p, pa.sbox, pa.gbox);
    if (pa.snap) {
      const bool out = k < re && !pf_within(p, b, pa.dx, pa.ds, pa.dv);
      if (__ballot(out) && (threadIdx.x & 63) == 0) pa.tpr_ctl[0] = 1ull;
      if (pa.pred) {  // HK: ... or pf x the budgets (a rebuild two detects on)
        const bool near = k < re && !pf_within(p, b, pa.pf * pa.dx, pa.pf * pa.ds, pa.pf * pa.dv);
        if (__ballot(near) && (threadIdx.x & 63) == 0) *pa.pred = 1ull;
      }
    }
    return;
  }
  if (k >= re) return;
  pilot_kin_row<FUSE, PREP>(rb, k, simdt, winddim, vwn, vwe, wf, d, mv, mp, pa);
}

static SimDev sim_dev(Ctx *c) {
  SimDev d;
  d.lat = (double *)c->own[0].p;
  d.lon = (double *)c->own[1].p;
  d.trk = (double *)c->own[2].p;
  d.gs = (double *)c->own[3].p;
  d.alt = (double *)c->own[4].p;
  d.vs = (double *)c->own[5].p;
  d.tas = (double *)c->s_tas.p;
  d.hdg = (double *)c->s_hdg.p;
  d.gse = (double *)c->s_gse.p;
  d.gsn = (double *)c->s_gsn.p;
  d.alt_w = d.alt;
  d.vs_w = d.vs;
  d.gse_w = d.gse;
  d.gsn_w = d.gsn;
  d.altprev = (double *)c->s_altprev.p;
  d.ax = (double *)c->s_ax.p;
  d.env = c->sim_limits ? (const double *)c->s_env.p : nullptr;
  d.ptab = c->sim_perf ? (const double *)c->s_ptab.p : nullptr;
  d.ptype = (const int *)c->s_ptype.p;
  d.phase = (uint8_t *)c->s_phase.p;
  d.atm = c->sim_atmos ? (double *)c->s_atm.p : nullptr;
  d.n = (int)c->n;
  d.aptrk = (const double *)c->s_aptrk.p;
  d.aptas = (const double *)c->s_aptas.p;
  d.apalt = (const double *)c->s_apalt.p;
  d.apvs = (const double *)c->s_apvs.p;
  d.bank = (const double *)c->s_bank.p;
  d.eps = (const double *)c->s_eps.p;
  d.accel = (const double *)c->s_accel.p;
  d.atrk = (const double *)c->s_atrk.p;
  d.atas = (const double *)c->s_atas.p;
  d.avs = (const double *)c->s_avs.p;
  d.aalt = (const double *)c->s_aalt.p;
  d.active = (const uint8_t *)c->s_active.p;
  d.sticky = (const unsigned *)((char *)c->sim_ctl.p + bsa::kSimCtlSticky);
  d.steps_done = (unsigned long long *)((char *)c->sim_ctl.p + kSimCtlSteps);
  return d;
}

// the ASAS bookkeeping's view of the sim (bsa_asas.hip), and K3's: full-n inputs, outputs on this rank's rows
static BkDev bk_dev(Ctx *c) {
  const SimDev s = sim_dev(c);
  char *ctl = (char *)c->sim_ctl.p;
  BkDev bk;
  bk.lat = s.lat, bk.lon = s.lon, bk.gse = s.gse, bk.gsn = s.gsn, bk.trk = s.trk;
  bk.h2id = (const unsigned *)c->h2id.p, bk.id2h = (const unsigned *)c->id2h.p;
  bk.active = (uint8_t *)c->s_active.p, bk.dropped = (uint8_t *)c->s_dropped.p, bk.dropcnt = (int *)c->s_dropcnt.p;
  bk.gate = (unsigned long long *)ctl, bk.sticky = (unsigned *)(ctl + kSimCtlSticky);
  bk.demand = (unsigned long long *)(ctl + kSimCtlDemand), bk.kdemand = (unsigned long long *)(ctl + kSimCtlKdemand);
  return bk;
}
static MvpDev mvp_dev(Ctx *c) {
  const SimDev s = sim_dev(c);
  const int64_t rb = c->sim_rb;
  MvpDev d;
  d.gseast = s.gse, d.gsnorth = s.gsn, d.vs = s.vs, d.alt = s.alt, d.trk = s.trk, d.gs = s.gs;
  d.selalt = (const double *)c->s_selalt.p, d.apvs = s.apvs, d.aptrk = s.aptrk, d.aptas = s.aptas, d.apalt = s.apalt;
  d.noreso = c->sim_noreso ? (const uint8_t *)c->s_noreso.p : nullptr;
  d.resooff = c->sim_resooff ? (const uint8_t *)c->s_resooff.p : nullptr;
  d.asas_alt = (double *)c->s_aalt.p + rb;
  d.o_trk = (double *)c->s_atrk.p + rb, d.o_tas = (double *)c->s_atas.p + rb, d.o_vs = (double *)c->s_avs.p + rb;
  d.o_asase = (float *)c->s_ase.p + rb, d.o_asasn = (float *)c->s_asn.p + rb;
  d.o_tsolv = nullptr;
  return d;
}

// Without wind, K4' sets gs = tas, trk = hdg and gseast / gsnorth =
// tas sin / cos(hdg) (traffic.py:455-460, bsa_kin_math.h): every rank derives
// the other ranks' gseast / gsnorth from their gathered gs / trk with the same
// expressions, bitwise, instead of receiving them (6 arrays over xGMI, not 8)
__global__ __launch_bounds__(256) void k_derive_gs(int n, int rb, int re, const double *__restrict__ gs,
                                                   const double *__restrict__ trk, double *__restrict__ gse,
                                                   double *__restrict__ gsn) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n || (k >= rb && k < re)) return;
  double st, ct;
  sincos(trk[k] * kD2R, &st, &ct);  // (as K4''s sincos of hdg)
  gsn[k] = gs[k] * ct;
  gse[k] = gs[k] * st;
}

// C1: replicate every rank's rows of the 8 arrays CD and MVP read for any row
static int sim_gather(Ctx *c) {
  if (c->nranks == 1 || c->sim_gathered) {
    c->sim_gathered = true;
    return 0;
  }
  SimDev d = sim_dev(c);
  // in place: the home ranges are contiguous and the arrays padded to nranks x rpr;
  // gseast / gsnorth are derived when every rank's came from K4' without wind
  double *const f[8] = {d.lat, d.lon, d.trk, d.gs, d.alt, d.vs, d.gse, d.gsn};
  const bool derive = c->simp.winddim == 0 && c->sim_gs_derivable;
  if (comm_allgather_inplace(c, f, derive ? 6 : 8, (size_t)c->sim_rpr)) return -1;
  if (derive) {
    hipLaunchKernelGGL(k_derive_gs, dim3((unsigned)((c->n + 255) / 256)), dim3(256), 0, c->stream, (int)c->n,
                       (int)c->sim_rb, (int)c->sim_re, (const double *)d.gs, (const double *)d.trk, d.gse, d.gsn);
    BSA_HIP(c, hipGetLastError());
  }
  c->sim_gathered = true;
  return 0;
}

// read-time gather of the per-rank ASAS outputs (only own rows are computed)
static int sim_gather_asas(Ctx *c) {
  if (c->nranks == 1) return 0;
  // (not synchronised here: the HomeBatch::run() of the read that follows does)
  return gather_rows(c, {{c->s_atrk.p, 8}, {c->s_atas.p, 8}, {c->s_avs.p, 8}, {c->s_aalt.p, 8}, {c->s_tas.p, 8},
                         {c->s_hdg.p, 8}, {c->s_active.p, 1}},
                     false);
}

// the resident step's last CD call as "the last detect" (its counts are
// read from the device; the host never synchronised on that detect)
int sim_adopt_pairs(Ctx *c) {
  if (c->have_pairs || !c->sim_ready || c->clk.cd_calls == 0) return 0;
  if (c->empty_detect) {
    c->last_conf = c->last_los = 0;
    c->have_pairs = true;
    return 0;
  }
  Counters h;
  BSA_HIP(c, hipMemcpyAsync(&h, c->counters.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  c->last_conf = (int64_t)h.conf;
  c->last_los = (int64_t)h.los;
  c->have_pairs = true;
  return 0;
}

void sim_release(Ctx *c) {
  for (const SimArray &a : kSimArrays) release(buf_at(c, a.buf));
  // not per aircraft: staging, control words, tables, the FMS undo set, K2 + K4' double buffers
  DevBuf *rest[] = {&c->red, &c->g_send, &c->g_recv, &c->pg_send, &c->pg_recv, &c->sim_ctl, &c->s_ptab, &c->s_ftab,
                    &c->f_const, &c->s_fmsrows, &c->s_fmstype, &c->s_fmsrows2, &c->s_fmstype2, &c->rt_stage, &c->rt_ws, &c->s_fmsur, &c->s_fmsuf, &c->s_fmsui, &c->gv_tab, &c->gv_shapes, &c->gv_undo,
                    &c->gv_cnt, &c->xfer_stage, &c->lbyidx, &c->xa_ws, &c->xa_rec, &c->tr_stage, &c->tr_seg, &c->tr_ws, &c->adsb_stage,
                    &c->fetch_stage, &c->tpr_snap, &c->tpr_ctl, &c->nx_alt, &c->nx_vs, &c->nx_gse, &c->nx_gsn};
  for (auto *b : rest) release(*b);
  bk_release(c);
  halo_release(c);
  comm_release(c);
}

// the maps of a home order h2id_h (host + device) and this rank's lpos
int set_home_maps(Ctx *c) {
  const int64_t n = c->n;
  c->id2h_h.assign((size_t)n, 0u);
  for (int64_t h = 0; h < n; ++h) c->id2h_h[c->h2id_h[(size_t)h]] = (unsigned)h;
  const int64_t rb = c->sim_rb, nr = c->sim_re - c->sim_rb;
  std::vector<unsigned> ord((size_t)nr);
  for (int64_t r = 0; r < nr; ++r) ord[(size_t)r] = (unsigned)r;
  std::sort(ord.begin(), ord.end(), [&](unsigned a, unsigned b) { return c->h2id_h[rb + a] < c->h2id_h[rb + b]; });
  c->lpos_h.assign((size_t)nr, 0u);
  for (int64_t k = 0; k < nr; ++k) c->lpos_h[ord[(size_t)k]] = (unsigned)k;
  if (!ensure(c, c->lbyidx, (size_t)std::max<int64_t>(nr, 1) * 4, "rows by index")) return -1;
  if (nr) BSA_HIP(c, hipMemcpyAsync(c->lbyidx.p, ord.data(), (size_t)nr * 4, hipMemcpyHostToDevice, c->stream));
  if (!ensure(c, c->h2id, (size_t)n * 4, "home -> index") || !ensure(c, c->id2h, (size_t)n * 4, "index -> home"))
    return -1;
  BSA_HIP(c, hipMemcpyAsync(c->h2id.p, c->h2id_h.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipMemcpyAsync(c->id2h.p, c->id2h_h.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

// rows of `rank`: a 512-aligned home range (the detect's row tiles are then
// column tiles)
void set_rank_rows(Ctx *c) {
  const int64_t n = c->n, R = c->nranks;
  c->sim_rpr = ((n + R - 1) / R + kTile - 1) / kTile * kTile;
  c->sim_rb = std::min<int64_t>(n, (int64_t)c->rank * c->sim_rpr);
  c->sim_re = std::min<int64_t>(n, c->sim_rb + c->sim_rpr);
}

// what one CD call hands to the step that enqueued it
struct CdOut {
  DetectResult det;           // (its kept K2 launch, its HK decision)
  bool mvp_deferred = false;  // K3's rows run inside the step's K4', with
  MvpIn mv{};                 // ... these arguments
};

// one CD call (enqueue only).  in_step (a CD step of bsa_sim_step): K3's
// per-row part may run inside the step's K4' (k_sim_pilot_kin<true>), which
// also publishes a host-decided detect's prediction, so the host may decide
// the list; a CD call without kinematics (bsa_sim_cd) launches K3 itself.
// keep_k2: the detect's K2 is left to the step too (StepPlan::k24), lean_k2: in its lean form (StepPlan::lean).  The
// caller counts the call (clk.cd_calls).  Its stages: gather, detect,
// bookkeeping count, gate all-reduce, K3, bookkeeping apply
static int sim_cd(Ctx *c, bool in_step, bool keep_k2, bool lean_k2, CdOut *out) {
  const bsa_sim_params &p = c->simp;
  // several ranks: the detect's halo exchange (bsa_halo.hip) refreshes the
  // other ranks' rows this rank reads; one rank holds everything
  if (c->halo_mode != 1 && sim_gather(c)) return -1;
  const BkDev bk = bk_dev(c);
  const MvpDev d = mvp_dev(c);
  DetectRequest q{p.rpz, p.hpz, p.tla, 0, c->sim_rb, c->sim_re, bk.gate};
  q.home = true;
  q.host_decides = in_step;
  q.keep_k2 = keep_k2;
  q.lean_k2 = keep_k2 && lean_k2;
  // MVP's per-pair vectors are evaluated by K2 as it places each pair;
  // k_mvp_row folds them after the gate
  if (p.reso) {
    q.mvp = &p.mvp;
    q.gse = d.gseast;
    q.gsn = d.gsnorth;
    q.vs = d.vs;
    q.alt = d.alt;
    q.noreso = d.noreso;
  }
  if (detect_enqueue(c, q, &out->det)) return -1;
  // ASAS bookkeeping, first half: kept-pair counts (may flag a resopairs overflow in the gate)
  if (p.resume_nav && bk_count(c, bk)) return -1;
  if (comm_allreduce_max_u64(c, bk.gate, kGateWords)) return -1;
  // K3 (+ gate, + asas.active = inconf unless ResumeNav runs) on the detect's own row offsets
  // without the bookkeeping (which runs between K3 and K4') K3's rows are
  // deferred into K4' of this step (k_sim_pilot_kin<true>)
  out->mvp_deferred = in_step && !p.resume_nav && c->sim_re > c->sim_rb;
  if (mvp_device(c, p.mvp, d, (const unsigned *)c->rowoff.p, bk.gate, bk.sticky,
                 p.resume_nav ? nullptr : (const uint8_t *)c->inconf.p, (uint8_t *)c->s_active.p, p.reso != 0,
                 out->det.pairs_done, out->det.rows_folded, out->mvp_deferred ? &out->mv : nullptr))
    return -1;
  // second half: resopairs rewrite, ResumeNav's asas.active, unique / cumulative counts
  return p.resume_nav ? bk_apply(c, bk) : 0;
}

// ---- one step of a batch: StepPlan (every decision, taken by step_decide
// from the host clocks before anything of the step is enqueued), one function
// per stage, step_enqueue runs them in order and step_advance moves the clocks
// (the stages in launch order: DESIGN.md 3.19; the detect side: DetectPlan, bsa_detect.h)
struct StepPlan {
  bool gv_apply;  // geovectoring applies in this step (geovec_applies_at on clk.gv_ctr)
  // OpenAP forces: the pending fuel of the step before is committed first --
  // not by the first step of a re-run attempt: it is the aborted step's own
  // 
  bool commit_fuel;
  // Autopilot.update ticks in this step: the reference's rule on the host's
  // copy of simt (autopilot.py:61-62, simulation.py:119); nothing is read back
  bool fms_tick;
  bool cd;  // a CD step (every cd_every steps)
  // one rank: K2 and this step's K4' as one launch (k24_launch; BSA_K24=0
  // off) -- K4' then starts on each workgroup's rows as soon as their fold is
  // done, instead of behind the whole of K2
  bool k24;
  // the fused K2 + K4' in its lean form: no block sums (no k_rowblk launch), no pair lists, no
  // rowoff, no conf / los counts -- a later CD step of the same bsa_sim_step call overwrites them all before the
  // host can read any, and with k24's conditions (one rank, no ASAS bookkeeping) nothing on the device reads them.
  // Not with a stage that can end the batch early (the stop protocol's: conditional commands, the experiment
  // area), whose stopping step would then be the one the host reads.  bsa_set_lean_pairs / BSA_LEAN_K2=0 off
  bool lean;
  // one rank, the next step a CD step: K4' also prepares that detect's
  // column records and boxes (its K0b launch is skipped; BSA_SIM_PREP=0 off)
  bool prep;
  // K4' workgroup size: one wave (at 100k rows 256-lane groups left half the
  // CUs one group short, 391 groups on 256 CUs: 0.1753 -> 0.1718 ms per
  // step with 64; BSA_K4_BLOCK=128/256 for A/B)
  int k4_block;
  bool sect_pass;  // the sector pass follows this step: clk.sect_ctr + 1 is a multiple of its cadence (3.27)
  // conditional commands (3.29): k_sim_cond is the step's last launch; cond_tag: the step's number in its batch
  // + 1, what a stop raised by it carries (no clock: the stage evaluates every step)
  bool cond;
  unsigned cond_tag;
  // the experiment area's pass (3.30) follows k_sim_cond: clk.area_ctr + 1 is a multiple of its cadence; a stop it
  // raises carries cond_tag too
  bool area_pass;
  // trails (3.31): Trails.update(trail_t) between k_sim_cond and the area's pass, behind the sticky word by
  // cond_tag; trail_t: clk.trail_simt at the step's start, the simt traf.update was called with
  bool trails;
  double trail_t;
  // the ADS-B model (3.32): ADSB.update(adsb_t) on the state the previous step left, before the FMS stage;
  // adsb_t: clk.adsb_simt at the step's start
  bool adsb;
  double adsb_t;
};
static StepPlan step_decide(const Ctx *c, bool rerun_first) {
  const DetectEnv &env = detect_env();
  const StepClocks &k = c->clk;
  const int64_t rb = c->sim_rb, re = c->sim_re;
  StepPlan sp{};
  sp.gv_apply = c->sim_gv && geovec_applies_at(c);
  sp.commit_fuel = !rerun_first;
  sp.fms_tick = c->sim_fms && fms_ticks_at(k.fms_simt, k.fms_t0);
  sp.cd = k.steps % c->simp.cd_every == 0;
  sp.k24 = sp.cd && env.k24 && c->nranks == 1 && c->halo_mode == 0 && !c->simp.resume_nav && re > rb &&
           c->k2_bucket > 0;
  sp.lean = sp.k24 && c->lean_on && env.lean_k2 && (c->lean_on == 2 || k.steps + c->simp.cd_every < c->batch_target) && !c->sim_cond &&
            !c->sim_exparea;
  sp.prep = env.sim_prep && c->nranks == 1 && c->home && !c->reuse_on && c->halo_mode == 0 && rb == 0 &&
            re == c->n && (k.steps + 1) % c->simp.cd_every == 0 &&
            !c->sim_turb;  // turbulence moves the aircraft after K4': the next detect makes its own records (K0b)
  sp.k4_block = env.k4_block;  // (PREP: whole waves = whole groups, rb = 0)
  sp.sect_pass = c->sim_sect && (k.sect_ctr + 1) % c->sect_every == 0;
  sp.cond = c->sim_cond;
  sp.cond_tag = (unsigned)(k.steps - c->batch_steps0 + 1);
  sp.area_pass = exparea_passes_at(c);
  sp.trails = c->sim_trails;
  sp.trail_t = k.trail_simt;
  sp.adsb = c->sim_adsb;
  sp.adsb_t = k.adsb_simt;
  return sp;
}

// The host clocks over one step: the only function that moves them.  step_enqueue calls it once everything
// of the step is enqueued; batch_rollback replays the completed steps of an aborted batch with it.  A stage
// that is off keeps its clock still
static void step_advance(Ctx *c, const StepPlan &sp) {
  StepClocks &k = c->clk;
  if (c->sim_gv) k.gv_ctr++;
  if (sp.fms_tick) k.fms_t0 = k.fms_simt, k.fms_ticks++;  // Autopilot.update's tick: t0 = simt (autopilot.py:62)
  if (c->sim_fms) k.fms_simt += c->simp.simdt;
  if (sp.cd) k.cd_calls++, (sp.lean ? k.lean_cd : k.full_cd)++;
  if (c->sim_turb) k.turb_call++;
  if (c->sim_sect) k.sect_ctr++;
  if (c->sim_exparea) k.area_ctr++;
  if (c->sim_trails) k.trail_last = k.trail_simt, k.trail_simt += c->simp.simdt;  // simt += simdt (simulation.py), accumulated as there
  if (c->sim_adsb) {  // simt as the trails' clock; the lastupdate buffers change roles; a call number per noisy update
    k.adsb_simt += c->simp.simdt, k.adsb_cur ^= 1;
    if (c->ad_noise) k.adsb_call++;
  }
  k.steps++;
}

// ---- a batch (the steps of one bsa_sim_step attempt, or one bsa_sim_cd
// call): enqueued without host synchronisation from the host state kept here,
// read back once (batch_end), rolled back to the aborted step if it aborted
struct BatchBase {
  bool kin;  // the batch runs K4' (bsa_sim_step; a CD call alone moves no state)
  StepClocks clk;
  bool gs_derivable;
};
static int batch_begin(Ctx *c, bool kin, BatchBase *b) {
  *b = BatchBase{kin, c->clk, c->sim_gs_derivable};
  c->batch_steps0 = c->clk.steps;
  BSA_HIP(c, hipMemsetAsync((char *)c->sim_ctl.p + kSimCtlSticky, 0, sizeof(BatchCtl), c->stream));
  return 0;
}
// the batch's only host synchronisation; the trail stage's words {total, demand} lie right behind the batch's and
// come back in the same copy
static int batch_end(Ctx *c, BatchCtl *ctl) {
  struct {
    BatchCtl ctl;
    unsigned trail[2];
  } h{};
  static_assert(sizeof(h) == kSimCtlAll - kSimCtlSticky, "the trail words follow BatchCtl");
  BSA_HIP(c, hipMemcpyAsync(&h, (char *)c->sim_ctl.p + kSimCtlSticky, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  *ctl = h.ctl;
  if (c->sim_trails) c->tr_undrained = h.trail[0], c->tr_demand = h.trail[1];
  return 0;
}

// An aborted batch: the state is that of the aborted step's start (step
// base.clk.steps + ctl.steps_done).  The gate is all-reduced, so every rank aborted at the
// same step; each rank grows only what overflowed on IT (another rank's
// overflow re-runs the step here with unchanged buffers) and all ranks re-run it
static int batch_rollback(Ctx *c, const BatchBase &base, const BatchCtl &ctl) {
  // the re-run rebuilds the candidate list and the tile-pair list / halo plan (every rank aborted alike) and zeroes
  // every per-detect buffer (an aborted K2 wrote no inconf / tcpamax); an aborted K4' prepared nothing, and the HK
  // decisions of the aborted steps never took effect
  invalidate(c, Change::BatchAborted);
  c->sim_aborts++;
  const int64_t done = (int64_t)ctl.steps_done;
  // the clocks of the completed steps, replayed from the batch base with each step's own plan (a CD call alone
  // completes no step: its count goes back to the base, the re-run counts it)
  c->clk = base.clk;
  for (int64_t k = 0; k < done; ++k) step_advance(c, step_decide(c, false));
  c->sim_gs_derivable = done > 0 ? c->simp.winddim == 0 : base.gs_derivable;  // K4' ran for the completed steps only
  if (base.kin) {
    c->sim_gathered = c->nranks == 1;
    // The aborted step's launches ran (later ones were no-ops): its plan, taken again on the replayed clocks,
    // says what they wrote.  A ticking FMS launch filled its undo set with the step's start -- put it back;
    // so did an applying geovector launch (later ones returned behind the sticky word) -- after the FMS undo
    // set, whose selspd / ap_trk / selalt are the values the stage left.
    // Turbulence: the draws are a pure function of (seed, call, index); the completed steps took one call
    // number each, the aborted step's k_sim_turb returned behind the sticky word -- nothing to undo.
    // Sectors: the pass only reads state; the completed steps' updates are counted, the aborted step's pass
    // returned behind the sticky word like every later one, so the re-run counts each update once.
    // Experiment area: the pass writes its accumulators only in steps that complete -- the abort is raised in the
    // step's detect, before the pass, which then returned behind the sticky word: nothing to undo, and the replayed
    // clock makes the re-run count the pass once.
    // Trails: an aborted step's pass wrote nothing, since the abort is raised in the step's detect -- its count
    // and emit launches returned behind the sticky word and left the running total as it was: nothing to undo,
    // and the replayed trail_simt hands the re-run the same t.
    // ADS-B: the stage runs BEFORE the step's detect, so the aborted step's launch did run.  Two lastupdate buffers:
    // it read the one clk.adsb_cur names and wrote the other for all its rows, and the replayed clock names the one
    // it read again, untouched; its picture writes are a pure function of that buffer, the state, adsb_simt and
    // adsb_call, all as they were, so the re-run writes the same values again.  Later launches returned behind the
    // sticky word.  Nothing to undo, no lastupdate += trunctime applied twice
    const StepPlan sp = step_decide(c, false);
    if (sp.fms_tick && fms_sim_restore(c)) return -1;
    if (sp.gv_apply && geovec_sim_restore(c)) return -1;
  }
  // the last detect's counters: every detect after the abort ran on the same, unchanged state
  Counters h;
  BSA_HIP(c, hipMemcpy(&h, c->counters.p, sizeof(h), hipMemcpyDeviceToHost));
  if (h.halo_miss)
    return fail(c, "internal error: the halo exchange and the tile-pair cull disagree (rank %d)", c->rank);
  // several ranks: every rank takes part in the capacity agreement (collective)
  if (c->halo_mode == 1 && halo_grow(c)) return -1;
  if (ctl.bk_demand > 0)  // this rank's resopairs outgrew their buffer
    c->bk_cap = std::max(2 * c->bk_cap, ctl.bk_demand + ctl.bk_demand / 4 + 1024);
  // pair keys outgrew their all-gather block on some rank: the block width is
  // part of the all-gather's layout, so every rank grows to the same width
  // (max-all-reduced demand; collective, every rank aborted at this step)
  // (with HK's stale flag: the device-decided stretch after a stale abort must
  // be the same on every rank -- the kept and the rebuilt plans issue
  // different collectives)
  double agree[2] = {(double)ctl.key_demand, ctl.stale ? 1.0 : 0.0};
  if (comm_multi(c) && comm_allreduce_host(c, agree, 2, true)) return -1;
  const double kdem = agree[0];
  if (agree[1] > 0.0) {  // an HK-kept list no longer covered some rank's records: device-decided for a while
    c->hk_stale++;
    c->hk.cool = c->hk_cool_len;
    c->hk_cool_len = std::min<int64_t>(2 * c->hk_cool_len, 4096);
  }
  if (kdem > 0)
    c->bk_kw = std::max<unsigned long long>(2 * c->bk_kw, (unsigned long long)kdem + (unsigned long long)kdem / 4 + 1024);
  if (detect_env().hk_trace)  // (diagnostics)
    fprintf(stderr, "[bsa hk] rank %d abort at step %lld: stale %d k2 %llu fuse %llu halo %llu/%llu\n", c->rank,
            (long long)c->clk.steps, ctl.stale ? 1 : 0, h.k2_demand, h.fuse_ovf, h.halo_ovf, h.halo_miss);
  if (h.k2_demand) grow_k2_bucket(c, h.k2_demand);  // a K2 row bucket was full on this rank
  if (h.fuse_ovf) {  // fused K1b out of flush records: the re-run's detect unfused
    c->fuse_skip = true;
    c->fuse_retries++;
  }
  // candidate overflow on this rank: enough for the last detect's demand (its
  // shard counters keep counting past the capacity)
  unsigned long long worst = 0;
  for (int q = 0; q < kCandShards; ++q) worst = std::max(worst, h.cshard[q][0]);
  if (worst > c->cand_cap / kCandShards)
    c->cand_cap = std::max(2 * c->cand_cap, (unsigned long long)kCandShards * (worst + worst / 4 + 1024));
  return 0;
}

// A stopped batch (kStickyStopped, bsa_internal.h): a stage of step `done` (counted from the batch base) raised
// the stop after that step was complete; every launch of the later steps returned behind the sticky word (the
// fused K2 + K4' copies its double buffers' halves, so the host's swaps of the no-op steps stay right, as after
// an abort).  The device state is exactly that after step `done`: nothing is re-run, nothing grown -- whatever a
// later, no-op step's detect overflowed is found again by the step the host resumes with.  The FMS and geovector
// undo sets are NOT put back: the step after the stop never executed, its launches returned before they saved
// anything, so the sets hold an earlier, completed tick's start.  Host state step_enqueue moved for the no-op
// steps: the clocks are replayed over the completed steps as batch_rollback does; prep.keep / drop and the HK
// decisions go with Change::BatchStopped; sim_gs_derivable / sim_gathered are those after a completed K4'.
// Every stopping stage with something for the host stored the step's tag into its pending word, the raiser too:
// each of them is told (stage_stopped), and its poll delivers
void stage_stopped(Ctx *c, StopStage s) { c->stops[s] = StopSide{true, c->clk.steps}; }

static int batch_stopped(Ctx *c, const BatchBase &base, const BatchCtl &ctl) {
  const unsigned stage = stop_stage(ctl.stop);
  const int64_t done = (int64_t)ctl.steps_done, tag = (int64_t)stop_tag(ctl.stop);
  if (done < 1 || tag != done || stage == kStopNone || stage >= kStopCount || ctl.pend[stage] != (unsigned long long)tag)
    return fail(c, "internal error: batch stopped by stage %u in step %lld with %lld steps done", stage, (long long)tag,
                (long long)done);
  invalidate(c, Change::BatchStopped);
  c->clk = base.clk;
  for (int64_t k = 0; k < done; ++k) step_advance(c, step_decide(c, false));
  c->sim_gs_derivable = c->simp.winddim == 0;
  c->sim_gathered = c->nranks == 1;
  for (unsigned s = kStopNone + 1; s < kStopCount; ++s)
    if (ctl.pend[s] == (unsigned long long)tag) stage_stopped(c, (StopStage)s);
  return 0;
}

static int check_params(Ctx *c, const bsa_sim_params *p) {
  if (p->cd_every < 1) return fail(c, "cd_every must be >= 1");
  if (p->resume_nav != 0 && p->resume_nav != 1) return fail(c, "resume_nav must be 0 or 1");
  if (p->winddim < 0 || p->winddim > 3) return fail(c, "winddim must be 0, 1, 2 or 3");
  if (p->reso != 0 && p->reso != 1) return fail(c, "reso must be 0 or 1");
  return 0;
}

// K4' as the preparer of the next detect's column records and boxes
// (StepPlan::prep): their buffers, a fresh non-finite epoch and, with a kept
// tile-pair list, its budgets.  After the step's CD call: Ctx::tiles and
// Ctx::hk.m are that detect's
static int step_prep_args(Ctx *c, PrepArgs *out) {
  PrepArgs &pa = *out;
  const int64_t n = c->n;
  pa.rec = home_records(c, n) ? 1 : 0;
  if (!ensure_col_prep(c, n, pa.rec != 0)) return -1;
  pa.out = PrepOut{(ColRec *)c->colrec.p, (PFRec *)c->pfcol.p, (PFVel *)c->pfvcol.p, (float4 *)c->pfpcol.p};
  pa.sbox = (TileBox *)c->sbox_c.p;
  pa.gbox = (TileBox *)c->gbox_c.p;
  pa.rpz = c->simp.rpz;
  pa.hpz = c->simp.hpz;
  pa.tla = c->simp.tla;
  pa.mid = stage1_mid(0, false, 0);
  pa.n = (int)n;
  if (!nonfin_word(c)) return -1;
  pa.nf = (unsigned long long *)c->nonfin.p;  // the next detect's records: a fresh epoch
  pa.nfe = c->nf_prep_epoch = ++c->nf_counter;
  if (c->tiles.kept_for(n) && c->tpr_snap.p && c->tpr_ctl.p) {  // the kept list's budgets
    pa.snap = (const PFRec *)c->tpr_snap.p;
    pa.tpr_ctl = (unsigned long long *)c->tpr_ctl.p;
    pa.dx = c->tpr_dx;
    pa.ds = c->tpr_ds;
    pa.dv = c->tpr_dv;
    // HK: the prediction word of the next detect (index hk.m, if it is host-decided)
    pa.pred = (unsigned long long *)c->tpr_ctl.p + 6 + (c->hk.m & 1);
    pa.pf = c->hk_f;
  }
  return 0;
}

// HK: the CD step's K4' (or K2 + K4') publishes a host-decided detect's
// prediction -- the rank's own word with K2 fused, else gate[2] after K2 and
// the all-reduce
static HkPub step_hk_pub(const Ctx *c, const DetectResult &det) {
  HkPub pub{};
  if (!det.hk) return pub;
  pub.slot = c->hk_hdev + (det.hk_m % kHkRing);
  pub.base = (unsigned long long)(det.hk_m + 1) << 2;
  if (det.k2_kept) {
    pub.src = (unsigned long long *)c->tpr_ctl.p + 6 + (det.hk_m & 1);
    pub.zero = 1;
  } else {
    pub.src = (unsigned long long *)c->sim_ctl.p + 2;
  }
  return pub;
}

// K4' of the step, or (the detect kept its K2) K2 + K4' as one launch on
// double-buffered alt / vs / gse / gsn
static int step_launch(Ctx *c, const StepPlan &sp, const CdOut &cd, const PrepArgs &pa, const HkPub &pub) {
  const bsa_sim_params &p = c->simp;
  const int64_t rb = c->sim_rb, re = c->sim_re, n = c->n;
  WindField wf = wind_field(c);
  if (p.winddim == 3) {  // the 3-D field at the pre-step state of the own rows: K4' (either form) reads it per aircraft
    const SimDev d0 = sim_dev(c);
    if (wind3d_launch(c, rb, re, n, d0.lat, d0.lon, d0.alt)) return -1;
    wf = wind_field_pa(c);
  }
  if (sp.lean && !(cd.det.k2_kept && cd.det.k2.lean)) return fail(c, "internal: a lean step without its lean K2 + K4'");
  if (cd.det.k2_kept) {
    if (!cd.mvp_deferred) return fail(c, "internal: fused K2 + K4' without the deferred MVP rows");
    if (!ensure(c, c->nx_alt, n * 8, "next altitudes") || !ensure(c, c->nx_vs, n * 8, "next vs") ||
        !ensure(c, c->nx_gse, n * 8, "next gseast") || !ensure(c, c->nx_gsn, n * 8, "next gsnorth"))
      return -1;
    SimDev d = sim_dev(c);
    d.alt_w = (double *)c->nx_alt.p;
    d.vs_w = (double *)c->nx_vs.p;
    d.gse_w = (double *)c->nx_gse.p;
    d.gsn_w = (double *)c->nx_gsn.p;
    const K24Args ka{d, cd.mv, p.mvp, pa, wf, p.simdt, p.windnorth, p.windeast, p.winddim,
                     sp.prep ? 1 : 0, pub};
    if (k24_launch(c, cd.det.k2, cd.det.k2_ev, ka)) return -1;
    std::swap(c->own[4], c->nx_alt);
    std::swap(c->own[5], c->nx_vs);
    std::swap(c->s_gse, c->nx_gse);
    std::swap(c->s_gsn, c->nx_gsn);
  } else {
    const int blk = sp.k4_block;
    const int64_t nb = std::max<int64_t>(1, (re - rb + blk - 1) / blk);
    const auto K4 = cd.mvp_deferred ? (sp.prep ? k_sim_pilot_kin<true, true> : k_sim_pilot_kin<true, false>)
                                    : (sp.prep ? k_sim_pilot_kin<false, true> : k_sim_pilot_kin<false, false>);
    hipLaunchKernelGGL(K4, dim3((unsigned)nb), dim3(blk), 0, c->stream, (int)rb, (int)re, p.simdt, p.winddim,
                       p.windnorth, p.windeast, wf, sim_dev(c), cd.mv, p.mvp, pa, pub);
  }
  BSA_HIP(c, hipGetLastError());
  return 0;
}

// one step of the batch (enqueue only), the stages in their fixed order, and the host state
// that follows it.  The clocks move last: a step that fails to enqueue leaves them at its start
static int step_enqueue(Ctx *c, const StepPlan &sp) {
  // geovectoring is the plugin's preupdate (tools/plugin.py:161-169): the first launch on the step's stream, so
  // that Autopilot.update already reads the limited selspd / selvs / selalt / ap.trk
  if (sp.gv_apply && geovec_sim_launch(c)) return -1;
  // adsb.update(simt) (traffic.py:392): the broadcast picture of the state the previous step left
  if (sp.adsb && adsb_sim_launch(c, sp.adsb_t)) return -1;
  // (forces and FMS read the pre-step state)
  if (c->sim_forces && forces_sim_launch(c, sp.commit_fuel)) return -1;
  if (c->sim_fms && fms_sim_launch(c, sp.fms_tick)) return -1;  // Autopilot.update (bsa_fms.hip)
  CdOut cd;
  if (sp.cd && sim_cd(c, true, sp.k24, sp.lean, &cd)) {
    invalidate(c, Change::StepNotEnqueued);  // (a detect may have been enqueued without its step's publication)
    return -1;
  }
  // waypoint recovery of the pairs ResumeNav just dropped: on the pre-step state, before K4' reads ap.alt
  if (c->sim_recovery && sp.cd && c->sim_fms && c->simp.resume_nav && fms_sim_recover(c)) return -1;
  PrepArgs pa{};
  if (sp.prep && step_prep_args(c, &pa)) return -1;
  if (step_launch(c, sp, cd, pa, step_hk_pub(c, cd.det))) return -1;
  if (c->sim_turb) {  // Turbulence.Woosh, the last statement of Traffic.update (traffic.py:416), on what K4' wrote
    const SimDev d = sim_dev(c);
    if (turb_sim_launch(c, c->sim_rb, c->sim_re, d.sticky, d.trk, d.lat, d.lon, d.alt)) return -1;
  }
  if (sp.sect_pass && sect_sim_launch(c)) return -1;  // sector occupancy: reads what the step left (sectorcount.py:53-79)
  // cond.update() (traffic.py:419): reads what the step left; last, so that a stop it raises cuts nothing of this step
  if (sp.cond && cond_sim_launch(c, sp.cond_tag)) return -1;
  // trails.update(simt), the last statement of Traffic.update (traffic.py:422): on the positions the step left
  if (sp.trails && trails_sim_launch(c, sp.trail_t, sp.cond_tag)) return -1;
  // the AREA plugin's update follows traf.update (simulation.py: plugin.update after traf.update), whose last
  // statements are cond.update() and trails.update: the step's last launch
  if (sp.area_pass && exparea_sim_launch(c, sp.cond_tag)) return -1;
  if (sp.prep)
    c->prep.keep({pa.rpz, pa.hpz, pa.tla, (double)pa.mid, c->n});
  else
    c->prep.drop();
  // every rank's rows now hold K4's gs / trk / gse / gsn: gse / gsn follow
  // from gs / trk bitwise only without wind (with wind gs / trk derive from
  // them, traffic.py:463-466, not the other way round)
  c->sim_gs_derivable = c->simp.winddim == 0;
  c->sim_gathered = c->nranks == 1;
  step_advance(c, sp);
  return 0;
}

// every stage with a launch of its own, off (fms_off takes recovery and the geovectors with it): a new sim
static void stages_off(Ctx *c) { forces_off(c), fms_off(c), turb_off(c), sect_off(c), cond_off(c), exparea_off(c), trails_off(c), adsb_off(c); }

// bsa_sim_create_with's hooks of the envelope and of OpenAP's type index (bsa_internal.h)
int limits_created(Ctx *c, int64_t n, int64_t m, const bsa_sim_create_extra &x) {
  if (!c->sim_limits) return 0;
  const double *src[6] = {x.hmax, x.vmin, x.vmax, x.vsmin, x.vsmax, x.axmax};
  for (int k = 0; k < 6; ++k)
    BSA_HIP(c, hipMemcpyAsync((double *)c->s_env.p + (size_t)k * (n + m) + n, src[k], (size_t)m * 8, hipMemcpyHostToDevice,
                              c->stream));
  return 0;
}

int perf_created(Ctx *c, int64_t n, int64_t m, const bsa_sim_create_extra &x) {
  if (!c->sim_perf) return 0;
  BSA_HIP(c, hipMemcpyAsync((int32_t *)c->s_ptype.p + n, x.type_idx, (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
  return 0;
}

}  // namespace bsa

using bsa::Ctx;

extern "C" {

int bsa_sim_init(bsa_ctx *cc, int64_t n, const bsa_sim_state *s, const bsa_sim_params *p) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!s || !p) return bsa::fail(c, "NULL sim state / params");
  // every parameter is checked before anything is uploaded; a failed init
  // leaves no half-initialised sim behind (sim_ready stays false)
  c->sim_ready = false;
  if (n <= 0 || n > 0x7fffffff) return bsa::fail(c, "bad n");
  if (bsa::check_params(c, p)) return -1;
  BSA_HIP(c, hipSetDevice(c->device));
  for (int k = 0; k < bsa::kSimStateFields; ++k)
    if (!bsa::ptr_at(s, k)) return bsa::fail(c, "bsa_sim_init: NULL array");
  // aircraft-index order first: the home order is the spatial order of this state
  if (bsa_set_state(cc, n, s->lat, s->lon, s->trk, s->gs, s->alt, s->vs)) return -1;
  if (bsa::home_order(c, p->tla, c->h2id_h)) return -1;
  bsa::set_rank_rows(c);
  if (bsa::set_home_maps(c)) return -1;
  c->sim_noreso = c->sim_resooff = false;  // empty NORESO / RESOOFF lists
  c->sim_atmos = c->sim_limits = c->sim_perf = false;
  bsa::stages_off(c);
  c->area_tab.clear();
  // every always-present array (kSimArrays); the all-gathered ones hold nranks
  // x rpr entries (in-place all-gather).  Zero unless a state field fills it:
  // asas.vs, asase / asasn, inactive, traf.ax, no ResumeNav drops
  const size_t NG = (size_t)std::max<int64_t>(n, c->sim_rpr * c->nranks);
  for (const bsa::SimArray &a : bsa::kSimArrays) {
    if (a.guard != bsa::kSimAlways) continue;
    bsa::DevBuf &b = bsa::buf_at(c, a.buf);
    if (!bsa::ensure(c, b, (a.gathered ? NG : (size_t)n) * a.esz, "sim state")) return -1;
    if (!bsa::sim_field_names(c, &b)) BSA_HIP(c, hipMemsetAsync(b.p, 0, (size_t)n * a.esz, c->stream));
  }
  // the state, and what starts at it: asas.trk / tas at traf.trk / tas (asas.py:405-409)
  bsa::HomeBatch up(c, true);
  for (int k = 0; k < bsa::kSimStateFields; ++k) {
    const bsa::SimField &f = bsa::kSimFields[k];
    if (up.add(bsa::buf_at(c, f.buf).p, bsa::ptr_at(s, k), nullptr, 8) ||
        (f.also && up.add((c->*f.also).p, bsa::ptr_at(s, k), nullptr, 8)))
      return -1;
  }
  if (up.run()) return -1;
  if (!bsa::ensure(c, c->sim_ctl, bsa::kSimCtlAll, "sim control words")) return -1;
  BSA_HIP(c, hipMemsetAsync(c->sim_ctl.p, 0, bsa::kSimCtlAll, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  c->simp = *p;
  c->bk_ready = false;  // empty resopairs / previous pair sets
  // several ranks: halo exchange instead of the full all-gather, with exact
  // initial capacities (every rank holds the whole state now)
  c->halo_mode = c->nranks > 1 ? 1 : 0;
  if (bsa::halo_init_caps(c)) return -1;
  c->clk = bsa::StepClocks{};
  c->sim_aborts = 0;
  c->sim_last_conf = c->sim_last_los = 0;
  c->sim_gathered = true;
  bsa::invalidate(c, bsa::Change::NewSim);
  c->hk.cool = 0;
  c->hk_cool_len = 32;
  if (!c->hk_host) {     // HK: the pinned ring the steps' K4' publish their predictions into
    void *hp = nullptr;
    BSA_HIP(c, hipHostMalloc(&hp, (size_t)bsa::kHkRing * 8, hipHostMallocMapped | hipHostMallocCoherent));
    memset(hp, 0, (size_t)bsa::kHkRing * 8);
    c->hk_host = (unsigned long long *)hp;
    void *dp = nullptr;
    BSA_HIP(c, hipHostGetDevicePointer(&dp, hp, 0));
    c->hk_hdev = (unsigned long long *)dp;
  }
  c->sim_gs_derivable = false;  // gseast / gsnorth are the host's until K4' runs
  if (c->feed_pending) {  // a snapshot of the previous sim is dropped
    BSA_HIP(c, hipEventSynchronize(c->feed_ev));
    c->feed_pending = false;
  }
  c->home = true;
  c->sim_ready = true;
  return 0;
}

int bsa_sim_step(bsa_ctx *cc, int nsteps) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_step before bsa_sim_init");
  if (c->simp.winddim == 2 && c->wf_nvec < 1)
    return bsa::fail(c, "winddim 2 needs a wind field (bsa_set_windfield)");
  if (c->simp.winddim == 3 && c->wf3_nvec < 1)
    return bsa::fail(c, "winddim 3 needs a 3-D wind field (bsa_set_windfield3d)");
  if (nsteps < 0) return bsa::fail(c, "negative step count");
  if ((c->sim_cond || c->sim_exparea) && (unsigned)nsteps > bsa::kStopTagMax)
    return bsa::fail(c, "at most %u steps per call while a stage that can stop the batch is on", bsa::kStopTagMax);
  BSA_HIP(c, hipSetDevice(c->device));
  if (bsa::trails_reserve(c, nsteps)) return -1;  // (before anything is enqueued: a refused batch runs no step)
  const int64_t start = c->clk.steps, target = start + nsteps;
  c->batch_target = target;
  c->steps_last = 0;
  for (int attempt = 0; c->clk.steps < target; ++attempt) {
    if (attempt > 6) return bsa::fail(c, "candidate buffer overflow in the resident step (retries exhausted)");
    bsa::BatchBase base;
    if (bsa::batch_begin(c, true, &base)) return -1;
    while (c->clk.steps < target)
      if (bsa::step_enqueue(c, bsa::step_decide(c, attempt > 0 && c->clk.steps == base.clk.steps))) return -1;
    bsa::BatchCtl ctl{};
    if (bsa::batch_end(c, &ctl)) return -1;  // did every step complete?
    if (c->sim_trails && c->tr_demand)
      return bsa::fail(c, "internal error: %lld trail segments did not fit the buffers sized for the batch", (long long)c->tr_demand);
#ifdef BSA_PF_TRACE
    if (bsa::pf_trace_dump(c, 0, 0)) return -1;  // (diagnostic builds: the batch's last prefilter)
#endif
    if (ctl.stop != 0) {  // stopped: the host has to act before the next step (bsa_sim_steps_run tells how far it got)
      if (bsa::batch_stopped(c, base, ctl)) return -1;
      break;
    }
    if (ctl.sticky == 0) break;
    if (bsa::batch_rollback(c, base, ctl)) return -1;
  }
  c->steps_last = c->clk.steps - start;
  return 0;
}

int bsa_sim_aborts(bsa_ctx *cc, int64_t *aborts) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_aborts before bsa_sim_init");
  if (aborts) *aborts = c->sim_aborts;
  return 0;
}

int bsa_sim_steps_run(bsa_ctx *cc, int64_t *last_batch, int64_t *total) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_steps_run before bsa_sim_init");
  if (last_batch) *last_batch = c->steps_last;
  if (total) *total = c->clk.steps;
  return 0;
}

int bsa_sim_set_limits(bsa_ctx *cc, const double *hmax, const double *vmin, const double *vmax,
                       const double *vsmin, const double *vsmax, const double *axmax) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_limits before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  if (!hmax) {
    c->sim_limits = false;
    return 0;
  }
  const double *src[6] = {hmax, vmin, vmax, vsmin, vsmax, axmax};
  for (auto q : src)
    if (!q) return bsa::fail(c, "bsa_sim_set_limits: NULL envelope array");
  const size_t N8 = (size_t)c->n * 8;
  if (!bsa::ensure(c, c->s_env, 6 * N8, "OpenAP envelope")) return -1;
  bsa::HomeBatch up(c, true);
  for (int k = 0; k < 6; ++k)
    if (up.add((char *)c->s_env.p + k * N8, src[k], nullptr, 8)) return -1;
  if (up.run()) return -1;
  c->sim_limits = true;
  return 0;
}

int bsa_sim_set_perf(bsa_ctx *cc, int64_t ntypes, const double *table, const int32_t *type_idx) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_perf before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  bsa::forces_off(c);  // the force table goes with the type table: bsa_sim_set_forces again
  if (!table) {
    c->sim_perf = false;
    return 0;
  }
  if (ntypes < 1 || !type_idx) return bsa::fail(c, "bsa_sim_set_perf: bad type table");
  // every index and lift type is checked here: the kernel reads the table unguarded
  for (int64_t t = 0; t < ntypes; ++t) {
    const double lt = table[t * bsa::kin::kPerfCols + 22];
    if (lt != 0.0 && lt != 1.0 && lt != 2.0) return bsa::fail(c, "type %lld: lifttype must be 0, 1 or 2", (long long)t);
  }
  const int64_t n = c->n;
  for (int64_t k = 0; k < n; ++k)
    if (type_idx[k] < 0 || type_idx[k] >= ntypes)
      return bsa::fail(c, "aircraft %lld: type index %d outside [0, %lld)", (long long)k, type_idx[k], (long long)ntypes);
  const size_t tb = (size_t)ntypes * bsa::kin::kPerfCols * 8;
  if (!bsa::ensure(c, c->s_ptab, tb, "OpenAP type table") || !bsa::ensure(c, c->s_ptype, (size_t)n * 4, "type index") ||
      !bsa::ensure(c, c->s_phase, (size_t)n, "flight phase"))
    return -1;
  BSA_HIP(c, hipMemcpyAsync(c->s_ptab.p, table, tb, hipMemcpyHostToDevice, c->stream));
  bsa::HomeBatch up(c, true);
  if (up.add(c->s_ptype.p, type_idx, nullptr, 4) || up.run()) return -1;
  BSA_HIP(c, hipMemsetAsync(c->s_phase.p, 0, (size_t)n, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  c->sim_perf = true;
  c->sim_ntypes = ntypes;
  return 0;
}

int bsa_sim_read_perf(bsa_ctx *cc, uint8_t *phase, double *ax) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_read_perf before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  if (phase && !c->sim_perf) return bsa::fail(c, "no flight phase: bsa_sim_set_perf is off");
  bsa::HomeBatch down(c, false, c->sim_rb, c->sim_re);
  if ((phase && down.add(c->s_phase.p, nullptr, phase, 1)) || (ax && down.add(c->s_ax.p, nullptr, ax, 8))) return -1;
  return down.run();
}

int bsa_sim_update(bsa_ctx *cc, const bsa_sim_state *s) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!s) return bsa::fail(c, "NULL sim state");
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_update before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  // the replicated CD inputs are rewritten on every rank (in the sim's home order)
  bool any_cd = false, all_rep = true;
  bsa::HomeBatch hb(c, true);
  for (int k = 0; k < bsa::kSimStateFields; ++k) {
    const bsa::SimField &f = bsa::kSimFields[k];
    const void *src = bsa::ptr_at(s, k);
    if (!src) {
      all_rep = all_rep && !f.replicated;
      continue;
    }
    any_cd = any_cd || f.cd_input;
    if (hb.add(bsa::buf_at(c, f.buf).p, src, nullptr, 8)) return -1;
  }
  if (hb.run()) return -1;
  bsa::invalidate(c, any_cd ? bsa::Change::EditedCdInput : bsa::Change::EditedArrays);
  if (any_cd) {
    // every rank passed the same full arrays: the replicas are consistent only
    // if ALL replicated arrays were passed; otherwise the next all-gather
    // repairs the other ranks' rows of the arrays not passed (each rank's
    // own rows are right either way)
    if (all_rep) c->sim_gathered = true;
    c->sim_gs_derivable = false;  // (gseast / gsnorth may be the host's)
  }
  return 0;
}

int bsa_sim_read(bsa_ctx *cc, bsa_sim_out *o) {
  Ctx *c = (Ctx *)cc;
  if (!c || !o) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_read before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  if (bsa::sim_gather(c) || bsa::sim_gather_asas(c)) return -1;
  // bsa_sim_out starts as bsa_sim_state does; then asas trk / tas / vs / alt and active
  bsa::HomeBatch hb(c, false);
  for (int k = 0; k < bsa::kSimOutFields; ++k)
    if (bsa::ptr_at(o, k) && hb.add(bsa::buf_at(c, bsa::kSimFields[k].buf).p, nullptr, bsa::ptr_at(o, k), 8)) return -1;
  void *asas[5] = {o->asas_trk, o->asas_tas, o->asas_vs, o->asas_alt, o->active};
  const int from[5] = {0, 1, 2, 3, 6};
  for (int k = 0; k < 5; ++k) {
    const bsa::AsasArray &a = bsa::kAsasArrays[from[k]];
    if (asas[k] && hb.add((c->*a.buf).p, nullptr, asas[k], a.esz)) return -1;
  }
  return hb.run();
}

int bsa_sim_stats(bsa_ctx *cc, int64_t *out6) {
  Ctx *c = (Ctx *)cc;
  if (!c || !out6) return -1;
  if (c->clk.cd_calls > 0 && c->counters.p) {  // counts of the last CD step
    BSA_HIP(c, hipSetDevice(c->device));
    bsa::Counters h;
    BSA_HIP(c, hipMemcpyAsync(&h, c->counters.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    BSA_HIP(c, hipStreamSynchronize(c->stream));
    c->sim_last_conf = (int64_t)h.conf;
    c->sim_last_los = (int64_t)h.los;
  }
  out6[0] = c->clk.steps;
  out6[1] = c->clk.cd_calls;
  out6[2] = c->sim_last_conf;
  out6[3] = c->sim_last_los;
  out6[4] = c->sim_rb;
  out6[5] = c->sim_re;
  return 0;
}

int bsa_sim_detect_rows(bsa_ctx *cc, int64_t row_begin, int64_t row_end, int64_t *n_conf, int64_t *n_los) {
  Ctx *c = (Ctx *)cc;
  if (!c || !n_conf || !n_los) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_detect_rows before bsa_sim_init");
  if (row_begin % bsa::kTile != 0) return bsa::fail(c, "row_begin must be a multiple of %d", bsa::kTile);
  BSA_HIP(c, hipSetDevice(c->device));
  if (bsa::sim_gather(c)) return -1;
  // as one rank of a sharded step: own tiles, halo plan, halo tiles (the
  // boxes of every tile, which the other ranks would send, are prepared
  // first, outside the detect's timed stages).  Those records carry the
  // detect's non-finite epoch: a NaN column outside this share's halo makes
  // every row's tcpamax NaN, as in the whole detect (StateBasedCD.py:90; the
  // sharded step carries it through the gate all-reduce instead)
  if (!bsa::nonfin_word(c)) return -1;
  const unsigned long long e = ++c->nf_counter;
  if (bsa::prep_all_tiles(c, c->simp.rpz, c->simp.hpz, c->simp.tla, e)) return -1;
  const int hm = c->halo_mode;
  c->halo_mode = 2;
  bsa::DetectRequest q{c->simp.rpz, c->simp.hpz, c->simp.tla, 0, row_begin, row_end};
  q.home = true;
  q.nf_epoch = e;  // (retries of the detect too)
  const int r = bsa::detect(c, q, n_conf, n_los);
  c->halo_mode = hm;
  return r;
}

int bsa_sim_probe_rank(bsa_ctx *cc, int rank, int nranks) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_probe_rank before bsa_sim_init");
  if (c->nranks != 1) return bsa::fail(c, "bsa_sim_probe_rank: a one-rank sim only (it plays one rank of several)");
  if (nranks < 1 || rank < 0 || rank >= nranks) return bsa::fail(c, "bad probe rank %d of %d", rank, nranks);
  BSA_HIP(c, hipSetDevice(c->device));
  const int64_t n = c->n;
  bsa::invalidate(c, bsa::Change::OtherRows);
  if (nranks == 1) {  // back to the whole sim
    c->sim_rb = 0;
    c->sim_re = n;
    c->halo_mode = 0;
    return bsa::set_home_maps(c);  // (the rows' index order: row ids, fetched pairs)
  }
  // the rank's home range (bsa_sim_init's partition) and the one-GPU halo
  // mode of bsa_sim_detect_rows: the other ranks' tiles are prepared once here
  // (their rows do not move: only this rank's K4' runs), the rank's own tiles
  // and its halo by every detect
  const int64_t rpr = ((n + nranks - 1) / nranks + bsa::kTile - 1) / bsa::kTile * bsa::kTile;
  c->sim_rb = std::min<int64_t>(n, (int64_t)rank * rpr);
  c->sim_re = std::min<int64_t>(n, c->sim_rb + rpr);
  if (c->sim_rb % bsa::kTile != 0) return bsa::fail(c, "probe rank %d of %d holds no rows", rank, nranks);
  if (bsa::set_home_maps(c) || bsa::sim_gather(c) || bsa::prep_all_tiles(c, c->simp.rpz, c->simp.hpz, c->simp.tla))
    return -1;
  c->halo_mode = 2;
  return 0;
}

int bsa_sim_halo_stats(bsa_ctx *cc, int64_t *out4) {
  Ctx *c = (Ctx *)cc;
  if (!c || !out4) return -1;
  BSA_HIP(c, hipSetDevice(c->device));
  unsigned tiles = 0;
  if (c->h_dem.p) {  // the received-tile total of the last plan (after its demand words)
    BSA_HIP(c, hipMemcpyAsync(&tiles, (const unsigned *)c->h_dem.p + c->halo_tot_word, 4, hipMemcpyDeviceToHost,
                              c->stream));
    BSA_HIP(c, hipStreamSynchronize(c->stream));
  }
  out4[0] = c->halo_rx;
  out4[1] = c->halo_tx;
  out4[2] = tiles;
  out4[3] = c->halo_grows;
  return 0;
}

int bsa_sim_set_halo_cap(bsa_ctx *cc, int sender, int receiver, int64_t tiles) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  const int R = c->nranks;
  if ((int64_t)c->halo_cap.size() != (int64_t)R * R) return bsa::fail(c, "no halo capacities (one rank, or no sim)");
  if (sender < 0 || sender >= R || receiver < 0 || receiver >= R || sender == receiver || tiles < 0)
    return bsa::fail(c, "bad halo capacity %d -> %d = %lld", sender, receiver, (long long)tiles);
  c->halo_cap[(size_t)sender * R + receiver] = tiles;
  return 0;
}

int bsa_sim_halo_recheck(bsa_ctx *cc) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  c->halo_chk_gen = -1;  // (collective by contract: every rank calls it before the same step)
  return 0;
}

int bsa_sim_row_ids(bsa_ctx *cc, int32_t *ids) {
  Ctx *c = (Ctx *)cc;
  if (!c || !ids) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_row_ids before bsa_sim_init");
  const int64_t rb = c->sim_rb, nr = c->sim_re - c->sim_rb;
  for (int64_t r = 0; r < nr; ++r) ids[c->lpos_h[(size_t)r]] = (int32_t)c->h2id_h[(size_t)(rb + r)];
  return 0;
}

int bsa_sim_asas_stats(bsa_ctx *cc, int64_t *out6) {
  Ctx *c = (Ctx *)cc;
  if (!c || !out6) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_asas_stats before bsa_sim_init");
  if (!c->simp.resume_nav) return bsa::fail(c, "ASAS bookkeeping is off (resume_nav = 0)");
  BSA_HIP(c, hipSetDevice(c->device));
  unsigned long long st[8] = {0};
  if (c->bk_ready) BSA_HIP(c, hipMemcpyAsync(st, c->bk_stats.p, 64, hipMemcpyDeviceToHost, c->stream));
  const int64_t rb = c->sim_rb, nr = c->sim_re - c->sim_rb;
  std::vector<uint8_t> act((size_t)std::max<int64_t>(nr, 1));
  if (nr > 0) BSA_HIP(c, hipMemcpyAsync(act.data(), (uint8_t *)c->s_active.p + rb, nr, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  int64_t na = 0;
  for (int64_t k = 0; k < nr; ++k) na += act[k] ? 1 : 0;
  out6[0] = (int64_t)st[0];
  for (int k = 1; k < 5; ++k) out6[k] = (int64_t)st[k];  // global sets (identical on every rank)
  out6[5] = na;
  return 0;
}

int bsa_sim_resopairs(bsa_ctx *cc, int32_t *idx1, int32_t *idx2, int64_t cap, int64_t *count) {
  Ctx *c = (Ctx *)cc;
  if (!c || !count) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_resopairs before bsa_sim_init");
  if (!c->simp.resume_nav) return bsa::fail(c, "ASAS bookkeeping is off (resume_nav = 0)");
  if (cap > 0 && (!idx1 || !idx2)) return bsa::fail(c, "NULL resopairs buffer");
  BSA_HIP(c, hipSetDevice(c->device));
  *count = 0;
  if (!c->bk_ready) return 0;
  const int64_t nr = c->last_re - c->last_rb;
  std::vector<unsigned> ptr((size_t)nr + 1);
  BSA_HIP(c, hipMemcpyAsync(ptr.data(), c->bk_rptr.p, (size_t)(nr + 1) * 4, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  const int64_t total = ptr[(size_t)nr];
  *count = total;
  if (total > cap || total == 0) return 0;
  std::vector<unsigned> col((size_t)total);
  BSA_HIP(c, hipMemcpyAsync(col.data(), c->bk_rcol.p, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  // rows in ascending aircraft index (each row's columns are ascending, a
  // deleted intruder's marker last)
  std::vector<unsigned> ord((size_t)nr);
  for (int64_t r = 0; r < nr; ++r) ord[(size_t)r] = (unsigned)r;
  const unsigned *H = c->h2id_h.data() + c->last_rb;
  std::sort(ord.begin(), ord.end(), [&](unsigned a, unsigned b) { return H[a] < H[b]; });
  int64_t at = 0;
  for (unsigned r : ord)
    for (unsigned k = ptr[r]; k < ptr[r + 1]; ++k, ++at) {
      idx1[at] = (int32_t)H[r];
      idx2[at] = (int32_t)col[k];
    }
  return 0;
}

int bsa_sim_cd(bsa_ctx *cc) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_cd before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  for (int attempt = 0;; ++attempt) {
    if (attempt > 6) return bsa::fail(c, "candidate buffer overflow in the CD call (retries exhausted)");
    bsa::BatchBase base;
    bsa::CdOut cd;
    if (bsa::batch_begin(c, false, &base) || bsa::sim_cd(c, false, false, false, &cd)) return -1;
    c->clk.cd_calls++;  // (a CD call outside a step: step_advance counts a step's)
    bsa::BatchCtl ctl{};
    if (bsa::batch_end(c, &ctl)) return -1;
    if (ctl.sticky == 0) break;
    // aborted: nothing persistent was written (the state did not move, so
    // the replicas stay consistent); grow and re-run
    if (bsa::batch_rollback(c, base, ctl)) return -1;
  }
  return 0;
}

int bsa_sim_set_params(bsa_ctx *cc, const bsa_sim_params *p) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!p) return bsa::fail(c, "NULL sim params");
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_params before bsa_sim_init");
  if (bsa::check_params(c, p)) return -1;
  if (p->resume_nav && !c->simp.resume_nav) c->bk_ready = false;  // the bookkeeping starts empty
  c->simp = *p;
  bsa::invalidate(c, bsa::Change::SimParams);
  return 0;
}

int bsa_sim_set_reso_lists(bsa_ctx *cc, const uint8_t *noreso, const uint8_t *resooff) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_reso_lists before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  struct {
    const uint8_t *h;
    bsa::DevBuf *b;
    bool *on;
  } ls[2] = {{noreso, &c->s_noreso, &c->sim_noreso}, {resooff, &c->s_resooff, &c->sim_resooff}};
  std::vector<uint8_t> v[2];  // membership normalised to 0 / 1
  bsa::HomeBatch up(c, true);
  for (int k = 0; k < 2; ++k) {
    *ls[k].on = false;
    if (!ls[k].h) continue;
    v[k].assign(ls[k].h, ls[k].h + c->n);
    for (auto &x : v[k]) x = x ? 1 : 0;
    if (!bsa::ensure(c, *ls[k].b, (size_t)c->n, "NORESO / RESOOFF list") || up.add(ls[k].b->p, v[k].data(), nullptr, 1))
      return -1;
  }
  if (up.run()) return -1;
  for (auto &l : ls) *l.on = l.h != nullptr;
  return 0;
}

int bsa_sim_read_asas(bsa_ctx *cc, bsa_asas_out *o) {
  Ctx *c = (Ctx *)cc;
  if (!c || !o) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_read_asas before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  bsa::HomeBatch down(c, false, c->sim_rb, c->sim_re);
  for (int k = 0; k < 8; ++k) {
    const bsa::AsasArray &a = bsa::kAsasArrays[k];
    if (bsa::ptr_at(o, k) && down.add((c->*a.buf).p, nullptr, bsa::ptr_at(o, k), a.esz)) return -1;
  }
  return down.run();
}

int bsa_sim_set_atmos(bsa_ctx *cc, int on) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_atmos before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  if (on && !c->sim_atmos) {
    if (!bsa::ensure(c, c->s_atm, (size_t)c->n * 24, "atmosphere")) return -1;
    BSA_HIP(c, hipMemsetAsync(c->s_atm.p, 0, (size_t)c->n * 24, c->stream));
  }
  c->sim_atmos = on != 0;
  return 0;
}

int bsa_sim_read_atmos(bsa_ctx *cc, double *p, double *rho, double *temp) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready || !c->sim_atmos) return bsa::fail(c, "bsa_sim_read_atmos: atmosphere outputs are off");
  BSA_HIP(c, hipSetDevice(c->device));
  bsa::HomeBatch down(c, false, c->sim_rb, c->sim_re);
  double *dst[3] = {p, rho, temp};
  for (int k = 0; k < 3; ++k)
    if (dst[k] && down.add((const double *)c->s_atm.p + (size_t)k * c->n, nullptr, dst[k], 8)) return -1;
  return down.run();
}

}  // extern "C"
