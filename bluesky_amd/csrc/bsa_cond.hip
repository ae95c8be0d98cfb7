// Conditional commands, Condition.update (bluesky/traffic/conditional.py:25-49)
// on the device (math: bsa_cond_math.h).
//
// k_cond_update   one update over host-given arrays: lastdif, a fired flag per condition
// k_sim_cond      the resident step's stage: the step's first stopping launch; a firing
//                 raises the batch's stop (bsa_stop.h; bsa_sim.hip: batch_stopped)
// The fired indices in ascending order (np.where's): flagged_list (bsa_scan.hip).
//
// One lane per condition, gathered loads of the aircraft's values: per condition 24 B of
// the table read, 8-9 B written, and 8 (standalone: 16) B gathered per aircraft array.
#include <algorithm>
#include <cmath>

#include "bsa_cond_math.h"
#include "bsa_kin_math.h"
#include "bsa_stop.h"

#pragma clang fp contract(off)

namespace bsa {

constexpr int kCondBlock = 256;
// the flag byte of a condition of the resident table; "fired" is flagged_list's mask 1 (a dead row has that bit clear)
constexpr uint8_t kCondLive = 0, kCondFired = 1, kCondDead = 2;

__global__ __launch_bounds__(kCondBlock) void k_cond_update(int ncond, const int *__restrict__ idx,
                                                              const int *__restrict__ type,
                                                              const double *__restrict__ target,
                                                              double *__restrict__ lastdif,
                                                              const double *__restrict__ alt,
                                                              const double *__restrict__ cas,
                                                              uint8_t *__restrict__ flag) {
  const int i = blockIdx.x * kCondBlock + threadIdx.x;
  if (i >= ncond) return;
  const int a = idx[i];
  const cond::Eval e = cond::eval(type[i], target[i], lastdif[i], alt[a], cas[a]);
  lastdif[i] = e.actdif;
  flag[i] = e.fired ? kCondFired : kCondLive;
}

// Behind the batch's sticky word by stop_runs' rule: no other stage can have raised a stop
// with this step's tag before this launch, so only another wave of this launch lets it run
// behind a stop.  Table rows are aircraft indices; the state is in home order (id2h).  traf.cas at
// cond.update() is vtas2cas(new tas, the altitude before UpdatePosition) (traffic.py:434
// against :480), untouched by Woosh; alt is what Woosh left
__global__ __launch_bounds__(kCondBlock) void k_sim_cond(int ncond, const int *__restrict__ idx,
                                                           const int *__restrict__ type,
                                                           const double *__restrict__ target,
                                                           double *__restrict__ lastdif, uint8_t *__restrict__ flag,
                                                           const unsigned *__restrict__ id2h,
                                                           const double *__restrict__ alt,
                                                           const double *__restrict__ altprev,
                                                           const double *__restrict__ tas,
                                                           unsigned long long *__restrict__ word,
                                                           unsigned long long *__restrict__ pend, unsigned tag) {
  if (!stop_runs(word, tag)) return;
  const int i = blockIdx.x * kCondBlock + threadIdx.x;
  bool fired = false;
  if (i < ncond) {
    const uint8_t f = flag[i];
    if (f == kCondFired) {
      flag[i] = kCondDead;  // fired at an earlier stop nobody polled: delcondition'ed, no longer "the last stop's"
    } else if (f == kCondLive) {
      const unsigned h = id2h[idx[i]];
      const cond::Eval e = cond::eval(type[i], target[i], lastdif[i], alt[h], kin::vtas2cas(tas[h], altprev[h]));
      lastdif[i] = e.actdif;
      if (e.fired) flag[i] = kCondFired;
      fired = e.fired;
    }
  }
  if (__ballot(fired) && (threadIdx.x & 63) == 0) stop_raise(word, pend, kStopCond, tag);  // one lane per wave
}

static unsigned cond_grid(int64_t n) { return (unsigned)((n + kCondBlock - 1) / kCondBlock); }

// every index the kernels gather with, and every type, on the host
static int cond_check(Ctx *c, const char *who, int64_t ncond, const int32_t *idx, const int32_t *type, int64_t n) {
  if (ncond < 0 || ncond > 0x7fffffff - 64) return fail(c, "%s: bad ncond", who);
  if (ncond == 0) return 0;
  if (!idx || !type) return fail(c, "%s: NULL condition array", who);
  for (int64_t i = 0; i < ncond; ++i) {
    if (idx[i] < 0 || idx[i] >= n)
      return fail(c, "%s: condition %lld: aircraft index %d outside [0, %lld)", who, (long long)i, idx[i], (long long)n);
    if (type[i] != cond::kAltType && type[i] != cond::kSpdType)
      return fail(c, "%s: condition %lld: type %d is neither 0 (altitude) nor 1 (speed)", who, (long long)i, type[i]);
  }
  return 0;
}

// ---- the resident table: Ctx::cond_* (host mirror of idx / type / target, every row of the device table
// -- dead ones until the next compaction), lastdif and the flags on the device
struct CondTable {
  std::vector<int32_t> idx, type;
  std::vector<double> target, lastdif;
};

static int cond_push(Ctx *c, const CondTable &t) {
  const size_t m = t.idx.size();
  c->cond_idx_h = t.idx, c->cond_type_h = t.type, c->cond_tgt_h = t.target;
  c->sim_cond = m > 0;
  if (!m) return 0;
  if (!ensure(c, c->cond_idx, m * 4, "condition aircraft") || !ensure(c, c->cond_type, m * 4, "condition types") ||
      !ensure(c, c->cond_tgt, m * 8, "condition targets") || !ensure(c, c->cond_last, m * 8, "condition lastdif") ||
      !ensure(c, c->cond_flag, m, "condition flags") || !ensure(c, c->cond_ws, flagged_ws_words((int64_t)m) * 4, "fired list"))
    return -1;
  BSA_HIP(c, hipMemcpyAsync(c->cond_idx.p, t.idx.data(), m * 4, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipMemcpyAsync(c->cond_type.p, t.type.data(), m * 4, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipMemcpyAsync(c->cond_tgt.p, t.target.data(), m * 8, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipMemcpyAsync(c->cond_last.p, t.lastdif.data(), m * 8, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipMemsetAsync(c->cond_flag.p, 0, m, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));  // (the host vectors go out of scope)
  return 0;
}

// the live rows of the device table (delcondition's result: order kept)
static int cond_pull(Ctx *c, CondTable *t) {
  const size_t m = c->cond_idx_h.size();
  *t = CondTable{};
  if (!m) return 0;
  std::vector<double> last(m);
  std::vector<uint8_t> flag(m);
  BSA_HIP(c, hipMemcpyAsync(last.data(), c->cond_last.p, m * 8, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipMemcpyAsync(flag.data(), c->cond_flag.p, m, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < m; ++i) {
    if (flag[i] != kCondLive) continue;
    t->idx.push_back(c->cond_idx_h[i]), t->type.push_back(c->cond_type_h[i]);
    t->target.push_back(c->cond_tgt_h[i]), t->lastdif.push_back(last[i]);
  }
  return 0;
}

int cond_sim_launch(Ctx *c, unsigned tag) {
  const int64_t m = (int64_t)c->cond_idx_h.size();
  if (m <= 0) return 0;
  hipLaunchKernelGGL(k_sim_cond, dim3(cond_grid(m)), dim3(kCondBlock), 0, c->stream, (int)m, (const int *)c->cond_idx.p,
                     (const int *)c->cond_type.p, (const double *)c->cond_tgt.p, (double *)c->cond_last.p,
                     (uint8_t *)c->cond_flag.p, (const unsigned *)c->id2h.p, (const double *)c->own[4].p,
                     (const double *)c->s_altprev.p, (const double *)c->s_tas.p,
                     (unsigned long long *)((char *)c->sim_ctl.p + kSimCtlSticky),
                     (unsigned long long *)((char *)c->sim_ctl.p + kSimCtlPend), tag);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

void cond_off(Ctx *c) {
  c->sim_cond = false, c->stops[kStopCond].pending = false;
  c->cond_idx_h.clear(), c->cond_type_h.clear(), c->cond_tgt_h.clear();
}

// Condition.delac (conditional.py:108-128) for the aircraft of a delete, one deloneac after another
// in the order given (Traffic.delete sorts an index array first, traffic.py:370-377): each removes
// the conditions at that index and shifts the indices above it down -- so in a multiple delete the
// later indices meet a table already shifted, as in the reference.  On a host copy, uploaded again
int cond_note_deleted(Ctx *c, const std::vector<int64_t> &d) {
  if (!c->sim_cond) return 0;
  CondTable t, u;
  if (cond_pull(c, &t)) return -1;
  for (int64_t ac : d) {
    u = CondTable{};
    for (size_t i = 0; i < t.idx.size(); ++i) {
      if (t.idx[i] == ac) continue;
      u.idx.push_back(t.idx[i] <= ac ? t.idx[i] : t.idx[i] - 1), u.type.push_back(t.type[i]);
      u.target.push_back(t.target[i]), u.lastdif.push_back(t.lastdif[i]);
    }
    t = u;
  }
  // (an index the shifted deletes left past the new n would be gathered out of bounds: such a condition
  // points at no aircraft in the reference either -- it raises there; dropped here)
  const int64_t nn = c->n - (int64_t)d.size();
  u = CondTable{};
  for (size_t i = 0; i < t.idx.size(); ++i) {
    if (t.idx[i] >= nn) continue;
    u.idx.push_back(t.idx[i]), u.type.push_back(t.type[i]), u.target.push_back(t.target[i]);
    u.lastdif.push_back(t.lastdif[i]);
  }
  c->stops[kStopCond].pending = false;  // (the fired rows of an unpolled stop are gone with the compaction)
  return cond_push(c, u);
}

}  // namespace bsa

using bsa::Ctx;

extern "C" {

int bsa_cond_update(bsa_ctx *cc, int64_t ncond, const int32_t *idx, const int32_t *type, const double *target,
                    double *lastdif, int64_t n, const double *alt, const double *cas, int32_t *fired,
                    int64_t *count) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!count) return bsa::fail(c, "bsa_cond_update: NULL count");
  *count = 0;
  if (n < 0 || n > 0x7fffffff) return bsa::fail(c, "bsa_cond_update: bad n");
  if (bsa::cond_check(c, "bsa_cond_update", ncond, idx, type, n)) return -1;
  if (ncond == 0) return 0;  // Condition.update returns at once (conditional.py:26): nothing is launched
  if (!target || !lastdif || !alt || !cas || !fired) return bsa::fail(c, "bsa_cond_update: NULL array");
  BSA_HIP(c, hipSetDevice(c->device));
  // stage: idx type (int32) | target lastdif alt cas (fp64) | flags | the compaction's words
  const size_t M = (size_t)ncond, N = (size_t)n, M8 = (M + 7) / 8 * 8;
  const size_t bytes = 2 * M8 * 4 + 2 * M * 8 + 2 * N * 8 + M8 + bsa::flagged_ws_words(ncond) * 4;
  if (!bsa::ensure(c, c->cond_stage, bytes, "condition arrays")) return -1;
  char *p = (char *)c->cond_stage.p;
  int *d_idx = (int *)p, *d_type = (int *)(p + M8 * 4);
  double *d_tgt = (double *)(p + 2 * M8 * 4), *d_last = d_tgt + M, *d_alt = d_last + M, *d_cas = d_alt + N;
  uint8_t *d_flag = (uint8_t *)(d_cas + N);
  unsigned *d_ws = (unsigned *)(d_flag + M8);
  hipStream_t s = c->stream;
  BSA_HIP(c, hipMemcpyAsync(d_idx, idx, M * 4, hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemcpyAsync(d_type, type, M * 4, hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemcpyAsync(d_tgt, target, M * 8, hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemcpyAsync(d_last, lastdif, M * 8, hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemcpyAsync(d_alt, alt, N * 8, hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemcpyAsync(d_cas, cas, N * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(bsa::k_cond_update, dim3(bsa::cond_grid(ncond)), dim3(bsa::kCondBlock), 0, s, (int)ncond,
                     (const int *)d_idx, (const int *)d_type, (const double *)d_tgt, d_last, (const double *)d_alt,
                     (const double *)d_cas, d_flag);
  BSA_HIP(c, hipGetLastError());
  std::vector<int32_t> list;
  if (bsa::flagged_list(c, ncond, d_flag, nullptr, bsa::kCondFired, d_ws, &list, nullptr)) return -1;
  BSA_HIP(c, hipMemcpy(lastdif, d_last, M * 8, hipMemcpyDeviceToHost));
  std::copy(list.begin(), list.end(), fired);
  *count = (int64_t)list.size();
  return 0;
}

int bsa_sim_set_conditions(bsa_ctx *cc, int64_t ncond, const int32_t *idx, const int32_t *type, const double *target,
                           const double *lastdif) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_conditions before bsa_sim_init");
  if (c->nranks > 1)
    return bsa::fail(c, "bsa_sim_set_conditions on %d ranks: a firing would have to stop every rank's batch at the same "
                        "step, and that agreement between the ranks is not built (one rank only)", c->nranks);
  if (bsa::cond_check(c, "bsa_sim_set_conditions", ncond, idx, type, c->n)) return -1;
  if (ncond > 0 && (!target || !lastdif)) return bsa::fail(c, "bsa_sim_set_conditions: NULL condition array");
  BSA_HIP(c, hipSetDevice(c->device));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  bsa::CondTable t;
  if (ncond > 0) {
    t.idx.assign(idx, idx + ncond), t.type.assign(type, type + ncond);
    t.target.assign(target, target + ncond), t.lastdif.assign(lastdif, lastdif + ncond);
  }
  c->stops[bsa::kStopCond].pending = false;
  return bsa::cond_push(c, t);
}

int bsa_sim_cond_poll(bsa_ctx *cc, int64_t cap, int32_t *fired, int64_t *count, int64_t *step) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_cond_poll before bsa_sim_init");
  if (!count) return bsa::fail(c, "bsa_sim_cond_poll: NULL count");
  *count = 0;
  bsa::StopSide &stop = c->stops[bsa::kStopCond];
  if (step) *step = stop.step;
  if (!c->sim_cond || !stop.pending) return 0;
  BSA_HIP(c, hipSetDevice(c->device));
  const int64_t m = (int64_t)c->cond_idx_h.size();
  std::vector<int32_t> list;
  if (bsa::flagged_list(c, m, (const uint8_t *)c->cond_flag.p, nullptr, bsa::kCondFired, (unsigned *)c->cond_ws.p, &list,
                        nullptr))
    return -1;
  *count = (int64_t)list.size();
  if (*count > cap) return 0;  // (nothing consumed: ask again with room for `count`)
  if (*count > 0 && !fired) return bsa::fail(c, "bsa_sim_cond_poll: NULL buffer");
  std::copy(list.begin(), list.end(), fired);
  // delcondition (conditional.py:75-98): the dead rows leave the table, the order of the rest stays
  bsa::CondTable t;
  if (bsa::cond_pull(c, &t)) return -1;
  stop.pending = false;
  return bsa::cond_push(c, t);
}

int bsa_sim_read_conditions(bsa_ctx *cc, int64_t cap, int32_t *idx, int32_t *type, double *target, double *lastdif,
                            int64_t *count) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_read_conditions before bsa_sim_init");
  if (!count) return bsa::fail(c, "bsa_sim_read_conditions: NULL count");
  *count = 0;
  if (!c->sim_cond) return 0;
  BSA_HIP(c, hipSetDevice(c->device));
  bsa::CondTable t;
  if (bsa::cond_pull(c, &t)) return -1;
  *count = (int64_t)t.idx.size();
  if (*count > cap) return 0;
  if (idx) std::copy(t.idx.begin(), t.idx.end(), idx);
  if (type) std::copy(t.type.begin(), t.type.end(), type);
  if (target) std::copy(t.target.begin(), t.target.end(), target);
  if (lastdif) std::copy(t.lastdif.begin(), t.lastdif.end(), lastdif);
  return 0;
}

}  // extern "C"
