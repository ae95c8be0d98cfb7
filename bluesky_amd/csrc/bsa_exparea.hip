// The experiment area, Area.update / Area.create (plugins/area.py:107-175) on the device
// (math: bsa_exparea_math.h; the inside test: bsa_area_wave.h).
//
// k_exparea_update  one update over host-given arrays: accumulators, oldalt, a flag byte per aircraft
// k_sim_exparea     the resident step's stage: the step's last launch (after k_sim_cond); an exit or a
//                   taxi delete raises the batch's stop (bsa_stop.h; bsa_sim.hip: batch_stopped)
// k_xa_records      the log columns of the exited aircraft the device has
// The delete lists in ascending index order (np.where's): flagged_list (bsa_scan.hip).
//
// One lane per aircraft, one wave per workgroup (a polygon's ring passes through the wave's LDS chunk).
// Per aircraft and pass: 48 B of state and 33 B of its own arrays read (+ 8 B thrust), 33 B written.
#include <algorithm>
#include <cmath>

#include "bsa_area_wave.h"
#include "bsa_exparea_math.h"
#include "bsa_stop.h"
#include "bsa_xfer.h"

#pragma clang fp contract(off)

namespace bsa {

constexpr int kXaBlock = 256;  // the records' workgroups (the pass itself: kAreaBlock, one wave)

struct XaArgs {
  int rb, re;  // aircraft (home rows) [rb, re) of the arrays
  const double *gs, *vs, *alt, *lat, *lon;
  const double *thrust;  // or NULL: work stays
  double *d2, *d3, *work, *oldalt;
  uint8_t *flag;
  double dt, swtaxialt;
  int swtaxi, has_shape;
  area::Shape shape;
  const area::Vert *verts;
};

// one aircraft of the pass; every lane of the workgroup reaches the inside test (a polygon's barriers), lanes
// past the end with a NaN point.  Returns: the aircraft is an exit or a taxi delete
__device__ __forceinline__ bool xa_row(const XaArgs &a, area::Vert *ring) {
  const int lane = threadIdx.x;
  const long long h = (long long)a.rb + (long long)blockIdx.x * kAreaBlock + lane;
  const bool live = h < a.re;
  const double nan = __longlong_as_double((long long)kNanBits);
  const double lat = live ? a.lat[h] : nan, lon = live ? a.lon[h] : nan, alt = live ? a.alt[h] : nan;
  bool in = false;
  if (a.has_shape) in = wave_shape_inside(a.shape, a.verts, ring, lane, lat, lon, alt, area::poly_point_ok(lat, lon));
  if (!live) return false;
  exparea::Row r{a.d2[h], a.d3[h], a.work[h], a.oldalt[h]};
  const bool delalt = exparea::advance(r, a.dt, a.gs[h], a.vs[h], alt, a.thrust != nullptr, a.thrust ? a.thrust[h] : 0.0,
                                       a.swtaxi != 0, a.swtaxialt);
  const uint8_t f = exparea::flags_after(a.flag[h], in, delalt);
  a.d2[h] = r.d2;
  a.d3[h] = r.d3;
  if (a.thrust) a.work[h] = r.work;
  if (!a.swtaxi) a.oldalt[h] = r.oldalt;
  a.flag[h] = f;
  return (f & (exparea::kExit | exparea::kTaxi)) != 0;
}

__global__ __launch_bounds__(kAreaBlock) void k_exparea_update(XaArgs a) {
  __shared__ area::Vert ring[kAreaChunk];
  xa_row(a, ring);
}

// Behind the batch's sticky word by stop_runs' rule: k_sim_cond, launched before, may have stopped the batch after
// this step, and so may another workgroup of this launch; the pass of a stopping step still runs in full
__global__ __launch_bounds__(kAreaBlock) void k_sim_exparea(XaArgs a, unsigned long long *__restrict__ word,
                                                             unsigned long long *__restrict__ pend, unsigned tag) {
  __shared__ area::Vert ring[kAreaChunk];
  if (!stop_runs(word, tag)) return;
  const bool flagged = xa_row(a, ring);
  if (__ballot(flagged) && threadIdx.x == 0) stop_raise(word, pend, kStopArea, tag);  // one lane per wave with a delete
}

// the reference's log columns the device has, per exited aircraft (exparea::kRecWords fp64 words each)
struct XaRecSrc {
  const double *ctime, *d2, *d3, *work, *lat, *lon, *alt, *tas, *vs, *hdg;
  const uint8_t *active;
  const double *apalt, *aptas, *apvs, *aptrk, *aalt, *atas, *avs, *atrk;
};
__global__ __launch_bounds__(kXaBlock) void k_xa_records(int m, const int *__restrict__ list,
                                                           const unsigned *__restrict__ id2h, XaRecSrc s,
                                                           double *__restrict__ rec) {
  const int k = blockIdx.x * kXaBlock + threadIdx.x;
  if (k >= m) return;
  const unsigned h = id2h[list[k]];
  double *r = rec + (size_t)k * exparea::kRecWords;
  const double *src[10] = {s.ctime, s.d2, s.d3, s.work, s.lat, s.lon, s.alt, s.tas, s.vs, s.hdg};
  for (int q = 0; q < 10; ++q) r[q] = src[q][h];
  r[10] = s.active[h] ? 1.0 : 0.0;
  const double *tgt[8] = {s.apalt, s.aptas, s.apvs, s.aptrk, s.aalt, s.atas, s.avs, s.atrk};
  for (int q = 0; q < 8; ++q) r[11 + q] = tgt[q][h];
}

static unsigned xa_grid(int64_t n) { return (unsigned)((n + kXaBlock - 1) / kXaBlock); }

static int xa_launch_update(Ctx *c, const XaArgs &a) {
  if (a.re <= a.rb) return 0;
  const unsigned grid = (unsigned)(((int64_t)a.re - a.rb + kAreaBlock - 1) / kAreaBlock);
  hipLaunchKernelGGL(k_exparea_update, dim3(grid), dim3(kAreaBlock), 0, c->stream, a);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

// ---- the resident step's stage
bool exparea_passes_at(const Ctx *c) {
  // Area.update returns at once when swtaxi and not active (area.py:115): nothing is launched, the clock runs on
  return c->sim_exparea && (c->clk.area_ctr + 1) % c->xa_every == 0 && !(c->xa_swtaxi && !c->xa_active);
}

static XaArgs xa_sim_args(Ctx *c) {
  XaArgs a{};
  a.rb = (int)c->sim_rb;
  a.re = (int)c->sim_re;
  a.gs = (const double *)c->own[3].p;
  a.vs = (const double *)c->own[5].p;
  a.alt = (const double *)c->own[4].p;
  a.lat = (const double *)c->own[0].p;
  a.lon = (const double *)c->own[1].p;
  // traf.perf.thrust when the plugin runs: what this step's forces launch wrote (s_fout: cd0 drag thrustratio thrust ...)
  a.thrust = c->sim_forces ? (const double *)c->s_fout.p + 3 * (size_t)c->n : nullptr;
  a.d2 = (double *)c->s_xd2.p;
  a.d3 = (double *)c->s_xd3.p;
  a.work = (double *)c->s_xwork.p;
  a.oldalt = (double *)c->s_xoldalt.p;
  a.flag = (uint8_t *)c->s_xflag.p;
  a.dt = c->xa_dt;
  a.swtaxialt = c->xa_swtaxialt;
  a.swtaxi = c->xa_swtaxi ? 1 : 0;
  a.has_shape = c->xa_has_shape ? 1 : 0;
  a.shape = c->xa_shape;
  a.verts = (const area::Vert *)c->area_verts.p;
  return a;
}

int exparea_sim_launch(Ctx *c, unsigned tag) {
  const XaArgs a = xa_sim_args(c);
  if (a.re <= a.rb) return 0;
  const unsigned grid = (unsigned)(((int64_t)a.re - a.rb + kAreaBlock - 1) / kAreaBlock);
  hipLaunchKernelGGL(k_sim_exparea, dim3(grid), dim3(kAreaBlock), 0, c->stream, a,
                     (unsigned long long *)((char *)c->sim_ctl.p + kSimCtlSticky), (unsigned long long *)((char *)c->sim_ctl.p + kSimCtlPend), tag);
  BSA_HIP(c, hipGetLastError());
  return 0;
}

int exparea_created(Ctx *c, int64_t n, int64_t m, const double *alt) {
  if (!c->sim_exparea || m <= 0) return 0;
  // Area.create (area.py:107-110): create_time = sim.simt, oldalt = traf.alt; the rest False / 0
  std::vector<double> t((size_t)m, c->xa_now);
  BSA_HIP(c, hipMemcpyAsync((double *)c->s_xoldalt.p + n, alt, (size_t)m * 8, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipMemcpyAsync((double *)c->s_xctime.p + n, t.data(), (size_t)m * 8, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));  // (the host vector goes out of scope)
  return 0;
}

void exparea_off(Ctx *c) {
  c->sim_exparea = false, c->stops[kStopArea].pending = false, c->xa_has_shape = false;
  c->clk.area_ctr = 0;
}

}  // namespace bsa

using bsa::Ctx;

extern "C" {

int bsa_exparea_update(bsa_ctx *cc, int64_t n, const double *gs, const double *vs, const double *alt, const double *lat,
                       const double *lon, const double *thrust, double *distance2D, double *distance3D, double *work,
                       double *oldalt, uint8_t *inside, double dt, const bsa_area_shape *shape, int64_t nvert,
                       const double *verts, int active, int swtaxi, double swtaxialt, int32_t *delidx, int64_t *ndel,
                       int32_t *delidxalt, int64_t *ndelalt) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!ndel || !ndelalt) return bsa::fail(c, "bsa_exparea_update: NULL count");
  *ndel = *ndelalt = 0;
  if (n < 0 || n > 0x7fffffff - 64) return bsa::fail(c, "bsa_exparea_update: bad n");
  std::vector<bsa::area::Shape> tab;
  if (bsa::area_pack(c, "bsa_exparea_update", shape ? 1 : 0, shape, shape ? nvert : 0, verts, &tab)) return -1;
  if (swtaxi && !active) return 0;  // area.py:115
  if (n == 0) return 0;             // nothing is launched
  if (!gs || !vs || !alt || !lat || !lon || !distance2D || !distance3D || !work || !oldalt || !inside || !delidx ||
      !delidxalt)
    return bsa::fail(c, "bsa_exparea_update: NULL array");
  BSA_HIP(c, hipSetDevice(c->device));
  // stage: gs vs alt lat lon thrust d2 d3 work oldalt (fp64) | vertices | flags | the compaction's words
  const size_t N = (size_t)n, N8 = (N + 7) / 8 * 8, vb = shape ? (size_t)nvert * 16 : 0;
  const size_t bytes = 10 * N * 8 + vb + N8 + bsa::flagged_ws_words(n) * 4 + 16;
  if (!bsa::ensure(c, c->xa_stage, bytes, "experiment area arrays")) return -1;
  double *d = (double *)c->xa_stage.p;
  bsa::area::Vert *dv = (bsa::area::Vert *)(d + 10 * N);
  uint8_t *d_flag = (uint8_t *)dv + vb;
  unsigned *d_ws = (unsigned *)(d_flag + N8);
  hipStream_t s = c->stream;
  std::vector<uint8_t> f(inside, inside + n);
  for (auto &x : f) x = x ? bsa::exparea::kInside : 0;
  const double *in[10] = {gs, vs, alt, lat, lon, thrust, distance2D, distance3D, work, oldalt};
  for (int q = 0; q < 10; ++q)
    if (in[q]) BSA_HIP(c, hipMemcpyAsync(d + (size_t)q * N, in[q], N * 8, hipMemcpyHostToDevice, s));
  if (vb) BSA_HIP(c, hipMemcpyAsync(dv, verts, vb, hipMemcpyHostToDevice, s));
  BSA_HIP(c, hipMemcpyAsync(d_flag, f.data(), N, hipMemcpyHostToDevice, s));
  bsa::XaArgs a{};
  a.rb = 0, a.re = (int)n;
  a.gs = d, a.vs = d + N, a.alt = d + 2 * N, a.lat = d + 3 * N, a.lon = d + 4 * N;
  a.thrust = thrust ? d + 5 * N : nullptr;
  a.d2 = d + 6 * N, a.d3 = d + 7 * N, a.work = d + 8 * N, a.oldalt = d + 9 * N;
  a.flag = d_flag;
  a.dt = dt, a.swtaxialt = swtaxialt, a.swtaxi = swtaxi ? 1 : 0;
  a.has_shape = shape ? 1 : 0;
  if (shape) a.shape = tab[0];
  a.verts = dv;
  if (bsa::xa_launch_update(c, a)) return -1;
  std::vector<int32_t> l1, l2;
  if (bsa::flagged_list(c, n, d_flag, nullptr, bsa::exparea::kExit, d_ws, &l1, nullptr) ||
      bsa::flagged_list(c, n, d_flag, nullptr, bsa::exparea::kTaxi, d_ws, &l2, nullptr))
    return -1;
  double *out[4] = {distance2D, distance3D, work, oldalt};
  for (int q = 0; q < 4; ++q) BSA_HIP(c, hipMemcpyAsync(out[q], d + (size_t)(6 + q) * N, N * 8, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipMemcpyAsync(f.data(), d_flag, N, hipMemcpyDeviceToHost, s));
  BSA_HIP(c, hipStreamSynchronize(s));
  for (int64_t k = 0; k < n; ++k) inside[k] = (f[(size_t)k] & bsa::exparea::kInside) ? 1 : 0;
  std::copy(l1.begin(), l1.end(), delidx);
  std::copy(l2.begin(), l2.end(), delidxalt);
  *ndel = (int64_t)l1.size();
  *ndelalt = (int64_t)l2.size();
  return 0;
}

int bsa_sim_set_exparea(bsa_ctx *cc, int on, int32_t shape_idx, double dt, int64_t every, double simt, int active,
                        int swtaxi, double swtaxialt) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_exparea before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  if (!on) {
    bsa::exparea_off(c);
    return 0;
  }
  if (c->nranks > 1)
    return bsa::fail(c, "bsa_sim_set_exparea on %d ranks: an exit would have to stop every rank's batch at the same "
                        "step, and that agreement between the ranks is not built (one rank only)", c->nranks);
  if (every < 1) return bsa::fail(c, "bsa_sim_set_exparea: every must be >= 1");
  if (shape_idx < -1 || (shape_idx >= 0 && (size_t)shape_idx >= c->area_tab.size()))
    return bsa::fail(c, "bsa_sim_set_exparea: shape %d of %zu (bsa_sim_set_areas)", shape_idx, c->area_tab.size());
  const size_t n = (size_t)c->n;
  if (!c->sim_exparea) {  // enabling: Area's arrays as after Area.create for every aircraft at `simt`
    bsa::DevBuf *f8[5] = {&c->s_xd2, &c->s_xd3, &c->s_xwork, &c->s_xoldalt, &c->s_xctime};
    for (bsa::DevBuf *b : f8)
      if (!bsa::ensure(c, *b, n * 8, "experiment area arrays")) return -1;
    if (!bsa::ensure(c, c->s_xflag, n, "experiment area flags")) return -1;
    hipStream_t s = c->stream;
    BSA_HIP(c, hipMemsetAsync(c->s_xd2.p, 0, n * 8, s));
    BSA_HIP(c, hipMemsetAsync(c->s_xd3.p, 0, n * 8, s));
    BSA_HIP(c, hipMemsetAsync(c->s_xwork.p, 0, n * 8, s));
    BSA_HIP(c, hipMemsetAsync(c->s_xflag.p, 0, n, s));  // inside all False: seen inside once before an exit (area.py:100)
    BSA_HIP(c, hipMemcpyAsync(c->s_xoldalt.p, c->own[4].p, n * 8, hipMemcpyDeviceToDevice, s));
    std::vector<double> t(n, simt);
    BSA_HIP(c, hipMemcpyAsync(c->s_xctime.p, t.data(), n * 8, hipMemcpyHostToDevice, s));
    BSA_HIP(c, hipStreamSynchronize(s));
    c->clk.area_ctr = 0;
    c->stops[bsa::kStopArea].pending = false;
    c->xa_now = simt;
  }
  c->xa_has_shape = shape_idx >= 0;
  if (c->xa_has_shape) c->xa_shape = c->area_tab[(size_t)shape_idx];
  c->xa_dt = dt;
  c->xa_every = every;
  c->xa_active = active != 0;
  c->xa_swtaxi = swtaxi != 0;
  c->xa_swtaxialt = swtaxialt;
  c->sim_exparea = true;
  return 0;
}

int bsa_sim_exparea_simt(bsa_ctx *cc, double simt) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  c->xa_now = simt;
  return 0;
}

int bsa_sim_exparea_poll(bsa_ctx *cc, int64_t cap, int32_t *delidx, int64_t *ndel, int32_t *delidxalt, int64_t *ndelalt,
                         double *records, int64_t *step) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_exparea_poll before bsa_sim_init");
  if (!ndel || !ndelalt) return bsa::fail(c, "bsa_sim_exparea_poll: NULL count");
  *ndel = *ndelalt = 0;
  bsa::StopSide &stop = c->stops[bsa::kStopArea];
  if (step) *step = stop.step;
  if (!c->sim_exparea || !stop.pending) return 0;
  BSA_HIP(c, hipSetDevice(c->device));
  const int64_t n = c->n;
  if (!bsa::ensure(c, c->xa_ws, bsa::flagged_ws_words(n) * 4, "delete lists")) return -1;
  const uint8_t *flag = (const uint8_t *)c->s_xflag.p;
  const unsigned *id2h = (const unsigned *)c->id2h.p;
  unsigned *ws = (unsigned *)c->xa_ws.p;
  std::vector<int32_t> l1, l2;
  const int *exits = nullptr;
  // (the taxi list first: the exit list then stays in the scratch for the records' gather)
  if (bsa::flagged_list(c, n, flag, id2h, bsa::exparea::kTaxi, ws, &l2, nullptr) ||
      bsa::flagged_list(c, n, flag, id2h, bsa::exparea::kExit, ws, &l1, &exits))
    return -1;
  *ndel = (int64_t)l1.size();
  *ndelalt = (int64_t)l2.size();
  if (*ndel > cap || *ndelalt > cap) return 0;  // (nothing consumed: ask again with room for both)
  if ((*ndel > 0 && (!delidx || !records)) || (*ndelalt > 0 && !delidxalt))
    return bsa::fail(c, "bsa_sim_exparea_poll: NULL buffer");
  if (!l1.empty()) {
    const size_t rb = l1.size() * bsa::exparea::kRecWords * 8;
    if (!bsa::ensure(c, c->xa_rec, rb, "exit records")) return -1;
    const bsa::XaRecSrc s{(const double *)c->s_xctime.p, (const double *)c->s_xd2.p,   (const double *)c->s_xd3.p,
                          (const double *)c->s_xwork.p,  (const double *)c->own[0].p,  (const double *)c->own[1].p,
                          (const double *)c->own[4].p,   (const double *)c->s_tas.p,   (const double *)c->own[5].p,
                          (const double *)c->s_hdg.p,    (const uint8_t *)c->s_active.p, (const double *)c->s_apalt.p,
                          (const double *)c->s_aptas.p,  (const double *)c->s_apvs.p,  (const double *)c->s_aptrk.p,
                          (const double *)c->s_aalt.p,   (const double *)c->s_atas.p,  (const double *)c->s_avs.p,
                          (const double *)c->s_atrk.p};
    hipLaunchKernelGGL(bsa::k_xa_records, dim3(bsa::xa_grid((int64_t)l1.size())), dim3(bsa::kXaBlock), 0, c->stream,
                       (int)l1.size(), exits, id2h, s, (double *)c->xa_rec.p);
    BSA_HIP(c, hipGetLastError());
    BSA_HIP(c, hipMemcpyAsync(records, c->xa_rec.p, rb, hipMemcpyDeviceToHost, c->stream));
    BSA_HIP(c, hipStreamSynchronize(c->stream));
  }
  std::copy(l1.begin(), l1.end(), delidx);
  std::copy(l2.begin(), l2.end(), delidxalt);
  stop.pending = false;
  return 0;
}

int bsa_sim_read_exparea(bsa_ctx *cc, double *distance2D, double *distance3D, double *work, double *oldalt,
                         double *create_time, uint8_t *inside) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready || !c->sim_exparea) return bsa::fail(c, "bsa_sim_read_exparea: the experiment area is off");
  BSA_HIP(c, hipSetDevice(c->device));
  bsa::HomeBatch down(c, false);
  double *dst[5] = {distance2D, distance3D, work, oldalt, create_time};
  bsa::DevBuf *src[5] = {&c->s_xd2, &c->s_xd3, &c->s_xwork, &c->s_xoldalt, &c->s_xctime};
  for (int k = 0; k < 5; ++k)
    if (dst[k] && down.add(src[k]->p, nullptr, dst[k], 8)) return -1;
  if (inside && down.add(c->s_xflag.p, nullptr, inside, 1)) return -1;
  if (down.run()) return -1;
  for (int64_t k = 0; inside && k < c->n; ++k) inside[k] &= bsa::exparea::kInside;
  return 0;
}

}  // extern "C"
