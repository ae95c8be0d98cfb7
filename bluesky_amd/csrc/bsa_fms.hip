// Autopilot LNAV / VNAV guidance and waypoint switching (Autopilot.update,
// autopilot.py:59-203) on the device: the standalone kernel over host arrays
// (bsa_fms_update) and the resident step's own launch (k_sim_fms,
// bsa_sim_set_fms), one lane per aircraft, one-wave workgroups like K4'.  The
// per-aircraft arrays are SoA; the route table (8 doubles = 64 B per
// waypoint) stays in HBM and only a lane that switches waypoint reads its row.
#include "bsa_fms_math.h"
#include "bsa_xfer.h"

#pragma clang fp contract(off)

namespace bsa {

__device__ __forceinline__ fms::Lane fms_load(const FmsArrays &a, int k) {
  fms::Lane L;
  L.lat = a.tr[0][k], L.lon = a.tr[1][k], L.alt = a.tr[2][k], L.tas = a.tr[3][k];
  L.gs = a.tr[4][k], L.trk = a.tr[5][k], L.ax = a.tr[6][k], L.bank = a.tr[7][k];
  L.wlat = a.st[0][k], L.wlon = a.st[1][k], L.nextaltco = a.st[2][k], L.xtoalt = a.st[3][k];
  L.spd = a.st[4][k], L.vs = a.st[5][k], L.turndist = a.st[6][k], L.flyby = a.st[7][k];
  L.next_qdr = a.st[8][k], L.dist2vs = a.st[9][k], L.vnavvs = a.st[10][k], L.swvnavvs = a.st[11][k];
  L.selspd = a.st[12][k], L.selvs = a.st[13][k], L.apvsdef = a.st[14][k];
  L.swlnav = a.fl[0][k] != 0, L.swvnav = a.fl[1][k] != 0, L.abco = a.fl[2][k] != 0, L.belco = a.fl[3][k] != 0;
  L.ap_trk = a.tg[0][k], L.ap_alt = a.tg[2][k], L.ap_vs = a.tg[3][k], L.selalt = a.tg[4][k];
  L.iactwp = a.iactwp[k];
  return L;
}

__device__ __forceinline__ void fms_store(const FmsArrays &a, int k, const fms::Lane &L) {
  a.st[0][k] = L.wlat, a.st[1][k] = L.wlon, a.st[2][k] = L.nextaltco, a.st[3][k] = L.xtoalt;
  a.st[4][k] = L.spd, a.st[5][k] = L.vs, a.st[6][k] = L.turndist, a.st[7][k] = L.flyby;
  a.st[8][k] = L.next_qdr, a.st[9][k] = L.dist2vs, a.st[10][k] = L.vnavvs, a.st[11][k] = L.swvnavvs;
  a.st[12][k] = L.selspd;
  a.fl[0][k] = L.swlnav ? 1 : 0, a.fl[1][k] = L.swvnav ? 1 : 0;
  a.tg[0][k] = L.ap_trk, a.tg[2][k] = L.ap_alt, a.tg[3][k] = L.ap_vs, a.tg[4][k] = L.selalt;
  a.iactwp[k] = L.iactwp;
}

// One full Autopilot.update call (forced tick) for aircraft [0, n)
__global__ __launch_bounds__(64) void k_fms_update(int n, FmsArrays a) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  fms::Lane L = fms_load(a, k);
  fms::tick(L, a.rows, a.rt_off[k], a.rt_n[k]);
  fms_store(a, k, L);
  a.tg[1][k] = fms::vcasormach2tas(L.selspd, L.alt);   // ap.tas, autopilot.py:203
}

// The undo set of a ticking launch: what the tick may overwrite, as it was at
// the step's start
struct FmsUndo {
  double *r;    // 17 x n: st[0 .. 12], ap_trk, ap_alt, ap_vs, selalt
  uint8_t *f;   // 2 x n: swlnav, swvnav
  int *iactwp;  // n
  int n;
};

// The resident step's launch, first on the step's stream: rows [rb, re) of the
// PRE-step state (ap.update is the first call of Traffic.update,
// traffic.py:395).  TICK: the FMS part, after the lane has copied what it may
// overwrite into the undo set; always ap.tas (autopilot.py:203).  Behind the
// batch's sticky abort word it changes nothing.
template <bool TICK>
__global__ __launch_bounds__(64) void k_sim_fms(int rb, int re, FmsArrays a, FmsUndo u,
                                                const unsigned *__restrict__ sticky) {
  if (*sticky != 0u) return;
  const int k = rb + blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= re) return;
  if (TICK) {
    fms::Lane L = fms_load(a, k);
    const size_t n = (size_t)u.n;
    const double keep[kFmsUndoReals] = {L.wlat, L.wlon, L.nextaltco, L.xtoalt, L.spd, L.vs, L.turndist, L.flyby,
                                        L.next_qdr, L.dist2vs, L.vnavvs, L.swvnavvs, L.selspd, L.ap_trk, L.ap_alt,
                                        L.ap_vs, L.selalt};  // from the lane's own loads: st[0 .. 12], the targets
#pragma unroll
    for (int q = 0; q < kFmsUndoReals; ++q) u.r[q * n + k] = keep[q];
    u.f[k] = L.swlnav ? 1 : 0, u.f[n + k] = L.swvnav ? 1 : 0;
    u.iactwp[k] = L.iactwp;
    fms::tick(L, a.rows, a.rt_off[k], a.rt_n[k]);
    fms_store(a, k, L);
    a.tg[1][k] = fms::vcasormach2tas(L.selspd, L.alt);
  } else {
    a.tg[1][k] = fms::vcasormach2tas(a.st[12][k], a.tr[2][k]);
  }
}

FmsArrays fms_sim_arrays(Ctx *c) {
  const size_t n = (size_t)c->n;
  FmsArrays a;
  const void *tr[8] = {c->own[0].p, c->own[1].p, c->own[4].p, c->s_tas.p, c->own[3].p, c->own[2].p, c->s_ax.p,
                       c->s_bank.p};  // lat lon alt tas gs trk ax bank
  for (int q = 0; q < 8; ++q) a.tr[q] = (const double *)tr[q];
  for (int q = 0; q < kFmsReals; ++q) a.st[q] = (double *)c->s_fmsr.p + q * n;
  for (int q = 0; q < 4; ++q) a.fl[q] = (uint8_t *)c->s_fmsf.p + q * n;
  void *tg[5] = {c->s_aptrk.p, c->s_aptas.p, c->s_apalt.p, c->s_apvs.p, c->s_selalt.p};
  for (int q = 0; q < 5; ++q) a.tg[q] = (double *)tg[q];
  a.iactwp = (int *)c->s_fmsi.p;
  a.rt_off = (const int *)c->s_fmsi.p + n;
  a.rt_n = (const int *)c->s_fmsi.p + 2 * n;
  a.rows = (const double *)c->s_fmsrows.p;
  return a;
}

int fms_sim_launch(Ctx *c, bool tick) {
  const int64_t rb = c->sim_rb, re = c->sim_re;
  if (re <= rb) return 0;
  const FmsArrays a = fms_sim_arrays(c);
  const FmsUndo u{(double *)c->s_fmsur.p, (uint8_t *)c->s_fmsuf.p, (int *)c->s_fmsui.p, (int)c->n};
  const auto K = tick ? k_sim_fms<true> : k_sim_fms<false>;
  hipLaunchKernelGGL(K, dim3((unsigned)((re - rb + 63) / 64)), dim3(64), 0, c->stream, (int)rb, (int)re, a, u,
                     (const unsigned *)((const char *)c->sim_ctl.p + kSimCtlSticky));
  BSA_HIP(c, hipGetLastError());
  return 0;
}

int fms_sim_restore(Ctx *c) {
  const int64_t rb = c->sim_rb, re = c->sim_re;
  if (re <= rb) return 0;
  const size_t n = (size_t)c->n, m = (size_t)(re - rb);
  const FmsArrays a = fms_sim_arrays(c);
  const double *ur = (const double *)c->s_fmsur.p;
  for (int q = 0; q < kFmsMutable; ++q)
    BSA_HIP(c, hipMemcpyAsync(a.st[q] + rb, ur + q * n + rb, m * 8, hipMemcpyDeviceToDevice, c->stream));
  const int tg[4] = {0, 2, 3, 4};
  for (int q = 0; q < 4; ++q)
    BSA_HIP(c, hipMemcpyAsync(a.tg[tg[q]] + rb, ur + (kFmsMutable + q) * n + rb, m * 8, hipMemcpyDeviceToDevice, c->stream));
  for (int q = 0; q < 2; ++q)
    BSA_HIP(c, hipMemcpyAsync(a.fl[q] + rb, (const uint8_t *)c->s_fmsuf.p + q * n + rb, m, hipMemcpyDeviceToDevice,
                              c->stream));
  BSA_HIP(c, hipMemcpyAsync(a.iactwp + rb, (const int *)c->s_fmsui.p + rb, m * 4, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

// ---- waypoint recovery: findact + direct once per resopair
// that ResumeNav dropped for the aircraft.  The lane loads and stores only what
// fms::fms_recover reads and writes (tr[6], traf.ax, is not read).
__device__ __forceinline__ void recover_lane(const FmsArrays &a, int k, int count) {
  const int nwp = a.rt_n[k];
  if (nwp <= 0) return;   // findact: -1, nothing is touched
  fms::Lane L;
  L.lat = a.tr[0][k], L.lon = a.tr[1][k], L.alt = a.tr[2][k], L.tas = a.tr[3][k];
  L.gs = a.tr[4][k], L.trk = a.tr[5][k], L.bank = a.tr[7][k];
  L.wlat = a.st[0][k], L.wlon = a.st[1][k], L.nextaltco = a.st[2][k], L.xtoalt = a.st[3][k];
  L.spd = a.st[4][k], L.vs = a.st[5][k], L.turndist = a.st[6][k], L.flyby = a.st[7][k];
  L.dist2vs = a.st[9][k], L.selspd = a.st[12][k];
  L.swlnav = a.fl[0][k] != 0, L.swvnav = a.fl[1][k] != 0;
  L.ap_alt = a.tg[2][k];
  L.iactwp = a.iactwp[k];
  fms::fms_recover(L, a.rows + (size_t)a.rt_off[k] * fms::kRouteCols, nwp, count);
  a.st[0][k] = L.wlat, a.st[1][k] = L.wlon, a.st[2][k] = L.nextaltco, a.st[3][k] = L.xtoalt;
  a.st[4][k] = L.spd, a.st[5][k] = L.vs, a.st[6][k] = L.turndist, a.st[7][k] = L.flyby;
  a.st[9][k] = L.dist2vs, a.st[12][k] = L.selspd;
  a.fl[0][k] = L.swlnav ? 1 : 0;
  a.tg[2][k] = L.ap_alt;
  a.iactwp[k] = L.iactwp;
}

// The standalone call: aircraft [0, n), count[k] applications each.  A wave
// without a non-zero count leaves after loading its counts.
__global__ __launch_bounds__(64) void k_fms_recover(int n, FmsArrays a, const int *__restrict__ count) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int cnt = count[k];
  if (cnt <= 0) return;
  recover_lane(a, k, cnt);
}

// The resident step's launch after k_bk_write of a CD step (resume_nav), on rows
// [rb, re) of the PRE-step state, before K4' forms pilot.alt from ap.alt.
// count: k_bk_write's pairs dropped per row in this call (home order).  Behind
// the abort test of the bookkeeping kernels it changes nothing.
__global__ __launch_bounds__(64) void k_sim_recover(int rb, int re, FmsArrays a, const int *__restrict__ count,
                                                    const unsigned long long *__restrict__ gate,
                                                    const unsigned *__restrict__ sticky) {
  if (bk_aborted(gate, sticky)) return;
  const int k = rb + blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= re) return;
  const int cnt = count[k];
  if (cnt <= 0) return;
  recover_lane(a, k, cnt);
}

int fms_sim_recover(Ctx *c) {
  const int64_t rb = c->sim_rb, re = c->sim_re;
  if (re <= rb) return 0;
  hipLaunchKernelGGL(k_sim_recover, dim3((unsigned)((re - rb + 63) / 64)), dim3(64), 0, c->stream, (int)rb, (int)re,
                     fms_sim_arrays(c), (const int *)c->s_dropcnt.p, (const unsigned long long *)c->sim_ctl.p,
                     (const unsigned *)((const char *)c->sim_ctl.p + kSimCtlSticky));
  BSA_HIP(c, hipGetLastError());
  return 0;
}

// Every index the kernel uses unguarded, checked on the host: each aircraft's
// rows inside the table, its active waypoint inside its route, and no LNAV
// without a route (only an aircraft with LNAV on ever reads a row).
int fms_check_routes(Ctx *c, const char *who, int64_t n, int64_t nrows, const int32_t *rt_off, const int32_t *rt_n,
                     const int32_t *iactwp, const uint8_t *swlnav) {
  for (int64_t k = 0; k < n; ++k) {
    const int64_t off = rt_off[k], m = rt_n[k];
    if (off < 0 || m < 0 || off + m > nrows)
      return fail(c, "%s: aircraft %lld: route rows [%lld, %lld) outside the table's %lld", who, (long long)k,
                  (long long)off, (long long)(off + m), (long long)nrows);
    if (m == 0) {
      if (swlnav[k]) return fail(c, "%s: aircraft %lld: LNAV on without a route", who, (long long)k);
      if (iactwp[k] != -1 && iactwp[k] != 0)
        return fail(c, "%s: aircraft %lld: active waypoint %d without a route (-1 or 0)", who, (long long)k, iactwp[k]);
    } else if (iactwp[k] < 0 || iactwp[k] >= m) {
      return fail(c, "%s: aircraft %lld: active waypoint %d outside [0, %lld)", who, (long long)k, iactwp[k],
                  (long long)m);
    }
  }
  return 0;
}

void fms_off(Ctx *c) {
  c->sim_fms = c->sim_recovery = false;
  c->clk.fms_simt = 0.0, c->clk.fms_t0 = -999.0, c->clk.fms_ticks = 0;
  geovec_off(c);  // selspd / selvs live in the FMS arrays
}

// bsa_sim_create_with's hook (bsa_internal.h).  The route table only grows: the new aircraft's rows go behind the
// ones it holds, deleted aircraft's among them
int fms_created(Ctx *c, int64_t n, int64_t m, const bsa_sim_create_extra &x) {
  if (!c->sim_fms) return 0;
  const size_t N = (size_t)(n + m);
  const int64_t base = c->fms_nrows;
  if (!ensure_keep(c, c->s_fmsrows, (size_t)(base + x.nrows) * 64 + 64, "route table") ||
      !ensure(c, c->s_fmsur, kFmsUndoReals * N * 8, "FMS undo set") || !ensure(c, c->s_fmsuf, 2 * N, "FMS undo flags") ||
      !ensure(c, c->s_fmsui, N * 4, "FMS undo waypoints"))
    return -1;
  if (x.nrows)
    BSA_HIP(c, hipMemcpyAsync((char *)c->s_fmsrows.p + (size_t)base * 64, x.route_rows, (size_t)x.nrows * 64,
                              hipMemcpyHostToDevice, c->stream));
  const FmsFields ff = fms_fields(*x.st);
  for (int q = 0; q < kFmsReals; ++q)
    BSA_HIP(c, hipMemcpyAsync((double *)c->s_fmsr.p + q * N + n, ff.reals[q], (size_t)m * 8, hipMemcpyHostToDevice, c->stream));
  for (int q = 0; q < kFmsFlags; ++q)
    BSA_HIP(c, hipMemcpyAsync((uint8_t *)c->s_fmsf.p + q * N + n, ff.flags[q], (size_t)m, hipMemcpyHostToDevice, c->stream));
  std::vector<int32_t> off(x.rt_off, x.rt_off + m);
  for (int32_t &o : off) o += (int32_t)base;
  const int32_t *ints[kFmsInts] = {x.iactwp, off.data(), x.rt_n};
  for (int q = 0; q < kFmsInts; ++q)
    BSA_HIP(c, hipMemcpyAsync((int32_t *)c->s_fmsi.p + q * N + n, ints[q], (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));  // (off goes out of scope)
  c->fms_nrows = base + x.nrows;
  return 0;
}

}  // namespace bsa

using bsa::Ctx;

extern "C" int bsa_fms_update(bsa_ctx *cc, int64_t n, int64_t nrows, const double *route_rows, const int32_t *rt_off,
                              const int32_t *rt_n, int32_t *iactwp, const double *lat, const double *lon,
                              const double *alt, const double *tas, const double *gs, const double *trk,
                              const double *ax, const double *bank, const bsa_fms_state *st, double *ap_trk,
                              double *ap_tas, double *ap_alt, double *ap_vs, double *selalt) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (n < 0 || n > 0x7fffffff) return bsa::fail(c, "bsa_fms_update: bad n");
  if (nrows < 0 || nrows > 0x7fffffff / bsa::fms::kRouteCols) return bsa::fail(c, "bsa_fms_update: bad route row count");
  if (!st) return bsa::fail(c, "bsa_fms_update: NULL state");
  const double *tr[8] = {lat, lon, alt, tas, gs, trk, ax, bank};
  const bsa::FmsFields ff = bsa::fms_fields(*st);
  double *const *reals = ff.reals;
  uint8_t *const *flags = ff.flags;
  double *tg[5] = {ap_trk, ap_tas, ap_alt, ap_vs, selalt};
  for (auto q : tr)
    if (!q) return bsa::fail(c, "bsa_fms_update: NULL array");
  for (auto q : ff.reals)
    if (!q) return bsa::fail(c, "bsa_fms_update: NULL array");
  for (auto q : ff.flags)
    if (!q) return bsa::fail(c, "bsa_fms_update: NULL array");
  for (auto q : tg)
    if (!q) return bsa::fail(c, "bsa_fms_update: NULL array");
  if (!rt_off || !rt_n || !iactwp || (nrows > 0 && !route_rows)) return bsa::fail(c, "bsa_fms_update: NULL array");
  if (bsa::fms_check_routes(c, "bsa_fms_update", n, nrows, rt_off, rt_n, iactwp, st->swlnav)) return -1;
  if (n == 0) return 0;
  BSA_HIP(c, hipSetDevice(c->device));
  // one device block: 8 + 15 + 5 fp64 arrays, 3 int32, 4 uint8, the route table
  const size_t N8 = ((size_t)n * 8 + 255) / 256 * 256, N4 = ((size_t)n * 4 + 255) / 256 * 256,
               N1 = ((size_t)n + 255) / 256 * 256;
  const size_t rb = (size_t)nrows * bsa::fms::kRouteCols * 8;
  constexpr int kD = 8 + bsa::kFmsReals + 5;
  bsa::DevBuf buf;
  struct Rel {
    bsa::DevBuf *b;
    ~Rel() { bsa::release(*b); }
  } rel{&buf};
  if (!bsa::ensure(c, buf, kD * N8 + 3 * N4 + 4 * N1 + rb + 256, "FMS staging")) return -1;
  char *base = (char *)buf.p;
  bsa::FmsArrays a;
  double *d8[kD];
  for (int q = 0; q < kD; ++q) d8[q] = (double *)(base + (size_t)q * N8);
  int *d4[3];
  for (int q = 0; q < 3; ++q) d4[q] = (int *)(base + kD * N8 + (size_t)q * N4);
  uint8_t *d1[4];
  for (int q = 0; q < 4; ++q) d1[q] = (uint8_t *)(base + kD * N8 + 3 * N4 + (size_t)q * N1);
  double *drows = (double *)(base + kD * N8 + 3 * N4 + 4 * N1);
  for (int q = 0; q < 8; ++q) {
    BSA_HIP(c, hipMemcpyAsync(d8[q], tr[q], (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    a.tr[q] = d8[q];
  }
  for (int q = 0; q < bsa::kFmsReals; ++q) {
    BSA_HIP(c, hipMemcpyAsync(d8[8 + q], reals[q], (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    a.st[q] = d8[8 + q];
  }
  for (int q = 0; q < 5; ++q) {
    BSA_HIP(c, hipMemcpyAsync(d8[8 + bsa::kFmsReals + q], tg[q], (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    a.tg[q] = d8[8 + bsa::kFmsReals + q];
  }
  const int32_t *h4[3] = {iactwp, rt_off, rt_n};
  for (int q = 0; q < 3; ++q)
    BSA_HIP(c, hipMemcpyAsync(d4[q], h4[q], (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  for (int q = 0; q < 4; ++q) {
    BSA_HIP(c, hipMemcpyAsync(d1[q], flags[q], (size_t)n, hipMemcpyHostToDevice, c->stream));
    a.fl[q] = d1[q];
  }
  if (rb) BSA_HIP(c, hipMemcpyAsync(drows, route_rows, rb, hipMemcpyHostToDevice, c->stream));
  a.iactwp = d4[0];
  a.rt_off = d4[1];
  a.rt_n = d4[2];
  a.rows = drows;
  hipLaunchKernelGGL(bsa::k_fms_update, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, (int)n, a);
  BSA_HIP(c, hipGetLastError());
  for (int q = 0; q < bsa::kFmsMutable; ++q)   // selvs, apvsdef are inputs only
    BSA_HIP(c, hipMemcpyAsync(reals[q], d8[8 + q], (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  for (int q = 0; q < 5; ++q)
    BSA_HIP(c, hipMemcpyAsync(tg[q], d8[8 + bsa::kFmsReals + q], (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  for (int q = 0; q < 2; ++q) BSA_HIP(c, hipMemcpyAsync(flags[q], d1[q], (size_t)n, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipMemcpyAsync(iactwp, d4[0], (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

extern "C" int bsa_fms_recover(bsa_ctx *cc, int64_t n, int64_t nrows, const double *route_rows, const int32_t *rt_off,
                               const int32_t *rt_n, int32_t *iactwp, const double *lat, const double *lon,
                               const double *alt, const double *tas, const double *gs, const double *trk,
                               const double *bank, const bsa_fms_state *st, double *ap_alt, const int32_t *count) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (n < 0 || n > 0x7fffffff) return bsa::fail(c, "bsa_fms_recover: bad n");
  if (nrows < 0 || nrows > 0x7fffffff / bsa::fms::kRouteCols) return bsa::fail(c, "bsa_fms_recover: bad route row count");
  if (!st) return bsa::fail(c, "bsa_fms_recover: NULL state");
  const double *tr[7] = {lat, lon, alt, tas, gs, trk, bank};
  const bsa::FmsFields ff = bsa::fms_fields(*st);
  for (auto q : tr)
    if (!q) return bsa::fail(c, "bsa_fms_recover: NULL array");
  for (auto q : ff.reals)
    if (!q) return bsa::fail(c, "bsa_fms_recover: NULL array");
  for (auto q : ff.flags)
    if (!q) return bsa::fail(c, "bsa_fms_recover: NULL array");
  if (!rt_off || !rt_n || !iactwp || !ap_alt || !count || (nrows > 0 && !route_rows))
    return bsa::fail(c, "bsa_fms_recover: NULL array");
  if (bsa::fms_check_routes(c, "bsa_fms_recover", n, nrows, rt_off, rt_n, iactwp, st->swlnav)) return -1;
  for (int64_t k = 0; k < n; ++k)
    if (count[k] < 0) return bsa::fail(c, "bsa_fms_recover: aircraft %lld: negative count %d", (long long)k, count[k]);
  if (n == 0) return 0;
  BSA_HIP(c, hipSetDevice(c->device));
  // one device block: 7 + 15 + 1 fp64 arrays, 4 int32, 4 uint8, the route table
  const size_t N8 = ((size_t)n * 8 + 255) / 256 * 256, N4 = ((size_t)n * 4 + 255) / 256 * 256,
               N1 = ((size_t)n + 255) / 256 * 256;
  const size_t rb = (size_t)nrows * bsa::fms::kRouteCols * 8;
  constexpr int kD = 7 + bsa::kFmsReals + 1;
  bsa::DevBuf buf;
  struct Rel {
    bsa::DevBuf *b;
    ~Rel() { bsa::release(*b); }
  } rel{&buf};
  if (!bsa::ensure(c, buf, kD * N8 + 4 * N4 + 4 * N1 + rb + 256, "FMS recovery staging")) return -1;
  char *base = (char *)buf.p;
  bsa::FmsArrays a{};
  double *d8[kD];
  for (int q = 0; q < kD; ++q) d8[q] = (double *)(base + (size_t)q * N8);
  int *d4[4];
  for (int q = 0; q < 4; ++q) d4[q] = (int *)(base + kD * N8 + (size_t)q * N4);
  uint8_t *d1[4];
  for (int q = 0; q < 4; ++q) d1[q] = (uint8_t *)(base + kD * N8 + 4 * N4 + (size_t)q * N1);
  double *drows = (double *)(base + kD * N8 + 4 * N4 + 4 * N1);
  const int slot[7] = {0, 1, 2, 3, 4, 5, 7};   // FmsArrays::tr without traf.ax
  for (int q = 0; q < 7; ++q) {
    BSA_HIP(c, hipMemcpyAsync(d8[q], tr[q], (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    a.tr[slot[q]] = d8[q];
  }
  for (int q = 0; q < bsa::kFmsReals; ++q) {
    BSA_HIP(c, hipMemcpyAsync(d8[7 + q], ff.reals[q], (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    a.st[q] = d8[7 + q];
  }
  double *dapalt = d8[7 + bsa::kFmsReals];
  BSA_HIP(c, hipMemcpyAsync(dapalt, ap_alt, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
  a.tg[2] = dapalt;
  const int32_t *h4[4] = {iactwp, rt_off, rt_n, count};
  for (int q = 0; q < 4; ++q)
    BSA_HIP(c, hipMemcpyAsync(d4[q], h4[q], (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  for (int q = 0; q < 4; ++q) {
    BSA_HIP(c, hipMemcpyAsync(d1[q], ff.flags[q], (size_t)n, hipMemcpyHostToDevice, c->stream));
    a.fl[q] = d1[q];
  }
  if (rb) BSA_HIP(c, hipMemcpyAsync(drows, route_rows, rb, hipMemcpyHostToDevice, c->stream));
  a.iactwp = d4[0];
  a.rt_off = d4[1];
  a.rt_n = d4[2];
  a.rows = drows;
  hipLaunchKernelGGL(bsa::k_fms_recover, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, (int)n, a,
                     (const int *)d4[3]);
  BSA_HIP(c, hipGetLastError());
  for (int q = 0; q < bsa::kFmsMutable; ++q)
    BSA_HIP(c, hipMemcpyAsync(ff.reals[q], d8[7 + q], (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipMemcpyAsync(ap_alt, dapalt, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
  for (int q = 0; q < 2; ++q)
    BSA_HIP(c, hipMemcpyAsync(ff.flags[q], d1[q], (size_t)n, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipMemcpyAsync(iactwp, d4[0], (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

// ---- the resident step's guidance: set / read, waypoint recovery
extern "C" int bsa_sim_set_fms(bsa_ctx *cc, int64_t nrows, const double *route_rows, const int32_t *rt_off,
                               const int32_t *rt_n, const int32_t *iactwp, const bsa_fms_state *st, double simt,
                               double t0) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_fms before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  if (!route_rows) {
    bsa::fms_off(c);
    return 0;
  }
  if (nrows < 0 || nrows > 0x7fffffff / 8) return bsa::fail(c, "bsa_sim_set_fms: bad route row count");
  if (!rt_off || !rt_n || !iactwp || !st) return bsa::fail(c, "bsa_sim_set_fms: NULL array");
  const bsa::FmsFields ff = bsa::fms_fields(*st);
  for (auto q : ff.reals)
    if (!q) return bsa::fail(c, "bsa_sim_set_fms: NULL array");
  for (auto q : ff.flags)
    if (!q) return bsa::fail(c, "bsa_sim_set_fms: NULL array");
  if (!std::isfinite(simt) || std::isnan(t0)) return bsa::fail(c, "bsa_sim_set_fms: simt / t0 not finite");
  const int64_t n = c->n;
  if (bsa::fms_check_routes(c, "bsa_sim_set_fms", n, nrows, rt_off, rt_n, iactwp, st->swlnav)) return -1;
  c->sim_fms = false;
  const bool gv_on = c->sim_gv;  // a new FMS state keeps the geovectors; a failed upload leaves both off
  c->sim_gv = false;
  const size_t N = (size_t)n;
  if (!bsa::ensure(c, c->s_fmsr, bsa::kFmsReals * N * 8, "FMS state") || !bsa::ensure(c, c->s_fmsf, bsa::kFmsFlags * N, "FMS flags") ||
      !bsa::ensure(c, c->s_fmsi, bsa::kFmsInts * N * 4, "route indices") ||
      !bsa::ensure(c, c->s_fmsrows, (size_t)nrows * 64 + 64, "route table") ||
      !bsa::ensure(c, c->s_fmsur, bsa::kFmsUndoReals * N * 8, "FMS undo set") || !bsa::ensure(c, c->s_fmsuf, 2 * N, "FMS undo flags") ||
      !bsa::ensure(c, c->s_fmsui, N * 4, "FMS undo waypoints"))
    return -1;
  bsa::HomeBatch up(c, true);
  const int32_t *ints[bsa::kFmsInts] = {iactwp, rt_off, rt_n};
  for (int q = 0; q < bsa::kFmsReals; ++q)
    if (up.add((double *)c->s_fmsr.p + q * N, ff.reals[q], nullptr, 8)) return -1;
  for (int q = 0; q < bsa::kFmsFlags; ++q)
    if (up.add((uint8_t *)c->s_fmsf.p + q * N, ff.flags[q], nullptr, 1)) return -1;
  for (int q = 0; q < bsa::kFmsInts; ++q)
    if (up.add((int32_t *)c->s_fmsi.p + q * N, ints[q], nullptr, 4)) return -1;
  if (up.run()) return -1;
  if (nrows) BSA_HIP(c, hipMemcpyAsync(c->s_fmsrows.p, route_rows, (size_t)nrows * 64, hipMemcpyHostToDevice, c->stream));
  BSA_HIP(c, hipStreamSynchronize(c->stream));
  c->clk.fms_simt = simt;
  c->clk.fms_t0 = t0;
  c->clk.fms_ticks = 0;
  c->fms_nrows = nrows;
  c->fms_ntypes = 0, c->rt_written = 0, c->rt_compactions = 0;  // a new table: every row type 0, no edit yet
  c->sim_fms = true;
  c->sim_gv = gv_on;
  return 0;
}

extern "C" int bsa_sim_set_recovery(bsa_ctx *cc, int on) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_set_recovery before bsa_sim_init");
  if (on && !c->sim_fms) return bsa::fail(c, "waypoint recovery needs the FMS guidance (bsa_sim_set_fms)");
  c->sim_recovery = on != 0;
  return 0;
}

extern "C" int bsa_sim_read_dropcount(bsa_ctx *cc, int32_t *count) {
  Ctx *c = (Ctx *)cc;
  if (!c || !count) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_read_dropcount before bsa_sim_init");
  BSA_HIP(c, hipSetDevice(c->device));
  bsa::HomeBatch down(c, false, c->sim_rb, c->sim_re);
  if (down.add(c->s_dropcnt.p, nullptr, count, 4)) return -1;
  return down.run();
}

extern "C" int bsa_sim_read_fms(bsa_ctx *cc, const bsa_fms_state *st, int32_t *iactwp, double *ap_trk, double *ap_tas,
                                double *ap_alt, double *ap_vs, double *selalt, double *simt, double *t0,
                                int64_t *ticks) {
  Ctx *c = (Ctx *)cc;
  if (!c) return -1;
  if (!c->sim_ready) return bsa::fail(c, "bsa_sim_read_fms before bsa_sim_init");
  if (!c->sim_fms) return bsa::fail(c, "no FMS state: bsa_sim_set_fms is off");
  BSA_HIP(c, hipSetDevice(c->device));
  const size_t N = (size_t)c->n;
  bsa::HomeBatch down(c, false, c->sim_rb, c->sim_re);
  if (st) {
    const bsa::FmsFields ff = bsa::fms_fields(*st);
    for (int q = 0; q < bsa::kFmsReals; ++q)
      if (ff.reals[q] && down.add((const double *)c->s_fmsr.p + q * N, nullptr, ff.reals[q], 8)) return -1;
    for (int q = 0; q < bsa::kFmsFlags; ++q)
      if (ff.flags[q] && down.add((const uint8_t *)c->s_fmsf.p + q * N, nullptr, ff.flags[q], 1)) return -1;
  }
  if (iactwp && down.add(c->s_fmsi.p, nullptr, iactwp, 4)) return -1;
  double *tg[5] = {ap_trk, ap_tas, ap_alt, ap_vs, selalt};
  const void *src[5] = {c->s_aptrk.p, c->s_aptas.p, c->s_apalt.p, c->s_apvs.p, c->s_selalt.p};
  for (int q = 0; q < 5; ++q)
    if (tg[q] && down.add(src[q], nullptr, tg[q], 8)) return -1;
  if (down.run()) return -1;
  if (simt) *simt = c->clk.fms_simt;
  if (t0) *t0 = c->clk.fms_t0;
  if (ticks) *ticks = c->clk.fms_ticks;
  return 0;
}
